// span_check.cpp -- csrc/pt_span.h under the sanitizers, without a GPU and outside Python: a stand-alone program
// (tests/test_span_check_cpu.py builds it with -fsanitize=address,undefined and runs it).  The buffers are sub-ranges of one host
// allocation, as the argument-error tests wrap sub-ranges of one device allocation; the cases are the buffer defects of
// gpu_support.assert_lit_argument_errors (one defect per call) and of the lit tests' "too small before it overlaps" cases (two),
// checked in the order render_lit checks a group: fits, aligned, apart.  TEST INFRASTRUCTURE.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/pt_shim.h"

struct pt_buffer_s { void* dptr; size_t bytes; };
static char g_err[256];
static int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#include "../oclpathtracer_amd/csrc/pt_span.h"

static int failures = 0;
static void expect(int got, int want, const char* what, const char* names = nullptr)
{
    const bool named = !names || got == PT_OK || strstr(g_err, names);
    if (got != want || !named) {
        printf("FAILED %s: code %d, wanted %d (%s)\n", what, got, want, got == PT_OK ? "" : g_err);
        ++failures;
    }
}

// a lit call's first two groups as render_lit orders them: what every kind uses, then the MIS counts
static int lit_groups(const PtSpan& M, const PtSpan& L, const PtSpan& S, const PtSpan& F, const PtSpan& N)
{
    int rc;
    PtSpan W = S;   // all of the workspace lies apart from the rest
    if (S.buf) W.bytes = S.buf->bytes;
    if ((rc = span_fits(M)) || (rc = span_fits(L)) || (rc = span_fits(S)) || (rc = span_fits(F))) return rc;
    if ((rc = span_aligned(S)) || (rc = span_aligned(F)) || (L.bytes && (rc = span_aligned(L))) || (rc = spans_apart({ W, F, L }))) return rc;
    if ((rc = span_fits(N)) || (rc = span_aligned(N)) || (rc = spans_apart({ N, W, F, L }))) return rc;
    return PT_OK;
}

int main()
{
    const size_t W = 16, H = 8, npix = W * H, ntri = 36;
    char* big = static_cast<char*>(aligned_alloc(64, 1 << 16));
    if (!big) return 2;
    auto buf = [&](size_t off, size_t bytes) { return pt_buffer_s{ big + off, bytes }; };
    // materials | lights (2) | workspace (one frame) | framebuffer | counts, 256 bytes apart
    const pt_buffer_s mats = buf(0, 12 * 64), lights = buf(1024, 8), ws = buf(2048, 12 * npix), fb = buf(4096, 16 * npix), cn = buf(8192, 4 * ntri);
    const PtSpan M = { &mats, 12 * 64, 1, "the material buffer" }, L = { &lights, 8, 4, "the light list" },
                 S = { &ws, 12 * npix, 4, "the sample workspace" }, F = { &fb, 16 * npix, 16, "the framebuffer" },
                 N = { &cn, 4 * ntri, 4, "the light-count buffer" }, none = { nullptr, 1u << 20, 64, "an optional buffer left out" };
    expect(lit_groups(M, L, S, F, N), PT_OK, "a good call");
    expect(lit_groups(M, none, S, F, none), PT_OK, "no lights, no counts");
    expect(span_fits(none) | span_aligned(none) | spans_apart({ none, S }, { none }), PT_OK, "a NULL buffer passes every check");

    // one defect each (assert_lit_argument_errors)
    PtSpan x = M; x.bytes += 64;
    expect(lit_groups(x, L, S, F, N), PT_ERR_RANGE, "num_materials + 1", "the material buffer holds 768 bytes, the call needs 832");
    x = L; x.bytes = 12;
    expect(lit_groups(M, x, S, F, N), PT_ERR_RANGE, "num_lights = 3 of 2", "the light list");
    x = S; x.bytes = 12 * (W + 16) * H;
    expect(lit_groups(M, L, x, F, N), PT_ERR_RANGE, "width + 16", "the sample workspace");
    const pt_buffer_s small = buf(2048, 12 * npix - 4);
    x = S; x.buf = &small;
    expect(lit_groups(M, L, x, F, N), PT_ERR_RANGE, "a workspace a float short", "the sample workspace");
    const pt_buffer_s f8 = buf(4096 + 8, 16 * npix), f0 = buf(2048 + 12 * npix - 16, 16 * npix), l2 = buf(1024 + 2, 8);
    x = F; x.buf = &f8;
    expect(lit_groups(M, L, S, x, N), PT_ERR_INVALID, "a framebuffer 8 bytes off", "must be 16-byte aligned");
    x = F; x.buf = &f0;
    expect(lit_groups(M, L, S, x, N), PT_ERR_INVALID, "workspace and framebuffer overlap", "the sample workspace and the framebuffer overlap");
    x = L; x.buf = &l2;
    expect(lit_groups(M, x, S, F, N), PT_ERR_INVALID, "a light list 2 bytes off", "the light list must be 4-byte aligned");
    x = L; x.buf = &l2; x.bytes = 0;
    expect(lit_groups(M, x, S, F, N), PT_OK, "... which is not read with no lights");

    // two defects: the order of the checks decides
    const pt_buffer_s c_in_ws_small = buf(2048 + 64, 4 * ntri - 4), c_in_fb = buf(4096 + 4, 4 * ntri);
    x = N; x.buf = &c_in_ws_small;
    expect(lit_groups(M, L, S, F, x), PT_ERR_RANGE, "counts too small AND inside the workspace: too small first", "the light-count buffer holds");
    x = N; x.buf = &c_in_fb;
    expect(lit_groups(M, L, S, F, x), PT_ERR_INVALID, "counts inside the framebuffer", "the light-count buffer and the framebuffer overlap");
    PtSpan y = F; y.buf = &f8;
    x = S; x.buf = &small;
    expect(lit_groups(M, L, x, y, N), PT_ERR_RANGE, "workspace too small AND framebuffer misaligned: too small first", "the sample workspace");
    x = N; x.bytes += 4;   // group order: the first group's alignment defect comes before the counts' size
    expect(lit_groups(M, L, S, y, x), PT_ERR_INVALID, "framebuffer misaligned AND counts too small: the first group first", "the framebuffer must be");

    // inputs may overlap one another, an output may overlap none (pt_light_table)
    const pt_buffer_s tris = buf(16384, 36 * 64), mats_in_tris = buf(16384 + 64, 64), cdf = buf(32768, 64), q_in_tris = buf(16384 + 128, 4 * ntri);
    const PtSpan R = { &tris, 36 * 64, 1, "the triangle buffer" }, M2 = { &mats_in_tris, 64, 1, "the material buffer" },
                 Q = { &cdf, 64, 8, "the light table's cdf" }, T = { &q_in_tris, 4 * ntri, 4, "the light table's tri_q" }, T0 = { &q_in_tris, 0, 4, "the light table's tri_q" };
    expect(spans_apart({ Q }, { R, M2 }), PT_OK, "inputs overlapping one another");
    expect(spans_apart({ Q, T }, { R, M2 }), PT_ERR_INVALID, "an output over an input", "the light table's tri_q and the triangle buffer overlap");
    expect(spans_apart({ Q, T0 }, { R, M2 }), PT_OK, "... of which nothing is used");
    expect(spans_apart({ Q, Q }), PT_ERR_INVALID, "a buffer given twice");

    // the last byte of the address space: no wrap in the overlap test's sums for buffers that end below it
    const pt_buffer_s hi = { reinterpret_cast<void*>(~(uintptr_t)0 - 4095), 4095 }, lo = { reinterpret_cast<void*>((uintptr_t)4096), 4096 };
    const PtSpan HI = { &hi, 4095, 1, "a buffer at the top" }, LO = { &lo, 4096, 4096, "a buffer at the bottom" };
    expect(spans_apart({ HI, LO }), PT_OK, "top and bottom of the address space");
    expect(span_aligned(LO), PT_OK, "4096-byte alignment");

    free(big);
    printf("%s\n", failures ? "span_check: FAILED" : "span_check: ok");
    return failures ? 1 : 0;
}
