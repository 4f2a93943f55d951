// pt_span.h -- the buffer checks of pt_shim.hip's entry points: plain host code, in a header of its own so that a stand-alone program
// can run it under the sanitizers (tests/span_check.cpp).  The includer declares, before this header,
//   struct pt_buffer_s with the members `void* dptr` and `size_t bytes`, and
//   int fail(int code, const char* fmt, ...), which records the message and returns the code (PT_ERR_* of include/pt_shim.h).
#pragma once

#include <initializer_list>
#include <stddef.h>
#include <stdint.h>

static bool ranges_overlap(const pt_buffer_s* a, size_t abytes, const pt_buffer_s* b, size_t bbytes)
{
    const uintptr_t a0 = (uintptr_t)a->dptr, b0 = (uintptr_t)b->dptr;
    return abytes && bbytes && a0 < b0 + bbytes && b0 < a0 + abytes;
}

// The part of a buffer that a call reads or writes, and what the kernels ask of it.  buf may be NULL -- an optional buffer the caller
// left out --, which passes every check.  Entry points call the three checks group by group in a fixed order: that order decides
// which of several defects is reported
struct PtSpan {
    const pt_buffer_s* buf;
    size_t bytes;        // what the call uses, from the buffer's start
    size_t align;        // of the address, a power of two
    const char* name;    // "the framebuffer": for the messages
};
static int span_fits(const PtSpan& s)
{
    if (s.buf && s.bytes > s.buf->bytes) return fail(PT_ERR_RANGE, "%s holds %zu bytes, the call needs %zu", s.name, s.buf->bytes, s.bytes);
    return PT_OK;
}
static int span_aligned(const PtSpan& s)
{
    if (s.buf && ((uintptr_t)s.buf->dptr & (s.align - 1))) return fail(PT_ERR_INVALID, "%s must be %zu-byte aligned", s.name, s.align);
    return PT_OK;
}
// every span of `spans` apart from every other of them and from every span of `inputs` (which may overlap one another: they are only read)
static int spans_apart(std::initializer_list<PtSpan> spans, std::initializer_list<PtSpan> inputs = {})
{
    for (const PtSpan* a = spans.begin(); a != spans.end(); ++a) {
        for (const PtSpan* b = a + 1; b != spans.end(); ++b)
            if (a->buf && b->buf && ranges_overlap(a->buf, a->bytes, b->buf, b->bytes)) return fail(PT_ERR_INVALID, "%s and %s overlap", a->name, b->name);
        for (const PtSpan& b : inputs)
            if (a->buf && b.buf && ranges_overlap(a->buf, a->bytes, b.buf, b.bytes)) return fail(PT_ERR_INVALID, "%s and %s overlap", a->name, b.name);
    }
    return PT_OK;
}
