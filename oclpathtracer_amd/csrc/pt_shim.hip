// pt_shim.hip -- implementation of the C ABI in include/pt_shim.h on the HIP runtime.
//
// Replaces, for the path-tracing hot path, what the reference does through
// Adl/CL/AdlCL.{inl,cpp} + Adl/CL/AdlKernelUtilsCL.{inl,cpp} + Adl/AdlKernel.cpp
// (OpenCL context/queue, cl_mem buffers, map/unmap, source->binary kernel cache,
// clSetKernelArg + clEnqueueNDRangeKernel).  There is no CPU path in this file.
#include "../../include/pt_shim.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "pt_denoise.h"
#include "pt_reproject.h"
#include "pt_kernels.h"
#include "pt_secmask.h"

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(PT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

extern "C" const char* pt_last_error(void) { return g_err; }
extern "C" int pt_abi_version(void) { return PT_SHIM_ABI_VERSION; }

// ------------------------------------------------------------------------------------------
// objects
// ------------------------------------------------------------------------------------------
enum { KERNEL_GENERATE_COLORS = 0, KERNEL_FILL = 1, KERNEL_MATH = 2, KERNEL_FOLD_CHECK = 3, KERNEL_SHADE_CHECK = 4, KERNEL_PAIR_CHECK = 5, KERNEL_SEARCH_CHECK = 6, KERNEL_COUNT = 7 };

struct pt_kernel_s {
    int id;
    const char* file;
    const char* func;
};

struct pt_buffer_s {
    pt_device_s* dev;
    void* dptr;
    size_t bytes;
    bool owned;
    uint64_t version;   // bumped by every API call that may change the contents
    void* staging;      // pinned host range of the last map (kept until the buffer dies)
    size_t staging_bytes;
    bool mapped;
    size_t mapped_bytes;  // size of the range handed out by the last pt_buffer_map (what unmap copies back)
    bool exposed;       // the raw device pointer has been handed out (pt_buffer_device_ptr): the caller may
                        // read or write the memory behind the shim's back, like wrapped memory
};

struct pt_event_s {
    pt_device_s* dev;
    hipEvent_t start, stop;
    bool recorded;
};

struct PendingFrames {  // deferred GenerateColors launches (PT_OPT_BATCH_FRAMES)
    bool active;
    pt_buffer_s *tris, *mats, *fb;
    int width, height, z_begin, z_count;
    uint32_t pixel_count;
};

// a device allocation the handle holds for itself, with its size (ws_malloc, ws_free): what pt_device_workspace_memory adds up
template <class T> struct PtWs {
    T* p;
    size_t bytes;
    operator T*() const { return p; }
};

// the pass-1 filter of one triangle table (pt_quad3_pass1): the brute-force scene's or the LBVH's table of big triangles
struct PtFilterTable {
    bool pairs;                 // every (2k, 2k+1) is a quad (a,b,c),(c,d,a), det-bounded: mode 3 if the radius allows
    int quads;                  // 0: independent triangles; 3: pairs, finite radius, margins and the packed table prepared
    float anchor[3]; bool anchor_valid;   // the eye the margins and the packed table were made about (ensure_anchor), since the table was last prepared
    PtWs<float> p1tab;          // the packed table
    float delta1, ray_radius, p1_lo, p1_hi;   // the filter's bounds: quad modes 2, 3 (pt_quad2_pass1, pt_quad3_pass1)
};

struct pt_device_s {
    int idx;
    hipDeviceProp_t prop;
    hipStream_t own_stream, stream;
    bool external;           // `stream` is the caller's (pt_device_set_stream)
    uint64_t used, peak;
    int live_buffers;
    uint64_t workspace;      // device bytes held by this handle for itself (every PtWs below)
    int64_t opt_batch, opt_chunk, opt_profile, opt_quads, opt_accel, opt_tally, opt_pmask, opt_bvh_stack, opt_lanes, opt_carry, opt_smask, opt_denoise, opt_reproject, opt_denoise_spatial;
    pt_kernel_s kernels[KERNEL_COUNT];
    PendingFrames pending;
    // ---- the prepared scene, its filter tables and its LBVH (ensure_prep, ensure_bvh, ensure_anchor, prepare_search)
    PtWs<PtPrepTriangle> prep;
    size_t prep_capacity;  // triangles
    const pt_buffer_s* prep_src;
    uint64_t prep_version;
    int prep_ntri;
    uint64_t prep_hash;         // checksum of the raw records the prepared scene was made from (pt_prep_kernel)
    bool prep_hash_valid;
    uint64_t scene_gen;         // bumped whenever the prepared scene's CONTENTS changed
    bool prep_det_bounded;      // scene extent allows the short exact reciprocal
    bool prep_finite;           // every vertex coordinate of the prepared scene is finite ...
    float prep_lo[3], prep_hi[3];  // ... and these are their per-axis extremes: the radius about any eye (anchor_radius)
    PtWs<unsigned int> det_bound_dev;  // PT_PREP_WORDS device words written by the prep kernel
    int blocks_per_cu;          // the table trace kernels' resident workgroups: follows the LDS footprint of the last scene that had triangles
    PtFilterTable scene_filter;    // the prepared scene's (p1tab sized with prep)
    PtFilterTable big_filter;      // the LBVH's table of big triangles (p1tab: ws_big_p1tab, the big triangles' raw records behind it)
    PtWs<PtBvh8Node> bvh;        // LBVH of the prepared scene (built on demand: ensure_bvh): its 64-byte records, sized with prep
    PtBvhGrid bvh_grid;         // the grid of its nodes' origins
    size_t bvh_records;         // records in use (nodes + leaves)
    PtWs<PtPrepTriangle> bigtab;   // the triangles kept out of the hierarchy (PT_BVH_BIG_MAX records + indices + count)
    PtWs<int> bigidx;
    int nbig;
    bool bvh_valid;
    uint64_t bvh_builds;        // LBVH builds so far (PT_OPT_BVH_BUILD_COUNT)
    int bvh_blocks_per_cu;
    int query_bvh_blocks_per_cu;   // the persistent grid of the LBVH query and ambient-occlusion kernels (pt_bvh_drive)
    int lit_bvh_blocks_per_cu[PT_LIT_KINDS];   // ... and of the lit renders' LBVH kernels, each kind its own (ptk_lit_kind: the second half the rays forms')
    unsigned int* trav_host; // the LBVH's sticky "search cut short" words: host memory the kernels store to (PT_ERR_TRAVERSAL)
    unsigned int* trav_dev;  // ... as the device addresses it
    // ---- fused-render workspace: the STREAMING renderer (render_part, plan_chunks, the ring).  A render walks its frames in chunks of
    // S frames (as many as a ring slot holds) through a ring of two radiance slots; chunk number seq (a running number over all renders of the handle) uses slot
    // seq % 2.  All launches of ONE render go to one lane, in order:
    //     T(0)  T(1) F(0)  T(2) F(1)  ...  T(n-1) F(n-2)  D  F(n-1)
    // T(c) = trace launch of chunk c, CHECKPOINTED (PtTraceParams::carry): it ends the moment its queue has handed out the last
    // batch, every wave saving the paths it still holds, and T(c+1) resumes them beside its own samples -- a launch has no tail
    // of waves running out of paths, so chunks as short as a 192 MiB slot forces cost 5 % over one long launch (the waves stop over ~100 us, and a fold follows: DESIGN.md S6).  F(c), the
    // fold of chunk c into the framebuffer, therefore follows T(c+1), which finishes chunk c's last paths; D is a launch with an
    // empty queue that finishes the last chunk's.  (The LBVH kernel's checkpoint is one SEARCH deep: a stopping launch starts no new
    // search, the lanes still searching finish theirs and are shaded, and the paths between two searches go to the next launch.
    // With PT_OPT_CHECKPOINT 0 every launch runs its paths out and the CHUNKS alternate lanes: T(0) F(0) T(1) F(1) ...)
    // Consecutive renders ALTERNATE between the two lanes: render k+1's T(0) needs the slot that F(n-2) of render k released, not
    // the one F(n-1) is still to read, so it fills the machine while D of render k runs dry.  The folds of all chunks of all renders
    // form ONE chain (events): every pixel folds its frames in ascending order (GenerateColors.cl:314-321).
    PtWs<float> ring;        // PT_RING_SLOTS x ring_slot_bytes: 12 bytes per (frame, pixel) of a chunk
    size_t ring_slot_bytes;
    hipStream_t lane[2];
    hipEvent_t ev_fork;      // recorded on `stream`: what the lanes must wait for before a render's first launches
    hipEvent_t ev_fold[2];   // recorded on lane L behind its latest fold
    hipEvent_t ev_slot[2];   // recorded behind the latest fold that read ring slot s: the slot may be written again
    hipEvent_t ev_ext;       // pt_device_wait_stream
    bool fold_recorded[2], slot_recorded[2];
    int last_fold_lane;      // the lane of the newest fold (its event is behind every earlier launch of both lanes)
    bool lanes_busy;         // lane work is enqueued that `stream` has not been ordered behind
    bool main_dirty;         // work has been enqueued on `stream` that the lanes have not been ordered behind
    uint64_t chunk_seq, render_seq;
    PtWs<uint32_t> carry[2]; // per lane: the checkpoint regions of its renders' trace launches (PT_CARRY_HIT_STRIDE_DW dwords per wave)
    PtWs<uint2> pmask;       // primary-ray candidate masks of the local pixels (pt_primary_mask_kernel), for as many pixels as it holds
    struct { uint64_t scene_gen; int32_t g[7]; PtCamera cam; bool valid; } pmask_key;  // what the masks in hand were made for
    PtWs<uint2> smask;       // secondary-ray candidate masks of the prepared scene (pt_secmask.h: PT_SM_TABLE_BYTES of the largest scene so far)
    struct { uint64_t scene_gen; int32_t ntri; bool valid, declined; } smask_key;  // the scene the table in hand was made for, as pmask_key; declined: that scene has a triangle without a table
    PtWs<unsigned int> counters;  // PT_QUEUE_COUNTERS work-queue counters, PT_QUEUE_STRIDE words apart: zero between launches
    bool counters_dirty;     // a failed call may have left one non-zero
    // ---- per-kernel timing (pt_profile_*)
    bool prof_on;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_pairs[PT_PROF_KINDS];
    size_t prof_used[PT_PROF_KINDS];
};

#define PT_RING_SLOTS 2
#define PT_DEFAULT_SLOT_BYTES ((size_t)192 << 20)   // sixteen 1024 x 1024 frames of 12-byte radiance
#define PT_QUEUE_COUNTERS 64                        // (the last two are the lanes' draining launches')
#define PT_QUEUE_STRIDE PT_QUEUE_WORDS              // words per queue: sharded counters + stop word (pt_kernels.h)

static int prof_begin(pt_device_s* d, int kind, hipStream_t st, hipEvent_t* stop_out)
{
    *stop_out = nullptr;
    if (!d->prof_on) return PT_OK;
    auto& v = d->prof_pairs[kind];
    if (d->prof_used[kind] == v.size()) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        v.push_back({ a, b });
    }
    auto& pr = v[d->prof_used[kind]++];
    HIP_TRY(hipEventRecord(pr.first, st));
    *stop_out = pr.second;
    return PT_OK;
}

static int prof_end(hipStream_t st, hipEvent_t stop)
{
    if (stop) HIP_TRY(hipEventRecord(stop, st));
    return PT_OK;
}

#ifndef PT_DEFAULT_PRIMARY_MASKS
#define PT_DEFAULT_PRIMARY_MASKS 1  // PT_OPT_PRIMARY_MASKS of a new device handle (A/B builds set 0)
#endif

#ifndef PT_DEFAULT_SECONDARY_MASKS
#define PT_DEFAULT_SECONDARY_MASKS 1  // PT_OPT_SECONDARY_MASKS of a new device handle (A/B builds set 0)
#endif

static int g_init_count = 0;

// device memory the handle holds for itself (pt_device_workspace_memory): an allocation carries its size from ws_malloc to ws_free
template <class T> static hipError_t ws_malloc(pt_device_s* d, PtWs<T>& w, size_t bytes)
{
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&w.p), bytes);
    if (e == hipSuccess) { w.bytes = bytes; d->workspace += bytes; }
    else { w = {}; (void)hipGetLastError(); }
    return e;
}

template <class T> static void ws_free(pt_device_s* d, PtWs<T>& w)
{
    if (!w.p) return;
    hipFree(w.p);
    d->workspace -= w.bytes;
    w = {};
}

static const size_t WS_BIGTAB = PT_BVH_BIG_MAX * sizeof(PtPrepTriangle);
static const size_t WS_BIGIDX = (PT_BVH_BIG_MAX + 1) * sizeof(int) + sizeof(PtBvhGrid) + sizeof(unsigned);  // indices, count, the LBVH's grid, records in use
static const size_t WS_COUNTERS = (size_t)PT_QUEUE_COUNTERS * PT_QUEUE_STRIDE * sizeof(unsigned int);
static const size_t WS_DETBOUND = PT_PREP_WORDS * sizeof(unsigned int);
static size_t ws_big_p1tab() { return ptk_p1tab_floats(PT_BVH_BIG_MAX) * sizeof(float) + PT_BVH_BIG_MAX * sizeof(PtRawTriangle); }  // + the big triangles' raw records

static int use_device(pt_device_s* d)
{
    if (!d) return fail(PT_ERR_INVALID, "null device handle");
    HIP_TRY(hipSetDevice(d->idx));
    return PT_OK;
}

// ------------------------------------------------------------------------------------------
// library / device lifetime
// ------------------------------------------------------------------------------------------
extern "C" int pt_init(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(PT_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    if (n <= 0) return fail(PT_ERR_NO_DEVICE, "no HIP device visible");
    ++g_init_count;
    return PT_OK;
}

extern "C" void pt_quit(void)
{
    if (g_init_count > 0) --g_init_count;
}

extern "C" int pt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// everything a device handle owns (also the unwinding path of a pt_device_create that failed half-way)
static void destroy_device_objects(pt_device_s* d)
{
    ws_free(d, d->prep);
    ws_free(d, d->scene_filter.p1tab);
    ws_free(d, d->bvh);
    ws_free(d, d->ring);
    ws_free(d, d->pmask);
    ws_free(d, d->smask);
    ws_free(d, d->counters);
    ws_free(d, d->bigtab);
    ws_free(d, d->bigidx);
    ws_free(d, d->big_filter.p1tab);
    ws_free(d, d->det_bound_dev);
    if (d->trav_host) hipHostFree(d->trav_host);
    for (auto& v : d->prof_pairs)
        for (auto& pr : v) {
            hipEventDestroy(pr.first);
            hipEventDestroy(pr.second);
        }
    for (int k = 0; k < 2; ++k) {
        if (d->ev_fold[k]) hipEventDestroy(d->ev_fold[k]);
        if (d->ev_slot[k]) hipEventDestroy(d->ev_slot[k]);
        ws_free(d, d->carry[k]);
        if (d->lane[k]) hipStreamDestroy(d->lane[k]);
    }
    if (d->ev_fork) hipEventDestroy(d->ev_fork);
    if (d->ev_ext) hipEventDestroy(d->ev_ext);
    if (d->own_stream) hipStreamDestroy(d->own_stream);
    delete d;
}

extern "C" int pt_device_create(int device_idx, pt_device_t* out)
{
    if (!out) return fail(PT_ERR_INVALID, "out == NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(PT_ERR_NO_DEVICE, "no HIP device visible (%s)", hipGetErrorString(e));
    if (device_idx < 0 || device_idx >= n) return fail(PT_ERR_NO_DEVICE, "device index %d out of range [0,%d)", device_idx, n);
    pt_device_s* d = new (std::nothrow) pt_device_s();   // value-initialised: every field zero, the profile pairs empty
    if (!d) return fail(PT_ERR_OOM, "host allocation failed");
    d->idx = device_idx;
    if (hipSetDevice(device_idx) != hipSuccess || hipGetDeviceProperties(&d->prop, device_idx) != hipSuccess) {
        delete d;
        return fail(PT_ERR_HIP, "cannot open device %d", device_idx);
    }
    if (strncmp(d->prop.gcnArchName, "gfx950", 6) != 0) {
        char arch[64];
        snprintf(arch, sizeof arch, "%s", d->prop.gcnArchName);
        delete d;
        return fail(PT_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 (MI355X) code only", device_idx, arch);
    }
    if (hipStreamCreateWithFlags(&d->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete d;
        return fail(PT_ERR_HIP, "hipStreamCreate failed");
    }
    d->stream = d->own_stream;
    d->opt_batch = 1;
    d->opt_pmask = PT_DEFAULT_PRIMARY_MASKS;
    d->opt_smask = PT_DEFAULT_SECONDARY_MASKS;
    d->opt_denoise = PT_DENOISE_GATHER_AUTO;
    d->opt_denoise_spatial = PT_DENOISE_POOL_AUTO;
    d->opt_reproject = PT_REPROJECT_FORM_AUTO;
    d->opt_bvh_stack = 64;
    d->opt_lanes = 2;
    d->opt_carry = 1;
    d->kernels[KERNEL_GENERATE_COLORS] = { KERNEL_GENERATE_COLORS, "GenerateColors", "GenerateColors" };
    d->kernels[KERNEL_FILL] = { KERNEL_FILL, "PtShimTest", "FillKernel" };
    d->kernels[KERNEL_MATH] = { KERNEL_MATH, "PtShimTest", "MathKernel" };
    d->kernels[KERNEL_FOLD_CHECK] = { KERNEL_FOLD_CHECK, "PtShimTest", "FoldCheckKernel" };
    d->kernels[KERNEL_SHADE_CHECK] = { KERNEL_SHADE_CHECK, "PtShimTest", "ShadeCheckKernel" };
    d->kernels[KERNEL_PAIR_CHECK] = { KERNEL_PAIR_CHECK, "PtShimTest", "PairCheckKernel" };
    d->kernels[KERNEL_SEARCH_CHECK] = { KERNEL_SEARCH_CHECK, "PtShimTest", "SearchCheckKernel" };
    bool ok = ws_malloc(d, d->bigtab, WS_BIGTAB) == hipSuccess && ws_malloc(d, d->bigidx, WS_BIGIDX) == hipSuccess &&
              ws_malloc(d, d->counters, WS_COUNTERS) == hipSuccess && ws_malloc(d, d->big_filter.p1tab, ws_big_p1tab()) == hipSuccess &&
              ws_malloc(d, d->det_bound_dev, WS_DETBOUND) == hipSuccess;
    // the render lanes and their events (no timing: they only order streams)
    for (int k = 0; ok && k < 2; ++k)
        ok = hipStreamCreateWithFlags(&d->lane[k], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&d->ev_fold[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&d->ev_slot[k], hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&d->ev_ext, hipEventDisableTiming) == hipSuccess;
    // the sticky words of PT_ERR_TRAVERSAL: host memory the LBVH kernels store to, read here without waiting for anything
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&d->trav_host), 64, hipHostMallocMapped) == hipSuccess &&
         hipHostGetDevicePointer(reinterpret_cast<void**>(&d->trav_dev), d->trav_host, 0) == hipSuccess;
    if (ok) {
        d->trav_host[0] = d->trav_host[1] = 0u;
        ok = hipMemsetAsync(d->counters, 0, WS_COUNTERS, d->own_stream) == hipSuccess && hipStreamSynchronize(d->own_stream) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        destroy_device_objects(d);
        return fail(PT_ERR_OOM, "workspace allocation failed");
    }
    d->blocks_per_cu = ptk_trace_blocks_per_cu(36);
    d->bvh_blocks_per_cu = ptk_trace_bvh_blocks_per_cu();
    d->query_bvh_blocks_per_cu = ptk_query_bvh_blocks_per_cu();
    for (unsigned kind = 0; kind < PT_LIT_KINDS; ++kind)
        if (ptk_lit_valid(kind)) d->lit_bvh_blocks_per_cu[kind] = ptk_lit_bvh_blocks_per_cu(kind);
    *out = d;
    return PT_OK;
}

static int flush_pending(pt_device_s* d);

static int stream_wait(pt_device_s* d);

extern "C" int pt_device_destroy(pt_device_t d)
{
    int rc = use_device(d);
    if (rc) return rc;
    rc = flush_pending(d);
    (void)stream_wait(d);   // (best effort on teardown)
    if (d->live_buffers != 0)
        return fail(PT_ERR_INVALID, "%d buffer(s) of this device are still alive", d->live_buffers);
    destroy_device_objects(d);
    return rc;
}

extern "C" int pt_device_info(pt_device_t d, int kind, char out[128])
{
    if (!d || !out) return fail(PT_ERR_INVALID, "null argument");
    out[0] = 0;
    switch (kind) {
    case PT_INFO_NAME:
    case PT_INFO_BOARD:
        // some driver stacks report an empty marketing name; fall back to the ISA name
        if (d->prop.name[0]) snprintf(out, 128, "%s", d->prop.name);
        else snprintf(out, 128, "AMD Instinct (%.*s)", 96, d->prop.gcnArchName);
        break;
    case PT_INFO_VENDOR: snprintf(out, 128, "Advanced Micro Devices, Inc."); break;
    case PT_INFO_VERSION: {
        int rt = 0;
        hipRuntimeGetVersion(&rt);
        snprintf(out, 128, "HIP %d %.*s", rt, 96, d->prop.gcnArchName);
        break;
    }
    default: return fail(PT_ERR_INVALID, "unknown info kind %d", kind);
    }
    return PT_OK;
}

extern "C" uint64_t pt_device_max_alloc(pt_device_t d) { return d ? (uint64_t)d->prop.totalGlobalMem : 0; }
extern "C" uint64_t pt_device_mem_size(pt_device_t d) { return d ? (uint64_t)d->prop.totalGlobalMem : 0; }
extern "C" uint64_t pt_device_used_memory(pt_device_t d) { return d ? d->used : 0; }
extern "C" uint64_t pt_device_peak_memory(pt_device_t d) { return d ? d->peak : 0; }
extern "C" uint64_t pt_device_workspace_memory(pt_device_t d) { return d ? d->workspace : 0; }
extern "C" int pt_device_num_cus(pt_device_t d) { return d ? d->prop.multiProcessorCount : 0; }

// ---- stream discipline -------------------------------------------------------------------------------------------------
// The handle's stream carries every call but the fused renders, whose launches live on the two lanes (pt_device_s).  Two
// one-way hand-overs keep the whole in call order:
//   fork  (render_internal): the lanes wait for what is on `stream` -- only when something has been put there since the
//         last fork (main_dirty), or the stream is the caller's, who may have enqueued on it without telling us;
//   join  (lanes_join): `stream` waits for the newest fold -- only when a call needs the renders' results on `stream`, so
//         that back-to-back renders never meet a join and overlap on the device.
// THE RULE: whoever enqueues on the handle's stream orders it behind the lanes and marks it dirty, so that the next fork happens.
// Nobody keeps it by hand; there are two primitives, and every site calls one of them:
//   stream_enqueue: "I am about to enqueue on the handle's stream": join, main_dirty = true (enter_stream: the entry points' form,
//                   which submits the deferred frames first);
//   stream_wait:    "the host waits for everything this handle has enqueued": join, hipStreamSynchronize.  Nothing is enqueued, so
//                   main_dirty stays as it is: a pt_sync between two renders does not make the second one fork.
// A bare lanes_join is left only where a call needs the order and enqueues no work on `stream` (event records at most).

// a caller's stream handle: PT_STREAM_LEGACY (the value of HIP's hipStreamLegacy sentinel) is the legacy default stream, which every
// HIP entry point knows as the null stream (the sentinel itself is not accepted by every runtime version torch ships)
static hipStream_t as_stream(void* h) { return h == PT_STREAM_LEGACY ? nullptr : (hipStream_t)h; }

static int lanes_join(pt_device_s* d)
{
    if (!d->lanes_busy) return PT_OK;
    if (d->fold_recorded[d->last_fold_lane]) HIP_TRY(hipStreamWaitEvent(d->stream, d->ev_fold[d->last_fold_lane], 0));
    d->lanes_busy = false;
    return PT_OK;
}

static int stream_enqueue(pt_device_s* d)
{
    int rc = lanes_join(d);
    d->main_dirty = true;
    return rc;
}

static int stream_wait(pt_device_s* d)
{
    int rc = lanes_join(d);
    hipError_t e = hipStreamSynchronize(d->stream);   // (after a failed join too: teardown ignores both)
    if (rc || e == hipSuccess) return rc;
    return fail(PT_ERR_HIP, "hipStreamSynchronize(d->stream) failed: %s", hipGetErrorString(e));
}

// every entry point that enqueues on the handle's stream: deferred frames are submitted first
static int enter_stream(pt_device_s* d)
{
    int rc = flush_pending(d), rc2 = stream_enqueue(d);   // (also after a flush that failed: it may have enqueued)
    return rc ? rc : rc2;
}

// PT_ERR_TRAVERSAL, deferred (include/pt_shim.h): read -- and clear -- the words the LBVH kernels raise.  Called wherever the
// host observes the device; never waits for anything itself.
static int check_traversal(pt_device_s* d)
{
    if (!d->trav_host) return PT_OK;
    const unsigned st = __atomic_exchange_n(&d->trav_host[0], 0u, __ATOMIC_ACQ_REL);
    const unsigned bu = __atomic_exchange_n(&d->trav_host[1], 0u, __ATOMIC_ACQ_REL);
    if (!st && !bu) return PT_OK;
    return fail(PT_ERR_TRAVERSAL, "LBVH search cut short (%s%s%s): the framebuffers of the renders since the last check are not valid",
                st ? "stack capacity" : "", st && bu ? ", " : "", bu ? "step budget" : "");
}

extern "C" int pt_device_set_stream(pt_device_t d, void* hip_stream)
{
    int rc = use_device(d);
    if (rc) return rc;
    if ((rc = enter_stream(d)) || (rc = stream_wait(d))) return rc;   // keep the one-queue ordering across the switch
    // NULL restores the handle's own (non-blocking) stream.  The legacy default stream -- what a
    // caller's "stream 0" means -- is named by PT_STREAM_LEGACY and used as HIP's null stream.
    d->stream = hip_stream ? as_stream(hip_stream) : d->own_stream;
    d->external = hip_stream != nullptr;
    return PT_OK;
}

extern "C" void* pt_device_get_stream(pt_device_t d) { return !d ? nullptr : d->external && !d->stream ? PT_STREAM_LEGACY : (void*)d->stream; }

extern "C" int pt_device_wait_stream(pt_device_t d, void* hip_stream)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!hip_stream) return fail(PT_ERR_INVALID, "hip_stream == NULL (the legacy default stream is PT_STREAM_LEGACY)");
    // (an event may be recorded again while a wait on its earlier record is pending: the wait keeps the record it saw)
    HIP_TRY(hipEventRecord(d->ev_ext, as_stream(hip_stream)));
    HIP_TRY(hipStreamWaitEvent(d->stream, d->ev_ext, 0));
    d->main_dirty = true;
    return PT_OK;
}

extern "C" int pt_device_wait_hip_event(pt_device_t d, void* hip_event)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!hip_event) return fail(PT_ERR_INVALID, "hip_event == NULL");
    HIP_TRY(hipStreamWaitEvent(d->stream, (hipEvent_t)hip_event, 0));
    d->main_dirty = true;
    return PT_OK;
}

extern "C" int pt_sync(pt_device_t d)
{
    int rc = use_device(d);
    if (rc) return rc;
    // Deferred frames (PT_OPT_BATCH_FRAMES) touch shim-owned, never-exposed buffers only
    // (launch_generate_colors), which can be observed through this ABI alone: every such
    // observation flushes.  Should a pending buffer have been exposed since (pt_buffer_device_ptr
    // flushes, so this is belt and braces), clFinish semantics are restored here.
    if (d->pending.active && (d->pending.tris->exposed || d->pending.mats->exposed || d->pending.fb->exposed) &&
        (rc = flush_pending(d)))
        return rc;
    if ((rc = stream_wait(d))) return rc;
    return check_traversal(d);
}

extern "C" int pt_flush(pt_device_t d)
{
    int rc = use_device(d);
    if (rc) return rc;
    return flush_pending(d);
}

static int free_ring(pt_device_s* d)
{
    int rc = stream_wait(d);   // nothing in flight may still write it
    if (rc) return rc;
    ws_free(d, d->ring);
    d->ring_slot_bytes = 0;
    return PT_OK;
}

static int alloc_ring(pt_device_s* d, size_t slot_bytes)
{
    slot_bytes = (slot_bytes + 255) & ~(size_t)255;
    hipError_t e = ws_malloc(d, d->ring, PT_RING_SLOTS * slot_bytes);
    if (e != hipSuccess) return fail(PT_ERR_OOM, "radiance staging ring (%d x %zu bytes) allocation failed: %s", PT_RING_SLOTS, slot_bytes, hipGetErrorString(e));
    d->ring_slot_bytes = slot_bytes;
    return PT_OK;
}

extern "C" int pt_device_reserve_staging(pt_device_t d, size_t bytes)
{
    int rc = use_device(d);
    if (rc) return rc;
    const size_t slot = bytes ? (bytes + PT_RING_SLOTS - 1) / PT_RING_SLOTS : PT_DEFAULT_SLOT_BYTES;
    if (slot < 12) return fail(PT_ERR_INVALID, "a staging slot holds at least one 12-byte sample");
    if ((rc = flush_pending(d))) return rc;
    if (d->ring && ((slot + 255) & ~(size_t)255) == d->ring_slot_bytes) return PT_OK;
    if (d->ring && (rc = free_ring(d))) return rc;
    return alloc_ring(d, slot);
}

extern "C" int pt_device_set_option(pt_device_t d, int option, int64_t value)
{
    int rc = use_device(d);
    if (rc) return rc;
    switch (option) {
    case PT_OPT_BATCH_FRAMES:
        rc = flush_pending(d);
        d->opt_batch = value ? 1 : 0;
        return rc;
    case PT_OPT_CHUNK_FRAMES:
        if (value < 0) return fail(PT_ERR_INVALID, "chunk frames must be >= 0");
        d->opt_chunk = value;
        return PT_OK;
    case PT_OPT_PROFILE_RETURN_TIME:
        d->opt_profile = value ? 1 : 0;
        return PT_OK;
    case PT_OPT_QUAD_FILTER:
        if (value < 0 || value > 4) return fail(PT_ERR_INVALID, "quad filter must be 0 (auto), 1..3 (independent triangles) or 4 (packed shared u)");
        d->opt_quads = value;
        return PT_OK;
    case PT_OPT_ACCEL:
        if (value < 0 || value > 2) return fail(PT_ERR_INVALID, "accel must be 0 (auto), 1 (brute force) or 2 (BVH)");
        d->opt_accel = value;
        return PT_OK;
    case PT_OPT_BVH_TALLY:
        d->opt_tally = value ? 1 : 0;
        return PT_OK;
    case PT_OPT_PRIMARY_MASKS:
        d->opt_pmask = value ? 1 : 0;
        return PT_OK;
    case PT_OPT_SECONDARY_MASKS:
        d->opt_smask = value ? 1 : 0;
        return PT_OK;
    case PT_OPT_DENOISE_TILE:
        if (value < 0 || value > 2) return fail(PT_ERR_INVALID, "the denoiser's gather must be 0 (auto), 1 (global loads) or 2 (LDS tile at steps 1 and 2)");
        d->opt_denoise = value;
        return PT_OK;
    case PT_OPT_REPROJECT_FORM:
        if (value < 0 || value > 2) return fail(PT_ERR_INVALID, "the reprojection's form must be 0 (auto), 1 (one kernel over the records) or 2 (a prepare pass first)");
        d->opt_reproject = value;
        return PT_OK;
    case PT_OPT_DENOISE_SPATIAL_FORM:
        if (value < 0 || value > 2) return fail(PT_ERR_INVALID, "the pool pass's form must be 0 (auto), 1 (global loads) or 2 (LDS tile)");
        d->opt_denoise_spatial = value;
        return PT_OK;
    case PT_OPT_BVH_STACK_LIMIT:
        if (value < 1 || value > 64) return fail(PT_ERR_INVALID, "the LBVH stack limit must be 1..64");
        d->opt_bvh_stack = value;
        return PT_OK;
    case PT_OPT_RENDER_LANES:
        if (value < 1 || value > 2) return fail(PT_ERR_INVALID, "render lanes must be 1 or 2");
        rc = enter_stream(d);   // the next render forks: both lanes start behind everything enqueued under the old setting
        d->opt_lanes = value;
        return rc;
    case PT_OPT_CHECKPOINT:
        d->opt_carry = value ? 1 : 0;
        return PT_OK;
    case PT_OPT_RESERVED_3:   // ABI version 1's kernel-variant switch: both of its values select the one variant left
        if (value != 0 && value != 1) return fail(PT_ERR_INVALID, "option 3 took 0 or 1");
        return PT_OK;
    default: return fail(PT_ERR_INVALID, "unknown option %d", option);
    }
}

extern "C" int64_t pt_device_get_option(pt_device_t d, int option)
{
    if (!d) return -1;
    switch (option) {
    case PT_OPT_BATCH_FRAMES: return d->opt_batch;
    case PT_OPT_CHUNK_FRAMES: return d->opt_chunk;
    case PT_OPT_PROFILE_RETURN_TIME: return d->opt_profile;
    case PT_OPT_QUAD_FILTER: return d->opt_quads;
    case PT_OPT_ACCEL: return d->opt_accel;
    case PT_OPT_BVH_TALLY: return d->opt_tally;
    case PT_OPT_PRIMARY_MASKS: return d->opt_pmask;
    case PT_OPT_SECONDARY_MASKS: return d->opt_smask;
    case PT_OPT_DENOISE_TILE: return d->opt_denoise;
    case PT_OPT_REPROJECT_FORM: return d->opt_reproject;
    case PT_OPT_DENOISE_SPATIAL_FORM: return d->opt_denoise_spatial;
    case PT_OPT_BVH_STACK_LIMIT: return d->opt_bvh_stack;
    case PT_OPT_RENDER_LANES: return d->opt_lanes;
    case PT_OPT_CHECKPOINT: return d->opt_carry;
    case PT_OPT_BVH_BUILD_COUNT: return (int64_t)d->bvh_builds;
    case PT_OPT_RESERVED_3: return 0;
    default: return -1;
    }
}

// ------------------------------------------------------------------------------------------
// buffers
// ------------------------------------------------------------------------------------------
extern "C" int pt_buffer_alloc(pt_device_t d, size_t bytes, pt_buffer_t* out)
{
    if (!out) return fail(PT_ERR_INVALID, "out == NULL");
    *out = nullptr;
    int rc = use_device(d);
    if (rc) return rc;
    pt_buffer_s* b = new (std::nothrow) pt_buffer_s();
    if (!b) return fail(PT_ERR_OOM, "host allocation failed");
    memset(static_cast<void*>(b), 0, sizeof *b);
    b->dev = d;
    b->bytes = bytes;
    b->owned = true;
    if (bytes) {
        hipError_t e = hipMalloc(&b->dptr, bytes);
        if (e != hipSuccess) {
            delete b;
            (void)hipGetLastError();  // clear the sticky error: later launches check hipGetLastError()
            return fail(PT_ERR_OOM, "hipMalloc(%zu) failed: %s (used %llu bytes)", bytes, hipGetErrorString(e),
                        (unsigned long long)d->used);
        }
    }
    d->used += bytes;
    d->peak = std::max(d->peak, d->used);
    d->live_buffers++;
    *out = b;
    return PT_OK;
}

extern "C" int pt_buffer_wrap(pt_device_t d, void* device_ptr, size_t bytes, pt_buffer_t* out)
{
    if (!out) return fail(PT_ERR_INVALID, "out == NULL");
    *out = nullptr;
    int rc = use_device(d);
    if (rc) return rc;
    if (!device_ptr && bytes) return fail(PT_ERR_INVALID, "null device pointer");
    pt_buffer_s* b = new (std::nothrow) pt_buffer_s();
    if (!b) return fail(PT_ERR_OOM, "host allocation failed");
    memset(static_cast<void*>(b), 0, sizeof *b);
    b->dev = d;
    b->dptr = device_ptr;
    b->bytes = bytes;
    b->owned = false;
    d->live_buffers++;
    *out = b;
    return PT_OK;
}

extern "C" int pt_buffer_free(pt_buffer_t b)
{
    if (!b) return fail(PT_ERR_INVALID, "null buffer handle");
    pt_device_s* d = b->dev;
    int rc = use_device(d);
    if (rc) return rc;
    if (d->pending.active && (d->pending.tris == b || d->pending.mats == b || d->pending.fb == b)) rc = flush_pending(d);
    (void)stream_wait(d);  // nothing in flight may still touch it (best effort)
    if (d->prep_src == b) d->prep_src = nullptr;
    if (b->staging) hipHostFree(b->staging);
    if (b->owned) {
        if (b->dptr) hipFree(b->dptr);
        d->used -= b->bytes;
    }
    d->live_buffers--;
    delete b;
    return rc;
}

extern "C" size_t pt_buffer_size(pt_buffer_t b) { return b ? b->bytes : 0; }
extern "C" void* pt_buffer_address(pt_buffer_t b) { return b ? b->dptr : nullptr; }

extern "C" void* pt_buffer_device_ptr(pt_buffer_t b)
{
    if (!b) return nullptr;
    // From here on the caller can observe (or change) the memory without going through this ABI:
    // submit what is deferred now and never defer launches on this buffer again.
    if (!b->exposed) {
        b->exposed = true;
        pt_device_s* d = b->dev;
        if (d->pending.active && (d->pending.tris == b || d->pending.mats == b || d->pending.fb == b) &&
            (use_device(d) || flush_pending(d)))
            return nullptr;
    }
    return b->dptr;
}

static int check_range(const pt_buffer_s* b, size_t off, size_t bytes, const char* what)
{
    if (!b) return fail(PT_ERR_INVALID, "null buffer handle (%s)", what);
    if (off > b->bytes || bytes > b->bytes - off)
        return fail(PT_ERR_RANGE, "%s: range [%zu, +%zu) outside buffer of %zu bytes", what, off, bytes, b->bytes);
    return PT_OK;
}

// the argument checks every entry point makes in the same words (null entries: optional buffers the caller left out)
static int check_same_device(const pt_device_s* d, std::initializer_list<const pt_buffer_s*> bufs)
{
    for (const pt_buffer_s* b : bufs)
        if (b && b->dev != d) return fail(PT_ERR_INVALID, "buffer belongs to another device");
    return PT_OK;
}
static int check_event(const pt_device_s* d, const pt_event_s* ev)
{
    return ev && ev->dev != d ? fail(PT_ERR_INVALID, "event belongs to another device") : PT_OK;
}
static int check_triangles(const pt_buffer_s* tris, int n)
{
    if ((size_t)n * sizeof(PtRawTriangle) > tris->bytes)
        return fail(PT_ERR_RANGE, "triangle buffer holds %zu bytes, %d triangles need %zu", tris->bytes, n, (size_t)n * sizeof(PtRawTriangle));
    return PT_OK;
}

#include "pt_span.h"   // PtSpan and ranges_overlap, span_fits, span_aligned, spans_apart: the buffer checks of the entry points

static int event_begin(pt_device_s* d, pt_event_s* ev)
{
    if (!ev) return PT_OK;
    if (ev->dev != d) return fail(PT_ERR_INVALID, "event belongs to another device");
    HIP_TRY(hipEventRecord(ev->start, d->stream));
    return PT_OK;
}

static int event_end(pt_device_s* d, pt_event_s* ev)
{
    if (!ev) return PT_OK;
    HIP_TRY(hipEventRecord(ev->stop, d->stream));
    ev->recorded = true;
    return PT_OK;
}

extern "C" int pt_buffer_write(pt_buffer_t dst, const void* host_src, size_t bytes, size_t dst_offset, pt_event_t ev)
{
    int rc = check_range(dst, dst_offset, bytes, "pt_buffer_write");
    if (rc) return rc;
    pt_device_s* d = dst->dev;
    if ((rc = use_device(d)) || (rc = enter_stream(d))) return rc;
    if (!host_src && bytes) return fail(PT_ERR_INVALID, "null host pointer");
    if ((rc = event_begin(d, ev))) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync((char*)dst->dptr + dst_offset, host_src, bytes, hipMemcpyHostToDevice, d->stream));
    dst->version++;
    return event_end(d, ev);
}

extern "C" int pt_buffer_read(pt_buffer_t src, void* host_dst, size_t bytes, size_t src_offset, pt_event_t ev)
{
    int rc = check_range(src, src_offset, bytes, "pt_buffer_read");
    if (rc) return rc;
    pt_device_s* d = src->dev;
    if ((rc = use_device(d)) || (rc = enter_stream(d))) return rc;
    if (!host_dst && bytes) return fail(PT_ERR_INVALID, "null host pointer");
    if ((rc = event_begin(d, ev))) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(host_dst, (const char*)src->dptr + src_offset, bytes, hipMemcpyDeviceToHost, d->stream));
    return event_end(d, ev);
}

extern "C" int pt_buffer_copy(pt_buffer_t dst, pt_buffer_t src, size_t bytes, size_t dst_offset, size_t src_offset,
                              pt_event_t ev)
{
    int rc = check_range(dst, dst_offset, bytes, "pt_buffer_copy(dst)");
    if (rc) return rc;
    if ((rc = check_range(src, src_offset, bytes, "pt_buffer_copy(src)"))) return rc;
    if (dst->dev != src->dev) return fail(PT_ERR_INVALID, "buffers belong to different devices");
    pt_device_s* d = dst->dev;
    if ((rc = use_device(d)) || (rc = enter_stream(d))) return rc;
    if ((rc = event_begin(d, ev))) return rc;
    if (bytes)
        HIP_TRY(hipMemcpyAsync((char*)dst->dptr + dst_offset, (const char*)src->dptr + src_offset, bytes,
                               hipMemcpyDeviceToDevice, d->stream));
    dst->version++;
    return event_end(d, ev);
}

extern "C" int pt_host_alloc(size_t bytes, void** out)
{
    if (!out) return fail(PT_ERR_INVALID, "null out pointer");
    *out = nullptr;
    if (g_init_count <= 0) return fail(PT_ERR_NO_DEVICE, "pt_init has not succeeded");
    hipError_t e = hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return fail(PT_ERR_OOM, "pinned host allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e)); }
    return PT_OK;
}

extern "C" int pt_host_free(void* host_ptr)
{
    if (!host_ptr) return PT_OK;
    HIP_TRY(hipHostFree(host_ptr));
    return PT_OK;
}

extern "C" void* pt_buffer_map(pt_buffer_t b, size_t bytes, int blocking)
{
    if (!b) { fail(PT_ERR_INVALID, "null buffer handle"); return nullptr; }
    pt_device_s* d = b->dev;
    if (use_device(d) || enter_stream(d)) return nullptr;
    if (bytes == (size_t)-1) bytes = b->bytes;
    if (check_range(b, 0, bytes, "pt_buffer_map")) return nullptr;
    if (b->mapped) { fail(PT_ERR_INVALID, "buffer is already mapped"); return nullptr; }
    size_t need = std::max<size_t>(bytes, 1);
    if (b->staging_bytes < need) {
        if (b->staging) {
            hipStreamSynchronize(d->stream);
            hipHostFree(b->staging);
            b->staging = nullptr;
            b->staging_bytes = 0;
        }
        hipError_t e = hipHostMalloc(&b->staging, need, hipHostMallocDefault);
        if (e != hipSuccess) { fail(PT_ERR_OOM, "hipHostMalloc(%zu) failed: %s", need, hipGetErrorString(e)); return nullptr; }
        b->staging_bytes = need;
    }
    if (bytes) {
        hipError_t e = hipMemcpyAsync(b->staging, b->dptr, bytes, hipMemcpyDeviceToHost, d->stream);
        if (e != hipSuccess) { fail(PT_ERR_HIP, "map copy failed: %s", hipGetErrorString(e)); return nullptr; }
    }
    if (blocking) {
        hipError_t e = hipStreamSynchronize(d->stream);
        if (e != hipSuccess) { fail(PT_ERR_HIP, "map sync failed: %s", hipGetErrorString(e)); return nullptr; }
        if (check_traversal(d)) return nullptr;   // (the contents would be those of a failed render)
    }
    b->mapped = true;
    b->mapped_bytes = bytes;
    return b->staging;
}

extern "C" int pt_buffer_unmap(pt_buffer_t b, void* host_ptr)
{
    if (!b) return fail(PT_ERR_INVALID, "null buffer handle");
    if (!b->mapped || host_ptr != b->staging) return fail(PT_ERR_INVALID, "pointer was not returned by pt_buffer_map of this buffer");
    pt_device_s* d = b->dev;
    int rc;
    if ((rc = use_device(d)) || (rc = enter_stream(d))) return rc;
    // exactly the range pt_buffer_map handed out: the staging allocation is kept at its largest size
    // ever, and whatever lies beyond this map's range is a stale snapshot
    size_t bytes = std::min(b->mapped_bytes, b->bytes);
    if (bytes) HIP_TRY(hipMemcpyAsync(b->dptr, b->staging, bytes, hipMemcpyHostToDevice, d->stream));
    b->mapped = false;
    b->version++;
    return PT_OK;
}

// ------------------------------------------------------------------------------------------
// events
// ------------------------------------------------------------------------------------------
extern "C" int pt_event_create(pt_device_t d, pt_event_t* out)
{
    if (!out) return fail(PT_ERR_INVALID, "out == NULL");
    *out = nullptr;
    int rc = use_device(d);
    if (rc) return rc;
    pt_event_s* e = new (std::nothrow) pt_event_s();
    if (!e) return fail(PT_ERR_OOM, "host allocation failed");
    e->dev = d;
    e->recorded = false;
    if (hipEventCreate(&e->start) != hipSuccess || hipEventCreate(&e->stop) != hipSuccess) {
        delete e;
        return fail(PT_ERR_HIP, "hipEventCreate failed");
    }
    *out = e;
    return PT_OK;
}

extern "C" int pt_event_destroy(pt_event_t e)
{
    if (!e) return fail(PT_ERR_INVALID, "null event handle");
    hipEventDestroy(e->start);
    hipEventDestroy(e->stop);
    delete e;
    return PT_OK;
}

extern "C" int pt_event_wait(pt_event_t e)
{
    if (!e) return fail(PT_ERR_INVALID, "null event handle");
    if (!e->recorded) return PT_OK;
    int rc = use_device(e->dev);
    if (rc) return rc;
    HIP_TRY(hipEventSynchronize(e->stop));
    return check_traversal(e->dev);
}

extern "C" int pt_event_wait_on(pt_event_t e, void* hip_stream)
{
    if (!e) return fail(PT_ERR_INVALID, "null event handle");
    if (!hip_stream) return fail(PT_ERR_INVALID, "hip_stream == NULL (the legacy default stream is PT_STREAM_LEGACY)");
    if (!e->recorded) return PT_OK;
    int rc = use_device(e->dev);
    if (rc) return rc;
    HIP_TRY(hipStreamWaitEvent(as_stream(hip_stream), e->stop, 0));
    return PT_OK;
}

extern "C" int pt_event_is_complete(pt_event_t e)
{
    if (!e) { fail(PT_ERR_INVALID, "null event handle"); return -1; }
    if (!e->recorded) return 1;
    if (use_device(e->dev)) return -1;
    hipError_t s = hipEventQuery(e->stop);
    if (s == hipSuccess) return 1;
    if (s == hipErrorNotReady) return 0;
    fail(PT_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(s));
    return -1;
}

extern "C" int pt_event_elapsed_ns(pt_event_t e, uint64_t* ns_out)
{
    if (!e || !ns_out) return fail(PT_ERR_INVALID, "null argument");
    if (!e->recorded) return fail(PT_ERR_INVALID, "event was never recorded");
    int rc = use_device(e->dev);
    if (rc) return rc;
    HIP_TRY(hipEventSynchronize(e->stop));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->start, e->stop));
    *ns_out = (uint64_t)((double)ms * 1.0e6);
    return check_traversal(e->dev);
}

// ------------------------------------------------------------------------------------------
// the fused renderer
// ------------------------------------------------------------------------------------------
extern "C" int pt_local_rows(int height, int stripe_rows, int n_ranks, int rank)
{
    if (height < 0 || stripe_rows < 1 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return -1;
    long long rows = 0;
    long long period = (long long)stripe_rows * n_ranks;
    long long full = height / period;
    rows = full * stripe_rows;
    long long rem = height - full * period;          // rows of the last, partial period
    long long start = (long long)rank * stripe_rows;  // this rank's stripe inside it
    if (rem > start) rows += std::min<long long>(stripe_rows, rem - start);
    return (int)rows;
}

// ---- the camera (GenerateColors.cl:263-276) -------------------------------------------------------------------------
// Derived once per render, here on the host, in binary32 with PTSPEC's cross / normalize (explicit fmaf, no contraction: this
// translation unit is compiled with -ffp-contract=off) in the reference's order -- the same bits as the reference evaluates
// per work-item.  The angle is the host libm's double tan of the float half-angle, rounded once to float (for 60 degrees:
// 0x1.279a74p-1f, the reference's constant); tests/camera_oracle.c uses the same expression and the same libm.
struct HostV3 { float x, y, z; };
static HostV3 hv_sub(HostV3 a, HostV3 b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
static HostV3 hv_cross(HostV3 a, HostV3 b)
{
    return { fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)) };
}
static HostV3 hv_normalize(HostV3 a)
{
    const float inv = 1.0f / sqrtf(fmaf(a.z, a.z, fmaf(a.y, a.y, a.x * a.x)));
    return { a.x * inv, a.y * inv, a.z * inv };
}

static_assert(sizeof(pt_camera) == 64 && offsetof(pt_camera, lens_radius) == 40 && offsetof(pt_camera, focus_distance) == 44 &&
              offsetof(pt_camera, reserved) == 48, "pt_camera layout");
static void camera_reference(pt_camera* c)
{
    memset(c, 0, sizeof *c);
    c->eye[0] = 0.0f; c->eye[1] = 2.75f; c->eye[2] = 4.0f;              // :265
    c->center[0] = 0.0f; c->center[1] = 2.75f; c->center[2] = 3.0f;     // :266 eye + (0, 0, -1)
    c->up[0] = 0.0f; c->up[1] = 1.0f; c->up[2] = 0.0f;                  // :267
    c->fov_y_deg = 60.0f;                                               // :263
}

// THE camera derivation, shared by every entry point: the pinhole's thirteen values and the thin lens (include/pt_shim.h: pt_camera).
// The lens is validated here and nowhere else; an entry point that takes none (pt_render_frames_camera) refuses lens_radius > 0 itself
static int camera_derive(const pt_camera* c, PtLensCamera* out)
{
    for (int i = 0; i < 4; ++i)
        if (c->reserved[i] != 0) return fail(PT_ERR_INVALID, "camera: reserved fields must be zero");
    if (!(std::isfinite(c->lens_radius) && c->lens_radius >= 0.0f)) return fail(PT_ERR_INVALID, "camera: lens_radius must be finite and >= 0");
    if (!(std::isfinite(c->focus_distance) && c->focus_distance >= 0.0f)) return fail(PT_ERR_INVALID, "camera: focus_distance must be 0 or finite and > 0");
    if (c->lens_radius > 0.0f && !(c->focus_distance > 0.0f)) return fail(PT_ERR_INVALID, "camera: lens_radius > 0 needs focus_distance > 0");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(c->eye[i]) || !std::isfinite(c->center[i]) || !std::isfinite(c->up[i]))
            return fail(PT_ERR_INVALID, "camera: eye, center and up must be finite");
    if (!(c->fov_y_deg > 0.0f && c->fov_y_deg < 180.0f)) return fail(PT_ERR_INVALID, "camera: fov_y_deg must lie in (0, 180)");
    const HostV3 eye = { c->eye[0], c->eye[1], c->eye[2] };
    const HostV3 center = { c->center[0], c->center[1], c->center[2] };
    const HostV3 up = { c->up[0], c->up[1], c->up[2] };
    const HostV3 view = hv_normalize(hv_sub(center, eye));   // :270
    const HostV3 hol = hv_normalize(hv_cross(view, up));     // :271
    const HostV3 upd = hv_normalize(hv_cross(hol, view));    // :272
    const float fov = (float)(((double)c->fov_y_deg * M_PI) / 180.0);
    const float angle = (float)tan((double)(0.5f * fov));
    const float v[13] = { eye.x, eye.y, eye.z, view.x, view.y, view.z, hol.x, hol.y, hol.z, upd.x, upd.y, upd.z, angle };
    for (float x : v)
        if (!std::isfinite(x)) return fail(PT_ERR_INVALID, "camera: degenerate (center == eye, or up parallel to the view direction)");
    memcpy(out->eye, v, sizeof out->eye);
    memcpy(out->view, v + 3, sizeof out->view);
    memcpy(out->hol, v + 6, sizeof out->hol);
    memcpy(out->up, v + 9, sizeof out->up);
    out->angle = angle;
    out->lens_radius = c->lens_radius;
    out->focus_distance = c->focus_distance;
    return PT_OK;
}

static PtLensCamera reference_camera()
{
    static const PtLensCamera c = [] {
        pt_camera rc;
        camera_reference(&rc);
        PtLensCamera r;
        camera_derive(&rc, &r);
        return r;
    }();
    return c;
}

extern "C" void pt_camera_reference(pt_camera* out)
{
    if (out) camera_reference(out);
}

extern "C" int pt_camera_derive(const pt_camera* cam, float out[16])
{
    if (!cam || !out) return fail(PT_ERR_INVALID, "null argument");
    PtLensCamera c;
    int rc = camera_derive(cam, &c);
    if (rc) return rc;
    const float v[16] = { c.eye[0], c.eye[1], c.eye[2], c.view[0], c.view[1], c.view[2], c.hol[0], c.hol[1], c.hol[2],
                          c.up[0], c.up[1], c.up[2], c.angle, c.lens_radius, c.focus_distance, 0.0f };
    memcpy(out, v, sizeof v);
    return PT_OK;
}

// the prep kernel over n raw records, then the PT_PREP_WORDS it wrote, read back: a host wait (once per scene upload)
static int prep_triangles(pt_device_s* d, const PtRawTriangle* raw, PtPrepTriangle* out, int n, unsigned int (&words)[PT_PREP_WORDS])
{
    HIP_TRY(ptk_prep_triangles(raw, out, n, d->det_bound_dev, d->stream));
    HIP_TRY(hipMemcpyAsync(words, d->det_bound_dev, sizeof words, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return PT_OK;
}

static int ensure_prep(pt_device_s* d, const pt_buffer_s* tris, int ntri)
{
    // wrapped (caller-owned) memory can change behind our back, and so can a buffer whose device pointer has been handed
    // out (pt_buffer_device_ptr: writes through it bump no version): always re-prepare those
    if (d->prep_capacity >= (size_t)ntri && d->prep_src == tris && d->prep_version == tris->version && d->prep_ntri == ntri && tris->owned && !tris->exposed)
        return PT_OK;
    // the prepared scene is about to change under whatever the lanes still run: the handle's stream goes behind them
    int rc = stream_enqueue(d);
    if (rc) return rc;
    if (d->prep_capacity < (size_t)ntri) {
        HIP_TRY(hipStreamSynchronize(d->stream));
        ws_free(d, d->prep);
        ws_free(d, d->scene_filter.p1tab);
        ws_free(d, d->bvh);
        d->bvh_valid = false;
        d->prep_capacity = 0;
        d->prep_src = nullptr;
        d->prep_hash_valid = false;
        size_t cap = std::max<size_t>((size_t)ntri, 64);
        hipError_t e = ws_malloc(d, d->prep, cap * sizeof(PtPrepTriangle));
        if (e == hipSuccess) e = ws_malloc(d, d->scene_filter.p1tab, ptk_p1tab_floats((int)cap) * sizeof(float));
        if (e != hipSuccess) {
            ws_free(d, d->prep);
            return fail(PT_ERR_OOM, "scene workspace allocation failed: %s", hipGetErrorString(e));
        }
        d->prep_capacity = cap;
    }
    unsigned int words[PT_PREP_WORDS];
    if ((rc = prep_triangles(d, (const PtRawTriangle*)tris->dptr, d->prep, ntri, words))) return rc;
    float bound;
    memcpy(&bound, &words[0], sizeof bound);
    d->prep_det_bounded = bound <= PT_DET_BOUND_MAX;  // false for NaN / Inf too
    d->prep_finite = words[2] == 0u && ntri > 0;
    for (int a = 0; a < 3; ++a) {
        d->prep_lo[a] = ptk_order_float(~words[6 + a]);
        d->prep_hi[a] = ptk_order_float(words[9 + a]);
    }
    // every (2k, 2k+1) has e2' == -e2 and is (a,b,c),(c,d,a): quad mode 3 for every camera about which the scene's radius is
    // finite and moderate (ensure_anchor: the margins and the packed table are made per anchor, on the device, no host wait)
    PtFilterTable& ft = d->scene_filter;
    ft.pairs = words[1] == 0u && words[3] == 0u && ntri > 0 && (ntri & 1) == 0 && d->prep_det_bounded && d->prep_finite;
    ft.quads = 0;
    ft.delta1 = 0.0f; ft.ray_radius = 0.0f;
    ft.anchor_valid = false;   // the prep kernel has just zeroed the margins
    d->blocks_per_cu = ptk_trace_blocks_per_cu(ntri);  // the LDS footprint follows the scene
    // Memory the caller can write behind the ABI is prepared again for every render; the checksum of the raw records says whether
    // that changed anything -- if not, the LBVH (a radix sort, a build, host waits) and the primary-ray masks still stand
    const uint64_t hash = (uint64_t)words[4] | ((uint64_t)words[5] << 32);
    if (!(d->prep_src == tris && d->prep_ntri == ntri && d->prep_hash_valid && d->prep_hash == hash)) {
        d->bvh_valid = false;
        d->scene_gen++;
    }
    d->prep_hash = hash;
    d->prep_hash_valid = true;
    d->prep_src = tris;
    d->prep_version = tris->version;
    d->prep_ntri = ntri;
    return PT_OK;
}

// LBVH of the current prepared scene: built on the GPU the first time a render
// of this scene wants it (PT_OPT_ACCEL), kept until the scene changes
static int ensure_bvh(pt_device_s* d, const pt_buffer_s* tris, int ntri)
{
    if (d->bvh_valid) return PT_OK;
    int rc = stream_enqueue(d);   // (a render through the old hierarchy may still be running)
    if (rc) return rc;
    if (!d->bvh) {
        hipError_t e = ws_malloc(d, d->bvh, ptk_bvh_record_count((int)d->prep_capacity) * sizeof(PtBvh8Node));
        if (e != hipSuccess) return fail(PT_ERR_OOM, "BVH allocation failed: %s", hipGetErrorString(e));
    }
    const size_t temp_bytes = ptk_bvh_temp_bytes(ntri);
    void* temp = nullptr;
    hipError_t e = hipMalloc(&temp, temp_bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(PT_ERR_OOM, "BVH build workspace allocation failed: %s", hipGetErrorString(e)); }
    PtBvhGrid* grid_dev = reinterpret_cast<PtBvhGrid*>(d->bigidx + PT_BVH_BIG_MAX + 1);
    e = ptk_bvh_build((const PtRawTriangle*)tris->dptr, d->prep, ntri, d->bvh, d->bigtab, d->bigidx, d->bigidx + PT_BVH_BIG_MAX, grid_dev,
                      reinterpret_cast<unsigned*>(grid_dev + 1), temp, temp_bytes, d->stream);
    struct { int nbig; PtBvhGrid grid; unsigned used; } back;
    memset(&back, 0, sizeof back);
    static_assert(sizeof back == sizeof(int) + sizeof(PtBvhGrid) + sizeof(unsigned), "count, grid and records in use are read back together");
    if (e == hipSuccess) e = hipMemcpyAsync(&back, d->bigidx + PT_BVH_BIG_MAX, sizeof back, hipMemcpyDeviceToHost, d->stream);
    int& nbig = back.nbig;
    hipError_t e2 = hipStreamSynchronize(d->stream);  // once per scene upload; the workspace is freed right after
    hipFree(temp);
    if (e != hipSuccess || e2 != hipSuccess) return fail(PT_ERR_HIP, "BVH build failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    d->nbig = nbig < 0 ? 0 : (nbig > PT_BVH_BIG_MAX ? PT_BVH_BIG_MAX : nbig);
    d->bvh_grid = back.grid;
    d->bvh_records = std::min<size_t>(back.used, ptk_bvh_record_count(ntri));   // (indices are checked against this: a tighter bound than the capacity)
    if (getenv("PT_SHIM_DEBUG"))
        fprintf(stderr, "pt_shim: LBVH over %d triangles: %u records in use (%u nodes, %.2f children per node), %d big triangles outside\n", ntri, back.used,
                back.used > (unsigned)ntri ? back.used - (unsigned)(ntri - d->nbig) : 0u,
                back.used > (unsigned)ntri ? (double)(back.used - 1) / (double)(back.used - (unsigned)(ntri - d->nbig)) : 0.0, d->nbig);
    // The big triangles are searched by the brute-force two-pass search before every traversal.  When their table is made
    // of quads (a,b,c),(c,d,a) -- the Cornell box's walls among a soup of small triangles -- it gets the packed shared-u
    // filter (pt_quad3_pass1) like a quad scene on the brute-force path: same preparation (ensure_prep), on the table.  The
    // filter's error bound is about where RAYS start: anywhere on the scene, so the radius is the whole scene's.
    PtFilterTable& ft = d->big_filter;
    ft.quads = 0; ft.pairs = false; ft.anchor_valid = false;
    if (d->nbig >= 2 && (d->nbig & 1) == 0 && d->prep_det_bounded && d->prep_finite) {
        PtRawTriangle* rawbig = reinterpret_cast<PtRawTriangle*>(ft.p1tab + ptk_p1tab_floats(PT_BVH_BIG_MAX));
        HIP_TRY(ptk_bvh_big_raw((const PtRawTriangle*)tris->dptr, d->bigidx, d->nbig, rawbig, d->stream));
        unsigned int words[PT_PREP_WORDS];
        if ((rc = prep_triangles(d, rawbig, d->bigtab, d->nbig, words))) return rc;  // (rewrites the same records)
        ft.pairs = words[1] == 0u && words[3] == 0u;   // margins and packed table: ensure_anchor, per camera
    }
    d->bvh_valid = true;
    d->bvh_builds++;
    return PT_OK;
}

// The LBVH trace kernels carry the ray term of the boxes' margin (ptk_trace: wide) unless the eye stands in or next to the scene:
// its largest |coordinate| at most PT_BVH_NEAR_EYE x the scene's.  (A scene with a non-finite coordinate: always.)
static bool eye_is_far(const pt_device_s* d, const float eye[3])
{
    if (!d->prep_finite) return true;
    float m = 0.0f, e = 0.0f;
    for (int a = 0; a < 3; ++a) {
        m = std::max(m, std::max(fabsf(d->prep_lo[a]), fabsf(d->prep_hi[a])));
        e = std::max(e, fabsf(eye[a]));
    }
    return !(e <= PT_BVH_NEAR_EYE * m);
}

// max |v - eye|_inf over the prepared scene's vertices, from its per-axis extremes: fl(v - e) is monotone in v, so the largest
// |fl(v - e)| of an axis is reached at its smallest or its largest coordinate -- the same float as a reduction over every
// vertex.  NaN when a coordinate is not finite.
static float anchor_radius(const pt_device_s* d, const float eye[3])
{
    if (!d->prep_finite) return NAN;
    float r = 0.0f;
    for (int a = 0; a < 3; ++a) {
        const float lo = fabsf(d->prep_lo[a] - eye[a]), hi = fabsf(d->prep_hi[a] - eye[a]);
        r = !(lo <= r) ? lo : r;
        r = !(hi <= r) ? hi : r;
    }
    return r;
}

// The pass-1 filter of a quad scene (pt_quad3_pass1) is made about an ANCHOR, the render's eye: its error bounds are sized by
// the scene's radius about it, its packed table holds K = cross(e2, a - eye).  When the eye moves, the margins (pad0 of the
// prepared records) and the packed table are rewritten by kernels enqueued on the handle's stream, behind the renders in
// flight (stream_enqueue: a device-side wait), for table ft -- the brute-force scene's or the LBVH's table of big triangles -- whose
// ntri prepared records are tris.  The pairing checks of the scene preparation do not depend on the camera and stand; the LBVH
// is not touched.  The same eye as the table's does nothing at all.
static int ensure_anchor(pt_device_s* d, PtFilterTable& ft, PtPrepTriangle* tris, int ntri, const float eye[3])
{
    if (ft.anchor_valid && memcmp(ft.anchor, eye, 3 * sizeof(float)) == 0) return PT_OK;
    const float radius = anchor_radius(d, eye);
    ft.quads = 0;
    if (ft.pairs && radius <= 1.0e15f) {
        // quad mode 2: secondary rays start 0.01 off a surface (GenerateColors.cl:253), so their origins stay within ray_radius
        // of the eye -- checked per ray, a ray outside keeps every triangle; the big triangles' filter is about where RAYS
        // start: anywhere on the scene, so its radius is the whole scene's too.  D bounds every coordinate difference between
        // two points of that box; delta1 = 128 u D^2 (derivation: pt_quad2_pass1)
        const float ray_radius = radius * 1.001f + 0.05f;
        const float diameter = 2.0f * ray_radius * 1.001f;
        const float delta1 = 128.0f * 5.9604645e-8f * diameter * diameter * 1.001f;
        // mode 3 (pt_quad3_pass1): deltaP = 192 u D^2; first triangle un >= -deltaP, second un <= delta1 + deltaP
        const float deltaP = 192.0f * 5.9604645e-8f * diameter * diameter * 1.001f;
        int rc = stream_enqueue(d);   // (a render through the old table may still be running)
        if (rc) return rc;
        HIP_TRY(ptk_prep_quad_margins(tris, ntri, diameter, delta1, ft.p1tab, eye, d->stream));
        ft.delta1 = delta1; ft.ray_radius = ray_radius;
        ft.p1_lo = -deltaP; ft.p1_hi = (delta1 + deltaP) * 1.001f;
        ft.quads = 3;
    }
    memcpy(ft.anchor, eye, 3 * sizeof(float));
    ft.anchor_valid = true;
    return PT_OK;
}

// THE search of a render, a query or an ambient-occlusion render, decided here and nowhere else: which one (PtSearchMode, what the
// launchers take), over which filter table, on what grid
struct PtSearch {
    PtSearchMode mode;
    const PtFilterTable* ft;   // the table the two-pass search runs over: the prepared scene's, or the LBVH's big triangles'
    int ntri;
    int driver_blocks;         // the persistent grid of the LBVH driver's kernels (queries, ambient occlusion); 0: brute force
    bool wide;                 // renders through the LBVH: the eye is far from the scene (eye_is_far), the slabs carry the ray term
};

// the search and what it reads: the prepared scene, its LBVH, the filter of the table the two-pass search runs over.
// PT_OPT_ACCEL: 0 = BVH for scenes of PT_BVH_AUTO_MIN triangles or more, 1 = brute force, 2 = BVH (needs >= 2 triangles)
// PT_OPT_QUAD_FILTER: 0 / 4 = the packed shared-u filter when the table allows it, 1..3 = independent triangles
// eye: the filter's anchor, the render's eye.  NULL (a ray query, whose origins are anywhere) keeps the anchor the table has, so
// that a query never rewrites the table under the renders of a moved camera, and makes the reference eye's when it has none.
// An empty scene has nothing to search: neither the prepared scene nor any table is touched
static int prepare_search(pt_device_s* d, const pt_buffer_s* tris, int ntri, const float* eye, PtSearch& s)
{
    s = PtSearch();
    s.ft = &d->scene_filter;
    if (ntri == 0) return PT_OK;
    const bool use_bvh = ntri >= 2 && (d->opt_accel == 2 || (d->opt_accel == 0 && ntri >= PT_BVH_AUTO_MIN));
    if (!use_bvh && ntri >= (1 << 26))
        return fail(PT_ERR_INVALID, "the brute-force search packs a triangle index in 26 bits: use PT_OPT_ACCEL 0 or 2 for %d triangles", ntri);
    if (use_bvh && ntri >= (1 << 25))
        return fail(PT_ERR_INVALID, "the LBVH search packs a record index (2 x triangles) in 26 bits: %d triangles are too many", ntri);
    int rc;
    if ((rc = ensure_prep(d, tris, ntri))) return rc;
    if (use_bvh && (rc = ensure_bvh(d, tris, ntri))) return rc;
    PtFilterTable& ft = use_bvh ? d->big_filter : d->scene_filter;
    const PtLensCamera ref = reference_camera();
    const float* anchor = eye ? eye : ft.anchor_valid ? ft.anchor : ref.eye;
    if ((rc = use_bvh ? ensure_anchor(d, ft, d->bigtab, d->nbig, anchor) : ensure_anchor(d, ft, d->prep, d->prep_ntri, anchor))) return rc;
    s.mode = { use_bvh, d->prep_det_bounded, (d->opt_quads == 0 || d->opt_quads == 4) ? ft.quads : 0 };
    s.ft = &ft;
    s.ntri = ntri;
    s.driver_blocks = use_bvh ? d->prop.multiProcessorCount * d->query_bvh_blocks_per_cu : 0;
    s.wide = use_bvh && eye && eye_is_far(d, eye);
    return PT_OK;
}

// the search fields of a PtTraceParams (for queries and ambient occlusion: PtQueryParams::t, PtAoParams::t): the scene, the filter of
// the table the two-pass search runs over with its anchor in cam.eye, the LBVH
static void search_fields(const pt_device_s* d, const PtSearch& s, PtTraceParams& t)
{
    const PtFilterTable& ft = *s.ft;
    t.tris = d->prep;
    t.ntri = s.ntri;
    t.quad_delta1 = ft.delta1; t.ray_radius = ft.ray_radius;
    t.p1tab = ft.p1tab; t.p1_lo = ft.p1_lo; t.p1_hi = ft.p1_hi;
    memcpy(t.cam.eye, ft.anchor, sizeof t.cam.eye);   // the anchor the table was made about
    t.bvh = d->bvh; t.bvh_records = (int32_t)d->bvh_records; t.grid = d->bvh_grid;
    t.bigtab = d->bigtab; t.bigidx = d->bigidx; t.nbig = s.mode.bvh ? d->nbig : 0;
    t.bvh_flags = d->trav_dev; t.bvh_stack_limit = (int32_t)d->opt_bvh_stack;
}

// ---- the staging ring: whole frames per chunk, as many as a slot holds -------------------------------------------------
// Steady state allocates nothing: the ring exists from the first render on (pt_device_reserve_staging) and is replaced
// only when ONE frame of this image does not fit a slot.  A render of frame_count frames goes in nchunks chunks of `chunk` frames.
static int plan_chunks(pt_device_s* d, int frame_count, uint32_t npix, int& nchunks, int& chunk)
{
    int rc;
    const uint64_t frame_bytes = (uint64_t)npix * 12;
    if (!d->ring || d->ring_slot_bytes < frame_bytes) {
        if (d->ring && (rc = free_ring(d))) return rc;
        if ((rc = alloc_ring(d, (size_t)std::max<uint64_t>(frame_bytes, PT_DEFAULT_SLOT_BYTES)))) return rc;
    }
    uint64_t slot_frames = std::min<uint64_t>(d->ring_slot_bytes / frame_bytes, 16383);   // (fl + ring_phase stays below 65 536: pt_kernels.h, ring_magic)
    if (d->opt_chunk > 0) slot_frames = std::min<uint64_t>(slot_frames, (uint64_t)d->opt_chunk);
    nchunks = (int)(((uint64_t)frame_count + slot_frames - 1) / slot_frames);
    chunk = (frame_count + nchunks - 1) / nchunks;      // S: equal chunks -- 40 frames through a 16-frame slot go 14, 14, 12
    return PT_OK;
}

// primary-ray candidate masks: quad scenes of up to 64 triangles on the brute-force path (PT_OPT_PRIMARY_MASKS).  They are a
// function of the image geometry, the camera and the prepared scene: made when any changes, on the handle's stream, behind the
// lanes.  make: the masks in hand are stale -- room for new ones is made here and their key updated; render_part launches them
static int refresh_pmask(pt_device_s* d, const pt_render_params& rp, const PtCamera& cam, uint32_t npix, bool& make)
{
    int rc;
    const int32_t g[7] = { rp.width, rp.height, rp.stripe_rows, rp.n_ranks, rp.rank, (int32_t)npix, rp.num_triangles };
    make = !d->pmask_key.valid || d->pmask_key.scene_gen != d->scene_gen || memcmp(d->pmask_key.g, g, sizeof g) != 0 ||
           memcmp(&d->pmask_key.cam, &cam, sizeof cam) != 0;
    if (!make) return PT_OK;
    if ((rc = stream_enqueue(d))) return rc;   // (a render with the old masks may still be running; render_part launches the new ones)
    d->pmask_key.valid = false;
    if (d->pmask.bytes < (size_t)npix * sizeof(uint2)) {
        HIP_TRY(hipStreamSynchronize(d->stream));
        ws_free(d, d->pmask);
        hipError_t e = ws_malloc(d, d->pmask, (size_t)npix * sizeof(uint2));
        if (e != hipSuccess) return fail(PT_ERR_OOM, "primary-mask allocation (%zu bytes) failed: %s", (size_t)npix * sizeof(uint2), hipGetErrorString(e));
    }
    d->pmask_key.scene_gen = d->scene_gen;
    memcpy(d->pmask_key.g, g, sizeof g);
    d->pmask_key.cam = cam;
    return PT_OK;
}

// secondary-ray candidate masks (PT_OPT_SECONDARY_MASKS, pt_secmask.h): a function of the prepared scene ALONE -- no camera, no image
// geometry -- made once per scene, on the handle's stream, behind the lanes.  The table is sized by the scene (the Cornell box: 15.9 MB;
// 64 triangles: 28.3 MB) and allocated where the scene's table is made; it grows for a scene of more triangles and is kept otherwise,
// so a render of a scene whose table stands neither allocates nor builds.
static int refresh_smask(pt_device_s* d, int ntri)
{
    int rc;
    if ((d->smask_key.valid || d->smask_key.declined) && d->smask_key.scene_gen == d->scene_gen && d->smask_key.ntri == ntri) return PT_OK;
    if ((rc = stream_enqueue(d))) return rc;   // (a render with the old table may still be running)
    d->smask_key.valid = d->smask_key.declined = false;
    // A triangle without a table (degenerate, too small or too far from the origin of coordinates for the classification's rounding:
    // pt_sm_geom) sends all its rays to pass 2 with every triangle, which costs far more than pass 1 saves: such a scene declines the
    // table.  The records are read back once per scene (4 KiB at the most; the upload has just waited for the device anyway).
    {
        PtPrepTriangle host[PT_SM_TRI_MAX];
        HIP_TRY(hipMemcpyAsync(host, d->prep.p, (size_t)ntri * sizeof(PtPrepTriangle), hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        bool all = true;
        for (int k = 0; k < ntri && all; ++k) all = pt_sm_geom(host[k].p1, host[k].e1, host[k].e2).valid;
        d->smask_key.scene_gen = d->scene_gen;
        d->smask_key.ntri = ntri;
        d->smask_key.declined = !all;
        if (!all) return PT_OK;
    }
    if (d->smask.bytes < PT_SM_TABLE_BYTES(ntri)) {
        HIP_TRY(hipStreamSynchronize(d->stream));
        ws_free(d, d->smask);
        hipError_t e = ws_malloc(d, d->smask, PT_SM_TABLE_BYTES(ntri));
        if (e != hipSuccess) return fail(PT_ERR_OOM, "secondary-mask allocation (%zu bytes) failed: %s", (size_t)PT_SM_TABLE_BYTES(ntri), hipGetErrorString(e));
    }
    HIP_TRY(ptk_secondary_masks(d->prep, ntri, d->smask, d->stream));
    d->smask_key.scene_gen = d->scene_gen;
    d->smask_key.ntri = ntri;
    d->smask_key.valid = true;
    return PT_OK;
}

// The masks' footprint bound (the comment above pt_primary_mask_kernel) takes every ray of a pixel to lie within
// eps = 1.01 h + 4e-6 of the centre ray, h = half a pixel's diagonal on the image plane: that needs the image-plane point the
// kernels compute to be the real one to a small part of a pixel.  It is not on a very large image.  With u = 2^-24 and a pixel
// coordinate of at most W, each of these roundings moves the point by at most u W pixels (to first order; W < 2^24, so (float)xc
// is exact):
//     pt_pixel_jitter:              fl(xc + r), fl(. - 0.5)                                                        2
//     pt_camera_aim's first line:   fl(x + 0.5); inv_w = RN(1 / W) and the product by it, 2; fl(2 c - 1), half (the value
//                                   is at most 1 where the image is 2 wide); the product by angle, half; aspect = RN(W / H)
//                                   and the product by it, 2 halves                                                5
// -- 7 for a sample and 5 for the mask kernel's centre (it has no jitter), 12 u W pixels of 2 angle aspect / W each: 24 u angle
// aspect between the two in x, and no more in y (the second line has no aspect): at most 24 u angle (aspect^2 + 1)^(1/2).
// The bound has 1.01 / (1 + 4e-6) - 1 > 0.0099 of h to give, and pixels are square (aspect / W = 1 / H), h = 2^(1/2) angle / H:
// the premise holds while 24 u (W^2 + H^2)^(1/2) <= 0.0099 2^(1/2).  Masks are made while 28 u (W^2 + H^2)^(1/2) <= 0.009 2^(1/2),
// W^2 + H^2 <= 7626^2 -- the margin covers the second-order terms, aspect's own rounding and the float evaluation of eps; the
// additive 4e-6 is not drawn on.  Every image of up to 4096 x 4096 keeps its masks; a larger one renders as under
// PT_OPT_PRIMARY_MASKS 0 (pass 1 for primary rays too).
static bool pmask_footprint_holds(int width, int height)
{
    return (double)width * width + (double)height * height <= 7626.0 * 7626.0;
}

// Samples per work-queue grab.  A wave that finds the queue empty idles until the last wave is
// done, on average for half a batch: large batches (fewer atomics) when every wave gets many of
// them, smaller ones when the launch is short (a rank's share of a multi-GPU render, small images).
// bpf: batches per frame.  blocks: the persistent grid -- it fills the chip, but never with more waves than a chunk has
// batches; ONE grid for all launches of the render (a checkpoint is resumed by the wave of the same number)
static int choose_batch(const pt_device_s* d, bool use_bvh, uint32_t npix, int chunk, uint32_t& batch, uint32_t& bpf, int& blocks)
{
    const int wg_waves = PT_TRACE_THREADS / 64;
    blocks = d->prop.multiProcessorCount * (use_bvh ? d->bvh_blocks_per_cu : d->blocks_per_cu);   // all the chip holds
    const uint64_t resident_waves = (uint64_t)blocks * wg_waves;
    const uint64_t chunk_samples = (uint64_t)npix * (uint64_t)chunk;
    // (not below 128: at 64 the ONE queue counter takes 4 M atomics per launch of configs[2] and the
    // L2 atomic unit saturates -- measured +30 % launch time)
    batch = PT_TRACE_BATCH;
    while (batch > 128u && chunk_samples / batch < 64u * resident_waves) batch >>= 1;
    bpf = (npix + batch - 1) / batch;
    if ((uint64_t)bpf * (uint64_t)chunk + PT_QUEUE_SHARDS > 0xffffffffull) return fail(PT_ERR_INVALID, "chunk too large");
    const uint64_t blocks_needed = ((uint64_t)bpf * (uint64_t)chunk + wg_waves - 1) / wg_waves;
    if ((uint64_t)blocks > blocks_needed) blocks = (int)blocks_needed;
    return PT_OK;
}

// the image-geometry fields of PtTraceParams: the per-image constants and this rank's stripes with their npix local pixels
static void image_geometry(PtTraceParams& t, int width, int height, int stripe_rows, int n_ranks, int rank, uint32_t npix)
{
    t.width = width; t.height = height;
    t.inv_width = 1.0f / (float)width;     // IEEE quotients: the translation unit is compiled without fast-math
    t.inv_height = 1.0f / (float)height;
    t.aspect = (float)width / (float)height;
    t.stripe_rows = stripe_rows; t.n_ranks = n_ranks; t.rank = rank;
    t.npix_local = npix;
}

// what every trace launch of the render is given; render_part's trace() sets the per-launch rest (queue, frames, checkpoints)
static PtTraceParams trace_params(const pt_device_s* d, const pt_buffer_s* mats, const pt_buffer_s* stats, const pt_render_params& rp,
                                  const PtCamera& cam, uint32_t npix, const PtSearch& search, bool use_pmask, int chunk, uint32_t batch, uint32_t bpf)
{
    PtTraceParams tp;
    memset(&tp, 0, sizeof tp);
    search_fields(d, search, tp);
    tp.mats = (const PtRawMaterial*)mats->dptr;
    tp.stats = stats ? (unsigned long long*)stats->dptr : nullptr;
    image_geometry(tp, rp.width, rp.height, rp.stripe_rows, rp.n_ranks, rp.rank, npix);
    tp.max_bounces = rp.max_bounces; tp.nmat = rp.num_materials;
    tp.batches_per_frame = bpf; tp.batch = batch;
    tp.pmask = use_pmask ? d->pmask.p : nullptr;
    tp.slot_frames = (uint32_t)chunk;
    tp.ring_magic = (uint32_t)(0x100000000ull / (2u * (uint32_t)chunk)) + 1u;
    tp.rad = d->ring;
    tp.rad1 = reinterpret_cast<float*>(reinterpret_cast<char*>(d->ring.p) + d->ring_slot_bytes);
    // the form of a sample's radiance address, once per render: a path carries its record's byte offset from the ring's base in 32 bits
    // while the whole ring is at most 4 GiB (the last record then ends at or below 2^32); a larger ring (pt_device_reserve_staging takes any
    // size) keeps the long form, which carries the local pixel and forms the 64-bit address at the store
    tp.rad1_off = (uint64_t)PT_RING_SLOTS * d->ring_slot_bytes <= 0x100000000ull ? (uint32_t)d->ring_slot_bytes : 0u;
    tp.cam = cam;   // (its eye is the table's anchor bit for bit: prepare_search anchored the table there)
    return tp;
}

// the checkpoint regions of both lanes, for as many waves as any kernel's grid can have
static int ensure_carry(pt_device_s* d, int blocks)
{
    const int wg_waves = PT_TRACE_THREADS / 64;
    const size_t waves = (size_t)d->prop.multiProcessorCount * 8 * wg_waves;   // (no kernel has more than 8 workgroups per CU resident)
    if ((size_t)blocks * wg_waves > waves) return fail(PT_ERR_INVALID, "grid larger than the checkpoint regions");
    for (int k = 0; k < 2; ++k)
        if (!d->carry[k]) {   // once per device handle, at its first such render
            // (a region serves whichever kernel the render runs: PT_POOL searched-path records of a table kernel are more than the LBVH
            // kernel's 64 paths -- pt_kernels.h asserts it)
            hipError_t e = ws_malloc(d, d->carry[k], waves * PT_CARRY_HIT_STRIDE_DW * sizeof(uint32_t));
            if (e != hipSuccess) return fail(PT_ERR_OOM, "checkpoint buffer allocation failed: %s", hipGetErrorString(e));
        }
    return PT_OK;
}

// one render of at most 32 768 frames: its launches on one lane (pt_device_s).  ev_start / ev_stop: the caller's event, when
// this part begins / ends the call
static int render_part(pt_device_s* d, pt_buffer_s* tris, pt_buffer_s* mats, pt_buffer_s* fb, const pt_render_params& rp, const PtCamera& cam,
                       uint32_t npix, pt_buffer_s* stats, pt_event_s* ev_start, pt_event_s* ev_stop)
{
    int rc;
    PtSearch search;
    if ((rc = prepare_search(d, tris, rp.num_triangles, cam.eye, search))) return rc;
    const bool use_bvh = search.mode.bvh;
    // the kernel with the table in LDS parks a path's bounce count in 8 bits (PT_PACKED_BOUNCE_MAX)
    if (!use_bvh && rp.num_triangles <= PT_LDS_TRI_MAX && rp.max_bounces > PT_PACKED_BOUNCE_MAX)
        return fail(PT_ERR_INVALID, "max_bounces above %d on a scene of at most %d triangles without the LBVH (a parked path packs its bounce count in 8 bits)",
                    PT_PACKED_BOUNCE_MAX, PT_LDS_TRI_MAX);
    int nchunks, chunk;
    if ((rc = plan_chunks(d, rp.frame_count, npix, nchunks, chunk))) return rc;
    const bool want_pmask = d->opt_pmask && search.mode.quads == 3 && !use_bvh && rp.num_triangles <= 64 && search.mode.det_bounded;
    const bool use_pmask = want_pmask && pmask_footprint_holds(rp.width, rp.height);
    if (want_pmask && !use_pmask) d->pmask_key.valid = false;   // declined: no table stands for this render (pt_primary_mask_snapshot)
    bool make_pmask = false;
    if (use_pmask && (rc = refresh_pmask(d, rp, cam, npix, make_pmask))) return rc;
    // the secondary rays' table: the same scenes, whatever the camera and the image; a scene that does not qualify declines it and
    // no table stands for it (pt_secondary_mask_snapshot) -- the allocation stays for the next one that does
    const bool can_smask = search.mode.quads == 3 && !use_bvh && rp.num_triangles <= PT_SM_TRI_MAX && search.mode.det_bounded;
    const bool use_smask = can_smask && d->opt_smask;
    if (!can_smask) d->smask_key.valid = d->smask_key.declined = false;
    if (use_smask && (rc = refresh_smask(d, rp.num_triangles))) return rc;
    if (d->counters_dirty) {   // an earlier call failed between a trace launch and the fold that resets its counter
        if ((rc = stream_enqueue(d))) return rc;
        HIP_TRY(hipMemsetAsync(d->counters, 0, WS_COUNTERS, d->stream));
        d->counters_dirty = false;
    }
    uint32_t batch, bpf;
    int blocks;
    if ((rc = choose_batch(d, use_bvh, npix, chunk, batch, bpf, blocks))) return rc;
    PtTraceParams tp = trace_params(d, mats, stats, rp, cam, npix, search, use_pmask, chunk, batch, bpf);
    tp.smask = use_smask && d->smask_key.valid ? d->smask.p : nullptr;
    if (make_pmask) {
        HIP_TRY(ptk_primary_masks(tp, d->stream));  // (once per scene, camera and image geometry: one thread per pixel)
        d->pmask_key.valid = true;
    }
    // checkpointed launches (PtTraceParams::carry): the table kernels stop at a fresh-phase boundary, the LBVH kernel between two searches
    // (a render of ONE chunk has nothing to hand on: its only launch runs its paths out, beside the next render's first launch on the other lane --
    // a checkpoint would add the draining launch and the checkpoint's traffic for nothing: 30.64 against 30.41 ms per one-launch configs[2] render)
    const bool carry = d->opt_carry != 0 && nchunks > 1;
    // the lane: one per render when its launches are checkpointed (each resumes its predecessor); otherwise the CHUNKS alternate, so that
    // chunk c+1's launch becomes resident while chunk c's runs its paths out (an LBVH launch's tail is milliseconds of falling lane use)
    int ln = d->opt_lanes == 2 ? (int)(d->render_seq++ & 1u) : 0;
    hipStream_t st = d->lane[ln];
    if (carry && (rc = ensure_carry(d, blocks))) return rc;
    const int wg_waves = PT_TRACE_THREADS / 64;

    // ---- fork: the lanes go behind the handle's stream (what uploaded the scene, cleared the framebuffer, made the masks ...)
    if (d->main_dirty || d->external) {
        HIP_TRY(hipEventRecord(d->ev_fork, d->stream));
        HIP_TRY(hipStreamWaitEvent(d->lane[0], d->ev_fork, 0));
        HIP_TRY(hipStreamWaitEvent(d->lane[1], d->ev_fork, 0));
        d->main_dirty = false;
    }
    d->lanes_busy = true;
    d->counters_dirty = true;   // until the last fold of this call is enqueued
    if (ev_start) HIP_TRY(hipEventRecord(ev_start->start, st));
    tp.ring_phase = (uint32_t)((d->chunk_seq & 1u) ? chunk : 0);   // the render's first chunk goes to slot chunk_seq % 2
    tp.carry = carry ? d->carry[ln].p : nullptr;
    unsigned int* const drain_counter = d->counters + (size_t)(PT_QUEUE_COUNTERS - 1 - ln) * PT_QUEUE_STRIDE;
    unsigned int* prev_counter = nullptr;
    int prev_slot = 0, prev_f0 = 0, prev_nf = 0;
    hipEvent_t pstop;
    // fold of the chunk [f0, f0 + nf) staged in ring slot `slot`: behind the newest fold of the other lane (the chain), then
    // the slot is free again
    bool chained = false;   // this render's folds are behind the previous render's (on the other lane)
    auto fold = [&](int slot, int f0, int nf, unsigned int* reset, unsigned int* reset2) -> int {
        const bool last = f0 + nf >= rp.frame_count || !carry, last_two = f0 + nf + chunk >= rp.frame_count;
        if ((!chained || !carry) && d->fold_recorded[ln ^ 1]) HIP_TRY(hipStreamWaitEvent(st, d->ev_fold[ln ^ 1], 0));
        chained = true;
        PtFoldParams fp;
        fp.rad = slot ? tp.rad1 : tp.rad;
        fp.fb = (float4*)fb->dptr;
        fp.npix_local = npix;
        fp.frame_begin = rp.frame_begin + f0;
        fp.frame_count = nf;
        fp.reset_counter = reset;
        fp.reset_counter2 = reset2;
        int r = prof_begin(d, PT_PROF_FOLD, st, &pstop);
        if (r) return r;
        HIP_TRY(ptk_fold(fp, st));
        if ((r = prof_end(st, pstop))) return r;
        // what other lanes wait for: the slot is free again (the next render's first two chunks), the fold chain's newest link (its
        // first fold; lanes_join) -- only a render's last two folds can be either when all its launches share a lane
        if (last_two) {
            HIP_TRY(hipEventRecord(d->ev_slot[slot], st));
            d->slot_recorded[slot] = true;
        }
        if (last) {
            HIP_TRY(hipEventRecord(d->ev_fold[ln], st));
            d->fold_recorded[ln] = true;
            d->last_fold_lane = ln;
        }
        return PT_OK;
    };
    auto trace = [&](int f0, int nf, unsigned int* counter, bool carry_in, bool carry_out) -> int {
        tp.batch_counter = counter;
        tp.frame_begin = rp.frame_begin + f0;
        tp.frame_count = nf;
        tp.chunk_f0 = (uint32_t)f0;
        tp.carry_in_waves = carry_in ? (uint32_t)(blocks * wg_waves) : 0u;
        tp.carry_out = carry_out ? 1u : 0u;
        tp.total_batches = (uint32_t)((uint64_t)bpf * (uint64_t)nf);
        int r = prof_begin(d, PT_PROF_TRACE, st, &pstop);
        if (r) return r;
        HIP_TRY(ptk_trace(tp, blocks, search.mode, d->opt_tally != 0 && stats != nullptr, search.wide, st));
        return prof_end(st, pstop);
    };
    for (int c = 0; c < nchunks; ++c) {
        const int f0 = c * chunk;
        const int nf = std::min(chunk, rp.frame_count - f0);
        const uint64_t seq = d->chunk_seq++;
        const int slot = (int)(seq & 1u);
        unsigned int* counter = d->counters + (size_t)(seq % (PT_QUEUE_COUNTERS - 2)) * PT_QUEUE_STRIDE;
        if (!carry && d->opt_lanes == 2 && c > 0) {
            ln ^= 1;
            st = d->lane[ln];
        }
        // the slot must have been folded out (by the other lane, when this is one of a render's first two chunks)
        if (c < 2 && d->slot_recorded[slot]) HIP_TRY(hipStreamWaitEvent(st, d->ev_slot[slot], 0));
        if ((rc = trace(f0, nf, counter, carry && c > 0, carry))) return rc;
        if (!carry) {
            if ((rc = fold(slot, f0, nf, counter, nullptr))) return rc;
        } else {
            // chunk c - 1 is complete now: this launch finished the paths its own left unfinished
            if (c > 0 && (rc = fold(prev_slot, prev_f0, prev_nf, prev_counter, nullptr))) return rc;
            prev_slot = slot; prev_f0 = f0; prev_nf = nf; prev_counter = counter;
        }
    }
    if (carry) {
        // D: an empty queue, no checkpoint at its end -- the last chunk's paths run out here (beside the next render's first
        // launch on the other lane) -- and the last fold
        if ((rc = trace(rp.frame_count, 0, drain_counter, true, false))) return rc;
        if ((rc = fold(prev_slot, prev_f0, prev_nf, prev_counter, drain_counter))) return rc;
    }
    d->counters_dirty = false;
    if (ev_stop) {
        HIP_TRY(hipEventRecord(ev_stop->stop, st));
        ev_stop->recorded = true;
    }
    // a stream of the caller's (pt_device_set_stream) promises stream order to code we cannot see: it goes behind the render now
    if (d->external && (rc = lanes_join(d))) return rc;
    return PT_OK;
}

// an image's geometry, this rank's stripes of it and a frame range, as every entry point that takes them checks them; npix: the
// rank's local pixels
static int check_image(const char* invalid, int width, int height, int frame_begin, int frame_count, int stripe_rows, int n_ranks, int rank, uint64_t& npix)
{
    if (width < 1 || height < 1 || frame_begin < 0 || frame_count < 0 || stripe_rows < 1 || n_ranks < 1 || rank < 0 || rank >= n_ranks)
        return fail(PT_ERR_INVALID, "%s", invalid);
    if ((long long)width * height > 0x7fffffffLL) return fail(PT_ERR_INVALID, "image too large");
    if ((long long)frame_begin + frame_count > 0x7fffffffLL) return fail(PT_ERR_INVALID, "frame index overflow");
    npix = (uint64_t)pt_local_rows(height, stripe_rows, n_ranks, rank) * (uint64_t)width;
    return PT_OK;
}

// pixel_count: 0 = all local pixels; otherwise the first pixel_count local pixels (n_ranks must be 1)
static int render_internal(pt_device_s* d, pt_buffer_s* tris, pt_buffer_s* mats, pt_buffer_s* fb,
                           const pt_render_params& rp, const PtCamera& cam, uint32_t pixel_count, pt_buffer_s* stats, pt_event_s* ev)
{
    if (!tris || !mats || !fb) return fail(PT_ERR_INVALID, "null buffer handle");
    int rc = check_same_device(d, { tris, mats, fb, stats });
    if (rc) return rc;
    if (rp.max_bounces < 1 || rp.num_triangles < 0 || rp.num_materials < 1) return fail(PT_ERR_INVALID, "invalid render parameters");
    // shading gathers the hit's {n, id} and its material by 32-bit byte offsets into the 64-byte records (pt_shade): brute force or LBVH alike
    if ((uint64_t)rp.num_triangles * 64u > 0xffffffffull || (uint64_t)rp.num_materials * 64u > 0xffffffffull)
        return fail(PT_ERR_INVALID, "a scene has fewer than 2^26 triangles and 2^26 materials");
    for (int i = 0; i < 6; ++i)
        if (rp.reserved[i] != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    uint64_t npix64;
    if ((rc = check_image("invalid render parameters", rp.width, rp.height, rp.frame_begin, rp.frame_count, rp.stripe_rows, rp.n_ranks, rp.rank, npix64))) return rc;
    if (rp.max_bounces > 65535) return fail(PT_ERR_INVALID, "max_bounces above 65535 (a parked path packs its bounce count in 16 bits)");
    if (pixel_count) {
        if (rp.n_ranks != 1) return fail(PT_ERR_INVALID, "pixel_count needs n_ranks == 1");
        npix64 = std::min<uint64_t>(npix64, pixel_count);
    }
    uint32_t npix = (uint32_t)npix64;
    if ((rc = check_triangles(tris, rp.num_triangles))) return rc;
    if ((size_t)rp.num_materials * sizeof(PtRawMaterial) > mats->bytes)
        return fail(PT_ERR_RANGE, "material buffer holds %zu bytes, %d materials need %zu", mats->bytes, rp.num_materials,
                    (size_t)rp.num_materials * sizeof(PtRawMaterial));
    if ((size_t)npix * sizeof(float4) > fb->bytes)
        return fail(PT_ERR_RANGE, "framebuffer holds %zu bytes, %u pixels need %zu", fb->bytes, npix, (size_t)npix * sizeof(float4));
    if (stats && stats->bytes < PT_STAT_WORDS * sizeof(uint64_t)) return fail(PT_ERR_RANGE, "stats buffer too small");

    // a search that was cut short in an earlier render is reported before anything new is enqueued (PT_ERR_TRAVERSAL is deferred)
    if ((rc = check_traversal(d)) || (rc = check_event(d, ev))) return rc;
    if (npix == 0 || rp.frame_count == 0) {
        if ((rc = lanes_join(d)) || (rc = event_begin(d, ev))) return rc;
        return event_end(d, ev);
    }
    // a path keeps its frame, counted from the render's first, in 16 bits: longer renders go in parts (each its own sequence
    // of launches on one lane; the fold chain joins them)
    const int PART = 32768;
    pt_render_params part = rp;
    for (int done = 0; done < rp.frame_count; done += PART) {
        part.frame_begin = rp.frame_begin + done;
        part.frame_count = std::min(PART, rp.frame_count - done);
        if ((rc = render_part(d, tris, mats, fb, part, cam, npix, stats, done == 0 ? ev : nullptr, done + PART >= rp.frame_count ? ev : nullptr))) return rc;
    }
    fb->version++;
    if (stats) stats->version++;
    return PT_OK;
}

// what GenerateColors launches render: the reference's constants, one rank
static pt_render_params reference_params(int width, int height, int frame_begin, int frame_count, const pt_buffer_s* mats)
{
    pt_render_params rp;
    memset(&rp, 0, sizeof rp);
    rp.width = width; rp.height = height;
    rp.frame_begin = frame_begin; rp.frame_count = frame_count;
    rp.max_bounces = 16;    // BOUNCES       GenerateColors.cl:5
    rp.num_triangles = 36;  // NUM_TRIANGLES GenerateColors.cl:6
    rp.num_materials = (int)std::min<size_t>(mats->bytes / sizeof(PtRawMaterial), 0x7fffffff);
    rp.stripe_rows = 1; rp.n_ranks = 1; rp.rank = 0;
    return rp;
}

static int flush_pending(pt_device_s* d)
{
    if (!d->pending.active) return PT_OK;
    PendingFrames p = d->pending;
    d->pending.active = false;
    return render_internal(d, p.tris, p.mats, p.fb, reference_params(p.width, p.height, p.z_begin, p.z_count, p.mats), reference_camera(),
                           p.pixel_count, nullptr, nullptr);
}

extern "C" int pt_render_frames_camera(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t framebuffer,
                                       const pt_render_params* params, const pt_camera* cam, pt_buffer_t stats, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!params) return fail(PT_ERR_INVALID, "params == NULL");
    PtLensCamera c = reference_camera();
    if (cam && (rc = camera_derive(cam, &c))) return rc;   // (nothing enqueued, nothing submitted)
    // the fused kernels' primary-ray masks and pass-1 tables are built on org == eye bit for bit: no lens here
    if (c.lens_radius > 0.0f)
        return fail(PT_ERR_INVALID, "pt_render_frames_camera takes no thin lens (lens_radius > 0): render it with pt_render_indirect and no lights "
                                    "(IndirectRenderer), which computes the same image and takes the lens");
    if ((rc = flush_pending(d))) return rc;
    return render_internal(d, triangles, materials, framebuffer, *params, c, 0, stats, ev);
}

extern "C" int pt_render_frames(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t framebuffer,
                                const pt_render_params* params, pt_buffer_t stats, pt_event_t ev)
{
    return pt_render_frames_camera(d, triangles, materials, framebuffer, params, nullptr, stats, ev);
}

// ---- batched ray queries (include/pt_shim.h) ------------------------------------------------------------------------------
// On the handle's stream, behind the renders in flight (enter_stream: a device-side wait), through the renders' prepared scene,
// LBVH and filter tables (prepare_search): a triangle buffer the renders use is neither prepared again nor rebuilt.
static_assert(sizeof(pt_ray) == 32 && sizeof(pt_hit) == 48, "query record layout");

// pt_intersect_rays and pt_occluded_rays: the argument checks, the deferred error, the stream, the scene, the launch.
// occluded: 1 / 0 results (int32) instead of pt_hit records; early_exit: (occluded only) through the LBVH the search is the any-hit
// one, which stops at the first accepted triangle -- brute force keeps the two-pass closest search (a few dozen triangles leave
// little to stop early from)
static int query_rays(pt_device_s* d, pt_buffer_s* triangles, int num_triangles, pt_buffer_s* rays, pt_buffer_s* out, size_t num_rays,
                      bool occluded, bool early_exit, pt_event_s* ev)
{
    int rc;
    if (!triangles || !rays || !out) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { triangles, rays, out })) || (rc = check_event(d, ev))) return rc;
    if (num_triangles < 0) return fail(PT_ERR_INVALID, "num_triangles < 0");
    if ((rc = check_triangles(triangles, num_triangles))) return rc;
    if (num_rays > 0x7fffffffu) return fail(PT_ERR_RANGE, "%zu rays: at most 2^31 - 1 per call", num_rays);
    const size_t ray_bytes = num_rays * sizeof(pt_ray), out_bytes = num_rays * (occluded ? sizeof(int32_t) : sizeof(pt_hit));
    if (ray_bytes > rays->bytes) return fail(PT_ERR_RANGE, "ray buffer holds %zu bytes, %zu rays need %zu", rays->bytes, num_rays, ray_bytes);
    if (out_bytes > out->bytes) return fail(PT_ERR_RANGE, "result buffer holds %zu bytes, %zu results need %zu", out->bytes, num_rays, out_bytes);
    if (num_rays && (((uintptr_t)rays->dptr | (uintptr_t)out->dptr) & 15u)) return fail(PT_ERR_INVALID, "ray and result buffers must be 16-byte aligned");
    if (ranges_overlap(rays, ray_bytes, out, out_bytes)) return fail(PT_ERR_INVALID, "the rays and the results overlap");
    // a search that was cut short earlier is reported before anything new is enqueued (PT_ERR_TRAVERSAL is deferred)
    if ((rc = check_traversal(d))) return rc;
    if ((rc = enter_stream(d))) return rc;
    PtSearch search;
    if (num_rays && (rc = prepare_search(d, triangles, num_triangles, nullptr, search))) return rc;
    if ((rc = event_begin(d, ev))) return rc;
    if (num_rays) {
        PtQueryParams q;
        memset(&q, 0, sizeof q);
        search_fields(d, search, q.t);
        q.rays = (const float4*)rays->dptr;
        q.out = out->dptr;
        q.nrays = (uint32_t)num_rays;
        q.occluded = occluded;
        HIP_TRY(ptk_query(q, search.driver_blocks, search.mode, early_exit && search.mode.bvh, d->stream));
    }
    out->version++;
    return event_end(d, ev);
}

extern "C" int pt_intersect_rays(pt_device_t d, pt_buffer_t triangles, int num_triangles, pt_buffer_t rays, pt_buffer_t out,
                                 size_t num_rays, int mode, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (mode != PT_QUERY_CLOSEST && mode != PT_QUERY_OCCLUDED) return fail(PT_ERR_INVALID, "mode %d is neither PT_QUERY_CLOSEST nor PT_QUERY_OCCLUDED", mode);
    return query_rays(d, triangles, num_triangles, rays, out, num_rays, mode == PT_QUERY_OCCLUDED, false, ev);
}

extern "C" int pt_occluded_rays(pt_device_t d, pt_buffer_t triangles, int num_triangles, pt_buffer_t rays, pt_buffer_t out,
                                size_t num_rays, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    return query_rays(d, triangles, num_triangles, rays, out, num_rays, true, true, ev);
}

// ---- ambient occlusion (include/pt_shim.h) -----------------------------------------------------------------------------------
static_assert(sizeof(pt_ao_params) == 64, "pt_ao_params layout");

extern "C" int pt_render_ao(pt_device_t d, pt_buffer_t triangles, pt_buffer_t counts, pt_buffer_t image, const pt_ao_params* params,
                            const pt_camera* cam, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!params) return fail(PT_ERR_INVALID, "params == NULL");
    const pt_ao_params a = *params;
    PtLensCamera c = reference_camera();
    if (cam && (rc = camera_derive(cam, &c))) return rc;
    if (!triangles || !counts) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { triangles, counts, image })) || (rc = check_event(d, ev))) return rc;
    if (a.num_triangles < 0 || a.rays_per_sample < 1 || a.rays_per_sample > 256 || !(std::isfinite(a.radius) && a.radius > 0.0f) || !std::isfinite(a.miss_value))
        return fail(PT_ERR_INVALID, "invalid AO parameters");
    for (int i = 0; i < 5; ++i)
        if (a.reserved[i] != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    uint64_t npix64;
    if ((rc = check_image("invalid AO parameters", a.width, a.height, a.frame_begin, a.frame_count, a.stripe_rows, a.n_ranks, a.rank, npix64))) return rc;
    // open <= frames K and K hits <= frames K: neither uint32 count can wrap
    if (((long long)a.frame_begin + a.frame_count) * a.rays_per_sample > 0xffffffffLL)
        return fail(PT_ERR_RANGE, "(frame_begin + frame_count) x rays_per_sample exceeds 2^32 - 1: the counts could wrap");
    const uint32_t npix = (uint32_t)npix64;
    const size_t count_bytes = (size_t)npix * 8;
    const PtSpan C = { counts, count_bytes, 8, "the count buffer" }, G = { image, (size_t)npix * sizeof(float4), 16, "the image buffer" };
    if ((rc = check_triangles(triangles, a.num_triangles)) || (rc = span_fits(C)) || (rc = span_fits(G))) return rc;
    if ((rc = span_aligned(C)) || (rc = span_aligned(G)) || (rc = spans_apart({ C, G }))) return rc;
    // a search that was cut short earlier is reported before anything new is enqueued (PT_ERR_TRAVERSAL is deferred)
    if ((rc = check_traversal(d))) return rc;
    if ((rc = enter_stream(d))) return rc;
    if (a.frame_count == 0 || npix == 0) {
        if ((rc = event_begin(d, ev))) return rc;
        return event_end(d, ev);
    }
    PtSearch search;
    if ((rc = prepare_search(d, triangles, a.num_triangles, nullptr, search))) return rc;
    if ((rc = event_begin(d, ev))) return rc;
    if (a.frame_begin == 0) HIP_TRY(hipMemsetAsync(counts->dptr, 0, count_bytes, d->stream));   // the :314-321 rule: frame 0 starts afresh
    if (a.num_triangles > 0) {
        PtAoParams p;
        memset(&p, 0, sizeof p);
        search_fields(d, search, p.t);
        image_geometry(p.t, a.width, a.height, a.stripe_rows, a.n_ranks, a.rank, npix);
        p.cam = c;
        p.counts = (unsigned long long*)counts->dptr;
        p.npix = npix;
        p.K = a.rays_per_sample;
        p.tlim = a.radius < 1e20f ? a.radius : 1e20f;
        // frame-major samples, fewer than 2^31 per launch
        const int per_launch = (int)std::max<uint32_t>(1u, 0x7fffffffu / npix);
        for (int64_t done = 0; done < a.frame_count; done += per_launch) {   // (64-bit: done + per_launch may pass 2^31 - 1)
            const int nf = (int)std::min<int64_t>(per_launch, a.frame_count - done);
            p.frame0 = a.frame_begin + (int)done;
            p.nitems = (uint32_t)nf * npix;
            HIP_TRY(ptk_ao(p, search.driver_blocks, search.mode, d->stream));
        }
    }
    if (image) HIP_TRY(ptk_ao_resolve((const uint2*)counts->dptr, (float4*)image->dptr, npix, (uint32_t)a.rays_per_sample, a.miss_value, d->stream));
    counts->version++;
    if (image) image->version++;
    return event_end(d, ev);
}

// ---- direct illumination (include/pt_shim.h) -----------------------------------------------------------------------------------
static_assert(sizeof(pt_direct_params) == 64, "pt_direct_params layout");
static_assert(sizeof(pt_indirect_params) == 64, "pt_indirect_params layout");

static_assert(sizeof(pt_roulette) == 16, "pt_roulette layout");
static_assert(sizeof(pt_ris) == 16, "pt_ris layout");
static_assert(sizeof(pt_environment) == 16, "pt_environment layout");
static_assert(sizeof(pt_adaptive_rule) == 32 && sizeof(pt_pixel_slot) == 8 && sizeof(pt_pixel_slot) == sizeof(uint2), "adaptive record layout");

// ONE lit call, as its entry point describes it: pt_render_direct, pt_render_indirect, pt_render_indirect_mis, the two _power entry
// points, pt_render_indirect_rr, pt_render_indirect_pixels, the three _ris and the two _env entry points and pt_radiance_rays each fill
// one and hand it to render_lit -- one validation, one chunk loop
struct PtLitCall {
    PtLitKind kind;             // which kernels (pt_kernels.h); what follows is read as far as the kind says
    pt_buffer_t triangles, materials, lights, samples, framebuffer;
    pt_buffer_t light_counts;   // kind.mis: the list entries per triangle (pt_light_counts)
    pt_buffer_t cdf, tri_q;     // kind.power: the selection table (pt_light_table)
    pt_buffer_t list;           // kind.list: the pixel list; frame_count frames of each of its num_listed slots are rendered, the
    uint32_t num_listed;        //   workspace is laid out for num_listed pixels and the fold is ptk_fold_list
    pt_direct_params a;         // the fields the parameter blocks share (each entry point has looked at its own reserved ones)
    int max_bounces;            // kind.indirect: the depth of the paths
    pt_roulette rr;             // kind.rr: the roulette (roulette_args has checked it)
    int candidates;             // kind.ris: M (ris_args has checked it)
    pt_buffer_t env, env_cdf;   // kind.env: the map and its selection table (pt_env_table)
    pt_environment e;           //   and its block (env_args has checked it)
    bool from_rays;             // pt_radiance_rays (ptk_lit_rays_valid(kind)): the caller's rays stand where the local pixels stand --
    pt_buffer_t rays, moments;  //   a.frame_begin / a.frame_count are the sample range, the image fields of `a` and the camera are not
    uint32_t num_rays;          //   read, there is no framebuffer and no fold; each chunk is followed by ptk_sample_moments into
    uint32_t first_ray;         //   `moments` (may be NULL), `reset` at the first
    int reset;
    const pt_camera* cam;
    pt_event_t ev;
    const char* what;           // the message for a field out of range
};

// (light_counts, cdf, tri_q: NULL from an entry point that has none; the counts are kept only for a kind that reads them)
static PtLitCall lit_call(PtLitKind kind, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, pt_buffer_t light_counts,
                          pt_buffer_t cdf, pt_buffer_t tri_q, pt_buffer_t samples, pt_buffer_t framebuffer, const pt_camera* cam, pt_event_t ev)
{
    PtLitCall c = {};
    c.kind = kind;
    c.triangles = triangles; c.materials = materials; c.lights = lights; c.samples = samples; c.framebuffer = framebuffer;
    c.light_counts = kind.mis ? light_counts : nullptr;
    c.cdf = cdf; c.tri_q = tri_q;
    c.cam = cam; c.ev = ev;
    c.what = kind.indirect ? "invalid indirect-illumination parameters" : "invalid direct-illumination parameters";
    return c;
}

static int render_lit(pt_device_t d, const PtLitCall& c)
{
    const pt_direct_params& a = c.a;
    const bool mis = c.kind.mis, power = c.kind.power;
    const pt_buffer_t triangles = c.triangles, materials = c.materials, lights = c.lights, light_counts = c.light_counts, cdf = c.cdf,
                      tri_q = c.tri_q, samples = c.samples, framebuffer = c.framebuffer, list = c.list;
    int rc;
    PtLensCamera cam = reference_camera();
    if (c.cam && (rc = camera_derive(c.cam, &cam))) return rc;
    const bool rays = c.from_rays;   // (no framebuffer: the rays stand in its place)
    if (!triangles || !materials || !samples || (!rays && !framebuffer) || (c.kind.list && !list) || (rays && !c.rays)) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { triangles, materials, lights, light_counts, samples, framebuffer, cdf, tri_q, list, c.env, c.env_cdf, c.rays, c.moments })) || (rc = check_event(d, c.ev))) return rc;
    if (a.num_triangles < 0 || a.num_materials < 1 || a.num_lights < 0 || a.light_samples < 1 || a.light_samples > 256)
        return fail(PT_ERR_INVALID, "%s", c.what);
    if (a.num_lights >= (1 << 24)) return fail(PT_ERR_INVALID, "num_lights must stay below 2^24 (its float32 value must be exact)");
    if (a.num_lights > 0 && !lights) return fail(PT_ERR_INVALID, "num_lights > 0 needs a light list");
    if (mis && a.num_lights > 0 && !light_counts) return fail(PT_ERR_INVALID, "num_lights > 0 needs the light counts (pt_light_counts)");
    if (power && a.num_lights > 0 && !(cdf && tri_q)) return fail(PT_ERR_INVALID, "num_lights > 0 needs the light table (pt_light_table)");
    // the light's record and the materials are gathered by 32-bit byte offsets into the 64-byte records, as shading gathers them
    if ((uint64_t)a.num_triangles * 64u > 0xffffffffull || (uint64_t)a.num_materials * 64u > 0xffffffffull)
        return fail(PT_ERR_INVALID, "a scene has fewer than 2^26 triangles and 2^26 materials");
    uint64_t npix64;
    if (rays) {   // the ids first_ray .. first_ray + n - 1 and the samples' numbers are the renderers' gid and frame: below 2^31
        if (a.frame_begin < 0 || a.frame_count < 0) return fail(PT_ERR_INVALID, "%s", c.what);
        if ((uint64_t)c.first_ray + c.num_rays > 0x7fffffffull) return fail(PT_ERR_INVALID, "first_ray + num_rays exceeds 2^31 - 1");
        if ((long long)a.frame_begin + a.frame_count > 0x7fffffffLL) return fail(PT_ERR_INVALID, "sample_begin + sample_count exceeds 2^31 - 1");
        npix64 = c.num_rays;
    } else if ((rc = check_image(c.what, a.width, a.height, a.frame_begin, a.frame_count, a.stripe_rows, a.n_ranks, a.rank, npix64)))
        return rc;
    const uint32_t npix = (uint32_t)npix64;
    if (c.kind.list && c.num_listed > npix) return fail(PT_ERR_INVALID, "%u pixels listed, the local image has %u", c.num_listed, npix);
    const uint32_t wpix = c.kind.list ? c.num_listed : npix;   // the pixels (the rays) of one frame of the workspace
    const size_t frame_bytes = (size_t)wpix * 12;
    // the spans, group by group: what every kind uses; the counts; the table; the list.  With no lights none of the light buffers is
    // read.  The workspace must hold one frame, and ALL of it must lie apart from the rest: a chunk may fill it
    const bool lit = a.num_lights > 0;
    const PtSpan M = { materials, (size_t)a.num_materials * sizeof(PtRawMaterial), 1, "the material buffer" },
                 L = { lights, (size_t)a.num_lights * sizeof(int32_t), 4, "the light list" },
                 S = { samples, frame_bytes, 4, "the sample workspace" }, W = { samples, samples->bytes, 4, "the sample workspace" },
                 F = { framebuffer, (size_t)npix * sizeof(float4), 16, "the framebuffer" },
                 N = { mis && lit ? light_counts : nullptr, (size_t)a.num_triangles * sizeof(int32_t), 4, "the light-count buffer" },
                 Q = { power && lit ? cdf : nullptr, ((size_t)a.num_lights + 1) * sizeof(uint64_t), 8, "the light table's cdf" },
                 T = { power && lit ? tri_q : nullptr, (size_t)a.num_triangles * sizeof(uint32_t), 4, "the light table's tri_q" },
                 P = { c.kind.list ? list : nullptr, 16 + (size_t)c.num_listed * sizeof(pt_pixel_slot), 8, "the pixel list" };
    if ((rc = check_triangles(triangles, a.num_triangles)) || (rc = span_fits(M)) || (rc = span_fits(L)) || (rc = span_fits(S)) || (rc = span_fits(F))) return rc;
    if ((rc = span_aligned(S)) || (rc = span_aligned(F)) || (lit && (rc = span_aligned(L))) || (rc = spans_apart({ W, F, L }))) return rc;
    if ((rc = span_fits(N)) || (rc = span_aligned(N)) || (rc = spans_apart({ N, W, F, L }))) return rc;
    if ((rc = span_fits(Q)) || (rc = span_fits(T)) || (rc = span_aligned(Q)) || (T.bytes && (rc = span_aligned(T))) || (rc = spans_apart({ Q, T, W, F, L, N }))) return rc;
    if ((rc = span_fits(P)) || (rc = span_aligned(P)) || (rc = spans_apart({ P, W, F }))) return rc;
    // the rays and the moments (from_rays).  Without moments nothing consumes a chunk before the next overwrites it: the workspace
    // must then hold every sample of the call
    const PtSpan Y = { rays ? c.rays : nullptr, (size_t)wpix * sizeof(pt_ray), 16, "the ray buffer" },
                 Z = { rays ? c.moments : nullptr, (size_t)wpix * sizeof(pt_pixel_moments), 8, "the moment buffer" };
    if ((rc = span_fits(Y)) || (rc = span_fits(Z))) return rc;
    if (rays && !c.moments && frame_bytes && (size_t)a.frame_count > samples->bytes / frame_bytes)   // (a quotient: the product may not fit a size_t)
        return fail(PT_ERR_RANGE, "the sample workspace holds %zu bytes, %d samples of %u rays without moments need more", samples->bytes, a.frame_count, wpix);
    if ((rc = span_aligned(Y)) || (rc = span_aligned(Z)) || (rc = spans_apart({ Y, Z, W }, { L, N, Q, T }))) return rc;
    // the map and its table (kind.env): read only, so they must lie apart from what is written; the table is not read when Ke = 0
    const size_t texels = c.kind.env ? (size_t)c.e.size * (size_t)c.e.size : 0;
    const PtSpan E = { c.kind.env ? c.env : nullptr, texels * sizeof(float4), 16, "the environment map" },
                 C = { c.kind.env && c.e.env_samples > 0 ? c.env_cdf : nullptr, (texels + 1) * sizeof(uint64_t), 8, "the environment table's cdf" };
    if ((rc = span_fits(E)) || (rc = span_fits(C)) || (rc = span_aligned(E)) || (rc = span_aligned(C)) || (rc = spans_apart({ E, C, W, F, L, N, Q, T }))) return rc;
    // a search that was cut short earlier is reported before anything new is enqueued (PT_ERR_TRAVERSAL is deferred)
    if ((rc = check_traversal(d))) return rc;
    if ((rc = enter_stream(d))) return rc;
    if (a.frame_count == 0 || wpix == 0) {   // (no local pixel: none listed)
        if ((rc = event_begin(d, c.ev))) return rc;
        return event_end(d, c.ev);
    }
    PtSearch search;
    if ((rc = prepare_search(d, triangles, a.num_triangles, nullptr, search))) return rc;
    if ((rc = event_begin(d, c.ev))) return rc;
    PtLitParams ip;   // (every kind's block is a base of it, or made of it: ptk_lit)
    memset(&ip, 0, sizeof ip);
    if (c.kind.env) {
        ip.env.texels = (const float4*)c.env->dptr;
        ip.env.cdf = C.buf ? (const uint64_t*)c.env_cdf->dptr : nullptr;
        ip.env.N = c.e.size;
        ip.env.Ke = c.e.env_samples;
    }
    ip.M = c.candidates;       // (zero without resampling)
    ip.B = c.max_bounces;
    ip.R = c.rr.first_bounce;   // (zeros without roulette)
    ip.cap = c.rr.max_survival;
    PtDirectParams& p = ip.d;
    search_fields(d, search, p.t);   // (an empty scene: the brute-force form over zero triangles, every sample the background)
    if (!rays) image_geometry(p.t, a.width, a.height, a.stripe_rows, a.n_ranks, a.rank, npix);   // (a ray launch reads no image field)
    p.t.mats = (const PtRawMaterial*)materials->dptr;
    p.t.nmat = a.num_materials;
    p.cam = cam;
    p.lights = lit ? (const int32_t*)lights->dptr : nullptr;
    p.samples = (float*)samples->dptr;
    p.npix = wpix;
    p.K = a.light_samples;
    p.nl = a.num_lights;
    ip.counts = N.buf ? (const int32_t*)light_counts->dptr : nullptr;
    ip.cdf = Q.buf ? (const uint64_t*)cdf->dptr : nullptr;
    ip.tri_q = T.buf ? (const uint32_t*)tri_q->dptr : nullptr;
    ip.slots = P.buf ? reinterpret_cast<const uint2*>(static_cast<const char*>(list->dptr) + 16) : nullptr;
    ip.rays = Y.buf ? (const float4*)c.rays->dptr : nullptr;
    ip.first_ray = c.first_ray;
    PtFoldParams fp;
    memset(&fp, 0, sizeof fp);
    fp.rad = p.samples;
    fp.fb = framebuffer ? (float4*)framebuffer->dptr : nullptr;
    fp.npix_local = npix;
    PtFoldListParams lp;
    memset(&lp, 0, sizeof lp);
    lp.rad = p.samples;
    lp.fb = fp.fb;
    lp.slots = ip.slots;
    lp.num_listed = wpix;
    lp.npix_local = npix;
    // each kind's LBVH kernel on its own grid (pt_kernels.h)
    const unsigned kind = ptk_lit_kind(c.kind, rays);
    const int bvh_blocks = !search.mode.bvh ? 0 : d->prop.multiProcessorCount * d->lit_bvh_blocks_per_cu[kind];
    // whole frames per chunk: what the workspace holds, fewer than 2^31 samples per launch; a launch, then its fold
    const int64_t per_chunk = (int64_t)std::min<uint64_t>(samples->bytes / frame_bytes, 0x7fffffffu / wpix);
    for (int64_t done = 0; done < a.frame_count; done += per_chunk) {
        const int nf = (int)std::min<int64_t>(per_chunk, a.frame_count - done);
        p.frame0 = fp.frame_begin = a.frame_begin + (int)done;
        p.nitems = (uint32_t)nf * wpix;
        fp.frame_count = lp.frame_count = nf;
        // a list: every slot continues from its own frame -- the call's offset, then the frames of the chunks before (no other kind's block holds it)
        ip.frame_off = lp.frame_off = (uint32_t)p.frame0;
        HIP_TRY(ptk_lit(ip, kind, bvh_blocks, search.mode, d->stream));
        // the rays: no fold -- the chunk's moments, in ascending sample order, from zeros at the call's first chunk when it says so
        if (rays) {
            if (c.moments) HIP_TRY(ptk_sample_moments(p.samples, (PtPixelMoments*)c.moments->dptr, wpix, nf, c.reset != 0 && done == 0, d->stream));
        } else
            HIP_TRY(c.kind.list ? ptk_fold_list(lp, d->stream) : ptk_fold(fp, d->stream));
    }
    samples->version++;
    if (framebuffer) framebuffer->version++;
    if (rays && c.moments) c.moments->version++;
    return event_end(d, c.ev);
}

// what the direct entry points check of their block, and what the indirect ones do -- both after use_device --: the block pointer,
// max_bounces, the reserved fields; the shared fields go to c.a
static int direct_block(const pt_direct_params* params, PtLitCall& c)
{
    if (!params) return fail(PT_ERR_INVALID, "params == NULL");
    c.a = *params;
    for (int i = 0; i < 5; ++i)
        if (c.a.reserved[i] != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    return PT_OK;
}
static int indirect_block(const pt_indirect_params* params, PtLitCall& c)
{
    if (!params) return fail(PT_ERR_INVALID, "params == NULL");
    const pt_indirect_params b = *params;
    if (b.max_bounces < 1 || b.max_bounces > 65535) return fail(PT_ERR_INVALID, "max_bounces must lie in 1..65535");
    for (int i = 0; i < 4; ++i)
        if (b.reserved[i] != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    pt_direct_params& a = c.a;   // (zeros: lit_call)
    a.width = b.width; a.height = b.height; a.frame_begin = b.frame_begin; a.frame_count = b.frame_count;
    a.num_triangles = b.num_triangles; a.num_materials = b.num_materials; a.num_lights = b.num_lights;
    a.light_samples = b.light_samples;
    a.stripe_rows = b.stripe_rows; a.n_ranks = b.n_ranks; a.rank = b.rank;
    c.max_bounces = b.max_bounces;
    return PT_OK;
}
// what pt_render_indirect_rr and pt_render_indirect_pixels check before anything else: mis, the roulette, the table's two halves
static int roulette_args(int mis, const pt_roulette* roulette, pt_buffer_t cdf, pt_buffer_t tri_q, const pt_indirect_params* params, PtLitCall& c)
{
    if (mis != 0 && mis != 1) return fail(PT_ERR_INVALID, "mis must be 0 or 1");
    if (!roulette) return fail(PT_ERR_INVALID, "roulette == NULL");
    c.rr = *roulette;
    if (c.rr.first_bounce < 1) return fail(PT_ERR_INVALID, "first_bounce must be at least 1");
    if (!(c.rr.max_survival > 0.0f && c.rr.max_survival <= 1.0f)) return fail(PT_ERR_INVALID, "max_survival must lie in (0, 1]");   // (false for NaN)
    if (c.rr.reserved[0] != 0 || c.rr.reserved[1] != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    if (params && params->num_lights > 0 && (cdf || tri_q) && !(cdf && tri_q))
        return fail(PT_ERR_INVALID, "the light table is cdf AND tri_q (pt_light_table), or neither for the uniform choice");
    return PT_OK;
}

extern "C" int pt_render_direct(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, pt_buffer_t samples,
                                pt_buffer_t framebuffer, const pt_direct_params* params, const pt_camera* cam, pt_event_t ev)
{
    PtLitKind k = {};
    PtLitCall c = lit_call(k, triangles, materials, lights, nullptr, nullptr, nullptr, samples, framebuffer, cam, ev);
    int rc = use_device(d);
    if (rc || (rc = direct_block(params, c))) return rc;
    return render_lit(d, c);
}

// ---- first-hit feature buffers (include/pt_shim.h) -----------------------------------------------------------------------------
static_assert(sizeof(pt_feature_params) == 64, "pt_feature_params layout");

extern "C" int pt_render_features(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t albedo, pt_buffer_t normal,
                                  pt_buffer_t depth, pt_buffer_t emission, const pt_feature_params* params, const pt_camera* cam, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!params) return fail(PT_ERR_INVALID, "params == NULL");
    const pt_feature_params a = *params;
    PtLensCamera c = reference_camera();
    if (cam && (rc = camera_derive(cam, &c))) return rc;
    if (!triangles || !materials) return fail(PT_ERR_INVALID, "null buffer handle");
    if (!albedo && !normal && !depth && !emission) return fail(PT_ERR_INVALID, "at least one of the four outputs must be given");
    if ((rc = check_same_device(d, { triangles, materials, albedo, normal, depth, emission })) || (rc = check_event(d, ev))) return rc;
    if (a.num_triangles < 0 || a.num_materials < 1) return fail(PT_ERR_INVALID, "invalid feature parameters");
    for (int i = 0; i < 7; ++i)
        if (a.reserved[i] != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    // the hit's {n, id} and its material are gathered by 32-bit byte offsets into the 64-byte records, as shading gathers them
    if ((uint64_t)a.num_triangles * 64u > 0xffffffffull || (uint64_t)a.num_materials * 64u > 0xffffffffull)
        return fail(PT_ERR_INVALID, "a scene has fewer than 2^26 triangles and 2^26 materials");
    uint64_t npix64;
    if ((rc = check_image("invalid feature parameters", a.width, a.height, a.frame_begin, a.frame_count, a.stripe_rows, a.n_ranks, a.rank, npix64)))
        return rc;
    const uint32_t npix = (uint32_t)npix64;
    // one launch, frame-major samples: fewer than 2^31 of them
    const uint64_t items = (uint64_t)a.frame_count * npix;
    if (items > 0x7fffffffull) return fail(PT_ERR_RANGE, "frame_count x local pixels = %llu samples: at most 2^31 - 1 per call", (unsigned long long)items);
    const size_t out_bytes = (size_t)items * 12;
    const PtSpan R = { triangles, (size_t)a.num_triangles * sizeof(PtRawTriangle), 1, "the triangle buffer" },
                 M = { materials, (size_t)a.num_materials * sizeof(PtRawMaterial), 1, "the material buffer" },
                 A = { albedo, out_bytes, 4, "the albedo buffer" }, N = { normal, out_bytes, 4, "the normal buffer" },
                 D = { depth, out_bytes, 4, "the depth buffer" }, E = { emission, out_bytes, 4, "the emission buffer" };
    if ((rc = check_triangles(triangles, a.num_triangles)) || (rc = span_fits(M))) return rc;
    if ((rc = span_fits(A)) || (rc = span_fits(N)) || (rc = span_fits(D)) || (rc = span_fits(E))) return rc;
    if ((rc = span_aligned(A)) || (rc = span_aligned(N)) || (rc = span_aligned(D)) || (rc = span_aligned(E))) return rc;
    if ((rc = spans_apart({ A, N, D, E }, { R, M }))) return rc;   // (the scene is only read)
    // a search that was cut short earlier is reported before anything new is enqueued (PT_ERR_TRAVERSAL is deferred)
    if ((rc = check_traversal(d))) return rc;
    if ((rc = enter_stream(d))) return rc;
    if (items == 0) {
        if ((rc = event_begin(d, ev))) return rc;
        return event_end(d, ev);
    }
    PtSearch search;
    if ((rc = prepare_search(d, triangles, a.num_triangles, nullptr, search))) return rc;
    if ((rc = event_begin(d, ev))) return rc;
    PtFeatureParams p;
    memset(&p, 0, sizeof p);
    search_fields(d, search, p.d.t);   // (an empty scene: the brute-force form over zero triangles, every sample a miss)
    image_geometry(p.d.t, a.width, a.height, a.stripe_rows, a.n_ranks, a.rank, npix);
    p.d.t.mats = (const PtRawMaterial*)materials->dptr;
    p.d.t.nmat = a.num_materials;
    p.d.cam = c;
    p.d.npix = npix;
    p.d.nitems = (uint32_t)items;
    p.d.frame0 = a.frame_begin;
    p.albedo = albedo ? (float*)albedo->dptr : nullptr;
    p.normal = normal ? (float*)normal->dptr : nullptr;
    p.depth = depth ? (float*)depth->dptr : nullptr;
    p.emission = emission ? (float*)emission->dptr : nullptr;
    HIP_TRY(ptk_render_features(p, search.driver_blocks, search.mode, d->stream));
    for (pt_buffer_t b : { albedo, normal, depth, emission })
        if (b) b->version++;
    return event_end(d, ev);
}

// ---- indirect illumination (include/pt_shim.h) ---------------------------------------------------------------------------------
extern "C" int pt_render_indirect(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, pt_buffer_t samples,
                                  pt_buffer_t framebuffer, const pt_indirect_params* params, const pt_camera* cam, pt_event_t ev)
{
    PtLitKind k = {}; k.indirect = true;
    PtLitCall c = lit_call(k, triangles, materials, lights, nullptr, nullptr, nullptr, samples, framebuffer, cam, ev);
    int rc = use_device(d);
    if (rc || (rc = indirect_block(params, c))) return rc;
    return render_lit(d, c);
}

extern "C" int pt_render_indirect_mis(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, pt_buffer_t light_counts,
                                      pt_buffer_t samples, pt_buffer_t framebuffer, const pt_indirect_params* params, const pt_camera* cam,
                                      pt_event_t ev)
{
    PtLitKind k = {}; k.indirect = k.mis = true;
    PtLitCall c = lit_call(k, triangles, materials, lights, light_counts, nullptr, nullptr, samples, framebuffer, cam, ev);
    int rc = use_device(d);
    if (rc || (rc = indirect_block(params, c))) return rc;
    return render_lit(d, c);
}

// ---- light choice by power (include/pt_shim.h) -----------------------------------------------------------------------------------
extern "C" int pt_render_direct_power(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, pt_buffer_t cdf,
                                      pt_buffer_t tri_q, pt_buffer_t samples, pt_buffer_t framebuffer, const pt_direct_params* params,
                                      const pt_camera* cam, pt_event_t ev)
{
    PtLitKind k = {}; k.power = true;
    PtLitCall c = lit_call(k, triangles, materials, lights, nullptr, cdf, tri_q, samples, framebuffer, cam, ev);
    int rc = use_device(d);
    if (rc || (rc = direct_block(params, c))) return rc;
    return render_lit(d, c);
}

extern "C" int pt_render_indirect_power(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, int mis,
                                        pt_buffer_t light_counts, pt_buffer_t cdf, pt_buffer_t tri_q, pt_buffer_t samples,
                                        pt_buffer_t framebuffer, const pt_indirect_params* params, const pt_camera* cam, pt_event_t ev)
{
    if (mis != 0 && mis != 1) return fail(PT_ERR_INVALID, "mis must be 0 or 1");
    PtLitKind k = {}; k.indirect = k.power = true; k.mis = mis != 0;
    PtLitCall c = lit_call(k, triangles, materials, lights, light_counts, cdf, tri_q, samples, framebuffer, cam, ev);
    int rc = use_device(d);
    if (rc || (rc = indirect_block(params, c))) return rc;
    return render_lit(d, c);
}

// ---- Russian roulette and adaptive sampling (include/pt_shim.h) --------------------------------------------------------------------
// (cdf and tri_q both NULL: the uniform choice)
extern "C" int pt_render_indirect_rr(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, int mis,
                                     pt_buffer_t light_counts, pt_buffer_t cdf, pt_buffer_t tri_q, pt_buffer_t samples, pt_buffer_t framebuffer,
                                     const pt_indirect_params* params, const pt_roulette* roulette, const pt_camera* cam, pt_event_t ev)
{
    PtLitKind k = {}; k.indirect = k.rr = true; k.mis = mis != 0; k.power = cdf || tri_q;
    PtLitCall c = lit_call(k, triangles, materials, lights, light_counts, cdf, tri_q, samples, framebuffer, cam, ev);
    int rc = roulette_args(mis, roulette, cdf, tri_q, params, c);
    if (rc || (rc = use_device(d)) || (rc = indirect_block(params, c))) return rc;
    return render_lit(d, c);
}

extern "C" int pt_render_indirect_pixels(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, int mis,
                                         pt_buffer_t light_counts, pt_buffer_t cdf, pt_buffer_t tri_q, pt_buffer_t samples, pt_buffer_t framebuffer,
                                         pt_buffer_t list, uint32_t num_listed, const pt_indirect_params* params, const pt_roulette* roulette,
                                         const pt_camera* cam, pt_event_t ev)
{
    PtLitKind k = {}; k.indirect = k.rr = k.list = true; k.mis = mis != 0; k.power = cdf || tri_q;
    PtLitCall c = lit_call(k, triangles, materials, lights, light_counts, cdf, tri_q, samples, framebuffer, cam, ev);
    c.list = list; c.num_listed = num_listed;
    int rc = roulette_args(mis, roulette, cdf, tri_q, params, c);
    if (rc || (rc = use_device(d)) || (rc = indirect_block(params, c))) return rc;
    return render_lit(d, c);
}

// ---- radiance queries (include/pt_shim.h) ------------------------------------------------------------------------------------------
static_assert(sizeof(pt_radiance_params) == 64, "pt_radiance_params layout");

// pt_render_indirect_rr's call with the caller's rays in place of the image: the ray count stands where the local pixels stand and
// the sample range where the frames stand (render_lit, from_rays)
extern "C" int pt_radiance_rays(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, int mis,
                                pt_buffer_t light_counts, pt_buffer_t cdf, pt_buffer_t tri_q, pt_buffer_t rays, pt_buffer_t samples,
                                pt_buffer_t moments, const pt_radiance_params* params, const pt_roulette* roulette, pt_event_t ev)
{
    PtLitKind k = {}; k.indirect = k.rr = true; k.mis = mis != 0; k.power = cdf || tri_q;
    PtLitCall c = lit_call(k, triangles, materials, lights, light_counts, cdf, tri_q, samples, nullptr, nullptr, ev);
    c.from_rays = true;
    c.what = "invalid radiance-query parameters";
    c.rays = rays; c.moments = moments;
    if (!params) return fail(PT_ERR_INVALID, "params == NULL");
    const pt_radiance_params b = *params;
    pt_indirect_params ib;   // the fields roulette_args and the parents' checks read
    memset(&ib, 0, sizeof ib);
    ib.num_lights = b.num_lights;
    int rc = roulette_args(mis, roulette, cdf, tri_q, &ib, c);
    if (rc || (rc = use_device(d))) return rc;
    if (b.max_bounces < 1 || b.max_bounces > 65535) return fail(PT_ERR_INVALID, "max_bounces must lie in 1..65535");
    for (int i = 0; i < 6; ++i)
        if (b.reserved[i] != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    pt_direct_params& a = c.a;   // (zeros: lit_call; the image fields stay zero and are not read)
    a.frame_begin = b.sample_begin; a.frame_count = b.sample_count;
    a.num_triangles = b.num_triangles; a.num_materials = b.num_materials; a.num_lights = b.num_lights;
    a.light_samples = b.light_samples;
    c.max_bounces = b.max_bounces;
    c.num_rays = b.num_rays; c.first_ray = b.first_ray;
    c.reset = b.reset;
    return render_lit(d, c);
}

// ---- resampled light sampling (include/pt_shim.h) ----------------------------------------------------------------------------------
// what the three _ris entry points check before anything else: the block, M, the reserved words, the table (there is no uniform form)
static int ris_args(const pt_ris* ris, pt_buffer_t cdf, pt_buffer_t tri_q, int num_lights, PtLitCall& c)
{
    if (!ris) return fail(PT_ERR_INVALID, "ris == NULL");
    const pt_ris r = *ris;
    if (r.candidates < 1 || r.candidates > 32) return fail(PT_ERR_INVALID, "candidates must lie in 1..32");
    if (r.reserved[0] != 0 || r.reserved[1] != 0 || r.reserved[2] != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    if (num_lights > 0 && !(cdf && tri_q)) return fail(PT_ERR_INVALID, "resampling needs the light table: cdf AND tri_q (pt_light_table)");
    c.candidates = r.candidates;
    return PT_OK;
}

extern "C" int pt_render_direct_ris(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, pt_buffer_t cdf,
                                    pt_buffer_t tri_q, pt_buffer_t samples, pt_buffer_t framebuffer, const pt_direct_params* params,
                                    const pt_ris* ris, const pt_camera* cam, pt_event_t ev)
{
    PtLitKind k = {}; k.power = k.ris = true;
    PtLitCall c = lit_call(k, triangles, materials, lights, nullptr, cdf, tri_q, samples, framebuffer, cam, ev);
    int rc = ris_args(ris, cdf, tri_q, params ? params->num_lights : 0, c);
    if (rc || (rc = use_device(d)) || (rc = direct_block(params, c))) return rc;
    return render_lit(d, c);
}

extern "C" int pt_render_indirect_ris(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, int mis,
                                      pt_buffer_t light_counts, pt_buffer_t cdf, pt_buffer_t tri_q, pt_buffer_t samples, pt_buffer_t framebuffer,
                                      const pt_indirect_params* params, const pt_roulette* roulette, const pt_ris* ris, const pt_camera* cam,
                                      pt_event_t ev)
{
    PtLitKind k = {}; k.indirect = k.rr = k.power = k.ris = true; k.mis = mis != 0;
    PtLitCall c = lit_call(k, triangles, materials, lights, light_counts, cdf, tri_q, samples, framebuffer, cam, ev);
    int rc = roulette_args(mis, roulette, cdf, tri_q, params, c);
    if (rc || (rc = ris_args(ris, cdf, tri_q, params ? params->num_lights : 0, c)) || (rc = use_device(d)) || (rc = indirect_block(params, c))) return rc;
    return render_lit(d, c);
}

extern "C" int pt_render_indirect_pixels_ris(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, int mis,
                                             pt_buffer_t light_counts, pt_buffer_t cdf, pt_buffer_t tri_q, pt_buffer_t samples,
                                             pt_buffer_t framebuffer, pt_buffer_t list, uint32_t num_listed, const pt_indirect_params* params,
                                             const pt_roulette* roulette, const pt_ris* ris, const pt_camera* cam, pt_event_t ev)
{
    PtLitKind k = {}; k.indirect = k.rr = k.list = k.power = k.ris = true; k.mis = mis != 0;
    PtLitCall c = lit_call(k, triangles, materials, lights, light_counts, cdf, tri_q, samples, framebuffer, cam, ev);
    c.list = list; c.num_listed = num_listed;
    int rc = roulette_args(mis, roulette, cdf, tri_q, params, c);
    if (rc || (rc = ris_args(ris, cdf, tri_q, params ? params->num_lights : 0, c)) || (rc = use_device(d)) || (rc = indirect_block(params, c))) return rc;
    return render_lit(d, c);
}

// ---- environment lighting (include/pt_shim.h) ----------------------------------------------------------------------------------------
static bool env_size_valid(int N) { return N >= 1 && N <= PT_ENV_SIZE_MAX && (N & (N - 1)) == 0; }

// what the two _env entry points check before anything else: the block, N, Ke, the reserved words, the map, the table when it is read
static int env_args(const pt_environment* environment, pt_buffer_t env, pt_buffer_t env_cdf, PtLitCall& c)
{
    if (!environment) return fail(PT_ERR_INVALID, "environment == NULL");
    c.e = *environment;
    if (!env_size_valid(c.e.size)) return fail(PT_ERR_INVALID, "the map's size must be a power of two in 1..%d", PT_ENV_SIZE_MAX);
    if (c.e.env_samples < 0 || c.e.env_samples > 256) return fail(PT_ERR_INVALID, "env_samples must lie in 0..256");
    if (c.e.reserved[0] != 0 || c.e.reserved[1] != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    if (!env) return fail(PT_ERR_INVALID, "the environment map is NULL");
    if (c.e.env_samples > 0 && !env_cdf) return fail(PT_ERR_INVALID, "env_samples > 0 needs the environment table (pt_env_table)");
    c.env = env; c.env_cdf = env_cdf;
    return PT_OK;
}

extern "C" int pt_render_direct_env(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, pt_buffer_t cdf,
                                    pt_buffer_t tri_q, pt_buffer_t env, pt_buffer_t env_cdf, pt_buffer_t samples, pt_buffer_t framebuffer,
                                    const pt_direct_params* params, const pt_environment* environment, const pt_camera* cam, pt_event_t ev)
{
    PtLitKind k = {}; k.power = k.env = true;
    PtLitCall c = lit_call(k, triangles, materials, lights, nullptr, cdf, tri_q, samples, framebuffer, cam, ev);
    int rc = env_args(environment, env, env_cdf, c);
    if (rc || (rc = use_device(d)) || (rc = direct_block(params, c))) return rc;
    return render_lit(d, c);
}

extern "C" int pt_render_indirect_env(pt_device_t d, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t lights, pt_buffer_t light_counts,
                                      pt_buffer_t cdf, pt_buffer_t tri_q, pt_buffer_t env, pt_buffer_t env_cdf, pt_buffer_t samples,
                                      pt_buffer_t framebuffer, const pt_indirect_params* params, const pt_roulette* roulette,
                                      const pt_environment* environment, const pt_camera* cam, pt_event_t ev)
{
    PtLitKind k = {}; k.indirect = k.mis = k.rr = k.power = k.env = true;
    PtLitCall c = lit_call(k, triangles, materials, lights, light_counts, cdf, tri_q, samples, framebuffer, cam, ev);
    int rc = roulette_args(1, roulette, cdf, tri_q, params, c);
    if (rc || (rc = env_args(environment, env, env_cdf, c)) || (rc = use_device(d)) || (rc = indirect_block(params, c))) return rc;
    return render_lit(d, c);
}

extern "C" size_t pt_env_table_bytes(int N) { return env_size_valid(N) ? PT_LIGHT_TABLE_WORDS((size_t)N * (size_t)N) * sizeof(uint64_t) : 0; }

extern "C" int pt_env_table(pt_device_t d, pt_buffer_t env, int N, pt_buffer_t cdf, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!env || !cdf) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { env, cdf })) || (rc = check_event(d, ev))) return rc;
    if (!env_size_valid(N)) return fail(PT_ERR_INVALID, "the map's size must be a power of two in 1..%d", PT_ENV_SIZE_MAX);
    const PtSpan E = { env, (size_t)N * (size_t)N * sizeof(float4), 16, "the environment map" },
                 Q = { cdf, pt_env_table_bytes(N), 8, "the environment table's cdf (pt_env_table_bytes)" };
    if ((rc = span_fits(E)) || (rc = span_fits(Q)) || (rc = span_aligned(E)) || (rc = span_aligned(Q)) || (rc = spans_apart({ Q }, { E }))) return rc;
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_env_table((const float4*)env->dptr, N, (uint64_t*)cdf->dptr, d->stream));
    cdf->version++;
    return event_end(d, ev);
}

extern "C" size_t pt_adaptive_list_bytes(uint32_t num_pixels) { return PT_ADAPTIVE_LIST_BYTES(num_pixels); }

extern "C" int pt_adaptive_select(pt_device_t d, pt_buffer_t moments, uint32_t num_pixels, const pt_adaptive_rule* rule, pt_buffer_t list, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!moments || !list) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { moments, list })) || (rc = check_event(d, ev))) return rc;
    if (!rule) return fail(PT_ERR_INVALID, "rule == NULL");
    const pt_adaptive_rule r = *rule;
    if (!(r.tol2 >= 0.0) || !(r.floor2 >= 0.0)) return fail(PT_ERR_INVALID, "tol2 and floor2 must not be negative or NaN");
    if (r.reserved[0] != 0 || r.reserved[1] != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    const PtSpan M = { moments, (size_t)num_pixels * sizeof(pt_pixel_moments), 8, "the moment buffer" },
                 P = { list, pt_adaptive_list_bytes(num_pixels), 8, "the pixel list (pt_adaptive_list_bytes)" };
    if ((rc = span_fits(M)) || (rc = span_fits(P)) || (rc = span_aligned(M)) || (rc = span_aligned(P)) || (rc = spans_apart({ M, P }))) return rc;
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    const PtAdaptiveRule k = { r.tol2, r.floor2, r.min_samples, r.max_samples };
    HIP_TRY(ptk_adaptive_select((const PtPixelMoments*)moments->dptr, num_pixels, k, list->dptr, d->stream));
    list->version++;
    return event_end(d, ev);
}

extern "C" int pt_sample_moments_pixels(pt_device_t d, pt_buffer_t samples, pt_buffer_t moments, pt_buffer_t list, uint32_t num_listed,
                                        int32_t frame_count, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!samples || !moments || !list) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { samples, moments, list })) || (rc = check_event(d, ev))) return rc;
    if (frame_count < 0) return fail(PT_ERR_INVALID, "frame_count < 0");
    // the local pixels: the whole records the moments buffer holds
    const size_t records = std::min<size_t>(moments->bytes / sizeof(pt_pixel_moments), 0xffffffffu);
    if ((size_t)num_listed > records) return fail(PT_ERR_INVALID, "%u pixels listed, the moments hold %zu records", num_listed, records);
    const size_t frame_bytes = (size_t)num_listed * 3u * sizeof(float);
    if (frame_bytes && (size_t)frame_count > samples->bytes / frame_bytes)   // (a quotient: the product may not fit a size_t)
        return fail(PT_ERR_RANGE, "sample buffer holds %zu bytes, %d frames of %u pixels need more", samples->bytes, frame_count, num_listed);
    const PtSpan S = { samples, frame_bytes * (size_t)frame_count, 4, "the sample buffer" }, M = { moments, records * sizeof(pt_pixel_moments), 8, "the moment buffer" },
                 P = { list, 16 + (size_t)num_listed * sizeof(pt_pixel_slot), 8, "the pixel list" };
    if ((rc = span_fits(P)) || (rc = span_aligned(M)) || (rc = span_aligned(S)) || (rc = span_aligned(P)) || (rc = spans_apart({ S, M, P }))) return rc;
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    if (num_listed && frame_count) {
        HIP_TRY(ptk_sample_moments_list((const float*)samples->dptr, (PtPixelMoments*)moments->dptr,
                                        reinterpret_cast<const uint2*>(static_cast<const char*>(list->dptr) + 16), num_listed, (uint32_t)records,
                                        frame_count, d->stream));
        moments->version++;
    }
    return event_end(d, ev);
}

extern "C" size_t pt_light_table_bytes(int num_lights)
{
    return num_lights < 0 || num_lights >= (1 << 24) ? 0 : PT_LIGHT_TABLE_WORDS(num_lights) * sizeof(uint64_t);
}

extern "C" int pt_light_table(pt_device_t d, pt_buffer_t triangles, int num_triangles, pt_buffer_t materials, int num_materials,
                              pt_buffer_t lights, int num_lights, pt_buffer_t cdf, pt_buffer_t tri_q, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!triangles || !materials || !cdf || !tri_q) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { triangles, materials, lights, cdf, tri_q })) || (rc = check_event(d, ev))) return rc;
    if (num_lights < 0 || num_triangles < 0 || num_materials < 1) return fail(PT_ERR_INVALID, "invalid light-table parameters");
    if (num_lights >= (1 << 24)) return fail(PT_ERR_INVALID, "num_lights must stay below 2^24 (its float32 value must be exact)");
    if (num_lights > 0 && !lights) return fail(PT_ERR_INVALID, "num_lights > 0 needs a light list");
    const PtSpan R = { triangles, (size_t)num_triangles * sizeof(PtRawTriangle), 1, "the triangle buffer" },
                 M = { materials, (size_t)num_materials * sizeof(PtRawMaterial), 1, "the material buffer" },
                 L = { lights, (size_t)num_lights * sizeof(int32_t), 4, "the light list" },
                 Q = { cdf, pt_light_table_bytes(num_lights), 8, "the light table's cdf (pt_light_table_bytes)" },
                 T = { tri_q, (size_t)num_triangles * sizeof(uint32_t), 4, "the light table's tri_q" };
    if ((rc = span_fits(R)) || (rc = span_fits(M)) || (rc = span_fits(L)) || (rc = span_fits(Q)) || (rc = span_fits(T))) return rc;
    if ((rc = span_aligned(Q)) || (T.bytes && (rc = span_aligned(T))) || (num_lights > 0 && (rc = span_aligned(L)))) return rc;
    if ((rc = spans_apart({ Q, T }, { R, M, L }))) return rc;   // (the inputs are only read)
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_light_table((const PtRawTriangle*)triangles->dptr, num_triangles, (const PtRawMaterial*)materials->dptr, num_materials,
                            num_lights > 0 ? (const int32_t*)lights->dptr : nullptr, num_lights, (uint64_t*)cdf->dptr, (uint32_t*)tri_q->dptr, d->stream));
    cdf->version++;
    tri_q->version++;
    return event_end(d, ev);
}

extern "C" int pt_light_counts(pt_device_t d, pt_buffer_t lights, int num_lights, int num_triangles, pt_buffer_t counts, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!counts) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { lights, counts })) || (rc = check_event(d, ev))) return rc;
    if (num_lights < 0 || num_triangles < 0) return fail(PT_ERR_INVALID, "invalid light-count parameters");
    if (num_lights >= (1 << 24)) return fail(PT_ERR_INVALID, "num_lights must stay below 2^24 (its float32 value must be exact)");
    if (num_lights > 0 && !lights) return fail(PT_ERR_INVALID, "num_lights > 0 needs a light list");
    const PtSpan L = { lights, (size_t)num_lights * sizeof(int32_t), 4, "the light list" },
                 N = { counts, (size_t)num_triangles * sizeof(int32_t), 4, "the light-count buffer" };
    if ((rc = span_fits(L)) || (rc = span_fits(N)) || (N.bytes && (rc = span_aligned(N))) || (num_lights > 0 && (rc = span_aligned(L))) ||
        (rc = spans_apart({ L, N })))
        return rc;
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_light_counts(num_lights > 0 ? (const int32_t*)lights->dptr : nullptr, num_lights, num_triangles, (int32_t*)counts->dptr, d->stream));
    counts->version++;
    return event_end(d, ev);
}

// ---- sample moments (include/pt_shim.h) ---------------------------------------------------------------------------------
static_assert(sizeof(pt_pixel_moments) == 56 && sizeof(PtPixelMoments) == 56 && sizeof(pt_noise_summary) == 48 && sizeof(PtNoiseSummary) == 48,
              "moment record layout");

extern "C" int pt_sample_moments(pt_device_t d, pt_buffer_t samples, pt_buffer_t moments, uint32_t num_pixels, int32_t frame_count,
                                 int reset, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!samples || !moments) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { samples, moments })) || (rc = check_event(d, ev))) return rc;
    if (frame_count < 0) return fail(PT_ERR_INVALID, "frame_count < 0");
    const size_t frame_bytes = (size_t)num_pixels * 3u * sizeof(float);
    if (frame_bytes && (size_t)frame_count > samples->bytes / frame_bytes)   // (a quotient: the product may not fit a size_t)
        return fail(PT_ERR_RANGE, "sample buffer holds %zu bytes, %d frames of %u pixels need more", samples->bytes, frame_count, num_pixels);
    const PtSpan S = { samples, frame_bytes * (size_t)frame_count, 4, "the sample buffer" },
                 M = { moments, (size_t)num_pixels * sizeof(pt_pixel_moments), 8, "the moment buffer" };
    if ((rc = span_fits(M)) || (rc = span_aligned(M)) || (rc = span_aligned(S)) || (rc = spans_apart({ S, M }))) return rc;
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    if (num_pixels && frame_count) {
        HIP_TRY(ptk_sample_moments((const float*)samples->dptr, (PtPixelMoments*)moments->dptr, num_pixels, frame_count, reset != 0, d->stream));
        moments->version++;
    }
    return event_end(d, ev);
}

extern "C" size_t pt_moments_summary_bytes(uint32_t num_pixels) { return PT_MOMENTS_SUMMARY_RECORDS(num_pixels) * sizeof(pt_noise_summary); }

extern "C" int pt_moments_resolve(pt_device_t d, pt_buffer_t moments, uint32_t num_pixels, pt_buffer_t noise, pt_buffer_t summary, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!moments) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { moments, noise, summary })) || (rc = check_event(d, ev))) return rc;
    const PtSpan M = { moments, (size_t)num_pixels * sizeof(pt_pixel_moments), 8, "the moment buffer" },
                 V = { noise, (size_t)num_pixels * 16u, 16, "the noise map" },
                 U = { summary, pt_moments_summary_bytes(num_pixels), 8, "the summary (pt_moments_summary_bytes)" };
    if ((rc = span_fits(M)) || (rc = span_fits(V)) || (rc = span_fits(U))) return rc;
    if ((rc = span_aligned(M)) || (rc = span_aligned(V)) || (rc = span_aligned(U)) || (rc = spans_apart({ M, V, U }))) return rc;
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    if (num_pixels && (noise || summary)) {
        HIP_TRY(ptk_moments_resolve((const PtPixelMoments*)moments->dptr, num_pixels, noise ? noise->dptr : nullptr,
                                    summary ? (PtNoiseSummary*)summary->dptr : nullptr, d->stream));
        if (noise) noise->version++;
        if (summary) summary->version++;
    }
    return event_end(d, ev);
}

// ---- the denoiser (include/pt_shim.h; kernels: pt_denoise.hip) -------------------------------------------------------------
static_assert(sizeof(pt_denoise_params) == 64, "pt_denoise_params layout");

extern "C" size_t pt_denoise_scratch_bytes(int32_t width, int32_t height)
{
    if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height > 0x7fffffffull) return 0;
    return (size_t)width * (size_t)height * PT_DENOISE_PLANES * sizeof(float4);
}

// pt_denoise (spatial_call false: `spatial` is not looked at) and pt_denoise_spatial: one validation, one enqueue
static int denoise_call(pt_device_t d, pt_buffer_t colour, pt_buffer_t albedo, pt_buffer_t normal, pt_buffer_t depth, pt_buffer_t emission,
                        pt_buffer_t scratch, pt_buffer_t out, const pt_denoise_params* params, bool spatial_call,
                        const pt_denoise_spatial_params* spatial, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!colour || !scratch || !out) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { colour, albedo, normal, depth, emission, scratch, out })) || (rc = check_event(d, ev))) return rc;
    if (!params) return fail(PT_ERR_INVALID, "params == NULL");
    const pt_denoise_params q = *params;
    const size_t scratch_bytes = pt_denoise_scratch_bytes(q.width, q.height);
    if (!scratch_bytes) return fail(PT_ERR_INVALID, "invalid image size %d x %d", q.width, q.height);
    if (q.levels < 0 || q.levels > PT_DENOISE_MAX_LEVELS) return fail(PT_ERR_INVALID, "levels must be 0..%d", PT_DENOISE_MAX_LEVELS);
    if (q.normal_squarings < 0 || q.normal_squarings > 8) return fail(PT_ERR_INVALID, "normal_squarings must be 0..8");
    for (float v : { q.sigma_l, q.sigma_z, q.sigma_a, q.sigma_e, q.eps_l, q.eps_z })
        if (!(v > 0.0f) || !std::isfinite(v)) return fail(PT_ERR_INVALID, "every sigma and eps must be finite and > 0");
    for (int32_t r : q.reserved)
        if (r != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    int32_t below = 0;
    if (spatial_call) {
        if (!spatial) return fail(PT_ERR_INVALID, "spatial == NULL");
        if (spatial->below < 0) return fail(PT_ERR_INVALID, "below must be >= 0");
        for (int32_t r : spatial->reserved)
            if (r != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
        below = spatial->below;
    }
    const size_t npix = (size_t)q.width * (size_t)q.height, rec = npix * sizeof(pt_pixel_moments);
    const PtSpan C = { colour, rec, 8, "the colour moments" }, A = { albedo, rec, 8, "the albedo moments" }, N = { normal, rec, 8, "the normal moments" },
                 Z = { depth, rec, 8, "the depth moments" }, E = { emission, rec, 8, "the emission moments" },
                 S = { scratch, scratch_bytes, 16, "the scratch (pt_denoise_scratch_bytes)" }, O = { out, npix * 16u, 16, "the output" };
    for (const PtSpan& s : { C, A, N, Z, E, S, O })
        if ((rc = span_fits(s))) return rc;
    for (const PtSpan& s : { C, A, N, Z, E, S, O })
        if ((rc = span_aligned(s))) return rc;
    if ((rc = spans_apart({ C, A, N, Z, E, S, O }))) return rc;
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    PtDenoiseArgs a;
    a.width = q.width, a.height = q.height, a.levels = q.levels, a.squarings = q.normal_squarings;
    a.guides = (albedo ? PT_DENOISE_GUIDE_ALBEDO : 0u) | (normal ? PT_DENOISE_GUIDE_NORMAL : 0u) | (depth ? PT_DENOISE_GUIDE_DEPTH : 0u) |
               (emission ? PT_DENOISE_GUIDE_EMISSION : 0u);
    a.sigma_l = q.sigma_l, a.sigma_z = q.sigma_z, a.sigma_a = q.sigma_a, a.sigma_e = q.sigma_e, a.eps_l = q.eps_l, a.eps_z = q.eps_z;
    const void *ca = albedo ? albedo->dptr : nullptr, *cn = normal ? normal->dptr : nullptr, *cz = depth ? depth->dptr : nullptr,
               *ce = emission ? emission->dptr : nullptr;
    if (spatial_call)
        HIP_TRY(ptk_denoise_spatial(colour->dptr, ca, cn, cz, ce, (float4*)scratch->dptr, (float4*)out->dptr, a, below, (int)d->opt_denoise,
                                    (int)d->opt_denoise_spatial, d->stream));
    else
        HIP_TRY(ptk_denoise(colour->dptr, ca, cn, cz, ce, (float4*)scratch->dptr, (float4*)out->dptr, a, (int)d->opt_denoise, d->stream));
    scratch->version++;
    out->version++;
    return event_end(d, ev);
}

extern "C" int pt_denoise(pt_device_t d, pt_buffer_t colour, pt_buffer_t albedo, pt_buffer_t normal, pt_buffer_t depth, pt_buffer_t emission,
                          pt_buffer_t scratch, pt_buffer_t out, const pt_denoise_params* params, pt_event_t ev)
{
    return denoise_call(d, colour, albedo, normal, depth, emission, scratch, out, params, false, nullptr, ev);
}

static_assert(sizeof(pt_denoise_spatial_params) == 32, "pt_denoise_spatial_params layout");

extern "C" int pt_denoise_spatial(pt_device_t d, pt_buffer_t colour, pt_buffer_t albedo, pt_buffer_t normal, pt_buffer_t depth,
                                  pt_buffer_t emission, pt_buffer_t scratch, pt_buffer_t out, const pt_denoise_params* params,
                                  const pt_denoise_spatial_params* spatial, pt_event_t ev)
{
    return denoise_call(d, colour, albedo, normal, depth, emission, scratch, out, params, true, spatial, ev);
}

// ---- temporal reprojection (include/pt_shim.h; kernels: pt_reproject.hip) ----------------------------------------------------
static_assert(sizeof(pt_reproject_params) == 64, "pt_reproject_params layout");

extern "C" size_t pt_reproject_scratch_bytes(int32_t width, int32_t height)
{
    if (width < 1 || height < 1 || (uint64_t)width * (uint64_t)height > 0x7fffffffull) return 0;
    return (size_t)width * (size_t)height * sizeof(float4);
}

static PtReprojectCam reproject_camera(const PtLensCamera& c)
{
    PtReprojectCam r;
    memcpy(r.eye, c.eye, sizeof r.eye);
    memcpy(r.view, c.view, sizeof r.view);
    memcpy(r.hol, c.hol, sizeof r.hol);
    memcpy(r.up, c.up, sizeof r.up);
    r.angle = c.angle;
    return r;
}

extern "C" int pt_reproject(pt_device_t d, pt_buffer_t prev_colour, pt_buffer_t prev_normal, pt_buffer_t prev_depth, pt_buffer_t cur_normal,
                            pt_buffer_t cur_depth, pt_buffer_t scratch, pt_buffer_t out_colour, pt_buffer_t out_info,
                            const pt_reproject_params* params, const pt_camera* prev_cam, const pt_camera* cur_cam, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!prev_colour || !prev_depth || !cur_depth || !scratch || !out_colour) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { prev_colour, prev_normal, prev_depth, cur_normal, cur_depth, scratch, out_colour, out_info })) ||
        (rc = check_event(d, ev)))
        return rc;
    if (!params) return fail(PT_ERR_INVALID, "params == NULL");
    const pt_reproject_params q = *params;
    const size_t scratch_bytes = pt_reproject_scratch_bytes(q.width, q.height);
    if (!scratch_bytes) return fail(PT_ERR_INVALID, "invalid image size %d x %d", q.width, q.height);
    if (q.max_history < 0) return fail(PT_ERR_INVALID, "max_history must be >= 0");
    if (!(q.tol_z > 0.0f) || !std::isfinite(q.tol_z)) return fail(PT_ERR_INVALID, "tol_z must be finite and > 0");
    if (!(q.cos_min >= 0.0f && q.cos_min <= 1.0f)) return fail(PT_ERR_INVALID, "cos_min must lie in [0, 1]");
    if (!(q.min_weight >= 0.0f && q.min_weight < 1.0f)) return fail(PT_ERR_INVALID, "min_weight must lie in [0, 1)");
    if (!(q.max_noise >= 0.0f) || !std::isfinite(q.max_noise)) return fail(PT_ERR_INVALID, "max_noise must be finite and >= 0");
    for (int32_t r : q.reserved)
        if (r != 0) return fail(PT_ERR_INVALID, "reserved fields must be zero");
    if ((prev_normal == nullptr) != (cur_normal == nullptr)) return fail(PT_ERR_INVALID, "the normal test takes both normal buffers or neither");
    PtLensCamera pc = reference_camera(), cc = reference_camera();
    if (prev_cam && (rc = camera_derive(prev_cam, &pc))) return rc;
    if (cur_cam && (rc = camera_derive(cur_cam, &cc))) return rc;
    if (pc.lens_radius > 0.0f || cc.lens_radius > 0.0f) return fail(PT_ERR_INVALID, "pt_reproject takes pinhole cameras: lens_radius must be 0");
    const size_t npix = (size_t)q.width * (size_t)q.height, rec = npix * sizeof(pt_pixel_moments);
    const PtSpan C = { prev_colour, rec, 8, "the previous colour moments" }, PN = { prev_normal, rec, 8, "the previous normal moments" },
                 PD = { prev_depth, rec, 8, "the previous depth moments" }, CN = { cur_normal, rec, 8, "the current normal moments" },
                 CD = { cur_depth, rec, 8, "the current depth moments" },
                 S = { scratch, scratch_bytes, 16, "the scratch (pt_reproject_scratch_bytes)" },
                 O = { out_colour, rec, 8, "the output moments" }, I = { out_info, npix * 16u, 16, "the output info" };
    for (const PtSpan& s : { C, PN, PD, CN, CD, S, O, I })
        if ((rc = span_fits(s))) return rc;
    for (const PtSpan& s : { C, PN, PD, CN, CD, S, O, I })
        if ((rc = span_aligned(s))) return rc;
    if ((rc = spans_apart({ C, PN, PD, CN, CD, S, O, I }))) return rc;
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    PtReprojectArgs a;
    a.width = q.width, a.height = q.height, a.max_history = q.max_history;
    a.tol_z = q.tol_z, a.cos_min2 = q.cos_min * q.cos_min, a.min_weight = q.min_weight;
    a.max_noise = q.max_noise;
    a.inv_width = 1.0f / (float)q.width, a.inv_height = 1.0f / (float)q.height, a.aspect = (float)q.width / (float)q.height;
    a.prev = reproject_camera(pc), a.cur = reproject_camera(cc);
    HIP_TRY(ptk_reproject(prev_colour->dptr, prev_normal ? prev_normal->dptr : nullptr, prev_depth->dptr, cur_normal ? cur_normal->dptr : nullptr,
                          cur_depth->dptr, (float4*)scratch->dptr, out_colour->dptr, out_info ? (float4*)out_info->dptr : nullptr, a,
                          (int)d->opt_reproject, d->stream));
    scratch->version++;
    out_colour->version++;
    if (out_info) out_info->version++;
    return event_end(d, ev);
}

extern "C" int pt_camera_rays(pt_device_t d, const pt_camera* cam, int width, int height, int frame, pt_buffer_t rays, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    PtLensCamera c = reference_camera();
    if (cam && (rc = camera_derive(cam, &c))) return rc;
    if (!rays) return fail(PT_ERR_INVALID, "null buffer handle");
    if ((rc = check_same_device(d, { rays })) || (rc = check_event(d, ev))) return rc;
    uint64_t npix;   // the part of check_image that applies: one frame, no frame range, the whole image as one rank's one stripe
    if ((rc = check_image("invalid image geometry or frame", width, height, frame, /*frame_count*/ 0, /*stripe_rows*/ 1, /*n_ranks*/ 1, /*rank*/ 0, npix)))
        return rc;
    const size_t bytes = (size_t)npix * sizeof(pt_ray);
    if (bytes > rays->bytes) return fail(PT_ERR_RANGE, "ray buffer holds %zu bytes, %d x %d rays need %zu", rays->bytes, width, height, bytes);
    if ((uintptr_t)rays->dptr & 15u) return fail(PT_ERR_INVALID, "the ray buffer must be 16-byte aligned");
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_camera_rays(c, width, height, frame, (float4*)rays->dptr, d->stream));
    rays->version++;
    return event_end(d, ev);
}

static int assemble_check(pt_device_s* d, pt_buffer_s* gathered, pt_buffer_s* image, int width, int height, int stripe_rows, int n_ranks, int slab_rows);

extern "C" int pt_assemble_stripes_on(pt_device_t d, pt_buffer_t gathered, pt_buffer_t image, int width, int height,
                                      int stripe_rows, int n_ranks, int slab_rows, void* hip_stream)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!hip_stream) return fail(PT_ERR_INVALID, "hip_stream == NULL (pt_assemble_stripes uses the handle's own stream)");
    if ((rc = assemble_check(d, gathered, image, width, height, stripe_rows, n_ranks, slab_rows)) || (rc = flush_pending(d))) return rc;
    HIP_TRY(ptk_assemble_stripes((const float4*)gathered->dptr, (float4*)image->dptr, width, height, stripe_rows, n_ranks,
                                 slab_rows, as_stream(hip_stream)));
    image->version++;
    return PT_OK;
}

static int assemble_check(pt_device_s* d, pt_buffer_s* gathered, pt_buffer_s* image, int width, int height, int stripe_rows, int n_ranks, int slab_rows)
{
    if (!gathered || !image) return fail(PT_ERR_INVALID, "null buffer handle");
    if (gathered->dev != d || image->dev != d) return fail(PT_ERR_INVALID, "buffer belongs to another device");
    if (width < 1 || height < 1 || stripe_rows < 1 || n_ranks < 1 || slab_rows < 0) return fail(PT_ERR_INVALID, "invalid geometry");
    for (int r = 0; r < n_ranks; ++r)
        if (pt_local_rows(height, stripe_rows, n_ranks, r) > slab_rows) return fail(PT_ERR_INVALID, "slab_rows too small for rank %d", r);
    if ((size_t)n_ranks * slab_rows * width * sizeof(float4) > gathered->bytes) return fail(PT_ERR_RANGE, "gathered buffer too small");
    if ((size_t)width * height * sizeof(float4) > image->bytes) return fail(PT_ERR_RANGE, "image buffer too small");
    return PT_OK;
}

extern "C" int pt_assemble_stripes(pt_device_t d, pt_buffer_t gathered, pt_buffer_t image, int width, int height,
                                   int stripe_rows, int n_ranks, int slab_rows, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if ((rc = assemble_check(d, gathered, image, width, height, stripe_rows, n_ranks, slab_rows))) return rc;
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_assemble_stripes((const float4*)gathered->dptr, (float4*)image->dptr, width, height, stripe_rows, n_ranks,
                                 slab_rows, d->stream));
    image->version++;
    return event_end(d, ev);
}

extern "C" int pt_tonemap_ppm(pt_device_t d, pt_buffer_t framebuffer, pt_buffer_t rgb_i32, size_t num_pixels, pt_event_t ev)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!framebuffer || !rgb_i32) return fail(PT_ERR_INVALID, "null buffer handle");
    if (framebuffer->dev != d || rgb_i32->dev != d) return fail(PT_ERR_INVALID, "buffer belongs to another device");
    if (num_pixels * sizeof(float4) > framebuffer->bytes) return fail(PT_ERR_RANGE, "framebuffer too small");
    if (num_pixels * 3 * sizeof(int32_t) > rgb_i32->bytes) return fail(PT_ERR_RANGE, "rgb buffer too small");
    if ((rc = enter_stream(d)) || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_tonemap_ppm((const float4*)framebuffer->dptr, (int32_t*)rgb_i32->dptr, num_pixels, d->stream));
    rgb_i32->version++;
    return event_end(d, ev);
}

extern "C" int pt_profile_enable(pt_device_t d, int on)
{
    int rc = use_device(d);
    if (rc) return rc;
    d->prof_on = on != 0;
    return PT_OK;
}

extern "C" int pt_profile_reset(pt_device_t d)
{
    int rc = use_device(d);
    if (rc) return rc;
    if ((rc = enter_stream(d)) || (rc = stream_wait(d))) return rc;
    for (int k = 0; k < PT_PROF_KINDS; ++k) d->prof_used[k] = 0;
    return PT_OK;
}

extern "C" int pt_profile_query(pt_device_t d, int kind, double* total_ms, uint64_t* launches)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (kind < 0 || kind >= PT_PROF_KINDS || !total_ms || !launches) return fail(PT_ERR_INVALID, "bad profile query");
    if ((rc = enter_stream(d)) || (rc = stream_wait(d))) return rc;
    double sum = 0.0;
    for (size_t i = 0; i < d->prof_used[kind]; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, d->prof_pairs[kind][i].first, d->prof_pairs[kind][i].second));
        sum += ms;
    }
    *total_ms = sum;
    *launches = d->prof_used[kind];
    return check_traversal(d);
}

// test hook (include/pt_shim.h): the hierarchy as the kernels read it, copied out; nothing of the device's state moves
extern "C" int pt_bvh_snapshot(pt_device_t d, pt_bvh_info* info, void* records, size_t record_capacity, int32_t* big_indices)
{
    static_assert(sizeof(pt_bvh_info) == 64, "pt_bvh_info layout");
    static_assert(PT_BVH_SNAPSHOT_BIG_MAX == PT_BVH_BIG_MAX, "the header's bound is the builder's");
    int rc = use_device(d);
    if (rc) return rc;
    if (!info) return fail(PT_ERR_INVALID, "pt_bvh_snapshot: info is null");
    // deferred frames are work the caller has already asked for: they are submitted first (they may prepare a scene and build its
    // hierarchy), and only then is the state looked at -- the snapshot itself prepares and builds nothing
    if ((rc = flush_pending(d)) || (rc = stream_wait(d))) return rc;
    if (!d->bvh_valid || !d->bvh) return fail(PT_ERR_INVALID, "no LBVH stands for the prepared scene");
    memset(info, 0, sizeof *info);
    info->records = (uint32_t)d->bvh_records;
    info->num_big = d->nbig;
    info->num_triangles = d->prep_ntri;
    for (int a = 0; a < 3; ++a) { info->grid_min[a] = d->bvh_grid.gmin[a]; info->grid_step[a] = d->bvh_grid.gstep[a]; }
    if (records) {
        if (record_capacity < d->bvh_records) return fail(PT_ERR_RANGE, "pt_bvh_snapshot: %zu records do not fit %zu", d->bvh_records, record_capacity);
        if (d->bvh_records) HIP_TRY(hipMemcpy(records, d->bvh, d->bvh_records * sizeof(PtBvh8Node), hipMemcpyDeviceToHost));
    }
    if (big_indices && d->nbig > 0) HIP_TRY(hipMemcpy(big_indices, d->bigidx, (size_t)d->nbig * sizeof(int), hipMemcpyDeviceToHost));
    return PT_OK;
}

// test hook (include/pt_shim.h): the primary-ray candidate masks as the trace kernel reads them, copied out
extern "C" int pt_primary_mask_snapshot(pt_device_t d, uint32_t* num_pixels, void* masks, size_t capacity)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!num_pixels) return fail(PT_ERR_INVALID, "pt_primary_mask_snapshot: num_pixels is null");
    if ((rc = flush_pending(d)) || (rc = stream_wait(d))) return rc;   // (the masks are made on the handle's stream, read by the lanes)
    if (!d->pmask_key.valid || d->pmask_key.scene_gen != d->scene_gen || !d->pmask.p)
        return fail(PT_ERR_INVALID, "no primary-ray masks stand for the prepared scene");
    const size_t npix = (size_t)(uint32_t)d->pmask_key.g[5];
    *num_pixels = (uint32_t)npix;
    if (masks) {
        if (capacity < npix) return fail(PT_ERR_RANGE, "pt_primary_mask_snapshot: %zu pixels do not fit %zu", npix, capacity);
        if (npix) HIP_TRY(hipMemcpy(masks, d->pmask.p, npix * sizeof(uint2), hipMemcpyDeviceToHost));
    }
    return PT_OK;
}

// test hook (include/pt_shim.h): the secondary-ray candidate masks of the scene in hand, copied out
extern "C" int pt_secondary_mask_snapshot(pt_device_t d, uint32_t info[4], void* masks, size_t capacity)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!info) return fail(PT_ERR_INVALID, "pt_secondary_mask_snapshot: info is null");
    if ((rc = flush_pending(d)) || (rc = stream_wait(d))) return rc;   // (the table is made on the handle's stream, read by the lanes)
    if (!d->smask_key.valid || d->smask_key.scene_gen != d->scene_gen || d->smask_key.ntri != d->prep_ntri || !d->smask.p)
        return fail(PT_ERR_INVALID, "no secondary-ray masks stand for the prepared scene");
    const size_t n = (size_t)d->smask_key.ntri * PT_SM_TRI_ENTRIES;
    info[0] = (uint32_t)n; info[1] = (uint32_t)d->smask_key.ntri; info[2] = PT_SM_T; info[3] = PT_SM_C;
    if (masks) {
        if (capacity < n) return fail(PT_ERR_RANGE, "pt_secondary_mask_snapshot: %zu entries do not fit %zu", n, capacity);
        HIP_TRY(hipMemcpy(masks, d->smask.p + PT_SM_HEAD_ENTRIES, n * sizeof(uint2), hipMemcpyDeviceToHost));
    }
    return PT_OK;
}

extern "C" int pt_profile_query_union(pt_device_t d, int kind, double* union_ms)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (kind < 0 || kind >= PT_PROF_KINDS || !union_ms) return fail(PT_ERR_INVALID, "bad profile query");
    if ((rc = enter_stream(d)) || (rc = stream_wait(d))) return rc;
    // launches are recorded in enqueue order and two lanes alternate: [start, stop] intervals relative to the first start,
    // swept in order of their starts
    const size_t n = d->prof_used[kind];
    std::vector<std::pair<double, double>> iv(n);
    for (size_t i = 0; i < n; ++i) {
        float a = 0.f, b = 0.f;
        if (i) HIP_TRY(hipEventElapsedTime(&a, d->prof_pairs[kind][0].first, d->prof_pairs[kind][i].first));
        HIP_TRY(hipEventElapsedTime(&b, d->prof_pairs[kind][0].first, d->prof_pairs[kind][i].second));
        iv[i] = { (double)a, (double)b };
    }
    std::sort(iv.begin(), iv.end());
    double total = 0.0, end = -1.0e300;
    for (auto& x : iv) {
        if (x.second <= end) continue;
        total += x.second - std::max(x.first, end);
        end = x.second;
    }
    *union_ms = total;
    return PT_OK;
}

// ------------------------------------------------------------------------------------------
// kernel registry + generic launcher
// ------------------------------------------------------------------------------------------
static const char* base_name(const char* path)
{
    const char* b = path;
    for (const char* p = path; *p; ++p)
        if (*p == '/' || *p == '\\') b = p + 1;
    return b;
}

extern "C" int pt_kernel_get(pt_device_t d, const char* file_name, const char* func_name, pt_kernel_t* out)
{
    if (!out) return fail(PT_ERR_INVALID, "out == NULL");
    *out = nullptr;
    if (!d || !file_name || !func_name) return fail(PT_ERR_INVALID, "null argument");
    std::string base = base_name(file_name);
    size_t dot = base.rfind('.');
    if (dot != std::string::npos) base.erase(dot);  // SELECT_KERNELPATH1 appends no extension; accept either
    for (int i = 0; i < KERNEL_COUNT; ++i)
        if (base == d->kernels[i].file && strcmp(func_name, d->kernels[i].func) == 0) {
            *out = &d->kernels[i];
            return PT_OK;
        }
    return fail(PT_ERR_NOT_FOUND, "no native kernel registered for (%s, %s)", file_name, func_name);
}

static int launch_generate_colors(pt_device_s* d, const pt_launch_arg* a, int nargs, long long n, pt_event_s* ev, float* ms_out)
{
    // __kernel void GenerateColors(tBuffer, matBuffer, gDst, const int4 cRes)  GenerateColors.cl:302-303
    if (nargs != 4 || !a[0].is_buffer || !a[1].is_buffer || !a[2].is_buffer || a[3].is_buffer || a[3].size != 16)
        return fail(PT_ERR_ARGS, "GenerateColors expects (buffer, buffer, buffer, int4)");
    pt_buffer_s *t = a[0].buffer, *m = a[1].buffer, *fb = a[2].buffer;
    if (!t || !m || !fb) return fail(PT_ERR_ARGS, "GenerateColors: null buffer argument");
    int32_t c[4];
    memcpy(c, a[3].data, 16);  // {W, H, frame, unused}: test/RaytraceTest.cpp:252-253
    if (c[0] < 1 || c[1] < 1 || c[2] < 0) return fail(PT_ERR_ARGS, "GenerateColors: invalid cRes {%d,%d,%d}", c[0], c[1], c[2]);
    long long npix = std::min<long long>(n, (long long)c[0] * c[1]);  // the kernel guards gid < W*H
    if (npix <= 0) return PT_OK;
    if (npix > 0xffffffffLL) return fail(PT_ERR_ARGS, "too many work-items");
    if (m->bytes < sizeof(PtRawMaterial)) return fail(PT_ERR_RANGE, "material buffer too small");

    // Deferral is invisible only while every buffer involved can be observed through this ABI alone.
    // Caller-owned (wrapped) memory, or memory whose device pointer has been handed out, may be read
    // after launch1D + waitForCompletion (clFinish in the reference) or rewritten before the next
    // launch: such launches execute at once, in order.
    const bool observable = !t->owned || !m->owned || !fb->owned || t->exposed || m->exposed || fb->exposed;
    bool immediate = !d->opt_batch || ev || d->opt_profile || observable;
    PendingFrames& p = d->pending;
    if (p.active && !(p.tris == t && p.mats == m && p.fb == fb && p.width == c[0] && p.height == c[1] &&
                      p.pixel_count == (uint32_t)npix && p.z_begin + p.z_count == c[2] && !immediate)) {
        int rc = flush_pending(d);
        if (rc) return rc;
    }
    if (!immediate) {
        // validate now what flush would reject later, so errors surface at the launch
        if ((size_t)36 * sizeof(PtRawTriangle) > t->bytes) return fail(PT_ERR_RANGE, "triangle buffer smaller than 36 triangles");
        if ((size_t)npix * sizeof(float4) > fb->bytes) return fail(PT_ERR_RANGE, "framebuffer smaller than the launch");
        if (t->dev != d || m->dev != d || fb->dev != d) return fail(PT_ERR_INVALID, "buffer belongs to another device");
        if (p.active) {
            p.z_count++;
        } else {
            p.active = true;
            p.tris = t; p.mats = m; p.fb = fb;
            p.width = c[0]; p.height = c[1];
            p.z_begin = c[2]; p.z_count = 1;
            p.pixel_count = (uint32_t)npix;
        }
        if (ms_out) *ms_out = 0.f;
        return PT_OK;
    }
    const pt_render_params rp = reference_params(c[0], c[1], c[2], 1, m);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (d->opt_profile) {
        int jrc = stream_enqueue(d);   // earlier renders are not part of this launch's time, and the lanes start behind e0
        if (jrc) return jrc;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, d->stream));
    }
    int rc = render_internal(d, t, m, fb, rp, reference_camera(), (uint32_t)npix, nullptr, ev);   // (the reference's kernel takes no camera)
    if (d->opt_profile) {
        float ms = 0.f;
        if (!rc) rc = lanes_join(d);   // PROFILE_RETURN_TIME: the launch's duration as the handle's stream sees it
        if (!rc) {
            hipEventRecord(e1, d->stream);
            hipEventSynchronize(e1);
            hipEventElapsedTime(&ms, e0, e1);
        }
        hipEventDestroy(e0);
        hipEventDestroy(e1);
        if (ms_out) *ms_out = ms;
    } else if (ms_out) {
        *ms_out = 0.f;
    }
    return rc;
}

static int launch_fill(pt_device_s* d, const pt_launch_arg* a, int nargs, long long n, pt_event_s* ev)
{
    // FillKernel(int* dst, int value): the shim smoke kernel (test/main.cpp:128-151 uses one from a
    // TestKernel.cl the reference does not ship)
    if (nargs != 2 || !a[0].is_buffer || a[1].is_buffer || a[1].size != 4) return fail(PT_ERR_ARGS, "FillKernel expects (buffer, int)");
    pt_buffer_s* b = a[0].buffer;
    if (!b || b->dev != d) return fail(PT_ERR_ARGS, "FillKernel: bad buffer");
    int32_t v;
    memcpy(&v, a[1].data, 4);
    long long cnt = std::min<long long>(n, (long long)(b->bytes / 4));
    int rc = enter_stream(d);
    if (rc || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_fill_i32((int32_t*)b->dptr, v, (int)std::min<long long>(cnt, 0x7fffffff), d->stream));
    b->version++;
    return event_end(d, ev);
}

static int launch_math(pt_device_s* d, const pt_launch_arg* a, int nargs, long long n, pt_event_s* ev)
{
    // MathKernel(const float* in, float* out): out[4i..4i+3] = sin, cos, pow(.,2.2f), pow(.,1/2.2f) of in[i]
    if (nargs != 2 || !a[0].is_buffer || !a[1].is_buffer) return fail(PT_ERR_ARGS, "MathKernel expects (buffer, buffer)");
    pt_buffer_s *in = a[0].buffer, *out = a[1].buffer;
    if (!in || !out || in->dev != d || out->dev != d) return fail(PT_ERR_ARGS, "MathKernel: bad buffer");
    long long cnt = std::min<long long>(n, std::min<long long>((long long)(in->bytes / 4), (long long)(out->bytes / 16)));
    int rc = enter_stream(d);
    if (rc || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_math((const float*)in->dptr, (float*)out->dptr, (int)std::min<long long>(cnt, 0x7fffffff), d->stream));
    out->version++;
    return event_end(d, ev);
}

static int launch_fold_check(pt_device_s* d, const pt_launch_arg* a, int nargs, pt_event_s* ev)
{
    // FoldCheckKernel(ulong* out, int mode, uint first, ulong count): the fold kernel's short forms of pow and "/"
    // against the literal operations, operand by operand (csrc/pt_kernels.hip, pt_fold_check_kernel); the work-item
    // count of the launch is ignored, `count` operands are checked
    if (nargs != 4 || !a[0].is_buffer || a[1].is_buffer || a[1].size != 4 || a[2].is_buffer || a[2].size != 4 || a[3].is_buffer ||
        a[3].size != 8)
        return fail(PT_ERR_ARGS, "FoldCheckKernel expects (buffer, int, uint, ulong)");
    pt_buffer_s* out = a[0].buffer;
    if (!out || out->dev != d || out->bytes < 6 * sizeof(unsigned long long)) return fail(PT_ERR_ARGS, "FoldCheckKernel: bad buffer");
    int32_t mode;
    uint32_t first;
    uint64_t count;
    memcpy(&mode, a[1].data, 4);
    memcpy(&first, a[2].data, 4);
    memcpy(&count, a[3].data, 8);
    if (mode < 0 || mode > 4) return fail(PT_ERR_ARGS, "FoldCheckKernel: mode %d", mode);
    int rc = enter_stream(d);
    if (rc || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_fold_check((unsigned long long*)out->dptr, mode, first, count, d->stream));
    out->version++;
    return event_end(d, ev);
}

static int launch_shade_check(pt_device_s* d, const pt_launch_arg* a, int nargs, pt_event_s* ev)
{
    // ShadeCheckKernel(ulong* out, int mode, uint first, ulong count): pt_shade's short forms of "/" and 1 / sqrt against the
    // literal operations, operand by operand (csrc/pt_kernels.hip, pt_shade_check_kernel); the work-item count of the launch is
    // ignored, `count` operands are checked
    if (nargs != 4 || !a[0].is_buffer || a[1].is_buffer || a[1].size != 4 || a[2].is_buffer || a[2].size != 4 || a[3].is_buffer ||
        a[3].size != 8)
        return fail(PT_ERR_ARGS, "ShadeCheckKernel expects (buffer, int, uint, ulong)");
    pt_buffer_s* out = a[0].buffer;
    if (!out || out->dev != d || out->bytes < 8 * sizeof(unsigned long long)) return fail(PT_ERR_ARGS, "ShadeCheckKernel: bad buffer");
    int32_t mode;
    uint32_t first;
    uint64_t count;
    memcpy(&mode, a[1].data, 4);
    memcpy(&first, a[2].data, 4);
    memcpy(&count, a[3].data, 8);
    if (mode < 1 || mode > 3) return fail(PT_ERR_ARGS, "ShadeCheckKernel: mode %d", mode);
    int rc = enter_stream(d);
    if (rc || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_shade_check((unsigned long long*)out->dptr, mode, first, count, d->stream));
    out->version++;
    return event_end(d, ev);
}

static int launch_pair_check(pt_device_s* d, const pt_launch_arg* a, int nargs, pt_event_s* ev)
{
    // PairCheckKernel(const uint2* masks, uint* out, int ntri, uint cases, uint cap): the masked search's pending-pair list on the
    // caller's masks, one wave of 64 lanes per case (csrc/pt_kernels.hip, pt_pair_check_kernel); the work-item count of the launch is
    // ignored.  masks: cases x 64 x 2 words; out: cases x (2 + cap) words
    if (nargs != 5 || !a[0].is_buffer || !a[1].is_buffer || a[2].is_buffer || a[2].size != 4 || a[3].is_buffer || a[3].size != 4 ||
        a[4].is_buffer || a[4].size != 4)
        return fail(PT_ERR_ARGS, "PairCheckKernel expects (buffer, buffer, int, uint, uint)");
    pt_buffer_s *masks = a[0].buffer, *out = a[1].buffer;
    if (!masks || !out || masks->dev != d || out->dev != d) return fail(PT_ERR_ARGS, "PairCheckKernel: bad buffer");
    int32_t ntri;
    uint32_t cases, cap;
    memcpy(&ntri, a[2].data, 4);
    memcpy(&cases, a[3].data, 4);
    memcpy(&cap, a[4].data, 4);
    if (ntri < 1 || ntri > 64) return fail(PT_ERR_ARGS, "PairCheckKernel: %d triangles", ntri);
    if (cases > 65536u || cap > 4096u) return fail(PT_ERR_ARGS, "PairCheckKernel: %u cases of %u pairs", cases, cap);
    if (masks->bytes < (size_t)cases * 64u * 8u || out->bytes < (size_t)cases * (2u + cap) * 4u)
        return fail(PT_ERR_ARGS, "PairCheckKernel: buffer too small");
    int rc = enter_stream(d);
    if (rc || (rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_pair_check((const uint2*)masks->dptr, (unsigned*)out->dptr, ntri, cases, cap, d->stream));
    out->version++;
    return event_end(d, ev);
}

static int launch_search_check(pt_device_s* d, const pt_launch_arg* a, int nargs, pt_event_s* ev)
{
    // SearchCheckKernel(const pt_triangle* tris, const float4* rays, const uint2* masks, uint4* out, int ntri, uint cases): the masked
    // search itself on the caller's rays and masks, one wave of 64 lanes per case (csrc/pt_kernels.hip, pt_search_check_kernel); the
    // work-item count of the launch is ignored.  tris: the raw scene, prepared here as a render prepares it (ensure_prep; the search
    // reads records only, so neither the quad pairing nor an anchor is asked for) -- finite and det-bounded, as every scene that
    // carries masks is; rays: cases x 64 x 8 words; masks: cases x 64 x 2 words; out: cases x 64 x 8 words
    if (nargs != 6 || !a[0].is_buffer || !a[1].is_buffer || !a[2].is_buffer || !a[3].is_buffer || a[4].is_buffer || a[4].size != 4 ||
        a[5].is_buffer || a[5].size != 4)
        return fail(PT_ERR_ARGS, "SearchCheckKernel expects (buffer, buffer, buffer, buffer, int, uint)");
    pt_buffer_s *tris = a[0].buffer, *rays = a[1].buffer, *masks = a[2].buffer, *out = a[3].buffer;
    if (!tris || !rays || !masks || !out || tris->dev != d || rays->dev != d || masks->dev != d || out->dev != d)
        return fail(PT_ERR_ARGS, "SearchCheckKernel: bad buffer");
    int32_t ntri;
    uint32_t cases;
    memcpy(&ntri, a[4].data, 4);
    memcpy(&cases, a[5].data, 4);
    if (ntri < 1 || ntri > 64) return fail(PT_ERR_ARGS, "SearchCheckKernel: %d triangles", ntri);
    if (cases > 65536u) return fail(PT_ERR_ARGS, "SearchCheckKernel: %u cases", cases);
    if (tris->bytes < (size_t)ntri * sizeof(PtRawTriangle) || rays->bytes < (size_t)cases * 64u * 32u || masks->bytes < (size_t)cases * 64u * 8u ||
        out->bytes < (size_t)cases * 64u * 32u)
        return fail(PT_ERR_ARGS, "SearchCheckKernel: buffer too small");
    if (out == tris || out == rays || out == masks) return fail(PT_ERR_ARGS, "SearchCheckKernel: the results overlap an input");
    int rc = enter_stream(d);
    if (rc || (rc = ensure_prep(d, tris, ntri))) return rc;
    if (!d->prep_finite || !d->prep_det_bounded)
        return fail(PT_ERR_ARGS, "SearchCheckKernel: the scene is not finite and det-bounded (no such scene carries masks)");
    if ((rc = event_begin(d, ev))) return rc;
    HIP_TRY(ptk_search_check(d->prep, ntri, (const float4*)rays->dptr, (const uint2*)masks->dptr, (uint4*)out->dptr, cases, d->stream));
    out->version++;
    return event_end(d, ev);
}

extern "C" int pt_launch_2d(pt_device_t d, pt_kernel_t k, const pt_launch_arg* args, int nargs, int ntx, int nty, int lx,
                            int ly, pt_event_t ev, float* ms_out)
{
    int rc = use_device(d);
    if (rc) return rc;
    if (!k) return fail(PT_ERR_NOT_FOUND, "null kernel (Device::getKernel returned 0)");
    if (k < d->kernels || k >= d->kernels + KERNEL_COUNT) return fail(PT_ERR_INVALID, "kernel belongs to another device");
    if (nargs < 0 || nargs > PT_MAX_ARG_COUNT || (nargs && !args)) return fail(PT_ERR_ARGS, "bad argument list");
    for (int i = 0; i < nargs; ++i)
        if (!args[i].is_buffer && args[i].size > PT_MAX_ARG_SIZE) return fail(PT_ERR_ARGS, "constant %d larger than %d bytes", i, PT_MAX_ARG_SIZE);
    if (ntx < 0 || nty < 0 || lx < 1 || ly < 1) return fail(PT_ERR_ARGS, "bad launch geometry");
    if (ev && ev->dev != d) return fail(PT_ERR_INVALID, "event belongs to another device");
    long long n = (long long)ntx * nty;  // work-items the caller asked for (kernels guard the rounded-up tail)
    if (ms_out) *ms_out = 0.f;
    switch (k->id) {
    case KERNEL_GENERATE_COLORS: return launch_generate_colors(d, args, nargs, n, ev, ms_out);
    case KERNEL_FILL: return launch_fill(d, args, nargs, n, ev);
    case KERNEL_MATH: return launch_math(d, args, nargs, n, ev);
    case KERNEL_FOLD_CHECK: return launch_fold_check(d, args, nargs, ev);
    case KERNEL_SHADE_CHECK: return launch_shade_check(d, args, nargs, ev);
    case KERNEL_PAIR_CHECK: return launch_pair_check(d, args, nargs, ev);
    case KERNEL_SEARCH_CHECK: return launch_search_check(d, args, nargs, ev);
    default: return fail(PT_ERR_NOT_FOUND, "unknown kernel id");
    }
}
