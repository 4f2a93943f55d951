/*
 * pt_shim.h -- C ABI of libptshim.so, the MI355X-native replacement for the Adl CL
 * device / buffer / kernel / launcher layer that the reference's RaytraceTest harness
 * drives (reference file:line cited per entry point; all paths relative to the
 * reference repository).
 *
 * Everything behind this boundary is HIP for gfx950.  There is no CPU fallback: every
 * entry point that needs the GPU fails with PT_ERR_NO_DEVICE / PT_ERR_HIP when none is
 * usable.  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - every int-returning function returns PT_OK (0) on success, a PT_ERR_* code
 *     otherwise; pt_last_error() gives the message for the calling thread.
 *   - handles are opaque.  Calls on one device handle are not thread-safe (the reference
 *     is single-threaded, one in-order queue per device: Adl/CL/AdlCL.cpp:215); different
 *     handles may be driven from different threads / processes (one per GPU).
 *   - all device work of a handle takes effect in call order, as on the reference's in-order
 *     cl_command_queue.  Everything but the fused renderer is enqueued on ONE stream (the handle's);
 *     pt_render_frames runs its trace / fold launches on two internal streams ("lanes") so that the
 *     next trace launch fills the machine while the current one drains, and the handle's stream is
 *     ordered behind them (by events, never a host wait) as soon as any other call needs its results.
 */
#ifndef PT_SHIM_H
#define PT_SHIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: PT_ERR_TRAVERSAL, PT_OPT_BVH_STACK_LIMIT, PT_OPT_RENDER_LANES, PT_STAT_BVH_*, pt_assemble_stripes_on, the staging ring
 *    (pt_device_reserve_staging, pt_device_workspace_memory), device-side hand-overs (pt_device_wait_stream, pt_device_wait_hip_event,
 *    pt_event_wait_on), pt_profile_query_union; option 3 (a kernel-variant switch of version 1) is accepted and ignored */
#define PT_SHIM_ABI_VERSION 2

enum pt_status {
    PT_OK = 0,
    PT_ERR_INVALID = 1,    /* bad handle / argument                                   */
    PT_ERR_NO_DEVICE = 2,  /* no usable gfx950 device (Adl: device with isValid()==0) */
    PT_ERR_OOM = 3,        /* allocation failed (Adl: m_size=0,m_ptr=0 + log)         */
    PT_ERR_HIP = 4,        /* a HIP runtime call failed                               */
    PT_ERR_NOT_FOUND = 5,  /* unknown kernel (Adl: getKernel returns 0)               */
    PT_ERR_ARGS = 6,       /* launch arguments do not match the kernel's signature    */
    PT_ERR_RANGE = 7,      /* offset/size outside a buffer                            */
    PT_ERR_TRAVERSAL = 8   /* an LBVH search was cut short (stack capacity or step budget): the pixels of the renders
                              enqueued since the last successful observation may be wrong and must be discarded.  The
                              reference's brute force (GenerateColors.cl:137-154) cannot skip a triangle, so this is an
                              error, never a silent approximation; it cannot occur with a hierarchy the library built
                              (csrc/pt_kernels.hip, PT_BVH_STACK) unless PT_OPT_BVH_STACK_LIMIT lowers the stack.
                              Renders are asynchronous, so the error is DEFERRED: the kernels raise a sticky word in
                              host-visible memory and the first call that observes the device afterwards reports it --
                              pt_sync, pt_event_wait / pt_event_elapsed_ns, a blocking pt_buffer_map, pt_profile_query,
                              or the next pt_render_frames (which then renders nothing).  Reporting clears the word. */
};

typedef struct pt_device_s* pt_device_t;
typedef struct pt_buffer_s* pt_buffer_t;
typedef struct pt_kernel_s* pt_kernel_t;
typedef struct pt_event_s* pt_event_t;

/* message of the last failing call on this thread ("" if none) */
const char* pt_last_error(void);
int pt_abi_version(void);

/* ---- library / device lifetime ---------------------------------------------------- */
/* adl::init(TYPE_CL) / adl::quit : Adl/Adl.cpp:39-58, 60-82 (CL: clewInit dlopen).      */
int pt_init(void);
void pt_quit(void);
/* DeviceUtils::getNDevices : Adl/Adl.cpp:84-110 */
int pt_device_count(void);
/* DeviceUtils::allocate(TYPE_CL, cfg{m_deviceIdx}) -> DeviceCL::initialize :
 * Adl/Adl.cpp:160-198, Adl/CL/AdlCL.cpp:68-271 (context + in-order queue + KernelManager) */
int pt_device_create(int device_idx, pt_device_t* out);
/* DeviceUtils::deallocate -> DeviceCL::release : Adl/Adl.cpp:200-208, AdlCL.cpp:273-280.
 * Flushes pending work, frees the device's kernels; returns PT_ERR_INVALID if buffers of
 * this device are still alive (the reference asserts used-memory == 0). */
int pt_device_destroy(pt_device_t dev);

enum pt_info_kind {
    PT_INFO_NAME = 0,    /* Device::getDeviceName    AdlCL.cpp:237-240 */
    PT_INFO_BOARD = 1,   /* Device::getBoardName                         */
    PT_INFO_VENDOR = 2,  /* Device::getDeviceVendor                      */
    PT_INFO_VERSION = 3  /* Device::getDeviceVersion  (used for the PPM file name, test/TestBase.h:45-51) */
};
int pt_device_info(pt_device_t dev, int kind, char out[128]);
uint64_t pt_device_max_alloc(pt_device_t dev);   /* Device::getMaxAllocationSize */
uint64_t pt_device_mem_size(pt_device_t dev);    /* Device::getMemSize           */
uint64_t pt_device_used_memory(pt_device_t dev); /* Device::getUsedMemory  (Adl.h:168) */
uint64_t pt_device_peak_memory(pt_device_t dev); /* Device::getPeakMemory  (Adl.h:170) */
/* Device memory the handle holds for ITSELF (not counted by pt_device_used_memory, which is the caller's buffers as in the
 * reference): the radiance staging ring, the prepared scene, the LBVH, the primary-ray masks, the side tables. */
uint64_t pt_device_workspace_memory(pt_device_t dev);
/* The fused renderer stages path radiance (12 B per sample) between its trace and fold kernels in a ring of TWO equal slots,
 * allocated ONCE per device handle: `bytes` is the size of the whole ring (0 = the default, 2 x 192 MiB: sixteen 1024^2
 * frames per slot).  pt_render_frames walks its frames through the ring in chunks of as many whole frames as a slot holds
 * and, once the ring exists, neither allocates, frees nor waits for the device.  Called implicitly with 0 by the first
 * render; calling it again waits for the device and replaces the ring.  An image of which ONE frame does not fit a slot
 * (more than 16.7 M pixels with the default) makes the render grow the ring to fit -- the only allocation a render can
 * still make; reserve enough beforehand to avoid it.  No reference counterpart (the reference keeps no staging: one launch
 * per frame, 32 B of framebuffer traffic per sample, GenerateColors.cl:314-321). */
int pt_device_reserve_staging(pt_device_t dev, size_t bytes);
int pt_device_num_cus(pt_device_t dev);          /* DeviceUtils::getNCUs               */

/* Plumbing, no reference counterpart: run this handle's work on an existing hipStream_t
 * (e.g. a torch stream, so torch.distributed collectives can be ordered after renders with
 * stream events).  NULL restores the handle's own (non-blocking) stream.  A caller whose
 * "stream handle 0" means the legacy default stream (torch's default stream reports 0) must
 * pass PT_STREAM_LEGACY, HIP's own sentinel hipStreamLegacy, so that it is not mistaken for NULL. */
#define PT_STREAM_LEGACY ((void*)1)
int pt_device_set_stream(pt_device_t dev, void* hip_stream);
void* pt_device_get_stream(pt_device_t dev);
/* Device-side hand-overs for a caller that keeps the handle on its OWN stream (what the N-rank driver does: renders of
 * consecutive images then overlap, which a shared stream would serialise).  No reference counterpart.
 *   pt_device_wait_stream    : the handle's later work starts after everything enqueued so far on hip_stream (a hipStream_t)
 *   pt_device_wait_hip_event : ... after a hipEvent_t the caller has recorded (e.g. torch.cuda.Event.cuda_event)
 *   pt_event_wait_on         : work enqueued later on hip_stream starts after the call the event was passed to has completed
 * None of them blocks the host. */
int pt_device_wait_stream(pt_device_t dev, void* hip_stream);
int pt_device_wait_hip_event(pt_device_t dev, void* hip_event);
int pt_event_wait_on(pt_event_t ev, void* hip_stream);

/* DeviceUtils::waitForCompletion(device) -> clFinish : Adl/Adl.cpp:210-213, AdlCL.cpp:282-285.
 * NOTE: with frame batching enabled (pt_device_set_option) this does not force deferred
 * GenerateColors frames to execute; observing a buffer, pt_flush or an event does.  Only launches
 * whose three buffers are all shim-allocated and whose device pointers were never handed out
 * (pt_buffer_device_ptr) are ever deferred -- memory the caller can reach behind this ABI
 * (pt_buffer_wrap, pt_buffer_device_ptr) gets clFinish semantics: the launch runs at once. */
int pt_sync(pt_device_t dev);
/* DeviceUtils::flush -> clFlush : AdlCL.cpp:303-306.  Submits deferred frames. */
int pt_flush(pt_device_t dev);

enum pt_option {
    /* 1 (default): consecutive GenerateColors launches on the same buffers with frame
     * indices z, z+1, z+2 ... are coalesced and executed as one fused multi-frame render
     * when a result is observed.  Pixel results are bit-identical either way.
     * 0: each launch executes immediately (the reference's behaviour). */
    PT_OPT_BATCH_FRAMES = 0,
    /* max frames traced per chunk of the fused renderer (radiance staging = 16 B x pixels x
     * frames per chunk).  0 = auto (fit staging in ~1/16 of device memory). */
    PT_OPT_CHUNK_FRAMES = 1,
    /* Device::toggleProfiling(PROFILE_RETURN_TIME) (Adl.h:171): launches synchronise and
     * return their duration in ms (AdlKernelUtilsCL.cpp:470-487). */
    PT_OPT_PROFILE_RETURN_TIME = 2,
    /* (3 selected between trace-kernel variants until only one was left: values 0 and 1 are accepted and ignored) */
    PT_OPT_RESERVED_3 = 3,
    /* conservative pass-1 filter of the closest-hit search, for A/B timing and parity tests:
     * 0 = the strongest the uploaded scene allows, 1..3 = independent triangles (pt_tri_pass1),
     * 4 = the packed shared-u filter when the scene is made of (a,b,c),(c,d,a) quads (two quads per
     * instruction, pt_quad3_pass1; same as 0).  All settings produce identical pixels. */
    PT_OPT_QUAD_FILTER = 4,
    /* closest-hit search: 0 = brute force below 512 triangles, LBVH from 512 on;
     * 1 = brute force (the reference's intersectWorld loop, GenerateColors.cl:137-154); 2 = LBVH
     * (built on the GPU when the scene is first rendered; scenes of >= 2 triangles).  The LBVH
     * applies the same exact triangle test to a conservative candidate set and resolves ties to the
     * lower index, as the reference's ascending loop does; see csrc/pt_bvh.hip for the one
     * theoretical caveat (rays within ~0.05 degrees of a triangle's plane). */
    PT_OPT_ACCEL = 5,
    /* measurement only (bench.py's roofline of LBVH runs): 1 = renders that pass a stats buffer and
     * take the LBVH use the tallying build of the search, which adds its work counters to
     * stats[PT_STAT_BVH_*].  Same pixels; slower; never the timed kernel.  Default 0. */
    PT_OPT_BVH_TALLY = 6,
    /* 1 (default): for quad scenes of up to 64 triangles on the brute-force path, every render first computes,
     * per pixel, a conservative candidate set of triangles its primary rays can meet (the camera is fixed:
     * GenerateColors.cl:265-272), and waves of fresh primary rays skip the pass-1 filter.  0 = off (A/B timing,
     * parity tests).  Identical pixels either way.  The sets are bounded over half a pixel around the pixel's centre ray, which
     * holds only while the float roundings of a pixel's image-plane point stay a small part of a pixel: masks are made for
     * images with width^2 + height^2 <= 7626^2 (every image of up to 4096 x 4096); a larger image renders as under 0 and
     * no table stands for it (pt_primary_mask_snapshot). */
    PT_OPT_PRIMARY_MASKS = 7,
    /* test hook of the LBVH's overflow report: the number of stack entries a ray's search may use (1..64; default 64,
     * which no hierarchy built by the library can exceed).  A search that needs more raises the sticky word behind
     * PT_ERR_TRAVERSAL (reported by the next call that observes the device; no render waits for the device to read it). */
    PT_OPT_BVH_STACK_LIMIT = 8,
    /* streams ("lanes") consecutive renders alternate between: 2 (default) = the first trace launch of render k+1 fills the
     * machine while the last launch of render k runs its paths out (about 0.3 ms of falling lane use,
     * profiles/r03/launch_overhead.txt), folds ordered by events so that every pixel folds its frames in ascending order
     * (GenerateColors.cl:314-321); 1 = one stream, every launch waits for the previous one (A/B timing).  Identical pixels. */
    PT_OPT_RENDER_LANES = 9,
    /* 1 (default): the trace launches of a render are CHECKPOINTED -- a launch ends the moment its work queue has handed out
     * the last batch, every wave saving the paths it still holds, and the render's next launch resumes them -- so that walking
     * a render through the bounded staging ring in many short launches costs 5 % over one long launch (measured: DESIGN.md S6), not a
     * tail of falling lane use per launch; a render of ONE chunk is one launch and takes no checkpoint; 0 = every launch runs its
     * paths out (A/B timing).  The LBVH kernel's checkpoint is one search deep: a stopping launch lets every lane finish its
     * current search and hands the shaded paths on.  Identical pixels either way. */
    PT_OPT_CHECKPOINT = 10,
    /* read-only (pt_device_get_option): LBVH builds this handle has made.  A scene is built once; a triangle buffer the caller can
     * write behind the ABI (pt_buffer_wrap, pt_buffer_device_ptr) is prepared again for every render, and built again only when the
     * checksum of its records has changed. */
    PT_OPT_BVH_BUILD_COUNT = 11,
    /* 1 (default): for quad scenes of up to 64 triangles on the brute-force path, the scene upload also tabulates, per cell of
     * (triangle a ray leaves, tile of that triangle's plane, cell of a cube map of directions), a conservative candidate set of
     * the triangles such a ray can meet; a path's secondary rays then look their candidates up instead of running the pass-1
     * filter.  The table depends on the scene alone -- a camera change or another image size does no table work -- and is part of
     * the handle's workspace (pt_device_workspace_memory; 442 368 bytes per triangle: 15.9 MB for the Cornell box's 36).  A ray the table does not cover (an origin
     * further than about 0.01 from the triangle it left, a direction that is not of unit length) keeps every triangle; a scene with a triangle for which no table is made (degenerate; a height of less than about 0.65, against
     * which the rays' 0.01 offset is not small; too far from the origin of coordinates for the classification's rounding) declines the
     * table and renders through pass 1, as the parent of this option did.  The scene's first render builds the table (about 23 ms for
     * the Cornell box) and, once per scene, waits for the device to read the prepared records back.  0 = off:
     * secondary rays run pass 1 (A/B timing, parity tests).  Identical pixels either way. */
    PT_OPT_SECONDARY_MASKS = 12,
    /* how a level of pt_denoise gathers its 5 x 5 taps, for A/B timing and parity tests: 1 = every lane loads its taps from global
     * memory (coalesced across the lanes of a row at every step); 2 = at steps 1 and 2 a workgroup first stages its 32 x 8 pixels
     * and their halo in LDS (larger steps gather as under 1: their halo dwarfs the tile); 0 (default) = the faster of the two per
     * step as measured (profiles/denoise/rates.txt).  Identical bits under every setting. */
    PT_OPT_DENOISE_TILE = 13,
    /* how pt_reproject reaches the previous view's records, for A/B timing and parity tests: 1 = one kernel, every lane reads its
     * four taps' 56-byte records directly; 2 = a prepare pass first turns the previous view's normal and depth records into one
     * float4 per pixel in the scratch, the taps read 16 bytes each and the colour record only where a tap survives; 0 (default) =
     * the faster of the two as measured (profiles/reproject/rates.txt).  Identical bits under every setting. */
    PT_OPT_REPROJECT_FORM = 14,
    /* how the pool pass of pt_denoise_spatial reaches its 7 x 7 taps, for A/B timing and parity tests: 1 = every lane loads its taps'
     * records and guides from global memory; 2 = a workgroup first stages its 32 x 8 pixels and their halo of 3 in LDS; 0 (default)
     * = the faster of the two as measured (profiles/denoise_spatial/rates.txt).  Identical bits under every setting. */
    PT_OPT_DENOISE_SPATIAL_FORM = 15
};
int pt_device_set_option(pt_device_t dev, int option, int64_t value);
int64_t pt_device_get_option(pt_device_t dev, int option);

/* ---- buffers ------------------------------------------------------------------------ */
/* Buffer<T>::allocate -> DeviceCL::allocate -> clCreateBuffer(READ_WRITE) :
 * Adl/Adl.inl:185-201, Adl/CL/AdlCL.inl:170-249.  bytes == 0 is allowed (no storage). */
int pt_buffer_alloc(pt_device_t dev, size_t bytes, pt_buffer_t* out);
/* Buffer<T>::setRawPtr (Adl.h:214): adopt device memory owned by the caller
 * (e.g. a torch tensor); pt_buffer_free does not free it. */
int pt_buffer_wrap(pt_device_t dev, void* device_ptr, size_t bytes, pt_buffer_t* out);
/* ~Buffer -> DeviceCL::deallocate : Adl.inl:153-165, AdlCL.inl:251-268 */
int pt_buffer_free(pt_buffer_t buf);
size_t pt_buffer_size(pt_buffer_t buf);
/* Buffer<T>::getInternalObject / m_ptr.  Submits deferred frames that touch the buffer and
 * switches frame batching off for it from now on (the caller can see the memory directly). */
void* pt_buffer_device_ptr(pt_buffer_t buf);
/* The buffer's device address as a VALUE (the facade's public Buffer<T>::m_ptr member, which in the reference holds
 * the opaque cl_mem: printing, identity).  It does not license access to the memory behind this ABI and changes
 * nothing; code that wants to read or write the memory itself must obtain the pointer with pt_buffer_device_ptr. */
void* pt_buffer_address(pt_buffer_t buf);
/* Buffer<T>::write / read (host) -> clEnqueueWrite/ReadBuffer : AdlCL.inl:297-340.
 * Asynchronous w.r.t. the host like the reference (non-blocking enqueue); the host range
 * must stay valid until pt_sync / the event.  ev may be NULL. */
int pt_buffer_write(pt_buffer_t dst, const void* host_src, size_t bytes, size_t dst_offset, pt_event_t ev);
int pt_buffer_read(pt_buffer_t src, void* host_dst, size_t bytes, size_t src_offset, pt_event_t ev);
/* Buffer<T>::write(Buffer&) / read(Buffer&) -> clEnqueueCopyBuffer : AdlCL.inl:270-295 */
int pt_buffer_copy(pt_buffer_t dst, pt_buffer_t src, size_t bytes, size_t dst_offset, size_t src_offset, pt_event_t ev);
/* Buffer<T>::getHostPtr(size=-1, blocking=false) -> clEnqueueMapBuffer(READ|WRITE) :
 * AdlCL.inl:434-445.  bytes == (size_t)-1 maps the whole buffer.  Returns a pinned host
 * staging range holding the buffer contents once the device has completed
 * (pt_sync, or blocking != 0); NULL on failure. */
void* pt_buffer_map(pt_buffer_t buf, size_t bytes, int blocking);
/* Buffer<T>::returnHostPtr -> clEnqueueUnmapMemObject : AdlCL.inl:447-451.
 * Copies the mapped range (the `bytes` of the matching pt_buffer_map, no more) back to the
 * device (asynchronously) and releases it. */
int pt_buffer_unmap(pt_buffer_t buf, void* host_ptr);

/* Page-locked host memory, so that pt_buffer_read / pt_buffer_write into it are truly asynchronous
 * (the progressive driver's double-buffered readback).  No Adl counterpart: the
 * reference only has the driver-owned mapping of getHostPtr. */
int pt_host_alloc(size_t bytes, void** out);
int pt_host_free(void* host_ptr);

/* ---- events (SyncObject : Adl/AdlKernel.h:45-54, AdlCL.inl:452-478) ------------------- */
int pt_event_create(pt_device_t dev, pt_event_t* out);
int pt_event_destroy(pt_event_t ev);
int pt_event_wait(pt_event_t ev);        /* DeviceUtils::waitForCompletion(SyncObject*) */
int pt_event_is_complete(pt_event_t ev); /* DeviceUtils::isComplete : 1 / 0, <0 on error */
/* Device::getExecutionTimeNanoseconds(SyncObject*) : AdlCL.cpp:508-517 */
int pt_event_elapsed_ns(pt_event_t ev, uint64_t* ns_out);

/* ---- kernels and launches -------------------------------------------------------------- */
/* Device::getKernel(fileName, funcName) -> KernelManager::query :
 * Adl/CL/AdlCL.cpp:490-493, Adl/AdlKernel.cpp:94-224.  The registry is static (kernels
 * are compiled into the library for gfx950; nothing is built at run time).  Only the
 * basename of file_name is significant, so the reference's "../test/ClKernels/GenerateColors"
 * resolves.  Unknown kernels -> PT_ERR_NOT_FOUND and *out = NULL (Adl returns 0).
 * Registered: ("GenerateColors","GenerateColors"), ("PtShimTest","FillKernel"),
 * ("PtShimTest","MathKernel"), ("PtShimTest","FoldCheckKernel"), ("PtShimTest","ShadeCheckKernel"),
 * ("PtShimTest","PairCheckKernel"), ("PtShimTest","SearchCheckKernel") -- the last six are smoke/parity-test kernels. */
int pt_kernel_get(pt_device_t dev, const char* file_name, const char* func_name, pt_kernel_t* out);

#define PT_MAX_ARG_SIZE 64  /* Launcher::MAX_ARG_SIZE  Adl/AdlKernel.h:129 */
#define PT_MAX_ARG_COUNT 64 /* Launcher::MAX_ARG_COUNT Adl/AdlKernel.h:130 */

/* One positional kernel argument; mirrors Launcher::Args (Adl/AdlKernel.h:133-140):
 * buffers first-class, constants by value (<= 64 bytes). */
typedef struct pt_launch_arg {
    int32_t is_buffer;   /* 1: buffer, 0: by-value constant */
    int32_t read_only;   /* BufferInfo::m_isReadOnly        */
    uint64_t size;       /* constants: byte count           */
    pt_buffer_t buffer;  /* when is_buffer                  */
    unsigned char data[PT_MAX_ARG_SIZE];
} pt_launch_arg;

/* Launcher::launch2D -> LauncherCL::launch2D : Adl/AdlKernel.inl:186-196,
 * Adl/CL/AdlKernelUtilsCL.cpp:440-500.  launch1D(n, l) is launch2D(n, 1, l, 1).  The global
 * size is rounded up to a multiple of the local size as the reference does (:461-468) but,
 * unlike the reference kernel, the HIP kernels guard gid < n so a ragged n is safe.
 * ms_out (may be NULL) receives the duration when PT_OPT_PROFILE_RETURN_TIME is set, else 0. */
int pt_launch_2d(pt_device_t dev, pt_kernel_t kernel, const pt_launch_arg* args, int nargs,
                 int num_threads_x, int num_threads_y, int local_x, int local_y,
                 pt_event_t ev, float* ms_out);

/* ---- the fused hot path -------------------------------------------------------------------
 * One call = frames [frame_begin, frame_begin+frame_count) of GenerateColors
 * (test/ClKernels/GenerateColors.cl:302-322) over this device's share of the image,
 * bit-identical to frame_count successive reference launches.  Asynchronous: the call returns when the work is enqueued;
 * `ev` (may be NULL) completes when the framebuffer holds the last frame.  Consecutive calls overlap on the device as far as
 * their data allows (the folds of all calls form one chain, so renders into the same framebuffer fold in call order).
 *
 * Image sharding: the image's rows are dealt to n_ranks devices in stripes
 * of stripe_rows rows, round-robin; this device (rank) renders the rows r with
 * (r / stripe_rows) % n_ranks == rank, in ascending order, into a LOCAL framebuffer of
 * pt_local_rows(...) x width float4.  Seeds and camera rays use the GLOBAL pixel id
 * (GenerateColors.cl:305-308), so the assembled image equals the single-device image bit
 * for bit.  n_ranks = 1 gives the plain full-image framebuffer. */
typedef struct pt_render_params {
    int32_t width, height;   /* cRes.x, cRes.y */
    int32_t frame_begin;     /* first cRes.z */
    int32_t frame_count;
    int32_t max_bounces;     /* BOUNCES (16, GenerateColors.cl:5); 2 = build-defined "direct" mode.  1..65535; at most 256 on a scene of
                              * at most 256 triangles rendered without the LBVH (PT_ERR_INVALID above that: a parked path of that
                              * kernel keeps its bounce count in 8 bits; PT_OPT_ACCEL 2 renders such a scene at any depth) */
    int32_t num_triangles;   /* NUM_TRIANGLES (36, :6) */
    int32_t num_materials;   /* bound for the material fetch at :239 */
    int32_t stripe_rows;     /* >= 1 */
    int32_t n_ranks;         /* >= 1 */
    int32_t rank;            /* 0 .. n_ranks-1 */
    int32_t reserved[6];     /* must be 0 */
} pt_render_params;

/* number of image rows owned by rank (see above) */
int pt_local_rows(int height, int stripe_rows, int n_ranks, int rank);

/* work counters accumulated by pt_render_frames when stats != NULL (uint64 each) */
enum {
    PT_STAT_SAMPLES = 0, PT_STAT_RAYS = 1,
    /* PT_OPT_BVH_TALLY renders only: box nodes entered and triangles tested (summed over the rays), and the phases
     * the waves executed for them (a node phase enters one node per participating lane, a triangle phase tests one
     * triangle per participating lane) */
    PT_STAT_BVH_NODES = 2, PT_STAT_BVH_TRIS = 3, PT_STAT_BVH_STEPS = 4 /* node phases */, PT_STAT_BVH_TRI_STEPS = 5,
    PT_STAT_BVH_MAX_STACK = 6 /* the deepest traversal stack any ray needed (a maximum, not a sum; capacity: 64) */,
    PT_STAT_CARRIED = 7 /* samples (paths under way + samples not yet started) that checkpointed launches handed to their successors */,
    /* PT_OPT_BVH_TALLY renders only: accepted closest hits at cos(incidence) < 1e-2, i.e. outside the range over which the LBVH's box
     * margin is argued conservative (csrc/pt_bvh.hip) -- the measured exposure of a scene to the LBVH's one theoretical caveat */
    PT_STAT_BVH_GRAZING = 8,
    PT_STAT_WORDS = 16
};

int pt_render_frames(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                     pt_buffer_t framebuffer, const pt_render_params* params,
                     pt_buffer_t stats /* may be NULL; PT_STAT_WORDS uint64, accumulated */,
                     pt_event_t ev);

/* ---- the camera --------------------------------------------------------------------------
 * The reference keeps its camera in the kernel source: GenerateColors.cl:263-269 declares fov, eye, center and up as
 * literals inside generateRay, and a user moves the camera by editing those lines (Adl compiles the .cl at run time).  The
 * kernels here are compiled ahead of time, so the same four values are passed instead; no Adl entry point has a counterpart.
 * The derived values -- viewDir, holDir, upDir (:270-272) and angle = tan(fov / 2) (:268) -- are computed once per render
 * on the host, in binary32 with the reference's normalize / cross, in its order; the per-ray expression
 * (:278-287) is the reference's, unchanged. */
typedef struct pt_camera {
    float eye[3];        /* GenerateColors.cl:265 (0, 2.75, 4) */
    float center[3];     /* :266, the point looked at (eye + (0, 0, -1)) */
    float up[3];         /* :267 (0, 1, 0) */
    float fov_y_deg;     /* vertical field of view in degrees, (0, 180) (:263: 60) */
    float lens_radius;   /* R, world units: finite and >= 0; 0 (or -0) is the pinhole */
    float focus_distance;/* F: 0 or finite and > 0; must be > 0 when lens_radius > 0 */
    int32_t reserved[4]; /* must be 0 */
} pt_camera;             /* 64 bytes; all six trailing words 0 is the camera without a lens (ABI version 2 as before) */
/* THE THIN LENS.  The reference has half of one: generateRay forms pointAimed = eye + 4.0f * dir (:285) and shoots from the eye through
 * it -- a focus distance of 4 and an aperture of zero.  With lens_radius == 0 a sample is exactly that: the literal 4.0f, no extra draw,
 * the same bits, whatever focus_distance holds.  With R = lens_radius > 0 and F = focus_distance: the two jitter draws come first
 * (:278-279), dir is formed as at :278-284, then two more uniforms are drawn, u1 then u2, before anything else touches the seed, and in
 * binary32 under PTSPEC (no contraction, scale3 then add3, the contract's sqrt, its sin / cos on [0, 2 pi]: getRandomFloat may
 * return 1.0, which stays inside that range)
 *     r   = R * sqrt(u1)            phi = TWO_PI * u2
 *     lx  = r * cos(phi)            ly  = r * sin(phi)
 *     org = (eye + holDir * lx) + upDir * ly
 *     pointAimed = eye + F * dir                       (:285 with its literal made a parameter)
 *     ray = getRay(org, normalize(pointAimed - org))   (:287; getRay normalises once more)
 * The focus surface is the SPHERE of radius F about the eye (the reference's own expression, not a plane); the lens is the disc of
 * radius R in the plane of holDir and upDir, sampled uniformly in area.  No relation between R and F is required; a degenerate
 * pointAimed == org makes a NaN ray, defined behaviour as every NaN path here is.  Everything after the primary ray -- the seed going
 * on, the walk, the light samples, the store, the fold -- is untouched.
 * WHO TAKES A LENS: every entry point that takes a pt_camera and starts its samples one by one -- pt_render_ao; pt_render_direct and
 * its _power, _ris, _env forms; pt_render_indirect and its _mis, _power, _rr, _ris, _env, _pixels, _pixels_ris forms; pt_camera_rays,
 * whose origins are then the lens points, so a query of those rays traces a lens render's first bounce bit for bit.
 * WHO REFUSES: pt_render_frames_camera returns PT_ERR_INVALID for lens_radius > 0, before anything is enqueued -- its kernels' primary-ray
 * masks and pass-1 tables are built on org == eye bit for bit.  pt_render_indirect with no lights renders that image bit for bit and
 * takes the lens.  pt_render_frames and the Adl-shaped launches have no camera at all. */

/* the reference's camera (:263-267) */
void pt_camera_reference(pt_camera* out);
/* Host only, no device: validate cam and return its derived values {eye xyz, viewDir xyz, holDir xyz, upDir xyz, angle, lens_radius,
 * focus_distance, 0}.  PT_ERR_INVALID when an input is not finite, fov_y_deg is outside (0, 180), a reserved field is not 0, lens_radius
 * is negative or not finite, focus_distance is negative or not finite, lens_radius > 0 with focus_distance == 0, or a derived value is
 * not finite (center == eye, up parallel to the view direction) -- cases in which the reference makes NaN rays.  Every entry point that
 * takes a camera validates it so, before anything is enqueued. */
int pt_camera_derive(const pt_camera* cam, float out[16]);
/* pt_render_frames seen from cam (validated as pt_camera_derive does; an invalid camera, or one with lens_radius > 0, renders nothing
 * and returns PT_ERR_INVALID).  cam == NULL is exactly pt_render_frames.  Rendering with another camera than the previous call rewrites
 * the pass-1 filter's tables on the device, behind the renders in flight; it neither waits for the device nor allocates.
 * (The Adl-shaped GenerateColors launches -- pt_launch_2d -- keep the reference's camera: its kernel signature has none.) */
int pt_render_frames_camera(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials, pt_buffer_t framebuffer,
                            const pt_render_params* params, const pt_camera* cam,
                            pt_buffer_t stats /* may be NULL */, pt_event_t ev);

/* ---- batched ray queries -----------------------------------------------------------------------------------------
 * The renderer's closest-hit search -- intersectWorld (GenerateColors.cl:137-154) over the reference's exact triangle test
 * (:96-125), ties to the lower index -- for rays of the caller's.  No Adl entry point has a counterpart: the reference reaches
 * the search only from inside its kernel.  The search is chosen exactly as for renders (PT_OPT_ACCEL, PT_OPT_QUAD_FILTER, the
 * scene's determinant bound) and uses the handle's prepared scene: querying the triangle buffer a render uses neither prepares
 * it again nor rebuilds its LBVH (PT_OPT_BVH_BUILD_COUNT), and a query never moves the pass-1 filter's anchor (the eye of the
 * last render).  Work goes to the handle's stream in call order, behind the renders in flight, and is asynchronous: `ev` (may
 * be NULL) completes with it.  Once the scene is prepared, a query neither allocates nor waits for the device.  An LBVH
 * search cut short raises the word behind PT_ERR_TRAVERSAL, reported as for renders.  Argument errors (PT_ERR_INVALID,
 * PT_ERR_RANGE) are returned before anything is enqueued; buffers are 16-byte aligned, rays and results do not overlap. */
typedef struct pt_ray {      /* 32 bytes: the arguments of getRay (GenerateColors.cl:73-77) */
    float origin[3];
    float tmax;              /* a hit counts at 0 < t < min(tmax, 1e20); tmax NaN or <= 0: the ray misses */
    float dir[3];            /* any length: normalised on the device exactly as getRay does; t is a distance */
    int32_t reserved;
} pt_ray;
typedef struct pt_hit {      /* 48 bytes */
    float t; int32_t tri; float u, v;   /* miss: t = +inf, tri = -1, u = v = 0 (and p = n = 0, material = -1) */
    float p[3]; int32_t material;       /* p = origin + normalize(dir) * t (:127); material = the triangle's id field */
    float n[3]; int32_t reserved;       /* the HitRecord's normal, normalize(N u + N v + N w), N = cross(e2, e1) (:123, :128-130) */
} pt_hit;
enum { PT_QUERY_CLOSEST = 0 /* one pt_hit per ray */, PT_QUERY_OCCLUDED = 1 /* one int32 per ray: 1 if the closest query hits, else 0 */ };
/* num_rays rays of `rays` (pt_ray) -> `out`, for the first num_triangles records of `triangles` (0: every ray misses) */
int pt_intersect_rays(pt_device_t dev, pt_buffer_t triangles, int num_triangles, pt_buffer_t rays,
                      pt_buffer_t out, size_t num_rays, int mode, pt_event_t ev);
/* width x height rays into `rays`: ray gid = y * width + x is the primary ray the renderer traces for pixel gid in frame
 * `frame` (seed gid + hash(frame), :305-308; the camera's jitter and expression, :278-287) seen from cam (NULL = the
 * reference's; validated as by pt_camera_derive).  origin = the eye -- with lens_radius > 0 the sample's lens point --, tmax = 1e20, dir = the vector the reference passes
 * to getRay at :287, normalised once: pt_intersect_rays normalises it again as getRay does, so a query of these rays traces the
 * renderer's primary rays bit for bit. */
int pt_camera_rays(pt_device_t dev, const pt_camera* cam /* NULL = reference */, int width, int height,
                   int frame, pt_buffer_t rays, pt_event_t ev);
/* One int32 per ray, the same value pt_intersect_rays(..., PT_QUERY_OCCLUDED) writes, found by a search that stops at the
 * first triangle the exact test accepts at 0 < t < min(tmax, 1e20) (through the LBVH; brute force runs the closest search).
 * Arguments, stream, scene preparation and the deferred PT_ERR_TRAVERSAL are pt_intersect_rays's. */
int pt_occluded_rays(pt_device_t dev, pt_buffer_t triangles, int num_triangles, pt_buffer_t rays, pt_buffer_t out,
                     size_t num_rays, pt_event_t ev);

/* ---- ambient occlusion ---------------------------------------------------------------------------------------------
 * The AmbientOcclusion case the reference's harness declares (test/RaytraceTest.cpp:293-295) with an empty body, composed of
 * the reference's own steps.  A sample of pixel gid = y * width + x in frame z: seed = gid + hash(z) (GenerateColors.cl:308), the
 * renderer's primary ray (:263-288) and its closest hit from tmax 1e20 (:141).  A miss adds nothing.  A hit adds 1 to `hits`; with
 * p = o + d t (:127) and n the HitRecord normal (:128-130) turned to face the ray (:243), K times in order: wi =
 * sampleHemisphereCosine(n, &seed) (:161-172, the same seed), and the ray getRay(p + wi 0.01, wi) (:257) adds 1 to `open` when no
 * triangle passes the exact test (:96-125) at 0 < t < min(radius, 1e20).  Every triangle occludes; materials play no part.
 * counts: pt_local_rows(...) x width records {uint32 open, uint32 hits} in the renderer's stripe layout (pt_render_params),
 * overwritten when frame_begin = 0 (the :314-321 rule), otherwise added to.  image (may be NULL): float4 (a, a, a, 1) per local
 * pixel from everything the counts hold after this call, a = hits > 0 ? (float)open / (float)(K hits) : miss_value (K hits in
 * uint32; one IEEE division) -- the renderer's framebuffer layout, for pt_assemble_stripes and pt_tonemap_ppm.
 * AO renders behave like queries: the handle's stream, behind renders in flight, asynchronous (ev); the scene, LBVH and filter
 * tables as a query uses them (no anchor move, no rebuild); once the scene is prepared no allocation and no wait; PT_OPT_ACCEL
 * and PT_OPT_QUAD_FILTER choose the search, PT_OPT_PRIMARY_MASKS is not used; a cut-short LBVH search raises PT_ERR_TRAVERSAL.
 * Errors come before anything is enqueued and leave the counts untouched: PT_ERR_INVALID for a field out of range, a reserved
 * field not 0, a camera pt_camera_derive rejects, counts not 8-byte or image not 16-byte aligned, counts and image overlapping,
 * a buffer of another device, frame_begin + frame_count or width x height above 2^31 - 1; PT_ERR_RANGE for a buffer too small
 * or (frame_begin + frame_count) x K above 2^32 - 1 (so that neither open nor K hits can wrap). */
typedef struct pt_ao_params {
    int32_t width, height;       /* the image */
    int32_t frame_begin;         /* first frame; 0 = the counts are overwritten, otherwise added to */
    int32_t frame_count;         /* >= 0; 0 enqueues nothing */
    int32_t num_triangles;       /* >= 0; 0 = every primary ray misses */
    int32_t rays_per_sample;     /* K, 1..256 */
    float radius;                /* finite, > 0: an occlusion ray counts hits at 0 < t < min(radius, 1e20) */
    float miss_value;            /* finite: the image value of a pixel none of whose samples hit the scene */
    int32_t stripe_rows, n_ranks, rank;   /* image sharding exactly as pt_render_params */
    int32_t reserved[5];         /* must be 0 */
} pt_ao_params;                  /* 64 bytes */
int pt_render_ao(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t counts, pt_buffer_t image /* may be NULL */,
                 const pt_ao_params* params, const pt_camera* cam /* NULL = the reference's */, pt_event_t ev);

/* ---- direct illumination -------------------------------------------------------------------------------------------
 * The DirectIllumination case the reference's harness declares (test/RaytraceTest.cpp:297-299) with an empty body: the emitted
 * light of the first hit plus one bounce of light sampled on the scene's emitters, composed of the reference's own steps.  Every
 * operation is binary32 under the arithmetic contract of the renderer (dot, cross, normalize, sqrt and "/" as there).
 * A sample of pixel gid = y * width + x in frame z:
 *  1. seed = gid + hash(z) (GenerateColors.cl:308), the renderer's primary ray (o, d) (:263-288) and its closest hit from 1e20
 *     (:137-154).  A miss gives L = max(0.45, 0) per channel (:235).
 *  2. On a hit: m = materials[the triangle's id, clamped into [0, num_materials) as shading clamps it]; E = 1.0f * m.emissive *
 *     3.0f (:241); p = o + d t (:127); n = the HitRecord normal (:128-130) turned to face the ray (:243); wo = -d.
 *  3. With nl = num_lights > 0, for k = 0 .. K-1 in order, on the same seed, S starting at 0:
 *     a. r0, r1, r2 = getRandomFloat(&seed), three times, always drawn whatever follows;
 *     b. j = lights[min((uint32)(r0 * (float)nl), nl - 1)], clamped into [0, num_triangles): an index out of range in the list
 *        is defined behaviour, never an out-of-range load;
 *     c. of triangle j: e1 = p2 - p1, e2 = p3 - p1 (:92-93), N = cross(e2, e1) (:123), nj = normalize(N), area = 0.5f *
 *        sqrt(dot(N, N)); su = sqrt(r1), b1 = 1.0f - su, b2 = r2 * su, q = (p1 + e1 * b1) + e2 * b2;
 *     d. dv = q - p, d2 = dot(dv, dv), dist = sqrt(d2), wi = normalize(dv), cs = dot(wi, n), cl = fabs(dot(wi, nj)) (emitters are
 *        two-sided, as :241 adds emission whichever side is hit).  The sample contributes only when cs > 0.0f && cl > 0.0f
 *        (false for NaN: q == p, a light of no area) and m.type is 1 or 2 (:220);
 *     e. the BRDF value: type 1: f = m.albedo * INV_PI (:203); type 2: wh = normalize(wo + wi), ct = dot(wh, n), D =
 *        distributionGGX(ct, m.roughness) (:174-178); f = 0 when dot(wi, n) * dot(wo, n) < 0 (:211), otherwise g = D / (4.0f *
 *        dot(wi, n) * dot(wo, n)) and f = (m.albedo * g) * 2.0f (:217);
 *     f. w = ((cs * cl) / d2) * (area * (float)nl); c = (f * (emissive of materials[id of j, clamped] * 3.0f)) * w per channel;
 *     g. the shadow ray getRay(p + wi * 0.01f, wi) (:257) with limit tl = min(dist - 0.02f, 1e20f) is occluded when any triangle
 *        passes the exact test (:96-125) at 0 < t < tl -- the any-hit search of pt_occluded_rays; tl <= 0 searches nothing and is
 *        open.  (The light lies at t ~ dist - 0.01, beyond the limit: no index is excluded.)  An open ray adds c to S.  A sample
 *        that does not contribute casts no ray.
 *  4. L = max(E + S / (float)K, 0) per channel with the reference's max; with num_lights = 0, S = 0: the renderer's radiance at
 *     max_bounces = 1, bit for bit.
 *  5. L goes to samples[frame - chunk's first][local pixel][3] (floats) and is folded into the framebuffer by the renderer's own
 *     fold, frames ascending: float4, the gamma-encoded running mean (:314-321), in the stripe layout of pt_render_params.
 *     frame_begin = 0 starts afresh; later frames resume the mean the buffer holds.
 * Sums are ordered per sample and the fold per pixel: the image does not depend on which lane or launch ran what.
 * samples: the caller's workspace, at least one frame (local pixels x 12 bytes).  The call walks its frames in chunks of
 * min(frames left, floor(bytes / (local pixels x 12)), floor((2^31 - 1) / local pixels)) frames: one launch and one fold per
 * chunk, on the handle's stream.  Direct renders behave like AO renders and queries: behind renders in flight, asynchronous (ev);
 * the scene, LBVH and filter tables as a query uses them (no anchor move, no rebuild); once the scene is prepared no allocation
 * and no wait; PT_OPT_ACCEL and PT_OPT_QUAD_FILTER choose the search; a cut-short LBVH search raises PT_ERR_TRAVERSAL (deferred).
 * num_triangles = 0 renders the background.
 * Errors come before anything is enqueued and leave the framebuffer untouched: PT_ERR_INVALID for a field out of range
 * (num_materials < 1, light_samples outside 1..256, num_lights < 0 or >= 2^24 -- (float)nl must be exact --, num_lights > 0 with
 * lights NULL), a reserved field not 0, a camera pt_camera_derive rejects, the framebuffer not 16-byte or samples / lights not
 * 4-byte aligned, samples, framebuffer and lights overlapping, a buffer of another device, frame_begin + frame_count or width x
 * height above 2^31 - 1; PT_ERR_RANGE for a buffer too small. */
typedef struct pt_direct_params {
    int32_t width, height, frame_begin, frame_count;   /* the image; frame_begin 0 = the framebuffer is overwritten; frame_count 0 enqueues nothing */
    int32_t num_triangles, num_materials, num_lights;  /* num_triangles >= 0, num_materials >= 1, 0 <= num_lights < 2^24 */
    int32_t light_samples;                             /* K, 1..256 */
    int32_t stripe_rows, n_ranks, rank;                /* image sharding exactly as pt_render_params */
    int32_t reserved[5];                               /* must be 0 */
} pt_direct_params;                                    /* 64 bytes */
int pt_render_direct(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                     pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, pt_buffer_t samples /* workspace */,
                     pt_buffer_t framebuffer, const pt_direct_params* params, const pt_camera* cam /* NULL = the reference's */,
                     pt_event_t ev);

/* ---- first-hit feature buffers -------------------------------------------------------------------------------------
 * What a denoiser, a compositor or a model takes beside the noisy image: albedo, shading normal, depth / coverage and emission at
 * the first hit, per SAMPLE, over the same jittered (and, with a lens, defocused) samples the lit renders take.  This call
 * neither filters nor denoises; pt_sample_moments turns each output into ordered binary64 sums, pt_moments_resolve into means and
 * variances, and pt_denoise takes the sums as the guides of its filter.  A sample of pixel gid = y * width + x in frame z is steps 1 and 2 of pt_render_direct, expression for expression:
 *  1. seed = gid + hash(z) (GenerateColors.cl:308), the renderer's primary ray (o, d) (:263-288; with the camera's lens when it has
 *     one) and its closest hit from 1e20 (:137-154).
 *  2. On a hit: p = o + d t (:127); n = the HitRecord normal (:128-130) turned to face the ray (:243: n when dot(n, d) < 0,
 *     otherwise n * -1.0f); m = materials[the triangle's id, clamped into [0, num_materials) as shading clamps it].
 * Item i = f * npix + lp -- frame frame_begin + f, local pixel lp of the stripe layout of pt_render_params, npix local pixels --
 * writes three floats to X[i] of every output X that is not NULL:
 *     albedo     m.albedo[0..2] as stored, whatever m.type          a miss: (0, 0, 0)
 *     normal     n                                                  a miss: (0, 0, 0)
 *     depth      (t, 1.0f, -dot(n, d)), the contract's dot          a miss: (0, 0, 0)
 *     emission   1.0f * m.emissive[0..2] * 3.0f (:241)              a miss: (0, 0, 0)
 * depth's second channel is the coverage weight: a pixel's mean depth over its hits is sum[0] / sum[1], its coverage sum[1] / n.
 * Nothing is clamped or filtered: the NaN normal of a degenerate triangle is stored as it is (pt_sample_moments counts the sample
 * as rejected).  The layout [frame][local pixel][3] is the sample workspace's: each output goes to pt_sample_moments as it is.
 * One launch per call, no chunking: every output given must hold frame_count x npix x 12 bytes, and frame_count x npix must stay
 * below 2^31.  frame_begin only numbers the frames: there is no framebuffer and nothing is accumulated here.
 * Feature renders behave like AO and direct renders: the handle's stream, behind renders in flight, asynchronous (ev); the scene,
 * LBVH and filter tables as a query uses them (no anchor move, no rebuild); once the scene is prepared no allocation and no wait;
 * PT_OPT_ACCEL and PT_OPT_QUAD_FILTER choose the search; a cut-short LBVH search raises PT_ERR_TRAVERSAL (deferred).
 * num_triangles = 0 writes misses.  The version of every buffer written is bumped.
 * Errors come before anything is enqueued and leave the outputs untouched: PT_ERR_INVALID for a field out of range (num_triangles
 * < 0, num_materials < 1), a reserved field not 0, a camera pt_camera_derive rejects, triangles or materials NULL, all four outputs
 * NULL, an output not 4-byte aligned, outputs overlapping each other or the triangle or material buffer, a buffer of another device,
 * frame_begin + frame_count or width x height above 2^31 - 1; PT_ERR_RANGE for a buffer too small or frame_count x npix above
 * 2^31 - 1. */
enum { PT_FEATURE_ALBEDO = 1, PT_FEATURE_NORMAL = 2, PT_FEATURE_DEPTH = 4, PT_FEATURE_EMISSION = 8 };   /* names for a caller's masks */
typedef struct pt_feature_params {
    int32_t width, height, frame_begin, frame_count;   /* the image; frame_begin numbers the frames; frame_count 0 enqueues nothing */
    int32_t num_triangles, num_materials;              /* num_triangles >= 0 (0 = every sample a miss), num_materials >= 1 */
    int32_t stripe_rows, n_ranks, rank;                /* image sharding exactly as pt_render_params */
    int32_t reserved[7];                               /* must be 0 */
} pt_feature_params;                                   /* 64 bytes */
int pt_render_features(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                       pt_buffer_t albedo, pt_buffer_t normal, pt_buffer_t depth, pt_buffer_t emission /* float[frame_count][npix][3]; each may be NULL */,
                       const pt_feature_params* params, const pt_camera* cam /* NULL = the reference's */, pt_event_t ev);

/* ---- indirect illumination -----------------------------------------------------------------------------------------
 * The IndirectIllumination case the reference's harness declares (test/RaytraceTest.cpp:301-303) with an empty body: the
 * renderer's multi-bounce walk (traceRays, GenerateColors.cl:223-261) with direct illumination's light sample taken at every
 * vertex of the path, not only the first.  Every operation is binary32 under the arithmetic contract of the renderer.
 * A sample of pixel gid in frame z, with B = max_bounces >= 1, K = light_samples and nl = num_lights:
 *  1. The seed, the primary ray (o, d) and the camera are exactly those of pt_render_direct step 1.  L = 0 and mask = 1 per channel.
 *  2. For i = 0 .. B-1: the closest hit of (o, d) from 1e20 (:137-154).  A miss gives L += mask * max(0.45, 0) (:235) and the path
 *     ends.  On a hit, in this order:
 *     a. the surface: m, p, n (turned to face the ray, :243) and wo = -d as in pt_render_direct step 2, the material's index clamped;
 *     b. the emission L.c = L.c + mask.c * m.emissive.c * 3.0f (:241, in that order), applied when i == 0 or nl == 0.  With a
 *        light list the emitted light of later vertices is what step c of the vertex before has sampled already, so it is not
 *        added a second time: THE LIST MUST HOLD EVERY EMISSIVE TRIANGLE of the scene for the image to be unbiased (the emitters
 *        of scene.emitters; a shorter list loses the light of the triangles left out at every vertex but the first);
 *     c. the light samples, when nl > 0: S = 0; K light samples on the same seed exactly as pt_render_direct steps 3a-3g at the
 *        vertex (p, n, wo, m) -- three uniforms always drawn per sample, the shadow ray through the any-hit search, an open ray
 *        adds c to S --; then L.c = L.c + mask.c * (S.c / (float)K);
 *     d. the BRDF sample: Brdf (:195-221) as the renderer shades it, two uniforms (phi first), giving wi, pdf and color;
 *        pdf <= 0 ends the path (:251); otherwise mask.c *= (color.c * dot(wi, n)) / pdf (three IEEE quotients, :253-255) and the
 *        next ray is getRay(p + wi * 0.01f, wi) (:257).  At i == B-1 the draw cannot be observed and may be skipped.
 *  3. L = max(L, 0) per channel with the reference's max (:260).
 *  4. L goes to the samples workspace and is folded by the renderer's fold exactly as pt_render_direct step 5; the chunks, the
 *     stripe layout and the frame_begin = 0 rule are direct's.
 * Light samples come before the BRDF sample at every vertex.  Two identities follow:
 *  - nl == 0: no light uniform is drawn, and the framebuffer is pt_render_frames' at the same max_bounces, bit for bit;
 *  - B == 1: the framebuffer is pt_render_direct's, bit for bit -- for emission that is not negative: with an emissive component
 *    of -0 direct forms E + S / K from E = -0 where this forms 0 + E = +0 first; that case is excluded.
 * Not done here: multiple importance sampling (a BRDF ray that finds a light adds nothing at i > 0, so glossy surfaces next to
 * a light are noisy; pt_render_indirect_mis below does it), light choice by power (every entry of the list is as likely as every
 * other; pt_render_indirect_power below does it), Russian roulette (every path walks all max_bounces vertices unless it misses or
 * draws pdf <= 0; pt_render_indirect_rr below does it).
 * Behaviour: pt_render_direct's, word for word -- the handle's stream, behind renders in flight, asynchronous (ev); the prepared
 * scene, LBVH and filter tables as a query uses them; no allocation and no wait once the scene is prepared; PT_OPT_ACCEL and
 * PT_OPT_QUAD_FILTER choose the search; PT_ERR_TRAVERSAL is deferred; num_triangles = 0 renders the background.  Errors are
 * pt_render_direct's, before anything is enqueued, plus PT_ERR_INVALID for max_bounces outside 1..65535. */
typedef struct pt_indirect_params {
    int32_t width, height, frame_begin, frame_count;   /* as pt_direct_params */
    int32_t num_triangles, num_materials, num_lights;
    int32_t light_samples;                             /* K, 1..256, per vertex */
    int32_t stripe_rows, n_ranks, rank;
    int32_t max_bounces;                               /* B, 1..65535 */
    int32_t reserved[4];                               /* must be 0 */
} pt_indirect_params;                                  /* 64 bytes */
int pt_render_indirect(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                       pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, pt_buffer_t samples /* workspace */,
                       pt_buffer_t framebuffer, const pt_indirect_params* params, const pt_camera* cam /* NULL = the reference's */,
                       pt_event_t ev);

/* ---- indirect illumination with multiple importance sampling ---------------------------------------------------------
 * pt_render_indirect's estimator with the balance heuristic between its two ways of finding a light: the light samples of a
 * vertex and the BRDF ray that leaves it.  A BRDF ray that runs into an emissive triangle at i > 0 adds its emission again,
 * and both contributions carry weights that sum to 1 for a direction that finds the front of a listed triangle, so glossy
 * surfaces next to a light stop being noisy.  A new estimator beside the old one: pt_render_indirect is unchanged.
 *
 * pt_light_counts writes counts[t] = the number of entries of lights[0 .. num_lights) whose index, clamped into [0,
 * num_triangles) as pt_render_direct step 3b clamps it, equals t.  counts: the caller's int32[num_triangles].  One clear and one
 * small kernel on the handle's stream, behind renders in flight, asynchronous (ev); nothing is allocated; num_lights = 0 clears;
 * num_triangles = 0 enqueues nothing.  Errors, before anything is enqueued: PT_ERR_INVALID for counts NULL, num_lights > 0 with
 * lights NULL, a negative size, num_lights >= 2^24, lights or counts not 4-byte aligned, the two overlapping, a buffer of another
 * device; PT_ERR_RANGE for a buffer too small.
 *
 * pt_render_indirect_mis takes pt_render_indirect's arguments and parameter block (all four reserved words 0) and light_counts,
 * an int32[num_triangles] as pt_light_counts writes it for the same list.  The estimator is pt_render_indirect's steps 1-4 with the
 * following changes, ALL OF THEM ONLY WHEN nl > 0; with K = light_samples, B = max_bounces, and every "/" an IEEE division:
 *  - A path carries one more value, pb: the pdf of the BRDF sample that made the current ray (step 2d's pdf, stored after the
 *    pdf <= 0 test).
 *  - A light sample (pt_render_direct steps 3a-3g, at any vertex) also forms sl = dot(wi, nj), so that cl = fabs(sl), and the
 *    density of the vertex's BRDF sample towards wi: type 1: pbl = cs * INV_PI (:201); type 2: pbl = D * ct / (4.0f * dot(wo, wh))
 *    (:215) from step 3e's wh, ct and D (formed whether or not :211 sets f = 0).  When i < B - 1 and sl > 0.0f, after step 3f:
 *    a = area * (float)nl; pe = d2 / (cl * a); kp = (float)K * pe; w = w * (kp / (kp * (float)counts[j] + pbl)).  Otherwise w is
 *    step 3f's, unchanged: at the last vertex no BRDF ray follows, and with sl <= 0 the vertex sees the light's back, the side the
 *    one-sided triangle test (:100) lets no ray hit, so no BRDF ray can share that sample's weight.  Both rules are part of the
 *    estimator, not options: without either the weights no longer sum to 1.
 *  - The emission at a later vertex: when i >= 1 and any component of m.emissive is != 0, with h the triangle hit, t the hit's
 *    distance, d the ray's direction and N = cross(e2, e1) of triangle h (:123): areah = 0.5f * sqrt(dot(N, N)); clh = fabs(dot(d,
 *    normalize(N))); tt = t + 0.01f (the ray began 0.01 off the vertex before, :257, so both techniques form pe from the same
 *    distance); pe = (tt * tt) / (clh * (areah * (float)nl)); wb = pb / (((float)K * pe) * (float)counts[h] + pb); L.c = L.c +
 *    ((mask.c * m.emissive.c) * 3.0f) * wb.  A hit on a material with no emissive component reads no count and adds nothing.  At
 *    i == 0 the emission is added as in step 2b.
 * Why the weights partition: for a direction that finds the front of triangle h, the counts[h] list entries that name it give the
 * light samples the density kp each against the BRDF's p, and counts[h] * kp / (kp * counts[h] + p) + p / (kp * counts[h] + p) = 1.
 * Because the count is per triangle, a duplicated entry, a missing emitter (counts[h] = 0: wb = 1, the BRDF ray carries all of it)
 * or an unsorted list leave the image unbiased AT EVERY VERTEX BUT THE LAST, where the light samples are unweighted and nothing
 * follows: there a duplicated entry still counts twice and an emitter missing from the list is still lost.  pt_render_indirect's
 * rule that the list must hold every emissive triangle is relaxed to that last vertex only.
 * Not changed by this: the bounded but large weight of a light sample that sees a light from its back at a short distance (a
 * ceiling vertex above a light that hangs just below it).
 * Identities: nl == 0: light_counts may be NULL and is not read, and the framebuffer is pt_render_frames' at the same
 * max_bounces, bit for bit; B == 1: the only vertex is the last, and the framebuffer is pt_render_direct's, bit for bit (under
 * pt_render_indirect's exclusion of an emissive component of -0).
 * Behaviour and errors: pt_render_indirect's, word for word -- one validation, one chunk loop, one fold --, plus, when num_lights
 * > 0: PT_ERR_INVALID for light_counts NULL, not 4-byte aligned, of another device, or overlapping samples, framebuffer or lights;
 * PT_ERR_RANGE for light_counts smaller than num_triangles x 4 bytes. */
int pt_light_counts(pt_device_t dev, pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, int num_lights, int num_triangles,
                    pt_buffer_t counts /* int32[num_triangles] */, pt_event_t ev);
int pt_render_indirect_mis(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                           pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */,
                           pt_buffer_t light_counts /* int32[num_triangles]; may be NULL when num_lights is 0 */,
                           pt_buffer_t samples /* workspace */, pt_buffer_t framebuffer, const pt_indirect_params* params,
                           const pt_camera* cam /* NULL = the reference's */, pt_event_t ev);

/* ---- light choice by power ---------------------------------------------------------------------------------------------
 * A second way to choose the light of a light sample, beside the uniform one, which is unchanged: entry i of the list is chosen in
 * proportion to the power its triangle emits, area x emission, so that one bright panel among many small dim emitters receives the
 * samples its light deserves.  The choice goes through a table that pt_light_table builds on the device, once per list.
 *
 * THE TABLE is integer on purpose: a float prefix sum depends on the order of the scan, an integer one does not, so the device may
 * scan in any order and still equal a sequential restatement bit for bit.  For entry i of lights[0 .. nl), nl = num_lights:
 *  1. j = lights[i] clamped into [0, num_triangles) as pt_render_direct step 3b clamps it; area = 0.5f * sqrt(dot(N, N)), N =
 *     cross(e2, e1), of triangle j as step 3c forms it; em = the emissive of materials[id of j, clamped into [0, num_materials)];
 *  2. p_i = area * ((em.x + em.y) + em.z), counted as 0 unless p_i > 0.0f && p_i < INFINITY (false for NaN, a light of no area, an
 *     entry that is no emitter);
 *  3. pmax = the largest p_i (of non-NaN floats: independent of the order);
 *  4. q_i = 0 when p_i is 0, otherwise max(1u, (uint32)((p_i / pmax) * 65536.0f)) with the IEEE "/": 1 .. 65536, and the floor of 1
 *     means that no emitter of positive power has probability 0;
 *  5. cdf[0] = 0, cdf[i + 1] = cdf[i] + q_i in uint64; total = cdf[nl] < 2^40;
 *  6. tri_q[t], a uint32 per triangle: the q of the entries that name t (they have one p, hence one q), 0 for a triangle no entry
 *     names.
 * cdf: the caller's buffer of pt_light_table_bytes(num_lights) bytes (0 for a num_lights out of range), at least 8 x (nl + 1): words
 * 0 .. nl are the cdf, whatever lies behind them is the build's scratch and unspecified.  tri_q: the caller's uint32[num_triangles].
 * triangles and materials are the scene's buffers as the render entry points take them.  Behaviour is pt_light_counts': one clear and
 * a few small kernels on the handle's stream, behind renders in flight, asynchronous (ev); nothing is allocated.  num_lights = 0
 * writes cdf[0] = 0 and clears tri_q; num_triangles = 0 writes a cdf of zeros.  Errors, before anything is enqueued: PT_ERR_INVALID for
 * a NULL handle (lights may be NULL when num_lights is 0), a negative size, num_materials < 1, num_lights >= 2^24, cdf not 8-byte or
 * tri_q / lights not 4-byte aligned, cdf or tri_q overlapping each other or an input, a buffer of another device; PT_ERR_RANGE for a
 * buffer too small.
 *
 * THE LIGHT SAMPLE with the table is pt_render_direct's steps 3a-3g with two changes:
 *  3b. u = min((uint32)(r0 * 16777216.0f), 16777215u) (getRandomFloat can return 1.0); x = (u * total) >> 24 in uint64 (u < 2^24 and
 *      total < 2^40: the product is below 2^64); i = the entry with cdf[i] <= x < cdf[i + 1] (binary search; an entry of q = 0 is
 *      never it); j = lights[i], clamped as before.  With total == 0 the three uniforms are drawn, the sample does not contribute
 *      and no ray is cast.
 *  3f. inv = (float)total / (float)(cdf[i + 1] - cdf[i]) (conversions to nearest, the IEEE "/"); w = ((cs * cl) / d2) * (area * inv):
 *      inv stands where (float)nl stood.
 * What the 24-bit uniform means: entry i is chosen for the u in [ceil(2^24 cdf[i] / total), ceil(2^24 cdf[i + 1] / total)), so the
 * probability with which it is really chosen differs from q_i / total, the one the weight assumes, by at most 2^-24 absolute -- the
 * granularity the uniform choice already has (its (uint32)(r0 * nl) of a 24-bit r0).
 * MIS keeps pt_render_indirect_mis' formulas and its two rules (the last vertex, sl <= 0): a = area * inv, so pe, kp and counts[j]
 * work as there; the later hit on an emissive triangle h forms, when counts[h] > 0, inv_h = (float)total / (float)tri_q[h] and puts
 * it where (float)nl stands in pe; with counts[h] == 0, wb = 1 and the table is not read.
 *
 * pt_render_direct_power and pt_render_indirect_power take their parents' arguments and parameter blocks (reserved words 0) and the
 * table; the indirect one also mis (0: pt_render_indirect's estimator, 1: pt_render_indirect_mis') and light_counts, which may be
 * NULL when mis == 0 or num_lights == 0.  Identities: a list of entries of bit-equal power whose number is a power of two dividing
 * 2^24 gives inv = nl and i = floor(u nl / 2^24) exactly: the parent's image bit for bit; num_lights == 0: the table may be NULL and is
 * not read, and the image is pt_render_frames'; B == 1: the indirect image is pt_render_direct_power's.
 * Behaviour and errors: the parents', word for word -- one validation, one chunk loop, one fold --, plus, when num_lights > 0:
 * PT_ERR_INVALID for cdf or tri_q NULL, cdf not 8-byte or tri_q not 4-byte aligned, of another device, or overlapping each other,
 * samples, framebuffer, lights or light_counts; PT_ERR_RANGE for cdf smaller than 8 x (num_lights + 1) bytes or tri_q smaller than
 * num_triangles x 4 bytes; PT_ERR_INVALID for mis other than 0 or 1. */
size_t pt_light_table_bytes(int num_lights);
int pt_light_table(pt_device_t dev, pt_buffer_t triangles, int num_triangles, pt_buffer_t materials, int num_materials,
                   pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, int num_lights,
                   pt_buffer_t cdf /* pt_light_table_bytes(num_lights) bytes */, pt_buffer_t tri_q /* uint32[num_triangles] */, pt_event_t ev);
int pt_render_direct_power(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                           pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, pt_buffer_t cdf, pt_buffer_t tri_q /* may be NULL when 0 */,
                           pt_buffer_t samples /* workspace */, pt_buffer_t framebuffer, const pt_direct_params* params,
                           const pt_camera* cam /* NULL = the reference's */, pt_event_t ev);
int pt_render_indirect_power(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                             pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, int mis,
                             pt_buffer_t light_counts /* int32[num_triangles]; may be NULL when mis or num_lights is 0 */,
                             pt_buffer_t cdf, pt_buffer_t tri_q /* may be NULL when num_lights is 0 */, pt_buffer_t samples /* workspace */,
                             pt_buffer_t framebuffer, const pt_indirect_params* params, const pt_camera* cam /* NULL = the reference's */,
                             pt_event_t ev);

/* ---- Russian roulette ----------------------------------------------------------------------------------------------------
 * The four indirect estimators -- pt_render_indirect, pt_render_indirect_mis, pt_render_indirect_power with mis 0 and 1 -- with paths
 * that may end early at random and are reweighted so that the expectation stays what it was: at the headline depth most of a
 * sample's searches are otherwise spent on vertices whose throughput is a few percent.  New estimators beside the old ones, which
 * are unchanged.  One entry point covers the four: mis as pt_render_indirect_power takes it; cdf and tri_q both NULL = the uniform
 * choice, both given = the choice by power.
 * The estimator is its parent's steps 1-4 with one addition at the end of step 2d, parameterised by R = first_bounce >= 1 and cap =
 * max_survival in (0, 1], B = max_bounces.  After the BRDF sample of vertex i has passed its pdf <= 0 test and mask has taken its
 * three quotients, the roulette applies when i + 1 >= R and i < B - 1 (at the last vertex nothing is drawn, as before).  When it
 * applies:
 *  1. r = getRandomFloat(&seed), drawn whatever follows;
 *  2. s = max(mask.x, max(mask.y, mask.z)) with the reference's max ((a < b) ? b : a); q = min(s, cap), the reference's min ((cap <
 *     s) ? cap : s).  A NaN mask.x, or NaN in both other channels, makes q NaN;
 *  3. q >= 1.0f: the path goes on with mask unchanged (getRandomFloat can return 1.0: r < q would wrongly end a path that must live);
 *  4. otherwise the path goes on if and only if r < q -- false for a NaN q, false for q <= 0 --, with mask.c = mask.c / q per channel:
 *     three IEEE divisions;
 *  5. a path that does not go on ends as a pdf <= 0 path does: L is stored (step 3).
 * With MIS, pb stays step 2d's pdf: it is NOT multiplied by q, and the light samples of vertex i are taken before the roulette.  Why
 * the weights still partition: for a direction that finds the front of triangle h, the light samples of vertex i carry counts[h] *
 * kp / (kp * counts[h] + p) of the light h sends along it, whatever the roulette does afterwards; the BRDF ray survives with
 * probability q and its contribution at vertex i + 1 is mask / q times the emission times wb = p / (kp * counts[h] + p), whose
 * expectation over the roulette is the unplayed path's mask * emission * wb.  The two weights are formed from the same p and kp as
 * without roulette and sum to 1; scaling pb by q would compare the BRDF sample's density in one measure with the light samples' in
 * another and break the partition.
 * Identities: R >= B: no roulette is played, no extra uniform is drawn, and the framebuffer is the parent's, bit for bit, for all
 * four estimators; num_lights == 0 and R >= B: it is pt_render_frames' at the same max_bounces.
 * Behaviour and errors: the parents', word for word -- one validation, one chunk loop, one fold, the handle's stream, the deferred
 * PT_ERR_TRAVERSAL --, plus, before anything is enqueued: PT_ERR_INVALID for roulette NULL, first_bounce < 1, max_survival NaN or
 * outside (0, 1], a reserved word of pt_roulette not 0, and exactly one of cdf / tri_q NULL while num_lights > 0. */
typedef struct pt_roulette {
    int32_t first_bounce;   /* R >= 1: vertex i plays when i + 1 >= R (R >= max_bounces: never) */
    float max_survival;     /* cap, in (0, 1] */
    int32_t reserved[2];    /* must be 0 */
} pt_roulette;              /* 16 bytes */
int pt_render_indirect_rr(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                          pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, int mis,
                          pt_buffer_t light_counts /* int32[num_triangles]; may be NULL when mis or num_lights is 0 */,
                          pt_buffer_t cdf, pt_buffer_t tri_q /* both NULL = the uniform choice */, pt_buffer_t samples /* workspace */,
                          pt_buffer_t framebuffer, const pt_indirect_params* params, const pt_roulette* roulette,
                          const pt_camera* cam /* NULL = the reference's */, pt_event_t ev);

/* ---- sample moments: per-pixel noise estimates of the lit renders -----------------------------------------------------------
 * Every lit entry point (pt_render_direct, pt_render_indirect and their _mis / _power forms) leaves each sample's linear radiance in
 * the caller's workspace, samples[frame - call's first][local pixel][3], before the fold.  These calls take the first and second
 * moments per pixel from that workspace on the device, and from the moments a per-pixel variance map and an image-wide noise figure
 * that is read back in 48 bytes.  No reference counterpart; no existing kernel, entry point or image changes.  The workspace holds
 * the frames of the LAST chunk of a render call (pt_render_direct step 5), so a caller who wants every frame counted renders at most as
 * many frames per call as the workspace holds and calls pt_sample_moments after each.
 *
 * pt_sample_moments, per pixel p of num_pixels (one lane per pixel; the frames are NOT split over lanes and merged):
 *  1. with reset != 0 the record starts from zeros and the buffer's old contents are not read; otherwise from moments[p];
 *  2. for f = 0 .. frame_count - 1 IN ASCENDING ORDER, with (x, y, z) = samples[f][p][0..2] (binary32):
 *     - all three finite: n = n + 1; per channel v: sum = sum + (double)v and sum2 = sum2 + (double)v * (double)v, each operation
 *       rounded on its own in binary64 (the product of two converted binary32 values is exact in binary64, so contraction could not
 *       change it);
 *     - otherwise (a NaN or an infinity in any channel): rejected = rejected + 1 and nothing else changes;
 *  3. the record is written back.  n and rejected wrap modulo 2^32.
 * The order over the frames is part of the contract: the sums equal a sequential restatement bit for bit, and two calls of a and b
 * frames equal one call of a + b frames.  Sums, not Welford's recurrence: sums of different calls, chunks or ranks merge exactly (add
 * them) and need no division per sample.  The price: pt_moments_resolve forms sum2 - sum * mean, which cancels when a pixel's variance
 * lies below about n * 2^-53 of its squared mean; such a pixel resolves to a variance of 0, or to a rounding residue of that size where
 * the difference happens to come out positive -- never to a negative one.
 *
 * pt_moments_resolve, per pixel, in binary64 with every operation rounded on its own (no contraction) and the IEEE "/":
 *  1. per channel: m = n > 0 ? sum / (double)n : 0;  with n >= 2: t = sum * m; d = sum2 - t; v = d / (double)(n - 1); v = v > 0 ? v : +0
 *     (the unbiased sample variance);  with n < 2: v = 0;
 *  2. noise (may be NULL): struct { float var[3]; uint32_t n; }[num_pixels], 16 bytes each: var = (float)v, rounded once;
 *  3. summary (may be NULL): the caller's buffer of pt_moments_summary_bytes(num_pixels) bytes.  Its first 48 bytes receive a
 *     pt_noise_summary; what lies behind them is the build's scratch and unspecified (nothing is allocated: pt_light_table's pattern).
 *     A pixel with n >= 2 contributes a = (v.x + v.y) + v.z to var_sum, b = ((v.x / n) + (v.y / n)) + (v.z / n) to se2_sum (the squared
 *     standard error of its mean), c = ((m.x * m.x) + (m.y * m.y)) + (m.z * m.z) to mean2_sum and 1 to pixels; every other pixel
 *     contributes +0 and is not counted.  samples and rejected sum n and rejected over ALL pixels (uint64).
 *     The three floating sums are taken by a FIXED TREE, so that the device's order is specified and a restatement can follow it: the
 *     per-pixel values are padded with +0 to the next power of two, and each level is x'[i] = x[2 i] + x[2 i + 1] until one value is
 *     left.  (The device reduces tiles of 2 048 pixels by adjacent-pair butterflies and runs the same kernel on the tile sums: exactly
 *     this tree -- every contribution is >= +0, so further padding with +0 changes nothing.  Three launches cover 2^32 - 1 pixels.)
 * From the summary: the mean variance per sample and channel is var_sum / (3 pixels); sqrt(se2_sum / mean2_sum) is the image's
 * relative standard error, the figure a progressive render stops on.
 *
 * Behaviour of both calls is pt_light_counts': the handle's stream, behind renders in flight, asynchronous (ev); nothing is
 * allocated and the host waits for nothing; the version of each buffer written is bumped.  frame_count = 0 or num_pixels = 0 runs no
 * kernel and touches no buffer, whatever reset says.
 * Errors, before anything is enqueued: PT_ERR_INVALID for a NULL handle (noise and summary may be NULL), a negative frame_count,
 * moments or summary not 8-byte aligned, noise not 16-byte aligned, samples not 4-byte aligned, any two of the buffers overlapping, a
 * buffer of another device; PT_ERR_RANGE for a buffer too small (samples: frame_count x num_pixels x 12 bytes; moments: num_pixels x
 * 56; noise: num_pixels x 16; summary: pt_moments_summary_bytes(num_pixels)). */
typedef struct pt_pixel_moments { double sum[3]; double sum2[3]; uint32_t n; uint32_t rejected; } pt_pixel_moments;   /* 56 bytes */
typedef struct pt_noise_summary { double var_sum, se2_sum, mean2_sum; uint64_t pixels, samples, rejected; } pt_noise_summary;   /* 48 bytes */
int pt_sample_moments(pt_device_t dev, pt_buffer_t samples /* float[frame_count][num_pixels][3] */,
                      pt_buffer_t moments /* pt_pixel_moments[num_pixels] */, uint32_t num_pixels, int32_t frame_count, int reset,
                      pt_event_t ev);
size_t pt_moments_summary_bytes(uint32_t num_pixels);
int pt_moments_resolve(pt_device_t dev, pt_buffer_t moments /* pt_pixel_moments[num_pixels] */, uint32_t num_pixels,
                       pt_buffer_t noise /* may be NULL */, pt_buffer_t summary /* may be NULL */, pt_event_t ev);

/* ---- adaptive sampling: later frames only for the pixels that are still noisy ---------------------------------------------
 * The moments are per pixel; these calls act on them per pixel.  pt_adaptive_select turns the moments into a LIST of the pixels
 * whose mean is not yet good enough, pt_render_indirect_pixels renders further frames of the listed pixels only, each continuing from
 * its own frame number, and pt_sample_moments_pixels counts those samples.  No reference counterpart; no existing kernel, entry
 * point or image changes.  A pixel's samples depend on its global id and the frame number alone, and its fold chain on its own frames
 * in ascending order, so THE IDENTITY holds: after any sequence of these calls, pixel p of the framebuffer holds exactly the bits a
 * uniform render (pt_render_indirect_rr over frames [0, n_p)) holds for p, n_p being the number of samples p has received.
 *
 * A LIST is a buffer: bytes 0-15 {uint32 count; uint32 reserved[3]}, then pt_pixel_slot[count], 8 bytes each: the LOCAL pixel and the
 * number of its next frame.
 *
 * pt_adaptive_select, per local pixel p of num_pixels, from its record moments[p] (pt_pixel_moments):
 *  1. taken = (uint64)n + (uint64)rejected;
 *  2. with n >= 2, in binary64, every operation rounded on its own (no contraction), the IEEE "/" -- pt_moments_resolve's step 1 and
 *     its se2_sum and mean2_sum terms, expression for expression: per channel m = sum / (double)n; t = sum * m; d = sum2 - t;
 *     v = d / (double)(n - 1); v = v > 0 ? v : +0;  b = ((v.x / n) + (v.y / n)) + (v.z / n);  c = ((m.x * m.x) + (m.y * m.y)) +
 *     (m.z * m.z);
 *  3. p is ACTIVE iff taken < max_samples && (n < min_samples || (n >= 2 && b > tol2 * (c + floor2))).  The inequality is strict,
 *     and a comparison with a NaN is false (a sum that has overflowed, tol2 = 0 against c = infinity: inactive);
 *  4. the list receives count = the number of active pixels, reserved = 0, and the active pixels' slots IN ASCENDING ORDER OF p:
 *     {pixel = p, frame = (uint32)taken}.
 * list: the caller's buffer of pt_adaptive_list_bytes(num_pixels) bytes; what lies behind the slots is the build's scratch and
 * unspecified (nothing is allocated: pt_light_table's pattern).  The compaction is ordered -- per-tile counts, their scan, a scatter
 * -- and all integer, so the list does not depend on the order of the scan.  The moments are only read.  num_pixels = 0 writes a
 * header of zeros.  Behaviour is pt_moments_resolve's: the handle's stream, asynchronous (ev), no allocation, no wait.
 * Errors, before anything is enqueued: PT_ERR_INVALID for a NULL handle, rule NULL, tol2 or floor2 negative or NaN, a reserved
 * field not 0, moments or list not 8-byte aligned, the two overlapping, a buffer of another device; PT_ERR_RANGE for a buffer too small
 * (moments: num_pixels x 56; list: pt_adaptive_list_bytes(num_pixels)).
 *
 * pt_render_indirect_pixels takes pt_render_indirect_rr's arguments -- through the same validation -- plus list and num_listed, the
 * count the HOST has read from the list's header: the device never reads the count.  num_listed must not exceed the local pixel
 * count.  With npix = the local pixels and F = params->frame_count, the frames PER LISTED PIXEL, item i of a launch is frame f = i /
 * num_listed of slot j = i % num_listed:
 *  1. its local pixel is min(slot[j].pixel, npix - 1): an out-of-range slot is defined behaviour, as a light index is, never an
 *     out-of-range access;
 *  2. its frame number is z = (slot[j].frame + params->frame_begin + f) & 0x7fffffff (f counted from the call's first frame);
 *  3. from there on it is pt_render_indirect_rr's sample of that pixel in frame z: the stripe mapping to the global pixel id, seed = gid
 *     + hash(z), the primary ray, the same walk with the same estimator (mis; cdf and tri_q; the roulette);
 *  4. the sample goes to samples[i]: the workspace is laid out [frames][num_listed][3], pt_render_direct step 5's with num_listed for
 *     the local pixels.  The frames are walked in chunks of min(frames left, floor(bytes / (num_listed x 12)), floor((2^31 - 1) /
 *     num_listed)); the workspace must hold one frame of the list;
 *  5. each chunk is followed by a LIST FOLD: one lane per (slot, channel) folds samples[f][j], f ascending, into framebuffer[the slot's
 *     pixel] by the renderer's fold with the frame numbers of step 2.  A frame number 0 overwrites the pixel, as frame 0 does in every
 *     render; every other one resumes the mean the pixel holds.
 * Pixels that are not listed are neither read nor written.  THE SLOTS MUST NAME DISTINCT PIXELS (pt_adaptive_select's do): duplicates,
 * which out-of-range slots clamped to the last pixel also are, race in the fold, so the pixel's VALUE is undefined -- but there is
 * never an out-of-range access.  roulette may not be NULL: first_bounce >= max_bounces plays none, so all four estimators are reached
 * with and without roulette through this one entry point; max_bounces = 1 is direct illumination.  The stream, the prepared scene, the
 * deferred PT_ERR_TRAVERSAL: pt_render_indirect_rr's.  frame_count = 0 or num_listed = 0 enqueues nothing.
 * Errors: pt_render_indirect_rr's (the workspace: one frame of num_listed pixels), plus PT_ERR_INVALID for list NULL, of another
 * device, not 8-byte aligned, overlapping the workspace or the framebuffer, num_listed above the local pixel count; PT_ERR_RANGE for a
 * list smaller than 16 + num_listed x 8 bytes.
 *
 * pt_sample_moments_pixels: moments[min(slot[j].pixel, P - 1)], P = the whole records the moments buffer holds (floor(bytes / 56): the
 * local pixels of a buffer sized for them), takes samples[f][j][0..2] for f = 0 .. frame_count - 1 ascending by pt_sample_moments' step
 * 2; one lane per listed pixel; it never resets.  Records that are not listed are neither read nor written.  Behaviour and errors are
 * pt_sample_moments', plus PT_ERR_INVALID for list NULL, not 8-byte aligned, overlapping, num_listed > P and PT_ERR_RANGE for a list
 * smaller than 16 + num_listed x 8 bytes. */
typedef struct pt_adaptive_rule {
    double tol2;             /* >= 0: the squared relative standard error a pixel must reach */
    double floor2;           /* >= 0: added to the squared mean, so that a black pixel can stop */
    uint32_t min_samples;    /* a pixel with fewer finite samples is active whatever its variance */
    uint32_t max_samples;    /* a pixel that has received this many samples (finite or rejected) is inactive */
    uint32_t reserved[2];    /* must be 0 */
} pt_adaptive_rule;          /* 32 bytes */
typedef struct pt_pixel_slot { uint32_t pixel; uint32_t frame; } pt_pixel_slot;   /* local pixel, its next frame number */
size_t pt_adaptive_list_bytes(uint32_t num_pixels);
int pt_adaptive_select(pt_device_t dev, pt_buffer_t moments /* pt_pixel_moments[num_pixels] */, uint32_t num_pixels,
                       const pt_adaptive_rule* rule, pt_buffer_t list /* pt_adaptive_list_bytes(num_pixels) bytes */, pt_event_t ev);
int pt_render_indirect_pixels(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                              pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, int mis,
                              pt_buffer_t light_counts /* int32[num_triangles]; may be NULL when mis or num_lights is 0 */,
                              pt_buffer_t cdf, pt_buffer_t tri_q /* both NULL = the uniform choice */, pt_buffer_t samples /* workspace */,
                              pt_buffer_t framebuffer, pt_buffer_t list, uint32_t num_listed, const pt_indirect_params* params,
                              const pt_roulette* roulette, const pt_camera* cam /* NULL = the reference's */, pt_event_t ev);
int pt_sample_moments_pixels(pt_device_t dev, pt_buffer_t samples /* float[frame_count][num_listed][3] */,
                             pt_buffer_t moments /* pt_pixel_moments[] */, pt_buffer_t list, uint32_t num_listed, int32_t frame_count,
                             pt_event_t ev);

/* ---- resampled light sampling (RIS) ---------------------------------------------------------------------------------------
 * Every estimator above chooses the light of a light sample without looking at the shading point: in a room of many emitters of
 * similar power the choice by power is the uniform choice, and almost every shadow ray goes to a light that is far away, faces
 * away or contributes little.  A shadow ray is the expensive part of a light sample -- on the LBVH a whole any-hit search --, a
 * candidate (three uniforms, one table lookup, a BRDF value, a geometry term) needs no search.  Resampled importance sampling draws
 * M = candidates of them from the table, keeps one in proportion to its unshadowed contribution at this vertex and casts the one ray.
 * New estimators beside the old ones, which are unchanged.
 *
 * RIS replaces a light sample: steps 3a-3g of pt_render_direct in the table form of "light choice by power", with the MIS weighting
 * of pt_render_indirect_mis where MIS is on.  1 <= M <= 32, a run-time value.  RIS requires the table: cdf and tri_q are needed
 * whenever num_lights > 0; there is no uniform-choice form.
 * For light sample k of a vertex: wsum = 0, have = false; for m = 0 .. M - 1, in this order:
 *  1. r0, r1, r2 are drawn and candidate m is evaluated exactly as the light sample by power is (3a-3g with 3b and 3f of the table):
 *     it contributes or not, and if it does it has c_m, the shadow ray (o_m, d_m) and its limit tl_m = min(dist - 0.02f, 1e20f).  With
 *     MIS c_m carries the balance factor kp / (kp * counts[j] + pbl) when the vertex is not the last and sl > 0, with the same kp = K
 *     * pe formed from the table's inv.  A table of total 0 draws the three uniforms and does not contribute.
 *  2. if m >= 1: r = getRandomFloat(&seed), drawn whether or not the candidate contributes.  A light sample therefore always consumes
 *     4M - 1 uniforms, and M = 1 the parent's three.
 *  3. if the candidate contributes: s_m = max(c.x, max(c.y, c.z)) with the reference's max ((a < b) ? b : a).  If s_m > 0 (false for
 *     NaN): wsum = wsum + s_m; then candidate m is kept (its c, o, d, tl, s) and have = true if and only if !have or r * wsum < s_m
 *     -- the product is one binary32 multiplication.  (A reservoir of one: candidate m replaces the kept one with probability s_m / wsum.)
 * After the loop: !have: no ray is cast and nothing is added.  Otherwise g = (wsum / (float)M) / s_sel, two generic IEEE divisions
 * (the operands have no proven window for a short form), and c = c_sel * g per channel.  The shadow ray is the parent's in every
 * respect: tl <= 0 is open and unsearched, otherwise the any-hit search up to tl, and S += c when open.  An infinite s gives a NaN
 * sample (inf / inf); that is defined behaviour, and pt_sample_moments rejects it.
 * Why it is unbiased: c_m is (the integrand without visibility) / (the source density q_i / total x 1 / area, in solid angle).  The
 * target s_m is its largest channel, positive wherever any channel of the integrand is, for materials that are not negative.  The
 * kept candidate's c_sel x V x (mean of the M weights s_m) / s_sel is the RIS estimator of the integral of integrand x visibility:
 * its expectation over the kept index and then over the candidates is that of one candidate's c_m x V, which is the parent's.
 * Why the MIS weights still partition: the light-side factor kp * counts / (kp * counts + pbl) is part of the candidate's integrand;
 * the BRDF ray's wb is untouched; both are formed from the same source densities as without RIS and sum to 1 for every direction,
 * and any partition of unity is unbiased.  This is NO LONGER the balance heuristic with respect to the resampled density, which is
 * intractable: it is the parent's weights applied to a better light technique.  The two MIS rules are unchanged: the last vertex
 * is not weighted, sl <= 0 is not weighted.
 * Identities: M = 1 draws nothing extra and has g = 1.0f exactly (wsum = s, s / 1 = s, s / s = 1 for a finite s > 0), so framebuffer
 * and workspace are the parent's bit for bit -- pt_render_direct_power for pt_render_direct_ris, pt_render_indirect_rr with the table
 * for pt_render_indirect_ris, pt_render_indirect_pixels for pt_render_indirect_pixels_ris -- on every input where each contributing
 * light sample has a finite c with s > 0, or c = 0 in all channels (the parent casts a ray for a zero c and adds zero; RIS casts
 * none).  num_lights == 0 is the parent's image for every M.  B == 1: the indirect image is pt_render_direct_ris' at the same M.
 *
 * The three entry points take their parents' arguments -- pt_render_direct_power's, pt_render_indirect_rr's (R >= B plays no
 * roulette, as there), pt_render_indirect_pixels' -- plus the pt_ris block.  Behaviour and errors: the parents', word for word -- one
 * validation, one chunk loop, one fold, the handle's stream, the deferred PT_ERR_TRAVERSAL --, plus, before anything is enqueued,
 * PT_ERR_INVALID for ris NULL, candidates outside 1 .. 32, a reserved word of pt_ris not 0, and cdf or tri_q NULL while num_lights > 0. */
typedef struct pt_ris {
    int32_t candidates;     /* M, 1 .. 32 */
    int32_t reserved[3];    /* must be 0 */
} pt_ris;                   /* 16 bytes */
int pt_render_direct_ris(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                         pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, pt_buffer_t cdf, pt_buffer_t tri_q /* may be NULL when 0 */,
                         pt_buffer_t samples /* workspace */, pt_buffer_t framebuffer, const pt_direct_params* params, const pt_ris* ris,
                         const pt_camera* cam /* NULL = the reference's */, pt_event_t ev);
int pt_render_indirect_ris(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                           pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, int mis,
                           pt_buffer_t light_counts /* int32[num_triangles]; may be NULL when mis or num_lights is 0 */,
                           pt_buffer_t cdf, pt_buffer_t tri_q /* may be NULL when num_lights is 0 */, pt_buffer_t samples /* workspace */,
                           pt_buffer_t framebuffer, const pt_indirect_params* params, const pt_roulette* roulette, const pt_ris* ris,
                           const pt_camera* cam /* NULL = the reference's */, pt_event_t ev);
int pt_render_indirect_pixels_ris(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                                  pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, int mis,
                                  pt_buffer_t light_counts /* int32[num_triangles]; may be NULL when mis or num_lights is 0 */,
                                  pt_buffer_t cdf, pt_buffer_t tri_q /* may be NULL when num_lights is 0 */, pt_buffer_t samples /* workspace */,
                                  pt_buffer_t framebuffer, pt_buffer_t list, uint32_t num_listed, const pt_indirect_params* params,
                                  const pt_roulette* roulette, const pt_ris* ris, const pt_camera* cam /* NULL = the reference's */,
                                  pt_event_t ev);

/* ---- environment lighting: an octahedral sky map ------------------------------------------------------------------------------
 * Every estimator above gives a ray that leaves the scene the constant max(0.45, 0) (:235).  These two take the sky from a map of
 * the caller's, look it up where a ray misses, and SAMPLE it: Ke environment samples per vertex, chosen through an integer table
 * in proportion to what a texel emits into its solid angle, balanced against the BRDF ray as the emitter samples are.  New
 * estimators beside the old ones, which are unchanged.  Every operation is binary32 under the renderer's arithmetic contract (dot,
 * normalize, sqrt and the IEEE "/" as there); sgn(v) = (v < 0.0f) ? -1.0f : 1.0f (-0 and NaN give +1).
 *
 * THE MAP: env = float4[N * N], row-major, w ignored; N a power of two, 1 <= N <= 2048; y is up.  Texels are used as they are: a
 * negative or NaN texel is the caller's business.  An octahedral map, because it needs no atan2 or acos: only fabs, +, *, "/", sqrt.
 *  - The index of a coordinate c: v = ((c + 1.0f) * 0.5f) * (float)N; !(v >= 0.0f) gives 0 (a NaN, a negative); v >= (float)(N - 1)
 *    gives N - 1 (an infinity too); otherwise (uint32)v, which the conversion defines because 0 <= v < N - 1.  Never out of range.
 *  - Direction to texel, for ANY d: s = (fabs(d.x) + fabs(d.y)) + fabs(d.z); x = d.x / s; z = d.z / s; with d.y >= 0.0f (true for -0)
 *    (a, b) = (x, z), otherwise -- a NaN d.y too -- (a, b) = ((1.0f - fabs(z)) * sgn(x), (1.0f - fabs(x)) * sgn(z)); texel = index(b) * N +
 *    index(a); Le(d) is its value.  A NaN direction has v = NaN in both coordinates: texel 0.
 *  - (a, b) to the octahedron's point: h = (1.0f - fabs(a)) - fabs(b); h >= 0.0f: P = (a, h, b), otherwise P = ((1.0f - fabs(b)) *
 *    sgn(a), h, (1.0f - fabs(a)) * sgn(b)); P2 = dot(P, P); r = sqrt(P2); the direction is normalize(P).
 *  - The solid angle of da db at P is da db / r^3 (the plane |x| + |y| + |z| = 1 lies at distance 1 / sqrt(3) and its area element is
 *    sqrt(3) da db); for a direction d, r = sqrt(dot(d, d)) / s.  A direction of a texel of table weight q therefore has the density
 *    pdf = (((float)q / (float)total) * (((float)N * (float)N) * 0.25f)) * ((r * r) * r) per solid angle.
 *
 * pt_env_table builds the table as pt_light_table builds its own, on its layout, tiling and scans, for the N * N texels in row-major
 * order: texel i = row * N + col has the centre (a, b) = (((float)col + 0.5f) * (2.0f / (float)N) - 1.0f, likewise of row), P and rc =
 * sqrt(dot(P, P)) as above, and the weight p_i = ((Le.x + Le.y) + Le.z) * (1.0f / ((rc * rc) * rc)), counted as 0 unless p_i > 0.0f &&
 * p_i < INFINITY; pmax, q_i = max(1, (uint32)((p_i / pmax) * 65536.0f)) (0 where p_i is 0) and the uint64 prefix sum cdf[0 .. N * N]
 * are pt_light_table's steps 3-5.  There is no second table: q_i = cdf[i + 1] - cdf[i].  cdf: pt_env_table_bytes(N) bytes (0 for an N
 * out of range); words 0 .. N * N are the table, what lies behind is the build's scratch.  Integer, so equal to a sequential
 * restatement bit for bit.  Behaviour is pt_light_table's; errors, before anything is enqueued: PT_ERR_INVALID for a NULL handle, N
 * not a power of two in 1..2048, env not 16-byte or cdf not 8-byte aligned, the two overlapping, a buffer of another device;
 * PT_ERR_RANGE for a buffer too small.
 *
 * pt_render_direct_env is pt_render_direct_power's estimator, pt_render_indirect_env is pt_render_indirect_rr's with mis = 1 and the
 * choice by power (cdf and tri_q; with num_lights == 0 lights, light_counts, cdf and tri_q may all be NULL), with these changes,
 * Ke = env_samples:
 *  - A MISS of a ray of direction d adds Le(d) where max(0.45, 0) stood.  Direct: L = max(Le(d).c, 0).  Indirect: L.c = L.c + mask.c *
 *    Le(d).c; at a vertex i >= 1 with Ke > 0 it is weighted, L.c = L.c + mask.c * (Le(d).c * wb), wb = pb / ((float)Ke * pdf(d) + pb) with
 *    pdf(d) formed from the texel's q and r = sqrt(dot(d, d)) / s; q == 0 or total == 0 gives wb = 1.0f.
 *  - AFTER THE K LIGHT SAMPLES of a vertex, Ke environment samples on the same seed, Se starting at 0.  For each:
 *     a. r0, r1, r2 = getRandomFloat(&seed), always drawn;
 *     b. total = cdf[N * N]; total == 0: the sample does not contribute.  Otherwise texel i by the table exactly as step 3b of the
 *        choice by power: u = min((uint32)(r0 * 16777216.0f), 16777215u), x = (u * total) >> 24, cdf[i] <= x < cdf[i + 1]; q = cdf[i + 1]
 *        - cdf[i]; col = i % N, row = i / N;
 *     c. (a, b) = (((float)col + r1) * (2.0f / (float)N) - 1.0f, ((float)row + r2) * (2.0f / (float)N) - 1.0f);
 *     d. P, P2, r as above; wi = normalize(P); cs = dot(wi, n);
 *     e. it contributes only when cs > 0.0f (false for NaN) and m.type is 1 or 2;
 *     f. f and, with MIS, pbl from pt_render_direct step 3e and pt_render_indirect_mis, unchanged;
 *     g. pdf as above from q, total and r; w = cs / pdf; c = (f * Le_i) * w per channel, Le_i the chosen texel's value -- the direction
 *        is not looked up a second time;
 *     h. indirect, when i < B - 1: kp = (float)Ke * pdf; w = w * (kp / (kp + pbl)) before c is formed;
 *     i. the shadow ray getRay(p + wi * 0.01f, wi) with limit 1e20f through the any-hit search; an open ray adds c to Se.
 *    Then indirect: L.c = L.c + mask.c * (Se.c / (float)Ke); direct: L = max((E + S / (float)K) + Se / (float)Ke, 0).  With Ke == 0
 *    nothing is drawn and nothing is added (no 0 / 0).
 *  - The order at a vertex: surface, emission, light samples, environment samples, BRDF sample, roulette.  The last vertex's
 *    environment samples are unweighted, for the reason its light samples are: no BRDF ray follows.
 * Why the weights partition: emitters and sky are disjoint sources -- a direction either finds a triangle or leaves the scene --, so
 * each is balanced against the BRDF ray alone.  For a direction that leaves the scene the Ke environment samples have the density kp
 * = Ke pdf against the BRDF's pb, and kp / (kp + pb) + pb / (kp + pb) = 1; the emitter samples never produce such a direction with an
 * open ray, and the environment samples never find an emitter (their ray is occluded by it).  The roulette leaves pb as it is.
 * Identities, bit for bit in workspace and framebuffer:
 *  - every texel (0.45, 0.45, 0.45) and Ke == 0: the parent's, pt_render_direct_power / pt_render_indirect_rr with mis = 1 and the table,
 *    for every N, every search and with or without roulette;
 *  - B == 1: the indirect form is the direct form (under pt_render_indirect's exclusion of an emissive component of -0, and for
 *    texels without a component of -0: direct keeps max(-0, 0) = -0 where indirect forms 0 + -0 = +0);
 *  - num_triangles == 0: every sample is max(Le(d), 0) of its primary ray, the map seen through the camera.
 * Behaviour and errors: the parents', word for word -- one validation, one chunk loop, one fold, the handle's stream, the deferred
 * PT_ERR_TRAVERSAL --, plus, before anything is enqueued: PT_ERR_INVALID for environment NULL, size not a power of two in 1..2048,
 * env_samples outside 0..256, a reserved word not 0, env NULL, env_cdf NULL while env_samples > 0, env not 16-byte or env_cdf not 8-byte
 * aligned, either overlapping any other buffer of the call, a buffer of another device; PT_ERR_RANGE for env smaller than N * N * 16
 * bytes or env_cdf smaller than 8 * (N * N + 1) bytes.  env_cdf is not read when env_samples == 0. */
typedef struct pt_environment {
    int32_t size;           /* N: a power of two, 1 .. 2048 */
    int32_t env_samples;    /* Ke, 0 .. 256, per vertex */
    int32_t reserved[2];    /* must be 0 */
} pt_environment;           /* 16 bytes */
size_t pt_env_table_bytes(int size);
int pt_env_table(pt_device_t dev, pt_buffer_t env /* float4[size * size] */, int size, pt_buffer_t cdf /* pt_env_table_bytes(size) bytes */,
                 pt_event_t ev);
int pt_render_direct_env(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                         pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, pt_buffer_t cdf, pt_buffer_t tri_q /* may be NULL when 0 */,
                         pt_buffer_t env, pt_buffer_t env_cdf /* may be NULL when env_samples is 0 */, pt_buffer_t samples /* workspace */,
                         pt_buffer_t framebuffer, const pt_direct_params* params, const pt_environment* environment,
                         const pt_camera* cam /* NULL = the reference's */, pt_event_t ev);
int pt_render_indirect_env(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                           pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */,
                           pt_buffer_t light_counts, pt_buffer_t cdf, pt_buffer_t tri_q /* may be NULL when num_lights is 0 */,
                           pt_buffer_t env, pt_buffer_t env_cdf /* may be NULL when env_samples is 0 */, pt_buffer_t samples /* workspace */,
                           pt_buffer_t framebuffer, const pt_indirect_params* params, const pt_roulette* roulette,
                           const pt_environment* environment, const pt_camera* cam /* NULL = the reference's */, pt_event_t ev);

/* ---- radiance queries: path-traced radiance along the caller's rays ---------------------------------------------------------------
 * pt_radiance_rays is pt_render_indirect_rr with the third sample start: the item's primary ray is read from a buffer of pt_ray, not
 * made by a camera for a pixel.  Light probes, lightmap and vertex baking, irradiance sensors, panoramic, orthographic or fisheye
 * cameras and per-ray radiance for a model trained elsewhere are all this call over rays the caller makes.
 *
 * THE ITEM.  With n = num_rays, item i = s * n + r is sample sample_begin + s of ray r:
 *   - its seed is (first_ray + r) + hash(sample_begin + s) in uint32 -- the renderers' gid + hash(frame), :308, with the ray's id
 *     first_ray + r standing for the pixel and the sample's number for the frame;
 *   - its primary ray is getRay(origin, dir) of rays[r] (:73-77): loaded and normalised exactly as pt_intersect_rays does it (a
 *     zero-length or non-finite direction is defined behaviour there and here: the search finds nothing or what IEEE makes of it);
 *   - NO uniform is drawn before the walk (the renderers draw the two jitter uniforms, and the lens two more);
 *   - tmax and reserved of the record are NOT read: a radiance ray is unbounded, as every path segment is;
 *   - from there on it is pt_render_indirect_rr's sample from its closest search from 1e20 on, word for word: the estimator chosen by
 *     mis and cdf / tri_q (both NULL = the uniform choice), K = light_samples per vertex, B = max_bounces vertices, the roulette
 *     (first_bounce >= B plays none);
 *   - samples[i] receives max(L, 0), 12 bytes: the layout [sample][ray][3] is the sample workspace's.
 * Put differently: a call computes pt_render_indirect_rr's workspace for an image of first_ray + num_rays x 1 pixels whose pixel id
 * starts at rays[id - first_ray] with no jitter draw.  Two calls over rays [0, a) and [a, n) with first_ray 0 and a equal one call.
 *
 * CHUNKS.  The samples are walked in chunks of min(samples left, floor(bytes of `samples` / (n x 12)), floor((2^31 - 1) / n)); there
 * is no framebuffer and no fold.  With `moments` given, each chunk is followed by pt_sample_moments' accumulation over it, in ascending
 * sample order, and `reset` applies to the first chunk only: one call of a + b samples equals two calls of a and b (reset, then not)
 * bit for bit, and the workspace may hold as little as one sample of every ray.  With moments == NULL the workspace must hold all
 * sample_count x n x 12 bytes (PT_ERR_RANGE otherwise: earlier chunks would be overwritten unseen).
 *
 * BEHAVIOUR is pt_render_indirect_rr's: the handle's stream, behind the work in flight, asynchronous (ev); the prepared scene, LBVH and
 * filter tables as a query uses them -- no anchor move, no rebuild; no allocation and no host wait once the scene is prepared;
 * PT_OPT_ACCEL and PT_OPT_QUAD_FILTER choose the search; PT_ERR_TRAVERSAL is deferred; num_triangles = 0 gives the background
 * (0.45 per channel); the versions of `samples` and `moments` are bumped.  num_rays = 0 or sample_count = 0 enqueues nothing and
 * touches no buffer, the moments with `reset` set included.
 *
 * ERRORS come before anything is enqueued and leave the buffers untouched: the parents' checks on scene, lights, counts, table,
 * roulette, K, B and reserved words; PT_ERR_INVALID for rays == NULL, rays or moments of another device, rays not 16-byte aligned,
 * moments not 8-byte aligned, samples not 4-byte aligned, any two of rays, samples, moments overlapping each other or the light
 * buffers, a negative sample_begin or sample_count, first_ray + num_rays or sample_begin + sample_count above 2^31 - 1; PT_ERR_RANGE
 * for rays smaller than n x 32 bytes, moments smaller than n x 56 bytes, a workspace that does not hold one sample of every ray, or
 * all of them when moments is NULL.
 * Not here: a ray set per sample, tmax on the first segment, resampling, the environment and pixel lists for rays. */
typedef struct pt_radiance_params {
    uint32_t num_rays;       /* n; 0 enqueues nothing */
    uint32_t first_ray;      /* the id of rays[0]: ray r has id first_ray + r; first_ray + num_rays <= 2^31 - 1 */
    int32_t  sample_begin;   /* >= 0: samples [sample_begin, sample_begin + sample_count) of every ray; the sum <= 2^31 - 1 */
    int32_t  sample_count;   /* >= 0; 0 enqueues nothing */
    int32_t  num_triangles, num_materials, num_lights, light_samples;   /* as pt_indirect_params */
    int32_t  max_bounces;    /* B, 1..65535 */
    int32_t  reset;          /* != 0: the moments start from zeros at this call's first chunk (pt_sample_moments' reset) */
    int32_t  reserved[6];    /* must be 0 */
} pt_radiance_params;        /* 64 bytes */
int pt_radiance_rays(pt_device_t dev, pt_buffer_t triangles, pt_buffer_t materials,
                     pt_buffer_t lights /* int32[num_lights]; may be NULL when 0 */, int mis,
                     pt_buffer_t light_counts /* mis only */, pt_buffer_t cdf, pt_buffer_t tri_q /* both NULL = uniform choice */,
                     pt_buffer_t rays /* pt_ray[num_rays] */, pt_buffer_t samples /* workspace */,
                     pt_buffer_t moments /* pt_pixel_moments[num_rays]; may be NULL */,
                     const pt_radiance_params* params, const pt_roulette* roulette /* not NULL; first_bounce >= B plays none */,
                     pt_event_t ev);

/* ---- the denoiser: a feature-guided a-trous filter over the moments ------------------------------------------------------
 * An image-space filter over records the library already writes: the lit renderers' per-pixel moments of the radiance
 * (pt_sample_moments) and the moments of pt_render_features' albedo, normal, depth and emission samples over the same frames.  No
 * reference counterpart; no existing kernel, entry point or image changes.  The filter is the edge-avoiding a-trous wavelet with a
 * variance-driven luminance term: `levels` passes of one 5 x 5 kernel whose taps lie 1 << i pixels apart in pass i, each tap
 * weighted down by how far its depth, albedo, emission, normal and -- measured against the pixel's own noise -- luminance lie from
 * the centre's.  The arithmetic below IS the contract: binary32 unless said otherwise, every operation rounded on its own (no
 * contraction), the IEEE "/" and sqrt, sums in the stated order.  A restatement that follows it equals `out` bit for bit.
 *
 * PREPARE, per pixel p = y * width + x (every quotient a binary64 division, rounded once to binary32):
 *  - colour: c[k] = (float)(n > 0 ? sum[k] / (double)n : 0) from colour[p];
 *  - with v[k] of pt_moments_resolve's step 1 and n >= 2: var = (float)(((v[0] / n) + (v[1] / n)) + (v[2] / n)), binary64 (that
 *    call's b: the squared standard error of the pixel's mean, summed over the channels); with n < 2: var = 0;
 *  - a, nrm, e: the means of albedo[p], normal[p], emission[p] by the colour's rule (nrm is not renormalised);
 *  - z = sum[1] > 0 ? (float)(sum[0] / sum[1]) : 0 from depth[p] (the mean t over the pixel's hits);
 *  - gx = 0.5f * (z(x + 1, y) - z(x - 1, y)), gy = 0.5f * (z(x, y + 1) - z(x, y - 1)), neighbour coordinates clamped into the image.
 * LEVEL i = 0 .. levels - 1, s = 1 << i, per pixel p = (x, y) from the level's input (c, var) -- prepare's for i = 0, the output of
 * level i - 1 otherwise; a, nrm, e, z, gx, gy stay prepare's:
 *  - l = (c[0] + c[1]) + c[2] (of p and of every tap);
 *  - the variance prefilter gv = (sum of k * var_q) / (sum of k), both sums from +0 over the taps dy = -1 .. 1 (outer), dx = -1 .. 1
 *    (inner), q = (x + dx, y + dy) (NOT scaled by s), taps outside the image skipped, k = kk[|dx|] * kk[|dy|], kk = (0.5f, 0.25f);
 *  - den_l = sigma_l * sqrt(gv) + eps_l;
 *  - sw, sc[0..2], sv start at +0; taps dy = -2 .. 2 (outer), dx = -2 .. 2 (inner), q = (x + dx s, y + dy s) (exact integers), taps
 *    outside the image skipped, h = kw[|dx|] * kw[|dy|], kw = (0.375f, 0.25f, 0.0625f):
 *      the centre tap: w = h, whatever the pixel holds (so sw >= 9/64 for finite inputs);
 *      every other tap: X = 0, then in this order
 *        depth:    t = (gx_p * (float)(dx s)) + (gy_p * (float)(dy s));  X = X + fabs(z_p - z_q) / (sigma_z * fabs(t) + eps_z)
 *        albedo:   d = a_p - a_q;  X = X + (((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])) / sigma_a
 *        emission: d = e_p - e_q;  X = X + (((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])) / sigma_e
 *        always:   X = X + fabs(l_p - l_q) / den_l
 *      Y = 1.0f + X * 0.0625f;  Y = Y * Y, four times;  w = h / Y   (h / (1 + X / 16)^16 stands in for h exp(-X): no exp here)
 *        normal:   D = ((nrm_p[0] * nrm_q[0]) + (nrm_p[1] * nrm_q[1])) + (nrm_p[2] * nrm_q[2]);  D = D > 0 ? D : 0;  D = D * D,
 *                  normal_squarings times;  w = w * D
 *      sw = sw + w;  sc[k] = sc[k] + w * c_q[k];  sv = sv + (w * w) * var_q;
 *  - the level's output: c[k] = sc[k] / sw, var = sv / (sw * sw).
 * out[p] = (c[0], c[1], c[2], var) after the last level; levels = 0 writes prepare's.  A guide that is NULL drops its term: no depth
 * = no depth term, no albedo / emission = that term left out of X, no normal = w is not multiplied by D.  Non-finite sums give what
 * IEEE makes of these expressions.
 *
 * scratch: the caller's buffer of pt_denoise_scratch_bytes(width, height) bytes (a function of width x height alone; 0 for an
 * invalid size); its contents are the build's and unspecified -- here six binary32 float4 planes: (c, var), (nrm, z), (a, gx),
 * (e, gy) and two for the levels to alternate between.  No guide is stored narrower than binary32.
 * PT_OPT_DENOISE_TILE chooses how a level gathers its taps; every setting gives the same bits (the tap order is per pixel).
 * Behaviour is pt_moments_resolve's: the handle's stream, behind work in flight, asynchronous (ev); nothing is allocated and the
 * host waits for nothing; the versions of out and scratch are bumped.  The image is the WHOLE image: the records of a striped or
 * multi-rank render are not one.
 * Errors come before anything is enqueued and leave the buffers untouched: PT_ERR_INVALID for dev, colour, scratch, out or params
 * NULL, a buffer of another device, width or height < 1, width x height > 2^31 - 1, levels or normal_squarings outside 0 .. 8, a
 * sigma or an eps that is not finite and > 0, a reserved word not 0, a moments buffer not 8-byte aligned, out or scratch not 16-byte
 * aligned, any two of the buffers overlapping; PT_ERR_RANGE for a buffer too small (a moments buffer: width x height x 56 bytes;
 * out: width x height x 16; scratch: pt_denoise_scratch_bytes). */
typedef struct pt_denoise_params {
    int32_t width, height;        /* the WHOLE image; width x height <= 2^31 - 1, both >= 1 */
    int32_t levels;               /* 0 .. 8 a-trous levels; level i has step 1 << i; 0 = prepare only */
    int32_t normal_squarings;     /* 0 .. 8: the normal weight is max(dot, 0)^(2^k) by k squarings */
    float   sigma_l, sigma_z, sigma_a, sigma_e;   /* finite, > 0 */
    float   eps_l, eps_z;                         /* finite, > 0 */
    int32_t reserved[6];          /* must be 0 */
} pt_denoise_params;              /* 64 bytes */
size_t pt_denoise_scratch_bytes(int32_t width, int32_t height);
int pt_denoise(pt_device_t dev, pt_buffer_t colour /* pt_pixel_moments[width x height] */,
               pt_buffer_t albedo, pt_buffer_t normal, pt_buffer_t depth, pt_buffer_t emission /* the same records; each may be NULL */,
               pt_buffer_t scratch, pt_buffer_t out /* float4[width x height]: r, g, b, variance */,
               const pt_denoise_params* params, pt_event_t ev);

/* ---- the denoiser for pixels that hold a single sample: a pooled variance before the levels --------------------------------
 * pt_denoise's prepare gives a pixel with n < 2 the variance 0: one sample carries none.  A level then forms den_l = eps_l, the
 * luminance term sends every tap but the centre to weight 0, and the pixel passes through unfiltered -- a one-frame render
 * whole, and after a camera move (pt_reproject) the pixels that took no history.  pt_denoise_spatial is pt_denoise with one pass
 * between PREPARE and the levels: a pixel whose own variance is unknown takes the pooled per-sample variance of its guide-similar
 * 7 x 7 neighbourhood, as the squared standard error of its own mean.  pt_denoise itself, its parameter block, its scratch size
 * and its bits do not change.  The arithmetic below IS the contract: binary32 unless it says binary64, every operation rounded on
 * its own (no contraction), the IEEE "/", sums in the stated order.  A restatement that follows it equals `out` bit for bit.
 *
 * PREPARE is pt_denoise's, for every pixel.
 * POOL, per pixel p = (x, y) with 1 <= n_p < below, n_p = colour[p].n:
 *  - Wn, A[0..2], B[0..2] are binary64 and start at +0; taps dy = -3 .. 3 (outer), dx = -3 .. 3 (inner), q = (x + dx, y + dy), taps
 *    outside the image skipped:
 *      the centre tap: w = 1.0f;
 *      every other tap: X = 0, then in this order
 *        depth:    t = (gx_p * (float)dx) + (gy_p * (float)dy);  X = X + fabs(z_p - z_q) / (sigma_z * fabs(t) + eps_z)
 *        albedo, emission: exactly the level's two terms
 *        (there is NO luminance term: the pixel's noise, which would scale it, is what is being estimated)
 *      Y = 1.0f + X * 0.0625f;  Y = Y * Y, four times;  w = 1.0f / Y
 *        normal:   the level's D (clamped at 0, squared normal_squarings times);  w = w * D
 *      with C = colour[q] and wd = (double)w:  Wn = Wn + wd * (double)C.n;  A[k] = A[k] + wd * C.sum[k];
 *      B[k] = B[k] + wd * C.sum2[k]   (each product and each sum rounded on its own);
 *  - per channel: M = A[k] / Wn;  T = M * M;  V = B[k] / Wn - T;  V = V > 0 ? V : +0;  Q[k] = V / (double)n_p;
 *  - var_p = (float)((Q[0] + Q[1]) + Q[2]).  The centre tap gives Wn >= n_p >= 1 for finite inputs.
 * A pixel with n_p = 0 or n_p >= below keeps PREPARE's var; c never changes.  A guide that is NULL drops its term as in the levels;
 * with no guide at all the pool is a 7 x 7 box.
 * LEVELS are pt_denoise's, run from (c, var); levels = 0 writes (c, var) with the pooled values in channel 3.
 * Identity: with below <= 1 no pixel is named and the bits of out equal pt_denoise's.  below = 2 names exactly the pixels whose
 * variance is unknown and is the recommended value: replacing the own two- or three-sample variance of a pixel by the pooled one
 * measured worse (a firefly's own variance is what lets the levels blur it away; profiles/denoise_spatial/quality.txt).
 *
 * Everything pt_denoise documents holds word for word: the buffers, the validation, errors before anything is enqueued, the
 * behaviour, and the scratch -- still pt_denoise_scratch_bytes (the pass writes one channel of the (c, var) plane).
 * PT_OPT_DENOISE_SPATIAL_FORM chooses how the pass gathers its taps; every setting gives the same bits.
 * Errors, added to pt_denoise's: PT_ERR_INVALID for spatial NULL, below < 0, a reserved word of spatial not 0. */
typedef struct pt_denoise_spatial_params {
    int32_t below;                /* >= 0: a pixel with 1 <= n < below takes the pooled variance; 0 and 1 name no pixel */
    int32_t reserved[7];          /* must be 0 */
} pt_denoise_spatial_params;      /* 32 bytes */
int pt_denoise_spatial(pt_device_t dev, pt_buffer_t colour, pt_buffer_t albedo, pt_buffer_t normal, pt_buffer_t depth,
                       pt_buffer_t emission, pt_buffer_t scratch, pt_buffer_t out,
                       const pt_denoise_params* params, const pt_denoise_spatial_params* spatial, pt_event_t ev);

/* ---- temporal reprojection: carry the moments across a camera move --------------------------------------------------------
 * The other half of a preview that survives a camera move: each pixel of the NEW view re-projects its first hit into the PREVIOUS
 * view and, where the same surface was seen there, takes that view's history -- its radiance moments -- over.  The inputs are records
 * the library already writes: the lit renderers' moments (pt_sample_moments) as the previous camera saw them, and the normal and depth
 * moments of pt_render_features under both cameras (depth samples are (t, 1, -dot(n, d)): sum[0] / sum[1] is the mean t over a pixel's
 * hits, sum[2] / sum[1] the mean incidence cosine).  The scene is static: a pixel's motion comes from the two cameras and its own
 * depth alone.  out_colour is the history ALONE, as cur_cam sees it; the moments are sums, so the caller accumulates the new camera's
 * samples on top of it with pt_sample_moments(..., reset = 0).  No reference counterpart; no existing kernel, entry point or image
 * changes.  The arithmetic below IS the contract: binary32 unless it says binary64, every operation rounded on its own (no
 * contraction), the IEEE "/" and sqrt, sums in the stated order, every comparison written so that a NaN makes it false.  A
 * restatement that follows it equals out_colour and out_info bit for bit.
 *
 * Here dot(a, b) = ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]), and vector operations act component by component.  Both cameras
 * are derived on the host exactly as pt_camera_derive derives them -- eye, viewDir, holDir, upDir, angle; primed names are prev_cam's
 * --, and the host forms, once, invWidth = 1.0f / (float)width, invHeight = 1.0f / (float)height, aspect = (float)width /
 * (float)height and cos_min2 = cos_min * cos_min.  mean(R) of a moment record R is (float)(R.sum[k] / (double)R.n), k = 0 .. 2, or 0
 * for R.n = 0; depth(R) is (float)(R.sum[0] / R.sum[1]).
 * Per pixel p = (x, y), index y * width + x.  Every pixel starts as a zero record in out_colour and (0, 0, 0, 0) in out_info; a step
 * that says "stop" leaves what has been written so far.
 *  1. D = cur_depth[p].  Unless D.sum[1] > 0, stop (no coverage, no history).  z = depth(D), cz = (float)(D.sum[2] / D.sum[1]).
 *  2. The pixel-centre ray of cur_cam (GenerateColors.cl:281-284 with the jitter at its centre):
 *       xs = (2.0f * (((float)x + 0.5f) * invWidth) - 1.0f) * angle * aspect;   ys = -(1.0f - 2.0f * (((float)y + 0.5f) * invHeight)) * angle;
 *       w = (holDir * xs + upDir * (-1.0f * ys)) + viewDir;   dir = w * (1.0f / sqrt(dot(w, w)));   P = eye + dir * z.
 *  3. P seen from prev_cam: v = P - eye';  dz = dot(v, viewDir').  Unless dz > 0, stop.
 *       a = dot(v, holDir') / dz;   b = dot(v, upDir') / dz;
 *       fx = ((a / (angle' * aspect) + 1.0f) * 0.5f) * (float)width - 0.5f;   fy = ((1.0f - b / angle') * 0.5f) * (float)height - 0.5f;
 *       r = sqrt(dot(v, v)).
 *  4. Unless fx > -1 && fx < (float)width && fy > -1 && fy < (float)height, stop.  x0 = (int)floor(fx), tx = fx - (float)x0; y0 and
 *     ty likewise from fy.  c = cz > 0.125f ? cz : 0.125f.  With both normal buffers given, nc = mean(cur_normal[p]).
 *  5. Four taps, dy = 0, 1 (outer), dx = 0, 1 (inner), q = (x0 + dx, y0 + dy); Wd, Nn, M[0..2], S[0..2] are binary64 and start at +0:
 *       - a tap outside the image is skipped;
 *       - bw = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty);
 *       - skipped when prev_colour[q].n == 0, or unless prev_depth[q].sum[1] > 0;
 *       - the depth test: z_q = depth(prev_depth[q]); skipped unless fabs(z_q - r) * c <= tol_z * r  (the surface the tap saw lies
 *         at the distance P has from the old eye; the cosine loosens the tolerance on a surface seen at a slant);
 *       - the normal test, only with both normal buffers given: nq = mean(prev_normal[q]) (neither mean is renormalised);
 *         Dn = dot(nc, nq); skipped unless Dn > 0 && Dn * Dn >= cos_min2 * (dot(nc, nc) * dot(nq, nq));
 *       - the noise test, only with max_noise > 0, in binary64 with C = prev_colour[q] and n_q = (double)C.n: m[k] = C.sum[k] / n_q;
 *         B = 0 for C.n < 2, otherwise with v[k] = (C.sum2[k] - C.sum[k] * m[k]) / (double)(C.n - 1), v[k] = v[k] > 0 ? v[k] : 0
 *         (pt_moments_resolve's step 1): B = ((v[0] / n_q) + (v[1] / n_q)) + (v[2] / n_q), the squared standard error of the tap's
 *         mean; skipped unless B <= (double)max_noise * (((m[0] * m[0]) + (m[1] * m[1])) + (m[2] * m[2])).  A record whose mean is
 *         one rare bright sample among dark ones has B equal to its squared mean, whatever its n: it knows no more than that one
 *         sample, and a history is not taken from it (the new view's own samples start the pixel afresh);
 *       - with C = prev_colour[q] and n_q = (double)C.n:  Wd = Wd + (double)bw;  Nn = Nn + (double)bw * n_q;
 *         M[k] = M[k] + (double)bw * (C.sum[k] / n_q);  S[k] = S[k] + (double)bw * (C.sum2[k] / n_q).
 *  6. out_info[p] = (fx, fy, (float)Wd, 0).  Unless Wd >= (double)min_weight && Wd > 0, stop.  N = Nn / Wd;
 *     N = N < (double)max_history ? N : (double)max_history;  n_h = (uint32)floor(N).  When n_h == 0, stop.
 *  7. out_colour[p]: sum[k] = (M[k] / Wd) * (double)n_h, sum2[k] = (S[k] / Wd) * (double)n_h, n = n_h, rejected = 0;
 *     out_info[p].w = (float)n_h.
 * So max_history = 0, and a prev_colour of zero records, write zero records.  With both cameras equal the result is close to, not
 * equal to, the history capped at max_history: the round trip of steps 2 and 3 is exact to about 1e-4 pixel, not exactly.
 * Non-finite inputs give what IEEE makes of these expressions.
 *
 * scratch: the caller's buffer of pt_reproject_scratch_bytes(width, height) bytes (a function of width x height alone; 0 for an
 * invalid size); its contents are the build's and unspecified -- here one float4 per pixel of the previous view, (nq, z_q), with a
 * NaN z_q standing for a tap step 5 skips for what the tap itself holds (no samples, no coverage, the noise test).  PT_OPT_REPROJECT_FORM chooses between that form and one kernel
 * that reads the records directly; both give the same bits.
 * Behaviour is pt_denoise's: the handle's stream, behind work in flight, asynchronous (ev); nothing is allocated and the host waits
 * for nothing; the versions of out_colour, out_info and scratch are bumped.  The image is the WHOLE image.
 * Errors come before anything is enqueued and leave the buffers untouched: PT_ERR_INVALID for dev, prev_colour, prev_depth,
 * cur_depth, scratch, out_colour or params NULL, a buffer of another device, width or height < 1, width x height > 2^31 - 1,
 * max_history < 0, tol_z not finite and > 0, cos_min not finite in [0, 1], min_weight not finite in [0, 1), max_noise not finite
 * and >= 0, a reserved word not 0,
 * exactly one of the two normal buffers given, a camera pt_camera_derive rejects, a camera with lens_radius > 0 (the geometry above
 * is the pinhole's), a moments buffer not 8-byte aligned, out_info or scratch not 16-byte aligned, any two of the buffers
 * overlapping; PT_ERR_RANGE for a buffer too small (moments: width x height x 56 bytes; out_info: width x height x 16). */
typedef struct pt_reproject_params {
    int32_t width, height;        /* the WHOLE image; width x height <= 2^31 - 1, both >= 1 */
    int32_t max_history;          /* >= 0: the cap on the history length a pixel takes over */
    float   tol_z;                /* finite, > 0: the relative depth tolerance of a tap */
    float   cos_min;              /* finite, in [0, 1]: the least cosine between the two mean normals */
    float   min_weight;           /* finite, in [0, 1): the least sum of the surviving taps' bilinear weights */
    float   max_noise;            /* finite, >= 0: the largest squared standard error of a tap's mean, relative to its squared mean; 0 = no noise test */
    int32_t reserved[9];          /* must be 0 */
} pt_reproject_params;            /* 64 bytes */
size_t pt_reproject_scratch_bytes(int32_t width, int32_t height);
int pt_reproject(pt_device_t dev,
                 pt_buffer_t prev_colour /* pt_pixel_moments[width x height], the history, seen from prev_cam */,
                 pt_buffer_t prev_normal /* feature moments under prev_cam; may be NULL */,
                 pt_buffer_t prev_depth /* feature moments under prev_cam; required */,
                 pt_buffer_t cur_normal /* feature moments under cur_cam; may be NULL */,
                 pt_buffer_t cur_depth /* feature moments under cur_cam; required */,
                 pt_buffer_t scratch,
                 pt_buffer_t out_colour /* pt_pixel_moments[width x height]: the history as cur_cam sees it */,
                 pt_buffer_t out_info /* float4[width x height], may be NULL: (fx, fy, weight, history length) */,
                 const pt_reproject_params* params, const pt_camera* prev_cam, const pt_camera* cur_cam /* NULL = the reference's */,
                 pt_event_t ev);

/* Per-kernel device timing for measurement (bench.py "roofline"): when enabled, every launch of
 * the trace / fold kernels is bracketed by a HIP event pair on the device's stream.
 * pt_profile_query synchronises the stream and returns the summed duration and launch count
 * since the last reset.  Reference hook: Device::toggleProfiling + LauncherCL::launch2D's
 * stopwatch (Adl/CL/AdlKernelUtilsCL.cpp:470-487), which the reference test never enables. */
enum { PT_PROF_TRACE = 0, PT_PROF_FOLD = 1, PT_PROF_KINDS = 2 };
int pt_profile_enable(pt_device_t dev, int on);
int pt_profile_query(pt_device_t dev, int kind, double* total_ms, uint64_t* launches);
/* The time during which AT LEAST ONE launch of the kind was executing (the union of the launches' [start, stop] intervals):
 * with PT_OPT_RENDER_LANES 2 consecutive trace launches overlap -- the next one's first workgroups start while the previous
 * one's last paths drain -- so the sum of their durations counts that time twice; the union is the machine time they took. */
int pt_profile_query_union(pt_device_t dev, int kind, double* union_ms);
int pt_profile_reset(pt_device_t dev);

/* Test hook: a read-only copy of the LBVH that stands for the scene this device prepared last (built by the first render, query or
 * AO call that searched it through the hierarchy: PT_OPT_ACCEL), for a check of the hierarchy that is independent of the builder
 * (tests/bvh_check.py).  Frames deferred by PT_OPT_BATCH_FRAMES are submitted first, as by every call that observes the device
 * (that is the caller's own work: it may prepare a scene and build its hierarchy); then the call waits for the device and looks.
 * The snapshot itself changes nothing: no preparation, no rebuild (PT_OPT_BVH_BUILD_COUNT stands), no filter anchor moves.  `info` receives the number of 64-byte records in use (eight-child nodes and one-triangle leaves of one
 * array, record 0 the root: csrc/pt_kernels.h), the grid of the nodes' 16-bit origins, the number of triangles kept out of the
 * hierarchy and the triangle count of the scene; `records` (may be NULL) receives the records -- record_capacity of them must
 * fit -- and `big_indices` (may be NULL; room for PT_BVH_SNAPSHOT_BIG_MAX) the indices of the triangles kept out, ascending.
 * PT_ERR_INVALID when no LBVH stands for the prepared scene, PT_ERR_RANGE when record_capacity is too small (info is still
 * filled). */
#define PT_BVH_SNAPSHOT_BIG_MAX 64
typedef struct pt_bvh_info {
    uint32_t records;            /* records in use */
    int32_t num_big;             /* triangles kept out of the hierarchy, 0..PT_BVH_SNAPSHOT_BIG_MAX */
    int32_t num_triangles;       /* triangles of the prepared scene */
    float grid_min[3], grid_step[3];   /* a node's origin on axis a is fma(org[a], grid_step[a], grid_min[a]) */
    int32_t reserved[7];
} pt_bvh_info;                   /* 64 bytes */
int pt_bvh_snapshot(pt_device_t dev, pt_bvh_info* info, void* records, size_t record_capacity, int32_t* big_indices);

/* Test hook: a read-only copy of the primary-ray candidate masks this device made last (PT_OPT_PRIMARY_MASKS: quad scenes of up
 * to 64 triangles on the brute-force path; one pair of 32-bit words per LOCAL pixel, in the framebuffer's order -- word c holds
 * triangles [32 c, 32 c + n), n = min(32, num_triangles - 32 c), triangle 32 c + j at bit n - 1 - j; a set bit = pass 2 tests the
 * triangle for that pixel's primary rays).  Frames deferred by PT_OPT_BATCH_FRAMES are submitted first; then the call waits for
 * the renders in flight and copies.  It changes nothing: no masks are made, no scene is prepared.  `num_pixels` receives the number
 * of local pixels the table stands for; `masks` (may be NULL) receives 8 bytes per pixel -- `capacity` pixels must fit.
 * PT_ERR_INVALID when no table stands (no render has used masks yet, or its scene has been replaced), PT_ERR_RANGE when
 * capacity is too small (num_pixels is still filled). */
int pt_primary_mask_snapshot(pt_device_t dev, uint32_t* num_pixels, void* masks, size_t capacity);

/* Test hook: a read-only copy of the secondary-ray candidate masks of the scene in hand (PT_OPT_SECONDARY_MASKS).  `info` receives
 * {entries, triangles, T, C}: entries = triangles * T * T * 6 * C * C; entry ((k T + iu) T + iv) 6 C C + (face C + ia) C + ib is the
 * cell of origin triangle k, tile (iu, iv) of its plane and direction cell (face, ia, ib) -- csrc/pt_secmask.h says which rays map
 * to it -- in the word format of pt_primary_mask_snapshot.  `masks` (may be NULL) receives 8 bytes per entry; `capacity` entries
 * must fit.  It changes nothing: no table is made, no scene is prepared.  PT_ERR_INVALID when no table stands for the prepared
 * scene (none rendered yet, or the scene declined it: more than 64 triangles, not made of quads, through the LBVH, the option 0 at
 * every render so far), PT_ERR_RANGE when capacity is too small (info is still filled). */
int pt_secondary_mask_snapshot(pt_device_t dev, uint32_t info[4], void* masks, size_t capacity);

/* Scatter the gathered per-rank local framebuffers (n_ranks slabs of slab_rows x width
 * float4 each, slab k = rank k) into the full image (height x width float4). */
int pt_assemble_stripes(pt_device_t dev, pt_buffer_t gathered, pt_buffer_t image, int width,
                        int height, int stripe_rows, int n_ranks, int slab_rows, pt_event_t ev);

/* The same on a stream of the caller's (a hipStream_t, e.g. torch.cuda.Stream().cuda_stream) instead of the device
 * handle's: rank 0 of an N-rank render assembles image k behind its collective while render k + 1 already occupies the
 * handle's stream (the reference is single-device and has no counterpart).  The caller orders the stream
 * against the producer of `gathered` and the consumers of `image` (events); deferred frames are submitted first. */
int pt_assemble_stripes_on(pt_device_t dev, pt_buffer_t gathered, pt_buffer_t image, int width, int height,
                           int stripe_rows, int n_ranks, int slab_rows, void* hip_stream);

/* Output stage on the device: rgb8[i] = f2c(sqrtf(fb[i].xyz))
 * of test/RaytraceTest.cpp:78-83,280-285, written as int32 triplets (what "%d %d %d " prints). */
int pt_tonemap_ppm(pt_device_t dev, pt_buffer_t framebuffer, pt_buffer_t rgb_i32, size_t num_pixels,
                   pt_event_t ev);

#ifdef __cplusplus
}
#endif
#endif /* PT_SHIM_H */
