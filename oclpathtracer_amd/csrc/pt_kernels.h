// pt_kernels.h -- host-callable launchers of the gfx950 kernels (pt_kernels.hip).
// Internal to libptshim.so; the public boundary is include/pt_shim.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// The reference's packed 64-byte device records (GenerateColors.cl:12-28).
struct PtRawTriangle { float p1[4], p2[4], p3[4]; int32_t id; char pad[12]; };
struct PtRawMaterial { float albedo[4], emissive[4]; float roughness; int32_t type; char pad[24]; };
static_assert(sizeof(PtRawTriangle) == 64 && sizeof(PtRawMaterial) == 64, "record layout");

// Triangle as the trace kernel consumes it: one 64-byte, 64-byte-aligned record =
// one s_load_dwordx16 per wave.  e1 = p2-p1, e2 = p3-p1, n = cross(e2,e1) are the values
// intersectTriangle recomputes on every call (GenerateColors.cl:92-93,123); computing them
// once per upload yields the same bits.
struct PtPrepTriangle {
    float p1[3];
    float e1[3];
    float e2[3];
    float pad0[3];
    float n[3];
    int32_t id;
};
static_assert(sizeof(PtPrepTriangle) == 64, "prep layout");

// LBVH internal node (pt_bvh.hip): the boxes of BOTH children and their links; a link is the child's
// node index, or 0x80000000 | triangle index for a leaf.  64 bytes = four 16-byte loads.
struct PtBvhNode {
    float lmin[3]; uint32_t link_l;
    float lmax[3]; uint32_t link_r;
    float rmin[3]; uint32_t pad0;
    float rmax[3]; uint32_t pad1;
};
static_assert(sizeof(PtBvhNode) == 64, "bvh node layout");

// The node the trace kernel walks: EIGHT children in 64 bytes -- one 64-byte sector of a cache line, four 16-byte loads
// (after Ylitie, Karras, Laine, "Efficient incoherent ray traversal on GPUs through compressed wide BVHs", 2017).  Round 3
// measured what the search is bound by (profiles/r03/lbvh_bottlenecks.txt): every 16-byte load of a wave whose 64 lanes
// read 64 different lines costs the CU's texture-address path 64 cycles -- one MORE such load per node visit cost 8.7 % --
// and the L2's miss path moves sectors, not requests (tools/ubench_gather: 64-byte records 111 G/s, 128-byte records 86 G/s).
// Round 2's node was 80 bytes in a 128-byte slot (five loads, both sectors); this one is 64 (four loads, one sector, two
// nodes per line: siblings lie next to each other and a ray that enters one often enters the other):
//   * which binary nodes of the radix tree become nodes here, and which of their descendants their (at most eight)
//     children are, is chosen by dynamic programming over surface-area costs (pt_bvh.hip);
//   * nodes and leaf records are 64-byte RECORDS of ONE array; the children of a node -- nodes and leaves alike -- are
//     stored consecutively in slot order from `base`: the child in slot s is record base + popcount((imask | lmask) &
//     ((1 << s) - 1)): no links, one base;
//   * a child sits in the slot whose three bits say on which side of the node's centre it lies (x = bit 0, y = bit 1,
//     z = bit 2; greedy assignment), so "slot XOR (ray direction's octant)" orders the children front to back for
//     every ray without a sort;
//   * boxes: 8 bits per coordinate in the node's own frame (origin = lower corner of the children's union, one
//     power-of-two step per axis), rounded OUTWARD and verified at build time by decoding (fma(q, step, origin) contains
//     the fp32 box); stored per axis (qlo[axis][slot], qhi[axis][slot]) so the ray's direction signs pick the near and
//     far planes of all eight children with four selects per axis; an empty slot holds an inverted box (255, 0) AND is
//     missing from both masks;
//   * the origin itself is 16 bits per axis on a grid over the scene (PtBvhGrid: origin = fma(org, grid step, grid min),
//     rounded DOWN and checked by decoding with the very expression the traversal uses; the boxes are quantised against
//     the decoded origin, so nothing is lost but up to one grid step -- 1 / 65 535 of the scene -- of the 8-bit range).
struct alignas(64) PtBvh8Node {
    uint16_t org[3];      // origin on the scene grid
    uint8_t ex[3];        // step exponents (biased as in binary32)
    uint8_t imask;        // slots that hold nodes
    uint8_t lmask;        // slots that hold leaves
    uint8_t pad;
    uint32_t base;        // record index of the first child
    uint8_t qlo[3][8];    // [axis][slot]
    uint8_t qhi[3][8];
};
static_assert(sizeof(PtBvh8Node) == 64, "bvh node layout");
struct PtBvhGrid { float gmin[3], gstep[3]; };  // the origins' grid (steps are powers of two: org * gstep is exact)

// A LEAF of the hierarchy is ONE triangle: a 64-byte record of the same array, three 16-byte loads.  (Leaves of four
// consecutive triangles of the Morton order were measured in round 2: the 10^6-triangle soup's leaf boxes grow 9x in
// cross-section, 184 instead of 5.4 triangle tests per ray, 35 instead of 86 Msamples/s.)
struct alignas(64) PtLeafTri {
    float p1[3], e1[3], e2[3];  // as in PtPrepTriangle
    uint32_t index;             // the triangle's index in the caller's buffer (ties in t go to the lowest)
    float pad[6];
};
static_assert(sizeof(PtLeafTri) == 64, "leaf record layout");

#define PT_TRACE_BATCH 256u    // largest number of samples per work-queue grab of a wave (PtTraceParams::batch)
#define PT_TRACE_THREADS 256   // 4 waves per workgroup (variant 1)
#define PT_LDS_TRI_STRIDE 12    // dwords per triangle record in the LDS copy (p1, e1, e2, 3 pad)
#define PT_LDS_TRI_MAX 256      // scenes up to this many triangles keep the copy (12 KiB per workgroup)

// the render's camera, derived on the host once per render (pt_camera_derive, include/pt_shim.h; GenerateColors.cl:263-276):
// eye, the orthonormal-to-rounding basis {viewDir, holDir, upDir} and angle = tan(fov / 2).  The eye is also the ANCHOR of the
// pass-1 filters (pt_quad3_pass1: K = cross(e2, a - eye), the tame check |o - eye|_inf <= ray_radius)
struct PtCamera {
    float eye[3], view[3], hol[3], up[3];
    float angle;
};
// ... and its thin lens (include/pt_shim.h: pt_camera), carried by the launches that start their samples through pt_item_begin,
// pt_list_item_begin or pt_camera_rays_kernel -- ambient occlusion, the lit renders, the camera-ray query.  lens_radius = 0 is the
// pinhole: the code of before, no extra draw.  The fused trace kernels have no lens: PtTraceParams keeps the plain PtCamera, so
// their kernel arguments do not move (their masks and pass-1 tables are built on org == eye bit for bit)
struct PtLensCamera : PtCamera {
    float lens_radius, focus_distance;
};

struct PtTraceParams {
    const PtPrepTriangle* tris;
    const PtRawMaterial* mats;
    float* rad;                   // the staging RING's two slots, [frames per slot][npix_local][3] path radiance max(L,0) each, 12 bytes per
    float* rad1;                  // sample.  A path's `fl` is its frame counted from the render's first (frame_begin - chunk_f0 is that frame's
                                  // absolute number); chunk c of the render is frames [c S, (c + 1) S) and goes to slot (c + ring_phase / S) % 2,
                                  // so a path CARRIED into the next launch (below) still stores to its own chunk's slot
    unsigned int* batch_counter;  // the work queue (PT_QUEUE_WORDS words: sharded counters + stop word); zero at the launch (the fold kernel that follows the trace launch on its stream resets it: PtFoldParams::reset_counter)
    unsigned long long* stats;    // may be null: [0] samples, [1] rays
    int32_t width, height;
    float inv_width, inv_height, aspect;  // 1.0f / W, 1.0f / H, (float)W / (float)H (IEEE, host-computed: GenerateColors.cl:266-267)
    int32_t frame_begin;          // first frame of this chunk (global frame index)
    int32_t frame_count;          // frames in this chunk
    uint32_t chunk_f0;            // ... and that first frame counted from the render's first (a multiple of the frames per ring slot)
    uint32_t slot_frames;         // S: frames per ring slot = frames per chunk (the render's last chunk may be shorter)
    uint32_t ring_phase;          // 0 or S: which slot the render's first chunk uses
    uint32_t ring_magic;          // floor(2^32 / 2S) + 1: (fl + ring_phase) % 2S by one v_mul_hi_u32 (exact below 65 536)
    uint32_t rad1_off;            // SHORT form of a sample's radiance address (pt_ring_offset; chosen per render, pt_shim.hip: trace_params): rad1's
                                  // byte offset from rad -- the two slots are one allocation -- when the whole ring is at most 4 GiB: a path then
                                  // carries its record's byte offset from rad (unsigned 32 bits), worked out once where the sample starts, and the
                                  // store is one global_store_dwordx3 against the scalar base.  0 = the LONG form: the ring is larger, a path carries
                                  // its local pixel and the store forms the 64-bit address from fl
    int32_t max_bounces, ntri, nmat;
    int32_t stripe_rows, n_ranks, rank;
    uint32_t npix_local;
    uint32_t batches_per_frame, total_batches;
    uint32_t batch;               // samples per work-queue grab: 64, 128 or 256 (<= PT_TRACE_BATCH)
    float quad_delta1;            // quad mode 2 (pt_quad2_pass1): slack of the shared-u bounds
    float ray_radius;             // quad modes 2, 3: rays with |origin - eye|_inf above this keep every triangle
    const float* p1tab;           // quad mode 3: packed pass-1 table, PT_P1_STRIDE floats per pair of quads
    float p1_lo, p1_hi;           // quad mode 3: bounds of the shared numerator for the first / second triangle
    const PtBvh8Node* bvh;        // accel = BVH: the hierarchy's 64-byte records (nodes and leaves), root = record 0, every node's
                                  //              children consecutive
    int32_t bvh_records;          //              capacity of that array (2 x triangles): indices are checked against it
    PtBvhGrid grid;               //              the grid of the nodes' 16-bit origins
    const PtPrepTriangle* bigtab; // accel = BVH: prepared records of the nbig triangles kept out of the hierarchy (brute-force searched)
    const int32_t* bigidx;        //              their triangle indices, ascending
    int32_t nbig;
    const uint2* pmask;           // quad mode 3, <= 64 triangles: per local pixel the primary rays' candidate masks of the two
                                  // 32-triangle chunks (pt_primary_mask_kernel); null = run pass 1 for primary rays too
    unsigned int* bvh_flags;      // accel = BVH: the sticky word a search that was cut short raises (PT_BVH_FLAG_* bits): host memory mapped into
                                  //              the device's address space, written with plain system-scope stores, read and cleared by the host
    int32_t bvh_stack_limit;      //              stack entries a lane may use, <= PT_BVH_STACK (lower only to test the overflow report)
    // CHECKPOINTED launches (table trace kernels): a launch with carry_out set ends the moment its work queue has
    // handed out the last batch -- every wave, at its next fresh-phase boundary, stores what it still holds (its live paths,
    // the unstarted rest of its batch) to its region of `carry` and exits -- and the next launch of the render (carry_in_waves = the grid of this one, in
    // waves) resumes them beside its own work: no launch but a render's last (carry_out = 0: total_batches may be 0) has a tail
    // of waves running out of paths.  Which launch finishes a path never affects its result.
    uint32_t* carry;              // per wave of the grid PT_CARRY_HIT_STRIDE_DW dwords (table kernels) or PT_CARRY_STRIDE_DW (LBVH kernel)
    uint32_t carry_in_waves;
    uint32_t carry_out;
    PtCamera cam;                 // read from the kernarg segment where rays are generated and where pass 1 checks a ray (every kernel)
    const uint2* smask;           // quad mode 3, <= 64 triangles: the scene's table of secondary-ray candidate masks (pt_secmask.h: the
                                  // classification records, then one uint2 per cell); null = pass 1 for secondary rays.  Read from the
                                  // kernarg segment by the table trace kernels only
};
// a work queue: PT_QUEUE_SHARDS counters and, behind them, the stop word of checkpointed launches (one bit per shard found empty), each on
// a line of its own, PT_QUEUE_SHARD_WORDS apart (4 KiB + 128 B: whatever the address-to-channel map is, neighbours differ in both fields)
#define PT_QUEUE_SHARDS 8
#define PT_QUEUE_SHARD_WORDS 1056
#define PT_QUEUE_STOP_WORD (PT_QUEUE_SHARDS * PT_QUEUE_SHARD_WORDS)
#define PT_QUEUE_WORDS ((PT_QUEUE_SHARDS + 1) * PT_QUEUE_SHARD_WORDS)
#define PT_POOL 56                // parked-path slots per wave of a table kernel (why 56: above PtWaveQueue, pt_kernels.hip)
#define PT_CARRY_RECORDS 64       // the LBVH kernel has no pool: a wave stops with its (at most 64) live lanes
#define PT_CARRY_STRIDE_DW (16 + PT_CARRY_RECORDS * 15)   // header (paths, pix, end, ring frame, absolute frame) + the parked-path record as arrays (the LBVH kernel's)
// the table kernels park SEARCHED paths (pt_trace_body): 18 dwords a record -- hit point, direction, mask, L, seed, ro, hu, hv, fl | bounce, triangle.
// A wave of theirs stops by parking its live paths into its EMPTY pool, as a fresh phase does, and stores the pool: at most PT_POOL records, never 64
#define PT_CARRY_HIT_RECORDS PT_POOL
#define PT_CARRY_HIT_STRIDE_DW (16 + PT_CARRY_HIT_RECORDS * 18)
// one allocation serves a render whichever kernel it runs (pt_shim.hip: PT_CARRY_HIT_STRIDE_DW dwords per wave); 1 024 dwords, 4 KiB, a region
static_assert(PT_CARRY_HIT_STRIDE_DW >= PT_CARRY_STRIDE_DW, "a checkpoint region holds either kernel's records");
static_assert(PT_CARRY_HIT_STRIDE_DW % 4 == 0 && PT_CARRY_STRIDE_DW % 4 == 0, "a region's float4 arrays begin 16 dwords in: every region 16-byte aligned");
// The kernel with the table in LDS packs fl | bounce << 16 | triangle << 24 into one dword (17 a record: what lets its pools fit 8 workgroups
// a CU): a parked path's bounce count, below max_bounces, must fit 8 bits, and so must its triangle (PT_LDS_TRI_MAX).  The host refuses a deeper render on that kernel (pt_shim.hip: render_part).
#define PT_PACKED_BOUNCE_MAX 256

struct PtFoldParams {
    const float* rad;   // [frame_count][npix_local][3]
    float4* fb;         // [npix_local] gamma-encoded running mean (GenerateColors.cl:314-321)
    uint32_t npix_local;
    int32_t frame_begin, frame_count;
    unsigned int* reset_counter;  // the work-queue counter of the trace launch whose chunk this is: set back to zero for its next user
    unsigned int* reset_counter2; // (may be null) a second one: the counter of the render's last, draining launch
};

// det_bound_bits: FOUR device words: [0] bit pattern of max_i (|e1|_1 * |e2|_1), [1] number of odd
// triangles whose e2 is not the exact negation of their predecessor's (0 = the scene is all quads),
// [2] non-zero when some vertex coordinate is not finite, [3] number of odd triangles whose p1 is not their
// predecessor's p3 (0 = every pair is (a,b,c),(c,d,a))
// [4], [5] (one 64-bit word): checksum of the raw records
// [6..8] per axis the COMPLEMENT of the order key (ptk_order_key) of the smallest vertex coordinate, [9..11] the order key of
// the largest (both reduced with atomicMax over zeroed words), once per scene upload: the host derives
// the scene's radius about ANY eye from them without another device read (fl(v - e) is monotone in v)
#define PT_PREP_WORDS 12
__host__ __device__ static inline unsigned ptk_order_key(float f)   // finite floats -> unsigned integers in the same order (-0 and +0 apart, harmlessly)
{
    unsigned u;
    __builtin_memcpy(&u, &f, sizeof u);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ static inline float ptk_order_float(unsigned k)
{
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    __builtin_memcpy(&f, &u, sizeof f);
    return f;
}
hipError_t ptk_prep_triangles(const PtRawTriangle* raw, PtPrepTriangle* out, int ntri, unsigned int* det_bound_bits,
                              hipStream_t s);
// quad mode 2: writes every odd record's pad0[0] = slack of its shared-u bound (needs the scene
// diameter bound D from word [2] of the first pass, hence a second tiny launch)
// p1tab (may be null): quad mode 3's table, PT_P1_STRIDE floats per pair of quads (pt_quad3_pass1)
// anchor: the render's eye (PtCamera), the point K = cross(e2, a - anchor) of the packed table is taken about.  Camera
// changes rerun this (pt_shim.hip: ensure_anchor); the pairing checks of the first pass are not redone
hipError_t ptk_prep_quad_margins(PtPrepTriangle* out, int ntri, float diameter, float delta1, float* p1tab, const float anchor[3], hipStream_t s);
#define PT_P1_STRIDE 24  // floats per quad pair: nx ny nz e2x e2y e2z Kx Ky Kz dhi, each {quad 2p, quad 2p+1}, 4 pad
static inline size_t ptk_p1tab_floats(int ntri) { return (size_t)((ntri / 2 + 1) / 2) * PT_P1_STRIDE; }
// fills p.pmask (when not null) for the image geometry and the camera of p from the prepared records p.tris: per pixel the triangles
// whose whole exact test (:96-125) some primary ray of the pixel can pass
hipError_t ptk_primary_masks(const PtTraceParams& p, hipStream_t s);
// fills table (PT_SM_TABLE_BYTES(ntri) bytes, pt_secmask.h) from the prepared records: per cell of (origin triangle, tile of its plane,
// direction cell) the triangles whose whole exact test some ray of the cell can pass.  ntri <= PT_SM_TRI_MAX
hipError_t ptk_secondary_masks(const PtPrepTriangle* tris, int ntri, uint2* table, hipStream_t s);
// which search a launch runs (pt_shim.hip: prepare_search decides it, once, for renders, queries and ambient occlusion alike)
struct PtSearchMode {
    // traverse p.bvh instead of the brute-force two-pass search; then `quads` is about the table of the big triangles kept out
    // of the hierarchy (p.bigtab: 3 = made of quads, p.p1tab / p1_lo / p1_hi / quad_delta1 / ray_radius prepared for IT)
    bool bvh;
    // every triangle satisfies |e1|_1*|e2|_1 <= PT_DET_BOUND_MAX (short exact reciprocal valid)
    bool det_bounded;
    // 0 = independent triangles (pt_tri_pass1); 3 = ntri is even, every pair (2k, 2k+1) is a quad (a,b,c),(c,d,a), the margins
    // and the packed table p.p1tab are prepared (pt_quad3_pass1)
    int quads;
};
// tally: (bvh only) the measurement variant that adds the search's work counters to p.stats[2..5]
// wide: (bvh only) the slabs carry the ray term of the margin, PT_BVH_RAY_EPS x the origin's largest |coordinate|.  Every path starts at
//       the eye and goes on from points of the scene, so the host leaves the term out (the kernels of before, instruction for instruction)
//       when the eye's largest |coordinate| is at most PT_BVH_NEAR_EYE x the scene's: there the term is below a third of eps and the
//       measured excess below 0.01 eps (pt_bvh.hip's table, D / m <= 10).  Queries and AO take rays from anywhere and always carry it.
hipError_t ptk_trace(const PtTraceParams& p, int num_blocks, PtSearchMode m, bool tally, bool wide, hipStream_t s);
#define PT_BVH_NEAR_EYE 4.0f
// out[k] = raw[bigidx[k]], k < nbig <= PT_BVH_BIG_MAX
hipError_t ptk_bvh_big_raw(const PtRawTriangle* raw, const int* bigidx, int nbig, PtRawTriangle* out, hipStream_t s);
static inline size_t ptk_bvh_record_count(int ntri) { return 2 * (size_t)(ntri > 0 ? ntri : 0); }  // < ntri nodes + ntri leaves
size_t ptk_bvh_temp_bytes(int ntri);
// prep: the prepared records of the same triangles.  bigtab[PT_BVH_BIG_MAX] / bigidx[PT_BVH_BIG_MAX] / *nbig_dev (device memory)
// receive the triangles kept OUT of the hierarchy (pt_bvh.hip: PT_BVH_BIG_DIV): their prepared records and indices, ascending
#define PT_BVH_BIG_MAX 64
// The boxes' margin has a part that follows the RAY: a binary32 hit is displaced by an amount that grows with the distance the
// ray has travelled, about one to two ulp of its origin's coordinates and more at grazing incidence, which the scene-sized margin
// PT_BVH_EPS cannot cover for an origin far outside the scene.  The traversal widens every slab by PT_BVH_RAY_EPS x (the origin's
// largest |coordinate|); the derivation and the measurements are in pt_bvh.hip's header.
#define PT_BVH_RAY_EPS 1.2e-4f
// recs[ptk_bvh_record_count(ntri)] (device memory) receives the hierarchy the trace kernel walks, *grid_dev its origin grid
// *used_dev (device memory, may be null) receives the number of records in use
hipError_t ptk_bvh_build(const PtRawTriangle* raw, const PtPrepTriangle* prep, int ntri, PtBvh8Node* recs,
                         PtPrepTriangle* bigtab, int* bigidx, int* nbig_dev, PtBvhGrid* grid_dev, unsigned* used_dev, void* temp, size_t temp_bytes,
                         hipStream_t s);
#define PT_DET_BOUND_MAX 2.0e19f
#define PT_BVH_AUTO_MIN 512      // PT_OPT_ACCEL = 0 uses the BVH from this many triangles on
hipError_t ptk_fold(const PtFoldParams& p, hipStream_t s);
hipError_t ptk_assemble_stripes(const float4* gathered, float4* image, int width, int height, int stripe_rows,
                                int n_ranks, int slab_rows, hipStream_t s);
hipError_t ptk_tonemap_ppm(const float4* fb, int32_t* rgb, size_t npix, hipStream_t s);
hipError_t ptk_fill_i32(int32_t* dst, int32_t value, int n, hipStream_t s);
hipError_t ptk_math(const float* in, float* out, int n, hipStream_t s);
// the fold kernel's short forms against the literal operations (pt_fold_check_kernel); out: 6 counters
hipError_t ptk_fold_check(unsigned long long* out, int mode, unsigned first, unsigned long long count, hipStream_t s);
// pt_shade's short forms -- the guarded quotients, 1 / sqrt -- against the literal operations (pt_shade_check_kernel); out: 8 counters
hipError_t ptk_shade_check(unsigned long long* out, int mode, unsigned first, unsigned long long count, hipStream_t s);
// the masked search's pending-pair list on given masks (pt_pair_check_kernel): masks: cases x 64 lanes x {low, high word};
// out: cases x (2 + cap) words -- pairs, rounds, then the pairs (triangle << 6 | ray lane) in the order the rounds test them
hipError_t ptk_pair_check(const uint2* masks, unsigned* out, int ntri, unsigned cases, unsigned cap, hipStream_t s);
// the masked search itself on given rays and masks (pt_search_check_kernel): tris: the prepared scene, 1 <= ntri <= 64, det-bounded;
// rays: cases x 64 lanes x {origin xyz, alive word | direction xyz, unused}; masks: cases x 64 x {low, high word};
// out: cases x 64 x {hidx, t, hu, hv (bits) | steps, 0, 0, 0}
hipError_t ptk_search_check(const PtPrepTriangle* tris, int ntri, const float4* rays, const uint2* masks, uint4* out, unsigned cases, hipStream_t s);
// batched ray queries (pt_intersect_rays): t carries the search -- the prepared scene (tris, ntri), the filter of the table the
// two-pass search runs over (quad_delta1 .. p1_hi, its anchor in cam.eye), the LBVH (bvh .. nbig, bvh_flags, bvh_stack_limit);
// the other fields of t are not read
struct PtQueryParams {
    PtTraceParams t;
    const float4* rays;   // [nrays] pt_ray: origin xyz tmax | dir xyz reserved (two float4)
    void* out;            // [nrays] pt_hit (three float4), or int32 when occluded
    uint32_t nrays;
    int32_t occluded;
};
// bvh_blocks: the persistent grid of the LBVH kernel (CUs x ptk_query_bvh_blocks_per_cu: the driver's kernels -- closest, any-hit, AO -- are all
// pinned to five waves per SIMD and use the trace kernel's LDS, so one figure, the closest kernel's, sizes every such grid)
// any: (bvh and q.occluded only) pt_occluded_rays: an any-hit search, which stops at the first accepted triangle
hipError_t ptk_query(const PtQueryParams& q, int bvh_blocks, PtSearchMode m, bool any, hipStream_t s);
int ptk_query_bvh_blocks_per_cu(void);
// ambient occlusion (pt_render_ao): t carries the search as PtQueryParams::t does (the filter's anchor in t.cam.eye) and the image
// geometry (width, inv_width, inv_height, aspect, stripe_rows, n_ranks, rank); cam is the camera
struct PtAoParams {
    PtTraceParams t;
    PtLensCamera cam;
    unsigned long long* counts;   // [npix] open | hits << 32 (the {open, hits} uint32 pair), added to
    uint32_t npix;                // local pixels
    uint32_t nitems;              // samples of this launch, frame-major: item = f * npix + local pixel (< 2^31)
    int32_t frame0;               // the frame of item 0
    int32_t K;                    // occlusion rays per hit
    float tlim;                   // min(radius, 1e20)
};
// (pt_kernels.hip reads the lens from the kernarg segment at this one place, whichever block the kernel takes: pt_lens_kargs)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"   // (PtLensCamera has a base: offsetof is conditionally supported, and clang supports it)
static_assert(offsetof(PtAoParams, cam) == sizeof(PtTraceParams), "PtAoParams begins { t, cam }");
#pragma clang diagnostic pop
hipError_t ptk_ao(const PtAoParams& a, int bvh_blocks, PtSearchMode m, hipStream_t s);
// image[i] = float4(a, a, a, 1) of counts[i] = {open, hits}: a = open / (K hits), miss_value when hits = 0
hipError_t ptk_ao_resolve(const uint2* counts, float4* image, uint32_t npix, uint32_t K, float miss_value, hipStream_t s);
// direct illumination (pt_render_direct): t carries the search and the image geometry as PtAoParams::t does, and the materials
// (mats, nmat >= 1); cam is the camera.  One launch writes the radiance of nitems samples, frame-major from frame0 on, 12 bytes each,
// which ptk_fold folds into the framebuffer (PtFoldParams::rad = samples, frame_begin = frame0)
struct PtDirectParams {
    PtTraceParams t;
    PtLensCamera cam;
    const int32_t* lights;        // [nl] triangle indices, clamped into [0, ntri) where they are used; not read when nl = 0
    float* samples;               // [nitems][3] max(E + S / K, 0)
    uint32_t npix;                // local pixels
    uint32_t nitems;              // samples of this launch: item = f * npix + local pixel (< 2^31)
    int32_t frame0;               // the frame of item 0
    int32_t K;                    // light samples per hit
    int32_t nl;                   // lights in the list, 0 .. 2^24 - 1 ((float)nl is exact)
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(offsetof(PtDirectParams, cam) == sizeof(PtTraceParams), "PtDirectParams begins { t, cam }");
#pragma clang diagnostic pop
// first-hit feature buffers (pt_render_features): direct illumination's sample up to its surface.  Of d the launch reads t (the search,
// the image geometry, mats and nmat >= 1), cam, npix, nitems and frame0; lights, samples, K and nl are not read.  Item i = f * npix +
// local pixel writes 12 bytes to X[i] of every output X that is not null: the first hit's albedo, facing normal, (t, 1, -dot(n, d)) and
// emission; a miss writes zeros
struct PtFeatureParams {
    PtDirectParams d;
    float* albedo;                // [nitems][3] each; null = the launch does not write it
    float* normal;
    float* depth;
    float* emission;
};
// bvh_blocks: ptk_query's (the LBVH form is a kernel of the driver at five waves per SIMD, as the closest query and ambient occlusion)
hipError_t ptk_render_features(const PtFeatureParams& f, int bvh_blocks, PtSearchMode m, hipStream_t s);
// indirect illumination (pt_render_indirect): direct illumination's launch with the path's depth.  samples[item] = max(L, 0) of the
// whole path; everything else is as PtDirectParams says (the helpers of both take its PtDirectParams)
struct PtIndirectParams {
    PtDirectParams d;
    int32_t B;                    // max_bounces, 1 .. 65535
};
// THE PARAMETER BLOCKS OF THE LIT KERNELS.  A kind's bits (PtLitKind, below) select the block its instantiations take; a kernel whose
// kind lacks a bit takes the block it took before that bit existed, at the same kernarg offsets.  The last row that applies wins:
//   kind bit            direct block          indirect block          what the block adds
//   (none)              PtDirectParams        PtIndirectParams        B
//   mis                 --                    PtIndirectMisParams     counts: the list entries per triangle (pt_render_indirect_mis)
//   power               PtDirectPowerParams   PtIndirectPowerParams   cdf, tri_q: pt_light_table's selection table (the _power entry points)
//   rr                  --                    PtIndirectRrParams      R, cap: the roulette, whichever estimator (counts, cdf, tri_q null where not read)
//   list                --                    PtIndirectListParams    slots, frame_off: a LIST of pixels (pt_render_indirect_pixels)
//   ris                 PtDirectRisParams     PtIndirectRisParams     M: the candidates of a resampled light sample (the _ris entry points)
//   env                 PtDirectEnvParams     PtIndirectEnvParams     env: the octahedral map and its table (the _env entry points)
//   rays (bit 7)        --                    PtIndirectRaysParams    rays, first_ray: the caller's rays (pt_radiance_rays)
// Every added field is wave-uniform: none adds per-lane state
struct PtIndirectMisParams : PtIndirectParams {
    const int32_t* counts;        // [ntri] list entries per triangle (ptk_light_counts); not read when nl = 0
};
// counts[t] = the entries of lights[0 .. nl) whose index, clamped into [0, ntri), is t: one clear, one kernel of vector atomics
hipError_t ptk_light_counts(const int32_t* lights, int nl, int ntri, int32_t* counts, hipStream_t s);
// cdf: uint64[nl + 1], tri_q: uint32[ntri], as pt_light_table writes them; neither is read when nl = 0
struct PtDirectPowerParams : PtDirectParams {
    const uint64_t* cdf;
    const uint32_t* tri_q;
};
struct PtIndirectPowerParams : PtIndirectMisParams {
    const uint64_t* cdf;
    const uint32_t* tri_q;
};
struct PtIndirectRrParams : PtIndirectPowerParams {
    int32_t R;                    // first_bounce >= 1: the roulette is played at vertex i when i + 1 >= R and i < B - 1
    float cap;                    // max_survival in (0, 1]
};
// A list launch: d.npix is the number of listed pixels, item = f * d.npix + j is frame f of slot j, whose local pixel is
// min(slots[j].x, d.t.npix_local - 1) and whose frame number is (slots[j].y + frame_off + f) & 0x7fffffff; d.frame0 is not read.  The
// sample is stored at samples[item] as before
struct PtIndirectListParams : PtIndirectRrParams {
    const uint2* slots;           // [d.npix] pt_pixel_slot {pixel, frame}
    uint32_t frame_off;           // the frames every listed pixel has received from this call already
};
struct PtDirectRisParams : PtDirectPowerParams {
    int32_t M;                    // candidates per light sample, 1 .. 32
};
struct PtIndirectRisParams : PtIndirectListParams {   // (the roulette form does not read slots and frame_off)
    int32_t M;
};
struct PtEnvMap {
    const float4* texels;         // [N * N] row-major, w ignored
    const uint64_t* cdf;          // [N * N + 1] as ptk_env_table writes it; not read when Ke = 0
    int32_t N;                    // a power of two, 1 .. 2048
    int32_t Ke;                   // environment samples per vertex, 0 .. 256
};
struct PtDirectEnvParams : PtDirectPowerParams {
    PtEnvMap env;
};
struct PtIndirectEnvParams : PtIndirectRrParams {
    PtEnvMap env;
};
// A rays launch: d.npix is the number of rays n, item = s * n + r is sample d.frame0 + s of ray r, whose seed is (first_ray + r) +
// pt_hash_u32(d.frame0 + s) and whose primary ray is getRay of rays[2 r], rays[2 r + 1] (pt_query_load: tmax and reserved are not
// read); d.cam and the image geometry of d.t are not read.  The sample is stored at samples[item] as before
struct PtIndirectRaysParams : PtIndirectRrParams {
    const float4* rays;           // [d.npix] pt_ray: origin xyz tmax | dir xyz reserved (two float4)
    uint32_t first_ray;           // the id of rays[0]
};
// what ptk_lit is handed: the largest block of the kinds without env, the map, and the rays
struct PtLitParams : PtIndirectRisParams {
    PtEnvMap env;
    const float4* rays;
    uint32_t first_ray;
};
// A kind of lit render names its kernels.  The 14 valid values without ris:
//   direct illumination (pt_direct_kernel, pt_direct_bvh_kernel):          indirect = mis = rr = list = 0;  power 0 / 1
//   indirect illumination (pt_indirect_kernel, pt_indirect_bvh_kernel):    indirect = 1, rr = list = 0;     mis 0 / 1 x power 0 / 1
//   ... with Russian roulette (pt_indirect_rr_kernel, ..._bvh_kernel):     indirect = rr = 1, list = 0;     mis x power
//   ... over a list of pixels (their list forms):                          indirect = rr = list = 1;        mis x power
// list implies rr, rr implies indirect, mis comes only with indirect
// and the 5 with ris: direct by power; the roulette and the list kinds by power, mis 0 / 1.  ris implies power, and an indirect ris kind
// has rr (R >= B plays no roulette); and the 2 with env: direct by power; the roulette kind by power with mis.  env implies power,
// excludes ris and list, and an indirect env kind has mis and rr
struct PtLitKind { bool indirect, mis, power, rr, list, ris, env; };
constexpr bool ptk_lit_kind_valid(PtLitKind k)
{
    return (!k.list || k.rr) && (!k.rr || k.indirect) && (!k.mis || k.indirect) && (!k.ris || (k.power && k.rr == k.indirect)) &&
           (!k.env || (k.power && !k.ris && !k.list && k.rr == k.indirect && k.mis == k.indirect));
}
// a table's index, and back (the bits above PT_LIT_KIND_INDICES are not read)
constexpr int ptk_lit_kind_index(PtLitKind k) { return k.indirect | k.mis << 1 | k.power << 2 | k.rr << 3 | k.list << 4 | k.ris << 5 | k.env << 6; }
#define PT_LIT_KIND_INDICES 128
constexpr PtLitKind ptk_lit_kind_of(unsigned i) { return { (i & 1) != 0, (i & 2) != 0, (i & 4) != 0, (i & 8) != 0, (i & 16) != 0, (i & 32) != 0, (i & 64) != 0 }; }
// Radiance queries (pt_radiance_rays) are a second START of a kind's items, beside the kind: a kind names the estimator and the item map
// of an image render and stays as it stands above; with `rays` its items are samples of the caller's rays.  The 4 kinds that take rays
// are the roulette kinds, mis 0 / 1 x power 0 / 1 -- the shape of the list kinds: rays need rr and exclude list, ris and env
constexpr bool ptk_lit_rays_valid(PtLitKind k) { return ptk_lit_kind_valid(k) && k.rr && !k.list && !k.ris && !k.env; }
// THE kind below the C ABI, one number: the kind's index, and bit 7 (PT_LIT_KIND_INDICES) for the forms that render the caller's rays --
// the kernels' one kind parameter (pt_kernels.hip: PtKindOf) and the index of a table over kinds, whose second half is the rays forms'.
// The two predicates above say which of the PT_LIT_KINDS values exist; nothing else lists them
#define PT_LIT_KINDS (2 * PT_LIT_KIND_INDICES)
constexpr unsigned ptk_lit_kind(PtLitKind k, bool rays) { return (unsigned)ptk_lit_kind_index(k) | (rays ? PT_LIT_KIND_INDICES : 0); }
constexpr bool ptk_lit_valid(unsigned kind)
{
    const PtLitKind k = ptk_lit_kind_of(kind);
    return kind < PT_LIT_KINDS && (kind & PT_LIT_KIND_INDICES ? ptk_lit_rays_valid(k) : ptk_lit_kind_valid(k));
}
// THE launch of a lit render, whatever its kind (ptk_lit_valid): `a` is the largest block, and each instantiation is passed its own,
// sliced from it (PtDirectPowerParams is made of a.d, a.cdf and a.tri_q).  LBVH (m.bvh): the kind's kernel on a persistent grid of at
// most bvh_blocks = CUs x ptk_lit_bvh_blocks_per_cu(kind) workgroups -- the occupancy of the kind's OWN <true, 3> instantiation with the
// trace kernel's LDS: the direct kernels run at four waves per SIMD, the indirect ones at three, so ptk_query_bvh_blocks_per_cu's
// premise (five) holds for none.  Brute force: one wave per 64 items; the roulette and list kinds one wave per PT_RR_RUN
// (pt_constants.h) consecutive items, which refills its dead lanes from its run.  A rays kind reads neither a.d.cam nor the image geometry
hipError_t ptk_lit(const PtLitParams& a, unsigned kind, int bvh_blocks, PtSearchMode m, hipStream_t s);
int ptk_lit_bvh_blocks_per_cu(unsigned kind);
// the fold of a list launch: one lane per (slot j, channel) folds rad[f][j], f = 0 .. frame_count - 1 ascending, into fb[the slot's
// pixel] with the slot's own frame numbers (pt_fold_frame); pixels that are not listed are neither read nor written
struct PtFoldListParams {
    const float* rad;             // [frame_count][num_listed][3]
    float4* fb;                   // [npix_local]
    const uint2* slots;           // [num_listed]
    uint32_t num_listed, npix_local;
    uint32_t frame_off;
    int32_t frame_count;
};
hipError_t ptk_fold_list(const PtFoldListParams& p, hipStream_t s);
// moments[the pixel of slot j] takes samples[f][j][0..2], f = 0 .. frames - 1 ascending; one lane per slot; never resets
struct PtPixelMoments;
hipError_t ptk_sample_moments_list(const float* samples, PtPixelMoments* moments, const uint2* slots, uint32_t num_listed, uint32_t npix,
                                   int32_t frames, hipStream_t s);
// pt_adaptive_select: list = {uint32 count, 0, 0, 0}, then the slots of the active pixels in ascending order, then the build's
// scratch: one uint64 per tile of PT_LIGHT_SCAN_TILE pixels.  Three kernels: per-tile counts, their scan, the scatter
struct PtAdaptiveRule {
    double tol2, floor2;
    uint32_t min_samples, max_samples;
};
#define PT_ADAPTIVE_LIST_BYTES(n) ((size_t)16 + (size_t)(n) * 8 + PT_LIGHT_TABLE_TILES(n) * 8)
hipError_t ptk_adaptive_select(const PtPixelMoments* moments, uint32_t npix, const PtAdaptiveRule& rule, void* list, hipStream_t s);
// pt_light_table: the selection table of lights[0 .. nl) over the RAW records (the prepared ones hold the same e1, e2 and N bit for
// bit: pt_prep_kernel).  cdf: PT_LIGHT_TABLE_WORDS(nl) uint64 -- cdf[0 .. nl], then the build's scratch: the largest power's bits and
// one sum per tile of PT_LIGHT_SCAN_TILE entries; tri_q: uint32[ntri].  One clear, then four kernels (weights and their maximum;
// quantise and tile sums; the scan of the tile sums; the scan of the tiles); nl = 0 or ntri = 0 only clears
#define PT_LIGHT_SCAN_BLOCK 256
#define PT_LIGHT_SCAN_ITEMS 8
#define PT_LIGHT_SCAN_TILE (PT_LIGHT_SCAN_BLOCK * PT_LIGHT_SCAN_ITEMS)
#define PT_LIGHT_TABLE_TILES(nl) (((size_t)(nl) + PT_LIGHT_SCAN_TILE - 1) / PT_LIGHT_SCAN_TILE)
#define PT_LIGHT_TABLE_WORDS(nl) ((size_t)(nl) + 2 + PT_LIGHT_TABLE_TILES(nl))
hipError_t ptk_light_table(const PtRawTriangle* tris, int ntri, const PtRawMaterial* mats, int nmat, const int32_t* lights, int nl,
                           uint64_t* cdf, uint32_t* tri_q, hipStream_t s);
// pt_env_table: the selection table of the N * N texels of an octahedral map, on the light table's layout, tiling and scan -- cdf:
// PT_LIGHT_TABLE_WORDS(N * N) uint64, cdf[0 .. N * N], then the same scratch.  Two kernels of its own (the texels' weights and their
// maximum; quantise and tile sums), then pt_light_table's two scans, unchanged.  There is no second table: q_i = cdf[i + 1] - cdf[i]
#define PT_ENV_SIZE_MAX 2048
hipError_t ptk_env_table(const float4* texels, int N, uint64_t* cdf, hipStream_t s);
// sample moments (pt_sample_moments, pt_moments_resolve): the records of include/pt_shim.h
struct PtPixelMoments {           // pt_pixel_moments, 56 bytes
    double sum[3], sum2[3];
    uint32_t n, rejected;
};
struct PtNoiseSummary {           // pt_noise_summary, 48 bytes
    double var_sum, se2_sum, mean2_sum;
    uint64_t pixels, samples, rejected;
};
#define PT_MOMENTS_UNROLL 8       // frames whose loads the accumulate kernel keeps in flight
#define PT_MOMENTS_TILE 2048      // elements a workgroup of the resolve kernel reduces: 2048^3 >= 2^32, three levels at the most
#define PT_MOMENTS_TILES(n) (((size_t)(n) + PT_MOMENTS_TILE - 1) / PT_MOMENTS_TILE)
// the summary buffer: record 0 the result, then the sums of level 0's tiles, then those of level 1's (the third level is one tile)
#define PT_MOMENTS_SUMMARY_RECORDS(n) ((size_t)1 + PT_MOMENTS_TILES(n) + PT_MOMENTS_TILES(PT_MOMENTS_TILES(n)))
// moments[p] (from zeros when reset) takes samples[f][p][0..2], f = 0 .. frames - 1 ascending; one lane per pixel, one launch
hipError_t ptk_sample_moments(const float* samples, PtPixelMoments* moments, uint32_t npix, int32_t frames, bool reset, hipStream_t s);
// noise (may be NULL): {float var[3]; uint32 n}[npix]; summary (may be NULL): PT_MOMENTS_SUMMARY_RECORDS(npix) records, the result in
// record 0.  One launch per level of 2048-element tiles
hipError_t ptk_moments_resolve(const PtPixelMoments* moments, uint32_t npix, void* noise, PtNoiseSummary* summary, hipStream_t s);
// rays[2 gid], rays[2 gid + 1] = the pt_ray of pixel gid, frame `frame` (the renderer's sample start) for the camera cam
hipError_t ptk_camera_rays(const PtLensCamera& cam, int width, int height, int frame, float4* rays, hipStream_t s);
// dynamic LDS of a trace workgroup (pt_kernels.hip: pt_lds_total, pt_bvh_lds_total)
size_t ptk_trace_lds_bytes(int ntri);
int ptk_trace_blocks_per_cu(int ntri);
int ptk_trace_bvh_blocks_per_cu(void);
size_t ptk_trace_bvh_lds_bytes(void);
