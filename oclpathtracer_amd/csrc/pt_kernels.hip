// pt_kernels.hip -- hand-written gfx950 kernels of the path-tracing hot path.
//
// What the reference runs as ONE OpenCL mega-kernel per frame
// (test/ClKernels/GenerateColors.cl:302-322: one work-item = one pixel = one path, then a
// read-modify-write of the gamma-encoded running mean) is restructured for CDNA4 as
//
//   pt_prep_kernel   once per scene upload: Triangle -> {p1, e1, e2, n, id}; for scenes made of
//                    quads also the slack and the packed table of the pass-1 filter
//   pt_trace_kernel  persistent waves; every LANE holds one path at a time.  A wave takes batches of consecutive
//                    samples off a global queue and keeps up to 64 PARKED paths in LDS: lanes whose path has
//                    ended take a parked one; when the pool is empty the wave parks its live paths and starts
//                    64 fresh samples -- 64 consecutive pixels, camera rays at full lane width, a coherent
//                    first bounce (pt_start_fresh, pt_pool_push / pt_pool_pop).  The closest-hit search is
//                    two-pass: pass 1 walks the triangles with a wave-uniform index (per-triangle constants are
//                    scalar loads consumed as SGPR operands) and keeps, per lane, a bit mask of the triangles
//                    that MAY pass the cull and u tests -- a conservative filter, in its strongest form one
//                    packed FMA chain deciding four triangles (pt_quad3_pass1; fresh primary rays read their
//                    masks from a per-pixel table instead: pt_primary_mask_kernel); pass 2 lets every lane run
//                    the exact reference test on its own survivors, fetched per lane from an LDS copy of the
//                    records, and balances the last ones across the wave's lanes (pt_tail_round).  Scenes of
//                    512 triangles or more walk an LBVH instead (pt_trace_bvh_body, pt_bvh_step, pt_bvh.hip).
//                    Path radiance goes to rad[frame][pixel] (three floats).
//   pt_fold_kernel   per pixel channel, in ascending frame order, replays the reference's
//                    gamma -> mean -> degamma arithmetic (GenerateColors.cl:314-321) over the
//                    staged radiances: bit-identical to frame-by-frame launches.
//
// The arithmetic is PTSPEC (pt_device_math.h); results are bit-identical to oracle/pt_oracle.c.
#include "pt_kernels.h"

#include "pt_device_math.h"
#include "pt_secmask.h"

#include <type_traits>
#include <utility>

typedef const __attribute__((address_space(4))) float* pt_const_f32p;  // scalar (SMEM) loads

PTK_DEV unsigned pt_lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// number of set bits of m below this lane's position
PTK_DEV unsigned pt_mbcnt(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); }

// The trace kernels' argument block, RE-READ where it is used.  Passed by value, PtTraceParams lands in ~40 SGPRs at
// kernel entry and stays live through the bounce loop; at 7 waves per SIMD the compiler then spills SGPRs to VGPR
// lanes and pays v_readlane_b32 -- VALU issue slots, the resource this kernel is bound by -- in every bounce (24 per
// bounce before this).  The fields that only regeneration and shading need are instead loaded from the kernarg
// segment at their point of use: s_load on the scalar memory pipe, nothing live in between.  (The empty asm makes the
// pointer opaque so the loads are not hoisted back out of the loop.)
typedef const __attribute__((address_space(4))) PtTraceParams* pt_kargs_p;
PTK_DEV pt_kargs_p pt_kargs()
{
    pt_kargs_p k = (pt_kargs_p)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return k;
}
// the anchor of the pass-1 filters (the render's eye, PtTraceParams::cam), read where a ray is checked -- in EVERY trace kernel,
// like the camera where rays are made (PT_CAM_K(K->cam)): the LBVH kernel's SGPRs are spent already
PTK_DEV f3 pt_anchor()
{
    const pt_kargs_p K = pt_kargs();
    return mk3(K->cam.eye[0], K->cam.eye[1], K->cam.eye[2]);
}
// LATE (template parameter of the functions below): read the argument where it is used (the table trace kernels), or take
// it from the by-value copy (the LBVH kernel, which has SGPRs to spare and measured 13 % slower with late reads)
#define PT_ARG(field) (LATE ? K->field : P.field)

// ------------------------------------------------------------------------------------------
// scene preparation
// ------------------------------------------------------------------------------------------
__global__ void pt_prep_kernel(const PtRawTriangle* __restrict__ raw, PtPrepTriangle* __restrict__ out, int ntri,
                               unsigned int* __restrict__ det_bound_bits)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntri) return;
    f3 p1 = mk3(raw[i].p1[0], raw[i].p1[1], raw[i].p1[2]);
    f3 p2 = mk3(raw[i].p2[0], raw[i].p2[1], raw[i].p2[2]);
    f3 p3 = mk3(raw[i].p3[0], raw[i].p3[1], raw[i].p3[2]);
    f3 e1 = sub3(p2, p1);          // GenerateColors.cl:92
    f3 e2 = sub3(p3, p1);          // :93
    f3 n = cross3(e2, e1);         // :123
    PtPrepTriangle t;
    t.p1[0] = p1.x; t.p1[1] = p1.y; t.p1[2] = p1.z;
    t.e1[0] = e1.x; t.e1[1] = e1.y; t.e1[2] = e1.z;
    t.e2[0] = e2.x; t.e2[1] = e2.y; t.e2[2] = e2.z;
    t.pad0[0] = t.pad0[1] = t.pad0[2] = 0.0f;
    t.n[0] = n.x; t.n[1] = n.y; t.n[2] = n.z;
    t.id = raw[i].id;
    out[i] = t;
    // upper bound of |det| = |dot(e1, cross(dir, e2))| <= |e1| |e2| |dir| for this triangle, as
    // L1 norms; non-negative floats order like their bit patterns, NaN/Inf sort above all finite
    float b = (__builtin_fabsf(e1.x) + __builtin_fabsf(e1.y) + __builtin_fabsf(e1.z)) *
              (__builtin_fabsf(e2.x) + __builtin_fabsf(e2.y) + __builtin_fabsf(e2.z));
    atomicMax(&det_bound_bits[0], __float_as_uint(b) & 0x7fffffffu);
    // quad structure (pt_quad_pass1): triangle 2k+1 must have e2 == -e2 of triangle 2k.  Numeric
    // equality, so a zero of either sign matches; a NaN never does.  word 1 counts violations.
    if (i & 1) {
        f3 q1 = mk3(raw[i - 1].p1[0], raw[i - 1].p1[1], raw[i - 1].p1[2]);
        f3 q3 = mk3(raw[i - 1].p3[0], raw[i - 1].p3[1], raw[i - 1].p3[2]);
        f3 f2 = sub3(q3, q1);
        if (!(e2.x == -f2.x && e2.y == -f2.y && e2.z == -f2.z)) atomicAdd(&det_bound_bits[1], 1u);
        // (a,b,c),(c,d,a): this triangle starts at its predecessor's third vertex (pt_quad2_pass1)
        if (!(p1.x == q3.x && p1.y == q3.y && p1.z == q3.z)) atomicAdd(&det_bound_bits[3], 1u);
    }
    // the scene's bounding box, per axis, for the radius about the render's eye (pt_quad2_pass1's error bound; the host
    // derives it per camera: pt_shim.hip, anchor_radius) and a flag for coordinates that are not finite
    {
        const f3 vs[3] = { p1, p2, p3 };
        bool fin = true;
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) { lo[a] = hi[a] = a == 0 ? p1.x : a == 1 ? p1.y : p1.z; }
        for (int k = 0; k < 3; ++k) {
            const float c[3] = { vs[k].x, vs[k].y, vs[k].z };
            for (int a = 0; a < 3; ++a) {
                fin = fin && __builtin_isfinite(c[a]);
                lo[a] = c[a] < lo[a] ? c[a] : lo[a];
                hi[a] = c[a] > hi[a] ? c[a] : hi[a];
            }
        }
        if (!fin) atomicOr(&det_bound_bits[2], 1u);
        for (int a = 0; a < 3; ++a) {
            atomicMax(&det_bound_bits[6 + a], ~ptk_order_key(lo[a]));
            atomicMax(&det_bound_bits[9 + a], ptk_order_key(hi[a]));
        }
    }
    // words 4, 5: a 64-bit checksum of the raw records (position-dependent mix per record, summed: order of arrival does not matter).
    // A buffer the caller can write behind the ABI is prepared again for every render (pt_shim.hip); the checksum tells whether that
    // changed anything, i.e. whether the LBVH and the primary-ray masks made from the previous contents still stand.
    {
        const unsigned* w = reinterpret_cast<const unsigned*>(raw + i);
        unsigned long long h = 0x9e3779b97f4a7c15ull * (unsigned long long)(i + 1);
        for (int k = 0; k < 16; ++k) {
            h ^= (unsigned long long)w[k] + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
            h *= 0xff51afd7ed558ccdull;
            h ^= h >> 33;
        }
        atomicAdd(reinterpret_cast<unsigned long long*>(det_bound_bits + 4), h);
    }
}

// Second pass of the scene preparation for quad mode 2 (see pt_quad2_pass1 for the derivation):
// record 2k+1 gets pad0[0] = delta3 = slack of the lower bound of its shared-u test.
//   delta2 = |e1' + e1|_2 |e2|_2 (how far the pair is from a parallelogram) + 128 u D^2
//   delta3 = delta2 * c + delta1
// every factor inflated by 0.1 % to cover the rounding of this very computation.
__global__ void pt_prep_quad_margins_kernel(PtPrepTriangle* __restrict__ out, int ntri, float diameter, float delta1)
{
    int i = 2 * (blockIdx.x * blockDim.x + threadIdx.x) + 1;
    if (i >= ntri) return;
    const PtPrepTriangle a = out[i - 1], b = out[i];
    float wx = b.e1[0] + a.e1[0], wy = b.e1[1] + a.e1[1], wz = b.e1[2] + a.e1[2];
    float wn = __builtin_sqrtf(wx * wx + wy * wy + wz * wz) * 1.001f;
    float en = __builtin_sqrtf(a.e2[0] * a.e2[0] + a.e2[1] * a.e2[1] + a.e2[2] * a.e2[2]) * 1.001f;
    float delta2 = wn * en * 1.001f + 128.0f * 5.9604645e-8f * diameter * diameter * 1.001f;
    float delta3 = (delta2 * 1.00001f + delta1) * 1.001f;
    out[i].pad0[0] = delta3;  // +Inf / NaN keep every second triangle of the pair: valid, merely slow
}

// Third pass of the scene preparation, quad mode 3 (pt_quad3_pass1): per PAIR of quads (2p, 2p+1)
// the operands of the packed pass-1 filter, interleaved {quad 2p, quad 2p+1} so that every one is
// an SGPR pair of a v_pk_fma_f32:
//   n' = cross(e2, e1) * 1.000002f   (det * c = dir . n')
//   e2, K = cross(e2, a - anchor)    (un = e2 . ((o - anchor) x dir) - dir . K; anchor = the render's eye)
//   dhi = delta3 + deltaD * c + deltaP (slack of the outer bound; -1 for the padding quad)
__global__ void pt_prep_p1tab_kernel(const PtPrepTriangle* __restrict__ tris, int ntri, float diameter, float* __restrict__ tab,
                                     float ax, float ay, float az)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int nquads = ntri / 2;
    if (2 * p >= nquads) return;
    const float uD2 = 5.9604645e-8f * diameter * diameter;
    const float deltaP = 192.0f * uD2 * 1.001f, deltaD = 128.0f * uD2 * 1.001f;
    float* t = tab + (size_t)p * PT_P1_STRIDE;
    for (int h = 0; h < 2; ++h) {
        const int q = 2 * p + h;
        float v[10] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1.0f };  // padding: |un| = 0 > -1 fails
        if (q < nquads) {
            const PtPrepTriangle a = tris[2 * q], b = tris[2 * q + 1];
            const f3 e2 = mk3(a.e2[0], a.e2[1], a.e2[2]);
            const f3 ac = mk3(a.p1[0] - ax, a.p1[1] - ay, a.p1[2] - az);
            const f3 K = cross3(e2, ac);
            v[0] = a.n[0] * 1.000002f; v[1] = a.n[1] * 1.000002f; v[2] = a.n[2] * 1.000002f;
            v[3] = e2.x; v[4] = e2.y; v[5] = e2.z;
            v[6] = K.x; v[7] = K.y; v[8] = K.z;
            v[9] = (b.pad0[0] + deltaD * 1.000002f + deltaP) * 1.001f;
        }
        for (int k = 0; k < 10; ++k) t[2 * k + h] = v[k];
    }
    for (int k = 20; k < PT_P1_STRIDE; ++k) t[k] = 0.0f;
}

// ------------------------------------------------------------------------------------------
// camera: GenerateColors.cl:73-87, 263-288
// ------------------------------------------------------------------------------------------
// the camera ray through image-plane position (x, y), in pixels (GenerateColors.cl:265-287 after the jitter).
// inv_w = 1.0f / (float)W, inv_h = 1.0f / (float)H, aspect = (float)W / (float)H are IEEE quotients of image constants:
// computed once on the host (PtTraceParams), the same bits as :266-267 evaluated per work-item.
// The camera (eye, and the basis of :270-276 with angle = tan(fov / 2) of :268) is the render's, derived ONCE per render on
// the host with PTSPEC's normalize / cross (pt_camera_derive, pt_shim.hip): the same bits as :270-276 evaluated per
// work-item.  For the reference's camera (eye (0, 2.75, 4), center = eye + (0,0,-1), up = (0,1,0), 60 degrees) it is exactly
//     viewDir = (+0, +0, -1)     holDir = (1, -0, +0)     upDir = (+0, 1, +0)     angle = 0x1.279a74p-1f
// (every length is exactly 1; the signed zeros are those of the fma forms).  The per-ray expression below is the reference's,
// unchanged.  Callers read the camera from the kernarg segment where rays are made (PT_CAM_K), so that its thirteen values
// occupy no registers for the kernel's lifetime.
struct PtCam { f3 eye, view, hol, up; float angle; };
#define PT_CAM_K(c) PtCam{ mk3((c).eye[0], (c).eye[1], (c).eye[2]), mk3((c).view[0], (c).view[1], (c).view[2]), \
                           mk3((c).hol[0], (c).hol[1], (c).hol[2]), mk3((c).up[0], (c).up[1], (c).up[2]), (c).angle }

// the ray of image point (x, y) as the reference hands it to getRay at :287: `aim` is normalised ONCE (getRay normalises it again)
PTK_DEV void pt_camera_aim(float x, float y, float inv_w, float inv_h, float aspect, const PtCam& c, f3& org, f3& aim)
{
    const float angle = c.angle;
    const f3 eye = c.eye;
    const f3 viewDir = c.view;
    const f3 holDir = c.hol;
    const f3 upDir = c.up;

    x = (2.0f * ((x + 0.5f) * inv_w) - 1.0f) * angle * aspect;
    y = -(1.0f - 2.0f * ((y + 0.5f) * inv_h)) * angle;

    float my = -1.0f * y;
    f3 d = add3(add3(scale3(holDir, x), scale3(upDir, my)), viewDir);
    f3 dir = normalize3(d);
    f3 pointAimed = add3(eye, scale3(dir, 4.0f));
    org = eye;
    aim = normalize3(sub3(pointAimed, eye));  // :287
}

PTK_DEV void pt_camera_ray(float x, float y, float inv_w, float inv_h, float aspect, const PtCam& c, f3& org, f3& dir_out)
{
    f3 aim;
    pt_camera_aim(x, y, inv_w, inv_h, aspect, c, org, aim);
    dir_out = normalize3(aim);  // getRay's own normalize (:75)
}

// the jittered image point of pixel (xc, yc): :278-279, two draws, x first
PTK_DEV void pt_pixel_jitter(int xc, int yc, uint32_t& seed, float& x, float& y)
{
    x = (float)xc + pt_random_float(seed) - 0.5f;
    y = (float)yc + pt_random_float(seed) - 0.5f;
}

PTK_DEV void pt_generate_ray(int xc, int yc, float inv_w, float inv_h, float aspect, const PtCam& c, uint32_t& seed, f3& org, f3& dir_out)
{
    float x, y;
    pt_pixel_jitter(xc, yc, seed, x, y);
    pt_camera_ray(x, y, inv_w, inv_h, aspect, c, org, dir_out);
}

// The thin lens (include/pt_shim.h: pt_camera), for lens_radius R > 0: after the jitter draws and `dir` of :278-284, two more draws,
// u1 then u2; the origin is the point (r cos(phi), r sin(phi)), r = R sqrt(u1), phi = TWO_PI u2, of the disc in the plane of holDir and
// upDir about the eye (uniform in area), and the ray goes from it through pointAimed = eye + F dir -- :285 with its literal 4.0f made
// the focus distance F.  `aim` is what getRay receives at :287, normalised once, as pt_camera_aim's.  Its temporaries die here: what
// leaves is an origin and a direction, as from the pinhole.
PTK_DEV void pt_lens_aim(float x, float y, float inv_w, float inv_h, float aspect, const PtCam& c, float R, float F, uint32_t& seed, f3& org,
                         f3& aim)
{
    // The two draws follow the jitter's in the seed's sequence; what is COMPUTED first is the lens point, while only x and y wait: at most
    // five values of this function are live at a time (its callers sit inside refill loops with every register spoken for).
    // phi = TWO_PI u2 <= RN(2 pi) < PTK_F32_SINCOS_MAX for u2 in [0, 1] (getRandomFloat may return 1.0): the binary32 form, no guard
    const float u1 = pt_random_float(seed);
    const float u2 = pt_random_float(seed);
    const float r = R * pt_sqrt(u1);
    const float phi = PTK_TWO_PI * u2;
    float sp, cp;
    pt_sincos_f32<true>(phi, sp, cp);
    const float lx = r * cp, ly = r * sp;
    org = add3(add3(c.eye, scale3(c.hol, lx)), scale3(c.up, ly));
    x = (2.0f * ((x + 0.5f) * inv_w) - 1.0f) * c.angle * aspect;
    y = -(1.0f - 2.0f * ((y + 0.5f) * inv_h)) * c.angle;
    const float my = -1.0f * y;
    const f3 dir = normalize3(add3(add3(scale3(c.hol, x), scale3(c.up, my)), c.view));
    const f3 pointAimed = add3(c.eye, scale3(dir, F));
    aim = normalize3(sub3(pointAimed, org));  // :287
}

// The lens of a launch that starts its samples through pt_item_begin / pt_list_item_begin, RE-READ from the kernarg segment where a sample
// starts, as the trace kernels re-read their block (pt_kargs): every such kernel's first argument begins { PtTraceParams t; PtLensCamera
// cam; ... } (PtAoParams, PtDirectParams and what is built on it).  The roulette, list and LBVH kernels start samples inside their refill
// loop and several sit exactly on a register step: taken from the by-value copy, the two values and the test on them were hoisted out of
// that loop and stayed live through the searches -- ten more SGPR spills and, in 24 instantiations, a vector spill.  Read here, nothing of
// the lens is live once the sample has its ray.
struct PtLensArgs { PtTraceParams t; PtLensCamera cam; };
PTK_DEV const __attribute__((address_space(4))) PtLensCamera* pt_lens_kargs()
{
    typedef const __attribute__((address_space(4))) PtLensArgs* args_p;
    args_p k = (args_p)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return &k->cam;
}

// the sample start's ray, with or without a lens: the branch is uniform for a launch, and lens_radius = 0 (-0, too) takes pt_generate_ray
// as it stands, whatever focus_distance holds.  `cam` is the launch's camera, the by-value copy of what pt_lens_kargs reads
PTK_DEV void pt_generate_lens_ray(int xc, int yc, float inv_w, float inv_h, float aspect, const PtLensCamera& cam, uint32_t& seed, f3& org,
                                  f3& dir_out)
{
    const auto* lens = pt_lens_kargs();
    const float R = lens->lens_radius;
    if (R > 0.0f) {
        float x, y;
        pt_pixel_jitter(xc, yc, seed, x, y);
        f3 aim;
        pt_lens_aim(x, y, inv_w, inv_h, aspect, PT_CAM_K(cam), R, lens->focus_distance, seed, org, aim);
        dir_out = normalize3(aim);  // getRay's own normalize (:75)
    } else {
        pt_generate_ray(xc, yc, inv_w, inv_h, aspect, PT_CAM_K(cam), seed, org, dir_out);
    }
}

// ------------------------------------------------------------------------------------------
// primary-ray candidate masks (quad scenes of up to 64 triangles)
// ------------------------------------------------------------------------------------------
// The camera is fixed for a render (eye, basis: PtCamera), so what a pixel's primary rays can hit is a property of the
// pixel: every frame's ray goes through the pixel's footprint, jittered by less than half a pixel (:278-281).  The packed
// table is made about the render's eye (K = cross(e2, a - eye)) and a primary ray starts exactly AT the eye (org = eye,
// bit for bit), so M = (o - eye) x dir = 0 and pass 1's two forms (pt_quad3_pass1) are LINEAR in the direction:
// un(d) = -K . d, T(d) = n' . d + dhi.  Over the footprint the direction stays within eps of the centre ray's d_c in every
// component:
//     the unnormalised direction x hol + my up + view moves by at most |dx hol + dmy up|_2 <= (|dx|^2 + |dmy|^2)^(1/2) (1 + 2e-6)
//     for dx <= angle aspect / W, dmy <= angle / H: hol and up come out of three float normalisations, so each has unit
//     length within a few ulp (< 1e-6 relative) and hol . up is a rounding residue of the same size, |cos| < 1e-6 -- the
//     Gram factor (1 + |cos|)^(1/2) (1 + 1e-6) stays below 1 + 2e-6.  Its length is >= |view| (1 - 1e-6) (view is
//     orthogonal to hol, up up to the same residues, and |view| = 1 within an ulp), and radial projection onto the unit
//     sphere from outside the ball of radius 1 - 1e-6 is (1 + 1e-6)-Lipschitz: together a factor below 1 + 4e-6;
//     eps = 1.01 h + 4e-6 covers it with room to spare (the 1.01 alone is 2 500 times the 4e-6 needed), and its additive
//     4e-6 covers the rounding of the reference's own ray set-up (three normalisations of a unit-length vector).
// PREMISE: dx and dmy above are half a pixel, that is, the image-plane point a kernel computes -- fl(fl(xc + r) - 0.5) of
// pt_pixel_jitter through the first two lines of pt_camera_aim -- is the real one to a small part of a pixel.  Those
// roundings are 2^-24-relative to the pixel COORDINATE: 12 of them between a sample and this kernel's centre, 24 2^-24 angle
// (aspect^2 + 1)^(1/2) on the image plane, against the 0.0099 h the 1.01 has to give (h = 2^(1/2) angle / H: pixels are
// square).  From column 2^23 on a jittered x is not even in its own pixel.  The HOST therefore launches this kernel only
// for images with W^2 + H^2 <= 7626^2 (pmask_footprint_holds, pt_shim.hip, where the roundings are counted one by one);
// every other render runs pass 1 for its primary rays, as under PT_OPT_PRIMARY_MASKS 0.
// A primary ray's origin is the eye bit for bit, so for triangle {p1, e1, e2} the reference's tvec = fl(eye - p1), its
// qvec = fl_cross(tvec, e1) and the numerator of t, tn = fl_dot(e2, qvec), are per-triangle CONSTANTS -- formed here by the
// very operations of pt_tri_pass2, hence the same bits -- and the other three numerators are LINEAR in the direction:
//     det(d) = d . Kd,  Kd = e2 x e1        un(d) = d . Ku,  Ku = e2 x tvec        vn(d) = d . qvec
// The reference accepts a pair (:96-125) only if det >= 1e-8, u >= 0, v >= 0, u + v <= 1 and 0 < t < 1e20, with
// u = fl(un inv), v = fl(vn inv), t = fl(tn inv), inv = RN(1 / det) > 0.  In terms of ITS floats un_ref, vn_ref, det_ref:
//     u >= 0 (or -0)   =>  un_ref >= -1e-24        (pt_tri_pass1: below that the product is a negative non-zero float)
//     v >= 0           =>  vn_ref >= -1e-24        (the same)
//     fl(u + v) <= 1   =>  un_ref + vn_ref <= det_ref * 1.000001   (three roundings and RN(1 / det), each 1 - 2^-24; an
//                          underflowing product loses at most 2^-150)
//     t > 0            =>  tn > 0                  (inv > 0: the sign of t is the sign of the constant; no footprint term)
// (u <= 1 follows from v >= 0 and u + v <= 1; t < 1e20 is left to pass 2.)
// What this kernel evaluates is X_c = fl_dot(d_c, fl_cross(.,.)) at the centre direction.  With S = |a|_1 |b|_1 for the form
// a . (d x b), u = 2^-24 and |d|_2^2 <= 1.001 (a thrice-normalised direction):
//     the reference:  a cross product's component is one product and one fma, |error| <= u (|x y| + |component|) <= 2.1 u S';
//                     a three-term fma dot errs by <= 3.01 u sum|x_i y_i|.  det_ref and un_ref (dot of a, the cross of d and
//                     b: S' = |b|_1, |pvec_k| <= 1.001 |b|_1) are within (2.1 + 3.02) u S of the real form, vn_ref (dot of
//                     d, |d|_1 <= 1.74, and a cross of constants) within (1.74 * 2.1 + 3.02) u S:           < 7 u S
//     here:           dot of d_c and a cross of constants, as vn_ref:                                      < 7 u S
//     the footprint:  |X(d) - X(d_c)| <= eps |K_real|_1 <= eps (|K_float|_1 + 6.3 u S)
//     the comparisons below: a sum of two of these floats errs by <= u (|X_c| + rho) with |X_c| <= 1.001 S:  < 2 u S each
// Together |X_ref(d) - X_c| <= eps |K|_1 + (32 + 8 eps) u S =: rho for every ray d of the pixel (32 against the 20 needed),
// inflated by 0.1 % against the roundings of forming it, plus an absolute 2e-24 that covers the -1e-24 above and every
// underflow.  The bit is cleared only when one of the five conditions then fails for ALL of the footprint; every comparison
// is written so that a NaN keeps the bit.  One thread per local pixel writes the two 32-bit chunk masks in pass 1's own bit
// order; a FRESH wave of primary rays then loads its masks instead of running pass 1 (which is a third of a bounce), and
// its pass 2 meets about 1.2 candidates per ray instead of 3 (oracle, Cornell box: 17.0 of 36 pairs culled, 15.9 fail u,
// 1.8 fail v, 1.2 accepted).  Everything downstream (the exact tests of pass 2) is unchanged, so the pixels are too;
// tools/validate_filter.py counts violations of the cached masks -- pairs the reference ACCEPTS but a mask dropped --
// like those of any other filter.
struct PtMaskParams {
    const PtPrepTriangle* tris;   // the prepared records {p1, e1, e2}
    uint2* out;
    int32_t width, height, ntri;
    int32_t stripe_rows, n_ranks, rank;
    uint32_t npix_local;
    PtCamera cam;   // the render's
};

PTK_DEV float pt_norm1(const f3& a) { return __builtin_fabsf(a.x) + __builtin_fabsf(a.y) + __builtin_fabsf(a.z); }

__global__ void pt_primary_mask_kernel(const PtMaskParams P)
{
    const unsigned lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= P.npix_local) return;
    const unsigned lr = lp / (unsigned)P.width, x = lp - lr * (unsigned)P.width;
    unsigned grow = lr;
    if (P.n_ranks > 1) {
        const unsigned sl = lr / (unsigned)P.stripe_rows;
        const unsigned within = lr - sl * (unsigned)P.stripe_rows;
        grow = (sl * (unsigned)P.n_ranks + (unsigned)P.rank) * (unsigned)P.stripe_rows + within;
    }
    f3 o, dc;
    const PtCam cam = PT_CAM_K(P.cam);
    pt_camera_ray((float)x, (float)grow, 1.0f / (float)P.width, 1.0f / (float)P.height, (float)P.width / (float)P.height, cam, o, dc);  // the jitter's midpoint: xi = 0.5
    const float hx = cam.angle * ((float)P.width / (float)P.height) / (float)P.width;
    const float hy = cam.angle / (float)P.height;
    const float eps = __builtin_sqrtf(hx * hx + hy * hy) * 1.01f + 4e-6f;
    const float uS = (32.0f + 8.0f * eps) * 5.9604645e-8f;  // (32 + 8 eps) u
    const float A = 2e-24f;
    unsigned m[2] = { 0u, 0u };
    for (int j = 0; j < P.ntri; ++j) {
        const PtPrepTriangle* t = P.tris + j;
        const f3 e1 = mk3(t->e1[0], t->e1[1], t->e1[2]), e2 = mk3(t->e2[0], t->e2[1], t->e2[2]);
        const f3 tv = mk3(o.x - t->p1[0], o.y - t->p1[1], o.z - t->p1[2]);  // o is the eye, bit for bit
        const f3 Kd = cross3(e2, e1), Ku = cross3(e2, tv), qv = cross3(tv, e1);
        const float tn = dot3(e2, qv);  // :122's numerator, the bits of pt_tri_pass2
        const float detc = dot3(dc, Kd), unc = dot3(dc, Ku), vnc = dot3(dc, qv);
        const float a1 = pt_norm1(e1), a2 = pt_norm1(e2), at = pt_norm1(tv);
        const float rho_d = (eps * pt_norm1(Kd) + uS * (a1 * a2)) * 1.001f + A;
        const float rho_u = (eps * pt_norm1(Ku) + uS * (at * a2)) * 1.001f + A;
        const float rho_v = (eps * pt_norm1(qv) + uS * (at * a1)) * 1.001f + A;
        // NaNs fail every comparison and are kept, as in pass 1
        const bool keep = !(detc + rho_d < 0.999e-8f)                                       // :100
                        & !(unc + rho_u < 0.0f)                                             // :109, u >= 0
                        & !(vnc + rho_v < 0.0f)                                             // :117, v >= 0
                        & !((unc - rho_u) + (vnc - rho_v) > (detc + rho_d) * 1.000002f)     // :117, u + v <= 1
                        & !(tn <= 0.0f);                                                    // :125, t > 0
        const int c = j >> 5;
        const int nc = P.ntri - 32 * c < 32 ? P.ntri - 32 * c : 32;
        m[c] |= (keep ? 1u : 0u) << (nc - 1 - (j & 31));
    }
    P.out[lp] = make_uint2(m[0], m[1]);
}

// ------------------------------------------------------------------------------------------
// secondary-ray candidate masks (quad scenes of up to 64 triangles): the table of pt_secmask.h, where the derivation stands
// ------------------------------------------------------------------------------------------
// Once per scene: the first ntri threads write the classification records of the table's head, then one thread per cell writes its
// mask (pt_sm_entry, binary64: the very function the host test compiles).  Nothing of it depends on a camera or an image.
// A cell's work is a walk through boxes whose length differs a hundredfold between cells, and a wave takes as long as its longest lane.
// How long a cell takes follows its direction more than its tile (a direction below the surface is done after one box per triangle),
// so the lanes of a wave take the SAME direction cell over consecutive tiles -- thread i of a triangle has the cell (tile i % T^2,
// direction i / T^2) -- and no register may spill: 256 threads per block leave the walk its 188 VGPRs (profiles/tight_masks/pmc_summary.txt).
__global__ __launch_bounds__(256) void pt_secondary_mask_kernel(const PtPrepTriangle* tris, int ntri, uint2* table)
{
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (unsigned)ntri) reinterpret_cast<PtSmTri*>(table)[i] = pt_sm_tri_record(tris[i].p1, tris[i].e1, tris[i].e2);
    if (i >= (unsigned)ntri * PT_SM_TRI_ENTRIES) return;
    const unsigned k = i / PT_SM_TRI_ENTRIES, within = i - k * PT_SM_TRI_ENTRIES;
    const unsigned dir = within / (PT_SM_T * PT_SM_T), tile = within - dir * (PT_SM_T * PT_SM_T);
    const unsigned e = k * PT_SM_TRI_ENTRIES + tile * PT_SM_DIRS + dir;   // (a permutation of the triangle's cells: e < ntri * PT_SM_TRI_ENTRIES)
    const PtSmMask m = pt_sm_entry(reinterpret_cast<const float*>(tris), ntri, e);
    table[PT_SM_HEAD_ENTRIES + e] = make_uint2(m.x, m.y);
}

// ------------------------------------------------------------------------------------------
// intersectTriangle (GenerateColors.cl:89-135) against a wave-uniform triangle record
// ------------------------------------------------------------------------------------------
struct PtTriRec { float p1x, p1y, p1z, e1x, e1y, e1z, e2x, e2y, e2z; };

PTK_DEV PtTriRec pt_load_tri(pt_const_f32p T, int i)
{
    pt_const_f32p t = T + 16 * i;  // constant address space + uniform index -> s_load
    PtTriRec r;
    r.p1x = t[0]; r.p1y = t[1]; r.p1z = t[2];
    r.e1x = t[3]; r.e1y = t[4]; r.e1z = t[5];
    r.e2x = t[6]; r.e2y = t[7]; r.e2z = t[8];
    return r;
}

// DET_BOUNDED: the host has verified |e1|*|e2| <= 2e19 for every triangle, so det <= 1e20 and
// the short exact reciprocal applies to every front-facing triangle.
#ifndef PT_VALIDATE_FILTER
#define PT_VALIDATE_FILTER 0  // diagnostic: check the pass-1 filter against the reference predicate
#endif
// ---- two-pass closest hit -------------------------------------------------------------------------
// SIMT executes all 44 instructions of the flat test for every lane, but only 9 % of the
// (ray, triangle) pairs get past the u test (:109) -- 50 % are culled at :100, 41 % fail :109.
// Pass 1 (wave-uniform triangle, SGPR operands, 24 VALU): det, 1/det, u and the predicate
// "passes :100 and :109", recorded as one bit per triangle in a per-lane mask.
// Pass 2 (per lane): each lane walks ITS surviving triangles in ascending index and runs the rest
// of the test on them (record fetched with per-lane vector loads, L1-resident); the wave iterates
// max-over-lanes(#survivors) times, ~8 for the Cornell box instead of 36.
// Exactness: a pair that fails :100 or :109 can never be accepted, the survivors are tested with
// the same operations on the same operands, in the same (ascending) order, against the same
// running tmax -- the accepted (t, index) are those of the one-pass loop bit for bit.
// Survivor masks are built MSB-first: m = 2 m + flag is ONE v_addc_co_u32 whose carry-in is the
// comparison's own lane mask (against v_cndmask + v_lshl_or per flag).  After the n flags of a
// chunk, triangle j of the chunk sits at bit n-1-j: pass 2 walks the mask from its highest bit.
// Flags travel as the comparisons' lane masks (ballot of a single compare IS the v_cmp result;
// the conjunction is then an s_and_b64), never as per-lane booleans.
typedef unsigned long long pt_lanes;
#define PT_LANES(cond) __builtin_amdgcn_ballot_w64(cond)
// the other direction: this lane's bit of a wave-uniform mask as a condition -- the mask itself becomes the exec mask or the select's
// condition operand, no per-lane 0/1 is formed
#define PT_ON(mask) __builtin_amdgcn_inverse_ballot_w64(mask)
PTK_DEV unsigned pt_push_flag(unsigned m, pt_lanes c)
{
    unsigned long long carry_out;
    unsigned r;
    asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(carry_out) : "v"(m), "s"(c));
    return r;
}

template <bool DET_BOUNDED>
PTK_DEV pt_lanes pt_tri_pass1(const PtTriRec& r, const f3& o, const f3& d)
{
    float pvx = pt_fma(d.y, r.e2z, -(d.z * r.e2y));
    float pvy = pt_fma(d.z, r.e2x, -(d.x * r.e2z));
    float pvz = pt_fma(d.x, r.e2y, -(d.y * r.e2x));
    float det = pt_fma(r.e1z, pvz, pt_fma(r.e1y, pvy, r.e1x * pvx));
    float tvx = o.x - r.p1x, tvy = o.y - r.p1y, tvz = o.z - r.p1z;
    float un = pt_fma(tvz, pvz, pt_fma(tvy, pvy, tvx * pvx));  // u = un * RN(1/det)
    pt_lanes ok;
    if (DET_BOUNDED) {
        // Pass 2 re-applies :100 and :109 exactly, so pass 1 only has to keep a SUPERSET of the
        // pairs that pass them -- without the reciprocal (a quarter-rate instruction + 2 fma).
        // With det in [1e-8, 1e20] (DET_BOUNDED) and inv = RN(1/det) in [1e-20, 1e8]:
        //   un < -1e-24        =>  un*inv <= -1e-44, rounds to a negative non-zero  =>  u < 0
        //   un > det*1.000001f =>  un*inv >= 1.000001*(1-2^-24)^2 > 1 + 8e-7        =>  u > 1
        // A NaN in det or un fails every "<"/">" here and stays in the mask, as it passes
        // :100/:109 in the reference.  The cull test (:100) itself is left to pass 2: a pair with
        // det < 1e-8 survives these two bounds only for det in [-1e-24, 1e-8), which is rare.
        ok = PT_LANES(!(un < -1e-24f)) & PT_LANES(!(un > det * 1.000001f));
    } else {
        float u = un * (1.0f / det);
        ok = PT_LANES(!(det < 1e-8f)) & PT_LANES(!(u < 0.0f)) & PT_LANES(!(u > 1.0f));  // :100, :109
    }
    return ok;
}

// dynamic LDS of the trace kernels: the workgroup's copy of the hot triangle records
extern __shared__ __attribute__((aligned(16))) float pt_lds_tab[];

// record i for pass 2.  LDS_TABLE selects where the records of a scene live for the per-lane fetches:
//   1  the whole prepared table is copied to LDS once per workgroup (scenes up to PT_LDS_TRI_MAX triangles);
//      i = triangle index, lds_off = 0
//   2  TILED: a larger scene searched by brute force streams the records of the current 32-triangle chunk into a
//      per-wave LDS tile when many lanes have survivors in it (pt_stage_tile); i = index inside the chunk,
//      lds_off = the wave's tile
//   0  per-lane loads from the prepared table in global memory (stride 16 dwords); i = triangle index
// (LDS: stride PT_LDS_TRI_STRIDE dwords, 32-bit LDS addressing; per-lane global loads of a small table saturate
// the CU's vector-memory address path: every lane is its own cache line.)
template <int LDS_TABLE>
PTK_DEV PtTriRec pt_fetch_rec(const PtPrepTriangle* tris, int i, unsigned lds_off = 0u)
{
    float4 q0, q1;
    float e2z;
    if (LDS_TABLE) {
        // 32-bit LDS addressing: through the generic pointer hipcc forms the address with a 64-bit
        // v_mad_u64_u32 per survivor
        typedef __attribute__((address_space(3))) const float pt_lds_f32;
        typedef float pt_v4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) const pt_v4 pt_lds_f32x4;
        pt_lds_f32* t = (pt_lds_f32*)pt_lds_tab + lds_off + __umul24((unsigned)i, (unsigned)PT_LDS_TRI_STRIDE);  // i <= 256
        const pt_v4 a = *(pt_lds_f32x4*)t, b = *(pt_lds_f32x4*)(t + 4);
        q0 = make_float4(a.x, a.y, a.z, a.w);
        q1 = make_float4(b.x, b.y, b.z, b.w);
        e2z = t[8];
    } else {
        const float* t = reinterpret_cast<const float*>(tris + i);
        q0 = *reinterpret_cast<const float4*>(t);
        q1 = *reinterpret_cast<const float4*>(t + 4);
        e2z = t[8];
    }
    PtTriRec r;
    r.p1x = q0.x; r.p1y = q0.y; r.p1z = q0.z;  // p1.xyz e1.x | e1.yz e2.xy | e2.z
    r.e1x = q0.w; r.e1y = q1.x; r.e1z = q1.y;
    r.e2x = q1.z; r.e2y = q1.w; r.e2z = e2z;
    return r;
}

// TILED mode: the records of chunk [base, base + n) into this wave's LDS tile (12 of each record's 16 dwords)
PTK_DEV void pt_stage_tile(const PtPrepTriangle* tris, int base, int n, unsigned tile_off, unsigned lane)
{
    const float* g = reinterpret_cast<const float*>(tris + base);
    for (unsigned k = lane; k < (unsigned)n * PT_LDS_TRI_STRIDE; k += 64u) {
        const unsigned tri = k / PT_LDS_TRI_STRIDE, w = k - tri * PT_LDS_TRI_STRIDE;
        pt_lds_tab[tile_off + k] = g[tri * 16u + w];
    }
    // the wave's own LDS writes, read back by other lanes of the same wave: program order suffices for the
    // hardware (one in-order LDS queue per wave); this keeps the compiler from reordering
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool DET_BOUNDED>
PTK_DEV void pt_tri_pass2(const PtTriRec& r, int i, bool valid, const f3& o, const f3& d, float& tmax, float& hu,
                          float& hv, int& hidx)
{
    float pvx = pt_fma(d.y, r.e2z, -(d.z * r.e2y));
    float pvy = pt_fma(d.z, r.e2x, -(d.x * r.e2z));
    float pvz = pt_fma(d.x, r.e2y, -(d.y * r.e2x));
    float det = pt_fma(r.e1z, pvz, pt_fma(r.e1y, pvy, r.e1x * pvx));
    float inv_det = DET_BOUNDED ? pt_rcp_fast(det) : 1.0f / det;
    float tvx = o.x - r.p1x, tvy = o.y - r.p1y, tvz = o.z - r.p1z;
    float u = pt_fma(tvz, pvz, pt_fma(tvy, pvy, tvx * pvx)) * inv_det;
    // :100, :109 (pass 1 kept a superset).  `u > 1.0f` of :109 needs no compare of its own here: with
    // v >= 0 (or -0) round-to-nearest gives u + v >= u > 1, which :117 rejects below; with v NaN the
    // same NaN reaches t (through qvec or inv_det) and :125 rejects.  The accepted set is unchanged.
    bool ok = valid & !(det < 1e-8f) & !(u < 0.0f);
    float qvx = pt_fma(tvy, r.e1z, -(tvz * r.e1y));
    float qvy = pt_fma(tvz, r.e1x, -(tvx * r.e1z));
    float qvz = pt_fma(tvx, r.e1y, -(tvy * r.e1x));
    float v = pt_fma(d.z, qvz, pt_fma(d.y, qvy, d.x * qvx)) * inv_det;
    ok &= !(v < 0.0f) & !(u + v > 1.0f);  // :117
    float tt = pt_fma(r.e2z, qvz, pt_fma(r.e2y, qvy, r.e2x * qvx)) * inv_det;
    ok &= (tt > 0.0f) & (tt < tmax);  // :125
    tmax = ok ? tt : tmax;
    hu = ok ? u : hu;  // pass 2 runs ~8 times per ray: carrying (u,v) here is cheaper than pt_hit_uv
    hv = ok ? v : hv;
    hidx = ok ? i : hidx;
}

// PT_STAMPS=1 is a DIAGNOSTIC build (tools/stamps.py): per-phase s_memtime shares of a
// wave-bounce go to stats[2..5], the split of pass 2 to stats[8..13]; never shipped, never timed for the bench.
#ifndef PT_STAMPS
#define PT_STAMPS 0
#endif
#if PT_STAMPS
#define PT_STAMP(var) do { __builtin_amdgcn_sched_barrier(0); var = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define PT_STAMP(var) do { } while (0)
#endif
// pass 2 of the PT_STAMPS build, split (ticks of a wave): its own steps, building the pending-pair list, the tail's rounds, the merge at
// the end; and two tallies: iterations of the list-building loops, searches.  Other builds pass no such record and compile none of it.
struct PtStampSplit { unsigned long long own, append, rounds, finish, iters, searches; };

// ---- pass 2, balanced across lanes: the TAIL ---------------------------------------------------------
// Survivors per ray: 3.3 on average, 8.3 at the wave's slowest lane -- walking every lane's own survivors
// to the end ran the exact test at 39 % lane efficiency.  The closest hit is order-free: the winner of the
// reference's ascending loop with its strict `t < tmax` (:125,:145-151) is argmin (t, index) over the
// triangles that pass every other test.  So each lane walks its own survivors only while MANY lanes still
// have one (PT_TAIL_LANES); what is left then -- a few survivors in a few lanes -- is appended as
// (triangle, ray lane) pairs to a per-wave list in LDS, and the pairs are tested 64 at a time, one pair per
// lane whoever owns the ray: the ray travels by ds_bpermute, the candidate's key (t bits, index) goes to the
// ray's slot with one 64-bit ds_min.  At the end of the search a ray whose slot holds a better key than its
// own walk found re-runs the exact test on that one triangle (same operations on the same operands: the
// same t, u, v bit for bit).  The list outlives the 32-triangle chunks of a large scene, so a brute-force
// search over thousands of triangles runs its rare survivors at full lane width too.
// The append loop below moves one pair per lane and iteration: it runs as long as the slowest lane has survivors, 7.4 iterations per
// masked search of the Cornell box and a seventh of a wave-iteration's ticks (profiles/pair_list/stamps.txt).  The masked search of the
// trace kernels builds its list otherwise (pt_pair_list_build, further down); the two-pass, tiled and LBVH searches keep this loop.
#ifndef PT_TAIL_LANES
#define PT_TAIL_LANES 32  // own steps continue while more lanes than this still hold a survivor; 0 = never use the tail
#endif
#define PT_TAIL_LIST 128u  // list capacity: a round is run as soon as 64 pairs are pending, one append adds <= 64

typedef __attribute__((address_space(3))) unsigned pt_lds_u32;
typedef __attribute__((address_space(3))) unsigned long long pt_lds_u64;
struct PtTail {
    pt_lds_u64* keys;  // [64]  best (t bits << 32 | triangle) the tail found for the ray of each lane; ~0 = none
    pt_lds_u32* list;  // [PT_TAIL_LIST]  pending pairs: triangle << 6 | ray lane  (ring)
    unsigned wr, rd;   // wave-uniform ring positions
    unsigned tile;     // TILED mode (pt_fetch_rec): dword offset of this wave's record tile in LDS
    // per lane (as the owner of a ray): the best key its slot has held so far and the (u, v) that came with it
    unsigned long long kbest;
    float ku, kv;
};

// a pending pair = triangle << 6 | ray lane: 2 bytes when the whole scene sits in the LDS table (<= 256 triangles: 14 bits),
// 4 bytes otherwise
typedef __attribute__((address_space(3))) unsigned short pt_lds_u16;
template <int LDS_TABLE> PTK_DEV unsigned pt_tail_get(const PtTail& tl, unsigned i)
{
    return LDS_TABLE == 1 ? (unsigned)((pt_lds_u16*)tl.list)[i] : tl.list[i];
}
template <int LDS_TABLE> PTK_DEV void pt_tail_put(const PtTail& tl, unsigned i, unsigned pair)
{
    if (LDS_TABLE == 1) ((pt_lds_u16*)tl.list)[i] = (unsigned short)pair;
    else tl.list[i] = pair;
}

// the reference's test of one (ray, triangle) pair without the running tmax: passes :100,:109,:117 and 0 < t < 1e20
template <bool DET_BOUNDED>
PTK_DEV bool pt_tri_candidate(const PtTriRec& r, const f3& o, const f3& d, float& t_out, float& u_out, float& v_out)
{
    float pvx = pt_fma(d.y, r.e2z, -(d.z * r.e2y));
    float pvy = pt_fma(d.z, r.e2x, -(d.x * r.e2z));
    float pvz = pt_fma(d.x, r.e2y, -(d.y * r.e2x));
    float det = pt_fma(r.e1z, pvz, pt_fma(r.e1y, pvy, r.e1x * pvx));
    float inv_det = DET_BOUNDED ? pt_rcp_fast(det) : 1.0f / det;
    float tvx = o.x - r.p1x, tvy = o.y - r.p1y, tvz = o.z - r.p1z;
    float u = pt_fma(tvz, pvz, pt_fma(tvy, pvy, tvx * pvx)) * inv_det;
    bool ok = !(det < 1e-8f) & !(u < 0.0f);  // (u > 1 is covered by u + v > 1: see pt_tri_pass2)
    float qvx = pt_fma(tvy, r.e1z, -(tvz * r.e1y));
    float qvy = pt_fma(tvz, r.e1x, -(tvx * r.e1z));
    float qvz = pt_fma(tvx, r.e1y, -(tvy * r.e1x));
    float v = pt_fma(d.z, qvz, pt_fma(d.y, qvy, d.x * qvx)) * inv_det;
    ok &= !(v < 0.0f) & !(u + v > 1.0f);
    float tt = pt_fma(r.e2z, qvz, pt_fma(r.e2y, qvy, r.e2x * qvx)) * inv_det;
    ok &= (tt > 0.0f) & (tt < 1e20f);  // :125 against the initial tmax (:141)
    t_out = tt;
    u_out = u;
    v_out = v;
    return ok;
}

PTK_DEV float pt_from_lane(unsigned byte_addr, float v)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute((int)byte_addr, __float_as_int(v)));
}

// test the first `cnt` (<= 64) pending pairs, one per lane; every lane of the wave takes part (the rays travel by
// ds_bpermute, which needs their owners' lanes enabled)
template <bool DET_BOUNDED, int LDS_TABLE>
PTK_DEV void pt_tail_round(PtTail& tl, unsigned cnt, unsigned lane, const PtPrepTriangle* tris, const f3& o, const f3& d)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const bool act = lane < cnt;
    const unsigned e = act ? pt_tail_get<LDS_TABLE>(tl, (tl.rd + lane) & (PT_TAIL_LIST - 1u)) : 0u;
    const unsigned ray = e & 63u, tri = e >> 6;
    const unsigned a = ray << 2;
    const f3 po = mk3(pt_from_lane(a, o.x), pt_from_lane(a, o.y), pt_from_lane(a, o.z));
    const f3 pd = mk3(pt_from_lane(a, d.x), pt_from_lane(a, d.y), pt_from_lane(a, d.z));
    const PtTriRec r = pt_fetch_rec<(LDS_TABLE == 1 ? 1 : 0)>(tris, (int)tri);  // (a pending pair may be of an earlier chunk than the tile's)
    float t, u, v;
    const bool ok = pt_tri_candidate<DET_BOUNDED>(r, po, pd, t, u, v) & act;
    if (ok) {
        // key = t bits | triangle | the lane that tested the pair: the minimum is the reference's winner (t, then the
        // lower index; a ray's pairs have distinct triangles), and its low bits say where its (u, v) are
        const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)((tri << 6) | lane);
        __hip_atomic_fetch_min(tl.keys + ray, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    // every lane, now as the owner of its ray: did this round improve my slot?  Then fetch (u, v) from the lane that did it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const unsigned long long slot = tl.keys[lane];
    const unsigned from = ((unsigned)slot & 63u) << 2;
    const float pu = pt_from_lane(from, u), pv = pt_from_lane(from, v);
    const bool changed = slot != tl.kbest;
    tl.kbest = slot;
    tl.ku = changed ? pu : tl.ku;
    tl.kv = changed ? pv : tl.kv;
    tl.rd += cnt;
}

// pass 2 of one 32-triangle chunk whose survivor mask is m (bit n-1-j <-> triangle base + j)
template <bool DET_BOUNDED, int LDS_TABLE>
PTK_DEV void pt_pass2_chunk(unsigned m, int base, int n, const PtPrepTriangle* tris, const f3& o, const f3& d, float& tmax, float& hu,
                            float& hv, int& hidx, PtTail& tl, unsigned lane, unsigned& steps, PtStampSplit* sp = nullptr)
{
    (void)sp;
#if PT_STAMPS
    unsigned long long s0 = 0, s1 = 0, s2 = 0, ra = 0, rb = 0, rsum = 0;
    PT_STAMP(s0);
#endif
    // own steps: every lane tests its next survivor (index 0 and ok = false once it has none left),
    // while more than PT_TAIL_LANES lanes still hold one
    if (LDS_TABLE == 2 && (unsigned)__popcll(PT_LANES(m != 0u)) > (unsigned)PT_TAIL_LANES) pt_stage_tile(tris, base, n, tl.tile, lane);
    for (pt_lanes more = PT_LANES(m != 0u); (unsigned)__popcll(more) > (unsigned)PT_TAIL_LANES; more = PT_LANES(m != 0u)) {
        ++steps;
        const bool valid = m != 0u;
        unsigned lz;  // leading zeros: the highest bit is the lowest triangle index (-1 for m = 0)
        asm("v_ffbh_u32_e32 %0, %1" : "=v"(lz) : "v"(m));
        // (a lane without survivors forms a wild index: harmless for the LDS copies -- out-of-range
        // LDS reads return 0 -- and its result is discarded; the global table needs a real address)
        const int i = (LDS_TABLE != 0 || valid) ? base + n - 32 + (int)lz : base;
        m &= ~(0x80000000u >> (lz & 31u));
        const PtTriRec r = LDS_TABLE == 2 ? pt_fetch_rec<2>(tris, n - 32 + (int)lz, tl.tile) : pt_fetch_rec<LDS_TABLE>(tris, i);
        pt_tri_pass2<DET_BOUNDED>(r, i, valid, o, d, tmax, hu, hv, hidx);
    }
    PT_STAMP(s1);
    // the rest of this chunk's survivors join the wave's pending pairs
    if (PT_TAIL_LANES > 0) {
        for (pt_lanes has = PT_LANES(m != 0u); has != 0ull; has = PT_LANES(m != 0u)) {
#if PT_STAMPS
            if (sp) sp->iters++;
#endif
            if (m != 0u) {
                unsigned lz;
                asm("v_ffbh_u32_e32 %0, %1" : "=v"(lz) : "v"(m));
                m &= ~(0x80000000u >> (lz & 31u));
                const unsigned tri = (unsigned)(base + n - 32) + lz;
                pt_tail_put<LDS_TABLE>(tl, (tl.wr + pt_mbcnt(has)) & (PT_TAIL_LIST - 1u), (tri << 6) | lane);
            }
            tl.wr += (unsigned)__popcll(has);
            if (tl.wr - tl.rd >= 64u) {
                ++steps;
                PT_STAMP(ra);
                pt_tail_round<DET_BOUNDED, LDS_TABLE>(tl, 64u, lane, tris, o, d);
#if PT_STAMPS
                PT_STAMP(rb);
                rsum += rb - ra;
#endif
            }
        }
    }
#if PT_STAMPS
    PT_STAMP(s2);
    if (sp) { sp->own += s1 - s0; sp->append += (s2 - s1) - rsum; sp->rounds += rsum; }
#endif
}

// end of a search: the pending pairs, then the merge of what the tail found
template <bool DET_BOUNDED, int LDS_TABLE>
PTK_DEV void pt_pass2_finish(const PtPrepTriangle* tris, const f3& o, const f3& d, float& tmax, float& hu, float& hv, int& hidx,
                             PtTail& tl, unsigned lane, unsigned& steps, PtStampSplit* sp = nullptr)
{
    (void)sp;
#if PT_STAMPS
    unsigned long long s0 = 0, s1 = 0, s2 = 0;
    PT_STAMP(s0);
#endif
    if (PT_TAIL_LANES > 0) {
        if (tl.wr != tl.rd) {
            ++steps;
            pt_tail_round<DET_BOUNDED, LDS_TABLE>(tl, tl.wr - tl.rd, lane, tris, o, d);
        }
        PT_STAMP(s1);
        if (tl.wr != 0u) {  // (wave-uniform) this search used the tail: merge what it found
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // (the constant is made here: hoisted out of the bounce loop it was the register pair the 64-VGPR kernel spilled,
            // and its reload from scratch waited for every store in flight)
            unsigned long long ones;
            asm volatile("v_mov_b64 %0, -1" : "=v"(ones));
            tl.keys[lane] = ones;
            const unsigned long long key = tl.kbest;
            const float kt = __uint_as_float((unsigned)(key >> 32));
            const int ki = (int)((unsigned)key >> 6);
            // the reference's winner is the lexicographic minimum of (t, index)
            const bool better = (key != ~0ull) & ((kt < tmax) | ((kt == tmax) & (ki < hidx)));
            tmax = better ? kt : tmax;
            hu = better ? tl.ku : hu;
            hv = better ? tl.kv : hv;
            hidx = better ? ki : hidx;
        }
    }
#if PT_STAMPS
    PT_STAMP(s2);
    if (sp) { sp->rounds += s1 - s0; sp->finish += s2 - s1; }
#endif
}

// closest hit over triangles [0, ntri): chunks of 32 triangles, pass 1 then pass 2 per chunk.
// (Software-pipelining pass 2 -- fetching the next survivor's record during the current test --
// was measured slower: 64.8 ms against 61.1 ms; the register copies cost more than the LDS latency
// that 7 waves per SIMD already hide.)
// Pass 1 for a quad (a,b,c),(c,d,a) in MODE 2: ONE u numerator decides both triangles.
//
// In A's barycentric frame the second triangle B is the strip u in [-1, 0]: with p1' = c,
// e2' = -e2 (so pvec' = -pvec bit for bit) the reference's own quantities for B are
//     un'  = -fl_dot(fl(o - c), pvec)        det' = -fl_dot(e1', pvec)
// and, were the arithmetic exact and the pair a parallelogram (e1' = -e1), un' = -unA and
// det' = detA.  In binary32 the two differ by rounding and by how far the pair is from a
// parallelogram.  With u = 2^-24, w = e1' + e1, every |coordinate difference| <= D and
// |dir|_2^2 <= 1.001 (both CHECKED per ray by the caller: a ray that violates them keeps every
// triangle), writing pvec = dir x e2 + zeta:
//   |un' + unA| <= |e2.zeta| + |(sigma + rho).pvec| + |eta_a| + |eta_b|
//               <= (9.3 + 6 + 12 + 36) u D^2 < 64 u D^2,          delta1 := 128 u D^2
//       (zeta: rounding of the cross product, <= 3.1 u D per component; sigma = (c - a) - fl(c - a);
//        rho: rounding of o - a and o - c; eta: rounding of a 3-term fma dot, <= 3 u sum|x_i p_i|)
//   |det' - detA| <= |w.pvec| + |eta| + |eta'| <= |w|_2 |e2|_2 1.001 + (18.6 + 36) u D^2 =: delta2
// A pair the reference accepts for B has det' >= 1e-8 and 0 <= u' <= 1, hence (pt_tri_pass1)
// -1e-24 <= un' <= det' * 1.000001, hence
//     unA <= delta1 + 1e-24      and      unA >= -(detA * 1.000001 + delta2 * 1.000001 + delta1).
// The filter below keeps a superset of that (m = fl(detA * 1.000002f) >= detA * 1.000001 for
// detA >= 0; for detA < 0 acceptance needs |detA| <= delta2, where the 0.1 % inflation of delta3
// dominates the 1e-6 relative difference).  delta3 = delta2 * c + delta1 comes prepared per pair
// (pt_prep_quad_margins_kernel).  A NaN anywhere fails every comparison and is kept.
// 25 VALU per quad instead of 34.  tools/validate_filter.py re-checks every dropped pair against
// the literal reference predicate (profiles/r01/filter_validation.txt).
// Pass 1 in MODE 3: the shared-u filter of mode 2 evaluated in Pluecker form, two quads per
// instruction.  tools/ubench_issue (profiles/r01/ubench_issue.log): on gfx950 an fp32 FMA/MUL/ADD
// whose operands are all VGPRs issues at double rate (~2.7 cycles per wave), ANY SGPR operand
// makes it single rate (~4.5), and v_pk_fma_f32 costs ~4.9 with or without an SGPR pair.  Mode 2
// spends 16 single-rate instructions per quad on SGPR operands; here
//     un  = tvec . (dir x e2) = e2 . ((o - eye) x dir) - dir . K,     K  = e2 x (a - eye)
//     T   = det * c + dhi     = dir . n' + dhi,                       n' = (e2 x e1) * c
// where "eye" is the ANCHOR, any fixed point: the identity holds for every one.  It is the render's eye (PtCamera), so a
// primary ray (o = eye bit for bit) has M = 0 exactly (pt_primary_mask_kernel), and the radius the bounds below are sized by
// is the scene's about it (pt_shim.hip: anchor_radius; a camera change rewrites the table and the margins, ensure_anchor).
// With M = (o - eye) x dir computed once per ray: 9 v_pk_fma_f32 give un and T of TWO quads, whose
// per-quad constants come interleaved from the table pt_prep_p1tab_kernel wrote.
// These are other roundings of the same real numbers than the reference's, so BOTH triangles now
// need slack (same assumptions as mode 2: D bounds every coordinate difference, |dir|^2 <= 1.001,
// u = 2^-24):
//   |un_here - un_ref|   <= 33.3 u D^2 (reference: tvec, cross, 3-term dot)
//                         + 51 u D^2 (here: o - eye, M, a - eye, K, 6-term fma chain)   < 192 u D^2 =: deltaP
//   |det_here - det_ref| <= 27.3 u D^2 + 27 u D^2 + 12 u D^2 (c folded into n', dhi into the chain) < 128 u D^2 =: deltaD
// A pair the reference accepts satisfies (pt_tri_pass1, pt_quad2_pass1)
//   first triangle:  -1e-24 <= un_ref <= det_ref c            second: -(det_ref c + delta3) <= un_ref <= delta1
// hence, with dhi = delta3 + deltaD c + deltaP >= deltaD c + deltaP,
//   both: |un_here| <= T;     first: un_here >= -deltaP (= lo);     second: un_here <= delta1 + deltaP (= hi).
// 9 packed + 6 compares + 4 v_addc per PAIR of quads (mode 2: 46).  NaNs fail every comparison and are kept.
typedef float pt_f2 __attribute__((ext_vector_type(2)));
// r = a.lo * s / a.hi * s / fma with the VGPR half broadcast to both results; s = SGPR pair
PTK_DEV pt_f2 pt_pk_mul_lo(pt_f2 a, pt_f2 s) { pt_f2 r; asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(a), "s"(s)); return r; }
PTK_DEV pt_f2 pt_pk_mul_hi(pt_f2 a, pt_f2 s) { pt_f2 r; asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "s"(s)); return r; }
PTK_DEV pt_f2 pt_pk_fma_lo(pt_f2 a, pt_f2 s, pt_f2 c) { pt_f2 r; asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(r) : "v"(a), "s"(s), "v"(c)); return r; }
PTK_DEV pt_f2 pt_pk_fma_hi(pt_f2 a, pt_f2 s, pt_f2 c) { pt_f2 r; asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "=v"(r) : "v"(a), "s"(s), "v"(c)); return r; }
PTK_DEV pt_f2 pt_pk_fnma_lo(pt_f2 a, pt_f2 s, pt_f2 c) { pt_f2 r; asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(r) : "v"(a), "s"(s), "v"(c)); return r; }
PTK_DEV pt_f2 pt_pk_fnma_hi(pt_f2 a, pt_f2 s, pt_f2 c) { pt_f2 r; asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(r) : "v"(a), "s"(s), "v"(c)); return r; }
// dhi + a.lo * s: the addend is the SGPR pair, the product's second factor too (one constant-bus
// operand only): so dhi is first copied to VGPRs by the first product instead -- see pt_quad3_pass1
struct PtRay3 { pt_f2 dxy, dzMx, Myz; };  // dir and M = (o - eye) x dir, as three register pairs

PTK_DEV void pt_quad3_pass1(pt_const_f32p t, const PtRay3& r, pt_f2& un, pt_f2& T)
{
    typedef const __attribute__((address_space(4))) pt_f2* pt_const_f2p;
    pt_const_f2p s = (pt_const_f2p)t;  // nx ny nz e2x e2y e2z Kx Ky Kz dhi
    pt_f2 dhi_v;
    { const pt_f2 dhi = s[9]; asm("v_pk_mul_f32 %0, %1, 1.0 op_sel_hi:[1,0]" : "=v"(dhi_v) : "s"(dhi)); }
    T = pt_pk_fma_lo(r.dxy, s[0], dhi_v);
    T = pt_pk_fma_hi(r.dxy, s[1], T);
    T = pt_pk_fma_lo(r.dzMx, s[2], T);
    un = pt_pk_mul_hi(r.dzMx, s[3]);
    un = pt_pk_fma_lo(r.Myz, s[4], un);
    un = pt_pk_fma_hi(r.Myz, s[5], un);
    un = pt_pk_fnma_lo(r.dxy, s[6], un);
    un = pt_pk_fnma_hi(r.dxy, s[7], un);
    un = pt_pk_fnma_lo(r.dzMx, s[8], un);
}

// QUADS: 0 = independent triangles (pt_tri_pass1), 3 = packed shared-u filter (pt_quad3_pass1)
// UNIT_DIR: the caller vouches for |d|^2 <= 1.001, the shared-u bound's assumption about the direction, and the filter does not test
// it.  Only pt_trace_body does: every direction a path of the trace kernels holds is the output of normalize3 / normalize3_unit
// (pt_generate_ray, the two exits of pt_shade_path) -- a correctly rounded quotient or product per component, |d|^2 within 1 +- 4e-7 --
// or that of pt_path_idle, and a parked or carried path brings those same bits back (pt_path_store / pt_path_load move dwords).  What
// normalising can make instead of a unit vector: the zero vector (|d|^2 = 0 passed the test anyway); a NaN component (a zero or NaN
// vector normalised), which makes un NaN for every quad -- it fails every comparison of the filter and is kept; an infinite component
// (a non-zero vector whose squared length underflows), with which the exact test's det is +-inf or NaN and its t = x * RN(1 / det) is
// +-0 or NaN for every triangle: the reference accepts no hit for such a ray, so nothing the filter drops is missed.  Rays that
// callers supply or kernels derive (queries, AO, the lit renderers, the LBVH kernels' big-triangle table) keep the test.  The origin's
// half of `tame` is tested everywhere.
template <bool DET_BOUNDED, int LDS_TABLE, int QUADS, bool UNIT_DIR = false>
PTK_DEV unsigned pt_intersect_two_pass(pt_const_f32p T, const PtPrepTriangle* tris, int ntri, const f3& o, const f3& d,
                                       bool alive, float& tmax, float& hu, float& hv, int& hidx,
                                       float delta1, float ray_radius, pt_const_f32p p1tab, float p1_lo, float p1_hi, const f3& anchor,
                                       PtTail tl, unsigned lane,
                                       unsigned long long* vstat = nullptr, unsigned long long* p1_ticks = nullptr)
{
    tl.wr = tl.rd = 0u;
    tl.kbest = ~0ull;
#if PT_STAMPS
    unsigned long long ta = 0, tb = 0;
#endif
    (void)vstat; (void)p1_ticks; (void)ray_radius; (void)p1tab; (void)p1_lo; (void)p1_hi; (void)anchor;
    unsigned steps = 0;  // pass-2 iterations of this wave (diagnostics only)
    // the assumptions of the shared-u error bound (derivation above pt_quad3_pass1), checked for THIS ray; the anchor is the
    // render's eye, the point the packed table's K was taken about (a primary ray starts exactly there: M = 0)
    bool tame = true;
    PtRay3 r3v;
    if (QUADS == 3 && DET_BOUNDED) {
        const f3 oc = mk3(o.x - anchor.x, o.y - anchor.y, o.z - anchor.z);
        const f3 M = cross3(oc, d);
        r3v.dxy = pt_f2{ d.x, d.y }; r3v.dzMx = pt_f2{ d.z, M.x }; r3v.Myz = pt_f2{ M.y, M.z };
    }
    if (QUADS == 3 && DET_BOUNDED) {
        if (UNIT_DIR) {
            tame = (__builtin_fabsf(o.x - anchor.x) <= ray_radius) & (__builtin_fabsf(o.y - anchor.y) <= ray_radius) &
                   (__builtin_fabsf(o.z - anchor.z) <= ray_radius);
        } else {
            float dd = pt_fma(d.z, d.z, pt_fma(d.y, d.y, d.x * d.x));
            tame = (dd <= 1.001f) & (__builtin_fabsf(o.x - anchor.x) <= ray_radius) &
                   (__builtin_fabsf(o.y - anchor.y) <= ray_radius) & (__builtin_fabsf(o.z - anchor.z) <= ray_radius);
        }
    }
    for (int base = 0; base < ntri; base += 32) {
        const int n = ntri - base < 32 ? ntri - base : 32;
        unsigned m = 0u;  // bit n-1-j <-> triangle base + j (pt_push_flag)
        PT_STAMP(ta);
        if (QUADS == 3 && DET_BOUNDED) {
            pt_const_f32p tp = p1tab + PT_P1_STRIDE * (base >> 2);  // base is a multiple of 32: 4 triangles per quad pair
            for (int j = 0; j < n; j += 4, tp += PT_P1_STRIDE) {
                pt_f2 un, th;
                pt_quad3_pass1(tp, r3v, un, th);
                {
                    const pt_lanes in = PT_LANES(!(__builtin_fabsf(un.x) > th.x));
                    m = pt_push_flag(pt_push_flag(m, in & PT_LANES(!(un.x < p1_lo))), in & PT_LANES(!(un.x > p1_hi)));
                }
                if (j + 2 < n) {
                    const pt_lanes in = PT_LANES(!(__builtin_fabsf(un.y) > th.y));
                    m = pt_push_flag(pt_push_flag(m, in & PT_LANES(!(un.y < p1_lo))), in & PT_LANES(!(un.y > p1_hi)));
                }
            }
            if (!tame) m = n == 32 ? ~0u : (1u << n) - 1u;
        } else {
            PtTriRec a = pt_load_tri(T, base);
            int j = 0;
            for (; j + 1 < n; j += 2) {
                PtTriRec b = pt_load_tri(T, base + j + 1);
                m = pt_push_flag(m, pt_tri_pass1<DET_BOUNDED>(a, o, d));
                a = pt_load_tri(T, base + (j + 2 < n ? j + 2 : j + 1));
                m = pt_push_flag(m, pt_tri_pass1<DET_BOUNDED>(b, o, d));
            }
            if (j < n) m = pt_push_flag(m, pt_tri_pass1<DET_BOUNDED>(a, o, d));
        }
#if PT_VALIDATE_FILTER
        // DIAGNOSTIC build (tools/validate_filter.py): the reference predicate of :100 and :109,
        // evaluated literally with IEEE division, must never accept a pair the filter dropped
        if (alive && vstat) {
            unsigned mx = 0u;
            for (int jj = 0; jj < n; ++jj) {
                const PtTriRec r = pt_load_tri(T, base + jj);
                float pvx = pt_fma(d.y, r.e2z, -(d.z * r.e2y));
                float pvy = pt_fma(d.z, r.e2x, -(d.x * r.e2z));
                float pvz = pt_fma(d.x, r.e2y, -(d.y * r.e2x));
                float det = pt_fma(r.e1z, pvz, pt_fma(r.e1y, pvy, r.e1x * pvx));
                bool keep = !(det < 1e-8f || -det > 1e-8f);
                float inv_det = 1.0f / det;
                float tvx = o.x - r.p1x, tvy = o.y - r.p1y, tvz = o.z - r.p1z;
                float u = pt_fma(tvz, pvz, pt_fma(tvy, pvy, tvx * pvx)) * inv_det;
                keep = keep && !(u < 0.0f || u > 1.0f);
                mx |= (keep ? 1u : 0u) << (n - 1 - jj);
            }
            atomicAdd(&vstat[0], (unsigned long long)n);                 // pairs examined
            atomicAdd(&vstat[1], (unsigned long long)__popc(mx));        // pairs the reference keeps
            atomicAdd(&vstat[2], (unsigned long long)__popc(m));         // pairs the filter keeps
            atomicAdd(&vstat[3], (unsigned long long)__popc(mx & ~m));   // VIOLATIONS: must stay 0
            if (QUADS == 3 && DET_BOUNDED && tame) {
                // how far mode 3's own roundings are from the reference's floats, relative to the slack
                // budgeted for that: |un_here - un_ref| / deltaP and |det_here c - det_ref c| / deltaD
                float r1 = 0.0f, r3 = 0.0f;
                {
                    const float deltaP = -p1_lo, deltaD = deltaP * (128.0f / 192.0f);
                    for (int jj = 0; jj + 1 < n; jj += 4) {
                        pt_f2 unp, thp;
                        pt_const_f32p tq = p1tab + PT_P1_STRIDE * ((base + jj) >> 2);
                        pt_quad3_pass1(tq, r3v, unp, thp);
                        for (int h = 0; h < 2 && jj + 2 * h + 1 < n; ++h) {
                            const PtTriRec a = pt_load_tri(T, base + jj + 2 * h);
                            float pvx = pt_fma(d.y, a.e2z, -(d.z * a.e2y)), pvy = pt_fma(d.z, a.e2x, -(d.x * a.e2z)), pvz = pt_fma(d.x, a.e2y, -(d.y * a.e2x));
                            float detA = pt_fma(a.e1z, pvz, pt_fma(a.e1y, pvy, a.e1x * pvx));
                            float unA = pt_fma(o.z - a.p1z, pvz, pt_fma(o.y - a.p1y, pvy, (o.x - a.p1x) * pvx));
                            const float dhi = tq[18 + h];
                            const float q1 = __builtin_fabsf((h ? unp.y : unp.x) - unA) / deltaP;
                            const float q3 = __builtin_fabsf(((h ? thp.y : thp.x) - dhi) - detA * 1.000002f) / deltaD;
                            r1 = q1 > r1 ? q1 : r1;
                            r3 = q3 > r3 ? q3 : r3;
                        }
                    }
                }
                atomicMax(&vstat[4], (unsigned long long)__float_as_uint(r1));
                atomicMax(&vstat[5], (unsigned long long)__float_as_uint(r3));
            }
        }
#endif
        if (!alive) m = 0u;  // a dead lane's stale ray must not cost pass-2 iterations
#if PT_STAMPS
        PT_STAMP(tb);
        if (p1_ticks) *p1_ticks += tb - ta;
#endif
        pt_pass2_chunk<DET_BOUNDED, LDS_TABLE>(m, base, n, tris, o, d, tmax, hu, hv, hidx, tl, lane, steps);
    }
    pt_pass2_finish<DET_BOUNDED, LDS_TABLE>(tris, o, d, tmax, hu, hv, hidx, tl, lane, steps);
    return steps;
}

// ---- the masked search's pending pairs: ONE survivor set per search, its list built with HELPER LANES ------------------------------
// A masked search of 33 .. 64 triangles used to run pt_pass2_chunk per mask word: two headers, two own walks, two append loops.  And an
// append loop moves one pair per lane and iteration, so it runs as long as the wave's slowest lane has survivors (8.3 of them, above) --
// its last iterations under an exec mask of a lane or two -- while the lanes whose own walk is over, more than half of the wave by
// then (PT_TAIL_LANES), idle.  Here the own steps walk the low word alone, as before, and what is left of it and the whole high word
// are appended ONCE, by twice the lanes:
//   * the k-th lane that still holds survivors (its rank: mbcnt of the ballot) sends its number to lane k, and the lanes that hold
//     none send theirs behind those -- a whole permutation, one ds_permute, every lane receives once, no LDS memory and no barrier;
//   * lanes 2k and 2k+1 fetch that owner's number and its two words (three ds_bpermute) and adopt one half of its survivors each:
//     the bits at odd positions of the low word with those at even positions of the high word, or the other way round.  The two
//     triangles of a quad are neighbours, so are their bits, and the halves come out even; both words fold into ONE 32-bit set whose bit
//     position still tells the word -- the loop's body is the 32-bit one plus the word's offset;
//   * more than 32 owners (PT_TAIL_LANES above 32 only) take a second turn of the same code.
// A pair is still (triangle << 6 | the RAY's lane), whoever appended it: pt_tail_round and pt_pass2_finish are the two-pass search's own.
// Every pair is listed exactly once (pt_pair_check_kernel, tests/test_gpu_pair_list.py); the search's winner is argmin (t, index)
// whatever the order the pairs are tested in -- the own walk keeps ascending order and its strict t < tmax, the merge compares (t, index).
// lo: bit nlo-1-j <-> triangle j (nlo = min(ntri, 32)); hi: bit ntri-33-j <-> triangle 32+j; both 0 in a lane without a ray.
// round(cnt): test the first cnt pending pairs (every lane calls it).  Returns the iterations of the loop (diagnostics).
#ifndef PT_PAIR_LIST
#define PT_PAIR_LIST 2  // the masked search's list: 0 = a chunk per word (the two-pass search's code), 1 = one survivor set, 2 = and helper lanes
#endif
#ifndef PT_PAIR_TAIL_LANES
// the masked search's own steps continue while more lanes than this hold a survivor of the low word.  Fewer than the two-pass search's 32:
// a pair listed by helper lanes costs less than it did, so more of them go to the rounds, which run full, and fewer own steps run half
// empty.  24.42 ms per step at 24 against 24.60 at 32, 24.50 at 28, 24.44 at 20 and 25.22 at 40 (profiles/pair_list/bench_ab.txt).
#define PT_PAIR_TAIL_LANES (PT_TAIL_LANES < 24 ? PT_TAIL_LANES : 24)
#endif
template <int LDS_TABLE, class ROUND>
PTK_DEV unsigned pt_pair_list_build(unsigned lo, unsigned hi, int ntri, PtTail& tl, unsigned lane, ROUND&& round)
{
    const bool mine = (lo | hi) != 0u;
    const pt_lanes owners = PT_LANES(mine);
    if (owners == 0ull) return 0u;
    const int off_lo = (ntri < 32 ? ntri : 32) - 32, off_hi = ntri - 32;   // triangle = leading zeros + the word's offset
    unsigned iters = 0u;
    if (PT_PAIR_LIST < 2) {
        // every lane appends its own survivors in ONE loop: the low word's while it has any, then the high word's
        for (pt_lanes has = owners; has != 0ull; has = PT_LANES((lo | hi) != 0u)) {
            ++iters;
            if ((lo | hi) != 0u) {
                const bool low = lo != 0u;
                unsigned m = low ? lo : hi, lz;
                asm("v_ffbh_u32_e32 %0, %1" : "=v"(lz) : "v"(m));
                m &= ~(0x80000000u >> (lz & 31u));
                lo = low ? m : lo;
                hi = low ? hi : m;
                pt_tail_put<LDS_TABLE>(tl, (tl.wr + pt_mbcnt(has)) & (PT_TAIL_LIST - 1u), ((unsigned)((low ? off_lo : off_hi) + (int)lz) << 6) | lane);
            }
            tl.wr += (unsigned)__popcll(has);
            if (tl.wr - tl.rd >= 64u) round(64u);
        }
        return iters;
    }
    const unsigned n_owners = (unsigned)__popcll(owners);
    const unsigned rank = pt_mbcnt(owners);
    const unsigned dest = mine ? rank : n_owners + lane - rank;   // (lane - rank: the lanes below this one that hold nothing)
    const unsigned owner_at = (unsigned)__builtin_amdgcn_ds_permute((int)(dest << 2), (int)lane);   // lane k: the k-th owner's number
    const unsigned own_bits = (lane & 1u) ? 0x55555555u : 0xAAAAAAAAu;   // this lane's half of a low word; of a high word the other bits
    const unsigned pair_lo = (unsigned)off_lo << 6, pair_hi = (unsigned)(off_hi - off_lo) << 6;   // (off_lo <= 0 wraps; lz + off_lo >= 0 for every set bit)
    for (unsigned first = 0u; first < n_owners; first += 32u) {
        const unsigned k = first + (lane >> 1);
        const unsigned ray = (unsigned)__builtin_amdgcn_ds_bpermute((int)(k << 2), (int)owner_at);
        const unsigned wlo = (unsigned)__builtin_amdgcn_ds_bpermute((int)(ray << 2), (int)lo);
        const unsigned whi = (unsigned)__builtin_amdgcn_ds_bpermute((int)(ray << 2), (int)hi);
        unsigned m = k < n_owners ? (wlo & own_bits) | (whi & ~own_bits) : 0u;
        for (pt_lanes has = PT_LANES(m != 0u); has != 0ull; has = PT_LANES(m != 0u)) {
            ++iters;
            if (m != 0u) {
                unsigned lz;
                asm("v_ffbh_u32_e32 %0, %1" : "=v"(lz) : "v"(m));
                m &= ~(0x80000000u >> (lz & 31u));
                // bit 31 - lz is of the low word where own_bits has it: lanes 2k at odd positions (lz even), lanes 2k+1 at even ones
                // (the word's offset, times 64, as ONE multiply-add on a wave-uniform operand: left to the compiler it is a select between two
                // copies of scalars, five instructions more)
                const unsigned high = (lz ^ lane) & 1u;
                unsigned pair;
                asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(pair) : "v"(high), "s"(pair_hi), "v"((lz << 6) | ray));
                pair += pair_lo;
                pt_tail_put<LDS_TABLE>(tl, (tl.wr + pt_mbcnt(has)) & (PT_TAIL_LIST - 1u), pair);
            }
            tl.wr += (unsigned)__popcll(has);
            if (tl.wr - tl.rd >= 64u) round(64u);
        }
    }
    return iters;
}

// closest hit of rays that bring their candidate masks along -- a FRESH wave of primary rays whose pixels have them
// (pt_primary_mask_kernel), or secondary rays whose cells have them (pt_secondary_mask_kernel; an uncovered ray brings all ones):
// pass 1 is skipped.  ntri <= 64 (two mask words).  Beside the LDS table (LDS_TABLE 1) the two words are ONE survivor set
// (pt_pair_list_build, above); elsewhere pass 2 is the one of pt_intersect_two_pass, chunk by chunk.
#if PT_VALIDATE_FILTER
// DIAGNOSTIC build (tools/validate_filter.py): one mask word m of the n triangles from base against the reference's test
PTK_DEV void pt_validate_mask_word(pt_const_f32p T, int base, int n, unsigned m, const f3& o, const f3& d, bool alive, unsigned long long* vstat)
{
    if (alive && vstat) {  // the reference's whole test (:96-125, against the initial tmax of :141) must never accept a pair the mask dropped
        unsigned mx = 0u;
        for (int jj = 0; jj < n; ++jj) {
            const PtTriRec r = pt_load_tri(T, base + jj);
            float pvx = pt_fma(d.y, r.e2z, -(d.z * r.e2y));
            float pvy = pt_fma(d.z, r.e2x, -(d.x * r.e2z));
            float pvz = pt_fma(d.x, r.e2y, -(d.y * r.e2x));
            float det = pt_fma(r.e1z, pvz, pt_fma(r.e1y, pvy, r.e1x * pvx));
            bool keep = !(det < 1e-8f || -det > 1e-8f);
            float inv_det = 1.0f / det;
            float tvx = o.x - r.p1x, tvy = o.y - r.p1y, tvz = o.z - r.p1z;
            float u = pt_fma(tvz, pvz, pt_fma(tvy, pvy, tvx * pvx)) * inv_det;
            keep = keep && !(u < 0.0f || u > 1.0f);
            float qvx = pt_fma(tvy, r.e1z, -(tvz * r.e1y));
            float qvy = pt_fma(tvz, r.e1x, -(tvx * r.e1z));
            float qvz = pt_fma(tvx, r.e1y, -(tvy * r.e1x));
            float v = pt_fma(d.z, qvz, pt_fma(d.y, qvy, d.x * qvx)) * inv_det;
            keep = keep && !(v < 0.0f || u + v > 1.0f);
            float tt = pt_fma(r.e2z, qvz, pt_fma(r.e2y, qvy, r.e2x * qvx)) * inv_det;
            keep = keep && (tt > 0.0f && tt < 1e20f);
            mx |= (keep ? 1u : 0u) << (n - 1 - jj);
        }
        atomicAdd(&vstat[0], (unsigned long long)n);
        atomicAdd(&vstat[1], (unsigned long long)__popc(mx));
        atomicAdd(&vstat[2], (unsigned long long)__popc(m));
        atomicAdd(&vstat[3], (unsigned long long)__popc(mx & ~m));   // VIOLATIONS: must stay 0
    }
}
#endif

template <bool DET_BOUNDED, int LDS_TABLE>
PTK_DEV unsigned pt_intersect_masked(pt_const_f32p T, const PtPrepTriangle* tris, int ntri, const f3& o, const f3& d, bool alive,
                                      float& tmax, float& hu, float& hv, int& hidx, uint2 pm, PtTail tl, unsigned lane,
                                      unsigned long long* vstat = nullptr, PtStampSplit* sp = nullptr)
{
    (void)T; (void)vstat; (void)sp;
    tl.wr = tl.rd = 0u;
    tl.kbest = ~0ull;
    unsigned steps = 0;
#if PT_STAMPS
    if (sp) sp->searches++;
#endif
    if (LDS_TABLE == 1 && PT_PAIR_LIST > 0 && PT_PAIR_TAIL_LANES > 0) {
        // one survivor set (pt_pair_list_build): own steps over the low word while more than PT_PAIR_TAIL_LANES lanes hold a survivor of
        // it -- the loop of pt_pass2_chunk -- then ONE list of what is left of it and of the high word
        const int n = ntri < 32 ? ntri : 32;
        unsigned m = pm.x, mh = ntri > 32 ? pm.y : 0u;
#if PT_VALIDATE_FILTER
        pt_validate_mask_word(T, 0, n, m, o, d, alive, vstat);
        if (ntri > 32) pt_validate_mask_word(T, 32, ntri - 32, mh, o, d, alive, vstat);
#endif
        if (!alive) m = mh = 0u;
#if PT_STAMPS
        unsigned long long s0 = 0, s1 = 0, s2 = 0, rsum = 0;
        PT_STAMP(s0);
#endif
        for (pt_lanes more = PT_LANES(m != 0u); (unsigned)__popcll(more) > (unsigned)PT_PAIR_TAIL_LANES; more = PT_LANES(m != 0u)) {
            ++steps;
            const bool valid = m != 0u;
            unsigned lz;  // (-1 for m = 0: a wild index into the LDS table, whose out-of-range reads return 0; the result is discarded)
            asm("v_ffbh_u32_e32 %0, %1" : "=v"(lz) : "v"(m));
            const int i = n - 32 + (int)lz;
            m &= ~(0x80000000u >> (lz & 31u));
            const PtTriRec r = pt_fetch_rec<1>(tris, i);
            pt_tri_pass2<DET_BOUNDED>(r, i, valid, o, d, tmax, hu, hv, hidx);
        }
        PT_STAMP(s1);
        const unsigned iters = pt_pair_list_build<LDS_TABLE>(m, mh, ntri, tl, lane, [&](unsigned cnt) {
#if PT_STAMPS
            unsigned long long ra = 0, rb = 0;
            PT_STAMP(ra);
#endif
            ++steps;
            pt_tail_round<DET_BOUNDED, LDS_TABLE>(tl, cnt, lane, tris, o, d);
#if PT_STAMPS
            PT_STAMP(rb);
            rsum += rb - ra;
#endif
        });
        (void)iters;
#if PT_STAMPS
        PT_STAMP(s2);
        if (sp) { sp->own += s1 - s0; sp->append += (s2 - s1) - rsum; sp->rounds += rsum; sp->iters += iters; }
#endif
    } else {
        for (int base = 0; base < ntri; base += 32) {
            const int n = ntri - base < 32 ? ntri - base : 32;
            unsigned m = base == 0 ? pm.x : pm.y;
#if PT_VALIDATE_FILTER
            pt_validate_mask_word(T, base, n, m, o, d, alive, vstat);
#endif
            if (!alive) m = 0u;
            pt_pass2_chunk<DET_BOUNDED, LDS_TABLE>(m, base, n, tris, o, d, tmax, hu, hv, hidx, tl, lane, steps, sp);
        }
    }
    pt_pass2_finish<DET_BOUNDED, LDS_TABLE>(tris, o, d, tmax, hu, hv, hidx, tl, lane, steps, sp);
    return steps;
}

// ------------------------------------------------------------------------------------------
// trace kernels
// ------------------------------------------------------------------------------------------

// one path: 16 dwords (what a lane holds, and what the per-wave pool parks: pt_pool_push / pt_pool_pop)
struct PtPath {
    f3 o, d;        // current ray (:257)
    f3 mask, L;     // throughput and radiance (:225-226)
    uint32_t seed;  // RNG state (:308)
    int bounce;     // loop index i of traceRays (:229)
    unsigned ro;    // where the path's radiance goes, fixed from the sample's first ray to its last (pt_ring_offset): the byte offset of its record
                    // from the ring's base -- or, when the ring is above 4 GiB (PtTraceParams::rad1_off == 0), its local pixel index
    unsigned fl;    // frame counted from the render's first (the stop test of a checkpointed launch, the long form's ring slot)
};

// The record of (local pixel lp, frame `frame` of the render) in the staging ring, as a byte offset from PtTraceParams::rad: entry
// (frame + phase) % 2S of the ring, the first S entries in slot 0, the others in slot 1, rad1_off bytes further.  Every input is fixed for
// the render -- a carried path never leaves its render -- so this runs ONCE per sample, at full lane width with `frame` wave-uniform
// (scalar work but for one multiply-add per lane), and not under the few-lane exec mask of every wave-bounce's store block.  Only the
// short form (rad1_off != 0): the host chooses it when 2 x slot bytes <= 2^32, so slot * rad1_off + (entry * npix + lp) * 12 + 12 <=
// 2^32 and nothing wraps.  (Read from the kernarg segment whichever the kernel, as the store's base is: no SGPR is held for it.)
PTK_DEV unsigned pt_ring_offset(unsigned lp, unsigned frame)
{
    const pt_kargs_p KR = pt_kargs();
    const unsigned fr = frame + KR->ring_phase, S = KR->slot_frames;
    const unsigned r = fr - __umulhi(fr, KR->ring_magic) * (2u * S);
    const bool upper = r >= S;
    return (upper ? KR->rad1_off : 0u) + ((upper ? r - S : r) * KR->npix_local + lp) * 12u;
}


// ---- shade one bounce of a live path (:229-258); on path end store its radiance --------------------
// Three parts, which the LBVH kernel runs as one (pt_shade_path below) and the table kernels where their loop has them (pt_trace_body):
// the miss, the hit, and the store of a finished path's radiance.

// the ray hit nothing: the background, and the path is over (:235)
PTK_DEV void pt_shade_miss(PtPath& s)
{
    const float bg = pt_max(0.45f, 0.0f);
    s.L = add3(s.L, scale3(s.mask, bg));  // :235
}

// The ray (origin no longer needed, s.d) hit triangle hidx at p = o + d t, barycentrics (hu, hv).  Returns true when the path has
// finished (pdf <= 0, depth); otherwise s.o / s.d are its next ray.  s.o is read only through p.
template <bool DET_BOUNDED, bool LATE>
PTK_DEV bool pt_shade_hit(const PtTraceParams& P, PtPath& s, const f3 p, float hu, float hv, int hidx)
{
    const pt_kargs_p K = pt_kargs();  // tris, mats, nmat, max_bounces: read here, not kept in SGPRs
    bool finished = false;
    {
        // The direction sample's angle first: here only the path state is live.  (pt_sincos takes its binary32 branch on every
        // angle this path forms, phi in [0, 2 pi]; its binary64 branch is dead at run time.)  Both BRDFs draw phi first, then the
        // second uniform (:163-164, :182-183).
        float phi = PTK_TWO_PI * pt_random_float(s.seed);
        float xi = pt_random_float(s.seed);
        float sp, cp;
        __builtin_amdgcn_sched_barrier(0);
        pt_sincos(phi, sp, cp);
        __builtin_amdgcn_sched_barrier(0);

        // deferred HitRecord of the closest hit (:127-130): same values as writing it at every
        // acceptance, only the last one is read.
        // (both gathers: a 32-bit per-lane byte offset against the wave-uniform base -- global_load v, v_off, s[base:base+1] -- instead of a
        // 64-bit per-lane address; ntri * 64 and nmat * 64 are below 2^32, pt_shim.hip: render_internal)
        const float4 nid = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(PT_ARG(tris)) + (size_t)((unsigned)hidx * 64u) + 48);
        const f3 N = mk3(nid.x, nid.y, nid.z);
        // never fault on a corrupt id: clamped to [0, nmat - 1] (the upper end is scalar work; max, then min: no branch)
        const int nm1 = PT_ARG(nmat) - 1;
        int mid = __float_as_int(nid.w);
        mid = mid < 0 ? 0 : mid;
        mid = mid > nm1 ? nm1 : mid;
        float w = 1.0f - hu - hv;
        f3 n = normalize3(add3(add3(scale3(N, hu), scale3(N, hv)), scale3(N, w)));

        const PtRawMaterial* mat = reinterpret_cast<const PtRawMaterial*>(reinterpret_cast<const char*>(PT_ARG(mats)) + (size_t)((unsigned)mid * 64u));  // :239
        const float4 alb = *reinterpret_cast<const float4*>(mat->albedo);
        const float4 emi = *reinterpret_cast<const float4*>(mat->emissive);
        const float rough = mat->roughness;
        const int type = mat->type;

        s.L.x = s.L.x + s.mask.x * emi.x * 3.0f;  // :241
        s.L.y = s.L.y + s.mask.y * emi.y * 3.0f;
        s.L.z = s.L.z + s.mask.z * emi.z * 3.0f;

        n = dot3(n, s.d) < 0.0f ? n : scale3(n, -1.0f);  // :243
        f3 wo = neg3(s.d);

        // sampleHemisphereCosine (:161-172) and sampleGGX (:180-192) share everything
        // except (sinTheta, cosTheta)
        f3 axis = __builtin_fabsf(n.x) > 0.001f ? mk3(0.0f, 1.0f, 0.0f) : mk3(1.0f, 0.0f, 0.0f);
        f3 tv = normalize3(cross3(axis, n));
        f3 sv = cross3(n, tv);
        // one sqrt pair for both BRDFs (a wave usually holds both material types): only the
        // radicands differ -- diffuse: sqrt(xi), sqrt(1-xi); GGX: sqrt((1-xi)/(xi(r^2-1)+1)), then
        // sqrt(max(0, 1-cos^2))
        float cos_arg = 1.0f - xi;
#if PT_GGX_FAST
        // (the numerator needs no guard: xi = (float)s * 2^-32 is in [0, 1], so 1 - xi is +0 or in [2^-24, 1])
        if (type == 2) cos_arg = pt_div_by(cos_arg, xi * (rough * rough - 1.0f) + 1.0f);
#else
        if (type == 2) cos_arg = cos_arg / (xi * (rough * rough - 1.0f) + 1.0f);
#endif
        const float cosTheta = pt_sqrt(cos_arg);
        const float sin_arg = type == 2 ? pt_max(0.0f, 1.0f - cosTheta * cosTheta) : xi;
        const float sinTheta = pt_sqrt(sin_arg);
        f3 a = scale3(scale3(sv, cp), sinTheta);
        f3 b = scale3(scale3(tv, sp), sinTheta);
        f3 c = scale3(n, cosTheta);
        f3 sdir = normalize3_unit(add3(add3(a, b), c));

        f3 wi = sdir;
        f3 color = mk3(0.0f, 0.0f, 0.0f);
        float pdf = 0.0f;
        float dwin = 0.0f;
        if (type == 1) {  // DIFFUSE (:197-204)
            dwin = dot3(wi, n);
            pdf = dwin * PTK_INV_PI;
            color = mk3(alb.x * PTK_INV_PI, alb.y * PTK_INV_PI, alb.z * PTK_INV_PI);
        } else if (type == 2) {  // SPECULAR (:205-218)
            float k2 = 2.0f * dot3(wo, sdir);
            wi = add3(neg3(wo), scale3(sdir, k2));  // reflect(wo, wh) (:156-159)
            dwin = dot3(wi, n);
            float dwon = dot3(wo, n);
            if (!(dwin * dwon < 0.0f)) {
                float r2 = rough * rough;
                const float gd = cosTheta * cosTheta * (r2 - 1.0f) + 1.0f;
#if PT_GGX_FAST
                // gd * gd reaches r^4 (4.1e-9 for the Cornell box's 0.008): inside the window of the short quotients
                const float D = pt_div(r2 * PTK_INV_PI, gd * gd);  // pow(x, 2.0f) is x*x in PTSPEC (:177)
                // pdf = D * cosTheta / (4 dot(wo, sdir)) and g = D / (4 dwin dwon) behind one guard: D * cosTheta <= D, for
                // cosTheta <= 1 or D is NaN -- cos_arg = RN(a / b) with b = RN(1 + RN(xi c)) >= RN(1 - xi) = a for c = RN(r^2 - 1)
                // in [-1, 0] (rounding is monotonic) and b >= 1 for any other c; a NaN cosTheta makes gd and with it D NaN
                float g;
                pt_div_pair(D * cosTheta, 4.0f * dot3(wo, sdir), D, 4.0f * dwin * dwon, pdf, g);
#else
                float D = r2 * PTK_INV_PI / (gd * gd);  // pow(x, 2.0f) is x*x in PTSPEC (:177)
                pdf = D * cosTheta / (4.0f * dot3(wo, sdir));
                float g = D / (4.0f * dwin * dwon);
#endif
                color = mk3(alb.x * g * 2.0f, alb.y * g * 2.0f, alb.z * g * 2.0f);
            }
        }
        if (pdf <= 0.0f) {  // :251
            finished = true;
        } else {
            float qx = color.x * dwin, qy = color.y * dwin, qz = color.z * dwin;
            pt_div3(qx, qy, qz, pdf);   // the three IEEE quotients of :253-255
            s.mask.x = s.mask.x * qx;
            s.mask.y = s.mask.y * qy;
            s.mask.z = s.mask.z * qz;
            s.bounce++;
            if (s.bounce >= PT_ARG(max_bounces)) {
                finished = true;
            } else {
                s.o = add3(p, scale3(wi, 0.01f));  // :257
                s.d = normalize3_unit(wi);
            }
        }
    }
    return finished;
}

// the finished path's radiance goes to its record of the staging ring
PTK_DEV void pt_path_finish(const PtPath& s)
{
    {
        // :260; the w lane of the reference's float4 is overwritten with 1.0 by gammaCorrect (:293) and never read
        // before: three floats per sample are staged, not four (measured at the full 256 spp, profiles/r02/
        // pmc_r02_summary.txt: 35.2 bytes of HBM traffic per sample against 41.0 with aligned 16-byte records --
        // the L2 cannot hold every partly filled line of the ~900 000 paths in flight until it is complete, and a
        // partly written sector costs a read-modify-write either way; fewer bytes written, fewer sectors touched)
        // Some lane finishes in practically every wave-bounce (a wave retires ~10 of its 64 paths per bounce), so this block issues every
        // time, under an exec mask of a few lanes: the path brings its record's offset along (PtPath::ro, pt_ring_offset) and the block is
        // max(L, 0) and one store against the ring's base.  (The base and the form are read from the kernarg segment here whichever the
        // kernel -- scalar loads, wave-uniform branch -- and hold no SGPR through the loop.)
        const pt_kargs_p KR = pt_kargs();
        float* const rad = KR->rad;
        const unsigned rad1_off = KR->rad1_off;   // (both loads in flight together, one wait)
        // (records are 12 bytes apart: the vector type is declared with the 4-byte alignment the address really has)
        typedef float pt_f3v __attribute__((ext_vector_type(3), aligned(4)));
        pt_f3v v;
        v.x = pt_max(s.L.x, 0.0f);
        v.y = pt_max(s.L.y, 0.0f);
        v.z = pt_max(s.L.z, 0.0f);
        if (rad1_off != 0u) {
            // one 12-byte store (global_store_dwordx3 v_off, v[..], s[base:base+1]); the offset is UNSIGNED: the upper slot of a 4 GiB ring lies above 2^31
            *reinterpret_cast<pt_f3v*>(reinterpret_cast<char*>(rad) + (size_t)s.ro) = v;
        } else {
            // the long form (a ring above 4 GiB): s.ro is the local pixel; frame f of the render is entry (f + phase) % 2S of the ring, the
            // first S entries in one slot, the others in the other
            const unsigned fr = s.fl + KR->ring_phase, S = KR->slot_frames;
            const unsigned r = fr - __umulhi(fr, KR->ring_magic) * (2u * S);
            float* out = (r < S ? rad : KR->rad1) + ((size_t)(r < S ? r : r - S) * KR->npix_local + s.ro) * 3u;
            *reinterpret_cast<pt_f3v*>(out) = v;
        }
    }
}

// One bounce of a live path whose search returned (tmax, hu, hv, hidx).  Returns true when the path has finished (its radiance is
// stored, what is left in `s` is dead).
template <bool DET_BOUNDED, bool LATE>
PTK_DEV bool pt_shade_path(const PtTraceParams& P, PtPath& s, float tmax, float hu, float hv, int hidx)
{
    bool finished = false;
    if (hidx < 0) {
        pt_shade_miss(s);
        finished = true;
    } else {
        finished = pt_shade_hit<DET_BOUNDED, LATE>(P, s, add3(s.o, scale3(s.d, tmax)), hu, hv, hidx);
    }
    if (finished) pt_path_finish(s);
    return finished;
}

// the same with a per-lane flag that a finished path clears (the LBVH kernel's call site)
template <bool DET_BOUNDED, bool LATE>
PTK_DEV void pt_shade(const PtTraceParams& P, PtPath& s, bool& alive, float tmax, float hu, float hv, int hidx)
{
    if (pt_shade_path<DET_BOUNDED, LATE>(P, s, tmax, hu, hv, hidx)) alive = false;
}

// (n_rays, n_samples: wave-uniform tallies kept in SGPRs -- popcounts of the lanes that shaded / finished; as per-lane counters they
// were the two registers the 64-VGPR kernel spilled, and the reload in the store block waited for the radiance store itself)
PTK_DEV void pt_flush_counters(const PtTraceParams& P, unsigned lane, unsigned n_rays, unsigned n_samples)
{
    if (!P.stats) return;
    // wave reduction of the work counters, one atomic pair per wave
    const unsigned long long r = n_rays, s = n_samples;
    if (lane == 0) {
        atomicAdd(&P.stats[0], s);
        atomicAdd(&P.stats[1], r);
    }
}

// ---- how lanes get their paths: a per-wave pool of parked paths + FRESH phases --------------------
// Lane = path.  A wave retires ~10 of its 64 paths per bounce.  Round 1 handed every dead lane the next
// sample of the wave's range on the spot (camera rays pre-generated 64 wide into LDS), so each bounce
// mixed ~10 primary rays into 54 incoherent secondary ones and every sample's bounce 0 took a full-price
// slot of the incoherent main loop.  Now the wave keeps a POOL of up to 64 parked paths in LDS (64 B each):
//   * dead lanes take parked paths from the pool;
//   * when lanes are dead and the pool is empty, the wave PARKS all its live paths and starts 64 fresh
//     samples -- 64 consecutive pixels of its range -- in all 64 lanes at once: camera rays at full lane
//     width straight into registers, and a bounce 0 whose 64 rays share the origin and are coherent
//     (pass 2 walks ~the same 3-4 survivors in every lane instead of max-over-lanes 8; a wave usually sees
//     one material, so the untaken BRDF branch is skipped wave-wide).  The following bounces refill the
//     ~10 lanes that end per bounce from the pool, which lasts ~5 bounces -- until the next fresh phase.
// Which lane runs which sample, and in which order, never affects a sample's result.
//
// The pool holds SEARCHED paths.  Lanes die at the search far more often than in shading (an open scene: 9 of 10 samples end at a
// miss), so a pool of paths waiting for their search -- parked and resumed before it -- left every lane whose ray missed idle through
// the shading phase that followed.  With hit records in the pool such a lane finishes the moment the search returns, takes a parked
// path on the spot and shades it in the same iteration: shading runs with every lane the pool can fill (pt_trace_body).
//
// 68-byte records (pt_hit_store) and the 20 480 B a workgroup may have for 8 of them to fit a CU leave room for 56 per wave, not 64:
// a fresh phase parks every live path, so it starts only when at most PT_POOL lanes are alive, i.e. at least 8 are dead.  Until then
// the iteration goes on with its fewer than 8 idle lanes and asks again after the next search.
// PT_POOL, the parked-path slots per wave, is defined in pt_kernels.h: the checkpoint regions are sized by it (PT_CARRY_HIT_RECORDS).

struct PtWaveQueue {  // wave-uniform (SGPRs): the wave's current range [pix, end) of local pixels of `frame`
    unsigned pix, end, frame;   // frame: counted from the render's first frame (what a path keeps as `fl`)
    unsigned row, col;       // local row / column of `pix`, kept incrementally: no per-lane division
    unsigned sl, within;     // row = sl * stripe_rows + within (the stripe of the multi-GPU split)
    unsigned g;              // the shard of the queue the wave takes its batches from, or PT_Q_EMPTY (pt_queue_refill)
};

#define PT_Q_EMPTY 0xffffffffu   // PtWaveQueue::g once the wave has found every shard of the queue empty

// q.row / col / sl / within of q.pix: wave-uniform divisions, once per batch
template <bool LATE>
PTK_DEV void pt_queue_locate(const PtTraceParams& P, pt_kargs_p K, PtWaveQueue& q)
{
    q.row = q.pix / (unsigned)PT_ARG(width);
    q.col = q.pix - q.row * (unsigned)PT_ARG(width);
    q.sl = q.row / (unsigned)PT_ARG(stripe_rows);
    q.within = q.row - q.sl * (unsigned)PT_ARG(stripe_rows);
}

// Makes [q.pix, q.end) non-empty when the current batch is used up; false when there is nothing (more) to start in this launch.
// The batches of a launch's chunk (128 or 256 consecutive pixels of one frame, numbered frame-major) come off a SHARDED queue:
// PT_QUEUE_SHARDS counters, each on a cache line of its own; shard s deals the batches s, s + NS, s + 2 NS, ...  One counter for
// 8 192 waves is an L2 channel's atomic unit doing nothing else -- at 128 samples per batch a 16-frame launch is an atomic every
// 14 ns, about what the unit serves, and the waves of a launch start TOGETHER, so their grabs arrive in bursts (a wave waits for its
// turn: measured ~50 us per launch, profiles/r04/queue_shards.txt).  A wave stays with its shard (the wave's number mod NS at
// first) and moves on to the next when it is used up; a shard found empty is marked in the queue's STOP word (one bit per shard,
// on a line of its own), which every wave polls at its fresh phases anyway (pt_queue_next) and which spares the others the grab.
// All bits set = the launch has handed out its last batch.
template <bool LATE>
PTK_DEV bool pt_queue_refill(const PtTraceParams& P, unsigned lane, PtWaveQueue& q, unsigned empty_mask)
{
    const pt_kargs_p K = pt_kargs();
    if (q.pix != q.end) return true;
    if (q.g == PT_Q_EMPTY) return false;
    const unsigned total = PT_ARG(total_batches);
    unsigned sh = q.g, b = 0u;
    bool got = false;
    for (unsigned tries = 0u; tries < PT_QUEUE_SHARDS && total != 0u; ++tries, sh = (sh + 1u) & (PT_QUEUE_SHARDS - 1u)) {
        if ((empty_mask >> sh) & 1u) continue;
        unsigned k = 0u;
        if (lane == 0) k = atomicAdd(PT_ARG(batch_counter) + sh * PT_QUEUE_SHARD_WORDS, 1u);
        k = __builtin_amdgcn_readfirstlane(k);
        b = k * PT_QUEUE_SHARDS + sh;
        if (b < total) { got = true; break; }
        // (mark it, and see what the others have marked meanwhile: no grab at a shard known to be empty)
        unsigned seen = 0u;
        if (lane == 0u) seen = atomicOr(PT_ARG(batch_counter) + PT_QUEUE_STOP_WORD, 1u << sh);
        empty_mask |= (1u << sh) | (unsigned)__builtin_amdgcn_readfirstlane(seen);
    }
    if (!got) { q.g = PT_Q_EMPTY; return false; }
    q.g = sh;
    const unsigned f = b / PT_ARG(batches_per_frame);
    const unsigned bi = b - f * PT_ARG(batches_per_frame);
    q.frame = PT_ARG(chunk_f0) + f;
    q.pix = bi * PT_ARG(batch);
    const unsigned e = q.pix + PT_ARG(batch);
    q.end = e < PT_ARG(npix_local) ? e : PT_ARG(npix_local);
    pt_queue_locate<LATE>(P, K, q);
    return true;
}

// PtPathSlots says where a waiting path's record lives: float4 word j of record k at A[j fs + k], dword j at W[j ws + k wk] (float4
// arrays: conflict-free b128 accesses in LDS, lane k moving entry k coalesced in a carry region).
// The record of a path BEFORE its search (the LBVH kernel's checkpoint): 60 bytes, three float4 and three dwords --
//   [0] o.xyz d.x   [1] d.yz mask.xy   [2] mask.z L.xyz   [3] seed, ro, fl | bounce << 16     (ro: PtPath::ro, where its radiance goes)
// in three float4 arrays and three dword arrays of PT_CARRY_RECORDS entries.
struct PtPathSlots {
    float4* A;
    unsigned* W;
    unsigned fs, ws, wk;
    PTK_DEV float4& vec(unsigned j, unsigned k) const { return A[j * fs + k]; }
    PTK_DEV unsigned& word(unsigned j, unsigned k) const { return W[j * ws + wk * k]; }
};

PTK_DEV PtPathSlots pt_carry_slots(uint32_t* region) { return { (float4*)(region + 16), region + 16 + PT_CARRY_RECORDS * 12, PT_CARRY_RECORDS, PT_CARRY_RECORDS, 1u }; }

// The table kernels park SEARCHED paths (pt_trace_body): the record keeps the hit, not the ray's origin and t --
//   [0] p.xyz d.x   [1] d.yz mask.xy   [2] mask.z L.xyz   [3] seed, ro, hu, hv     (p = o + d t: all that shading reads of o)
// and NW dwords: fl | bounce << 16 | triangle << 24 beside the LDS table (NW 1: a triangle below PT_LDS_TRI_MAX and a bounce count below
// PT_PACKED_BOUNCE_MAX fit 8 bits each, 68 bytes a record), fl | bounce << 16 and the triangle otherwise (NW 2).  The pool keeps four
// float4 arrays of PT_POOL entries and one array of NW dwords per record, a carry region four float4 arrays and two dword arrays of
// PT_CARRY_HIT_RECORDS = PT_POOL entries (PT_CARRY_HIT_STRIDE_DW: one stride for both forms).
static_assert(PT_LDS_TRI_MAX <= 256 && PT_PACKED_BOUNCE_MAX <= 256, "triangle and bounce count of a parked path: 8 bits each of the packed word");
template <int LDS_TABLE> __host__ __device__ constexpr unsigned pt_hit_words() { return LDS_TABLE == 1 ? 1u : 2u; }
template <int LDS_TABLE> __host__ __device__ constexpr unsigned pt_pool_dwords() { return PT_POOL * (16u + pt_hit_words<LDS_TABLE>()); }
// the waves' pools follow one another, and each begins with its float4 arrays: a pool is whole float4s (56 records are, 57 of 17 dwords
// are not), or the next wave's b128 accesses are misaligned; and a stopping wave's pool goes to its region record by record
static_assert(pt_pool_dwords<1>() % 4u == 0u && pt_pool_dwords<2>() % 4u == 0u, "a wave's pool must be a whole number of float4: the next pool's 16-byte alignment");
static_assert(PT_POOL <= PT_CARRY_HIT_RECORDS, "a checkpoint region holds a whole pool");
template <unsigned NW> PTK_DEV PtPathSlots pt_pool_slots(float4* pool) { return { pool, reinterpret_cast<unsigned*>(pool + 4 * PT_POOL), PT_POOL, 1u, NW }; }
PTK_DEV PtPathSlots pt_carry_hit_slots(uint32_t* region) { return { (float4*)(region + 16), region + 16 + PT_CARRY_HIT_RECORDS * 16, PT_CARRY_HIT_RECORDS, PT_CARRY_HIT_RECORDS, 1u }; }

// what a lane of a table kernel holds between the search and shading: the path (s.o is the hit point) and the hit
struct PtHit {
    float hu, hv;
    int hidx;
};

template <unsigned NW>
PTK_DEV void pt_hit_store(const PtPathSlots& S, unsigned k, const PtPath& s, const PtHit& h)
{
    S.vec(0, k) = make_float4(s.o.x, s.o.y, s.o.z, s.d.x);
    S.vec(1, k) = make_float4(s.d.y, s.d.z, s.mask.x, s.mask.y);
    S.vec(2, k) = make_float4(s.mask.z, s.L.x, s.L.y, s.L.z);
    S.vec(3, k) = make_float4(__uint_as_float(s.seed), __uint_as_float(s.ro), h.hu, h.hv);
    const unsigned w = s.fl | ((unsigned)s.bounce << 16);  // fl below 65 536 (pt_render_frames checks: the ring has fewer frames); a parked path hit: hidx >= 0
    if (NW == 1u) {
        S.word(0, k) = w | ((unsigned)h.hidx << 24);       // bounce < max_bounces <= PT_PACKED_BOUNCE_MAX (render_part checks), hidx < PT_LDS_TRI_MAX
    } else {
        S.word(0, k) = w;                                  // bounce < max_bounces <= 65 535 (pt_render_frames checks)
        S.word(1, k) = (unsigned)h.hidx;
    }
}

template <unsigned NW>
PTK_DEV void pt_hit_load(const PtPathSlots& S, unsigned k, PtPath& s, PtHit& h)
{
    const float4 a0 = S.vec(0, k), a1 = S.vec(1, k), a2 = S.vec(2, k), a3 = S.vec(3, k);
    const unsigned w = S.word(0, k);
    s.o = mk3(a0.x, a0.y, a0.z);
    s.d = mk3(a0.w, a1.x, a1.y);
    s.mask = mk3(a1.z, a1.w, a2.x);
    s.L = mk3(a2.y, a2.z, a2.w);
    s.seed = __float_as_uint(a3.x);
    s.ro = __float_as_uint(a3.y);
    h.hu = a3.z;
    h.hv = a3.w;
    s.fl = w & 0xffffu;
    if (NW == 1u) {
        s.bounce = (int)((w >> 16) & 0xffu);
        h.hidx = (int)(w >> 24);
    } else {
        s.bounce = (int)(w >> 16);
        h.hidx = (int)S.word(1, k);
    }
}

PTK_DEV void pt_path_store(const PtPathSlots& S, unsigned k, const PtPath& s)
{
    S.vec(0, k) = make_float4(s.o.x, s.o.y, s.o.z, s.d.x);
    S.vec(1, k) = make_float4(s.d.y, s.d.z, s.mask.x, s.mask.y);
    S.vec(2, k) = make_float4(s.mask.z, s.L.x, s.L.y, s.L.z);
    S.word(0, k) = s.seed;
    S.word(1, k) = s.ro;
    S.word(2, k) = s.fl | ((unsigned)s.bounce << 16);  // both below 65 536 (pt_render_frames checks: the ring has fewer frames)
}

PTK_DEV void pt_path_load(const PtPathSlots& S, unsigned k, PtPath& s)
{
    const float4 a0 = S.vec(0, k), a1 = S.vec(1, k), a2 = S.vec(2, k);
    const unsigned w2 = S.word(2, k);
    s.o = mk3(a0.x, a0.y, a0.z);
    s.d = mk3(a0.w, a1.x, a1.y);
    s.mask = mk3(a1.z, a1.w, a2.x);
    s.L = mk3(a2.y, a2.z, a2.w);
    s.seed = S.word(0, k);
    s.ro = S.word(1, k);
    s.fl = w2 & 0xffffu;
    s.bounce = (int)(w2 >> 16);
}

// (alive: the wave's live lanes as a lane mask, here and in pt_pool_pop / pt_start_fresh -- see pt_trace_body)
template <unsigned NW>
PTK_DEV void pt_pool_push(float4* pool, unsigned& pool_n, const PtPath& s, const PtHit& h, pt_lanes& alive)
{
    const pt_lanes live = alive;
    if (PT_ON(live)) {
        const unsigned k = pool_n + pt_mbcnt(live);   // (below PT_POOL: the caller parks into an empty pool at most PT_POOL live paths)
        pt_hit_store<NW>(pt_pool_slots<NW>(pool), k, s, h);
    }
    pool_n += (unsigned)__popcll(live);
    alive = 0ull;
}

template <unsigned NW>
PTK_DEV void pt_pool_pop(float4* pool, unsigned& pool_n, PtPath& s, PtHit& h, pt_lanes& alive)
{
    const pt_lanes need = ~alive;
    const unsigned n_need = (unsigned)__popcll(need);
    const unsigned take = n_need < pool_n ? n_need : pool_n;
    if (take == 0u) return;
    // the wave's own LDS writes (pt_pool_push), read back by other lanes of the same wave: program order
    // suffices for the hardware (one in-order LDS queue per wave); this keeps the compiler from reordering
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const unsigned rank = pt_mbcnt(need);
    const pt_lanes taking = need & PT_LANES(rank < take);   // the first `take` dead lanes
    if (PT_ON(taking)) {
        const unsigned k = pool_n - 1u - rank;
        pt_hit_load<NW>(pt_pool_slots<NW>(pool), k, s, h);
    }
    alive |= taking;
    pool_n -= take;
    // reads of the slots just released must complete before a later push overwrites them: same in-order queue
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- checkpointed launches (PtTraceParams::carry) ---------------------------------------------------------------------
// A wave stops only where its pool is empty and a fresh phase would begin: it parks its live paths exactly as a fresh phase does
// (the bounce loop's own pt_pool_push site -- a second copy of that code after the loop cost fourteen spilled registers INSIDE
// the loop) and leaves; the pool then goes to the wave's region: 16 header dwords and n records of searched paths (pt_hit_store), the
// regions PT_CARRY_HIT_STRIDE_DW apart.  (The LBVH kernel's regions: n records of pt_path_store, PT_CARRY_STRIDE_DW apart.)

// the header: n paths, the rest of the batch, the wave's tallies.  The tallies travel with the checkpoint and reach the stats buffer
// at the end of the render's last launch, where the waves leave one by one: 8 192 waves leaving TOGETHER, two or three atomics each
// on the same line, measured 0.25 ms per launch
PTK_DEV void pt_carry_header(uint32_t* region, unsigned n, const PtWaveQueue& q, unsigned n_rays, unsigned n_samples, unsigned n_carried)
{
    region[0] = n;
    region[1] = q.pix;
    region[2] = q.end;
    region[3] = q.frame;
    region[4] = n_rays;
    region[5] = n_samples;
    region[6] = n_carried + n + (q.end - q.pix);
}

template <unsigned NW>
PTK_DEV void pt_carry_store(uint32_t* region, unsigned lane, float4* pool, unsigned pool_n, const PtWaveQueue& q, unsigned n_rays, unsigned n_samples,
                            unsigned n_carried)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the wave's own pool writes, read by other lanes: as in pt_pool_pop
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < pool_n) {   // (pool_n <= PT_POOL = PT_CARRY_HIT_RECORDS)
        const PtPathSlots from = pt_pool_slots<NW>(pool), to = pt_carry_hit_slots(region);
        for (unsigned j = 0; j < 4u; ++j) to.vec(j, lane) = from.vec(j, lane);
        for (unsigned j = 0; j < NW; ++j) to.word(j, lane) = from.word(j, lane);
    }
    if (lane == 0u) pt_carry_header(region, pool_n, q, n_rays, n_samples, n_carried);
}

// the LBVH kernel's checkpoint: no pool -- the live lanes go to the region directly, compacted (its registers have room for it)
PTK_DEV void pt_carry_store_lanes(uint32_t* region, unsigned lane, const PtPath& s, bool alive, const PtWaveQueue& q, unsigned n_rays, unsigned n_samples,
                                  unsigned n_carried)
{
    const unsigned long long live = __ballot(alive);
    const unsigned n_live = (unsigned)__popcll(live);
    if (alive) {
        const unsigned k = pt_mbcnt(live);
        pt_path_store(pt_carry_slots(region), k, s);
    }
    if (lane == 0u) pt_carry_header(region, n_live, q, n_rays, n_samples, n_carried);
}

// Resuming a checkpoint.  The header first, for either kernel: the tallies, and the rest of the batch becomes the wave's current
// range; returns the number of records.  Then the records go straight into lanes (at most 64, of a table kernel at most PT_POOL: the pool was empty when they were
// parked) -- pt_carry_load for the LBVH kernel's paths, pt_carry_hit_load for the table kernels' searched ones.
template <bool LATE>
PTK_DEV unsigned pt_carry_header_load(const PtTraceParams& P, const uint32_t* region, PtWaveQueue& q, unsigned& n_rays, unsigned& n_samples, unsigned& n_carried)
{
    const pt_kargs_p K = pt_kargs();
    const unsigned n = __builtin_amdgcn_readfirstlane(region[0]);
    n_rays = __builtin_amdgcn_readfirstlane(region[4]);
    n_samples = __builtin_amdgcn_readfirstlane(region[5]);
    n_carried = __builtin_amdgcn_readfirstlane(region[6]);
    q.pix = __builtin_amdgcn_readfirstlane(region[1]);
    q.end = __builtin_amdgcn_readfirstlane(region[2]);
    q.frame = __builtin_amdgcn_readfirstlane(region[3]);
    pt_queue_locate<LATE>(P, K, q);
    return n;
}

template <bool LATE>
PTK_DEV void pt_carry_load(const PtTraceParams& P, uint32_t* region, unsigned lane, PtPath& s, bool& alive, PtWaveQueue& q, unsigned& n_rays,
                           unsigned& n_samples, unsigned& n_carried)
{
    const unsigned n = pt_carry_header_load<LATE>(P, region, q, n_rays, n_samples, n_carried);
    if (lane < n) {
        pt_path_load(pt_carry_slots(region), lane, s);
        alive = true;
    }
}

// the table kernels': the records are searched paths (pt_hit_store; NW as the kernel that stored them, the same kernel of the same render)
template <bool LATE, unsigned NW>
PTK_DEV void pt_carry_hit_load(const PtTraceParams& P, uint32_t* region, unsigned lane, PtPath& s, PtHit& h, bool& alive, PtWaveQueue& q, unsigned& n_rays,
                               unsigned& n_samples, unsigned& n_carried)
{
    const unsigned n = pt_carry_header_load<LATE>(P, region, q, n_rays, n_samples, n_carried);
    if (lane < n) {
        pt_hit_load<NW>(pt_carry_hit_slots(region), lane, s, h);
        alive = true;
    }
}

// The wave is at a fresh-phase boundary (its pool is empty, some lane is dead).  1: [q.pix, q.end) holds samples to start;
// 0: nothing left to start (the classic end: the wave runs its last paths out); 2: STOP -- this launch ends with a
// checkpoint (carry_out): its queue has handed out the last batch (every shard's bit of the stop word is up: a line of its
// own, polled by one lane per wave and fresh phase), and this wave holds nothing of the PREVIOUS launch's chunk any more, whose
// fold follows this launch.
template <bool LATE>
PTK_DEV int pt_queue_next(const PtTraceParams& P, unsigned lane, PtWaveQueue& q, const PtPath& s, pt_lanes alive)
{
    const pt_kargs_p K = pt_kargs();
    unsigned empty_mask = 0u;
    if (PT_ARG(carry_out) != 0u) {
        if (lane == 0u) empty_mask = __hip_atomic_load(PT_ARG(batch_counter) + PT_QUEUE_STOP_WORD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        empty_mask = (unsigned)__builtin_amdgcn_readfirstlane(empty_mask);
        // (of the previous chunk: a batch under way, paths in lanes -- the pool is empty)
        if (empty_mask == (1u << PT_QUEUE_SHARDS) - 1u && !(q.pix != q.end && q.frame < PT_ARG(chunk_f0)) && (alive & PT_LANES(s.fl < PT_ARG(chunk_f0))) == 0ull)
            return 2;
    }
    return pt_queue_refill<LATE>(P, lane, q, empty_mask) ? 1 : 0;
}

// local row sl * stripe_rows + within -> global row: the image's rows are dealt to the ranks in stripes
template <bool LATE>
PTK_DEV unsigned pt_stripe_row(const PtTraceParams& P, pt_kargs_p K, unsigned sl, unsigned within)
{
    return (sl * (unsigned)PT_ARG(n_ranks) + (unsigned)PT_ARG(rank)) * (unsigned)PT_ARG(stripe_rows) + within;
}

// local pixel lp of a rank's stripes -> its column and its row in the whole image
template <bool LATE>
PTK_DEV void pt_pixel_xy(const PtTraceParams& P, pt_kargs_p K, unsigned lp, unsigned& x, unsigned& grow)
{
    const unsigned lr = lp / (unsigned)PT_ARG(width);
    x = lp - lr * (unsigned)PT_ARG(width);
    grow = lr;
    if (PT_ARG(n_ranks) > 1) {
        const unsigned sl = lr / (unsigned)PT_ARG(stripe_rows);
        grow = pt_stripe_row<LATE>(P, K, sl, lr - sl * (unsigned)PT_ARG(stripe_rows));
    }
}

// a new sample of (column x, global row grow) -- local pixel lp, frame `frame` of the render -- at bounce 0: seed :308, camera ray :310
template <bool LATE>
PTK_DEV void pt_sample_begin(const PtTraceParams& P, pt_kargs_p K, unsigned x, unsigned grow, unsigned lp, unsigned frame, PtPath& s)
{
    const unsigned gid = grow * (unsigned)PT_ARG(width) + x;
    const int f = PT_ARG(frame_begin) - (int)PT_ARG(chunk_f0) + (int)frame;   // (the render's first frame + frame)
    s.seed = gid + pt_hash_u32((uint32_t)f);
    pt_generate_ray((int)x, (int)grow, PT_ARG(inv_width), PT_ARG(inv_height), PT_ARG(aspect), PT_CAM_K(K->cam), s.seed, s.o, s.d);
    s.mask = mk3(1.0f, 1.0f, 1.0f);
    s.L = mk3(0.0f, 0.0f, 0.0f);
    s.bounce = 0;
    s.ro = K->rad1_off != 0u ? pt_ring_offset(lp, frame) : lp;   // (from the kernarg segment whichever the kernel, as the store reads it)
    s.fl = frame;
}

// FRESH phase: every lane is dead (its path parked); the next (up to) 64 samples of the wave's range start
// in lanes 0.. at bounce 0 -- seed :308, camera ray :310
// returns true when all 64 lanes started a primary ray; pix0 (wave-uniform): lane k's sample is local pixel pix0 + k -- what the primary
// rays' candidate masks are indexed by (a path does not keep its pixel: PtPath::ro)
template <bool LATE>
PTK_DEV bool pt_start_fresh(const PtTraceParams& P, unsigned lane, PtWaveQueue& q, PtPath& s, pt_lanes& alive, unsigned& pix0)
{
    const pt_kargs_p K = pt_kargs();
    pix0 = q.pix;
    const unsigned avail = q.end - q.pix;
    const unsigned count = avail < 64u ? avail : 64u;
    const unsigned W = (unsigned)PT_ARG(width), SR = (unsigned)PT_ARG(stripe_rows);
    if (lane < count) {
        // local pixel -> (local row, column): walk from the range's own (row, col); 64 pixels span one or two rows
        // unless the image is narrower than a wave
        unsigned x = q.col + lane, up = 0u;
        while (x >= W) { x -= W; ++up; }
        unsigned grow = q.row + up;
        if (PT_ARG(n_ranks) > 1) {
            unsigned sl = q.sl, within = q.within + up;
            while (within >= SR) { within -= SR; ++sl; }
            grow = pt_stripe_row<LATE>(P, K, sl, within);
        }
        pt_sample_begin<LATE>(P, K, x, grow, q.pix + lane, q.frame, s);
    }
    alive = count == 64u ? ~0ull : (1ull << count) - 1ull;   // lanes 0 .. count - 1 (every lane was dead: scalar work)
    q.pix += count;
    q.col += count;
    while (q.col >= W) {
        q.col -= W;
        ++q.row;
        if (++q.within == SR) { q.within = 0u; ++q.sl; }
    }
    return count == 64u;
}

// ---- what both kinds of trace kernel do around their loops ----------------------------------------------------------
PTK_DEV PtPath pt_path_idle()  // what a lane without a path holds
{
    PtPath s;
    s.o = mk3(0.0f, 0.0f, 0.0f); s.d = mk3(0.0f, 0.0f, 1.0f);
    s.mask = mk3(1.0f, 1.0f, 1.0f); s.L = mk3(0.0f, 0.0f, 0.0f);
    s.seed = 0; s.bounce = 0; s.ro = 0; s.fl = 0;
    return s;
}

// the wave's number in its workgroup and in the grid, through readfirstlane: to the compiler threadIdx.x >> 6 differs between lanes,
// and so would everything computed from it (the addresses that use it live in SGPRs)
PTK_DEV unsigned pt_wave_in_wg() { return (unsigned)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
PTK_DEV unsigned pt_wave() { return blockIdx.x * (PT_TRACE_THREADS / 64) + pt_wave_in_wg(); }
// (stride: PT_CARRY_STRIDE_DW for the LBVH kernel, PT_CARRY_HIT_STRIDE_DW for the table kernels)
PTK_DEV uint32_t* pt_carry_region(uint32_t* carry, unsigned wave, unsigned stride = PT_CARRY_STRIDE_DW) { return carry + (size_t)wave * stride; }

// this wave's pass-2 tail: 64 key slots at w, then the pending-pair ring; tile: its record tile (TILED mode only)
PTK_DEV PtTail pt_tail_init(pt_lds_u32* w, unsigned tile, unsigned lane)
{
    PtTail tl;
    tl.keys = (pt_lds_u64*)w;
    tl.list = w + 128;
    tl.wr = tl.rd = 0u;
    tl.kbest = ~0ull; tl.ku = tl.kv = 0.0f;
    tl.tile = tile;
    tl.keys[lane] = ~0ull;
    return tl;
}

// the first n prepared records (12 of their 16 dwords each) into the front of the workgroup's LDS; the caller's barrier follows
PTK_DEV void pt_lds_table_load(const PtPrepTriangle* tris, int n)
{
    const float* g = reinterpret_cast<const float*>(tris);
    for (int k = (int)threadIdx.x; k < n * PT_LDS_TRI_STRIDE; k += PT_TRACE_THREADS) {
        const int tri = k / PT_LDS_TRI_STRIDE, w = k - tri * PT_LDS_TRI_STRIDE;
        pt_lds_tab[k] = g[tri * 16 + w];
    }
}

// ---- the LDS of a table-kernel workgroup, in dwords (the bodies, ptk_trace_lds_bytes): the triangle table (LDS_TABLE 1,
// ntri <= PT_LDS_TRI_MAX), then the waves' pools of parked paths (pt_pool_dwords each), then their pass-2 tails (64 x 8 B keys + PT_TAIL_LIST
// pairs of 2 B beside the table, of 4 B without), then their record tiles of the current 32-triangle chunk (LDS_TABLE 2: TILED)
#define PT_LDS_TILE_DW (32u * PT_LDS_TRI_STRIDE)
template <int LDS_TABLE> __host__ __device__ __forceinline__ unsigned pt_lds_tail_dw() { return 128u + (LDS_TABLE == 1 ? PT_TAIL_LIST / 2u : PT_TAIL_LIST); }
template <int LDS_TABLE> __host__ __device__ __forceinline__ unsigned pt_lds_pools(int ntri) { return LDS_TABLE == 1 ? ntri * PT_LDS_TRI_STRIDE : 0; }
// (POOLS = false: the brute-force query and AO kernels, which park nothing)
template <int LDS_TABLE, bool POOLS = true> __host__ __device__ __forceinline__ unsigned pt_lds_tails(int ntri) { return pt_lds_pools<LDS_TABLE>(ntri) + (POOLS ? (PT_TRACE_THREADS / 64) * pt_pool_dwords<LDS_TABLE>() : 0u); }
template <int LDS_TABLE, bool POOLS = true> __host__ __device__ __forceinline__ unsigned pt_lds_tiles(int ntri) { return pt_lds_tails<LDS_TABLE, POOLS>(ntri) + (PT_TRACE_THREADS / 64) * pt_lds_tail_dw<LDS_TABLE>(); }
template <int LDS_TABLE, bool POOLS = true> __host__ __device__ __forceinline__ unsigned pt_lds_total(int ntri) { return pt_lds_tiles<LDS_TABLE, POOLS>(ntri) + (LDS_TABLE == 2 ? (PT_TRACE_THREADS / 64) * PT_LDS_TILE_DW : 0u); }

#ifndef PT_TRACE_UNIT_DIR
#define PT_TRACE_UNIT_DIR 1  // 0: the trace kernels' filter tests |d|^2 as every other kernel's does (A/B builds, tools/build_variant.sh)
#endif
#ifndef PT_TRACE_SECONDARY_MASKS
#define PT_TRACE_SECONDARY_MASKS 1  // 0: the lookup of secondary rays' candidate masks is compiled out (A/B builds, tools/build_variant.sh)
#endif
template <bool DET_BOUNDED, int LDS_TABLE, int QUADS>
PTK_DEV void pt_trace_body(const PtTraceParams& P)
{
    const unsigned lane = pt_lane_id();
    pt_const_f32p T = (pt_const_f32p)(const float*)P.tris;
    const int ntri = P.ntri;
    if (LDS_TABLE == 1) {
        pt_lds_table_load(P.tris, ntri);
        __syncthreads();
    }
    // this wave's pool of parked paths, pass-2 tail and record tile
    const unsigned wave_in_wg = pt_wave_in_wg();
    constexpr unsigned NW = pt_hit_words<LDS_TABLE>();   // the parked record's dwords beside its four float4 (pt_hit_store)
    float4* pool = reinterpret_cast<float4*>(pt_lds_tab + pt_lds_pools<LDS_TABLE>(ntri) + wave_in_wg * pt_pool_dwords<LDS_TABLE>());
    unsigned pool_n = 0u;                    // parked paths (wave-uniform)
    PtTail tl = pt_tail_init((pt_lds_u32*)pt_lds_tab + pt_lds_tails<LDS_TABLE>(ntri) + (threadIdx.x >> 6) * pt_lds_tail_dw<LDS_TABLE>(),
                             pt_lds_tiles<LDS_TABLE>(ntri) + (threadIdx.x >> 6) * PT_LDS_TILE_DW, lane);

    PtWaveQueue q = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u };   // wave-uniform (SGPRs)
    // Which lanes hold a live path: a wave-uniform LANE MASK (an SGPR pair), changed by scalar instructions where paths park, resume,
    // start and finish, and used as it is where lanes are selected by it (PT_ON) -- not a per-lane 0/1 in a VGPR that every such
    // place first compares into a mask and selects back out of one.
    pt_lanes alive = 0ull;
    // A live lane holds a SEARCHED path at the top of the loop: s with the hit point in s.o (all that shading reads of the origin) and
    // the hit h -- or a miss (h.hidx < 0), which ends there.
    PtPath s = pt_path_idle();
    PtHit h = { 0.0f, 0.0f, -1 };
    pt_lanes ended = 0ull;   // lanes whose path the last shading phase ended: their radiance goes out with the misses', at the loop's one store
    unsigned n_rays = 0, n_samples = 0, n_carried = 0;   // (n_carried: samples this wave's checkpoints have handed on, PT_STAT_CARRIED)
    // checkpointed launches: resume what the previous launch of the render left in this wave's region (searched paths, all of them hits)
    const unsigned wave = pt_wave();
    if (wave < P.carry_in_waves) {
        bool resumed = false;
        pt_carry_hit_load<true, NW>(P, pt_carry_region(P.carry, wave, PT_CARRY_HIT_STRIDE_DW), lane, s, h, resumed, q, n_rays, n_samples, n_carried);
        alive = PT_LANES(resumed);
    }
    q.g = wave & (PT_QUEUE_SHARDS - 1u);   // the wave's first shard of this launch's queue
#if PT_STAMPS
    unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0, c_regen = 0, c_loop = 0, c_shade = 0, c_iters = 0, c_steps = 0, c_p1 = 0;
    PtStampSplit c_split = { 0, 0, 0, 0, 0, 0 };   // (the masked searches' pass 2 alone)
#endif

    // One iteration: the paths the search ended (misses) and the ones shading ended store their radiance; dead lanes take parked
    // paths -- or, when the pool is empty, the live ones are parked and 64 fresh samples start (no shading then: straight to their
    // search, and round again); the live lanes, every one with a hit, shade; the lanes that shading left with a new ray search.
    // Each of these -- the store, the park, the pop, shading, the search -- has ONE site in the loop (a second copy of the park code once
    // cost fourteen spilled registers inside it).
    for (;;) {
        PT_STAMP(t0);
        {
            const pt_lanes missed = alive & PT_LANES(h.hidx < 0);
            if (PT_ON(missed)) pt_shade_miss(s);
            const pt_lanes over = missed | ended;   // (ended lanes left `alive` where they shaded; their L has waited in their registers)
            if (PT_ON(over)) pt_path_finish(s);
            n_samples += (unsigned)__popcll(over);
            alive &= ~missed;
            ended = 0ull;
        }
        bool fresh = false;     // (wave-uniform) this iteration starts samples: no shading, their primary rays are searched next ...
        bool primary = false;   // ... as a full wave of 64 primary rays ...
        unsigned pix0 = 0u;     // ... of the local pixels pix0 + lane
        if (~alive != 0ull) {
            // (a fresh phase parks every live path: it needs room for them -- PT_POOL)
            if (pool_n == 0u && (unsigned)__popcll(alive) <= (unsigned)PT_POOL) {
                const int next = pt_queue_next<true>(P, lane, q, s, alive);
                if (next != 0) {
                    pt_pool_push<NW>(pool, pool_n, s, h, alive);         // park every live path ...
                    if (next == 2) break;                                // ... for the next launch (a checkpoint) ...
                    primary = pt_start_fresh<true>(P, lane, q, s, alive, pix0);   // ... or start 64 coherent primary rays
                    fresh = true;
                }
            }
            if (!fresh) pt_pool_pop<NW>(pool, pool_n, s, h, alive);   // dead lanes resume parked paths
        }
        if (!fresh && alive == 0ull) break;
        PT_STAMP(t1);

        // ---- shading: every live lane has a hit ------------------------------------------------
        if (!fresh) {
            bool finished = false;
            if (PT_ON(alive)) finished = pt_shade_hit<DET_BOUNDED, true>(P, s, s.o, h.hu, h.hv, h.hidx);
            ended = PT_LANES(finished);   // (a dead lane did not shade: its bit is 0)
            alive &= ~ended;
        }
        PT_STAMP(t2);

        // ---- intersectWorld (:137-154): the new rays -- of the lanes that shading left alive, or of the fresh samples --------------
        float tmax = 1e20f, hu = 0.0f, hv = 0.0f;
        int hidx = -1;
        unsigned p2steps = 0;
        n_rays += (unsigned)__popcll(alive);
        // the rays' candidate masks, where a table has them (ONE site for the masked search: the primary rays' masks by pixel, a
        // secondary ray's by the cell of (the triangle it leaves, its origin's tile, its direction): pt_secmask.h)
        bool masked = false;
        uint2 pm = make_uint2(0u, 0u);
        if (QUADS == 3 && DET_BOUNDED && alive != 0ull) {
            if (primary && P.pmask != nullptr) {
                pm = P.pmask[pix0 + lane];
                masked = true;
            } else if (LDS_TABLE == 1 && PT_TRACE_SECONDARY_MASKS && !fresh) {
                // (the table and the triangle count from the kernarg segment -- the compiler loads the count behind the null test, a second scalar
                // load with its own wait: no SGPR is held for either through the loop, and the loop's own copy of ntri, which the register
                // allocator keeps in a spill lane, is not touched)
                const pt_kargs_p KS = pt_kargs();
                const uint2* const sm = KS->smask;
                const int nt = KS->ntri;
                if (sm != nullptr) {
#if PT_STAMPS
                    unsigned long long ta = 0, tb = 0;
                    PT_STAMP(ta);
#endif
                    const PtSmMask ones = pt_sm_all_ones(nt);   // (scalar)
                    pm = make_uint2(ones.x, ones.y);
                    if (PT_ON(alive)) {
                        // the record of the triangle just shaded and the cell's mask: 32-bit offsets against the scalar base, as the
                        // {n, id} gather; every alive lane shaded a hit, and the index is clamped into the table whatever it is
                        const char* const base = reinterpret_cast<const char*>(sm);
                        // (the table holds the cells of ntri triangles, 1 <= ntri <= PT_SM_TRI_MAX: pt_shim.hip, refresh_smask)
                        const unsigned k = (unsigned)h.hidx < (unsigned)(nt - 1) ? (unsigned)h.hidx : (unsigned)(nt - 1);
                        const float4 ra = *reinterpret_cast<const float4*>(base + (size_t)(k * 48u));
                        const float4 rb = *reinterpret_cast<const float4*>(base + (size_t)(k * 48u + 16u));
                        const float4 rn = *reinterpret_cast<const float4*>(base + (size_t)(k * 48u + 32u));
                        const float A[4] = { ra.x, ra.y, ra.z, ra.w }, B[4] = { rb.x, rb.y, rb.z, rb.w }, N[4] = { rn.x, rn.y, rn.z, rn.w };
                        unsigned entry;
                        const bool covered = pt_sm_classify(A, B, N, s.o.x, s.o.y, s.o.z, s.d.x, s.d.y, s.d.z, k, &entry);
                        const uint2 v = *reinterpret_cast<const uint2*>(base + (size_t)(entry * 8u + (unsigned)(PT_SM_HEAD_ENTRIES * 8)));
                        if (covered) pm = v;
#if PT_VALIDATE_FILTER
                        // DIAGNOSTIC build: secondary rays that looked their mask up, and those of them the table does not cover (stats[10], [11])
                        if (P.stats) {
                            const pt_lanes unc = PT_LANES(!covered);
                            if (lane == (unsigned)__builtin_ctzll(alive)) {
                                atomicAdd(&P.stats[10], (unsigned long long)__popcll(alive));
                                atomicAdd(&P.stats[11], (unsigned long long)__popcll(unc & alive));
                            }
                        }
#endif
                    }
                    masked = true;
#if PT_STAMPS
                    PT_STAMP(tb);
                    c_p1 += tb - ta;
#endif
                }
            }
        }
        if (alive == 0ull) {
            // (shading ended every path: nothing to search)
        } else if (masked)
            p2steps = pt_intersect_masked<DET_BOUNDED, LDS_TABLE>(T, P.tris, ntri, s.o, s.d, PT_ON(alive), tmax, hu, hv, hidx, pm, tl, lane,
                                                                  PT_VALIDATE_FILTER && P.stats ? P.stats + 2 : nullptr,
#if PT_STAMPS
                                                                  &c_split
#else
                                                                  nullptr
#endif
                                                                  );
        else
            p2steps = pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS, PT_TRACE_UNIT_DIR != 0>(T, P.tris, ntri, s.o, s.d, PT_ON(alive), tmax, hu, hv, hidx,
                                                                                          P.quad_delta1, P.ray_radius,
                                                                                          (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, pt_anchor(), tl, lane,
                                                                                          PT_VALIDATE_FILTER && P.stats ? P.stats + 2 : nullptr,
#if PT_STAMPS
                                                                                          &c_p1
#else
                                                                                          nullptr
#endif
                                                                                          );
#if PT_STAMPS
        c_steps += p2steps;
#else
        (void)p2steps;
#endif

        // the searched path: its hit point by the very operations shading formed it with (:257 reads the origin only through it)
        s.o = add3(s.o, scale3(s.d, tmax));
        h.hu = hu; h.hv = hv; h.hidx = hidx;
#if PT_STAMPS
        PT_STAMP(t3);
        c_regen += t1 - t0; c_shade += t2 - t1; c_loop += t3 - t2; c_iters++;
#endif
    }

#if PT_STAMPS
    if (P.stats && lane == 0) {
        atomicAdd(&P.stats[2], c_regen);
        atomicAdd(&P.stats[3], c_loop);
        atomicAdd(&P.stats[4], c_shade);
        atomicAdd(&P.stats[5], c_iters);
        atomicAdd(&P.stats[7], c_steps);
        atomicAdd(&P.stats[6], c_p1);
        atomicAdd(&P.stats[8], c_split.own);
        atomicAdd(&P.stats[9], c_split.append);
        atomicAdd(&P.stats[10], c_split.rounds);
        atomicAdd(&P.stats[11], c_split.finish);
        atomicAdd(&P.stats[12], c_split.iters);
        atomicAdd(&P.stats[13], c_split.searches);
    }
#endif
    {
        // (a wave that left the loop because nothing was alive holds nothing: no parked path, no rest of a batch -- an empty checkpoint)
        const pt_kargs_p K = pt_kargs();
        if (K->carry_out != 0u) {
            pt_carry_store<NW>(pt_carry_region(K->carry, wave, PT_CARRY_HIT_STRIDE_DW), lane, pool, pool_n, q, n_rays, n_samples, n_carried);
            return;   // (the tallies went with it)
        }
    }
#if !PT_STAMPS && !PT_VALIDATE_FILTER   // (the diagnostic builds report their own figures in stats[2..7])
    if (P.stats && lane == 0 && n_carried != 0u) atomicAdd(&P.stats[7], (unsigned long long)n_carried);
#endif
    pt_flush_counters(P, lane, n_rays, n_samples);
}

// Waves per SIMD.  More resident waves is what this issue-bound kernel wants (round 2, same source: 5 -> 35.8 ms,
// 6 -> 34.1, 7 -> 32.0); three things had to give for 8: the arguments only regeneration and shading need are re-read
// from the kernarg segment instead of living in SGPRs (pt_kargs: no v_readlane spills, 78 SGPRs), the fresh phase lost
// its per-lane divisions and the camera basis its registers (64 VGPRs without scratch), and the LDS of a workgroup
// stays within 20 480 B (20 032: 56 pool slots of 68 bytes per wave, 2-byte tail pairs) so that 8 workgroups fit the CU's 160 KB.
#ifndef PT_TRACE_WAVES
#define PT_TRACE_WAVES 8
#endif
template <bool DET_BOUNDED, int LDS_TABLE, int QUADS>
__global__ __launch_bounds__(PT_TRACE_THREADS) __attribute__((amdgpu_waves_per_eu(PT_TRACE_WAVES, PT_TRACE_WAVES)))
void pt_trace_kernel(const PtTraceParams P)
{
    pt_trace_body<DET_BOUNDED, LDS_TABLE, QUADS>(P);
}

// TILED brute force (257+ triangles): its LDS (pool + 4-byte pair ring + record tiles = 25.6 KB) admits 6 workgroups
// per CU, so it may as well use the registers of 6 waves per SIMD
template <bool DET_BOUNDED>
__global__ __launch_bounds__(PT_TRACE_THREADS) __attribute__((amdgpu_waves_per_eu(6, 6)))
void pt_trace_tiled_kernel(const PtTraceParams P)
{
    pt_trace_body<DET_BOUNDED, 2, 0>(P);
}

// ---- the LBVH trace kernel -------------------------------------------------------------------------
// Lane = path, and every lane walks its own ray through the hierarchy -- but rays differ wildly in how many nodes they
// enter, so a wave that waits for its slowest lane before shading runs the search at a third of its lanes (round 1:
// 34 %).  Here the search is a per-lane STATE that survives the shading phase: the wave steps all traversing lanes
// together, and as soon as no more than PT_BVH_REFILL of them are still traversing, the finished lanes are shaded,
// dead ones take new samples, and all of them start their next search while the stragglers simply keep theirs.
//   * the hierarchy: eight-child nodes of 64 bytes (PtBvh8Node, pt_kernels.h; built by pt_bvh.hip): one sector, four
//     16-byte loads.  Three things bound the search about equally (profiles/r03/lbvh_bottlenecks.txt): vector-ALU issue,
//     the texture-address path (64 cycles for every load whose lanes read 64 different lines) and the L2's miss path; so a
//     node is as small as eight children allow and the node step is built for few instructions: entry / exit distances are one
//     FMA per plane straight from the quantised bytes, the ray's direction signs select the near and far planes of all
//     eight children at once, the children's slots encode their octant so "slot XOR ray octant" is the front-to-back
//     order (no sort), and the hits of a node travel as ONE stack entry (base index, hit mask) instead of one per child;
//   * a lane's state: the current GROUP of node children still to enter (gbase, gm = hits by slot | imask << 8; which
//     of them comes next is one lookup in a 2 KB table in LDS indexed by the ray's octant and the hits),
//     the leaf children still to test (tbase, tm = hits by slot | lmask << 8), and a stack of earlier groups
//     (PT_BVH_LDS_STACK entries in LDS, entry-major: conflict-free; deeper ones in a private array: a radix tree over
//     64-bit keys has at most 64 levels = 22 levels of eight-child nodes, one entry each);
//   * one wave step = a NODE phase (every lane without pending leaves enters its next node) and, when at least
//     PT_BVH_TRI_LANES lanes hold pending leaves or nobody can enter a node, a TRIANGLE phase (one exact test per such
//     lane): with 64 incoherent lanes some lane meets a leaf at nearly every step, and running the ~70-instruction
//     triangle test for a handful of lanes each time cost more than letting them wait a step or two;
//   * the triangles the builder kept out of the hierarchy (pt_bvh.hip: the few that span the scene) are searched
//     first, by the brute-force two-pass search over their own table, which also hands the traversal a tight tmax;
//   * a step budget and index checks make a damaged hierarchy end the search instead of hanging or faulting the GPU.
// TALLY: the measurement variant (PT_OPT_BVH_TALLY) adds the search's work counters to stats[2..4]: nodes entered,
// triangles tested (both per lane), node and triangle phases executed by the waves.  Never the timed kernel.
// Stack capacity.  An entry is a node's group with children still to enter, so the stack is never deeper than the
// eight-child hierarchy, whose nodes are binary nodes of the radix tree (pt_bvh.hip) in ancestor order: at most the 62 levels
// of a radix tree over 62-bit keys (30-bit Morton code << 32 | index).  64 entries cannot overflow on a hierarchy the builder
// made; PtTraceParams::bvh_stack_limit (<= PT_BVH_STACK) lowers the capacity for the test of the overflow report.
// (The overflow array lives in scratch; one of fewer than 64 dwords would be promoted to registers.)
#ifndef PT_BVH_STACK
#define PT_BVH_STACK 64
#endif
#ifndef PT_BVH_LDS_STACK
#define PT_BVH_LDS_STACK 8
#endif
#ifndef PT_BVH_REFILL
#define PT_BVH_REFILL 40
#endif

// ---- the LDS of an LBVH workgroup, in dwords (pt_trace_bvh_body, ptk_trace_bvh_lds_bytes): the table of the triangles outside the
// hierarchy, the stacks of the workgroup's lanes (PT_BVH_LDS_STACK two-dword entries each), the waves' pass-2 tails (64 x 8 B keys +
// PT_TAIL_LIST x 4 B pairs each), the 2 KB child-order table nxt
#define PT_BVH_TAIL_DW (128u + PT_TAIL_LIST)
__host__ __device__ __forceinline__ unsigned pt_bvh_lds_stacks() { return PT_BVH_BIG_MAX * PT_LDS_TRI_STRIDE; }
__host__ __device__ __forceinline__ unsigned pt_bvh_lds_tails() { return pt_bvh_lds_stacks() + 2 * PT_BVH_LDS_STACK * PT_TRACE_THREADS; }
__host__ __device__ __forceinline__ unsigned pt_bvh_lds_nxt() { return pt_bvh_lds_tails() + (PT_TRACE_THREADS / 64) * PT_BVH_TAIL_DW; }
__host__ __device__ __forceinline__ unsigned pt_bvh_lds_total() { return pt_bvh_lds_nxt() + 2048u / 4u; }

// dead lanes take the next samples of the wave's range, one by one (no coherence to keep here: the search dominates)
template <bool LATE>
PTK_DEV void pt_regenerate_lanes(const PtTraceParams& P, unsigned lane, PtWaveQueue& q, PtPath& s, bool& alive)
{
    const pt_kargs_p K = pt_kargs();
    unsigned long long need = __ballot(!alive);
    while (need != 0ull && pt_queue_refill<true>(P, lane, q, 0u)) {   // (once per batch: its arguments come from the kernarg segment whichever the kernel)
        const unsigned n_need = (unsigned)__popcll(need);
        const unsigned avail = q.end - q.pix;
        const unsigned take = n_need < avail ? n_need : avail;
        const unsigned rank = pt_mbcnt(need);
        if (!alive && rank < take) {
            const unsigned lp = q.pix + rank;
            unsigned x, grow;
            pt_pixel_xy<LATE>(P, K, lp, x, grow);
            pt_sample_begin<LATE>(P, K, x, grow, lp, q.frame, s);
            alive = true;
        }
        q.pix += take;
        need = __ballot(!alive);
    }
}

// a lane's search state (pt_bvh_step): the closest hit so far, the group of node children still to enter (gbase, gm = hits by
// slot | imask << 8), the stack depth.  (Leaf children never wait in the lane: they go to the wave's pair ring, pt_bvh_round.)
struct PtBvhLane {
    float tmax, hu, hv;
    int hidx;
    unsigned gbase, gm;
    unsigned oct;  // bit a set: the ray runs towards +a (children on the low side come first)
    int sp;
    float ix, iy, iz;  // 1 / (dir * tmax): distances along the ray in units of tmax (pt_bvh_scale)
    unsigned budget;
};

// Distances in units of tmax.  The slab test wants, per child, max(entry, 0) <= min(exit, tmax).  With every distance
// divided by tmax the search interval is [0, 1] -- exactly what the VOP3 `clamp` output modifier clamps to, for free: the 48
// FMAs of a node step deliver their planes' distances already clamped, the test is one max3, one min3 and ONE comparison,
// and the 16 v_max / v_min against 0 and tmax of the plain form (9 % of a node step's issue cycles) are gone.  The comparison
// becomes STRICT: a box wholly beyond tmax has entry = exit = 1 after the clamp (one behind the origin 0 = 0) and must
// fail; a box that holds a hit point of the ray is entered strictly before it is left (its faces lie PT_BVH_EPS x the scene
// outside the triangle: pt_bvh.hip), so nothing a triangle needs is lost.  The scaled inverse direction is refreshed whenever
// tmax shrinks (pt_bvh_round); rounding differences against the unscaled form are ~1e-7 of the largest coordinate involved --
// the scene's or the ray origin's -- three orders of magnitude inside the margin's two terms (PT_BVH_EPS, PT_BVH_RAY_EPS).
PTK_DEV void pt_bvh_scale(PtBvhLane& L, const f3& d)
{
    // 1/dir for the slab tests only (conservative boxes: the error of v_rcp_f32 is far inside the boxes' margin), clamped
    // to +-2^60: a zero component keeps its sign and every product stays finite
    // tmax in (0, 1e20]; the cap keeps every product finite for a hit at a denormal distance (the interval then ends below 1:
    // still a superset of [0, tmax])
    const float it = __builtin_fminf(__builtin_amdgcn_rcpf(L.tmax), 0x1p40f);
    L.ix = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d.x), -0x1p60f, 0x1p60f) * it;
    L.iy = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d.y), -0x1p60f, 0x1p60f) * it;
    L.iz = __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d.z), -0x1p60f, 0x1p60f) * it;
}
PTK_DEV float pt_fma_clamp(float a, float b, float c)  // min(max(fma(a, b, c), 0), 1): the clamp is an output modifier, no instruction
{
    float r;
    asm("v_fma_f32 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// the search of a new ray starts at the root (tmax, hu, hv, hidx are the caller's: the big triangles were searched first)
PTK_DEV void pt_bvh_lane_start(PtBvhLane& L, const f3& d, int ntri)
{
    pt_bvh_scale(L, d);
    L.oct = (L.ix < 0.0f ? 0u : 1u) | (L.iy < 0.0f ? 0u : 2u) | (L.iz < 0.0f ? 0u : 4u);
    L.gbase = 0u;  // the root (node 0) as a group of one: slot 0
    L.gm = 1u | (1u << 8);
    L.sp = 0;
    // every node is entered at most once and a hierarchy over ntri leaves has fewer than ntri nodes: a valid tree never
    // uses the budget up (PT_BVH_FLAG_BUDGET reports a damaged one)
    L.budget = (unsigned)ntri + 64u;
}

typedef __attribute__((address_space(3))) unsigned char pt_lds_u8;

// sticky bits of *PtTraceParams::bvh_flags: the search of some ray was CUT SHORT -- its closest hit may be wrong.  The host
// turns them into PT_ERR_TRAVERSAL (pt_render_frames); neither can happen with a hierarchy pt_bvh.hip built (see PT_BVH_STACK)
#define PT_BVH_FLAG_STACK 1u   // a group had to be pushed beyond the stack's capacity
#define PT_BVH_FLAG_BUDGET 2u  // more node visits than the hierarchy has nodes
// The word lives in HOST memory mapped into the device's address space (pt_shim.hip: no render waits for the device to read
// it): one word per bit, raised by a plain system-scope store -- no read-modify-write travels over PCIe, nothing is ever
// read back by a kernel, and the path is taken by no ray of a valid hierarchy.
PTK_DEV void pt_raise_flag(unsigned int* flags, unsigned bit)
{
    __hip_atomic_store(flags + (bit == PT_BVH_FLAG_STACK ? 0 : 1), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- the leaves: (leaf record, ray lane) pairs, tested 64 at a time --------------------------------------------------
// With 64 incoherent lanes some lane meets a leaf at nearly every step, and each lane meets one only every ~10 nodes.  Round
// 2 let a lane WAIT with its leaves until 8 lanes had some and then ran the ~70-instruction exact test for those ~10 lanes
// (16 % of the lanes busy in a triangle phase, 74 % in a node phase: waiting lanes enter no nodes).  Now a lane never waits:
// the leaf children its node test hits are appended, as (record, ray lane) pairs, to the wave's ring in LDS -- the one the
// brute-force search's tail uses (pt_tail_round) -- and the lane goes on to its next node; as soon as PT_BVH_RING_MIN pairs
// are pending the wave tests up to 64 of them at once, one pair per lane whoever owns the ray: the ray travels by
// ds_bpermute, the candidate's key (t bits << 32 | triangle << 6 | testing lane) goes to the ray's slot with one
// ds_min_u64, and the owner picks (t, index) from its slot and (u, v) from the lane that tested the winner.  The reference's
// closest hit is the lexicographic minimum of (t, index) over the triangles that pass the exact test (strict t < tmax in an
// ascending loop, GenerateColors.cl:125,145-151), and the key's order IS that order (t > 0: float bits are monotone), so
// the slot, initialised with the ray's incumbent (tmax, hidx), ends up holding the reference's winner whatever the order of
// the tests.  A ray's tmax now shrinks a few steps later than it could (its leaf waits in the ring), which costs some node
// visits; PT_BVH_RING_MIN trades that against the rounds' occupancy.
// pair = leaf record index << 6 | ray lane; record indices are below 2^26 (2 x triangles: checked by the host)
#ifndef PT_BVH_RING_MIN
#define PT_BVH_RING_MIN 32u
#endif
// ANY: some lanes run an ANY-HIT search (any, per lane: pt_occluded_rays, the occlusion rays of pt_render_ao).  Such a ray's limit
// L.tmax never shrinks, a pair counts only at t < that limit (the closest search's key minimum lets a candidate AT tmax beat the
// incumbent (tmax, no triangle): pt_query_store filters it, an any-hit search must not take it), and the owner keeps the first
// winner's index in L.hidx -- pt_bvh_step then ends its search.  ANY = false is the closest search alone, as before.
template <bool DET_BOUNDED, bool ANY = false>
PTK_DEV void pt_bvh_round(const PtTraceParams& P, PtBvhLane& L, PtTail& tl, unsigned cnt, unsigned lane, const f3& o, const f3& d,
                          unsigned n_recs, bool any = false)
{
    // every lane, as the owner of a ray, publishes its incumbent; a slot nobody improves reads back unchanged
    const unsigned long long k0 = ((unsigned long long)__float_as_uint(L.tmax) << 32) |
                                  (unsigned long long)(((((unsigned)L.hidx) & 0x3ffffffu) << 6) | lane);
    tl.keys[lane] = k0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const bool act = lane < cnt;
    const unsigned e = act ? tl.list[(tl.rd + lane) & (PT_TAIL_LIST - 1u)] : 0u;
    const unsigned ray = e & 63u, idx = e >> 6;
    const unsigned a = ray << 2;
    const f3 po = mk3(pt_from_lane(a, o.x), pt_from_lane(a, o.y), pt_from_lane(a, o.z));
    const f3 pd = mk3(pt_from_lane(a, d.x), pt_from_lane(a, d.y), pt_from_lane(a, d.z));
    const bool valid = act & (idx < n_recs);
    const float4* qp = reinterpret_cast<const float4*>(P.bvh + (valid ? idx : 0u));
    const float4 q0 = qp[0], q1 = qp[1], q2 = qp[2];
    PtTriRec r;  // p1.xyz e1.x | e1.yz e2.xy | e2.z index ...
    r.p1x = q0.x; r.p1y = q0.y; r.p1z = q0.z;
    r.e1x = q0.w; r.e1y = q1.x; r.e1z = q1.y;
    r.e2x = q1.z; r.e2y = q1.w; r.e2z = q2.x;
    const unsigned tri = __float_as_uint(q2.y) & 0x3ffffffu;
    float t, u, v;
    bool ok;
    {   // the reference's test (:96-125) without the running tmax: the slot's minimum applies that
        float pvx = pt_fma(pd.y, r.e2z, -(pd.z * r.e2y));
        float pvy = pt_fma(pd.z, r.e2x, -(pd.x * r.e2z));
        float pvz = pt_fma(pd.x, r.e2y, -(pd.y * r.e2x));
        float det = pt_fma(r.e1z, pvz, pt_fma(r.e1y, pvy, r.e1x * pvx));
        float inv_det = DET_BOUNDED ? pt_rcp(det) : 1.0f / det;  // pt_rcp: exact, range-checked (det may be anything here)
        float tvx = po.x - r.p1x, tvy = po.y - r.p1y, tvz = po.z - r.p1z;
        u = pt_fma(tvz, pvz, pt_fma(tvy, pvy, tvx * pvx)) * inv_det;
        ok = !(det < 1e-8f) & !(-det > 1e-8f) & !(u < 0.0f) & !(u > 1.0f);  // :100, :109
        float qvx = pt_fma(tvy, r.e1z, -(tvz * r.e1y));
        float qvy = pt_fma(tvz, r.e1x, -(tvx * r.e1z));
        float qvz = pt_fma(tvx, r.e1y, -(tvy * r.e1x));
        v = pt_fma(pd.z, qvz, pt_fma(pd.y, qvy, pd.x * qvx)) * inv_det;
        ok &= !(v < 0.0f) & !(u + v > 1.0f);  // :117
        t = pt_fma(r.e2z, qvz, pt_fma(r.e2y, qvy, r.e2x * qvx)) * inv_det;
        ok &= (t > 0.0f) & (t < 1e20f);  // :125 against the initial tmax (:141)
    }
    if (ANY) {   // the owner's search kind and limit travel with its ray
        const bool pany = __builtin_amdgcn_ds_bpermute((int)a, any ? 1 : 0) != 0;
        ok &= !pany | (t < pt_from_lane(a, L.tmax));
    }
    if (ok & valid) {
        const unsigned long long key = ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)((tri << 6) | lane);
        __hip_atomic_fetch_min(tl.keys + ray, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const unsigned long long slot = tl.keys[lane];
    const unsigned from = ((unsigned)slot & 63u) << 2;
    const float pu = pt_from_lane(from, u), pv = pt_from_lane(from, v);
    if (slot != k0) {  // (t, index) < the incumbent's: the new closest hit
        if (ANY && any) {
            L.hidx = (int)(((unsigned)slot >> 6) & 0x3ffffffu);   // an any-hit search: some triangle is hit below the limit
        } else {
            L.tmax = __uint_as_float((unsigned)(slot >> 32));
            L.hidx = (int)(((unsigned)slot >> 6) & 0x3ffffffu);
            L.hu = pu;
            L.hv = pv;
            pt_bvh_scale(L, d);
        }
    }
    tl.rd += cnt;
}

// one step of the wave: a node phase for every traversing lane (trav: the lane still has nodes to enter), its leaf hits to the
// ring, a round when enough pairs are pending.  stk: this lane's stack in LDS, ovf: its overflow in scratch, nxt: the 2 KB
// child-order table
// (ANY, any: pt_bvh_round -- an any-hit lane leaves its traversal at the first accepted pair; its pairs still in the ring are
// tested for it alone and change nothing)
// c_*: the search's work counters, touched by the TALLY instantiations alone.  (Five scalars on purpose: bundled into a struct they move
// the compiled code of the timed trace kernels, profiles/driver/disasm_comparison.txt.)  A caller that keeps none uses the form below.
template <bool DET_BOUNDED, bool TALLY, bool ANY = false, bool WIDE = true>
PTK_DEV void pt_bvh_step(const PtTraceParams& P, PtBvhLane& L, bool& trav, const f3& o, const f3& d, pt_lds_u32* stk, unsigned* ovf,
                         const pt_lds_u8* nxt, PtTail& tl, unsigned lane, unsigned n_recs, unsigned& c_nodes, unsigned& c_leaves,
                         unsigned long long& c_steps, unsigned long long& c_tsteps, unsigned& c_maxsp, bool any = false)
{
    unsigned ht = 0u, cmask = 0u, cbase = 0u;
    if (TALLY) ++c_steps;
    if (trav) {
        if (TALLY) ++c_nodes;
        if ((L.gm & 255u) == 0u) {  // (then L.sp > 0)
            L.sp = L.sp > 0 ? L.sp - 1 : 0;
            if (L.sp < PT_BVH_LDS_STACK) { L.gbase = stk[(2 * L.sp) * PT_TRACE_THREADS]; L.gm = stk[(2 * L.sp + 1) * PT_TRACE_THREADS]; }
            else { L.gbase = ovf[2 * (L.sp - PT_BVH_LDS_STACK)]; L.gm = ovf[2 * (L.sp - PT_BVH_LDS_STACK) + 1]; }
        }
        // the group's next child: highest priority first; its slot, its rank among its parent's children
        const unsigned slot = nxt[(L.oct << 8) | (L.gm & 255u)];
        L.gm &= ~(1u << slot);
        const unsigned node = L.gbase + (unsigned)__popc((L.gm >> 8) & ((1u << slot) - 1u));
        unsigned h = 0u, imask = 0u, lmask = 0u;
        if (node < n_recs) {
            const uint4* np = reinterpret_cast<const uint4*>(P.bvh + node);
            const uint4 w0 = np[0], w2 = np[1], w3 = np[2], w4 = np[3];
            // header: org.x | org.y << 16, org.z | ex.x << 16 | ex.y << 24, ex.z | imask << 8 | lmask << 16, base
            const float sx = __uint_as_float(((w0.y >> 16) & 255u) << 23), sy = __uint_as_float((w0.y >> 24) << 23),
                        sz = __uint_as_float((w0.z & 255u) << 23);
            imask = (w0.z >> 8) & 255u;
            lmask = (w0.z >> 16) & 255u;
            cbase = w0.w;
            // the origin off its 16-bit grid position: the builder checked the boxes against this very expression
            const float ox = pt_fma((float)(w0.x & 0xffffu), P.grid.gstep[0], P.grid.gmin[0]);
            const float oy = pt_fma((float)(w0.x >> 16), P.grid.gstep[1], P.grid.gmin[1]);
            const float oz = pt_fma((float)(w0.y & 0xffffu), P.grid.gstep[2], P.grid.gmin[2]);
            // entry / exit distances straight from the bytes, in units of tmax and clamped to [0, 1] (pt_bvh_scale):
            // t = fma(q, step / (d tmax), (origin - o) / (d tmax)); against decoding the box first this differs by a few
            // ulp of |coordinate| / |d|, orders of magnitude inside the boxes' PT_BVH_EPS margin
            const float kx = sx * L.ix, ky = sy * L.iy, kz = sz * L.iz;
            // every slab is widened by w = PT_BVH_RAY_EPS x (the origin's largest |coordinate|) on both sides (pt_kernels.h): the
            // near planes' constant lies w / |d| earlier, the far planes' w / |d| later.  (While kx, ky, kz are finite, an infinite
            // w |i| -- an absurdly far origin -- makes the constants -Inf and +Inf, which clamp to 0 and 1: every box is entered.)
            // WIDE = false: the renderer's kernels when every ray starts in or next to the scene (ptk_trace): w = 0, the plain form.
            float cnx, cny, cnz, cfx, cfy, cfz;
            if (WIDE) {
                const float w = PT_BVH_RAY_EPS * __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)), __builtin_fabsf(o.z));
                const float wx = w * __builtin_fabsf(L.ix), wy = w * __builtin_fabsf(L.iy), wz = w * __builtin_fabsf(L.iz);
                const float dx = ox - o.x, dy = oy - o.y, dz = oz - o.z;
                cnx = pt_fma(dx, L.ix, -wx); cny = pt_fma(dy, L.iy, -wy); cnz = pt_fma(dz, L.iz, -wz);
                cfx = pt_fma(dx, L.ix, wx); cfy = pt_fma(dy, L.iy, wy); cfz = pt_fma(dz, L.iz, wz);
            } else {
                const float cx = (ox - o.x) * L.ix, cy = (oy - o.y) * L.iy, cz = (oz - o.z) * L.iz;
                cnx = cfx = cx; cny = cfy = cy; cnz = cfz = cz;
            }
            // near / far planes of all eight children by the direction's signs: qlo x y z = w2.xy w2.zw w3.xy,
            // qhi x y z = w3.zw w4.xy w4.zw (slots 0-3 in the first word, 4-7 in the second)
            const bool px = (L.oct & 1u) != 0u, py = (L.oct & 2u) != 0u, pz = (L.oct & 4u) != 0u;
            const unsigned nx0 = px ? w2.x : w3.z, nx1 = px ? w2.y : w3.w, fx0 = px ? w3.z : w2.x, fx1 = px ? w3.w : w2.y;
            const unsigned ny0 = py ? w2.z : w4.x, ny1 = py ? w2.w : w4.y, fy0 = py ? w4.x : w2.z, fy1 = py ? w4.y : w2.w;
            const unsigned nz0 = pz ? w3.x : w4.z, nz1 = pz ? w3.y : w4.w, fz0 = pz ? w4.z : w3.x, fz1 = pz ? w4.w : w3.y;
#define PT_B8(lo_, hi_, k) (float)((((k) < 4 ? (lo_) : (hi_)) >> (8 * ((k) & 3))) & 255u)
#pragma unroll
            for (int k = 7; k >= 0; --k) {  // (MSB first: slot k ends up in bit k)
                const float tnx = pt_fma_clamp(PT_B8(nx0, nx1, k), kx, cnx), tfx = pt_fma_clamp(PT_B8(fx0, fx1, k), kx, cfx);
                const float tny = pt_fma_clamp(PT_B8(ny0, ny1, k), ky, cny), tfy = pt_fma_clamp(PT_B8(fy0, fy1, k), ky, cfy);
                const float tnz = pt_fma_clamp(PT_B8(nz0, nz1, k), kz, cnz), tfz = pt_fma_clamp(PT_B8(fz0, fz1, k), kz, cfz);
                const float tn = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), tnz);  // already within [0, 1] = [0, tmax]
                const float tf = __builtin_fminf(__builtin_fminf(tfx, tfy), tfz);
                h = pt_push_flag(h, PT_LANES(tn < tf));
            }
#undef PT_B8
        }
        const unsigned hn = h & imask;
        ht = h & lmask;
        cmask = imask | lmask;
        // the rest of the old group goes on the stack, the children just hit become the current group
        if ((L.gm & 255u) != 0u && hn != 0u) {
            if (L.sp < PT_BVH_LDS_STACK) { stk[(2 * L.sp) * PT_TRACE_THREADS] = L.gbase; stk[(2 * L.sp + 1) * PT_TRACE_THREADS] = L.gm; }
            else if (L.sp < (int)P.bvh_stack_limit) { ovf[2 * (L.sp - PT_BVH_LDS_STACK)] = L.gbase; ovf[2 * (L.sp - PT_BVH_LDS_STACK) + 1] = L.gm; }
            if (L.sp < (int)P.bvh_stack_limit) ++L.sp;
            else pt_raise_flag(P.bvh_flags, PT_BVH_FLAG_STACK);  // the group is lost: the host reports the render as failed
            if (TALLY) c_maxsp = (unsigned)L.sp > c_maxsp ? (unsigned)L.sp : c_maxsp;
        }
        if (hn != 0u) {
            L.gbase = cbase;
            L.gm = hn | (cmask << 8);
        }
        --L.budget;
        // a lane with nothing left to enter is done with the nodes (its last leaves may still be in the ring)
        if (((L.gm & 255u) == 0u) && L.sp == 0) trav = false;
        if ((int)L.budget <= 0) { if (trav) pt_raise_flag(P.bvh_flags, PT_BVH_FLAG_BUDGET); trav = false; }
    }
    // ---- the leaf children just hit join the wave's pending pairs ----------------------------
    for (pt_lanes has = PT_LANES(ht != 0u); has != 0ull; has = PT_LANES(ht != 0u)) {
        if (ht != 0u) {
            if (TALLY) ++c_leaves;
            const unsigned slot = (unsigned)__builtin_ctz(ht);
            ht &= ht - 1u;
            const unsigned rec = cbase + (unsigned)__popc(cmask & ((1u << slot) - 1u));
            tl.list[(tl.wr + pt_mbcnt(has)) & (PT_TAIL_LIST - 1u)] = (rec << 6) | lane;
        }
        tl.wr += (unsigned)__popcll(has);
        if (tl.wr - tl.rd >= 64u) {  // (room for the next 64)
            if (TALLY) ++c_tsteps;
            pt_bvh_round<DET_BOUNDED, ANY>(P, L, tl, 64u, lane, o, d, n_recs, any);
        }
    }
    if (tl.wr - tl.rd >= (unsigned)PT_BVH_RING_MIN) {
        if (TALLY) ++c_tsteps;
        pt_bvh_round<DET_BOUNDED, ANY>(P, L, tl, tl.wr - tl.rd, lane, o, d, n_recs, any);
    }
    if (ANY && any && L.hidx >= 0) trav = false;
}
// ... for the callers that keep no counters (pt_bvh_drive)
template <bool DET_BOUNDED, bool ANY>
PTK_DEV void pt_bvh_step(const PtTraceParams& P, PtBvhLane& L, bool& trav, const f3& o, const f3& d, pt_lds_u32* stk, unsigned* ovf,
                         const pt_lds_u8* nxt, PtTail& tl, unsigned lane, unsigned n_recs, bool any)
{
    unsigned c32 = 0u;
    unsigned long long c64 = 0ull;
    pt_bvh_step<DET_BOUNDED, false, ANY>(P, L, trav, o, d, stk, ovf, nxt, tl, lane, n_recs, c32, c32, c64, c64, c32, any);
}

// What an LBVH workgroup holds in LDS before its loop (pt_bvh_lds_*): the table of the triangles outside the hierarchy (pass 2
// fetches its records per lane: pt_fetch_rec) and the 2 KB child-order table, which it returns: nxt[oct << 8 | hits] = the slot s
// among the hits (by slot) with the largest s ^ oct -- the octant nearest to where the ray comes from
PTK_DEV pt_lds_u8* pt_bvh_wg_setup(const PtTraceParams& P)
{
    pt_lds_table_load(P.bigtab, P.nbig);
    pt_lds_u8* nxt = (pt_lds_u8*)((pt_lds_u32*)pt_lds_tab + pt_bvh_lds_nxt());
    for (unsigned k = threadIdx.x; k < 2048u; k += PT_TRACE_THREADS) {
        const unsigned o = k >> 8, h = k & 255u;
        unsigned best = 0u, bp = 0u;
        for (unsigned sl = 0; sl < 8u; ++sl)
            if (((h >> sl) & 1u) && ((sl ^ o) >= bp)) { bp = sl ^ o; best = sl; }
        nxt[k] = (unsigned char)best;
    }
    __syncthreads();
    return nxt;
}

// a lane's search state at the start of a new ray: the limit, no hit
PTK_DEV void pt_bvh_lane_clear(PtBvhLane& L, float tlim)
{
    L.tmax = tlim; L.hu = 0.0f; L.hv = 0.0f; L.hidx = -1;
}

PTK_DEV PtBvhLane pt_bvh_lane_idle(float tlim)   // what a lane that searches nothing holds
{
    PtBvhLane L;
    pt_bvh_lane_clear(L, tlim);
    L.gbase = L.gm = L.oct = 0u; L.sp = 0; L.ix = L.iy = L.iz = 0.0f; L.budget = 0u;
    return L;
}

// The start of a ray's LBVH search for the lanes in `start`: the triangles outside the hierarchy by the two-pass search (its
// tail shares the key slots with pt_bvh_round and expects them empty: the ring has just been flushed), then the root.  An
// any-hit ray (any) that hits one of them is done: it does not traverse.
template <bool DET_BOUNDED, int BIGQ>
PTK_DEV void pt_bvh_search_start(const PtTraceParams& P, PtBvhLane& L, bool& trav, bool start, bool any, const f3& o, const f3& d,
                                 PtTail& tl, unsigned lane)
{
    if (__ballot(start) == 0ull) return;
    if (P.nbig > 0) {
        int hp = -1;
        tl.keys[lane] = ~0ull;
        pt_intersect_two_pass<DET_BOUNDED, 1, (DET_BOUNDED ? BIGQ : 0)>((pt_const_f32p)(const float*)P.bigtab, P.bigtab, P.nbig, o, d, start,
                                                                          L.tmax, L.hu, L.hv, hp, P.quad_delta1, P.ray_radius,
                                                                          (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi,
                                                                          mk3(P.cam.eye[0], P.cam.eye[1], P.cam.eye[2]), tl, lane);
        if (start && hp >= 0) L.hidx = P.bigidx[hp];
    }
    if (start && !(any && L.hidx >= 0)) {
        pt_bvh_lane_start(L, d, P.ntri);
        trav = true;
    }
}

// BIGQ: the filter of the brute-force search over the big triangles: 0 = independent triangles, 3 = the packed shared-u filter
// (their table is made of quads -- the Cornell box's walls among a soup -- and the host prepared its pass-1 table)
template <bool DET_BOUNDED, bool TALLY, int BIGQ, bool WIDE>
PTK_DEV void pt_trace_bvh_body(const PtTraceParams& P)
{
    const unsigned lane = pt_lane_id();
    const int ntri = P.ntri;
    const unsigned n_recs = (unsigned)P.bvh_records;
    const pt_lds_u8* nxt = pt_bvh_wg_setup(P);
    // stack entry e of this lane: stk[2 e * PT_TRACE_THREADS] = base, stk[(2 e + 1) * PT_TRACE_THREADS] = masks
    pt_lds_u32* stk = (pt_lds_u32*)pt_lds_tab + pt_bvh_lds_stacks() + threadIdx.x;
    unsigned ovf[2 * (PT_BVH_STACK - PT_BVH_LDS_STACK)];
    PtTail tl = pt_tail_init((pt_lds_u32*)pt_lds_tab + pt_bvh_lds_tails() + (threadIdx.x >> 6) * PT_BVH_TAIL_DW, 0u, lane);
    pt_const_f32p bigT = (pt_const_f32p)(const float*)P.bigtab;

    PtWaveQueue q = { 0u, 0u, 0u, 0u, 0u, 0u, 0u, pt_wave() & (PT_QUEUE_SHARDS - 1u) };
    bool alive = false;  // the lane holds a path
    bool trav = false;   // ... whose closest-hit search is in progress
    PtPath s = pt_path_idle();
    unsigned n_rays = 0, n_samples = 0, n_carried = 0;
    // checkpointed launches (PtTraceParams::carry), as in the table kernels: a launch whose queue has handed out its last batch stops
    // starting searches -- the lanes still searching finish THAT search (a hundred node steps, not the up to sixteen bounces a path has
    // left), are shaded, and what every lane then holds is a path about to start its next search: 60 bytes a lane, resumed by the next
    // launch of the render.  A launch's end is one search deep instead of one path deep.
    // (the fields only this needs are read from the kernarg segment where they are used, pt_kargs: the kernel's SGPRs are spoken for)
    unsigned visits = 0u;   // (wave-uniform) passes through the refill point
    bool parked = false;    // the lane's path is between two searches (shaded; its next search not begun): what a checkpoint holds
    {
        const pt_kargs_p K = pt_kargs();
        const unsigned wave = pt_wave();
        if (wave < K->carry_in_waves) {
            const unsigned shard = q.g;
            pt_carry_load<true>(P, pt_carry_region(K->carry, wave), lane, s, alive, q, n_rays, n_samples, n_carried);
            q.g = shard;
            parked = alive;
        }
    }
    PtBvhLane L = pt_bvh_lane_idle(1e20f);  // the search's state
    unsigned c_nodes = 0, c_leaves = 0, c_maxsp = 0, c_graze = 0;
    unsigned long long c_steps = 0, c_tsteps = 0;

    for (;;) {
        if ((unsigned)__popcll(__ballot(trav)) <= (unsigned)PT_BVH_REFILL) {
            // the pending pairs first: a lane that has no nodes left has its closest hit only once its leaves are tested
            if (tl.wr != tl.rd) {
                if (TALLY) ++c_tsteps;
                pt_bvh_round<DET_BOUNDED>(P, L, tl, tl.wr - tl.rd, lane, s.o, s.d, n_recs);
            }
            // (a lane that holds a path and is not searching has FINISHED a search -- unless the path is PARKED: shaded already and waiting
            // for the checkpoint of a launch that is stopping, or just resumed from one; those start their next search below)
            const unsigned long long shaded = __ballot(alive && !trav && !parked);
            n_rays += (unsigned)__popcll(shaded);
            if (TALLY && alive && !trav && !parked && L.hidx >= 0) {
                // the LBVH's exposure (pt_bvh.hip: no finite box margin is PROVABLY conservative for rays within a fraction of a degree
                // of a triangle's plane; the margin covers cos(incidence) >= 1e-2 with a factor 10 to spare): accepted hits that lie
                // outside that range.  cos(incidence) = |dir . n| / |n|, n = e2 x e1 (the prepared record's), |dir| = 1.
                const PtPrepTriangle* t = P.tris + L.hidx;
                const float nx = t->n[0], ny = t->n[1], nz = t->n[2];
                const float dn = __builtin_fabsf(s.d.x * nx + s.d.y * ny + s.d.z * nz);
                if (dn < 1.0e-2f * __builtin_sqrtf(nx * nx + ny * ny + nz * nz)) ++c_graze;
            }
            if (alive && !trav && !parked) pt_shade<DET_BOUNDED, false>(P, s, alive, L.tmax, L.hu, L.hv, L.hidx);
            n_samples += (unsigned)__popcll(shaded & ~__ballot(alive));
            // stop?  (carry_out launches: the queue has nothing left for this wave, and it holds nothing of the previous launch's chunk any
            // more, whose fold follows this launch)
            // (this point is passed every few node steps: the queue's stop word is polled at every 16th pass only; otherwise the wave learns
            // that the queue is empty from its own grabs.  Either way q.g says so from then on, and what is left of the wave's batch
            // travels with the checkpoint.  The kernarg fields are read only here.)
            bool stopping = false;
            if (q.g != PT_Q_EMPTY && (++visits & 15u) == 0u) {
                const pt_kargs_p K = pt_kargs();
                if (K->carry_out != 0u) {
                    unsigned empty_mask = 0u;
                    if (lane == 0u) empty_mask = __hip_atomic_load(K->batch_counter + PT_QUEUE_STOP_WORD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if ((unsigned)__builtin_amdgcn_readfirstlane(empty_mask) == (1u << PT_QUEUE_SHARDS) - 1u) q.g = PT_Q_EMPTY;
                }
            }
            if (q.g == PT_Q_EMPTY) {
                const pt_kargs_p K = pt_kargs();
                stopping = K->carry_out != 0u && !(q.pix != q.end && q.frame < K->chunk_f0) && __ballot(alive && s.fl < K->chunk_f0) == 0ull;
            }
            if (stopping) {
                parked = alive && !trav;
                if (__ballot(trav) == 0ull) break;   // every lane holds a path between two searches (or none): the checkpoint
                pt_bvh_step<DET_BOUNDED, TALLY, false, WIDE>(P, L, trav, s.o, s.d, stk, ovf, nxt, tl, lane, n_recs, c_nodes, c_leaves, c_steps, c_tsteps, c_maxsp);
                continue;
            }
            pt_regenerate_lanes<false>(P, lane, q, s, alive);
            const bool start = alive && !trav;
            parked = false;
            if (__ballot(start) != 0ull) {
                if (start) pt_bvh_lane_clear(L, 1e20f);
                // (pt_bvh_search_start's steps, kept in place here: routed through it, this kernel's compiled code moves)
                if (P.nbig > 0) {
                    // the triangles outside the hierarchy, in ascending index order; hp = position in their table.  (Its tail
                    // shares the key slots with pt_bvh_round and expects them empty: the ring has just been flushed.)
                    int hp = -1;
                    tl.keys[lane] = ~0ull;
                    pt_intersect_two_pass<DET_BOUNDED, 1, (DET_BOUNDED ? BIGQ : 0)>(bigT, P.bigtab, P.nbig, s.o, s.d, start, L.tmax, L.hu, L.hv, hp,
                                                                                      P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, pt_anchor(), tl, lane,
                                                                                      PT_VALIDATE_FILTER && !TALLY && P.stats ? P.stats + 2 : nullptr);  // (diagnostic build: tools/validate_filter.py)
                    if (start && hp >= 0) L.hidx = P.bigidx[hp];
                }
                if (start) {
                    pt_bvh_lane_start(L, s.d, ntri);
                    trav = true;
                }
            }
            if (__ballot(alive) == 0ull) break;
        }
        pt_bvh_step<DET_BOUNDED, TALLY, false, WIDE>(P, L, trav, s.o, s.d, stk, ovf, nxt, tl, lane, n_recs, c_nodes, c_leaves, c_steps, c_tsteps, c_maxsp);
    }

    if (TALLY && P.stats) {
        unsigned long long n = c_nodes, l = c_leaves, gz = c_graze;
        for (int off = 32; off > 0; off >>= 1) {
            n += __shfl_down(n, off);
            l += __shfl_down(l, off);
            gz += __shfl_down(gz, off);
        }
        if (lane == 0) {
            atomicAdd(&P.stats[2], n);
            atomicAdd(&P.stats[3], l);
            if (gz) atomicAdd(&P.stats[8], gz);   // PT_STAT_BVH_GRAZING
            atomicAdd(&P.stats[4], c_steps);
            atomicAdd(&P.stats[5], c_tsteps);
        }
        atomicMax(&P.stats[6], (unsigned long long)c_maxsp);  // deepest stack any ray of the launch needed
    }
    {
        // (a wave that left the loop because nothing was alive holds nothing -- no path, no rest of a batch: an empty checkpoint; its tallies
        // travel with it either way)
        const pt_kargs_p K = pt_kargs();
        if (K->carry_out != 0u) {
            pt_carry_store_lanes(pt_carry_region(K->carry, pt_wave()), lane, s, alive, q, n_rays, n_samples, n_carried);
            return;
        }
    }
#if !PT_VALIDATE_FILTER
    if (P.stats && lane == 0 && n_carried != 0u) atomicAdd(&P.stats[7], (unsigned long long)n_carried);
#endif
    pt_flush_counters(P, lane, n_rays, n_samples);
}

// five waves per SIMD (96 VGPRs): what the search is balanced at (round 3: four and six are both 10 % slower); left to itself hipcc takes
// 102 registers for the checkpointed body -- four waves
#ifndef PT_BVH_WAVES
#define PT_BVH_WAVES 5
#endif
#define PT_BVH_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(PT_BVH_WAVES, PT_BVH_WAVES)))
// WIDE: the slabs carry the ray term of the margin (pt_bvh_step); false when the host knows that every ray starts in or next to the scene
template <bool DET_BOUNDED, bool TALLY, int BIGQ, bool WIDE = false>
__global__ __launch_bounds__(PT_TRACE_THREADS) PT_BVH_WAVES_ATTR
void pt_trace_bvh_kernel(const PtTraceParams P)
{
    pt_trace_bvh_body<DET_BOUNDED, TALLY, BIGQ, WIDE>(P);
}

// ------------------------------------------------------------------------------------------
// fold kernel: GenerateColors.cl:290-300, 314-321, frames in ascending order per pixel
// ------------------------------------------------------------------------------------------
// Per frame z >= 1 and channel the reference computes
//     o = pow(m, 2.2f);   m = pow((o * (z - 1) + c) / z, 1.0f / 2.2f)              (:316-320)
// where m is the pixel it wrote one frame earlier: two pow and one division per sample and channel,
// all of the fold's time.  Written literally (round 2) that is 112 vector instructions per frame, 27 of
// them binary64.  Two of the three operations have an operand with structure, and each gets a short
// form that returns THE SAME BITS (tests/test_gpu_fold_exact.py compares each with the literal form
// over every binary32 operand, on the GPU):
//
//  * decode, o = pow(m, 2.2f).  m is not any number: it is m = fl32(E), E = the binary64 value of
//    pow(v, 1/2.2f) one step earlier, and v, E and log2(v) are still in registers.  Exactly,
//        m^y2 = v * v^eta * (1 + delta)^y2,      delta = (m - E) / E,   eta = y1 * y2 - 1 = -1.41e-8
//    (y1 = fl32(1/2.2f), y2 = 2.2f), up to the 2^-49 of the two binary64 evaluations.  So o lies within
//    a few ulps of v, and   o = fl32(v + v * (y2 * delta + eta * ln v))   whenever that rounding is the
//    same at both ends of the expression's uncertainty interval (Ziv's test; the neglected terms are
//    (eta ln v)^2 / 2 < 2^-41 and y2 (y2 - 1) delta^2 / 2 < 2^-47, binary32 evaluation of the small
//    term adds < 2^-42: the interval is +- 2^-36 v).  One sample in 3 000 fails the test and
//    takes the literal pow; 14 instructions replace 50.
//  * the division by z.  z is the same for the whole launch step, 1/z correctly rounded comes from a
//    table in LDS, and Markstein's sequence (IBM J. R&D 34, 1990: y = RN(1/b), q0 = RN(a y),
//    r = fma(-b, q0, a), q = fma(r, y, q0)) gives the IEEE quotient in three instructions (checked over every
//    pair of significands: pt_device_math.h, pt_div3) as long as nothing underflows: numerators in
//    [PT_FOLD_NUM_MIN, 2^80), whose quotient is in the range where the next pow needs no special case.
//  * encode, m = pow(a, 1/2.2f): pt_pow_regular (no special cases left to test).
// Zero (black so far) is common and handled by selection; anything else outside the regular range
// (negative, NaN, infinite, tiny, huge) takes the literal operations in a branch that whole waves skip.
#define PT_FOLD_RCP_N 2048            // 1/z tabulated for z < this; later frames divide
#define PT_FOLD_ETA_LN2 -0x1.4f889ep-27f   // (fl32(1/2.2f) * 2.2f - 1) * ln 2
#define PT_FOLD_ZIV 0x1p-36f
#define PT_FOLD_NUM_MIN 0x1p-69f       // PTK_POW_REGULAR_MIN * PT_FOLD_RCP_N

struct PtFoldChain {
    float m;      // the pixel: gamma-encoded running mean
    float v;      // what m was encoded from
    double E, l;  // binary64 pow(v, 1/2.2f) before its rounding to m, and log2(v)
    bool reg;     // v was regular: E and l are valid
};

// a / zf for a regular: IEEE quotient (Markstein, pt_device_math.h); y = RN(1 / zf)
PTK_DEV float pt_fold_div(float a, float zf, float y) { return pt_div_markstein(a, zf, y); }

// o = pow(s.m, 2.2f)
PTK_DEV float pt_fold_decode(const PtFoldChain& s, const double* LC, const double* LL, const double* ET, unsigned* n_slow)
{
    float o = 0.0f;
    bool ok = s.reg;
    if (ok) {
        const float df = (float)((double)s.m - s.E);
        const float c = pt_fma(PT_FOLD_ETA_LN2, (float)s.l, (PTK_GAMMA * df) * __builtin_amdgcn_rcpf(s.m));
        const float t1 = s.v * c;
        const float u = s.v * PT_FOLD_ZIV;
        const float lo = s.v + (t1 - u), hi = s.v + (t1 + u);
        o = lo;
        ok = lo == hi;
    }
    if (!ok && s.m != 0.0f) {
        o = pt_pow(s.m, PTK_GAMMA, LC, LL, ET);
        if (n_slow) ++*n_slow;
    }
    return o;
}

// s <- the chain after m = pow(a, 1/2.2f)
PTK_DEV void pt_fold_encode(PtFoldChain& s, float a, bool reg, const double* LC, const double* LL, const double* ET)
{
    const float inv_gamma = 1.0f / PTK_GAMMA;
    s.E = pt_pow_regular(reg ? a : 1.0f, inv_gamma, LC, LL, ET, s.l);
    s.m = (float)s.E;
    s.v = a;
    s.reg = reg;
    if (!reg) s.m = (a == 0.0f) ? 0.0f : pt_pow(a, inv_gamma, LC, LL, ET);
}

// one frame of :314-321 for one channel: z = the frame's number, c = its radiance, rz = RN(1/z) if z < PT_FOLD_RCP_N
PTK_DEV void pt_fold_frame(PtFoldChain& s, int z, float c, const float* rcp_z, const double* LC, const double* LL,
                           const double* ET, unsigned* n_slow)
{
    float a = c;
    bool reg = pt_pow_is_regular(c);
    if (z != 0) {
        const float o = pt_fold_decode(s, LC, LL, ET, n_slow);
        const float zm1 = (float)(z - 1), zf = (float)z;
        const float num = o * zm1 + c;
        if (z < PT_FOLD_RCP_N) {
            // numerators in [2^-69, 2^80): the quotient by z < 2^11 is then regular itself -- inside the range over which the
            // encode and the next decode were compared with the literal pow exhaustively
            reg = (__float_as_uint(num) - __float_as_uint(PT_FOLD_NUM_MIN)) < (__float_as_uint(PTK_POW_REGULAR_MAX) - __float_as_uint(PT_FOLD_NUM_MIN));
            a = pt_fold_div(reg ? num : 1.0f, zf, rcp_z[z]);
            if (!reg) {
                a = (num == 0.0f) ? 0.0f : num / zf;
                reg = pt_pow_is_regular(a);
            }
        } else {
            a = num / zf;
            reg = pt_pow_is_regular(a);
        }
    }
    pt_fold_encode(s, a, reg, LC, LL, ET);
}

__global__ __launch_bounds__(256) void pt_fold_kernel(const PtFoldParams P)
{
    // the three pow tables (3 KiB) and the reciprocals of the frame numbers (8 KiB) in LDS
    __shared__ double tab[3][128];
    __shared__ float rcp_z[PT_FOLD_RCP_N];
    for (int k = (int)threadIdx.x; k < 384; k += 256) {
        int w = k >> 7, i = k & 127;
        tab[w][i] = w == 0 ? pt_pow_logc_tab[i] : w == 1 ? pt_pow_logl_tab[i] : pt_pow_exp2_tab[i];
    }
    {
        // only the frames of this launch (z0 is clamped: frame_begin + threadIdx.x must not pass 2^31 - 1 -- wrapped to a negative
        // k, the loop below ran 8 M times per thread and stored over the pow tables)
        const int z0 = min(P.frame_begin, PT_FOLD_RCP_N), z1 = min(P.frame_begin + P.frame_count, PT_FOLD_RCP_N);
        for (int k = z0 + (int)threadIdx.x; k < z1; k += 256) rcp_z[k] = 1.0f / (float)k;
    }
    __syncthreads();
    const double* LC = tab[0];
    const double* LL = tab[1];
    const double* ET = tab[2];
    // one lane per (pixel, channel): the three channels are independent chains, and
    // a rank's share of a multi-GPU render has too few pixels to fill the chip with one lane per pixel
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid == 0u) {   // (the trace launches that used them have completed: stream order)
        for (int k = 0; k <= PT_QUEUE_SHARDS; ++k) {   // (the shards' counters and the stop word behind them)
            if (P.reset_counter != nullptr) P.reset_counter[k * PT_QUEUE_SHARD_WORDS] = 0u;
            if (P.reset_counter2 != nullptr) P.reset_counter2[k * PT_QUEUE_SHARD_WORDS] = 0u;
        }
    }
    const unsigned lp = tid / 3u, ch = tid - 3u * lp;
    if (lp >= P.npix_local) return;
    float* fbp = reinterpret_cast<float*>(P.fb + lp) + ch;
    PtFoldChain s;
    s.m = 0.0f;
    s.v = 0.0f;
    s.E = 0.0;
    s.l = 0.0;
    s.reg = false;
    int z = P.frame_begin;
    if (z != 0) s.m = *fbp;   // a resumed pixel: its first decode is the literal pow
    const float* radp = P.rad + (size_t)lp * 3u + ch;  // == P.rad + tid: consecutive lanes read consecutive floats
    // (the next frame's radiance is requested before this frame's arithmetic: the chain never waits for memory)
    const size_t stride = (size_t)P.npix_local * 3u;
    float c = P.frame_count > 0 ? radp[0] : 0.0f;
    asm volatile("" : "+v"(c));   // wait for the first value here, not at the loop's head (where the wait would cover every later load too)
    for (int f = 0; f < P.frame_count; ++f, ++z) {
        const float cn = f + 1 < P.frame_count ? radp[(size_t)(f + 1) * stride] : 0.0f;
        __builtin_amdgcn_sched_barrier(0);   // (left alone, hipcc sinks the load to the end of the iteration)
        pt_fold_frame(s, z, c, rcp_z, LC, LL, ET, nullptr);
        c = cn;
    }
    if (P.frame_count > 0) {
        *fbp = s.m;
        if (ch == 0u) reinterpret_cast<float*>(P.fb + lp)[3] = 1.0f;
    }
}

// The short forms against the literal ones, operand by operand (tests/test_gpu_fold_exact.py).  Work-item i of mode
//   0: x = the binary32 with bits first + i: pt_pow_regular(x, 1/2.2f) rounded against pt_pow(x, 1/2.2f)      -> out[0] mismatches
//   1: v = those bits: the decode of the chain after encoding v against pow(pow(v, 1/2.2f), 2.2f)             -> out[1], literal-pow fallbacks out[2]
//   2: numerator mantissa i & 0x7fffff at three exponents, z = first + (i >> 23): pt_fold_div against "/"      -> out[3]
//   4: divisor significand first + i against ALL 2^23 numerator significands: pt_fold_div with pt_rcp_fast against "/"  -> out[3]
//   3: chain i (seed first): 32 frames of arbitrary radiance -- ordinary values over 40 binades, zeros, huge, tiny and
//      subnormal ones, negatives, infinities, NaN -- from frame 0 or resumed at a later frame from an arbitrary pixel:
//      pt_fold_frame against the literal :314-321, every frame's pixel compared                                -> out[5]
// out[4] counts the operands that were checked (modes 0-2: regular ones; the others take the literal operations by construction).
__global__ __launch_bounds__(256) void pt_fold_check_kernel(unsigned long long* __restrict__ out, int mode, unsigned first,
                                                            unsigned long long count)
{
    __shared__ double tab[3][128];
    __shared__ float rcp_z[PT_FOLD_RCP_N];
    for (int k = (int)threadIdx.x; k < 384; k += 256) {
        int w = k >> 7, i = k & 127;
        tab[w][i] = w == 0 ? pt_pow_logc_tab[i] : w == 1 ? pt_pow_logl_tab[i] : pt_pow_exp2_tab[i];
    }
    if (mode == 3)
        for (int k = (int)threadIdx.x; k < PT_FOLD_RCP_N; k += 256) rcp_z[k] = 1.0f / (float)k;
    __syncthreads();
    const double* LC = tab[0];
    const double* LL = tab[1];
    const double* ET = tab[2];
    const float inv_gamma = 1.0f / PTK_GAMMA;
    unsigned bad = 0, slow = 0, seen = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (mode == 0 || mode == 1) {
            const float x = __uint_as_float(first + (unsigned)i);
            if (!pt_pow_is_regular(x)) continue;
            ++seen;
            if (mode == 0) {
                double l;
                const float got = (float)pt_pow_regular(x, inv_gamma, LC, LL, ET, l);
                const float want = pt_pow(x, inv_gamma, LC, LL, ET);
                bad += __float_as_uint(got) != __float_as_uint(want);
            } else {
                PtFoldChain s;
                pt_fold_encode(s, x, true, LC, LL, ET);
                const float got = pt_fold_decode(s, LC, LL, ET, &slow);
                const float want = pt_pow(pt_pow(x, inv_gamma, LC, LL, ET), PTK_GAMMA, LC, LL, ET);
                bad += __float_as_uint(got) != __float_as_uint(want);
            }
        } else if (mode == 3) {
            uint32_t h = pt_hash_u32(first ^ (uint32_t)i) ^ (uint32_t)(i >> 32);
            auto arbitrary = [&](bool pixel) -> float {
                const float u = pt_random_float(h), w = pt_random_float(h);
                const unsigned kind = (unsigned)(pt_random_float(h) * 64.0f);
                const unsigned mant = (unsigned)(w * 8388608.0f) & 0x7fffffu;
                if (kind < 44u) return __uint_as_float(((unsigned)(97.0f + u * 40.0f) << 23) | mant);    // 2^-30 .. 2^10
                if (kind < 50u) return 0.0f;
                if (kind < 53u) return __uint_as_float(((unsigned)(190.0f + u * 64.0f) << 23) | mant);   // 2^63 .. 2^127
                if (kind < 56u) return __uint_as_float(((unsigned)(u * 60.0f) << 23) | mant);            // subnormal .. 2^-67
                if (kind < 58u) return __uint_as_float(((unsigned)(40.0f + u * 20.0f) << 23) | mant);    // around 2^-80
                if (kind < 60u) return __uint_as_float(((unsigned)(200.0f + u * 12.0f) << 23) | mant);   // around 2^80
                if (kind == 60u) return pixel ? 1.0f : -__uint_as_float(((unsigned)(120.0f + u * 10.0f) << 23) | mant);
                if (kind == 61u) return __builtin_inff();
                if (kind == 62u) return pixel ? 0.5f : __builtin_nanf("");
                return __uint_as_float(((unsigned)(126.0f + u * 2.0f) << 23));                           // powers of two near 1
            };
            PtFoldChain s;
            s.m = 0.0f; s.v = 0.0f; s.E = 0.0; s.l = 0.0; s.reg = false;
            float ml = 0.0f;
            int z = 0;
            if (i & 1ull) {
                z = 1 + (int)(pt_random_float(h) * ((i & 2ull) ? 3000.0f : 40.0f));
                s.m = ml = arbitrary(true);
            }
            for (int f = 0; f < 32; ++f, ++z) {
                const float c = arbitrary(false);
                pt_fold_frame(s, z, c, rcp_z, LC, LL, ET, nullptr);
                if (z == 0) ml = pt_pow(c, inv_gamma, LC, LL, ET);
                else {
                    const float zm1 = (float)(z - 1), zf = (float)z;
                    const float o = pt_pow(ml, PTK_GAMMA, LC, LL, ET);
                    ml = pt_pow((o * zm1 + c) / zf, inv_gamma, LC, LL, ET);
                }
                ++seen;
                const bool same = (s.m != s.m && ml != ml) || __float_as_uint(s.m) == __float_as_uint(ml);
                bad += !same;
            }
        } else if (mode == 4) {
            // EVERY pair of significands: divisor 1.b (b = first + i), all 2^23 numerators 1.a; the quotient's significand
            // depends on nothing else while no operand or intermediate leaves the normal range (the callers' guards)
            const float b = __uint_as_float(0x3f800000u | ((first + (unsigned)i) & 0x7fffffu));
            const float y = pt_rcp_fast(b);
            unsigned nb = 0;
            for (unsigned a_m = 0; a_m < 0x800000u; ++a_m) {
                const float a = __uint_as_float(0x3f800000u | a_m);
                nb += __float_as_uint(pt_fold_div(a, b, y)) != __float_as_uint(a / b);
            }
            bad += nb;
            seen += 1u;   // (divisors; x 2^23 numerators each)
        } else {
            const unsigned z = first + (unsigned)(i >> 23);
            const float zf = (float)z, y = 1.0f / zf;
            const unsigned mant = (unsigned)i & 0x7fffffu;
            // the quotient's significand depends on the numerator's significand alone while nothing under- or overflows:
            // the two ends of the regular range and the middle
            const unsigned exps[3] = { __float_as_uint(PTK_POW_REGULAR_MIN), 0x3f800000u, __float_as_uint(PTK_POW_REGULAR_MAX) - 0x00800000u };
            for (int k = 0; k < 3; ++k) {
                const float a = __uint_as_float(exps[k] | mant);
                ++seen;
                bad += __float_as_uint(pt_fold_div(a, zf, y)) != __float_as_uint(a / zf);
            }
        }
    }
    if (mode == 0 && bad) atomicAdd(out + 0, (unsigned long long)bad);
    if (mode == 1 && bad) atomicAdd(out + 1, (unsigned long long)bad);
    if (mode == 1 && slow) atomicAdd(out + 2, (unsigned long long)slow);
    if ((mode == 2 || mode == 4) && bad) atomicAdd(out + 3, (unsigned long long)bad);
    if (mode == 3 && bad) atomicAdd(out + 5, (unsigned long long)bad);
    if (seen) atomicAdd(out + 4, (unsigned long long)seen);
}

// pt_shade's short forms against the literal ones, operand by operand (tests/test_gpu_shade_forms.py).  Work-item i of mode
//   1: x = the binary32 with bits first + i, within 2^-11 of 1: pt_rsqrt_near1(x) against 1.0f / sqrtf(x)                      -> out[1]
//   2: the guarded quotients against "/".  Numerator and divisor binades 2^-61 .. 2^60 -- the window [2^-60, 2^60) and the first
//      binade outside on each side -- in every combination (pair i / PT_SHADE_CHECK_SIGS), PT_SHADE_CHECK_SIGS pairs of
//      significands each: all zeros and all ones in their four combinations, a +0 numerator, arbitrary ones.  pt_div and, where
//      the numerator is what it asks for, pt_div_by; pt_div_pair with a smaller first numerator (the same times a factor in
//      [0, 1]: 0, 1 and arbitrary ones) and a second divisor of an arbitrary binade                                           -> out[2]
//   3: x = those bits, in [2^-60, 1e20]: pt_rcp_fast(x) against 1.0f / x                                                       -> out[3]
// (There is no mode 0: it was the check of a 1 / sqrt for normalize3 seeded by the square-root iteration's h, which cannot be
// exact -- DESIGN.md S3.)  out[4] counts the operands that were checked, out[5] those of mode 2 inside the window (the others take
// the generic division by construction), out[6] is the largest failing operand's bits and out[7] the complement of the smallest's
// (mode 2: the numerator's).
#define PT_SHADE_CHECK_BINADES 122
#define PT_SHADE_CHECK_SIGS 4096
__global__ __launch_bounds__(256) void pt_shade_check_kernel(unsigned long long* __restrict__ out, int mode, unsigned first,
                                                             unsigned long long count)
{
    unsigned bad = 0, seen = 0, inside = 0, worst_hi = 0, worst_lo = 0;
    auto differ = [&](float got, float want, float operand) {
        const bool same = (got != got && want != want) || __float_as_uint(got) == __float_as_uint(want);
        if (!same) {
            ++bad;
            worst_hi = max(worst_hi, __float_as_uint(operand));
            worst_lo = max(worst_lo, ~__float_as_uint(operand));
        }
    };
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        if (mode == 1) {
            const float x = __uint_as_float(first + (unsigned)i);
            if (!pt_is_near1(x)) continue;
            ++seen;
            differ(pt_rsqrt_near1(x), 1.0f / __builtin_sqrtf(x), x);
        } else if (mode == 3) {
            const float x = __uint_as_float(first + (unsigned)i);
            if (!(x >= 0x1p-60f && x <= PTK_RCP_FAST_MAX)) continue;
            ++seen;
            differ(pt_rcp_fast(x), 1.0f / x, x);
        } else {
            const unsigned pair = (unsigned)(i / PT_SHADE_CHECK_SIGS), k = (unsigned)(i % PT_SHADE_CHECK_SIGS);
            if (pair >= PT_SHADE_CHECK_BINADES * PT_SHADE_CHECK_BINADES) continue;
            const unsigned ea = 127u - 61u + pair / PT_SHADE_CHECK_BINADES, eb = 127u - 61u + pair % PT_SHADE_CHECK_BINADES;
            uint32_t h = pt_hash_u32(first ^ (uint32_t)i);
            const unsigned ma = (unsigned)(pt_random_float(h) * 8388608.0f) & 0x7fffffu;
            const unsigned mb = (unsigned)(pt_random_float(h) * 8388608.0f) & 0x7fffffu;
            const unsigned mb2 = (unsigned)(pt_random_float(h) * 8388608.0f) & 0x7fffffu;
            const unsigned eb2 = 127u - 61u + (unsigned)(pt_random_float(h) * (float)PT_SHADE_CHECK_BINADES) % PT_SHADE_CHECK_BINADES;
            const float c = (k & 7u) == 5u ? 1.0f : (k & 7u) == 6u ? 0.0f : pt_random_float(h);
            float a = __uint_as_float((ea << 23) | (k == 0u || k == 2u ? 0u : k == 1u || k == 3u ? 0x7fffffu : ma));
            const float b = __uint_as_float((eb << 23) | (k == 0u || k == 3u ? 0u : k == 1u || k == 2u ? 0x7fffffu : mb));
            const float b2 = __uint_as_float((eb2 << 23) | mb2);
            if (k == 4u) a = 0.0f;
            const bool a_in = pt_div_in_window(__float_as_uint(a)), b_in = pt_div_in_window(__float_as_uint(b));
            ++seen;
            inside += a_in && b_in;
            differ(pt_div(a, b), a / b, a);
            if (a_in || k == 4u) differ(pt_div_by(a, b), a / b, a);
            const float a0 = a * c;
            float q0, q1;
            pt_div_pair(a0, b, a, b2, q0, q1);
            differ(q0, a0 / b, a);
            differ(q1, a / b2, a);
        }
    }
    if (bad) {
        atomicAdd(out + (mode == 1 ? 1 : mode == 3 ? 3 : 2), (unsigned long long)bad);
        atomicMax(out + 6, (unsigned long long)worst_hi);
        atomicMax(out + 7, (unsigned long long)worst_lo);
    }
    if (seen) atomicAdd(out + 4, (unsigned long long)seen);
    if (inside) atomicAdd(out + 5, (unsigned long long)inside);
}

// the masked search's list builder (pt_pair_list_build) and the rounds' lane mapping (pt_tail_get, as pt_tail_round reads the ring) on
// masks the caller gives: one wave of 64 lanes per case, masks[case * 64 + lane] = that lane's two words (the high one counts where
// ntri > 32, as in pt_intersect_masked).  out[case * (2 + cap)]: the pairs the rounds would test, then the rounds, then the pairs
// themselves (triangle << 6 | ray lane) in the order tested, the first `cap` of them.  The ring is the search's: PT_TAIL_LIST pairs of 2 bytes.
__global__ __launch_bounds__(64) void pt_pair_check_kernel(const uint2* __restrict__ masks, unsigned* __restrict__ out, int ntri, unsigned cap)
{
    __shared__ __attribute__((aligned(4))) unsigned short ring[PT_TAIL_LIST];
    const unsigned lane = pt_lane_id();
    PtTail tl;
    tl.keys = nullptr;
    tl.list = (pt_lds_u32*)ring;
    tl.wr = tl.rd = 0u;
    tl.kbest = ~0ull; tl.ku = tl.kv = 0.0f;
    tl.tile = 0u;
    const uint2 pm = masks[(size_t)blockIdx.x * 64u + lane];
    unsigned* const o = out + (size_t)blockIdx.x * (2u + cap);
    unsigned n_out = 0u, rounds = 0u;
    auto round = [&](unsigned cnt) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane < cnt && n_out + lane < cap) o[2u + n_out + lane] = pt_tail_get<1>(tl, (tl.rd + lane) & (PT_TAIL_LIST - 1u));
        n_out += cnt;
        tl.rd += cnt;
        ++rounds;
    };
    pt_pair_list_build<1>(pm.x, ntri > 32 ? pm.y : 0u, ntri, tl, lane, round);
    if (tl.wr != tl.rd) round(tl.wr - tl.rd);   // (pt_pass2_finish)
    if (lane == 0u) { o[0] = n_out; o[1] = rounds; }
}

// the masked search ITSELF -- pt_intersect_masked<true, 1>, the trace kernel's call: own steps, list, rounds, merge -- on rays and masks
// the caller gives: one wave of 64 lanes per case, workgroups of the trace kernel's size whose waves share ONE LDS triangle table and
// hold a tail each, as there (the layout of the brute-force query kernel: pt_lds_*, POOLS = false).  rays[2 (case * 64 + lane)] =
// origin xyz and an alive word (bits, 0 = a lane without a ray), then direction xyz -- handed to the search as it is -- and a word not
// read; masks[case * 64 + lane] = the lane's two words (lo: bit nlo-1-j <-> triangle j, hi: bit ntri-33-j <-> triangle 32+j).  Bits of
// triangles the scene does not have are dropped here: no table holds one, and they would index past the records; a high word at 32
// triangles or fewer goes in as it is -- the search must not read it.  out[2 (case * 64 + lane)] = {hidx, t, hu, hv} (bits), then the
// search's step count and three zeros.
__global__ __launch_bounds__(PT_TRACE_THREADS) void pt_search_check_kernel(const PtPrepTriangle* __restrict__ tris, int ntri, const float4* __restrict__ rays,
                                                                          const uint2* __restrict__ masks, uint4* __restrict__ out, unsigned cases)
{
    const unsigned lane = pt_lane_id();
    pt_lds_table_load(tris, ntri);
    __syncthreads();
    PtTail tl = pt_tail_init((pt_lds_u32*)pt_lds_tab + pt_lds_tails<1, false>(ntri) + pt_wave_in_wg() * pt_lds_tail_dw<1>(), 0u, lane);
    const unsigned c = pt_wave();
    if (c >= cases) return;   // (wave-uniform, behind the workgroup's only barrier)
    const size_t i = (size_t)c * 64u + lane;
    const float4 ro = rays[2 * i], rd = rays[2 * i + 1];
    uint2 pm = masks[i];
    const int nlo = ntri < 32 ? ntri : 32, nhi = ntri - 32;
    pm.x &= 0xFFFFFFFFu >> (32 - nlo);
    if (nhi > 0) pm.y &= 0xFFFFFFFFu >> (32 - nhi);
    float tmax = 1e20f, hu = 0.0f, hv = 0.0f;
    int hidx = -1;
    const unsigned steps = pt_intersect_masked<true, 1>((pt_const_f32p)(const float*)tris, tris, ntri, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z),
                                                        __float_as_uint(ro.w) != 0u, tmax, hu, hv, hidx, pm, tl, lane);
    out[2 * i] = make_uint4((unsigned)hidx, __float_as_uint(tmax), __float_as_uint(hu), __float_as_uint(hv));
    out[2 * i + 1] = make_uint4(steps, 0u, 0u, 0u);
}

// ------------------------------------------------------------------------------------------
// multi-GPU assembly, output stage, shim smoke-test kernel
// ------------------------------------------------------------------------------------------
__global__ void pt_assemble_kernel(const float4* __restrict__ gathered, float4* __restrict__ image, int width,
                                   int height, int stripe_rows, int n_ranks, int slab_rows)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)width * height;
    if (i >= total) return;
    unsigned row = (unsigned)(i / (unsigned)width);
    unsigned x = (unsigned)(i - (size_t)row * width);
    unsigned stripe = row / (unsigned)stripe_rows;
    unsigned within = row - stripe * (unsigned)stripe_rows;
    unsigned rank = stripe % (unsigned)n_ranks;
    unsigned sl = stripe / (unsigned)n_ranks;
    size_t src = ((size_t)rank * slab_rows + (size_t)sl * stripe_rows + within) * width + x;
    image[i] = gathered[src];
}

// f2c(sqrtf(v)) of test/RaytraceTest.cpp:78-83,280-285: a *= 255; min((int)a, 255)
PTK_DEV int32_t pt_f2c(float v)
{
    float a = __builtin_sqrtf(v) * 255.0f;
    int32_t i;
    if (a != a) i = (int32_t)0x80000000;        // (int)NaN on the reference's x86 host
    else if (a >= 2147483648.0f) i = (int32_t)0x80000000;  // cvttss2si overflow value
    else if (a <= -2147483648.0f) i = (int32_t)0x80000000;
    else i = (int32_t)a;
    return i < 255 ? i : 255;
}

__global__ void pt_tonemap_kernel(const float4* __restrict__ fb, int32_t* __restrict__ rgb, size_t npix)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    float4 v = fb[i];
    rgb[3 * i + 0] = pt_f2c(v.x);
    rgb[3 * i + 1] = pt_f2c(v.y);
    rgb[3 * i + 2] = pt_f2c(v.z);
}

// PTSPEC transcendentals on arrays, for direct device-vs-oracle parity tests:
// out[4i] = sin(in[i]), cos(in[i]), pow(in[i], 2.2f), pow(in[i], 1/2.2f)
__global__ void pt_math_kernel(const float* __restrict__ in, float* __restrict__ out, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = in[i];
    float s = 0.0f, c = 0.0f;
    if (x >= 0.0f && x <= 1.0e6f) pt_sincos(x, s, c);  // PTSPEC defines sin/cos for phi >= 0 (binary32 path on [0, 2 pi])
    out[4 * i + 0] = s;
    out[4 * i + 1] = c;
    out[4 * i + 2] = pt_pow(x, PTK_GAMMA, pt_pow_logc_tab, pt_pow_logl_tab, pt_pow_exp2_tab);
    out[4 * i + 3] = pt_pow(x, 1.0f / PTK_GAMMA, pt_pow_logc_tab, pt_pow_logl_tab, pt_pow_exp2_tab);
}

__global__ void pt_fill_i32_kernel(int32_t* dst, int32_t value, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = value;
}

// ------------------------------------------------------------------------------------------
// batched ray queries (pt_intersect_rays, pt_camera_rays)
// ------------------------------------------------------------------------------------------
// A query ray is the pair of arguments of getRay (GenerateColors.cl:73-77): the direction is normalised here as getRay does it,
// the search is the renderer's own (pt_intersect_two_pass over the prepared scene, or the big-triangle table and then the LBVH:
// pt_bvh_step / pt_bvh_round), and the HitRecord (:126-130) is pt_shade's deferred one.  Nothing here is new arithmetic.
// The caller's tmax (pt_ray::tmax) starts the search in place of the reference's 1e20 (:141): a hit counts at
// 0 < t < min(tmax, 1e20); a tmax that is NaN or <= 0 searches nothing and misses.  Strictness: pass 2 and the tail merge of the
// two-pass search compare t < tmax as the reference does, but the LBVH's ring keeps a 64-bit (t, index) minimum whose incumbent is
// (tmax, no triangle) -- a candidate AT tmax beats that key.  The renderer never meets it (its tmax is 1e20, which the exact
// test already excludes); a query does, so the result is taken as a hit only when t < tmax as well (pt_query_store).  The
// minimum over {t <= tmax} is below tmax exactly when the reference's strict winner exists, and then it is that winner.
struct PtQueryRay {
    f3 o, d;      // origin, normalize(dir) (:75)
    float tlim;   // min(tmax, 1e20); 0 when the ray is not live, so that no t counts
    bool live;    // tmax > 0 (false for NaN): the search runs
};

PTK_DEV PtQueryRay pt_query_load(const float4* rays, unsigned i)
{
    const float4 a = rays[2 * (size_t)i], b = rays[2 * (size_t)i + 1];   // origin xyz tmax | dir xyz reserved
    PtQueryRay r;
    r.o = mk3(a.x, a.y, a.z);
    r.d = normalize3(mk3(b.x, b.y, b.z));
    r.live = a.w > 0.0f;
    r.tlim = !r.live ? 0.0f : (a.w < 1e20f ? a.w : 1e20f);
    return r;
}

PTK_DEV PtQueryRay pt_query_idle()   // what a lane without a ray holds
{
    PtQueryRay r;
    r.o = mk3(0.0f, 0.0f, 0.0f); r.d = mk3(0.0f, 0.0f, 1.0f);
    r.tlim = 0.0f; r.live = false;
    return r;
}

// pt_shade's deferred HitRecord (:127-130) of the hit (t, u, v) of the ray (o, d) on triangle hidx: the point and the normal;
// returns the triangle's id field, as stored
PTK_DEV float pt_hit_record(const PtPrepTriangle* tris, int hidx, const f3& o, const f3& d, float t, float u, float v, f3& p, f3& n)
{
    const float4 nid = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(tris + hidx) + 12);
    const f3 N = mk3(nid.x, nid.y, nid.z);
    p = add3(o, scale3(d, t));
    const float w = 1.0f - u - v;
    n = normalize3(add3(add3(scale3(N, u), scale3(N, v)), scale3(N, w)));
    return nid.w;
}

// result i: a pt_hit (three 16-byte stores) or, for occlusion queries, 1 / 0
PTK_DEV void pt_query_store(const PtQueryParams& Q, unsigned i, const PtQueryRay& r, float t, float u, float v, int hidx)
{
    const bool hit = (hidx >= 0) & (t < r.tlim);
    if (Q.occluded) {
        reinterpret_cast<int32_t*>(Q.out)[i] = hit ? 1 : 0;
        return;
    }
    float4* o = reinterpret_cast<float4*>(Q.out) + 3 * (size_t)i;
    if (!hit) {
        o[0] = make_float4(__builtin_inff(), __int_as_float(-1), 0.0f, 0.0f);
        o[1] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
        o[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    f3 p, n;
    const float id = pt_hit_record(Q.t.tris, hidx, r.o, r.d, t, u, v, p, n);
    o[0] = make_float4(t, __int_as_float(hidx), u, v);
    o[1] = make_float4(p.x, p.y, p.z, id);   // material
    o[2] = make_float4(n.x, n.y, n.z, 0.0f);
}

// What a brute-force query / AO workgroup holds in LDS before its search: the table (LDS_TABLE 1), the waves' pass-2 tails, their record
// tiles (LDS_TABLE 2) -- the trace kernel's layout without the pools of parked paths (pt_lds_*, POOLS = false).  Returns this wave's tail.
template <int LDS_TABLE>
PTK_DEV PtTail pt_table_wg_setup(const PtTraceParams& P, unsigned lane)
{
    if (LDS_TABLE == 1) {
        pt_lds_table_load(P.tris, P.ntri);
        __syncthreads();
    }
    const unsigned wave_in_wg = pt_wave_in_wg();
    return pt_tail_init((pt_lds_u32*)pt_lds_tab + pt_lds_tails<LDS_TABLE, false>(P.ntri) + wave_in_wg * pt_lds_tail_dw<LDS_TABLE>(),
                        pt_lds_tiles<LDS_TABLE, false>(P.ntri) + wave_in_wg * PT_LDS_TILE_DW, lane);
}

// brute force: one wave = 64 consecutive rays, one search (the search is wave-uniform over the triangles: every lane finishes
// together, so there is nothing to refill)
template <bool DET_BOUNDED, int LDS_TABLE, int QUADS>
__global__ __launch_bounds__(PT_TRACE_THREADS) void pt_query_kernel(const PtQueryParams Q)
{
    const PtTraceParams& P = Q.t;
    const unsigned lane = pt_lane_id();
    const int ntri = P.ntri;
    PtTail tl = pt_table_wg_setup<LDS_TABLE>(P, lane);
    const unsigned i = pt_wave() * 64u + lane;
    const bool act = i < Q.nrays;
    const PtQueryRay r = act ? pt_query_load(Q.rays, i) : pt_query_idle();
    float tmax = r.tlim, hu = 0.0f, hv = 0.0f;
    int hidx = -1;
    // (the filter's anchor is the table's, P.cam.eye: a ray far from it fails the tame check and keeps every triangle)
    pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, r.o, r.d, r.live, tmax, hu, hv, hidx,
                                                         P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi,
                                                         mk3(P.cam.eye[0], P.cam.eye[1], P.cam.eye[2]), tl, lane);
    if (act) pt_query_store(Q, i, r, tmax, hu, hv, hidx);
}

// ---- the persistent LBVH search driver (pt_query_bvh_kernel, pt_ao_bvh_kernel) -----------------------------------------------
// A persistent grid over n work items: wave w takes the groups of 64 consecutive items w, w + W, w + 2W ... (W = the grid's
// waves).  Its cursor is wave-uniform: [next, gend) is what is left of the wave's current group; groups start at multiples of 64.
struct PtWorkCursor { unsigned next, gend, stride, n; };

PTK_DEV PtWorkCursor pt_cursor_init(unsigned n)
{
    PtWorkCursor c;
    c.n = n;
    c.stride = gridDim.x * (PT_TRACE_THREADS / 64) * 64u;
    c.next = pt_wave() * 64u;
    c.gend = c.next + 64u < n ? c.next + 64u : n;
    return c;
}

// the lanes without an item take the wave's next ones, in order (the lane of rank r among them: item next + r -- neighbours get
// neighbouring rays); true for a lane that got one, which is alive from then on
PTK_DEV bool pt_cursor_take(PtWorkCursor& c, bool& alive, unsigned& item)
{
    bool got = false;
    for (unsigned long long need = __ballot(!alive); need != 0ull && c.next < c.n; need = __ballot(!alive)) {
        const unsigned n_need = (unsigned)__popcll(need), avail = c.gend - c.next;
        const unsigned take = n_need < avail ? n_need : avail;
        const unsigned rank = pt_mbcnt(need);
        if (!alive && rank < take) {
            item = c.next + rank;
            alive = got = true;
        }
        c.next += take;
        if (c.next == c.gend) {   // the wave's next group
            c.next = ((c.gend - 1u) & ~63u) + c.stride;
            c.next = c.next < c.n ? c.next : c.n;
            c.gend = c.next + 64u < c.n ? c.next + 64u : c.n;
        }
    }
    return got;
}

// The loop of a persistent LBVH kernel.  Like the LBVH trace kernel it steps all traversing lanes together and, as soon as no more
// than PT_BVH_REFILL of them still traverse, refills: the lanes whose search has ended hand it to their work (next_ray), which may
// go on with another ray of the same item; the free ones take the wave's next items (begin); all of them start their searches
// while the stragglers keep theirs, so that a wave does not wait for its slowest ray.  Its LDS is the trace kernel's (pt_bvh_lds_*).
// Work, per lane:  n            the launch's items (uniform)
//                  begin(item)  the lane takes an item: its first ray
//                  next_ray(L)  the search of the current ray has ended with L: keep the result; true = the item has another ray
//                  org(), dir(), limit(), live()   the current ray, its tmax, whether it searches anything at all
//                  ANY, any()   some searches are any-hit ones (pt_bvh_round) / the current one is
template <bool DET_BOUNDED, int BIGQ, class Work>
PTK_DEV void pt_bvh_drive(const PtTraceParams& P, Work& W)
{
    const unsigned lane = pt_lane_id();
    const unsigned n_recs = (unsigned)P.bvh_records;
    const pt_lds_u8* nxt = pt_bvh_wg_setup(P);
    pt_lds_u32* stk = (pt_lds_u32*)pt_lds_tab + pt_bvh_lds_stacks() + threadIdx.x;
    unsigned ovf[2 * (PT_BVH_STACK - PT_BVH_LDS_STACK)];
    PtTail tl = pt_tail_init((pt_lds_u32*)pt_lds_tab + pt_bvh_lds_tails() + (threadIdx.x >> 6) * PT_BVH_TAIL_DW, 0u, lane);
    PtWorkCursor c = pt_cursor_init(W.n);
    bool alive = false;   // the lane holds an item that is not finished
    bool trav = false;    // ... and the search of its current ray is in progress
    PtBvhLane L = pt_bvh_lane_idle(0.0f);

    for (;;) {
        if ((unsigned)__popcll(__ballot(trav)) <= (unsigned)PT_BVH_REFILL) {
            // the pending pairs first: a lane with no nodes left has its result only once its leaves are tested
            if (tl.wr != tl.rd) pt_bvh_round<DET_BOUNDED, Work::ANY>(P, L, tl, tl.wr - tl.rd, lane, W.org(), W.dir(), n_recs, W.any());
            bool fresh = false;   // the lane has a new ray
            if (alive && !trav) alive = fresh = W.next_ray(L);
            unsigned item = 0u;
            if (pt_cursor_take(c, alive, item)) {
                W.begin(item);
                fresh = true;
            }
            // every fresh lane drops the previous ray's result (a fresh ray that searches nothing ends as a miss at the next refill)
            if (fresh) pt_bvh_lane_clear(L, W.limit());
            pt_bvh_search_start<DET_BOUNDED, BIGQ>(P, L, trav, fresh && W.live(), W.any(), W.org(), W.dir(), tl, lane);
            if (__ballot(alive) == 0ull) break;
        }
        pt_bvh_step<DET_BOUNDED, Work::ANY>(P, L, trav, W.org(), W.dir(), stk, ovf, nxt, tl, lane, n_recs, W.any());
    }
}

// pt_intersect_rays / pt_occluded_rays through the LBVH: one item = one ray.  ANYHIT: every search is an any-hit one
// (pt_occluded_rays: the search stops at the first accepted triangle) and the result is PT_QUERY_OCCLUDED's 1 / 0.
template <bool ANYHIT>
struct PtQueryWork {
    static constexpr bool ANY = ANYHIT;
    const PtQueryParams& Q;
    unsigned n, ray;
    PtQueryRay r;
    PTK_DEV void begin(unsigned item) { ray = item; r = pt_query_load(Q.rays, item); }
    PTK_DEV bool next_ray(const PtBvhLane& L)
    {
        // Two rules, each where it belongs.  A closest search's ring lets a candidate exactly AT tmax beat the incumbent (tmax, no
        // triangle), so its hit counts only at t < tlim as well: pt_query_store.  An any-hit lane's L.tmax never shrinks -- it
        // stays at the ray's limit, where that comparison would turn every hit into a miss -- and pt_bvh_round has compared
        // strictly already: its result is L.hidx >= 0 alone.
        if (ANYHIT) reinterpret_cast<int32_t*>(Q.out)[ray] = L.hidx >= 0 ? 1 : 0;
        else pt_query_store(Q, ray, r, L.tmax, L.hu, L.hv, L.hidx);
        return false;
    }
    PTK_DEV const f3& org() const { return r.o; }
    PTK_DEV const f3& dir() const { return r.d; }
    PTK_DEV float limit() const { return r.tlim; }
    PTK_DEV bool live() const { return r.live; }
    PTK_DEV bool any() const { return ANYHIT; }
};

template <bool DET_BOUNDED, int BIGQ, bool ANYHIT>
__global__ __launch_bounds__(PT_TRACE_THREADS) PT_BVH_WAVES_ATTR
void pt_query_bvh_kernel(const PtQueryParams Q)
{
    PtQueryWork<ANYHIT> W = { Q, Q.nrays, 0u, pt_query_idle() };
    pt_bvh_drive<DET_BOUNDED, BIGQ>(Q.t, W);
}

// ray gid of frame `frame` as the renderer traces it (seed :305-308, pixel jitter, the camera's expression), with the direction
// getRay receives at :287 -- a query normalises it once more, as getRay does, and traces the renderer's primary ray bit for bit
__global__ __launch_bounds__(256) void pt_camera_rays_kernel(const PtLensCamera cam, int width, unsigned npix, float inv_w, float inv_h, float aspect,
                                                             int frame, float4* __restrict__ rays)
{
    const unsigned gid = blockIdx.x * 256u + threadIdx.x;
    if (gid >= npix) return;
    uint32_t seed = gid + pt_hash_u32((uint32_t)frame);
    const unsigned y = gid / (unsigned)width, x = gid - y * (unsigned)width;
    float fx, fy;
    pt_pixel_jitter((int)x, (int)y, seed, fx, fy);
    f3 org, aim;
    if (cam.lens_radius > 0.0f) pt_lens_aim(fx, fy, inv_w, inv_h, aspect, PT_CAM_K(cam), cam.lens_radius, cam.focus_distance, seed, org, aim);
    else pt_camera_aim(fx, fy, inv_w, inv_h, aspect, PT_CAM_K(cam), org, aim);
    rays[2 * (size_t)gid] = make_float4(org.x, org.y, org.z, 1e20f);
    rays[2 * (size_t)gid + 1] = make_float4(aim.x, aim.y, aim.z, 0.0f);
}

// ------------------------------------------------------------------------------------------
// ambient occlusion (pt_render_ao)
// ------------------------------------------------------------------------------------------
// One work item is one sample (local pixel lp, frame f0 + j / npix): the renderer's primary ray (seed :308, pt_generate_ray), its
// closest hit from tmax 1e20 (:141); on a hit, K occlusion rays getRay(p + wi 0.01, wi) (:257) with wi = sampleHemisphereCosine
// (n, &seed) (:161-172) about the HitRecord normal turned to face the ray (:243), each an any-hit search at 0 < t < min(radius, 1e20).
// counts[lp] += open | hits << 32: hits = 1 for a primary hit, open = the occlusion rays that hit nothing.

// the start of sample `item` of a frame-major launch over npix local pixels from frame frame0 on (item = f * npix + local pixel): its
// local pixel and its primary ray (pt_sample_begin's seed and camera ray) -- ambient occlusion and direct illumination alike
PTK_DEV void pt_item_begin(const PtTraceParams& P, const PtLensCamera& cam, unsigned npix, int frame0, unsigned item, unsigned& lp, uint32_t& seed,
                           f3& o, f3& d)
{
    const unsigned f = item / npix;
    lp = item - f * npix;
    unsigned x, grow;
    pt_pixel_xy<false>(P, nullptr, lp, x, grow);
    const unsigned gid = grow * (unsigned)P.width + x;
    seed = gid + pt_hash_u32((uint32_t)(frame0 + (int)f));
    pt_generate_lens_ray((int)x, (int)grow, P.inv_width, P.inv_height, P.aspect, cam, seed, o, d);
}

PTK_DEV void pt_ao_begin(const PtAoParams& A, unsigned item, unsigned& lp, uint32_t& seed, f3& o, f3& d)
{
    pt_item_begin(A.t, A.cam, A.npix, A.frame0, item, lp, seed, o, d);
}

// the primary hit's point and normal: the HitRecord's, turned to face the ray as at :243
PTK_DEV void pt_ao_surface(const PtTraceParams& P, const f3& o, const f3& d, float t, float hu, float hv, int hidx, f3& p, f3& n)
{
    pt_hit_record(P.tris, hidx, o, d, t, hu, hv, p, n);
    n = dot3(n, d) < 0.0f ? n : scale3(n, -1.0f);
}

// occlusion ray k of the sample: wi = sampleHemisphereCosine(n, &seed) (:161-172: phi, then sinThetaSqr -- pt_shade's diffuse
// branch), the ray getRay(p + wi 0.01, wi) (:257)
PTK_DEV void pt_ao_ray(const f3& p, const f3& n, uint32_t& seed, f3& o, f3& d)
{
    const float phi = PTK_TWO_PI * pt_random_float(seed);
    const float xi = pt_random_float(seed);
    float sp, cp;
    pt_sincos(phi, sp, cp);
    const f3 axis = __builtin_fabsf(n.x) > 0.001f ? mk3(0.0f, 1.0f, 0.0f) : mk3(1.0f, 0.0f, 0.0f);
    const f3 tv = normalize3(cross3(axis, n));
    const f3 sv = cross3(n, tv);
    const float cosTheta = pt_sqrt(1.0f - xi);
    const float sinTheta = pt_sqrt(xi);
    const f3 a = scale3(scale3(sv, cp), sinTheta);
    const f3 b = scale3(scale3(tv, sp), sinTheta);
    const f3 c = scale3(n, cosTheta);
    const f3 wi = normalize3(add3(add3(a, b), c));
    o = add3(p, scale3(wi, 0.01f));
    d = normalize3(wi);
}

PTK_DEV void pt_ao_count(const PtAoParams& A, unsigned lp, unsigned hits, unsigned open)
{
    if (hits | open)
        __hip_atomic_fetch_add(A.counts + lp, (unsigned long long)open | ((unsigned long long)hits << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// brute force: one wave = 64 consecutive samples; the primary search, then the K occlusion rays of the lanes that hit, all in step
// (the search is wave-uniform over the triangles: pt_query_kernel)
template <bool DET_BOUNDED, int LDS_TABLE, int QUADS>
__global__ __launch_bounds__(PT_TRACE_THREADS) void pt_ao_kernel(const PtAoParams A)
{
    const PtTraceParams& P = A.t;
    const unsigned lane = pt_lane_id();
    const int ntri = P.ntri;
    PtTail tl = pt_table_wg_setup<LDS_TABLE>(P, lane);
    const f3 anchor = mk3(P.cam.eye[0], P.cam.eye[1], P.cam.eye[2]);
    const unsigned item = pt_wave() * 64u + lane;
    const bool act = item < A.nitems;
    unsigned lp = 0u;
    uint32_t seed = 0u;
    f3 o = mk3(0.0f, 0.0f, 0.0f), d = mk3(0.0f, 0.0f, 1.0f);
    if (act) pt_ao_begin(A, item, lp, seed, o, d);
    float tmax = 1e20f, hu = 0.0f, hv = 0.0f;
    int hidx = -1;
    pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, act, tmax, hu, hv, hidx,
                                                         P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
    const bool hit = act & (hidx >= 0);
    if (__ballot(hit) == 0ull) return;
    f3 p = o, n = d;
    if (hit) pt_ao_surface(P, o, d, tmax, hu, hv, hidx, p, n);
    unsigned open = 0u;
    for (int k = 0; k < A.K; ++k) {
        if (hit) pt_ao_ray(p, n, seed, o, d);
        float t = A.tlim, su = 0.0f, sv = 0.0f;
        int sidx = -1;
        pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, hit, t, su, sv, sidx,
                                                             P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
        open += (hit & !((sidx >= 0) & (t < A.tlim))) ? 1u : 0u;   // pt_query_store's occlusion test
    }
    if (hit) pt_ao_count(A, lp, 1u, open);
}

// LBVH (pt_bvh_drive): one item = one sample; the lane runs its searches one after the other -- the primary ray's closest search,
// then its occlusion rays' any-hit searches -- and is free when the sample is counted
struct PtAoWork {
    static constexpr bool ANY = true;
    const PtAoParams& A;
    unsigned n;
    int k;           // the current ray: -1 = the primary, 0 .. K-1 = occlusion ray k
    unsigned lp, open;
    uint32_t seed;
    f3 o, d, p, nrm;
    PTK_DEV void begin(unsigned item)
    {
        pt_ao_begin(A, item, lp, seed, o, d);
        k = -1;
        open = 0u;
    }
    PTK_DEV bool next_ray(const PtBvhLane& L)
    {
        if (k < 0) {
            if (L.hidx < 0) return false;   // a primary miss adds nothing
            pt_ao_surface(A.t, o, d, L.tmax, L.hu, L.hv, L.hidx, p, nrm);
        } else {
            open += L.hidx < 0 ? 1u : 0u;   // (an any-hit search: L.hidx >= 0 alone says occluded, PtQueryWork::next_ray)
        }
        if (++k < A.K) {
            pt_ao_ray(p, nrm, seed, o, d);
            return true;
        }
        pt_ao_count(A, lp, 1u, open);
        return false;
    }
    PTK_DEV const f3& org() const { return o; }
    PTK_DEV const f3& dir() const { return d; }
    PTK_DEV float limit() const { return k < 0 ? 1e20f : A.tlim; }
    PTK_DEV bool live() const { return true; }
    PTK_DEV bool any() const { return k >= 0; }
};

template <bool DET_BOUNDED, int BIGQ>
__global__ __launch_bounds__(PT_TRACE_THREADS) PT_BVH_WAVES_ATTR
void pt_ao_bvh_kernel(const PtAoParams A)
{
    const f3 o0 = mk3(0.0f, 0.0f, 0.0f), d0 = mk3(0.0f, 0.0f, 1.0f);
    PtAoWork W = { A, A.nitems, -1, 0u, 0u, 0u, o0, d0, o0, d0 };
    pt_bvh_drive<DET_BOUNDED, BIGQ>(A.t, W);
}

// image[i] = (a, a, a, 1), a = open / (K hits) (each converted to float, then one IEEE division), miss_value for a pixel never hit
__global__ __launch_bounds__(256) void pt_ao_resolve_kernel(const uint2* __restrict__ counts, float4* __restrict__ image, unsigned npix,
                                                            unsigned K, float miss_value)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npix) return;
    const uint2 c = counts[i];
    const float a = c.y > 0u ? (float)c.x / (float)(K * c.y) : miss_value;
    image[i] = make_float4(a, a, a, 1.0f);
}

// ------------------------------------------------------------------------------------------
// direct illumination (pt_render_direct)
// ------------------------------------------------------------------------------------------
// One work item is one sample, as for ambient occlusion (pt_item_begin): the renderer's primary ray and its closest hit from tmax
// 1e20; a miss stores the background (:235).  On a hit, K light samples on the same seed (include/pt_shim.h states every expression
// and its order): three uniforms, a light triangle of the list, a point on it, the BRDF value at the direction to it (pt_shade's
// expressions for f, not its sampling), the geometry term, and a shadow ray getRay(p + wi 0.01, wi) (:257) that an any-hit search
// at 0 < t < min(dist - 0.02, 1e20) finds occluded or open.  samples[item] = max(E + S / K, 0), 12 bytes; pt_fold_kernel folds them.
// Between the rays of a sample a lane holds the surface (p, n, wo), the hit's material INDEX -- the material is gathered again
// per light sample and for E, which costs a load and saves eight registers across the searches -- the sum S and the contribution
// c that the ray under way decides about.

typedef float pt_f3v __attribute__((ext_vector_type(3), aligned(4)));   // (records are 12 bytes apart)

PTK_DEV void pt_direct_store(const PtDirectParams& D, unsigned item, const f3& L)
{
    pt_f3v v;
    v.x = L.x; v.y = L.y; v.z = L.z;
    *reinterpret_cast<pt_f3v*>(D.samples + (size_t)item * 3u) = v;
}

// a 64-byte record's 16 bytes at byte offset `off`: a 32-bit per-lane offset against the wave-uniform base (pt_shade's gathers; the
// host keeps ntri * 64 and nmat * 64 below 2^32)
PTK_DEV float4 pt_rec16(const void* base, unsigned index, unsigned off)
{
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + (size_t)(index * 64u + off));
}

PTK_DEV unsigned pt_clamp_index(int v, int n)   // into [0, n - 1], n >= 1: never an out-of-range load
{
    v = v < 0 ? 0 : v;
    return (unsigned)(v > n - 1 ? n - 1 : v);
}

// the primary hit: the HitRecord's point and normal, the normal turned to face the ray (:243), wo = -d, the material's index
// clamped as pt_shade clamps it
PTK_DEV void pt_direct_surface(const PtDirectParams& D, const f3& o, const f3& d, float t, float hu, float hv, int hidx, f3& p, f3& n, f3& wo,
                               unsigned& mid)
{
    const float id = pt_hit_record(D.t.tris, hidx, o, d, t, hu, hv, p, n);
    n = dot3(n, d) < 0.0f ? n : scale3(n, -1.0f);
    wo = neg3(d);
    mid = pt_clamp_index(__float_as_int(id), D.t.nmat);
}

// THE kind of a lit kernel (pt_kernels.h: ptk_lit_kind): the one kind parameter of every lit template, its bits by name, and which of
// them go together -- the two predicates of pt_kernels.h, so that no template can be instantiated for a kind that does not exist
template <unsigned KIND> struct PtKindOf {
    static constexpr PtLitKind k = ptk_lit_kind_of(KIND);
    static constexpr bool indirect = k.indirect, mis = k.mis, power = k.power, rr = k.rr, list = k.list, ris = k.ris, env = k.env;
    static constexpr bool rays = (KIND & PT_LIT_KIND_INDICES) != 0;
    static_assert(ptk_lit_valid(KIND), "not a kind of lit render (ptk_lit_kind_valid, ptk_lit_rays_valid)");
    // (never called) its return type is the kind's parameter block: the table of pt_kernels.h from its last row up
    static auto block()
    {
        if constexpr (rays) return PtIndirectRaysParams();
        else if constexpr (env) return std::conditional_t<indirect, PtIndirectEnvParams, PtDirectEnvParams>();
        else if constexpr (ris) return std::conditional_t<indirect, PtIndirectRisParams, PtDirectRisParams>();
        else if constexpr (list) return PtIndirectListParams();
        else if constexpr (rr) return PtIndirectRrParams();
        else if constexpr (power) return std::conditional_t<indirect, PtIndirectPowerParams, PtDirectPowerParams>();
        else if constexpr (mis) return PtIndirectMisParams();
        else return std::conditional_t<indirect, PtIndirectParams, PtDirectParams>();
    }
};
template <unsigned KIND> using PtKindArgs = decltype(PtKindOf<KIND>::block());

// Light sample k of the sample at (p, n, wo) on material mid (steps a-g of the contract).  True when it contributes: then c is its
// contribution if the shadow ray (o, d) is open, and tl the ray's limit (not above 0: nothing is searched, the ray is open).  The
// three uniforms are drawn whatever follows.  The quotients are pt_div's: the short form inside its guarded window, the generic
// division outside it -- the IEEE quotient either way.
// MIS, POWER: the kind's bits.
// MIS (pt_render_indirect_mis): with `weigh` (the vertex is not the path's last) and the light's front towards the vertex (sl > 0) the
// weight takes the balance factor kp / (kp counts[j] + pbl) against the BRDF's density pbl towards wi; these quotients are the
// generic IEEE division (their operands have no proven window).  MIS = false is the code of pt_render_direct and pt_render_indirect.
// POWER (pt_render_direct_power, pt_render_indirect_power): the entry is chosen through pt_light_table's cdf -- x = (u total) >> 24 of
// the 24-bit uniform u, the entry with cdf[i] <= x < cdf[i + 1] by binary search -- and total / q_i stands where (float)nl stands in the
// weight; an empty table (total = 0) contributes nothing.  The search's temporaries die before the light's record is gathered.
// POWER = false is the uniform choice, the parent's code.
// WI_ONLY (pt_ris_light's candidates): o returns wi and d is not written -- the ray (o, d) is formed from wi by the caller, for the kept
// candidate alone, with the two statements below.
PTK_DEV float pt_light_table_inv(const uint64_t* cdf, int nl, float r0, unsigned& li)
{
    const uint64_t total = cdf[nl];
    li = 0u;
    if (total == 0ull) return 0.0f;   // (an empty table: nothing is searched)
    unsigned u = (unsigned)(r0 * 16777216.0f);   // (getRandomFloat can return 1.0)
    u = u > 16777215u ? 16777215u : u;
    const uint64_t x = ((uint64_t)u * total) >> 24;   // < total < 2^40: the product stays below 2^64
    unsigned lo = 0u, hi = (unsigned)nl;              // cdf[lo] <= x < cdf[hi]
    while (hi - lo > 1u) {
        const unsigned m = (lo + hi) >> 1;
        if (cdf[m] <= x) lo = m; else hi = m;
    }
    li = lo;
    return (float)total / (float)(cdf[lo + 1u] - cdf[lo]);   // >= 1
}

template <unsigned KIND, bool WI_ONLY = false>
PTK_DEV bool pt_direct_light(const PtDirectParams& D, const f3& p, const f3& n, const f3& wo, unsigned mid, uint32_t& seed, f3& c, f3& o, f3& d,
                             float& tl, const int32_t* counts, bool weigh, const uint64_t* cdf)
{
    constexpr bool MIS = PtKindOf<KIND>::mis, POWER = PtKindOf<KIND>::power;
    const float r0 = pt_random_float(seed), r1 = pt_random_float(seed), r2 = pt_random_float(seed);
    float nlf;       // the reciprocal of the probability of the entry chosen: nl, or total / q_i
    unsigned li;
    if constexpr (POWER) {
        nlf = pt_light_table_inv(cdf, D.nl, r0, li);
        if (nlf == 0.0f) return false;   // (total = 0: the three uniforms are drawn, no ray is cast)
    } else {
        nlf = (float)D.nl;
        li = (unsigned)(r0 * nlf);
        li = li > (unsigned)D.nl - 1u ? (unsigned)D.nl - 1u : li;
    }
    const unsigned j = pt_clamp_index(D.lights[li], D.t.ntri);
    // the light's prepared record: p1, e1 = p2 - p1, e2 = p3 - p1, N = cross(e2, e1) (:92-93, :123; computed once per upload, the same bits)
    const float4 ra = pt_rec16(D.t.tris, j, 0u), rb = pt_rec16(D.t.tris, j, 16u), rc = pt_rec16(D.t.tris, j, 32u), nid = pt_rec16(D.t.tris, j, 48u);
    const f3 p1 = mk3(ra.x, ra.y, ra.z), e1 = mk3(ra.w, rb.x, rb.y), e2 = mk3(rb.z, rb.w, rc.x), N = mk3(nid.x, nid.y, nid.z);
    const float N2 = dot3(N, N);
    const f3 nj = scale3(N, pt_normalize_factor(N2));
    const float area = 0.5f * pt_sqrt(N2);
    const float su = pt_sqrt(r1), b1 = 1.0f - su, b2 = r2 * su;
    const f3 q = add3(add3(p1, scale3(e1, b1)), scale3(e2, b2));
    const f3 dv = sub3(q, p);
    const float d2 = dot3(dv, dv);
    const float dist = pt_sqrt(d2);
    const f3 wi = scale3(dv, pt_normalize_factor(d2));
    const float cs = dot3(wi, n), sl = dot3(wi, nj), cl = __builtin_fabsf(sl);
    if (!(cs > 0.0f && cl > 0.0f)) return false;   // (false for NaN: q == p, a light of no area)
    const float4 alb = pt_rec16(D.t.mats, mid, 0u), rt = pt_rec16(D.t.mats, mid, 32u);   // albedo | roughness, type
    const int type = __float_as_int(rt.y);
    f3 f;
    float pbl = 0.0f;   // (MIS) the BRDF sample's density towards wi
    if (type == 1) {   // :203
        f = mk3(alb.x * PTK_INV_PI, alb.y * PTK_INV_PI, alb.z * PTK_INV_PI);
        if constexpr (MIS) pbl = cs * PTK_INV_PI;   // :201
    } else if (type == 2) {   // :205-217 at the half vector of wo and wi
        const f3 wh = normalize3(add3(wo, wi));
        const float ct = dot3(wh, n);
        const float r2g = rt.x * rt.x;
        const float gd = ct * ct * (r2g - 1.0f) + 1.0f;
        const float Dg = pt_div(r2g * PTK_INV_PI, gd * gd);   // pow(x, 2.0f) is x*x in PTSPEC (:177)
        if constexpr (MIS) pbl = Dg * ct / (4.0f * dot3(wo, wh));   // :215
        const float dwon = dot3(wo, n);
        if (cs * dwon < 0.0f) {   // :211
            f = mk3(0.0f, 0.0f, 0.0f);
        } else {
            const float g = pt_div(Dg, 4.0f * cs * dwon);
            f = mk3(alb.x * g * 2.0f, alb.y * g * 2.0f, alb.z * g * 2.0f);
        }
    } else {
        return false;   // :220
    }
    const float4 emj = pt_rec16(D.t.mats, pt_clamp_index(__float_as_int(nid.w), D.t.nmat), 16u);
    float w = pt_div(cs * cl, d2) * (area * nlf);
    if constexpr (MIS) {
        if (weigh && sl > 0.0f) {
            const float a = area * nlf;
            const float pe = d2 / (cl * a);
            const float kp = (float)D.K * pe;
            w = w * (kp / (kp * (float)counts[j] + pbl));
        }
    }
    c = mk3((f.x * (emj.x * 3.0f)) * w, (f.y * (emj.y * 3.0f)) * w, (f.z * (emj.z * 3.0f)) * w);
    if constexpr (WI_ONLY) {
        o = wi;
    } else {
        o = add3(p, scale3(wi, 0.01f));   // :257
        d = normalize3(wi);
    }
    tl = dist - 0.02f;
    tl = tl < 1e20f ? tl : 1e20f;
    return true;
}

// Resampled light sample (RIS; include/pt_shim.h states every step): M candidates, each pt_direct_light's -- its three
// uniforms, its table lookup, its c with the balance factor where the parent has it -- and from the second on one uniform r more, drawn
// whether or not the candidate contributes: 4M - 1 uniforms.  A candidate that contributes with s = max channel of c > 0 (false for
// NaN) adds s to wsum and is kept iff none is held or r * wsum < s, a reservoir of one.  True when one is held: c = c_sel * ((wsum / M)
// / s_sel), two generic IEEE divisions, and (o, d, tl) are its ray -- the caller casts it as the parent casts its own.  False: nothing
// is written.  M is wave-uniform, so the lanes of a wave evaluate their candidates in step; the reservoir -- the kept c, wi (the ray is
// formed from it after the loop: nine registers, not twelve), tl and s, and wsum -- dies here: what a lane holds across the search is
// the parent's c, o, d, tl.  M = 1: no r, wsum = s, g = 1.0f.
template <unsigned KIND>
PTK_DEV bool pt_ris_light(const PtDirectParams& D, const f3& p, const f3& n, const f3& wo, unsigned mid, uint32_t& seed, f3& c, f3& o, f3& d,
                          float& tl, const int32_t* counts, bool weigh, const uint64_t* cdf, int M)
{
    float wsum = 0.0f, ssel = 0.0f;
    bool have = false;
    f3 cs = mk3(0.0f, 0.0f, 0.0f), ws = cs;
    float ts = 0.0f;
    for (int m = 0; m < M; ++m) {
        f3 cm = mk3(0.0f, 0.0f, 0.0f), wm = cm, unused = cm;
        float tm = 0.0f;
        const bool ok = pt_direct_light<KIND, true>(D, p, n, wo, mid, seed, cm, wm, unused, tm, counts, weigh, cdf);
        float r = 0.0f;
        if (m >= 1) r = pt_random_float(seed);
        if (ok) {
            const float s = pt_max(cm.x, pt_max(cm.y, cm.z));
            if (s > 0.0f) {
                wsum = wsum + s;
                if (!have || r * wsum < s) {
                    cs = cm; ws = wm; ts = tm; ssel = s;
                    have = true;
                }
            }
        }
    }
    if (!have) return false;
    const float g = (wsum / (float)M) / ssel;
    c = mk3(cs.x * g, cs.y * g, cs.z * g);
    o = add3(p, scale3(ws, 0.01f));   // :257
    d = normalize3(ws);
    tl = ts;
    return true;
}

// ---- environment lighting: an octahedral sky map (include/pt_shim.h, "environment lighting", states every expression) ----
// The map is N x N texels, N a power of two, y up; a direction d maps to the unit square through its L1 normalisation, the lower
// hemisphere folded outward over the diagonals.  Only fabs, +, *, the IEEE "/" and sqrt: a CPU restatement agrees bit for bit.

PTK_DEV float pt_env_sgn(float v) { return v < 0.0f ? -1.0f : 1.0f; }   // (-0 and NaN give +1)

// the index of coordinate c in [-1, 1]: floor(((c + 1) * 0.5) * N) clamped into [0, N - 1], comparison first, so that it is defined for
// every float -- a NaN or a negative v gives 0, anything from N - 1 up (infinity too) gives N - 1 -- and the conversion only ever sees a
// value in [0, N - 1)
PTK_DEV unsigned pt_env_index(float c, int N)
{
    const float v = ((c + 1.0f) * 0.5f) * (float)N;
    if (!(v >= 0.0f)) return 0u;
    return v >= (float)(N - 1) ? (unsigned)(N - 1) : (unsigned)v;
}

// the texel of direction d (any length, any float): row * N + col < N * N; s = (|d.x| + |d.y|) + |d.z| is returned for the density
PTK_DEV unsigned pt_env_texel(const f3& d, int N, float& s)
{
    s = (__builtin_fabsf(d.x) + __builtin_fabsf(d.y)) + __builtin_fabsf(d.z);
    const float x = d.x / s, z = d.z / s;
    float a = x, b = z;
    if (!(d.y >= 0.0f)) {   // the lower hemisphere (and a NaN d.y)
        a = (1.0f - __builtin_fabsf(z)) * pt_env_sgn(x);
        b = (1.0f - __builtin_fabsf(x)) * pt_env_sgn(z);
    }
    return pt_env_index(b, N) * (unsigned)N + pt_env_index(a, N);
}

// the point P of the octahedron |x| + |y| + |z| = 1 over (a, b) in [-1, 1]^2; its direction is normalize(P), r = |P|
PTK_DEV f3 pt_env_point(float a, float b)
{
    const float fa = __builtin_fabsf(a), fb = __builtin_fabsf(b);
    const float h = (1.0f - fa) - fb;
    if (h >= 0.0f) return mk3(a, h, b);
    return mk3((1.0f - fb) * pt_env_sgn(a), h, (1.0f - fa) * pt_env_sgn(b));
}

// the density, per solid angle, of a direction of texel weight q whose octahedron point lies at distance r: (q / total) (N^2 / 4) r^3
PTK_DEV float pt_env_pdf(uint64_t q, uint64_t total, int N, float r)
{
    const float nn4 = ((float)N * (float)N) * 0.25f;   // exact: N is a power of two
    return (((float)q / (float)total) * nn4) * ((r * r) * r);
}

// a 16-byte texel / an 8-byte table word at a 32-bit byte offset from the wave-uniform base (N * N <= 2^22 texels)
PTK_DEV float4 pt_env_load(const float4* texels, unsigned i)
{
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(texels) + (size_t)(i * 16u));
}
PTK_DEV uint64_t pt_env_word(const uint64_t* cdf, unsigned i)
{
    return *reinterpret_cast<const uint64_t*>(reinterpret_cast<const char*>(cdf) + (size_t)(i * 8u));
}

// What a ray (direction d) that leaves the scene adds per unit of mask: the texel of d.  `weigh` (MIS, a vertex i >= 1, Ke > 0): times
// wb = pb / (Ke pdf(d) + pb), the balance against the environment samples of the vertex before; q = 0 or total = 0 gives wb = 1
PTK_DEV f3 pt_env_miss(const PtEnvMap& E, const f3& d, bool weigh, float pb)
{
    float s;
    const unsigned i = pt_env_texel(d, E.N, s);
    const float4 le = pt_env_load(E.texels, i);
    f3 Le = mk3(le.x, le.y, le.z);
    if (weigh) {
        const uint64_t total = pt_env_word(E.cdf, (unsigned)(E.N * E.N));
        const uint64_t q = pt_env_word(E.cdf, i + 1u) - pt_env_word(E.cdf, i);
        float wb = 1.0f;
        if (q != 0ull && total != 0ull) {
            const float r = pt_sqrt(dot3(d, d)) / s;
            wb = pb / ((float)E.Ke * pt_env_pdf(q, total, E.N, r) + pb);
        }
        Le = scale3(Le, wb);
    }
    return Le;
}

// Environment sample of the vertex (p, n, wo) on material mid (steps a-i of the contract): pt_direct_light's shape -- true when it
// contributes, then c is its contribution if the shadow ray (o, d) is open; the ray's limit is 1e20, always searched.  The three
// uniforms are drawn whatever follows.  The texel is chosen through the table as the choice by power chooses its entry; the BRDF value
// f and the density pbl are pt_direct_light's statements.  MIS with `weigh` (the vertex is not the path's last): c carries kp / (kp +
// pbl), kp = Ke pdf -- the sky has no back side and no count
template <bool MIS>
PTK_DEV bool pt_env_light(const PtDirectParams& D, const PtEnvMap& E, const f3& p, const f3& n, const f3& wo, unsigned mid, uint32_t& seed, f3& c,
                          f3& o, f3& d, bool weigh)
{
    const float r0 = pt_random_float(seed), r1 = pt_random_float(seed), r2 = pt_random_float(seed);
    const unsigned nn = (unsigned)(E.N * E.N);
    const uint64_t total = pt_env_word(E.cdf, nn);
    if (total == 0ull) return false;   // (an empty table: the three uniforms are drawn, no ray is cast)
    unsigned u = (unsigned)(r0 * 16777216.0f);   // (getRandomFloat can return 1.0)
    u = u > 16777215u ? 16777215u : u;
    const uint64_t x = ((uint64_t)u * total) >> 24;
    unsigned lo = 0u, hi = nn;   // cdf[lo] <= x < cdf[hi]
    while (hi - lo > 1u) {
        const unsigned m = (lo + hi) >> 1;
        if (pt_env_word(E.cdf, m) <= x) lo = m; else hi = m;
    }
    const uint64_t q = pt_env_word(E.cdf, lo + 1u) - pt_env_word(E.cdf, lo);
    const unsigned col = lo & (unsigned)(E.N - 1), row = lo >> (31 - __builtin_clz((unsigned)E.N));
    const float step = 2.0f / (float)E.N;   // exact
    const f3 P = pt_env_point(((float)col + r1) * step - 1.0f, ((float)row + r2) * step - 1.0f);
    const float P2 = dot3(P, P);
    const float r = pt_sqrt(P2);
    const f3 wi = scale3(P, pt_normalize_factor(P2));
    const float cs = dot3(wi, n);
    if (!(cs > 0.0f)) return false;   // (false for NaN)
    const float4 alb = pt_rec16(D.t.mats, mid, 0u), rt = pt_rec16(D.t.mats, mid, 32u);   // albedo | roughness, type
    const int type = __float_as_int(rt.y);
    f3 f;
    float pbl = 0.0f;   // (MIS) the BRDF sample's density towards wi
    if (type == 1) {   // :203
        f = mk3(alb.x * PTK_INV_PI, alb.y * PTK_INV_PI, alb.z * PTK_INV_PI);
        if constexpr (MIS) pbl = cs * PTK_INV_PI;   // :201
    } else if (type == 2) {   // :205-217 at the half vector of wo and wi
        const f3 wh = normalize3(add3(wo, wi));
        const float ct = dot3(wh, n);
        const float r2g = rt.x * rt.x;
        const float gd = ct * ct * (r2g - 1.0f) + 1.0f;
        const float Dg = pt_div(r2g * PTK_INV_PI, gd * gd);   // pow(x, 2.0f) is x*x in PTSPEC (:177)
        if constexpr (MIS) pbl = Dg * ct / (4.0f * dot3(wo, wh));   // :215
        const float dwon = dot3(wo, n);
        if (cs * dwon < 0.0f) {   // :211
            f = mk3(0.0f, 0.0f, 0.0f);
        } else {
            const float g = pt_div(Dg, 4.0f * cs * dwon);
            f = mk3(alb.x * g * 2.0f, alb.y * g * 2.0f, alb.z * g * 2.0f);
        }
    } else {
        return false;   // :220
    }
    const float4 le = pt_env_load(E.texels, lo);
    const float pdf = pt_env_pdf(q, total, E.N, r);
    float w = cs / pdf;
    if constexpr (MIS) {
        if (weigh) {
            const float kp = (float)E.Ke * pdf;
            w = w * (kp / (kp + pbl));
        }
    }
    c = mk3((f.x * le.x) * w, (f.y * le.y) * w, (f.z * le.z) * w);
    o = add3(p, scale3(wi, 0.01f));   // :257
    d = normalize3(wi);
    return true;
}

// L += mask * (Se / Ke) of a vertex's environment samples
PTK_DEV void pt_env_lit(int Ke, const f3& mask, const f3& S, f3& L)
{
    const float Kf = (float)Ke;
    L.x = L.x + mask.x * (S.x / Kf);
    L.y = L.y + mask.y * (S.y / Kf);
    L.z = L.z + mask.z * (S.z / Kf);
}

// direct illumination under the map: max((E + S / K) + Se / Ke, 0); Ke = 0 adds nothing (pt_direct_radiance's value, bit for bit)
PTK_DEV f3 pt_direct_env_radiance(const PtDirectParams& D, int Ke, unsigned mid, const f3& S, const f3& Se)
{
    const float4 emi = pt_rec16(D.t.mats, mid, 16u);
    const float Kf = (float)D.K;
    f3 v = mk3(emi.x * 3.0f + S.x / Kf, emi.y * 3.0f + S.y / Kf, emi.z * 3.0f + S.z / Kf);
    if (Ke > 0) {
        const float Kef = (float)Ke;
        v = mk3(v.x + Se.x / Kef, v.y + Se.y / Kef, v.z + Se.z / Kef);
    }
    return mk3(pt_max(v.x, 0.0f), pt_max(v.y, 0.0f), pt_max(v.z, 0.0f));
}

// the sample's radiance max(E + S / K, 0), E = 1.0f * emissive * 3.0f of the hit's material (:241)
PTK_DEV f3 pt_direct_radiance(const PtDirectParams& D, unsigned mid, const f3& S)
{
    const float4 emi = pt_rec16(D.t.mats, mid, 16u);
    const float Kf = (float)D.K;
    return mk3(pt_max(emi.x * 3.0f + S.x / Kf, 0.0f), pt_max(emi.y * 3.0f + S.y / Kf, 0.0f), pt_max(emi.z * 3.0f + S.z / Kf, 0.0f));
}

// the light sample of a vertex as the kind draws it: resampled (pt_ris_light), chosen by power, or uniform; A is the kind's block, D its
// PtDirectParams.  weigh: (MIS) the vertex is not the path's last
template <unsigned KIND>
PTK_DEV bool pt_kind_light(const PtKindArgs<KIND>& A, const PtDirectParams& D, const f3& p, const f3& n, const f3& wo, unsigned mid, uint32_t& seed,
                           f3& c, f3& o, f3& d, float& tl, bool weigh)
{
    using K = PtKindOf<KIND>;
    const int32_t* counts = nullptr;   // (no kind without MIS reads the counts, none without POWER the table)
    const uint64_t* cdf = nullptr;
    if constexpr (K::mis) counts = A.counts;
    if constexpr (K::power) cdf = A.cdf;
    if constexpr (K::ris) return pt_ris_light<KIND>(D, p, n, wo, mid, seed, c, o, d, tl, counts, weigh, cdf, A.M);
    else return pt_direct_light<KIND>(D, p, n, wo, mid, seed, c, o, d, tl, counts, weigh, cdf);
}

// brute force: one wave = 64 consecutive samples; the primary search, then the K shadow rays of the lanes whose light sample
// contributes, all in step (pt_ao_kernel's shape); a light sample no lane of the wave casts a ray for costs no search.
// env (pt_render_direct_env): a miss stores the map's texel, and the Ke environment samples follow the K light samples in the same
// shape -- a search only when some lane casts --, summed apart in Se
template <bool DET_BOUNDED, int LDS_TABLE, int QUADS, unsigned KIND>
__global__ __launch_bounds__(PT_TRACE_THREADS) void pt_direct_kernel(const PtKindArgs<KIND> D)
{
    constexpr bool ENV = PtKindOf<KIND>::env;
    const PtTraceParams& P = D.t;
    const unsigned lane = pt_lane_id();
    const int ntri = P.ntri;
    PtTail tl = pt_table_wg_setup<LDS_TABLE>(P, lane);
    const f3 anchor = mk3(P.cam.eye[0], P.cam.eye[1], P.cam.eye[2]);
    const unsigned item = pt_wave() * 64u + lane;
    const bool act = item < D.nitems;
    unsigned lp = 0u;
    uint32_t seed = 0u;
    f3 o = mk3(0.0f, 0.0f, 0.0f), d = mk3(0.0f, 0.0f, 1.0f);
    if (act) pt_item_begin(P, D.cam, D.npix, D.frame0, item, lp, seed, o, d);
    float tmax = 1e20f, hu = 0.0f, hv = 0.0f;
    int hidx = -1;
    pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, act, tmax, hu, hv, hidx,
                                                         P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
    const bool hit = act & (hidx >= 0);
    const float bg = pt_max(0.45f, 0.0f);   // :235
    f3 L = mk3(bg, bg, bg);
    if constexpr (ENV) {
        if (act & !hit) {
            const f3 le = pt_env_miss(D.env, d, false, 0.0f);
            L = mk3(pt_max(le.x, 0.0f), pt_max(le.y, 0.0f), pt_max(le.z, 0.0f));
        }
    }
    if (__ballot(hit) != 0ull) {
        f3 p = o, n = d, wo = d, S = mk3(0.0f, 0.0f, 0.0f);
        unsigned mid = 0u;
        if (hit) pt_direct_surface(D, o, d, tmax, hu, hv, hidx, p, n, wo, mid);
        for (int k = 0; k < D.K && D.nl > 0; ++k) {
            f3 c = mk3(0.0f, 0.0f, 0.0f);
            float tlim = 0.0f;
            bool cast = false;
            if (hit) cast = pt_kind_light<KIND>(D, D, p, n, wo, mid, seed, c, o, d, tlim, false);
            const bool live = cast & (tlim > 0.0f);
            bool occluded = false;
            if (__ballot(live) != 0ull) {
                float t = live ? tlim : 0.0f, su = 0.0f, sv = 0.0f;
                int sidx = -1;
                pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, live, t, su, sv, sidx,
                                                                     P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
                occluded = live & (sidx >= 0) & (t < tlim);   // pt_query_store's occlusion test
            }
            if (cast & !occluded) S = add3(S, c);
        }
        if constexpr (ENV) {
            f3 Se = mk3(0.0f, 0.0f, 0.0f);
            for (int k = 0; k < D.env.Ke; ++k) {
                f3 c = mk3(0.0f, 0.0f, 0.0f);
                bool cast = false;
                if (hit) cast = pt_env_light<false>(D, D.env, p, n, wo, mid, seed, c, o, d, false);
                bool occluded = false;
                if (__ballot(cast) != 0ull) {
                    float t = cast ? 1e20f : 0.0f, su = 0.0f, sv = 0.0f;
                    int sidx = -1;
                    pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, cast, t, su, sv, sidx,
                                                                         P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
                    occluded = cast & (sidx >= 0) & (t < 1e20f);
                }
                if (cast & !occluded) Se = add3(Se, c);
            }
            if (hit) L = pt_direct_env_radiance(D, D.env.Ke, mid, S, Se);
        } else {
            if (hit) L = pt_direct_radiance(D, mid, S);
        }
    }
    if (act) pt_direct_store(D, item, L);
}

// LBVH (pt_bvh_drive): one item = one sample; the lane runs its searches one after the other -- the primary ray's closest search,
// then the any-hit searches of the light samples that contribute -- and is free when the sample is stored.  A light sample that
// does not contribute is passed over inside next_ray: it costs the lane no refill
// ENV: k goes on over K .. K + Ke - 1, the environment samples.  Before the first of them E + S / K is folded into `base` and S starts
// again as Se: a lane's state grows by these three registers (PtNoEnv is empty in every other instantiation)
struct PtNoEnv {};
template <unsigned KIND>
struct PtDirectWork {
    static constexpr bool ANY = true, ENV = PtKindOf<KIND>::env;
    const PtKindArgs<KIND>& D;
    unsigned n;
    int k;           // the current ray: -1 = the primary, 0 .. K-1 = the shadow ray of light sample k
    unsigned item, mid;
    uint32_t seed;
    float tl;        // the shadow ray's limit
    f3 o, d, p, nrm, wo, S, c;
    [[no_unique_address]] std::conditional_t<ENV, f3, PtNoEnv> base;
    PTK_DEV void begin(unsigned item_)
    {
        unsigned lp;
        item = item_;
        pt_item_begin(D.t, D.cam, D.npix, D.frame0, item, lp, seed, o, d);
        k = -1;
    }
    PTK_DEV bool next_ray(const PtBvhLane& L)
    {
        if (k < 0) {
            if (L.hidx < 0) {
                if constexpr (ENV) {
                    const f3 le = pt_env_miss(D.env, d, false, 0.0f);
                    pt_direct_store(D, item, mk3(pt_max(le.x, 0.0f), pt_max(le.y, 0.0f), pt_max(le.z, 0.0f)));
                    return false;
                }
                const float bg = pt_max(0.45f, 0.0f);   // :235
                pt_direct_store(D, item, mk3(bg, bg, bg));
                return false;
            }
            pt_direct_surface(D, o, d, L.tmax, L.hu, L.hv, L.hidx, p, nrm, wo, mid);
            S = mk3(0.0f, 0.0f, 0.0f);
        } else if (L.hidx < 0) {   // (an any-hit search: L.hidx >= 0 alone says occluded; a ray that searched nothing is open)
            S = add3(S, c);
        }
        if constexpr (ENV) {
            if (k < D.K) {   // the light samples are not over (k = -1 among them)
                if (D.nl > 0)
                    while (++k < D.K)
                        if (pt_kind_light<KIND>(D, D, p, nrm, wo, mid, seed, c, o, d, tl, false)) return true;
                const float4 emi = pt_rec16(D.t.mats, mid, 16u);
                const float Kf = (float)D.K;
                base = mk3(emi.x * 3.0f + S.x / Kf, emi.y * 3.0f + S.y / Kf, emi.z * 3.0f + S.z / Kf);   // pt_direct_env_radiance's first line
                S = mk3(0.0f, 0.0f, 0.0f);
                k = D.K - 1;
            }
            tl = 1e20f;
            while (++k < D.K + D.env.Ke)
                if (pt_env_light<false>(D, D.env, p, nrm, wo, mid, seed, c, o, d, false)) return true;
            f3 v = base;
            if (D.env.Ke > 0) {
                const float Kef = (float)D.env.Ke;
                v = mk3(v.x + S.x / Kef, v.y + S.y / Kef, v.z + S.z / Kef);
            }
            pt_direct_store(D, item, mk3(pt_max(v.x, 0.0f), pt_max(v.y, 0.0f), pt_max(v.z, 0.0f)));
            return false;
        }
        if (D.nl > 0)
            while (++k < D.K) {
                if (pt_kind_light<KIND>(D, D, p, nrm, wo, mid, seed, c, o, d, tl, false)) return true;
            }
        pt_direct_store(D, item, pt_direct_radiance(D, mid, S));
        return false;
    }
    PTK_DEV const f3& org() const { return o; }
    PTK_DEV const f3& dir() const { return d; }
    PTK_DEV float limit() const { return k < 0 ? 1e20f : tl; }
    PTK_DEV bool live() const { return k < 0 || tl > 0.0f; }
    PTK_DEV bool any() const { return k >= 0; }
};

// Four waves per SIMD (128 VGPRs), not the five of the driver's other kernels: a sample's state between its rays is 25 registers
// against ambient occlusion's 16, and at five waves (96 VGPRs) the kernel spills 19 of them (profiles/direct/kernel_resources.txt).
// Its persistent grid is therefore its own figure, ptk_lit_bvh_blocks_per_cu of its kind, not ptk_query_bvh_blocks_per_cu
#define PT_DIRECT_BVH_WAVES 4
// The env kinds run at three: next_ray holds the light sample and the environment sample -- its table search in 64-bit
// words among them -- and at four waves would spill 33 VGPRs (profiles/env/kernel_resources.txt has both figures)
#ifndef PT_DIRECT_ENV_BVH_WAVES   // (tools/kernel_resources.sh -DPT_DIRECT_ENV_BVH_WAVES=4 reads the other choice)
#define PT_DIRECT_ENV_BVH_WAVES 3
#endif
constexpr int pt_direct_bvh_waves(unsigned kind) { return ptk_lit_kind_of(kind).env ? PT_DIRECT_ENV_BVH_WAVES : PT_DIRECT_BVH_WAVES; }
template <bool DET_BOUNDED, int BIGQ, unsigned KIND>
__global__ __launch_bounds__(PT_TRACE_THREADS) __attribute__((amdgpu_waves_per_eu(pt_direct_bvh_waves(KIND), pt_direct_bvh_waves(KIND))))
void pt_direct_bvh_kernel(const PtKindArgs<KIND> D)
{
    const f3 o0 = mk3(0.0f, 0.0f, 0.0f), d0 = mk3(0.0f, 0.0f, 1.0f);
    PtDirectWork<KIND> W = { D, D.nitems, -1, 0u, 0u, 0u, 0.0f, o0, d0, o0, d0, d0, o0, o0, {} };
    pt_bvh_drive<DET_BOUNDED, BIGQ>(D.t, W);
}

// ------------------------------------------------------------------------------------------
// first-hit feature buffers (pt_render_features)
// ------------------------------------------------------------------------------------------
// One work item is one sample, as for direct illumination (pt_item_begin): the renderer's primary ray and its closest hit from tmax
// 1e20, the surface and the clamped material index (pt_direct_surface) -- direct illumination's steps 1 and 2, and nothing after them.
// Item i writes 12 bytes to X[i] of every output X the launch has: the material's albedo as stored, the facing normal, (t, 1, -dot(n, d))
// and the emission emissive * 3 (:241); a miss writes zeros.  Nothing is clamped: a NaN goes out as it is.  Which outputs exist is
// uniform for the launch: the four pointers are tested on the by-value block, once per record.
PTK_DEV void pt_feature_put(float* out, unsigned item, const f3& v)
{
    pt_f3v w;
    w.x = v.x; w.y = v.y; w.z = v.z;
    *reinterpret_cast<pt_f3v*>(out + (size_t)item * 3u) = w;
}

// the records of sample `item`: hit = its primary ray (direction d) hit at t, n the facing normal, mid the clamped material index --
// one gather of the material's first 32 bytes, then up to four stores
PTK_DEV void pt_feature_store(const PtFeatureParams& F, unsigned item, bool hit, const f3& d, float t, const f3& n, unsigned mid)
{
    f3 alb = mk3(0.0f, 0.0f, 0.0f), emi = alb, nrm = alb, dep = alb;
    if (hit) {
        const float4 a = pt_rec16(F.d.t.mats, mid, 0u), e = pt_rec16(F.d.t.mats, mid, 16u);
        alb = mk3(a.x, a.y, a.z);
        emi = mk3(e.x * 3.0f, e.y * 3.0f, e.z * 3.0f);   // 1.0f * emissive * 3.0f (:241)
        nrm = n;
        dep = mk3(t, 1.0f, -dot3(n, d));
    }
    if (F.albedo) pt_feature_put(F.albedo, item, alb);
    if (F.normal) pt_feature_put(F.normal, item, nrm);
    if (F.depth) pt_feature_put(F.depth, item, dep);
    if (F.emission) pt_feature_put(F.emission, item, emi);
}

// brute force: one wave = 64 consecutive samples and one search -- pt_direct_kernel up to its surface.  A wave none of whose lanes
// hit stores its miss records and is done
template <bool DET_BOUNDED, int LDS_TABLE, int QUADS>
__global__ __launch_bounds__(PT_TRACE_THREADS) void pt_feature_kernel(const PtFeatureParams F)
{
    const PtTraceParams& P = F.d.t;
    const unsigned lane = pt_lane_id();
    const int ntri = P.ntri;
    PtTail tl = pt_table_wg_setup<LDS_TABLE>(P, lane);
    const f3 anchor = mk3(P.cam.eye[0], P.cam.eye[1], P.cam.eye[2]);
    const unsigned item = pt_wave() * 64u + lane;
    const bool act = item < F.d.nitems;
    unsigned lp = 0u;
    uint32_t seed = 0u;
    f3 o = mk3(0.0f, 0.0f, 0.0f), d = mk3(0.0f, 0.0f, 1.0f);
    if (act) pt_item_begin(P, F.d.cam, F.d.npix, F.d.frame0, item, lp, seed, o, d);
    float tmax = 1e20f, hu = 0.0f, hv = 0.0f;
    int hidx = -1;
    pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, act, tmax, hu, hv, hidx,
                                                         P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
    const bool hit = act & (hidx >= 0);
    f3 p = o, n = d, wo = d;
    unsigned mid = 0u;
    if (__ballot(hit) == 0ull) {
        if (act) pt_feature_store(F, item, false, d, tmax, n, mid);
        return;
    }
    if (hit) pt_direct_surface(F.d, o, d, tmax, hu, hv, hidx, p, n, wo, mid);
    if (act) pt_feature_store(F, item, hit, d, tmax, n, mid);
}

// LBVH (pt_bvh_drive): one item = one sample = one closest search; the lane is free when its records are stored.  A ray starts
// at the lens, which may lie anywhere: the slabs carry the ray term of the margin, as for queries and ambient occlusion
struct PtFeatureWork {
    static constexpr bool ANY = false;
    const PtFeatureParams& F;
    unsigned n, item;
    f3 o, d;
    PTK_DEV void begin(unsigned item_)
    {
        unsigned lp;
        uint32_t seed;
        item = item_;
        pt_item_begin(F.d.t, F.d.cam, F.d.npix, F.d.frame0, item, lp, seed, o, d);
    }
    PTK_DEV bool next_ray(const PtBvhLane& L)
    {
        f3 p = o, nrm = d, wo = d;
        unsigned mid = 0u;
        const bool hit = L.hidx >= 0;
        if (hit) pt_direct_surface(F.d, o, d, L.tmax, L.hu, L.hv, L.hidx, p, nrm, wo, mid);
        pt_feature_store(F, item, hit, d, L.tmax, nrm, mid);
        return false;
    }
    PTK_DEV const f3& org() const { return o; }
    PTK_DEV const f3& dir() const { return d; }
    PTK_DEV float limit() const { return 1e20f; }
    PTK_DEV bool live() const { return true; }
    PTK_DEV bool any() const { return false; }
};

template <bool DET_BOUNDED, int BIGQ>
__global__ __launch_bounds__(PT_TRACE_THREADS) PT_BVH_WAVES_ATTR
void pt_feature_bvh_kernel(const PtFeatureParams F)
{
    const f3 o0 = mk3(0.0f, 0.0f, 0.0f), d0 = mk3(0.0f, 0.0f, 1.0f);
    PtFeatureWork W = { F, F.d.nitems, 0u, o0, d0 };
    pt_bvh_drive<DET_BOUNDED, BIGQ>(F.d.t, W);
}

// ------------------------------------------------------------------------------------------
// indirect illumination (pt_render_indirect)
// ------------------------------------------------------------------------------------------
// The renderer's multi-bounce walk (traceRays, :223-261) with direct illumination's light sample taken at every vertex
// (include/pt_shim.h states every step and its order).  One work item is one sample (pt_item_begin).  For i = 0 .. B-1: the closest
// hit from 1e20; a miss adds mask * max(0.45, 0) and ends the path.  On a hit: the surface (pt_direct_surface), the emission when
// i == 0 or there are no lights, K light samples (pt_direct_light) whose open shadow rays sum to S and L += mask * (S / K), then the
// BRDF sample (pt_indirect_bounce), which ends the path at pdf <= 0 and otherwise scales mask and gives the next ray.
// samples[item] = max(L, 0); pt_fold_kernel folds them.
// MIS (pt_render_indirect_mis) is a compile-time flag of the same kernels: the light samples of every vertex but the last are
// weighted against the BRDF sample (pt_direct_light), the path carries that sample's pdf (pb), and a later vertex on an emitter
// adds its emission weighted the other way (pt_indirect_emission_mis).  The MIS = false instantiations are pt_render_indirect's code,
// instruction for instruction (profiles/mis/disasm_comparison.txt).

// The BRDF sample at the vertex (p, n, wo) on material mid: Brdf (:195-221) and :251-257 as pt_shade states them -- the same draws
// (phi, then the second uniform), the same shared sqrt pair, the same guarded short quotients (pt_div_by, pt_div, pt_div_pair,
// pt_div3) and near-1 normalisations (normalize3_unit).  A second statement of pt_shade's bounce, kept apart so that the renderer's
// kernels do not move; with no lights the two must agree bit for bit (tests/test_gpu_indirect.py).  False: pdf <= 0, the path ends
// (:251); true: mask has taken the bounce's three quotients and (o, d) is the next ray (:257).  The material is gathered by its index
// (pt_direct_light's gathers): nothing of it is held across a search.
template <bool MIS = false>
PTK_DEV bool pt_indirect_bounce(const PtDirectParams& D, const f3& p, const f3& n, const f3& wo, unsigned mid, uint32_t& seed, f3& mask, f3& o,
                                f3& d, float* pb = nullptr)
{
    const float phi = PTK_TWO_PI * pt_random_float(seed);
    const float xi = pt_random_float(seed);
    float sp, cp;
    pt_sincos(phi, sp, cp);
    const float4 alb = pt_rec16(D.t.mats, mid, 0u), rt = pt_rec16(D.t.mats, mid, 32u);   // albedo | roughness, type
    const float rough = rt.x;
    const int type = __float_as_int(rt.y);

    // sampleHemisphereCosine (:161-172) and sampleGGX (:180-192) share everything except (sinTheta, cosTheta)
    const f3 axis = __builtin_fabsf(n.x) > 0.001f ? mk3(0.0f, 1.0f, 0.0f) : mk3(1.0f, 0.0f, 0.0f);
    const f3 tv = normalize3(cross3(axis, n));
    const f3 sv = cross3(n, tv);
    float cos_arg = 1.0f - xi;
    if (type == 2) cos_arg = pt_div_by(cos_arg, xi * (rough * rough - 1.0f) + 1.0f);   // (1 - xi is +0 or in [2^-24, 1]: pt_shade)
    const float cosTheta = pt_sqrt(cos_arg);
    const float sin_arg = type == 2 ? pt_max(0.0f, 1.0f - cosTheta * cosTheta) : xi;
    const float sinTheta = pt_sqrt(sin_arg);
    const f3 a = scale3(scale3(sv, cp), sinTheta);
    const f3 b = scale3(scale3(tv, sp), sinTheta);
    const f3 c = scale3(n, cosTheta);
    const f3 sdir = normalize3_unit(add3(add3(a, b), c));

    f3 wi = sdir;
    f3 color = mk3(0.0f, 0.0f, 0.0f);
    float pdf = 0.0f;
    float dwin = 0.0f;
    if (type == 1) {   // DIFFUSE (:197-204)
        dwin = dot3(wi, n);
        pdf = dwin * PTK_INV_PI;
        color = mk3(alb.x * PTK_INV_PI, alb.y * PTK_INV_PI, alb.z * PTK_INV_PI);
    } else if (type == 2) {   // SPECULAR (:205-218)
        const float k2 = 2.0f * dot3(wo, sdir);
        wi = add3(neg3(wo), scale3(sdir, k2));   // reflect(wo, wh) (:156-159)
        dwin = dot3(wi, n);
        const float dwon = dot3(wo, n);
        if (!(dwin * dwon < 0.0f)) {
            const float r2 = rough * rough;
            const float gd = cosTheta * cosTheta * (r2 - 1.0f) + 1.0f;
            const float Dg = pt_div(r2 * PTK_INV_PI, gd * gd);   // pow(x, 2.0f) is x*x in PTSPEC (:177)
            float g;
            pt_div_pair(Dg * cosTheta, 4.0f * dot3(wo, sdir), Dg, 4.0f * dwin * dwon, pdf, g);   // (one guard for both: pt_shade)
            color = mk3(alb.x * g * 2.0f, alb.y * g * 2.0f, alb.z * g * 2.0f);
        }
    }
    if (pdf <= 0.0f) return false;   // :251
    if constexpr (MIS) *pb = pdf;   // (MIS: the path carries it to the next vertex's emission)
    float qx = color.x * dwin, qy = color.y * dwin, qz = color.z * dwin;
    pt_div3(qx, qy, qz, pdf);   // the three IEEE quotients of :253-255
    mask.x = mask.x * qx;
    mask.y = mask.y * qy;
    mask.z = mask.z * qz;
    o = add3(p, scale3(wi, 0.01f));   // :257
    d = normalize3_unit(wi);
    return true;
}

// pt_light_counts: counts[t] = the list entries that name triangle t, each clamped as pt_direct_light clamps it (the host has cleared
// counts; ntri >= 1).  One vector atomic per entry
__global__ __launch_bounds__(256) void pt_light_counts_kernel(const int32_t* __restrict__ lights, int nl, int ntri, int32_t* __restrict__ counts)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)nl) return;
    atomicAdd(counts + pt_clamp_index(lights[i], ntri), 1);
}

// ---- pt_light_table: the selection table of light choice by power (include/pt_shim.h states every expression) ----
// The weight of entry i is integer once quantised, so the sums do not depend on the order of the scan.  Four kernels behind a clear:
//   pt_light_weight_kernel    p_i of every entry, and their maximum by a vector atomic max on the float's bits (p_i > 0: the bits order as
//                             the values do);
//   pt_light_quantise_kernel  p_i again (the same bits), q_i, tri_q[j] = q_i (entries that name one triangle store one value), q_i parked
//                             in cdf[i + 1], and the sum of each tile of PT_LIGHT_SCAN_TILE entries;
//   pt_light_tiles_kernel     one workgroup: the tile sums become the tiles' offsets; cdf[0] = 0;
//   pt_light_scan_kernel      each tile's running sum from its offset, in place.
// A thread owns PT_LIGHT_SCAN_ITEMS consecutive entries, a workgroup one tile.

// p_i of the contract: area * ((em.x + em.y) + em.z) of the entry's triangle, 0 unless positive and finite
PTK_DEV float pt_light_power(const PtRawTriangle* __restrict__ tris, int ntri, const PtRawMaterial* __restrict__ mats, int nmat, int index)
{
    const PtRawTriangle& t = tris[pt_clamp_index(index, ntri)];
    const f3 p1 = mk3(t.p1[0], t.p1[1], t.p1[2]);
    const f3 e1 = sub3(mk3(t.p2[0], t.p2[1], t.p2[2]), p1), e2 = sub3(mk3(t.p3[0], t.p3[1], t.p3[2]), p1);   // :92-93
    const f3 N = cross3(e2, e1);                                                                           // :123
    const float area = 0.5f * pt_sqrt(dot3(N, N));
    const float* em = mats[pt_clamp_index(t.id, nmat)].emissive;
    const float pw = area * ((em[0] + em[1]) + em[2]);
    return pw > 0.0f && pw < __builtin_inff() ? pw : 0.0f;
}

PTK_DEV uint32_t pt_light_quantum(float pw, float pmax)
{
    if (!(pw > 0.0f)) return 0u;
    const uint32_t q = (uint32_t)((pw / pmax) * 65536.0f);
    return q > 1u ? q : 1u;
}

__global__ __launch_bounds__(PT_LIGHT_SCAN_BLOCK) void pt_light_weight_kernel(const PtRawTriangle* __restrict__ tris, int ntri,
                                                                              const PtRawMaterial* __restrict__ mats, int nmat,
                                                                              const int32_t* __restrict__ lights, int nl, uint32_t* __restrict__ pmax_bits)
{
    const unsigned i = blockIdx.x * PT_LIGHT_SCAN_BLOCK + threadIdx.x;
    if (i >= (unsigned)nl) return;
    const float pw = pt_light_power(tris, ntri, mats, nmat, lights[i]);
    if (pw > 0.0f) atomicMax(pmax_bits, __float_as_uint(pw));
}

// the workgroup's exclusive prefix sum of v over its PT_LIGHT_SCAN_BLOCK threads (Hillis-Steele in LDS); *total = the sum of all
PTK_DEV uint64_t pt_light_block_scan(uint64_t v, uint64_t* lds, uint64_t* total)
{
    const unsigned t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (unsigned off = 1u; off < PT_LIGHT_SCAN_BLOCK; off <<= 1) {
        const uint64_t add = t >= off ? lds[t - off] : 0ull;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const uint64_t incl = lds[t];
    *total = lds[PT_LIGHT_SCAN_BLOCK - 1];
    __syncthreads();   // (lds may be used again)
    return incl - v;
}

__global__ __launch_bounds__(PT_LIGHT_SCAN_BLOCK) void pt_light_quantise_kernel(const PtRawTriangle* __restrict__ tris, int ntri,
                                                                                const PtRawMaterial* __restrict__ mats, int nmat,
                                                                                const int32_t* __restrict__ lights, int nl,
                                                                                const uint32_t* __restrict__ pmax_bits, uint64_t* __restrict__ cdf,
                                                                                uint32_t* __restrict__ tri_q, uint64_t* __restrict__ tile_sums)
{
    __shared__ uint64_t lds[PT_LIGHT_SCAN_BLOCK];
    const float pmax = __uint_as_float(*pmax_bits);
    const unsigned first = blockIdx.x * PT_LIGHT_SCAN_TILE + threadIdx.x * PT_LIGHT_SCAN_ITEMS;
    uint64_t sum = 0ull;
    for (unsigned k = 0; k < PT_LIGHT_SCAN_ITEMS; ++k) {
        const unsigned i = first + k;
        if (i >= (unsigned)nl) break;
        const int index = lights[i];
        const uint32_t q = pt_light_quantum(pt_light_power(tris, ntri, mats, nmat, index), pmax);
        tri_q[pt_clamp_index(index, ntri)] = q;
        cdf[i + 1u] = q;
        sum += q;
    }
    uint64_t total;
    pt_light_block_scan(sum, lds, &total);
    if (threadIdx.x == 0u) tile_sums[blockIdx.x] = total;
}

// one workgroup: tile_sums[0 .. ntiles) become exclusive prefix sums
__global__ __launch_bounds__(PT_LIGHT_SCAN_BLOCK) void pt_light_tiles_kernel(uint64_t* __restrict__ tile_sums, unsigned ntiles, uint64_t* __restrict__ cdf)
{
    __shared__ uint64_t lds[PT_LIGHT_SCAN_BLOCK];
    const unsigned per = (ntiles + PT_LIGHT_SCAN_BLOCK - 1u) / PT_LIGHT_SCAN_BLOCK;
    const unsigned first = threadIdx.x * per, end = first + per < ntiles ? first + per : ntiles;
    uint64_t sum = 0ull;
    for (unsigned i = first; i < end; ++i) sum += tile_sums[i];
    uint64_t total;
    uint64_t run = pt_light_block_scan(sum, lds, &total);
    for (unsigned i = first; i < end; ++i) {
        const uint64_t v = tile_sums[i];
        tile_sums[i] = run;
        run += v;
    }
    if (threadIdx.x == 0u) cdf[0] = 0ull;
}

__global__ __launch_bounds__(PT_LIGHT_SCAN_BLOCK) void pt_light_scan_kernel(uint64_t* __restrict__ cdf, int nl, const uint64_t* __restrict__ tile_sums)
{
    __shared__ uint64_t lds[PT_LIGHT_SCAN_BLOCK];
    const unsigned first = blockIdx.x * PT_LIGHT_SCAN_TILE + threadIdx.x * PT_LIGHT_SCAN_ITEMS;
    uint64_t q[PT_LIGHT_SCAN_ITEMS];
    uint64_t sum = 0ull;
    for (unsigned k = 0; k < PT_LIGHT_SCAN_ITEMS; ++k) {
        q[k] = first + k < (unsigned)nl ? cdf[first + k + 1u] : 0ull;
        sum += q[k];
    }
    uint64_t total;
    uint64_t run = tile_sums[blockIdx.x] + pt_light_block_scan(sum, lds, &total);
    for (unsigned k = 0; k < PT_LIGHT_SCAN_ITEMS; ++k) {
        run += q[k];
        if (first + k < (unsigned)nl) cdf[first + k + 1u] = run;
    }
}

// ---- pt_env_table: the selection table of an octahedral map's texels (include/pt_shim.h) ----
// pt_light_table's construction with another weight: p_i = ((Le.x + Le.y) + Le.z) * (1 / rc^3), rc the distance of the octahedron's
// point over the texel's centre -- the texel's solid angle up to the constant 4 / N^2 --, 0 unless positive and finite.  The two
// kernels below stand where pt_light_weight_kernel and pt_light_quantise_kernel stand; the two scans are pt_light_table's own
PTK_DEV float pt_env_weight(const float4* __restrict__ texels, int N, unsigned i)
{
    const unsigned col = i & (unsigned)(N - 1), row = i >> (31 - __builtin_clz((unsigned)N));
    const float step = 2.0f / (float)N;
    const f3 P = pt_env_point(((float)col + 0.5f) * step - 1.0f, ((float)row + 0.5f) * step - 1.0f);
    const float rc = pt_sqrt(dot3(P, P));
    const float4 le = texels[i];
    const float pw = ((le.x + le.y) + le.z) * (1.0f / ((rc * rc) * rc));
    return pw > 0.0f && pw < __builtin_inff() ? pw : 0.0f;
}

__global__ __launch_bounds__(PT_LIGHT_SCAN_BLOCK) void pt_env_weight_kernel(const float4* __restrict__ texels, int N, uint32_t* __restrict__ pmax_bits)
{
    const unsigned i = blockIdx.x * PT_LIGHT_SCAN_BLOCK + threadIdx.x;
    if (i >= (unsigned)(N * N)) return;
    const float pw = pt_env_weight(texels, N, i);
    if (pw > 0.0f) atomicMax(pmax_bits, __float_as_uint(pw));
}

__global__ __launch_bounds__(PT_LIGHT_SCAN_BLOCK) void pt_env_quantise_kernel(const float4* __restrict__ texels, int N, const uint32_t* __restrict__ pmax_bits,
                                                                              uint64_t* __restrict__ cdf, uint64_t* __restrict__ tile_sums)
{
    __shared__ uint64_t lds[PT_LIGHT_SCAN_BLOCK];
    const float pmax = __uint_as_float(*pmax_bits);
    const unsigned nl = (unsigned)(N * N);
    const unsigned first = blockIdx.x * PT_LIGHT_SCAN_TILE + threadIdx.x * PT_LIGHT_SCAN_ITEMS;
    uint64_t sum = 0ull;
    for (unsigned k = 0; k < PT_LIGHT_SCAN_ITEMS; ++k) {
        const unsigned i = first + k;
        if (i >= nl) break;
        const uint32_t q = pt_light_quantum(pt_env_weight(texels, N, i), pmax);
        cdf[i + 1u] = q;
        sum += q;
    }
    uint64_t total;
    pt_light_block_scan(sum, lds, &total);
    if (threadIdx.x == 0u) tile_sums[blockIdx.x] = total;
}

// :241, in that order
PTK_DEV void pt_indirect_emission(const PtDirectParams& D, unsigned mid, const f3& mask, f3& L)
{
    const float4 emi = pt_rec16(D.t.mats, mid, 16u);
    L.x = L.x + mask.x * emi.x * 3.0f;
    L.y = L.y + mask.y * emi.y * 3.0f;
    L.z = L.z + mask.z * emi.z * 3.0f;
}

// (MIS) the emission of a vertex i >= 1, found by the BRDF ray (o, d) at distance t, weighted against the light samples of the vertex
// before: pe is the density those give the same point -- from the hit triangle's record N = cross(e2, e1), its own distance
// tt = t + 0.01f (the ray began 0.01 off that vertex, :257) and its count --, pb the density of the BRDF sample that made the ray.
// A material with no emissive component reads no count and adds nothing.  POWER: total / tri_q[h] stands where (float)nl stands, formed
// when counts[h] > 0; with counts[h] = 0 the weight is 1 and the table is not read
template <bool POWER = false>
PTK_DEV void pt_indirect_emission_mis(const PtDirectParams& D, const int32_t* counts, unsigned mid, int hidx, const f3& d, float t, float pb,
                                      const f3& mask, f3& L, const uint64_t* cdf = nullptr, const uint32_t* tri_q = nullptr)
{
    const float4 emi = pt_rec16(D.t.mats, mid, 16u);
    if (!(emi.x != 0.0f || emi.y != 0.0f || emi.z != 0.0f)) return;
    const float4 nid = pt_rec16(D.t.tris, (unsigned)hidx, 48u);
    const f3 N = mk3(nid.x, nid.y, nid.z);
    const float N2 = dot3(N, N);
    const float areah = 0.5f * pt_sqrt(N2);
    const float clh = __builtin_fabsf(dot3(d, scale3(N, pt_normalize_factor(N2))));
    const float tt = t + 0.01f;
    float wb;
    if constexpr (POWER) {
        const int cnt = counts[hidx];
        wb = 1.0f;
        if (cnt > 0) {
            const float invh = (float)cdf[D.nl] / (float)tri_q[hidx];
            const float pe = (tt * tt) / (clh * (areah * invh));
            wb = pb / (((float)D.K * pe) * (float)cnt + pb);
        }
    } else {
        const float pe = (tt * tt) / (clh * (areah * (float)D.nl));
        wb = pb / (((float)D.K * pe) * (float)counts[hidx] + pb);
    }
    L.x = L.x + ((mask.x * emi.x) * 3.0f) * wb;
    L.y = L.y + ((mask.y * emi.y) * 3.0f) * wb;
    L.z = L.z + ((mask.z * emi.z) * 3.0f) * wb;
}

// the emission of vertex i as the kind adds it: whole at the first vertex and without lights; at a later vertex weighted (MIS), or not at
// all -- there the light samples of the vertex before have counted it
template <unsigned KIND>
PTK_DEV void pt_kind_emission(const PtKindArgs<KIND>& I, int i, unsigned mid, int hidx, const f3& d, float t, float pb, const f3& mask, f3& L)
{
    using K = PtKindOf<KIND>;
    if (i == 0 || I.d.nl == 0) pt_indirect_emission(I.d, mid, mask, L);
    else if constexpr (K::mis && K::power) pt_indirect_emission_mis<true>(I.d, I.counts, mid, hidx, d, t, pb, mask, L, I.cdf, I.tri_q);
    else if constexpr (K::mis) pt_indirect_emission_mis(I.d, I.counts, mid, hidx, d, t, pb, mask, L);
}

// L += mask * (S / K) of a vertex's light samples
PTK_DEV void pt_indirect_lit(const PtDirectParams& D, const f3& mask, const f3& S, f3& L)
{
    const float Kf = (float)D.K;
    L.x = L.x + mask.x * (S.x / Kf);
    L.y = L.y + mask.y * (S.y / Kf);
    L.z = L.z + mask.z * (S.z / Kf);
}

PTK_DEV void pt_indirect_store(const PtDirectParams& D, unsigned item, const f3& L)   // :260
{
    pt_direct_store(D, item, mk3(pt_max(L.x, 0.0f), pt_max(L.y, 0.0f), pt_max(L.z, 0.0f)));
}

// Russian roulette (pt_render_indirect_rr, whose contract states every step) at a vertex where it applies -- the caller has checked
// i + 1 >= R and i < B - 1 --, after pt_indirect_bounce has returned true: the uniform is drawn whatever follows; q = min(max channel
// of mask, cap) with the reference's max and min (a NaN in mask.x, or in both others, makes q NaN); q >= 1 leaves the path as it is
// (the uniform can be 1.0); otherwise the path goes on when r < q -- false for a NaN q and for q <= 0 -- with mask / q, three IEEE
// divisions (q has no proven window: no short form).  False: the path ends as a pdf <= 0 path does
PTK_DEV bool pt_roulette(float cap, uint32_t& seed, f3& mask)
{
    const float r = pt_random_float(seed);
    const float s = pt_max(mask.x, pt_max(mask.y, mask.z));
    const float q = cap < s ? cap : s;
    if (q >= 1.0f) return true;
    if (!(r < q)) return false;
    mask.x = mask.x / q;
    mask.y = mask.y / q;
    mask.z = mask.z / q;
    return true;
}

// brute force: one wave = 64 consecutive samples, pt_direct_kernel's shape inside a loop over the bounces.  The wave searches in step
// with the lanes still alive and leaves the loop when none is; a light sample no lane casts a ray for costs no search.  Lanes whose
// path has ended are NOT given new samples: the wave runs as long as its longest path (DESIGN.md S4 states the cost).
template <bool DET_BOUNDED, int LDS_TABLE, int QUADS, unsigned KIND>
__global__ __launch_bounds__(PT_TRACE_THREADS) void pt_indirect_kernel(const PtKindArgs<KIND> I)
{
    constexpr bool MIS = PtKindOf<KIND>::mis;
    static_assert(PtKindOf<KIND>::indirect && !PtKindOf<KIND>::rr, "the roulette kinds' table kernel is pt_indirect_rr_kernel");
    const PtDirectParams& D = I.d;
    const PtTraceParams& P = D.t;
    const unsigned lane = pt_lane_id();
    const int ntri = P.ntri;
    PtTail tl = pt_table_wg_setup<LDS_TABLE>(P, lane);
    const f3 anchor = mk3(P.cam.eye[0], P.cam.eye[1], P.cam.eye[2]);
    const unsigned item = pt_wave() * 64u + lane;
    const bool act = item < D.nitems;
    unsigned lp = 0u;
    uint32_t seed = 0u;
    f3 o = mk3(0.0f, 0.0f, 0.0f), d = mk3(0.0f, 0.0f, 1.0f);
    if (act) pt_item_begin(P, D.cam, D.npix, D.frame0, item, lp, seed, o, d);
    f3 L = mk3(0.0f, 0.0f, 0.0f), mask = mk3(1.0f, 1.0f, 1.0f);
    [[maybe_unused]] float pb = 0.0f;   // (MIS) the pdf of the BRDF sample that made the current ray
    bool alive = act;
    for (int i = 0; i < I.B; ++i) {
        float tmax = 1e20f, hu = 0.0f, hv = 0.0f;
        int hidx = -1;
        pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, alive, tmax, hu, hv, hidx,
                                                             P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
        const bool hit = alive & (hidx >= 0);
        if (alive & !hit) L = add3(L, scale3(mask, pt_max(0.45f, 0.0f)));   // :235
        alive = hit;
        if (__ballot(hit) == 0ull) break;
        f3 p = o, n = d, wo = d;
        unsigned mid = 0u;
        if (hit) {
            pt_direct_surface(D, o, d, tmax, hu, hv, hidx, p, n, wo, mid);
            pt_kind_emission<KIND>(I, i, mid, hidx, d, tmax, pb, mask, L);
        }
        if (D.nl > 0) {
            f3 S = mk3(0.0f, 0.0f, 0.0f);
            for (int k = 0; k < D.K; ++k) {
                f3 c = mk3(0.0f, 0.0f, 0.0f);
                float tlim = 0.0f;
                bool cast = false;
                if (hit) cast = pt_kind_light<KIND>(I, D, p, n, wo, mid, seed, c, o, d, tlim, i < I.B - 1);
                const bool live = cast & (tlim > 0.0f);
                bool occluded = false;
                if (__ballot(live) != 0ull) {
                    float t = live ? tlim : 0.0f, su = 0.0f, sv = 0.0f;
                    int sidx = -1;
                    pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, live, t, su, sv, sidx,
                                                                         P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
                    occluded = live & (sidx >= 0) & (t < tlim);   // pt_query_store's occlusion test
                }
                if (cast & !occluded) S = add3(S, c);
            }
            if (hit) pt_indirect_lit(D, mask, S, L);
        }
        if (i == I.B - 1) break;   // (the last vertex's draw cannot be observed)
        if (hit) alive = pt_indirect_bounce<MIS>(D, p, n, wo, mid, seed, mask, o, d, &pb);
        if (__ballot(alive) == 0ull) break;
    }
    if (act) pt_indirect_store(D, item, L);
}

// the start of item `item` of a LIST launch (PtIndirectListParams; pt_render_indirect_pixels): frame f = item / listed pixels of slot
// j = item % listed pixels -- one 8-byte vector load, consecutive lanes consecutive slots --, the slot's pixel clamped into the local
// image (an out-of-range slot is defined behaviour, as a light index is), its own frame number; from there on pt_item_begin's sample
PTK_DEV void pt_list_item_begin(const PtIndirectListParams& I, unsigned item, unsigned& lp, uint32_t& seed, f3& o, f3& d)
{
    const PtTraceParams& P = I.d.t;
    const unsigned f = item / I.d.npix;
    const uint2 slot = I.slots[item - f * I.d.npix];
    lp = slot.x < P.npix_local ? slot.x : P.npix_local - 1u;
    const uint32_t frame = (slot.y + I.frame_off + f) & 0x7fffffffu;
    unsigned x, grow;
    pt_pixel_xy<false>(P, nullptr, lp, x, grow);
    const unsigned gid = grow * (unsigned)P.width + x;
    seed = gid + pt_hash_u32(frame);
    pt_generate_lens_ray((int)x, (int)grow, P.inv_width, P.inv_height, P.aspect, I.d.cam, seed, o, d);
}

// the start of item `item` of a RAYS launch (PtIndirectRaysParams; pt_radiance_rays): sample s = item / rays of ray r = item % rays.  Its
// seed is the renderers' gid + pt_hash_u32(frame) with gid = first_ray + r and frame = frame0 + s, in uint32; its primary ray is the
// record's, loaded and normalised as a query's (pt_query_load: two 16-byte vector loads per lane, consecutive lanes consecutive 32-byte
// records -- 2 KiB contiguous per wave).  No uniform is drawn, and tmax and reserved are loaded with their float4 but not read
PTK_DEV void pt_ray_item_begin(const PtIndirectRaysParams& I, unsigned item, uint32_t& seed, f3& o, f3& d)
{
    const unsigned s = item / I.d.npix;
    const unsigned r = item - s * I.d.npix;
    seed = (I.first_ray + r) + pt_hash_u32((uint32_t)I.d.frame0 + s);
    const PtQueryRay q = pt_query_load(I.rays, r);
    o = q.o;
    d = q.d;
}

// Brute force with Russian roulette (pt_render_indirect_rr): a NEW kernel beside pt_indirect_kernel, which stays as it is.  Roulette
// shortens the average path, hardly the longest of 64, so in a kernel that walks 64 samples in lock step it would only empty the exec
// mask.  Here a wave owns a contiguous RUN of PT_RR_RUN items, [run0, end), and REFILLS: at the top of every iteration the lanes whose
// path has ended and been stored take the next unstarted items of the run, in lane order (a ballot of the dead lanes and its mbcnt
// prefix: no atomics, no state shared between waves).  A sample's value depends on its item alone (pt_item_begin: the pixel and the
// frame give the seed; pt_indirect_store: samples[item]), so which lane walks it changes no bit.  The bounce index is per lane.  The
// searches, the light samples and the bounce are pt_indirect_kernel's calls in its order.
// Termination: an iteration starts with at least one live lane (else the wave leaves: no lane alive means the refill found the run
// exhausted), and every live lane either ends its path in it or raises its bounce, which is below B; every refill raises `next`,
// which is at most `end`.  So a wave runs at most PT_RR_RUN * B iterations.  No spin, no persistent grid.
// The kind's bits (PtKindOf):
// list (pt_render_indirect_pixels): the items are frames of a list of pixels; only the sample's start differs (pt_list_item_begin)
// rays (pt_radiance_rays): the items are samples of the caller's rays; only the sample's start differs (pt_ray_item_begin).  No pin:
// the compiler holds every form at its parent's waves per SIMD (profiles/radiance/kernel_resources.txt)
// ris (pt_render_indirect_ris, pt_render_indirect_pixels_ris): the light sample is pt_ris_light's -- the candidates of the wave's
// lanes in step, then the one shadow search, none when no lane holds a candidate.  These forms carry an occupancy pin, the parents'
// six waves per SIMD (80 VGPRs): unpinned the compiler takes 81-82 registers for a loop it holds in 80 without a spill.  The tiled MIS
// forms are the exception: at six waves they spill 3 VGPRs (16 bytes of scratch), so they are pinned to the five they need (85 VGPRs,
// no scratch); profiles/ris/kernel_resources.txt has both figures.  A pin of 0 is no pin: the attribute is not emitted
#ifndef PT_RR_RIS_TILED_MIS_WAVES   // (tools/kernel_resources.sh -DPT_RR_RIS_TILED_MIS_WAVES=6 reads the other choice)
#define PT_RR_RIS_TILED_MIS_WAVES 5
#endif
// env (pt_render_indirect_env): a miss adds mask times the map's texel -- weighted against the environment samples of the vertex
// before when i >= 1 and Ke > 0 --, and the Ke environment samples of a vertex follow its K light samples in the same shape, a search
// only when some lane casts.  Their pin is the parents' six waves per SIMD for the tiled forms; the forms with the table in LDS would
// spill a VGPR at six (8 bytes of scratch) and are pinned to five (profiles/env/kernel_resources.txt has both figures)
#ifndef PT_RR_ENV_LDS_WAVES   // (tools/kernel_resources.sh -DPT_RR_ENV_LDS_WAVES=6 reads the other choice)
#define PT_RR_ENV_LDS_WAVES 5
#endif
constexpr int pt_rr_waves_pin(unsigned kind, int lds_table)
{
    const PtLitKind k = ptk_lit_kind_of(kind);
    return k.env ? (lds_table == 1 ? PT_RR_ENV_LDS_WAVES : 6) : !k.ris ? 0 : (lds_table == 2 && k.mis) ? PT_RR_RIS_TILED_MIS_WAVES : 6;
}
template <bool DET_BOUNDED, int LDS_TABLE, int QUADS, unsigned KIND>
__global__ __launch_bounds__(PT_TRACE_THREADS) __attribute__((amdgpu_waves_per_eu(pt_rr_waves_pin(KIND, LDS_TABLE))))
void pt_indirect_rr_kernel(const PtKindArgs<KIND> I)
{
    using K = PtKindOf<KIND>;
    constexpr bool MIS = K::mis, LIST = K::list, ENV = K::env, RAYS = K::rays;
    static_assert(K::rr, "the refilling kernel is the roulette kinds'");
    static_assert(PT_RR_RUN % 64 == 0 && PT_RR_RUN >= 64, "a run is whole waves of items");
    const PtDirectParams& D = I.d;
    const PtTraceParams& P = D.t;
    const unsigned lane = pt_lane_id();
    const int ntri = P.ntri;
    PtTail tl = pt_table_wg_setup<LDS_TABLE>(P, lane);
    const f3 anchor = mk3(P.cam.eye[0], P.cam.eye[1], P.cam.eye[2]);
    // the run (wave-uniform): nitems < 2^31 and the grid is ceil(nitems / PT_RR_RUN) waves rounded up to workgroups, so run0 fits
    const unsigned run0 = pt_wave() * (unsigned)PT_RR_RUN;
    unsigned next = run0 < D.nitems ? run0 : D.nitems;
    const unsigned end = D.nitems - next < (unsigned)PT_RR_RUN ? D.nitems : next + (unsigned)PT_RR_RUN;
    unsigned item = 0u;
    uint32_t seed = 0u;
    int i = 0;   // the lane's bounce: loop index i of traceRays (:229)
    f3 o = mk3(0.0f, 0.0f, 0.0f), d = mk3(0.0f, 0.0f, 1.0f);
    f3 L = mk3(0.0f, 0.0f, 0.0f), mask = mk3(1.0f, 1.0f, 1.0f);
    [[maybe_unused]] float pb = 0.0f;   // (MIS) the pdf of the BRDF sample that made the current ray
    bool alive = false;
    for (;;) {
        // refill: the dead lane of rank r among the dead takes item next + r while the run lasts
        const unsigned long long dead = __ballot(!alive);
        if (!alive) {
            const unsigned it = next + pt_mbcnt(dead);
            if (it < end) {
                [[maybe_unused]] unsigned lp;
                item = it;
                if constexpr (RAYS) pt_ray_item_begin(I, item, seed, o, d);
                else if constexpr (LIST) pt_list_item_begin(I, item, lp, seed, o, d);
                else pt_item_begin(P, D.cam, D.npix, D.frame0, item, lp, seed, o, d);
                L = mk3(0.0f, 0.0f, 0.0f);
                mask = mk3(1.0f, 1.0f, 1.0f);
                i = 0;
                alive = true;
            }
        }
        const unsigned ndead = (unsigned)__popcll(dead);
        next = end - next < ndead ? end : next + ndead;
        if (__ballot(alive) == 0ull) break;   // the run is exhausted and every path stored

        float tmax = 1e20f, hu = 0.0f, hv = 0.0f;
        int hidx = -1;
        pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, alive, tmax, hu, hv, hidx,
                                                             P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
        const bool hit = alive & (hidx >= 0);
        if constexpr (ENV) {
            if (alive & !hit) {
                const f3 le = pt_env_miss(I.env, d, i >= 1 && I.env.Ke > 0, pb);
                L = mk3(L.x + mask.x * le.x, L.y + mask.y * le.y, L.z + mask.z * le.z);
            }
        } else {
            if (alive & !hit) L = add3(L, scale3(mask, pt_max(0.45f, 0.0f)));   // :235
        }
        f3 p = o, n = d, wo = d;
        unsigned mid = 0u;
        if (hit) {
            pt_direct_surface(D, o, d, tmax, hu, hv, hidx, p, n, wo, mid);
            pt_kind_emission<KIND>(I, i, mid, hidx, d, tmax, pb, mask, L);
        }
        if (D.nl > 0 && __ballot(hit) != 0ull) {
            f3 S = mk3(0.0f, 0.0f, 0.0f);
            for (int k = 0; k < D.K; ++k) {
                f3 c = mk3(0.0f, 0.0f, 0.0f);
                float tlim = 0.0f;
                bool cast = false;
                if (hit) cast = pt_kind_light<KIND>(I, D, p, n, wo, mid, seed, c, o, d, tlim, i < I.B - 1);
                const bool live = cast & (tlim > 0.0f);
                bool occluded = false;
                if (__ballot(live) != 0ull) {
                    float t = live ? tlim : 0.0f, su = 0.0f, sv = 0.0f;
                    int sidx = -1;
                    pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, live, t, su, sv, sidx,
                                                                         P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
                    occluded = live & (sidx >= 0) & (t < tlim);   // pt_query_store's occlusion test
                }
                if (cast & !occluded) S = add3(S, c);
            }
            if (hit) pt_indirect_lit(D, mask, S, L);
        }
        if constexpr (ENV) {
            if (I.env.Ke > 0 && __ballot(hit) != 0ull) {
                f3 S = mk3(0.0f, 0.0f, 0.0f);
                for (int k = 0; k < I.env.Ke; ++k) {
                    f3 c = mk3(0.0f, 0.0f, 0.0f);
                    bool cast = false;
                    if (hit) cast = pt_env_light<true>(D, I.env, p, n, wo, mid, seed, c, o, d, i < I.B - 1);
                    bool occluded = false;
                    if (__ballot(cast) != 0ull) {
                        float t = cast ? 1e20f : 0.0f, su = 0.0f, sv = 0.0f;
                        int sidx = -1;
                        pt_intersect_two_pass<DET_BOUNDED, LDS_TABLE, QUADS>((pt_const_f32p)(const float*)P.tris, P.tris, ntri, o, d, cast, t, su, sv, sidx,
                                                                             P.quad_delta1, P.ray_radius, (pt_const_f32p)P.p1tab, P.p1_lo, P.p1_hi, anchor, tl, lane);
                        occluded = cast & (sidx >= 0) & (t < 1e20f);
                    }
                    if (cast & !occluded) S = add3(S, c);
                }
                if (hit) pt_env_lit(I.env.Ke, mask, S, L);
            }
        }
        // the BRDF sample and the roulette of vertex i; at the last vertex nothing is drawn
        bool on = false;
        if (hit && i < I.B - 1) {
            on = pt_indirect_bounce<MIS>(D, p, n, wo, mid, seed, mask, o, d, &pb);
            if (on && i + 1 >= I.R) on = pt_roulette(I.cap, seed, mask);
        }
        if (alive & !on) pt_indirect_store(D, item, L);   // a miss, pdf <= 0, the roulette, or the depth
        alive = on;
        ++i;
    }
}

// LBVH (pt_bvh_drive): one item = one sample; the lane walks its path as a sequence of searches -- per vertex the closest search, then
// the any-hit searches of the light samples that contribute -- and is free only when the sample is stored.  next_ray is the state
// machine between two searches: a closest result leads to the surface, the emission and the first contributing light sample; an
// any-hit result to the next contributing one; after the last comes the BRDF sample and the next closest search, or the store.
// Between searches a lane holds PtDirectWork's state (the surface p, n, wo, the material's INDEX, S, c) and mask, L and the bounce.
// wo is the negated incoming direction, which the shadow rays overwrite in d, so it is kept; o is dead while p is live.
// With MIS a lane also holds pb from the BRDF sample to the next closest hit, across that search: 34 registers.  The counts and the
// emitter's record are gathered where they are used, as the materials are.
// ENV: k goes on over K .. K + Ke - 1, the environment samples of the vertex.  S / K is folded into L before the first of them and S
// starts again as Se: a lane's state does not grow
template <unsigned KIND>
struct PtIndirectWork {
    using K = PtKindOf<KIND>;
    static constexpr bool ANY = true, MIS = K::mis, RR = K::rr, LIST = K::list, ENV = K::env, RAYS = K::rays;
    const PtKindArgs<KIND>& I;
    unsigned n;
    int k;           // the current ray: -1 = the vertex's closest search, 0 .. K-1 = the shadow ray of light sample k
    int bounce;      // loop index i of traceRays (:229)
    unsigned item, mid;
    uint32_t seed;
    float tl;        // the shadow ray's limit
    f3 o, d, p, nrm, wo, S, c, mask, L;
    float pb;        // (MIS; otherwise never touched) the pdf of the BRDF sample that made the current ray
    PTK_DEV void begin(unsigned item_)
    {
        [[maybe_unused]] unsigned lp;
        item = item_;
        if constexpr (RAYS) pt_ray_item_begin(I, item, seed, o, d);
        else if constexpr (LIST) pt_list_item_begin(I, item, lp, seed, o, d);
        else pt_item_begin(I.d.t, I.d.cam, I.d.npix, I.d.frame0, item, lp, seed, o, d);
        k = -1;
        bounce = 0;
        mask = mk3(1.0f, 1.0f, 1.0f);
        L = mk3(0.0f, 0.0f, 0.0f);
    }
    PTK_DEV bool next_ray(const PtBvhLane& R)
    {
        const PtDirectParams& D = I.d;
        if (k < 0) {
            if (R.hidx < 0) {
                if constexpr (ENV) {
                    const f3 le = pt_env_miss(I.env, d, bounce >= 1 && I.env.Ke > 0, pb);
                    L = mk3(L.x + mask.x * le.x, L.y + mask.y * le.y, L.z + mask.z * le.z);
                } else {
                    L = add3(L, scale3(mask, pt_max(0.45f, 0.0f)));   // :235
                }
                pt_indirect_store(D, item, L);
                return false;
            }
            pt_direct_surface(D, o, d, R.tmax, R.hu, R.hv, R.hidx, p, nrm, wo, mid);
            pt_kind_emission<KIND>(I, bounce, mid, R.hidx, d, R.tmax, pb, mask, L);
            S = mk3(0.0f, 0.0f, 0.0f);
        } else if (R.hidx < 0) {   // (an any-hit search: R.hidx >= 0 alone says occluded; a ray that searched nothing is open)
            S = add3(S, c);
        }
        if constexpr (ENV) {
            if (k < D.K) {   // the light samples are not over (k = -1 among them)
                if (D.nl > 0) {
                    while (++k < D.K)
                        if (pt_kind_light<KIND>(I, D, p, nrm, wo, mid, seed, c, o, d, tl, bounce < I.B - 1)) return true;
                    pt_indirect_lit(D, mask, S, L);
                    S = mk3(0.0f, 0.0f, 0.0f);
                }
                k = D.K - 1;
            }
            tl = 1e20f;
            while (++k < D.K + I.env.Ke)
                if (pt_env_light<true>(D, I.env, p, nrm, wo, mid, seed, c, o, d, bounce < I.B - 1)) return true;
            if (I.env.Ke > 0) pt_env_lit(I.env.Ke, mask, S, L);
        } else if (D.nl > 0) {
            while (++k < D.K) {
                if (pt_kind_light<KIND>(I, D, p, nrm, wo, mid, seed, c, o, d, tl, bounce < I.B - 1)) return true;
            }
            pt_indirect_lit(D, mask, S, L);
        }
        bool on;
        if constexpr (MIS) on = ++bounce < I.B && pt_indirect_bounce<true>(D, p, nrm, wo, mid, seed, mask, o, d, &pb);
        else on = ++bounce < I.B && pt_indirect_bounce(D, p, nrm, wo, mid, seed, mask, o, d);
        if constexpr (RR) {   // (the vertex is i = bounce - 1: i + 1 >= R, and on says i < B - 1)
            if (on && bounce >= I.R) on = pt_roulette(I.cap, seed, mask);
        }
        if (on) {
            k = -1;
            return true;
        }
        pt_indirect_store(D, item, L);
        return false;
    }
    PTK_DEV const f3& org() const { return o; }
    PTK_DEV const f3& dir() const { return d; }
    PTK_DEV float limit() const { return k < 0 ? 1e20f : tl; }
    PTK_DEV bool live() const { return k < 0 || tl > 0.0f; }
    PTK_DEV bool any() const { return k >= 0; }
};

// Three waves per SIMD (168 VGPRs), chosen from the compiler's resource report (profiles/indirect/kernel_resources.txt): a path's
// state between its searches is 33 registers against direct's 25, and at direct's four waves (128 VGPRs) the kernel spills 25 of
// them to scratch; at three it uses 158-159 and spills none.  Its persistent grid is its own figure, ptk_lit_bvh_blocks_per_cu of its kind.
// The MIS instantiations use 163-164 of the 168 at the same three waves and spill none either (profiles/mis/kernel_resources.txt);
// their grid figure is their own kind's (the same occupancy, asked of their own code objects)
#ifndef PT_INDIRECT_BVH_WAVES   // (tools/kernel_resources.sh -DPT_INDIRECT_BVH_WAVES=4 reads the other choice)
#define PT_INDIRECT_BVH_WAVES 3
#endif
// The other kinds keep the three waves: what their blocks add is scalar (R and cap, the slot pointer and the frame offset, the ray
// pointer and first_ray, M), and what they load dies where it is used -- the roulette's r, s and q, the slot and the ray record in
// begin(), the reservoir inside pt_ris_light (profiles/roulette, adaptive, radiance, ris: kernel_resources.txt)
// The env kinds: the map's fields are scalar, Se shares S's registers.  They run at TWO waves: at three they would spill 37 VGPRs
// inside next_ray (profiles/env/kernel_resources.txt has both figures)
#ifndef PT_INDIRECT_ENV_BVH_WAVES   // (tools/kernel_resources.sh -DPT_INDIRECT_ENV_BVH_WAVES=3 reads the other choice)
#define PT_INDIRECT_ENV_BVH_WAVES 2
#endif
constexpr int pt_indirect_bvh_waves(unsigned kind) { return ptk_lit_kind_of(kind).env ? PT_INDIRECT_ENV_BVH_WAVES : PT_INDIRECT_BVH_WAVES; }
template <bool DET_BOUNDED, int BIGQ, unsigned KIND>
__global__ __launch_bounds__(PT_TRACE_THREADS) __attribute__((amdgpu_waves_per_eu(pt_indirect_bvh_waves(KIND), pt_indirect_bvh_waves(KIND))))
void pt_indirect_bvh_kernel(const PtKindArgs<KIND> I)
{
    const f3 o0 = mk3(0.0f, 0.0f, 0.0f), d0 = mk3(0.0f, 0.0f, 1.0f);
    PtIndirectWork<KIND> W = { I, I.d.nitems, -1, 0, 0u, 0u, 0u, 0.0f, o0, d0, o0, d0, d0, o0, o0, o0, o0, 0.0f };
    pt_bvh_drive<DET_BOUNDED, BIGQ>(I.d.t, W);
}

// ---- sample moments (pt_sample_moments, pt_moments_resolve; include/pt_shim.h states every step) ----
// pt_sample_moments_kernel: one lane per pixel, so that the pixel's sums are taken over the frames in ascending order by one lane and
// equal a sequential restatement bit for bit.  Consecutive lanes read consecutive 12-byte records (768 contiguous bytes per wave and
// frame).  A 256 x 256 image is four waves per CU: the loads of PT_MOMENTS_UNROLL frames are issued before the first of them is
// used, so that the kernel waits for memory once per eight frames, not once per frame.  The 56-byte record is read (unless reset) and
// written once per call.
PTK_DEV bool pt_moments_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

struct PtMomentsAcc {
    double s0, s1, s2, q0, q1, q2;
    uint32_t n, rejected;
};

// the product of two converted binary32 values is exact in binary64: contraction could not change q
PTK_DEV void pt_moments_add(PtMomentsAcc& a, float x, float y, float z)
{
    if (pt_moments_finite(x) && pt_moments_finite(y) && pt_moments_finite(z)) {
        const double dx = (double)x, dy = (double)y, dz = (double)z;
        a.n += 1u;
        a.s0 = a.s0 + dx;
        a.s1 = a.s1 + dy;
        a.s2 = a.s2 + dz;
        a.q0 = a.q0 + dx * dx;
        a.q1 = a.q1 + dy * dy;
        a.q2 = a.q2 + dz * dz;
    } else {
        a.rejected += 1u;
    }
}

__global__ __launch_bounds__(256) void pt_sample_moments_kernel(const float* __restrict__ samples, PtPixelMoments* __restrict__ moments,
                                                                uint32_t npix, int32_t frames, int reset)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= npix) return;
    PtMomentsAcc a = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0u, 0u };
    if (!reset) {
        const PtPixelMoments& m = moments[p];
        a.s0 = m.sum[0], a.s1 = m.sum[1], a.s2 = m.sum[2];
        a.q0 = m.sum2[0], a.q1 = m.sum2[1], a.q2 = m.sum2[2];
        a.n = m.n, a.rejected = m.rejected;
    }
    const size_t stride = (size_t)npix * 3u;                 // floats per frame
    const float* src = samples + (size_t)p * 3u;
    int32_t f = 0;
    for (; f + PT_MOMENTS_UNROLL <= frames; f += PT_MOMENTS_UNROLL) {
        float v[PT_MOMENTS_UNROLL][3];
#pragma unroll
        for (int k = 0; k < PT_MOMENTS_UNROLL; ++k) {
            const float* r = src + (size_t)k * stride;
            v[k][0] = r[0], v[k][1] = r[1], v[k][2] = r[2];
        }
#pragma unroll
        for (int k = 0; k < PT_MOMENTS_UNROLL; ++k) pt_moments_add(a, v[k][0], v[k][1], v[k][2]);
        src += (size_t)PT_MOMENTS_UNROLL * stride;
    }
    for (; f < frames; ++f) {
        pt_moments_add(a, src[0], src[1], src[2]);
        src += stride;
    }
    PtPixelMoments& o = moments[p];
    o.sum[0] = a.s0, o.sum[1] = a.s1, o.sum[2] = a.s2;
    o.sum2[0] = a.q0, o.sum2[1] = a.q1, o.sum2[2] = a.q2;
    o.n = a.n, o.rejected = a.rejected;
}

// pt_moments_resolve_kernel: a workgroup owns a tile of PT_MOMENTS_TILE consecutive elements and reduces it by adjacent-pair
// butterflies -- eleven levels of x'[i] = x[2 i] + x[2 i + 1] over the tile padded with +0 --, which is the fixed tree of the contract
// for the tile; the same kernel run on the tile sums continues the tree.  (A level's pair sum is formed in both lanes of the pair,
// from the same two operands: IEEE addition commutes.)  Level 0 (moments != NULL) resolves the pixels' records -- and writes `noise`
// when given --; later levels (in != NULL) read the sums of the level before.  The three counters are integers: any order.
// out == NULL (noise only) reduces nothing.
PTK_DEV double pt_moments_pair(double x, int lane_mask) { return x + __shfl_xor(x, lane_mask, 64); }
PTK_DEV unsigned long long pt_moments_pair(unsigned long long x, int lane_mask) { return x + __shfl_xor(x, lane_mask, 64); }

__global__ __launch_bounds__(256) void pt_moments_resolve_kernel(const PtPixelMoments* __restrict__ moments, const PtNoiseSummary* __restrict__ in,
                                                                 uint32_t count, uint4* __restrict__ noise, PtNoiseSummary* __restrict__ out)
{
    constexpr unsigned ROUNDS = PT_MOMENTS_TILE / 256u, PARTS = PT_MOMENTS_TILE / 64u;   // 8 rounds of 256 elements; 32 wave sums
    __shared__ double lds_f[3][PARTS];
    __shared__ unsigned long long lds_u[3][PARTS];
    const uint32_t tile = blockIdx.x * PT_MOMENTS_TILE;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (unsigned r = 0; r < ROUNDS; ++r) {
        const uint32_t i = tile + r * 256u + threadIdx.x;
        double a = 0.0, b = 0.0, c = 0.0;
        unsigned long long px = 0ull, ns = 0ull, rj = 0ull;
        if (i < count) {
            if (moments) {
                const PtPixelMoments& m = moments[i];
                const uint32_t n = m.n;
                const double nd = (double)n;
                double mean[3], var[3] = { 0.0, 0.0, 0.0 };
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    mean[ch] = n ? m.sum[ch] / nd : 0.0;
                    if (n >= 2u) {
                        const double t = m.sum[ch] * mean[ch];
                        const double d = m.sum2[ch] - t;
                        const double v = d / (double)(n - 1u);
                        var[ch] = v > 0.0 ? v : 0.0;
                    }
                }
                if (noise) noise[i] = make_uint4(__float_as_uint((float)var[0]), __float_as_uint((float)var[1]), __float_as_uint((float)var[2]), n);
                if (n >= 2u) {
                    a = (var[0] + var[1]) + var[2];
                    b = ((var[0] / nd) + (var[1] / nd)) + (var[2] / nd);
                    c = ((mean[0] * mean[0]) + (mean[1] * mean[1])) + (mean[2] * mean[2]);
                    px = 1ull;
                }
                ns = n;
                rj = m.rejected;
            } else {
                const PtNoiseSummary& s = in[i];
                a = s.var_sum, b = s.se2_sum, c = s.mean2_sum;
                px = s.pixels, ns = s.samples, rj = s.rejected;
            }
        }
        if (!out) continue;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            a = pt_moments_pair(a, k), b = pt_moments_pair(b, k), c = pt_moments_pair(c, k);
            px = pt_moments_pair(px, k), ns = pt_moments_pair(ns, k), rj = pt_moments_pair(rj, k);
        }
        if (lane == 0u) {
            const unsigned part = r * 4u + wave;
            lds_f[0][part] = a, lds_f[1][part] = b, lds_f[2][part] = c;
            lds_u[0][part] = px, lds_u[1][part] = ns, lds_u[2][part] = rj;
        }
    }
    if (!out) return;
    __syncthreads();
    if (wave != 0u) return;
    // the 32 wave sums, padded with +0 to the wave: five more levels
    const bool live = lane < PARTS;
    double a = live ? lds_f[0][lane & (PARTS - 1u)] : 0.0, b = live ? lds_f[1][lane & (PARTS - 1u)] : 0.0, c = live ? lds_f[2][lane & (PARTS - 1u)] : 0.0;
    unsigned long long px = live ? lds_u[0][lane & (PARTS - 1u)] : 0ull, ns = live ? lds_u[1][lane & (PARTS - 1u)] : 0ull,
                       rj = live ? lds_u[2][lane & (PARTS - 1u)] : 0ull;
#pragma unroll
    for (int k = 1; k < (int)PARTS; k <<= 1) {
        a = pt_moments_pair(a, k), b = pt_moments_pair(b, k), c = pt_moments_pair(c, k);
        px = pt_moments_pair(px, k), ns = pt_moments_pair(ns, k), rj = pt_moments_pair(rj, k);
    }
    if (lane == 0u) {
        PtNoiseSummary& o = out[blockIdx.x];
        o.var_sum = a, o.se2_sum = b, o.mean2_sum = c;
        o.pixels = px, o.samples = ns, o.rejected = rj;
    }
}

// ---- adaptive sampling (pt_adaptive_select, pt_render_indirect_pixels, pt_sample_moments_pixels; include/pt_shim.h) ----
// the pixel a slot names, clamped into the local image: an out-of-range slot is defined behaviour, never an out-of-range access
PTK_DEV uint32_t pt_slot_pixel(uint2 slot, uint32_t npix) { return slot.x < npix ? slot.x : npix - 1u; }

// pt_fold_list_kernel: pt_fold_kernel's chain for the pixels of a list.  One lane per (slot j, channel): the radiance of frame f of
// the launch is rad[f][j], its number z = (the slot's frame + frame_off + f) & 0x7fffffff -- the number the list kernels seeded it
// with.  A slot that starts at frame 0 starts afresh, every other one resumes the pixel's mean.  The slots' frames differ, so 1/z is
// tabulated for all of [1, PT_FOLD_RCP_N).  Listed pixels are distinct (the caller's contract), so no two lanes share a word.
__global__ __launch_bounds__(256) void pt_fold_list_kernel(const PtFoldListParams P)
{
    __shared__ double tab[3][128];
    __shared__ float rcp_z[PT_FOLD_RCP_N];
    for (int k = (int)threadIdx.x; k < 384; k += 256) {
        int w = k >> 7, i = k & 127;
        tab[w][i] = w == 0 ? pt_pow_logc_tab[i] : w == 1 ? pt_pow_logl_tab[i] : pt_pow_exp2_tab[i];
    }
    for (int k = 1 + (int)threadIdx.x; k < PT_FOLD_RCP_N; k += 256) rcp_z[k] = 1.0f / (float)k;
    __syncthreads();
    const double* LC = tab[0];
    const double* LL = tab[1];
    const double* ET = tab[2];
    const unsigned tid = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned j = tid / 3u, ch = tid - 3u * j;
    if (j >= P.num_listed) return;
    const uint2 slot = P.slots[j];
    float* px = reinterpret_cast<float*>(P.fb + pt_slot_pixel(slot, P.npix_local));
    const uint32_t z0 = slot.y + P.frame_off;
    PtFoldChain s;
    s.m = 0.0f;
    s.v = 0.0f;
    s.E = 0.0;
    s.l = 0.0;
    s.reg = false;
    if ((z0 & 0x7fffffffu) != 0u) s.m = px[ch];   // a resumed pixel: its first decode is the literal pow
    const float* radp = P.rad + (size_t)tid;      // (== rad + j * 3 + ch: consecutive lanes read consecutive floats)
    const size_t stride = (size_t)P.num_listed * 3u;
    for (int f = 0; f < P.frame_count; ++f) {
        const float c = radp[(size_t)f * stride];
        pt_fold_frame(s, (int)((z0 + (uint32_t)f) & 0x7fffffffu), c, rcp_z, LC, LL, ET, nullptr);
    }
    if (P.frame_count > 0) {
        px[ch] = s.m;
        if (ch == 0u) px[3] = 1.0f;
    }
}

// pt_sample_moments_list_kernel: pt_sample_moments_kernel's rule (pt_moments_add, frames ascending, one lane per pixel) for the
// pixels of a list: slot j's samples are samples[f][j].  The record is read, never reset
__global__ __launch_bounds__(256) void pt_sample_moments_list_kernel(const float* __restrict__ samples, PtPixelMoments* __restrict__ moments,
                                                                     const uint2* __restrict__ slots, uint32_t num_listed, uint32_t npix,
                                                                     int32_t frames)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= num_listed) return;
    PtPixelMoments& m = moments[pt_slot_pixel(slots[j], npix)];
    PtMomentsAcc a = { m.sum[0], m.sum[1], m.sum[2], m.sum2[0], m.sum2[1], m.sum2[2], m.n, m.rejected };
    const size_t stride = (size_t)num_listed * 3u;
    const float* src = samples + (size_t)j * 3u;
    for (int32_t f = 0; f < frames; ++f) {
        pt_moments_add(a, src[0], src[1], src[2]);
        src += stride;
    }
    m.sum[0] = a.s0, m.sum[1] = a.s1, m.sum[2] = a.s2;
    m.sum2[0] = a.q0, m.sum2[1] = a.q1, m.sum2[2] = a.q2;
    m.n = a.n, m.rejected = a.rejected;
}

// The rule of pt_adaptive_select for one record: *taken = n + rejected (64 bits).  mean, var, b and c restate the expressions of
// pt_moments_resolve_kernel (which stays as it is): binary64, every operation rounded on its own.  The comparison is false for a NaN.
PTK_DEV bool pt_adaptive_active(const PtPixelMoments& m, const PtAdaptiveRule& R, uint64_t* taken)
{
    const uint32_t n = m.n;
    *taken = (uint64_t)n + (uint64_t)m.rejected;
    if (*taken >= (uint64_t)R.max_samples) return false;
    if (n < R.min_samples) return true;
    if (n < 2u) return false;
    const double nd = (double)n;
    double mean[3], var[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        mean[ch] = m.sum[ch] / nd;
        const double t = m.sum[ch] * mean[ch];
        const double d = m.sum2[ch] - t;
        const double v = d / (double)(n - 1u);
        var[ch] = v > 0.0 ? v : 0.0;
    }
    const double b = ((var[0] / nd) + (var[1] / nd)) + (var[2] / nd);
    const double c = ((mean[0] * mean[0]) + (mean[1] * mean[1])) + (mean[2] * mean[2]);
    return b > R.tol2 * (c + R.floor2);
}

// An ordered compaction on the light table's tiling (a thread owns PT_LIGHT_SCAN_ITEMS consecutive pixels, a workgroup one tile of
// PT_LIGHT_SCAN_TILE): pt_adaptive_count_kernel counts each tile's active pixels, pt_adaptive_tiles_kernel turns the counts into the
// tiles' offsets and writes the header, pt_adaptive_scatter_kernel evaluates the rule again (the same bits) and stores the slots at
// offset + the prefix within the tile.  Integer throughout: the list does not depend on the order of the scan.
__global__ __launch_bounds__(PT_LIGHT_SCAN_BLOCK) void pt_adaptive_count_kernel(const PtPixelMoments* __restrict__ moments, uint32_t npix,
                                                                                const PtAdaptiveRule R, uint64_t* __restrict__ tile_sums)
{
    __shared__ uint64_t lds[PT_LIGHT_SCAN_BLOCK];
    const uint64_t first = (uint64_t)blockIdx.x * PT_LIGHT_SCAN_TILE + threadIdx.x * PT_LIGHT_SCAN_ITEMS;
    uint64_t sum = 0ull;
    for (unsigned k = 0; k < PT_LIGHT_SCAN_ITEMS; ++k) {
        uint64_t taken;
        if (first + k < (uint64_t)npix && pt_adaptive_active(moments[first + k], R, &taken)) ++sum;
    }
    uint64_t total;
    pt_light_block_scan(sum, lds, &total);
    if (threadIdx.x == 0u) tile_sums[blockIdx.x] = total;
}

// one workgroup: tile_sums[0 .. ntiles) become exclusive prefix sums; the header takes the count
__global__ __launch_bounds__(PT_LIGHT_SCAN_BLOCK) void pt_adaptive_tiles_kernel(uint64_t* __restrict__ tile_sums, unsigned ntiles, uint32_t* __restrict__ header)
{
    __shared__ uint64_t lds[PT_LIGHT_SCAN_BLOCK];
    const unsigned per = (ntiles + PT_LIGHT_SCAN_BLOCK - 1u) / PT_LIGHT_SCAN_BLOCK;
    const unsigned first = threadIdx.x * per < ntiles ? threadIdx.x * per : ntiles, end = ntiles - first < per ? ntiles : first + per;
    uint64_t sum = 0ull;
    for (unsigned i = first; i < end; ++i) sum += tile_sums[i];
    uint64_t total;
    uint64_t run = pt_light_block_scan(sum, lds, &total);
    for (unsigned i = first; i < end; ++i) {
        const uint64_t v = tile_sums[i];
        tile_sums[i] = run;
        run += v;
    }
    if (threadIdx.x < 4u) header[threadIdx.x] = threadIdx.x == 0u ? (uint32_t)total : 0u;   // (total <= npix < 2^32)
}

__global__ __launch_bounds__(PT_LIGHT_SCAN_BLOCK) void pt_adaptive_scatter_kernel(const PtPixelMoments* __restrict__ moments, uint32_t npix,
                                                                                  const PtAdaptiveRule R, const uint64_t* __restrict__ tile_sums,
                                                                                  uint2* __restrict__ slots)
{
    __shared__ uint64_t lds[PT_LIGHT_SCAN_BLOCK];
    const uint64_t first = (uint64_t)blockIdx.x * PT_LIGHT_SCAN_TILE + threadIdx.x * PT_LIGHT_SCAN_ITEMS;
    uint32_t frame[PT_LIGHT_SCAN_ITEMS];
    unsigned active = 0u;   // bit k: pixel first + k is listed
    for (unsigned k = 0; k < PT_LIGHT_SCAN_ITEMS; ++k) {
        uint64_t taken = 0ull;
        if (first + k < (uint64_t)npix && pt_adaptive_active(moments[first + k], R, &taken)) active |= 1u << k;
        frame[k] = (uint32_t)taken;
    }
    uint64_t total;
    uint64_t at = tile_sums[blockIdx.x] + pt_light_block_scan((uint64_t)__popc(active), lds, &total);   // (at most the pixel's own index)
    for (unsigned k = 0; k < PT_LIGHT_SCAN_ITEMS; ++k)
        if (active & (1u << k)) slots[at++] = make_uint2((uint32_t)(first + k), frame[k]);
}

// ------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------
hipError_t ptk_fold_list(const PtFoldListParams& p, hipStream_t s)
{
    if (p.num_listed == 0 || p.frame_count <= 0) return hipSuccess;
    hipLaunchKernelGGL(pt_fold_list_kernel, dim3((unsigned)(((size_t)p.num_listed * 3 + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t ptk_sample_moments_list(const float* samples, PtPixelMoments* moments, const uint2* slots, uint32_t num_listed, uint32_t npix,
                                   int32_t frames, hipStream_t s)
{
    if (num_listed == 0 || npix == 0 || frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(pt_sample_moments_list_kernel, dim3((unsigned)(((uint64_t)num_listed + 255u) / 256u)), dim3(256), 0, s, samples, moments, slots,
                       num_listed, npix, frames);
    return hipGetLastError();
}

hipError_t ptk_adaptive_select(const PtPixelMoments* moments, uint32_t npix, const PtAdaptiveRule& rule, void* list, hipStream_t s)
{
    if (npix == 0) return hipMemsetAsync(list, 0, 16, s);
    const unsigned ntiles = (unsigned)PT_LIGHT_TABLE_TILES(npix);
    uint2* slots = reinterpret_cast<uint2*>(static_cast<char*>(list) + 16);
    uint64_t* tile_sums = reinterpret_cast<uint64_t*>(slots + npix);   // the build's scratch, behind the specified part
    hipLaunchKernelGGL(pt_adaptive_count_kernel, dim3(ntiles), dim3(PT_LIGHT_SCAN_BLOCK), 0, s, moments, npix, rule, tile_sums);
    hipLaunchKernelGGL(pt_adaptive_tiles_kernel, dim3(1), dim3(PT_LIGHT_SCAN_BLOCK), 0, s, tile_sums, ntiles, static_cast<uint32_t*>(list));
    hipLaunchKernelGGL(pt_adaptive_scatter_kernel, dim3(ntiles), dim3(PT_LIGHT_SCAN_BLOCK), 0, s, moments, npix, rule, tile_sums, slots);
    return hipGetLastError();
}

hipError_t ptk_prep_triangles(const PtRawTriangle* raw, PtPrepTriangle* out, int ntri, unsigned int* det_bound_bits,
                              hipStream_t s)
{
    hipError_t e = hipMemsetAsync(det_bound_bits, 0, PT_PREP_WORDS * sizeof(unsigned int), s);
    if (e != hipSuccess || ntri <= 0) return e;
    hipLaunchKernelGGL(pt_prep_kernel, dim3((ntri + 255) / 256), dim3(256), 0, s, raw, out, ntri, det_bound_bits);
    return hipGetLastError();
}

hipError_t ptk_prep_quad_margins(PtPrepTriangle* out, int ntri, float diameter, float delta1, float* p1tab, const float anchor[3], hipStream_t s)
{
    if (ntri < 2) return hipSuccess;
    const int pairs = ntri / 2;
    hipLaunchKernelGGL(pt_prep_quad_margins_kernel, dim3((pairs + 255) / 256), dim3(256), 0, s, out, ntri, diameter, delta1);
    if (p1tab) {
        const int qpairs = (pairs + 1) / 2;
        hipLaunchKernelGGL(pt_prep_p1tab_kernel, dim3((qpairs + 255) / 256), dim3(256), 0, s, out, ntri, diameter, p1tab, anchor[0], anchor[1], anchor[2]);
    }
    return hipGetLastError();
}

hipError_t ptk_primary_masks(const PtTraceParams& p, hipStream_t s)
{
    if (!p.pmask || p.npix_local == 0) return hipSuccess;
    PtMaskParams m;
    m.tris = p.tris;
    m.out = const_cast<uint2*>(p.pmask);
    m.width = p.width; m.height = p.height; m.ntri = p.ntri;
    m.stripe_rows = p.stripe_rows; m.n_ranks = p.n_ranks; m.rank = p.rank;
    m.npix_local = p.npix_local;
    m.cam = p.cam;
    hipLaunchKernelGGL(pt_primary_mask_kernel, dim3((p.npix_local + 255u) / 256u), dim3(256), 0, s, m);
    return hipGetLastError();
}

hipError_t ptk_secondary_masks(const PtPrepTriangle* tris, int ntri, uint2* table, hipStream_t s)
{
    if (!table || ntri <= 0 || ntri > PT_SM_TRI_MAX) return hipErrorInvalidValue;
    const unsigned n = (unsigned)ntri * PT_SM_TRI_ENTRIES;
    hipLaunchKernelGGL(pt_secondary_mask_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, tris, ntri, table);
    return hipGetLastError();
}

hipError_t ptk_trace(const PtTraceParams& p, int num_blocks, PtSearchMode m, bool tally, bool wide, hipStream_t s)
{
    // (the order the instantiations appear in is the order of the kernels in the code object)
    const bool q3 = m.quads == 3;
    void (*kernel)(const PtTraceParams);
    if (m.bvh && wide)
        kernel = tally ? (m.det_bounded ? (q3 ? pt_trace_bvh_kernel<true, true, 3, true> : pt_trace_bvh_kernel<true, true, 0, true>) : pt_trace_bvh_kernel<false, true, 0, true>)
                       : (m.det_bounded ? (q3 ? pt_trace_bvh_kernel<true, false, 3, true> : pt_trace_bvh_kernel<true, false, 0, true>) : pt_trace_bvh_kernel<false, false, 0, true>);
    else if (m.bvh)
        kernel = tally ? (m.det_bounded ? (q3 ? pt_trace_bvh_kernel<true, true, 3> : pt_trace_bvh_kernel<true, true, 0>) : pt_trace_bvh_kernel<false, true, 0>)
                       : (m.det_bounded ? (q3 ? pt_trace_bvh_kernel<true, false, 3> : pt_trace_bvh_kernel<true, false, 0>) : pt_trace_bvh_kernel<false, false, 0>);
    else if (p.ntri <= PT_LDS_TRI_MAX)
        kernel = m.det_bounded ? (q3 ? pt_trace_kernel<true, 1, 3> : pt_trace_kernel<true, 1, 0>) : pt_trace_kernel<false, 1, 0>;
    else
        kernel = m.det_bounded ? pt_trace_tiled_kernel<true> : pt_trace_tiled_kernel<false>;
    const size_t lds = m.bvh ? ptk_trace_bvh_lds_bytes() : ptk_trace_lds_bytes(p.ntri);
    hipLaunchKernelGGL(kernel, dim3(num_blocks), dim3(PT_TRACE_THREADS), lds, s, p);
    return hipGetLastError();
}

hipError_t ptk_fold(const PtFoldParams& p, hipStream_t s)
{
    if (p.npix_local == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_fold_kernel, dim3((unsigned)(((size_t)p.npix_local * 3 + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t ptk_assemble_stripes(const float4* gathered, float4* image, int width, int height, int stripe_rows,
                                int n_ranks, int slab_rows, hipStream_t s)
{
    size_t total = (size_t)width * height;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_assemble_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, gathered, image,
                       width, height, stripe_rows, n_ranks, slab_rows);
    return hipGetLastError();
}

hipError_t ptk_tonemap_ppm(const float4* fb, int32_t* rgb, size_t npix, hipStream_t s)
{
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_tonemap_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, fb, rgb, npix);
    return hipGetLastError();
}

hipError_t ptk_fold_check(unsigned long long* out, int mode, unsigned first, unsigned long long count, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    const unsigned long long want = (count + 255) / 256;
    hipLaunchKernelGGL(pt_fold_check_kernel, dim3((unsigned)(want < 65536ull ? want : 65536ull)), dim3(256), 0, s, out, mode, first, count);
    return hipGetLastError();
}

hipError_t ptk_shade_check(unsigned long long* out, int mode, unsigned first, unsigned long long count, hipStream_t s)
{
    if (count == 0) return hipSuccess;
    const unsigned long long want = (count + 255) / 256;
    hipLaunchKernelGGL(pt_shade_check_kernel, dim3((unsigned)(want < 65536ull ? want : 65536ull)), dim3(256), 0, s, out, mode, first, count);
    return hipGetLastError();
}

hipError_t ptk_pair_check(const uint2* masks, unsigned* out, int ntri, unsigned cases, unsigned cap, hipStream_t s)
{
    if (cases == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_pair_check_kernel, dim3(cases), dim3(64), 0, s, masks, out, ntri, cap);
    return hipGetLastError();
}

hipError_t ptk_search_check(const PtPrepTriangle* tris, int ntri, const float4* rays, const uint2* masks, uint4* out, unsigned cases, hipStream_t s)
{
    if (cases == 0) return hipSuccess;
    const unsigned wg_waves = PT_TRACE_THREADS / 64;
    const size_t lds = (size_t)pt_lds_total<1, false>(ntri) * sizeof(float);
    hipLaunchKernelGGL(pt_search_check_kernel, dim3((cases + wg_waves - 1) / wg_waves), dim3(PT_TRACE_THREADS), lds, s, tris, ntri, rays, masks, out, cases);
    return hipGetLastError();
}

hipError_t ptk_math(const float* in, float* out, int n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pt_math_kernel, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n);
    return hipGetLastError();
}

hipError_t ptk_fill_i32(int32_t* dst, int32_t value, int n, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pt_fill_i32_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dst, value, n);
    return hipGetLastError();
}

size_t ptk_trace_lds_bytes(int ntri)
{
    return (size_t)(ntri <= PT_LDS_TRI_MAX ? pt_lds_total<1>(ntri) : pt_lds_total<2>(ntri)) * sizeof(float);
}

size_t ptk_trace_bvh_lds_bytes(void)
{
    return (size_t)pt_bvh_lds_total() * sizeof(float);
}

// resident workgroups per CU of a kernel of PT_TRACE_THREADS threads with `lds` bytes of dynamic LDS
template <class Kernel> static int pt_blocks_per_cu(Kernel kernel, size_t lds)
{
    int nb = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, PT_TRACE_THREADS, lds);
    if (e != hipSuccess || nb < 1) nb = 2;
    return nb;
}

int ptk_trace_bvh_blocks_per_cu(void) { return pt_blocks_per_cu(pt_trace_bvh_kernel<true, false, 3>, ptk_trace_bvh_lds_bytes()); }
int ptk_query_bvh_blocks_per_cu(void) { return pt_blocks_per_cu(pt_query_bvh_kernel<true, 3, false>, ptk_trace_bvh_lds_bytes()); }
int ptk_trace_blocks_per_cu(int ntri)
{
    return ntri <= PT_LDS_TRI_MAX ? pt_blocks_per_cu(pt_trace_kernel<true, 1, 3>, ptk_trace_lds_bytes(ntri))
                                  : pt_blocks_per_cu(pt_trace_tiled_kernel<true>, ptk_trace_lds_bytes(ntri));
}

// ---- searches that take items: ray queries, ambient occlusion, the lit renders ------------------------------------------------
// (instantiated here, after every trace kernel)
// A kernel FAMILY names a parameter block and its two templates: bvh<DET_BOUNDED, BIGQ>() on the LBVH driver and
// table<DET_BOUNDED, LDS_TABLE, QUADS>() over the brute-force table.  THE choice of a family's instantiation for a scene, written
// once: the LBVH, the table in LDS or the tiled table; the packed filter (3) needs the bounded reciprocal, and the tiled table has
// no packed form.  Eight instantiations per family, no other
template <class F> static auto pt_choose(PtSearchMode m, int ntri) -> void (*)(const typename F::Params)
{
    const bool q3 = m.quads == 3;
    if (m.bvh) return m.det_bounded ? (q3 ? F::template bvh<true, 3>() : F::template bvh<true, 0>()) : F::template bvh<false, 0>();
    if (ntri <= PT_LDS_TRI_MAX) return m.det_bounded ? (q3 ? F::template table<true, 1, 3>() : F::template table<true, 1, 0>()) : F::template table<false, 1, 0>();
    return m.det_bounded ? F::template table<true, 2, 0>() : F::template table<false, 2, 0>();
}

template <bool ANY> struct PtQueryFamily {   // ANY: the any-hit search through the LBVH; the table search is the closest one
    using Params = PtQueryParams;
    template <bool DB, int BIGQ> static constexpr auto bvh() { return pt_query_bvh_kernel<DB, BIGQ, ANY>; }
    template <bool DB, int LDS_TABLE, int QUADS> static constexpr auto table() { return pt_query_kernel<DB, LDS_TABLE, QUADS>; }
};
struct PtAoFamily {
    using Params = PtAoParams;
    template <bool DB, int BIGQ> static constexpr auto bvh() { return pt_ao_bvh_kernel<DB, BIGQ>; }
    template <bool DB, int LDS_TABLE, int QUADS> static constexpr auto table() { return pt_ao_kernel<DB, LDS_TABLE, QUADS>; }
};
struct PtFeatureFamily {
    using Params = PtFeatureParams;
    template <bool DB, int BIGQ> static constexpr auto bvh() { return pt_feature_bvh_kernel<DB, BIGQ>; }
    template <bool DB, int LDS_TABLE, int QUADS> static constexpr auto table() { return pt_feature_kernel<DB, LDS_TABLE, QUADS>; }
};
// a kind of lit render (ptk_lit_kind); rr: the table kernels are the refilling ones, a wave of which owns PT_RR_RUN items
template <unsigned KIND> struct PtLitFamily {
    using K = PtKindOf<KIND>;
    using Params = PtKindArgs<KIND>;
    static constexpr unsigned run = K::rr ? PT_RR_RUN : 64;
    template <bool DB, int BIGQ> static constexpr auto bvh()
    {
        if constexpr (K::indirect) return pt_indirect_bvh_kernel<DB, BIGQ, KIND>;
        else return pt_direct_bvh_kernel<DB, BIGQ, KIND>;
    }
    template <bool DB, int LDS_TABLE, int QUADS> static constexpr auto table()
    {
        if constexpr (K::rr) return pt_indirect_rr_kernel<DB, LDS_TABLE, QUADS, KIND>;
        else if constexpr (K::indirect) return pt_indirect_kernel<DB, LDS_TABLE, QUADS, KIND>;
        else return pt_direct_kernel<DB, LDS_TABLE, QUADS, KIND>;
    }
    // the instantiations' own block, sliced from the largest (every indirect block is a base of it; direct by power: direct's and the table)
    static Params params(const PtLitParams& a)
    {
        if constexpr (K::indirect && !K::env && !K::rays) return a;
        else if constexpr (!K::indirect && !K::power) return a.d;
        else {
            Params p;
            __builtin_memset(&p, 0, sizeof p);
            if constexpr (K::indirect) static_cast<PtIndirectRrParams&>(p) = a;
            else { static_cast<PtDirectParams&>(p) = a.d; p.cdf = a.cdf; p.tri_q = a.tri_q; }
            if constexpr (K::ris) p.M = a.M;
            if constexpr (K::env) p.env = a.env;
            if constexpr (K::rays) { p.rays = a.rays; p.first_ray = a.first_ray; }
            return p;
        }
    }
};
// fn(the family of `kind`), instantiated for every value ptk_lit_valid accepts and for no other: the predicates of pt_kernels.h ARE
// the list of kinds.  `none` is the answer for a value they refuse
template <class R, class Fn, unsigned... I> static R pt_lit_family(unsigned kind, R none, Fn fn, std::integer_sequence<unsigned, I...>)
{
    auto one = [&](auto i) {
        if constexpr (ptk_lit_valid(decltype(i)::value))
            if (kind == decltype(i)::value) none = fn(PtLitFamily<decltype(i)::value>());
    };
    (one(std::integral_constant<unsigned, I>()), ...);
    return none;
}
template <class R, class Fn> static R pt_lit_family(unsigned kind, R none, Fn fn) { return pt_lit_family(kind, none, fn, std::make_integer_sequence<unsigned, PT_LIT_KINDS>()); }

// One launch of a kernel over nitems items of a scene of ntri triangles -- LBVH: a persistent grid of at most bvh_blocks workgroups (what the chip
// holds), its waves take 64 items at a time, with the trace kernel's LDS; brute force: one wave per `run` items, the table kernels' LDS without the pools
template <class Params>
static hipError_t pt_launch_search(void (*kernel)(const Params), const Params& p, int ntri, unsigned nitems, unsigned run, bool bvh, int bvh_blocks, hipStream_t s)
{
    const unsigned wg_waves = PT_TRACE_THREADS / 64, per_wave = bvh ? 64u : run;
    unsigned blocks = ((nitems + per_wave - 1u) / per_wave + wg_waves - 1u) / wg_waves;
    if (bvh && bvh_blocks > 0 && blocks > (unsigned)bvh_blocks) blocks = (unsigned)bvh_blocks;
    const size_t lds = bvh ? ptk_trace_bvh_lds_bytes()
                           : (size_t)(ntri <= PT_LDS_TRI_MAX ? pt_lds_total<1, false>(ntri) : pt_lds_total<2, false>(ntri)) * sizeof(float);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(PT_TRACE_THREADS), lds, s, p);
    return hipGetLastError();
}

hipError_t ptk_query(const PtQueryParams& q, int bvh_blocks, PtSearchMode m, bool any, hipStream_t s)
{
    if (q.nrays == 0) return hipSuccess;
    const auto kernel = any ? pt_choose<PtQueryFamily<true>>(m, q.t.ntri) : pt_choose<PtQueryFamily<false>>(m, q.t.ntri);
    return pt_launch_search(kernel, q, q.t.ntri, q.nrays, 64u, m.bvh, bvh_blocks, s);
}

hipError_t ptk_ao(const PtAoParams& a, int bvh_blocks, PtSearchMode m, hipStream_t s)
{
    if (a.nitems == 0) return hipSuccess;
    return pt_launch_search(pt_choose<PtAoFamily>(m, a.t.ntri), a, a.t.ntri, a.nitems, 64u, m.bvh, bvh_blocks, s);
}

hipError_t ptk_render_features(const PtFeatureParams& f, int bvh_blocks, PtSearchMode m, hipStream_t s)
{
    if (f.d.nitems == 0) return hipSuccess;
    return pt_launch_search(pt_choose<PtFeatureFamily>(m, f.d.t.ntri), f, f.d.t.ntri, f.d.nitems, 64u, m.bvh, bvh_blocks, s);
}

hipError_t ptk_lit(const PtLitParams& a, unsigned kind, int bvh_blocks, PtSearchMode m, hipStream_t s)
{
    if (a.d.nitems == 0) return hipSuccess;
    return pt_lit_family(kind, hipErrorInvalidValue, [&](auto f) {
        using F = decltype(f);
        const typename F::Params p = F::params(a);
        return pt_launch_search(pt_choose<F>(m, a.d.t.ntri), p, a.d.t.ntri, a.d.nitems, F::run, m.bvh, bvh_blocks, s);
    });
}

int ptk_lit_bvh_blocks_per_cu(unsigned kind)
{
    return pt_lit_family(kind, 0, [](auto f) { return pt_blocks_per_cu(decltype(f)::template bvh<true, 3>(), ptk_trace_bvh_lds_bytes()); });
}

hipError_t ptk_light_table(const PtRawTriangle* tris, int ntri, const PtRawMaterial* mats, int nmat, const int32_t* lights, int nl,
                           uint64_t* cdf, uint32_t* tri_q, hipStream_t s)
{
    hipError_t e = hipSuccess;
    if (ntri > 0 && (e = hipMemsetAsync(tri_q, 0, (size_t)ntri * sizeof(uint32_t), s)) != hipSuccess) return e;
    if (nl == 0 || ntri == 0) return hipMemsetAsync(cdf, 0, ((size_t)nl + 1) * sizeof(uint64_t), s);   // (no triangle to name: every q is 0)
    const unsigned ntiles = (unsigned)PT_LIGHT_TABLE_TILES(nl);
    uint64_t* pmax = cdf + (size_t)nl + 1;   // the build's scratch, behind the specified part: the maximum's bits, then the tile sums
    uint64_t* tile_sums = pmax + 1;
    if ((e = hipMemsetAsync(pmax, 0, sizeof(uint64_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(pt_light_weight_kernel, dim3(((unsigned)nl + PT_LIGHT_SCAN_BLOCK - 1u) / PT_LIGHT_SCAN_BLOCK), dim3(PT_LIGHT_SCAN_BLOCK), 0, s,
                       tris, ntri, mats, nmat, lights, nl, reinterpret_cast<uint32_t*>(pmax));
    hipLaunchKernelGGL(pt_light_quantise_kernel, dim3(ntiles), dim3(PT_LIGHT_SCAN_BLOCK), 0, s, tris, ntri, mats, nmat, lights, nl,
                       reinterpret_cast<const uint32_t*>(pmax), cdf, tri_q, tile_sums);
    hipLaunchKernelGGL(pt_light_tiles_kernel, dim3(1), dim3(PT_LIGHT_SCAN_BLOCK), 0, s, tile_sums, ntiles, cdf);
    hipLaunchKernelGGL(pt_light_scan_kernel, dim3(ntiles), dim3(PT_LIGHT_SCAN_BLOCK), 0, s, cdf, nl, tile_sums);
    return hipGetLastError();
}

hipError_t ptk_env_table(const float4* texels, int N, uint64_t* cdf, hipStream_t s)
{
    const int nl = N * N;   // 1 .. 2^22
    const unsigned ntiles = (unsigned)PT_LIGHT_TABLE_TILES(nl);
    uint64_t* pmax = cdf + (size_t)nl + 1;   // pt_light_table's scratch: the maximum's bits, then the tile sums
    uint64_t* tile_sums = pmax + 1;
    hipError_t e = hipMemsetAsync(pmax, 0, sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pt_env_weight_kernel, dim3(((unsigned)nl + PT_LIGHT_SCAN_BLOCK - 1u) / PT_LIGHT_SCAN_BLOCK), dim3(PT_LIGHT_SCAN_BLOCK), 0, s,
                       texels, N, reinterpret_cast<uint32_t*>(pmax));
    hipLaunchKernelGGL(pt_env_quantise_kernel, dim3(ntiles), dim3(PT_LIGHT_SCAN_BLOCK), 0, s, texels, N, reinterpret_cast<const uint32_t*>(pmax), cdf,
                       tile_sums);
    hipLaunchKernelGGL(pt_light_tiles_kernel, dim3(1), dim3(PT_LIGHT_SCAN_BLOCK), 0, s, tile_sums, ntiles, cdf);
    hipLaunchKernelGGL(pt_light_scan_kernel, dim3(ntiles), dim3(PT_LIGHT_SCAN_BLOCK), 0, s, cdf, nl, tile_sums);
    return hipGetLastError();
}

hipError_t ptk_light_counts(const int32_t* lights, int nl, int ntri, int32_t* counts, hipStream_t s)
{
    if (ntri <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)ntri * sizeof(int32_t), s);
    if (e != hipSuccess || nl <= 0) return e;
    hipLaunchKernelGGL(pt_light_counts_kernel, dim3(((unsigned)nl + 255u) / 256u), dim3(256), 0, s, lights, nl, ntri, counts);
    return hipGetLastError();
}

hipError_t ptk_sample_moments(const float* samples, PtPixelMoments* moments, uint32_t npix, int32_t frames, bool reset, hipStream_t s)
{
    if (npix == 0u || frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(pt_sample_moments_kernel, dim3((unsigned)(((uint64_t)npix + 255u) / 256u)), dim3(256), 0, s, samples, moments, npix, frames, reset ? 1 : 0);
    return hipGetLastError();
}

hipError_t ptk_moments_resolve(const PtPixelMoments* moments, uint32_t npix, void* noise, PtNoiseSummary* summary, hipStream_t s)
{
    if (npix == 0u || (!noise && !summary)) return hipSuccess;
    // level 0 over the pixels; while more than one tile sum is left, the same kernel over the sums (summary[1 ..]: the scratch)
    uint32_t tiles = (uint32_t)PT_MOMENTS_TILES(npix);
    PtNoiseSummary* scratch = summary ? summary + 1 : nullptr;
    PtNoiseSummary* out = !summary ? nullptr : tiles == 1u ? summary : scratch;
    hipLaunchKernelGGL(pt_moments_resolve_kernel, dim3(tiles), dim3(256), 0, s, moments, (const PtNoiseSummary*)nullptr, npix, (uint4*)noise, out);
    hipError_t e = hipGetLastError();
    while (e == hipSuccess && summary && tiles > 1u) {
        const PtNoiseSummary* in = out;
        const uint32_t count = tiles;
        tiles = (uint32_t)PT_MOMENTS_TILES(count);
        scratch += count;
        out = tiles == 1u ? summary : scratch;
        hipLaunchKernelGGL(pt_moments_resolve_kernel, dim3(tiles), dim3(256), 0, s, (const PtPixelMoments*)nullptr, in, count, (uint4*)nullptr, out);
        e = hipGetLastError();
    }
    return e;
}

hipError_t ptk_ao_resolve(const uint2* counts, float4* image, uint32_t npix, uint32_t K, float miss_value, hipStream_t s)
{
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_ao_resolve_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, s, counts, image, npix, K, miss_value);
    return hipGetLastError();
}

hipError_t ptk_camera_rays(const PtLensCamera& cam, int width, int height, int frame, float4* rays, hipStream_t s)
{
    const unsigned npix = (unsigned)width * (unsigned)height;
    if (npix == 0) return hipSuccess;
    // the renderer's per-image constants (pt_shim.hip: image_geometry)
    const float inv_w = 1.0f / (float)width, inv_h = 1.0f / (float)height, aspect = (float)width / (float)height;
    hipLaunchKernelGGL(pt_camera_rays_kernel, dim3((npix + 255u) / 256u), dim3(256), 0, s, cam, width, npix, inv_w, inv_h, aspect, frame, rays);
    return hipGetLastError();
}
