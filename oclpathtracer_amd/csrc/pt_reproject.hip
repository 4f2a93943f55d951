// pt_reproject.hip -- temporal reprojection of the moments (pt_reproject).  include/pt_shim.h states every expression and their order;
// this file follows it operation by operation (the build contracts nothing: -ffp-contract=off, no fast-math; "/" and sqrt are hipcc's
// correctly rounded ones).  One lane per pixel of the NEW view, workgroups of 32 x 8 pixels: neighbouring lanes re-project to
// neighbouring pixels of the previous view, so a wave's four taps fall into a few rows of it.  Two forms with the same per-pixel
// arithmetic, hence the same bits:
//   PREPARED = false  one kernel; every lane reads what it needs of its taps' 56-byte records (n of the colour, two doubles of the
//                     depth, three doubles and n of the normal), then the colour record where the tap survives;
//   PREPARED = true   pt_reproject_prepare_kernel first turns the previous view's records into one float4 (nq, z_q) per pixel of
//                     the scratch -- z_q a NaN where step 5 skips the tap for what the tap itself holds (no samples, no coverage,
//                     the noise test), which the depth test then does: a NaN fails it --, read coalesced and once; the taps read those 16 bytes, and the colour record where a tap
//                     survives.
// No atomics, no flags, no LDS, nothing the host waits for.
#include "pt_reproject.h"

#define PTR_TW 32
#define PTR_TH 8
#define PTR_THREADS (PTR_TW * PTR_TH)

namespace {

struct PtrRecord {   // pt_pixel_moments
    double sum[3];
    double sum2[3];
    uint32_t n, rejected;
};
static_assert(sizeof(PtrRecord) == 56, "moment record layout");

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(const float* a) { return { a[0], a[1], a[2] }; }
__device__ __forceinline__ float ptr_dot(V3 a, V3 b) { return ((a.x * b.x) + (a.y * b.y)) + (a.z * b.z); }

// mean(R): (float)(sum[k] / (double)n), 0 for n = 0
__device__ __forceinline__ V3 ptr_mean(const PtrRecord& m)
{
    const uint32_t n = m.n;
    const double nd = (double)n;
    return { (float)(n ? m.sum[0] / nd : 0.0), (float)(n ? m.sum[1] / nd : 0.0), (float)(n ? m.sum[2] / nd : 0.0) };
}

// the noise test of step 5: true when the tap counts (max_noise > 0 is the caller's to check)
__device__ __forceinline__ bool ptr_quiet(const PtrRecord& C, float max_noise)
{
    const uint32_t n = C.n;
    const double nd = (double)n;
    double b = 0.0, m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        m[k] = C.sum[k] / nd;
        if (n >= 2u) {
            const double t = C.sum[k] * m[k];
            const double d = C.sum2[k] - t;
            double v = d / (double)(n - 1u);
            v = v > 0.0 ? v : 0.0;
            const double q = v / nd;
            b = k == 0 ? q : b + q;
        }
    }
    return b <= (double)max_noise * (((m[0] * m[0]) + (m[1] * m[1])) + (m[2] * m[2]));
}

// the pixel of this lane: tiles of 32 x 8 numbered along x, a one-dimensional grid (an image may be 1 x 2^31 - 1 or 2^31 - 1 x 1)
__device__ __forceinline__ bool ptr_pixel(int width, int height, int& x, int& y)
{
    const uint32_t tiles_x = ((uint32_t)width + PTR_TW - 1u) / PTR_TW;
    x = (int)((blockIdx.x % tiles_x) * PTR_TW + threadIdx.x % PTR_TW);
    y = (int)((blockIdx.x / tiles_x) * PTR_TH + threadIdx.x / PTR_TW);
    return x < width && y < height;
}

__global__ __launch_bounds__(PTR_THREADS) void pt_reproject_prepare_kernel(const PtrRecord* __restrict__ colour, const PtrRecord* __restrict__ normal,
                                                                           const PtrRecord* __restrict__ depth, float4* __restrict__ plane,
                                                                           int width, int height, float max_noise)
{
    int x, y;
    if (!ptr_pixel(width, height, x, y)) return;
    const size_t q = (size_t)y * (size_t)width + (size_t)x;
    V3 nq = { 0.0f, 0.0f, 0.0f };
    if (normal) nq = ptr_mean(normal[q]);
    const double t = depth[q].sum[0], c = depth[q].sum[1];
    bool counts = colour[q].n != 0u && c > 0.0;
    if (counts && max_noise > 0.0f) counts = ptr_quiet(colour[q], max_noise);   // (the whole record, read once per pixel, not per tap)
    const float zq = counts ? (float)(t / c) : __builtin_nanf("");
    plane[q] = make_float4(nq.x, nq.y, nq.z, zq);
}

template <bool PREPARED>
__global__ __launch_bounds__(PTR_THREADS) void pt_reproject_kernel(const PtrRecord* __restrict__ prev_colour, const PtrRecord* __restrict__ prev_normal,
                                                                   const PtrRecord* __restrict__ prev_depth, const float4* __restrict__ plane,
                                                                   const PtrRecord* __restrict__ cur_normal, const PtrRecord* __restrict__ cur_depth,
                                                                   PtrRecord* __restrict__ out_colour, float4* __restrict__ out_info,
                                                                   const PtReprojectArgs A)
{
    const int width = A.width, height = A.height;
    int x, y;
    if (!ptr_pixel(width, height, x, y)) return;
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    const bool normals = cur_normal != nullptr;

    double Wd = 0.0, Nn = 0.0, M[3] = { 0.0, 0.0, 0.0 }, S[3] = { 0.0, 0.0, 0.0 };
    float fx = 0.0f, fy = 0.0f;
    bool taps = false;   // step 6 is reached

    const double dsum = cur_depth[p].sum[1];
    if (dsum > 0.0) {                                                               // step 1
        const float z = (float)(cur_depth[p].sum[0] / dsum);
        const float cz = (float)(cur_depth[p].sum[2] / dsum);
        // step 2
        const float xs = (2.0f * (((float)x + 0.5f) * A.inv_width) - 1.0f) * A.cur.angle * A.aspect;
        const float ys = -(1.0f - 2.0f * (((float)y + 0.5f) * A.inv_height)) * A.cur.angle;
        const float my = -1.0f * ys;
        const V3 hol = v3(A.cur.hol), up = v3(A.cur.up), view = v3(A.cur.view), eye = v3(A.cur.eye);
        const V3 w = { (hol.x * xs + up.x * my) + view.x, (hol.y * xs + up.y * my) + view.y, (hol.z * xs + up.z * my) + view.z };
        const float inv = 1.0f / __builtin_sqrtf(ptr_dot(w, w));
        const V3 dir = { w.x * inv, w.y * inv, w.z * inv };
        const V3 P = { eye.x + dir.x * z, eye.y + dir.y * z, eye.z + dir.z * z };
        // step 3
        const V3 v = { P.x - A.prev.eye[0], P.y - A.prev.eye[1], P.z - A.prev.eye[2] };
        const float dz = ptr_dot(v, v3(A.prev.view));
        if (dz > 0.0f) {
            const float a = ptr_dot(v, v3(A.prev.hol)) / dz;
            const float b = ptr_dot(v, v3(A.prev.up)) / dz;
            fx = ((a / (A.prev.angle * A.aspect) + 1.0f) * 0.5f) * (float)width - 0.5f;
            fy = ((1.0f - b / A.prev.angle) * 0.5f) * (float)height - 0.5f;
            const float r = __builtin_sqrtf(ptr_dot(v, v));
            if (fx > -1.0f && fx < (float)width && fy > -1.0f && fy < (float)height) {   // step 4
                taps = true;
                const int x0 = (int)__builtin_floorf(fx), y0 = (int)__builtin_floorf(fy);
                const float tx = fx - (float)x0, ty = fy - (float)y0;
                const float c = cz > 0.125f ? cz : 0.125f;
                const float tol_r = A.tol_z * r;
                V3 nc = { 0.0f, 0.0f, 0.0f };
                float nc2 = 0.0f;
                if (normals) {
                    nc = ptr_mean(cur_normal[p]);
                    nc2 = ptr_dot(nc, nc);
                }
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {                                    // step 5
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int qx = x0 + dx, qy = y0 + dy;   // (x0 <= width - 1: no overflow)
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
                        const float bw = (dx ? tx : 1.0f - tx) * (dy ? ty : 1.0f - ty);
                        float zq;
                        V3 nq = { 0.0f, 0.0f, 0.0f };
                        if (PREPARED) {
                            const float4 g = plane[q];
                            zq = g.w;
                            nq = { g.x, g.y, g.z };
                        } else {
                            if (prev_colour[q].n == 0u) continue;
                            const double cq = prev_depth[q].sum[1];
                            if (!(cq > 0.0)) continue;
                            zq = (float)(prev_depth[q].sum[0] / cq);
                        }
                        if (!(__builtin_fabsf(zq - r) * c <= tol_r)) continue;
                        if (normals) {
                            if (!PREPARED) nq = ptr_mean(prev_normal[q]);
                            const float Dn = ptr_dot(nc, nq);
                            if (!(Dn > 0.0f && Dn * Dn >= A.cos_min2 * (nc2 * ptr_dot(nq, nq)))) continue;
                        }
                        const PtrRecord& C = prev_colour[q];
                        if (!PREPARED && A.max_noise > 0.0f && !ptr_quiet(C, A.max_noise)) continue;
                        const double nqd = (double)C.n, bd = (double)bw;
                        Wd = Wd + bd;
                        Nn = Nn + bd * nqd;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            M[k] = M[k] + bd * (C.sum[k] / nqd);
                            S[k] = S[k] + bd * (C.sum2[k] / nqd);
                        }
                    }
                }
            }
        }
    }

    PtrRecord out;
    out.sum[0] = out.sum[1] = out.sum[2] = out.sum2[0] = out.sum2[1] = out.sum2[2] = 0.0;
    out.n = out.rejected = 0u;
    float4 info = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (taps) {                                                                     // steps 6 and 7
        info = make_float4(fx, fy, (float)Wd, 0.0f);
        if (Wd >= (double)A.min_weight && Wd > 0.0) {
            double N = Nn / Wd;
            N = N < (double)A.max_history ? N : (double)A.max_history;
            const uint32_t nh = (uint32_t)__builtin_floor(N);
            if (nh != 0u) {
                const double nhd = (double)nh;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    out.sum[k] = (M[k] / Wd) * nhd;
                    out.sum2[k] = (S[k] / Wd) * nhd;
                }
                out.n = nh;
                info.w = (float)nh;
            }
        }
    }
    out_colour[p] = out;
    if (out_info) out_info[p] = info;
}

}   // namespace

hipError_t ptk_reproject(const void* prev_colour, const void* prev_normal, const void* prev_depth, const void* cur_normal, const void* cur_depth,
                         float4* scratch, void* out_colour, float4* out_info, const PtReprojectArgs& a, int form, hipStream_t s)
{
    const uint32_t tiles = (((uint32_t)a.width + PTR_TW - 1u) / PTR_TW) * (((uint32_t)a.height + PTR_TH - 1u) / PTR_TH);
    const PtrRecord *pc = (const PtrRecord*)prev_colour, *pn = (const PtrRecord*)prev_normal, *pd = (const PtrRecord*)prev_depth;
    const PtrRecord *cn = (const PtrRecord*)cur_normal, *cd = (const PtrRecord*)cur_depth;
    // PT_REPROJECT_FORM_AUTO is the faster form as measured on the MI355X (profiles/reproject/rates.txt): at 1024^2 the prepare pass
    // and the kernel over its plane take 0.126 ms together, the one kernel over the records 0.230 ms -- so auto is the prepared form
    if (form == PT_REPROJECT_FORM_DIRECT) {
        hipLaunchKernelGGL(pt_reproject_kernel<false>, dim3(tiles), dim3(PTR_THREADS), 0, s, pc, pn, pd, (const float4*)nullptr, cn, cd,
                           (PtrRecord*)out_colour, out_info, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(pt_reproject_prepare_kernel, dim3(tiles), dim3(PTR_THREADS), 0, s, pc, pn, pd, scratch, a.width, a.height, a.max_noise);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pt_reproject_kernel<true>, dim3(tiles), dim3(PTR_THREADS), 0, s, pc, pn, pd, (const float4*)scratch, cn, cd,
                       (PtrRecord*)out_colour, out_info, a);
    return hipGetLastError();
}
