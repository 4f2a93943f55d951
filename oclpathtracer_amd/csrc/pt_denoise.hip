// pt_denoise.hip -- the feature-guided a-trous filter of pt_denoise.  include/pt_shim.h states every expression and their order; this
// file follows it operation by operation (the build contracts nothing: -ffp-contract=off, no fast-math; "/" and sqrt are hipcc's
// correctly rounded ones).  Two kernels:
//   pt_denoise_prepare_kernel  moments -> four float4 planes of the scratch: (c, var), (nrm, z), (a, gx), (e, gy)
//   pt_denoise_level_kernel    one a-trous level, launched `levels` times: (c, var) of the level before -> (c, var), the last into `out`
// Shape: workgroups of 32 x 8 pixels, one pixel per lane, a wave = two rows of 32 -- so a wave's loads of one tap are two runs of
// 512 contiguous bytes per plane at EVERY step (a step moves the runs, it does not spread the lanes).  The variance prefilter is fused:
// it is needed at the pixel itself only.  A level comes in two forms with the same per-pixel tap order, hence the same bits:
//   TILE_S = 0     every lane loads its taps from global memory;
//   TILE_S = 1, 2  the workgroup first stages its pixels and their halo of 2 s, (32 + 4 s) x (8 + 4 s) float4 per plane, in LDS
//                  (27 648 and 40 960 bytes) and the taps read that.  At s >= 4 the halo dwarfs the tile: those steps gather globally.
// pt_denoise_spatial runs a third kernel between the two, pt_denoise_pool_kernel (below, with its own comment).
// No atomics, no flags, nothing the host waits for.
#include "pt_denoise.h"

#define PTD_TW 32
#define PTD_TH 8
#define PTD_THREADS (PTD_TW * PTD_TH)

namespace {

struct PtdRecord {   // pt_pixel_moments
    double sum[3];
    double sum2[3];
    uint32_t n, rejected;
};
static_assert(sizeof(PtdRecord) == 56, "moment record layout");

__device__ __forceinline__ float4 ptd_zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// the mean of a record's three channels: (float)(n > 0 ? sum / (double)n : 0)
__device__ __forceinline__ void ptd_mean(const PtdRecord* __restrict__ rec, size_t p, float& x, float& y, float& z)
{
    const PtdRecord& m = rec[p];
    const uint32_t n = m.n;
    const double nd = (double)n;
    x = (float)(n ? m.sum[0] / nd : 0.0);
    y = (float)(n ? m.sum[1] / nd : 0.0);
    z = (float)(n ? m.sum[2] / nd : 0.0);
}

// z = sum[1] > 0 ? (float)(sum[0] / sum[1]) : 0
__device__ __forceinline__ float ptd_depth(const PtdRecord* __restrict__ rec, size_t p)
{
    const double t = rec[p].sum[0], c = rec[p].sum[1];
    return c > 0.0 ? (float)(t / c) : 0.0f;
}

// the pixel of this lane: tiles of 32 x 8 numbered along x, a one-dimensional grid (an image may be 1 x 2^31 - 1 or 2^31 - 1 x 1)
__device__ __forceinline__ void ptd_tile_origin(int width, int& x0, int& y0)
{
    const uint32_t tiles_x = ((uint32_t)width + PTD_TW - 1u) / PTD_TW;
    x0 = (int)((blockIdx.x % tiles_x) * PTD_TW);
    y0 = (int)((blockIdx.x / tiles_x) * PTD_TH);
}

__global__ __launch_bounds__(PTD_THREADS) void pt_denoise_prepare_kernel(const PtdRecord* __restrict__ colour, const PtdRecord* __restrict__ albedo,
                                                                         const PtdRecord* __restrict__ normal, const PtdRecord* __restrict__ depth,
                                                                         const PtdRecord* __restrict__ emission, float4* __restrict__ cv,
                                                                         float4* __restrict__ nz, float4* __restrict__ ag, float4* __restrict__ eg,
                                                                         int width, int height)
{
    int x0, y0;
    ptd_tile_origin(width, x0, y0);
    const int x = x0 + (int)(threadIdx.x % PTD_TW), y = y0 + (int)(threadIdx.x / PTD_TW);
    if (x >= width || y >= height) return;
    const size_t p = (size_t)y * (size_t)width + (size_t)x;

    float4 c = ptd_zero4();
    {
        const PtdRecord& m = colour[p];
        const uint32_t n = m.n;
        const double nd = (double)n;
        double b = 0.0;
        float mean[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double mk = n ? m.sum[k] / nd : 0.0;
            mean[k] = (float)mk;
            if (n >= 2u) {   // pt_moments_resolve's step 1, then its b
                const double t = m.sum[k] * mk;
                const double d = m.sum2[k] - t;
                double v = d / (double)(n - 1u);
                v = v > 0.0 ? v : 0.0;
                const double q = v / nd;
                b = k == 0 ? q : b + q;
            }
        }
        c = make_float4(mean[0], mean[1], mean[2], n >= 2u ? (float)b : 0.0f);
    }
    cv[p] = c;

    float4 n4 = ptd_zero4(), a4 = ptd_zero4(), e4 = ptd_zero4();
    if (normal) ptd_mean(normal, p, n4.x, n4.y, n4.z);
    if (albedo) ptd_mean(albedo, p, a4.x, a4.y, a4.z);
    if (emission) ptd_mean(emission, p, e4.x, e4.y, e4.z);
    if (depth) {
        const int xl = x > 0 ? x - 1 : 0, xr = x + 1 < width ? x + 1 : width - 1;
        const int yu = y > 0 ? y - 1 : 0, yd = y + 1 < height ? y + 1 : height - 1;
        const size_t row = (size_t)y * (size_t)width;
        n4.w = ptd_depth(depth, p);
        a4.w = 0.5f * (ptd_depth(depth, row + (size_t)xr) - ptd_depth(depth, row + (size_t)xl));
        e4.w = 0.5f * (ptd_depth(depth, (size_t)yd * (size_t)width + (size_t)x) - ptd_depth(depth, (size_t)yu * (size_t)width + (size_t)x));
    }
    nz[p] = n4;
    ag[p] = a4;
    eg[p] = e4;
}

struct PtdLevel {
    const float4* cv_in;   // (c, var) of the level before
    const float4* nz;      // (nrm, z)
    const float4* ag;      // (a, gx)
    const float4* eg;      // (e, gy)
    float4* cv_out;
    int32_t width, height, step, squarings;
    uint32_t guides;
    float sigma_l, sigma_z, sigma_a, sigma_e, eps_l, eps_z;
};

template <int TILE_S>
__global__ __launch_bounds__(PTD_THREADS) void pt_denoise_level_kernel(const PtdLevel L)
{
    constexpr int HALO = 2 * TILE_S, HW = PTD_TW + 2 * HALO, HH = PTD_TH + 2 * HALO;
    __shared__ float4 lds[TILE_S ? 4 : 1][TILE_S ? HW * HH : 1];
    const int width = L.width, height = L.height;
    const int s = TILE_S ? TILE_S : L.step;
    const bool g_a = L.guides & PT_DENOISE_GUIDE_ALBEDO, g_n = L.guides & PT_DENOISE_GUIDE_NORMAL, g_z = L.guides & PT_DENOISE_GUIDE_DEPTH,
               g_e = L.guides & PT_DENOISE_GUIDE_EMISSION;
    int x0, y0;
    ptd_tile_origin(width, x0, y0);

    if (TILE_S) {   // stage the tile and its halo; an entry outside the image is never read (its tap is skipped)
        for (int i = (int)threadIdx.x; i < HW * HH; i += PTD_THREADS) {
            const int hx = x0 - HALO + i % HW, hy = y0 - HALO + i / HW;
            if (hx < 0 || hy < 0 || hx >= width || hy >= height) continue;
            const size_t q = (size_t)hy * (size_t)width + (size_t)hx;
            lds[0][i] = L.cv_in[q];
            if (g_n || g_z) lds[1][i] = L.nz[q];
            if (g_a || g_z) lds[2][i] = L.ag[q];
            if (g_e || g_z) lds[3][i] = L.eg[q];
        }
        __syncthreads();
    }

    const int x = x0 + (int)(threadIdx.x % PTD_TW), y = y0 + (int)(threadIdx.x / PTD_TW);
    if (x >= width || y >= height) return;   // (after the only barrier)
    const size_t p = (size_t)y * (size_t)width + (size_t)x;

    // plane k at pixel (qx, qy), inside the image
    auto at = [&](int k, int qx, int qy) -> float4 {
        if (TILE_S) return lds[TILE_S ? k : 0][(qy - y0 + HALO) * HW + (qx - x0 + HALO)];
        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
        return k == 0 ? L.cv_in[q] : k == 1 ? L.nz[q] : k == 2 ? L.ag[q] : L.eg[q];
    };

    const float4 cp = at(0, x, y);
    const float4 np = g_n || g_z ? at(1, x, y) : ptd_zero4();
    const float4 ap = g_a || g_z ? at(2, x, y) : ptd_zero4();
    const float4 ep = g_e || g_z ? at(3, x, y) : ptd_zero4();
    const float lp = (cp.x + cp.y) + cp.z;

    // the variance prefilter: 3 x 3 around p, unscaled
    float gk = 0.0f, gs = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
            const float k = (dx ? 0.25f : 0.5f) * (dy ? 0.25f : 0.5f);
            const float vq = TILE_S ? at(0, qx, qy).w : L.cv_in[(size_t)qy * (size_t)width + (size_t)qx].w;
            gs = gs + k * vq;
            gk = gk + k;
        }
    }
    const float gv = gs / gk;
    const float den_l = L.sigma_l * __builtin_sqrtf(gv) + L.eps_l;

    float sw = 0.0f, sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            // (64-bit: x + 2 * 128 cannot overflow an int, but keep the comparison plain)
            const long long qxl = (long long)x + (long long)dx * s, qyl = (long long)y + (long long)dy * s;
            if (qxl < 0 || qyl < 0 || qxl >= width || qyl >= height) continue;
            const int qx = (int)qxl, qy = (int)qyl;
            const float kx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
            const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
            const float h = kx * ky;
            const float4 cq = at(0, qx, qy);
            float w;
            if (dx == 0 && dy == 0) {
                w = h;
            } else {
                float X = 0.0f;
                float4 nq = ptd_zero4();
                if (g_n || g_z) nq = at(1, qx, qy);
                if (g_z) {
                    const float t = (ap.w * (float)(dx * s)) + (ep.w * (float)(dy * s));
                    X = X + __builtin_fabsf(np.w - nq.w) / (L.sigma_z * __builtin_fabsf(t) + L.eps_z);
                }
                if (g_a) {
                    const float4 aq = at(2, qx, qy);
                    const float d0 = ap.x - aq.x, d1 = ap.y - aq.y, d2 = ap.z - aq.z;
                    X = X + (((d0 * d0) + (d1 * d1)) + (d2 * d2)) / L.sigma_a;
                }
                if (g_e) {
                    const float4 eq = at(3, qx, qy);
                    const float d0 = ep.x - eq.x, d1 = ep.y - eq.y, d2 = ep.z - eq.z;
                    X = X + (((d0 * d0) + (d1 * d1)) + (d2 * d2)) / L.sigma_e;
                }
                const float lq = (cq.x + cq.y) + cq.z;
                X = X + __builtin_fabsf(lp - lq) / den_l;
                float Y = 1.0f + X * 0.0625f;
                Y = Y * Y;
                Y = Y * Y;
                Y = Y * Y;
                Y = Y * Y;
                w = h / Y;
                if (g_n) {
                    float D = ((np.x * nq.x) + (np.y * nq.y)) + (np.z * nq.z);
                    D = D > 0.0f ? D : 0.0f;
                    for (int k = 0; k < L.squarings; ++k) D = D * D;
                    w = w * D;
                }
            }
            sw = sw + w;
            sc0 = sc0 + w * cq.x;
            sc1 = sc1 + w * cq.y;
            sc2 = sc2 + w * cq.z;
            sv = sv + (w * w) * cq.w;
        }
    }
    L.cv_out[p] = make_float4(sc0 / sw, sc1 / sw, sc2 / sw, sv / (sw * sw));
}

// ---- pt_denoise_spatial's POOL (include/pt_shim.h): a pixel with 1 <= n < below takes the pooled per-sample variance of its
// guide-similar 7 x 7 neighbourhood, over its own n.  One lane per pixel; a lane reads the colour RECORDS of its neighbours and the
// prepared guide planes, and writes channel .w of its own pixel of (c, var) alone: nothing in the launch reads what it writes.
// Two forms with the same per-pixel tap order, hence the same bits:
//   TILE = false  every lane loads its 49 taps from global memory: 52 bytes of a record and up to three float4 a tap;
//   TILE = true   the workgroup first stages its pixels and their halo of 3, 38 x 14 entries, in LDS -- one array per field, so that
//                 a row of lanes reads consecutive 4-, 8- and 16-byte words: n 2 128, sum and sum2 12 768 each, three guide planes
//                 8 512 each, 53 200 bytes.
// A workgroup none of whose pixels is listed leaves before it stages or gathers anything: one vote, after each lane has read its own
// n, through a barrier every lane reaches.
#define PTD_PR PT_DENOISE_POOL_RADIUS
#define PTD_PW (PTD_TW + 2 * PTD_PR)
#define PTD_PH (PTD_TH + 2 * PTD_PR)
#define PTD_PN (PTD_PW * PTD_PH)

struct PtdPool {
    const PtdRecord* colour;
    const float4* nz;   // (nrm, z)
    const float4* ag;   // (a, gx)
    const float4* eg;   // (e, gy)
    float4* cv;         // (c, var): .w of a listed pixel is written
    int32_t width, height, squarings;
    uint32_t below, guides;
    float sigma_z, sigma_a, sigma_e, eps_z;
};

template <bool TILE>
__global__ __launch_bounds__(PTD_THREADS) void pt_denoise_pool_kernel(const PtdPool P)
{
    __shared__ uint32_t vote[PTD_THREADS / 64];
    __shared__ uint32_t l_n[TILE ? PTD_PN : 1];
    __shared__ double l_sum[3][TILE ? PTD_PN : 1], l_sum2[3][TILE ? PTD_PN : 1];
    __shared__ float4 l_g[3][TILE ? PTD_PN : 1];
    const int width = P.width, height = P.height;
    const bool g_a = P.guides & PT_DENOISE_GUIDE_ALBEDO, g_n = P.guides & PT_DENOISE_GUIDE_NORMAL, g_z = P.guides & PT_DENOISE_GUIDE_DEPTH,
               g_e = P.guides & PT_DENOISE_GUIDE_EMISSION;
    int x0, y0;
    ptd_tile_origin(width, x0, y0);
    const int x = x0 + (int)(threadIdx.x % PTD_TW), y = y0 + (int)(threadIdx.x / PTD_TW);
    const bool inside = x < width && y < height;
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    const uint32_t n_p = inside ? P.colour[p].n : 0u;
    const bool listed = n_p >= 1u && n_p < P.below;

    // the vote: a wave's ballot, then one word per wave across the barrier (the four words are uniform, so is the exit)
    const bool wave_any = __ballot(listed) != 0ull;
    if (threadIdx.x % 64u == 0u) vote[threadIdx.x / 64u] = wave_any;
    __syncthreads();
    if (!(vote[0] | vote[1] | vote[2] | vote[3])) return;

    if (TILE) {   // stage the tile and its halo; an entry outside the image is never read (its tap is skipped)
        for (int i = (int)threadIdx.x; i < PTD_PN; i += PTD_THREADS) {
            const int hx = x0 - PTD_PR + i % PTD_PW, hy = y0 - PTD_PR + i / PTD_PW;
            if (hx < 0 || hy < 0 || hx >= width || hy >= height) continue;
            const size_t q = (size_t)hy * (size_t)width + (size_t)hx;
            const PtdRecord& m = P.colour[q];
            l_n[i] = m.n;
#pragma unroll
            for (int k = 0; k < 3; ++k) l_sum[k][i] = m.sum[k], l_sum2[k][i] = m.sum2[k];
            if (g_n || g_z) l_g[0][i] = P.nz[q];
            if (g_a) l_g[1][i] = P.ag[q];
            if (g_e) l_g[2][i] = P.eg[q];
        }
        __syncthreads();
    }
    if (!listed) return;   // (after the last barrier)

    // the centre's guides: gx and gy are needed here alone, so the tile's taps never read (e, gy) without the emission guide
    const float4 np = g_n || g_z ? P.nz[p] : ptd_zero4();
    const float4 ap = g_a || g_z ? P.ag[p] : ptd_zero4();
    const float4 ep = g_e || g_z ? P.eg[p] : ptd_zero4();

    double Wn = 0.0, A[3] = { 0.0, 0.0, 0.0 }, B[3] = { 0.0, 0.0, 0.0 };
#pragma unroll 1
    for (int dy = -PTD_PR; dy <= PTD_PR; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= height) continue;
#pragma unroll
        for (int dx = -PTD_PR; dx <= PTD_PR; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= width) continue;
            const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
            const int li = (qy - y0 + PTD_PR) * PTD_PW + (qx - x0 + PTD_PR);
            float w;
            if (dx == 0 && dy == 0) {
                w = 1.0f;
            } else {
                float X = 0.0f;
                float4 nq = ptd_zero4();
                if (g_n || g_z) nq = TILE ? l_g[0][TILE ? li : 0] : P.nz[q];
                if (g_z) {
                    const float t = (ap.w * (float)dx) + (ep.w * (float)dy);
                    X = X + __builtin_fabsf(np.w - nq.w) / (P.sigma_z * __builtin_fabsf(t) + P.eps_z);
                }
                if (g_a) {
                    const float4 aq = TILE ? l_g[1][TILE ? li : 0] : P.ag[q];
                    const float d0 = ap.x - aq.x, d1 = ap.y - aq.y, d2 = ap.z - aq.z;
                    X = X + (((d0 * d0) + (d1 * d1)) + (d2 * d2)) / P.sigma_a;
                }
                if (g_e) {
                    const float4 eq = TILE ? l_g[2][TILE ? li : 0] : P.eg[q];
                    const float d0 = ep.x - eq.x, d1 = ep.y - eq.y, d2 = ep.z - eq.z;
                    X = X + (((d0 * d0) + (d1 * d1)) + (d2 * d2)) / P.sigma_e;
                }
                float Y = 1.0f + X * 0.0625f;
                Y = Y * Y;
                Y = Y * Y;
                Y = Y * Y;
                Y = Y * Y;
                w = 1.0f / Y;
                if (g_n) {
                    float D = ((np.x * nq.x) + (np.y * nq.y)) + (np.z * nq.z);
                    D = D > 0.0f ? D : 0.0f;
                    for (int k = 0; k < P.squarings; ++k) D = D * D;
                    w = w * D;
                }
            }
            const double wd = (double)w;
            const PtdRecord& m = P.colour[q];
            Wn = Wn + wd * (double)(TILE ? l_n[TILE ? li : 0] : m.n);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                A[k] = A[k] + wd * (TILE ? l_sum[k][TILE ? li : 0] : m.sum[k]);
                B[k] = B[k] + wd * (TILE ? l_sum2[k][TILE ? li : 0] : m.sum2[k]);
            }
        }
    }
    double Q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double M = A[k] / Wn;
        const double T = M * M;
        double V = B[k] / Wn - T;
        V = V > 0.0 ? V : 0.0;
        Q[k] = V / (double)n_p;
    }
    P.cv[p].w = (float)((Q[0] + Q[1]) + Q[2]);
}

}   // namespace

static void ptd_planes(float4* scratch, const PtDenoiseArgs& a, float4*& cv, float4*& nz, float4*& ag, float4*& eg, float4* pong[2],
                       uint32_t& tiles)
{
    const size_t npix = (size_t)a.width * (size_t)a.height;
    tiles = (((uint32_t)a.width + PTD_TW - 1u) / PTD_TW) * (((uint32_t)a.height + PTD_TH - 1u) / PTD_TH);
    cv = scratch, nz = scratch + npix, ag = scratch + 2 * npix, eg = scratch + 3 * npix;
    pong[0] = scratch + 4 * npix, pong[1] = scratch + 5 * npix;
}

// prepare: (c, var) into the scratch, or into `out` when no level follows
static hipError_t ptd_prepare(const void* colour, const void* albedo, const void* normal, const void* depth, const void* emission,
                              float4* scratch, float4* out, const PtDenoiseArgs& a, hipStream_t s)
{
    float4 *cv, *nz, *ag, *eg, *pong[2];
    uint32_t tiles;
    ptd_planes(scratch, a, cv, nz, ag, eg, pong, tiles);
    hipLaunchKernelGGL(pt_denoise_prepare_kernel, dim3(tiles), dim3(PTD_THREADS), 0, s, (const PtdRecord*)colour, (const PtdRecord*)albedo,
                       (const PtdRecord*)normal, (const PtdRecord*)depth, (const PtdRecord*)emission, a.levels ? cv : out, nz, ag, eg, a.width,
                       a.height);
    return hipGetLastError();
}

static hipError_t ptd_levels(float4* scratch, float4* out, const PtDenoiseArgs& a, int gather, hipStream_t s)
{
    float4 *cv, *nz, *ag, *eg, *pong[2];
    uint32_t tiles;
    ptd_planes(scratch, a, cv, nz, ag, eg, pong, tiles);
    hipError_t e = hipSuccess;
    for (int i = 0; i < a.levels && e == hipSuccess; ++i) {
        PtdLevel L;
        L.cv_in = i == 0 ? cv : pong[(i - 1) & 1];
        L.nz = nz, L.ag = ag, L.eg = eg;
        L.cv_out = i == a.levels - 1 ? out : pong[i & 1];
        L.width = a.width, L.height = a.height, L.step = 1 << i, L.squarings = a.squarings;
        L.guides = a.guides;
        L.sigma_l = a.sigma_l, L.sigma_z = a.sigma_z, L.sigma_a = a.sigma_a, L.sigma_e = a.sigma_e, L.eps_l = a.eps_l, L.eps_z = a.eps_z;
        // PT_DENOISE_GATHER_AUTO is the faster form per step as measured on the MI355X (profiles/denoise/rates.txt): at 1024^2 the tile
        // takes 0.079 and 0.084 ms at steps 1 and 2, the global gathers 0.181 and 0.176 ms -- so auto is the tile wherever it exists
        const bool tile = gather != PT_DENOISE_GATHER_GLOBAL && i < 2;
        if (tile && i == 0) hipLaunchKernelGGL(pt_denoise_level_kernel<1>, dim3(tiles), dim3(PTD_THREADS), 0, s, L);
        else if (tile) hipLaunchKernelGGL(pt_denoise_level_kernel<2>, dim3(tiles), dim3(PTD_THREADS), 0, s, L);
        else hipLaunchKernelGGL(pt_denoise_level_kernel<0>, dim3(tiles), dim3(PTD_THREADS), 0, s, L);
        e = hipGetLastError();
    }
    return e;
}

hipError_t ptk_denoise(const void* colour, const void* albedo, const void* normal, const void* depth, const void* emission,
                       float4* scratch, float4* out, const PtDenoiseArgs& a, int gather, hipStream_t s)
{
    const hipError_t e = ptd_prepare(colour, albedo, normal, depth, emission, scratch, out, a, s);
    return e == hipSuccess ? ptd_levels(scratch, out, a, gather, s) : e;
}

hipError_t ptk_denoise_spatial(const void* colour, const void* albedo, const void* normal, const void* depth, const void* emission,
                               float4* scratch, float4* out, const PtDenoiseArgs& a, int32_t below, int gather, int pool_form, hipStream_t s)
{
    hipError_t e = ptd_prepare(colour, albedo, normal, depth, emission, scratch, out, a, s);
    if (e == hipSuccess && below > 1) {   // (0 and 1 name no pixel)
        float4 *cv, *nz, *ag, *eg, *pong[2];
        uint32_t tiles;
        ptd_planes(scratch, a, cv, nz, ag, eg, pong, tiles);
        PtdPool P;
        P.colour = (const PtdRecord*)colour;
        P.nz = nz, P.ag = ag, P.eg = eg;
        P.cv = a.levels ? cv : out;
        P.width = a.width, P.height = a.height, P.squarings = a.squarings;
        P.below = (uint32_t)below, P.guides = a.guides;
        P.sigma_z = a.sigma_z, P.sigma_a = a.sigma_a, P.sigma_e = a.sigma_e, P.eps_z = a.eps_z;
        // PT_DENOISE_POOL_AUTO is the faster form as measured on the MI355X (profiles/denoise_spatial/rates.txt): at 1024^2 with every
        // pixel listed the tile takes 0.19 ms, the global gathers 0.75 ms; with 3 % listed after a camera move both take 0.18 ms
        if (pool_form == PT_DENOISE_POOL_GLOBAL) hipLaunchKernelGGL(pt_denoise_pool_kernel<false>, dim3(tiles), dim3(PTD_THREADS), 0, s, P);
        else hipLaunchKernelGGL(pt_denoise_pool_kernel<true>, dim3(tiles), dim3(PTD_THREADS), 0, s, P);
        e = hipGetLastError();
    }
    return e == hipSuccess ? ptd_levels(scratch, out, a, gather, s) : e;
}
