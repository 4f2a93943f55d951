// pt_secmask.h -- candidate masks of SECONDARY rays: which triangles a ray that leaves triangle k can hit.
// One implementation for the device (pt_secondary_mask_kernel, pt_trace_body: pt_kernels.hip) and for the host (g++ compiles this
// header into the stand-alone program of tests/test_secondary_masks_cpu.py).  No contraction on either side (-ffp-contract=off).
//
// A path that continues after shading starts its next ray at o = p + 0.01 wi (:257), p the hit point on triangle k: the origin
// lies within about 0.01 of k's plane, over k or just beside it.  What such a ray can hit depends on the scene alone -- not on the
// camera, the image or the frame -- so the answer is tabulated once per scene: one uint2 (pass 1's bit order, the format of
// pt_primary_mask_kernel) per CELL = (origin triangle k, tile (iu, iv) of k's plane, direction cell (face, ia, ib) of a cube map).
// The trace kernel classifies a ray from its own floats o, d and k (pt_sm_classify), loads the cell's mask and runs pass 2 on it;
// pass 1 is not run.  Pass 2 applies the reference's whole test exactly, so the masks only have to be SUPERSETS:
//
//   CONTRACT.  Bit j of a cell is cleared only if the reference's test (GenerateColors.cl:96-125, against the initial tmax)
//   accepts triangle j for NO ray that pt_sm_classify can map to the cell.
//
// ---- the classification (binary32, pt_sm_classify) and its real-number preimage ------------------------------------------------
// Triangle k = {p1, e1, e2} (the floats of the prepared record, exact numbers here), n = e1 x e2, nh = n / |n|.  Every point is
// o = p1 + uu e1 + vv e2 + hh nh for unique reals (uu, vv, hh).  With the dual vectors a* = (e2 x n) / |n|^2, b* = (n x e1) / |n|^2
// (a* . e1 = 1, a* . e2 = 0, a* . nh = 0, likewise b*):  uu = a* . (o - p1), vv = b* . (o - p1), hh = nh . (o - p1).
// The record PtSmTri holds three affine forms, made in binary64 and rounded to binary32:
//     tu = A . o + A3 ~ (uu + G) / (1 + 2 G) * T       tv likewise       th = N . o + N3 ~ hh / H
// G = PT_SM_GUARD is a guard band: the tiles cover uu, vv in [-G, 1 + G], so an origin pushed 0.01 past an edge of k still has a
// tile.  A triangle gets a table only if the band holds that push whatever its direction: 0.0101 |a*| <= G and 0.0101 |b*| <= G (edges
// and heights of about 0.65 and more).  A ray from a hit inside such a triangle is then covered but for rounding; a smaller triangle has
// no table (pt_sm_geom: invalid), and the host declines the whole table for a scene that holds one (pt_shim.hip: refresh_smask), because a
// lane with the all-ones mask makes its whole wave's pass 2 long: 20 % of the rays of a scene of such triangles were uncovered.  (They cover the whole parallelogram, not only the triangle: the origin over the other half of a quad is as common.)
// H = 0.0101 + 32 u max_i(|p1_i| + |e1_i| + |e2_i|) is the plane distance the table is proved for: 0.01 |wi| of :257 (wi is unit to
// rounding) and the rounding of the hit point.  Nothing is assumed about it: the device tests |th| <= 1 with its own floats.
// A ray is COVERED when  0 <= tu < T,  0 <= tv < T,  |th| <= 1  and  0.999 <= fl(d . d) <= 1.001; its tile is (trunc tu, trunc tv).
// Any NaN fails a comparison: uncovered.  An uncovered ray keeps every triangle (the caller gives it the all-ones mask).
//   Rounding of a form.  The device evaluates fma(A2, oz, fma(A1, oy, fma(A0, ox, A3))): three roundings, each relative 2^-24 =: u
//   of a partial sum bounded by Q = sum_i |A_i o_i| + |A3|, and the four constants are within u relative of their real values
//   (binary64 work is 2^-29 times finer).  So |tu - tu_real| <= 4.02 u Q.  Q needs a bound on o.  Let m >= 1 be the least number with
//   |uu|, |vv| <= m (1 + G) and |hh| <= m H; then |o_i - p1_i| <= m ((1 + G)(|e1_i| + |e2_i|) + H) and Q <= m E with
//   E = sum_i |A_i| (|p1_i| + (1 + G)(|e1_i| + |e2_i|) + H) + |A3|.  A covered ray has its three floats in range, so each real
//   form is in range up to its rounding: m <= 1 + 4.02 u m Emax, Emax the largest of E_u / T, E_v / T, E_h.  The builder REQUIRES
//   8 u E_u <= 0.25, 8 u E_v <= 0.25 (a quarter of a tile) and 8 u E_h <= 0.25 (else triangle k has no table: its record is NaN,
//   every ray from it is uncovered, its cells are all-ones); then 4.02 u Emax <= 0.126, m <= 1.15 and |tu - tu_real| <= 4.02 * 1.15
//   u E < 8 u E =: du (tile units), dv likewise, |th - th_real| <= 8 u E_h =: dh.  (A triangle far from the origin of coordinates
//   meets the limit through E_h: |p1| / H roundings of 2^-24.)
//   Preimage of tile (iu, iv):  tu_real in [iu - du, iu + 1 + du], so uu = tu_real (1 + 2G) / T - G within ru = (0.5 + du)(1 + 2G) / T
//   of its centre uc; vv likewise; |hh| <= Hr = H (1 + dh).  The origins of a cell are oc + Du e1 + Dv e2 + Dh nh with
//   oc = p1 + uc e1 + vc e2, |Du| <= ru, |Dv| <= rv, |Dh| <= Hr: a boundary origin belongs to both neighbours' sets.
// The direction.  m = the axis of the largest |d_i| (ties: the lower axis), a = (m + 1) % 3, b = (m + 2) % 3, face = 2 m + (d_m < 0),
//     ca = fma(d_a * r, C / 2, C / 2), r ~ 1 / |d_m|,  ia = clamp(trunc ca, 0, C - 1),  ib likewise.
// r is the quotient rounded (host) or v_rcp_f32 (device, 1 ulp): relative 2^-23 at the most; the product and the fma add 2^-24 each of
// values below 1 and C: |ca - ca_real| <= (2.5 * 2^-23) C / 2 + 2^-24 C < 3.4e-6 for C <= 16.  The builder takes dc = 1e-4 cell units.
// |d_a| <= |d_m| holds for the floats, so the real ratio qa = d_a / |d_m| is in [-1, 1] and in [(ia - dc) 2 / C - 1, (ia + 1 + dc) 2 / C - 1].
// With L = |d|_2: fl(d . d) in [0.999, 1.001] gives L in [0.9994, 1.0006] (three roundings of u).  d = L g (s, qa, qb) in the axes
// (m, a, b), g = (1 + qa^2 + qb^2)^(-1/2), which is largest where |qa|, |qb| are smallest in the cell and smallest where they are
// largest.  So |d_m| in [0.9994 gmin, 1.0006 gmax] =: [l0, l1] and d_a in the interval product of [qa0, qa1] and [l0, l1]; d_b
// likewise: a BOX dc +- rd for the direction.  (The trace kernels' directions are unit to 1 +- 4e-7, the UNIT_DIR comment of
// pt_kernels.hip; nothing here relies on it -- the classification tests the length itself.)
//
// ---- the bounds (binary64, pt_sm_entry) -------------------------------------------------------------------------------------------
// Target triangle j = {q1, f1, f2}, tvec = o - q1 = tc + D, tc = oc - q1, D = Du e1 + Dv e2 + Dh nh, d = dc + e, |e_i| <= rd_i.  The
// reference's four numerators, as real forms:
//     det = d . (f2 x f1)                   linear in d
//     un  = d . (f2 x tvec)                 bilinear
//     vn  = d . (tvec x f1)                 bilinear
//     tn  = tvec . (f1 x f2)                linear in o
// For a vector X:  radd(X) = sum_i rd_i |X_i|  bounds |e . X|;  rado(X) = ru |e1 . X| + rv |e2 . X| + Hr |nh . X|  bounds |D . X|.
//     det: centre dc . Kd, Kd = f2 x f1;              radius radd(Kd)
//     un:  centre dc . (f2 x tc);                     radius radd(f2 x tc) + rado(dc x f2) + X(f2)       [dc . (f2 x D) = D . (dc x f2)]
//     vn:  centre dc . (tc x f1);                     radius radd(tc x f1) + rado(f1 x dc) + X(f1)       [dc . (D x f1) = D . (f1 x dc)]
//     tn:  centre tc . G, G = f1 x f2;                radius rado(G)
// X(f) = sum_i rd_i (ru |(f x e1)_i| + rv |(f x e2)_i| + Hr |(f x nh)_i|) bounds the second-order term |e . (f x D)|.
// The reference's own rounding: its floats un_ref .. differ from these real forms by at most (the accounting of the comment above
// pt_primary_mask_kernel, 7 u S per form with S = |a|_1 |b|_1 for a . (d x b); here tvec = fl(o - q1) is not a constant but one more
// rounding of u per component, and tn_ref = fl_dot(f2, fl_cross(tvec, f1)) errs by less than 6.3 u |tvec|_1 |f1|_1 |f2|_1)
//     rho = 32 u S,   S_det = |f1|_1 |f2|_1,  S_u = tv1 |f2|_1,  S_v = tv1 |f1|_1,  S_t = tv1 |f1|_1 |f2|_1,
//     tv1 = |tc|_1 + ru |e1|_1 + rv |e2|_1 + 3 Hr >= |tvec|_1 over the cell
// (32 against the 9 needed).  Radius and rho are inflated by 0.1 % against the builder's own (binary64) rounding, plus an absolute
// 2e-24 that covers the -1e-24 threshold of pt_tri_pass1 and every underflow.  With lo / hi = centre -+ that:
//     the reference accepts only if  det_ref >= 1e-8,  un_ref >= -1e-24,  vn_ref >= -1e-24,  un_ref + vn_ref <= det_ref * 1.000001,  tn_ref > 0
// (the thresholds derived above pt_primary_mask_kernel), so bit j is CLEARED only when, for the whole cell,
//     det_hi < 0.999e-8   or   un_hi < 0   or   vn_hi < 0   or   un_lo + vn_lo > det_hi * 1.000002   or   tn_hi <= 0.
// REFINEMENT.  First-order bounds over a whole cell are loose (the Cornell box: 6.9 candidates per ray at T = C = 8 where pass 1 keeps
// 3.3), so pt_sm_entry refines, per target triangle j: a BOX is a product of sub-ranges of the cell's four ranges -- [iu - du, iu + 1 + du],
// the same for v, and the two ratio ranges -- and is bounded exactly as a cell above.  Starting at the whole cell a box is, in this order,
//     CLEARED  when one of the five bounds above (pt_sm_keep) or the separating plane below (pt_sm_sep) shows that no ray of it is accepted;
//     KEPT     when a witness ray of it is accepted: the box's centre origin at plane distance 0, +Hr or -Hr and its centre direction pass
//              the real forms strictly (pt_sm_witness, binary64).  A witness only spares work: keeping a bit is always within the CONTRACT;
//     KEPT     when it stands at depth PT_SM_DEPTH, or when PT_SM_BUDGET boxes of the pair (cell, j) have been bounded;
//     otherwise all four ranges are halved, and j is kept when any of the 16 children keeps it.
// The children's preimages cover the parent's (the halves of a width are inflated by 1e-9 of it: the cuts are formed in binary64), so a
// bit is cleared only when boxes that cover the whole cell were each cleared.  The walk is depth first in a fixed order without recursion:
// the box at depth L is named by L bits in each of four index words, whose lowest bits are the child counter of that depth (the stack).
// Every comparison is written so that a NaN keeps the bit.  A degenerate origin triangle (n = 0, a non-finite or oversized
// constant: pt_sm_geom) has all-ones cells.  Directions below the surface are bounded like any other.
//
// ---- the separating plane (binary64, pt_sm_sep) ---------------------------------------------------------------------------------
// Each of the five bounds asks whether some ray of the box passes ONE condition; none asks whether one ray passes all of them.  The
// plane does.  For a real ray with det != 0 Cramer's rule gives, exactly,  o + (tn / det) d = q1 + (un / det) f1 + (vn / det) f2.  Let
// det_lo = centre - radius - rho_det > 0 bound det from below over the box (the quantities of pt_sm_keep).  By the acceptance
// conditions above and |x_ref - x| <= rho_x, a ray the reference accepts has, with u = un / det, v = vn / det, t = tn / det,
//     u >= -eu,  eu = (rho_u + 1e-24) / det_lo;      v >= -ev likewise;      t >= -et,  et = rho_t / det_lo;
//     u + v <= 1 + es,  es = 2e-6 + (1.000001 rho_det + rho_u + rho_v) / det_lo        [un + vn <= 1.000001 (det + rho_det) + rho_u + rho_v]
// so its point P = o + t d lies in the INFLATED triangle with the corners (u, v) = (-eu, -ev), (1 + es + ev, -ev), (-eu, 1 + es + eu).
// Also t |d|_2 = |P - o|_2 <= |tvec|_1 + (|u| + |v|)-weighted edges <= tv1 + (1 + eu + ev + es)(|f1|_1 + |f2|_1), and |d|_2 >= 0.9994:
// t <= R = 1.001 (tv1 + (1 + eu + ev + es)(|f1|_1 + |f2|_1)).  Now take ANY vector w.  Over the box  w . d <= mw = w . dc + radd(w)  and
// |w . d| <= aw = |w . dc| + radd(w);  w . o <= w . oc + rado(w).  Hence for every accepted ray of the box, relative to q1,
//     w . (P - q1)  <=  w . tc + rado(w) + et aw + R max(mw, 0)            [t w . d <= R mw for t >= 0, <= et aw for -et <= t < 0]
// while w . (P - q1) >= the least of u (w . f1) + v (w . f2) over the three corners.  If the first is LESS than the second no ray of
// the box is accepted: the bit is cleared.  The choice of w needs no proof, only the inequality does.  pt_sm_sep tries, for each
// a of {e1, e2, nh, f1, f2, f2 - f1}, the plane through a and an extreme direction dk of the box: w = +-(a x dk), the sign towards
// the triangle's centroid, dk the corner of the direction box that maximises w . d (found from w = +-(a x dc) in two rounds; then
// mw is a rounding of 0).  The radii and the rho are inflated by 0.1 % and the absolute 2e-24 as above, and 1e-13 |w|_1 R is added
// against the builder's own rounding of the two sides (a few 1e-16 of |w|_1 times lengths below R).  The test is used only where
// det_lo > PT_SM_SEP_DET |f1|_1 |f2|_1 (the e are then at most 0.02 tv1 / |f|_1); elsewhere the box has the five bounds alone.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_SM_HD __host__ __device__ static inline
#else
#define PT_SM_HD static inline
#endif

// tiles per edge of a triangle's plane, direction cells per edge of a cube face (profiles/secondary_masks/steps.txt; the split between
// the two, and the odd C: profiles/table_shape/steps.txt)
#ifndef PT_SM_T
#define PT_SM_T 12
#endif
#ifndef PT_SM_C
#define PT_SM_C 11
#endif
// the builder's refinement (pt_sm_entry): the depth at which a box is kept, the boxes bounded per pair (cell, target triangle) before
// it is kept, and the least det_lo / (|f1|_1 |f2|_1) at which the separating plane is tried (profiles/tight_masks/steps.txt)
#ifndef PT_SM_DEPTH
#define PT_SM_DEPTH 3
#endif
#ifndef PT_SM_BUDGET
#define PT_SM_BUDGET 96
#endif
#ifndef PT_SM_SEP_DET
#define PT_SM_SEP_DET 1e-4
#endif
#define PT_SM_GUARD (1.0 / 64.0)
#define PT_SM_DIRS (6 * PT_SM_C * PT_SM_C)
#define PT_SM_TRI_ENTRIES (PT_SM_T * PT_SM_T * PT_SM_DIRS)
#define PT_SM_TRI_MAX 64
// the table: PT_SM_TRI_MAX classification records, padded to PT_SM_HEAD_ENTRIES uint2, then ntri * PT_SM_TRI_ENTRIES masks
struct PtSmTri { float A[4], B[4], N[4]; };   // tu = A . o + A[3], tv = B . o + B[3], th = N . o + N[3]
#define PT_SM_HEAD_ENTRIES (PT_SM_TRI_MAX * sizeof(PtSmTri) / 8)
#define PT_SM_TABLE_BYTES(ntri) ((PT_SM_HEAD_ENTRIES + (size_t)(ntri) * PT_SM_TRI_ENTRIES) * 8)
// the classification's rounding bound (|ca - ca_real| < 3.4e-6 against the builder's dc = 1e-4, above) is worked out for C <= 16; C / 2 and
// C - 1 are exact floats for any such C, odd or even.  The trace kernel and the builder address an entry by a 32-bit byte offset
static_assert(PT_SM_T >= 1 && PT_SM_C >= 1 && PT_SM_C <= 16, "pt_sm_classify's rounding bound is derived for C <= 16");
static_assert(PT_SM_TABLE_BYTES(PT_SM_TRI_MAX) < 0x100000000ull, "an entry's byte offset in the largest table must fit 32 bits");

struct PtSmMask { unsigned x, y; };   // uint2

// ---- the classification ---------------------------------------------------------------------------------------------------------
PT_SM_HD float pt_sm_form(const float* F, float ox, float oy, float oz)
{
    return __builtin_fmaf(F[2], oz, __builtin_fmaf(F[1], oy, __builtin_fmaf(F[0], ox, F[3])));
}

// the cell of the ray (o, d) leaving triangle k, as an index into the masks behind the table's head; false: uncovered
PT_SM_HD bool pt_sm_classify(const float* A, const float* B, const float* N, float ox, float oy, float oz, float dx, float dy, float dz,
                             unsigned k, unsigned* entry)
{
    const float tu = pt_sm_form(A, ox, oy, oz), tv = pt_sm_form(B, ox, oy, oz), th = pt_sm_form(N, ox, oy, oz);
    const float dd = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
    const bool covered = (tu >= 0.0f) & (tu < (float)PT_SM_T) & (tv >= 0.0f) & (tv < (float)PT_SM_T) & (__builtin_fabsf(th) <= 1.0f) &
                         (dd >= 0.999f) & (dd <= 1.001f);
    const float ax = __builtin_fabsf(dx), ay = __builtin_fabsf(dy), az = __builtin_fabsf(dz);
    const bool mx = (ax >= ay) & (ax >= az), my = ay >= az;
    const unsigned m = mx ? 0u : my ? 1u : 2u;
    const float dm = mx ? dx : my ? dy : dz;
    const float da = mx ? dy : my ? dz : dx;
    const float db = mx ? dz : my ? dx : dy;
#if defined(__HIP_DEVICE_COMPILE__)
    const float r = __builtin_amdgcn_rcpf(__builtin_fabsf(dm));
#else
    const float r = 1.0f / __builtin_fabsf(dm);
#endif
    // (an uncovered ray's numbers may be anything: they are replaced before the conversions, whose result is never used then)
    const float ca = covered ? __builtin_fmaf(da * r, 0.5f * PT_SM_C, 0.5f * PT_SM_C) : 0.0f;
    const float cb = covered ? __builtin_fmaf(db * r, 0.5f * PT_SM_C, 0.5f * PT_SM_C) : 0.0f;
    const float ca_c = __builtin_fminf(__builtin_fmaxf(ca, 0.0f), (float)(PT_SM_C - 1));
    const float cb_c = __builtin_fminf(__builtin_fmaxf(cb, 0.0f), (float)(PT_SM_C - 1));
    const unsigned ia = (unsigned)(int)ca_c, ib = (unsigned)(int)cb_c;
    const unsigned iu = (unsigned)(int)(covered ? tu : 0.0f), iv = (unsigned)(int)(covered ? tv : 0.0f);
    const unsigned face = 2u * m + (dm < 0.0f ? 1u : 0u);
    *entry = ((k * PT_SM_T + iu) * PT_SM_T + iv) * PT_SM_DIRS + (face * PT_SM_C + ia) * PT_SM_C + ib;
    return covered;
}

// ---- the builder ------------------------------------------------------------------------------------------------------------------
struct PtSmV3 { double x, y, z; };
PT_SM_HD PtSmV3 pt_sm_v(double x, double y, double z) { PtSmV3 r = { x, y, z }; return r; }
PT_SM_HD PtSmV3 pt_sm_vf(const float* p) { return pt_sm_v((double)p[0], (double)p[1], (double)p[2]); }
PT_SM_HD PtSmV3 pt_sm_cross(PtSmV3 a, PtSmV3 b) { return pt_sm_v(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
PT_SM_HD double pt_sm_dot(PtSmV3 a, PtSmV3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
PT_SM_HD PtSmV3 pt_sm_sub(PtSmV3 a, PtSmV3 b) { return pt_sm_v(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_SM_HD PtSmV3 pt_sm_axpy(double s, PtSmV3 a, PtSmV3 b) { return pt_sm_v(s * a.x + b.x, s * a.y + b.y, s * a.z + b.z); }
PT_SM_HD double pt_sm_n1(PtSmV3 a) { return fabs(a.x) + fabs(a.y) + fabs(a.z); }
PT_SM_HD double pt_sm_absdot(PtSmV3 r, PtSmV3 a) { return r.x * fabs(a.x) + r.y * fabs(a.y) + r.z * fabs(a.z); }

#define PT_SM_U 5.9604644775390625e-8   // 2^-24

// an origin triangle's frame: what the classification record is made from and what the bounds need of it
struct PtSmGeom {
    PtSmV3 p1, e1, e2, nh;
    double H, du, dv, dh;   // the plane distance; the forms' rounding in tile units (du, dv) and in units of H (dh)
    PtSmTri rec;            // NaN when !valid
    bool valid;
};

PT_SM_HD void pt_sm_form_make(PtSmV3 w, double c, double scale, PtSmV3 reach, PtSmV3 p1, float* F, double* E)
{
    // F . o + F[3] ~ (w . (o - p1) + c) * scale; E: the bound of sum |F_i o_i| + |F[3]| over the origins within `reach` of p1
    F[0] = (float)(w.x * scale); F[1] = (float)(w.y * scale); F[2] = (float)(w.z * scale);
    F[3] = (float)((c - pt_sm_dot(w, p1)) * scale);
    *E = fabs((double)F[0]) * (fabs(p1.x) + reach.x) + fabs((double)F[1]) * (fabs(p1.y) + reach.y) + fabs((double)F[2]) * (fabs(p1.z) + reach.z) +
         fabs((double)F[3]);
}

PT_SM_HD PtSmGeom pt_sm_geom(const float* p1, const float* e1, const float* e2)
{
    PtSmGeom g;
    g.p1 = pt_sm_vf(p1); g.e1 = pt_sm_vf(e1); g.e2 = pt_sm_vf(e2);
    const PtSmV3 n = pt_sm_cross(g.e1, g.e2);
    const double nn = pt_sm_dot(n, n), ln = sqrt(nn);
    g.nh = pt_sm_v(n.x / ln, n.y / ln, n.z / ln);
    const PtSmV3 as = pt_sm_cross(g.e2, n), bs = pt_sm_cross(n, g.e1);   // a* |n|^2, b* |n|^2
    const double ext = fmax(fabs(g.p1.x) + fabs(g.e1.x) + fabs(g.e2.x), fmax(fabs(g.p1.y) + fabs(g.e1.y) + fabs(g.e2.y), fabs(g.p1.z) + fabs(g.e1.z) + fabs(g.e2.z)));
    g.H = 0.0101 + 32.0 * PT_SM_U * ext;
    const double G = PT_SM_GUARD, st = (double)PT_SM_T / (1.0 + 2.0 * G);
    const PtSmV3 reach = pt_sm_v((1.0 + G) * (fabs(g.e1.x) + fabs(g.e2.x)) + g.H, (1.0 + G) * (fabs(g.e1.y) + fabs(g.e2.y)) + g.H,
                                 (1.0 + G) * (fabs(g.e1.z) + fabs(g.e2.z)) + g.H);
    double Eu, Ev, Eh;
    pt_sm_form_make(pt_sm_v(as.x / nn, as.y / nn, as.z / nn), G, st, reach, g.p1, g.rec.A, &Eu);
    pt_sm_form_make(pt_sm_v(bs.x / nn, bs.y / nn, bs.z / nn), G, st, reach, g.p1, g.rec.B, &Ev);
    pt_sm_form_make(g.nh, 0.0, 1.0 / g.H, reach, g.p1, g.rec.N, &Eh);
    g.du = 8.0 * PT_SM_U * Eu; g.dv = 8.0 * PT_SM_U * Ev; g.dh = 8.0 * PT_SM_U * Eh;
    bool ok = nn > 0.0 && g.du <= 0.25 && g.dv <= 0.25 && g.dh <= 0.25;   // (a NaN fails)
    // the guard band must hold the ray's offset: 0.0101 along any direction of the plane moves uu by at most 0.0101 |a*|, vv by 0.0101 |b*|
    ok = ok && 0.0101 * sqrt(pt_sm_dot(as, as)) / nn <= G && 0.0101 * sqrt(pt_sm_dot(bs, bs)) / nn <= G;
    for (int i = 0; i < 4; ++i)
        ok = ok && fabs((double)g.rec.A[i]) < 1e30 && fabs((double)g.rec.B[i]) < 1e30 && fabs((double)g.rec.N[i]) < 1e30;
    g.valid = ok;
    if (!ok)
        for (int i = 0; i < 4; ++i) g.rec.A[i] = g.rec.B[i] = g.rec.N[i] = __builtin_nanf("");
    return g;
}

// the record alone (the trace kernel's gather)
PT_SM_HD PtSmTri pt_sm_tri_record(const float* p1, const float* e1, const float* e2) { return pt_sm_geom(p1, e1, e2).rec; }

PT_SM_HD PtSmMask pt_sm_all_ones(int ntri)
{
    PtSmMask m;
    const int n0 = ntri < 32 ? ntri : 32, n1 = ntri - 32 < 0 ? 0 : ntri - 32 > 32 ? 32 : ntri - 32;
    m.x = n0 == 32 ? ~0u : (1u << n0) - 1u;
    m.y = n1 == 32 ? ~0u : (1u << n1) - 1u;
    return m;
}

// [lo, hi] of q / |d_m| for direction cell index i, clipped to [-1, 1]
PT_SM_HD void pt_sm_ratio_range(int i, double* lo, double* hi)
{
    const double dc = 1e-4;
    *lo = fmax(-1.0, ((double)i - dc) * (2.0 / PT_SM_C) - 1.0);
    *hi = fmin(1.0, ((double)i + 1.0 + dc) * (2.0 / PT_SM_C) - 1.0);
}
PT_SM_HD double pt_sm_absmin(double lo, double hi) { return lo > 0.0 ? lo : hi < 0.0 ? -hi : 0.0; }
PT_SM_HD double pt_sm_absmax(double lo, double hi) { return fmax(fabs(lo), fabs(hi)); }
PT_SM_HD void pt_sm_set(PtSmV3* v, unsigned axis, double x) { if (axis == 0u) v->x = x; else if (axis == 1u) v->y = x; else v->z = x; }

// bit j of the cell's mask over ONE box, by the five bounds: origins oc + Du e1 + Dv e2 + Dh nh (|Du| <= ru, |Dv| <= rv, |Dh| <= Hr), directions dc +- rd
PT_SM_HD bool pt_sm_keep(const PtSmGeom& g, PtSmV3 oc, double ru, double rv, double Hr, PtSmV3 dc, PtSmV3 rd, const float* tj)
{
    const double INF = 1.001, ABS = 2e-24, RHO = 32.0 * PT_SM_U;
    const PtSmV3 q1 = pt_sm_vf(tj), f1 = pt_sm_vf(tj + 3), f2 = pt_sm_vf(tj + 6);
    const PtSmV3 tc = pt_sm_sub(oc, q1);
    const double f1n = pt_sm_n1(f1), f2n = pt_sm_n1(f2);
    const double tv1 = pt_sm_n1(tc) + ru * pt_sm_n1(g.e1) + rv * pt_sm_n1(g.e2) + 3.0 * Hr;
    // det
    const PtSmV3 Kd = pt_sm_cross(f2, f1);
    const double det_hi = pt_sm_dot(dc, Kd) + ((pt_sm_absdot(rd, Kd) + RHO * f1n * f2n) * INF + ABS);
    if (det_hi < 0.999e-8) return false;                                                // :100 (a NaN fails the comparison and goes on)
    // tn = tvec . (f1 x f2)
    const PtSmV3 Gt = pt_sm_cross(f1, f2);
    const double tn_c = pt_sm_dot(tc, Gt);
    const double tn_r = (ru * fabs(pt_sm_dot(g.e1, Gt)) + rv * fabs(pt_sm_dot(g.e2, Gt)) + Hr * fabs(pt_sm_dot(g.nh, Gt)) + RHO * tv1 * f1n * f2n) * INF + ABS;
    if (tn_c + tn_r <= 0.0) return false;                                               // :125, t > 0
    // un = d . (f2 x tvec)
    const PtSmV3 Ku = pt_sm_cross(f2, tc), Du = pt_sm_cross(dc, f2);
    const PtSmV3 x1 = pt_sm_cross(f2, g.e1), x2 = pt_sm_cross(f2, g.e2), x3 = pt_sm_cross(f2, g.nh);
    const double un_c = pt_sm_dot(dc, Ku);
    const double un_r = (pt_sm_absdot(rd, Ku) + ru * fabs(pt_sm_dot(g.e1, Du)) + rv * fabs(pt_sm_dot(g.e2, Du)) + Hr * fabs(pt_sm_dot(g.nh, Du)) +
                         ru * pt_sm_absdot(rd, x1) + rv * pt_sm_absdot(rd, x2) + Hr * pt_sm_absdot(rd, x3) + RHO * tv1 * f2n) * INF + ABS;
    if (un_c + un_r < 0.0) return false;                                                // :109, u >= 0
    // vn = d . (tvec x f1)
    const PtSmV3 Kv = pt_sm_cross(tc, f1), Dv = pt_sm_cross(f1, dc);
    const PtSmV3 y1 = pt_sm_cross(f1, g.e1), y2 = pt_sm_cross(f1, g.e2), y3 = pt_sm_cross(f1, g.nh);
    const double vn_c = pt_sm_dot(dc, Kv);
    const double vn_r = (pt_sm_absdot(rd, Kv) + ru * fabs(pt_sm_dot(g.e1, Dv)) + rv * fabs(pt_sm_dot(g.e2, Dv)) + Hr * fabs(pt_sm_dot(g.nh, Dv)) +
                         ru * pt_sm_absdot(rd, y1) + rv * pt_sm_absdot(rd, y2) + Hr * pt_sm_absdot(rd, y3) + RHO * tv1 * f1n) * INF + ABS;
    if (vn_c + vn_r < 0.0) return false;                                                // :117, v >= 0
    if ((un_c - un_r) + (vn_c - vn_r) > det_hi * 1.000002) return false;                // :117, u + v <= 1
    return true;
}

// a host program may count the builder's work: PT_SM_TALLY(0) per box bounded, PT_SM_TALLY(1 + i) when the plane of the i-th a separates
#ifndef PT_SM_TALLY
#define PT_SM_TALLY(i)
#endif

// the corner of the direction box dc +- rd at which w . d is largest
PT_SM_HD PtSmV3 pt_sm_corner(PtSmV3 dc, PtSmV3 rd, PtSmV3 w)
{
    return pt_sm_v(w.x < 0.0 ? dc.x - rd.x : dc.x + rd.x, w.y < 0.0 ? dc.y - rd.y : dc.y + rd.y, w.z < 0.0 ? dc.z - rd.z : dc.z + rd.z);
}

// true: a plane separates the rays of the box from the inflated triangle j (the derivation: "the separating plane" above)
PT_SM_HD bool pt_sm_sep(const PtSmGeom& g, PtSmV3 oc, double ru, double rv, double Hr, PtSmV3 dc, PtSmV3 rd, const float* tj)
{
    const double INF = 1.001, ABS = 2e-24, RHO = 32.0 * PT_SM_U;
    const PtSmV3 q1 = pt_sm_vf(tj), f1 = pt_sm_vf(tj + 3), f2 = pt_sm_vf(tj + 6);
    const PtSmV3 tc = pt_sm_sub(oc, q1);
    const double f1n = pt_sm_n1(f1), f2n = pt_sm_n1(f2);
    const double tv1 = pt_sm_n1(tc) + ru * pt_sm_n1(g.e1) + rv * pt_sm_n1(g.e2) + 3.0 * Hr;
    const PtSmV3 Kd = pt_sm_cross(f2, f1);
    const double rho_d = RHO * f1n * f2n * INF + ABS, rho_u = RHO * tv1 * f2n * INF + ABS, rho_v = RHO * tv1 * f1n * INF + ABS;
    const double det_lo = pt_sm_dot(dc, Kd) - (pt_sm_absdot(rd, Kd) * INF + rho_d);
    if (!(det_lo > PT_SM_SEP_DET * f1n * f2n)) return false;   // (a NaN: no plane)
    const double eu = rho_u / det_lo, ev = rho_v / det_lo, et = (RHO * tv1 * f1n * f2n * INF + ABS) / det_lo;
    const double es = 2e-6 + (1.000001 * rho_d + rho_u + rho_v) / det_lo;
    const double R = 1.001 * (tv1 + (1.0 + eu + ev + es) * (f1n + f2n));
    // towards the triangle: its centroid from the box's centre, (f1 + f2) / 3 - tc
    const PtSmV3 to = pt_sm_v((f1.x + f2.x) / 3.0 - tc.x, (f1.y + f2.y) / 3.0 - tc.y, (f1.z + f2.z) / 3.0 - tc.z);
    for (int i = 0; i < 6; ++i) {
        const PtSmV3 a = i == 0 ? g.e1 : i == 1 ? g.e2 : i == 2 ? g.nh : i == 3 ? f1 : i == 4 ? f2 : pt_sm_sub(f2, f1);
        PtSmV3 w = pt_sm_cross(a, dc);
        const double sg = pt_sm_dot(w, to) < 0.0 ? -1.0 : 1.0;
        for (int round = 0; round < 3; ++round) {
            w = pt_sm_v(sg * w.x, sg * w.y, sg * w.z);
            if (round < 2) w = pt_sm_cross(a, pt_sm_corner(dc, rd, w));
        }
        const double wdc = pt_sm_dot(w, dc), rdw = pt_sm_absdot(rd, w), mw = wdc + rdw;
        const double mpos = mw <= 0.0 ? 0.0 : mw;   // (a NaN stays one)
        const double lhs = pt_sm_dot(w, tc) + ((ru * fabs(pt_sm_dot(g.e1, w)) + rv * fabs(pt_sm_dot(g.e2, w)) + Hr * fabs(pt_sm_dot(g.nh, w)) +
                                                et * (fabs(wdc) + rdw) + R * mpos) * INF + 1e-13 * pt_sm_n1(w) * R);
        const double w1 = pt_sm_dot(w, f1), w2 = pt_sm_dot(w, f2);
        const double c0 = -eu * w1 - ev * w2, c1 = (1.0 + es + ev) * w1 - ev * w2, c2 = -eu * w1 + (1.0 + es + eu) * w2;
        if (lhs < c0 && lhs < c1 && lhs < c2) { PT_SM_TALLY(1 + i); return true; }
    }
    return false;
}

// true: the ray (o, d) passes triangle j's real forms strictly (binary64; the test is invariant under the length of d)
PT_SM_HD bool pt_sm_witness(PtSmV3 o, PtSmV3 d, const float* tj)
{
    const PtSmV3 q1 = pt_sm_vf(tj), f1 = pt_sm_vf(tj + 3), f2 = pt_sm_vf(tj + 6);
    const PtSmV3 tv = pt_sm_sub(o, q1);
    const double det = pt_sm_dot(d, pt_sm_cross(f2, f1)), un = pt_sm_dot(d, pt_sm_cross(f2, tv)), vn = pt_sm_dot(d, pt_sm_cross(tv, f1));
    const double tn = pt_sm_dot(tv, pt_sm_cross(f1, f2));
    const double m = 1e-6 * det;
    return det > 1e-6 * pt_sm_n1(f1) * pt_sm_n1(f2) && un > m && vn > m && un + vn < det - m && tn > 0.0;
}

// the ranges of a cell in the builder's terms, and one box of them
struct PtSmCell {
    double tu0, tuw, tv0, tvw, qa0, qaw, qb0, qbw;   // the low end and the width of [iu - du, iu + 1 + du], of v's, of the two ratio ranges
    double su, Hr, s;                                // tile units to uu; the plane distance; the sign of d_m
    unsigned m, a, b;                                // the axes of the face
};

// the box at depth `lvl` with the indices (xu, xv, xa, xb), each below 2^lvl, against triangle j: 0 cleared, 1 kept, 2 undecided
PT_SM_HD int pt_sm_box(const PtSmGeom& g, const PtSmCell& c, int lvl, unsigned xu, unsigned xv, unsigned xa, unsigned xb, const float* tj)
{
    const double G = PT_SM_GUARD, sc = 1.0 / (double)(1u << lvl);
    PT_SM_TALLY(0);
    // ---- the directions of the box (each end moved out by 1e-9 of the width: the cuts are formed in binary64)
    const double qaw = c.qaw * sc, qbw = c.qbw * sc;
    const double a0 = c.qa0 + qaw * ((double)xa - 1e-9), a1 = c.qa0 + qaw * ((double)xa + (1.0 + 1e-9));
    const double b0 = c.qb0 + qbw * ((double)xb - 1e-9), b1 = c.qb0 + qbw * ((double)xb + (1.0 + 1e-9));
    const double amin = pt_sm_absmin(a0, a1), amax = pt_sm_absmax(a0, a1), bmin = pt_sm_absmin(b0, b1), bmax = pt_sm_absmax(b0, b1);
    const double l0 = 0.9994 / sqrt(1.0 + amax * amax + bmax * bmax), l1 = 1.0006 / sqrt(1.0 + amin * amin + bmin * bmin);
    const double a_lo = fmin(a0 * l0, a0 * l1), a_hi = fmax(a1 * l0, a1 * l1);
    const double b_lo = fmin(b0 * l0, b0 * l1), b_hi = fmax(b1 * l0, b1 * l1);
    PtSmV3 dc = pt_sm_v(0, 0, 0), rd = pt_sm_v(0, 0, 0);
    pt_sm_set(&dc, c.m, c.s * 0.5 * (l0 + l1)); pt_sm_set(&rd, c.m, 0.5 * (l1 - l0));
    pt_sm_set(&dc, c.a, 0.5 * (a_lo + a_hi)); pt_sm_set(&rd, c.a, 0.5 * (a_hi - a_lo));
    pt_sm_set(&dc, c.b, 0.5 * (b_lo + b_hi)); pt_sm_set(&rd, c.b, 0.5 * (b_hi - b_lo));
    // ---- its origins (the halves of a width are inflated by 1e-9 of it: the cuts are formed in binary64)
    const double tuw = c.tuw * sc, tvw = c.tvw * sc;
    const double uc = (c.tu0 + tuw * ((double)xu + 0.5)) * c.su - G, vc = (c.tv0 + tvw * ((double)xv + 0.5)) * c.su - G;
    const double ru = 0.5 * tuw * c.su * (1.0 + 1e-9), rv = 0.5 * tvw * c.su * (1.0 + 1e-9);
    const PtSmV3 oc = pt_sm_axpy(uc, g.e1, pt_sm_axpy(vc, g.e2, g.p1));
    if (!pt_sm_keep(g, oc, ru, rv, c.Hr, dc, rd, tj)) return 0;
    if (pt_sm_sep(g, oc, ru, rv, c.Hr, dc, rd, tj)) return 0;
    if (pt_sm_witness(oc, dc, tj) || pt_sm_witness(pt_sm_axpy(c.Hr, g.nh, oc), dc, tj) || pt_sm_witness(pt_sm_axpy(-c.Hr, g.nh, oc), dc, tj)) return 1;
    return 2;
}

// the mask of one cell.  tris: ntri records of 16 floats {p1, e1, e2, ...} (PtPrepTriangle); entry: the cell's index as
// pt_sm_classify forms it (k = entry / PT_SM_TRI_ENTRIES < ntri)
PT_SM_HD PtSmMask pt_sm_entry(const float* tris, int ntri, unsigned entry)
{
    const unsigned k = entry / PT_SM_TRI_ENTRIES, within = entry - k * PT_SM_TRI_ENTRIES;
    const unsigned tile = within / PT_SM_DIRS, cell = within - tile * PT_SM_DIRS;
    const unsigned iu = tile / PT_SM_T, iv = tile - iu * PT_SM_T;
    const unsigned face = cell / (PT_SM_C * PT_SM_C), ia = (cell / PT_SM_C) % PT_SM_C, ib = cell % PT_SM_C;
    const float* tk = tris + 16 * k;
    const PtSmGeom g = pt_sm_geom(tk, tk + 3, tk + 6);
    if (!g.valid) return pt_sm_all_ones(ntri);
    PtSmCell c;
    c.su = (1.0 + 2.0 * PT_SM_GUARD) / PT_SM_T; c.Hr = g.H * (1.0 + g.dh);
    c.m = face >> 1; c.a = (c.m + 1u) % 3u; c.b = (c.m + 2u) % 3u;
    c.s = (face & 1u) ? -1.0 : 1.0;
    double qa1, qb1;
    pt_sm_ratio_range((int)ia, &c.qa0, &qa1);
    pt_sm_ratio_range((int)ib, &c.qb0, &qb1);
    c.qaw = qa1 - c.qa0; c.qbw = qb1 - c.qb0;
    // tu_real in [iu - du, iu + 1 + du], tv_real likewise
    c.tu0 = (double)iu - g.du; c.tuw = 1.0 + 2.0 * g.du; c.tv0 = (double)iv - g.dv; c.tvw = 1.0 + 2.0 * g.dv;
    // ONE loop over the boxes of all pairs (cell, j), a box per round: on the device a lane that is done with an easy triangle goes on to
    // its next one while its neighbours still refine theirs.  Per j the walk is depth first ("REFINEMENT" above); the lowest bits of
    // xu, xv, xa, xb are the child counter of the depth
    PtSmMask out = { 0u, 0u };
    unsigned xu = 0u, xv = 0u, xa = 0u, xb = 0u;
    int j = 0, lvl = 0, boxes = 0;
    while (j < ntri) {
        const int r = pt_sm_box(g, c, lvl, xu, xv, xa, xb, tris + 16 * j);
        ++boxes;
        const bool keep = r == 1 || (r == 2 && (lvl >= PT_SM_DEPTH || boxes >= PT_SM_BUDGET));
        bool done = keep;
        if (!keep && r == 2) { ++lvl; xu <<= 1; xv <<= 1; xa <<= 1; xb <<= 1; }   // the first child
        if (r == 0) {
            // cleared: the next sibling, or the parent's when this was the last; the pair is done when the whole cell is cleared
            for (;;) {
                if (lvl == 0) { done = true; break; }
                const unsigned child = (xu & 1u) | ((xv & 1u) << 1) | ((xa & 1u) << 2) | ((xb & 1u) << 3);
                if (child < 15u) {
                    const unsigned n = child + 1u;
                    xu = (xu & ~1u) | (n & 1u); xv = (xv & ~1u) | ((n >> 1) & 1u); xa = (xa & ~1u) | ((n >> 2) & 1u); xb = (xb & ~1u) | ((n >> 3) & 1u);
                    break;
                }
                --lvl; xu >>= 1; xv >>= 1; xa >>= 1; xb >>= 1;
            }
        }
        if (done) {
            if (keep) {
                const int ch = j >> 5;
                const int nc = ntri - 32 * ch < 32 ? ntri - 32 * ch : 32;
                const unsigned bit = 1u << (nc - 1 - (j & 31));
                if (ch == 0) out.x |= bit; else out.y |= bit;
            }
            ++j; lvl = 0; boxes = 0; xu = xv = xa = xb = 0u;
        }
    }
    return out;
}
