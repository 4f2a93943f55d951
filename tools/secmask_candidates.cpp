// secmask_candidates.cpp -- what the secondary rays' table (csrc/pt_secmask.h) brings pass 2, estimated on the host without a GPU.
// build: g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -o secmask_candidates tools/secmask_candidates.cpp
//        (add -DPT_SM_DEPTH=.., -DPT_SM_BUDGET=.., -DPT_SM_T=.. to try other knobs: the header's #ifndef defaults are the shipped ones)
// usage: secmask_candidates <records.f32> <ntri> <seed> <rays> [<dense cells> [<dense rays per cell>]]
//
// records: ntri prepared records of 16 floats {p1, e1, e2, ...}, the file tests/test_secondary_masks_cpu.py::records writes.
// The rays are drawn as the renderer forms them: a point uniform by area on the scene's triangles, a cosine-distributed unit direction
// about the normal, the origin moved 0.01 along the ray (binary32, GenerateColors.cl:257).  The side of the triangle is the one a second
// area-uniform point of the scene lies on, so a side sees rays in proportion to the scene in front of it.  Each ray is classified by
// pt_sm_classify; its cell's mask comes from pt_sm_entry (computed once per visited cell).  One line of figures is printed:
//   candidates   popcount of the ray's mask, per ray (an uncovered ray counts every triangle)
//   accepted     pairs the reference's binary32 test accepts, per ray
//   union        over the first <dense cells> visited cells, weighted by their rays: the triangles ANY of <dense rays per cell> rays of the
//                cell is accepted by (origins over the whole tile and the whole +-H slab, directions over the whole direction cell): a
//                slight underestimate of the tightest mask the contract allows; `union_table` is the table's popcount over the same cells
//   boxes        boxes bounded per entry computed (pt_sm_box), and how often the plane of each a of pt_sm_sep separated
#include <cstdio>
static unsigned long long g_tally[8];
#define PT_SM_TALLY(i) (++g_tally[i])
#include "../oclpathtracer_amd/csrc/pt_secmask.h"

#include <cstdlib>
#include <random>
#include <unordered_map>
#include <vector>

static float fma32(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// intersectTriangle (:89-135) in the oracle's binary32 operations, without the running tmax
static bool reference_accepts(const float* t, const float o[3], const float d[3])
{
    const float *p1 = t, *e1 = t + 3, *e2 = t + 6;
    const float pvx = fma32(d[1], e2[2], -(d[2] * e2[1])), pvy = fma32(d[2], e2[0], -(d[0] * e2[2])), pvz = fma32(d[0], e2[1], -(d[1] * e2[0]));
    const float det = fma32(e1[2], pvz, fma32(e1[1], pvy, e1[0] * pvx));
    if (det < 1e-8f || -det > 1e-8f) return false;
    const float inv = 1.0f / det;
    const float tx = o[0] - p1[0], ty = o[1] - p1[1], tz = o[2] - p1[2];
    const float u = fma32(tz, pvz, fma32(ty, pvy, tx * pvx)) * inv;
    if (u < 0.0f || u > 1.0f) return false;
    const float qx = fma32(ty, e1[2], -(tz * e1[1])), qy = fma32(tz, e1[0], -(tx * e1[2])), qz = fma32(tx, e1[1], -(ty * e1[0]));
    const float v = fma32(d[2], qz, fma32(d[1], qy, d[0] * qx)) * inv;
    if (v < 0.0f || u + v > 1.0f) return false;
    const float tt = fma32(e2[2], qz, fma32(e2[1], qy, e2[0] * qx)) * inv;
    return tt > 0.0f && tt < 1e20f;
}

static int popcount(PtSmMask m) { return __builtin_popcount(m.x) + __builtin_popcount(m.y); }

int main(int argc, char** argv)
{
    if (argc < 5) { fprintf(stderr, "usage: secmask_candidates <records.f32> <ntri> <seed> <rays> [<dense cells> [<dense rays per cell>]]\n"); return 2; }
    const int ntri = atoi(argv[2]);
    if (ntri < 1 || ntri > PT_SM_TRI_MAX) { fprintf(stderr, "ntri out of range\n"); return 2; }
    std::vector<float> tris((size_t)ntri * 16);
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f || fread(tris.data(), sizeof(float), tris.size(), f) != tris.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        fclose(f);
    }
    const unsigned seed = (unsigned)strtoul(argv[3], nullptr, 10);
    const unsigned long nrays = strtoul(argv[4], nullptr, 10);
    const unsigned long dense_cells = argc > 5 ? strtoul(argv[5], nullptr, 10) : 0ul, dense_rays = argc > 6 ? strtoul(argv[6], nullptr, 10) : 2000ul;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double PI = 3.14159265358979323846;

    std::vector<PtSmGeom> geom;
    std::vector<double> cdf;
    double area = 0.0;
    for (int k = 0; k < ntri; ++k) {
        geom.push_back(pt_sm_geom(&tris[16 * k], &tris[16 * k + 3], &tris[16 * k + 6]));
        const PtSmV3 n = pt_sm_cross(geom[k].e1, geom[k].e2);
        area += 0.5 * sqrt(pt_sm_dot(n, n));
        cdf.push_back(area);
    }
    auto point = [&](int* k) {   // area-uniform
        const double r = U(rng) * area;
        int i = 0;
        while (i < ntri - 1 && cdf[i] < r) ++i;
        double a = U(rng), b = U(rng);
        if (a + b > 1.0) { a = 1.0 - a; b = 1.0 - b; }
        *k = i;
        return pt_sm_axpy(a, geom[i].e1, pt_sm_axpy(b, geom[i].e2, geom[i].p1));
    };

    std::unordered_map<unsigned, PtSmMask> cache;
    std::vector<unsigned> order;                       // the visited cells in the order met
    std::unordered_map<unsigned, unsigned long> hits;  // rays per visited cell
    unsigned long long cand = 0, acc = 0, uncovered = 0;
    const unsigned long long boxes_before = g_tally[0];
    for (unsigned long n = 0; n < nrays; ++n) {
        int k, k2;
        const PtSmV3 p = point(&k), p2 = point(&k2);
        const PtSmGeom& g = geom[k];
        const double side = pt_sm_dot(g.nh, pt_sm_sub(p2, p)) < 0.0 ? -1.0 : 1.0;
        // a cosine-distributed direction about side * nh, in the frame (e1 / |e1|, nh x that, nh)
        const double le = sqrt(pt_sm_dot(g.e1, g.e1));
        const PtSmV3 t1 = pt_sm_v(g.e1.x / le, g.e1.y / le, g.e1.z / le), t2 = pt_sm_cross(g.nh, t1);
        const double r = sqrt(U(rng)), phi = 2.0 * PI * U(rng), cz = sqrt(fmax(0.0, 1.0 - r * r)) * side;
        const double cx = r * cos(phi), cy = r * sin(phi);
        float d[3] = { (float)(cx * t1.x + cy * t2.x + cz * g.nh.x), (float)(cx * t1.y + cy * t2.y + cz * g.nh.y), (float)(cx * t1.z + cy * t2.z + cz * g.nh.z) };
        const float pf[3] = { (float)p.x, (float)p.y, (float)p.z };
        const float o[3] = { pf[0] + 0.01f * d[0], pf[1] + 0.01f * d[1], pf[2] + 0.01f * d[2] };
        unsigned e = 0;
        const bool covered = pt_sm_classify(g.rec.A, g.rec.B, g.rec.N, o[0], o[1], o[2], d[0], d[1], d[2], (unsigned)k, &e);
        PtSmMask m = pt_sm_all_ones(ntri);
        if (covered) {
            auto it = cache.find(e);
            if (it == cache.end()) { it = cache.emplace(e, pt_sm_entry(tris.data(), ntri, e)).first; order.push_back(e); }
            m = it->second;
            hits[e]++;
        }
        uncovered += !covered;
        cand += (unsigned long long)popcount(m);
        for (int j = 0; j < ntri; ++j) acc += reference_accepts(&tris[16 * j], o, d);
    }
    const unsigned long long boxes = g_tally[0] - boxes_before;

    // ---- the dense-sample union of the first visited cells
    double un_sum = 0.0, tab_sum = 0.0, w_sum = 0.0;
    unsigned long long outside = 0;
    const double G = PT_SM_GUARD, su = (1.0 + 2.0 * G) / PT_SM_T;
    for (unsigned long ci = 0; ci < dense_cells && ci < order.size(); ++ci) {
        const unsigned e = order[ci];
        const unsigned k = e / PT_SM_TRI_ENTRIES, within = e % PT_SM_TRI_ENTRIES, tile = within / PT_SM_DIRS, cell = within % PT_SM_DIRS;
        const unsigned iu = tile / PT_SM_T, iv = tile % PT_SM_T, face = cell / (PT_SM_C * PT_SM_C), ia = (cell / PT_SM_C) % PT_SM_C, ib = cell % PT_SM_C;
        const PtSmGeom& g = geom[k];
        const unsigned m = face >> 1, a = (m + 1) % 3, b = (m + 2) % 3;
        const double s = (face & 1u) ? -1.0 : 1.0;
        PtSmMask un = { 0u, 0u };
        for (unsigned long n = 0; n < dense_rays; ++n) {
            const double uu = ((double)iu + U(rng)) * su - G, vv = ((double)iv + U(rng)) * su - G, hh = (2.0 * U(rng) - 1.0) * g.H;
            const float o[3] = { (float)(g.p1.x + uu * g.e1.x + vv * g.e2.x + hh * g.nh.x), (float)(g.p1.y + uu * g.e1.y + vv * g.e2.y + hh * g.nh.y),
                                 (float)(g.p1.z + uu * g.e1.z + vv * g.e2.z + hh * g.nh.z) };
            const double qa = ((double)ia + U(rng)) * (2.0 / PT_SM_C) - 1.0, qb = ((double)ib + U(rng)) * (2.0 / PT_SM_C) - 1.0;
            const double len = sqrt(1.0 + qa * qa + qb * qb);
            float d[3];
            d[m] = (float)(s / len); d[a] = (float)(qa / len); d[b] = (float)(qb / len);
            unsigned e2 = 0;
            if (!pt_sm_classify(g.rec.A, g.rec.B, g.rec.N, o[0], o[1], o[2], d[0], d[1], d[2], k, &e2) || e2 != e) continue;
            for (int j = 0; j < ntri; ++j)
                if (reference_accepts(&tris[16 * j], o, d)) {
                    const int ch = j >> 5, nc = ntri - 32 * ch < 32 ? ntri - 32 * ch : 32;
                    const unsigned bit = 1u << (nc - 1 - (j & 31));
                    if (ch == 0) un.x |= bit; else un.y |= bit;
                }
        }
        const PtSmMask tab = cache[e];
        outside += (unsigned long long)popcount(PtSmMask{ un.x & ~tab.x, un.y & ~tab.y });
        const double w = (double)hits[e];
        un_sum += w * popcount(un); tab_sum += w * popcount(tab); w_sum += w;
    }
    printf("rays %lu uncovered %llu candidates %.4f accepted %.4f cells %zu boxes %.1f", nrays, uncovered, (double)cand / (double)nrays,
           (double)acc / (double)nrays, order.size(), order.empty() ? 0.0 : (double)boxes / (double)order.size());
    if (w_sum > 0.0) printf(" union %.4f union_table %.4f outside %llu", un_sum / w_sum, tab_sum / w_sum, outside);
    printf(" planes");
    for (int i = 1; i <= 6; ++i) printf(" %llu", g_tally[i]);
    printf(" T %d C %d depth %d budget %d\n", PT_SM_T, PT_SM_C, PT_SM_DEPTH, PT_SM_BUDGET);
    return outside == 0 ? 0 : 1;
}
