// secondary_masks_check.cpp -- the host build of csrc/pt_secmask.h against the reference's own test, without a GPU and outside Python:
// a stand-alone program (tests/test_secondary_masks_cpu.py builds and runs it; it can be built under the sanitizers as it is).
//
//   secondary_masks_check check  <records.f32> <ntri> <seed> <cells>     sample cells, draw rays inside them, test the contract
//   secondary_masks_check table  <records.f32> <ntri> <out.u32> <stride> [<first> <count>]   entries first, first + stride, .. (count of them; default: from
//                                                                          0 to the table's end) of the table pt_secondary_mask_snapshot returns
//   secondary_masks_check valid  <records.f32> <ntri>                     how many triangles have no table (pt_sm_geom): a scene with one declines
//   secondary_masks_check rays   <records.f32> <ntri> <seed> <cells> <table.u32>   the check's rays against a whole table from elsewhere
//
// records: ntri prepared records of 16 floats {p1, e1, e2, ...} (e1 = fl(p2 - p1), e2 = fl(p3 - p1): what the prep kernel stores).
// CONTRACT (pt_secmask.h): a pair (ray, triangle) the reference accepts -- GenerateColors.cl:96-125 against the initial tmax, restated
// below in the oracle's binary32 operations -- is never missing from the mask of the cell pt_sm_classify maps the ray to.  A ray it
// declares uncovered is only counted: the trace kernel searches it with every triangle (pt_trace_body: "if (covered) pm = v"), which
// the GPU parity cases exercise, not this program.  Prints one line of counters; exit status 0 when nothing is missing.
#include "../oclpathtracer_amd/csrc/pt_secmask.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <unordered_map>
#include <vector>

static float fma32(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// intersectTriangle (:89-135) as oracle/pt_oracle.c evaluates it, without the running tmax
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

struct Counters { unsigned long long cells, skipped, rays, uncovered, accepted, missing, kept; };

struct Checker {
    const float* tris;
    int ntri;
    const PtSmMask* table;   // null: entries are computed on demand
    std::unordered_map<unsigned, PtSmMask> cache;
    Counters c;

    PtSmMask entry(unsigned e)
    {
        if (table) return table[e];
        auto it = cache.find(e);
        if (it != cache.end()) return it->second;
        const PtSmMask m = pt_sm_entry(tris, ntri, e);
        cache.emplace(e, m);
        return m;
    }

    // one ray leaving triangle k; returns true when it is covered and maps to cell `want`
    bool ray(unsigned k, const PtSmTri& rec, const float o[3], const float d[3], unsigned want)
    {
        unsigned e = 0;
        const bool covered = pt_sm_classify(rec.A, rec.B, rec.N, o[0], o[1], o[2], d[0], d[1], d[2], k, &e);
        const PtSmMask m = covered ? entry(e) : pt_sm_all_ones(ntri);
        c.rays++;
        c.uncovered += !covered;
        for (int j = 0; j < ntri; ++j) {
            const int ch = j >> 5, nc = ntri - 32 * ch < 32 ? ntri - 32 * ch : 32;
            const bool bit = (((ch ? m.y : m.x) >> (nc - 1 - (j & 31))) & 1u) != 0u;
            c.kept += bit;
            if (reference_accepts(tris + 16 * j, o, d)) {
                c.accepted++;
                if (!bit) {
                    if (c.missing < 5)
                        fprintf(stderr, "MISSING: triangle %d from the mask of entry %u (ray from triangle %u: o = %a %a %a, d = %a %a %a)\n", j, e, k,
                                o[0], o[1], o[2], d[0], d[1], d[2]);
                    c.missing++;
                }
            }
        }
        return covered && e == want;
    }
};

int main(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "usage: see the head of secondary_masks_check.cpp\n"); return 2; }
    const char* mode = argv[1];
    const int ntri = atoi(argv[3]);
    if (ntri < 1 || ntri > PT_SM_TRI_MAX) { fprintf(stderr, "ntri out of range\n"); return 2; }
    std::vector<float> tris((size_t)ntri * 16);
    {
        FILE* f = fopen(argv[2], "rb");
        if (!f || fread(tris.data(), sizeof(float), tris.size(), f) != tris.size()) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        fclose(f);
    }
    const unsigned total = (unsigned)ntri * PT_SM_TRI_ENTRIES;
    if (!strcmp(mode, "valid")) {
        int invalid = 0;
        for (int k = 0; k < ntri; ++k) invalid += !pt_sm_geom(&tris[16 * k], &tris[16 * k + 3], &tris[16 * k + 6]).valid;
        printf("invalid %d of %d\n", invalid, ntri);
        return 0;
    }
    if (!strcmp(mode, "table")) {
        if (argc < 6) return 2;
        const unsigned stride = (unsigned)strtoul(argv[5], nullptr, 10);
        if (stride == 0) return 2;
        std::vector<PtSmMask> out;
        const unsigned first = argc > 6 ? (unsigned)strtoul(argv[6], nullptr, 10) : 0u;
        const unsigned count = argc > 7 ? (unsigned)strtoul(argv[7], nullptr, 10) : ~0u;
        for (unsigned e = first, n = 0; e < total && n < count; e += stride, ++n) out.push_back(pt_sm_entry(tris.data(), ntri, e));
        FILE* f = fopen(argv[4], "wb");
        if (!f || fwrite(out.data(), sizeof(PtSmMask), out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[4]); return 2; }
        fclose(f);
        printf("entries %u of %u T %d C %d\n", (unsigned)out.size(), total, PT_SM_T, PT_SM_C);
        return 0;
    }
    if (argc < 6) return 2;
    const unsigned seed = (unsigned)strtoul(argv[4], nullptr, 10);
    const unsigned ncells = (unsigned)strtoul(argv[5], nullptr, 10);
    std::vector<PtSmMask> given;
    if (!strcmp(mode, "rays")) {
        if (argc < 7) return 2;
        given.resize(total);
        FILE* f = fopen(argv[6], "rb");
        if (!f || fread(given.data(), sizeof(PtSmMask), given.size(), f) != given.size()) { fprintf(stderr, "cannot read %s\n", argv[6]); return 2; }
        fclose(f);
    }
    Checker ck = { tris.data(), ntri, given.empty() ? nullptr : given.data(), {}, {} };
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double G = PT_SM_GUARD, su = (1.0 + 2.0 * G) / PT_SM_T;
    // the fractions of a tile / a direction cell the draws take: corners and edges, just inside them, the middle, random ones
    const double edge[6] = { 0.0, 1.0, 1e-9, 1.0 - 1e-9, 0.5, -1.0 };
    for (unsigned n = 0; n < ncells; ++n) {
        const unsigned e = (unsigned)(rng() % total);
        const unsigned k = e / PT_SM_TRI_ENTRIES, within = e % PT_SM_TRI_ENTRIES, tile = within / PT_SM_DIRS, cell = within % PT_SM_DIRS;
        const unsigned iu = tile / PT_SM_T, iv = tile % PT_SM_T, face = cell / (PT_SM_C * PT_SM_C), ia = (cell / PT_SM_C) % PT_SM_C, ib = cell % PT_SM_C;
        const float* tk = tris.data() + 16 * k;
        const PtSmGeom g = pt_sm_geom(tk, tk + 3, tk + 6);
        ck.c.cells++;
        bool any = false;
        const unsigned m = face >> 1, a = (m + 1) % 3, b = (m + 2) % 3;
        const double s = (face & 1u) ? -1.0 : 1.0;
        const double nh[3] = { g.nh.x, g.nh.y, g.nh.z };
        for (int draw = 0; draw < 48; ++draw) {
            // ---- the origin: a point of the tile (corners, edges, inside), at plane distance +-H, 0 or between
            const double fu = edge[draw % 6] < 0 ? U(rng) : edge[draw % 6], fv = edge[(draw / 6) % 6] < 0 ? U(rng) : edge[(draw / 6) % 6];
            const double uu = ((double)iu + fu) * su - G, vv = ((double)iv + fv) * su - G;
            const int hk = draw % 5;
            const double hh = hk == 0 ? g.H : hk == 1 ? -g.H : hk == 2 ? 0.0 : hk == 3 ? 0.01 : (2.0 * U(rng) - 1.0) * g.H;
            float o[3];
            o[0] = (float)(g.p1.x + uu * g.e1.x + vv * g.e2.x + hh * g.nh.x);
            o[1] = (float)(g.p1.y + uu * g.e1.y + vv * g.e2.y + hh * g.nh.y);
            o[2] = (float)(g.p1.z + uu * g.e1.z + vv * g.e2.z + hh * g.nh.z);
            // ---- the direction: ratios on the cell's boundary, inside it, and grazing the origin triangle where the cell allows
            const int da = (draw / 2) % 6, db = (draw / 12) % 6;
            double qa = ((double)ia + (edge[da] < 0 ? U(rng) : edge[da])) * (2.0 / PT_SM_C) - 1.0;
            double qb = ((double)ib + (edge[db] < 0 ? U(rng) : edge[db])) * (2.0 / PT_SM_C) - 1.0;
            if (draw % 4 == 3 && nh[b] != 0.0) {   // d . nh = 0: qb from qa
                const double q = -(nh[m] * s + nh[a] * qa) / nh[b];
                if (q >= ((double)ib) * (2.0 / PT_SM_C) - 1.0 && q <= ((double)ib + 1.0) * (2.0 / PT_SM_C) - 1.0) qb = q;
            }
            const double len = sqrt(1.0 + qa * qa + qb * qb);
            float d[3];
            d[m] = (float)(s / len); d[a] = (float)(qa / len); d[b] = (float)(qb / len);
            any |= ck.ray(k, g.rec, o, d, e);
            // one ulp to either side, in either ratio
            for (int side = 0; side < 4; ++side) {
                float d2[3] = { d[0], d[1], d[2] };
                const unsigned ax = side < 2 ? a : b;
                d2[ax] = nextafterf(d2[ax], (side & 1) ? 2.0f : -2.0f);
                any |= ck.ray(k, g.rec, o, d2, e);
            }
        }
        if (!any) ck.c.skipped++;
    }
    const Counters& c = ck.c;
    printf("cells %llu skipped %llu rays %llu uncovered %llu accepted %llu missing %llu kept %llu T %d C %d\n", c.cells, c.skipped, c.rays,
           c.uncovered, c.accepted, c.missing, c.kept, PT_SM_T, PT_SM_C);
    return c.missing == 0 ? 0 : 1;
}
