// secondary_masks_tight_check.cpp -- DENSE containment for the refined builder of csrc/pt_secmask.h (adaptive boxes, the separating plane), on the
// host, outside Python: a stand-alone program (tests/test_secondary_masks_tight_cpu.py builds and runs it; it can be built with
// -fsanitize=address,undefined as it is).
//
//   secondary_masks_tight_check <records.f32> <ntri> <seed> <cells> <rays per cell>
//
// records: ntri prepared records of 16 floats {p1, e1, e2, ...}.  For <cells> entries of the table drawn from the seed, <rays per cell> rays
// are drawn over the cell's preimage: the origin anywhere in the tile and the +-H slab, on the tile's edges and corners and at plane
// distance +H, -H and 0; the direction ratios anywhere in the direction cell, on its edges and grazing the origin triangle; three rays
// of ten with every coordinate at an end.  Every ray is classified by pt_sm_classify and checked against the mask of the cell it LANDS
// in (its own or a neighbour's, computed once): a pair the reference's binary32 test accepts (GenerateColors.cl:96-125 in the oracle's
// operations, the initial tmax) must be in that mask.  Where tests/secondary_masks_check.cpp draws 240 rays at the places the five
// first-order bounds are weakest, this one fills the cell: a plane that cuts a corner off the cell's true set shows only to a ray
// inside that corner.  Prints one line of counters; exit status 0 when nothing is missing.
#include "../oclpathtracer_amd/csrc/pt_secmask.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <unordered_map>
#include <vector>

static float fma32(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

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

int main(int argc, char** argv)
{
    if (argc < 6) { fprintf(stderr, "usage: secondary_masks_tight_check <records.f32> <ntri> <seed> <cells> <rays per cell>\n"); return 2; }
    const int ntri = atoi(argv[2]);
    if (ntri < 1 || ntri > PT_SM_TRI_MAX) { fprintf(stderr, "ntri out of range\n"); return 2; }
    std::vector<float> tris((size_t)ntri * 16);
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f || fread(tris.data(), sizeof(float), tris.size(), f) != tris.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
        fclose(f);
    }
    const unsigned seed = (unsigned)strtoul(argv[3], nullptr, 10);
    const unsigned long ncells = strtoul(argv[4], nullptr, 10), nrays = strtoul(argv[5], nullptr, 10);
    const unsigned total = (unsigned)ntri * PT_SM_TRI_ENTRIES;
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const double G = PT_SM_GUARD, su = (1.0 + 2.0 * G) / PT_SM_T;
    std::unordered_map<unsigned, PtSmMask> cache;
    unsigned long long cells = 0, skipped = 0, rays = 0, own = 0, uncovered = 0, accepted = 0, missing = 0, kept = 0;
    // a fraction of a tile or of a direction cell: mostly anywhere, sometimes an end or just inside one.  `corners` (3 rays of 10) puts
    // every coordinate of the ray at an end: a bound that is linear in a coordinate is weakest at the corners of the box
    bool corners = false;
    auto frac = [&]() {
        const double r = corners ? 0.70 + 0.30 * U(rng) : U(rng);
        return r < 0.70 ? U(rng) : r < 0.78 ? 0.0 : r < 0.86 ? 1.0 : r < 0.93 ? 1e-7 : 1.0 - 1e-7;
    };
    for (unsigned long n = 0; n < ncells; ++n) {
        const unsigned e = (unsigned)(rng() % total);
        const unsigned k = e / PT_SM_TRI_ENTRIES, within = e % PT_SM_TRI_ENTRIES, tile = within / PT_SM_DIRS, cell = within % PT_SM_DIRS;
        const unsigned iu = tile / PT_SM_T, iv = tile % PT_SM_T, face = cell / (PT_SM_C * PT_SM_C), ia = (cell / PT_SM_C) % PT_SM_C, ib = cell % PT_SM_C;
        const float* tk = tris.data() + 16 * k;
        const PtSmGeom g = pt_sm_geom(tk, tk + 3, tk + 6);
        const unsigned m = face >> 1, a = (m + 1) % 3, b = (m + 2) % 3;
        const double s = (face & 1u) ? -1.0 : 1.0;
        const double nhv[3] = { g.nh.x, g.nh.y, g.nh.z };
        unsigned long long landed = 0;
        ++cells;
        for (unsigned long r = 0; r < nrays; ++r) {
            corners = U(rng) < 0.3;
            const double uu = ((double)iu + frac()) * su - G, vv = ((double)iv + frac()) * su - G;
            const double hr = corners ? 0.3 * U(rng) : U(rng), hh = hr < 0.15 ? g.H : hr < 0.30 ? -g.H : hr < 0.40 ? 0.0 : hr < 0.50 ? 0.01 : (2.0 * U(rng) - 1.0) * g.H;
            const float o[3] = { (float)(g.p1.x + uu * g.e1.x + vv * g.e2.x + hh * g.nh.x), (float)(g.p1.y + uu * g.e1.y + vv * g.e2.y + hh * g.nh.y),
                                 (float)(g.p1.z + uu * g.e1.z + vv * g.e2.z + hh * g.nh.z) };
            const double qa = ((double)ia + frac()) * (2.0 / PT_SM_C) - 1.0;
            double qb = ((double)ib + frac()) * (2.0 / PT_SM_C) - 1.0;
            if (U(rng) < 0.15 && nhv[b] != 0.0) {   // grazing the origin triangle, where the cell allows: d . nh = 0 gives qb from qa
                const double q = -(nhv[m] * s + nhv[a] * qa) / nhv[b];
                if (q >= ((double)ib) * (2.0 / PT_SM_C) - 1.0 && q <= ((double)ib + 1.0) * (2.0 / PT_SM_C) - 1.0) qb = q;
            }
            const double len = sqrt(1.0 + qa * qa + qb * qb);
            float d[3];
            d[m] = (float)(s / len); d[a] = (float)(qa / len); d[b] = (float)(qb / len);
            unsigned e2 = 0;
            const bool covered = pt_sm_classify(g.rec.A, g.rec.B, g.rec.N, o[0], o[1], o[2], d[0], d[1], d[2], k, &e2);
            ++rays;
            if (!covered) { ++uncovered; continue; }
            auto it = cache.find(e2);
            if (it == cache.end()) it = cache.emplace(e2, pt_sm_entry(tris.data(), ntri, e2)).first;
            const PtSmMask mk = it->second;
            landed += e2 == e;
            for (int j = 0; j < ntri; ++j) {
                const int ch = j >> 5, nc = ntri - 32 * ch < 32 ? ntri - 32 * ch : 32;
                const bool bit = (((ch ? mk.y : mk.x) >> (nc - 1 - (j & 31))) & 1u) != 0u;
                kept += bit;
                if (!reference_accepts(tris.data() + 16 * j, o, d)) continue;
                ++accepted;
                if (bit) continue;
                if (missing < 5)
                    fprintf(stderr, "MISSING: triangle %d from the mask of entry %u (ray from triangle %u: o = %a %a %a, d = %a %a %a)\n", j, e2, k, o[0],
                            o[1], o[2], d[0], d[1], d[2]);
                ++missing;
            }
        }
        own += landed;
        skipped += landed == 0;
    }
    printf("cells %llu skipped %llu rays %llu own %llu uncovered %llu accepted %llu missing %llu kept %llu T %d C %d\n", cells, skipped, rays, own,
           uncovered, accepted, missing, kept, PT_SM_T, PT_SM_C);
    return missing == 0 ? 0 : 1;
}
