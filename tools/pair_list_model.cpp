// pair_list_model.cpp -- what the masked search's pass 2 (csrc/pt_kernels.hip: pt_intersect_masked) costs in its forms, modelled on the
// host without a GPU from the candidate masks of renderer-like rays.
// build: g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -o pair_list_model tools/pair_list_model.cpp
// usage: pair_list_model <records.f32> <ntri> <seed> <rays> [<rays per wave> [<tail lanes>]]
//
// records and rays: as tools/secmask_candidates.cpp draws them (a point uniform by area, a cosine-distributed direction, the origin moved
// 0.01 along the ray; the ray's mask is its cell's entry of the table, csrc/pt_secmask.h).  Every ray's mask is kept, and the rays fill
// waves of <rays per wave> lanes (61: the lanes a secondary search runs at; the rest of the 64 hold no ray).  Per wave each form of the
// search is walked as the kernel walks it -- own steps while more than <tail lanes> (32) lanes hold a survivor, the list-building loop's
// iterations, the rounds of 64 pairs -- and priced with static instruction counts:
//     own step 56 VALU, round 75, merge 12; a list iteration 13 (a chunk's), 17 (one set, the word chosen per iteration), 16 (helper
//     lanes, the word told by the bit's position) and 14 once per search for the helper lanes' hand-over.  (Prices set before the kernel
//     was written; the shipped helper loop came out at 14 per iteration: profiles/pair_list/steps.txt.)
// Forms:
//   chunks   pt_pass2_chunk per mask word: own steps and an append loop for each
//   one_set  own steps on the low word, ONE loop over what is left of it and the high word
//   helpers  as one_set, the list built by helper lanes: lanes 2k and 2k+1 take a half each of the k-th holder's survivors, the low
//            word's bits at odd positions with the high word's at even ones or the other way round
// One line per form: own steps, list iterations and rounds per search, the modelled VALU per search.  Exit status 0.
#include <cstdio>
#define PT_SM_TALLY(i) ((void)0)
#include "../oclpathtracer_amd/csrc/pt_secmask.h"

#include <cstdlib>
#include <random>
#include <unordered_map>
#include <vector>

struct Tally { unsigned long long own = 0, iters = 0, rounds = 0, handovers = 0; };

static int pc(unsigned m) { return __builtin_popcount(m); }
static unsigned strip(unsigned m) { return m & ~(0x80000000u >> __builtin_clz(m)); }   // the highest bit: the lowest triangle

// own steps of one word while more than `tail` lanes hold a survivor
static void own_steps(std::vector<unsigned>& m, unsigned tail, Tally& t)
{
    for (;;) {
        unsigned more = 0;
        for (unsigned v : m) more += v != 0u;
        if (more <= tail) return;
        ++t.own;
        for (unsigned& v : m) if (v) v = strip(v);
    }
}

// a list-building loop: lane l appends one of its n[l] pairs per iteration; a round as soon as 64 are pending
static void append(const std::vector<int>& n, unsigned& pending, Tally& t)
{
    int longest = 0;
    for (int v : n) longest = v > longest ? v : longest;
    for (int it = 0; it < longest; ++it) {
        ++t.iters;
        for (int v : n) pending += v > it;
        if (pending >= 64u) { ++t.rounds; pending -= 64u; }
    }
}

int main(int argc, char** argv)
{
    if (argc < 5) { fprintf(stderr, "usage: pair_list_model <records.f32> <ntri> <seed> <rays> [<rays per wave> [<tail lanes>]]\n"); return 2; }
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
    const unsigned per_wave = argc > 5 ? (unsigned)strtoul(argv[5], nullptr, 10) : 61u, tail = argc > 6 ? (unsigned)strtoul(argv[6], nullptr, 10) : 32u;
    if (per_wave < 1u || per_wave > 64u) { fprintf(stderr, "rays per wave out of range\n"); return 2; }
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
    std::vector<PtSmMask> masks;
    unsigned long long cand_lo = 0, cand_hi = 0, with_hi = 0;
    for (unsigned long n = 0; n < nrays; ++n) {
        int k, k2;
        const PtSmV3 p = point(&k), p2 = point(&k2);
        const PtSmGeom& g = geom[k];
        const double side = pt_sm_dot(g.nh, pt_sm_sub(p2, p)) < 0.0 ? -1.0 : 1.0;
        const double le = sqrt(pt_sm_dot(g.e1, g.e1));
        const PtSmV3 t1 = pt_sm_v(g.e1.x / le, g.e1.y / le, g.e1.z / le), t2 = pt_sm_cross(g.nh, t1);
        const double r = sqrt(U(rng)), phi = 2.0 * PI * U(rng), cz = sqrt(fmax(0.0, 1.0 - r * r)) * side;
        const double cx = r * cos(phi), cy = r * sin(phi);
        float d[3] = { (float)(cx * t1.x + cy * t2.x + cz * g.nh.x), (float)(cx * t1.y + cy * t2.y + cz * g.nh.y), (float)(cx * t1.z + cy * t2.z + cz * g.nh.z) };
        const float pf[3] = { (float)p.x, (float)p.y, (float)p.z };
        const float o[3] = { pf[0] + 0.01f * d[0], pf[1] + 0.01f * d[1], pf[2] + 0.01f * d[2] };
        unsigned e = 0;
        PtSmMask m = pt_sm_all_ones(ntri);
        if (pt_sm_classify(g.rec.A, g.rec.B, g.rec.N, o[0], o[1], o[2], d[0], d[1], d[2], (unsigned)k, &e)) {
            auto it = cache.find(e);
            if (it == cache.end()) it = cache.emplace(e, pt_sm_entry(tris.data(), ntri, e)).first;
            m = it->second;
        }
        if (ntri <= 32) m.y = 0u;
        masks.push_back(m);
        cand_lo += (unsigned long long)pc(m.x);
        cand_hi += (unsigned long long)pc(m.y);
        with_hi += m.y != 0u;
    }

    Tally chunks, one_set, helpers;
    unsigned long searches = 0, waves_with_hi = 0;
    for (size_t w0 = 0; w0 + per_wave <= masks.size(); w0 += per_wave, ++searches) {
        std::vector<unsigned> lo(64, 0u), hi(64, 0u);
        bool any_hi = false;
        for (unsigned l = 0; l < per_wave; ++l) { lo[l] = masks[w0 + l].x; hi[l] = masks[w0 + l].y; any_hi |= hi[l] != 0u; }
        waves_with_hi += any_hi;
        {   // a chunk per word
            unsigned pending = 0;
            for (int w = 0; w < (ntri > 32 ? 2 : 1); ++w) {
                std::vector<unsigned> m = w ? hi : lo;
                own_steps(m, tail, chunks);
                std::vector<int> n(64);
                for (int l = 0; l < 64; ++l) n[l] = pc(m[l]);
                append(n, pending, chunks);
            }
            chunks.rounds += pending != 0u;
        }
        std::vector<unsigned> left = lo;
        Tally own_only;
        own_steps(left, tail, own_only);
        {   // one survivor set, every lane its own
            unsigned pending = 0;
            one_set.own += own_only.own;
            std::vector<int> n(64);
            for (int l = 0; l < 64; ++l) n[l] = pc(left[l]) + pc(hi[l]);
            append(n, pending, one_set);
            one_set.rounds += pending != 0u;
        }
        {   // helper lanes
            unsigned pending = 0;
            helpers.own += own_only.own;
            std::vector<int> holders;
            for (int l = 0; l < 64; ++l) if (left[l] | hi[l]) holders.push_back(l);
            helpers.handovers += !holders.empty();
            for (size_t first = 0; first < holders.size(); first += 32) {
                std::vector<int> n(64, 0);
                for (int l = 0; l < 64; ++l) {
                    const size_t k = first + (size_t)(l >> 1);
                    if (k >= holders.size()) continue;
                    const unsigned bits = (l & 1) ? 0x55555555u : 0xAAAAAAAAu;
                    n[l] = pc((left[holders[k]] & bits) | (hi[holders[k]] & ~bits));
                }
                append(n, pending, helpers);
            }
            helpers.rounds += pending != 0u;
        }
    }
    const double S = searches ? (double)searches : 1.0;
    printf("rays %lu searches %lu lanes %u tail_lanes %u candidates %.4f low %.4f high %.4f rays_with_high %.4f waves_with_high %.4f\n", nrays, searches,
           per_wave, tail, (double)(cand_lo + cand_hi) / (double)nrays, (double)cand_lo / (double)nrays, (double)cand_hi / (double)nrays,
           (double)with_hi / (double)nrays, (double)waves_with_hi / S);
    struct { const char* name; const Tally* t; double per_iter; } forms[3] = { { "chunks", &chunks, 13.0 }, { "one_set", &one_set, 17.0 }, { "helpers", &helpers, 16.0 } };
    for (auto& f : forms) {
        const double own = (double)f.t->own / S, it = (double)f.t->iters / S, rounds = (double)f.t->rounds / S, hand = (double)f.t->handovers / S;
        printf("form %s own_steps %.4f list_iterations %.4f rounds %.4f valu %.1f\n", f.name, own, it, rounds,
               56.0 * own + f.per_iter * it + 14.0 * hand + 75.0 * rounds + 12.0);
    }
    return 0;
}
