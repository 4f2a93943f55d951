/*
 * ris_oracle.c -- the CPU oracle's resampled light sampling (RIS): pt_render_direct_ris, pt_render_indirect_ris (mis 0 and 1, with the
 * roulette of pt_render_indirect_rr) in their layouts.  TEST INFRASTRUCTURE.
 *
 * Stated from include/pt_shim.h alone ("resampled light sampling").  Follows tests/roulette_oracle.c in tests/ris_oracles.c, so the
 * oracle, the camera and the illumination restatements come as that unit's statics; what it takes from them is the oracle's own
 * operations, odi_fold, odi_clampi, odi_camera, opw_tab and the ODI_R_* / OMI_W_* / OPW_R_* / OII_END_* / ORR_* codes.
 *   - ors_candidate: opw_light's statements, in their order, up to the shadow ray -- the three uniforms, the choice through the cdf,
 *     the candidate's c with inv = total / q_i and the MIS factor -- without the search: a candidate costs none;
 *   - ors_light: the reservoir of one over M candidates (the extra uniform from the second candidate on, s = the largest channel, wsum,
 *     "kept iff !have or r * wsum < s"), g = (wsum / M) / s_sel, then the parent's shadow search of the kept candidate alone;
 *   - ors_direct: opw_direct's walk, ors_path: orr_path's (the table is required), with ors_light where they take their light sample.
 * Per light sample the optional account says which candidate was kept (-1: none), wsum, s_sel, how many candidates had s > 0, the
 * reason code of the kept one (ORS_R_NONE: none was kept) and its MIS weight code.
 * The identity M = 1 against opw_render / orr_render, bit for bit, pins it to them (tests/test_ris_cpu.py).
 * Compiled with oracle/Makefile's flags (tests/ris_oracle.py).
 */
enum { ORS_R_NONE = 9 };   /* beside ODI_R_* and OPW_R_EMPTY_TABLE: the candidates were drawn, none was kept, no ray was cast */
enum { ORS_MAX_CANDIDATES = 32 };

typedef struct ors_cand {
    v3 c;
    v3 o, wi;   /* the shadow ray's arguments (:257) */
    float tl;
    float s;
    int wcode;
} ors_cand;

/* candidate of the light sample at the vertex (p, n, wo) of material m: ODI_R_OPEN when it contributes (the search has not been made),
 * otherwise the reason it does not */
PTOR_INLINE int ors_candidate(const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl, const opw_tab* tab,
                              const int32_t* counts, int K, int mis, int last, const ptor_material* m, v3 p, v3 n, v3 wo, uint32_t* seed,
                              ors_cand* out)
{
    const v3 albedo = v3_make(m->albedo[0], m->albedo[1], m->albedo[2]);
    const float r0 = ptor_random_float(seed), r1 = ptor_random_float(seed), r2 = ptor_random_float(seed);
    const uint64_t total = tab->cdf[nl];
    out->wcode = OMI_W_NONE;
    if (total == 0u) return OPW_R_EMPTY_TABLE;
    uint32_t u = (uint32_t)(r0 * 16777216.0f);
    if (u > 16777215u) u = 16777215u;
    const uint64_t x = ((uint64_t)u * total) >> 24;
    int lo = 0, hi = nl;   /* cdf[lo] <= x < cdf[hi] */
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (tab->cdf[mid] <= x) lo = mid; else hi = mid;
    }
    const uint64_t qi = tab->cdf[lo + 1] - tab->cdf[lo];
    const float inv = (float)total / (float)qi;
    const int j = odi_clampi(lights[lo], ntri);
    const ptor_triangle* tj = &tris[j];
    const v3 p1 = v3_make(tj->p1[0], tj->p1[1], tj->p1[2]);
    const v3 e1 = v3_sub(v3_make(tj->p2[0], tj->p2[1], tj->p2[2]), p1);   /* :92-93 */
    const v3 e2 = v3_sub(v3_make(tj->p3[0], tj->p3[1], tj->p3[2]), p1);
    const v3 N = v3_cross(e2, e1);                                         /* :123 */
    const v3 nj = v3_normalize(N);
    const float area = 0.5f * sqrtf(v3_dot(N, N));
    const float su = sqrtf(r1), b1 = 1.0f - su, b2 = r2 * su;
    const v3 q = v3_add(v3_add(p1, v3_scale(e1, b1)), v3_scale(e2, b2));
    const v3 dv = v3_sub(q, p);
    const float d2 = v3_dot(dv, dv);
    const float dist = sqrtf(d2);
    const v3 wi = v3_normalize(dv);
    const float sl = v3_dot(wi, nj);
    const float cs = v3_dot(wi, n), cl = fabsf(sl);
    if (!(cs > 0.0f && cl > 0.0f)) return (cs != cs || cl != cl) ? ODI_R_NAN : (cs <= 0.0f ? ODI_R_NOT_FACING : ODI_R_EDGE_ON);
    v3 f;
    float pbl;
    if (m->type == PTOR_DIFFUSE) {
        f = v3_scale(albedo, PTOR_INV_PI);   /* :203 */
        pbl = cs * PTOR_INV_PI;              /* :201 */
    } else if (m->type == PTOR_SPECULAR) {
        const v3 wh = v3_normalize(v3_add(wo, wi));
        const float ct = v3_dot(wh, n);
        const float D = ptor_distribution_ggx(ct, m->roughness);
        pbl = D * ct / (4.0f * v3_dot(wo, wh));   /* :215 */
        if (v3_dot(wi, n) * v3_dot(wo, n) < 0.0f) {   /* :211 */
            f = v3_make(0.0f, 0.0f, 0.0f);
        } else {
            const float g = D / (4.0f * v3_dot(wi, n) * v3_dot(wo, n));
            f = v3_scale(v3_scale(albedo, g), 2.0f);   /* :217 */
        }
    } else {
        return ODI_R_OTHER_TYPE;   /* :220 */
    }
    const ptor_material* mj = &mats[tj->id];
    float w = ((cs * cl) / d2) * (area * inv);
    if (mis) {
        if (last) {
            out->wcode = OMI_W_LAST_VERTEX;
        } else if (!(sl > 0.0f)) {
            out->wcode = OMI_W_BACK_SIDE;
        } else {
            const float a = area * inv;
            const float pe = d2 / (cl * a);
            const float kp = (float)K * pe;
            w = w * (kp / (kp * (float)counts[j] + pbl));
            out->wcode = OMI_W_WEIGHTED;
        }
    }
    out->c = v3_make((f.x * (mj->emissive[0] * 3.0f)) * w, (f.y * (mj->emissive[1] * 3.0f)) * w, (f.z * (mj->emissive[2] * 3.0f)) * w);
    out->o = v3_add(p, v3_scale(wi, 0.01f));   /* :257 */
    out->wi = wi;
    float tl = dist - 0.02f;
    out->tl = tl < 1e20f ? tl : 1e20f;
    return ODI_R_OPEN;
}

/* a light sample's account */
typedef struct ors_pick {
    int32_t kept;      /* the kept candidate's index, -1: none */
    float wsum, ssel;
    int32_t positive;  /* candidates with s > 0 */
    int32_t replaced;  /* times a later candidate replaced a kept one */
    int wcode;         /* OMI_W_* of the kept one */
} ors_pick;

/* light sample with M candidates.  Returns ODI_R_OPEN / _OPEN_UNSEARCHED / _OCCLUDED of the kept candidate's ray (c_out is then its
 * scaled contribution), or ORS_R_NONE */
PTOR_INLINE int ors_light(const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl, const opw_tab* tab,
                          const int32_t* counts, int K, int mis, int last, int M, const ptor_material* m, v3 p, v3 n, v3 wo, uint32_t* seed,
                          v3* c_out, ors_pick* pick, ptor_stats* st)
{
    float wsum = 0.0f;
    int have = 0;
    ors_cand sel;
    memset(&sel, 0, sizeof sel);
    pick->kept = -1;
    pick->positive = pick->replaced = 0;
    pick->wcode = OMI_W_NONE;
    for (int mi = 0; mi < M; ++mi) {
        ors_cand cand;
        memset(&cand, 0, sizeof cand);
        const int why = ors_candidate(tris, ntri, mats, lights, nl, tab, counts, K, mis, last, m, p, n, wo, seed, &cand);
        float r = 0.0f;
        if (mi >= 1) r = ptor_random_float(seed);
        if (why == ODI_R_OPEN) {
            const float s = ptor_max(cand.c.x, ptor_max(cand.c.y, cand.c.z));
            if (s > 0.0f) {
                wsum = wsum + s;
                pick->positive++;
                if (!have || r * wsum < s) {
                    if (have) pick->replaced++;
                    sel = cand;
                    sel.s = s;
                    have = 1;
                    pick->kept = mi;
                }
            }
        }
    }
    pick->wsum = wsum;
    pick->ssel = sel.s;
    if (!have) return ORS_R_NONE;
    pick->wcode = sel.wcode;
    const float g = (wsum / (float)M) / sel.s;
    *c_out = v3_make(sel.c.x * g, sel.c.y * g, sel.c.z * g);
    const ptor_ray sr = ptor_get_ray(sel.o, sel.wi);
    int occluded = 0;
    if (sel.tl > 0.0f) {
        ptor_hit srec;
        for (int i = 0; i < ntri && !occluded; i++) occluded = ptor_intersect_triangle(&sr, &tris[i], i, &srec, sel.tl, st);
    }
    return occluded ? ODI_R_OCCLUDED : (sel.tl > 0.0f ? ODI_R_OPEN : ODI_R_OPEN_UNSEARCHED);
}

/* the optional account of a sample's first V vertices, per light sample; the caller has filled the arrays with "nothing" */
typedef struct ors_why {
    int V;
    int32_t* kept;       /* [V * K] */
    float* wsum;         /* [V * K] */
    float* ssel;         /* [V * K] */
    int32_t* positive;   /* [V * K] */
    int32_t* replaced;   /* [V * K] */
    uint8_t* reason;     /* [V * K] */
    uint8_t* wcode;      /* [V * K] */
} ors_why;

PTOR_INLINE void ors_tell(const ors_why* why, int i, int K, int k, const ors_pick* pick, int reason)
{
    if (!why || i >= why->V) return;
    const int at = i * K + k;
    why->kept[at] = pick->kept;
    why->wsum[at] = pick->wsum;
    why->ssel[at] = pick->ssel;
    why->positive[at] = pick->positive;
    why->replaced[at] = pick->replaced;
    why->reason[at] = (uint8_t)reason;
    why->wcode[at] = (uint8_t)pick->wcode;
}

/* pt_render_direct_ris' sample: opw_direct's walk */
PTOR_INLINE v3 ors_direct(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl,
                          const opw_tab* tab, int x, int grow, int W, int H, int frame, int K, int M, const ors_why* why)
{
    ptor_stats st;
    memset(&st, 0, sizeof st);
    const int gid = grow * W + x;
    uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)frame);
    const ptor_ray r = ocam_generate_ray(cam, x, grow, W, H, &seed);
    ptor_hit rec;
    memset(&rec, 0, sizeof rec);
    if (!ptor_intersect_world(&r, tris, ntri, &rec, &st)) {
        const float bg = ptor_max(0.45f, 0.0f);   /* :235 */
        return v3_make(bg, bg, bg);
    }
    const ptor_material* m = &mats[tris[rec.tri].id];
    const v3 E = v3_make(1.0f * m->emissive[0] * 3.0f, 1.0f * m->emissive[1] * 3.0f, 1.0f * m->emissive[2] * 3.0f);   /* :241 */
    const int facing = v3_dot(rec.n, r.dir) < 0.0f;
    const v3 n = facing ? rec.n : v3_scale(rec.n, -1.0f);   /* :243 */
    const v3 wo = v3_neg(r.dir);
    v3 S = v3_make(0.0f, 0.0f, 0.0f);
    for (int k = 0; k < K && nl > 0; ++k) {
        v3 c = v3_make(0.0f, 0.0f, 0.0f);
        ors_pick pick;
        const int why_k = ors_light(tris, ntri, mats, lights, nl, tab, 0, K, 0, 1, M, m, rec.p, n, wo, &seed, &c, &pick, &st);
        if (why_k == ODI_R_OPEN || why_k == ODI_R_OPEN_UNSEARCHED) S = v3_add(S, c);
        ors_tell(why, 0, K, k, &pick, why_k);
    }
    const float Kf = (float)K;
    return v3_make(ptor_max(E.x + S.x / Kf, 0.0f), ptor_max(E.y + S.y / Kf, 0.0f), ptor_max(E.z + S.z / Kf, 0.0f));
}

/* pt_render_indirect_ris' sample: orr_path's walk with the table */
PTOR_INLINE v3 ors_path(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl,
                        const opw_tab* tab, const int32_t* counts, int mis, int x, int grow, int W, int H, int frame, int K, int B, int R,
                        float cap, int M, const ors_why* why)
{
    ptor_stats st;
    memset(&st, 0, sizeof st);
    const int gid = grow * W + x;
    uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)frame);
    ptor_ray r = ocam_generate_ray(cam, x, grow, W, H, &seed);
    v3 L = v3_make(0.0f, 0.0f, 0.0f);
    v3 mask = v3_make(1.0f, 1.0f, 1.0f);
    const float bg = ptor_max(0.45f, 0.0f);   /* :235 */
    const float Kf = (float)K;
    float pb = 0.0f;
    for (int i = 0; i < B; ++i) {
        ptor_hit rec;
        memset(&rec, 0, sizeof rec);
        if (!ptor_intersect_world(&r, tris, ntri, &rec, &st)) {
            L = v3_add(L, v3_scale(mask, bg));
            break;
        }
        const ptor_triangle* th = &tris[rec.tri];
        const ptor_material* m = &mats[th->id];
        if (i == 0 || nl == 0) {   /* :241 */
            L.x = L.x + mask.x * m->emissive[0] * 3.0f;
            L.y = L.y + mask.y * m->emissive[1] * 3.0f;
            L.z = L.z + mask.z * m->emissive[2] * 3.0f;
        } else if (mis && (m->emissive[0] != 0.0f || m->emissive[1] != 0.0f || m->emissive[2] != 0.0f)) {
            const int cnt = counts[rec.tri];
            float wb = 1.0f;
            if (cnt > 0) {   /* (counts[h] = 0 gives wb = 1 and reads no table) */
                const v3 p1 = v3_make(th->p1[0], th->p1[1], th->p1[2]);
                const v3 e1 = v3_sub(v3_make(th->p2[0], th->p2[1], th->p2[2]), p1);
                const v3 e2 = v3_sub(v3_make(th->p3[0], th->p3[1], th->p3[2]), p1);
                const v3 N = v3_cross(e2, e1);                                     /* :123 */
                const float areah = 0.5f * sqrtf(v3_dot(N, N));
                const float clh = fabsf(v3_dot(r.dir, v3_normalize(N)));
                const float tt = rec.t + 0.01f;
                const float invh = (float)tab->cdf[nl] / (float)tab->tri_q[rec.tri];
                const float pe = (tt * tt) / (clh * (areah * invh));
                wb = pb / ((Kf * pe) * (float)cnt + pb);
            }
            L.x = L.x + ((mask.x * m->emissive[0]) * 3.0f) * wb;
            L.y = L.y + ((mask.y * m->emissive[1]) * 3.0f) * wb;
            L.z = L.z + ((mask.z * m->emissive[2]) * 3.0f) * wb;
        }
        const int facing = v3_dot(rec.n, r.dir) < 0.0f;
        const v3 n = facing ? rec.n : v3_scale(rec.n, -1.0f);   /* :243 */
        const v3 wo = v3_neg(r.dir);
        if (nl > 0) {
            v3 S = v3_make(0.0f, 0.0f, 0.0f);
            for (int k = 0; k < K; ++k) {
                v3 c = v3_make(0.0f, 0.0f, 0.0f);
                ors_pick pick;
                const int why_k = ors_light(tris, ntri, mats, lights, nl, tab, counts, K, mis, i == B - 1, M, m, rec.p, n, wo, &seed, &c, &pick, &st);
                if (why_k == ODI_R_OPEN || why_k == ODI_R_OPEN_UNSEARCHED) S = v3_add(S, c);
                ors_tell(why, i, K, k, &pick, why_k);
            }
            L.x = L.x + mask.x * (S.x / Kf);
            L.y = L.y + mask.y * (S.y / Kf);
            L.z = L.z + mask.z * (S.z / Kf);
        }
        if (i == B - 1) break;   /* the draw cannot be observed */
        v3 wi = v3_make(0.0f, 0.0f, 0.0f);
        float pdf = 0.0f;
        const v3 color = ptor_brdf(wo, &wi, &pdf, n, m, &seed, &st);
        if (pdf <= 0.0f) break;   /* :251 */
        pb = pdf;
        const float d = v3_dot(wi, n);
        mask.x = mask.x * (color.x * d / pdf);
        mask.y = mask.y * (color.y * d / pdf);
        mask.z = mask.z * (color.z * d / pdf);
        r = ptor_get_ray(v3_add(rec.p, v3_scale(wi, 0.01f)), wi);   /* :257 */
        if (i + 1 >= R) {   /* the roulette (i < B - 1 here) */
            const float u = ptor_random_float(&seed);
            const float s = ptor_max(mask.x, ptor_max(mask.y, mask.z));
            const float q = (cap < s) ? cap : s;   /* OpenCL min() */
            if (!(q >= 1.0f)) {
                if (!(u < q)) break;
                mask.x = mask.x / q;
                mask.y = mask.y / q;
                mask.z = mask.z / q;
            }
        }
    }
    return v3_make(ptor_max(L.x, 0.0f), ptor_max(L.y, 0.0f), ptor_max(L.z, 0.0f));   /* :260 */
}

/* indirect: 0 = pt_render_direct_ris (mis, B, R, cap are not read), 1 = pt_render_indirect_ris */
PTOR_INLINE v3 ors_sample(int indirect, const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights,
                          int nl, const opw_tab* tab, const int32_t* counts, int mis, int x, int grow, int W, int H, int frame, int K, int B,
                          int R, float cap, int M, const ors_why* why)
{
    if (!indirect) return ors_direct(cam, tris, ntri, mats, lights, nl, tab, x, grow, W, H, frame, K, M, why);
    return ors_path(cam, tris, ntri, mats, lights, nl, tab, counts, mis, x, grow, W, H, frame, K, B, R, cap, M, why);
}

/* orr_render's layout; M: 1 .. ORS_MAX_CANDIDATES; cdf, tri_q: the table (required when nl > 0) */
PTOR_CLONES
int ors_render(int indirect, int mis, const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const uint64_t* cdf,
               const uint32_t* tri_q, const int32_t* counts, const float* cam10, int W, int H, int stripe_rows, int n_ranks, int rank,
               int frame_begin, int frame_count, int K, int B, int R, float cap, int M, float* fb)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    if (M < 1 || M > ORS_MAX_CANDIDATES || (nl > 0 && !(cdf && tri_q))) return -2;
    const opw_tab tab = { cdf, tri_q };
    int64_t lp = 0;
    for (int grow = 0; grow < H; ++grow) {
        if ((grow / stripe_rows) % n_ranks != rank) continue;
        for (int x = 0; x < W; ++x, ++lp)
            for (int f = 0; f < frame_count; ++f) {
                const v3 L = ors_sample(indirect, &c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, &tab, counts, mis,
                                        x, grow, W, H, frame_begin + f, K, B, R, cap, M, 0);
                odi_fold(fb + 4 * lp, L, frame_begin + f);
            }
    }
    return 0;
}

/* n samples (gid[i], frame[i]): radiance[i * 3 ..] = L before the fold; with kept != NULL also, for the first V = (indirect ? min(B, 8) : 1)
 * vertices and light sample k: kept[(i * V + v) * K + k] = the kept candidate's index (-1: none, or not drawn), wsum, ssel (0 where none),
 * positive = the candidates with s > 0, replaced = how often a later candidate replaced a kept one, reason = ODI_R_OPEN / _OPEN_UNSEARCHED
 * / _OCCLUDED of the kept one's ray, ORS_R_NONE when none was kept, ODI_R_NOT_DRAWN where the light sample was not taken, and wcode = the
 * kept one's OMI_W_* */
PTOR_CLONES
int ors_samples(int indirect, int mis, const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const uint64_t* cdf,
                const uint32_t* tri_q, const int32_t* counts, const float* cam10, int W, int H, const int32_t* gid, const int32_t* frame,
                int64_t n, int K, int B, int R, float cap, int M, float* radiance, int32_t* kept, float* wsum, float* ssel, int32_t* positive,
                int32_t* replaced, uint8_t* reason, uint8_t* wcode)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    if (M < 1 || M > ORS_MAX_CANDIDATES || (nl > 0 && !(cdf && tri_q))) return -2;
    const opw_tab tab = { cdf, tri_q };
    const int V = !indirect ? 1 : (B < 8 ? B : 8);
    const int64_t per = (int64_t)V * K;
    if (kept) {
        for (int64_t i = 0; i < n * per; ++i) {
            kept[i] = -1;
            wsum[i] = ssel[i] = 0.0f;
            positive[i] = replaced[i] = 0;
        }
        memset(reason, ODI_R_NOT_DRAWN, (size_t)(n * per));
        memset(wcode, OMI_W_NONE, (size_t)(n * per));
    }
    for (int64_t i = 0; i < n; ++i) {
        const ors_why why = { V, kept ? kept + i * per : 0, kept ? wsum + i * per : 0, kept ? ssel + i * per : 0, kept ? positive + i * per : 0,
                              kept ? replaced + i * per : 0, kept ? reason + i * per : 0, kept ? wcode + i * per : 0 };
        const v3 L = ors_sample(indirect, &c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, &tab, counts, mis,
                                gid[i] % W, gid[i] / W, W, H, frame[i], K, B, R, cap, M, kept ? &why : 0);
        radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
    }
    return 0;
}
