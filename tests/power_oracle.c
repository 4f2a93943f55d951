/*
 * power_oracle.c -- the CPU oracle's light choice by power: pt_light_table's table and the three lit estimators with it, in the
 * layouts of pt_render_direct_power and pt_render_indirect_power.  TEST INFRASTRUCTURE.
 *
 * Stated from include/pt_shim.h alone ("light choice by power").  Follows tests/mis_oracle.c in tests/power_oracles.c, so the oracle,
 * the camera and the illumination restatements come as that unit's statics; what it takes from them is the oracle's own operations,
 * odi_fold, odi_clampi, odi_camera and the ODI_R_* / OMI_W_* / OII_END_* codes.
 *   - opw_table: steps 1-6 of the table, sequentially: p_i, pmax, q_i, the uint64 running sum, tri_q;
 *   - opw_light: omi_light's body with step 3b's choice through the cdf and step 3f's inv = total / q_i where (float)nl stood; the MIS
 *     weight (mis != 0) with a = area * inv;
 *   - opw_direct: odi_sample's walk, opw_path: omi_sample's (mis = 0: oii_sample's), the later emissive hit with inv_h = total /
 *     tri_q[h] when counts[h] > 0 and wb = 1 when it is 0.
 * Per light sample the optional account says which entry was chosen, its q and the ODI_R_* reason (OPW_R_EMPTY_TABLE: total == 0).
 * Compiled with oracle/Makefile's flags (tests/power_oracle.py).
 */
enum { OPW_R_EMPTY_TABLE = 8 };   /* beside ODI_R_*: the three uniforms were drawn, the table's total is 0 */
enum { OPW_DIRECT = 0, OPW_INDIRECT = 1, OPW_MIS = 2 };

/* cdf[nl + 1], tri_q[ntri] */
PTOR_CLONES
int opw_table(const void* tris_, int ntri, const void* mats_, int nmat, const int32_t* lights, int nl, uint64_t* cdf, uint32_t* tri_q)
{
    const ptor_triangle* tris = (const ptor_triangle*)tris_;
    const ptor_material* mats = (const ptor_material*)mats_;
    for (int t = 0; t < ntri; ++t) tri_q[t] = 0u;
    cdf[0] = 0u;
    if (ntri == 0) {
        for (int i = 0; i < nl; ++i) cdf[i + 1] = 0u;
        return 0;
    }
    float* pw = (float*)malloc(sizeof(float) * (size_t)(nl > 0 ? nl : 1));
    if (!pw) return -1;
    float pmax = 0.0f;
    for (int i = 0; i < nl; ++i) {
        const ptor_triangle* tj = &tris[odi_clampi(lights[i], ntri)];
        const v3 p1 = v3_make(tj->p1[0], tj->p1[1], tj->p1[2]);
        const v3 e1 = v3_sub(v3_make(tj->p2[0], tj->p2[1], tj->p2[2]), p1);   /* :92-93 */
        const v3 e2 = v3_sub(v3_make(tj->p3[0], tj->p3[1], tj->p3[2]), p1);
        const v3 N = v3_cross(e2, e1);                                         /* :123 */
        const float area = 0.5f * sqrtf(v3_dot(N, N));
        const float* em = mats[odi_clampi((int)tj->id, nmat)].emissive;
        const float p = area * ((em[0] + em[1]) + em[2]);
        pw[i] = (p > 0.0f && p < INFINITY) ? p : 0.0f;
        if (pw[i] > pmax) pmax = pw[i];
    }
    for (int i = 0; i < nl; ++i) {
        uint32_t q = 0u;
        if (pw[i] > 0.0f) {
            q = (uint32_t)((pw[i] / pmax) * 65536.0f);
            if (q < 1u) q = 1u;
        }
        cdf[i + 1] = cdf[i] + q;
        tri_q[odi_clampi(lights[i], ntri)] = q;
    }
    free(pw);
    return 0;
}

/* the table as the estimators read it */
typedef struct opw_tab {
    const uint64_t* cdf;     /* [nl + 1] */
    const uint32_t* tri_q;   /* [ntri] */
} opw_tab;

/* a light sample's account: the entry chosen (-1: none, the table is empty) and its q */
typedef struct opw_pick {
    int32_t entry;
    uint32_t q;
} opw_pick;

/* light sample at the vertex (p, n, wo) of material m.  mis: weigh against the BRDF sample unless `last`.  Returns the reason code */
PTOR_INLINE int opw_light(const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl, const opw_tab* tab,
                          const int32_t* counts, int K, int mis, int last, const ptor_material* m, v3 p, v3 n, v3 wo, uint32_t* seed,
                          v3* c_out, int* wcode, opw_pick* pick, ptor_stats* st)
{
    const v3 albedo = v3_make(m->albedo[0], m->albedo[1], m->albedo[2]);
    const float r0 = ptor_random_float(seed), r1 = ptor_random_float(seed), r2 = ptor_random_float(seed);
    const uint64_t total = tab->cdf[nl];
    *wcode = OMI_W_NONE;
    pick->entry = -1;
    pick->q = 0u;
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
    pick->entry = lo;
    pick->q = (uint32_t)qi;
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
            *wcode = OMI_W_LAST_VERTEX;
        } else if (!(sl > 0.0f)) {
            *wcode = OMI_W_BACK_SIDE;
        } else {
            const float a = area * inv;
            const float pe = d2 / (cl * a);
            const float kp = (float)K * pe;
            w = w * (kp / (kp * (float)counts[j] + pbl));
            *wcode = OMI_W_WEIGHTED;
        }
    }
    *c_out = v3_make((f.x * (mj->emissive[0] * 3.0f)) * w, (f.y * (mj->emissive[1] * 3.0f)) * w, (f.z * (mj->emissive[2] * 3.0f)) * w);
    const ptor_ray s = ptor_get_ray(v3_add(p, v3_scale(wi, 0.01f)), wi);   /* :257 */
    float tl = dist - 0.02f;
    tl = tl < 1e20f ? tl : 1e20f;
    int occluded = 0;
    if (tl > 0.0f) {
        ptor_hit srec;
        for (int i = 0; i < ntri && !occluded; i++) occluded = ptor_intersect_triangle(&s, &tris[i], i, &srec, tl, st);
    }
    return occluded ? ODI_R_OCCLUDED : (tl > 0.0f ? ODI_R_OPEN : ODI_R_OPEN_UNSEARCHED);
}

/* the optional account of a sample's first V vertices: per light sample the entry, its q and the reason; per vertex counts[h] of a
 * later emissive hit of the MIS estimator (-1: none there).  The caller has filled the arrays with "nothing". */
typedef struct opw_why {
    int V;
    int32_t* entry;     /* [V * K] */
    uint32_t* q;        /* [V * K] */
    uint8_t* reason;    /* [V * K] */
    int32_t* later;     /* [V] */
} opw_why;

PTOR_INLINE void opw_tell(const opw_why* why, int i, int K, int k, const opw_pick* pick, int reason)
{
    if (!why || i >= why->V) return;
    why->entry[i * K + k] = pick->entry;
    why->q[i * K + k] = pick->q;
    why->reason[i * K + k] = (uint8_t)reason;
}

/* pt_render_direct_power's sample: odi_sample's walk */
PTOR_INLINE v3 opw_direct(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl,
                          const opw_tab* tab, int x, int grow, int W, int H, int frame, int K, const opw_why* why)
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
        int wcode;
        opw_pick pick;
        const int why_k = opw_light(tris, ntri, mats, lights, nl, tab, 0, K, 0, 1, m, rec.p, n, wo, &seed, &c, &wcode, &pick, &st);
        if (why_k == ODI_R_OPEN || why_k == ODI_R_OPEN_UNSEARCHED) S = v3_add(S, c);
        opw_tell(why, 0, K, k, &pick, why_k);
    }
    const float Kf = (float)K;
    return v3_make(ptor_max(E.x + S.x / Kf, 0.0f), ptor_max(E.y + S.y / Kf, 0.0f), ptor_max(E.z + S.z / Kf, 0.0f));
}

/* pt_render_indirect_power's sample: omi_sample's walk (mis = 0: oii_sample's) */
PTOR_INLINE v3 opw_path(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl,
                        const opw_tab* tab, const int32_t* counts, int mis, int x, int grow, int W, int H, int frame, int K, int B,
                        const opw_why* why)
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
            if (cnt > 0) {
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
            if (why && i < why->V) why->later[i] = cnt;
        }
        const int facing = v3_dot(rec.n, r.dir) < 0.0f;
        const v3 n = facing ? rec.n : v3_scale(rec.n, -1.0f);   /* :243 */
        const v3 wo = v3_neg(r.dir);
        if (nl > 0) {
            v3 S = v3_make(0.0f, 0.0f, 0.0f);
            for (int k = 0; k < K; ++k) {
                v3 c = v3_make(0.0f, 0.0f, 0.0f);
                int wcode;
                opw_pick pick;
                const int why_k = opw_light(tris, ntri, mats, lights, nl, tab, counts, K, mis, i == B - 1, m, rec.p, n, wo, &seed, &c, &wcode,
                                            &pick, &st);
                if (why_k == ODI_R_OPEN || why_k == ODI_R_OPEN_UNSEARCHED) S = v3_add(S, c);
                opw_tell(why, i, K, k, &pick, why_k);
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
    }
    return v3_make(ptor_max(L.x, 0.0f), ptor_max(L.y, 0.0f), ptor_max(L.z, 0.0f));   /* :260 */
}

PTOR_INLINE v3 opw_sample(int mode, const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights,
                          int nl, const opw_tab* tab, const int32_t* counts, int x, int grow, int W, int H, int frame, int K, int B,
                          const opw_why* why)
{
    if (mode == OPW_DIRECT) return opw_direct(cam, tris, ntri, mats, lights, nl, tab, x, grow, W, H, frame, K, why);
    return opw_path(cam, tris, ntri, mats, lights, nl, tab, counts, mode == OPW_MIS, x, grow, W, H, frame, K, B, why);
}

/* omi_render's arguments and layout; mode: OPW_*; cdf, tri_q: the table (opw_table); counts: read by OPW_MIS only */
PTOR_CLONES
int opw_render(int mode, const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const uint64_t* cdf,
               const uint32_t* tri_q, const int32_t* counts, const float* cam10, int W, int H, int stripe_rows, int n_ranks, int rank,
               int frame_begin, int frame_count, int K, int B, float* fb)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    const opw_tab tab = { cdf, tri_q };
    int64_t lp = 0;
    for (int grow = 0; grow < H; ++grow) {
        if ((grow / stripe_rows) % n_ranks != rank) continue;
        for (int x = 0; x < W; ++x, ++lp)
            for (int f = 0; f < frame_count; ++f) {
                const v3 L = opw_sample(mode, &c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, &tab, counts, x,
                                        grow, W, H, frame_begin + f, K, B, 0);
                odi_fold(fb + 4 * lp, L, frame_begin + f);
            }
    }
    return 0;
}

/* n samples (gid[i], frame[i]): radiance[i * 3 ..] = L before the fold; with entry != NULL also, for the first V = (mode == OPW_DIRECT
 * ? 1 : min(B, 8)) vertices: entry[(i * V + v) * K + k] = the list entry light sample k at vertex v chose (-1: not drawn, or the table
 * is empty), q[...] its q (0 where none), reason[...] its ODI_R_* / OPW_R_EMPTY_TABLE code (ODI_R_NOT_DRAWN where not drawn), and
 * later[i * V + v] = counts[h] of the MIS estimator's later emissive hit at vertex v (-1: none) */
PTOR_CLONES
int opw_samples(int mode, const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const uint64_t* cdf,
                const uint32_t* tri_q, const int32_t* counts, const float* cam10, int W, int H, const int32_t* gid, const int32_t* frame,
                int64_t n, int K, int B, float* radiance, int32_t* entry, uint32_t* q, uint8_t* reason, int32_t* later)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    const opw_tab tab = { cdf, tri_q };
    const int V = mode == OPW_DIRECT ? 1 : (B < 8 ? B : 8);
    if (entry) {
        for (int64_t i = 0; i < n * V * K; ++i) entry[i] = -1;
        for (int64_t i = 0; i < n * V * K; ++i) q[i] = 0u;
        memset(reason, ODI_R_NOT_DRAWN, (size_t)(n * V * K));
        for (int64_t i = 0; i < n * V; ++i) later[i] = -1;
    }
    for (int64_t i = 0; i < n; ++i) {
        const opw_why why = { V, entry ? entry + i * V * K : 0, q ? q + i * V * K : 0, reason ? reason + i * V * K : 0, later ? later + i * V : 0 };
        const v3 L = opw_sample(mode, &c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, &tab, counts,
                                gid[i] % W, gid[i] / W, W, H, frame[i], K, B, entry ? &why : 0);
        radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
    }
    return 0;
}
