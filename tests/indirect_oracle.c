/*
 * indirect_oracle.c -- the CPU oracle's path tracing with light sampling at every vertex, in the layout of pt_render_indirect.
 * TEST INFRASTRUCTURE.
 *
 * Follows tests/direct_oracle.c in tests/oracles.c (oracle/pt_oracle.c, the camera restatement and direct
 * illumination's come as that unit's statics) and composes the estimator of pt_render_indirect (include/pt_shim.h)
 * from the oracle's own operations, in the order the contract states them:
 *   - the sample of pixel gid in frame z: seed = gid + hash(z), ocam_generate_ray (GenerateColors.cl:263-288, :308), L = 0,
 *     mask = 1;
 *   - for i = 0 .. B-1 the closest hit by ptor_intersect_world (:137-154); a miss adds mask * max(0.45, 0) (:235) and ends the path;
 *   - on a hit, ptor_trace_rays's statements (pt_oracle.c:462-482) with one insertion and one condition: the emission (:241) is
 *     added when i == 0 or there are no lights; with lights, S = the K light samples of odi_sample's loop (oii_light below is that
 *     loop's body, statement for statement, at the vertex (p, n, wo, m)), then L += mask * (S / K); then ptor_brdf (:195-221) on the
 *     same seed, pdf <= 0 ends the path (:251), mask *= color * dot(wi, n) / pdf, the next ray ptor_get_ray(p + wi 0.01, wi) (:257).
 *     At i == B-1 the BRDF draw cannot be observed and is skipped;
 *   - L = max(L, 0) (:260), folded by odi_fold.
 * Two identities pin this to the statements it repeats (tests/test_indirect_cpu.py): with no lights the image is ptor_render's at
 * the same depth, and at B = 1 it is odi_render's, both bit for bit.
 * oii_details reports, from that same walk, what happened at each of a path's first vertices (tests/test_indirect_cpu.py proves with
 * it that each input of tests/test_gpu_indirect_edges.py reaches the edge it is rendered for).
 * Compiled with oracle/Makefile's flags (tests/oracles.py).
 */
enum { OII_END_MISS = 0, OII_END_PDF = 1, OII_END_DEPTH = 2 };

/* what oii_sample says about a path beside its radiance */
typedef struct oii_info {
    int vertices;         /* closest hits: the vertices the path reached, 0 .. B */
    int end;              /* OII_END_* */
    int end_at;           /* the loop index i at which the path ended: the search that missed, the vertex whose pdf <= 0, or B - 1 */
    int later_open;       /* light samples at a vertex >= 2 (i >= 1) whose shadow ray was open ... */
    int later_occluded;   /* ... and occluded */
} oii_info;

/* oii_sample's optional account of the first V vertices of a path (oii_details): per vertex the hit's material type (0 = the path
 * has no such vertex) and index, whether the normal was negated at :243, whether the hit triangle's material is emissive, and the
 * ODI_R_* reason code of each of its K light samples (ODI_R_NOT_DRAWN where none was drawn).  The caller clears the arrays. */
typedef struct oii_why {
    int V;
    uint8_t* mtype;      /* [V] */
    int32_t* material;   /* [V] */
    uint8_t* flipped;    /* [V] */
    uint8_t* emissive;   /* [V] */
    uint8_t* reason;     /* [V * K] */
} oii_why;

/* light sample at the vertex (p, n, wo) of material m: odi_sample's loop body.  Returns its ODI_R_* reason code (direct_oracle.c):
 * NOT_FACING, EDGE_ON, NAN and OTHER_TYPE contribute nothing (the three uniforms are drawn all the same), OCCLUDED neither;
 * OPEN_UNSEARCHED (tl <= 0: nothing is searched) and OPEN contribute *c */
PTOR_INLINE int oii_light(const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl,
                          const ptor_material* m, v3 p, v3 n, v3 wo, uint32_t* seed, v3* c_out, ptor_stats* st)
{
    const v3 albedo = v3_make(m->albedo[0], m->albedo[1], m->albedo[2]);
    const float r0 = ptor_random_float(seed), r1 = ptor_random_float(seed), r2 = ptor_random_float(seed);
    uint32_t li = (uint32_t)(r0 * (float)nl);
    if (li > (uint32_t)nl - 1u) li = (uint32_t)nl - 1u;
    const int j = odi_clampi(lights[li], ntri);
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
    const float cs = v3_dot(wi, n), cl = fabsf(v3_dot(wi, nj));
    if (!(cs > 0.0f && cl > 0.0f)) return (cs != cs || cl != cl) ? ODI_R_NAN : (cs <= 0.0f ? ODI_R_NOT_FACING : ODI_R_EDGE_ON);
    v3 f;
    if (m->type == PTOR_DIFFUSE) {
        f = v3_scale(albedo, PTOR_INV_PI);   /* :203 */
    } else if (m->type == PTOR_SPECULAR) {
        const v3 wh = v3_normalize(v3_add(wo, wi));
        const float ct = v3_dot(wh, n);
        const float D = ptor_distribution_ggx(ct, m->roughness);
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
    const float w = ((cs * cl) / d2) * (area * (float)nl);
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

/* one sample: its radiance L before the fold; info and why (each may be NULL) are accounts of the same walk */
PTOR_INLINE v3 oii_sample(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights,
                          int nl, int x, int grow, int W, int H, int frame, int K, int B, oii_info* info, const oii_why* why)
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
    oii_info acc = { 0, OII_END_DEPTH, B - 1, 0, 0 };
    for (int i = 0; i < B; ++i) {
        ptor_hit rec;
        memset(&rec, 0, sizeof rec);
        if (!ptor_intersect_world(&r, tris, ntri, &rec, &st)) {
            L = v3_add(L, v3_scale(mask, bg));
            acc.end = OII_END_MISS;
            acc.end_at = i;
            break;
        }
        acc.vertices++;
        const ptor_material* m = &mats[tris[rec.tri].id];
        if (i == 0 || nl == 0) {   /* :241 */
            L.x = L.x + mask.x * m->emissive[0] * 3.0f;
            L.y = L.y + mask.y * m->emissive[1] * 3.0f;
            L.z = L.z + mask.z * m->emissive[2] * 3.0f;
        }
        const int facing = v3_dot(rec.n, r.dir) < 0.0f;
        const v3 n = facing ? rec.n : v3_scale(rec.n, -1.0f);   /* :243 */
        const v3 wo = v3_neg(r.dir);
        const int told = why && i < why->V;
        if (told) {
            why->mtype[i] = (uint8_t)m->type;
            why->material[i] = (int32_t)tris[rec.tri].id;
            why->flipped[i] = (uint8_t)!facing;
            why->emissive[i] = (uint8_t)(m->emissive[0] > 0.0f || m->emissive[1] > 0.0f || m->emissive[2] > 0.0f);
        }
        if (nl > 0) {
            v3 S = v3_make(0.0f, 0.0f, 0.0f);
            for (int k = 0; k < K; ++k) {
                v3 c = v3_make(0.0f, 0.0f, 0.0f);
                const int why_k = oii_light(tris, ntri, mats, lights, nl, m, rec.p, n, wo, &seed, &c, &st);
                const int open = why_k == ODI_R_OPEN || why_k == ODI_R_OPEN_UNSEARCHED;
                if (open) S = v3_add(S, c);
                if (i >= 1 && open) acc.later_open++;
                if (i >= 1 && why_k == ODI_R_OCCLUDED) acc.later_occluded++;
                if (told) why->reason[i * K + k] = (uint8_t)why_k;
            }
            L.x = L.x + mask.x * (S.x / Kf);
            L.y = L.y + mask.y * (S.y / Kf);
            L.z = L.z + mask.z * (S.z / Kf);
        }
        if (i == B - 1) break;   /* the draw cannot be observed */
        v3 wi = v3_make(0.0f, 0.0f, 0.0f);
        float pdf = 0.0f;
        const v3 color = ptor_brdf(wo, &wi, &pdf, n, m, &seed, &st);
        if (pdf <= 0.0f) {   /* :251 */
            acc.end = OII_END_PDF;
            acc.end_at = i;
            break;
        }
        const float d = v3_dot(wi, n);
        mask.x = mask.x * (color.x * d / pdf);
        mask.y = mask.y * (color.y * d / pdf);
        mask.z = mask.z * (color.z * d / pdf);
        r = ptor_get_ray(v3_add(rec.p, v3_scale(wi, 0.01f)), wi);   /* :257 */
    }
    if (info) *info = acc;
    return v3_make(ptor_max(L.x, 0.0f), ptor_max(L.y, 0.0f), ptor_max(L.z, 0.0f));   /* :260 */
}

/* fb[local pixel][4]: frames [frame_begin, frame_begin + frame_count) folded in ascending order into what fb holds (frame 0 starts
 * afresh), in the stripe layout of pt_render_params; cam10 as for odi_render.  Returns -1 for a camera ocam_derive rejects. */
PTOR_CLONES
int oii_render(const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const float* cam10, int W, int H,
               int stripe_rows, int n_ranks, int rank, int frame_begin, int frame_count, int K, int B, float* fb)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    int64_t lp = 0;
    for (int grow = 0; grow < H; ++grow) {
        if ((grow / stripe_rows) % n_ranks != rank) continue;
        for (int x = 0; x < W; ++x, ++lp)
            for (int f = 0; f < frame_count; ++f) {
                const v3 L = oii_sample(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, x, grow, W, H,
                                        frame_begin + f, K, B, 0, 0);
                odi_fold(fb + 4 * lp, L, frame_begin + f);
            }
    }
    return 0;
}

/* n samples (gid[i], frame[i]): radiance[i * 3 ..] = L before the fold, vertices[i], end[i] = OII_END_*, later[i * 2 ..] = the
 * light samples at vertices >= 2 whose shadow ray was {open, occluded} */
PTOR_CLONES
int oii_samples(const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const float* cam10, int W, int H,
                const int32_t* gid, const int32_t* frame, int64_t n, int K, int B, float* radiance, int32_t* vertices, uint8_t* end,
                int32_t* later)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    for (int64_t i = 0; i < n; ++i) {
        oii_info info;
        const v3 L = oii_sample(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, gid[i] % W, gid[i] / W,
                                W, H, frame[i], K, B, &info, 0);
        radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
        vertices[i] = info.vertices;
        end[i] = (uint8_t)info.end;
        later[2 * i] = info.later_open;
        later[2 * i + 1] = info.later_occluded;
    }
    return 0;
}

/* n samples (gid[i], frame[i]), the first V = min(B, 8) vertices of each: mtype[i * V + v] (0 = no such vertex), material (the
 * index, -1 = no such vertex), flipped and emissive likewise, reason[(i * V + v) * K + k] = ODI_R_* of light sample k at vertex v; end[i * 2 ..] = {OII_END_*, the loop
 * index it happened at}, radiance[i * 3 ..] = L before the fold, nonfinite[i] = a component of L is NaN or infinite */
PTOR_CLONES
int oii_details(const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const float* cam10, int W, int H,
                const int32_t* gid, const int32_t* frame, int64_t n, int K, int B, uint8_t* mtype, int32_t* material, uint8_t* flipped,
                uint8_t* emissive, uint8_t* reason, int32_t* end, float* radiance, uint8_t* nonfinite)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    const int V = B < 8 ? B : 8;
    memset(mtype, 0, (size_t)(n * V));
    for (int64_t i = 0; i < n * V; ++i) material[i] = -1;
    memset(flipped, 0, (size_t)(n * V));
    memset(emissive, 0, (size_t)(n * V));
    memset(reason, ODI_R_NOT_DRAWN, (size_t)(n * V * K));
    for (int64_t i = 0; i < n; ++i) {
        oii_info info;
        const oii_why why = { V, mtype + i * V, material + i * V, flipped + i * V, emissive + i * V, reason + i * V * K };
        const v3 L = oii_sample(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, gid[i] % W, gid[i] / W,
                                W, H, frame[i], K, B, &info, &why);
        radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
        end[2 * i] = info.end;
        end[2 * i + 1] = info.end_at;
        nonfinite[i] = (uint8_t)!(isfinite(L.x) && isfinite(L.y) && isfinite(L.z));
    }
    return 0;
}
