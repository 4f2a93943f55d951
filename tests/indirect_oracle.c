/*
 * indirect_oracle.c -- the CPU oracle's path tracing with light sampling at every vertex, in the layout of pt_render_indirect.
 * TEST INFRASTRUCTURE.
 *
 * Follows tests/direct_oracle.c (tests/indirect_oracles.c includes direct_oracles.c whole: oracle/pt_oracle.c, the camera
 * restatement and direct illumination's come as its statics) and composes the estimator of pt_render_indirect (include/pt_shim.h)
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
 * Compiled with oracle/Makefile's flags (tests/indirect_oracle.py).
 */
enum { OII_END_MISS = 0, OII_END_PDF = 1, OII_END_DEPTH = 2 };

/* what oii_sample says about a path beside its radiance */
typedef struct oii_info {
    int vertices;         /* closest hits: the vertices the path reached, 0 .. B */
    int end;              /* OII_END_* */
    int later_open;       /* light samples at a vertex >= 2 (i >= 1) whose shadow ray was open ... */
    int later_occluded;   /* ... and occluded */
} oii_info;

/* light sample at the vertex (p, n, wo) of material m: odi_sample's loop body.  Returns ODI_NONE (no contribution; the three uniforms
 * are drawn all the same), ODI_OCCLUDED, or ODI_OPEN with *c the contribution */
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
    if (!(cs > 0.0f && cl > 0.0f)) return ODI_NONE;
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
        return ODI_NONE;   /* :220 */
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
    return occluded ? ODI_OCCLUDED : ODI_OPEN;
}

/* one sample: its radiance L before the fold; info (may be NULL) */
PTOR_INLINE v3 oii_sample(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights,
                          int nl, int x, int grow, int W, int H, int frame, int K, int B, oii_info* info)
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
    oii_info acc = { 0, OII_END_DEPTH, 0, 0 };
    for (int i = 0; i < B; ++i) {
        ptor_hit rec;
        memset(&rec, 0, sizeof rec);
        if (!ptor_intersect_world(&r, tris, ntri, &rec, &st)) {
            L = v3_add(L, v3_scale(mask, bg));
            acc.end = OII_END_MISS;
            break;
        }
        acc.vertices++;
        const ptor_material* m = &mats[tris[rec.tri].id];
        if (i == 0 || nl == 0) {   /* :241 */
            L.x = L.x + mask.x * m->emissive[0] * 3.0f;
            L.y = L.y + mask.y * m->emissive[1] * 3.0f;
            L.z = L.z + mask.z * m->emissive[2] * 3.0f;
        }
        const v3 n = v3_dot(rec.n, r.dir) < 0.0f ? rec.n : v3_scale(rec.n, -1.0f);   /* :243 */
        const v3 wo = v3_neg(r.dir);
        if (nl > 0) {
            v3 S = v3_make(0.0f, 0.0f, 0.0f);
            for (int k = 0; k < K; ++k) {
                v3 c = v3_make(0.0f, 0.0f, 0.0f);
                const int dec = oii_light(tris, ntri, mats, lights, nl, m, rec.p, n, wo, &seed, &c, &st);
                if (dec == ODI_OPEN) S = v3_add(S, c);
                if (i >= 1 && dec == ODI_OPEN) acc.later_open++;
                if (i >= 1 && dec == ODI_OCCLUDED) acc.later_occluded++;
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
                                        frame_begin + f, K, B, 0);
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
                                W, H, frame[i], K, B, &info);
        radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
        vertices[i] = info.vertices;
        end[i] = (uint8_t)info.end;
        later[2 * i] = info.later_open;
        later[2 * i + 1] = info.later_occluded;
    }
    return 0;
}
