/*
 * direct_oracle.c -- the CPU oracle's direct illumination in the layout of pt_render_direct.  TEST INFRASTRUCTURE.
 *
 * Follows tests/ao_oracle.c in tests/oracles.c (oracle/pt_oracle.c and the camera restatement come as that unit's
 * statics) and composes the estimator of pt_render_direct (include/pt_shim.h) from the oracle's own operations, in the order the
 * contract states them:
 *   - the sample of pixel gid in frame z: seed = gid + hash(z), ocam_generate_ray (GenerateColors.cl:263-288, :308), its closest
 *     hit by ptor_intersect_world (:137-154); a miss is the background (:235);
 *   - on a hit E = 1.0f * emissive * 3.0f (:241), n = rec.n turned to face the ray (:243), wo = -d; then K light samples on the
 *     same seed: three uniforms, a light triangle, a point on it, the BRDF value from ptor_brdf's expressions (:203, :211-217,
 *     ptor_distribution_ggx), the geometry term, and a shadow ray ptor_get_ray(p + wi 0.01, wi) (:257) that is occluded when any
 *     triangle passes ptor_intersect_triangle at 0 < t < min(dist - 0.02, 1e20);
 *   - L = max(E + S / K, 0), folded into the pixel as ptor_sample_pixel folds a sample (:314-321).
 * The fold: ptor_sample_pixel traces its own radiance and cannot be handed one, so odi_fold below is its accumulation with the
 * radiance as an argument, statement for statement, as ocam_sample_pixel's is; test_direct_cpu.py pins it to ocam_render with
 * num_lights = 0, where the two must agree bit for bit.
 * Compiled with oracle/Makefile's flags (tests/oracles.py).
 */
enum { ODI_NONE = 0, ODI_OCCLUDED = 1, ODI_OPEN = 2 };

/* Why a light sample ended as it did (odi_details).  ODI_NONE splits into NOT_DRAWN (the primary ray missed or the list is empty:
 * no uniforms are drawn), NOT_FACING (cs <= 0), EDGE_ON (cl <= 0, cs > 0, both finite), NAN (cs or cl NaN) and OTHER_TYPE (:220);
 * ODI_OPEN into OPEN_UNSEARCHED (tl <= 0: nothing is searched) and OPEN; ODI_OCCLUDED stays. */
enum { ODI_R_NOT_DRAWN = 0, ODI_R_NOT_FACING = 1, ODI_R_EDGE_ON = 2, ODI_R_NAN = 3, ODI_R_OTHER_TYPE = 4, ODI_R_OPEN_UNSEARCHED = 5,
       ODI_R_OPEN = 6, ODI_R_OCCLUDED = 7 };

/* odi_sample's optional account of a sample: *flipped = the normal was negated at :243; per light sample its reason code and d2
 * (-1 where the sample was not drawn) */
typedef struct odi_why {
    uint8_t* flipped;
    uint8_t* reason;   /* [K] */
    float* d2;         /* [K] */
} odi_why;

/* ptor_sample_pixel's accumulation (pt_oracle.c:500-513) of the sample radiance c of frame `frame` into px */
PTOR_INLINE void odi_fold(float* px, v3 c, int frame)
{
    const float inv_gamma = 1.0f / PTOR_GAMMA;
    if (frame == 0) {
        px[0] = ptor_pow(c.x, inv_gamma);
        px[1] = ptor_pow(c.y, inv_gamma);
        px[2] = ptor_pow(c.z, inv_gamma);
        px[3] = 1.0f;
    } else {
        float zm1 = (float)(frame - 1), z = (float)frame;
        float ox = ptor_pow(px[0], PTOR_GAMMA), oy = ptor_pow(px[1], PTOR_GAMMA), oz = ptor_pow(px[2], PTOR_GAMMA);
        px[0] = ptor_pow((ox * zm1 + c.x) / z, inv_gamma);
        px[1] = ptor_pow((oy * zm1 + c.y) / z, inv_gamma);
        px[2] = ptor_pow((oz * zm1 + c.z) / z, inv_gamma);
        px[3] = 1.0f;
    }
}

PTOR_INLINE int odi_clampi(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }

/* one sample: its radiance L; *hit = the primary ray hit; dec (may be NULL): per light sample ODI_NONE / ODI_OCCLUDED / ODI_OPEN;
 * why (may be NULL): the reasons behind them */
PTOR_INLINE v3 odi_sample(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights,
                          int nl, int x, int grow, int W, int H, int frame, int K, int* hit, uint8_t* dec, const odi_why* why)
{
    ptor_stats st;
    memset(&st, 0, sizeof st);
    const int gid = grow * W + x;
    uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)frame);
    const ptor_ray r = ocam_generate_ray(cam, x, grow, W, H, &seed);
    ptor_hit rec;
    memset(&rec, 0, sizeof rec);
    if (dec) memset(dec, ODI_NONE, (size_t)K);
    if (why) {
        *why->flipped = 0;
        memset(why->reason, ODI_R_NOT_DRAWN, (size_t)K);
        for (int k = 0; k < K; ++k) why->d2[k] = -1.0f;
    }
    *hit = ptor_intersect_world(&r, tris, ntri, &rec, &st);
    if (!*hit) {
        const float bg = ptor_max(0.45f, 0.0f);   /* :235 */
        return v3_make(bg, bg, bg);
    }
    const ptor_material* m = &mats[tris[rec.tri].id];
    const v3 E = v3_make(1.0f * m->emissive[0] * 3.0f, 1.0f * m->emissive[1] * 3.0f, 1.0f * m->emissive[2] * 3.0f);   /* :241 */
    const v3 p = rec.p;
    const int facing = v3_dot(rec.n, r.dir) < 0.0f;
    const v3 n = facing ? rec.n : v3_scale(rec.n, -1.0f);   /* :243 */
    if (why) *why->flipped = (uint8_t)!facing;
    const v3 wo = v3_neg(r.dir);
    const v3 albedo = v3_make(m->albedo[0], m->albedo[1], m->albedo[2]);
    v3 S = v3_make(0.0f, 0.0f, 0.0f);
    for (int k = 0; k < K && nl > 0; ++k) {
        const float r0 = ptor_random_float(&seed), r1 = ptor_random_float(&seed), r2 = ptor_random_float(&seed);
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
        if (why) why->d2[k] = d2;
        if (!(cs > 0.0f && cl > 0.0f)) {
            if (why) why->reason[k] = (cs != cs || cl != cl) ? ODI_R_NAN : (cs <= 0.0f ? ODI_R_NOT_FACING : ODI_R_EDGE_ON);
            continue;
        }
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
            if (why) why->reason[k] = ODI_R_OTHER_TYPE;
            continue;   /* :220 */
        }
        const ptor_material* mj = &mats[tj->id];
        const float w = ((cs * cl) / d2) * (area * (float)nl);
        const v3 c = v3_make((f.x * (mj->emissive[0] * 3.0f)) * w, (f.y * (mj->emissive[1] * 3.0f)) * w,
                             (f.z * (mj->emissive[2] * 3.0f)) * w);
        const ptor_ray s = ptor_get_ray(v3_add(p, v3_scale(wi, 0.01f)), wi);   /* :257 */
        float tl = dist - 0.02f;
        tl = tl < 1e20f ? tl : 1e20f;
        int occluded = 0;
        if (tl > 0.0f) {
            ptor_hit srec;
            for (int i = 0; i < ntri && !occluded; i++) occluded = ptor_intersect_triangle(&s, &tris[i], i, &srec, tl, &st);
        }
        if (dec) dec[k] = occluded ? ODI_OCCLUDED : ODI_OPEN;
        if (why) why->reason[k] = occluded ? ODI_R_OCCLUDED : (tl > 0.0f ? ODI_R_OPEN : ODI_R_OPEN_UNSEARCHED);
        if (!occluded) S = v3_add(S, c);
    }
    const float Kf = (float)K;
    return v3_make(ptor_max(E.x + S.x / Kf, 0.0f), ptor_max(E.y + S.y / Kf, 0.0f), ptor_max(E.z + S.z / Kf, 0.0f));
}

static int odi_camera(const float* cam10, ocam* c)
{
    static const float ref10[10] = { 0.0f, 2.75f, 4.0f, 0.0f, 2.75f, 3.0f, 0.0f, 1.0f, 0.0f, 60.0f };
    float d16[16];
    if (ocam_derive(cam10 ? cam10 : ref10, d16) != 0) return -1;
    *c = ocam_from(d16);
    return 0;
}

/* fb[local pixel][4]: frames [frame_begin, frame_begin + frame_count) folded in ascending order into what fb holds (frame 0 starts
 * afresh): the local rows of rank in the stripe layout of pt_render_params, ascending.  cam10: eye xyz, center xyz, up xyz,
 * fov_y_deg (NULL = the reference's).  Returns -1 for a camera ocam_derive rejects. */
PTOR_CLONES
int odi_render(const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const float* cam10, int W, int H,
               int stripe_rows, int n_ranks, int rank, int frame_begin, int frame_count, int K, float* fb)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    int64_t lp = 0;
    for (int grow = 0; grow < H; ++grow) {
        if ((grow / stripe_rows) % n_ranks != rank) continue;
        for (int x = 0; x < W; ++x, ++lp)
            for (int f = 0; f < frame_count; ++f) {
                int hit;
                const v3 L = odi_sample(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, x, grow, W, H,
                                        frame_begin + f, K, &hit, 0, 0);
                odi_fold(fb + 4 * lp, L, frame_begin + f);
            }
    }
    return 0;
}

/* n samples (gid[i], frame[i]): hit[i], dec[i * K + k] = ODI_* of light sample k, radiance[i * 3 ..] = L (may be NULL) */
PTOR_CLONES
int odi_decisions(const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const float* cam10, int W, int H,
                  const int32_t* gid, const int32_t* frame, int64_t n, int K, uint8_t* hit, uint8_t* dec, float* radiance)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    for (int64_t i = 0; i < n; ++i) {
        int h;
        const v3 L = odi_sample(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, gid[i] % W, gid[i] / W,
                                W, H, frame[i], K, &h, dec + i * K, 0);
        hit[i] = (uint8_t)h;
        if (radiance) { radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z; }
    }
    return 0;
}

/* n samples (gid[i], frame[i]): hit[i], flipped[i], reason[i * K + k] = ODI_R_* and d2[i * K + k] of light sample k,
 * radiance[i * 3 ..] = L */
PTOR_CLONES
int odi_details(const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const float* cam10, int W, int H,
                const int32_t* gid, const int32_t* frame, int64_t n, int K, uint8_t* hit, uint8_t* flipped, uint8_t* reason, float* d2,
                float* radiance)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    for (int64_t i = 0; i < n; ++i) {
        int h;
        const odi_why why = { flipped + i, reason + i * K, d2 + i * K };
        const v3 L = odi_sample(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, gid[i] % W, gid[i] / W,
                                W, H, frame[i], K, &h, 0, &why);
        hit[i] = (uint8_t)h;
        radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
    }
    return 0;
}
