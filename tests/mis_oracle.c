/*
 * mis_oracle.c -- the CPU oracle's path tracing with light sampling at every vertex AND multiple importance sampling, in the layout
 * of pt_render_indirect_mis.  TEST INFRASTRUCTURE.
 *
 * The walk of oii_sample (tests/indirect_oracle.c, which it follows in tests/oracles.c, so the oracle, the camera
 * and both illumination restatements come as that unit's statics) with the changes pt_render_indirect_mis states (include/pt_shim.h), all
 * of them only when nl > 0, and counts[t] = the number of list entries that name triangle t as an input:
 *   - a path carries pb, the pdf of the BRDF sample that made the current ray;
 *   - a light sample (omi_light is oii_light's body with three more values) also forms sl = dot(wi, nj) -- cl = fabs(sl) -- and the
 *     BRDF's density towards wi, pbl; when i < B - 1 and sl > 0 its weight w is multiplied by kp / (kp * counts[j] + pbl), kp = K pe,
 *     pe = d2 / (cl * (area * nl)).  At the last vertex no BRDF ray follows, with sl <= 0 no ray can hit that side of the one-sided
 *     triangle test (:100): w stays;
 *   - at a vertex i >= 1 whose material has an emissive component != 0 the emission IS added, weighted by
 *     wb = pb / ((K pe) * counts[h] + pb) with pe formed from the hit's own distance tt = t + 0.01f (the ray began 0.01 off the vertex
 *     before, :257), so that both techniques form the same pe for the same direction.
 * Two identities pin it (tests/test_mis_cpu.py): with no lights the image is ptor_render's, at B = 1 it is odi_render's, bit for bit;
 * and a sample with no weighted light sample and no later emissive hit is oii_sample's, bit for bit.
 * Compiled with oracle/Makefile's flags (tests/oracles.py).
 */
enum { OMI_W_NONE = 0, OMI_W_WEIGHTED = 1, OMI_W_LAST_VERTEX = 2, OMI_W_BACK_SIDE = 3 };

/* what omi_sample says about a path beside its radiance */
typedef struct omi_info {
    oii_info path;        /* as oii_sample reports it */
    int weighted;         /* light samples of the whole path whose weight was multiplied by the MIS factor */
    int later_emissive;   /* vertices i >= 1 on a material with an emissive component != 0 (nl > 0) */
} omi_info;

/* omi_sample's optional account of the first V vertices (omi_details): oii_why's arrays, and per light sample what became of its
 * weight (OMI_W_*; NONE where the sample did not reach step f), per vertex counts[h] (-1 = no later emissive hit there) and wb */
typedef struct omi_why {
    oii_why base;
    uint8_t* weight;     /* [V * K] */
    int32_t* count;      /* [V] */
    float* wb;           /* [V] */
} omi_why;

/* light sample at the vertex (p, n, wo) of material m: oii_light with the MIS weight.  last: i == B - 1.  *wcode = OMI_W_* */
PTOR_INLINE int omi_light(const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl,
                          const int32_t* counts, int K, int last, const ptor_material* m, v3 p, v3 n, v3 wo, uint32_t* seed, v3* c_out,
                          int* wcode, ptor_stats* st)
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
    const float sl = v3_dot(wi, nj);
    const float cs = v3_dot(wi, n), cl = fabsf(sl);
    *wcode = OMI_W_NONE;
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
    float w = ((cs * cl) / d2) * (area * (float)nl);
    if (last) {
        *wcode = OMI_W_LAST_VERTEX;
    } else if (!(sl > 0.0f)) {
        *wcode = OMI_W_BACK_SIDE;
    } else {
        const float a = area * (float)nl;
        const float pe = d2 / (cl * a);
        const float kp = (float)K * pe;
        w = w * (kp / (kp * (float)counts[j] + pbl));
        *wcode = OMI_W_WEIGHTED;
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

/* one sample: its radiance L before the fold; info and why (each may be NULL) are accounts of the same walk */
PTOR_INLINE v3 omi_sample(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights,
                          int nl, const int32_t* counts, int x, int grow, int W, int H, int frame, int K, int B, omi_info* info,
                          const omi_why* why)
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
    omi_info acc = { { 0, OII_END_DEPTH, B - 1, 0, 0 }, 0, 0 };
    for (int i = 0; i < B; ++i) {
        ptor_hit rec;
        memset(&rec, 0, sizeof rec);
        if (!ptor_intersect_world(&r, tris, ntri, &rec, &st)) {
            L = v3_add(L, v3_scale(mask, bg));
            acc.path.end = OII_END_MISS;
            acc.path.end_at = i;
            break;
        }
        acc.path.vertices++;
        const ptor_triangle* th = &tris[rec.tri];
        const ptor_material* m = &mats[th->id];
        const int told = why && i < why->base.V;
        if (i == 0 || nl == 0) {   /* :241 */
            L.x = L.x + mask.x * m->emissive[0] * 3.0f;
            L.y = L.y + mask.y * m->emissive[1] * 3.0f;
            L.z = L.z + mask.z * m->emissive[2] * 3.0f;
        } else if (m->emissive[0] != 0.0f || m->emissive[1] != 0.0f || m->emissive[2] != 0.0f) {
            const v3 p1 = v3_make(th->p1[0], th->p1[1], th->p1[2]);
            const v3 e1 = v3_sub(v3_make(th->p2[0], th->p2[1], th->p2[2]), p1);
            const v3 e2 = v3_sub(v3_make(th->p3[0], th->p3[1], th->p3[2]), p1);
            const v3 N = v3_cross(e2, e1);                                     /* :123 */
            const float areah = 0.5f * sqrtf(v3_dot(N, N));
            const float clh = fabsf(v3_dot(r.dir, v3_normalize(N)));
            const float tt = rec.t + 0.01f;
            const float pe = (tt * tt) / (clh * (areah * (float)nl));
            const float wb = pb / ((Kf * pe) * (float)counts[rec.tri] + pb);
            L.x = L.x + ((mask.x * m->emissive[0]) * 3.0f) * wb;
            L.y = L.y + ((mask.y * m->emissive[1]) * 3.0f) * wb;
            L.z = L.z + ((mask.z * m->emissive[2]) * 3.0f) * wb;
            acc.later_emissive++;
            if (told) {
                why->count[i] = counts[rec.tri];
                why->wb[i] = wb;
            }
        }
        const int facing = v3_dot(rec.n, r.dir) < 0.0f;
        const v3 n = facing ? rec.n : v3_scale(rec.n, -1.0f);   /* :243 */
        const v3 wo = v3_neg(r.dir);
        if (told) {
            why->base.mtype[i] = (uint8_t)m->type;
            why->base.material[i] = (int32_t)th->id;
            why->base.flipped[i] = (uint8_t)!facing;
            why->base.emissive[i] = (uint8_t)(m->emissive[0] > 0.0f || m->emissive[1] > 0.0f || m->emissive[2] > 0.0f);
        }
        if (nl > 0) {
            v3 S = v3_make(0.0f, 0.0f, 0.0f);
            for (int k = 0; k < K; ++k) {
                v3 c = v3_make(0.0f, 0.0f, 0.0f);
                int wcode;
                const int why_k = omi_light(tris, ntri, mats, lights, nl, counts, K, i == B - 1, m, rec.p, n, wo, &seed, &c, &wcode, &st);
                const int open = why_k == ODI_R_OPEN || why_k == ODI_R_OPEN_UNSEARCHED;
                if (open) S = v3_add(S, c);
                if (i >= 1 && open) acc.path.later_open++;
                if (i >= 1 && why_k == ODI_R_OCCLUDED) acc.path.later_occluded++;
                if (wcode == OMI_W_WEIGHTED) acc.weighted++;
                if (told) {
                    why->base.reason[i * K + k] = (uint8_t)why_k;
                    why->weight[i * K + k] = (uint8_t)wcode;
                }
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
            acc.path.end = OII_END_PDF;
            acc.path.end_at = i;
            break;
        }
        pb = pdf;
        const float d = v3_dot(wi, n);
        mask.x = mask.x * (color.x * d / pdf);
        mask.y = mask.y * (color.y * d / pdf);
        mask.z = mask.z * (color.z * d / pdf);
        r = ptor_get_ray(v3_add(rec.p, v3_scale(wi, 0.01f)), wi);   /* :257 */
    }
    if (info) *info = acc;
    return v3_make(ptor_max(L.x, 0.0f), ptor_max(L.y, 0.0f), ptor_max(L.z, 0.0f));   /* :260 */
}

/* oii_render's arguments and layout, with counts: int32[ntri] (not read when nl = 0) */
PTOR_CLONES
int omi_render(const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const int32_t* counts, const float* cam10,
               int W, int H, int stripe_rows, int n_ranks, int rank, int frame_begin, int frame_count, int K, int B, float* fb)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    int64_t lp = 0;
    for (int grow = 0; grow < H; ++grow) {
        if ((grow / stripe_rows) % n_ranks != rank) continue;
        for (int x = 0; x < W; ++x, ++lp)
            for (int f = 0; f < frame_count; ++f) {
                const v3 L = omi_sample(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, counts, x, grow, W, H,
                                        frame_begin + f, K, B, 0, 0);
                odi_fold(fb + 4 * lp, L, frame_begin + f);
            }
    }
    return 0;
}

/* oii_samples' outputs, and mis[i * 2 ..] = {weighted light samples of the whole path, its later emissive hits} */
PTOR_CLONES
int omi_samples(const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const int32_t* counts, const float* cam10,
                int W, int H, const int32_t* gid, const int32_t* frame, int64_t n, int K, int B, float* radiance, int32_t* vertices,
                uint8_t* end, int32_t* later, int32_t* mis)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    for (int64_t i = 0; i < n; ++i) {
        omi_info info;
        const v3 L = omi_sample(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, counts, gid[i] % W,
                                gid[i] / W, W, H, frame[i], K, B, &info, 0);
        radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
        vertices[i] = info.path.vertices;
        end[i] = (uint8_t)info.path.end;
        later[2 * i] = info.path.later_open;
        later[2 * i + 1] = info.path.later_occluded;
        mis[2 * i] = info.weighted;
        mis[2 * i + 1] = info.later_emissive;
    }
    return 0;
}

/* oii_details' outputs for the first V = min(B, 8) vertices, and weight[(i * V + v) * K + k] = OMI_W_* of light sample k at vertex v,
 * count[i * V + v] = counts[h] of a later emissive hit at vertex v (-1 = none), wb[i * V + v] its weight (0 where none) */
PTOR_CLONES
int omi_details(const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const int32_t* counts, const float* cam10,
                int W, int H, const int32_t* gid, const int32_t* frame, int64_t n, int K, int B, uint8_t* mtype, int32_t* material,
                uint8_t* flipped, uint8_t* emissive, uint8_t* reason, int32_t* end, float* radiance, uint8_t* nonfinite, uint8_t* weight,
                int32_t* count, float* wb)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    const int V = B < 8 ? B : 8;
    memset(mtype, 0, (size_t)(n * V));
    for (int64_t i = 0; i < n * V; ++i) material[i] = -1;
    for (int64_t i = 0; i < n * V; ++i) count[i] = -1;
    for (int64_t i = 0; i < n * V; ++i) wb[i] = 0.0f;
    memset(flipped, 0, (size_t)(n * V));
    memset(emissive, 0, (size_t)(n * V));
    memset(reason, ODI_R_NOT_DRAWN, (size_t)(n * V * K));
    memset(weight, OMI_W_NONE, (size_t)(n * V * K));
    for (int64_t i = 0; i < n; ++i) {
        omi_info info;
        const omi_why why = { { V, mtype + i * V, material + i * V, flipped + i * V, emissive + i * V, reason + i * V * K },
                              weight + i * V * K, count + i * V, wb + i * V };
        const v3 L = omi_sample(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, counts, gid[i] % W,
                                gid[i] / W, W, H, frame[i], K, B, &info, &why);
        radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
        end[2 * i] = info.path.end;
        end[2 * i + 1] = info.path.end_at;
        nonfinite[i] = (uint8_t)!(isfinite(L.x) && isfinite(L.y) && isfinite(L.z));
    }
    return 0;
}
