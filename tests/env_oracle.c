/*
 * env_oracle.c -- the CPU oracle's environment lighting: pt_env_table's table, the two mappings of the octahedral map and the two
 * estimators pt_render_direct_env and pt_render_indirect_env in their layouts.  TEST INFRASTRUCTURE.
 *
 * Stated from include/pt_shim.h alone ("environment lighting").  Follows tests/roulette_oracle.c in tests/env_oracles.c, so the oracle,
 * the camera and the illumination restatements come as that unit's statics; what it takes from them is the oracle's own operations,
 * odi_fold, odi_camera, opw_tab, opw_light (the light sample by power, with its MIS weight) and the ODI_R_* / OMI_W_* codes.
 *   - oev_index, oev_texel, oev_point, oev_pdf: the map's geometry, expression for expression;
 *   - oev_table: the table, sequentially;
 *   - oev_light: an environment sample, steps a-i; oev_miss: what a ray that leaves the scene adds;
 *   - oev_direct: opw_direct's walk, oev_path: orr_path's with mis = 1 and the table, with the environment where the contract puts it.
 * Per environment sample the optional account says why it ended (OEV_R_*), per vertex the texel and the weight of a miss.
 * The identity "every texel 0.45, Ke = 0" against opw_render / orr_render, bit for bit, pins it to them (tests/test_env_cpu.py).
 * Compiled with oracle/Makefile's flags (tests/env_oracle.py).
 */
enum { OEV_R_NOT_DRAWN = 0, OEV_R_BELOW_HORIZON = 1, OEV_R_OTHER_TYPE = 2, OEV_R_EMPTY_TABLE = 3, OEV_R_OPEN = 4, OEV_R_OCCLUDED = 5, OEV_R_NAN = 6 };
enum { OEV_SIZE_MAX = 2048, OEV_DETAIL_VERTICES = 8 };

typedef struct oev_map {
    const float* texels;   /* [N * N][4] */
    const uint64_t* cdf;   /* [N * N + 1]; may be 0 when Ke == 0 */
    int N, Ke;
} oev_map;

PTOR_INLINE float oev_sgn(float v) { return v < 0.0f ? -1.0f : 1.0f; }

PTOR_INLINE uint32_t oev_index(float c, int N)
{
    const float v = ((c + 1.0f) * 0.5f) * (float)N;
    if (!(v >= 0.0f)) return 0u;
    return v >= (float)(N - 1) ? (uint32_t)(N - 1) : (uint32_t)v;
}

PTOR_INLINE uint32_t oev_texel(v3 d, int N, float* s_out)
{
    const float s = (fabsf(d.x) + fabsf(d.y)) + fabsf(d.z);
    const float x = d.x / s, z = d.z / s;
    float a = x, b = z;
    if (!(d.y >= 0.0f)) {
        a = (1.0f - fabsf(z)) * oev_sgn(x);
        b = (1.0f - fabsf(x)) * oev_sgn(z);
    }
    *s_out = s;
    return oev_index(b, N) * (uint32_t)N + oev_index(a, N);
}

PTOR_INLINE v3 oev_point(float a, float b)
{
    const float fa = fabsf(a), fb = fabsf(b);
    const float h = (1.0f - fa) - fb;
    if (h >= 0.0f) return v3_make(a, h, b);
    return v3_make((1.0f - fb) * oev_sgn(a), h, (1.0f - fa) * oev_sgn(b));
}

PTOR_INLINE float oev_pdf(uint64_t q, uint64_t total, int N, float r)
{
    const float nn4 = ((float)N * (float)N) * 0.25f;
    return (((float)q / (float)total) * nn4) * ((r * r) * r);
}

PTOR_INLINE int oev_size_valid(int N) { return N >= 1 && N <= OEV_SIZE_MAX && (N & (N - 1)) == 0; }

/* n directions [n][3] -> texel[n] */
PTOR_CLONES
int oev_texels(const float* dirs, int64_t n, int N, uint32_t* texel)
{
    if (!oev_size_valid(N)) return -2;
    for (int64_t i = 0; i < n; ++i) {
        float s;
        texel[i] = oev_texel(v3_make(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), N, &s);
    }
    return 0;
}

/* n points (a, b) [n][2] -> the normalised direction [n][3] and r[n] */
PTOR_CLONES
int oev_directions(const float* ab, int64_t n, float* dirs, float* r)
{
    for (int64_t i = 0; i < n; ++i) {
        const v3 P = oev_point(ab[2 * i], ab[2 * i + 1]);
        const v3 w = v3_normalize(P);
        dirs[3 * i] = w.x; dirs[3 * i + 1] = w.y; dirs[3 * i + 2] = w.z;
        r[i] = sqrtf(v3_dot(P, P));
    }
    return 0;
}

/* cdf[N * N + 1] */
PTOR_CLONES
int oev_table(const float* texels, int N, uint64_t* cdf)
{
    if (!oev_size_valid(N)) return -2;
    const int64_t nn = (int64_t)N * N;
    float* pw = (float*)malloc(sizeof(float) * (size_t)nn);
    if (!pw) return -1;
    const float step = 2.0f / (float)N;
    float pmax = 0.0f;
    for (int64_t i = 0; i < nn; ++i) {
        const int col = (int)(i % N), row = (int)(i / N);
        const v3 P = oev_point(((float)col + 0.5f) * step - 1.0f, ((float)row + 0.5f) * step - 1.0f);
        const float rc = sqrtf(v3_dot(P, P));
        const float* le = texels + 4 * i;
        const float p = ((le[0] + le[1]) + le[2]) * (1.0f / ((rc * rc) * rc));
        pw[i] = (p > 0.0f && p < INFINITY) ? p : 0.0f;
        if (pw[i] > pmax) pmax = pw[i];
    }
    cdf[0] = 0u;
    for (int64_t i = 0; i < nn; ++i) {
        uint32_t q = 0u;
        if (pw[i] > 0.0f) {
            q = (uint32_t)((pw[i] / pmax) * 65536.0f);
            if (q < 1u) q = 1u;
        }
        cdf[i + 1] = cdf[i] + q;
    }
    free(pw);
    return 0;
}

/* what a ray of direction d that leaves the scene adds per unit of mask; weigh: balanced against the Ke environment samples of the
 * vertex before.  texel_out / wb_out: the account */
PTOR_INLINE v3 oev_miss(const oev_map* E, v3 d, int weigh, float pb, int32_t* texel_out, float* wb_out)
{
    float s;
    const uint32_t i = oev_texel(d, E->N, &s);
    const float* le = E->texels + 4 * (size_t)i;
    v3 Le = v3_make(le[0], le[1], le[2]);
    float wb = 1.0f;
    if (weigh) {
        const uint64_t total = E->cdf[(size_t)E->N * E->N];
        const uint64_t q = E->cdf[i + 1] - E->cdf[i];
        if (q != 0u && total != 0u) {
            const float r = sqrtf(v3_dot(d, d)) / s;
            wb = pb / ((float)E->Ke * oev_pdf(q, total, E->N, r) + pb);
        }
        Le = v3_scale(Le, wb);
    }
    if (texel_out) *texel_out = (int32_t)i;
    if (wb_out) *wb_out = wb;
    return Le;
}

/* environment sample at the vertex (p, n, wo) of material m.  mis: weigh against the BRDF sample unless `last`.  Returns the reason */
PTOR_INLINE int oev_light(const ptor_triangle* tris, int ntri, const oev_map* E, int mis, int last, const ptor_material* m, v3 p, v3 n, v3 wo,
                          uint32_t* seed, v3* c_out, int32_t* texel_out, ptor_stats* st)
{
    const v3 albedo = v3_make(m->albedo[0], m->albedo[1], m->albedo[2]);
    const float r0 = ptor_random_float(seed), r1 = ptor_random_float(seed), r2 = ptor_random_float(seed);
    const int64_t nn = (int64_t)E->N * E->N;
    const uint64_t total = E->cdf[nn];
    *texel_out = -1;
    if (total == 0u) return OEV_R_EMPTY_TABLE;
    uint32_t u = (uint32_t)(r0 * 16777216.0f);
    if (u > 16777215u) u = 16777215u;
    const uint64_t x = ((uint64_t)u * total) >> 24;
    int64_t lo = 0, hi = nn;   /* cdf[lo] <= x < cdf[hi] */
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (E->cdf[mid] <= x) lo = mid; else hi = mid;
    }
    const uint64_t q = E->cdf[lo + 1] - E->cdf[lo];
    *texel_out = (int32_t)lo;
    const int col = (int)(lo % E->N), row = (int)(lo / E->N);
    const float step = 2.0f / (float)E->N;
    const v3 P = oev_point(((float)col + r1) * step - 1.0f, ((float)row + r2) * step - 1.0f);
    const float P2 = v3_dot(P, P);
    const float r = sqrtf(P2);
    const v3 wi = v3_normalize(P);
    const float cs = v3_dot(wi, n);
    if (!(cs > 0.0f)) return cs != cs ? OEV_R_NAN : OEV_R_BELOW_HORIZON;
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
        return OEV_R_OTHER_TYPE;   /* :220 */
    }
    const float* le = E->texels + 4 * (size_t)lo;
    const float pdf = oev_pdf(q, total, E->N, r);
    float w = cs / pdf;
    if (mis && !last) {
        const float kp = (float)E->Ke * pdf;
        w = w * (kp / (kp + pbl));
    }
    *c_out = v3_make((f.x * le[0]) * w, (f.y * le[1]) * w, (f.z * le[2]) * w);
    const ptor_ray s = ptor_get_ray(v3_add(p, v3_scale(wi, 0.01f)), wi);   /* :257 */
    int occluded = 0;
    ptor_hit srec;
    for (int i = 0; i < ntri && !occluded; i++) occluded = ptor_intersect_triangle(&s, &tris[i], i, &srec, 1e20f, st);
    return occluded ? OEV_R_OCCLUDED : OEV_R_OPEN;
}

/* one environment sample at a vertex of the caller's -- point p, normal n, wo, a material of (type, albedo, roughness) -- in an empty
 * scene, from `seed`: c[3], the reason, the texel.  For the edges no ray reaches (a NaN normal) */
PTOR_CLONES
int oev_sample_at(const float* texels, const uint64_t* env_cdf, int N, int Ke, int mis, int last, int type, const float* albedo, float roughness,
                  const float* p, const float* n, const float* wo, uint32_t seed, float* c, int32_t* texel)
{
    if (!oev_size_valid(N) || !texels || !env_cdf) return -2;
    const oev_map E = { texels, env_cdf, N, Ke };
    ptor_material m;
    memset(&m, 0, sizeof m);
    m.albedo[0] = albedo[0]; m.albedo[1] = albedo[1]; m.albedo[2] = albedo[2];
    m.roughness = roughness;
    m.type = type;
    ptor_stats st;
    memset(&st, 0, sizeof st);
    v3 cc = v3_make(0.0f, 0.0f, 0.0f);
    const int why = oev_light(0, 0, &E, mis, last, &m, v3_make(p[0], p[1], p[2]), v3_make(n[0], n[1], n[2]), v3_make(wo[0], wo[1], wo[2]), &seed,
                              &cc, texel, &st);
    c[0] = cc.x; c[1] = cc.y; c[2] = cc.z;
    return why;
}

/* the optional account of a sample's first V vertices; the caller has filled the arrays with "nothing" */
typedef struct oev_why {
    int V;
    uint8_t* reason;      /* [V * Ke] */
    int32_t* texel;       /* [V * Ke] the texel chosen, -1: none */
    int32_t* miss_texel;  /* [V] the texel of the ray that left the scene at vertex v, -1: none did */
    float* miss_wb;       /* [V] and its weight (1 where unweighted) */
} oev_why;

PTOR_INLINE v3 oev_max0(v3 L) { return v3_make(ptor_max(L.x, 0.0f), ptor_max(L.y, 0.0f), ptor_max(L.z, 0.0f)); }

/* the Ke environment samples of a vertex: Se */
PTOR_INLINE v3 oev_samples_at(const ptor_triangle* tris, int ntri, const oev_map* E, int mis, int last, const ptor_material* m, v3 p, v3 n, v3 wo,
                              uint32_t* seed, const oev_why* why, int i, ptor_stats* st)
{
    v3 Se = v3_make(0.0f, 0.0f, 0.0f);
    for (int k = 0; k < E->Ke; ++k) {
        v3 c = v3_make(0.0f, 0.0f, 0.0f);
        int32_t texel;
        const int why_k = oev_light(tris, ntri, E, mis, last, m, p, n, wo, seed, &c, &texel, st);
        if (why_k == OEV_R_OPEN) Se = v3_add(Se, c);
        if (why && i < why->V) {
            why->reason[i * E->Ke + k] = (uint8_t)why_k;
            why->texel[i * E->Ke + k] = texel;
        }
    }
    return Se;
}

/* pt_render_direct_env's sample: opw_direct's walk */
PTOR_INLINE v3 oev_direct(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl,
                          const opw_tab* tab, const oev_map* E, int x, int grow, int W, int H, int frame, int K, const oev_why* why)
{
    ptor_stats st;
    memset(&st, 0, sizeof st);
    const int gid = grow * W + x;
    uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)frame);
    const ptor_ray r = ocam_generate_ray(cam, x, grow, W, H, &seed);
    ptor_hit rec;
    memset(&rec, 0, sizeof rec);
    if (!ptor_intersect_world(&r, tris, ntri, &rec, &st))
        return oev_max0(oev_miss(E, r.dir, 0, 0.0f, why ? &why->miss_texel[0] : 0, why ? &why->miss_wb[0] : 0));
    const ptor_material* m = &mats[tris[rec.tri].id];
    const v3 Em = v3_make(1.0f * m->emissive[0] * 3.0f, 1.0f * m->emissive[1] * 3.0f, 1.0f * m->emissive[2] * 3.0f);   /* :241 */
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
    }
    const float Kf = (float)K;
    v3 v = v3_make(Em.x + S.x / Kf, Em.y + S.y / Kf, Em.z + S.z / Kf);
    if (E->Ke > 0) {
        const v3 Se = oev_samples_at(tris, ntri, E, 0, 1, m, rec.p, n, wo, &seed, why, 0, &st);
        const float Kef = (float)E->Ke;
        v = v3_make(v.x + Se.x / Kef, v.y + Se.y / Kef, v.z + Se.z / Kef);
    }
    return oev_max0(v);
}

/* pt_render_indirect_env's sample: orr_path's walk with mis = 1 and the table */
PTOR_INLINE v3 oev_path(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl,
                        const opw_tab* tab, const int32_t* counts, const oev_map* E, int x, int grow, int W, int H, int frame, int K, int B, int R,
                        float cap, const oev_why* why)
{
    ptor_stats st;
    memset(&st, 0, sizeof st);
    const int gid = grow * W + x;
    uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)frame);
    ptor_ray r = ocam_generate_ray(cam, x, grow, W, H, &seed);
    v3 L = v3_make(0.0f, 0.0f, 0.0f);
    v3 mask = v3_make(1.0f, 1.0f, 1.0f);
    const float Kf = (float)K;
    float pb = 0.0f;
    for (int i = 0; i < B; ++i) {
        ptor_hit rec;
        memset(&rec, 0, sizeof rec);
        if (!ptor_intersect_world(&r, tris, ntri, &rec, &st)) {
            const int told = why && i < why->V;
            const v3 le = oev_miss(E, r.dir, i >= 1 && E->Ke > 0, pb, told ? &why->miss_texel[i] : 0, told ? &why->miss_wb[i] : 0);
            L.x = L.x + mask.x * le.x;
            L.y = L.y + mask.y * le.y;
            L.z = L.z + mask.z * le.z;
            break;
        }
        const ptor_triangle* th = &tris[rec.tri];
        const ptor_material* m = &mats[th->id];
        if (i == 0 || nl == 0) {   /* :241 */
            L.x = L.x + mask.x * m->emissive[0] * 3.0f;
            L.y = L.y + mask.y * m->emissive[1] * 3.0f;
            L.z = L.z + mask.z * m->emissive[2] * 3.0f;
        } else if (m->emissive[0] != 0.0f || m->emissive[1] != 0.0f || m->emissive[2] != 0.0f) {
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
                int wcode;
                opw_pick pick;
                const int why_k = opw_light(tris, ntri, mats, lights, nl, tab, counts, K, 1, i == B - 1, m, rec.p, n, wo, &seed, &c, &wcode, &pick, &st);
                if (why_k == ODI_R_OPEN || why_k == ODI_R_OPEN_UNSEARCHED) S = v3_add(S, c);
            }
            L.x = L.x + mask.x * (S.x / Kf);
            L.y = L.y + mask.y * (S.y / Kf);
            L.z = L.z + mask.z * (S.z / Kf);
        }
        if (E->Ke > 0) {
            const v3 Se = oev_samples_at(tris, ntri, E, 1, i == B - 1, m, rec.p, n, wo, &seed, why, i, &st);
            const float Kef = (float)E->Ke;
            L.x = L.x + mask.x * (Se.x / Kef);
            L.y = L.y + mask.y * (Se.y / Kef);
            L.z = L.z + mask.z * (Se.z / Kef);
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
    return oev_max0(L);   /* :260 */
}

PTOR_INLINE v3 oev_sample(int indirect, const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights,
                          int nl, const opw_tab* tab, const int32_t* counts, const oev_map* E, int x, int grow, int W, int H, int frame, int K,
                          int B, int R, float cap, const oev_why* why)
{
    if (!indirect) return oev_direct(cam, tris, ntri, mats, lights, nl, tab, E, x, grow, W, H, frame, K, why);
    return oev_path(cam, tris, ntri, mats, lights, nl, tab, counts, E, x, grow, W, H, frame, K, B, R, cap, why);
}

PTOR_INLINE int oev_args(int nl, const uint64_t* cdf, const uint32_t* tri_q, const float* texels, const uint64_t* env_cdf, int N, int Ke)
{
    if (nl > 0 && !(cdf && tri_q)) return -2;
    if (!oev_size_valid(N) || Ke < 0 || Ke > 256 || !texels || (Ke > 0 && !env_cdf)) return -2;
    return 0;
}

/* orr_render's layout */
PTOR_CLONES
int oev_render(int indirect, const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const uint64_t* cdf,
               const uint32_t* tri_q, const int32_t* counts, const float* texels, const uint64_t* env_cdf, int N, int Ke, const float* cam10, int W,
               int H, int stripe_rows, int n_ranks, int rank, int frame_begin, int frame_count, int K, int B, int R, float cap, float* fb)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    if (oev_args(nl, cdf, tri_q, texels, env_cdf, N, Ke) != 0) return -2;
    const opw_tab tab = { cdf, tri_q };
    const oev_map E = { texels, env_cdf, N, Ke };
    int64_t lp = 0;
    for (int grow = 0; grow < H; ++grow) {
        if ((grow / stripe_rows) % n_ranks != rank) continue;
        for (int x = 0; x < W; ++x, ++lp)
            for (int f = 0; f < frame_count; ++f) {
                const v3 L = oev_sample(indirect, &c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, &tab, counts, &E, x,
                                        grow, W, H, frame_begin + f, K, B, R, cap, 0);
                odi_fold(fb + 4 * lp, L, frame_begin + f);
            }
    }
    return 0;
}

/* n samples (gid[i], frame[i]): radiance[i * 3 ..] = L before the fold; with reason != NULL also, for the first V = (indirect ? min(B, 8) :
 * 1) vertices: reason[(i * V + v) * Ke + k] = OEV_R_* of environment sample k (OEV_R_NOT_DRAWN where it was not taken), texel = the texel
 * it chose (-1: none); miss_texel[i * V + v] = the texel of the ray that left the scene at vertex v (-1: none did), miss_wb its weight */
PTOR_CLONES
int oev_samples(int indirect, const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const uint64_t* cdf,
                const uint32_t* tri_q, const int32_t* counts, const float* texels, const uint64_t* env_cdf, int N, int Ke, const float* cam10, int W,
                int H, const int32_t* gid, const int32_t* frame, int64_t n, int K, int B, int R, float cap, float* radiance, uint8_t* reason,
                int32_t* texel, int32_t* miss_texel, float* miss_wb)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    if (oev_args(nl, cdf, tri_q, texels, env_cdf, N, Ke) != 0) return -2;
    const opw_tab tab = { cdf, tri_q };
    const oev_map E = { texels, env_cdf, N, Ke };
    const int V = !indirect ? 1 : (B < OEV_DETAIL_VERTICES ? B : OEV_DETAIL_VERTICES);
    const int64_t per = (int64_t)V * Ke;
    if (reason) {
        memset(reason, OEV_R_NOT_DRAWN, (size_t)(n * per));
        for (int64_t i = 0; i < n * per; ++i) texel[i] = -1;
        for (int64_t i = 0; i < n * V; ++i) {
            miss_texel[i] = -1;
            miss_wb[i] = 1.0f;
        }
    }
    for (int64_t i = 0; i < n; ++i) {
        const oev_why why = { V, reason ? reason + i * per : 0, reason ? texel + i * per : 0, reason ? miss_texel + i * V : 0, reason ? miss_wb + i * V : 0 };
        const v3 L = oev_sample(indirect, &c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, &tab, counts, &E,
                                gid[i] % W, gid[i] / W, W, H, frame[i], K, B, R, cap, reason ? &why : 0);
        radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
    }
    return 0;
}
