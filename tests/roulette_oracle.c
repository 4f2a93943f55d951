/*
 * roulette_oracle.c -- the CPU oracle's Russian roulette: the four indirect estimators (pt_render_indirect, pt_render_indirect_mis,
 * pt_render_indirect_power with mis 0 and 1) with the roulette of pt_render_indirect_rr, in its layout.  TEST INFRASTRUCTURE.
 *
 * Stated from include/pt_shim.h alone ("Russian roulette").  Follows tests/power_oracle.c in tests/roulette_oracles.c, so the oracle, the
 * camera and the illumination restatements come as that unit's statics; what it takes from them is the oracle's own operations and the
 * light samples oii_light / omi_light / opw_light, odi_fold, odi_camera and the ODI_R_* / OII_END_* codes.
 *   - orr_path: oii_sample's walk (mis: omi_sample's; power: opw_path's) -- the statements are theirs, in their order -- with the
 *     roulette at the end of step 2d: when i + 1 >= R and i < B - 1, r is drawn, s = max(mask.x, max(mask.y, mask.z)), q = min(s, cap);
 *     q >= 1 goes on unchanged; otherwise the path goes on iff r < q with mask / q.  pb is not touched.
 * Per sample the account says how many vertices the path reached and why it ended (ORR_END_ROULETTE beside OII_END_*), and per
 * vertex what the roulette did (ORR_RR_*) with its s, q and r.
 * The identity R >= B against oii_render / omi_render / opw_render, bit for bit, pins it to them (tests/test_roulette_cpu.py).
 * Compiled with oracle/Makefile's flags (tests/roulette_oracle.py).
 */
enum { ORR_END_ROULETTE = 3 };   /* beside OII_END_MISS, _PDF, _DEPTH */
/* what the roulette did at a vertex: not played (R, the last vertex, or the path ended before); q >= 1, on unchanged; r < q, on with
 * mask / q; ended */
enum { ORR_RR_NONE = 0, ORR_RR_PASS = 1, ORR_RR_SURVIVED = 2, ORR_RR_ENDED = 3 };

/* the optional account of a sample's first V vertices; the caller has filled the arrays with "nothing" */
typedef struct orr_why {
    int V;
    uint8_t* code;   /* [V] ORR_RR_* */
    float* s;        /* [V] */
    float* q;        /* [V] */
    float* r;        /* [V] */
} orr_why;

typedef struct orr_info {
    int vertices;   /* closest hits */
    int end;        /* OII_END_* or ORR_END_ROULETTE */
    int end_at;     /* the loop index at which the path ended */
} orr_info;

PTOR_INLINE v3 orr_path(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats, const int32_t* lights, int nl,
                        const opw_tab* tab /* NULL = the uniform choice */, const int32_t* counts, int mis, int x, int grow, int W, int H,
                        int frame, int K, int B, int R, float cap, orr_info* info, const orr_why* why)
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
    orr_info acc = { 0, OII_END_DEPTH, B - 1 };
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
        const ptor_triangle* th = &tris[rec.tri];
        const ptor_material* m = &mats[th->id];
        if (i == 0 || nl == 0) {   /* :241 */
            L.x = L.x + mask.x * m->emissive[0] * 3.0f;
            L.y = L.y + mask.y * m->emissive[1] * 3.0f;
            L.z = L.z + mask.z * m->emissive[2] * 3.0f;
        } else if (mis && (m->emissive[0] != 0.0f || m->emissive[1] != 0.0f || m->emissive[2] != 0.0f)) {
            const int cnt = counts[rec.tri];
            float wb = 1.0f;
            if (!tab || cnt > 0) {   /* (by power: counts[h] = 0 gives wb = 1 and reads no table) */
                const v3 p1 = v3_make(th->p1[0], th->p1[1], th->p1[2]);
                const v3 e1 = v3_sub(v3_make(th->p2[0], th->p2[1], th->p2[2]), p1);
                const v3 e2 = v3_sub(v3_make(th->p3[0], th->p3[1], th->p3[2]), p1);
                const v3 N = v3_cross(e2, e1);                                     /* :123 */
                const float areah = 0.5f * sqrtf(v3_dot(N, N));
                const float clh = fabsf(v3_dot(r.dir, v3_normalize(N)));
                const float tt = rec.t + 0.01f;
                const float invh = tab ? (float)tab->cdf[nl] / (float)tab->tri_q[rec.tri] : (float)nl;
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
                int wcode, why_k;
                opw_pick pick;
                if (tab) why_k = opw_light(tris, ntri, mats, lights, nl, tab, counts, K, mis, i == B - 1, m, rec.p, n, wo, &seed, &c, &wcode, &pick, &st);
                else if (mis) why_k = omi_light(tris, ntri, mats, lights, nl, counts, K, i == B - 1, m, rec.p, n, wo, &seed, &c, &wcode, &st);
                else why_k = oii_light(tris, ntri, mats, lights, nl, m, rec.p, n, wo, &seed, &c, &st);
                if (why_k == ODI_R_OPEN || why_k == ODI_R_OPEN_UNSEARCHED) S = v3_add(S, c);
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
            int code;
            if (q >= 1.0f) {
                code = ORR_RR_PASS;
            } else if (u < q) {
                code = ORR_RR_SURVIVED;
                mask.x = mask.x / q;
                mask.y = mask.y / q;
                mask.z = mask.z / q;
            } else {
                code = ORR_RR_ENDED;
            }
            if (why && i < why->V) {
                why->code[i] = (uint8_t)code;
                why->s[i] = s;
                why->q[i] = q;
                why->r[i] = u;
            }
            if (code == ORR_RR_ENDED) {
                acc.end = ORR_END_ROULETTE;
                acc.end_at = i;
                break;
            }
        }
    }
    if (info) *info = acc;
    return v3_make(ptor_max(L.x, 0.0f), ptor_max(L.y, 0.0f), ptor_max(L.z, 0.0f));   /* :260 */
}

/* opw_render's layout.  mis: 0 / 1; cdf, tri_q: both NULL = the uniform choice; counts: read with mis only */
PTOR_CLONES
int orr_render(int mis, const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const uint64_t* cdf,
               const uint32_t* tri_q, const int32_t* counts, const float* cam10, int W, int H, int stripe_rows, int n_ranks, int rank,
               int frame_begin, int frame_count, int K, int B, int R, float cap, float* fb)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    const opw_tab tab = { cdf, tri_q };
    int64_t lp = 0;
    for (int grow = 0; grow < H; ++grow) {
        if ((grow / stripe_rows) % n_ranks != rank) continue;
        for (int x = 0; x < W; ++x, ++lp)
            for (int f = 0; f < frame_count; ++f) {
                const v3 L = orr_path(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, cdf ? &tab : 0, counts,
                                      mis, x, grow, W, H, frame_begin + f, K, B, R, cap, 0, 0);
                odi_fold(fb + 4 * lp, L, frame_begin + f);
            }
    }
    return 0;
}

/* n samples (gid[i], frame[i]): radiance[i * 3 ..] = L before the fold, vertices[i], end[i * 2 ..] = {ORR/OII_END_*, end_at}; with
 * code != NULL also, for the first V = min(B, 16) vertices: code[i * V + v] = ORR_RR_* of the roulette at vertex v, and its s, q, r
 * (0 where it was not played) */
PTOR_CLONES
int orr_samples(int mis, const void* tris_, int ntri, const void* mats_, const int32_t* lights, int nl, const uint64_t* cdf,
                const uint32_t* tri_q, const int32_t* counts, const float* cam10, int W, int H, const int32_t* gid, const int32_t* frame,
                int64_t n, int K, int B, int R, float cap, float* radiance, int32_t* vertices, int32_t* end, uint8_t* code, float* s, float* q,
                float* r)
{
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    const opw_tab tab = { cdf, tri_q };
    const int V = B < 16 ? B : 16;
    if (code) {
        memset(code, ORR_RR_NONE, (size_t)(n * V));
        for (int64_t i = 0; i < n * V; ++i) s[i] = q[i] = r[i] = 0.0f;
    }
    for (int64_t i = 0; i < n; ++i) {
        const orr_why why = { V, code ? code + i * V : 0, s ? s + i * V : 0, q ? q + i * V : 0, r ? r + i * V : 0 };
        orr_info info;
        const v3 L = orr_path(&c, (const ptor_triangle*)tris_, ntri, (const ptor_material*)mats_, lights, nl, cdf ? &tab : 0, counts, mis,
                              gid[i] % W, gid[i] / W, W, H, frame[i], K, B, R, cap, &info, code ? &why : 0);
        radiance[3 * i] = L.x; radiance[3 * i + 1] = L.y; radiance[3 * i + 2] = L.z;
        vertices[i] = info.vertices;
        end[2 * i] = info.end;
        end[2 * i + 1] = info.end_at;
    }
    return 0;
}
