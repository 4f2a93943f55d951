/*
 * ao_oracle.c -- the CPU oracle's ambient occlusion in the layout of pt_render_ao.  TEST INFRASTRUCTURE.
 *
 * Follows tests/camera_oracle.c (and through it oracle/pt_oracle.c, whole) in tests/oracles.c and composes the estimator of
 * pt_render_ao from the oracle's own operations, in the order the renderer uses them:
 *   - the sample of pixel gid in frame z: seed = gid + hash(z), ocam_generate_ray (GenerateColors.cl:263-288, :308);
 *   - its closest hit: ptor_intersect_triangle over the triangles in ascending order from hitDistance 1e20 (:137-154);
 *   - on a hit: hits += 1, p = rec.p, n = rec.n turned to face the ray (:243), then K times: wi =
 *     ptor_sample_hemisphere_cosine(n, &seed) (:161-172), the ray ptor_get_ray(p + wi 0.01, wi) (:257), and open += 1 unless some
 *     triangle passes ptor_intersect_triangle at 0 < t < min(radius, 1e20).
 * Compiled with oracle/Makefile's flags (tests/oracles.py).
 */
/* one sample; returns 1 when the primary ray hits (then *open = its open occlusion rays, and open_k[k] = 1 for each open one
 * when open_k is not NULL), else 0 */
PTOR_INLINE int oao_sample(const ocam* cam, const ptor_triangle* tris, int ntri, int x, int grow, int W, int H, int frame, int K,
                           float radius, uint32_t* open, uint8_t* open_k)
{
    ptor_stats st;
    memset(&st, 0, sizeof st);
    const int gid = grow * W + x;
    uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)frame);
    const ptor_ray r = ocam_generate_ray(cam, x, grow, W, H, &seed);
    ptor_hit rec;
    memset(&rec, 0, sizeof rec);
    if (!ptor_intersect_world(&r, tris, ntri, &rec, &st)) return 0;
    const v3 n = v3_dot(rec.n, r.dir) < 0.0f ? rec.n : v3_scale(rec.n, -1.0f);
    const float tlim = radius < 1e20f ? radius : 1e20f;
    uint32_t nopen = 0;
    for (int k = 0; k < K; ++k) {
        const v3 wi = ptor_sample_hemisphere_cosine(n, &seed);
        const ptor_ray s = ptor_get_ray(v3_add(rec.p, v3_scale(wi, 0.01f)), wi);
        ptor_hit srec;
        int occluded = 0;
        for (int i = 0; i < ntri && !occluded; i++) occluded = ptor_intersect_triangle(&s, &tris[i], i, &srec, tlim, &st);
        nopen += occluded ? 0u : 1u;
        if (open_k) open_k[k] = occluded ? 0 : 1;
    }
    *open = nopen;
    return 1;
}

/* counts[local pixel] += {open, hits} over frames [frame_begin, frame_begin + frame_count): the local rows of rank in the stripe
 * layout of pt_render_params, ascending.  cam10: eye xyz, center xyz, up xyz, fov_y_deg (NULL = the reference's).  Returns -1 for
 * a camera ocam_derive rejects. */
PTOR_CLONES
int oao_render(const void* tris_, int ntri, const float* cam10, int W, int H, int stripe_rows, int n_ranks, int rank,
               int frame_begin, int frame_count, int K, float radius, uint32_t* counts)
{
    static const float ref10[10] = { 0.0f, 2.75f, 4.0f, 0.0f, 2.75f, 3.0f, 0.0f, 1.0f, 0.0f, 60.0f };
    float d16[16];
    if (ocam_derive(cam10 ? cam10 : ref10, d16) != 0) return -1;
    const ocam c = ocam_from(d16);
    const ptor_triangle* tris = (const ptor_triangle*)tris_;
    int64_t lp = 0;
    for (int grow = 0; grow < H; ++grow) {
        if ((grow / stripe_rows) % n_ranks != rank) continue;
        for (int x = 0; x < W; ++x, ++lp)
            for (int f = 0; f < frame_count; ++f) {
                uint32_t open = 0;
                if (oao_sample(&c, tris, ntri, x, grow, W, H, frame_begin + f, K, radius, &open, 0)) {
                    counts[2 * lp] += open;
                    counts[2 * lp + 1] += 1u;
                }
            }
    }
    return 0;
}

/* n samples (gid[i], frame[i]) of the reference's camera: hit[i], and open_k[i * K + k] = 1 when occlusion ray k is open */
PTOR_CLONES
void oao_decisions(const void* tris_, int ntri, int W, int H, const int32_t* gid, const int32_t* frame, int64_t n, int K, float radius,
                   uint8_t* hit, uint8_t* open_k)
{
    static const float ref10[10] = { 0.0f, 2.75f, 4.0f, 0.0f, 2.75f, 3.0f, 0.0f, 1.0f, 0.0f, 60.0f };
    float d16[16];
    ocam_derive(ref10, d16);
    const ocam c = ocam_from(d16);
    for (int64_t i = 0; i < n; ++i) {
        uint32_t open = 0;
        memset(open_k + i * K, 0, (size_t)K);
        hit[i] = (uint8_t)oao_sample(&c, (const ptor_triangle*)tris_, ntri, gid[i] % W, gid[i] / W, W, H, frame[i], K, radius, &open, open_k + i * K);
    }
}
