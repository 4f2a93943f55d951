/*
 * feature_oracle.c -- the one translation unit of tests/libtest_feature_oracle.so (tests/feature_oracle.py builds it): the CPU
 * oracle's first-hit feature samples in the layout of pt_render_features.  TEST INFRASTRUCTURE.
 *
 * Follows tests/lens_oracles.c, which brings oracle/pt_oracle.c, the camera restatement and the thin lens (ocam_generate_ray is
 * olens_generate_ray from there on: with the lens (0, 0) the pinhole's ray, bit for bit), and composes the sample of
 * pt_render_features (include/pt_shim.h) from the oracle's own operations, in the order the contract states them:
 *   - the sample of pixel gid in frame z: seed = gid + hash(z), the primary ray (GenerateColors.cl:263-288, :308), its closest hit
 *     by ptor_intersect_world (:137-154);
 *   - on a hit n = rec.n turned to face the ray (:243), m = mats[the triangle's id clamped into [0, nmat)];
 *   - albedo = m.albedo as stored, normal = n, depth = (t, 1, -dot(n, d)), emission = 1.0f * m.emissive * 3.0f (:241); a miss is zeros.
 * Compiled with oracle/Makefile's flags (tests/oracles.py: CFLAGS).
 */
#include "lens_oracles.c"

/* [frame_count][local pixels][3] floats into each output that is not NULL: the local rows of rank in the stripe layout of
 * pt_render_params, ascending.  info (may be NULL): per sample three int32 -- the triangle hit (-1: a miss), its id as stored, 1 when
 * the normal was negated at :243.  cam10: eye xyz, center xyz, up xyz, fov_y_deg (NULL = the reference's); (R, F): the thin lens,
 * (0, 0) the pinhole.  Returns -1 for a camera or a lens the contract rejects. */
PTOR_CLONES
int ofe_samples(const void* tris_, int ntri, const void* mats_, int nmat, const float* cam10, float R, float F, int W, int H,
                int stripe_rows, int n_ranks, int rank, int frame_begin, int frame_count, float* albedo, float* normal, float* depth,
                float* emission, int32_t* info)
{
    const ptor_triangle* tris = (const ptor_triangle*)tris_;
    const ptor_material* mats = (const ptor_material*)mats_;
    ocam c;
    if (odi_camera(cam10, &c) != 0) return -1;
    if (olens_set(R, F) != 0) return -1;
    int64_t npix = 0;
    for (int grow = 0; grow < H; ++grow)
        if ((grow / stripe_rows) % n_ranks == rank) npix += W;
    for (int f = 0; f < frame_count; ++f) {
        int64_t lp = 0;
        for (int grow = 0; grow < H; ++grow) {
            if ((grow / stripe_rows) % n_ranks != rank) continue;
            for (int x = 0; x < W; ++x, ++lp) {
                ptor_stats st;
                memset(&st, 0, sizeof st);
                const int gid = grow * W + x;
                uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)(frame_begin + f));
                const ptor_ray r = ocam_generate_ray(&c, x, grow, W, H, &seed);
                ptor_hit rec;
                memset(&rec, 0, sizeof rec);
                const int hit = ptor_intersect_world(&r, tris, ntri, &rec, &st);
                v3 a = v3_make(0.0f, 0.0f, 0.0f), n = a, d = a, e = a;
                int32_t tri = -1, id = 0, flipped = 0;
                if (hit) {
                    tri = rec.tri;
                    id = tris[rec.tri].id;
                    const ptor_material* m = &mats[odi_clampi(id, nmat)];
                    const int facing = v3_dot(rec.n, r.dir) < 0.0f;
                    n = facing ? rec.n : v3_scale(rec.n, -1.0f);   /* :243 */
                    flipped = !facing;
                    a = v3_make(m->albedo[0], m->albedo[1], m->albedo[2]);
                    d = v3_make(rec.t, 1.0f, -v3_dot(n, r.dir));
                    e = v3_make(1.0f * m->emissive[0] * 3.0f, 1.0f * m->emissive[1] * 3.0f, 1.0f * m->emissive[2] * 3.0f);   /* :241 */
                }
                const int64_t i = (int64_t)f * npix + lp;
                if (albedo) { albedo[3 * i] = a.x; albedo[3 * i + 1] = a.y; albedo[3 * i + 2] = a.z; }
                if (normal) { normal[3 * i] = n.x; normal[3 * i + 1] = n.y; normal[3 * i + 2] = n.z; }
                if (depth) { depth[3 * i] = d.x; depth[3 * i + 1] = d.y; depth[3 * i + 2] = d.z; }
                if (emission) { emission[3 * i] = e.x; emission[3 * i + 1] = e.y; emission[3 * i + 2] = e.z; }
                if (info) { info[3 * i] = tri; info[3 * i + 1] = id; info[3 * i + 2] = flipped; }
            }
        }
    }
    olens_set(0.0f, 0.0f);
    return 0;
}
