/*
 * primary_accept.c -- which triangles the reference's test accepts for a sample's PRIMARY ray.  TEST INFRASTRUCTURE.
 *
 * Follows camera_oracle.c in tests/oracles.c (and with it oracle/pt_oracle.c: the RNG, the ray set-up and the v3
 * math come as their statics, unchanged).  It adds one thing: intersectWorld's loop (GenerateColors.cl:137-154) over
 * intersectTriangle (:89-135) for the first ray of sample (gid, frame), restated so that it REPORTS, per triangle, how far
 * the test got instead of keeping the closest hit only:
 *   - accepted: the call returned true (:125 against the running hitDistance of :141-151) -- ptor_stats' `accept`;
 *   - reach_u:  the call got past the cull (:100) and the u test (:109) -- ptor_stats' `rej_v + reach_t`.
 * Triangle j is bit j of a 64-bit set (scenes of up to 64 triangles).  Compiled with oracle/Makefile's flags
 * (tests/oracles.py): strict IEEE, no contraction.
 */
static void opa_sample(const ocam* cam, const ptor_triangle* tris, int ntri, int gid, int W, int H, int frame,
                       uint64_t* accepted, uint64_t* reach_u)
{
    uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)frame);
    const ptor_ray r = cam ? ocam_generate_ray(cam, gid % W, gid / W, W, H, &seed) : ptor_generate_ray(gid % W, gid / W, W, H, &seed);
    float hitDistance = 1e20f;   /* :141 */
    uint64_t acc = 0, ru = 0;
    for (int i = 0; i < ntri; i++) {
        const ptor_triangle* tri = &tris[i];
        v3 p1 = v3_make(tri->p1[0], tri->p1[1], tri->p1[2]);
        v3 p2 = v3_make(tri->p2[0], tri->p2[1], tri->p2[2]);
        v3 p3 = v3_make(tri->p3[0], tri->p3[1], tri->p3[2]);
        v3 e1 = v3_sub(p2, p1);
        v3 e2 = v3_sub(p3, p1);

        v3 pvec = v3_cross(r.dir, e2);
        float det = v3_dot(e1, pvec);
        if (det < 1e-8f || -det > 1e-8f) continue;   /* :100 */

        float inv_det = 1.0f / det;
        v3 tvec = v3_sub(r.origin, p1);
        float u = v3_dot(tvec, pvec) * inv_det;
        if (u < 0.0f || u > 1.0f) continue;          /* :109 */
        ru |= 1ull << i;

        v3 qvec = v3_cross(tvec, e1);
        float v = v3_dot(r.dir, qvec) * inv_det;
        if (v < 0.0f || u + v > 1.0f) continue;      /* :117 */

        float t = v3_dot(e2, qvec) * inv_det;
        if (t > 0.0f && t < hitDistance) {           /* :125 */
            hitDistance = t;                         /* :146 */
            acc |= 1ull << i;
        }
    }
    *accepted = acc;
    *reach_u = ru;
}

/* Per pixel gid[k] (k < n) the UNION over frames [frame_begin, frame_begin + frame_count) of both sets, and in counts[0..1]
 * the number of (sample, triangle) pairs accepted / past u, summed over all those samples.  cam_in: eye xyz, center xyz, up
 * xyz, fov_y_deg, or NULL for the reference's built-in camera.  returns -1 for a camera ocam_derive rejects or ntri > 64 */
int opa_union(const void* tris, int ntri, const float* cam_in, int W, int H, int frame_begin, int frame_count,
              const int32_t* gid, int64_t n, uint64_t* accepted, uint64_t* reach_u, uint64_t* counts)
{
    ocam cam;
    if (ntri < 0 || ntri > 64) return -1;
    if (cam_in) {
        float d[16];
        if (ocam_derive(cam_in, d) != 0) return -1;
        cam = ocam_from(d);
    }
    counts[0] = counts[1] = 0;
    for (int64_t k = 0; k < n; ++k) {
        uint64_t ua = 0, ur = 0;
        for (int f = 0; f < frame_count; ++f) {
            uint64_t a, r;
            opa_sample(cam_in ? &cam : 0, (const ptor_triangle*)tris, ntri, gid[k], W, H, frame_begin + f, &a, &r);
            ua |= a;
            ur |= r;
            counts[0] += (uint64_t)__builtin_popcountll(a);
            counts[1] += (uint64_t)__builtin_popcountll(r);
        }
        accepted[k] = ua;
        reach_u[k] = ur;
    }
    return 0;
}
