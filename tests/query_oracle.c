/*
 * query_oracle.c -- the CPU oracle's closest hit and camera rays in the layouts of pt_intersect_rays / pt_camera_rays.
 * TEST INFRASTRUCTURE.
 *
 * Follows tests/camera_oracle.c (and through it oracle/pt_oracle.c, whole) in tests/oracles.c; the operations are the oracle's:
 *   - oq_closest: ptor_get_ray, then ptor_intersect_triangle over the triangles in ascending order (the loop of
 *     ptor_intersect_world, GenerateColors.cl:137-154) with hitDistance starting at min(tmax, 1e20) instead of 1e20 -- a ray
 *     whose tmax is NaN or <= 0 tests nothing -- plus the winner's (u, v) and material, which ptor_hit does not keep: u and v
 *     restate :96-117 with the oracle's v3 functions;
 *   - oq_all_hits: the same test over every triangle with hitDistance held at min(tmax, 1e20): every triangle the exact test accepts
 *     for a ray, not only the closest (the measurement of the LBVH's margin, tests/test_lbvh_margin_cpu.py);
 *   - oq_get_rays: the origin and the direction ptor_get_ray makes of a ray (the direction every test above really uses);
 *   - oq_camera_rays: ocam_generate_ray's expression up to the argument the reference passes to getRay at :287 (normalised once).
 * Compiled with oracle/Makefile's flags (tests/oracles.py).
 */
/* n rays of 8 floats (origin xyz, tmax, dir xyz, reserved) -> n records of 12 words in pt_hit's layout:
 * t, tri, u, v, p xyz, material, n xyz, 0; a miss is t = +inf, tri = -1, material = -1, everything else 0 */
PTOR_CLONES
void oq_closest(const void* tris_, int ntri, const float* rays, int64_t n, float* out)
{
    const ptor_triangle* tris = (const ptor_triangle*)tris_;
    ptor_stats st;
    memset(&st, 0, sizeof st);
    for (int64_t k = 0; k < n; ++k) {
        const float* r8 = rays + 8 * k;
        float* o = out + 12 * k;
        int32_t* oi = (int32_t*)o;
        const ptor_ray r = ptor_get_ray(v3_make(r8[0], r8[1], r8[2]), v3_make(r8[4], r8[5], r8[6]));
        ptor_hit rec;
        memset(&rec, 0, sizeof rec);
        rec.tri = -1;
        int hit = 0;
        if (r8[3] > 0.0f) {
            float hitDistance = r8[3] < 1e20f ? r8[3] : 1e20f;
            for (int i = 0; i < ntri; i++)
                if (ptor_intersect_triangle(&r, &tris[i], i, &rec, hitDistance, &st)) {
                    hitDistance = rec.t;
                    hit = 1;
                }
        }
        memset(o, 0, 12 * sizeof(float));
        if (!hit) {
            o[0] = INFINITY;
            oi[1] = -1;
            oi[7] = -1;
            continue;
        }
        const ptor_triangle* t = &tris[rec.tri];
        const v3 p1 = v3_make(t->p1[0], t->p1[1], t->p1[2]);
        const v3 e1 = v3_sub(v3_make(t->p2[0], t->p2[1], t->p2[2]), p1);
        const v3 e2 = v3_sub(v3_make(t->p3[0], t->p3[1], t->p3[2]), p1);
        const v3 pvec = v3_cross(r.dir, e2);
        const float inv_det = 1.0f / v3_dot(e1, pvec);
        const v3 tvec = v3_sub(r.origin, p1);
        const float u = v3_dot(tvec, pvec) * inv_det;
        const v3 qvec = v3_cross(tvec, e1);
        const float v = v3_dot(r.dir, qvec) * inv_det;
        o[0] = rec.t;
        oi[1] = rec.tri;
        o[2] = u;
        o[3] = v;
        o[4] = rec.p.x; o[5] = rec.p.y; o[6] = rec.p.z;
        oi[7] = t->id;
        o[8] = rec.n.x; o[9] = rec.n.y; o[10] = rec.n.z;
    }
}

/* Every (ray, triangle, t) the exact test accepts at 0 < t < min(tmax, 1e20), rays ascending and triangles ascending within a ray.
 * At most `cap` records are written; the return value is how many there are (call again with more room if it exceeds cap). */
PTOR_CLONES
int64_t oq_all_hits(const void* tris_, int ntri, const float* rays, int64_t n, int64_t cap, int64_t* ray_out, int32_t* tri_out, float* t_out)
{
    const ptor_triangle* tris = (const ptor_triangle*)tris_;
    ptor_stats st;
    memset(&st, 0, sizeof st);
    int64_t m = 0;
    for (int64_t k = 0; k < n; ++k) {
        const float* r8 = rays + 8 * k;
        if (!(r8[3] > 0.0f)) continue;
        const ptor_ray r = ptor_get_ray(v3_make(r8[0], r8[1], r8[2]), v3_make(r8[4], r8[5], r8[6]));
        const float hitDistance = r8[3] < 1e20f ? r8[3] : 1e20f;
        for (int i = 0; i < ntri; i++) {
            ptor_hit rec;
            if (!ptor_intersect_triangle(&r, &tris[i], i, &rec, hitDistance, &st)) continue;
            if (m < cap) { ray_out[m] = k; tri_out[m] = i; t_out[m] = rec.t; }
            ++m;
        }
    }
    return m;
}

/* n rays of 8 floats -> n x 6 floats: origin, then the normalised direction of ptor_get_ray */
void oq_get_rays(const float* rays, int64_t n, float* out)
{
    for (int64_t k = 0; k < n; ++k) {
        const float* r8 = rays + 8 * k;
        const ptor_ray r = ptor_get_ray(v3_make(r8[0], r8[1], r8[2]), v3_make(r8[4], r8[5], r8[6]));
        float* o = out + 6 * k;
        o[0] = r.origin.x; o[1] = r.origin.y; o[2] = r.origin.z;
        o[3] = r.dir.x; o[4] = r.dir.y; o[5] = r.dir.z;
    }
}

/* width x height rays of 8 floats: eye, 1e20, the direction getRay receives at :287, 0; seed gid + hash(frame) (:305-308).
 * cam10: eye xyz, center xyz, up xyz, fov_y_deg (NULL = the reference's).  Returns -1 for a camera ocam_derive rejects. */
PTOR_CLONES
int oq_camera_rays(const float* cam10, int W, int H, int frame, float* out)
{
    static const float ref10[10] = { 0.0f, 2.75f, 4.0f, 0.0f, 2.75f, 3.0f, 0.0f, 1.0f, 0.0f, 60.0f };
    float d16[16];
    if (ocam_derive(cam10 ? cam10 : ref10, d16) != 0) return -1;
    const ocam c = ocam_from(d16);
    const float invWidth = 1.0f / (float)W, invHeight = 1.0f / (float)H;
    const float aspectratio = (float)W / (float)H;
    for (int64_t gid = 0; gid < (int64_t)W * H; ++gid) {
        uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)frame);
        float x = (float)(gid % W) + ptor_random_float(&seed) - 0.5f;
        float y = (float)(gid / W) + ptor_random_float(&seed) - 0.5f;
        x = (2.0f * ((x + 0.5f) * invWidth) - 1.0f) * c.angle * aspectratio;
        y = -(1.0f - 2.0f * ((y + 0.5f) * invHeight)) * c.angle;
        float my = -1.0f * y;
        v3 d = v3_add(v3_add(v3_scale(c.hol, x), v3_scale(c.up, my)), c.view);
        v3 dir = v3_normalize(d);
        v3 pointAimed = v3_add(c.eye, v3_scale(dir, 4.0f));
        const v3 aim = v3_normalize(v3_sub(pointAimed, c.eye));
        float* o = out + 8 * gid;
        o[0] = c.eye.x; o[1] = c.eye.y; o[2] = c.eye.z; o[3] = 1e20f;
        o[4] = aim.x; o[5] = aim.y; o[6] = aim.z; o[7] = 0.0f;
    }
    return 0;
}
