/*
 * camera_oracle.c -- the CPU oracle (oracle/pt_oracle.c) with the camera as a parameter.  TEST INFRASTRUCTURE.
 *
 * pt_oracle.c restates GenerateColors.cl with the reference's camera built in (ptor_generate_ray).  This file includes it
 * whole -- the RNG, ptor_trace_rays, ptor_pow and the v3 math come as its statics, unchanged -- and adds three things only:
 *   - ocam_generate_ray: ptor_generate_ray (pt_oracle.c:278-303) with eye, basis and angle taken from a camera whose
 *     derived values follow include/pt_shim.h's contract (ocam_derive, the mirror of pt_camera_derive);
 *   - ocam_sample_pixel: ptor_sample_pixel (:490-513), the sample and the gamma fold, with that ray;
 *   - ocam_render: the threaded render over a gid range (ptor_render's driver).
 * Compiled with oracle/Makefile's flags (tests/oracles.py): strict IEEE, no contraction.
 */
#include "../oracle/pt_oracle.c"

typedef struct { v3 eye, view, hol, up; float angle; } ocam;

/* in: eye xyz, center xyz, up xyz, fov_y_deg.  out: eye xyz, viewDir xyz, holDir xyz, upDir xyz, angle, 0, 0, 0.
 * returns 0, or -1 for a camera pt_camera_derive rejects (the reserved fields are not modelled here) */
int ocam_derive(const float* in, float* out)
{
    for (int i = 0; i < 10; ++i)
        if (!isfinite(in[i])) return -1;
    if (!(in[9] > 0.0f && in[9] < 180.0f)) return -1;
    const v3 eye = v3_make(in[0], in[1], in[2]);
    const v3 center = v3_make(in[3], in[4], in[5]);
    const v3 up = v3_make(in[6], in[7], in[8]);
    const v3 viewDir = v3_normalize(v3_sub(center, eye));      /* GenerateColors.cl:270 */
    const v3 holDir = v3_normalize(v3_cross(viewDir, up));     /* :271 */
    const v3 upDir = v3_normalize(v3_cross(holDir, viewDir));  /* :272 */
    const float fov = (float)(((double)in[9] * M_PI) / 180.0);
    const float angle = (float)tan((double)(0.5f * fov));
    const float v[16] = { eye.x, eye.y, eye.z, viewDir.x, viewDir.y, viewDir.z, holDir.x, holDir.y, holDir.z,
                          upDir.x, upDir.y, upDir.z, angle, 0.0f, 0.0f, 0.0f };
    for (int i = 0; i < 13; ++i)
        if (!isfinite(v[i])) return -1;
    memcpy(out, v, sizeof v);
    return 0;
}

static ocam ocam_from(const float* d)
{
    ocam c;
    c.eye = v3_make(d[0], d[1], d[2]);
    c.view = v3_make(d[3], d[4], d[5]);
    c.hol = v3_make(d[6], d[7], d[8]);
    c.up = v3_make(d[9], d[10], d[11]);
    c.angle = d[12];
    return c;
}

/* ptor_generate_ray with the camera's values in place of the literals; the expression is unchanged */
PTOR_INLINE ptor_ray ocam_generate_ray(const ocam* c, int xc, int yc, int width, int height, uint32_t* seed)
{
    float invWidth = 1.0f / (float)width, invHeight = 1.0f / (float)height;
    float aspectratio = (float)width / (float)height;
    float angle = c->angle;

    const v3 eye = c->eye;
    const v3 viewDir = c->view;
    const v3 holDir = c->hol;
    const v3 upDir = c->up;

    float x = (float)xc + ptor_random_float(seed) - 0.5f;
    float y = (float)yc + ptor_random_float(seed) - 0.5f;

    x = (2.0f * ((x + 0.5f) * invWidth) - 1.0f) * angle * aspectratio;
    y = -(1.0f - 2.0f * ((y + 0.5f) * invHeight)) * angle;

    float my = -1.0f * y;
    v3 d = v3_add(v3_add(v3_scale(holDir, x), v3_scale(upDir, my)), viewDir);
    v3 dir = v3_normalize(d);
    v3 pointAimed = v3_add(eye, v3_scale(dir, 4.0f));
    return ptor_get_ray(eye, v3_normalize(v3_sub(pointAimed, eye)));
}

/* ptor_sample_pixel with ocam_generate_ray */
PTOR_INLINE void ocam_sample_pixel(const ocam* cam, const ptor_triangle* tris, int ntri, const ptor_material* mats,
                                   float* px, int gid, int W, int H, int frame, int max_bounces, ptor_stats* st)
{
    const int gi = gid % W;
    const int gj = gid / W;
    uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)frame);
    ptor_ray r = ocam_generate_ray(cam, gi, gj, W, H, &seed);
    v3 c = ptor_trace_rays(&r, tris, ntri, mats, &seed, max_bounces, st, 0);
    st->samples++;
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

typedef struct {
    ptor_job job;
    ocam cam;
} ocam_job;

PTOR_CLONES
static void ocam_run_chunks(ocam_job* oj)
{
    ptor_job* job = &oj->job;
    ptor_stats st;
    memset(&st, 0, sizeof st);
    for (;;) {
        int64_t c = __atomic_fetch_add(job->next_chunk, 1, __ATOMIC_RELAXED);
        int64_t b = c * PTOR_CHUNK;
        if (b >= job->gid_count) break;
        int64_t e = b + PTOR_CHUNK < job->gid_count ? b + PTOR_CHUNK : job->gid_count;
        for (int64_t k = b; k < e; ++k) {
            int gid = (int)(job->gid_begin + k);
            for (int f = 0; f < job->frame_count; ++f)
                ocam_sample_pixel(&oj->cam, job->tris, job->ntri, job->mats, job->fb + 4 * (int64_t)gid, gid,
                                  job->W, job->H, job->frame_begin + f, job->max_bounces, &st);
        }
    }
    job->st = st;
}

static void* ocam_thread_main(void* arg) { ocam_run_chunks((ocam_job*)arg); return 0; }

/* ptor_render seen from a camera: cam_in = eye xyz, center xyz, up xyz, fov_y_deg (derived by ocam_derive).
 * returns -1 for an invalid camera or gid range */
int ocam_render(const void* tris, int ntri, const void* mats, int nmat, float* fb, int W, int H,
                int frame_begin, int frame_count, int max_bounces, int64_t gid_begin,
                int64_t gid_count, int nthreads, ptor_stats* stats, const float* cam_in)
{
    (void)nmat;
    float d[16];
    if (ocam_derive(cam_in, d) != 0) return -1;
    const ocam cam = ocam_from(d);
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 256) nthreads = 256;
    if (gid_begin < 0 || gid_count < 0 || gid_begin + gid_count > (int64_t)W * H) return -1;
    int64_t next = 0;
    ocam_job* jobs = (ocam_job*)calloc((size_t)nthreads, sizeof(ocam_job));
    pthread_t* th = (pthread_t*)calloc((size_t)nthreads, sizeof(pthread_t));
    for (int i = 0; i < nthreads; ++i) {
        ptor_job j = { (const ptor_triangle*)tris, ntri, (const ptor_material*)mats, fb, W, H,
                       frame_begin, frame_count, max_bounces, gid_begin, gid_count, &next, { 0 } };
        jobs[i].job = j;
        jobs[i].cam = cam;
    }
    for (int i = 1; i < nthreads; ++i) pthread_create(&th[i], 0, ocam_thread_main, &jobs[i]);
    ocam_run_chunks(&jobs[0]);
    for (int i = 1; i < nthreads; ++i) pthread_join(th[i], 0);
    if (stats) {
        memset(stats, 0, sizeof *stats);
        for (int i = 0; i < nthreads; ++i) ptor_stats_add(stats, &jobs[i].job.st);
    }
    free(jobs);
    free(th);
    return 0;
}
