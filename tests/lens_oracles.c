/*
 * lens_oracles.c -- the one translation unit of tests/libtest_lens_oracle.so (tests/lens_oracle.py builds it).  TEST INFRASTRUCTURE.
 *
 * The thin lens of include/pt_shim.h (pt_camera), restated once: olens_generate_ray is ocam_generate_ray (camera_oracle.c) with the
 * lens step, on a file-scope lens that olens_set(R, F) sets BEFORE a call -- the worker threads of the restatements only read it.
 * Then ocam_generate_ray is #defined to it and the ambient-occlusion, direct, indirect, MIS, power, roulette, RIS and environment
 * restatements are included AS THEY ARE: every estimator's lens form comes from the files that pin its pinhole form, and with
 * olens_set(0, F) each of them is its pinhole form bit for bit (olens_generate_ray then calls ocam_generate_ray itself).
 */
#include "camera_oracle.c"

static float olens_R = 0.0f, olens_F = 0.0f;

/* the lens of every call that follows; returns -1 (and sets the pinhole) for a pair pt_camera_derive rejects */
int olens_set(float R, float F)
{
    olens_R = olens_F = 0.0f;
    if (!(isfinite(R) && R >= 0.0f) || !(isfinite(F) && F >= 0.0f) || (R > 0.0f && !(F > 0.0f))) return -1;
    olens_R = R;
    olens_F = F;
    return 0;
}

/* what the reference passes to getRay at :287 with the lens: the two jitter draws, dir as at :278-284, then u1 and u2;
 *   r = R sqrt(u1), phi = TWO_PI u2, org = (eye + holDir (r cos phi)) + upDir (r sin phi), pointAimed = eye + F dir */
PTOR_INLINE void olens_aim(const ocam* c, float R, float F, int xc, int yc, int width, int height, uint32_t* seed, v3* org, v3* aim)
{
    float invWidth = 1.0f / (float)width, invHeight = 1.0f / (float)height;
    float aspectratio = (float)width / (float)height;
    float angle = c->angle;

    float x = (float)xc + ptor_random_float(seed) - 0.5f;
    float y = (float)yc + ptor_random_float(seed) - 0.5f;

    x = (2.0f * ((x + 0.5f) * invWidth) - 1.0f) * angle * aspectratio;
    y = -(1.0f - 2.0f * ((y + 0.5f) * invHeight)) * angle;

    float my = -1.0f * y;
    v3 d = v3_add(v3_add(v3_scale(c->hol, x), v3_scale(c->up, my)), c->view);
    v3 dir = v3_normalize(d);

    if (!(R > 0.0f)) {   /* the pinhole (olens_camera_rays only): :285 as it stands, no draw */
        *org = c->eye;
        *aim = v3_normalize(v3_sub(v3_add(c->eye, v3_scale(dir, 4.0f)), c->eye));
        return;
    }
    float u1 = ptor_random_float(seed);
    float u2 = ptor_random_float(seed);
    float r = R * sqrtf(u1);
    float phi = PTOR_TWO_PI * u2;
    float sp, cp;
    ptor_sincos(phi, &sp, &cp);
    float lx = r * cp, ly = r * sp;
    *org = v3_add(v3_add(c->eye, v3_scale(c->hol, lx)), v3_scale(c->up, ly));
    v3 pointAimed = v3_add(c->eye, v3_scale(dir, F));
    *aim = v3_normalize(v3_sub(pointAimed, *org));
}

PTOR_INLINE ptor_ray olens_generate_ray(const ocam* c, int xc, int yc, int width, int height, uint32_t* seed)
{
    if (!(olens_R > 0.0f)) return ocam_generate_ray(c, xc, yc, width, height, seed);   /* the pinhole, whatever F holds */
    v3 org, aim;
    olens_aim(c, olens_R, olens_F, xc, yc, width, height, seed, &org, &aim);
    return ptor_get_ray(org, aim);
}

/* the lens form of oq_camera_rays (query_oracle.c): width x height rays of 8 floats -- origin, 1e20, the direction getRay receives at
 * :287 (normalised once), 0 -- with the lens olens_set has set; seed gid + hash(frame).  cam10 NULL = the reference's camera */
int olens_camera_rays(const float* cam10, int W, int H, int frame, float* out)
{
    static const float ref10[10] = { 0.0f, 2.75f, 4.0f, 0.0f, 2.75f, 3.0f, 0.0f, 1.0f, 0.0f, 60.0f };
    float d16[16];
    if (ocam_derive(cam10 ? cam10 : ref10, d16) != 0) return -1;
    const ocam c = ocam_from(d16);
    for (int64_t gid = 0; gid < (int64_t)W * H; ++gid) {
        uint32_t seed = (uint32_t)gid + ptor_hash_u32((uint32_t)frame);
        v3 org, aim;
        olens_aim(&c, olens_R, olens_F, (int)(gid % W), (int)(gid / W), W, H, &seed, &org, &aim);
        float* o = out + 8 * gid;
        o[0] = org.x; o[1] = org.y; o[2] = org.z; o[3] = 1e20f;
        o[4] = aim.x; o[5] = aim.y; o[6] = aim.z; o[7] = 0.0f;
    }
    return 0;
}

/* the ray of one sample, for the geometric checks: out = origin xyz, direction xyz (after getRay) */
void olens_rays(const float* cam10, int W, int H, const int32_t* gid, const int32_t* frame, int64_t n, float* out)
{
    static const float ref10[10] = { 0.0f, 2.75f, 4.0f, 0.0f, 2.75f, 3.0f, 0.0f, 1.0f, 0.0f, 60.0f };
    float d16[16];
    if (ocam_derive(cam10 ? cam10 : ref10, d16) != 0) return;
    const ocam c = ocam_from(d16);
    for (int64_t k = 0; k < n; ++k) {
        uint32_t seed = (uint32_t)gid[k] + ptor_hash_u32((uint32_t)frame[k]);
        const ptor_ray r = olens_generate_ray(&c, gid[k] % W, gid[k] / W, W, H, &seed);
        float* o = out + 6 * k;
        o[0] = r.origin.x; o[1] = r.origin.y; o[2] = r.origin.z;
        o[3] = r.dir.x; o[4] = r.dir.y; o[5] = r.dir.z;
    }
}

#define ocam_generate_ray olens_generate_ray
#include "ao_oracle.c"
#include "direct_oracle.c"
#include "indirect_oracle.c"
#include "mis_oracle.c"
#include "power_oracle.c"
#include "roulette_oracle.c"
#include "ris_oracle.c"
#include "env_oracle.c"
