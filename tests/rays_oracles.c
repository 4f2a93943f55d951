/*
 * rays_oracles.c -- the one translation unit of tests/libtest_rays_oracle.so (tests/rays_oracle.py builds it).  TEST INFRASTRUCTURE.
 *
 * The sample start of include/pt_shim.h's pt_radiance_rays, restated once: orays_generate_ray returns getRay(origin, dir) of a record of
 * a file-scope ray table that orays_set(rays8, n, first_ray) sets BEFORE a call -- the worker threads of the restatements only read
 * it -- and draws nothing.  Then ocam_generate_ray is #defined to it and the direct, indirect, MIS, power and roulette restatements are
 * included AS THEY ARE: a call of theirs for an image of W = first_ray + n by H = 1 pixels computes, for pixel gid, the sample of ray
 * gid - first_ray -- the seed gid + hash(frame) is theirs, the estimators are theirs, only the primary ray is the table's.
 */
#include "camera_oracle.c"

static const float* orays_tab = NULL;   /* n records of 8 floats: origin, tmax (not read), direction, reserved (not read) */
static int64_t orays_n = 0, orays_first = 0;

/* the table of every call that follows (NULL, 0, 0 clears it); the caller keeps the memory alive.  Returns -1 for ids past 2^31 - 1 */
int orays_set(const float* rays8, int64_t n, int64_t first_ray)
{
    orays_tab = NULL;
    orays_n = orays_first = 0;
    if (n < 0 || first_ray < 0 || first_ray + n > 0x7fffffffLL || (n > 0 && !rays8)) return -1;
    orays_tab = rays8;
    orays_n = n;
    orays_first = first_ray;
    return 0;
}

/* pixel (xc, yc) of a width-wide image is the id yc * width + xc; the ray of an id outside the table is a ray that hits nothing
 * anywhere near a scene (a test that reads it has asked for the wrong image) */
PTOR_INLINE ptor_ray orays_generate_ray(const ocam* c, int xc, int yc, int width, int height, uint32_t* seed)
{
    (void)c; (void)height; (void)seed;
    const int64_t k = (int64_t)yc * width + xc - orays_first;
    if (k < 0 || k >= orays_n) return ptor_get_ray(v3_make(1e30f, 1e30f, 1e30f), v3_make(0.0f, 1.0f, 0.0f));
    const float* r8 = orays_tab + 8 * k;
    return ptor_get_ray(v3_make(r8[0], r8[1], r8[2]), v3_make(r8[4], r8[5], r8[6]));
}

#define ocam_generate_ray orays_generate_ray
#include "direct_oracle.c"
#include "indirect_oracle.c"
#include "mis_oracle.c"
#include "power_oracle.c"
#include "roulette_oracle.c"
