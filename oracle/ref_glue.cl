#include "GenerateColors.cl"
/*
 * ref_glue.cl -- entry points with plain pointer arguments into the reference kernel file, which the line above includes by
 * name (the include directory is given at build time: oracle/Makefile, target `ref`).  TEST INFRASTRUCTURE.
 *
 * Nothing of the reference is restated here: every type and function named below is the included file's own.  Each wrapper
 * loads its arguments, calls ONE function of the reference and stores what it returned.  Every wrapper works on n records.
 * The built-ins the reference calls are oracle/ref_builtins.cpp.
 */
void ref_set_global_id(ulong gid); /* oracle/ref_builtins.cpp */

float3 ref_ld3(__global const float* p) { return (float3)(p[0], p[1], p[2]); }
void ref_st3(__global float* p, float3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
void ref_st4(__global float* p, float4 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }

void ref_hash(__global const uint* x, __global uint* out, long n)
{
    for (long i = 0; i < n; ++i) out[i] = hashUInt32(x[i]);
}

void ref_random(__global const uint* seed, __global uint* seed_after, __global float* value, long n)
{
    for (long i = 0; i < n; ++i) {
        unsigned int s = seed[i];
        value[i] = getRandomFloat(&s);
        seed_after[i] = s;
    }
}

/* out12 = origin, dir, invDir, then the three signs as floats */
void ref_get_ray(__global const float* origin3, __global const float* dir3, __global float* out12, long n)
{
    for (long i = 0; i < n; ++i) {
        Ray r = getRay(ref_ld3(origin3 + 3 * i), ref_ld3(dir3 + 3 * i));
        ref_st3(out12 + 12 * i, r.origin);
        ref_st3(out12 + 12 * i + 3, r.dir);
        ref_st3(out12 + 12 * i + 6, r.invDir);
        for (int k = 0; k < 3; ++k) out12[12 * i + 9 + k] = (float)r.sign[k];
    }
}

/* out6 = origin, dir */
void ref_generate_ray(__global const int* xc, __global const int* yc, int width, int height, __global const uint* seed,
                      __global float* out6, __global uint* seed_after, long n)
{
    for (long i = 0; i < n; ++i) {
        unsigned int s = seed[i];
        Ray r = generateRay(xc[i], yc[i], width, height, &s);
        ref_st3(out6 + 6 * i, r.origin);
        ref_st3(out6 + 6 * i + 3, r.dir);
        seed_after[i] = s;
    }
}

/* ray i against triangle tri[i] with tmax[i]; the direction is taken as given.  out7 = t, p, n (zeros when not accepted) */
void ref_intersect_triangle(__global const Triangle* tBuffer, __global const int* tri, __global const float* origin3,
                            __global const float* dir3, __global const float* tmax, __global float* out7, __global int* hit, long n)
{
    for (long i = 0; i < n; ++i) {
        Ray r;
        r.origin = ref_ld3(origin3 + 3 * i);
        r.dir = ref_ld3(dir3 + 3 * i);
        HitRecord h;
        h.t = 0.0f;
        h.p = (float3)(0.0f, 0.0f, 0.0f);
        h.n = (float3)(0.0f, 0.0f, 0.0f);
        h.intersectedTriangle = 0;
        hit[i] = intersectTriangle(&r, &tBuffer[tri[i]], &h, tmax[i]) ? 1 : 0;
        out7[7 * i] = h.t;
        ref_st3(out7 + 7 * i + 1, h.p);
        ref_st3(out7 + 7 * i + 4, h.n);
    }
}

/* ray i through getRay against the NUM_TRIANGLES triangles; out7 = t, p, n; tri = the triangle's index, -1 without a hit */
void ref_intersect_world(__global const Triangle* tBuffer, __global const float* origin3, __global const float* dir3,
                         __global float* out7, __global int* tri, __global int* hit, long n)
{
    for (long i = 0; i < n; ++i) {
        Ray r = getRay(ref_ld3(origin3 + 3 * i), ref_ld3(dir3 + 3 * i));
        HitRecord h;
        h.t = 0.0f;
        h.p = (float3)(0.0f, 0.0f, 0.0f);
        h.n = (float3)(0.0f, 0.0f, 0.0f);
        h.intersectedTriangle = 0;
        hit[i] = intersectWorld(&r, tBuffer, &h) ? 1 : 0;
        out7[7 * i] = h.t;
        ref_st3(out7 + 7 * i + 1, h.p);
        ref_st3(out7 + 7 * i + 4, h.n);
        tri[i] = h.intersectedTriangle ? (int)(h.intersectedTriangle - tBuffer) : -1;
    }
}

void ref_reflect(__global const float* v3, __global const float* n3, __global float* out3, long n)
{
    for (long i = 0; i < n; ++i) ref_st3(out3 + 3 * i, reflect(ref_ld3(v3 + 3 * i), ref_ld3(n3 + 3 * i)));
}

void ref_sample_hemisphere_cosine(__global const float* n3, __global const uint* seed, __global float* out3,
                                  __global uint* seed_after, long n)
{
    for (long i = 0; i < n; ++i) {
        unsigned int s = seed[i];
        ref_st3(out3 + 3 * i, sampleHemisphereCosine(ref_ld3(n3 + 3 * i), &s));
        seed_after[i] = s;
    }
}

void ref_sample_ggx(__global const float* n3, __global const float* roughness, __global const uint* seed, __global float* out3,
                    __global float* cos_theta, __global uint* seed_after, long n)
{
    for (long i = 0; i < n; ++i) {
        unsigned int s = seed[i];
        float ct = 0.0f;
        ref_st3(out3 + 3 * i, sampleGGX(ref_ld3(n3 + 3 * i), roughness[i], &ct, &s));
        cos_theta[i] = ct;
        seed_after[i] = s;
    }
}

void ref_distribution_ggx(__global const float* cos_theta, __global const float* roughness, __global float* out, long n)
{
    for (long i = 0; i < n; ++i) out[i] = distributionGGX(cos_theta[i], roughness[i]);
}

/* wi3 and pdf are in-out: a branch that leaves one untouched leaves what the caller put there */
void ref_brdf(__global const float* wo3, __global const float* normal3, __global const Material* mat, __global const int* mat_index,
              __global const uint* seed, __global float* colour4, __global float* wi3, __global float* pdf,
              __global uint* seed_after, long n)
{
    for (long i = 0; i < n; ++i) {
        unsigned int s = seed[i];
        float3 wi = ref_ld3(wi3 + 3 * i);
        float p = pdf[i];
        ref_st4(colour4 + 4 * i, Brdf(ref_ld3(wo3 + 3 * i), &wi, &p, ref_ld3(normal3 + 3 * i), &mat[mat_index[i]], &s));
        ref_st3(wi3 + 3 * i, wi);
        pdf[i] = p;
        seed_after[i] = s;
    }
}

/* the ray is taken as given (generateRay's result has passed getRay already) */
void ref_trace_rays(__global const Triangle* tBuffer, __global const Material* matBuffer, __global const float* origin3,
                    __global const float* dir3, __global const uint* seed, __global float* radiance4, __global uint* seed_after, long n)
{
    for (long i = 0; i < n; ++i) {
        unsigned int s = seed[i];
        Ray r;
        r.origin = ref_ld3(origin3 + 3 * i);
        r.dir = ref_ld3(dir3 + 3 * i);
        ref_st4(radiance4 + 4 * i, traceRays(&r, tBuffer, matBuffer, &s));
        seed_after[i] = s;
    }
}

void ref_gamma_correct(__global const float4* value, __global float4* out, long n)
{
    for (long i = 0; i < n; ++i) out[i] = gammaCorrect(value[i]);
}

void ref_read_from_gamma(__global const float4* value, __global float4* out, long n)
{
    for (long i = 0; i < n; ++i) out[i] = readFromGamma(value[i]);
}

/* one invocation of the kernel, as work-item gid */
void ref_kernel(__global Triangle* tBuffer, __global Material* matBuffer, __global float4* gDst, int width, int height, int z, int w,
                ulong gid)
{
    ref_set_global_id(gid);
    GenerateColors(tBuffer, matBuffer, gDst, (int4)(width, height, z, w));
}

/* the launch order of the reference's host: frame z = frame_begin, frame_begin + 1, ... each over all width * height work-items */
void ref_render(__global Triangle* tBuffer, __global Material* matBuffer, __global float4* gDst, int width, int height,
                int frame_begin, int frames)
{
    for (int f = 0; f < frames; ++f)
        for (ulong gid = 0; gid < (ulong)width * (ulong)height; ++gid)
            ref_kernel(tBuffer, matBuffer, gDst, width, height, frame_begin + f, 0, gid);
}
