/*
 * ref_builtins.cpp -- the thirteen OpenCL built-ins that the reference kernel file calls, under PTSPEC, so that
 * the reference's own program text can be compiled for the host and run (oracle/ref_glue.cl, oracle/Makefile: target `ref`).
 * TEST INFRASTRUCTURE.  The arithmetic contract is the given here; the reference's text is what is under test.
 *
 * The names below are the C++ manglings of OpenCL's overloadable built-ins, which is why this is a C++ file: no <cmath>, so that
 * sqrt(float), cos(float), ... are declared here and nowhere else.  sin, cos and pow are the oracle library's exported functions
 * (oracle/pt_oracle.c: ptor_kat_sincos, ptor_kat_pow).  Compile with -ffp-contract=off and no fast-math flag.
 *
 * REF_NO_FMA_CONVENTION: dot and cross with every product and sum rounded (libgencolors_ref_nofma.so, the counterpart of
 * libptoracle_nofma.so).
 */
typedef float float3 __attribute__((ext_vector_type(3)));
typedef float float4 __attribute__((ext_vector_type(4)));
typedef unsigned long ref_size_t; /* OpenCL's size_t on a 64-bit host */

extern "C" void ptor_kat_sincos(float phi, float* s, float* c);
extern "C" float ptor_kat_pow(float x, float y);

static thread_local ref_size_t ref_global_id = 0;

extern "C" void ref_set_global_id(ref_size_t gid) { ref_global_id = gid; }

ref_size_t get_global_id(unsigned int dim) { return dim == 0 ? ref_global_id : 0; }

float sqrt(float x) { return __builtin_sqrtf(x); }
float fabs(float x) { return __builtin_fabsf(x); }
float tan(float x) { return (float)__builtin_tan((double)x); }

float cos(float x)
{
    float s, c;
    ptor_kat_sincos(x, &s, &c);
    return c;
}

float sin(float x)
{
    float s, c;
    ptor_kat_sincos(x, &s, &c);
    return s;
}

float pow(float x, float y) { return ptor_kat_pow(x, y); }

float4 pow(float4 x, float4 y)
{
    float4 r;
    r.x = ptor_kat_pow(x.x, y.x);
    r.y = ptor_kat_pow(x.y, y.y);
    r.z = ptor_kat_pow(x.z, y.z);
    r.w = ptor_kat_pow(x.w, y.w);
    return r;
}

float max(float a, float b) { return (a < b) ? b : a; }

float4 max(float4 a, float b)
{
    float4 r;
    r.x = (a.x < b) ? b : a.x;
    r.y = (a.y < b) ? b : a.y;
    r.z = (a.z < b) ? b : a.z;
    r.w = (a.w < b) ? b : a.w;
    return r;
}

float dot(float3 a, float3 b)
{
#ifdef REF_NO_FMA_CONVENTION
    return (a.x * b.x + a.y * b.y) + a.z * b.z;
#else
    return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x));
#endif
}

float3 cross(float3 a, float3 b)
{
    float3 r;
#ifdef REF_NO_FMA_CONVENTION
    r.x = a.y * b.z - a.z * b.y;
    r.y = a.z * b.x - a.x * b.z;
    r.z = a.x * b.y - a.y * b.x;
#else
    r.x = __builtin_fmaf(a.y, b.z, -(a.z * b.y));
    r.y = __builtin_fmaf(a.z, b.x, -(a.x * b.z));
    r.z = __builtin_fmaf(a.x, b.y, -(a.y * b.x));
#endif
    return r;
}

float3 normalize(float3 v)
{
    float inv = 1.0f / sqrt(dot(v, v));
    return v * inv;
}
