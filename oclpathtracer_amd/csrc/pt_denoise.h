// pt_denoise.h -- the launch side of pt_denoise (include/pt_shim.h states the arithmetic; pt_denoise.hip holds the kernels).
// A header of its own, beside pt_kernels.h: the denoiser shares no code with the renderers and rebuilds none of theirs.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define PT_DENOISE_PLANES 6u   // float4 planes of the scratch: (c, var), (nrm, z), (a, gx), (e, gy), two for the levels to alternate between
#define PT_DENOISE_MAX_LEVELS 8
enum { PT_DENOISE_GUIDE_ALBEDO = 1, PT_DENOISE_GUIDE_NORMAL = 2, PT_DENOISE_GUIDE_DEPTH = 4, PT_DENOISE_GUIDE_EMISSION = 8 };
enum { PT_DENOISE_GATHER_AUTO = 0, PT_DENOISE_GATHER_GLOBAL = 1, PT_DENOISE_GATHER_LDS = 2 };   // PT_OPT_DENOISE_TILE
enum { PT_DENOISE_POOL_AUTO = 0, PT_DENOISE_POOL_GLOBAL = 1, PT_DENOISE_POOL_LDS = 2 };         // PT_OPT_DENOISE_SPATIAL_FORM
#define PT_DENOISE_POOL_RADIUS 3   // pt_denoise_spatial pools over 7 x 7

struct PtDenoiseArgs {
    int32_t width, height, levels, squarings;
    uint32_t guides;   // PT_DENOISE_GUIDE_*: the guides given
    float sigma_l, sigma_z, sigma_a, sigma_e, eps_l, eps_z;
};

// 56-byte moment records (PtPixelMoments of pt_kernels.h), passed untyped: this header includes none of the renderers'
hipError_t ptk_denoise(const void* colour, const void* albedo, const void* normal, const void* depth, const void* emission,
                       float4* scratch, float4* out, const PtDenoiseArgs& args, int gather, hipStream_t s);
// pt_denoise_spatial: the same launches with the pool pass between prepare and level 0; `below` <= 1 names no pixel and skips it
hipError_t ptk_denoise_spatial(const void* colour, const void* albedo, const void* normal, const void* depth, const void* emission,
                               float4* scratch, float4* out, const PtDenoiseArgs& args, int32_t below, int gather, int pool_form, hipStream_t s);
