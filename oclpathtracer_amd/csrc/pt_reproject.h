// pt_reproject.h -- the launch side of pt_reproject (include/pt_shim.h states the arithmetic; pt_reproject.hip holds the kernels).
// A header of its own, beside pt_denoise.h: the reprojection shares no code with the renderers and rebuilds none of theirs.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

enum { PT_REPROJECT_FORM_AUTO = 0, PT_REPROJECT_FORM_DIRECT = 1, PT_REPROJECT_FORM_PREPARED = 2 };   // PT_OPT_REPROJECT_FORM

// a camera as pt_camera_derive derives it (the pinhole's thirteen values)
struct PtReprojectCam {
    float eye[3], view[3], hol[3], up[3], angle;
};

struct PtReprojectArgs {
    int32_t width, height, max_history;
    float tol_z, cos_min2, min_weight;     // cos_min2 = cos_min * cos_min, formed once on the host
    float max_noise;                       // 0 = no noise test
    float inv_width, inv_height, aspect;   // 1.0f / W, 1.0f / H, (float)W / (float)H, IEEE quotients formed once on the host
    PtReprojectCam prev, cur;
};

// 56-byte moment records (PtPixelMoments of pt_kernels.h), passed untyped: this header includes none of the renderers'.
// prev_normal and cur_normal are both given or both NULL; out_info may be NULL; scratch holds one float4 per pixel
hipError_t ptk_reproject(const void* prev_colour, const void* prev_normal, const void* prev_depth, const void* cur_normal, const void* cur_depth,
                         float4* scratch, void* out_colour, float4* out_info, const PtReprojectArgs& args, int form, hipStream_t s);
