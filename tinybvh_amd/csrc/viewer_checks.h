// viewer_checks.h — the argument rules of include/tinybvh_amd.h that the device entry points (capi_viewer.hip) and the host twins (viewer_host.cpp) of the viewer
// frame share: the default light direction, the camera, record arrays, a host sky, the mode.
#pragma once
#include "../../include/tinybvh_amd.h"
#include "viewer.h"

#include <string.h>

namespace tbvh_capi {
int fail(int code, const char* fmt, ...);   // (capi_context.hip) sets tbvh_last_error() of the calling thread, returns code
}

namespace tbvh_viewer_checks {
using tbvh_capi::fail;
using namespace tbvh;

// light_dir of the header: null or all zero = normalize( 2, 4, 5 ) as the demos compute it
inline void lightDir(const float* given, float L[3]) {
    if (given && (given[0] != 0.f || given[1] != 0.f || given[2] != 0.f)) { L[0] = given[0]; L[1] = given[1]; L[2] = given[2]; return; }
    const ShadeV3 d = shade_normalize(ShadeV3{2.f, 4.f, 5.f});
    L[0] = d.x; L[1] = d.y; L[2] = d.z;
}

inline int checkCam(const char* who, const tbvh_camera* cam, ViewerCam* out) {
    if (!cam) return fail(TBVH_E_INVALID, "%s: null camera", who);
    if (cam->width == 0 || cam->height == 0 || (uint64_t)cam->width * cam->height >> 31)
        return fail(TBVH_E_INVALID, "%s: a %u x %u image (positive, below 2^31 pixels in all)", who, cam->width, cam->height);
    memcpy(out->eye, cam->eye, 12); memcpy(out->p1, cam->p1, 12); memcpy(out->p2, cam->p2, 12); memcpy(out->p3, cam->p3, 12);
    out->width = cam->width; out->height = cam->height;
    return 0;
}

inline int checkRecords(const char* who, const void* rays, uint32_t stride, uint64_t n) {
    if (stride < 64 || (stride & 15)) return fail(TBVH_E_INVALID, "%s: a record stride of %u bytes (64 or more, a multiple of 16)", who, stride);
    if (n && !rays) return fail(TBVH_E_INVALID, "%s: null records", who);
    if ((uintptr_t)rays & 15) return fail(TBVH_E_INVALID, "%s: records must be 16-byte aligned", who);
    return 0;
}

inline int checkSkyHost(const char* who, const float* pixels12, uint32_t w, uint32_t h) {
    if (!pixels12 && (w || h)) return fail(TBVH_E_INVALID, "%s: a %u x %u sky without pixels", who, w, h);
    if (pixels12 && (w == 0 || h == 0 || (uint64_t)w * h >> 31)) return fail(TBVH_E_INVALID, "%s: a %u x %u sky (1 .. 2^31 - 1 texels in all)", who, w, h);
    if ((uintptr_t)pixels12 & 3) return fail(TBVH_E_INVALID, "%s: misaligned sky pixels (4 bytes)", who);
    return 0;
}

inline int checkMode(const char* who, uint32_t mode) {
    return mode == TBVH_VIEWER_GLTF || mode == TBVH_VIEWER_FOLIAGE ? 0 : fail(TBVH_E_INVALID, "%s: mode %u (TBVH_VIEWER_GLTF or TBVH_VIEWER_FOLIAGE)", who, mode);
}

}  // namespace tbvh_viewer_checks
