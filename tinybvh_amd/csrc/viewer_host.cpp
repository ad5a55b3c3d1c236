// viewer_host.cpp — the host twins of the viewer frame (tbvh_host_sky_* / tbvh_host_viewer_*; include/tinybvh_amd.h, DESIGN.md par. 22): viewer.h's arithmetic
// over host arrays, one thread, no context, no device call.  A translation unit of its own, as pose_host.cpp and omm_host.cpp are, so that
// tools/viewer_sanitize.cpp can compile these very loops — the stride arithmetic, the `continued` / `occ` / `rgb` indexing, the sky passes — with the
// sanitizers; the library builds it with the HIP compiler because viewer.h takes its vector types from the HIP headers.
#include "viewer_checks.h"

#include "../../include/tinybvh_amd_debug.h"

using namespace tbvh;
using namespace tbvh_viewer_checks;

extern "C" {

int tbvh_host_sky_sample(const float* pixels12, uint32_t w, uint32_t h, const void* dirs16, uint64_t n, void* out16) {
    if (int r = checkSkyHost("tbvh_host_sky_sample", pixels12, w, h)) return r;
    if (n && (!dirs16 || !out16)) return fail(TBVH_E_INVALID, "tbvh_host_sky_sample: null directions or output");
    if (((uintptr_t)dirs16 | (uintptr_t)out16) & 3) return fail(TBVH_E_INVALID, "tbvh_host_sky_sample: misaligned directions or output (4 bytes)");
    const ViewerSky sky{pixels12, w, h};
    for (uint64_t i = 0; i < n; i++) {
        float d[4];
        memcpy(d, (const char*)dirs16 + 16 * i, 16);
        uint32_t idx;
        const ShadeV3 c = vw_sample_sky(sky, ShadeV3{d[0], d[1], d[2]}, &idx);
        const float o[4] = {c.x, c.y, c.z, shade_bits_to_float(idx)};
        memcpy((char*)out16 + 16 * i, o, 16);
    }
    return 0;
}

int tbvh_host_sky_prepare(float* pixels12, uint64_t nTexels, const float* scale3, int fromHdr) {
    if (nTexels && !pixels12) return fail(TBVH_E_INVALID, "tbvh_host_sky_prepare: null pixels");
    const float one[3] = {1.f, 1.f, 1.f};
    const float* sc = scale3 ? scale3 : one;
    for (uint64_t i = 0; i < 3 * nTexels; i++) {
        float p = pixels12[i];
        if (fromHdr) p = shade_sqrt(p);
        pixels12[i] = (p * p) * sc[i % 3];
    }
    return 0;
}

// ---- the host twins: viewer.h compiled for the host, one thread, no context ---------------------------------------------------------------------------------
int tbvh_host_viewer_generate(const tbvh_camera* cam, void* rays64, uint64_t first, uint64_t n) {
    ViewerCam vc;
    if (int r = checkCam("tbvh_host_viewer_generate", cam, &vc)) return r;
    if (first + n < first || first + n > (uint64_t)vc.width * vc.height) return fail(TBVH_E_INVALID, "tbvh_host_viewer_generate: rays %llu .. of a %u x %u image", (unsigned long long)first, vc.width, vc.height);
    if (int r = checkRecords("tbvh_host_viewer_generate", rays64, 64, n)) return r;
    for (uint64_t k = 0; k < n; k++) vw_generate(vc, first + k, (float4*)rays64 + 4 * k);
    return 0;
}

int tbvh_host_viewer_continue(const tbvh_material* materials, uint32_t nMats, uint32_t nTex, void* rays, uint32_t stride, const void* out48, uint64_t n, uint8_t* continuedOrNull,
                              uint64_t* nContinuedOrNull) {
    if (!materials || nMats == 0) return fail(TBVH_E_INVALID, "tbvh_host_viewer_continue: no materials");
    if (int r = checkRecords("tbvh_host_viewer_continue", rays, stride, n)) return r;
    if ((n && !out48) || ((uintptr_t)out48 & 15)) return fail(TBVH_E_INVALID, "tbvh_host_viewer_continue: null or misaligned shading records (16 bytes)");
    uint64_t count = 0;
    for (uint64_t i = 0; i < n; i++) {
        float4* rec = (float4*)((char*)rays + i * stride);
        const float4* o = (const float4*)out48 + 3 * i;
        const bool go = vw_continues((const ShadeMat*)materials, nMats, nTex, rec[3], o[0], o[1], o[2]);
        if (go) vw_step_on(rec[0], rec[1], rec[3]);
        if (continuedOrNull) continuedOrNull[i] = go;
        count += go;
    }
    if (nContinuedOrNull) *nContinuedOrNull = count;
    return 0;
}

int tbvh_host_viewer_shadow_rays(const void* rays, uint32_t stride, uint64_t n, const float* lightDirOrNull, void* shadow64) {
    if (int r = checkRecords("tbvh_host_viewer_shadow_rays", rays, stride, n)) return r;
    if (int r = checkRecords("tbvh_host_viewer_shadow_rays", shadow64, 64, n)) return r;
    float Lf[3];
    lightDir(lightDirOrNull, Lf);
    const ShadeV3 L = {Lf[0], Lf[1], Lf[2]};
    for (uint64_t i = 0; i < n; i++) {
        const float4* rec = (const float4*)((const char*)rays + i * stride);
        vw_shadow_ray(rec[0], rec[1], rec[3], L, (float4*)shadow64 + 4 * i);
    }
    return 0;
}

int tbvh_host_viewer_light(uint32_t mode, const float* skyPixels12, uint32_t skyW, uint32_t skyH, const void* rays, uint32_t stride, const void* out48, const uint8_t* occOrNull,
                           uint64_t n, const float* lightDirOrNull, void* rgb16) {
    if (int r = checkMode("tbvh_host_viewer_light", mode)) return r;
    if (int r = checkSkyHost("tbvh_host_viewer_light", skyPixels12, skyW, skyH)) return r;
    if (int r = checkRecords("tbvh_host_viewer_light", rays, stride, n)) return r;
    if (n && (!out48 || !rgb16)) return fail(TBVH_E_INVALID, "tbvh_host_viewer_light: null shading records or output");
    if (((uintptr_t)out48 | (uintptr_t)rgb16) & 15) return fail(TBVH_E_INVALID, "tbvh_host_viewer_light: shading records and output must be 16-byte aligned");
    float Lf[3];
    lightDir(lightDirOrNull, Lf);
    const ShadeV3 L = {Lf[0], Lf[1], Lf[2]};
    const ViewerSky sky{skyPixels12, skyW, skyH};
    for (uint64_t i = 0; i < n; i++) {
        const float4* rec = (const float4*)((const char*)rays + i * stride);
        const float4* o = (const float4*)out48 + 3 * i;
        const bool shaded = mode == kViewerFoliage && occOrNull && rec[3].x < 10000.f && occOrNull[i] != 0;
        const ShadeV3 c = vw_light(mode, sky, rec[1], rec[3], o[0], o[2], shaded, L);
        ((float4*)rgb16)[i] = make_float4(c.x, c.y, c.z, 0.f);
    }
    return 0;
}

int tbvh_host_viewer_pack(const void* rgb16, uint64_t n, uint32_t* pixels) {
    if (n && (!rgb16 || !pixels)) return fail(TBVH_E_INVALID, "tbvh_host_viewer_pack: null colours or pixels");
    if (((uintptr_t)rgb16 & 15) || ((uintptr_t)pixels & 3)) return fail(TBVH_E_INVALID, "tbvh_host_viewer_pack: misaligned colours (16 bytes) or pixels (4)");
    for (uint64_t i = 0; i < n; i++) {
        const float4 c = ((const float4*)rgb16)[i];
        pixels[i] = vw_pack(c.x, c.y, c.z);
    }
    return 0;
}

int tbvh_debug_viewer_math(int kind, const float* a, const float* b, uint64_t n, float* out) {
    if (kind < 0 || kind > 1 || (n && (!a || !out || (kind == 0 && !b)))) return fail(TBVH_E_INVALID, "tbvh_debug_viewer_math: kind %d, null array", kind);
    for (uint64_t i = 0; i < n; i++) out[i] = kind == 0 ? vw_atan2f(a[i], b[i]) : vw_acosf(a[i]);
    return 0;
}

}  // extern "C"
