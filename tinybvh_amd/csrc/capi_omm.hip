// capi_omm.hip — opacity micromaps baked from alpha textures on the device (tbvh_bake_opacity_micromaps / tbvh_bake_set_opacity_micromaps;
// include/tinybvh_amd.h, DESIGN.md par. 15): Mesh::CreateOpacityMicroMaps of tiny_scene.h.  A source is validated (omm_host.cpp: omm_check_source — host arrays
// are range-checked before anything is allocated), host-resident arrays are copied into allocations that live for the call, the texture descriptors go
// up in stream order through the context's pinned area, and the kernel of kernels_omm.hip writes the words.  The fused call bakes into the buffer the
// scene then owns (capi_scene.hip: allocOpacityMaps / installOpacityMaps).  The host variant (the same header on the CPU) is in omm_host.cpp.
#include "capi_internal.h"
#include "omm.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace {

// a source as the kernel sees it: device-resident arrays are used in place, host arrays are copied into allocations this object owns (asynchronous on
// the context's stream: synchronise before the caller's arrays may change and before this object goes)
struct DeviceOmmSource {
    OmmSrc src;
    DevBuf<void> uv;
    DevBuf<uint32_t> indices, triTexture;
    std::vector<DevBuf<uint32_t>> texels;
};

int upload(tbvh_context* c, const char* who, DevBuf<uint32_t>& dst, const uint32_t* src, uint64_t n) {
    if (dst.alloc(n) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: %llu bytes of device memory", who, (unsigned long long)(n * 4)); }
    HIP_TRY(hipMemcpyAsync(dst, src, n * 4, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// the descriptor array on the device, in stream order behind whatever still reads the previous one
int sendDescriptors(tbvh_context* c, const char* who, const std::vector<OmmTex>& desc, const OmmTex** dDesc) {
    const size_t bytes = desc.size() * sizeof(OmmTex);
    *dDesc = nullptr;
    if (!bytes) return 0;
    if (c->ommPinUsed) HIP_TRY(hipEventSynchronize(c->ommEv));   // the previous bake's copy has left the pinned area
    if (bytes > c->ommPinBytes) {
        if (c->ommPin) hipHostFree(c->ommPin);
        c->ommPin = nullptr; c->ommPinBytes = 0; c->ommPinUsed = false;
        if (hipHostMalloc(&c->ommPin, bytes) != hipSuccess) { (void)hipGetLastError(); c->ommPin = nullptr; return fail(TBVH_E_NOMEM, "%s: %llu bytes of pinned host memory", who, (unsigned long long)bytes); }
        c->ommPinBytes = bytes;
    }
    if (!c->ommEv) HIP_TRY(hipEventCreateWithFlags(&c->ommEv, hipEventDisableTiming));
    // (growing frees the old array: hipFree waits for the kernels that read it)
    if (c->ommDesc.reserve(bytes) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: %llu bytes of device memory", who, (unsigned long long)bytes); }
    memcpy(c->ommPin, desc.data(), bytes);
    HIP_TRY(hipMemcpyAsync(c->ommDesc, c->ommPin, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->ommEv, c->stream));
    c->ommPinUsed = true;
    *dDesc = (const OmmTex*)c->ommDesc.get();
    return 0;
}

// a validated source -> the kernel's; the launch, timed.  Asynchronous: the caller synchronises before `dev` goes when the source was host-resident.
int bakeChecked(tbvh_context* c, const char* who, const tbvh_omm_source* src, uint32_t N, uint32_t* dOut, DeviceOmmSource& dev) {
    std::vector<OmmTex> desc(src->n_textures);
    for (uint32_t k = 0; k < src->n_textures; k++) desc[k] = OmmTex{src->textures[k].texels, src->textures[k].width, src->textures[k].height};
    OmmSrc& s = dev.src;
    s = OmmSrc{(const char*)src->uv, src->uv_stride_bytes, (uint32_t)src->n_uv, src->indices, src->tri_texture, nullptr, src->n_textures, src->n_tris};
    if (!src->on_device) {
        const uint64_t uvBytes = (src->n_uv - 1) * src->uv_stride_bytes + 8;   // (the last UV: two floats, whatever the stride)
        if (dev.uv.alloc(uvBytes) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: %llu bytes of device memory", who, (unsigned long long)uvBytes); }
        HIP_TRY(hipMemcpyAsync(dev.uv, src->uv, uvBytes, hipMemcpyHostToDevice, c->stream));
        s.uv = (const char*)dev.uv.get();
        if (src->indices) { if (int r = upload(c, who, dev.indices, src->indices, 3 * src->n_tris)) return r; s.indices = dev.indices; }
        if (src->tri_texture) { if (int r = upload(c, who, dev.triTexture, src->tri_texture, src->n_tris)) return r; s.triTexture = dev.triTexture; }
        dev.texels.resize(src->n_textures);
        for (uint32_t k = 0; k < src->n_textures; k++) {
            if (int r = upload(c, who, dev.texels[k], desc[k].texels, (uint64_t)desc[k].width * desc[k].height)) return r;
            desc[k].texels = dev.texels[k];
        }
    }
    if (int r = sendDescriptors(c, who, desc, &s.textures)) return r;
    HIP_TRY(timedBegin(c));
    launch_omm_bake(s, N, dOut, c->status, (uint32_t)c->numCUs * 32u, c->stream);   // (one-wave workgroups: 8 per SIMD fill a CU)
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    return 0;
}

}  // namespace

namespace tbvh_capi {
void freeOmmStagingOf(tbvh_context* c) {
    if (c->ommEv) hipEventDestroy(c->ommEv);
    if (c->ommPin) hipHostFree(c->ommPin);
    c->ommEv = nullptr; c->ommPin = nullptr; c->ommPinBytes = 0; c->ommPinUsed = false;
}
}  // namespace tbvh_capi

extern "C" {

int tbvh_bake_opacity_micromaps(tbvh_context* c, const tbvh_omm_source* src, uint32_t N, uint32_t* dMapsOut) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_bake_opacity_micromaps: null context");
    if (int r = omm_check_source(src, N, "tbvh_bake_opacity_micromaps", src && !src->on_device)) return r;
    if (!dMapsOut || ((uintptr_t)dMapsOut & 3)) return fail(TBVH_E_INVALID, "tbvh_bake_opacity_micromaps: null or misaligned output");
    TBVH_ENTER(c);
    DeviceOmmSource dev;
    int r = bakeChecked(c, "tbvh_bake_opacity_micromaps", src, N, dMapsOut, dev);
    if (!src->on_device) {   // the staged arrays go at return (also after a failure half-way: copies may be in flight)
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (!r && e != hipSuccess) r = fail(TBVH_E_HIP, "tbvh_bake_opacity_micromaps: %s", hipGetErrorString(e));
    }
    return r;
}

int tbvh_bake_set_opacity_micromaps(tbvh_scene* s, const tbvh_omm_source* src, uint32_t N) {
    TBVH_REFUSE_DOUBLE(s, "tbvh_bake_set_opacity_micromaps");
    TBVH_REFUSE_VOXEL(s, "tbvh_bake_set_opacity_micromaps");
    TBVH_REFUSE_CUSTOM(s, "tbvh_bake_set_opacity_micromaps");
    if (!s || s->isTlas) return fail(TBVH_E_INVALID, "tbvh_bake_set_opacity_micromaps: not a BLAS scene (set the maps on the BLASes before uploading their TLAS)");
    if (int r = omm_check_source(src, N, "tbvh_bake_set_opacity_micromaps", src && !src->on_device)) return r;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    // as tbvh_set_opacity_micromaps: the new maps are complete before they are swapped in, every failure leaves the scene on its old ones
    DevBuf<uint32_t> fresh;
    uint64_t words = 0;
    if (int r = allocOpacityMaps(c, N, src->n_tris, "tbvh_bake_set_opacity_micromaps", fresh, &words)) return r;
    DeviceOmmSource dev;
    int r = bakeChecked(c, "tbvh_bake_set_opacity_micromaps", src, N, fresh, dev);
    const int st = checkStatus(c);   // (synchronizes: the staged arrays may go, and a bad device-resident index is known)
    if (r || st) return r ? r : st;
    return installOpacityMaps(s, std::move(fresh), N);
}

}  // extern "C"
