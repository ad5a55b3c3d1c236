// capi_shade.hip — hits resolved to shading data on the device (tbvh_shading_* / tbvh_shade_hits; include/tinybvh_amd.h, DESIGN.md par. 16): GetShadingData
// of tiny_bvh_foliage.cpp.  A tbvh_shading owns device copies of the materials, the texture descriptors (and of the texels when they came from the
// host) and, per BLAS slot, of the FatTri records, taken verbatim.  Host-resident input is range-checked before anything is allocated; device-resident
// input is checked by the kernel (kernels_shade.hip), index by index, before use.  tbvh_shade_hits_device launches the kernel on the context's stream;
// tbvh_shade_hits stages host records around it; tbvh_host_shade_hits is shade.h compiled for the host and needs no context.
#include "capi_internal.h"
#include "shade.h"

#include <stddef.h>

using namespace tbvh;
using namespace tbvh_capi;

// tinyscene::FatTri, the fields this file and shade.h name (192 bytes; the rest is carried along)
struct FatTriCheck {
    float u0, u1, u2; int32_t ltriIdx;
    float v0, v1, v2; uint32_t material;
    float vN0[3], Nx, vN1[3], Ny, vN2[3], Nz;
    float vertex0[3], u0_2, vertex1[3], u1_2, vertex2[3], u2_2;
    float T[3], area, B[3], invArea;
    float alpha[3], LOD, v0_2, v1_2, v2_2, dummy4;
};
static_assert(sizeof(FatTriCheck) == 192 && sizeof(FatTriCheck) == kFatTriQuads * 16, "FatTri is 192 bytes");
static_assert(offsetof(FatTriCheck, u0) == 0 && offsetof(FatTriCheck, v0) == 16 && offsetof(FatTriCheck, material) == 28, "FatTri: q0 = u0 u1 u2 ., q1 = v0 v1 v2 material");
static_assert(offsetof(FatTriCheck, vN0) == 32 && offsetof(FatTriCheck, Nx) == 44 && offsetof(FatTriCheck, vN1) == 48 && offsetof(FatTriCheck, Ny) == 60 &&
              offsetof(FatTriCheck, vN2) == 64 && offsetof(FatTriCheck, Nz) == 76, "FatTri: q2..q4 = vN0 Nx, vN1 Ny, vN2 Nz");
static_assert(offsetof(FatTriCheck, vertex0) == 80 && offsetof(FatTriCheck, vertex1) == 96 && offsetof(FatTriCheck, vertex2) == 112, "FatTri: q5..q7 = the vertices");
static_assert(offsetof(FatTriCheck, T) == 128 && offsetof(FatTriCheck, B) == 144, "FatTri: q8 = T area, q9 = B invArea");
static_assert(offsetof(BLASInstanceCheck, blasIdx) == 35 * 4, "BLASInstance: transform rows in float4 0..3, blasIdx at dword 35");
static_assert(sizeof(ShadeMat) == sizeof(tbvh_material) && offsetof(ShadeMat, colorTex) == offsetof(tbvh_material, color_texture) &&
              offsetof(ShadeMat, normalTex) == offsetof(tbvh_material, normal_texture), "ShadeMat is tbvh_material");
static_assert(sizeof(ShadeTex) == sizeof(tbvh_alpha_texture) && offsetof(ShadeTex, width) == offsetof(tbvh_alpha_texture, width), "ShadeTex is tbvh_alpha_texture");
static_assert(kShadeNoTexture == TBVH_OMM_NO_TEXTURE && kShadeLayoutSphere == TBVH_LAYOUT_BVH2_WALD && kShadeLayoutVoxel == TBVH_LAYOUT_VOXELSET, "shade.h and the public header agree");
static_assert(sizeof(BlasDesc) % 4 == 0 && offsetof(BlasDesc, layout) % 4 == 0, "the BLAS layouts are read as dwords a fixed stride apart");

struct tbvh_shading {
    tbvh_context* ctx = nullptr;
    uint32_t nMats = 0, nTex = 0;
    bool anyColorTex = false;                // some material may name a colour texture (device-resident materials: there are textures at all)
    DevBuf<ShadeMat> mats;
    DevBuf<ShadeTex> tex;                    // the descriptors, their texel pointers on the device
    std::vector<DevBuf<uint32_t>> texels;    // the texels that came from the host (device-resident ones stay the caller's)
    std::vector<DevBuf<float4>> tris;        // per BLAS slot: 12 float4 per FatTri
    std::vector<ShadeSlot> slots;            // what slotsDev holds
    DevBuf<ShadeSlot> slotsDev;
    ShadeTables tables() const { return ShadeTables{slotsDev.get(), mats.get(), tex.get(), (uint32_t)slots.size(), nMats, nTex}; }
};

namespace {

int allocFail(const char* who, uint64_t bytes) {
    (void)hipGetLastError();
    return fail(TBVH_E_NOMEM, "%s: %llu bytes of device memory", who, (unsigned long long)bytes);
}

// the rules of the header for the two descriptor arrays; host-resident materials are range-checked too
int checkTables(const char* who, const tbvh_material* materials, uint32_t nMats, const tbvh_alpha_texture* textures, uint32_t nTex, bool matsOnHost, uintptr_t texelAlign) {
    if (!materials || nMats == 0) return fail(TBVH_E_INVALID, "%s: no materials", who);
    if ((uintptr_t)materials & 3) return fail(TBVH_E_INVALID, "%s: misaligned material array (4 bytes)", who);
    if (nTex && !textures) return fail(TBVH_E_INVALID, "%s: %u textures, null descriptor array", who, nTex);
    for (uint32_t k = 0; k < nTex; k++) {
        const tbvh_alpha_texture& t = textures[k];
        if (!t.texels || ((uintptr_t)t.texels & texelAlign)) return fail(TBVH_E_INVALID, "%s: texture %u: null or misaligned texels", who, k);
        if (t.width == 0 || t.height == 0 || (uint64_t)t.width * t.height >> 31) return fail(TBVH_E_INVALID, "%s: texture %u: %u x %u texels (1 .. 2^31 - 1 in all)", who, k, t.width, t.height);
    }
    if (matsOnHost)
        for (uint32_t k = 0; k < nMats; k++)
            for (uint32_t id : {materials[k].color_texture, materials[k].normal_texture})
                if (id != TBVH_OMM_NO_TEXTURE && id >= nTex) return fail(TBVH_E_FORMAT, "%s: material %u names texture %u (%u textures)", who, k, id, nTex);
    return 0;
}

// host-resident FatTri records: the first triangle whose material is not one
int checkFatTris(const char* who, uint32_t slot, const void* fatTris192, uint64_t nTris, uint32_t nMats) {
    const char* p = (const char*)fatTris192;
    for (uint64_t i = 0; i < nTris; i++) {
        uint32_t m;
        memcpy(&m, p + i * 192 + offsetof(FatTriCheck, material), 4);
        if (m >= nMats) return fail(TBVH_E_FORMAT, "%s: slot %u, triangle %llu: material %u (%u materials)", who, slot, (unsigned long long)i, m, nMats);
    }
    return 0;
}

int checkRays(const char* who, const void* rays, uint64_t n, uint32_t stride, const void* out48) {
    if (stride < 64 || (stride & 15)) return fail(TBVH_E_INVALID, "%s: a record stride of %u bytes (64 or more, a multiple of 16)", who, stride);
    if (n && (!rays || !out48)) return fail(TBVH_E_INVALID, "%s: null records or output", who);
    if (((uintptr_t)rays | (uintptr_t)out48) & 15) return fail(TBVH_E_INVALID, "%s: records and output must be 16-byte aligned", who);
    return 0;
}

void destroyShading(tbvh_shading* sh) { delete sh; }

}  // namespace

namespace tbvh_capi {
void freeShadingsOf(tbvh_context* c) {
    for (tbvh_shading* sh : c->shadings) { detachPosesFrom(c, sh); destroyShading(sh); }
    c->shadings.clear();
}
tbvh_context* shadingContext(const tbvh_shading* sh) { return sh->ctx; }
void shadingSlotRecords(const tbvh_shading* sh, uint32_t slot, float4** tris, uint64_t* nTris) {
    const bool has = slot < sh->slots.size() && sh->slots[slot].tris;
    *tris = has ? sh->tris[slot].get() : nullptr;
    *nTris = has ? sh->slots[slot].nTris : 0;
}
void shadingLaunch(const tbvh_shading* sh, tbvh_scene* s, const void* dRays, uint64_t n, uint32_t strideBytes, void* dOut48, const unsigned long long* nDev) {
    tbvh_context* c = sh->ctx;
    if (s->isTlas)
        launch_shade_hits(sh->tables(), s->tlas.instances, s->tlas.nInst, (const uint32_t*)((const char*)s->tlas.blasDesc.get() + offsetof(BlasDesc, layout)), sizeof(BlasDesc) / 4,
                          (uint32_t)s->tlas.nBlas, dRays, n, strideBytes, dOut48, c->status, c->stream, nDev);
    else
        launch_shade_hits(sh->tables(), nullptr, 0, nullptr, 0, 0, dRays, n, strideBytes, dOut48, c->status, c->stream, nDev);
}
void shadingMaterials(const tbvh_shading* sh, const ShadeMat** mats, uint32_t* nMats, uint32_t* nTex, bool* anyColorTexture) {
    *mats = sh->mats.get(); *nMats = sh->nMats; *nTex = sh->nTex; *anyColorTexture = sh->anyColorTex;
}
}  // namespace tbvh_capi

extern "C" {

int tbvh_shading_create(tbvh_context* c, const tbvh_material* materials, uint32_t nMats, const tbvh_alpha_texture* textures, uint32_t nTex, int onDevice, tbvh_shading** out) {
    if (!c || !out) return fail(TBVH_E_INVALID, "tbvh_shading_create: null argument");
    if (int r = checkTables("tbvh_shading_create", materials, nMats, textures, nTex, !onDevice, 3)) return r;
    TBVH_ENTER(c);
    tbvh_shading* sh = new (std::nothrow) tbvh_shading;
    if (!sh) return fail(TBVH_E_NOMEM, "tbvh_shading_create: out of host memory");
    sh->ctx = c; sh->nMats = nMats; sh->nTex = nTex;
    sh->anyColorTex = onDevice && nTex;
    if (!onDevice)
        for (uint32_t k = 0; k < nMats; k++) sh->anyColorTex |= materials[k].color_texture != TBVH_OMM_NO_TEXTURE;
    std::vector<ShadeTex> desc(nTex);
    int r = 0;
    if (sh->mats.alloc(nMats) != hipSuccess || (nTex && sh->tex.alloc(nTex) != hipSuccess)) r = allocFail("tbvh_shading_create", nMats * sizeof(ShadeMat) + nTex * sizeof(ShadeTex));
    if (!r && !onDevice) sh->texels.resize(nTex);
    for (uint32_t k = 0; k < nTex && !r; k++) {
        desc[k] = ShadeTex{textures[k].texels, textures[k].width, textures[k].height};
        if (onDevice) continue;
        const uint64_t n = (uint64_t)desc[k].width * desc[k].height;
        if (sh->texels[k].alloc(n) != hipSuccess) { r = allocFail("tbvh_shading_create", n * 4); break; }
        if (hipMemcpyAsync(sh->texels[k], desc[k].texels, n * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess) r = fail(TBVH_E_HIP, "tbvh_shading_create: copying texture %u failed: %s", k, hipGetErrorString(hipGetLastError()));
        desc[k].texels = sh->texels[k];
    }
    if (!r && (hipMemcpyAsync(sh->mats, materials, nMats * sizeof(ShadeMat), onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream) != hipSuccess ||
               (nTex && hipMemcpyAsync(sh->tex, desc.data(), nTex * sizeof(ShadeTex), hipMemcpyHostToDevice, c->stream) != hipSuccess)))
        r = fail(TBVH_E_HIP, "tbvh_shading_create: copying the tables failed: %s", hipGetErrorString(hipGetLastError()));
    const hipError_t e = hipStreamSynchronize(c->stream);   // (the caller's arrays and `desc` are free from here on; also after a failure half-way)
    if (!r && e != hipSuccess) r = fail(TBVH_E_HIP, "tbvh_shading_create: %s", hipGetErrorString(e));
    if (r) { destroyShading(sh); return r; }
    c->shadings.push_back(sh);
    *out = sh;
    return 0;
}

int tbvh_shading_set_fat_tris(tbvh_shading* sh, uint32_t slot, const void* fatTris192, uint64_t nTris, int onDevice) {
    if (!sh || !fatTris192) return fail(TBVH_E_INVALID, "tbvh_shading_set_fat_tris: null argument");
    if (nTris == 0 || nTris >> 32) return fail(TBVH_E_INVALID, "tbvh_shading_set_fat_tris: %llu triangles", (unsigned long long)nTris);
    if (slot >= (1u << 24)) return fail(TBVH_E_INVALID, "tbvh_shading_set_fat_tris: BLAS slot %u (below 2^24)", slot);
    if ((uintptr_t)fatTris192 & (onDevice ? 15 : 3)) return fail(TBVH_E_INVALID, "tbvh_shading_set_fat_tris: misaligned records (device: 16 bytes, host: 4)");
    if (!onDevice)
        if (int r = checkFatTris("tbvh_shading_set_fat_tris", slot, fatTris192, nTris, sh->nMats)) return r;
    tbvh_context* c = sh->ctx;
    TBVH_ENTER(c);
    // the new records and a NEW slot table are complete before anything is swapped: a failure leaves the table, on the host and on the device, as it was
    DevBuf<float4> fresh;
    if (fresh.alloc(nTris * kFatTriQuads) != hipSuccess) return allocFail("tbvh_shading_set_fat_tris", nTris * 192);
    std::vector<ShadeSlot> slots = sh->slots;
    if (slot >= slots.size()) slots.resize(slot + 1, ShadeSlot{nullptr, 0});
    slots[slot] = ShadeSlot{fresh.get(), nTris};
    DevBuf<ShadeSlot> table;
    if (table.alloc(slots.size()) != hipSuccess) return allocFail("tbvh_shading_set_fat_tris", slots.size() * sizeof(ShadeSlot));
    HIP_TRY(hipMemcpyAsync(fresh, fatTris192, nTris * 192, onDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(table, slots.data(), slots.size() * sizeof(ShadeSlot), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (also: the kernels in flight that read the old table and the old records are done)
    sh->slotsDev = std::move(table);            // (the old table and the slot's previous records go)
    if (slot >= sh->tris.size()) sh->tris.resize(slot + 1);
    sh->tris[slot] = std::move(fresh);
    sh->slots.swap(slots);
    return 0;
}

int tbvh_shading_fat_tris(tbvh_shading* sh, uint32_t slot, void** dFatTris192, uint64_t* nTris) {
    if (!sh || !dFatTris192) return fail(TBVH_E_INVALID, "tbvh_shading_fat_tris: null argument");
    TBVH_LOCK(sh->ctx);
    if (slot >= sh->slots.size() || !sh->slots[slot].tris) return fail(TBVH_E_INVALID, "tbvh_shading_fat_tris: slot %u has no records", slot);
    *dFatTris192 = sh->tris[slot].get();
    if (nTris) *nTris = sh->slots[slot].nTris;
    return 0;
}

int tbvh_shading_download_fat_tris(tbvh_shading* sh, uint32_t slot, void* dst192, uint64_t capTris) {
    if (!sh || !dst192) return fail(TBVH_E_INVALID, "tbvh_shading_download_fat_tris: null argument");
    tbvh_context* c = sh->ctx;
    TBVH_ENTER(c);
    if (slot >= sh->slots.size() || !sh->slots[slot].tris) return fail(TBVH_E_INVALID, "tbvh_shading_download_fat_tris: slot %u has no records", slot);
    const uint64_t n = sh->slots[slot].nTris;
    if (capTris < n) return fail(TBVH_E_INVALID, "tbvh_shading_download_fat_tris: room for %llu triangles, the slot has %llu", (unsigned long long)capTris, (unsigned long long)n);
    HIP_TRY(hipMemcpyAsync(dst192, sh->tris[slot], n * 192, hipMemcpyDeviceToHost, c->stream));
    return checkStatus(c);   // (synchronizes)
}

void tbvh_shading_free(tbvh_shading* sh) {
    if (!sh) return;
    tbvh_context* c = sh->ctx;
    TBVH_LOCK(c);
    (void)tbvh_capi::setDevice(c);   // (joins the launch lanes)
    hipStreamSynchronize(c->stream);   // (kernels in flight read the tables)
    for (size_t i = 0; i < c->shadings.size(); i++)
        if (c->shadings[i] == sh) { c->shadings.erase(c->shadings.begin() + i); break; }
    detachPosesFrom(c, sh);
    destroyShading(sh);
}

int tbvh_shade_hits_device(tbvh_shading* sh, tbvh_scene* s, const void* dRays, uint64_t n, uint32_t strideBytes, void* dOut48) {
    if (!sh || !s) return fail(TBVH_E_INVALID, "tbvh_shade_hits_device: null argument");
    TBVH_REFUSE_DOUBLE(s, "tbvh_shade_hits_device");
    TBVH_REFUSE_VOXEL(s, "tbvh_shade_hits_device");
    TBVH_REFUSE_CUSTOM(s, "tbvh_shade_hits_device");
    if (s->ctx != sh->ctx) return fail(TBVH_E_INVALID, "tbvh_shade_hits_device: the shading table and the scene belong to different contexts");
    if (int r = checkRays("tbvh_shade_hits_device", dRays, n, strideBytes, dOut48)) return r;
    tbvh_context* c = sh->ctx;
    TBVH_ENTER(c);
    if (!n) return 0;
    HIP_TRY(timedBegin(c));
    shadingLaunch(sh, s, dRays, n, strideBytes, dOut48, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    return 0;
}

int tbvh_shade_hits(tbvh_shading* sh, tbvh_scene* s, const void* rays, uint64_t n, uint32_t strideBytes, void* out48) {
    if (!sh || !s) return fail(TBVH_E_INVALID, "tbvh_shade_hits: null argument");
    if (strideBytes < 64 || (strideBytes & 3)) return fail(TBVH_E_INVALID, "tbvh_shade_hits: a record stride of %u bytes (64 or more, a multiple of 4)", strideBytes);
    if (n && (!rays || !out48)) return fail(TBVH_E_INVALID, "tbvh_shade_hits: null records or output");
    if (((uintptr_t)rays | (uintptr_t)out48) & 3) return fail(TBVH_E_INVALID, "tbvh_shade_hits: misaligned records or output (4 bytes)");
    tbvh_context* c = sh->ctx;
    TBVH_ENTER(c);
    if (!n) return 0;
    // the 64-byte prefixes go up packed, the 48-byte records come back; both staging areas live for the call
    DevBuf<void> dRays, dOut;
    if (dRays.alloc(n * 64) != hipSuccess || dOut.alloc(n * 48) != hipSuccess) return allocFail("tbvh_shade_hits", n * 112);
    HIP_TRY(hipMemcpy2DAsync(dRays, 64, rays, strideBytes, 64, n, hipMemcpyHostToDevice, c->stream));
    int r = tbvh_shade_hits_device(sh, s, dRays, n, 64, dOut);
    if (!r && hipMemcpyAsync(out48, dOut, n * 48, hipMemcpyDeviceToHost, c->stream) != hipSuccess) r = fail(TBVH_E_HIP, "tbvh_shade_hits: copying the records back failed: %s", hipGetErrorString(hipGetLastError()));
    const int st = checkStatus(c);   // (synchronizes: the staging areas may go)
    return r ? r : st;
}

int tbvh_shade_continue_device(tbvh_context* c, void* dRays, uint32_t strideBytes, const void* dOut48, uint64_t n, unsigned long long* dContinued) {
    if (!c) return fail(TBVH_E_INVALID, "tbvh_shade_continue_device: null context");
    if (int r = checkRays("tbvh_shade_continue_device", dRays, n, strideBytes, dOut48)) return r;
    if ((uintptr_t)dContinued & 7) return fail(TBVH_E_INVALID, "tbvh_shade_continue_device: misaligned counter (8 bytes)");
    TBVH_ENTER(c);
    launch_shade_continue(dRays, strideBytes, dOut48, n, dContinued, c->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int tbvh_host_shade_hits(const tbvh_material* materials, uint32_t nMats, const tbvh_alpha_texture* textures, uint32_t nTex, const void* const* fatTris192,
                         const uint64_t* nTris, uint32_t nSlots, const void* instances192, uint64_t nInst, const void* rays, uint64_t n, uint32_t strideBytes,
                         void* out48) {
    if (int r = checkTables("tbvh_host_shade_hits", materials, nMats, textures, nTex, true, 3)) return r;
    if (!fatTris192 || !nTris || nSlots == 0) return fail(TBVH_E_INVALID, "tbvh_host_shade_hits: no BLAS slots");
    if (int r = checkRays("tbvh_host_shade_hits", rays, n, strideBytes, out48)) return r;
    if ((uintptr_t)instances192 & 15) return fail(TBVH_E_INVALID, "tbvh_host_shade_hits: misaligned instance records (16 bytes)");
    if (instances192 && nInst == 0) return fail(TBVH_E_INVALID, "tbvh_host_shade_hits: an instance array without instances");
    std::vector<ShadeSlot> slots(nSlots);
    for (uint32_t k = 0; k < nSlots; k++) {
        if (!fatTris192[k] != !nTris[k] || nTris[k] >> 32) return fail(TBVH_E_INVALID, "tbvh_host_shade_hits: slot %u: %llu triangles at %p", k, (unsigned long long)nTris[k], fatTris192[k]);
        if ((uintptr_t)fatTris192[k] & 15) return fail(TBVH_E_INVALID, "tbvh_host_shade_hits: slot %u: misaligned records (16 bytes)", k);
        if (int r = checkFatTris("tbvh_host_shade_hits", k, fatTris192[k], nTris[k], nMats)) return r;
        slots[k] = ShadeSlot{(const float4*)fatTris192[k], nTris[k]};
    }
    const ShadeTables tb{slots.data(), (const ShadeMat*)materials, (const ShadeTex*)textures, nSlots, nMats, nTex};
    bool ok = true;
    for (uint64_t i = 0; i < n; i++) {
        const float4* rec = (const float4*)((const char*)rays + i * strideBytes);
        uint32_t inst;
        memcpy(&inst, &rec[2].w, 4);
        ok &= shade_hit(tb, (const float4*)instances192, nInst, nullptr, 0, 0, rec[1], inst, rec[3], (float4*)out48 + 3 * i);
    }
    return ok ? 0 : fail(TBVH_E_FORMAT, "tbvh_host_shade_hits: a hit record's instance, BLAS slot or primitive is out of range (the record got no surface)");
}

}  // extern "C"
