// capi_custom.hip — custom-geometry sphere BLASes (BVH::Build( customGetAABB, n ), tiny_bvh.h:2190-2219, traced through the sphere callback of the
// reference's anim demo): upload with validation and the host builder behind tbvh_host_build_custom_spheres.  The kernels are kernels_custom.hip;
// queries reach them through launchQuery (capi_query.hip), TLASes over sphere BLASes through tbvh_upload_tlas (capi_scene.hip).
// Sphere sets that move: tbvh_build_device_custom_spheres / _sah / tbvh_rebuild_custom_spheres_device (the LBVH / PLOC builders of kernels_build.hip, or the SAH builder of kernels_sahbuild.hip, with the
// spheres as their box source, then the record gather) and tbvh_refit_custom_spheres (kernels_custom_build.hip); tbvh_custom_spheres_download reads a
// sphere scene back.
// A sphere scene (layout TBVH_LAYOUT_BVH2_WALD) keeps the Wald nodes as uploaded in `nodes` and the spheres gathered in primIdx order in `tris`
// (2 float4 per index entry: {x, y, z, r}, {prim, 0, 0, 0}); a TLAS's BlasDesc points at the two.  tbvh_free_scene frees them like any scene's.
#include "capi_internal.h"
#include "sahbuild.h"

using namespace tbvh;
using namespace tbvh_capi;

extern "C" {

int tbvh_upload_custom_spheres(tbvh_context* c, const void* nodes32, uint64_t nNodes, const uint32_t* primIdx, uint64_t nIdx, const void* spheres16,
                               uint64_t nSpheres, tbvh_scene** out) {
    if (!c || !nodes32 || !primIdx || !spheres16 || !out) return fail(TBVH_E_INVALID, "tbvh_upload_custom_spheres: null argument");
    if (!nNodes || !nIdx || !nSpheres) return fail(TBVH_E_INVALID, "tbvh_upload_custom_spheres: empty argument");
    // device offsets are 32-bit: node indices (a child pair leftFirst + 1 included), index entries, primitive numbers
    if (nNodes > 0xFFFFFFFFull || nIdx > 0xFFFFFFFFull || nSpheres > 0x100000000ull)
        return fail(TBVH_E_FORMAT, "tbvh_upload_custom_spheres: %llu nodes, %llu indices, %llu spheres: beyond the 32-bit device offsets",
                    (unsigned long long)nNodes, (unsigned long long)nIdx, (unsigned long long)nSpheres);
    if (const char* why = validate_bvh2((const Node2*)nodes32, nNodes, primIdx, nIdx, nSpheres))
        return fail(why == kValidateNoMemory ? TBVH_E_NOMEM : TBVH_E_FORMAT, "tbvh_upload_custom_spheres: %s", why);
    std::vector<Vec4> recs;
    try { recs.resize(nIdx * 2); } catch (const std::bad_alloc&) { return fail(TBVH_E_NOMEM, "out of host memory"); }
    const Vec4* sph = (const Vec4*)spheres16;
    for (uint64_t k = 0; k < nIdx; k++) {   // gathered in leaf order, with the primitive index (as BVH_GPU triangles are gathered)
        recs[2 * k] = sph[primIdx[k]];
        Vec4 p{0.f, 0.f, 0.f, 0.f};
        std::memcpy(&p.x, &primIdx[k], 4);
        recs[2 * k + 1] = p;
    }
    TBVH_ENTER(c);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH2_WALD);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    if (s->nodes.alloc(nNodes * 2) != hipSuccess || s->tris.alloc(nIdx * 2) != hipSuccess) {
        tbvh_free_scene(s);
        return fail(TBVH_E_NOMEM, "tbvh_upload_custom_spheres: out of device memory");
    }
    if (hipMemcpyAsync(s->nodes, nodes32, nNodes * 32, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(s->tris, recs.data(), nIdx * 32, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
        tbvh_free_scene(s);
        return fail(TBVH_E_HIP, "tbvh_upload_custom_spheres: copy to the device failed");
    }
    s->nNodes = (uint32_t)nNodes;
    s->nNodeBlocks = nNodes * 2; s->nTriBlocks = nIdx * 2;
    s->sphN = nSpheres;
    *out = s;
    return 0;
}

int tbvh_host_build_custom_spheres(const void* spheres16, uint64_t n, tbvh_hostbvh** out) {
    if (!spheres16 || !out || !n) return fail(TBVH_E_INVALID, "tbvh_host_build_custom_spheres: null/empty argument");
    if (n > 0x7FFFFFFFull) return fail(TBVH_E_INVALID, "tbvh_host_build_custom_spheres: %llu spheres: at most 2^31 - 1", (unsigned long long)n);
    const Vec4* sph = (const Vec4*)spheres16;
    tbvh_hostbvh* h = new (std::nothrow) tbvh_hostbvh;
    if (!h) return fail(TBVH_E_NOMEM, "out of host memory");
    h->layout = TBVH_LAYOUT_BVH2_WALD;
    try {
        std::vector<float> boxes(n * 6);
        for (uint64_t i = 0; i < n; i++) {   // the demos' sphereAABB: pos - bvhvec3( r ), pos + bvhvec3( r )
            const Vec4& p = sph[i];
            float* b = boxes.data() + i * 6;
            b[0] = p.x - p.w; b[1] = p.y - p.w; b[2] = p.z - p.w;
            b[3] = p.x + p.w; b[4] = p.y + p.w; b[5] = p.z + p.w;
        }
        BuildParams bp;
        build_bvh2_boxes(boxes.data(), (uint32_t)n, bp, h->bvh2);
    } catch (const std::bad_alloc&) {
        delete h;
        return fail(TBVH_E_NOMEM, "out of host memory while building");
    }
    *out = h;
    return 0;
}

}  // extern "C"

namespace {

// the refusals the calls on an existing sphere scene share; 0: s is a sphere BLAS and spheres16 / n are usable
int checkMovingSpheres(const char* who, const tbvh_scene* s, const void* spheres16, uint64_t n) {
    if (!s || !spheres16) return fail(TBVH_E_INVALID, "%s: null argument", who);
    if (s->isTlas || s->layout != TBVH_LAYOUT_BVH2_WALD) return fail(TBVH_E_INVALID, "%s: not a sphere BLAS (layout %d)", who, s->layout);
    if (n != s->sphN) return fail(TBVH_E_INVALID, "%s: %llu spheres, the scene holds %llu", who, (unsigned long long)n, (unsigned long long)s->sphN);
    return 0;
}

// the caller's spheres on the device: where they are, or staged in the scene (asynchronous, as tbvh_refit stages vertices)
int stageSpheres(tbvh_scene* s, const char* who, const void* spheres16, uint64_t n, int onDevice, const float4** out) {
    *out = (const float4*)spheres16;
    if (onDevice) return 0;
    if (s->vertStage.reserve(n * 16) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: out of device memory (staging %llu spheres)", who, (unsigned long long)n); }
    if (hipMemcpyAsync(s->vertStage, spheres16, n * 16, hipMemcpyHostToDevice, s->ctx->stream) != hipSuccess) return fail(TBVH_E_HIP, "%s: copy to the device failed", who);
    *out = (const float4*)s->vertStage.get();
    return 0;
}

// A new tree over dSph (device, n spheres) in scene s with the builder s remembers, and the records gathered: one timed operation.  The scene's
// arrays hold 2n nodes and n records; an uploaded scene's smaller ones are replaced once, and the TLASes over it re-pointed (reclassifyTlas)
// BEFORE anything is built, so that no descriptor is ever left on freed memory.
int buildSphereTree(tbvh_scene* s, const char* who, const float4* dSph, uint64_t n) {
    tbvh_context* c = s->ctx;
    const uint64_t nNodes = n > 1 ? 2 * n : 2;   // root, the unused node 1, the n - 1 child pairs
    if (s->buildScratchFor != n || !s->buildScratch) {
        s->buildScratchFor = 0;
        const size_t bytes = s->sphBuilder == 2   ? sah_scratch_bytes((uint32_t)n, &s->sortTempBytes, &s->scanTempBytes)
                             : s->sphBuilder == 1 ? ploc_scratch_bytes((uint32_t)n, &s->sortTempBytes, &s->scanTempBytes)
                                                  : lbvh_scratch_bytes((uint32_t)n, &s->sortTempBytes);
        if (s->buildScratch.alloc(bytes) != hipSuccess || s->sphIdx.reserve(n) != hipSuccess) {
            (void)hipGetLastError();
            return fail(TBVH_E_NOMEM, "%s: out of device memory (%llu bytes of build scratch)", who, (unsigned long long)bytes);
        }
        s->buildScratchFor = n;
    }
    if (s->nodes.count() < nNodes * 2 || s->tris.count() < n * 2) {
        DevBuf<float4> nodes, recs;
        if (nodes.alloc(nNodes * 2) != hipSuccess || recs.alloc(n * 2) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "%s: out of device memory (%llu spheres)", who, (unsigned long long)n); }
        HIP_TRY(hipStreamSynchronize(c->stream));   // (queries in flight read the old arrays)
        DevBuf<float4> oldNodes = std::move(s->nodes), oldRecs = std::move(s->tris);
        s->nodes = std::move(nodes); s->tris = std::move(recs);
        int r = 0;
        for (size_t i = 0; i < s->usedBy.size() && !r; i++) {
            bool seen = false;
            for (size_t k = 0; k < i; k++) seen |= s->usedBy[k] == s->usedBy[i];
            if (!seen) r = reclassifyTlas(s->usedBy[i]);
        }
        if (r) { (void)oldNodes.release(); (void)oldRecs.release(); return r; }   // (a descriptor may still point at the old arrays: leak them rather than dangle)
    }
    uint32_t built = (uint32_t)nNodes;
    HIP_TRY(timedBegin(c));
    // builder 2: the reference's BVH::Build( customGetAABB, n ) with the sphereAABB callback (kernels_sahbuild.hip over sphere boxes); the tree has as many
    // nodes as the SAH loop made (at most 2 n), leaves of any size unless sphMaxLeaf cuts them (SplitLeafs)
    if (s->sphBuilder == 2)
        HIP_TRY(run_sah_build(SahSrc(sah_boxes_spheres(dSph)), (uint32_t)n, s->sphMaxLeaf, c->sahSmallSubtree, c->sahOneGroup, s->nodes, s->sphIdx, s->buildScratch,
                              s->sortTempBytes, s->scanTempBytes, c->status, c->stream, &built));
    else if (s->sphBuilder == 1) HIP_TRY(launch_ploc_build(MeshSrc{}, (uint32_t)n, s->sphRadius, s->nodes, s->sphIdx, s->buildScratch, s->sortTempBytes, s->scanTempBytes, c->stream, nullptr, dSph));
    else HIP_TRY(launch_lbvh_build(MeshSrc{}, (uint32_t)n, s->sphMaxLeaf, s->nodes, s->sphIdx, s->buildScratch, s->sortTempBytes, c->stream, dSph));
    launch_gather_sphere_records(s->sphIdx, dSph, s->tris, (uint32_t)n, c->stream);
    HIP_TRY(timedEnd(c));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (the caller's spheres may change; a launch error surfaces here)
    s->nNodes = built;
    s->nNodeBlocks = (uint64_t)built * 2; s->nTriBlocks = n * 2;
    return 0;
}

}  // namespace

extern "C" {

int tbvh_build_device_custom_spheres(tbvh_context* c, const void* spheres16, uint64_t n, int onDevice, int builder, uint32_t maxLeaf, uint32_t radius,
                                     tbvh_scene** out) {
    if (!c || !spheres16 || !out || !n) return fail(TBVH_E_INVALID, "tbvh_build_device_custom_spheres: null/empty argument");
    if (n > 0x7FFFFFFFull) return fail(TBVH_E_INVALID, "tbvh_build_device_custom_spheres: %llu spheres: at most 2^31 - 1", (unsigned long long)n);
    if (builder != 0 && builder != 1) return fail(TBVH_E_INVALID, "tbvh_build_device_custom_spheres: builder %d (0 = LBVH, 1 = PLOC)", builder);
    if (maxLeaf > 4u) return fail(TBVH_E_INVALID, "tbvh_build_device_custom_spheres: %u spheres per leaf (1..4; 0 = the default 1)", maxLeaf);
    if (radius > 32u) return fail(TBVH_E_INVALID, "tbvh_build_device_custom_spheres: search radius %u (1..32; 0 = the default 16)", radius);
    TBVH_ENTER(c);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH2_WALD);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    s->sphN = n; s->sphBuilder = builder;
    s->sphMaxLeaf = builder == 1 || maxLeaf == 0 ? 1u : maxLeaf;   // (PLOC: one sphere per leaf)
    s->sphRadius = radius ? radius : 16u;
    const float4* dSph = nullptr;
    int r = stageSpheres(s, "tbvh_build_device_custom_spheres", spheres16, n, onDevice, &dSph);
    if (!r) r = buildSphereTree(s, "tbvh_build_device_custom_spheres", dSph, n);
    if (r) { tbvh_free_scene(s); return r; }
    *out = s;
    return 0;
}

int tbvh_build_device_custom_spheres_sah(tbvh_context* c, const void* spheres16, uint64_t n, int onDevice, uint32_t maxLeaf, tbvh_scene** out) {
    const char* who = "tbvh_build_device_custom_spheres_sah";
    if (!c || !spheres16 || !out || !n) return fail(TBVH_E_INVALID, "%s: null/empty argument", who);
    if (n > 0x3fffffffull) return fail(TBVH_E_INVALID, "%s: %llu spheres: at most 2^30 - 1", who, (unsigned long long)n);
    if (maxLeaf > 4u) return fail(TBVH_E_INVALID, "%s: %u spheres per leaf (1..4; 0 = the leaves BVH::Build makes)", who, maxLeaf);
    TBVH_ENTER(c);
    tbvh_scene* s = newScene(c, TBVH_LAYOUT_BVH2_WALD);
    if (!s) return fail(TBVH_E_NOMEM, "out of host memory");
    s->sphN = n; s->sphBuilder = 2; s->sphMaxLeaf = maxLeaf;
    const float4* dSph = nullptr;
    int r = stageSpheres(s, who, spheres16, n, onDevice, &dSph);
    if (!r) r = buildSphereTree(s, who, dSph, n);
    if (r) { tbvh_free_scene(s); return r; }
    *out = s;
    return 0;
}

int tbvh_rebuild_custom_spheres_device(tbvh_scene* s, const void* spheres16, uint64_t n, int onDevice) {
    if (int r = checkMovingSpheres("tbvh_rebuild_custom_spheres_device", s, spheres16, n)) return r;
    if (n > 0x7FFFFFFFull) return fail(TBVH_E_INVALID, "tbvh_rebuild_custom_spheres_device: %llu spheres: at most 2^31 - 1", (unsigned long long)n);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    const float4* dSph = nullptr;
    if (int r = stageSpheres(s, "tbvh_rebuild_custom_spheres_device", spheres16, n, onDevice, &dSph)) return r;
    return buildSphereTree(s, "tbvh_rebuild_custom_spheres_device", dSph, n);
}

int tbvh_refit_custom_spheres(tbvh_scene* s, const void* spheres16, uint64_t n, int onDevice) {
    if (int r = checkMovingSpheres("tbvh_refit_custom_spheres", s, spheres16, n)) return r;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    const float4* dSph = nullptr;
    if (int r = stageSpheres(s, "tbvh_refit_custom_spheres", spheres16, n, onDevice, &dSph)) return r;
    if (s->refitScratch.reserve((size_t)s->nNodes * 4) != hipSuccess) { (void)hipGetLastError(); return fail(TBVH_E_NOMEM, "tbvh_refit_custom_spheres: out of device memory"); }
    HIP_TRY(timedBegin(c));
    HIP_TRY(launch_refit_spheres(s->nodes, s->nNodes, s->tris, s->nTriBlocks / 2, dSph, n, (uint32_t*)s->refitScratch.get(), c->stream));
    HIP_TRY(timedEnd(c));
    HIP_TRY(hipStreamSynchronize(c->stream));   // (the caller's spheres may change)
    return 0;
}

int tbvh_custom_spheres_download(tbvh_scene* s, void* nodes32, uint64_t capNodes, uint32_t* primIdx, uint64_t capIdx, void* spheres16, uint64_t capSpheres,
                                 uint64_t* nNodesOut, uint64_t* nIdxOut) {
    if (!s) return fail(TBVH_E_INVALID, "tbvh_custom_spheres_download: null argument");
    if (s->isTlas || s->layout != TBVH_LAYOUT_BVH2_WALD) return fail(TBVH_E_INVALID, "tbvh_custom_spheres_download: not a sphere BLAS (layout %d)", s->layout);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    const uint64_t nNodes = s->nNodes, nIdx = s->nTriBlocks / 2;
    if (nNodesOut) *nNodesOut = nNodes;
    if (nIdxOut) *nIdxOut = nIdx;
    if (nodes32 && capNodes < nNodes) return fail(TBVH_E_INVALID, "tbvh_custom_spheres_download: node buffer too small (%llu < %llu)", (unsigned long long)capNodes, (unsigned long long)nNodes);
    if (primIdx && capIdx < nIdx) return fail(TBVH_E_INVALID, "tbvh_custom_spheres_download: index buffer too small (%llu < %llu)", (unsigned long long)capIdx, (unsigned long long)nIdx);
    if (spheres16 && capSpheres < nIdx) return fail(TBVH_E_INVALID, "tbvh_custom_spheres_download: sphere buffer too small (%llu < %llu)", (unsigned long long)capSpheres, (unsigned long long)nIdx);
    if (!nodes32 && !primIdx && !spheres16) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nodes32) HIP_TRY(hipMemcpy(nodes32, s->nodes, nNodes * 32, hipMemcpyDeviceToHost));
    if (primIdx || spheres16) {   // the records {sphere}, {prim, 0, 0, 0} come back whole and are taken apart here
        std::vector<Vec4> recs;
        try { recs.resize(nIdx * 2); } catch (const std::bad_alloc&) { return fail(TBVH_E_NOMEM, "out of host memory"); }
        HIP_TRY(hipMemcpy(recs.data(), s->tris, nIdx * 32, hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < nIdx; k++) {
            if (spheres16) ((Vec4*)spheres16)[k] = recs[2 * k];
            if (primIdx) std::memcpy(&primIdx[k], &recs[2 * k + 1].x, 4);
        }
    }
    return 0;
}

int tbvh_custom_spheres_bounds(tbvh_scene* s, float bounds6[6]) {
    if (!s || !bounds6) return fail(TBVH_E_INVALID, "tbvh_custom_spheres_bounds: null argument");
    if (s->isTlas || s->layout != TBVH_LAYOUT_BVH2_WALD) return fail(TBVH_E_INVALID, "tbvh_custom_spheres_bounds: not a sphere BLAS (layout %d)", s->layout);
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    float root[8];
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(root, s->nodes, 32, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; k++) { bounds6[k] = root[k]; bounds6[3 + k] = root[4 + k]; }
    return 0;
}

}  // extern "C"
