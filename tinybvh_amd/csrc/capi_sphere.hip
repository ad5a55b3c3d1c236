// capi_sphere.hip — BVH::IntersectSphere (tiny_bvh.h:3140-3200) batched: tbvh_intersect_spheres / _device.  The kernels are
// kernels_sphere.hip (DESIGN.md par. 11); the launch shares the context's ray-pool counters, stack spill area, staging buffers and timing
// ring with the ray queries (capi_query.hip: launchQuery).
#include "capi_internal.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace tbvh_capi {
int checkSphereScene(tbvh_scene* s, const char* who) {
    if (!s) return fail(TBVH_E_INVALID, "%s: null scene", who);
    TBVH_REFUSE_DOUBLE(s, who);
    TBVH_REFUSE_VOXEL(s, who);
    TBVH_REFUSE_CUSTOM(s, who);
    if (s->isTlas) return fail(TBVH_E_INVALID, "%s: a TLAS has no sphere query (the reference's would read instance indices as triangles); query its BLASes", who);
    if (s->layout != TBVH_LAYOUT_BVH_GPU && s->layout != TBVH_LAYOUT_BVH4_GPU && s->layout != TBVH_LAYOUT_CWBVH)
        return fail(TBVH_E_INVALID, "%s: scene layout %d has no sphere query", who, s->layout);
    return 0;
}
}  // namespace tbvh_capi

namespace {

// the refusals every entry point makes before it touches the scene's memory or launches anything
int checkSphereArgs(tbvh_scene* s, const void* spheres, uint64_t n, const void* verts, uint64_t nTris, const void* hit, const char* who) {
    if (int r = checkSphereScene(s, who)) return r;
    if (n == 0) return 0;
    if (!spheres || !verts || !hit) return fail(TBVH_E_INVALID, "%s: null argument", who);
    if (nTris == 0) return fail(TBVH_E_INVALID, "%s: empty vertex array", who);
    if (nTris > (1ull << 32)) return fail(TBVH_E_INVALID, "%s: %llu triangles: primitive indices are 32-bit", who, (unsigned long long)nTris);
    return 0;
}

}  // namespace

namespace tbvh_capi {
// one launch on the context's stream (asynchronous); dSpheres / dHit are device arrays, verts a device-resident source (mesh_source.h)
int launchSpheres(tbvh_scene* s, const float4* dSpheres, uint64_t n, const MeshSrc& verts, uint8_t* dHit) {
    tbvh_context* c = s->ctx;
    const size_t poolWords = (size_t)(kPoolParts + 1) * kPoolCounterStride;
    if (!c->poolClean) HIP_TRY(hipMemsetAsync(c->pool, 0, poolWords * 4 * 2, c->stream));
    c->poolClean = false;
    SphereArgs q;
    q.spheres = dSpheres; q.nSpheres = n; q.hit = dHit;
    q.nodes = s->nodes; q.tris = s->tris;   // the uploaded arrays, not the 8-wide copy of a BVH_GPU / BVH4_GPU scene
    q.verts = verts;
    q.spill = c->spill; q.spillStride = c->spillEntries / 2;   // 8-byte stack entries
    q.counter = (uint32_t*)c->pool + (size_t)c->poolCur * poolWords; q.counterNext = (uint32_t*)c->pool + (size_t)(c->poolCur ^ 1) * poolWords;
    q.poolParts = c->poolParts;
    // one workgroup per 128 spheres, at least four per CU, at most the persistent grid the spill area is sized for
    const uint64_t want = (n + 127) / 128, lo = (uint64_t)c->numCUs * 4u;
    const uint32_t blocks = (uint32_t)(want < lo ? lo : (want > c->blocks ? c->blocks : want));
    HIP_TRY(timedBegin(c));
    launch_spheres(s->layout, q, c->status, blocks, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timedEnd(c));
    c->poolCur ^= 1; c->poolClean = true;
    return 0;
}
}  // namespace tbvh_capi

extern "C" {

int tbvh_intersect_spheres_device(tbvh_scene* s, const void* dSpheres, uint64_t n, const void* dVerts, uint64_t nTris, uint8_t* dHit) {
    if (int r = checkSphereArgs(s, dSpheres, n, dVerts, nTris, dHit, "tbvh_intersect_spheres_device")) return r;
    if (n == 0) return 0;
    if ((((uintptr_t)dSpheres) | ((uintptr_t)dVerts)) & 15) return fail(TBVH_E_INVALID, "tbvh_intersect_spheres_device: sphere and vertex arrays must be 16-byte aligned");
    TBVH_ENTER(s->ctx);
    return launchSpheres(s, (const float4*)dSpheres, n, flat_mesh((const float4*)dVerts, nTris), dHit);
}

// host arrays: the spheres go up through the context's ray staging buffer (4 spheres per 64-byte record), the vertices through the scene's
// vertex staging buffer (the one tbvh_refit uses), the answers come back through the any-hit result buffer
int tbvh_intersect_spheres(tbvh_scene* s, const void* spheres, uint64_t n, const void* verts, uint64_t nTris, uint8_t* hit) {
    if (int r = checkSphereArgs(s, spheres, n, verts, nTris, hit, "tbvh_intersect_spheres")) return r;
    if (n == 0) return 0;
    tbvh_context* c = s->ctx;
    TBVH_ENTER(c);
    if (int r = ensureStage(c, (n + 3) / 4)) return r;
    if (int r = ensureStageOcc(c, n)) return r;
    HIP_TRY(s->vertStage.reserve(nTris * 48));
    HIP_TRY(hipMemcpyAsync(c->stageRays, spheres, n * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(s->vertStage, verts, nTris * 48, hipMemcpyHostToDevice, c->stream));
    int r = launchSpheres(s, (const float4*)c->stageRays.get(), n, flat_mesh((const float4*)s->vertStage.get(), nTris), c->stageOcc);
    if (!r && hipMemcpyAsync(hit, c->stageOcc, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) r = fail(TBVH_E_HIP, "tbvh_intersect_spheres: copy from the device failed");
    if (!r) return checkStatus(c);   // (synchronizes)
    hipStreamSynchronize(c->stream);
    return r;
}

}  // extern "C"
