// capi_custom.hip — custom-geometry sphere BLASes (BVH::Build( customGetAABB, n ), tiny_bvh.h:2190-2219, traced through the sphere callback of the
// reference's anim demo): upload with validation and the host builder behind tbvh_host_build_custom_spheres.  The kernels are kernels_custom.hip;
// queries reach them through launchQuery (capi_query.hip), TLASes over sphere BLASes through tbvh_upload_tlas (capi_scene.hip).
// A sphere scene (layout TBVH_LAYOUT_BVH2_WALD) keeps the Wald nodes as uploaded in `nodes` and the spheres gathered in primIdx order in `tris`
// (2 float4 per index entry: {x, y, z, r}, {prim, 0, 0, 0}); a TLAS's BlasDesc points at the two.  tbvh_free_scene frees them like any scene's.
#include "capi_internal.h"

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
    s->bytes = nNodes * 32 + nIdx * 32;
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
