// capi_watertight.hip — a scene's choice of triangle test (tbvh_set_triangle_test / tbvh_scene_triangle_test): Moeller-Trumbore over the records as
// uploaded (the default; nothing in here touches such a scene) or the watertight test of device_common.h (tri_test_wt) over the triangle's three vertices.
// A watertight scene keeps its own flat copy of the caller's vertices; the records, the nodes and every derived copy stay what they were, so switching back
// restores the default's records and kernels by doing nothing to them.  DESIGN.md par. 4.6 has the measurements and the node test's bound.
#include "capi_internal.h"

using namespace tbvh;
using namespace tbvh_capi;

namespace tbvh_capi {
void shareTriangleTest(tbvh_scene* s) {
    if (tbvh_scene* w = s->copies.copy8) { w->triTest = s->triTest; w->wtVerts = s->wtVerts; w->wtTris = s->wtTris; }   // (shared, owned by s)
}

// The scene's vertices from a device-resident source, flattened to 3 float4 per triangle; asynchronous on the context's stream.
static int takeVertices(tbvh_scene* s, const MeshSrc& src) {
    tbvh_context* c = s->ctx;
    bool moved = false;
    if (src.nTris * 3 > s->wtVertsOwn.count() || !s->wtVertsOwn) {
        HIP_TRY(hipStreamSynchronize(c->stream));   // (launches in flight read the old array)
        s->wtVertsOwn.reset();
        HIP_TRY(s->wtVertsOwn.alloc(src.nTris * 3));
        moved = true;
    }
    launch_flatten_mesh(src, s->wtVertsOwn, c->status, c->stream);
    HIP_TRY(hipGetLastError());
    moved |= s->wtTris != src.nTris;
    s->wtVerts = s->wtVertsOwn; s->wtTris = src.nTris;
    shareTriangleTest(s);
    // the TLASes over this BLAS hold the array's address and count in their descriptor tables
    if (moved) return forEachTlasOver(s, [](tbvh_scene* t) { return reclassifyTlas(t); });
    return 0;
}

int refreshWatertightVerts(tbvh_scene* s, const MeshSrc& src) {
    if (!s->triTest || !s->wtVertsOwn) return 0;   // (a copy reads its owner's array: the owner's refit has written it)
    return takeVertices(s, src);
}
}  // namespace tbvh_capi

extern "C" {

int tbvh_scene_triangle_test(const tbvh_scene* s) {
    if (!s) return fail(TBVH_E_INVALID, "tbvh_scene_triangle_test: null scene");
    if (s->isTlas) {   // a TLAS has no mode of its own: it reports its BLASes' (one and the same: tbvh_upload_tlas admits no mix)
        for (const tbvh_scene* b : s->tlas.blasList) if (b && b->triTest) return b->triTest;
        return TBVH_TRITEST_MOLLER_TRUMBORE;
    }
    return s->triTest;
}

int tbvh_set_triangle_test(tbvh_scene* s, int test, const void* verts16, uint64_t nTris, int onDevice) {
    const char* who = "tbvh_set_triangle_test";
    if (!s) return fail(TBVH_E_INVALID, "%s: null scene", who);
    if (test != TBVH_TRITEST_MOLLER_TRUMBORE && test != TBVH_TRITEST_WATERTIGHT) return fail(TBVH_E_INVALID, "%s: test %d (0 = Moeller-Trumbore, 1 = watertight)", who, test);
    if (s->layout == TBVH_LAYOUT_BVH_DOUBLE) return fail(TBVH_E_INVALID, "%s: a BVH_DOUBLE scene has one triangle test, the reference's fp64 one", who);
    if (s->layout == TBVH_LAYOUT_VOXELSET || s->layout == TBVH_LAYOUT_BVH2_WALD) return fail(TBVH_E_INVALID, "%s: a voxel set or a sphere BLAS holds no triangles", who);
    if (s->isTlas) return fail(TBVH_E_INVALID, "%s: a TLAS has no triangle test of its own; it is set on the BLASes", who);
    if (s->layout != TBVH_LAYOUT_CWBVH && s->layout != TBVH_LAYOUT_BVH_GPU && s->layout != TBVH_LAYOUT_BVH4_GPU) return fail(TBVH_E_INVALID, "%s: layout %d is not a triangle BLAS", who, s->layout);
    tbvh_context* c = s->ctx;
    TBVH_LOCK(c);
    if (!s->usedBy.empty()) return fail(TBVH_E_INVALID, "%s: a TLAS is built over this BLAS; free the TLAS first (a TLAS reads its BLASes' test when it is uploaded)", who);
    if (s->variant != 0) return fail(TBVH_E_INVALID, "%s: the scene is pinned to kernel variant %d (tbvh_set_variant), which has no watertight form", who, s->variant);
    if (test == TBVH_TRITEST_WATERTIGHT && !verts16 && !s->wtVertsOwn)
        return fail(TBVH_E_INVALID, "%s: the watertight test reads the triangles' vertices; the scene holds none, pass verts16", who);
    if (verts16 && !nTris) return fail(TBVH_E_INVALID, "%s: verts16 with n_tris = 0", who);
    if (verts16 && nTris > 0xffffffffull) return fail(TBVH_E_INVALID, "%s: more than 2^32 - 1 triangles", who);
    if (int r = setDevice(c)) return r;
    if (test == TBVH_TRITEST_MOLLER_TRUMBORE) {
        if (!s->triTest) return 0;
        HIP_TRY(hipStreamSynchronize(c->stream));   // (launches in flight read the vertices)
        s->triTest = 0; s->wtVerts = nullptr; s->wtTris = 0; s->wtVertsOwn.reset();
        shareTriangleTest(s);
        // a BVH_GPU / BVH4_GPU scene too small for an 8-wide copy of its own got one for this mode: it goes, and the scene decides about a copy as a scene
        // that never saw this call does (capi_copies.hip: makeCopyOnce at its next query)
        if (s->layout != TBVH_LAYOUT_CWBVH) { freeCopy(s, kCopyWide8); s->copies.tried8 = false; s->copies.tlasOnly = false; }
        return 0;
    }
    if (verts16) {
        const tbvh_mesh m = flatMesh(verts16, nTris, onDevice);
        DeviceMesh dm;
        if (int r = stageMesh(c, m, dm)) return r;
        const int wasTest = s->triTest;
        s->triTest = TBVH_TRITEST_WATERTIGHT;
        int r = takeVertices(s, dm.src);
        if (!r && hipStreamSynchronize(c->stream) != hipSuccess) r = fail(TBVH_E_HIP, "%s: the vertex copy failed", who);   // (the staged copy goes with this call)
        if (r) { s->triTest = wasTest; if (!wasTest) { s->wtVerts = nullptr; s->wtTris = 0; s->wtVertsOwn.reset(); } shareTriangleTest(s); return r; }
    }
    s->triTest = TBVH_TRITEST_WATERTIGHT;
    shareTriangleTest(s);
    if (s->layout != TBVH_LAYOUT_CWBVH) if (int r = ensureWatertightCopy(s)) {
        s->triTest = 0; s->wtVerts = nullptr; s->wtTris = 0; s->wtVertsOwn.reset();
        return r;
    }
    return 0;
}

// The triangle tests on the host, one pair per call (tests/test_watertight_host.py): ray64 = a 64-byte ray record (O, D, rD, hit.t = the ray's tmax), v0, v1, v2 =
// three floats each.  Returns 1 (accepted; *t, *u, *v written), 0 (rejected) or a negative TBVH_E_* code.  test 0 runs tri_test over {v0, v1 - v0, v2 - v0}.
int tbvh_host_tri_test(int test, const void* ray64, const float* v0, const float* v1, const float* v2, float* t, float* u, float* v) {
    if (!ray64 || !v0 || !v1 || !v2 || !t || !u || !v) return fail(TBVH_E_INVALID, "tbvh_host_tri_test: null argument");
    if (test != TBVH_TRITEST_MOLLER_TRUMBORE && test != TBVH_TRITEST_WATERTIGHT) return fail(TBVH_E_INVALID, "tbvh_host_tri_test: test %d", test);
    const RayRec* r = (const RayRec*)ray64;
    RayRec ray;
    memcpy(&ray, r, sizeof(ray));
    const float3 O = make_float3(ray.O.x, ray.O.y, ray.O.z), D = make_float3(ray.D.x, ray.D.y, ray.D.z), rD = make_float3(ray.rD.x, ray.rD.y, ray.rD.z);
    const float3 a = make_float3(v0[0], v0[1], v0[2]), b = make_float3(v1[0], v1[1], v1[2]), cc = make_float3(v2[0], v2[1], v2[2]);
    TriHit h = {0.f, 0.f, 0.f};
    bool ok;
    if (test == TBVH_TRITEST_WATERTIGHT) ok = tri_test_wt(O, wt_precalc(D, rD), a, b, cc, ray.hit.x, h);
    else ok = tri_test(O, D, a, make_float3(b.x - a.x, b.y - a.y, b.z - a.z), make_float3(cc.x - a.x, cc.y - a.y, cc.z - a.z), ray.hit.x, h);
    if (ok) { *t = h.t; *u = h.u; *v = h.v; }
    return ok ? 1 : 0;
}

// ... and n pairs per call: rays64 = n ray records, tris9 = n x {v0, v1, v2}; accept: n bytes; tuv: n x 3 floats (written for accepted pairs, else 0);
// uvw: n x 3 floats, the watertight test's three edge functions U, V, W (or NULL; test 1 only); roles: 0 = IntersectTri's, 1 = TriOccludes'
int tbvh_debug_tri_test_batch(int test, int roles, const void* rays64, const float* tris9, uint64_t n, uint8_t* accept, float* tuv, float* uvw) {
    if (n && (!rays64 || !tris9 || !accept || !tuv)) return fail(TBVH_E_INVALID, "tbvh_debug_tri_test_batch: null argument");
    if (test != TBVH_TRITEST_MOLLER_TRUMBORE && test != TBVH_TRITEST_WATERTIGHT) return fail(TBVH_E_INVALID, "tbvh_debug_tri_test_batch: test %d", test);
    for (uint64_t i = 0; i < n; i++) {
        RayRec ray;
        memcpy(&ray, (const char*)rays64 + i * 64, sizeof(ray));
        const float* p = tris9 + 9 * i;
        const float3 O = make_float3(ray.O.x, ray.O.y, ray.O.z), D = make_float3(ray.D.x, ray.D.y, ray.D.z), rD = make_float3(ray.rD.x, ray.rD.y, ray.rD.z);
        const float3 a = make_float3(p[0], p[1], p[2]), b = make_float3(p[3], p[4], p[5]), cc = make_float3(p[6], p[7], p[8]);
        TriHit h = {0.f, 0.f, 0.f};
        bool ok;
        if (test == TBVH_TRITEST_WATERTIGHT) {
            const WtPre pre = wt_precalc(D, rD);
            ok = roles ? tri_test_wt(O, pre, cc, a, b, ray.hit.x, h, Omm{nullptr, 0u}, 0u, true, uvw ? uvw + 3 * i : nullptr)
                       : tri_test_wt(O, pre, a, b, cc, ray.hit.x, h, Omm{nullptr, 0u}, 0u, false, uvw ? uvw + 3 * i : nullptr);
        } else ok = tri_test(O, D, a, make_float3(b.x - a.x, b.y - a.y, b.z - a.z), make_float3(cc.x - a.x, cc.y - a.y, cc.z - a.z), ray.hit.x, h);
        accept[i] = ok ? 1 : 0;
        tuv[3 * i] = ok ? h.t : 0.f; tuv[3 * i + 1] = ok ? h.u : 0.f; tuv[3 * i + 2] = ok ? h.v : 0.f;
    }
    return 0;
}

}  // extern "C"
