// watertight_ref_shim.cpp — the real reference behind the watertight-mode tests (tests/watertight_lib.py compiles it per session; nothing of it is kept).
// Built three ways over a temporary copy of tiny_bvh.h whose TriOccludes got the one line it lacks under WATERTIGHT_TRITEST (watertight_lib.patched_header):
//   -DWATERTIGHT_TRITEST -ffp-contract=off   the test the library restates: every product and sum rounded on its own
//   -DWATERTIGHT_TRITEST                     the same source as the reference's usual flags build it (g++ -mfma contracts Cx * By - Cy * Bx): it leaks
//   (no define)                              Moeller-Trumbore
// Offers (a) IntersectTri / TriOccludes on one triangle per ray, (b) the brute force: every triangle in index order through IntersectTri (on an exact tie the
// smaller index stays: tiny_bvh.h:8506 rejects t >= hit.t) and the occlusion flag through TriOccludes, with or without opacity micromaps, and (c) BVH::Build +
// Intersect / IsOccluded, for the record.  Rays are 64-byte records: the first 64 bytes of tinybvh::Ray, rD taken as the record holds it.
#define TINYBVH_IMPLEMENTATION
#include "tiny_bvh.h"

#include <cstdint>
#include <cstring>

using namespace tinybvh;

namespace {
struct Open : public BVH {   // IntersectTri and TriOccludes are protected members of BVHBase
    void tri(Ray& r, uint32_t idx, const bvhvec4slice& v, uint32_t i0, uint32_t i1, uint32_t i2) const { IntersectTri(r, idx, v, i0, i1, i2); }
    bool occ(const Ray& r, const bvhvec4slice& v, uint32_t idx, uint32_t i0, uint32_t i1, uint32_t i2) const { return TriOccludes(r, v, idx, i0, i1, i2); }
};
Ray load(const void* rays64, uint64_t i) {
    Ray r;
    memcpy((void*)&r, (const char*)rays64 + i * 64, 64);
    return r;
}
void store(void* rays64, uint64_t i, const Ray& r) { memcpy((char*)rays64 + i * 64 + 48, (const char*)&r + 48, 16); }
}  // namespace

extern "C" {

int wref_watertight(void) {
#ifdef WATERTIGHT_TRITEST
    return 1;
#else
    return 0;
#endif
}

// (a) pair i: ray i against the triangle tris9[9 i ..] (as three bvhvec4, w = 0); accept / tuv as IntersectTri leaves the ray; occ as TriOccludes answers
void wref_pairs(const void* rays64, const float* tris9, uint64_t n, uint8_t* accept, float* tuv, uint8_t* occ) {
    Open b;
    for (uint64_t i = 0; i < n; i++) {
        bvhvec4 v[3];
        for (int k = 0; k < 3; k++) v[k] = bvhvec4(tris9[9 * i + 3 * k], tris9[9 * i + 3 * k + 1], tris9[9 * i + 3 * k + 2], 0);
        const bvhvec4slice s(v, 3);
        Ray r = load(rays64, i);
        const Ray r0 = r;
        r.hit.prim = 0xFFFFFFFFu;
        b.tri(r, 7u, s, 0, 1, 2);
        accept[i] = r.hit.prim == 7u ? 1 : 0;
        tuv[3 * i] = accept[i] ? r.hit.t : 0.f; tuv[3 * i + 1] = accept[i] ? r.hit.u : 0.f; tuv[3 * i + 2] = accept[i] ? r.hit.v : 0.f;
        occ[i] = b.occ(r0, s, 0u, 0, 1, 2) ? 1 : 0;
    }
}

// (b) brute force over verts (3 bvhvec4 per triangle): the rays' hit records are updated in place, occ[i] = some triangle occludes ray i (as the ray came in)
void wref_brute(const float* verts16, uint32_t nTris, void* rays64, uint64_t n, uint8_t* occ, uint32_t* opmap, uint32_t opmapN) {
    Open b;
    if (opmap) b.SetOpacityMicroMaps(opmap, opmapN);
    const bvhvec4slice s((const bvhvec4*)verts16, nTris * 3);
    for (uint64_t i = 0; i < n; i++) {
        Ray r = load(rays64, i);
        const Ray r0 = r;
        bool o = false;
        for (uint32_t t = 0; t < nTris; t++) {
            b.tri(r, t, s, 3 * t, 3 * t + 1, 3 * t + 2);
            if (!o) o = b.occ(r0, s, t, 3 * t, 3 * t + 1, 3 * t + 2);
        }
        store(rays64, i, r);
        if (occ) occ[i] = o ? 1 : 0;
    }
}

// (b') the same through instances, entered as IntersectTLAS enters them (tiny_bvh.h:3329-3333: the ray's origin and direction through the instance's inverse
// transform by the reference's own tinybvh_transform_point / _vector, rD by its tinybvh_rcp), instances in index order, each BLAS's triangles in index order:
// on an exact tie the smaller instance, then the smaller primitive, stays.  inv16: nInst x 16 floats; the winning instance goes to byte 44 of the record.
void wref_brute_tlas(const float* const* blasVerts, const uint32_t* blasTris, const float* inv16, const uint32_t* instBlas, uint32_t nInst, void* rays64, uint64_t n,
                     uint8_t* occ) {
    Open b;
    for (uint64_t i = 0; i < n; i++) {
        Ray r = load(rays64, i);
        const Ray r0 = r;
        uint32_t inst = 0;
        bool o = false;
        for (uint32_t k = 0; k < nInst; k++) {
            bvhmat4 M;
            memcpy((void*)&M, inv16 + 16 * k, 64);
            Ray t = r, t0 = r0;
            t.O = t0.O = tinybvh_transform_point(r.O, M);
            t.D = t0.D = tinybvh_transform_vector(r.D, M);
            t.rD = t0.rD = tinybvh_rcp(t.D);
            const uint32_t nT = blasTris[instBlas[k]];
            const bvhvec4slice s((const bvhvec4*)blasVerts[instBlas[k]], nT * 3);
            const float before = t.hit.t;
            for (uint32_t p = 0; p < nT; p++) {
                b.tri(t, p, s, 3 * p, 3 * p + 1, 3 * p + 2);
                if (!o) o = b.occ(t0, s, p, 3 * p, 3 * p + 1, 3 * p + 2);
            }
            if (t.hit.t < before) { r.hit = t.hit; inst = k; }
        }
        store(rays64, i, r);
        if (r.hit.t < r0.hit.t) memcpy((char*)rays64 + i * 64 + 44, &inst, 4);
        if (occ) occ[i] = o ? 1 : 0;
    }
}

// The reference keeps its edge functions to itself, so the edge-function check of a contracted build restates the ONE expression whose contraction is the point,
// `Px * Qy - Py * Qx`, inside the same build: this compiler, with this build's flags, contracts it here as it does in the reference's test (under -mfma one
// product is fused into the subtraction; under -ffp-contract=off none).  Everything around it is the caller's: pq4[4 i ..] = the sheared coordinates Px, Py, Qx,
// Qy of the edge's two vertices as ray i sees them (tests/test_watertight_host.py computes them in numpy, one rounding per operation); e[i] = the edge function
// of the directed edge P -> Q.  A triangle sharing the edge sees Q -> P.
void wref_edge(const float* pq4, uint64_t n, float* e) {
    for (uint64_t i = 0; i < n; i++) {
        const float Px = pq4[4 * i], Py = pq4[4 * i + 1], Qx = pq4[4 * i + 2], Qy = pq4[4 * i + 3];
        e[i] = Px * Qy - Py * Qx;
    }
}

// (c) the reference's own traversal: BVH::Build (hq: BuildHQ), Intersect and IsOccluded
void wref_bvh(const float* verts16, uint32_t nTris, int hq, void* rays64, uint64_t n, uint8_t* occ) {
    BVH b;
    if (hq) b.BuildHQ((const bvhvec4*)verts16, nTris); else b.Build((const bvhvec4*)verts16, nTris);
    for (uint64_t i = 0; i < n; i++) {
        Ray r = load(rays64, i);
        if (occ) occ[i] = b.IsOccluded(r) ? 1 : 0;
        b.Intersect(r);
        store(rays64, i, r);
    }
}

}  // extern "C"
