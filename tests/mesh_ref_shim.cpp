// mesh_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's indexed / strided triangle input behind a C interface:
// BVH_GPU::Build( bvhvec4slice, indices, n ) and Build( bvhvec4slice ), then BVH::Intersect / IsOccluded / IntersectSphere / Refit over
// BVH::vertIdx and BVH_GPU::ConvertFrom again.
//
// Compiled at test time (tests/mesh_lib.py: compile_ref_shim) from $TBVH_REFERENCE/tiny_bvh.h with the flags of oracle/Makefile, into the pytest
// temp dir; nothing of the reference is copied into the repository.  The reference reads a whole bvhvec4 at data + i * stride, so the shim keeps
// the vertices in a 64-byte-aligned copy with 16 spare bytes behind it, and callers pass strides that are multiples of 16.  The meshes used are
// below the reference's threshold for threaded builds, so node numbering is reproducible.
// BVH::IntersectSphere does not terminate for every sphere (DESIGN.md par. 11, defect 1): callers pass only spheres the restatement's verbatim
// walk (tests/oracle_sphere.c) has shown to terminate.
#include <algorithm>
#include <atomic>
#include <cassert>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <functional>
#include <malloc.h>
#include <math.h>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <thread>
#include <vector>
#include <immintrin.h>
#include <xmmintrin.h>

#define private public
#define TINYBVH_IMPLEMENTATION
#include "tiny_bvh.h"
#undef private

using namespace tinybvh;

namespace {
struct MeshRef {
    void* verts = nullptr;          // 64-byte aligned copy, vertBytes + 16 bytes
    size_t vertBytes = 0;
    std::vector<uint32_t> idx;
    BVH_GPU gpu;
    ~MeshRef() { free(verts); }
};
inline void load(Ray& r, const char* src) { std::memset((void*)&r, 0, sizeof(Ray)); std::memcpy((void*)&r, src, 64); }
inline void store(char* dst, const Ray& r) { std::memcpy(dst + 44, (const char*)&r + 44, 20); }
}  // namespace

extern "C" {

// verts: nVerts * stride bytes (stride a multiple of 16); indices: 3 per triangle, or null: triangle i = vertices 3i, 3i + 1, 3i + 2
void* mref_build(const void* verts, uint32_t nVerts, uint32_t stride, const uint32_t* indices, uint32_t nTris) {
    MeshRef* m = new MeshRef;
    m->vertBytes = (size_t)nVerts * stride;
    m->verts = aligned_alloc(64, (m->vertBytes + 16 + 63) & ~(size_t)63);
    std::memset(m->verts, 0, (m->vertBytes + 16 + 63) & ~(size_t)63);
    std::memcpy(m->verts, verts, m->vertBytes);
    const bvhvec4slice slice((const bvhvec4*)m->verts, nVerts, stride);
    if (indices) {
        m->idx.assign(indices, indices + (size_t)nTris * 3);
        m->gpu.Build(slice, m->idx.data(), nTris);
    } else m->gpu.Build(slice);
    return m;
}
void mref_free(void* h) { delete (MeshRef*)h; }
// 0 = BVH_GPU nodes (64 bytes, usedNodes), 1 = primIdx (idxCount), 2 = the BVH's Wald nodes (32 bytes, usedNodes)
uint64_t mref_blob(void* h, int which, const void** out) {
    MeshRef* m = (MeshRef*)h;
    if (which == 0) { *out = m->gpu.bvhNode; return m->gpu.usedNodes; }
    if (which == 1) { *out = m->gpu.bvh.primIdx; return m->gpu.bvh.idxCount; }
    *out = m->gpu.bvh.bvhNode; return m->gpu.bvh.usedNodes;
}
void mref_intersect(void* h, void* rays, uint64_t n) {
    const BVH& bvh = ((MeshRef*)h)->gpu.bvh;
    char* p = (char*)rays;
    for (uint64_t i = 0; i < n; i++, p += 64) { Ray r; load(r, p); bvh.Intersect(r); store(p, r); }
}
void mref_occluded(void* h, const void* rays, uint64_t n, uint8_t* out) {
    const BVH& bvh = ((MeshRef*)h)->gpu.bvh;
    const char* p = (const char*)rays;
    for (uint64_t i = 0; i < n; i++, p += 64) { Ray r; load(r, p); out[i] = bvh.IsOccluded(r) ? 1 : 0; }
}
void mref_spheres(void* h, const float* spheres16, uint64_t n, uint8_t* out) {
    const BVH& bvh = ((MeshRef*)h)->gpu.bvh;
    for (uint64_t i = 0; i < n; i++) { const float* p = spheres16 + 4 * i; out[i] = bvh.IntersectSphere(bvhvec3(p[0], p[1], p[2]), p[3]) ? 1 : 0; }
}
// moved vertices (same layout as at build time), BVH::Refit, BVH_GPU::ConvertFrom again
void mref_refit(void* h, const void* verts) {
    MeshRef* m = (MeshRef*)h;
    std::memcpy(m->verts, verts, m->vertBytes);
    m->gpu.bvh.Refit();
    m->gpu.ConvertFrom(m->gpu.bvh, false);
}

}  // extern "C"
