// sphere_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's BVH::IntersectSphere behind a C interface.
//
// Compiled at test time (tests/sphere_lib.py: ref_shim) from $TBVH_REFERENCE/tiny_bvh.h with the flags of oracle/Makefile, into the pytest
// temp dir; nothing of the reference is copied into the repository.  The node arrays are private in the reference; the standard headers are
// included first and `private` is then read as `public` while the reference header is compiled, so the arrays can be handed out as they are.
//
// BVH::IntersectSphere (tiny_bvh.h:3140-3200) does not terminate for every sphere (DESIGN.md par. 11, defect 1): callers pass only spheres
// that the restatement's verbatim walk (tests/oracle_sphere.c, mode 0) has shown to terminate inside the node array.
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
struct Scene {
    std::vector<bvhvec4> verts;
    BVH bvh;
    BVH_GPU* gpu2 = nullptr;
    BVH4_GPU* gpu4 = nullptr;
    BVH8_CWBVH* cw = nullptr;
    int hq = 0;
};
}  // namespace

extern "C" {

// BVH::Build (hq = 0) or BVH::BuildHQ (hq = 1) over n_tris x 3 bvhvec4 vertices (copied)
void* sref_build(const void* verts16, uint32_t nTris, int hq) {
    Scene* s = new Scene();
    s->verts.assign((const bvhvec4*)verts16, (const bvhvec4*)verts16 + (size_t)nTris * 3);
    s->hq = hq;
    if (hq) s->bvh.BuildHQ(s->verts.data(), nTris); else s->bvh.Build(s->verts.data(), nTris);
    return s;
}
void sref_free(void* h) {
    Scene* s = (Scene*)h;
    delete s->gpu2; delete s->gpu4; delete s->cw; delete s;
}

// which: 0 = Wald nodes (32 bytes, usedNodes), 1 = primIdx (idxCount; sphere_lib.py keeps the sref_used_indices the leaves use), 2 = BVH_GPU
// nodes (64 bytes), 3 = BVH4_GPU blocks (16 bytes),
// 4 = CWBVH node blocks, 5 = CWBVH triangle blocks.  The wide layouts are built by the reference's own Build / BuildHQ of that class.
uint64_t sref_blob(void* h, int which, const void** out) {
    Scene* s = (Scene*)h;
    const uint32_t n = (uint32_t)(s->verts.size() / 3);
    switch (which) {
    case 0: *out = s->bvh.bvhNode; return s->bvh.usedNodes;
    case 1: *out = s->bvh.primIdx; return s->bvh.idxCount;
    case 2:
        if (!s->gpu2) { s->gpu2 = new BVH_GPU(); s->gpu2->ConvertFrom(s->bvh, false); }
        *out = s->gpu2->bvhNode; return s->gpu2->usedNodes;
    case 3:
        if (!s->gpu4) { s->gpu4 = new BVH4_GPU(); if (s->hq) s->gpu4->BuildHQ(s->verts.data(), n); else s->gpu4->Build(s->verts.data(), n); }
        *out = s->gpu4->bvh4Data; return s->gpu4->usedBlocks;
    case 4:
    case 5:
        if (!s->cw) { s->cw = new BVH8_CWBVH(); if (s->hq) s->cw->BuildHQ(s->verts.data(), n); else s->cw->Build(s->verts.data(), n); }
        if (which == 4) { *out = s->cw->bvh8Data; return s->cw->usedBlocks; }
        *out = s->cw->bvh8Tris; return (uint64_t)s->cw->bvh8.idxCount * 3;
    }
    *out = nullptr;
    return 0;
}

// BVH::IntersectSphere for spheres {x, y, z, r}; one byte per sphere
void sref_intersect_spheres(void* h, const float* spheres, uint64_t n, uint8_t* out) {
    const BVH& b = ((Scene*)h)->bvh;
    for (uint64_t i = 0; i < n; i++) {
        const float* p = spheres + i * 4;
        out[i] = b.IntersectSphere(bvhvec3(p[0], p[1], p[2]), p[3]) ? 1 : 0;
    }
}

// The same function over the tree with its root turned into one leaf of every primIdx entry the leaves use: the leaf's dist2 test against
// the root box, then the triangle test of every one of those triangles in primIdx order — the reference's arithmetic on every sphere,
// whatever its walk would do.  (BuildHQ's idxCount includes unused slack entries: the leaves' extent is what counts.)
uint32_t sref_used_indices(void* h) {
    const BVH& b = ((Scene*)h)->bvh;
    uint32_t used = 0;
    for (uint32_t i = 0; i < b.usedNodes; i++)
        if (b.bvhNode[i].triCount) used = std::max(used, b.bvhNode[i].leftFirst + b.bvhNode[i].triCount);
    return used;
}
void sref_intersect_spheres_flat(void* h, const float* spheres, uint64_t n, uint8_t* out) {
    BVH& b = ((Scene*)h)->bvh;
    const uint32_t used = sref_used_indices(h);
    const BVH::BVHNode keep = b.bvhNode[0];
    b.bvhNode[0].leftFirst = 0;
    b.bvhNode[0].triCount = used;
    for (uint64_t i = 0; i < n; i++) {
        const float* p = spheres + i * 4;
        out[i] = b.IntersectSphere(bvhvec3(p[0], p[1], p[2]), p[3]) ? 1 : 0;
    }
    b.bvhNode[0] = keep;
}

}  // extern "C"
