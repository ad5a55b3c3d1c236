// voxel_edit_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's VoxelSet::Set / UpdateTopGrid / GetNormal behind a C interface.
//
// Compiled at test time (tests/voxel_edit_lib.py) from $TBVH_REFERENCE/tiny_bvh.h with the flags of oracle/Makefile plus -DNDEBUG, into the
// pytest temp dir; nothing of the reference is copied into the repository.  The brick map is private in the reference; the standard headers
// are included first and `private` is then read as `public` while the reference header is compiled (as tests/voxel_ref_shim.cpp does).
// vscene_* / vedit_voxelize_hits state the scene-to-voxels loop of tiny_bvh_foliage.cpp:222-258 in the project's own words, calling only BVH::Build /
// BVH::Intersect and the Ray constructor: the hits of every axis ray in loop order.  What becomes of a hit (alpha, colour, Set) is done by the caller
// with the library's CPU shading twin and vedit_set.
// vedit_normals is also where the contraction of GetNormal's ( O + t * D ) is read from: DESIGN.md par. 21 quotes this file's object code.
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

extern "C" {

void* vedit_new() { return new VoxelSet(); }
void vedit_free(void* h) { delete (VoxelSet*)h; }

// xyzv: n records of {x, y, z, value}, set in the order given
void vedit_set(void* h, const uint32_t* xyzv, uint64_t n) {
    VoxelSet* v = (VoxelSet*)h;
    for (uint64_t i = 0; i < n; i++) v->Set(xyzv[i * 4], xyzv[i * 4 + 1], xyzv[i * 4 + 2], xyzv[i * 4 + 3]);
}
void vedit_update_top_grid(void* h) { ((VoxelSet*)h)->UpdateTopGrid(); }

// the three arrays; returns the number of bricks in use (freeBrickPtr: brick 0 included, never written)
uint32_t vedit_arrays(void* h, const uint32_t** grid, const uint32_t** brick, const uint32_t** top) {
    const VoxelSet* v = (const VoxelSet*)h;
    *grid = v->grid; *brick = v->brick; *top = v->topGrid;
    return v->freeBrickPtr;
}

// VoxelSet::GetNormal over records of `stride` bytes whose first 64 are the library's ray record; out: 4 floats per ray (normal, 0).
// GetNormal reads O, D and hit.t only, and no member of the set.
__attribute__((noinline)) void vedit_normals(void* h, const void* rays, uint32_t stride, uint64_t n, float* out) {
    const VoxelSet* v = (const VoxelSet*)h;
    for (uint64_t i = 0; i < n; i++) {
        Ray r;
        std::memcpy((void*)&r, (const char*)rays + i * stride, 64);
        const bvhvec3 N = v->GetNormal(r);
        out[i * 4] = N.x; out[i * 4 + 1] = N.y; out[i * 4 + 2] = N.z; out[i * 4 + 3] = 0;
    }
}

// ---- the traced scene of the voxelise goldens: one BVH over triangles, or a TLAS of instances over such BVHs ---------------------------------
struct VScene {
    BVH bvh;                             // the BLAS, or the TLAS
    std::vector<bvhvec4> verts;
    std::vector<BLASInstance> inst;
    std::vector<BVHBase*> blas;
};
void* vscene_blas(const float* verts16, uint32_t nTris) {
    VScene* s = new VScene();
    s->verts.assign((const bvhvec4*)verts16, (const bvhvec4*)verts16 + (size_t)nTris * 3);
    s->bvh.Build(s->verts.data(), nTris);
    return s;
}
// instances192 is updated in place by BLASInstance::Update (invTransform, bounds)
void* vscene_tlas(void* instances192, uint32_t nInst, void** blasScenes, uint32_t nBlas) {
    VScene* s = new VScene();
    s->inst.assign((BLASInstance*)instances192, (BLASInstance*)instances192 + nInst);
    for (uint32_t i = 0; i < nBlas; i++) s->blas.push_back(&((VScene*)blasScenes[i])->bvh);
    s->bvh.Build(s->inst.data(), nInst, s->blas.data(), nBlas);
    std::memcpy(instances192, s->inst.data(), (size_t)nInst * sizeof(BLASInstance));
    return s;
}
void vscene_free(void* h) { delete (VScene*)h; }
void vscene_bounds(void* h, float* out6) {
    const BVH& b = ((VScene*)h)->bvh;
    out6[0] = b.aabbMin.x; out6[1] = b.aabbMin.y; out6[2] = b.aabbMin.z; out6[3] = b.aabbMax.x; out6[4] = b.aabbMax.y; out6[5] = b.aabbMax.z;
}

// the loop: 3 x 256^2 axis rays, each marched hit by hit until hit.t >= 10000 (or hitCap hits: the reference's loop has no cap).  Per hit, in loop
// order: the ray record as Intersect left it (64 bytes, O the origin it was traced from) and four words { a, x, y, P[a] }.  hitsPerRay: 3 x 65536
// counts.  Returns the number of hits (those beyond `cap` are counted, not stored).
__attribute__((noinline)) uint64_t vedit_voxelize_hits(void* h, const float* bminIn, float maxSize, const float* extIn, uint32_t hitCap, uint64_t cap, void* outRays64,
                                                       uint32_t* outMeta, uint32_t* hitsPerRay) {
    const BVH& tlas = ((VScene*)h)->bvh;
    const bvhvec3 bmin(bminIn[0], bminIn[1], bminIn[2]), ext(extIn[0], extIn[1], extIn[2]);
    uint64_t n = 0;
    for (int a = 0; a < 3; a++) {
        const int u = (a + 1) % 3, v = (a + 2) % 3;
        const float reciDim = 1.0f / (float)VoxelSet::objectDim;
        const float reciExt = 1.0f / ext[a];
        bvhvec3 D(0);
        D[a] = 1;
        for (int x = 0; x < VoxelSet::objectDim; x++) for (int y = 0; y < VoxelSet::objectDim; y++) {
            const float fx = (float)x * reciDim, fy = (float)y * reciDim;
            bvhvec3 O;
            O[a] = bmin[a] - 0.0001f, O[u] = bmin[u] + maxSize * fx, O[v] = bmin[v] + maxSize * fy;
            Ray ray(O, D);
            uint32_t hits = 0;
            while (hits < hitCap) {
                tlas.Intersect(ray);
                if (ray.hit.t >= 10000) break;
                const bvhvec3 I = ray.O + ray.D * ray.hit.t;
                if (n < cap) {
                    std::memcpy((char*)outRays64 + n * 64, (const void*)&ray, 64);
                    uint32_t* m = outMeta + n * 4;
                    m[0] = (uint32_t)a; m[1] = (uint32_t)x; m[2] = (uint32_t)y;
                    m[3] = (uint32_t)(int)((float)VoxelSet::objectDim * (I[a] - bmin[a]) * reciExt);
                }
                n++; hits++;
                ray.O = I + ray.D * 0.0001f, ray.hit.t = 1e34f;
            }
            hitsPerRay[(a * 256 + x) * 256 + y] = hits;
        }
    }
    return n;
}

}  // extern "C"
