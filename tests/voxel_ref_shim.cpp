// voxel_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's VoxelSet behind a C interface.
//
// Compiled at test time (tests/voxel_lib.py: ref_shim) from $TBVH_REFERENCE/tiny_bvh.h with the flags of oracle/Makefile plus -DNDEBUG, into
// the pytest temp dir; nothing of the reference is copied into the repository.  -DNDEBUG leaves the arithmetic alone; it disarms the TLAS
// asserts, which do not list LAYOUT_VOXELSET (tiny_bvh.h:3339-3340, 3489-3490).  The VoxelSet constructor leaves `layout` UNDEFINED
// (tiny_bvh.h:3775-3784), so a TLAS would skip every voxel BLAS; it is set to LAYOUT_VOXELSET here by hand.
// The brick map is private in the reference; the standard headers are included first and `private` is then read as `public` while the
// reference header is compiled, so the arrays can be handed out as they are.
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

static_assert(sizeof(BLASInstance) == 192, "BLASInstance is 192 bytes");
static_assert(INST_IDX_BITS == 32, "the shim assumes the default INST_IDX_BITS");

namespace {
// the first 64 bytes of a tinybvh::Ray are the library's ray record; the rest (the reference's own bookkeeping) stays as the constructor left it
void loadRay(Ray& r, const void* rec) { std::memcpy((void*)&r, rec, 64); }
void storeRay(void* rec, const Ray& r) { std::memcpy(rec, (const void*)&r, 64); }

struct Tlas {
    BVH bvh;
    std::vector<BVHBase*> blas;
    std::vector<BLASInstance> inst;
    BVH_GPU* gpu = nullptr;
};
}  // namespace

extern "C" {

void* vref_new() {
    VoxelSet* v = new VoxelSet();
    v->layout = BVHBase::LAYOUT_VOXELSET;   // (defect 1: the constructor does not)
    return v;
}
void vref_free(void* h) { delete (VoxelSet*)h; }

// xyzv: n records of {x, y, z, value}, set in the order given
void vref_set(void* h, const uint32_t* xyzv, uint64_t n) {
    VoxelSet* v = (VoxelSet*)h;
    for (uint64_t i = 0; i < n; i++) v->Set(xyzv[i * 4], xyzv[i * 4 + 1], xyzv[i * 4 + 2], xyzv[i * 4 + 3]);
}
void vref_update_top_grid(void* h) { ((VoxelSet*)h)->UpdateTopGrid(); }

// the three arrays; returns the number of bricks in use (freeBrickPtr: brick 0 included, never written)
uint32_t vref_arrays(void* h, const uint32_t** grid, const uint32_t** brick, const uint32_t** top) {
    const VoxelSet* v = (const VoxelSet*)h;
    *grid = v->grid; *brick = v->brick; *top = v->topGrid;
    return v->freeBrickPtr;
}
int vref_object_dim() { return VoxelSet::objectDim; }

// VoxelSet::Intersect / IsOccluded over 64-byte records (in place / one byte per ray)
void vref_intersect(void* h, void* rays, uint64_t n) {
    const VoxelSet* v = (const VoxelSet*)h;
    for (uint64_t i = 0; i < n; i++) { Ray r; loadRay(r, (char*)rays + i * 64); v->Intersect(r); storeRay((char*)rays + i * 64, r); }
}
void vref_occluded(void* h, const void* rays, uint64_t n, uint8_t* out) {
    const VoxelSet* v = (const VoxelSet*)h;
    for (uint64_t i = 0; i < n; i++) { Ray r; loadRay(r, (const char*)rays + i * 64); out[i] = v->IsOccluded(r) ? 1 : 0; }
}

// BVH::Build( BLASInstance*, ... ) over voxel sets (tiny_bvh.h:2221-2259); instances192 is updated in place by BLASInstance::Update
void* vref_tlas_build(void* instances192, uint32_t nInst, void** sets, uint32_t nSets) {
    Tlas* t = new Tlas();
    t->inst.assign((BLASInstance*)instances192, (BLASInstance*)instances192 + nInst);
    for (uint32_t i = 0; i < nSets; i++) t->blas.push_back((BVHBase*)(VoxelSet*)sets[i]);
    t->bvh.Build(t->inst.data(), nInst, t->blas.data(), nSets);
    std::memcpy(instances192, t->inst.data(), (size_t)nInst * sizeof(BLASInstance));
    return t;
}
void vref_tlas_free(void* h) { Tlas* t = (Tlas*)h; delete t->gpu; delete t; }
// 0: the TLAS in BVH_GPU format (BVH_GPU::ConvertFrom, 64-byte nodes), 1: its instance indices, 2: the Wald-format nodes (32 bytes)
uint64_t vref_tlas_blob(void* h, int which, const void** out) {
    Tlas* t = (Tlas*)h;
    if (!t->gpu) { t->gpu = new BVH_GPU(); t->gpu->ConvertFrom(t->bvh, false); }
    if (which == 0) { *out = t->gpu->bvhNode; return t->gpu->usedNodes; }
    if (which == 1) { *out = t->bvh.primIdx; return t->bvh.idxCount; }
    *out = t->bvh.bvhNode; return t->bvh.usedNodes;
}
void vref_tlas_intersect(void* h, void* rays, uint64_t n) {
    Tlas* t = (Tlas*)h;
    for (uint64_t i = 0; i < n; i++) { Ray r; loadRay(r, (char*)rays + i * 64); t->bvh.Intersect(r); storeRay((char*)rays + i * 64, r); }
}
void vref_tlas_occluded(void* h, const void* rays, uint64_t n, uint8_t* out) {
    Tlas* t = (Tlas*)h;
    for (uint64_t i = 0; i < n; i++) { Ray r; loadRay(r, (const char*)rays + i * 64); out[i] = t->bvh.IsOccluded(r) ? 1 : 0; }
}

}  // extern "C"
