// boxbuild_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's three builds over BOXES behind a C interface, each with
// threadedBuild = false (the non-threaded node numbering):
//   which 0   BVH::BuildAABB( aabbs, n )                          n x {min bvhvec4, max bvhvec4}
//   which 1   BVH::Build( customGetAABB, n )                      with the demos' sphereAABB callback over n x {x, y, z, r}
//   which 2   BVH::Build( BLASInstance*, n, 0, 0 )                over records already updated (the null blasList form)
//   which 3   BVH_GPU::Build( BLASInstance*, n, 0, 0 )            the same tree as Aila-Laine nodes (BVH_GPU::ConvertFrom)
//
// Compiled at test time (tests/boxbuild_lib.py: compile_ref_shim) from $TBVH_REFERENCE/tiny_bvh.h with the flags of oracle/Makefile, into the
// pytest temp dir; nothing of the reference is copied into the repository.
#include <algorithm>
#include <atomic>
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <malloc.h>
#include <math.h>
#include <mutex>
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
struct BoxRef {
    void* data = nullptr;   // 64-byte aligned copy of the input with 64 spare bytes behind it
    BVH bvh;
    BVH_GPU gpu;
    bool isGpu = false;
    ~BoxRef() { free(data); }
};

const bvhvec4* g_spheres = nullptr;   // what the callback reads (one build at a time: the tests are sequential)
void sphereAABB(const unsigned i, bvhvec3& bmin, bvhvec3& bmax) {
    const bvhvec3 pos(g_spheres[i].x, g_spheres[i].y, g_spheres[i].z);
    bmin = pos - bvhvec3(g_spheres[i].w), bmax = pos + bvhvec3(g_spheres[i].w);
}
}  // namespace

extern "C" {

void* bref_build(int which, const void* data, uint32_t n) {
    static_assert(sizeof(BLASInstance) == 192, "BLASInstance is 192 bytes");
    BoxRef* m = new BoxRef;
    const size_t rec = which == 0 ? 32 : which == 1 ? 16 : 192;
    const size_t bytes = ((size_t)n * rec + 64 + 63) & ~(size_t)63;
    m->data = aligned_alloc(64, bytes);
    std::memset(m->data, 0, bytes);
    std::memcpy(m->data, data, (size_t)n * rec);
    m->bvh.threadedBuild = false;
    if (which == 0) m->bvh.BuildAABB((const bvhvec4*)m->data, n);
    else if (which == 1) { g_spheres = (const bvhvec4*)m->data; m->bvh.Build(&sphereAABB, n); g_spheres = nullptr; }
    else if (which == 2) m->bvh.Build((BLASInstance*)m->data, n, 0, 0);
    else { m->isGpu = true; m->gpu.bvh.threadedBuild = false; m->gpu.Build((BLASInstance*)m->data, n, 0, 0); }
    return m;
}
void bref_free(void* h) { delete (BoxRef*)h; }
// 0 = nodes (Wald, 32 bytes, usedNodes; which 3: Aila-Laine, 64 bytes, usedNodes), 1 = primIdx (idxCount)
uint64_t bref_blob(void* h, int what, const void** out) {
    BoxRef* m = (BoxRef*)h;
    const BVH& b = m->isGpu ? m->gpu.bvh : m->bvh;
    if (what == 1) { *out = b.primIdx; return b.idxCount; }
    if (m->isGpu) { *out = m->gpu.bvhNode; return m->gpu.usedNodes; }
    *out = b.bvhNode; return b.usedNodes;
}

}  // extern "C"
