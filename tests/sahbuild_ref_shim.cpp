// sahbuild_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's default builder behind a C interface: BVH::Build( verts, n ) and
// BVH::Build( slice, indices, n ) with threadedBuild = false (the non-threaded node numbering), optionally followed by BVH::SplitLeafs( k ).
//
// Compiled at test time (tests/sahbuild_lib.py: compile_ref_shim) from $TBVH_REFERENCE/tiny_bvh.h with the flags of oracle/Makefile, into the
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
struct SahRef {
    void* verts = nullptr;   // 64-byte aligned copy with 16 spare bytes behind it (the reference loads whole bvhvec4s)
    std::vector<uint32_t> idx;
    BVH bvh;
    ~SahRef() { free(verts); }
};
}  // namespace

extern "C" {

// verts: nVerts bvhvec4; indices: 3 per triangle, or null: triangle i = vertices 3i, 3i + 1, 3i + 2.  splitLeafs > 0: BVH::SplitLeafs( splitLeafs ) afterwards.
void* sref_build(const void* verts, uint32_t nVerts, const uint32_t* indices, uint32_t nTris, uint32_t splitLeafs) {
    SahRef* m = new SahRef;
    const size_t bytes = ((size_t)nVerts * 16 + 16 + 63) & ~(size_t)63;
    m->verts = aligned_alloc(64, bytes);
    std::memset(m->verts, 0, bytes);
    std::memcpy(m->verts, verts, (size_t)nVerts * 16);
    m->bvh.threadedBuild = false;
    if (indices) {
        m->idx.assign(indices, indices + (size_t)nTris * 3);
        m->bvh.Build(bvhvec4slice((const bvhvec4*)m->verts, nVerts, 16), m->idx.data(), nTris);
    } else m->bvh.Build((const bvhvec4*)m->verts, nTris);
    if (splitLeafs) m->bvh.SplitLeafs(splitLeafs);
    return m;
}
void sref_free(void* h) { delete (SahRef*)h; }
// 0 = Wald nodes (32 bytes, usedNodes), 1 = primIdx (idxCount)
uint64_t sref_blob(void* h, int which, const void** out) {
    SahRef* m = (SahRef*)h;
    if (which == 1) { *out = m->bvh.primIdx; return m->bvh.idxCount; }
    *out = m->bvh.bvhNode; return m->bvh.usedNodes;
}

}  // extern "C"
