// sbvhbuild_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's spatial-split builder over an index buffer behind a C interface:
// BVH::BuildHQ( slice, indices, n ) with threadedBuild = false.  (The flat form goes through oracle/_ref: ref_build( .., hq = 1, threaded ).)
//
// Compiled at test time (tests/sbvhbuild_lib.py: compile_ref_shim) from $TBVH_REFERENCE/tiny_bvh.h with the flags of oracle/Makefile, into the
// pytest temp dir; nothing of the reference is copied into the repository.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#define TINYBVH_IMPLEMENTATION
#include "tiny_bvh.h"

using namespace tinybvh;

namespace {
struct SbvhRef {
    void* verts = nullptr;   // 64-byte aligned copy with 16 spare bytes behind it (the reference loads whole bvhvec4s)
    std::vector<uint32_t> idx;
    BVH bvh;
    ~SbvhRef() { free(verts); }
};
}  // namespace

extern "C" {

// verts: nVerts bvhvec4; indices: 3 per triangle
void* qref_build(const void* verts, uint32_t nVerts, const uint32_t* indices, uint32_t nTris) {
    SbvhRef* m = new SbvhRef;
    const size_t bytes = ((size_t)nVerts * 16 + 16 + 63) & ~(size_t)63;
    m->verts = aligned_alloc(64, bytes);
    std::memset(m->verts, 0, bytes);
    std::memcpy(m->verts, verts, (size_t)nVerts * 16);
    m->bvh.threadedBuild = false;
    m->idx.assign(indices, indices + (size_t)nTris * 3);
    m->bvh.BuildHQ(bvhvec4slice((const bvhvec4*)m->verts, nVerts, 16), m->idx.data(), nTris);
    return m;
}
void qref_free(void* h) { delete (SbvhRef*)h; }
// 0 = Wald nodes (32 bytes, usedNodes), 1 = primIdx (idxCount entries; only the leaves' references are defined)
uint64_t qref_blob(void* h, int which, const void** out) {
    SbvhRef* m = (SbvhRef*)h;
    if (which == 1) { *out = m->bvh.primIdx; return m->bvh.idxCount; }
    *out = m->bvh.bvhNode; return m->bvh.usedNodes;
}

}  // extern "C"
