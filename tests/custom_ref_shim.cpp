// custom_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's custom-geometry BVH (BVH::Build( customGetAABB, n ), the custom
// branches of BVH::Intersect / IsOccluded and IntersectTLAS / IsOccludedTLAS) behind a C interface.
//
// Compiled at test time (tests/custom_lib.py: compile_ref_shim) from $TBVH_REFERENCE/tiny_bvh.h with the flags of oracle/Makefile, into the
// pytest temp dir; nothing of the reference is copied into the repository.  The callbacks below are this project's own: a sphere {x, y, z, r}
// per primitive, tested by the operations the anim demo's callback performs (the form that stays right for a direction of any length).  The
// callbacks take no context, so every sphere BLAS gets a slot of its own (at most kSlots per process).
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

struct Sph { bvhvec3 pos; float r; };
constexpr int kSlots = 8;
const Sph* g_sph[kSlots];

// This project's sphere test (DESIGN.md par. 12), component by component: the distance to the sphere along the normalised direction, and
// the direction's length to turn it into a ray parameter.  No fma is written here: the file is compiled with oracle/Makefile's flags, so the
// compiler's default contraction makes the fusions of the x86 build, which DESIGN.md par. 12 lists (read from this file's disassembly) and
// custom_sphere.h / tests/oracle_custom.c spell out.
struct Probe { float len, inv, dist; };
inline bool probeSphere(const Ray& ray, const Sph& s, Probe& p) {
    const float dx = ray.D.x, dy = ray.D.y, dz = ray.D.z;
    p.len = sqrtf(dx * dx + dy * dy + dz * dz);
    p.inv = 1.0f / p.len;
    const float ex = ray.O.x - s.pos.x, ey = ray.O.y - s.pos.y, ez = ray.O.z - s.pos.z;
    const float along = (ex * dx + ey * dy + ez * dz) * p.inv;
    const float excess = (ex * ex + ey * ey + ez * ez) - s.r * s.r;
    const float disc = along * along - excess;
    if (disc <= 0) return false;
    p.dist = -along - sqrtf(disc);
    return true;
}
// the callbacks: a candidate lies in front of the origin and below hit.t (a ray parameter, so compared after scaling by the length)
template <int S> __attribute__((noinline)) bool sphIntersect(Ray& ray, const unsigned prim) {
    Probe p;
    if (!probeSphere(ray, g_sph[S][prim], p)) return false;
    if (!(p.dist < ray.hit.t * p.len) || !(p.dist > 0)) return false;
    ray.hit.t = p.dist * p.inv;
    ray.hit.prim = prim;
    return true;
}
template <int S> __attribute__((noinline)) bool sphIsOccluded(const Ray& ray, const unsigned prim) {
    Probe p;
    return probeSphere(ray, g_sph[S][prim], p) && p.dist < ray.hit.t * p.len && p.dist > 0;
}
// the bounding box of a sphere: its centre -/+ r on every axis
template <int S> void sphAABB(const unsigned prim, bvhvec3& bmin, bvhvec3& bmax) {
    const Sph& s = g_sph[S][prim];
    bmin = bvhvec3(s.pos.x - s.r, s.pos.y - s.r, s.pos.z - s.r);
    bmax = bvhvec3(s.pos.x + s.r, s.pos.y + s.r, s.pos.z + s.r);
}

typedef bool (*IsectFn)(Ray&, const unsigned);
typedef bool (*OccFn)(const Ray&, const unsigned);
typedef void (*BoxFn)(const unsigned, bvhvec3&, bvhvec3&);
template <int... S> struct Tables {
    static constexpr IsectFn isect[] = {&sphIntersect<S>...};
    static constexpr OccFn occ[] = {&sphIsOccluded<S>...};
    static constexpr BoxFn box[] = {&sphAABB<S>...};
};
typedef Tables<0, 1, 2, 3, 4, 5, 6, 7> T8;

struct Blas {
    std::vector<Sph> spheres;   // sphere BLAS
    std::vector<bvhvec4> verts; // triangle BLAS
    BVH bvh;
    BVH_GPU* gpu2 = nullptr;
    int slot = -1;
};
bool g_used[kSlots];

struct Tlas {
    std::vector<BLASInstance> inst;
    std::vector<BVHBase*> blas;
    BVH tlas;
    BVH_GPU* gpu = nullptr;
};

// device ray (64 B) <-> host Ray: the first 64 bytes of tinybvh::Ray are the device record
inline void load(Ray& r, const char* src) { std::memset((void*)&r, 0, sizeof(Ray)); std::memcpy((void*)&r, src, 64); }
inline void store(char* dst, const Ray& r) { std::memcpy(dst + 44, (const char*)&r + 44, 20); }

}  // namespace

extern "C" {

// BVH::Build( customGetAABB, n ) over spheres {x, y, z, r} (copied); nullptr when every slot is taken
void* cref_build_spheres(const float* spheres16, uint32_t n) {
    int slot = -1;
    for (int i = 0; i < kSlots && slot < 0; i++) if (!g_used[i]) slot = i;
    if (slot < 0) return nullptr;
    Blas* b = new Blas();
    b->spheres.assign((const Sph*)spheres16, (const Sph*)spheres16 + n);
    b->slot = slot; g_used[slot] = true;
    g_sph[slot] = b->spheres.data();
    b->bvh.Build(T8::box[slot], n);
    b->bvh.customIntersect = T8::isect[slot];
    b->bvh.customIsOccluded = T8::occ[slot];
    return b;
}
// BVH::Build over n_tris x 3 bvhvec4 vertices (copied): a triangle BLAS for a mixed TLAS
void* cref_build_tris(const float* verts16, uint32_t nTris) {
    Blas* b = new Blas();
    b->verts.assign((const bvhvec4*)verts16, (const bvhvec4*)verts16 + (size_t)nTris * 3);
    b->bvh.Build(b->verts.data(), nTris);
    return b;
}
void cref_free(void* h) {
    Blas* b = (Blas*)h;
    if (b->slot >= 0) g_used[b->slot] = false;
    delete b->gpu2; delete b;
}
// which: 0 = Wald nodes (32 bytes, usedNodes), 1 = primIdx (idxCount), 2 = BVH_GPU::ConvertFrom nodes (64 bytes)
uint64_t cref_blob(void* h, int which, const void** out) {
    Blas* b = (Blas*)h;
    if (which == 0) { *out = b->bvh.bvhNode; return b->bvh.usedNodes; }
    if (which == 1) { *out = b->bvh.primIdx; return b->bvh.idxCount; }
    if (!b->gpu2) { b->gpu2 = new BVH_GPU(); b->gpu2->ConvertFrom(b->bvh, false); }
    *out = b->gpu2->bvhNode; return b->gpu2->usedNodes;
}
void cref_intersect(void* h, void* rays, uint64_t n) {
    const BVH& bvh = ((Blas*)h)->bvh;
    char* p = (char*)rays;
    for (uint64_t i = 0; i < n; i++, p += 64) { Ray r; load(r, p); bvh.Intersect(r); store(p, r); }
}
void cref_occluded(void* h, const void* rays, uint64_t n, uint8_t* out) {
    const BVH& bvh = ((Blas*)h)->bvh;
    const char* p = (const char*)rays;
    for (uint64_t i = 0; i < n; i++, p += 64) { Ray r; load(r, p); out[i] = bvh.IsOccluded(r) ? 1 : 0; }
}

// BVH::Build( BLASInstance*, ... ) over BLASes made above; instances192 is updated in place (bounds, inverse transforms)
void* cref_tlas_build(void* instances192, uint32_t nInst, void** blas, uint32_t nBlas) {
    Tlas* t = new Tlas;
    t->inst.resize(nInst);
    std::memcpy((void*)t->inst.data(), instances192, (size_t)nInst * 192);
    for (uint32_t i = 0; i < nBlas; i++) t->blas.push_back(&((Blas*)blas[i])->bvh);
    t->tlas.Build(t->inst.data(), nInst, t->blas.data(), nBlas);
    std::memcpy(instances192, (void*)t->inst.data(), (size_t)nInst * 192);
    return t;
}
void cref_tlas_free(void* h) { Tlas* t = (Tlas*)h; delete t->gpu; delete t; }
// 0 = BVH_GPU::ConvertFrom nodes of the TLAS (64 bytes), 1 = its primIdx, 2 = its Wald nodes
uint64_t cref_tlas_blob(void* h, int which, const void** out) {
    Tlas* t = (Tlas*)h;
    if (!t->gpu) { t->gpu = new BVH_GPU(); t->gpu->ConvertFrom(t->tlas, false); }
    if (which == 0) { *out = t->gpu->bvhNode; return t->gpu->usedNodes; }
    if (which == 1) { *out = t->tlas.primIdx; return t->tlas.idxCount; }
    *out = t->tlas.bvhNode; return t->tlas.usedNodes;
}
void cref_tlas_intersect(void* h, void* rays, uint64_t n) {
    Tlas* t = (Tlas*)h;
    char* p = (char*)rays;
    for (uint64_t i = 0; i < n; i++, p += 64) { Ray r; load(r, p); t->tlas.Intersect(r); store(p, r); }
}
void cref_tlas_occluded(void* h, const void* rays, uint64_t n, uint8_t* out) {
    Tlas* t = (Tlas*)h;
    const char* p = (const char*)rays;
    for (uint64_t i = 0; i < n; i++, p += 64) { Ray r; load(r, p); out[i] = t->tlas.IsOccluded(r) ? 1 : 0; }
}

}  // extern "C"
