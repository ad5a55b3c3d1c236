// custom_double_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's BVH_Double over custom geometry (BVH_Double::Build( customGetAABB, n ),
// the custom branch of BVH_Double::Intersect, IntersectTLAS over BLASInstanceEx records) behind a C interface.
//
// Compiled at test time (tests/custom_double_lib.py: compile_ref_shim) from $TBVH_REFERENCE/tiny_bvh.h, without contraction (-ffp-contract=off: the
// fp64 path rounds once per operation), into the pytest temp dir; nothing of the reference is copied into the repository.  The callbacks below are
// this project's own: a sphere {pos, r} of doubles per primitive, tested by the operations of include/tinybvh_amd.h ("double precision, custom
// geometry"), component by component.  The callbacks take no context, so every sphere BLAS gets a slot of its own (at most kSlots per process).
// The occlusion entries (cdref_occluded, cdref_tlas_occluded) are for triangle scenes only: over custom geometry the reference discards its
// callback's answer (tiny_bvh.h:8278-8279), which the library does not restate.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define private public
#define TINYBVH_IMPLEMENTATION
#include "tiny_bvh.h"
#undef private

using namespace tinybvh;

namespace {

struct Sph { double x, y, z, r; };
constexpr int kSlots = 4;
const Sph* g_sph[kSlots];
bool g_used[kSlots];

// the distance to the sphere along the normalised direction, and the direction's length to turn it into a ray parameter
template <int S> __attribute__((noinline)) bool sphIntersect(RayEx& ray, const uint64_t prim) {
    const Sph& s = g_sph[S][prim];
    const double dx = ray.D.x, dy = ray.D.y, dz = ray.D.z;
    const double len = sqrt(dx * dx + dy * dy + dz * dz);
    const double inv = 1.0 / len;
    const double ex = ray.O.x - s.x, ey = ray.O.y - s.y, ez = ray.O.z - s.z;
    const double along = (ex * dx + ey * dy + ez * dz) * inv;
    const double excess = (ex * ex + ey * ey + ez * ez) - s.r * s.r;
    const double disc = along * along - excess;
    if (disc <= 0) return false;
    const double dist = -along - sqrt(disc);
    if (!(dist < ray.hit.t * len) || !(dist > 0)) return false;
    ray.hit.t = dist * inv;
    ray.hit.prim = prim;
    return true;
}
template <int S> bool sphIsOccluded(const RayEx& ray, const uint64_t prim) { RayEx r = ray; return sphIntersect<S>(r, prim); }
template <int S> void sphAABB(const uint64_t prim, bvhdbl3& bmin, bvhdbl3& bmax) {
    const Sph& s = g_sph[S][prim];
    bmin = bvhdbl3(s.x - s.r, s.y - s.r, s.z - s.r);
    bmax = bvhdbl3(s.x + s.r, s.y + s.r, s.z + s.r);
}

typedef bool (*IsectFn)(RayEx&, const uint64_t);
typedef bool (*OccFn)(const RayEx&, const uint64_t);
typedef void (*BoxFn)(const uint64_t, bvhdbl3&, bvhdbl3&);
template <int... S> struct Tables {
    static constexpr IsectFn isect[] = {&sphIntersect<S>...};
    static constexpr OccFn occ[] = {&sphIsOccluded<S>...};
    static constexpr BoxFn box[] = {&sphAABB<S>...};
};
typedef Tables<0, 1, 2, 3> T4;

struct Blas {
    std::vector<Sph> spheres;     // sphere BLAS
    std::vector<bvhdbl3> verts;   // triangle BLAS
    BVH_Double bvh;
    int slot = -1;
};
struct Tlas {
    std::vector<BLASInstanceEx> inst;
    std::vector<BVH_Double*> blas;
    BVH_Double tlas;
};

}  // namespace

static_assert(sizeof(RayEx) == 128 && sizeof(BLASInstanceEx) == 320 && sizeof(BVH_Double::BVHNode) == 64, "the records the library documents");

extern "C" {

// BVH_Double::Build( customGetAABB, n ) over spheres {x, y, z, r} (copied); nullptr when every slot is taken
void* cdref_build_spheres(const double* spheres32, uint64_t n) {
    int slot = -1;
    for (int i = 0; i < kSlots && slot < 0; i++) if (!g_used[i]) slot = i;
    if (slot < 0) return nullptr;
    Blas* b = new Blas();
    b->spheres.assign((const Sph*)spheres32, (const Sph*)spheres32 + n);
    b->slot = slot; g_used[slot] = true;
    g_sph[slot] = b->spheres.data();
    b->bvh.Build(T4::box[slot], n);
    b->bvh.customIntersect = T4::isect[slot];
    b->bvh.customIsOccluded = T4::occ[slot];
    return b;
}
// BVH_Double::Build over n_tris x 3 bvhdbl3 vertices (copied): a triangle BLAS for a mixed TLAS
void* cdref_build_tris(const double* verts, uint64_t nTris) {
    Blas* b = new Blas();
    b->verts.assign((const bvhdbl3*)verts, (const bvhdbl3*)verts + nTris * 3);
    b->bvh.Build(b->verts.data(), nTris);
    return b;
}
void cdref_free(void* h) {
    Blas* b = (Blas*)h;
    if (b->slot >= 0) g_used[b->slot] = false;
    delete b;
}
// which: 0 = bvhNode (64 bytes, usedNodes), 1 = primIdx (idxCount)
uint64_t cdref_blob(void* h, int which, const void** out) {
    Blas* b = (Blas*)h;
    if (which == 0) { *out = b->bvh.bvhNode; return b->bvh.usedNodes; }
    *out = b->bvh.primIdx; return b->bvh.idxCount;
}
void cdref_intersect(void* h, void* rays128, uint64_t n) {
    const BVH_Double& bvh = ((Blas*)h)->bvh;
    RayEx* r = (RayEx*)rays128;
    for (uint64_t i = 0; i < n; i++) bvh.Intersect(r[i]);
}

// BVH_Double::Build( BLASInstanceEx*, ... ) over BLASes made above; instances320 is updated in place (bounds, inverse transforms)
void* cdref_tlas_build(void* instances320, uint64_t nInst, void** blas, uint64_t nBlas) {
    Tlas* t = new Tlas;
    t->inst.resize(nInst);
    std::memcpy((void*)t->inst.data(), instances320, nInst * 320);
    for (uint64_t i = 0; i < nBlas; i++) t->blas.push_back(&((Blas*)blas[i])->bvh);
    t->tlas.Build(t->inst.data(), nInst, t->blas.data(), nBlas);
    std::memcpy(instances320, (void*)t->inst.data(), nInst * 320);
    return t;
}
void cdref_tlas_free(void* h) { delete (Tlas*)h; }
uint64_t cdref_tlas_blob(void* h, int which, const void** out) {
    Tlas* t = (Tlas*)h;
    if (which == 0) { *out = t->tlas.bvhNode; return t->tlas.usedNodes; }
    *out = t->tlas.primIdx; return t->tlas.idxCount;
}
void cdref_tlas_intersect(void* h, void* rays128, uint64_t n) {
    Tlas* t = (Tlas*)h;
    RayEx* r = (RayEx*)rays128;
    for (uint64_t i = 0; i < n; i++) t->tlas.Intersect(r[i]);
}

// BVH_Double::IsOccluded of a triangle BLAS (for triangle scenes only: the custom branch discards its callback's answer)
void cdref_occluded(void* h, const void* rays128, uint64_t n, uint8_t* out) {
    const BVH_Double& bvh = ((Blas*)h)->bvh;
    const RayEx* r = (const RayEx*)rays128;
    for (uint64_t i = 0; i < n; i++) out[i] = bvh.IsOccluded(r[i]) ? 1 : 0;
}
// BVH_Double::IsOccluded of a TLAS over triangle BLASes.  IsOccludedTLAS hands the BLASes a RayEx whose hit.t it never sets (tiny_bvh.h:8322): what the
// BLAS walk compares against is whatever the stack held.  fillStack writes the ray's own hit.t into every slot of the stack the call is about to use, so
// that read gives the value IntersectTLAS copies there (tmp.hit = ray.hit).  Whether that took is checked against the reference itself (tests/test_double_edges_host.py: a ray is occluded iff the closest
// hit of the reference's Intersect lies before tmax), so a compiler that keeps the slot elsewhere fails a test instead of passing one.
__attribute__((noinline)) void fillStack(double v) {
    volatile double slots[8192];
    for (int i = 0; i < 8192; i++) slots[i] = v;
}
void cdref_tlas_occluded(void* h, const void* rays128, uint64_t n, uint8_t* out) {
    Tlas* t = (Tlas*)h;
    const RayEx* r = (const RayEx*)rays128;
    for (uint64_t i = 0; i < n; i++) {
        fillStack(r[i].hit.t);
        out[i] = t->tlas.IsOccluded(r[i]) ? 1 : 0;
    }
}

}  // extern "C"
