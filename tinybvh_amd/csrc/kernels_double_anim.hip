// kernels_double_anim.hip — BVH_Double scenes that move, for gfx950 (MI355X), in fp64: the per-frame TLAS rebuild and the BLAS refit.
//
// TLAS rebuild.  Replaces, for a TLAS_Double that already lives on the GPU, the host work of the reference's double frame loop
// (tiny_bvh_anim_double.cpp:110: "just move build to Tick if instance transforms are not static"): BLASInstanceEx::Update for every
// instance (tiny_bvh.h:8432-8472: invert the transform, world box of the 8 transformed BLAS-box corners) and
// BVH_Double::Build( BLASInstanceEx*, ... ) (tiny_bvh.h:7955-...).  The instance records keep the reference's 320-byte format and the
// result is a BVH_Double node array + instance index list, exactly what k_double traverses.  Five steps; the encoding of the bounds, the keys,
// the prefix lengths and the Karras range search are lbvh.h's, shared with the fp32 builders:
//   1. instance update, one thread per instance: the expressions of capi_double.hip: updateInstanceDbl, operation for operation (the
//      Makefile's -ffp-contract=off keeps them uncontracted), so device-updated and host-updated records are bit-identical.  The BLAS box
//      is node 0 of the BLAS (tiny_bvh.h:8133: aabbMin / aabbMax = bvhNode[0]'s), read through the BlasDbl descriptors: no bounds argument.
//   2. 63-bit Morton keys, 21 bits per axis, of the box centres relative to the centre bounds, computed in double.  (30 bits over an
//      extent of 1e7 units are cells of 1e4 units: a cluster of nearby instances far from the rest would share ONE key.)  The centre
//      bounds are reduced per wave, then one set of 64-bit atomicMin / atomicMax per wave on an order-preserving encoding.
//   3. hipcub::DeviceRadixSort::SortPairs on the uint64_t keys.
//   4. Karras 2012 topology in one pass; equal keys are told apart by their position.
//   5. nodes, bottom-up: leaf threads climb, the second thread to reach an interior node owns it (one atomic flag per node), the first
//      returns: nothing waits or spins.  Numbering: root = 0, the children of Karras interior node i at 1 + 2 i and 2 + 2 i — 2 n - 1
//      nodes without an unused slot, as the library's host builder numbers them.  One leaf per instance.
// The tree is an LBVH instead of the host builder's binned-SAH tree: a different but valid TLAS — hit records do not depend on the TLAS
// shape (device_common.h: hit_wins_dbl), up to rays that a box of one tree culls within the eight-ulp slack and the other's does not.
//
// Sphere BLAS build (tbvh_build_device_custom_spheres_double / tbvh_rebuild_custom_spheres_double_device): steps 2-5 with a second box source, the
// boxes pos -/+ r of spheres {pos, r}; the same numbering (2 n - 1 nodes, root 0, one sphere per leaf, n = 1 a leaf root), the leaf thread also
// writes the 48-byte record the traversal reads.
//
// BLAS refit.  The reference has no BVH_Double::Refit; this is the fp64 twin of kernels_refit.hip: same topology, new vertices.  One
// thread per leaf rewrites its TriDbl records ({v0, e1 = v1 - v0, e2 = v2 - v0, prim}: the subtractions of k_gather_tris_dbl; prim comes
// from the record), takes the leaf box from the three VERTICES (v0 + e1 would round) and climbs by parent index under the same
// second-arrival rule; no stack, so chains of any depth work.  BVH_Double nodes carry no parent index: k_parents_dbl fills a parent array
// and the list of leaf nodes once per scene, walking the tree from the root (slots the root does not reach — the reference's builder
// leaves node 1 unused — are never read).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdio>

#include "custom_sphere_dbl.h"
#include "dev_buf.h"
#include "device_common.h"
#include "kernels.h"
#include "lbvh.h"

namespace tbvh {

namespace {

constexpr double kDblFar = 1e300;   // BVH_DBL_FAR, tiny_bvh.h:145
constexpr uint32_t kNoParent = 0xffffffffu;

__device__ __forceinline__ double ld_agent(const double* p) {   // bypass this CU's (non-coherent) L1: a sibling on another CU wrote it
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// node `out` = the union of its two children c and c + 1 (tinybvh_min / _max: the ternaries); the children were written by other threads
__device__ __forceinline__ void write_union(NodeDbl* __restrict__ nodes, uint64_t at, uint64_t c) {
    const double* l = nodes[c].mn;       // (mn[3], mx[3] are contiguous)
    const double* r = nodes[c + 1].mn;
    for (int a = 0; a < 3; a++) {
        const double lmn = ld_agent(l + a), rmn = ld_agent(r + a), lmx = ld_agent(l + 3 + a), rmx = ld_agent(r + 3 + a);
        nodes[at].mn[a] = lmn < rmn ? lmn : rmn;
        nodes[at].mx[a] = lmx > rmx ? lmx : rmx;
    }
}

// ---- 1. BLASInstanceEx::Update + InvertTransform (tiny_bvh.h:8432-8472), one thread per instance ----------------------------------
__global__ void k_instance_update_dbl(InstanceDbl* __restrict__ instances, const double* __restrict__ transforms, const BlasDbl* __restrict__ blas,
                                      uint32_t n, uint64_t nBlas, uint64_t* __restrict__ centreBounds) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double cLo[3] = {kDblFar, kDblFar, kDblFar}, cHi[3] = {-kDblFar, -kDblFar, -kDblFar};   // this lane's centre, reduced over the wave below
    if (i < n) {
        InstanceDbl& in = instances[i];
        double T[16], iT[16];
        if (transforms) {
            for (int k = 0; k < 16; k++) { T[k] = transforms[(size_t)i * 16 + k]; in.transform[k] = T[k]; }
        } else {
            for (int k = 0; k < 16; k++) T[k] = in.transform[k];
        }
        iT[0] = T[5] * T[10] * T[15] - T[5] * T[11] * T[14] - T[9] * T[6] * T[15] + T[9] * T[7] * T[14] + T[13] * T[6] * T[11] - T[13] * T[7] * T[10];
        iT[1] = -T[1] * T[10] * T[15] + T[1] * T[11] * T[14] + T[9] * T[2] * T[15] - T[9] * T[3] * T[14] - T[13] * T[2] * T[11] + T[13] * T[3] * T[10];
        iT[2] = T[1] * T[6] * T[15] - T[1] * T[7] * T[14] - T[5] * T[2] * T[15] + T[5] * T[3] * T[14] + T[13] * T[2] * T[7] - T[13] * T[3] * T[6];
        iT[3] = -T[1] * T[6] * T[11] + T[1] * T[7] * T[10] + T[5] * T[2] * T[11] - T[5] * T[3] * T[10] - T[9] * T[2] * T[7] + T[9] * T[3] * T[6];
        iT[4] = -T[4] * T[10] * T[15] + T[4] * T[11] * T[14] + T[8] * T[6] * T[15] - T[8] * T[7] * T[14] - T[12] * T[6] * T[11] + T[12] * T[7] * T[10];
        iT[5] = T[0] * T[10] * T[15] - T[0] * T[11] * T[14] - T[8] * T[2] * T[15] + T[8] * T[3] * T[14] + T[12] * T[2] * T[11] - T[12] * T[3] * T[10];
        iT[6] = -T[0] * T[6] * T[15] + T[0] * T[7] * T[14] + T[4] * T[2] * T[15] - T[4] * T[3] * T[14] - T[12] * T[2] * T[7] + T[12] * T[3] * T[6];
        iT[7] = T[0] * T[6] * T[11] - T[0] * T[7] * T[10] - T[4] * T[2] * T[11] + T[4] * T[3] * T[10] + T[8] * T[2] * T[7] - T[8] * T[3] * T[6];
        iT[8] = T[4] * T[9] * T[15] - T[4] * T[11] * T[13] - T[8] * T[5] * T[15] + T[8] * T[7] * T[13] + T[12] * T[5] * T[11] - T[12] * T[7] * T[9];
        iT[9] = -T[0] * T[9] * T[15] + T[0] * T[11] * T[13] + T[8] * T[1] * T[15] - T[8] * T[3] * T[13] - T[12] * T[1] * T[11] + T[12] * T[3] * T[9];
        iT[10] = T[0] * T[5] * T[15] - T[0] * T[7] * T[13] - T[4] * T[1] * T[15] + T[4] * T[3] * T[13] + T[12] * T[1] * T[7] - T[12] * T[3] * T[5];
        iT[11] = -T[0] * T[5] * T[11] + T[0] * T[7] * T[9] + T[4] * T[1] * T[11] - T[4] * T[3] * T[9] - T[8] * T[1] * T[7] + T[8] * T[3] * T[5];
        iT[12] = -T[4] * T[9] * T[14] + T[4] * T[10] * T[13] + T[8] * T[5] * T[14] - T[8] * T[6] * T[13] - T[12] * T[5] * T[10] + T[12] * T[6] * T[9];
        iT[13] = T[0] * T[9] * T[14] - T[0] * T[10] * T[13] - T[8] * T[1] * T[14] + T[8] * T[2] * T[13] + T[12] * T[1] * T[10] - T[12] * T[2] * T[9];
        iT[14] = -T[0] * T[5] * T[14] + T[0] * T[6] * T[13] + T[4] * T[1] * T[14] - T[4] * T[2] * T[13] - T[12] * T[1] * T[6] + T[12] * T[2] * T[5];
        iT[15] = T[0] * T[5] * T[10] - T[0] * T[6] * T[9] - T[4] * T[1] * T[10] + T[4] * T[2] * T[9] + T[8] * T[1] * T[6] - T[8] * T[2] * T[5];
        const double det = T[0] * iT[0] + T[1] * iT[4] + T[2] * iT[8] + T[3] * iT[12];
        if (det != 0) {   // (the reference returns here and keeps the unscaled cofactors)
            const double invdet = 1. / det;
            for (int k = 0; k < 16; k++) iT[k] *= invdet;
        }
        for (int k = 0; k < 16; k++) in.invTransform[k] = iT[k];
        const uint64_t bi = in.blasIdx;
        const NodeDbl* root = blas[bi < nBlas ? bi : 0].nodes;   // (blasIdx < n_blas: validated by the upload / update)
        const double bb[6] = {root->mn[0], root->mn[1], root->mn[2], root->mx[0], root->mx[1], root->mx[2]};
        const double far32 = (double)1e30f;   // aabbMin = bvhdbl3( BVH_FAR ): the float constant
        double mn[3] = {far32, far32, far32}, mx[3] = {-far32, -far32, -far32};
        for (int j = 0; j < 8; j++) {
            const double p[3] = {j & 1 ? bb[3] : bb[0], j & 2 ? bb[4] : bb[1], j & 4 ? bb[5] : bb[2]};
            // tinybvh_transform_point (tiny_bvh.h:576-584), the w != 1 divide included
            double t[3] = {T[0] * p[0] + T[1] * p[1] + T[2] * p[2] + T[3], T[4] * p[0] + T[5] * p[1] + T[6] * p[2] + T[7], T[8] * p[0] + T[9] * p[1] + T[10] * p[2] + T[11]};
            const double w = T[12] * p[0] + T[13] * p[1] + T[14] * p[2] + T[15];
            if (w != 1) { const double rw = 1. / w; for (int a = 0; a < 3; a++) t[a] = t[a] * rw; }
            for (int a = 0; a < 3; a++) {
                mn[a] = mn[a] < t[a] ? mn[a] : t[a];
                mx[a] = mx[a] > t[a] ? mx[a] : t[a];
            }
        }
        for (int a = 0; a < 3; a++) { in.aabbMin[a] = mn[a]; in.aabbMax[a] = mx[a]; }   // (blasIdx and mask, in the same records, stay)
        for (int a = 0; a < 3; a++) {
            const double c = 0.5 * mn[a] + 0.5 * mx[a];
            if (c > -kDblFar && c < kDblFar) cLo[a] = cHi[a] = c;   // (a NaN or infinite box — w == 0 — takes no part in the bounds; its key is 0)
        }
    }
    lbvh::wave_centre_bounds(cLo, cHi, centreBounds);   // one set of six atomics per wave, an axis without a finite centre left out
}

// ---- the box sources of steps 2-5 -----------------------------------------------------------------------------------------------------------
// A box source supplies the box of primitive i and says what the leaf thread writes beside the leaf node (`side`, indexed by sorted position).
// Instances: the world box step 1 wrote into the record; beside the leaf goes the instance's index, tlasIdx[k].
struct InstanceBoxes {
    using Prim = InstanceDbl;
    using Side = uint64_t;
    struct Box {
        const Prim& in;
        __device__ __forceinline__ double lo(int a) const { return in.aabbMin[a]; }
        __device__ __forceinline__ double hi(int a) const { return in.aabbMax[a]; }
    };
    static __device__ __forceinline__ Box box(const Prim& in) { return Box{in}; }
    static __device__ __forceinline__ void leaf(Side* __restrict__ tlasIdx, uint32_t k, uint32_t i, const Prim&) { tlasIdx[k] = i; }
};
// Spheres {pos, r} (a BVH_Double over custom geometry, custom_sphere_dbl.h; the demos' obj.Build( &sphereAABB, n ) per frame): the boxes pos -/+ r;
// beside the leaf goes the gathered record {pos, r, prim, 0} the traversal reads (the record carries its primIdx entry).
struct SphereBoxes {
    using Prim = SphereDbl;
    using Side = SphereRecDbl;
    struct Box {
        double mn[3], mx[3];
        __device__ __forceinline__ double lo(int a) const { return mn[a]; }
        __device__ __forceinline__ double hi(int a) const { return mx[a]; }
    };
    static __device__ __forceinline__ Box box(const Prim& s) { Box b; sphere_box_dbl(s, b.mn, b.mx); return b; }
    static __device__ __forceinline__ void leaf(Side* __restrict__ recs, uint32_t k, uint32_t i, const Prim& s) {
        recs[k] = SphereRecDbl{{s.pos[0], s.pos[1], s.pos[2]}, s.r, i, 0};
    }
};

// ---- 2. Morton keys ---------------------------------------------------------------------------------------------------------------------
template <class Src>
__global__ void k_morton_dbl(const typename Src::Prim* __restrict__ prims, const uint64_t* __restrict__ centreBounds, uint32_t n,
                             uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const typename Src::Box b = Src::box(prims[i]);
    uint32_t q[3];
    for (int a = 0; a < 3; a++) {
        const double c = 0.5 * b.lo(a) + 0.5 * b.hi(a);
        q[a] = lbvh::morton_axis(c, lbvh::ordered_decode(centreBounds[a]), lbvh::ordered_decode(centreBounds[3 + a]), 2097151u);   // (a NaN centre: cell 0)
    }
    keys[i] = lbvh::morton63(q);
    vals[i] = i;
}

// ---- 4. Karras 2012 topology ---------------------------------------------------------------------------------------------------------
// Karras ids: interior node i -> i, leaf k -> (n - 1) + k.  parent[id] = the Karras interior node above id, slot[id] = where id goes in the
// BVH_Double node array: the root at 0, the children of interior node i at 1 + 2 i and 2 + 2 i.
__global__ void k_lbvh_topology_dbl(const uint64_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ parent, uint32_t* __restrict__ slot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int)n - 1) return;
    const lbvh::KarrasNode k = lbvh::karras_node(keys, (int)n, i);
    parent[k.left] = (uint32_t)i; slot[k.left] = 1u + 2u * (uint32_t)i;
    parent[k.right] = (uint32_t)i; slot[k.right] = 2u + 2u * (uint32_t)i;
    if (i == 0) slot[0] = 0u;
}

// ---- 5. nodes: one thread per leaf writes what stands beside the leaf and the leaf node, then climbs ------------------------------------------
template <class Src>
__global__ void k_lbvh_nodes_dbl(const uint32_t* __restrict__ sortedIdx, const typename Src::Prim* __restrict__ prims, const uint32_t* __restrict__ parent,
                                 const uint32_t* __restrict__ slot, uint32_t* __restrict__ flags, uint32_t n, NodeDbl* __restrict__ nodes,
                                 typename Src::Side* __restrict__ side) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t p = sortedIdx[k];   // (< n: a permutation of the values k_morton_dbl wrote)
    const typename Src::Prim& prim = prims[p];
    Src::leaf(side, k, p, prim);
    const uint32_t id = n - 1 + k;
    NodeDbl* ln = nodes + (n == 1 ? 0u : slot[id]);   // with a single primitive the leaf IS the root
    const typename Src::Box b = Src::box(prim);
    for (int a = 0; a < 3; a++) { ln->mn[a] = b.lo(a); ln->mx[a] = b.hi(a); }
    ln->leftFirst = k; ln->triCount = 1;
    if (n == 1) return;
    __threadfence();
    uint32_t node = parent[id];
    for (;;) {
        if (atomicAdd(flags + node, 1u) == 0u) return;   // first to arrive: the sibling subtree is not finished yet
        __threadfence();
        const uint32_t at = slot[node], c = 1u + 2u * node;
        write_union(nodes, at, c);
        nodes[at].leftFirst = c; nodes[at].triCount = 0;
        if (node == 0) return;
        __threadfence();
        node = parent[node];
    }
}

// Step 1 of a sphere build: there are no records to update, it only reduces the centre bounds.
__global__ void k_sphere_centres_dbl(const SphereDbl* __restrict__ sph, uint32_t n, uint64_t* __restrict__ centreBounds) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    double cLo[3] = {kDblFar, kDblFar, kDblFar}, cHi[3] = {-kDblFar, -kDblFar, -kDblFar};
    if (i < n) {
        double mn[3], mx[3];
        sphere_box_dbl(sph[i], mn, mx);
        for (int a = 0; a < 3; a++) {
            const double c = 0.5 * mn[a] + 0.5 * mx[a];
            if (c > -kDblFar && c < kDblFar) cLo[a] = cHi[a] = c;   // (a NaN or infinite box takes no part in the bounds; its key is 0)
        }
    }
    lbvh::wave_centre_bounds(cLo, cHi, centreBounds);
}

// ---- refit ----------------------------------------------------------------------------------------------------------------------------
// Once per scene, ONE workgroup: walk the tree from the root level by level (two frontier lists in global memory), parent[] of every node
// reached and the list of the leaves reached.  A tree (validated at upload) reaches every node at most once, so at most nNodes entries are
// ever appended; the bounds checks keep a wrong blob from writing beyond them all the same.
constexpr uint32_t kParentsBlock = 1024;
__global__ __launch_bounds__(kParentsBlock) void k_parents_dbl(const NodeDbl* __restrict__ nodes, uint32_t nNodes, uint32_t* __restrict__ parent,
                                                               uint32_t* __restrict__ leaves, uint32_t* frontA, uint32_t* frontB, uint32_t* __restrict__ nLeavesOut) {
    __shared__ uint32_t nCur, nNext, nLeaf;
    if (threadIdx.x == 0) { frontA[0] = 0; parent[0] = kNoParent; nCur = 1; nNext = 0; nLeaf = 0; }
    __syncthreads();
    for (;;) {
        const uint32_t cur = nCur;
        if (cur == 0) break;
        for (uint32_t i = threadIdx.x; i < cur; i += kParentsBlock) {
            const uint32_t node = frontA[i];
            if (nodes[node].triCount != 0) {
                const uint32_t at = atomicAdd(&nLeaf, 1u);
                if (at < nNodes) leaves[at] = node;
            } else {
                const uint64_t c = nodes[node].leftFirst;
                if (c + 1 < nNodes) {
                    const uint32_t at = atomicAdd(&nNext, 2u);
                    if (at + 1 < nNodes) { parent[c] = node; parent[c + 1] = node; frontB[at] = (uint32_t)c; frontB[at + 1] = (uint32_t)c + 1u; }
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) { nCur = nNext < nNodes ? nNext : 0u; nNext = 0; }
        uint32_t* t = frontA; frontA = frontB; frontB = t;
        __syncthreads();
    }
    if (threadIdx.x == 0) *nLeavesOut = nLeaf < nNodes ? nLeaf : nNodes;
}

// One thread per leaf node: its records from the new vertices, its box from the vertices, then the climb.
__global__ void k_refit_dbl(NodeDbl* __restrict__ nodes, uint32_t nNodes, TriDbl* __restrict__ tris, uint64_t nRecs, const double* __restrict__ verts,
                            uint64_t nTris, const uint32_t* __restrict__ leaves, uint32_t nLeaves, const uint32_t* __restrict__ parent,
                            uint32_t* __restrict__ flags) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nLeaves) return;
    const uint32_t leaf = leaves[j];
    const uint64_t first = nodes[leaf].leftFirst, cnt = nodes[leaf].triCount;
    double mn[3] = {kDblFar, kDblFar, kDblFar}, mx[3] = {-kDblFar, -kDblFar, -kDblFar};
    for (uint64_t r = first; r < first + cnt && r < nRecs; r++) {
        const uint64_t p = tris[r].prim;
        if (p >= nTris) continue;   // (< n_tris: validated at upload)
        const double* v = verts + p * 9;
        for (int a = 0; a < 3; a++) {
            const double x = v[a], y = v[3 + a], z = v[6 + a];
            tris[r].v0[a] = x; tris[r].e1[a] = y - x; tris[r].e2[a] = z - x;
            const double lo = x < y ? (x < z ? x : z) : (y < z ? y : z), hi = x > y ? (x > z ? x : z) : (y > z ? y : z);
            mn[a] = mn[a] < lo ? mn[a] : lo;
            mx[a] = mx[a] > hi ? mx[a] : hi;
        }
    }
    for (int a = 0; a < 3; a++) { nodes[leaf].mn[a] = mn[a]; nodes[leaf].mx[a] = mx[a]; }
    uint32_t node = parent[leaf];
    if (node == kNoParent) return;   // the root is a leaf
    __threadfence();
    for (;;) {
        if (node >= nNodes || atomicAdd(flags + node, 1u) == 0u) return;   // first to arrive: the sibling subtree is not finished yet
        __threadfence();
        write_union(nodes, node, nodes[node].leftFirst);
        node = parent[node];
        if (node == kNoParent) return;
        __threadfence();
    }
}

struct Scratch {
    uint64_t *keysA, *keysB;
    uint32_t *valsA, *valsB, *parent, *slot, *flags;
    uint64_t* bounds;
    double* xforms;
    void* sortTemp;
    size_t total;
};
// one allocation, carved up here (every part 256-byte aligned); base may be null to just measure
Scratch carve(void* base, uint32_t n, size_t sortTempBytes, bool xforms = true) {
    tbvh_capi::ScratchCarver c(base);
    const size_t N = n;
    Scratch s;
    s.keysA = c.take<uint64_t>(N); s.keysB = c.take<uint64_t>(N);
    s.valsA = c.take<uint32_t>(N); s.valsB = c.take<uint32_t>(N);
    s.parent = c.take<uint32_t>(2 * N); s.slot = c.take<uint32_t>(2 * N);   // 2n - 1 Karras ids
    s.flags = c.take<uint32_t>(N);
    s.bounds = c.take<uint64_t>(8);
    s.xforms = xforms ? c.take<double>(16 * N) : nullptr;   // staged host transforms (a TLAS's only)
    s.sortTemp = c.take_bytes(sortTempBytes);
    s.total = c.total();
    return s;
}

constexpr uint32_t kBuildBlock = 128;   // every build step is one thread per primitive in blocks of this size

// steps 2-5 over a box source: keys, the radix sort, the topology, then the nodes (flags: one word per Karras interior node, zeroed here)
template <class Src>
hipError_t lbvh_over(const char* who, const typename Src::Prim* prims, typename Src::Side* side, NodeDbl* nodes, uint32_t n, const Scratch& sc, size_t sortTempBytes,
                     hipStream_t s) {
    hipError_t e;
    const uint32_t bs = kBuildBlock, nb = (n + bs - 1) / bs;
    hipLaunchKernelGGL(k_morton_dbl<Src>, dim3(nb), dim3(bs), 0, s, prims, sc.bounds, n, sc.keysA, sc.valsA);
    TBVH_STEP(who, "morton keys");
    size_t tmp = sortTempBytes;
    if ((e = hipcub::DeviceRadixSort::SortPairs(sc.sortTemp, tmp, sc.keysA, sc.keysB, sc.valsA, sc.valsB, (int)n, 0, 64, s)) != hipSuccess) {
        fprintf(stderr, "[tinybvh_amd] %s: radix sort (%zu temp bytes): %s\n", who, sortTempBytes, hipGetErrorString(e));
        return e;
    }
    if (n > 1) hipLaunchKernelGGL(k_lbvh_topology_dbl, dim3(nb), dim3(bs), 0, s, sc.keysB, n, sc.parent, sc.slot);
    TBVH_STEP(who, "topology");
    if ((e = hipMemsetAsync(sc.flags, 0, (size_t)n * 4, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_lbvh_nodes_dbl<Src>, dim3(nb), dim3(bs), 0, s, sc.valsB, prims, sc.parent, sc.slot, sc.flags, n, nodes, side);
    TBVH_STEP(who, "nodes");
    return hipGetLastError();
}

size_t sort_temp_bytes(uint32_t n) {
    size_t tmp = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, 64);
    return tmp;
}

}  // namespace

size_t tlas_dbl_build_scratch_bytes(uint32_t n, size_t* sortTempBytes) { return tlas_dbl_build_scratch_total(n, *sortTempBytes = sort_temp_bytes(n)); }
size_t tlas_dbl_build_scratch_total(uint32_t n, size_t sortTempBytes) { return carve(nullptr, n, sortTempBytes).total; }
size_t spheres_dbl_build_scratch_bytes(uint32_t n, size_t* sortTempBytes) { return carve(nullptr, n, *sortTempBytes = sort_temp_bytes(n), false).total; }

double* tlas_dbl_xform_stage(void* scratch, uint32_t n, size_t sortTempBytes) { return carve(scratch, n, sortTempBytes).xforms; }

hipError_t launch_tlas_dbl_rebuild(NodeDbl* tlasNodes, uint64_t* tlasIdx, InstanceDbl* instances, const BlasDbl* blas, uint64_t nBlas, const double* transformsDev,
                                   uint32_t n, void* scratch, size_t sortTempBytes, hipStream_t s) {
    const Scratch sc = carve(scratch, n, sortTempBytes);
    hipError_t e;
    if ((e = reset_centre_bounds(sc.bounds, 8, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_instance_update_dbl, dim3((n + kBuildBlock - 1) / kBuildBlock), dim3(kBuildBlock), 0, s, instances, transformsDev, blas, n, nBlas, sc.bounds);
    TBVH_STEP("TLAS_Double rebuild", "instance update");
    return lbvh_over<InstanceBoxes>("TLAS_Double rebuild", instances, tlasIdx, tlasNodes, n, sc, sortTempBytes, s);
}

hipError_t launch_spheres_dbl_build(NodeDbl* nodes, void* recs48, const void* spheres32, uint32_t n, void* scratch, size_t sortTempBytes, hipStream_t s) {
    const Scratch sc = carve(scratch, n, sortTempBytes, false);
    const SphereDbl* sph = (const SphereDbl*)spheres32;
    hipError_t e;
    if ((e = reset_centre_bounds(sc.bounds, 8, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sphere_centres_dbl, dim3((n + kBuildBlock - 1) / kBuildBlock), dim3(kBuildBlock), 0, s, sph, n, sc.bounds);
    TBVH_STEP("SphereBVH_Double build", "centre bounds");
    return lbvh_over<SphereBoxes>("SphereBVH_Double build", sph, (SphereRecDbl*)recs48, nodes, n, sc, sortTempBytes, s);
}

void launch_parents_dbl(const NodeDbl* nodes, uint32_t nNodes, uint32_t* parent, uint32_t* leaves, uint32_t* frontA, uint32_t* frontB, uint32_t* nLeavesOut, hipStream_t s) {
    hipLaunchKernelGGL(k_parents_dbl, dim3(1), dim3(kParentsBlock), 0, s, nodes, nNodes, parent, leaves, frontA, frontB, nLeavesOut);
}

hipError_t launch_refit_dbl(NodeDbl* nodes, uint32_t nNodes, TriDbl* tris, uint64_t nRecs, const double* verts, uint64_t nTris, const uint32_t* leaves,
                            uint32_t nLeaves, const uint32_t* parent, uint32_t* flags, hipStream_t s) {
    hipError_t e;
    if ((e = hipMemsetAsync(flags, 0, (size_t)nNodes * 4, s)) != hipSuccess) return e;
    const uint32_t bs = 128;
    hipLaunchKernelGGL(k_refit_dbl, dim3((nLeaves + bs - 1) / bs), dim3(bs), 0, s, nodes, nNodes, tris, nRecs, verts, nTris, leaves, nLeaves, parent, flags);
    return hipGetLastError();
}

}  // namespace tbvh
