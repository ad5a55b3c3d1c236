// kernels_sbvhbuild.hip — the reference's spatial-split tree (SBVH: BVH::BuildHQ, tiny_bvh.h:2623-3040) built on the device, node for node
// (DESIGN.md §19).  All arithmetic is sbvh_split.h's, shared with the host twin.
//
// Level-synchronous over TEMPORARY nodes numbered as kernels_sahbuild.hip numbers them (root 0, 1 unused, a level = the range of ids the splits of the
// level before took from one counter), with one small read-back per level.  A node carries the reference's bookkeeping: its range of primIdx and
// its slice [sliceStart, sliceEnd) of the double-buffered index arrays (the children get [sliceStart, (A + B) >> 1) and [(A + B) >> 1, sliceEnd)).
// ONE BLOCK PER OPEN NODE, because everything a node does after its bins is ordered by the node's own fragments; three kernels per level:
//   k_sbvh_decide
//     object bins    the node's fragments into 3 x 8 bins in LDS: integer atomic min / max on order-preserving keys (sah_split.h: key), integer counts
//     spatial bins   if the object sweep leaves the node eligible: one item per (fragment, axis), the fragment clipped to every bin it overlaps
//                    (sbvh::spatial_bin_fragment), the same key atomics, countIn / countOut by atomicAdd; then the final decision: leaf / object / spatial
//     classification every position of a spatially split node: left, right or straddler
//   k_sbvh_chain     (one wave per node; nothing to do unless the node is split spatially)
//     unsplit chain  the one serial part: the wave walks the straddlers in source order, 64 positions at a time (ballot, then one uniform
//                    sbvh::unsplit_step per straddler with the box handed round by __shfl).  A straddler that stays split records the plane it is
//                    cut at — the chain moves it — and is cut afterwards in parallel (sbvh::split_frag)
//   k_sbvh_partition
//     cuts           the straddlers that stayed split; the second half's fragment index comes from one device-wide atomic counter: fragment
//                    indices never reach the output
//     stable scatter left entries in source order from sliceStart up, right entries from sliceEnd - 1 down (ballots and per-wave sums, no atomic
//                    cursors: the order inside a range decides the straddler order of the next level and the leaves' order in the output)
//     children       object split: the sweep's prefix / suffix boxes; spatial split: refreshed from the fragments of each side (key atomics in LDS)
//   A node that does not split writes fragment[].primIdx over its range in place.
// Then the interior counts and reference counts of the subtrees bottom-up and BVH::Compact's numbering top-down (child pairs in the pre-order of the
// interior nodes; a leaf's first reference = the references of the leaves before it in that walk), the leaves' references copied to their places,
// and for maxLeafTris the leaf chains of sahbuild.h with every new box intersected with its leaf's.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <vector>

#include "dev_buf.h"
#include "sbvhbuild.h"

namespace tbvh {

namespace {

using sbvh::Frag;

constexpr uint32_t kB = 256;
constexpr uint32_t kCtrNext = 0, kCtrFrag = 1, kCtrOverflow = 2, kCtrExtra = 3, kCtrStats = 4 /* .. 12 */, kCtrRoot = 16 /* .. 21 */, kCtrWords = 24;
constexpr uint32_t kAxisWords = 64;   // per axis in LDS: 24 min keys (bin * 3 + k), 24 max keys, 8 countIn, 8 countOut

// what k_sbvh_decide leaves for the node's chain and partition: one record per node of the level
struct NodeDec {
    int kind;
    uint32_t axis, pos;
    int nl, nr;
    float splitCost;
    float lmin[3], lmax[3], rmin[3], rmax[3];
};

struct SbvhScratch {
    Frag* frag;               // n + n / 2 fragments
    uint32_t *idx, *tmp;      // primIdx and idxTmp of the reference, n + n / 2 each
    uint8_t* cls;             // per position of a spatially split node: sbvh::kToLeft / kToRight / kStraddler / kSplit
    float* cut;               // per position: the plane a split straddler is cut at, then (as bits) the index of its right half
    float4* tbox;             // temporary nodes, Wald form: {min, first}, {max, count}
    uint2* slice;             // per temporary node
    uint4* aux;               // x: left child (0: a leaf), y: the pre-order index among interior nodes, z: interior nodes below, w: final id
    uint2* refs;              // x: references below, y: references in the leaves before this subtree
    NodeDec* dec;             // one record per node of a level: a level's nodes hold disjoint, non-empty sets of references, so it has at most n + n / 2
    uint32_t *ctr, *extra, *offset;
    void* scanTemp;
};

SbvhScratch carve(void* base, uint32_t n, size_t scanTempBytes, size_t* total) {
    tbvh_capi::ScratchCarver c(base);
    SbvhScratch s;
    const size_t cap = (size_t)n + n / 2, capNodes = (size_t)n * 3 + 2;
    s.frag = c.take<Frag>(cap);
    s.idx = c.take<uint32_t>(cap); s.tmp = c.take<uint32_t>(cap);
    s.cls = c.take<uint8_t>(cap); s.cut = c.take<float>(cap);
    s.tbox = c.take<float4>(2 * capNodes); s.slice = c.take<uint2>(capNodes); s.aux = c.take<uint4>(capNodes); s.refs = c.take<uint2>(capNodes);
    s.dec = c.take<NodeDec>(cap + 2);
    s.ctr = c.take<uint32_t>(kCtrWords);
    s.extra = c.take<uint32_t>(capNodes); s.offset = c.take<uint32_t>(capNodes);
    s.scanTemp = c.take_bytes(scanTempBytes);
    if (total) *total = c.total();
    return s;
}

__device__ __forceinline__ Frag load_frag(const Frag* __restrict__ frag, uint32_t fi) {
    const float4 a = ((const float4*)frag)[2 * (size_t)fi], b = ((const float4*)frag)[2 * (size_t)fi + 1];
    Frag f;
    f.mn[0] = a.x; f.mn[1] = a.y; f.mn[2] = a.z; f.prim = __float_as_uint(a.w);
    f.mx[0] = b.x; f.mx[1] = b.y; f.mx[2] = b.z; f.clipped = __float_as_uint(b.w);
    return f;
}
__device__ __forceinline__ void store_frag(Frag* __restrict__ frag, uint32_t fi, const Frag& f) {
    ((float4*)frag)[2 * (size_t)fi] = make_float4(f.mn[0], f.mn[1], f.mn[2], __uint_as_float(f.prim));
    ((float4*)frag)[2 * (size_t)fi + 1] = make_float4(f.mx[0], f.mx[1], f.mx[2], __uint_as_float(f.clipped));
}

// the triangle's vertices; an index that is not a vertex (already reported by k_sbvh_fragments) is never dereferenced
template <bool GENERAL>
struct Fetch {
    const MeshSrc& m;
    __device__ __forceinline__ void operator()(uint32_t prim, float v[3][3]) const {
        float4 v0, v1, v2;
        if (!mesh_tri<GENERAL>(m, prim, v0, v1, v2)) v0 = v1 = v2 = make_float4(0.f, 0.f, 0.f, 0.f);
        v[0][0] = v0.x; v[0][1] = v0.y; v[0][2] = v0.z; v[1][0] = v1.x; v[1][1] = v1.y; v[1][2] = v1.z; v[2][0] = v2.x; v[2][1] = v2.y; v[2][2] = v2.z;
    }
};

// ---- fragments and the root -----------------------------------------------------------------------------------------------------------

__global__ void k_sbvh_init(uint32_t* __restrict__ ctr, uint32_t n) {
    if (threadIdx.x >= kCtrWords) return;
    uint32_t v = 0;
    if (threadIdx.x == kCtrNext) v = 2;
    if (threadIdx.x == kCtrFrag) v = n;
    if (threadIdx.x >= kCtrRoot && threadIdx.x < kCtrRoot + 3) v = 0xffffffffu;   // (min keys; the max keys start at 0)
    ctr[threadIdx.x] = v;
}

template <bool GENERAL>
__global__ __launch_bounds__(kB) void k_sbvh_fragments(const MeshSrc verts, uint32_t n, Frag* __restrict__ frag, uint32_t* __restrict__ idx, uint32_t* __restrict__ ctr,
                                                       uint32_t* __restrict__ status) {
    __shared__ uint32_t box[6];
    if (threadIdx.x < 3) box[threadIdx.x] = 0xffffffffu; else if (threadIdx.x < 6) box[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * kB + threadIdx.x;
    if (i < n) {
        float4 v0, v1, v2;
        if (!mesh_tri<GENERAL>(verts, i, v0, v1, v2)) { atomicOr(status, kStatusMeshIndex); v0 = v1 = v2 = make_float4(0.f, 0.f, 0.f, 0.f); }
        const float a[3] = {v0.x, v0.y, v0.z}, b[3] = {v1.x, v1.y, v1.z}, c[3] = {v2.x, v2.y, v2.z};
        Frag f;
        sah::fragment_box(a, b, c, f.mn, f.mx);
        f.prim = i; f.clipped = 0;
        store_frag(frag, i, f);
        idx[i] = i;
        for (int k = 0; k < 3; k++) { atomicMin(&box[k], sah::key(f.mn[k])); atomicMax(&box[3 + k], sah::key(f.mx[k])); }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&ctr[kCtrRoot + threadIdx.x], box[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&ctr[kCtrRoot + threadIdx.x], box[threadIdx.x]);
}

__global__ void k_sbvh_root(const uint32_t* __restrict__ ctr, uint32_t n, float4* __restrict__ tbox, uint2* __restrict__ slice, uint4* __restrict__ aux) {
    float mn[3], mx[3];
    for (int k = 0; k < 3; k++) {
        mn[k] = sah::min_ord(sah::kFar, sah::unkey(ctr[kCtrRoot + k]));
        mx[k] = sah::max_ord(-sah::kFar, sah::unkey(ctr[kCtrRoot + 3 + k]));
    }
    tbox[0] = make_float4(mn[0], mn[1], mn[2], __uint_as_float(0u)); tbox[1] = make_float4(mx[0], mx[1], mx[2], __uint_as_float(n));
    tbox[2] = tbox[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    slice[0] = make_uint2(0u, n + n / 2); slice[1] = make_uint2(0u, 0u);
    aux[0] = make_uint4(0, 0, 0, 0); aux[1] = make_uint4(0, 0, 0, 1);
}

// ---- one level ------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t bin_init(uint32_t w) {
    const uint32_t j = w % kAxisWords;
    return j < 24 ? sah::key(sah::kFar) : j < 48 ? sah::key(-sah::kFar) : 0u;
}

struct LdsSink {
    uint32_t* w;
    __device__ __forceinline__ void in(int a, int b) { atomicAdd(w + a * kAxisWords + 48 + b, 1u); }
    __device__ __forceinline__ void out(int a, int b) { atomicAdd(w + a * kAxisWords + 56 + b, 1u); }
    __device__ __forceinline__ void box(int a, int b, const float mn[3], const float mx[3]) {
        for (int k = 0; k < 3; k++) { atomicMin(w + a * kAxisWords + b * 3 + k, sah::key(mn[k])); atomicMax(w + a * kAxisWords + 24 + b * 3 + k, sah::key(mx[k])); }
    }
};

// object = true: the counts were taken once (countIn), and both sums use them
__device__ void load_axis(const uint32_t* w, bool object, sbvh::AxisBins& b) {
    for (int i = 0; i < sah::kBins; i++) {
        for (int k = 0; k < 3; k++) { b.mn[i][k] = sah::unkey(w[i * 3 + k]); b.mx[i][k] = sah::unkey(w[24 + i * 3 + k]); }
        b.nin[i] = w[48 + i]; b.nout[i] = object ? w[48 + i] : w[56 + i];
    }
}

enum { kLeaf = 0, kObject = 1, kSpatial = 2 };

template <bool GENERAL>
__global__ __launch_bounds__(kB) void k_sbvh_decide(const MeshSrc verts, uint32_t lvlStart, const Frag* __restrict__ frag, uint32_t* __restrict__ idx, uint8_t* __restrict__ cls,
                                                    const float4* __restrict__ tbox, const uint2* __restrict__ slice, uint4* __restrict__ aux, NodeDec* __restrict__ dec,
                                                    uint32_t* __restrict__ ctr) {
    __shared__ uint32_t s_bins[3 * kAxisWords];
    __shared__ sbvh::Best s_best;
    __shared__ int s_kind, s_eligible;

    const uint32_t t = lvlStart + blockIdx.x, tid = threadIdx.x;
    const float4 nmn4 = tbox[2 * (size_t)t], nmx4 = tbox[2 * (size_t)t + 1], rmn4 = tbox[0], rmx4 = tbox[1];
    const uint32_t first = __float_as_uint(nmn4.w), count = __float_as_uint(nmx4.w);
    const uint2 sl = slice[t];
    const float nmn[3] = {nmn4.x, nmn4.y, nmn4.z}, nmx[3] = {nmx4.x, nmx4.y, nmx4.z};
    const float rmn[3] = {rmn4.x, rmn4.y, rmn4.z}, rmx[3] = {rmx4.x, rmx4.y, rmx4.z};
    const float minDim[3] = {(rmx[0] - rmn[0]) * 1e-7f, (rmx[1] - rmn[1]) * 1e-7f, (rmx[2] - rmn[2]) * 1e-7f};
    const bool axisOn[3] = {(nmx[0] - nmn[0]) > minDim[0], (nmx[1] - nmn[1]) > minDim[1], (nmx[2] - nmn[2]) > minDim[2]};
    const float noSplitCost = (float)count * 1.0f, rSAV = 1.0f / sbvh::area3(nmx, nmn);
    const int budget = (int)(sl.y - sl.x);
    const Fetch<GENERAL> fetch{verts};

    // object bins
    for (uint32_t w = tid; w < 3 * kAxisWords; w += kB) s_bins[w] = bin_init(w);
    __syncthreads();
    {
        float rpd[3];
        for (int a = 0; a < 3; a++) rpd[a] = sah::bin_scale(nmn[a], nmx[a]);
        for (uint32_t j = tid; j < count; j += kB) {
            const Frag f = load_frag(frag, idx[first + j]);
            for (int a = 0; a < 3; a++) {
                uint32_t* w = s_bins + a * kAxisWords;
                const int b = sah::bin_index(f.mn[a], f.mx[a], nmn[a], rpd[a]);
                for (int k = 0; k < 3; k++) { atomicMin(w + b * 3 + k, sah::key(f.mn[k])); atomicMax(w + 24 + b * 3 + k, sah::key(f.mx[k])); }
                atomicAdd(w + 48 + b, 1u);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        sbvh::Best best;
        best.splitCost = noSplitCost; best.axis = best.pos = 0; best.nl = best.nr = 0; best.spatial = false;
        for (int k = 0; k < 3; k++) best.lmin[k] = best.lmax[k] = best.rmin[k] = best.rmax[k] = 0.f;
        float unused = 0.f;
        for (int a = 0; a < 3; a++) if (axisOn[a]) {
            sbvh::AxisBins b;
            load_axis(s_bins + a * kAxisWords, true, b);
            sbvh::sweep_axis(b, a, rSAV, false, 0, unused, best);
        }
        s_best = best;
        s_eligible = sbvh::spatial_eligible(best, noSplitCost, budget, count, sbvh::area3(rmx, rmn)) ? 1 : 0;
    }
    __syncthreads();
    if (s_eligible) {
        // spatial bins: one item per (fragment, axis)
        for (uint32_t w = tid; w < 3 * kAxisWords; w += kB) s_bins[w] = bin_init(w);
        __syncthreads();
        LdsSink sink{s_bins};
        for (uint64_t it = tid; it < (uint64_t)count * 3u; it += kB) {
            const uint32_t j = (uint32_t)(it / 3u);
            const int a = (int)(it - (uint64_t)j * 3u);
            if (!axisOn[a]) continue;
            const Frag f = load_frag(frag, idx[first + j]);
            sbvh::spatial_bin_fragment(f, nmn, nmx, minDim, a, fetch, sink);
        }
        __syncthreads();
        if (tid == 0) {
            sbvh::Best best = s_best;
            float minSplitCost = best.splitCost * 0.985f;
            uint32_t refused = 0;
            for (int a = 0; a < 3; a++) if (axisOn[a]) {
                sbvh::AxisBins b;
                load_axis(s_bins + a * kAxisWords, false, b);
                refused += sbvh::sweep_axis(b, a, rSAV, true, budget, minSplitCost, best);
            }
            if (refused) atomicAdd(&ctr[kCtrStats + sbvh::kStBudget], refused);
            s_best = best;
        }
    }
    if (tid == 0) {
        const sbvh::Best& b = s_best;
        NodeDec d;
        d.kind = s_kind = b.splitCost >= noSplitCost ? kLeaf : b.spatial ? kSpatial : kObject;   // (as the reference writes it: a NaN cost splits)
        d.axis = b.axis; d.pos = b.pos; d.nl = b.nl; d.nr = b.nr; d.splitCost = b.splitCost;
        for (int k = 0; k < 3; k++) { d.lmin[k] = b.lmin[k]; d.lmax[k] = b.lmax[k]; d.rmin[k] = b.rmin[k]; d.rmax[k] = b.rmax[k]; }
        dec[blockIdx.x] = d;
    }
    __syncthreads();
    const int kind = s_kind;
    if (kind == kLeaf) {
        // not splitting is better: the fragments' primitives, in place
        for (uint32_t j = tid; j < count; j += kB) idx[first + j] = __float_as_uint(((const float4*)frag)[2 * (size_t)idx[first + j]].w);
        if (tid == 0) aux[t].x = 0;
        return;
    }
    if (kind == kSpatial) {
        const uint32_t axis = s_best.axis, pos = s_best.pos;
        const float nodeMin = nmn[axis], rPlaneDist = 1.0f / sbvh::plane_dist(nodeMin, nmx[axis]);
        for (uint32_t j = tid; j < count; j += kB) cls[first + j] = (uint8_t)sbvh::classify(load_frag(frag, idx[first + j]), axis, pos, nodeMin, rPlaneDist);
    }
}

// the unsplit chain of a spatially split node: one wave, every lane carrying the same state
__global__ __launch_bounds__(64) void k_sbvh_chain(uint32_t lvlStart, const Frag* __restrict__ frag, const uint32_t* __restrict__ idx, uint8_t* __restrict__ cls,
                                                   float* __restrict__ cut, const float4* __restrict__ tbox, const NodeDec* __restrict__ dec, uint32_t* __restrict__ ctr) {
    const NodeDec& d = dec[blockIdx.x];
    if (d.kind != kSpatial) return;
    const uint32_t t = lvlStart + blockIdx.x, lane = threadIdx.x, axis = d.axis;
    const float4 nmn4 = tbox[2 * (size_t)t], nmx4 = tbox[2 * (size_t)t + 1];
    const uint32_t first = __float_as_uint(nmn4.w), count = __float_as_uint(nmx4.w);
    const float nmn[3] = {nmn4.x, nmn4.y, nmn4.z}, nmx[3] = {nmx4.x, nmx4.y, nmx4.z};
    const float rSAV = 1.0f / sbvh::area3(nmx, nmn);
    sbvh::Chain c;
    for (int k = 0; k < 3; k++) { c.lmin[k] = d.lmin[k]; c.lmax[k] = d.lmax[k]; c.rmin[k] = d.rmin[k]; c.rmax[k] = d.rmax[k]; }
    c.nl = d.nl; c.nr = d.nr; c.splitCost = d.splitCost;
    uint32_t nLeft = 0, nRight = 0;
    for (uint32_t j0 = 0; j0 < count; j0 += 64) {
        const uint32_t j = j0 + lane;
        const bool mine = j < count && cls[first + j] == sbvh::kStraddler;
        unsigned long long m = __ballot(mine);
        if (!m) continue;
        float fmn[3] = {0.f, 0.f, 0.f}, fmx[3] = {0.f, 0.f, 0.f};
        if (mine) {
            const Frag f = load_frag(frag, idx[first + j]);
            for (int k = 0; k < 3; k++) { fmn[k] = f.mn[k]; fmx[k] = f.mx[k]; }
        }
        int decision = -1;
        float plane = 0.f;
        while (m) {   // the straddlers of these 64 positions in source order; the box comes from its lane, the step is the same in every lane
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            const float bmn[3] = {__shfl(fmn[0], l), __shfl(fmn[1], l), __shfl(fmn[2], l)}, bmx[3] = {__shfl(fmx[0], l), __shfl(fmx[1], l), __shfl(fmx[2], l)};
            const int go = sbvh::unsplit_step(c, bmn, bmx, rSAV);
            nLeft += go == sbvh::kToLeft ? 1u : 0u; nRight += go == sbvh::kToRight ? 1u : 0u;
            if ((int)lane == l) { decision = go; plane = axis == 0 ? c.lmax[0] : axis == 1 ? c.lmax[1] : c.lmax[2]; }
        }
        if (decision >= 0) { cls[first + j] = (uint8_t)decision; cut[first + j] = plane; }
    }
    if (lane == 0) {
        atomicAdd(&ctr[kCtrStats + sbvh::kStSpatial], 1u);
        if (nLeft) atomicAdd(&ctr[kCtrStats + sbvh::kStUnsplitL], nLeft);
        if (nRight) atomicAdd(&ctr[kCtrStats + sbvh::kStUnsplitR], nRight);
    }
}

// cuts the straddlers that stayed split, scatters the node's entries to the two ends of its slice and writes the children
template <bool GENERAL>
__global__ __launch_bounds__(kB) void k_sbvh_partition(const MeshSrc verts, uint32_t lvlStart, uint32_t capFrag, Frag* frag, uint32_t* idx, uint32_t* tmp, uint8_t* cls, float* cut,
                                                       float4* tbox, uint2* slice, uint4* aux, const NodeDec* __restrict__ dec, uint32_t* __restrict__ ctr) {
    __shared__ uint32_t s_wsum[2][kB / 64];
    __shared__ uint32_t s_box[12];
    const NodeDec& d = dec[blockIdx.x];
    const int kind = d.kind;
    if (kind == kLeaf) return;
    const uint32_t t = lvlStart + blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, axis = d.axis, pos = d.pos;
    const float4 nmn4 = tbox[2 * (size_t)t], nmx4 = tbox[2 * (size_t)t + 1], rmn4 = tbox[0], rmx4 = tbox[1];
    const uint32_t first = __float_as_uint(nmn4.w), count = __float_as_uint(nmx4.w);
    const uint2 sl = slice[t];
    const float minDim[3] = {(rmx4.x - rmn4.x) * 1e-7f, (rmx4.y - rmn4.y) * 1e-7f, (rmx4.z - rmn4.z) * 1e-7f};
    const float nodeMin = axis == 0 ? nmn4.x : axis == 1 ? nmn4.y : nmn4.z, nodeMax = axis == 0 ? nmx4.x : axis == 1 ? nmx4.y : nmx4.z;
    const Fetch<GENERAL> fetch{verts};
    if (kind == kSpatial) {
        // a half without vertices sends the whole fragment to the other side
        for (uint32_t j = tid; j < count; j += kB) {
            if (cls[first + j] != sbvh::kSplit) continue;
            const uint32_t fi = idx[first + j];
            const Frag f = load_frag(frag, fi);
            float v[3][3];
            fetch(f.prim, v);
            Frag p1, p2;
            bool leftOK, rightOK;
            sbvh::split_frag(f, v, minDim, axis, cut[first + j], p1, p2, leftOK, rightOK);
            if (f.clipped) atomicAdd(&ctr[kCtrStats + sbvh::kStReclips], 1u);
            if (leftOK && rightOK) {
                const uint32_t nf = atomicAdd(&ctr[kCtrFrag], 1u);
                if (nf < capFrag) {   // (always: a split adds one reference, and a slice never holds more references than it has room for)
                    store_frag(frag, fi, p1); store_frag(frag, nf, p2);
                    cut[first + j] = __uint_as_float(nf);
                    atomicAdd(&ctr[kCtrStats + sbvh::kStFragSplits], 1u);
                    continue;
                }
                atomicOr(&ctr[kCtrOverflow], 1u);
            } else atomicAdd(&ctr[kCtrStats + sbvh::kStOneSided], 1u);
            cls[first + j] = (uint8_t)(leftOK ? sbvh::kToLeft : sbvh::kToRight);
        }
        __syncthreads();
    }
    // the stable scatter into the other index array
    uint32_t A = 0, Bn = 0;   // entries on the left / on the right so far
    {
        const float rpd = sah::bin_scale(nodeMin, nodeMax);
        for (uint32_t j0 = 0; j0 < count; j0 += kB) {
            const uint32_t j = j0 + tid;
            bool left = false, right = false;
            uint32_t fi = 0, fr = 0;
            if (j < count) {
                fi = fr = idx[first + j];
                if (kind == kSpatial) {
                    const uint32_t c = cls[first + j];
                    left = c == sbvh::kToLeft || c == sbvh::kSplit; right = c == sbvh::kToRight || c == sbvh::kSplit;
                    if (c == sbvh::kSplit) fr = __float_as_uint(cut[first + j]);
                } else {
                    const Frag f = load_frag(frag, fi);
                    const float flo = axis == 0 ? f.mn[0] : axis == 1 ? f.mn[1] : f.mn[2], fhi = axis == 0 ? f.mx[0] : axis == 1 ? f.mx[1] : f.mx[2];
                    left = (uint32_t)sah::bin_index(flo, fhi, nodeMin, rpd) <= pos; right = !left;
                }
            }
            const unsigned long long mL = __ballot(left), mR = __ballot(right), lt = (1ull << lane) - 1ull;
            if (lane == 0) { s_wsum[0][wave] = (uint32_t)__popcll(mL); s_wsum[1][wave] = (uint32_t)__popcll(mR); }
            __syncthreads();
            uint32_t offL = (uint32_t)__popcll(mL & lt), offR = (uint32_t)__popcll(mR & lt), totL = 0, totR = 0;
            for (uint32_t w = 0; w < kB / 64; w++) {
                if (w < wave) { offL += s_wsum[0][w]; offR += s_wsum[1][w]; }
                totL += s_wsum[0][w]; totR += s_wsum[1][w];
            }
            if (left) tmp[sl.x + A + offL] = fi;
            if (right) tmp[sl.y - 1u - (Bn + offR)] = fr;
            A += totL; Bn += totR;
            __syncthreads();
        }
    }
    const uint32_t leftCount = A, rightCount = Bn, Bpos = sl.y - rightCount;
    if (kind == kSpatial && tid < 12) s_box[tid] = tid < 3 || (tid >= 6 && tid < 9) ? 0xffffffffu : 0u;   // {lmin, lmax, rmin, rmax} keys
    __threadfence_block();
    __syncthreads();
    // copy the two ends of the slice back; a spatial split refreshes the children's boxes from the fragments of each side
    for (uint32_t i = tid; i < leftCount + rightCount; i += kB) {
        const bool right = i >= leftCount;
        const uint32_t p = right ? Bpos + (i - leftCount) : sl.x + i, fi = tmp[p];
        idx[p] = fi;
        if (kind == kSpatial) {
            const Frag f = load_frag(frag, fi);
            uint32_t* b = s_box + (right ? 6 : 0);
            for (int k = 0; k < 3; k++) { atomicMin(b + k, sah::key(f.mn[k])); atomicMax(b + 3 + k, sah::key(f.mx[k])); }
        }
    }
    __threadfence_block();
    __syncthreads();
    float lmin[3], lmax[3], rmin[3], rmax[3];
    for (int k = 0; k < 3; k++) {
        if (kind == kSpatial) {
            lmin[k] = sah::min_ord(sah::kFar, sah::unkey(s_box[k])); lmax[k] = sah::max_ord(-sah::kFar, sah::unkey(s_box[3 + k]));
            rmin[k] = sah::min_ord(sah::kFar, sah::unkey(s_box[6 + k])); rmax[k] = sah::max_ord(-sah::kFar, sah::unkey(s_box[9 + k]));
        } else { lmin[k] = d.lmin[k]; lmax[k] = d.lmax[k]; rmin[k] = d.rmin[k]; rmax[k] = d.rmax[k]; }
    }
    if (leftCount == 0 || rightCount == 0) {
        // the path the reference cannot be followed on (sbvhbuild.h): a leaf over the fragments where the partition put them, refreshed bounds
        const uint32_t at = leftCount ? sl.x : Bpos, total = leftCount + rightCount;
        for (uint32_t j = tid; j < total; j += kB) idx[at + j] = __float_as_uint(((const float4*)frag)[2 * (size_t)idx[at + j]].w);
        if (tid == 0) {
            tbox[2 * (size_t)t] = make_float4(sah::min_ord(lmin[0], rmin[0]), sah::min_ord(lmin[1], rmin[1]), sah::min_ord(lmin[2], rmin[2]), __uint_as_float(at));
            tbox[2 * (size_t)t + 1] = make_float4(sah::max_ord(lmax[0], rmax[0]), sah::max_ord(lmax[1], rmax[1]), sah::max_ord(lmax[2], rmax[2]), __uint_as_float(total));
            aux[t].x = 0;
            atomicAdd(&ctr[kCtrStats + sbvh::kStFailed], 1u);
        }
        return;
    }
    if (tid == 0) {
        const uint32_t c = atomicAdd(&ctr[kCtrNext], 2u), mid = (sl.x + leftCount + Bpos) >> 1;
        tbox[2 * (size_t)c] = make_float4(lmin[0], lmin[1], lmin[2], __uint_as_float(sl.x));
        tbox[2 * (size_t)c + 1] = make_float4(lmax[0], lmax[1], lmax[2], __uint_as_float(leftCount));
        tbox[2 * (size_t)c + 2] = make_float4(rmin[0], rmin[1], rmin[2], __uint_as_float(Bpos));
        tbox[2 * (size_t)c + 3] = make_float4(rmax[0], rmax[1], rmax[2], __uint_as_float(rightCount));
        slice[c] = make_uint2(sl.x, mid); slice[c + 1] = make_uint2(mid, sl.y);
        aux[c] = make_uint4(0, 0, 0, 0); aux[c + 1] = make_uint4(0, 0, 0, 0);
        aux[t].x = c;
    }
}

// ---- numbering ------------------------------------------------------------------------------------------------------------------------

__global__ void k_sbvh_count_up(uint32_t lvlStart, uint32_t lvlEnd, const float4* __restrict__ tbox, uint4* __restrict__ aux, uint2* __restrict__ refs) {
    const uint32_t t = lvlStart + blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lvlEnd) return;
    const uint32_t l = aux[t].x;
    aux[t].z = l ? 1u + aux[l].z + aux[l + 1].z : 0u;
    refs[t].x = l ? refs[l].x + refs[l + 1].x : __float_as_uint(tbox[2 * (size_t)t + 1].w);
}

// aux[t].y = the pre-order index among interior nodes, .w = the final id, refs[t].y = the references of the leaves before the subtree: all set by the
// parent's level.  Writes node t and hands its children theirs.
__global__ void k_sbvh_number_down(uint32_t lvlStart, uint32_t lvlEnd, const float4* __restrict__ tbox, uint4* __restrict__ aux, uint2* __restrict__ refs,
                                   float4* __restrict__ nodes32) {
    const uint32_t t = lvlStart + blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lvlEnd) return;
    uint4 a = aux[t];
    uint2 r = refs[t];
    if (t == 0) { a.y = 0; a.w = 0; r.y = 0; refs[0].y = 0; }
    float4 mn = tbox[2 * (size_t)t], mx = tbox[2 * (size_t)t + 1];
    if (a.x) {
        const uint32_t pair = 2u + 2u * a.y;
        aux[a.x].y = a.y + 1u; aux[a.x].w = pair;
        aux[a.x + 1].y = a.y + 1u + aux[a.x].z; aux[a.x + 1].w = pair + 1u;
        refs[a.x].y = r.y; refs[a.x + 1].y = r.y + refs[a.x].x;
        mn.w = __uint_as_float(pair); mx.w = __uint_as_float(0u);
    } else mn.w = __uint_as_float(r.y);
    nodes32[2 * (size_t)a.w] = mn; nodes32[2 * (size_t)a.w + 1] = mx;
    if (t == 0) nodes32[2] = nodes32[3] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// one wave per temporary node: a leaf's references to their place in the output
__global__ __launch_bounds__(64) void k_sbvh_leaf_refs(uint32_t nNodes, const float4* __restrict__ tbox, const uint4* __restrict__ aux, const uint2* __restrict__ refs,
                                                       const uint32_t* __restrict__ idx, uint32_t* __restrict__ primIdx) {
    const uint32_t t = blockIdx.x;
    if (t >= nNodes || t == 1 || aux[t].x) return;
    const uint32_t first = __float_as_uint(tbox[2 * (size_t)t].w), count = __float_as_uint(tbox[2 * (size_t)t + 1].w), at = refs[t].y;
    for (uint32_t i = threadIdx.x; i < count; i += 64) primIdx[at + i] = idx[first + i];
}

// ---- maxLeafTris ----------------------------------------------------------------------------------------------------------------------

__global__ void k_sbvh_split_count(const float4* __restrict__ nodes32, uint32_t nNodes, uint32_t k, uint32_t* __restrict__ extra) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nNodes) extra[i] = sah::split_leaf_pairs(__float_as_uint(nodes32[2 * (size_t)i + 1].w), k);
}

// as k_sah_split_emit (kernels_sahbuild.hip), the leaf's own order kept, with the triangles' boxes taken from the mesh and every new box intersected
// with the leaf's: a leaf that a spatial split has clipped must not grow back
template <bool GENERAL>
__global__ void k_sbvh_split_emit(const MeshSrc verts, float4* __restrict__ nodes32, uint32_t nNodes, uint32_t k, const uint32_t* __restrict__ extra,
                                  const uint32_t* __restrict__ offset, const uint32_t* __restrict__ primIdx, uint32_t* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nNodes) return;
    if (i == nNodes - 1) ctr[kCtrExtra] = offset[i] + extra[i];
    const uint32_t pairs = extra[i];
    if (!pairs) return;
    const float4 lmn = nodes32[2 * (size_t)i], lmx = nodes32[2 * (size_t)i + 1];
    const float leafMn[3] = {lmn.x, lmn.y, lmn.z}, leafMx[3] = {lmx.x, lmx.y, lmx.z};
    const uint32_t base = nNodes + 2u * offset[i], first = __float_as_uint(lmn.w), count = __float_as_uint(lmx.w);
    float smn[3] = {sah::kFar, sah::kFar, sah::kFar}, smx[3] = {-sah::kFar, -sah::kFar, -sah::kFar};
    uint32_t end = count;
    for (uint32_t j = pairs + 1; j-- > 0;) {
        float cmn[3] = {sah::kFar, sah::kFar, sah::kFar}, cmx[3] = {-sah::kFar, -sah::kFar, -sah::kFar};
        for (uint32_t q = j * k; q < end; q++) {
            float4 v0, v1, v2;
            if (!mesh_tri<GENERAL>(verts, primIdx[first + q], v0, v1, v2)) v0 = v1 = v2 = make_float4(0.f, 0.f, 0.f, 0.f);
            const float a[3] = {v0.x, v0.y, v0.z}, b[3] = {v1.x, v1.y, v1.z}, c[3] = {v2.x, v2.y, v2.z};
            float mn[3], mx[3];
            sah::fragment_box(a, b, c, mn, mx);
            for (int d = 0; d < 3; d++) { cmn[d] = sah::min_ord(cmn[d], mn[d]); cmx[d] = sah::max_ord(cmx[d], mx[d]); }
        }
        for (int d = 0; d < 3; d++) { cmn[d] = sah::max_ord(cmn[d], leafMn[d]); cmx[d] = sah::min_ord(cmx[d], leafMx[d]); }
        if (j < pairs) {
            const uint32_t at = base + 2u * j;
            const bool last = j == pairs - 1;
            nodes32[2 * (size_t)at] = make_float4(cmn[0], cmn[1], cmn[2], __uint_as_float(first + j * k));
            nodes32[2 * (size_t)at + 1] = make_float4(cmx[0], cmx[1], cmx[2], __uint_as_float(k));
            nodes32[2 * (size_t)at + 2] = make_float4(smn[0], smn[1], smn[2], __uint_as_float(last ? first + (j + 1) * k : at + 2u));
            nodes32[2 * (size_t)at + 3] = make_float4(smx[0], smx[1], smx[2], __uint_as_float(last ? count - (j + 1) * k : 0u));
        }
        for (int d = 0; d < 3; d++) { smn[d] = sah::min_ord(smn[d], cmn[d]); smx[d] = sah::max_ord(smx[d], cmx[d]); }
        end = j * k;
    }
    nodes32[2 * (size_t)i].w = __uint_as_float(base); nodes32[2 * (size_t)i + 1].w = __uint_as_float(0u);
}

inline uint32_t blocksFor(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

size_t sbvh_scratch_bytes(uint32_t n, size_t* scanTempBytes) {
    size_t scanTemp = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, scanTemp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(3 * (size_t)n + 2));
    *scanTempBytes = scanTemp;
    return sbvh_scratch_total(n, scanTemp);
}
size_t sbvh_scratch_total(uint32_t n, size_t scanTempBytes) {
    size_t total = 0;
    carve(nullptr, n, scanTempBytes, &total);
    return total;
}

hipError_t run_sbvh_build(const MeshSrc& verts, uint32_t n, uint32_t maxLeafTris, float4* nodes32, uint32_t* primIdx, void* scratch, size_t scanTempBytes,
                          uint32_t* status, hipStream_t s, uint32_t* nNodesOut, uint32_t* nIdxOut, sbvh::Stats* stats) {
    SbvhScratch sc = carve(scratch, n, scanTempBytes, nullptr);
    const uint32_t capFrag = n + n / 2, capNodes = 3 * n;
    const bool general = verts.general();
    hipError_t e;
    k_sbvh_init<<<1, 64, 0, s>>>(sc.ctr, n);
    if (general) k_sbvh_fragments<true><<<blocksFor(n, kB), kB, 0, s>>>(verts, n, sc.frag, sc.idx, sc.ctr, status);
    else k_sbvh_fragments<false><<<blocksFor(n, kB), kB, 0, s>>>(verts, n, sc.frag, sc.idx, sc.ctr, status);
    k_sbvh_root<<<1, 1, 0, s>>>(sc.ctr, n, sc.tbox, sc.slice, sc.aux);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    std::vector<uint2> levels;   // [first, end) temporary ids
    NodeDec* dec = sc.dec;
    uint32_t back[kCtrWords] = {};
    uint32_t lvlStart = 0, lvlEnd = 1, next = 2;
    while (lvlEnd > lvlStart) {
        const uint32_t width = lvlEnd - lvlStart;
        if (width > capFrag) return hipErrorUnknown;   // (cannot happen: see SbvhScratch::dec)
        if (general) k_sbvh_decide<true><<<width, kB, 0, s>>>(verts, lvlStart, sc.frag, sc.idx, sc.cls, sc.tbox, sc.slice, sc.aux, dec, sc.ctr);
        else k_sbvh_decide<false><<<width, kB, 0, s>>>(verts, lvlStart, sc.frag, sc.idx, sc.cls, sc.tbox, sc.slice, sc.aux, dec, sc.ctr);
        k_sbvh_chain<<<width, 64, 0, s>>>(lvlStart, sc.frag, sc.idx, sc.cls, sc.cut, sc.tbox, dec, sc.ctr);
        if (general) k_sbvh_partition<true><<<width, kB, 0, s>>>(verts, lvlStart, capFrag, sc.frag, sc.idx, sc.tmp, sc.cls, sc.cut, sc.tbox, sc.slice, sc.aux, dec, sc.ctr);
        else k_sbvh_partition<false><<<width, kB, 0, s>>>(verts, lvlStart, capFrag, sc.frag, sc.idx, sc.tmp, sc.cls, sc.cut, sc.tbox, sc.slice, sc.aux, dec, sc.ctr);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        levels.push_back(make_uint2(lvlStart, lvlEnd));
        // the one read-back of the level: the id counter says which nodes the next level opens
        if ((e = hipMemcpyAsync(back, sc.ctr, sizeof(back), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        const uint32_t after = back[kCtrNext];
        // (cannot happen: at most n + n / 2 references, so fewer than 3 n nodes, and every split fragment has room)
        if (after < next || after > capNodes || back[kCtrOverflow]) return hipErrorUnknown;
        lvlStart = next; lvlEnd = after; next = after;
    }
    const uint32_t nNodes = next;
    for (size_t l = levels.size(); l-- > 0;)
        k_sbvh_count_up<<<blocksFor(levels[l].y - levels[l].x, 256), 256, 0, s>>>(levels[l].x, levels[l].y, sc.tbox, sc.aux, sc.refs);
    for (size_t l = 0; l < levels.size(); l++)
        k_sbvh_number_down<<<blocksFor(levels[l].y - levels[l].x, 256), 256, 0, s>>>(levels[l].x, levels[l].y, sc.tbox, sc.aux, sc.refs, nodes32);
    k_sbvh_leaf_refs<<<nNodes, 64, 0, s>>>(nNodes, sc.tbox, sc.aux, sc.refs, sc.idx, primIdx);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint32_t nRefs = 0;
    if ((e = hipMemcpyAsync(&nRefs, &sc.refs[0].x, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    uint32_t total = nNodes;
    if (maxLeafTris) {
        k_sbvh_split_count<<<blocksFor(nNodes, 256), 256, 0, s>>>(nodes32, nNodes, maxLeafTris, sc.extra);
        size_t tmpBytes = scanTempBytes;
        if ((e = hipcub::DeviceScan::ExclusiveSum(sc.scanTemp, tmpBytes, sc.extra, sc.offset, (int)nNodes, s)) != hipSuccess) return e;
        if (general) k_sbvh_split_emit<true><<<blocksFor(nNodes, 256), 256, 0, s>>>(verts, nodes32, nNodes, maxLeafTris, sc.extra, sc.offset, primIdx, sc.ctr);
        else k_sbvh_split_emit<false><<<blocksFor(nNodes, 256), 256, 0, s>>>(verts, nodes32, nNodes, maxLeafTris, sc.extra, sc.offset, primIdx, sc.ctr);
        uint32_t pairs = 0;
        if ((e = hipMemcpyAsync(&pairs, sc.ctr + kCtrExtra, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        total = nNodes + 2 * pairs;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *nNodesOut = total; *nIdxOut = nRefs;
    if (stats) {
        const uint32_t* c = back + kCtrStats;
        stats->refs = nRefs;
        stats->spatialSplits = c[sbvh::kStSpatial]; stats->unsplitLeft = c[sbvh::kStUnsplitL]; stats->unsplitRight = c[sbvh::kStUnsplitR];
        stats->fragmentSplits = c[sbvh::kStFragSplits]; stats->oneSidedSplits = c[sbvh::kStOneSided]; stats->clippedReclips = c[sbvh::kStReclips];
        stats->budgetRefusals = c[sbvh::kStBudget]; stats->failedPartitions = c[sbvh::kStFailed];
    }
    return hipSuccess;
}

}  // namespace tbvh
