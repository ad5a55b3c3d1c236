// kernels_sahbuild.hip — the reference's binned-SAH tree (BVH::Build, tiny_bvh.h:2332-2461) built on the device, node for node.
//
// Level-synchronous over TEMPORARY nodes, numbered in the order the levels allocate them (root 0, 1 unused, level k + 1 = the ids the splits of
// level k took from one counter, so a level is a range of ids).  Per level, over all open nodes:
//   k_sah_bin        every primitive position of an open node adds its fragment to the node's 3 x 8 bins: integer atomic min / max on
//                    order-preserving keys (sah_split.h: key) and integer counts — no float atomics, no float sums, so the bins do not depend
//                    on the order.  A tile of positions that lies inside ONE node bins privately in LDS and flushes its 168 words once.
//   k_sah_eval       one thread per open node: sah::find_split on the bins; a split takes two ids, writes the children (boxes = the sweep's own)
//   k_sah_partition  every position of a split node moves to the left or right end of the node's range through two cursors (one atomic per
//                    wave and side when the wave sits inside one node); the order inside a range is free until the end
// and the host reads the counters back (one 64-byte copy) to learn the next level.  A child of at most `smallSubtree` primitives is not opened by
// the next level: it is listed, and once a level opens nothing
//   k_sah_small      finishes every listed subtree with one wave each, bins in LDS, over the same sah_split.h (see there)
// Then:
//   k_sah_count_up / k_sah_number_down / k_sah_number_small   interior counts of the subtrees bottom-up, then the reference's numbering top-down: child pairs in the
//                    pre-order of the interior nodes (split a node, continue with the left child, take the right one later from the stack)
//   sort             every leaf range ascending, leaves of any size at once: one radix sort of (leaf's first position << 32 | primitive)
//   k_sah_split_*    BVH::SplitLeafs( k ): an exclusive scan of the extra pairs per leaf places them behind the built nodes
// Only the fragment step knows what a primitive is: k_sah_fragments reads triangles, k_sah_fragments_boxes box pairs or spheres (sahbuild.h: SahBoxes).
// Small inputs: k_sah_one_group runs the same level loop, the count and the numbering in ONE workgroup and one launch, with workgroup barriers where
// the host loop has kernel boundaries (DESIGN.md par. 20).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <vector>

#include "dev_buf.h"
#include "dev_buf.h"
#include "sah_split.h"
#include "sahbuild.h"

namespace tbvh {

namespace {

constexpr uint32_t kBlock = 256, kItems = 4, kTile = kBlock * kItems;
constexpr uint32_t kCtrNext = 0, kCtrRoot = 1 /* .. 6 */, kCtrExtra = 8, kCtrSmall = 9, kCtrOpen = 10, kCtrResult = 11, kCtrWords = 16;
constexpr uint32_t kNone = 0xffffffffu;
// a temporary node that the level path leaves to k_sah_small (a small-subtree root) carries this in cursor[t].y, which only nodes split by the
// level path ever count in
constexpr uint32_t kSmallMark = 0xffffffffu;

struct SahScratch {
    float4 *fmin, *fmax;          // fragment boxes
    uint32_t *idxB, *posA, *posB; // the second primIdx, and the temporary node of every position (two of each: the partition is out of place)
    float4* tbox;                 // temporary nodes, Wald form: {min, first}, {max, count}
    uint4* taux;                  // x: left child (0: a leaf), y: axis | pos << 2 while open, then the pre-order index, z: interior nodes below, w: final id
    uint2* cursor;                // per temporary node: positions handed out at the left / right end
    uint32_t* ctr;
    unsigned long long *keysA, *keysB;
    void *sortTemp, *scanTemp;
    uint32_t* groupBins;          // k_sah_one_group's global bins, n x 672 bytes, for inputs it may build (n <= kSahOneGroupMax), else null
};

SahScratch carve(void* base, uint32_t n, size_t sortTempBytes, size_t scanTempBytes, size_t* total) {
    tbvh_capi::ScratchCarver c(base);
    const size_t N = n;
    SahScratch s;
    s.fmin = c.take<float4>(N); s.fmax = c.take<float4>(N);
    s.idxB = c.take<uint32_t>(N); s.posA = c.take<uint32_t>(N); s.posB = c.take<uint32_t>(N);
    s.tbox = c.take<float4>(4 * N); s.taux = c.take<uint4>(2 * N); s.cursor = c.take<uint2>(2 * N);   // 2 n temporary nodes
    s.ctr = c.take<uint32_t>(kCtrWords);
    s.keysA = c.take<unsigned long long>(N); s.keysB = c.take<unsigned long long>(N);
    s.sortTemp = c.take_bytes(sortTempBytes); s.scanTemp = c.take_bytes(scanTempBytes);
    s.groupBins = n <= kSahOneGroupMax ? c.take<uint32_t>(N * sah::kNodeBinWords) : nullptr;
    if (total) *total = c.total();
    return s;
}

// ---- fragments and the root -----------------------------------------------------------------------------------------------------------

template <bool GENERAL>
__global__ __launch_bounds__(kBlock) void k_sah_fragments(const MeshSrc verts, uint32_t n, float4* __restrict__ fmin, float4* __restrict__ fmax,
                                                          uint32_t* __restrict__ idx, uint32_t* __restrict__ pos, uint32_t* __restrict__ ctr,
                                                          uint32_t* __restrict__ status) {
    __shared__ uint32_t box[6];
    if (threadIdx.x < 3) box[threadIdx.x] = 0xffffffffu; else if (threadIdx.x < 6) box[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        float4 v0, v1, v2;
        if (!mesh_tri<GENERAL>(verts, i, v0, v1, v2)) { atomicOr(status, kStatusMeshIndex); v0 = v1 = v2 = make_float4(0.f, 0.f, 0.f, 0.f); }
        const float a[3] = {v0.x, v0.y, v0.z}, b[3] = {v1.x, v1.y, v1.z}, c[3] = {v2.x, v2.y, v2.z};
        float mn[3], mx[3];
        sah::fragment_box(a, b, c, mn, mx);
        fmin[i] = make_float4(mn[0], mn[1], mn[2], 0.f); fmax[i] = make_float4(mx[0], mx[1], mx[2], 0.f);
        idx[i] = i; pos[i] = 0;
        for (int k = 0; k < 3; k++) { atomicMin(&box[k], sah::key(mn[k])); atomicMax(&box[3 + k], sah::key(mx[k])); }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&ctr[kCtrRoot + threadIdx.x], box[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&ctr[kCtrRoot + threadIdx.x], box[threadIdx.x]);
}

// the same over boxes (sahbuild.h: SahBoxes): fragment i is read, or made from sphere i, and nothing else differs
__global__ __launch_bounds__(kBlock) void k_sah_fragments_boxes(const SahBoxes src, uint32_t n, float4* __restrict__ fmin, float4* __restrict__ fmax,
                                                                uint32_t* __restrict__ idx, uint32_t* __restrict__ pos, uint32_t* __restrict__ ctr) {
    __shared__ uint32_t box[6];
    if (threadIdx.x < 3) box[threadIdx.x] = 0xffffffffu; else if (threadIdx.x < 6) box[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        const float* rec = src.data + (size_t)i * src.stride;
        float mn[3], mx[3];
        if (src.spheres) {
            const float s4[4] = {rec[0], rec[1], rec[2], rec[3]};
            sah::sphere_box(s4, mn, mx);
        } else for (int k = 0; k < 3; k++) { mn[k] = rec[src.offMin + k]; mx[k] = rec[src.offMax + k]; }
        fmin[i] = make_float4(mn[0], mn[1], mn[2], 0.f); fmax[i] = make_float4(mx[0], mx[1], mx[2], 0.f);
        idx[i] = i; pos[i] = 0;
        for (int k = 0; k < 3; k++) { atomicMin(&box[k], sah::key(mn[k])); atomicMax(&box[3 + k], sah::key(mx[k])); }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&ctr[kCtrRoot + threadIdx.x], box[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&ctr[kCtrRoot + threadIdx.x], box[threadIdx.x]);
}

__global__ void k_sah_init(uint32_t* __restrict__ ctr) {
    if (threadIdx.x >= kCtrWords) return;
    uint32_t v = 0;
    if (threadIdx.x == kCtrNext) v = 2;
    if (threadIdx.x >= kCtrRoot && threadIdx.x < kCtrRoot + 3) v = 0xffffffffu;   // (min keys; the max keys start at 0)
    ctr[threadIdx.x] = v;
}

// root: min( BVH_FAR, .. ) / max( -BVH_FAR, .. ) of the fragments, as PrepareBuild leaves it
__global__ void k_sah_root(uint32_t* __restrict__ ctr, uint32_t n, uint32_t smallSubtree, float4* __restrict__ tbox, uint4* __restrict__ taux,
                           uint2* __restrict__ cursor, uint32_t* __restrict__ smallRoots) {
    float mn[3], mx[3];
    for (int k = 0; k < 3; k++) {
        mn[k] = sah::min_ord(sah::kFar, sah::unkey(ctr[kCtrRoot + k]));
        mx[k] = sah::max_ord(-sah::kFar, sah::unkey(ctr[kCtrRoot + 3 + k]));
    }
    tbox[0] = make_float4(mn[0], mn[1], mn[2], __uint_as_float(0u)); tbox[1] = make_float4(mx[0], mx[1], mx[2], __uint_as_float(n));
    tbox[2] = tbox[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    taux[0] = make_uint4(0, 0, 0, 0); taux[1] = make_uint4(0, 0, 0, 1);
    const bool small = n <= smallSubtree;
    cursor[0] = make_uint2(0, small ? kSmallMark : 0u);
    if (small) { smallRoots[0] = 0; ctr[kCtrSmall] = 1; }
}

// ---- one level ------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t bin_init(uint32_t w) {   // word w of a node's bins when empty
    const uint32_t j = w % sah::kBinWords;
    return j < 3 ? sah::key(sah::kFar) : j < 6 ? sah::key(-sah::kFar) : 0u;
}

__global__ void k_sah_bins_clear(uint32_t* __restrict__ bins, uint64_t words) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) bins[i] = bin_init((uint32_t)(i % sah::kNodeBinWords));
}

__global__ __launch_bounds__(kBlock) void k_sah_bin(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ pos, uint32_t n, uint32_t lvlStart,
                                                    const float4* __restrict__ fmin, const float4* __restrict__ fmax, const float4* __restrict__ tbox,
                                                    const uint2* __restrict__ cursor, uint32_t* __restrict__ bins) {
    __shared__ uint32_t lds[sah::kNodeBinWords];
    const uint32_t tile0 = blockIdx.x * kTile, tileLast = min(tile0 + kTile, n) - 1;
    // the positions of a node are one range: a tile whose first and last position name the same open node lies inside it
    const uint32_t tFirst = pos[tile0], tLast = pos[tileLast];
    if (tFirst == tLast && (tFirst < lvlStart || cursor[tFirst].y == kSmallMark)) return;   // (the whole tile in one closed leaf or one small subtree)
    const bool priv = tFirst == tLast;
    if (priv) {
        for (uint32_t w = threadIdx.x; w < sah::kNodeBinWords; w += kBlock) lds[w] = bin_init(w);
        __syncthreads();
    }
    for (uint32_t j = 0; j < kItems; j++) {
        const uint32_t p = tile0 + j * kBlock + threadIdx.x;
        if (p >= n) break;
        const uint32_t t = priv ? tFirst : pos[p];
        if (t < lvlStart || (!priv && cursor[t].y == kSmallMark)) continue;   // (a leaf of an earlier level, or a small subtree: k_sah_small's)
        const uint32_t fi = idx[p];
        const float4 bmn = fmin[fi], bmx = fmax[fi], nmn = tbox[2 * (size_t)t], nmx = tbox[2 * (size_t)t + 1];
        const float fmn3[3] = {bmn.x, bmn.y, bmn.z}, fmx3[3] = {bmx.x, bmx.y, bmx.z}, nmn3[3] = {nmn.x, nmn.y, nmn.z}, nmx3[3] = {nmx.x, nmx.y, nmx.z};
        uint32_t kmn[3], kmx[3];
        for (int k = 0; k < 3; k++) { kmn[k] = sah::key(fmn3[k]); kmx[k] = sah::key(fmx3[k]); }
        uint32_t* dst = priv ? lds : bins + (size_t)(t - lvlStart) * sah::kNodeBinWords;
        for (int a = 0; a < 3; a++) {
            const int b = sah::bin_index(fmn3[a], fmx3[a], nmn3[a], sah::bin_scale(nmn3[a], nmx3[a]));
            uint32_t* w = dst + (a * sah::kBins + b) * sah::kBinWords;
            for (int k = 0; k < 3; k++) { atomicMin(w + k, kmn[k]); atomicMax(w + 3 + k, kmx[k]); }
            atomicAdd(w + 6, 1u);
        }
    }
    if (priv) {
        __syncthreads();
        uint32_t* dst = bins + (size_t)(tFirst - lvlStart) * sah::kNodeBinWords;
        for (uint32_t w = threadIdx.x; w < sah::kNodeBinWords; w += kBlock) {
            const uint32_t v = lds[w], j = w % sah::kBinWords;
            if (v == bin_init(w)) continue;
            if (j < 3) atomicMin(dst + w, v); else if (j < 6) atomicMax(dst + w, v); else atomicAdd(dst + w, v);
        }
    }
}

struct DevBins {
    const uint32_t* w;
    __device__ __forceinline__ float mn(int a, int i, int k) const { return sah::unkey(w[(a * sah::kBins + i) * sah::kBinWords + k]); }
    __device__ __forceinline__ float mx(int a, int i, int k) const { return sah::unkey(w[(a * sah::kBins + i) * sah::kBinWords + 3 + k]); }
    __device__ __forceinline__ uint32_t count(int a, int i) const { return w[(a * sah::kBins + i) * sah::kBinWords + 6]; }
};

// one open node t: sah::find_split on its bins (b); a split takes two ids and writes the children.  cap: the temporary nodes there is room for (2 n; a
// split that would not fit — impossible while every split leaves both sides non-empty — is not made)
__device__ __forceinline__ void eval_node(uint32_t t, const uint32_t* nodeBins, uint32_t cap, float4* tbox, uint4* taux, uint2* cursor, uint32_t* ctr,
                                          uint32_t smallSubtree, uint32_t* smallRoots) {
    const float4 nmn = tbox[2 * (size_t)t], nmx = tbox[2 * (size_t)t + 1], rmn = tbox[0], rmx = tbox[1];
    const float nmn3[3] = {nmn.x, nmn.y, nmn.z}, nmx3[3] = {nmx.x, nmx.y, nmx.z};
    const float minDim[3] = {(rmx.x - rmn.x) * 1e-20f, (rmx.y - rmn.y) * 1e-20f, (rmx.z - rmn.z) * 1e-20f};
    const uint32_t first = __float_as_uint(nmn.w), count = __float_as_uint(nmx.w);
    DevBins b{nodeBins};
    sah::Split s;
    uint4 aux = taux[t];
    aux.x = 0;
    if (sah::find_split(b, nmn3, nmx3, minDim, count, t == 0u, s)) {
        const uint32_t leftCount = sah::left_count(b, s), rightCount = count - leftCount;
        if (leftCount != 0 && rightCount != 0 && leftCount < count) {
            const uint32_t c = atomicAdd(&ctr[kCtrNext], 2u);
            if (c + 1u < cap) {
                tbox[2 * (size_t)c] = make_float4(s.lmin[0], s.lmin[1], s.lmin[2], __uint_as_float(first));
                tbox[2 * (size_t)c + 1] = make_float4(s.lmax[0], s.lmax[1], s.lmax[2], __uint_as_float(leftCount));
                tbox[2 * (size_t)c + 2] = make_float4(s.rmin[0], s.rmin[1], s.rmin[2], __uint_as_float(first + leftCount));
                tbox[2 * (size_t)c + 3] = make_float4(s.rmax[0], s.rmax[1], s.rmax[2], __uint_as_float(rightCount));
                taux[c] = make_uint4(0, 0, 0, 0); taux[c + 1] = make_uint4(0, 0, 0, 0);
                // a child of at most smallSubtree primitives is finished by one wave (k_sah_small) once the levels are done; the others open the next level
                const bool smallL = leftCount <= smallSubtree, smallR = rightCount <= smallSubtree;
                cursor[c] = make_uint2(0, smallL ? kSmallMark : 0u); cursor[c + 1] = make_uint2(0, smallR ? kSmallMark : 0u);
                if (smallL || smallR) {
                    const uint32_t at = atomicAdd(&ctr[kCtrSmall], (smallL ? 1u : 0u) + (smallR ? 1u : 0u));
                    if (smallL) smallRoots[at] = c;
                    if (smallR) smallRoots[at + (smallL ? 1u : 0u)] = c + 1;
                }
                if (!smallL || !smallR) atomicAdd(&ctr[kCtrOpen], (smallL ? 0u : 1u) + (smallR ? 0u : 1u));
                aux.x = c; aux.y = s.axis | (s.pos << 2);
            }
        }
    }
    taux[t] = aux;
}

__global__ void k_sah_eval(uint32_t lvlStart, uint32_t lvlEnd, uint32_t cap, const uint32_t* __restrict__ bins, float4* __restrict__ tbox, uint4* __restrict__ taux,
                           uint2* __restrict__ cursor, uint32_t* __restrict__ ctr, uint32_t smallSubtree, uint32_t* __restrict__ smallRoots) {
    const uint32_t t = lvlStart + blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lvlEnd || cursor[t].y == kSmallMark) return;
    eval_node(t, bins + (size_t)(t - lvlStart) * sah::kNodeBinWords, cap, tbox, taux, cursor, ctr, smallSubtree, smallRoots);
}

// position p of a level (every lane of the wave comes here, p < n or not): a position of a split node moves to the left or right end of the node's range
__device__ __forceinline__ void partition_position(uint32_t p, const uint32_t* idxIn, const uint32_t* posIn, uint32_t* idxOut, uint32_t* posOut, uint32_t n,
                                                   uint32_t lvlStart, const float4* fmin, const float4* fmax, const float4* tbox, const uint4* taux, uint2* cursor) {
    uint32_t t = 0, fi = 0, child = 0, first = 0, count = 0;
    bool moves = false, left = false;
    if (p < n) {
        t = posIn[p]; fi = idxIn[p];
        if (t >= lvlStart && t < 2u * n && fi < n) {   // (a position's node is a temporary id, below 2 n; its primitive is below n)
            const uint4 aux = taux[t];
            if (aux.x) {
                const uint32_t axis = aux.y & 3u, sp = aux.y >> 2;
                const float4 nmn = tbox[2 * (size_t)t], nmx = tbox[2 * (size_t)t + 1], bmn = fmin[fi], bmx = fmax[fi];
                const float lo = axis == 0 ? nmn.x : axis == 1 ? nmn.y : nmn.z, hi = axis == 0 ? nmx.x : axis == 1 ? nmx.y : nmx.z;
                const float flo = axis == 0 ? bmn.x : axis == 1 ? bmn.y : bmn.z, fhi = axis == 0 ? bmx.x : axis == 1 ? bmx.y : bmx.z;
                left = (uint32_t)sah::bin_index(flo, fhi, lo, sah::bin_scale(lo, hi)) <= sp;
                moves = true; child = aux.x + (left ? 0u : 1u);
                first = __float_as_uint(nmn.w); count = __float_as_uint(nmx.w);
            }
        }
    }
    // a wave inside one node takes its places with one atomic per side
    const unsigned long long act = __ballot(moves);
    const int lane = (int)(threadIdx.x & 63u), leader = act ? __ffsll((long long)act) - 1 : 0;
    const uint32_t tL = __shfl(t, leader);
    const bool uniform = __ballot(moves && t != tL) == 0ull;
    uint32_t off = 0;
    if (uniform) {
        const unsigned long long mL = __ballot(moves && left), mR = act & ~mL;
        uint32_t baseL = 0, baseR = 0;
        if (act && lane == leader) {
            if (mL) baseL = atomicAdd(&cursor[tL].x, (uint32_t)__popcll(mL));
            if (mR) baseR = atomicAdd(&cursor[tL].y, (uint32_t)__popcll(mR));
        }
        baseL = __shfl(baseL, leader); baseR = __shfl(baseR, leader);
        const unsigned long long lt = (1ull << lane) - 1ull;
        off = left ? baseL + (uint32_t)__popcll(mL & lt) : baseR + (uint32_t)__popcll(mR & lt);
    } else if (moves) off = left ? atomicAdd(&cursor[t].x, 1u) : atomicAdd(&cursor[t].y, 1u);
    if (p < n) {
        const uint32_t dst = !moves ? p : left ? first + off : first + count - 1u - off;
        if (dst < n) { idxOut[dst] = fi; posOut[dst] = moves ? child : t; }   // (dst lies inside the node's range: the bins counted the same answers)
    }
}

__global__ __launch_bounds__(kBlock) void k_sah_partition(const uint32_t* __restrict__ idxIn, const uint32_t* __restrict__ posIn, uint32_t* __restrict__ idxOut,
                                                          uint32_t* __restrict__ posOut, uint32_t n, uint32_t lvlStart, const float4* __restrict__ fmin,
                                                          const float4* __restrict__ fmax, const float4* __restrict__ tbox, const uint4* __restrict__ taux,
                                                          uint2* __restrict__ cursor) {
    partition_position(blockIdx.x * kBlock + threadIdx.x, idxIn, posIn, idxOut, posOut, n, lvlStart, fmin, fmax, tbox, taux, cursor);
}

// ---- numbering ------------------------------------------------------------------------------------------------------------------------

// cap: the temporary nodes there are (2 n); no id read from memory is used as an index before it is checked against it
__device__ __forceinline__ void count_up_node(uint32_t t, uint32_t cap, uint4* taux) {
    const uint32_t l = taux[t].x;
    taux[t].z = (l && l + 1u < cap) ? 1u + taux[l].z + taux[l + 1].z : 0u;
}

__global__ void k_sah_count_up(uint32_t lvlStart, uint32_t lvlEnd, uint32_t cap, uint4* __restrict__ taux, const uint2* __restrict__ cursor) {
    const uint32_t t = lvlStart + blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lvlEnd || cursor[t].y == kSmallMark) return;   // (a small-subtree root has its count from k_sah_small)
    count_up_node(t, cap, taux);
}

// taux[t].y = the pre-order index among interior nodes, .w = the final id, both set by the parent's level; writes node t and hands its children theirs
__device__ __forceinline__ void number_down_node(uint32_t t, uint32_t cap, const float4* tbox, uint4* taux, float4* nodes32) {
    uint4 aux = taux[t];
    if (t == 0) aux.y = 0, aux.w = 0;   // the root: pre-order index 0, node 0 (its .y still holds the split of its level)
    float4 mn = tbox[2 * (size_t)t], mx = tbox[2 * (size_t)t + 1];
    if (aux.w >= cap) return;   // (cannot happen: the final ids of a tree over n primitives are below 2 n)
    if (aux.x && aux.x + 1u < cap) {
        const uint32_t pair = 2u + 2u * aux.y;
        taux[aux.x].y = aux.y + 1u; taux[aux.x].w = pair;
        taux[aux.x + 1].y = aux.y + 1u + taux[aux.x].z; taux[aux.x + 1].w = pair + 1u;
        mn.w = __uint_as_float(pair); mx.w = __uint_as_float(0u);
    }
    nodes32[2 * (size_t)aux.w] = mn; nodes32[2 * (size_t)aux.w + 1] = mx;
    if (t == 0) nodes32[2] = nodes32[3] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void k_sah_number_down(uint32_t lvlStart, uint32_t lvlEnd, uint32_t cap, const float4* __restrict__ tbox, uint4* __restrict__ taux, const uint2* __restrict__ cursor,
                                  float4* __restrict__ nodes32) {
    const uint32_t t = lvlStart + blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= lvlEnd || cursor[t].y == kSmallMark) return;   // (k_sah_number_small writes a small subtree, its root included)
    number_down_node(t, cap, tbox, taux, nodes32);
}

// ---- small subtrees -------------------------------------------------------------------------------------------------------------------
// One wave finishes the subtree below one small root, node after node in the reference's own order (split, continue left, the right child
// waits): the node's bins are built in LDS by the lanes (the same integer atomics on the same keys as k_sah_bin), every lane then runs
// sah::find_split on them (uniform: no lane waits for another's answer), the range is partitioned through ballots into the second primIdx and
// copied back, and lane 0 takes the two ids and writes the children.  Pending right children are a list threaded through taux[].y, so no depth is
// too deep.  What lane 0 wrote is read by lane 0 and handed round by __shfl; primIdx entries cross lanes behind __threadfence_block().
struct LdsBins {
    const uint32_t* w;
    __device__ __forceinline__ float mn(int a, int i, int k) const { return sah::unkey(w[(a * sah::kBins + i) * sah::kBinWords + k]); }
    __device__ __forceinline__ float mx(int a, int i, int k) const { return sah::unkey(w[(a * sah::kBins + i) * sah::kBinWords + 3 + k]); }
    __device__ __forceinline__ uint32_t count(int a, int i) const { return w[(a * sah::kBins + i) * sah::kBinWords + 6]; }
};

__global__ __launch_bounds__(64) void k_sah_small(const uint32_t* __restrict__ smallRoots, uint32_t* idx, uint32_t* tmp, uint32_t* __restrict__ pos,
                                                  const float4* __restrict__ fmin, const float4* __restrict__ fmax, float4* tbox, uint4* taux,
                                                  uint32_t* __restrict__ ctr) {
    __shared__ uint32_t lds[sah::kNodeBinWords];
    const uint32_t root = smallRoots[blockIdx.x], lane = threadIdx.x;
    const float4 rmn = tbox[0], rmx = tbox[1];
    const float minDim[3] = {(rmx.x - rmn.x) * 1e-20f, (rmx.y - rmn.y) * 1e-20f, (rmx.z - rmn.z) * 1e-20f};
    uint32_t t = root, head = kNone, nSplits = 0;
    float4 nmn = tbox[2 * (size_t)root], nmx = tbox[2 * (size_t)root + 1];   // (written by an earlier kernel)
    for (;;) {
        const uint32_t first = __float_as_uint(nmn.w), count = __float_as_uint(nmx.w);
        const float nmn3[3] = {nmn.x, nmn.y, nmn.z}, nmx3[3] = {nmx.x, nmx.y, nmx.z};
        float rpd[3];
        for (int a = 0; a < 3; a++) rpd[a] = sah::bin_scale(nmn3[a], nmx3[a]);
        __syncthreads();
        for (uint32_t w = lane; w < sah::kNodeBinWords; w += 64) lds[w] = bin_init(w);
        __syncthreads();
        for (uint32_t j = lane; j < count; j += 64) {
            const uint32_t fi = idx[first + j];
            const float4 bmn = fmin[fi], bmx = fmax[fi];
            const float fmn3[3] = {bmn.x, bmn.y, bmn.z}, fmx3[3] = {bmx.x, bmx.y, bmx.z};
            for (int a = 0; a < 3; a++) {
                uint32_t* w = lds + (a * sah::kBins + sah::bin_index(fmn3[a], fmx3[a], nmn3[a], rpd[a])) * sah::kBinWords;
                for (int k = 0; k < 3; k++) { atomicMin(w + k, sah::key(fmn3[k])); atomicMax(w + 3 + k, sah::key(fmx3[k])); }
                atomicAdd(w + 6, 1u);
            }
        }
        __syncthreads();
        LdsBins b{lds};
        sah::Split sp;
        uint32_t leftCount = 0;
        bool split = sah::find_split(b, nmn3, nmx3, minDim, count, t == 0u, sp);
        if (split) { leftCount = sah::left_count(b, sp); split = leftCount != 0 && leftCount != count; }
        if (split) {
            const float lo = nmn3[sp.axis], r = rpd[sp.axis];
            uint32_t baseL = 0, baseR = 0;
            for (uint32_t j0 = 0; j0 < count; j0 += 64) {
                const uint32_t j = j0 + lane;
                const bool valid = j < count;
                uint32_t fi = 0;
                bool left = false;
                if (valid) {
                    fi = idx[first + j];
                    const float4 bmn = fmin[fi], bmx = fmax[fi];
                    const float flo = sp.axis == 0 ? bmn.x : sp.axis == 1 ? bmn.y : bmn.z, fhi = sp.axis == 0 ? bmx.x : sp.axis == 1 ? bmx.y : bmx.z;
                    left = (uint32_t)sah::bin_index(flo, fhi, lo, r) <= sp.pos;
                }
                const unsigned long long mL = __ballot(valid && left), mR = __ballot(valid && !left), lt = (1ull << lane) - 1ull;
                if (valid) tmp[first + (left ? baseL + (uint32_t)__popcll(mL & lt) : count - 1u - (baseR + (uint32_t)__popcll(mR & lt)))] = fi;
                baseL += (uint32_t)__popcll(mL); baseR += (uint32_t)__popcll(mR);
            }
            __threadfence_block();
            for (uint32_t j = lane; j < count; j += 64) idx[first + j] = tmp[first + j];
            __threadfence_block();
            uint32_t c = 0;
            if (lane == 0) {
                c = atomicAdd(&ctr[kCtrNext], 2u);
                tbox[2 * (size_t)c] = make_float4(sp.lmin[0], sp.lmin[1], sp.lmin[2], __uint_as_float(first));
                tbox[2 * (size_t)c + 1] = make_float4(sp.lmax[0], sp.lmax[1], sp.lmax[2], __uint_as_float(leftCount));
                tbox[2 * (size_t)c + 2] = make_float4(sp.rmin[0], sp.rmin[1], sp.rmin[2], __uint_as_float(first + leftCount));
                tbox[2 * (size_t)c + 3] = make_float4(sp.rmax[0], sp.rmax[1], sp.rmax[2], __uint_as_float(count - leftCount));
                taux[c] = make_uint4(0, 0, 0, 0); taux[c + 1] = make_uint4(0, head, 0, 0);   // (the right child waits, in front of the list)
                taux[t].x = c;
            }
            c = __shfl(c, 0);
            head = c + 1; nSplits++;
            t = c;
            nmn = make_float4(sp.lmin[0], sp.lmin[1], sp.lmin[2], __uint_as_float(first));
            nmx = make_float4(sp.lmax[0], sp.lmax[1], sp.lmax[2], __uint_as_float(leftCount));
            continue;
        }
        for (uint32_t j = lane; j < count; j += 64) pos[first + j] = t;   // a leaf
        if (head == kNone) break;
        t = head;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), bb = a;
        uint32_t nextHead = 0;
        if (lane == 0) { a = tbox[2 * (size_t)t]; bb = tbox[2 * (size_t)t + 1]; nextHead = taux[t].y; }
        nmn = make_float4(__shfl(a.x, 0), __shfl(a.y, 0), __shfl(a.z, 0), __shfl(a.w, 0));
        nmx = make_float4(__shfl(bb.x, 0), __shfl(bb.y, 0), __shfl(bb.z, 0), __shfl(bb.w, 0));
        head = __shfl(nextHead, 0);
    }
    if (lane == 0) taux[root].z = nSplits;
}

// one thread per small root, after k_sah_number_down gave the root its pre-order index (.y) and final id (.w): the subtree in pre-order — an
// interior node takes the next index, its children sit at 2 + 2 index, left first — with the pending right children again a list through taux[].y
__global__ void k_sah_number_small(const uint32_t* __restrict__ smallRoots, uint32_t nRoots, const float4* __restrict__ tbox, uint4* taux, float4* __restrict__ nodes32) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nRoots) return;
    uint32_t cur = smallRoots[i], head = kNone;
    uint32_t p = cur ? taux[cur].y : 0u, fid = cur ? taux[cur].w : 0u;
    if (cur == 0) nodes32[2] = nodes32[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (;;) {
        const uint32_t l = taux[cur].x;
        float4 mn = tbox[2 * (size_t)cur], mx = tbox[2 * (size_t)cur + 1];
        if (l) {
            const uint32_t pair = 2u + 2u * p++;
            mn.w = __uint_as_float(pair); mx.w = __uint_as_float(0u);
            nodes32[2 * (size_t)fid] = mn; nodes32[2 * (size_t)fid + 1] = mx;
            taux[l + 1].y = head; taux[l + 1].w = pair + 1u; head = l + 1;
            cur = l; fid = pair;
            continue;
        }
        nodes32[2 * (size_t)fid] = mn; nodes32[2 * (size_t)fid + 1] = mx;
        if (head == kNone) break;
        cur = head; fid = taux[cur].w; head = taux[cur].y;
    }
}

// ---- one workgroup ------------------------------------------------------------------------------------------------------------------------
// The whole build of a small input in one launch: the level loop of run_sah_build — clear the level's bins, bin every position of an open node,
// sah::find_split per open node (eval_node: the same id counter), partition through the cursors (partition_position) — then the counts bottom-up, the
// numbering top-down and the leaf-order keys, by ONE workgroup, with __threadfence_block() + __syncthreads() where the host loop has kernel boundaries:
// all waves of a workgroup run on one CU and share its vector cache, so a workgroup-scope fence makes a wave's global writes visible to the others.
// No pointer that is written here is const or __restrict__ (nothing written in the kernel may be read through the scalar cache), and the id counter,
// which only atomics write, is read with an atomic load.  Bins: built in LDS while the level's nodes fit (ldsNodes x 672 bytes of dynamic LDS) and copied
// to the global array gbins (binCap nodes) for the sweep, built in gbins otherwise.  The level ranges go to `levels` (n entries: a tree over n primitives has at most n levels).  Every loop is
// bounded by n or by a range the kernel checked; a broken invariant (a level that does not fit, an id counter that went backwards or past 2 n, a
// level beyond the n-th) leaves the loop and reports 0 nodes in ctr[kCtrResult], which run_sah_build turns into an error.  Small subtrees are not
// handed to single waves here (smallSubtree = 0): every wave of the group is already on the tree.
constexpr uint32_t kGroup = 1024;

__device__ __forceinline__ void bin_position(uint32_t p, uint32_t n, const uint32_t* idx, const uint32_t* pos, uint32_t lvlStart, uint32_t lvlEnd, const float4* fmin,
                                             const float4* fmax, const float4* tbox, uint32_t* bins) {
    const uint32_t t = pos[p];
    if (t < lvlStart || t >= lvlEnd) return;   // (a leaf of an earlier level; an open node is one of this level's)
    const uint32_t fi = idx[p];
    if (fi >= n) return;                        // (primIdx is a permutation of 0 .. n - 1)
    const float4 bmn = fmin[fi], bmx = fmax[fi], nmn = tbox[2 * (size_t)t], nmx = tbox[2 * (size_t)t + 1];
    const float fmn3[3] = {bmn.x, bmn.y, bmn.z}, fmx3[3] = {bmx.x, bmx.y, bmx.z}, nmn3[3] = {nmn.x, nmn.y, nmn.z}, nmx3[3] = {nmx.x, nmx.y, nmx.z};
    uint32_t kmn[3], kmx[3];
    for (int k = 0; k < 3; k++) { kmn[k] = sah::key(fmn3[k]); kmx[k] = sah::key(fmx3[k]); }
    uint32_t* dst = bins + (size_t)(t - lvlStart) * sah::kNodeBinWords;
    for (int a = 0; a < 3; a++) {
        const int b = sah::bin_index(fmn3[a], fmx3[a], nmn3[a], sah::bin_scale(nmn3[a], nmx3[a]));
        uint32_t* w = dst + (a * sah::kBins + b) * sah::kBinWords;
        for (int k = 0; k < 3; k++) { atomicMin(w + k, kmn[k]); atomicMax(w + 3 + k, kmx[k]); }
        atomicAdd(w + 6, 1u);
    }
}

__global__ __launch_bounds__(kGroup) void k_sah_one_group(uint32_t n, uint32_t ldsNodes, uint32_t binCap, const float4* __restrict__ fmin,
                                                          const float4* __restrict__ fmax, uint32_t* idxA, uint32_t* idxB, uint32_t* posA, uint32_t* posB,
                                                          float4* tbox, uint4* taux, uint2* cursor, uint32_t* ctr, uint2* levels, uint32_t* gbins,
                                                          float4* nodes32, unsigned long long* keys) {
    extern __shared__ uint32_t ldsBins[];
    const uint32_t tid = threadIdx.x;
    uint32_t *idxIn = idxA, *idxOut = idxB, *posIn = posA, *posOut = posB;
    uint32_t lvlStart = 0, lvlEnd = 1, next = 2, nLevels = 0;
    bool fault = false;
    for (uint32_t iter = 0;; iter++) {
        const uint32_t width = lvlEnd - lvlStart;
        const bool inLds = width <= ldsNodes;
        if (iter >= n || width > binCap) { fault = true; break; }   // (uniform: every thread holds the same ranges)
        const uint32_t words = width * (uint32_t)sah::kNodeBinWords;            // (width <= binCap or ldsNodes: far below 2^32 / 168)
        if (inLds) {
            for (uint32_t w = tid; w < words; w += kGroup) ldsBins[w] = bin_init(w);
            __syncthreads();
            for (uint32_t p = tid; p < n; p += kGroup) bin_position(p, n, idxIn, posIn, lvlStart, lvlEnd, fmin, fmax, tbox, ldsBins);
            __syncthreads();
            // the finished bins go to the global array once, coalesced: the sweep reads 28-byte records at dword alignment, which global loads take as they
            // come; nothing in LDS is ever addressed through a generic pointer
            for (uint32_t w = tid; w < words; w += kGroup) gbins[w] = ldsBins[w];
        } else {
            for (uint32_t w = tid; w < words; w += kGroup) gbins[w] = bin_init(w);
            __threadfence_block(); __syncthreads();
            for (uint32_t p = tid; p < n; p += kGroup) bin_position(p, n, idxIn, posIn, lvlStart, lvlEnd, fmin, fmax, tbox, gbins);
        }
        __threadfence_block(); __syncthreads();
        for (uint32_t t = lvlStart + tid; t < lvlEnd; t += kGroup)
            eval_node(t, gbins + (size_t)(t - lvlStart) * sah::kNodeBinWords, 2u * n, tbox, taux, cursor, ctr, 0u, nullptr);
        if (tid == 0) levels[nLevels] = make_uint2(lvlStart, lvlEnd);   // (nLevels = iter < n)
        nLevels++;
        __threadfence_block(); __syncthreads();
        // (no thread takes an id again before all have passed the barrier that ends this level's partition: every thread reads the same value)
        const uint32_t after = __hip_atomic_load(&ctr[kCtrNext], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (after == next) break;   // nothing split: every node of this level is a leaf
        if (after < next || after > 2u * n || ((after - next) & 1u)) { fault = true; break; }
        for (uint32_t p0 = 0; p0 < n; p0 += kGroup)   // (whole waves: partition_position ballots)
            partition_position(p0 + tid, idxIn, posIn, idxOut, posOut, n, lvlStart, fmin, fmax, tbox, taux, cursor);
        __threadfence_block(); __syncthreads();
        uint32_t* x = idxIn; idxIn = idxOut; idxOut = x;
        x = posIn; posIn = posOut; posOut = x;
        lvlStart = next; lvlEnd = after; next = after;
    }
    if (fault) {
        if (tid == 0) ctr[kCtrResult] = 0u;
        return;
    }
    for (uint32_t l = nLevels; l-- > 0;) {
        const uint2 r = levels[l];
        for (uint32_t t = r.x + tid; t < r.y; t += kGroup) count_up_node(t, 2u * n, taux);
        __threadfence_block(); __syncthreads();
    }
    for (uint32_t l = 0; l < nLevels; l++) {
        const uint2 r = levels[l];
        for (uint32_t t = r.x + tid; t < r.y; t += kGroup) number_down_node(t, 2u * n, tbox, taux, nodes32);
        __threadfence_block(); __syncthreads();
    }
    // the leaf-order keys (k_sah_leaf_keys) of the arrays the last partition wrote; the primitives land in the caller's primIdx behind the sort (k_sah_unkey)
    for (uint32_t p = tid; p < n; p += kGroup) {
        const uint32_t t = posIn[p] < 2u * n ? posIn[p] : 0u;
        keys[p] = ((unsigned long long)__float_as_uint(tbox[2 * (size_t)t].w) << 32) | idxIn[p];
    }
    if (tid == 0) ctr[kCtrResult] = next;
}

// ---- leaves ---------------------------------------------------------------------------------------------------------------------------

__global__ void k_sah_leaf_keys(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ pos, uint32_t n, const float4* __restrict__ tbox,
                                unsigned long long* __restrict__ keys) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    keys[p] = ((unsigned long long)__float_as_uint(tbox[2 * (size_t)pos[p]].w) << 32) | idx[p];
}

__global__ void k_sah_unkey(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t* __restrict__ primIdx) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) primIdx[p] = (uint32_t)keys[p];
}

__global__ void k_sah_split_count(const float4* __restrict__ nodes32, uint32_t nNodes, uint32_t k, uint32_t* __restrict__ extra) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nNodes) extra[i] = sah::split_leaf_pairs(__float_as_uint(nodes32[2 * (size_t)i + 1].w), k);
}

// a leaf of c > k primitives becomes a chain of pairs: pair j holds primitives [j k, j k + k) on the left and the rest on the right.  Every new
// node gets the bounds of ITS primitives (the reference copies the leaf's box to both halves; the tight box is what the wide encoders and the
// tree check expect of a leaf).  Written from the last pair to the first, carrying the box of the rest along.  One thread per leaf: O(N) in one lane
// for an unsplittable leaf of N equal triangles, correct and slow for huge duplicate sets.
__global__ void k_sah_split_emit(float4* __restrict__ nodes32, uint32_t nNodes, uint32_t k, const uint32_t* __restrict__ extra, const uint32_t* __restrict__ offset,
                                 const uint32_t* __restrict__ primIdx, const float4* __restrict__ fmin, const float4* __restrict__ fmax, uint32_t* __restrict__ ctr) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nNodes) return;
    if (i == nNodes - 1) ctr[kCtrExtra] = offset[i] + extra[i];
    const uint32_t pairs = extra[i];
    if (!pairs) return;
    const uint32_t base = nNodes + 2u * offset[i], first = __float_as_uint(nodes32[2 * (size_t)i].w), count = __float_as_uint(nodes32[2 * (size_t)i + 1].w);
    float smn[3] = {sah::kFar, sah::kFar, sah::kFar}, smx[3] = {-sah::kFar, -sah::kFar, -sah::kFar};   // the box of everything right of the current chunk
    uint32_t end = count;
    for (uint32_t j = pairs + 1; j-- > 0;) {   // chunk j = [j k, end)
        float cmn[3] = {sah::kFar, sah::kFar, sah::kFar}, cmx[3] = {-sah::kFar, -sah::kFar, -sah::kFar};
        for (uint32_t q = j * k; q < end; q++) {
            const uint32_t fi = primIdx[first + q];
            const float4 a = fmin[fi], b = fmax[fi];
            cmn[0] = sah::min_ord(cmn[0], a.x); cmn[1] = sah::min_ord(cmn[1], a.y); cmn[2] = sah::min_ord(cmn[2], a.z);
            cmx[0] = sah::max_ord(cmx[0], b.x); cmx[1] = sah::max_ord(cmx[1], b.y); cmx[2] = sah::max_ord(cmx[2], b.z);
        }
        if (j < pairs) {   // pair j: chunk j on the left, the rest (a leaf for the last pair, else pair j + 1's parent) on the right
            const uint32_t at = base + 2u * j;
            const bool last = j == pairs - 1;
            nodes32[2 * (size_t)at] = make_float4(cmn[0], cmn[1], cmn[2], __uint_as_float(first + j * k));
            nodes32[2 * (size_t)at + 1] = make_float4(cmx[0], cmx[1], cmx[2], __uint_as_float(k));
            nodes32[2 * (size_t)at + 2] = make_float4(smn[0], smn[1], smn[2], __uint_as_float(last ? first + (j + 1) * k : at + 2u));
            nodes32[2 * (size_t)at + 3] = make_float4(smx[0], smx[1], smx[2], __uint_as_float(last ? count - (j + 1) * k : 0u));
        }
        for (int c = 0; c < 3; c++) { smn[c] = sah::min_ord(smn[c], cmn[c]); smx[c] = sah::max_ord(smx[c], cmx[c]); }
        end = j * k;
    }
    nodes32[2 * (size_t)i].w = __uint_as_float(base); nodes32[2 * (size_t)i + 1].w = __uint_as_float(0u);
}

// ---- BVH_GPU::ConvertFrom on the device ---------------------------------------------------------------------------------------------------------
// Wald nodes (the builder's numbering: node 1 unused, child pairs (c, c + 1) with c even, so an odd id is a right child) to Aila-Laine nodes in
// depth-first pre-order (tiny_bvh.h:4612-4655; host form: host_builder.cpp: encode_bvh_gpu), without a stack and without waiting between threads:
//   k_al_prepare    every interior node writes its children's parent; every leaf flags the primIdx position it starts at.  An exclusive scan of
//                   the flags numbers the leaves in depth-first order (the leaves tile primIdx left to right).
//   k_al_leftmost   every leaf hands its number up the chain of ancestors it is the LEFTMOST leaf of (while the node is a left child): each node is
//                   written by exactly one leaf.  A subtree between leftmost leaves a and b holds b - a leaves and 2 (b - a) - 1 nodes.
//   k_al_emit       every node walks up to the root: index = 1 per step + the size of the left sibling's subtree at every step it takes as a right
//                   child, i.e. index( left ) = index( parent ) + 1, index( right ) = index( parent ) + 1 + size( left ); then writes its node: an
//                   interior one both children's boxes and left / right, a leaf zeros and triCount / firstTri.  The pad node 1 is not emitted.
// Every walk is bounded by the node count and every index read from a node is checked before use.
__global__ void k_al_prepare(const float4* __restrict__ nodes32, uint32_t nNodes, uint32_t n, uint32_t* __restrict__ parent, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nNodes || i == 1u) return;
    if (i == 0u) parent[0] = kNone;
    const uint32_t first = __float_as_uint(nodes32[2 * (size_t)i].w), count = __float_as_uint(nodes32[2 * (size_t)i + 1].w);
    if (count) { if (first < n) flag[first] = 1u; }
    else if (first >= 2u && first + 1u < nNodes) { parent[first] = i; parent[first + 1u] = i; }
}

__global__ void k_al_leftmost(const float4* __restrict__ nodes32, uint32_t nNodes, uint32_t n, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rank,
                              uint32_t* __restrict__ lm) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nNodes || i == 1u) return;
    const uint32_t first = __float_as_uint(nodes32[2 * (size_t)i].w), count = __float_as_uint(nodes32[2 * (size_t)i + 1].w);
    if (!count || first >= n) return;
    const uint32_t r = rank[first];
    uint32_t cur = i;
    lm[cur] = r;
    for (uint32_t step = 0; step < nNodes && cur != 0u && !(cur & 1u); step++) {
        cur = parent[cur];
        if (cur >= nNodes) return;
        lm[cur] = r;
    }
}

__global__ void k_al_emit(const float4* __restrict__ nodes32, uint32_t nNodes, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ lm,
                          float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nNodes || i == 1u) return;
    uint32_t index = 0, cur = i;
    for (uint32_t step = 0; cur != 0u; step++) {
        if (step >= nNodes) return;   // (not a tree)
        index += 1u;
        if (cur & 1u) index += 2u * (lm[cur] - lm[cur - 1u]) - 1u;   // the left sibling's subtree
        cur = parent[cur];
        if (cur >= nNodes) return;
    }
    if (index + 1u >= nNodes) return;   // (nNodes - 1 nodes are emitted: indices 0 .. nNodes - 2)
    const float4 mn = nodes32[2 * (size_t)i], mx = nodes32[2 * (size_t)i + 1];
    const uint32_t first = __float_as_uint(mn.w), count = __float_as_uint(mx.w);
    float4* o = out + 4 * (size_t)index;
    if (count) {
        o[0] = o[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        o[2] = make_float4(0.f, 0.f, 0.f, __uint_as_float(count));
        o[3] = make_float4(0.f, 0.f, 0.f, __uint_as_float(first));
        return;
    }
    if (first < 2u || first + 1u >= nNodes) return;
    const float4 lmn = nodes32[2 * (size_t)first], lmx = nodes32[2 * (size_t)first + 1], rmn = nodes32[2 * (size_t)first + 2], rmx = nodes32[2 * (size_t)first + 3];
    const uint32_t left = index + 1u, right = left + 2u * (lm[first + 1u] - lm[first]) - 1u;
    o[0] = make_float4(lmn.x, lmn.y, lmn.z, __uint_as_float(left));
    o[1] = make_float4(lmx.x, lmx.y, lmx.z, __uint_as_float(right));
    o[2] = make_float4(rmn.x, rmn.y, rmn.z, __uint_as_float(0u));
    o[3] = make_float4(rmx.x, rmx.y, rmx.z, __uint_as_float(0u));
}

inline uint32_t blocksFor(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }

}  // namespace

size_t sah_scratch_bytes(uint32_t n, size_t* sortTempBytes, size_t* scanTempBytes) {
    size_t sortTemp = 0, scanTemp = 0;
    hipcub::DeviceRadixSort::SortKeys(nullptr, sortTemp, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)n, 0, 64);
    hipcub::DeviceScan::ExclusiveSum(nullptr, scanTemp, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(2 * n));
    *sortTempBytes = sortTemp; *scanTempBytes = scanTemp;
    return sah_scratch_total(n, sortTemp, scanTemp);
}
size_t sah_scratch_total(uint32_t n, size_t sortTempBytes, size_t scanTempBytes) {
    size_t total = 0;
    carve(nullptr, n, sortTempBytes, scanTempBytes, &total);
    return total;
}

// the dynamic LDS of k_sah_one_group on the current device: what a workgroup may have (160 KiB on gfx950) less a margin for the kernel's own words, in whole
// nodes; asked of the runtime, and set on the kernel, once per device and process
static hipError_t one_group_lds(uint32_t* ldsNodes) {
    static uint32_t known[64] = {};
    int dev = 0, maxLds = 0;
    hipError_t e;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && known[dev]) { *ldsNodes = known[dev]; return hipSuccess; }
    if ((e = hipDeviceGetAttribute(&maxLds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev)) != hipSuccess) return e;
    const uint32_t bytes = (uint32_t)(maxLds > 160 * 1024 ? 160 * 1024 : maxLds) - 1024u;
    *ldsNodes = bytes / (sah::kNodeBinWords * 4u);
    if ((e = hipFuncSetAttribute((const void*)k_sah_one_group, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(*ldsNodes * sah::kNodeBinWords * 4u))) != hipSuccess) return e;
    if (dev >= 0 && dev < 64) known[dev] = *ldsNodes;
    return hipSuccess;
}

hipError_t run_sah_build(const SahSrc& src, uint32_t n, uint32_t maxLeafTris, uint32_t smallSubtree, uint32_t oneGroup, float4* nodes32, uint32_t* primIdx,
                         void* scratch, size_t sortTempBytes, size_t scanTempBytes, uint32_t* status, hipStream_t s, uint32_t* nNodesOut) {
    SahScratch sc = carve(scratch, n, sortTempBytes, scanTempBytes, nullptr);
    hipError_t e;
    const bool group = oneGroup != 0 && n <= oneGroup && n <= kSahOneGroupMax;
    if (group) smallSubtree = 0;
    k_sah_init<<<1, 64, 0, s>>>(sc.ctr);
    uint32_t *idxIn = primIdx, *idxOut = sc.idxB, *posIn = sc.posA, *posOut = sc.posB;
    uint32_t* smallRoots = (uint32_t*)sc.keysA;   // (at most n of them; the sort keys come later)
    if (src.boxes.data) k_sah_fragments_boxes<<<blocksFor(n, kBlock), kBlock, 0, s>>>(src.boxes, n, sc.fmin, sc.fmax, idxIn, posIn, sc.ctr);
    else if (src.mesh.general()) k_sah_fragments<true><<<blocksFor(n, kBlock), kBlock, 0, s>>>(src.mesh, n, sc.fmin, sc.fmax, idxIn, posIn, sc.ctr, status);
    else k_sah_fragments<false><<<blocksFor(n, kBlock), kBlock, 0, s>>>(src.mesh, n, sc.fmin, sc.fmax, idxIn, posIn, sc.ctr, status);
    k_sah_root<<<1, 1, 0, s>>>(sc.ctr, n, smallSubtree, sc.tbox, sc.taux, sc.cursor, smallRoots);
    if ((e = hipGetLastError()) != hipSuccess) return e;

    // bins of the widest level: 672 bytes per node of the level.  With a small-subtree threshold T only nodes of more than T primitives split in the
    // level path, so a level has at most 2 n / (T + 1) nodes (21 bytes per triangle at T = 64); without one (T = 0) up to 336 bytes per triangle.
    // Grown when a level needs more (one synchronisation per growth; the contents are not carried over).
    tbvh_capi::DevBuf<uint32_t> bins;
    uint32_t nNodes = 0;
    if (group) {
        // one launch; the level ranges live where the sort's second key array will (n x 8 bytes), the keys come out in the first
        uint32_t ldsNodes = 0;
        if ((e = one_group_lds(&ldsNodes)) != hipSuccess) return e;
        const uint32_t binCap = n;   // (the nodes of a level hold at least one primitive each; the bins are part of the scratch: no allocation here)
        k_sah_one_group<<<1, kGroup, (size_t)ldsNodes * sah::kNodeBinWords * 4u, s>>>(n, ldsNodes, binCap, sc.fmin, sc.fmax, idxIn, idxOut, posIn, posOut, sc.tbox, sc.taux,
                                                                                     sc.cursor, sc.ctr, (uint2*)sc.keysB, sc.groupBins, nodes32, sc.keysA);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    } else {
        std::vector<uint2> levels;   // [first, end) temporary ids
        uint32_t lvlStart = 0, lvlEnd = 1, next = 2, nSmall = n <= smallSubtree ? 1u : 0u;
        bool open = nSmall == 0;
        while (open) {
            const uint32_t width = lvlEnd - lvlStart;
            const uint64_t words = (uint64_t)width * sah::kNodeBinWords;
            if (bins.count() < words) {
                if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
                if ((e = bins.alloc((size_t)(words > 2 * bins.count() ? words : 2 * bins.count()))) != hipSuccess) return e;
            }
            if ((e = hipMemsetAsync(sc.ctr + kCtrOpen, 0, 4, s)) != hipSuccess) return e;
            k_sah_bins_clear<<<blocksFor(words, 256), 256, 0, s>>>(bins, words);
            k_sah_bin<<<blocksFor(n, kTile), kBlock, 0, s>>>(idxIn, posIn, n, lvlStart, sc.fmin, sc.fmax, sc.tbox, sc.cursor, bins);
            k_sah_eval<<<blocksFor(width, 64), 64, 0, s>>>(lvlStart, lvlEnd, 2u * n, bins, sc.tbox, sc.taux, sc.cursor, sc.ctr, smallSubtree, smallRoots);
            k_sah_partition<<<blocksFor(n, kBlock), kBlock, 0, s>>>(idxIn, posIn, idxOut, posOut, n, lvlStart, sc.fmin, sc.fmax, sc.tbox, sc.taux, sc.cursor);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            std::swap(idxIn, idxOut); std::swap(posIn, posOut);
            levels.push_back(make_uint2(lvlStart, lvlEnd));
            uint32_t back[kCtrWords] = {};   // the one read-back of the level: the id counter, the small roots so far, the nodes the next level opens
            if ((e = hipMemcpyAsync(back, sc.ctr, sizeof(back), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            const uint32_t after = back[kCtrNext];
            if (after < next || after > 2 * n || back[kCtrSmall] > n) return hipErrorUnknown;   // (cannot happen: a binary tree over n leaves has fewer than 2 n nodes)
            nSmall = back[kCtrSmall]; open = back[kCtrOpen] != 0;
            lvlStart = next; lvlEnd = after; next = after;
        }
        if (nSmall) {
            k_sah_small<<<nSmall, 64, 0, s>>>(smallRoots, idxIn, idxOut, posIn, sc.fmin, sc.fmax, sc.tbox, sc.taux, sc.ctr);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(&next, sc.ctr + kCtrNext, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
            if (next > 2 * n) return hipErrorUnknown;
        }
        nNodes = next;
        for (size_t l = levels.size(); l-- > 0;)
            k_sah_count_up<<<blocksFor(levels[l].y - levels[l].x, 256), 256, 0, s>>>(levels[l].x, levels[l].y, 2u * n, sc.taux, sc.cursor);
        for (size_t l = 0; l < levels.size(); l++)
            k_sah_number_down<<<blocksFor(levels[l].y - levels[l].x, 256), 256, 0, s>>>(levels[l].x, levels[l].y, 2u * n, sc.tbox, sc.taux, sc.cursor, nodes32);
        if (nSmall) k_sah_number_small<<<blocksFor(nSmall, 64), 64, 0, s>>>(smallRoots, nSmall, sc.tbox, sc.taux, nodes32);
        // every leaf range ascending: positions keep their leaf (the high word), primitives order inside it (the low word)
        k_sah_leaf_keys<<<blocksFor(n, 256), 256, 0, s>>>(idxIn, posIn, n, sc.tbox, sc.keysA);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    size_t tmp = sortTempBytes;
    int endBit = 33;
    while (endBit < 64 && ((uint64_t)n >> (endBit - 32))) endBit++;   // (a leaf's first position is below n)
    if ((e = hipcub::DeviceRadixSort::SortKeys(sc.sortTemp, tmp, sc.keysA, sc.keysB, (int)n, 0, endBit, s)) != hipSuccess) return e;
    k_sah_unkey<<<blocksFor(n, 256), 256, 0, s>>>(sc.keysB, n, primIdx);
    if (group) {   // the one read-back of this path: the node count (0: the kernel met a broken invariant and stopped)
        if ((e = hipMemcpyAsync(&nNodes, sc.ctr + kCtrResult, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        if (nNodes < 2 || nNodes > 2 * n) return hipErrorUnknown;
    }
    uint32_t total = nNodes;
    if (maxLeafTris) {
        uint32_t* extra = (uint32_t*)sc.keysA;   // (the sort is done with both: 2 n words each, and there are at most 2 n nodes)
        uint32_t* offset = (uint32_t*)sc.keysB;
        k_sah_split_count<<<blocksFor(nNodes, 256), 256, 0, s>>>(nodes32, nNodes, maxLeafTris, extra);
        size_t tmp2 = scanTempBytes;
        if ((e = hipcub::DeviceScan::ExclusiveSum(sc.scanTemp, tmp2, extra, offset, (int)nNodes, s)) != hipSuccess) return e;
        k_sah_split_emit<<<blocksFor(nNodes, 256), 256, 0, s>>>(nodes32, nNodes, maxLeafTris, extra, offset, primIdx, sc.fmin, sc.fmax, sc.ctr);
        uint32_t pairs = 0;
        if ((e = hipMemcpyAsync(&pairs, sc.ctr + kCtrExtra, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        total = nNodes + 2 * pairs;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;   // (the bins go with this call)
    *nNodesOut = total;
    return hipSuccess;
}

hipError_t run_al_encode(const float4* nodes32, uint32_t nNodes, uint32_t n, void* scratch, size_t sortTempBytes, size_t scanTempBytes, float4* nodes64, hipStream_t s) {
    // the parts of the builder's scratch that are free once run_sah_build has returned: both key arrays (2 n words each), a position array, the second primIdx
    SahScratch sc = carve(scratch, n, sortTempBytes, scanTempBytes, nullptr);
    uint32_t *parent = (uint32_t*)sc.keysA, *lm = (uint32_t*)sc.keysB, *flag = sc.idxB, *rank = sc.posA;
    hipError_t e;
    if (nNodes < 2 || nNodes > 2 * n) return hipErrorInvalidValue;
    if ((e = hipMemsetAsync(flag, 0, (size_t)n * 4, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(lm, 0, (size_t)n * 8, s)) != hipSuccess) return e;
    k_al_prepare<<<blocksFor(nNodes, 256), 256, 0, s>>>(nodes32, nNodes, n, parent, flag);
    size_t tmp = scanTempBytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(sc.scanTemp, tmp, flag, rank, (int)n, s)) != hipSuccess) return e;
    k_al_leftmost<<<blocksFor(nNodes, 256), 256, 0, s>>>(nodes32, nNodes, n, parent, rank, lm);
    k_al_emit<<<blocksFor(nNodes, 256), 256, 0, s>>>(nodes32, nNodes, parent, lm, nodes64);
    return hipGetLastError();
}

}  // namespace tbvh
