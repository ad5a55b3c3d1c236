// cwbvh_packet.h — the node test of the wave-packet traversals (kernels_cwbvh_packet.hip; also the two-level experiment tools/experiments/kernels_tlas8_packet.hip): ONE BVH8_CWBVH node, decoded once
// for the wave, against every lane's own ray.
#pragma once
#include "device_common.h"
#include "cwbvh_node.h"
#include "packet_cull.h"

namespace tbvh {

constexpr int kPacketWG = 64;

__device__ __forceinline__ uint32_t sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// This lane's bit of a wave-uniform lane mask (a ballot's result, or several OR-ed together): the scalar pair IS the predicate, no instruction is spent.
__device__ __forceinline__ bool pk_lane_bit(unsigned long long waveMask) { return __builtin_amdgcn_inverse_ballot_w64(waveMask); }

// The children of the wave's current node against THIS lane's ray; the planes come from LDS (decoded once for the wave, near / far in the order of the
// wave's octant).  Returns the WAVE's ordered hit mask (a child counts when any lane's ray enters its box).  Empty slots (meta byte 0) cost
// no vector instruction — a wave-uniform branch.  They are rare where it matters: counted over ALL nodes of the bench scene's tree the mean is 5.6 children
// of 8, but the nodes rays VISIT are almost full — 7.75 children per visited node for the bench's camera batch (7.67 for its diffuse batch), 97 % (96 %) of the
// visited nodes with more than 4 children, 91 % (88 %) with all 8 (the oracle's visit counts on a 256 x 256 camera; profiles/r07_overlap.txt) —, so compacting
// the non-empty children or testing nodes in 4-child half steps has nothing to save.  The planes of
// slot c + 1 are read from LDS while slot c is tested.  MIXED: some lane's octant differs from the wave's — near and far are sorted per lane through min / max.
// The scalar unit is shared by the CU's four SIMDs and this kernel leans on it as hard as on the vector units (67 scalar + 20 branch against 81 vector
// instructions per ray before this form), so what a slot's bits look like in the hit mask (`placed`: its unary triangle bits at its offset, or bit
// 24 + (slot ^ octant) for an interior child) is worked out by LANES 0..7 in a handful of vector instructions and read back per slot, instead of eight
// times a dozen scalar ones; a lane whose ray is out of the game carries tcull = -1 and needs no mask of its own.
// (Compaction "has nothing to save" is about EMPTY slots.  Children no ray of the wave enters are another matter — four out of five of a camera wave's: the
// interval filter of packet_cull.h rejects most of them for the wave at once, and pk_test_survivors below runs the per-lane test for the rest.)
struct PkMeta { uint32_t placedL, nonEmpty; };
__device__ __forceinline__ PkMeta pk_meta(uint32_t m0, uint32_t m1, uint32_t oct0) {
    const uint32_t lane = threadIdx.x;
    const uint32_t metaL = ((lane & 4u) ? m1 : m0) >> (8u * (lane & 3u)) & 255u;          // lane c (< 8): slot c's meta byte
    const bool innerL = (metaL & 0x18u) == 0x18u;
    PkMeta m;
    m.placedL = (metaL >> 5) << ((innerL ? (metaL ^ oct0) : metaL) & 31u);
    m.nonEmpty = (uint32_t)wave_ballot(metaL != 0u) & 0xFFu;   // (lanes 8..63 repeat lanes 0..7: a mask of the ballot, not of the predicate)
    return m;
}

// every child of `todo` (a wave-uniform mask of slots), all eight slots unrolled
template <bool MIXED>
__device__ __forceinline__ uint32_t pk_test_children_of(const float (*planes)[8], float ax, float ay, float az, float ox, float oy, float oz, float tcull,
                                                        uint32_t placedL, uint32_t todo) {
    uint32_t hitmask = 0;
    float4 pa = *(const float4*)&planes[0][0];
    float2 pb = *(const float2*)&planes[0][4];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const float4 qa = pa; const float2 qb = pb;
        if (c < 7) { pa = *(const float4*)&planes[c + 1][0]; pb = *(const float2*)&planes[c + 1][4]; }
        if (!((todo >> c) & 1u)) continue;
        const uint32_t placed = (uint32_t)__builtin_amdgcn_readlane((int)placedL, c);
        hitmask |= wave_ballot(pk_child_exact<MIXED>(qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, ax, ay, az, ox, oy, oz, tcull)) != 0ull ? placed : 0u;
    }
    return hitmask;
}

template <bool MIXED>
__device__ __forceinline__ uint32_t pk_test_children(const float (*planes)[8], float ax, float ay, float az, float ox, float oy, float oz, float tcull,
                                                     uint32_t m0, uint32_t m1, uint32_t oct0) {
    const PkMeta m = pk_meta(m0, m1, oct0);
    return pk_test_children_of<MIXED>(planes, ax, ay, az, ox, oy, oz, tcull, m.placedL, m.nonEmpty);
}

// The few children the wave's filter left (`todo`: 1.4 of a camera wave's 7.6 on average, often none; not zero here), one after the other: nothing is read from
// LDS and no branch is taken for a slot that is not in the mask.  Wave-octant order only (a mixed chunk does not use the filter).
// PEEL = false: the plain loop (the closest-hit kernel with opacity micromaps has no registers left for a second child's planes).
template <bool PEEL>
__device__ __forceinline__ uint32_t pk_test_survivors(const float (*planes)[8], float ax, float ay, float az, float ox, float oy, float oz, float tcull,
                                                      uint32_t placedL, uint32_t todo) {
    uint32_t hitmask = 0;
    if constexpr (PEEL) {
    // The first two survivors peeled (more than two are rare): both slot numbers up front, both children's planes and `placed` words fetched before the first
    // test — the loop below pays an LDS round trip per survivor —, one merged update of the hit mask.  `todo` is not zero.
    const uint32_t c0 = (uint32_t)__builtin_ctz(todo);
    todo &= todo - 1u;
    const float4 qa0 = *(const float4*)&planes[c0][0];
    const float2 qb0 = *(const float2*)&planes[c0][4];
    const uint32_t placed0 = (uint32_t)__builtin_amdgcn_readlane((int)placedL, (int)c0);
    if (todo == 0u)
        return wave_ballot(pk_child_exact<false>(qa0.x, qa0.y, qa0.z, qa0.w, qb0.x, qb0.y, ax, ay, az, ox, oy, oz, tcull)) != 0ull ? placed0 : 0u;
    const uint32_t c1 = (uint32_t)__builtin_ctz(todo);
    todo &= todo - 1u;
    const float4 qa1 = *(const float4*)&planes[c1][0];
    const float2 qb1 = *(const float2*)&planes[c1][4];
    const uint32_t placed1 = (uint32_t)__builtin_amdgcn_readlane((int)placedL, (int)c1);
    const bool in0 = wave_ballot(pk_child_exact<false>(qa0.x, qa0.y, qa0.z, qa0.w, qb0.x, qb0.y, ax, ay, az, ox, oy, oz, tcull)) != 0ull;
    const bool in1 = wave_ballot(pk_child_exact<false>(qa1.x, qa1.y, qa1.z, qa1.w, qb1.x, qb1.y, ax, ay, az, ox, oy, oz, tcull)) != 0ull;
    hitmask = (in0 ? placed0 : 0u) | (in1 ? placed1 : 0u);
    }
    while (todo != 0u) {
        const uint32_t c = (uint32_t)__builtin_ctz(todo);
        todo &= todo - 1u;
        const float4 qa = *(const float4*)&planes[c][0];
        const float2 qb = *(const float2*)&planes[c][4];
        const uint32_t placed = (uint32_t)__builtin_amdgcn_readlane((int)placedL, (int)c);
        hitmask |= wave_ballot(pk_child_exact<false>(qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, ax, ay, az, ox, oy, oz, tcull)) != 0ull ? placed : 0u;
    }
    return hitmask;
}

// Wave-wide max / min of a float, the same value returned to every lane (wave-uniform).  All 64 lanes must be active.  Four rotations within each row of 16
// lanes (DPP row_ror 1, 2, 4, 8: afterwards every lane holds its row's result), then the four rows through v_readlane.  fmaxf / fminf: a NaN is dropped.
template <bool MAX>
__device__ __forceinline__ float pk_wave_reduce(float v) {
#define TBVH_PK_ROR(n) { const float o_ = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + (n), 0xF, 0xF, false)); \
                         v = MAX ? __builtin_fmaxf(v, o_) : __builtin_fminf(v, o_); }
    TBVH_PK_ROR(1) TBVH_PK_ROR(2) TBVH_PK_ROR(4) TBVH_PK_ROR(8)
#undef TBVH_PK_ROR
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return MAX ? __builtin_fmaxf(__builtin_fmaxf(r0, r1), __builtin_fmaxf(r2, r3)) : __builtin_fminf(__builtin_fminf(r0, r1), __builtin_fminf(r2, r3));
}

}  // namespace tbvh
