// packet_cull.h — the wave packet's child filter (kernels_cwbvh_packet.hip, cwbvh_packet.h): ONE conservative interval slab test per wave and node, for all
// eight children at once, ahead of the exact per-lane test.  No HIP in here: the kernel and the host entry tbvh_debug_packet_cull (capi_context.hip;
// tests/test_packet_cull_host.py) run the same expressions.  DESIGN.md §3.3.
//
// Why: a wave of 64 neighbouring camera rays visits a node and then tests each of its ~7.6 non-empty children per lane (6 FMA + 4 min / max + 1 compare,
// and per child a v_readlane, a ballot, a select and a branch for the wave), and for four children out of five NO ray of the wave enters the box.  The
// rays of such a wave share (almost) an origin and their reciprocal directions span a tiny interval, so the box of the wave's origins [Olo, Ohi] and the
// box of its reciprocal directions [rlo, rhi] — taken once per 64-ray chunk over the lanes that hold a ray — reject most of those children in a single
// pass over the node's 48 planes, one plane per lane.  A child that passes still gets the exact per-lane test, so the wave visits exactly the nodes and
// tests exactly the triangles it did without the filter: the filter only ever removes tests whose answer was "no lane".
//
// The bound.  Per node and axis a, with the node's exponent e and a child's near / far plane bytes qn, qf (near and far by the wave's octant), the exact
// test (pk_child_exact below) computes per lane
//     ax = ldexpf(rD.a, e)        ox = (n0.a - O.a) * rD.a   (two roundings)        tn = fmaf(qn, ax, ox)        tf = fmaf(qf, ax, ox)
// and the filter evaluates THE SAME operations at interval endpoints:
//     A_lo = ldexpf(rlo, e)       A_hi = ldexpf(rhi, e)
//     d_lo = n0.a - Ohi           d_hi = n0.a - Olo
//     OX_lo / OX_hi = min / max of { d_lo*rlo, d_lo*rhi, d_hi*rlo, d_hi*rhi }
//     TN_lb = fmaf(qn, A_lo, OX_lo)          TF_ub = fmaf(qf, A_hi, OX_hi)
//     pass  <=>  max(max3(TN_lb), 0) <= min(min3(TF_ub), TC)          TC = max over the live lanes of tcull
// Every float operation rounds monotonically (x <= y  =>  round(op(x)) <= round(op(y)) for an operation that is monotone in real arithmetic): ldexpf in
// its first argument; n0.a - O in O; a product d * r of d in [d_lo, d_hi], r in [rlo, rhi] lies between the smallest and the largest corner product in
// real arithmetic, hence also after rounding; fmaf(q, a, o) with q >= 0 (a plane byte) in a and in o.  So TN_lb <= tn and TF_ub >= tf hold for every live
// lane AS COMPUTED, not only in real arithmetic, whatever the signs of the directions: no epsilon appears, and a child some lane enters always passes.
//
// Rules around it:
//   * Non-finite values.  fminf / fmaxf drop a NaN operand, so a NaN among the corner products (0 * inf) or behind an ldexpf that overflows at a large
//     exponent or rD = +-1e30 from tinybvh_safercp times a large distance (inf - inf in the FMA) would silently fall out of a bound.  pk_cull_plane reports whether
//     everything it touched was finite (the corner products through their sum: a finite sum of four floats has four finite terms); if ANY of a node's
//     48 planes is not, EVERY child of the node passes (pk_cull_pass's `allFinite`): coarser than "that child passes", one ballot for the wave.
//   * A chunk whose live lanes differ in octant ("mixed": the exact test sorts near / far per lane there) does not use the filter: every child passes.
//     Nor does a chunk with a non-finite origin or reciprocal direction in a live lane: the exact test drops such a lane's NaN planes ("no bound on this
//     axis"), which no box of the wave can express.
//   * Lanes without a ray do not enter the boxes (their defaults O = 0, rD = (1e30, 1e30, 1) would blow them up): the kernel substitutes the first live
//     lane's values before it reduces.
//   * TC only has to be AT LEAST every live lane's tcull; hits only come closer, so a stale TC is conservative.  The kernel refreshes it after a triangle
//     phase in which some lane's hit changed (one ballot, then a wave max).  A lane whose tcull is NaN culls nothing in the exact test (fminf drops it):
//     pk_cull_tc maps it to +inf.
//   * The any-hit kernel does not run the filter (TC would be taken over the lanes still unoccluded): shadow rays start at scattered hit points, the
//     origin box is wide, most children pass and the filter costs more than it saves there (profiles/r08_packet_cull.txt).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PKC_HD __host__ __device__ __forceinline__
#else
#define PKC_HD inline
#endif

namespace tbvh {

PKC_HD float pkc_min3(float a, float b, float c) { return __builtin_fminf(__builtin_fminf(a, b), c); }
PKC_HD float pkc_max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
PKC_HD bool pkc_finite(float x) { return __builtin_fabsf(x) <= 3.402823466e38f; }   // (false for NaN)

// The exact test of ONE child against ONE lane's ray: near / far planes (as floats, in the order of the wave's octant) and the lane's ax..oz, tcull.
// MIXED: this lane's octant may differ from the wave's — near and far are sorted per axis.  What pk_test_children runs per lane and child.
template <bool MIXED>
PKC_HD bool pk_child_exact(float qnx, float qny, float qnz, float qfx, float qfy, float qfz, float ax, float ay, float az, float ox, float oy, float oz,
                           float tcull) {
    // (the six FMAs as three v_pk_fma_f32 — the planes do arrive in register pairs — measured 6 % SLOWER on camera rays, same records: profiles/r06_packet_counters.txt)
    float tnx = __builtin_fmaf(qnx, ax, ox), tny = __builtin_fmaf(qny, ay, oy), tnz = __builtin_fmaf(qnz, az, oz);
    float tfx = __builtin_fmaf(qfx, ax, ox), tfy = __builtin_fmaf(qfy, ay, oy), tfz = __builtin_fmaf(qfz, az, oz);
    if (MIXED) {
        const float a0 = __builtin_fminf(tnx, tfx), a1 = __builtin_fmaxf(tnx, tfx), b0 = __builtin_fminf(tny, tfy), b1 = __builtin_fmaxf(tny, tfy);
        const float c0 = __builtin_fminf(tnz, tfz), c1 = __builtin_fmaxf(tnz, tfz);
        tnx = a0; tfx = a1; tny = b0; tfy = b1; tnz = c0; tfz = c1;
    }
    const float cmin = __builtin_fmaxf(pkc_max3(tnx, tny, tnz), 0.0f);
    const float cmax = __builtin_fminf(pkc_min3(tfx, tfy, tfz), tcull);
    return cmin <= cmax;
}

// One plane's bound: TF_ub of a far plane (isFar), TN_lb of a near one.  q: the plane byte as a float; n0a, e: the node's origin and exponent on the plane's
// axis; Olo..rhi: the wave's boxes on that axis.  finite: false when an intermediate or the bound is not finite (see above).
PKC_HD float pk_cull_plane(bool isFar, float q, float n0a, int e, float Olo, float Ohi, float rlo, float rhi, bool& finite) {
    const float A = ldexpf(isFar ? rhi : rlo, e);
    const float dlo = n0a - Ohi, dhi = n0a - Olo;
    const float p0 = dlo * rlo, p1 = dlo * rhi, p2 = dhi * rlo, p3 = dhi * rhi;
    const float oxLo = __builtin_fminf(pkc_min3(p0, p1, p2), p3), oxHi = __builtin_fmaxf(pkc_max3(p0, p1, p2), p3);
    const float bound = __builtin_fmaf(q, A, isFar ? oxHi : oxLo);
    finite = pkc_finite((p0 + p1) + (p2 + p3)) && pkc_finite(bound);
    return bound;
}

// The six bounds of one child combined: may a live lane's ray enter it?
PKC_HD bool pk_cull_pass(float tnx, float tny, float tnz, float tfx, float tfy, float tfz, float TC, bool allFinite) {
    const float lb = __builtin_fmaxf(pkc_max3(tnx, tny, tnz), 0.0f);
    const float ub = __builtin_fminf(pkc_min3(tfx, tfy, tfz), TC);
    return !allFinite || lb <= ub;
}

// A lane's contribution to TC, the wave maximum of tcull
PKC_HD float pk_cull_tc(float tcull) { return tcull == tcull ? tcull : __builtin_inff(); }

}  // namespace tbvh
