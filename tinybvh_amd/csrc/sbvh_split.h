// sbvh_split.h — everything that decides a tree of the reference's spatial-split builder, BVH::BuildHQTask (tiny_bvh.h:2732-3003, with PrepareHQBuild,
// 2647-2711, ClipFrag, 8614-8728, and SplitFrag, 8731-8793), for its defaults hqbvhbins = 8, hqbvhoddeven = false, l_quads = false,
// c_trav = c_int = 1 and SBVH_UNSPLITTING, written once for the device builder (kernels_sbvhbuild.hip) and its host twin (sbvhbuild_host.cpp).
// DESIGN.md §19.
//
// The arithmetic contract is sah_split.h's: every operation as the reference writes it, each rounded once (-ffp-contract=off), EXCEPT where the
// reference build (gcc -O3 -mavx2 -mfma) fuses, read from its disassembly and written out here:
//   - tinybvh_half_area / BVHBase::SA           fmaf( z, x, fmaf( x, y, y * z ) )                         (sah::half_area)
//   - SplitCostSAH                              fmaf( c_int * rA, fmaf( AL, NL, AR * NR ), c_trav )       (split_cost)
//   - v0 + f * (v1 - v0), all nine sites        fmaf( f, v1 - v0, v0 ) per component                      (lerp)
//   - nodeMin + planeDist * j                   fmaf( planeDist, (float)j, nodeMin )                      (spatial_bin_fragment)
//   - ((bmin + bmax) * 0.5f - nmin) is a vfmsub in the reference; the product with 0.5 is exact, so the unfused form of sah::bin_index is the same
//     number (but for a sum that is subnormal, which no scene box produces).
// Reductions over fragments (boxes into bins, the refreshed child boxes of a spatial split) are mins and maxes in the total order of sah::key,
// with the signed-zero caveat of sah_split.h.  Everything the reference computes in a fixed order (the sweeps, the clipping, the unsplit chain)
// keeps tinybvh_min / tinybvh_max and that order.
#pragma once
#include "sah_split.h"

namespace tbvh {
namespace sbvh {

using sah::kBins;
using sah::kFar;
using sah::max_ref;
using sah::min_ref;

constexpr int kMaxPoly = 16;   // vin / vout / vleft / vright of ClipFrag and SplitFrag ("occasionally exceeds 9, but never 12"); a write beyond it is dropped here

// BVHBase::Fragment, field for field (32 bytes)
struct Frag {
    float mn[3]; uint32_t prim;
    float mx[3]; uint32_t clipped;
};

struct Stats {
    unsigned long long refs, spatialSplits, unsplitLeft, unsplitRight, fragmentSplits, oneSidedSplits, clippedReclips, budgetRefusals, failedPartitions;
};
enum { kStRefs, kStSpatial, kStUnsplitL, kStUnsplitR, kStFragSplits, kStOneSided, kStReclips, kStBudget, kStFailed, kStWords };

SAH_HD float clampf(float x, float a, float b) { return x > a ? (x < b ? x : b) : a; }
SAH_HD float lerp(float v0, float v1, float f) { return sah::fma1(f, v1 - v0, v0); }
SAH_HD float area3(const float mx[3], const float mn[3]) { return sah::half_area(mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]); }
// SplitCostSAH (2713-2718)
SAH_HD float split_cost(float rA, float AL, int NL, float AR, int NR) { return sah::fma1(1.0f * rA, sah::fma1(AL, (float)NL, AR * (float)NR), 1.0f); }

// (int32_t)v as x86's cvttss2si gives it: INT_MIN for a NaN and anything outside the int range
SAH_HD int cvt_i32(float v) { return (v > -2147483648.f && v < 2147483648.f) ? (int)v : (int)0x80000000u; }
// tinybvh_clamp( (int32_t)((x - nodeMin) * rPlaneDist), 0, 7 ) (2827-2828)
SAH_HD int spatial_bin(float x, float nodeMin, float rPlaneDist) {
    const int b = cvt_i32((x - nodeMin) * rPlaneDist);
    return b > 0 ? (b < kBins - 1 ? b : kBins - 1) : 0;
}
// (uint32_t)tinybvh_max( (x - nodeMin) * rPlaneDist, 0.0f ) (2891-2892): unclamped above; x86 converts through 64 bits and keeps the low word
SAH_HD uint32_t partition_bin(float x, float nodeMin, float rPlaneDist) {
    const float v = max_ref((x - nodeMin) * rPlaneDist, 0.0f);
    return v < 9223372036854775808.f ? (uint32_t)(unsigned long long)v : 0u;
}
SAH_HD float plane_dist(float nmin, float nmax) { return (nmax - nmin) / (8.0f * 0.9999f); }

// ---- the two sweeps -------------------------------------------------------------------------------------------------------------------------

struct Best {
    float splitCost;
    uint32_t axis, pos;
    int nl, nr;
    bool spatial;
    float lmin[3], lmax[3], rmin[3], rmax[3];
};

// the 8 bins of one axis: boxes, and the counts the left-to-right (nin) and right-to-left (nout) sums take.  An object split counts a fragment once
// (nin = nout = count); a spatial split counts it where it enters and where it leaves (countIn, countOut).
struct AxisBins {
    float mn[kBins][3], mx[kBins][3];
    uint32_t nin[kBins], nout[kBins];
};

// One axis of the object sweep (2781-2803) or of the spatial sweep (2847-2871).  Object: strict C >= splitCost rejection, so the first axis, then
// the first bin, wins ties.  Spatial: C < minSplitCost, NL + NR < budget, NL * NR > 0 (the reference's 32-bit product, wrapped as its imul wraps).
// Returns the candidates of a spatial sweep that were refused by the budget alone (statistics).
SAH_HD uint32_t sweep_axis(const AxisBins& b, int a, float rSAV, bool spatial, int budget, float& minSplitCost, Best& best) {
    float rBMin[kBins - 1][3], rBMax[kBins - 1][3], AR[kBins - 1];
    int NR[kBins - 1];
    {
        float r1[3] = {kFar, kFar, kFar}, r2[3] = {-kFar, -kFar, -kFar};
        uint32_t rN = 0;
        for (int i = 0; i < kBins - 1; i++) {
            const int s = kBins - 1 - i, d = kBins - 2 - i;
            for (int k = 0; k < 3; k++) { rBMin[d][k] = r1[k] = min_ref(r1[k], b.mn[s][k]); rBMax[d][k] = r2[k] = max_ref(r2[k], b.mx[s][k]); }
            rN += b.nout[s];
            NR[d] = (int)rN;
            AR[d] = rN == 0 ? kFar : area3(r2, r1);
        }
    }
    uint32_t refused = 0;
    float l1[3] = {kFar, kFar, kFar}, l2[3] = {-kFar, -kFar, -kFar};
    uint32_t lN = 0;
    for (int i = 0; i < kBins - 1; i++) {
        for (int k = 0; k < 3; k++) { l1[k] = min_ref(l1[k], b.mn[i][k]); l2[k] = max_ref(l2[k], b.mx[i][k]); }
        lN += b.nin[i];
        const float AL = lN == 0 ? kFar : area3(l2, l1);
        const int NL = (int)lN;
        const float C = split_cost(rSAV, AL, NL, AR[i], NR[i]);
        if (!spatial) {
            if (C >= best.splitCost) continue;
            best.splitCost = C;
        } else {
            const bool alive = (int)((uint32_t)NL * (uint32_t)NR[i]) > 0;
            if (!(C < minSplitCost && alive)) continue;
            if (!(NL + NR[i] < budget)) { refused++; continue; }
            best.spatial = true; minSplitCost = best.splitCost = C;
            best.nl = NL; best.nr = NR[i];
        }
        best.axis = (uint32_t)a; best.pos = (uint32_t)i;
        for (int k = 0; k < 3; k++) { best.lmin[k] = l1[k]; best.lmax[k] = l2[k]; best.rmin[k] = rBMin[i][k]; best.rmax[k] = rBMax[i][k]; }
        if (spatial) best.lmax[a] = best.rmin[a];   // "accurate" (2869)
    }
    return refused;
}

// budget > triCount && (overlap of the object split's children / rootArea > 1e-4f || no object split found) (2807-2810).  Without an object split
// bestLMax / bestRMin are whatever the task's last node left there; the second operand is true then, so they are never looked at here.
SAH_HD bool spatial_eligible(const Best& best, float noSplitCost, int budget, uint32_t triCount, float rootArea) {
    if (!(budget > (int)triCount)) return false;
    if (best.splitCost >= noSplitCost) return true;
    const float u[3] = {best.lmax[0] - best.rmin[0], best.lmax[1] - best.rmin[1], best.lmax[2] - best.rmin[2]};
    return sah::half_area(u[0], u[1], u[2]) / rootArea > 1e-4f;
}

// ---- clipping -------------------------------------------------------------------------------------------------------------------------------

// BVH::ClipFrag: v = the triangle's three vertices.  *generic (statistics): the fragment had been clipped before, all six planes were used.
SAH_HD bool clip_frag(const Frag& orig, const float v[3][3], const float bmin_[3], const float bmax_[3], const float minDim[3], uint32_t axis, Frag& out,
                      bool& generic) {
    float bmin[3], bmax[3], extent[3];
    for (int k = 0; k < 3; k++) { bmin[k] = max_ref(bmin_[k], orig.mn[k]); bmax[k] = min_ref(bmax_[k], orig.mx[k]); extent[k] = bmax[k] - bmin[k]; }
    out.prim = orig.prim; out.clipped = 1;
    generic = orig.clipped != 0;
    if (orig.clipped) {
        float vin[kMaxPoly][3], vout[kMaxPoly][3];
        uint32_t Nin = 3;
        for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) vin[i][k] = v[i][k];
        for (uint32_t a = 0; a < 3; a++) {
            const float eps = minDim[a];
            if (!(extent[a] > eps)) continue;
            uint32_t Nout = 0;
            const float l = bmin[a], r = bmax[a];
            for (uint32_t i = 0; i < Nin; i++) {
                const float* v0 = vin[i]; const float* v1 = vin[(i + 1) % Nin];
                const bool v0in = v0[a] >= l - eps, v1in = v1[a] >= l - eps;
                if (!(v0in || v1in)) continue;
                if (v0in ^ v1in) {
                    const float f = (l - v0[a]) / (v1[a] - v0[a]);
                    if (Nout < (uint32_t)kMaxPoly) { for (int k = 0; k < 3; k++) vout[Nout][k] = lerp(v0[k], v1[k], f); vout[Nout][a] = l; Nout++; }
                }
                if (v1in && Nout < (uint32_t)kMaxPoly) { for (int k = 0; k < 3; k++) vout[Nout][k] = v1[k]; Nout++; }
            }
            Nin = 0;
            for (uint32_t i = 0; i < Nout; i++) {
                const float* v0 = vout[i]; const float* v1 = vout[(i + 1) % Nout];
                const bool v0in = v0[a] <= r + eps, v1in = v1[a] <= r + eps;
                if (!(v0in || v1in)) continue;
                if (v0in ^ v1in) {
                    const float f = (r - v0[a]) / (v1[a] - v0[a]);
                    if (Nin < (uint32_t)kMaxPoly) { for (int k = 0; k < 3; k++) vin[Nin][k] = lerp(v0[k], v1[k], f); vin[Nin][a] = r; Nin++; }
                }
                if (v1in && Nin < (uint32_t)kMaxPoly) { for (int k = 0; k < 3; k++) vin[Nin][k] = v1[k]; Nin++; }
            }
        }
        float mn[3] = {kFar, kFar, kFar}, mx[3] = {-kFar, -kFar, -kFar};
        for (uint32_t i = 0; i < Nin; i++) for (int k = 0; k < 3; k++) { mn[k] = min_ref(mn[k], vin[i][k]); mx[k] = max_ref(mx[k], vin[i][k]); }
        for (int k = 0; k < 3; k++) { out.mn[k] = max_ref(mn[k], bmin[k]); out.mx[k] = min_ref(mx[k], bmax[k]); }
        return Nin > 0;
    }
    // not clipped before: only the two planes on the split axis
    bool hasVerts = false;
    float mn[3] = {kFar, kFar, kFar}, mx[3] = {-kFar, -kFar, -kFar};
    if (extent[axis] > minDim[axis]) {
        const float l = bmin[axis], r = bmax[axis];
        float vout[4][3];
        uint32_t Nout = 0;
        const bool in[3] = {v[0][axis] >= l, v[1][axis] >= l, v[2][axis] >= l};
        for (int e = 0; e < 3; e++) {   // edges v0 v1, v1 v2, v2 v0
            const int i0 = e, i1 = e == 2 ? 0 : e + 1;
            if (!(in[i0] || in[i1])) continue;
            if (in[i0] ^ in[i1]) {
                const float f = clampf((l - v[i0][axis]) / (v[i1][axis] - v[i0][axis]), 0.0f, 1.0f);
                for (int k = 0; k < 3; k++) vout[Nout][k] = lerp(v[i0][k], v[i1][k], f);
                vout[Nout][axis] = l; Nout++;
            }
            if (in[i1]) { for (int k = 0; k < 3; k++) vout[Nout][k] = v[i1][k]; Nout++; }
        }
        for (uint32_t i = 0; i < Nout; i++) {
            const float* v0 = vout[i]; const float* v1 = vout[(i + 1) % Nout];
            const bool v0in = v0[axis] <= r, v1in = v1[axis] <= r;
            if (!(v0in || v1in)) continue;
            if (v0in ^ v1in) {
                const float f = clampf((r - v0[axis]) / (v1[axis] - v0[axis]), 0.0f, 1.0f);
                float C[3];
                for (int k = 0; k < 3; k++) C[k] = lerp(v0[k], v1[k], f);
                C[axis] = r; hasVerts = true;
                for (int k = 0; k < 3; k++) { mn[k] = min_ref(mn[k], C[k]); mx[k] = max_ref(mx[k], C[k]); }
            }
            if (v1in) { hasVerts = true; for (int k = 0; k < 3; k++) { mn[k] = min_ref(mn[k], v1[k]); mx[k] = max_ref(mx[k], v1[k]); } }
        }
    }
    for (int k = 0; k < 3; k++) { out.mn[k] = max_ref(mn[k], bmin[k]); out.mx[k] = min_ref(mx[k], bmax[k]); }
    return hasVerts;
}

// BVH::SplitFrag
SAH_HD void split_frag(const Frag& orig, const float v[3][3], const float minDim[3], uint32_t splitAxis, float splitPos, Frag& left, Frag& right, bool& leftOK,
                       bool& rightOK) {
    float vin[kMaxPoly][3], vout[kMaxPoly][3];
    uint32_t Nin = 3, Nout = 0;
    for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) vin[i][k] = v[i][k];
    if (orig.clipped) for (int a = 0; a < 3; a++) if ((orig.mx[a] - orig.mn[a]) > minDim[a]) {
        const float l = orig.mn[a], r = orig.mx[a];
        Nout = 0;
        for (uint32_t i = 0; i < Nin; i++) {
            const float* v0 = vin[i]; const float* v1 = vin[(i + 1) % Nin];
            const bool v0in = v0[a] >= l, v1in = v1[a] >= l;
            if (!(v0in || v1in)) continue;
            if (v0in ^ v1in) {
                const float f = clampf((l - v0[a]) / (v1[a] - v0[a]), 0.0f, 1.0f);
                if (Nout < (uint32_t)kMaxPoly) { for (int k = 0; k < 3; k++) vout[Nout][k] = lerp(v0[k], v1[k], f); vout[Nout][a] = l; Nout++; }
            }
            if (v1in && Nout < (uint32_t)kMaxPoly) { for (int k = 0; k < 3; k++) vout[Nout][k] = v1[k]; Nout++; }
        }
        Nin = 0;
        for (uint32_t i = 0; i < Nout; i++) {
            const float* v0 = vout[i]; const float* v1 = vout[(i + 1) % Nout];
            const bool v0in = v0[a] <= r, v1in = v1[a] <= r;
            if (!(v0in || v1in)) continue;
            if (v0in ^ v1in) {
                const float f = clampf((r - v0[a]) / (v1[a] - v0[a]), 0.0f, 1.0f);
                if (Nin < (uint32_t)kMaxPoly) { for (int k = 0; k < 3; k++) vin[Nin][k] = lerp(v0[k], v1[k], f); vin[Nin][a] = r; Nin++; }
            }
            if (v1in && Nin < (uint32_t)kMaxPoly) { for (int k = 0; k < 3; k++) vin[Nin][k] = v1[k]; Nin++; }
        }
    }
    // the two polygons are only ever reduced to their boxes: every vertex goes straight into its side's box (vleft / vright of the reference)
    uint32_t Nleft = 0, Nright = 0;
    for (int k = 0; k < 3; k++) { left.mn[k] = right.mn[k] = kFar; left.mx[k] = right.mx[k] = -kFar; }
    auto addL = [&](const float* p) { Nleft++; for (int k = 0; k < 3; k++) { left.mn[k] = min_ref(left.mn[k], p[k]); left.mx[k] = max_ref(left.mx[k], p[k]); } };
    auto addR = [&](const float* p) { Nright++; for (int k = 0; k < 3; k++) { right.mn[k] = min_ref(right.mn[k], p[k]); right.mx[k] = max_ref(right.mx[k], p[k]); } };
    for (uint32_t i = 0; i < Nin; i++) {
        const float* v0 = vin[i]; const float* v1 = vin[(i + 1) % Nin];
        const bool v0left = v0[splitAxis] < splitPos, v1left = v1[splitAxis] < splitPos;
        if (v0left && v1left) addL(v1);
        else if (!v0left && !v1left) addR(v1);
        else {
            const float f = clampf((splitPos - v0[splitAxis]) / (v1[splitAxis] - v0[splitAxis]), 0.0f, 1.0f);
            float C[3];
            for (int k = 0; k < 3; k++) C[k] = lerp(v0[k], v1[k], f);
            C[splitAxis] = splitPos;
            addL(C); addR(C);
            if (v0left) addR(v1); else addL(v1);
        }
    }
    left.clipped = right.clipped = 1; left.prim = right.prim = orig.prim;
    leftOK = Nleft > 0; rightOK = Nright > 0;
}

// ---- spatial binning of one fragment on one axis (2822-2844) -------------------------------------------------------------------------------
// sink.in( a, bin ), sink.out( a, bin ): countIn / countOut; sink.box( a, bin, mn, mx ): a (clipped) box into bin `bin` of axis a; fetch( prim, v ): the
// triangle's vertices, asked for only when the fragment overlaps more than one bin.
template <class Fetch, class Sink>
SAH_HD void spatial_bin_fragment(const Frag& f, const float nmin[3], const float nmax[3], const float minDim[3], int a, const Fetch& fetch, Sink& sink) {
    const float planeDist = plane_dist(nmin[a], nmax[a]), rPlaneDist = 1.0f / planeDist, nodeMin = nmin[a];
    const int bin1 = spatial_bin(f.mn[a], nodeMin, rPlaneDist), bin2 = spatial_bin(f.mx[a], nodeMin, rPlaneDist);
    sink.in(a, bin1); sink.out(a, bin2);
    if (bin2 == bin1) { sink.box(a, bin1, f.mn, f.mx); return; }
    float v[3][3];
    fetch(f.prim, v);
    for (int j = bin1; j <= bin2; j++) {
        float bmin[3] = {nmin[0], nmin[1], nmin[2]}, bmax[3] = {nmax[0], nmax[1], nmax[2]};
        bmin[a] = sah::fma1(planeDist, (float)j, nodeMin);
        bmax[a] = j == kBins - 2 ? nmax[a] : (bmin[a] + planeDist);
        Frag tmp;
        bool g;
        const bool ok = clip_frag(f, v, bmin, bmax, minDim, (uint32_t)a, tmp, g);
        if (ok) sink.box(a, j, tmp.mn, tmp.mx);
    }
}

// ---- the unsplit chain (2897-2925) ----------------------------------------------------------------------------------------------------------
// The state a spatially split node carries from one straddler to the next, in source order.
struct Chain {
    float lmin[3], lmax[3], rmin[3], rmax[3];
    int nl, nr;
    float splitCost;
};
enum { kToLeft = 0, kToRight = 1, kStraddler = 2, kSplit = 3 };

// kToLeft / kToRight: the straddler goes to that side whole and the state moves on; kSplit: it is cut at c.lmax[axis] AS IT IS NOW (an earlier
// straddler that went left whole has moved that plane), which does not touch the state.
SAH_HD int unsplit_step(Chain& c, const float fmn[3], const float fmx[3], float rSAV) {
    if (c.nr > 1) {
        float umn[3], umx[3];
        for (int k = 0; k < 3; k++) { umn[k] = min_ref(c.lmin[k], fmn[k]); umx[k] = max_ref(c.lmax[k], fmx[k]); }
        const float AL = area3(umx, umn), AR = area3(c.rmax, c.rmin);
        const float C = split_cost(rSAV, AL, c.nl, AR, c.nr - 1);
        if (C <= c.splitCost) {
            c.nr--; c.splitCost = C;
            for (int k = 0; k < 3; k++) { c.lmin[k] = umn[k]; c.lmax[k] = umx[k]; }
            return kToLeft;
        }
    }
    if (c.nl > 1) {
        float umn[3], umx[3];
        for (int k = 0; k < 3; k++) { umn[k] = min_ref(c.rmin[k], fmn[k]); umx[k] = max_ref(c.rmax[k], fmx[k]); }
        const float AL = area3(c.lmax, c.lmin), AR = area3(umx, umn);
        const float C = split_cost(rSAV, AL, c.nl - 1, AR, c.nr);
        if (C <= c.splitCost) {
            c.nl--; c.splitCost = C;
            for (int k = 0; k < 3; k++) { c.rmin[k] = umn[k]; c.rmax[k] = umx[k]; }
            return kToRight;
        }
    }
    return kSplit;
}

// where a position of a spatially split node goes before the chain has its say (2891-2893)
SAH_HD int classify(const Frag& f, uint32_t axis, uint32_t pos, float nodeMin, float rPlaneDist) {
    const uint32_t bin1 = partition_bin(f.mn[axis], nodeMin, rPlaneDist), bin2 = partition_bin(f.mx[axis], nodeMin, rPlaneDist);
    return bin2 <= pos ? kToLeft : bin1 > pos ? kToRight : kStraddler;
}

}  // namespace sbvh
}  // namespace tbvh
