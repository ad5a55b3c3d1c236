// tlas_plan.h — which two-level kernel serves a TLAS, for each kind of query, and what the TLAS must hold for it: the arrays each BLAS is entered
// through, the class of those arrays, the wide TLAS trees wanted.  No HIP in here, like launch_plan.h and overlap_lanes.h: plain rules over the facts the
// caller states, so that they are tested on the CPU (tests/test_tlas_plan_host.py through tbvh_debug_tlas_plan).  capi_scene.hip (reclassifyTlas) states the
// facts and stores the plan whenever a BLAS's copies, its pin or the TLAS's size change; capi_query.hip reads the stored plan at every launch.
//
// The rule (closest-hit = Intersect, any-hit = IsOccluded; a view = the arrays a TLAS enters a BLAS through):
//    1. A pinned BLAS (tbvh_set_variant != 0) is entered through its own arrays.
//    2. Otherwise a closest-hit query enters a BVH_GPU or BVH8_CWBVH BLAS through its 4-wide copy, if the BLAS has one and 4-wide copies are allowed.
//    3. Otherwise a BVH_GPU BLAS (either kind of query) or a BVH4_GPU BLAS (any-hit only) is entered through its 8-wide copy, if it has one.
//    4. Otherwise the BLAS is entered through its own arrays.
//    5. A kind's class is the views' common layout, or 0.
//    6. `mix` means class 0 with no BVH4_GPU view: the reference's two BLAS types, BVH8_CWBVH and BVH_GPU (traverse_tlas.cl:50-72).
//    7. If the closest-hit class comes out 0 without `mix` (a BLAS too small for a copy next to copied ones), it is formed again with 4-wide copies
//       disallowed.
//    8. Any-hit queries get a class of their own only if the TLAS has had an any-hit query (anyHitSeen), some BLAS's any-hit view differs from its
//       closest-hit view, and the any-hit class is BVH8_CWBVH or `mix`: a class the flat loop would serve is not worth a second descriptor table.
//       Without one, any-hit queries take the closest-hit views and class.
//    9. A TLAS with a sphere BLAS has one class for both kinds: every BLAS through its own arrays, no copies, no wide trees.
//   10. The 8-wide tree is wanted if a class in use is BVH8_CWBVH or `mix`.  It fits up to 0x00ffffff nodes (wide-node indices share a word with 8 flag bits).
//   11. The 4-wide tree is wanted if the closest-hit class is BVH4_GPU.  It fits up to 0x7fffffff blocks (31-bit block offsets).
//       (A tree of a TLAS that has no nodes yet — tbvh_upload_tlas classifies before it copies — fits nothing.)
//   12. Family: spheres -> TlasSphere (the flat loop with the sphere step).
//   13. Class BVH4_GPU with the 4-wide tree wanted and fitting -> Tlas4.
//   14. Class BVH8_CWBVH or `mix` with the 8-wide tree wanted and fitting -> Tlas8.
//   15. Class VOXELSET -> TlasVoxel (tbvh_upload_tlas admits voxel sets only all together).
//   16. Class BVH_GPU -> Tlas2 (the TLAS already has their node format).
//   17. Otherwise TlasFlat, with the class layout (0 = per instance).
//   18. A TLAS whose BLASes are in watertight mode (tbvh_set_triangle_test; tbvh_upload_tlas admits all or none) has one class for both kinds: every BLAS
//       through BVH8_CWBVH arrays — its own, or its 8-wide copy, which a watertight BVH_GPU / BVH4_GPU BLAS always has —, no 4-wide copies, the 8-wide tree,
//       Tlas8 in its watertight form.  No other two-level kernel has one: a plan that comes out otherwise (the 8-wide tree does not fit) is an error of the
//       caller's operation, never another kernel.
// Tlas8, TlasFlat and TlasSphere push 8-byte stack entries, the others 4-byte ones.
#pragma once
#include <cstdint>

namespace tbvh_capi {

constexpr int kTlasLayoutSphere = 1, kTlasLayoutBvhGpu = 5, kTlasLayoutBvh4Gpu = 8, kTlasLayoutCwbvh = 10, kTlasLayoutVoxel = 12;   // TBVH_LAYOUT_* (capi_internal.h holds them together)
constexpr uint64_t kTlas8MaxNodes = 0x00ffffffull, kTlas4MaxBlocks = 0x7fffffffull;

enum TlasView : uint8_t { kViewOwn = 0, kViewWide8 = 1, kViewWide4 = 2 };
enum class TlasFamily : uint32_t { kTlasSphere = 0, kTlas4 = 1, kTlas8 = 2, kTlasVoxel = 3, kTlas2 = 4, kTlasFlat = 5 };

struct TlasBlasFacts {
    int layout = 0;
    bool pinned = false;          // variant != 0
    bool has8 = false, has4 = false;   // its 8-wide / 4-wide copy exists
    bool watertight = false;           // its triangle test (tbvh_set_triangle_test)
};

struct TlasFacts {
    const TlasBlasFacts* blas = nullptr;
    uint32_t nBlas = 0;
    bool anyHitSeen = false;
    bool hasNodes = false;        // the TLAS's own nodes are on the device
    uint64_t cap8 = 0, cap4 = 0;  // tlas8_cap_nodes / tlas4_cap_blocks of the TLAS as it is (kernels_tlaswide.hip)
};

struct TlasKindPlan {
    int layout = 0;               // the class (0 = the views mix layouts)
    bool mix = false;
    TlasFamily family = TlasFamily::kTlasFlat;
    uint32_t entryBytes = 8;      // of a stack entry
};

struct TlasPlan {
    TlasKindPlan kind[2];         // [0] closest-hit, [1] any-hit (equal to [0] without a class of its own)
    bool anyOwn = false;          // any-hit queries have views and a class of their own
    bool spheres = false;
    bool watertight = false;      // sentence 18
    bool want8 = false, fits8 = false, want4 = false, fits4 = false;
};

// sentences 1 - 4
inline TlasView tlasBlasView(const TlasBlasFacts& b, bool any, bool allow4) {
    if (b.pinned) return kViewOwn;
    if (!any && allow4 && b.has4 && (b.layout == kTlasLayoutBvhGpu || b.layout == kTlasLayoutCwbvh)) return kViewWide4;
    if (b.has8 && (b.layout == kTlasLayoutBvhGpu || (any && b.layout == kTlasLayoutBvh4Gpu))) return kViewWide8;
    return kViewOwn;
}

inline int tlasViewLayout(const TlasBlasFacts& b, TlasView v) { return v == kViewWide4 ? kTlasLayoutBvh4Gpu : v == kViewWide8 ? kTlasLayoutCwbvh : b.layout; }

// sentences 10 - 17 over classes already formed: which trees fit, which family serves each kind.  Also on its own when only the TLAS's size changed
// (an update, a device rebuild: the views stay), and with a capacity beyond every limit for a tree that could not be allocated.
inline void planTlasFit(TlasPlan& p, bool hasNodes, uint64_t cap8, uint64_t cap4) {
    p.fits8 = p.want8 && hasNodes && cap8 <= kTlas8MaxNodes;
    p.fits4 = p.want4 && hasNodes && cap4 <= kTlas4MaxBlocks;
    for (TlasKindPlan& k : p.kind) {
        using F = TlasFamily;
        k.family = p.spheres ? F::kTlasSphere
                 : k.layout == kTlasLayoutBvh4Gpu && p.fits4 ? F::kTlas4
                 : (k.layout == kTlasLayoutCwbvh || k.mix) && p.fits8 ? F::kTlas8
                 : k.layout == kTlasLayoutVoxel ? F::kTlasVoxel
                 : k.layout == kTlasLayoutBvhGpu ? F::kTlas2 : F::kTlasFlat;
        k.entryBytes = (k.family == F::kTlasSphere || k.family == F::kTlas8 || k.family == F::kTlasFlat) ? 8u : 4u;
    }
}

// The plan of a TLAS.  view[0] / view[1]: nBlas entries each, the closest-hit and any-hit view of every BLAS.
inline TlasPlan planTlas(const TlasFacts& f, TlasView* const* view) {
    TlasPlan p;
    for (uint32_t i = 0; i < f.nBlas; i++) { p.spheres |= f.blas[i].layout == kTlasLayoutSphere; p.watertight |= f.blas[i].watertight; }
    // sentences 5 and 6 over one kind's views
    auto form = [&](int kind, bool any, bool allow4) {
        int layout = 0;
        bool bvh4 = false;
        for (uint32_t i = 0; i < f.nBlas; i++) {
            const TlasView v = p.spheres ? kViewOwn
                               : p.watertight ? ((f.blas[i].layout != kTlasLayoutCwbvh && f.blas[i].has8 && !f.blas[i].pinned) ? kViewWide8 : kViewOwn)   // sentence 18
                                              : tlasBlasView(f.blas[i], any, allow4);
            const int l = tlasViewLayout(f.blas[i], v);
            view[kind][i] = v;
            layout = i == 0 ? l : (layout == l ? layout : 0);
            bvh4 |= l == kTlasLayoutBvh4Gpu;
        }
        p.kind[kind].layout = layout;
        p.kind[kind].mix = !p.spheres && layout == 0 && !bvh4;
    };
    form(0, false, true);
    if (!p.spheres && !p.watertight && p.kind[0].layout == 0 && !p.kind[0].mix) form(0, false, false);   // sentence 7
    if (!p.spheres && !p.watertight) {
        form(1, true, true);
        bool differs = false;
        for (uint32_t i = 0; i < f.nBlas; i++) differs |= view[1][i] != view[0][i];
        p.anyOwn = f.anyHitSeen && differs && (p.kind[1].layout == kTlasLayoutCwbvh || p.kind[1].mix);   // sentence 8
    }
    if (!p.anyOwn) {
        p.kind[1] = p.kind[0];
        for (uint32_t i = 0; i < f.nBlas; i++) view[1][i] = view[0][i];
    }
    if (!p.spheres) {
        for (const TlasKindPlan& k : p.kind) p.want8 |= k.layout == kTlasLayoutCwbvh || k.mix;
        p.want4 = p.kind[0].layout == kTlasLayoutBvh4Gpu;
    }
    planTlasFit(p, f.hasNodes, f.cap8, f.cap4);
    return p;
}

// The facts and the plan as flat words: what tbvh_debug_tlas_plan reads and writes and tbvh_debug_tlas_state reports.
//   facts: {BLAS count n, anyHitSeen, nodes present, 8-wide capacity in nodes, 4-wide capacity in blocks}, then one word per BLAS:
//          layout | pinned << 8 | has an 8-wide copy << 9 | has a 4-wide copy << 10 | watertight << 11
//   plan:  closest-hit {class layout, mix, family, stack entry bytes}, any-hit {the same four}, any-hit has a class of its own, 8-wide tree wanted, fits,
//          4-wide tree wanted, fits, then one word per BLAS: closest-hit view | any-hit view << 8 (0 own arrays, 1 8-wide copy, 2 4-wide copy)
constexpr uint32_t kTlasFactHead = 5, kTlasPlanHead = 13;

inline TlasBlasFacts tlasBlasFactsFromWord(uint64_t w) {
    TlasBlasFacts b;
    b.layout = (int)(w & 0xff); b.pinned = (w >> 8 & 1) != 0; b.has8 = (w >> 9 & 1) != 0; b.has4 = (w >> 10 & 1) != 0; b.watertight = (w >> 11 & 1) != 0;
    return b;
}
inline uint64_t tlasBlasFactsToWord(const TlasBlasFacts& b) { return (uint64_t)(b.layout & 0xff) | (uint64_t)b.pinned << 8 | (uint64_t)b.has8 << 9 | (uint64_t)b.has4 << 10 | (uint64_t)b.watertight << 11; }

inline void tlasPlanToWords(const TlasPlan& p, const TlasView* const* view, uint32_t nBlas, uint32_t* out) {
    for (int k = 0; k < 2; k++) {
        out[4 * k] = (uint32_t)p.kind[k].layout; out[4 * k + 1] = p.kind[k].mix; out[4 * k + 2] = (uint32_t)p.kind[k].family; out[4 * k + 3] = p.kind[k].entryBytes;
    }
    out[8] = p.anyOwn; out[9] = p.want8; out[10] = p.fits8; out[11] = p.want4; out[12] = p.fits4;
    for (uint32_t i = 0; i < nBlas; i++) out[kTlasPlanHead + i] = (uint32_t)view[0][i] | (uint32_t)view[1][i] << 8;
}

}  // namespace tbvh_capi
