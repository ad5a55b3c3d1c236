// copy_policy.h — when a BLAS's derived copies (capi_copies.hip) are dropped, kept and made again: plain arithmetic on counters, no device and no scene
// involved, so a host program can drive it (tests/copy_policy_driver.cpp).
//
// tbvh_update_* (the reference's animation flow: BVH::Refit + ConvertFrom on the host, the blob re-uploaded) DROPS the copies — making them again costs
// milliseconds, more than a frame's queries gain — and they come back once the scene has answered `recopyAfter` queries without another update; an
// update that arrives soon after they came back quadruples that number (a blob that keeps changing ends up without copies, a blob updated once has
// them again after four queries).
// tbvh_refit refits the copies in place (0.3-0.5 ms each for 100 k triangles) — unless fewer than kRefitKeepRays rays were traced through the scene (or the
// TLASes over it) since the previous refit: then the copies cost a frame more than they save and are dropped like after an update.
#pragma once
#include <cstdint>

namespace tbvh_capi {

// the derived copies of a BLAS: the 8-wide one of a BVH_GPU / BVH4_GPU scene (made lazily, by its first query) and the 4-wide one of a BVH_GPU /
// BVH8_CWBVH BLAS (closest-hit queries of the TLASes over it).  The values are the bits of CopyPolicy::pendingCopies.
enum CopyKind { kCopyWide8 = 1, kCopyWide4 = 2 };

constexpr uint64_t kRefitKeepRays = 8ull << 20;   // a copy's refit (0.3-0.5 ms per 100 k triangles) pays from about this many rays per refit on (0.04-0.08 ns gained per ray)
constexpr uint64_t kWideCopyMin = 32768;          // blob entries from which a scene's own queries go through its 8-wide copy (TBVH_WIDE_COPY_MIN)

struct CopyPolicy {
    uint8_t pendingCopies = 0;           // CopyKind bits: dropped, to be made again
    uint32_t recopyAfter = 4, queriesSinceUpdate = 0;
    bool remadeSinceUpdate = false;
    uint64_t raysAtRefit = 0;            // rays traced through the scene + the TLASes over it, at the previous refit
    bool refitSeen = false;

    // the copies `liveKinds` were dropped (an update, or a refit that did not pay)
    void dropped(uint8_t liveKinds) {
        const uint8_t had = (uint8_t)(liveKinds | pendingCopies);
        if (!had) return;
        if (remadeSinceUpdate && recopyAfter < (1u << 20)) recopyAfter *= 4u;   // dropped again soon after the copies came back: a blob that keeps changing
        remadeSinceUpdate = false;
        pendingCopies = had; queriesSinceUpdate = 0;
    }
    // one query on the scene (or through a TLAS over it): the kinds to make again now, or 0
    uint8_t query() {
        if (!pendingCopies || ++queriesSinceUpdate < recopyAfter) return 0;
        const uint8_t kinds = pendingCopies;
        pendingCopies = 0; remadeSinceUpdate = true;
        return kinds;
    }
    // one refit, totalRays traced so far: true = the copies go instead of being refitted
    bool refit(uint64_t totalRays, bool hasCopies) {
        const bool drop = hasCopies && refitSeen && totalRays - raysAtRefit < kRefitKeepRays;
        refitSeen = true; raysAtRefit = totalRays;
        return drop;
    }
};

}  // namespace tbvh_capi
