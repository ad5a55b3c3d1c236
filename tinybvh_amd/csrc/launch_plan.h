// launch_plan.h — what a query launch of n rays on a scene of b bytes will do (capi_query.hip: launchQuery): the class of the scene and of the batch, the
// grids, whether the batch is probed for its coherence, which kernels a BVH8_CWBVH launch is made of.  No HIP in here, like overlap_lanes.h: plain
// arithmetic over the facts the caller states, so that the rule is tested on the CPU (tests/test_launch_plan_host.py through tbvh_debug_launch_plan).
//
// Two steps, because the first decides something that changes a fact the second reads:
//   1. planBatch(facts): the classes and the grids.  `probed` is known from here on; the first probed launch on a scene makes the scene's copies for
//      incoherent batches (capi_copies.hip: prepareIncoherentCopies), after which hasPadded / hasHybrid / hasTrisPadded are stated again;
//   2. planShape(plan, facts): with the copies as they now are, the kernels of a BVH8_CWBVH launch and whether the probe's verdict may be remembered.
// What depends on the history of a context or a scene is not in here and stays with the caller: the tuner's choice of a schedule and its samples
// (CohTuner), the verdict memory's answer (probe_memory.h), the lanes (overlap_lanes.h).
//
// The scene classes (single-level BVH8_CWBVH and the rest alike, by the bytes of the uploaded blob without the library's own copies):
//   small: under 48 MB, the scene lives in the L2s: a third more waves of fewer rays each;  huge: beyond 384 MB, out of the Infinity Cache's reach.
// The probe: a BVH8_CWBVH scene between the two, batches of 2^21 rays and more (`probed`: deferred + gated, strict or packet schedule for a coherent
// batch, the incoherent flavor for the others); a small scene from 3 * 2^18 rays, a huge one from 6 * 2^20 (`probedSmall`: the packet kernel for a coherent
// batch, the scene's unprobed kernel behind it) unless the schedule pinned or measured for that class of batch size is a per-lane one (1 or 2): then the
// batch runs unprobed, as ONE kernel, and the caller notes the class (probedSmallCancelled).
#pragma once
#include <cstdint>

namespace tbvh_capi {

constexpr int kPlanLayoutCwbvh = 10;   // TBVH_LAYOUT_CWBVH (capi_internal.h holds the two together)
constexpr uint64_t kSmallSceneBytes = 48ull << 20, kHugeSceneBytes = 384ull << 20;

struct LaunchFacts {
    bool isTlas = false;
    int layout = 0, variant = 0;
    uint64_t blobBytes = 0;       // BVH8_CWBVH: node + triangle blocks as uploaded; otherwise the scene's bytes
    uint64_t n = 0;               // rays (the capacity, where only the device knows the count)
    bool sizeKnown = true;        // the host knows n
    bool any = false;             // IsOccluded
    bool gridOverride = false;    // TBVH_BLOCKS_PER_CU / TBVH_RAYS_PER_BLOCK given: no per-scene adjustment
    uint32_t numCUs = 0, blocks = 0, raysPerBlock = 0;   // blocks: the persistent grid (24 one-wave workgroups per CU unless overridden)
    uint32_t expFlags = 0;        // tbvh_debug_set_flags
    int cohTunerMode = 0;         // TBVH_COHERENT_TUNER pinned for the context
    int decided[4] = {0, 0, 0, 0};   // what the scene's tuners (closest or any hit, as `any` says) have settled on, per size class
    bool hasPadded = false, hasHybrid = false, hasTrisPadded = false;   // the scene's derived copies (tbvh_scene::cw)
    bool probeMemoryOn = true, skipTiming = false;
    int triTest = 0;              // the scene's triangle test (tbvh_set_triangle_test): 1 = watertight
};

// The kernels of a launch on a single-level BVH8_CWBVH scene (capi_query.hip: launchCwbvhKernels)
enum class CwbvhShape : uint32_t {
    kOneKernel = 0,       // the scene's kernel, probed or not
    kTwoFlavors = 1,      // the coherent flavor in the tuner's schedule, then the incoherent one on the hybrid node copy and the 64-byte triangle records
    kFlavorAndBehind = 2, // (probedSmall) the coherent flavor, then the scene's unprobed kernel for what the pool still holds
    kVariant90 = 3, kVariant91 = 4, kVariant92 = 5,   // diagnostic: the incoherent flavor / the coherent flavor / the packet kernel whatever the batch
};

struct LaunchPlan {
    bool small = false, huge = false;
    bool probed = false, probedSmall = false;
    bool probedSmallCancelled = false;   // probedSmall by size, taken back by the schedule of its class: the caller records sizeClass as the latest
    int sizeClass = 0;                   // which of the scene's four tuners the batch belongs to
    uint32_t blocksBase = 0;             // the grid by the batch's size: an incoherent or unprobed batch, and QueryArgs::baseBlocks of a probed one
    uint32_t blocks = 0;                 // the grid of a coherent batch: a third more waves when `probed` fills the persistent grid
    uint32_t blocks7Tlas = 0;            // the grid of the kernels built for 7 waves per SIMD (fullGrid7) where a launch fills the persistent grid:
    uint32_t blocks7Cwbvh = 0;           //   the two-level kernels keep the launch's grid otherwise, launch_cwbvh is told "no such grid" under gridOverride
    bool tunerMeasures = false;          // a CohTuner may time this launch: it and the launch after it do not overlap others
    bool soloCandidate = false;          // (planShape) a launch that could ever leave out its coherent flavor
    bool wantsVerdictSlot = false;       // (planShape) ... and whose verdict the host can read back: it asks for a slot and is remembered
    CwbvhShape shape = CwbvhShape::kOneKernel;   // (planShape)
    bool autoPad = false;                // (planShape) kOneKernel and the kernel behind of kFlavorAndBehind walk the padded node copy
    bool watertight = false;             // the scene is in watertight mode: ONE kernel, a watertight instantiation of the per-lane k_cwbvh on the packed nodes — never probed,
                                         //   so never the packet kernel or a two-flavor launch, no padded or hybrid copy, no verdict slot
};

inline uint32_t fullGrid7(const LaunchFacts& f) { return f.numCUs * 28u; }
inline int tunedSchedule(const LaunchFacts& f, int sizeClass) { return f.cohTunerMode ? f.cohTunerMode : f.decided[sizeClass]; }

// What the thresholds were measured on:
// A scene that (nearly) lives in the L2s — the Sponza class: < 48 MB of nodes and triangles against 8 x 4 MB of L2 plus the Infinity Cache — is
// latency-bound, not cache-bound: it runs best with a third more waves (32 per CU) of fewer rays each (measured +1..20 % on the Sponza stand-in from
// 0.26 M to 16.7 M rays; the same shape costs the 196 MB Bistro stand-in 5-10 % on bounce and shadow rays, which thrash the caches more with more waves).
// `probed`: BVH8_CWBVH scenes beyond the L2s (the `small` class runs dense triangle phases, where the gated schedule loses 15 %) but within reach
// of the Infinity Cache (beyond it camera rays are bound by memory too: 30 M / 60 M triangles lose 11 / 19 % under the gate), batches of 2 M
// rays and more: a probe of the batch's coherence (256 neighbouring ray pairs, sampled by every wave of the traversal kernel itself: kernels_cwbvh.hip)
// lets the traversal kernel pick its schedule for the launch; a coherent batch also gets a third more waves (the surplus leaves at once
// otherwise).  Bistro stand-in, 16.7 M rays: camera rays +4.5 %, shadow rays +6 %, bounce rays unchanged.
// `probedSmall`, scenes under 48 MB (round 6): batches of 768 k rays and more whose size the host knows are probed too — not for the deferred schedule (it
// loses there) but for the PACKET kernel: one traversal per wave traces the Sponza stand-in's camera rays 1.23 / 1.64 / 1.56 x as fast at 1 / 4.2 / 16.7 M
// rays, its shadow rays 0.97 / 1.51 / 1.74 x (profiles/r06_small_scene_packet.txt).  Two kernels back to back as on the larger scenes: the coherent
// flavor the scene's tuner has settled on (strict per-lane, or packet) leaves at once unless the batch is coherent, the unprobed kernel behind it
// takes what the pool still holds.
// The two-kernel launch costs a small launch 10-20 us (the probe, the second kernel's start and exit): where the scene's tuner has measured the per-lane
// kernel faster — the Dragon stand-in: a 16 x 4-pixel chunk of camera rays covers hundreds of its triangles, the packet walk is 5-8 x slower — or only
// a few us slower, the batch runs as before round 6: ONE unprobed kernel.  Only the measuring launches (6-9 per class of batch size) pay.
// ... and scenes beyond 384 MB (never probed either: the deferred schedule loses there), from 6 M rays on: the street at 12 M triangles traces 16.7 M camera
// rays at 7094 instead of 4718 MRays/s with the packet kernel — and 4.2 M at 3383 instead of 3733, shadow rays slower throughout: measured per class too.

// Step 1: everything that does not read the scene's derived copies.
inline LaunchPlan planBatch(const LaunchFacts& f) {
    LaunchPlan p;
    p.watertight = !f.isTlas && f.triTest != 0;
    const bool cwbvh = !f.isTlas && f.layout == kPlanLayoutCwbvh, noProbe = (f.expFlags & 64u) != 0 || p.watertight;
    p.small = !f.isTlas && !f.gridOverride && f.blobBytes < kSmallSceneBytes;
    p.huge = !p.small && f.blobBytes > kHugeSceneBytes;
    // persistent grid: 24 one-wave workgroups per CU for large batches (a third more on a small scene); small batches get about one workgroup per
    // raysPerBlock rays, never fewer than 4 per CU
    const uint32_t cap = p.small ? f.blocks + f.blocks / 3u : f.blocks, lo = f.numCUs * 4u;
    const uint64_t want = (f.n + f.raysPerBlock - 1) / f.raysPerBlock;
    p.blocksBase = (uint32_t)(want < lo ? lo : (want > cap ? cap : want));
    p.probed = cwbvh && !p.small && !p.huge && f.n >= (1ull << 21) && (f.variant == 0 || f.variant == 88) && !noProbe;
    p.sizeClass = (p.small && f.n < (3ull << 19)) ? 3 : f.n < (6ull << 20) ? 0 : f.n < (12ull << 20) ? 1 : 2;
    const bool bySize = cwbvh && (p.small || p.huge) && f.variant == 0 && f.sizeKnown && f.n >= (p.small ? (3ull << 18) : (6ull << 20)) && !noProbe &&
                        !f.gridOverride;
    const int m = tunedSchedule(f, p.sizeClass);
    p.probedSmallCancelled = bySize && (m == 1 || m == 2);
    p.probedSmall = bySize && !p.probedSmallCancelled;
    p.blocks = (p.probed && !f.gridOverride && p.blocksBase == f.blocks) ? f.blocks + f.blocks / 3u : p.blocksBase;   // 24 -> 32 workgroups per CU
    p.blocks7Tlas = (!f.gridOverride && p.blocks == f.blocks) ? fullGrid7(f) : p.blocks;
    p.blocks7Cwbvh = f.gridOverride ? 0xFFFFFFFFu : fullGrid7(f);
    p.tunerMeasures = (p.probed || p.probedSmall) && !tunedSchedule(f, p.sizeClass);
    return p;
}

// Step 2: what reads the derived copies, stated in `f` as they are after step 1's consequence (see above).
inline void planShape(LaunchPlan& p, const LaunchFacts& f) {
    const bool copies = f.hasHybrid && f.hasTrisPadded;
    p.autoPad = f.variant == 0 && f.hasPadded && !p.watertight;   // nodes beyond the Infinity Cache: the padded copy (padCwbvhIfLarge)
    const bool twoFlavors = (p.probed || p.probedSmall) && f.variant == 0 && ((!p.autoPad && copies) || p.probedSmall) && !(f.expFlags & 4u);
    p.shape = p.watertight                ? CwbvhShape::kOneKernel   // (its own kernel: capi_query.hip, launchCwbvhKernels; tbvh_set_variant refuses such a scene anyway)
              : (f.variant == 90 && copies) ? CwbvhShape::kVariant90
              : f.variant == 91           ? CwbvhShape::kVariant91
              : f.variant == 92           ? CwbvhShape::kVariant92
              : !twoFlavors               ? CwbvhShape::kOneKernel
              : p.probedSmall             ? CwbvhShape::kFlavorAndBehind
                                          : CwbvhShape::kTwoFlavors;
    // Only a launch that could ever go solo is given a slot and remembered: two flavors on the incoherent-batch copies, variant 0, nothing diagnostic
    // set — variant 88, the one-kernel launch of a padded scene and runs under debug flags neither ask the events nor take an entry of the table.
    p.soloCandidate = p.probed && f.variant == 0 && !f.hasPadded && copies && !f.expFlags && !f.cohTunerMode && !f.gridOverride;
    p.wantsVerdictSlot = p.soloCandidate && f.probeMemoryOn && !f.skipTiming && f.sizeKnown;
}

// The facts and the plan as flat words, in the order of the structs' members: what tbvh_debug_launch_plan reads and writes.
// (a 23rd fact word, the scene's triangle test, and a 16th plan word, `watertight`, are optional: callers from before the mode state 22 and read 15)
constexpr uint32_t kLaunchFactWords = 22, kLaunchPlanWords = 15, kLaunchFactWordsTest = 23, kLaunchPlanWordsTest = 16;

inline LaunchFacts launchFactsFromWords(const uint64_t* w, uint32_t nWords = kLaunchFactWords) {
    LaunchFacts f;
    f.isTlas = w[0] != 0; f.layout = (int)w[1]; f.variant = (int)w[2]; f.blobBytes = w[3]; f.n = w[4]; f.sizeKnown = w[5] != 0; f.any = w[6] != 0;
    f.gridOverride = w[7] != 0; f.numCUs = (uint32_t)w[8]; f.blocks = (uint32_t)w[9]; f.raysPerBlock = (uint32_t)w[10]; f.expFlags = (uint32_t)w[11];
    f.cohTunerMode = (int)w[12];
    for (int k = 0; k < 4; k++) f.decided[k] = (int)w[13 + k];
    f.hasPadded = w[17] != 0; f.hasHybrid = w[18] != 0; f.hasTrisPadded = w[19] != 0; f.probeMemoryOn = w[20] != 0; f.skipTiming = w[21] != 0;
    if (nWords > kLaunchFactWords) f.triTest = (int)w[22];
    return f;
}

inline void launchPlanToWords(const LaunchPlan& p, uint32_t* out, uint32_t nWords = kLaunchPlanWords) {
    if (nWords > kLaunchPlanWords) out[kLaunchPlanWords] = p.watertight;
    const uint32_t w[kLaunchPlanWords] = {p.small, p.huge, p.probed, p.probedSmall, p.probedSmallCancelled, (uint32_t)p.sizeClass, p.blocksBase, p.blocks,
                                          p.blocks7Tlas, p.blocks7Cwbvh, p.tunerMeasures, p.soloCandidate, p.wantsVerdictSlot, (uint32_t)p.shape, p.autoPad};
    for (uint32_t k = 0; k < kLaunchPlanWords; k++) out[k] = w[k];
}

}  // namespace tbvh_capi
