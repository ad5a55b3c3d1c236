// overlap_lanes.h — which of a context's two launch lanes an independent query launch takes (capi_query.hip: launchQuery).  No HIP in here: the
// caller says which records have finished (LaneBook::prune) and carries out what decide() answers, so that the rule is tested on the CPU
// (tests/test_overlap_lanes_host.py, tools/overlap_lanes_sanitize.cpp).
//
// A lane is a stream.  Two launches on ONE lane run in the order they were enqueued; two launches on different lanes may run at the same time.
// A launch writes its ray records (and an any-hit launch its flags), so two launches whose byte ranges intersect must keep their order:
//   * no in-flight launch on either lane intersects the new one: it takes the lane the previous launch did not take (its tail is then filled
//     by this launch, and this launch's tail by the next one);
//   * in-flight launches on ONE lane intersect it: it takes THAT lane, behind them — stream order is the order;
//   * in-flight launches on both lanes intersect it, or the lane it should take already holds kMaxInFlight records: the lanes are joined (every
//     earlier launch on either lane comes before everything enqueued from here on; both lists are empty then) and it takes lane 0.
// A launch on a lane replaces the lane's records whose bytes it covers (LaneBook::add), so only launches on kMaxInFlight different buffers fill a list.
//
// When a launch may START is a second rule (LaneBook::gate): launches on different lanes start in the order they were enqueued, give or take `depth`
// launches.  depth 1: a launch waits for the start of the other lane's latest launch while that lane holds anything in flight.  depth 2: it waits for the
// start of the other lane's launch BEFORE its latest one, and only while that launch is still in flight — a caller that alternates two buffers (camera
// rays, bounce rays: C1 D1 C2 D2 ...) then has C(k+2) start in the tail of D(k) rather than behind the start of D(k+1), which stream order holds back until
// D(k) has ended.  Neither lane runs more than `depth` launches ahead of the other.  A join empties the history: nothing enqueued before it is waited for
// by name, the join itself orders it.  The rule orders launches that are independent; footprint conflicts are kept by the lane choice above and by stream
// order, never by it.  (Which launches then run side by side depends on the phase the two lanes settle into, not on the rule alone: in a loop C1 D1 C2 D2
// D(k) may run beside C(k), or — when something holds D(1) back to C(1)'s end — beside C(k + 1), where C(k + 2) waits as described:
// profiles/r09_runahead.txt, section 2.)
#pragma once
#include <cstdint>

namespace tbvh_capi {

struct ByteRange {
    uintptr_t lo = 0, hi = 0;   // [lo, hi); lo == hi: empty
    bool empty() const { return hi <= lo; }
};
inline bool rangesIntersect(const ByteRange& a, const ByteRange& b) { return !a.empty() && !b.empty() && a.lo < b.hi && b.lo < a.hi; }

struct LaneFootprint {          // what one launch touches: its ray records and, for an any-hit launch, its flags
    ByteRange rays, occ;
};
inline bool footprintsIntersect(const LaneFootprint& a, const LaneFootprint& b) {
    return rangesIntersect(a.rays, b.rays) || rangesIntersect(a.rays, b.occ) || rangesIntersect(a.occ, b.rays) || rangesIntersect(a.occ, b.occ);
}

inline bool rangeCovers(const ByteRange& outer, const ByteRange& inner) { return inner.empty() || (!outer.empty() && outer.lo <= inner.lo && inner.hi <= outer.hi); }
inline bool footprintCovers(const LaneFootprint& outer, const LaneFootprint& inner) { return rangeCovers(outer.rays, inner.rays) && rangeCovers(outer.occ, inner.occ); }

struct LaneChoice {
    int lane;    // 0 or 1
    bool join;   // join the lanes first (LaneBook::joined), then launch on `lane` (always 0 then)
};

struct LaneBook {
    static constexpr int kLanes = 2;
    static constexpr int kMaxInFlight = 8;
    struct Record { LaneFootprint fp; uint32_t slot; };   // slot: the caller's name for the launch's end event
    Record rec[kLanes][kMaxInFlight];
    int count[kLanes] = {0, 0};
    int lastLane = 1;           // the lane the previous launch took (the first launch of a context takes lane 0)
    static constexpr int kMaxDepth = 2;
    uint64_t recent[kLanes][kMaxDepth] = {};   // the caller's names (`id` of add) of each lane's last launches since the last join, latest first
    int nRecent[kLanes] = {0, 0};

    // done(lane, slot) -> true once that launch has finished: finished records leave, the others keep their order
    template <class Done>
    void prune(Done done) {
        for (int l = 0; l < kLanes; l++) {
            int kept = 0;
            for (int i = 0; i < count[l]; i++)
                if (!done(l, rec[l][i].slot)) rec[l][kept++] = rec[l][i];
            count[l] = kept;
        }
    }
    bool conflicts(int lane, const LaneFootprint& fp) const {
        for (int i = 0; i < count[lane]; i++) if (footprintsIntersect(rec[lane][i].fp, fp)) return true;
        return false;
    }
    // allowLane1 = false: lane 1 cannot be used for this launch (no resources for it): lane 0, joined first if lane 1 holds a conflicting launch
    LaneChoice decide(const LaneFootprint& fp, bool allowLane1 = true) const {
        const bool c0 = conflicts(0, fp), c1 = conflicts(1, fp);
        if (c0 && c1) return LaneChoice{0, true};
        int lane = c0 ? 0 : c1 ? 1 : (lastLane ^ 1);
        if (lane == 1 && !allowLane1) { if (c1) return LaneChoice{0, true}; lane = 0; }
        if (count[lane] >= kMaxInFlight) return LaneChoice{0, true};
        return LaneChoice{lane, false};
    }
    // The launch is enqueued on `lane`.  Records of that lane whose bytes are all among the new launch's leave: the new launch ends after them (stream order)
    // and conflicts with everything they conflict with, so it stands for them — a loop over the same few buffers keeps one record per buffer however many
    // of its launches are in flight, and never fills a list.
    // id: the caller's name for the launch in gate() (its start event); by default its slot
    void add(int lane, const LaneFootprint& fp, uint32_t slot) { add(lane, fp, slot, slot); }
    void add(int lane, const LaneFootprint& fp, uint32_t slot, uint64_t id) {
        for (int i = kMaxDepth - 1; i > 0; i--) recent[lane][i] = recent[lane][i - 1];
        recent[lane][0] = id;
        if (nRecent[lane] < kMaxDepth) nRecent[lane]++;
        int kept = 0;
        for (int i = 0; i < count[lane]; i++)
            if (!footprintCovers(fp, rec[lane][i].fp)) rec[lane][kept++] = rec[lane][i];
        count[lane] = kept;
        if (count[lane] < kMaxInFlight) rec[lane][count[lane]++] = Record{fp, slot};
        lastLane = lane;
    }
    void joined() { count[0] = count[1] = 0; nRecent[0] = nRecent[1] = 0; }
    // The launch whose START a new launch on `lane` waits for (the id given to add), or kNoGate.  Call after prune() and decide() (and joined(), if decide
    // asked for it), before add().  done(id) -> true once that launch has finished (asked at depth 2 only, and only about the launch it would name).
    static constexpr uint64_t kNoGate = ~0ull;
    template <class Done>
    uint64_t gate(int lane, int depth, Done done) const {
        const int o = lane ^ 1;
        if (depth <= 1) return (!idle(o) && nRecent[o] >= 1) ? recent[o][0] : kNoGate;
        if (nRecent[o] < 2 || done(recent[o][1])) return kNoGate;   // (the older of two unfinished: the latest has not finished either — stream order)
        return recent[o][1];
    }
    bool idle(int lane) const { return count[lane] == 0; }
};

}  // namespace tbvh_capi
