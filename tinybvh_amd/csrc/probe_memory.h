// probe_memory.h — what a context remembers of the coherence probe's verdicts (cwbvh_probe.h), per ray buffer: when may a probed two-flavor launch
// (capi_query.hip: launchCwbvhKernels) leave out the coherent flavor, which an incoherent batch makes 8192 workgroups sample the probe and leave?
// No HIP in here, like overlap_lanes.h: the caller says which launches have finished and what their probe counted, so that the rule is tested on the CPU
// (tests/test_lane_runahead_host.py, tools/overlap_lanes_sanitize.cpp).
//
// A launch is remembered while in flight (note); once the caller has SEEN it finished, its verdict joins the table entry of its footprint (harvest):
// the exact ray range, closest or any hit, the scene.  A launch goes solo only if a footprint equal in all of these holds two verdicts and both said
// incoherent.  One coherent verdict, a footprint that merely overlaps, a launch still in flight: two flavors.  The prediction never decides which rays
// are traced — the incoherent flavor draws every ray from the pool whatever it is told — only whether a kernel that would have left at once is launched.
#pragma once
#include <cstdint>

namespace tbvh_capi {

struct ProbeKey {
    uintptr_t lo = 0, hi = 0;   // the ray records, [lo, hi)
    const void* scene = nullptr;
    bool any = false;
    bool operator==(const ProbeKey& o) const { return lo == o.lo && hi == o.hi && scene == o.scene && any == o.any; }
};

struct ProbeMemory {
    static constexpr int kEntries = 8, kPending = 64;
    enum Verdict : uint8_t { kNone = 0, kIncoherent = 1, kCoherent = 2 };
    struct Entry { ProbeKey key; uint8_t last[2] = {kNone, kNone}; uint64_t used = 0; bool live = false; };   // last[0]: the latest finished launch's verdict
    struct Pending { ProbeKey key; uint64_t id; int lane; };   // id: the caller's name for the launch (its end event and its verdict slot)
    Entry entry[kEntries];
    Pending pending[kPending];
    int nPending = 0;
    uint64_t tick = 0;

    // the launch is enqueued on `lane` (launches of one lane finish in the order they were noted)
    void note(const ProbeKey& key, uint64_t id, int lane) {
        if (nPending == kPending) {   // (a caller 64 launches ahead of the device: the oldest launch goes unremembered)
            for (int i = 1; i < nPending; i++) pending[i - 1] = pending[i];
            nPending--;
        }
        pending[nPending++] = Pending{key, id, lane};
    }
    // state(id) -> 0: still in flight, 1: finished, 2: finished or not, its verdict can no longer be had (it leaves without a vote);
    // verdict(id) -> what a finished launch's probe said (kNone: nothing).  A lane's launches are asked in order, up to the first still in flight.
    template <class State, class Read>
    void harvest(State state, Read verdict) {
        bool blocked[2] = {false, false};
        int kept = 0;
        for (int i = 0; i < nPending; i++) {
            const Pending p = pending[i];
            const int st = blocked[p.lane & 1] ? 0 : state(p.id);
            if (st == 0) { blocked[p.lane & 1] = true; pending[kept++] = p; continue; }
            if (st == 1) vote(p.key, (Verdict)verdict(p.id));
        }
        nPending = kept;
    }
    void vote(const ProbeKey& key, Verdict v) {
        if (v == kNone) return;
        Entry* e = nullptr;
        for (Entry& x : entry) if (x.live && x.key == key) e = &x;
        if (!e) {   // a new footprint takes a free entry, or the one that has gone longest without a verdict
            e = &entry[0];
            for (Entry& x : entry) {
                if (!x.live) { e = &x; break; }
                if (x.used < e->used) e = &x;
            }
            *e = Entry{};
            e->key = key; e->live = true;
        }
        e->last[1] = e->last[0]; e->last[0] = v;
        e->used = ++tick;
    }
    bool solo(const ProbeKey& key) const {
        for (const Entry& x : entry)
            if (x.live && x.key == key) return x.last[0] == kIncoherent && x.last[1] == kIncoherent;
        return false;
    }
    void clear() { *this = ProbeMemory{}; }
};

}  // namespace tbvh_capi
