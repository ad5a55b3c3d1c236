// overlap_lanes_sanitize.cpp — a stand-alone program for a sanitizer run of the lane rule (tinybvh_amd/csrc/overlap_lanes.h, header only): the cases of
// tests/test_overlap_lanes_host.py on the book itself, then a long random script against a model that keeps EVERY launch in flight (no cap, no covering),
// checking the property the rule exists for: whenever the book lets two launches run on different lanes without a join between them, their bytes are
// disjoint.  Any read or write past the record arrays, and any undefined operation, stops it.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itinybvh_amd/csrc tools/overlap_lanes_sanitize.cpp \
//       -o /tmp/overlap_lanes_sanitize && /tmp/overlap_lanes_sanitize
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "overlap_lanes.h"
#include "probe_memory.h"

using namespace tbvh_capi;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

static LaneFootprint fp(uintptr_t lo, uintptr_t hi, uintptr_t olo = 0, uintptr_t ohi = 0) {
    LaneFootprint f;
    f.rays.lo = lo; f.rays.hi = hi; f.occ.lo = olo; f.occ.hi = ohi;
    return f;
}

struct Live { LaneFootprint f; int lane; bool done; };

int main() {
    {   // touching ranges are independent, one shared byte is not; empty ranges touch nothing
        CHECK(!rangesIntersect(ByteRange{0, 64}, ByteRange{64, 128}));
        CHECK(rangesIntersect(ByteRange{0, 65}, ByteRange{64, 128}));
        CHECK(!rangesIntersect(ByteRange{10, 10}, ByteRange{0, 100}));
        CHECK(rangeCovers(ByteRange{0, 100}, ByteRange{10, 10}) && !rangeCovers(ByteRange{10, 10}, ByteRange{0, 1}));
        CHECK(footprintsIntersect(fp(0, 640), fp(1000, 1640, 100, 110)));
    }
    {   // the full list: 8 launches that share bytes without covering each other, the ninth joins
        LaneBook b;
        for (uint32_t k = 0; k < 8; k++) {
            const LaneChoice ch = b.decide(fp(k, 64 + k));
            CHECK(ch.lane == 0 && !ch.join);
            b.add(0, fp(k, 64 + k), k);
        }
        CHECK(b.count[0] == LaneBook::kMaxInFlight);
        const LaneChoice ch = b.decide(fp(8, 72));
        CHECK(ch.join && ch.lane == 0);
        b.add(0, fp(8, 72), 8);             // (without the join the caller is told to make: the list stays within its array)
        CHECK(b.count[0] == LaneBook::kMaxInFlight);
        b.joined();
        CHECK(b.idle(0) && b.idle(1));
    }
    // random scripts: launches over a small address space (so that they collide often), random completions, the second lane going away and coming back
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&](uint64_t m) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng % m; };
    for (int script = 0; script < 200; script++) {
        LaneBook b;
        std::vector<Live> live;             // every launch since the last join that has not finished
        bool allow = true;
        for (uint32_t i = 0; i < 400; i++) {
            const uint64_t what = next(10);
            if (what == 0 && !live.empty()) {   // a launch finishes — and with it, by stream order, every earlier launch of its lane
                const size_t k = next(live.size());
                for (size_t j = 0; j <= k; j++) if (live[j].lane == live[k].lane) live[j].done = true;
                continue;
            }
            if (what == 1) { allow = next(4) != 0; continue; }
            const uintptr_t lo = 64 * next(24), len = 64 * (1 + next(6));
            const bool any = next(3) == 0;
            const uintptr_t olo = 4096 + next(24), olen = any ? 1 + next(6) : 0;
            const LaneFootprint f = fp(lo, lo + len, olo, olo + olen);
            // the caller's prune: finished launches leave.  The model keeps its own list; the book's records name launches by their index in it
            b.prune([&](int, uint32_t slot) { return slot < live.size() ? live[slot].done : true; });
            const LaneChoice ch = b.decide(f, allow);
            CHECK(ch.lane == 0 || (ch.lane == 1 && allow && !ch.join));
            if (ch.join) { b.joined(); live.clear(); }
            for (const Live& l : live)      // the property: a launch still running on the OTHER lane shares no byte with this one
                if (!l.done && l.lane != ch.lane) CHECK(!footprintsIntersect(l.f, f));
            // the start rule at either depth: the launch named is an unfinished one of the other lane since the last join — at depth 2 not that lane's latest
            for (int depth = 1; depth <= LaneBook::kMaxDepth; depth++) {
                const uint64_t g = b.gate(ch.lane, depth, [&](uint64_t id) { return id < live.size() ? live[id].done : true; });
                if (g == LaneBook::kNoGate) continue;
                CHECK(g < live.size() && live[g].lane != ch.lane);
                size_t later = 0;
                for (size_t j = (size_t)g + 1; j < live.size(); j++) later += live[j].lane == live[g].lane;
                CHECK(later == (size_t)depth - 1);
                if (depth == 2) CHECK(!live[g].done);
            }
            live.push_back(Live{f, ch.lane, false});
            b.add(ch.lane, f, (uint32_t)live.size() - 1);
            CHECK(b.count[0] >= 0 && b.count[0] <= LaneBook::kMaxInFlight && b.count[1] >= 0 && b.count[1] <= LaneBook::kMaxInFlight);
            CHECK(b.lastLane == ch.lane);
        }
    }
    // the verdict memory (probe_memory.h): random launches on a dozen footprints, random completions in lane order, against a model that keeps every
    // footprint's finished verdicts — a launch goes solo only if the model's last two for exactly that footprint are incoherent (the table may have
    // forgotten a footprint: never the other way round)
    for (int script = 0; script < 200; script++) {
        ProbeMemory m;
        struct Flight { ProbeKey key; int lane; uint8_t said; bool done, lost; };
        std::vector<Flight> flights;
        std::vector<std::vector<uint8_t>> votes(12);
        size_t harvested[2] = {0, 0};       // per lane: flights before this index have been offered to the table
        for (uint32_t i = 0; i < 600; i++) {
            if (next(3) == 0 && !flights.empty()) {
                const size_t k = next(flights.size());
                for (size_t j = 0; j <= k; j++) if (flights[j].lane == flights[k].lane) flights[j].done = true;
                continue;
            }
            if (flights.size() - (harvested[0] < harvested[1] ? harvested[0] : harvested[1]) >= 40)   // (the model has no cap on launches in flight; the memory's is 64)
                for (Flight& f : flights) f.done = true;
            const uint32_t which = (uint32_t)next(12);
            ProbeKey key;
            key.lo = 1000 * (which % 6); key.hi = key.lo + 1000; key.scene = (const void*)(uintptr_t)(1 + which / 6); key.any = false;
            m.harvest([&](uint64_t id) { return flights[id].lost ? 2 : flights[id].done ? 1 : 0; }, [&](uint64_t id) { return (int)flights[id].said; });
            for (int lane = 0; lane < 2; lane++)    // the model: what the table has been offered by now, in the same order
                for (size_t& j = harvested[lane]; j < flights.size(); j++) {
                    if (flights[j].lane != lane) continue;
                    if (!flights[j].done && !flights[j].lost) break;
                    if (!flights[j].lost && flights[j].said) votes[(flights[j].key.lo / 1000) + 6 * ((uintptr_t)flights[j].key.scene - 1)].push_back(flights[j].said);
                }
            const std::vector<uint8_t>& v = votes[which];
            const bool may = v.size() >= 2 && v[v.size() - 1] == ProbeMemory::kIncoherent && v[v.size() - 2] == ProbeMemory::kIncoherent;
            if (m.solo(key)) CHECK(may);
            CHECK(m.nPending >= 0 && m.nPending <= ProbeMemory::kPending);
            flights.push_back(Flight{key, (int)(which & 1u), (uint8_t)next(3), false, next(16) == 0});   // (launches on one buffer conflict: always the same lane)
            m.note(key, flights.size() - 1, flights.back().lane);
        }
    }
    std::puts("overlap_lanes: ok");
    return 0;
}
