// copy_policy_driver.cpp — drives CopyPolicy (tinybvh_amd/csrc/copy_policy.h) from a list of events on stdin, one per line, and prints the call's result
// and the whole state after each (tests/test_copy_policy.py builds it with g++ and compares with values written out there).
//   d <kinds>              dropped(kinds)                   result printed as 0
//   q [<times>]            query(), <times> times           result: that of the LAST call; `first` = the 1-based call that returned non-zero first (0: none)
//   r <totalRays> <0|1>    refit(totalRays, hasCopies)
// Output per event: result first pendingCopies recopyAfter queriesSinceUpdate remadeSinceUpdate raysAtRefit refitSeen
#include <cinttypes>
#include <cstdio>

#include "copy_policy.h"

int main() {
    tbvh_capi::CopyPolicy p;
    char line[128];
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a = 0, b = 0;
        char op = 0;
        const int got = sscanf(line, " %c %llu %llu", &op, &a, &b);
        if (got < 1 || op == '#') continue;
        unsigned result = 0;
        unsigned long long first = 0;
        if (op == 'd' && got >= 2) p.dropped((uint8_t)a);
        else if (op == 'q') {
            const unsigned long long times = got >= 2 ? a : 1;
            for (unsigned long long i = 1; i <= times; i++) {
                result = p.query();
                if (result && !first) first = i;
            }
        } else if (op == 'r' && got >= 3) result = p.refit(a, b != 0) ? 1u : 0u;
        else { fprintf(stderr, "bad event: %s", line); return 2; }
        printf("%u %llu %u %u %u %d %" PRIu64 " %d\n", result, first, (unsigned)p.pendingCopies, (unsigned)p.recopyAfter, (unsigned)p.queriesSinceUpdate,
               (int)p.remadeSinceUpdate, p.raysAtRefit, (int)p.refitSeen);
    }
    return 0;
}
