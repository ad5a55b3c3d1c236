// pose_sanitize.cpp — a stand-alone program for a sanitizer run of the host pose path: it calls tbvh_host_pose_skin / tbvh_host_pose_morph themselves
// (tinybvh_amd/csrc/pose_host.cpp over pose.h, compiled into this program: validation, the joint-index check, the skin pass, the morph pass) on heap
// arrays of EXACTLY the sizes the entry points document, at the odd sizes the tests use, and through every refusal they make.  Any read or write past an
// array, and any undefined operation, stops it.  The library's error helper (capi_context.hip) is the one thing supplied here.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Itinybvh_amd/csrc \
//       tools/pose_sanitize.cpp tinybvh_amd/csrc/pose_host.cpp -o /tmp/pose_sanitize && /tmp/pose_sanitize
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "tinybvh_amd.h"

static char g_err[512];
namespace tbvh_capi {
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace tbvh_capi

#define EXPECT(call, want) do { const int rc_ = (call); if (rc_ != (want)) { fprintf(stderr, "%s -> %d, expected %d (%s)\n", #call, rc_, (want), g_err); return 1; } } while (0)

static uint32_t rng = 0x2545f491u;
static uint32_t next() { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return rng; }
static float unit() { return (float)(next() >> 8) * (1.0f / 16777216.0f); }

int main() {
    const uint64_t sizes[] = {1, 63, 64, 65, 3 * 313, 13056};
    const uint32_t jointCounts[] = {1, 24};
    double sum = 0;
    for (uint64_t n : sizes) {
        for (uint32_t nJoints : jointCounts) {
            std::unique_ptr<float[]> rest(new float[n * 4]), weights(new float[n * 4]), mats(new float[nJoints * 16]), out(new float[n * 4]);
            std::unique_ptr<uint32_t[]> joints(new uint32_t[n * 4]);
            for (uint64_t i = 0; i < n * 4; i++) { rest[i] = unit() * 4 - 2; weights[i] = unit(); joints[i] = next() % nJoints; }
            for (uint32_t i = 0; i < nJoints * 16; i++) mats[i] = (i % 16) / 5 * 5 == i % 16 ? 1.0f : unit() * 0.1f;   // near identity, last row not 0 0 0 1: the divide branch too
            joints[4 * (n - 1) + 3] = nJoints;   // the last index of the last vertex: found, named, and nothing is read past it or written
            out[0] = 123.0f;
            EXPECT(tbvh_host_pose_skin(rest.get(), n, joints.get(), weights.get(), mats.get(), nJoints, out.get()), TBVH_E_FORMAT);
            char want[64];
            snprintf(want, sizeof want, "vertex %llu:", (unsigned long long)(n - 1));
            if (!strstr(g_err, want) || out[0] != 123.0f) { fprintf(stderr, "bad joint index: '%s'\n", g_err); return 1; }
            joints[4 * (n - 1) + 3] = nJoints - 1;
            EXPECT(tbvh_host_pose_skin(nullptr, n, joints.get(), weights.get(), mats.get(), nJoints, out.get()), TBVH_E_INVALID);
            EXPECT(tbvh_host_pose_skin(rest.get(), n, joints.get(), weights.get(), mats.get(), 0, out.get()), TBVH_E_INVALID);
            EXPECT(tbvh_host_pose_skin(rest.get(), 0, joints.get(), weights.get(), mats.get(), nJoints, out.get()), TBVH_E_INVALID);
            EXPECT(tbvh_host_pose_skin(rest.get(), n, joints.get(), weights.get(), mats.get(), nJoints, out.get()), 0);
            for (uint64_t i = 0; i < n * 4; i++) sum += out[i];
        }
        for (uint32_t nTargets : {0u, 1u, 3u}) {
            std::unique_ptr<float[]> pos(new float[(nTargets + 1) * n * 3]), w(new float[nTargets ? nTargets : 1]), out(new float[n * 4]);
            for (uint64_t i = 0; i < (nTargets + 1) * n * 3; i++) pos[i] = unit() * 4 - 2;
            for (uint32_t t = 0; t < nTargets; t++) w[t] = unit() * 2 - 1;
            if (nTargets) EXPECT(tbvh_host_pose_morph(pos.get(), n, nTargets, nullptr, out.get()), TBVH_E_INVALID);
            EXPECT(tbvh_host_pose_morph(pos.get(), n, nTargets, nullptr, nullptr), TBVH_E_INVALID);
            EXPECT(tbvh_host_pose_morph(pos.get(), n, nTargets, nTargets ? w.get() : nullptr, out.get()), 0);
            for (uint64_t i = 0; i < n; i++) if (out[4 * i + 3] != 1.0f) { fprintf(stderr, "morph: w is not 1\n"); return 1; }
            for (uint64_t i = 0; i < n * 4; i++) sum += out[i];
        }
    }
    printf("pose host path: clean (checksum %.6f)\n", sum);
    return 0;
}
