// scenegraph_sanitize.cpp — a stand-alone program for a sanitizer run of the host scene graph: it calls tbvh_host_scenegraph_* themselves
// (tinybvh_amd/csrc/scenegraph_host.cpp over scenegraph.h, compiled into this program: validation, compilation, the channels, the walk, the kernels' ancestor-chain form of it, the outputs) on heap
// arrays of EXACTLY the sizes the descriptor documents, for a chain, a fan and a skin at odd sizes, with every interpolation and value type, and through
// the refusals.  Any read or write past an array, and any undefined operation, stops it.  The library's error helper (capi_context.hip) is supplied here.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude -Itinybvh_amd/csrc \
//       tools/scenegraph_sanitize.cpp tinybvh_amd/csrc/scenegraph_host.cpp -o /tmp/scenegraph_sanitize && /tmp/scenegraph_sanitize
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tinybvh_amd.h"
#include "tinybvh_amd_debug.h"

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

// exactly-sized heap copies: the descriptor points into these and nowhere else
template <class T>
static T* exact(const std::vector<T>& v) {
    T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

static int run(uint32_t nNodes, uint32_t fresh, double& sum) {
    std::vector<int32_t> parent(nNodes);
    std::vector<float> T(nNodes * 3), Rq(nNodes * 4), S(nNodes * 3), M(nNodes * 16), Lc(nNodes * 16), W, times, values, ib;
    std::vector<uint32_t> nW(nNodes), interp, type, koff(1, 0), voff(1, 0), cAnim, cSamp, cNode, cTarget, inst, mesh, joff(1, 0), joint;
    for (uint32_t n = 0; n < nNodes; n++) {
        parent[n] = n == 0 ? -1 : (n % 3 == 0 ? 0 : (int32_t)(n - 1));   // chains hanging off a fan
        for (int i = 0; i < 3; i++) { T[3 * n + i] = unit() - 0.5f; S[3 * n + i] = 0.5f + unit(); }
        float q[4], l = 0;
        for (int i = 0; i < 4; i++) { q[i] = unit() - 0.5f; l += q[i] * q[i]; }
        for (int i = 0; i < 4; i++) Rq[4 * n + i] = q[i] / std::sqrt(l);
        for (int i = 0; i < 16; i++) { M[16 * n + i] = i % 5 == 0 ? 1.f : 0.f; Lc[16 * n + i] = i % 5 == 0 ? 1.f : 0.1f * unit(); }
        nW[n] = n % 4 == 1 ? 1 + n % 3 : 0;
        for (uint32_t i = 0; i < nW[n]; i++) W.push_back(unit());
    }
    auto sampler = [&](uint32_t in, uint32_t ty, uint32_t keys, uint32_t count, float t0) {
        interp.push_back(in); type.push_back(ty);
        float t = t0;
        for (uint32_t k = 0; k < keys; k++) { times.push_back(t); t += 0.1f + unit(); }
        const uint32_t per = ty == TBVH_GRAPH_VEC3 ? 3 : ty == TBVH_GRAPH_QUAT ? 4 : count;
        uint32_t nv = keys * per * (in == TBVH_GRAPH_SPLINE ? 3 : 1);
        if (ty == TBVH_GRAPH_FLOAT && in == TBVH_GRAPH_STEP) nv = keys > 1 ? keys - 1 : 1;                     // (the least the entry point accepts)
        if (ty == TBVH_GRAPH_FLOAT && in == TBVH_GRAPH_SPLINE && keys > 1) nv = ((keys - 1) * count + count - 1) * 3 + 2;
        if (ty != TBVH_GRAPH_FLOAT && in == TBVH_GRAPH_SPLINE && keys > 1) nv = ((keys - 1) * 3 + 2) * per;
        for (uint32_t i = 0; i < nv; i++) values.push_back(unit() * 2 - 1);
        koff.push_back((uint32_t)times.size()); voff.push_back((uint32_t)values.size());
        return (uint32_t)interp.size() - 1;
    };
    for (uint32_t a = 0; a < 2; a++)
        for (uint32_t n = 0; n < nNodes; n++) {
            const uint32_t in = (n + a) % 3, keys = n % 5 == 4 ? 1 : 2 + n % 4;
            const float t0 = n % 7 == 3 ? 0.3f : 0.f;
            if ((n + a) % 2 == 0) { cAnim.push_back(a); cSamp.push_back(sampler(in, TBVH_GRAPH_VEC3, keys, 0, t0)); cNode.push_back(n); cTarget.push_back(a ? 2 : 0); }
            cAnim.push_back(a); cSamp.push_back(sampler(in, TBVH_GRAPH_QUAT, keys, 0, t0)); cNode.push_back(n); cTarget.push_back(1);
            if (nW[n]) { cAnim.push_back(a); cSamp.push_back(sampler(in, TBVH_GRAPH_FLOAT, keys, nW[n], t0)); cNode.push_back(n); cTarget.push_back(3); }
        }
    for (uint32_t n = 0; n < nNodes; n += 2) inst.push_back(n);
    for (uint32_t u = 0; u < 2 && u < nNodes; u++) {
        mesh.push_back(u ? nNodes - 1 : 0);
        for (uint32_t n = u; n < nNodes; n += 1 + u) { joint.push_back(n); for (int i = 0; i < 16; i++) ib.push_back(i % 5 == 0 ? 1.f : 0.05f * unit()); }
        joff.push_back((uint32_t)joint.size());
    }
    tbvh_scenegraph_desc d;
    memset(&d, 0, sizeof d);
    d.flags = fresh; d.n_nodes = nNodes; d.n_samplers = interp.size(); d.n_animations = 2; d.n_channels = cNode.size(); d.n_instances = inst.size(); d.n_skin_uses = mesh.size();
    void* owned[32]; int nOwned = 0;
    auto keep = [&](auto* p) { owned[nOwned++] = (void*)p; return p; };
    d.parent = keep(exact(parent)); d.translation = keep(exact(T)); d.rotation = keep(exact(Rq)); d.scale = keep(exact(S)); d.matrix = keep(exact(M));
    d.local_transform = keep(exact(Lc)); d.n_weights = keep(exact(nW)); d.weights = keep(exact(W));
    d.sampler_interpolation = keep(exact(interp)); d.sampler_type = keep(exact(type)); d.sampler_key_offset = keep(exact(koff)); d.sampler_value_offset = keep(exact(voff));
    d.key_times = keep(exact(times)); d.key_values = keep(exact(values));
    d.channel_animation = keep(exact(cAnim)); d.channel_sampler = keep(exact(cSamp)); d.channel_node = keep(exact(cNode)); d.channel_target = keep(exact(cTarget));
    d.node_of_instance = keep(exact(inst)); d.skin_mesh_node = keep(exact(mesh)); d.skin_joint_offset = keep(exact(joff)); d.skin_joint_node = keep(exact(joint));
    d.skin_inverse_bind = keep(exact(ib));

    tbvh_host_scenegraph* g = nullptr;
    // the refusals: the last entry of an array is the bad one, so that it is found, named, and nothing is read past it
    ((uint32_t*)d.channel_node)[cNode.size() - 1] = nNodes;
    EXPECT(tbvh_host_scenegraph_create(&d, &g), TBVH_E_FORMAT);
    ((uint32_t*)d.channel_node)[cNode.size() - 1] = cNode.back();
    ((uint32_t*)d.skin_joint_node)[joint.size() - 1] = nNodes;
    EXPECT(tbvh_host_scenegraph_create(&d, &g), TBVH_E_FORMAT);
    ((uint32_t*)d.skin_joint_node)[joint.size() - 1] = joint.back();
    ((float*)d.key_times)[times.size() - 1] = NAN;
    EXPECT(tbvh_host_scenegraph_create(&d, &g), TBVH_E_FORMAT);
    ((float*)d.key_times)[times.size() - 1] = times.back();
    ((int32_t*)d.parent)[0] = (int32_t)nNodes - 1;
    if (nNodes > 1) EXPECT(tbvh_host_scenegraph_create(&d, &g), TBVH_E_FORMAT);
    ((int32_t*)d.parent)[0] = -1;
    d.n_channels = 1ull << 32;
    EXPECT(tbvh_host_scenegraph_create(&d, &g), TBVH_E_INVALID);
    d.n_channels = cNode.size();
    const float* savedScale = d.scale; d.scale = nullptr;
    EXPECT(tbvh_host_scenegraph_create(&d, &g), TBVH_E_INVALID);
    d.scale = savedScale;
    EXPECT(tbvh_host_scenegraph_create(nullptr, &g), TBVH_E_INVALID);
    EXPECT(tbvh_host_scenegraph_create(&d, &g), 0);
    for (int i = 0; i < nOwned; i++) free(owned[i]);   // the graph holds copies: the descriptor's arrays are the caller's again

    std::vector<float> out((size_t)nNodes * 16);
    const float dts[] = {0.f, 0.05f, 0.4f, -0.3f, 2.5f, NAN};
    for (float dt : dts) {
        EXPECT(tbvh_host_scenegraph_advance(g, dt), 0);
        for (int what = TBVH_GRAPH_TRS; what <= TBVH_GRAPH_TRIG; what++) {
            std::vector<char> dst(64 * (size_t)(nNodes + cNode.size() + joint.size()) + 64);
            EXPECT(tbvh_host_scenegraph_download(g, what, dst.data(), dst.size()), 0);
            EXPECT(tbvh_host_scenegraph_download(g, what, dst.data(), 0), what == TBVH_GRAPH_WEIGHTS && W.empty() ? 0 : TBVH_E_INVALID);
        }
        EXPECT(tbvh_host_scenegraph_download(g, TBVH_GRAPH_COMBINED, out.data(), out.size() * 4), 0);
        { uint64_t differ = 1; EXPECT(tbvh_debug_host_scenegraph_check_chains(g, &differ), 0); if (differ && dt == dt) { fprintf(stderr, "%llu nodes: the ancestor-chain product differs from the walk\n", (unsigned long long)differ); return 1; } }
        if (dt == dt) for (float v : out) if (v == v && std::fabs(v) < 1e30f) sum += v;
        if (dt != dt) { EXPECT(tbvh_host_scenegraph_set_time(g, 0, 0.2f), 0); EXPECT(tbvh_host_scenegraph_reset(g, 1), 0); }
    }
    EXPECT(tbvh_host_scenegraph_advance_animation(g, 1, 0.1f), 0);
    EXPECT(tbvh_host_scenegraph_advance_animation(g, 2, 0.1f), TBVH_E_INVALID);
    EXPECT(tbvh_host_scenegraph_advance(g, INFINITY), TBVH_E_INVALID);
    EXPECT(tbvh_host_scenegraph_set_time(g, 0, 1e30f), TBVH_E_INVALID);
    EXPECT(tbvh_host_scenegraph_set_local(g, nNodes, out.data()), TBVH_E_INVALID);
    EXPECT(tbvh_host_scenegraph_set_local(g, nNodes - 1, out.data()), 0);
    EXPECT(tbvh_host_scenegraph_update_nodes(g), 0);
    const float* p = nullptr; uint64_t n64 = 0; uint32_t n32 = 0;
    EXPECT(tbvh_host_scenegraph_instance_transforms(g, &p, &n64), 0);
    for (uint64_t i = 0; i < n64 * 16; i++) sum += p[i] == p[i] && std::fabs(p[i]) < 1e30f ? p[i] : 0;
    for (uint32_t u = 0; u < mesh.size(); u++) {
        EXPECT(tbvh_host_scenegraph_joint_matrices(g, u, &p, &n32), 0);
        for (uint32_t i = 0; i < n32 * 16; i++) sum += p[i] == p[i] && std::fabs(p[i]) < 1e30f ? p[i] : 0;
    }
    EXPECT(tbvh_host_scenegraph_joint_matrices(g, (uint32_t)mesh.size(), &p, &n32), TBVH_E_INVALID);
    for (uint32_t n = 0; n < nNodes; n++) {
        EXPECT(tbvh_host_scenegraph_morph_weights(g, n, &p, &n32), 0);
        if (n32 != nW[n]) { fprintf(stderr, "node %u: %u weights, not %u\n", n, n32, nW[n]); return 1; }
        for (uint32_t i = 0; i < n32; i++) sum += p[i] == p[i] ? p[i] : 0;
    }
    tbvh_host_scenegraph_free(g);
    return 0;
}

int main() {
    double sum = 0;
    for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 257u})
        for (uint32_t fresh : {0u, TBVH_SCENEGRAPH_FRESH_JOINTS})
            if (run(n, fresh, sum)) return 1;
    printf("scene graph host path: clean (checksum %.6f)\n", sum);
    return 0;
}
