// indexed_mesh.cpp — the README's "new indexed interface" through tinyhip: a tinybvh::BVH_GPU built over an index buffer —
// Build( vertices, indices, n ), and Build( bvhvec4slice( stride 32 ), indices, n ) over an interleaved buffer — uploaded as it is with
// tinyhip::Scene( gpu ), traced, refitted to moved shared vertices with Scene::Refit( slice ) and queried with IntersectSpheres( .., slice, .. ).
// Hit records are compared with the reference's own on the host (BVH::Intersect, Refit() + Intersect), sphere flags with the flat call.  A 24 x 24 height
// field: 625 shared vertices, 1 152 triangles.  Prints one line per form: "<form> rays <differing> of <n> refit <differing> spheres <differing>
// of <m> hits <k>" (tests/test_mesh_gpu.py: test_tiny_hip_indexed_binding_runs).  Built by __graft_entry__.build() where tiny_bvh.h is found.
#define TINYBVH_IMPLEMENTATION
#include "tiny_bvh.h"
#include "tiny_hip.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
using namespace tinybvh;

static float height(int x, int y, float phase) { return 0.15f * std::sin(0.7f * x + phase) * std::cos(0.5f * y - phase); }

int main() {
    const int N = 24, V = N + 1;
    std::vector<uint32_t> idx;
    for (int y = 0; y < N; y++) for (int x = 0; x < N; x++) {
        const uint32_t a = y * V + x, b = a + 1, c = a + V, d = c + 1;
        const uint32_t t[6] = {a, b, c, b, d, c};
        idx.insert(idx.end(), t, t + 6);
    }
    const uint32_t nTris = (uint32_t)idx.size() / 3, nVerts = V * V;
    for (int form = 0; form < 2; form++) {
        const uint32_t stride = form ? 32u : 16u;
        float* buf = (float*)malloc64((size_t)nVerts * stride + 64);
        auto fill = [&](float phase) {
            for (int y = 0; y < V; y++) for (int x = 0; x < V; x++) {
                float* p = buf + (size_t)(y * V + x) * (stride / 4);
                p[0] = x / (float)N; p[1] = y / (float)N; p[2] = height(x, y, phase); p[3] = 0;
                for (uint32_t k = 4; k < stride / 4; k++) p[k] = 7.5f;   // the interleaved attributes: nobody's business
            }
        };
        fill(0.f);
        const bvhvec4slice slice((const bvhvec4*)buf, nVerts, stride);
        BVH_GPU gpu;
        gpu.Build(slice, idx.data(), nTris);
        tinyhip::Scene scene(gpu);
        const int R = 4096;
        std::vector<Ray> rays, want;
        for (int i = 0; i < R; i++) {
            const float u = (i % 64 + 0.37f) / 64.f, v = (i / 64 + 0.61f) / 64.f;
            rays.push_back(Ray(bvhvec3(u, v, 2.f), tinybvh_normalize(bvhvec3(0.1f * (u - 0.5f), 0.07f * (v - 0.5f), -1.f))));
        }
        auto trace = [&](int& differ, int& hits) {
            std::vector<Ray> a = rays, b = rays;
            for (Ray& r : a) gpu.bvh.Intersect(r);
            scene.Intersect(b.data(), b.size());
            differ = hits = 0;
            for (int i = 0; i < R; i++) { differ += std::memcmp(&a[i].hit, &b[i].hit, 16) != 0; hits += b[i].hit.t < 1e30f; }
        };
        int d0, h0, d1, h1;
        trace(d0, h0);
        fill(1.3f);                       // the shared vertices move
        gpu.bvh.Refit();                  // the reference on the host ...
        scene.Refit(slice);               // ... the device refit, from the same slice
        trace(d1, h1);
        const int S = 1024;
        std::vector<bvhvec4> sph;
        for (int i = 0; i < S; i++) sph.push_back(bvhvec4((i % 32 + 0.5f) / 32.f, (i / 32 + 0.5f) / 32.f, -0.3f + 0.6f * ((i * 7) % 13) / 13.f, 0.02f + 0.002f * (i % 9)));
        std::vector<uint8_t> hit(S);
        scene.IntersectSpheres(sph.data(), S, slice, hit.data());
        // the flat call over the flattened triangles must answer the same (the reference's own IntersectSphere does not terminate for every
        // sphere, DESIGN.md par. 11: its answers are compared through the goldens of tests/golden/mesh instead)
        std::vector<bvhvec4> flat;
        for (uint32_t i = 0; i < nTris * 3; i++) flat.push_back(slice[idx[i]]);
        for (bvhvec4& v : flat) v.w = 0;
        std::vector<uint8_t> hitFlat(S);
        scene.IntersectSpheres(sph.data(), S, flat.data(), nTris, hitFlat.data());
        int ds = 0, touching = 0;
        for (int i = 0; i < S; i++) { ds += hit[i] != hitFlat[i]; touching += hit[i]; }
        std::printf("%s rays %d of %d refit %d spheres %d of %d hits %d %d touching %d\n", form ? "stride32" : "indexed", d0, R, d1, ds, S, h0, h1, touching);
        free64(buf);
    }
    return 0;
}
