// sahbuild_sanitize.cpp — a stand-alone program for a sanitizer run of the sequential SAH builder (tinybvh_amd/csrc/sahbuild_host.cpp over
// sah_split.h): random soups of 1..4000 triangles, degenerate sets (all triangles equal, all in a plane, two far clusters, zeros of both signs),
// flat and indexed, with and without SplitLeafs; every tree is walked: each primitive in exactly one leaf, leaves ascending and within the limit,
// every node inside its parent.  Any read or write past an array, and any undefined operation (the float -> int conversion of the bin index among
// them), stops it.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Itinybvh_amd/csrc tools/sahbuild_sanitize.cpp \
//       tinybvh_amd/csrc/sahbuild_host.cpp -o /tmp/sahbuild_sanitize && /tmp/sahbuild_sanitize
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "sahbuild.h"

using namespace tbvh;

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

static void walk(const std::vector<Node2>& nodes, const std::vector<uint32_t>& idx, uint32_t nTris, uint32_t maxLeaf) {
    std::vector<int> seen(nTris, 0);
    std::vector<uint32_t> stack{0};
    size_t visited = 0;
    while (!stack.empty()) {
        const uint32_t i = stack.back(); stack.pop_back();
        CHECK(i < nodes.size());
        visited++;
        const Node2& n = nodes[i];
        if (n.triCount) {
            CHECK(maxLeaf == 0 || n.triCount <= maxLeaf);
            CHECK((size_t)n.leftFirst + n.triCount <= idx.size());
            for (uint32_t k = 0; k < n.triCount; k++) {
                const uint32_t p = idx[n.leftFirst + k];
                CHECK(p < nTris);
                CHECK(k == 0 || idx[n.leftFirst + k - 1] < p);
                seen[p]++;
            }
        } else {
            CHECK(n.leftFirst >= 2 && (size_t)n.leftFirst + 1 < nodes.size());
            for (uint32_t c = n.leftFirst; c < n.leftFirst + 2; c++)
                for (int a = 0; a < 3; a++) CHECK(nodes[c].mn[a] >= n.mn[a] && nodes[c].mx[a] <= n.mx[a]);
            stack.push_back(n.leftFirst); stack.push_back(n.leftFirst + 1);
        }
    }
    CHECK(visited + 1 == nodes.size());
    for (int s : seen) CHECK(s == 1);
}

static void run(const std::vector<Vec4>& verts, const char* what) {
    const uint32_t nTris = (uint32_t)(verts.size() / 3);
    std::vector<uint32_t> indices(verts.size());
    for (size_t i = 0; i < indices.size(); i++) indices[i] = (uint32_t)(indices.size() - 1 - i);   // the same triangles, reversed, through an index buffer
    std::vector<Vec4> rev(verts.rbegin(), verts.rend());
    for (uint32_t k : {0u, 1u, 3u, 4u}) {
        std::vector<Node2> nodes, nodesI;
        std::vector<uint32_t> idx, idxI;
        CHECK(sah_build_host(HostMesh(verts.data()), nTris, k, nodes, idx) == nodes.size());
        walk(nodes, idx, nTris, k);
        sah_build_host(HostMesh(rev.data(), 16, indices.data()), nTris, k, nodesI, idxI);
        CHECK(nodesI.size() == nodes.size());
        walk(nodesI, idxI, nTris, k);
    }
    std::printf("%-28s %u triangles ok\n", what, nTris);
}

int main() {
    std::mt19937 rng(12345);
    std::uniform_real_distribution<float> pos(-10.f, 10.f), off(-0.6f, 0.6f);
    auto soup = [&](uint32_t n, float zscale, float shift) {
        std::vector<Vec4> v;
        for (uint32_t i = 0; i < n; i++) {
            const float c[3] = {pos(rng) + (i & 1 ? shift : 0.f), pos(rng), pos(rng) * zscale};
            for (int k = 0; k < 3; k++) v.push_back(Vec4{c[0] + off(rng), c[1] + off(rng), (c[2] + off(rng)) * zscale, 0.f});
        }
        return v;
    };
    for (uint32_t n : {1u, 2u, 3u, 5u, 9u, 64u, 65u, 700u, 4000u}) run(soup(n, 1.f, 0.f), "soup");
    run(soup(500, 0.f, 0.f), "flat (z = 0)");
    run(soup(600, 1.f, 1e6f), "two clusters 1e6 apart");
    {
        std::vector<Vec4> one = soup(1, 1.f, 0.f), v;
        for (int i = 0; i < 700; i++) v.insert(v.end(), one.begin(), one.end());
        run(v, "700 equal triangles");
    }
    {   // zeros of both signs, a denormal extent, huge coordinates
        std::vector<Vec4> v = soup(300, 1.f, 0.f);
        for (size_t i = 0; i < v.size(); i += 7) v[i].x = (i & 1) ? -0.f : 0.f;
        for (size_t i = 3; i < v.size(); i += 11) v[i].y = std::numeric_limits<float>::denorm_min() * (float)(i % 5);
        for (size_t i = 5; i < v.size(); i += 13) v[i].z = 3e37f;
        run(v, "signed zeros, denormals, 3e37");
    }
    std::printf("all ok\n");
    return 0;
}
