// sphere_particles.cpp — a particle set that moves, from C++ (tinyhip::SphereBVH): the frame loop of tiny_bvh_anim.cpp, whose obj.Build( &sphereAABB, n )
// per frame becomes BuildOnDevice once, then Refit for a few frames of motion, then Rebuild when the particles have drifted.  After every step the same
// rays are traced and the program checks each record against a brute-force loop of its own over the moved spheres (the callback of custom_sphere.h
// restated: smallest recorded distance, then the smaller prim), prints the hit count per frame and "sphere particles ok".
// Built by __graft_entry__.build() where tiny_bvh.h is found (tests/test_custom_dynamic_gpu.py: test_example_runs).
#include "tiny_bvh.h"
#include "tiny_hip.h"
#include <cmath>
#include <cstdio>
#include <vector>

static uint32_t seed = 0x12345u;
static float rnd() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) * (1.0f / 16777216.0f); }

// the anim demo's callback for one ray over every sphere; D as the Ray constructor left it
static void brute(const std::vector<float>& sph, const tinybvh::Ray& r, float& tBest, uint32_t& primBest) {
    const float Dx = r.D.x, Dy = r.D.y, Dz = r.D.z;
    const float mag = std::sqrt(std::fmaf(Dz, Dz, std::fmaf(Dx, Dx, Dy * Dy))), reciMag = 1.0f / mag, tmaxMag = 1e30f * mag;
    tBest = 1e30f; primBest = 0xffffffffu;
    for (uint32_t i = 0; i < sph.size() / 4; i++) {
        const float ocx = r.O.x - sph[4 * i], ocy = r.O.y - sph[4 * i + 1], ocz = r.O.z - sph[4 * i + 2], rad = sph[4 * i + 3];
        const float b = std::fmaf(ocz, Dz, std::fmaf(ocx, Dx, ocy * Dy)) * reciMag;
        const float c = std::fmaf(-rad, rad, std::fmaf(ocz, ocz, std::fmaf(ocx, ocx, ocy * ocy)));
        const float d = std::fmaf(b, b, -c);
        if (d <= 0.f) continue;
        const float t = -b - std::sqrt(d);
        if (!(t < tmaxMag && t > 0.f)) continue;
        const float stored = t * reciMag;
        if (primBest == 0xffffffffu || stored < tBest) { tBest = stored; primBest = i; }   // (ascending i: the smaller prim keeps a tie)
    }
}

int main() {
    const uint32_t n = 3000, nRays = 2048;
    std::vector<float> sph(n * 4), vel(n * 3);
    for (uint32_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) { sph[4 * i + k] = rnd() * 20.f - 10.f; vel[3 * i + k] = rnd() * 0.4f - 0.2f; }
        sph[4 * i + 3] = 0.05f + 0.3f * rnd();
    }
    std::vector<tinybvh::Ray> rays;
    for (uint32_t i = 0; i < nRays; i++) {
        const tinybvh::bvhvec3 O(rnd() * 24.f - 12.f, rnd() * 24.f - 12.f, -30.f), T(rnd() * 16.f - 8.f, rnd() * 16.f - 8.f, 0.f);
        rays.push_back(tinybvh::Ray(O, T - O));
    }
    tinyhip::SphereBVH bvh;
    bool ok = true;
    for (int frame = 0; frame < 6; frame++) {
        const char* step = frame == 0 ? "build" : (frame < 5 ? "refit" : "rebuild");
        if (frame) for (uint32_t i = 0; i < n; i++) for (int k = 0; k < 3; k++) sph[4 * i + k] += vel[3 * i + k];
        if (frame == 0) bvh.BuildOnDevice(sph.data(), n);
        else if (frame < 5) bvh.Refit(sph.data(), n);
        else bvh.Rebuild(sph.data(), n);
        std::vector<tinybvh::Ray> r = rays;
        bvh.Intersect(r.data(), r.size());
        uint32_t hits = 0, wrong = 0;
        for (uint32_t i = 0; i < nRays; i++) {
            float t; uint32_t prim;
            brute(sph, rays[i], t, prim);
            const bool hit = r[i].hit.t < 1e30f;
            hits += hit;
            wrong += hit != (prim != 0xffffffffu) || (hit && (r[i].hit.t != t || r[i].hit.prim != prim));
        }
        float box[6];
        bvh.Bounds(box);
        std::printf("frame %d %-7s %u of %u rays hit, %u differ from brute force, bounds x %.3f .. %.3f\n", frame, step, hits, nRays, wrong, box[0], box[3]);
        ok = ok && wrong == 0 && hits > 0;
    }
    std::printf(ok ? "sphere particles ok\n" : "sphere particles FAILED\n");
    return ok ? 0 : 1;
}
