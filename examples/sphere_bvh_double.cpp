// sphere_bvh_double.cpp — the frame of the reference's tiny_bvh_custom_double.cpp on the engine: one sphere per triangle of a mesh, a BVH_Double
// built over the spheres' boxes with Build( &sphereAABB, n ), a pinhole camera whose rays are RayEx( eye, float-normalised D ), and the demo's
// shading (|N . L| as a grey level over a light-blue clear colour).  The tree tinybvh built is uploaded as it is (tinyhip::SphereBVH_Double), the
// frame's rays are traced in one batch on the device, and the same rays are traced on the host by BVH_Double::Intersect through sphere callbacks
// written here from the arithmetic the device runs (tinybvh_amd.h, "double precision, custom geometry"): every pixel must agree.  The mesh is
// procedural (a ridged terrain), so the program needs no data file.  Prints "<n> differing pixels" (tests/test_custom_double_gpu.py checks for 0).
// Built by __graft_entry__.build() where tiny_bvh.h is found, without contraction: the callbacks round once per operation, as the device does.
#define TINYBVH_IMPLEMENTATION
#include "tiny_bvh.h"
#include "tiny_hip.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace tinybvh;

struct Sphere { bvhdbl3 pos; double r; };
static std::vector<Sphere> spheres;

// ray / sphere, the form that stays right when |D| != 1 (the constructor normalises a float-normalised D again, in double)
static bool sphereIntersect(RayEx& ray, const uint64_t prim) {
    const Sphere& s = spheres[prim];
    const double mag = sqrt(ray.D.x * ray.D.x + ray.D.y * ray.D.y + ray.D.z * ray.D.z), reciMag = 1.0 / mag;
    const double ocx = ray.O.x - s.pos.x, ocy = ray.O.y - s.pos.y, ocz = ray.O.z - s.pos.z;
    const double b = (ocx * ray.D.x + ocy * ray.D.y + ocz * ray.D.z) * reciMag;
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - s.r * s.r;
    const double d = b * b - c;
    if (d <= 0) return false;
    const double t = -b - sqrt(d);
    if (!(t < ray.hit.t * mag && t > 0)) return false;
    ray.hit.t = t * reciMag; ray.hit.prim = prim;
    return true;
}
static bool sphereIsOccluded(const RayEx& ray, const uint64_t prim) {
    RayEx r = ray;
    return sphereIntersect(r, prim);
}
static void sphereAABB(const uint64_t prim, bvhdbl3& mn, bvhdbl3& mx) {
    const Sphere& s = spheres[prim];
    mn = bvhdbl3(s.pos.x - s.r, s.pos.y - s.r, s.pos.z - s.r);
    mx = bvhdbl3(s.pos.x + s.r, s.pos.y + s.r, s.pos.z + s.r);
}

static uint32_t shade(const RayEx& ray) {
    if (!(ray.hit.t < 10000)) return 0xaaaaff;
    const double L[3] = {1 / sqrt(14.0), 2 / sqrt(14.0), 3 / sqrt(14.0)};
    const Sphere& s = spheres[ray.hit.prim];
    const double n[3] = {ray.O.x + ray.hit.t * ray.D.x - s.pos.x, ray.O.y + ray.hit.t * ray.D.y - s.pos.y, ray.O.z + ray.hit.t * ray.D.z - s.pos.z};
    const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const int c = (int)(255.9 * fabs((n[0] * L[0] + n[1] * L[1] + n[2] * L[2]) / len));
    return (uint32_t)(c + (c << 8) + (c << 16));
}

int main() {
    // a ridged terrain of G x G quads, two triangles each; one sphere per triangle as the demo makes them
    const int G = 64, W = 320, H = 200;
    auto height = [](double x, double z) { return 1.5 * sin(0.35 * x) * cos(0.27 * z) + 0.4 * sin(1.3 * x + 0.7 * z); };
    for (int iz = 0; iz < G; iz++) for (int ix = 0; ix < G; ix++) {
        const double x0 = 0.5 * (ix - G / 2), z0 = 0.5 * (iz - G / 2), x1 = x0 + 0.5, z1 = z0 + 0.5;
        const bvhdbl3 q[4] = {bvhdbl3(x0, height(x0, z0), z0), bvhdbl3(x1, height(x1, z0), z0), bvhdbl3(x0, height(x0, z1), z1), bvhdbl3(x1, height(x1, z1), z1)};
        const int tri[2][3] = {{0, 1, 2}, {1, 3, 2}};
        for (auto& t : tri) {
            const bvhdbl3 v0 = q[t[0]], v1 = q[t[1]], v2 = q[t[2]];
            Sphere s;
            s.r = tinybvh_min(0.35, 0.25 * tinybvh_min(tinybvh_length(v1 - v0), tinybvh_length(v2 - v0)));
            s.pos = (v0 + v1 + v2) * 0.33333;
            spheres.push_back(s);
        }
    }
    BVH_Double bvh;
    bvh.Build(&sphereAABB, spheres.size());
    bvh.customIntersect = &sphereIntersect;
    bvh.customIsOccluded = &sphereIsOccluded;
    tinyhip::SphereBVH_Double scene(bvh, spheres.data(), spheres.size());

    // the demo's view pyramid, in float
    const bvhvec3 eye(-14.f, 9.f, -12.f), view = tinybvh_normalize(bvhvec3(0.66f, -0.45f, 0.6f));
    const bvhvec3 right = tinybvh_normalize(tinybvh_cross(bvhvec3(0, 1, 0), view)), up = 0.8f * tinybvh_cross(view, right);
    const bvhvec3 C = eye + 2 * view, p1 = C - right + up, p2 = C + right + up, p3 = C - right - up;
    std::vector<RayEx> rays;
    for (int y = 0; y < H; y++) for (int x = 0; x < W; x++) {
        const float u = (float)x / W, v = (float)y / H;
        const bvhvec3 D = tinybvh_normalize(p1 + u * (p2 - p1) + v * (p3 - p1) - eye);
        rays.push_back(RayEx(eye, D, 1e30f));
    }
    std::vector<RayEx> host = rays;
    scene.Intersect(rays.data(), rays.size());
    for (RayEx& r : host) bvh.Intersect(r);
    std::vector<uint8_t> occ(rays.size());
    scene.IsOccluded(host.data(), host.size(), occ.data());   // (over the traced records: tmax = the hit distance)

    size_t hits = 0, differing = 0, records = 0, occluded = 0;
    for (size_t i = 0; i < rays.size(); i++) {
        hits += rays[i].hit.t < 10000;
        differing += shade(rays[i]) != shade(host[i]);
        records += memcmp(&rays[i].hit, &host[i].hit, sizeof(rays[i].hit)) != 0;
        occluded += occ[i];
    }
    std::printf("%zu spheres, %d x %d pixels, %zu hit a sphere (device %.3f ms)\n", spheres.size(), W, H, hits, scene.LastKernelMs());
    std::printf("%zu differing pixels, %zu differing hit records, %zu of the traced rays occluded before their hit\n", differing, records, occluded);
    return differing || records ? 1 : 0;
}
