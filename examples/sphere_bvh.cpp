// sphere_bvh.cpp — tinyhip::SphereBVH from C++: a BVH over spheres built by the library (Build) and uploaded from a tree made by hand (Upload),
// traced with Intersect / IsOccluded over tinybvh::Ray records.  Three unit spheres on the z axis at z = 5, 10, 15 and one off the axis; rays from
// x = 0, 0.5, 3 along +z.  Prints, per ray, the hit of both scenes, then the occlusion answer and whether Handle() is a sphere BLAS
// (tests/test_custom_gpu.py: test_tiny_hip_sphere_binding_runs checks the lines).  Built by __graft_entry__.build() where tiny_bvh.h is found.
#include "tiny_bvh.h"
#include "tiny_hip.h"
#include <cstdio>
int main() {
    const float sph[16] = {0, 0, 15, 1, 0, 0, 5, 1, 0, 0, 10, 1, 3, 0, 30, 0.5f};
    tinyhip::SphereBVH a, b;
    a.Build(sph, 4);
    struct Node { tinybvh::bvhvec3 mn; uint32_t leftFirst; tinybvh::bvhvec3 mx; uint32_t triCount; };   // BVH::BVHNode's layout
    const Node root = {tinybvh::bvhvec3(-1, -1, 4), 0, tinybvh::bvhvec3(3.5f, 1, 30.5f), 4};              // the Upload path: one leaf of all four
    const uint32_t idx[4] = {3, 2, 1, 0};
    b.Upload(&root, 1, idx, 4, sph, 4);
    tinybvh::Ray r[3] = {tinybvh::Ray(tinybvh::bvhvec3(0, 0, 0), tinybvh::bvhvec3(0, 0, 1)), tinybvh::Ray(tinybvh::bvhvec3(0.5f, 0, 0), tinybvh::bvhvec3(0, 0, 1)),
                         tinybvh::Ray(tinybvh::bvhvec3(3, 0, 0), tinybvh::bvhvec3(0, 0, 1))};
    tinybvh::Ray q[3] = {r[0], r[1], r[2]};
    a.Intersect(r, 3); b.Intersect(q, 3);
    uint8_t occ[3];
    r[0].hit.t = 1e30f; a.IsOccluded(r, 1, occ);
    for (int i = 0; i < 3; i++) std::printf("%u %.6f %u %.6f\n", r[i].hit.prim, i ? r[i].hit.t : 0.f, q[i].hit.prim, q[i].hit.t);
    std::printf("occ %u handle %d\n", occ[0], a.Handle() && tbvh_scene_layout(a.Handle()) == TBVH_LAYOUT_BVH2_WALD);
    return 0;
}
