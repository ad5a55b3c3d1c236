// custom_sphere_dbl.h — custom-geometry sphere BLASes in double precision (BVH_Double::Build( customGetAABB, n ) traced through customIntersect /
// customIsOccluded, as tiny_bvh_custom_double.cpp and tiny_bvh_anim_double.cpp do): the record, the box and the primitive test, for the device
// (the sphere forms of kernels_double.hip, the box source of kernels_double_anim.hip) and for the host code of capi_double.hip.
//
// A sphere is the demos' struct Sphere { bvhdbl3 pos; double r; }, 32 bytes.  Gathered at upload (and by a device build) in primIdx order, one
// 48-byte record per index entry: {pos, r, prim, 0}, three aligned 16-byte reads.
//
// The primitive test restates the callback of tiny_bvh_anim_double.cpp, the form that stays right when |D| != 1 (a scaled instance; and the RayEx
// constructor is fed a float-normalised D in both demos, so |D| is 1 only to float precision even without a TLAS):
//   mag = sqrt(dot(D, D)), reciMag = 1 / mag;  oc = O - pos;  b = dot(oc, D) * reciMag;  c = dot(oc, oc) - r * r;  d = b * b - c
//   d <= 0 is a miss;  t = -b - sqrt(d);  a candidate iff t < tmax_in * mag && t > 0;  it records hit.t = t * reciMag
// Every operation is a separate IEEE double operation in the order written (dot: (x x + y y) + z z), sqrt and the division correctly rounded:
// the convention of the fp64 path (-ffp-contract=off, nothing fused).  The fp32 header custom_sphere.h differs here: it restates the fusions of the
// reference's x86 build.  tests/oracle_custom_double.c restates the same operations; the device matches it byte for byte.
//
// Winner rule (DESIGN.md par. 12, in double): a candidate is checked against the record's INCOMING hit.t; the ray keeps the candidate with the
// smallest recorded distance, then the smaller prim, then the smaller instance.  A hit writes t, prim and inst and leaves u, v as the record had them.
//
// DEVIATION from the reference, deliberate: BVH_Double::IsOccluded calls the customIsOccluded callback and throws its result away
// (tiny_bvh.h:8278-8279), so a custom BLAS can never occlude there; the fp32 path (:3424) returns it.  Here occlusion is 1 iff some sphere is a
// candidate, which is "the closest-hit query has a candidate".
#pragma once
#include <stdint.h>

#include "device_common.h"

namespace tbvh {

struct SphereDbl { double pos[3], r; };                                  // the caller's spheres32
static_assert(sizeof(SphereDbl) == 32, "a double sphere is 32 bytes");
struct SphereRecDbl { double pos[3], r; uint64_t prim, pad; };           // gathered: one per primIdx entry
static_assert(sizeof(SphereRecDbl) == 48, "a gathered double sphere is three 16-byte blocks");

// the demos' sphereAABB: pos - bvhdbl3( r ), pos + bvhdbl3( r ), one operation per component
__device__ __host__ __forceinline__ void sphere_box_dbl(const SphereDbl& s, double* mn, double* mx) {
    for (int a = 0; a < 3; a++) { mn[a] = s.pos[a] - s.r; mx[a] = s.pos[a] + s.r; }
}

// the per-ray (per-instance under a TLAS) factors of the callback: the same bits the reference recomputes for every sphere
struct SphereRayDbl {
    double reciMag;   // 1 / |D|
    double tmaxMag;   // tmax_in * |D|: a candidate lies below it
};
__device__ __host__ __forceinline__ SphereRayDbl sphere_ray_dbl(double Dx, double Dy, double Dz, double tmaxIn) {
    const double mag = __builtin_sqrt(Dx * Dx + Dy * Dy + Dz * Dz);
    SphereRayDbl r;
    r.reciMag = 1.0 / mag;
    r.tmaxMag = tmaxIn * mag;
    return r;
}

// true: the sphere {px, py, pz, r} is a candidate; stored = the distance it records (a ray parameter, t * reciMag)
__device__ __host__ __forceinline__ bool sphere_test_dbl(double Ox, double Oy, double Oz, double Dx, double Dy, double Dz, double px, double py, double pz, double r,
                                                         const SphereRayDbl& sr, double& stored) {
    const double ocx = Ox - px, ocy = Oy - py, ocz = Oz - pz;
    const double b = (ocx * Dx + ocy * Dy + ocz * Dz) * sr.reciMag;
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - r * r;
    const double d = b * b - c;
    if (d <= 0) return false;
    const double t = -b - __builtin_sqrt(d);
    if (!(t < sr.tmaxMag && t > 0)) return false;
    stored = t * sr.reciMag;
    return true;
}

// the winner rule for a sphere candidate: complete (the candidate's recorded distance may lie beyond the closest hit so far)
__device__ __host__ __forceinline__ bool sphere_wins_dbl(double t, uint64_t prim, uint64_t inst, bool found, double bestT, uint64_t bestPrim, uint64_t bestInst) {
    if (!found || t < bestT) return true;
    if (!(t == bestT)) return false;
    return prim < bestPrim || (prim == bestPrim && inst < bestInst);
}

}  // namespace tbvh
