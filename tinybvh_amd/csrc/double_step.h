// double_step.h — the fp64 pieces of the BVH_Double traversal (kernels_double.hip): the reference's min / max, its vector helpers and transforms,
// BVH_Double::BVHNode::Intersect, and the triangle test in the spelling the sphere TLAS forms use.  Everything is an expression of tiny_bvh.h
// restated operation for operation; the Makefile's -ffp-contract=off keeps each a separate IEEE operation.
#pragma once
#include "device_common.h"

namespace tbvh {

namespace {

constexpr double kDblFar = 1e300;              // BVH_DBL_FAR, tiny_bvh.h:145

struct D3 { double x, y, z; };

__device__ __forceinline__ double dmin(double a, double b) { return a < b ? a : b; }   // tinybvh_min (double), tiny_bvh.h:447
__device__ __forceinline__ double dmax(double a, double b) { return a > b ? a : b; }   // tinybvh_max (double), tiny_bvh.h:448
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// tinybvh_transform_point / tinybvh_transform_vector (tiny_bvh.h:576-590)
__device__ __forceinline__ D3 xform_point(D3 v, const double* T) {
    const D3 r{T[0] * v.x + T[1] * v.y + T[2] * v.z + T[3], T[4] * v.x + T[5] * v.y + T[6] * v.z + T[7], T[8] * v.x + T[9] * v.y + T[10] * v.z + T[11]};
    const double w = T[12] * v.x + T[13] * v.y + T[14] * v.z + T[15];
    if (w == 1) return r;
    const double rw = 1. / w;
    return D3{r.x * rw, r.y * rw, r.z * rw};
}
__device__ __forceinline__ D3 xform_vector(D3 v, const double* T) {
    return D3{T[0] * v.x + T[1] * v.y + T[2] * v.z, T[4] * v.x + T[5] * v.y + T[6] * v.z, T[8] * v.x + T[9] * v.y + T[10] * v.z};
}
__device__ __forceinline__ double guarded_rcp(double d) { return d > 1e-24 ? (1.0 / d) : (d < -1e-24 ? (1.0 / d) : kDblFar); }   // tiny_bvh.h:8336-8338

// BVH_Double::BVHNode::Intersect (tiny_bvh.h:8363-8375), culling against `bound` (the closest hit so far plus the slack)
__device__ __forceinline__ double node_dist(const double2* n, D3 O, D3 rD, double bound) {
    const double2 a = n[0], b = n[1], c = n[2];   // {mn.x, mn.y}, {mn.z, mx.x}, {mx.y, mx.z}
    const double tx1 = (a.x - O.x) * rD.x, tx2 = (b.y - O.x) * rD.x;
    double tmin = dmin(tx1, tx2), tmax = dmax(tx1, tx2);
    const double ty1 = (a.y - O.y) * rD.y, ty2 = (c.x - O.y) * rD.y;
    tmin = dmax(tmin, dmin(ty1, ty2));
    tmax = dmin(tmax, dmax(ty1, ty2));
    const double tz1 = (b.x - O.z) * rD.z, tz2 = (c.y - O.z) * rD.z;
    tmin = dmax(tmin, dmin(tz1, tz2));
    tmax = dmin(tmax, dmax(tz1, tz2));
    return (tmax >= tmin && tmin < bound && tmax >= 0) ? tmin : kDblFar;
}

// Moller-Trumbore as BVH_Double::Intersect writes it (tiny_bvh.h:8177-8194) over one gathered record {v0, e1, e2, prim}: true with t, u, v when the
// triangle's plane is met with u, v inside; the caller applies t > 0 and its winner rule
__device__ __forceinline__ bool tri_test_dbl(const double2* tr, D3 O, D3 D, double& t, double& u, double& v, uint64_t& prim) {
    const double2 t0 = tr[0], t1 = tr[1], t2 = tr[2], t3 = tr[3], t4 = tr[4];
    const D3 v0{t0.x, t0.y, t1.x}, e1{t1.y, t2.x, t2.y}, e2{t3.x, t3.y, t4.x};
    prim = (uint64_t)__double_as_longlong(t4.y);
    const D3 h = cross(D, e2);
    const double a = dot(e1, h);
    if (fabs(a) < 0.0000001) return false;
    const double f = 1 / a;
    const D3 s = sub(O, v0);
    u = f * dot(s, h);
    const D3 qv = cross(s, e1);
    v = f * dot(D, qv);
    if (u < 0 || v < 0 || u + v > 1) return false;
    t = f * dot(e2, qv);
    return true;
}

}  // namespace

}  // namespace tbvh
