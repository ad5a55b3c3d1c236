// pose.h — the arithmetic of the reference's Mesh::SetPose( const Skin* ) and Mesh::SetPose( const vector<float>& ) (tiny_scene.h:1785-1825, 1751-1778),
// float operation for float operation as the reference's build performs them (DESIGN.md par. 14).  One copy for the kernels
// (kernels_pose.hip), the library's host path (pose_host.cpp) and, through that, the tests.  Everything that includes this is built
// -ffp-contract=off: the three fused multiply-adds below are the only ones.
//
//   skin    S = w.x * M[j.x]; S += w.y * M[j.y]; S += w.z * M[j.z]; S += w.w * M[j.w]     every product rounded, then every sum (operator*( float, bvhmat4 )
//                                                                                        is an out-of-line call: nothing fuses across it)
//           row_r = fma( S[4r+2], z, fma( S[4r], x, S[4r+1] * y ) ) + S[4r+3]             ts_transform_point's rows as g++ -O3 -mfma contracts them
//           row_3 == 1 ? (row_0, row_1, row_2) : (row_0, row_1, row_2) * (1.0f / row_3)   the reciprocal is rounded, then multiplied; output w = 0
//   morph   v = positions[0][i]; v = fma( weight[j-1], positions[j][i], v ), j = 1 .. T   output w = 1
// and the FatTri half of both (tiny_scene.h:1761-1777, 1809-1824; DESIGN.md par. 16), read from the same object code:
//   normalize      l2 = fma( z, z, fma( x, x, y * y ) ), l = sqrtf( l2 ), a * ( l == 0 ? 0 : 1 / l )
//   skin normal    normalize( row_r = fma( S[4r+2], nz, fma( S[4r], nx, S[4r+1] * ny ) ), r = 0 .. 2 ) with the vertex's own blended S
//   skin N         a = v1 - v0, b = v2 - v0; normalize( fma( a.y, b.z, -( a.z * b.y ) ), fma( a.z, b.x, -( a.x * b.z ) ), fma( a.x, b.y, -( a.y * b.x ) ) )
//   morph normal   normalize( normals[0][i] + normals[1][i] + ... + normals[T][i] ): plain sums in order, and NO weights — the reference's arithmetic
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TBVH_POSE_HD __host__ __device__ __forceinline__
#else
#define TBVH_POSE_HD inline
#endif

namespace tbvh {

TBVH_POSE_HD float pose_fma(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return __builtin_fmaf(a, b, c);
#endif
}

// one cell of the blended matrix: a, b, c, d = that cell of M[j.x], M[j.y], M[j.z], M[j.w]
TBVH_POSE_HD float pose_blend(float a, float b, float c, float d, float wx, float wy, float wz, float ww) {
    float s = a * wx;
    s = s + b * wy;
    s = s + c * wz;
    s = s + d * ww;
    return s;
}

// one row of blended matrix times (x, y, z, 1); V4: anything with float members x, y, z, w holding row r of the four joint matrices
template <class V4>
TBVH_POSE_HD float pose_skin_row(const V4& a, const V4& b, const V4& c, const V4& d, float wx, float wy, float wz, float ww, float x, float y, float z) {
    const float s0 = pose_blend(a.x, b.x, c.x, d.x, wx, wy, wz, ww);
    const float s1 = pose_blend(a.y, b.y, c.y, d.y, wx, wy, wz, ww);
    const float s2 = pose_blend(a.z, b.z, c.z, d.z, wx, wy, wz, ww);
    const float s3 = pose_blend(a.w, b.w, c.w, d.w, wx, wy, wz, ww);
    return pose_fma(s2, z, pose_fma(s0, x, s1 * y)) + s3;
}

// the homogeneous divide of ts_transform_point: taken whenever row_3 is not exactly 1, which weights normalised in fp32 make common
TBVH_POSE_HD void pose_skin_finish(float r0, float r1, float r2, float r3, float out[4]) {
    if (r3 == 1) { out[0] = r0; out[1] = r1; out[2] = r2; }
    else { const float inv = 1.0f / r3; out[0] = r0 * inv; out[1] = r1 * inv; out[2] = r2 * inv; }
    out[3] = 0.f;
}

// the same row and, from the same blended cells, the row of blended matrix times the normal (nx, ny, nz, 0)
template <class V4>
TBVH_POSE_HD float pose_skin_row_n(const V4& a, const V4& b, const V4& c, const V4& d, float wx, float wy, float wz, float ww, float x, float y, float z, float nx, float ny,
                                   float nz, float& nrow) {
    const float s0 = pose_blend(a.x, b.x, c.x, d.x, wx, wy, wz, ww);
    const float s1 = pose_blend(a.y, b.y, c.y, d.y, wx, wy, wz, ww);
    const float s2 = pose_blend(a.z, b.z, c.z, d.z, wx, wy, wz, ww);
    const float s3 = pose_blend(a.w, b.w, c.w, d.w, wx, wy, wz, ww);
    nrow = pose_fma(s2, nz, pose_fma(s0, nx, s1 * ny));
    return pose_fma(s2, z, pose_fma(s0, x, s1 * y)) + s3;
}

// ts_normalize: correctly rounded square root and division on both sides (the builtins; not HIP's __fsqrt_rn, which is the native approximation)
TBVH_POSE_HD void pose_normalize(float v[3]) {
    const float l = __builtin_sqrtf(pose_fma(v[2], v[2], pose_fma(v[0], v[0], v[1] * v[1])));
    const float rl = l == 0 ? 0.f : 1.0f / l;
    v[0] = v[0] * rl; v[1] = v[1] * rl; v[2] = v[2] * rl;
}

// normalize( cross( v1 - v0, v2 - v0 ) )
TBVH_POSE_HD void pose_geometric_normal(const float* v0, const float* v1, const float* v2, float N[3]) {
    const float ax = v1[0] - v0[0], ay = v1[1] - v0[1], az = v1[2] - v0[2];
    const float bx = v2[0] - v0[0], by = v2[1] - v0[1], bz = v2[2] - v0[2];
    N[0] = pose_fma(ay, bz, -(az * by));
    N[1] = pose_fma(az, bx, -(ax * bz));
    N[2] = pose_fma(ax, by, -(ay * bx));
    pose_normalize(N);
}

// One FatTri of a posed mesh, as 48 floats: vertex0..2 (floats 20, 24, 28) and vN0..2 (floats 8, 12, 16) are rewritten, three floats each; a skin
// pose also rewrites Nx Ny Nz (floats 11, 15, 19) from the posed corners, a morph pose leaves them.  Every other float keeps its bytes.
TBVH_POSE_HD void pose_fat_tri(float* tri, const float* v0, const float* v1, const float* v2, const float* n0, const float* n1, const float* n2, bool skin) {
    const float* v[3] = {v0, v1, v2};
    const float* n[3] = {n0, n1, n2};
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 3; c++) { tri[20 + 4 * k + c] = v[k][c]; tri[8 + 4 * k + c] = n[k][c]; }
    if (skin) {
        float N[3];
        pose_geometric_normal(v0, v1, v2, N);
        tri[11] = N[0]; tri[15] = N[1]; tri[19] = N[2];
    }
}

struct PoseRow { float x, y, z, w; };
TBVH_POSE_HD PoseRow pose_row(const float* m) { PoseRow r = {m[0], m[1], m[2], m[3]}; return r; }

// one vertex from plain arrays: rest (x, y, z), 4 joint indices (all < the table's size: the caller has checked), 4 weights, the joint table
TBVH_POSE_HD void pose_skin_vertex(const float* rest, const uint32_t* j, const float* w, const float* mats16, float out[4]) {
    const float* m0 = mats16 + 16 * (uint64_t)j[0];
    const float* m1 = mats16 + 16 * (uint64_t)j[1];
    const float* m2 = mats16 + 16 * (uint64_t)j[2];
    const float* m3 = mats16 + 16 * (uint64_t)j[3];
    float r[4];
    for (int k = 0; k < 4; k++)
        r[k] = pose_skin_row(pose_row(m0 + 4 * k), pose_row(m1 + 4 * k), pose_row(m2 + 4 * k), pose_row(m3 + 4 * k), w[0], w[1], w[2], w[3], rest[0], rest[1], rest[2]);
    pose_skin_finish(r[0], r[1], r[2], r[3], out);
}

// one vertex of a morph pose: positions12 = (nTargets + 1) arrays of nVerts * 3 floats, array 0 the base
TBVH_POSE_HD void pose_morph_vertex(const float* positions12, uint64_t nVerts, uint32_t nTargets, const float* weights, uint64_t i, float out[4]) {
    const float* p = positions12 + 3 * i;
    float x = p[0], y = p[1], z = p[2];
    for (uint32_t t = 1; t <= nTargets; t++) {
        p += 3 * nVerts;
        const float wt = weights[t - 1];
        x = pose_fma(wt, p[0], x); y = pose_fma(wt, p[1], y); z = pose_fma(wt, p[2], z);
    }
    out[0] = x; out[1] = y; out[2] = z; out[3] = 1.f;
}

// the posed normal of one skinned vertex: normal12 = its rest normal (x, y, z)
TBVH_POSE_HD void pose_skin_normal(const float* normal12, const uint32_t* j, const float* w, const float* mats16, float out[4]) {
    const float* m0 = mats16 + 16 * (uint64_t)j[0];
    const float* m1 = mats16 + 16 * (uint64_t)j[1];
    const float* m2 = mats16 + 16 * (uint64_t)j[2];
    const float* m3 = mats16 + 16 * (uint64_t)j[3];
    for (int k = 0; k < 3; k++)
        (void)pose_skin_row_n(pose_row(m0 + 4 * k), pose_row(m1 + 4 * k), pose_row(m2 + 4 * k), pose_row(m3 + 4 * k), w[0], w[1], w[2], w[3], 0.f, 0.f, 0.f, normal12[0],
                              normal12[1], normal12[2], out[k]);
    pose_normalize(out);
    out[3] = 0.f;
}

// the normal of one vertex of a morph pose: normals12 = (nTargets + 1) arrays of nVerts * 3 floats; the sum takes no weights
TBVH_POSE_HD void pose_morph_normal(const float* normals12, uint64_t nVerts, uint32_t nTargets, uint64_t i, float out[4]) {
    const float* p = normals12 + 3 * i;
    float x = p[0], y = p[1], z = p[2];
    for (uint32_t t = 1; t <= nTargets; t++) {
        p += 3 * nVerts;
        x = x + p[0]; y = y + p[1]; z = z + p[2];
    }
    out[0] = x; out[1] = y; out[2] = z; out[3] = 0.f;
    pose_normalize(out);
}

// (pose_host.cpp) whole arrays on the CPU, under tbvh_host_pose_skin / tbvh_host_pose_morph, which are defined there as well
uint64_t pose_first_bad_joint(const uint32_t* joints4, uint64_t nVerts, uint32_t nJoints);   // the first vertex with an index >= nJoints, or nVerts
void pose_skin_host(const float* rest16, uint64_t nVerts, const uint32_t* joints4, const float* weights16, const float* mats16, float* out16);
void pose_morph_host(const float* positions12, uint64_t nVerts, uint32_t nTargets, const float* weights, float* out16);
uint64_t pose_first_bad_corner(const uint32_t* indices, uint64_t nTris, uint64_t nVerts);   // the first triangle with an index >= nVerts, or nTris

}  // namespace tbvh
