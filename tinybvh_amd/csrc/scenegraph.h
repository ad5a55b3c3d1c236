// scenegraph.h — the arithmetic and the state machine of the reference's Scene::UpdateSceneGraph (tiny_scene.h: Animation::Channel::Update, the three
// Sampler::Sample*, ts_quat::slerp, Node::UpdateTransformFromTRS, Node::Update's matrix products, ts_invert), float operation for float operation as the
// reference's build (g++ -O3 -mavx2 -mfma, tinyscene's vector types = tinybvh's) performs them (DESIGN.md par. 17).  One copy for the kernels
// (kernels_scenegraph.hip) and the library's host twin (scenegraph_host.cpp).  Everything that includes this is built -ffp-contract=off: the fused
// multiply-adds written out below are the only ones.  There is NO single contraction rule: which product of a sum stays rounded was read from that build's
// object code function by function (DESIGN.md par. 17 has the table) and differs between them — bvhmat4 operator* and the dot products fuse the FIRST product onto
// the rounded second, ts_invert's cofactors and the vec3 / quaternion spline sums round the first and fuse the second, SampleVec3's and slerp's lerp fuse f * b
// onto the rounded (1 - f) * a while SampleFloat's lerp and spline do the opposite.  Do not normalise these: every one is pinned bytewise against the real
// reference (tests/test_scenegraph_host.py).  Divide and square root are the correctly rounded ones on both sides; acosf / sinf (slerp's branch for
// cosTheta <= 0.99) are the host's and the device's own math libraries, the one place where the two sides may differ.
//
// A graph is held as flat arrays behind one SgView (host vectors or device buffers, the same struct).  Work items: one channel (sg_channel), one node
// (sg_node_local, sg_node_combine), one instance (sg_instance), one (skin use, joint) pair (sg_joint_pair).  No item reads what another item of the same
// step writes, so the host loops over them in any order and the device gives each a lane.  Every index that comes from an array (sampler, node, k, key
// and value positions, ancestors) is compared with its bound before an address is formed; a violation leaves the item's output unwritten and raises
// kStatusGraph in the status word.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TBVH_SG_HD __host__ __device__ __forceinline__
#else
#define TBVH_SG_HD inline
#endif

namespace tbvh {

constexpr uint32_t kStatusGraph = 512u;   // status word: a scene graph index (sampler, node, key state, key position) was out of range on the device

enum { kSgLinear = 0, kSgSpline = 1, kSgStep = 2 };   // Sampler::interpolation as the reference numbers it
enum { kSgVec3 = 0, kSgQuat = 1, kSgFloat = 2 };      // which of a sampler's three key vectors it fills
enum { kSgShadowAll = 1u, kSgShadowAnim = 2u };       // channel flags: a later channel (of any animation / of the same one) writes the same field
constexpr uint32_t kSgWrapLimit = 1u << 16;           // a time is refused when Channel::Update's wrap loop would take more turns than this

struct SgView {
    uint32_t nNodes, nSamplers, nChannels, nInstances, nPairs, nTimes, nValues, nWeights, nAnc;
    const uint32_t *sInterp, *sType, *sKeyOff, *sValOff;   // samplers: sKeyOff / sValOff have nSamplers + 1 entries into times / values
    const float *times, *values;
    const uint32_t *cSampler, *cNode, *cTarget, *cFlags;   // channels, in (animation, channel) order
    float* cT;                                             // Channel::t
    int32_t* cK;                                           // Channel::k
    uint32_t* cTrig;                                       // 1: the channel's last sample took slerp's trigonometric branch (the one inexact path)
    const uint32_t* wOff;                                  // nodes: nNodes + 1 entries into weights
    float *trs, *weights;                                  // 10 floats per node: translation, rotation (w x y z), scale
    uint32_t* written;                                     // Node::transformed
    const float* matrix;
    float *local, *combined;                               // 16 floats per node; combined: this frame's
    const float* combinedPrev;                             // last frame's (identity before the first)
    const uint32_t *ancOff, *anc;                          // per node its ancestors root first, itself last
    const uint32_t* instNode;
    float* instOut;
    const uint32_t *pairMesh, *pairJoint, *pairStale;      // per (skin use, joint): the mesh node, the joint node, 1 = the joint is visited after the mesh node
    const float* invBind;
    float* jointOut;
    uint32_t* status;
};

TBVH_SG_HD float sg_fma(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return __builtin_fmaf(a, b, c);
#endif
}

TBVH_SG_HD void sg_raise(uint32_t* status) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(status, kStatusGraph);
#else
    *status |= kStatusGraph;
#endif
}

// a0*b0 + a1*b1 + a2*b2 + a3*b3 as that build contracts it
TBVH_SG_HD float sg_dot4(float a0, float b0, float a1, float b1, float a2, float b2, float a3, float b3) {
    return sg_fma(a3, b3, sg_fma(a2, b2, sg_fma(a0, b0, a1 * b1)));
}

// bvhmat4 operator*( a, b ), row-major; r may not alias a or b
TBVH_SG_HD void sg_mul(const float* a, const float* b, float* r) {
    for (int i = 0; i < 16; i += 4)
        for (int j = 0; j < 4; j++) r[i + j] = sg_dot4(a[i], b[j], a[i + 1], b[j + 4], a[i + 2], b[j + 8], a[i + 3], b[j + 12]);
}

TBVH_SG_HD void sg_identity(float* m) {
    for (int i = 0; i < 16; i++) m[i] = (i % 5) == 0 ? 1.f : 0.f;
}

// one cell of ts_invert's cofactor table: s0*a0*b0*c0 + s1*a1*b1*c1 + ... (six terms, each (a*b)*c, signs +-1)
TBVH_SG_HD float sg_cof(const float* T, int s0, int a0, int b0, int c0, int s1, int a1, int b1, int c1, int s2, int a2, int b2, int c2, int s3, int a3, int b3, int c3, int s4,
                        int a4, int b4, int c4, int s5, int a5, int b5, int c5) {
    // a leading minus belongs to the first factor ( -T[a] * T[b] * T[c] ); a subtracted term negates the product (exact either way)
    const float p0 = (s0 < 0 ? -T[a0] : T[a0]) * T[b0];
    const float p1 = T[a1] * T[b1], p2 = T[a2] * T[b2], p3 = T[a3] * T[b3], p4 = T[a4] * T[b4], p5 = T[a5] * T[b5];
    const float m0 = p0 * T[c0];   // (in this function that build rounds the FIRST term and fuses the second onto it)
    float r = sg_fma(s1 < 0 ? -p1 : p1, T[c1], m0);
    r = sg_fma(s2 < 0 ? -p2 : p2, T[c2], r);
    r = sg_fma(s3 < 0 ? -p3 : p3, T[c3], r);
    r = sg_fma(s4 < 0 ? -p4 : p4, T[c4], r);
    r = sg_fma(s5 < 0 ? -p5 : p5, T[c5], r);
    return r;
}

// ts_invert( T ) into r (r = T when the determinant is 0, as the reference leaves it)
TBVH_SG_HD void sg_invert(const float* T, float* r) {
    float inv[16];
    inv[0] = sg_cof(T, 1, 5, 10, 15, -1, 5, 11, 14, -1, 9, 6, 15, 1, 9, 7, 14, 1, 13, 6, 11, -1, 13, 7, 10);
    inv[1] = sg_cof(T, -1, 1, 10, 15, 1, 1, 11, 14, 1, 9, 2, 15, -1, 9, 3, 14, -1, 13, 2, 11, 1, 13, 3, 10);
    inv[2] = sg_cof(T, 1, 1, 6, 15, -1, 1, 7, 14, -1, 5, 2, 15, 1, 5, 3, 14, 1, 13, 2, 7, -1, 13, 3, 6);
    inv[3] = sg_cof(T, -1, 1, 6, 11, 1, 1, 7, 10, 1, 5, 2, 11, -1, 5, 3, 10, -1, 9, 2, 7, 1, 9, 3, 6);
    inv[4] = sg_cof(T, -1, 4, 10, 15, 1, 4, 11, 14, 1, 8, 6, 15, -1, 8, 7, 14, -1, 12, 6, 11, 1, 12, 7, 10);
    inv[5] = sg_cof(T, 1, 0, 10, 15, -1, 0, 11, 14, -1, 8, 2, 15, 1, 8, 3, 14, 1, 12, 2, 11, -1, 12, 3, 10);
    inv[6] = sg_cof(T, -1, 0, 6, 15, 1, 0, 7, 14, 1, 4, 2, 15, -1, 4, 3, 14, -1, 12, 2, 7, 1, 12, 3, 6);
    inv[7] = sg_cof(T, 1, 0, 6, 11, -1, 0, 7, 10, -1, 4, 2, 11, 1, 4, 3, 10, 1, 8, 2, 7, -1, 8, 3, 6);
    inv[8] = sg_cof(T, 1, 4, 9, 15, -1, 4, 11, 13, -1, 8, 5, 15, 1, 8, 7, 13, 1, 12, 5, 11, -1, 12, 7, 9);
    inv[9] = sg_cof(T, -1, 0, 9, 15, 1, 0, 11, 13, 1, 8, 1, 15, -1, 8, 3, 13, -1, 12, 1, 11, 1, 12, 3, 9);
    inv[10] = sg_cof(T, 1, 0, 5, 15, -1, 0, 7, 13, -1, 4, 1, 15, 1, 4, 3, 13, 1, 12, 1, 7, -1, 12, 3, 5);
    inv[11] = sg_cof(T, -1, 0, 5, 11, 1, 0, 7, 9, 1, 4, 1, 11, -1, 4, 3, 9, -1, 8, 1, 7, 1, 8, 3, 5);
    inv[12] = sg_cof(T, -1, 4, 9, 14, 1, 4, 10, 13, 1, 8, 5, 14, -1, 8, 6, 13, -1, 12, 5, 10, 1, 12, 6, 9);
    inv[13] = sg_cof(T, 1, 0, 9, 14, -1, 0, 10, 13, -1, 8, 1, 14, 1, 8, 2, 13, 1, 12, 1, 10, -1, 12, 2, 9);
    inv[14] = sg_cof(T, -1, 0, 5, 14, 1, 0, 6, 13, 1, 4, 1, 14, -1, 4, 2, 13, -1, 12, 1, 6, 1, 12, 2, 5);
    inv[15] = sg_cof(T, 1, 0, 5, 10, -1, 0, 6, 9, -1, 4, 1, 10, 1, 4, 2, 9, 1, 8, 1, 6, -1, 8, 2, 5);
    const float det = sg_dot4(T[0], inv[0], T[1], inv[4], T[2], inv[8], T[3], inv[12]);
    if (det == 0) { for (int i = 0; i < 16; i++) r[i] = T[i]; return; }
    const float invdet = 1.0f / det;
    for (int i = 0; i < 16; i++) r[i] = inv[i] * invdet;
}

// Node::UpdateTransformFromTRS: localTransform = T * R * S * matrix; trs = translation (3), rotation (w x y z), scale (3)
TBVH_SG_HD void sg_local_from_trs(const float* trs, const float* matrix, float* local) {
    float T[16], R[16], S[16], a[16], b[16];
    sg_identity(T); sg_identity(R); sg_identity(S);
    T[3] = trs[0]; T[7] = trs[1]; T[11] = trs[2];
    const float rw = trs[3], rx = trs[4], ry = trs[5], rz = trs[6];
    const float x2 = 2 * rx, y2 = 2 * ry, z2 = 2 * rz, w2 = 2 * rw;
    R[0] = sg_fma(-z2, rz, sg_fma(-y2, ry, 1.f)); R[1] = sg_fma(x2, ry, -(w2 * rz));
    R[2] = sg_fma(x2, rz, w2 * ry); R[4] = sg_fma(x2, ry, w2 * rz);
    R[5] = sg_fma(-z2, rz, sg_fma(-x2, rx, 1.f)); R[6] = sg_fma(y2, rz, -(w2 * rx));
    R[8] = sg_fma(x2, rz, -(w2 * ry)); R[9] = sg_fma(y2, rz, w2 * rx);
    R[10] = sg_fma(-y2, ry, sg_fma(-x2, rx, 1.f));
    S[0] = trs[7]; S[5] = trs[8]; S[10] = trs[9];
    sg_mul(T, R, a); sg_mul(a, S, b); sg_mul(b, matrix, local);
}

// ts_quat::ts_normalize: scale by the rounded 1 / magnitude; q = w x y z
TBVH_SG_HD void sg_quat_normalize(float* q) {
    const float m = __builtin_sqrtf(sg_dot4(q[0], q[0], q[1], q[1], q[2], q[2], q[3], q[3]));
    const float s = 1 / m;
    q[0] = q[0] * s; q[1] = q[1] * s; q[2] = q[2] * s; q[3] = q[3] * s;
}

TBVH_SG_HD float sg_acosf(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return acosf(x);
#else
    return __builtin_acosf(x);
#endif
}
TBVH_SG_HD float sg_sinf(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return sinf(x);
#else
    return __builtin_sinf(x);
#endif
}

// ts_quat::slerp( a, b, t ) (not normalised); returns 1 when the trigonometric branch was taken
TBVH_SG_HD int sg_slerp(const float* a, const float* b, float t, float* r) {
    r[0] = b[0]; r[1] = b[1]; r[2] = b[2]; r[3] = b[3];
    float cosTheta = sg_dot4(a[0], r[0], a[1], r[1], a[2], r[2], a[3], r[3]);
    if (cosTheta < 0) { r[0] = r[0] * -1.0f; r[1] = r[1] * -1.0f; r[2] = r[2] * -1.0f; r[3] = r[3] * -1.0f; cosTheta = -cosTheta; }
    if (cosTheta > 0.99f) {
        const float u = 1 - t;
        for (int i = 0; i < 4; i++) r[i] = sg_fma(t, r[i], u * a[i]);
        return 0;
    }
    const float angle = sg_acosf(cosTheta);
    const float s1 = sg_sinf((1 - t) * angle), s2 = sg_sinf(t * angle), rs3 = 1.0f / sg_sinf(angle);
    for (int i = 0; i < 4; i++) r[i] = sg_fma(s1, a[i], s2 * r[i]) * rs3;
    return 1;
}

// the four weights of the samplers' cubic spline at tt: m0 * c[0] + p0 * c[1] + p1 * c[2] + m1 * c[3]
TBVH_SG_HD void sg_spline_coeffs(float tt, float* c) {
    const float t2 = tt * tt, t3 = t2 * tt;
    c[0] = sg_fma(-2.f, t2, t3) + tt;
    c[1] = sg_fma(2.f, t3, -(3 * t2)) + 1;
    c[2] = sg_fma(-2.f, t3, 3 * t2);
    c[3] = t3 - t2;
}
// SampleVec3 / SampleQuat round the first product and fuse the second onto it, SampleFloat the other way round (read from that build's object code)
TBVH_SG_HD float sg_spline(float m0, float p0, float p1, float m1, const float* c) {
    return sg_fma(m1, c[3], sg_fma(p1, c[2], sg_fma(p0, c[1], m0 * c[0])));
}
TBVH_SG_HD float sg_spline_float(float m0, float p0, float p1, float m1, const float* c) {
    return sg_fma(m1, c[3], sg_fma(p1, c[2], sg_fma(m0, c[0], p0 * c[1])));
}

// Sampler::SampleVec3 / SampleQuat over one sampler's keys: W floats per key (3 or 4), val = its values (nVal floats), tm = its key times.
// Returns 0, or 1 when a position it needs lies outside the arrays (out is then not written).  trig: set when slerp took the trigonometric branch.
TBVH_SG_HD int sg_sample_vec(int W, uint32_t interp, const float* tm, uint32_t keyCount, const float* val, uint32_t nVal, float t, int32_t k, float* out, int* trig) {
    const uint32_t nEl = nVal / (uint32_t)W;
    if (k < 0 || (uint32_t)k + 1 >= keyCount) return 1;
    uint32_t e = 0xffffffffu;                         // the single element returned as it is, if any
    if (k == 0 && t < tm[0]) e = interp == kSgSpline ? 1u : 0u;
    const float t0 = tm[k], t1 = tm[k + 1];
    const float f = (t - t0) / (t1 - t0);
    if (e == 0xffffffffu && f <= 0) e = 0;
    if (e == 0xffffffffu && interp == kSgStep) e = (uint32_t)k;
    if (e != 0xffffffffu) {
        if (e >= nEl) return 1;
        for (int i = 0; i < W; i++) out[i] = val[(uint64_t)e * W + i];
        return 0;
    }
    if (interp == kSgSpline) {
        if (((uint64_t)k + 1) * 3 + 1 >= nEl) return 1;   // (elements k * 3 + 1, k * 3 + 2, (k + 1) * 3, (k + 1) * 3 + 1)
        const float* p0 = val + ((uint64_t)k * 3 + 1) * W;
        const float* m0 = val + ((uint64_t)k * 3 + 2) * W;
        const float* p1 = val + (((uint64_t)k + 1) * 3 + 1) * W;
        const float* m1 = val + (((uint64_t)k + 1) * 3) * W;
        float c[4];
        sg_spline_coeffs(f, c);
        const float d = t1 - t0;
        for (int i = 0; i < W; i++) out[i] = sg_spline(W == 3 ? d * m0[i] : m0[i] * d, p0[i], p1[i], W == 3 ? d * m1[i] : m1[i] * d, c);
        if (W == 4) sg_quat_normalize(out);
        return 0;
    }
    if ((uint32_t)k + 1 >= nEl) return 1;
    const float* a = val + (uint64_t)k * W;
    const float* b = val + ((uint64_t)k + 1) * W;
    if (W == 3) {
        const float u = 1 - f;
        for (int i = 0; i < 3; i++) out[i] = sg_fma(f, b[i], u * a[i]);
    } else {
        *trig |= sg_slerp(a, b, f, out);
        sg_quat_normalize(out);
    }
    return 0;
}

// Sampler::SampleFloat( t, k, i, count )
TBVH_SG_HD int sg_sample_float(uint32_t interp, const float* tm, uint32_t keyCount, const float* val, uint32_t nVal, float t, int32_t k, uint32_t i, uint32_t count, float* out) {
    if (k < 0 || (uint32_t)k + 1 >= keyCount) return 1;
    uint64_t e = ~0ull;
    if (k == 0 && t < tm[0]) e = interp == kSgSpline ? 1 : 0;
    const float t0 = tm[k], t1 = tm[k + 1];
    const float f = (t - t0) / (t1 - t0);
    if (e == ~0ull && f <= 0) e = 0;
    if (e == ~0ull && interp == kSgStep) e = (uint64_t)k;   // floatKey[k], whatever i
    if (e != ~0ull) {
        if (e >= nVal) return 1;
        *out = val[e];
        return 0;
    }
    const uint64_t a = (uint64_t)k * count + i, b = ((uint64_t)k + 1) * count + i;
    if (interp == kSgSpline) {
        if (b * 3 + 1 >= nVal) return 1;
        float c[4];
        sg_spline_coeffs(f, c);
        const float d = t1 - t0;
        *out = sg_spline_float(d * val[a * 3 + 2], val[a * 3 + 1], val[b * 3 + 1], d * val[b * 3], c);
        return 0;
    }
    if (b >= nVal) return 1;
    *out = sg_fma(1 - f, val[a], f * val[b]);   // (here the first product is the fused one)
    return 0;
}

// Channel::Update( dt ) for channel c.  shadowMask: the flags that make this call skip the write (kSgShadowAll when every animation advances,
// kSgShadowAnim when one does).  The channel's t and k advance either way.
TBVH_SG_HD void sg_channel(const SgView& g, uint32_t c, float dt, uint32_t shadowMask) {
    const uint32_t s = g.cSampler[c], node = g.cNode[c], target = g.cTarget[c];
    if (s >= g.nSamplers || node >= g.nNodes || target > 3) { sg_raise(g.status); return; }
    const uint32_t k0 = g.sKeyOff[s], k1 = g.sKeyOff[s + 1], v0 = g.sValOff[s], v1 = g.sValOff[s + 1];
    if (k0 >= k1 || k1 > g.nTimes || v0 > v1 || v1 > g.nValues) { sg_raise(g.status); return; }
    const uint32_t keyCount = k1 - k0, nVal = v1 - v0, interp = g.sInterp[s];
    const float* tm = g.times + k0;
    const float* val = g.values + v0;
    const uint32_t w0 = g.wOff[node], w1 = g.wOff[node + 1];
    if (w0 > w1 || w1 > g.nWeights) { sg_raise(g.status); return; }
    const bool write = (g.cFlags[c] & shadowMask) == 0;
    float t = g.cT[c] + dt;
    int32_t k = g.cK[c];
    const float animDuration = tm[keyCount - 1];
    const int W = target == 1 ? 4 : 3;
    float out[4];
    int trig = 0;
    if (animDuration == 0 || keyCount == 1) {
        g.cT[c] = t;
        if (target == 3) {
            if (nVal < 1) { sg_raise(g.status); return; }
            if (write) for (uint32_t i = w0; i < w1; i++) g.weights[i] = val[0];
            return;
        }
        if (nVal < (uint32_t)W) { sg_raise(g.status); return; }
        for (int i = 0; i < W; i++) out[i] = val[i];
    } else {
        if (k < 0 || (uint32_t)k >= keyCount) { sg_raise(g.status); return; }
        while (t >= animDuration) {
            const float n = t - animDuration;
            if (n == t) { sg_raise(g.status); return; }   // (the reference would not leave this loop; the time limits of the entry points keep it from being reached)
            t = n; k = 0;
        }
        while (t >= tm[((uint32_t)k + 1) % keyCount]) k++;
        g.cT[c] = t; g.cK[c] = k;
        if (target == 3) {
            const uint32_t count = w1 - w0;
            for (uint32_t i = 0; i < count; i++) {
                float w;
                if (sg_sample_float(interp, tm, keyCount, val, nVal, t, k, i, count, &w)) { sg_raise(g.status); return; }
                if (write) g.weights[w0 + i] = w;
            }
            return;
        }
        if (sg_sample_vec(W, interp, tm, keyCount, val, nVal, t, k, out, &trig)) { sg_raise(g.status); return; }
    }
    g.written[node] = 1;
    g.cTrig[c] = (uint32_t)trig;
    if (!write) return;
    float* dst = g.trs + 10 * (uint64_t)node + (target == 0 ? 0 : target == 1 ? 3 : 7);
    for (int i = 0; i < W; i++) dst[i] = out[i];
}

// the head of Node::Update: a node an animation channel wrote since the last walk rebuilds its local transform from T, R, S
TBVH_SG_HD void sg_node_local(const SgView& g, uint32_t n) {
    if (!g.written[n]) return;
    g.written[n] = 0;
    sg_local_from_trs(g.trs + 10 * (uint64_t)n, g.matrix + 16 * (uint64_t)n, g.local + 16 * (uint64_t)n);
}

// combinedTransform of node n: identity * local[root] * ... * local[n], multiplied left to right down its own ancestor chain — the products Node::Update's
// recursion performs for this node, so the same bits, without waiting for any other node
TBVH_SG_HD void sg_node_combine(const SgView& g, uint32_t n) {
    const uint32_t a0 = g.ancOff[n], a1 = g.ancOff[n + 1];
    if (a0 >= a1 || a1 > g.nAnc) { sg_raise(g.status); return; }
    float cur[16], nxt[16];
    sg_identity(cur);
    for (uint32_t i = a0; i < a1; i++) {
        const uint32_t a = g.anc[i];
        if (a >= g.nNodes) { sg_raise(g.status); return; }
        sg_mul(cur, g.local + 16 * (uint64_t)a, nxt);
        for (int j = 0; j < 16; j++) cur[j] = nxt[j];
    }
    float* dst = g.combined + 16 * (uint64_t)n;
    for (int j = 0; j < 16; j++) dst[j] = cur[j];
}

TBVH_SG_HD void sg_instance(const SgView& g, uint32_t i) {
    const uint32_t n = g.instNode[i];
    if (n >= g.nNodes) { sg_raise(g.status); return; }
    const float* src = g.combined + 16 * (uint64_t)n;
    float* dst = g.instOut + 16 * (uint64_t)i;
    for (int j = 0; j < 16; j++) dst[j] = src[j];
}

// jointMat = inverse( mesh node ) * joint node * inverseBind; a stale pair reads the joint node's combined transform of the previous walk
TBVH_SG_HD void sg_joint_pair(const SgView& g, uint32_t p) {
    const uint32_t m = g.pairMesh[p], j = g.pairJoint[p];
    if (m >= g.nNodes || j >= g.nNodes) { sg_raise(g.status); return; }
    float inv[16], a[16], r[16];
    sg_invert(g.combined + 16 * (uint64_t)m, inv);
    sg_mul(inv, (g.pairStale[p] ? g.combinedPrev : g.combined) + 16 * (uint64_t)j, a);
    sg_mul(a, g.invBind + 16 * (uint64_t)p, r);
    float* dst = g.jointOut + 16 * (uint64_t)p;
    for (int i = 0; i < 16; i++) dst[i] = r[i];
}

}  // namespace tbvh
