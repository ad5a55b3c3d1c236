// pose_host.cpp — pose.h over whole host arrays, and the two entry points that offer it: tbvh_host_pose_skin / tbvh_host_pose_morph.  Plain C++ that needs
// pose.h, the public header and the library's error helper only, so that it can also be compiled on its own (with a sanitizer, into a stand-alone program
// that supplies tbvh_capi::fail: tools/pose_sanitize.cpp).  Built -ffp-contract=off like the rest.
#include "../../include/tinybvh_amd.h"
#include "pose.h"

namespace tbvh_capi {
int fail(int code, const char* fmt, ...);   // (capi_context.hip) sets tbvh_last_error() of the calling thread, returns code
}
using tbvh_capi::fail;

namespace tbvh {

uint64_t pose_first_bad_joint(const uint32_t* joints4, uint64_t nVerts, uint32_t nJoints) {
    for (uint64_t i = 0; i < nVerts; i++)
        for (int k = 0; k < 4; k++)
            if (joints4[4 * i + k] >= nJoints) return i;
    return nVerts;
}

void pose_skin_host(const float* rest16, uint64_t nVerts, const uint32_t* joints4, const float* weights16, const float* mats16, float* out16) {
    for (uint64_t i = 0; i < nVerts; i++) pose_skin_vertex(rest16 + 4 * i, joints4 + 4 * i, weights16 + 4 * i, mats16, out16 + 4 * i);
}

void pose_morph_host(const float* positions12, uint64_t nVerts, uint32_t nTargets, const float* weights, float* out16) {
    for (uint64_t i = 0; i < nVerts; i++) pose_morph_vertex(positions12, nVerts, nTargets, weights, i, out16 + 4 * i);
}

uint64_t pose_first_bad_corner(const uint32_t* indices, uint64_t nTris, uint64_t nVerts) {
    for (uint64_t i = 0; i < nTris; i++)
        for (int k = 0; k < 3; k++)
            if (indices[3 * i + k] >= nVerts) return i;
    return nTris;
}

}  // namespace tbvh

using namespace tbvh;

extern "C" {

int tbvh_host_pose_skin(const void* rest16, uint64_t nVerts, const uint32_t* joints4, const void* weights16, const float* mats16, uint32_t nJoints, void* out16) {
    if (!rest16 || !joints4 || !weights16 || !mats16 || !out16) return fail(TBVH_E_INVALID, "tbvh_host_pose_skin: null argument");
    if (nVerts == 0 || nJoints == 0) return fail(TBVH_E_INVALID, "tbvh_host_pose_skin: %llu vertices, %u joints", (unsigned long long)nVerts, nJoints);
    const uint64_t bad = pose_first_bad_joint(joints4, nVerts, nJoints);
    if (bad != nVerts)
        return fail(TBVH_E_FORMAT, "tbvh_host_pose_skin: vertex %llu: a joint index (%u %u %u %u) is not a joint (%u joints)", (unsigned long long)bad, joints4[4 * bad],
                    joints4[4 * bad + 1], joints4[4 * bad + 2], joints4[4 * bad + 3], nJoints);
    pose_skin_host((const float*)rest16, nVerts, joints4, (const float*)weights16, mats16, (float*)out16);
    return 0;
}

int tbvh_host_pose_morph(const float* positions12, uint64_t nVerts, uint32_t nTargets, const float* weights, void* out16) {
    if (!positions12 || !out16 || (nTargets && !weights)) return fail(TBVH_E_INVALID, "tbvh_host_pose_morph: null argument");
    if (nVerts == 0) return fail(TBVH_E_INVALID, "tbvh_host_pose_morph: no vertices");
    pose_morph_host(positions12, nVerts, nTargets, weights, (float*)out16);
    return 0;
}

int tbvh_host_pose_skin_normals(uint64_t nVerts, const uint32_t* joints4, const void* weights16, const float* mats16, uint32_t nJoints, const float* normals12,
                                void* out16) {
    if (!joints4 || !weights16 || !mats16 || !normals12 || !out16) return fail(TBVH_E_INVALID, "tbvh_host_pose_skin_normals: null argument");
    if (nVerts == 0 || nJoints == 0) return fail(TBVH_E_INVALID, "tbvh_host_pose_skin_normals: %llu vertices, %u joints", (unsigned long long)nVerts, nJoints);
    const uint64_t bad = pose_first_bad_joint(joints4, nVerts, nJoints);
    if (bad != nVerts) return fail(TBVH_E_FORMAT, "tbvh_host_pose_skin_normals: vertex %llu: a joint index is not a joint (%u joints)", (unsigned long long)bad, nJoints);
    for (uint64_t i = 0; i < nVerts; i++) pose_skin_normal(normals12 + 3 * i, joints4 + 4 * i, (const float*)weights16 + 4 * i, mats16, (float*)out16 + 4 * i);
    return 0;
}

int tbvh_host_pose_morph_normals(const float* normals12, uint64_t nVerts, uint32_t nTargets, void* out16) {
    if (!normals12 || !out16 || nVerts == 0) return fail(TBVH_E_INVALID, "tbvh_host_pose_morph_normals: null argument or no vertices");
    for (uint64_t i = 0; i < nVerts; i++) pose_morph_normal(normals12, nVerts, nTargets, i, (float*)out16 + 4 * i);
    return 0;
}

int tbvh_host_pose_update_fat_tris(void* fatTris192, uint64_t nTris, const void* verts16, const void* normals16, uint64_t nVerts, const uint32_t* indices, int skin) {
    if (!fatTris192 || !verts16 || !normals16 || nTris == 0) return fail(TBVH_E_INVALID, "tbvh_host_pose_update_fat_tris: null argument or no triangles");
    if (!indices && nVerts != 3 * nTris) return fail(TBVH_E_INVALID, "tbvh_host_pose_update_fat_tris: %llu vertices for %llu triangles without indices", (unsigned long long)nVerts, (unsigned long long)nTris);
    if (indices) {
        const uint64_t bad = pose_first_bad_corner(indices, nTris, nVerts);
        if (bad != nTris) return fail(TBVH_E_FORMAT, "tbvh_host_pose_update_fat_tris: triangle %llu: an index is not a vertex (%llu vertices)", (unsigned long long)bad, (unsigned long long)nVerts);
    }
    const float *v = (const float*)verts16, *n = (const float*)normals16;
    for (uint64_t i = 0; i < nTris; i++) {
        const uint64_t a = indices ? indices[3 * i] : 3 * i, b = indices ? indices[3 * i + 1] : 3 * i + 1, c = indices ? indices[3 * i + 2] : 3 * i + 2;
        pose_fat_tri((float*)fatTris192 + 48 * i, v + 4 * a, v + 4 * b, v + 4 * c, n + 4 * a, n + 4 * b, n + 4 * c, skin != 0);
    }
    return 0;
}

}  // extern "C"
