// pose_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's Mesh::SetPose( const Skin* ) and Mesh::SetPose( const vector<float>& )
// (tiny_scene.h) behind a C interface.
//
// Compiled at test time (tests/pose_lib.py: compile_ref_shim) from $TBVH_REFERENCE with the flags of oracle/Makefile, into the pytest temp dir;
// nothing of the reference is copied into the repository.  tiny_scene.h as it lies does not compile with g++ (a bare `#elif`), so the helper puts a
// temp copy with that one directive turned into `#else` first on the include path; the two *_s names the header uses are macros here.  The vector
// types are set up exactly as tiny_bvh_gltf.cpp sets them (tinyscene's types = tinybvh's), which is the build whose float operations DESIGN.md par. 14
// restates: operator*( float, bvhmat4 ) is then tiny_bvh.h's out-of-line one.
//
// Mesh::SetPose( skin ) also transforms one normal per vertex (read from a backup it takes of the triangles' normals) and rebuilds its FatTris from
// vertices 3 i .. 3 i + 2: the shim gives the mesh ceil( n / 3 ) zeroed triangles and pads the vertex arrays to a multiple of 3 with zero-weight
// vertices, so those loops stay inside their vectors.  Only the first n posed vertices are returned.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#define sprintf_s(buf, ...) snprintf((buf), sizeof(buf), __VA_ARGS__)
#define strcat_s(dst, src) strncat((dst), (src), sizeof(dst) - strlen(dst) - 1)

#define TINYBVH_IMPLEMENTATION
#include "tiny_bvh.h"
#define TINYSCENE_USE_CUSTOM_VECTOR_TYPES
namespace tinyscene {
using ts_int2 = tinybvh::bvhint2;
using ts_int3 = tinybvh::bvhint3;
using ts_uint2 = tinybvh::bvhuint2;
using ts_uint3 = tinybvh::bvhuint3;
using ts_uint4 = tinybvh::bvhuint4;
using ts_vec2 = tinybvh::bvhvec2;
using ts_vec3 = tinybvh::bvhvec3;
using ts_vec4 = tinybvh::bvhvec4;
using ts_mat4 = tinybvh::bvhmat4;
}  // namespace tinyscene
#define TINYSCENE_IMPLEMENTATION
#include "tiny_scene.h"

using namespace tinybvh;
using namespace tinyscene;

extern "C" {

// rest16: n x 4 floats (w ignored), joints4: n x 4 u32, weights16: n x 4 floats, mats16: nJoints x 16 floats (row-major); out16: n x 4 floats
void pref_skin(const float* rest16, uint32_t n, const uint32_t* joints4, const float* weights16, const float* mats16, uint32_t nJoints, float* out16) {
    const uint32_t np = (n + 2) / 3 * 3;
    Mesh* mesh = new Mesh();
    mesh->vertices.resize(np);
    mesh->joints.resize(np);
    mesh->weights.resize(np);
    std::memset((void*)mesh->vertices.data(), 0, np * sizeof(bvhvec4));
    std::memset((void*)mesh->joints.data(), 0, np * sizeof(bvhuint4));
    std::memset((void*)mesh->weights.data(), 0, np * sizeof(bvhvec4));
    std::memcpy((void*)mesh->vertices.data(), rest16, (size_t)n * 16);
    std::memcpy((void*)mesh->joints.data(), joints4, (size_t)n * 16);
    std::memcpy((void*)mesh->weights.data(), weights16, (size_t)n * 16);
    mesh->triangles.resize(np / 3);
    std::memset((void*)mesh->triangles.data(), 0, (np / 3) * sizeof(FatTri));
    // Skin has no default constructor: one in zeroed storage (its members are a string, an int and vectors), the members it needs constructed in place
    void* store = calloc(1, sizeof(Skin));
    Skin* skin = (Skin*)store;
    new (&skin->name) std::string();
    new (&skin->inverseBindMatrices) std::vector<bvhmat4>();
    new (&skin->jointMat) std::vector<bvhmat4>();
    new (&skin->joints) std::vector<int>();
    skin->jointMat.resize(nJoints);
    std::memcpy((void*)skin->jointMat.data(), mats16, (size_t)nJoints * 64);
    mesh->SetPose(skin);
    std::memcpy(out16, mesh->vertices.data(), (size_t)n * 16);
    skin->~Skin();
    free(store);
    delete mesh;
}

// positions12: (nTargets + 1) arrays of n x 3 floats, array 0 the base; weights: nTargets floats; out16: n x 4 floats
void pref_morph(const float* positions12, uint32_t n, uint32_t nTargets, const float* weights, float* out16) {
    Mesh* mesh = new Mesh();
    mesh->vertices.resize(n);
    mesh->poses.resize(nTargets + 1);
    for (uint32_t j = 0; j <= nTargets; j++) {
        mesh->poses[j].positions.resize(n);
        std::memcpy((void*)mesh->poses[j].positions.data(), positions12 + (size_t)j * n * 3, (size_t)n * 12);
    }
    std::vector<float> w(weights, weights + nTargets);
    mesh->SetPose(w);
    std::memcpy(out16, mesh->vertices.data(), (size_t)n * 16);
    delete mesh;
}

}  // extern "C"
