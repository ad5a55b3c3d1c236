// omm_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's CreateOpacityMicroMap (tiny_scene.h, the worker of Mesh::CreateOpacityMicroMaps)
// behind a C interface.
//
// Compiled at test time (tests/omm_lib.py: compile_ref_shim) from $TBVH_REFERENCE with the flags of oracle/Makefile, into the pytest temp dir;
// nothing of the reference is copied into the repository.  The set-up is tests/pose_ref_shim.cpp's: a temp copy of tiny_scene.h with its bare
// `#elif` turned into `#else` goes first on the include path, the two *_s names are macros, tinyscene's vector types are tinybvh's.
//
// The worker reads the triangle's material, that material's color.textureID (used only when > 1) and Scene::textures[ id ]: the shim fills
// Scene::materials / Scene::textures with stand-ins — textures 0 and 1 are empty placeholders, caller's texture k is Scene texture k + 2 and
// material k points at it, and one more material without a texture stands for TBVH_OMM_NO_TEXTURE.  Both vectors are restored afterwards.  The worker
// is called directly for the whole range (Mesh::CreateOpacityMicroMaps only slices the range over 32 threads and prints).
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

// uv: nTris x 6 floats (u0 v0 u1 v1 u2 v2), triTexture: nTris u32 (0xFFFFFFFF = none), texels[k]: widths[k] x heights[k] u32; out: nTris x ((N*N+31)/32) u32
void oref_bake(const float* uv, uint32_t nTris, const uint32_t* triTexture, const uint32_t* const* texels, const uint32_t* widths, const uint32_t* heights,
               uint32_t nTextures, int N, uint32_t* out) {
    std::vector<Material*> keepM;
    std::vector<Texture*> keepT;
    keepM.swap(Scene::materials);
    keepT.swap(Scene::textures);
    Scene::textures.push_back(new Texture());   // IDs 0 and 1: never looked at (the worker wants an ID above 1)
    Scene::textures.push_back(new Texture());
    for (uint32_t k = 0; k < nTextures; k++) {
        Texture* t = new Texture();
        t->width = widths[k]; t->height = heights[k];
        t->idata = (decltype(t->idata))texels[k];
        Scene::textures.push_back(t);
        Material* m = new Material();
        m->color.textureID = (int)k + 2;
        Scene::materials.push_back(m);
    }
    Scene::materials.push_back(new Material());   // textureID -1: the opaque one
    Mesh* mesh = new Mesh();
    mesh->triangles.resize(nTris);
    for (uint32_t i = 0; i < nTris; i++) {
        FatTri& t = mesh->triangles[i];
        t.u0 = uv[6 * i + 0]; t.v0 = uv[6 * i + 1];
        t.u1 = uv[6 * i + 2]; t.v1 = uv[6 * i + 3];
        t.u2 = uv[6 * i + 4]; t.v2 = uv[6 * i + 5];
        t.material = triTexture[i] == 0xFFFFFFFFu ? nTextures : triTexture[i];
    }
    mesh->omaps = out;   // (the caller's buffer: the worker writes triangle i's words at i * dwordsPerTri)
    CreateOpacityMicroMap(mesh, N, 0, (int)nTris);
    mesh->omaps = 0;
    delete mesh;
    for (Texture* t : Scene::textures) { t->idata = nullptr; delete t; }
    for (Material* m : Scene::materials) delete m;
    Scene::materials.swap(keepM);
    Scene::textures.swap(keepT);
}

}  // extern "C"
