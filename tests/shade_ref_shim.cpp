// shade_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's GetShadingData (tiny_bvh_foliage.cpp:80-125) behind a C interface.
//
// Compiled at test time (tests/shade_lib.py: compile_ref_shim) from $TBVH_REFERENCE with the flags of oracle/Makefile, into the pytest temp dir;
// nothing of the reference is copied into the repository.  tiny_bvh_foliage.cpp is included where it lies: FENSTER_H is predefined so that its window
// header stays out, a stand-in `struct fenster` and the two window calls the file names take its place (the file has no main of its own: that is in
// the window header).  tiny_scene.h as it lies does not compile with g++ (a bare `#elif`), and an #include "tiny_scene.h" inside the reference's file
// finds the one beside it first: so the temp copy with that directive turned into `#else` (tests/pose_ref_shim.cpp's trick) is included HERE, with
// the vector types set up exactly as the file sets them, and the header's guard makes the file's own include a no-op.
//
// The second interface puts the real Mesh::SetPose( const Skin* ) and Mesh::SetPose( const vector<float>& ) (tiny_scene.h) behind sref_setpose_skin /
// sref_setpose_morph and returns the mesh's `triangles` array: the FatTri half of the pose (vertex0..2, vN0..2 and, for a skin, Nx Ny Nz).
//
// GetShadingData reads scene.instPool, scene.meshPool[ blasIdx ]->triangles, Scene::materials and Scene::textures: the shim fills them with stand-ins
// (as tests/omm_ref_shim.cpp does) and restores them afterwards.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#define sprintf_s(buf, ...) snprintf((buf), sizeof(buf), __VA_ARGS__)
#define strcat_s(dst, src) strncat((dst), (src), sizeof(dst) - strlen(dst) - 1)

#define FENSTER_H
struct fenster { int keys[256]; };
static void fenster_update_title(fenster*, char*) {}
static int GetAsyncKeyState(int) { return 0; }

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
#include "tiny_scene.h"   // (the temp copy: first on the include path)

#undef TINYBVH_IMPLEMENTATION     // (the implementation halves lie outside the headers' guards: once is enough)
#undef TINYSCENE_IMPLEMENTATION
#undef TINYOBJLOADER_IMPLEMENTATION
#undef TINYGLTF_IMPLEMENTATION
#undef STB_IMAGE_IMPLEMENTATION
#include "tiny_bvh_foliage.cpp"

static_assert(sizeof(FatTri) == 192 && sizeof(BLASInstance) == 192, "record sizes");
static_assert(offsetof(Ray, D) == 16 && offsetof(Ray, hit) == 44 && sizeof(Ray) >= 64, "the ray record the queries leave");

extern "C" {

// instances192: nInst BLASInstance records; fatTris[s] / nTris[s]: the FatTri array of BLAS slot s (may be null / 0); materials5: nMat x (3 float colour,
// u32 colour texture, u32 normal texture; 0xFFFFFFFF = none); texels[k]: widths[k] x heights[k] u32; rays: n records `stride` bytes apart (the first 64
// are read); out: n x 12 floats = albedo, alpha, N, bits of material, iN, 0 (the colour texel's word of tbvh_shade_hits is an input byte, not arithmetic:
// the tests take it from the restatement).  Every record must be a hit with in-range indices whose texel reads lie inside the textures.
void sref_shade(const void* instances192, uint32_t nInst, const void* const* fatTris, const uint32_t* nTris, uint32_t nSlots, const uint32_t* materials5,
                uint32_t nMat, const uint32_t* const* texels, const uint32_t* widths, const uint32_t* heights, uint32_t nTex, const void* rays, uint32_t stride,
                uint32_t n, float* out) {
    std::vector<Material*> keepM;
    std::vector<Texture*> keepT;
    std::vector<Mesh*> keepP;
    std::vector<BLASInstance> keepI;
    keepM.swap(Scene::materials); keepT.swap(Scene::textures); keepP.swap(Scene::meshPool); keepI.swap(Scene::instPool);
    for (uint32_t k = 0; k < nTex; k++) {
        Texture* t = new Texture();
        t->width = widths[k]; t->height = heights[k];
        t->idata = (decltype(t->idata))texels[k];
        Scene::textures.push_back(t);
    }
    for (uint32_t k = 0; k < nMat; k++) {
        Material* m = new Material();
        float c[3];
        memcpy(c, materials5 + 5 * k, 12);
        m->color.value = bvhvec3(c[0], c[1], c[2]);
        m->color.textureID = (int)materials5[5 * k + 3];     // (0xFFFFFFFF -> -1)
        m->normals.textureID = (int)materials5[5 * k + 4];
        Scene::materials.push_back(m);
    }
    for (uint32_t s = 0; s < nSlots; s++) {
        Mesh* mesh = new Mesh();
        mesh->triangles.resize(nTris[s]);
        if (nTris[s]) memcpy((void*)mesh->triangles.data(), fatTris[s], (size_t)nTris[s] * sizeof(FatTri));
        Scene::meshPool.push_back(mesh);
    }
    Scene::instPool.resize(nInst);
    memcpy((void*)Scene::instPool.data(), instances192, (size_t)nInst * sizeof(BLASInstance));
    for (uint32_t i = 0; i < n; i++) {
        Ray ray;
        memset((void*)&ray, 0, sizeof(Ray));
        memcpy((void*)&ray, (const char*)rays + (size_t)i * stride, 64);
        bvhvec3 albedo( 0 ), N( 0 ), iN( 0 );
        float alpha = 0;
        GetShadingData(ray, albedo, alpha, N, iN);
        float* o = out + 12 * (size_t)i;
        o[0] = albedo.x; o[1] = albedo.y; o[2] = albedo.z; o[3] = alpha;
        o[4] = N.x; o[5] = N.y; o[6] = N.z;
        o[8] = iN.x; o[9] = iN.y; o[10] = iN.z;
        const uint32_t mat = Scene::meshPool[Scene::instPool[ray.hit.inst].blasIdx]->triangles[ray.hit.prim].material;
        memcpy(o + 7, &mat, 4);
        o[11] = 0;   // (the texel word: the caller fills it from the restatement; it is an input byte, not arithmetic)
    }
    for (Mesh* m : Scene::meshPool) delete m;
    for (Texture* t : Scene::textures) { t->idata = nullptr; delete t; }
    for (Material* m : Scene::materials) delete m;
    Scene::materials.swap(keepM); Scene::textures.swap(keepT); Scene::meshPool.swap(keepP); Scene::instPool.swap(keepI);
}

// The real Mesh::SetPose( skin ) over a flat mesh of n vertices (n a multiple of 3) whose n / 3 FatTri records are `fat` (in and out): the rest normals
// are put where the reference's first call backs them up from (the records' vN0..2).  rest16, joints4, weights16: n x 4; mats16: nJoints x 16 floats.
void sref_setpose_skin(const float* rest16, uint32_t n, const uint32_t* joints4, const float* weights16, const float* normals12, const float* mats16, uint32_t nJoints,
                       void* fat) {
    Mesh* mesh = new Mesh();
    mesh->vertices.resize(n); mesh->joints.resize(n); mesh->weights.resize(n);
    memcpy((void*)mesh->vertices.data(), rest16, (size_t)n * 16);
    memcpy((void*)mesh->joints.data(), joints4, (size_t)n * 16);
    memcpy((void*)mesh->weights.data(), weights16, (size_t)n * 16);
    mesh->triangles.resize(n / 3);
    memcpy((void*)mesh->triangles.data(), fat, (size_t)(n / 3) * sizeof(FatTri));
    for (uint32_t i = 0; i < n / 3; i++) {
        FatTri& t = mesh->triangles[i];
        memcpy((void*)&t.vN0, normals12 + 9 * (size_t)i, 12); memcpy((void*)&t.vN1, normals12 + 9 * (size_t)i + 3, 12); memcpy((void*)&t.vN2, normals12 + 9 * (size_t)i + 6, 12);
    }
    void* store = calloc(1, sizeof(Skin));   // (Skin has no default constructor: the members it needs constructed in place, as tests/pose_ref_shim.cpp does)
    Skin* skin = (Skin*)store;
    new (&skin->name) std::string();
    new (&skin->inverseBindMatrices) std::vector<bvhmat4>();
    new (&skin->jointMat) std::vector<bvhmat4>();
    new (&skin->joints) std::vector<int>();
    skin->jointMat.resize(nJoints);
    memcpy((void*)skin->jointMat.data(), mats16, (size_t)nJoints * 64);
    mesh->SetPose(skin);
    memcpy(fat, mesh->triangles.data(), (size_t)(n / 3) * sizeof(FatTri));
    skin->~Skin();
    free(store);
    delete mesh;
}

// The real Mesh::SetPose( weights ): positions12 and normals12 hold (nTargets + 1) arrays of n x 3 floats, array 0 the base; fat: n / 3 records, in and out.
void sref_setpose_morph(const float* positions12, const float* normals12, uint32_t n, uint32_t nTargets, const float* weights, void* fat) {
    Mesh* mesh = new Mesh();
    mesh->vertices.resize(n);
    mesh->poses.resize(nTargets + 1);
    for (uint32_t j = 0; j <= nTargets; j++) {
        mesh->poses[j].positions.resize(n); mesh->poses[j].normals.resize(n);
        memcpy((void*)mesh->poses[j].positions.data(), positions12 + (size_t)j * n * 3, (size_t)n * 12);
        memcpy((void*)mesh->poses[j].normals.data(), normals12 + (size_t)j * n * 3, (size_t)n * 12);
    }
    mesh->triangles.resize(n / 3);
    memcpy((void*)mesh->triangles.data(), fat, (size_t)(n / 3) * sizeof(FatTri));
    std::vector<float> w(weights, weights + nTargets);
    mesh->SetPose(w);
    memcpy(fat, mesh->triangles.data(), (size_t)(n / 3) * sizeof(FatTri));
    delete mesh;
}

}  // extern "C"
