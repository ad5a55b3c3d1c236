// viewer_ref_shim.cpp — TEST INFRASTRUCTURE ONLY: the real reference's CPU viewers (tiny_bvh_gltf.cpp, or with -DVIEWER_REF_FOLIAGE tiny_bvh_foliage.cpp)
// behind a C interface: their SampleSky, Trace and WorkerThread over a scene the test hands in.
//
// Compiled at test time (tests/viewer_lib.py: compile_ref_shim) from $TBVH_REFERENCE with the flags of oracle/Makefile, into the pytest temp dir; nothing
// of the reference is copied into the repository.  The viewer file is included where it lies, with the FENSTER_H / temp-tiny_scene.h trick of
// tests/shade_ref_shim.cpp (see there).  vref_scene fills Scene's pools (instances, meshes with their FatTri records, materials, textures), Scene::sky and
// a Scene::tlas built by the reference over BLASes the reference builds from the vertices; vref_frame sets the file's eye, p1, p2, p3 and runs its
// WorkerThread on one thread (800 x 600 is fixed by the file's macros).
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
// The viewer file defines a global `Scene scene`, whose destructor deletes whatever Scene's STATIC pools hold — pools that every shim of the reference loaded
// into one process shares.  If another shim left something there, each such global would delete it again at exit.  So this shim's own `scene` is destroyed
// over empty pools: g_guard (constructed after it, destroyed before it) moves the pools' contents into g_stash (constructed before it, destroyed after it),
// which puts them back.
struct VrefStash {
    std::vector<tinyscene::Material*> m; std::vector<tinyscene::Texture*> t; std::vector<tinyscene::Mesh*> p; tinyscene::SkyDome* sky = nullptr;
    void exchange() {
        using tinyscene::Scene;
        m.swap(Scene::materials); t.swap(Scene::textures); p.swap(Scene::meshPool);
        tinyscene::SkyDome* s = Scene::sky; Scene::sky = sky; sky = s;
    }
    ~VrefStash() { exchange(); }
};
static VrefStash g_stash;
#ifdef VIEWER_REF_FOLIAGE
#include "tiny_bvh_foliage.cpp"
#define VREF_TRACE(ray) Trace(ray, false)
#define VREF_WORKER(buf) WorkerThread(buf, false)
#else
#include "tiny_bvh_gltf.cpp"
#define VREF_TRACE(ray) Trace(ray)
#define VREF_WORKER(buf) WorkerThread(buf)
#endif

static struct VrefGuard { ~VrefGuard() { g_stash.exchange(); } } g_guard;

static_assert(sizeof(FatTri) == 192 && sizeof(BLASInstance) == 192, "record sizes");
static_assert(offsetof(Ray, D) == 16 && offsetof(Ray, hit) == 44 && sizeof(Ray) >= 64, "the ray record the queries leave");
static_assert(SCRWIDTH == 800 && SCRHEIGHT == 600, "the frame size of the file");

static std::vector<BVH*> g_blas;
static std::vector<std::vector<bvhvec4>> g_verts;
static std::vector<BVHBase*> g_list;
static SkyDome g_sky;
// Scene's pools are static members shared by every shim of the reference that one process has loaded: what another shim left there is set aside by vref_scene
// and put back by vref_release (as tests/shade_ref_shim.cpp does around each call)
static std::vector<Material*> g_keepM;
static std::vector<Texture*> g_keepT;
static std::vector<Mesh*> g_keepP;
static std::vector<BLASInstance> g_keepI;
static decltype(Scene::tlas) g_keepTlas = nullptr;
static SkyDome* g_keepSky = nullptr;

extern "C" {

// instances192: nInst complete BLASInstance records (transform, inverse, bounds, blasIdx); verts[s]: 3 x nTris[s] float4 of BLAS slot s, fatTris[s] its FatTri
// records; materials5: nMat x (3 float colour, u32 colour texture, u32 normal texture; 0xFFFFFFFF = none); texels[k]: widths[k] x heights[k] u32;
// sky: skyW x skyH x 3 floats, or null for no sky.  The arrays behind texels and sky must outlive the scene.
void vref_scene(const void* instances192, uint32_t nInst, const void* const* verts, const void* const* fatTris, const uint32_t* nTris, uint32_t nSlots,
                const uint32_t* materials5, uint32_t nMat, const uint32_t* const* texels, const uint32_t* widths, const uint32_t* heights, uint32_t nTex, const float* sky,
                uint32_t skyW, uint32_t skyH) {
    g_keepM.swap(Scene::materials); g_keepT.swap(Scene::textures); g_keepP.swap(Scene::meshPool); g_keepI.swap(Scene::instPool);
    g_keepTlas = Scene::tlas; g_keepSky = Scene::sky;
    Scene::tlas = nullptr;
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
        m->color.textureID = (int)materials5[5 * k + 3];
        m->normals.textureID = (int)materials5[5 * k + 4];
        Scene::materials.push_back(m);
    }
    g_verts.resize(nSlots);
    for (uint32_t s = 0; s < nSlots; s++) {
        Mesh* mesh = new Mesh();
        mesh->triangles.resize(nTris[s]);
        memcpy((void*)mesh->triangles.data(), fatTris[s], (size_t)nTris[s] * sizeof(FatTri));
        Scene::meshPool.push_back(mesh);
        g_verts[s].resize(3 * (size_t)nTris[s]);
        memcpy((void*)g_verts[s].data(), verts[s], 48 * (size_t)nTris[s]);
        BVH* b = new BVH();
        b->Build(g_verts[s].data(), nTris[s]);
        g_blas.push_back(b);
        g_list.push_back(b);
    }
    Scene::instPool.resize(nInst);
    memcpy((void*)Scene::instPool.data(), instances192, (size_t)nInst * sizeof(BLASInstance));
    Scene::tlas = new BVH();
    Scene::tlas->Build(Scene::instPool.data(), nInst, g_list.data(), nSlots);
    if (sky) {
        g_sky.pixels = (bvhvec3*)sky; g_sky.width = (int)skyW; g_sky.height = (int)skyH;
        Scene::sky = &g_sky;
    } else Scene::sky = nullptr;
}

// gives back what vref_scene made and puts Scene's pools back as it found them, so that nothing of the caller's is freed by a destructor at exit
void vref_release() {
    for (Mesh* m : Scene::meshPool) delete m;
    for (Texture* t : Scene::textures) { t->idata = nullptr; delete t; }
    for (Material* m : Scene::materials) delete m;
    Scene::meshPool.clear(); Scene::textures.clear(); Scene::materials.clear(); Scene::instPool.clear();
    delete Scene::tlas;
    for (BVH* b : g_blas) delete b;
    g_blas.clear(); g_list.clear(); g_verts.clear();
    g_sky.pixels = nullptr;
    Scene::materials.swap(g_keepM); Scene::textures.swap(g_keepT); Scene::meshPool.swap(g_keepP); Scene::instPool.swap(g_keepI);
    Scene::tlas = g_keepTlas; Scene::sky = g_keepSky;
    g_keepTlas = nullptr; g_keepSky = nullptr;
}

static void load(Ray& ray, const void* rays, uint32_t i) {
    memset((void*)&ray, 0, sizeof(Ray));
    memcpy((void*)&ray, (const char*)rays + 64 * (size_t)i, 64);
}

// Scene::tlas->Intersect / IsOccluded on 64-byte records, in place
void vref_intersect(void* rays, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) {
        Ray ray;
        load(ray, rays, i);
        Scene::tlas->Intersect(ray);
        memcpy((char*)rays + 64 * (size_t)i, (void*)&ray, 64);
    }
}
void vref_occluded(const void* rays, uint32_t n, uint8_t* out) {
    for (uint32_t i = 0; i < n; i++) {
        Ray ray;
        load(ray, rays, i);
        out[i] = Scene::tlas->IsOccluded(ray) ? 1 : 0;
    }
}

// the file's Trace on 64-byte records: rgb (3 floats each) out, the records as Trace leaves them
void vref_trace(void* rays, uint32_t n, float* rgb) {
    for (uint32_t i = 0; i < n; i++) {
        Ray ray;
        load(ray, rays, i);
        const bvhvec3 c = VREF_TRACE(ray);
        rgb[3 * i] = c.x; rgb[3 * i + 1] = c.y; rgb[3 * i + 2] = c.z;
        memcpy((char*)rays + 64 * (size_t)i, (void*)&ray, 64);
    }
}

void vref_sky(const float* pixels, uint32_t w, uint32_t h, const float* dirs3, uint32_t n, float* out3) {
    SkyDome* keep = Scene::sky;
    SkyDome tmp;
    tmp.pixels = (bvhvec3*)pixels; tmp.width = (int)w; tmp.height = (int)h;
    Scene::sky = &tmp;
    for (uint32_t i = 0; i < n; i++) {
        const bvhvec3 c = SampleSky(bvhvec3(dirs3[3 * i], dirs3[3 * i + 1], dirs3[3 * i + 2]));
        out3[3 * i] = c.x; out3[3 * i + 1] = c.y; out3[3 * i + 2] = c.z;
    }
    tmp.pixels = nullptr;
    Scene::sky = keep;
}

// WorkerThread on one thread with the file's eye, p1, p2, p3 set: buf = 800 x 600 words
void vref_frame(const float* e, const float* a, const float* b, const float* c, uint32_t* buf) {
    eye = bvhvec3(e[0], e[1], e[2]); p1 = bvhvec3(a[0], a[1], a[2]); p2 = bvhvec3(b[0], b[1], b[2]); p3 = bvhvec3(c[0], c[1], c[2]);
    jobCount = SCRWIDTH * SCRHEIGHT / 400;
    VREF_WORKER(buf);
}

}  // extern "C"
