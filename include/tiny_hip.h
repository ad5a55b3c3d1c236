// tiny_hip.h — the binding a tinybvh maintainer adds next to tiny_ocl.h: a header-only C++ layer over the C ABI of the MI355X engine
// (tinybvh_amd.h; link with -ltinybvh_amd) for the GPU call sites of the reference:
//   tiny_bvh_speedtest.cpp:1092-1241   three blocks of { tinyocl::Buffer x 2-3, CopyToDevice, Kernel::SetArguments, Kernel::Run,
//                                      clWaitForEvents, clGetEventProfilingInfo, CopyFromDevice }      ->  tinyhip::Scene
//   tiny_bvh_minimal_gpu.cpp:50-93     the same for one layout                                         ->  tinyhip::Scene
//   tiny_bvh_gpu.cpp:128-158           the wavefront frame loop over wavefront.cl                      ->  tinyhip::PathTracer
//   tiny_ocl.h:362-364                 ONE process-global OpenCL device                                ->  tinyhip::Context(device), any number
// Include AFTER tiny_bvh.h (it uses tinybvh::BVH_GPU / BVH4_GPU / BVH8_CWBVH / Ray / bvhvec4 as they are).  Errors: the C ABI returns status
// codes and never exits; this layer mirrors tinyocl's FatalError for the demos — it prints tbvh_last_error() and exits — IN THE APPLICATION.
// Compiled and run by examples/speedtest_gpu_section.cpp and examples/wavefront_demos.cpp (tests/test_examples.py).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "tinybvh_amd.h"

namespace tinyhip {

inline void Check(int rc, const char* what) {
    if (rc) { fprintf(stderr, "tinyhip: %s -> %d: %s\n", what, rc, tbvh_last_error()); exit(1); }
}

// one shared tbvh_context per HIP device, created on first use (tinyocl::Kernel::InitCL creates its single context the same way, tiny_ocl.h:945-1139).
// Threads: every call of the C ABI takes its context's lock, so host threads may share this context and the Scenes on it the way the
// reference's callers share a const BVH (tiny_bvh_speedtest.cpp:1077-1083: Intersect from 8 threads) — their calls serialise.  A thread whose
// queries should OVERLAP with other threads' on the device takes a context of its own: NewContext() + the Scene constructors' last argument.
inline tbvh_context* Context(int device = 0) {
    static tbvh_context* ctx[64] = {};
    static std::mutex m;
    if (device < 0 || device >= 64) { fprintf(stderr, "tinyhip: device %d out of range\n", device); exit(1); }
    std::lock_guard<std::mutex> lk(m);
    if (!ctx[device]) Check(tbvh_init(device, &ctx[device]), "tbvh_init");
    return ctx[device];
}
// a context of the caller's own on `device` (its own stream, staging buffers and lock); release with tbvh_shutdown after its Scenes are gone
inline tbvh_context* NewContext(int device = 0) {
    tbvh_context* c = nullptr;
    Check(tbvh_init(device, &c), "tbvh_init");
    return c;
}
inline int DeviceCount() { const int n = tbvh_device_count(); return n < 0 ? 0 : n; }
// the CL_PROFILING_COMMAND_* equivalent costs two event records per query: a renderer that never calls LastKernelMs() switches it off
inline void SetTiming(bool enabled, tbvh_context* ctx = nullptr, int device = 0) { Check(tbvh_set_timing(ctx ? ctx : Context(device), enabled ? 1 : 0), "tbvh_set_timing"); }

// One uploaded layout: replaces the Buffer triple + Kernel of a speedtest GPU block.  The blobs are consumed verbatim.
class Scene {
public:
    // own: a context from NewContext() for a thread of its own; nullptr = the shared context of the device
    Scene(const tinybvh::BVH_GPU& b, const tinybvh::bvhvec4* verts, int device = 0, tbvh_context* own = nullptr) : dev(device), ctx(own ? own : Context(device)) {
        Check(tbvh_upload_bvh_gpu(ctx, b.bvhNode, b.usedNodes, b.bvh.primIdx, b.bvh.idxCount, verts, b.triCount, &s), "tbvh_upload_bvh_gpu");
    }
    // a BVH_GPU uploads however it was built: the vertices, their stride and the index buffer are taken from the object itself (b.bvh.verts.data /
    // .stride, b.bvh.vertIdx — Build( verts, indices, n ), Build( bvhvec4slice, indices, n ) or the flat Build( verts, n ); tbvh_upload_bvh_gpu_mesh).
    // vertCount: the number of vertices behind the slice; 0 = found here — BVH_GPU::Build( verts, indices, n ) sets slice.count = 3 n, not the vertex
    // count (tiny_bvh.h:4564), so for an indexed BVH it is max( index ) + 1, for a flat one slice.count.  The arrays stay the caller's.
    explicit Scene(const tinybvh::BVH_GPU& b, int device = 0, tbvh_context* own = nullptr, uint32_t vertCount = 0) : dev(device), ctx(own ? own : Context(device)) {
        vertIdx = b.bvh.vertIdx; meshTris = b.triCount;
        nVerts = vertCount ? vertCount : b.bvh.verts.count;
        if (!vertCount && vertIdx) { nVerts = 0; for (size_t i = 0; i < (size_t)meshTris * 3; i++) if (vertIdx[i] >= nVerts) nVerts = vertIdx[i] + 1; }
        const tbvh_mesh m = MeshOf(b.bvh.verts, vertIdx);
        Check(tbvh_upload_bvh_gpu_mesh(ctx, b.bvhNode, b.usedNodes, b.bvh.primIdx, b.bvh.idxCount, &m, &s), "tbvh_upload_bvh_gpu_mesh");
    }
    explicit Scene(const tinybvh::BVH4_GPU& b, int device = 0, tbvh_context* own = nullptr) : dev(device), ctx(own ? own : Context(device)) {
        Check(tbvh_upload_bvh4_gpu(ctx, b.bvh4Data, b.usedBlocks, &s), "tbvh_upload_bvh4_gpu");
    }
    explicit Scene(const tinybvh::BVH8_CWBVH& b, int device = 0, tbvh_context* own = nullptr) : dev(device), ctx(own ? own : Context(device)) {
        Check(tbvh_upload_cwbvh(ctx, b.bvh8Data, b.usedBlocks, b.bvh8Tris, (uint64_t)b.bvh8.idxCount * 3, &s), "tbvh_upload_cwbvh");
    }
#ifdef DOUBLE_PRECISION_SUPPORT
    // BVH_Double (tiny_bvh.h:1035-1090): traced in fp64 over RayEx records (tbvh_upload_bvh_double; custom geometry: SphereBVH_Double below)
    explicit Scene(const tinybvh::BVH_Double& b, int device = 0, tbvh_context* own = nullptr) : dev(device), ctx(own ? own : Context(device)) {
        Check(tbvh_upload_bvh_double(ctx, b.bvhNode, b.usedNodes, b.primIdx, b.idxCount, b.verts, b.triCount, &s), "tbvh_upload_bvh_double");
    }
    // a BVH_Double built over BLASInstanceEx records (BVH_Double::Build( BLASInstanceEx*, ... )): blas[i] is the Scene of blasIdx == i
    Scene(const tinybvh::BVH_Double& tlas, const std::vector<Scene*>& blas, int device = 0, tbvh_context* own = nullptr) : dev(device), ctx(own ? own : Context(device)) {
        std::vector<tbvh_scene*> h;
        for (Scene* b : blas) h.push_back(b->Handle());
        Check(tbvh_upload_tlas_double(ctx, tlas.bvhNode, tlas.usedNodes, tlas.primIdx, tlas.idxCount, tlas.instList, tlas.triCount, h.data(), h.size(), &s),
              "tbvh_upload_tlas_double");
    }
    // BVH_Double::Intersect( RayEx& ) / IsOccluded( const RayEx& ) (TLAS: IntersectTLAS / IsOccludedTLAS) over a host RayEx[], in place
    void Intersect(tinybvh::RayEx* rays, size_t n) { Check(tbvh_intersect_ex(s, rays, n), "tbvh_intersect_ex"); }
    void IsOccluded(const tinybvh::RayEx* rays, size_t n, uint8_t* out) { Check(tbvh_occluded_ex(s, rays, n, out), "tbvh_occluded_ex"); }
    // double scenes that move.  A TLAS: "just move build to Tick if instance transforms are not static" (tiny_bvh_anim_double.cpp:110) —
    // BLASInstanceEx::Update + BVH_Double::Build( BLASInstanceEx*, ... ) on the device from n_inst x 16 row-major doubles (nullptr: the transforms
    // the records hold; onDevice: a device array), asynchronous ...
    void RebuildOnDevice(const double* transforms16 = nullptr, bool onDevice = false) {
        Check(tbvh_rebuild_tlas_double_device(s, transforms16, onDevice ? 1 : 0), "tbvh_rebuild_tlas_double_device");
    }
    // ... or the TLAS rebuilt by tinybvh on the host, into the same Scene (the BLAS list stays)
    void Update(const tinybvh::BVH_Double& tlas) {
        Check(tbvh_update_tlas_double(s, tlas.bvhNode, tlas.usedNodes, tlas.primIdx, tlas.idxCount, tlas.instList, tlas.triCount), "tbvh_update_tlas_double");
    }
    // A BLAS: same topology, new vertices (the reference has no BVH_Double::Refit); RebuildOnDevice() of the TLASes over it then reads the new bounds
    void Refit(const tinybvh::bvhdbl3* verts, size_t triCount, bool onDevice = false) { Check(tbvh_refit_double(s, verts, triCount, onDevice ? 1 : 0), "tbvh_refit_double"); }
    // read-back for inspection: the node array of a BLAS; of a TLAS also its instance indices and BLASInstanceEx records
    std::vector<tinybvh::BVH_Double::BVHNode> Download() {
        uint64_t n = 0;
        Check(tbvh_double_download(s, nullptr, 0, &n), "tbvh_double_download");
        std::vector<tinybvh::BVH_Double::BVHNode> nodes(n);
        Check(tbvh_double_download(s, nodes.data(), n, nullptr), "tbvh_double_download");
        return nodes;
    }
    // (any buffer may be nullptr; a buffer smaller than its array is refused; returns the node count)
    uint64_t Download(tinybvh::BVH_Double::BVHNode* nodes, size_t capNodes, uint64_t* idx, size_t capIdx, tinybvh::BLASInstanceEx* instances, size_t capInst) {
        uint64_t n = 0;
        Check(tbvh_tlas_double_download(s, nodes, capNodes, idx, capIdx, instances, capInst, &n), "tbvh_tlas_double_download");
        return n;
    }
#endif
    // the reference's flow for animated geometry — bvh.Refit() on the host, X.ConvertFrom( bvh ) again (tiny_bvh.h:3055-3093) — without a new
    // Scene: the refitted blob goes into the same device memory, TLASes over this BLAS keep working (tbvh_update_*)
    void Update(const tinybvh::BVH_GPU& b, const tinybvh::bvhvec4* verts) { Check(tbvh_update_bvh_gpu(s, b.bvhNode, b.usedNodes, b.bvh.primIdx, b.bvh.idxCount, verts, b.triCount), "tbvh_update_bvh_gpu"); }
    void Update(const tinybvh::BVH4_GPU& b) { Check(tbvh_update_bvh4_gpu(s, b.bvh4Data, b.usedBlocks), "tbvh_update_bvh4_gpu"); }
    void Update(const tinybvh::BVH8_CWBVH& b) { Check(tbvh_update_cwbvh(s, b.bvh8Data, b.usedBlocks, b.bvh8Tris, (uint64_t)b.bvh8.idxCount * 3), "tbvh_update_cwbvh"); }
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;
    ~Scene() { tbvh_free_scene(s); }
    // batched equivalents of X::Intersect( Ray& ) / X::IsOccluded( const Ray& ): a host tinybvh::Ray[] traced in place (the first 64 of every
    // 128 bytes go to the device, hit.t / u / v / prim come back: the memcpy loop of tiny_bvh_speedtest.cpp:1110-1115 and CopyFromDevice in one call)
    void Intersect(tinybvh::Ray* rays, size_t n) { Check(tbvh_intersect(s, rays, n, sizeof(tinybvh::Ray)), "tbvh_intersect"); }
    void IsOccluded(const tinybvh::Ray* rays, size_t n, uint8_t* out) { Check(tbvh_occluded(s, rays, n, sizeof(tinybvh::Ray), out), "tbvh_occluded"); }
    // device time of the last launch in ms: the CL_PROFILING_COMMAND_START / END read of tiny_bvh_speedtest.cpp:1126-1131
    float LastKernelMs() const { return tbvh_time_last_ms(ctx); }
    // animated geometry: BVH::Refit + ConvertFrom + upload of the reference flow, on the device
    void Refit(const tinybvh::bvhvec4* verts, size_t triCount) { Check(tbvh_refit(s, verts, triCount, 0), "tbvh_refit"); }
    // (Refit( slice ) and IntersectSpheres( .., slice, .. ) belong to a Scene made by Scene( const BVH_GPU& ), which knows the vertex and triangle
    // counts; on a Scene made by one of the other constructors they send an empty mesh and the library refuses it: TBVH_E_INVALID, "null/empty mesh")
    // the same for a Scene made from the BVH_GPU itself: the moved vertices as the slice the BVH reads (data and stride; the vertex count is the
    // constructor's).  An indexed scene holds its index buffer on the device, so only the shared vertices go up (tbvh_refit_mesh, indices = NULL).
    void Refit(const tinybvh::bvhvec4slice& verts) {
        const tbvh_mesh m = MeshOf(verts, nullptr);
        Check(tbvh_refit_mesh(s, &m), "tbvh_refit_mesh");
    }
    // WATERTIGHT_TRITEST (tiny_bvh.h:141) as a choice per scene instead of a build-time define: TBVH_TRITEST_MOLLER_TRUMBORE (the default) or
    // TBVH_TRITEST_WATERTIGHT; verts = the scene's bvhvec4 vertex array, 3 per triangle, as Refit takes it (nullptr on a scene that is watertight already).
    // Triangle BLASes only (tinybvh_amd.h: tbvh_set_triangle_test).
    void SetTriangleTest(int test, const tinybvh::bvhvec4* verts = nullptr, size_t triCount = 0) { Check(tbvh_set_triangle_test(s, test, verts, triCount, 0), "tbvh_set_triangle_test"); }
    int TriangleTest() const { return tbvh_scene_triangle_test(s); }
    // BVHBase::SetOpacityMicroMaps( maps, N ) (tiny_bvh.h:823-826): N x N bits per triangle, (N * N + 31) / 32 words each, copied to the device; honoured by
    // Intersect and IsOccluded, also of the TLASes over this scene.  maps == nullptr or N == 0 removes them.
    void SetOpacityMicroMaps(const uint32_t* maps, uint32_t N, size_t triCount) { Check(tbvh_set_opacity_micromaps(s, maps, N, triCount, 0), "tbvh_set_opacity_micromaps"); }
    // Mesh::CreateOpacityMicroMaps( N ) of tiny_scene.h followed by SetOpacityMicroMaps, on the device: the maps are baked from UVs and alpha textures into the
    // buffer the scene then owns (tinybvh_amd.h: tbvh_omm_source; N a power of two from 1 to 64)
    void BakeOpacityMicroMaps(const tbvh_omm_source& source, uint32_t N = 32) { Check(tbvh_bake_set_opacity_micromaps(s, &source, N), "tbvh_bake_set_opacity_micromaps"); }
    // BVH::IntersectSphere( pos, r ) batched (tiny_bvh.h:3140-3200; tiny_bvh_collide.cpp:169): hit[i] = 1 if sphere i = {x, y, z, r} touches a
    // triangle; verts = the scene's bvhvec4 vertex array, 3 per triangle, as Refit takes it.  BLAS scenes of the three GPU layouts only.
    void IntersectSpheres(const tinybvh::bvhvec4* spheres, size_t n, const tinybvh::bvhvec4* verts, size_t triCount, uint8_t* hit) {
        Check(tbvh_intersect_spheres(s, spheres, n, verts, triCount, hit), "tbvh_intersect_spheres");
    }
    // ... with the vertices as the slice the BVH reads, through the index buffer the Scene was made with (tbvh_intersect_spheres_mesh)
    void IntersectSpheres(const tinybvh::bvhvec4* spheres, size_t n, const tinybvh::bvhvec4slice& verts, uint8_t* hit) {
        const tbvh_mesh m = MeshOf(verts, vertIdx);
        Check(tbvh_intersect_spheres_mesh(s, spheres, n, &m, hit), "tbvh_intersect_spheres_mesh");
    }
    // the same over device arrays, asynchronous on the context's stream
    void IntersectSpheresDevice(const void* dSpheres, size_t n, const void* dVerts, size_t triCount, uint8_t* dHit) {
        Check(tbvh_intersect_spheres_device(s, dSpheres, n, dVerts, triCount, dHit), "tbvh_intersect_spheres_device");
    }
    tbvh_scene* Handle() const { return s; }
    // a TLAS scene: which tree tbvh_rebuild_tlas_device builds from now on — the LBVH (default) or, sah = true, the reference's own BVH::Build( BLASInstance*, n ) tree
    void SetTlasBuilder(bool sah) { Check(tbvh_tlas_set_builder(s, sah ? 2 : 0), "tbvh_tlas_set_builder"); }
    int Device() const { return dev; }
    tbvh_context* Ctx() const { return ctx; }
protected:
    // for a class whose own constructor uploads (SphereBVH_Double): no scene yet, Slot() receives it
    Scene(int device, tbvh_context* own) : dev(device), ctx(own ? own : Context(device)) {}
    tbvh_scene** Slot() { return &s; }
private:
    tbvh_mesh MeshOf(const tinybvh::bvhvec4slice& v, const uint32_t* indices) const {
        tbvh_mesh m;
        m.verts = v.data; m.n_verts = nVerts; m.stride_bytes = v.stride; m.on_device = 0; m.indices = indices; m.n_tris = meshTris;
        return m;
    }
    tbvh_scene* s = nullptr;
    int dev = 0;
    tbvh_context* ctx = nullptr;
    const uint32_t* vertIdx = nullptr;   // Scene( const BVH_GPU& ): the BVH's index buffer (the caller's), vertex and triangle counts
    uint32_t nVerts = 0, meshTris = 0;
};

#ifdef DOUBLE_PRECISION_SUPPORT
// BVH_Double over custom geometry, for the primitive of the reference's fp64 demos (tiny_bvh_custom_double.cpp, the sphere bunny of
// tiny_bvh_anim_double.cpp): struct Sphere { bvhdbl3 pos; double r; }, 32 bytes.  It is a Scene: Intersect / IsOccluded over RayEx records (a hit writes
// t, prim and inst and leaves u, v alone), and Scene( tlas, blas ) takes it in its BLAS list next to triangle BVH_Double scenes.  The callbacks are not
// called: the device runs the sphere test of tiny_bvh_anim_double.cpp (tinybvh_amd.h, "double precision, custom geometry"; IsOccluded answers what
// the closest-hit query would find, where the reference discards the callback's result).
class SphereBVH_Double : public Scene {
public:
    // b after b.Build( &sphereAABB, n ); spheres: the array the callbacks read
    SphereBVH_Double(const tinybvh::BVH_Double& b, const void* spheres32, size_t n, int device = 0, tbvh_context* own = nullptr) : Scene(device, own) {
        Check(tbvh_upload_custom_spheres_double(Ctx(), b.bvhNode, b.usedNodes, b.primIdx, b.idxCount, spheres32, n, Slot()), "tbvh_upload_custom_spheres_double");
    }
    // obj.Build( &sphereAABB, n ) on the device (an LBVH, one sphere per leaf); onDevice: spheres32 is device memory
    SphereBVH_Double(const void* spheres32, size_t n, bool onDevice = false, int device = 0, tbvh_context* own = nullptr) : Scene(device, own) {
        Check(tbvh_build_device_custom_spheres_double(Ctx(), spheres32, n, onDevice ? 1 : 0, Slot()), "tbvh_build_device_custom_spheres_double");
    }
    // ... again per frame, in the same scene: the TLASes over it keep working and need only their RebuildOnDevice() for the new root box
    void RebuildOnDevice(const void* spheres32, size_t n, bool onDevice = false) {
        Check(tbvh_rebuild_custom_spheres_double_device(Handle(), spheres32, n, onDevice ? 1 : 0), "tbvh_rebuild_custom_spheres_double_device");
    }
};
#endif

// VoxelSet (tiny_bvh.h:988-1030) on the device, with the reference's method names: Set fills a brick map on the host exactly as VoxelSet::Set
// does (tiny_bvh.h:3786-3807: the same brick numbering, so the same arrays), UpdateTopGrid (3809-3827) completes it and uploads it
// (tbvh_upload_voxelset); Intersect / IsOccluded trace a host tinybvh::Ray[] in place.  The reference's own VoxelSet keeps its arrays private,
// so this class holds its own.  Handle() is the scene a TLAS takes as a BLAS (tbvh_upload_tlas: every BLAS a voxel set; bounds the unit cube).
// One deviation, DESIGN.md par. 10: a voxel hit is recorded only if it beats the ray's hit.t (the reference's Intersect records the first
// filled voxel whatever hit.t holds).
class VoxelSet {
public:
    static constexpr uint32_t objectDim = 256;
    explicit VoxelSet(int device = 0, tbvh_context* own = nullptr) : ctx(own ? own : Context(device)), grid(32768u, 0u), brick(512u, 0u), top(16u, 0u) {}
    VoxelSet(const VoxelSet&) = delete;
    VoxelSet& operator=(const VoxelSet&) = delete;
    ~VoxelSet() { if (s) tbvh_free_scene(s); }
    void Set(const uint32_t x, const uint32_t y, const uint32_t z, const uint32_t v) {
        const uint32_t g = x / 8 + (y / 8) * 32 + (z / 8) * 1024;
        uint32_t b = grid[g];
        if (!b) { b = grid[g] = (uint32_t)(brick.size() / 512); brick.resize(brick.size() + 512, 0u); }
        brick[(size_t)b * 512 + (x & 7) + (y & 7) * 8 + (z & 7) * 64] = v;
    }
    // the top grid, then the upload (again after further Set calls: the set is re-uploaded; TLASes over the old upload keep the old one)
    void UpdateTopGrid() {
        for (uint32_t& w : top) w = 0;
        for (uint32_t x = 0; x < 8; x++) for (uint32_t y = 0; y < 8; y++) for (uint32_t z = 0; z < 8; z++) {
            bool has = false;
            for (uint32_t u = 0; u < 4 && !has; u++) for (uint32_t v = 0; v < 4 && !has; v++) for (uint32_t w = 0; w < 4 && !has; w++)
                has = grid[(x * 4 + u) + (y * 4 + v) * 32 + (z * 4 + w) * 1024] != 0;
            if (has) { const uint32_t ti = x + y * 8 + z * 64; top[ti >> 5] |= 1u << (ti & 31); }
        }
        if (s) { tbvh_free_scene(s); s = nullptr; }
        Check(tbvh_upload_voxelset(ctx, grid.data(), brick.data(), brick.size() / 512, top.data(), &s), "tbvh_upload_voxelset");
    }
    // VoxelSet::Intersect( Ray& ) / IsOccluded( const Ray& ) over a host tinybvh::Ray[] (after UpdateTopGrid)
    void Intersect(tinybvh::Ray* rays, size_t n) { Check(tbvh_intersect(s, rays, n, sizeof(tinybvh::Ray)), "tbvh_intersect"); }
    void IsOccluded(const tinybvh::Ray* rays, size_t n, uint8_t* out) { Check(tbvh_occluded(s, rays, n, sizeof(tinybvh::Ray), out), "tbvh_occluded"); }
    // ---- editing on the device (tinybvh_amd.h: "editing a voxel set"; DESIGN.md par. 21): the set changes where it lies, TLASes over it keep working.
    // The host arrays above do not follow device edits until Arrays() reads them back.
    void CreateOnDevice(uint64_t brickCapacity = 1024) {   // an empty set as the reference's constructor leaves it
        if (s) { tbvh_free_scene(s); s = nullptr; }
        Check(tbvh_voxelset_create(ctx, brickCapacity, &s), "tbvh_voxelset_create");
    }
    void Reserve(uint64_t nBricks) { Check(tbvh_voxelset_reserve(s, nBricks), "tbvh_voxelset_reserve"); }
    // n records { x, y, z, v }: the result of Set( x, y, z, v ) on each in turn; onDevice: the records are in device memory (16-byte aligned)
    void SetOnDevice(const uint32_t* xyzv, uint64_t n, bool onDevice = false) { Check(tbvh_voxelset_set(s, xyzv, n, onDevice ? 1 : 0), "tbvh_voxelset_set"); }
    void UpdateTopGridOnDevice() { Check(tbvh_voxelset_update_top_grid(s), "tbvh_voxelset_update_top_grid"); }
    // the device's arrays read back into this object's; returns the bricks in use (freeBrickPtr)
    uint64_t Arrays(const uint32_t** gridOut = nullptr, const uint32_t** brickOut = nullptr, const uint32_t** topOut = nullptr) {
        uint64_t used = 0;
        Check(tbvh_voxelset_download(s, nullptr, nullptr, 0, nullptr, &used), "tbvh_voxelset_download");
        brick.assign((size_t)used * 512, 0u);
        Check(tbvh_voxelset_download(s, grid.data(), brick.data(), used, top.data(), nullptr), "tbvh_voxelset_download");
        if (gridOut) *gridOut = grid.data();
        if (brickOut) *brickOut = brick.data();
        if (topOut) *topOut = top.data();
        return used;
    }
    // VoxelSet::GetNormal( const Ray& ) for a host tinybvh::Ray[] that holds hits on this set: normals16 gets { nx, ny, nz, 0 } per ray, zeros for a miss
    void Normals(const tinybvh::Ray* rays, size_t n, float* normals16) {
        Check(tbvh_voxel_normals(ctx, s, rays, (uint32_t)sizeof(tinybvh::Ray), n, normals16), "tbvh_voxel_normals");
    }
    // the scene-to-voxels loop of tiny_bvh_foliage.cpp:222-258 on the device: every opaque hit of 3 x 256^2 axis rays through `traced` (a triangle BLAS or a
    // TLAS over triangle BLASes of this context) becomes a Set here, then UpdateTopGrid.  shading: the table whose alpha skips a hit and whose albedo is the
    // value, or nullptr (params.color).  VoxelizeBounds / VoxelizeMatrix: the demo's bounding cube (216-220) and its matrix T (256-262, row-major).
    tbvh_voxelize_stats Voxelize(tbvh_scene* traced, const tbvh_voxelize_params& params, tbvh_shading* shading = nullptr) {
        tbvh_voxelize_stats st{};
        Check(tbvh_voxelize_device(traced, shading, &params, s, &st), "tbvh_voxelize_device");
        return st;
    }
    static tbvh_voxelize_params VoxelizeBounds(const float bmin[3], const float bmax[3]) {
        tbvh_voxelize_params p{};
        float c[3];
        for (int k = 0; k < 3; k++) { p.ext[k] = bmax[k] - bmin[k]; c[k] = (bmax[k] + bmin[k]) * 0.5f; }
        p.maxSize = p.ext[1] > p.ext[0] ? p.ext[1] : p.ext[0];
        if (p.ext[2] > p.maxSize) p.maxSize = p.ext[2];
        const float half = 0.525f * p.maxSize;
        for (int k = 0; k < 3; k++) p.bmin[k] = c[k] - half;
        p.color = 0xFFFFFFu;
        return p;
    }
    static void VoxelizeMatrix(const tbvh_voxelize_params& p, float T[16]) {
        const float scale = 1.0f / p.maxSize;
        for (int k = 0; k < 16; k++) T[k] = 0;
        T[0] = T[5] = T[10] = scale; T[15] = 1;
        T[3] = -p.bmin[0] * scale; T[7] = -p.bmin[1] * scale; T[11] = -p.bmin[2] * scale;
    }
    tbvh_scene* Handle() const { return s; }
    tbvh_context* Ctx() const { return ctx; }
private:
    tbvh_context* ctx;
    tbvh_scene* s = nullptr;
    std::vector<uint32_t> grid, brick, top;   // 32^3 brick indices, the bricks in use (brick 0 the empty one), 512 occupancy bits
};

// A BVH over custom geometry whose primitives are spheres (tinybvh's BVH::Build( customGetAABB, n ) with the anim demo's sphere callbacks) on the
// device: Build() takes the spheres {x, y, z, r} and builds with the library's builder, Upload() takes a reference BVH's own arrays (bvhNode,
// usedNodes, primIdx, idxCount).  Handle() is usable as a BLAS of tbvh_upload_tlas, also next to triangle BLASes (DESIGN.md par. 12).
class SphereBVH {
public:
    explicit SphereBVH(int device = 0, tbvh_context* own = nullptr) : ctx(own ? own : Context(device)) {}
    SphereBVH(const SphereBVH&) = delete;
    SphereBVH& operator=(const SphereBVH&) = delete;
    ~SphereBVH() { if (s) tbvh_free_scene(s); }
    void Build(const float* spheres16, uint32_t n) {
        tbvh_hostbvh* h = nullptr;
        Check(tbvh_host_build_custom_spheres(spheres16, n, &h), "tbvh_host_build_custom_spheres");
        const int r = tbvh_upload_custom_spheres(ctx, tbvh_host_blob(h, 0), tbvh_host_blob_count(h, 0), (const uint32_t*)tbvh_host_blob(h, 1),
                                                 tbvh_host_blob_count(h, 1), spheres16, n, Fresh());
        tbvh_host_free(h);
        Check(r, "tbvh_upload_custom_spheres");
    }
    void Upload(const void* nodes32, uint32_t usedNodes, const uint32_t* primIdx, uint32_t idxCount, const float* spheres16, uint32_t n) {
        Check(tbvh_upload_custom_spheres(ctx, nodes32, usedNodes, primIdx, idxCount, spheres16, n, Fresh()), "tbvh_upload_custom_spheres");
    }
    // sphere sets that move (tiny_bvh_anim.cpp's obj.Build( &sphereAABB, n ) per frame), on the device: LBVH (maxLeaf 1..4, 0 = 1) or PLOC
    // (ploc = true; radius 1..32, 0 = 16); Rebuild = a new tree in the same scene with the same builder, Refit = the same tree, new boxes.
    // spheres16 in host memory, or in device memory with onDevice = true.  A TLAS over Handle() needs no new upload after Rebuild / Refit.
    void BuildOnDevice(const float* spheres16, uint32_t n, bool ploc = false, uint32_t maxLeaf = 0, uint32_t radius = 0, bool onDevice = false) {
        Check(tbvh_build_device_custom_spheres(ctx, spheres16, n, onDevice ? 1 : 0, ploc ? 1 : 0, maxLeaf, radius, Fresh()), "tbvh_build_device_custom_spheres");
    }
    // the reference's own tree over the spheres, BVH::Build( &sphereAABB, n ), built on the device (maxLeaf 0 = its leaves, 1..4 = SplitLeafs); Rebuild
    // then rebuilds with SAH as well
    void BuildOnDeviceSAH(const float* spheres16, uint32_t n, uint32_t maxLeaf = 0, bool onDevice = false) {
        Check(tbvh_build_device_custom_spheres_sah(ctx, spheres16, n, onDevice ? 1 : 0, maxLeaf, Fresh()), "tbvh_build_device_custom_spheres_sah");
    }
    void Rebuild(const float* spheres16, uint32_t n, bool onDevice = false) {
        Check(tbvh_rebuild_custom_spheres_device(s, spheres16, n, onDevice ? 1 : 0), "tbvh_rebuild_custom_spheres_device");
    }
    void Refit(const float* spheres16, uint32_t n, bool onDevice = false) {
        Check(tbvh_refit_custom_spheres(s, spheres16, n, onDevice ? 1 : 0), "tbvh_refit_custom_spheres");
    }
    // the root box as it is on the device now: {min, max}, what tbvh_rebuild_tlas_device takes as this BLAS's bounds
    void Bounds(float bounds6[6]) const { Check(tbvh_custom_spheres_bounds(s, bounds6), "tbvh_custom_spheres_bounds"); }
    // BVH::Intersect( Ray& ) / IsOccluded( const Ray& ) with the sphere callbacks, over a host tinybvh::Ray[]
    void Intersect(tinybvh::Ray* rays, size_t n) { Check(tbvh_intersect(s, rays, n, sizeof(tinybvh::Ray)), "tbvh_intersect"); }
    void IsOccluded(const tinybvh::Ray* rays, size_t n, uint8_t* out) { Check(tbvh_occluded(s, rays, n, sizeof(tinybvh::Ray), out), "tbvh_occluded"); }
    tbvh_scene* Handle() const { return s; }
    tbvh_context* Ctx() const { return ctx; }
private:
    tbvh_scene** Fresh() { if (s) { tbvh_free_scene(s); s = nullptr; } return &s; }
    tbvh_context* ctx;
    tbvh_scene* s = nullptr;
};

// Mesh::SetPose of tiny_scene.h on the device (tbvh_pose_*): what Node::Update (tiny_scene.h:1973-2027) does per skinned / morphed mesh and frame —
// mesh->SetPose( skin ) or SetPose( weights ) on the CPU, then blas.dynamicGPU->Build( ... ) — becomes pose.SetPose( skin->jointMat.data(), n ) +
// pose.Refit( scene ): 64 bytes per joint go up, the vertices are made where the refit reads them.  Skin() / Morph() once per mesh; nVerts counts
// vertices (an indexed mesh: every shared vertex once).  Matrices are row-major 4 x 4 (ts_mat4 / bvhmat4::cell).  A Pose on a NewContext() context
// must be destroyed before that context's tbvh_shutdown (which frees the poses still alive on it).
class Pose {
public:
    explicit Pose(tbvh_context* own = nullptr, int device = 0) : ctx(own ? own : Context(device)) {}
    Pose(const Pose&) = delete;
    Pose& operator=(const Pose&) = delete;
    ~Pose() { tbvh_pose_free(p); }
    // Mesh::original / joints / weights: rest16 = bvhvec4 per vertex, joints4 = bvhuint4 per vertex, weights16 = bvhvec4 per vertex
    void Skin(const void* rest16, size_t nVerts, const uint32_t* joints4, const void* weights16, uint32_t nJoints) {
        tbvh_pose_free(p); p = nullptr;
        Check(tbvh_pose_create_skin(ctx, rest16, nVerts, joints4, weights16, nJoints, 0, &p), "tbvh_pose_create_skin");
    }
    // Mesh::poses[ 0 .. nTargets ].positions back to back: (nTargets + 1) arrays of nVerts * 3 floats, the base pose first
    void Morph(const float* positions12, size_t nVerts, uint32_t nTargets) {
        tbvh_pose_free(p); p = nullptr;
        Check(tbvh_pose_create_morph(ctx, positions12, nVerts, nTargets, 0, &p), "tbvh_pose_create_morph");
    }
    // Mesh::SetPose( const Skin* ): skin->jointMat.data(), skin->jointMat.size()
    void SetPose(const float* jointMats16, uint32_t nJoints, bool onDevice = false) { Check(tbvh_pose_set_skin(p, jointMats16, nJoints, onDevice ? 1 : 0), "tbvh_pose_set_skin"); }
    // Mesh::SetPose( const vector<float>& )
    void SetPose(const std::vector<float>& weights) { Check(tbvh_pose_set_morph(p, weights.data(), (uint32_t)weights.size(), 0), "tbvh_pose_set_morph"); }
    // the BLAS follows the posed vertices (a Scene made from an indexed mesh: through the index buffer it holds)
    void Refit(Scene& scene) { Check(tbvh_pose_refit(p, scene.Handle()), "tbvh_pose_refit"); }
    void Refit(tbvh_scene* scene) { Check(tbvh_pose_refit(p, scene), "tbvh_pose_refit"); }
    // the posed vertices on the device (bvhvec4 each): vertex input of tbvh_refit / tbvh_build_device* / a tbvh_mesh with on_device = 1
    const void* Vertices(size_t* nVerts = nullptr) const {
        const void* d = nullptr; uint64_t n = 0;
        Check(tbvh_pose_vertices(p, &d, &n), "tbvh_pose_vertices");
        if (nVerts) *nVerts = (size_t)n;
        return d;
    }
    void Download(void* dst16, size_t capVerts) { Check(tbvh_pose_download(p, dst16, capVerts), "tbvh_pose_download"); }
    // the FatTri half of Mesh::SetPose: every SetPose from now on also rewrites the records of blasSlot of `shading` (a tbvh_shading*, e.g. Shading::Handle()).
    // normals12: Mesh::origNormal (skin) or poses[ 0 .. nTargets ].normals back to back (morph); indices: nullptr for a flat mesh
    void AttachFatTris(tbvh_shading* shading, uint32_t blasSlot, const float* normals12, size_t nTris, const uint32_t* indices = nullptr) {
        Check(tbvh_pose_attach_fat_tris(p, shading, blasSlot, normals12, indices, nTris, 0), "tbvh_pose_attach_fat_tris");
    }
    tbvh_pose* Handle() const { return p; }
private:
    tbvh_context* ctx;
    tbvh_pose* p = nullptr;
};

// Scene::UpdateSceneGraph( dt ) without the BLAS / TLAS builds, kept on the device (tbvh_scenegraph_*): made once from a tbvh_scenegraph_desc (plain arrays: the
// node tree, the samplers' keys, the channels, the instances' nodes, the skins' joints and inverse bind matrices), then per frame Advance( dt ).  The three
// outputs are device pointers owned by the graph: InstanceTransforms() feeds tbvh_rebuild_tlas_device( tlas, ptr, 1, .. ), JointMatrices( use ) feeds
// Pose::SetPose( ptr, n, true ), MorphWeights( node ) feeds tbvh_pose_set_morph( pose, ptr, n, 1 ).
class SceneGraph {
public:
    explicit SceneGraph(const tbvh_scenegraph_desc& desc, tbvh_context* own = nullptr, int device = 0) : ctx(own ? own : Context(device)) {
        Check(tbvh_scenegraph_create(ctx, &desc, &g), "tbvh_scenegraph_create");
    }
    SceneGraph(const SceneGraph&) = delete;
    SceneGraph& operator=(const SceneGraph&) = delete;
    ~SceneGraph() { tbvh_scenegraph_free(g); }
    void Advance(float dt) { Check(tbvh_scenegraph_advance(g, dt), "tbvh_scenegraph_advance"); }                                   // Scene::UpdateSceneGraph
    void AdvanceAnimation(uint32_t anim, float dt) { Check(tbvh_scenegraph_advance_animation(g, anim, dt), "tbvh_scenegraph_advance_animation"); }   // Scene::UpdateAnimation
    void UpdateNodes() { Check(tbvh_scenegraph_update_nodes(g), "tbvh_scenegraph_update_nodes"); }                                 // the walk of Node::Update alone
    void SetTime(uint32_t anim, float t) { Check(tbvh_scenegraph_set_time(g, anim, t), "tbvh_scenegraph_set_time"); }              // Animation::SetTime
    void Reset(uint32_t anim) { Check(tbvh_scenegraph_reset(g, anim), "tbvh_scenegraph_reset"); }                                  // Animation::Reset
    void SetNodeTransform(uint32_t node, const float* mat16) { Check(tbvh_scenegraph_set_local(g, node, mat16), "tbvh_scenegraph_set_local"); }   // Scene::SetNodeTransform
    const float* InstanceTransforms(size_t* n = nullptr) const {
        const float* d = nullptr; uint64_t k = 0;
        Check(tbvh_scenegraph_instance_transforms(g, &d, &k), "tbvh_scenegraph_instance_transforms");
        if (n) *n = (size_t)k;
        return d;
    }
    const float* JointMatrices(uint32_t skinUse, uint32_t* nJoints = nullptr) const {
        const float* d = nullptr;
        Check(tbvh_scenegraph_joint_matrices(g, skinUse, &d, nJoints), "tbvh_scenegraph_joint_matrices");
        return d;
    }
    const float* MorphWeights(uint32_t node, uint32_t* nWeights = nullptr) const {
        const float* d = nullptr;
        Check(tbvh_scenegraph_morph_weights(g, node, &d, nWeights), "tbvh_scenegraph_morph_weights");
        return d;
    }
    void Download(int what, void* dst, size_t capBytes) { Check(tbvh_scenegraph_download(g, what, dst, capBytes), "tbvh_scenegraph_download"); }
    tbvh_scenegraph* Handle() const { return g; }
private:
    tbvh_context* ctx;
    tbvh_scenegraph* g = nullptr;
};

// GetShadingData of the reference's renderers on the device (tbvh_shading_*, tbvh_shade_hits): materials and textures once, the FatTri records of every BLAS
// slot (Mesh::triangles.data(), taken verbatim), then per frame ShadeHits after the trace: 48 bytes per ray — albedo + alpha, N + material, iN + texel.
//   tinyhip::Shading shading( materials, nMaterials, textures, nTextures );
//   shading.SetFatTris( blasIdx, mesh->triangles.data(), mesh->triangles.size() );
//   tlas.Intersect( rays, n ); shading.ShadeHits( tlas, rays, n, sizeof( tinybvh::Ray ), out48 );
class Shading {
public:
    Shading(const tbvh_material* materials, uint32_t nMaterials, const tbvh_alpha_texture* textures, uint32_t nTextures, tbvh_context* own = nullptr, int device = 0)
        : ctx(own ? own : Context(device)) {
        Check(tbvh_shading_create(ctx, materials, nMaterials, textures, nTextures, 0, &p), "tbvh_shading_create");
    }
    Shading(const Shading&) = delete;
    Shading& operator=(const Shading&) = delete;
    ~Shading() { tbvh_shading_free(p); }
    void SetFatTris(uint32_t blasSlot, const void* fatTris192, size_t nTris, bool onDevice = false) {
        Check(tbvh_shading_set_fat_tris(p, blasSlot, fatTris192, nTris, onDevice ? 1 : 0), "tbvh_shading_set_fat_tris");
    }
    // host ray records as Intersect left them, rayStride bytes apart (sizeof( tinybvh::Ray ) or 64); out48: 12 floats per ray
    void ShadeHits(Scene& scene, const void* rays, size_t n, uint32_t rayStride, void* out48) { Check(tbvh_shade_hits(p, scene.Handle(), rays, n, rayStride, out48), "tbvh_shade_hits"); }
    void ShadeHits(tbvh_scene* scene, const void* rays, size_t n, uint32_t rayStride, void* out48) { Check(tbvh_shade_hits(p, scene, rays, n, rayStride, out48), "tbvh_shade_hits"); }
    // device-resident records and output; asynchronous on the context's stream
    void ShadeHitsDevice(tbvh_scene* scene, const void* dRays, size_t n, uint32_t rayStride, void* dOut48) {
        Check(tbvh_shade_hits_device(p, scene, dRays, n, rayStride, dOut48), "tbvh_shade_hits_device");
    }
    void Download(uint32_t blasSlot, void* dst192, size_t capTris) { Check(tbvh_shading_download_fat_tris(p, blasSlot, dst192, capTris), "tbvh_shading_download_fat_tris"); }
    tbvh_shading* Handle() const { return p; }
private:
    tbvh_context* ctx;
    tbvh_shading* p = nullptr;
};

// tinyscene::SkyDome on the device (tbvh_sky_*): pixels as SkyDome::pixels after Load, 3 floats per texel, copied
class SkyDome {
public:
    SkyDome(const float* pixels12, uint32_t width, uint32_t height, tbvh_context* own = nullptr, int device = 0) : ctx(own ? own : Context(device)) {
        Check(tbvh_sky_create(ctx, pixels12, width, height, 0, &p), "tbvh_sky_create");
    }
    SkyDome(const SkyDome&) = delete;
    SkyDome& operator=(const SkyDome&) = delete;
    ~SkyDome() { tbvh_sky_free(p); }
    // n device-resident directions (float4, xyz read) -> the texel as ( z, y, x ) and its index; asynchronous on the context's stream
    void SampleDevice(const void* dDirs16, size_t n, void* dOut16) { Check(tbvh_sky_sample_device(p, dDirs16, n, dOut16), "tbvh_sky_sample_device"); }
    tbvh_sky* Handle() const { return p; }
private:
    tbvh_context* ctx;
    tbvh_sky* p = nullptr;
};

// A frame of the reference's CPU viewers (tiny_bvh_gltf.cpp / tiny_bvh_foliage.cpp: WorkerThread, Trace, SampleSky) rendered on the device (tbvh_viewer_*):
// eye, p1, p2, p3 as UpdateCamera leaves them; Pixels() is the window buffer (0x00BBGGRR, width * height words).  scene: a TLAS or a single triangle BLAS;
// sky may be null (every sample is 0).
class Viewer {
public:
    Viewer(uint32_t width, uint32_t height, tbvh_context* own = nullptr, int device = 0) : ctx(own ? own : Context(device)), w(width), h(height) {
        Check(tbvh_viewer_create(ctx, width, height, &p), "tbvh_viewer_create");
    }
    Viewer(const Viewer&) = delete;
    Viewer& operator=(const Viewer&) = delete;
    ~Viewer() { tbvh_viewer_destroy(p); }
    // stats == nullptr: asynchronous on the context's stream
    void Render(tbvh_scene* scene, const Shading& shading, const SkyDome* sky, const float eye[3], const float p1[3], const float p2[3], const float p3[3],
                uint32_t mode = TBVH_VIEWER_GLTF, const float* lightDir = nullptr, uint32_t maxRounds = 0, tbvh_viewer_stats* stats = nullptr) {
        tbvh_camera cam;
        for (int k = 0; k < 3; k++) { cam.eye[k] = eye[k]; cam.p1[k] = p1[k]; cam.p2[k] = p2[k]; cam.p3[k] = p3[k]; }
        cam.width = w; cam.height = h; cam.spp_x = cam.spp_y = 1;
        tbvh_viewer_params params = {mode, maxRounds, {lightDir ? lightDir[0] : 0.f, lightDir ? lightDir[1] : 0.f, lightDir ? lightDir[2] : 0.f}, 0u};
        Check(tbvh_viewer_render(p, scene, shading.Handle(), sky ? sky->Handle() : nullptr, &cam, &params, stats), "tbvh_viewer_render");
    }
    void Pixels(uint32_t* pixels) { Check(tbvh_viewer_read_pixels(p, pixels), "tbvh_viewer_read_pixels"); }   // synchronous
    void RGB(void* rgb16) { Check(tbvh_viewer_read_rgb(p, rgb16), "tbvh_viewer_read_rgb"); }
    void* RaysDevice() { void* d = nullptr; Check(tbvh_viewer_rays(p, &d), "tbvh_viewer_rays"); return d; }
    tbvh_viewer* Handle() const { return p; }
private:
    tbvh_context* ctx;
    uint32_t w, h;
    tbvh_viewer* p = nullptr;
};

// tinyocl::Buffer( bytes ) for a ray array that is traced many times (tiny_bvh_speedtest.cpp:1101-1108 wraps its ray array in one per GPU block): page-locked
// host memory of the library's for the object's lifetime (tbvh_pinned_malloc); a PACKED 64-byte ray array in it goes up by DMA straight from there.
class PinnedBuffer {
public:
    explicit PinnedBuffer(size_t bytes, tbvh_context* own = nullptr, int device = 0) : ctx(own ? own : Context(device)) { Check(tbvh_pinned_malloc(ctx, bytes, &p), "tbvh_pinned_malloc"); }
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() { tbvh_pinned_free(ctx, p); }
    void* GetHostPtr() const { return p; }      // (tinyocl::Buffer::GetHostPtr)
private:
    void* p = nullptr;
    tbvh_context* ctx;
};

// One host Ray[] over several devices (each holds a Scene of the same BVH): contiguous shards, results in place.
inline void IntersectSharded(const std::vector<Scene*>& replicas, tinybvh::Ray* rays, size_t n) {
    std::vector<tbvh_scene*> h;
    for (Scene* r : replicas) h.push_back(r->Handle());
    Check(tbvh_intersect_sharded(h.data(), (uint32_t)h.size(), rays, n, sizeof(tinybvh::Ray)), "tbvh_intersect_sharded");
}

// The frame loop of tiny_bvh_gpu.cpp:128-158 (SetRenderData, Generate, { Extend, Shade } x depth, Connect, Finalize) as one object: the image is
// cut into bands of rows, one per device, every band generated, traced, shaded and accumulated where it lives; Pixels() gathers the image.
// With one device this is tbvh_wavefront_render on the whole image.
class PathTracer {
public:
    // scenes[i]: the same BVH uploaded on device i; verts: the scene's vertex array (copied to every device)
    PathTracer(const std::vector<Scene*>& scenes, const tinybvh::bvhvec4* verts, size_t vertCount, uint32_t width, uint32_t height) : W(width), H(height) {
        const uint32_t n = (uint32_t)scenes.size();
        uint32_t row = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t next = (uint32_t)((uint64_t)(H / 4) * (i + 1) / n) * 4;   // bands of whole 4-row tiles
            tbvh_context* c = scenes[i]->Ctx();
            tbvh_wavefront* w = nullptr;
            Check(tbvh_wavefront_create(c, W, next - row, &w), "tbvh_wavefront_create");
            Check(tbvh_wavefront_set_band(w, row, H), "tbvh_wavefront_set_band");
            void* dv = nullptr;
            Check(tbvh_device_malloc(c, vertCount * sizeof(tinybvh::bvhvec4), &dv), "tbvh_device_malloc");
            Check(tbvh_copy_to_device(c, dv, verts, vertCount * sizeof(tinybvh::bvhvec4)), "tbvh_copy_to_device");
            wf.push_back(w); dverts.push_back(dv); sc.push_back(scenes[i]->Handle()); ctx.push_back(c);
            row = next;
        }
    }
    PathTracer(const PathTracer&) = delete;
    PathTracer& operator=(const PathTracer&) = delete;
    ~PathTracer() {
        for (size_t i = 0; i < wf.size(); i++) { tbvh_wavefront_destroy(wf[i]); tbvh_device_free(ctx[i], dverts[i]); }
    }
    // one frame (sample) of every band; accumulates unless params.clear
    void Render(const tbvh_camera& cam, const tbvh_wf_params& params, std::vector<tbvh_wf_stats>* stats = nullptr, std::vector<float>* dispatchMs = nullptr) {
        if (stats) stats->resize(wf.size());
        if (dispatchMs) dispatchMs->resize(wf.size());
        Check(tbvh_wavefront_render_sharded(wf.data(), sc.data(), dverts.data(), (uint32_t)wf.size(), &cam, &params, stats ? stats->data() : nullptr,
                                            dispatchMs ? dispatchMs->data() : nullptr), "tbvh_wavefront_render_sharded");
    }
    // the float RGBA accumulator of the whole image (W x H x 4)
    void Read(float* rgba) { Check(tbvh_wavefront_read_sharded(wf.data(), (uint32_t)wf.size(), rgba), "tbvh_wavefront_read_sharded"); }
    uint32_t Bands() const { return (uint32_t)wf.size(); }
private:
    uint32_t W, H;
    std::vector<tbvh_wavefront*> wf;
    std::vector<void*> dverts;
    std::vector<tbvh_scene*> sc;
    std::vector<tbvh_context*> ctx;
};

}  // namespace tinyhip
