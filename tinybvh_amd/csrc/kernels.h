// kernels.h — host-visible launchers of the device kernels (defined in kernels_*.hip).
#pragma once
#include <cstdio>
#include <vector>
#include "device_common.h"
#include "mesh_source.h"
#include "scenegraph.h"

namespace tbvh {

// layout codes as in include/tinybvh_amd.h (= BVHBase::BVHType, tiny_bvh.h:773-791); capi.hip checks they agree
constexpr int kLayoutBvhGpu = 5, kLayoutBvh4Gpu = 8, kLayoutCwbvh = 10;

void launch_bvh2(bool anyhit, int variant, const float4* nodes, const float4* tris, const QueryArgs& q, uint32_t* status,
                 uint32_t blocks, hipStream_t s);
void launch_bvh4(bool anyhit, int variant, const float4* data, const QueryArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s);
// nodeStride: 5 = `nodes` is the packed array; 8 = the copy with one node per 128-byte line (scenes whose nodes outgrow the Infinity
// Cache); 13 (cwbvh_node.h: kNodeHybrid) = the priority-ordered copy whose first q.hybridK nodes are packed and the others one per line
// the coherent flavor of a probed launch as ONE traversal per wave of 64 consecutive rays (kernels_cwbvh_packet.hip)
void launch_cwbvh_packet(bool anyhit, const float4* nodes, const float4* tris, const QueryArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s);
void launch_cwbvh(bool anyhit, int variant, const float4* nodes, const float4* tris, const QueryArgs& q, uint32_t* status,
                  uint32_t blocks, hipStream_t s, int nodeStride = 5, bool shallow = false, uint32_t blocks7 = 0xFFFFFFFFu);   // blocks7: grid of the kernels built for 7 waves per SIMD
// a scene in watertight mode (tbvh_set_triangle_test): q.wtVerts / q.wtTris are set; packed nodes and 48-byte records only
constexpr uint32_t kWatertightWavesPerSimd = 5;   // what the split-ray forms of those kernels are built for (kernels_cwbvh.hip): 20 one-wave workgroups per CU are resident
void launch_cwbvh_watertight(bool anyhit, const float4* nodes, const float4* tris, const QueryArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s);
void launch_cwbvh_derive_hybrid(const float4* src, const uint32_t* perm, float4* dst, uint32_t nNodes, uint32_t hybridK, const float4* tris, hipStream_t s);   // tris: the packed 48-byte records (one per node is embedded in its line), or nullptr
bool cwbvh_variant_valid(int variant);     // diagnostic variants of the BVH8_CWBVH kernel (tbvh_set_variant); the other layouts have none
void launch_cwbvh_pad(const float4* src, float4* dst, uint32_t nNodes, hipStream_t s);
void launch_cwbvh_pad_tris(const float4* src, float4* dst, uint64_t nTris, hipStream_t s);
struct BlasDesc { const float4* nodes; const float4* tris; const uint32_t* opmap; uint32_t opmapN; uint32_t layout; };  // one per BLAS of a TLAS (layout: TBVH_LAYOUT_*)
// ... of a TLAS over watertight BLASes (tbvh_set_triangle_test; kernels_tlas8.hip: WT): the same, then the BLAS's vertices (3 float4 per triangle in primitive
// order) and their count.  A table of its own type, so that BlasDesc and every kernel reading it stay what they were; it travels through the same pointer.
struct BlasDescWt { BlasDesc d; const float4* wtVerts; uint64_t wtTris; uint64_t pad[2]; };
static_assert(sizeof(BlasDesc) == 32 && sizeof(BlasDescWt) == 64, "a watertight descriptor is two plain ones wide");
void launch_tlas(bool anyhit, int blasLayout, const float4* tlasNodes, const uint32_t* tlasIdx, const float4* instances,
                 const BlasDesc* blas, const QueryArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s);
// 4-wide TLAS in the BVH4_GPU node format + the unified two-level kernel for BVH4_GPU BLASes (kernels_tlas4.hip)
size_t tlas_wide_scratch_bytes(uint64_t nAL, uint64_t nInst);   // kernels_tlaswide.hip builds both wide TLAS formats
uint64_t tlas4_cap_blocks(uint64_t nAL, uint64_t nInst);
void launch_tlas4_build(const float4* al, uint32_t nAL, const uint32_t* idx, uint32_t nIdx, const float4* inst, uint32_t nInst, float4* blocks, uint32_t capBlocks,
                        void* scratch, uint32_t* status, hipStream_t s);   // status |= 4 when the capacity does not hold the tree
void launch_tlas4(bool anyhit, int variant, const float4* tlas4, const float4* instances, const BlasDesc* blas, const QueryArgs& q, uint32_t* status, uint32_t blocks,
                  hipStream_t s, uint32_t blocks7);
// 8-wide TLAS in the BVH8_CWBVH node format + the unified two-level kernel for BVH8_CWBVH BLASes (kernels_tlas8.hip)
uint64_t tlas8_cap_nodes(uint64_t nAL, uint64_t nInst);
void launch_tlas8_build(const float4* al, uint32_t nAL, const uint32_t* idx, uint32_t nIdx, const float4* inst, uint32_t nInst, float4* nodes, uint32_t capNodes,
                        uint32_t* instRef, uint32_t capRefs, void* scratch, uint32_t* status, hipStream_t s);
void launch_tlas8(bool anyhit, int variant, const float4* tlasNodes, const uint32_t* instRef, const float4* instances, const BlasDesc* blas, const QueryArgs& q,
                  uint32_t* status, uint32_t blocks, hipStream_t s, uint32_t blocks7, bool mixed = false, bool watertight = false);   // watertight: blas is a BlasDescWt table
void launch_tlas2(bool anyhit, int variant, const float4* tlasNodes, const uint32_t* tlasIdx, const float4* instances, const BlasDesc* blas, const QueryArgs& q,
                  uint32_t* status, uint32_t blocks, hipStream_t s, uint32_t blocks7);   // BVH_GPU BLASes (kernels_tlas2.hip)
// BVH_Double scenes (kernels_double.hip; records as tinybvh defines them, tiny_bvh.h:733-761, 1035-1090, 1462-1474)
struct __attribute__((aligned(16))) RayExRec {   // tinybvh::RayEx, 128 bytes
    double O[3], D[3], rD[3];
    double t, u, v;
    uint64_t inst, prim, instIdx, mask;
};
static_assert(sizeof(RayExRec) == 128, "RayEx is 128 bytes");
struct NodeDbl { double mn[3], mx[3]; uint64_t leftFirst, triCount; };   // BVH_Double::BVHNode, 64 bytes
static_assert(sizeof(NodeDbl) == 64, "BVH_Double::BVHNode is 64 bytes");
struct TriDbl { double v0[3], e1[3], e2[3]; uint64_t prim; };             // gathered at upload: one per primIdx entry, 80 bytes
static_assert(sizeof(TriDbl) == 80, "double triangle record is 80 bytes");
struct InstanceDbl {                                                         // BLASInstanceEx, 320 bytes
    double transform[16], invTransform[16];
    double aabbMin[3]; uint64_t blasIdx;
    double aabbMax[3]; uint64_t mask;
};
static_assert(sizeof(InstanceDbl) == 320, "BLASInstanceEx is 320 bytes");
struct BlasDbl { const NodeDbl* nodes; const TriDbl* tris; };   // one per BLAS of a double TLAS
struct DoubleArgs {
    RayExRec* rays;
    uint64_t nRays;
    uint8_t* occluded;     // any-hit output, 1 byte per ray
    uint32_t* spill;       // stack spill area and its entries per lane
    uint32_t spillStride;
    uint32_t* counter;     // ray-pool counters of this launch / of the next one (ray_pool.h)
    uint32_t* counterNext;
    uint32_t poolParts;
    const NodeDbl* nodes;  // BLAS: its nodes and records; TLAS: the TLAS nodes, its instance indices, the instances and the BLASes
    const TriDbl* tris;
    const uint64_t* tlasIdx;
    const InstanceDbl* inst;
    const BlasDbl* blas;
};
// spheres: q.tris holds a sphere BLAS's records (custom_sphere_dbl.h); under a TLAS, the TLAS lists a sphere BLAS and the low bit of a BlasDbl's `tris` marks one
void launch_double(bool spheres, bool anyhit, bool tlas, const DoubleArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s);
void launch_gather_tris_dbl(const uint64_t* primIdx, const void* verts72, void* recs80, uint64_t nIdx, hipStream_t s);   // (the signature of the spheres' gather)
// BVH_Double scenes that move (kernels_double_anim.hip).  TLAS rebuild: BLASInstanceEx::Update of every instance (transformsDev: 16 doubles per instance, or
// nullptr: the transforms in the records; the BLAS boxes are node 0 of each BLAS), then an LBVH of 2 n - 1 nodes over the instance boxes into tlasNodes /
// tlasIdx.  The scratch is one allocation of tlas_dbl_build_scratch_bytes(n); host transforms are staged in its part tlas_dbl_xform_stage names.
size_t tlas_dbl_build_scratch_bytes(uint32_t n, size_t* sortTempBytes);
double* tlas_dbl_xform_stage(void* scratch, uint32_t n, size_t sortTempBytes);
hipError_t launch_tlas_dbl_rebuild(NodeDbl* tlasNodes, uint64_t* tlasIdx, InstanceDbl* instances, const BlasDbl* blas, uint64_t nBlas, const double* transformsDev,
                                   uint32_t n, void* scratch, size_t sortTempBytes, hipStream_t s);
// BLAS refit: parent[] and the leaf list of a tree (once per scene; nNodes entries each, frontA / frontB: nNodes entries of scratch), then per call the
// records and boxes from verts (9 doubles per triangle); flags: nNodes words, zeroed by the launcher
void launch_parents_dbl(const NodeDbl* nodes, uint32_t nNodes, uint32_t* parent, uint32_t* leaves, uint32_t* frontA, uint32_t* frontB, uint32_t* nLeavesOut, hipStream_t s);
hipError_t launch_refit_dbl(NodeDbl* nodes, uint32_t nNodes, TriDbl* tris, uint64_t nRecs, const double* verts, uint64_t nTris, const uint32_t* leaves,
                            uint32_t nLeaves, const uint32_t* parent, uint32_t* flags, hipStream_t s);
// BVH_Double over custom geometry: spheres {pos, r} of 32 bytes, gathered into 48-byte records {pos, r, prim, 0} (custom_sphere_dbl.h).  Queries are
// launch_double's sphere forms; the upload's gather stands beside the triangles' in kernels_double.hip.
// The build is kernels_double_anim.hip's LBVH with the spheres as its box source: 2 n - 1 nodes over the boxes pos -/+ r into nodes / recs48 (a record
// carries its primIdx entry); the scratch is one allocation of spheres_dbl_build_scratch_bytes(n).
void launch_gather_spheres_dbl(const uint64_t* primIdx, const void* spheres32, void* recs48, uint64_t nIdx, hipStream_t s);
size_t spheres_dbl_build_scratch_bytes(uint32_t n, size_t* sortTempBytes);
hipError_t launch_spheres_dbl_build(NodeDbl* nodes, void* recs48, const void* spheres32, uint32_t n, void* scratch, size_t sortTempBytes,
                                    hipStream_t s);

// VoxelSet scenes (kernels_voxel.hip): vox = one set's [top grid 16 | grid 32768 | bricks] words; tlasNodes != nullptr: a BVH_GPU-format TLAS over
// BLASInstance records whose BLASes are all voxel sets (BlasDesc::nodes = each set's array)
void launch_voxel(bool anyhit, const uint32_t* vox, const float4* tlasNodes, const uint32_t* tlasIdx, const float4* instances, const BlasDesc* blas,
                  const QueryArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s);

// BVH::IntersectSphere batched (kernels_sphere.hip): hit[i] = 1 if sphere i = {x, y, z, r} touches a triangle of a BVH_GPU / BVH4_GPU / BVH8_CWBVH
// BLAS; verts = the caller's vertex array (3 float4 per triangle, nTris triangles), indexed by the primitive index of each triangle record
struct SphereArgs {
    const float4* spheres;   // device, 16 bytes per sphere
    uint64_t nSpheres;
    uint8_t* hit;            // device, 1 byte per sphere
    const float4* nodes;     // the scene's node array (BVH4_GPU: the stream, triangles inline)
    const float4* tris;      // BVH_GPU / BVH8_CWBVH triangle records
    MeshSrc verts;           // the caller's vertices (mesh_source.h); verts.nTris triangles
    uint32_t* spill;         // stack spill area (8-byte entries)
    uint32_t spillStride;    // 8-byte entries per lane in `spill`
    uint32_t* counter;       // ray-pool counters of this launch and of the next one (ray_pool.h)
    uint32_t* counterNext;
    uint32_t poolParts;
};
void launch_spheres(int layout, const SphereArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s);   // status |= 16: a record's primitive is beyond nTris

// custom-geometry sphere BLASes (kernels_custom.hip, custom_sphere.h): nodes = the Wald nodes (32 bytes: 2 float4 each), recs = the spheres gathered
// in primIdx order, 2 float4 each ({x, y, z, r}, {prim, 0, 0, 0})
void launch_custom(bool anyhit, const float4* nodes, const float4* recs, const QueryArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s);
// TLASes with sphere BLASes (kernels_tlas.hip: the flat loop with the sphere step): blasLayout = TBVH_LAYOUT_BVH2_WALD when every BLAS is a sphere
// BLAS, 0 when they mix with BVH_GPU / BVH4_GPU / BVH8_CWBVH BLASes (BlasDesc::layout per BLAS: nodes = Wald nodes, tris = sphere records)
void launch_tlas_custom(bool anyhit, int blasLayout, const float4* tlasNodes, const uint32_t* tlasIdx, const float4* instances,
                        const BlasDesc* blas, const QueryArgs& q, uint32_t* status, uint32_t blocks, hipStream_t s);

// ---- what the LBVH builders' launchers share (the kernels' shared core is lbvh.h) ----
// the centre bounds before a build: three minima at the ordered encoding's largest value, three maxima at its smallest; wordBytes: 4 (float) or 8
inline hipError_t reset_centre_bounds(void* bounds, size_t wordBytes, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(bounds, 0xff, 3 * wordBytes, s);
    return e != hipSuccess ? e : hipMemsetAsync((char*)bounds + 3 * wordBytes, 0x00, 3 * wordBytes, s);
}
// after a launch of a rebuild `who`: names the step that failed and returns its error (the caller declares hipError_t e)
#define TBVH_STEP(who, what) do { if ((e = hipGetLastError()) != hipSuccess) { fprintf(stderr, "[tinybvh_amd] %s: %s: %s\n", who, what, hipGetErrorString(e)); return e; } } while (0)
// the size of each builder's scratch allocation given hipcub's temporary sizes: no device needed (the *_scratch_bytes below ask hipcub first);
// sah_scratch_total and sbvh_scratch_total are in sahbuild.h and sbvhbuild.h
size_t lbvh_scratch_total(uint32_t n, size_t sortTempBytes);
size_t ploc_scratch_total(uint32_t n, size_t sortTempBytes, size_t scanTempBytes);
size_t tlas_build_scratch_total(uint32_t n, size_t sortTempBytes);
size_t tlas_dbl_build_scratch_total(uint32_t n, size_t sortTempBytes);

// device TLAS rebuild (kernels_tlasbuild.hip)
size_t tlas_build_scratch_bytes(uint32_t n, size_t* sortTempBytes);
hipError_t launch_tlas_instance_update(float4* instances, const float* transformsDev, const float* blasBoundsDev, uint32_t n, uint32_t nBlas, void* scratch,
                                       size_t sortTempBytes, hipStream_t s);   // the first step of launch_tlas_rebuild alone
hipError_t launch_tlas_rebuild(float4* tlasNodes, uint32_t* tlasIdx, float4* instances, const float* transformsDev, const float* blasBoundsDev,
                               uint32_t n, uint32_t nBlas, void* scratch, size_t sortTempBytes, hipStream_t s);
// LBVH build on the device (kernels_build.hip)
size_t lbvh_scratch_bytes(uint32_t n, size_t* sortTempBytes);
size_t ploc_scratch_bytes(uint32_t n, size_t* sortTempBytes, size_t* scanTempBytes);
hipError_t launch_ploc_build(const MeshSrc& verts, uint32_t n, uint32_t radius, float4* nodes32, uint32_t* primIdx, void* scratch, size_t sortTempBytes,
                             size_t scanTempBytes, hipStream_t s, uint32_t* steps, const float4* spheres = nullptr);
hipError_t launch_lbvh_build(const MeshSrc& verts, uint32_t n, uint32_t maxLeaf, float4* nodes32, uint32_t* primIdx, void* scratch, size_t sortTempBytes,
                             hipStream_t s, const float4* spheres = nullptr);   // spheres: the box source is {x, y, z, r} x n (capi_custom.hip), verts is not read
// custom-geometry sphere BLASes that move (kernels_custom_build.hip): the record gather after a build, and the refit of a Wald tree over sphere records
void launch_gather_sphere_records(const uint32_t* primIdx, const float4* spheres, float4* recs, uint32_t n, hipStream_t s);
hipError_t launch_refit_spheres(float4* nodes32, uint32_t nNodes, float4* recs, uint64_t nRecs, const float4* spheres, uint64_t nSpheres, uint32_t* done,
                                hipStream_t s);
// BVH2 -> CWBVH conversion on the device (kernels_convert.hip)
hipError_t run_convert_cwbvh(const float4* nodes2, uint32_t nNodes2, const uint32_t* primIdx, uint64_t nIdx, const MeshSrc& verts,
                             float4* cwNodes, uint32_t capNodes, float4* cwTris, uint64_t capTris, uint2* itemsA, uint2* itemsB, uint32_t* counters,
                             uint32_t* status, hipStream_t s, uint32_t* nNodesOut, uint64_t* nTrisOut, uint32_t* levelsOut);
hipError_t run_convert_bvh4(const float4* nodes2, uint32_t nNodes2, const uint32_t* primIdx, uint64_t nIdx, const MeshSrc& verts,
                            float4* blocks, uint64_t capBlocks, uint2* itemsA, uint2* itemsB, uint32_t* counters, uint32_t* status, hipStream_t s,
                            uint64_t* nBlocksOut, uint32_t* levelsOut);
// device BLAS refit (kernels_refit.hip)
hipError_t run_refit_bvh4(float4* blocks, uint64_t nBlocks, const MeshSrc& verts, void* itemsDev, uint32_t capNodes, uint32_t* counterDev,
                          float4* childBox, std::vector<uint32_t>& levelFirst, uint32_t* status, hipStream_t s);
size_t refit_scratch_bytes(int layout, uint32_t nNodes);
hipError_t launch_refit(int layout, float4* nodes, uint32_t nNodes, float4* tris, uint64_t nTriRecords, const MeshSrc& verts,
                        void* scratch, uint32_t* status, hipStream_t s);
void launch_stream_copy(const float4* src, float4* dst, uint64_t n16, hipStream_t s);
void launch_stream_read(const float4* src, float* sink, uint64_t n16, uint32_t blocks, hipStream_t s);
void launch_valu_mix(float* out, int iters, uint32_t blocks, hipStream_t s);   // 32 VALU instructions per iteration and wave
void launch_pack_hits(const RayRec* rays, uint32_t* out, uint64_t n, hipStream_t s);
// (kernels_mesh.hip) every kernel that reads vertices takes a MeshSrc (mesh_source.h): flat 3 x float4 per triangle, or indexed / strided
void launch_gather_tris(const uint32_t* primIdx, const MeshSrc& verts, float4* out, uint64_t nIdx, uint32_t* status, hipStream_t s);
void launch_flatten_mesh(const MeshSrc& verts, float4* out, uint32_t* status, hipStream_t s);   // 3 float4 per triangle, in triangle order
// (kernels_pose.hip) Mesh::SetPose on the device, one vertex per lane through pose.h: skin (rest16, joints4, weights16: one float4 / uint4 per vertex;
// mats: 4 float4 per joint; a vertex with a joint index >= nJoints is left unwritten and status |= kStatusPoseJoint) and morph (positions12: nTargets + 1
// arrays of nVerts * 3 floats)
constexpr uint32_t kStatusPoseJoint = 64u;
void launch_pose_skin(const float4* rest16, const uint4* joints4, const float4* weights16, const float4* mats, uint32_t nJoints, float4* out, uint64_t nVerts,
                      uint32_t* status, hipStream_t s);
void launch_pose_morph(const float* positions12, const float* weights, uint32_t nTargets, float4* out, uint64_t nVerts, hipStream_t s);
// ... and for a pose with FatTri records attached: the same vertices plus one posed normal per vertex, then the records' vertex0..2, vN0..2 and (skin) Nx Ny Nz
void launch_pose_skin_normals(const float4* rest16, const uint4* joints4, const float4* weights16, const float4* mats, uint32_t nJoints, const float* normals12, float4* out,
                              float4* nOut, uint64_t nVerts, uint32_t* status, hipStream_t s);
void launch_pose_morph_normals(const float* positions12, const float* weights, uint32_t nTargets, const float* normals12, float4* out, float4* nOut, uint64_t nVerts,
                               hipStream_t s);
void launch_pose_fat_tris(float4* tris, uint64_t nTris, const float4* verts, const float4* normals, uint64_t nVerts, const uint32_t* indices, bool skin, uint32_t* status,
                          hipStream_t s);   // a corner index >= nVerts: the triangle is left, kStatusMeshIndex (mesh_source.h) is raised
// (kernels_omm.hip) Mesh::CreateOpacityMicroMaps on the device, one wave per triangle through omm.h: src with every pointer (the texture descriptors and
// the texels they name included) in device memory; out: nTris * ((N * N + 31) / 32) words; N a power of two from 1 to 64.  A corner index >= nUV is clamped,
// a texture index >= nTextures that is not the no-texture mark means no texture, and status |= kStatusOmmIndex for either.  maxBlocks: the grid's cap.
constexpr uint32_t kStatusOmmIndex = 128u;
struct OmmSrc;
void launch_omm_bake(const OmmSrc& src, uint32_t N, uint32_t* out, uint32_t* status, uint32_t maxBlocks, hipStream_t s);
// (kernels_shade.hip) GetShadingData on the device, one hit record per lane through shade.h: 48 bytes out per record; an inst / slot / prim / material /
// texture index that is out of range is never used as an address and sets kStatusShade.  launch_shade_continue: the alpha-continue step (records whose
// out48 alpha is 0 step on; how many did is ADDED to *nContinued when that is not null)
constexpr uint32_t kStatusShade = 256u;
struct ShadeTables;
// nDev: null, or the record count in device memory (a queue filled on the device: at most n records, the grid is sized for n)
void launch_shade_hits(const ShadeTables& tb, const float4* instances, uint64_t nInst, const uint32_t* blasLayout, uint32_t blasStride, uint32_t nBlas, const void* rays,
                       uint64_t n, uint32_t strideBytes, void* out48, uint32_t* status, hipStream_t s, const unsigned long long* nDev = nullptr);
void launch_shade_continue(void* rays, uint32_t strideBytes, const void* out48, uint64_t n, unsigned long long* nContinued, hipStream_t s);
// (kernels_viewer.hip) a viewer frame lit and finished on the device, one pixel per lane through viewer.h: WorkerThread's row-major generator, SampleSky, the
// alpha loop's queue (compact: round 0's masked records, stepped on, with their pixel; requeue: over the device-side count, masked again -> the next queue,
// everything else scattered back to its pixel; cap = the frame's pixel count bounds every slot and pixel index), the foliage viewer's shadow rays (*nReal += the
// rays that are not null), the light of either mode with its sky gather, and the pack to 0x00BBGGRR
struct ViewerCam;
struct ViewerSky;
struct ShadeMat;
void launch_viewer_generate(const ViewerCam& cam, void* rays64, uint64_t first, uint64_t n, hipStream_t s);
void launch_sky_sample(const ViewerSky& sky, const void* dirs16, uint64_t n, void* out16, hipStream_t s);
void launch_viewer_compact(const void* rays64, const void* out48, uint64_t n, const ShadeMat* mats, uint32_t nMats, uint32_t nTex, void* qRays64, uint32_t* qPix,
                           unsigned long long* qCount, hipStream_t s);
void launch_viewer_requeue(const void* qRays64, const uint32_t* qPix, const void* qOut48, const unsigned long long* qCount, uint64_t cap, const ShadeMat* mats, uint32_t nMats,
                           uint32_t nTex, bool lastRound, void* nextRays64, uint32_t* nextPix, unsigned long long* nextCount, void* rays64, void* out48, hipStream_t s);
void launch_viewer_shadow_rays(const void* rays, uint32_t strideBytes, uint64_t n, const float L[3], void* shadow64, unsigned long long* nReal, hipStream_t s);
void launch_viewer_light(uint32_t mode, const ViewerSky& sky, const void* rays, uint32_t strideBytes, const void* out48, const uint8_t* occ, uint64_t n, const float L[3],
                         void* rgb16, hipStream_t s);
void launch_viewer_pack(const void* rgb16, uint64_t n, uint32_t* pixels, hipStream_t s);
// (kernels_voxel_edit.hip) the batched VoxelSet::Set in deterministic passes over records { x, y, z, v } (voxel_edit.h), vox = the set's one allocation:
//   mark   — work.cellFirst[g] = the smallest record index touching a grid cell g that has no brick; counters[0] = such cells, [1] = records out of range (skipped
//            by every pass); the launch resets the work area first
//   number — the marked cells sorted by that index: grid[cell of rank r] = used + r (nNew of them; the caller has read counters[0] and zeroed the bricks)
//   winner — winner[brick * 512 + voxel] = 1 + the largest record index writing that voxel
//   store  — the record that is its voxel's winner stores v and clears the winner word: the words are all zero again afterwards
// launch_voxel_top_grid is UpdateTopGrid (512 lanes, one top cell each); launch_voxel_normals GetNormal per hit record (voxel_edit.h: voxel_normal_record)
struct VoxelEditWork {
    uint32_t *cellFirst, *cellIds, *sortedFirst, *sortedCells;   // 32768 words each
    uint32_t* counters;                                          // 64 words
    void* sortTemp;
    size_t sortTempBytes;
};
size_t voxel_edit_work_words(size_t* sortTempBytes);             // the work area's size in uint32 words
VoxelEditWork voxel_edit_work(uint32_t* base, size_t sortTempBytes);
void launch_voxel_mark(const uint32_t* vox, const uint4* recs, uint64_t n, const VoxelEditWork& w, hipStream_t s);
hipError_t launch_voxel_number(uint32_t* vox, const VoxelEditWork& w, uint32_t used, uint32_t nNew, hipStream_t s);
void launch_voxel_winner(const uint32_t* vox, const uint4* recs, uint64_t n, uint32_t* winner, hipStream_t s);
void launch_voxel_store(uint32_t* vox, const uint4* recs, uint64_t n, uint32_t* winner, hipStream_t s);
void launch_voxel_top_grid(uint32_t* vox, hipStream_t s);
// ... and the scene-to-voxels loop (tiny_bvh_foliage.cpp:222-258).  launch_voxelize_rays: the 3 x 256^2 axis rays, ids and hit numbers (0).  launch_voxelize_step:
// one round after trace (and shade: out48, or nullptr for the constant colour) over n live rays — a ray without a hit below 10000 ends, one with maxHits hits
// behind it is cut (counters[2]), a hit with alpha != 0 appends a record { x, y, z, v } and its key id << 32 | hit number (counters[1], never reset: the
// records of all rounds), and the ray, advanced, goes to the next round's arrays (counters[0]).  launch_voxelize_sort: the records in key order.
struct VoxelizeArgs;
void launch_voxelize_rays(const VoxelizeArgs& p, RayRec* rays, uint32_t* ids, uint32_t* hitNo, hipStream_t s);
void launch_voxelize_step(const VoxelizeArgs& p, const RayRec* rays, const uint32_t* ids, const uint32_t* hitNo, const float4* out48, uint64_t n, RayRec* raysOut,
                          uint32_t* idsOut, uint32_t* hitNoOut, unsigned long long* keys, uint4* recs, uint32_t* counters, hipStream_t s);
size_t voxelize_sort_temp_bytes(uint64_t n);
hipError_t launch_voxelize_sort(const unsigned long long* keys, unsigned long long* keysOut, uint32_t* order, uint32_t* orderOut, const uint4* recs, uint4* recsOut,
                                uint64_t n, void* temp, size_t tempBytes, hipStream_t s);
void launch_voxel_normals(const float4* instances, uint64_t nInst, const void* rays, uint32_t strideBytes, uint64_t n, float4* out, uint32_t* status, hipStream_t s);

// ray generators (kernels_raygen.hip)
struct CameraArgs {
    float eye[3], p1[3], p2[3], p3[3];
    uint32_t width, height, sppX, sppY;
};
void launch_gen_primary(const CameraArgs& cam, RayRec* rays, uint64_t first, uint64_t n, hipStream_t s);
// triangle fetch mode for the bounce generator: how to find the geometric normal of prim p
struct TriSource {
    int mode;              // 0: verts (3 float4 per prim, original order); 1: none
    const float4* verts;
};
void launch_gen_bounce(const TriSource& src, const RayRec* in, RayRec* out, uint64_t n, uint32_t seed, hipStream_t s);
void launch_reset_hits(RayRec* rays, uint64_t n, float tmax, hipStream_t s);
void launch_gen_shadow(const RayRec* in, RayRec* out, uint64_t n, float lx, float ly, float lz, float eps, hipStream_t s);

// ray binning (kernels_raybin.hip): counting sort of a batch by (Morton code of the origin's cell, direction octant)
struct RayBinArgs {
    float lo[3], scale[3];   // cell = (O - lo) * scale, clamped to [0, 2^cellBits)
    uint32_t cellBits;       // 0..6 bits per axis
    uint32_t flags;          // 1: octant as the minor part of the key, 2: as the major part, 0: cell only
};
uint32_t ray_bin_count(uint32_t cellBits, uint32_t flags);
size_t ray_bin_scratch_bytes(uint64_t n, uint32_t cellBits, uint32_t flags, size_t* scanTempBytes);
hipError_t launch_ray_bin(const RayRec* in, RayRec* out, uint32_t* perm, uint64_t n, const unsigned long long* nDev, const RayBinArgs& a, void* scratch,
                          size_t scanTempBytes, uint32_t blocks, hipStream_t s);

// wavefront path tracer stages (kernels_wavefront.hip)
struct PathAux { float T[3]; uint32_t pixel; };   // throughput + pixel << 8 | depth << 4 | path flags (paths), or pending contribution + pixel (shadow rays); 16 bytes
struct ShadeArgs {
    const RayRec* in; const PathAux* auxIn; const unsigned long long* nIn;
    RayRec* out; PathAux* auxOut; unsigned long long* nOut;
    RayRec* shadow; PathAux* shadowAux; unsigned long long* nShadow;
    const float4* verts; float* accum;
    const float4* const* blasVerts; const float4* instances;   // TLAS scenes: vertex array per BLAS, BLASInstance records (else nullptr)
    float lightPos[3], lightColor[3], skyLo[3], skyHi[3];
    float lightSize[2];   // extent of the rectangular light along x and z (0, 0 = point light)
    float eps; uint32_t depth, maxDepth, seed, flags;   // flags bit 0: at most one diffuse bounce per path (wavefront.cl:233); bit 1: wavefront.cl to the letter
    const uint32_t* blueNoise; uint32_t sampleIdx, width, height;   // 128 x 128 x 8 table (or nullptr), the frame's sample index, size of the FULL image
    uint32_t pixelOffset;   // a band of a larger image (tbvh_wavefront_set_band): index of the band's first pixel in the full image (else 0)
};
void launch_wf_generate(const CameraArgs& cam, RayRec* rays, PathAux* aux, uint64_t n, uint32_t seed, uint32_t firstRow, uint32_t bandRows, unsigned long long* queueCounters,
                        uint32_t nCounterWords, hipStream_t s);
void launch_wf_shade(const ShadeArgs& a, uint64_t capacity, hipStream_t s);
void launch_wf_finalize(const float* accum, float scale, uint32_t* pixels, uint64_t n, hipStream_t s);
void launch_wf_connect(const uint8_t* occ, const PathAux* aux, const unsigned long long* nShadow, float* accum, uint64_t capacity, hipStream_t s);

// kernels_scenegraph.hip: the animated scene graph (tbvh_scenegraph_*; scenegraph.h holds the arithmetic and kStatusGraph).  One work item per lane, exact grids.
// launch_graph_sample: channels [c0, c1) advance by dt and write their node's T, R, S or weights unless (flags & shadowMask).  launch_graph_walk: the three kernels
// of one walk (local transforms of written nodes; combined transforms down each node's own ancestor chain; instance transforms and joint matrices).
void launch_graph_sample(const SgView& g, uint32_t c0, uint32_t c1, float dt, uint32_t shadowMask, hipStream_t s);
void launch_graph_walk(const SgView& g, int only, hipStream_t s);   // only: -1 all, 1 local, 2 combine, 3 outputs
void launch_graph_set_time(float* cT, int32_t* cK, uint32_t c0, uint32_t c1, float t, hipStream_t s);
struct SgMat { float m[16]; };
void launch_graph_set_local(float* local, uint32_t node, const SgMat& m, hipStream_t s);   // (the matrix travels as a kernel argument: nothing of the caller's is read after the call)

}  // namespace tbvh
