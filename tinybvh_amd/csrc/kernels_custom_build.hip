// kernels_custom_build.hip — custom-geometry sphere BLASes that move (capi_custom.hip: tbvh_build_device_custom_spheres,
// tbvh_rebuild_custom_spheres_device, tbvh_refit_custom_spheres): the record gather that follows a device build (kernels_build.hip with
// k_sphere_boxes as its box source), and the refit of a Wald tree over sphere records.
//
// Refit = BVH::Refit (tiny_bvh.h:3087-3090) for spheres: a leaf's box is the min of pos - r / the max of pos + r over its records, an interior
// box the min / max of its two children, the root included (a TLAS reads the root box as the BLAS bounds).  The tree may be an uploaded one:
// children need not be numbered after their parents, and nodes the root never reaches may hold anything.  So, as k_wald_pass (kernels_build.hip)
// and for its reasons — no device-scope fence, no waiting between workgroups —:
//   pass 1      one thread per node record: a leaf re-gathers its records through the primitive index each carries, writes its box, done = 1;
//   pass p > 1  one thread per node that is not done: if both children were done BEFORE this pass (kernel boundaries make them visible), take
//               the min / max, write the box, done = p.
// A node at height h completes in pass h + 1.  Every index read from a node is checked against the array before it is used, and only the root's
// done word is waited for: a node the root does not reach can neither be indexed out of range nor hold the loop up.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "kernels.h"
#include "sah_split.h"

namespace tbvh {

namespace {

// one thread per primIdx entry: {sphere}, {prim, 0, 0, 0}, what tbvh_upload_custom_spheres gathers on the host
__global__ void k_gather_sphere_records(const uint32_t* __restrict__ primIdx, const float4* __restrict__ spheres, float4* __restrict__ recs, uint32_t n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t prim = primIdx[k];
    recs[2 * (size_t)k] = spheres[prim];
    recs[2 * (size_t)k + 1] = make_float4(as_f32(prim), 0.f, 0.f, 0.f);
}

__global__ void k_sphere_refit_leaves(float4* __restrict__ nodes32, uint32_t nNodes, float4* __restrict__ recs, uint64_t nRecs,
                                      const float4* __restrict__ spheres, uint64_t nSpheres, uint32_t* __restrict__ done) {
    const uint32_t node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= nNodes) return;
    float4* o = nodes32 + 2 * (size_t)node;
    const uint32_t first = as_u32(o[0].w), count = as_u32(o[1].w);
    if (count == 0u) { done[node] = 0u; return; }                                  // interior: the passes
    if ((uint64_t)first + count > nRecs) { done[node] = 0u; return; }               // (only a node the root does not reach: never done, never read)
    float3 mn = make_float3(0.f, 0.f, 0.f), mx = mn;
    bool any = false;
    for (uint32_t k = 0; k < count; k++) {
        float4* r = recs + 2 * ((size_t)first + k);
        const uint32_t prim = as_u32(r[1].x);
        if (prim >= nSpheres) continue;
        const float4 p = spheres[prim];
        r[0] = p;
        const float s4[4] = {p.x, p.y, p.z, p.w};
        float bl[3], bh[3];
        sah::sphere_box(s4, bl, bh);   // (sah_split.h: the box the builders gave this sphere, bit for bit)
        const float3 lo = make_float3(bl[0], bl[1], bl[2]), hi = make_float3(bh[0], bh[1], bh[2]);
        mn = any ? make_float3(fminf(mn.x, lo.x), fminf(mn.y, lo.y), fminf(mn.z, lo.z)) : lo;
        mx = any ? make_float3(fmaxf(mx.x, hi.x), fmaxf(mx.y, hi.y), fmaxf(mx.z, hi.z)) : hi;
        any = true;
    }
    if (any) { o[0] = make_float4(mn.x, mn.y, mn.z, as_f32(first)); o[1] = make_float4(mx.x, mx.y, mx.z, as_f32(count)); }
    done[node] = 1u;
}

__global__ void k_sphere_refit_pass(float4* __restrict__ nodes32, uint32_t nNodes, uint32_t* __restrict__ done, uint32_t pass) {
    const uint32_t node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= nNodes) return;
    if (done[node]) return;
    float4* o = nodes32 + 2 * (size_t)node;
    const uint32_t left = as_u32(o[0].w);
    if (as_u32(o[1].w) != 0u || (uint64_t)left + 1u >= nNodes) return;              // (a leaf beyond the records, a child pair beyond the array: unreachable)
    const uint32_t dl = done[left], dr = done[left + 1u];
    if (dl == 0u || dr == 0u || dl >= pass || dr >= pass) return;                  // both children finished in an EARLIER pass
    const float4* c = nodes32 + 2 * (size_t)left;
    const float4 lmn = c[0], lmx = c[1], rmn = c[2], rmx = c[3];
    o[0] = make_float4(fminf(lmn.x, rmn.x), fminf(lmn.y, rmn.y), fminf(lmn.z, rmn.z), as_f32(left));
    o[1] = make_float4(fmaxf(lmx.x, rmx.x), fmaxf(lmx.y, rmx.y), fmaxf(lmx.z, rmx.z), as_f32(0u));
    done[node] = pass;
}

}  // namespace

void launch_gather_sphere_records(const uint32_t* primIdx, const float4* spheres, float4* recs, uint32_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_sphere_records, dim3((n + 255u) / 256u), dim3(256), 0, s, primIdx, spheres, recs, n);
}

// nodes32: nNodes Wald nodes; recs: nRecs sphere records (2 float4 each); spheres: {x, y, z, r} x nSpheres by primitive index (device); done: nNodes
// words of scratch.  Synchronizes the stream once per batch of passes (a 4-byte read-back of the root's word).
hipError_t launch_refit_spheres(float4* nodes32, uint32_t nNodes, float4* recs, uint64_t nRecs, const float4* spheres, uint64_t nSpheres, uint32_t* done,
                                hipStream_t s) {
    const uint32_t bs = 256, nb = (nNodes + bs - 1) / bs;
    hipLaunchKernelGGL(k_sphere_refit_leaves, dim3(nb), dim3(bs), 0, s, nodes32, nNodes, recs, nRecs, spheres, nSpheres, done);
    hipError_t e;
    uint32_t pass = 2, rootDone = 0;
    if (nNodes < 3u) return hipGetLastError();   // the root is the only node: a leaf
    while (!rootDone) {
        for (int k = 0; k < 24; k++, pass++) hipLaunchKernelGGL(k_sphere_refit_pass, dim3(nb), dim3(bs), 0, s, nodes32, nNodes, done, pass);
        if ((e = hipMemcpyAsync(&rootDone, done, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
        if (pass > nNodes + 26u) return hipErrorUnknown;   // (a tree of nNodes nodes is at most that high: the root is not the root of a tree)
    }
    return hipGetLastError();
}

}  // namespace tbvh
