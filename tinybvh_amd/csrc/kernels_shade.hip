// kernels_shade.hip — GetShadingData on the device (tbvh_shade_hits / _device): one hit record per lane, the arithmetic of shade.h, no LDS.
//   k_shade_hits     per ray: float4 1..3 of the record (D; the quarter that ends in hit.inst; t u v prim), consecutive lanes one stride apart; a wave
//                    whose 64 lanes all missed writes its "no surface" records and leaves there.  A hit then gathers: three rows of its instance's
//                    transform and the blasIdx dword, the slot's descriptor, five quarters of its FatTri (UVs + material, the three vertex normals
//                    with the geometric normal in their w), the 20-byte material, and per texture one descriptor and one texel, all addressed per
//                    lane; the T / B quarters only under a normal map.  Every one of these is WRITTEN as a 16-byte load (shade.h); the compiler narrows
//                    a load whose last components nothing reads and drops the FatTri's three vertex quarters, of which the shading reads nothing: the
//                    ISA has 4 global_load_dwordx4, 4 dwordx3, 2 dwordx2, 4 dwords and — through the pointers read from the tables — 4 flat_load_dwordx4, 3 dwordx3, 2 dwords.  Output: three 16-byte stores per lane, consecutive
//                    lanes 48 bytes apart.
//                    Every index is compared with its table's size before it becomes an address (shade.h: shade_hit); a bad one sets kStatusShade
//                    with a vector atomic, once per wave.  nDev (optional): the record count in device memory, for a queue filled on the device.
//   k_shade_continue the alpha-continue step of the reference's renderers (tiny_bvh_gltf.cpp:140-150): a record whose shading came back with alpha == 0
//                    steps on — O = ( O + D * t ) + D * 1e-4, every product and sum rounded, hit.t = 1e30, u v prim cleared — and is ready for the next
//                    tbvh_intersect_device; every other record is left as it is (traced again it keeps its hit: nothing closer is recorded twice).
//                    The number of records that stepped on is added to a device counter, one atomic per wave.
#include "device_common.h"
#include "kernels.h"
#include "shade.h"

namespace tbvh {

namespace {

constexpr uint32_t kShadeBlock = 256;

__global__ __launch_bounds__(kShadeBlock) void k_shade_hits(ShadeTables tb, const float4* __restrict__ instances, uint64_t nInst, const uint32_t* __restrict__ blasLayout,
                                                            uint32_t blasStride, uint32_t nBlas, const char* __restrict__ rays, uint64_t n, uint32_t strideBytes,
                                                            float4* __restrict__ out, uint32_t* __restrict__ status, const unsigned long long* __restrict__ nDev) {
    const uint64_t i = (uint64_t)blockIdx.x * kShadeBlock + threadIdx.x;
    const bool live = i < (nDev && *nDev < n ? *nDev : n);   // (a queue filled on the device: its count, never beyond the n the grid was sized for)
    float4 r1 = make_float4(0.f, 0.f, 0.f, 0.f), r2 = r1, r3 = make_float4(1e30f, 0.f, 0.f, 0.f);
    if (live) {
        const float4* rec = (const float4*)(rays + i * strideBytes);
        r1 = rec[1]; r2 = rec[2]; r3 = rec[3];
    }
    float4 o[3];
    bool ok = true;
    if (__ballot(live && !(r3.x >= 1e30f)) == 0ull) shade_no_surface(o);   // the whole wave missed
    else ok = shade_hit(tb, instances, nInst, blasLayout, blasStride, nBlas, r1, __float_as_uint(r2.w), r3, o);
    if (live) {
        float4* dst = out + 3 * i;
        dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    }
    const unsigned long long bad = __ballot(live && !ok);
    if (bad && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)bad) - 1u) atomicOr(status, kStatusShade);
}

__global__ __launch_bounds__(kShadeBlock) void k_shade_continue(char* __restrict__ rays, uint32_t strideBytes, const float4* __restrict__ out48, uint64_t n,
                                                                unsigned long long* __restrict__ nContinued) {
    const uint64_t i = (uint64_t)blockIdx.x * kShadeBlock + threadIdx.x;
    bool go = false;
    if (i < n) {
        go = out48[3 * i].w == 0.f;
        if (go) {
            float4* rec = (float4*)(rays + i * strideBytes);
            float4 O = rec[0];
            const float4 D = rec[1];
            const float t = rec[3].x;
            O.x = (O.x + D.x * t) + D.x * 0.0001f;
            O.y = (O.y + D.y * t) + D.y * 0.0001f;
            O.z = (O.z + D.z * t) + D.z * 0.0001f;
            rec[0] = O;
            rec[3] = make_float4(1e30f, 0.f, 0.f, 0.f);
        }
    }
    if (nContinued) {
        const unsigned long long m = __ballot(go);
        if (m && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(nContinued, (unsigned long long)__popcll(m));
    }
}

}  // namespace

void launch_shade_hits(const ShadeTables& tb, const float4* instances, uint64_t nInst, const uint32_t* blasLayout, uint32_t blasStride, uint32_t nBlas, const void* rays,
                       uint64_t n, uint32_t strideBytes, void* out48, uint32_t* status, hipStream_t s, const unsigned long long* nDev) {
    if (!n) return;
    const dim3 grid((uint32_t)((n + kShadeBlock - 1) / kShadeBlock));
    hipLaunchKernelGGL(k_shade_hits, grid, dim3(kShadeBlock), 0, s, tb, instances, nInst, blasLayout, blasStride, nBlas, (const char*)rays, n, strideBytes, (float4*)out48,
                       status, nDev);
}

void launch_shade_continue(void* rays, uint32_t strideBytes, const void* out48, uint64_t n, unsigned long long* nContinued, hipStream_t s) {
    if (!n) return;
    const dim3 grid((uint32_t)((n + kShadeBlock - 1) / kShadeBlock));
    hipLaunchKernelGGL(k_shade_continue, grid, dim3(kShadeBlock), 0, s, (char*)rays, strideBytes, (const float4*)out48, n, nContinued);
}

}  // namespace tbvh
