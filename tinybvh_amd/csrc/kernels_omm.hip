// kernels_omm.hip — Mesh::CreateOpacityMicroMaps on the device (tbvh_bake_opacity_micromaps): the arithmetic of omm.h, one wave per triangle.
//   k_omm_bake   a 64-thread workgroup (one wave) takes triangles in a grid-stride loop.  The triangle's words (at most 128, N = 64) live in LDS, zeroed —
//                or set to all ones for a triangle without a texture, which then skips the sampling.  The (4N - 1) * 2N samples are walked as the rectangle
//                of omm_sample_xy, 2N lines of 4N: consecutive LANES take consecutive LINES of one column, so the lanes of one instruction sit in different
//                sample rows, their bits in different words, and the LDS OR atomics that merge them hit different addresses (lanes along one row would pile
//                onto one or two words).  Many samples share a bit; OR does not care about order, so the words do not depend on scheduling.  Per sample:
//                ~30 VALU operations, one texel gathered through the ordinary cache path (the samples of an instruction lie on a line in texture space),
//                one LDS atomic when the texel is opaque.  Then the wave writes its words with coalesced dword stores.
//                Small N: 8 N^2 places are fewer than 64 for N = 1 and 2, so a wave takes 8 resp. 2 triangles at once, 8 resp. 32 lanes each; their words
//                are consecutive in the output, which keeps the store coalesced.
// Nothing outside the arrays is read whatever they hold (omm_triangle, omm_texel): a bad corner or texture index sets kStatusOmmIndex.
#include "device_common.h"
#include "kernels.h"
#include "omm.h"

namespace tbvh {

namespace {

constexpr uint32_t kOmmBlock = 64;

__global__ __launch_bounds__(kOmmBlock) void k_omm_bake(OmmSrc src, uint32_t N, uint32_t logN, uint32_t* __restrict__ out, uint32_t* __restrict__ status) {
    __shared__ uint32_t words[2 * kOmmMaxN];                 // kOmmMaxN^2 / 32
    const uint32_t W = omm_words(N);
    const uint32_t logL = min(6u, 3u + 2u * logN);           // lanes per triangle: min( 64, 8 N^2 )
    const uint32_t L = 1u << logL, T = 64u >> logL;          // ... and triangles per wave
    const uint32_t lane = threadIdx.x, slot = lane >> logL, sl = lane & (L - 1);
    const uint32_t places = 8u * N * N;                      // 2N lines of 4N
    uint32_t* mine = words + slot * W;
    const uint64_t nGroups = (src.nTris + T - 1) / T;
    for (uint64_t g = blockIdx.x; g < nGroups; g += gridDim.x) {
        const uint64_t first = g * T, tri = first + slot;
        OmmUV t = {};
        OmmTex tex = {nullptr, 0u, 0u};
        bool bad = false;
        if (tri < src.nTris)
            if (const OmmTex* p = omm_triangle(src, tri, t, bad)) tex = *p;
        if (bad && sl == 0) atomicOr(status, kStatusOmmIndex);
        for (uint32_t k = sl; k < W; k += L) mine[k] = tex.texels ? 0u : 0xFFFFFFFFu;
        __syncthreads();
        if (tex.texels)
            for (uint32_t q = sl; q < places; q += L) {
                uint32_t x, y, idx;
                if (!omm_sample_xy(N, q & (2 * N - 1), q >> (logN + 1), x, y)) continue;
                if (omm_sample(N, x, y, t, tex, idx)) atomicOr(&mine[idx >> 5], 1u << (idx & 31));
            }
        __syncthreads();
        const uint64_t left = src.nTris - first;
        const uint32_t nOut = (uint32_t)(left < T ? left : T) * W;
        for (uint32_t k = lane; k < nOut; k += kOmmBlock) out[first * W + k] = words[k];
        __syncthreads();                                     // (the words are overwritten by the next triangle)
    }
}

}  // namespace

void launch_omm_bake(const OmmSrc& src, uint32_t N, uint32_t* out, uint32_t* status, uint32_t maxBlocks, hipStream_t s) {
    uint32_t logN = 0;
    while ((1u << logN) < N) logN++;
    const uint32_t T = 64u >> (logN >= 2 ? 6u : 3u + 2u * logN);
    const uint64_t nGroups = (src.nTris + T - 1) / T;
    const dim3 grid((uint32_t)(nGroups < maxBlocks ? nGroups : maxBlocks));
    hipLaunchKernelGGL(k_omm_bake, grid, dim3(kOmmBlock), 0, s, src, N, logN, out, status);
}

}  // namespace tbvh
