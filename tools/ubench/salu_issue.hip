// salu_issue.hip — how many scalar-side instructions (SALU, branches) does one CU of gfx950 issue per second and per shader cycle?
//
// Behind profiles/packet_scalar.txt: the wave-packet kernel (kernels_cwbvh_packet.hip) runs about 2.1 G scalar-side instructions per second per CU on a
// camera launch; whether that is near what the CU's scalar side can issue decides whether cutting scalar instructions can speed it up.  Here:
//   * W one-wave workgroups per CU (W = 4, 8, 16, 32: one to eight waves per SIMD; dynamic LDS sized so that exactly W fit a CU), each a long stream of
//     s_add_u32 / s_xor_b32 over eight independent accumulators, no memory access inside the loop;
//   * three streams: the scalar instructions alone; 1:1 with v_fma_f32 (eight independent vector accumulators); with a TAKEN s_cbranch_scc1 as every
//     eighth instruction (six ALU, one s_cmp_eq_u32 that sets SCC, the branch over one instruction that is never issued);
//   * cycles are read in the kernel (s_memtime, the shader clock: clock64()), per wave, next to the HIP-event time of the launch.
// Per CU: instructions per cycle = W x instructions per wave / mean wave lifetime in cycles (the W waves of a CU live side by side for the same time);
// instructions per second = the same over the launch's wall time.  The loop's own s_add / s_cmp / s_cbranch (3 per 128 stream instructions) are not counted.
// Results leave through vector stores only.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

enum Mode { ALONE, MIX_FMA, BRANCH8, NMODES };
static const char* kNames[] = {"scalar ALU alone", "scalar ALU 1:1 with v_fma_f32", "taken s_cbranch every 8th instruction"};

// one group: 8 scalar-side instructions of the stream (MIX_FMA: plus 8 v_fma_f32 in between)
#define SALU8 \
    "s_add_u32 %0, %0, %8\n s_xor_b32 %1, %1, %8\n s_add_u32 %2, %2, %8\n s_xor_b32 %3, %3, %8\n" \
    "s_add_u32 %4, %4, %8\n s_xor_b32 %5, %5, %8\n s_add_u32 %6, %6, %8\n s_xor_b32 %7, %7, %8\n"
#define MIX8 \
    "s_add_u32 %0, %0, %16\n v_fma_f32 %8, %8, %17, %18\n s_xor_b32 %1, %1, %16\n v_fma_f32 %9, %9, %17, %18\n" \
    "s_add_u32 %2, %2, %16\n v_fma_f32 %10, %10, %17, %18\n s_xor_b32 %3, %3, %16\n v_fma_f32 %11, %11, %17, %18\n" \
    "s_add_u32 %4, %4, %16\n v_fma_f32 %12, %12, %17, %18\n s_xor_b32 %5, %5, %16\n v_fma_f32 %13, %13, %17, %18\n" \
    "s_add_u32 %6, %6, %16\n v_fma_f32 %14, %14, %17, %18\n s_xor_b32 %7, %7, %16\n v_fma_f32 %15, %15, %17, %18\n"
#define BR8 \
    "s_add_u32 %0, %0, %8\n s_xor_b32 %1, %1, %8\n s_add_u32 %2, %2, %8\n s_xor_b32 %3, %3, %8\n" \
    "s_add_u32 %4, %4, %8\n s_xor_b32 %5, %5, %8\n s_cmp_eq_u32 %8, %8\n s_cbranch_scc1 .Ltaken%=\n" \
    "s_add_u32 %6, %6, %8\n" \
    ".Ltaken%=:\n"

template <int MODE> __global__ __launch_bounds__(64) void k(float* out, unsigned long long* cyc, int iters, unsigned kk, float a, float b) {
    extern __shared__ char pad[];   // only sizes the workgroup (waves per CU)
    unsigned s0 = kk, s1 = kk + 1, s2 = kk + 2, s3 = kk + 3, s4 = kk + 4, s5 = kk + 5, s6 = kk + 6, s7 = kk + 7;
    float r0 = threadIdx.x, r1 = r0 + 1, r2 = r0 + 2, r3 = r0 + 3, r4 = r0 + 4, r5 = r0 + 5, r6 = r0 + 6, r7 = r0 + 7;
    const unsigned long long t0 = clock64();
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (MODE == ALONE)
                asm volatile(SALU8 : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3), "+s"(s4), "+s"(s5), "+s"(s6), "+s"(s7) : "s"(kk) : "scc");
            else if (MODE == MIX_FMA)
                asm volatile(MIX8 : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3), "+s"(s4), "+s"(s5), "+s"(s6), "+s"(s7),
                                    "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), "+v"(r7)
                             : "s"(kk), "v"(a), "v"(b) : "scc");
            else
                asm volatile(BR8 : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3), "+s"(s4), "+s"(s5), "+s"(s6), "+s"(s7) : "s"(kk) : "scc");
        }
    }
    const unsigned long long t1 = clock64();
    if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
    out[blockIdx.x * 64 + threadIdx.x] = r0 + r1 + r2 + r3 + r4 + r5 + r6 + r7 + (float)(s0 ^ s1 ^ s2 ^ s3 ^ s4 ^ s5 ^ s6 ^ s7);
}

struct Res { double perCycle, perSec, ghz; };

template <int MODE> Res run(float* d, unsigned long long* dc, int cus, int wavesPerCU, int iters) {
    const int blocks = cus * wavesPerCU;
    const size_t lds = (size_t)(160 * 1024) / wavesPerCU - 64;   // exactly wavesPerCU one-wave workgroups fit a CU
    hipFuncSetAttribute((const void*)k<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(64), lds, 0, d, dc, 64, 3u, 1.0001f, 0.5f);
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(64), lds, 0, d, dc, iters, 3u, 1.0001f, 0.5f);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> c(blocks);
    hipMemcpy(c.data(), dc, blocks * 8, hipMemcpyDeviceToHost);
    double sum = 0; for (auto v : c) sum += (double)v;
    const double meanCyc = sum / blocks;
    const double perWave = (double)iters * 128.0;   // scalar-side instructions of the stream per wave (the v_fma_f32 of MIX_FMA are not counted)
    Res r;
    r.perCycle = wavesPerCU * perWave / meanCyc;
    r.perSec = wavesPerCU * perWave / (ms * 1e-3);
    r.ghz = meanCyc / (ms * 1e6);
    hipEventDestroy(e0); hipEventDestroy(e1);
    return r;
}

int main(int argc, char** argv) {
    int iters = 4000;   // 512 000 stream instructions per wave: about 0.1 s of GPU time for all rows
    if (argc > 1) iters = atoi(argv[1]);
    hipDeviceProp_t p; hipGetDeviceProperties(&p, 0);
    const int cus = p.multiProcessorCount;
    printf("device %s: %d CUs; %d x 128 scalar-side instructions per wave\n", p.name, cus, iters);
    printf("per CU: instructions per shader cycle (s_memtime, mean wave lifetime) and G instructions per second (HIP-event time of the launch)\n");
    float* d; hipMalloc(&d, (size_t)cus * 32 * 64 * 4);
    unsigned long long* dc; hipMalloc(&dc, (size_t)cus * 32 * 8);
    printf("%-40s %9s %12s %12s %10s\n", "stream", "waves/CU", "instr/cycle", "G instr/s", "clock GHz");
    for (int w : {4, 8, 16, 32}) {
        const Res r[NMODES] = {run<ALONE>(d, dc, cus, w, iters), run<MIX_FMA>(d, dc, cus, w, iters), run<BRANCH8>(d, dc, cus, w, iters)};
        for (int i = 0; i < NMODES; i++) printf("%-40s %9d %12.3f %12.3f %10.2f\n", kNames[i], w, r[i].perCycle, r[i].perSec * 1e-9, r[i].ghz);
        fflush(stdout);
    }
    hipFree(d); hipFree(dc);
    return 0;
}
