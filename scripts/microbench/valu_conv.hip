// What fraction of the fp32 VALU peak (32 MAC/clk/SIMD: v_fma_f32 on a wave64 takes 2 cycles) does the inner loop of a
// direct level-0 convolution sustain?  The loop the kernels would have: acc = fmaf(x_vgpr, w_uniform, acc) streaming into
// SHARE x CLS x NCOL accumulators per lane, x from an LDS patch (one ds_read_b32 per NCOL fmas), the wave-uniform weights
//   MODE 0: as SGPR operands, scalar loads from global memory (the compiler's s_load_dwordx4/x8/x16 stream);
//   MODE 1: as VGPRs filled by broadcast ds_read_b128 (all lanes one address) from an LDS weight image.
// Shapes:  gates  SHARE = 2x2 blocks per lane, CLS = 4 parity classes, NCOL = 9 / 12 gate columns,
//                 48 channels x 4 collapsed taps x 4 classes of weights (27 / 36 KB: more than the scalar cache)
//          A0     SHARE = the 4 pixels of a pooling window, CLS = 1, NCOL = 16, 36 steps of weights (2.3 KB)
// 256 threads per workgroup, LDS sized so that exactly OCC workgroups share a CU = OCC waves per SIMD (2 unless said).
// Prints one JSON line per shape: achieved MAC/clk/SIMD and the in-kernel clock (s_memtime / s_memrealtime x 100 MHz).
// (MODE 1 reads LDS through asm volatile, one step ahead: left to the compiler, the LDS reads of the whole loop body are
// hoisted to its top and the accumulators spill.)
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off valu_conv.hip -o valu_conv && timeout 120 ./valu_conv
// plain v_fma_f32 in place of the packed form: add -fno-slp-vectorize -DNOSLP
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

#ifdef NOSLP
#define BUILD_LABEL "O3_noslp"
#else
#define BUILD_LABEL "O3"   // the project's flags: the SLP vectoriser packs pairs of chains into v_pk_fma_f32
#endif
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ unsigned lds_addr(const float* p) { return (unsigned)(unsigned long long)(const __attribute__((address_space(3))) void*)p; }
static constexpr int XS = 4096;              // floats of the x patch
// LDS per workgroup sized so that exactly OCC workgroups (= OCC waves per SIMD) share a CU's 160 KB
constexpr int lds_floats(int occ) { return occ == 2 ? 14 * 1024 : occ == 3 ? 11 * 1024 : 9 * 1024; }   // 56 / 44 / 36 KB

// one step = one (class, tap, channel): NCOL weights, SHARE x values, SHARE x NCOL fmas
template <int MODE, int PIPE, int SHARE, int CLS, int NCOL, int UNR, int OCC>
__global__ __launch_bounds__(256, OCC) void k(const float* __restrict__ w, const float* __restrict__ xg, float* __restrict__ out,
                                            unsigned long long* __restrict__ stamps, int iters, int reps, int wfloats) {
    constexpr int NCP = (NCOL + 3) & ~3;
    __shared__ __attribute__((aligned(16))) float smem[lds_floats(OCC)];
    float* xs = smem;
    float* ws = smem + XS;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < XS; i += 256) xs[i] = xg[i];
    if (MODE == 1)
        for (int i = tid; i < wfloats; i += 256) ws[i] = w[i];
    __syncthreads();
    float acc[SHARE][CLS][NCOL];
#pragma unroll
    for (int s = 0; s < SHARE; ++s)
#pragma unroll
        for (int c = 0; c < CLS; ++c)
#pragma unroll
            for (int j = 0; j < NCOL; ++j) acc[s][c][j] = 0.0f;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    // operands of one step: NCOL weights (padded to a multiple of 4) and SHARE x values
    auto load = [&](int step, int rep, float (&wr)[NCP], float (&x)[SHARE]) {
        if (MODE == 0) {
#pragma unroll
            for (int j = 0; j < NCP; ++j) wr[j] = w[step * NCP + j];
        } else {
            f32x4 v[NCP / 4];
#pragma unroll
            for (int j = 0; j < NCP / 4; ++j)
                asm volatile("ds_read_b128 %0, %1" : "=v"(v[j]) : "v"(lds_addr(ws + step * NCP + 4 * j)) : "memory");
#pragma unroll
            for (int s = 0; s < SHARE; ++s)
                asm volatile("ds_read_b32 %0, %1" : "=v"(x[s]) : "v"(lds_addr(xs + ((tid * SHARE + s + (step + rep) * 17) & (XS - 1)))) : "memory");
#pragma unroll
            for (int j = 0; j < NCP / 4; ++j) { wr[4 * j] = v[j][0]; wr[4 * j + 1] = v[j][1]; wr[4 * j + 2] = v[j][2]; wr[4 * j + 3] = v[j][3]; }
            return;
        }
#pragma unroll
        for (int s = 0; s < SHARE; ++s) x[s] = xs[(tid * SHARE + s + (step + rep) * 17) & (XS - 1)];
    };
    // MODE 1: the reads issued by the last load() have landed, and nothing reads their registers before this
    auto landed = [&](float (&wr)[NCP], float (&x)[SHARE]) {
        if (MODE == 0) return;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < NCP; ++j) asm volatile("" : "+v"(wr[j]));
#pragma unroll
        for (int s = 0; s < SHARE; ++s) asm volatile("" : "+v"(x[s]));
    };
    const int nsteps = iters * UNR * CLS * 4;
    float wn[NCP], xn[SHARE];
    if (PIPE) { load(0, 0, wn, xn); landed(wn, xn); }
    for (int rep = 0; rep < reps; ++rep) {
#pragma unroll 1
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int c = 0; c < CLS; ++c)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int step = ((it * UNR + u) * CLS + c) * 4 + t;
                        float wr[NCP], x[SHARE];
                        if (PIPE) {   // one step ahead, and the scheduler keeps it at one 
#pragma unroll
                            for (int j = 0; j < NCP; ++j) wr[j] = wn[j];
#pragma unroll
                            for (int s = 0; s < SHARE; ++s) x[s] = xn[s];
                            load(step + 1 == nsteps ? 0 : step + 1, rep, wn, xn);
                        } else {
                            load(step, rep, wr, x);
                        }
#pragma unroll
                        for (int s = 0; s < SHARE; ++s)
#pragma unroll
                            for (int j = 0; j < NCOL; ++j) acc[s][c][j] = __builtin_fmaf(x[s], wr[j], acc[s][c][j]);
                        if (PIPE) { landed(wn, xn); __builtin_amdgcn_sched_barrier(0); }
                    }
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    float sum = 0.0f;
#pragma unroll
    for (int s = 0; s < SHARE; ++s)
#pragma unroll
        for (int c = 0; c < CLS; ++c)
#pragma unroll
            for (int j = 0; j < NCOL; ++j) sum += acc[s][c][j];
    out[(size_t)blockIdx.x * 256 + tid] = sum;
    if (tid == 0) {
        stamps[2 * blockIdx.x] = t1 - t0;
        stamps[2 * blockIdx.x + 1] = r1 - r0;
    }
}

static float *d_w, *d_x, *d_out;
static unsigned long long* d_st;
static constexpr int GRID = 256 * 12;   // 6 / 4 / 3 rounds of 2 / 3 / 4 workgroups per CU

template <int MODE, int PIPE, int SHARE, int CLS, int NCOL, int UNR, int OCC = 2>
static void run(const char* name, int iters, int reps) {
    constexpr int NCP = (NCOL + 3) & ~3;
    const int wfloats = iters * UNR * CLS * 4 * NCP;
    if (MODE == 1 && XS + wfloats > lds_floats(OCC)) { fprintf(stderr, "%s: weight image does not fit\n", name); exit(1); }
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    auto launch = [&]() { hipLaunchKernelGGL((k<MODE, PIPE, SHARE, CLS, NCOL, UNR, OCC>), dim3(GRID), dim3(256), 0, 0, d_w, d_x, d_out, d_st, iters, reps, wfloats); };
    for (int i = 0; i < 10; ++i) launch();
    CHECK(hipDeviceSynchronize());
    const int L = 30;
    CHECK(hipEventRecord(e0));
    for (int i = 0; i < L; ++i) launch();
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    std::vector<unsigned long long> st(2 * GRID);
    CHECK(hipMemcpy(st.data(), d_st, st.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> clk(GRID), cyc(GRID);
    for (int i = 0; i < GRID; ++i) {
        clk[i] = st[2 * i + 1] ? (double)st[2 * i] / (double)st[2 * i + 1] * 0.1 : 0.0;   // GHz
        cyc[i] = (double)st[2 * i];
    }
    std::sort(clk.begin(), clk.end());
    std::sort(cyc.begin(), cyc.end());
    const double ghz = clk[GRID / 2];
    const double macs_wave = (double)reps * iters * UNR * CLS * 4 * SHARE * NCOL * 64;   // lane MACs of one wave
    const double us = ms * 1e3 / L;
    // whole launch, tails and staging included
    const double launch_rate = macs_wave * 4 * GRID / (us * 1e-6 * ghz * 1e9 * 1024);
    // the loop alone: a SIMD runs OCC waves side by side for the median workgroup's loop cycles
    const double loop_rate = OCC * macs_wave / cyc[GRID / 2];
    printf("{\"build\": \"" BUILD_LABEL "\", \"shape\": \"%s\", \"weights\": \"%s\", \"schedule\": \"%s\", \"waves_per_simd\": %d, \"acc_per_lane\": %d, \"us_per_launch\": %.1f, \"clock_ghz\": %.3f, "
           "\"mac_per_clk_simd_launch\": %.2f, \"mac_per_clk_simd_loop\": %.2f, \"of_peak_loop\": %.3f}\n",
           name, MODE == 0 ? "sgpr" : "lds_broadcast", PIPE ? "one_step_ahead" : "compiler", OCC, SHARE * CLS * NCOL, us, ghz, launch_rate, loop_rate, loop_rate / 32.0);
    fflush(stdout);
}

int main() {
    std::vector<float> h(64 * 1024);
    unsigned s = 12345u;
    for (auto& v : h) { s = s * 1664525u + 1013904223u; v = ((int)(s >> 8) - (1 << 23)) * (1.0f / (1 << 23)); }
    CHECK(hipMalloc(&d_w, h.size() * 4));
    CHECK(hipMalloc(&d_x, XS * 4));
    CHECK(hipMalloc(&d_out, (size_t)GRID * 256 * 4));
    CHECK(hipMalloc(&d_st, (size_t)GRID * 16));
    CHECK(hipMemcpy(d_w, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_x, h.data() + 1000, XS * 4, hipMemcpyHostToDevice));
    // gates: 48 channels = 24 iterations of 2; 8 tiles per workgroup
    run<0, 0, 2, 4, 9, 2>("gates9_2blocks", 24, 8);
    run<0, 1, 2, 4, 9, 2>("gates9_2blocks", 24, 8);
    run<1, 1, 2, 4, 9, 2>("gates9_2blocks", 24, 8);
    run<0, 0, 2, 4, 12, 2>("gates12_2blocks", 24, 8);
    run<0, 1, 2, 4, 12, 2>("gates12_2blocks", 24, 8);
    run<1, 1, 2, 4, 12, 2>("gates12_2blocks", 24, 8);
    run<0, 0, 4, 4, 9, 1>("gates9_4blocks", 48, 8);
    run<0, 1, 4, 4, 9, 1>("gates9_4blocks", 48, 8);
    run<1, 1, 4, 4, 9, 1>("gates9_4blocks", 48, 8);
    // A0: 36 steps (27 taps x channels and their pads) = 3 iterations of 3 x 4; 64 tiles per workgroup
    run<0, 0, 4, 1, 16, 3>("a0_16cols", 3, 64);
    run<0, 1, 4, 1, 16, 3>("a0_16cols", 3, 64);
    run<1, 1, 4, 1, 16, 3>("a0_16cols", 3, 64);
    // more waves per SIMD, where the registers allow
    run<0, 1, 2, 4, 9, 2, 3>("gates9_2blocks", 24, 8);
    run<0, 1, 2, 4, 9, 2, 4>("gates9_2blocks", 24, 8);
    run<0, 0, 4, 1, 16, 3, 3>("a0_16cols", 3, 64);
    run<0, 1, 4, 1, 16, 3, 3>("a0_16cols", 3, 64);
    run<1, 1, 4, 1, 16, 3, 3>("a0_16cols", 3, 64);
    run<0, 1, 4, 1, 16, 3, 4>("a0_16cols", 3, 64);
    run<1, 1, 4, 1, 16, 3, 4>("a0_16cols", 3, 64);
    return 0;
}
