// The level-0 gate convolution of the reference shape (stack[0] == 3, R_0 == 3, E_0 stored one half per quad) on the vector
// ALU (device code; included by tz_prednet.hip).  At level 0 the matrix pipe multiplies mostly padding -- K is 3 of 4, N is
// 9..12 of 16 -- and in k_conv16b matrix, vector and DMA time add up (profiles/r03/level0_phases.md); a direct kernel pads
// nothing, holds the weights as wave-uniform scalar operands and does the LSTM update inside a lane.  (A_0 was built the
// same way and was not faster than k_conv16b: EXPERIMENTS.md, "Level 0 on the vector ALU".)
//
// Arithmetic: TZ-PA1, the SAME chain per output as k_conv16b / k_conv3x3 / the oracle, in pack_conv's slot order, from
// pack_conv's float32 weights (ConvArgs::Wp).  The pad terms are part of the chain: a zero-padded k position is
// fmaf(+0, +0, acc), which turns an accumulator of -0 into +0 and changes nothing else, and a chain can come back to -0
// behind it (a product that underflows below the smallest subnormal rounds to a signed zero), so every run of pads is kept as
// ONE real addition acc + (+0) that nothing folds away (`zero2`).  Under DEAD0 the positive half of E_0 is left out exactly
// as k_conv16b<.., DEAD0> leaves it out: the pad term behind the negative half ends every tap.
//
// The multiply-adds are written on pairs of neighbouring output columns: v_pk_fma_f32 is two fmaf, bit for bit, x
// broadcast, the two weights an aligned scalar register pair.  In a loop of nothing but multiply-adds the packed form
// sustained 0.52-0.73 of the vector peak at 2-3 waves per SIMD where v_fma_f32 with a scalar operand stayed at 0.34-0.50
// (scripts/microbench/valu_conv.hip, profiles/l0_valu_2026-10-21.json).
#pragma once
#include "tz_conv_kernels.hip.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace tzl0 {

// Per-model constants (weights, biases) read through the constant address space: nothing writes them while a kernel runs,
// and a wave-uniform load from it is a scalar load whatever else the kernel stores.
typedef const __attribute__((address_space(4))) f32x2* cpair;
__device__ __forceinline__ cpair as_const(const float* p) { return (cpair)(unsigned long long)p; }

// two fmaf: acc + x * w per column of the pair
__device__ __forceinline__ f32x2 fma2(float x, f32x2 w, f32x2 acc) { return __builtin_elementwise_fma((f32x2){x, x}, w, acc); }

// a pair of +0 that the compiler cannot see through: `acc + zero2()` stays an addition ((-0) + (+0) = +0 is not the identity)
__device__ __forceinline__ f32x2 zero2() {
    f32x2 z = {0.0f, 0.0f};
    asm volatile("" : "+v"(z));
    return z;
}

// (+0) + x as an instruction of its own (k_wino's fadd_zero)
__device__ __forceinline__ float add_zero(float x) {
    float r;
    asm("v_add_f32 %0, 0, %1" : "=v"(r) : "v"(x));
    return r;
}

}  // namespace tzl0

// The level-0 gate convolution over [E_0, up(R_1)] and the LSTM update, EPI_LSTM_PACKED of k_conv16b (R_0 = 3: columns
// [i | f | g | o] x 3 of one 16-column tile) as a direct kernel.
// Workgroup = 4 waves = one 32x32-pixel tile = 16x16 blocks of 2x2 pixels, the block under one pixel of R_1.  Wave = one
// parity class (py & 1, px & 1), so the collapsed weights of the upsampled source are wave-uniform; lane = the pixels of
// that class in four neighbouring blocks of a row, all gate columns of a pixel in the lane: 4 x 12 accumulators, and a
// loaded weight row is used four times.  NP = column pairs per pixel: 6, or 5 = (i0 i1) (i2 f0) (g0 g1) (g2 o0) (o1 o2) where
// the forget gate is out (f0 rides along in a pair and is not read; NP == 5 takes c = (+0) + i g).
// launch_conv takes <true, 5> only, where both skips apply: with both halves and four gates k_conv16b measured faster
// (the other forms compile and gave the same bits as k_conv16b when they were launched; EXPERIMENTS.md).
// Chain per pixel and column, pack_conv's slot order: acc = G0; E_0: tap (ky, kx) ascending, [positive half: 3 channels,
// pad] negative half: 3 channels, pad; then per 16-channel block of R_1: collapsed tap tp = 0..3 of the pixel's class,
// channels ascending (those weights from `wg`: pack_conv's values per class, block, tap and channel, 12 columns a row).
// One LDS region holds the 34x34 halo patch of E_0 (a quad per pixel and half), then, block after block, the 18x18
// half-resolution patch of R_1 as 16 channel planes; the next block waits in registers meanwhile.
namespace tzl0 {
static constexpr int GT = 32;              // tile edge, pixels
static constexpr int EW = GT + 2;          // E_0 patch edge
static constexpr int RW = GT / 2 + 2;      // R_1 patch edge
static constexpr int RPIX = RW * RW;
static constexpr int R_ITEMS = (RPIX * 4 + 255) / 256;   // 16-byte items of one R_1 block per thread
template <int NP>
__device__ __forceinline__ constexpr int pair_col(int p) { return NP == 6 ? 2 * p : (p < 2 ? 2 * p : 2 * p + 2); }
template <int NP>
__device__ __forceinline__ float col_of(const f32x2 (&acc)[NP], int col) {   // col: constant after unrolling
    return NP == 6 || col < 4 ? acc[col >> 1][col & 1] : acc[(col - 2) >> 1][col & 1];
}
}  // namespace tzl0

template <bool DEAD0, int NP>
__global__ __launch_bounds__(256, DEAD0 && NP == 5 ? 4 : 3) void k_l0_gates(const ConvArgs a, const float* wg) {
    using namespace tzl0;
    constexpr int NQ = DEAD0 ? 1 : 2;
    constexpr int LDSQ = NQ * EW * EW > 16 * RPIX / 4 ? NQ * EW * EW : 16 * RPIX / 4;
    __shared__ f32x4 smem[LDSQ];
    float* const planes = (float*)smem;   // [16 channels][RW][RW]
    const int tid = threadIdx.x, lane = tid & 63, cls = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pa = cls >> 1, pb = cls & 1;
    const int tx32 = (a.W + GT - 1) / GT, ty32 = (a.H + GT - 1) / GT;
    const int tile = blockIdx.x % (tx32 * ty32), n = blockIdx.x / (tx32 * ty32);
    const int ty0 = (tile / tx32) * GT, tx0 = (tile % tx32) * GT;
    const int H2 = a.H >> 1, W2 = a.W >> 1;
    const int nub = a.src[1].cpt;

    // 16 channels of block b of R_1 over the half-resolution patch, out-of-image pixels zero: global -> registers
    const float* r1 = a.src[1].p + (long long)n * a.src[1].nstride;
    const int rps = a.src[1].pstride;
    f32x4 pre[R_ITEMS];
    auto fetch_r1 = [&](int b) {
#pragma unroll
        for (int k = 0; k < R_ITEMS; ++k) {
            const int i = tid + 256 * k, px = i >> 2, q = i & 3;
            const int Y = px / RW, X = px - Y * RW;
            const int ly = (ty0 >> 1) - 1 + Y, lx = (tx0 >> 1) - 1 + X;
            pre[k] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            if (px < RPIX && ly >= 0 && ly < H2 && lx >= 0 && lx < W2) pre[k] = *(const f32x4*)(r1 + ((long long)ly * W2 + lx) * rps + b * 16 + 4 * q);
        }
    };
    auto store_r1 = [&]() {   // registers -> channel planes
#pragma unroll
        for (int k = 0; k < R_ITEMS; ++k) {
            const int i = tid + 256 * k, px = i >> 2, q = i & 3;
            if (px < RPIX) {
#pragma unroll
                for (int c = 0; c < 4; ++c) planes[(4 * q + c) * RPIX + px] = pre[k][c];
            }
        }
    };
    if (nub > 0) fetch_r1(0);
    {   // E_0 patch
        const float* base = a.src[0].p + (long long)n * a.src[0].nstride;
        for (int i = tid; i < NQ * EW * EW; i += 256) {
            const int q = DEAD0 ? 1 : i / (EW * EW), slot = DEAD0 ? i : i - q * (EW * EW);
            const int y = slot / EW, x = slot - y * EW;
            const int yy = ty0 - 1 + y, xx = tx0 - 1 + x;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) v = *(const f32x4*)(base + ((long long)yy * a.W + xx) * 8 + 4 * q);
            smem[i] = v;
        }
    }
    // this lane's pixels: block row by, blocks 4 bxg + k of the row, k = 0..3
    const int by = lane >> 2, bxg = lane & 3;
    const int y = ty0 + 2 * by + pa, x0 = tx0 + 8 * bxg + pb;   // pixel k: (y, x0 + 2 k)
    f32x2 acc[4][NP];   // from G0_0 (launch_conv sends no convolution without start values here)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + 2 * k;
        const long long pix = (y < a.H && x < a.W) ? (long long)y * a.W + x : 0;
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[k][p] = *(const f32x2*)(a.init + pix * a.ncols + pair_col<NP>(p));
    }
    const f32x2 z = zero2();
    __syncthreads();
    // ---- E_0: 9 taps x [3 channels, pad] per half
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        f32x4 xr[NQ][9];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int j = 0; j < 9; ++j) xr[q][j] = smem[q * (EW * EW) + (2 * by + pa + dy) * EW + 8 * bxg + pb + j];
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int tap = dy * 3 + dx;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float* wrow = a.Wp + (tap * 16 + 4 * (DEAD0 ? 1 : q) + ch) * a.ncols;
                    f32x2 w[NP];
#pragma unroll
                    for (int p = 0; p < NP; ++p) w[p] = as_const(wrow + pair_col<NP>(p))[0];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int p = 0; p < NP; ++p) acc[k][p] = fma2(xr[q][2 * k + dx][ch], w[p], acc[k][p]);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int p = 0; p < NP; ++p) acc[k][p] = acc[k][p] + z;   // the quad's pad term
            }
        }
    }
    // ---- up(R_1): per 16-channel block 4 collapsed taps of this wave's class x 16 channels
    const float* xbase = planes + (by + pa) * RW + 4 * bxg + pb;
#pragma unroll 1
    for (int b = 0; b < nub; ++b) {
        __syncthreads();   // the region was last read by the phase before
        store_r1();
        __syncthreads();
        if (b + 1 < nub) fetch_r1(b + 1);
        // 32 steps of (collapsed tap, two channels), rolled (unrolled, the scheduler hoists the LDS reads of all of them and
        // the accumulators spill) and pipelined by hand: the operands of step s + 1 are requested once those of step s have
        // landed and before step s computes.  Scalar loads return out of order, so a wait for them is a wait for every one in
        // flight: requested any earlier, step s + 1 would be waited for in front of step s.
        // (weights from the class-major image `wg`, choose_l0_forms: the steps of a class are one linear stream of 24 floats)
        const float* wblk = wg + (long long)(cls * nub + b) * (64 * 12);
        auto request = [&](int s, f32x2 (&w)[2][6], float (&xv)[2][4]) {
            const int tp = s >> 3, c0 = 2 * (s & 7);
            const cpair wrow = as_const(wblk + s * 24);
            const float* xp = xbase + c0 * RPIX + (tp >> 1) * RW + (tp & 1);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
#pragma unroll
                for (int p = 0; p < 6; ++p) w[c][p] = wrow[6 * c + p];   // columns 0..11 of the row
#pragma unroll
                for (int k = 0; k < 4; ++k) xv[c][k] = xp[c * RPIX + k];
            }
        };
        auto landed = [&]() {
            __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
            __builtin_amdgcn_sched_barrier(0);
        };
        auto compute = [&](const f32x2 (&w)[2][6], const float (&xv)[2][4]) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int p = 0; p < NP; ++p) acc[k][p] = fma2(xv[c][k], w[c][pair_col<NP>(p) >> 1], acc[k][p]);
            __builtin_amdgcn_sched_barrier(0);
        };
        f32x2 wa[2][6], wb[2][6];
        float xa[2][4], xb[2][4];
        request(0, wa, xa);
        landed();
#pragma unroll 1
        for (int s = 0; s < 32; s += 2) {
            request(s + 1, wb, xb);
            compute(wa, xa);
            landed();
            request(s + 2, wa, xa);   // (the last one is not used: the next block's first rows, or the image's tail pad; x: inside the region)
            compute(wb, xb);
            landed();
        }
    }
    // ---- prednet.py:255-259 as conv_epilogue's EPI_LSTM_PACKED: c = f * c_prev + i * g; r = o * tanh(c)
    constexpr int R = 3;
    float* o0 = a.out0 + (long long)n * a.out0_nstride;
    float* o1 = a.out1 ? a.out1 + (long long)n * a.out1_nstride : nullptr;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + 2 * k;
        const bool ok = y < a.H && x < a.W;
        const long long pix = ok ? (long long)y * a.W + x : 0;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const float gi = tz_hard_sigmoid(col_of<NP>(acc[k], c));
            const float gg = tz_tanh(col_of<NP>(acc[k], 2 * R + c));
            const float go = tz_hard_sigmoid(col_of<NP>(acc[k], 3 * R + c));
            const float t2 = gi * gg;
            float cc;
            if (NP == 6) {
                const float gf = tz_hard_sigmoid(col_of<NP>(acc[k], R + c));
                const float cp = a.aux ? a.aux[pix * R + c] : 0.0f;
                const float t1 = gf * cp;
                cc = t1 + t2;
            } else {
                cc = add_zero(t2);   // f * (+0) = +0 for every f a hard sigmoid returns
            }
            const float rr = go * tz_tanh(cc);
            if (ok) {
                o0[pix * R + c] = rr;
                if (o1) o1[pix * R + c] = cc;
            }
        }
    }
}
