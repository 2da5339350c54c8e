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
// ONE real addition acc + (+0) that nothing folds away (`zero2`).  The positive half of E_0 is left out exactly as
// k_conv16b<.., DEAD0> leaves it out: the pad term behind the negative half ends every tap.
//
// The multiply-adds are written on pairs of PIXELS of one output column: v_pk_fma_f32 is two fmaf, bit for bit, the two x a
// register pair that one ds_read2_b32 delivers, the weight one half of an aligned scalar register pair, chosen by the
// instruction's op_sel bits.  Nine live columns x four pixels of a lane are 18 such pairs and no lane of a pair is idle (pairs
// of columns, the form before this one, needed 20: the unread forget column f0 rode along).  In a loop of nothing but
// multiply-adds the packed form sustained 0.52-0.73 of the vector peak at 2-3 waves per SIMD where v_fma_f32 with a scalar
// operand stayed at 0.34-0.50 (scripts/microbench/valu_conv.hip, profiles/l0_valu_2026-10-21.json).
#pragma once
#include "tz_conv_kernels.hip.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace tzl0 {

// Per-model constants (weights, biases) read through the constant address space: nothing writes them while a kernel runs,
// and a wave-uniform load from it is a scalar load whatever else the kernel stores.
typedef const __attribute__((address_space(4))) f32x2* cpair;
__device__ __forceinline__ cpair as_const(const float* p) { return (cpair)(unsigned long long)p; }

// two fmaf: acc + x * w[h] per pixel of the pair (h: constant after unrolling).  The half of the scalar pair is chosen by
// op_sel / op_sel_hi of the second source; written out, because from `fma(x, {w[h], w[h]}, acc)` the compiler copies most odd
// halves into an even scalar register first.
__device__ __forceinline__ f32x2 fma2(f32x2 x, f32x2 w, int h, f32x2 acc) {
    if (h) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(x), "s"(w));
    else asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "+v"(acc) : "v"(x), "s"(w));
    return acc;
}

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

static constexpr int GT = 32;              // tile edge, pixels
static constexpr int EW = GT + 2;          // E_0 patch edge
static constexpr int EPL = EW * EW;        // floats of one channel plane of the E_0 patch
static constexpr int RW = GT / 2 + 2;      // R_1 patch edge
static constexpr int RPIX = RW * RW;
// R_1 planes: row stride 20 and a lane's blocks 4 apart put the 32 lanes of an LDS lane group on 32 banks (20 by + bxg mod 32,
// by = 0..7, bxg = 0..3); with rows of 18 and neighbouring blocks in a lane the same reads met four deep.  Plane stride 362:
// the four channel quads of a pixel are stored 8 banks apart.
static constexpr int RS = 20;
static constexpr int RPL = RW * RS + 2;
static constexpr int R_ITEMS = (RPIX * 4 + 255) / 256;   // 16-byte items of one R_1 block per thread
static constexpr int NC = 9;               // live gate columns i0 i1 i2 g0 g1 g2 o0 o1 o2
static constexpr int NCOLS = 16;           // columns of a row of G0_0 and of pack_conv's weights: what choose_l0_forms asks of the convolution
__device__ __forceinline__ constexpr int gate_col(int c) { return c < 3 ? c : c + 3; }   // ... of the 12 [i | f | g | o] x 3

// (wave-uniform) the 32 x 32 tile at (y0, x0) lies where a constant is its uniform row (tile_uniform of the 16-pixel kernels)
__device__ __forceinline__ bool tile32_uniform(const float* u, int ring, int y0, int x0, int H, int W) {
    return u && ring >= 0 && y0 >= ring && y0 + GT <= H - ring && x0 >= ring && x0 + GT <= W - ring;
}
}  // namespace tzl0

// The level-0 gate convolution over [E_0, up(R_1)] and the LSTM update, EPI_LSTM_PACKED of k_conv16b (R_0 = 3: columns
// [i | f | g | o] x 3 of one 16-column tile) as a direct kernel, for the case launch_conv sends here: the positive half of
// E_0 dead and the forget gate out (C0_0 = +0: c = (+0) + i g), nine live columns.  (With both halves and four gates
// k_conv16b measured faster; those forms of this kernel were never launched and are gone: EXPERIMENTS.md.)
// Workgroup = 4 waves = one 32x32-pixel tile = 16x16 blocks of 2x2 pixels, the block under one pixel of R_1.  Wave = one
// parity class (py & 1, px & 1), so the collapsed weights of the upsampled source are wave-uniform; lane = the pixels of
// that class in blocks bxg, bxg + 4, bxg + 8, bxg + 12 of block row by: 4 pixels x 9 columns = 18 accumulator pairs
// (pixels 0 1) and (pixels 2 3) of a column, and a loaded weight is used four times.
// Chain per pixel and column, pack_conv's slot order: acc = G0; E_0: tap (ky, kx) ascending, negative half: 3 channels, pad;
// then per 16-channel block of R_1: collapsed tap tp = 0..3 of the pixel's class, channels ascending (those weights from
// `wg`: pack_conv's values per class, block, tap and channel, 12 columns a row).
// G0: on a tile where it is one row (ConvArgs::init_u, measured at prepare time) nine scalar loads; elsewhere per pixel.
// One LDS region holds the 34x34 halo patch of E_0's negative half as three channel planes, then, block after block, the
// 18x18 half-resolution patch of R_1 as 16 channel planes; the next block waits in registers meanwhile.
__global__ __launch_bounds__(256, 4) void k_l0_gates(const ConvArgs a, const float* wg) {
    using namespace tzl0;
    constexpr int LDSF = 3 * EPL > 16 * RPL ? 3 * EPL : 16 * RPL;
    __shared__ float planes[LDSF];   // E_0: [3 channels][EW][EW]; R_1: [16 channels][RW][RS]
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
            const int Y = px / RW, X = px - Y * RW;
            if (px < RPIX) {
#pragma unroll
                for (int c = 0; c < 4; ++c) planes[(4 * q + c) * RPL + Y * RS + X] = pre[k][c];
            }
        }
    };
    if (nub > 0) fetch_r1(0);
    {   // E_0 patch, the negative half (the second quad of a pixel)
        const float* base = a.src[0].p + (long long)n * a.src[0].nstride;
        for (int i = tid; i < EPL; i += 256) {
            const int y = i / EW, x = i - y * EW;
            const int yy = ty0 - 1 + y, xx = tx0 - 1 + x;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) v = *(const f32x4*)(base + ((long long)yy * a.W + xx) * 8 + 4);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) planes[ch * EPL + i] = v[ch];
        }
    }
    // this lane's pixels: block row by, blocks bxg + 4 k of the row, k = 0..3
    const int by = lane >> 2, bxg = lane & 3;
    const int y = ty0 + 2 * by + pa, x0 = tx0 + 2 * bxg + pb;   // pixel k: (y, x0 + 8 k)
    f32x2 acc[2][NC];   // [pixels (0 1) | (2 3)][column], from G0_0 (launch_conv sends no convolution without start values here)
    if (tile32_uniform(a.init_u, a.init_ring, ty0, tx0, a.H, a.W)) {   // (uniform)
        const cpair row = as_const(a.init_u);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float s = row[gate_col(c) >> 1][gate_col(c) & 1];
            acc[0][c] = acc[1][c] = (f32x2){s, s};
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x = x0 + 8 * k;
            const long long pix = (y < a.H && x < a.W) ? (long long)y * a.W + x : 0;
            const float* g = a.init + pix * NCOLS;   // columns 0..3, 6..7, 8..11
            const f32x4 v0 = *(const f32x4*)g, v2 = *(const f32x4*)(g + 8);
            const f32x2 v1 = *(const f32x2*)(g + 6);
            const float col[NC] = {v0[0], v0[1], v0[2], v1[0], v1[1], v2[0], v2[1], v2[2], v2[3]};
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[k >> 1][c][k & 1] = col[c];
        }
    }
    const f32x2 z = zero2();
    __syncthreads();
    // ---- E_0: 9 taps x [3 channels, pad]
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        f32x2 xe[3][3][2];   // [channel][dx][pixel pair]: patch columns 8 apart
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* xp = planes + ch * EPL + (2 * by + pa + dy) * EW + 2 * bxg + pb;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) xe[ch][dx][pp] = (f32x2){xp[dx + 16 * pp], xp[dx + 16 * pp + 8]};
        }
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int tap = dy * 3 + dx;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const cpair wrow = as_const(a.Wp + (tap * 16 + 4 + ch) * NCOLS);
                f32x2 w[6];
#pragma unroll
                for (int p = 0; p < 6; ++p)
                    if (p != 2) w[p] = wrow[p];   // (columns 4, 5 are the forget gate's)
#pragma unroll
                for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[pp][c] = fma2(xe[ch][dx][pp], w[gate_col(c) >> 1], gate_col(c) & 1, acc[pp][c]);
            }
#pragma unroll
            for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[pp][c] = acc[pp][c] + z;   // the quad's pad term
        }
    }
    // ---- up(R_1): per 16-channel block 4 collapsed taps of this wave's class x 16 channels
    const float* xbase = planes + (by + pa) * RS + bxg + pb;
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
        auto request = [&](int s, f32x2 (&w)[2][6], f32x2 (&xv)[2][2]) {
            const int tp = s >> 3, c0 = 2 * (s & 7);
            const cpair wrow = as_const(wblk + s * 24);
            const float* xp = xbase + c0 * RPL + (tp >> 1) * RS + (tp & 1);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
#pragma unroll
                for (int p = 0; p < 6; ++p)
                    if (p != 2) w[c][p] = wrow[6 * c + p];   // columns 0..3, 6..11 of the row
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) xv[c][pp] = (f32x2){xp[c * RPL + 8 * pp], xp[c * RPL + 8 * pp + 4]};
            }
        };
        auto landed = [&]() {
            __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
            __builtin_amdgcn_sched_barrier(0);
        };
        auto compute = [&](const f32x2 (&w)[2][6], const f32x2 (&xv)[2][2]) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                    for (int col = 0; col < NC; ++col) acc[pp][col] = fma2(xv[c][pp], w[c][gate_col(col) >> 1], gate_col(col) & 1, acc[pp][col]);
            __builtin_amdgcn_sched_barrier(0);
        };
        f32x2 wa[2][6], wb[2][6];
        f32x2 xa[2][2], xb[2][2];
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
    // ---- prednet.py:255-259 as conv_epilogue's EPI_LSTM_PACKED with f * c_prev = +0: c = (+0) + i * g; r = o * tanh(c)
    constexpr int R = 3;
    float* o0 = a.out0 + (long long)n * a.out0_nstride;
    float* o1 = a.out1 ? a.out1 + (long long)n * a.out1_nstride : nullptr;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + 8 * k;
        const bool ok = y < a.H && x < a.W;
        const long long pix = ok ? (long long)y * a.W + x : 0;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const float gi = tz_hard_sigmoid(acc[k >> 1][c][k & 1]);
            const float gg = tz_tanh(acc[k >> 1][R + c][k & 1]);
            const float go = tz_hard_sigmoid(acc[k >> 1][2 * R + c][k & 1]);
            const float cc = add_zero(gi * gg);   // f * (+0) = +0 for every f a hard sigmoid returns
            const float rr = go * tz_tanh(cc);
            if (ok) {
                o0[pix * R + c] = rr;
                if (o1) o1[pix * R + c] = cc;
            }
        }
    }
}
