// k_wino: the per-frame convolutions of levels >= 1 under arithmetic contract TZ-PA2 (round 4).
//
// What it computes (prednet.py:254-259 gate convolutions over [r_{t-1}, e_{t-1}, up(r_{l+1})] with the LSTM update,
// prednet.py:289-291 + 274-277 A convolutions with pooling and the next level's error unit): the same convolutions as
// k_conv16, with the SAME-RESOLUTION source evaluated as Winograd F(2x2, 3x3) -- 16 multiplies per input channel and 2x2
// outputs instead of 36 -- in the fixed order that oracle/tz_oracle.c::conv3x3_wino states (TZ-PA2):
//   tile (ty, tx) = outputs (2ty + a, 2tx + b); V = B^T d B of its 4x4 input patch, columns first, in float32;
//   D[i][j] = ONE fmaf chain from 0 over the input channels in ascending order: D = fmaf(V[i][j](c), U[i][j](c, col), D)
//             with U = G g G^T evaluated on the host in float32 -- what v_mfma_f32_16x16x4_f32 computes along k;
//   Z[i][0] = (D[i][0] + D[i][1]) + D[i][2],  Z[i][1] = (D[i][1] - D[i][2]) - D[i][3];
//   y[0][b] = ((init + Z[0][b]) + Z[1][b]) + Z[2][b],  y[1][b] = ((init + Z[1][b]) - Z[2][b]) - Z[3][b],
//             init = bias, or G0 = bias + the direct TZ-PA1 chain over the constant r_{t-1} source (tz_model_prepare);
//   an upsampled source then continues every output's chain with its 4 collapsed taps (the four outputs of a tile are the
//   four parity classes over the same 2x2 half-resolution pixels), order: 16-channel block, channel quad, tap, channel.
//
// How (scripts/microbench/wino8.hip is the measured skeleton):
//   workgroup = 8 waves = 16x16 output pixels x 64 (48) columns, ONE per CU (123 KB of LDS, 256 registers per wave), two
//   waves per SIMD.  Wave (mt, ph): the 16 tiles of quadrant mt and the transform rows i = 2 ph, 2 ph + 1: 8 positions x NT
//   column tiles = 128 accumulation registers, held in AGPRs by asm MFMAs with a tied operand.  The channel quad is the
//   outermost loop: a STAGE = 16 KB of transformed weights [position][lane][4 column tiles] + one quad plane of the 18x18
//   halo patch (columns stored evens first: the 16 tiles of a wave sit on consecutive slots, 2-way bank conflicts instead of
//   4-way), DMA'd into a ring of 4 slots 3 stages ahead; per stage and wave 32 MFMAs, 8 ds_read_b128 of weights in one
//   continuous stream 4 positions ahead, 6 ds_read2_b32 of the patch and 10 packed adds for the next stage's B^T d B, one
//   counted vmcnt wait and one barrier.  The stage loops are unrolled once per ring slot; the DMA issue of a stage sits
//   behind its first four MFMAs (right behind the barrier both waves of a SIMD ran its scalar code with the matrix pipe
//   empty: 5.5 % of the kernel).  After the last channel quad the partners exchange two row sums each through LDS and form
//   their two outputs per tile; the upsampled source then runs through the same pipeline (stage = one channel quad: 4
//   classes x 4 taps of collapsed weights, 3 patch reads, no transform), the epilogue is fused.  A workgroup does `ipw`
//   column blocks of its tile one after the other (items): the stage image is [column block][stage], the DMA stream runs
//   on from one item into the next.
// Invariants nobody checks for us (DESIGN.md section 5 "hand-scheduled kernels" applies here too):
//   * every wave issues exactly 3 LDS-DMA instructions per stage, all of them before the stage's tail, so `vmcnt(3)` there
//     = "my pieces of stage s + 2 have landed" (other loads or stores in flight only make that wait longer, never shorter:
//     loads return in order);
//   * S1 and S2 are multiples of 4 (sources of 16 k channels): an item starts in ring slot 0 whatever came before it;
//   * the LDS queue is in order, so the lgkmcnt immediates below are counts of younger reads;
//   * asm MFMAs get no hazard handling from the compiler: a VALU result is never consumed by the very next MFMA (empty
//     asm statements pin the transform away from its first use), accumulators are read behind explicit wait states.
#pragma once
#include "tz_conv_kernels.hip.h"

namespace tzw {
#ifndef TZW_LEAD
#define TZW_LEAD 3
#endif
#ifndef TZW_NS
#define TZW_NS 4
#endif
// ring slots; stages in flight ahead of the one being multiplied (<= NS - 1).  Measured on one box (scripts/gpu_wino_ab.sh,
// ms of k_wino per cfg3 step), first kernel: LEAD 5: 43.64, 4: 43.62, 3: 43.21, 2: 43.34; final schedule: 3: 37.2, 2: 39.2 --
// three stages (3 us) cover the memory latency, more only fills the queues.  (The whole exchange of the output transform in
// one round, 64 KB of LDS: measured 6 % SLOWER, 46.0 against 43.3 ms; it stays one column tile a round.)
static constexpr int NS = TZW_NS, LEAD = TZW_LEAD;
static_assert(LEAD >= 2 && LEAD <= NS - 1, "the slot a stage is DMA'd into must be one nobody reads any more");
static_assert(NS == 4, "the stage loops are unrolled once per ring slot (every LDS address a constant), 4 stages = one 16-channel block");
static constexpr int WBYTES = 16 * 1024;             // weights of a stage
static constexpr int PP = 41, P1BYTES = 8 * PP * 16; // same-resolution patch plane: 8 DMA pieces of 41 slots (>= 18 x 18)
static constexpr int UP = 13, P2BYTES = 8 * UP * 16; // half-resolution patch plane: 8 pieces of 13 slots (>= 10 x 10)
static constexpr int SLOT = WBYTES + P1BYTES + P2BYTES;
static constexpr int XBYTES = 32 * 1024;             // exchange areas of the wave pairs: two of 16 KB, used in turn
static constexpr int LDS_BYTES = NS * SLOT + XBYTES; // 125,952: one workgroup per CU all the same (256 registers per wave)
static_assert(LDS_BYTES <= 160 * 1024, "LDS of a CU");
static constexpr int WPW = 18, WLW = 10;   // halo patch of 18 x 18 pixels, half-resolution patch of 10 x 10

__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(unsigned long long)(const __attribute__((address_space(3))) void*)p;
}
// (TZW_ABL 32, diagnostic: everything around a DMA stays, the DMA instruction itself is left out)
#if defined(TZW_ABL) && (TZW_ABL & 32)
#define TZW_DMA_INS "; "
#else
#define TZW_DMA_INS "global_load_lds_dwordx4 "
#endif
__device__ __forceinline__ void dma_lanes(const float* ubase, unsigned voff, unsigned lds) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\t" TZW_DMA_INS "%0, %1" : : "v"(voff), "s"(ubase), "s"(lds) : "memory");
}
__device__ __forceinline__ void dma_gather(const float* ubase, unsigned voff, unsigned long long mask, unsigned lds) {
    unsigned long long saved;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %4\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t" TZW_DMA_INS "%1, %2\n\t"
                 "s_mov_b64 exec, %0"
                 : "=&s"(saved) : "v"(voff), "s"(ubase), "s"(lds), "s"(mask) : "memory");
}
template <int O0, int O1>
__device__ __forceinline__ f32x2 lds_read2(unsigned addr) {
    f32x2 v;
    asm volatile("ds_read2_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(v) : "v"(addr), "n"(O0), "n"(O1) : "memory");
    return v;
}
template <int OFF>
__device__ __forceinline__ f32x4 lds_read16(unsigned addr) {
    f32x4 v;
#if defined(TZW_ABL) && (TZW_ABL & 4)
    v = (f32x4){1.f, 2.f, 3.f, 4.f};
    asm volatile("" : "+v"(v), "+v"(addr));
    return v;
#endif
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
// in-place accumulation in an AGPR tuple (see the header: the register allocator must not get a say)
__device__ __forceinline__ void mfma_acc(f32x4& acc, float a, float b) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
// the first multiplication of a chain: the accumulator starts at the literal 0 (fma(a, b, +0), the same operation as on a zeroed
// register -- without the 128 register writes per item that zeroing was)
__device__ __forceinline__ void mfma_first(f32x4& acc, float a, float b) {
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=a"(acc) : "v"(a), "v"(b));
}
// float32 add / subtract the compiler cannot pair into v_pk_add_f32 (it did: 16 packed adds + 12 moves to line their
// operands up, 28 instructions where 20 do -- and a packed fp32 instruction takes the SIMD longer than a plain one, all of
// it time the matrix pipe does not get).  Same IEEE results.
__device__ __forceinline__ float fsub(float a, float b) {
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float fadd(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (+0) + x as an instruction of its own: nothing folds it away (it is not the identity: (+0) + (-0) = +0), and x arrives
// rounded, so nothing fuses the multiplication in front of it into it either
__device__ __forceinline__ float fadd_zero(float x) {
    float r;
    asm("v_add_f32 %0, 0, %1" : "=v"(r) : "v"(x));
    return r;
}
// every wave issues 3 LDS-DMA instructions per stage: "my pieces of all but the N youngest stages have landed"
template <int N>
__device__ __forceinline__ void wait_vm_stages() {
    static_assert(N >= 0 && N <= 3, "immediate of s_waitcnt");
    if (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (N == 1) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if (N == 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
}
#ifndef TZW_PK
#define TZW_PK 1
#endif
template <int K>
__device__ __forceinline__ void read_rows(unsigned ad, f32x2 (&d)[3][2]) {   // row k of the wave's three patch rows
#if TZW_PK
    d[K][0] = lds_read2<72 * K, 72 * K + 36>(ad);       // (d0, d1): columns 0 and 1 (evens first: column 1 sits 9 slots on)
    d[K][1] = lds_read2<72 * K + 4, 72 * K + 40>(ad);   // (d2, d3)
#else
    d[K][0] = lds_read2<72 * K, 72 * K + 4>(ad);        // (d0, d2)
    d[K][1] = lds_read2<72 * K + 36, 72 * K + 40>(ad);  // (d1, d3)
#endif
}
// packed float32 add / subtract with the operand halves chosen per instruction (same IEEE results as two scalar ones):
//   pk_sub(a, b)  = (a.lo - b.lo, a.hi - b.hi);  pk_add likewise
//   pk_cross(a, b) = (a.hi + b.lo, b.lo - a.hi)   -- the two middle columns of B^T d: (d1 + d2, d2 - d1) from (d0, d1), (d2, d3)
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
    f32x2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) {
    f32x2 r;
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ f32x2 pk_cross(f32x2 a, f32x2 b) {
    f32x2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,0] neg_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
}  // namespace tzw

#define TZW_TIE8(X) asm volatile("" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3]), "+v"(X[4]), "+v"(X[5]), "+v"(X[6]), "+v"(X[7]))
#define TZW_TIE6(X) asm volatile("" : "+v"(X[0]), "+v"(X[1]), "+v"(X[2]), "+v"(X[3]), "+v"(X[4]), "+v"(X[5]))
#define TZW_TIED(d) asm volatile("" : "+v"(d[0][0]), "+v"(d[0][1]), "+v"(d[1][0]), "+v"(d[1][1]), "+v"(d[2][0]), "+v"(d[2][1]))
#define TZW_TIEU(u) asm volatile("" : "+v"(u[0]), "+v"(u[1]), "+v"(u[2]))

#ifdef TZW_STAMPS
// diagnostic build: s_memrealtime (100 MHz) at six points of a workgroup's life, wave 0, per (kernel shape slot, workgroup)
__device__ unsigned long long tzw_stamps[8][4096][16];   // [0..6] real time at the phase boundaries, [7] where, [8 + K] the core clock counter at stamp K
#define TZW_STAMP(K) if (tid == 0 && stamp_id < 4096) { tzw_stamps[(a.ncb & 3) | (EPI == EPI_LSTM ? 4 : 0)][stamp_id][K] = __builtin_amdgcn_s_memrealtime(); tzw_stamps[(a.ncb & 3) | (EPI == EPI_LSTM ? 4 : 0)][stamp_id][8 + (K)] = __builtin_amdgcn_s_memtime(); }
#else
#define TZW_STAMP(K)
#endif
// EPI: EPI_LSTM (NT = 4: columns [i | f | g | o] x 16 channels), EPI_POOL_ERR (NT = 3 or 4), EPI_RAW (NT = 4),
// EPI_LSTM3 (NT = 3: columns [i | g | o] x 16 of a stage image packed without the forget gate -- a level whose start cell
// state is +0 at every pixel, tz_prednet.hip measure_deadf: c = f * (+0) + i * g = (+0) + i * g for every non-NaN f, so the f
// columns are neither multiplied nor transformed; start values and biases stay 64 columns per block, column tile t of
// the kernel = gate column 16 (t + (t > 0)) of them), EPI_RAW3 (NT = 3: the first half of a split over that image: start values
// as EPI_LSTM3, rows of 3 Cout columns out; the second half <3, EPI_LSTM3, true, NOSAME> starts from those rows, a.ncols = 3 Cout).
// src[0]: the same-resolution source (multiple of 16 channels); src[1] (UPS): the half-resolution source.
// A gate convolution can also run as TWO launches (round 5, tz_prednet.hip "E-part ahead"; launches that cannot fill the
// chip): <4, EPI_RAW, false> over the same-resolution source alone, which leaves every output's chain as it stands behind
// the output transform in out0 ([pixel][column], per batch item), and <4, EPI_LSTM, true, NOSAME> which starts from those
// values (a.init with a.init_nstride per item) and walks the upsampled source only.  Same chains, same order, the
// intermediate is a float32 either way: same bits.  Both walk a PART of the stage image: a.wino_stride / a.wino_first.
template <int NT, int EPI, bool UPS, bool NOSAME = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_wino(const ConvArgs a) {
    static_assert(!NOSAME || UPS, "a launch without the same-resolution phase walks the upsampled source");
    static_assert((EPI != EPI_LSTM3 && EPI != EPI_RAW3) || NT == 3, "three gates");
    static_assert(EPI != EPI_LSTM || NT == 4, "four gates");
    static_assert(EPI != EPI_RAW3 || !UPS, "the first half of a split walks the same-resolution source");
    // (the four sections this kernel shares with k_wino2, which differs in its stage loops alone, are the text of the
    // tz_wino_*.inc.h files: the same object code here as when they stood in this body)
#define TZW_XOFF (NS * SLOT)   // the exchange areas sit behind the ring
#include "tz_wino_geometry.inc.h"
    // ---- the DMA stream.  Stage si goes into ring slot si mod 4: 2 KB of weights + one patch piece per wave = 3 DMA
    // instructions.  The stage loops are unrolled once per ring slot, so every LDS address below is a constant; the global
    // addresses are running scalar pointers (the first form recomputed them from the stage number: ~40 scalar instructions
    // per stage and wave, 3.4 % of the kernel -- TZW_ABL 32 against 8).
    // (the stage image is [column block][stage]: the weight pointer simply runs on from one item into the next)
    const float* wp = a.Wwino + (((long long)cb0 * SI + a.wino_first) * 16 + 2 * wv) * 256;   // weights of the next stage to issue
    const float* xp0 = a.src[0].p + (long long)n * a.src[0].nstride;                       // ... its quad of the same-resolution source
    const float* xp1 = UPS ? a.src[1].p + (long long)n * a.src[1].nstride : nullptr;       // ... of the upsampled one
    int si = 0;                                                                            // ... its number
    const unsigned wvw = (unsigned)(2 * wv) * 1024, wvp = WBYTES + (unsigned)wv * (PP * 16), wvu = WBYTES + P1BYTES + (unsigned)wv * (UP * 16);
#define TZW_ISSUE_W0(KI) dma_lanes(wp, lane16, sbase + (unsigned)(KI) * SLOT + wvw);
#define TZW_ISSUE_W1(KI) dma_lanes(wp + 256, lane16, sbase + (unsigned)(KI) * SLOT + wvw + 1024);
#define TZW_ISSUE_P(KI)                                                                                                     \
    {                                                                                                                       \
        const unsigned so = sbase + (unsigned)(KI) * SLOT;                                                                  \
        if (!UPS || si < S1) {                                                                                              \
            dma_gather(xp0, poff, pmask, so + wvp);                                                                         \
            xp0 += 4;                                                                                                       \
        } else {                                                                                                            \
            dma_gather(xp1, uoff, umask, so + wvu);                                                                         \
            xp1 += 4;                                                                                                       \
        }                                                                                                                   \
        wp += 16 * 256;                                                                                                     \
        if (++si == S) {   /* on to the next item: the next column block's stage 0, the sources from their first quad */   \
            si = 0;                                                                                                         \
            wp += (SI - S) * (16 * 256);   /* (a launch over a part of the stages skips the rest of the block's) */          \
            xp0 -= 4 * S1;                                                                                                  \
            if (UPS) xp1 -= 4 * (S - S1);                                                                                   \
        }                                                                                                                   \
    }
#define TZW_ISSUE_TO(KI) { TZW_ISSUE_W0(KI) TZW_ISSUE_W1(KI) TZW_ISSUE_P(KI) }
    // zero the patch areas once: the slots of out-of-image pixels are never written by the DMA (a tile whose halo lies
    // inside the image has none)
    const bool interior = ty0 >= 2 && tx0 >= 2 && ty0 + 18 <= a.H && tx0 + 18 <= a.W;
    if (!interior)
    for (int i = tid; i < NS * ((P1BYTES + P2BYTES) / 16); i += 512) {
        const int sl = i / ((P1BYTES + P2BYTES) / 16), o = i - sl * ((P1BYTES + P2BYTES) / 16);
        *(f32x4*)(smem + sl * SLOT + WBYTES + o * 16) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    const int nlead = LEAD;   // (S >= 4: sources are multiples of 16 channels)
    TZW_ISSUE_TO(0)
    TZW_ISSUE_TO(1)
    if (LEAD > 2) TZW_ISSUE_TO(2)

    // A address of this lane: tile r = (tyl, txl) of quadrant mt, channel g of the quad, first of the wave's three rows
    const int tyl = r >> 2, txl = r & 3;
    const unsigned abase = WBYTES + (unsigned)(((8 * (mt >> 1) + 2 * tyl + ph) * WPW + 4 * (mt & 1) + txl) * 16 + 4 * g);
    const unsigned ubase = WBYTES + P1BYTES + (unsigned)(((4 * (mt >> 1) + tyl + ph) * WLW + 4 * (mt & 1) + txl) * 16 + 4 * g);
    const unsigned bbase = (unsigned)(8 * ph) * 1024 + lane16;
    // LDS read addresses, one register set for the whole kernel: weights of slots 0, 1 from wbL and of slots 2, 3 from wbH (the
    // 16-bit immediate of ds_read_b128 covers a slot and a half), patch planes per slot (ds_read2 immediates are 8 bits)
    const unsigned wbL = sbase + bbase, wbH = wbL + 2 * SLOT;
    unsigned adA[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) adA[k] = sbase + (unsigned)k * SLOT + abase;
#include "tz_wino_transform.inc.h"

    // stages 0 and 1 landed for everyone (from the second item on the last stage of the item before has seen to that)
    if (nlead == LEAD) wait_vm_stages<LEAD - 2>();
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll 1
    for (int it = 0; it < ipw; ++it) {
    const int cb = cb0 + it;
    const bool more = it + 1 < ipw;   // (uniform) the DMA stream runs on into another item
    // (the pixel offsets of the output transform and of the epilogue do not depend on the item: hoisted out of this loop they
    // sat in 16 registers through every stage loop and were spilled to scratch; they are made to depend on this)
    int per_item = 0;
    asm volatile("" : "+s"(per_item));
    f32x4 D[8][4];   // (first written by the first stage of the item: mfma_first)
    TZW_STAMP(1)
    float V0[8], V1[8];
    f32x4 B[8];
    if (!NOSAME) {
        {
            f32x2 d[3][2];
            read_d(adA[0], d);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(d[0][0]), "+v"(d[0][1]), "+v"(d[1][0]), "+v"(d[1][1]), "+v"(d[2][0]), "+v"(d[2][1]) : : "memory");
            transform(d, V0);
            TZW_TIE8(V0);
        }
        // the weight reads run as one continuous stream, four positions ahead, across the stage boundaries
        B[0] = lds_read16<0>(wbL);
        B[1] = lds_read16<1024>(wbL);
        B[2] = lds_read16<2048>(wbL);
        B[3] = lds_read16<3072>(wbL);
    }
    int s = 0;   // (its ring slot is s mod 4 = the position in the unrolled loop body)
    // One stage of a wave: 8 positions x NT column tiles.  The LDS queue is in order, so every wait is a count:
    //   pos 0, 1  wait 3 (the three younger weight reads); behind pos 1 the patch reads of the NEXT stage (NA instructions)
    //   pos 2-5   wait 3 + NA
    //   pos 6     wait 3: the patch reads are done -> (phase 1) transform for the next stage
    //   pos 4-7   issue B[0..3] of the next stage from the next slot
// TZW_ABL (diagnostic builds, WRONG results, scripts/gpu_wino_ab.sh): 1 no barrier in the loops; 2 no patch reads / transform;
// 4 no weight reads; 8 no DMA in the loops; 16 (with 8) every stage loop twice
#ifndef TZW_ABL
#define TZW_ABL 0
#endif
#define TZW_WAIT(P, N) if (!(TZW_ABL & 4)) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(B[P]) : : "memory")
#ifndef TZW_ISSUE_AT
#define TZW_ISSUE_AT 1
#endif
#define TZW_ISSUE_HERE(K, AT)                                                                                               \
        if (TZW_ISSUE_AT == (AT) && !(TZW_ABL & 8) && (s + LEAD < S || more)) TZW_ISSUE_TO(((K) + LEAD) % NS)                         \
        if (TZW_ISSUE_AT == 10 + (AT) - 1 && !(TZW_ABL & 8) && (s + LEAD < S || more)) TZW_ISSUE_W0(((K) + LEAD) % NS)                \
        if (TZW_ISSUE_AT == 10 + (AT) - 2 && !(TZW_ABL & 8) && (s + LEAD < S || more)) TZW_ISSUE_W1(((K) + LEAD) % NS)                \
        if (TZW_ISSUE_AT == 10 + (AT) - 3 && !(TZW_ABL & 8) && (s + LEAD < S || more)) TZW_ISSUE_P(((K) + LEAD) % NS)
#define TZW_STAGE_HEAD(K)                                                                                                   \
        TZW_ISSUE_HERE(K, 0)                                                                                                \
        constexpr int KN = ((K) + 1) % NS;                                    /* the next stage's slot */                   \
        const unsigned wb = ((K) & 2) ? wbH : wbL, wn = (KN & 2) ? wbH : wbL;                                               \
        constexpr int WO = ((K) & 1) * SLOT, WN = (KN & 1) * SLOT;            /* ... folded into the read immediates */
#define TZW_STAGE_TAIL                                                                                                      \
        if (s + LEAD < S || more) wait_vm_stages<LEAD - 2>();                                                               \
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                               \
        if (!(TZW_ABL & 1)) __builtin_amdgcn_s_barrier();                                                                   \
        ++s;
#define TZW_MMF(F, ACC, P, AV)                                                                                              \
        _Pragma("unroll") for (int t = 0; t < NT; ++t) F(ACC[t], AV, B[P][t]);
#define TZW_MM(ACC, P, AV) TZW_MMF(mfma_acc, ACC, P, AV)
#define TZW_STAGE1(K, VC, VN) TZW_STAGE1_(K, VC, VN, mfma_acc)
#define TZW_STAGE1_(K, VC, VN, F)                                                                                           \
    {                                                                                                                       \
        TZW_STAGE_HEAD(K)                                                                                                   \
        f32x2 d[3][2];                                                                                                      \
        TZW_WAIT(0, 3); TZW_MMF(F, D[0], 0, VC[0]) B[4] = lds_read16<WO + 4 * 1024>(wb);                                        \
        TZW_ISSUE_HERE(K, 1)                                                                                                \
        TZW_WAIT(1, 3); TZW_MMF(F, D[1], 1, VC[1]) B[5] = lds_read16<WO + 5 * 1024>(wb);                                        \
        TZW_ISSUE_HERE(K, 2)                                                                                                \
        if (!(TZW_ABL & 2)) read_d(adA[KN], d);                                                                             \
        TZW_WAIT(2, 9); TZW_MMF(F, D[2], 2, VC[2]) B[6] = lds_read16<WO + 6 * 1024>(wb);                                        \
        TZW_ISSUE_HERE(K, 3)                                                                                                \
        TZW_WAIT(3, 9); TZW_MMF(F, D[3], 3, VC[3]) B[7] = lds_read16<WO + 7 * 1024>(wb);                                        \
        TZW_ISSUE_HERE(K, 4)                                                                                                \
        TZW_WAIT(4, 9); TZW_MMF(F, D[4], 4, VC[4]) B[0] = lds_read16<WN>(wn);                                                   \
        TZW_WAIT(5, 9); TZW_MMF(F, D[5], 5, VC[5]) B[1] = lds_read16<WN + 1024>(wn);                                            \
        TZW_WAIT(6, 3); TZW_MMF(F, D[6], 6, VC[6]) B[2] = lds_read16<WN + 2048>(wn);                                            \
        /* the patch reads have arrived (empty asm: nothing is computed with d before here) and the transform is done */   \
        /* HERE, not sunk to its first use right in front of an asm MFMA                                              */   \
        if (!(TZW_ABL & 2)) { TZW_TIED(d); transform(d, VN); }                                                              \
        else { _Pragma("unroll") for (int q = 0; q < 8; ++q) VN[q] = VC[q]; }                                               \
        TZW_TIE8(VN);                                                                                                       \
        TZW_WAIT(7, 3); TZW_MMF(F, D[7], 7, VC[7]) B[3] = lds_read16<WN + 3072>(wn);                                            \
        TZW_STAGE_TAIL                                                                                                      \
    }
    if (!NOSAME) {
#pragma unroll 1
    for (int rep = 0; rep < ((TZW_ABL & 16) ? 2 : 1); ++rep) {   // (ablation 16, with 8: every loop twice -> time per stage)
    if (TZW_ABL & 16) s = 0;
    if (rep == 0) {    // the first block of an item: its first stage starts the chains
        TZW_STAGE1_(0, V0, V1, mfma_first)
        TZW_STAGE1(1, V1, V0)
        TZW_STAGE1(2, V0, V1)
        TZW_STAGE1(3, V1, V0)
    }
#pragma unroll 1
    while (s < S1) {   // one 16-channel block = four stages = once round the ring
        TZW_STAGE1(0, V0, V1)
        TZW_STAGE1(1, V1, V0)
        TZW_STAGE1(2, V0, V1)
        TZW_STAGE1(3, V1, V0)
    }
    }
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // the last MFMAs have written their accumulators
    }
    TZW_STAMP(2)

#include "tz_wino_output.inc.h"

    TZW_STAMP(3)
    // ---- the upsampled source: every output's chain goes on with its collapsed taps.  Stage = one channel quad; the
    // wave's classes are (a = ph, b = 0, 1); weight sets in consumption order lp = 2 tap + b; A fragments = the 2 x 3
    // half-resolution pixels around the tile (rows ph + tpy, columns b + tpx)
    if (UPS) {
        unsigned udA[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) udA[k] = sbase + (unsigned)k * SLOT + ubase;
        auto read_u = [&](unsigned ad, f32x2 (&u)[3]) {
            u[0] = lds_read2<0, 4>(ad);             // (row 0, columns 0, 1)
            u[1] = lds_read2<8, WLW * 4>(ad);        // (row 0, column 2), (row 1, column 0)
            u[2] = lds_read2<WLW * 4 + 4, WLW * 4 + 8>(ad);   // (row 1, columns 1, 2)
        };
        // (the fragments stay where the reads put them -- pairs; a copy into scalars was a register move per stage behind an
        // asm read, which tests/test_build_guard.py does not let through)
        f32x2 A0[3], A1[3];
        {
            read_u(udA[0], A0);   // (S1 is a multiple of 4: the first stage of this phase sits in slot 0)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(A0[0]), "+v"(A0[1]), "+v"(A0[2]) : : "memory");
            // (the weight stream was drained by that wait: restart it)
            B[0] = lds_read16<0>(wbL);
            B[1] = lds_read16<1024>(wbL);
            B[2] = lds_read16<2048>(wbL);
            B[3] = lds_read16<3072>(wbL);
        }
        // lp = 2 tap + b: tap = (tpy, tpx) -> A[3 tpy + b + tpx]  (A[q] = fragment pair q >> 1, half q & 1)
#define TZW_STAGE2(K, AC, AN)                                                                                               \
    {                                                                                                                       \
        TZW_STAGE_HEAD(K)                                                                                                   \
        TZW_WAIT(0, 3); TZW_MM(Y[0], 0, AC[0][0]) B[4] = lds_read16<WO + 4 * 1024>(wb);                                     \
        TZW_ISSUE_HERE(K, 1)                                                                                                \
        TZW_WAIT(1, 3); TZW_MM(Y[1], 1, AC[0][1]) B[5] = lds_read16<WO + 5 * 1024>(wb);                                     \
        TZW_ISSUE_HERE(K, 2)                                                                                                \
        if (!(TZW_ABL & 2)) read_u(udA[KN], AN);                                                                            \
        TZW_WAIT(2, 6); TZW_MM(Y[0], 2, AC[0][1]) B[6] = lds_read16<WO + 6 * 1024>(wb);                                     \
        TZW_ISSUE_HERE(K, 3)                                                                                                \
        TZW_WAIT(3, 6); TZW_MM(Y[1], 3, AC[1][0]) B[7] = lds_read16<WO + 7 * 1024>(wb);                                     \
        TZW_ISSUE_HERE(K, 4)                                                                                                \
        TZW_WAIT(4, 6); TZW_MM(Y[0], 4, AC[1][1]) B[0] = lds_read16<WN>(wn);                                                \
        TZW_WAIT(5, 6); TZW_MM(Y[1], 5, AC[2][0]) B[1] = lds_read16<WN + 1024>(wn);                                         \
        TZW_WAIT(6, 3); TZW_MM(Y[0], 6, AC[2][0]) B[2] = lds_read16<WN + 2048>(wn);                                         \
        /* the patch reads have arrived (they are older than the three weight reads that wait left outstanding) */          \
        if (TZW_ABL & 2) { AN[0] = AC[0]; AN[1] = AC[1]; AN[2] = AC[2]; }                                                   \
        TZW_TIEU(AN);                                                                                                       \
        TZW_WAIT(7, 3); TZW_MM(Y[1], 7, AC[2][1]) B[3] = lds_read16<WN + 3072>(wn);                                         \
        TZW_STAGE_TAIL                                                                                                      \
    }
#pragma unroll 1
        for (int rep = 0; rep < ((TZW_ABL & 16) ? 2 : 1); ++rep) {
        if (TZW_ABL & 16) s = S1;
#pragma unroll 1
        while (s < S) {
            TZW_STAGE2(0, A0, A1)
            TZW_STAGE2(1, A1, A0)
            TZW_STAGE2(2, A0, A1)
            TZW_STAGE2(3, A1, A0)
        }
        }
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads issued for a stage past the end
    TZW_STAMP(4)
#undef TZW_STAGE2
#undef TZW_STAGE1
#undef TZW_STAGE1_
#undef TZW_MMF
#undef TZW_MM
#undef TZW_STAGE_TAIL
#undef TZW_STAGE_HEAD
#undef TZW_ISSUE_TO
#undef TZW_ISSUE_W0
#undef TZW_ISSUE_W1
#undef TZW_ISSUE_P
#undef TZW_ISSUE_HERE
#undef TZW_WAIT
#undef TZW_COLT

#include "tz_wino_epilogue.inc.h"
#undef TZW_XOFF
#ifdef TZW_STAMPS
    TZW_STAMP(5)
    if (more) {
        ++stamp_id;
        TZW_STAMP(0)   // (of the next item)
    }
#endif
    }   // items
}

// k_wino2: the three-tile forms of k_wino (NT = 3) with a stage of TWO consecutive channel quads.  A stage carries a fixed
// cost -- the barrier, the counted vmcnt wait, the DMA issue burst, the loop bookkeeping -- that does not shrink with the number
// of column tiles; here it is paid once per 48 MFMAs of a wave instead of once per 24.  Everything outside the stage loops is
// k_wino's text (the tz_wino_*.inc.h sections); every chain is still one fmaf chain over the channels in ascending order
// (within a stage all of quad q is multiplied before quad q + 1), so the bits are k_wino's.
//   Stage image (tz_prednet.hip choose_wino_forms): per channel quad 12 KB, [ph][read 6][lane][4]: fragment v = 3 p + t (position p of the wave's 8,
//   column tile t) sits in read v >> 2, slot v & 3 -- no fourth column tile is stored, DMA'd or read.  A double stage = 24 KB.
//   Ring: 3 double slots [weights 24 KB | two same-resolution planes | two half-resolution planes] = 38,400 bytes each, the DMA
//   stream 2 double stages ahead; the stage loops are unrolled once per slot (every LDS address a constant), so the executed
//   stages of either source are a multiple of 6 quads and wino_first / wino_stride are even (launch_wino checks).
//   Per wave and double stage: 48 MFMAs, 12 ds_read_b128 of weights in one continuous stream (register k of 6 is read again
//   right behind the last position that multiplies from it), the patch reads and B^T d B of the next double stage (one quad
//   under each half), 5 LDS-DMA instructions (3 KB of weights, two patch pieces) behind the first position, one vmcnt wait,
//   one barrier.
// Ordering (cdna_hip_programming.md: read a staged buffer one phase AFTER the wait that retires it), stage n in slot n mod 3:
//   RAW  stage n + 2 is issued during stage n by every wave and is the youngest thing the wave has in flight at the tail of
//        stage n, where it waits vmcnt(0) in front of the barrier; the first reads of slot (n + 2) mod 3 -- the patch reads
//        of stage n + 1, and the weight reads behind its second half -- come behind that barrier.
//   WAR  slot (n + 2) mod 3 = (n - 1) mod 3 was last read for stage n - 1: its planes during stage n - 2, its weights by the
//        reads issued up to the first half of stage n - 1, all of them consumed -- so returned -- by MFMAs of stage n - 1,
//        in front of that stage's barrier.  The DMA into it is issued behind that barrier by every wave.
//   The lgkmcnt immediates are counts of younger reads in the in-order LDS queue (NA = patch reads of a half: 6 or 3):
//        position 0: 5, 1: 4, 2: 4 + NA, 4: 5 + NA, 5: 4 + NA, 6: 3 (the patch reads are done too); 3 and 7 need no new register.
namespace tzw {
static constexpr int NS2 = 3;                                   // double slots of the ring, the stream 2 double stages ahead
static constexpr int W3BYTES = 12 * 1024;                       // dense weights of a channel quad
static constexpr int DWBYTES = 2 * W3BYTES;
static constexpr int DSLOT = DWBYTES + 2 * P1BYTES + 2 * P2BYTES;   // 38,400
static constexpr int LDS2_BYTES = NS2 * DSLOT + XBYTES;             // 147,968
static_assert(LDS2_BYTES <= 160 * 1024, "LDS of a CU");
static_assert(DSLOT + DWBYTES <= 65536, "the 16-bit immediate of ds_read_b128 reaches slot 1's weights from slot 0's base");
}  // namespace tzw

template <int EPI, bool UPS, bool NOSAME = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_wino2(const ConvArgs a) {
    constexpr int NT = 3;
    static_assert(!NOSAME || UPS, "a launch without the same-resolution phase walks the upsampled source");
    static_assert(EPI == EPI_LSTM3 || EPI == EPI_RAW3 || EPI == EPI_POOL_ERR, "the three-tile forms");
    static_assert(EPI != EPI_RAW3 || !UPS, "the first half of a split walks the same-resolution source");
    static_assert(EPI != EPI_POOL_ERR || !UPS, "A convolutions have one source");
#define TZW_XOFF (NS2 * DSLOT)
#include "tz_wino_geometry.inc.h"
    // ---- the DMA stream.  Double stage n (quads 2 n, 2 n + 1 of the walk) goes into ring slot n mod 3.  The dense image is one
    // stream of 3072 floats a quad: wave wv moves floats [768 wv, 768 wv + 768) of a double stage's 6144 with three
    // instructions, then its piece of the two quads' patch planes: 5 LDS-DMA instructions per wave and double stage.
    const float* wp = a.Wwino + ((long long)cb0 * SI + a.wino_first) * 3072 + 768 * wv;   // weights of the next double stage to issue
    const float* xp0 = a.src[0].p + (long long)n * a.src[0].nstride;                   // ... its first quad of the same-resolution source
    const float* xp1 = UPS ? a.src[1].p + (long long)n * a.src[1].nstride : nullptr;   // ... of the upsampled one
    int si = 0;                                                                        // ... its first quad's number
    const unsigned wvw = (unsigned)wv * 3072, wvp = DWBYTES + (unsigned)wv * (PP * 16), wvu = DWBYTES + 2 * P1BYTES + (unsigned)wv * (UP * 16);
#define TZW2_ISSUE_TO(KI)                                                                                                   \
    {                                                                                                                       \
        const unsigned so = sbase + (unsigned)(KI) * DSLOT;                                                                 \
        dma_lanes(wp, lane16, so + wvw);                                                                                    \
        dma_lanes(wp + 256, lane16, so + wvw + 1024);                                                                       \
        dma_lanes(wp + 512, lane16, so + wvw + 2048);                                                                       \
        if (!UPS || si < S1) {   /* (S1 is even: both quads of a double stage are of one source) */                         \
            dma_gather(xp0, poff, pmask, so + wvp);                                                                         \
            dma_gather(xp0 + 4, poff, pmask, so + wvp + P1BYTES);                                                           \
            xp0 += 8;                                                                                                       \
        } else {                                                                                                            \
            dma_gather(xp1, uoff, umask, so + wvu);                                                                         \
            dma_gather(xp1 + 4, uoff, umask, so + wvu + P2BYTES);                                                           \
            xp1 += 8;                                                                                                       \
        }                                                                                                                   \
        wp += 2 * 3072;                                                                                                     \
        si += 2;                                                                                                            \
        if (si == S) {   /* on to the next item: the next column block's first executed quad, the sources from the start */ \
            si = 0;                                                                                                         \
            wp += (SI - S) * 3072;                                                                                          \
            xp0 -= 4 * S1;                                                                                                  \
            if (UPS) xp1 -= 4 * (S - S1);                                                                                   \
        }                                                                                                                   \
    }
    // zero the patch areas once: the slots of out-of-image pixels are never written by the DMA
    const bool interior = ty0 >= 2 && tx0 >= 2 && ty0 + 18 <= a.H && tx0 + 18 <= a.W;
    if (!interior)
    for (int i = tid; i < NS2 * ((DSLOT - DWBYTES) / 16); i += 512) {
        const int sl = i / ((DSLOT - DWBYTES) / 16), o = i - sl * ((DSLOT - DWBYTES) / 16);
        *(f32x4*)(smem + sl * DSLOT + DWBYTES + o * 16) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    TZW2_ISSUE_TO(0)   // (S >= 6: at least three double stages)
    TZW2_ISSUE_TO(1)

    // A address of this lane: tile r = (tyl, txl) of quadrant mt, channel g of the quad, first of the wave's three rows
    const int tyl = r >> 2, txl = r & 3;
    const unsigned abase = DWBYTES + (unsigned)(((8 * (mt >> 1) + 2 * tyl + ph) * WPW + 4 * (mt & 1) + txl) * 16 + 4 * g);
    const unsigned ubase = DWBYTES + 2 * P1BYTES + (unsigned)(((4 * (mt >> 1) + tyl + ph) * WLW + 4 * (mt & 1) + txl) * 16 + 4 * g);
    // weights: the wave's six reads of a quad sit at ph * 6 KB; slots 0, 1 are read from wbL, slot 2 from wbH
    const unsigned wbL = sbase + (unsigned)ph * (W3BYTES / 2) + lane16, wbH = wbL + 2 * DSLOT;
    unsigned adA[NS2][2];   // patch planes per slot and half (ds_read2 immediates are 8 bits)
#pragma unroll
    for (int k = 0; k < NS2; ++k) {
        adA[k][0] = sbase + (unsigned)k * DSLOT + abase;
        adA[k][1] = adA[k][0] + P1BYTES;
    }
#include "tz_wino_transform.inc.h"

    // double stages 0 and 1 landed for everyone (from the second item on the last stage of the item before has seen to that)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll 1
    for (int it = 0; it < ipw; ++it) {
    const int cb = cb0 + it;
    const bool more = it + 1 < ipw;   // (uniform) the DMA stream runs on into another item
    int per_item = 0;                 // (see k_wino: keeps the pixel offsets of the serial sections out of the stage loops)
    asm volatile("" : "+s"(per_item));
    f32x4 D[8][NT];   // (first written by the first quad of the item: mfma_first)
    // B^T d B of the quads in flight, three sets in rotation: a stage multiplies (first half, second half) = (X, Y), (Z, X), (Y, Z)
    // and computes the next stage's into the set that is free -- period 3, as the ring
    float VX[8], VY[8], VZ[8];
    f32x4 B[6];
    int s = 0;   // quads done; the ring slot of a double stage is its position in the unrolled loop body
#define TZW2_WAIT(R, N) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(B[R]) : : "memory")
#define TZW2_MM(F, ACC, P, AV)                                                                                              \
        _Pragma("unroll") for (int t = 0; t < NT; ++t) F(ACC[t], AV, B[(3 * (P) + t) >> 2][(3 * (P) + t) & 3]);
#define TZW2_ISSUE_HERE(K) if (s + 4 < S || more) TZW2_ISSUE_TO(((K) + 2) % NS2)
    // every wave issued the 5 LDS-DMA instructions of the stage two ahead (if there is one) in front of this: they are the
    // youngest it has in flight, and the next stage reads that slot
#define TZW2_STAGE_TAIL                                                                                                     \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                                    \
        __builtin_amdgcn_s_barrier();                                                                                       \
        s += 2;
    // where slot K's weights are read from: base register and immediate
#define TZW2_WB(K) (((K) & 2) ? wbH : wbL)
#define TZW2_WO(K) (((K) & 1) * DSLOT)
    // one half of a same-resolution double stage: quad VC from the six registers, the next reads of each register from
    // (WR, WRO), the next stage's patch plane ADN transformed into VN
#define TZW2_HALF1(F, VC, VN, ADN, WR, WRO, ISSUE)                                                                          \
    {                                                                                                                       \
        f32x2 d[3][2];                                                                                                      \
        TZW2_WAIT(0, 5);  TZW2_MM(F, D[0], 0, VC[0])                                                                        \
        ISSUE                                                                                                               \
        TZW2_WAIT(1, 4);  TZW2_MM(F, D[1], 1, VC[1]) B[0] = lds_read16<(WRO)>(WR);                                          \
        read_d(ADN, d);                                                                                                     \
        TZW2_WAIT(2, 10); TZW2_MM(F, D[2], 2, VC[2]) B[1] = lds_read16<(WRO) + 1024>(WR);                                   \
                          TZW2_MM(F, D[3], 3, VC[3]) B[2] = lds_read16<(WRO) + 2048>(WR);                                   \
        TZW2_WAIT(3, 11); TZW2_MM(F, D[4], 4, VC[4])                                                                        \
        TZW2_WAIT(4, 10); TZW2_MM(F, D[5], 5, VC[5]) B[3] = lds_read16<(WRO) + 3072>(WR);                                   \
        TZW2_WAIT(5, 3);  TZW2_MM(F, D[6], 6, VC[6]) B[4] = lds_read16<(WRO) + 4096>(WR);                                   \
        /* the patch reads have arrived (they are older than the three reads that wait left outstanding); the transform is */ \
        /* done HERE, not sunk to its first use right in front of an asm MFMA                                              */ \
        TZW_TIED(d);                                                                                                        \
        transform(d, VN);                                                                                                   \
        TZW_TIE8(VN);                                                                                                       \
                          TZW2_MM(F, D[7], 7, VC[7]) B[5] = lds_read16<(WRO) + 5120>(WR);                                   \
    }
#define TZW2_STAGE1(K, VA, VB, VNA, VNB, F)                                                                                 \
    {                                                                                                                       \
        constexpr int KN = ((K) + 1) % NS2;                                                                                 \
        TZW2_HALF1(F, VA, VNA, adA[KN][0], TZW2_WB(K), TZW2_WO(K) + W3BYTES, TZW2_ISSUE_HERE(K))                            \
        TZW2_HALF1(mfma_acc, VB, VNB, adA[KN][1], TZW2_WB(KN), TZW2_WO(KN), )                                               \
        TZW2_STAGE_TAIL                                                                                                     \
    }
    if (!NOSAME) {
        {
            f32x2 d[3][2], e[3][2];
            read_d(adA[0][0], d);
            read_d(adA[0][1], e);
            asm volatile("s_waitcnt lgkmcnt(0)"
                         : "+v"(d[0][0]), "+v"(d[0][1]), "+v"(d[1][0]), "+v"(d[1][1]), "+v"(d[2][0]), "+v"(d[2][1]), "+v"(e[0][0]), "+v"(e[0][1]),
                           "+v"(e[1][0]), "+v"(e[1][1]), "+v"(e[2][0]), "+v"(e[2][1])
                         :
                         : "memory");
            transform(d, VX);
            transform(e, VY);
            TZW_TIE8(VX);
            TZW_TIE8(VY);
        }
        // the weight reads run as one continuous stream across the halves and the stage boundaries
        B[0] = lds_read16<0>(wbL);
        B[1] = lds_read16<1024>(wbL);
        B[2] = lds_read16<2048>(wbL);
        B[3] = lds_read16<3072>(wbL);
        B[4] = lds_read16<4096>(wbL);
        B[5] = lds_read16<5120>(wbL);
        // the first three double stages of an item: its first quad starts the chains
        TZW2_STAGE1(0, VX, VY, VZ, VX, mfma_first)
        TZW2_STAGE1(1, VZ, VX, VY, VZ, mfma_acc)
        TZW2_STAGE1(2, VY, VZ, VX, VY, mfma_acc)
#pragma unroll 1
        while (s < S1) {   // six quads = once round the ring
            TZW2_STAGE1(0, VX, VY, VZ, VX, mfma_acc)
            TZW2_STAGE1(1, VZ, VX, VY, VZ, mfma_acc)
            TZW2_STAGE1(2, VY, VZ, VX, VY, mfma_acc)
        }
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");   // the last MFMAs have written their accumulators
    }

#include "tz_wino_output.inc.h"

    // ---- the upsampled source, as in k_wino: a quad = 4 classes x 4 taps of collapsed weights, the wave's 8 sets in consumption
    // order lp = 2 tap + b, A fragments = the 2 x 3 half-resolution pixels around the tile, three sets in rotation
    if (UPS) {
        unsigned udA[NS2][2];
#pragma unroll
        for (int k = 0; k < NS2; ++k) {
            udA[k][0] = sbase + (unsigned)k * DSLOT + ubase;
            udA[k][1] = udA[k][0] + P2BYTES;
        }
        auto read_u = [&](unsigned ad, f32x2 (&u)[3]) {
            u[0] = lds_read2<0, 4>(ad);             // (row 0, columns 0, 1)
            u[1] = lds_read2<8, WLW * 4>(ad);        // (row 0, column 2), (row 1, column 0)
            u[2] = lds_read2<WLW * 4 + 4, WLW * 4 + 8>(ad);   // (row 1, columns 1, 2)
        };
        f32x2 AX[3], AY[3], AZ[3];
        {
            read_u(udA[0][0], AX);   // (S1 is a multiple of 6: the first double stage of this phase sits in slot 0)
            read_u(udA[0][1], AY);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(AX[0]), "+v"(AX[1]), "+v"(AX[2]), "+v"(AY[0]), "+v"(AY[1]), "+v"(AY[2]) : : "memory");
            // (the weight stream was drained by that wait: restart it)
            B[0] = lds_read16<0>(wbL);
            B[1] = lds_read16<1024>(wbL);
            B[2] = lds_read16<2048>(wbL);
            B[3] = lds_read16<3072>(wbL);
            B[4] = lds_read16<4096>(wbL);
            B[5] = lds_read16<5120>(wbL);
        }
        // lp = 2 tap + b: tap = (tpy, tpx) -> A[3 tpy + b + tpx]  (A[q] = fragment pair q >> 1, half q & 1)
#define TZW2_HALF2(AC, AN, ADN, WR, WRO, ISSUE)                                                                             \
    {                                                                                                                       \
        TZW2_WAIT(0, 5); TZW2_MM(mfma_acc, Y[0], 0, AC[0][0])                                                               \
        ISSUE                                                                                                               \
        TZW2_WAIT(1, 4); TZW2_MM(mfma_acc, Y[1], 1, AC[0][1]) B[0] = lds_read16<(WRO)>(WR);                                 \
        read_u(ADN, AN);                                                                                                    \
        TZW2_WAIT(2, 7); TZW2_MM(mfma_acc, Y[0], 2, AC[0][1]) B[1] = lds_read16<(WRO) + 1024>(WR);                          \
                         TZW2_MM(mfma_acc, Y[1], 3, AC[1][0]) B[2] = lds_read16<(WRO) + 2048>(WR);                          \
        TZW2_WAIT(3, 8); TZW2_MM(mfma_acc, Y[0], 4, AC[1][1])                                                               \
        TZW2_WAIT(4, 7); TZW2_MM(mfma_acc, Y[1], 5, AC[2][0]) B[3] = lds_read16<(WRO) + 3072>(WR);                          \
        TZW2_WAIT(5, 3); TZW2_MM(mfma_acc, Y[0], 6, AC[2][0]) B[4] = lds_read16<(WRO) + 4096>(WR);                          \
        /* the patch reads have arrived (they are older than the three reads that wait left outstanding) */                 \
        TZW_TIEU(AN);                                                                                                       \
                         TZW2_MM(mfma_acc, Y[1], 7, AC[2][1]) B[5] = lds_read16<(WRO) + 5120>(WR);                          \
    }
#define TZW2_STAGE2(K, AA, AB, ANA, ANB)                                                                                    \
    {                                                                                                                       \
        constexpr int KN = ((K) + 1) % NS2;                                                                                 \
        TZW2_HALF2(AA, ANA, udA[KN][0], TZW2_WB(K), TZW2_WO(K) + W3BYTES, TZW2_ISSUE_HERE(K))                               \
        TZW2_HALF2(AB, ANB, udA[KN][1], TZW2_WB(KN), TZW2_WO(KN), )                                                         \
        TZW2_STAGE_TAIL                                                                                                     \
    }
#pragma unroll 1
        while (s < S) {
            TZW2_STAGE2(0, AX, AY, AZ, AX)
            TZW2_STAGE2(1, AZ, AX, AY, AZ)
            TZW2_STAGE2(2, AY, AZ, AX, AY)
        }
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads issued for a stage past the end
#undef TZW2_STAGE2
#undef TZW2_HALF2
#undef TZW2_STAGE1
#undef TZW2_HALF1
#undef TZW2_WO
#undef TZW2_WB
#undef TZW2_STAGE_TAIL
#undef TZW2_ISSUE_HERE
#undef TZW2_MM
#undef TZW2_WAIT
#undef TZW2_ISSUE_TO
#undef TZW_COLT

#include "tz_wino_epilogue.inc.h"
#undef TZW_XOFF
    }   // items
}

// The dense image of k_wino2 from the three-tile image of pack_wino, quad by quad: [set 16][lane][4 column tiles, the fourth
// zero] -> [ph][read 6][lane][4], fragment v = 3 p + t of set 8 ph + p in read v >> 2, slot v & 3.  A permutation of the values
// k_wino and k_wino_ref read: a packing error cannot hide between them and k_wino2 (tests/test_gpu_wino2q.py).
__global__ __launch_bounds__(256) void k_dense_stages(const float* __restrict__ src, float* __restrict__ dst, long long nquads) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nquads * 3072; i += (long long)gridDim.x * blockDim.x) {
        const long long q = i / 3072;
        const int rem = (int)(i - q * 3072);
        const int ph = rem / 1536, rd = (rem % 1536) >> 8, lane = (rem & 255) >> 2, v = 4 * rd + (rem & 3);
        dst[i] = src[((q * 16 + 8 * ph + v / 3) * 64 + lane) * 4 + v % 3];
    }
}

// k_wino_ref: the same TZ-PA2 convolutions (and epilogues) as k_wino, written the plain way -- one thread per (tile, column
// group), every chain a loop of fmaf in the order the contract states -- as the device-side cross-check of the hand-scheduled
// kernel (tz_set_conv_impl(0), as k_conv3x3 is for k_conv16).  It reads the same packed stage image (pack_wino), so a packing
// error cannot hide between the two; ~50x slower.
//   EPI_LSTM: thread = (tile, channel of the column block): its four gate columns one after the other, then the cell update
//   EPI_POOL_ERR / EPI_RAW: thread = (tile, column)
template <int NT, int EPI, bool UPS>
__global__ __launch_bounds__(256) void k_wino_ref(const ConvArgs a) {
    const int TX = (a.W + 1) / 2, TY = (a.H + 1) / 2;
    const int gcols = EPI == EPI_LSTM ? 16 : 16 * NT;           // threads per tile and column block
    const long long nthreads = (long long)TX * TY * a.ncb * gcols;
    const int n = blockIdx.y;
    const int S1 = a.src[0].C >> 2, C0 = a.src[0].C;
    const int SR = S1 + (UPS ? a.src[1].C >> 2 : 0);            // stages of a column block in the image
    const float* x0 = a.src[0].p + (long long)n * a.src[0].nstride;
    const float* x1 = UPS ? a.src[1].p + (long long)n * a.src[1].nstride : nullptr;
    for (long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x; id < nthreads; id += (long long)gridDim.x * blockDim.x) {
        const int jc = (int)(id % gcols);
        long long q = id / gcols;
        const int cb = (int)(q % a.ncb);
        q /= a.ncb;
        const int tx = (int)(q % TX), ty = (int)(q / TX);
        float Yg[4][4];   // [gate or 0][output 2 a + b]
        const int ngate = EPI == EPI_LSTM ? 4 : 1;
        for (int gt = 0; gt < ngate; ++gt) {
            const int nt = EPI == EPI_LSTM ? gt : jc >> 4, j = jc & 15;
            const int col = cb * (16 * NT) + 16 * nt + j;
            float D[16];
            for (int p = 0; p < 16; ++p) D[p] = 0.0f;
            for (int c = 0; c < C0; ++c) {
                float d[4][4], t[4][4];
                for (int rr = 0; rr < 4; ++rr)
                    for (int cc = 0; cc < 4; ++cc) {
                        const int yy = 2 * ty - 1 + rr, xx = 2 * tx - 1 + cc;
                        d[rr][cc] = (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) ? x0[((long long)yy * a.W + xx) * a.src[0].pstride + c] : 0.0f;
                    }
                for (int rr = 0; rr < 4; ++rr) {
                    t[rr][0] = d[rr][0] - d[rr][2];
                    t[rr][1] = d[rr][1] + d[rr][2];
                    t[rr][2] = d[rr][2] - d[rr][1];
                    t[rr][3] = d[rr][1] - d[rr][3];
                }
                const float* wq = a.Wwino + ((((long long)cb * SR + (c >> 2)) * 16) * 64 + (c & 3) * 16 + j) * 4 + nt;
                for (int jj = 0; jj < 4; ++jj) {
                    const float v0 = t[0][jj] - t[2][jj], v1 = t[1][jj] + t[2][jj], v2 = t[2][jj] - t[1][jj], v3 = t[1][jj] - t[3][jj];
                    D[0 + jj] = fmaf(v0, wq[(0 + jj) * 256], D[0 + jj]);
                    D[4 + jj] = fmaf(v1, wq[(4 + jj) * 256], D[4 + jj]);
                    D[8 + jj] = fmaf(v2, wq[(8 + jj) * 256], D[8 + jj]);
                    D[12 + jj] = fmaf(v3, wq[(12 + jj) * 256], D[12 + jj]);
                }
            }
            float z0[4], z1[4];
            for (int i = 0; i < 4; ++i) {
                z0[i] = (D[4 * i] + D[4 * i + 1]) + D[4 * i + 2];
                z1[i] = (D[4 * i + 1] - D[4 * i + 2]) - D[4 * i + 3];
            }
            float in[4];
            for (int o = 0; o < 4; ++o) {
                const int y = 2 * ty + (o >> 1), x = 2 * tx + (o & 1);
                in[o] = a.init ? a.init[((long long)(y < a.H && x < a.W ? y * a.W + x : 0)) * a.ncols + col] : a.bias[col];
            }
            float* Y = Yg[gt];
            Y[0] = ((in[0] + z0[0]) + z0[1]) + z0[2];
            Y[1] = ((in[1] + z1[0]) + z1[1]) + z1[2];
            Y[2] = ((in[2] + z0[1]) - z0[2]) - z0[3];
            Y[3] = ((in[3] + z1[1]) - z1[2]) - z1[3];
            if (UPS) {   // channel quads ascending, the 4 taps of a quad, its 4 channels
                const int H2 = a.H >> 1, W2 = a.W >> 1, C1 = a.src[1].C;
                for (int o = 0; o < 4; ++o) {
                    const int ay = o >> 1, bx = o & 1;
                    float acc = Y[o];
                    for (int c0 = 0; c0 < C1; c0 += 4)
                        for (int tp = 0; tp < 4; ++tp) {
                            const int ly = ty - 1 + ay + (tp >> 1), lx = tx - 1 + bx + (tp & 1);
                            const bool inside = ly >= 0 && ly < H2 && lx >= 0 && lx < W2;
                            const float* wq = a.Wwino + ((((long long)cb * SR + S1 + (c0 >> 2)) * 16 + 8 * ay + 2 * tp + bx) * 64 + j) * 4 + nt;
                            for (int k = 0; k < 4; ++k) {
                                const float xv = inside ? x1[((long long)ly * W2 + lx) * a.src[1].pstride + c0 + k] : 0.0f;
                                acc = fmaf(xv, wq[k * 64], acc);
                            }
                        }
                    Y[o] = acc;
                }
            }
        }
        if (EPI == EPI_RAW) {
            float* on = a.out0 + (long long)n * a.out0_nstride;
            for (int o = 0; o < 4; ++o) {
                const int y = 2 * ty + (o >> 1), x = 2 * tx + (o & 1);
                if (y < a.H && x < a.W) on[((long long)y * a.W + x) * a.ncols + cb * (16 * NT) + jc] = Yg[0][o];
            }
        } else if (EPI == EPI_LSTM) {
            const int ch = cb * 16 + jc, R = a.Cout;
            float* o0 = a.out0 + (long long)n * a.out0_nstride;
            float* o1 = a.out1 ? a.out1 + (long long)n * a.out1_nstride : nullptr;
            for (int o = 0; o < 4; ++o) {
                const int y = 2 * ty + (o >> 1), x = 2 * tx + (o & 1);
                if (y >= a.H || x >= a.W) continue;
                const long long pix = (long long)y * a.W + x;
                const float cp = a.aux ? a.aux[pix * R + ch] : 0.0f;
                const float gi = tz_hard_sigmoid(Yg[0][o]), gf = tz_hard_sigmoid(Yg[1][o]), gg = tz_tanh(Yg[2][o]), go = tz_hard_sigmoid(Yg[3][o]);
                const float t1 = gf * cp;
                const float t2 = gi * gg;
                const float c = t1 + t2;
                const float rr = go * tz_tanh(c);
                o0[pix * R + ch] = rr;
                if (o1) o1[pix * R + ch] = c;
            }
        } else {   // EPI_POOL_ERR: the pooling window is the tile
            const int H2 = a.H >> 1, W2 = a.W >> 1, C = a.Cout, ch = cb * (16 * NT) + jc;
            if (ty < H2 && tx < W2 && ch < C) {
                float m = tz_relu(Yg[0][0]);
                for (int o = 1; o < 4; ++o) {
                    const float t = tz_relu(Yg[0][o]);
                    if (t > m) m = t;
                }
                const long long pp = (long long)ty * W2 + tx;
                const float h = a.aux[pp * C + ch];
                const float d1 = h - m, d2 = m - h;
                float* o = a.out0 + (long long)n * a.out0_nstride;
                o[pp * 2 * C + ch] = tz_relu(d1);
                o[pp * 2 * C + C + ch] = tz_relu(d2);
            }
        }
    }
}
