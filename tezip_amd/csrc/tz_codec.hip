// Delta / quantise / entropy-prep kernels and their inverses for gfx950 (MI355X).
// HBM-bound integer/byte work: wide coalesced accesses (16 B per lane where the layout
// allows), LDS-privatised histogram, grid-stride launches of ~8 blocks per CU.
// Reference semantics are cited per kernel (paths into /root/reference/src).
#include <algorithm>
#include <vector>

#include "tz_internal.h"

static constexpr int kBlocksPerCU = 8;
static constexpr int kCUs = 256;

static inline int grid_for(size_t work_items, int block) {
    size_t g = (work_items + block - 1) / block;
    size_t cap = (size_t)kCUs * kBlocksPerCU;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

typedef short short8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------- delta
// compress.py:292-314: d = (int)(pred_f32 * 255.0f) - orig ; frames flagged in zero_mask -> 0.
// Fast path: frame needs no padding (H==Hp, W==Wp): pred, orig and out share one flat index.  16-byte loads of pred, 8-byte
// loads of orig, 16-byte stores: tzk_delta takes it only for buffers on those boundaries.
__global__ __launch_bounds__(256) void k_delta_flat(const float4* __restrict__ pred, const uint2* __restrict__ orig,
                                                    const uint8_t* __restrict__ zero_mask, size_t n8,
                                                    unsigned frame_elems8, short8* __restrict__ out) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        float4 p0 = pred[2 * i], p1 = pred[2 * i + 1];
        uint2 o = orig[i];
        unsigned f = (unsigned)(i / frame_elems8);
        short8 r;
        if (zero_mask[f]) {
            r = (short8)(0);
        } else {
            r[0] = (short)((int)(p0.x * 255.0f) - (int)(o.x & 0xff));
            r[1] = (short)((int)(p0.y * 255.0f) - (int)((o.x >> 8) & 0xff));
            r[2] = (short)((int)(p0.z * 255.0f) - (int)((o.x >> 16) & 0xff));
            r[3] = (short)((int)(p0.w * 255.0f) - (int)(o.x >> 24));
            r[4] = (short)((int)(p1.x * 255.0f) - (int)(o.y & 0xff));
            r[5] = (short)((int)(p1.y * 255.0f) - (int)((o.y >> 8) & 0xff));
            r[6] = (short)((int)(p1.z * 255.0f) - (int)((o.y >> 16) & 0xff));
            r[7] = (short)((int)(p1.w * 255.0f) - (int)(o.y >> 24));
        }
        out[i] = r;
    }
}

// General path: crop of a padded prediction (pitch Wp*3).
__global__ __launch_bounds__(256) void k_delta_crop(const float* __restrict__ pred, const uint8_t* __restrict__ orig,
                                                    const uint8_t* __restrict__ zero_mask, size_t n, int H, int W,
                                                    int Hp, int Wp, int16_t* __restrict__ out) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t row = (size_t)W * 3, fe = (size_t)H * row, fp = (size_t)Hp * Wp * 3;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        size_t f = i / fe, r = i - f * fe;
        size_t y = r / row, xc = r - y * row;
        float p = pred[f * fp + y * (size_t)Wp * 3 + xc];
        out[i] = zero_mask[f] ? (int16_t)0 : (int16_t)((int)(p * 255.0f) - (int)orig[i]);
    }
}

int tzk_delta(tz_ctx* ctx, const float* pred, const uint8_t* orig, const uint8_t* d_zero_mask, int nframes, int H,
              int W, int Hp, int Wp, int16_t* out) {
    size_t n = (size_t)nframes * H * W * 3;
    if (n == 0) return TZ_OK;
    tz_prof_scope ps(ctx, TZP_DELTA);
    const bool aligned = ((((uintptr_t)pred | (uintptr_t)out) & 15) | ((uintptr_t)orig & 7)) == 0;
    if (H == Hp && W == Wp && ((size_t)H * W * 3) % 8 == 0 && aligned) {
        size_t n8 = n / 8;
        hipLaunchKernelGGL(k_delta_flat, dim3(grid_for(n8, 256)), dim3(256), 0, ctx->stream, (const float4*)pred,
                           (const uint2*)orig, d_zero_mask, n8, (unsigned)((size_t)H * W * 3 / 8), (short8*)out);
    } else {
        hipLaunchKernelGGL(k_delta_crop, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, pred, orig, d_zero_mask,
                           n, H, W, Hp, Wp, out);
    }
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------------------- block-private symbol histogram
// compress.py:354 (bincount of the symbols 1600 - sd).  The symbols of a prediction residual pile up
// on a handful of values around the centre c (1600, or 0 without the offset), so a plain LDS
// histogram spends its time serialising atomics on the same few words (rounds 1-2: one copy per wave,
// 4.7 M bank-conflict cycles per 7.9 M LDS operations, the spatial-delta kernel ran at 41 % of HBM
// against 74 % without the histogram).  Now:
//   * the centre symbol never touches the bins: a wave counts it with a ballot into a scalar register;
//   * the 128 bins around c have 8 copies per wave, interleaved as [bin][copy] with copy = lane & 7, so
//     that a wave's 64 lanes spread over all 32 banks (bank = (bin % 4) * 8 + copy) and only the ~2 lanes
//     that share copy AND bin % 4 meet in a bank;
//   * everything else (rare) goes to one full-range copy per block.
// flush() folds the copies into the full-range one and adds its non-zero bins to the global counters.
static constexpr int HC_HALF = 64, HC_BINS = 2 * HC_HALF, HC_COPIES = 8;
// Blocks of the histogram kernels are 1024 threads, two per CU: what a block's flush costs is global --
// every block adds each of its non-zero bins to the same ~450 counters, and same-address atomics from
// different workgroups are served one after the other (about 12 ns each): with 2048 blocks of 256
// threads that was 25 us of a 76 us kernel, whatever the LDS part did.  (The copies are per BLOCK, not per
// wave: only the lanes of one instruction can conflict, instructions of different waves pass through the
// LDS one after the other anyway.)
static constexpr int HB_THREADS = 1024, HB_GRID = 2 * kCUs;
static constexpr int HL_CENTRAL = 0, HL_FULL = (HC_BINS + 1) * HC_COPIES /* + one junk bin per copy */,
                     HL_SINK = HL_FULL + TZ_NBINS + 1, HL_WORDS = HL_SINK + 64;
struct HistLds {
    // [bin][copy] | full range | one sink word per lane
    unsigned w[HL_WORDS];
};

struct HistAcc {
    unsigned n0 = 0;   // wave-uniform count of the centre symbol
};

__device__ __forceinline__ void hist_clear(HistLds& h) {
    for (int k = threadIdx.x; k < HL_WORDS; k += blockDim.x) h.w[k] = 0;
    __syncthreads();
}

// 2 NDW symbols of one lane, packed two per dword.  The update is ONE unconditional LDS atomic per
// element in straight-line code (a branch per element cost more than the atomics it saved: the
// spatial-delta kernel is as much VALU-issue as HBM bound): the centre symbol goes to the lane's own
// sink word (it is counted by the ballot), symbols within +-64 of the centre to [bin][copy], anything
// farther to the junk bin of the copy -- and, in a branch the wave takes only when one of its 512
// symbols is that far out, to the full-range bins.
template <int NDW>
__device__ __forceinline__ void hist_add(HistLds& h, HistAcc& acc, const unsigned* Y, int c) {
    const int lane = threadIdx.x & 63;
    const int base = HL_CENTRAL + (lane & 7), sink = HL_SINK + lane;
    unsigned far = 0;
#pragma unroll
    for (int k = 0; k < 2 * NDW; ++k) {
        const int y = (k & 1) ? ((int)Y[k >> 1] >> 16) : (int)(short)(Y[k >> 1] & 0xFFFFu);
        const bool hot = y == c;
        acc.n0 += (unsigned)__popcll(__ballot(hot));
        const unsigned rel = (unsigned)(y - (c - HC_HALF));
        const unsigned idx = min(rel, (unsigned)HC_BINS);
        far |= idx >> 7;   // HC_BINS == 128
        atomicAdd(&h.w[hot ? sink : base + (int)idx * HC_COPIES], 1u);
    }
    if (__any(far != 0)) {
#pragma unroll
        for (int k = 0; k < 2 * NDW; ++k) {
            const int y = (k & 1) ? ((int)Y[k >> 1] >> 16) : (int)(short)(Y[k >> 1] & 0xFFFFu);
            if ((unsigned)(y - (c - HC_HALF)) >= (unsigned)HC_BINS && (unsigned)y < (unsigned)TZ_NBINS) atomicAdd(&h.w[HL_FULL + y], 1u);
        }
    }
}
__device__ __forceinline__ void hist_add8(HistLds& h, HistAcc& acc, const unsigned* Y, int c) { hist_add<4>(h, acc, Y, c); }
static_assert(HC_BINS == 128, "hist_add8 takes the far flag from bit 7 of the clamped index");

// every thread of the block calls this (after its last add)
__device__ __forceinline__ void hist_flush(HistLds& h, const HistAcc& a, int c, unsigned long long* __restrict__ hist) {
    if ((threadIdx.x & 63) == 0 && a.n0 && c >= 0 && c < TZ_NBINS) atomicAdd(&h.w[HL_FULL + c], a.n0);
    __syncthreads();
    for (int b = threadIdx.x; b < HC_BINS; b += blockDim.x) {
        const int y = c - HC_HALF + b;
        unsigned t = 0;
#pragma unroll
        for (int k = 0; k < HC_COPIES; ++k) t += h.w[HL_CENTRAL + b * HC_COPIES + k];
        if (t && y >= 0 && y < TZ_NBINS) atomicAdd(&h.w[HL_FULL + y], t);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < TZ_NBINS; k += blockDim.x) {
        const unsigned v = h.w[HL_FULL + k];
        if (v) atomicAdd(&hist[k], (unsigned long long)v);
    }
}

typedef short short2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_sub(unsigned a, unsigned b) {   // two int16 lanes, wrap-around
    const short2v r = __builtin_bit_cast(short2v, a) - __builtin_bit_cast(short2v, b);
    return __builtin_bit_cast(unsigned, r);
}

// spatial delta of 8 consecutive int16 (V, two per dword) given the element in front of them:
// sd[k] = x[k-1] - x[k]; symbols y = 1600 - sd when `offs` = (1600, 1600), y = sd when offs is 0 and `negate`
// is false ... both forms are y = offs - (P - V) resp. P - V; P is V shifted up by one element.
__device__ __forceinline__ void sdelta8(const uint4 V, unsigned prev16, bool apply_offset, unsigned* Y) {
    const unsigned P0 = __builtin_amdgcn_alignbit(V.x, prev16 << 16, 16);
    const unsigned P1 = __builtin_amdgcn_alignbit(V.y, V.x, 16);
    const unsigned P2 = __builtin_amdgcn_alignbit(V.z, V.y, 16);
    const unsigned P3 = __builtin_amdgcn_alignbit(V.w, V.z, 16);
    const unsigned C = ((unsigned)TZ_OFFSET << 16) | (unsigned)TZ_OFFSET;
    Y[0] = pk_sub(P0, V.x);
    Y[1] = pk_sub(P1, V.y);
    Y[2] = pk_sub(P2, V.z);
    Y[3] = pk_sub(P3, V.w);
    if (apply_offset) {
#pragma unroll
        for (int j = 0; j < 4; ++j) Y[j] = pk_sub(C, Y[j]);
    }
}

// --------------------------------------------------------------------------- quantiser
// compress.py:23-70, one chain per (frame, channel) over H*W elements, row-major.
// Stage 1 (k_q_minmax, k_q_bound): per-chain tolerance E for rel / absrel from max-min of the
//                      ORIGINAL slab (compress.py:31-33,36-43).  Under one abs bound per frame (tzk_quant_frames) k_q_frame_bound
//                      fills the same array from the frames' bounds instead.
// Stage 2 (k_q_width, k_q_tiles, k_q_chain, k_q_bstitch, k_q_serial): exact parallel form of the greedy
//                      interval-intersection segmentation (see the kernels).  Result: one bit per element (`spec`, a 64-bit
//                      mask per 64-element chunk and chain) that says where a run starts, and the
//                      truncated median of every run at its HEAD position of `tmp` (positions that are
//                      not heads hold garbage: the masks are authoritative, nothing initialises tmp).
// Stage 3 (k_q_last / k_q_carry / k_q_fill): forward-fill the run values.  k_q_fill either writes them
//                      back as the quantised delta stack (stand-alone tz_error_bound, delta tap) or --
//                      fused encode -- goes straight on to the spatial delta, the 1600 offset and the
//                      histogram (compress.py:339-355) and writes symbols: the quantised deltas never
//                      exist in memory.
// The deltas a chain is made of come from a materialised int16 stack or, fused encode, straight from
// prediction and original (compress.py:292-314 evaluated where it is needed): QSrc.
// Round 3 at cfg3, `abs 2` (profiles/r03/quantiser.md): the tiles read pred / orig (315 MB) and write the values
// (126 MB), the fill reads them and the masks and writes symbols (270 MB), the remap 252 MB: about 1.0 GB and
// 0.5 ms against 1.75 GB and 1.1 ms through k_delta, k_q_init, k_q_heads, k_q_last over tmp, k_q_fill, k_sdelta
// in round 2.
struct QParams {
    int mode;
    double b0, b1;
};

struct QSrc {
    const int16_t* diff;   // nframes * HW * 3, or nullptr: then
    const float* pred;     // ... trunc(pred * 255) - orig of unpadded frames (H == Hp, W == Wp)
};

template <bool FP>
__device__ __forceinline__ int q_delta(const QSrc& s, const uint8_t* __restrict__ orig, size_t e) {
    if (FP) return (int)(s.pred[e] * 255.0f) - (int)orig[e];
    return (int)s.diff[e];
}

// the 12 bytes at stack offset `off` (4 pixels x 3 channels), packed 4 per word.  Aligned dword loads -- three where the
// address is a multiple of 4, else four and a funnel shift -- wherever those dwords lie inside the stack [x, x + total); the
// groups at the stack's two ends that they would leave take byte loads (volatile: twelve plain ones the compiler folds into ONE
// 12-byte load at a byte address).  Nothing outside the stack is read, and what is wider than a byte lies on a dword boundary.
__device__ __forceinline__ void ss_row12(const uint8_t* __restrict__ x, size_t off, size_t total, unsigned w[3]) {
    const uintptr_t addr = (uintptr_t)x + off, m = addr & 3, p0 = addr - m;
    if (p0 >= (uintptr_t)x && p0 + (m ? 16 : 12) <= (uintptr_t)x + total) {
        const unsigned* p = (const unsigned*)(x + off - m);   // (= p0, as a pointer into x: a global load)
        const unsigned d0 = p[0], d1 = p[1], d2 = p[2], d3 = m ? p[3] : 0u;
        const unsigned sh = 8u * (unsigned)m;
        w[0] = (unsigned)((((unsigned long long)d1 << 32) | d0) >> sh);
        w[1] = (unsigned)((((unsigned long long)d2 << 32) | d1) >> sh);
        w[2] = (unsigned)((((unsigned long long)d3 << 32) | d2) >> sh);
    } else {
        const volatile uint8_t* b = x + off;
        w[0] = w[1] = w[2] = 0;
#pragma unroll
        for (int j = 0; j < 12; ++j) w[j >> 2] |= (unsigned)b[j] << (8 * (j & 3));
    }
}

// min/max of the original slab per (frame, channel): 12 bytes (4 interleaved RGB pixels) per
// lane and iteration, QBB blocks per frame combined with integer atomics (mm[f][c] = {min, max}).
static constexpr int QBB = 16;
__global__ __launch_bounds__(256) void k_q_minmax(const uint8_t* __restrict__ orig, const uint8_t* __restrict__ skip,
                                                  int HW, int* __restrict__ mm) {
    const int f = blockIdx.y;
    if (skip[f]) return;
    const uint8_t* o = orig + (size_t)f * HW * 3;
    int mn[3] = {255, 255, 255}, mx[3] = {0, 0, 0};
    const int ngroups = HW / 4;  // 4 pixels = 12 bytes: 3 aligned dwords where the frame starts on a 4-byte boundary, else 4 and a shift
    const size_t total = (size_t)gridDim.y * HW * 3;
    for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += QBB * 256) {
        unsigned w[3];
        ss_row12(orig, (size_t)f * HW * 3 + (size_t)g * 12, total, w);
#pragma unroll
        for (int b = 0; b < 12; ++b) {
            int v = (w[b >> 2] >> (8 * (b & 3))) & 0xff, c = b % 3;
            mn[c] = min(mn[c], v);
            mx[c] = max(mx[c], v);
        }
    }
    if (blockIdx.x == 0)
        for (int p = ngroups * 4 + threadIdx.x; p < HW; p += 256)
            for (int c = 0; c < 3; ++c) {
                int v = o[(size_t)p * 3 + c];
                mn[c] = min(mn[c], v);
                mx[c] = max(mx[c], v);
            }
    for (int c = 0; c < 3; ++c) {
        for (int s = 32; s >= 1; s >>= 1) {
            mn[c] = min(mn[c], __shfl_down(mn[c], s, 64));
            mx[c] = max(mx[c], __shfl_down(mx[c], s, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&mm[(f * 3 + c) * 2], mn[c]);
            atomicMax(&mm[(f * 3 + c) * 2 + 1], mx[c]);
        }
    }
}

__global__ void k_q_mm_init(int* __restrict__ mm, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mm[i] = (i & 1) ? 0 : 255;
}

// tolerance per chain from max-min of the ORIGINAL slab (compress.py:31-33, 36-43)
__global__ void k_q_bound(const int* __restrict__ mm, const uint8_t* __restrict__ skip, QParams qp, int nframes,
                          double* __restrict__ E) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nframes * 3 || skip[i / 3]) return;
    double range = (double)(mm[2 * i + 1] - mm[2 * i]);
    double e;
    if (qp.mode == TZ_MODE_REL) {
        e = range * qp.b0;
    } else {  // absrel
        double a = fabs(qp.b0), r = range * qp.b1;
        e = a < r ? a : r;
    }
    E[i] = e;
}

// tolerance per chain from one abs bound per frame (tz_set_frame_bounds, tz_error_bound_frames): the frame's three chains
// share it.  The walks then read it as they read k_q_bound's.
__global__ void k_q_frame_bound(const double* __restrict__ fb, const uint8_t* __restrict__ skip, int nframes, double* __restrict__ E) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nframes * 3 || skip[i / 3]) return;
    E[i] = fb[i / 3];
}

// Two forms of the exact greedy segmentation live here.
//
// (1) WAVE-parallel, one 64-element chunk at a time (lane i <-> element; q_chunk).  A run started at s breaks
// at the first i with min(Du[s..i]) < max(Dl[s..i]) (compress.py:60 -- a-b<0 <=> a<b in IEEE), monotone in i, so
// a wave computes per chunk
//   1. range tables T_k[i] = (min Du, max Dl) over [i, i+2^k) by shuffles (k = 0..5),
//   2. nxt[s] = first break after s for EVERY s (fresh start) by binary lifting over T_k, together with the
//      run's (u, l) up to the break,
//   3. the inclusive prefix (min Du, max Dl) from the chunk start,
//   2b. heads[s] = bit mask of the run heads reached from a start at s (pointer doubling),
// and a run carried in from earlier chunks is then resolved without knowing in advance where it breaks:
//   4. it breaks at the first i with min(u, P_u[i]) < max(l, P_l[i]) (ballot); the true heads of the chunk are
//      heads[that i],
//   5. every head whose run closes inside the chunk gets trunc((u+l)/2) (compress.py:61, truncation by the
//      int64 store) at its position of `tmp`; the last head carries on.
// That is about 250 vector instructions and 35 cross-lane shuffles per chunk.  Rounds 1-2 ran the whole chain
// through it (k_q_heads: worker waves + a resolver wave per segment of a chain, 1.29 -> 0.63 ms per cfg3 step;
// profiles/r02/quantiser.md).  Now it serves where a run of UNKNOWN origin has to be taken into a chunk: at the
// tile boundaries (k_q_bstitch) and in the serial fallback (k_q_serial).
//
// (2) LANE-parallel walks from speculative fresh starts (k_q_tiles, below): a dozen integer instructions per
// element instead, because a walk that starts fresh never has to ask where somebody else's run breaks.  What
// makes the guesses exact: two greedy chains over the same data never cross, and they coincide from their first
// common head on; so the chain that really enters a region is followed only until it hits a head of the region's
// speculative chain -- speculative heads in front of that point leave the masks, true ones enter, behind it
// everything is already right.  Nothing depends on run lengths; elements past the chain end are (+inf, -inf)
// and can neither break nor tighten a run.
__device__ __forceinline__ double shfl_d(double v, int src) { return __shfl(v, src, 64); }

struct QChunk {
    double cu, cl, pu, pl;
    unsigned long long heads;
    int nxt;
};

struct QState {  // the run that is open at a segment boundary
    double u, l;
    int head, pad;
};

// steps 1-3 for chunk `ch` of channel c (every lane returns its element's entries).
//
// The cross-lane traffic of these steps is what the quantiser costs: a 64-bit shuffle is two
// ds_bpermute_b32, and with (min Du, max Dl) as two doubles a chunk took 86 of them -- 1.1 ms of LDS
// crossbar per 4096-chunk chain and CU, which is the 1.29 ms k_q_heads ran at in round 1 (cutting the
// resolver's walk into segments alone changed nothing: profiles/r02/quantiser.md).  For abs / rel /
// absrel the tolerance E is one constant per chain, so Du = fl(d + E) and Dl = fl(d - E) are monotone
// in the integer delta d: min Du = fl(min d + E), max Dl = fl(max d - E) EXACTLY.  The tables, the
// prefix and the lifting therefore run on (min d, max d) packed as two int16 in ONE 32-bit word (35
// shuffles per chunk), and the doubles the reference compares (compress.py:55-60) are formed from
// them only where a break is tested or a run value is produced.  pwrel (E = orig * b per element)
// keeps the double tables.
__device__ __forceinline__ int q_pack(int mn, int mx) { return (mn & 0xFFFF) | (mx << 16); }
__device__ __forceinline__ int q_lo(int p) { return (int)(short)(p & 0xFFFF); }
__device__ __forceinline__ int q_hi(int p) { return p >> 16; }

// Where a walk takes its tolerance from (the PW template value of q_chunk and k_q_tiles, of lat_apply and its kernels):
//   Q_TOL_CHAIN  one E per chain (abs, rel, absrel, frame bounds): the integer walk
//   Q_TOL_ORIG   E = orig * b0 per element (pwrel): the double walk
//   Q_TOL_MAP    E = M[pixel] per element, M an H x W uint8 map shared by every frame and channel (TZ-BM1, tz_set_bound_map):
//                the double walk; the map itself is the only tolerance storage, `orig` is read for the deltas alone (FP)
// The kernels' argument lists are what they were without the map (one argument more moves the hidden ones, and with them an
// offset in every existing instantiation's instruction stream): under Q_TOL_MAP the map travels in the slot of an argument that
// source never reads -- `Echain` in the walks (q_tol_map), `orig` in k_lattice, the eight bytes of `b0` in k_lattice_sd (lat_tol_map).
static constexpr int Q_TOL_CHAIN = 0, Q_TOL_ORIG = 1, Q_TOL_MAP = 2;
__device__ __forceinline__ const uint8_t* q_tol_map(const double* Echain) { return (const uint8_t*)Echain; }

// fe0 = element index of the frame's first sample in the whole stack (f * HW * 3)
template <int PW, bool FP>
__device__ __forceinline__ QChunk q_chunk(const QSrc& src, const uint8_t* __restrict__ orig, size_t fe0, int c, int ch, int HW,
                                          const QParams& qp, double E, int lane, const uint8_t* __restrict__ tolmap = nullptr) {
    const int idx = ch * 64 + lane;
    unsigned long long M = 1ull << lane;
    int pos = lane + 1;
    QChunk out;
    if (!PW) {
        // past the chain end: (min, max) = (+32767, -32768) can neither break nor tighten a run
        int mn = 32767, mx = -32768;
        if (idx < HW) mn = mx = q_delta<FP>(src, orig, fe0 + (size_t)idx * 3 + c);
        int tb[6];
        tb[0] = q_pack(mn, mx);
#pragma unroll
        for (int k = 1; k < 6; ++k) {  // shfl_down past lane 63 returns the caller's own value
            const int q = __shfl_down(tb[k - 1], 1 << (k - 1), 64);
            tb[k] = q_pack(min(q_lo(tb[k - 1]), q_lo(q)), max(q_hi(tb[k - 1]), q_hi(q)));
        }
        int pp = tb[0];
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            const int q = __shfl_up(pp, sft, 64);
            if (lane >= sft) pp = q_pack(min(q_lo(pp), q_lo(q)), max(q_hi(pp), q_hi(q)));
        }
        int cmn = mn, cmx = mx;
#pragma unroll
        for (int k = 5; k >= 0; --k) {
            const int step = 1 << k;
            const int srcl = pos < 63 ? pos : 63;
            const int q = __shfl(tb[k], srcl, 64);
            const int nmn = min(cmn, q_lo(q)), nmx = max(cmx, q_hi(q));
            const double nu = (double)nmn + E, nl = (double)nmx - E;
            const bool ok = (pos + step <= 64) && !(nu - nl < 0.0);
            if (ok) {
                cmn = nmn;
                cmx = nmx;
                pos += step;
            }
        }
        out.cu = (double)cmn + E;
        out.cl = (double)cmx - E;
        out.pu = (double)q_lo(pp) + E;
        out.pl = (double)q_hi(pp) - E;
    } else {
        const double inf = __builtin_huge_val();
        double du = inf, dl = -inf;
        if (idx < HW) {
            const size_t e = fe0 + (size_t)idx * 3 + c;
            const double tol = PW == Q_TOL_MAP ? (double)tolmap[idx] : (double)orig[e] * qp.b0;
            const double df = (double)q_delta<FP>(src, orig, e);
            du = df + tol;
            dl = df - tol;
        }
        double tu[6], tl[6];
        tu[0] = du;
        tl[0] = dl;
#pragma unroll
        for (int k = 1; k < 6; ++k) {
            double a = __shfl_down(tu[k - 1], 1 << (k - 1), 64), b = __shfl_down(tl[k - 1], 1 << (k - 1), 64);
            tu[k] = tu[k - 1] < a ? tu[k - 1] : a;
            tl[k] = tl[k - 1] > b ? tl[k - 1] : b;
        }
        double pu = du, pl = dl;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            double a = __shfl_up(pu, sft, 64), b = __shfl_up(pl, sft, 64);
            if (lane >= sft) {
                pu = pu < a ? pu : a;
                pl = pl > b ? pl : b;
            }
        }
        double cu = du, cl = dl;
#pragma unroll
        for (int k = 5; k >= 0; --k) {
            const int step = 1 << k;
            int srcl = pos < 63 ? pos : 63;
            double xu = shfl_d(tu[k], srcl), xl = shfl_d(tl[k], srcl);
            double nu = cu < xu ? cu : xu, nl = cl > xl ? cl : xl;
            bool ok = (pos + step <= 64) && !(nu - nl < 0.0);
            if (ok) {
                cu = nu;
                cl = nl;
                pos += step;
            }
        }
        out.cu = cu;
        out.cl = cl;
        out.pu = pu;
        out.pl = pl;
    }
    // 2b. pointer doubling: the set of run heads reached from a start at this lane.  (Following the chain
    // of ONE start with scalar instructions in the resolver instead -- v_readlane of nxt, one hop per run --
    // was tried in round 3: 17 instead of 35 shuffles per chunk, but the hops sit on the serial path and
    // noise-like data has up to 64 runs per chunk: `rel 1e-3` went from 0.9 to 1.8 ms per step, `abs 2`
    // gained nothing.)
    int J = pos;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int srcl = J < 64 ? J : lane;
        unsigned long long Mj = __shfl(M, srcl, 64);
        int Jj = __shfl(J, srcl, 64);
        if (J < 64) {
            M |= Mj;
            J = Jj;
        }
    }
    out.heads = M;
    out.nxt = pos;  // in [lane+1, 64]; 64 = the run leaves the chunk
    return out;
}

__device__ __forceinline__ double q_rl_d(double v, int src) {  // src is wave-uniform
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ unsigned long long q_rl_u64(unsigned long long v, int src) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src) << 32) |
           (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
}

// ---------------------------------------------------------------------------------------------------------
// The segmentation as LANE-parallel greedy walks (round 3; form (2) above).
//   k_q_tiles   a wave owns 4096 consecutive elements of a chain, staged transposed in LDS; lane j walks chunk j
//               (64 elements = one mask word) from a fresh start and notes the heads in its mask.  Then the
//               lanes are stitched: lane j takes the run lane j-1 leaves open, lets it pass if its whole chunk fits
//               (one test on the chunk's min / max), else walks until the true chain meets a head of its own
//               speculative chain; heads in front of that point are replaced, behind it the guess stands and the
//               lane's exit state is the speculative one.  Repeated until no lane's incoming run changes (a lane
//               whose chunk the true chain leaves unmerged, or passes through, changes its successor's input:
//               typically 2-3 rounds, 64 at worst).  With the heads final, one more walk forms the run values and
//               puts them at their heads in the LDS tile, which leaves the way it came: 24 bytes per thread, all
//               three channels.  Output per tile: masks, values, the run left open, min / max.
//   k_q_chain   one wave per chain: the tiles' open runs chained -- a run that swallows a whole tile (one test on the
//               tile's min / max) passes, otherwise the tile's own exit state stands (assuming the true chain meets
//               the tile's speculative one inside it) -- giving every tile the run that really enters it.
//   k_q_bstitch one wave per tile boundary, all in parallel: the entering run is walked into the tile with the
//               wave-parallel machinery (q_chunk) until it meets the tile's chain -- usually in the first chunk.
//               A tile it crosses without meeting the speculative chain marks its chain for
//   k_q_serial  the exact serial walk of a whole chain (the algorithm of round 1), which runs only for such chains.
// For abs / rel / absrel the walks are integer: a run is (min d, max d), and "does it break" is
// fl(min d + E) < fl(max d - E) (compress.py:55-60), monotone in both arguments; k_q_width finds per chain the
// widths w = max d - min d that are always fine (w <= wmin) and always a break (w > wmax) by evaluating the
// double test itself on all 511 x 3 candidate pairs -- the two differ only when 2E sits within a rounding error
// of an integer, and then the walk evaluates the double test for the widths in between.  Run values are
// trunc((fl(min d + E) + fl(max d - E)) / 2) in double, as the reference computes them.
struct QWidth {
    int wmin, wmax;
};

__device__ __forceinline__ bool q_ok_exact(int mn, int mx, double E) { return !(((double)mn + E) < ((double)mx - E)); }

__global__ __launch_bounds__(64) void k_q_width(const double* __restrict__ Echain, const uint8_t* __restrict__ skip, QParams qp,
                                              QWidth* __restrict__ width) {
    const int chain = blockIdx.x, lane = threadIdx.x;
    if (skip[chain / 3]) return;
    const double E = qp.mode == TZ_MODE_ABS ? fabs(qp.b0) : Echain[chain];
    int wmin = 511, wmax = -1;
    for (int mn = -255 + lane; mn <= 255; mn += 64) {
        // W(mn) = largest w with ok(mn, mn + w) (monotone in w); 511 when every feasible w is fine
        int W;
        if (!q_ok_exact(mn, mn, E)) W = -1;
        else if (q_ok_exact(mn, 255, E)) W = 511;
        else {
            int lo = 0, hi = 255 - mn;   // ok(lo), !ok(hi)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (q_ok_exact(mn, mn + mid, E)) lo = mid;
                else hi = mid;
            }
            W = lo;
        }
        wmin = min(wmin, W);
        wmax = max(wmax, W);
    }
    for (int s = 32; s >= 1; s >>= 1) {
        wmin = min(wmin, __shfl_down(wmin, s, 64));
        wmax = max(wmax, __shfl_down(wmax, s, 64));
    }
    if (lane == 0) width[chain] = QWidth{wmin, wmax};
}

static constexpr int QT_CHUNKS = 64;                 // chunks (= lanes) per tile
static constexpr int QT_TILE = QT_CHUNKS * 64;       // elements per tile
static constexpr int QT_S16 = 66, QT_S32 = 65;       // LDS row strides (int16 / int32 elements): lanes j, j+32 share a bank, no more

// run state of the integer walk: mn > mx = empty
struct QRunI {
    int mn, mx, hd;   // hd: chain index of the run's head
};
struct QRunD {
    double u, l;
    int hd;
};

template <int PW, bool FP>
__global__ __launch_bounds__(192) void k_q_tiles(QSrc src, const uint8_t* __restrict__ orig, const uint8_t* __restrict__ skip,
                                                 int HW, int ntiles, QParams qp, const double* __restrict__ Echain,
                                                 const QWidth* __restrict__ width, int16_t* __restrict__ tmp,
                                                 unsigned long long* __restrict__ spec, QState* __restrict__ tile_out,
                                                 double2* __restrict__ tile_agg) {
    __shared__ int lds_raw[3 * (PW ? 64 * QT_S32 : 64 * QT_S16 / 2)];
    const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;   // one wave per channel of the same pixels (they share cache lines)
    const int f = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    if (skip[f]) return;
    const uint8_t* const tolmap = PW == Q_TOL_MAP ? q_tol_map(Echain) : nullptr;
    const int chain = f * 3 + c;
    const size_t fe0 = (size_t)f * HW * 3;
    int16_t* t = tmp + fe0;
    const int nch = (HW + 63) >> 6;
    const int e0 = tile * QT_TILE;                              // first element of the tile in the chain
    short* ls = (short*)lds_raw + c * 64 * QT_S16;              // !PW: int16 deltas
    unsigned* lw = (unsigned*)lds_raw + c * 64 * QT_S32;        //  PW: delta | orig << 16 (Q_TOL_MAP: delta | M[pixel] << 16)
    // ---- stage the tile transposed: row r = the 64 elements of chunk r (lane r walks it).
    // Frames of whole 4-pixel groups: the block's three waves load the tile TOGETHER -- a thread takes 4 pixels =
    // 12 consecutive samples (three 16-byte loads of the prediction + 12 original bytes, or 24 bytes of the delta
    // stack), forms the deltas and deals them to the three channel planes.  (A wave per channel fetching its own
    // samples with a stride of three touched every cache line three times, 2-byte / 4-byte accesses: 141 of the
    // first version's 280 us.)
    const bool grouped = (HW & 3) == 0 && (((uintptr_t)src.pred & 15) | ((uintptr_t)src.diff & 7) | ((uintptr_t)orig & 3) | ((uintptr_t)tmp & 7)) == 0 &&
                         (PW != Q_TOL_MAP || ((uintptr_t)tolmap & 3) == 0);   // (the map: a thread's four pixels as one 4-byte load)
    // The integer walk below rests on k_q_width's table, which covers deltas in [-255, 255] -- everything compress.py:292-314
    // can produce.  The stand-alone tz_error_bound takes ANY int16 stack: a tile that holds a value outside that range
    // (`wide`) evaluates the double test of compress.py:60 itself at every step instead.
    int wide = 0;
    if (grouped) {
        const int npix = min(QT_TILE, HW - e0);
        for (int g = threadIdx.x; g < QT_TILE / 4; g += 192) {
            const int p0 = g * 4;
            int d[12], o[12];
            unsigned mw = 0;   // Q_TOL_MAP: the tolerances of the thread's four pixels
#pragma unroll
            for (int k = 0; k < 12; ++k) d[k] = o[k] = 0;
            if (p0 < npix) {
                const size_t e = fe0 + (size_t)(e0 + p0) * 3;
                if (PW == Q_TOL_MAP) mw = *(const unsigned*)(tolmap + e0 + p0);
                if (FP || PW == Q_TOL_ORIG) {
                    const uint3 ob = *(const uint3*)(orig + e);
                    const unsigned ow[3] = {ob.x, ob.y, ob.z};
#pragma unroll
                    for (int k = 0; k < 12; ++k) o[k] = (int)((ow[k >> 2] >> (8 * (k & 3))) & 0xFFu);
                }
                if (FP) {
                    const float4* pp = (const float4*)(src.pred + e);
                    const float4 f0 = pp[0], f1 = pp[1], f2 = pp[2];
                    const float fv[12] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w, f2.x, f2.y, f2.z, f2.w};
#pragma unroll
                    for (int k = 0; k < 12; ++k) d[k] = (int)(fv[k] * 255.0f) - o[k];
                } else {
                    const uint2* dp = (const uint2*)(src.diff + e);
                    const uint2 a0 = dp[0], a1 = dp[1], a2 = dp[2];
                    const unsigned dw[6] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y};
#pragma unroll
                    for (int k = 0; k < 12; ++k) {
                        d[k] = (int)(short)((dw[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
                        wide |= (unsigned)(d[k] + 255) > 510u;
                    }
                }
            }
            const int row = p0 >> 6, col = p0 & 63;
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {   // sample k of the group = pixel k / 3, channel k % 3
                if (PW) {
                    unsigned* w = (unsigned*)lds_raw + cc * 64 * QT_S32 + row * QT_S32 + col;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        w[i] = ((unsigned)d[3 * i + cc] & 0xFFFFu) | ((PW == Q_TOL_MAP ? (mw >> (8 * i)) & 0xFFu : (unsigned)o[3 * i + cc]) << 16);
                } else {
                    unsigned* w = (unsigned*)((short*)lds_raw + cc * 64 * QT_S16 + row * QT_S16 + col);   // 4-byte aligned: 132 r + 2 col
                    w[0] = ((unsigned)d[cc] & 0xFFFFu) | ((unsigned)d[3 + cc] << 16);
                    w[1] = ((unsigned)d[6 + cc] & 0xFFFFu) | ((unsigned)d[9 + cc] << 16);
                }
            }
        }
        if (FP || PW) __syncthreads();
        else wide = __syncthreads_or(wide);
    } else {
#pragma unroll 8
        for (int r = 0; r < 64; ++r) {
            const int idx = e0 + r * 64 + lane;
            int d = 0, o = 0;
            if (idx < HW) {
                const size_t e = fe0 + (size_t)idx * 3 + c;
                d = q_delta<FP>(src, orig, e);
                if (PW == Q_TOL_ORIG) o = orig[e];
                if (PW == Q_TOL_MAP) o = tolmap[idx];
                if (!FP && !PW) wide |= (unsigned)(d + 255) > 510u;
            }
            if (PW) lw[r * QT_S32 + lane] = ((unsigned)d & 0xFFFFu) | ((unsigned)o << 16);
            else ls[r * QT_S16 + lane] = (short)d;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const int base = e0 + lane * 64;                            // chain index of my chunk's first element
    const int len = max(0, min(64, HW - base));
    double E = 0.0;
    int wmin = 0, wmax = 0;
    if (!PW) {
        E = qp.mode == TZ_MODE_ABS ? fabs(qp.b0) : Echain[chain];
        const QWidth wd = width[chain];
        wmin = wd.wmin;
        wmax = wd.wmax;
        if (!FP && __any(wide)) {   // no width is taken from the table: "ambiguous" always, q_ok_exact decides
            wmin = -1;
            wmax = 0x7FFFFFFF;
        }
    }
    const double inf = __builtin_huge_val();
    // element access and the run algebra of the two arithmetic forms
    auto elem_i = [&](int tt) { return (int)ls[lane * QT_S16 + tt]; };
    // (wave-uniform, and opaque to the compiler: it would otherwise evaluate the double test speculatively in every step)
    const bool banded = __builtin_amdgcn_readfirstlane(wmin != wmax) != 0;
    auto ok_i = [&](int mn, int mx) {   // may the run (mn, mx) stand?  exact form of compress.py:60
        const int w = mx - mn;
        bool ok = w <= wmin;
        if (banded) {
            const bool amb = !ok && w <= wmax;
            if (__any(amb)) ok = ok || (amb && q_ok_exact(mn, mx, E));
        }
        return ok;
    };
    // |value| <= 255 + E: the int conversion is the int64 store of compress.py:61 (one instruction instead of five)
    auto val_i = [&](int mn, int mx) { return (int)((((double)mn + E) + ((double)mx - E)) / 2); };
    auto elem_d = [&](int tt, double& du, double& dl) {
        const unsigned w = lw[lane * QT_S32 + tt];
        const double df = (double)(int)(short)(w & 0xFFFFu);
        const double tol = PW == Q_TOL_MAP ? (double)(int)(w >> 16) : (double)(int)(w >> 16) * qp.b0;
        du = df + tol;
        dl = df - tol;
    };

    // ---- 1. speculative walk of my chunk from a fresh start: heads only (the values follow once the heads are final)
    unsigned long long Ms = len > 0 ? 1ull : 0ull;
    QRunI xi{32767, -32768, base};      // !PW
    QRunD xd{inf, -inf, base};          //  PW
    int amn = 32767, amx = -32768;      // chunk aggregate (!PW)
    double au = inf, al = -inf;         //                 ( PW)
    for (int tt = 0; tt < 64; ++tt) {
        const bool act = tt < len;
        if (!PW) {
            const int d = elem_i(tt);
            const int nmn = min(xi.mn, d), nmx = max(xi.mx, d);
            const bool brk = act && xi.mn <= xi.mx && !ok_i(nmn, nmx);
            if (brk) {
                Ms |= 1ull << tt;
                xi = QRunI{d, d, base + tt};
            } else if (act) {
                xi.mn = nmn;
                xi.mx = nmx;
            }
            if (act) {
                amn = min(amn, d);
                amx = max(amx, d);
            }
        } else {
            double du, dl;
            elem_d(tt, du, dl);
            const double nu = xd.u < du ? xd.u : du, nl = xd.l > dl ? xd.l : dl;
            const bool brk = act && (nu < nl);   // a fresh run (inf, -inf) cannot break: du >= dl for a tolerance >= 0
            if (brk) {
                Ms |= 1ull << tt;
                xd = QRunD{du, dl, base + tt};
            } else if (act) {
                xd.u = nu;
                xd.l = nl;
            }
            if (act) {
                au = au < du ? au : du;
                al = al > dl ? al : dl;
            }
        }
    }
    const QRunI xsi = xi;
    const QRunD xsd = xd;
    // ---- 2. stitch the lanes: my incoming run is what lane - 1 leaves open; repeat until nothing changes
    unsigned long long M = Ms;
    QRunI pini{0, 0, -2};               // the incoming run my current (M, exit) was computed for; hd -2 = none yet
    QRunD pind{0.0, 0.0, -2};
    for (int iter = 0; iter < 66; ++iter) {
        bool dirty;
        QRunI ini{};
        QRunD ind{};
        if (!PW) {
            ini.mn = __shfl_up(xi.mn, 1, 64);
            ini.mx = __shfl_up(xi.mx, 1, 64);
            ini.hd = __shfl_up(xi.hd, 1, 64);
            dirty = lane > 0 && len > 0 && (ini.mn != pini.mn || ini.mx != pini.mx || ini.hd != pini.hd);
        } else {
            ind.u = __shfl_up(xd.u, 1, 64);
            ind.l = __shfl_up(xd.l, 1, 64);
            ind.hd = __shfl_up(xd.hd, 1, 64);
            dirty = lane > 0 && len > 0 && (ind.u != pind.u || ind.l != pind.l || ind.hd != pind.hd);
        }
        if (!__any(dirty)) break;
        bool walking = false;
        unsigned long long newm = 0;
        if (dirty) {
            pini = ini;
            pind = ind;
            if (!PW) {
                const int qmn = min(ini.mn, amn), qmx = max(ini.mx, amx);
                if (ok_i(qmn, qmx)) {       // the run passes through my whole chunk
                    M = 0;
                    xi = QRunI{qmn, qmx, ini.hd};
                } else {
                    walking = true;
                    xi = ini;
                }
            } else {
                const double qu = ind.u < au ? ind.u : au, ql = ind.l > al ? ind.l : al;
                if (!(qu < ql)) {
                    M = 0;
                    xd = QRunD{qu, ql, ind.hd};
                } else {
                    walking = true;
                    xd = ind;
                }
            }
        }
        for (int tt = 0; tt < 64 && __any(walking); ++tt) {
            const bool act = walking && tt < len;
            bool brk;
            if (!PW) {
                const int d = elem_i(tt);
                const int nmn = min(xi.mn, d), nmx = max(xi.mx, d);
                brk = act && !ok_i(nmn, nmx);
                if (brk) xi = QRunI{d, d, base + tt};
                else if (act) {
                    xi.mn = nmn;
                    xi.mx = nmx;
                }
            } else {
                double du, dl;
                elem_d(tt, du, dl);
                const double nu = xd.u < du ? xd.u : du, nl = xd.l > dl ? xd.l : dl;
                brk = act && (nu < nl);
                if (brk) xd = QRunD{du, dl, base + tt};
                else if (act) {
                    xd.u = nu;
                    xd.l = nl;
                }
            }
            if (brk) {
                if ((Ms >> tt) & 1ull) {   // the true chain starts a run where my speculative chain does: from here on they are one
                    M = newm | (Ms & ~((1ull << tt) - 1ull));
                    xi = xsi;
                    xd = xsd;
                    walking = false;
                } else {
                    newm |= 1ull << tt;
                }
            }
            if (walking && tt == len - 1) {   // left my chunk without meeting the speculative chain
                M = newm;
                walking = false;
            }
        }
    }
    // ---- 3. the run values, now that the heads are final: one more walk of my chunk, which starts with the run that
    // really enters it (pini / pind: what the last stitch round was computed for; lane 0 starts fresh).  A run's value
    // replaces the delta at its head IN the LDS tile -- the element has been consumed by then; the one run that may
    // close in my chunk but started in an earlier lane's row is written after the walk (its row's owner may not have
    // read that element yet).  The run open at the end of the tile is closed by k_q_chain / k_q_bstitch.
    {
        QRunI ri{32767, -32768, base};
        QRunD rd{inf, -inf, base};
        if (lane > 0 && len > 0) {
            ri = pini;
            rd = pind;
        }
        int late_hd = -1, late_v = 0;
        for (int tt = 0; tt < 64; ++tt) {
            const bool act = tt < len;
            const bool head = act && ((M >> tt) & 1ull);
            int d = 0;
            double du = 0.0, dl = 0.0;
            if (!PW) d = elem_i(tt);
            else elem_d(tt, du, dl);
            if (__any(head)) {
                // (the run in front of a head is empty only for lane 0's first element)
                if (head && (!PW ? ri.mn <= ri.mx : (rd.u != inf || rd.l != -inf))) {
                    const int v = !PW ? val_i(ri.mn, ri.mx) : (int)((rd.u + rd.l) / 2);
                    const int hd = !PW ? ri.hd : rd.hd;
                    if (hd >= base) {
                        if (!PW) ls[lane * QT_S16 + (hd - base)] = (short)v;
                        else lw[lane * QT_S32 + (hd - base)] = (unsigned)v & 0xFFFFu;
                    } else {
                        late_hd = hd;
                        late_v = v;
                    }
                }
            }
            if (head) {
                ri = QRunI{d, d, base + tt};
                rd = QRunD{du, dl, base + tt};
            } else if (act) {
                ri.mn = min(ri.mn, d);
                ri.mx = max(ri.mx, d);
                rd.u = rd.u < du ? rd.u : du;
                rd.l = rd.l > dl ? rd.l : dl;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (late_hd >= 0) {
            const int rel = late_hd - e0;
            if (!PW) ls[(rel >> 6) * QT_S16 + (rel & 63)] = (short)late_v;
            else lw[(rel >> 6) * QT_S32 + (rel & 63)] = (unsigned)late_v & 0xFFFFu;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (grouped) {
            // flush, the way the tile came in: all three planes, 12 consecutive samples = 24 bytes per thread.  Dense -- what is
            // not a head carries its delta along, which nobody reads (the masks say where the heads are)
            __syncthreads();
            const int npix = min(QT_TILE, HW - e0);
            for (int g = threadIdx.x; g < QT_TILE / 4; g += 192) {
                const int p0 = g * 4;
                if (p0 >= npix) continue;
                const int row = p0 >> 6, col = p0 & 63;
                unsigned v[12];
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) {
                    if (PW) {
                        const unsigned* w = (const unsigned*)lds_raw + cc * 64 * QT_S32 + row * QT_S32 + col;
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[3 * i + cc] = w[i] & 0xFFFFu;
                    } else {
                        const unsigned* w = (const unsigned*)((const short*)lds_raw + cc * 64 * QT_S16 + row * QT_S16 + col);
                        const unsigned w0 = w[0], w1 = w[1];
                        v[cc] = w0 & 0xFFFFu;
                        v[3 + cc] = w0 >> 16;
                        v[6 + cc] = w1 & 0xFFFFu;
                        v[9 + cc] = w1 >> 16;
                    }
                }
                uint2* dst = (uint2*)(t + (size_t)(e0 + p0) * 3);
                dst[0] = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
                dst[1] = make_uint2(v[4] | (v[5] << 16), v[6] | (v[7] << 16));
                dst[2] = make_uint2(v[8] | (v[9] << 16), v[10] | (v[11] << 16));
            }
        } else {
            // flush: row r = chunk r, a lane per element; only heads carry a value
            const unsigned mlo = (unsigned)M, mhi = (unsigned)(M >> 32);
#pragma unroll 8
            for (int r = 0; r < 64; ++r) {
                const unsigned long long mr = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)mhi, r) << 32) |
                                              (unsigned)__builtin_amdgcn_readlane((int)mlo, r);
                if ((mr >> lane) & 1ull) {
                    const int v = !PW ? (int)ls[r * QT_S16 + lane] : (int)(short)(lw[r * QT_S32 + lane] & 0xFFFFu);
                    t[(size_t)(e0 + r * 64 + lane) * 3 + c] = (int16_t)v;
                }
            }
        }
    }
    // ---- 4. results
    const int chunk = tile * QT_CHUNKS + lane;
    if (chunk < nch) spec[(size_t)chain * nch + chunk] = M;
    const int lastl = min(63, (min(HW, e0 + QT_TILE) - e0 - 1) >> 6);   // the last lane that holds elements
    if (!PW) {
        int tmn = len > 0 ? amn : 32767, tmx = len > 0 ? amx : -32768;
        for (int sft = 32; sft >= 1; sft >>= 1) {
            tmn = min(tmn, __shfl_xor(tmn, sft, 64));
            tmx = max(tmx, __shfl_xor(tmx, sft, 64));
        }
        if (lane == lastl) {
            tile_out[(size_t)chain * ntiles + tile] = QState{(double)xi.mn + E, (double)xi.mx - E, xi.hd, 0};
            tile_agg[(size_t)chain * ntiles + tile] = make_double2((double)tmn + E, (double)tmx - E);
        }
    } else {
        double tu = au, tl = al;
        for (int sft = 32; sft >= 1; sft >>= 1) {
            const double a = __shfl_xor(tu, sft, 64), b = __shfl_xor(tl, sft, 64);
            tu = tu < a ? tu : a;
            tl = tl > b ? tl : b;
        }
        if (lane == lastl) {
            tile_out[(size_t)chain * ntiles + tile] = QState{xd.u, xd.l, xd.hd, 0};
            tile_agg[(size_t)chain * ntiles + tile] = make_double2(tu, tl);
        }
    }
}

// The run that really enters every tile (see k_q_tiles); closes the run that is open at the end of the chain.
__global__ __launch_bounds__(64) void k_q_chain(const uint8_t* __restrict__ skip, int HW, int ntiles, const QState* __restrict__ tile_out,
                                              const double2* __restrict__ tile_agg, QState* __restrict__ tile_in,
                                              uint8_t* __restrict__ swallowed, int16_t* __restrict__ tmp) {
    const int chain = blockIdx.x, f = chain / 3, c = chain % 3, lane = threadIdx.x;
    if (skip[f]) return;
    double su = 0.0, sl = 0.0;
    int sh = 0;
    for (int t0 = 0; t0 < ntiles; t0 += 64) {
        const int T = t0 + lane;
        QState o{0.0, 0.0, 0, 0};
        double2 g = make_double2(0.0, 0.0);
        if (T < ntiles) {
            o = tile_out[(size_t)chain * ntiles + T];
            g = tile_agg[(size_t)chain * ntiles + T];
        }
        double iu = 0.0, il = 0.0;
        int ih = 0, sw = 0;
        const int cnt = min(64, ntiles - t0);
        for (int k = 0; k < cnt; ++k) {
            const double ou = q_rl_d(o.u, k), ol = q_rl_d(o.l, k);
            const int oh = __builtin_amdgcn_readlane(o.head, k);
            if (t0 + k == 0) {          // the first tile starts where the chain starts: its guess is the truth
                su = ou;
                sl = ol;
                sh = oh;
                continue;
            }
            const double gu = q_rl_d(g.x, k), gl = q_rl_d(g.y, k);
            const double qu = su < gu ? su : gu, ql = sl > gl ? sl : gl;
            const bool pass = !(qu < ql);
            if (lane == k) {
                iu = su;
                il = sl;
                ih = sh;
                sw = pass;
            }
            if (pass) {
                su = qu;
                sl = ql;
            } else {
                su = ou;
                sl = ol;
                sh = oh;
            }
        }
        if (T < ntiles && T > 0) {
            tile_in[(size_t)chain * ntiles + T] = QState{iu, il, ih, 0};
            swallowed[(size_t)chain * ntiles + T] = (uint8_t)sw;
        }
    }
    if (lane == 0 && HW > 0) tmp[((size_t)f * HW + sh) * 3 + c] = (int16_t)(long long)((su + sl) / 2);
}

// The run entering tile T walked into the tile until it meets the tile's own chain (see k_q_tiles); a tile that is
// crossed without that marks the chain for k_q_serial.
template <bool FP, bool MAP>
__global__ __launch_bounds__(64) void k_q_bstitch(QSrc src, const uint8_t* __restrict__ orig, const uint8_t* __restrict__ skip,
                                                int HW, int ntiles, QParams qp, const double* __restrict__ Echain,
                                                int16_t* __restrict__ tmp, unsigned long long* __restrict__ spec,
                                                const QState* __restrict__ tile_in, const uint8_t* __restrict__ swallowed,
                                                int* __restrict__ bad) {
    const int chain = blockIdx.x / (ntiles - 1), T = 1 + blockIdx.x % (ntiles - 1);
    const int f = chain / 3, c = chain % 3, lane = threadIdx.x;
    if (skip[f]) return;
    const size_t fe0 = (size_t)f * HW * 3;
    int16_t* t = tmp + fe0;
    const int nch = (HW + 63) >> 6;
    unsigned long long* sp = spec + (size_t)chain * nch;
    const int c0 = T * QT_CHUNKS, c1 = min(nch, c0 + QT_CHUNKS);
    if (swallowed[(size_t)chain * ntiles + T]) {   // the entering run covers the whole tile: none of its guessed heads is one
        if (c0 + lane < c1) sp[c0 + lane] = 0ull;
        return;
    }
    double E = 0.0;
    if (MAP) E = 0.0;   // (per element, from the map)
    else if (qp.mode == TZ_MODE_ABS) E = fabs(qp.b0);
    else if (qp.mode != TZ_MODE_PWREL) E = Echain[chain];
    const QState st = tile_in[(size_t)chain * ntiles + T];
    double u = st.u, l = st.l;
    int chead = st.head;
    bool merged = false;
    for (int ch = c0; ch < c1 && !merged; ++ch) {
        const QChunk q = MAP ? q_chunk<Q_TOL_MAP, FP>(src, orig, fe0, c, ch, HW, qp, E, lane, q_tol_map(Echain))
                         : qp.mode == TZ_MODE_PWREL ? q_chunk<Q_TOL_ORIG, FP>(src, orig, fe0, c, ch, HW, qp, E, lane)
                                                    : q_chunk<Q_TOL_CHAIN, FP>(src, orig, fe0, c, ch, HW, qp, E, lane);
        const unsigned long long S = sp[ch];
        const double eu = u < q.pu ? u : q.pu, el = l > q.pl ? l : q.pl;
        const unsigned long long brk = __ballot(eu - el < 0.0);
        if (brk == 0ull) {                  // the true run swallows the chunk: every guessed head in it is wrong
            if (lane == 0) sp[ch] = 0ull;
            u = q_rl_d(eu, 63);
            l = q_rl_d(el, 63);
            continue;
        }
        const int j0 = __ffsll((long long)brk) - 1;
        double uc = u, lc = l;
        if (j0 > 0) {
            uc = q_rl_d(eu, j0 - 1);
            lc = q_rl_d(el, j0 - 1);
        }
        const unsigned long long Tm = q_rl_u64(q.heads, j0);         // true heads of this chunk
        const unsigned long long common = Tm & S;
        const int m = common ? __ffsll((long long)common) - 1 : 64;  // first common head
        const unsigned long long below = m >= 64 ? ~0ull : ((1ull << m) - 1ull);
        const bool mine = (below >> lane) & 1ull;
        if (mine && ((Tm >> lane) & 1ull) && q.nxt < 64)
            t[(size_t)(ch * 64 + lane) * 3 + c] = (int16_t)(long long)((q.cu + q.cl) / 2);
        if (lane == 0) {
            sp[ch] = (S & ~below) | (Tm & below);
            t[(size_t)chead * 3 + c] = (int16_t)(long long)((uc + lc) / 2);   // the entering run closes at j0
        }
        if (common) {
            merged = true;
        } else {
            const int last = 63 - __clzll((long long)Tm);
            u = q_rl_d(q.cu, last);
            l = q_rl_d(q.cl, last);
            chead = ch * 64 + last;
        }
    }
    if (!merged && lane == 0) atomicOr(&bad[chain], 1);
}

// Exact serial walk of a whole chain (one wave, chunk after chunk: the algorithm of round 1), for the chains
// k_q_bstitch marked: the true chain crossed a whole 4096-element tile out of step with the tile's speculative chain
// (regular ramps do that).  Rewrites every mask word and run value of the chain.
template <bool FP, bool MAP>
__global__ __launch_bounds__(64) void k_q_serial(QSrc src, const uint8_t* __restrict__ orig, const uint8_t* __restrict__ skip, int HW,
                                               QParams qp, const double* __restrict__ Echain, int16_t* __restrict__ tmp,
                                               unsigned long long* __restrict__ spec, const int* __restrict__ bad) {
    const int chain = blockIdx.x, f = chain / 3, c = chain % 3, lane = threadIdx.x;
    if (skip[f] || !bad[chain] || HW <= 0) return;
    const size_t fe0 = (size_t)f * HW * 3;
    int16_t* t = tmp + fe0;
    const int nch = (HW + 63) >> 6;
    unsigned long long* sp = spec + (size_t)chain * nch;
    double E = 0.0;
    if (MAP) E = 0.0;   // (per element, from the map)
    else if (qp.mode == TZ_MODE_ABS) E = fabs(qp.b0);
    else if (qp.mode != TZ_MODE_PWREL) E = Echain[chain];
    double u = __builtin_huge_val(), l = -__builtin_huge_val();
    int chead = 0;
    for (int ch = 0; ch < nch; ++ch) {
        const QChunk q = MAP ? q_chunk<Q_TOL_MAP, FP>(src, orig, fe0, c, ch, HW, qp, E, lane, q_tol_map(Echain))
                         : qp.mode == TZ_MODE_PWREL ? q_chunk<Q_TOL_ORIG, FP>(src, orig, fe0, c, ch, HW, qp, E, lane)
                                                    : q_chunk<Q_TOL_CHAIN, FP>(src, orig, fe0, c, ch, HW, qp, E, lane);
        const unsigned long long first = ch == 0 ? 1ull : 0ull;
        const double eu = u < q.pu ? u : q.pu, el = l > q.pl ? l : q.pl;
        const unsigned long long brk = __ballot(eu - el < 0.0);
        if (brk == 0ull) {
            u = q_rl_d(eu, 63);
            l = q_rl_d(el, 63);
            if (lane == 0) sp[ch] = first;
            continue;
        }
        const int j0 = __ffsll((long long)brk) - 1;
        double uc = u, lc = l;
        if (j0 > 0) {
            uc = q_rl_d(eu, j0 - 1);
            lc = q_rl_d(el, j0 - 1);
        }
        if (lane == 0) t[(size_t)chead * 3 + c] = (int16_t)(long long)((uc + lc) / 2);
        const unsigned long long heads = q_rl_u64(q.heads, j0);
        const int last = 63 - __clzll((long long)heads);
        if (((heads >> lane) & 1ull) && q.nxt < 64) t[(size_t)(ch * 64 + lane) * 3 + c] = (int16_t)(long long)((q.cu + q.cl) / 2);
        if (lane == 0) sp[ch] = heads | first;
        u = q_rl_d(q.cu, last);
        l = q_rl_d(q.cl, last);
        chead = ch * 64 + last;
    }
    if (lane == 0) t[(size_t)chead * 3 + c] = (int16_t)(long long)((u + l) / 2);
}

static constexpr int QFB = QT_TILE;  // pixels per fill item = one tile of k_q_tiles (64 chunks of 64: a lane per mask word)

// value of the last run head in each fill item (from the masks: one thread per (frame, item, channel))
__global__ __launch_bounds__(256) void k_q_last(const int16_t* __restrict__ tmp, const unsigned long long* __restrict__ spec,
                                                const uint8_t* __restrict__ skip, int HW, int nch, int nblk, int nframes,
                                                int16_t* __restrict__ carry) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nframes * nblk * 3) return;
    const int c = id % 3, b = (id / 3) % nblk, f = id / (3 * nblk);
    if (skip[f]) return;
    const unsigned long long* sp = spec + (size_t)(f * 3 + c) * nch;
    const int w0 = b * (QFB / 64), w1 = min(nch, w0 + QFB / 64);
    int16_t v = TZ_SENTINEL;
    for (int w = w1 - 1; w >= w0; --w) {
        const unsigned long long m = sp[w];
        if (m) {
            const int pos = w * 64 + 63 - __clzll((long long)m);
            v = tmp[((size_t)f * HW + pos) * 3 + c];
            break;
        }
    }
    carry[((size_t)f * nblk + b) * 3 + c] = v;
}

// exclusive forward fill over the items of a chain, one wave per chain (64 items per pass; the last value seen
// carries from pass to pass); ftail = value of the chain's last run (its last element)
__global__ __launch_bounds__(64) void k_q_carry(int16_t* __restrict__ carry, const uint8_t* __restrict__ skip, int nblk, int nframes,
                                                int16_t* __restrict__ ftail) {
    const int id = blockIdx.x, lane = threadIdx.x;
    if (id >= nframes * 3) return;
    const int f = id / 3, c = id % 3;
    if (skip[f]) return;
    int run = (int)TZ_SENTINEL;
    for (int b0 = 0; b0 < nblk; b0 += 64) {
        const int b = b0 + lane;
        const size_t k = ((size_t)f * nblk + b) * 3 + c;
        const int v = b < nblk ? (int)carry[k] : (int)TZ_SENTINEL;
        const unsigned long long has = __ballot(v != (int)TZ_SENTINEL);
        const unsigned long long below = has & ((1ull << lane) - 1ull);       // items in front of mine that hold a head
        const int src = below ? 63 - __clzll((long long)below) : lane;
        const int got = __shfl(v, src, 64);
        if (b < nblk) carry[k] = (int16_t)(below ? got : run);                 // exclusive: last head value strictly before this item
        if (has) run = __shfl(v, 63 - __clzll((long long)has), 64);
    }
    if (lane == 0) ftail[id] = (int16_t)run;
}

// Forward fill of the run values back into a DELTA STACK (stand-alone tz_error_bound, delta tap of tz_encode; frames
// flagged in `skip` are not touched), one wave per 64-element chunk, no communication between waves: the masks say where
// the run heads are, so a lane finds the head of ITS run with bit operations (highest mask bit at or below its lane;
// else the highest bit of the nearest non-empty mask word in front of the chunk within its tile; else the tile's carry
// value from k_q_last / k_q_carry) and fetches the value there -- rounds 1-2 propagated the values themselves with 18
// shuffles and two barriers per 256 pixels.  (The fused encode uses k_q_fill_sym below.)
struct QFill {
    const int16_t* tmp;
    const unsigned long long* spec;
    const uint8_t *skip, *zero;
    const int16_t *carry, *ftail;
    const float* pred;
    const uint8_t* orig;
    int16_t* out;           // delta stack (in place) or symbols
    unsigned long long* hist;
    int16_t* edge;
    int HW, nch, nblk, nframes, apply_offset;
};

static constexpr int QF_THREADS = 512, QF_WAVES = QF_THREADS / 64;

// what a wave needs of one chunk before it can fetch run values: loaded one chunk AHEAD of its use, so that the
// mask / carry round trip of chunk k+1 overlaps the value gather and the stores of chunk k
struct QFillPre {
    unsigned long long mw[3], m[3];
    int cv[3];
    int skipped;
};

__device__ __forceinline__ QFillPre q_fill_pre(const QFill& a, int f, int ch, int lane) {
    QFillPre r;
    const int nch = a.nch;
    const int b = (ch * 64) / QFB, w0 = b * (QFB / 64);
    r.skipped = a.skip[f];
#pragma unroll
    for (int c = 0; c < 3; ++c) {   // (a skipped frame's entries are never written: loaded all the same, not used)
        const unsigned long long* sp = a.spec + (size_t)(f * 3 + c) * nch;
        const int wi = w0 + lane;
        r.mw[c] = (lane < QFB / 64 && wi < ch) ? sp[wi] : 0ull;   // the tile's mask words in front of the chunk, one per lane
        r.m[c] = sp[ch];
        r.cv[c] = (int)a.carry[((size_t)f * a.nblk + b) * 3 + c];  // value of the last head in front of the tile
    }
    return r;
}

__global__ __launch_bounds__(QF_THREADS) void k_q_fill(const QFill a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int HW = a.HW, nch = a.nch;
    // work item = (frame, chunk of 64 pixels, all three channels); a wave takes every (gridDim * waves)-th of them,
    // (f, ch) advanced without divisions
    const int wstride = (int)gridDim.x * QF_WAVES, df = wstride / nch, dch = wstride % nch;
    const int w_first = (int)blockIdx.x * QF_WAVES + wv;
    int f = w_first / nch, ch = w_first % nch;
    QFillPre nxt{};
    if (f < a.nframes) nxt = q_fill_pre(a, f, ch, lane);
    while (f < a.nframes) {
        const QFillPre cur = nxt;
        const int fc = f, chc = ch;
        f += df;
        ch += dch;
        if (ch >= nch) {
            ch -= nch;
            ++f;
        }
        if (f < a.nframes) nxt = q_fill_pre(a, f, ch, lane);
        if (cur.skipped) continue;
        const size_t fe0 = (size_t)fc * HW * 3;
        const int16_t* t = a.tmp + fe0;
        const int p = chc * 64 + lane;
        const int w0 = ((chc * 64) / QFB) * (QFB / 64);   // first mask word of the tile this chunk belongs to
        int hp[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned long long mw = cur.mw[c];
            const unsigned long long nz = __ballot(mw != 0ull);
            int before = -1;   // position of the last head in front of the chunk (within the tile), or -1
            if (nz) {
                const int wl = 63 - __clzll((long long)nz);
                const unsigned long long mm = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(mw >> 32), wl) << 32) |
                                              (unsigned)__builtin_amdgcn_readlane((int)(unsigned)mw, wl);
                before = (w0 + wl) * 64 + 63 - __clzll((long long)mm);
            }
            const unsigned long long mine = cur.m[c] & ((2ull << lane) - 1ull);
            hp[c] = mine ? chc * 64 + 63 - __clzll((long long)mine) : before;
        }
        int16_t tv[3];   // the gathers of the three channels go out together
#pragma unroll
        for (int c = 0; c < 3; ++c) tv[c] = hp[c] >= 0 ? t[(size_t)hp[c] * 3 + c] : (int16_t)0;
        if (p < HW)
#pragma unroll
            for (int c = 0; c < 3; ++c) a.out[fe0 + (size_t)p * 3 + c] = hp[c] >= 0 ? tv[c] : (int16_t)cur.cv[c];
    }
}

// Fused encode: forward fill + spatial delta + 1600 offset + histogram, tile by tile (the tiles of k_q_tiles), by
// resident blocks of three waves.  The values of a tile come in the way k_q_tiles left them -- 24 bytes per thread,
// dealt to three channel planes in LDS, row r = chunk r --; lane j of the channel's wave fills row j from its mask
// word (the value in front of the row comes from the nearest lane above that holds a head, else from the tile's carry);
// then the block walks the tile in memory order again, 4 pixels = 12 consecutive samples per thread: spatial delta in
// packed int16 arithmetic (the sample in front of a group is channel 2 of the pixel before it: LDS, or the tile's /
// frame's carry), symbols out in 24 bytes, histogram.  Frames the quantiser skips take their deltas from pred / orig
// (compress.py:292-314; 0 where zero_mask says so).  About 40 vector instructions per 12 symbols; the first version of
// the fused fill (a wave per 64-pixel chunk gathering run values from global memory, k_q_fill<true>) spent 300 per
// 192 and was bound by them: 193 us at cfg3.
template <bool HIST>
__global__ __launch_bounds__(192) void k_q_fill_sym(const QFill a) {
    __shared__ int planes[3 * 64 * QT_S16 / 2];
    __shared__ unsigned hraw[HIST ? HL_WORDS : 1];
    HistLds& hl = *(HistLds*)hraw;
    HistAcc acc;
    const int centre = a.apply_offset ? TZ_OFFSET : 0;
    if (HIST) hist_clear(hl);
    const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int HW = a.HW, nch = a.nch, ntiles = a.nblk;
    short* ls = (short*)planes + c * 64 * QT_S16;
    auto raw = [&](size_t e) { return (int)(a.pred[e] * 255.0f) - (int)a.orig[e]; };
    for (int item = blockIdx.x; item < a.nframes * ntiles; item += gridDim.x) {
        const int f = item / ntiles, T = item % ntiles;
        const bool skipped = a.skip[f] != 0, zero = skipped && a.zero[f] != 0;
        const size_t fe0 = (size_t)f * HW * 3;
        const int e0 = T * QT_TILE, npix = min(QT_TILE, HW - e0);
        __syncthreads();   // the previous item's readers of the planes are done
        // ---- A. the tile's values (or raw deltas) into the channel planes
        for (int g = threadIdx.x; g < QT_TILE / 4; g += 192) {
            const int p0 = g * 4;
            unsigned v[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k] = 0;
            if (p0 < npix && !zero) {
                const size_t e = fe0 + (size_t)(e0 + p0) * 3;
                if (skipped) {
                    const uint3 ob = *(const uint3*)(a.orig + e);
                    const unsigned ow[3] = {ob.x, ob.y, ob.z};
                    const float4* pp = (const float4*)(a.pred + e);
                    const float4 f0 = pp[0], f1 = pp[1], f2 = pp[2];
                    const float fv[12] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w, f2.x, f2.y, f2.z, f2.w};
#pragma unroll
                    for (int k = 0; k < 12; ++k) v[k] = (unsigned)((int)(fv[k] * 255.0f) - (int)((ow[k >> 2] >> (8 * (k & 3))) & 0xFFu)) & 0xFFFFu;
                } else {
                    const uint2* dp = (const uint2*)(a.tmp + e);
                    const uint2 a0 = dp[0], a1 = dp[1], a2 = dp[2];
                    const unsigned dw[6] = {a0.x, a0.y, a1.x, a1.y, a2.x, a2.y};
#pragma unroll
                    for (int k = 0; k < 12; ++k) v[k] = (dw[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
                }
            }
            const int row = p0 >> 6, col = p0 & 63;
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                unsigned* w = (unsigned*)((short*)planes + cc * 64 * QT_S16 + row * QT_S16 + col);
                w[0] = v[cc] | (v[3 + cc] << 16);
                w[1] = v[6 + cc] | (v[9 + cc] << 16);
            }
        }
        __syncthreads();
        // ---- B. forward fill of my row
        const int cv = skipped ? 0 : (int)a.carry[((size_t)f * ntiles + T) * 3 + c];   // value of the last head in front of the tile
        if (!skipped) {
            const int chunk = T * QT_CHUNKS + lane;
            const unsigned long long M = chunk < nch ? a.spec[(size_t)(f * 3 + c) * nch + chunk] : 0ull;
            const int lastv = M ? (int)ls[lane * QT_S16 + 63 - __clzll((long long)M)] : 0;
            const unsigned long long has = __ballot(M != 0ull), below = has & ((1ull << lane) - 1ull);
            const int got = __shfl(lastv, below ? 63 - __clzll((long long)below) : lane, 64);
            int cur = below ? got : cv;
            __builtin_amdgcn_wave_barrier();   // every lane has read its lastv before any row is rewritten
            const int len = max(0, min(64, npix - lane * 64));
            for (int tt = 0; tt < len; ++tt) {
                const int x = (int)ls[lane * QT_S16 + tt];
                cur = ((M >> tt) & 1ull) ? x : cur;
                ls[lane * QT_S16 + tt] = (short)cur;
            }
        }
        __syncthreads();
        // ---- C. memory order again: spatial delta, offset, histogram, symbols
        // the sample in front of the tile's first one
        int tprev = 0;
        bool tfirst = false;   // start of the stream: sd[0] = x[0]
        if (T > 0) {
            tprev = skipped ? (zero ? 0 : raw(fe0 + (size_t)e0 * 3 - 1)) : (int)a.carry[((size_t)f * ntiles + T) * 3 + 2];
        } else if (f > 0) {
            if (a.skip[f - 1]) tprev = a.zero[f - 1] ? 0 : raw(fe0 - 1);
            else tprev = (int)a.ftail[(f - 1) * 3 + 2];
        } else {
            tfirst = true;
        }
        for (int g = threadIdx.x; g < QT_TILE / 4; g += 192) {
            const int p0 = g * 4;
            if (p0 >= npix) continue;
            const int row = p0 >> 6, col = p0 & 63;
            unsigned r[12];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                const unsigned* w = (const unsigned*)((const short*)planes + cc * 64 * QT_S16 + row * QT_S16 + col);
                const unsigned w0 = w[0], w1 = w[1];
                r[cc] = w0 & 0xFFFFu;
                r[3 + cc] = w0 >> 16;
                r[6 + cc] = w1 & 0xFFFFu;
                r[9 + cc] = w1 >> 16;
            }
            unsigned V[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) V[k] = r[2 * k] | (r[2 * k + 1] << 16);
            unsigned prev16;
            if (p0 > 0) prev16 = (unsigned)(unsigned short)((const short*)planes)[2 * 64 * QT_S16 + ((p0 - 1) >> 6) * QT_S16 + ((p0 - 1) & 63)];
            else prev16 = tfirst ? ((V[0] << 1) & 0xFFFFu) : ((unsigned)tprev & 0xFFFFu);   // sd[0] = x[0] as "prev = 2 x[0]"
            unsigned Y[6];
            unsigned hi = prev16 << 16;
            const unsigned C2 = ((unsigned)TZ_OFFSET << 16) | (unsigned)TZ_OFFSET;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const unsigned P = __builtin_amdgcn_alignbit(V[k], hi, 16);
                hi = V[k];
                Y[k] = pk_sub(P, V[k]);
                if (a.apply_offset) Y[k] = pk_sub(C2, Y[k]);
            }
            uint2* dst = (uint2*)(a.out + fe0 + (size_t)(e0 + p0) * 3);
            dst[0] = make_uint2(Y[0], Y[1]);
            dst[1] = make_uint2(Y[2], Y[3]);
            dst[2] = make_uint2(Y[4], Y[5]);
            if (HIST) hist_add<6>(hl, acc, Y, centre);
            if (f == 0 && T == 0 && p0 == 0) a.edge[0] = (int16_t)(short)r[0];
            if (f == a.nframes - 1 && e0 + p0 + 4 == HW) a.edge[1] = (int16_t)(short)r[11];
        }
    }
    if (HIST) hist_flush(hl, acc, centre, a.hist);
}

struct QFused {   // fused encode: symbols + histogram + edge elements instead of a delta stack
    const float* pred;
    const uint8_t* d_zero;
    int apply_offset;
    int16_t* sym;
    unsigned long long* d_hist;
    int16_t* d_edge;
};

// h_fb (may be NULL): nframes abs tolerances, one per frame, in place of (mode, b0, b1).  The walks run in their per-chain
// form, the one rel / absrel run: k_q_frame_bound fills the array k_q_bound would fill, and a frame whose bound is 0 is
// skipped, which is what `abs 0` does to it (compress.py:24).
// d_map (may be NULL; device, H * W bytes): the bound map of TZ-BM1 in place of (mode, b0, b1) -- the per-element walks with the map as
// their tolerance source (Q_TOL_MAP).  Every scratch block below is what a pwrel job allocates: nothing of the map's is expanded
// per frame or channel.  orig may then be NULL unless `fu` forms the deltas from it.
static int quant_run(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const QFused* fu, const uint8_t* h_skip, int nframes,
                     int H, int W, int mode, double b0, double b1, const double* h_fb = nullptr, const uint8_t* d_map = nullptr) {
    int HW = H * W;
    size_t fe = (size_t)HW * 3;
    int nblk = (HW + QFB - 1) / QFB;
    void *d_skip, *d_E, *d_tmp, *d_carry, *d_mm, *d_spec, *d_ftail;
    TZ_TRY(tz_pool_alloc(ctx, nframes, &d_skip));
    TZ_TRY(tz_pool_alloc(ctx, sizeof(double) * 3 * nframes, &d_E));
    TZ_TRY(tz_pool_alloc(ctx, sizeof(int) * 6 * nframes, &d_mm));
    TZ_TRY(tz_pool_alloc(ctx, fe * nframes * 2, &d_tmp));
    TZ_TRY(tz_pool_alloc(ctx, (size_t)nframes * nblk * 3 * 2, &d_carry));
    TZ_TRY(tz_pool_alloc(ctx, (size_t)nframes * 3 * 2, &d_ftail));
    const int nch = (HW + 63) / 64;
    TZ_TRY(tz_pool_alloc(ctx, (size_t)nframes * 3 * nch * sizeof(unsigned long long), &d_spec));
    std::vector<uint8_t> fb_skip;
    void* d_fb = nullptr;
    if (h_fb) {
        fb_skip.assign(h_skip, h_skip + nframes);
        for (int f = 0; f < nframes; ++f)
            if (h_fb[f] == 0.0) fb_skip[f] = 1;
        h_skip = fb_skip.data();
        TZ_TRY(tz_pool_alloc(ctx, sizeof(double) * nframes, &d_fb));
        TZ_TRY(tz_upload(ctx, d_fb, h_fb, sizeof(double) * nframes));
        mode = TZ_MODE_REL;   // what makes every walk read Echain; no kernel below reads b0 or b1 in this mode
        b0 = b1 = 0.0;
    }
    if (d_map) {
        mode = TZ_MODE_PWREL;   // what makes every walk per element; no kernel below reads b0 or b1 under Q_TOL_MAP
        b0 = b1 = 0.0;
    }
    TZ_TRY(tz_upload(ctx, d_skip, h_skip, nframes));
    QParams qp{mode, b0, b1};
    QSrc src{diff, fu ? fu->pred : nullptr};
    if (d_map) d_E = (void*)d_map;   // (q_tol_map: the walks' Echain slot carries the map; the pool block is handed back with the call)
    {
        tz_prof_scope ps(ctx, TZP_QUANT);
        if (h_fb) {
            hipLaunchKernelGGL(k_q_frame_bound, dim3((3 * nframes + 63) / 64), dim3(64), 0, ctx->stream, (const double*)d_fb,
                               (const uint8_t*)d_skip, nframes, (double*)d_E);
        } else if (mode == TZ_MODE_REL || mode == TZ_MODE_ABSREL) {
            hipLaunchKernelGGL(k_q_mm_init, dim3((6 * nframes + 255) / 256), dim3(256), 0, ctx->stream, (int*)d_mm, 6 * nframes);
            hipLaunchKernelGGL(k_q_minmax, dim3(QBB, nframes), dim3(256), 0, ctx->stream, orig, (const uint8_t*)d_skip, HW,
                               (int*)d_mm);
            hipLaunchKernelGGL(k_q_bound, dim3((3 * nframes + 63) / 64), dim3(64), 0, ctx->stream, (const int*)d_mm,
                               (const uint8_t*)d_skip, qp, nframes, (double*)d_E);
        }
        {
            const int ntiles = (nch + QT_CHUNKS - 1) / QT_CHUNKS, nchains = nframes * 3;
            void *d_width, *d_tout, *d_tin, *d_tagg, *d_swal, *d_bad;
            TZ_TRY(tz_pool_alloc(ctx, sizeof(QWidth) * nchains, &d_width));
            TZ_TRY(tz_pool_alloc(ctx, sizeof(QState) * (size_t)nchains * ntiles, &d_tout));
            TZ_TRY(tz_pool_alloc(ctx, sizeof(QState) * (size_t)nchains * ntiles, &d_tin));
            TZ_TRY(tz_pool_alloc(ctx, sizeof(double2) * (size_t)nchains * ntiles, &d_tagg));
            TZ_TRY(tz_pool_alloc(ctx, (size_t)nchains * ntiles, &d_swal));
            TZ_TRY(tz_pool_alloc(ctx, sizeof(int) * nchains, &d_bad));
            TZ_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof(int) * nchains, ctx->stream));
            const bool pw = mode == TZ_MODE_PWREL;
            if (!pw)
                hipLaunchKernelGGL(k_q_width, dim3(nchains), dim3(64), 0, ctx->stream, (const double*)d_E, (const uint8_t*)d_skip, qp,
                                   (QWidth*)d_width);
#define TZ_Q_TILES(PWV, FPV)                                                                                                    \
    hipLaunchKernelGGL((k_q_tiles<PWV, FPV>), dim3(nframes * ntiles), dim3(192), 0, ctx->stream, src, orig, (const uint8_t*)d_skip, HW, \
                       ntiles, qp, (const double*)d_E, (const QWidth*)d_width, (int16_t*)d_tmp, (unsigned long long*)d_spec,         \
                       (QState*)d_tout, (double2*)d_tagg)
            if (d_map && fu) TZ_Q_TILES(Q_TOL_MAP, true);
            else if (d_map) TZ_Q_TILES(Q_TOL_MAP, false);
            else if (pw && fu) TZ_Q_TILES(Q_TOL_ORIG, true);
            else if (pw) TZ_Q_TILES(Q_TOL_ORIG, false);
            else if (fu) TZ_Q_TILES(Q_TOL_CHAIN, true);
            else TZ_Q_TILES(Q_TOL_CHAIN, false);
#undef TZ_Q_TILES
            hipLaunchKernelGGL(k_q_chain, dim3(nchains), dim3(64), 0, ctx->stream, (const uint8_t*)d_skip, HW, ntiles,
                               (const QState*)d_tout, (const double2*)d_tagg, (QState*)d_tin, (uint8_t*)d_swal, (int16_t*)d_tmp);
            if (ntiles > 1) {
#define TZ_Q_STITCH(FPV, MAPV)                                                                                                  \
    do {                                                                                                                        \
        hipLaunchKernelGGL((k_q_bstitch<FPV, MAPV>), dim3(nchains * (ntiles - 1)), dim3(64), 0, ctx->stream, src, orig,          \
                           (const uint8_t*)d_skip, HW, ntiles, qp, (const double*)d_E, (int16_t*)d_tmp,                         \
                           (unsigned long long*)d_spec, (const QState*)d_tin, (const uint8_t*)d_swal, (int*)d_bad);             \
        hipLaunchKernelGGL((k_q_serial<FPV, MAPV>), dim3(nchains), dim3(64), 0, ctx->stream, src, orig, (const uint8_t*)d_skip,  \
                           HW, qp, (const double*)d_E, (int16_t*)d_tmp, (unsigned long long*)d_spec, (const int*)d_bad);        \
    } while (0)
                if (fu && d_map) TZ_Q_STITCH(true, true);
                else if (fu) TZ_Q_STITCH(true, false);
                else if (d_map) TZ_Q_STITCH(false, true);
                else TZ_Q_STITCH(false, false);
#undef TZ_Q_STITCH
                if (ctx->prof_on) {   // how many chains took the fallback (a test asserts that its ramps really do)
                    std::vector<int> hb(nchains, 0);
                    TZ_HIP(ctx, hipMemcpyAsync(hb.data(), d_bad, sizeof(int) * nchains, hipMemcpyDeviceToHost, ctx->stream));
                    TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
                    for (int v : hb) ctx->prof[TZP_QSERIAL].launches += v != 0;
                }
            }
        }
        hipLaunchKernelGGL(k_q_last, dim3((nframes * nblk * 3 + 255) / 256), dim3(256), 0, ctx->stream, (const int16_t*)d_tmp,
                           (const unsigned long long*)d_spec, (const uint8_t*)d_skip, HW, nch, nblk, nframes, (int16_t*)d_carry);
        hipLaunchKernelGGL(k_q_carry, dim3(nframes * 3), dim3(64), 0, ctx->stream, (int16_t*)d_carry,
                           (const uint8_t*)d_skip, nblk, nframes, (int16_t*)d_ftail);
    }
    QFill a{};
    a.tmp = (const int16_t*)d_tmp;
    a.spec = (const unsigned long long*)d_spec;
    a.skip = (const uint8_t*)d_skip;
    a.carry = (const int16_t*)d_carry;
    a.ftail = (const int16_t*)d_ftail;
    a.HW = HW;
    a.nch = nch;
    a.nblk = nblk;
    a.nframes = nframes;
    const long long nwork = (long long)nframes * nch;
    const int grid = (int)std::min<long long>(4 * kCUs, (nwork + QF_WAVES - 1) / QF_WAVES);
    if (!fu) {
        tz_prof_scope ps(ctx, TZP_QUANT);
        a.out = diff;
        hipLaunchKernelGGL(k_q_fill, dim3(grid), dim3(QF_THREADS), 0, ctx->stream, a);
    } else {
        tz_prof_scope ps(ctx, TZP_SDELTA);
        a.zero = fu->d_zero;
        a.pred = fu->pred;
        a.orig = orig;
        a.out = fu->sym;
        a.hist = fu->d_hist;
        a.edge = fu->d_edge;
        a.apply_offset = fu->apply_offset;
        const int gsym = std::min(4 * kCUs, nframes * nblk);
        if (fu->d_hist) hipLaunchKernelGGL(k_q_fill_sym<true>, dim3(gsym), dim3(192), 0, ctx->stream, a);
        else hipLaunchKernelGGL(k_q_fill_sym<false>, dim3(gsym), dim3(192), 0, ctx->stream, a);
    }
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_error_bound(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* h_skip, int nframes, int H,
                    int W, int mode, double b0, double b1) {
    if (mode < 0 || mode > 3) return tz_fail(ctx, TZ_ERR_INVALID, "unknown error-bound mode %d", mode);
    if (b0 == 0.0) return TZ_OK;                          // compress.py:24
    if (mode == TZ_MODE_ABSREL && b1 == 0.0) return TZ_OK;  // compress.py:35
    if ((mode == TZ_MODE_PWREL || mode == TZ_MODE_REL) && b0 < 0.0)
        return tz_fail(ctx, TZ_ERR_INVALID, "%s bound must be >= 0 (the reference raises on a negative one)", mode == TZ_MODE_REL ? "rel" : "pwrel");
    if (mode == TZ_MODE_ABSREL && b1 < 0.0)
        return tz_fail(ctx, TZ_ERR_INVALID, "the rel bound of absrel must be >= 0 (the reference raises on a negative one)");
    // a NaN tolerance makes every run's value (u + l) / 2 NaN: the reference raises assigning it into its int array
    if (std::isnan(b0) || (mode == TZ_MODE_ABSREL && std::isnan(b1)))
        return tz_fail(ctx, TZ_ERR_INVALID, "error bound is NaN (the reference raises on a NaN tolerance)");
    if (nframes <= 0 || H <= 0 || W <= 0) return TZ_OK;
    return quant_run(ctx, orig, diff, nullptr, h_skip, nframes, H, W, mode, b0, b1);
}

// Lossy fused encode (compress.py:292-355 without a delta stack in memory): applies to unpadded frames with
// whole 16-byte groups per frame; *done says whether it ran (else the caller takes the unfused kernels).
int tzk_quant_sd_fused(tz_ctx* ctx, const float* pred, const uint8_t* orig, const uint8_t* d_zero_mask, const uint8_t* h_skip,
                       int nframes, int H, int W, int Hp, int Wp, int mode, double b0, double b1, int apply_offset,
                       int16_t* sym, unsigned long long* d_hist, int16_t* d_edge, bool* done) {
    *done = false;
    if (mode < 0 || mode > 3) return tz_fail(ctx, TZ_ERR_INVALID, "unknown error-bound mode %d", mode);
    // a negative tolerance makes the reference assign NaN into its int array (compress.py:61 at the first element): it raises
    if ((mode == TZ_MODE_PWREL || mode == TZ_MODE_REL) && b0 < 0.0)
        return tz_fail(ctx, TZ_ERR_INVALID, "%s bound must be >= 0 (the reference raises on a negative one)", mode == TZ_MODE_REL ? "rel" : "pwrel");
    if (mode == TZ_MODE_ABSREL && b1 < 0.0)
        return tz_fail(ctx, TZ_ERR_INVALID, "the rel bound of absrel must be >= 0 (the reference raises on a negative one)");
    // a NaN tolerance makes every run's value (u + l) / 2 NaN: the reference raises assigning it into its int array
    if (std::isnan(b0) || (mode == TZ_MODE_ABSREL && std::isnan(b1)))
        return tz_fail(ctx, TZ_ERR_INVALID, "error bound is NaN (the reference raises on a NaN tolerance)");
    if (H != Hp || W != Wp || ((size_t)H * W) % 8 || nframes <= 0 || (((uintptr_t)sym) & 15)) return TZ_OK;
    if ((((uintptr_t)pred & 15) | ((uintptr_t)orig & 3)) != 0) return TZ_OK;   // k_q_fill_sym: 16-byte pred, 4-byte orig loads
    QFused fu{pred, d_zero_mask, apply_offset, sym, d_hist, d_edge};
    TZ_TRY(quant_run(ctx, orig, nullptr, &fu, h_skip, nframes, H, W, mode, b0, b1));
    *done = true;
    return TZ_OK;
}

// `abs` with one tolerance per frame (tz_set_frame_bounds, tz_error_bound_frames): frame f is quantised as `abs h_bounds[f]`
// quantises it, bit for bit -- the walks read the same E, from the per-chain array instead of the launch's parameters.
// diff != NULL: the delta stack is quantised in place, as by tzk_error_bound.  diff == NULL: the fused lossy front on
// pred / orig, as tzk_quant_sd_fused and under its conditions; *done says whether it ran.  The entries are finite and >= 0
// (the setters check).
int tzk_quant_frames(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const tz_quant_fused* fu, const uint8_t* h_skip, int nframes,
                     int H, int W, const double* h_bounds, bool* done) {
    if (done) *done = false;
    if (nframes <= 0 || H <= 0 || W <= 0) return TZ_OK;
    if (diff) {
        bool any = false;
        for (int f = 0; f < nframes; ++f) any = any || (h_bounds[f] != 0.0 && !h_skip[f]);
        if (!any) return TZ_OK;   // every frame is left as it is
        return quant_run(ctx, orig, diff, nullptr, h_skip, nframes, H, W, TZ_MODE_ABS, 0.0, 0.0, h_bounds);
    }
    if (H != fu->Hp || W != fu->Wp || ((size_t)H * W) % 8 || (((uintptr_t)fu->sym) & 15)) return TZ_OK;
    if ((((uintptr_t)fu->pred & 15) | ((uintptr_t)orig & 3)) != 0) return TZ_OK;   // k_q_fill_sym: 16-byte pred, 4-byte orig loads
    QFused q{fu->pred, fu->d_zero_mask, fu->apply_offset, fu->sym, fu->d_hist, fu->d_edge};
    TZ_TRY(quant_run(ctx, orig, nullptr, &q, h_skip, nframes, H, W, TZ_MODE_ABS, 0.0, 0.0, h_bounds));
    *done = true;
    return TZ_OK;
}

// The bound map TZ-BM1 (tz_set_bound_map, tz_error_bound_map): every sample of pixel p is quantised under the abs tolerance
// d_map[p] (device, H * W bytes), by the reference's pwrel walk with the map in place of orig * b0.  diff != NULL: the delta
// stack is quantised in place (orig is not read).  diff == NULL: the fused lossy front on pred / orig, as tzk_quant_sd_fused and
// under its conditions; *done says whether it ran.
int tzk_quant_map(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const tz_quant_fused* fu, const uint8_t* h_skip, int nframes, int H,
                  int W, const uint8_t* d_map, bool* done) {
    if (done) *done = false;
    if (nframes <= 0 || H <= 0 || W <= 0) return TZ_OK;
    if (diff) return quant_run(ctx, orig, diff, nullptr, h_skip, nframes, H, W, TZ_MODE_ABS, 0.0, 0.0, nullptr, d_map);
    if (H != fu->Hp || W != fu->Wp || ((size_t)H * W) % 8 || (((uintptr_t)fu->sym) & 15)) return TZ_OK;
    if ((((uintptr_t)fu->pred & 15) | ((uintptr_t)orig & 3)) != 0) return TZ_OK;   // k_q_fill_sym: 16-byte pred, 4-byte orig loads
    QFused q{fu->pred, fu->d_zero_mask, fu->apply_offset, fu->sym, fu->d_hist, fu->d_edge};
    TZ_TRY(quant_run(ctx, orig, nullptr, &q, h_skip, nframes, H, W, TZ_MODE_ABS, 0.0, 0.0, nullptr, d_map));
    *done = true;
    return TZ_OK;
}

// ------------------------------------------------------- spatial delta (+offset, histogram)
// compress.py:73-77: out[0]=in[0], out[i]=in[i-1]-in[i] over the whole flat array (int16
// wrap); compress.py:348: y = 1600 - sd; compress.py:354: bincount(y).
// 8 elements (16 B) per lane; the element before a lane's first comes from one extra 2-byte
// load (same cache line).  Histogram: HistLds / HistAcc above.
template <bool HIST>
__global__ __launch_bounds__(HIST ? HB_THREADS : 256) void k_sdelta(const int16_t* __restrict__ in, size_t n, int has_carry, int16_t carry,
                                                int apply_offset, int16_t* __restrict__ out,
                                                unsigned long long* __restrict__ hist) {
    __shared__ unsigned hraw[HIST ? HL_WORDS : 1];
    HistLds& hl = *(HistLds*)hraw;
    if (HIST) hist_clear(hl);
    const int centre = apply_offset ? TZ_OFFSET : 0;
    HistAcc acc;
    size_t n8 = n / 8;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint4* in8 = (const uint4*)in;
    uint4* out8 = (uint4*)out;
    const unsigned short* inu = (const unsigned short*)in;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const uint4 v = in8[i];
        // the element in front; without one (start of the stream, no carry) sd[0] = x[0], i.e. "prev" = 2 x[0]
        unsigned prev = i ? (unsigned)inu[8 * i - 1] : (has_carry ? (unsigned)(unsigned short)carry : ((v.x << 1) & 0xFFFFu));
        unsigned Y[4];
        sdelta8(v, prev, apply_offset != 0, Y);
        out8[i] = make_uint4(Y[0], Y[1], Y[2], Y[3]);
        if (HIST) hist_add8(hl, acc, Y, centre);
    }
    // tail (n % 8 elements) by the first lanes of block 0
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
        size_t i = n8 * 8 + threadIdx.x;
        short cur = in[i];
        short sd = i ? (short)(in[i - 1] - cur) : (has_carry ? (short)(carry - cur) : cur);
        short y = apply_offset ? (short)(TZ_OFFSET - sd) : sd;
        out[i] = y;
        if (HIST && y >= 0 && y < TZ_NBINS) atomicAdd(&hl.w[HL_FULL + y], 1u);
    }
    if (HIST) hist_flush(hl, acc, centre, hist);
}

// Lossless fast path (error_bound is the identity, compress.py:24): delta, spatial delta,
// 1600 offset and histogram in ONE pass over pred/orig -- 7 B/element instead of 7 + 4.
// Same arithmetic as k_delta_flat followed by k_sdelta; the element before a lane's first is
// recomputed from pred/orig (one extra float + byte, same cache lines).
template <bool HIST>
__global__ __launch_bounds__(HIST ? HB_THREADS : 256) void k_delta_sd_fused(const float4* __restrict__ pred, const uint2* __restrict__ orig,
                                                        const uint8_t* __restrict__ zero_mask, size_t n8,
                                                        unsigned frame_elems8, int apply_offset,
                                                        short8* __restrict__ out, unsigned long long* __restrict__ hist,
                                                        int16_t* __restrict__ edge) {
    __shared__ unsigned hraw[HIST ? HL_WORDS : 1];
    HistLds& hl = *(HistLds*)hraw;
    constexpr bool do_hist = HIST;
    if (do_hist) hist_clear(hl);
    const int centre = apply_offset ? TZ_OFFSET : 0;
    HistAcc acc;
    const float* predf = (const float*)pred;
    const uint8_t* origb = (const uint8_t*)orig;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        float4 p0 = pred[2 * i], p1 = pred[2 * i + 1];
        uint2 o = orig[i];
        const bool zero = zero_mask[i / frame_elems8] != 0;
        short d[8];
        d[0] = (short)((int)(p0.x * 255.0f) - (int)(o.x & 0xff));
        d[1] = (short)((int)(p0.y * 255.0f) - (int)((o.x >> 8) & 0xff));
        d[2] = (short)((int)(p0.z * 255.0f) - (int)((o.x >> 16) & 0xff));
        d[3] = (short)((int)(p0.w * 255.0f) - (int)(o.x >> 24));
        d[4] = (short)((int)(p1.x * 255.0f) - (int)(o.y & 0xff));
        d[5] = (short)((int)(p1.y * 255.0f) - (int)((o.y >> 8) & 0xff));
        d[6] = (short)((int)(p1.z * 255.0f) - (int)((o.y >> 16) & 0xff));
        d[7] = (short)((int)(p1.w * 255.0f) - (int)(o.y >> 24));
        short prev = 0;
        if (i) {
            size_t e = 8 * i - 1;
            if (!zero_mask[(i * 8 - 1) / ((size_t)frame_elems8 * 8)]) prev = (short)((int)(predf[e] * 255.0f) - (int)origb[e]);
        }
        // pack the (masked) deltas two per dword and take the spatial delta in packed int16 arithmetic
        uint4 V;
        {
            unsigned q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                q[j] = zero ? 0u : (((unsigned)(unsigned short)d[2 * j]) | ((unsigned)(unsigned short)d[2 * j + 1] << 16));
            V = make_uint4(q[0], q[1], q[2], q[3]);
        }
        const unsigned pv = i ? (unsigned)(unsigned short)prev : ((V.x << 1) & 0xFFFFu);   // stream start: sd[0] = x[0]
        unsigned Y[4];
        sdelta8(V, pv, apply_offset != 0, Y);
        ((uint4*)out)[i] = make_uint4(Y[0], Y[1], Y[2], Y[3]);
        if (do_hist) hist_add8(hl, acc, Y, centre);
        // first / last element of the delta stack (shard boundaries, tz_encode_begin)
        if (i == 0) edge[0] = zero ? (short)0 : d[0];
        if (i == n8 - 1) edge[1] = zero ? (short)0 : d[7];
    }
    if (do_hist) hist_flush(hl, acc, centre, hist);
}

// returns TZ_OK and sets *done when the fused path applies (unpadded frames, whole 8-element groups)
int tzk_delta_sd_fused(tz_ctx* ctx, const float* pred, const uint8_t* orig, const uint8_t* d_zero_mask, int nframes, int H,
                       int W, int Hp, int Wp, int apply_offset, int16_t* out, unsigned long long* d_hist, int16_t* d_edge,
                       bool* done) {
    *done = false;
    size_t fe = (size_t)H * W * 3;
    if (H != Hp || W != Wp || fe % 8 || nframes <= 0) return TZ_OK;
    if (((((uintptr_t)pred | (uintptr_t)out) & 15) | ((uintptr_t)orig & 7)) != 0) return TZ_OK;   // 16-byte pred / out, 8-byte orig accesses
    size_t n8 = fe * nframes / 8;
    tz_prof_scope ps(ctx, TZP_DELTA);
    if (d_hist)
        hipLaunchKernelGGL(k_delta_sd_fused<true>, dim3(std::min(HB_GRID, grid_for(n8, HB_THREADS))), dim3(HB_THREADS), 0, ctx->stream,
                           (const float4*)pred, (const uint2*)orig, d_zero_mask, n8, (unsigned)(fe / 8), apply_offset, (short8*)out,
                           d_hist, d_edge);
    else
        hipLaunchKernelGGL(k_delta_sd_fused<false>, dim3(grid_for(n8, 256)), dim3(256), 0, ctx->stream, (const float4*)pred,
                           (const uint2*)orig, d_zero_mask, n8, (unsigned)(fe / 8), apply_offset, (short8*)out, d_hist, d_edge);
    TZ_HIP(ctx, hipGetLastError());
    *done = true;
    return TZ_OK;
}

// When is error_bound (compress.py:23-70) the IDENTITY on a stack of integer deltas?  (round 6)
// The greedy walk closes a run at the first element i with min(u, Du[i]) - max(l, Dl[i]) < 0, Du = d + E, Dl = d - E in
// float64, and gives the run trunc((u + l) / 2).  Deltas are integers (|d| <= 255 in the encoder, compress.py:292-314).
//  (1) With E <= 0.499 two DIFFERENT neighbours a != b always close the run: (min - max) = -|a - b| + 2E <= -0.002, three
//      orders of magnitude beyond the rounding of sums below 256; two EQUAL ones never do: fl(d + E) >= fl(d - E) for
//      E >= 0 (rounding is monotone).  So every run is a run of equal deltas d, u = fl(d + E), l = fl(d - E).
//  (2) fl(u + l) = 2d exactly, hence the run's value is d.  u and l are multiples of their ulp; unless d is a power of two
//      they share one binade (ulp q): |u + l - 2d| = |e_u + e_l| <= q with equality only if both roundings were ties in
//      the same direction -- but 2d is an even multiple of q, so when d + E lies halfway between k q and (k + 1) q, d - E
//      lies halfway between (m - k - 1) q and (m - k) q with m even: round-to-even sends the two opposite ways.  So
//      u + l - 2d is a multiple of q smaller than q: zero.  For d = 2^k (u in the upper binade, ulp 2q; l in the lower,
//      ulp q) u + l - 2d is one of -q, 0, +q; 2d + q rounds down to 2d (spacing 4q above 2^(k+1)), 2d - q is a tie
//      between 2d - 2q and 2d = 2^(k+1), whose mantissa is even.  d = 0: u + l = E - E = 0.
//      (Checked numerically over every integer d in [-255, 255] for 200,000 random and all 3- and 4-digit tolerances.)
// Per-chain tolerances (compress.py:28-48): abs |b0|; rel range * b0 with range <= 255; absrel the smaller of the two --
// so the WORST case over the chains of a job decides, before any data is looked at.  pwrel has a tolerance per ELEMENT,
// E_i = orig_i * b0 <= 255 b0: (1) holds with the elements' own tolerances (all <= 0.499), and a run of equal deltas d has
// u = min fl(d + E_i) = fl(d + min E_i), l = max fl(d - E_i) = fl(d - min E_i) (rounding is monotone) -- the same
// tolerance on both sides, so (2) applies.  BASELINE.json's cfg3 (`rel 1e-3`: E <= 0.255) is such a job: SURVEY.md section 8(d) calls it
// "effectively lossless", and the reference's own runs at such tolerances decode bit-exact (tests/golden/ref_runs4.npz).
static constexpr double kQIdentityMaxE = 0.499;

bool tz_quant_is_identity(int mode, double b0, double b1) {
    static const bool enabled = !getenv("TEZIP_QMAP") || atoi(getenv("TEZIP_QMAP")) != 0;   // (0: A/B against the general quantiser)
    // a NaN tolerance goes to the general path, which refuses it (std::min(|b0|, NaN) would be |b0|: absrel 0.3 nan looked
    // like the identity and was encoded lossless)
    if (std::isnan(b0) || (mode == TZ_MODE_ABSREL && std::isnan(b1))) return false;
    double worst;
    if (mode == TZ_MODE_ABS) worst = fabs(b0);
    else if (mode == TZ_MODE_REL) worst = 255.0 * b0;
    else if (mode == TZ_MODE_ABSREL) worst = std::min(fabs(b0), 255.0 * b1);
    else if (mode == TZ_MODE_PWREL) worst = 255.0 * b0;
    else return false;
    return enabled && worst >= 0.0 && worst <= kQIdentityMaxE;   // (a NaN or a negative tolerance: the general path and its errors)
}

// ------------------------------------------------- spatial delta of channel 0 alone (one-channel payload of a gray job)
// tz_set_payload_channels(1): finding_difference (compress.py:73-77) over channel 0 of the interleaved (frame, y, x, 3) stack,
// out[0] = x[0] (or carry - x[0]), out[p] = x[3(p-1)] - x[3p]; then 1600 - y and the histogram as k_sdelta.  Channels 1 and 2
// are fetched with the cache lines they share with channel 0 and never looked at.
// Fast form: a lane takes 8 pixels, i.e. 24 elements as three 16-byte loads, picks the 8 channel-0 halves out of the 12
// dwords, and writes one 16-byte store; the channel-0 element in front of its first pixel is one extra 2-byte load (the cache
// line of the neighbouring lane).  `head` pixels in front (those up to the first pixel at which in3 AND out are 16-byte
// aligned; all npix when there is no such pixel) and the npix - head - 8 n8 pixels behind go one by one.
// edge (may be NULL): edge[0], edge[1] = the first and the last channel-0 element, as encode_front leaves them.
__device__ __forceinline__ void sdelta_gray1(const int16_t* __restrict__ in, size_t p, int has_carry, int16_t carry, int apply_offset,
                                             int16_t* __restrict__ out, HistLds* hl) {
    const short cur = in[3 * p];
    const short sd = p ? (short)(in[3 * (p - 1)] - cur) : (has_carry ? (short)(carry - cur) : cur);
    const short y = apply_offset ? (short)(TZ_OFFSET - sd) : sd;
    out[p] = y;
    if (hl && y >= 0 && y < TZ_NBINS) atomicAdd(&hl->w[HL_FULL + y], 1u);
}

template <bool HIST>
__global__ __launch_bounds__(HIST ? HB_THREADS : 256) void k_sdelta_gray(const int16_t* __restrict__ in, size_t npix, size_t head, size_t n8,
                                                     int has_carry, int16_t carry, int apply_offset, int16_t* __restrict__ out,
                                                     unsigned long long* __restrict__ hist, int16_t* __restrict__ edge) {
    __shared__ unsigned hraw[HIST ? HL_WORDS : 1];
    HistLds& hl = *(HistLds*)hraw;
    if (HIST) hist_clear(hl);
    const int centre = apply_offset ? TZ_OFFSET : 0;
    HistAcc acc;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint4* in8 = (const uint4*)(in + 3 * head);   // 16-byte aligned when n8 > 0 (tzk_spatial_delta_gray)
    uint4* out8 = (uint4*)(out + head);
    const unsigned short* inu = (const unsigned short*)in;
    for (size_t i = t0; i < n8; i += stride) {
        const uint4 a = in8[3 * i], b = in8[3 * i + 1], c = in8[3 * i + 2];
        // elements 0, 3, 6, .. 21 of the 24: the low half of dwords 0, 3, 6, 9 and the high half of dwords 1, 4, 7, 10
        const uint4 v = make_uint4((a.x & 0xFFFFu) | (a.y & 0xFFFF0000u), (a.w & 0xFFFFu) | (b.x & 0xFFFF0000u),
                                   (b.z & 0xFFFFu) | (b.w & 0xFFFF0000u), (c.y & 0xFFFFu) | (c.z & 0xFFFF0000u));
        const size_t p0 = head + 8 * i;   // the lane's first pixel
        // the channel-0 element in front; without one (start of the stream, no carry) sd[0] = x[0], i.e. "prev" = 2 x[0]
        const unsigned prev = p0 ? (unsigned)inu[3 * (p0 - 1)] : (has_carry ? (unsigned)(unsigned short)carry : ((v.x << 1) & 0xFFFFu));
        unsigned Y[4];
        sdelta8(v, prev, apply_offset != 0, Y);
        out8[i] = make_uint4(Y[0], Y[1], Y[2], Y[3]);
        if (HIST) hist_add8(hl, acc, Y, centre);
    }
    // the pixels in front of and behind the vector groups
    const size_t v_end = head + 8 * n8, nscalar = head + (npix - v_end);
    for (size_t j = t0; j < nscalar; j += stride)
        sdelta_gray1(in, j < head ? j : v_end + (j - head), has_carry, carry, apply_offset, out, HIST ? &hl : nullptr);
    if (edge && t0 == 0) {
        edge[0] = in[0];
        edge[1] = in[3 * (npix - 1)];
    }
    if (HIST) hist_flush(hl, acc, centre, hist);
}

// ------------------------------------------------- spatial delta at the channel stride (tz_set_delta_stride(1))
// Not in the reference: out[i] = in[i-3] - in[i] (int16 wrap) over the flattened (frame, y, x, 3) stack, out[i] = in[i] (or
// carry[i] - in[i]) for i < 3 -- the neighbour of a sample is the SAME channel of the pixel in front, not another channel of
// its own pixel (tezip_amd/sdelta.py).  Offset and histogram as k_sdelta.  A lane takes 8 elements (16 B); the elements in
// front of them come from one more 8-byte load (the four in front, of which three are used; same or neighbouring cache line).
// vec = 0 (a buffer off the 16-byte grid) and the n % 8 elements behind the vectors go one by one.
__device__ __forceinline__ void sdelta_s3_1(const int16_t* __restrict__ in, size_t i, int has_carry, short c0, short c1, short c2,
                                            int apply_offset, int16_t* __restrict__ out, HistLds* hl) {
    const short cur = in[i];
    const short front = i >= 3 ? in[i - 3] : (i == 0 ? c0 : (i == 1 ? c1 : c2));
    const short sd = (i >= 3 || has_carry) ? (short)(front - cur) : cur;
    const short y = apply_offset ? (short)(TZ_OFFSET - sd) : sd;
    out[i] = y;
    if (hl && y >= 0 && y < TZ_NBINS) atomicAdd(&hl->w[HL_FULL + y], 1u);
}

template <bool HIST>
__global__ __launch_bounds__(HIST ? HB_THREADS : 256) void k_sdelta_s3(const int16_t* __restrict__ in, size_t n, size_t n8, int has_carry,
                                                   short c0, short c1, short c2, int apply_offset, int16_t* __restrict__ out,
                                                   unsigned long long* __restrict__ hist) {
    __shared__ unsigned hraw[HIST ? HL_WORDS : 1];
    HistLds& hl = *(HistLds*)hraw;
    if (HIST) hist_clear(hl);
    const int centre = apply_offset ? TZ_OFFSET : 0;
    HistAcc acc;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint4* in8 = (const uint4*)in;   // 16-byte aligned when n8 > 0 (tzk_spatial_delta_s3)
    uint4* out8 = (uint4*)out;
    for (size_t i = t0; i < n8; i += stride) {
        const uint4 v = in8[i];
        // w = (e[-4], e[-3]), (e[-2], e[-1]): the elements in front of the lane's eight.  At the start of the stream they are
        // the carry, or -- out[k] = x[k] for k < 3 -- "2 x[k]"
        uint2 w;
        if (i) w = *(const uint2*)(in + 8 * i - 4);
        else if (has_carry) w = make_uint2((unsigned)(unsigned short)c0 << 16, (unsigned)(unsigned short)c1 | ((unsigned)(unsigned short)c2 << 16));
        else w = make_uint2(v.x << 17, ((v.x >> 15) & 0xFFFEu) | (v.y << 17));
        // P = the eight elements three places in front, two per dword
        const unsigned P0 = __builtin_amdgcn_alignbit(w.y, w.x, 16), P1 = __builtin_amdgcn_alignbit(v.x, w.y, 16),
                       P2 = __builtin_amdgcn_alignbit(v.y, v.x, 16), P3 = __builtin_amdgcn_alignbit(v.z, v.y, 16);
        unsigned Y[4] = {pk_sub(P0, v.x), pk_sub(P1, v.y), pk_sub(P2, v.z), pk_sub(P3, v.w)};
        if (apply_offset) {
            const unsigned C = ((unsigned)TZ_OFFSET << 16) | (unsigned)TZ_OFFSET;
#pragma unroll
            for (int j = 0; j < 4; ++j) Y[j] = pk_sub(C, Y[j]);
        }
        out8[i] = make_uint4(Y[0], Y[1], Y[2], Y[3]);
        if (HIST) hist_add8(hl, acc, Y, centre);
    }
    for (size_t j = 8 * n8 + t0; j < n; j += stride) sdelta_s3_1(in, j, has_carry, c0, c1, c2, apply_offset, out, HIST ? &hl : nullptr);
    if (HIST) hist_flush(hl, acc, centre, hist);
}

// ------------------------------------------------- 2-D spatial delta of the payload (TZ-SD2, tz_set_delta_plane(1))
// Not in the reference (tezip_amd/sdelta.py encode_plane).  Per frame and channel of the (frame, y, x, C) stack, every
// neighbour outside the frame taken as 0:
//     sd = wrap9(q[y, x-1] + q[y-1, x] - q[y-1, x-1] - q[y, x]),   wrap9(v) = ((v + 256) mod 512) - 256
// then 1600 - sd and the histogram as k_sdelta.  Elementwise: the element, the C elements in front, and the same two places in
// the row above; nothing is read across a frame boundary.  Vector route (n8 > 0: CIN == C, a row is whole 16-byte groups on
// 16-byte boundaries): a lane takes 8 elements of a row and the 8 above them as 16-byte loads, the elements in front of either
// from one more 8-byte load, and forms (left - cur) - (upleft - up) in packed int16 arithmetic.  Any other W, alignment or
// channel count goes one element at a time; CIN = 3 with C = 1 reads channel 0 of the interleaved three-channel stack.
__device__ __forceinline__ unsigned pk_wrap9(unsigned x) {   // two int16 lanes
    return pk_sub(pk_sub(x, 0xFF00FF00u) & 0x01FF01FFu, 0x01000100u);
}

// P = the eight elements C places in front of the group v at p; no front (the row starts here): zeros
template <int C>
__device__ __forceinline__ void plane_front8(const int16_t* __restrict__ p, bool has_front, const uint4 v, unsigned* P) {
    const uint2 w = has_front ? *(const uint2*)(p - 4) : make_uint2(0u, 0u);   // (e[-4], e[-3]), (e[-2], e[-1])
    if (C == 3) {
        P[0] = __builtin_amdgcn_alignbit(w.y, w.x, 16);
        P[1] = __builtin_amdgcn_alignbit(v.x, w.y, 16);
        P[2] = __builtin_amdgcn_alignbit(v.y, v.x, 16);
        P[3] = __builtin_amdgcn_alignbit(v.z, v.y, 16);
    } else {
        P[0] = __builtin_amdgcn_alignbit(v.x, w.y, 16);
        P[1] = __builtin_amdgcn_alignbit(v.y, v.x, 16);
        P[2] = __builtin_amdgcn_alignbit(v.z, v.y, 16);
        P[3] = __builtin_amdgcn_alignbit(v.w, v.z, 16);
    }
}

template <bool HIST, int CIN, int C>
__global__ __launch_bounds__(HIST ? HB_THREADS : 256) void k_sdelta_plane(const int16_t* __restrict__ in, size_t n, size_t n8, int H, int W,
                                                      int apply_offset, int16_t* __restrict__ out,
                                                      unsigned long long* __restrict__ hist) {
    __shared__ unsigned hraw[HIST ? HL_WORDS : 1];
    HistLds& hl = *(HistLds*)hraw;
    if (HIST) hist_clear(hl);
    const int centre = apply_offset ? TZ_OFFSET : 0;
    HistAcc acc;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (CIN == C && n8) {
        const size_t rw = (size_t)W * C, rw8 = rw / 8;   // elements, groups of a row
        for (size_t i = t0; i < n8; i += stride) {
            const size_t row = i / rw8;
            const bool front = i != row * rw8, top = row % (size_t)H == 0;
            const int16_t* p = in + 8 * i;
            const uint4 v = *(const uint4*)p;
            uint4 u = make_uint4(0u, 0u, 0u, 0u);
            unsigned Pc[4], Pu[4] = {0u, 0u, 0u, 0u};
            plane_front8<C>(p, front, v, Pc);
            if (!top) {
                u = *(const uint4*)(p - rw);
                plane_front8<C>(p - rw, front, u, Pu);
            }
            unsigned Y[4] = {pk_wrap9(pk_sub(pk_sub(Pc[0], v.x), pk_sub(Pu[0], u.x))), pk_wrap9(pk_sub(pk_sub(Pc[1], v.y), pk_sub(Pu[1], u.y))),
                             pk_wrap9(pk_sub(pk_sub(Pc[2], v.z), pk_sub(Pu[2], u.z))), pk_wrap9(pk_sub(pk_sub(Pc[3], v.w), pk_sub(Pu[3], u.w)))};
            if (apply_offset) {
                const unsigned K = ((unsigned)TZ_OFFSET << 16) | (unsigned)TZ_OFFSET;
#pragma unroll
                for (int j = 0; j < 4; ++j) Y[j] = pk_sub(K, Y[j]);
            }
            *(uint4*)(out + 8 * i) = make_uint4(Y[0], Y[1], Y[2], Y[3]);
            if (HIST) hist_add8(hl, acc, Y, centre);
        }
    } else {
        for (size_t j = t0; j < n; j += stride) {
            const size_t pix = j / C, row = pix / (size_t)W;
            const int c = (int)(j - pix * C);
            const bool left = pix != row * (size_t)W, top = row % (size_t)H == 0;
            const int16_t* p = in + pix * CIN + c;
            const int cur = p[0], l = left ? (int)p[-CIN] : 0, up = top ? 0 : (int)p[-(ptrdiff_t)W * CIN],
                      ul = (left && !top) ? (int)p[-((ptrdiff_t)W + 1) * CIN] : 0;
            const int sd = ((l + up - ul - cur + 256) & 511) - 256;
            const short y = (short)(apply_offset ? TZ_OFFSET - sd : sd);
            out[j] = y;
            if (HIST && y >= 0 && y < TZ_NBINS) atomicAdd(&hl.w[HL_FULL + y], 1u);
        }
    }
    if (HIST) hist_flush(hl, acc, centre, hist);
}

// in: nframes x H x W x cin elements (cin == C, or 3 with C = 1: channel 0 is taken) -> nframes x H x W x C at out; the counts
// are ADDED to d_hist (may be NULL).  Buffers at any 2-byte alignment.
int tzk_sdelta_plane(tz_ctx* ctx, const int16_t* in, int cin, int nframes, int H, int W, int C, int apply_offset, int16_t* out,
                     unsigned long long* d_hist) {
    if (nframes < 0 || H < 1 || W < 1 || (C != 1 && C != 3) || (cin != C && cin != 3))
        return tz_fail(ctx, TZ_ERR_INVALID, "spatial_delta_plane: %d frames of %d x %d with %d of %d channels", nframes, H, W, C, cin);
    const size_t n = (size_t)nframes * H * W * C;
    if (n == 0) return TZ_OK;
    const uintptr_t both = (uintptr_t)in | (uintptr_t)out;
    if (both & 1) return tz_fail(ctx, TZ_ERR_INVALID, "spatial_delta_plane buffers must be 2-byte aligned");
    const size_t n8 = (cin == C && ((size_t)W * C) % 8 == 0 && (both & 15) == 0) ? n / 8 : 0;
    const size_t items = n8 ? n8 : n;
    tz_prof_scope ps(ctx, TZP_SDELTA);
    const dim3 grid(d_hist ? std::min(HB_GRID, grid_for(items, HB_THREADS)) : grid_for(items, 256)), block(d_hist ? HB_THREADS : 256);
#define TZ_PLANE_LAUNCH(CI, CO)                                                                                                  \
    do {                                                                                                                         \
        if (d_hist) hipLaunchKernelGGL((k_sdelta_plane<true, CI, CO>), grid, block, 0, ctx->stream, in, n, n8, H, W, apply_offset, out, d_hist);  \
        else hipLaunchKernelGGL((k_sdelta_plane<false, CI, CO>), grid, block, 0, ctx->stream, in, n, n8, H, W, apply_offset, out, d_hist);        \
    } while (0)
    if (C == 3) TZ_PLANE_LAUNCH(3, 3);
    else if (cin == 1) TZ_PLANE_LAUNCH(1, 1);
    else TZ_PLANE_LAUNCH(3, 1);
#undef TZ_PLANE_LAUNCH
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// The spatial delta of every layout (tz_internal.h): k_sdelta (flat), k_sdelta_gray or k_sdelta_s3, each with its own alignment
// rule and its own cut into vector groups and single elements; one grid rule over the resulting work items.  The plane layout
// goes to tzk_sdelta_plane above.
int tzk_spatial_delta(tz_ctx* ctx, tz_layout layout, const int16_t* in, size_t n, const int16_t* carry, int apply_offset, int16_t* out,
                      unsigned long long* d_hist, int16_t* d_edge) {
    if (n == 0) return TZ_OK;
    if (layout.plane_h) {   // TZ-SD2: whole frames, no carry; a one-channel payload reads channel 0 of the three, as the gray front
        const size_t fe = tz_frame_elems(layout, layout.plane_h, layout.plane_w);
        if (carry || n % fe) return tz_fail(ctx, TZ_ERR_INVALID, "spatial_delta_plane takes whole frames and no carry");
        return tzk_sdelta_plane(ctx, in, 3, (int)(n / fe), layout.plane_h, layout.plane_w, layout.channels, apply_offset, out, d_hist);
    }
    const bool gray = layout.channels == 1, s3 = layout.stride == 3;
    const uintptr_t both = (uintptr_t)in | (uintptr_t)out;
    if (gray && (both & 1)) return tz_fail(ctx, TZ_ERR_INVALID, "spatial_delta_gray buffers must be 2-byte aligned");
    if (s3 && (both & 1)) return tz_fail(ctx, TZ_ERR_INVALID, "spatial_delta_s3 buffers must be 2-byte aligned");
    if (!gray && !s3 && (both & 15)) return tz_fail(ctx, TZ_ERR_INVALID, "spatial_delta buffers must be 16-byte aligned");
    size_t head = 0, n8 = 0, items = n / 8 + 1;   // flat: the kernel cuts the stack itself
    if (gray) {
        // the first pixel h at which both in + 3 h and out + h sit on a 16-byte boundary: 6 h = -in (mod 16) has one solution
        // in [0, 8) and so has 2 h = -out; when the two differ nothing can be vectorised
        head = n;
        for (size_t h = 0; h < 8 && h < n; ++h)
            if ((((uintptr_t)in + 6 * h) & 15) == 0 && (((uintptr_t)out + 2 * h) & 15) == 0) {
                head = h;
                break;
            }
        n8 = (n - head) / 8;
        if (n8 == 0) head = n;
        items = std::max(n8, head + (n - head - 8 * n8));
    } else if (s3) {
        n8 = (both & 15) == 0 ? n / 8 : 0;
        items = std::max(n8, n - 8 * n8);
    }
    const int has_carry = carry != nullptr;
    const short c0 = carry ? carry[0] : 0, c1 = carry && s3 ? carry[1] : 0, c2 = carry && s3 ? carry[2] : 0;
    tz_prof_scope ps(ctx, TZP_SDELTA);
    const dim3 grid(d_hist ? std::min(HB_GRID, grid_for(items, HB_THREADS)) : grid_for(items, 256)), block(d_hist ? HB_THREADS : 256);
#define TZ_SDELTA_LAUNCH(K, ...)                                                                   \
    do {                                                                                           \
        if (d_hist) hipLaunchKernelGGL(K<true>, grid, block, 0, ctx->stream, __VA_ARGS__);         \
        else hipLaunchKernelGGL(K<false>, grid, block, 0, ctx->stream, __VA_ARGS__);               \
    } while (0)
    // (flat first: the kernels' place in the code object follows their first mention)
    if (!gray && !s3) TZ_SDELTA_LAUNCH(k_sdelta, in, n, has_carry, c0, apply_offset, out, d_hist);
    else if (gray) TZ_SDELTA_LAUNCH(k_sdelta_gray, in, n, head, n8, has_carry, c0, apply_offset, out, d_hist, d_edge);
    else TZ_SDELTA_LAUNCH(k_sdelta_s3, in, n, n8, has_carry, c0, c1, c2, apply_offset, out, d_hist);
#undef TZ_SDELTA_LAUNCH
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// --------------------------------------------------------------------- lattice quantiser (TZ-QL1)
// Not in the reference (include/tezip_hip.h: tz_set_quantiser; slow statement: tezip_amd/lattice.py).  For a delta d and the
// tolerance e of its chain -- the float64 the greedy walk above forms, from the same launches (k_q_minmax / k_q_bound,
// k_q_frame_bound's rule) --
//     E = min(255, floor(e)),  s = 2E + 1,  q = clamp(sign(d) * ((|d| + E) div s) * s, -255, 255),  E == 0: q = d.
// A pure function of one delta and one tolerance: no walk, no stitch, no fallback.  Per chain the host side of the launch is
// LatP {E, M}, M = floor(2^32 / s) + 1: (a * M) >> 32 == a div s exactly while a * s < 2^32, and a = |d| + E <= 33023,
// s <= 511 for every int16 d.  pwrel has a tolerance per element (orig * b0 in fp64): E is formed in the lane and the division
// is the compiler's; LatP.E then only says whether the frame is quantised at all.
struct LatP {
    int E;        // 0: the chain is left as it is (a skipped frame, or e < 1)
    unsigned M;
};

__global__ void k_lat_params(const double* __restrict__ Echain, const uint8_t* __restrict__ skip, int nframes, int pw,
                             LatP* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nframes * 3) return;
    LatP p{0, 0u};
    if (!skip[i / 3]) {
        if (pw) {
            p.E = 1;
        } else {
            const double e = Echain[i];                          // >= 0 (a NaN, 0 * inf, counts as 0)
            const int E = e >= 255.0 ? 255 : (e >= 1.0 ? (int)e : 0);
            p.E = E;
            p.M = E ? (unsigned)(0x100000000ull / (unsigned)(2 * E + 1)) + 1u : 0u;
        }
    }
    out[i] = p;
}

// PW: the tolerance source (Q_TOL_*).  o: the original sample under Q_TOL_ORIG, the map byte M[pixel] under Q_TOL_MAP (TZ-BM1:
// e = M[p] is an integer in [0, 255], so E = e)
template <int PW>
__device__ __forceinline__ int lat_apply(int d, unsigned o, const LatP p, double b0) {
    const unsigned ad = (unsigned)(d < 0 ? -d : d);
    unsigned E, k;
    if (PW == Q_TOL_MAP) {
        E = p.E ? o : 0u;
        k = (ad + E) / (2u * E + 1u);
    } else if (PW) {
        const double e = o ? (double)o * b0 : 0.0;               // (0 * inf is no tolerance)
        E = e >= 255.0 ? 255u : (e >= 1.0 ? (unsigned)e : 0u);
        if (!p.E) E = 0u;
        k = (ad + E) / (2u * E + 1u);
    } else {
        E = (unsigned)p.E;
        k = __umulhi(ad + E, p.M);
    }
    const int m = (int)min(k * (2u * E + 1u), 255u);
    return E ? (d < 0 ? -m : m) : d;
}

// the three chains of frame f, rotated so that r[j] belongs to the element j places behind one of channel c0
__device__ __forceinline__ void lat_chains(const LatP* __restrict__ P, size_t f, unsigned c0, LatP r[3]) {
    const LatP a = P[3 * f], b = P[3 * f + 1], c = P[3 * f + 2];
    r[0] = c0 == 0 ? a : (c0 == 1 ? b : c);
    r[1] = c0 == 0 ? b : (c0 == 1 ? c : a);
    r[2] = c0 == 0 ? c : (c0 == 1 ? a : b);
}

// Stand-alone / unfused form: an int16 delta stack in place (tz_lattice_bound, and tz_encode where the fused front below does
// not apply).  diff need only be 2-byte aligned: `head` elements in front of the first 16-byte boundary and the n - head - 8 n8
// behind the vector groups go one by one; a group of 8 that straddles a frame boundary takes its chains element by element.
// Q_TOL_MAP: `orig` is the bound map, one byte per pixel of a frame (the deltas are there already: no original is read)
template <int PW>
__device__ __forceinline__ void lattice1(int16_t* __restrict__ diff, const uint8_t* __restrict__ orig, const LatP* __restrict__ P,
                                         double b0, size_t fe, size_t e) {
    const size_t f = e / fe;
    const unsigned c = (unsigned)((e - f * fe) % 3);
    diff[e] = (int16_t)lat_apply<PW>(diff[e], PW == Q_TOL_MAP ? orig[(e - f * fe) / 3] : (PW ? orig[e] : 0u), P[3 * f + c], b0);
}

template <int PW>
__global__ __launch_bounds__(256) void k_lattice(int16_t* __restrict__ diff, const uint8_t* __restrict__ orig, const LatP* __restrict__ P,
                                                 double b0, size_t n, size_t fe, size_t head, size_t n8) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint4* v8 = (uint4*)(diff + head);   // 16-byte aligned when n8 > 0 (tzk_lattice)
    for (size_t i = t0; i < n8; i += stride) {
        const size_t e0 = head + 8 * i, f = e0 / fe, r0 = e0 - f * fe;
        if (r0 + 8 > fe) {   // the group straddles a frame boundary
            for (int k = 0; k < 8; ++k) lattice1<PW>(diff, orig, P, b0, fe, e0 + k);
            continue;
        }
        LatP r[3];
        lat_chains(P, f, (unsigned)(r0 % 3), r);
        const uint4 v = v8[i];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        unsigned q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int lo = lat_apply<PW>((int)(short)(w[j] & 0xFFFFu), PW == Q_TOL_MAP ? orig[(r0 + 2 * j) / 3] : (PW ? orig[e0 + 2 * j] : 0u),
                                         r[(2 * j) % 3], b0);
            const int hi = lat_apply<PW>((int)w[j] >> 16, PW == Q_TOL_MAP ? orig[(r0 + 2 * j + 1) / 3] : (PW ? orig[e0 + 2 * j + 1] : 0u),
                                         r[(2 * j + 1) % 3], b0);
            q[j] = ((unsigned)lo & 0xFFFFu) | ((unsigned)hi << 16);
        }
        v8[i] = make_uint4(q[0], q[1], q[2], q[3]);
    }
    const size_t v_end = head + 8 * n8, nscalar = head + (n - v_end);
    for (size_t j = t0; j < nscalar; j += stride) lattice1<PW>(diff, orig, P, b0, fe, j < head ? j : v_end + (j - head));
}

// what tzk_error_bound refuses, refused in its words
static int lattice_check(tz_ctx* ctx, int mode, double b0, double b1) {
    if (mode < 0 || mode > 3) return tz_fail(ctx, TZ_ERR_INVALID, "unknown error-bound mode %d", mode);
    if ((mode == TZ_MODE_PWREL || mode == TZ_MODE_REL) && b0 < 0.0)
        return tz_fail(ctx, TZ_ERR_INVALID, "%s bound must be >= 0 (the reference raises on a negative one)", mode == TZ_MODE_REL ? "rel" : "pwrel");
    if (mode == TZ_MODE_ABSREL && b1 < 0.0)
        return tz_fail(ctx, TZ_ERR_INVALID, "the rel bound of absrel must be >= 0 (the reference raises on a negative one)");
    if (std::isnan(b0) || (mode == TZ_MODE_ABSREL && std::isnan(b1)))
        return tz_fail(ctx, TZ_ERR_INVALID, "error bound is NaN (the reference raises on a NaN tolerance)");
    return TZ_OK;
}

bool tz_lattice_is_identity(int mode, double b0, double b1) {
    if (std::isnan(b0) || (mode == TZ_MODE_ABSREL && std::isnan(b1))) return false;   // (the general path and its refusal)
    double worst;
    if (mode == TZ_MODE_ABS) worst = fabs(b0);
    else if (mode == TZ_MODE_REL || mode == TZ_MODE_PWREL) worst = 255.0 * b0;        // (rounding is monotone: range * b0 <= 255 b0)
    else if (mode == TZ_MODE_ABSREL) worst = std::min(fabs(b0), 255.0 * b1);
    else return false;
    return worst >= 0.0 && worst < 1.0;
}

// LatP per chain on the device: the tolerances as quant_run's first stage forms them (the same kernels for rel / absrel), then
// k_lat_params.  h_fb (may be NULL): one abs tolerance per frame in place of (mode, b0, b1).
static int lattice_params(tz_ctx* ctx, const uint8_t* orig, const uint8_t* h_skip, int nframes, int HW, int mode, double b0, double b1,
                          const double* h_fb, const LatP** out) {
    void *d_skip, *d_E, *d_lp;
    TZ_TRY(tz_pool_alloc(ctx, nframes, &d_skip));
    TZ_TRY(tz_pool_alloc(ctx, sizeof(double) * 3 * nframes, &d_E));
    TZ_TRY(tz_pool_alloc(ctx, sizeof(LatP) * 3 * nframes, &d_lp));
    TZ_TRY(tz_upload(ctx, d_skip, h_skip, nframes));
    tz_prof_scope ps(ctx, TZP_QUANT);
    if (!h_fb && (mode == TZ_MODE_REL || mode == TZ_MODE_ABSREL)) {
        void* d_mm;
        TZ_TRY(tz_pool_alloc(ctx, sizeof(int) * 6 * nframes, &d_mm));
        QParams qp{mode, b0, b1};
        hipLaunchKernelGGL(k_q_mm_init, dim3((6 * nframes + 255) / 256), dim3(256), 0, ctx->stream, (int*)d_mm, 6 * nframes);
        hipLaunchKernelGGL(k_q_minmax, dim3(QBB, nframes), dim3(256), 0, ctx->stream, orig, (const uint8_t*)d_skip, HW, (int*)d_mm);
        hipLaunchKernelGGL(k_q_bound, dim3((3 * nframes + 63) / 64), dim3(64), 0, ctx->stream, (const int*)d_mm, (const uint8_t*)d_skip, qp,
                           nframes, (double*)d_E);
    } else {
        std::vector<double> e(3 * (size_t)nframes);
        for (int i = 0; i < 3 * nframes; ++i) e[i] = h_fb ? h_fb[i / 3] : fabs(b0);   // (pwrel: not read)
        TZ_TRY(tz_upload(ctx, d_E, e.data(), sizeof(double) * e.size()));
    }
    hipLaunchKernelGGL(k_lat_params, dim3((3 * nframes + 63) / 64), dim3(64), 0, ctx->stream, (const double*)d_E, (const uint8_t*)d_skip,
                       nframes, !h_fb && mode == TZ_MODE_PWREL ? 1 : 0, (LatP*)d_lp);
    TZ_HIP(ctx, hipGetLastError());
    *out = (const LatP*)d_lp;
    return TZ_OK;
}

// d_map (may be NULL; device, H * W bytes): the bound map of TZ-BM1 in place of (mode, b0, b1) and h_bounds; orig is then not read
int tzk_lattice(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* h_skip, int nframes, int H, int W, int mode, double b0,
                double b1, const double* h_bounds, const uint8_t* d_map) {
    if (d_map) {
        h_bounds = nullptr;
        mode = TZ_MODE_PWREL;   // (lattice_params: LatP.E only says whether the frame is quantised)
        b0 = 1.0;
        b1 = 0.0;
    } else if (!h_bounds) {
        TZ_TRY(lattice_check(ctx, mode, b0, b1));
        if (b0 == 0.0 || (mode == TZ_MODE_ABSREL && b1 == 0.0)) return TZ_OK;   // no tolerance: nothing changes
        if (tz_lattice_is_identity(mode, b0, b1)) return TZ_OK;                 // every chain has E == 0
    }
    if (nframes <= 0 || H <= 0 || W <= 0) return TZ_OK;
    if (h_bounds) {
        bool any = false;
        for (int f = 0; f < nframes; ++f) any = any || (h_bounds[f] >= 1.0 && !h_skip[f]);
        if (!any) return TZ_OK;   // every frame is left as it is
    }
    if ((uintptr_t)diff & 1) return tz_fail(ctx, TZ_ERR_INVALID, "lattice_bound: the delta stack must be 2-byte aligned");
    const size_t fe = (size_t)H * W * 3, n = fe * nframes;
    const LatP* d_lp;
    TZ_TRY(lattice_params(ctx, orig, h_skip, nframes, H * W, mode, b0, b1, h_bounds, &d_lp));
    size_t head = std::min(n, (size_t)((16 - ((uintptr_t)diff & 15)) & 15) / 2), n8 = (n - head) / 8;
    if (n8 == 0) head = n;
    const bool pw = !h_bounds && mode == TZ_MODE_PWREL;
    const size_t items = std::max(n8, head + (n - head - 8 * n8));
    tz_prof_scope ps(ctx, TZP_QUANT);
    // (true = Q_TOL_ORIG, false = Q_TOL_CHAIN; under Q_TOL_MAP the map goes in the orig slot)
    if (d_map) hipLaunchKernelGGL(k_lattice<Q_TOL_MAP>, dim3(grid_for(items, 256)), dim3(256), 0, ctx->stream, diff, d_map, d_lp, b0, n, fe, head, n8);
    else if (pw) hipLaunchKernelGGL(k_lattice<true>, dim3(grid_for(items, 256)), dim3(256), 0, ctx->stream, diff, orig, d_lp, b0, n, fe, head, n8);
    else hipLaunchKernelGGL(k_lattice<false>, dim3(grid_for(items, 256)), dim3(256), 0, ctx->stream, diff, orig, d_lp, b0, n, fe, head, n8);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// The fused lattice front: k_delta_sd_fused with TZ-QL1 between the delta and the spatial delta, in every payload layout.  A lane
// makes 8 symbols: flat and channel stride from 8 consecutive elements (two 16-byte loads of pred, one 8-byte load of orig),
// gray from channel 0 of 8 pixels (six and three loads; channels 1 and 2 share their cache lines and are not looked at).  The
// elements in front of a lane's first -- one, or three at the channel stride -- are made again from pred / orig and quantised
// with THEIR chain's tolerance (the last frame's at a frame start).  Histogram: HistLds / HistAcc above.
static constexpr int LAT_FLAT = 0, LAT_GRAY = 1, LAT_S3 = 2;

// Q_TOL_MAP: the tolerance of an element is the byte of its pixel in the map (H x W, shared by all frames and channels: cached),
// which travels as the eight bytes of b0 (lat_tol_arg on the host): that source reads no b0.
__device__ __forceinline__ const uint8_t* lat_tol_map(double b0) { return (const uint8_t*)(uintptr_t)__double_as_longlong(b0); }
static double lat_tol_arg(const uint8_t* d_map) {
    double v;
    static_assert(sizeof(v) == sizeof(d_map), "a device pointer fills the argument's eight bytes");
    memcpy(&v, &d_map, sizeof(v));
    return v;
}

template <int LAY, bool HIST, int PW>
__global__ __launch_bounds__(HIST ? HB_THREADS : 256) void k_lattice_sd(const float4* __restrict__ pred, const uint2* __restrict__ orig,
                                                                        const uint8_t* __restrict__ zero_mask, const LatP* __restrict__ P,
                                                                        double b0, size_t n8, unsigned frame_items, int apply_offset,
                                                                        uint4* __restrict__ out, unsigned long long* __restrict__ hist,
                                                                        int16_t* __restrict__ edge) {
    const uint8_t* const tol = PW == Q_TOL_MAP ? lat_tol_map(b0) : nullptr;
    __shared__ unsigned hraw[HIST ? HL_WORDS : 1];
    HistLds& hl = *(HistLds*)hraw;
    constexpr bool do_hist = HIST;
    if (do_hist) hist_clear(hl);
    const int centre = apply_offset ? TZ_OFFSET : 0;
    HistAcc acc;
    const float* predf = (const float*)pred;
    const uint8_t* origb = (const uint8_t*)orig;
    constexpr int ES = LAY == LAT_GRAY ? 3 : 1;        // input elements per symbol
    constexpr int NPREV = LAY == LAT_S3 ? 3 : 1;       // elements in front of the lane's first that its symbols need
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const size_t f = i / frame_items;
        const bool fstart = i - f * frame_items == 0;
        const bool zero = zero_mask[f] != 0;
        int d[8];
        unsigned ob[8];
        if (LAY == LAT_GRAY) {
            const float4 p0 = pred[6 * i], p1 = pred[6 * i + 1], p2 = pred[6 * i + 2], p3 = pred[6 * i + 3], p4 = pred[6 * i + 4],
                         p5 = pred[6 * i + 5];
            const uint2 o0 = orig[3 * i], o1 = orig[3 * i + 1], o2 = orig[3 * i + 2];
            const float pv[8] = {p0.x, p0.w, p1.z, p2.y, p3.x, p3.w, p4.z, p5.y};     // elements 0, 3, .. 21 of the 24
            const unsigned w[6] = {o0.x, o0.y, o1.x, o1.y, o2.x, o2.y};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                ob[k] = (w[(3 * k) >> 2] >> (8 * ((3 * k) & 3))) & 0xffu;
                d[k] = (int)(pv[k] * 255.0f) - (int)ob[k];
            }
        } else {
            const float4 p0 = pred[2 * i], p1 = pred[2 * i + 1];
            const uint2 o = orig[i];
            const float pv[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                ob[k] = ((k < 4 ? o.x : o.y) >> (8 * (k & 3))) & 0xffu;
                d[k] = (int)(pv[k] * 255.0f) - (int)ob[k];
            }
        }
        LatP r[3];
        if (LAY == LAT_GRAY) r[0] = r[1] = r[2] = P[3 * f];
        else lat_chains(P, f, (unsigned)(((i % 3) * 2) % 3), r);   // (a frame holds a multiple of 3 elements: channel of 8 i = 8 i mod 3)
        int q[8];
        if (PW == Q_TOL_MAP) {   // the lane's 8 symbols start at element 8 ES (i - f frame_items) of frame f
            const unsigned fi = (unsigned)(i - f * frame_items) * 8u;
#pragma unroll
            for (int k = 0; k < 8; ++k) ob[k] = tol[LAY == LAT_GRAY ? fi + k : (fi + k) / 3u];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) q[k] = lat_apply<PW>(zero ? 0 : d[k], ob[k], r[LAY == LAT_GRAY ? 0 : k % 3], b0);
        int pq[3] = {0, 0, 0};
        if (i) {
            const size_t pf = fstart ? f - 1 : f;
            const bool pzero = zero_mask[pf] != 0;
#pragma unroll
            for (int j = 0; j < NPREV; ++j) {
                const size_t e = (size_t)8 * ES * i - (size_t)ES * (NPREV - j);
                const int c = LAY == LAT_GRAY ? 0 : (LAY == LAT_FLAT ? 2 : j);      // at a frame start the elements in front are ..., 1, 2
                const LatP lp = fstart ? P[3 * pf + c] : r[c];
                const unsigned o = origb[e];
                // (the pixel of e within ITS frame pf: a frame holds 8 ES frame_items elements, three per pixel)
                const unsigned t = PW == Q_TOL_MAP ? tol[(e - pf * ((size_t)8 * ES * frame_items)) / 3] : o;
                pq[j] = lat_apply<PW>(pzero ? 0 : (int)(predf[e] * 255.0f) - (int)o, t, lp, b0);
            }
        }
        unsigned V[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) V[j] = ((unsigned)q[2 * j] & 0xFFFFu) | ((unsigned)q[2 * j + 1] << 16);
        unsigned Y[4];
        if (LAY == LAT_S3) {
            // w = (e[-4], e[-3]), (e[-2], e[-1]); at the stream start out[k] = x[k] for k < 3, i.e. the elements in front are "2 x[k]"
            const uint2 w = i ? make_uint2((unsigned)pq[0] << 16, ((unsigned)pq[1] & 0xFFFFu) | ((unsigned)pq[2] << 16))
                              : make_uint2(V[0] << 17, ((V[0] >> 15) & 0xFFFEu) | (V[1] << 17));
            const unsigned P0 = __builtin_amdgcn_alignbit(w.y, w.x, 16), P1 = __builtin_amdgcn_alignbit(V[0], w.y, 16),
                           P2 = __builtin_amdgcn_alignbit(V[1], V[0], 16), P3 = __builtin_amdgcn_alignbit(V[2], V[1], 16);
            Y[0] = pk_sub(P0, V[0]);
            Y[1] = pk_sub(P1, V[1]);
            Y[2] = pk_sub(P2, V[2]);
            Y[3] = pk_sub(P3, V[3]);
            if (apply_offset) {
                const unsigned C = ((unsigned)TZ_OFFSET << 16) | (unsigned)TZ_OFFSET;
#pragma unroll
                for (int j = 0; j < 4; ++j) Y[j] = pk_sub(C, Y[j]);
            }
        } else {
            const unsigned pv = i ? ((unsigned)pq[0] & 0xFFFFu) : ((V[0] << 1) & 0xFFFFu);   // stream start: sd[0] = x[0]
            sdelta8(make_uint4(V[0], V[1], V[2], V[3]), pv, apply_offset != 0, Y);
        }
        out[i] = make_uint4(Y[0], Y[1], Y[2], Y[3]);
        if (do_hist) hist_add8(hl, acc, Y, centre);
        if (LAY != LAT_S3 && edge) {   // first / last element of the quantised stack (channel 0's under the gray layout)
            if (i == 0) edge[0] = (int16_t)q[0];
            if (i == n8 - 1) edge[1] = (int16_t)q[7];
        }
    }
    if (do_hist) hist_flush(hl, acc, centre, hist);
}

int tzk_lattice_sd_fused(tz_ctx* ctx, tz_layout layout, const float* pred, const uint8_t* orig, const uint8_t* d_zero_mask,
                         const uint8_t* h_skip, int nframes, int H, int W, int Hp, int Wp, int mode, double b0, double b1,
                         const double* h_bounds, int apply_offset, int16_t* sym, unsigned long long* d_hist, int16_t* d_edge, bool* done,
                         const uint8_t* d_map) {
    *done = false;
    if (d_map) {
        h_bounds = nullptr;
        mode = TZ_MODE_PWREL;   // (lattice_params: LatP.E only says whether the frame is quantised)
        b0 = 1.0;
        b1 = 0.0;
    }
    if (!h_bounds) TZ_TRY(lattice_check(ctx, mode, b0, b1));
    if (layout.plane_h) return TZ_OK;   // TZ-SD2 has no fused front
    const int lay = layout.channels == 1 ? LAT_GRAY : (layout.stride == 3 ? LAT_S3 : LAT_FLAT);
    const size_t fsym = tz_frame_elems(layout, H, W);   // symbols of a frame
    if (H != Hp || W != Wp || fsym % 8 || nframes <= 0) return TZ_OK;
    if (((((uintptr_t)pred | (uintptr_t)sym) & 15) | ((uintptr_t)orig & 7)) != 0) return TZ_OK;   // 16-byte pred / sym, 8-byte orig accesses
    const LatP* d_lp;
    TZ_TRY(lattice_params(ctx, orig, h_skip, nframes, H * W, mode, b0, b1, h_bounds, &d_lp));
    const size_t n8 = fsym * nframes / 8;
    const bool pw = !h_bounds && mode == TZ_MODE_PWREL;
    if (d_map) b0 = lat_tol_arg(d_map);
    tz_prof_scope ps(ctx, TZP_DELTA);
    const dim3 grid(d_hist ? std::min(HB_GRID, grid_for(n8, HB_THREADS)) : grid_for(n8, 256)), block(d_hist ? HB_THREADS : 256);
#define TZ_LAT_LAUNCH(L, HV, PWV)                                                                                                 \
    hipLaunchKernelGGL((k_lattice_sd<L, HV, PWV>), grid, block, 0, ctx->stream, (const float4*)pred, (const uint2*)orig, d_zero_mask, \
                       d_lp, b0, n8, (unsigned)(fsym / 8), apply_offset, (uint4*)sym, d_hist, d_edge)
#define TZ_LAT_LAYOUT(L)                            \
    do {                                            \
        if (d_hist && d_map) TZ_LAT_LAUNCH(L, true, Q_TOL_MAP);       \
        else if (d_map) TZ_LAT_LAUNCH(L, false, Q_TOL_MAP);           \
        else if (d_hist && pw) TZ_LAT_LAUNCH(L, true, Q_TOL_ORIG);    \
        else if (d_hist) TZ_LAT_LAUNCH(L, true, Q_TOL_CHAIN);         \
        else if (pw) TZ_LAT_LAUNCH(L, false, Q_TOL_ORIG);             \
        else TZ_LAT_LAUNCH(L, false, Q_TOL_CHAIN);                    \
    } while (0)
    if (lay == LAT_FLAT) TZ_LAT_LAYOUT(LAT_FLAT);
    else if (lay == LAT_GRAY) TZ_LAT_LAYOUT(LAT_GRAY);
    else TZ_LAT_LAYOUT(LAT_S3);
#undef TZ_LAT_LAYOUT
#undef TZ_LAT_LAUNCH
    TZ_HIP(ctx, hipGetLastError());
    *done = true;
    return TZ_OK;
}

// ----------------------------------------------------------------------- rank remap / unmap
// compress.py:84-90 and decompress.py:31-36 are T sequential `where` passes (O(N*T)); here
// one pass through a 2112-entry LUT held in LDS.  Values outside [0, 2112) pass through
// (then 1600 - v when post_offset, decompress.py:236).  The host builds the LUT so that it
// reproduces the sequential-pass semantics exactly.
__global__ __launch_bounds__(256) void k_lut(const int16_t* __restrict__ in, size_t n, const int16_t* __restrict__ lut,
                                             int post_offset, int16_t* __restrict__ out) {
    __shared__ int16_t sl[TZ_NBINS + 1];
    for (int k = threadIdx.x; k < TZ_NBINS + 1; k += 256) sl[k] = lut[k];
    __syncthreads();
    size_t n8 = n / 8;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    const short8* in8 = (const short8*)in;
    short8* out8 = (short8*)out;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        short8 v = in8[i], r;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int x = v[k];
            r[k] = (x >= 0 && x <= TZ_NBINS) ? sl[x] : (short)(post_offset ? TZ_OFFSET - x : x);
        }
        out8[i] = r;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
        size_t i = n8 * 8 + threadIdx.x;
        int x = in[i];
        out[i] = (x >= 0 && x <= TZ_NBINS) ? sl[x] : (int16_t)(post_offset ? TZ_OFFSET - x : x);
    }
}

int tzk_lut(tz_ctx* ctx, const int16_t* in, size_t n, const int16_t* h_lut2112, int post_offset, int16_t* out) {
    if (n == 0) return TZ_OK;
    if (((uintptr_t)in & 15) || ((uintptr_t)out & 15))
        return tz_fail(ctx, TZ_ERR_INVALID, "remap buffers must be 16-byte aligned");
    void* d_lut;
    TZ_TRY(tz_pool_alloc(ctx, (TZ_NBINS + 1) * 2, &d_lut));
    TZ_TRY(tz_upload(ctx, d_lut, h_lut2112, (TZ_NBINS + 1) * 2));
    tz_prof_scope ps(ctx, TZP_LUT);
    hipLaunchKernelGGL(k_lut, dim3(grid_for(n / 8 + 1, 256)), dim3(256), 0, ctx->stream, in, n, (const int16_t*)d_lut,
                       post_offset, out);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ---------------------------------------------------------------------------- byte shuffle
// Opt-in stage that is NOT in the reference (BASELINE.json's north star names it): the int16 payload
// is stored as two byte planes, all low bytes then all high bytes, before zstd sees it.  Ranks are
// < 1021, so the high plane is almost constant and the low plane loses the interleaved zeros.
// 4 B/element of HBM traffic each way; 8 elements per lane (16 B in, two 8 B stores).
__global__ __launch_bounds__(256) void k_shuffle(const int16_t* __restrict__ in, size_t n, uint8_t* __restrict__ out) {
    const size_t n8 = n / 8, stride = (size_t)gridDim.x * blockDim.x;
    const short8* in8 = (const short8*)in;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const short8 v = in8[i];
        unsigned long long lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned u = (unsigned short)v[k];
            lo |= (unsigned long long)(u & 0xFF) << (8 * k);
            hi |= (unsigned long long)(u >> 8) << (8 * k);
        }
        *(unsigned long long*)(out + 8 * i) = lo;
        *(unsigned long long*)(out + n + 8 * i) = hi;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
        const size_t i = n8 * 8 + threadIdx.x;
        const unsigned u = (unsigned short)in[i];
        out[i] = (uint8_t)(u & 0xFF);
        out[n + i] = (uint8_t)(u >> 8);
    }
}

__global__ __launch_bounds__(256) void k_unshuffle(const uint8_t* __restrict__ in, size_t n, int16_t* __restrict__ out) {
    const size_t n8 = n / 8, stride = (size_t)gridDim.x * blockDim.x;
    short8* out8 = (short8*)out;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        // `in` is 16-byte aligned (tzk_shuffle); the high plane starts at n, which need not be a multiple of 8: then its bytes
        // come one by one (volatile: eight plain byte loads, or a memcpy, the compiler folds into ONE 8-byte load at a byte address)
        const unsigned long long lo = *(const unsigned long long*)(in + 8 * i);
        unsigned long long hi = 0;
        if ((n & 7) == 0) {
            hi = *(const unsigned long long*)(in + n + 8 * i);
        } else {
            const volatile uint8_t* b = (const volatile uint8_t*)(in + n + 8 * i);
#pragma unroll
            for (int k = 0; k < 8; ++k) hi |= (unsigned long long)b[k] << (8 * k);
        }
        short8 r;
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = (short)(((lo >> (8 * k)) & 0xFF) | (((hi >> (8 * k)) & 0xFF) << 8));
        out8[i] = r;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
        const size_t i = n8 * 8 + threadIdx.x;
        out[i] = (int16_t)((unsigned)in[i] | ((unsigned)in[n + i] << 8));
    }
}

int tzk_shuffle(tz_ctx* ctx, const int16_t* in, size_t n, uint8_t* out, int inverse) {
    if (n == 0) return TZ_OK;
    if (((uintptr_t)in & 15) || ((uintptr_t)out & 15))
        return tz_fail(ctx, TZ_ERR_INVALID, "byte-shuffle buffers must be 16-byte aligned");
    tz_prof_scope ps(ctx, TZP_LUT);
    if (!inverse) {
        if (n & 7) return tz_fail(ctx, TZ_ERR_INVALID, "byte shuffle needs a multiple of 8 elements");
        hipLaunchKernelGGL(k_shuffle, dim3(grid_for(n / 8 + 1, 256)), dim3(256), 0, ctx->stream, in, n, out);
    } else {
        hipLaunchKernelGGL(k_unshuffle, dim3(grid_for(n / 8 + 1, 256)), dim3(256), 0, ctx->stream, (const uint8_t*)in, n,
                           (int16_t*)out);
    }
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------------------- inverse spatial delta (scan)
// decompress.py:22-29 is a serial loop x[i] = x[i-1] - s[i] (pure Python, forced onto the
// CPU by the reference, docs/index.rst:1392-1396).  It is the wrap-around prefix scan
//   x[i] = c0 - sum_{j<=i} s'[j]   (mod 2^16),  s'[0] = -s[0] and c0 = 0 without a carry.
// ONE launch of up to SCAN_G blocks (round 3; rounds 1-2: three launches, 85 us per 62.9 M elements):
// every wave of a block owns a contiguous run of wave-tiles; the block (1) sums its runs, (2) publishes the
// sum and reads the sums of the blocks in front of it -- they run at the same time (or ran before) and do the
// same work, so they are there within a round trip --, (3) walks its runs again, scanning tile by tile with
// wave shuffles only.  6 B/element move for 4 algorithmic, as before, but without the launch gaps and the
// scan-of-sums kernel in between.  A single pass with decoupled look-back (4 B/element) was built and measured
// and is NOT faster here: a look-back hop between workgroups on different XCDs takes several microseconds
// under streaming load (and a ticket counter serialises at 12 ns per block): 170-220 us in every
// variant (scripts/microbench/scan_lookback.hip, profiles/r03/scan_lookback.txt).
// With LUT the decoder's inverse rank remap (decompress.py:31-36,236: rank -> 1600 - symbol) is
// applied to the elements as they are loaded (both times), which removes the separate k_lut pass
// over the payload (4 B/element) from tz_decode; with RECON the reconstruction follows in the same walk.
// Progress: a block waits for lower-numbered blocks only, and the workgroups of a launch start in index order
// (per XCD), so the lowest-numbered unfinished block is always running and waits for nothing unfinished -- also
// when the grid is larger than what the chip holds at once (it is: two rounds measured fastest).
static constexpr unsigned SCAN_POLL_LIMIT = 1u << 22;   // polls of ONE status word before a thread gives up (a healthy wait is
                                                        // tens of polls; 2^22 L2 round trips are seconds)
static constexpr int SCAN_EPT = 16;                 // elements per thread
static constexpr int SCAN_KEEP = 4;                 // wave-tiles of a wave's run that stay in registers between the two phases
static constexpr int SCAN_G = 4096;                 // blocks of a launch: two rounds of the 2048 the chip holds (measured at
                                                    // 62.9 M elements, fused tail: 1024 108 us, 2048 107, 4096 96, 8192 110)

__device__ __forceinline__ unsigned block_scan_excl(unsigned v, unsigned* total) {
    __shared__ unsigned wsum[4];
    int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned inc = v;
    for (int s = 1; s < 64; s <<= 1) {
        unsigned up = __shfl_up(inc, s);
        if (lane >= s) inc += up;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned pre = 0, tot = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wv) pre += wsum[w];
        tot += wsum[w];
    }
    __syncthreads();
    *total = tot;
    return pre + inc - v;
}

// 16 consecutive elements of a tile for this thread: two 16-byte accesses (scalar at the ragged tail and
// for unaligned buffers), through the decoder LUT when there is one, the first element of the stream
// negated (s'[0] = -s[0]); elements past the end count as 0
template <bool LUT>
__device__ __forceinline__ void scan_load16(const int16_t* __restrict__ in, size_t base, size_t n, bool vec, bool first_neg,
                                            const int16_t* sl, int post_offset, int* v) {
    if (vec && base + SCAN_EPT <= n) {
        short8 a = *(const short8*)(in + base), b = *(const short8*)(in + base + 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            v[k] = a[k];
            v[8 + k] = b[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < SCAN_EPT; ++k) v[k] = base + k < n ? (int)in[base + k] : 0;
    }
    if (LUT) {
#pragma unroll
        for (int k = 0; k < SCAN_EPT; ++k) {
            const int x = v[k];
            const int y = (x >= 0 && x <= TZ_NBINS) ? (int)sl[x] : (int)(short)(post_offset ? TZ_OFFSET - x : x);
            v[k] = base + k < n ? y : 0;
        }
    }
    if (base == 0 && first_neg) v[0] = -v[0];
}

__device__ __forceinline__ unsigned st_load(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_store(unsigned* p, unsigned v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// What phase 3 does with the scanned values: store them (tz_spatial_undelta, tz_decode_delta's producer), or -- RECON, the
// decoder's tail in one kernel -- go straight on to decompress.py:252-256,269: the thread's 16 elements lie in one frame
// (frame_elems % 16 == 0, unpadded frames), whose base is 16 key bytes or 16 truncated predictions (loaded before the
// tile's scan so that their latency hides behind its barriers); 16 bytes out.  9 B/element move instead of 13.
struct ScanRecon {
    const float4* pred;       // [frame][H*W*3] floats
    const uint8_t* key;       // key-frame stack (bytes of non-key slots unused)
    const uint8_t* key_mask;  // [frame]
    unsigned long long fe;    // elements per frame
    uint8_t* out;
    int keep_regs;            // (every launch, RECON or not) 1: a wave's run stays in registers between the phases; TEZIP_SCAN_KEEP=0: A/B
};

// status[g] = epoch << 16 | (sum of block g's chunk mod 2^16); the words of a launch carry its epoch (1..65535, the
// context counts them), so nothing has to be cleared between launches.  Inside a block every WAVE owns a contiguous run of
// `wtiles` wave-tiles (64 lanes x 16 elements), so that the walks of phases 1 and 3 need wave shuffles only -- the block
// meets at two barriers, around the exchange of sums.
static constexpr int SCAN_WT = 64 * SCAN_EPT;   // elements per wave-tile

__device__ __forceinline__ unsigned wave_scan_incl(unsigned v) {
    const int lane = threadIdx.x & 63;
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned up = __shfl_up(v, s);
        if (lane >= s) v += up;
    }
    return v;
}

template <bool LUT, bool RECON>
__global__ __launch_bounds__(256) void k_scan2p(const int16_t* __restrict__ in, size_t n, int wtiles, int has_carry,
                                                int16_t carry, int vec, const int16_t* __restrict__ lut, int post_offset,
                                                unsigned* __restrict__ status, unsigned epoch, unsigned poll_epoch,
                                                unsigned poll_limit, unsigned* __restrict__ fault, int16_t* __restrict__ out,
                                                const ScanRecon rc) {
    __shared__ int16_t sl[LUT ? TZ_NBINS + 1 : 1];
    __shared__ unsigned wsum[4];
    if (LUT) {
        for (int k = threadIdx.x; k < TZ_NBINS + 1; k += 256) sl[k] = lut[k];
        __syncthreads();
    }
    const int g = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t chunk0 = ((size_t)g * 4 + wv) * (size_t)wtiles * SCAN_WT;   // of this wave
    // (1) the sum of the wave's run, then of the block's.  Round 6: a wave's run of up to SCAN_KEEP tiles STAYS IN REGISTERS
    // for phase 3 (two int16 per register, 32 registers; the loops are unrolled so that nothing is indexed at run time):
    // the payload is read once instead of twice -- the second read came from HBM (counter traffic 557 MB against 440 MB
    // algorithmic at 62.9 M elements).  Launches with longer runs (more than SCAN_G * 4 * SCAN_KEEP
    // wave-tiles: 67 M elements) read twice as before.
    unsigned s = 0;
    const bool keep = wtiles <= SCAN_KEEP && rc.keep_regs;   // (uniform over the launch)
    unsigned kept[SCAN_KEEP][SCAN_EPT / 2];
    if (keep) {
#pragma unroll
        for (int t = 0; t < SCAN_KEEP; ++t) {
            const size_t base = chunk0 + (size_t)t * SCAN_WT + (size_t)lane * SCAN_EPT;
            int v[SCAN_EPT];
#pragma unroll
            for (int k = 0; k < SCAN_EPT; ++k) v[k] = 0;
            if (t < wtiles && base < n) scan_load16<LUT>(in, base, n, vec != 0, !has_carry, sl, post_offset, v);
#pragma unroll
            for (int k = 0; k < SCAN_EPT; ++k) s += (unsigned)v[k];
#pragma unroll
            for (int k = 0; k < SCAN_EPT / 2; ++k) kept[t][k] = ((unsigned)v[2 * k] & 0xFFFFu) | ((unsigned)v[2 * k + 1] << 16);
        }
    } else {
        for (int t = 0; t < wtiles; ++t) {
            const size_t base = chunk0 + (size_t)t * SCAN_WT + (size_t)lane * SCAN_EPT;
            if (base >= n) break;
            int v[SCAN_EPT];
            scan_load16<LUT>(in, base, n, vec != 0, !has_carry, sl, post_offset, v);
#pragma unroll
            for (int k = 0; k < SCAN_EPT; ++k) s += (unsigned)v[k];
        }
    }
    s = wave_scan_incl(s);
    if (lane == 63) wsum[wv] = s;
    __syncthreads();
    unsigned front = 0, tot = 0;   // of the waves in front of this one in the block; of the block
    for (int w = 0; w < 4; ++w) {
        if (w < wv) front += wsum[w];
        tot += wsum[w];
    }
    if (threadIdx.x == 0) st_store(&status[g], epoch << 16 | (tot & 0xFFFFu));
    // (2) the sums of the blocks in front: thread t takes blocks t, t + 256, ...
    // The poll is BOUNDED: the argument above rests on the dispatch order of today's hardware, which HIP does not
    // promise.  A thread that has polled one word poll_limit times gives up, says so in the context's fault word (pinned
    // host memory, read by the host at its next synchronisation: TZ_ERR_HIP) and goes on with a wrong sum -- every block
    // has published its own sum BEFORE it polls, so a launch always drains.
    unsigned mine = 0;
    for (int b = threadIdx.x; b < g; b += 256) {
        unsigned w = st_load(&status[b]), spins = 0;
        while ((w >> 16) != poll_epoch) {
            if (++spins > poll_limit) {
                *(volatile unsigned*)fault = TZ_FAULT_SCAN_POLL;
                break;
            }
            w = st_load(&status[b]);
        }
        mine += w & 0xFFFFu;
    }
    unsigned run;
    block_scan_excl(mine, &run);
    run += front;
    // (3) scan the wave's run tile by tile
    const unsigned c0 = has_carry ? (unsigned)(int)carry : 0u;
    unsigned long long fr = 0, rr = 0;   // RECON: frame and offset in it of the tile's first element
    if (RECON) {
        fr = chunk0 / rc.fe;
        rr = chunk0 - fr * rc.fe;
    }
    auto tile = [&](int t, const unsigned* kv) {   // kv: the tile's values as phase 1 left them, or nullptr: load them again
        const size_t base = chunk0 + (size_t)t * SCAN_WT + (size_t)lane * SCAN_EPT;
        int bv[SCAN_EPT];
        if (RECON) {
            unsigned long long f = fr, r = rr + (unsigned long long)lane * SCAN_EPT;
            while (r >= rc.fe) {
                r -= rc.fe;
                ++f;
            }
            rr += SCAN_WT;
            while (rr >= rc.fe) {
                rr -= rc.fe;
                ++fr;
            }
            if (base < n) {   // n is a multiple of 16 here: all 16 elements exist
                if (rc.key_mask[f]) {
                    const uint4 k = *(const uint4*)(rc.key + base);
                    const unsigned kw[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
                    for (int j = 0; j < SCAN_EPT; ++j) bv[j] = (kw[j >> 2] >> (8 * (j & 3))) & 0xff;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float4 p = rc.pred[base / 4 + j];
                        bv[4 * j] = (int)(p.x * 255.0f);
                        bv[4 * j + 1] = (int)(p.y * 255.0f);
                        bv[4 * j + 2] = (int)(p.z * 255.0f);
                        bv[4 * j + 3] = (int)(p.w * 255.0f);
                    }
                }
            }
        }
        int v[SCAN_EPT];
        if (kv) {
#pragma unroll
            for (int k = 0; k < SCAN_EPT / 2; ++k) {
                v[2 * k] = (int)(short)(kv[k] & 0xFFFFu);
                v[2 * k + 1] = (int)(short)(kv[k] >> 16);
            }
        } else {
            scan_load16<LUT>(in, base, n, vec != 0, !has_carry, sl, post_offset, v);
        }
        unsigned q = 0;
#pragma unroll
        for (int k = 0; k < SCAN_EPT; ++k) q += (unsigned)v[k];
        const unsigned incl = wave_scan_incl(q);
        unsigned pre = incl - q + run;
        run += __shfl(incl, 63);
        short r[SCAN_EPT];
#pragma unroll
        for (int k = 0; k < SCAN_EPT; ++k) {
            pre += (unsigned)v[k];
            r[k] = (short)(uint16_t)(c0 - pre);
        }
        if (RECON) {
            if (base < n) {
                unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < SCAN_EPT; ++k) {
                    int x = bv[k] - (int)r[k];
                    x = x < 0 ? 0 : (x > 255 ? 255 : x);
                    w[k >> 2] |= (unsigned)x << (8 * (k & 3));
                }
                *(uint4*)(rc.out + base) = make_uint4(w[0], w[1], w[2], w[3]);
            }
        } else if (vec && base + SCAN_EPT <= n) {
            short8 a, b;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                a[k] = r[k];
                b[k] = r[8 + k];
            }
            *(short8*)(out + base) = a;
            *(short8*)(out + base + 8) = b;
        } else {
#pragma unroll
            for (int k = 0; k < SCAN_EPT; ++k)
                if (base + k < n) out[base + k] = r[k];
        }
    };
    if (keep) {
#pragma unroll
        for (int t = 0; t < SCAN_KEEP; ++t)
            if (t < wtiles && chunk0 + (size_t)t * SCAN_WT < n) tile(t, kept[t]);   // (uniform for the wave)
    } else {
        for (int t = 0; t < wtiles; ++t) {
            if (chunk0 + (size_t)t * SCAN_WT >= n) break;   // uniform for the wave
            tile(t, nullptr);
        }
    }
}

// pool memory holding the 2112+1-entry decode LUT (*d_lut = NULL without one)
static int upload_dec_lut(tz_ctx* ctx, const int16_t* h_lut2112, void** d_lut) {
    *d_lut = nullptr;
    if (!h_lut2112) return TZ_OK;
    TZ_TRY(tz_pool_alloc(ctx, (TZ_NBINS + 1) * 2, d_lut));
    return tz_upload(ctx, *d_lut, h_lut2112, (TZ_NBINS + 1) * 2);
}

// The host steps of an inverse-scan launch, k_scan2p's and k_scan3p's alike: the geometry (wave-tiles, blocks, tiles per wave),
// the LUT, the fault word, the status words of the kernel (its own buffer and epoch counter) tagged with a fresh epoch, the
// vec test; then launch(G, tiles per wave, d_lut, vec, epoch, the epoch to poll for, the poll limit).
template <class Status, class Launch>
static int scan_run(tz_ctx* ctx, const char* what, const int16_t* in, size_t n, const int16_t* out, const int16_t* h_lut2112,
                    Status** d_status, unsigned* epoch_counter, Launch launch) {
    if (n == 0) return TZ_OK;
    const size_t tiles = (n + SCAN_WT - 1) / SCAN_WT;                 // wave-tiles
    const int G = (int)std::min<size_t>(SCAN_G, (tiles + 3) / 4);
    const size_t tpb = (tiles + (size_t)G * 4 - 1) / ((size_t)G * 4);   // per wave
    if (tpb > 0x7FFFFFFFull) return tz_fail(ctx, TZ_ERR_INVALID, "%s: too many elements", what);
    void* d_lut;
    TZ_TRY(upload_dec_lut(ctx, h_lut2112, &d_lut));
    if (!*d_status) TZ_HIP(ctx, hipMalloc((void**)d_status, sizeof(Status) * SCAN_G));
    TZ_TRY(tz_fault_word(ctx));
    tz_prof_scope ps(ctx, TZP_SCAN);
    if (*epoch_counter == 0 || *epoch_counter == 0xFFFFu) {   // first launch, or the epochs have gone round
        TZ_HIP(ctx, hipMemsetAsync(*d_status, 0, sizeof(Status) * SCAN_G, ctx->stream));
        *epoch_counter = 0;
    }
    const unsigned epoch = ++*epoch_counter;
    const int vec = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    launch(G, (int)tpb, (const int16_t*)d_lut, vec, epoch, (epoch + ctx->scan_dbg_skew) & 0xFFFFu,
           ctx->scan_dbg_limit ? ctx->scan_dbg_limit : SCAN_POLL_LIMIT);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// k_scan2p over n elements: into `out`, or (recon) through the reconstruct into recon->out
static int scan_launch(tz_ctx* ctx, const int16_t* in, size_t n, int has_carry, int16_t carry, const int16_t* h_lut2112,
                       int post_offset, int16_t* out, const ScanRecon* recon = nullptr) {
    static const int keep_regs = !getenv("TEZIP_SCAN_KEEP") || atoi(getenv("TEZIP_SCAN_KEEP")) != 0;   // (0: A/B against the two reads)
    ScanRecon rcv = recon ? *recon : ScanRecon{};
    rcv.keep_regs = keep_regs;
    return scan_run(ctx, "inverse scan", in, n, out, h_lut2112, &ctx->d_scan_status, &ctx->scan_epoch,
                    [&](int G, int tpb, const int16_t* d_lut, int vec, unsigned epoch, unsigned poll_epoch, unsigned limit) {
#define TZ_SCAN_LAUNCH(L, R)                                                                                                     \
    hipLaunchKernelGGL((k_scan2p<L, R>), dim3(G), dim3(256), 0, ctx->stream, in, n, tpb, has_carry, carry, vec, d_lut, post_offset, \
                       ctx->d_scan_status, epoch, poll_epoch, limit, ctx->d_fault, out, rcv)
                        if (recon) {
                            if (h_lut2112) TZ_SCAN_LAUNCH(true, true);
                            else TZ_SCAN_LAUNCH(false, true);
                        } else {
                            if (h_lut2112) TZ_SCAN_LAUNCH(true, false);
                            else TZ_SCAN_LAUNCH(false, false);
                        }
#undef TZ_SCAN_LAUNCH
                    });
}

// ------------------------------------------------------------------------ prefix carry of the inverse scan
// A decoder that starts the inverse spatial delta at element n0 (tz_decode_range) needs the decoded element in front of
// it: x[n0-1] = -(sum_{j<n0} s'[j]) mod 2^16 (the scan above with c0 = 0, s'[0] = -s[0]; with LUT the symbols are the
// ones scan_load16<LUT> produces).  One read-only pass over the prefix, 2 B/element: 16-byte loads, a scalar head up to
// the first 16-byte boundary and a scalar tail; per-wave shuffle sums, then LDS, then ONE agent-scope atomic add per
// workgroup into a word the host clears with hipMemsetAsync in front of the launch.  The word sums the NEGATED symbols
// mod 2^32, so its low 16 bits are x[n0-1].  No hand-off between workgroups inside the launch: the consumer is the next
// launch on the stream, or a 4-byte read.
static constexpr int CARRY_UNROLL = 8;   // 16-byte loads in flight per thread and iteration (predicated: no serial tail)

template <bool LUT>
__device__ __forceinline__ unsigned carry_sym(int x, const int16_t* sl, int post_offset) {
    if (LUT) x = (x >= 0 && x <= TZ_NBINS) ? (int)sl[x] : (int)(short)(post_offset ? TZ_OFFSET - x : x);
    return (unsigned)x;
}

template <bool LUT>
__device__ __forceinline__ unsigned carry_sum8(short8 v, const int16_t* sl, int post_offset) {
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += carry_sym<LUT>(v[k], sl, post_offset);
    return s;
}

// head: elements in front of the first 16-byte boundary (0..7); the vectors start at in + head
template <bool LUT>
__global__ __launch_bounds__(256) void k_undelta_carry(const int16_t* __restrict__ in, size_t n, unsigned head,
                                                       const int16_t* __restrict__ lut, int post_offset,
                                                       unsigned* __restrict__ word) {
    __shared__ int16_t sl[LUT ? TZ_NBINS + 1 : 1];
    __shared__ unsigned wsum[4];
    if (LUT) {
        for (int k = threadIdx.x; k < TZ_NBINS + 1; k += 256) sl[k] = lut[k];
        __syncthreads();
    }
    const size_t n8 = (n - head) / 8, nthr = (size_t)gridDim.x * 256;
    const short8* in8 = (const short8*)(in + head);
    unsigned s = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += CARRY_UNROLL * nthr) {
        short8 v[CARRY_UNROLL];
#pragma unroll
        for (int u = 0; u < CARRY_UNROLL; ++u)
            if (i + u * nthr < n8) v[u] = in8[i + u * nthr];
#pragma unroll
        for (int u = 0; u < CARRY_UNROLL; ++u)
            if (i + u * nthr < n8) s += carry_sum8<LUT>(v[u], sl, post_offset);
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        const size_t t = head + n8 * 8 + threadIdx.x;                  // ragged tail
        if (threadIdx.x < head) s += carry_sym<LUT>(in[threadIdx.x], sl, post_offset);
        if (t < n) s += carry_sym<LUT>(in[t], sl, post_offset);
        if (threadIdx.x == 0) s -= 2u * carry_sym<LUT>(in[0], sl, post_offset);   // s'[0] = -s[0]
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_fetch_add(word, 0u - (wsum[0] + wsum[1] + wsum[2] + wsum[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// --------------------------------------------- inverse spatial delta at the channel stride (tz_set_delta_stride(1))
// x[i] = x[i-3] - s[i]: three interleaved wrap-around scans, one per class c = i mod 3 of the element index,
//   x[i] = c0[c] - sum_{j <= i, j = c (mod 3)} s'[j]   (mod 2^16),  s'[j] = -s[j] for j < 3 and c0 = 0 without a carry.
// k_scan3p has the two-phase shape of k_scan2p -- a wave owns a contiguous run of wave-tiles; sum the run, publish the block's
// sums, poll the blocks in front (bounded, fault word), walk the run again -- with THREE sums wherever k_scan2p has one.
// A thread's 16 elements start at an index that is no multiple of 3 (16 = 1 mod 3): it sums them by the class RELATIVE to
// its first element (k % 3, a compile-time index into three registers) and rotates the three sums into stream classes by
// r = base % 3 with selects (rot3); prefixes go back the same way.  No register is indexed at run time.
// status[g] = epoch << 48 | sum2 << 32 | sum1 << 16 | sum0 (each mod 2^16) is ONE naturally aligned 64-bit word, written by
// one 64-bit atomic store and read by 64-bit atomic loads: such an access is single-copy atomic, so a reader that sees the
// launch's epoch sees the three sums stored with it -- there is no second word whose order against the first would matter,
// and relaxed ordering suffices because nothing else is communicated through memory.  The words have their own epoch counter
// (1..65535) and are cleared when it wraps, as k_scan2p's.  The payload is read twice (no register-kept run) and the
// reconstruction is a second kernel: 6 B/element here plus tzk_reconstruct.
__device__ __forceinline__ unsigned long long st_load64(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_store64(unsigned long long* p, unsigned long long v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// g[(r + j) % 3] = a[j]: from classes relative to an element of class r to stream classes.  rot3((3 - r) % 3, ...) is the inverse.
__device__ __forceinline__ void rot3(unsigned r, unsigned a0, unsigned a1, unsigned a2, unsigned& g0, unsigned& g1, unsigned& g2) {
    g0 = r == 0 ? a0 : (r == 1 ? a2 : a1);
    g1 = r == 0 ? a1 : (r == 1 ? a0 : a2);
    g2 = r == 0 ? a2 : (r == 1 ? a1 : a0);
}

// scan_load16 for the strided scan: the first THREE elements of the stream are negated; then the thread's sums by relative class
template <bool LUT>
__device__ __forceinline__ void scan3_load16(const int16_t* __restrict__ in, size_t base, size_t n, bool vec, bool neg_head,
                                             const int16_t* sl, int post_offset, int* v, unsigned* a) {
    scan_load16<LUT>(in, base, n, vec, false, sl, post_offset, v);
    if (base == 0 && neg_head) {   // (elements past the end are 0)
        v[0] = -v[0];
        v[1] = -v[1];
        v[2] = -v[2];
    }
    a[0] = a[1] = a[2] = 0;
#pragma unroll
    for (int k = 0; k < SCAN_EPT; ++k) a[k % 3] += (unsigned)v[k];
}

template <bool LUT>
__global__ __launch_bounds__(256) void k_scan3p(const int16_t* __restrict__ in, size_t n, int wtiles, int has_carry, short c0, short c1,
                                                short c2, int vec, const int16_t* __restrict__ lut, int post_offset,
                                                unsigned long long* __restrict__ status, unsigned epoch, unsigned poll_epoch,
                                                unsigned poll_limit, unsigned* __restrict__ fault, int16_t* __restrict__ out) {
    __shared__ int16_t sl[LUT ? TZ_NBINS + 1 : 1];
    __shared__ unsigned wsum[4][3], bsum[4][3];
    if (LUT) {
        for (int k = threadIdx.x; k < TZ_NBINS + 1; k += 256) sl[k] = lut[k];
        __syncthreads();
    }
    const int g = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t chunk0 = ((size_t)g * 4 + wv) * (size_t)wtiles * SCAN_WT;   // of this wave
    // (1) the three sums of the wave's run, then of the block's
    unsigned s0 = 0, s1 = 0, s2 = 0;
    for (int t = 0; t < wtiles; ++t) {
        const size_t base = chunk0 + (size_t)t * SCAN_WT + (size_t)lane * SCAN_EPT;
        if (base >= n) break;
        int v[SCAN_EPT];
        unsigned a[3], g0, g1, g2;
        scan3_load16<LUT>(in, base, n, vec != 0, !has_carry, sl, post_offset, v, a);
        rot3((unsigned)(base % 3), a[0], a[1], a[2], g0, g1, g2);
        s0 += g0;
        s1 += g1;
        s2 += g2;
    }
    s0 = wave_scan_incl(s0);
    s1 = wave_scan_incl(s1);
    s2 = wave_scan_incl(s2);
    if (lane == 63) {
        wsum[wv][0] = s0;
        wsum[wv][1] = s1;
        wsum[wv][2] = s2;
    }
    __syncthreads();
    unsigned front[3] = {0, 0, 0}, tot[3] = {0, 0, 0};   // of the waves in front of this one in the block; of the block
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (w < wv) front[c] += wsum[w][c];
            tot[c] += wsum[w][c];
        }
    if (threadIdx.x == 0)
        st_store64(&status[g], (unsigned long long)epoch << 48 | (unsigned long long)(tot[2] & 0xFFFFu) << 32 |
                                   (unsigned long long)(tot[1] & 0xFFFFu) << 16 | (unsigned long long)(tot[0] & 0xFFFFu));
    // (2) the sums of the blocks in front: thread t takes blocks t, t + 256, ...; the poll is bounded as k_scan2p's, and every
    // block has published its own word BEFORE it polls, so a launch always drains
    unsigned m0 = 0, m1 = 0, m2 = 0;
    for (int b = threadIdx.x; b < g; b += 256) {
        unsigned long long w = st_load64(&status[b]);
        unsigned spins = 0;
        while ((unsigned)(w >> 48) != poll_epoch) {
            if (++spins > poll_limit) {
                *(volatile unsigned*)fault = TZ_FAULT_SCAN_POLL;
                break;
            }
            w = st_load64(&status[b]);
        }
        m0 += (unsigned)w & 0xFFFFu;
        m1 += (unsigned)(w >> 16) & 0xFFFFu;
        m2 += (unsigned)(w >> 32) & 0xFFFFu;
    }
    m0 = wave_scan_incl(m0);
    m1 = wave_scan_incl(m1);
    m2 = wave_scan_incl(m2);
    if (lane == 63) {
        bsum[wv][0] = m0;
        bsum[wv][1] = m1;
        bsum[wv][2] = m2;
    }
    __syncthreads();
    unsigned run[3];   // per stream class: the sum of everything in front of the wave's next tile
#pragma unroll
    for (int c = 0; c < 3; ++c) run[c] = front[c] + bsum[0][c] + bsum[1][c] + bsum[2][c] + bsum[3][c];
    // (3) scan the wave's run tile by tile
    const unsigned cc0 = has_carry ? (unsigned)(int)c0 : 0u, cc1 = has_carry ? (unsigned)(int)c1 : 0u, cc2 = has_carry ? (unsigned)(int)c2 : 0u;
    for (int t = 0; t < wtiles; ++t) {
        if (chunk0 + (size_t)t * SCAN_WT >= n) break;   // uniform for the wave
        const size_t base = chunk0 + (size_t)t * SCAN_WT + (size_t)lane * SCAN_EPT;
        int v[SCAN_EPT];
        unsigned a[3], q0, q1, q2;
        scan3_load16<LUT>(in, base, n, vec != 0, !has_carry, sl, post_offset, v, a);   // (all 0 for a lane past the end)
        const unsigned r = (unsigned)(base % 3), rinv = (3u - r) % 3u;
        rot3(r, a[0], a[1], a[2], q0, q1, q2);
        const unsigned i0 = wave_scan_incl(q0), i1 = wave_scan_incl(q1), i2 = wave_scan_incl(q2);
        unsigned p[3], cl[3];   // by relative class: the sums in front of the thread's elements, and the carries
        rot3(rinv, i0 - q0 + run[0], i1 - q1 + run[1], i2 - q2 + run[2], p[0], p[1], p[2]);
        rot3(rinv, cc0, cc1, cc2, cl[0], cl[1], cl[2]);
        run[0] += __shfl(i0, 63);
        run[1] += __shfl(i1, 63);
        run[2] += __shfl(i2, 63);
        short res[SCAN_EPT];
#pragma unroll
        for (int k = 0; k < SCAN_EPT; ++k) {
            p[k % 3] += (unsigned)v[k];
            res[k] = (short)(uint16_t)(cl[k % 3] - p[k % 3]);
        }
        if (vec && base + SCAN_EPT <= n) {
            short8 x, y;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                x[k] = res[k];
                y[k] = res[8 + k];
            }
            *(short8*)(out + base) = x;
            *(short8*)(out + base + 8) = y;
        } else {
#pragma unroll
            for (int k = 0; k < SCAN_EPT; ++k)
                if (base + k < n) out[base + k] = res[k];
        }
    }
}

// The inverse spatial delta at either stride: k_scan2p, or k_scan3p over any 2-byte aligned buffers.  carry: NULL at the stream
// start, else the `stride` HOST elements in front of in[0]; h_lut2112 NULL = symbols as stored.
int tzk_undelta(tz_ctx* ctx, int stride, const int16_t* in, size_t n, const int16_t* carry, const int16_t* h_lut2112, int post_offset,
                int16_t* out) {
    if (stride != 3) return scan_launch(ctx, in, n, carry != nullptr, carry ? carry[0] : (int16_t)0, h_lut2112, post_offset, out);
    if (n == 0) return TZ_OK;
    if (((uintptr_t)in | (uintptr_t)out) & 1) return tz_fail(ctx, TZ_ERR_INVALID, "strided inverse scan: buffers must be 2-byte aligned");
    const short c0 = carry ? carry[0] : 0, c1 = carry ? carry[1] : 0, c2 = carry ? carry[2] : 0;
    return scan_run(ctx, "strided inverse scan", in, n, out, h_lut2112, &ctx->d_scan3_status, &ctx->scan3_epoch,
                    [&](int G, int tpb, const int16_t* d_lut, int vec, unsigned epoch, unsigned poll_epoch, unsigned limit) {
#define TZ_SCAN3_LAUNCH(L)                                                                                                       \
    hipLaunchKernelGGL((k_scan3p<L>), dim3(G), dim3(256), 0, ctx->stream, in, n, tpb, carry != nullptr, c0, c1, c2, vec, d_lut,   \
                       post_offset, ctx->d_scan3_status, epoch, poll_epoch, limit, ctx->d_fault, out)
                        if (h_lut2112) TZ_SCAN3_LAUNCH(true);
                        else TZ_SCAN3_LAUNCH(false);
#undef TZ_SCAN3_LAUNCH
                    });
}

// The three class sums of a prefix: k_undelta_carry with one sum per class of the element index mod 3.  A thread takes 24
// elements per step (three 16-byte loads), so the class of its k-th element RELATIVE to in[head] is k % 3 in every step: three
// registers indexed at compile time, rotated once at the end by head % 3.  The head in front of the first 16-byte boundary and
// the (n - head) % 24 elements behind the vectors are taken one by one by the first lanes of block 0.  words[c] receives the
// negated sum of class c: its low 16 bits are the decoded element of class c in front of in[n].
template <bool LUT>
__global__ __launch_bounds__(256) void k_undelta_carry_s3(const int16_t* __restrict__ in, size_t n, unsigned head,
                                                          const int16_t* __restrict__ lut, int post_offset,
                                                          unsigned* __restrict__ words) {
    __shared__ int16_t sl[LUT ? TZ_NBINS + 1 : 1];
    __shared__ unsigned wsum[4][3];
    if (LUT) {
        for (int k = threadIdx.x; k < TZ_NBINS + 1; k += 256) sl[k] = lut[k];
        __syncthreads();
    }
    const size_t n24 = (n - head) / 24, nthr = (size_t)gridDim.x * 256;
    const short8* in8 = (const short8*)(in + head);
    unsigned a[3] = {0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n24; i += nthr) {
        const short8 v0 = in8[3 * i], v1 = in8[3 * i + 1], v2 = in8[3 * i + 2];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            a[k % 3] += carry_sym<LUT>(v0[k], sl, post_offset);
            a[(8 + k) % 3] += carry_sym<LUT>(v1[k], sl, post_offset);
            a[(16 + k) % 3] += carry_sym<LUT>(v2[k], sl, post_offset);
        }
    }
    unsigned s[3];
    rot3(head % 3u, a[0], a[1], a[2], s[0], s[1], s[2]);
    if (blockIdx.x == 0 && threadIdx.x < 32) {   // head < 8 and tail < 24 elements: one per lane
        const size_t e = threadIdx.x < head ? (size_t)threadIdx.x : head + n24 * 24 + (threadIdx.x - head);
        if (e < n) {
            const unsigned x = carry_sym<LUT>(in[e], sl, post_offset);
            const unsigned c = (unsigned)(e % 3);
            s[0] += c == 0 ? x : 0u;
            s[1] += c == 1 ? x : 0u;
            s[2] += c == 2 ? x : 0u;
        }
        if (threadIdx.x < 3) {   // s'[j] = -s[j] for j < 3 (n >= 3)
            const unsigned x = 2u * carry_sym<LUT>(in[threadIdx.x], sl, post_offset);
            s[0] -= threadIdx.x == 0 ? x : 0u;
            s[1] -= threadIdx.x == 1 ? x : 0u;
            s[2] -= threadIdx.x == 2 ? x : 0u;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        for (int off = 32; off > 0; off >>= 1) s[c] += __shfl_down(s[c], off);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < 3)
        __hip_atomic_fetch_add(&words[threadIdx.x], 0u - (wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x]),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// enqueue the carry of payload[0, n0) into d_words[0 .. stride) (device; the low 16 bits of each word): the decoded elements in
// front of in[n0].  h_lut2112 NULL = symbols as stored.  Stride 3: n0 a positive multiple of 3.
int tzk_undelta_carry(tz_ctx* ctx, int stride, const int16_t* in, size_t n0, const int16_t* h_lut2112, int post_offset, unsigned* d_words) {
    const bool s3 = stride == 3;
    if (s3 && (n0 == 0 || n0 % 3)) return tz_fail(ctx, TZ_ERR_INVALID, "strided undelta carry: n0 = %zu is not a positive multiple of 3", n0);
    if (n0 == 0) return tz_fail(ctx, TZ_ERR_INVALID, "undelta carry: the stream start has no carry");
    if (((uintptr_t)in & 1) != 0) return tz_fail(ctx, TZ_ERR_INVALID, "%sundelta carry: payload not 2-byte aligned", s3 ? "strided " : "");
    void* d_lut;
    TZ_TRY(upload_dec_lut(ctx, h_lut2112, &d_lut));
    const unsigned head = (unsigned)std::min<size_t>(n0, ((16 - ((uintptr_t)in & 15)) & 15) / 2);
    TZ_HIP(ctx, hipMemsetAsync(d_words, 0, (s3 ? 3 : 1) * sizeof(unsigned), ctx->stream));
    const int G = grid_for((n0 - head) / (s3 ? 24 : 8 * CARRY_UNROLL) + 1, 256);
    tz_prof_scope ps(ctx, TZP_CARRY);
#define TZ_CARRY_LAUNCH(K) \
    hipLaunchKernelGGL(K, dim3(G), dim3(256), 0, ctx->stream, in, n0, head, (const int16_t*)d_lut, post_offset, d_words)
    if (!s3 && h_lut2112) TZ_CARRY_LAUNCH(k_undelta_carry<true>);
    else if (!s3) TZ_CARRY_LAUNCH(k_undelta_carry<false>);
    else if (h_lut2112) TZ_CARRY_LAUNCH(k_undelta_carry_s3<true>);
    else TZ_CARRY_LAUNCH(k_undelta_carry_s3<false>);
#undef TZ_CARRY_LAUNCH
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ----------------------------------------------------------------------------- reconstruct
// decompress.py:252-256,269: pred*255 - diff, clip [0,255], truncate.  pred*255 in float64
// minus an integer, clipped and truncated equals clamp(trunc(f32(pred*255)) - diff, 0, 255)
// (DESIGN.md §"Why reconstruct is integer"); key slots use the key byte as base.
__global__ __launch_bounds__(256) void k_recon(const float* __restrict__ pred, const uint8_t* __restrict__ key,
                                               const uint8_t* __restrict__ key_mask, const int16_t* __restrict__ diff,
                                               size_t n, int H, int W, int Hp, int Wp, int out_dwords, uint8_t* __restrict__ out) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t row = (size_t)W * 3, fe = (size_t)H * row, fp = (size_t)Hp * Wp * 3;
    size_t n4 = n / 4;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4 + (n & 3 ? 1 : 0); q += stride) {
        unsigned packed = 0;
        int cnt = q < n4 ? 4 : (int)(n & 3);
        for (int k = 0; k < cnt; ++k) {
            size_t i = q * 4 + k;
            size_t f = i / fe, r = i - f * fe;
            int base;
            if (key_mask[f]) {
                base = key[i];
            } else {
                size_t y = r / row, xc = r - y * row;
                base = (int)(pred[f * fp + y * (size_t)Wp * 3 + xc] * 255.0f);
            }
            int v = base - (int)diff[i];
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            packed |= (unsigned)v << (8 * k);
        }
        if (cnt == 4 && out_dwords) ((unsigned*)out)[q] = packed;   // (out_dwords: `out` is on a 4-byte boundary)
        else
            for (int k = 0; k < cnt; ++k) out[q * 4 + k] = (uint8_t)(packed >> (8 * k));
    }
}

// Group i (8 elements) of an unpadded three-channel stack: its 8 key bytes or 8 truncated predictions, minus the deltas d, clamped.
__device__ __forceinline__ uint2 recon8_flat(const float4* __restrict__ pred, const uint2* __restrict__ key, bool is_key, size_t i,
                                             const short8 d) {
    int base[8];
    if (is_key) {
        uint2 k = key[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            base[j] = (k.x >> (8 * j)) & 0xff;
            base[4 + j] = (k.y >> (8 * j)) & 0xff;
        }
    } else {
        float4 p0 = pred[2 * i], p1 = pred[2 * i + 1];
        base[0] = (int)(p0.x * 255.0f); base[1] = (int)(p0.y * 255.0f);
        base[2] = (int)(p0.z * 255.0f); base[3] = (int)(p0.w * 255.0f);
        base[4] = (int)(p1.x * 255.0f); base[5] = (int)(p1.y * 255.0f);
        base[6] = (int)(p1.z * 255.0f); base[7] = (int)(p1.w * 255.0f);
    }
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int a = base[j] - (int)d[j], b = base[4 + j] - (int)d[4 + j];
        a = a < 0 ? 0 : (a > 255 ? 255 : a);
        b = b < 0 ? 0 : (b > 255 ? 255 : b);
        lo |= (unsigned)a << (8 * j);
        hi |= (unsigned)b << (8 * j);
    }
    return make_uint2(lo, hi);
}

// Fast path: unpadded frames, 8 elements per lane (2x16 B pred, 16 B diff, 8 B key, 8 B out).
__global__ __launch_bounds__(256) void k_recon_flat(const float4* __restrict__ pred, const uint2* __restrict__ key,
                                                    const uint8_t* __restrict__ key_mask, const short8* __restrict__ diff,
                                                    size_t n8, unsigned frame_elems8, uint2* __restrict__ out) {
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride)
        out[i] = recon8_flat(pred, key, key_mask[i / frame_elems8] != 0, i, diff[i]);
}

// ---------------------------------------------------------- reconstruct from a one-channel payload (gray job)
// tz_set_payload_channels(1): diff holds ONE delta per pixel; base = the key byte of channel 0 (key slots) or
// trunc(pred channel 0 * 255), v = clamp(base - d, 0, 255) is written to all three channels.  General form: crop of a padded
// prediction as k_recon; a thread takes 4 pixels and writes their 12 bytes as three dwords when `out` allows it.
__global__ __launch_bounds__(256) void k_recon_gray(const float* __restrict__ pred, const uint8_t* __restrict__ key,
                                                    const uint8_t* __restrict__ key_mask, const int16_t* __restrict__ diff,
                                                    size_t n1, int H, int W, int Hp, int Wp, int out_dwords, uint8_t* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t fpix = (size_t)H * W, fp = (size_t)Hp * Wp * 3;
    const size_t n4 = n1 / 4;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n4 + (n1 & 3 ? 1 : 0); q += stride) {
        unsigned v4[4] = {0, 0, 0, 0};
        const int cnt = q < n4 ? 4 : (int)(n1 & 3);
        for (int k = 0; k < cnt; ++k) {
            const size_t p = q * 4 + k;
            const size_t f = p / fpix, r = p - f * fpix;
            int base;
            if (key_mask[f]) {
                base = key[3 * p];
            } else {
                const size_t y = r / (size_t)W, x = r - y * (size_t)W;
                base = (int)(pred[f * fp + (y * (size_t)Wp + x) * 3] * 255.0f);
            }
            int v = base - (int)diff[p];
            v4[k] = (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
        if (cnt == 4 && out_dwords) {   // bytes v0 v0 v0 v1 | v1 v1 v2 v2 | v2 v3 v3 v3
            unsigned* o = (unsigned*)(out + 12 * q);
            o[0] = v4[0] * 0x010101u | (v4[1] << 24);
            o[1] = v4[1] * 0x0101u | (v4[2] * 0x0101u << 16);
            o[2] = v4[2] | (v4[3] * 0x010101u << 8);
        } else {
            for (int k = 0; k < cnt; ++k) {
                uint8_t* o = out + 3 * (q * 4 + k);
                o[0] = o[1] = o[2] = (uint8_t)v4[k];
            }
        }
    }
}

// Pixel group i (8 pixels) of an unpadded stack under a one-channel payload: channel 0's key byte or truncated prediction minus
// the delta, clamped, to all three channels.
__device__ __forceinline__ void recon8_gray(const float4* __restrict__ pred, const uint2* __restrict__ key, bool is_key, size_t i,
                                            const short8 d, uint2* __restrict__ out) {
    int base[8];
    if (is_key) {
        const uint2 k0 = key[3 * i], k1 = key[3 * i + 1], k2 = key[3 * i + 2];
        // channel 0 of pixel k is byte 3 k of the 24
        base[0] = k0.x & 0xff;          base[1] = k0.x >> 24;
        base[2] = (k0.y >> 16) & 0xff;  base[3] = (k1.x >> 8) & 0xff;
        base[4] = k1.y & 0xff;          base[5] = k1.y >> 24;
        base[6] = (k2.x >> 16) & 0xff;  base[7] = (k2.y >> 8) & 0xff;
    } else {
        // channel 0 of pixel k is float 3 k of the 24
        const float4 p0 = pred[6 * i], p1 = pred[6 * i + 1], p2 = pred[6 * i + 2], p3 = pred[6 * i + 3], p4 = pred[6 * i + 4],
                     p5 = pred[6 * i + 5];
        base[0] = (int)(p0.x * 255.0f); base[1] = (int)(p0.w * 255.0f);
        base[2] = (int)(p1.z * 255.0f); base[3] = (int)(p2.y * 255.0f);
        base[4] = (int)(p3.x * 255.0f); base[5] = (int)(p3.w * 255.0f);
        base[6] = (int)(p4.z * 255.0f); base[7] = (int)(p5.y * 255.0f);
    }
    unsigned v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int a = base[j] - (int)d[j];
        v[j] = (unsigned)(a < 0 ? 0 : (a > 255 ? 255 : a));
    }
    // bytes v0 v0 v0 v1 | v1 v1 v2 v2 | v2 v3 v3 v3, twice
    out[3 * i] = make_uint2(v[0] * 0x010101u | (v[1] << 24), v[1] * 0x0101u | (v[2] * 0x0101u << 16));
    out[3 * i + 1] = make_uint2(v[2] | (v[3] * 0x010101u << 8), v[4] * 0x010101u | (v[5] << 24));
    out[3 * i + 2] = make_uint2(v[5] * 0x0101u | (v[6] * 0x0101u << 16), v[6] | (v[7] * 0x010101u << 8));
}

// Flat form: unpadded frames of a multiple of 8 pixels, 8 pixels per lane: 16 B of deltas, the 96 B of prediction (or the
// 24 B of key bytes) that hold their channel 0, 24 B out as three aligned 8-byte stores.
__global__ __launch_bounds__(256) void k_recon_gray_flat(const float4* __restrict__ pred, const uint2* __restrict__ key,
                                                         const uint8_t* __restrict__ key_mask, const short8* __restrict__ diff,
                                                         size_t n8, unsigned frame_pix8, uint2* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride)
        recon8_gray(pred, key, key_mask[i / frame_pix8] != 0, i, diff[i], out);
}

// k_recon* over a diff stack of three elements per pixel, k_recon_gray* over one (channels = 1): the flat form where the frames
// are unpadded and a frame holds whole groups of 8 elements, on aligned buffers; else the general form.
int tzk_reconstruct(tz_ctx* ctx, int channels, const float* pred, const uint8_t* key, const uint8_t* d_key_mask, const int16_t* diff,
                    int nframes, int H, int W, int Hp, int Wp, uint8_t* out) {
    const size_t fe = (size_t)H * W * channels, n = (size_t)nframes * fe;   // diff elements
    if (n == 0) return TZ_OK;
    const bool gray = channels == 1;
    tz_prof_scope ps(ctx, TZP_RECON);
    if (H == Hp && W == Wp && fe % 8 == 0 && key && ((((uintptr_t)diff | (uintptr_t)pred) & 15) == 0) &&
        ((((uintptr_t)key | (uintptr_t)out) & 7) == 0)) {
        hipLaunchKernelGGL(gray ? k_recon_gray_flat : k_recon_flat, dim3(grid_for(n / 8, 256)), dim3(256), 0, ctx->stream,
                           (const float4*)pred, (const uint2*)key, d_key_mask, (const short8*)diff, n / 8, (unsigned)(fe / 8), (uint2*)out);
    } else if (gray) {
        hipLaunchKernelGGL(k_recon_gray, dim3(grid_for(n / 4 + 1, 256)), dim3(256), 0, ctx->stream, pred, key, d_key_mask, diff, n, H, W,
                           Hp, Wp, (int)(((uintptr_t)out & 3) == 0), out);
    } else {
        hipLaunchKernelGGL(k_recon, dim3(grid_for(n / 4 + 1, 256)), dim3(256), 0, ctx->stream, pred, key, d_key_mask, diff, n, H, W, Hp,
                           Wp, (int)(((uintptr_t)out & 3) == 0), out);
    }
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------- inverse of the 2-D spatial delta (TZ-SD2, tz_set_delta_plane(1))
// q = wrap9(S), S[y, x] the inclusive 2-D prefix sum of -sd over the frame and channel (tezip_amd/sdelta.py decode_plane).  The
// sum is separable -- down the columns, then along the rows -- and sums are taken mod 2^16 (512 divides 65536).  Two launches;
// neither waits on another workgroup: no status words, no polling.
// Pass one, k_unplane_cols<LUT, V>: a frame is H rows of W*C independent columns.  Lanes lie along the row (V columns each:
// 4 as one 8-byte access where a row is whole 8-byte groups on 8-byte boundaries, else 1), the decoder LUT is applied on load,
// the value negated, and each lane walks down with running sums, several rows' loads in flight.  The four waves of a workgroup
// take four row bands of one column strip (one band while H <= UNPLANE_BAND_ROWS): they sum their bands, exchange the sums
// through LDS behind ONE barrier, then walk again and store.
// Pass two, k_unplane_rows<C>: a wave owns whole rows and walks one in wave-tiles of UNPLANE_ROW_TILE elements: per-thread sums
// by class mod C (relative to the thread's first element, rotated into row classes by rot3 as k_scan3p does), a wave shuffle
// scan, a running row carry in registers; then wrap9.  A lane reads its 8 elements before it writes them and a row's tiles are
// walked in order by one wave, so the pass runs IN PLACE on pass one's output.  RECON (the decoder's tail on unpadded frames whose
// rows are whole 16-byte groups on 16-byte boundaries): the lane goes straight on to decompress.py:252-256,269 with its 8 deltas
// -- the group's key bytes or truncated predictions, clamp, uint8 out; with C = 1 the sample goes to all three channels
// (recon8_flat / recon8_gray, the bodies of k_recon_flat / k_recon_gray_flat) -- and no delta stack is written.
// Pass one carries the LUT because it is the pass that reads the payload; pass two carries wrap9 and RECON because it is the last
// one, and because it leaves the frame in row order, which is the order of pred, key and out: rows last, a lane's 8 deltas are
// 8 neighbouring bytes of the frame, columns last they would be 8 rows apart.
static constexpr int UNPLANE_BAND_ROWS = 32;                  // fewest rows of a band of k_unplane_cols
static constexpr int UNPLANE_ROW_EPT = 8;                     // elements per lane of k_unplane_rows
static constexpr int UNPLANE_ROW_TILE = 64 * UNPLANE_ROW_EPT; // elements of its wave-tile

template <bool LUT>
__device__ __forceinline__ unsigned unplane_sym(int x, const int16_t* sl, int post_offset) {
    if (LUT) return (unsigned)((x >= 0 && x <= TZ_NBINS) ? (int)sl[x] : (int)(short)(post_offset ? TZ_OFFSET - x : x));
    return (unsigned)x;
}

template <int V>
__device__ __forceinline__ void unplane_load(const int16_t* p, int* x) {
    if (V == 4) {
        const uint2 w = *(const uint2*)p;
        x[0] = (int)(short)(w.x & 0xFFFFu);
        x[1] = (int)w.x >> 16;
        x[2] = (int)(short)(w.y & 0xFFFFu);
        x[3] = (int)w.y >> 16;
    } else {
        x[0] = p[0];
    }
}

template <bool LUT, int V>
__global__ __launch_bounds__(256) void k_unplane_cols(const int16_t* __restrict__ in, int nframes, int H, int RW, int band_rows,
                                                      const int16_t* __restrict__ lut, int post_offset, int16_t* __restrict__ out) {
    __shared__ int16_t sl[LUT ? TZ_NBINS + 1 : 1];
    __shared__ unsigned bsum[2][4][64 * V];
    if (LUT) {
        for (int k = threadIdx.x; k < TZ_NBINS + 1; k += 256) sl[k] = lut[k];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * V;
    const bool active = col < RW;   // (V == 4: RW is a multiple of 4, so are the lane's columns)
    const bool multi = band_rows < H;   // uniform for the launch
    const int y0 = multi ? min(H, wv * band_rows) : (wv == 0 ? 0 : H), y1 = multi ? min(H, y0 + band_rows) : (wv == 0 ? H : H);
    int it = 0;
    for (int f = blockIdx.y; f < nframes; f += gridDim.y, ++it) {
        const size_t fbase = (size_t)f * H * RW + col;
        unsigned acc[V];
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = 0u;
        if (multi) {
            if (active && wv < 3) {   // (nobody needs the last band's sum)
#pragma unroll 4
                for (int y = y0; y < y1; ++y) {
                    int x[V];
                    unplane_load<V>(in + fbase + (size_t)y * RW, x);
#pragma unroll
                    for (int k = 0; k < V; ++k) acc[k] -= unplane_sym<LUT>(x[k], sl, post_offset);
                }
            }
            unsigned(*bs)[64 * V] = bsum[it & 1];   // (two sets: the next frame's sums never meet a late reader of this one's)
#pragma unroll
            for (int k = 0; k < V; ++k) bs[wv][lane * V + k] = acc[k];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < V; ++k) {
                acc[k] = 0u;
                for (int w = 0; w < 3; ++w)
                    if (w < wv) acc[k] += bs[w][lane * V + k];
            }
        }
        if (!active) continue;
#pragma unroll 4
        for (int y = y0; y < y1; ++y) {
            int x[V];
            unplane_load<V>(in + fbase + (size_t)y * RW, x);
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] -= unplane_sym<LUT>(x[k], sl, post_offset);
            int16_t* o = out + fbase + (size_t)y * RW;
            if (V == 4) *(uint2*)o = make_uint2((acc[0] & 0xFFFFu) | (acc[1] << 16), (acc[2] & 0xFFFFu) | (acc[3] << 16));
            else o[0] = (int16_t)(uint16_t)acc[0];
        }
    }
}

__device__ __forceinline__ short unplane_wrap9(unsigned s) { return (short)((int)((s + 256u) & 511u) - 256); }

struct PlaneRecon {
    const float4* pred;       // [frame][H*W*3] floats
    const uint8_t* key;       // key-frame stack (bytes of non-key slots unused)
    const uint8_t* key_mask;  // [frame]
    int H;                    // rows of a frame
    uint8_t* out;
};

// in and out may be the same buffer (RECON: out is not written, vec is set and RW is a multiple of 8)
template <int C, bool RECON>
__global__ __launch_bounds__(256) void k_unplane_rows(const int16_t* in, size_t nrows, int RW, int vec, int16_t* out, const PlaneRecon rc) {
    const int lane = threadIdx.x & 63;
    const size_t nwaves = (size_t)gridDim.x * 4;
    for (size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < nrows; row += nwaves) {
        const int16_t* src = in + row * (size_t)RW;
        int16_t* dst = out + row * (size_t)RW;
        unsigned run[3] = {0u, 0u, 0u};   // per row class: the sum of everything in front of the next tile
        for (int tb = 0; tb < RW; tb += UNPLANE_ROW_TILE) {   // uniform for the wave
            const int base = tb + lane * UNPLANE_ROW_EPT;
            const bool whole = vec && base + UNPLANE_ROW_EPT <= RW;
            int v[UNPLANE_ROW_EPT];
            if (whole) {
                const short8 a = *(const short8*)(src + base);
#pragma unroll
                for (int k = 0; k < UNPLANE_ROW_EPT; ++k) v[k] = a[k];
            } else {
#pragma unroll
                for (int k = 0; k < UNPLANE_ROW_EPT; ++k) v[k] = base + k < RW ? (int)src[base + k] : 0;
            }
            short res[UNPLANE_ROW_EPT];
            if (C == 3) {
                unsigned a[3] = {0u, 0u, 0u}, q0, q1, q2;
#pragma unroll
                for (int k = 0; k < UNPLANE_ROW_EPT; ++k) a[k % 3] += (unsigned)v[k];
                const unsigned r = (unsigned)(base % 3), rinv = (3u - r) % 3u;
                rot3(r, a[0], a[1], a[2], q0, q1, q2);
                const unsigned i0 = wave_scan_incl(q0), i1 = wave_scan_incl(q1), i2 = wave_scan_incl(q2);
                unsigned p[3];   // by relative class: the sums in front of the thread's elements
                rot3(rinv, i0 - q0 + run[0], i1 - q1 + run[1], i2 - q2 + run[2], p[0], p[1], p[2]);
                run[0] += __shfl(i0, 63);
                run[1] += __shfl(i1, 63);
                run[2] += __shfl(i2, 63);
#pragma unroll
                for (int k = 0; k < UNPLANE_ROW_EPT; ++k) {
                    p[k % 3] += (unsigned)v[k];
                    res[k] = unplane_wrap9(p[k % 3]);
                }
            } else {
                unsigned q = 0u;
#pragma unroll
                for (int k = 0; k < UNPLANE_ROW_EPT; ++k) q += (unsigned)v[k];
                const unsigned incl = wave_scan_incl(q);
                unsigned pre = incl - q + run[0];
                run[0] += __shfl(incl, 63);
#pragma unroll
                for (int k = 0; k < UNPLANE_ROW_EPT; ++k) {
                    pre += (unsigned)v[k];
                    res[k] = unplane_wrap9(pre);
                }
            }
            if (RECON) {
                if (whole) {   // (a lane's group lies in the row or behind it)
                    short8 d;
#pragma unroll
                    for (int k = 0; k < UNPLANE_ROW_EPT; ++k) d[k] = res[k];
                    const size_t i = (row * (size_t)RW + (size_t)base) / 8;   // the group (C = 1: the pixel group) in the stack
                    const bool is_key = rc.key_mask[row / (size_t)rc.H] != 0;
                    if (C == 3) ((uint2*)rc.out)[i] = recon8_flat(rc.pred, (const uint2*)rc.key, is_key, i, d);
                    else recon8_gray(rc.pred, (const uint2*)rc.key, is_key, i, d, (uint2*)rc.out);
                }
            } else if (whole) {
                short8 o;
#pragma unroll
                for (int k = 0; k < UNPLANE_ROW_EPT; ++k) o[k] = res[k];
                *(short8*)(dst + base) = o;
            } else {
#pragma unroll
                for (int k = 0; k < UNPLANE_ROW_EPT; ++k)
                    if (base + k < RW) dst[base + k] = res[k];
            }
        }
    }
}

// nframes x H x W x C elements at `in` -> the delta stack at `out` (any 2-byte alignment; h_lut2112 NULL = symbols as stored).
// recon (may be NULL; the caller has checked k_unplane_rows<.., true>'s conditions): `out` is scratch for pass one, and pass two
// writes the frames to recon->out.
static int unplane_launch(tz_ctx* ctx, const int16_t* in, int nframes, int H, int W, int C, const int16_t* h_lut2112, int post_offset,
                          int16_t* out, const PlaneRecon* recon) {
    if (nframes < 0 || H < 1 || W < 1 || (C != 1 && C != 3) || (size_t)W * C > 0x3FFFFFFFull)
        return tz_fail(ctx, TZ_ERR_INVALID, "spatial_undelta_plane: %d frames of %d x %d x %d", nframes, H, W, C);
    if (nframes == 0) return TZ_OK;
    const uintptr_t both = (uintptr_t)in | (uintptr_t)out;
    if (both & 1) return tz_fail(ctx, TZ_ERR_INVALID, "spatial_undelta_plane buffers must be 2-byte aligned");
    const int RW = W * C;
    void* d_lut;
    TZ_TRY(upload_dec_lut(ctx, h_lut2112, &d_lut));
    tz_prof_scope ps(ctx, TZP_SCAN);
    const int band_rows = std::max(UNPLANE_BAND_ROWS, (H + 3) / 4);
    const bool v4 = RW % 4 == 0 && (both & 7) == 0;
    const dim3 grid((unsigned)((RW + (v4 ? 256 : 64) - 1) / (v4 ? 256 : 64)), (unsigned)std::min(nframes, 65535));
#define TZ_UNPLANE_COLS(L, V) \
    hipLaunchKernelGGL((k_unplane_cols<L, V>), grid, dim3(256), 0, ctx->stream, in, nframes, H, RW, band_rows, (const int16_t*)d_lut, post_offset, out)
    if (h_lut2112 && v4) TZ_UNPLANE_COLS(true, 4);
    else if (h_lut2112) TZ_UNPLANE_COLS(true, 1);
    else if (v4) TZ_UNPLANE_COLS(false, 4);
    else TZ_UNPLANE_COLS(false, 1);
#undef TZ_UNPLANE_COLS
    TZ_HIP(ctx, hipGetLastError());
    const size_t nrows = (size_t)nframes * H;
    const int vec = RW % 8 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 rgrid((unsigned)std::min<size_t>((nrows + 3) / 4, (size_t)kCUs * kBlocksPerCU));
    const PlaneRecon rc = recon ? *recon : PlaneRecon{};
#define TZ_UNPLANE_ROWS(CV, R) hipLaunchKernelGGL((k_unplane_rows<CV, R>), rgrid, dim3(256), 0, ctx->stream, (const int16_t*)out, nrows, RW, vec, out, rc)
    if (recon && !vec) return tz_fail(ctx, TZ_ERR_INVALID, "spatial_undelta_plane: the fused reconstruct needs rows of whole 16-byte groups");
    if (C == 3 && recon) TZ_UNPLANE_ROWS(3, true);
    else if (C == 3) TZ_UNPLANE_ROWS(3, false);
    else if (recon) TZ_UNPLANE_ROWS(1, true);
    else TZ_UNPLANE_ROWS(1, false);
#undef TZ_UNPLANE_ROWS
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_unplane(tz_ctx* ctx, const int16_t* in, int nframes, int H, int W, int C, const int16_t* h_lut2112, int post_offset, int16_t* out) {
    return unplane_launch(ctx, in, nframes, H, W, C, h_lut2112, post_offset, out, nullptr);
}

// the decoder's tail over frames [first, first + nframes) of a stream (tz_decode, tz_decode_range, tz_encode_quality): `in`,
// pred, key and d_key_mask point at the range's first frame and `carry` holds the layout.stride decoded elements in front of it (NULL
// at the stream start).  One launch (inverse remap when there is a table, inverse spatial delta, reconstruct) where the
// layout allows it: unpadded frames of a multiple of 16 elements, 16-byte aligned buffers, and no TEZIP_DECODE_UNFUSED.
// Else, and for the gray and the channel-stride layout always, a scan into a temporary and k_recon* / k_recon_gray*.  The plane
// layout (TZ-SD2): k_unplane_cols into a temporary, then k_unplane_rows -- with the reconstruct fused where the frames allow it.
int tzk_decode_tail(tz_ctx* ctx, tz_layout layout, const int16_t* in, const int16_t* h_lut2112, int post_offset, const int16_t* carry,
                    const float* pred, const uint8_t* key, const uint8_t* d_key_mask, int nframes, int H, int W, int Hp, int Wp,
                    uint8_t* out) {
    const size_t fe = tz_frame_elems(layout, H, W), n = (size_t)nframes * fe;
    if (n == 0) return TZ_OK;
    if (layout.channels == 3 && layout.stride == 1 && !layout.plane_h && H == Hp && W == Wp && fe % SCAN_EPT == 0 && key && !ctx->decode_unfused &&
        ((((uintptr_t)in | (uintptr_t)pred | (uintptr_t)key | (uintptr_t)out) & 15) == 0)) {
        const ScanRecon rc = {(const float4*)pred, key, d_key_mask, (unsigned long long)fe, out};
        return scan_launch(ctx, in, n, carry != nullptr, carry ? carry[0] : (int16_t)0, h_lut2112, post_offset, nullptr, &rc);
    }
    void* d_diff;
    TZ_TRY(tz_pool_alloc(ctx, n * 2, &d_diff));
    if (layout.plane_h) {   // TZ-SD2: every frame on its own, no carry
        if (carry) return tz_fail(ctx, TZ_ERR_INVALID, "the plane payload takes no carry");
        // unpadded frames whose rows are whole 16-byte groups, aligned buffers, no TEZIP_DECODE_UNFUSED: pass two reconstructs
        if (H == Hp && W == Wp && ((size_t)W * layout.channels) % 8 == 0 && key && !ctx->decode_unfused &&
            ((((uintptr_t)d_diff | (uintptr_t)pred) & 15) | (((uintptr_t)key | (uintptr_t)out) & 7)) == 0) {
            const PlaneRecon rc = {(const float4*)pred, key, d_key_mask, H, out};
            return unplane_launch(ctx, in, nframes, H, W, layout.channels, h_lut2112, post_offset, (int16_t*)d_diff, &rc);
        }
        TZ_TRY(tzk_unplane(ctx, in, nframes, H, W, layout.channels, h_lut2112, post_offset, (int16_t*)d_diff));
    } else {
        TZ_TRY(tzk_undelta(ctx, layout.stride, in, n, carry, h_lut2112, post_offset, (int16_t*)d_diff));
    }
    return tzk_reconstruct(ctx, layout.channels, pred, key, d_key_mask, (const int16_t*)d_diff, nframes, H, W, Hp, Wp, out);
}

// ------------------------------------------------------------------------ reconstruction statistics
// tz_encode_quality: per frame f of two unpadded uint8 stacks (the originals and what the decoder's tail makes of the
// stored payload) sse = sum (dec - orig)^2, max |dec - orig| and #(dec != orig), as exact integers.  Streaming, 2 B read
// per element: a workgroup owns a contiguous range of whole tiles (256 lanes x one 16-byte load of each stack), cut
// without regard to frame boundaries so that small frames still fill the chip.  The running sums belong to one frame;
// where a tile crosses the frame's end the lanes add the part in front of the boundary, the workgroup flushes (shuffle
// reduction per wave, LDS across the four waves, then ONE u64 add, u32 max and u32 add per frame it touched, agent
// scope) and carries on with the next frame.  A lane's loads of the next tile are issued before the current one is
// summed (two 16-byte loads of each stack in flight per lane).  Integer reductions: the records do not depend on the grid.  The elements
// in front of the first 16-byte boundary of `orig` (0..15) are added one by one by workgroup 0; stacks whose addresses
// differ modulo 16 take byte loads throughout (VEC = false).
static constexpr int QY_TILE = 256 * 16;   // elements per workgroup and step

struct QyPart {
    unsigned long long sse;
    unsigned mx, cnt;
};

__device__ __forceinline__ void qy_add(unsigned long long* sse, unsigned* mx, unsigned* cnt, tz_frame_quality* q) {
    __hip_atomic_fetch_add(&q->sse, *sse, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(&q->max_abs, *mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&q->n_changed, *cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every thread of the workgroup calls this (block-uniform control flow); q = the frame's record
__device__ __forceinline__ void qy_flush(unsigned long long sse, unsigned mx, unsigned cnt, QyPart* red, tz_frame_quality* q) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sse += __shfl_xor(sse, off, 64);
        mx = max(mx, (unsigned)__shfl_xor((int)mx, off, 64));
        cnt += (unsigned)__shfl_xor((int)cnt, off, 64);
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = QyPart{sse, mx, cnt};
    __syncthreads();
    if (threadIdx.x == 0) {
        sse = red[0].sse + red[1].sse + red[2].sse + red[3].sse;
        mx = max(max(red[0].mx, red[1].mx), max(red[2].mx, red[3].mx));
        cnt = red[0].cnt + red[1].cnt + red[2].cnt + red[3].cnt;
        if (sse != 0) qy_add(&sse, &mx, &cnt, q);   // (sse == 0: nothing changed, the record stays as cleared)
    }
    __syncthreads();   // red is written again by the next flush
}

// elements e .. e+15 of both stacks, packed 4 per word; 0 in both for those at or behind `end`
struct QyRaw {
    uint4 a, b;
};

template <bool VEC>
__device__ __forceinline__ QyRaw qy_fetch(const uint8_t* __restrict__ orig, const uint8_t* __restrict__ dec, size_t e, size_t end) {
    QyRaw r;
    if (VEC && e + 16 <= end) {
        r.a = *(const uint4*)(orig + e);
        r.b = *(const uint4*)(dec + e);
    } else {
        unsigned aw[4] = {0, 0, 0, 0}, bw[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (e + j < end) {
                aw[j >> 2] |= (unsigned)orig[e + j] << (8 * (j & 3));
                bw[j >> 2] |= (unsigned)dec[e + j] << (8 * (j & 3));
            }
        r.a = make_uint4(aw[0], aw[1], aw[2], aw[3]);
        r.b = make_uint4(bw[0], bw[1], bw[2], bw[3]);
    }
    return r;
}

// |dec - orig| per element
__device__ __forceinline__ void qy_absdiff(const QyRaw& r, unsigned ad[16]) {
    const unsigned aw[4] = {r.a.x, r.a.y, r.a.z, r.a.w}, bw[4] = {r.b.x, r.b.y, r.b.z, r.b.w};
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = (int)((bw[w] >> (8 * k)) & 0xffu) - (int)((aw[w] >> (8 * k)) & 0xffu);
            ad[4 * w + k] = (unsigned)(d < 0 ? -d : d);
        }
}

// per_block: elements per workgroup, a multiple of QY_TILE; tiles start at `head`
template <bool VEC>
__global__ __launch_bounds__(256) void k_quality(const uint8_t* __restrict__ orig, const uint8_t* __restrict__ dec, size_t n,
                                                 size_t fe, unsigned head, size_t per_block, tz_frame_quality* __restrict__ out) {
    __shared__ QyPart red[4];
    if (blockIdx.x == 0 && threadIdx.x < head) {   // in front of the first 16-byte boundary: element by element
        const size_t i = threadIdx.x;
        const int d = (int)dec[i] - (int)orig[i];
        if (d != 0) {
            unsigned long long s = (unsigned long long)(d * d);
            unsigned m = (unsigned)(d < 0 ? -d : d), c = 1;
            qy_add(&s, &m, &c, out + i / fe);
        }
    }
    const size_t b0 = head + (size_t)blockIdx.x * per_block;
    if (b0 >= n) return;   // (workgroup-uniform)
    const size_t b1 = min(n, b0 + per_block);
    size_t f = b0 / fe;                          // the frame the running sums belong to
    unsigned long long sse = 0;
    unsigned mx = 0, cnt = 0;
    QyRaw cur = qy_fetch<VEC>(orig, dec, b0 + (size_t)threadIdx.x * 16, min(b1, b0 + (size_t)QY_TILE));
    for (size_t t = b0; t < b1; t += QY_TILE) {
        const size_t tend = min(b1, t + (size_t)QY_TILE), e = t + (size_t)threadIdx.x * 16;
        QyRaw nxt{};   // the next tile's loads are in flight while this one is summed
        if (tend < b1) nxt = qy_fetch<VEC>(orig, dec, e + QY_TILE, min(b1, tend + (size_t)QY_TILE));
        unsigned ad[16];
        qy_absdiff(cur, ad);
        cur = nxt;
        for (size_t lo = t;;) {                  // segments [lo, lim) of the tile inside frame f
            const size_t bnd = (f + 1) * fe, lim = min(bnd, tend);
            unsigned s = 0, m = 0, c = 0;        // (16 x 255^2 fits)
            if (lo == t && lim == tend) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    s += ad[j] * ad[j];
                    m = max(m, ad[j]);
                    c += ad[j] != 0;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const unsigned v = (e + j >= lo && e + j < lim) ? ad[j] : 0u;
                    s += v * v;
                    m = max(m, v);
                    c += v != 0;
                }
            }
            sse += s;
            mx = max(mx, m);
            cnt += c;
            if (lim < bnd) break;                // frame f goes on behind this tile
            qy_flush(sse, mx, cnt, red, out + f);
            sse = 0;
            mx = cnt = 0;
            ++f;
            lo = lim;
            if (lo >= tend) break;
        }
    }
    if (f * fe < n) qy_flush(sse, mx, cnt, red, out + f);
}

int tzk_quality(tz_ctx* ctx, const uint8_t* orig, const uint8_t* dec, int nframes, size_t fe, tz_frame_quality* d_out) {
    if (nframes <= 0 || fe == 0) return TZ_OK;
    const size_t n = (size_t)nframes * fe;
    TZ_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(tz_frame_quality) * nframes, ctx->stream));
    const bool vec = (((uintptr_t)orig ^ (uintptr_t)dec) & 15) == 0;
    const unsigned head = vec ? (unsigned)std::min<size_t>(n, (16 - ((uintptr_t)orig & 15)) & 15) : 0u;
    const size_t tiles = std::max<size_t>(1, (n - head + QY_TILE - 1) / QY_TILE);
    size_t G = ctx->quality_grid > 0 ? (size_t)ctx->quality_grid : (size_t)grid_for(tiles, 1);
    G = std::max<size_t>(1, std::min(G, tiles));
    const size_t per_block = (tiles + G - 1) / G * QY_TILE;
    G = std::max<size_t>(1, (n - head + per_block - 1) / per_block);   // (no workgroup without a tile)
    tz_prof_scope ps(ctx, TZP_QUALITY);
    if (vec)
        hipLaunchKernelGGL(k_quality<true>, dim3((unsigned)G), dim3(256), 0, ctx->stream, orig, dec, n, fe, head, per_block, d_out);
    else
        hipLaunchKernelGGL(k_quality<false>, dim3((unsigned)G), dim3(256), 0, ctx->stream, orig, dec, n, fe, head, per_block, d_out);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------------------------- bound-map check (TZ-BM1)
// tz_map_check / tz_encode_map_check (slow statement: tezip_amd/boundmap.py check): per frame of two unpadded uint8 stacks the
// number of samples with |dec - orig| > M[pixel] and the largest max(|dec - orig| - M[pixel], 0).  A workgroup owns a run of
// pixels of ONE frame (grid.y), a thread a pixel at a time: 7 B read per pixel, the map's byte from cache.  Exact integers per
// thread, per wave, per workgroup, then one atomic pair per workgroup that found something, as k_quality.
__global__ __launch_bounds__(256) void k_map_check(const uint8_t* __restrict__ orig, const uint8_t* __restrict__ dec,
                                                   const uint8_t* __restrict__ map, size_t HW, tz_map_record* __restrict__ out) {
    __shared__ unsigned long long red_n[4];
    __shared__ unsigned red_x[4];
    const size_t f = blockIdx.y, fe0 = f * HW * 3;
    unsigned long long nv = 0;
    unsigned mx = 0;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (size_t)gridDim.x * 256) {
        const int m = map[p];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int d = (int)dec[fe0 + 3 * p + c] - (int)orig[fe0 + 3 * p + c];
            const int x = (d < 0 ? -d : d) - m;
            nv += x > 0;
            mx = max(mx, (unsigned)max(x, 0));
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        nv += __shfl_xor(nv, off, 64);
        mx = max(mx, (unsigned)__shfl_xor((int)mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        red_n[threadIdx.x >> 6] = nv;
        red_x[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        nv = red_n[0] + red_n[1] + red_n[2] + red_n[3];
        mx = max(max(red_x[0], red_x[1]), max(red_x[2], red_x[3]));
        if (nv != 0) {   // (nothing found: the record stays as cleared)
            __hip_atomic_fetch_add(&out[f].violations, nv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&out[f].max_excess, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

int tzk_map_check(tz_ctx* ctx, const uint8_t* orig, const uint8_t* dec, const uint8_t* d_map, int nframes, int H, int W,
                  tz_map_record* d_out) {
    if (nframes <= 0 || H <= 0 || W <= 0) return TZ_OK;
    const size_t HW = (size_t)H * W;
    TZ_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(tz_map_record) * nframes, ctx->stream));
    // enough workgroups per frame to fill the chip over the whole stack, none without a pixel
    const size_t want = std::max<size_t>(1, (size_t)(4 * kCUs + nframes - 1) / nframes);
    const unsigned gx = (unsigned)std::min(want, (HW + 255) / 256);
    tz_prof_scope ps(ctx, TZP_QUALITY);
    for (int f0 = 0; f0 < nframes; f0 += 65535) {   // (grid.y holds 65535 frames)
        const int nf = std::min(65535, nframes - f0);
        hipLaunchKernelGGL(k_map_check, dim3(gx, (unsigned)nf), dim3(256), 0, ctx->stream, orig + (size_t)f0 * HW * 3,
                           dec + (size_t)f0 * HW * 3, d_map, HW, d_out + f0);
    }
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------------------------- error of a candidate bound
// tz_bound_probe / tz_bound_err (TZ-TPSNR-1; slow statement in tezip_amd/target.py errors_of): what
// tz_encode_quality would report for a quantised delta stack, without a decoded stack in memory.  Per element of the
// unpadded stacks orig (uint8), d (the deltas of tzk_delta) and q (d behind the quantiser):
//   xh = orig + d  (the integer prediction the decoder reconstructs from; a masked frame has d = q = 0, and there the
//                   decoder's base is the key byte = orig, the same sum),  r = clamp(xh - q, 0, 255)  (k_recon),  e = r - orig
// and per frame sum e^2, max |e| and #(e != 0): k_recon plus k_quality in one pass, 5 B read per element and nothing
// written but the records.  Shaped like k_quality, whose records and flush it shares: a workgroup owns a contiguous run of
// whole tiles (256 lanes x 8 elements: one 16-byte load of d and of q, one 8-byte load of orig), cut without regard to
// frame boundaries; the next tile's loads are in flight while the current one is summed; where a tile crosses a frame's end
// the workgroup flushes (qy_flush: shuffle, LDS, one set of relaxed agent-scope atomics per frame it touched).  Tiles start
// at the first element `head` at which orig is 8-byte and d and q are 16-byte aligned; workgroup 0 adds the elements in
// front of it one by one; stacks that share no such element take element loads throughout (VEC = false).  A lane's
// loads are whole or, at the end of the run, element by element under `end`: nothing outside the stacks is read.
// GRAY: the records of a one-channel payload (tz_set_payload_channels(1)), whose decoder reconstructs channel 0 and writes
// the sample to all three channels (k_recon_gray) of a frame whose originals have three equal channels: the error of every
// channel is channel 0's, so only the elements with index % 3 == 0 count (fe is a multiple of 3: a frame starts a pixel),
// and their squares and their count go in three times.
static constexpr int BE_TILE = 256 * 8;   // elements per workgroup and step

// elements e .. e+7: orig packed 4 per word, d and q 2 per word; 0 in all three for those at or behind `end`
struct BeRaw {
    uint4 d, q;
    uint2 o;
};

template <bool VEC>
__device__ __forceinline__ BeRaw be_fetch(const uint8_t* __restrict__ orig, const int16_t* __restrict__ d, const int16_t* __restrict__ q,
                                          size_t e, size_t end) {
    BeRaw r;
    if (VEC && e + 8 <= end) {
        r.o = *(const uint2*)(orig + e);
        r.d = *(const uint4*)(d + e);
        r.q = *(const uint4*)(q + e);
    } else {
        unsigned ow[2] = {0, 0}, dw[4] = {0, 0, 0, 0}, qw[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (e + j < end) {
                ow[j >> 2] |= (unsigned)orig[e + j] << (8 * (j & 3));
                dw[j >> 1] |= (unsigned)(unsigned short)d[e + j] << (16 * (j & 1));
                qw[j >> 1] |= (unsigned)(unsigned short)q[e + j] << (16 * (j & 1));
            }
        r.o = make_uint2(ow[0], ow[1]);
        r.d = make_uint4(dw[0], dw[1], dw[2], dw[3]);
        r.q = make_uint4(qw[0], qw[1], qw[2], qw[3]);
    }
    return r;
}

// one element: |clamp(orig + d - q, 0, 255) - orig|
__device__ __forceinline__ unsigned be_abs1(int o, int d, int q) {
    int r = o + d - q;
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    const int e = r - o;
    return (unsigned)(e < 0 ? -e : e);
}

// e: the stack index of the lane's first element (GRAY: elements of channels 1 and 2 give 0)
template <bool GRAY>
__device__ __forceinline__ void be_abserr(const BeRaw& r, size_t e, unsigned ad[8]) {
    const unsigned ow[2] = {r.o.x, r.o.y}, dw[4] = {r.d.x, r.d.y, r.d.z, r.d.w}, qw[4] = {r.q.x, r.q.y, r.q.z, r.q.w};
#pragma unroll
    for (int j = 0; j < 8; ++j)
        ad[j] = be_abs1((int)((ow[j >> 2] >> (8 * (j & 3))) & 0xffu), (int)(short)(dw[j >> 1] >> (16 * (j & 1))),
                        (int)(short)(qw[j >> 1] >> (16 * (j & 1))));
    if (GRAY) {
        const unsigned c0 = (unsigned)(e % 3);   // channel of element e
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if ((c0 + j) % 3 != 0) ad[j] = 0;
    }
}

// per_block: elements per workgroup, a multiple of BE_TILE; tiles start at `head`
template <bool VEC, bool GRAY>
__global__ __launch_bounds__(256) void k_bound_err(const uint8_t* __restrict__ orig, const int16_t* __restrict__ d,
                                                   const int16_t* __restrict__ q, size_t n, size_t fe, unsigned head, size_t per_block,
                                                   tz_frame_quality* __restrict__ out) {
    __shared__ QyPart red[4];
    constexpr unsigned WT = GRAY ? 3 : 1;           // how often an element that counts is counted
    if (blockIdx.x == 0 && threadIdx.x < head) {   // in front of the first aligned element: one by one
        const size_t i = threadIdx.x;
        const unsigned a = (GRAY && i % 3 != 0) ? 0u : be_abs1((int)orig[i], (int)d[i], (int)q[i]);
        if (a != 0) {
            unsigned long long s = (unsigned long long)(a * a * WT);
            unsigned m = a, c = WT;
            qy_add(&s, &m, &c, out + i / fe);
        }
    }
    const size_t b0 = head + (size_t)blockIdx.x * per_block;
    if (b0 >= n) return;   // (workgroup-uniform)
    const size_t b1 = min(n, b0 + per_block);
    size_t f = b0 / fe;                          // the frame the running sums belong to
    unsigned long long sse = 0;
    unsigned mx = 0, cnt = 0;
    BeRaw cur = be_fetch<VEC>(orig, d, q, b0 + (size_t)threadIdx.x * 8, min(b1, b0 + (size_t)BE_TILE));
    for (size_t t = b0; t < b1; t += BE_TILE) {
        const size_t tend = min(b1, t + (size_t)BE_TILE), e = t + (size_t)threadIdx.x * 8;
        BeRaw nxt{};   // the next tile's loads are in flight while this one is summed
        if (tend < b1) nxt = be_fetch<VEC>(orig, d, q, e + BE_TILE, min(b1, tend + (size_t)BE_TILE));
        unsigned ad[8];
        be_abserr<GRAY>(cur, e, ad);
        cur = nxt;
        for (size_t lo = t;;) {                  // segments [lo, lim) of the tile inside frame f
            const size_t bnd = (f + 1) * fe, lim = min(bnd, tend);
            unsigned s = 0, m = 0, c = 0;        // (8 x 255^2 fits)
            if (lo == t && lim == tend) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    s += ad[j] * ad[j];
                    m = max(m, ad[j]);
                    c += ad[j] != 0;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned v = (e + j >= lo && e + j < lim) ? ad[j] : 0u;
                    s += v * v;
                    m = max(m, v);
                    c += v != 0;
                }
            }
            sse += s * WT;
            mx = max(mx, m);
            cnt += c * WT;
            if (lim < bnd) break;                // frame f goes on behind this tile
            qy_flush(sse, mx, cnt, red, out + f);
            sse = 0;
            mx = cnt = 0;
            ++f;
            lo = lim;
            if (lo >= tend) break;
        }
    }
    if (f * fe < n) qy_flush(sse, mx, cnt, red, out + f);
}

int tzk_bound_err(tz_ctx* ctx, int channels, const uint8_t* orig, const int16_t* d, const int16_t* q, int nframes, size_t fe,
                  tz_frame_quality* d_out) {
    if (nframes <= 0 || fe == 0) return TZ_OK;
    if (channels == 1 && fe % 3) return tz_fail(ctx, TZ_ERR_INVALID, "frames of %zu elements: a one-channel payload describes whole pixels", fe);
    const size_t n = (size_t)nframes * fe;
    TZ_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(tz_frame_quality) * nframes, ctx->stream));
    const unsigned h = (unsigned)((8 - ((uintptr_t)orig & 7)) & 7);   // the first element at which orig is 8-byte aligned
    const bool vec = ((((uintptr_t)d + 2 * h) | ((uintptr_t)q + 2 * h)) & 15) == 0;
    const unsigned head = vec ? (unsigned)std::min<size_t>(n, h) : 0u;
    const size_t tiles = std::max<size_t>(1, (n - head + BE_TILE - 1) / BE_TILE);
    size_t G = std::min<size_t>((size_t)grid_for(tiles, 1), tiles);
    const size_t per_block = (tiles + G - 1) / G * BE_TILE;
    G = std::max<size_t>(1, (n - head + per_block - 1) / per_block);   // (no workgroup without a tile)
    tz_prof_scope ps(ctx, TZP_QUALITY);
#define TZ_BE_LAUNCH(V, GR) \
    hipLaunchKernelGGL((k_bound_err<V, GR>), dim3((unsigned)G), dim3(256), 0, ctx->stream, orig, d, q, n, fe, head, per_block, d_out)
    if (vec && channels == 1) TZ_BE_LAUNCH(true, true);
    else if (vec) TZ_BE_LAUNCH(true, false);
    else if (channels == 1) TZ_BE_LAUNCH(false, true);
    else TZ_BE_LAUNCH(false, false);
#undef TZ_BE_LAUNCH
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------------------------------------ frame digests
// TZD64 version 1 (slow statement in tezip_amd/digest.py): per frame of an unpadded uint8 stack the
// sum mod 2^64 over its bytes of mix(256 * i + x[i]), i the byte's position inside ITS frame and mix splitmix64's output
// function.  An error-detection code, not a cryptographic hash.  The sum is commutative, so any cut of a frame over lanes,
// waves and workgroups gives the same 64 bits.  Streaming, 1 B read per element, shaped like k_quality: a workgroup owns a
// contiguous run of whole tiles (256 lanes x one 16-byte load), cut without regard to frame boundaries; the running sum
// belongs to one frame, and where a tile crosses the frame's end the workgroup flushes (shuffle reduction per wave, LDS
// across the four waves, then ONE relaxed u64 add per frame it touched, agent scope -- the kernel's only global atomic) and
// carries on with the next frame.  Tiles are laid over the stack from the 16-byte boundary at or in front of its first
// byte: positions are v = element index + pre (pre = address mod 16), so every full lane is an aligned 16-byte load, and
// the lane that holds the bytes in front of the first boundary, like the one that holds the tail, loads byte by byte with
// every index checked against [pre, n + pre): nothing outside the stack is read.  frame_bytes < 2^32, so a position is
// 32 bits and a key 40; the 64-bit multiplies are what the compiler builds from 32-bit ones.
static constexpr int DG_TILE = 256 * 16;   // elements per workgroup and step

__device__ __forceinline__ unsigned long long dg_mix(unsigned long long k) {
    unsigned long long z = k + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// every thread of the workgroup calls this (block-uniform control flow); word = the frame's digest
__device__ __forceinline__ void dg_flush(unsigned long long sum, unsigned long long* red, unsigned long long* word) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        sum = red[0] + red[1] + red[2] + red[3];
        __hip_atomic_fetch_add(word, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();   // red is written again by the next flush
}

// positions v .. v+15, packed 4 per word; bytes outside [pre, end) are not read (and 0 here)
__device__ __forceinline__ uint4 dg_fetch(const uint8_t* __restrict__ x, unsigned pre, size_t v, size_t end) {
    if (v >= pre && v + 16 <= end) return *(const uint4*)(x + (v - pre));
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (v + j >= pre && v + j < end) w[j >> 2] |= (unsigned)x[v + j - pre] << (8 * (j & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// nv = n + pre positions; per_block: positions per workgroup, a multiple of DG_TILE
__global__ __launch_bounds__(256) void k_digest(const uint8_t* __restrict__ x, size_t nv, size_t fe, unsigned pre, size_t per_block,
                                                unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[4];
    const size_t b0 = (size_t)blockIdx.x * per_block;
    if (b0 >= nv) return;   // (workgroup-uniform)
    const size_t b1 = min(nv, b0 + per_block);
    size_t f = (max(b0, (size_t)pre) - pre) / fe;   // the frame the running sum belongs to
    unsigned long long sum = 0;
    uint4 cur = dg_fetch(x, pre, b0 + (size_t)threadIdx.x * 16, min(b1, b0 + (size_t)DG_TILE));
    for (size_t t = b0; t < b1; t += DG_TILE) {
        const size_t tend = min(b1, t + (size_t)DG_TILE), e = t + (size_t)threadIdx.x * 16;
        uint4 nxt = make_uint4(0, 0, 0, 0);   // the next tile's load is in flight while this one is mixed
        if (tend < b1) nxt = dg_fetch(x, pre, e + DG_TILE, min(b1, tend + (size_t)DG_TILE));
        const unsigned w[4] = {cur.x, cur.y, cur.z, cur.w};
        cur = nxt;
        for (size_t lo = max(t, (size_t)pre);;) {   // segments [lo, lim) of the tile inside frame f
            const size_t fs = f * fe + pre, bnd = fs + fe, lim = min(bnd, tend);
            if (e >= lo && e + 16 <= lim) {          // the lane's 16 bytes lie inside the segment
                const unsigned p0 = (unsigned)(e - fs);
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    sum += dg_mix(((unsigned long long)(p0 + j) << 8) | ((w[j >> 2] >> (8 * (j & 3))) & 0xffu));
            } else if (e + 16 > lo && e < lim) {     // some of them do
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (e + j >= lo && e + j < lim)
                        sum += dg_mix(((unsigned long long)(unsigned)(e + j - fs) << 8) | ((w[j >> 2] >> (8 * (j & 3))) & 0xffu));
            }
            if (lim < bnd) break;                    // frame f goes on behind this tile
            dg_flush(sum, red, out + f);
            sum = 0;
            ++f;
            lo = lim;
            if (lo >= tend) break;
        }
    }
    if (f * fe + pre < b1) dg_flush(sum, red, out + f);   // (the frame began inside this run and goes on behind it)
}

int tzk_digest(tz_ctx* ctx, const uint8_t* x, int nframes, size_t fe, unsigned long long* d_out) {
    if (nframes <= 0) return TZ_OK;
    if (fe >> 32) return tz_fail(ctx, TZ_ERR_INVALID, "frames of %zu bytes: a digest covers fewer than 2^32", fe);
    TZ_HIP(ctx, hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * nframes, ctx->stream));
    if (fe == 0) return TZ_OK;   // (the digest of no bytes)
    const unsigned pre = (unsigned)((uintptr_t)x & 15);
    const size_t nv = (size_t)nframes * fe + pre;
    const size_t tiles = (nv + DG_TILE - 1) / DG_TILE;
    size_t G = ctx->digest_grid > 0 ? (size_t)ctx->digest_grid : (size_t)grid_for(tiles, 1);
    G = std::max<size_t>(1, std::min(G, tiles));
    const size_t per_block = (tiles + G - 1) / G * DG_TILE;
    G = (nv + per_block - 1) / per_block;   // (no workgroup without a tile)
    tz_prof_scope ps(ctx, TZP_DIGEST);
    hipLaunchKernelGGL(k_digest, dim3((unsigned)G), dim3(256), 0, ctx->stream, x, nv, fe, pre, per_block, d_out);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------------------------------------ structural similarity
// TZ-SSIM-1 (include/tezip_hip.h, DESIGN.md section 9, slow statement in tezip_amd/ssim.py): per frame of two unpadded uint8
// stacks the sum and the minimum of the integer Q of every 8 x 8 window (stride 4, per channel).  A window is 2 x 2 CELLS of
// 4 x 4 pixels, so the five moments are formed once per cell and summed four at a time.
// A workgroup walks a contiguous run of TILES; a tile is SS_T x SS_T window origins of one frame, i.e. (SS_T + 1)^2 = 256 cells,
// one per lane: 64 x 64 pixels, of which the last 4 columns and rows are the apron that the neighbouring tiles read again
// (a 16 x 16 tile of origins has 289 cells and a second, nearly empty pass over them: measured 79 us against 65 us on cfg3's job).
//   phase 1: a lane forms one cell: 4 rows of 12 bytes of each stack (ss_row12), 15 integer moments, one 16-byte record per
//            channel into LDS: {s1 | s2 << 16, sa, sb, s12} (s1, s2 <= 16 * 255; the others < 2^21).
//   phase 2: a lane per window origin (225 of the 256) reads the four records of each channel (consecutive lanes read
//            consecutive 16-byte records, a row of 15 lanes skips one record of the 16-record pitch), forms
//            the four int64 factors and evaluates Q: two fp64 multiplies, ONE correctly rounded fp64 division, a multiply
//            by 2^32 (exact) and rint (half to even) -- no other floating-point operation, -ffp-contract=off.
// The running sum and minimum belong to one frame; where the run of tiles moves on to the next frame, and at its end, the
// workgroup flushes: shuffle reduction per wave, LDS across the four waves, then ONE 64-bit add and ONE signed 64-bit min per
// frame it touched (relaxed, agent scope).  Integer reductions: the records do not depend on the grid (TEZIP_SSIM_GRID).
// k_ssim_init writes the records first: sum 0, min INT64_MAX (0 for frames without a window), the window count, reserved 0.
static constexpr int SS_T = 15;                       // window origins per tile side
static constexpr int SS_C = SS_T + 1;                 // cells per tile side
static constexpr int SS_CELLS = SS_C * SS_C;

struct SsPart {
    long long sum, mn;
};

__device__ __forceinline__ long long ss_min(long long x, long long y) { return y < x ? y : x; }

// Q of one window from its five moments (exact integers; every factor below 2^53 in magnitude, d1, d2 > 0)
__device__ __forceinline__ long long ss_q(long long s1, long long s2, long long sa, long long sb, long long s12) {
    const long long n1 = 200 * s1 * s2 + 2663424;
    const long long n2 = 200 * (64 * s12 - s1 * s2) + 23970816;
    const long long d1 = 100 * (s1 * s1 + s2 * s2) + 2663424;
    const long long d2 = 100 * (64 * (sa + sb) - s1 * s1 - s2 * s2) + 23970816;
    const double p = (double)n1 * (double)n2;
    const double q = (double)d1 * (double)d2;
    const double r = p / q;
    return (long long)__builtin_rint(r * 4294967296.0);   // |r * 2^32| < 2^34: the conversion is exact
}

// every thread of the workgroup calls this (block-uniform control flow); rec = the frame's record
__device__ __forceinline__ void ss_flush(long long sum, long long mn, SsPart* red, tz_frame_ssim* rec) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        mn = ss_min(mn, __shfl_xor(mn, off, 64));
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = SsPart{sum, mn};
    __syncthreads();
    if (threadIdx.x == 0) {
        sum = red[0].sum + red[1].sum + red[2].sum + red[3].sum;
        mn = ss_min(ss_min(red[0].mn, red[1].mn), ss_min(red[2].mn, red[3].mn));
        __hip_atomic_fetch_add(&rec->sum_q32, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_min(&rec->min_q32, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();   // red is written again by the next flush
}

__global__ __launch_bounds__(256) void k_ssim_init(tz_frame_ssim* __restrict__ out, int nframes, unsigned windows) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < nframes) out[f] = tz_frame_ssim{0, windows ? INT64_MAX : 0, windows, 0u};
}

// CH x CW cells and (CH - 1) x (CW - 1) window origins per channel (CH = H / 4, CW = W / 4, both >= 2); TY x TX tiles per
// frame, ntiles in all; workgroup b walks tiles [b * per_block, (b + 1) * per_block)
__global__ __launch_bounds__(256) void k_ssim(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, size_t total, size_t fe,
                                              int W, int CH, int CW, int TY, int TX, size_t ntiles, size_t per_block,
                                              tz_frame_ssim* __restrict__ out) {
    __shared__ uint4 cell[3][SS_CELLS];
    __shared__ SsPart red[4];
    const size_t t0 = (size_t)blockIdx.x * per_block;
    if (t0 >= ntiles) return;   // (workgroup-uniform)
    const size_t t1 = min(ntiles, t0 + per_block), per_frame = (size_t)TY * TX;
    size_t f = t0 / per_frame;                    // the frame the running sum and minimum belong to
    long long sum = 0, mn = INT64_MAX;
    for (size_t t = t0; t < t1; ++t) {
        const size_t tf = t / per_frame;
        if (tf != f) {
            ss_flush(sum, mn, red, out + f);
            sum = 0;
            mn = INT64_MAX;
            f = tf;
        }
        const int rem = (int)(t - tf * per_frame), ty = rem / TX, tx = rem - ty * TX;
        // phase 1: the cells of the tile that lie inside the frame's cell grid
        for (int ci = threadIdx.x; ci < SS_CELLS; ci += 256) {
            const int ly = ci / SS_C, lx = ci - ly * SS_C, cy = ty * SS_T + ly, cx = tx * SS_T + lx;
            if (cy >= CH || cx >= CW) continue;
            unsigned s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0}, sa[3] = {0, 0, 0}, sb[3] = {0, 0, 0}, s12[3] = {0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t off = tf * fe + ((size_t)(cy * 4 + r) * W + (size_t)cx * 4) * 3;   // (< total: the cell lies inside the frame)
                unsigned wa[3], wb[3];
                ss_row12(a, off, total, wa);
                ss_row12(b, off, total, wb);
#pragma unroll
                for (int j = 0; j < 12; ++j) {
                    const unsigned av = (wa[j >> 2] >> (8 * (j & 3))) & 0xffu, bv = (wb[j >> 2] >> (8 * (j & 3))) & 0xffu;
                    const int c = j % 3;
                    s1[c] += av;
                    s2[c] += bv;
                    sa[c] += av * av;
                    sb[c] += bv * bv;
                    s12[c] += av * bv;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) cell[c][ci] = make_uint4(s1[c] | (s2[c] << 16), sa[c], sb[c], s12[c]);
        }
        __syncthreads();
        // phase 2: one window origin per lane, three channels
        {
            const int ly = threadIdx.x / SS_T, lx = threadIdx.x % SS_T, wy = ty * SS_T + ly, wx = tx * SS_T + lx;
            if (threadIdx.x < SS_T * SS_T && wy < CH - 1 && wx < CW - 1) {
                const int i00 = ly * SS_C + lx;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint4 q0 = cell[c][i00], q1 = cell[c][i00 + 1], q2 = cell[c][i00 + SS_C], q3 = cell[c][i00 + SS_C + 1];
                    const unsigned m1 = (q0.x & 0xffffu) + (q1.x & 0xffffu) + (q2.x & 0xffffu) + (q3.x & 0xffffu);
                    const unsigned m2 = (q0.x >> 16) + (q1.x >> 16) + (q2.x >> 16) + (q3.x >> 16);
                    const long long Q = ss_q((long long)m1, (long long)m2, (long long)(q0.y + q1.y + q2.y + q3.y),
                                             (long long)(q0.z + q1.z + q2.z + q3.z), (long long)(q0.w + q1.w + q2.w + q3.w));
                    sum += Q;
                    mn = ss_min(mn, Q);
                }
            }
        }
        __syncthreads();   // the cells are written again by the next tile
    }
    ss_flush(sum, mn, red, out + f);
}

// per-frame TZ-SSIM-1 records of two unpadded nframes x H x W x 3 uint8 stacks; d_out (device) is written whole here
int tzk_ssim(tz_ctx* ctx, const uint8_t* a, const uint8_t* b, int nframes, int H, int W, tz_frame_ssim* d_out) {
    if (nframes <= 0) return TZ_OK;
    const size_t fe = (size_t)H * W * 3;
    if (H <= 0 || W <= 0 || (fe >> 32)) return tz_fail(ctx, TZ_ERR_INVALID, "frames of %d x %d: SSIM covers frames of fewer than 2^32 bytes", H, W);
    const int CH = H / 4, CW = W / 4;
    const bool any = CH >= 2 && CW >= 2;
    const unsigned windows = any ? 3u * (unsigned)(CH - 1) * (unsigned)(CW - 1) : 0u;
    tz_prof_scope ps(ctx, TZP_QUALITY);
    hipLaunchKernelGGL(k_ssim_init, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0, ctx->stream, d_out, nframes, windows);
    TZ_HIP(ctx, hipGetLastError());
    if (!any) return TZ_OK;
    const int TY = (CH - 1 + SS_T - 1) / SS_T, TX = (CW - 1 + SS_T - 1) / SS_T;
    const size_t ntiles = (size_t)nframes * TY * TX;
    size_t G = ctx->ssim_grid > 0 ? (size_t)ctx->ssim_grid : (size_t)grid_for(ntiles, 1);
    G = std::max<size_t>(1, std::min(G, ntiles));
    const size_t per_block = (ntiles + G - 1) / G;
    G = (ntiles + per_block - 1) / per_block;   // (no workgroup without a tile)
    hipLaunchKernelGGL(k_ssim, dim3((unsigned)G), dim3(256), 0, ctx->stream, a, b, (size_t)nframes * fe, fe, W, CH, CW, TY, TX,
                       ntiles, per_block, d_out);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------------------------------------ window SSE
// compress.py:246: mean((X_test_pad - pred)^2) in float64 over PADDED frames.  Per frame the
// sum is taken in a fixed order so that it is reproducible: 4096-element blocks; thread t sums
// elements t, t+256, ... of its block; halving tree over the 256 partials; blocks are added
// in order on the host.  x = float32(k)/255 inside the image, 0 in the pad region.
__global__ __launch_bounds__(256) void k_sse(const uint8_t* __restrict__ orig, const float* __restrict__ pred, int H,
                                             int W, int Hp, int Wp, int nblk, double* __restrict__ partial) {
    __shared__ double s[256];
    const int f = blockIdx.y, b = blockIdx.x;
    const double t = tz_sse_block(orig + (size_t)f * H * W * 3, pred + (size_t)f * ((size_t)Hp * Wp * 3), H, W, Hp, Wp, b, s);
    if (threadIdx.x == 0) partial[(size_t)f * nblk + b] = t;
}

int tzk_sse_blocks(int Hp, int Wp) { return (int)(((size_t)Hp * Wp * 3 + 4095) / 4096); }

// launch only: per-block partial sums of nframes frames into d_part[nframes][tzk_sse_blocks]
int tzk_sse_launch(tz_ctx* ctx, const uint8_t* orig, const float* pred, int nframes, int H, int W, int Hp, int Wp,
                   double* d_part) {
    if (nframes <= 0) return TZ_OK;
    const int nblk = tzk_sse_blocks(Hp, Wp);
    tz_prof_scope ps(ctx, TZP_SSE);
    hipLaunchKernelGGL(k_sse, dim3(nblk, nframes), dim3(256), 0, ctx->stream, orig, pred, H, W, Hp, Wp, nblk, d_part);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_sse(tz_ctx* ctx, const uint8_t* orig, const float* pred, int nframes, int H, int W, int Hp, int Wp,
            double* h_sse) {
    if (nframes <= 0) return TZ_OK;
    const int nblk = tzk_sse_blocks(Hp, Wp);
    void* d_part;
    TZ_TRY(tz_pool_alloc(ctx, sizeof(double) * nblk * nframes, &d_part));
    TZ_TRY(tzk_sse_launch(ctx, orig, pred, nframes, H, W, Hp, Wp, (double*)d_part));
    std::vector<double> part((size_t)nblk * nframes);
    TZ_HIP(ctx, hipMemcpyAsync(part.data(), d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost, ctx->stream));
    TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int f = 0; f < nframes; ++f) {
        double t = 0.0;
        for (int b = 0; b < nblk; ++b) t = t + part[(size_t)f * nblk + b];
        h_sse[f] = t;
    }
    return TZ_OK;
}

// ---------------------------------------------------------------------------- Huffman coder
// Opt-in stage that is NOT in the reference (`--coder huff`; format: DESIGN.md section 9, tezip_amd/huff.py is the slow
// statement of it): an order-0 canonical Huffman code over the 16-bit payload symbols, lengths <= 12.  A RUN is 256
// consecutive symbols coded back to back by one lane, a CHUNK is 64 runs = one wave and starts on a 32-bit word, so no two
// waves ever write the same word of global memory.  Codes are stored bit-reversed from the least significant end, so the
// decoder looks up the next 12 bits of the stream in a 4096-entry table of symbol | length << 12.
static constexpr int HF_L = TZ_HUFF_L, HF_R = TZ_HUFF_RUN, HF_CR = TZ_HUFF_CHUNK_RUNS;
static constexpr int HF_CHUNK = HF_R * HF_CR;                  // symbols per chunk
static constexpr int HF_CHUNK_WORDS = HF_CHUNK * HF_L / 32;    // the most words a chunk can need (6144 = 24 KB of LDS)
static constexpr int HF_ENC_PAD = (TZ_NBINS + 7) & ~7;

// 8 consecutive payload elements from element e0 (elements at or behind n read as `fill`); VEC: in + e0 is 16-byte aligned
template <bool VEC>
__device__ __forceinline__ short8 hf_load8(const int16_t* __restrict__ in, size_t e0, size_t n, short fill) {
    short8 v;
    if (VEC && e0 + 8 <= n) return *(const short8*)(in + e0);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = e0 + k < n ? in[e0 + k] : fill;
    return v;
}

// exclusive prefix sum over the 64 lanes of a wave; *total = the wave's sum
__device__ __forceinline__ unsigned hf_wave_excl(unsigned v, unsigned* total) {
    const int lane = threadIdx.x & 63;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    *total = __shfl(inc, 63, 64);
    return inc - v;
}

// What the pack kernels (k_huff_enc, k_huffr_enc) share.  hf_enc_begin: the code table `enc` of nsym entries into tab[PAD],
// the bit offset of this lane's run inside the chunk (returned) and the chunk's size in words *cw, clamped to the image,
// whose first *cw words are cleared.  Ends with a barrier.
template <int PAD>
__device__ __forceinline__ unsigned hf_enc_begin(uint16_t* tab, unsigned* img, const uint16_t* __restrict__ enc, int nsym, size_t run, size_t nruns,
                                                 const uint16_t* __restrict__ run_bits, unsigned* cw) {
    const int lane = threadIdx.x;
    for (int k = lane; k < PAD; k += 64) tab[k] = k < nsym ? enc[k] : (uint16_t)0;
    unsigned tot;
    const unsigned pos = hf_wave_excl(run < nruns ? (unsigned)run_bits[run] : 0u, &tot);
    *cw = std::min((tot + 31u) >> 5, (unsigned)HF_CHUNK_WORDS);
    for (unsigned k = lane; k < *cw; k += 64) img[k] = 0;
    __syncthreads();
    return pos;
}

// a full word of the accumulator leaves for the image (the first and the last word of a run are shared with the
// neighbouring lanes: ds_or, no return value)
__device__ __forceinline__ void hf_flush(unsigned long long& acc, unsigned& nb, unsigned& wi, unsigned cw, unsigned* img) {
    if (nb >= 32) {
        if (wi < cw) atomicOr(&img[wi], (unsigned)acc);
        ++wi;
        acc >>= 32;
        nb -= 32;
    }
}

// the last, partial word of the run, then the image leaves with coalesced stores, clamped to the stream
__device__ __forceinline__ void hf_enc_end(unsigned long long acc, unsigned nb, unsigned wi, unsigned cw, unsigned* img,
                                           const unsigned* __restrict__ chunk_off, size_t chunk, unsigned* __restrict__ words, size_t stream_words) {
    if (nb > 0 && wi < cw) atomicOr(&img[wi], (unsigned)acc);
    __syncthreads();
    const size_t w0 = chunk_off[chunk];
    for (unsigned k = threadIdx.x; k < cw; k += 64)
        if (w0 + k < stream_words) words[w0 + k] = img[k];
}

// What the expand kernels (k_huff_dec, k_huffr_dec) share, and with it every clamp that makes a corrupt body harmless.
// hf_dec_begin: the decode table into tab, the chunk's words into img -- chunk offsets clamped to the stream, the staged
// words to the image, a zero word behind them at img[*cw] -- and this lane's bit offset from the run sizes, each clamped to
// R * L (returned).  Ends with a barrier.
__device__ __forceinline__ unsigned hf_dec_begin(uint16_t* tab, unsigned* img, const uint16_t* __restrict__ dec, const unsigned* __restrict__ chunk_off,
                                                 const uint16_t* __restrict__ run_bits, const unsigned* __restrict__ words, size_t stream_words,
                                                 size_t nruns, size_t nchunks, size_t chunk, size_t run, unsigned* cw_out) {
    const int lane = threadIdx.x;
    for (int k = lane; k < (1 << HF_L) / 8; k += 64) ((uint4*)tab)[k] = ((const uint4*)dec)[k];
    const size_t w0 = std::min((size_t)chunk_off[chunk], stream_words);
    const size_t w1 = chunk + 1 < nchunks ? std::min((size_t)chunk_off[chunk + 1], stream_words) : stream_words;
    const unsigned cw = w1 > w0 ? (unsigned)std::min(w1 - w0, (size_t)HF_CHUNK_WORDS) : 0u;
    for (unsigned k = lane; k < cw; k += 64) img[k] = words[w0 + k];
    if (lane == 0) img[cw] = 0;
    unsigned tot;
    const unsigned pos = hf_wave_excl(run < nruns ? std::min((unsigned)run_bits[run], (unsigned)(HF_R * HF_L)) : 0u, &tot);
    __syncthreads();
    *cw_out = cw;
    return pos;
}

// the first two words of the run that starts at bit `pos` of the image: nb valid bits in acc, more than 32; wi: the next word
__device__ __forceinline__ void hf_dec_first(const unsigned* img, unsigned pos, unsigned cw, unsigned long long& acc, unsigned& nb, unsigned& wi) {
    wi = pos >> 5;
    acc = (unsigned long long)img[std::min(wi, cw)] >> (pos & 31u);
    nb = 32u - (pos & 31u);
    ++wi;
    acc |= (unsigned long long)img[std::min(wi, cw)] << nb;
    nb += 32;
    ++wi;
}

// the next word of the image joins the accumulator once 32 bits or fewer are left; reads are clamped to the zero word
__device__ __forceinline__ void hf_refill(unsigned long long& acc, unsigned& nb, unsigned& wi, unsigned cw, const unsigned* img) {
    if (nb <= 32) {
        acc |= (unsigned long long)img[std::min(wi, cw)] << nb;
        nb += 32;
        ++wi;
    }
}

// elements j .. j + 7 of the run at r0 leave (those in front of cnt); VEC: out + r0 is 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void hf_store8(int16_t* __restrict__ out, size_t r0, int j, int cnt, short8 v) {
    if (VEC && j + 8 <= cnt) {
        *(short8*)(out + r0 + j) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (j + k < cnt) out[r0 + j + k] = v[k];
    }
}

// Counts of the payload values (bin = value + TZ_HUFF_COUNT_BIAS; anything outside the 4096 bins sets meta->bad): the
// histogram a payload has when no earlier pass left one (a payload without a rank table, a tz_encode_finish).  One read
// of the payload, 2 B/element; equal neighbours are merged in the thread before they reach the LDS counters.
__global__ __launch_bounds__(256) void k_huff_count(const int16_t* __restrict__ in, size_t n, unsigned long long* __restrict__ hist,
                                                    tz_huff_meta* __restrict__ meta) {
    __shared__ unsigned h[TZ_HUFF_COUNT_BINS];
    for (int k = threadIdx.x; k < TZ_HUFF_COUNT_BINS; k += 256) h[k] = 0;
    __syncthreads();
    const size_t n8 = (n + 7) / 8, stride = (size_t)gridDim.x * 256;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        const short8 v = hf_load8<true>(in, i * 8, n, (short)0);
        const int valid = (int)std::min((size_t)8, n - i * 8);
        int prev = v[0], cnt = 1;
#pragma unroll
        for (int k = 1; k <= 8; ++k) {
            const bool more = k < valid;
            if (more && v[k < 8 ? k : 7] == prev) {
                ++cnt;
                continue;
            }
            const int b = prev + TZ_HUFF_COUNT_BIAS;
            if (b >= 0 && b < TZ_HUFF_COUNT_BINS) atomicAdd(&h[b], (unsigned)cnt);
            else bad = true;
            if (!more) break;
            prev = v[k < 8 ? k : 7];
            cnt = 1;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < TZ_HUFF_COUNT_BINS; k += 256)
        if (h[k]) atomicAdd(&hist[k], (unsigned long long)h[k]);
    if (bad) atomicOr(&meta->bad, 1u);
}

int tzk_huff_count(tz_ctx* ctx, const int16_t* in, size_t n, unsigned long long* d_hist, tz_huff_meta* d_meta) {
    if ((uintptr_t)in & 15) return tz_fail(ctx, TZ_ERR_INVALID, "k_huff_count needs a 16-byte aligned payload");
    TZ_HIP(ctx, hipMemsetAsync(d_hist, 0, TZ_HUFF_COUNT_BINS * sizeof(unsigned long long), ctx->stream));
    TZ_HIP(ctx, hipMemsetAsync(d_meta, 0, sizeof(tz_huff_meta), ctx->stream));
    tz_prof_scope ps(ctx, TZP_HUFF);
    hipLaunchKernelGGL(k_huff_count, dim3(grid_for((n + 7) / 8, 256)), dim3(256), 0, ctx->stream, in, n, d_hist, d_meta);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// Size pass: one wave per chunk, four chunks per workgroup.  A 16-byte load per lane covers two runs per step (32 lanes x
// 8 symbols = one run), so the loads are fully coalesced; the 32 partial sums of a run meet in a butterfly.  run_bits[r]
// is the index's 16-bit entry of run r; chunk_bits[c] feeds k_huff_scan.
template <bool VEC>
__global__ __launch_bounds__(256) void k_huff_size(const int16_t* __restrict__ in, size_t n, const uint16_t* __restrict__ enc, int A,
                                                   int base, size_t nruns, size_t nchunks, uint16_t* __restrict__ run_bits,
                                                   unsigned* __restrict__ chunk_bits, tz_huff_meta* __restrict__ meta) {
    __shared__ uint8_t len[HF_ENC_PAD];
    for (int k = threadIdx.x; k < HF_ENC_PAD; k += 256) len[k] = k < A ? (uint8_t)(enc[k] >> 12) : 0;
    __syncthreads();
    const size_t chunk = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= nchunks) return;
    const int lane = threadIdx.x & 63;
    const size_t c0 = chunk * HF_CHUNK;
    unsigned mine = 0;
    bool bad = false;
    for (int j = 0; j < HF_CR / 2; ++j) {
        const size_t e0 = c0 + (size_t)j * 512 + (size_t)lane * 8;
        unsigned s = 0;
        if (e0 < n) {
            const short8 v = hf_load8<VEC>(in, e0, n, (short)0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const unsigned sym = (unsigned)((int)v[k] - base);
                const unsigned l = sym < (unsigned)A ? len[sym] : 0u;
                if (e0 + k < n) {
                    s += l;
                    bad |= l == 0;
                }
            }
        }
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        const size_t run = chunk * HF_CR + 2 * j + (lane >> 5);
        if ((lane & 31) == 0 && run < nruns) {
            run_bits[run] = (uint16_t)s;
            mine += s;
        }
    }
    mine += __shfl_xor(mine, 32, 64);
    if (lane == 0) chunk_bits[chunk] = mine;
    if (bad) atomicOr(&meta->bad, 1u);
}

// Chunk word offsets: exclusive scan of ceil(bits / 32) over the chunks (a few 10^4 values: one workgroup, each thread a
// contiguous slice, the 1024 slice sums scanned in LDS).
__global__ __launch_bounds__(1024) void k_huff_scan(const unsigned* __restrict__ chunk_bits, size_t nchunks, unsigned* __restrict__ chunk_off,
                                                    tz_huff_meta* __restrict__ meta) {
    __shared__ unsigned long long part[1024];
    const size_t per = (nchunks + 1023) / 1024, a = std::min(nchunks, (size_t)threadIdx.x * per), b = std::min(nchunks, a + per);
    unsigned long long s = 0;
    for (size_t c = a; c < b; ++c) s += (chunk_bits[c] + 31u) >> 5;
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned long long t = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += t;
        __syncthreads();
    }
    unsigned long long off = part[threadIdx.x] - s;
    for (size_t c = a; c < b; ++c) {
        chunk_off[c] = (unsigned)off;   // (the host refuses a stream of 2^32 words or more before anything reads these)
        off += (chunk_bits[c] + 31u) >> 5;
    }
    if (threadIdx.x == 1023) meta->total_words = part[1023];
}

// Pack pass: one wave (= one workgroup) per chunk.  Every lane packs its run into a 64-bit accumulator and ORs whole
// 32-bit words into the chunk's image in LDS (the first and the last word of a run are shared with the neighbouring
// lanes: ds_or, no return value); the image then leaves with coalesced stores.  No global atomics.
template <bool VEC>
__global__ __launch_bounds__(64) void k_huff_enc(const int16_t* __restrict__ in, size_t n, const uint16_t* __restrict__ enc, int A, int base,
                                                 size_t nruns, const uint16_t* __restrict__ run_bits, const unsigned* __restrict__ chunk_off,
                                                 unsigned* __restrict__ words, size_t stream_words) {
    __shared__ uint16_t tab[HF_ENC_PAD];
    __shared__ unsigned img[HF_CHUNK_WORDS];
    const size_t chunk = blockIdx.x, run = chunk * HF_CR + threadIdx.x;
    unsigned cw;
    const unsigned pos = hf_enc_begin<HF_ENC_PAD>(tab, img, enc, A, run, nruns, run_bits, &cw);
    const size_t r0 = run * HF_R;
    const int cnt = r0 < n ? (int)std::min((size_t)HF_R, n - r0) : 0;
    unsigned long long acc = 0;
    unsigned nb = pos & 31u, wi = pos >> 5;
    for (int j = 0; j < cnt; j += 8) {
        const short8 v = hf_load8<VEC>(in, r0 + j, n, (short)0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned sym = (unsigned)((int)v[k] - base);
            const unsigned e = (sym < (unsigned)A && j + k < cnt) ? tab[sym] : 0u;   // (no code: nothing is written; k_huff_size said so)
            acc |= (unsigned long long)(e & 0xFFFu) << nb;
            nb += e >> 12;
            hf_flush(acc, nb, wi, cw, img);
        }
    }
    hf_enc_end(acc, nb, wi, cw, img, chunk_off, chunk, words, stream_words);
}

// Expand pass: one wave (= one workgroup) per chunk.  The chunk's words are staged in LDS behind the decode table; every
// lane decodes its run from its own bit offset (exclusive wave scan of the run sizes) and writes 16-byte pieces of its 512
// output bytes.  Nothing taken from the stream becomes an address unchecked: chunk offsets are clamped to the stream, a
// chunk's staged words to the LDS image, every read of the image to its end (a zero word stands behind it), run sizes to
// R * L, and a lane stops after its run's symbol count, which comes from n alone.  Every table entry has a length >= 1
// and a symbol inside the alphabet (the host builds it from validated lengths), so a corrupt body yields wrong symbols,
// never an access outside the buffers.
template <bool VEC>
__global__ __launch_bounds__(64) void k_huff_dec(const unsigned* __restrict__ chunk_off, const uint16_t* __restrict__ run_bits,
                                                 const unsigned* __restrict__ words, size_t stream_words, size_t nruns, size_t nchunks,
                                                 const uint16_t* __restrict__ dec, int base, size_t n, int16_t* __restrict__ out) {
    __shared__ uint16_t tab[1 << HF_L];
    __shared__ unsigned img[HF_CHUNK_WORDS + 1];
    const size_t chunk = blockIdx.x, run = chunk * HF_CR + threadIdx.x;
    unsigned cw, nb, wi;
    unsigned long long acc;
    const unsigned pos = hf_dec_begin(tab, img, dec, chunk_off, run_bits, words, stream_words, nruns, nchunks, chunk, run, &cw);
    const size_t r0 = run * HF_R;
    const int cnt = r0 < n ? (int)std::min((size_t)HF_R, n - r0) : 0;
    hf_dec_first(img, pos, cw, acc, nb, wi);
    for (int j = 0; j < cnt; j += 8) {
        short8 v;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned e = tab[(unsigned)acc & 0xFFFu];
            const unsigned l = e >> 12;
            v[k] = (short)((int)(e & 0xFFFu) + base);
            acc >>= l;
            nb -= l;
            hf_refill(acc, nb, wi, cw, img);
        }
        hf_store8<VEC>(out, r0, j, cnt, v);
    }
}

// ---------------------------------------------------------------------------- Huffman coder with repeat tokens
// Opt-in stage `--coder huffr` (format TZR1: DESIGN.md section 9, tezip_amd/huffr.py is the slow statement of it).  The
// geometry is the Huffman coder's above -- a lane owns a run of 256 payload elements, a wave a chunk of 64 runs that starts
// on a word -- but a lane no longer codes one symbol per element: element j of a run MATCHES when j >= 3 and
// s[j] == s[j - 3] (the payload interleaves three channels, so a quantiser run repeats with period 3), every maximal
// stretch of m matches becomes the token T_k = symbol A + k, k = floor(log2 m), followed by k raw bits m - 2^k, and the
// other elements are literals.  The three encoder passes share ONE walk of a run (hfr_walk), so the histogram, the sizes
// and the packed bits cannot disagree about the tokens.  The walk is uniform over the lanes of a wave: every lane takes
// one element per step, and what a step emits is predicated.
static constexpr int HFR_NTOK = TZ_HUFFR_NTOK, HFR_DIST = 3;
static constexpr int HFR_ENC_PAD = (TZ_NBINS + HFR_NTOK + 7) & ~7;

// Walks the run of `cnt` elements at r0.  f(m, lit, s) is called once per element and once behind the run: m > 0 is a
// stretch of m matches that ended in front of this point (to be coded first), lit says the element s is a literal.
// DIST is the match distance: 3 (TZR1, and TZR2 with D = 3) or 1 (TZR2 with D = 1: the neighbour in front).
template <bool VEC, int DIST, class F>
__device__ __forceinline__ void hfr_walk(const int16_t* __restrict__ in, size_t n, size_t r0, int cnt, F&& f) {
    static_assert(DIST == 1 || DIST == 3, "match distances of the formats: 1 and 3");
    int h1 = 0, h2 = 0, h3 = 0, m = 0;
    for (int j = 0; j < cnt; j += 8) {
        const short8 v = hf_load8<VEC>(in, r0 + j, n, (short)0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int s = v[k];
            const bool live = j + k < cnt, match = live && j + k >= DIST && s == (DIST == 1 ? h1 : h3), lit = live && !match;
            f(lit ? m : 0, lit, s);
            m = match ? m + 1 : (lit ? 0 : m);
            h3 = h2;
            h2 = h1;
            h1 = s;
        }
    }
    f(m, false, 0);   // the stretch the run's end cuts
}

// Token counts of the payload: bins [0, 4096) are the literals (bin = value + TZ_HUFF_COUNT_BIAS; a literal outside sets
// meta->bad), bins 4096 + k the tokens T_k.  One thread per run, the histogram of a workgroup in LDS.
template <bool VEC>
__global__ __launch_bounds__(256) void k_huffr_count(const int16_t* __restrict__ in, size_t n, size_t nruns, unsigned long long* __restrict__ hist,
                                                     tz_huff_meta* __restrict__ meta) {
    __shared__ unsigned h[TZ_HUFF_COUNT_BINS + HFR_NTOK];
    for (int k = threadIdx.x; k < TZ_HUFF_COUNT_BINS + HFR_NTOK; k += 256) h[k] = 0;
    __syncthreads();
    bool bad = false;
    for (size_t run = (size_t)blockIdx.x * 256 + threadIdx.x; run < nruns; run += (size_t)gridDim.x * 256) {
        const size_t r0 = run * HF_R;
        hfr_walk<VEC, HFR_DIST>(in, n, r0, (int)std::min((size_t)HF_R, n - r0), [&](int m, bool lit, int s) {
            if (m) atomicAdd(&h[TZ_HUFF_COUNT_BINS + (31 - __clz(m))], 1u);
            if (lit) {
                const int b = s + TZ_HUFF_COUNT_BIAS;
                if (b >= 0 && b < TZ_HUFF_COUNT_BINS) atomicAdd(&h[b], 1u);
                else bad = true;
            }
        });
    }
    __syncthreads();
    for (int k = threadIdx.x; k < TZ_HUFF_COUNT_BINS + HFR_NTOK; k += 256)
        if (h[k]) atomicAdd(&hist[k], (unsigned long long)h[k]);
    if (bad) atomicOr(&meta->bad, 1u);
}

int tzk_huffr_count(tz_ctx* ctx, const int16_t* in, size_t n, unsigned long long* d_hist, tz_huff_meta* d_meta) {
    const size_t nruns = (n + HF_R - 1) / HF_R;
    TZ_HIP(ctx, hipMemsetAsync(d_hist, 0, (TZ_HUFF_COUNT_BINS + HFR_NTOK) * sizeof(unsigned long long), ctx->stream));
    TZ_HIP(ctx, hipMemsetAsync(d_meta, 0, sizeof(tz_huff_meta), ctx->stream));
    tz_prof_scope ps(ctx, TZP_HUFF);
    const dim3 grid((unsigned)std::min((nruns + 255) / 256, (size_t)2048));
    if ((uintptr_t)in & 15) hipLaunchKernelGGL(k_huffr_count<false>, grid, dim3(256), 0, ctx->stream, in, n, nruns, d_hist, d_meta);
    else hipLaunchKernelGGL(k_huffr_count<true>, grid, dim3(256), 0, ctx->stream, in, n, nruns, d_hist, d_meta);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// Opt-in stage `--coder huffd` (format TZR2: DESIGN.md section 9, tezip_amd/huffd.py): the coder picks its match distance
// D in {0: no tokens, 1, 3} from exact counts, so ONE read of the payload fills the three histograms the choice needs, each of
// k_huffr_count's layout (4096 literal bins, then T_0..T_7): hist[0] the plain literals, hist[1] the tokens at distance 1,
// hist[2] those at distance 3.  One thread per run as there; a lane carries both match states (the neighbour h1 with its
// stretch m1, the element three back h3 with m3) through the same uniform steps.  A stretch at distance 1 is a run of equal
// values, so the plain histogram takes such a stretch with one add when it ends, not one per element.  A value outside the
// 4096 bins sets meta->bad (it is a literal at its first place in a run under every distance).
template <bool VEC>
__global__ __launch_bounds__(256) void k_huffd_count(const int16_t* __restrict__ in, size_t n, size_t nruns, unsigned long long* __restrict__ hist,
                                                     tz_huff_meta* __restrict__ meta) {
    constexpr int BINS = TZ_HUFF_COUNT_BINS + HFR_NTOK;
    __shared__ unsigned h[3 * BINS];
    for (int k = threadIdx.x; k < 3 * BINS; k += 256) h[k] = 0;
    __syncthreads();
    bool bad = false;
    for (size_t run = (size_t)blockIdx.x * 256 + threadIdx.x; run < nruns; run += (size_t)gridDim.x * 256) {
        const size_t r0 = run * HF_R;
        const int cnt = (int)std::min((size_t)HF_R, n - r0);
        int h1 = 0, h2 = 0, h3 = 0, m1 = 0, m3 = 0;
        for (int j = 0; j < cnt; j += 8) {
            const short8 v = hf_load8<VEC>(in, r0 + j, n, (short)0);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int s = v[k];
                if (j + k >= cnt) continue;   // (uniform but for the last run of the payload)
                const int b = s + TZ_HUFF_COUNT_BIAS, b1 = h1 + TZ_HUFF_COUNT_BIAS;
                const bool ok = b >= 0 && b < TZ_HUFF_COUNT_BINS;
                const bool match1 = j + k >= 1 && s == h1, match3 = j + k >= HFR_DIST && s == h3;
                bad |= !ok;
                if (match1) {
                    ++m1;
                } else {
                    if (m1) {   // the stretch in front: its token, and its elements as plain literals (h1 was counted in range)
                        atomicAdd(&h[BINS + TZ_HUFF_COUNT_BINS + (31 - __clz(m1))], 1u);
                        if (b1 >= 0 && b1 < TZ_HUFF_COUNT_BINS) atomicAdd(&h[b1], (unsigned)m1);
                        m1 = 0;
                    }
                    if (ok) {
                        atomicAdd(&h[b], 1u);
                        atomicAdd(&h[BINS + b], 1u);
                    }
                }
                if (match3) {
                    ++m3;
                } else {
                    if (m3) atomicAdd(&h[2 * BINS + TZ_HUFF_COUNT_BINS + (31 - __clz(m3))], 1u);
                    m3 = 0;
                    if (ok) atomicAdd(&h[2 * BINS + b], 1u);
                }
                h3 = h2;
                h2 = h1;
                h1 = s;
            }
        }
        const int b1 = h1 + TZ_HUFF_COUNT_BIAS;   // the stretches the run's end cuts
        if (m1) {
            atomicAdd(&h[BINS + TZ_HUFF_COUNT_BINS + (31 - __clz(m1))], 1u);
            if (b1 >= 0 && b1 < TZ_HUFF_COUNT_BINS) atomicAdd(&h[b1], (unsigned)m1);
        }
        if (m3) atomicAdd(&h[2 * BINS + TZ_HUFF_COUNT_BINS + (31 - __clz(m3))], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * BINS; k += 256)
        if (h[k]) atomicAdd(&hist[k], (unsigned long long)h[k]);
    if (bad) atomicOr(&meta->bad, 1u);
}

// d_hist: 3 x (TZ_HUFF_COUNT_BINS + 8) counts, distance 0 | 1 | 3
int tzk_huffd_count(tz_ctx* ctx, const int16_t* in, size_t n, unsigned long long* d_hist, tz_huff_meta* d_meta) {
    const size_t nruns = (n + HF_R - 1) / HF_R;
    TZ_HIP(ctx, hipMemsetAsync(d_hist, 0, 3 * (TZ_HUFF_COUNT_BINS + HFR_NTOK) * sizeof(unsigned long long), ctx->stream));
    TZ_HIP(ctx, hipMemsetAsync(d_meta, 0, sizeof(tz_huff_meta), ctx->stream));
    tz_prof_scope ps(ctx, TZP_HUFF);
    const dim3 grid((unsigned)std::min((nruns + 255) / 256, (size_t)2048));
    if ((uintptr_t)in & 15) hipLaunchKernelGGL(k_huffd_count<false>, grid, dim3(256), 0, ctx->stream, in, n, nruns, d_hist, d_meta);
    else hipLaunchKernelGGL(k_huffd_count<true>, grid, dim3(256), 0, ctx->stream, in, n, nruns, d_hist, d_meta);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// Size pass: one wave per chunk, four chunks per workgroup; a lane sums the bits of its run (code lengths of its literals
// and tokens plus the raw bits), run_bits[r] is the index's entry of run r, chunk_bits[c] feeds k_huff_scan.  `enc` holds
// A + 8 entries: the literals, then T_0..T_7.
template <bool VEC, int DIST>
__global__ __launch_bounds__(256) void k_huffr_size(const int16_t* __restrict__ in, size_t n, const uint16_t* __restrict__ enc, int A,
                                                    int base, size_t nruns, size_t nchunks, uint16_t* __restrict__ run_bits,
                                                    unsigned* __restrict__ chunk_bits, tz_huff_meta* __restrict__ meta) {
    __shared__ uint8_t len[HFR_ENC_PAD];
    for (int k = threadIdx.x; k < HFR_ENC_PAD; k += 256) len[k] = k < A + HFR_NTOK ? (uint8_t)(enc[k] >> 12) : 0;
    __syncthreads();
    const size_t chunk = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= nchunks) return;
    const int lane = threadIdx.x & 63;
    const size_t run = chunk * HF_CR + lane, r0 = run * HF_R;
    unsigned bits = 0;
    bool bad = false;
    if (run < nruns)
        hfr_walk<VEC, DIST>(in, n, r0, (int)std::min((size_t)HF_R, n - r0), [&](int m, bool lit, int s) {
            if (m) {
                const int k = 31 - __clz(m);
                const unsigned l = len[A + k];
                bits += l + k;
                bad |= l == 0;
            }
            if (lit) {
                const unsigned sym = (unsigned)(s - base);
                const unsigned l = sym < (unsigned)A ? len[sym] : 0u;
                bits += l;
                bad |= l == 0;
            }
        });
    if (run < nruns) run_bits[run] = (uint16_t)bits;
    unsigned tot = bits;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) tot += __shfl_xor(tot, d, 64);
    if (lane == 0) chunk_bits[chunk] = tot;
    if (bad) atomicOr(&meta->bad, 1u);
}

// Pack pass: k_huff_enc's scheme (one wave per chunk, 64-bit accumulator per lane, whole words ORed into the chunk's image
// in LDS, coalesced stores of the image, no global atomics) over the tokens of hfr_walk.  A step appends at most a token
// with its raw bits and a literal: 12 + 7 + 12 bits on top of fewer than 32, so the accumulator holds them.
template <bool VEC, int DIST>
__global__ __launch_bounds__(64) void k_huffr_enc(const int16_t* __restrict__ in, size_t n, const uint16_t* __restrict__ enc, int A, int base,
                                                  size_t nruns, const uint16_t* __restrict__ run_bits, const unsigned* __restrict__ chunk_off,
                                                  unsigned* __restrict__ words, size_t stream_words) {
    __shared__ uint16_t tab[HFR_ENC_PAD];
    __shared__ unsigned img[HF_CHUNK_WORDS];
    const size_t chunk = blockIdx.x, run = chunk * HF_CR + threadIdx.x;
    unsigned cw;
    const unsigned pos = hf_enc_begin<HFR_ENC_PAD>(tab, img, enc, A + HFR_NTOK, run, nruns, run_bits, &cw);
    const size_t r0 = run * HF_R;
    const int cnt = r0 < n ? (int)std::min((size_t)HF_R, n - r0) : 0;
    unsigned long long acc = 0;
    unsigned nb = pos & 31u, wi = pos >> 5;
    hfr_walk<VEC, DIST>(in, n, r0, cnt, [&](int m, bool lit, int s) {
        if (m) {
            const int k = 31 - __clz(m);
            const unsigned e = tab[A + k];            // (no code: k_huffr_size said so, and the host launched nothing)
            acc |= (unsigned long long)((e & 0xFFFu) | ((unsigned)(m - (1 << k)) << (e >> 12))) << nb;
            nb += (e >> 12) + k;
        }
        if (lit) {
            const unsigned sym = (unsigned)(s - base);
            const unsigned e = sym < (unsigned)A ? tab[sym] : 0u;
            acc |= (unsigned long long)(e & 0xFFFu) << nb;
            nb += e >> 12;
        }
        hf_flush(acc, nb, wi, cw, img);
    });
    hf_enc_end(acc, nb, wi, cw, img, chunk_off, chunk, words, stream_words);
}

// Expand pass: k_huff_dec's scheme and clamps (chunk offsets to the stream, staged words to the image, reads of the image
// to its end, run sizes to R * L, a lane stops after its run's element count, which comes from n alone).  Every lane
// produces one element per step: inside a stretch it copies the element DIST back, which it holds in registers (the
// history in front of a run is DIST times `base`); otherwise it looks up a symbol, and a token >= A starts a stretch of
// 2^k + k raw bits elements whose first one is this step's.  A stretch ends with the run, whatever its token says.  After
// a refill the accumulator holds more than 32 valid bits and a step takes at most 12 + 7, so a corrupt body yields wrong
// elements, never an access outside the buffers.
template <bool VEC, int DIST>
__global__ __launch_bounds__(64) void k_huffr_dec(const unsigned* __restrict__ chunk_off, const uint16_t* __restrict__ run_bits,
                                                  const unsigned* __restrict__ words, size_t stream_words, size_t nruns, size_t nchunks,
                                                  const uint16_t* __restrict__ dec, int A, int base, size_t n, int16_t* __restrict__ out) {
    __shared__ uint16_t tab[1 << HF_L];
    __shared__ unsigned img[HF_CHUNK_WORDS + 1];
    const size_t chunk = blockIdx.x, run = chunk * HF_CR + threadIdx.x;
    unsigned cw, nb, wi;
    unsigned long long acc;
    const unsigned pos = hf_dec_begin(tab, img, dec, chunk_off, run_bits, words, stream_words, nruns, nchunks, chunk, run, &cw);
    const size_t r0 = run * HF_R;
    const int cnt = r0 < n ? (int)std::min((size_t)HF_R, n - r0) : 0;
    hf_dec_first(img, pos, cw, acc, nb, wi);
    int h1 = base, h2 = base, h3 = base;
    unsigned m = 0;
    for (int j = 0; j < cnt; j += 8) {
        short8 v;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            int val = DIST == 1 ? h1 : h3;
            if (m == 0) {
                const unsigned e = tab[(unsigned)acc & 0xFFFu];
                const unsigned l = e >> 12, sym = e & 0xFFFu;
                acc >>= l;
                nb -= l;
                if (sym < (unsigned)A) {
                    val = (int)sym + base;
                    m = 1;
                } else {
                    const unsigned tk = std::min(sym - (unsigned)A, (unsigned)(HFR_NTOK - 1));
                    m = (1u << tk) + ((unsigned)acc & ((1u << tk) - 1u));
                    acc >>= tk;
                    nb -= tk;
                }
                hf_refill(acc, nb, wi, cw, img);
            }
            --m;
            v[k] = (short)val;
            h3 = h2;
            h2 = h1;
            h1 = val;
        }
        hf_store8<VEC>(out, r0, j, cnt, v);
    }
}

// The launchers of the size, pack and expand passes of the coder at the match distance `dist`: 0 (TZH1, the key frames, a TZR2
// file without tokens) runs the k_huff_* kernels, 3 (TZR1) and 1 (the other one a TZR2 file may name) the k_huffr_* ones at that
// distance (d_enc then holds A + TZ_HUFFR_NTOK entries); VEC says that the payload is 16-byte aligned.
int tzk_huff_size(tz_ctx* ctx, const int16_t* in, size_t n, const uint16_t* d_enc, int A, int base, uint16_t* d_run_bits,
                  unsigned* d_chunk_off, tz_huff_meta* d_meta, int dist) {
    if (dist != 0 && dist != 1 && dist != HFR_DIST) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: match distance %d, the kernels know 1 and 3", dist);
    const size_t nruns = (n + HF_R - 1) / HF_R, nchunks = (nruns + HF_CR - 1) / HF_CR;
    void* d_cbits;
    TZ_TRY(tz_pool_alloc(ctx, nchunks * sizeof(unsigned), &d_cbits));
    TZ_HIP(ctx, hipMemsetAsync(d_meta, 0, sizeof(tz_huff_meta), ctx->stream));
    tz_prof_scope ps(ctx, TZP_HUFF);
    const bool vec = !((uintptr_t)in & 15);
    const auto k = !dist      ? (vec ? k_huff_size<true> : k_huff_size<false>)
                   : dist == 1 ? (vec ? k_huffr_size<true, 1> : k_huffr_size<false, 1>)
                               : (vec ? k_huffr_size<true, HFR_DIST> : k_huffr_size<false, HFR_DIST>);
    hipLaunchKernelGGL(k, dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, ctx->stream, in, n, d_enc, A, base, nruns, nchunks, d_run_bits,
                       (unsigned*)d_cbits, d_meta);
    TZ_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_huff_scan, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned*)d_cbits, nchunks, d_chunk_off, d_meta);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_huff_enc(tz_ctx* ctx, const int16_t* in, size_t n, const uint16_t* d_enc, int A, int base, const uint16_t* d_run_bits,
                 const unsigned* d_chunk_off, unsigned* d_words, size_t stream_words, int dist) {
    if (dist != 0 && dist != 1 && dist != HFR_DIST) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: match distance %d, the kernels know 1 and 3", dist);
    const size_t nruns = (n + HF_R - 1) / HF_R, nchunks = (nruns + HF_CR - 1) / HF_CR;
    tz_prof_scope ps(ctx, TZP_HUFF);
    const bool vec = !((uintptr_t)in & 15);
    const auto k = !dist      ? (vec ? k_huff_enc<true> : k_huff_enc<false>)
                   : dist == 1 ? (vec ? k_huffr_enc<true, 1> : k_huffr_enc<false, 1>)
                               : (vec ? k_huffr_enc<true, HFR_DIST> : k_huffr_enc<false, HFR_DIST>);
    hipLaunchKernelGGL(k, dim3((unsigned)nchunks), dim3(64), 0, ctx->stream, in, n, d_enc, A, base, nruns, d_run_bits, d_chunk_off, d_words,
                       stream_words);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_huff_dec(tz_ctx* ctx, const unsigned* d_chunk_off, const uint16_t* d_run_bits, const unsigned* d_words, size_t stream_words,
                 const uint16_t* d_dec, int A, int base, size_t n, int16_t* out, int dist) {
    if (dist != 0 && dist != 1 && dist != HFR_DIST) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: match distance %d, the kernels know 1 and 3", dist);
    const size_t nruns = (n + HF_R - 1) / HF_R, nchunks = (nruns + HF_CR - 1) / HF_CR;
    tz_prof_scope ps(ctx, TZP_HUFF);
    const bool vec = !((uintptr_t)out & 15);
    const dim3 grid((unsigned)nchunks);
    if (dist)   // (the literal count A tells k_huffr_dec the tokens from the literals; k_huff_dec has no use for it)
        hipLaunchKernelGGL(dist == 1 ? (vec ? k_huffr_dec<true, 1> : k_huffr_dec<false, 1>)
                                     : (vec ? k_huffr_dec<true, HFR_DIST> : k_huffr_dec<false, HFR_DIST>),
                           grid, dim3(64), 0, ctx->stream, d_chunk_off, d_run_bits, d_words, stream_words, nruns, nchunks, d_dec, A, base, n, out);
    else
        hipLaunchKernelGGL(vec ? k_huff_dec<true> : k_huff_dec<false>, grid, dim3(64), 0, ctx->stream, d_chunk_off, d_run_bits, d_words,
                           stream_words, nruns, nchunks, d_dec, base, n, out);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ---------------------------------------------------------------------------- size of a candidate bound
// tz_size_probe (`-c --target-ratio`, definition TZ-TRATIO-1: DESIGN.md section 9, slow statement in tezip_amd/ratetarget.py
// count_of / bits_of): what the entropy coders would make of the quantised delta stack q, without a payload.  Both kernels
// form the payload symbols on the fly -- the spatial delta of the layout (k_sdelta: flat, k_sdelta_gray: channel 0 alone,
// k_sdelta_s3: the channel stride; the stream start has no element in front, sd = x), then 1600 - sd when apply_offset --
// and stop in front of the rank remap: it is a bijection on the symbols present, so equality at a distance is the payload's
// and the host permutes the literal counts.  Geometry and structure are k_huffd_count's: one lane per run of 256 symbols,
// 16-byte loads, no match across a run start.
// Two more layouts form the symbols of the 2-D spatial delta TZ-SD2 (k_sdelta_plane; tz_sdelta_probe, `-c --sdelta auto`,
// definition TZ-SDA1): SZ_P3 three channels, SZ_P1 channel 0 alone of q's whole pixels.  They walk in the overload of sz_walk
// that takes the frame, which the kernels pass on as their last argument; the three layouts above pass nothing, and their
// instructions are what they were.
enum { SZ_FLAT = 0, SZ_GRAY = 1, SZ_S3 = 2, SZ_P3 = 3, SZ_P1 = 4 };
template <bool VECU>
struct sz_frame {   // the frame of the plane layouts: rows and columns (H * W * 3 < 2^32); VECU: the row above loads 16 bytes
    int H, W;
};

// Walks the run of `cnt` symbols at symbol r0 (a multiple of 256) of the n symbols q yields: f(j, s) once per symbol, j its
// place in the run.  q holds n elements, 3 n under SZ_GRAY; VEC: q is 16-byte aligned.
template <int LAY, bool VEC, class F>
__device__ __forceinline__ void sz_walk(const int16_t* __restrict__ q, size_t n, size_t r0, int cnt, int apply_offset, F&& f) {
    constexpr int STRIDE = LAY == SZ_S3 ? 3 : 1;
    short p1 = 0, p2 = 0, p3 = 0;   // the elements one, two and three symbols in front
    if (r0) {
        if (LAY == SZ_GRAY) {
            p1 = q[3 * (r0 - 1)];
        } else {
            p1 = q[r0 - 1];
            if (LAY == SZ_S3) {
                p2 = q[r0 - 2];
                p3 = q[r0 - 3];
            }
        }
    }
    for (int j = 0; j < cnt; j += 8) {
        short8 v;
        if (LAY == SZ_GRAY) {   // 8 pixels = 24 elements, of which channel 0 is taken
            const size_t e0 = 3 * (r0 + j);
            const short8 a = hf_load8<VEC>(q, e0, 3 * n, (short)0), b = hf_load8<VEC>(q, e0 + 8, 3 * n, (short)0),
                         c = hf_load8<VEC>(q, e0 + 16, 3 * n, (short)0);
            v[0] = a[0], v[1] = a[3], v[2] = a[6], v[3] = b[1], v[4] = b[4], v[5] = b[7], v[6] = c[2], v[7] = c[5];
        } else {
            v = hf_load8<VEC>(q, r0 + j, n, (short)0);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const short cur = v[k], front = STRIDE == 3 ? p3 : p1;
            const short sd = (r0 || j + k >= STRIDE) ? (short)(front - cur) : cur;
            const short y = apply_offset ? (short)(TZ_OFFSET - sd) : sd;
            if (j + k < cnt) f(j + k, (int)y);   // (uniform but for the last run)
            p3 = p2;
            p2 = p1;
            p1 = cur;
        }
    }
}

// 8 consecutive symbols from symbol s0 of the plane layouts (SZ_P1: channel 0 of 8 pixels); VEC: the first is 16-byte aligned
template <int LAY, bool VEC>
__device__ __forceinline__ short8 sz_load8(const int16_t* __restrict__ q, size_t s0, size_t n) {
    if (LAY == SZ_P1) {
        const short8 a = hf_load8<VEC>(q, 3 * s0, 3 * n, (short)0), b = hf_load8<VEC>(q, 3 * s0 + 8, 3 * n, (short)0),
                     c = hf_load8<VEC>(q, 3 * s0 + 16, 3 * n, (short)0);
        short8 v;
        v[0] = a[0], v[1] = a[3], v[2] = a[6], v[3] = b[1], v[4] = b[4], v[5] = b[7], v[6] = c[2], v[7] = c[5];
        return v;
    }
    return hf_load8<VEC>(q, s0, n, (short)0);
}

// sz_walk for the plane layouts (the overload that takes the frame): symbol i <-> (f, y, x, c) is
// wrap9(q[y, x-1] + q[y-1, x] - q[y-1, x-1] - q[y, x]), every neighbour outside the frame 0 (tezip_amd/sdelta.py encode_plane
// at index i; x below counts symbols, so it runs over pixel and channel), then 1600 - sd when apply_offset.  A run starts
// anywhere in a row and may cross rows and frames: the place of its first symbol comes from one division by the frame and one
// by the row, and a counter pair follows from there.  The row above is a second load stream one row of symbols back -- in
// the flattened stack that is so across a row's end too -- VECU: it is 16-byte aligned (q is, and a row is whole 16-byte
// groups).  No index in front of q is formed: a group that starts inside row 0 of frame 0 loads element by element, and what
// a load brings from the frame in front (y == 0) or the row's far end (x == 0) is never used.
template <int LAY, bool VEC, bool VECU, class F>
__device__ __forceinline__ void sz_walk(const int16_t* __restrict__ q, size_t n, size_t r0, int cnt, int apply_offset, sz_frame<VECU> g,
                                        F&& f) {
    constexpr int C = LAY == SZ_P3 ? 3 : 1;    // symbols per pixel
    constexpr int QE = LAY == SZ_P3 ? 1 : 3;   // elements of q per symbol
    const unsigned rs = (unsigned)g.W * C, fs = rs * (unsigned)g.H;   // symbols of a row and of a frame
    const unsigned rem = (unsigned)(r0 % fs);
    unsigned y = rem / rs, x = rem - y * rs;   // the row in the frame, the symbol in the row
    short p1 = 0, p2 = 0, p3 = 0, u1 = 0, u2 = 0, u3 = 0;   // one, two and three symbols in front: this row, the row above
    if (x >= 1) {   // (x >= k: symbol r0 - k is in this row, and with y > 0 symbol r0 - k - rs in the row above, same frame)
        p1 = q[QE * (r0 - 1)];
        if (y) u1 = q[QE * (r0 - 1 - rs)];
    }
    if (C == 3 && x >= 2) {
        p2 = q[r0 - 2];
        if (y) u2 = q[r0 - 2 - rs];
    }
    if (C == 3 && x >= 3) {
        p3 = q[r0 - 3];
        if (y) u3 = q[r0 - 3 - rs];
    }
    for (int j = 0; j < cnt; j += 8) {
        const size_t s0 = r0 + j;
        const short8 v = sz_load8<LAY, VEC>(q, s0, n);
        short8 u;
        if (s0 >= rs) {
            u = sz_load8<LAY, VECU>(q, s0 - rs, n);
        } else {   // the group starts inside row 0 of frame 0
#pragma unroll
            for (int k = 0; k < 8; ++k) u[k] = (s0 + k >= rs && s0 + k - rs < n) ? q[QE * (s0 + k - rs)] : (short)0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool left = x >= (unsigned)C, up = y > 0;
            const int cur = v[k], a = left ? (int)(C == 3 ? p3 : p1) : 0, b = up ? (int)u[k] : 0,
                      c = left && up ? (int)(C == 3 ? u3 : u1) : 0;   // left, up, upleft
            const int sd = ((a + b - c - cur + 256) & 511) - 256;
            const int s = apply_offset ? TZ_OFFSET - sd : sd;
            if (j + k < cnt) f(j + k, s);   // (uniform but for the last run)
            p3 = p2, p2 = p1, p1 = v[k];
            u3 = u2, u2 = u1, u1 = u[k];
            if (++x == rs) {
                x = 0;
                if (++y == (unsigned)g.H) y = 0;
            }
        }
    }
}

// k_huffd_count over the symbols of sz_walk: hist[0] the plain histogram (the one the rank table is built from, bin = symbol +
// TZ_HUFF_COUNT_BIAS), hist[1] and hist[2] the token histograms at match distance 1 and 3.  No payload is written.
// (g: nothing, or the sz_frame of the plane layouts)
template <int LAY, bool VEC, class... G>
__global__ __launch_bounds__(256) void k_size_count(const int16_t* __restrict__ q, size_t n, size_t nruns, int apply_offset,
                                                    unsigned long long* __restrict__ hist, tz_huff_meta* __restrict__ meta, G... g) {
    constexpr int BINS = TZ_HUFF_COUNT_BINS + HFR_NTOK;
    __shared__ unsigned h[3 * BINS];
    for (int k = threadIdx.x; k < 3 * BINS; k += 256) h[k] = 0;
    __syncthreads();
    bool bad = false;
    for (size_t run = (size_t)blockIdx.x * 256 + threadIdx.x; run < nruns; run += (size_t)gridDim.x * 256) {
        const size_t r0 = run * HF_R;
        int h1 = 0, h2 = 0, h3 = 0, m1 = 0, m3 = 0;
        sz_walk<LAY, VEC>(q, n, r0, (int)std::min((size_t)HF_R, n - r0), apply_offset, g..., [&](int j, int s) {
            const int b = s + TZ_HUFF_COUNT_BIAS, b1 = h1 + TZ_HUFF_COUNT_BIAS;
            const bool ok = b >= 0 && b < TZ_HUFF_COUNT_BINS;
            const bool match1 = j >= 1 && s == h1, match3 = j >= HFR_DIST && s == h3;
            bad |= !ok;
            if (match1) {
                ++m1;
            } else {
                if (m1) {   // the stretch in front: its token, and its elements as plain literals
                    atomicAdd(&h[BINS + TZ_HUFF_COUNT_BINS + (31 - __clz(m1))], 1u);
                    if (b1 >= 0 && b1 < TZ_HUFF_COUNT_BINS) atomicAdd(&h[b1], (unsigned)m1);
                    m1 = 0;
                }
                if (ok) {
                    atomicAdd(&h[b], 1u);
                    atomicAdd(&h[BINS + b], 1u);
                }
            }
            if (match3) {
                ++m3;
            } else {
                if (m3) atomicAdd(&h[2 * BINS + TZ_HUFF_COUNT_BINS + (31 - __clz(m3))], 1u);
                m3 = 0;
                if (ok) atomicAdd(&h[2 * BINS + b], 1u);
            }
            h3 = h2;
            h2 = h1;
            h1 = s;
        });
        const int b1 = h1 + TZ_HUFF_COUNT_BIAS;   // the stretches the run's end cuts
        if (m1) {
            atomicAdd(&h[BINS + TZ_HUFF_COUNT_BINS + (31 - __clz(m1))], 1u);
            if (b1 >= 0 && b1 < TZ_HUFF_COUNT_BINS) atomicAdd(&h[b1], (unsigned)m1);
        }
        if (m3) atomicAdd(&h[2 * BINS + TZ_HUFF_COUNT_BINS + (31 - __clz(m3))], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 3 * BINS; k += 256)
        if (h[k]) atomicAdd(&hist[k], (unsigned long long)h[k]);
    if (bad) atomicOr(&meta->bad, 1u);
}

// The size pass without an index: one wave per chunk, four chunks per workgroup, a lane sums the bits of its run under the
// lengths in LDS -- len[bin] the code length of the symbol of that bin AFTER the rank remap (0: no code), then T_0..T_7 -- at
// the match distance dist (0: every symbol a literal; 1 or 3: hfr_walk's tokens, length + raw bits).  Every chunk's sum is
// rounded up to words and joins one 64-bit total; nothing else is written.
template <int LAY, bool VEC, class... G>
__global__ __launch_bounds__(256) void k_size_bits(const int16_t* __restrict__ q, size_t n, size_t nruns, size_t nchunks, int apply_offset,
                                                   const uint8_t* __restrict__ lens, int dist, tz_size_meta* __restrict__ meta, G... g) {
    __shared__ uint8_t len[TZ_HUFF_COUNT_BINS + HFR_NTOK];
    for (int k = threadIdx.x; k < (TZ_HUFF_COUNT_BINS + HFR_NTOK) / 4; k += 256) ((unsigned*)len)[k] = ((const unsigned*)lens)[k];
    __syncthreads();
    const size_t chunk = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= nchunks) return;
    const int lane = threadIdx.x & 63;
    const size_t run = chunk * HF_CR + lane, r0 = run * HF_R;
    unsigned bits = 0;
    bool bad = false;
    if (run < nruns) {
        int h1 = 0, h2 = 0, h3 = 0, m = 0;
        const auto stretch = [&]() {
            const int k = 31 - __clz(m);
            const unsigned l = len[TZ_HUFF_COUNT_BINS + k];
            bits += l + k;
            bad |= l == 0;
        };
        sz_walk<LAY, VEC>(q, n, r0, (int)std::min((size_t)HF_R, n - r0), apply_offset, g..., [&](int j, int s) {
            const bool match = dist && j >= dist && s == (dist == 1 ? h1 : h3);
            if (match) {
                ++m;
            } else {
                if (m) stretch();
                m = 0;
                const unsigned b = (unsigned)(s + TZ_HUFF_COUNT_BIAS);
                const unsigned l = b < (unsigned)TZ_HUFF_COUNT_BINS ? len[b] : 0u;
                bits += l;
                bad |= l == 0;
            }
            h3 = h2;
            h2 = h1;
            h1 = s;
        });
        if (m) stretch();   // the stretch the run's end cuts
    }
    unsigned tot = bits;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) tot += __shfl_xor(tot, d, 64);
    if (lane == 0) {
        atomicAdd(&meta->words, (unsigned long long)((tot + 31u) >> 5));
        atomicAdd(&meta->bits, (unsigned long long)tot);
    }
    if (bad) atomicOr(&meta->bad, 1u);
}

static int sz_layout(tz_ctx* ctx, tz_layout layout, const int16_t* q, size_t n, int* lay) {
    if ((uintptr_t)q & 1) return tz_fail(ctx, TZ_ERR_INVALID, "size probe: the delta stack must be 2-byte aligned");
    if (layout.plane_h || layout.plane_w) {   // TZ-SD2: whole frames of plane_h x plane_w, three channels or channel 0 alone
        const size_t fs = tz_frame_elems(layout, layout.plane_h, layout.plane_w);
        if (layout.plane_h < 1 || layout.plane_w < 1 || (size_t)layout.plane_h * layout.plane_w > 0x0FFFFFFFull || layout.stride != 1 ||
            (layout.channels != 3 && layout.channels != 1) || n % fs)
            return tz_fail(ctx, TZ_ERR_INVALID, "size probe: no plane layout of %zu symbols in frames of %d x %d x %d", n, layout.plane_h,
                           layout.plane_w, layout.channels);
        *lay = layout.channels == 3 ? SZ_P3 : SZ_P1;
        return TZ_OK;
    }
    if (layout.channels == 3 && layout.stride == 1) *lay = SZ_FLAT;
    else if (layout.channels == 1 && layout.stride == 1) *lay = SZ_GRAY;
    else if (layout.channels == 3 && layout.stride == 3) *lay = SZ_S3;
    else return tz_fail(ctx, TZ_ERR_INVALID, "size probe: no payload layout of %d channels at stride %d", layout.channels, layout.stride);
    return TZ_OK;
}

#define TZ_SIZE_LAUNCH(K, GRID, ...)                                                                                           \
    do {                                                                                                                       \
        const bool vec = !((uintptr_t)q & 15);                                                                                 \
        const auto kern = lay == SZ_FLAT   ? (vec ? K<SZ_FLAT, true> : K<SZ_FLAT, false>)                                      \
                          : lay == SZ_GRAY ? (vec ? K<SZ_GRAY, true> : K<SZ_GRAY, false>)                                      \
                                           : (vec ? K<SZ_S3, true> : K<SZ_S3, false>);                                         \
        hipLaunchKernelGGL(kern, GRID, dim3(256), 0, ctx->stream, __VA_ARGS__);                                                \
    } while (0)
// (the plane kernels: the row above is a 16-byte stream when q is one and a row of q, 3 W elements, is whole 16-byte groups)
#define TZ_SIZE_LAUNCH_PLANE(K, GRID, ...)                                                                                     \
    do {                                                                                                                       \
        const bool vec = !((uintptr_t)q & 15), vecu = vec && layout.plane_w % 8 == 0;                                          \
        const int H = layout.plane_h, W = layout.plane_w;                                                                      \
        if (vecu) {                                                                                                            \
            const auto kern = lay == SZ_P3 ? K<SZ_P3, true, sz_frame<true>> : K<SZ_P1, true, sz_frame<true>>;                  \
            hipLaunchKernelGGL(kern, GRID, dim3(256), 0, ctx->stream, __VA_ARGS__, sz_frame<true>{H, W});                      \
        } else {                                                                                                               \
            const auto kern = lay == SZ_P3 ? (vec ? K<SZ_P3, true, sz_frame<false>> : K<SZ_P3, false, sz_frame<false>>)        \
                                           : (vec ? K<SZ_P1, true, sz_frame<false>> : K<SZ_P1, false, sz_frame<false>>);       \
            hipLaunchKernelGGL(kern, GRID, dim3(256), 0, ctx->stream, __VA_ARGS__, sz_frame<false>{H, W});                     \
        }                                                                                                                      \
    } while (0)

// d_hist: 3 x (TZ_HUFF_COUNT_BINS + 8) counts, distance 0 | 1 | 3, of the n symbols q yields under the layout (cleared here)
int tzk_size_count(tz_ctx* ctx, tz_layout layout, const int16_t* q, size_t n, int apply_offset, unsigned long long* d_hist,
                   tz_huff_meta* d_meta) {
    int lay;
    TZ_TRY(sz_layout(ctx, layout, q, n, &lay));
    const size_t nruns = (n + HF_R - 1) / HF_R;
    TZ_HIP(ctx, hipMemsetAsync(d_hist, 0, 3 * (TZ_HUFF_COUNT_BINS + HFR_NTOK) * sizeof(unsigned long long), ctx->stream));
    TZ_HIP(ctx, hipMemsetAsync(d_meta, 0, sizeof(tz_huff_meta), ctx->stream));
    if (n == 0) return TZ_OK;
    tz_prof_scope ps(ctx, TZP_HUFF);
    const dim3 grid((unsigned)std::min((nruns + 255) / 256, (size_t)2048));
    if (lay == SZ_P3 || lay == SZ_P1)
        TZ_SIZE_LAUNCH_PLANE(k_size_count, grid, q, n, nruns, apply_offset, d_hist, d_meta);
    else
        TZ_SIZE_LAUNCH(k_size_count, grid, q, n, nruns, apply_offset, d_hist, d_meta);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// d_lens: TZ_HUFF_COUNT_BINS + 8 code lengths (by bin, then the tokens), 4-byte aligned; d_meta is cleared here
int tzk_size_bits(tz_ctx* ctx, tz_layout layout, const int16_t* q, size_t n, int apply_offset, const uint8_t* d_lens, int dist,
                  tz_size_meta* d_meta) {
    int lay;
    TZ_TRY(sz_layout(ctx, layout, q, n, &lay));
    if (dist != 0 && dist != 1 && dist != HFR_DIST) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: match distance %d, the kernels know 1 and 3", dist);
    if ((uintptr_t)d_lens & 3) return tz_fail(ctx, TZ_ERR_INVALID, "size probe: the code lengths must be 4-byte aligned");
    const size_t nruns = (n + HF_R - 1) / HF_R, nchunks = (nruns + HF_CR - 1) / HF_CR;
    TZ_HIP(ctx, hipMemsetAsync(d_meta, 0, sizeof(tz_size_meta), ctx->stream));
    if (n == 0) return TZ_OK;
    tz_prof_scope ps(ctx, TZP_HUFF);
    const dim3 grid((unsigned)((nchunks + 3) / 4));
    if (lay == SZ_P3 || lay == SZ_P1)
        TZ_SIZE_LAUNCH_PLANE(k_size_bits, grid, q, n, nruns, nchunks, apply_offset, d_lens, dist, d_meta);
    else
        TZ_SIZE_LAUNCH(k_size_bits, grid, q, n, nruns, nchunks, apply_offset, d_lens, dist, d_meta);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}
#undef TZ_SIZE_LAUNCH
#undef TZ_SIZE_LAUNCH_PLANE

// ---------------------------------------------------------------------------- key-frame coder
// Opt-in stage `--key-coder huff` (format TZK1: DESIGN.md section 9, tezip_amd/keycoder.py is the slow statement of it).
// A key frame is turned into the residuals of one of four predictors over its own samples -- 0: none, 1: the left
// neighbour a, 2: the upper neighbour b, 3: a + b - c with c the upper-left one, always of the same channel and 0 outside
// the frame, everything mod 256 -- and the residuals of all key frames are coded by the k_huff_* kernels above as int16
// symbols 0..255.  The inverses are prefix sums mod 256 along the rows (1), the columns (2) or both (3).
// `--key-coder huffg` (format TZK2, tezip_amd/keycoderg.py) is the same with one more bit per key frame: a key frame whose
// three channels are equal at every pixel is GRAY (bit 2, value 4, of its pred byte), contributes the H * W residuals of
// channel 0 alone, and the inverse writes each sample to all three channels.  Frames therefore differ in size: frame k's symbols
// start at off[k], the u64 exclusive prefix of the per-frame symbol counts the host passes in.  TZK1 = TZK2 with no GRAY bit
// (off[k] = k * fe), so one residual kernel and one set of inverse kernels serve both.
// A frame is fe = H * W3 bytes, W3 = 3 W; a thread takes a UNIT of it: unit 0 is the head in front of the first 16-byte
// boundary of the frame's address (fewer than 16 samples, possibly none), unit u >= 1 the 16 samples from there on.
struct KeyWin {
    unsigned x[16], a[16], b[16], c[16];   // the samples and their left, upper and upper-left neighbours (0 outside the frame)
};

__device__ __forceinline__ unsigned key_head(const uint8_t* f, size_t fe) {
    return (unsigned)min(fe, (size_t)((16 - ((uintptr_t)f & 15)) & 15));
}

// *e / *cnt: first sample and number of samples of unit u (cnt 0: nothing to do)
__device__ __forceinline__ void key_unit(size_t u, unsigned head, size_t fe, size_t* e, int* cnt) {
    if (u == 0) {
        *e = 0;
        *cnt = (int)head;
    } else {
        *e = head + (u - 1) * 16;
        *cnt = *e < fe ? (int)min((size_t)16, fe - *e) : 0;
    }
}

__device__ __forceinline__ void key_window(const uint8_t* __restrict__ f, size_t fe, unsigned W3, size_t e, int cnt, KeyWin& w) {
    unsigned cw[19], uw[19];   // samples e - 3 .. e + 15 and the 19 one row above them
    if (cnt == 16 && e >= (size_t)W3 + 4) {   // a whole unit with every neighbour inside the frame; f + e is 16-byte aligned
        const uint4 cur = *(const uint4*)(f + e);
        const unsigned left = *(const unsigned*)(f + e - 4);
        uint8_t up[19];
        __builtin_memcpy(up, f + e - W3 - 3, 19);   // (no alignment: W3 is any multiple of 3)
        const unsigned cq[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
        for (int j = 0; j < 3; ++j) cw[j] = (left >> (8 * (j + 1))) & 0xffu;
#pragma unroll
        for (int j = 0; j < 16; ++j) cw[j + 3] = (cq[j >> 2] >> (8 * (j & 3))) & 0xffu;
#pragma unroll
        for (int j = 0; j < 19; ++j) uw[j] = up[j];
    } else {                                   // the head, the tail and the first row: sample by sample, each index checked
#pragma unroll
        for (int j = 0; j < 19; ++j) {
            const long long i = (long long)e - 3 + j, iu = i - (long long)W3;
            cw[j] = (i >= 0 && i < (long long)fe && j < cnt + 3) ? f[i] : 0u;
            uw[j] = (iu >= 0 && iu < (long long)fe && j < cnt + 3) ? f[iu] : 0u;
        }
    }
    unsigned y = (unsigned)(e / W3), r = (unsigned)(e - (size_t)y * W3);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const bool hl = r >= 3, hu = y > 0;
        w.x[j] = cw[j + 3];
        w.a[j] = hl ? cw[j] : 0u;
        w.b[j] = hu ? uw[j + 3] : 0u;
        w.c[j] = (hl && hu) ? uw[j] : 0u;
        if (++r == W3) {
            r = 0;
            ++y;
        }
    }
}

// Counts of the residual values of key frame idx[k] under all four predictors, from ONE read of the frame:
// counts[k][p][256].  Every wave of a workgroup has its own 4 x 256 counters in LDS (the residuals of a smooth frame crowd
// into a few bins); a workgroup adds each (predictor, bin) it touched to the global counters once.
__global__ __launch_bounds__(256) void k_key_hist(const uint8_t* __restrict__ frames, size_t fe, unsigned W3, const int* __restrict__ idx,
                                                  unsigned* __restrict__ counts) {
    __shared__ unsigned h[4][1024];
    for (int k = threadIdx.x; k < 4096; k += 256) (&h[0][0])[k] = 0;
    __syncthreads();
    const int key = blockIdx.y;
    const uint8_t* f = frames + (size_t)idx[key] * fe;
    const unsigned head = key_head(f, fe);
    const size_t nunits = 1 + (fe - head + 15) / 16, stride = (size_t)gridDim.x * 256;
    unsigned* hw = h[threadIdx.x >> 6];
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < nunits; u += stride) {
        size_t e;
        int cnt;
        key_unit(u, head, fe, &e, &cnt);
        if (cnt <= 0) continue;
        KeyWin w;
        key_window(f, fe, W3, e, cnt, w);
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < cnt) {
                atomicAdd(&hw[w.x[j]], 1u);
                atomicAdd(&hw[256 + ((w.x[j] - w.a[j]) & 255u)], 1u);
                atomicAdd(&hw[512 + ((w.x[j] - w.b[j]) & 255u)], 1u);
                atomicAdd(&hw[768 + ((w.x[j] - w.a[j] - w.b[j] + w.c[j]) & 255u)], 1u);
            }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 1024; k += 256) {
        const unsigned s = h[0][k] + h[1][k] + h[2][k] + h[3][k];
        if (s) atomicAdd(&counts[(size_t)key * 1024 + k], s);
    }
}

static dim3 key_grid(size_t fe, int nkeys) {
    return dim3((unsigned)std::min<size_t>((fe / 16 + 2 + 255) / 256, 256), (unsigned)nkeys);
}

int tzk_key_hist(tz_ctx* ctx, const uint8_t* d_frames, int H, int W, const int* d_idx, int nkeys, unsigned* d_counts) {
    const size_t fe = (size_t)H * W * 3;
    TZ_HIP(ctx, hipMemsetAsync(d_counts, 0, (size_t)nkeys * 1024 * sizeof(unsigned), ctx->stream));
    tz_prof_scope ps(ctx, TZP_HUFF);
    hipLaunchKernelGGL(k_key_hist, key_grid(fe, nkeys), dim3(256), 0, ctx->stream, d_frames, fe, (unsigned)W * 3u, d_idx, d_counts);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// flags[k] becomes non-zero iff key frame idx[k] has a pixel with unequal channels.  The frame is gray iff f[i] == f[i + 1] for
// every byte index i with i % 3 != 2 (fe is a multiple of 3, so i + 1 < fe for those).  Unit 0 is the head in front of the first
// 16-byte boundary, unit u >= 1 the 48 bytes from there on: three 16-byte loads, every byte compared with its successor through
// a funnel shift (the successor of the 48th byte is loaded by itself), the comparisons at i % 3 == 2 masked out.  48 is a
// multiple of 3, so the mask depends on the frame alone.  One OR per workgroup that saw an unequal pixel.
__global__ __launch_bounds__(256) void k_key_gray(const uint8_t* __restrict__ frames, size_t fe, const int* __restrict__ idx,
                                                  unsigned* __restrict__ flags) {
    const int key = blockIdx.y;
    const uint8_t* f = frames + (size_t)idx[key] * fe;
    const unsigned head = key_head(f, fe);
    const size_t nunits = 1 + (fe - head + 47) / 48, stride = (size_t)gridDim.x * 256;
    unsigned mask[3];   // byte k of mask[d]: 0xff where (head + 4 d + k) % 3 != 2
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        mask[d] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((head + 4u * d + k) % 3u != 2u) mask[d] |= 0xffu << (8 * k);
    }
    unsigned bad = 0;
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < nunits; u += stride) {
        if (u == 0) {
            for (unsigned i = 0; i < head; ++i)
                if (i % 3u != 2u) bad |= (unsigned)(f[i] ^ f[i + 1]);     // i + 1 < fe: i is not the last byte of its pixel
            continue;
        }
        const size_t e = head + (u - 1) * 48;
        if (e >= fe) continue;
        if (fe - e >= 48) {   // a whole unit; f + e is 16-byte aligned
            const uint4 q0 = *(const uint4*)(f + e), q1 = *(const uint4*)(f + e + 16), q2 = *(const uint4*)(f + e + 32);
            const unsigned next = e + 48 < fe ? f[e + 48] : 0u;            // (when e + 48 == fe, byte 47 ends a pixel: masked)
            const unsigned w[13] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, next};
#pragma unroll
            for (int j = 0; j < 12; ++j) bad |= (w[j] ^ ((w[j] >> 8) | (w[j + 1] << 24))) & mask[j % 3];
        } else {              // the tail: byte by byte
            for (size_t i = e; i < fe; ++i)
                if (i % 3 != 2) bad |= (unsigned)(f[i] ^ f[i + 1]);
        }
    }
    if (__syncthreads_or(bad != 0) && threadIdx.x == 0) atomicOr(&flags[key], 1u);
}

int tzk_key_gray(tz_ctx* ctx, const uint8_t* d_frames, int H, int W, const int* d_idx, int nkeys, unsigned* d_flags) {
    const size_t fe = (size_t)H * W * 3;
    TZ_HIP(ctx, hipMemsetAsync(d_flags, 0, (size_t)nkeys * sizeof(unsigned), ctx->stream));
    tz_prof_scope ps(ctx, TZP_HUFF);
    hipLaunchKernelGGL(k_key_gray, dim3((unsigned)std::min<size_t>((fe / 48 + 2 + 255) / 256, 256), (unsigned)nkeys), dim3(256), 0, ctx->stream,
                       d_frames, fe, d_idx, d_flags);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// Residuals of key frame idx[k] under pred byte pred[k] as int16 symbols 0..255 at sym[off[k] ...]: what k_huff_size /
// k_huff_enc code.  GRAY: a thread per pixel reads channel 0 of the pixel and of its three neighbours at stride 3 (a wave covers
// 192 contiguous bytes of a row) and writes one symbol, so a wave stores 128 contiguous bytes.  Any other frame: a thread per
// unit, 16-byte loads of the samples; 16-byte stores where the output's address allows them.
__global__ __launch_bounds__(256) void k_key_resid(const uint8_t* __restrict__ frames, int H, int W, const int* __restrict__ idx,
                                                   const uint8_t* __restrict__ pred, const unsigned long long* __restrict__ off,
                                                   int16_t* __restrict__ sym) {
    const int key = blockIdx.y;
    const size_t W3 = (size_t)W * 3, fe = (size_t)H * W3, stride = (size_t)gridDim.x * 256;
    const uint8_t* f = frames + (size_t)idx[key] * fe;
    int16_t* out = sym + off[key];
    const unsigned p = pred[key] & 3u;
    if (pred[key] & 4u) {   // (workgroup-uniform)
        const size_t np = (size_t)H * W;
        for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < np; q += stride) {
            const size_t y = q / (size_t)W, col = q - y * (size_t)W;
            const bool hl = col > 0, hu = y > 0;
            const unsigned x = f[q * 3];
            const unsigned a = hl ? f[(q - 1) * 3] : 0u, b = hu ? f[(q - W) * 3] : 0u, c = (hl && hu) ? f[(q - W - 1) * 3] : 0u;
            const unsigned pr = (p & 1u ? a : 0u) + (p & 2u ? b : 0u) - (p == 3u ? c : 0u);
            out[q] = (int16_t)((x - pr) & 255u);
        }
        return;
    }
    const unsigned head = key_head(f, fe);
    const size_t nunits = 1 + (fe - head + 15) / 16;
    for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < nunits; u += stride) {
        size_t e;
        int cnt;
        key_unit(u, head, fe, &e, &cnt);
        if (cnt <= 0) continue;
        KeyWin w;
        key_window(f, fe, (unsigned)W3, e, cnt, w);
        short8 lo, hi;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned q = (p & 1u ? w.a[j] : 0u) + (p & 2u ? w.b[j] : 0u) - (p == 3u ? w.c[j] : 0u);
            const short v = (short)((w.x[j] - q) & 255u);
            if (j < 8) lo[j] = v;
            else hi[j - 8] = v;
        }
        if (cnt == 16 && ((uintptr_t)(out + e) & 15) == 0) {
            *(short8*)(out + e) = lo;
            *(short8*)(out + e + 8) = hi;
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (j < cnt) out[e + j] = j < 8 ? lo[j] : hi[j - 8];
        }
    }
}

int tzk_key_resid(tz_ctx* ctx, const uint8_t* d_frames, int H, int W, const int* d_idx, const uint8_t* d_pred,
                  const unsigned long long* d_off, int nkeys, int16_t* d_sym) {
    tz_prof_scope ps(ctx, TZP_HUFF);
    hipLaunchKernelGGL(k_key_resid, key_grid((size_t)H * W * 3, nkeys), dim3(256), 0, ctx->stream, d_frames, H, W, d_idx, d_pred, d_off, d_sym);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// A wave holds one sample per lane, those of ncols (1..64) neighbouring pixels; their 3 * ncols bytes -- every sample three
// times -- go to g as aligned dwords: lane d builds the d-th aligned dword at or below g from the samples of the (at most two)
// pixels it covers, fetched by shuffles, and stores it whole where all four bytes belong to the chunk, byte by byte at the two
// ends.  g has any alignment; 3 * 64 bytes and up to 3 bytes of misalignment touch at most 49 dwords.  Every lane of the wave
// must call this.
__device__ __forceinline__ void keyg_store3(unsigned v, int lane, int ncols, uint8_t* g) {
    const int n = ncols * 3, t0 = lane * 4 - (int)((uintptr_t)g & 3);   // t0: this lane's dword, as a byte offset from g
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = min(max(t0 + j, 0), 191);
        w |= (__shfl(v, t / 3, 64) & 255u) << (8 * j);
    }
    if (t0 >= n) return;
    if (t0 >= 0 && t0 + 4 <= n) {
        *(unsigned*)(g + t0) = w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (t0 + j >= 0 && t0 + j < n) g[t0 + j] = (uint8_t)(w >> (8 * j));
    }
}

// One sample per lane, 64 neighbouring columns of a row: the inclusive prefix sum over the lanes plus *carry, what the columns
// in front of them add up to; *carry becomes the last lane's sum mod 256.  Every lane of the wave must call this.
__device__ __forceinline__ unsigned key_scan64(unsigned v, int lane, unsigned* carry) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    v += *carry;
    *carry = __shfl(v, 63, 64) & 255u;
    return v;
}

// The inverse, first pass: one wave per (key frame, row) turns the row's symbols into bytes of frame idx[k] -- under
// predictors 1 and 3 as the inclusive prefix sum mod 256 along the row, per channel, 64 columns at a time (key_scan64).  GRAY:
// the row's W sums go replicated into the frame (keyg_store3) -- or, when a column pass follows (predictors 2 and 3), as
// single bytes to tmp[off[k] + y * W + col], from where k_key_unresid_colg finishes them.  Only the low byte of a symbol counts.
__global__ __launch_bounds__(256) void k_key_unresid_row(const int16_t* __restrict__ sym, int H, int W, const int* __restrict__ idx,
                                                         const uint8_t* __restrict__ pred, const unsigned long long* __restrict__ off,
                                                         uint8_t* __restrict__ tmp, uint8_t* __restrict__ frames) {
    const int key = blockIdx.y, y = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (y >= H) return;   // (wave-uniform)
    const size_t W3 = (size_t)W * 3, fe = (size_t)H * W3;
    const unsigned pb = pred[key];
    const bool scan = (pb & 1u) != 0;
    uint8_t* o = frames + (size_t)idx[key] * fe + (size_t)y * W3;
    if (pb & 4u) {   // (workgroup-uniform)
        const int16_t* s = sym + off[key] + (size_t)y * W;
        uint8_t* t = tmp + off[key] + (size_t)y * W;
        unsigned carry = 0;
        for (int c0 = 0; c0 < W; c0 += 64) {
            const int col = c0 + lane;
            unsigned v = col < W ? (unsigned)s[col] & 255u : 0u;
            if (scan) v = key_scan64(v, lane, &carry);
            if (pb & 2u) {
                if (col < W) t[col] = (uint8_t)v;
            } else {
                keyg_store3(v, lane, min(64, W - c0), o + (size_t)c0 * 3);
            }
        }
        return;
    }
    const int16_t* s = sym + off[key] + (size_t)y * W3;
    unsigned carry[3] = {0u, 0u, 0u};
    for (int c0 = 0; c0 < W; c0 += 64) {
        const int col = c0 + lane;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            unsigned v = col < W ? (unsigned)s[(size_t)col * 3 + ch] & 255u : 0u;
            if (scan) v = key_scan64(v, lane, &carry[ch]);
            if (col < W) o[(size_t)col * 3 + ch] = (uint8_t)v;
        }
    }
}

// Second pass, predictors 2 and 3 of a frame that is not GRAY: a thread per (key frame, sample of a row) walks down its column
// and replaces every byte by the running sum mod 256; neighbouring threads touch neighbouring bytes.  Eight rows are loaded
// before they are summed.
__global__ __launch_bounds__(256) void k_key_unresid_col(int H, int W, const int* __restrict__ idx, const uint8_t* __restrict__ pred,
                                                         uint8_t* __restrict__ frames) {
    const int key = blockIdx.y;
    if ((pred[key] & 6u) != 2u) return;   // (workgroup-uniform)
    const size_t W3 = (size_t)W * 3, fe = (size_t)H * W3, j = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= W3) return;
    uint8_t* o = frames + (size_t)idx[key] * fe + j;
    unsigned acc = 0;
    for (int y0 = 0; y0 < H; y0 += 8) {
        unsigned v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = y0 + i < H ? o[(size_t)(y0 + i) * W3] : 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            acc += v[i];
            if (y0 + i < H) o[(size_t)(y0 + i) * W3] = (uint8_t)acc;
        }
    }
}

// Second pass of a GRAY frame under predictors 2 and 3: a thread per (key frame, column) walks down its column of tmp, eight
// rows loaded ahead, and every wave writes the running sums mod 256 of its 64 columns replicated into the frame (keyg_store3).
__global__ __launch_bounds__(256) void k_key_unresid_colg(int H, int W, const int* __restrict__ idx, const uint8_t* __restrict__ pred,
                                                          const unsigned long long* __restrict__ off, const uint8_t* __restrict__ tmp,
                                                          uint8_t* __restrict__ frames) {
    const int key = blockIdx.y, lane = threadIdx.x & 63;
    if ((pred[key] & 6u) != 6u) return;   // (workgroup-uniform)
    const int c0 = (int)(blockIdx.x * 256 + (threadIdx.x & ~63u));   // the wave's first column
    if (c0 >= W) return;                   // (wave-uniform)
    const int col = c0 + lane, ncols = min(64, W - c0);
    const size_t W3 = (size_t)W * 3, fe = (size_t)H * W3;
    const uint8_t* t = tmp + off[key] + col;
    uint8_t* o = frames + (size_t)idx[key] * fe + (size_t)c0 * 3;
    unsigned acc = 0;
    for (int y0 = 0; y0 < H; y0 += 8) {
        unsigned v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (y0 + i < H && col < W) ? t[(size_t)(y0 + i) * W] : 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            acc += v[i];
            if (y0 + i < H) keyg_store3(acc, lane, ncols, o + (size_t)(y0 + i) * W3);   // (the condition is wave-uniform)
        }
    }
}

// d_tmp: scratch of one byte per symbol for the GRAY frames' column pass, or NULL when no frame has (pred & 6) == 6 -- the host
// knows the pred bytes -- and k_key_unresid_colg has nothing to do
int tzk_key_unresid(tz_ctx* ctx, const int16_t* d_sym, int H, int W, const int* d_idx, const uint8_t* d_pred, const unsigned long long* d_off,
                    int nkeys, uint8_t* d_tmp, uint8_t* d_frames) {
    tz_prof_scope ps(ctx, TZP_HUFF);
    hipLaunchKernelGGL(k_key_unresid_row, dim3((unsigned)((H + 3) / 4), (unsigned)nkeys), dim3(256), 0, ctx->stream, d_sym, H, W, d_idx, d_pred,
                       d_off, d_tmp, d_frames);
    TZ_HIP(ctx, hipGetLastError());
    if (d_tmp) {
        hipLaunchKernelGGL(k_key_unresid_colg, dim3((unsigned)((W + 255) / 256), (unsigned)nkeys), dim3(256), 0, ctx->stream, H, W, d_idx, d_pred,
                           d_off, d_tmp, d_frames);
        TZ_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_key_unresid_col, dim3((unsigned)(((size_t)W * 3 + 255) / 256), (unsigned)nkeys), dim3(256), 0, ctx->stream, H, W, d_idx,
                       d_pred, d_frames);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------------------------------ closed-loop prediction (TZ-CL1)
// tz_rollout_closed / tz_rollout_decode_closed (include/tezip_hip.h; slow statement in
// tezip_amd/closedloop.py): between two predictor steps the frames the step predicted are DECODED, and the decoded bytes are what
// the next step is fed.  Per sample, with x = (int)(pred * 255.0f) the truncated prediction (compress.py:307,311) cropped to H x W:
//   k_cl_step  (encoder)  d = x - orig, q = TZ-QL1(d, E) as lat_apply forms it for a uniform abs tolerance, dec = clamp(x - q, 0, 255)
//   k_cl_recon (decoder)  dec = clamp(x - q, 0, 255) with q read from the int16 stack the payload decodes to (k_recon's arithmetic)
// blockIdx.y walks `list`, the sequence indices of the step's frames; pred is the padded stack (pitch Wp * 3), orig / q / dec the
// unpadded ones.  A lane makes 16 samples: one 16-byte load of orig (two of q), one 16-byte store of dec, and the 16 predictions
// as four 16-byte loads where the frame is unpadded (FLAT) or one by one across the crop.  vec == 0 (a stack off the 16-byte
// boundary): every sample goes one by one; else the `head` samples in front of the frame's first 16-byte boundary and the tail
// behind the last whole group do.
__device__ __forceinline__ unsigned cl_sample(float p, int o, int E) {
    const int x = (int)(p * 255.0f), d = x - o;
    const unsigned ad = (unsigned)(d < 0 ? -d : d), s = 2u * (unsigned)E + 1u;
    const int m = (int)min((ad + (unsigned)E) / s * s, 255u);
    const int q = E ? (d < 0 ? -m : m) : d;
    const int v = x - q;
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ unsigned cl_recon_sample(float p, int q) {
    const int v = (int)(p * 255.0f) - q;
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// the prediction of sample r of an unpadded frame (row = W * 3 samples a row, pitch = Wp * 3)
__device__ __forceinline__ float cl_pred(const float* __restrict__ pf, size_t r, unsigned row, unsigned pitch) {
    const size_t y = r / row;
    return pf[y * pitch + (r - y * row)];
}

template <bool RECON, bool FLAT>
__device__ __forceinline__ void cl_frames(const float* __restrict__ pred, const uint8_t* __restrict__ orig, const int16_t* __restrict__ qs,
                                          uint8_t* __restrict__ dec, const int* __restrict__ list, int H, int W, int Hp, int Wp, int E, int vec) {
    const size_t f = (size_t)list[blockIdx.y];
    const unsigned row = (unsigned)W * 3u, pitch = (unsigned)Wp * 3u;
    const size_t fe = (size_t)H * row, base = f * fe;
    const float* pf = pred + f * (size_t)Hp * pitch;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t head = vec ? min(fe, (size_t)((16u - (unsigned)(base & 15)) & 15u)) : fe;
    const size_t n16 = (fe - head) / 16;
    for (size_t g = t0; g < n16; g += stride) {
        const size_t r0 = head + 16 * g;
        float p[16];
        if (FLAT) {   // (an unpadded frame is whole groups of 64 samples: head == 0 and r0 is a multiple of 16)
            const float4* p4 = (const float4*)(pf + r0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 v = p4[j];
                p[4 * j] = v.x; p[4 * j + 1] = v.y; p[4 * j + 2] = v.z; p[4 * j + 3] = v.w;
            }
        } else {
            size_t y = r0 / row;
            unsigned xc = (unsigned)(r0 - y * row);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                p[j] = pf[y * pitch + xc];
                if (++xc == row) {
                    xc = 0;
                    ++y;
                }
            }
        }
        unsigned b[16];
        if (RECON) {
            const uint4* q4 = (const uint4*)(qs + base + r0);
            const uint4 a = q4[0], c = q4[1];
            const unsigned w[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                b[2 * j] = cl_recon_sample(p[2 * j], (int)(short)(w[j] & 0xFFFFu));
                b[2 * j + 1] = cl_recon_sample(p[2 * j + 1], (int)w[j] >> 16);
            }
        } else {
            const uint4 o = *(const uint4*)(orig + base + r0);
            const unsigned w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) b[j] = cl_sample(p[j], (int)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu), E);
        }
        uint4 out;
        out.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        out.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
        out.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
        out.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
        *(uint4*)(dec + base + r0) = out;
    }
    const size_t v_end = head + 16 * n16, nscalar = head + (fe - v_end);
    for (size_t j = t0; j < nscalar; j += stride) {
        const size_t r = j < head ? j : v_end + (j - head);
        const float p = cl_pred(pf, r, row, pitch);
        dec[base + r] = (uint8_t)(RECON ? cl_recon_sample(p, (int)qs[base + r]) : cl_sample(p, (int)orig[base + r], E));
    }
}

template <bool FLAT>
__global__ __launch_bounds__(256) void k_cl_step(const float* __restrict__ pred, const uint8_t* __restrict__ orig, uint8_t* __restrict__ dec,
                                                 const int* __restrict__ list, int H, int W, int Hp, int Wp, int E, int vec) {
    cl_frames<false, FLAT>(pred, orig, nullptr, dec, list, H, W, Hp, Wp, E, vec);
}

template <bool FLAT>
__global__ __launch_bounds__(256) void k_cl_recon(const float* __restrict__ pred, const int16_t* __restrict__ qs, uint8_t* __restrict__ dec,
                                                  const int* __restrict__ list, int H, int W, int Hp, int Wp, int vec) {
    cl_frames<true, FLAT>(pred, nullptr, qs, dec, list, H, W, Hp, Wp, 0, vec);
}

// d_list: nlist sequence indices (device); every stack is the whole sequence's.  orig (step) or q (recon) is NULL for the other form.
static int cl_launch(tz_ctx* ctx, const float* pred, const uint8_t* orig, const int16_t* q, uint8_t* dec, const int* d_list, int nlist,
                     int H, int W, int Hp, int Wp, int E) {
    if (nlist <= 0) return TZ_OK;
    const bool recon = q != nullptr;
    const size_t fe = (size_t)H * W * 3;
    const int vec = ((((uintptr_t)dec | (uintptr_t)(recon ? (const void*)q : (const void*)orig) | (uintptr_t)pred) & 15) == 0) ? 1 : 0;
    const bool flat = vec && H == Hp && W == Wp;
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((fe / 16 + 255) / 256, 64));   // (times nlist frames)
    const dim3 grid(gx, (unsigned)nlist);
    tz_prof_scope ps(ctx, recon ? TZP_RECON : TZP_QUANT);
    if (recon) {
        if (flat) hipLaunchKernelGGL(k_cl_recon<true>, grid, dim3(256), 0, ctx->stream, pred, q, dec, d_list, H, W, Hp, Wp, vec);
        else hipLaunchKernelGGL(k_cl_recon<false>, grid, dim3(256), 0, ctx->stream, pred, q, dec, d_list, H, W, Hp, Wp, vec);
    } else {
        if (flat) hipLaunchKernelGGL(k_cl_step<true>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, d_list, H, W, Hp, Wp, E, vec);
        else hipLaunchKernelGGL(k_cl_step<false>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, d_list, H, W, Hp, Wp, E, vec);
    }
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_cl_step(tz_ctx* ctx, const float* pred, const uint8_t* orig, uint8_t* dec, const int* d_list, int nlist, int H, int W, int Hp, int Wp,
                int E) {
    return cl_launch(ctx, pred, orig, nullptr, dec, d_list, nlist, H, W, Hp, Wp, E);
}

int tzk_cl_recon(tz_ctx* ctx, const float* pred, const int16_t* q, uint8_t* dec, const int* d_list, int nlist, int H, int W, int Hp, int Wp) {
    return cl_launch(ctx, pred, nullptr, q, dec, d_list, nlist, H, W, Hp, Wp, 0);
}

// ------------------------------------------------------------------------ closed loop, one abs bound per frame (TZ-CLF1)
// tz_rollout_closed_frames (include/tezip_hip.h; slow statement in tezip_amd/closedframes.py): TZ-CL1 with
// the radius E of a frame's own bound, given (E[nt]) or found while the loop stands at the frame: when a step's predictions
// exist, every candidate k of the bisection lo = 0, hi = 511, mid = (lo + hi) / 2, pass <=> sse(mid) <= limit is priced by one
// pass over (pred, orig) -- sse(k) = sum (clamp(x - Q_{k >> 1}(x - orig), 0, 255) - orig)^2, an exact integer.
//   k_clf_probe  round r for every frame of the step: a workgroup replays rounds 0 .. r - 1 of its frame from sse[round][frame]
//                (uniform scalar work), leaves at once when the interval has closed, else adds its samples' squared errors under
//                E = mid >> 1 to sse[r][frame].  Integer sums: no order shows.  Round r + 1 is the next launch; nothing else
//                synchronises.
//   k_clf_step   k_cl_step with the frame's E: E[frame], or lo >> 1 of the replay of all CLF_ROUNDS rounds, in which case one
//                lane per frame also leaves k = lo and sse(k) (0 for k = 0, which is never probed).
// Sample mapping, FLAT and vec as cl_frames.
constexpr int CLF_ROUNDS = TZ_CLF_ROUNDS;
constexpr int CLF_K_END = 511;   // candidates k = 0 .. 510
static_assert((1 << CLF_ROUNDS) >= CLF_K_END, "the interval [0, 511) closes within the rounds");

struct clf_interval {
    int lo, hi;
    unsigned long long sse_lo;
};

// the bisection of frame f after `rounds` rounds (those behind a closed interval did not run and are not read)
__device__ __forceinline__ clf_interval clf_replay(const unsigned long long* __restrict__ sse, int nt, size_t f, int rounds,
                                                   unsigned long long limit) {
    clf_interval s{0, CLF_K_END, 0ull};
    for (int i = 0; i < rounds && s.hi - s.lo > 1; ++i) {
        const int mid = (s.lo + s.hi) >> 1;
        const unsigned long long v = sse[(size_t)i * nt + f];
        if (v <= limit) {
            s.lo = mid;
            s.sse_lo = v;
        } else {
            s.hi = mid;
        }
    }
    return s;
}

__device__ __forceinline__ unsigned clf_err2(float p, int o, int E) {
    const int e = (int)cl_sample(p, o, E) - o;
    return (unsigned)(e * e);
}

template <bool FLAT>
__global__ __launch_bounds__(256) void k_clf_probe(const float* __restrict__ pred, const uint8_t* __restrict__ orig, const int* __restrict__ list,
                                                   int H, int W, int Hp, int Wp, int vec, int round, unsigned long long* __restrict__ sse,
                                                   int nt, unsigned long long limit) {
    const size_t f = (size_t)list[blockIdx.y];
    const clf_interval s = clf_replay(sse, nt, f, round, limit);
    if (s.hi - s.lo <= 1) return;   // (uniform: the whole workgroup leaves)
    const int E = ((s.lo + s.hi) >> 1) >> 1;
    const unsigned row = (unsigned)W * 3u, pitch = (unsigned)Wp * 3u;
    const size_t fe = (size_t)H * row, base = f * fe;
    const float* pf = pred + f * (size_t)Hp * pitch;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t head = vec ? min(fe, (size_t)((16u - (unsigned)(base & 15)) & 15u)) : fe;
    const size_t n16 = (fe - head) / 16;
    // a group's 16 squared errors are summed in 32 bits, everything wider in 64: no bound on the frame size is needed
    static_assert(16ull * 65025ull < (1ull << 32), "16 squared errors of at most 255^2 fit 32 bits");
    unsigned long long acc = 0;
    for (size_t g = t0; g < n16; g += stride) {
        const size_t r0 = head + 16 * g;
        float p[16];
        if (FLAT) {
            const float4* p4 = (const float4*)(pf + r0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 v = p4[j];
                p[4 * j] = v.x; p[4 * j + 1] = v.y; p[4 * j + 2] = v.z; p[4 * j + 3] = v.w;
            }
        } else {
            size_t y = r0 / row;
            unsigned xc = (unsigned)(r0 - y * row);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                p[j] = pf[y * pitch + xc];
                if (++xc == row) {
                    xc = 0;
                    ++y;
                }
            }
        }
        const uint4 o = *(const uint4*)(orig + base + r0);
        const unsigned w[4] = {o.x, o.y, o.z, o.w};
        unsigned part = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) part += clf_err2(p[j], (int)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu), E);
        acc += part;
    }
    const size_t v_end = head + 16 * n16, nscalar = head + (fe - v_end);
    for (size_t j = t0; j < nscalar; j += stride) {
        const size_t r = j < head ? j : v_end + (j - head);
        acc += clf_err2(cl_pred(pf, r, row, pitch), (int)orig[base + r], E);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&sse[(size_t)round * nt + f], acc);   // one 64-bit vector atomic a wave
}

template <bool FLAT>
__global__ __launch_bounds__(256) void k_clf_step(const float* __restrict__ pred, const uint8_t* __restrict__ orig, uint8_t* __restrict__ dec,
                                                  const int* __restrict__ list, int H, int W, int Hp, int Wp, int vec,
                                                  const int* __restrict__ radius, const unsigned long long* __restrict__ sse, int nt,
                                                  unsigned long long limit, int* __restrict__ k_out, unsigned long long* __restrict__ sse_out) {
    const size_t f = (size_t)list[blockIdx.y];
    int E;
    if (radius) {
        E = radius[f];
    } else {
        const clf_interval s = clf_replay(sse, nt, f, CLF_ROUNDS, limit);
        E = s.lo >> 1;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            k_out[f] = s.lo;
            sse_out[f] = s.sse_lo;
        }
    }
    cl_frames<false, FLAT>(pred, orig, nullptr, dec, list, H, W, Hp, Wp, E, vec);
}

static dim3 clf_grid(int nlist, int H, int W) {   // (cl_launch's)
    const size_t fe = (size_t)H * W * 3;
    return dim3((unsigned)std::max<size_t>(1, std::min<size_t>((fe / 16 + 255) / 256, 64)), (unsigned)nlist);
}

int tzk_clf_probe(tz_ctx* ctx, const float* pred, const uint8_t* orig, const int* d_list, int nlist, int H, int W, int Hp, int Wp, int round,
                  unsigned long long* d_sse, int nt, unsigned long long limit) {
    if (nlist <= 0) return TZ_OK;
    if (round < 0 || round >= CLF_ROUNDS) return tz_fail(ctx, TZ_ERR_INVALID, "tzk_clf_probe: round %d", round);
    const int vec = ((((uintptr_t)orig | (uintptr_t)pred) & 15) == 0) ? 1 : 0;
    const dim3 grid = clf_grid(nlist, H, W);
    tz_prof_scope ps(ctx, TZP_QUANT);
    if (vec && H == Hp && W == Wp)
        hipLaunchKernelGGL(k_clf_probe<true>, grid, dim3(256), 0, ctx->stream, pred, orig, d_list, H, W, Hp, Wp, vec, round, d_sse, nt, limit);
    else
        hipLaunchKernelGGL(k_clf_probe<false>, grid, dim3(256), 0, ctx->stream, pred, orig, d_list, H, W, Hp, Wp, vec, round, d_sse, nt, limit);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_clf_step(tz_ctx* ctx, const float* pred, const uint8_t* orig, uint8_t* dec, const int* d_list, int nlist, int H, int W, int Hp, int Wp,
                 const int* d_radius, const unsigned long long* d_sse, int nt, unsigned long long limit, int* d_k, unsigned long long* d_sse_out) {
    if (nlist <= 0) return TZ_OK;
    const int vec = ((((uintptr_t)dec | (uintptr_t)orig | (uintptr_t)pred) & 15) == 0) ? 1 : 0;
    const dim3 grid = clf_grid(nlist, H, W);
    tz_prof_scope ps(ctx, TZP_QUANT);
    if (vec && H == Hp && W == Wp)
        hipLaunchKernelGGL(k_clf_step<true>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, d_list, H, W, Hp, Wp, vec, d_radius, d_sse, nt,
                           limit, d_k, d_sse_out);
    else
        hipLaunchKernelGGL(k_clf_step<false>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, d_list, H, W, Hp, Wp, vec, d_radius, d_sse, nt,
                           limit, d_k, d_sse_out);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------------------------------ closed loop, one abs bound per pixel (TZ-CLM1)
// tz_rollout_closed_map (include/tezip_hip.h; slow statement in tezip_amd/closedmap.py): TZ-CL1 with the
// radius E = map[pixel] of the context's own H * W byte map (tz_set_bound_map), shared by every frame and channel and read through
// the cache.  k_clm_step takes k_cl_step's place.  A lane owns WHOLE pixels, so that its tolerances are one aligned load:
//   CLM_FLAT  (stacks on 16-byte boundaries, an unpadded frame: H * W is a multiple of 64)  group g = pixels 16 g .. 16 g + 15 of
//             the frame: one 16-byte load of the map, three of orig, twelve of pred, three 16-byte stores of dec
//   CLM_ROWS  (stacks on 16-byte boundaries, a padded frame whose W is a multiple of 16)  the same group inside one row of the
//             crop: pixel (y, x0) with y = g / (W / 16), x0 = 16 (g % (W / 16)); every address stays a 16-byte multiple
//   CLM_SCALAR (a stack off its boundary, or a W that does not divide)  one pixel a lane and trip, byte by byte
// The division (|d| + E) div (2 E + 1) has a divisor that varies per pixel: one v_rcp_f32 per pixel, shared by its three channels,
// and trunc((f32(|d| + E) + 0.5f) * r) per sample -- exact for every numerator and E the quantiser meets, whatever the last bit of
// r (closedmap.div_shortcut; tests/test_closedmap.py walks all 511 x 256 pairs with r one ulp either way).
enum { CLM_SCALAR = 0, CLM_FLAT = 1, CLM_ROWS = 2 };

__device__ __forceinline__ float clm_rcp(unsigned E) { return __builtin_amdgcn_rcpf((float)(2u * E + 1u)); }

__device__ __forceinline__ int clm_quant(int d, unsigned E, float r) {   // (ps_quant's q with the pixel's E)
    const unsigned ad = (unsigned)(d < 0 ? -d : d), s = 2u * E + 1u;
    const unsigned k = (unsigned)(((float)(ad + E) + 0.5f) * r);
    const int m = (int)min(k * s, 255u);
    return E ? (d < 0 ? -m : m) : d;
}

__device__ __forceinline__ unsigned clm_sample(float p, int o, unsigned E, float r) {
    const int x = (int)(p * 255.0f), v = x - clm_quant(x - o, E, r);
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

template <int FORM>
__global__ __launch_bounds__(256) void k_clm_step(const float* __restrict__ pred, const uint8_t* __restrict__ orig, uint8_t* __restrict__ dec,
                                                  const uint8_t* __restrict__ map, const int* __restrict__ list, int H, int W, int Hp, int Wp) {
    const size_t f = (size_t)list[blockIdx.y];
    const size_t npix = (size_t)H * W, base = f * npix * 3;
    const float* pf = pred + f * (size_t)Hp * Wp * 3;
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (FORM == CLM_SCALAR) {
        for (size_t i = t0; i < npix; i += stride) {
            const size_t y = i / (size_t)W, x = i - y * (size_t)W;
            const float* pp = pf + (y * Wp + x) * 3;
            const unsigned E = map[i];
            const float r = clm_rcp(E);
#pragma unroll
            for (int c = 0; c < 3; ++c) dec[base + 3 * i + c] = (uint8_t)clm_sample(pp[c], (int)orig[base + 3 * i + c], E, r);
        }
        return;
    }
    const size_t rowg = (size_t)W / 16;                                          // (CLM_ROWS: groups a row)
    const size_t ngroups = FORM == CLM_FLAT ? npix / 16 : (size_t)H * rowg;
    for (size_t g = t0; g < ngroups; g += stride) {
        size_t pix, pat;                                                         // first pixel in the unpadded stacks / in pred
        if (FORM == CLM_FLAT) {
            pix = pat = 16 * g;
        } else {
            const size_t y = g / rowg, x0 = 16 * (g - y * rowg);
            pix = y * W + x0;
            pat = y * Wp + x0;
        }
        const uint4 m4 = *(const uint4*)(map + pix);
        const unsigned mw[4] = {m4.x, m4.y, m4.z, m4.w};
        const uint4* o4 = (const uint4*)(orig + base + 3 * pix);
        const float4* p4 = (const float4*)(pf + 3 * pat);
        uint4* d4 = (uint4*)(dec + base + 3 * pix);
#pragma unroll
        for (int h = 0; h < 3; ++h) {                                            // 16 samples = pixels 5 1/3 h .. of the group
            const uint4 o = o4[h];
            const unsigned ow[4] = {o.x, o.y, o.z, o.w};
            float p[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 v = p4[4 * h + j];
                p[4 * j] = v.x; p[4 * j + 1] = v.y; p[4 * j + 2] = v.z; p[4 * j + 3] = v.w;
            }
            unsigned b[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int px = (16 * h + j) / 3;                                 // (a constant after unrolling)
                const unsigned E = (mw[px >> 2] >> (8 * (px & 3))) & 0xFFu;
                b[j] = clm_sample(p[j], (int)((ow[j >> 2] >> (8 * (j & 3))) & 0xFFu), E, clm_rcp(E));   // (one rcp a pixel after CSE)
            }
            uint4 out;
            out.x = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            out.y = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            out.z = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
            out.w = b[12] | (b[13] << 8) | (b[14] << 16) | (b[15] << 24);
            d4[h] = out;
        }
    }
}

// d_map: the H * W byte map (device).  FLAT / vec are chosen as cl_launch chooses them; the grid is cl_launch's.
int tzk_clm_step(tz_ctx* ctx, const float* pred, const uint8_t* orig, uint8_t* dec, const uint8_t* d_map, const int* d_list, int nlist, int H,
                 int W, int Hp, int Wp) {
    if (nlist <= 0) return TZ_OK;
    const bool vec = (((uintptr_t)dec | (uintptr_t)orig | (uintptr_t)pred | (uintptr_t)d_map) & 15) == 0;
    const int form = vec && H == Hp && W == Wp ? CLM_FLAT : (vec && W % 16 == 0 ? CLM_ROWS : CLM_SCALAR);
    const dim3 grid = clf_grid(nlist, H, W);
    tz_prof_scope ps(ctx, TZP_QUANT);
    if (form == CLM_FLAT) hipLaunchKernelGGL(k_clm_step<CLM_FLAT>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, d_map, d_list, H, W, Hp, Wp);
    else if (form == CLM_ROWS) hipLaunchKernelGGL(k_clm_step<CLM_ROWS>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, d_map, d_list, H, W, Hp, Wp);
    else hipLaunchKernelGGL(k_clm_step<CLM_SCALAR>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, d_map, d_list, H, W, Hp, Wp);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// ------------------------------------------------------------------------ per-tile choice of the prediction (TZ-PS1)
// tz_set_pred_select (include/tezip_hip.h; slow statement in tezip_amd/predselect.py): in a closed loop every
// 16 x 16 tile of a predicted frame takes whichever of x_net = (int)(pred * 255.0f) and x_prev = dec[t-1] leaves the smaller
// sum |Q(x - orig)| over its samples inside H x W (a tie goes to the network), one mode byte per tile says which, and a tile that
// took the frame in front is EXPRESSED in the prediction stack so that the back half, which forms x from that stack, needs no change:
//   pv(v) = (v + 0.5f) / 255.0f for v < 255, 1.0f for v = 255:  (int)(pv(v) * 255.0f) == v for all 256 values in float32 with the
//   correctly rounded divide this library is built with (tests/test_predselect.py walks them; the unguarded formula gives a value
//   above 1.0 at v = 255 alone).  Samples of the padded stack outside H x W stay as the network left them.
//   k_ps_select (lossless encoder)     prev = orig[t-1], Q the identity (E = 0): mode byte, patched pred; nothing else is written
//   k_ps_step   (lossy encoder)        prev = dec[t-1], Q = TZ-QL1(E) as cl_sample forms it: mode byte, patched pred and dec[t]
//   k_ps_recon  (decoder)              the mode byte picks x: dec[t] = clamp(x - q, 0, 255), patched pred; nothing to reduce
// Mapping: a workgroup of 256 lanes owns a strip of PS_STRIP = 4 tiles of one tile row, 16 rows of 64 pixels.  A lane holds 4
// pixels = 12 samples of one row (three 16-byte loads of pred, whose pitch and x0 * 3 floats are 16-byte multiples for any shape;
// three 4-byte loads of each u8 stack where W is a multiple of 4 and the stacks sit on 4-byte boundaries, VEC, else byte by byte
// with the crop checked per sample), 16 consecutive lanes cover 768 contiguous bytes of a pred row, a wave covers 4 rows, the 4 waves
// the 16 rows.  The lanes of a tile inside a wave are 4 neighbours in each of 4 rows: lane bits 0, 1, 4, 5, summed with four
// __shfl_xor; the four waves' partial sums meet in LDS (two buffers by the trip's parity: one barrier a trip).  blockIdx.y walks
// `list`, blockIdx.x the strips of a frame in a grid-stride loop (at most PS_GRID workgroups a frame).
enum { PS_SELECT = 0, PS_STEP = 1, PS_RECON = 2 };
constexpr int PS_TILE = 16, PS_STRIP = 4, PS_GRID = 64;

__device__ __forceinline__ int ps_quant(int d, int E) {   // (cl_sample's q)
    const unsigned ad = (unsigned)(d < 0 ? -d : d), s = 2u * (unsigned)E + 1u;
    const int m = (int)min((ad + (unsigned)E) / s * s, 255u);
    return E ? (d < 0 ? -m : m) : d;
}

__device__ __forceinline__ float ps_pv(unsigned v) { return v == 255u ? 1.0f : ((float)v + 0.5f) / 255.0f; }

// MAP (TZ-CLM1, tz_rollout_closed_map): Q takes the pixel's own E = map[y * W + x] in place of the uniform one -- the lane's four
// tolerances are one 4-byte load where VEC holds, else byte by byte with the crop check -- and divides by clm_quant's reciprocal,
// one per pixel.  Without MAP the map is never read and the instruction stream is what it was.
template <int KIND, bool VEC, bool MAP = false>
__device__ __forceinline__ void ps_strips(float* pred, const uint8_t* orig, const uint8_t* prev, const int16_t* __restrict__ qs, uint8_t* dec,
                                          uint8_t* modes, const int* __restrict__ list, int H, int W, int Hp, int Wp, int TH, int TW, int E,
                                          const uint8_t* __restrict__ map = nullptr) {
    __shared__ unsigned s_cost[2][4][PS_STRIP][2];
    const int f = list[blockIdx.y];
    const unsigned row = (unsigned)W * 3u, pitch = (unsigned)Wp * 3u;
    const size_t fe = (size_t)H * row;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tis = (lane >> 2) & 3;                       // the lane's tile inside the strip
    const int SW = (TW + PS_STRIP - 1) / PS_STRIP, nstrips = TH * SW;
    int par = 0;
    for (int s = blockIdx.x; s < nstrips; s += gridDim.x, par ^= 1) {
        const int ty = s / SW, sx = s - ty * SW;
        const int tx = sx * PS_STRIP + tis;
        const int y = ty * PS_TILE + wave * 4 + (lane >> 4), x0 = sx * (PS_STRIP * PS_TILE) + (lane & 15) * 4;
        const bool active = y < H && x0 < W;
        const int ns = active ? min(4, W - x0) * 3 : 0;     // the lane's samples inside the frame (VEC: 12 or 0)
        float* pf = pred + (size_t)f * Hp * pitch + (size_t)y * pitch + (size_t)x0 * 3;
        const size_t at = (size_t)f * fe + (size_t)y * row + (size_t)x0 * 3;     // in the unpadded stacks
        int xn[12], o[12], v[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) xn[j] = o[j] = v[j] = 0;
        unsigned pe[4] = {0u, 0u, 0u, 0u};                   // MAP: the tolerances of the lane's pixels and 1 / (2 E + 1)
        float pr[4] = {1.0f, 1.0f, 1.0f, 1.0f};
        if (active) {
            const float4 a = ((const float4*)pf)[0], b = ((const float4*)pf)[1], c = ((const float4*)pf)[2];
            const float p[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
#pragma unroll
            for (int j = 0; j < 12; ++j) xn[j] = (int)(p[j] * 255.0f);
            if (MAP) {
                const size_t mat = (size_t)y * W + x0;
                if (VEC) {
                    const unsigned mw = *(const unsigned*)(map + mat);
#pragma unroll
                    for (int i = 0; i < 4; ++i) pe[i] = (mw >> (8 * i)) & 0xFFu;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (3 * i < ns) pe[i] = map[mat + i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) pr[i] = clm_rcp(pe[i]);
            }
            if (VEC) {
                const unsigned* pw = (const unsigned*)(prev + at - fe);
                const unsigned w0[3] = {pw[0], pw[1], pw[2]};
#pragma unroll
                for (int j = 0; j < 12; ++j) v[j] = (int)((w0[j >> 2] >> (8 * (j & 3))) & 0xFFu);
                if (KIND != PS_RECON) {
                    const unsigned* ow = (const unsigned*)(orig + at);
                    const unsigned w1[3] = {ow[0], ow[1], ow[2]};
#pragma unroll
                    for (int j = 0; j < 12; ++j) o[j] = (int)((w1[j >> 2] >> (8 * (j & 3))) & 0xFFu);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    if (j < ns) {
                        v[j] = (int)prev[at - fe + j];
                        if (KIND != PS_RECON) o[j] = (int)orig[at + j];
                    }
            }
        }
        bool m;
        if (KIND == PS_RECON) {
            m = active && modes[((size_t)f * TH + ty) * TW + tx] != 0;     // (an active lane's tile is inside the frame)
        } else {
            unsigned cn = 0, cp = 0;
#pragma unroll
            for (int j = 0; j < 12; ++j)
                if (j < ns) {
                    const int qn = MAP ? clm_quant(xn[j] - o[j], pe[j / 3], pr[j / 3]) : ps_quant(xn[j] - o[j], E);
                    const int qp = MAP ? clm_quant(v[j] - o[j], pe[j / 3], pr[j / 3]) : ps_quant(v[j] - o[j], E);
                    cn += (unsigned)(qn < 0 ? -qn : qn);
                    cp += (unsigned)(qp < 0 ? -qp : qp);
                }
            cn += (unsigned)__shfl_xor((int)cn, 1);  cp += (unsigned)__shfl_xor((int)cp, 1);
            cn += (unsigned)__shfl_xor((int)cn, 2);  cp += (unsigned)__shfl_xor((int)cp, 2);
            cn += (unsigned)__shfl_xor((int)cn, 16); cp += (unsigned)__shfl_xor((int)cp, 16);
            cn += (unsigned)__shfl_xor((int)cn, 32); cp += (unsigned)__shfl_xor((int)cp, 32);
            if ((lane & 0x33) == 0) {
                s_cost[par][wave][tis][0] = cn;
                s_cost[par][wave][tis][1] = cp;
            }
            __syncthreads();
            cn = s_cost[par][0][tis][0] + s_cost[par][1][tis][0] + s_cost[par][2][tis][0] + s_cost[par][3][tis][0];
            cp = s_cost[par][0][tis][1] + s_cost[par][1][tis][1] + s_cost[par][2][tis][1] + s_cost[par][3][tis][1];
            m = cp < cn;                                    // a tie goes to the network
            if (wave == 0 && (lane & 0x33) == 0 && tx < TW) modes[((size_t)f * TH + ty) * TW + tx] = m ? 1 : 0;
        }
        if (!active) continue;
        if (KIND != PS_SELECT) {
            unsigned b[12];
            if (KIND == PS_RECON) {
                int q[12];
                if (VEC) {
                    const uint2* q2 = (const uint2*)(qs + at);
                    const uint2 q0 = q2[0], q1 = q2[1], q3 = q2[2];
                    const unsigned w2[6] = {q0.x, q0.y, q1.x, q1.y, q3.x, q3.y};
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        q[2 * j] = (int)(short)(w2[j] & 0xFFFFu);
                        q[2 * j + 1] = (int)w2[j] >> 16;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 12; ++j) q[j] = j < ns ? (int)qs[at + j] : 0;
                }
#pragma unroll
                for (int j = 0; j < 12; ++j) {
                    const int r = (m ? v[j] : xn[j]) - q[j];
                    b[j] = (unsigned)(r < 0 ? 0 : (r > 255 ? 255 : r));
                }
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j) {
                    const int x = m ? v[j] : xn[j], r = x - (MAP ? clm_quant(x - o[j], pe[j / 3], pr[j / 3]) : ps_quant(x - o[j], E));
                    b[j] = (unsigned)(r < 0 ? 0 : (r > 255 ? 255 : r));
                }
            }
            if (VEC) {
                unsigned* dw = (unsigned*)(dec + at);
#pragma unroll
                for (int j = 0; j < 3; ++j) dw[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    if (j < ns) dec[at + j] = (uint8_t)b[j];
            }
        }
        if (m) {   // the chosen tile in the prediction stack: pv of the frame in front, inside H x W only
            if (VEC) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    ((float4*)pf)[j] = make_float4(ps_pv((unsigned)v[4 * j]), ps_pv((unsigned)v[4 * j + 1]), ps_pv((unsigned)v[4 * j + 2]),
                                                   ps_pv((unsigned)v[4 * j + 3]));
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    if (j < ns) pf[j] = ps_pv((unsigned)v[j]);
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_ps_select(float* pred, const uint8_t* orig, uint8_t* modes, const int* __restrict__ list, int H, int W,
                                                   int Hp, int Wp, int TH, int TW) {
    ps_strips<PS_SELECT, VEC>(pred, orig, orig, nullptr, nullptr, modes, list, H, W, Hp, Wp, TH, TW, 0);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_ps_step(float* pred, const uint8_t* orig, uint8_t* dec, uint8_t* modes, const int* __restrict__ list,
                                                 int H, int W, int Hp, int Wp, int TH, int TW, int E) {
    ps_strips<PS_STEP, VEC>(pred, orig, dec, nullptr, dec, modes, list, H, W, Hp, Wp, TH, TW, E);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_ps_recon(float* pred, const int16_t* __restrict__ qs, uint8_t* dec, const uint8_t* modes,
                                                  const int* __restrict__ list, int H, int W, int Hp, int Wp, int TH, int TW) {
    ps_strips<PS_RECON, VEC>(pred, nullptr, dec, qs, dec, const_cast<uint8_t*>(modes), list, H, W, Hp, Wp, TH, TW, 0);
}

// TZ-CLM1: k_ps_step with Q under the map.  A map that is zero in some region only is still lossy and comes here; the all-zero map
// is the lossless job and takes k_ps_select as it is, so k_ps_select has no map form: nothing would launch it.
template <bool VEC>
__global__ __launch_bounds__(256) void k_psm_step(float* pred, const uint8_t* orig, uint8_t* dec, uint8_t* modes, const uint8_t* __restrict__ map,
                                                  const int* __restrict__ list, int H, int W, int Hp, int Wp, int TH, int TW) {
    ps_strips<PS_STEP, VEC, true>(pred, orig, dec, nullptr, dec, modes, list, H, W, Hp, Wp, TH, TW, 0, map);
}

int tzk_ps_grid(int H, int W) {
    const int TH = (H + PS_TILE - 1) / PS_TILE, TW = (W + PS_TILE - 1) / PS_TILE;
    return std::min(TH * ((TW + PS_STRIP - 1) / PS_STRIP), (int)PS_GRID);
}

// d_list: nlist sequence indices (device); every stack is the whole sequence's; modes: nt * TH * TW bytes (device).
static int ps_launch(tz_ctx* ctx, int kind, float* pred, const uint8_t* orig, const int16_t* q, uint8_t* dec, uint8_t* modes, const int* d_list,
                     int nlist, int H, int W, int Hp, int Wp, int E) {
    if (nlist <= 0) return TZ_OK;
    const int TH = (H + PS_TILE - 1) / PS_TILE, TW = (W + PS_TILE - 1) / PS_TILE;
    const bool vec = W % 4 == 0 && (((uintptr_t)orig | (uintptr_t)dec) & 3) == 0 && ((uintptr_t)q & 7) == 0;
    if ((uintptr_t)pred & 15) return tz_fail(ctx, TZ_ERR_INVALID, "the prediction stack is off the 16-byte boundary");
    const dim3 grid((unsigned)tzk_ps_grid(H, W), (unsigned)nlist);
    tz_prof_scope ps(ctx, kind == PS_RECON ? TZP_RECON : TZP_QUANT);
    if (kind == PS_SELECT) {
        if (vec) hipLaunchKernelGGL(k_ps_select<true>, grid, dim3(256), 0, ctx->stream, pred, orig, modes, d_list, H, W, Hp, Wp, TH, TW);
        else hipLaunchKernelGGL(k_ps_select<false>, grid, dim3(256), 0, ctx->stream, pred, orig, modes, d_list, H, W, Hp, Wp, TH, TW);
    } else if (kind == PS_STEP) {
        if (vec) hipLaunchKernelGGL(k_ps_step<true>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, modes, d_list, H, W, Hp, Wp, TH, TW, E);
        else hipLaunchKernelGGL(k_ps_step<false>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, modes, d_list, H, W, Hp, Wp, TH, TW, E);
    } else {
        if (vec) hipLaunchKernelGGL(k_ps_recon<true>, grid, dim3(256), 0, ctx->stream, pred, q, dec, (const uint8_t*)modes, d_list, H, W, Hp, Wp, TH, TW);
        else hipLaunchKernelGGL(k_ps_recon<false>, grid, dim3(256), 0, ctx->stream, pred, q, dec, (const uint8_t*)modes, d_list, H, W, Hp, Wp, TH, TW);
    }
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_ps_select(tz_ctx* ctx, float* pred, const uint8_t* orig, uint8_t* modes, const int* d_list, int nlist, int H, int W, int Hp, int Wp) {
    return ps_launch(ctx, PS_SELECT, pred, orig, nullptr, nullptr, modes, d_list, nlist, H, W, Hp, Wp, 0);
}

int tzk_ps_step(tz_ctx* ctx, float* pred, const uint8_t* orig, uint8_t* dec, uint8_t* modes, const int* d_list, int nlist, int H, int W, int Hp,
                int Wp, int E) {
    return ps_launch(ctx, PS_STEP, pred, orig, nullptr, dec, modes, d_list, nlist, H, W, Hp, Wp, E);
}

int tzk_psm_step(tz_ctx* ctx, float* pred, const uint8_t* orig, uint8_t* dec, uint8_t* modes, const uint8_t* d_map, const int* d_list, int nlist,
                 int H, int W, int Hp, int Wp) {
    if (nlist <= 0) return TZ_OK;
    const int TH = (H + PS_TILE - 1) / PS_TILE, TW = (W + PS_TILE - 1) / PS_TILE;
    const bool vec = W % 4 == 0 && (((uintptr_t)orig | (uintptr_t)dec | (uintptr_t)d_map) & 3) == 0;   // (ps_launch's rule, and the map's words)
    if ((uintptr_t)pred & 15) return tz_fail(ctx, TZ_ERR_INVALID, "the prediction stack is off the 16-byte boundary");
    const dim3 grid((unsigned)tzk_ps_grid(H, W), (unsigned)nlist);
    tz_prof_scope ps(ctx, TZP_QUANT);
    if (vec) hipLaunchKernelGGL(k_psm_step<true>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, modes, d_map, d_list, H, W, Hp, Wp, TH, TW);
    else hipLaunchKernelGGL(k_psm_step<false>, grid, dim3(256), 0, ctx->stream, pred, orig, dec, modes, d_map, d_list, H, W, Hp, Wp, TH, TW);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_ps_recon(tz_ctx* ctx, float* pred, const int16_t* q, uint8_t* dec, const uint8_t* modes, const int* d_list, int nlist, int H, int W,
                 int Hp, int Wp) {
    return ps_launch(ctx, PS_RECON, pred, nullptr, q, dec, const_cast<uint8_t*>(modes), d_list, nlist, H, W, Hp, Wp, 0);
}

// ------------------------------------------------------------------------ motion-compensated tiles (TZ-PM1)
// tz_set_pred_motion (include/tezip_hip.h; slow statement in tezip_amd/predmotion.py): TZ-PS1's tiles and
// modes, but the second candidate is the frame in front DISPLACED by a vector (dy, dx), -7 <= dy, dx <= 7, found per tile:
//   ref(y, x, c) = prev[clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1), c];  SAD(dy, dx) = sum |ref - orig| over the tile's
//   samples inside H x W (raw u8 values: the search does not depend on the quantiser);  the vector is the one with the smallest
//   key = SAD * 4096 + (|dy| + |dx|) * 256 + (dy + 7) * 16 + (dx + 7) (below 2^30; no two vectors share a key, so the minimum does
//   not depend on the order of the reduction);  mode 1 iff sum |Q(ref - orig)| < sum |Q(x_net - orig)|, a tie goes to the network.
// A chosen tile is expressed in the prediction stack as ps_pv(ref); a tile of mode 0 has vector (0, 0).
//   k_pm_select (lossless encoder)     prev = orig[t-1], Q the identity: mode byte, vector, patched pred
//   k_pm_step   (lossy encoder)        prev = dec[t-1], Q = TZ-QL1(E): mode byte, vector, patched pred and dec[t]
//   k_pm_recon  (decoder)              mode byte and vector pick x (a gather, no search): dec[t] = clamp(x - q, 0, 255), patched pred
// Mapping: a workgroup of 256 lanes owns one tile; blockIdx.y walks `list`, blockIdx.x the tiles of a frame in a grid-stride loop
// (at most PM_GRID workgroups a frame).  The encoders stage the tile of orig (16 rows of 12 words, samples outside the frame as 0)
// and the 30 x 30 pixel window of prev around it (30 rows of 90 bytes in a pitch of 23 words, coordinates clamped WHILE staging:
// the search has no bounds logic) in LDS.  Lanes 0 .. 224 own one vector each: per tile row 12 words of the window at byte
// offset (dx + 7) * 3, each formed from two aligned LDS words by v_alignbyte_b32, against the 12 words of orig with v_sad_u8; a
// ragged tile limits the rows and the words and masks the last word.  The minimum key is taken per wave by __shfl_xor and over
// the waves by an LDS atomic.  Then lane (row, pixel) forms its three samples of x_net and of ref (from the LDS window), the two
// costs are summed as in ps_strips, and lane 0 writes mode and vector.  One path serves every W and alignment: the u8 stacks are
// read and written byte by byte (the window's left edge, (x0 - 7) * 3 bytes, is on no word boundary anyway).
enum { PM_SELECT = 0, PM_STEP = 1 };
constexpr int PM_R = 7, PM_WIN = PS_TILE + 2 * PM_R, PM_ROWW = 23, PM_GRID = 128;

template <int KIND>
__device__ __forceinline__ void pm_tiles(float* pred, const uint8_t* __restrict__ orig, const uint8_t* prev, uint8_t* dec, uint8_t* modes,
                                         int8_t* vecs, const int* __restrict__ list, int H, int W, int Hp, int Wp, int TH, int TW, int E) {
    __shared__ unsigned s_o[PS_TILE * 12];
    __shared__ unsigned s_r[PM_WIN * PM_ROWW];
    __shared__ unsigned s_key;
    __shared__ unsigned s_cost[4][2];
    const int f = list[blockIdx.y];
    const unsigned row = (unsigned)W * 3u, pitch = (unsigned)Wp * 3u;
    const size_t fe = (size_t)H * row;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ly = tid >> 4, lx = tid & 15;               // the lane's pixel inside the tile
    const uint8_t* pframe = prev + (size_t)(f - 1) * fe;  // (a predicted frame has a frame in front: frame 0 is a key frame)
    uint8_t* ob = (uint8_t*)s_o;
    uint8_t* rb = (uint8_t*)s_r;
    for (int t = blockIdx.x; t < TH * TW; t += gridDim.x) {
        const int ty = t / TW, tx = t - ty * TW;
        const int y0 = ty * PS_TILE, x0 = tx * PS_TILE;
        const int nrows = min(PS_TILE, H - y0), nbytes = min(PS_TILE, W - x0) * 3;   // what the tile owns
        const int nwords = (nbytes + 3) >> 2;
        const unsigned lastmask = (nbytes & 3) ? (1u << (8 * (nbytes & 3))) - 1u : 0xFFFFFFFFu;
        const int y = y0 + ly, x = x0 + lx;
        const bool active = y < H && x < W;
        const size_t at = active ? (size_t)f * fe + (size_t)y * row + (size_t)x * 3 : 0;   // (formed inside the frame only)
        int o[3] = {0, 0, 0};
        if (active) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = (int)orig[at + c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) ob[ly * 48 + lx * 3 + c] = (uint8_t)o[c];
        for (int i = tid; i < PM_WIN * PM_ROWW * 4; i += 256) {
            const int r = i / (PM_ROWW * 4), b = i - r * (PM_ROWW * 4);
            const int px = b / 3, c = b - px * 3;
            const int yy = min(max(y0 - PM_R + r, 0), H - 1), xx = min(max(x0 - PM_R + px, 0), W - 1);
            rb[i] = b < PM_WIN * 3 ? pframe[(size_t)yy * row + (size_t)xx * 3 + c] : (uint8_t)0;
        }
        if (tid == 0) s_key = 0xFFFFFFFFu;
        __syncthreads();
        unsigned key = 0xFFFFFFFFu;                         // (idle lanes)
        if (tid < (2 * PM_R + 1) * (2 * PM_R + 1)) {
            const int vy = tid / (2 * PM_R + 1), vx = tid - vy * (2 * PM_R + 1);
            const int dy = vy - PM_R, dx = vx - PM_R;
            const int off = vx * 3, wb = off >> 2;
            const unsigned sh = (unsigned)(off & 3);
            unsigned sad = 0;
            for (int r = 0; r < nrows; ++r) {
                const unsigned* rw = s_r + (r + vy) * PM_ROWW + wb;   // window row r + dy + 7
                const unsigned* ow = s_o + r * 12;
                unsigned lo = rw[0];
                for (int j = 0; j < nwords; ++j) {
                    const unsigned hi = rw[j + 1];                    // (at most word 10 + 12 = 22 of the row's 23)
                    unsigned wv = __builtin_amdgcn_alignbyte(hi, lo, sh);
                    if (j == nwords - 1) wv &= lastmask;
                    sad = __builtin_amdgcn_sad_u8(wv, ow[j], sad);
                    lo = hi;
                }
            }
            key = sad * 4096u + (unsigned)((dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx)) * 256u + (unsigned)vy * 16u + (unsigned)vx;
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) key = min(key, (unsigned)__shfl_xor((int)key, d));
        if (lane == 0) atomicMin(&s_key, key);
        __syncthreads();
        key = s_key;
        const int vy = (int)((key >> 4) & 15u), vx = (int)(key & 15u);
        int xn[3] = {0, 0, 0}, v[3] = {0, 0, 0};
        float* pf = active ? pred + (size_t)f * Hp * pitch + (size_t)y * pitch + (size_t)x * 3 : pred;
        unsigned cn = 0, cp = 0;
        if (active) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                xn[c] = (int)(pf[c] * 255.0f);
                v[c] = (int)rb[(ly + vy) * (PM_ROWW * 4) + (lx + vx) * 3 + c];
                const int qn = ps_quant(xn[c] - o[c], E), qp = ps_quant(v[c] - o[c], E);
                cn += (unsigned)(qn < 0 ? -qn : qn);
                cp += (unsigned)(qp < 0 ? -qp : qp);
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            cn += (unsigned)__shfl_xor((int)cn, d);
            cp += (unsigned)__shfl_xor((int)cp, d);
        }
        if (lane == 0) {
            s_cost[wave][0] = cn;
            s_cost[wave][1] = cp;
        }
        __syncthreads();
        cn = s_cost[0][0] + s_cost[1][0] + s_cost[2][0] + s_cost[3][0];
        cp = s_cost[0][1] + s_cost[1][1] + s_cost[2][1] + s_cost[3][1];
        const bool m = cp < cn;                             // a tie goes to the network
        if (tid == 0) {
            const size_t ti = ((size_t)f * TH + ty) * TW + tx;
            modes[ti] = m ? 1 : 0;
            vecs[2 * ti] = (int8_t)(m ? vy - PM_R : 0);
            vecs[2 * ti + 1] = (int8_t)(m ? vx - PM_R : 0);
        }
        if (active) {
            if (KIND == PM_STEP) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int xv = m ? v[c] : xn[c], r = xv - ps_quant(xv - o[c], E);
                    dec[at + c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
                }
            }
            if (m) {   // the chosen tile in the prediction stack: pv of the displaced frame in front, inside H x W only
#pragma unroll
                for (int c = 0; c < 3; ++c) pf[c] = ps_pv((unsigned)v[c]);
            }
        }
        __syncthreads();                                    // the next trip stages into the same LDS
    }
}

__global__ __launch_bounds__(256) void k_pm_select(float* pred, const uint8_t* orig, uint8_t* modes, int8_t* vecs, const int* __restrict__ list,
                                                   int H, int W, int Hp, int Wp, int TH, int TW) {
    pm_tiles<PM_SELECT>(pred, orig, orig, nullptr, modes, vecs, list, H, W, Hp, Wp, TH, TW, 0);
}

__global__ __launch_bounds__(256) void k_pm_step(float* pred, const uint8_t* orig, uint8_t* dec, uint8_t* modes, int8_t* vecs,
                                                 const int* __restrict__ list, int H, int W, int Hp, int Wp, int TH, int TW, int E) {
    pm_tiles<PM_STEP>(pred, orig, dec, dec, modes, vecs, list, H, W, Hp, Wp, TH, TW, E);
}

// the decoder: lane (row, pixel) of a tile's workgroup gathers its three displaced samples of dec[t-1] where the mode byte is set
__global__ __launch_bounds__(256) void k_pm_recon(float* pred, const int16_t* __restrict__ qs, uint8_t* dec, const uint8_t* __restrict__ modes,
                                                  const int8_t* __restrict__ vecs, const int* __restrict__ list, int H, int W, int Hp, int Wp,
                                                  int TH, int TW) {
    const int f = list[blockIdx.y];
    const unsigned row = (unsigned)W * 3u, pitch = (unsigned)Wp * 3u;
    const size_t fe = (size_t)H * row;
    const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
    for (int t = blockIdx.x; t < TH * TW; t += gridDim.x) {
        const int ty = t / TW, tx = t - ty * TW;
        const int y = ty * PS_TILE + ly, x = tx * PS_TILE + lx;
        if (y >= H || x >= W) continue;
        const size_t ti = ((size_t)f * TH + ty) * TW + tx;
        const bool m = modes[ti] != 0;
        const size_t at = (size_t)f * fe + (size_t)y * row + (size_t)x * 3;
        float* pf = pred + (size_t)f * Hp * pitch + (size_t)y * pitch + (size_t)x * 3;
        int xv[3];
        if (m) {
            const int yy = min(max(y + (int)vecs[2 * ti], 0), H - 1), xx = min(max(x + (int)vecs[2 * ti + 1], 0), W - 1);
            const uint8_t* src = dec + (size_t)(f - 1) * fe + (size_t)yy * row + (size_t)xx * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                xv[c] = (int)src[c];
                pf[c] = ps_pv((unsigned)xv[c]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) xv[c] = (int)(pf[c] * 255.0f);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int r = xv[c] - (int)qs[at + c];
            dec[at + c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
        }
    }
}

int tzk_pm_grid(int H, int W) {
    const int TH = (H + PS_TILE - 1) / PS_TILE, TW = (W + PS_TILE - 1) / PS_TILE;
    return std::min(TH * TW, (int)PM_GRID);
}

// d_list: nlist sequence indices (device); every stack is the whole sequence's; modes: nt * TH * TW bytes, vecs: twice that (device).
int tzk_pm_select(tz_ctx* ctx, float* pred, const uint8_t* orig, uint8_t* modes, int8_t* vecs, const int* d_list, int nlist, int H, int W,
                  int Hp, int Wp) {
    if (nlist <= 0) return TZ_OK;
    const int TH = (H + PS_TILE - 1) / PS_TILE, TW = (W + PS_TILE - 1) / PS_TILE;
    tz_prof_scope ps(ctx, TZP_QUANT);
    hipLaunchKernelGGL(k_pm_select, dim3((unsigned)tzk_pm_grid(H, W), (unsigned)nlist), dim3(256), 0, ctx->stream, pred, orig, modes, vecs, d_list,
                       H, W, Hp, Wp, TH, TW);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_pm_step(tz_ctx* ctx, float* pred, const uint8_t* orig, uint8_t* dec, uint8_t* modes, int8_t* vecs, const int* d_list, int nlist, int H,
                int W, int Hp, int Wp, int E) {
    if (nlist <= 0) return TZ_OK;
    const int TH = (H + PS_TILE - 1) / PS_TILE, TW = (W + PS_TILE - 1) / PS_TILE;
    tz_prof_scope ps(ctx, TZP_QUANT);
    hipLaunchKernelGGL(k_pm_step, dim3((unsigned)tzk_pm_grid(H, W), (unsigned)nlist), dim3(256), 0, ctx->stream, pred, orig, dec, modes, vecs,
                       d_list, H, W, Hp, Wp, TH, TW, E);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

int tzk_pm_recon(tz_ctx* ctx, float* pred, const int16_t* q, uint8_t* dec, const uint8_t* modes, const int8_t* vecs, const int* d_list,
                 int nlist, int H, int W, int Hp, int Wp) {
    if (nlist <= 0) return TZ_OK;
    const int TH = (H + PS_TILE - 1) / PS_TILE, TW = (W + PS_TILE - 1) / PS_TILE;
    tz_prof_scope ps(ctx, TZP_RECON);
    hipLaunchKernelGGL(k_pm_recon, dim3((unsigned)tzk_pm_grid(H, W), (unsigned)nlist), dim3(256), 0, ctx->stream, pred, q, dec, modes, vecs,
                       d_list, H, W, Hp, Wp, TH, TW);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}
