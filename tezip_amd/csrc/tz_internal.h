// Internal declarations shared by the translation units of libtezip_hip.so (gfx950 only).
#pragma once
#include <assert.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/tezip_hip.h"

#define TZ_SENTINEL ((int16_t)0x7FFF)

enum tz_prof_class {
    TZP_CONV = 0,   // implicit-GEMM MFMA convolutions (all PredNet convs)
    TZP_ERR0,       // level-0 error unit
    TZP_DELTA,      // pred/orig -> int16 delta
    TZP_QUANT,      // error-bound quantiser kernels
    TZP_SDELTA,     // spatial delta (+offset, histogram)
    TZP_LUT,        // rank remap / unmap
    TZP_SCAN,       // inverse spatial delta (prefix scan)
    TZP_RECON,      // reconstruct
    TZP_SSE,        // window MSE partial sums
    // sub-classes of TZP_CONV (a launch is counted in TZP_CONV and in exactly one of these)
    TZP_CONV16,     // k_conv16: LDS-DMA kernel, sources with a multiple of 16 channels (levels >= 1)
    TZP_CONV16B,    // k_conv16b: level-0 block-step kernel
    TZP_CONV_SMALL, // k_conv_small: direct VALU 3 -> 3 convolution
    TZP_CONV_GEN,   // k_conv3x3: general kernel
    TZP_CONVLAT,    // k_convlat: one accumulator tile per wave, for grids that cannot fill the chip
    TZP_WINO,       // k_wino: TZ-PA2 form (Winograd F(2x2, 3x3) on the same-resolution source) of the k_conv16 convolutions
    TZP_TABLE,      // HOST time: rank table + LUT from the downloaded histogram (compress.py:356-361)
    TZP_QSERIAL,    // not a time: `launches` counts the chains the quantiser sent through its serial fallback (k_q_serial)
    TZP_CARRY,      // prefix carry of the inverse scan (k_undelta_carry, tz_decode_range)
    TZP_QUALITY,    // reconstruction statistics of an encode (k_quality, tz_encode_quality; k_ssim, tz_encode_ssim / tz_ssim_frames;
                    // k_bound_err, tz_bound_probe / tz_bound_err)
    TZP_HUFF,       // opt-in Huffman coder: k_huff_count / k_huff_size / k_huff_scan / k_huff_enc / k_huff_dec (and k_huffr_*),
                    // and the key-frame coders in front of it: k_key_hist / k_key_gray / k_key_resid / k_key_unresid_*
    TZP_DIGEST,     // per-frame digests TZD64 (k_digest: tz_frame_digests, tz_decoded_digests, tz_encode_digests)
    TZP_COUNT
};

struct tz_model;      // tz_prednet.hip

struct tz_prof_slot {
    double total_ms = 0;
    long long launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    std::vector<int> pending_sub;  // parallel to `pending`: second class of the interval or -1
};

struct tz_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string last_error;
    // device scratch pool (staging of host-pointer arguments, temporaries): grown on demand and
    // reused; the top bit of the size marks a block that is handed out until the entry point's tz_call scope closes
    std::vector<std::pair<void*, size_t>> pool;
    bool in_call = false;             // a tz_call scope is open (scopes do not nest)
    // model + rollout state
    tz_model* model = nullptr;
    int conv_impl = 1;                // tz_set_conv_impl: 1 = LDS-DMA kernels where they apply
    int lat_mode = 1;                 // k_convlat: 0 never, 1 where the cost model says so, 2 wherever eligible (TEZIP_LAT)
    int contract = 0;                 // arithmetic contract of the predictor: 0 = by frame size, 1 = TZ-PA1, 2 = TZ-PA2 (tz_set_contract, TEZIP_PA)
    int num_cus = 256;                // compute units of the device (k_wino: column blocks per workgroup)
    int wino_ipw = 0;                 // TEZIP_WINO_IPW (measurements): column blocks per k_wino workgroup, 0 = chosen per launch
    int quality_grid = 0;             // TEZIP_QUALITY_GRID (diagnostic): workgroups of k_quality, 0 = chosen per launch
    int digest_grid = 0;              // TEZIP_DIGEST_GRID (diagnostic): workgroups of k_digest, 0 = chosen per launch
    int ssim_grid = 0;                // TEZIP_SSIM_GRID (diagnostic): workgroups of k_ssim, 0 = chosen per launch
    // rollout-resident data
    int nt = 0, H = 0, W = 0, Hp = 0, Wp = 0, warm_up = 0;
    uint8_t* d_frames = nullptr;      // nt*H*W*3 (encoder: originals; decoder: key stack)
    float* d_pred = nullptr;          // nt*Hp*Wp*3
    size_t cap_frames = 0, cap_pred = 0;
    std::vector<uint8_t> key_mask;    // nt
    std::vector<uint8_t> group_first; // nt: 1 where a group starts (delta slot 0 -> 0)
    std::vector<uint8_t> quant_skip;  // nt: 1 where error_bound is not applied
    // the resident prediction stack: made by which rollout, and holding frames [pred_first, pred_end) of the nt-frame
    // sequence (slot i = frame pred_first + i; key_mask is indexed the same way).  tz_rollout and tz_rollout_decode leave
    // the whole stack [0, nt); tz_rollout_decode_range a sub-stack, which only tz_decode_range reads.
    enum tz_rollout_kind { ROLLOUT_NONE = 0, ROLLOUT_ENCODE, ROLLOUT_DECODE } rollout_kind = ROLLOUT_NONE;
    int pred_first = 0, pred_end = 0;
    int pred_contract = 0;            // the arithmetic contract that produced the resident prediction stack (stamped by
                                      // tz_rollout / tz_rollout_decode*; tz_encode* / tz_decode* refuse a flip in between)
    // tz_rollout_closed (TZ-CL1): the resident predictions are those of a closed loop that fed back what (mode, b0, b1, quantiser)
    // decodes to -- the only job whose quantised deltas they serve (every rollout clears the stamp, tz_rollout_closed sets it)
    int loop_closed = 0;
    int loop_mode = 0, loop_quantiser = 0;
    double loop_b0 = 0.0, loop_b1 = 0.0;
    // tz_rollout_closed_frames (TZ-CLF1): the stamped loop ran under one abs bound per frame -- loop_bounds, 0 at fixed frames,
    // which tz_set_frame_bounds must hold for the rollout to serve a job; loop_frame_sse: sse(k) of a searched frame (0: given
    // bounds); loop_trace: the search's TZ_CLF_ROUNDS * nt sums, round-major, ~0 where a round did not run (empty: given bounds)
    int loop_frames = 0;
    std::vector<double> loop_bounds;
    // tz_rollout_closed_map (TZ-CLM1): the stamped loop ran under the bound map loop_map_bytes of loop_map_h x loop_map_w (a copy of
    // the bytes: setting an equal map again still serves the job); map_host: the bytes of the map in force
    int loop_map = 0, loop_map_h = 0, loop_map_w = 0;
    std::vector<uint8_t> loop_map_bytes, map_host;
    std::vector<unsigned long long> loop_frame_sse, loop_trace;
    // tz_set_pred_select (TZ-PS1): the setting; whether the stamped loop ran under it (part of the stamp: predictions with chosen
    // tiles expressed in them serve a select job alone, and the other way round); the modes of that loop (nt * TH * TW bytes,
    // tz_pred_modes), and the modes a decoder was given (tz_put_pred_modes) for its next tz_rollout_decode_closed
    int pred_select = 0, loop_select = 0;
    std::vector<uint8_t> pred_modes, put_modes;
    // tz_set_pred_motion (TZ-PM1): the search radius (0: off, 7), the radius the stamped loop ran under (part of the stamp like
    // loop_select), its vectors (2 * nt * TH * TW int8 (dy, dx), tz_pred_vectors) and a decoder's (tz_put_pred_vectors)
    int pred_motion = 0, loop_motion = 0;
    std::vector<int8_t> pred_vectors, put_vectors;
    // pinned staging ring for small host->device uploads (index arrays, masks, LUTs): the copy
    // out of it is truly asynchronous and the memory outlives the caller's locals
    uint8_t* ring = nullptr;
    size_t ring_size = 0, ring_pos = 0;
    // index table of the static rollout schedule (SWP encoder / decoder replay): [batches][3][stride]
    int* d_sched = nullptr;
    size_t cap_sched = 0;
    // copy engine: host<->device transfers of the frame stack and the payload run on their own
    // stream so that they overlap the predictor (key frames go first, the rest follows while the
    // rollout computes; the payload leaves chunk by chunk behind the remap kernel).  Pinned host
    // memory (tz_host_alloc) is DMA'd directly; pageable memory is pipelined through `stage`.
    hipStream_t copy_stream = nullptr;
    hipStream_t down_stream = nullptr;   // device -> host leg of the payload hand-over: a stream of its own, so that a deferred
                                         // transfer (tz_set_payload_deferred) does not sit in front of the next sequence's uploads
    hipEvent_t ev_keys = nullptr, ev_frames = nullptr, ev_compute = nullptr;
    // second compute stream of a static rollout schedule (run_schedule): the windows advance as two independent
    // groups, so that one group's launch fills the CUs the other group's draining launch leaves idle
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int split_rollout = 0;            // TEZIP_SPLIT=1 turns it on (measured in round 3: slower, see run_schedule)
    // "E-part ahead" (round 5, tz_model_predict_batch_dev): per level, E_l ready on the compute stream / the launch over it
    // finished on stream2
    hipEvent_t ev_epart_src[TZ_MAX_LEVELS] = {nullptr}, ev_epart_done[TZ_MAX_LEVELS] = {nullptr};
    hipEvent_t ev_cal[2] = {nullptr, nullptr};   // epart_measure: timing events on the compute stream (tz_prednet.hip)
    int epart_mode = -1;              // TEZIP_EPART: -1 where launches cannot fill the chip (default), 0 never, 1 wherever possible
    static constexpr int kStages = 4;
    static constexpr size_t kStageBytes = (size_t)8 << 20;
    uint8_t* stage[kStages] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t stage_ev[kStages] = {nullptr, nullptr, nullptr, nullptr};
    bool stage_busy[kStages] = {false, false, false, false};
    int stage_next = 0;
    bool staged = false;                    // d_frames was filled by tz_frames_begin / tz_frames_put
    int16_t* d_payload = nullptr;           // resident payload of a tz_encode(payload = NULL)
    size_t cap_payload = 0, payload_len = 0;
    // what d_payload holds for the encoder on the current rollout: nothing, the symbols of a tz_encode_begin (before
    // the carry and the remap of tz_encode_finish) or the payload of a tz_encode(payload = NULL)
    enum tz_enc_kind { ENC_NONE = 0, ENC_SYMBOLS, ENC_PAYLOAD } enc_kind = ENC_NONE;
    bool enc_entropy = false;               // ENC_SYMBOLS: they are 1600 - sd (tz_encode_begin's entropy flag)
    int16_t enc_first = 0;                  // ENC_SYMBOLS: first element of the shard's quantised delta stack
    unsigned* d_scan_status = nullptr;      // inverse scan: one word per resident block, tagged with the launch's epoch
    unsigned scan_epoch = 0;
    unsigned scan_dbg_skew = 0, scan_dbg_limit = 0;   // tz_scan_fault_inject: poll for another epoch / give up sooner
    // fault word: one pinned, device-visible host word that a kernel with a hand-built wait sets when the wait expires
    // (k_scan2p's bounded poll); the host reads it behind every stream synchronisation (tz_stream_sync)
    volatile unsigned* h_fault = nullptr;
    unsigned* d_fault = nullptr;
    int decode_unfused = 0;                 // TEZIP_DECODE_UNFUSED=1: tz_decode as scan + reconstruct launches (cross-check)
    int payload_channels = 3;               // tz_set_payload_channels: 1 = the payload of a gray job holds channel 0 alone
    std::vector<double> frame_bounds;       // tz_set_frame_bounds: one abs tolerance per frame of the encoder rollout (empty: none)
    // tz_set_bound_map (TZ-BM1): the H x W uint8 map of abs tolerances, resident on the device from the call that set it
    // (map_h == 0: none); map_max = its largest entry (0: the lossless job)
    uint8_t* d_bound_map = nullptr;
    int map_h = 0, map_w = 0, map_max = 0;
    int delta_stride_mode = 0;              // tz_set_delta_stride: 1 = the spatial delta of the payload runs at the channel stride
    int delta_plane = 0;                    // tz_set_delta_plane: 1 = the spatial delta of the payload is the 2-D one, TZ-SD2
    int quantiser = 0;                      // tz_set_quantiser: 0 = the reference's greedy walk, 1 = the lattice quantiser TZ-QL1
    unsigned long long* d_scan3_status = nullptr;   // strided inverse scan (k_scan3p): one 64-bit word per block, own epochs
    unsigned scan3_epoch = 0;
    // opt-in Huffman coder (tz_huff_*): the coded stream (index | bits) of the resident payload, or the stream a decoder
    // stages with tz_huff_begin / tz_huff_put together with what tz_huff_decode needs to expand it
    uint8_t* d_huff = nullptr;
    size_t cap_huff = 0, huff_bytes = 0;
    // what tz_huff_begin / tz_huffr_begin / tz_huffd_begin staged in d_huff, so that no decoder expands another's stream
    enum tz_huff_kind { HUFF_NONE, HUFF_TZH1, HUFF_TZR1, HUFF_TZR2 } huff_kind = HUFF_NONE;
    int huff_dist = 0;                      // the match distance of the staged stream: 0 (TZH1: no tokens), 3 (TZR1), a TZR2 stream's 0, 1 or 3
    size_t huff_n = 0;                      // elements the staged stream decodes to
    int huff_A = 0, huff_base = 0;          // literals of the staged code (a TZR1 code has its repeat tokens behind them)
    std::vector<uint16_t> huff_dec_tab;     // the 2^12-entry decode table of the staged stream's lengths
    // opt-in key-frame coder (tz_keys_*): buffers of its own, so that an entropy stream staged with tz_huff_begin /
    // tz_huffr_begin survives it.  d_keys: the coded stream (index | bits) tz_keys_encode left or tz_keys_begin / tz_keys_put
    // stage; d_keysym: the int16 residual symbols between the predictor kernels and the Huffman kernels
    uint8_t* d_keys = nullptr;
    int16_t* d_keysym = nullptr;
    size_t cap_keys = 0, cap_keysym = 0, keys_bytes = 0;
    // what tz_keys_begin / tz_keysg_begin staged in d_keys, so that neither decoder expands the other's stream
    enum tz_keys_kind { KEYS_NONE, KEYS_TZK1, KEYS_TZK2 } keys_kind = KEYS_NONE;
    size_t keys_n = 0;                      // symbols the staged stream decodes to
    size_t keys_put = 0;                    // bytes tz_keys_put / tz_keysg_put have staged since the begin
    int keys_nt = 0, keys_H = 0, keys_W = 0;
    std::vector<int> keys_idx;              // the key frames' indices ...
    std::vector<uint8_t> keys_pred;         // ... and predictor ids (TZK1) or pred bytes (TZK2)
    std::vector<uint16_t> keys_dec_tab;     // the 2^12-entry decode table of the staged stream's lengths
    uint8_t* d_out = nullptr;               // resident decoded frames of a tz_decode(frames_out = NULL)
    size_t cap_out = 0;
    bool have_decoded = false;
    int dec_first = 0, dec_count = 0;       // frames of the sequence that d_out holds (tz_decode: all, tz_decode_range: its range)
    const uint8_t* pending_src = nullptr;  // host frame stack whose non-key frames are still to be sent
    std::vector<uint8_t> pending_sent;     // nt: 1 = already on its way
    std::vector<hipEvent_t> chunk_ev;  // payload chunk hand-over events (compute -> copy stream)
    // deferred payload hand-over (tz_set_payload_deferred): tz_encode returns once the last chunk of the payload is QUEUED
    // on the copy stream; the device -> host transfer then runs under the next sequence's rollout.  The chunks leave from
    // a staging buffer of the context's own (a pool block would be handed out again by the next call).
    int defer_payload = 0;
    bool payload_inflight = false;
    hipEvent_t ev_payload = nullptr;        // recorded on the copy stream behind the last chunk
    int16_t* d_payload_stage = nullptr;
    size_t cap_payload_stage = 0;
    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool prof_on = false;
    tz_prof_slot prof[TZP_COUNT];
};

int tz_fail(tz_ctx* ctx, int status, const char* fmt, ...);
// TZ_ERR_STATE when the contract in force is no longer the one the resident prediction stack was made under
int tz_check_pred_contract(tz_ctx* ctx, const char* who);
static constexpr unsigned TZ_FAULT_SCAN_POLL = 1u;   // k_scan2p: a status word never showed the launch's epoch
int tz_fault_word(tz_ctx* ctx);      // makes the fault word on first use
int tz_stream_sync(tz_ctx* ctx);     // hipStreamSynchronize(ctx->stream) + TZ_ERR_HIP if a kernel reported a fault
int tz_payload_settle(tz_ctx* ctx);  // waits for a deferred payload transfer still in flight (no-op without one)

#define TZ_HIP(ctx, expr)                                                                      \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return tz_fail(ctx, TZ_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                           __FILE__, __LINE__);                                                \
    } while (0)

#define TZ_TRY(expr)            \
    do {                        \
        int _s = (expr);        \
        if (_s != TZ_OK) return _s; \
    } while (0)

// ---- window SSE: one 4096-element block of one padded frame (compress.py:246), the fixed order of tz_codec.hip k_sse:
// thread t sums elements t, t + 256, ... of the block, then a halving tree over the 256 partials; the result is valid on
// thread 0.  `s` = 256 doubles of LDS.  Shared by k_sse and by the DWP step kernel of tz_api.hip (k_sse_decide).
static __device__ __forceinline__ double tz_sse_block(const uint8_t* __restrict__ o, const float* __restrict__ p, int H, int W, int Hp,
                                                      int Wp, int b, double* s) {
    // (32-bit index arithmetic: a padded frame has fewer than 2^29 elements, tz_model_prepare; the 64-bit divisions this
    // loop used to do per element were 27 us per 512x512 frame -- 4 % of a one-window predictor step)
    const unsigned n = (unsigned)Hp * (unsigned)Wp * 3u, uWp = (unsigned)Wp;
    // all 32 loads of the thread first (they are independent; issued one iteration at a time their round trips added up to
    // most of the kernel), then the sum in its fixed order
    float pv[16], xv[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const unsigned i = (unsigned)b * 4096u + (unsigned)j * 256u + threadIdx.x;
        pv[j] = 0.0f;
        xv[j] = 0.0f;
        if (i < n) {
            const unsigned pix = i / 3u, c = i - pix * 3u, y = pix / uWp, x = pix - y * uWp;
            pv[j] = p[i];
            if (y < (unsigned)H && x < (unsigned)W) xv[j] = (float)o[((size_t)y * W + x) * 3 + c] / 255.0f;
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const double d = (double)xv[j] - (double)pv[j];
        acc = acc + d * d;   // (an element past the end of the frame adds +0.0, as before)
    }
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + st];
        __syncthreads();
    }
    return s[0];
}

// ---- device memory helpers -------------------------------------------------------------
bool tz_is_device_ptr(const void* p);
int tz_poison_byte();                                 // TEZIP_POISON diagnostic: 0x100 | byte, or 0
int tz_poison(tz_ctx*, void* p, size_t bytes);        // fill a freshly handed-out device buffer when it is on
int tz_pool_alloc(tz_ctx* ctx, size_t bytes, void** out);   // handed out until the caller's tz_call scope closes
void tz_pool_release_all(tz_ctx* ctx);                      // (~tz_call and tz_ctx_destroy alone)
int tz_ensure(tz_ctx* ctx, void** buf, size_t* cap, size_t bytes);  // persistent buffer growth
// Stream-ordered upload of a small host block to `dst` (device) through the pinned ring.
int tz_upload(tz_ctx* ctx, void* dst, const void* src, size_t bytes);

// 0 = pageable host, 1 = pinned / registered host, 2 = device
int tz_ptr_kind(const void* p);
// Stream-ordered host -> device copy on stream `s`.  Pinned source: one asynchronous DMA (the
// source must stay valid until `s` reaches it).  Pageable source: pipelined through the pinned
// staging buffers; the source is free again when the call returns.
int tz_h2d(tz_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s);
// Device -> host copy on stream `s`.  Pinned destination: asynchronous (complete when `s` is
// synchronised).  Pageable destination: pipelined through the staging buffers, complete on return.
int tz_d2h(tz_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s);
// Input argument: returns a device pointer holding `bytes` of *p (staging if host).
int tz_dev_in(tz_ctx* ctx, const void* p, size_t bytes, const void** dev);
// Output argument: returns a device pointer to write; tz_call::finish copies back if host.
struct tz_out {
    void* host = nullptr;
    void* dev = nullptr;
    size_t bytes = 0;
    bool done = false;  // already copied back (chunked hand-over on the copy stream)
};
int tz_dev_out(tz_ctx* ctx, void* p, size_t bytes, tz_out* o);

// The scope of one entry point: opened once, behind the argument checks, it owns the outputs of the call
// and hands every pool block back on whichever path the call leaves.  Helpers allocate from the pool under their caller's
// scope and never release; a call that wants its blocks back half way closes a braced scope of its own first.
struct tz_call {
    tz_ctx* ctx;
    std::vector<tz_out> outs;   // copied back by finish(), in this order
    explicit tz_call(tz_ctx* c) : ctx(c) {
        assert(!ctx->in_call);
        ctx->in_call = true;
    }
    ~tz_call() {
        tz_pool_release_all(ctx);
        ctx->in_call = false;
    }
    tz_call(const tz_call&) = delete;
    tz_call& operator=(const tz_call&) = delete;
    template <class T>
    int in(const T* p, size_t bytes, const T** dev) {   // tz_dev_in
        const void* d = nullptr;
        TZ_TRY(tz_dev_in(ctx, p, bytes, &d));
        *dev = (const T*)d;
        return TZ_OK;
    }
    template <class T>
    int alloc(size_t bytes, T** p) {   // tz_pool_alloc
        void* d = nullptr;
        TZ_TRY(tz_pool_alloc(ctx, bytes, &d));
        *p = (T*)d;
        return TZ_OK;
    }
    template <class T>
    int out(T* p, size_t bytes, T** dev) {   // tz_dev_out; the tz_out joins outs (outs.back())
        tz_out o;
        TZ_TRY(tz_dev_out(ctx, p, bytes, &o));
        outs.push_back(o);
        *dev = (T*)o.dev;
        return TZ_OK;
    }
    int finish();   // D2H copies of the outputs not yet done + stream sync if any was a host pointer
};

// ---- profiling wrapper ------------------------------------------------------------------
struct tz_prof_scope {
    tz_ctx* ctx;
    int cls;
    int sub = -1;  // optional second class the same interval is added to (set before the scope ends)
    hipEvent_t a = nullptr, b = nullptr;
    bool rx = false;   // a ROCTx range is open (TEZIP_ROCTX=1)
    tz_prof_scope(tz_ctx* c, int k);
    ~tz_prof_scope();
};

// ROCTx ranges ("same -v lines + rocprofv3 / roctx ranges"): with TEZIP_ROCTX=1 the library opens
// librocprofiler-sdk-roctx.so (else libroctx64.so) and brackets every C-ABI stage call and every stage class of
// tz_prof_scope with roctxRangePushA / roctxRangePop, so that `rocprofv3 --marker-trace --kernel-trace` shows the launches
// of a stage under its name.  Off (the default): one branch on a cached flag.  A library that cannot be opened is said
// once on stderr and the run goes on without ranges -- a diagnostic must never be what a job fails on.
bool tz_roctx_push(const char* name);   // returns whether a range was opened
void tz_roctx_pop();
struct tz_roctx_range {
    bool on;
    explicit tz_roctx_range(const char* name) : on(tz_roctx_push(name)) {}
    ~tz_roctx_range() {
        if (on) tz_roctx_pop();
    }
};

// ---- kernels' host launchers (device pointers only) ---------------------------------------
// tz_codec.hip
int tzk_delta(tz_ctx*, const float* pred, const uint8_t* orig, const uint8_t* d_zero_mask, int nframes,
              int H, int W, int Hp, int Wp, int16_t* out);
int tzk_delta_sd_fused(tz_ctx*, const float* pred, const uint8_t* orig, const uint8_t* d_zero_mask, int nframes, int H,
                       int W, int Hp, int Wp, int apply_offset, int16_t* out, unsigned long long* d_hist, int16_t* d_edge,
                       bool* done);
int tzk_error_bound(tz_ctx*, const uint8_t* orig, int16_t* diff, const uint8_t* h_skip, int nframes, int H,
                    int W, int mode, double b0, double b1);
bool tz_quant_is_identity(int mode, double b0, double b1);   // error_bound leaves every integer delta as it is (tz_codec.hip)
int tzk_quant_sd_fused(tz_ctx*, const float* pred, const uint8_t* orig, const uint8_t* d_zero_mask, const uint8_t* h_skip,
                       int nframes, int H, int W, int Hp, int Wp, int mode, double b0, double b1, int apply_offset,
                       int16_t* sym, unsigned long long* d_hist, int16_t* d_edge, bool* done);
// `abs` with one tolerance per frame (h_bounds: nframes finite doubles >= 0): on a delta stack in place (diff), or -- diff NULL --
// as the fused lossy front that `fu` describes, where its kernels apply (*done).
struct tz_quant_fused {
    const float* pred;
    const uint8_t* d_zero_mask;
    int Hp, Wp, apply_offset;
    int16_t* sym;
    unsigned long long* d_hist;
    int16_t* d_edge;
};
int tzk_quant_frames(tz_ctx*, const uint8_t* orig, int16_t* diff, const tz_quant_fused* fu, const uint8_t* h_skip, int nframes,
                     int H, int W, const double* h_bounds, bool* done);
// the greedy walk under the bound map d_map (TZ-BM1; device, H * W bytes), in the two forms of tzk_quant_frames; orig is read only
// by the fused front
int tzk_quant_map(tz_ctx*, const uint8_t* orig, int16_t* diff, const tz_quant_fused* fu, const uint8_t* h_skip, int nframes, int H,
                  int W, const uint8_t* d_map, bool* done);
// The layout of the payload, stated once per layer: elements per pixel, and how far in front the element
// lies that the spatial delta subtracts.  flat {3, 1} is the reference's; gray {1, 1} stores channel 0 alone
// (tz_set_payload_channels(1)); channel stride {3, 3} takes the same channel of the pixel in front (tz_set_delta_stride(1));
// plane {3 or 1, 1, H, W} predicts from the pixel in front and the row above within a frame (tz_set_delta_plane(1)).
// A carry is `stride` HOST elements, the ones in front of the first element, or NULL at the stream start.
// plane_h, plane_w (0: not plane): the frame's rows and columns when the spatial delta is the 2-D one, TZ-SD2
// (tz_set_delta_plane(1)); stride is then 1 and no carry exists -- every frame is coded on its own.
struct tz_layout {
    int channels, stride;
    int plane_h = 0, plane_w = 0;
};
static inline size_t tz_frame_elems(tz_layout l, int H, int W) { return (size_t)H * W * l.channels; }   // payload elements of a frame
// in -> n elements at out.  flat, channel stride: in holds n elements; gray: the interleaved three-channel stack of n pixels, of
// which channel 0 is taken, and d_edge (may be NULL) receives its first and last element.  Then 1600 - y when apply_offset,
// and the counts ADDED to d_hist (may be NULL).  Flat wants 16-byte aligned buffers, the other two 2-byte aligned ones.
int tzk_spatial_delta(tz_ctx*, tz_layout, const int16_t* in, size_t n, const int16_t* carry, int apply_offset, int16_t* out,
                      unsigned long long* d_hist, int16_t* d_edge);
// The lattice quantiser TZ-QL1 (include/tezip_hip.h: tz_set_quantiser).  (mode, b0, b1) as tzk_error_bound's
// and refused as there; h_bounds (may be NULL): nframes abs tolerances, finite and >= 0, in their place.
// tzk_lattice: the int16 delta stack diff (any 2-byte alignment) is quantised in place; frames with h_skip[f] stay as they are.
// tzk_lattice_sd_fused: the fused front -- delta, TZ-QL1, the layout's spatial delta, 1600 offset and histogram in one pass over
// pred / orig, where its kernel applies (unpadded frames of whole 16-byte groups on 16-byte boundaries: *done).  d_zero_mask as
// tzk_delta's; d_edge (may be NULL) receives the first and the last element of the quantised stack (channel 0's under the gray
// layout, nothing under the channel stride).
// d_map (may be NULL; device, H * W bytes): the bound map of TZ-BM1 in place of (mode, b0, b1) and h_bounds -- e = d_map[pixel].
int tzk_lattice(tz_ctx*, const uint8_t* orig, int16_t* diff, const uint8_t* h_skip, int nframes, int H, int W, int mode, double b0,
                double b1, const double* h_bounds, const uint8_t* d_map = nullptr);
int tzk_lattice_sd_fused(tz_ctx*, tz_layout, const float* pred, const uint8_t* orig, const uint8_t* d_zero_mask, const uint8_t* h_skip,
                         int nframes, int H, int W, int Hp, int Wp, int mode, double b0, double b1, const double* h_bounds,
                         int apply_offset, int16_t* sym, unsigned long long* d_hist, int16_t* d_edge, bool* done,
                         const uint8_t* d_map = nullptr);
bool tz_lattice_is_identity(int mode, double b0, double b1);   // the worst-case tolerance of the job is below 1: q == d everywhere
// TZ-SD2 (k_sdelta_plane; k_unplane_cols + k_unplane_rows) on nframes x H x W x C elements at any 2-byte alignment.  in of
// tzk_sdelta_plane holds cin elements per pixel: cin == C, or 3 with C = 1 (channel 0 is taken).  tzk_unplane may run in place.
int tzk_sdelta_plane(tz_ctx*, const int16_t* in, int cin, int nframes, int H, int W, int C, int apply_offset, int16_t* out,
                     unsigned long long* d_hist);
int tzk_unplane(tz_ctx*, const int16_t* in, int nframes, int H, int W, int C, const int16_t* h_lut2112, int post_offset, int16_t* out);
int tzk_lut(tz_ctx*, const int16_t* in, size_t n, const int16_t* h_lut2112, int post_offset, int16_t* out);
// forward: int16[n] -> low-byte plane | high-byte plane (2n bytes); inverse: planes (passed as `in`) -> int16[n] at `out`
int tzk_shuffle(tz_ctx*, const int16_t* in, size_t n, uint8_t* out, int inverse);
// the inverse: x[i] = x[i - stride] - s[i], through the decoder LUT when there is one (k_scan2p; stride 3: k_scan3p)
int tzk_undelta(tz_ctx*, int stride, const int16_t* in, size_t n, const int16_t* carry, const int16_t* h_lut2112, int post_offset,
                int16_t* out);
// the `stride` decoded elements in front of in[n0] into d_words[0 .. stride) (low 16 bits); stride 3: n0 a multiple of 3
int tzk_undelta_carry(tz_ctx*, int stride, const int16_t* in, size_t n0, const int16_t* h_lut2112, int post_offset, unsigned* d_words);
// diff holds `channels` deltas per pixel; with one, the sample goes to all three channels of out
int tzk_reconstruct(tz_ctx*, int channels, const float* pred, const uint8_t* key, const uint8_t* d_key_mask, const int16_t* diff,
                    int nframes, int H, int W, int Hp, int Wp, uint8_t* out);
// inverse remap, inverse spatial delta and reconstruct of nframes frames of the payload `in`
int tzk_decode_tail(tz_ctx*, tz_layout, const int16_t* in, const int16_t* h_lut2112, int post_offset, const int16_t* carry,
                    const float* pred, const uint8_t* key, const uint8_t* d_key_mask, int nframes, int H, int W, int Hp, int Wp,
                    uint8_t* out);
// per-frame (sse, max |dec - orig|, #changed) of two unpadded nframes x fe uint8 stacks; d_out (device) is cleared here
int tzk_quality(tz_ctx*, const uint8_t* orig, const uint8_t* dec, int nframes, size_t fe, tz_frame_quality* d_out);
// per-frame (#samples with |dec - orig| > d_map[pixel], largest excess) of two unpadded nframes x H x W x 3 uint8 stacks under the
// H x W bound map d_map (device); d_out (device) is cleared here
int tzk_map_check(tz_ctx*, const uint8_t* orig, const uint8_t* dec, const uint8_t* d_map, int nframes, int H, int W, tz_map_record* d_out);
// the same records for what the quantised deltas q of the deltas d (tzk_delta's, int16, unpadded like orig) reconstruct to:
// clamp(orig + d - q, 0, 255) against orig, with no decoded stack in memory (k_bound_err); d_out (device) is cleared here.
// channels 1: what a one-channel payload decodes to -- channel 0's reconstruction in all three channels (fe % 3 == 0)
int tzk_bound_err(tz_ctx*, int channels, const uint8_t* orig, const int16_t* d, const int16_t* q, int nframes, size_t fe, tz_frame_quality* d_out);
// TZD64 digests of nframes frames of fe bytes (fe < 2^32, else TZ_ERR_INVALID before any launch); d_out: nframes words, cleared here
int tzk_digest(tz_ctx*, const uint8_t* x, int nframes, size_t fe, unsigned long long* d_out);
// TZ-SSIM-1 records of two unpadded nframes x H x W x 3 uint8 stacks (a frame of 2^32 bytes or more: TZ_ERR_INVALID before any
// launch); d_out: nframes records, written whole here
int tzk_ssim(tz_ctx*, const uint8_t* a, const uint8_t* b, int nframes, int H, int W, tz_frame_ssim* d_out);
// Huffman coder.  Geometry: runs of TZ_HUFF_RUN symbols, chunks of TZ_HUFF_CHUNK_RUNS runs.
static constexpr int TZ_HUFF_L = 12, TZ_HUFF_RUN = 256, TZ_HUFF_CHUNK_RUNS = 64;
static constexpr int TZ_HUFF_COUNT_BINS = 4096, TZ_HUFF_COUNT_BIAS = 1024;   // k_huff_count: bin = value + bias
struct tz_huff_meta {            // device words the size / scan launches leave for the host
    unsigned long long total_words;
    unsigned bad;                // a payload value without a code (k_huff_size) or outside the counted range (k_huff_count)
    unsigned pad;
};
int tzk_huff_count(tz_ctx*, const int16_t* in, size_t n, unsigned long long* d_hist4096, tz_huff_meta* d_meta);
// Huffman coder with repeat tokens (TZR1): the same geometry and index; a code has A literals and then
// TZ_HUFFR_NTOK repeat tokens, so the histogram holds TZ_HUFF_COUNT_BINS + 8 bins.
int tzk_huffr_count(tz_ctx*, const int16_t* in, size_t n, unsigned long long* d_hist4104, tz_huff_meta* d_meta);
// The coder that picks its match distance (TZR2): three such histograms from one read, distance 0 (no tokens) | 1 | 3.
int tzk_huffd_count(tz_ctx*, const int16_t* in, size_t n, unsigned long long* d_hist3x4104, tz_huff_meta* d_meta);
// The passes of the coder at the match distance dist: 0 (TZH1: no tokens), or a tokenised stream's 3 (TZR1) or 1 (a TZR2 file
// names any of the three); d_enc then holds TZ_HUFFR_NTOK entries behind the A literals.
// run sizes (u16, bits) and chunk word offsets (u32) of the payload under the code `d_enc` (u16: stored code | length << 12)
int tzk_huff_size(tz_ctx*, const int16_t* in, size_t n, const uint16_t* d_enc, int A, int base, uint16_t* d_run_bits,
                  unsigned* d_chunk_off, tz_huff_meta* d_meta, int dist);
int tzk_huff_enc(tz_ctx*, const int16_t* in, size_t n, const uint16_t* d_enc, int A, int base, const uint16_t* d_run_bits,
                 const unsigned* d_chunk_off, unsigned* d_words, size_t stream_words, int dist);
int tzk_huff_dec(tz_ctx*, const unsigned* d_chunk_off, const uint16_t* d_run_bits, const unsigned* d_words, size_t stream_words,
                 const uint16_t* d_dec_tab4096, int A, int base, size_t n, int16_t* out, int dist);
// The size of a candidate bound (tz_size_probe, TZ-TRATIO-1): both kernels form the payload symbols of `layout` from the
// quantised delta stack q on the fly (n symbols: q holds n elements, 3 n under the one-channel layout; 2-byte aligned, 16 for
// vector loads), in front of the rank remap.  A layout with plane_h, plane_w (tz_sdelta_probe, TZ-SDA1: stride 1, n whole frames)
// yields the symbols of TZ-SD2, three channels or channel 0 alone of q's whole pixels.  tzk_size_count: tzk_huffd_count's three histograms of those symbols.
// tzk_size_bits: the stream's size under d_lens -- TZ_HUFF_COUNT_BINS code lengths by bin (= symbol + TZ_HUFF_COUNT_BIAS; the
// length of the symbol's rank, 0: no code), then the 8 token lengths -- at the match distance dist.
struct tz_size_meta {            // device words k_size_bits leaves for the host
    unsigned long long words;    // sum over the chunks of ceil(chunk bits / 32)
    unsigned long long bits;     // sum of the chunk bits
    unsigned bad;                // a symbol or a token without a code
    unsigned pad;
};
int tzk_size_count(tz_ctx*, tz_layout, const int16_t* q, size_t n, int apply_offset, unsigned long long* d_hist3x4104, tz_huff_meta* d_meta);
int tzk_size_bits(tz_ctx*, tz_layout, const int16_t* q, size_t n, int apply_offset, const uint8_t* d_lens, int dist, tz_size_meta* d_meta);
// key-frame coders (TZK1, and TZK2 = TZK1 with a GRAY bit: DESIGN.md section 9).  d_frames: a stack of H x W x 3 frames of which
// frame d_idx[k] is key frame k; d_pred[k] its pred byte: predictor id 0..3, | 4 for a GRAY frame (TZK2 alone), which has H * W
// symbols instead of H * W * 3; d_sym: the int16 symbols 0..255, key after key; d_off[k]: where frame k's symbols start in d_sym
// (u64 exclusive prefix of the per-frame counts; k * H * W * 3 without a GRAY frame); d_flags[k] != 0: not gray; d_tmp: scratch of
// one byte per symbol, or NULL when no frame has (d_pred[k] & 6) == 6
int tzk_key_hist(tz_ctx*, const uint8_t* d_frames, int H, int W, const int* d_idx, int nkeys, unsigned* d_counts /* [nkeys][4][256] */);
int tzk_key_gray(tz_ctx*, const uint8_t* d_frames, int H, int W, const int* d_idx, int nkeys, unsigned* d_flags);
int tzk_key_resid(tz_ctx*, const uint8_t* d_frames, int H, int W, const int* d_idx, const uint8_t* d_pred, const unsigned long long* d_off,
                  int nkeys, int16_t* d_sym);
int tzk_key_unresid(tz_ctx*, const int16_t* d_sym, int H, int W, const int* d_idx, const uint8_t* d_pred, const unsigned long long* d_off,
                    int nkeys, uint8_t* d_tmp, uint8_t* d_frames);
// closed-loop prediction TZ-CL1: the frames d_list[0 .. nlist) (device, sequence indices) of the padded prediction stack pred and of
// the unpadded whole-sequence stacks.  tzk_cl_step: dec = clamp(x - TZ-QL1(x - orig, E), 0, 255), x the truncated prediction
// (E = 0: dec = the clamped original's own value, x - (x - orig)); tzk_cl_recon: dec = clamp(x - q, 0, 255).
int tzk_cl_step(tz_ctx*, const float* pred, const uint8_t* orig, uint8_t* dec, const int* d_list, int nlist, int H, int W, int Hp, int Wp,
                int E);
int tzk_cl_recon(tz_ctx*, const float* pred, const int16_t* q, uint8_t* dec, const int* d_list, int nlist, int H, int W, int Hp, int Wp);
// TZ-CLF1 (tz_rollout_closed_frames): the closed loop under one abs bound per frame.  d_sse: TZ_CLF_ROUNDS * nt sums, round-major,
// zeroed once per rollout.  tzk_clf_probe: round `round` of the bisection against `limit` for the nlist frames of a step (a frame
// whose interval has closed is left alone).  tzk_clf_step: tzk_cl_step with E = d_radius[frame], or (d_radius NULL) with the result
// of the frame's TZ_CLF_ROUNDS rounds, which also leaves k in d_k[frame] and sse(k) in d_sse_out[frame].
constexpr int TZ_CLF_ROUNDS = 9;
int tzk_clf_probe(tz_ctx*, const float* pred, const uint8_t* orig, const int* d_list, int nlist, int H, int W, int Hp, int Wp, int round,
                  unsigned long long* d_sse, int nt, unsigned long long limit);
int tzk_clf_step(tz_ctx*, const float* pred, const uint8_t* orig, uint8_t* dec, const int* d_list, int nlist, int H, int W, int Hp, int Wp,
                 const int* d_radius, const unsigned long long* d_sse, int nt, unsigned long long limit, int* d_k, unsigned long long* d_sse_out);
// TZ-CLM1 (tz_rollout_closed_map): tzk_cl_step / tzk_ps_step with E = d_map[pixel], the H * W byte bound map on the device
int tzk_clm_step(tz_ctx*, const float* pred, const uint8_t* orig, uint8_t* dec, const uint8_t* d_map, const int* d_list, int nlist, int H,
                 int W, int Hp, int Wp);
int tzk_psm_step(tz_ctx*, float* pred, const uint8_t* orig, uint8_t* dec, uint8_t* modes, const uint8_t* d_map, const int* d_list, int nlist,
                 int H, int W, int Hp, int Wp);
// per-tile choice of the prediction TZ-PS1 (tezip_amd/predselect.py) on the same frames and stacks; modes: nt * ceil(H/16) * ceil(W/16)
// bytes on the device, frame-major.  Per 16 x 16 tile, x_prev = the frame in front (orig[t-1] for tzk_ps_select, dec[t-1] for the
// others) replaces x_net = the truncated prediction iff it leaves the smaller sum |Q(x - orig)| (TZ-QL1 with E, the identity for
// E = 0); a chosen tile is written into pred as (v + 0.5f) / 255.0f (1.0f for v = 255), which truncates back to v.
// tzk_ps_select: the mode bytes and the patched pred (lossless: dec is the original); tzk_ps_step: also dec[t] as tzk_cl_step;
// tzk_ps_recon: the mode bytes are read, dec[t] as tzk_cl_recon.  tzk_ps_grid: the workgroups a frame's launch starts (grid.x).
int tzk_ps_select(tz_ctx*, float* pred, const uint8_t* orig, uint8_t* modes, const int* d_list, int nlist, int H, int W, int Hp, int Wp);
int tzk_ps_step(tz_ctx*, float* pred, const uint8_t* orig, uint8_t* dec, uint8_t* modes, const int* d_list, int nlist, int H, int W, int Hp,
                int Wp, int E);
int tzk_ps_recon(tz_ctx*, float* pred, const int16_t* q, uint8_t* dec, const uint8_t* modes, const int* d_list, int nlist, int H, int W,
                 int Hp, int Wp);
int tzk_ps_grid(int H, int W);
// motion-compensated tiles TZ-PM1 (tezip_amd/predmotion.py): as the three above, but the second candidate is the frame in front
// displaced by the tile's vector, -7 <= dy, dx <= 7 with clamped coordinates, found by a full search on raw u8 values (smallest
// SAD * 4096 + (|dy| + |dx|) * 256 + (dy + 7) * 16 + (dx + 7)).  vecs: 2 * nt * TH * TW int8 (dy, dx) on the device, (0, 0) where
// the mode byte is 0; the encoders write them, tzk_pm_recon reads them.  tzk_pm_grid: the workgroups a frame's launch starts.
int tzk_pm_select(tz_ctx*, float* pred, const uint8_t* orig, uint8_t* modes, int8_t* vecs, const int* d_list, int nlist, int H, int W, int Hp,
                  int Wp);
int tzk_pm_step(tz_ctx*, float* pred, const uint8_t* orig, uint8_t* dec, uint8_t* modes, int8_t* vecs, const int* d_list, int nlist, int H,
                int W, int Hp, int Wp, int E);
int tzk_pm_recon(tz_ctx*, float* pred, const int16_t* q, uint8_t* dec, const uint8_t* modes, const int8_t* vecs, const int* d_list, int nlist,
                 int H, int W, int Hp, int Wp);
int tzk_pm_grid(int H, int W);
int tzk_sse(tz_ctx*, const uint8_t* orig, const float* pred, int nframes, int H, int W, int Hp, int Wp,
            double* h_sse);
int tzk_sse_blocks(int Hp, int Wp);
int tzk_sse_launch(tz_ctx*, const uint8_t* orig, const float* pred, int nframes, int H, int W, int Hp, int Wp,
                   double* d_part);
// tz_prednet.hip
void tz_model_free(tz_ctx* ctx);
int tz_model_predict_batch(tz_ctx* ctx, int n, const int* h_in_is_key, const int* h_in_idx, const int* h_out_idx,
                           const uint8_t* d_frames_u8, int H, int W, const float* d_in_stack, float* d_out_stack);
// slot0: first activation slot of the batch (a rollout that advances two groups of windows on two streams
// gives each group its own range of the max_batch slots)
// d_next_slot (may be NULL): per item the activation slot its prediction will occupy as the INPUT of the next call on
// this stream (-1: none) -- the prediction kernel then also writes that call's level-0 error maps (*fused_next says whether
// it did), and that call may be told to skip_err0 -- or, when only the device knows whether an item of that call starts from a
// key frame instead (DWP), to launch the error unit for err0_keys_only.
int tz_model_predict_batch_dev(tz_ctx* ctx, int n, const int* d_idx, int stride, const uint8_t* d_frames_u8, int H, int W,
                               const float* d_in_stack, float* d_out_stack, int slot0 = 0, const int* d_next_slot = nullptr,
                               bool skip_err0 = false, bool* fused_next = nullptr, bool err0_keys_only = false);
int tz_model_c0_dev(tz_ctx* ctx, const float** c0);
int tz_model_dims(tz_ctx* ctx, int* Hp, int* Wp, int* max_batch);
