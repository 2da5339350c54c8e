/* tezip_hip.h -- C ABI of the MI355X-native TEZip hot path (libtezip_hip.so).
 *
 * The reference (kento/TEZip, /root/reference) is pure Python and has no FFI: the hot path
 * sits behind compress.run / decompress.run (src/compress.py:93, src/decompress.py:39) and
 * the operator seams inside them.  Each entry point below names the reference code it
 * replaces.  A ctypes binding (tezip_amd/_lib.py) is the "reference-side stub"; see
 * INTEGRATION.md for how the reference's own compress.py would call these.
 *
 * Conventions
 *  - extern "C", int return: 0 = TZ_OK, negative = tz_status; no exceptions cross the ABI.
 *  - Every data pointer may be HOST or DEVICE memory (detected with hipPointerGetAttributes);
 *    host buffers are staged through the context.  Outputs are complete when the call
 *    returns for host pointers; for device pointers the work is enqueued on the context's
 *    stream (tz_ctx_synchronize to wait).
 *  - One context per GPU/process; a context is not thread-safe; contexts are independent.
 *  - Frames are HWC, 3 channels; "padded" means H,W rounded up to a multiple of 8
 *    (data_utils.py:77-107) with pitch Wp*3.
 *  - All integer streams are int16, C-order over (frame, y, x, channel) (compress.py:329-340).  The one exception is opt-in:
 *    under tz_set_payload_channels(ctx, 1) the PAYLOAD holds channel 0 alone, nt*H*W elements over (frame, y, x), wherever
 *    a comment below says nt*H*W*3 of it; frames keep three channels.
 */
#ifndef TEZIP_HIP_H
#define TEZIP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tz_ctx tz_ctx;

/* tz_encode_quality: one record per frame (16 bytes) */
typedef struct {
    unsigned long long sse;   /* sum over the frame of (decoded - original)^2 */
    unsigned max_abs;         /* max |decoded - original| */
    unsigned n_changed;       /* samples with decoded != original */
} tz_frame_quality;

/* tz_map_check / tz_encode_map_check: one record per frame (16 bytes), definition TZ-BM1 below */
typedef struct {
    unsigned long long violations;   /* samples with |decoded - original| > M[pixel] */
    unsigned max_excess;             /* max over the frame of max(|decoded - original| - M[pixel], 0) */
    unsigned reserved;               /* 0 */
} tz_map_record;

/* tz_ssim_frames / tz_encode_ssim: one record per frame (24 bytes), definition TZ-SSIM-1 below */
typedef struct {
    long long sum_q32;        /* sum of Q over the frame's windows; frame SSIM = sum_q32 / (windows * 2^32) */
    long long min_q32;        /* the smallest Q of the frame (its worst window = min_q32 / 2^32), 0 when there is no window */
    unsigned windows;         /* windows of the frame, three channels together */
    unsigned reserved;        /* 0 */
} tz_frame_ssim;

typedef enum {
    TZ_OK = 0,
    TZ_ERR_INVALID = -1,     /* bad argument (the reference prints + exit()s or raises) */
    TZ_ERR_NO_DEVICE = -2,   /* no usable HIP device */
    TZ_ERR_HIP = -3,         /* a HIP runtime call failed: see tz_last_error */
    TZ_ERR_STATE = -4,       /* call order (no model / not prepared / no rollout) */
    TZ_ERR_NOMEM = -5,
    TZ_ERR_UNSUPPORTED = -6  /* model shape outside what the kernels cover */
} tz_status;

/* -m abs|rel|absrel|pwrel (tezip.py:96, compress.py:28-45) */
typedef enum { TZ_MODE_ABS = 0, TZ_MODE_REL = 1, TZ_MODE_ABSREL = 2, TZ_MODE_PWREL = 3 } tz_mode;

#define TZ_OFFSET 1600   /* compress.py:348 */
#define TZ_NBINS 2111    /* symbols 1600 - sd, sd in [-510, 510] (docs/index.rst:1222-1232) */
#define TZ_MAX_TABLE 1021
#define TZ_MAX_LEVELS 8

int tz_version(void);
/* "tezip_hip <version> gfx950 defines:<diagnostic switches this library was compiled with>".  A library whose string
 * names a switch after "defines:" is a measurement build (csrc/tz_wino_kernels.hip.h: TZW_ABL computes WRONG results by
 * design); bench.py and the tests refuse it.  No reference counterpart (the reference is interpreted Python). */
const char* tz_build_info(void);
const char* tz_strerror(int status);
const char* tz_last_error(const tz_ctx* ctx);

/* ---- context -------------------------------------------------------------------------
 * Replaces the device probe + TF session of tezip.py:16-26 / compress.py:281-287.
 * hip_stream: a hipStream_t to launch on (e.g. torch's current stream), or NULL to let the
 * context create its own. */
int tz_ctx_create(int device, void* hip_stream, tz_ctx** out);
int tz_ctx_destroy(tz_ctx* ctx);
int tz_ctx_synchronize(tz_ctx* ctx);
void* tz_ctx_stream(tz_ctx* ctx);
/* Pinned (page-locked) host memory for frame stacks and payloads: the reference builds its
 * stacks with np.array / np.hstack (compress.py:116-122, 329-333); a caller that decodes its images
 * into such a buffer lets the library DMA it directly and overlap the transfer with the
 * predictor (key frames first).  Pageable pointers are accepted everywhere too; they are
 * pipelined through pinned staging buffers inside the context. */
int tz_host_alloc(size_t bytes, void** out);
int tz_host_free(void* p);

/* ---- predictor (prednet.py:24-325 used through Model.predict, compress.py:155-173,227) ----
 * weights: the Keras weight list of the PredNet layer (prednet.py:210-227): for key in
 * sorted(a, ahat, c, f, i, o), for level: kernel (3,3,Cin,Cout) HWIO float32, bias (Cout).
 * 2*(6*nb_layers-1) arrays.  Only 3x3 filters (train.py:53-55). */
int tz_model_load(tz_ctx* ctx, int nb_layers, const int* stack_sizes, const int* r_stack_sizes,
                  const float* const* weights);
/* Fix the padded frame size and the largest number of windows advanced together; allocates
 * activations and evaluates everything that does not depend on the input (t=0 states).
 * Hp, Wp: multiples of 8 and of 2^(levels-1) (compress.py:178-181: "Image size is out of scope").
 * TZ_ERR_UNSUPPORTED when a level's widest per-frame plane (gate columns / error maps) would
 * reach 2^30 floats: the kernels address inside one frame's plane with 32-bit offsets (frames and
 * batch items are 64-bit strides).  Which level binds depends on the model: for the reference's
 * (3,48,96,192) it is level 1's 192 gate columns: the largest square frame is exactly 4728 x 4728
 * (4736 x 4736 is refused), the largest one-tile strip 8 x 2,796,200, ~22.3 M pixels in all;
 * models with R_l < S_l bind on their error maps instead (2 S_l floats per pixel).  The error text
 * names the model's limit; tests/test_gpu_frame_limit.py holds these edges.  A deviation: the
 * reference's frame size is bounded by memory only. */
int tz_model_prepare(tz_ctx* ctx, int Hp, int Wp, int max_batch);
/* X_hat[0,0] of predict((1,2,Hp,Wp,3)) (compress.py:197): input independent. out: Hp*Wp*3 f32 */
int tz_predict_c0(tz_ctx* ctx, float* out);
/* X_hat[0,1] for n independent padded float32 frames (compress.py:224-229). */
int tz_predict_next(tz_ctx* ctx, const float* frames, int n, float* out);
/* Debug/parity taps of the last tz_predict_next call with n == 1: kind 0 = e_l(t0),
 * 1 = r_l(t1); out sized (Hp>>l)*(Wp>>l)*channels. */
int tz_predict_tap(tz_ctx* ctx, int kind, int level, float* out);
/* Diagnostic: which convolution kernels the predictor launches.  1 (default; env TEZIP_CONV16=0
 * starts a context at 0) = the LDS-DMA kernels k_conv16 / k_conv16b / k_conv_small wherever a
 * convolution qualifies, 0 = the general register-staged kernel k_conv3x3 everywhere.  Both walk
 * the same fmaf chains: results are bit-identical (tests/test_gpu_fullsize.py).
 * Bits 1-2 select the small-grid kernel k_convlat (one accumulator tile per wave): 0 = where a cost
 * model expects it to be faster (default; env TEZIP_LAT=0|1|2 sets a context's start value),
 * 1 (value 2) = never, 2 (value 4) = wherever a convolution is eligible. */
int tz_set_conv_impl(tz_ctx* ctx, int lds_dma);
/* The arithmetic contract of the predictor.  The reference leaves the float32 summation order of its
 * convolutions (prednet.py:254-277) to Keras / TensorFlow / cuDNN; this library fixes it, because a lossless decoder must
 * regenerate the encoder's predictions bit for bit (decompress.py:252-253).  1 = TZ-PA1: every convolution one direct fmaf
 * chain (rounds 1-3; what files written by earlier builds need).  2 = TZ-PA2: the per-frame convolutions of levels >= 1
 * evaluate their same-resolution source as Winograd F(2x2, 3x3) chains (2.25x fewer multiplies; oracle/tz_oracle.c
 * conv3x3_wino), everything else as in TZ-PA1.  Encoder and decoder must use the same contract: the on-disk format of the
 * reference has no place to record it.  0 (the default; or the environment variable TEZIP_PA) = by padded frame size, which
 * both sides know: TZ-PA2 from 256 x 256 pixels on, TZ-PA1 below.  tz_get_contract returns the contract in force (1 or 2)
 * for the prepared model.  Switching re-prepares nothing.
 * The prediction stack a rollout leaves in the context is STAMPED with the contract that produced it: tz_rollout_contract
 * returns that stamp (1 or 2; TZ_ERR_STATE without a rollout) -- it is what the host records next to entropy.dat
 * (tezip_amd.json) and what a decoder adopts --, and tz_encode / tz_encode_begin / tz_encode_delta / tz_decode /
 * tz_decode_delta fail with TZ_ERR_STATE when the contract in force differs from the stamp (a tz_set_contract between a
 * rollout and its encode/decode), because decompress.py:252-253 needs the decoder's predictions bit-identical to the
 * encoder's. */
int tz_set_contract(tz_ctx* ctx, int contract);
int tz_get_contract(tz_ctx* ctx);
int tz_rollout_contract(tz_ctx* ctx);
/* Diagnostic: the inverse scan of decompress.py:22-29 (k_scan2p) lets a workgroup wait for the block sums of the workgroups
 * in front of it; that wait is bounded, and an expiry surfaces as TZ_ERR_HIP at the context's next stream synchronisation
 * (tz_ctx_synchronize, or any call that delivers host results).  This entry makes the next scans wait for the status words
 * of the launch `epoch_skew` launches ahead (never written when != 0) and give up after poll_limit polls (0 = built-in
 * 2^22), so that a test can see the failure path; (0, 0) restores normal operation. */
int tz_scan_fault_inject(tz_ctx* ctx, unsigned epoch_skew, unsigned poll_limit);
/* Diagnostic: the number of blocks of the context's device scratch pool that are handed out right now (TZ_ERR_INVALID without
 * a context); *blocks (may be NULL) receives the number of blocks the pool holds.  Every entry point hands its blocks back
 * on every path it leaves by, so between calls the answer is 0, and a pool that recycles does not grow from one job to the
 * same job again.  Launches nothing. */
int tz_pool_held(tz_ctx* ctx, int* blocks);
/* Diagnostic: the device's own statement of the predictor's scalar functions (prednet.py:79-81,198-205: Keras
 * hard_sigmoid and tanh in the fixed arithmetic of DESIGN.md section 3) on n caller-chosen inputs, so that a test can
 * compare them bit for bit with the oracle's; recip_mismatches (may be NULL) receives the number of float32 values d in
 * [4, 2^27] for which the kernels' division-free 1 - 2/d differs from the IEEE division it stands for (must be 0). */
int tz_act_probe(tz_ctx* ctx, const float* x, size_t n, float* hard_sigmoid, float* tanh_out,
                 unsigned long long* recip_mismatches);

/* ---- rollout (compress.py:183-268 encoder; decompress.py:115-186 decoder) -----------------
 * frames: nt*H*W*3 uint8.  window > 0: SWP (-w); window == 0: DWP with `threshold` (-t).
 * key_mask[nt] (host) receives 1 for key frames.  mse_log (host, nt doubles, may be NULL)
 * receives the per-step window MSE of compress.py:246 (entries 0..warm_up are 0); it is
 * always computed for DWP and only on request for SWP.
 * The prediction stack (nt padded float32 frames; key slots hold C0) and the frames stay in
 * the context for tz_encode.  Rejects nt < warm_up+2 (the reference misbehaves there). */
int tz_rollout(tz_ctx* ctx, const uint8_t* frames, int nt, int H, int W, int warm_up, int window,
               double threshold, uint8_t* key_mask, double* mse_log);
/* Streaming ingestion (the reference holds every frame in RAM, compress.py:116-122): instead of one
 * stack, stage the frames window by window -- tz_frames_begin(nt,H,W), then tz_frames_put for any
 * partition of [0,nt) (asynchronous on the context's copy stream; a pageable source is free again
 * on return, a pinned one after tz_frames_fence) -- and call tz_rollout with frames == NULL.
 * tz_frames_get copies frames of the resident stack back (e.g. the key frames for key_frame.dat). */
int tz_frames_begin(tz_ctx* ctx, int nt, int H, int W);
int tz_frames_put(tz_ctx* ctx, int first, int count, const uint8_t* frames);
int tz_frames_fence(tz_ctx* ctx);
int tz_frames_get(tz_ctx* ctx, int first, int count, uint8_t* out);
/* Decoder replay: key_frames = the key_frame.dat stack (zeros except key frames); key
 * positions are recovered as decompress.py:123-129 does (any non-zero sample). */
int tz_rollout_decode(tz_ctx* ctx, const uint8_t* key_frames, int nt, int H, int W, int warm_up,
                      uint8_t* key_mask);
/* Copy out the prediction stack of the last rollout: nt*Hp*Wp*3 float32. */
int tz_get_predictions(tz_ctx* ctx, float* out);
/* ---- closed-loop prediction, definition TZ-CL1 (no reference counterpart: inside a window compress.py:230 feeds the predictor
 * its own last prediction, so a w-frame window ends on a (w-1)-step extrapolation; `tezip.py -c --loop closed`, DESIGN.md
 * section 9, slow statement in tezip_amd/closedloop.py).  The decoder holds the decoded frame t-1 when it predicts frame t; fed
 * THAT frame, every prediction is a one-step prediction, and encoder and decoder stay in lock-step because both feed the same
 * decoded bytes.
 *   key mask, groups   exactly those of tz_rollout with the same warm_up and window > 0 (a trigger on frame nt-1 makes it a key
 *                      frame).  Frame 0, warm-up frames and key frames are stored exactly: their decoded frame is the original.
 *   non-key frame t, in order inside its window:
 *                      in     = dec[t-1] / 255 as a float32 divide, zero outside H x W (how a key frame is fed)
 *                      pred_t = next(in)
 *                      x      = trunc(f32(pred_t * 255)) cropped to H x W        d = x - orig_t
 *                      q_t    = d where the job's quantiser is the identity (tz_encode's rule), else TZ-QL1 with E = min(255, floor(|b0|))
 *                      dec[t] = clamp(x - q_t, 0, 255)                            (what tz_decode computes)
 *   stored stack       what tz_encode(mode, b0, b1) makes of the final predictions: q is a pure function of (pred_t, orig_t, bound),
 *                      so the unchanged back half reproduces the loop's q under every layout, coder and report.
 * tz_rollout_closed: frames, nt, H, W, warm_up, key_mask as tz_rollout (frames == NULL: the staged stack); window > 0.
 *   Lossless (b0 == 0, or an identity by tz_encode's rule under the quantiser in force): the decoded frame is the original, so all
 *   predictions are independent -- one schedule of "predict from a u8 frame" items over the frame stack, in full batches.
 *   Lossy: step s predicts frame k + s of every window that still has one, then k_cl_step forms d, q and dec for exactly those
 *   frames into a u8 stack the next step reads.  Needs tz_set_quantiser(1) and TZ_MODE_ABS: the greedy walk and the rel bounds
 *   are no function of one sample (TZ_ERR_UNSUPPORTED; also for window == 0, per-frame bounds, a bound map and a one-channel payload).
 *   It leaves the context as tz_rollout does (prediction stack, key mask, contract stamp) and STAMPS the loop: tz_rollout_loop
 *   returns 1 (0 after any other rollout, TZ_ERR_STATE without one).  On a stamped rollout tz_encode, tz_encode_begin, tz_encode_delta,
 *   tz_bound_probe, tz_size_probe and tz_sdelta_probe return TZ_ERR_STATE, with a message that names the loop's parameters, when
 *   called with another mode, bound or quantiser, under tz_set_frame_bounds or tz_set_bound_map, or with
 *   tz_set_payload_channels(ctx, 1): the predictions serve the loop's job alone.
 * tz_rollout_decode_closed: key_frames / key discovery as tz_rollout_decode; payload (host, device, or NULL = the payload staged
 *   with tz_payload_begin / tz_payload_put), payload_len == nt*H*W*3, table / table_len as tz_decode.  The payload becomes q by the
 *   inverse remap and inverse spatial delta of the layout in force (flat, tz_set_delta_stride, tz_set_delta_plane; byte planes are
 *   undone by the caller as for tz_decode); then the same loop runs with k_cl_recon (dec = clamp(x - q, 0, 255)) on each step's
 *   frames, reading dec[t-1] from its own output.  The decoded stack stays resident for tz_decoded_get / tz_decoded_digests.
 *   A one-channel payload is TZ_ERR_UNSUPPORTED. */
int tz_rollout_closed(tz_ctx* ctx, const uint8_t* frames, int nt, int H, int W, int warm_up, int window, int mode, double b0,
                      double b1, uint8_t* key_mask);
int tz_rollout_loop(tz_ctx* ctx);
int tz_rollout_decode_closed(tz_ctx* ctx, const uint8_t* key_frames, int nt, int H, int W, int warm_up, const int16_t* payload,
                             size_t payload_len, const int16_t* table, int table_len, uint8_t* key_mask);
/* ---- the closed loop under one abs bound per frame, definition TZ-CLF1 (no reference counterpart; slow
 * statement in tezip_amd/closedframes.py).  TZ-CL1 except for the tolerance of a non-key frame t: q = Q_{E_t}(d) with
 * E_t = min(255, floor(b_t)), TZ-QL1's quantiser.  When the loop stands at frame t, pred_t is fixed (it depends on dec[t-1] alone),
 * so b_t can be GIVEN, or FOUND there: sse_t(k) = sum (clamp(x - Q_{k/2}(x - orig_t), 0, 255) - orig_t)^2 over the frame's H*W*3
 * samples; lo = 0, hi = 511, mid = (lo + hi) / 2, pass <=> sse_t(mid) <= sse_limit, at most 9 rounds; k_t = lo, b_t = k_t / 2.
 * Per searched frame: sse_t(k_t) <= sse_limit, and k_t == 510 or sse_t(k_t + 1) > sse_limit -- a boundary, not the largest passing
 * bound, and greedy in time: sse_t is taken given the dec[t-1] the earlier frames' results produced.
 * tz_rollout_closed_frames: frames, nt, H, W, warm_up, window, key_mask as tz_rollout_closed.  Exactly one of bounds (nt finite
 *   numbers >= 0; entries at frame 0, warm-up and key frames are taken as 0) and sse_limit > 0 (TZ_ERR_INVALID otherwise, and for a
 *   bound that is negative or not finite).  TZ_ERR_UNSUPPORTED, naming the setter, unless: tz_set_quantiser(1), a three-channel
 *   payload, no tz_set_bound_map, no tz_set_frame_bounds in force, no tz_set_pred_select / tz_set_pred_motion, window > 0.
 *   Per step: the predictor; for a search 9 launches of k_clf_probe (one bisection round each for every frame of the step, the
 *   sums kept on the device); k_clf_step, which decodes the step's frames under their own E.  No host wait inside the loop; one
 *   copy-back behind it.  Given bounds whose E are all 0 run the lossless closed job's one schedule.
 *   It stamps the loop as tz_rollout_closed does (tz_rollout_loop returns 1), and the stamp carries the bounds (0 at fixed frames):
 *   tz_encode, tz_encode_begin, tz_encode_delta, tz_bound_probe, tz_size_probe and tz_sdelta_probe return TZ_ERR_STATE unless the
 *   mode is TZ_MODE_ABS, the quantiser the lattice and tz_set_frame_bounds holds exactly those bounds (b0 / b1 are not read).  The
 *   unchanged back half then forms the loop's q again, and the stream is an ordinary closed-loop stream: tz_rollout_decode_closed
 *   decodes it.
 * tz_loop_frame_bounds(ctx, bounds, sse, cap): the stamp's nt bounds and, after a search, sse_t(k_t) (0 at fixed frames, at k_t = 0
 *   and after given bounds); either pointer may be NULL.  Returns nt.  TZ_ERR_INVALID for cap < nt.
 * tz_loop_search_trace(ctx, sse, cap): the search's 9*nt sums, round-major (sse[r*nt + f]); 2^64-1 where round r did not run for
 *   frame f (a fixed frame, or an interval that had closed).  Returns 9*nt.
 *   Both: TZ_ERR_STATE when the resident rollout is of another kind (the trace also after given bounds). */
int tz_rollout_closed_frames(tz_ctx* ctx, const uint8_t* frames, int nt, int H, int W, int warm_up, int window, const double* bounds,
                             unsigned long long sse_limit, uint8_t* key_mask);
int tz_loop_frame_bounds(tz_ctx* ctx, double* bounds, unsigned long long* sse, int cap);
int tz_loop_search_trace(tz_ctx* ctx, unsigned long long* sse, int cap);
/* ---- the closed loop under one abs bound per pixel, definition TZ-CLM1 (no reference counterpart; `tezip.py -c --loop closed --quant
 * lattice -m abs --loop-map FILE`; slow statement in tezip_amd/closedmap.py).  TZ-CL1 except for the quantiser
 * of a non-key frame: q = Q_{M[p]}(d), TZ-QL1 with E = M[p] of the bound map in force (tz_set_bound_map), the same E for the three
 * channels of a pixel in every frame; dec = clamp(x - q, 0, 255) is fed to the next step.  |dec - orig| <= M[p] at every sample, a
 * pixel with M = 0 is restored exactly, a map that is k everywhere gives tz_rollout_closed's job under abs k byte for byte.
 * tz_rollout_closed_map: frames, nt, H, W, warm_up, window, key_mask as tz_rollout_closed (frames NULL: the staged stack).
 *   TZ_ERR_STATE without a bound map in force, TZ_ERR_INVALID when its size is not H x W (both name tz_set_bound_map).
 *   TZ_ERR_UNSUPPORTED, naming the setter, unless: tz_set_quantiser(1), a three-channel payload, no tz_set_frame_bounds in force, no
 *   tz_set_pred_motion, window > 0.  Under tz_set_pred_select(1) it runs TZ-PS1 with that Q (cost_c = sum |Q_{M[p]}(x_c - orig)|),
 *   and tz_pred_modes delivers the modes as after tz_rollout_closed.  A map of zeros takes the lossless closed job's one schedule.
 *   Per step: the predictor, then k_clm_step (or k_psm_step), which reads the context's own H*W-byte map; no host wait inside the loop.
 *   It stamps the loop as tz_rollout_closed does (tz_rollout_loop returns 1), and the stamp carries the map's bytes: tz_encode,
 *   tz_encode_begin, tz_encode_delta, tz_bound_probe, tz_size_probe and tz_sdelta_probe return TZ_ERR_STATE, naming
 *   tz_rollout_closed_map, unless the mode is TZ_MODE_ABS, the quantiser the lattice and the map in force holds exactly those bytes
 *   (b0 / b1 are not read; setting an equal map again is fine).  The unchanged back half then forms the loop's q again
 *   (tz_encode_begin and tz_size_probe go on to refuse any bound map, as ever), tz_encode_map_check and the quality, SSIM and digest
 *   entries work on the payload, and the stream is an ordinary closed-loop stream: tz_rollout_decode_closed decodes it and never
 *   sees a bound.  tz_rollout_closed under a map stays TZ_ERR_UNSUPPORTED. */
int tz_rollout_closed_map(tz_ctx* ctx, const uint8_t* frames, int nt, int H, int W, int warm_up, int window, uint8_t* key_mask);
/* ---- per-tile choice between the network and the frame in front, definition TZ-PS1 (no reference counterpart;
 * `tezip.py -c --loop closed --pred select`, DESIGN.md section 9, slow statement in tezip_amd/predselect.py).  In a closed loop both
 * sides hold dec[t-1] when frame t is predicted: a second predictor.  TZ-PS1 is TZ-CL1 except for the value x of a non-key frame:
 *   tiles       16 x 16 pixels over the unpadded frame, TH = ceil(H/16) by TW = ceil(W/16), all three channels; edge tiles own the
 *               samples inside the frame
 *   mode        m = 1 iff sum |Q(dec[t-1] - orig_t)| < sum |Q(x_net - orig_t)| over the tile, Q the loop's quantiser, integers; a
 *               tie goes to the network; key frames have mode 0
 *   x           m ? dec[t-1] : x_net;  q = Q(x - orig);  dec[t] = clamp(x - q, 0, 255).  The network is always fed dec[t-1].
 *   predictions a chosen tile is written into the prediction stack as (v + 0.5f) / 255.0f (1.0f for v = 255), which truncates back
 *               to v: tz_encode, the probes, tz_encode_quality, tz_encode_ssim and tz_encode_digests work on it unchanged.
 * tz_set_pred_select(ctx, on): on = 0 (the default) or 1.  Under 0 tz_rollout_closed and tz_rollout_decode_closed make exactly the
 *   launches they make without this call.  The open-loop entry points ignore the setting.  The setting a closed loop ran under is
 *   part of its stamp: tz_encode and the other calls listed at tz_rollout_closed return TZ_ERR_STATE under the other setting.
 * tz_pred_modes(ctx, out, cap): after a tz_rollout_closed under selection, the nt*TH*TW mode bytes (0 / 1): frame-major, row-major
 *   tiles, 0 at key frames.  TZ_ERR_STATE when the resident rollout is not such a rollout, TZ_ERR_INVALID for cap < nt*TH*TW.
 * tz_put_pred_modes(ctx, modes, n): the modes of the stream, ahead of a tz_rollout_decode_closed under selection (host memory; the
 *   context keeps a copy).  TZ_ERR_INVALID for a byte above 1, and from the rollout for n != nt*TH*TW or a set byte in a key frame. */
int tz_set_pred_select(tz_ctx* ctx, int on);
int tz_get_pred_select(tz_ctx* ctx);
int tz_pred_modes(tz_ctx* ctx, uint8_t* out, size_t cap);
int tz_put_pred_modes(tz_ctx* ctx, const uint8_t* modes, size_t n);
/* ---- motion-compensated tiles, definition TZ-PM1 (no reference counterpart; `tezip.py -c --loop closed --pred motion`, DESIGN.md
 * section 9, slow statement in tezip_amd/predmotion.py).  TZ-PS1 with another second candidate: the frame in front DISPLACED per tile,
 *   ref(y, x, c) = dec[t-1][clamp(y + dy, 0, H-1), clamp(x + dx, 0, W-1), c],  -7 <= dy, dx <= 7 (the edge is replicated)
 *   search      on raw u8 values: SAD(dy, dx) = sum |ref - orig_t| over the tile's samples inside the frame; the tile's vector has
 *               the smallest SAD * 4096 + (|dy| + |dx|) * 256 + (dy + 7) * 16 + (dx + 7) of all 225
 *   mode        m = 1 iff sum |Q(ref - orig_t)| < sum |Q(x_net - orig_t)| at that vector; a tie goes to the network.  Tiles of mode 0
 *               and of key frames have the vector (0, 0).  x, q, dec[t], the feedback and the patched predictions as in TZ-PS1 with
 *               ref in dec[t-1]'s place.
 * tz_set_pred_motion(ctx, r): r = 0 (the default, off) or 7.  It excludes tz_set_pred_select(ctx, 1) and the other way round
 *   (TZ_ERR_INVALID).  Under 0 every launch is what it is without this call.  The setting is part of the closed loop's stamp like
 *   tz_set_pred_select's.  tz_pred_modes and tz_put_pred_modes serve a motion rollout too.
 * tz_pred_vectors(ctx, out, cap): after a tz_rollout_closed under motion, 2*nt*TH*TW int8, (dy, dx) per tile in the order of the
 *   mode bytes.  TZ_ERR_STATE when the resident rollout is not such a rollout, TZ_ERR_INVALID for cap < 2*nt*TH*TW.
 * tz_put_pred_vectors(ctx, vectors, n): the vectors of the stream, next to tz_put_pred_modes, ahead of a tz_rollout_decode_closed
 *   under motion (host memory; the context keeps a copy).  TZ_ERR_INVALID for a component outside -7 .. 7, and from the rollout for
 *   n != 2*nt*TH*TW or a non-zero vector on a tile of mode 0 (a key frame's tiles among them). */
int tz_set_pred_motion(tz_ctx* ctx, int r);
int tz_get_pred_motion(tz_ctx* ctx);
int tz_pred_vectors(tz_ctx* ctx, int8_t* out, size_t cap);
int tz_put_pred_vectors(tz_ctx* ctx, const int8_t* vectors, size_t n);

/* ---- encoder back half on the context-resident rollout (compress.py:289-373) ---------------
 * payload: nt*H*W*3 int16 = rank(1600 - sd) when bit 0 of `entropy` is set, else sd.
 * Bit 1 of `entropy` (value 2; NOT a reference feature, off in the reference's format): the
 * payload is returned byte-shuffled, i.e. as nt*H*W*3 low bytes followed by as many high bytes.
 * table: >= TZ_MAX_TABLE int16 (host), *table_len receives T (or -1 when entropy == 0).
 * delta_out (may be NULL): the int16 delta stack after quantisation, before the spatial delta.
 * A job whose WORST-CASE tolerance is <= 0.499 (abs |b0|; rel / pwrel 255 b0; absrel the smaller of |b0| and 255 b1)
 * is served by the lossless kernels: compress.py:23-70 then leaves every integer delta as it is (two different
 * neighbours always close a run, and a run of equal deltas d gets trunc((fl(d+E) + fl(d-E)) / 2) = d; proof at
 * tz_quant_is_identity in csrc/tz_codec.hip).  The result is the general quantiser's, byte for byte; TEZIP_QMAP=0 runs
 * that instead. */
int tz_encode(tz_ctx* ctx, int mode, double b0, double b1, int entropy, int16_t* payload,
              int16_t* table, int* table_len, int16_t* delta_out);
/* Opt-in one-channel payload of a gray job (no reference counterpart: compress.py:114 widens a single-channel source to RGB and
 * the payload carries every delta three times; `tezip.py -c --gray`, format in DESIGN.md section 9, slow statement of it in
 * tezip_amd/graypayload.py).  channels: 3 (the default: every entry point does exactly what it does without this call) or 1;
 * anything else is TZ_ERR_INVALID.  tz_get_payload_channels returns the value in force.  With 1:
 *  - tz_encode first checks that EVERY frame of the resident stack is gray (three equal channels at every pixel, k_key_gray)
 *    and returns TZ_ERR_INVALID naming the first frame that is not: the library never drops colour.  The quantiser runs per
 *    frame and channel (compress.py:316-319) and the decoder's predictions depend on the key frames alone
 *    (decompress.py:143-175), so channel 0 of the quantised delta stack reconstructs channel 0 within the bound, and the
 *    other two channels, whose originals equal channel 0, get the same sample and the same error.  The payload holds the
 *    nt*H*W elements of finding_difference (compress.py:73-77) over channel 0 alone, the rank table is built from their
 *    histogram; payload == NULL, the deferred hand-over and the shuffle bit (nt*H*W a multiple of 8) work as with 3.  A
 *    non-NULL delta_out is TZ_ERR_INVALID.
 *  - tz_decode, tz_decode_range, tz_encode_quality and tz_encode_digests take payload_len == nt*H*W and still yield frames of
 *    H*W*3 bytes, the decoded sample written to all three channels; tz_undelta_carry serves a range with n0 = first*H*W.
 *  - tz_encode_begin, tz_encode_finish, tz_encode_delta and tz_decode_delta return TZ_ERR_UNSUPPORTED (sharded gray jobs are
 *    out of scope).  tz_huff_* / tz_huffr_* code whatever the resident payload holds. */
int tz_set_payload_channels(tz_ctx* ctx, int channels);
int tz_get_payload_channels(tz_ctx* ctx);
/* Opt-in stride of the payload's spatial delta (no reference counterpart: finding_difference, compress.py:73-77, subtracts the
 * flat neighbour, which on a colour stack is another channel of the same pixel; `tezip.py -c --sdelta channel`, format in
 * DESIGN.md section 9, slow statement in tezip_amd/sdelta.py).  mode 0 (the default: every entry point does exactly what it does
 * without this call) = flat; mode 1 = the channel stride S = tz_get_payload_channels(): out[i] = in[i] for i < S, else
 * in[i-S] - in[i] (int16 wrap), over the flattened stack across pixel, row and frame boundaries.  Anything else is
 * TZ_ERR_INVALID.  A change drops a resident payload.  With a one-channel payload S = 1 and mode 1 is the flat delta.  Under
 * mode 1 with three channels:
 *  - tz_encode (payload == NULL, the deferred hand-over, the shuffle bit and delta_out included) yields the strided payload:
 *    quantiser, 1600 offset, histogram, rank table and remap are unchanged, sd stays in [-510, 510].
 *  - tz_decode, tz_decode_range, tz_encode_quality, tz_encode_ssim and tz_encode_digests take such a payload and yield what they
 *    yield under mode 0 from the flat payload of the same job.
 *  - tz_encode_begin, tz_encode_finish, tz_encode_delta, tz_decode_delta and tz_undelta_carry return TZ_ERR_UNSUPPORTED under
 *    mode 1 (whatever the channel count): one carry element is not the carry of a strided scan, sharded jobs are out of scope. */
int tz_set_delta_stride(tz_ctx* ctx, int mode);
int tz_get_delta_stride(tz_ctx* ctx);
/* Opt-in 2-D spatial delta of the payload, definition TZ-SD2 (no reference counterpart; `tezip.py -c --sdelta plane`, format in
 * DESIGN.md section 9, slow statement in tezip_amd/sdelta.py encode_plane / decode_plane).  on: 0 (the default: every entry point
 * launches exactly what it launches without this call) or 1; anything else is TZ_ERR_INVALID.  A change drops a resident payload.
 * tz_set_delta_plane(1) while tz_set_delta_stride(1) is in force is TZ_ERR_INVALID, and so is tz_set_delta_stride(1) while
 * tz_set_delta_plane(1) is.  With q[f, y, x, c] the quantised delta stack, C = tz_get_payload_channels() and every neighbour
 * outside the frame taken as 0, per frame and channel
 *     sd = wrap9(q[y, x-1] + q[y-1, x] - q[y-1, x-1] - q[y, x]),   wrap9(v) = ((v + 256) mod 512) - 256  in [-256, 255]
 * and the symbol is 1600 - sd in [1345, 1856]: TZ_NBINS and TZ_MAX_TABLE hold.  The inverse is q = wrap9(S), S the inclusive 2-D
 * prefix sum of -sd over the frame and channel.  Every frame is coded on its own.  On one channel this is NOT the flat delta.
 * Under 1:
 *  - tz_encode (payload == NULL, the deferred hand-over, the shuffle bit, delta_out with three channels, tz_set_frame_bounds and
 *    both quantisers) yields the plane payload, by the unfused chain in every mode: delta, quantiser, k_sdelta_plane with the
 *    histogram, remap.  tz_encode_delta and tz_bound_probe do not depend on the spatial delta and serve as ever.
 *  - tz_decode, tz_decode_range, tz_encode_quality, tz_encode_ssim and tz_encode_digests take such a payload and yield what they
 *    yield without the call from the flat payload of the same job; tz_decode_range with first > 0 computes no carry and reads
 *    nothing in front of the range.
 *  - tz_encode_begin, tz_encode_finish, tz_decode_delta, tz_undelta_carry, tz_undelta_carry_stride and tz_size_probe return
 *    TZ_ERR_UNSUPPORTED with a message that names tz_set_delta_plane.  (tz_sdelta_probe sizes the plane payload next to the
 *    flat and the channel-stride one, whatever this setting says.) */
int tz_set_delta_plane(tz_ctx* ctx, int on);
int tz_get_delta_plane(tz_ctx* ctx);
/* The seams of TZ-SD2, whatever the context's setting: nframes x H x W x channels int16 elements (channels 3 or 1), host or
 * device buffers at any 2-byte alignment.  tz_spatial_delta_plane: out = sd, or 1600 - sd when apply_offset; the counts of out
 * are ADDED to hist (TZ_NBINS words, may be NULL).  tz_spatial_undelta_plane: the inverse; table_len -1: `in` holds sd as
 * stored, else the ranks of the symbols 1600 - sd under `table` (tz_decode's reading of a payload). */
int tz_spatial_delta_plane(tz_ctx* ctx, const int16_t* in, int nframes, int H, int W, int channels, int apply_offset, int16_t* out,
                           unsigned long long* hist);
int tz_spatial_undelta_plane(tz_ctx* ctx, const int16_t* in, int nframes, int H, int W, int channels, const int16_t* table,
                             int table_len, int16_t* out);
/* Opt-in: one abs tolerance per frame (no reference counterpart: compress.py takes one bound per job, but its error_bound runs
 * per frame and channel, compress.py:316-319, so a frame's quantised delta depends on that frame's tolerance alone;
 * `tezip.py -c --target-psnr DB --per-frame`, `-c -m abs --frame-bounds FILE`).
 * bounds: n host doubles, bounds[f] = the abs tolerance of frame f.  NULL or n == 0 clears the setting.  A NaN, infinite or
 * negative entry, or n < 0, is TZ_ERR_INVALID and leaves the setting as it was.  tz_get_frame_bounds returns n, 0 when none
 * is set.  With nothing set every entry point launches exactly what it launches without these calls.  While bounds are set:
 *  - tz_encode, tz_encode_delta, tz_bound_probe, tz_size_probe and tz_sdelta_probe quantise frame f of the context's encoder rollout as
 *    `abs bounds[f]` does: the quantised delta of frame f is bit for bit the one tz_encode_delta(ctx, TZ_MODE_ABS, bounds[f],
 *    0, ...) leaves for frame f, and a bound of 0 leaves the frame's deltas untouched, as `abs 0` does.  Frames the encoder
 *    never quantises (frame 0, warm-up and key frames) stay as they are whatever their entry says.
 *  - mode must be TZ_MODE_ABS (b0 and b1 are not read) and n must equal the rollout's nt: else TZ_ERR_INVALID, with a
 *    message that names the rule.
 *  - tz_encode_begin and tz_encode_finish return TZ_ERR_UNSUPPORTED (sharded jobs take one bound).
 *  - the stand-alone tz_error_bound is not affected; the decoder never sees a bound, so tz_decode, tz_encode_quality,
 *    tz_encode_ssim and tz_encode_digests take the payload as any other.
 * The payload is the one the unfused chain gives (tz_encode_delta, then the layout's spatial delta), whichever fused pass
 * serves: the lossless one when every bound is 0 or an identity (E <= 0.499), else the fused lossy front with the per-frame
 * tolerances (one small launch, k_q_frame_bound, fills the per-chain array that rel / absrel jobs fill from the data). */
int tz_set_frame_bounds(tz_ctx* ctx, const double* bounds, int n);
int tz_get_frame_bounds(tz_ctx* ctx);
/* Opt-in: one abs tolerance per PIXEL, definition TZ-BM1 (no reference counterpart: compress.py takes one bound per job;
 * `tezip.py -c -m abs --bound-map FILE`; DESIGN.md section 9, slow statement in tezip_amd/boundmap.py).
 * map: H x W host bytes, row-major, of the source frames' own (unpadded) size: map[y * W + x] is the abs tolerance, an integer
 * 0..255, of all three channels of pixel (y, x) in every frame the encoder quantises.  NULL clears the setting.  H < 1 or W < 1
 * with a map is TZ_ERR_INVALID.  The map is copied to the device in this call and stays resident: H * W bytes, shared by all
 * frames and channels -- no per-frame or per-channel copy of it is ever made.  tz_get_bound_map returns 1 and the size, or 0.
 * With no map set every entry point launches exactly what it launches without these calls.  A change drops a resident payload.
 *   Greedy quantiser (tz_set_quantiser 0): per quantised frame and channel the chain of H * W deltas in row-major order is
 *   walked as compress.py:55-67 walks it, with E_i = (double)map[i], Du = d + E_i, Dl = d - E_i: the reference's pwrel walk
 *   with the tolerance vector replaced by the map (error_bound(map, diff, "pwrel", (1.0,)) is it, bit for bit).
 *   Lattice quantiser (tz_set_quantiser 1): TZ-QL1 with e = map[p] per sample.
 * Under both |q - d| <= map[p] at every sample (a run's value lies in [l, u], a subset of every member's [d - E, d + E]; the ends
 * are integers, so the truncation of (u + l) / 2 stays inside), hence |decoded - original| <= map[p]; a pixel with map 0 is
 * restored exactly; a map that is k everywhere gives byte for byte the job `abs k`; a map of zeros gives the lossless job.
 * While a map is set:
 *  - tz_encode (payload == NULL, the deferred hand-over, the shuffle bit and delta_out included), tz_encode_delta,
 *    tz_bound_probe and tz_sdelta_probe quantise by TZ-BM1 under the context's quantiser and honour tz_set_payload_channels,
 *    tz_set_delta_stride and tz_set_delta_plane.  Frame 0, warm-up and key frames are stored exactly, as ever.
 *  - mode must be TZ_MODE_ABS (b0 and b1 are not read) and the map's size must be the rollout's H, W: else TZ_ERR_INVALID with
 *    a message that names the rule.
 *  - tz_set_frame_bounds is TZ_ERR_INVALID and leaves both settings as they were; tz_set_bound_map while frame bounds are set is
 *    refused the same way.
 *  - tz_encode_begin, tz_encode_finish and tz_size_probe return TZ_ERR_UNSUPPORTED.
 *  - a map whose maximum is 0 is the lossless job byte for byte and takes the lossless kernels.
 *  - the greedy walk is the per-element one in float64 (the Q_TOL_MAP instantiations of k_q_tiles, k_q_bstitch and k_q_serial),
 *    with the direct-from-predictions front where uniform abs jobs have it; the lattice runs k_lattice_sd / k_lattice with the
 *    same source.  The decoder never sees a bound: tz_decode, tz_decode_range, tz_encode_quality, tz_encode_ssim and
 *    tz_encode_digests take the payload as any other, and with the default formats so does the reference's decoder. */
int tz_set_bound_map(tz_ctx* ctx, const uint8_t* map, int H, int W);
int tz_get_bound_map(tz_ctx* ctx, int* H, int* W);
/* The seams of TZ-BM1, independent of the context's settings: the int16 stack diff (nframes x H x W x 3, ANY values; host or
 * device at any alignment) is quantised in place under `map` (H x W bytes, host or device at any alignment); frames with
 * skip_mask[f] != 0 (host, may be NULL) stay as they are.  No originals are needed.  tz_error_bound_map: the greedy walk;
 * tz_lattice_bound_map: TZ-QL1 (diff 2-byte aligned). */
int tz_error_bound_map(tz_ctx* ctx, int16_t* diff, const uint8_t* skip_mask, int nframes, int H, int W, const uint8_t* map);
int tz_lattice_bound_map(tz_ctx* ctx, int16_t* diff, const uint8_t* skip_mask, int nframes, int H, int W, const uint8_t* map);
/* tz_map_check: the check kernel of TZ-BM1 over any two unpadded uint8 stacks of nframes x H x W x 3 (host or device) and a map
 * of H x W bytes (host or device): out[f] (host or device, complete on return) = the number of samples of frame f with
 * |decoded - orig| > map[pixel] and the largest excess.  Exact integers.  nframes <= 0 does nothing.
 * tz_encode_map_check: the front of tz_encode_quality (the decoder's tail over the stored payload with the encoder's own
 * predictions; its arguments, state rules and errors), then that kernel against the originals under the context's map
 * (TZ_ERR_STATE when none is set).  Nothing of the context changes. */
int tz_map_check(tz_ctx* ctx, const uint8_t* orig, const uint8_t* decoded, const uint8_t* map, int nframes, int H, int W,
                 tz_map_record* out);
int tz_encode_map_check(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len, int shuffled,
                        tz_map_record* out);
/* Opt-in: the quantiser of a lossy job (no reference counterpart: compress.py:23-70 is the only one the reference has, a greedy
 * walk that merges runs of neighbouring deltas which fit into one 2E window; `tezip.py -c --quant lattice`, DESIGN.md section 9,
 * slow statement in tezip_amd/lattice.py).  q: 0 (the default: every entry point launches exactly what it launches without this
 * call) = that greedy walk; 1 = the lattice quantiser, definition TZ-QL1: for a delta d in [-255, 255] and the tolerance e, the
 * float64 the greedy walk forms (abs |b0|; rel (max - min of the slab) * b0; absrel the smaller of the two; pwrel orig * b0 per
 * element; under tz_set_frame_bounds bounds[f])
 *     E = min(255, floor(e))      s = 2E + 1      q = clamp(sign(d) * ((|d| + E) div s) * s, -255, 255)
 * so that |q - d| <= E <= e (the clamp projects onto an interval that contains d), |q| <= 255 (the spatial delta stays in
 * [-510, 510]: TZ_NBINS and TZ_MAX_TABLE hold), e < 1 is the identity and E = 255 maps everything to 0.  A pure function of one
 * delta and one tolerance: no walk, no stitch, no serial fallback.  Anything else is TZ_ERR_INVALID.  tz_get_quantiser returns
 * the value in force.  A change drops a resident payload.  Under 1:
 *  - tz_encode (payload == NULL, the deferred hand-over, the shuffle bit and delta_out included), tz_encode_delta,
 *    tz_bound_probe, tz_size_probe and tz_sdelta_probe quantise by TZ-QL1 and honour tz_set_frame_bounds, tz_set_payload_channels and
 *    tz_set_delta_stride as under 0.  Frame 0, warm-up frames and key frames are not quantised, as under 0; an unknown mode, a
 *    NaN and a negative rel / pwrel tolerance are refused where they are refused under 0.
 *  - a job whose worst-case tolerance is below 1 (abs |b0|; rel / pwrel 255 b0; absrel the smaller of |b0| and 255 b1; every
 *    frame bound) is the lossless job, byte for byte, and takes the lossless kernels.
 *  - where the lossless one-pass front applies (unpadded frames of whole 16-byte groups, no delta_out) tz_encode runs ONE pass
 *    over predictions and originals in every layout (k_lattice_sd: delta, TZ-QL1, the layout's spatial delta, offset,
 *    histogram); elsewhere the delta stack is quantised in place (k_lattice) between the kernels of the unfused chain.  The
 *    payload is the same.
 *  - tz_encode_begin and tz_encode_finish return TZ_ERR_UNSUPPORTED (sharded jobs are out of scope).
 *  - the payload carries the quantised deltas themselves, not lattice indices: the decoder never sees a bound, so tz_decode,
 *    tz_decode_range, tz_encode_quality, tz_encode_ssim and tz_encode_digests take the payload as any other, and with the
 *    default formats so does the reference's decoder. */
int tz_set_quantiser(tz_ctx* ctx, int q);
int tz_get_quantiser(tz_ctx* ctx);
/* Streaming delivery: tz_encode with payload == NULL keeps the payload in the context; it is then
 * fetched in pieces of `count` int16 elements starting at `offset` (compress.py:375-400 appends and
 * compresses one monolithic array). */
int tz_payload_get(tz_ctx* ctx, size_t offset, size_t count, int16_t* out);
/* Deferred hand-over of the payload (a caller that compresses one sequence after the other; compress.py:375-400 is one
 * blocking pass per job).  With tz_set_payload_deferred(ctx, 1) a tz_encode whose `payload` is PINNED host memory
 * (tz_host_alloc) and whose entropy bit is set returns as soon as the last chunk of the payload is queued on the copy
 * stream: table and *table_len are final, the payload buffer is complete only after tz_payload_wait -- the device -> host
 * transfer (2.4 ms for a cfg3 sequence) then runs under the next sequence's tz_rollout instead of in front of it.  At
 * most one transfer is in flight: the next tz_encode orders its own remap behind it, so a caller alternates between two
 * host buffers and calls tz_payload_wait (free by then) before it reads the older one.  Every other form of tz_encode,
 * tz_ctx_synchronize and tz_ctx_destroy settle a transfer in flight first. */
int tz_set_payload_deferred(tz_ctx* ctx, int on);
int tz_payload_wait(tz_ctx* ctx);
/* First stage of tz_encode only (compress.py:292-319): delta + error-bound quantisation of the
 * context-resident rollout -> int16 delta stack nt*H*W*3, the stack tz_encode's delta_out receives.
 * (The sharded encoder does not need it: it runs tz_encode_begin / tz_encode_finish.) */
int tz_encode_delta(tz_ctx* ctx, int mode, double b0, double b1, int16_t* delta_out);
/* tz_encode in two phases, for jobs whose frame windows are sharded over GPUs (the
 * reference is single-process).  The spatial delta runs over the whole flattened stack
 * (compress.py:339) and the rank table comes from the global histogram (compress.py:354-361), so a
 * shard runs compress.py:292-355 on its own frames (begin), the ranks exchange one carry element
 * and sum the 2111 counters, and the shard finishes compress.py:356-373 with the global table
 * (finish).  tz_encode is the one-shard case: the same code runs both.
 * begin: hist (host, TZ_NBINS counters, may be NULL when entropy == 0) receives this shard's counts
 * taken WITHOUT a carry; edge[0], edge[1] (host) the first and the last element of the shard's
 * quantised delta stack.  edge[1] is the carry of the next shard; with its own carry c a shard moves
 * its first symbol in the histogram from 1600 - edge[0] to 1600 - (int16)(c - edge[0]).
 * finish: has_carry/carry as in tz_spatial_delta; table_len >= 0: remap with `table` (the table of the
 * summed histogram, tz_build_table), -1: no remap (must match begin's entropy flag); payload NULL: the
 * payload stays in the context (tz_payload_get). */
int tz_encode_begin(tz_ctx* ctx, int mode, double b0, double b1, int entropy, unsigned long long* hist,
                    int16_t* edge);
int tz_encode_finish(tz_ctx* ctx, int has_carry, int16_t carry, const int16_t* table, int table_len,
                     int16_t* payload);
/* ---- decoder back half (decompress.py:203-256): payload (+table) -> nt*H*W*3 uint8 frames,
 * using the prediction stack of the last tz_rollout_decode (or tz_rollout_decode_range of [0, nt)).  payload_len
 * (elements) must be nt*H*W*3 of that rollout: the reference fails at its reshape otherwise (decompress.py:240).
 * table_len: -1 = no table, else 0..TZ_NBINS (anything else is TZ_ERR_INVALID). */
int tz_decode(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len,
              uint8_t* frames_out);
/* Streaming decode (decompress.py:87-113 decompresses and holds both files whole): stage the
 * payload in pieces -- tz_payload_begin(count), tz_payload_put(offset, count, src) on the copy
 * stream -- and the key-frame stack with tz_frames_begin / tz_frames_put, then tz_rollout_decode
 * with key_frames == NULL and tz_decode with payload == NULL; with frames_out == NULL the decoded
 * frames stay in the context and are fetched window by window with tz_decoded_get. */
int tz_payload_begin(tz_ctx* ctx, size_t count);
int tz_payload_put(tz_ctx* ctx, size_t offset, size_t count, const int16_t* src);
int tz_decoded_get(tz_ctx* ctx, int first, int count, uint8_t* out);
/* Last stage of tz_decode only (decompress.py:252-256): reconstruct from an already decoded
 * int16 delta stack (sharded decoding: the inverse scan carry comes from the previous shard). */
int tz_decode_delta(tz_ctx* ctx, const int16_t* delta, uint8_t* frames_out);

/* ---- range decode (no reference counterpart: decompress.py:39 always writes every frame) -------------------
 * Frames [first, first + count) of a stream without the whole-sequence work.  The predictor restarts at every key frame
 * (decompress.py:143-175) and the inverse spatial delta (decompress.py:22-29) needs only the decoded element in front of
 * the range, so a range costs one read of the payload prefix (tz_undelta_carry), the predictor steps from the range's
 * restart frame to its last frame, and the scan + reconstruct of the range alone.
 * tz_range_restart (host only, like tz_build_table): the frame at which a decoder must start its rollout to reproduce
 * frame `first` bit for bit.  key_mask[nt]: the key frames key discovery finds (decompress.py:123-129: any non-zero
 * sample).  Rule: the largest key frame k with warm_up < k <= first, else 0.  A rollout from such a k is the sub-stack
 * [k, end) replayed with warm_up = 0: its predictions depend on frame k alone and frame k is its own base, as in the
 * whole-stack replay.  A rollout from 0 is the sub-stack [0, end) with the job's warm_up; it must reach frame warm_up
 * (the replay's key-interval walk starts there), so tz_rollout_decode_range extends it to max(end, warm_up + 1) frames
 * and returns nothing of the extension.  A sub-stack needs no other minimum length (a lone key frame is a 1-frame
 * replay); the length conditions of the sharded decoder's cuts (tezip_amd/dist.py) concern the shard in FRONT of a cut,
 * which a range never decodes.  Key frames k in (0, warm_up] are not restarts: frames below warm_up are C0 copies in the
 * replay, and from k = warm_up the predictor does exactly the steps a restart at 0 does.  Any earlier valid restart is
 * also correct, only slower. */
int tz_range_restart(const uint8_t* key_mask, int nt, int warm_up, int first, int* restart);
/* tz_rollout_decode_range: tz_rollout_decode for frames [first, first + count) only.  Key discovery runs over the whole
 * stack (key_mask[nt], host, receives it); the predictor runs over [restart, first + count) (plus the extension above)
 * of the resident stack, and the prediction stack holds those frames only.  key_frames == NULL: the stack staged with
 * tz_frames_begin / tz_frames_put, whose nt, H, W must be the call's (else TZ_ERR_INVALID).  A stack short of [0, nt)
 * serves tz_decode_range only: tz_decode / tz_get_predictions / tz_decode_delta report TZ_ERR_STATE until the next whole
 * rollout; a range of [0, nt) is the whole rollout and serves them all.  TZ_ERR_INVALID for first / count outside
 * [0, nt). */
int tz_rollout_decode_range(tz_ctx* ctx, const uint8_t* key_frames, int nt, int H, int W, int warm_up, int first, int count,
                            uint8_t* key_mask);
/* tz_undelta_carry: the decoded element x[n0-1] of the inverse spatial delta over payload[0, n0), i.e.
 * -(sum of s'[0..n0)) mod 2^16 with s'[0] = -s[0] (k_undelta_carry: one read of the prefix, 2 B/element).
 * payload == NULL: the payload staged with tz_payload_begin / tz_payload_put.  table_len == -1: the payload holds the
 * symbols as they are (no remap), else the inverse rank remap and 1600 - x of decompress.py:31-36,236 apply first, as in
 * tz_decode.  n0 == 0 is TZ_ERR_INVALID: the stream start has no carry.  *carry (host) receives the element. */
int tz_undelta_carry(tz_ctx* ctx, const int16_t* payload, size_t n0, const int16_t* table, int table_len, int16_t* carry);
/* tz_decode_range: tz_decode for frames [first, first + count), on the prediction stack of the last
 * tz_rollout_decode_range or tz_rollout_decode (the range must lie inside the frames that call covered).  payload_len is the WHOLE stream,
 * nt*H*W*3, checked as tz_decode checks it; elements behind the range are not read.  For first > 0 the scan starts from
 * tz_undelta_carry's element over [0, first*H*W*3).  frames_out: count*H*W*3 uint8, or NULL to keep the frames in the
 * context for tz_decoded_get, whose frame indices are then sequence indices inside [first, first + count). */
int tz_decode_range(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len, int first,
                    int count, uint8_t* frames_out);

/* tz_encode_quality: what the stored payload of an encode decodes to, compared with the originals (no reference
 * counterpart; `tezip.py -c --report`).  On the context's ENCODER rollout (tz_rollout, SWP or DWP; anything else, a
 * tz_rollout_decode included, is TZ_ERR_STATE) the decoder's tail -- inverse remap, inverse spatial delta, reconstruct,
 * the launches tz_decode makes -- runs over `payload` with the encoder's own predictions and frames, under the mask the
 * decoder's rollout would reconstruct with (frame 0 and every key frame from the warm_up-th on; warm-up frames 1..p-1
 * take their C0 slot), and k_quality compares the frames it yields with the originals.  The decoder's rollout
 * regenerates the encoder's predictions bit for bit, so out[f] describes frame f exactly as
 * `-u` writes it; zstd and the decoder's own rollout are not exercised.
 *  payload: nt*H*W*3 int16 (host or device), or NULL = the resident payload of the last tz_encode(payload = NULL) on the
 *           current rollout (TZ_ERR_STATE when there is none).  payload_len must be nt*H*W*3 (else TZ_ERR_INVALID).
 *  table / table_len: as tz_decode (table_len == -1: no rank table).  shuffled: the payload holds byte planes
 *           (tz_encode's opt-in shuffle); they are undone into scratch first.
 *  out:     nt records, host or device.  The call returns once they are complete.
 * Nothing of the context changes: payload, predictions, frames and rollout state are as they were.
 * Limitation: a key frame whose samples are all zero is not found again by the decoder's key discovery
 * (decompress.py:123-129) and `-u` fails on such a stream; the records describe the stream the
 * encoder meant to write. */
int tz_encode_quality(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len,
                      int shuffled, tz_frame_quality* out);

/* ---- the bound for a PSNR target (no reference counterpart; `tezip.py -c --target-psnr DB`; definition TZ-TPSNR-1 in DESIGN.md
 * section 9 and tezip_amd/target.py) ------------------------------------------------------------------------------------------
 * tz_bound_probe: one candidate bound.  On the context's ENCODER rollout (state rules and errors are tz_encode_quality's; an
 * unknown mode, a NaN or a refused negative bound are TZ_ERR_INVALID as in tz_encode) out[f] is, field for field, what
 * tz_encode(ctx, mode, b0, b1, ...) followed by tz_encode_quality would report for frame f.  The predictions do not depend on
 * the bound, so one rollout serves any number of probes.  A probe forms the delta stack, sends a copy of it through the
 * quantiser and compares the two against the originals in one pass (k_bound_err, profiling class "quality"): no spatial
 * delta, histogram, table or payload is made and nothing but the records leaves the device.
 *  out: nt records, host or device; complete on return.
 * The quantiser is the three-channel one in every layout.  Under tz_set_delta_stride(ctx, 1) the records are unchanged (the
 * spatial delta is lossless).  Under tz_set_payload_channels(ctx, 1) they describe the one-channel job, as tz_encode_quality
 * does: that job stores channel 0's quantised delta alone and its decoder writes channel 0's reconstruction to all three
 * channels, so the kernel takes channel 0's error for every channel of a pixel (the model's three output channels differ
 * even on a gray source: the three-channel job's records are NOT the one-channel job's); a stack with colour is refused as
 * tz_encode refuses it (TZ_ERR_INVALID).  Nothing of the context changes: a resident payload, its kind, predictions, frames
 * and rollout state are as they were. */
int tz_bound_probe(tz_ctx* ctx, int mode, double b0, double b1, tz_frame_quality* out);
/* tz_bound_err: the kernel of tz_bound_probe alone, over any three unpadded stacks of nframes frames of frame_elems
 * elements, host or device: per element e = clamp(orig + delta - qdelta, 0, 255) - orig, per frame sum e^2, max |e| and the
 * count of e != 0.  nframes <= 0 or frame_elems == 0 does nothing.  Under tz_set_payload_channels(ctx, 1) it is the one-channel
 * form: element i of a frame counts only where i % 3 == 0, three times (frame_elems % 3 != 0: TZ_ERR_INVALID). */
int tz_bound_err(tz_ctx* ctx, const uint8_t* orig, const int16_t* delta, const int16_t* qdelta, int nframes,
                 size_t frame_elems, tz_frame_quality* out);

/* ---- per-frame digests (no reference counterpart; `tezip.py -c --digests`, `-u --verify`; format TZD64 version 1 in
 * DESIGN.md section 9, slow statement of it in tezip_amd/digest.py) ------------------------------------------------------
 * For a frame of n bytes x[0..n) in (H, W, 3) memory order, all arithmetic mod 2^64:
 *   digest = sum over i of mix(256 * i + x[i]),  mix = splitmix64's output function
 *   (z = k + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31).
 * mix is a bijection and the keys of a frame are distinct, so a change of one sample always changes the digest; the sum is
 * commutative, so the value does not depend on how k_digest cuts a frame over lanes and workgroups (TEZIP_DIGEST_GRID
 * forces the number of workgroups, a diagnostic).  An error-detection code, NOT a cryptographic hash: it guards against
 * damage and against decoders that stopped agreeing with the encoder, not against an adversary.
 * tz_frame_digests: the stand-alone form, nframes frames of frame_bytes bytes each, frames and out (nframes words) host or
 * device.  frame_bytes >= 2^32 is TZ_ERR_INVALID before any launch; an empty frame has the digest 0. */
int tz_frame_digests(tz_ctx* ctx, const uint8_t* frames, int nframes, size_t frame_bytes, unsigned long long* out);
/* The digests of the decoded frames [first, first + count) that tz_decode / tz_decode_range left in the context with
 * frames_out == NULL, taken where they lie, before any of them is fetched; frame indices follow tz_decoded_get's rule
 * (sequence indices inside the decoded range).  TZ_ERR_STATE without such frames, TZ_ERR_INVALID for a range outside them. */
int tz_decoded_digests(tz_ctx* ctx, int first, int count, unsigned long long* out);
/* tz_encode_quality's twin: arguments, state rules and errors are exactly its own, and both run the same front (checks,
 * unshuffle, mask, the decoder's tail into scratch), so they cannot disagree about what "decoded" means.  decoded[nt]: the
 * digests of what the stored payload decodes to, i.e. of the images `-u` writes; original[nt] (may be NULL): those of the
 * resident source frames.  Host or device; complete on return.  Nothing of the context changes. */
int tz_encode_digests(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len,
                      int shuffled, unsigned long long* decoded, unsigned long long* original);

/* ---- structural similarity (no reference counterpart; `tezip.py -c --report --ssim`; definition TZ-SSIM-1, also in DESIGN.md
 * section 9, slow statement of it in tezip_amd/ssim.py) ---------------------------------------------------------------------
 * For two uint8 frames a, b of shape (H, W, 3), each channel on its own:
 *   windows  8 x 8 pixels at every origin (y, x) with y % 4 == 0, x % 4 == 0, y + 8 <= H, x + 8 <= W: per channel
 *            ((H-8)/4 + 1) * ((W-8)/4 + 1) windows when H, W >= 8, else none; a frame has three times as many.  Up to 3 rows at
 *            the bottom and 3 columns at the right edge (H % 4, W % 4) lie in no window and are not compared.
 *   moments  exact integers over the window's 64 samples: s1 = sum a, s2 = sum b, sa = sum a^2, sb = sum b^2, s12 = sum ab.
 *   factors  the usual SSIM with C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2 and the population variance, multiplied through by
 *            64^2 and by 100 so that the constants are integers; int64, all four below 2^53 in magnitude, d1, d2 > 0:
 *              n1 = 200 * s1 * s2 + 2663424                     d1 = 100 * (s1^2 + s2^2) + 2663424
 *              n2 = 200 * (64 * s12 - s1 * s2) + 23970816       d2 = 100 * (64 * (sa + sb) - s1^2 - s2^2) + 23970816
 *   value    in float64, in exactly this order: p = double(n1) * double(n2), q = double(d1) * double(d2), r = p / q,
 *            Q = llrint(r * 4294967296.0), round half to even.  There is no other floating-point operation; the library is
 *            built with -ffp-contract=off -fno-fast-math and the device's fp64 division is the correctly rounded one, so Q is
 *            the integer numpy computes (tests/test_gpu_ssim.py compares every field as integers, with no tolerance).
 *   record   sum_q32 = sum of Q, min_q32 = the smallest Q over the frame's windows (0 without a window), windows, reserved = 0.
 *            Sum and minimum of integers do not depend on how k_ssim cuts a frame over lanes and workgroups
 *            (TEZIP_SSIM_GRID forces the number of workgroups, a diagnostic): the record is a function of the two frames.
 * Figures (host, tezip_amd/ssim.py): frame SSIM = sum_q32 / (windows * 2^32); sequence SSIM = sum of sums / (sum of windows *
 * 2^32), not a mean of frame values; none where windows == 0.
 * tz_ssim_frames: the stand-alone form over two stacks of nframes frames, a, b and out (nframes records) host or device;
 * complete on return.  TZ_ERR_INVALID for nframes < 0, H or W <= 0 or a frame of 2^32 bytes or more, before any launch;
 * nframes == 0 launches nothing. */
int tz_ssim_frames(tz_ctx* ctx, const uint8_t* a, const uint8_t* b, int nframes, int H, int W, tz_frame_ssim* out);
/* tz_encode_quality's third twin: arguments, state rules and errors are exactly its own (a resident payload, the shuffle and
 * tz_set_payload_channels(ctx, 1) with payload_len == nt*H*W included) and it runs the same front, then k_ssim over the
 * decoded scratch frames and the resident originals: out[f] is the SSIM record of frame f as `-u` writes it against its
 * source.  out: nt records, host or device; complete on return.  Nothing of the context changes.  The launches are counted
 * in the profiling class "quality". */
int tz_encode_ssim(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len,
                   int shuffled, tz_frame_ssim* out);

/* ---- alignment of device buffers --------------------------------------------------------------
 * Every buffer argument below may be a host or a device pointer.  A host array is copied through the context's pool and may
 * lie anywhere.  A DEVICE buffer is handed to the kernels as it is and need only be aligned to its element type (1, 2 or 4
 * bytes: uint8_t, int16_t, float): each kernel picks its vector form from the addresses it is given and gives the same bits
 * in its element-wise form (DESIGN.md section 0 lists every wide access and the term that guards it).  The exceptions are
 * the entry points whose kernels have no element-wise form and which therefore REFUSE a device buffer, input or output,
 * that is off a 16-byte boundary: tz_spatial_delta (and tz_spatial_delta_stride with stride 1: "spatial_delta buffers must
 * be 16-byte aligned"), tz_remap and tz_unmap ("remap buffers must be 16-byte aligned"), tz_byte_shuffle and
 * tz_byte_unshuffle ("byte-shuffle buffers must be 16-byte aligned"); and tz_encode for a device `payload`, which the last
 * of these stages writes (its message).  Each refuses with TZ_ERR_INVALID and that message before any launch that writes
 * the buffer: nothing of it is written. */

/* ---- operator seams, usable stand-alone (each mirrors one reference helper) -----------------
 * tz_delta_encode: compress.py:292-314.  pred: nframes padded f32 frames; orig: nframes
 * unpadded u8 frames; zero_mask[nframes] (host): 1 => that frame's delta is forced to 0. */
int tz_delta_encode(tz_ctx* ctx, const float* pred, const uint8_t* orig, const uint8_t* zero_mask,
                    int nframes, int H, int W, int16_t* out);
/* tz_error_bound: compress.py:23-70 applied per frame and channel as compress.py:316-319 does.
 * diff is updated in place; skip_mask[nframes] (host): 1 => frame left untouched.
 * Domain: any int16 stack (the deltas of compress.py:292-314 lie in [-255, 255]; wider values take the reference's
 * double test at every step instead of the integer walk's width table -- same results, slower).
 * Negative tolerances: `abs` takes |b| (compress.py:29).  For rel / pwrel with b < 0 and absrel with a negative relative
 * bound the reference fails only where E < 0 meets the FIRST element of a chain ((inf + -inf)/2 = NaN stored into an int
 * array, compress.py:60-61) and otherwise carries on with every element a run of its own; this library rejects every
 * such call with TZ_ERR_INVALID -- a deliberate superset of the reference's failure, both oracles do the same. */
int tz_error_bound(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* skip_mask,
                   int nframes, int H, int W, int mode, double b0, double b1);
/* tz_error_bound_frames: the seam of tz_set_frame_bounds -- tz_error_bound in abs mode with one tolerance per frame.  orig and
 * diff are host or device stacks as tz_error_bound's; bounds: nframes host doubles, finite and >= 0 (else TZ_ERR_INVALID and
 * diff is untouched).  Frame f of diff ends as tz_error_bound(.., TZ_MODE_ABS, bounds[f], 0) leaves it, bit for bit; a bound
 * of 0 and a skipped frame leave it untouched.  Independent of the context's own frame bounds. */
int tz_error_bound_frames(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* skip_mask,
                          int nframes, int H, int W, const double* bounds);
/* tz_lattice_bound: the lattice quantiser TZ-QL1 (tz_set_quantiser) per frame and channel, in place, with the argument rules of
 * tz_error_bound: orig and diff host or device stacks, skip_mask[nframes] (host, may be NULL), the same refusals of an unknown
 * mode, of a NaN and of a negative rel / pwrel / absrel tolerance; b0 == 0 (and absrel with b1 == 0) leaves diff as it is.
 * Defined for every int16 delta (the error bound holds for those in [-255, 255]).  tz_lattice_bound_frames: the twin of
 * tz_error_bound_frames, abs with bounds[f] for frame f (finite and >= 0, else TZ_ERR_INVALID and diff is untouched).  Both are
 * independent of the context's own quantiser and frame bounds. */
int tz_lattice_bound(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* skip_mask,
                     int nframes, int H, int W, int mode, double b0, double b1);
int tz_lattice_bound_frames(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* skip_mask,
                            int nframes, int H, int W, const double* bounds);
/* tz_spatial_delta: compress.py:73-77 (+ the 1600 offset of :348 when apply_offset).
 * has_carry: treat `carry` as the element preceding in[0] (shard boundary). hist (may be
 * NULL): TZ_NBINS uint64 counts of the output symbols are ADDED (compress.py:354). */
int tz_spatial_delta(tz_ctx* ctx, const int16_t* in, size_t n, int has_carry, int16_t carry,
                     int apply_offset, int16_t* out, unsigned long long* hist);
/* Opt-in byte shuffle (no reference counterpart; BASELINE.json's north star names the stage):
 * int16[n] <-> n low bytes | n high bytes.  n must be a multiple of 8 for the forward direction. */
int tz_byte_shuffle(tz_ctx* ctx, const int16_t* in, size_t n, uint8_t* out);
int tz_byte_unshuffle(tz_ctx* ctx, const uint8_t* in, size_t n, int16_t* out);
/* tz_build_table: compress.py:352-361 (host): count desc, ties ascending symbol. */
int tz_build_table(const unsigned long long* hist, int nbins, int16_t* table, int* table_len);
/* tz_remap: compress.py:84-90 (symbol -> rank). */
int tz_remap(tz_ctx* ctx, const int16_t* in, size_t n, const int16_t* table, int table_len, int16_t* out);
/* tz_unmap: decompress.py:31-36 (+ 1600 - x of :236 when apply_offset). */
int tz_unmap(tz_ctx* ctx, const int16_t* in, size_t n, const int16_t* table, int table_len,
             int apply_offset, int16_t* out);
/* tz_spatial_undelta: decompress.py:22-29 as a wrap-around prefix scan. has_carry: `carry`
 * is the decoded element preceding in[0]. */
int tz_spatial_undelta(tz_ctx* ctx, const int16_t* in, size_t n, int has_carry, int16_t carry,
                       int16_t* out);
/* tz_reconstruct: decompress.py:252-256,269.  key_mask[nframes] (host): 1 => the base is
 * the key byte (key_frames), else trunc(pred*255). */
int tz_reconstruct(tz_ctx* ctx, const float* pred, const uint8_t* key_frames, const uint8_t* key_mask,
                   const int16_t* diff, int nframes, int H, int W, uint8_t* out);
/* The two kernels of the one-channel payload (tz_set_payload_channels), stand-alone.
 * tz_spatial_delta_gray: tz_spatial_delta over channel 0 of an interleaved 3-channel int16 stack.  in3: npix*3 elements in
 * (frame, y, x, 3) order; out: npix elements, out[0] = in3[0] (or carry - in3[0]), out[i] = in3[3(i-1)] - in3[3i], then
 * 1600 - x when apply_offset; channels 1 and 2 are never read.  hist as tz_spatial_delta's (symbols outside [0, TZ_NBINS)
 * are not counted). */
int tz_spatial_delta_gray(tz_ctx* ctx, const int16_t* in3, size_t npix, int has_carry, int16_t carry, int apply_offset,
                          int16_t* out, unsigned long long* hist);
/* The kernels of the channel-stride spatial delta (tz_set_delta_stride), stand-alone and independent of the context's mode.
 * stride: 1 or 3 (else TZ_ERR_INVALID); with 1 they are tz_spatial_delta / tz_spatial_undelta / tz_undelta_carry.  carry: NULL,
 * or `stride` HOST elements, the ones in front of in[0] (carry[c] in front of in[c]).
 * tz_spatial_delta_stride: out[i] = in[i-stride] - in[i] (in[i] itself for i < stride without a carry), then 1600 - x when
 * apply_offset; hist as tz_spatial_delta's.  tz_spatial_undelta_stride: the inverse, x[i] = x[i-stride] - in[i].
 * tz_undelta_carry_stride: the `stride` decoded elements in front of payload[n0] (carry_out[c] = x[n0 - stride + c]), n0 a
 * positive multiple of stride, through the rank table as tz_undelta_carry; payload NULL = the staged payload. */
int tz_spatial_delta_stride(tz_ctx* ctx, const int16_t* in, size_t n, int stride, const int16_t* carry, int apply_offset,
                            int16_t* out, unsigned long long* hist);
int tz_spatial_undelta_stride(tz_ctx* ctx, const int16_t* in, size_t n, int stride, const int16_t* carry, int16_t* out);
int tz_undelta_carry_stride(tz_ctx* ctx, const int16_t* payload, size_t n0, int stride, const int16_t* table, int table_len,
                            int16_t* carry_out);
/* tz_reconstruct_gray: tz_reconstruct from ONE int16 delta per pixel (diff1: nframes*H*W): base = the key byte of channel 0
 * where key_mask says so, else trunc(pred channel 0 * 255); v = clamp(base - d, 0, 255) goes to all three channels of out
 * (nframes*H*W*3).  pred, key_frames: the 3-channel stacks tz_reconstruct takes. */
int tz_reconstruct_gray(tz_ctx* ctx, const float* pred, const uint8_t* key_frames, const uint8_t* key_mask,
                        const int16_t* diff1, int nframes, int H, int W, uint8_t* out);
/* tz_window_sse: the inner sum of compress.py:246 for nframes (sum over the padded frame of
 * (x/255 - pred)^2 in float64, fixed summation order). sse: nframes doubles (host). */
int tz_window_sse(tz_ctx* ctx, const uint8_t* orig, const float* pred, int nframes, int H, int W, double* sse);

/* ---- opt-in Huffman coder of the payload (no reference counterpart: compress.py:375-400 hands the int16 payload to zstd;
 * `tezip.py -c --coder huff`, format in DESIGN.md section 9, slow statement of it in tezip_amd/huff.py) ---------------------
 * An order-0 canonical Huffman code over the payload's 16-bit values: symbol = value - base, alphabet A <= TZ_NBINS, code
 * lengths <= 12, codes canonical (shorter first, then by symbol), so `lengths` (A bytes, 0 = absent) is the whole code.
 * The coded stream is index | bits: one u32 word offset per chunk (64 runs), one u16 size in bits per run (256 symbols),
 * padded to 4 bytes, then the 32-bit words of the bit stream.
 * tz_huff_lengths (host only, like tz_build_table): optimal lengths under the limit max_len (package-merge) from A counts;
 * deterministic, Kraft sum exactly 1 with two or more symbols present, one present symbol gets length 1, zero counts get 0.
 * TZ_ERR_INVALID: no symbol present, more than 2^max_len present, A outside [1, TZ_NBINS], max_len outside [1, 15]. */
int tz_huff_lengths(const unsigned long long* counts, int A, int max_len, uint8_t* lengths);
/* Counts of the context-resident payload (tz_encode / tz_encode_finish with payload == NULL) in symbol order:
 * counts[TZ_NBINS] (host) receives them, *base the smallest value present, *A the span up to the largest.  One read of the
 * payload (k_huff_count).  TZ_ERR_INVALID when the values span more than TZ_NBINS symbols. */
int tz_huff_counts(tz_ctx* ctx, unsigned long long* counts, int* A, int* base);
/* Codes the context-resident payload into a context-resident stream; *bytes receives its size, tz_huff_get fetches it in
 * pieces like tz_payload_get.  The payload stays as it is.  TZ_ERR_INVALID before any launch for a bad code (A, base, a
 * length above 12, Kraft sum > 1), and after the size pass for a payload value the code has no symbol for. */
int tz_huff_encode(tz_ctx* ctx, const uint8_t* lengths, int A, int base, size_t* bytes);
int tz_huff_get(tz_ctx* ctx, size_t offset, size_t count, uint8_t* out);
/* Decoder: stage a coded stream of `bytes` bytes for n elements in pieces on the copy stream (begin, then put for any
 * partition of [0, bytes)), then expand it into the context's payload buffer exactly as if tz_payload_begin /
 * tz_payload_put had staged n elements: tz_decode (payload == NULL), tz_decode_range, tz_undelta_carry run unchanged on it.
 * R must be 256.  The caller validates the index (tezip_amd/huff.py: parse); the kernel itself clamps every offset and read
 * to the stream, so a corrupt body gives wrong symbols, never an access outside the buffers. */
int tz_huff_begin(tz_ctx* ctx, size_t bytes, size_t n, const uint8_t* lengths, int A, int base, int R);
int tz_huff_put(tz_ctx* ctx, size_t offset, size_t count, const uint8_t* src);
int tz_huff_decode(tz_ctx* ctx);
/* Stand-alone forms on host or device arrays (they use, and overwrite, the context's resident stream buffer).
 * capacity: bytes `out` holds; a larger stream is TZ_ERR_INVALID with *bytes set to what it needs. */
int tz_huff_encode_buf(tz_ctx* ctx, const int16_t* in, size_t n, const uint8_t* lengths, int A, int base, uint8_t* out,
                       size_t capacity, size_t* bytes);
int tz_huff_decode_buf(tz_ctx* ctx, const uint8_t* stream, size_t bytes, size_t n, const uint8_t* lengths, int A, int base,
                       int R, int16_t* out);

/* ---- opt-in Huffman coder with repeat tokens (`tezip.py -c --coder huffr`, format TZR1 in DESIGN.md section 9, slow
 * statement of it in tezip_amd/huffr.py) ---------------------------------------------------------------------------------
 * The coder above with a tokeniser in front: the payload interleaves three channels, so a quantiser run repeats with
 * period 3.  Element j of a run of R = 256 elements is a match when j >= 3 and equals element j - 3; a maximal stretch of
 * m matches is coded as the token T_k, k = floor(log2 m), plus k raw bits, every other element as a literal.  A code has
 * the A <= TZ_NBINS literals (symbol = value - base) and then the TZ_HUFFR_NTOK tokens: `lengths` holds A + 8 bytes and
 * `counts` TZ_NBINS + 8 entries in every call below, while A and base keep describing the literals.  Index, bit stream,
 * refusals and clamps are tz_huff_*'s; the resident stream buffer is shared with them (a tz_huffr_begin replaces a stream
 * tz_huff_begin staged and the other way round, and each decoder refuses the other's stream with TZ_ERR_STATE). */
#define TZ_HUFFR_NTOK 8
int tz_huffr_lengths(const unsigned long long* counts, int total, int max_len, uint8_t* lengths);   /* total = A + 8 */
/* counts[0 .. A) the literals, counts[A .. A + 8) the tokens T_0..T_7 of the resident payload (k_huffr_count) */
int tz_huffr_counts(tz_ctx* ctx, unsigned long long* counts, int* A, int* base);
int tz_huffr_counts_buf(tz_ctx* ctx, const int16_t* in, size_t n, unsigned long long* counts, int* A, int* base);
int tz_huffr_encode(tz_ctx* ctx, const uint8_t* lengths, int A, int base, size_t* bytes);
int tz_huffr_get(tz_ctx* ctx, size_t offset, size_t count, uint8_t* out);
int tz_huffr_begin(tz_ctx* ctx, size_t bytes, size_t n, const uint8_t* lengths, int A, int base, int R);
int tz_huffr_put(tz_ctx* ctx, size_t offset, size_t count, const uint8_t* src);
int tz_huffr_decode(tz_ctx* ctx);
int tz_huffr_encode_buf(tz_ctx* ctx, const int16_t* in, size_t n, const uint8_t* lengths, int A, int base, uint8_t* out,
                        size_t capacity, size_t* bytes);
int tz_huffr_decode_buf(tz_ctx* ctx, const uint8_t* stream, size_t bytes, size_t n, const uint8_t* lengths, int A, int base,
                        int R, int16_t* out);

/* ---- opt-in Huffman coder that picks its match distance (`tezip.py -c --coder huffd`, format TZR2 in DESIGN.md section 9,
 * slow statement of it in tezip_amd/huffd.py) ----------------------------------------------------------------------------
 * One coder over the two above: a file names its match distance D.  D = 0: no repeat tokens, the stream is tz_huff_*'s for
 * the same literal lengths.  D = 1 or 3: tz_huffr_*'s tokeniser with "three" replaced by D (element j of a run matches when
 * j >= D and equals element j - D; the history in front of a run is D elements equal to base); for D = 3 the stream is
 * tz_huffr_*'s byte for byte.  `lengths` holds A + 8 bytes for every D, and with D = 0 the eight token lengths must be 0.
 * tz_huffd_counts fills THREE histograms from one read of the payload (k_huffd_count): `counts` holds 3 rows of TZ_NBINS + 8
 * entries, row 0 for D = 0, row 1 for D = 1, row 2 for D = 3, each the A literals, then T_0..T_7 (all 0 in row 0), then
 * zeros; the host chooses D from them (tezip_amd/huffd.py: choose).  TZ_ERR_INVALID for a D outside {0, 1, 3}; every other
 * refusal and clamp is tz_huffr_*'s.  The resident stream buffer is the one tz_huff_* / tz_huffr_* use: a tz_huffd_begin
 * replaces what they staged and the other way round, and each decoder refuses the others' streams with TZ_ERR_STATE. */
int tz_huffd_counts(tz_ctx* ctx, unsigned long long* counts /* [3][TZ_NBINS + 8] */, int* A, int* base);
int tz_huffd_counts_buf(tz_ctx* ctx, const int16_t* in, size_t n, unsigned long long* counts, int* A, int* base);
int tz_huffd_encode(tz_ctx* ctx, const uint8_t* lengths, int A, int base, int D, size_t* bytes);
int tz_huffd_get(tz_ctx* ctx, size_t offset, size_t count, uint8_t* out);
int tz_huffd_begin(tz_ctx* ctx, size_t bytes, size_t n, const uint8_t* lengths, int A, int base, int R, int D);
int tz_huffd_put(tz_ctx* ctx, size_t offset, size_t count, const uint8_t* src);
int tz_huffd_decode(tz_ctx* ctx);
int tz_huffd_encode_buf(tz_ctx* ctx, const int16_t* in, size_t n, const uint8_t* lengths, int A, int base, int D, uint8_t* out,
                        size_t capacity, size_t* bytes);
int tz_huffd_decode_buf(tz_ctx* ctx, const uint8_t* stream, size_t bytes, size_t n, const uint8_t* lengths, int A, int base,
                        int R, int D, int16_t* out);

/* ---- the bound for a compression-ratio target (no reference counterpart; `tezip.py -c --target-ratio R --coder huff|huffr|huffd`;
 * definition TZ-TRATIO-1 in DESIGN.md section 9 and tezip_amd/ratetarget.py) ------------------------------------------------------
 * With a GPU coder the size of entropy.dat is an exact function of integer counts.  tz_size_probe: one candidate bound.  On
 * the context's ENCODER rollout (state rules, the refusal of a stack with colour under tz_set_payload_channels(ctx, 1) and
 * the errors of a bound are tz_encode's) *out describes the stream that tz_encode(ctx, mode, b0, b1, entropy, NULL, ...),
 * tz_<coder>_counts, the host's choice of the code (tz_huff_lengths / tz_huffr_lengths, tezip_amd/huffd.py: choose) and
 * tz_<coder>_encode would leave, in the payload layout in force (flat, tz_set_payload_channels(ctx, 1),
 * tz_set_delta_stride(ctx, 1)); a candidate that chain refuses (values that span more than TZ_NBINS symbols, a stream of 2^32
 * words) is refused here with the same status and message.  A probe forms the delta stack, quantises it and reads the result
 * twice: k_size_count forms every payload symbol on the fly, in front of the rank remap, and fills the plain histogram and the
 * token histograms at match distance 1 and 3; the host builds the table, permutes the counts by it and derives the code;
 * k_size_bits sums the bits per run of 256 and chunk of 64 runs under that code, rounds every chunk up to 32-bit words and
 * returns their total.  No payload, remapped copy, index or bit stream is made, and nothing of the context changes: a
 * resident payload, its kind, a resident stream, predictions, frames and rollout state are as they were.
 *  entropy: 0 or 1 as tz_encode's (byte planes, bit 1, are TZ_ERR_INVALID); coder: 0 = huff, 1 = huffr, 2 = huffd.
 *  out: host. */
typedef struct {
    unsigned long long n;             /* payload elements */
    unsigned long long stream_words;  /* 32-bit words of the bit stream */
    unsigned long long bytes;         /* index | bits: what tz_<coder>_encode reports in *bytes */
    unsigned long long cost_bits[3];  /* stream bits in front of the chunks' padding at match distance 0 | 1 | 3 (huffd: the three
                                         totals of its choice; huff: [0] alone, huffr: [2] alone, the others 0) */
    int A, base;                      /* the literals of the code, as tz_<coder>_counts reports them */
    int dist;                         /* the match distance of the stream: 0 (huff), 3 (huffr), huffd's choice */
    int table_len;                    /* length of the rank table, -1 without one (entropy == 0) */
} tz_size_record;                     /* 64 bytes */
int tz_size_probe(tz_ctx* ctx, int mode, double b0, double b1, int entropy, int coder, tz_size_record* out);
/* The two kernels alone, over any int16 stack q of nq elements (host or device, 2-byte aligned) read as the quantised deltas of
 * the layout (channels, stride): (3, 1) flat, (3, 3) the channel stride, (1, 1) one channel -- q then holds whole pixels (nq % 3
 * == 0) and yields nq / 3 symbols.  Symbol i is the spatial delta of the layout (the first `stride` symbols: the element
 * itself), then 1600 - it when apply_offset.  Bins: TZ_SIZE_BINS literal bins (bin = symbol + TZ_SIZE_BIAS), then T_0..T_7.
 * tz_size_count_buf: counts (host) receives 3 rows of TZ_SIZE_BINS + 8 entries, match distance 0 | 1 | 3 as tz_huffd_counts';
 * *bad: a symbol outside the bins.  tz_size_bits_buf: lens (host) holds TZ_SIZE_BINS + 8 code lengths by bin; *bits the sum
 * of the stream's bits at the match distance dist (0, 1 or 3), *words the sum over the chunks of ceil(bits / 32), *bad: a
 * symbol or token of length 0. */
#define TZ_SIZE_BINS 4096
#define TZ_SIZE_BIAS 1024
int tz_size_count_buf(tz_ctx* ctx, const int16_t* q, size_t nq, int channels, int stride, int apply_offset,
                      unsigned long long* counts /* [3][TZ_SIZE_BINS + 8] */, int* bad);
int tz_size_bits_buf(tz_ctx* ctx, const int16_t* q, size_t nq, int channels, int stride, int apply_offset, const uint8_t* lens,
                     int dist, unsigned long long* words, unsigned long long* bits, int* bad);

/* ---- the payload's spatial delta by exact size (no reference counterpart; `tezip.py -c --sdelta auto --coder huff|huffr|huffd`;
 * definition TZ-SDA1 in DESIGN.md section 9 and tezip_amd/sdauto.py) ---------------------------------------------------------------
 * TZ-SDA1.  Candidates in the order flat, channel, plane (TZ-SD2); on a one-channel payload channel IS flat and is no
 * candidate.  E(layout) = the bytes of the entropy.dat whose stream is the tz_size_record of the stream that the job's own
 * tz_encode -> tz_<coder>_counts -> host code choice -> tz_<coder>_encode would write under that layout, whole files (the
 * front differs per layout: A, table_len).  The choice is the smallest E, a tie goes to the earlier candidate, and the job
 * runs as `--sdelta <chosen>`: every file is byte for byte that job's.
 * tz_sdelta_probe: tz_size_probe's state rules, refusals and arguments, but out receives THREE records, out[0] flat (channel 0
 * alone under tz_set_payload_channels(ctx, 1)), out[1] the channel stride, out[2] the plane; out[i].n == 0 marks a layout that
 * is no candidate.  The delta stack is formed and quantised ONCE (the quantised deltas do not depend on the layout), then
 * k_size_count and k_size_bits read it once per candidate.  It honours tz_set_payload_channels (with the colour refusal),
 * tz_set_quantiser and tz_set_frame_bounds; it does NOT read tz_set_delta_stride / tz_set_delta_plane, and leaves them, a
 * resident payload and everything else of the context as they were.  (tz_size_probe itself keeps refusing
 * tz_set_delta_plane(ctx, 1) with TZ_ERR_UNSUPPORTED.) */
int tz_sdelta_probe(tz_ctx* ctx, int mode, double b0, double b1, int entropy, int coder, tz_size_record out[3]);
/* The two kernels alone over the plane symbols: q (host or device, 2-byte aligned) holds nframes x H x W x 3 quantised deltas
 * in [-255, 255]; channels 3: every element yields a symbol, 1: channel 0 of every pixel does.  Symbol i <-> (f, y, x, c) is
 * wrap9(q[y, x-1] + q[y-1, x] - q[y-1, x-1] - q[y, x]), neighbours outside the frame 0, then 1600 - it when apply_offset
 * (tezip_amd/sdelta.py: encode_plane).  Otherwise the twins of tz_size_count_buf / tz_size_bits_buf. */
int tz_size_count_plane_buf(tz_ctx* ctx, const int16_t* q, int nframes, int H, int W, int channels, int apply_offset,
                            unsigned long long* counts /* [3][TZ_SIZE_BINS + 8] */, int* bad);
int tz_size_bits_plane_buf(tz_ctx* ctx, const int16_t* q, int nframes, int H, int W, int channels, int apply_offset, const uint8_t* lens,
                           int dist, unsigned long long* words, unsigned long long* bits, int* bad);

/* ---- opt-in key-frame coder (`tezip.py -c --key-coder huff`, format TZK1 in DESIGN.md section 9, slow statement of it in
 * tezip_amd/keycoder.py; no reference counterpart: compress.py:271-278 hands a zero-except-keys stack to zstd) -----------------
 * Only the key frames are stored: each as the residuals mod 256 of one of four predictors over its own samples (0: none,
 * 1: left neighbour, 2: upper neighbour, 3: left + up - upleft; same channel, 0 outside the frame), all of them under one
 * canonical Huffman code of 256 symbols (`lengths`, as tz_huff_*; index | bits as there).  idx: nkeys >= 1 frame indices,
 * strictly ascending inside the stack; pred: nkeys predictor ids 0..3.  TZ_ERR_INVALID for anything else, for a bad code and
 * for a stream size that cannot hold nkeys * H * W * 3 symbols.  The coder keeps a stream and a symbol buffer of its own:
 * what tz_huff_* / tz_huffr_* hold or have staged is left as it is.
 * Encoder, on the frame stack resident after tz_frames_put or tz_rollout (TZ_ERR_STATE without one):
 * tz_keys_counts: counts[nkeys][4][256] (host) of the residual values of every key frame under every predictor, from one
 * read of the key frames (k_key_hist); the caller chooses the predictors and the code from them. */
int tz_keys_counts(tz_ctx* ctx, const int* idx, int nkeys, unsigned* counts);
/* Codes the key frames into a context-resident stream; *bytes receives its size, tz_keys_get fetches it in pieces. */
int tz_keys_encode(tz_ctx* ctx, const int* idx, int nkeys, const uint8_t* pred, const uint8_t* lengths, size_t* bytes);
int tz_keys_get(tz_ctx* ctx, size_t offset, size_t count, uint8_t* out);
/* Decoder: begin, then put for any partition of [0, bytes) on the copy stream, then tz_keys_decode, which leaves the context's
 * frame stack exactly as tz_frames_begin(nt, H, W) and tz_frames_put of the whole zero-except-keys stack leave it (the other
 * frames are zeroed): tz_frames_get, tz_rollout_decode(NULL, ...) and tz_rollout_decode_range(NULL, ...) run unchanged.
 * TZ_ERR_STATE when tz_keys_decode runs before every byte was put.  The caller validates the index
 * (tezip_amd/keycoder.py: parse); the kernels clamp as tz_huff_decode's do. */
int tz_keys_begin(tz_ctx* ctx, size_t bytes, int nt, int H, int W, const int* idx, int nkeys, const uint8_t* pred,
                  const uint8_t* lengths);
int tz_keys_put(tz_ctx* ctx, size_t offset, size_t count, const uint8_t* src);
int tz_keys_decode(tz_ctx* ctx);
/* Stand-alone forms on host or device arrays: frames (k, H, W, 3) <-> k * H * W * 3 int16 symbols 0..255, pred[k] per frame. */
int tz_keys_residual_buf(tz_ctx* ctx, const uint8_t* frames, int k, int H, int W, const uint8_t* pred, int16_t* sym);
int tz_keys_unresidual_buf(tz_ctx* ctx, const int16_t* sym, int k, int H, int W, const uint8_t* pred, uint8_t* frames);

/* ---- the same with gray key frames stored once (`--key-coder huffg`, format TZK2 in DESIGN.md section 9, slow statement of it
 * in tezip_amd/keycoderg.py) ---------------------------------------------------------------------------------------------------
 * A key frame whose three channels are equal at every pixel is GRAY: it contributes the H * W residuals of channel 0, and the
 * decoder writes each sample to all three channels.  predg: nkeys pred bytes, bits 0-1 the predictor id, bit 2 (value 4) GRAY;
 * TZ_ERR_INVALID above 7.  The symbols of frame k start at the sum of the counts of the frames before it.  The tz_keysg_*
 * calls share the buffers of tz_keys_*; a stream staged by tz_keysg_begin is refused by tz_keys_put / tz_keys_decode and the
 * other way round (TZ_ERR_INVALID / TZ_ERR_STATE), and each begin discards what the other had staged.
 * tz_keys_gray: gray[k] = 1 iff frame idx[k] of the resident stack is GRAY (k_key_gray, one read of the key frames). */
int tz_keys_gray(tz_ctx* ctx, const int* idx, int nkeys, uint8_t* gray);
int tz_keysg_encode(tz_ctx* ctx, const int* idx, int nkeys, const uint8_t* predg, const uint8_t* lengths, size_t* bytes);
int tz_keysg_get(tz_ctx* ctx, size_t offset, size_t count, uint8_t* out);
int tz_keysg_begin(tz_ctx* ctx, size_t bytes, int nt, int H, int W, const int* idx, int nkeys, const uint8_t* predg,
                   const uint8_t* lengths);
int tz_keysg_put(tz_ctx* ctx, size_t offset, size_t count, const uint8_t* src);
int tz_keysg_decode(tz_ctx* ctx);
/* Stand-alone forms: frames (k, H, W, 3) <-> the sum over k of H * W (GRAY) or H * W * 3 int16 symbols.  The GRAY bit is taken
 * as given: tz_keysg_residual_buf codes channel 0 of such a frame whatever the other channels hold. */
int tz_keysg_residual_buf(tz_ctx* ctx, const uint8_t* frames, int k, int H, int W, const uint8_t* predg, int16_t* sym);
int tz_keysg_unresidual_buf(tz_ctx* ctx, const int16_t* sym, int k, int H, int W, const uint8_t* predg, uint8_t* frames);

/* ---- timing helper: HIP events on the context's stream (bench.py) -------------------------- */
int tz_timer_start(tz_ctx* ctx);
int tz_timer_stop(tz_ctx* ctx, float* ms);
/* Per-kernel-class accumulated device time since the last reset, measured with HIP events
 * around every launch of that class when profiling is enabled (adds a sync per query only).
 * names: tz_prof_name(i), i < tz_prof_count(). */
int tz_prof_enable(tz_ctx* ctx, int on);
int tz_prof_count(void);
const char* tz_prof_name(int i);
int tz_prof_get(tz_ctx* ctx, int i, double* total_ms, long long* launches);
int tz_prof_reset(tz_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
