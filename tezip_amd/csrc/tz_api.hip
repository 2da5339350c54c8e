// Context, staging helpers, rollout state machine and the encode/decode drivers of
// libtezip_hip.so.  Reference control flow: /root/reference/src/compress.py:183-373 and
// /root/reference/src/decompress.py:105-256 (cited per function).
#include <dlfcn.h>
#include <stdarg.h>

#include <algorithm>
#include <chrono>
#include <thread>

#include "tz_internal.h"

// ------------------------------------------------------------------------------ errors
int tz_fail(tz_ctx* ctx, int status, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->last_error = buf;
    return status;
}

// Kernels whose waits are hand-built (k_scan2p polls status words of other workgroups) bound those waits and report an
// expiry here instead of hanging the GPU: one pinned host word the device can write.
int tz_fault_word(tz_ctx* ctx) {
    if (ctx->h_fault) return TZ_OK;
    void* h = nullptr;
    TZ_HIP(ctx, hipHostMalloc(&h, sizeof(unsigned), hipHostMallocMapped));
    *(volatile unsigned*)h = 0;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipHostFree(h);
        return tz_fail(ctx, TZ_ERR_HIP, "no device pointer for the fault word");
    }
    ctx->h_fault = (volatile unsigned*)h;
    ctx->d_fault = (unsigned*)d;
    return TZ_OK;
}

int tz_stream_sync(tz_ctx* ctx) {
    TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->h_fault && *ctx->h_fault) {
        const unsigned f = *ctx->h_fault;
        *ctx->h_fault = 0;
        if (f & TZ_FAULT_SCAN_POLL)
            return tz_fail(ctx, TZ_ERR_HIP,
                           "inverse scan (k_scan2p): a workgroup gave up waiting for the block sum of a workgroup in front of it "
                           "(workgroups not dispatched in index order?); the scanned output of that launch is invalid");
        return tz_fail(ctx, TZ_ERR_HIP, "a kernel reported fault 0x%x", f);
    }
    return TZ_OK;
}

// diagnostic: makes the next inverse scans poll for the epoch `epoch_skew` launches ahead (never published when != 0) and
// give up after `poll_limit` polls (0 = the built-in 2^22); (0, 0) restores normal operation.  tests/test_gpu_parity.py
// uses it to see the bounded wait fail loudly.
extern "C" int tz_scan_fault_inject(tz_ctx* ctx, unsigned epoch_skew, unsigned poll_limit) {
    if (!ctx) return TZ_ERR_INVALID;
    ctx->scan_dbg_skew = epoch_skew & 0xFFFFu;
    ctx->scan_dbg_limit = poll_limit;
    return TZ_OK;
}

extern "C" int tz_version(void) { return 101; }

// What this library was compiled with: "tezip_hip <version> gfx950" and, after "defines:", every diagnostic switch of
// csrc/ that was on (TZW_ABL produces WRONG results by design; TZW_STAMPS / TZW_LEAD / TZW_ISSUE_AT / TZW_PK change the
// kernels that are measured).  A library whose string names any of them is a measurement build: bench.py and the test
// suite refuse it (tezip_amd/_lib.py diagnostic_defines).
extern "C" const char* tz_build_info(void) {
    return "tezip_hip 101 gfx950 defines:"
#ifdef TZW_ABL
           " TZW_ABL"
#endif
#ifdef TZW_STAMPS
           " TZW_STAMPS"
#endif
#ifdef TZW_LEAD
           " TZW_LEAD"
#endif
#ifdef TZW_ISSUE_AT
           " TZW_ISSUE_AT"
#endif
#ifdef TZW_PK
           " TZW_PK"
#endif
        ;
}

int tz_check_pred_contract(tz_ctx* ctx, const char* who) {
    const int now = tz_get_contract(ctx);
    if (ctx->pred_contract && now != ctx->pred_contract)
        return tz_fail(ctx, TZ_ERR_STATE,
                       "%s: the resident predictions were made under TZ-PA%d, the contract in force is now TZ-PA%d "
                       "(tz_set_contract between the rollout and its encode/decode): roll out again",
                       who, ctx->pred_contract, now);
    return TZ_OK;
}

extern "C" int tz_rollout_contract(tz_ctx* ctx) {
    if (!ctx) return TZ_ERR_INVALID;
    if (ctx->rollout_kind == tz_ctx::ROLLOUT_NONE) return tz_fail(ctx, TZ_ERR_STATE, "no rollout in this context");
    return ctx->pred_contract;
}

extern "C" const char* tz_strerror(int s) {
    switch (s) {
        case TZ_OK: return "ok";
        case TZ_ERR_INVALID: return "invalid argument";
        case TZ_ERR_NO_DEVICE: return "no HIP device";
        case TZ_ERR_HIP: return "HIP runtime error";
        case TZ_ERR_STATE: return "call order / missing state";
        case TZ_ERR_NOMEM: return "out of device memory";
        case TZ_ERR_UNSUPPORTED: return "unsupported model shape";
    }
    return "unknown status";
}

extern "C" const char* tz_last_error(const tz_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

// ----------------------------------------------------------------------------- context
extern "C" int tz_ctx_create(int device, void* hip_stream, tz_ctx** out) {
    if (!out) return TZ_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TZ_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return TZ_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return TZ_ERR_NO_DEVICE;
    tz_ctx* ctx = new tz_ctx();
    {
        const char* e = getenv("TEZIP_CONV16");  // diagnostic default of tz_set_conv_impl
        if (e && e[0] == '0') ctx->conv_impl = 0;
        e = getenv("TEZIP_LAT");                 // k_convlat: 0 never, 1 cost model (default), 2 wherever eligible
        if (e) ctx->lat_mode = atoi(e);
        e = getenv("TEZIP_PA");                  // arithmetic contract a context starts with (tz_set_contract): 0 (default), 1 or 2
        if (e && e[0] >= '0' && e[0] <= '2' && !e[1]) ctx->contract = e[0] - '0';
        e = getenv("TEZIP_WINO_IPW");            // measurements: column blocks per k_wino workgroup (0 = per launch)
        if (e) ctx->wino_ipw = atoi(e);
        e = getenv("TEZIP_QUALITY_GRID");        // diagnostic: workgroups of k_quality (0 = per launch; tests of launch-shape invariance)
        if (e) ctx->quality_grid = atoi(e);
        e = getenv("TEZIP_DIGEST_GRID");         // diagnostic: workgroups of k_digest (0 = per launch; tests of launch-shape invariance)
        if (e) ctx->digest_grid = atoi(e);
        e = getenv("TEZIP_SSIM_GRID");           // diagnostic: workgroups of k_ssim (0 = per launch; tests of launch-shape invariance)
        if (e) ctx->ssim_grid = atoi(e);
    }
    ctx->device = device;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ctx->num_cus = prop.multiProcessorCount;
    }
    if (hip_stream) {
        ctx->stream = (hipStream_t)hip_stream;
        // a caller's stream: the split gate launches of "E-part ahead" only pay when the compute stream outranks stream2
        // (measured: at equal priority the side workgroups sit on the CUs the critical path wants, +5 % per step)
        int prio = 0, prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        if (hipStreamGetPriority(ctx->stream, &prio) != hipSuccess || prio != prio_greatest || prio_greatest == prio_least) {
            (void)hipGetLastError();
            if (ctx->epart_mode < 0) ctx->epart_mode = 0;
        }
    } else {
        // (highest dispatch priority: the side launches on stream2 -- lowest -- are there to fill what this stream leaves idle)
        int prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        if (hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, prio_greatest) != hipSuccess) {
            delete ctx;
            return TZ_ERR_HIP;
        }
        ctx->own_stream = true;
        if (prio_greatest == prio_least && ctx->epart_mode < 0) ctx->epart_mode = 0;   // no priorities on this device: no side launches by default
    }
    (void)hipEventCreate(&ctx->ev0);
    (void)hipEventCreate(&ctx->ev1);
    if (hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->down_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_keys, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_frames, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_compute, hipEventDisableTiming) != hipSuccess) {
        tz_ctx_destroy(ctx);
        return TZ_ERR_HIP;
    }
    {
        const char* e = getenv("TEZIP_SPLIT");
        if (e) ctx->split_rollout = atoi(e);
        e = getenv("TEZIP_DECODE_UNFUSED");
        if (e) ctx->decode_unfused = atoi(e);
        e = getenv("TEZIP_EPART");
        if (e) ctx->epart_mode = atoi(e);
        // stream2 takes work that must not delay the compute stream's (the side launches of "E-part ahead" fill the CUs the
        // critical path leaves idle): lowest dispatch priority the device offers
        int prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        if (hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, prio_least) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
            tz_ctx_destroy(ctx);
            return TZ_ERR_HIP;
        }
    }
    ctx->ring_size = 1 << 20;
    if (hipHostMalloc((void**)&ctx->ring, ctx->ring_size, hipHostMallocDefault) != hipSuccess) {
        ctx->ring = nullptr;
        ctx->ring_size = 0;
    }
    *out = ctx;
    return TZ_OK;
}

extern "C" int tz_ctx_destroy(tz_ctx* ctx) {
    if (!ctx) return TZ_OK;
    (void)hipSetDevice(ctx->device);
    (void)tz_payload_settle(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    tz_model_free(ctx);
    tz_pool_release_all(ctx);
    for (auto& p : ctx->pool) (void)hipFree(p.first);
    if (ctx->d_frames) (void)hipFree(ctx->d_frames);
    if (ctx->d_pred) (void)hipFree(ctx->d_pred);
    if (ctx->d_sched) (void)hipFree(ctx->d_sched);
    if (ctx->d_payload) (void)hipFree(ctx->d_payload);
    if (ctx->d_bound_map) (void)hipFree(ctx->d_bound_map);
    if (ctx->d_payload_stage) (void)hipFree(ctx->d_payload_stage);
    if (ctx->ev_payload) (void)hipEventDestroy(ctx->ev_payload);
    if (ctx->d_out) (void)hipFree(ctx->d_out);
    if (ctx->d_huff) (void)hipFree(ctx->d_huff);
    if (ctx->d_keys) (void)hipFree(ctx->d_keys);
    if (ctx->d_keysym) (void)hipFree(ctx->d_keysym);
    if (ctx->d_scan_status) (void)hipFree(ctx->d_scan_status);
    if (ctx->d_scan3_status) (void)hipFree(ctx->d_scan3_status);
    if (ctx->h_fault) (void)hipHostFree((void*)ctx->h_fault);
    for (auto& s : ctx->prof)
        for (auto& e : s.pending) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    if (ctx->ring) (void)hipHostFree(ctx->ring);
    if (ctx->copy_stream) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamDestroy(ctx->copy_stream);
    }
    if (ctx->down_stream) {
        (void)hipStreamSynchronize(ctx->down_stream);
        (void)hipStreamDestroy(ctx->down_stream);
    }
    for (int i = 0; i < tz_ctx::kStages; ++i) {
        if (ctx->stage[i]) (void)hipHostFree(ctx->stage[i]);
        if (ctx->stage_ev[i]) (void)hipEventDestroy(ctx->stage_ev[i]);
    }
    for (auto e : ctx->chunk_ev) (void)hipEventDestroy(e);
    if (ctx->stream2) {
        (void)hipStreamSynchronize(ctx->stream2);
        (void)hipStreamDestroy(ctx->stream2);
    }
    for (int l = 0; l < TZ_MAX_LEVELS; ++l) {
        if (ctx->ev_epart_src[l]) (void)hipEventDestroy(ctx->ev_epart_src[l]);
        if (ctx->ev_epart_done[l]) (void)hipEventDestroy(ctx->ev_epart_done[l]);
        if (l < 2 && ctx->ev_cal[l]) (void)hipEventDestroy(ctx->ev_cal[l]);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->ev_keys) (void)hipEventDestroy(ctx->ev_keys);
    if (ctx->ev_frames) (void)hipEventDestroy(ctx->ev_frames);
    if (ctx->ev_compute) (void)hipEventDestroy(ctx->ev_compute);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return TZ_OK;
}

extern "C" int tz_ctx_synchronize(tz_ctx* ctx) {
    if (!ctx) return TZ_ERR_INVALID;
    TZ_TRY(tz_payload_settle(ctx));
    return tz_stream_sync(ctx);
}

int tz_payload_settle(tz_ctx* ctx) {
    if (!ctx->payload_inflight) return TZ_OK;
    ctx->payload_inflight = false;
    TZ_HIP(ctx, hipEventSynchronize(ctx->ev_payload));
    return TZ_OK;
}

extern "C" int tz_set_payload_deferred(tz_ctx* ctx, int on) {
    if (!ctx) return TZ_ERR_INVALID;
    if (!on) TZ_TRY(tz_payload_settle(ctx));
    ctx->defer_payload = on ? 1 : 0;
    return TZ_OK;
}

extern "C" int tz_payload_wait(tz_ctx* ctx) {
    if (!ctx) return TZ_ERR_INVALID;
    return tz_payload_settle(ctx);
}

extern "C" void* tz_ctx_stream(tz_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

// ---------------------------------------------------------------------- memory helpers
int tz_ptr_kind(const void* p) {
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // unregistered host memory: clear the sticky error
        return 0;
    }
    if (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged) return 2;
    return attr.type == hipMemoryTypeHost ? 1 : 0;
}

bool tz_is_device_ptr(const void* p) { return tz_ptr_kind(p) == 2; }

extern "C" int tz_host_alloc(size_t bytes, void** out) {
    if (!out) return TZ_ERR_INVALID;
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return e == hipErrorNoDevice || e == hipErrorInvalidDevice ? TZ_ERR_NO_DEVICE : TZ_ERR_NOMEM;
    }
    return TZ_OK;
}

extern "C" int tz_host_free(void* p) {
    if (!p) return TZ_OK;
    return hipHostFree(p) == hipSuccess ? TZ_OK : TZ_ERR_HIP;
}

// one pinned staging buffer, free to be overwritten (its previous DMA has completed)
static int stage_acquire(tz_ctx* ctx, int* idx) {
    const int i = ctx->stage_next;
    ctx->stage_next = (i + 1) % tz_ctx::kStages;
    if (!ctx->stage[i] || !ctx->stage_ev[i]) {
        hipError_t e = hipSuccess;
        if (!ctx->stage[i]) e = hipHostMalloc((void**)&ctx->stage[i], tz_ctx::kStageBytes, hipHostMallocDefault);
        if (e == hipSuccess && !ctx->stage_ev[i]) e = hipEventCreateWithFlags(&ctx->stage_ev[i], hipEventDisableTiming);
        if (e != hipSuccess) {   // a buffer without its event is no use: the next call starts over
            if (ctx->stage[i]) (void)hipHostFree(ctx->stage[i]);
            ctx->stage[i] = nullptr;
            ctx->stage_ev[i] = nullptr;
            (void)hipGetLastError();
            return tz_fail(ctx, TZ_ERR_NOMEM, "pinned staging buffer: %s", hipGetErrorString(e));
        }
    }
    if (ctx->stage_busy[i]) {
        TZ_HIP(ctx, hipEventSynchronize(ctx->stage_ev[i]));
        ctx->stage_busy[i] = false;
    }
    *idx = i;
    return TZ_OK;
}

// memcpy between pageable memory and a pinned staging buffer on a few threads: one core moves
// ~8-10 GB/s, a PCIe 5 x16 link four to five times that
static void copy_mt(void* dst, const void* src, size_t n) {
    constexpr size_t kMin = (size_t)2 << 20;
    constexpr int kThreads = 4;
    if (n < 2 * kMin) {
        memcpy(dst, src, n);
        return;
    }
    const size_t per = ((n + kThreads - 1) / kThreads + 4095) & ~(size_t)4095;
    std::thread th[kThreads - 1];
    int started = 0;
    for (int i = 1; i < kThreads; ++i) {
        const size_t off = per * i;
        if (off >= n) break;
        th[started++] = std::thread([=] { memcpy((uint8_t*)dst + off, (const uint8_t*)src + off, std::min(per, n - off)); });
    }
    memcpy(dst, src, std::min(per, n));
    for (int i = 0; i < started; ++i) th[i].join();
}

int tz_h2d(tz_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return TZ_OK;
    if (tz_ptr_kind(src) != 0) {
        TZ_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, s));
        return TZ_OK;
    }
    // pageable: memcpy of chunk k+1 into a pinned buffer overlaps the DMA of chunk k
    for (size_t off = 0; off < bytes; off += tz_ctx::kStageBytes) {
        const size_t n = std::min(tz_ctx::kStageBytes, bytes - off);
        int i;
        TZ_TRY(stage_acquire(ctx, &i));
        copy_mt(ctx->stage[i], (const uint8_t*)src + off, n);
        TZ_HIP(ctx, hipMemcpyAsync((uint8_t*)dst + off, ctx->stage[i], n, hipMemcpyHostToDevice, s));
        TZ_HIP(ctx, hipEventRecord(ctx->stage_ev[i], s));
        ctx->stage_busy[i] = true;
    }
    return TZ_OK;
}

int tz_d2h(tz_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return TZ_OK;
    if (tz_ptr_kind(dst) != 0) {
        TZ_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, s));
        return TZ_OK;
    }
    // pageable: the DMA of chunk k+1 into a pinned buffer overlaps the memcpy of chunk k out of one
    int prev = -1;
    size_t prev_off = 0, prev_n = 0;
    for (size_t off = 0; off < bytes; off += tz_ctx::kStageBytes) {
        const size_t n = std::min(tz_ctx::kStageBytes, bytes - off);
        int i;
        TZ_TRY(stage_acquire(ctx, &i));
        TZ_HIP(ctx, hipMemcpyAsync(ctx->stage[i], (const uint8_t*)src + off, n, hipMemcpyDeviceToHost, s));
        TZ_HIP(ctx, hipEventRecord(ctx->stage_ev[i], s));
        ctx->stage_busy[i] = true;
        if (prev >= 0) {
            TZ_HIP(ctx, hipEventSynchronize(ctx->stage_ev[prev]));
            ctx->stage_busy[prev] = false;
            copy_mt((uint8_t*)dst + prev_off, ctx->stage[prev], prev_n);
        }
        prev = i;
        prev_off = off;
        prev_n = n;
    }
    if (prev >= 0) {
        TZ_HIP(ctx, hipEventSynchronize(ctx->stage_ev[prev]));
        ctx->stage_busy[prev] = false;
        copy_mt((uint8_t*)dst + prev_off, ctx->stage[prev], prev_n);
    }
    return TZ_OK;
}

static constexpr size_t kPoolUsed = (size_t)1 << 63;  // top bit of the size marks "handed out"

// TEZIP_POISON=<byte> (diagnostic): every device buffer handed out -- fresh or recycled -- is first filled with that byte,
// so that a kernel reading something nobody wrote shows up as a parity failure instead of depending on what the memory
// held before (tests/test_gpu_poison.py runs the parity cases this way).
int tz_poison_byte() {
    static const int v = [] {
        const char* e = getenv("TEZIP_POISON");
        return e && *e ? (atoi(e) & 0xff) | 0x100 : 0;
    }();
    return v;
}
int tz_poison(tz_ctx* ctx, void* p, size_t bytes) {
    const int v = tz_poison_byte();
    if (v && p && bytes) {   // finished before the caller goes on: some initialisations are synchronous copies
        TZ_HIP(ctx, hipMemsetAsync(p, v & 0xff, bytes, ctx->stream));
        TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return TZ_OK;
}

int tz_pool_alloc(tz_ctx* ctx, size_t bytes, void** out) {
    if (bytes == 0) bytes = 16;
    bytes = (bytes + 255) & ~(size_t)255;
    int best = -1;
    for (int i = 0; i < (int)ctx->pool.size(); ++i) {
        size_t sz = ctx->pool[i].second;
        if ((sz & kPoolUsed) || sz < bytes) continue;
        if (best < 0 || sz < ctx->pool[best].second) best = i;
    }
    if (best >= 0 && ctx->pool[best].second <= 2 * bytes + (1 << 20)) {
        ctx->pool[best].second |= kPoolUsed;
        *out = ctx->pool[best].first;
        return tz_poison(ctx, *out, ctx->pool[best].second & ~kPoolUsed);
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    ctx->pool.push_back({p, bytes | kPoolUsed});
    *out = p;
    return tz_poison(ctx, p, bytes);
}

void tz_pool_release_all(tz_ctx* ctx) {
    for (auto& e : ctx->pool) e.second &= ~kPoolUsed;
}

// diagnostic: blocks of the scratch pool that are handed out right now (0 between calls), *blocks (may be NULL): all of them
extern "C" int tz_pool_held(tz_ctx* ctx, int* blocks) {
    if (!ctx) return TZ_ERR_INVALID;
    int held = 0;
    for (auto& e : ctx->pool) held += (e.second & kPoolUsed) != 0;
    if (blocks) *blocks = (int)ctx->pool.size();
    return held;
}

int tz_ensure(tz_ctx* ctx, void** buf, size_t* cap, size_t bytes) {
    if (*cap >= bytes && *buf) return TZ_OK;
    if (*buf) {
        TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(*buf);
        *buf = nullptr;
        *cap = 0;
    }
    hipError_t e = hipMalloc(buf, bytes ? bytes : 16);
    if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    *cap = bytes;
    return tz_poison(ctx, *buf, bytes);
}

int tz_upload(tz_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return TZ_OK;
    size_t need = (bytes + 63) & ~(size_t)63;
    if (!ctx->ring || need > ctx->ring_size / 4) {  // large or no ring: the caller's block is free on return
        TZ_TRY(tz_h2d(ctx, dst, src, bytes, ctx->stream));
        if (tz_ptr_kind(src) != 0) TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return TZ_OK;
    }
    if (ctx->ring_pos + need > ctx->ring_size) {  // wrap: everything queued so far must have left the ring
        TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->ring_pos = 0;
    }
    uint8_t* slot = ctx->ring + ctx->ring_pos;
    ctx->ring_pos += need;
    memcpy(slot, src, bytes);
    TZ_HIP(ctx, hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
    return TZ_OK;
}

int tz_dev_in(tz_ctx* ctx, const void* p, size_t bytes, const void** dev) {
    if (bytes == 0 || tz_is_device_ptr(p)) {
        *dev = p;
        return TZ_OK;
    }
    void* d;
    TZ_TRY(tz_pool_alloc(ctx, bytes, &d));
    TZ_TRY(tz_h2d(ctx, d, p, bytes, ctx->stream));
    if (tz_ptr_kind(p) != 0) TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller's buffer is free again on return
    *dev = d;
    return TZ_OK;
}

int tz_dev_out(tz_ctx* ctx, void* p, size_t bytes, tz_out* o) {
    o->bytes = bytes;
    if (bytes == 0 || tz_is_device_ptr(p)) {
        o->host = nullptr;
        o->dev = p;
        return TZ_OK;
    }
    o->host = p;
    return tz_pool_alloc(ctx, bytes, &o->dev);
}

int tz_call::finish() {
    bool any = false;
    for (auto& o : outs)
        if (o.host && o.bytes && !o.done) {
            TZ_TRY(tz_d2h(ctx, o.host, o.dev, o.bytes, ctx->stream));
            any = true;
        }
    if (any) TZ_TRY(tz_stream_sync(ctx));
    return TZ_OK;
}

// --------------------------------------------------------------------------- profiling
static const char* kProfNames[TZP_COUNT] = {"conv3x3_mfma", "err0", "delta", "quant", "spatial_delta_hist",
                                            "lut_remap", "undelta_scan", "reconstruct", "sse",
                                            "conv16_lds_dma", "conv16b_level0", "conv_small_valu", "conv3x3_general",
                                            "convlat_small_grid", "wino_pa2", "table_create", "quant_serial_chains",
                                            "undelta_carry", "quality", "huffman", "digest"};

namespace {
struct RoctxApi {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    RoctxApi() {
        const char* e = getenv("TEZIP_ROCTX");
        if (!e || atoi(e) == 0) return;
        void* h = nullptr;
        for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
        if (h) {
            push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
            pop = (int (*)())dlsym(h, "roctxRangePop");
        }
        if (!push || !pop) {
            const char* why = dlerror();         // (once: a second call returns NULL)
            fprintf(stderr, "[tezip] TEZIP_ROCTX is set but no ROCTx library could be opened (%s): no ranges\n", why ? why : "symbols missing");
            push = nullptr;
            pop = nullptr;
            if (h) dlclose(h);
        }
    }
};
const RoctxApi& roctx_api() {
    static RoctxApi api;
    return api;
}
}  // namespace

bool tz_roctx_push(const char* name) {
    const RoctxApi& r = roctx_api();
    if (!r.push) return false;
    r.push(name);
    return true;
}
void tz_roctx_pop() {
    const RoctxApi& r = roctx_api();
    if (r.pop) r.pop();
}

tz_prof_scope::tz_prof_scope(tz_ctx* c, int k) : ctx(c), cls(k) {
    rx = tz_roctx_push(k >= 0 && k < TZP_COUNT ? kProfNames[k] : "tz_stage");
    if (!ctx->prof_on) return;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        a = b = nullptr;
        return;
    }
    (void)hipEventRecord(a, ctx->stream);
}
tz_prof_scope::~tz_prof_scope() {
    if (rx) tz_roctx_pop();
    if (!a || !b) return;
    (void)hipEventRecord(b, ctx->stream);
    ctx->prof[cls].pending.push_back({a, b});
    ctx->prof[cls].pending_sub.push_back(sub);
}

extern "C" int tz_prof_enable(tz_ctx* ctx, int on) {
    if (!ctx) return TZ_ERR_INVALID;
    ctx->prof_on = on != 0;
    return TZ_OK;
}
extern "C" int tz_prof_count(void) { return TZP_COUNT; }
extern "C" const char* tz_prof_name(int i) { return (i >= 0 && i < TZP_COUNT) ? kProfNames[i] : ""; }

static int prof_drain(tz_ctx* ctx) {
    TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (auto& s : ctx->prof) {
        for (size_t k = 0; k < s.pending.size(); ++k) {
            auto& e = s.pending[k];
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) {
                s.total_ms += ms;
                s.launches += 1;
                const int sub = s.pending_sub[k];
                if (sub >= 0 && sub < TZP_COUNT) {
                    ctx->prof[sub].total_ms += ms;
                    ctx->prof[sub].launches += 1;
                }
            }
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        s.pending.clear();
        s.pending_sub.clear();
    }
    return TZ_OK;
}

extern "C" int tz_prof_get(tz_ctx* ctx, int i, double* total_ms, long long* launches) {
    if (!ctx || i < 0 || i >= TZP_COUNT) return TZ_ERR_INVALID;
    TZ_TRY(prof_drain(ctx));
    if (total_ms) *total_ms = ctx->prof[i].total_ms;
    if (launches) *launches = ctx->prof[i].launches;
    return TZ_OK;
}

extern "C" int tz_prof_reset(tz_ctx* ctx) {
    if (!ctx) return TZ_ERR_INVALID;
    TZ_TRY(prof_drain(ctx));
    for (auto& s : ctx->prof) {
        s.total_ms = 0;
        s.launches = 0;
    }
    return TZ_OK;
}

extern "C" int tz_timer_start(tz_ctx* ctx) {
    if (!ctx) return TZ_ERR_INVALID;
    TZ_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    return TZ_OK;
}
extern "C" int tz_timer_stop(tz_ctx* ctx, float* ms) {
    if (!ctx || !ms) return TZ_ERR_INVALID;
    TZ_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    TZ_HIP(ctx, hipEventSynchronize(ctx->ev1));
    TZ_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return TZ_OK;
}

// ------------------------------------------------------------------------------ rollout
static int pad8(int v) { return (v + 7) / 8 * 8; }  // data_utils.py:103-107
// frames of a sequence: the trailer stores nt as int16 (compress.py:390-394)
constexpr int kMaxFrames = 32767;

static void set_rollout(tz_ctx* ctx, tz_ctx::tz_rollout_kind kind, int pred_first, int pred_end) {
    ctx->rollout_kind = kind;
    ctx->loop_closed = 0;   // (tz_rollout_closed stamps its loop behind this)
    ctx->loop_select = 0;
    ctx->loop_motion = 0;
    ctx->loop_frames = 0;   // (tz_rollout_closed_frames likewise)
    ctx->loop_map = 0;      // (tz_rollout_closed_map likewise)
    ctx->pred_modes.clear();
    ctx->pred_vectors.clear();
    ctx->pred_first = pred_first;
    ctx->pred_end = pred_end;
}

// the prediction stack is one of `kind` and holds every frame of the sequence
static bool whole_stack(const tz_ctx* ctx, tz_ctx::tz_rollout_kind kind) {
    return ctx->rollout_kind == kind && ctx->pred_first == 0 && ctx->pred_end == ctx->nt;
}

// decompress.py:123-129: is there a non-zero sample in frame f?  16 bytes per lane where the frame allows it.
// Key frames of a PINNED host stack, fetched by the compute stream itself (zero-copy reads over PCIe: page-locked host
// memory is device-addressable): the first predictor step then never waits for a DMA engine that may still be busy with
// the previous sequence's deferred payload (tz_set_payload_deferred) -- HIP hands streams to SDMA engines as it likes, and
// a host -> device copy queued behind a 126 MB device -> host transfer starts 2.3 ms late.
__global__ __launch_bounds__(256) void k_fetch_frames(const uint8_t* __restrict__ host, uint8_t* __restrict__ dev, const int* __restrict__ which,
                                                      size_t frame_bytes) {
    const size_t base = (size_t)which[blockIdx.y] * frame_bytes;
    const size_t n16 = frame_bytes / 16;
    const uint4* s = (const uint4*)(host + base);
    uint4* d = (uint4*)(dev + base);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
    if (blockIdx.x == 0 && threadIdx.x < (frame_bytes & 15)) dev[base + n16 * 16 + threadIdx.x] = host[base + n16 * 16 + threadIdx.x];
}

__global__ void k_any_nonzero(const uint8_t* __restrict__ frames, size_t frame_bytes, int* __restrict__ flags) {
    int f = blockIdx.y;
    const uint8_t* p = frames + (size_t)f * frame_bytes;
    int any = 0;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
    if ((((uintptr_t)p) & 15) == 0) {
        const uint4* q = (const uint4*)p;
        const size_t n16 = frame_bytes / 16;
        for (size_t i = tid; i < n16; i += nthr) {
            const uint4 v = q[i];
            any |= (v.x | v.y | v.z | v.w) != 0;
        }
        for (size_t i = n16 * 16 + tid; i < frame_bytes; i += nthr) any |= p[i] != 0;
    } else {
        for (size_t i = tid; i < frame_bytes; i += nthr) any |= p[i] != 0;
    }
    if (__any(any) && (threadIdx.x & 63) == 0) atomicOr(&flags[f], 1);
}

__global__ void k_bcast_frame(const float* __restrict__ src, size_t fe, const int* __restrict__ slots, int nslots,
                              float* __restrict__ stack) {
    int s = blockIdx.y;
    if (s >= nslots) return;
    float* dst = stack + (size_t)slots[s] * fe;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < fe; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

// Host frames travel on the copy stream: the frames in `first` (the key frames the rollout
// reads) go ahead and the compute stream waits for them only; rollout_finish_upload sends the rest
// once the predictor launches are queued, so that the bulk of the stack (needed by the delta stage
// only) crosses PCIe while the predictor runs.
// ---- DWP control on the device (compress.py:245-264)
struct DwpState {
    int key_idx;   // first predicted frame of the open window (the reference's key_idx)
    int pad;
    double run;    // squared-error sum of the open window
};

static constexpr int kDwpLds = 2048;  // partial sums staged per pass of k_dwp_decide (16 KB)

__global__ void k_dwp_init(DwpState* st, int p, int nt, int* idx_table, int stride, uint8_t* key) {
    st->key_idx = p + 1;
    st->run = 0.0;
    idx_table[0] = 1;              // idx == key_idx: the input of the first step is the real frame p
    idx_table[stride] = p;
    idx_table[2 * stride] = p + 1;
    if (p < nt) key[p] = 1;        // compress.py:219-220
}

// The DWP step's window SSE and its decision in ONE launch (round 5; until then k_sse, then a one-workgroup k_dwp_decide,
// then a conditional C0 broadcast: three dependent launches behind every predictor step of a B = 1 rollout).  Every
// workgroup writes its block's partial sum (the arithmetic of k_sse: tz_sse_block) and takes a ticket; the workgroup that
// draws the last ticket -- every partial was performed before its ticket, both as device-scope atomics, and is read back
// with atomics -- adds them in block order exactly as tzk_sse does on the host, and lane 0 decides.
// No workgroup waits for another one.  part[nblk]; *ticket is 0 on entry and is left at 0.
__global__ __launch_bounds__(256) void k_sse_decide(const uint8_t* __restrict__ orig, const float* __restrict__ pred, int H, int W, int Hp,
                                                     int Wp, int nblk, double* part, unsigned* ticket, DwpState* st, int idx, int nt,
                                                     double fe_pad, double threshold, int* idx_table, int stride, uint8_t* key,
                                                     uint8_t* gfirst, double* mse, int* c0_flag) {
    __shared__ double s[256];
    __shared__ double s_part[kDwpLds];
    __shared__ unsigned s_last;
    const double mine = tz_sse_block(orig, pred, H, W, Hp, Wp, blockIdx.x, s);
    if (threadIdx.x == 0) {
        // The partial goes out as a device-scope RETURNING exchange; its return value is consumed by an asm the compiler
        // cannot see through, which also drains vmcnt: the exchange has been performed (its old value has come back) before
        // the ticket increment is even issued.  Two relaxed atomics on different addresses are NOT ordered by issue order
        // (different L2 channels); a C-level "dependency" such as `1u + (old & 0)` is folded away by the compiler and left
        // a non-returning swap with no wait in front of the add (round 5's defect; tests/test_build_guard.py now reads
        // the sequence swap sc0 -> s_waitcnt vmcnt(0) -> add off the object code).  No agent-scope fence: that writes
        // back / invalidates a whole per-XCD L2 (measured: 22 us with __threadfence() on both sides).  The reader below
        // loads part[] with agent-scope atomic loads (`sc1`), after its own ticket add has returned and a barrier.
        unsigned long long old = atomicExch((unsigned long long*)(part + blockIdx.x), (unsigned long long)__double_as_longlong(mine));
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(old) : : "memory");
        s_last = atomicAdd(ticket, 1u) == (unsigned)(nblk - 1);
    }
    __syncthreads();
    if (!s_last) return;
    double t = 0.0;
    for (int b0 = 0; b0 < nblk; b0 += kDwpLds) {
        const int nb = min(kDwpLds, nblk - b0);
        __syncthreads();
        for (int b = threadIdx.x; b < nb; b += blockDim.x)
            s_part[b] = __hip_atomic_load(part + b0 + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sc1 load: never this CU's L1
        __syncthreads();
        if (threadIdx.x == 0)
            for (int b = 0; b < nb; ++b) t = t + s_part[b];
    }
    if (threadIdx.x != 0) return;
    *ticket = 0u;
    int key_idx = st->key_idx;
    double run = st->run + t;
    const double stop = run / ((double)(idx - key_idx + 1) * fe_pad);   // compress.py:246
    mse[idx] = stop;
    if (stop > threshold) {                                            // compress.py:249
        gfirst[idx] = 1;
        if (idx == nt - 1) key[idx] = 1;                               // compress.py:260-262
        else c0_flag[idx] = 1;
        key_idx = idx + 1;
        run = 0.0;
    }
    st->key_idx = key_idx;
    st->run = run;
    const int nidx = idx + 1;                                          // selection of the next step (218-222)
    if (nidx < nt) {
        const int from_key = nidx == key_idx;
        idx_table[0] = from_key;
        idx_table[stride] = nidx - 1;
        idx_table[2 * stride] = nidx;
        if (from_key) key[nidx - 1] = 1;
    }
}

// slot 0 of every group the DWP loop opened holds C0 (compress.py:258): one launch behind the loop, frame = blockIdx.y
// (nothing in the loop reads such a slot: the step after a boundary starts from the real frame)
__global__ void k_bcast_frames_flagged(const float* __restrict__ src, size_t fe, const int* __restrict__ flag, float* __restrict__ pred) {
    if (!flag[blockIdx.y]) return;
    float* dst = pred + (size_t)blockIdx.y * fe;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < fe; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

static int rollout_setup(tz_ctx* ctx, const uint8_t* frames, int nt, int H, int W, int warm_up,
                         const std::vector<int>* first = nullptr, int pred_frames = -1) {
    if (!ctx->model) return tz_fail(ctx, TZ_ERR_STATE, "no model loaded");
    if (nt < 1 || H < 1 || W < 1 || warm_up < 0 || nt > kMaxFrames || H > 32767 || W > 32767)
        return tz_fail(ctx, TZ_ERR_INVALID, "bad sequence shape nt=%d H=%d W=%d warm_up=%d (int16 trailer limits)", nt, H, W, warm_up);
    int Hp, Wp, maxB;
    TZ_TRY(tz_model_dims(ctx, &Hp, &Wp, &maxB));
    if (pad8(H) != Hp || pad8(W) != Wp)
        return tz_fail(ctx, TZ_ERR_INVALID,
                       "Image size is out of scope for this model: compatible sizes are height %d to %d and width %d to %d",
                       Hp - 7, Hp, Wp - 7, Wp);  // compress.py:178-181
    if (!frames && (!ctx->staged || ctx->nt != nt || ctx->H != H || ctx->W != W))
        return tz_fail(ctx, TZ_ERR_STATE, "no frame stack of this shape was staged (tz_frames_begin / tz_frames_put)");
    ctx->nt = nt;
    ctx->H = H;
    ctx->W = W;
    ctx->Hp = Hp;
    ctx->Wp = Wp;
    ctx->warm_up = warm_up;
    set_rollout(ctx, tz_ctx::ROLLOUT_NONE, 0, 0);
    ctx->pending_src = nullptr;
    ctx->pending_sent.clear();
    const size_t fsz = (size_t)H * W * 3;
    size_t fb = (size_t)nt * fsz, pb = (size_t)(pred_frames < 0 ? nt : pred_frames) * Hp * Wp * 3 * 4;
    if (frames) ctx->staged = false;
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_frames, &ctx->cap_frames, fb));
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_pred, &ctx->cap_pred, pb));
    if (!frames) {  // staged by tz_frames_put on the copy stream: the compute stream waits for the last of them
        TZ_HIP(ctx, hipEventRecord(ctx->ev_frames, ctx->copy_stream));
        TZ_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_frames, 0));
        return TZ_OK;
    }
    if (tz_is_device_ptr(frames)) {
        TZ_HIP(ctx, hipMemcpyAsync(ctx->d_frames, frames, fb, hipMemcpyDeviceToDevice, ctx->stream));
        return TZ_OK;
    }
    // earlier work queued on the compute stream may still read d_frames
    TZ_HIP(ctx, hipEventRecord(ctx->ev_compute, ctx->stream));
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute, 0));
    if (first && !first->empty() && (int)first->size() < nt) {
        ctx->pending_sent.assign(nt, 0);
        // frames at 16-byte-aligned offsets of a pinned stack: the compute stream reads them itself (k_fetch_frames)
        // (the device's view of the block: the same address for tz_host_alloc memory, possibly another one for memory the
        // caller registered himself; no mapping -> the copy engine as before)
        const uint8_t* dev_view = nullptr;
        bool fetch = tz_ptr_kind(frames) == 1 && fsz % 16 == 0 && first->size() <= 4096;
        if (fetch && (hipHostGetDevicePointer((void**)&dev_view, (void*)frames, 0) != hipSuccess || !dev_view || ((uintptr_t)dev_view & 15))) {
            (void)hipGetLastError();
            fetch = false;
        }
        std::vector<int> which;
        for (int f : *first) {
            if (f < 0 || f >= nt || ctx->pending_sent[f]) continue;
            if (fetch) which.push_back(f);
            else TZ_TRY(tz_h2d(ctx, ctx->d_frames + (size_t)f * fsz, frames + (size_t)f * fsz, fsz, ctx->copy_stream));
            ctx->pending_sent[f] = 1;
        }
        if (fetch && !which.empty()) {
            void* d_which;
            TZ_TRY(tz_pool_alloc(ctx, which.size() * sizeof(int), &d_which));
            TZ_TRY(tz_upload(ctx, d_which, which.data(), which.size() * sizeof(int)));
            const unsigned gx = (unsigned)std::min<size_t>((fsz / 16 + 255) / 256, 256);
            hipLaunchKernelGGL(k_fetch_frames, dim3(gx, (unsigned)which.size()), dim3(256), 0, ctx->stream, dev_view, ctx->d_frames,
                               (const int*)d_which, fsz);
            TZ_HIP(ctx, hipGetLastError());
        } else {
            TZ_HIP(ctx, hipEventRecord(ctx->ev_keys, ctx->copy_stream));
            TZ_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_keys, 0));
        }
        ctx->pending_src = frames;
        return TZ_OK;
    }
    TZ_TRY(tz_h2d(ctx, ctx->d_frames, frames, fb, ctx->copy_stream));
    TZ_HIP(ctx, hipEventRecord(ctx->ev_frames, ctx->copy_stream));
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_frames, 0));
    return TZ_OK;
}

// second half of a split upload: every frame not sent by rollout_setup, in contiguous runs; the
// compute stream continues (delta stage, window MSE) only after they have landed
static int rollout_finish_upload(tz_ctx* ctx) {
    if (!ctx->pending_src) return TZ_OK;
    const size_t fsz = (size_t)ctx->H * ctx->W * 3;
    const uint8_t* src = ctx->pending_src;
    ctx->pending_src = nullptr;
    for (int f = 0; f < ctx->nt;) {
        if (ctx->pending_sent[f]) {
            ++f;
            continue;
        }
        int g = f;
        while (g < ctx->nt && !ctx->pending_sent[g]) ++g;
        TZ_TRY(tz_h2d(ctx, ctx->d_frames + (size_t)f * fsz, src + (size_t)f * fsz, (size_t)(g - f) * fsz, ctx->copy_stream));
        f = g;
    }
    TZ_HIP(ctx, hipEventRecord(ctx->ev_frames, ctx->copy_stream));
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_frames, 0));
    return TZ_OK;
}

// copy C0 into the given slots of the prediction stack
static int fill_c0(tz_ctx* ctx, const std::vector<int>& slots) {
    if (slots.empty()) return TZ_OK;
    const float* c0;
    TZ_TRY(tz_model_c0_dev(ctx, &c0));
    size_t fe = (size_t)ctx->Hp * ctx->Wp * 3;
    void* d_slots;
    TZ_TRY(tz_pool_alloc(ctx, slots.size() * sizeof(int), &d_slots));
    TZ_TRY(tz_upload(ctx, d_slots, slots.data(), slots.size() * sizeof(int)));
    int gx = (int)std::min<size_t>((fe + 255) / 256, 1024);
    hipLaunchKernelGGL(k_bcast_frame, dim3(gx, (unsigned)slots.size()), dim3(256), 0, ctx->stream, c0, fe,
                       (const int*)d_slots, (int)slots.size(), ctx->d_pred);
    TZ_HIP(ctx, hipGetLastError());
    return TZ_OK;
}

// Run a static schedule: items (out frame, from_key, in frame) grouped by depth; every depth
// is one batched predictor call over all windows (their recursions are independent).
struct PredItem {
    int out, from_key, in, depth;
};
// The schedule is static: its index table is uploaded once and every depth is one batched
// predictor call over all windows (launch-only, no per-step copies).  Capturing this sequence
// into a hipGraph was measured and brings nothing (cfg1/cfg2 are bound by the latency of their
// tiny grids, not by launch overhead; cfg3+ are GPU-bound), so the launches stay plain.
// frames: the stack the items' frame indices refer to (NULL = the context's whole stack; a range rollout passes a sub-stack)
static int run_schedule(tz_ctx* ctx, std::vector<PredItem>& items, const uint8_t* frames = nullptr) {
    int Hp, Wp, maxB;
    TZ_TRY(tz_model_dims(ctx, &Hp, &Wp, &maxB));
    if (items.empty()) return TZ_OK;
    std::stable_sort(items.begin(), items.end(), [](const PredItem& a, const PredItem& b) { return a.depth < b.depth; });
    // A window is a chain of items (each reads what the one before it wrote); chains never touch each other.
    // TEZIP_SPLIT=1 deals them to two GROUPS that advance on two streams with their own activation slots: the
    // launches of a predictor step depend on each other, so on one stream every launch ramps up and drains alone
    // (0.895 of the MFMA peak at 4 windows against 0.917 at 32), and with two independent launch
    // chains one group's launch could fill the CUs the other's draining launch leaves idle.  Measured in round 3
    // (bit-identical, all GPU tests green with it on): 62.5 -> 65.4 ms per cfg3 step -- two half-sized launches
    // lose more to their own ramps than the overlap returns -- so it is OFF by default and kept as a switch.
    // (tests/test_gpu_two_groups.py runs it against the one-group rollout and the C oracle; TEZIP_SPLIT_LOG=1 says that it ran.)
    // Per-launch event timing needs launches that run alone: profiling keeps one stream in any case.
    const bool split = ctx->split_rollout && ctx->stream2 && maxB >= 2 && !ctx->prof_on;
    const int capA = split ? (maxB + 1) / 2 : maxB, capB = maxB - capA;
    std::vector<int> group(items.size(), 0);
    if (split) {
        std::vector<int> chain_of(ctx->nt, -1);   // frame slot -> group of the chain that wrote it
        int nchains = 0;
        for (size_t i = 0; i < items.size(); ++i) {
            int g;
            if (items[i].from_key || chain_of[items[i].in] < 0) g = (nchains++) & 1;
            else g = chain_of[items[i].in];
            group[i] = g;
            chain_of[items[i].out] = g;
        }
    }
    // per group: batches of one depth, [is_key | in | out | next slot] x maxB ints each.  next slot: where the item's
    // prediction sits in the NEXT batch of its group when that batch holds its consumer (the next step of the window);
    // the prediction kernel then writes the consumer's level-0 error maps itself, and a batch all of whose items were
    // served that way runs without its k_err0 launch (18 of the 19 steps of a cfg3 rollout).
    std::vector<int> table;
    std::vector<int> counts[2];
    std::vector<size_t> offs[2];
    std::vector<char> all_fed[2];   // per batch: every item's E_0 slot comes from the batch in front
    for (int g = 0; g < (split ? 2 : 1); ++g) {
        const int cap = g == 0 ? capA : capB;
        std::vector<std::vector<size_t>> batches;
        size_t i = 0;
        while (i < items.size()) {
            const int depth = items[i].depth;
            size_t j = i;
            while (j < items.size() && items[j].depth == depth) ++j;
            std::vector<size_t> mine;
            for (size_t k = i; k < j; ++k)
                if (group[k] == g) mine.push_back(k);
            for (size_t q = 0; q < mine.size(); q += cap)
                batches.emplace_back(mine.begin() + q, mine.begin() + std::min(mine.size(), q + (size_t)cap));
            i = j;
        }
        for (size_t b = 0; b < batches.size(); ++b) {
            const size_t nb = batches[b].size(), base = table.size();
            table.resize(base + 4 * (size_t)maxB, 0);
            for (size_t k = 0; k < nb; ++k) {
                const PredItem& it = items[batches[b][k]];
                table[base + k] = it.from_key;
                table[base + maxB + k] = it.in;
                table[base + 2 * maxB + k] = it.out;
                int next = -1;
                if (b + 1 < batches.size())
                    for (size_t k2 = 0; k2 < batches[b + 1].size(); ++k2) {
                        const PredItem& c = items[batches[b + 1][k2]];
                        if (!c.from_key && c.in == it.out) next = (int)k2;
                    }
                table[base + 3 * maxB + k] = next;
            }
            bool fed = b > 0;
            if (b > 0)
                for (size_t k = 0; k < nb && fed; ++k) {
                    const PredItem& c = items[batches[b][k]];
                    bool found = false;
                    for (size_t k0 = 0; k0 < batches[b - 1].size() && !found; ++k0)
                        found = !c.from_key && items[batches[b - 1][k0]].out == c.in;
                    fed = found;
                }
            counts[g].push_back((int)nb);
            offs[g].push_back(base);
            all_fed[g].push_back(fed ? 1 : 0);
        }
    }
    if (split && getenv("TEZIP_SPLIT_LOG"))
        fprintf(stderr, "[tezip] two-group rollout: caps %d + %d, batches %zu + %zu\n", capA, capB, counts[0].size(), counts[1].size());
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_sched, &ctx->cap_sched, table.size() * sizeof(int)));
    TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));  // an earlier rollout may still read the old table
    TZ_HIP(ctx, hipMemcpy(ctx->d_sched, table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice));
    if (split && !counts[1].empty()) {
        TZ_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));          // everything queued so far (frames, C0 slots)
        TZ_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
    }
    hipStream_t main_stream = ctx->stream;
    int rc = TZ_OK;
    const size_t steps = std::max(counts[0].size(), counts[1].size());
    bool fused[2] = {false, false};   // did the previous batch of the group write the next one's error maps?
    for (size_t b = 0; b < steps && rc == TZ_OK; ++b) {
        for (int g = 0; g < 2 && rc == TZ_OK; ++g) {
            if (b >= counts[g].size()) continue;
            const int slot0 = g == 0 ? 0 : capA;
            const int* tab = ctx->d_sched + offs[g][b];
            // the slot numbers of the table are positions in the batch: the activation slots of a group start at slot0
            const bool skip = fused[g] && all_fed[g][b];
            if (g == 1) ctx->stream = ctx->stream2;   // the launchers take the context's stream
            rc = tz_model_predict_batch_dev(ctx, counts[g][b], tab, maxB, frames ? frames : ctx->d_frames, ctx->H, ctx->W, ctx->d_pred, ctx->d_pred, slot0,
                                            tab + 3 * (size_t)maxB, skip, &fused[g]);
            ctx->stream = main_stream;
        }
    }
    if (split && !counts[1].empty()) {
        hipError_t e = hipEventRecord(ctx->ev_join, ctx->stream2);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);
        if (e != hipSuccess && rc == TZ_OK) rc = tz_fail(ctx, TZ_ERR_HIP, "rollout join: %s", hipGetErrorString(e));
    }
    return rc;
}

// ---- streaming ingestion / delivery: the frame stack enters window by window and the payload
// leaves chunk by chunk, so that the host never holds more than a few windows (SURVEY.md §8f-3;
// the reference keeps everything in RAM, compress.py:116-122,329-333).
extern "C" int tz_frames_begin(tz_ctx* ctx, int nt, int H, int W) {
    if (!ctx) return TZ_ERR_INVALID;
    if (nt < 1 || H < 1 || W < 1 || nt > kMaxFrames || H > 32767 || W > 32767)
        return tz_fail(ctx, TZ_ERR_INVALID, "bad sequence shape nt=%d H=%d W=%d (int16 trailer limits)", nt, H, W);
    set_rollout(ctx, tz_ctx::ROLLOUT_NONE, 0, 0);
    ctx->staged = false;
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_frames, &ctx->cap_frames, (size_t)nt * H * W * 3));
    // earlier work queued on the compute stream may still read d_frames
    TZ_HIP(ctx, hipEventRecord(ctx->ev_compute, ctx->stream));
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute, 0));
    ctx->nt = nt;
    ctx->H = H;
    ctx->W = W;
    ctx->staged = true;
    return TZ_OK;
}

extern "C" int tz_frames_put(tz_ctx* ctx, int first, int count, const uint8_t* frames) {
    if (!ctx || !frames) return TZ_ERR_INVALID;
    if (!ctx->staged) return tz_fail(ctx, TZ_ERR_STATE, "tz_frames_put needs a tz_frames_begin first");
    if (first < 0 || count < 0 || first + count > ctx->nt) return tz_fail(ctx, TZ_ERR_INVALID, "frames [%d, %d) outside the stack", first, first + count);
    const size_t fsz = (size_t)ctx->H * ctx->W * 3;
    return tz_h2d(ctx, ctx->d_frames + (size_t)first * fsz, frames, (size_t)count * fsz, ctx->copy_stream);
}

extern "C" int tz_frames_fence(tz_ctx* ctx) {
    if (!ctx) return TZ_ERR_INVALID;
    TZ_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    return TZ_OK;
}

extern "C" int tz_frames_get(tz_ctx* ctx, int first, int count, uint8_t* out) {
    if (!ctx || !out) return TZ_ERR_INVALID;
    if (!ctx->d_frames || first < 0 || count < 0 || first + count > ctx->nt)
        return tz_fail(ctx, TZ_ERR_INVALID, "frames [%d, %d) outside the resident stack", first, first + count);
    const size_t fsz = (size_t)ctx->H * ctx->W * 3;
    TZ_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    TZ_TRY(tz_d2h(ctx, out, ctx->d_frames + (size_t)first * fsz, (size_t)count * fsz, ctx->stream));
    TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TZ_OK;
}

extern "C" int tz_payload_begin(tz_ctx* ctx, size_t count) {
    if (!ctx) return TZ_ERR_INVALID;
    ctx->enc_kind = tz_ctx::ENC_NONE;   // whatever the encoder left in d_payload is about to be overwritten
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_payload, &ctx->cap_payload, std::max<size_t>(count, 8) * 2));
    ctx->payload_len = count;
    TZ_HIP(ctx, hipEventRecord(ctx->ev_compute, ctx->stream));  // earlier work may still read the old payload
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute, 0));
    return TZ_OK;
}

extern "C" int tz_payload_put(tz_ctx* ctx, size_t offset, size_t count, const int16_t* src) {
    if (!ctx || !src) return TZ_ERR_INVALID;
    if (!ctx->d_payload || offset + count > ctx->payload_len) return tz_fail(ctx, TZ_ERR_INVALID, "payload range outside the staged payload");
    return tz_h2d(ctx, ctx->d_payload + offset, src, count * 2, ctx->copy_stream);
}

extern "C" int tz_decoded_get(tz_ctx* ctx, int first, int count, uint8_t* out) {
    if (!ctx || !out) return TZ_ERR_INVALID;
    if (!ctx->d_out || !ctx->have_decoded || first < ctx->dec_first || count < 0 || first + count > ctx->dec_first + ctx->dec_count)
        return tz_fail(ctx, TZ_ERR_INVALID, "frames [%d, %d) outside the resident decoded stack", first, first + count);
    const size_t fsz = (size_t)ctx->H * ctx->W * 3;
    TZ_TRY(tz_d2h(ctx, out, ctx->d_out + (size_t)(first - ctx->dec_first) * fsz, (size_t)count * fsz, ctx->stream));
    return tz_stream_sync(ctx);
}

extern "C" int tz_payload_get(tz_ctx* ctx, size_t offset, size_t count, int16_t* out) {
    if (!ctx || !out) return TZ_ERR_INVALID;
    if (!ctx->d_payload || offset + count > ctx->payload_len) return tz_fail(ctx, TZ_ERR_INVALID, "payload range outside the resident payload");
    TZ_TRY(tz_d2h(ctx, out, ctx->d_payload + offset, count * 2, ctx->stream));
    TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TZ_OK;
}

// SWP: window boundaries are known up front (compress.py:249: (idx-p) % w == 0), so all windows advance together.  The
// prediction the reference makes and drops at a boundary (251-253) is only evaluated when the MSE log is wanted (-v prints
// it, 245-247).  key, gfirst, c0_slots: what the warm-up left, completed here; mse: the log, when wanted.
static int rollout_swp(tz_ctx* ctx, int window, bool want_mse, std::vector<int>& c0_slots, std::vector<uint8_t>& key,
                       std::vector<uint8_t>& gfirst, std::vector<double>& mse) {
    const int nt = ctx->nt, p = ctx->warm_up;
    const size_t fe_pad = (size_t)ctx->Hp * ctx->Wp * 3;
    std::vector<PredItem> items;
    std::vector<int> dropped;
    int key_idx = p + 1;
    for (int idx = p + 1; idx < nt; ++idx) {
        bool from_key = idx == key_idx;
        if (from_key) key[idx - 1] = 1;
        bool trig = (idx - p) % window == 0;
        if (trig) gfirst[idx] = 1;
        if (trig && !want_mse) {
            c0_slots.push_back(idx);
        } else {
            items.push_back(PredItem{idx, from_key ? 1 : 0, idx - 1, idx - (key_idx - 1)});
            if (trig && idx != nt - 1) dropped.push_back(idx);  // the last frame keeps it (260-262)
        }
        if (trig) {
            if (idx == nt - 1) key[idx] = 1;  // compress.py:260-262
            key_idx = idx + 1;
        }
    }
    TZ_TRY(fill_c0(ctx, c0_slots));
    TZ_TRY(run_schedule(ctx, items));
    TZ_TRY(rollout_finish_upload(ctx));
    if (!want_mse) return TZ_OK;
    std::vector<double> sse(nt, 0.0);
    TZ_TRY(tzk_sse(ctx, ctx->d_frames, ctx->d_pred, nt, ctx->H, ctx->W, ctx->Hp, ctx->Wp, sse.data()));
    int k0 = p + 1;
    double run = 0.0;
    for (int idx = p + 1; idx < nt; ++idx) {
        run = run + sse[idx];
        mse[idx] = run / (double)((size_t)(idx - k0 + 1) * fe_pad);
        if (gfirst[idx]) {
            k0 = idx + 1;
            run = 0.0;
        }
    }
    return fill_c0(ctx, dropped);  // slot 0 of the next group holds C0 (258)
}

// DWP: boundaries depend on the window MSE of the padded frames (compress.py:245-249).  The decision is taken ON THE DEVICE
// (k_sse_decide): it sums the frame's partial squared errors in the fixed order, compares the window mean with the
// threshold, marks the key frame and writes the input selection of the next predictor step, so the host only queues
// launches -- no round trip per frame -- and reads the key mask / MSE log once at the end.
static int rollout_dwp(tz_call& call, double threshold, const std::vector<int>& c0_slots, std::vector<uint8_t>& key,
                       std::vector<uint8_t>& gfirst, std::vector<double>& mse) {
    tz_ctx* ctx = call.ctx;
    const int nt = ctx->nt, H = ctx->H, W = ctx->W, p = ctx->warm_up;
    const size_t fe_pad = (size_t)ctx->Hp * ctx->Wp * 3;
    TZ_TRY(fill_c0(ctx, c0_slots));
    int Hp_, Wp_, maxB;
    TZ_TRY(tz_model_dims(ctx, &Hp_, &Wp_, &maxB));
    const int nblk = tzk_sse_blocks(ctx->Hp, ctx->Wp);
    DwpState* d_state;
    double *d_part, *d_mse;
    uint8_t *d_key, *d_gf;
    int *d_flag, *d_slot0;   // (d_slot0: one int 0 = "the prediction is the input of slot 0 of the next step")
    unsigned* d_ticket;
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_sched, &ctx->cap_sched, 3 * (size_t)maxB * sizeof(int)));
    TZ_TRY(call.alloc(sizeof(DwpState), &d_state));
    TZ_TRY(call.alloc(sizeof(double) * nblk, &d_part));
    TZ_TRY(call.alloc(nt, &d_key));
    TZ_TRY(call.alloc(nt, &d_gf));
    TZ_TRY(call.alloc(sizeof(double) * nt, &d_mse));
    TZ_TRY(call.alloc(sizeof(int) * nt, &d_flag));
    TZ_TRY(call.alloc(256, &d_ticket));
    TZ_TRY(call.alloc(256, &d_slot0));
    TZ_TRY(tz_upload(ctx, d_key, key.data(), nt));
    TZ_TRY(tz_upload(ctx, d_gf, gfirst.data(), nt));
    hipError_t e = hipMemsetAsync(d_mse, 0, sizeof(double) * nt, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_flag, 0, sizeof(int) * nt, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_ticket, 0, 256, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_slot0, 0, 256, ctx->stream);
    if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "DWP state: %s", hipGetErrorString(e));
    const float* c0 = nullptr;
    TZ_TRY(tz_model_c0_dev(ctx, &c0));
    hipLaunchKernelGGL(k_dwp_init, dim3(1), dim3(1), 0, ctx->stream, d_state, p, nt, ctx->d_sched, maxB, d_key);
    if (hipGetLastError() != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "k_dwp_init launch failed");
    const int gx = (int)std::min<size_t>((fe_pad + 255) / 256, 1024);
    bool prev_fused = false;
    for (int idx = p + 1; idx < nt; ++idx) {
        // the prediction kernel also writes the level-0 error maps of the NEXT step as if that step went on from this
        // prediction (as in the static schedule); the next step's error unit then runs for a key-frame start only --
        // which of the two it is, k_sse_decide says on the device
        bool fused = false;
        static const bool spec = !getenv("TEZIP_DWP_SPEC") || atoi(getenv("TEZIP_DWP_SPEC")) != 0;   // (0: measurements)
        TZ_TRY(tz_model_predict_batch_dev(ctx, 1, ctx->d_sched, maxB, ctx->d_frames, H, W, ctx->d_pred, ctx->d_pred, 0,
                                          spec ? (const int*)d_slot0 : nullptr, false, &fused, prev_fused));
        prev_fused = fused;
        {
            tz_prof_scope ps(ctx, TZP_SSE);
            hipLaunchKernelGGL(k_sse_decide, dim3(nblk), dim3(256), 0, ctx->stream, ctx->d_frames + (size_t)idx * H * W * 3,
                               ctx->d_pred + (size_t)idx * fe_pad, H, W, ctx->Hp, ctx->Wp, nblk, d_part, d_ticket, d_state, idx, nt,
                               (double)fe_pad, threshold, ctx->d_sched, maxB, d_key, d_gf, d_mse, d_flag);
        }
        if (hipGetLastError() != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "DWP launch failed");
    }
    // slot 0 of every group opened on the way holds C0 (258); the last frame keeps its prediction (260-262: k_sse_decide
    // does not flag it)
    if (nt > 1) {
        static_assert(kMaxFrames <= 65535, "gridDim.y = nt");   // (rollout_setup refuses nt > kMaxFrames)
        hipLaunchKernelGGL(k_bcast_frames_flagged, dim3(std::min(gx, 128), nt), dim3(256), 0, ctx->stream, c0, fe_pad, (const int*)d_flag, ctx->d_pred);
        if (hipGetLastError() != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "DWP launch failed");
    }
    e = hipMemcpyAsync(key.data(), d_key, nt, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(gfirst.data(), d_gf, nt, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(mse.data(), d_mse, sizeof(double) * nt, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "DWP result download: %s", hipGetErrorString(e));
    return TZ_OK;
}

extern "C" int tz_rollout(tz_ctx* ctx, const uint8_t* frames, int nt, int H, int W, int warm_up, int window,
                          double threshold, uint8_t* key_mask, double* mse_log) {
    tz_roctx_range roctx_("tz_rollout");
    if (!ctx) return TZ_ERR_INVALID;
    ctx->enc_kind = tz_ctx::ENC_NONE;   // the symbols of a tz_encode_begin or a resident payload belong to the rollout before it
    if (window < 0) return tz_fail(ctx, TZ_ERR_INVALID, "window must be >= 0");
    if (nt < warm_up + 2)  // the reference breaks here
        return tz_fail(ctx, TZ_ERR_INVALID, "need at least warm_up+2 frames (nt=%d, warm_up=%d)", nt, warm_up);
    const int p = warm_up;
    const bool dwp = window == 0;
    std::vector<int> first;  // SWP reads exactly the frames that start a window (compress.py:218-220)
    if (!dwp)
        for (int f = p; f < nt; f += window) first.push_back(f);
    tz_call call(ctx);
    TZ_TRY(rollout_setup(ctx, frames, nt, H, W, warm_up, dwp ? nullptr : &first));
    std::vector<uint8_t> key(nt, 0), gfirst(nt, 0), qskip(nt, 0);
    std::vector<double> mse(nt, 0.0);
    std::vector<int> c0_slots;
    // compress.py:188-211: warm-up frames are key frames whose "prediction" is C0
    for (int i = 0; i < p; ++i) {
        key[i] = 1;
        qskip[i] = 1;  // error_bound is skipped for group 0 (compress.py:315)
        c0_slots.push_back(i);
    }
    gfirst[0] = 1;
    if (p > 0) {
        gfirst[p] = 1;
        c0_slots.push_back(p);
    } else {
        c0_slots.push_back(0);
    }
    const int rc = dwp ? rollout_dwp(call, threshold, c0_slots, key, gfirst, mse)
                       : rollout_swp(ctx, window, mse_log != nullptr, c0_slots, key, gfirst, mse);
    if (rc != TZ_OK) {  // nothing of a failed rollout may still read the caller's frames when we return
        (void)hipStreamSynchronize(ctx->copy_stream);
        ctx->pending_src = nullptr;
        return rc;
    }
    for (int i = 0; i < nt; ++i)
        if (gfirst[i]) qskip[i] = 1;
    ctx->key_mask = key;
    ctx->group_first = gfirst;
    ctx->quant_skip = qskip;
    set_rollout(ctx, tz_ctx::ROLLOUT_ENCODE, 0, nt);
    ctx->pred_contract = tz_get_contract(ctx);
    if (key_mask) memcpy(key_mask, key.data(), nt);
    if (mse_log) memcpy(mse_log, mse.data(), sizeof(double) * nt);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "rollout failed: %s", hipGetErrorString(e));
    return TZ_OK;
}
// decompress.py:138-186: the frames the decoder reconstructs from their key-frame bytes rather than from a prediction slot
// -- frame 0 and every key frame from the warm_up-th on; the warm-up frames 1..warm_up-1 reconstruct from their C0 slot.
// key: the key mask of an n-frame stack.  The decoder's rollouts leave this in ctx->key_mask; tz_encode_quality derives
// it from the encoder's key mask, so that its tail reconstructs what -u does.
static std::vector<uint8_t> recon_key_mask(const uint8_t* key, int n, int warm_up) {
    std::vector<uint8_t> r(n, 0);
    for (int i = 0, k = 0; i < n; ++i)
        if (key[i]) r[i] = k++ >= warm_up;
    if (n > 0) r[0] = 1;   // decompress.py:186
    return r;
}

// decompress.py:123-129: a frame of the resident stack is a key frame iff it has a non-zero sample (flags back on the host)
static int discover_keys(tz_ctx* ctx, int nt, int H, int W, std::vector<int>* flags) {
    void* d_flags;
    TZ_TRY(tz_pool_alloc(ctx, sizeof(int) * nt, &d_flags));
    size_t fb = (size_t)H * W * 3;
    hipError_t e = hipMemsetAsync(d_flags, 0, sizeof(int) * nt, ctx->stream);
    int gx = (int)std::min<size_t>((fb + 255) / 256, 64);
    static_assert(kMaxFrames <= 65535, "gridDim.y = nt");   // (rollout_setup refuses nt > kMaxFrames)
    hipLaunchKernelGGL(k_any_nonzero, dim3(gx, nt), dim3(256), 0, ctx->stream, ctx->d_frames, fb, (int*)d_flags);
    if (e == hipSuccess) e = hipMemcpyAsync(flags->data(), d_flags, sizeof(int) * nt, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "key discovery failed: %s", hipGetErrorString(e));
    return TZ_OK;
}

// The decoder's rollout (decompress.py:138-179) of frames [first, first + count) of the nt-frame key stack: the whole key
// stack is staged (key discovery looks at every frame), the predictor runs from the range's restart frame r
// (tz_range_restart) to the range's end, and slot i of the prediction stack holds frame r + i.  [0, nt) is the whole
// decode.  range: tz_rollout_decode_range's refusals -- frames 0..warm_up must be key frames -- ahead of the walk's own.
static int rollout_decode(tz_ctx* ctx, const uint8_t* key_frames, int nt, int H, int W, int warm_up, int first, int count,
                          uint8_t* key_mask, bool range) {
    ctx->enc_kind = tz_ctx::ENC_NONE;
    tz_call call(ctx);
    // (a range sizes its prediction stack once it knows its restart frame)
    TZ_TRY(rollout_setup(ctx, key_frames, nt, H, W, warm_up, nullptr, first == 0 && count == nt ? nt : 1));
    std::vector<int> flags(nt, 0);
    TZ_TRY(discover_keys(ctx, nt, H, W, &flags));
    for (int i = 0; range && i <= warm_up; ++i)
        if (i >= nt || !flags[i]) return tz_fail(ctx, TZ_ERR_INVALID, "key frames do not cover the sequence (frame %d)", i);
    std::vector<uint8_t> mask(nt);
    for (int i = 0; i < nt; ++i) mask[i] = flags[i] ? 1 : 0;
    int r = 0;
    TZ_TRY(tz_range_restart(mask.data(), nt, warm_up, first, &r));
    // sub-stack [r, end): from a key frame r > warm_up with warm_up 0, or from frame 0 with the job's warm_up -- and then
    // reaching frame warm_up, which the key-interval walk starts from (the whole decode of warm_up == nt: all C0 copies)
    const int end = r == 0 ? std::min(nt, std::max(first + count, warm_up + 1)) : first + count;
    const int ns = end - r, sw = r == 0 ? warm_up : 0;
    std::vector<int> kfc;
    for (int i = 0; i < nt; ++i)
        if (flags[i]) kfc.push_back(i);
    kfc.push_back(nt);
    // warm_up copies of C0, then for every key interval: the key frame itself, one prediction from the key frame, then
    // recursion on the previous prediction.  The walk checks the whole stack and keeps the frames of [r, end).
    std::vector<int> c0_slots;
    std::vector<PredItem> items;
    for (int i = 0; i < std::min(sw, ns); ++i) c0_slots.push_back(i);
    int produced = warm_up;
    for (int k = warm_up; k + 1 < (int)kfc.size(); ++k)
        for (int pi = kfc[k]; pi < kfc[k + 1]; ++pi, ++produced) {
            if (produced != pi) return tz_fail(ctx, TZ_ERR_INVALID, "key frames do not cover the sequence (frame %d)", pi);
            if (pi < r || pi >= end) continue;
            if (pi == kfc[k]) {
                c0_slots.push_back(pi - r);  // slot content is never used for reconstruction
            } else {
                items.push_back(PredItem{pi - r, pi == kfc[k] + 1 ? 1 : 0, pi - 1 - r, pi - kfc[k]});
            }
        }
    if (produced != nt) return tz_fail(ctx, TZ_ERR_INVALID, "key frames do not cover the sequence (%d of %d frames)", produced, nt);
    const std::vector<uint8_t> recon_key = recon_key_mask(mask.data() + r, ns, sw);   // (frame 0 of it: 0, or the key frame r)
    const size_t fsz = (size_t)H * W * 3;
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_pred, &ctx->cap_pred, (size_t)ns * ctx->Hp * ctx->Wp * 3 * 4));
    TZ_TRY(fill_c0(ctx, c0_slots));
    TZ_TRY(run_schedule(ctx, items, ctx->d_frames + (size_t)r * fsz));
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "%sdecode rollout failed: %s", range ? "range " : "", hipGetErrorString(e));
    ctx->key_mask = recon_key;
    set_rollout(ctx, tz_ctx::ROLLOUT_DECODE, r, end);
    ctx->pred_contract = tz_get_contract(ctx);
    if (key_mask) memcpy(key_mask, mask.data(), nt);
    return TZ_OK;
}

extern "C" int tz_rollout_decode(tz_ctx* ctx, const uint8_t* key_frames, int nt, int H, int W, int warm_up,
                                 uint8_t* key_mask) {
    tz_roctx_range roctx_("tz_rollout_decode");
    if (!ctx) return TZ_ERR_INVALID;
    return rollout_decode(ctx, key_frames, nt, H, W, warm_up, 0, nt, key_mask, false);
}

extern "C" int tz_range_restart(const uint8_t* key_mask, int nt, int warm_up, int first, int* restart) {
    if (!key_mask || !restart || nt < 1 || warm_up < 0 || first < 0 || first >= nt) return TZ_ERR_INVALID;
    int r = 0;
    for (int k = first; k > warm_up; --k)
        if (key_mask[k]) {
            r = k;
            break;
        }
    *restart = r;
    return TZ_OK;
}

extern "C" int tz_rollout_decode_range(tz_ctx* ctx, const uint8_t* key_frames, int nt, int H, int W, int warm_up, int first,
                                       int count, uint8_t* key_mask) {
    tz_roctx_range roctx_("tz_rollout_decode_range");
    if (!ctx) return TZ_ERR_INVALID;
    if (nt < 1 || first < 0 || count < 1 || first >= nt || count > nt - first)
        return tz_fail(ctx, TZ_ERR_INVALID, "frame range [%d, %d + %d) outside the %d-frame sequence", first, first, count, nt);
    if (!key_frames && ctx->staged && (ctx->nt != nt || ctx->H != H || ctx->W != W))
        return tz_fail(ctx, TZ_ERR_INVALID, "range decode of a %d x %d x %d stack, the staged stack is %d x %d x %d", nt, H, W,
                       ctx->nt, ctx->H, ctx->W);
    return rollout_decode(ctx, key_frames, nt, H, W, warm_up, first, count, key_mask, true);
}

extern "C" int tz_get_predictions(tz_ctx* ctx, float* out) {
    if (!ctx || !out) return TZ_ERR_INVALID;
    if (ctx->rollout_kind == tz_ctx::ROLLOUT_NONE || !whole_stack(ctx, ctx->rollout_kind))
        return tz_fail(ctx, TZ_ERR_STATE, "no rollout in this context");
    size_t bytes = (size_t)ctx->nt * ctx->Hp * ctx->Wp * 3 * 4;
    TZ_HIP(ctx, hipMemcpyAsync(out, ctx->d_pred, bytes, hipMemcpyDefault, ctx->stream));
    TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TZ_OK;
}

// --------------------------------------------------------------------- table / LUT (host)
extern "C" int tz_build_table(const unsigned long long* hist, int nbins, int16_t* table, int* table_len) {
    if (!hist || !table || !table_len || nbins < 1 || nbins > 32767) return TZ_ERR_INVALID;
    // compress.py:352-361: symbols with count > 0, count descending; Python's stable sort with
    // reverse=True keeps ascending symbol order among equal counts.
    std::vector<int> syms;
    for (int s = 0; s < nbins; ++s)
        if (hist[s]) syms.push_back(s);
    std::stable_sort(syms.begin(), syms.end(), [&](int a, int b) { return hist[a] > hist[b]; });
    if ((int)syms.size() > TZ_MAX_TABLE) return TZ_ERR_INVALID;
    for (size_t i = 0; i < syms.size(); ++i) table[i] = (int16_t)syms[i];
    *table_len = (int)syms.size();
    return TZ_OK;
}

static int build_enc_lut(tz_ctx* ctx, const int16_t* table, int T, std::vector<int16_t>* lut) {
    lut->resize(TZ_NBINS + 1);
    for (int v = 0; v <= TZ_NBINS; ++v) (*lut)[v] = (int16_t)v;
    for (int idx = 0; idx < T; ++idx) {
        int s = table[idx];
        // compress.py:87-88 applied to arbitrary tables would chain substitutions; the
        // encoder only ever sees its own table (symbols >= 1090 > any rank), so reject others.
        if (s < TZ_MAX_TABLE || s > TZ_NBINS) return tz_fail(ctx, TZ_ERR_INVALID, "table symbol %d outside [%d, %d]", s, TZ_MAX_TABLE, TZ_NBINS);
        (*lut)[s] = (int16_t)idx;
    }
    return TZ_OK;
}

// decompress.py:31-36 sequential-pass semantics (incl. chained substitutions) + optional 1600-x
static void build_dec_lut(const int16_t* table, int T, int apply_offset, std::vector<int16_t>* lut) {
    lut->resize(TZ_NBINS + 1);
    for (int v = 0; v <= TZ_NBINS; ++v) {
        int cur = v, last = -1;
        while (cur >= 0 && cur < T && cur > last) {
            last = cur;
            cur = table[cur];
        }
        (*lut)[v] = (int16_t)(apply_offset ? TZ_OFFSET - cur : cur);
    }
}

// ------------------------------------------------------------------------ encode / decode
// Last stage of tz_encode: rank remap (compress.py:369).  A host payload leaves chunk by chunk on
// the copy stream behind the remap kernel, so that the device -> host transfer overlaps it.
static int remap_out(tz_ctx* ctx, const int16_t* d_sd, size_t N, const int16_t* lut, tz_out* o, bool defer = false) {
    constexpr int kChunks = 8;
    if (!o->host || (N < ((size_t)1 << 22) && !defer)) return tzk_lut(ctx, d_sd, N, lut, 0, (int16_t*)o->dev);
    const size_t per = ((N + kChunks - 1) / kChunks + 7) & ~(size_t)7;
    while (ctx->chunk_ev.size() < (size_t)kChunks) {
        hipEvent_t e;
        TZ_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->chunk_ev.push_back(e);
    }
    int k = 0;
    for (size_t off = 0; off < N; off += per, ++k) {
        const size_t n = std::min(per, N - off);
        TZ_TRY(tzk_lut(ctx, d_sd + off, n, lut, 0, (int16_t*)o->dev + off));
        TZ_HIP(ctx, hipEventRecord(ctx->chunk_ev[k], ctx->stream));
    }
    k = 0;
    for (size_t off = 0; off < N; off += per, ++k) {
        const size_t n = std::min(per, N - off);
        TZ_HIP(ctx, hipStreamWaitEvent(ctx->down_stream, ctx->chunk_ev[k], 0));
        TZ_TRY(tz_d2h(ctx, (int16_t*)o->host + off, (const int16_t*)o->dev + off, n * 2, ctx->down_stream));
    }
    if (defer) {   // the caller collects the payload with tz_payload_wait: the transfer runs under whatever comes next
        if (!ctx->ev_payload) TZ_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_payload, hipEventDisableTiming));
        TZ_HIP(ctx, hipEventRecord(ctx->ev_payload, ctx->down_stream));
        ctx->payload_inflight = true;
    } else {
        TZ_HIP(ctx, hipStreamSynchronize(ctx->down_stream));
    }
    o->done = true;
    return TZ_OK;
}

// What every encode entry checks before it touches a buffer (a NaN bound is refused by the quantiser's own launches).
static int encode_check(tz_ctx* ctx, const char* who, int mode) {
    if (!whole_stack(ctx, tz_ctx::ROLLOUT_ENCODE)) return tz_fail(ctx, TZ_ERR_STATE, "%s needs a tz_rollout first", who);
    TZ_TRY(tz_check_pred_contract(ctx, who));
    if (mode < 0 || mode > 3) return tz_fail(ctx, TZ_ERR_INVALID, "unknown error-bound mode %d", mode);
    if (!ctx->frame_bounds.empty()) {   // tz_set_frame_bounds: b0 and b1 are not read
        if (mode != TZ_MODE_ABS)
            return tz_fail(ctx, TZ_ERR_INVALID, "%s: frame bounds are set (tz_set_frame_bounds), the mode must be abs, not %d", who, mode);
        if ((int)ctx->frame_bounds.size() != ctx->nt)
            return tz_fail(ctx, TZ_ERR_INVALID, "%s: frame bounds are set for %d frames (tz_set_frame_bounds), the rollout has %d", who,
                           (int)ctx->frame_bounds.size(), ctx->nt);
    }
    if (ctx->map_h) {   // tz_set_bound_map: b0 and b1 are not read
        if (mode != TZ_MODE_ABS)
            return tz_fail(ctx, TZ_ERR_INVALID, "%s: a bound map is set (tz_set_bound_map), the mode must be abs, not %d", who, mode);
        if (ctx->map_h != ctx->H || ctx->map_w != ctx->W)
            return tz_fail(ctx, TZ_ERR_INVALID, "%s: the bound map is %d x %d (tz_set_bound_map), the rollout's frames are %d x %d: a map has the frames' own size",
                           who, ctx->map_h, ctx->map_w, ctx->H, ctx->W);
    }
    return TZ_OK;
}

// TZ-CL1: the predictions of a closed loop (tz_rollout_closed) depend on what its job decodes to, so they serve that job alone:
// the loop's mode, bound and quantiser, one bound for every sample and the three-channel payload.
static int loop_check(tz_ctx* ctx, const char* who, int mode, double b0, double b1) {
    if (!ctx->loop_closed) return TZ_OK;
    if (ctx->loop_select != ctx->pred_select)   // TZ-PS1: chosen tiles are expressed in the predictions, or they are not
        return tz_fail(ctx, TZ_ERR_STATE,
                       "%s: the resident predictions are those of a closed loop (tz_rollout_closed) run %s per-tile selection "
                       "(tz_set_pred_select(%d)); they serve that kind of job alone, the setting is now %d",
                       who, ctx->loop_select ? "with" : "without", ctx->loop_select, ctx->pred_select);
    if (ctx->loop_motion != ctx->pred_motion)   // TZ-PM1: likewise
        return tz_fail(ctx, TZ_ERR_STATE,
                       "%s: the resident predictions are those of a closed loop (tz_rollout_closed) run %s motion-compensated tiles "
                       "(tz_set_pred_motion(%d)); they serve that kind of job alone, the setting is now %d",
                       who, ctx->loop_motion ? "with" : "without", ctx->loop_motion, ctx->pred_motion);
    if (ctx->loop_map) {   // TZ-CLM1: every pixel was decoded under its own bound; the job is the one under exactly that map
        const bool same_map = ctx->map_h == ctx->loop_map_h && ctx->map_w == ctx->loop_map_w && ctx->map_host == ctx->loop_map_bytes;
        if (mode == TZ_MODE_ABS && ctx->quantiser == 1 && same_map && ctx->frame_bounds.empty() && ctx->payload_channels == 3) return TZ_OK;
        return tz_fail(ctx, TZ_ERR_STATE,
                       "%s: the resident predictions are those of a closed loop run under one abs bound per pixel "
                       "(tz_rollout_closed_map); they serve the abs job of the lattice quantiser (tz_set_quantiser(1)) under "
                       "tz_set_bound_map with exactly that %d x %d map alone, not mode %d, quantiser %d, %s%s%s",
                       who, ctx->loop_map_h, ctx->loop_map_w, mode, ctx->quantiser,
                       !ctx->map_h ? "no bound map" : (same_map ? "that map" : "another bound map"),
                       ctx->frame_bounds.empty() ? "" : ", frame bounds (tz_set_frame_bounds)",
                       ctx->payload_channels == 3 ? "" : ", a one-channel payload (tz_set_payload_channels)");
    }
    if (ctx->loop_frames) {   // TZ-CLF1: every frame was decoded under its own bound; the job is the one under exactly those bounds
        if (mode == TZ_MODE_ABS && ctx->quantiser == 1 && ctx->frame_bounds == ctx->loop_bounds && !ctx->map_h && ctx->payload_channels == 3)
            return TZ_OK;
        return tz_fail(ctx, TZ_ERR_STATE,
                       "%s: the resident predictions are those of a closed loop run under one abs bound per frame "
                       "(tz_rollout_closed_frames); they serve the abs job of the lattice quantiser (tz_set_quantiser(1)) under "
                       "tz_set_frame_bounds with exactly those %d bounds (tz_loop_frame_bounds) alone, not mode %d, quantiser %d, %s%s%s",
                       who, (int)ctx->loop_bounds.size(), mode, ctx->quantiser,
                       ctx->frame_bounds.empty() ? "no frame bounds" : (ctx->frame_bounds == ctx->loop_bounds ? "those bounds" : "other frame bounds"),
                       ctx->map_h ? ", a bound map (tz_set_bound_map)" : "",
                       ctx->payload_channels == 3 ? "" : ", a one-channel payload (tz_set_payload_channels)");
    }
    const bool same = mode == ctx->loop_mode && b0 == ctx->loop_b0 && (mode != TZ_MODE_ABSREL || b1 == ctx->loop_b1) &&
                      ctx->quantiser == ctx->loop_quantiser;
    if (same && ctx->frame_bounds.empty() && !ctx->map_h && ctx->payload_channels == 3) return TZ_OK;
    return tz_fail(ctx, TZ_ERR_STATE,
                   "%s: the resident predictions are those of a closed loop (tz_rollout_closed) run with mode %d, bound %.17g (%.17g) and "
                   "quantiser %d; they serve that job alone, not mode %d, bound %.17g (%.17g), quantiser %d%s%s%s",
                   who, ctx->loop_mode, ctx->loop_b0, ctx->loop_b1, ctx->loop_quantiser, mode, b0, b1, ctx->quantiser,
                   ctx->frame_bounds.empty() ? "" : ", frame bounds (tz_set_frame_bounds)", ctx->map_h ? ", a bound map (tz_set_bound_map)" : "",
                   ctx->payload_channels == 3 ? "" : ", a one-channel payload (tz_set_payload_channels)");
}

// encode_check with the bound: what tz_encode and the probes check (the loop's rule comes first: it concerns the setters, whose own
// refusals would otherwise hide it; tz_encode_begin, tz_encode_delta and tz_size_probe call loop_check ahead of their layout checks)
static int encode_check(tz_ctx* ctx, const char* who, int mode, double b0, double b1) {
    TZ_TRY(loop_check(ctx, who, mode, b0, b1));
    return encode_check(ctx, who, mode);
}

// ---- one abs bound per frame (include/tezip_hip.h: tz_set_frame_bounds)
extern "C" int tz_set_frame_bounds(tz_ctx* ctx, const double* bounds, int n) {
    if (!ctx) return TZ_ERR_INVALID;
    if (n < 0) return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_frame_bounds: %d bounds", n);
    if (ctx->map_h && bounds && n > 0)
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_frame_bounds while a bound map is set (tz_set_bound_map): a job takes one of the two");
    if (!bounds || n == 0) {
        ctx->frame_bounds.clear();
        return TZ_OK;
    }
    for (int f = 0; f < n; ++f)
        if (!std::isfinite(bounds[f]) || bounds[f] < 0.0)
            return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_frame_bounds: bound %g of frame %d is not a finite number >= 0", bounds[f], f);
    ctx->frame_bounds.assign(bounds, bounds + n);
    return TZ_OK;
}

extern "C" int tz_get_frame_bounds(tz_ctx* ctx) { return ctx ? (int)ctx->frame_bounds.size() : TZ_ERR_INVALID; }

// ---- one abs bound per pixel, TZ-BM1 (include/tezip_hip.h: tz_set_bound_map)
extern "C" int tz_set_bound_map(tz_ctx* ctx, const uint8_t* map, int H, int W) {
    if (!ctx) return TZ_ERR_INVALID;
    if (!map) {
        if (ctx->map_h) ctx->enc_kind = tz_ctx::ENC_NONE;   // a resident payload was made under the map
        ctx->map_h = ctx->map_w = ctx->map_max = 0;
        ctx->map_host.clear();
        return TZ_OK;
    }
    if (H < 1 || W < 1) return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_bound_map: a map of %d x %d", H, W);
    if (!ctx->frame_bounds.empty())
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_bound_map while frame bounds are set (tz_set_frame_bounds): a job takes one of the two");
    const size_t n = (size_t)H * W;
    if (!ctx->d_bound_map || (size_t)ctx->map_h * ctx->map_w < n) {   // the one copy: H * W bytes for every frame and channel
        uint8_t* d = nullptr;
        TZ_HIP(ctx, hipMalloc((void**)&d, n));
        if (ctx->d_bound_map) {
            TZ_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (a launch may still read the old map)
            (void)hipFree(ctx->d_bound_map);
        }
        ctx->d_bound_map = d;
        ctx->map_h = ctx->map_w = ctx->map_max = 0;
    }
    TZ_TRY(tz_h2d(ctx, ctx->d_bound_map, map, n, ctx->stream));
    TZ_TRY(tz_stream_sync(ctx));   // (the caller's buffer is free on return)
    int mx = 0;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, (int)map[i]);
    ctx->map_h = H;
    ctx->map_w = W;
    ctx->map_max = mx;
    ctx->map_host.assign(map, map + n);   // (what a tz_rollout_closed_map stamps its loop with)
    ctx->enc_kind = tz_ctx::ENC_NONE;   // a resident payload was made under another tolerance
    return TZ_OK;
}

extern "C" int tz_get_bound_map(tz_ctx* ctx, int* H, int* W) {
    if (!ctx) return TZ_ERR_INVALID;
    if (H) *H = ctx->map_h;
    if (W) *W = ctx->map_w;
    return ctx->map_h ? 1 : 0;
}

// The sharded entry points and the size probe take one bound per job.
static int no_bound_map(tz_ctx* ctx, const char* who) {
    if (ctx->map_h)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "%s does not serve a bound map (tz_set_bound_map): sharded jobs and the size probe take one bound", who);
    return TZ_OK;
}

// The sharded entry points quantise one shard's frames under one bound.
static int no_frame_bounds(tz_ctx* ctx, const char* who) {
    if (!ctx->frame_bounds.empty())
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "%s does not serve per-frame bounds (tz_set_frame_bounds): sharded jobs take one bound", who);
    return TZ_OK;
}

// every frame's bound leaves its deltas as they are (0, or an identity by tz_quant_is_identity): the lossless job
static bool frame_bounds_identity(const tz_ctx* ctx) {
    for (double b : ctx->frame_bounds)
        if (b != 0.0 && !(ctx->quantiser == 1 ? tz_lattice_is_identity(TZ_MODE_ABS, b, 0.0) : tz_quant_is_identity(TZ_MODE_ABS, b, 0.0))) return false;
    return true;
}

// ---- the quantiser of a lossy job (include/tezip_hip.h: tz_set_quantiser)
extern "C" int tz_set_quantiser(tz_ctx* ctx, int q) {
    if (!ctx) return TZ_ERR_INVALID;
    if (q != 0 && q != 1) return tz_fail(ctx, TZ_ERR_INVALID, "quantiser must be 0 (greedy) or 1 (lattice, TZ-QL1), not %d", q);
    if (q != ctx->quantiser) ctx->enc_kind = tz_ctx::ENC_NONE;   // a resident payload was made by the other quantiser
    ctx->quantiser = q;
    return TZ_OK;
}

extern "C" int tz_get_quantiser(tz_ctx* ctx) { return ctx ? ctx->quantiser : TZ_ERR_INVALID; }

// The sharded entry points run the reference's quantiser.
static int greedy_only(tz_ctx* ctx, const char* who) {
    if (ctx->quantiser != 0)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "%s does not serve the lattice quantiser (tz_set_quantiser(1)): sharded jobs are out of scope", who);
    return TZ_OK;
}

// compress.py:315-319 on the delta stack of the context's rollout, under the frame bounds when some are set (encode_check has
// passed)
static int quantise_rollout(tz_ctx* ctx, int16_t* d_q, int mode, double b0, double b1) {
    const int nt = ctx->nt, H = ctx->H, W = ctx->W;
    if (ctx->map_h) {   // TZ-BM1 (tz_set_bound_map): a map of zeros leaves every delta as it is
        if (ctx->map_max == 0) return TZ_OK;
        if (ctx->quantiser == 1)
            return tzk_lattice(ctx, ctx->d_frames, d_q, ctx->quant_skip.data(), nt, H, W, TZ_MODE_ABS, 0.0, 0.0, nullptr, ctx->d_bound_map);
        return tzk_quant_map(ctx, ctx->d_frames, d_q, nullptr, ctx->quant_skip.data(), nt, H, W, ctx->d_bound_map, nullptr);
    }
    if (ctx->quantiser == 1)   // TZ-QL1 (tz_set_quantiser): one pass over the stack in place
        return tzk_lattice(ctx, ctx->d_frames, d_q, ctx->quant_skip.data(), nt, H, W, mode, b0, b1,
                           ctx->frame_bounds.empty() ? nullptr : ctx->frame_bounds.data());
    if (ctx->frame_bounds.empty()) return tzk_error_bound(ctx, ctx->d_frames, d_q, ctx->quant_skip.data(), nt, H, W, mode, b0, b1);
    return tzk_quant_frames(ctx, ctx->d_frames, d_q, nullptr, ctx->quant_skip.data(), nt, H, W, ctx->frame_bounds.data(), nullptr);
}

// compress.py:292-355 on the context-resident rollout: delta, quantiser, spatial delta over the whole flattened stack
// (no carry), 1600 offset + bincount when `entropy`.  d_sym receives the symbols (or the raw spatial delta) of the layout,
// nt * tz_frame_elems of them, d_hist the counters (zeroed here), d_edge[0..1] the first and the last element of the quantised
// delta stack (what a shard boundary needs; channel 0's under the gray layout, nothing under the channel
// stride).  d_delta_tap (may be NULL): the quantised delta stack, three channels in every layout, is also wanted there.
// d_sym NULL: stop after the quantiser (compress.py:292-319), the delta stack in d_delta_tap is all that is wanted.
static int encode_front(tz_ctx* ctx, tz_layout layout, int mode, double b0, double b1, int entropy, int16_t* d_delta_tap, int16_t* d_sym,
                        unsigned long long* d_hist, int16_t* d_edge) {
    const int nt = ctx->nt, H = ctx->H, W = ctx->W;
    const size_t N = (size_t)nt * H * W * 3;
    const bool flat = layout.channels == 3 && layout.stride == 1 && !layout.plane_h;   // (plane: the unfused chain in every mode)
    void *d_mask = nullptr, *d_delta = d_delta_tap;
    TZ_TRY(tz_pool_alloc(ctx, nt, &d_mask));
    TZ_TRY(tz_upload(ctx, d_mask, ctx->group_first.data(), nt));
    if (entropy) TZ_HIP(ctx, hipMemsetAsync(d_hist, 0, TZ_NBINS * sizeof(unsigned long long), ctx->stream));
    if (ctx->quantiser == 1 && d_sym && !d_delta_tap) {
        // TZ-QL1 (tz_set_quantiser): a job whose worst-case tolerance is below 1 is the lossless job and takes its kernels (the
        // flat one-pass front below, or the unfused chain, whose quantiser step then launches nothing); every other job has
        // one fused pass in EVERY layout -- the quantised value is a function of one delta and one tolerance.
        // Under a bound map (tz_set_bound_map) the same pass takes e from the map; a map of zeros is the lossless job.
        const bool per_frame = !ctx->frame_bounds.empty(), mapped = ctx->map_h != 0;
        const bool lossless = mapped ? ctx->map_max == 0 : (per_frame ? frame_bounds_identity(ctx) : tz_lattice_is_identity(mode, b0, b1));
        bool fused = false;
        if (!lossless)
            TZ_TRY(tzk_lattice_sd_fused(ctx, layout, ctx->d_pred, ctx->d_frames, (const uint8_t*)d_mask, ctx->quant_skip.data(), nt, H, W,
                                        ctx->Hp, ctx->Wp, mode, b0, b1, per_frame ? ctx->frame_bounds.data() : nullptr, entropy ? 1 : 0,
                                        d_sym, entropy ? d_hist : nullptr, d_edge, &fused, mapped ? ctx->d_bound_map : nullptr));
        else if (flat)
            TZ_TRY(tzk_delta_sd_fused(ctx, ctx->d_pred, ctx->d_frames, (const uint8_t*)d_mask, nt, H, W, ctx->Hp, ctx->Wp,
                                      entropy ? 1 : 0, d_sym, entropy ? d_hist : nullptr, d_edge, &fused));
        if (fused) return TZ_OK;
    } else if (flat && !d_delta_tap) {   // nobody asked for the delta stack: one of the two fused passes, where its kernel applies
        // error_bound returns its input untouched in these cases (compress.py:24,35), and COMPUTES its input back wherever
        // the worst-case tolerance of the job cannot merge two different deltas (E <= 0.499: tz_quant_is_identity, with the
        // proof).  A caller that taps the delta stack still gets it through the general quantiser (the parity tests compare
        // the two).  The gray layout and the channel stride have no fused pass.
        // Frame bounds (tz_set_frame_bounds): the lossless job when every frame's bound is such a one, else the same lossy
        // front with the per-frame tolerances.
        // A bound map (tz_set_bound_map): the lossless job when the map is zero everywhere, else the same lossy front with the
        // map as the walks' tolerance source.
        const bool per_frame = !ctx->frame_bounds.empty(), mapped = ctx->map_h != 0;
        const bool lossless = mapped      ? ctx->map_max == 0
                              : per_frame ? frame_bounds_identity(ctx)
                                          : b0 == 0.0 || (mode == TZ_MODE_ABSREL && b1 == 0.0) || tz_quant_is_identity(mode, b0, b1);
        bool fused = false;
        if (lossless)   // delta and spatial delta in one pass (compress.py:292-355)
            TZ_TRY(tzk_delta_sd_fused(ctx, ctx->d_pred, ctx->d_frames, (const uint8_t*)d_mask, nt, H, W, ctx->Hp, ctx->Wp,
                                      entropy ? 1 : 0, d_sym, entropy ? d_hist : nullptr, d_edge, &fused));
        else if (mapped) {
            const tz_quant_fused fu{ctx->d_pred, (const uint8_t*)d_mask, ctx->Hp, ctx->Wp, entropy ? 1 : 0, d_sym, entropy ? d_hist : nullptr, d_edge};
            TZ_TRY(tzk_quant_map(ctx, ctx->d_frames, nullptr, &fu, ctx->quant_skip.data(), nt, H, W, ctx->d_bound_map, &fused));
        } else if (per_frame) {
            const tz_quant_fused fu{ctx->d_pred, (const uint8_t*)d_mask, ctx->Hp, ctx->Wp, entropy ? 1 : 0, d_sym, entropy ? d_hist : nullptr, d_edge};
            TZ_TRY(tzk_quant_frames(ctx, ctx->d_frames, nullptr, &fu, ctx->quant_skip.data(), nt, H, W, ctx->frame_bounds.data(), &fused));
        } else          // quantiser on pred / orig, fill fused with the spatial delta
            TZ_TRY(tzk_quant_sd_fused(ctx, ctx->d_pred, ctx->d_frames, (const uint8_t*)d_mask, ctx->quant_skip.data(), nt, H, W,
                                      ctx->Hp, ctx->Wp, mode, b0, b1, entropy ? 1 : 0, d_sym, entropy ? d_hist : nullptr, d_edge,
                                      &fused));
        if (fused) return TZ_OK;
    }
    if (!d_delta) TZ_TRY(tz_pool_alloc(ctx, N * 2, &d_delta));
    // compress.py:292-314
    TZ_TRY(tzk_delta(ctx, ctx->d_pred, ctx->d_frames, (const uint8_t*)d_mask, nt, H, W, ctx->Hp, ctx->Wp, (int16_t*)d_delta));
    // compress.py:315-319 (under the gray layout the quantiser also walks channels 1 and 2, whose output is dropped)
    TZ_TRY(quantise_rollout(ctx, (int16_t*)d_delta, mode, b0, b1));
    if (!d_sym) return TZ_OK;
    // compress.py:339-355
    TZ_TRY(tzk_spatial_delta(ctx, layout, (const int16_t*)d_delta, (size_t)nt * tz_frame_elems(layout, H, W), nullptr, entropy ? 1 : 0,
                             d_sym, entropy ? d_hist : nullptr, d_edge));
    if (flat) {   // (k_sdelta_gray leaves the edge elements itself)
        TZ_HIP(ctx, hipMemcpyAsync(d_edge, d_delta, 2, hipMemcpyDeviceToDevice, ctx->stream));
        TZ_HIP(ctx, hipMemcpyAsync(d_edge + 1, (const int16_t*)d_delta + (N - 1), 2, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return TZ_OK;
}

// compress.py:356-373 from the N symbols of encode_front to the payload `o`, which joins the call's outputs to leave.  carry (may be
// NULL): the previous shard's last delta element, with which the first symbol of a tz_encode_begin is made again.  lut
// (NULL: none): the rank remap, by remap_out (in place when o is d_sym itself); else the symbols are copied unless
// they are already in o.  o_shuffled (may be NULL): the payload leaves from there, as the byte planes of o.
static int encode_tail(tz_call& call, int16_t* d_sym, size_t N, const int16_t* carry, const int16_t* lut, tz_out* o,
                       tz_out* o_shuffled, bool defer) {
    tz_ctx* ctx = call.ctx;
    if (carry) {   // sd = carry - x[0] instead of x[0] (compress.py:73-77 across the boundary)
        const int16_t sd = (int16_t)(*carry - ctx->enc_first);
        const int16_t y = ctx->enc_entropy ? (int16_t)(TZ_OFFSET - sd) : sd;
        TZ_TRY(tz_upload(ctx, d_sym, &y, 2));
    }
    if (lut) {
        TZ_TRY(remap_out(ctx, d_sym, N, lut, o, defer));  // compress.py:369
    } else if (o->dev != d_sym) {
        hipError_t e = hipMemcpyAsync(o->dev, d_sym, N * 2, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "payload copy: %s", hipGetErrorString(e));
    }
    if (o_shuffled) {
        TZ_TRY(tzk_shuffle(ctx, (const int16_t*)o->dev, N, (uint8_t*)o_shuffled->dev, 0));
        o = o_shuffled;
    }
    call.outs.push_back(*o);
    return call.finish();
}

// ---- one-channel payload of a gray job (include/tezip_hip.h: tz_set_payload_channels)
extern "C" int tz_set_payload_channels(tz_ctx* ctx, int channels) {
    if (!ctx) return TZ_ERR_INVALID;
    if (channels != 1 && channels != 3) return tz_fail(ctx, TZ_ERR_INVALID, "payload channels must be 3 or 1, not %d", channels);
    if (channels != ctx->payload_channels) ctx->enc_kind = tz_ctx::ENC_NONE;   // a resident payload was made for the other count
    ctx->payload_channels = channels;
    return TZ_OK;
}

extern "C" int tz_get_payload_channels(tz_ctx* ctx) { return ctx ? ctx->payload_channels : TZ_ERR_INVALID; }

// ---- spatial delta at the channel stride (include/tezip_hip.h: tz_set_delta_stride)
extern "C" int tz_set_delta_stride(tz_ctx* ctx, int mode) {
    if (!ctx) return TZ_ERR_INVALID;
    if (mode != 0 && mode != 1) return tz_fail(ctx, TZ_ERR_INVALID, "delta stride mode must be 0 (flat) or 1 (channel), not %d", mode);
    if (mode == 1 && ctx->delta_plane)
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_delta_stride(1) while tz_set_delta_plane(1) is in force: a payload has one spatial delta");
    if (mode != ctx->delta_stride_mode) ctx->enc_kind = tz_ctx::ENC_NONE;   // a resident payload was made under the other stride
    ctx->delta_stride_mode = mode;
    return TZ_OK;
}

extern "C" int tz_get_delta_stride(tz_ctx* ctx) { return ctx ? ctx->delta_stride_mode : TZ_ERR_INVALID; }

// ---- 2-D spatial delta of the payload, TZ-SD2 (include/tezip_hip.h: tz_set_delta_plane)
extern "C" int tz_set_delta_plane(tz_ctx* ctx, int on) {
    if (!ctx) return TZ_ERR_INVALID;
    if (on != 0 && on != 1) return tz_fail(ctx, TZ_ERR_INVALID, "delta plane must be 0 (off) or 1 (TZ-SD2), not %d", on);
    if (on == 1 && ctx->delta_stride_mode == 1)
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_delta_plane(1) while tz_set_delta_stride(1) is in force: a payload has one spatial delta");
    if (on != ctx->delta_plane) ctx->enc_kind = tz_ctx::ENC_NONE;   // a resident payload was made under the other predictor
    ctx->delta_plane = on;
    return TZ_OK;
}

extern "C" int tz_get_delta_plane(tz_ctx* ctx) { return ctx ? ctx->delta_plane : TZ_ERR_INVALID; }

// the layout in force (tz_internal.h): mode 1 on a one-channel payload is the flat delta; plane fills the frame's rows and
// columns from the context (with plane off the layout is what it was: every launcher chooses what it chose)
static const tz_layout kFlat = {3, 1};
static tz_layout layout_of(const tz_ctx* ctx) {
    tz_layout l = {ctx->payload_channels, ctx->delta_stride_mode == 1 && ctx->payload_channels == 3 ? 3 : 1};
    if (ctx->delta_plane) {
        l.plane_h = ctx->H;
        l.plane_w = ctx->W;
    }
    return l;
}

// The entry points that serve no plane payload: sharded jobs, carries (a plane frame is coded on its own) and tz_size_probe
// (tz_sdelta_probe sizes the plane payload, next to the other two, whatever the setting).
static int no_plane(tz_ctx* ctx, const char* who) {
    if (ctx->delta_plane)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "%s does not serve the 2-D spatial delta (tz_set_delta_plane(1)): sharded jobs, carries and the size probe are out of its scope", who);
    return TZ_OK;
}

// The entry points of the sharded encoder / decoder serve the flat layout alone: not a one-channel payload, and one carry
// element is not the carry of a strided scan.  (tz_undelta_carry serves a gray payload: its carry is one element.)
// (tz_encode_delta serves a plane job: the quantised delta stack does not depend on the spatial delta.)
static int flat_only(tz_ctx* ctx, const char* who, bool serves_gray = false, bool serves_plane = false) {
    if (ctx->payload_channels == 1 && !serves_gray)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "%s does not serve a one-channel payload (tz_set_payload_channels(1)): sharded gray jobs are not supported", who);
    if (ctx->delta_stride_mode == 1)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "%s does not serve the channel-stride spatial delta (tz_set_delta_stride(1)): sharded jobs and one-element carries are flat only", who);
    if (serves_plane) return TZ_OK;
    return no_plane(ctx, who);
}

static int keys_gray(tz_ctx* ctx, const int* idx, int nkeys, uint8_t* gray);   // (k_key_gray: with the key-frame coders below)

// TZ_ERR_INVALID naming the first frame of the resident stack that has a pixel with unequal channels (k_key_gray over all frames)
static int encode_all_gray(tz_ctx* ctx) {
    const int nt = ctx->nt;
    std::vector<int> idx(nt);
    for (int i = 0; i < nt; ++i) idx[i] = i;
    std::vector<uint8_t> gray(nt);
    TZ_TRY(keys_gray(ctx, idx.data(), nt, gray.data()));
    for (int i = 0; i < nt; ++i)
        if (!gray[i]) return tz_fail(ctx, TZ_ERR_INVALID, "tz_encode: frame %d has colour, a one-channel payload would drop it", i);
    return TZ_OK;
}

extern "C" int tz_encode(tz_ctx* ctx, int mode, double b0, double b1, int entropy, int16_t* payload, int16_t* table,
                         int* table_len, int16_t* delta_out) {
    tz_roctx_range roctx_("tz_encode");
    if (!ctx || !table_len || ((entropy & 1) && !table)) return TZ_ERR_INVALID;
    TZ_TRY(encode_check(ctx, "tz_encode", mode, b0, b1));
    const tz_layout layout = layout_of(ctx);
    if (layout.channels == 1) {
        if (delta_out) return tz_fail(ctx, TZ_ERR_INVALID, "tz_encode: no delta_out with a one-channel payload");
        tz_call gray_check(ctx);   // (a scope of its own: the encode reuses its blocks)
        TZ_TRY(encode_all_gray(ctx));
    }
    const size_t N = (size_t)ctx->nt * tz_frame_elems(layout, ctx->H, ctx->W);
    const bool shuffle = (entropy & 2) != 0;  // opt-in byte planes (not a reference format)
    entropy &= 1;
    if (shuffle && (N & 7)) return tz_fail(ctx, TZ_ERR_INVALID, "byte shuffle needs a multiple of 8 elements");
    ctx->enc_kind = tz_ctx::ENC_NONE;
    const bool to_resident = payload == nullptr;
    if (to_resident) {  // keep the payload in the context: it leaves through tz_payload_get
        TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_payload, &ctx->cap_payload, N * 2));
        ctx->payload_len = N;
        payload = ctx->d_payload;
    }
    tz_call call(ctx);
    tz_out o_pay, o_plain{nullptr, nullptr, N * 2};
    tz_out* o = shuffle ? &o_plain : &o_pay;   // where the plain payload goes (scratch when it is shuffled into o_pay)
    // a transfer of the call before may still be reading the staging buffer (and writing the caller's previous host
    // buffer): it has ~a rollout's time to finish, and must have before this call's remap writes the buffer again
    const bool defer = ctx->defer_payload && entropy && !shuffle && tz_ptr_kind(payload) == 1;
    if (ctx->payload_inflight) {
        if (defer) {
            hipError_t e = hipStreamWaitEvent(ctx->stream, ctx->ev_payload, 0);
            if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "hipStreamWaitEvent: %s", hipGetErrorString(e));
        } else {
            TZ_TRY(tz_payload_settle(ctx));
        }
    }
    if (defer) {
        if (ctx->cap_payload_stage < N * 2) TZ_TRY(tz_payload_settle(ctx));   // (growing frees the old buffer)
        TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_payload_stage, &ctx->cap_payload_stage, N * 2));
        o_pay = tz_out{payload, ctx->d_payload_stage, N * 2};
    } else {
        TZ_TRY(tz_dev_out(ctx, payload, N * 2, &o_pay));   // (joins the outputs last, in encode_tail)
    }
    if (shuffle) TZ_TRY(call.alloc(N * 2, &o_plain.dev));
    int16_t *d_delta = nullptr, *d_edge = nullptr, *d_sd = nullptr;
    unsigned long long* d_hist = nullptr;
    if (delta_out) TZ_TRY(call.out(delta_out, N * 2, &d_delta));
    TZ_TRY(call.alloc(16, &d_edge));
    if (entropy) {
        TZ_TRY(call.alloc(TZ_NBINS * sizeof(unsigned long long), &d_hist));
        TZ_TRY(call.alloc(N * 2, &d_sd));
    }
    int16_t* d_sym = entropy ? d_sd : (int16_t*)o->dev;   // without a table the symbols are the payload
    TZ_TRY(encode_front(ctx, layout, mode, b0, b1, entropy, d_delta, d_sym, d_hist, d_edge));
    std::vector<int16_t> lut;
    if (!entropy) {
        *table_len = -1;
    } else {
        std::vector<unsigned long long> hist(TZ_NBINS, 0);
        hipError_t e = hipMemcpyAsync(hist.data(), d_hist, TZ_NBINS * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "hist download: %s", hipGetErrorString(e));
        const auto t0 = std::chrono::steady_clock::now();
        TZ_TRY(tz_build_table(hist.data(), TZ_NBINS, table, table_len));  // 356-361
        TZ_TRY(build_enc_lut(ctx, table, *table_len, &lut));
        if (ctx->prof_on) {
            ctx->prof[TZP_TABLE].total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            ctx->prof[TZP_TABLE].launches += 1;
        }
    }
    TZ_TRY(encode_tail(call, d_sym, N, nullptr, entropy ? lut.data() : nullptr, o, shuffle ? &o_pay : nullptr, defer));
    if (to_resident) ctx->enc_kind = tz_ctx::ENC_PAYLOAD;   // (tz_encode_quality's payload == NULL)
    return TZ_OK;
}
// ---- tz_encode in two phases, for jobs whose frame windows are sharded over GPUs.  The spatial delta
// runs over the WHOLE flattened stack (compress.py:339) and the rank table comes from the GLOBAL histogram
// (compress.py:354-361): a shard runs encode_front into the context's resident payload buffer (begin), the ranks exchange
// one carry element and sum 2111 counters, and the shard runs encode_tail with the global table (finish).  tz_encode is
// the one-shard case.
extern "C" int tz_encode_begin(tz_ctx* ctx, int mode, double b0, double b1, int entropy, unsigned long long* hist,
                               int16_t* edge) {
    tz_roctx_range roctx_("tz_encode_begin");
    if (!ctx || !edge || (entropy && !hist)) return TZ_ERR_INVALID;
    TZ_TRY(loop_check(ctx, "tz_encode_begin", mode, b0, b1));
    TZ_TRY(flat_only(ctx, "tz_encode_begin"));
    TZ_TRY(no_frame_bounds(ctx, "tz_encode_begin"));
    TZ_TRY(no_bound_map(ctx, "tz_encode_begin"));
    TZ_TRY(greedy_only(ctx, "tz_encode_begin"));
    TZ_TRY(encode_check(ctx, "tz_encode_begin", mode));
    ctx->enc_kind = tz_ctx::ENC_NONE;   // d_payload now receives a shard's symbols
    const size_t N = (size_t)ctx->nt * ctx->H * ctx->W * 3;
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_payload, &ctx->cap_payload, N * 2));
    ctx->payload_len = N;
    tz_call call(ctx);
    unsigned long long* d_hist = nullptr;
    int16_t* d_edge = nullptr;
    TZ_TRY(call.alloc(16, &d_edge));
    if (entropy) TZ_TRY(call.alloc(TZ_NBINS * sizeof(unsigned long long), &d_hist));
    TZ_TRY(encode_front(ctx, kFlat, mode, b0, b1, entropy ? 1 : 0, nullptr, ctx->d_payload, d_hist, d_edge));
    hipError_t e = hipMemcpyAsync(edge, d_edge, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && entropy)
        e = hipMemcpyAsync(hist, d_hist, TZ_NBINS * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "tz_encode_begin: %s", hipGetErrorString(e));
    ctx->enc_kind = tz_ctx::ENC_SYMBOLS;
    ctx->enc_entropy = entropy != 0;
    ctx->enc_first = edge[0];
    return TZ_OK;
}

extern "C" int tz_encode_finish(tz_ctx* ctx, int has_carry, int16_t carry, const int16_t* table, int table_len,
                                int16_t* payload) {
    tz_roctx_range roctx_("tz_encode_finish");
    if (!ctx) return TZ_ERR_INVALID;
    TZ_TRY(flat_only(ctx, "tz_encode_finish"));
    TZ_TRY(no_frame_bounds(ctx, "tz_encode_finish"));
    TZ_TRY(no_bound_map(ctx, "tz_encode_finish"));
    TZ_TRY(greedy_only(ctx, "tz_encode_finish"));
    if (ctx->enc_kind != tz_ctx::ENC_SYMBOLS) return tz_fail(ctx, TZ_ERR_STATE, "tz_encode_finish needs a tz_encode_begin first");
    if (ctx->enc_entropy != (table_len >= 0) || (table_len > 0 && !table) || table_len > TZ_MAX_TABLE)
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_encode_finish: table does not match the entropy flag of tz_encode_begin");
    const size_t N = ctx->payload_len;
    if (!whole_stack(ctx, tz_ctx::ROLLOUT_ENCODE) || N != (size_t)ctx->nt * ctx->H * ctx->W * 3) {
        ctx->enc_kind = tz_ctx::ENC_NONE;
        return tz_fail(ctx, TZ_ERR_STATE, "tz_encode_finish: the resident symbols (%zu) are not those of the current rollout", N);
    }
    std::vector<int16_t> lut;
    if (ctx->enc_entropy) TZ_TRY(build_enc_lut(ctx, table, table_len, &lut));
    tz_call call(ctx);
    tz_out o{nullptr, ctx->d_payload};   // payload NULL: the symbols become the payload in place and stay resident
    if (payload) TZ_TRY(tz_dev_out(ctx, payload, N * 2, &o));   // (joins the outputs in encode_tail)
    TZ_TRY(encode_tail(call, ctx->d_payload, N, has_carry ? &carry : nullptr, ctx->enc_entropy ? lut.data() : nullptr, &o, nullptr, false));
    ctx->enc_kind = tz_ctx::ENC_NONE;
    return TZ_OK;
}

// Opt-in byte shuffle of an int16 stream and its inverse (stand-alone; tz_encode applies the
// forward direction itself when bit 1 of `entropy` is set).
extern "C" int tz_byte_shuffle(tz_ctx* ctx, const int16_t* in, size_t n, uint8_t* out) {
    if (!ctx || !in || !out) return TZ_ERR_INVALID;
    tz_call call(ctx);
    const int16_t* din;
    uint8_t* dout;
    TZ_TRY(call.in(in, n * 2, &din));
    TZ_TRY(call.out(out, n * 2, &dout));
    TZ_TRY(tzk_shuffle(ctx, (const int16_t*)din, n, (uint8_t*)dout, 0));
    return call.finish();
}

extern "C" int tz_byte_unshuffle(tz_ctx* ctx, const uint8_t* in, size_t n, int16_t* out) {
    if (!ctx || !in || !out) return TZ_ERR_INVALID;
    tz_call call(ctx);
    const uint8_t* din;
    int16_t* dout;
    TZ_TRY(call.in(in, n * 2, &din));
    TZ_TRY(call.out(out, n * 2, &dout));
    TZ_TRY(tzk_shuffle(ctx, (const int16_t*)din, n, (uint8_t*)dout, 1));
    return call.finish();
}

extern "C" int tz_encode_delta(tz_ctx* ctx, int mode, double b0, double b1, int16_t* delta_out) {
    if (!ctx || !delta_out) return TZ_ERR_INVALID;
    TZ_TRY(loop_check(ctx, "tz_encode_delta", mode, b0, b1));
    TZ_TRY(flat_only(ctx, "tz_encode_delta", false, true));
    TZ_TRY(encode_check(ctx, "tz_encode_delta", mode));
    const size_t N = (size_t)ctx->nt * ctx->H * ctx->W * 3;
    tz_call call(ctx);
    int16_t* d_delta;
    TZ_TRY(call.out(delta_out, N * 2, &d_delta));
    TZ_TRY(encode_front(ctx, kFlat, mode, b0, b1, 0, d_delta, nullptr, nullptr, nullptr));
    return call.finish();
}

extern "C" int tz_decode_delta(tz_ctx* ctx, const int16_t* delta, uint8_t* frames_out) {
    if (!ctx || !delta || !frames_out) return TZ_ERR_INVALID;
    TZ_TRY(flat_only(ctx, "tz_decode_delta"));
    if (!whole_stack(ctx, tz_ctx::ROLLOUT_DECODE)) return tz_fail(ctx, TZ_ERR_STATE, "tz_decode_delta needs a tz_rollout_decode first");
    TZ_TRY(tz_check_pred_contract(ctx, "tz_decode_delta"));
    const int nt = ctx->nt, H = ctx->H, W = ctx->W;
    const size_t N = (size_t)nt * H * W * 3;
    tz_call call(ctx);
    const int16_t* d_diff;
    uint8_t *d_out, *d_mask;
    TZ_TRY(call.in(delta, N * 2, &d_diff));
    TZ_TRY(call.out(frames_out, N, &d_out));
    TZ_TRY(call.alloc(nt, &d_mask));
    TZ_TRY(tz_upload(ctx, d_mask, ctx->key_mask.data(), nt));
    TZ_TRY(tzk_reconstruct(ctx, 3, ctx->d_pred, ctx->d_frames, d_mask, d_diff, nt, H, W, ctx->Hp, ctx->Wp, d_out));
    return call.finish();
}

// the `stride` decoded elements in front of payload[n0] (k_undelta_carry, k_undelta_carry_s3): enqueued, then read back
static int undelta_carry(tz_ctx* ctx, int stride, const int16_t* d_pay, size_t n0, const int16_t* h_lut, int16_t* carry) {
    void* d_words;
    unsigned w[3] = {0, 0, 0};
    TZ_TRY(tz_pool_alloc(ctx, stride * sizeof(unsigned), &d_words));
    TZ_TRY(tzk_undelta_carry(ctx, stride, d_pay, n0, h_lut, 1, (unsigned*)d_words));
    TZ_TRY(tz_d2h(ctx, w, d_words, stride * sizeof(unsigned), ctx->stream));
    TZ_TRY(tz_stream_sync(ctx));
    for (int c = 0; c < stride; ++c) carry[c] = (int16_t)(w[c] & 0xFFFFu);
    return TZ_OK;
}

// payload == NULL: the payload staged with tz_payload_begin / tz_payload_put, which must hold `need` elements
static int staged_payload(tz_ctx* ctx, size_t need, const int16_t** payload) {
    if (!ctx->d_payload || ctx->payload_len < need) return tz_fail(ctx, TZ_ERR_STATE, "no staged payload of %zu elements", need);
    TZ_HIP(ctx, hipEventRecord(ctx->ev_frames, ctx->copy_stream));
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_frames, 0));
    *payload = ctx->d_payload;
    return TZ_OK;
}

// table_len: -1 = no table (entropy remap off), else the length of the rank table
static int check_table(tz_ctx* ctx, const int16_t* table, int table_len) {
    if (table_len < -1 || table_len > TZ_NBINS || (table_len > 0 && !table)) return tz_fail(ctx, TZ_ERR_INVALID, "bad table");
    return TZ_OK;
}

// the body of tz_undelta_carry and tz_undelta_carry_stride, behind their own checks of the mode, the stride and n0
static int undelta_carry_seam(tz_ctx* ctx, int stride, const int16_t* payload, size_t n0, const int16_t* table, int table_len,
                              int16_t* carry) {
    TZ_TRY(check_table(ctx, table, table_len));
    if (!payload) TZ_TRY(staged_payload(ctx, n0, &payload));
    std::vector<int16_t> lut;
    if (table_len >= 0) build_dec_lut(table, table_len, 1, &lut);
    tz_call call(ctx);
    const int16_t* d_pay;
    TZ_TRY(call.in(payload, n0 * 2, &d_pay));
    return undelta_carry(ctx, stride, d_pay, n0, table_len >= 0 ? lut.data() : nullptr, carry);
}

extern "C" int tz_undelta_carry(tz_ctx* ctx, const int16_t* payload, size_t n0, const int16_t* table, int table_len,
                                int16_t* carry) {
    tz_roctx_range roctx_("tz_undelta_carry");
    if (!ctx || !carry) return TZ_ERR_INVALID;
    TZ_TRY(flat_only(ctx, "tz_undelta_carry", true));
    if (n0 == 0) return tz_fail(ctx, TZ_ERR_INVALID, "tz_undelta_carry: n0 = 0, the stream start has no carry");
    return undelta_carry_seam(ctx, 1, payload, n0, table, table_len, carry);
}

// Frames [first, first + count) of the stream (decompress.py:203-256): the carry of the inverse scan in front of the range
// when it does not start the stream, then the decoder's tail over the range.  The range lies inside the resident prediction
// stack; payload is the WHOLE stream, of which nothing behind the range is read.
static int decode_frames(tz_ctx* ctx, const char* who, const int16_t* payload, size_t payload_len, const int16_t* table,
                         int table_len, int first, int count, uint8_t* frames_out) {
    TZ_TRY(tz_check_pred_contract(ctx, who));
    TZ_TRY(check_table(ctx, table, table_len));
    const int nt = ctx->nt, H = ctx->H, W = ctx->W, r = ctx->pred_first;
    if (first < r || count < 1 || first >= ctx->pred_end || count > ctx->pred_end - first)
        return tz_fail(ctx, TZ_ERR_INVALID, "frame range [%d, %d + %d) outside the frames [%d, %d) the range rollout covered", first,
                       first, count, r, ctx->pred_end);
    // fe: bytes of a decoded frame; pe: payload elements of a frame (H*W of them under tz_set_payload_channels(1))
    const tz_layout layout = layout_of(ctx);
    const size_t fe = (size_t)H * W * 3, pe = tz_frame_elems(layout, H, W), N = (size_t)nt * pe, n0 = (size_t)first * pe,
                 np = (size_t)count * pe, nr = (size_t)count * fe;
    if (!payload) TZ_TRY(staged_payload(ctx, N, &payload));
    ctx->have_decoded = false;
    if (payload_len != N)  // decompress.py:240: the reshape raises
        return tz_fail(ctx, TZ_ERR_INVALID, "payload holds %zu elements, the key-frame stack implies %zu", payload_len, N);
    const bool resident = frames_out == nullptr;
    if (resident) {  // keep the frames in the context: tz_decoded_get (sequence coordinates)
        TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_out, &ctx->cap_out, nr));
        frames_out = ctx->d_out;
    }
    tz_call call(ctx);
    const int16_t* d_pay;
    uint8_t *d_out, *d_mask;
    int16_t carry[3] = {0, 0, 0};   // the layout.stride decoded elements in front of the range
    TZ_TRY(call.in(payload, n0 * 2 + np * 2, &d_pay));
    TZ_TRY(call.out(frames_out, nr, &d_out));
    TZ_TRY(call.alloc(count, &d_mask));
    TZ_TRY(tz_upload(ctx, d_mask, ctx->key_mask.data() + (first - r), count));
    std::vector<int16_t> lut;
    if (table_len >= 0) build_dec_lut(table, table_len, 1, &lut);
    const int16_t* h_lut = table_len >= 0 ? lut.data() : nullptr;
    const bool has_carry = first > 0 && !layout.plane_h;   // (a plane frame is coded on its own)
    if (has_carry) TZ_TRY(undelta_carry(ctx, layout.stride, d_pay, n0, h_lut, carry));
    TZ_TRY(tzk_decode_tail(ctx, layout, d_pay + n0, h_lut, 1, has_carry ? carry : nullptr,
                           ctx->d_pred + (size_t)(first - r) * ctx->Hp * ctx->Wp * 3, ctx->d_frames + (size_t)first * fe, d_mask, count, H,
                           W, ctx->Hp, ctx->Wp, d_out));
    TZ_TRY(call.finish());
    if (resident) {   // only a decode whose work is queued leaves frames to fetch
        ctx->have_decoded = true;
        ctx->dec_first = first;
        ctx->dec_count = count;
    }
    return TZ_OK;
}

extern "C" int tz_decode(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len,
                         uint8_t* frames_out) {
    tz_roctx_range roctx_("tz_decode");
    if (!ctx) return TZ_ERR_INVALID;
    if (!whole_stack(ctx, tz_ctx::ROLLOUT_DECODE)) return tz_fail(ctx, TZ_ERR_STATE, "tz_decode needs a tz_rollout_decode first");
    return decode_frames(ctx, "tz_decode", payload, payload_len, table, table_len, 0, ctx->nt, frames_out);
}

extern "C" int tz_decode_range(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len,
                               int first, int count, uint8_t* frames_out) {
    tz_roctx_range roctx_("tz_decode_range");
    if (!ctx) return TZ_ERR_INVALID;
    if (ctx->rollout_kind != tz_ctx::ROLLOUT_DECODE)
        return tz_fail(ctx, TZ_ERR_STATE, "tz_decode_range needs a tz_rollout_decode_range first");
    return decode_frames(ctx, "tz_decode_range", payload, payload_len, table, table_len, first, count, frames_out);
}

// ---- closed-loop prediction, definition TZ-CL1 (include/tezip_hip.h: tz_rollout_closed; slow statement in
// tezip_amd/closedloop.py).  The steps of a closed loop: step s holds the frames k + s of every key interval [k, next key) that
// still has one, so that step s reads what step s - 1 decoded (or the key frame itself).  key: the key mask of the sequence
// (frame 0 is a key frame).  Every frame of a step is an item "predict from the u8 frame in front" of run_schedule.
static std::vector<std::vector<int>> closed_steps(const std::vector<uint8_t>& key) {
    std::vector<std::vector<int>> steps;
    for (int t = 0, s = 0; t < (int)key.size(); ++t) {
        s = key[t] ? 0 : s + 1;
        if (!s) continue;
        if ((int)steps.size() < s) steps.resize(s);
        steps[s - 1].push_back(t);
    }
    return steps;
}

// one schedule over the frames `list`, each predicted from frame - 1 of the u8 stack `src`
static int closed_predict(tz_ctx* ctx, const std::vector<int>& list, const uint8_t* src) {
    std::vector<PredItem> items;
    for (int t : list) items.push_back(PredItem{t, 1, t - 1, 1});
    return run_schedule(ctx, items, src);
}

// the steps' frame lists, one after the other, on the device
static int closed_lists(tz_call& call, const std::vector<std::vector<int>>& steps, const int** d_lists) {
    std::vector<int> all;
    for (const auto& st : steps) all.insert(all.end(), st.begin(), st.end());
    int* d = nullptr;
    TZ_TRY(call.alloc(std::max<size_t>(all.size(), 1) * sizeof(int), &d));
    if (!all.empty()) TZ_TRY(tz_upload(call.ctx, d, all.data(), all.size() * sizeof(int)));
    *d_lists = d;
    return TZ_OK;
}

// ---- per-tile choice of the prediction, definition TZ-PS1 (include/tezip_hip.h: tz_set_pred_select; slow statement in
// tezip_amd/predselect.py): the mode bytes of a sequence, nt * ceil(H / 16) * ceil(W / 16), frame-major, row-major tiles
static size_t select_count(int nt, int H, int W) { return (size_t)nt * ((H + 15) / 16) * ((W + 15) / 16); }

// the mode bytes on the device: zero (the encoder's kernels write the tiles of the frames they choose for), or a decoder's
static int select_modes(tz_call& call, size_t n, const uint8_t* host, uint8_t** d_modes) {
    TZ_TRY(call.alloc(std::max<size_t>(n, 1), d_modes));
    if (host) return tz_upload(call.ctx, *d_modes, host, n);
    if (hipMemsetAsync(*d_modes, 0, n, call.ctx->stream) != hipSuccess) return tz_fail(call.ctx, TZ_ERR_HIP, "clearing the mode bytes failed");
    return TZ_OK;
}

extern "C" int tz_set_pred_select(tz_ctx* ctx, int on) {
    if (!ctx) return TZ_ERR_INVALID;
    if (on != 0 && on != 1) return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_pred_select takes 0 or 1, not %d", on);
    if (on && ctx->pred_motion)
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_pred_select(1) while tz_set_pred_motion(%d) is in force: a tile has one second candidate", ctx->pred_motion);
    if (on != ctx->pred_select) ctx->enc_kind = tz_ctx::ENC_NONE;   // a resident payload was made under the other setting
    ctx->pred_select = on;
    return TZ_OK;
}

extern "C" int tz_get_pred_select(tz_ctx* ctx) { return ctx ? ctx->pred_select : TZ_ERR_INVALID; }

extern "C" int tz_pred_modes(tz_ctx* ctx, uint8_t* out, size_t cap) {
    if (!ctx) return TZ_ERR_INVALID;
    if ((!ctx->loop_closed || !ctx->loop_motion) && ctx->pred_motion)   // (asked for under motion: say so; else the message as it was)
        return tz_fail(ctx, TZ_ERR_STATE, "tz_pred_modes: the resident rollout is no tz_rollout_closed under tz_set_pred_motion(7)");
    if (!ctx->loop_closed || (!ctx->loop_select && !ctx->loop_motion))
        return tz_fail(ctx, TZ_ERR_STATE, "tz_pred_modes: the resident rollout is no tz_rollout_closed under tz_set_pred_select(1)");
    const size_t n = ctx->pred_modes.size();
    if (!out || cap < n) return tz_fail(ctx, TZ_ERR_INVALID, "tz_pred_modes: room for %zu mode bytes, the rollout has %zu", out ? cap : (size_t)0, n);
    memcpy(out, ctx->pred_modes.data(), n);
    return TZ_OK;
}

extern "C" int tz_put_pred_modes(tz_ctx* ctx, const uint8_t* modes, size_t n) {
    if (!ctx) return TZ_ERR_INVALID;
    ctx->put_modes.clear();
    if (!modes || !n) return tz_fail(ctx, TZ_ERR_INVALID, "tz_put_pred_modes: no mode bytes");
    for (size_t i = 0; i < n; ++i)
        if (modes[i] > 1) return tz_fail(ctx, TZ_ERR_INVALID, "tz_put_pred_modes: mode byte %zu is %d, 0 or 1 wanted", i, (int)modes[i]);
    ctx->put_modes.assign(modes, modes + n);
    return TZ_OK;
}

// ---- motion-compensated tiles, definition TZ-PM1 (include/tezip_hip.h: tz_set_pred_motion; slow statement in
// tezip_amd/predmotion.py): TZ-PS1's mode bytes plus one vector (dy, dx) per tile, 2 * select_count int8
static int motion_vectors(tz_call& call, size_t n, const int8_t* host, int8_t** d_vecs) {
    TZ_TRY(call.alloc(std::max<size_t>(n, 1), d_vecs));
    if (host) return tz_upload(call.ctx, *d_vecs, host, n);
    if (hipMemsetAsync(*d_vecs, 0, n, call.ctx->stream) != hipSuccess) return tz_fail(call.ctx, TZ_ERR_HIP, "clearing the vectors failed");
    return TZ_OK;
}

extern "C" int tz_set_pred_motion(tz_ctx* ctx, int r) {
    if (!ctx) return TZ_ERR_INVALID;
    if (r != 0 && r != 7) return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_pred_motion takes 0 (off) or the search radius 7, not %d", r);
    if (r && ctx->pred_select)
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_set_pred_motion(%d) while tz_set_pred_select(1) is in force: a tile has one second candidate", r);
    if (r != ctx->pred_motion) ctx->enc_kind = tz_ctx::ENC_NONE;   // a resident payload was made under the other setting
    ctx->pred_motion = r;
    return TZ_OK;
}

extern "C" int tz_get_pred_motion(tz_ctx* ctx) { return ctx ? ctx->pred_motion : TZ_ERR_INVALID; }

extern "C" int tz_pred_vectors(tz_ctx* ctx, int8_t* out, size_t cap) {
    if (!ctx) return TZ_ERR_INVALID;
    if (!ctx->loop_closed || !ctx->loop_motion)
        return tz_fail(ctx, TZ_ERR_STATE, "tz_pred_vectors: the resident rollout is no tz_rollout_closed under tz_set_pred_motion(7)");
    const size_t n = ctx->pred_vectors.size();
    if (!out || cap < n) return tz_fail(ctx, TZ_ERR_INVALID, "tz_pred_vectors: room for %zu vector components, the rollout has %zu", out ? cap : (size_t)0, n);
    memcpy(out, ctx->pred_vectors.data(), n);
    return TZ_OK;
}

extern "C" int tz_put_pred_vectors(tz_ctx* ctx, const int8_t* vectors, size_t n) {
    if (!ctx) return TZ_ERR_INVALID;
    ctx->put_vectors.clear();
    if (!vectors || !n) return tz_fail(ctx, TZ_ERR_INVALID, "tz_put_pred_vectors: no vectors");
    for (size_t i = 0; i < n; ++i)
        if (vectors[i] < -7 || vectors[i] > 7)
            return tz_fail(ctx, TZ_ERR_INVALID, "tz_put_pred_vectors: component %zu is %d, -7 .. 7 wanted", i, (int)vectors[i]);
    ctx->put_vectors.assign(vectors, vectors + n);
    return TZ_OK;
}

// The loop of tz_rollout_closed and tz_rollout_closed_map behind their checks: the key mask and groups, the lossless job's one
// schedule or the steps, each decoded under E (d_map NULL) or under d_map[pixel], and the stamp both share.
static int closed_rollout(tz_ctx* ctx, const char* who, const uint8_t* frames, int nt, int H, int W, int warm_up, int window, bool lossless, int E,
                          const uint8_t* d_map, uint8_t* key_mask) {
    const int p = warm_up;
    const bool select = ctx->pred_select != 0, motion = ctx->pred_motion != 0;
    const size_t nmodes = select_count(nt, H, W);
    uint8_t* d_modes = nullptr;
    int8_t* d_vecs = nullptr;
    tz_call call(ctx);
    TZ_TRY(rollout_setup(ctx, frames, nt, H, W, warm_up));   // (the whole stack goes up ahead: every frame is read by a step)
    // key mask and groups of the open-loop SWP job (rollout_swp; compress.py:188-220, 249-262)
    std::vector<uint8_t> key(nt, 0), gfirst(nt, 0), qskip(nt, 0);
    std::vector<int> c0_slots;
    for (int i = 0; i < p; ++i) {
        key[i] = 1;
        qskip[i] = 1;
        c0_slots.push_back(i);
    }
    gfirst[0] = 1;
    if (p > 0) gfirst[p] = 1;
    c0_slots.push_back(p > 0 ? p : 0);
    key[p] = 1;   // (nt >= p + 2: frame p + 1 starts from frame p)
    for (int idx = p + 1; idx < nt; ++idx)
        if ((idx - p) % window == 0) {
            gfirst[idx] = 1;
            key[idx] = 1;   // the frame the next window starts from, or the last frame (compress.py:260-262)
            c0_slots.push_back(idx);
        }
    for (int i = 0; i < nt; ++i)
        if (gfirst[i]) qskip[i] = 1;
    int rc = fill_c0(ctx, c0_slots);
    const std::vector<std::vector<int>> steps = closed_steps(key);
    if (rc == TZ_OK && lossless) {   // the decoded frame is the original: every prediction is independent of every other
        std::vector<int> all;
        for (const auto& st : steps) all.insert(all.end(), st.begin(), st.end());
        rc = closed_predict(ctx, all, ctx->d_frames);
        if (rc == TZ_OK && select) {   // TZ-PS1: one launch over all of them (the frame in front is the original)
            const int* d_all = nullptr;
            rc = closed_lists(call, steps, &d_all);
            if (rc == TZ_OK) rc = select_modes(call, nmodes, nullptr, &d_modes);
            if (rc == TZ_OK) rc = tzk_ps_select(ctx, ctx->d_pred, ctx->d_frames, d_modes, d_all, (int)all.size(), H, W, ctx->Hp, ctx->Wp);
        } else if (rc == TZ_OK && motion) {   // TZ-PM1: likewise, with the search
            const int* d_all = nullptr;
            rc = closed_lists(call, steps, &d_all);
            if (rc == TZ_OK) rc = select_modes(call, nmodes, nullptr, &d_modes);
            if (rc == TZ_OK) rc = motion_vectors(call, 2 * nmodes, nullptr, &d_vecs);
            if (rc == TZ_OK) rc = tzk_pm_select(ctx, ctx->d_pred, ctx->d_frames, d_modes, d_vecs, d_all, (int)all.size(), H, W, ctx->Hp, ctx->Wp);
        }
    } else if (rc == TZ_OK) {
        const size_t fb = (size_t)nt * H * W * 3;
        uint8_t* d_dec = nullptr;
        const int* d_lists = nullptr;
        rc = call.alloc(fb, &d_dec);
        if (rc == TZ_OK) rc = closed_lists(call, steps, &d_lists);
        if (rc == TZ_OK && (select || motion)) rc = select_modes(call, nmodes, nullptr, &d_modes);
        if (rc == TZ_OK && motion) rc = motion_vectors(call, 2 * nmodes, nullptr, &d_vecs);
        if (rc == TZ_OK && hipMemcpyAsync(d_dec, ctx->d_frames, fb, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)   // the key frames
            rc = tz_fail(ctx, TZ_ERR_HIP, "%s: copy of the frame stack failed", who);
        size_t at = 0;
        for (size_t s = 0; s < steps.size() && rc == TZ_OK; at += steps[s].size(), ++s) {
            rc = closed_predict(ctx, steps[s], d_dec);
            if (rc == TZ_OK && d_map && select)   // TZ-CLM1: the same two kernels' places, Q under the map
                rc = tzk_psm_step(ctx, ctx->d_pred, ctx->d_frames, d_dec, d_modes, d_map, d_lists + at, (int)steps[s].size(), H, W, ctx->Hp, ctx->Wp);
            else if (rc == TZ_OK && d_map)
                rc = tzk_clm_step(ctx, ctx->d_pred, ctx->d_frames, d_dec, d_map, d_lists + at, (int)steps[s].size(), H, W, ctx->Hp, ctx->Wp);
            else if (rc == TZ_OK && select)   // TZ-PS1 in the step's place: the mode bytes, the chosen tiles in the predictions, dec[t]
                rc = tzk_ps_step(ctx, ctx->d_pred, ctx->d_frames, d_dec, d_modes, d_lists + at, (int)steps[s].size(), H, W, ctx->Hp, ctx->Wp, E);
            else if (rc == TZ_OK && motion)   // TZ-PM1 in the step's place: also the vectors
                rc = tzk_pm_step(ctx, ctx->d_pred, ctx->d_frames, d_dec, d_modes, d_vecs, d_lists + at, (int)steps[s].size(), H, W, ctx->Hp, ctx->Wp, E);
            else if (rc == TZ_OK)
                rc = tzk_cl_step(ctx, ctx->d_pred, ctx->d_frames, d_dec, d_lists + at, (int)steps[s].size(), H, W, ctx->Hp, ctx->Wp, E);
        }
    }
    std::vector<uint8_t> modes(select || motion ? nmodes : 0);
    std::vector<int8_t> vectors(motion ? 2 * nmodes : 0);
    if (rc == TZ_OK && (select || motion)) rc = tz_d2h(ctx, modes.data(), d_modes, nmodes, ctx->stream);
    if (rc == TZ_OK && motion) rc = tz_d2h(ctx, vectors.data(), d_vecs, 2 * nmodes, ctx->stream);
    if (rc == TZ_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = tz_fail(ctx, TZ_ERR_HIP, "closed-loop rollout failed");
    if (rc != TZ_OK) {  // nothing of a failed rollout may still read the caller's frames when we return
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    ctx->key_mask = key;
    ctx->group_first = gfirst;
    ctx->quant_skip = qskip;
    set_rollout(ctx, tz_ctx::ROLLOUT_ENCODE, 0, nt);
    ctx->pred_contract = tz_get_contract(ctx);
    ctx->loop_closed = 1;   // (the caller adds what the loop ran under)
    ctx->loop_select = select ? 1 : 0;
    ctx->loop_motion = motion ? ctx->pred_motion : 0;
    ctx->pred_modes.swap(modes);
    ctx->pred_vectors.swap(vectors);
    if (key_mask) memcpy(key_mask, key.data(), nt);
    return TZ_OK;
}

extern "C" int tz_rollout_closed(tz_ctx* ctx, const uint8_t* frames, int nt, int H, int W, int warm_up, int window, int mode, double b0,
                                 double b1, uint8_t* key_mask) {
    tz_roctx_range roctx_("tz_rollout_closed");
    if (!ctx) return TZ_ERR_INVALID;
    ctx->enc_kind = tz_ctx::ENC_NONE;
    if (window < 0) return tz_fail(ctx, TZ_ERR_INVALID, "window must be >= 0");
    if (mode < 0 || mode > 3) return tz_fail(ctx, TZ_ERR_INVALID, "unknown error-bound mode %d", mode);
    if (std::isnan(b0) || (mode == TZ_MODE_ABSREL && std::isnan(b1)))
        return tz_fail(ctx, TZ_ERR_INVALID, "error bound is NaN (the reference raises on a NaN tolerance)");
    if (window == 0)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed: the closed loop serves fixed windows (window > 0), not the threshold rule");
    if (nt < warm_up + 2)
        return tz_fail(ctx, TZ_ERR_INVALID, "need at least warm_up+2 frames (nt=%d, warm_up=%d)", nt, warm_up);
    // what the loop feeds back: the original where the job's quantiser leaves every delta as it is, else TZ-QL1 under one abs bound
    const bool lossless = b0 == 0.0 || (mode == TZ_MODE_ABSREL && b1 == 0.0) ||
                          (ctx->quantiser == 1 ? tz_lattice_is_identity(mode, b0, b1) : tz_quant_is_identity(mode, b0, b1));
    if (!lossless && ctx->quantiser != 1)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed: a lossy closed loop needs the lattice quantiser (tz_set_quantiser(1)): the greedy walk is no function of one sample");
    if (!lossless && mode != TZ_MODE_ABS)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed: a lossy closed loop takes mode abs, not %d: rel bounds depend on whole frames", mode);
    if (ctx->payload_channels != 3 || !ctx->frame_bounds.empty() || ctx->map_h)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed: the closed loop takes one bound and a three-channel payload (no tz_set_payload_channels(1), tz_set_frame_bounds or tz_set_bound_map)");
    TZ_TRY(closed_rollout(ctx, "tz_rollout_closed", frames, nt, H, W, warm_up, window, lossless, fabs(b0) >= 255.0 ? 255 : (int)fabs(b0), nullptr,
                          key_mask));
    ctx->loop_mode = mode;
    ctx->loop_b0 = b0;
    ctx->loop_b1 = b1;
    ctx->loop_quantiser = ctx->quantiser;
    return TZ_OK;
}

// ---- the closed loop under one abs bound per pixel, definition TZ-CLM1 (include/tezip_hip.h: tz_rollout_closed_map; slow statement
// in tezip_amd/closedmap.py): tz_rollout_closed's loop with E = map[pixel] of the bound map in force.  TZ-BM1 under the lattice
// quantiser is a pure function of one delta and one tolerance, which is all the loop needs.
extern "C" int tz_rollout_closed_map(tz_ctx* ctx, const uint8_t* frames, int nt, int H, int W, int warm_up, int window, uint8_t* key_mask) {
    tz_roctx_range roctx_("tz_rollout_closed_map");
    if (!ctx) return TZ_ERR_INVALID;
    ctx->enc_kind = tz_ctx::ENC_NONE;
    if (window < 0) return tz_fail(ctx, TZ_ERR_INVALID, "window must be >= 0");
    if (window == 0)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_map: the closed loop serves fixed windows (window > 0), not the threshold rule");
    if (nt < warm_up + 2 || warm_up < 0)
        return tz_fail(ctx, TZ_ERR_INVALID, "need at least warm_up+2 frames (nt=%d, warm_up=%d)", nt, warm_up);
    if (ctx->quantiser != 1)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_map needs the lattice quantiser (tz_set_quantiser(1)): the greedy walk is no function of one sample");
    if (ctx->payload_channels != 3)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_map: the loop decodes three channels (no tz_set_payload_channels(1))");
    if (!ctx->frame_bounds.empty())
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_map takes one bound per pixel, not one per frame as well: clear tz_set_frame_bounds first");
    if (ctx->pred_motion)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_map does not serve motion-compensated tiles (tz_set_pred_motion): tz_set_pred_select is served");
    // (behind the setters' refusals: frame bounds exclude a map at the setters, so "no map" would hide what is in the way)
    if (!ctx->map_h) return tz_fail(ctx, TZ_ERR_STATE, "tz_rollout_closed_map needs a bound map in force (tz_set_bound_map)");
    if (ctx->map_h != H || ctx->map_w != W)
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_rollout_closed_map: the bound map is %d x %d (tz_set_bound_map), the frames are %d x %d: a map has the frames' own size",
                       ctx->map_h, ctx->map_w, H, W);
    TZ_TRY(closed_rollout(ctx, "tz_rollout_closed_map", frames, nt, H, W, warm_up, window, ctx->map_max == 0, 0, ctx->d_bound_map, key_mask));
    ctx->loop_mode = TZ_MODE_ABS;
    ctx->loop_b0 = ctx->loop_b1 = 0.0;
    ctx->loop_quantiser = 1;
    ctx->loop_map = 1;
    ctx->loop_map_h = ctx->map_h;
    ctx->loop_map_w = ctx->map_w;
    ctx->loop_map_bytes = ctx->map_host;
    return TZ_OK;
}

// ---- the closed loop under one abs bound per frame, definition TZ-CLF1 (include/tezip_hip.h: tz_rollout_closed_frames; slow
// statement in tezip_amd/closedframes.py).  When the loop stands at frame t, pred_t is fixed, so every candidate bound of frame t
// is priced by a pass over (pred_t, orig_t) alone: the search costs TZ_CLF_ROUNDS small launches a step and no host wait.
extern "C" int tz_rollout_closed_frames(tz_ctx* ctx, const uint8_t* frames, int nt, int H, int W, int warm_up, int window, const double* bounds,
                                        unsigned long long sse_limit, uint8_t* key_mask) {
    tz_roctx_range roctx_("tz_rollout_closed_frames");
    if (!ctx) return TZ_ERR_INVALID;
    ctx->enc_kind = tz_ctx::ENC_NONE;
    if (window < 0) return tz_fail(ctx, TZ_ERR_INVALID, "window must be >= 0");
    if ((bounds != nullptr) == (sse_limit > 0))
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_rollout_closed_frames takes either the bounds or an sse limit > 0 to search them under, not %s",
                       bounds ? "both" : "neither");
    if (window == 0)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_frames: the closed loop serves fixed windows (window > 0), not the threshold rule");
    if (nt < warm_up + 2 || warm_up < 0)
        return tz_fail(ctx, TZ_ERR_INVALID, "need at least warm_up+2 frames (nt=%d, warm_up=%d)", nt, warm_up);
    if (bounds)
        for (int f = 0; f < nt; ++f)
            if (!std::isfinite(bounds[f]) || bounds[f] < 0.0)
                return tz_fail(ctx, TZ_ERR_INVALID, "tz_rollout_closed_frames: bound %g of frame %d is not a finite number >= 0", bounds[f], f);
    if (ctx->quantiser != 1)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_frames needs the lattice quantiser (tz_set_quantiser(1)): the greedy walk is no function of one sample");
    if (ctx->payload_channels != 3)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_frames: the loop decodes three channels (no tz_set_payload_channels(1))");
    if (ctx->map_h) return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_frames does not serve a bound map (tz_set_bound_map)");
    if (!ctx->frame_bounds.empty())
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_frames takes its bounds itself: clear tz_set_frame_bounds first, and set it to tz_loop_frame_bounds' answer for the job");
    if (ctx->pred_select)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_frames does not serve per-tile selection (tz_set_pred_select)");
    if (ctx->pred_motion)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_closed_frames does not serve motion-compensated tiles (tz_set_pred_motion)");
    const int p = warm_up;
    tz_call call(ctx);
    TZ_TRY(rollout_setup(ctx, frames, nt, H, W, warm_up));
    // key mask and groups: tz_rollout_closed's
    std::vector<uint8_t> key(nt, 0), gfirst(nt, 0), qskip(nt, 0);
    std::vector<int> c0_slots;
    for (int i = 0; i < p; ++i) {
        key[i] = 1;
        qskip[i] = 1;
        c0_slots.push_back(i);
    }
    gfirst[0] = 1;
    if (p > 0) gfirst[p] = 1;
    c0_slots.push_back(p > 0 ? p : 0);
    key[p] = 1;
    for (int idx = p + 1; idx < nt; ++idx)
        if ((idx - p) % window == 0) {
            gfirst[idx] = 1;
            key[idx] = 1;
            c0_slots.push_back(idx);
        }
    for (int i = 0; i < nt; ++i)
        if (gfirst[i]) qskip[i] = 1;
    // the bounds of the stamp (0 at the frames stored exactly) and their radii E = min(255, floor(b))
    std::vector<double> norm(nt, 0.0);
    std::vector<int> radius(nt, 0);
    bool lossless = bounds != nullptr;
    for (int f = 0; f < nt && bounds; ++f) {
        if (key[f]) continue;
        norm[f] = bounds[f];
        radius[f] = bounds[f] >= 255.0 ? 255 : (int)bounds[f];
        if (radius[f]) lossless = false;
    }
    std::vector<unsigned long long> fsse(nt, 0ull), trace;
    std::vector<int> ks(nt, 0);
    int rc = fill_c0(ctx, c0_slots);
    const std::vector<std::vector<int>> steps = closed_steps(key);
    if (rc == TZ_OK && lossless) {   // every E is 0: the lossless closed job, one schedule
        std::vector<int> all;
        for (const auto& st : steps) all.insert(all.end(), st.begin(), st.end());
        rc = closed_predict(ctx, all, ctx->d_frames);
    } else if (rc == TZ_OK) {
        const size_t fb = (size_t)nt * H * W * 3, ntrace = (size_t)TZ_CLF_ROUNDS * nt;
        uint8_t* d_dec = nullptr;
        const int* d_lists = nullptr;
        int *d_radius = nullptr, *d_k = nullptr;
        unsigned long long *d_sse = nullptr, *d_fsse = nullptr;
        rc = call.alloc(fb, &d_dec);
        if (rc == TZ_OK) rc = closed_lists(call, steps, &d_lists);
        if (rc == TZ_OK && bounds) {
            rc = call.alloc((size_t)nt * sizeof(int), &d_radius);
            if (rc == TZ_OK) rc = tz_upload(ctx, d_radius, radius.data(), (size_t)nt * sizeof(int));
        } else if (rc == TZ_OK) {
            rc = call.alloc(ntrace * sizeof(unsigned long long), &d_sse);
            if (rc == TZ_OK) rc = call.alloc((size_t)nt * sizeof(unsigned long long), &d_fsse);
            if (rc == TZ_OK) rc = call.alloc((size_t)nt * sizeof(int), &d_k);
            if (rc == TZ_OK && (hipMemsetAsync(d_sse, 0, ntrace * sizeof(unsigned long long), ctx->stream) != hipSuccess ||
                                hipMemsetAsync(d_fsse, 0, (size_t)nt * sizeof(unsigned long long), ctx->stream) != hipSuccess ||
                                hipMemsetAsync(d_k, 0, (size_t)nt * sizeof(int), ctx->stream) != hipSuccess))
                rc = tz_fail(ctx, TZ_ERR_HIP, "tz_rollout_closed_frames: clearing the search's sums failed");
        }
        if (rc == TZ_OK && hipMemcpyAsync(d_dec, ctx->d_frames, fb, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)   // the key frames
            rc = tz_fail(ctx, TZ_ERR_HIP, "tz_rollout_closed_frames: copy of the frame stack failed");
        size_t at = 0;
        for (size_t s = 0; s < steps.size() && rc == TZ_OK; at += steps[s].size(), ++s) {
            const int n = (int)steps[s].size();
            rc = closed_predict(ctx, steps[s], d_dec);
            for (int r = 0; r < TZ_CLF_ROUNDS && rc == TZ_OK && !bounds; ++r)
                rc = tzk_clf_probe(ctx, ctx->d_pred, ctx->d_frames, d_lists + at, n, H, W, ctx->Hp, ctx->Wp, r, d_sse, nt, sse_limit);
            if (rc == TZ_OK)
                rc = tzk_clf_step(ctx, ctx->d_pred, ctx->d_frames, d_dec, d_lists + at, n, H, W, ctx->Hp, ctx->Wp, d_radius, d_sse, nt, sse_limit,
                                  d_k, d_fsse);
        }
        if (rc == TZ_OK && !bounds) {   // one copy-back behind the loop: k, sse(k) and the rounds' sums
            trace.resize(ntrace);
            rc = tz_d2h(ctx, ks.data(), d_k, (size_t)nt * sizeof(int), ctx->stream);
            if (rc == TZ_OK) rc = tz_d2h(ctx, fsse.data(), d_fsse, (size_t)nt * sizeof(unsigned long long), ctx->stream);
            if (rc == TZ_OK) rc = tz_d2h(ctx, trace.data(), d_sse, ntrace * sizeof(unsigned long long), ctx->stream);
        }
    }
    if (rc == TZ_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = tz_fail(ctx, TZ_ERR_HIP, "closed-loop rollout failed");
    if (rc != TZ_OK) {  // nothing of a failed rollout may still read the caller's frames when we return
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    if (!bounds) {   // the bounds found, and ~0 in the rounds that did not run for a frame (the device array starts from zeros)
        for (int f = 0; f < nt; ++f) {
            norm[f] = key[f] ? 0.0 : ks[f] / 2.0;
            int lo = 0, hi = key[f] ? 1 : 511;
            for (int r = 0; r < TZ_CLF_ROUNDS; ++r) {
                unsigned long long& v = trace[(size_t)r * nt + f];
                if (hi - lo <= 1) {
                    v = ~0ull;
                    continue;
                }
                const int mid = (lo + hi) / 2;
                if (v <= sse_limit) lo = mid;
                else hi = mid;
            }
        }
    }
    ctx->key_mask = key;
    ctx->group_first = gfirst;
    ctx->quant_skip = qskip;
    set_rollout(ctx, tz_ctx::ROLLOUT_ENCODE, 0, nt);
    ctx->pred_contract = tz_get_contract(ctx);
    ctx->loop_closed = 1;
    ctx->loop_mode = TZ_MODE_ABS;
    ctx->loop_b0 = ctx->loop_b1 = 0.0;
    ctx->loop_quantiser = 1;
    ctx->loop_frames = 1;
    ctx->loop_bounds.swap(norm);
    ctx->loop_frame_sse.swap(fsse);
    ctx->loop_trace.swap(trace);
    if (key_mask) memcpy(key_mask, key.data(), nt);
    return TZ_OK;
}

extern "C" int tz_loop_frame_bounds(tz_ctx* ctx, double* bounds, unsigned long long* sse, int cap) {
    if (!ctx) return TZ_ERR_INVALID;
    if (ctx->rollout_kind != tz_ctx::ROLLOUT_ENCODE || !ctx->loop_closed || !ctx->loop_frames)
        return tz_fail(ctx, TZ_ERR_STATE, "tz_loop_frame_bounds: the resident rollout is no tz_rollout_closed_frames");
    const int nt = (int)ctx->loop_bounds.size();
    if ((bounds || sse) && cap < nt) return tz_fail(ctx, TZ_ERR_INVALID, "tz_loop_frame_bounds: room for %d frames, the rollout has %d", cap, nt);
    if (bounds) memcpy(bounds, ctx->loop_bounds.data(), (size_t)nt * sizeof(double));
    if (sse) memcpy(sse, ctx->loop_frame_sse.data(), (size_t)nt * sizeof(unsigned long long));
    return nt;
}

extern "C" int tz_loop_search_trace(tz_ctx* ctx, unsigned long long* sse, int cap) {
    if (!ctx) return TZ_ERR_INVALID;
    if (ctx->rollout_kind != tz_ctx::ROLLOUT_ENCODE || !ctx->loop_closed || !ctx->loop_frames || ctx->loop_trace.empty())
        return tz_fail(ctx, TZ_ERR_STATE, "tz_loop_search_trace: the resident rollout is no tz_rollout_closed_frames that searched its bounds");
    const int n = (int)ctx->loop_trace.size();
    if (sse && cap < n) return tz_fail(ctx, TZ_ERR_INVALID, "tz_loop_search_trace: room for %d sums, the search has %d", cap, n);
    if (sse) memcpy(sse, ctx->loop_trace.data(), (size_t)n * sizeof(unsigned long long));
    return n;
}

extern "C" int tz_rollout_loop(tz_ctx* ctx) {
    if (!ctx) return TZ_ERR_INVALID;
    if (ctx->rollout_kind == tz_ctx::ROLLOUT_NONE) return tz_fail(ctx, TZ_ERR_STATE, "no rollout in this context");
    return ctx->loop_closed;
}

extern "C" int tz_rollout_decode_closed(tz_ctx* ctx, const uint8_t* key_frames, int nt, int H, int W, int warm_up, const int16_t* payload,
                                        size_t payload_len, const int16_t* table, int table_len, uint8_t* key_mask) {
    tz_roctx_range roctx_("tz_rollout_decode_closed");
    if (!ctx) return TZ_ERR_INVALID;
    if (ctx->payload_channels != 3)
        return tz_fail(ctx, TZ_ERR_UNSUPPORTED, "tz_rollout_decode_closed does not serve a one-channel payload (tz_set_payload_channels(1))");
    TZ_TRY(check_table(ctx, table, table_len));
    const bool select = ctx->pred_select != 0, motion = ctx->pred_motion != 0;
    if (select && nt > 0 && H > 0 && W > 0 && ctx->put_modes.size() != select_count(nt, H, W))
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_rollout_decode_closed under tz_set_pred_select(1): %zu mode bytes were put (tz_put_pred_modes), "
                       "the stack has %zu tiles", ctx->put_modes.size(), select_count(nt, H, W));
    if (motion && nt > 0 && H > 0 && W > 0 && ctx->put_modes.size() != select_count(nt, H, W))
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_rollout_decode_closed under tz_set_pred_motion(%d): %zu mode bytes were put (tz_put_pred_modes), "
                       "the stack has %zu tiles", ctx->pred_motion, ctx->put_modes.size(), select_count(nt, H, W));
    if (motion && nt > 0 && H > 0 && W > 0 && ctx->put_vectors.size() != 2 * select_count(nt, H, W))
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_rollout_decode_closed under tz_set_pred_motion(%d): %zu vector components were put "
                       "(tz_put_pred_vectors), the stack has %zu tiles of two", ctx->pred_motion, ctx->put_vectors.size(), select_count(nt, H, W));
    ctx->have_decoded = false;
    tz_call call(ctx);
    TZ_TRY(rollout_setup(ctx, key_frames, nt, H, W, warm_up));
    ctx->enc_kind = tz_ctx::ENC_NONE;
    const size_t fe = (size_t)H * W * 3, N = (size_t)nt * fe;
    if (!payload) TZ_TRY(staged_payload(ctx, N, &payload));   // (a rollout leaves the staged payload alone)
    if (payload_len != N)
        return tz_fail(ctx, TZ_ERR_INVALID, "payload holds %zu elements, the key-frame stack implies %zu", payload_len, N);
    std::vector<int> flags(nt, 0);
    TZ_TRY(discover_keys(ctx, nt, H, W, &flags));
    std::vector<uint8_t> key(nt);
    for (int i = 0; i < nt; ++i) key[i] = flags[i] ? 1 : 0;
    for (int i = 0; i <= warm_up; ++i)   // decompress.py:138-179: frames 0 .. warm_up are key frames
        if (i >= nt || !key[i]) return tz_fail(ctx, TZ_ERR_INVALID, "key frames do not cover the sequence (frame %d)", i);
    // q: the quantised delta stack, by the layout's inverse remap and inverse spatial delta -- no prediction is needed for it
    const tz_layout layout = layout_of(ctx);
    const int16_t* d_pay;
    int16_t* d_q;
    const int* d_lists = nullptr;
    TZ_TRY(call.in(payload, N * 2, &d_pay));
    TZ_TRY(call.alloc(N * 2, &d_q));
    std::vector<int16_t> lut;
    if (table_len >= 0) build_dec_lut(table, table_len, 1, &lut);
    const int16_t* h_lut = table_len >= 0 ? lut.data() : nullptr;
    if (layout.plane_h) TZ_TRY(tzk_unplane(ctx, d_pay, nt, H, W, 3, h_lut, 1, d_q));
    else TZ_TRY(tzk_undelta(ctx, layout.stride, d_pay, N, nullptr, h_lut, 1, d_q));
    // the decoded stack starts as the key stack: key frames are stored exactly, every other frame is written by its step
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_out, &ctx->cap_out, N));
    TZ_HIP(ctx, hipMemcpyAsync(ctx->d_out, ctx->d_frames, N, hipMemcpyDeviceToDevice, ctx->stream));
    std::vector<int> c0_slots;
    for (int i = 0; i < nt; ++i)
        if (key[i]) c0_slots.push_back(i);   // (a key slot is never read for reconstruction)
    TZ_TRY(fill_c0(ctx, c0_slots));
    const std::vector<std::vector<int>> steps = closed_steps(key);
    TZ_TRY(closed_lists(call, steps, &d_lists));
    uint8_t* d_modes = nullptr;
    int8_t* d_vecs = nullptr;
    if (motion) {   // TZ-PM1: a vector belongs to a tile of mode 1, and a key frame has none
        const size_t per = select_count(1, H, W);
        for (int i = 0; i < nt; ++i)
            if (key[i] && std::any_of(ctx->put_vectors.begin() + 2 * i * per, ctx->put_vectors.begin() + 2 * (i + 1) * per, [](int8_t v) { return v != 0; }))
                return tz_fail(ctx, TZ_ERR_INVALID, "tz_rollout_decode_closed: a vector of key frame %d is non-zero (key frames are stored exactly)", i);
        for (size_t i = 0; i < ctx->put_modes.size(); ++i)
            if (!ctx->put_modes[i] && (ctx->put_vectors[2 * i] || ctx->put_vectors[2 * i + 1]))
                return tz_fail(ctx, TZ_ERR_INVALID, "tz_rollout_decode_closed: tile %zu has mode 0 and the vector (%d, %d): only a tile taken from "
                               "the frame in front is displaced", i, (int)ctx->put_vectors[2 * i], (int)ctx->put_vectors[2 * i + 1]);
        TZ_TRY(motion_vectors(call, ctx->put_vectors.size(), ctx->put_vectors.data(), &d_vecs));
    }
    if (select || motion) {   // TZ-PS1: the stored modes, now that the keys are known
        const size_t per = select_count(1, H, W);
        for (int i = 0; i < nt; ++i)
            if (key[i] && std::any_of(ctx->put_modes.begin() + i * per, ctx->put_modes.begin() + (i + 1) * per, [](uint8_t m) { return m != 0; }))
                return tz_fail(ctx, TZ_ERR_INVALID, "tz_rollout_decode_closed: a mode byte of key frame %d is set (key frames are stored exactly)", i);
        TZ_TRY(select_modes(call, ctx->put_modes.size(), ctx->put_modes.data(), &d_modes));
    }
    size_t at = 0;
    for (size_t s = 0; s < steps.size(); at += steps[s].size(), ++s) {
        TZ_TRY(closed_predict(ctx, steps[s], ctx->d_out));
        if (motion) TZ_TRY(tzk_pm_recon(ctx, ctx->d_pred, d_q, ctx->d_out, d_modes, d_vecs, d_lists + at, (int)steps[s].size(), H, W, ctx->Hp, ctx->Wp));
        else if (select) TZ_TRY(tzk_ps_recon(ctx, ctx->d_pred, d_q, ctx->d_out, d_modes, d_lists + at, (int)steps[s].size(), H, W, ctx->Hp, ctx->Wp));
        else TZ_TRY(tzk_cl_recon(ctx, ctx->d_pred, d_q, ctx->d_out, d_lists + at, (int)steps[s].size(), H, W, ctx->Hp, ctx->Wp));
    }
    TZ_TRY(tz_stream_sync(ctx));
    ctx->key_mask = recon_key_mask(key.data(), nt, warm_up);
    set_rollout(ctx, tz_ctx::ROLLOUT_DECODE, 0, nt);
    ctx->pred_contract = tz_get_contract(ctx);
    ctx->have_decoded = true;
    ctx->dec_first = 0;
    ctx->dec_count = nt;
    if (key_mask) memcpy(key_mask, key.data(), nt);
    return TZ_OK;
}

// What the stored payload of an encode decodes to (include/tezip_hip.h: tz_encode_quality, tz_encode_digests): the decoder's
// tail over the payload on the ENCODER's predictions and frames -- the reconstruct reads frames only where the mask says
// "key", and there the encoder's originals are the bytes key_frame.dat stores -- into pool scratch (*d_dec, nt*H*W*3
// bytes, queued on the context's stream).  Only scratch is written, under the caller's scope.  One statement of
// "decoded" for every entry point that describes it.
static int encode_decoded(tz_call& call, const char* who, const int16_t* payload, size_t payload_len, const int16_t* table,
                          int table_len, int shuffled, const uint8_t** d_dec_out) {
    tz_ctx* ctx = call.ctx;
    if (!whole_stack(ctx, tz_ctx::ROLLOUT_ENCODE)) return tz_fail(ctx, TZ_ERR_STATE, "%s needs the encoder rollout of a tz_rollout", who);
    TZ_TRY(tz_check_pred_contract(ctx, who));
    TZ_TRY(check_table(ctx, table, table_len));
    const int nt = ctx->nt, H = ctx->H, W = ctx->W;
    const tz_layout layout = layout_of(ctx);
    const size_t fe = (size_t)H * W * 3, N = (size_t)nt * tz_frame_elems(layout, H, W);   // N: payload elements
    if (!payload) {
        if (ctx->enc_kind != tz_ctx::ENC_PAYLOAD || !ctx->d_payload || ctx->payload_len != N)
            return tz_fail(ctx, TZ_ERR_STATE, "no resident payload of a tz_encode on this rollout");
        payload = ctx->d_payload;
    }
    if (payload_len != N)
        return tz_fail(ctx, TZ_ERR_INVALID, "payload holds %zu elements, the encoded stack %zu", payload_len, N);
    if (shuffled && (N & 7)) return tz_fail(ctx, TZ_ERR_INVALID, "byte shuffle needs a multiple of 8 elements");
    const int16_t* d_pay;
    uint8_t *d_plain, *d_mask, *d_dec;
    TZ_TRY(call.in(payload, N * 2, &d_pay));
    if (shuffled) {   // byte planes -> int16 in scratch (the caller's payload stays as it is)
        TZ_TRY(call.alloc(N * 2, &d_plain));
        TZ_TRY(tzk_shuffle(ctx, d_pay, N, d_plain, 1));
        d_pay = (const int16_t*)d_plain;
    }
    const std::vector<uint8_t> recon = recon_key_mask(ctx->key_mask.data(), nt, ctx->warm_up);
    TZ_TRY(call.alloc(nt, &d_mask));
    TZ_TRY(tz_upload(ctx, d_mask, recon.data(), nt));
    TZ_TRY(call.alloc((size_t)nt * fe, &d_dec));
    std::vector<int16_t> lut;
    if (table_len >= 0) build_dec_lut(table, table_len, 1, &lut);
    *d_dec_out = d_dec;
    // the launches of tz_decode
    return tzk_decode_tail(ctx, layout, d_pay, table_len >= 0 ? lut.data() : nullptr, 1, nullptr, ctx->d_pred, ctx->d_frames, d_mask, nt, H, W,
                           ctx->Hp, ctx->Wp, d_dec);
}

// The report of `-c --report`: k_quality of the decoded stack against the originals.
extern "C" int tz_encode_quality(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len,
                                 int shuffled, tz_frame_quality* out) {
    tz_roctx_range roctx_("tz_encode_quality");
    if (!ctx || !out) return TZ_ERR_INVALID;
    tz_call call(ctx);
    const uint8_t* d_dec;
    tz_frame_quality* d_out;
    TZ_TRY(encode_decoded(call, "tz_encode_quality", payload, payload_len, table, table_len, shuffled, &d_dec));
    TZ_TRY(call.out(out, sizeof(tz_frame_quality) * ctx->nt, &d_out));
    TZ_TRY(tzk_quality(ctx, ctx->d_frames, d_dec, ctx->nt, (size_t)ctx->H * ctx->W * 3, d_out));
    TZ_TRY(call.finish());
    return tz_stream_sync(ctx);   // (device records too: complete on return)
}

// The bound-map line of `-c --bound-map --report`: k_map_check of the decoded stack against the originals under the context's map.
extern "C" int tz_encode_map_check(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len,
                                   int shuffled, tz_map_record* out) {
    tz_roctx_range roctx_("tz_encode_map_check");
    if (!ctx || !out) return TZ_ERR_INVALID;
    if (!ctx->map_h) return tz_fail(ctx, TZ_ERR_STATE, "tz_encode_map_check needs a bound map (tz_set_bound_map)");
    if (ctx->map_h != ctx->H || ctx->map_w != ctx->W)
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_encode_map_check: the bound map is %d x %d, the rollout's frames are %d x %d: a map has the frames' own size",
                       ctx->map_h, ctx->map_w, ctx->H, ctx->W);
    tz_call call(ctx);
    const uint8_t* d_dec;
    tz_map_record* d_out;
    TZ_TRY(encode_decoded(call, "tz_encode_map_check", payload, payload_len, table, table_len, shuffled, &d_dec));
    TZ_TRY(call.out(out, sizeof(tz_map_record) * ctx->nt, &d_out));
    TZ_TRY(tzk_map_check(ctx, ctx->d_frames, d_dec, ctx->d_bound_map, ctx->nt, ctx->H, ctx->W, d_out));
    TZ_TRY(call.finish());
    return tz_stream_sync(ctx);   // (device records too: complete on return)
}

// k_map_check alone, on any two stacks and any map (tests against tezip_amd/boundmap.py check).
extern "C" int tz_map_check(tz_ctx* ctx, const uint8_t* orig, const uint8_t* decoded, const uint8_t* map, int nframes, int H, int W,
                            tz_map_record* out) {
    tz_roctx_range roctx_("tz_map_check");
    if (!ctx) return TZ_ERR_INVALID;
    if (nframes <= 0) return TZ_OK;
    if (!orig || !decoded || !map || !out) return TZ_ERR_INVALID;
    if (H < 1 || W < 1) return tz_fail(ctx, TZ_ERR_INVALID, "frames of %d x %d", H, W);
    const size_t n = (size_t)nframes * H * W * 3;
    tz_call call(ctx);
    const uint8_t *d_o, *d_d, *d_m;
    tz_map_record* d_out;
    TZ_TRY(call.in(orig, n, &d_o));
    TZ_TRY(call.in(decoded, n, &d_d));
    TZ_TRY(call.in(map, (size_t)H * W, &d_m));
    TZ_TRY(call.out(out, sizeof(tz_map_record) * nframes, &d_out));
    TZ_TRY(tzk_map_check(ctx, d_o, d_d, d_m, nframes, H, W, d_out));
    TZ_TRY(call.finish());
    return tz_stream_sync(ctx);
}

// One candidate bound of `-c --target-psnr` (TZ-TPSNR-1): the records tz_encode(mode, b0, b1) + tz_encode_quality would give,
// from the delta stack, a quantised copy of it and k_bound_err -- no spatial delta, histogram, table or payload.  The mask
// that zeroes a frame's delta (group_first) and the frames the quantiser skips (quant_skip) are the encoder's own; a frame
// they leave with q == d reconstructs to its original, which is what the decoder's key bytes and C0 slots give.
// Under a one-channel payload the job stores channel 0 alone and its decoder writes that reconstruction to all three
// channels: tz_encode's refusal of a stack with colour comes first, and the kernel counts channel 0 three times.  (The
// model's three output channels differ even on a gray source, so the three-channel records would be another job's.)
extern "C" int tz_bound_probe(tz_ctx* ctx, int mode, double b0, double b1, tz_frame_quality* out) {
    tz_roctx_range roctx_("tz_bound_probe");
    if (!ctx || !out) return TZ_ERR_INVALID;
    TZ_TRY(encode_check(ctx, "tz_bound_probe", mode, b0, b1));
    const int channels = layout_of(ctx).channels;
    if (channels == 1) {
        tz_call gray_check(ctx);   // (a scope of its own: the probe reuses its blocks)
        TZ_TRY(encode_all_gray(ctx));
    }
    const int nt = ctx->nt, H = ctx->H, W = ctx->W;
    const size_t fe = (size_t)H * W * 3, N = (size_t)nt * fe;
    tz_call call(ctx);
    uint8_t* d_mask;
    int16_t *d_delta, *d_q;
    tz_frame_quality* d_out;
    TZ_TRY(call.alloc(nt, &d_mask));
    TZ_TRY(tz_upload(ctx, d_mask, ctx->group_first.data(), nt));
    TZ_TRY(call.alloc(N * 2, &d_delta));
    TZ_TRY(call.alloc(N * 2, &d_q));
    TZ_TRY(tzk_delta(ctx, ctx->d_pred, ctx->d_frames, d_mask, nt, H, W, ctx->Hp, ctx->Wp, d_delta));
    if (hipMemcpyAsync(d_q, d_delta, N * 2, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
        return tz_fail(ctx, TZ_ERR_HIP, "tz_bound_probe: copy of the delta stack failed");
    TZ_TRY(quantise_rollout(ctx, d_q, mode, b0, b1));
    TZ_TRY(call.out(out, sizeof(tz_frame_quality) * nt, &d_out));
    TZ_TRY(tzk_bound_err(ctx, channels, ctx->d_frames, d_delta, d_q, nt, fe, d_out));
    TZ_TRY(call.finish());
    return tz_stream_sync(ctx);   // (device records too: complete on return)
}

// k_bound_err alone, on any three stacks (tests against tezip_amd/target.py errors_of), in the form the context's payload
// channels select.
extern "C" int tz_bound_err(tz_ctx* ctx, const uint8_t* orig, const int16_t* delta, const int16_t* qdelta, int nframes,
                            size_t frame_elems, tz_frame_quality* out) {
    tz_roctx_range roctx_("tz_bound_err");
    if (!ctx) return TZ_ERR_INVALID;
    if (nframes <= 0 || frame_elems == 0) return TZ_OK;
    if (!orig || !delta || !qdelta || !out) return TZ_ERR_INVALID;
    const size_t n = (size_t)nframes * frame_elems;
    tz_call call(ctx);
    const uint8_t* d_o;
    const int16_t *d_d, *d_q;
    tz_frame_quality* d_out;
    TZ_TRY(call.in(orig, n, &d_o));
    TZ_TRY(call.in(delta, n * 2, &d_d));
    TZ_TRY(call.in(qdelta, n * 2, &d_q));
    TZ_TRY(call.out(out, sizeof(tz_frame_quality) * nframes, &d_out));
    TZ_TRY(tzk_bound_err(ctx, ctx->payload_channels, d_o, d_d, d_q, nframes, frame_elems, d_out));
    TZ_TRY(call.finish());
    return tz_stream_sync(ctx);
}

// The records of `-c --digests`: k_digest of the decoded stack, and of the resident originals when asked for.
extern "C" int tz_encode_digests(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len,
                                 int shuffled, unsigned long long* decoded, unsigned long long* original) {
    tz_roctx_range roctx_("tz_encode_digests");
    if (!ctx || !decoded) return TZ_ERR_INVALID;
    tz_call call(ctx);
    const uint8_t* d_dec;
    unsigned long long* d_out;
    TZ_TRY(encode_decoded(call, "tz_encode_digests", payload, payload_len, table, table_len, shuffled, &d_dec));
    const int nt = ctx->nt;
    const size_t fe = (size_t)ctx->H * ctx->W * 3;
    TZ_TRY(call.out(decoded, sizeof(unsigned long long) * nt, &d_out));
    TZ_TRY(tzk_digest(ctx, d_dec, nt, fe, d_out));
    if (original) {
        TZ_TRY(call.out(original, sizeof(unsigned long long) * nt, &d_out));
        TZ_TRY(tzk_digest(ctx, ctx->d_frames, nt, fe, d_out));
    }
    TZ_TRY(call.finish());
    return tz_stream_sync(ctx);   // (device words too: complete on return)
}

// The records of `-c --report --ssim`: k_ssim of the decoded stack against the originals.
extern "C" int tz_encode_ssim(tz_ctx* ctx, const int16_t* payload, size_t payload_len, const int16_t* table, int table_len,
                              int shuffled, tz_frame_ssim* out) {
    tz_roctx_range roctx_("tz_encode_ssim");
    if (!ctx || !out) return TZ_ERR_INVALID;
    tz_call call(ctx);
    const uint8_t* d_dec;
    tz_frame_ssim* d_out;
    TZ_TRY(encode_decoded(call, "tz_encode_ssim", payload, payload_len, table, table_len, shuffled, &d_dec));
    TZ_TRY(call.out(out, sizeof(tz_frame_ssim) * ctx->nt, &d_out));
    TZ_TRY(tzk_ssim(ctx, d_dec, ctx->d_frames, ctx->nt, ctx->H, ctx->W, d_out));
    TZ_TRY(call.finish());
    return tz_stream_sync(ctx);   // (device records too: complete on return)
}

// TZ-SSIM-1 records of any two unpadded uint8 stacks (tests against tezip_amd/ssim.py).
extern "C" int tz_ssim_frames(tz_ctx* ctx, const uint8_t* a, const uint8_t* b, int nframes, int H, int W, tz_frame_ssim* out) {
    tz_roctx_range roctx_("tz_ssim_frames");
    if (!ctx || nframes < 0 || (nframes > 0 && (!out || !a || !b))) return TZ_ERR_INVALID;
    if (H <= 0 || W <= 0) return tz_fail(ctx, TZ_ERR_INVALID, "frames of %d x %d", H, W);
    const size_t fe = (size_t)H * W * 3;
    if (fe >> 32) return tz_fail(ctx, TZ_ERR_INVALID, "frames of %zu bytes: SSIM covers frames of fewer than 2^32", fe);
    if (nframes == 0) return TZ_OK;
    tz_call call(ctx);
    const uint8_t *d_a, *d_b;
    tz_frame_ssim* d_out;
    TZ_TRY(call.in(a, (size_t)nframes * fe, &d_a));
    TZ_TRY(call.in(b, (size_t)nframes * fe, &d_b));
    TZ_TRY(call.out(out, sizeof(tz_frame_ssim) * nframes, &d_out));
    TZ_TRY(tzk_ssim(ctx, d_a, d_b, nframes, H, W, d_out));
    TZ_TRY(call.finish());
    return tz_stream_sync(ctx);
}

// TZD64 digests of any unpadded uint8 stack (`-u --verify` on the whole-array path; tests against tezip_amd/digest.py).
extern "C" int tz_frame_digests(tz_ctx* ctx, const uint8_t* frames, int nframes, size_t frame_bytes, unsigned long long* out) {
    tz_roctx_range roctx_("tz_frame_digests");
    if (!ctx || nframes < 0 || (nframes > 0 && (!out || (!frames && frame_bytes)))) return TZ_ERR_INVALID;
    if (frame_bytes >> 32) return tz_fail(ctx, TZ_ERR_INVALID, "frames of %zu bytes: a digest covers fewer than 2^32", frame_bytes);
    if (nframes == 0) return TZ_OK;
    tz_call call(ctx);
    const uint8_t* d_in;
    unsigned long long* d_out;
    TZ_TRY(call.in(frames, (size_t)nframes * frame_bytes, &d_in));
    TZ_TRY(call.out(out, sizeof(unsigned long long) * nframes, &d_out));
    TZ_TRY(tzk_digest(ctx, d_in, nframes, frame_bytes, d_out));
    TZ_TRY(call.finish());
    return tz_stream_sync(ctx);
}

// The same over the decoded frames a tz_decode / tz_decode_range with frames_out == NULL left in the context (`-u --verify`
// on the streaming path, before any frame is fetched); frame indices as tz_decoded_get's.
extern "C" int tz_decoded_digests(tz_ctx* ctx, int first, int count, unsigned long long* out) {
    tz_roctx_range roctx_("tz_decoded_digests");
    if (!ctx || !out) return TZ_ERR_INVALID;
    if (!ctx->d_out || !ctx->have_decoded) return tz_fail(ctx, TZ_ERR_STATE, "tz_decoded_digests needs the resident frames of a tz_decode / tz_decode_range");
    if (first < ctx->dec_first || count < 0 || first > ctx->dec_first + ctx->dec_count || count > ctx->dec_first + ctx->dec_count - first)
        return tz_fail(ctx, TZ_ERR_INVALID, "frames [%d, %d + %d) outside the resident decoded stack", first, first, count);
    if (count == 0) return TZ_OK;
    const size_t fsz = (size_t)ctx->H * ctx->W * 3;
    tz_call call(ctx);
    unsigned long long* d_out;
    TZ_TRY(call.out(out, sizeof(unsigned long long) * count, &d_out));
    TZ_TRY(tzk_digest(ctx, ctx->d_out + (size_t)(first - ctx->dec_first) * fsz, count, fsz, d_out));
    TZ_TRY(call.finish());
    return tz_stream_sync(ctx);
}

// ------------------------------------------------------------------ stand-alone operators
extern "C" int tz_delta_encode(tz_ctx* ctx, const float* pred, const uint8_t* orig, const uint8_t* zero_mask, int nframes,
                               int H, int W, int16_t* out) {
    if (!ctx || !pred || !orig || !out || nframes < 0 || H < 1 || W < 1) return TZ_ERR_INVALID;
    int Hp = pad8(H), Wp = pad8(W);
    size_t N = (size_t)nframes * H * W * 3;
    std::vector<uint8_t> zm(nframes, 0);
    if (zero_mask) memcpy(zm.data(), zero_mask, nframes);
    tz_call call(ctx);
    const float* dp;
    const uint8_t* dor;
    uint8_t* dm;
    int16_t* dout;
    TZ_TRY(call.in(pred, (size_t)nframes * Hp * Wp * 3 * 4, &dp));
    TZ_TRY(call.in(orig, N, &dor));
    TZ_TRY(call.alloc(nframes, &dm));
    if (nframes) TZ_TRY(tz_upload(ctx, dm, zm.data(), nframes));
    TZ_TRY(call.out(out, N * 2, &dout));
    TZ_TRY(tzk_delta(ctx, dp, dor, dm, nframes, H, W, Hp, Wp, dout));
    return call.finish();
}

extern "C" int tz_error_bound(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* skip_mask, int nframes, int H,
                              int W, int mode, double b0, double b1) {
    if (!ctx || !orig || !diff || nframes < 0 || H < 1 || W < 1) return TZ_ERR_INVALID;
    size_t N = (size_t)nframes * H * W * 3;
    std::vector<uint8_t> sk(nframes, 0);
    if (skip_mask) memcpy(sk.data(), skip_mask, nframes);
    tz_call call(ctx);
    const uint8_t* dor;
    int16_t* ddiff;
    TZ_TRY(call.in(orig, N, &dor));
    TZ_TRY(call.out(diff, N * 2, &ddiff));
    if (call.outs.back().host) {
        hipError_t e = hipMemcpyAsync(ddiff, diff, N * 2, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "diff upload: %s", hipGetErrorString(e));
    }
    TZ_TRY(tzk_error_bound(ctx, dor, ddiff, sk.data(), nframes, H, W, mode, b0, b1));
    return call.finish();
}

// tz_error_bound in abs mode with one tolerance per frame: the seam of tz_set_frame_bounds
extern "C" int tz_error_bound_frames(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* skip_mask, int nframes, int H,
                                     int W, const double* bounds) {
    if (!ctx || !orig || !diff || nframes < 0 || H < 1 || W < 1 || (nframes > 0 && !bounds)) return TZ_ERR_INVALID;
    for (int f = 0; f < nframes; ++f)
        if (!std::isfinite(bounds[f]) || bounds[f] < 0.0)
            return tz_fail(ctx, TZ_ERR_INVALID, "tz_error_bound_frames: bound %g of frame %d is not a finite number >= 0", bounds[f], f);
    size_t N = (size_t)nframes * H * W * 3;
    std::vector<uint8_t> sk(nframes, 0);
    if (skip_mask) memcpy(sk.data(), skip_mask, nframes);
    tz_call call(ctx);
    const uint8_t* dor;
    int16_t* ddiff;
    TZ_TRY(call.in(orig, N, &dor));
    TZ_TRY(call.out(diff, N * 2, &ddiff));
    if (call.outs.back().host) {
        hipError_t e = hipMemcpyAsync(ddiff, diff, N * 2, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "diff upload: %s", hipGetErrorString(e));
    }
    TZ_TRY(tzk_quant_frames(ctx, dor, ddiff, nullptr, sk.data(), nframes, H, W, bounds, nullptr));
    return call.finish();
}

// The lattice quantiser TZ-QL1 on any stack, in place: tz_error_bound's arguments and refusals (bounds NULL), or
// tz_error_bound_frames' (one abs tolerance per frame).  Independent of the context's quantiser and frame bounds.
static int lattice_seam(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* skip_mask, int nframes, int H, int W, int mode,
                        double b0, double b1, const double* bounds) {
    size_t N = (size_t)nframes * H * W * 3;
    std::vector<uint8_t> sk(nframes, 0);
    if (skip_mask) memcpy(sk.data(), skip_mask, nframes);
    tz_call call(ctx);
    const uint8_t* dor;
    int16_t* ddiff;
    TZ_TRY(call.in(orig, N, &dor));
    TZ_TRY(call.out(diff, N * 2, &ddiff));
    if (call.outs.back().host) {
        hipError_t e = hipMemcpyAsync(ddiff, diff, N * 2, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "diff upload: %s", hipGetErrorString(e));
    }
    TZ_TRY(tzk_lattice(ctx, dor, ddiff, sk.data(), nframes, H, W, mode, b0, b1, bounds));
    return call.finish();
}

extern "C" int tz_lattice_bound(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* skip_mask, int nframes, int H,
                                int W, int mode, double b0, double b1) {
    if (!ctx || !orig || !diff || nframes < 0 || H < 1 || W < 1) return TZ_ERR_INVALID;
    return lattice_seam(ctx, orig, diff, skip_mask, nframes, H, W, mode, b0, b1, nullptr);
}

extern "C" int tz_lattice_bound_frames(tz_ctx* ctx, const uint8_t* orig, int16_t* diff, const uint8_t* skip_mask, int nframes, int H,
                                       int W, const double* bounds) {
    if (!ctx || !orig || !diff || nframes < 0 || H < 1 || W < 1 || (nframes > 0 && !bounds)) return TZ_ERR_INVALID;
    for (int f = 0; f < nframes; ++f)
        if (!std::isfinite(bounds[f]) || bounds[f] < 0.0)
            return tz_fail(ctx, TZ_ERR_INVALID, "tz_lattice_bound_frames: bound %g of frame %d is not a finite number >= 0", bounds[f], f);
    return lattice_seam(ctx, orig, diff, skip_mask, nframes, H, W, TZ_MODE_ABS, 0.0, 0.0, bounds);
}

// The seams of TZ-BM1 (tz_set_bound_map): any int16 stack in place under any H x W map, by the greedy walk (lattice == false) or
// TZ-QL1.  No originals.  Independent of the context's settings.
static int bound_map_seam(tz_ctx* ctx, bool lattice, int16_t* diff, const uint8_t* skip_mask, int nframes, int H, int W, const uint8_t* map) {
    if (!ctx || !diff || !map || nframes < 0 || H < 1 || W < 1) return TZ_ERR_INVALID;
    if (nframes == 0) return TZ_OK;
    size_t N = (size_t)nframes * H * W * 3;
    std::vector<uint8_t> sk(nframes, 0);
    if (skip_mask) memcpy(sk.data(), skip_mask, nframes);
    tz_call call(ctx);
    const uint8_t* dmap;
    int16_t* ddiff;
    TZ_TRY(call.in(map, (size_t)H * W, &dmap));
    TZ_TRY(call.out(diff, N * 2, &ddiff));
    if (call.outs.back().host) {
        hipError_t e = hipMemcpyAsync(ddiff, diff, N * 2, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "diff upload: %s", hipGetErrorString(e));
    }
    if (lattice) TZ_TRY(tzk_lattice(ctx, nullptr, ddiff, sk.data(), nframes, H, W, TZ_MODE_ABS, 0.0, 0.0, nullptr, dmap));
    else TZ_TRY(tzk_quant_map(ctx, nullptr, ddiff, nullptr, sk.data(), nframes, H, W, dmap, nullptr));
    return call.finish();
}

extern "C" int tz_error_bound_map(tz_ctx* ctx, int16_t* diff, const uint8_t* skip_mask, int nframes, int H, int W, const uint8_t* map) {
    return bound_map_seam(ctx, false, diff, skip_mask, nframes, H, W, map);
}

extern "C" int tz_lattice_bound_map(tz_ctx* ctx, int16_t* diff, const uint8_t* skip_mask, int nframes, int H, int W, const uint8_t* map) {
    return bound_map_seam(ctx, true, diff, skip_mask, nframes, H, W, map);
}

// The seams.  Each operation has one body, which takes the layout (tz_internal.h); the exported names of the gray payload
// (tz_set_payload_channels) and of the channel-stride spatial delta (tz_set_delta_stride) state theirs.  A seam at stride 1
// is the flat seam, bytes and messages.
static int check_stride(tz_ctx* ctx, const char* who, int stride) {
    if (stride != 1 && stride != 3) return tz_fail(ctx, TZ_ERR_INVALID, "%s: stride must be 1 or 3, not %d", who, stride);
    return TZ_OK;
}

// n_in elements at `in` -> n_out at `out`, by launch(din, dout, dh) on the device buffers
template <class Launch>
static int delta_seam(tz_ctx* ctx, const int16_t* in, size_t n_in, size_t n_out, int16_t* out, unsigned long long* hist, Launch launch) {
    tz_call call(ctx);
    const int16_t* din;
    int16_t* dout;
    unsigned long long* dh = nullptr;
    TZ_TRY(call.in(in, n_in * 2, &din));
    TZ_TRY(call.out(out, n_out * 2, &dout));
    if (hist) {
        TZ_TRY(call.out(hist, TZ_NBINS * sizeof(unsigned long long), &dh));
        if (call.outs.back().host) {  // counts are ADDED to what the caller holds
            hipError_t e = hipMemcpyAsync(dh, hist, TZ_NBINS * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "hist upload: %s", hipGetErrorString(e));
        }
    }
    TZ_TRY(launch(din, dout, dh));
    return call.finish();
}

// (gray: three interleaved channels in, channel 0's delta out)
static int spatial_delta_seam(tz_ctx* ctx, tz_layout layout, const int16_t* in, size_t n_in, size_t n_out, const int16_t* carry,
                              int apply_offset, int16_t* out, unsigned long long* hist) {
    return delta_seam(ctx, in, n_in, n_out, out, hist, [&](const int16_t* din, int16_t* dout, unsigned long long* dh) {
        return tzk_spatial_delta(ctx, layout, din, n_out, carry, apply_offset, dout, dh, nullptr);
    });
}

extern "C" int tz_spatial_delta(tz_ctx* ctx, const int16_t* in, size_t n, int has_carry, int16_t carry, int apply_offset,
                                int16_t* out, unsigned long long* hist) {
    if (!ctx || !in || !out) return TZ_ERR_INVALID;
    return spatial_delta_seam(ctx, kFlat, in, n, n, has_carry ? &carry : nullptr, apply_offset, out, hist);
}

extern "C" int tz_spatial_delta_gray(tz_ctx* ctx, const int16_t* in3, size_t npix, int has_carry, int16_t carry, int apply_offset,
                                     int16_t* out, unsigned long long* hist) {
    if (!ctx || !in3 || !out) return TZ_ERR_INVALID;
    return spatial_delta_seam(ctx, {1, 1}, in3, npix * 3, npix, has_carry ? &carry : nullptr, apply_offset, out, hist);
}

extern "C" int tz_spatial_delta_stride(tz_ctx* ctx, const int16_t* in, size_t n, int stride, const int16_t* carry, int apply_offset,
                                       int16_t* out, unsigned long long* hist) {
    if (!ctx || !in || !out) return TZ_ERR_INVALID;
    TZ_TRY(check_stride(ctx, "tz_spatial_delta_stride", stride));
    return spatial_delta_seam(ctx, {3, stride}, in, n, n, carry, apply_offset, out, hist);
}

// The seams of TZ-SD2 (tezip_amd/sdelta.py encode_plane / decode_plane) on nframes x H x W x channels elements, channels 3 or 1,
// whatever the context's own setting.
static int check_plane_dims(tz_ctx* ctx, const char* who, int nframes, int H, int W, int channels) {
    if (nframes < 0 || H < 1 || W < 1 || (channels != 1 && channels != 3) || (size_t)H * W > 0x0FFFFFFFull)
        return tz_fail(ctx, TZ_ERR_INVALID, "%s: %d frames of %d x %d with %d channels (channels: 3 or 1)", who, nframes, H, W, channels);
    return TZ_OK;
}

extern "C" int tz_spatial_delta_plane(tz_ctx* ctx, const int16_t* in, int nframes, int H, int W, int channels, int apply_offset,
                                      int16_t* out, unsigned long long* hist) {
    if (!ctx || !in || !out) return TZ_ERR_INVALID;
    TZ_TRY(check_plane_dims(ctx, "tz_spatial_delta_plane", nframes, H, W, channels));
    const size_t n = (size_t)nframes * H * W * channels;
    return delta_seam(ctx, in, n, n, out, hist, [&](const int16_t* din, int16_t* dout, unsigned long long* dh) {
        return tzk_sdelta_plane(ctx, din, channels, nframes, H, W, channels, apply_offset, dout, dh);
    });
}

// table_len -1: `in` holds the spatial delta as stored; else ranks under the table, with the 1600 offset (tz_decode's reading)
extern "C" int tz_spatial_undelta_plane(tz_ctx* ctx, const int16_t* in, int nframes, int H, int W, int channels, const int16_t* table,
                                        int table_len, int16_t* out) {
    if (!ctx || !in || !out) return TZ_ERR_INVALID;
    TZ_TRY(check_plane_dims(ctx, "tz_spatial_undelta_plane", nframes, H, W, channels));
    TZ_TRY(check_table(ctx, table, table_len));
    const size_t n = (size_t)nframes * H * W * channels;
    std::vector<int16_t> lut;
    if (table_len >= 0) build_dec_lut(table, table_len, 1, &lut);
    tz_call call(ctx);
    const int16_t* din;
    int16_t* dout;
    TZ_TRY(call.in(in, n * 2, &din));
    TZ_TRY(call.out(out, n * 2, &dout));
    TZ_TRY(tzk_unplane(ctx, din, nframes, H, W, channels, table_len >= 0 ? lut.data() : nullptr, 1, dout));
    return call.finish();
}

static int lut_op(tz_ctx* ctx, const int16_t* in, size_t n, const std::vector<int16_t>& lut, int post, int16_t* out) {
    tz_call call(ctx);
    const int16_t* din;
    int16_t* dout;
    TZ_TRY(call.in(in, n * 2, &din));
    TZ_TRY(call.out(out, n * 2, &dout));
    TZ_TRY(tzk_lut(ctx, din, n, lut.data(), post, dout));
    return call.finish();
}

extern "C" int tz_remap(tz_ctx* ctx, const int16_t* in, size_t n, const int16_t* table, int table_len, int16_t* out) {
    if (!ctx || !in || !out || !table || table_len < 0 || table_len > TZ_MAX_TABLE) return TZ_ERR_INVALID;
    std::vector<int16_t> lut;
    TZ_TRY(build_enc_lut(ctx, table, table_len, &lut));
    return lut_op(ctx, in, n, lut, 0, out);
}

extern "C" int tz_unmap(tz_ctx* ctx, const int16_t* in, size_t n, const int16_t* table, int table_len, int apply_offset,
                        int16_t* out) {
    if (!ctx || !in || !out || !table || table_len < 0 || table_len > TZ_NBINS) return TZ_ERR_INVALID;
    std::vector<int16_t> lut;
    build_dec_lut(table, table_len, apply_offset, &lut);
    return lut_op(ctx, in, n, lut, apply_offset, out);
}

// (stride 3 ends with a synchronisation that reads the fault word of the scan's bounded poll; the flat seam leaves that to the
// caller's next synchronising call -- an open difference)
static int spatial_undelta_seam(tz_ctx* ctx, int stride, const int16_t* in, size_t n, const int16_t* carry, int16_t* out) {
    tz_call call(ctx);
    const int16_t* din;
    int16_t* dout;
    TZ_TRY(call.in(in, n * 2, &din));
    TZ_TRY(call.out(out, n * 2, &dout));
    TZ_TRY(tzk_undelta(ctx, stride, din, n, carry, nullptr, 0, dout));
    TZ_TRY(call.finish());
    return stride == 3 ? tz_stream_sync(ctx) : TZ_OK;
}

extern "C" int tz_spatial_undelta(tz_ctx* ctx, const int16_t* in, size_t n, int has_carry, int16_t carry, int16_t* out) {
    if (!ctx || !in || !out) return TZ_ERR_INVALID;
    return spatial_undelta_seam(ctx, 1, in, n, has_carry ? &carry : nullptr, out);
}

extern "C" int tz_spatial_undelta_stride(tz_ctx* ctx, const int16_t* in, size_t n, int stride, const int16_t* carry, int16_t* out) {
    if (!ctx || !in || !out) return TZ_ERR_INVALID;
    TZ_TRY(check_stride(ctx, "tz_spatial_undelta_stride", stride));
    return spatial_undelta_seam(ctx, stride, in, n, carry, out);
}

extern "C" int tz_undelta_carry_stride(tz_ctx* ctx, const int16_t* payload, size_t n0, int stride, const int16_t* table, int table_len,
                                       int16_t* carry_out) {
    tz_roctx_range roctx_("tz_undelta_carry_stride");
    if (!ctx || !carry_out) return TZ_ERR_INVALID;
    TZ_TRY(check_stride(ctx, "tz_undelta_carry_stride", stride));
    TZ_TRY(no_plane(ctx, "tz_undelta_carry_stride"));
    if (n0 == 0 || n0 % (size_t)stride)
        return tz_fail(ctx, TZ_ERR_INVALID, "tz_undelta_carry_stride: n0 = %zu is not a positive multiple of the stride %d", n0, stride);
    return undelta_carry_seam(ctx, stride, payload, n0, table, table_len, carry_out);
}

// diff: `channels` deltas per pixel
static int reconstruct_seam(tz_ctx* ctx, int channels, const float* pred, const uint8_t* key_frames, const uint8_t* key_mask,
                            const int16_t* diff, int nframes, int H, int W, uint8_t* out) {
    if (!ctx || !pred || !diff || !out || nframes < 0 || H < 1 || W < 1) return TZ_ERR_INVALID;
    int Hp = pad8(H), Wp = pad8(W);
    size_t N = (size_t)nframes * H * W * 3;
    std::vector<uint8_t> km(nframes, 0);
    if (key_mask && key_frames) memcpy(km.data(), key_mask, nframes);
    tz_call call(ctx);
    const float* dp;
    const uint8_t* dk = nullptr;
    const int16_t* dd;
    uint8_t *dm, *dout;
    TZ_TRY(call.in(pred, (size_t)nframes * Hp * Wp * 3 * 4, &dp));
    if (key_frames) TZ_TRY(call.in(key_frames, N, &dk));
    TZ_TRY(call.in(diff, N / 3 * channels * 2, &dd));
    TZ_TRY(call.alloc(nframes, &dm));
    if (nframes) TZ_TRY(tz_upload(ctx, dm, km.data(), nframes));
    TZ_TRY(call.out(out, N, &dout));
    TZ_TRY(tzk_reconstruct(ctx, channels, dp, dk, dm, dd, nframes, H, W, Hp, Wp, dout));
    return call.finish();
}

extern "C" int tz_reconstruct(tz_ctx* ctx, const float* pred, const uint8_t* key_frames, const uint8_t* key_mask,
                              const int16_t* diff, int nframes, int H, int W, uint8_t* out) {
    return reconstruct_seam(ctx, 3, pred, key_frames, key_mask, diff, nframes, H, W, out);
}

extern "C" int tz_reconstruct_gray(tz_ctx* ctx, const float* pred, const uint8_t* key_frames, const uint8_t* key_mask,
                                   const int16_t* diff1, int nframes, int H, int W, uint8_t* out) {
    return reconstruct_seam(ctx, 1, pred, key_frames, key_mask, diff1, nframes, H, W, out);
}

extern "C" int tz_window_sse(tz_ctx* ctx, const uint8_t* orig, const float* pred, int nframes, int H, int W, double* sse) {
    if (!ctx || !orig || !pred || !sse || nframes < 0 || H < 1 || W < 1) return TZ_ERR_INVALID;
    int Hp = pad8(H), Wp = pad8(W);
    tz_call call(ctx);
    const uint8_t* dor;
    const float* dp;
    TZ_TRY(call.in(orig, (size_t)nframes * H * W * 3, &dor));
    TZ_TRY(call.in(pred, (size_t)nframes * Hp * Wp * 3 * 4, &dp));
    return tzk_sse(ctx, dor, dp, nframes, H, W, Hp, Wp, sse);
}

// --------------------------------------------------------------------------- Huffman coder
// Opt-in entropy coder of the payload (`--coder huff`; NOT a reference feature: compress.py:375-400 hands the int16 payload
// to zstd).  Format and geometry: DESIGN.md section 9; kernels: tz_codec.hip.
//
// tz_huff_lengths: optimal code lengths under the limit max_len by PACKAGE-MERGE (Larmore & Hirschberg 1990), the plain
// list form: level j holds the leaves merged by weight with the pairs ("packages") of level j - 1; the first 2m - 2 items
// of the last level are taken, a taken package takes its two items one level down, and a symbol's length is the number of
// levels on which its leaf is taken.  Leaves are merged in ascending (count, then descending symbol) order and a leaf goes
// before a package of equal weight, so the result is a function of the counts alone, the taken leaves of a level are a
// prefix of that order (lengths never increase with the count), and the code is complete (Kraft sum exactly 1).
static int huff_package_merge(const unsigned long long* counts, int A, int max_a, int max_len, uint8_t* lengths) {
    if (!counts || !lengths || A < 1 || A > max_a || max_len < 1 || max_len > 15) return TZ_ERR_INVALID;
    std::vector<int> sym;
    unsigned long long total = 0;
    for (int s = 0; s < A; ++s) {
        lengths[s] = 0;
        if (!counts[s]) continue;
        if (counts[s] >= (1ull << 58) || total + counts[s] >= (1ull << 58)) return TZ_ERR_INVALID;   // (weights are summed over <= 15 levels)
        total += counts[s];
        sym.push_back(s);
    }
    const size_t m = sym.size();
    if (m == 0 || m > ((size_t)1 << max_len)) return TZ_ERR_INVALID;
    if (m == 1) {
        lengths[sym[0]] = 1;
        return TZ_OK;
    }
    std::sort(sym.begin(), sym.end(), [&](int a, int b) { return counts[a] != counts[b] ? counts[a] < counts[b] : a > b; });
    std::vector<std::vector<unsigned long long>> w(max_len);
    std::vector<std::vector<uint8_t>> leaf(max_len);
    for (int j = 0; j < max_len; ++j) {
        const size_t npk = j ? w[j - 1].size() / 2 : 0;
        size_t a = 0, b = 0;
        while (a < m || b < npk) {
            const unsigned long long wp = b < npk ? w[j - 1][2 * b] + w[j - 1][2 * b + 1] : 0;
            if (a < m && (b >= npk || counts[sym[a]] <= wp)) {
                w[j].push_back(counts[sym[a++]]);
                leaf[j].push_back(1);
            } else {
                w[j].push_back(wp);
                leaf[j].push_back(0);
                ++b;
            }
        }
    }
    size_t take = 2 * m - 2;
    for (int j = max_len - 1; j >= 0 && take; --j) {
        if (take > w[j].size()) return TZ_ERR_INVALID;   // (cannot happen for m <= 2^max_len)
        size_t q = 0;
        for (size_t i = 0; i < take; ++i) q += leaf[j][i];
        for (size_t i = 0; i < q; ++i) lengths[sym[i]] += 1;
        take = 2 * (take - q);
    }
    return TZ_OK;
}

extern "C" int tz_huff_lengths(const unsigned long long* counts, int A, int max_len, uint8_t* lengths) {
    return huff_package_merge(counts, A, TZ_NBINS, max_len, lengths);
}

// the same over the symbols of a TZR1 code: `total` = literals + the TZ_HUFFR_NTOK repeat tokens behind them
extern "C" int tz_huffr_lengths(const unsigned long long* counts, int total, int max_len, uint8_t* lengths) {
    if (total <= TZ_HUFFR_NTOK) return TZ_ERR_INVALID;
    return huff_package_merge(counts, total, TZ_NBINS + TZ_HUFFR_NTOK, max_len, lengths);
}

// the repeat tokens behind the literals of a code at the match distance dist (0: a stream without tokens)
static int huff_ntok(int dist) { return dist ? TZ_HUFFR_NTOK : 0; }

// The two tables of a code given by its lengths (canonical: shorter first, then by symbol; stored bit-reversed):
// enc[s] = stored code | length << 12 (0: absent), dec[next 12 bits] = symbol | length << 12.  Checks everything a launch
// depends on: A, base, lengths <= 12, at least one symbol, Kraft sum <= 1.  dist: the match distance of the stream (see HuffFmt
// below); a tokenised one (dist != 0) has TZ_HUFFR_NTOK more symbols in `lengths` behind the A literals, the repeat tokens; A
// and base still describe the literals, one of which must be present.
static int huff_tables(tz_ctx* ctx, const uint8_t* lengths, int A, int base, std::vector<uint16_t>* enc, std::vector<uint16_t>* dec, int dist) {
    if (!lengths || A < 1 || A > TZ_NBINS) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: alphabet size %d outside [1, %d]", A, TZ_NBINS);
    if (base < -32768 || base + A - 1 > 32767) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: base %d with %d symbols leaves int16", base, A);
    unsigned long long kraft = 0;
    int first = -1;
    const int lits = A;
    A += huff_ntok(dist);
    for (int s = 0; s < A; ++s) {
        if (lengths[s] > TZ_HUFF_L) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: code length %d of symbol %d exceeds %d", lengths[s], s, TZ_HUFF_L);
        if (lengths[s]) {
            kraft += 1ull << (TZ_HUFF_L - lengths[s]);
            if (first < 0) first = s;
        }
    }
    if (first < 0 || first >= lits) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: the code lengths name no symbol");
    if (kraft > (1ull << TZ_HUFF_L)) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: Kraft sum of the code lengths exceeds 1");
    if (enc) enc->assign(A, 0);
    if (dec) dec->assign((size_t)1 << TZ_HUFF_L, (uint16_t)(first | (1 << 12)));   // unreachable entries: a valid symbol, length 1
    unsigned code = 0;
    for (int l = 1; l <= TZ_HUFF_L; ++l) {
        for (int s = 0; s < A; ++s) {
            if (lengths[s] != l) continue;
            unsigned rev = 0;
            for (int b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
            ++code;
            if (enc) (*enc)[s] = (uint16_t)(rev | (l << 12));
            if (dec)
                for (unsigned k = 0; k < (1u << (TZ_HUFF_L - l)); ++k) (*dec)[rev | (k << l)] = (uint16_t)(s | (l << 12));
        }
        code <<= 1;
    }
    return TZ_OK;
}

static void huff_geometry(size_t n, size_t* nruns, size_t* nchunks, size_t* index_bytes) {
    *nruns = (n + TZ_HUFF_RUN - 1) / TZ_HUFF_RUN;
    *nchunks = (*nruns + TZ_HUFF_CHUNK_RUNS - 1) / TZ_HUFF_CHUNK_RUNS;
    *index_bytes = *nchunks * 4 + ((*nruns * 2 + 3) & ~(size_t)3);
}

// d_in (device, n int16) -> ctx->d_huff = index | bits; *bytes its size.  Waits once, for the size of the bit stream.
// dist: the match distance, 0 for a stream without tokens (k_huff_size / k_huff_enc), else 1 or 3 (lengths then holds A +
// TZ_HUFFR_NTOK entries, k_huffr_size / k_huffr_enc at that distance).
// keys: the stream goes to the key-frame coder's buffer ctx->d_keys instead, and what the entropy coders hold stays.
static int huff_encode_dev(tz_ctx* ctx, const int16_t* d_in, size_t n, const uint8_t* lengths, int A, int base, size_t* bytes, int dist,
                           bool keys) {
    if (n < 1 || n >= ((size_t)1 << 40)) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: %zu elements outside [1, 2^40)", n);
    std::vector<uint16_t> enc;
    TZ_TRY(huff_tables(ctx, lengths, A, base, &enc, nullptr, dist));
    size_t nruns, nchunks, index_bytes;
    huff_geometry(n, &nruns, &nchunks, &index_bytes);
    void *d_enc, *d_idx, *d_meta;
    TZ_TRY(tz_pool_alloc(ctx, enc.size() * 2, &d_enc));
    TZ_TRY(tz_pool_alloc(ctx, index_bytes, &d_idx));
    TZ_TRY(tz_pool_alloc(ctx, sizeof(tz_huff_meta), &d_meta));
    TZ_TRY(tz_upload(ctx, d_enc, enc.data(), enc.size() * 2));
    TZ_HIP(ctx, hipMemsetAsync(d_idx, 0, index_bytes, ctx->stream));   // (the padding behind an odd number of run sizes is part of the file)
    unsigned* d_chunk_off = (unsigned*)d_idx;
    uint16_t* d_run_bits = (uint16_t*)((uint8_t*)d_idx + nchunks * 4);
    TZ_TRY(tzk_huff_size(ctx, d_in, n, (const uint16_t*)d_enc, A, base, d_run_bits, d_chunk_off, (tz_huff_meta*)d_meta, dist));
    tz_huff_meta meta;
    TZ_TRY(tz_d2h(ctx, &meta, d_meta, sizeof(meta), ctx->stream));
    TZ_TRY(tz_stream_sync(ctx));
    if (meta.bad) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: the payload holds a value the code lengths give no code");
    if (meta.total_words >= (1ull << 32)) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: a bit stream of %llu words does not fit the format", meta.total_words);
    const size_t total = index_bytes + (size_t)meta.total_words * 4;
    uint8_t* d_stream;
    if (keys) {
        ctx->keys_kind = tz_ctx::KEYS_NONE;   // (a staged decoder stream, if any, is gone)
        TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_keys, &ctx->cap_keys, total));
        ctx->keys_bytes = total;
        d_stream = ctx->d_keys;
    } else {
        ctx->huff_kind = tz_ctx::HUFF_NONE;
        TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_huff, &ctx->cap_huff, total));
        ctx->huff_bytes = total;
        d_stream = ctx->d_huff;
    }
    TZ_HIP(ctx, hipMemcpyAsync(d_stream, d_idx, index_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    TZ_TRY(tzk_huff_enc(ctx, d_in, n, (const uint16_t*)d_enc, A, base, d_run_bits, d_chunk_off, (unsigned*)(d_stream + index_bytes),
                        (size_t)meta.total_words, dist));
    *bytes = total;
    return TZ_OK;
}

// what a stream of `bytes` bytes must satisfy to be the index | bits of n elements; *stream_words its bit stream
static int huff_check_stream(tz_ctx* ctx, size_t bytes, size_t n, int R, size_t* stream_words) {
    if (R != TZ_HUFF_RUN) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: run length %d, this build codes runs of %d", R, TZ_HUFF_RUN);
    if (n < 1 || n >= ((size_t)1 << 40)) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: %zu elements outside [1, 2^40)", n);
    size_t nruns, nchunks, index_bytes;
    huff_geometry(n, &nruns, &nchunks, &index_bytes);
    if (bytes < index_bytes || ((bytes - index_bytes) & 3) || (bytes - index_bytes) / 4 >= ((size_t)1 << 32))
        return tz_fail(ctx, TZ_ERR_INVALID, "huffman: a stream of %zu bytes cannot hold the %zu-byte index of %zu elements and whole words", bytes,
                       index_bytes, n);
    *stream_words = (bytes - index_bytes) / 4;
    return TZ_OK;
}

static int huff_decode_dev(tz_ctx* ctx, const uint8_t* d_stream, size_t stream_words, size_t n, const std::vector<uint16_t>& dec, int A, int base,
                           int dist, int16_t* d_out) {
    size_t nruns, nchunks, index_bytes;
    huff_geometry(n, &nruns, &nchunks, &index_bytes);
    void* d_dec;
    TZ_TRY(tz_pool_alloc(ctx, dec.size() * 2, &d_dec));
    TZ_TRY(tz_upload(ctx, d_dec, dec.data(), dec.size() * 2));
    return tzk_huff_dec(ctx, (const unsigned*)d_stream, (const uint16_t*)(d_stream + nchunks * 4), (const unsigned*)(d_stream + index_bytes),
                        stream_words, (const uint16_t*)d_dec, A, base, n, d_out, dist);
}

// One body per entry point of the three entropy coders, which are ONE coder at three match distances: what tells them apart
// is a HuffFmt.  dist == 0: no element matches, the stream is the plain one of the k_huff_* kernels and `lengths` holds A
// bytes (`--coder huff`, TZH1).  dist == 1 or 3: the runs are tokenised first (tezip_amd/huffr.py), the k_huffr_* kernels run at
// that distance and `lengths` holds A + 8 bytes (`--coder huffr`, TZR1, is dist == 3).  `--coder huffd` (TZR2,
// tezip_amd/huffd.py) names its distance D per stream: 0, 1 or 3, `lengths` always A + 8 bytes, the eight token lengths 0 under
// D == 0.  `who` is the entry point's family for the messages.  All stage into the same buffers; ctx->huff_kind says which
// format's begin did, so each put and decode refuses another's stream (a TZR1 stream and a TZR2 one at D == 3 too), and
// ctx->huff_dist holds the staged stream's distance, which is all that decode needs to pick its kernel.
struct HuffFmt {
    tz_ctx::tz_huff_kind kind;
    int dist;
    const char* who;
};
static constexpr HuffFmt FMT_TZH1{tz_ctx::HUFF_TZH1, 0, "tz_huff"}, FMT_TZR1{tz_ctx::HUFF_TZR1, 3, "tz_huffr"};
// (a TZR2 descriptor exists per stream only, huffd_family fills it: put and decode, which know no D, take the kind and the name)

typedef int (*huff_count_launch)(tz_ctx*, const int16_t*, size_t, unsigned long long*, tz_huff_meta*);

// the counts of n device elements, `rows` rows (1, or huffd's 3: match distance 0 | 1 | 3) of TZ_NBINS + ntok entries as `launch`
// leaves them: the A literals from the lowest to the highest value present, then the ntok tokens, then zeros
static int huff_counts_dev(tz_ctx* ctx, const char* who, int ntok, int rows, huff_count_launch launch, const int16_t* d_in, size_t n,
                           unsigned long long* counts, int* A, int* base) {
    const int BINS = TZ_HUFF_COUNT_BINS + ntok, ROW = TZ_NBINS + ntok;
    void *d_hist, *d_meta;
    std::vector<unsigned long long> h((size_t)rows * BINS);
    tz_huff_meta meta;
    TZ_TRY(tz_pool_alloc(ctx, h.size() * sizeof(unsigned long long), &d_hist));
    TZ_TRY(tz_pool_alloc(ctx, sizeof(tz_huff_meta), &d_meta));
    TZ_TRY(launch(ctx, d_in, n, (unsigned long long*)d_hist, (tz_huff_meta*)d_meta));
    TZ_TRY(tz_d2h(ctx, h.data(), d_hist, h.size() * sizeof(unsigned long long), ctx->stream));
    TZ_TRY(tz_d2h(ctx, &meta, d_meta, sizeof(meta), ctx->stream));
    TZ_TRY(tz_stream_sync(ctx));
    // Row 0 alone gives the span.  Every value of a run is a literal at its first occurrence there, so the literals of a
    // tokenised row span the values; huffd's row 0 counts every element, and its other rows' literals span the same values.
    int lo = -1, hi = -1;
    for (int b = 0; b < TZ_HUFF_COUNT_BINS; ++b)
        if (h[b]) {
            if (lo < 0) lo = b;
            hi = b;
        }
    if (meta.bad || lo < 0 || hi - lo + 1 > TZ_NBINS)
        return tz_fail(ctx, TZ_ERR_INVALID, "%s_counts: the payload's values span more than %d symbols", who, TZ_NBINS);
    const int a = hi - lo + 1;
    for (int d = 0; d < rows; ++d)
        for (int s = 0; s < ROW; ++s)
            counts[d * ROW + s] = s < a ? h[d * BINS + lo + s] : s < a + ntok ? h[d * BINS + TZ_HUFF_COUNT_BINS + s - a] : 0;
    *A = a;
    *base = lo - TZ_HUFF_COUNT_BIAS;
    return TZ_OK;
}

// in == NULL: the resident payload; else a stand-alone host or device array of n elements
static int huff_counts(tz_ctx* ctx, const char* who, int ntok, int rows, huff_count_launch launch, const int16_t* in, size_t n,
                       unsigned long long* counts, int* A, int* base) {
    if (!ctx || !counts || !A || !base) return TZ_ERR_INVALID;
    tz_call call(ctx);
    const int16_t* din = ctx->d_payload;
    if (!in) {
        if (!ctx->d_payload || !ctx->payload_len)
            return tz_fail(ctx, TZ_ERR_STATE, "%s_counts needs a resident payload (tz_encode with payload == NULL)", who);
        n = ctx->payload_len;
    } else if (n < 1 || n >= ((size_t)1 << 40)) {
        return tz_fail(ctx, TZ_ERR_INVALID, "huffman: %zu elements outside [1, 2^40)", n);
    } else {
        TZ_TRY(call.in(in, n * 2, &din));
    }
    return huff_counts_dev(ctx, who, ntok, rows, launch, din, n, counts, A, base);
}

static int huff_encode(tz_ctx* ctx, const HuffFmt& f, const uint8_t* lengths, int A, int base, size_t* bytes) {
    if (!ctx || !bytes) return TZ_ERR_INVALID;
    if (!ctx->d_payload || !ctx->payload_len) return tz_fail(ctx, TZ_ERR_STATE, "%s_encode needs a resident payload (tz_encode with payload == NULL)", f.who);
    tz_call call(ctx);
    return huff_encode_dev(ctx, ctx->d_payload, ctx->payload_len, lengths, A, base, bytes, f.dist, false);
}

static int huff_begin(tz_ctx* ctx, const HuffFmt& f, size_t bytes, size_t n, const uint8_t* lengths, int A, int base, int R) {
    if (!ctx) return TZ_ERR_INVALID;
    size_t sw;
    TZ_TRY(huff_check_stream(ctx, bytes, n, R, &sw));
    std::vector<uint16_t> dec;
    TZ_TRY(huff_tables(ctx, lengths, A, base, nullptr, &dec, f.dist));
    ctx->huff_kind = tz_ctx::HUFF_NONE;
    ctx->enc_kind = tz_ctx::ENC_NONE;   // d_payload is about to receive the expanded stream
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_huff, &ctx->cap_huff, std::max<size_t>(bytes, 16)));
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_payload, &ctx->cap_payload, std::max<size_t>(n, 8) * 2));
    ctx->payload_len = 0;
    ctx->huff_bytes = bytes;
    ctx->huff_dec_tab.swap(dec);
    ctx->huff_base = base;
    ctx->huff_A = A;
    ctx->huff_n = n;
    ctx->huff_dist = f.dist;
    ctx->huff_kind = f.kind;
    TZ_HIP(ctx, hipEventRecord(ctx->ev_compute, ctx->stream));  // earlier work may still read the old stream
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute, 0));
    return TZ_OK;
}

static int huff_put(tz_ctx* ctx, tz_ctx::tz_huff_kind kind, size_t offset, size_t count, const uint8_t* src) {
    if (!ctx || !src) return TZ_ERR_INVALID;
    if (!ctx->d_huff || ctx->huff_kind != kind || offset > ctx->huff_bytes || count > ctx->huff_bytes - offset)
        return tz_fail(ctx, TZ_ERR_INVALID, "byte range outside the staged Huffman stream");
    return tz_h2d(ctx, ctx->d_huff + offset, src, count, ctx->copy_stream);
}

static int huff_decode(tz_ctx* ctx, tz_ctx::tz_huff_kind kind, const char* who) {
    if (!ctx) return TZ_ERR_INVALID;
    if (ctx->huff_kind != kind || !ctx->d_huff || !ctx->d_payload || ctx->cap_payload < ctx->huff_n * 2)
        return tz_fail(ctx, TZ_ERR_STATE, "%s_decode needs a stream staged with %s_begin / %s_put", who, who, who);
    size_t sw;
    TZ_TRY(huff_check_stream(ctx, ctx->huff_bytes, ctx->huff_n, TZ_HUFF_RUN, &sw));
    TZ_HIP(ctx, hipEventRecord(ctx->ev_frames, ctx->copy_stream));   // the pieces of the puts
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_frames, 0));
    tz_call call(ctx);
    TZ_TRY(huff_decode_dev(ctx, ctx->d_huff, sw, ctx->huff_n, ctx->huff_dec_tab, ctx->huff_A, ctx->huff_base, ctx->huff_dist, ctx->d_payload));
    ctx->payload_len = ctx->huff_n;   // exactly as if tz_payload_begin / tz_payload_put had staged them
    return TZ_OK;
}

static int huff_encode_buf(tz_ctx* ctx, const HuffFmt& f, const int16_t* in, size_t n, const uint8_t* lengths, int A, int base, uint8_t* out,
                           size_t capacity, size_t* bytes) {
    if (!ctx || !in || !out || !bytes) return TZ_ERR_INVALID;
    if (n < 1 || n >= ((size_t)1 << 40)) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: %zu elements outside [1, 2^40)", n);
    tz_call call(ctx);
    const int16_t* din;
    TZ_TRY(call.in(in, n * 2, &din));
    TZ_TRY(huff_encode_dev(ctx, din, n, lengths, A, base, bytes, f.dist, false));
    if (*bytes > capacity) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: the stream needs %zu bytes, the buffer holds %zu", *bytes, capacity);
    if (tz_is_device_ptr(out)) {
        hipError_t e = hipMemcpyAsync(out, ctx->d_huff, *bytes, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) return tz_fail(ctx, TZ_ERR_HIP, "stream copy: %s", hipGetErrorString(e));
    } else {
        TZ_TRY(tz_d2h(ctx, out, ctx->d_huff, *bytes, ctx->stream));
    }
    return tz_stream_sync(ctx);
}

// The stand-alone forms that turn one host or device array into another: `in` is made a device array, `out` one to be copied
// back if it is none, run(device in, device out) launches under the scope opened here, the copy back and the stream are awaited.
// A device array whose address has a bit of in_mask / out_mask set is refused with `misaligned`.
template <class F>
static int buf_op(tz_ctx* ctx, const void* in, size_t in_bytes, unsigned in_mask, void* out, size_t out_bytes, unsigned out_mask,
                  const char* misaligned, F&& run) {
    tz_call call(ctx);
    const void* din;
    void* dout;
    TZ_TRY(call.in(in, in_bytes, &din));
    if ((uintptr_t)din & in_mask) return tz_fail(ctx, TZ_ERR_INVALID, "%s", misaligned);
    TZ_TRY(call.out(out, out_bytes, &dout));
    if ((uintptr_t)dout & out_mask) return tz_fail(ctx, TZ_ERR_INVALID, "%s", misaligned);
    TZ_TRY(run(din, dout));
    TZ_TRY(call.finish());
    return call.outs.back().host ? TZ_OK : tz_stream_sync(ctx);
}

static int huff_decode_buf(tz_ctx* ctx, const HuffFmt& f, const uint8_t* stream, size_t bytes, size_t n, const uint8_t* lengths, int A, int base,
                           int R, int16_t* out) {
    if (!ctx || !stream || !out) return TZ_ERR_INVALID;
    size_t sw;
    TZ_TRY(huff_check_stream(ctx, bytes, n, R, &sw));
    std::vector<uint16_t> dec;
    TZ_TRY(huff_tables(ctx, lengths, A, base, nullptr, &dec, f.dist));
    return buf_op(ctx, stream, bytes, 3, out, n * 2, 0, "huffman: a device stream must be 4-byte aligned", [&](const void* din, void* dout) {
        return huff_decode_dev(ctx, (const uint8_t*)din, sw, n, dec, A, base, f.dist, (int16_t*)dout);
    });
}

extern "C" int tz_huff_counts(tz_ctx* ctx, unsigned long long* counts, int* A, int* base) {
    tz_roctx_range roctx_("tz_huff_counts");
    return huff_counts(ctx, "tz_huff", 0, 1, tzk_huff_count, nullptr, 0, counts, A, base);
}

extern "C" int tz_huff_encode(tz_ctx* ctx, const uint8_t* lengths, int A, int base, size_t* bytes) {
    tz_roctx_range roctx_("tz_huff_encode");
    return huff_encode(ctx, FMT_TZH1, lengths, A, base, bytes);
}

extern "C" int tz_huff_get(tz_ctx* ctx, size_t offset, size_t count, uint8_t* out) {
    if (!ctx || !out) return TZ_ERR_INVALID;
    if (!ctx->d_huff || offset > ctx->huff_bytes || count > ctx->huff_bytes - offset)
        return tz_fail(ctx, TZ_ERR_INVALID, "byte range outside the resident Huffman stream");
    TZ_TRY(tz_d2h(ctx, out, ctx->d_huff + offset, count, ctx->stream));
    return tz_stream_sync(ctx);
}

extern "C" int tz_huff_begin(tz_ctx* ctx, size_t bytes, size_t n, const uint8_t* lengths, int A, int base, int R) {
    return huff_begin(ctx, FMT_TZH1, bytes, n, lengths, A, base, R);
}

extern "C" int tz_huff_put(tz_ctx* ctx, size_t offset, size_t count, const uint8_t* src) { return huff_put(ctx, tz_ctx::HUFF_TZH1, offset, count, src); }

extern "C" int tz_huff_decode(tz_ctx* ctx) {
    tz_roctx_range roctx_("tz_huff_decode");
    return huff_decode(ctx, tz_ctx::HUFF_TZH1, "tz_huff");
}

extern "C" int tz_huff_encode_buf(tz_ctx* ctx, const int16_t* in, size_t n, const uint8_t* lengths, int A, int base, uint8_t* out,
                                  size_t capacity, size_t* bytes) {
    return huff_encode_buf(ctx, FMT_TZH1, in, n, lengths, A, base, out, capacity, bytes);
}

extern "C" int tz_huff_decode_buf(tz_ctx* ctx, const uint8_t* stream, size_t bytes, size_t n, const uint8_t* lengths, int A, int base, int R,
                                  int16_t* out) {
    return huff_decode_buf(ctx, FMT_TZH1, stream, bytes, n, lengths, A, base, R, out);
}

extern "C" int tz_huffr_counts(tz_ctx* ctx, unsigned long long* counts, int* A, int* base) {
    tz_roctx_range roctx_("tz_huffr_counts");
    return huff_counts(ctx, "tz_huffr", TZ_HUFFR_NTOK, 1, tzk_huffr_count, nullptr, 0, counts, A, base);
}

extern "C" int tz_huffr_encode(tz_ctx* ctx, const uint8_t* lengths, int A, int base, size_t* bytes) {
    tz_roctx_range roctx_("tz_huffr_encode");
    return huff_encode(ctx, FMT_TZR1, lengths, A, base, bytes);
}

extern "C" int tz_huffr_get(tz_ctx* ctx, size_t offset, size_t count, uint8_t* out) { return tz_huff_get(ctx, offset, count, out); }

extern "C" int tz_huffr_begin(tz_ctx* ctx, size_t bytes, size_t n, const uint8_t* lengths, int A, int base, int R) {
    return huff_begin(ctx, FMT_TZR1, bytes, n, lengths, A, base, R);
}

extern "C" int tz_huffr_put(tz_ctx* ctx, size_t offset, size_t count, const uint8_t* src) {
    return huff_put(ctx, tz_ctx::HUFF_TZR1, offset, count, src);
}

extern "C" int tz_huffr_decode(tz_ctx* ctx) {
    tz_roctx_range roctx_("tz_huffr_decode");
    return huff_decode(ctx, tz_ctx::HUFF_TZR1, "tz_huffr");
}

extern "C" int tz_huffr_encode_buf(tz_ctx* ctx, const int16_t* in, size_t n, const uint8_t* lengths, int A, int base, uint8_t* out,
                                   size_t capacity, size_t* bytes) {
    return huff_encode_buf(ctx, FMT_TZR1, in, n, lengths, A, base, out, capacity, bytes);
}

extern "C" int tz_huffr_decode_buf(tz_ctx* ctx, const uint8_t* stream, size_t bytes, size_t n, const uint8_t* lengths, int A, int base, int R,
                                   int16_t* out) {
    return huff_decode_buf(ctx, FMT_TZR1, stream, bytes, n, lengths, A, base, R, out);
}

// the counts of a stand-alone host or device array, as tz_huffr_counts gives them for the resident payload
extern "C" int tz_huffr_counts_buf(tz_ctx* ctx, const int16_t* in, size_t n, unsigned long long* counts, int* A, int* base) {
    return in ? huff_counts(ctx, "tz_huffr", TZ_HUFFR_NTOK, 1, tzk_huffr_count, in, n, counts, A, base) : TZ_ERR_INVALID;
}

// ---- `--coder huffd` (TZR2): the coder that picks its match distance
// D must be 0, 1 or 3, and the eight token lengths of D = 0 must be 0; *f = the descriptor of a TZR2 stream at that distance
static int huffd_family(tz_ctx* ctx, int D, const uint8_t* lengths, int A, HuffFmt* f) {
    if (D != 0 && D != 1 && D != 3) return tz_fail(ctx, TZ_ERR_INVALID, "tz_huffd: match distance %d, the format knows 0 (no tokens), 1 and 3", D);
    *f = HuffFmt{tz_ctx::HUFF_TZR2, D, "tz_huffd"};
    if (D == 0 && lengths && A >= 1 && A <= TZ_NBINS)
        for (int k = 0; k < TZ_HUFFR_NTOK; ++k)
            if (lengths[A + k]) return tz_fail(ctx, TZ_ERR_INVALID, "tz_huffd: match distance 0 with a code length %d for the token T_%d", lengths[A + k], k);
    return TZ_OK;
}

// counts: three rows of TZ_NBINS + 8 entries (match distance 0 | 1 | 3), each the A literals, then T_0..T_7, then zeros
extern "C" int tz_huffd_counts(tz_ctx* ctx, unsigned long long* counts, int* A, int* base) {
    tz_roctx_range roctx_("tz_huffd_counts");
    return huff_counts(ctx, "tz_huffd", TZ_HUFFR_NTOK, 3, tzk_huffd_count, nullptr, 0, counts, A, base);
}

extern "C" int tz_huffd_counts_buf(tz_ctx* ctx, const int16_t* in, size_t n, unsigned long long* counts, int* A, int* base) {
    return in ? huff_counts(ctx, "tz_huffd", TZ_HUFFR_NTOK, 3, tzk_huffd_count, in, n, counts, A, base) : TZ_ERR_INVALID;
}

extern "C" int tz_huffd_encode(tz_ctx* ctx, const uint8_t* lengths, int A, int base, int D, size_t* bytes) {
    tz_roctx_range roctx_("tz_huffd_encode");
    if (!ctx || !bytes) return TZ_ERR_INVALID;
    HuffFmt f;
    TZ_TRY(huffd_family(ctx, D, lengths, A, &f));
    return huff_encode(ctx, f, lengths, A, base, bytes);
}

extern "C" int tz_huffd_get(tz_ctx* ctx, size_t offset, size_t count, uint8_t* out) { return tz_huff_get(ctx, offset, count, out); }

extern "C" int tz_huffd_begin(tz_ctx* ctx, size_t bytes, size_t n, const uint8_t* lengths, int A, int base, int R, int D) {
    if (!ctx) return TZ_ERR_INVALID;
    HuffFmt f;
    TZ_TRY(huffd_family(ctx, D, lengths, A, &f));
    return huff_begin(ctx, f, bytes, n, lengths, A, base, R);
}

extern "C" int tz_huffd_put(tz_ctx* ctx, size_t offset, size_t count, const uint8_t* src) {
    return huff_put(ctx, tz_ctx::HUFF_TZR2, offset, count, src);
}

extern "C" int tz_huffd_decode(tz_ctx* ctx) {
    tz_roctx_range roctx_("tz_huffd_decode");
    return huff_decode(ctx, tz_ctx::HUFF_TZR2, "tz_huffd");
}

extern "C" int tz_huffd_encode_buf(tz_ctx* ctx, const int16_t* in, size_t n, const uint8_t* lengths, int A, int base, int D, uint8_t* out,
                                   size_t capacity, size_t* bytes) {
    if (!ctx) return TZ_ERR_INVALID;
    HuffFmt f;
    TZ_TRY(huffd_family(ctx, D, lengths, A, &f));
    return huff_encode_buf(ctx, f, in, n, lengths, A, base, out, capacity, bytes);
}

extern "C" int tz_huffd_decode_buf(tz_ctx* ctx, const uint8_t* stream, size_t bytes, size_t n, const uint8_t* lengths, int A, int base, int R,
                                   int D, int16_t* out) {
    if (!ctx) return TZ_ERR_INVALID;
    HuffFmt f;
    TZ_TRY(huffd_family(ctx, D, lengths, A, &f));
    return huff_decode_buf(ctx, f, stream, bytes, n, lengths, A, base, R, out);
}

// --------------------------------------------------------------------------- the size of a candidate bound (TZ-TRATIO-1)
// `-c --target-ratio` (NOT a reference feature; DESIGN.md section 9, tezip_amd/ratetarget.py): with a GPU coder the size of
// entropy.dat is an exact function of integer counts, so a candidate bound costs a quantiser run and two reads of its output
// (k_size_count, k_size_bits) -- no spatial delta stack, no remapped payload, no index, no bit stream.  Between the two kernels
// the host does what the real job does between tz_encode, tz_<coder>_counts and tz_<coder>_encode, on counts: the rank table
// from the plain histogram (tz_build_table), the counts permuted by it (the remap is a bijection on the symbols present, so
// the token histograms of the remapped payload are these with the literals moved), A and base, the code lengths
// (tz_huff_lengths / tz_huffr_lengths) and, for huffd, the distance by tezip_amd/huffd.py's rule.  Every refusal of that chain
// is made here with its status and message.
static_assert(TZ_SIZE_BINS == TZ_HUFF_COUNT_BINS && TZ_SIZE_BIAS == TZ_HUFF_COUNT_BIAS, "the seams' bins are k_huffd_count's");
static constexpr int SZ_BINS = TZ_HUFF_COUNT_BINS + TZ_HUFFR_NTOK;
static const char* const kSizeWho[3] = {"tz_huff", "tz_huffr", "tz_huffd"};

// h: the three rows of k_size_count (unremapped symbols).  -> rec (all but stream_words and bytes) and lens, the LUT of k_size_bits
static int size_code(tz_ctx* ctx, const unsigned long long* h, bool bad, size_t n, int entropy, int coder, tz_size_record* rec,
                     std::vector<uint8_t>* lens) {
    const char* who = kSizeWho[coder];
    std::vector<int16_t> lut;
    rec->table_len = -1;
    if (entropy) {   // tz_encode: the table from the counts of the symbols inside [0, TZ_NBINS)
        std::vector<unsigned long long> hist(TZ_NBINS);
        for (int y = 0; y < TZ_NBINS; ++y) hist[y] = h[y + TZ_HUFF_COUNT_BIAS];
        int16_t table[TZ_MAX_TABLE];
        TZ_TRY(tz_build_table(hist.data(), TZ_NBINS, table, &rec->table_len));
        TZ_TRY(build_enc_lut(ctx, table, rec->table_len, &lut));
    }
    const auto rank = [&](int v) { return entropy && v >= 0 && v <= TZ_NBINS ? (int)lut[v] : v; };   // k_lut
    // the histograms of the remapped payload: literals moved to their ranks, tokens as they are
    std::vector<unsigned long long> r(3 * (size_t)SZ_BINS, 0);
    for (int d = 0; d < 3; ++d) {
        for (int b = 0; b < TZ_HUFF_COUNT_BINS; ++b)
            if (h[d * SZ_BINS + b]) {
                const int rb = rank(b - TZ_HUFF_COUNT_BIAS) + TZ_HUFF_COUNT_BIAS;
                if (rb < 0 || rb >= TZ_HUFF_COUNT_BINS) bad = true;
                else r[d * SZ_BINS + rb] += h[d * SZ_BINS + b];
            }
        for (int k = 0; k < TZ_HUFFR_NTOK; ++k) r[d * SZ_BINS + TZ_HUFF_COUNT_BINS + k] = h[d * SZ_BINS + TZ_HUFF_COUNT_BINS + k];
    }
    int lo = -1, hi = -1;   // huff_counts_dev
    for (int b = 0; b < TZ_HUFF_COUNT_BINS; ++b)
        if (r[b]) {
            if (lo < 0) lo = b;
            hi = b;
        }
    if (bad || lo < 0 || hi - lo + 1 > TZ_NBINS)
        return tz_fail(ctx, TZ_ERR_INVALID, "%s_counts: the payload's values span more than %d symbols", who, TZ_NBINS);
    const int A = hi - lo + 1, base = lo - TZ_HUFF_COUNT_BIAS;
    // the code of every distance the coder may name (huff: 0, huffr: 3, huffd: all three) and its cost
    static const int kDist[3] = {0, 1, 3};
    std::vector<uint8_t> len[3];
    int best = -1;
    for (int d = 0; d < 3; ++d) {
        rec->cost_bits[d] = 0;
        if (coder != 2 && d != (coder == 0 ? 0 : 2)) continue;
        std::vector<unsigned long long> c(A + TZ_HUFFR_NTOK, 0);
        for (int s = 0; s < A; ++s) c[s] = r[d * SZ_BINS + lo + s];
        for (int k = 0; k < TZ_HUFFR_NTOK; ++k) c[A + k] = r[d * SZ_BINS + TZ_HUFF_COUNT_BINS + k];
        len[d].assign(A + TZ_HUFFR_NTOK, 0);
        if ((d == 0 ? tz_huff_lengths(c.data(), A, TZ_HUFF_L, len[d].data()) : tz_huffr_lengths(c.data(), A + TZ_HUFFR_NTOK, TZ_HUFF_L, len[d].data())) != TZ_OK)
            return tz_fail(ctx, TZ_ERR_INVALID, "%s_lengths refused the counts of the candidate", who);
        unsigned long long cost = 0;
        for (int s = 0; s < A + TZ_HUFFR_NTOK; ++s) cost += c[s] * len[d][s];
        for (int k = 0; k < TZ_HUFFR_NTOK; ++k) cost += c[A + k] * (unsigned long long)k;
        rec->cost_bits[d] = cost;
        if (best < 0 || cost < rec->cost_bits[best]) best = d;   // (a tie goes to the smaller distance)
    }
    rec->n = n;
    rec->A = A;
    rec->base = base;
    rec->dist = kDist[best];
    lens->assign(SZ_BINS, 0);
    for (int b = 0; b < TZ_HUFF_COUNT_BINS; ++b) {
        const int s = rank(b - TZ_HUFF_COUNT_BIAS) - base;
        if (s >= 0 && s < A) (*lens)[b] = len[best][s];
    }
    for (int k = 0; k < TZ_HUFFR_NTOK; ++k) (*lens)[TZ_HUFF_COUNT_BINS + k] = len[best][A + k];
    return TZ_OK;
}

// the two kernels and the host between them, on the n symbols the device stack d_q yields under `layout`
static int size_run(tz_ctx* ctx, tz_layout layout, const int16_t* d_q, size_t n, int entropy, int coder, tz_size_record* rec) {
    if (n < 1 || n >= ((size_t)1 << 40)) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: %zu elements outside [1, 2^40)", n);
    unsigned long long* d_hist;
    tz_huff_meta *d_meta, meta;
    tz_size_meta *d_smeta, smeta;
    uint8_t* d_lens;
    std::vector<unsigned long long> h(3 * (size_t)SZ_BINS);
    TZ_TRY(tz_pool_alloc(ctx, h.size() * sizeof(unsigned long long), (void**)&d_hist));
    TZ_TRY(tz_pool_alloc(ctx, sizeof(meta), (void**)&d_meta));
    TZ_TRY(tzk_size_count(ctx, layout, d_q, n, entropy, d_hist, d_meta));
    TZ_TRY(tz_d2h(ctx, h.data(), d_hist, h.size() * sizeof(unsigned long long), ctx->stream));
    TZ_TRY(tz_d2h(ctx, &meta, d_meta, sizeof(meta), ctx->stream));
    TZ_TRY(tz_stream_sync(ctx));
    std::vector<uint8_t> lens;
    TZ_TRY(size_code(ctx, h.data(), meta.bad != 0, n, entropy, coder, rec, &lens));
    TZ_TRY(tz_pool_alloc(ctx, lens.size(), (void**)&d_lens));
    TZ_TRY(tz_pool_alloc(ctx, sizeof(smeta), (void**)&d_smeta));
    TZ_TRY(tz_upload(ctx, d_lens, lens.data(), lens.size()));
    TZ_TRY(tzk_size_bits(ctx, layout, d_q, n, entropy, d_lens, rec->dist, d_smeta));
    TZ_TRY(tz_d2h(ctx, &smeta, d_smeta, sizeof(smeta), ctx->stream));
    TZ_TRY(tz_stream_sync(ctx));
    if (smeta.bad) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: the payload holds a value the code lengths give no code");
    if (smeta.words >= (1ull << 32)) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: a bit stream of %llu words does not fit the format", smeta.words);
    const int di = rec->dist == 0 ? 0 : rec->dist == 1 ? 1 : 2;
    if (smeta.bits != rec->cost_bits[di])
        return tz_fail(ctx, TZ_ERR_HIP, "tz_size_probe: k_size_bits summed %llu bits, the counts of k_size_count give %llu", smeta.bits, rec->cost_bits[di]);
    size_t nruns, nchunks, index_bytes;
    huff_geometry(n, &nruns, &nchunks, &index_bytes);
    rec->stream_words = smeta.words;
    rec->bytes = index_bytes + smeta.words * 4;
    return TZ_OK;
}

extern "C" int tz_size_probe(tz_ctx* ctx, int mode, double b0, double b1, int entropy, int coder, tz_size_record* out) {
    tz_roctx_range roctx_("tz_size_probe");
    if (!ctx || !out) return TZ_ERR_INVALID;
    if (coder < 0 || coder > 2) return tz_fail(ctx, TZ_ERR_INVALID, "tz_size_probe: coder %d, 0 (huff), 1 (huffr) or 2 (huffd) wanted", coder);
    if (entropy & ~1) return tz_fail(ctx, TZ_ERR_INVALID, "tz_size_probe: byte planes are not Huffman-coded");
    TZ_TRY(loop_check(ctx, "tz_size_probe", mode, b0, b1));
    TZ_TRY(no_plane(ctx, "tz_size_probe"));
    TZ_TRY(no_bound_map(ctx, "tz_size_probe"));
    TZ_TRY(encode_check(ctx, "tz_size_probe", mode, b0, b1));
    const tz_layout layout = layout_of(ctx);
    if (layout.channels == 1) {
        tz_call gray_check(ctx);   // (a scope of its own: the probe reuses its blocks)
        TZ_TRY(encode_all_gray(ctx));
    }
    const int nt = ctx->nt, H = ctx->H, W = ctx->W;
    const size_t N = (size_t)nt * H * W * 3;
    tz_call call(ctx);
    uint8_t* d_mask;
    int16_t* d_q;
    TZ_TRY(call.alloc(nt, &d_mask));
    TZ_TRY(tz_upload(ctx, d_mask, ctx->group_first.data(), nt));
    TZ_TRY(call.alloc(N * 2, &d_q));
    // compress.py:292-319 as encode_front's general path runs them (the quantiser walks three channels in every layout)
    TZ_TRY(tzk_delta(ctx, ctx->d_pred, ctx->d_frames, d_mask, nt, H, W, ctx->Hp, ctx->Wp, d_q));
    TZ_TRY(quantise_rollout(ctx, d_q, mode, b0, b1));
    memset(out, 0, sizeof(*out));
    return size_run(ctx, layout, d_q, (size_t)nt * tz_frame_elems(layout, H, W), entropy, coder, out);
}

// `-c --sdelta auto` (NOT a reference feature; definition TZ-SDA1: DESIGN.md section 9, tezip_amd/sdauto.py): the quantised
// deltas do not depend on the payload's spatial delta, so ONE delta + quantiser run serves the three layouts, and each costs
// the two reads of size_run -- flat (or channel 0 alone), the channel stride, the 2-D plane TZ-SD2.  out[0..2] in that order;
// n == 0: no candidate (the channel stride on a one-channel payload IS the flat delta).  The context's own spatial delta
// (tz_set_delta_stride / tz_set_delta_plane) is neither read nor changed.
extern "C" int tz_sdelta_probe(tz_ctx* ctx, int mode, double b0, double b1, int entropy, int coder, tz_size_record* out) {
    tz_roctx_range roctx_("tz_sdelta_probe");
    if (!ctx || !out) return TZ_ERR_INVALID;
    if (coder < 0 || coder > 2) return tz_fail(ctx, TZ_ERR_INVALID, "tz_sdelta_probe: coder %d, 0 (huff), 1 (huffr) or 2 (huffd) wanted", coder);
    if (entropy & ~1) return tz_fail(ctx, TZ_ERR_INVALID, "tz_sdelta_probe: byte planes are not Huffman-coded");
    TZ_TRY(encode_check(ctx, "tz_sdelta_probe", mode, b0, b1));
    const int channels = ctx->payload_channels;
    if (channels == 1) {
        tz_call gray_check(ctx);   // (a scope of its own: the probe reuses its blocks)
        TZ_TRY(encode_all_gray(ctx));
    }
    const int nt = ctx->nt, H = ctx->H, W = ctx->W;
    const size_t N = (size_t)nt * H * W * 3;
    tz_call call(ctx);
    uint8_t* d_mask;
    int16_t* d_q;
    TZ_TRY(call.alloc(nt, &d_mask));
    TZ_TRY(tz_upload(ctx, d_mask, ctx->group_first.data(), nt));
    TZ_TRY(call.alloc(N * 2, &d_q));
    TZ_TRY(tzk_delta(ctx, ctx->d_pred, ctx->d_frames, d_mask, nt, H, W, ctx->Hp, ctx->Wp, d_q));
    TZ_TRY(quantise_rollout(ctx, d_q, mode, b0, b1));
    memset(out, 0, 3 * sizeof(*out));
    tz_layout plane = {channels, 1};
    plane.plane_h = H;
    plane.plane_w = W;
    const tz_layout cand[3] = {tz_layout{channels, 1}, tz_layout{3, 3}, plane};
    for (int i = 0; i < 3; ++i) {
        if (i == 1 && channels == 1) continue;
        TZ_TRY(size_run(ctx, cand[i], d_q, (size_t)nt * tz_frame_elems(cand[i], H, W), entropy, coder, &out[i]));
    }
    return TZ_OK;
}

// the layout of a seam: 3 channels at stride 1 (flat) or 3 (channel stride), 1 channel at stride 1 (gray: q holds whole pixels)
static int size_seam_layout(tz_ctx* ctx, size_t nq, int channels, int stride, tz_layout* layout, size_t* n) {
    if (!((channels == 3 && (stride == 1 || stride == 3)) || (channels == 1 && stride == 1)))
        return tz_fail(ctx, TZ_ERR_INVALID, "size probe: no payload layout of %d channels at stride %d", channels, stride);
    if (channels == 1 && nq % 3) return tz_fail(ctx, TZ_ERR_INVALID, "size probe: a one-channel payload describes whole pixels, not %zu elements", nq);
    *layout = tz_layout{channels, stride};
    *n = channels == 1 ? nq / 3 : nq;
    return TZ_OK;
}

// the layout of a plane seam: nframes x H x W pixels, 3 channels, or channel 0 alone of q's whole pixels; q holds *nq elements
static int size_seam_plane(tz_ctx* ctx, const char* who, int nframes, int H, int W, int channels, tz_layout* layout, size_t* n, size_t* nq) {
    TZ_TRY(check_plane_dims(ctx, who, nframes, H, W, channels));
    *layout = tz_layout{channels, 1};
    layout->plane_h = H;
    layout->plane_w = W;
    *n = (size_t)nframes * tz_frame_elems(*layout, H, W);
    *nq = (size_t)nframes * H * W * 3;
    return TZ_OK;
}

static int size_count_seam(tz_ctx* ctx, tz_layout layout, const int16_t* q, size_t nq, size_t n, int apply_offset, unsigned long long* counts,
                           int* bad);
static int size_bits_seam(tz_ctx* ctx, tz_layout layout, const int16_t* q, size_t nq, size_t n, int apply_offset, const uint8_t* lens, int dist,
                          unsigned long long* words, unsigned long long* bits, int* bad);

extern "C" int tz_size_count_plane_buf(tz_ctx* ctx, const int16_t* q, int nframes, int H, int W, int channels, int apply_offset,
                                       unsigned long long* counts, int* bad) {
    if (!ctx || !q || !counts || !bad) return TZ_ERR_INVALID;
    tz_layout layout;
    size_t n, nq;
    TZ_TRY(size_seam_plane(ctx, "tz_size_count_plane_buf", nframes, H, W, channels, &layout, &n, &nq));
    return size_count_seam(ctx, layout, q, nq, n, apply_offset, counts, bad);
}

extern "C" int tz_size_bits_plane_buf(tz_ctx* ctx, const int16_t* q, int nframes, int H, int W, int channels, int apply_offset,
                                      const uint8_t* lens, int dist, unsigned long long* words, unsigned long long* bits, int* bad) {
    if (!ctx || !q || !lens || !words || !bits || !bad) return TZ_ERR_INVALID;
    tz_layout layout;
    size_t n, nq;
    TZ_TRY(size_seam_plane(ctx, "tz_size_bits_plane_buf", nframes, H, W, channels, &layout, &n, &nq));
    return size_bits_seam(ctx, layout, q, nq, n, apply_offset, lens, dist, words, bits, bad);
}

extern "C" int tz_size_count_buf(tz_ctx* ctx, const int16_t* q, size_t nq, int channels, int stride, int apply_offset,
                                 unsigned long long* counts, int* bad) {
    if (!ctx || !q || !counts || !bad) return TZ_ERR_INVALID;
    tz_layout layout;
    size_t n;
    TZ_TRY(size_seam_layout(ctx, nq, channels, stride, &layout, &n));
    return size_count_seam(ctx, layout, q, nq, n, apply_offset, counts, bad);
}

static int size_count_seam(tz_ctx* ctx, tz_layout layout, const int16_t* q, size_t nq, size_t n, int apply_offset, unsigned long long* counts,
                           int* bad) {
    if (n < 1 || n >= ((size_t)1 << 40)) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: %zu elements outside [1, 2^40)", n);
    tz_call call(ctx);
    const int16_t* d_q;
    unsigned long long* d_hist;
    tz_huff_meta *d_meta, meta;
    TZ_TRY(call.in(q, nq * 2, &d_q));
    TZ_TRY(call.alloc(3 * (size_t)SZ_BINS * sizeof(unsigned long long), &d_hist));
    TZ_TRY(call.alloc(sizeof(meta), &d_meta));
    TZ_TRY(tzk_size_count(ctx, layout, d_q, n, apply_offset ? 1 : 0, d_hist, d_meta));
    TZ_TRY(tz_d2h(ctx, counts, d_hist, 3 * (size_t)SZ_BINS * sizeof(unsigned long long), ctx->stream));
    TZ_TRY(tz_d2h(ctx, &meta, d_meta, sizeof(meta), ctx->stream));
    TZ_TRY(tz_stream_sync(ctx));
    *bad = meta.bad != 0;
    return TZ_OK;
}

extern "C" int tz_size_bits_buf(tz_ctx* ctx, const int16_t* q, size_t nq, int channels, int stride, int apply_offset, const uint8_t* lens,
                                int dist, unsigned long long* words, unsigned long long* bits, int* bad) {
    if (!ctx || !q || !lens || !words || !bits || !bad) return TZ_ERR_INVALID;
    tz_layout layout;
    size_t n;
    TZ_TRY(size_seam_layout(ctx, nq, channels, stride, &layout, &n));
    return size_bits_seam(ctx, layout, q, nq, n, apply_offset, lens, dist, words, bits, bad);
}

static int size_bits_seam(tz_ctx* ctx, tz_layout layout, const int16_t* q, size_t nq, size_t n, int apply_offset, const uint8_t* lens, int dist,
                          unsigned long long* words, unsigned long long* bits, int* bad) {
    if (n < 1 || n >= ((size_t)1 << 40)) return tz_fail(ctx, TZ_ERR_INVALID, "huffman: %zu elements outside [1, 2^40)", n);
    tz_call call(ctx);
    const int16_t* d_q;
    uint8_t* d_lens;
    tz_size_meta *d_smeta, smeta;
    TZ_TRY(call.in(q, nq * 2, &d_q));
    TZ_TRY(call.alloc(SZ_BINS, &d_lens));
    TZ_TRY(call.alloc(sizeof(smeta), &d_smeta));
    TZ_TRY(tz_upload(ctx, d_lens, lens, SZ_BINS));
    TZ_TRY(tzk_size_bits(ctx, layout, d_q, n, apply_offset ? 1 : 0, d_lens, dist, d_smeta));
    TZ_TRY(tz_d2h(ctx, &smeta, d_smeta, sizeof(smeta), ctx->stream));
    TZ_TRY(tz_stream_sync(ctx));
    *words = smeta.words;
    *bits = smeta.bits;
    *bad = smeta.bad != 0;
    return TZ_OK;
}

// --------------------------------------------------------------------------- key-frame coders (TZK1, TZK2)
// `--key-coder huff` (NOT a reference feature: compress.py:271-278 hands a zero-except-keys stack of the whole sequence to
// zstd): the key frames alone, as predictor residuals under one TZH1 code (tezip_amd/keycoder.py, k_key_* in tz_codec.hip).
// The coder has buffers of its own (d_keys, d_keysym): what tz_huff_* / tz_huffr_* hold or have staged is left alone.
// `--key-coder huffg` (TZK2, tezip_amd/keycoderg.py) is TZK1 with a GRAY bit per key frame, and TZK1 = TZK2 with no GRAY bit:
// one path serves both, and a format is what KeysFmt says.  ctx->keys_kind says which format's begin staged a stream, so each
// put and decode refuses a body staged for the other format.
static constexpr int TZ_KEYS_A = 256;

struct KeysFmt {
    tz_ctx::tz_keys_kind kind;
    int max_pred;           // the largest pred byte: predictor ids 0..3, | 4 (GRAY) where the format has the bit
    const char* who;        // the entry points' prefix
    const char* bad_pred;   // the refusal of a pred byte above max_pred: its value and its entry
    const char* put_note;   // what the refusal of a put adds to "... the staged key-frame stream"
};
static constexpr KeysFmt FMT_TZK1{tz_ctx::KEYS_TZK1, 3, "tz_keys", "key frames: predictor id %d (entry %d) outside [0, 3]", ""},
    FMT_TZK2{tz_ctx::KEYS_TZK2, 7, "tz_keysg", "key frames: pred byte %d (entry %d) outside [0, 7]", " (TZK2)"};

// the key list of a stack of nt frames: at least one index, strictly ascending, inside [0, nt)
static int keys_check(tz_ctx* ctx, int nt, const int* idx, int nkeys) {
    if (!idx || nkeys < 1 || nkeys > nt) return tz_fail(ctx, TZ_ERR_INVALID, "key frames: %d indices for a stack of %d frames", nkeys, nt);
    for (int k = 0; k < nkeys; ++k)
        if (idx[k] < 0 || idx[k] >= nt || (k && idx[k] <= idx[k - 1]))
            return tz_fail(ctx, TZ_ERR_INVALID, "key frames: index %d (entry %d) is not ascending inside [0, %d)", idx[k], k, nt);
    return TZ_OK;
}

// pred bytes the format allows -> off[k], the exclusive prefix of the frames' symbol counts (k * H * W * 3 without a GRAY
// frame), and their sum
static int keys_layout(tz_ctx* ctx, const KeysFmt& f, const uint8_t* pred, int nkeys, int H, int W, std::vector<unsigned long long>* off,
                       size_t* n) {
    off->resize(nkeys);
    unsigned long long at = 0;
    for (int k = 0; k < nkeys; ++k) {
        if (pred[k] > f.max_pred) return tz_fail(ctx, TZ_ERR_INVALID, f.bad_pred, pred[k], k);
        (*off)[k] = at;
        at += (unsigned long long)H * W * ((pred[k] & 4) ? 1 : 3);
    }
    *n = (size_t)at;
    return TZ_OK;
}

struct KeysDev {
    const int* idx = nullptr;
    const uint8_t* pred = nullptr;
    const unsigned long long* off = nullptr;
};

// idx, and pred and off where given, in pool blocks
static int keys_upload(tz_ctx* ctx, const int* idx, const uint8_t* pred, const std::vector<unsigned long long>* off, int nkeys, KeysDev* d) {
    void* p;
    TZ_TRY(tz_pool_alloc(ctx, sizeof(int) * nkeys, &p));
    TZ_TRY(tz_upload(ctx, p, idx, sizeof(int) * nkeys));
    d->idx = (const int*)p;
    if (pred) {
        TZ_TRY(tz_pool_alloc(ctx, nkeys, &p));
        TZ_TRY(tz_upload(ctx, p, pred, nkeys));
        d->pred = (const uint8_t*)p;
    }
    if (off) {
        TZ_TRY(tz_pool_alloc(ctx, sizeof(unsigned long long) * nkeys, &p));
        TZ_TRY(tz_upload(ctx, p, off->data(), sizeof(unsigned long long) * nkeys));
        d->off = (const unsigned long long*)p;
    }
    return TZ_OK;
}

// the encoder's precondition: a frame stack in the context (tz_frames_put or a rollout), everything of it arrived
static int keys_resident(tz_ctx* ctx, const char* who) {
    if (!ctx->d_frames || ctx->nt < 1 || !(ctx->staged || ctx->rollout_kind != tz_ctx::ROLLOUT_NONE))
        return tz_fail(ctx, TZ_ERR_STATE, "%s needs a resident frame stack (tz_frames_begin / tz_frames_put, or a rollout)", who);
    TZ_HIP(ctx, hipEventRecord(ctx->ev_frames, ctx->copy_stream));
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_frames, 0));
    return TZ_OK;
}

extern "C" int tz_keys_counts(tz_ctx* ctx, const int* idx, int nkeys, unsigned* counts) {
    tz_roctx_range roctx_("tz_keys_counts");
    if (!ctx || !counts) return TZ_ERR_INVALID;
    TZ_TRY(keys_resident(ctx, "tz_keys_counts"));
    TZ_TRY(keys_check(ctx, ctx->nt, idx, nkeys));
    tz_call call(ctx);
    KeysDev d;
    unsigned* d_counts;
    const size_t cb = (size_t)nkeys * 4 * TZ_KEYS_A * sizeof(unsigned);
    TZ_TRY(keys_upload(ctx, idx, nullptr, nullptr, nkeys, &d));
    TZ_TRY(call.alloc(cb, &d_counts));
    TZ_TRY(tzk_key_hist(ctx, ctx->d_frames, ctx->H, ctx->W, d.idx, nkeys, d_counts));
    TZ_TRY(tz_d2h(ctx, counts, d_counts, cb, ctx->stream));
    return tz_stream_sync(ctx);
}

static int keys_gray(tz_ctx* ctx, const int* idx, int nkeys, uint8_t* gray) {
    KeysDev d;
    void* d_flags;
    std::vector<unsigned> flags(nkeys);
    TZ_TRY(keys_upload(ctx, idx, nullptr, nullptr, nkeys, &d));
    TZ_TRY(tz_pool_alloc(ctx, sizeof(unsigned) * nkeys, &d_flags));
    TZ_TRY(tzk_key_gray(ctx, ctx->d_frames, ctx->H, ctx->W, d.idx, nkeys, (unsigned*)d_flags));
    TZ_TRY(tz_d2h(ctx, flags.data(), d_flags, sizeof(unsigned) * nkeys, ctx->stream));
    TZ_TRY(tz_stream_sync(ctx));
    for (int k = 0; k < nkeys; ++k) gray[k] = flags[k] ? 0 : 1;
    return TZ_OK;
}

extern "C" int tz_keys_gray(tz_ctx* ctx, const int* idx, int nkeys, uint8_t* gray) {
    tz_roctx_range roctx_("tz_keys_gray");
    if (!ctx || !gray) return TZ_ERR_INVALID;
    TZ_TRY(keys_resident(ctx, "tz_keys_gray"));
    TZ_TRY(keys_check(ctx, ctx->nt, idx, nkeys));
    tz_call call(ctx);
    return keys_gray(ctx, idx, nkeys, gray);
}

static int keys_encode(tz_ctx* ctx, const KeysFmt& f, const char* who, const int* idx, int nkeys, const uint8_t* pred, const uint8_t* lengths,
                       size_t* bytes) {
    if (!ctx || !pred || !lengths || !bytes) return TZ_ERR_INVALID;
    std::vector<unsigned long long> off;
    size_t n;
    TZ_TRY(keys_resident(ctx, who));
    TZ_TRY(keys_check(ctx, ctx->nt, idx, nkeys));
    TZ_TRY(keys_layout(ctx, f, pred, nkeys, ctx->H, ctx->W, &off, &n));
    tz_call call(ctx);
    KeysDev d;
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_keysym, &ctx->cap_keysym, n * 2));
    TZ_TRY(keys_upload(ctx, idx, pred, &off, nkeys, &d));
    TZ_TRY(tzk_key_resid(ctx, ctx->d_frames, ctx->H, ctx->W, d.idx, d.pred, d.off, nkeys, ctx->d_keysym));
    return huff_encode_dev(ctx, ctx->d_keysym, n, lengths, TZ_KEYS_A, 0, bytes, 0, true);   // (dist 0: plain TZH1 codes)
}

extern "C" int tz_keys_encode(tz_ctx* ctx, const int* idx, int nkeys, const uint8_t* pred, const uint8_t* lengths, size_t* bytes) {
    tz_roctx_range roctx_("tz_keys_encode");
    return keys_encode(ctx, FMT_TZK1, "tz_keys_encode", idx, nkeys, pred, lengths, bytes);
}

extern "C" int tz_keysg_encode(tz_ctx* ctx, const int* idx, int nkeys, const uint8_t* predg, const uint8_t* lengths, size_t* bytes) {
    tz_roctx_range roctx_("tz_keysg_encode");
    return keys_encode(ctx, FMT_TZK2, "tz_keysg_encode", idx, nkeys, predg, lengths, bytes);
}

extern "C" int tz_keys_get(tz_ctx* ctx, size_t offset, size_t count, uint8_t* out) {
    if (!ctx || !out) return TZ_ERR_INVALID;
    if (!ctx->d_keys || offset > ctx->keys_bytes || count > ctx->keys_bytes - offset)
        return tz_fail(ctx, TZ_ERR_INVALID, "byte range outside the resident key-frame stream");
    TZ_TRY(tz_d2h(ctx, out, ctx->d_keys + offset, count, ctx->stream));
    return tz_stream_sync(ctx);
}

extern "C" int tz_keysg_get(tz_ctx* ctx, size_t offset, size_t count, uint8_t* out) {
    return tz_keys_get(ctx, offset, count, out);   // (an encoder's stream carries no format of its own: index | bits)
}

// symbols (device) -> the frames idx[k] of a stack at d_frames; the other frames of the stack are not touched
static int keys_unresidual(tz_ctx* ctx, const KeysFmt& f, const int16_t* d_sym, int H, int W, const int* idx, const uint8_t* pred, int nkeys,
                           uint8_t* d_frames) {
    std::vector<unsigned long long> off;
    size_t n;
    TZ_TRY(keys_layout(ctx, f, pred, nkeys, H, W, &off, &n));
    KeysDev d;
    TZ_TRY(keys_upload(ctx, idx, pred, &off, nkeys, &d));
    void* d_tmp = nullptr;   // the scratch plane of the GRAY frames' column pass, where a frame has one
    if (std::any_of(pred, pred + nkeys, [](uint8_t p) { return (p & 6) == 6; })) TZ_TRY(tz_pool_alloc(ctx, n, &d_tmp));
    return tzk_key_unresid(ctx, d_sym, H, W, d.idx, d.pred, d.off, nkeys, (uint8_t*)d_tmp, d_frames);
}

static int keys_begin(tz_ctx* ctx, const KeysFmt& f, size_t bytes, int nt, int H, int W, const int* idx, int nkeys, const uint8_t* pred,
                      const uint8_t* lengths) {
    if (!ctx || !pred) return TZ_ERR_INVALID;
    if (nt < 1 || H < 1 || W < 1 || nt > kMaxFrames || H > 32767 || W > 32767)
        return tz_fail(ctx, TZ_ERR_INVALID, "bad sequence shape nt=%d H=%d W=%d (int16 trailer limits)", nt, H, W);
    TZ_TRY(keys_check(ctx, nt, idx, nkeys));
    std::vector<unsigned long long> off;
    size_t n, sw;
    TZ_TRY(keys_layout(ctx, f, pred, nkeys, H, W, &off, &n));
    TZ_TRY(huff_check_stream(ctx, bytes, n, TZ_HUFF_RUN, &sw));
    std::vector<uint16_t> dec;
    TZ_TRY(huff_tables(ctx, lengths, TZ_KEYS_A, 0, nullptr, &dec, 0));
    ctx->keys_kind = tz_ctx::KEYS_NONE;
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_keys, &ctx->cap_keys, std::max<size_t>(bytes, 16)));
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_keysym, &ctx->cap_keysym, std::max<size_t>(n, 8) * 2));
    ctx->keys_bytes = bytes;
    ctx->keys_put = 0;
    ctx->keys_nt = nt;
    ctx->keys_H = H;
    ctx->keys_W = W;
    ctx->keys_idx.assign(idx, idx + nkeys);
    ctx->keys_pred.assign(pred, pred + nkeys);
    ctx->keys_dec_tab.swap(dec);
    ctx->keys_n = n;
    ctx->keys_kind = f.kind;
    TZ_HIP(ctx, hipEventRecord(ctx->ev_compute, ctx->stream));  // earlier work may still read the old stream
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute, 0));
    return TZ_OK;
}

static int keys_put(tz_ctx* ctx, const KeysFmt& f, size_t offset, size_t count, const uint8_t* src) {
    if (!ctx || !src) return TZ_ERR_INVALID;
    if (!ctx->d_keys || ctx->keys_kind != f.kind || offset > ctx->keys_bytes || count > ctx->keys_bytes - offset)
        return tz_fail(ctx, TZ_ERR_INVALID, "byte range outside the staged key-frame stream%s", f.put_note);
    TZ_TRY(tz_h2d(ctx, ctx->d_keys + offset, src, count, ctx->copy_stream));
    ctx->keys_put += count;
    return TZ_OK;
}

static int keys_decode(tz_ctx* ctx, const KeysFmt& f) {
    if (!ctx) return TZ_ERR_INVALID;
    if (ctx->keys_kind != f.kind || !ctx->d_keys || !ctx->d_keysym)
        return tz_fail(ctx, TZ_ERR_STATE, "%s_decode needs a stream staged with %s_begin / %s_put", f.who, f.who, f.who);
    if (ctx->keys_put != ctx->keys_bytes)
        return tz_fail(ctx, TZ_ERR_STATE, "%s_decode: %zu of the stream's %zu bytes were put", f.who, ctx->keys_put, ctx->keys_bytes);
    tz_call call(ctx);
    const int nt = ctx->keys_nt, H = ctx->keys_H, W = ctx->keys_W;
    size_t sw;
    TZ_TRY(huff_check_stream(ctx, ctx->keys_bytes, ctx->keys_n, TZ_HUFF_RUN, &sw));
    // what tz_frames_begin does: the stack's buffer and shape; whatever rollout was resident is gone
    set_rollout(ctx, tz_ctx::ROLLOUT_NONE, 0, 0);
    ctx->staged = false;
    const size_t fb = (size_t)nt * H * W * 3;
    TZ_TRY(tz_ensure(ctx, (void**)&ctx->d_frames, &ctx->cap_frames, fb));
    TZ_HIP(ctx, hipEventRecord(ctx->ev_frames, ctx->copy_stream));   // the pieces of the puts (and older copies into d_frames)
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_frames, 0));
    TZ_TRY(huff_decode_dev(ctx, ctx->d_keys, sw, ctx->keys_n, ctx->keys_dec_tab, TZ_KEYS_A, 0, 0, ctx->d_keysym));
    TZ_HIP(ctx, hipMemsetAsync(ctx->d_frames, 0, fb, ctx->stream));   // the frames that are no key frames (a fresh buffer holds anything)
    TZ_TRY(keys_unresidual(ctx, f, ctx->d_keysym, H, W, ctx->keys_idx.data(), ctx->keys_pred.data(), (int)ctx->keys_idx.size(), ctx->d_frames));
    TZ_HIP(ctx, hipEventRecord(ctx->ev_compute, ctx->stream));       // a later tz_frames_put waits for the frames written here
    TZ_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute, 0));
    ctx->nt = nt;
    ctx->H = H;
    ctx->W = W;
    ctx->staged = true;
    return TZ_OK;
}

extern "C" int tz_keys_begin(tz_ctx* ctx, size_t bytes, int nt, int H, int W, const int* idx, int nkeys, const uint8_t* pred,
                             const uint8_t* lengths) {
    return keys_begin(ctx, FMT_TZK1, bytes, nt, H, W, idx, nkeys, pred, lengths);
}

extern "C" int tz_keys_put(tz_ctx* ctx, size_t offset, size_t count, const uint8_t* src) { return keys_put(ctx, FMT_TZK1, offset, count, src); }

extern "C" int tz_keys_decode(tz_ctx* ctx) {
    tz_roctx_range roctx_("tz_keys_decode");
    return keys_decode(ctx, FMT_TZK1);
}

extern "C" int tz_keysg_begin(tz_ctx* ctx, size_t bytes, int nt, int H, int W, const int* idx, int nkeys, const uint8_t* predg,
                              const uint8_t* lengths) {
    return keys_begin(ctx, FMT_TZK2, bytes, nt, H, W, idx, nkeys, predg, lengths);
}

extern "C" int tz_keysg_put(tz_ctx* ctx, size_t offset, size_t count, const uint8_t* src) { return keys_put(ctx, FMT_TZK2, offset, count, src); }

extern "C" int tz_keysg_decode(tz_ctx* ctx) {
    tz_roctx_range roctx_("tz_keysg_decode");
    return keys_decode(ctx, FMT_TZK2);
}

// stand-alone forms on host or device arrays: frames (k, H, W, 3) <-> the int16 symbols keys_layout counts under pred[k]
static const char* const kKeySymAlign = "key frames: a device symbol array must be 2-byte aligned";

// the k frames of a buffer form are their own key list; *n: their symbols
static int keys_buf_layout(tz_ctx* ctx, const KeysFmt& f, int k, int H, int W, const uint8_t* pred, std::vector<int>* idx,
                           std::vector<unsigned long long>* off, size_t* n) {
    if (k < 1 || H < 1 || W < 1 || k > kMaxFrames || H > 32767 || W > 32767)
        return tz_fail(ctx, TZ_ERR_INVALID, "bad key-frame stack k=%d H=%d W=%d", k, H, W);
    idx->resize(k);
    for (int i = 0; i < k; ++i) (*idx)[i] = i;
    return keys_layout(ctx, f, pred, k, H, W, off, n);
}

static int keys_residual_buf(tz_ctx* ctx, const KeysFmt& f, const uint8_t* frames, int k, int H, int W, const uint8_t* pred, int16_t* sym) {
    if (!ctx || !frames || !pred || !sym) return TZ_ERR_INVALID;
    std::vector<int> idx;
    std::vector<unsigned long long> off;
    size_t n;
    TZ_TRY(keys_buf_layout(ctx, f, k, H, W, pred, &idx, &off, &n));
    return buf_op(ctx, frames, (size_t)k * H * W * 3, 0, sym, n * 2, 1, kKeySymAlign, [&](const void* din, void* dout) {
        KeysDev d;
        TZ_TRY(keys_upload(ctx, idx.data(), pred, &off, k, &d));
        return tzk_key_resid(ctx, (const uint8_t*)din, H, W, d.idx, d.pred, d.off, k, (int16_t*)dout);
    });
}

static int keys_unresidual_buf(tz_ctx* ctx, const KeysFmt& f, const int16_t* sym, int k, int H, int W, const uint8_t* pred, uint8_t* frames) {
    if (!ctx || !frames || !pred || !sym) return TZ_ERR_INVALID;
    std::vector<int> idx;
    std::vector<unsigned long long> off;
    size_t n;
    TZ_TRY(keys_buf_layout(ctx, f, k, H, W, pred, &idx, &off, &n));
    return buf_op(ctx, sym, n * 2, 1, frames, (size_t)k * H * W * 3, 0, kKeySymAlign, [&](const void* din, void* dout) {
        return keys_unresidual(ctx, f, (const int16_t*)din, H, W, idx.data(), pred, k, (uint8_t*)dout);
    });
}

extern "C" int tz_keys_residual_buf(tz_ctx* ctx, const uint8_t* frames, int k, int H, int W, const uint8_t* pred, int16_t* sym) {
    return keys_residual_buf(ctx, FMT_TZK1, frames, k, H, W, pred, sym);
}

extern "C" int tz_keys_unresidual_buf(tz_ctx* ctx, const int16_t* sym, int k, int H, int W, const uint8_t* pred, uint8_t* frames) {
    return keys_unresidual_buf(ctx, FMT_TZK1, sym, k, H, W, pred, frames);
}

extern "C" int tz_keysg_residual_buf(tz_ctx* ctx, const uint8_t* frames, int k, int H, int W, const uint8_t* predg, int16_t* sym) {
    return keys_residual_buf(ctx, FMT_TZK2, frames, k, H, W, predg, sym);
}

extern "C" int tz_keysg_unresidual_buf(tz_ctx* ctx, const int16_t* sym, int k, int H, int W, const uint8_t* predg, uint8_t* frames) {
    return keys_unresidual_buf(ctx, FMT_TZK2, sym, k, H, W, predg, frames);
}
