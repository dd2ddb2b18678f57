// engine.cpp -- C ABI of the MI355X SDA engine (include/sda_engine.h).
//
// Host-side responsibilities only: argument validation with the reference's error behaviour
// (Err strings of client/src/crypto/sharing/*.rs -> status 1..6, assert!/panic -> PRECONDITION),
// staging of host buffers to HBM, kernel launches (kernels.h) and copying results back.  No
// arithmetic on the data happens here and there is no CPU fallback: if the device path fails
// the call fails.
#include "../../include/sda_engine.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host_pack.h"
#include "kernels.h"

struct sda_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    void* work = nullptr;
    size_t work_bytes = 0;
    void* stage = nullptr;        // staging for host-path inputs/outputs
    size_t stage_bytes = 0;
    sda::DeviceTable gen_tab;     // packed-Shamir twiddles (per scheme)
    void* gen_log = nullptr;      // packed-Shamir generic fix-up log (sda::packed_gen_log_bytes())
    size_t gen_log_bytes = 0;
    bool gen_log_used = false;    // the last packed launch zeroed gen_log's count and logs into it
    void* gen32_tmp = nullptr;    // sda_packed_generate32_dev at n + 1 = 81: i64 shares before the narrowing pass
    size_t gen32_tmp_bytes = 0;
    void* codec_work = nullptr;   // varint codec plan / scan workspace
    size_t codec_work_bytes = 0;
    void* codec_mat = nullptr;    // decoded [N][len] matrix of the clerk decode+combine path
    size_t codec_mat_bytes = 0;
    void* pipe = nullptr;         // recipient / participant pipeline scratch (mask, masked, compacted shares)
    size_t pipe_bytes = 0;
    sda::DeviceTable rev_tab;     // packed-Shamir Newton/Lagrange tables (per scheme + clerk set)
    void* snap = nullptr;         // snapshot transposition copy plan
    size_t snap_bytes = 0;
    // The scratch buffers above are shared by every call on the handle.  A call on another stream
    // than the previous one first waits (on the device) for the work queued on that stream.
    hipStream_t last_stream = nullptr;
    hipEvent_t order_ev = nullptr;
    bool order_ok = true;         // order_ev was recorded when the last call ended (else: host sync)
    unsigned long long* rej_host = nullptr;   // pinned: the ChaCha rejection count of a pipeline's mask
    // sda_chacha_last_launch: how the last mask combine or participant mask on this handle ran; chacha_split:
    // that call split its seeds over the handle's devices (chacha_combine_multi), each recording its own part
    sda::ChachaLaunchInfo chacha_last;
    bool chacha_split = false;
    // sda_codec_last_launch: how the last decode -> combine on this handle produced its result (decode_combine)
    sda::CodecLaunchInfo codec_last;
    // sda_combine_last_launch: which combine kernel this handle (of a multi-device handle: this device) launched
    // last and on what grid, filled by the launcher where it decides; a call that launches nothing leaves it
    sda::CombineLaunchInfo combine_last;
    // streaming host path (host rows -> HBM in row tiles, host_path section): pinned staging and device
    // tiles, double buffered, and a copy stream so a tile's upload overlaps the previous tile's combine
    hipStream_t copy_stream = nullptr;
    hipEvent_t h2d_done[2] = {nullptr, nullptr}, tile_free[2] = {nullptr, nullptr};
    void* hs_pin = nullptr;       // pinned host: 2 tiles
    size_t hs_pin_bytes = 0;
    void* hs_dev = nullptr;       // device: 2 tiles + the accumulator
    size_t hs_dev_bytes = 0;
    // sda_host_stream_stats: tiles staged as int32 / as i64 and the bytes of their host -> device copies, since
    // the handle was created (a sub-handle is driven by one host thread at a time)
    uint64_t hs_tiles32 = 0, hs_tiles64 = 0, hs_bytes_h2d = 0;
    // a handle over G devices (sda_engine_create_multi): sub[0] is this handle, sub[1..G) are owned
    // single-device handles; empty for a single-device handle
    std::vector<sda_engine*> sub;
    void** comms = nullptr;       // ncclComm_t[G], created on first use (RCCL, loaded at run time)
};

namespace {

thread_local std::string g_last_error;

// The handle and stream of the call in progress on this thread (set by pick()): when the call returns,
// its stream records the handle's order event, so the NEXT call -- on whatever stream -- only waits on
// that event and never touches this call's stream again (the caller may destroy it in between).
thread_local sda_engine* t_call_h = nullptr;
thread_local hipStream_t t_call_s = nullptr;

void end_call() {
    if (t_call_h) {
        t_call_h->order_ok = hipEventRecord(t_call_h->order_ev, t_call_s) == hipSuccess;
        t_call_h = nullptr;
    }
}

// Every extern "C" entry point opens a CallScope (SDA_ENTRY) as its first statement; the outermost scope
// ends the call's ordering scope (end_call) on every return path, after everything the call queued.
// Internal helpers -- and entry points called from entry points -- may return ok()/fail() freely.
thread_local int t_depth = 0;
struct CallScope {
    CallScope() { ++t_depth; }
    ~CallScope() {
        if (--t_depth == 0) end_call();
    }
    CallScope(const CallScope&) = delete;
    CallScope& operator=(const CallScope&) = delete;
};
#define SDA_ENTRY CallScope sda_call_scope_

sda_status fail(sda_status st, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return st;
}

sda_status ok() {
    g_last_error.clear();
    return SDA_OK;
}

// A failed HIP call also sets the thread's sticky last-error, which the caller's own runtime checks (torch's
// hipGetLastError after each launch) would then report against their next, unrelated op: the status we
// return carries the error, so the sticky copy is cleared.
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            (void)hipGetLastError();                                                               \
            return fail(_e == hipErrorOutOfMemory ? SDA_ERR_OUT_OF_MEMORY : SDA_ERR_DEVICE,        \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                          \
    } while (0)

// Engine scratch comes from hipMalloc.  SDA_SCRATCH_HBM=1 takes scratch of at least kScratchHbmMin bytes from
// sda_hbm_alloc's chunk-mapped backing instead: on a clean box that measured 1.5 % slower for
// the codec's 4 GB slot buffer and neutral for the pipelines (profiles/r05f/ab_scratch_hbm.txt), the same
// direction as the combine's input (§4.1), so it stays opt-in for boxes whose VRAM is fragmented.
constexpr size_t kScratchHbmMin = (size_t)256 << 20;
bool scratch_hbm(size_t bytes) {
    static const bool on = [] {
        const char* e = getenv("SDA_SCRATCH_HBM");
        return e && atoi(e) == 1;
    }();
    return on && bytes >= kScratchHbmMin;
}
bool hbm_owned(void* p);      // (HBM section) p was returned by sda_hbm_alloc and not freed
void hbm_engine_opened(int device);   // (HBM section) live engine handles per device
bool hbm_engine_closed(int device);   // true when that was the device's last live handle

void dev_free(void* p) {
    if (!p) return;
    if (hbm_owned(p)) (void)sda_hbm_free(p);     // pooled; reused only after a device sync (§2)
    else (void)hipFree(p);
}

sda_status dev_alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (scratch_hbm(bytes)) {
        int d = 0;
        HIP_TRY(hipGetDevice(&d));
        return sda_hbm_alloc(d, bytes, p);
    }
    HIP_TRY(hipMalloc(p, bytes));
    return SDA_OK;
}

sda_status ensure(void** buf, size_t* have, size_t need) {
    if (need <= *have) return SDA_OK;
    dev_free(*buf);
    *buf = nullptr;
    *have = 0;
    size_t want = need + need / 4 + 4096;
    if (sda_status e = dev_alloc(buf, want)) return e;
    *have = want;
    return SDA_OK;
}

// `_dev` entry points run on the caller's stream; NULL is the HIP null (default) stream, which is
// also what torch's default stream reports -- so work stays ordered with the caller's own ops.
// Switching streams orders the new stream after the previous call (event wait, no host sync), so a
// call never reuses a scratch buffer that work queued on another stream may still be reading.  The
// event was recorded on the previous call's stream when that call returned (end_call), so the previous
// stream itself is never touched here and may have been destroyed since.
hipStream_t pick(sda_engine* h, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (s != h->last_stream) {
        // a failed record leaves a stale event: order from the host instead (the previous stream may be
        // gone, so the whole device)
        if (!h->order_ok || hipStreamWaitEvent(s, h->order_ev, 0) != hipSuccess) (void)hipDeviceSynchronize();
        h->last_stream = s;
    }
    t_call_h = h;
    t_call_s = s;
    return s;
}

bool is_pow(uint64_t x, uint64_t b) {
    if (x < 1) return false;
    while (x % b == 0) x /= b;
    return x == 1;
}

// Rust `x % m` with m < 0 equals `x % |m|`; m == 0 panics.
sda_status modulus_abs(int64_t m, int64_t* out) {
    if (m == 0) return fail(SDA_ERR_PRECONDITION, "attempt to calculate the remainder with a divisor of zero");
    if (m == INT64_MIN) return fail(SDA_ERR_UNSUPPORTED, "modulus i64::MIN is outside the engine's domain");
    *out = m < 0 ? -m : m;
    return SDA_OK;
}

// Packed-Shamir parameter domain of the engine (DESIGN.md "Domain").
sda_status check_packed(const sda_sharing_scheme* s) {
    const uint64_t k = s->secret_count, t = s->privacy_threshold, n = s->share_count;
    const int64_t p = s->modulus;
    if (k == 0) return fail(SDA_ERR_UNSUPPORTED, "secret_count must be >= 1");
    if (n + 1 < k + t + 1)   // tss: vec![0; share_count - reconstruct_limit()] underflows
        return fail(SDA_ERR_PRECONDITION, "share_count (%llu) < secret_count + privacy_threshold (%llu)",
                    (unsigned long long)n, (unsigned long long)(k + t));
    if (!is_pow(k + t + 1, 2) || k + t + 1 > sda::kWideMaxL)
        return fail(SDA_ERR_UNSUPPORTED, "secret_count + privacy_threshold + 1 = %llu must be a power of 2 <= %u",
                    (unsigned long long)(k + t + 1), sda::kWideMaxL);
    if (!is_pow(n + 1, 3) || n + 1 > sda::kWideMaxN3)
        return fail(SDA_ERR_UNSUPPORTED, "share_count + 1 = %llu must be a power of 3 <= %u",
                    (unsigned long long)(n + 1), sda::kWideMaxN3);
    if (p < 3 || p % 2 == 0 || p >= ((int64_t)1 << 31))
        return fail(SDA_ERR_UNSUPPORTED, "prime_modulus %lld must be odd and < 2^31 (tss i64 headroom)",
                    (long long)p);
    if (s->omega_secrets <= 0 || s->omega_secrets >= p || s->omega_shares <= 0 || s->omega_shares >= p)
        return fail(SDA_ERR_UNSUPPORTED, "omega_secrets / omega_shares must lie in (0, p)");
    return SDA_OK;
}

struct DevArena {   // bump allocator over the engine's staging buffer
    char* base;
    size_t off = 0;
    template <typename T> T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base + off);
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};

sda_status stage(sda_engine* h, size_t bytes, DevArena* a) {
    (void)pick(h, h->stream);                  // host entry points run on the engine's own stream
    sda_status st = ensure(&h->stage, &h->stage_bytes, bytes + 4096);
    if (st) return st;
    a->base = static_cast<char*>(h->stage);
    a->off = 0;
    return SDA_OK;
}

size_t rup(size_t b) { return (b + 255) & ~(size_t)255; }

// chacha.rs:57-76: combine of n seed streams ([n][w] u32 words on the device) into out (device, D
// values).  The fast counter-mode kernel where its rejection log suffices; otherwise (moduli above
// 2^62, high rejection rates, or a log overflow) the exact stream path.
// Every ChaCha launch leaves how it ran in the handle (sda_chacha_last_launch).
void record_chacha(sda_engine* h, const sda::ChachaLaunchInfo& info) {
    h->chacha_last = info;
    h->chacha_split = false;
}

sda_status chacha_combine(sda_engine* h, int64_t m, uint64_t D, const uint32_t* seeds, uint32_t w, uint64_t n,
                          int64_t* out, hipStream_t st) {
    if (D == 0) return SDA_OK;
    sda::ChachaLaunchInfo info;
    // SDA_CHACHA_PATH=stream: test hook forcing the stream path (both paths are exact; the tests
    // compare them at sizes the oracle cannot finish)
    const char* force = getenv("SDA_CHACHA_PATH");
    if (!sda::chacha_needs_stream_path(m) && !(force && strcmp(force, "stream") == 0)) {
        if (sda_status e = ensure(&h->work, &h->work_bytes, sda::chacha_work_bytes(D, n))) return e;
        bool overflow = false;
        int fixups = 0;
        HIP_TRY(sda::launch_chacha_mask_combine(m, D, seeds, w, n, out, h->work, st, &overflow, &fixups, &info));
        record_chacha(h, info);
        if (!overflow) return SDA_OK;
        info.path = sda::kChachaOverflow;        // grid_y and fixups stay those of the fast attempt
    } else {
        info.path = sda::kChachaStream;
    }
    if (sda_status e = ensure(&h->work, &h->work_bytes, sda::chacha_stream_work_bytes(D, n, m))) return e;
    HIP_TRY(sda::launch_chacha_streams_combine(m, D, seeds, w, n, out, h->work, st));
    record_chacha(h, info);
    return SDA_OK;
}

// chacha_combine for a pipeline that keeps queueing work behind the mask: the rejection count is copied
// to the handle's pinned word instead of being waited for, and chacha_combine_end -- called after the
// pipeline's own final stream sync -- applies the fix-ups (each draw is rejected with probability
// < 2^-28 on this path, so a call rarely has any).  *changed tells the caller to redo what it queued on
// `out`.  Moduli that need the stream path run it synchronously in _begin, as chacha_combine does.
struct PendingChacha {
    bool pending = false;
    int64_t m = 0;
    uint64_t D = 0, n = 0;
    const uint32_t* seeds = nullptr;
    uint32_t w = 0;
    int64_t* out = nullptr;
};
sda_status chacha_combine_begin(sda_engine* h, int64_t m, uint64_t D, const uint32_t* seeds, uint32_t w, uint64_t n,
                                int64_t* out, hipStream_t st, PendingChacha* pc) {
    *pc = PendingChacha{};
    if (D == 0) return SDA_OK;
    const char* force = getenv("SDA_CHACHA_PATH");
    if (sda::chacha_needs_stream_path(m) || (force && strcmp(force, "stream") == 0) || n == 0)
        return chacha_combine(h, m, D, seeds, w, n, out, st);
    if (sda_status e = ensure(&h->work, &h->work_bytes, sda::chacha_work_bytes(D, n))) return e;
    sda::ChachaLaunchInfo info;
    HIP_TRY(sda::launch_chacha_mask_combine_async(m, D, seeds, w, n, out, h->work, st, h->rej_host, &info));
    record_chacha(h, info);
    *pc = PendingChacha{true, m, D, n, seeds, w, out};
    return SDA_OK;
}
sda_status chacha_combine_end(sda_engine* h, const PendingChacha& pc, hipStream_t st, bool* changed) {
    *changed = false;
    if (!pc.pending || *h->rej_host == 0) return SDA_OK;
    *changed = true;
    bool overflow = false;
    int fixups = 0;
    HIP_TRY(sda::resolve_chacha_mask_combine(pc.m, pc.D, pc.seeds, pc.w, pc.n, pc.out, h->work, st, *h->rej_host,
                                             &overflow, &fixups));
    h->chacha_last.fixups = (uint64_t)fixups;    // the late resolve of the plan chacha_combine_begin recorded
    if (!overflow) return SDA_OK;
    if (sda_status e = ensure(&h->work, &h->work_bytes, sda::chacha_stream_work_bytes(pc.D, pc.n, pc.m))) return e;
    HIP_TRY(sda::launch_chacha_streams_combine(pc.m, pc.D, pc.seeds, pc.w, pc.n, pc.out, h->work, st));
    h->chacha_last.path = sda::kChachaOverflow;
    return SDA_OK;
}

// chacha.rs:36-45: masked = (secrets + draw) % m for one seed (host words); mask = scratch of D values
sda_status chacha_mask(sda_engine* h, int64_t m, const uint32_t* seed_host, uint32_t w, const int64_t* secrets,
                       uint64_t D, int64_t* mask, uint32_t* seed_dev, int64_t* masked, hipStream_t st) {
    if (D == 0) return SDA_OK;
    if (w) HIP_TRY(hipMemcpyAsync(seed_dev, seed_host, w * 4, hipMemcpyHostToDevice, st));
    if (sda_status e = chacha_combine(h, m, D, seed_dev, w, 1, mask, st)) return e;   // one stream == its draws
    HIP_TRY(sda::launch_addsub_trem(secrets, mask, +1, D, masked, m, st));
    return SDA_OK;
}

sda_status finish(sda_engine* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ok();
}

// streaming, multi-device host path (defined at the end of this file)
sda_status host_combine(sda_engine* h, int64_t m, const int64_t* const* rows, uint64_t n_rows, uint64_t dim,
                        int64_t* out);
sda_status host_chacha_combine(sda_engine* h, int64_t m, uint64_t D, const std::vector<uint32_t>& seeds, uint32_t w,
                               uint64_t n, int64_t* out_host);
void destroy_comms(sda_engine* h);
sda_status chacha_combine_multi(sda_engine* h, int64_t m, uint64_t D, const std::vector<uint32_t>& seeds, uint32_t w,
                                uint64_t n, int64_t* dst);
sda_status host_stream_ensure(sda_engine* h, size_t tile_bytes, size_t acc_bytes);
sda_status host_decode_combine(sda_engine* h, int64_t m, const uint8_t* const* blobs, const uint64_t* lens, uint64_t n,
                               int64_t* out, uint64_t out_cap, uint64_t* out_len);
// kd != nullptr (sda_share_generate_keyed): `draws` is NULL and every device makes its own slice of them
struct KeyedDraws {
    const uint32_t* key;          // host, 8 words
    uint32_t stream_id;
};
sda_status host_additive_generate(sda_engine* h, int64_t m, uint64_t n, const int64_t* secrets, uint64_t D,
                                  const int64_t* draws, int64_t* out, const KeyedDraws* kd = nullptr);
sda_status host_packed_generate(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets, uint64_t D,
                                const int64_t* draws, int64_t* out, const KeyedDraws* kd = nullptr);
sda_status host_packed_reconstruct(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                   const uint64_t* indices, const int64_t* const* rows, uint64_t n_rows, int64_t* out);

}  // namespace

extern "C" {

int sda_abi_version(void) { return SDA_ENGINE_ABI_VERSION; }

const char* sda_last_error_message(void) { return g_last_error.c_str(); }

const char* sda_status_string(int st) {
    SDA_ENTRY;
    switch (st) {
        case SDA_OK: return "ok";
        case SDA_ERR_BATCH_INPUT_WRONG_LENGTH: return "Batch input wrong length";
        case SDA_ERR_PACKED_SHARING_FAILED: return "Sharing failed for packed secret sharing scheme";
        case SDA_ERR_WRONG_DIMENSION: return "Wrong dimension";
        case SDA_ERR_MISMATCHING_DIMENSION: return "Mismatching dimension";
        case SDA_ERR_INPUTS_MUST_HAVE_SAME_LENGTH: return "Inputs must have same length";
        case SDA_ERR_NOT_ENOUGH_SHARES: return "Not enough shares to reconstruct";
        case SDA_ERR_PRECONDITION: return "precondition violated (the reference panics here)";
        case SDA_ERR_INVALID_ARGUMENT: return "invalid argument";
        case SDA_ERR_UNSUPPORTED: return "unsupported parameters";
        case SDA_ERR_DEVICE: return "device error";
        case SDA_ERR_OUT_OF_MEMORY: return "out of device memory";
    }
    return "unknown status";
}

sda_status sda_engine_create(int device_ordinal, sda_engine** out) {
    SDA_ENTRY;
    if (!out) return fail(SDA_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device_ordinal < 0 || device_ordinal >= n)
        return fail(SDA_ERR_INVALID_ARGUMENT, "device %d out of range (%d devices)", device_ordinal, n);
    HIP_TRY(hipSetDevice(device_ordinal));
    sda_engine* h = new sda_engine();
    h->device = device_ordinal;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&h->rej_host), 64, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (h->order_ev) (void)hipEventDestroy(h->order_ev);
        if (h->stream) (void)hipStreamDestroy(h->stream);
        delete h;
        return fail(SDA_ERR_DEVICE, "hipStreamCreate/hipEventCreate: %s", hipGetErrorString(e));
    }
    h->last_stream = h->stream;
    hbm_engine_opened(device_ordinal);
    *out = h;
    return ok();
}

void sda_engine_destroy(sda_engine* h) {
    SDA_ENTRY;
    if (!h) return;
    if (t_call_h == h) t_call_h = nullptr;
    if (h->comms) {                          // the handle's RCCL communicators (multi-device reduce)
        destroy_comms(h);
    }
    for (size_t g = 1; g < h->sub.size(); ++g) sda_engine_destroy(h->sub[g]);
    h->sub.clear();
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();            // _dev work may still be queued on callers' streams
    dev_free(h->work);
    dev_free(h->gen_log);
    dev_free(h->gen32_tmp);
    dev_free(h->codec_work);
    dev_free(h->codec_mat);
    dev_free(h->pipe);
    dev_free(h->snap);
    dev_free(h->stage);
    sda::free_table(h->gen_tab);
    sda::free_table(h->rev_tab);
    if (h->rej_host) (void)hipHostFree(h->rej_host);
    if (h->hs_pin) (void)hipHostFree(h->hs_pin);
    dev_free(h->hs_dev);
    for (int b = 0; b < 2; ++b) {
        if (h->h2d_done[b]) (void)hipEventDestroy(h->h2d_done[b]);
        if (h->tile_free[b]) (void)hipEventDestroy(h->tile_free[b]);
    }
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if (h->order_ev) (void)hipEventDestroy(h->order_ev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    // the device's last engine handle gives its pooled sda_hbm_alloc buffers back to the driver (with other
    // handles alive, buffers they or torch freed stay pooled for them)
    if (hbm_engine_closed(h->device)) (void)sda_hbm_trim(h->device, 0);
    delete h;
}

sda_status sda_engine_synchronize(sda_engine* h) {
    SDA_ENTRY;
    if (!h) return fail(SDA_ERR_INVALID_ARGUMENT, "engine handle is NULL");
    for (size_t g = 0; g < (h->sub.empty() ? 1 : h->sub.size()); ++g) {   // every device of a multi-device handle
        HIP_TRY(hipSetDevice(h->sub.empty() ? h->device : h->sub[g]->device));
        HIP_TRY(hipDeviceSynchronize());
    }
    HIP_TRY(hipSetDevice(h->device));
    return ok();
}

// ---------------- protocol/src/crypto.rs:117-155 ----------------
uint64_t sda_scheme_input_size(const sda_sharing_scheme* s) {
    SDA_ENTRY;
    return s->kind == SDA_SHARING_ADDITIVE ? 1 : s->secret_count;
}
uint64_t sda_scheme_output_size(const sda_sharing_scheme* s) { return s->share_count; }
uint64_t sda_scheme_privacy_threshold(const sda_sharing_scheme* s) {
    SDA_ENTRY;
    return s->kind == SDA_SHARING_ADDITIVE ? s->share_count - 1 : s->privacy_threshold;
}
uint64_t sda_scheme_reconstruction_threshold(const sda_sharing_scheme* s) {
    SDA_ENTRY;
    return s->kind == SDA_SHARING_ADDITIVE ? s->share_count : s->privacy_threshold + s->secret_count;
}
uint64_t sda_share_length(const sda_sharing_scheme* s, uint64_t dimension) {
    SDA_ENTRY;
    const uint64_t k = sda_scheme_input_size(s);
    return k ? (dimension + k - 1) / k : 0;
}

// ---------------- ShareGenerator::generate ----------------
sda_status sda_share_generate(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets, uint64_t D,
                              const int64_t* draws, uint64_t n_draws, int64_t* out, uint64_t out_cap) {
    SDA_ENTRY;
    if (!h || !s) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL handle or scheme");
    if ((D && !secrets) || (n_draws && !draws)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL input buffer");
    HIP_TRY(hipSetDevice(h->device));
    if (s->kind == SDA_SHARING_ADDITIVE) {
        const uint64_t n = s->share_count;
        if (n == 0) return fail(SDA_ERR_PRECONDITION, "share_count - 1 underflows (additive.rs:42)");
        if (s->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
        if (n_draws != D * (n - 1))
            return fail(SDA_ERR_INVALID_ARGUMENT, "expected %llu draws (dimension * (share_count - 1)), got %llu",
                        (unsigned long long)(D * (n - 1)), (unsigned long long)n_draws);
        if (out_cap < n * D) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
        if (D == 0) return ok();
        (void)pick(h, h->stream);
        if (sda_status st = host_additive_generate(h, s->modulus, n, secrets, D, draws, out)) return st;
        return ok();
    }
    if (s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    if (sda_status st = check_packed(s)) return st;
    const uint64_t k = s->secret_count, t = s->privacy_threshold, n = s->share_count;
    const uint64_t B = (D + k - 1) / k;
    if (n_draws != B * t)
        return fail(SDA_ERR_INVALID_ARGUMENT, "expected %llu draws (batches * privacy_threshold), got %llu",
                    (unsigned long long)(B * t), (unsigned long long)n_draws);
    if (out_cap < n * B) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    if (B == 0) return ok();
    (void)pick(h, h->stream);
    if (sda_status st = host_packed_generate(h, s, secrets, D, draws, out)) return st;
    return ok();
}

// sda_share_generate with its draws made on the device (draws.hip): every scheme check, status and output layout
// of sda_share_generate; each device of a multi-device handle draws its own slice, so the result does not depend
// on the device count.
sda_status sda_share_generate_keyed(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets, uint64_t D,
                                    const uint32_t* key, uint32_t stream_id, int64_t* out, uint64_t out_cap) {
    SDA_ENTRY;
    if (!h || !s || !key) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL handle, scheme or key");
    if (D && !secrets) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL input buffer");
    HIP_TRY(hipSetDevice(h->device));
    const KeyedDraws kd{key, stream_id};
    if (s->kind == SDA_SHARING_ADDITIVE) {
        const uint64_t n = s->share_count;
        if (n == 0) return fail(SDA_ERR_PRECONDITION, "share_count - 1 underflows (additive.rs:42)");
        if (s->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
        if (out_cap < n * D || (n * D && !out)) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
        if (D == 0) return ok();
        (void)pick(h, h->stream);
        if (sda_status st = host_additive_generate(h, s->modulus, n, secrets, D, nullptr, out, &kd)) return st;
        return ok();
    }
    if (s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    if (sda_status st = check_packed(s)) return st;
    const uint64_t k = s->secret_count, n = s->share_count;
    const uint64_t B = (D + k - 1) / k;
    if (out_cap < n * B || (n * B && !out)) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    if (B == 0) return ok();
    (void)pick(h, h->stream);
    if (sda_status st = host_packed_generate(h, s, secrets, D, nullptr, out, &kd)) return st;
    return ok();
}

// ---------------- ShareCombiner::combine ----------------
static sda_status combine_rows(sda_engine* h, int64_t modulus, const int64_t* const* rows, const uint64_t* lens,
                               uint64_t n_rows, int64_t* out, uint64_t out_cap, uint64_t* out_len,
                               sda_status dim_err, const char* dim_msg) {
    if (!h || (n_rows && (!rows || !lens)) || !out_len) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t dim = n_rows ? lens[0] : 0;              // combiner.rs:17
    *out_len = 0;
    int64_t m;
    // combiner.rs:20-25 / additive.rs:62-67: row 0 (of length dim) is folded -- `%= 0` panics there --
    // before row 1's length is checked
    if (dim && modulus == 0) return modulus_abs(modulus, &m);
    for (uint64_t i = 0; i < n_rows; ++i)
        if (lens[i] != dim) return fail(dim_err, "%s (row %llu has %llu elements, expected %llu)", dim_msg,
                                        (unsigned long long)i, (unsigned long long)lens[i],
                                        (unsigned long long)dim);
    if (dim && n_rows) {
        if (sda_status st = modulus_abs(modulus, &m)) return st;
    } else {
        m = 1;
    }
    if (out_cap < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    *out_len = dim;
    if (dim == 0) return ok();
    for (uint64_t i = 0; i < n_rows; ++i)
        if (!rows[i]) return fail(SDA_ERR_INVALID_ARGUMENT, "row %llu is NULL", (unsigned long long)i);
    (void)pick(h, h->stream);                  // host entry points run on the engine's own stream(s)
    // row tiles through pinned double buffers, column slices over the handle's devices (host path section):
    // jobs larger than HBM stream through, bit-identical to one pass
    if (sda_status st = host_combine(h, m, rows, n_rows, dim, out)) return st;
    return ok();
}

sda_status sda_share_combine(sda_engine* h, const sda_sharing_scheme* s, const int64_t* const* rows,
                             const uint64_t* lens, uint64_t n_rows, int64_t* out, uint64_t out_cap,
                             uint64_t* out_len) {
    SDA_ENTRY;
    if (!s) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL scheme");
    // sharing/mod.rs:61-69: Additive -> modulus, PackedShamir -> prime_modulus (same field here)
    return combine_rows(h, s->modulus, rows, lens, n_rows, out, out_cap, out_len, SDA_ERR_WRONG_DIMENSION,
                        "Wrong dimension");
}

// ---------------- SecretReconstructor::reconstruct ----------------
sda_status sda_secret_reconstruct(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                  const uint64_t* indices, const int64_t* const* rows, const uint64_t* lens,
                                  uint64_t n_rows, int64_t* out, uint64_t out_cap, uint64_t* out_len) {
    SDA_ENTRY;
    if (!h || !s || !out_len) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (s->kind == SDA_SHARING_ADDITIVE) {
        // additive.rs:56-72: dimension = first row's length; indices are ignored
        return combine_rows(h, s->modulus, rows, lens, n_rows, out, out_cap, out_len,
                            SDA_ERR_MISMATCHING_DIMENSION, "Mismatching dimension");
    }
    if (s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    if (sda_status st = check_packed(s)) return st;
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t k = s->secret_count;
    const uint64_t B = (dimension + k - 1) / k;             // batched.rs:77
    *out_len = 0;
    if (out_cap < dimension) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    if (B == 0) { *out_len = 0; return ok(); }              // no batch => no error checks run
    if (n_rows && (!rows || !lens || !indices)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // batched.rs:82-86: batch 0 gathers [clerk][0] (a panic on an empty row), then
    // packed_shamir.rs:75 may fail; any later batch b panics on a row shorter than b + 1
    const bool enough = n_rows >= s->privacy_threshold + k;
    for (uint64_t i = 0; i < n_rows; ++i)
        if (lens[i] < (enough ? B : 1))
            return fail(SDA_ERR_PRECONDITION, "index out of bounds: row %llu has %llu < %llu batches",
                        (unsigned long long)i, (unsigned long long)lens[i], (unsigned long long)(enough ? B : 1));
    if (!enough)
        return fail(SDA_ERR_NOT_ENOUGH_SHARES, "Not enough shares to reconstruct (%llu < %llu)",
                    (unsigned long long)n_rows, (unsigned long long)(s->privacy_threshold + k));
    if (n_rows > sda::kRevealMaxShares)
        return fail(SDA_ERR_UNSUPPORTED, "more than %u clerk shares per batch", sda::kRevealMaxShares);
    (void)pick(h, h->stream);
    if (sda_status st = host_packed_reconstruct(h, s, dimension, indices, rows, n_rows, out)) return st;
    *out_len = dimension;
    return ok();
}

// ---------------- masking ----------------
sda_status sda_secret_mask(sda_engine* h, const sda_masking_scheme* s, const int64_t* secrets, uint64_t D,
                           const uint32_t* seed, uint64_t seed_words, const int64_t* full_masks, int64_t* mask_out,
                           uint64_t mask_cap, uint64_t* mask_len, int64_t* masked_out) {
    SDA_ENTRY;
    if (!h || !s || !mask_len || (D && (!secrets || !masked_out)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    *mask_len = 0;
    if (s->kind == SDA_MASKING_NONE) {                      // none.rs:14-19
        if (D) memcpy(masked_out, secrets, D * 8);
        return ok();
    }
    if (s->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    if (s->kind == SDA_MASKING_FULL) {                      // full.rs:22-35
        if (D && !full_masks) return fail(SDA_ERR_INVALID_ARGUMENT, "Full masking needs the drawn masks");
        if (mask_cap < D) return fail(SDA_ERR_INVALID_ARGUMENT, "mask buffer too small");
        if (D == 0) return ok();
        DevArena a;
        if (sda_status st = stage(h, 3 * rup(D * 8), &a)) return st;
        int64_t* ds = a.take<int64_t>(D);
        int64_t* dm = a.take<int64_t>(D);
        int64_t* dout = a.take<int64_t>(D);
        HIP_TRY(hipMemcpyAsync(ds, secrets, D * 8, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dm, full_masks, D * 8, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(sda::launch_addsub_trem(ds, dm, +1, D, dout, s->modulus, h->stream));
        HIP_TRY(hipMemcpyAsync(masked_out, dout, D * 8, hipMemcpyDeviceToHost, h->stream));
        memcpy(mask_out, full_masks, D * 8);
        *mask_len = D;
        return finish(h);
    }
    if (s->kind != SDA_MASKING_CHACHA) return fail(SDA_ERR_INVALID_ARGUMENT, "unknown masking scheme kind");
    // chacha.rs:26 assert_eq!(self.dimension, secrets.len())
    if (s->dimension != D) return fail(SDA_ERR_PRECONDITION, "assertion failed: dimension == secrets.len()");
    const uint64_t want_words = (s->seed_bitsize + 31) / 32;   // chacha.rs:30
    if (seed_words != want_words || (seed_words && !seed))
        return fail(SDA_ERR_PRECONDITION, "expected %llu seed words for seed_bitsize %llu",
                    (unsigned long long)want_words, (unsigned long long)s->seed_bitsize);
    if (mask_cap < seed_words) return fail(SDA_ERR_INVALID_ARGUMENT, "mask buffer too small");
    for (uint64_t i = 0; i < seed_words; ++i) mask_out[i] = (int64_t)seed[i];   // chacha.rs:48-50
    *mask_len = seed_words;
    if (D == 0) return ok();
    const uint32_t w = (uint32_t)(seed_words < 8 ? seed_words : 8);           // key holds 8 words
    DevArena a;
    if (sda_status st = stage(h, 3 * rup(D * 8) + rup(64), &a)) return st;
    int64_t* ds = a.take<int64_t>(D);
    int64_t* dmask = a.take<int64_t>(D);
    int64_t* dout = a.take<int64_t>(D);
    uint32_t* dseed = a.take<uint32_t>(16);
    HIP_TRY(hipMemcpyAsync(ds, secrets, D * 8, hipMemcpyHostToDevice, h->stream));
    if (sda_status st = chacha_mask(h, s->modulus, seed, w, ds, D, dmask, dseed, dout, h->stream)) return st;
    HIP_TRY(hipMemcpyAsync(masked_out, dout, D * 8, hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

// Full masking (full.rs:22-35) with the mask drawn on the device: element d of (key, stream_id), bound = modulus
sda_status sda_secret_mask_keyed(sda_engine* h, const sda_masking_scheme* s, const int64_t* secrets, uint64_t D,
                                 const uint32_t* key, uint32_t stream_id, int64_t* mask_out, uint64_t mask_cap,
                                 uint64_t* mask_len, int64_t* masked_out) {
    SDA_ENTRY;
    if (!h || !s || !key || !mask_len || (D && (!secrets || !masked_out || !mask_out)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *mask_len = 0;
    if (s->kind != SDA_MASKING_FULL)
        return fail(SDA_ERR_INVALID_ARGUMENT,
                    "sda_secret_mask_keyed draws Full masks only: None draws nothing and ChaCha expands its own "
                    "seed (use sda_secret_mask)");
    if (s->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    if (mask_cap < D) return fail(SDA_ERR_INVALID_ARGUMENT, "mask buffer too small");
    if (D == 0) return ok();
    HIP_TRY(hipSetDevice(h->device));
    DevArena a;
    if (sda_status st = stage(h, 3 * rup(D * 8), &a)) return st;
    int64_t* ds = a.take<int64_t>(D);
    int64_t* dm = a.take<int64_t>(D);
    int64_t* dout = a.take<int64_t>(D);
    HIP_TRY(hipMemcpyAsync(ds, secrets, D * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(sda::launch_draws(key, stream_id, 0, D, s->modulus, dm, h->stream));
    HIP_TRY(sda::launch_addsub_trem(ds, dm, +1, D, dout, s->modulus, h->stream));
    HIP_TRY(hipMemcpyAsync(masked_out, dout, D * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(mask_out, dm, D * 8, hipMemcpyDeviceToHost, h->stream));
    *mask_len = D;
    return finish(h);
}

sda_status sda_mask_combine(sda_engine* h, const sda_masking_scheme* s, const int64_t* const* rows,
                            const uint64_t* lens, uint64_t n_rows, int64_t* out, uint64_t out_cap,
                            uint64_t* out_len) {
    SDA_ENTRY;
    if (!h || !s || !out_len || (n_rows && (!rows || !lens))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_len = 0;
    if (s->kind == SDA_MASKING_NONE) {                      // none.rs:22-25
        for (uint64_t i = 0; i < n_rows; ++i)
            if (lens[i]) return fail(SDA_ERR_PRECONDITION, "assertion failed: masks.iter().all(|mask| mask.len() == 0)");
        return ok();
    }
    if (s->kind == SDA_MASKING_FULL) {                      // full.rs:38-50 (panics on mismatch)
        const uint64_t dim = n_rows ? lens[0] : 0;
        for (uint64_t i = 0; i < n_rows; ++i)
            if (lens[i] != dim) return fail(SDA_ERR_PRECONDITION, "assertion failed: mask.len() == dimension");
        return combine_rows(h, s->modulus, rows, lens, n_rows, out, out_cap, out_len, SDA_ERR_PRECONDITION,
                            "assertion failed");
    }
    if (s->kind != SDA_MASKING_CHACHA) return fail(SDA_ERR_INVALID_ARGUMENT, "unknown masking scheme kind");
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t D = s->dimension;                        // chacha.rs:58 vec![0; self.dimension]
    if (out_cap < D) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    if (D && s->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    uint64_t w = 0;
    for (uint64_t i = 0; i < n_rows; ++i) w = lens[i] > w ? lens[i] : w;
    if (w > 8) w = 8;                                       // ChaChaRng key = first 8 seed words
    if (w == 0) w = 1;                                      // empty seeds == all-zero key
    std::vector<uint32_t> seeds(n_rows * w, 0u);            // shorter seeds pad with zero key words
    for (uint64_t i = 0; i < n_rows; ++i)
        for (uint64_t j = 0; j < lens[i] && j < w; ++j) seeds[i * w + j] = (uint32_t)rows[i][j];   // chacha.rs:62-64
    *out_len = D;
    if (D == 0) return ok();
    // seeds split over the handle's devices, one RCCL reduce (host path section); one device: all seeds
    if (sda_status st = host_chacha_combine(h, s->modulus, D, seeds, (uint32_t)w, n_rows, out)) return st;
    return ok();
}

sda_status sda_secret_unmask(sda_engine* h, const sda_masking_scheme* s, const int64_t* mask, uint64_t mask_len,
                             const int64_t* masked, uint64_t masked_len, int64_t* out, uint64_t out_cap,
                             uint64_t* out_len) {
    SDA_ENTRY;
    if (!h || !s || !out_len || (masked_len && (!masked || !out))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_len = 0;
    if (out_cap < masked_len) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    if (s->kind == SDA_MASKING_NONE) {                      // none.rs:28-32
        if (mask_len != 0) return fail(SDA_ERR_PRECONDITION, "assertion failed: values.0.len() == 0");
        if (masked_len) memcpy(out, masked, masked_len * 8);
        *out_len = masked_len;
        return ok();
    }
    if (s->kind != SDA_MASKING_FULL && s->kind != SDA_MASKING_CHACHA)
        return fail(SDA_ERR_INVALID_ARGUMENT, "unknown masking scheme kind");
    if (mask_len != masked_len) return fail(SDA_ERR_PRECONDITION, "assertion failed: mask.len() == masked_secrets.len()");
    *out_len = masked_len;
    if (masked_len == 0) return ok();
    int64_t m;
    if (sda_status st = modulus_abs(s->modulus, &m)) return st;
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t D = masked_len;
    DevArena a;
    if (sda_status st = stage(h, 3 * rup(D * 8), &a)) return st;
    int64_t* dm = a.take<int64_t>(D);
    int64_t* dms = a.take<int64_t>(D);
    int64_t* dout = a.take<int64_t>(D);
    HIP_TRY(hipMemcpyAsync(dm, mask, D * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dms, masked, D * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(sda::launch_addsub_trem(dms, dm, -1, D, dout, m, h->stream));      // (ms - m) % q
    HIP_TRY(hipMemcpyAsync(out, dout, D * 8, hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

sda_status sda_recipient_positive(sda_engine* h, int64_t modulus, const int64_t* values, uint64_t n, int64_t* out) {
    SDA_ENTRY;
    if (!h || (n && (!values || !out))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n == 0) return ok();
    HIP_TRY(hipSetDevice(h->device));
    DevArena a;
    if (sda_status st = stage(h, 2 * rup(n * 8), &a)) return st;
    int64_t* dv = a.take<int64_t>(n);
    int64_t* dout = a.take<int64_t>(n);
    HIP_TRY(hipMemcpyAsync(dv, values, n * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(sda::launch_positive(dv, n, dout, modulus, h->stream));
    HIP_TRY(hipMemcpyAsync(out, dout, n * 8, hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

// ---------------- device-resident entry points ----------------
sda_status sda_combine_dev(sda_engine* h, int64_t modulus, const int64_t* shares, uint64_t n, uint64_t dim,
                           uint64_t row_stride, int64_t* out, void* stream) {
    SDA_ENTRY;
    if (!h || (dim && (!out || (n && !shares)))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > 1 && row_stride < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "row_stride < dim");
    int64_t m;
    if (sda_status st = modulus_abs(modulus, &m)) return st;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_combine_exact(shares, n, dim, n > 1 ? row_stride : dim, out, m, pick(h, stream), false,
                                      &h->combine_last));
    return ok();
}

sda_status sda_combine_accumulate_dev(sda_engine* h, int64_t modulus, const int64_t* shares, uint64_t n,
                                      uint64_t dim, uint64_t row_stride, int64_t* inout, void* stream) {
    SDA_ENTRY;
    if (!h || (dim && (!inout || (n && !shares)))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > 1 && row_stride < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "row_stride < dim");
    int64_t m;
    if (sda_status st = modulus_abs(modulus, &m)) return st;
    HIP_TRY(hipSetDevice(h->device));
    if (n == 0) return ok();
    HIP_TRY(sda::launch_combine_exact(shares, n, dim, n > 1 ? row_stride : dim, inout, m, pick(h, stream), true,
                                      &h->combine_last));
    return ok();
}

// int32 share rows (|v| < 2^31: every shipped configuration): half the bytes per share; the kernels sign-extend
// and run the i64 recurrence, so the result is that of the widened rows for any modulus
sda_status sda_combine32_dev(sda_engine* h, int64_t modulus, const int32_t* shares, uint64_t n, uint64_t dim,
                             uint64_t row_stride, int64_t* out, void* stream) {
    SDA_ENTRY;
    if (!h || (dim && (!out || (n && !shares)))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > 1 && row_stride < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "row_stride < dim");
    int64_t m;
    if (sda_status st = modulus_abs(modulus, &m)) return st;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_combine_wide32(shares, n, dim, n > 1 ? row_stride : dim, out, m, pick(h, stream), false,
                                       &h->combine_last));
    return ok();
}

sda_status sda_combine32_accumulate_dev(sda_engine* h, int64_t modulus, const int32_t* shares, uint64_t n,
                                        uint64_t dim, uint64_t row_stride, int64_t* inout, void* stream) {
    SDA_ENTRY;
    if (!h || (dim && (!inout || (n && !shares)))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > 1 && row_stride < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "row_stride < dim");
    int64_t m;
    if (sda_status st = modulus_abs(modulus, &m)) return st;
    HIP_TRY(hipSetDevice(h->device));
    if (n == 0) return ok();
    HIP_TRY(sda::launch_combine_wide32(shares, n, dim, n > 1 ? row_stride : dim, inout, m, pick(h, stream), true,
                                       &h->combine_last));
    return ok();
}

sda_status sda_narrow32_dev(sda_engine* h, const int64_t* src, uint64_t n, uint64_t dim, uint64_t src_stride,
                            int32_t* dst, uint64_t dst_stride, int64_t* flag, void* stream) {
    SDA_ENTRY;
    if (!h || (n && dim && (!src || !dst || !flag))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > 1 && (src_stride < dim || dst_stride < dim)) return fail(SDA_ERR_INVALID_ARGUMENT, "row stride < dim");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_narrow32(src, n, dim, n > 1 ? src_stride : dim, dst, n > 1 ? dst_stride : dim, flag,
                                 pick(h, stream)));
    return ok();
}

sda_status sda_host_stream_stats(const sda_engine* h, uint64_t* tiles_i32, uint64_t* tiles_i64,
                                 uint64_t* bytes_h2d) {
    SDA_ENTRY;
    if (!h) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    uint64_t t32 = 0, t64 = 0, by = 0;
    auto add = [&](const sda_engine* e) {
        t32 += e->hs_tiles32;
        t64 += e->hs_tiles64;
        by += e->hs_bytes_h2d;
    };
    if (h->sub.empty()) add(h);
    for (const sda_engine* e : h->sub) add(e);           // sub[0] is the handle itself
    if (tiles_i32) *tiles_i32 = t32;
    if (tiles_i64) *tiles_i64 = t64;
    if (bytes_h2d) *bytes_h2d = by;
    return ok();
}

sda_status sda_packed_fixup_count(sda_engine* h, uint64_t* batches) {
    SDA_ENTRY;
    if (!h || !batches) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *batches = 0;
    uint64_t total = 0;
    auto add = [&](sda_engine* e) -> sda_status {
        if (!e->gen_log || !e->gen_log_used) return SDA_OK;
        HIP_TRY(hipSetDevice(e->device));
        // the last call's stream may be gone (pick()): wait on the event that call recorded when it ended, and
        // on the handle's own stream (the host entry points' launches)
        if (e->order_ok) HIP_TRY(hipEventSynchronize(e->order_ev));
        else HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipStreamSynchronize(e->stream));
        unsigned int n = 0;
        HIP_TRY(hipMemcpy(&n, e->gen_log, sizeof(n), hipMemcpyDeviceToHost));
        total += n;
        return SDA_OK;
    };
    if (h->sub.empty()) {
        if (sda_status st = add(h)) return st;
    }
    for (sda_engine* e : h->sub)                          // sub[0] is the handle itself
        if (sda_status st = add(e)) return st;
    if (!h->sub.empty()) HIP_TRY(hipSetDevice(h->device));
    *batches = total;
    return ok();
}

sda_status sda_chacha_last_launch(sda_engine* h, uint32_t* path, uint64_t* grid_y, uint64_t* fixups) {
    SDA_ENTRY;
    if (!h || !path || !grid_y || !fixups) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // host-side records, final when the call that made them returned: nothing to wait for
    *path = h->chacha_last.path;
    *grid_y = h->chacha_last.grid_y;
    uint64_t total = h->chacha_last.fixups;
    if (h->chacha_split)
        for (size_t g = 1; g < h->sub.size(); ++g) total += h->sub[g]->chacha_last.fixups;   // sub[0] is the handle
    *fixups = total;
    return ok();
}

sda_status sda_codec_last_launch(sda_engine* h, uint32_t* path, uint32_t* width, uint32_t* fell_back,
                                 uint64_t* passes) {
    SDA_ENTRY;
    if (!h || !path || !width || !fell_back || !passes) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for
    *path = h->codec_last.path;
    *width = h->codec_last.width;
    *fell_back = h->codec_last.fell_back;
    *passes = h->codec_last.passes;
    return ok();
}

sda_status sda_combine_last_launch(sda_engine* h, uint32_t* kind, uint32_t* elem_bytes, uint32_t* vec, uint32_t* rows,
                                   uint32_t* variant, uint64_t* grid, uint32_t* wlo, uint32_t* nwide,
                                   uint32_t* per_cu) {
    SDA_ENTRY;
    if (!h || !kind || !elem_bytes || !vec || !rows || !variant || !grid || !wlo || !nwide || !per_cu)
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for.  A multi-device handle
    // is its own first device (sub[0]): its record is that device's
    const sda::CombineLaunchInfo& c = h->combine_last;
    *kind = c.kind;
    *elem_bytes = c.elem_bytes;
    *vec = c.vec;
    *rows = c.rows;
    *variant = c.variant;
    *grid = c.grid;
    *wlo = c.wlo;
    *nwide = c.nwide;
    *per_cu = c.per_cu;
    return ok();
}

sda_status sda_combine_finalize_dev(sda_engine* h, int64_t modulus, const int64_t* sums, uint64_t dim, int64_t* out,
                                    void* stream) {
    SDA_ENTRY;
    if (!h || (dim && (!sums || !out))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    int64_t m;
    if (sda_status st = modulus_abs(modulus, &m)) return st;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_mod_canonical(sums, dim, out, m, pick(h, stream)));
    return ok();
}

sda_status sda_combine_split_dev(sda_engine* h, int64_t modulus, const int64_t* shares, uint64_t n, uint64_t dim,
                                 uint64_t row_stride, int64_t* inout, int64_t* flags, void* stream) {
    SDA_ENTRY;
    if (!h || (dim && (!inout || !flags || (n && !shares)))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > 1 && row_stride < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "row_stride < dim");
    int64_t m;
    if (sda_status st = modulus_abs(modulus, &m)) return st;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_combine_split(shares, n, dim, n > 1 ? row_stride : dim, inout, m, flags, pick(h, stream),
                                      &h->combine_last));
    return ok();
}

sda_status sda_combine_split_prefix_dev(sda_engine* h, int64_t modulus, const int64_t* gathered, uint64_t world,
                                        uint64_t rank, uint64_t dim, int64_t* c_in, int64_t* total, int32_t* code,
                                        void* stream) {
    SDA_ENTRY;
    if (!h || (dim && (!gathered || !c_in || !total || !code))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (rank >= world || world > (1u << 29)) return fail(SDA_ERR_INVALID_ARGUMENT, "rank %llu of world %llu",
                                                         (unsigned long long)rank, (unsigned long long)world);
    int64_t m;
    if (sda_status st = modulus_abs(modulus, &m)) return st;
    if ((unsigned __int128)world * (uint64_t)(m - 1) > (unsigned __int128)INT64_MAX)
        return fail(SDA_ERR_INVALID_ARGUMENT, "world * (m - 1) exceeds 2^63 - 1");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_split_prefix(gathered, world, rank, dim, c_in, total, code, m, pick(h, stream)));
    return ok();
}

sda_status sda_combine_split_replay_dev(sda_engine* h, int64_t modulus, const int64_t* shares, uint64_t n,
                                        uint64_t dim, uint64_t row_stride, uint64_t rank, int64_t* state,
                                        int32_t* code, void* stream) {
    SDA_ENTRY;
    if (!h || (dim && (!state || !code || (n && !shares)))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > 1 && row_stride < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "row_stride < dim");
    if (rank > (1u << 29)) return fail(SDA_ERR_INVALID_ARGUMENT, "rank %llu too large", (unsigned long long)rank);
    int64_t m;
    if (sda_status st = modulus_abs(modulus, &m)) return st;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_combine_replay(shares, n, dim, n > 1 ? row_stride : dim, state, code, (int32_t)(2 * rank + 1),
                                       m, pick(h, stream), &h->combine_last));
    return ok();
}

sda_status sda_combine_split_resolve_dev(sda_engine* h, int64_t modulus, const int64_t* total, const int32_t* code,
                                         uint64_t dim, int64_t* out, void* stream) {
    SDA_ENTRY;
    if (!h || (dim && (!total || !code || !out))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    int64_t m;
    if (sda_status st = modulus_abs(modulus, &m)) return st;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_split_resolve(total, code, dim, out, m, pick(h, stream)));
    return ok();
}

sda_status sda_packed_generate_dev(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets,
                                   uint64_t dimension, uint64_t n_vectors, const int64_t* draws, int64_t* out,
                                   void* stream) {
    SDA_ENTRY;
    if (!h || !s || s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (sda_status st = check_packed(s)) return st;
    if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
    HIP_TRY(hipSetDevice(h->device));
    sda::PackedGenArgs ga{secrets, dimension, n_vectors, draws, out};
    if (sda_status st = ensure(&h->gen_log, &h->gen_log_bytes, sda::packed_gen_log_bytes())) return st;
    HIP_TRY(sda::launch_packed_generate(ga, (uint32_t)s->secret_count, (uint32_t)s->privacy_threshold,
                                        (uint32_t)s->share_count, (uint32_t)s->modulus, (uint32_t)s->omega_secrets,
                                        (uint32_t)s->omega_shares, h->gen_tab, h->gen_log, pick(h, stream),
                                        &h->gen_log_used));
    return ok();
}

sda_status sda_packed_generate_mode_dev(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets,
                                        uint64_t dimension, uint64_t n_vectors, const int64_t* draws, int64_t* out,
                                        int32_t mode, void* stream) {
    SDA_ENTRY;
    if (!h || !s || s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (mode != SDA_REVEAL_EXACT && mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
    if (sda_status st = check_packed(s)) return st;
    if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
    HIP_TRY(hipSetDevice(h->device));
    sda::PackedGenArgs ga{secrets, dimension, n_vectors, draws, out, mode == SDA_REVEAL_CANONICAL};
    if (sda_status st = ensure(&h->gen_log, &h->gen_log_bytes, sda::packed_gen_log_bytes())) return st;
    HIP_TRY(sda::launch_packed_generate(ga, (uint32_t)s->secret_count, (uint32_t)s->privacy_threshold,
                                        (uint32_t)s->share_count, (uint32_t)s->modulus, (uint32_t)s->omega_secrets,
                                        (uint32_t)s->omega_shares, h->gen_tab, h->gen_log, pick(h, stream),
                                        &h->gen_log_used));
    return ok();
}

sda_status sda_packed_reconstruct_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                      const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                      const int64_t* shares, int64_t* out, int32_t mode, void* stream) {
    SDA_ENTRY;
    if (!h || !s || s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (sda_status st = check_packed(s)) return st;
    if (mode != SDA_REVEAL_EXACT && mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
    if (dimension == 0) return ok();                        // batched.rs:77-81: no batch, no check
    if (n_idx < s->privacy_threshold + s->secret_count)
        return fail(SDA_ERR_NOT_ENOUGH_SHARES, "Not enough shares to reconstruct");
    if (n_idx > sda::kRevealMaxShares)
        return fail(SDA_ERR_UNSUPPORTED, "more than %u clerk shares per batch", sda::kRevealMaxShares);
    if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick(h, stream);
    if (sda_status e = ensure(&h->gen_log, &h->gen_log_bytes, sda::packed_gen_log_bytes())) return e;
    sda::PackedRevealArgs ra{shares, dimension, n_vectors, out};
    hipError_t e = sda::launch_packed_reveal(ra, indices, (uint32_t)n_idx, (uint32_t)s->secret_count,
                                             (uint32_t)s->privacy_threshold,
                                             (uint32_t)s->modulus, (uint32_t)s->omega_secrets,
                                             (uint32_t)s->omega_shares, mode, h->rev_tab, h->gen_log, st,
                                             &h->gen_log_used);
    if (e == hipErrorInvalidValue && mode == SDA_REVEAL_CANONICAL)
        return fail(SDA_ERR_UNSUPPORTED, "canonical reveal needs distinct clerk indices");
    HIP_TRY(e);
    return ok();
}

// int32 shares (every share is a `% p` result, p < 2^31): native int32 kernels, or at n + 1 = 81 the i64 register
// kernels into handle-owned scratch and a narrowing pass (packed_gen.hip, launch_packed_generate)
sda_status sda_packed_generate32_dev(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets,
                                     uint64_t dimension, uint64_t n_vectors, const int64_t* draws, int32_t* out,
                                     int32_t mode, void* stream) {
    SDA_ENTRY;
    if (!h || !s || s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (mode != SDA_REVEAL_EXACT && mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
    if (sda_status st = check_packed(s)) return st;
    if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
    if (dimension && n_vectors && (!out || !secrets || (s->privacy_threshold && !draws)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    sda::PackedGenArgs ga{secrets, dimension, n_vectors, draws, nullptr, mode == SDA_REVEAL_CANONICAL};
    ga.out32 = out;
    const uint32_t k = (uint32_t)s->secret_count, t = (uint32_t)s->privacy_threshold, n = (uint32_t)s->share_count;
    hipStream_t st = pick(h, stream);
    if (sda_status e = ensure(&h->gen_log, &h->gen_log_bytes, sda::packed_gen_log_bytes())) return e;
    if (const size_t tmp = sda::packed_gen32_scratch_bytes(ga, k, t, n, (uint32_t)s->modulus)) {
        if (sda_status e = ensure(&h->gen32_tmp, &h->gen32_tmp_bytes, tmp + 64)) return e;
        ga.scratch = static_cast<int64_t*>(h->gen32_tmp);
        ga.flag = ga.scratch + tmp / sizeof(int64_t);      // launch_narrow32's overflow word: never set here
    }
    HIP_TRY(sda::launch_packed_generate(ga, k, t, n, (uint32_t)s->modulus, (uint32_t)s->omega_secrets,
                                        (uint32_t)s->omega_shares, h->gen_tab, h->gen_log, st, &h->gen_log_used));
    return ok();
}

sda_status sda_packed_reconstruct32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                        const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                        const int32_t* shares, int64_t* out, int32_t mode, void* stream) {
    SDA_ENTRY;
    if (!h || !s || s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (sda_status st = check_packed(s)) return st;
    if (mode != SDA_REVEAL_EXACT && mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
    if (dimension == 0) return ok();                        // batched.rs:77-81: no batch, no check
    if (n_idx < s->privacy_threshold + s->secret_count)
        return fail(SDA_ERR_NOT_ENOUGH_SHARES, "Not enough shares to reconstruct");
    if (n_idx > sda::kRevealMaxShares)
        return fail(SDA_ERR_UNSUPPORTED, "more than %u clerk shares per batch", sda::kRevealMaxShares);
    if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
    if (n_vectors && (!out || !shares || !indices)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick(h, stream);
    if (sda_status e = ensure(&h->gen_log, &h->gen_log_bytes, sda::packed_gen_log_bytes())) return e;
    sda::PackedRevealArgs ra{nullptr, dimension, n_vectors, out};
    ra.shares32 = shares;
    hipError_t e = sda::launch_packed_reveal(ra, indices, (uint32_t)n_idx, (uint32_t)s->secret_count,
                                             (uint32_t)s->privacy_threshold,
                                             (uint32_t)s->modulus, (uint32_t)s->omega_secrets,
                                             (uint32_t)s->omega_shares, mode, h->rev_tab, h->gen_log, st,
                                             &h->gen_log_used);
    if (e == hipErrorInvalidValue && mode == SDA_REVEAL_CANONICAL)
        return fail(SDA_ERR_UNSUPPORTED, "canonical reveal needs distinct clerk indices");
    HIP_TRY(e);
    return ok();
}

sda_status sda_additive_generate_dev(sda_engine* h, int64_t modulus, uint64_t share_count, const int64_t* secrets,
                                     uint64_t dimension, const int64_t* draws, int64_t* out, void* stream) {
    SDA_ENTRY;
    if (!h) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL handle");
    if (share_count == 0) return fail(SDA_ERR_PRECONDITION, "share_count - 1 underflows (additive.rs:42)");
    if (modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_additive_generate(secrets, dimension, draws, share_count, out, modulus, pick(h, stream)));
    return ok();
}

sda_status sda_chacha_mask_combine_dev(sda_engine* h, int64_t modulus, uint64_t dimension, const uint32_t* seeds,
                                       uint64_t w, uint64_t n_seeds, int64_t* out, void* stream) {
    SDA_ENTRY;
    if (!h || (dimension && !out) || (n_seeds && w && !seeds)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (dimension && modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    if (w == 0 || w > 8) return fail(SDA_ERR_INVALID_ARGUMENT, "seed width must be 1..8 words");
    HIP_TRY(hipSetDevice(h->device));
    if (sda_status st = chacha_combine(h, modulus, dimension, seeds, (uint32_t)w, n_seeds, out, pick(h, stream)))
        return st;
    return ok();
}

// The argument checks the two draws entry points share, in the header's order; *out_st is the status to return
// when the result is true (SDA_OK for count == 0: nothing to launch).
static bool draws_done(sda_engine* h, const uint32_t* key, uint64_t first, uint64_t count, int64_t bound,
                       const int64_t* out, sda_status* out_st) {
    if (!h || !key || (count && !out)) {
        *out_st = fail(SDA_ERR_INVALID_ARGUMENT, "NULL handle, key or output buffer");
    } else if (bound <= 0) {
        *out_st = fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    } else if (count && first + (count - 1) < first) {
        *out_st = fail(SDA_ERR_INVALID_ARGUMENT, "first + count wraps past 2^64");
    } else if (count == 0) {
        *out_st = ok();
    } else {
        return false;
    }
    return true;
}

sda_status sda_draws_dev(sda_engine* h, const uint32_t* key, uint32_t stream_id, uint64_t first, uint64_t count,
                         int64_t bound, int64_t* out, void* stream) {
    SDA_ENTRY;
    sda_status st;
    if (draws_done(h, key, first, count, bound, out, &st)) return st;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_draws(key, stream_id, first, count, bound, out, pick(h, stream)));
    return ok();
}

sda_status sda_draws(sda_engine* h, const uint32_t* key, uint32_t stream_id, uint64_t first, uint64_t count,
                     int64_t bound, int64_t* out, uint64_t out_cap) {
    SDA_ENTRY;
    sda_status st;
    if (draws_done(h, key, first, count, bound, out, &st)) return st;
    if (out_cap < count) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    HIP_TRY(hipSetDevice(h->device));
    DevArena a;
    if (sda_status e = stage(h, rup(count * 8), &a)) return e;
    int64_t* dd = a.take<int64_t>(count);
    HIP_TRY(sda::launch_draws(key, stream_id, first, count, bound, dd, h->stream));
    HIP_TRY(hipMemcpyAsync(out, dd, count * 8, hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

sda_status sda_synth_fill_dev(sda_engine* h, int64_t* dst, uint64_t rows, uint64_t cols, uint64_t seed, int64_t lo,
                              int64_t hi, void* stream) {
    SDA_ENTRY;
    if (!h || (rows * cols && !dst)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (hi <= lo) return fail(SDA_ERR_INVALID_ARGUMENT, "need hi > lo");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_synth_fill(dst, rows, cols, seed, lo, hi, pick(h, stream)));
    return ok();
}

}  // extern "C"

// ---------------- HBM buffers built from fixed-size physical chunks ----------------
// A plain hipMalloc of tens of GB takes whatever physical blocks the driver's VRAM manager has free; on a
// box whose VRAM earlier processes left fragmented, that backing can cost share-gen 15 % (the same kernel,
// the same buffer size: 6.45 vs 7.4-7.65 ms, profiles/r04p and r04r).  Buffers mapped from physical
// chunks of a fixed size (hipMemCreate, SDA_HBM_CHUNK_MB, default 64 MiB) ran at the fast rate in every
// case measured, whatever the chunk size (2 MiB - 1 GiB) and whether the chunks were mapped in order or
// shuffled (profiles/r04r).  sda_hbm_alloc / sda_hbm_free give the resident hot-path buffers that backing.
//
// Life cycle ("HBM backing"):
//   - Size classes.  A request of n chunks belongs to class cls(n): n itself up to 4 chunks, then 4..7 x 2^e
//     (at most 25 % above n).  A buffer reserves its class's whole virtual range but maps only the chunks
//     asked for; a later request of the same class reuses it and maps more chunks at the range's never-mapped
//     tail if it needs them.  So a steady stream of jobs -- same sizes or mixed -- finds its buffers in the
//     pool and never trims (tests/abi_c/hbm_cycle.c: 10,000 alloc/free cycles of mixed sizes, nothing retired).
//   - sda_hbm_free never waits: the buffer goes to a per-process pool, still mapped, stamped with the number
//     of device-wide syncs the allocator had begun.  Work queued on any stream may still use it; a reuse
//     waits for one sync begun after the free (hipDeviceSynchronize, outside the allocator's lock).
//     (SDA_HBM_POOL_MB=0 disables the pool: free then syncs the device and releases the buffer at once.)
//   - The pool is bounded: SDA_HBM_POOL_MB (default 32768) per device.  An allocation that finds no pooled
//     buffer of its class first trims the oldest pooled buffers down to that bound; one that hits
//     OUT_OF_MEMORY trims the whole pool and retries once.  sda_hbm_trim trims explicitly, and the last engine
//     handle of a device trims its pool when it is destroyed.
//   - Trimming syncs the device, unmaps the chunks and releases them (the HBM returns to the driver), but
//     the VIRTUAL range stays reserved, retired, for the life of the process: it is never mapped again.
//     Cause (profiles/r05b/hbm_repro_suite_sequence.txt): when a freed range was also returned with
//     hipMemAddressFree, the next hipMemAddressReserve of the same size handed the same range out again, and
//     the GPU's view of the new mapping was inconsistent -- in the suite's own sequence (a buffer touched by
//     torch kernels, freed, the same size allocated at once) `fill_(-1)` followed by `max()` read 0s (twice out
//     of twice), as r04y's share-gen buffer read back a different zero count on every read.  With the range
//     retired the same sequence passes (twice out of twice), as does the whole suite.  Retired ranges cost
//     only address space (2^47 bytes of it per process), and only trims retire any (sda_hbm_stats counts it).
//     SDA_HBM_VA_FREE=1 restores the address free for that A/B (scripts/hbm_repro.sh).
namespace {

struct HbmBuffer {
    int device = 0;
    size_t chunk = 0;
    size_t cls = 0;                                     // reserved chunks (the size class)
    std::vector<hipMemGenericAllocationHandle_t> chunks;   // mapped chunks, from the range's start
    uint64_t freed_ticket = 0;                          // pool only: device syncs begun at free time
    uint64_t freed_seq = 0;                             // pool only: free order (oldest is trimmed first)
    size_t mapped_bytes() const { return chunks.size() * chunk; }
    size_t reserved_bytes() const { return cls * chunk; }
};
std::mutex g_hbm_mu;
std::map<uintptr_t, HbmBuffer> g_hbm;                   // handed out
std::map<uintptr_t, HbmBuffer> g_hbm_pool;              // freed, still mapped
constexpr int kHbmMaxDev = 64;
uint64_t g_hbm_sync_begun[kHbmMaxDev];                  // device-wide syncs the allocator has begun ...
uint64_t g_hbm_sync_done[kHbmMaxDev];                   // ... and the highest such id that has completed
uint64_t g_hbm_retired[kHbmMaxDev];                     // bytes of virtual ranges retired (never remapped)
uint64_t g_hbm_seq = 0;
int g_engines[kHbmMaxDev];                              // live engine handles per device (destroy-time trim)

size_t hbm_chunk_bytes() {
    const char* e = getenv("SDA_HBM_CHUNK_MB");
    const long mb = e ? atol(e) : 64;
    return (size_t)(mb > 0 ? mb : 64) << 20;
}

uint64_t hbm_pool_cap() {
    const char* e = getenv("SDA_HBM_POOL_MB");
    const long long mb = e ? atoll(e) : 32768;
    return (uint64_t)(mb > 0 ? mb : 0) << 20;
}

bool hbm_va_free() {
    const char* e = getenv("SDA_HBM_VA_FREE");
    return e && atoi(e) == 1;
}

// the size class of a request of n chunks: n up to 4, then the next 4..7 x 2^e (at most 25 % more)
size_t hbm_class(size_t n) {
    if (n <= 4) return n;
    size_t e = 0;
    while ((n >> e) >= 8) ++e;                          // n in [4, 8) x 2^e
    const size_t m = (n + ((size_t)1 << e) - 1) >> e;  // ceil(n / 2^e) in 4..8
    return m << e;
}

// One device-wide sync, outside the allocator's lock: afterwards every buffer freed before it began is idle.
hipError_t hbm_sync(int device) {
    uint64_t id;
    {
        std::lock_guard<std::mutex> lk(g_hbm_mu);
        id = ++g_hbm_sync_begun[device];
    }
    const hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(g_hbm_mu);
        if (id > g_hbm_sync_done[device]) g_hbm_sync_done[device] = id;
    }
    return e;
}

bool hbm_idle(const HbmBuffer& b) {   // g_hbm_mu held: a sync begun after its free has completed
    return g_hbm_sync_done[b.device] > b.freed_ticket;
}

// unmap and release the buffer's chunks; the virtual range is retired (kept reserved) unless
// SDA_HBM_VA_FREE=1.  The caller owns the buffer and has made sure no queued work uses it.
void hbm_release(void* ptr, HbmBuffer& b) {
    for (size_t i = 0; i < b.chunks.size(); ++i) (void)hipMemUnmap(static_cast<char*>(ptr) + i * b.chunk, b.chunk);
    for (auto& c : b.chunks) (void)hipMemRelease(c);
    b.chunks.clear();
    if (!ptr) return;
    if (hbm_va_free()) {
        (void)hipMemAddressFree(ptr, b.reserved_bytes());
    } else {
        std::lock_guard<std::mutex> lk(g_hbm_mu);
        g_hbm_retired[b.device] += b.reserved_bytes();
    }
}

bool hbm_owned(void* p) {
    std::lock_guard<std::mutex> lk(g_hbm_mu);
    return g_hbm.count(reinterpret_cast<uintptr_t>(p)) != 0;
}

void hbm_engine_opened(int device) {
    std::lock_guard<std::mutex> lk(g_hbm_mu);
    if (device >= 0 && device < kHbmMaxDev) ++g_engines[device];
}

bool hbm_engine_closed(int device) {
    std::lock_guard<std::mutex> lk(g_hbm_mu);
    return device >= 0 && device < kHbmMaxDev && --g_engines[device] == 0;
}

uint64_t hbm_pooled_bytes(int device) {   // g_hbm_mu held
    uint64_t s = 0;
    for (auto& kv : g_hbm_pool)
        if (kv.second.device == device) s += kv.second.mapped_bytes();
    return s;
}

// Trim the device's pool (oldest first) until at most `keep` bytes stay pooled.  The victims leave the pool
// under the lock; the sync (when one of them may still be in use) and the unmapping run outside it.  The
// device is current.
hipError_t hbm_trim(int device, uint64_t keep) {
    std::vector<std::pair<uintptr_t, HbmBuffer>> victims;
    bool busy = false;
    {
        std::lock_guard<std::mutex> lk(g_hbm_mu);
        uint64_t pooled = hbm_pooled_bytes(device);
        while (pooled > keep) {
            auto old = g_hbm_pool.end();
            for (auto it = g_hbm_pool.begin(); it != g_hbm_pool.end(); ++it)
                if (it->second.device == device &&
                    (old == g_hbm_pool.end() || it->second.freed_seq < old->second.freed_seq))
                    old = it;
            if (old == g_hbm_pool.end()) break;
            pooled -= old->second.mapped_bytes();
            busy = busy || !hbm_idle(old->second);
            victims.emplace_back(old->first, std::move(old->second));
            g_hbm_pool.erase(old);
        }
    }
    if (victims.empty()) return hipSuccess;
    hipError_t e = busy ? hbm_sync(device) : hipSuccess;
    if (e != hipSuccess) {                               // keep them pooled (nothing was unmapped)
        std::lock_guard<std::mutex> lk(g_hbm_mu);
        for (auto& v : victims) g_hbm_pool[v.first] = std::move(v.second);
        return e;
    }
    for (auto& v : victims) hbm_release(reinterpret_cast<void*>(v.first), v.second);
    return hipSuccess;
}

// Map chunks [b.chunks.size(), n) of the buffer's reserved range: fresh chunks at a never-mapped tail.
hipError_t hbm_map_to(void* ptr, HbmBuffer* b, size_t n, const hipMemAllocationProp& prop) {
    const size_t m0 = b->chunks.size();
    hipError_t e = hipSuccess;
    for (size_t i = m0; i < n && e == hipSuccess; ++i) {
        hipMemGenericAllocationHandle_t c;
        e = hipMemCreate(&c, b->chunk, &prop, 0);
        if (e != hipSuccess) break;
        e = hipMemMap(static_cast<char*>(ptr) + i * b->chunk, b->chunk, 0, c, 0);
        if (e != hipSuccess) {
            (void)hipMemRelease(c);
            break;
        }
        b->chunks.push_back(c);
    }
    if (e == hipSuccess && n > m0) {
        hipMemAccessDesc acc = {};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        e = hipMemSetAccess(static_cast<char*>(ptr) + m0 * b->chunk, (n - m0) * b->chunk, &acc, 1);
    }
    if (e != hipSuccess) {   // chunks mapped by this call were never accessed by a kernel: undo them
        for (size_t i = m0; i < b->chunks.size(); ++i) {
            (void)hipMemUnmap(static_cast<char*>(ptr) + i * b->chunk, b->chunk);
            (void)hipMemRelease(b->chunks[i]);
        }
        b->chunks.resize(m0);
    }
    return e;
}

// Reserve a class-sized range and map its first n chunks.
hipError_t hbm_create(int device, size_t n, size_t chunk, const hipMemAllocationProp& prop, void** out, HbmBuffer* b) {
    b->device = device;
    b->chunk = chunk;
    b->cls = hbm_class(n);
    void* ptr = nullptr;
    hipError_t e = hipMemAddressReserve(&ptr, b->reserved_bytes(), chunk, nullptr, 0);
    if (e != hipSuccess) return e;
    b->chunks.reserve(n);
    e = hbm_map_to(ptr, b, n, prop);
    if (e != hipSuccess) {                               // never mapped for a kernel: the range may go back
        (void)hipMemAddressFree(ptr, b->reserved_bytes());
        return e;
    }
    *out = ptr;
    return hipSuccess;
}

}  // namespace

extern "C" {

// The caller's current device is left as it was (the HBM calls take a device, not a handle).
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

sda_status sda_hbm_alloc(int device, uint64_t bytes, void** out) {
    SDA_ENTRY;
    if (!out) return fail(SDA_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (bytes == 0) return fail(SDA_ERR_INVALID_ARGUMENT, "bytes must be > 0");
    if (device < 0 || device >= kHbmMaxDev) return fail(SDA_ERR_INVALID_ARGUMENT, "device %d out of range", device);
    DeviceGuard dg;
    HIP_TRY(hipSetDevice(device));
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t gran = 0;
    HIP_TRY(hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum));
    if (gran == 0) gran = 4096;
    const size_t chunk = (hbm_chunk_bytes() + gran - 1) / gran * gran;
    const size_t n = (size_t)((bytes + chunk - 1) / chunk), cls = hbm_class(n);
    // 1. a pooled buffer of this class (the one with the most chunks mapped up to n; fewest past n): taken out
    //    of the pool under the lock, waited for and grown outside it
    uintptr_t key = 0;
    HbmBuffer b;
    bool need_sync = false;
    {
        std::lock_guard<std::mutex> lk(g_hbm_mu);
        auto best = g_hbm_pool.end();
        auto rank = [&](const HbmBuffer& c) { return c.chunks.size() >= n ? c.chunks.size() - n : 4 * (n - c.chunks.size()); };
        for (auto it = g_hbm_pool.begin(); it != g_hbm_pool.end(); ++it) {
            const HbmBuffer& c = it->second;
            if (c.device == device && c.chunk == chunk && c.cls == cls &&
                (best == g_hbm_pool.end() || rank(c) < rank(best->second)))
                best = it;
        }
        if (best != g_hbm_pool.end()) {
            key = best->first;
            b = std::move(best->second);
            g_hbm_pool.erase(best);
            need_sync = !hbm_idle(b);
        }
    }
    if (key) {
        hipError_t e = need_sync ? hbm_sync(device) : hipSuccess;
        if (e == hipSuccess && b.chunks.size() < n) {
            e = hbm_map_to(reinterpret_cast<void*>(key), &b, n, prop);
            if (e == hipErrorOutOfMemory) {              // give the rest of the pool back, then retry once
                (void)hipGetLastError();
                (void)hbm_trim(device, 0);
                e = hbm_map_to(reinterpret_cast<void*>(key), &b, n, prop);
            }
        }
        std::lock_guard<std::mutex> lk(g_hbm_mu);
        if (e != hipSuccess) {                           // back to the pool as it was
            g_hbm_pool[key] = std::move(b);
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? SDA_ERR_OUT_OF_MEMORY : SDA_ERR_DEVICE,
                        "sda_hbm_alloc(%llu bytes): growing a pooled buffer: %s", (unsigned long long)bytes,
                        hipGetErrorString(e));
        }
        g_hbm[key] = std::move(b);
        *out = reinterpret_cast<void*>(key);
        return ok();
    }
    // 2. a new buffer: the pool first goes down to its bound
    HIP_TRY(hbm_trim(device, hbm_pool_cap()));
    void* ptr = nullptr;
    hipError_t e = hbm_create(device, n, chunk, prop, &ptr, &b);
    if (e == hipErrorOutOfMemory) {                      // give the pool back, then retry once
        bool any;
        {
            std::lock_guard<std::mutex> lk(g_hbm_mu);
            any = hbm_pooled_bytes(device) > 0;
        }
        if (any) {
            (void)hipGetLastError();
            HIP_TRY(hbm_trim(device, 0));
            b = HbmBuffer();
            e = hbm_create(device, n, chunk, prop, &ptr, &b);
        }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? SDA_ERR_OUT_OF_MEMORY : SDA_ERR_DEVICE,
                    "sda_hbm_alloc(%llu bytes in %zu MiB chunks): %s", (unsigned long long)bytes, chunk >> 20,
                    hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lk(g_hbm_mu);
    g_hbm[reinterpret_cast<uintptr_t>(ptr)] = std::move(b);
    *out = ptr;
    return ok();
}

sda_status sda_hbm_free(void* ptr) {
    SDA_ENTRY;
    if (!ptr) return ok();
    HbmBuffer b;
    {
        std::lock_guard<std::mutex> lk(g_hbm_mu);
        auto it = g_hbm.find(reinterpret_cast<uintptr_t>(ptr));
        if (it == g_hbm.end())
            return fail(SDA_ERR_INVALID_ARGUMENT, "%p was not returned by sda_hbm_alloc (or freed twice)", ptr);
        if (hbm_pool_cap() != 0) {                       // pooled: no wait
            it->second.freed_ticket = g_hbm_sync_begun[it->second.device];
            it->second.freed_seq = ++g_hbm_seq;
            g_hbm_pool[it->first] = std::move(it->second);
            g_hbm.erase(it);
            return ok();
        }
        b = std::move(it->second);
        g_hbm.erase(it);
    }
    // no pool (SDA_HBM_POOL_MB=0): release at once, after the device is idle
    DeviceGuard dg;
    HIP_TRY(hipSetDevice(b.device));
    HIP_TRY(hbm_sync(b.device));
    hbm_release(ptr, b);
    return ok();
}

sda_status sda_hbm_trim(int device, uint64_t keep_bytes) {
    SDA_ENTRY;
    if (device < 0 || device >= kHbmMaxDev) return fail(SDA_ERR_INVALID_ARGUMENT, "device %d out of range", device);
    DeviceGuard dg;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hbm_trim(device, keep_bytes));
    return ok();
}

sda_status sda_hbm_stats(int device, uint64_t* live_bytes, uint64_t* pooled_bytes, uint64_t* retired_bytes) {
    SDA_ENTRY;
    if (device < 0 || device >= kHbmMaxDev) return fail(SDA_ERR_INVALID_ARGUMENT, "device %d out of range", device);
    std::lock_guard<std::mutex> lk(g_hbm_mu);
    uint64_t live = 0;
    for (auto& kv : g_hbm)
        if (kv.second.device == device) live += kv.second.mapped_bytes();
    if (live_bytes) *live_bytes = live;
    if (pooled_bytes) *pooled_bytes = hbm_pooled_bytes(device);
    if (retired_bytes) *retired_bytes = g_hbm_retired[device];
    return ok();
}

}  // extern "C"

// ---------------- share payload codec (sodium.rs:36-41 / :82-88) ----------------
namespace {

// Plan + count N device-resident blobs; counts[n] on the host.
sda_status codec_count(sda_engine* h, const uint8_t* bytes, const uint64_t* blob_off, uint64_t n_blobs,
                       sda::VarintPlan* plan, uint64_t* counts, bool* irregular, hipStream_t st,
                       bool sub_counts = false, bool* long_any = nullptr) {
    if (((uintptr_t)bytes & 15) != 0) return fail(SDA_ERR_INVALID_ARGUMENT, "byte buffer must be 16-byte aligned");
    for (uint64_t b = 0; b < n_blobs; ++b)
        if (blob_off[b + 1] < blob_off[b]) return fail(SDA_ERR_INVALID_ARGUMENT, "blob offsets must be non-decreasing");
    sda::varint_plan(blob_off, n_blobs, plan);
    if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes,
                              sda::varint_decode_work_bytes(plan->regions, n_blobs)))
        return e;
    HIP_TRY(sda::launch_varint_count(bytes, blob_off, n_blobs, *plan, h->codec_work, counts, irregular, st,
                                     sub_counts, long_any));
    return SDA_OK;
}

// decode + combiner.rs:16-28 over device-resident blobs; out (device) gets out_len = count of blob 0
sda_status decode_combine(sda_engine* h, int64_t m, const uint8_t* bytes, const uint64_t* blob_off, uint64_t n_blobs,
                          int64_t* out, uint64_t out_cap, uint64_t* out_len, hipStream_t st) {
    *out_len = 0;
    // sda_codec_last_launch: NONE until this call returns SDA_OK; `info` collects each decision where it is taken
    h->codec_last = sda::CodecLaunchInfo();
    sda::CodecLaunchInfo info;
    if (n_blobs == 0) return ok();                                  // combiner.rs:17: empty input
    // SDA_CODEC_PATH=fused (A/B and test knob) runs the column-tile decode+combine, which reads the payload
    // once instead of writing and re-reading an int32 matrix but measured slower (VALU-bound: 3.4 ms per
    // 1000 x 1M launch vs 2.2 + 0.7 ms, profiles/r02d/ab_codec_fused.txt); the default is the matrix path.
    const char* path = getenv("SDA_CODEC_PATH");
    const bool force_fused = path && strcmp(path, "fused") == 0, force_matrix = !force_fused;
    const char* env = getenv("SDA_CODEC_NARROW");                    // "0": A/B and test knob
    const bool narrow_ok = !(env && atoi(env) == 0);
    sda::VarintPlan plan;
    std::vector<uint64_t> counts(n_blobs);
    // Default: decode once into int32 slots per 16 KiB region (no count pass), then the exact combine
    // over the slots.  SDA_CODEC_PATH=matrix (A/B and test knob) takes the count pass + dense int32
    // matrix path; any element longer than 5 bytes or outside int32 (malformed or raw i64 payloads)
    // falls back to it as well.
    if (narrow_ok && !force_fused && !(path && strcmp(path, "matrix") == 0)) {
        if (((uintptr_t)bytes & 15) != 0) return fail(SDA_ERR_INVALID_ARGUMENT, "byte buffer must be 16-byte aligned");
        for (uint64_t b = 0; b < n_blobs; ++b)
            if (blob_off[b + 1] < blob_off[b]) return fail(SDA_ERR_INVALID_ARGUMENT, "blob offsets must be non-decreasing");
        sda::varint_plan(blob_off, n_blobs, &plan);
        if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes,
                                  sda::varint_decode_work_bytes(plan.regions, n_blobs)))
            return e;
        // the slots are sized by the bytes, the tile plan by the dimension (<= the bytes of blob 0)
        const uint64_t dim_max = blob_off[1] - blob_off[0];
        if (sda_status e = ensure(&h->codec_mat, &h->codec_mat_bytes, sda::varint_slot_bytes(plan, n_blobs, dim_max)))
            return e;
        // everything is queued before the host sees a count: the combine itself exits when a flag is set
        // or blob 0's count exceeds out_cap, and the checks below then report it in the reference's order
        const bool m_ok = m != 0 && m != INT64_MIN;
        uint32_t flags = 0;
        HIP_TRY(sda::launch_varint_decode_slots_combine(bytes, blob_off, n_blobs, plan, h->codec_work, h->codec_mat,
                                                        out, out_cap, m_ok ? (m < 0 ? -m : m) : 0, counts.data(),
                                                        &flags, st, &info));
        if (!(flags & 1u)) {
            const uint64_t dim = counts[0];
            int64_t mm = 1;
            if (dim && m == 0) return modulus_abs(m, &mm);     // blob 0 is folded first (combiner.rs:20-25)
            for (uint64_t i = 1; i < n_blobs; ++i)
                if (counts[i] != dim)
                    return fail(SDA_ERR_WRONG_DIMENSION,
                                "Wrong dimension (participation %llu decodes to %llu shares, expected %llu)",
                                (unsigned long long)i, (unsigned long long)counts[i], (unsigned long long)dim);
            if (dim) {
                if (sda_status e = modulus_abs(m, &mm)) return e;
            }
            if (out_cap < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
            *out_len = dim;
            h->codec_last = info;
            return SDA_OK;
        }
        info = sda::CodecLaunchInfo();                 // the slot attempt wrote nothing: the count pass takes over
        info.fell_back = sda::kCodecSlotWide;
    }
    bool irregular = false, long_elems = false;
    if (sda_status e = codec_count(h, bytes, blob_off, n_blobs, &plan, counts.data(), &irregular, st, !force_matrix,
                                   &long_elems))
        return e;
    const uint64_t dim = counts[0];
    int64_t mm;
    if (dim && m == 0) return modulus_abs(m, &mm);             // blob 0 is folded first (combiner.rs:20-25)
    for (uint64_t i = 1; i < n_blobs; ++i)
        if (counts[i] != dim)
            return fail(SDA_ERR_WRONG_DIMENSION, "Wrong dimension (participation %llu decodes to %llu shares, expected %llu)",
                        (unsigned long long)i, (unsigned long long)counts[i], (unsigned long long)dim);
    if (dim) {
        if (sda_status e = modulus_abs(m, &mm)) return e;
    }
    if (out_cap < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    *out_len = dim;
    if (dim == 0) return ok();
    if (force_fused && irregular) info.fell_back |= sda::kCodecFusedIrregular;
    if (!irregular && force_fused) {
        // one pass over the payload: no [N][dim] matrix (the matrix buffer holds the tile plan)
        if (sda_status e = ensure(&h->codec_mat, &h->codec_mat_bytes, sda::varint_tile_plan_bytes(n_blobs, dim)))
            return e;
        HIP_TRY(sda::launch_varint_decode_combine(bytes, n_blobs, plan, h->codec_work,
                                                  static_cast<uint64_t*>(h->codec_mat), dim, out, mm, long_elems, st,
                                                  &info));
        h->codec_last = info;
        return SDA_OK;
    }
    if (sda_status e = ensure(&h->codec_mat, &h->codec_mat_bytes, n_blobs * dim * 8)) return e;
    // Decoded field shares fit in int32 (|share| < m <= 2^31 for every field the reference uses): the
    // [N][dim] matrix between the decode and the combine is stored narrowed, which halves its write and
    // its read.  Any value that does not fit (or a malformed blob) takes the int64 matrix instead.
    if (narrow_ok && !irregular) {
        bool wide = false;
        int32_t* mat32 = static_cast<int32_t*>(h->codec_mat);
        HIP_TRY(sda::launch_varint_decode_narrow(bytes, n_blobs, plan, h->codec_work, mat32, dim, &wide, st,
                                                 &info));
        if (!wide) {
            HIP_TRY(sda::launch_combine_exact32(mat32, n_blobs, dim, dim, out, mm, st, false, &h->combine_last));
            info.path = sda::kCodecMatrix32;
            h->codec_last = info;
            return SDA_OK;
        }
        info.fell_back |= sda::kCodecNarrowWide;
    }
    int64_t* mat = static_cast<int64_t*>(h->codec_mat);
    HIP_TRY(sda::launch_varint_decode(bytes, n_blobs, plan, h->codec_work, mat, dim, dim, irregular, st, &info));
    HIP_TRY(sda::launch_combine_exact(mat, n_blobs, dim, dim, out, mm, st, false, &h->combine_last));
    info.path = sda::kCodecMatrix64;
    h->codec_last = info;
    return SDA_OK;
}

// concatenate host blobs into a 16-byte aligned, padded device buffer
sda_status upload_blobs(sda_engine* h, const uint8_t* const* blobs, const uint64_t* lens, uint64_t n,
                        DevArena* a, uint8_t** dev, std::vector<uint64_t>* off) {
    off->assign(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        if (lens[i] && !blobs[i]) return fail(SDA_ERR_INVALID_ARGUMENT, "blob %llu is NULL", (unsigned long long)i);
        (*off)[i + 1] = (*off)[i] + lens[i];
    }
    const uint64_t total = (*off)[n];
    std::vector<uint8_t> host(total + 32, 0);
    for (uint64_t i = 0; i < n; ++i)
        if (lens[i]) memcpy(host.data() + (*off)[i], blobs[i], lens[i]);
    *dev = a->take<uint8_t>(total + 32);
    HIP_TRY(hipMemcpyAsync(*dev, host.data(), total + 32, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));       // `host` goes out of scope
    return SDA_OK;
}

}  // namespace

extern "C" {

sda_status sda_varint_encode(sda_engine* h, const int64_t* vals, uint64_t n, uint8_t* out, uint64_t out_cap,
                             uint64_t* out_len) {
    SDA_ENTRY;
    if (!h || !out_len || (n && !vals)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_len = 0;
    if (n == 0) return ok();
    HIP_TRY(hipSetDevice(h->device));
    DevArena a;
    if (sda_status st = stage(h, rup(n * 8) + rup(n * 10 + 16), &a)) return st;
    int64_t* dv = a.take<int64_t>(n);
    uint8_t* db = a.take<uint8_t>(n * 10 + 16);
    HIP_TRY(hipMemcpyAsync(dv, vals, n * 8, hipMemcpyHostToDevice, h->stream));
    if (sda_status st = ensure(&h->codec_work, &h->codec_work_bytes, sda::varint_encode_work_bytes(1, n))) return st;
    uint64_t bytes = 0;
    HIP_TRY(sda::launch_varint_encode(dv, 1, n, n, db, n * 10 + 16, h->codec_work, &bytes, h->stream));
    if (bytes > out_cap) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small (%llu bytes needed)",
                                     (unsigned long long)bytes);
    HIP_TRY(hipMemcpyAsync(out, db, bytes, hipMemcpyDeviceToHost, h->stream));
    *out_len = bytes;
    return finish(h);
}

sda_status sda_varint_decode(sda_engine* h, const uint8_t* bytes, uint64_t n_bytes, int64_t* out, uint64_t out_cap,
                             uint64_t* out_len) {
    SDA_ENTRY;
    if (!h || !out_len || (n_bytes && !bytes)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_len = 0;
    HIP_TRY(hipSetDevice(h->device));
    DevArena a;
    if (sda_status st = stage(h, rup(n_bytes + 32) + rup(n_bytes * 8 + 8), &a)) return st;
    uint8_t* db;
    std::vector<uint64_t> off;
    const uint8_t* const blobs[1] = {bytes};
    if (sda_status st = upload_blobs(h, blobs, &n_bytes, 1, &a, &db, &off)) return st;
    int64_t* dv = a.take<int64_t>(n_bytes + 1);
    sda::VarintPlan plan;
    uint64_t count = 0;
    bool irregular = false;
    if (sda_status st = codec_count(h, db, off.data(), 1, &plan, &count, &irregular, h->stream)) return st;
    if (count > out_cap) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small (%llu values)",
                                     (unsigned long long)count);
    HIP_TRY(sda::launch_varint_decode(db, 1, plan, h->codec_work, dv, count, count, irregular, h->stream));
    if (count) HIP_TRY(hipMemcpyAsync(out, dv, count * 8, hipMemcpyDeviceToHost, h->stream));
    *out_len = count;
    return finish(h);
}

sda_status sda_clerk_decode_combine(sda_engine* h, const sda_sharing_scheme* s, const uint8_t* const* blobs,
                                    const uint64_t* blob_lens, uint64_t n_blobs, int64_t* out, uint64_t out_cap,
                                    uint64_t* out_len) {
    SDA_ENTRY;
    if (!h || !s || !out_len || (n_blobs && (!blobs || !blob_lens))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_len = 0;
    for (uint64_t i = 0; i < n_blobs; ++i)
        if (blob_lens[i] && !blobs[i]) return fail(SDA_ERR_INVALID_ARGUMENT, "blob %llu is NULL", (unsigned long long)i);
    HIP_TRY(hipSetDevice(h->device));
    (void)pick(h, h->stream);
    // blob groups streamed through pinned double buffers, decoded and combined on device (host path section)
    if (sda_status st = host_decode_combine(h, s->modulus, blobs, blob_lens, n_blobs, out, out_cap, out_len)) return st;
    return ok();
}

sda_status sda_varint_decode_dev(sda_engine* h, const uint8_t* bytes, const uint64_t* blob_off, uint64_t n_blobs,
                                 int64_t* out, uint64_t out_stride, uint64_t* counts, void* stream) {
    SDA_ENTRY;
    if (!h || !blob_off || !counts || (n_blobs && (!bytes || !out))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick(h, stream);
    if (n_blobs == 0) return ok();
    if (((uintptr_t)bytes & 15) != 0) return fail(SDA_ERR_INVALID_ARGUMENT, "byte buffer must be 16-byte aligned");
    for (uint64_t b = 0; b < n_blobs; ++b)
        if (blob_off[b + 1] < blob_off[b]) return fail(SDA_ERR_INVALID_ARGUMENT, "blob offsets must be non-decreasing");
    sda::VarintPlan plan;
    sda::varint_plan(blob_off, n_blobs, &plan);
    if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes, sda::varint_decode_work_bytes(plan.regions, n_blobs)))
        return e;
    // count, check the capacity and decode without a host wait in between: a blob longer than out_stride
    // stops every write on the device and is reported here (nothing written)
    bool too_long = false;
    HIP_TRY(sda::launch_varint_decode_one_wait(bytes, blob_off, n_blobs, plan, h->codec_work, out, out_stride, counts,
                                               &too_long, st));
    if (too_long)
        for (uint64_t i = 0; i < n_blobs; ++i)
            if (counts[i] > out_stride)
                return fail(SDA_ERR_INVALID_ARGUMENT, "blob %llu decodes to %llu values > out_stride",
                            (unsigned long long)i, (unsigned long long)counts[i]);
    return ok();
}

sda_status sda_clerk_decode_combine_dev(sda_engine* h, int64_t modulus, const uint8_t* bytes, const uint64_t* blob_off,
                                        uint64_t n_blobs, int64_t* out, uint64_t out_cap, uint64_t* out_len,
                                        void* stream) {
    SDA_ENTRY;
    if (!h || !blob_off || !out_len || (n_blobs && !bytes)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    if (sda_status e = decode_combine(h, modulus, bytes, blob_off, n_blobs, out, out_cap, out_len, pick(h, stream)))
        return e;
    return ok();
}

sda_status sda_varint_encode_dev(sda_engine* h, const int64_t* vals, uint64_t rows, uint64_t len, uint64_t stride,
                                 uint8_t* dst, uint64_t dst_cap, uint64_t* row_bytes, void* stream) {
    SDA_ENTRY;
    if (!h || !row_bytes || (rows && len && (!vals || !dst))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (rows > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 rows per call");
    if (stride < len) return fail(SDA_ERR_INVALID_ARGUMENT, "stride < len");
    HIP_TRY(hipSetDevice(h->device));
    if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes, sda::varint_encode_work_bytes(rows, len))) return e;
    hipError_t e = sda::launch_varint_encode(vals, rows, len, stride, dst, dst_cap, h->codec_work, row_bytes,
                                             pick(h, stream));
    if (e == hipErrorInvalidValue) return fail(SDA_ERR_INVALID_ARGUMENT, "dst_cap too small");
    HIP_TRY(e);
    return ok();
}

sda_status sda_varint_encode32_dev(sda_engine* h, const int32_t* vals, uint64_t rows, uint64_t len, uint64_t stride,
                                   uint8_t* dst, uint64_t dst_cap, uint64_t* row_bytes, void* stream) {
    SDA_ENTRY;
    if (!h || !row_bytes || (rows && len && (!vals || !dst))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (rows > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 rows per call");
    if (stride < len) return fail(SDA_ERR_INVALID_ARGUMENT, "stride < len");
    HIP_TRY(hipSetDevice(h->device));
    if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes, sda::varint_encode32_work_bytes(rows, len))) return e;
    hipError_t e = sda::launch_varint_encode32(vals, rows, len, stride, dst, dst_cap, h->codec_work, row_bytes,
                                               pick(h, stream));
    if (e == hipErrorInvalidValue) return fail(SDA_ERR_INVALID_ARGUMENT, "dst_cap too small");
    HIP_TRY(e);
    return ok();
}

// ---------------- snapshot transposition (stores.rs:86-101) ----------------
// Offsets are a host-side plan (like the codec's blob_off); the bytes move on the device.
sda_status sda_snapshot_transpose_dev(sda_engine* h, const uint8_t* src, const uint64_t* part_off,
                                      uint64_t n_participations, uint64_t n_clerks, uint8_t* dst, uint64_t dst_cap,
                                      uint64_t* dst_len, uint64_t* clerk_base, uint64_t* clerk_off, void* stream) {
    SDA_ENTRY;
    if (!h || !part_off || !dst_len || (n_clerks && (!clerk_base || !clerk_off)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    const uint64_t P = n_participations, n = n_clerks, nb = P * n;
    if (n && P > ((uint64_t)1 << 32) / n) return fail(SDA_ERR_UNSUPPORTED, "at most 2^32 blobs per snapshot");
    for (uint64_t b = 0; b < nb; ++b)
        if (part_off[b + 1] < part_off[b]) return fail(SDA_ERR_INVALID_ARGUMENT, "blob offsets must be non-decreasing");
    // clerk c's job: its P blobs back to back in snapshot order, the job 16-byte aligned and followed
    // by 16 readable bytes (what sda_clerk_decode_combine_dev takes)
    uint64_t total = 0;
    for (uint64_t c = 0; c < n; ++c) {
        clerk_base[c] = total;
        uint64_t* off = clerk_off + c * (P + 1);
        off[0] = 0;
        for (uint64_t p = 0; p < P; ++p) off[p + 1] = off[p] + (part_off[p * n + c + 1] - part_off[p * n + c]);
        total += ((off[P] + 15) & ~(uint64_t)15) + 16;
    }
    *dst_len = total;
    if (!dst) return ok();                                          // sizing query
    if (dst_cap < total) return fail(SDA_ERR_INVALID_ARGUMENT, "dst_cap %llu < %llu bytes needed",
                                     (unsigned long long)dst_cap, (unsigned long long)total);
    if (nb && !src) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (((uintptr_t)src & 15) || ((uintptr_t)dst & 15))
        return fail(SDA_ERR_INVALID_ARGUMENT, "src and dst must be 16-byte aligned");
    const uint64_t chunk = sda::snapshot_chunk_bytes();
    std::vector<sda::SnapshotCopy> blobs;                          // clerk-major, non-empty blobs only
    std::vector<uint64_t> cstart(1, 0);
    blobs.reserve(nb);
    cstart.reserve(nb + 1);
    for (uint64_t c = 0; c < n; ++c)
        for (uint64_t p = 0; p < P; ++p) {
            const uint64_t len = part_off[p * n + c + 1] - part_off[p * n + c];
            if (!len) continue;
            blobs.push_back({part_off[p * n + c], clerk_base[c] + clerk_off[c * (P + 1) + p], len});
            cstart.push_back(cstart.back() + (len + chunk - 1) / chunk);
        }
    if (blobs.empty()) return ok();
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick(h, stream);
    const size_t b0 = rup(blobs.size() * sizeof(sda::SnapshotCopy));
    if (sda_status e = ensure(&h->snap, &h->snap_bytes, b0 + rup(cstart.size() * 8))) return e;
    char* plan = static_cast<char*>(h->snap);
    HIP_TRY(hipMemcpyAsync(plan, blobs.data(), blobs.size() * sizeof(sda::SnapshotCopy), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(plan + b0, cstart.data(), cstart.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(sda::launch_snapshot_transpose(src, dst, reinterpret_cast<const sda::SnapshotCopy*>(plan),
                                           reinterpret_cast<const uint64_t*>(plan + b0), blobs.size(),
                                           cstart.back(), st));
    HIP_TRY(hipStreamSynchronize(st));                             // the host plan vectors go out of scope
    return ok();
}

}  // extern "C"

// ---------------- fused role pipelines ----------------
namespace {

// receive.rs:80-157 + :14-20 on device-resident inputs (see sda_recipient_reveal_dev).
sda_status recipient_pipeline(sda_engine* h, const sda_masking_scheme* ms, const void* mask_in, uint64_t n_masks,
                              uint64_t mask_width, const sda_sharing_scheme* ss, uint64_t dimension,
                              const uint64_t* indices, const int64_t* shares, uint64_t n_idx, uint64_t share_len,
                              int64_t output_modulus, int32_t mode, int64_t* out, uint64_t out_cap,
                              uint64_t* out_len, hipStream_t st) {
    *out_len = 0;
    // Checks in the reference's order: mask combine (receive.rs:101-117), reconstruct (:120-146),
    // unmask (:149-152).
    // ---- 1. mask combine: its length and panics ----
    uint64_t mask_len = 0;
    if (ms->kind == SDA_MASKING_NONE) {
        if (n_masks && mask_width) return fail(SDA_ERR_PRECONDITION, "assertion failed: masks.iter().all(|mask| mask.len() == 0)");
    } else if (ms->kind == SDA_MASKING_FULL) {
        mask_len = n_masks ? mask_width : 0;                // full.rs:38-40
        if (mask_len) {                                     // full.rs:45 `%= modulus`
            int64_t q0;
            if (sda_status e = modulus_abs(ms->modulus, &q0)) return e;
        }
    } else if (ms->kind == SDA_MASKING_CHACHA) {
        mask_len = ms->dimension;                           // chacha.rs:58
        if (mask_width == 0 || mask_width > 8) return fail(SDA_ERR_UNSUPPORTED, "device seeds must be 1..8 words");
        if (mask_len && n_masks && ms->modulus <= 0)        // chacha.rs:69 gen_range(0, m)
            return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    } else {
        return fail(SDA_ERR_INVALID_ARGUMENT, "unknown masking scheme kind");
    }
    // ---- 2. reconstruct: masked output length and errors ----
    uint64_t D;
    if (ss->kind == SDA_SHARING_ADDITIVE) {
        D = n_idx ? share_len : 0;                           // additive.rs:56-60
        if (D) {                                             // additive.rs:67 `%= modulus`
            int64_t m0;
            if (sda_status e = modulus_abs(ss->modulus, &m0)) return e;
        }
    } else if (ss->kind == SDA_SHARING_PACKED_SHAMIR) {
        if (sda_status e = check_packed(ss)) return e;
        if (mode != SDA_REVEAL_EXACT && mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
        const uint64_t B = (dimension + ss->secret_count - 1) / ss->secret_count;
        if (B) {                                             // batched.rs:77-81: no batch => no check
            const bool enough = n_idx >= ss->privacy_threshold + ss->secret_count;
            if (n_idx && share_len < (enough ? B : 1))      // batched.rs:84 indexes [batch_index]
                return fail(SDA_ERR_PRECONDITION, "index out of bounds: clerk vector shorter than the batch count");
            if (!enough) return fail(SDA_ERR_NOT_ENOUGH_SHARES, "Not enough shares to reconstruct");  // packed_shamir.rs:75
            if (n_idx > sda::kRevealMaxShares)
                return fail(SDA_ERR_UNSUPPORTED, "more than %u clerk shares per batch", sda::kRevealMaxShares);
        }
        D = dimension;
    } else {
        return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    }
    // ---- 3. unmask ----
    if (ms->kind != SDA_MASKING_NONE && mask_len != D)     // chacha.rs:83 / full.rs:58 assert_eq!
        return fail(SDA_ERR_PRECONDITION, "assertion failed: mask.len() == masked_secrets.len() (%llu vs %llu)",
                    (unsigned long long)mask_len, (unsigned long long)D);
    if (out_cap < D) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    if (D == 0) return ok();
    int64_t q = 1;
    if (ms->kind != SDA_MASKING_NONE)
        if (sda_status e = modulus_abs(ms->modulus, &q)) return e;
    const bool packed = ss->kind == SDA_SHARING_PACKED_SHAMIR;
    const uint64_t B = packed ? (dimension + ss->secret_count - 1) / ss->secret_count : 0;
    const bool compact = packed && share_len != B;
    if (sda_status e = ensure(&h->pipe, &h->pipe_bytes, 2 * rup(D * 8) + (compact ? rup(n_idx * B * 8) : 0) + 256))
        return e;
    int64_t* dmask = static_cast<int64_t*>(h->pipe);
    int64_t* dmasked = dmask + rup(D * 8) / 8;
    // 1. masks (receive.rs:101-117)
    if (ms->kind == SDA_MASKING_FULL) {
        if (sda_status e = modulus_abs(ms->modulus, &q)) return e;
        HIP_TRY(sda::launch_combine_exact(static_cast<const int64_t*>(mask_in), n_masks, D, mask_width, dmask, q, st,
                                          false, &h->combine_last));
    }
    PendingChacha pc;                                       // ChaCha: its rejection count is checked at the end
    if (ms->kind == SDA_MASKING_CHACHA) {
        if (sda_status e = chacha_combine_begin(h, ms->modulus, D, static_cast<const uint32_t*>(mask_in),
                                                (uint32_t)mask_width, n_masks, dmask, st, &pc))
            return e;
    }
    // 2. reconstruct (receive.rs:120-146)
    if (!packed) {
        int64_t m;
        if (sda_status e = modulus_abs(ss->modulus, &m)) return e;
        HIP_TRY(sda::launch_combine_exact(shares, n_idx, D, share_len, dmasked, m, st, false, &h->combine_last));
    } else {
        const int64_t* src = shares;
        if (compact) {                                      // batched.rs:83-85 reads [clerk][0..B)
            int64_t* c = dmasked + rup(D * 8) / 8;
            HIP_TRY(hipMemcpy2DAsync(c, B * 8, shares, share_len * 8, B * 8, n_idx, hipMemcpyDeviceToDevice, st));
            src = c;
        }
        if (sda_status e = ensure(&h->gen_log, &h->gen_log_bytes, sda::packed_gen_log_bytes())) return e;
        sda::PackedRevealArgs ra{src, dimension, 1, dmasked};
        // The output is positive(unmask(reveal)).  When the masking modulus (or no mask) and output_modulus are
        // both the sharing prime, that is the canonical residue of (reveal - mask) mod p, which depends only on
        // the reveal's residue: tss' signed representatives (EXACT, 2.1x the canonical reveal's time) cannot
        // change a byte of it, so the canonical reveal runs.  Duplicate clerk points (no Lagrange form) fall
        // back to EXACT.  SDA_RECIPIENT_EXACT=1 keeps EXACT (A/B and test knob).
        const int64_t p = ss->modulus;
        const char* keep = getenv("SDA_RECIPIENT_EXACT");
        const bool residue_only = output_modulus == p && (ms->kind == SDA_MASKING_NONE || q == p) &&
                                  !(keep && atoi(keep) == 1);
        const int32_t run_mode = (mode == SDA_REVEAL_EXACT && residue_only) ? SDA_REVEAL_CANONICAL : mode;
        hipError_t e = sda::launch_packed_reveal(ra, indices, (uint32_t)n_idx, (uint32_t)ss->secret_count,
                                                 (uint32_t)ss->privacy_threshold,
                                                 (uint32_t)p, (uint32_t)ss->omega_secrets,
                                                 (uint32_t)ss->omega_shares, run_mode, h->rev_tab, h->gen_log, st,
                                                 &h->gen_log_used);
        if (e == hipErrorInvalidValue && run_mode != mode)
            e = sda::launch_packed_reveal(ra, indices, (uint32_t)n_idx, (uint32_t)ss->secret_count,
                                          (uint32_t)ss->privacy_threshold, (uint32_t)p,
                                          (uint32_t)ss->omega_secrets, (uint32_t)ss->omega_shares, mode, h->rev_tab,
                                          h->gen_log, st, &h->gen_log_used);
        if (e == hipErrorInvalidValue && mode == SDA_REVEAL_CANONICAL)
            return fail(SDA_ERR_UNSUPPORTED, "canonical reveal needs distinct clerk indices");
        HIP_TRY(e);
    }
    // 3. unmask (receive.rs:149-152) + RecipientOutput::positive (:14-20), one pass
    HIP_TRY(sda::launch_unmask_positive(dmasked, ms->kind == SDA_MASKING_NONE ? nullptr : dmask, D, q,
                                        output_modulus, out, st));
    if (pc.pending) {            // the mask's rejection count: fix the mask and unmask again if it had any
        HIP_TRY(hipStreamSynchronize(st));
        bool changed = false;
        if (sda_status e = chacha_combine_end(h, pc, st, &changed)) return e;
        if (changed)
            HIP_TRY(sda::launch_unmask_positive(dmasked, dmask, D, q, output_modulus, out, st));
    }
    *out_len = D;
    return SDA_OK;
}

}  // namespace

extern "C" {

sda_status sda_recipient_reveal_dev(sda_engine* h, const sda_masking_scheme* ms, const void* mask_in, uint64_t n_masks,
                                    uint64_t mask_width, const sda_sharing_scheme* ss, uint64_t dimension,
                                    const uint64_t* indices, const int64_t* shares, uint64_t n_idx,
                                    uint64_t share_len, int64_t output_modulus, int32_t mode, int64_t* out,
                                    uint64_t out_cap, uint64_t* out_len, void* stream) {
    SDA_ENTRY;
    if (!h || !ms || !ss || !out_len || (n_idx && (!shares || !indices)) || (n_masks && mask_width && !mask_in))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    if (sda_status e = recipient_pipeline(h, ms, mask_in, n_masks, mask_width, ss, dimension, indices, shares, n_idx,
                                          share_len, output_modulus, mode, out, out_cap, out_len, pick(h, stream)))
        return e;
    return ok();
}

sda_status sda_recipient_reveal(sda_engine* h, const sda_masking_scheme* ms, const int64_t* const* mask_rows,
                                const uint64_t* mask_lens, uint64_t n_masks, const sda_sharing_scheme* ss,
                                uint64_t dimension, const uint64_t* indices, const int64_t* const* share_rows,
                                const uint64_t* share_lens, uint64_t n_idx, int64_t output_modulus, int32_t mode,
                                int64_t* out, uint64_t out_cap, uint64_t* out_len) {
    SDA_ENTRY;
    if (!h || !ms || !ss || !out_len || (n_masks && (!mask_rows || !mask_lens)) ||
        (n_idx && (!share_rows || !share_lens || !indices)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_len = 0;
    HIP_TRY(hipSetDevice(h->device));
    // host-side shape checks in the reference's order, then one upload
    uint64_t share_len = n_idx ? share_lens[0] : 0;
    for (uint64_t i = 0; i < n_idx; ++i) {
        if (share_lens[i] == share_len) continue;
        if (ss->kind == SDA_SHARING_ADDITIVE) return fail(SDA_ERR_MISMATCHING_DIMENSION, "Mismatching dimension");
        share_len = share_lens[i] < share_len ? share_lens[i] : share_len;   // packed: reads [0, B) of each
    }
    uint64_t width = 0;
    std::vector<uint32_t> seeds;
    if (ms->kind == SDA_MASKING_FULL) {
        width = n_masks ? mask_lens[0] : 0;
        for (uint64_t i = 0; i < n_masks; ++i)
            if (mask_lens[i] != width) return fail(SDA_ERR_PRECONDITION, "assertion failed: mask.len() == dimension");
    } else if (ms->kind == SDA_MASKING_CHACHA) {
        for (uint64_t i = 0; i < n_masks; ++i) width = mask_lens[i] > width ? mask_lens[i] : width;
        width = width > 8 ? 8 : (width == 0 ? 1 : width);    // key = first 8 words, zero padded
        seeds.assign(n_masks * width, 0u);
        for (uint64_t i = 0; i < n_masks; ++i)
            for (uint64_t j = 0; j < mask_lens[i] && j < width; ++j) seeds[i * width + j] = (uint32_t)mask_rows[i][j];
    } else {
        for (uint64_t i = 0; i < n_masks; ++i)
            if (mask_lens[i]) return fail(SDA_ERR_PRECONDITION, "assertion failed: masks.iter().all(|mask| mask.len() == 0)");
    }
    const uint64_t outn = ss->kind == SDA_SHARING_ADDITIVE ? share_len : dimension;
    // A multi-device handle spreads the mask combine (receive.rs:113-116, the dominant cost at configs[4]) over its
    // devices -- seeds split, one RCCL reduce onto device 0 (host path section) -- and runs the rest of the
    // pipeline on device 0 with the combined mask as one Full mask row: (0 + c) % m = c for the canonical c, so
    // the unmask sees the same mask.  Only where the reference would not panic in the mask combine (m > 0).
    const sda_masking_scheme full_row = {SDA_MASKING_FULL, ms->modulus, 0, 0};
    const bool multi_mask = ms->kind == SDA_MASKING_CHACHA && !h->sub.empty() && n_masks && ms->dimension &&
                            ms->modulus > 0;
    if (multi_mask) {
        if (sda_status e = host_stream_ensure(h, 0, ms->dimension * 8)) return e;
        if (sda_status e = chacha_combine_multi(h, ms->modulus, ms->dimension, seeds, (uint32_t)width, n_masks,
                                                static_cast<int64_t*>(h->hs_dev)))
            return e;
    }
    DevArena a;
    if (sda_status e = stage(h, rup(n_idx * share_len * 8 + 8) + rup(n_masks * width * 8 + 8) + rup(outn * 8 + 8), &a))
        return e;
    int64_t* dsh = a.take<int64_t>(n_idx * share_len + 1);
    void* dmask = a.take<int64_t>(n_masks * width + 1);
    int64_t* dout = a.take<int64_t>(outn + 1);
    for (uint64_t i = 0; i < n_idx; ++i)
        if (share_len) HIP_TRY(hipMemcpyAsync(dsh + i * share_len, share_rows[i], share_len * 8, hipMemcpyHostToDevice, h->stream));
    if (ms->kind == SDA_MASKING_FULL)
        for (uint64_t i = 0; i < n_masks; ++i)
            if (width) HIP_TRY(hipMemcpyAsync(static_cast<int64_t*>(dmask) + i * width, mask_rows[i], width * 8,
                                              hipMemcpyHostToDevice, h->stream));
    if (ms->kind == SDA_MASKING_CHACHA && !seeds.empty() && !multi_mask)
        HIP_TRY(hipMemcpyAsync(dmask, seeds.data(), seeds.size() * 4, hipMemcpyHostToDevice, h->stream));
    uint64_t len = 0;
    if (sda_status e = multi_mask
                           ? recipient_pipeline(h, &full_row, h->hs_dev, 1, ms->dimension, ss, dimension, indices, dsh,
                                                n_idx, share_len, output_modulus, mode, dout, (uint64_t)-1, &len, h->stream)
                           : recipient_pipeline(h, ms, dmask, n_masks, ms->kind == SDA_MASKING_NONE ? 0 : width, ss,
                                                dimension, indices, dsh, n_idx, share_len, output_modulus, mode, dout,
                                                (uint64_t)-1, &len, h->stream))
        return e;
    if (out_cap < len) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    if (len) HIP_TRY(hipMemcpyAsync(out, dout, len * 8, hipMemcpyDeviceToHost, h->stream));
    *out_len = len;
    return finish(h);
}

// The participant pipeline behind sda_participant_share_dev and sda_participant_share32_dev.  One of shares64 /
// shares32 is the [n][B] output (shares32: int32 rows, PackedShamir only, encoded by the int32 encoder).
static sda_status participant_share(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                    uint64_t seed_words, const int64_t* full_masks, const sda_sharing_scheme* ss,
                                    const int64_t* secrets, uint64_t dimension, const int64_t* draws, int32_t mode,
                                    int64_t* shares64, int32_t* shares32, uint8_t* payload, uint64_t payload_cap,
                                    uint64_t* payload_row_bytes, void* stream) {
    if (!h || !ms || !ss || (dimension && (!secrets || (!shares64 && !shares32))) || (payload && !payload_row_bytes))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick(h, stream);
    const uint64_t D = dimension;
    const bool packed = ss->kind == SDA_SHARING_PACKED_SHAMIR;
    if (!packed && ss->kind != SDA_SHARING_ADDITIVE) return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    if (!packed && shares32)
        return fail(SDA_ERR_UNSUPPORTED, "int32 shares need a PackedShamir scheme: an additive scheme's first n - 1 "
                                         "shares are the caller's draws, copied unchecked");
    if (mode != SDA_REVEAL_EXACT && mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
    if (packed) {
        if (sda_status e = check_packed(ss)) return e;
    } else {
        if (ss->share_count == 0) return fail(SDA_ERR_PRECONDITION, "share_count - 1 underflows (additive.rs:42)");
        if (ss->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    }
    // 1. SecretMasker::mask (participate.rs:53-54)
    const int64_t* masked = secrets;
    // ChaCha on the fast path: the masked secrets come straight out of the ChaCha kernel and its rejection
    // count is checked at the end of the call (a nonzero count -- probability < 2^-28 per draw -- redoes
    // the mask exactly, then every later step)
    bool mask_pending = false;
    int64_t* cmask = nullptr;
    uint32_t* cseed = nullptr;
    uint32_t cw = 0;
    if (ms->kind != SDA_MASKING_NONE && D) {
        if (ms->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
        if (sda_status e = ensure(&h->pipe, &h->pipe_bytes, 2 * rup(D * 8) + 256)) return e;
        int64_t* dm = static_cast<int64_t*>(h->pipe);
        if (ms->kind == SDA_MASKING_FULL) {
            if (!full_masks) return fail(SDA_ERR_INVALID_ARGUMENT, "Full masking needs the drawn masks");
            HIP_TRY(sda::launch_addsub_trem(secrets, full_masks, +1, D, dm, ms->modulus, st));      // full.rs:28-31
        } else if (ms->kind == SDA_MASKING_CHACHA) {
            if (ms->dimension != D) return fail(SDA_ERR_PRECONDITION, "assertion failed: dimension == secrets.len()");
            const uint64_t want = (ms->seed_bitsize + 31) / 32;
            if (seed_words != want || (seed_words && !seed))
                return fail(SDA_ERR_PRECONDITION, "expected %llu seed words", (unsigned long long)want);
            int64_t* dmask = dm + rup(D * 8) / 8;
            uint32_t* dseed = reinterpret_cast<uint32_t*>(dmask + rup(D * 8) / 8);
            const uint32_t w = (uint32_t)(seed_words < 8 ? seed_words : 8);
            if (w) HIP_TRY(hipMemcpyAsync(dseed, seed, w * 4, hipMemcpyHostToDevice, st));
            // chacha.rs:36-45: masked = (secrets + draw) % m over one stream
            const char* force = getenv("SDA_CHACHA_PATH");
            if (!sda::chacha_needs_stream_path(ms->modulus) && !(force && strcmp(force, "stream") == 0)) {
                if (sda_status e = ensure(&h->work, &h->work_bytes, sda::chacha_work_bytes(D, 0))) return e;
                sda::ChachaLaunchInfo info;
                HIP_TRY(sda::launch_chacha_mask_add_async(ms->modulus, D, dseed, w, secrets, dm, h->work, st,
                                                          h->rej_host, &info));
                record_chacha(h, info);
                mask_pending = true;
            } else {
                if (sda_status e = chacha_combine(h, ms->modulus, D, dseed, w, 1, dmask, st)) return e;
                HIP_TRY(sda::launch_addsub_trem(secrets, dmask, +1, D, dm, ms->modulus, st));
            }
            cmask = dmask;
            cseed = dseed;
            cw = w;
        } else {
            return fail(SDA_ERR_INVALID_ARGUMENT, "unknown masking scheme kind");
        }
        masked = dm;
    }
    // 2. ShareGenerator::generate (participate.rs:75-76): shares [n][B]
    const uint64_t n = ss->share_count;
    const uint64_t B = packed ? (D + ss->secret_count - 1) / ss->secret_count : D;
    if (B && !draws) return fail(SDA_ERR_INVALID_ARGUMENT, "need the randomness draws");
    if (payload && n > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 clerks");
    auto share_and_encode = [&]() -> sda_status {
        if (B) {
            if (packed) {
                if (sda_status e = ensure(&h->gen_log, &h->gen_log_bytes, sda::packed_gen_log_bytes())) return e;
                sda::PackedGenArgs ga{masked, D, 1, draws, shares64, mode == SDA_REVEAL_CANONICAL};
                const uint32_t k = (uint32_t)ss->secret_count, t = (uint32_t)ss->privacy_threshold;
                if (shares32) {                  // as sda_packed_generate32_dev: scratch + narrowing at n + 1 = 81
                    ga.out32 = shares32;
                    if (const size_t tmp = sda::packed_gen32_scratch_bytes(ga, k, t, (uint32_t)n, (uint32_t)ss->modulus)) {
                        if (sda_status e = ensure(&h->gen32_tmp, &h->gen32_tmp_bytes, tmp + 64)) return e;
                        ga.scratch = static_cast<int64_t*>(h->gen32_tmp);
                        ga.flag = ga.scratch + tmp / sizeof(int64_t);
                    }
                }
                HIP_TRY(sda::launch_packed_generate(ga, k, t, (uint32_t)n, (uint32_t)ss->modulus,
                                                    (uint32_t)ss->omega_secrets, (uint32_t)ss->omega_shares,
                                                    h->gen_tab, h->gen_log, st, &h->gen_log_used));
            } else {
                HIP_TRY(sda::launch_additive_generate(masked, D, draws, n, shares64, ss->modulus, st));
            }
        }
        // 3. per-clerk payload encoding (participate.rs:79-98 -> sodium.rs:36-41); sealing stays on the host
        if (payload) {
            if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes,
                                      shares32 ? sda::varint_encode32_work_bytes(n, B)
                                               : sda::varint_encode_work_bytes(n, B)))
                return e;
            hipError_t e = shares32 ? sda::launch_varint_encode32(shares32, n, B, B, payload, payload_cap,
                                                                  h->codec_work, payload_row_bytes, st)
                                    : sda::launch_varint_encode(shares64, n, B, B, payload, payload_cap,
                                                                h->codec_work, payload_row_bytes, st);
            if (e == hipErrorInvalidValue) return fail(SDA_ERR_INVALID_ARGUMENT, "payload_cap too small");
            HIP_TRY(e);
        }
        return SDA_OK;
    };
    if (sda_status e = share_and_encode()) return e;
    if (mask_pending) {          // the mask's rejection count: redo the mask exactly, and every later step
        HIP_TRY(hipStreamSynchronize(st));
        if (*h->rej_host) {
            if (sda_status e = chacha_combine(h, ms->modulus, D, cseed, cw, 1, cmask, st)) return e;
            // the record stays the mask add's, with the redo's fix-up count (or its log overflow)
            if (h->chacha_last.path != sda::kChachaOverflow) {
                h->chacha_last.path = sda::kChachaMaskAdd;
                h->chacha_last.grid_y = 1;
            }
            HIP_TRY(sda::launch_addsub_trem(secrets, cmask, +1, D, const_cast<int64_t*>(masked), ms->modulus, st));
            if (sda_status e = share_and_encode()) return e;
        }
    }
    return ok();
}

// participate.rs:53-76 (+ the encoding step of Encryptor::encrypt, sodium.rs:36-41) on device.
sda_status sda_participant_share_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                     uint64_t seed_words, const int64_t* full_masks, const sda_sharing_scheme* ss,
                                     const int64_t* secrets, uint64_t dimension, const int64_t* draws,
                                     int32_t mode, int64_t* shares_out, uint8_t* payload, uint64_t payload_cap,
                                     uint64_t* payload_row_bytes, void* stream) {
    SDA_ENTRY;
    return participant_share(h, ms, seed, seed_words, full_masks, ss, secrets, dimension, draws, mode, shares_out,
                             nullptr, payload, payload_cap, payload_row_bytes, stream);
}

// The same with the shares as int32 rows, from sda_packed_generate32_dev's kernels into the int32 encoder.
sda_status sda_participant_share32_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                       uint64_t seed_words, const int64_t* full_masks, const sda_sharing_scheme* ss,
                                       const int64_t* secrets, uint64_t dimension, const int64_t* draws, int32_t mode,
                                       int32_t* shares_out, uint8_t* payload, uint64_t payload_cap,
                                       uint64_t* payload_row_bytes, void* stream) {
    SDA_ENTRY;
    return participant_share(h, ms, seed, seed_words, full_masks, ss, secrets, dimension, draws, mode, nullptr,
                             shares_out, payload, payload_cap, payload_row_bytes, stream);
}

}  // extern "C"

// ---------------- streaming, multi-device host path ----------------
// The host entry points take the reference's host buffers (a Vec<Vec<i64>> of rows, clerk.rs:79-86) and
// return when the result is in host memory.  A clerk job may be larger than HBM, so rows never sit in one
// device buffer: each device streams them in row tiles through two pinned host buffers and two device tiles
// (host_stage_bytes() each).  Tile i is packed on the host (host threads copying the rows' column slice into
// pinned memory) while tile i - 1 uploads on the copy stream and tile i - 2's combine runs on the compute
// stream; the combine continues the recurrence across tiles (launch_combine_exact, accumulate), so the
// result is bit-identical to one pass over all rows.
//
// Half-width tiles (SDA_HOST_NARROW, host_narrow()): a tile is first packed as int32 (pack_rows32); when every
// value fits -- |v| < m <= 2^31 in every shipped configuration -- it ships and combines as int32 rows
// (launch_combine_wide32, accumulate) in half of its buffers: half the bytes over PCIe.  A tile with a value
// that does not fit is repacked as i64, and the rest of that column chunk's tiles ship as i64 without trying,
// so raw i64 rows cost at most one wasted pack per chunk.  sda_host_stream_stats counts both kinds.
//
// A handle over G devices (sda_engine_create_multi) splits the host calls:
//   - combine (ShareCombiner, Full MaskCombiner, Additive reconstruct): by COLUMNS.  Device g walks every
//     row, in order, over its column slice and writes that slice of the result: exact for signed inputs in
//     one pass with no exchange.  A participation split would have to stream a signed
//     job's rows over PCIe twice (DESIGN.md §5's two-pass split), and the rows come from the host anyway.
//   - ChaCha MaskCombiner: by SEEDS (the expansion is compute-bound, the rows are a few words).  Each device
//     sums its seeds' canonical draws; one RCCL ncclReduce(SUM, int64) over xGMI onto device 0 and the
//     device finalize give the reference's result (every draw is >= 0; headroom G (m - 1) <= 2^63 - 1 is
//     checked).  Moduli above 2^62 (the reference's own sum wraps there) and handles whose ordinals repeat
//     run on device 0 alone.
//   - packed share generate / reconstruct: by BATCHES; additive share generate: by columns.
namespace {

long long env_ll(const char* name, long long dflt) {
    const char* e = getenv(name);
    return e && *e ? atoll(e) : dflt;
}

// host threads for packing rows into pinned memory, over all the handle's devices (SDA_HOST_THREADS; default:
// the CPUs, at most 16 per device)
int host_threads(size_t devices = 1) {
    const long long t = env_ll("SDA_HOST_THREADS", 0);
    if (t > 0) return (int)std::min<long long>(t, 1024);
    const unsigned hc = std::thread::hardware_concurrency();
    return (int)std::max<unsigned>(1u, std::min<unsigned>(hc ? hc : 1u, 16u * (unsigned)devices));
}

// bytes of one staging tile (SDA_HOST_STAGE_MB, default 256 MiB; at least 1 MiB)
uint64_t host_stage_bytes() {
    const long long mb = env_ll("SDA_HOST_STAGE_MB", 256);
    return (uint64_t)std::max<long long>(mb, 1) << 20;
}

// (the tile packing -- pack_rows, pack_rows32 -- is host_pack.h: HIP-free, tested under a host sanitizer)
using sda::pack_rows;
using sda::pack_rows32;

// SDA_HOST_NARROW (read per call): 1 ships every tile whose values fit as int32 rows -- half the bytes over
// PCIe and into the combine --, 0 ships every tile as i64.  The results are bit-identical.
bool host_narrow() { return env_ll("SDA_HOST_NARROW", 1) != 0; }

sda_status host_stream_ensure(sda_engine* h, size_t tile_bytes, size_t acc_bytes) {
    if (!h->copy_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(hipEventCreateWithFlags(&h->h2d_done[b], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&h->tile_free[b], hipEventDisableTiming));
        }
    }
    if (h->hs_pin_bytes < 2 * rup(tile_bytes)) {
        if (h->hs_pin) (void)hipHostFree(h->hs_pin);
        h->hs_pin = nullptr;
        h->hs_pin_bytes = 0;
        HIP_TRY(hipHostMalloc(&h->hs_pin, 2 * rup(tile_bytes), hipHostMallocDefault));
        h->hs_pin_bytes = 2 * rup(tile_bytes);
    }
    const size_t dev_need = 2 * rup(tile_bytes) + rup(acc_bytes);
    if (h->hs_dev_bytes < dev_need) {
        dev_free(h->hs_dev);
        h->hs_dev = nullptr;
        h->hs_dev_bytes = 0;
        if (sda_status e = dev_alloc(&h->hs_dev, dev_need)) return e;
        h->hs_dev_bytes = dev_need;
    }
    return SDA_OK;
}

// combiner.rs:22-25 (|m| > 0) over the column slice [lo, lo + w) of n_rows host rows on h's device, streamed
// in row tiles (section comment); the w results land in out_host.  A row slice wider than a tile is taken in
// column chunks, each a full pass over the rows.
sda_status stream_combine_slice(sda_engine* h, int64_t m, const int64_t* const* rows, uint64_t n_rows, uint64_t lo,
                                uint64_t w, int64_t* out_host, int threads) {
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t stage = host_stage_bytes();
    const bool narrow = host_narrow();
    const uint64_t wc_max = std::max<uint64_t>(2, stage / 8 / 2 * 2);
    for (uint64_t c0 = 0; c0 < w; c0 += wc_max) {
        const uint64_t wc = std::min(wc_max, w - c0);
        const uint64_t R = std::max<uint64_t>(1, stage / (wc * 8));
        const size_t tile = (size_t)(std::min(R, std::max<uint64_t>(n_rows, 1)) * wc * 8);
        if (sda_status e = host_stream_ensure(h, tile, wc * 8)) return e;
        int64_t* dt[2] = {static_cast<int64_t*>(h->hs_dev), static_cast<int64_t*>(h->hs_dev) + rup(tile) / 8};
        int64_t* acc = static_cast<int64_t*>(h->hs_dev) + 2 * rup(tile) / 8;
        int64_t* hp[2] = {static_cast<int64_t*>(h->hs_pin), static_cast<int64_t*>(h->hs_pin) + rup(tile) / 8};
        uint64_t i = 0;
        bool try32 = narrow;                     // until a tile of this column chunk has to ship wide
        for (uint64_t r0 = 0; r0 < n_rows; r0 += R, ++i) {
            const uint64_t Ri = std::min(R, n_rows - r0);
            const int b = (int)(i & 1);
            if (i >= 2) HIP_TRY(hipEventSynchronize(h->h2d_done[b]));        // tile i - 2 has left hp[b]
            if (try32) try32 = pack_rows32(reinterpret_cast<int32_t*>(hp[b]), rows, r0, Ri, lo + c0, wc, threads);
            if (!try32) pack_rows(hp[b], rows, r0, Ri, lo + c0, wc, threads);
            const size_t bytes = (size_t)(Ri * wc * (try32 ? 4 : 8));
            if (i >= 2) HIP_TRY(hipStreamWaitEvent(h->copy_stream, h->tile_free[b], 0));   // ... and dt[b]
            HIP_TRY(hipMemcpyAsync(dt[b], hp[b], bytes, hipMemcpyHostToDevice, h->copy_stream));
            HIP_TRY(hipEventRecord(h->h2d_done[b], h->copy_stream));
            HIP_TRY(hipStreamWaitEvent(h->stream, h->h2d_done[b], 0));
            if (try32)
                HIP_TRY(sda::launch_combine_wide32(reinterpret_cast<const int32_t*>(dt[b]), Ri, wc, wc, acc, m,
                                                   h->stream, i > 0, &h->combine_last));
            else
                HIP_TRY(sda::launch_combine_exact(dt[b], Ri, wc, wc, acc, m, h->stream, i > 0, &h->combine_last));
            HIP_TRY(hipEventRecord(h->tile_free[b], h->stream));
            ++(try32 ? h->hs_tiles32 : h->hs_tiles64);
            h->hs_bytes_h2d += bytes;
        }
        HIP_TRY(hipMemcpyAsync(out_host + c0, acc, wc * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return SDA_OK;
}

size_t n_devices(const sda_engine* h) { return h->sub.empty() ? 1 : h->sub.size(); }

// run fn(g) for every device of the handle, one host thread per device (fn(0) on the caller's thread); the first
// failing device's status and message are returned
template <typename F>
sda_status for_devices(sda_engine* h, F fn) {
    const size_t G = n_devices(h);
    if (G == 1) return fn(0);
    std::vector<sda_status> st(G, SDA_OK);
    std::vector<std::string> msg(G);
    std::vector<std::thread> ts;
    for (size_t g = 1; g < G; ++g)
        ts.emplace_back([&, g] {
            st[g] = fn(g);
            if (st[g]) msg[g] = g_last_error;
        });
    st[0] = fn(0);
    if (st[0]) msg[0] = g_last_error;
    for (auto& t : ts) t.join();
    for (size_t g = 0; g < G; ++g)
        if (st[g]) return fail(st[g], "device %d: %s", h->sub[g]->device, msg[g].c_str());
    return SDA_OK;
}

// even-aligned column split (sda_amd/distributed.py column_slice): [lo, lo + w) of dim for part g of G
void column_slice(uint64_t dim, size_t g, size_t G, uint64_t* lo, uint64_t* w) {
    const uint64_t pairs = (dim + 1) / 2, base = pairs / G, extra = pairs % G;
    const uint64_t start = g * base + std::min<uint64_t>(g, extra), count = base + (g < extra ? 1 : 0);
    *lo = std::min(dim, 2 * start);
    *w = std::min(dim, 2 * (start + count)) - *lo;
}

// contiguous near-equal split of n items (shard_range)
void shard(uint64_t n, size_t g, size_t G, uint64_t* start, uint64_t* count) {
    const uint64_t base = n / G, extra = n % G;
    *start = g * base + std::min<uint64_t>(g, extra);
    *count = base + (g < extra ? 1 : 0);
}

sda_engine* dev_of(sda_engine* h, size_t g) { return h->sub.empty() ? h : h->sub[g]; }

// combiner.rs:16-28 over host rows (validated by combine_rows): one device streams all columns, G devices
// a column slice each
sda_status host_combine(sda_engine* h, int64_t m, const int64_t* const* rows, uint64_t n_rows, uint64_t dim,
                        int64_t* out) {
    const size_t G = n_devices(h);
    const int T = std::max(1, host_threads(G) / (int)G);
    return for_devices(h, [&](size_t g) -> sda_status {
        uint64_t lo, w;
        column_slice(dim, g, G, &lo, &w);
        if (w == 0) return SDA_OK;
        return stream_combine_slice(dev_of(h, g), m, rows, n_rows, lo, w, out + lo, T);
    });
}

// ---- RCCL, loaded when a multi-device handle first reduces (single-device users never load it) ----
struct Rccl {
    bool ok = false;
    std::string err;
    ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t,
                           hipStream_t) = nullptr;
    ncclResult_t (*group_start)() = nullptr;
    ncclResult_t (*group_end)() = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
};

Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) {
            r.err = dlerror() ? dlerror() : "dlopen(librccl.so.1) failed";
            return;
        }
        r.comm_init_all = reinterpret_cast<decltype(r.comm_init_all)>(dlsym(lib, "ncclCommInitAll"));
        r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(lib, "ncclCommDestroy"));
        r.reduce = reinterpret_cast<decltype(r.reduce)>(dlsym(lib, "ncclReduce"));
        r.group_start = reinterpret_cast<decltype(r.group_start)>(dlsym(lib, "ncclGroupStart"));
        r.group_end = reinterpret_cast<decltype(r.group_end)>(dlsym(lib, "ncclGroupEnd"));
        r.error_string = reinterpret_cast<decltype(r.error_string)>(dlsym(lib, "ncclGetErrorString"));
        r.ok = r.comm_init_all && r.comm_destroy && r.reduce && r.group_start && r.group_end && r.error_string;
        if (!r.ok) r.err = "librccl.so.1 lacks an entry point";
    });
    return r;
}

#define NCCL_TRY(expr)                                                                                  \
    do {                                                                                                \
        ncclResult_t _r = (expr);                                                                       \
        if (_r != ncclSuccess)                                                                          \
            return fail(SDA_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, rccl().error_string(_r), __FILE__, \
                        __LINE__);                                                                      \
    } while (0)

bool distinct_devices(const sda_engine* h) {
    for (size_t a = 0; a < h->sub.size(); ++a)
        for (size_t b = a + 1; b < h->sub.size(); ++b)
            if (h->sub[a]->device == h->sub[b]->device) return false;
    return true;
}

sda_status ensure_comms(sda_engine* h) {
    if (h->comms) return SDA_OK;
    Rccl& r = rccl();
    if (!r.ok) return fail(SDA_ERR_DEVICE, "RCCL unavailable: %s", r.err.c_str());
    const size_t G = n_devices(h);
    std::vector<int> devs(G);
    for (size_t g = 0; g < G; ++g) devs[g] = dev_of(h, g)->device;
    std::vector<ncclComm_t> comms(G, nullptr);
    NCCL_TRY(r.comm_init_all(comms.data(), (int)G, devs.data()));
    h->comms = new void*[G];
    for (size_t g = 0; g < G; ++g) h->comms[g] = comms[g];
    return SDA_OK;
}

void destroy_comms(sda_engine* h) {
    if (!h->comms) return;
    for (size_t g = 0; g < n_devices(h); ++g)
        if (h->comms[g]) (void)rccl().comm_destroy(static_cast<ncclComm_t>(h->comms[g]));
    delete[] h->comms;
    h->comms = nullptr;
}

// chacha.rs:57-76 over host seed words [n][w], the combined mask (D values) left in dst on device 0 (ordered on
// h->stream; the other devices are idle again at return): seeds split over the devices, one RCCL reduce onto
// device 0 (section comment).  dst must not lie in device 0's staging arena or work buffer.
sda_status chacha_combine_multi(sda_engine* h, int64_t m, uint64_t D, const std::vector<uint32_t>& seeds, uint32_t w,
                                uint64_t n, int64_t* dst) {
    // (a one-device handle from sda_engine_create_multi takes the split path too: a one-rank reduce)
    const size_t G = n_devices(h);
    const bool split = !h->sub.empty() && distinct_devices(h) && n >= G && !sda::chacha_needs_stream_path(m) &&
                       (unsigned __int128)G * (uint64_t)(m - 1) <= (unsigned __int128)INT64_MAX;
    const size_t parts = split ? G : 1;
    std::vector<int64_t*> partial(parts, nullptr);
    sda_status st = for_devices(h, [&](size_t g) -> sda_status {
        if (g >= parts) return SDA_OK;
        sda_engine* d = dev_of(h, g);
        HIP_TRY(hipSetDevice(d->device));
        uint64_t s0 = 0, cnt = n;
        if (split) shard(n, g, G, &s0, &cnt);
        DevArena a;
        if (sda_status e = stage(d, rup(cnt * w * 4 + 4) + rup(D * 8), &a)) return e;
        uint32_t* dseeds = a.take<uint32_t>(cnt * w + 1);
        partial[g] = split ? a.take<int64_t>(D) : dst;
        if (cnt) HIP_TRY(hipMemcpyAsync(dseeds, seeds.data() + s0 * w, cnt * w * 4, hipMemcpyHostToDevice, d->stream));
        return chacha_combine(d, m, D, dseeds, w, cnt, partial[g], d->stream);
    });
    if (st) return st;
    HIP_TRY(hipSetDevice(h->device));
    if (!split) return SDA_OK;
    h->chacha_split = true;                      // every device recorded its part (sda_chacha_last_launch)
    if (sda_status e = ensure_comms(h)) return e;
    Rccl& r = rccl();
    NCCL_TRY(r.group_start());
    for (size_t g = 0; g < G; ++g) {
        sda_engine* d = dev_of(h, g);
        ncclResult_t rr = r.reduce(partial[g], partial[g], D, ncclInt64, ncclSum, 0,
                                   static_cast<ncclComm_t>(h->comms[g]), d->stream);
        if (rr != ncclSuccess) {
            (void)r.group_end();
            return fail(SDA_ERR_DEVICE, "ncclReduce: %s", r.error_string(rr));
        }
    }
    NCCL_TRY(r.group_end());
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_mod_canonical(partial[0], D, dst, m, h->stream));
    for (size_t g = 1; g < G; ++g) HIP_TRY(hipStreamSynchronize(dev_of(h, g)->stream));   // reduce sent
    return SDA_OK;
}

// the same, the combined mask copied to out_host (MaskCombiner::combine)
sda_status host_chacha_combine(sda_engine* h, int64_t m, uint64_t D, const std::vector<uint32_t>& seeds, uint32_t w,
                               uint64_t n, int64_t* out_host) {
    HIP_TRY(hipSetDevice(h->device));
    if (sda_status e = host_stream_ensure(h, 0, D * 8)) return e;          // dst: the host path's accumulator
    int64_t* dst = static_cast<int64_t*>(h->hs_dev);
    if (sda_status e = chacha_combine_multi(h, m, D, seeds, w, n, dst)) return e;
    HIP_TRY(hipMemcpyAsync(out_host, dst, D * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SDA_OK;
}

// The clerk's job after the sealed-box opens (clerk.rs:79-86): decode every participation's payload
// (sodium.rs:82-88), then combiner.rs:16-28 over the decoded rows in participation order.  Blobs go in groups
// of at most host_stage_bytes() of payload: a host thread packs group g + 1 into pinned buffer (g + 1) mod 2
// while group g uploads and is decoded (int64 rows: any payload, malformed ones included) and combined on the
// compute stream, the recurrence continued across groups -- so a job larger than HBM runs, bit-identical to
// one pass.  The payload crosses PCIe instead of the decoded rows: 4.9 bytes per field share instead of 8.
// Errors in the reference's order: `% 0` folds row 0 before row 1's length is checked, then "Wrong dimension"
// at the first participation whose length differs from participation 0's.  One device (ordinals[0] of a
// multi-device handle): a participation's columns are not locatable in its bytes before it is decoded.
sda_status host_decode_combine(sda_engine* h, int64_t m, const uint8_t* const* blobs, const uint64_t* lens, uint64_t n,
                               int64_t* out, uint64_t out_cap, uint64_t* out_len) {
    *out_len = 0;
    h->codec_last = sda::CodecLaunchInfo();     // this path keeps no record: a stale one must not be read
    if (n == 0) return SDA_OK;                                        // combiner.rs:17: empty input
    const uint64_t stage = host_stage_bytes();
    struct Group { uint64_t b0, nb, bytes; };
    std::vector<Group> groups;
    for (uint64_t i = 0; i < n;) {
        Group g{i, 0, 0};
        while (i < n && (g.nb == 0 || g.bytes + lens[i] <= stage)) g.bytes += lens[i++], ++g.nb;
        groups.push_back(g);
    }
    uint64_t biggest = 0;
    for (auto& g : groups) biggest = std::max(biggest, g.bytes);
    const size_t slot = rup(biggest + 32);                           // 16-byte aligned, 16+ readable bytes past
    if (sda_status e = host_stream_ensure(h, slot, 0)) return e;
    uint8_t* hp[2] = {static_cast<uint8_t*>(h->hs_pin), static_cast<uint8_t*>(h->hs_pin) + rup(slot)};
    uint8_t* dbytes[2] = {static_cast<uint8_t*>(h->hs_dev), static_cast<uint8_t*>(h->hs_dev) + rup(slot)};
    const int T = host_threads();
    auto pack = [&](const Group& g, uint8_t* dst, std::vector<uint64_t>* off) {
        off->assign(g.nb + 1, 0);
        for (uint64_t i = 0; i < g.nb; ++i) (*off)[i + 1] = (*off)[i] + lens[g.b0 + i];
        std::vector<std::thread> ts;
        const uint64_t per = (g.nb + T - 1) / T;
        for (int t = 0; t < T && (uint64_t)t * per < g.nb; ++t)
            ts.emplace_back([&, t] {
                for (uint64_t i = (uint64_t)t * per; i < g.nb && i < (uint64_t)(t + 1) * per; ++i)
                    if (lens[g.b0 + i]) memcpy(dst + (*off)[i], blobs[g.b0 + i], lens[g.b0 + i]);
            });
        for (auto& t : ts) t.join();
        memset(dst + (*off)[g.nb], 0, 32);
    };
    std::vector<uint64_t> off[2], counts;
    pack(groups[0], hp[0], &off[0]);
    uint64_t dim = 0, stride = 0;
    int64_t mm = 1;
    int64_t* acc = nullptr;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const Group& g = groups[gi];
        const int b = (int)(gi & 1);
        HIP_TRY(hipMemcpyAsync(dbytes[b], hp[b], off[b][g.nb] + 32, hipMemcpyHostToDevice, h->copy_stream));
        HIP_TRY(hipEventRecord(h->h2d_done[b], h->copy_stream));
        HIP_TRY(hipStreamWaitEvent(h->stream, h->h2d_done[b], 0));
        // pack the next group while this one decodes (its pinned buffer's previous upload has to be done)
        std::thread next;
        if (gi + 1 < groups.size()) {
            if (gi >= 1) HIP_TRY(hipEventSynchronize(h->h2d_done[b ^ 1]));
            next = std::thread(pack, std::cref(groups[gi + 1]), hp[b ^ 1], &off[b ^ 1]);
        }
        struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } } join{next};
        // rows of this group as int64 [nb][stride]; participation 0 has at most one element per byte
        if (gi == 0) stride = std::max<uint64_t>(lens[0], 1);
        if (sda_status e = ensure(&h->codec_mat, &h->codec_mat_bytes, g.nb * stride * 8 + 8)) return e;
        sda::VarintPlan plan;
        sda::varint_plan(off[b].data(), g.nb, &plan);
        if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes, sda::varint_decode_work_bytes(plan.regions, g.nb)))
            return e;
        counts.assign(g.nb, 0);
        bool too_long = false;
        int64_t* mat = static_cast<int64_t*>(h->codec_mat);
        HIP_TRY(sda::launch_varint_decode_one_wait(dbytes[b], off[b].data(), g.nb, plan, h->codec_work, mat, stride,
                                                   counts.data(), &too_long, h->stream));
        if (gi == 0) {
            dim = counts[0];
            if (dim && m == 0) return modulus_abs(m, &mm);         // row 0 is folded first (combiner.rs:20-25)
            if (dim) {
                if (sda_status e = modulus_abs(m, &mm)) return e;
            }
            if (out_cap < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
            if (dim) {
                if (sda_status e = ensure(&h->work, &h->work_bytes, dim * 8)) return e;
                acc = static_cast<int64_t*>(h->work);
            }
        }
        for (uint64_t i = 0; i < g.nb; ++i)
            if (counts[i] != dim)
                return fail(SDA_ERR_WRONG_DIMENSION, "Wrong dimension (participation %llu decodes to %llu shares, expected %llu)",
                            (unsigned long long)(g.b0 + i), (unsigned long long)counts[i], (unsigned long long)dim);
        if (dim)
            HIP_TRY(sda::launch_combine_exact(mat, g.nb, dim, stride, acc, mm, h->stream, gi > 0, &h->combine_last));
        if (gi == 0) stride = std::max<uint64_t>(dim, 1);            // later groups: rows of exactly dim values
    }
    if (dim) HIP_TRY(hipMemcpyAsync(out, acc, dim * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *out_len = dim;
    return SDA_OK;
}

// additive.rs:32-51 per column (batched.rs:19-53 with input_size 1): columns split over the devices;
// out [n][D] clerk-major
sda_status host_additive_generate(sda_engine* h, int64_t m, uint64_t n, const int64_t* secrets, uint64_t D,
                                  const int64_t* draws, int64_t* out, const KeyedDraws* kd) {
    const size_t G = n_devices(h);
    return for_devices(h, [&](size_t g) -> sda_status {
        uint64_t lo, w;
        column_slice(D, g, G, &lo, &w);
        if (w == 0) return SDA_OK;
        sda_engine* d = dev_of(h, g);
        HIP_TRY(hipSetDevice(d->device));
        DevArena a;
        if (sda_status e = stage(d, rup(w * 8) + rup(w * (n - 1) * 8 + 8) + rup(n * w * 8), &a)) return e;
        int64_t* dsec = a.take<int64_t>(w);
        int64_t* ddr = a.take<int64_t>(w * (n - 1) + 1);
        int64_t* dout = a.take<int64_t>(n * w);
        HIP_TRY(hipMemcpyAsync(dsec, secrets + lo, w * 8, hipMemcpyHostToDevice, d->stream));
        if (n > 1 && kd)      // element d * (n - 1) + j of the call's draws: this slice starts at column lo
            HIP_TRY(sda::launch_draws(kd->key, kd->stream_id, lo * (n - 1), w * (n - 1), m, ddr, d->stream));
        else if (n > 1)
            HIP_TRY(hipMemcpyAsync(ddr, draws + lo * (n - 1), w * (n - 1) * 8, hipMemcpyHostToDevice, d->stream));
        HIP_TRY(sda::launch_additive_generate(dsec, w, ddr, n, dout, m, d->stream));
        HIP_TRY(hipMemcpy2DAsync(out + lo, D * 8, dout, w * 8, w * 8, n, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        return SDA_OK;
    });
}

// packed_shamir.rs:40-43 per batch (batched.rs:19-53): batches split over the devices; out [n][B]
sda_status host_packed_generate(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets, uint64_t D,
                                const int64_t* draws, int64_t* out, const KeyedDraws* kd) {
    const uint64_t k = s->secret_count, t = s->privacy_threshold, n = s->share_count, B = (D + k - 1) / k;
    const size_t G = n_devices(h);
    return for_devices(h, [&](size_t g) -> sda_status {
        uint64_t b0, nb;
        shard(B, g, G, &b0, &nb);
        if (nb == 0) return SDA_OK;
        sda_engine* d = dev_of(h, g);
        HIP_TRY(hipSetDevice(d->device));
        const uint64_t s0 = b0 * k, ds = std::min(D, (b0 + nb) * k) - s0;   // the last batch may be short (padded)
        DevArena a;
        if (sda_status e = stage(d, rup(ds * 8) + rup(nb * t * 8 + 8) + rup(n * nb * 8), &a)) return e;
        int64_t* dsec = a.take<int64_t>(ds);
        int64_t* ddr = a.take<int64_t>(nb * t + 1);
        int64_t* dout = a.take<int64_t>(n * nb);
        HIP_TRY(hipMemcpyAsync(dsec, secrets + s0, ds * 8, hipMemcpyHostToDevice, d->stream));
        if (t && kd)          // element b * t + j of the call's draws: this slice starts at batch b0
            HIP_TRY(sda::launch_draws(kd->key, kd->stream_id, b0 * t, nb * t, s->modulus - 1, ddr, d->stream));
        else if (t)
            HIP_TRY(hipMemcpyAsync(ddr, draws + b0 * t, nb * t * 8, hipMemcpyHostToDevice, d->stream));
        if (sda_status e = ensure(&d->gen_log, &d->gen_log_bytes, sda::packed_gen_log_bytes())) return e;
        sda::PackedGenArgs ga{dsec, ds, 1, ddr, dout};
        HIP_TRY(sda::launch_packed_generate(ga, (uint32_t)k, (uint32_t)t, (uint32_t)n, (uint32_t)s->modulus,
                                            (uint32_t)s->omega_secrets, (uint32_t)s->omega_shares, d->gen_tab,
                                            d->gen_log, d->stream, &d->gen_log_used));
        HIP_TRY(hipMemcpy2DAsync(out + b0, B * 8, dout, nb * 8, nb * 8, n, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        return SDA_OK;
    });
}

// packed_shamir.rs:73-77 per batch (batched.rs:69-97), exact: batches split over the devices; out [dimension]
sda_status host_packed_reconstruct(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                   const uint64_t* indices, const int64_t* const* rows, uint64_t n_rows, int64_t* out) {
    const uint64_t k = s->secret_count, B = (dimension + k - 1) / k;
    const size_t G = n_devices(h);
    return for_devices(h, [&](size_t g) -> sda_status {
        uint64_t b0, nb;
        shard(B, g, G, &b0, &nb);
        if (nb == 0) return SDA_OK;
        sda_engine* d = dev_of(h, g);
        HIP_TRY(hipSetDevice(d->device));
        const uint64_t s0 = b0 * k, ds = std::min(dimension, (b0 + nb) * k) - s0;
        DevArena a;
        if (sda_status e = stage(d, rup(n_rows * nb * 8) + rup(ds * 8), &a)) return e;
        int64_t* din = a.take<int64_t>(n_rows * nb);
        int64_t* dout = a.take<int64_t>(ds);
        for (uint64_t i = 0; i < n_rows; ++i)        // batched.rs:83-85: clerk i's batches [b0, b0 + nb)
            HIP_TRY(hipMemcpyAsync(din + i * nb, rows[i] + b0, nb * 8, hipMemcpyHostToDevice, d->stream));
        if (sda_status e = ensure(&d->gen_log, &d->gen_log_bytes, sda::packed_gen_log_bytes())) return e;
        sda::PackedRevealArgs ra{din, ds, 1, dout};
        HIP_TRY(sda::launch_packed_reveal(ra, indices, (uint32_t)n_rows, (uint32_t)k, (uint32_t)s->privacy_threshold,
                                          (uint32_t)s->modulus,
                                          (uint32_t)s->omega_secrets, (uint32_t)s->omega_shares, SDA_REVEAL_EXACT,
                                          d->rev_tab, d->gen_log, d->stream, &d->gen_log_used));
        HIP_TRY(hipMemcpyAsync(out + s0, dout, ds * 8, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        return SDA_OK;
    });
}

}  // namespace

extern "C" {

sda_status sda_engine_create_multi(const int* ordinals, int n_devices_, sda_engine** out) {
    SDA_ENTRY;
    if (!out) return fail(SDA_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!ordinals || n_devices_ < 1 || n_devices_ > 64)
        return fail(SDA_ERR_INVALID_ARGUMENT, "need 1..64 device ordinals");
    sda_engine* h = nullptr;
    if (sda_status e = sda_engine_create(ordinals[0], &h)) return e;
    if (n_devices_ == 1) {                       // a one-device handle that still reduces through RCCL
        h->sub.push_back(h);
        *out = h;
        return ok();
    }
    h->sub.push_back(h);
    for (int g = 1; g < n_devices_; ++g) {
        sda_engine* d = nullptr;
        if (sda_status e = sda_engine_create(ordinals[g], &d)) {
            const std::string msg = g_last_error;
            sda_engine_destroy(h);
            return fail(e, "device %d: %s", ordinals[g], msg.c_str());
        }
        h->sub.push_back(d);
    }
    HIP_TRY(hipSetDevice(h->device));
    *out = h;
    return ok();
}

int sda_engine_device_count(const sda_engine* h) { return h ? (int)n_devices(h) : 0; }

}  // extern "C"
