// engine.cpp -- C ABI of the MI355X SDA engine (include/sda_engine.h): the handle's life cycle, the call scope,
// scratch management, the scheme helpers, the reference's trait calls on host buffers and the diagnostics.  The other
// subsystems are the translation units engine_internal.h lists.
#include "engine_internal.h"

namespace sda_host __attribute__((visibility("hidden"))) {

static thread_local std::string g_last_error;
std::string& last_error() { return g_last_error; }

// The handle and stream of the call in progress on this thread (set by pick()): when the call returns,
// its stream records the handle's order event, so the NEXT call -- on whatever stream -- only waits on
// that event and never touches this call's stream again (the caller may destroy it in between).
static thread_local sda_engine* t_call_h = nullptr;
static thread_local hipStream_t t_call_s = nullptr;
__thread int t_depth = 0;

void end_call() {
    if (t_call_h) {
        t_call_h->order_ok = hipEventRecord(t_call_h->order_ev, t_call_s) == hipSuccess;
        t_call_h = nullptr;
    }
}

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

// Engine scratch comes from hipMalloc.  SDA_SCRATCH_HBM=1 takes scratch of at least kScratchHbmMin bytes from
// sda_hbm_alloc's chunk-mapped backing instead: on a clean box that measured 1.5 % slower for
// the codec's 4 GB slot buffer and neutral for the pipelines (profiles/r05f/ab_scratch_hbm.txt), the same
// direction as the combine's input (§4.1), so it stays opt-in for boxes whose VRAM is fragmented.
constexpr size_t kScratchHbmMin = (size_t)256 << 20;
static bool scratch_hbm(size_t bytes) {
    static const bool on = [] {
        const char* e = getenv("SDA_SCRATCH_HBM");
        return e && atoi(e) == 1;
    }();
    return on && bytes >= kScratchHbmMin;
}

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

static bool is_pow(uint64_t x, uint64_t b) {
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

sda_status stage(sda_engine* h, size_t bytes, DevArena* a) {
    (void)pick(h, h->stream);                  // host entry points run on the engine's own stream
    sda_status st = ensure(&h->stage, &h->stage_bytes, bytes + 4096);
    if (st) return st;
    a->base = static_cast<char*>(h->stage);
    a->off = 0;
    return SDA_OK;
}

bool chacha_fast_path(int64_t m) {
    const char* force = getenv("SDA_CHACHA_PATH");
    return !sda::chacha_needs_stream_path(m) && !(force && strcmp(force, "stream") == 0);
}

// chacha.rs:57-76: combine of n seed streams ([n][w] u32 words on the device) into out (device, D
// values).  The fast counter-mode kernel where its rejection log suffices; otherwise (moduli above
// 2^62, high rejection rates, or a log overflow) the exact stream path.
// Every ChaCha launch leaves how it ran in the handle (sda_chacha_last_launch).
void record_chacha(sda_engine* h, const sda::ChachaLaunchInfo& info) {
    h->last.chacha = info;
    h->last.chacha_split = false;
}

sda_status chacha_combine(sda_engine* h, int64_t m, uint64_t D, const uint32_t* seeds, uint32_t w, uint64_t n,
                          int64_t* out, hipStream_t st) {
    if (D == 0) return SDA_OK;
    sda::ChachaLaunchInfo info;
    if (chacha_fast_path(m)) {
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
sda_status chacha_combine_begin(sda_engine* h, int64_t m, uint64_t D, const uint32_t* seeds, uint32_t w, uint64_t n,
                                int64_t* out, hipStream_t st, PendingChacha* pc) {
    *pc = PendingChacha{};
    if (D == 0) return SDA_OK;
    if (!chacha_fast_path(m) || n == 0)
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
    h->last.chacha.fixups = (uint64_t)fixups;    // the late resolve of the plan chacha_combine_begin recorded
    if (!overflow) return SDA_OK;
    if (sda_status e = ensure(&h->work, &h->work_bytes, sda::chacha_stream_work_bytes(pc.D, pc.n, pc.m))) return e;
    HIP_TRY(sda::launch_chacha_streams_combine(pc.m, pc.D, pc.seeds, pc.w, pc.n, pc.out, h->work, st));
    h->last.chacha.path = sda::kChachaOverflow;
    return SDA_OK;
}

// chacha.rs:36-45: masked = (secrets + draw) % m for one seed (host words); mask = scratch of D values
static sda_status chacha_mask(sda_engine* h, int64_t m, const uint32_t* seed_host, uint32_t w, const int64_t* secrets,
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

std::vector<uint32_t> pack_seeds(const int64_t* const* rows, const uint64_t* lens, uint64_t n, uint32_t* width) {
    uint64_t w = 0;
    for (uint64_t i = 0; i < n; ++i) w = lens[i] > w ? lens[i] : w;
    if (w > 8) w = 8;                                       // ChaChaRng key = first 8 seed words
    if (w == 0) w = 1;                                      // empty seeds == all-zero key
    std::vector<uint32_t> seeds(n * w, 0u);                 // shorter seeds pad with zero key words
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = 0; j < lens[i] && j < w; ++j) seeds[i * w + j] = (uint32_t)rows[i][j];   // chacha.rs:62-64
    *width = (uint32_t)w;
    return seeds;
}

// The staged round trip of the elementwise host calls over D values: x is uploaded from x_host and y from y_host
// (y_host NULL: launch fills y), launch(x, y, out) queues the kernels on the handle's stream, then out is copied to
// out_host (and y to y_out when given) and the call waits for its stream.
template <typename F>
static sda_status elementwise_round_trip(sda_engine* h, uint64_t D, const int64_t* x_host, const int64_t* y_host,
                                         int64_t* out_host, int64_t* y_out, F launch) {
    DevArena a;
    if (sda_status st = stage(h, 3 * rup(D * 8), &a)) return st;
    int64_t* dx = a.take<int64_t>(D);
    int64_t* dy = a.take<int64_t>(D);
    int64_t* dout = a.take<int64_t>(D);
    HIP_TRY(hipMemcpyAsync(dx, x_host, D * 8, hipMemcpyHostToDevice, h->stream));
    if (y_host) HIP_TRY(hipMemcpyAsync(dy, y_host, D * 8, hipMemcpyHostToDevice, h->stream));
    if (sda_status st = launch(dx, dy, dout)) return st;
    HIP_TRY(hipMemcpyAsync(out_host, dout, D * 8, hipMemcpyDeviceToHost, h->stream));
    if (y_out) HIP_TRY(hipMemcpyAsync(y_out, dy, D * 8, hipMemcpyDeviceToHost, h->stream));
    return finish(h);
}

}  // namespace sda_host

using namespace sda_host;

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
    dev_free(h->chk_buf);
    dev_free(h->rep_ver);
    dev_free(h->gen32_tmp);
    dev_free(h->keyed_draws);
    dev_free(h->codec_work);
    dev_free(h->codec_mat);
    dev_free(h->job_work);
    dev_free(h->job_shares);
    dev_free(h->pipe);
    dev_free(h->snap);
    dev_free(h->stage);
    sda::free_table(h->gen_tab);
    sda::free_table(h->rev_tab);
    sda::free_table(h->chk_tab);
    sda::free_table(h->dec_tab);
    if (h->rej_host) (void)hipHostFree(h->rej_host);
    if (h->hs_pin) (void)hipHostFree(h->hs_pin);
    dev_free(h->hs_dev);
    for (int b = 0; b < 2; ++b) {
        if (h->h2d_done[b]) (void)hipEventDestroy(h->h2d_done[b]);
        if (h->tile_free[b]) (void)hipEventDestroy(h->tile_free[b]);
        if (h->d2h_done[b]) (void)hipEventDestroy(h->d2h_done[b]);
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
    if (sda_status st = for_each_device(h, [](sda_engine* d) -> sda_status {   // every device of a multi-device handle
            HIP_TRY(hipSetDevice(d->device));
            HIP_TRY(hipDeviceSynchronize());
            return SDA_OK;
        }))
        return st;
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
    // row tiles through pinned double buffers, column slices over the handle's devices (engine_host.cpp):
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
        auto add = [&](const int64_t* ds, const int64_t* dm, int64_t* dout) -> sda_status {
            HIP_TRY(sda::launch_addsub_trem(ds, dm, +1, D, dout, s->modulus, h->stream));
            return SDA_OK;
        };
        if (sda_status st = elementwise_round_trip(h, D, secrets, full_masks, masked_out, nullptr, add)) return st;
        memcpy(mask_out, full_masks, D * 8);
        *mask_len = D;
        return ok();
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
    auto draw_add = [&](const int64_t* ds, int64_t* dm, int64_t* dout) -> sda_status {
        HIP_TRY(sda::launch_draws(key, stream_id, 0, D, s->modulus, dm, h->stream));
        HIP_TRY(sda::launch_addsub_trem(ds, dm, +1, D, dout, s->modulus, h->stream));
        return SDA_OK;
    };
    if (sda_status st = elementwise_round_trip(h, D, secrets, nullptr, masked_out, mask_out, draw_add)) return st;
    *mask_len = D;
    return ok();
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
    if (D && !out) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // chacha.rs:69 gen_range(0, m) runs once per seed row and element: no row, no draw, whatever the modulus
    if (D && n_rows && s->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    *out_len = D;
    if (D == 0) return ok();
    if (n_rows == 0) {                                      // chacha.rs:58 vec![0; self.dimension], returned as it is
        memset(out, 0, D * 8);
        return ok();
    }
    uint32_t w;
    const std::vector<uint32_t> seeds = pack_seeds(rows, lens, n_rows, &w);
    // seeds split over the handle's devices, one RCCL reduce (engine_host.cpp); one device: all seeds
    if (sda_status st = host_chacha_combine(h, s->modulus, D, seeds, w, n_rows, out)) return st;
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
    return elementwise_round_trip(h, D, masked, mask, out, nullptr,
                                  [&](const int64_t* dms, const int64_t* dm, int64_t* dout) -> sda_status {
                                      HIP_TRY(sda::launch_addsub_trem(dms, dm, -1, D, dout, m, h->stream));   // (ms - m) % q
                                      return SDA_OK;
                                  });
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


sda_status sda_host_stream_stats(const sda_engine* h, uint64_t* tiles_i32, uint64_t* tiles_i64,
                                 uint64_t* bytes_h2d) {
    SDA_ENTRY;
    if (!h) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    uint64_t t32 = 0, t64 = 0, by = 0;
    (void)for_each_device(h, [&](const sda_engine* e) {
        t32 += e->hs_tiles32;
        t64 += e->hs_tiles64;
        by += e->hs_bytes_h2d;
        return SDA_OK;
    });
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
    if (sda_status st = for_each_device(h, add)) return st;
    if (is_multi(h)) HIP_TRY(hipSetDevice(h->device));
    *batches = total;
    return ok();
}

sda_status sda_chacha_last_launch(sda_engine* h, uint32_t* path, uint64_t* grid_y, uint64_t* fixups) {
    SDA_ENTRY;
    if (!h || !path || !grid_y || !fixups) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // host-side records, final when the call that made them returned: nothing to wait for
    *path = h->last.chacha.path;
    *grid_y = h->last.chacha.grid_y;
    uint64_t total = h->last.chacha.fixups;
    if (h->last.chacha_split)
        for (size_t g = 1; g < h->sub.size(); ++g) total += h->sub[g]->last.chacha.fixups;   // sub[0] is the handle
    *fixups = total;
    return ok();
}

sda_status sda_codec_last_launch(sda_engine* h, uint32_t* path, uint32_t* width, uint32_t* fell_back,
                                 uint64_t* passes) {
    SDA_ENTRY;
    if (!h || !path || !width || !fell_back || !passes) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for
    *path = h->last.codec.path;
    *width = h->last.codec.width;
    *fell_back = h->last.codec.fell_back;
    *passes = h->last.codec.passes;
    return ok();
}

sda_status sda_clerk_job_last_launch(sda_engine* h, uint32_t* continued, uint32_t* encode_route,
                                     uint64_t* encode_chunks) {
    SDA_ENTRY;
    if (!h || !continued || !encode_route || !encode_chunks) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for
    *continued = h->last.clerk_job.continued;
    *encode_route = h->last.clerk_job.encode_route;
    *encode_chunks = h->last.clerk_job.encode_chunks;
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
    const sda::CombineLaunchInfo& c = h->last.combine;
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

sda_status sda_snapshot_last_launch(sda_engine* h, uint64_t* blobs, uint64_t* chunks, uint64_t* grid,
                                    uint64_t* chunk_bytes, uint32_t* shifts) {
    SDA_ENTRY;
    if (!h || !blobs || !chunks || !grid || !chunk_bytes || !shifts)
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for
    const sda::SnapshotLaunchInfo& s = h->last.snapshot;
    *blobs = s.blobs;
    *chunks = s.chunks;
    *grid = s.grid;
    *chunk_bytes = s.chunk_bytes;
    *shifts = s.shifts;
    return ok();
}

sda_status sda_recipient_last_launch(sda_engine* h, uint32_t* mask_kind, uint32_t* reveal_mode, uint32_t* fell_back,
                                     uint32_t* compact, uint32_t* unmask_launches) {
    SDA_ENTRY;
    if (!h || !mask_kind || !reveal_mode || !fell_back || !compact || !unmask_launches)
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for
    const sda_engine::RecipientLaunchInfo& r = h->last.recipient;
    *mask_kind = r.mask_kind;
    *reveal_mode = r.reveal_mode;
    *fell_back = r.fell_back;
    *compact = r.compact;
    *unmask_launches = r.unmask_launches;
    return ok();
}

sda_status sda_participant_last_launch(sda_engine* h, uint32_t* mask_route, uint32_t* share_route, uint32_t* passes) {
    SDA_ENTRY;
    if (!h || !mask_route || !share_route || !passes) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for
    const sda_engine::ParticipantLaunchInfo& r = h->last.participant;
    *mask_route = r.mask_route;
    *share_route = r.share_route;
    *passes = r.passes;
    return ok();
}

}  // extern "C"
