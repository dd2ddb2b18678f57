// engine_internal.h -- what the host translation units of the C ABI (include/sda_engine.h) share: the handle, the
// failure / call-scope plumbing, scratch management, and the helpers that more than one of them calls.
//
//   engine.cpp              handle life cycle, call scope, scratch, scheme helpers, the trait calls on host buffers
//   engine_dev.cpp          the device-resident (`_dev`) entry points
//   engine_check.cpp        the packed-Shamir share consistency check, the checked reveal and the decoded reveal
//                           (device and host forms)
//   hbm.cpp                 sda_hbm_*: HBM buffers built from fixed-size physical chunks
//   engine_codec.cpp        the share payload codec's host side and the snapshot transposition
//   engine_recipient.cpp    the fused recipient pipeline, sda_recipient_reveal, the recipient job and their robust
//                           forms over the decoded reveal
//   engine_participant.cpp  the participant pipeline's steps, sda_participant_share*_dev and the participant job
//   engine_host.cpp         the streaming, multi-device host path (RCCL loaded at run time)
//
// Host-side responsibilities only: argument validation with the reference's error behaviour
// (Err strings of client/src/crypto/sharing/*.rs -> status 1..6, assert!/panic -> PRECONDITION),
// staging of host buffers to HBM, kernel launches (kernels.h) and copying results back.  No
// arithmetic on the data happens here and there is no CPU fallback: if the device path fails
// the call fails.
#pragma once

#include "../../include/sda_engine.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "kernels.h"
#include "participant_job_plan.h"

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
    void* keyed_draws = nullptr;  // keyed PackedShamir calls on the staged path: the n_vectors * B * t draws made on the device
    size_t keyed_draws_bytes = 0;
    void* codec_work = nullptr;   // varint codec plan / scan workspace
    size_t codec_work_bytes = 0;
    void* codec_mat = nullptr;    // decoded [N][len] matrix of the clerk decode+combine path
    size_t codec_mat_bytes = 0;
    void* job_work = nullptr;     // sda_clerk_job_dev: the queued encode's workspace (codec_work still holds the decode's);
                                  // a recipient job: the decoded ChaCha seed words and the seed blobs' offsets
    size_t job_work_bytes = 0;
    void* pipe = nullptr;         // recipient / participant pipeline scratch (mask, masked, compacted shares)
    size_t pipe_bytes = 0;
    sda::DeviceTable rev_tab;     // packed-Shamir Newton/Lagrange tables (per scheme + clerk set)
    sda::DeviceTable chk_tab;     // share check and checked reveal: parity rows, basis Lagrange rows, inverse weights
                                  // (per scheme + clerk set; sda::ensure_check_table)
    sda::DeviceTable dec_tab;     // decoded reveal: syndrome rows, points and inverse multipliers (per scheme + clerk
                                  // set; sda::ensure_decode_table)
    void* chk_buf = nullptr;      // their counters, blame words and bad-batch log (sda::packed_check_buf_bytes())
    size_t chk_buf_bytes = 0;
    void* rep_ver = nullptr;      // checked reveal: verdict words when the caller gives no buffer and something is bad
    size_t rep_ver_bytes = 0;
    void* snap = nullptr;         // snapshot transposition copy plan
    size_t snap_bytes = 0;
    // The scratch buffers above are shared by every call on the handle.  A call on another stream
    // than the previous one first waits (on the device) for the work queued on that stream.
    hipStream_t last_stream = nullptr;
    hipEvent_t order_ev = nullptr;
    bool order_ok = true;         // order_ev was recorded when the last call ended (else: host sync)
    unsigned long long* rej_host = nullptr;   // pinned: the ChaCha rejection count of a pipeline's mask
    // The launch records behind the *_last_launch getters, one block per device, so that a job that fails puts every
    // one of them back at once (RecordsGuard).  The launchers receive &h->last.combine and so on.
    struct ClerkJobLaunchInfo {
        uint32_t continued = 0, encode_route = 0;
        uint64_t encode_chunks = 0;
    };
    struct RecipientLaunchInfo {
        uint32_t mask_kind = 0, reveal_mode = 0, fell_back = 0, compact = 0, unmask_launches = 0;
    };
    struct RecipientDecodedLaunchInfo {
        uint32_t unmask_route = 0, reveal_runs = 0, compact = 0;
    };
    struct ParticipantLaunchInfo {
        uint32_t mask_route = 0, share_route = 0, passes = 0;
    };
    struct RecipientJobLaunchInfo {
        uint32_t mask_route = 0, share_route = 0, seeds_decoded = 0;
    };
    struct ParticipantJobLaunchInfo {
        uint32_t mask_route = 0, share_route = 0, share_bytes = 0;
        uint64_t tiles = 0;
    };
    struct CheckLaunchInfo {
        uint32_t path = 0, bucket = 0, overflowed = 0;
        uint64_t located = 0;
    };
    struct RepairLaunchInfo {
        uint32_t path = 0, bucket = 0, overflowed = 0;
        uint64_t fixed = 0;
    };
    struct DecodeLaunchInfo {
        uint32_t path = 0, bucket = 0, max_errors = 0, overflowed = 0;
        uint64_t decoded = 0, fixed = 0;
    };
    struct Records {
        // sda_chacha_last_launch: how the last mask combine or participant mask on this handle ran; chacha_split:
        // that call split its seeds over the handle's devices (chacha_combine_multi), each recording its own part
        sda::ChachaLaunchInfo chacha;
        bool chacha_split = false;
        // sda_codec_last_launch: how the last decode -> combine on this handle produced its result (decode_combine)
        sda::CodecLaunchInfo codec;
        // sda_combine_last_launch: which combine kernel this handle (of a multi-device handle: this device) launched
        // last and on what grid, filled by the launcher where it decides; a call that launches nothing leaves it
        sda::CombineLaunchInfo combine;
        // sda_snapshot_last_launch: what the last successful, non-sizing sda_snapshot_transpose_dev planned and launched
        sda::SnapshotLaunchInfo snapshot;
        // sda_clerk_job_last_launch: written when a clerk job call that launched something returns SDA_OK
        ClerkJobLaunchInfo clerk_job;
        // sda_recipient_last_launch / sda_participant_last_launch: the decisions the last role pipeline call on this
        // handle took (engine_recipient.cpp, engine_participant.cpp), written when a call of dimension > 0 returns SDA_OK
        RecipientLaunchInfo recipient;
        ParticipantLaunchInfo participant;
        // sda_recipient_job_last_launch: where the last recipient job's mask and clerk results came from, written as
        // `recipient` is; sda_participant_job_last_launch: written when a participant job of dimension > 0 returns SDA_OK
        RecipientJobLaunchInfo recipient_job;
        ParticipantJobLaunchInfo participant_job;
        // sda_recipient_decoded_last_launch: how the last robust recipient call (sda_recipient_job_decoded and its
        // device forms) unmasked and how often its reveal passes ran, written as `recipient` is
        RecipientDecodedLaunchInfo recipient_decoded;
        // sda_packed_keyed_last_launch: how the last keyed packed launch on this handle got its draws -- 0 none yet,
        // 1 made in the share kernels, 2 staged through keyed_draws -- and the draw bytes that crossed HBM
        uint32_t keyed_path = 0;
        uint64_t keyed_staged_bytes = 0;
        // sda_packed_check_last_launch: written when a share check that launched something returns SDA_OK
        CheckLaunchInfo check;
        // sda_packed_reveal_checked_last_launch: written when a checked reveal that launched something returns SDA_OK
        RepairLaunchInfo repair;
        // sda_packed_decode_last_launch: written when a decoded reveal that launched something returns SDA_OK
        DecodeLaunchInfo decode;
    } last;
    // participant job (sda_participant_job, sda_participant_job_dev): the share rows [n][B] of a call (a tile of the
    // host form) and the Full mask row behind them -- int32 where they fit by construction, else i64
    void* job_shares = nullptr;
    size_t job_shares_bytes = 0;
    // streaming host path (host rows -> HBM in row tiles, engine_host.cpp): pinned staging and device
    // tiles, double buffered, and a copy stream so a tile's upload overlaps the previous tile's combine
    hipStream_t copy_stream = nullptr;
    hipEvent_t h2d_done[2] = {nullptr, nullptr}, tile_free[2] = {nullptr, nullptr};
    hipEvent_t d2h_done[2] = {nullptr, nullptr};   // the host participant job: a tile's payloads have reached pinned memory
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

// Everything below is internal to the library: hidden, so the dynamic symbol table holds the C ABI alone.
namespace sda_host __attribute__((visibility("hidden"))) {

// ---------------- failures and the call scope (engine.cpp) ----------------
// The thread-local state has one definition each, in engine.cpp: a failure recorded in any translation unit is what
// sda_last_error_message() returns.  last_error() is the thread's message (fail() sets it, ok() clears it).
std::string& last_error();

// Ends the ordering scope of the call in progress on this thread (the handle and stream pick() noted).
void end_call();

// Every extern "C" entry point opens a CallScope (SDA_ENTRY) as its first statement; the outermost scope
// ends the call's ordering scope (end_call) on every return path, after everything the call queued.
// Internal helpers -- and entry points called from entry points -- may return ok()/fail() freely.
extern __thread int t_depth;   // __thread: constant-initialised, so other translation units read it directly
struct CallScope {
    CallScope() { ++t_depth; }
    ~CallScope() {
        if (--t_depth == 0) end_call();
    }
    CallScope(const CallScope&) = delete;
    CallScope& operator=(const CallScope&) = delete;
};
#define SDA_ENTRY ::sda_host::CallScope sda_call_scope_

sda_status fail(sda_status st, const char* fmt, ...);
sda_status ok();

// A failed HIP call also sets the thread's sticky last-error, which the caller's own runtime checks (torch's
// hipGetLastError after each launch) would then report against their next, unrelated op: the status we
// return carries the error, so the sticky copy is cleared.
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            (void)hipGetLastError();                                                               \
            return ::sda_host::fail(_e == hipErrorOutOfMemory ? SDA_ERR_OUT_OF_MEMORY : SDA_ERR_DEVICE, \
                                    "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                          \
    } while (0)

// ---------------- scratch, streams, staging (engine.cpp) ----------------
void dev_free(void* p);
sda_status dev_alloc(void** p, size_t bytes);
sda_status ensure(void** buf, size_t* have, size_t need);
hipStream_t pick(sda_engine* h, void* stream);

struct DevArena {   // bump allocator over the engine's staging buffer
    char* base;
    size_t off = 0;
    template <typename T> T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base + off);
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};
sda_status stage(sda_engine* h, size_t bytes, DevArena* a);
sda_status finish(sda_engine* h);
inline size_t rup(size_t b) { return (b + 255) & ~(size_t)255; }

// ---------------- scheme helpers (engine.cpp) ----------------
sda_status modulus_abs(int64_t m, int64_t* out);
sda_status check_packed(const sda_sharing_scheme* s);

// ---------------- the handle's devices ----------------
inline size_t n_devices(const sda_engine* h) { return h->sub.empty() ? 1 : h->sub.size(); }
// device g of the handle: sub[0] is the handle itself
template <typename H> H* dev_of(H* h, size_t g) { return g == 0 ? h : h->sub[g]; }
// the handle came from sda_engine_create_multi (over one device too: it still reduces through RCCL)
inline bool is_multi(const sda_engine* h) { return !h->sub.empty(); }
// fn(device handle) for the handle itself, or for every device of a multi-device handle, one after the other on
// the caller's thread; stops at the first failure (engine_host.cpp's for_devices is the threaded walk)
template <typename H, typename F>
sda_status for_each_device(H* h, F fn) {
    for (size_t g = 0; g < n_devices(h); ++g)
        if (sda_status st = fn(dev_of(h, g))) return st;
    return SDA_OK;
}

// Every launch record of every device of the handle, copied when the guard is made and written back when it goes
// out of scope unless keep() was called: a job entry point makes one before its first step and calls keep() on its
// success return, so each failing path in between leaves every *_last_launch record the previous call's.
class RecordsGuard {
    sda_engine* h_;
    std::vector<sda_engine::Records> saved_;
    bool keep_ = false;

public:
    explicit RecordsGuard(sda_engine* h) : h_(h) {
        for (size_t g = 0; g < n_devices(h); ++g) saved_.push_back(dev_of(h, g)->last);
    }
    ~RecordsGuard() {
        if (!keep_)
            for (size_t g = 0; g < saved_.size(); ++g) dev_of(h_, g)->last = saved_[g];
    }
    void keep() { keep_ = true; }
    RecordsGuard(const RecordsGuard&) = delete;
    RecordsGuard& operator=(const RecordsGuard&) = delete;
};

// ---------------- ChaCha mask combine (engine.cpp) ----------------
// The fast counter-mode kernel may serve modulus m; SDA_CHACHA_PATH=stream (read per call) is the test hook that
// forces the stream path (both paths are exact; the tests compare them at sizes the oracle cannot finish)
bool chacha_fast_path(int64_t m);
void record_chacha(sda_engine* h, const sda::ChachaLaunchInfo& info);
sda_status chacha_combine(sda_engine* h, int64_t m, uint64_t D, const uint32_t* seeds, uint32_t w, uint64_t n,
                          int64_t* out, hipStream_t st);
struct PendingChacha {
    bool pending = false;
    int64_t m = 0;
    uint64_t D = 0, n = 0;
    const uint32_t* seeds = nullptr;
    uint32_t w = 0;
    int64_t* out = nullptr;
};
sda_status chacha_combine_begin(sda_engine* h, int64_t m, uint64_t D, const uint32_t* seeds, uint32_t w, uint64_t n,
                                int64_t* out, hipStream_t st, PendingChacha* pc);
sda_status chacha_combine_end(sda_engine* h, const PendingChacha& pc, hipStream_t st, bool* changed);
// chacha.rs:62-64: the seed rows as an [n][*width] matrix of key words; *width is the longest row's word count, at
// most 8 (ChaChaRng's key is the first 8 seed words) and at least 1 (empty seeds == the all-zero key); shorter rows
// pad with zero key words
std::vector<uint32_t> pack_seeds(const int64_t* const* rows, const uint64_t* lens, uint64_t n, uint32_t* width);

// ---------------- packed-Shamir launches (engine_dev.cpp) ----------------
// Share generation of `ga` under scheme s on stream st with h's tables and fix-up log; int32 shares (ga.out32)
// at n + 1 = 81 get the handle-owned scratch their narrowing pass needs, and a keyed call (ga.key) off the in-kernel
// path the handle-owned draw scratch; a keyed call that launches records its path (sda_packed_keyed_last_launch).
sda_status packed_generate(sda_engine* h, const sda_sharing_scheme* s, sda::PackedGenArgs ga, hipStream_t st);
// Reveal of `ra` from n_idx clerk shares with h's table and fix-up log (allocated here).  A CANONICAL reveal of
// repeated clerk indices fails with SDA_ERR_UNSUPPORTED and sets *refused (optional), for a caller that can run
// EXACT instead.
sda_status packed_reveal(sda_engine* h, const sda_sharing_scheme* s, const sda::PackedRevealArgs& ra,
                         const uint64_t* indices, uint64_t n_idx, int32_t mode, hipStream_t st,
                         bool* refused = nullptr);

// ---------------- decoded reveal inside the recipient pipeline (engine_check.cpp) ----------------
// What a robust recipient call asks of the decoded reveal and gets back from it: the device buffers of its per-batch
// words (either may be nullptr), then sda_packed_reveal_decoded_dev's counts of the run.
struct DecodedReveal {
    uint16_t* verdict = nullptr;  // device [B]
    uint32_t* wrong = nullptr;    // device [B], 4-byte aligned
    uint64_t redundancy = 0, bad_batches = 0, first_bad = UINT64_MAX, undecoded = 0;
    std::vector<uint64_t> blame;  // [n_idx]
};
// The decoded reveal of one vector of i64 clerk rows (PackedShamir, k + t <= n_idx <= 32, k <= 8, at least one
// batch) with the same table caches, counter block and records as sda_packed_reveal_decoded_dev, and its wait.
// mask == nullptr: ra.out holds the secrets.  Else ra.out[i] = (secret_i - mask[i]) mod p: subtracted in the first
// pass's write-back, or with `unfused` (device scratch of `dimension` values) by a pass of its own behind the plain
// first pass.  Repeated clerk indices are refused before anything is queued.
sda_status reveal_decoded_masked(sda_engine* h, const sda_sharing_scheme* s, const sda::PackedRepairArgs& ra,
                                 const int64_t* mask, int64_t* unfused, const uint64_t* indices, uint64_t n_idx,
                                 DecodedReveal* d, hipStream_t st);

// ---------------- payload encoder (engine_codec.cpp) ----------------
// rows x len values of [rows][stride] device rows (T: int64_t or int32_t) encoded back to back into dst;
// cap_name names the caller's capacity argument in the "too small" failure.
template <typename T>
sda_status encode_rows(sda_engine* h, const T* vals, uint64_t rows, uint64_t len, uint64_t stride, uint8_t* dst,
                       uint64_t dst_cap, uint64_t* row_bytes, hipStream_t st, const char* cap_name);

// ---------------- payload decoder (engine_codec.cpp) ----------------
// The checks every `_dev` call makes of a (bytes, blob_off) pair before anything reads it: the alignment, then the
// offsets' order.  A caller that accepts any pointer with no blobs tests n_blobs first.
sda_status check_blob_buffer(const uint8_t* bytes, const uint64_t* blob_off, uint64_t n_blobs);
// Plan + count n_blobs device-resident blobs (the argument checks of every `_dev` byte buffer, then one wait);
// counts[n_blobs] on the host.
sda_status codec_count(sda_engine* h, const uint8_t* bytes, const uint64_t* blob_off, uint64_t n_blobs,
                       sda::VarintPlan* plan, uint64_t* counts, bool* irregular, hipStream_t st,
                       bool sub_counts = false, bool* long_any = nullptr);
// What sda_clerk_job_dev adds to the decode -> combine (job == nullptr: sda_clerk_decode_combine_dev exactly).
struct ClerkJob {
    uint64_t first;            // participations folded by earlier calls; > 0: a continuing call
    uint64_t prior_dim;        // the dimension they established (continuing calls)
    uint8_t* payload;          // device; nullptr: no encode
    uint64_t payload_cap;
    uint64_t* payload_len;     // host; non-NULL when payload is
};
// decode + combiner.rs:16-28 over device-resident blobs into out (device); *out_len = the count of blob 0.  One
// host wait.  The recipient job reconstructs an Additive scheme's clerk results with it (additive.rs:56-72 is the
// same recurrence).
sda_status decode_combine(sda_engine* h, int64_t m, const uint8_t* bytes, const uint64_t* blob_off, uint64_t n_blobs,
                          int64_t* out, uint64_t out_cap, uint64_t* out_len, hipStream_t st,
                          const ClerkJob* job = nullptr);
// host blobs concatenated into a 16-byte aligned, padded device buffer taken from `a`; (*off)[n + 1]
sda_status upload_blobs(sda_engine* h, const uint8_t* const* blobs, const uint64_t* lens, uint64_t n, DevArena* a,
                        uint8_t** dev, std::vector<uint64_t>* off);

// ---------------- HBM allocator (hbm.cpp) ----------------
bool hbm_owned(void* p);              // p was returned by sda_hbm_alloc and not freed
void hbm_engine_opened(int device);   // live engine handles per device
bool hbm_engine_closed(int device);   // true when that was the device's last live handle

// ---------------- streaming, multi-device host path (engine_host.cpp) ----------------
sda_status host_combine(sda_engine* h, int64_t m, const int64_t* const* rows, uint64_t n_rows, uint64_t dim,
                        int64_t* out);
sda_status host_chacha_combine(sda_engine* h, int64_t m, uint64_t D, const std::vector<uint32_t>& seeds, uint32_t w,
                               uint64_t n, int64_t* out_host);
void destroy_comms(sda_engine* h);
sda_status chacha_combine_multi(sda_engine* h, int64_t m, uint64_t D, const std::vector<uint32_t>& seeds, uint32_t w,
                                uint64_t n, int64_t* dst);
sda_status host_stream_ensure(sda_engine* h, size_t tile_bytes, size_t acc_bytes);
// bytes of one staging tile of the streamed host calls (SDA_HOST_STAGE_MB, read per call)
uint64_t host_stage_bytes();
// out == nullptr (sda_clerk_job): no copy to the host and no capacity check; *acc_dev (optional) = the device
// accumulator holding the *out_len results (handle scratch: valid until the handle's next call), nullptr for none
sda_status host_decode_combine(sda_engine* h, int64_t m, const uint8_t* const* blobs, const uint64_t* lens, uint64_t n,
                               int64_t* out, uint64_t out_cap, uint64_t* out_len, int64_t** acc_dev = nullptr);
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

}  // namespace sda_host
