// engine_participant.cpp -- the participant pipeline of the C ABI (include/sda_engine.h) as
// three steps (checks, mask, share generation + payload encoding), and sda_participant_share*_dev and the participant
// job built from them.
#include "engine_internal.h"

using namespace sda_host;

namespace {

// One participant call (participate.rs:53-98 without the sealing) on device-resident inputs.  A tile of the host
// job is a call of its own: its secrets, rows and payload buffers differ, the rest is the job's.
struct ParticipantCall {
    const sda_masking_scheme* ms;
    const sda_sharing_scheme* ss;
    const int64_t* secrets;
    uint64_t dimension;
    int32_t mode;
    hipStream_t st = nullptr;
    // the mask: ChaCha's seed words (host), or the drawn Full masks (device)
    const uint32_t* seed = nullptr;
    uint64_t seed_words = 0;
    const int64_t* full_masks = nullptr;
    // a job's Full mask: `full_masks` is NULL and the mask is drawn in the masking kernel (mask_keyed.hip) from
    // (mask_key, mask_stream_id); its `dimension` values go to mask64, or to mask32 as int32 when that is given
    const uint32_t* mask_key = nullptr;
    uint32_t mask_stream_id = 0;
    int64_t* mask64 = nullptr;
    int32_t* mask32 = nullptr;
    // the share-generation draws: `draws` on the device, or (keyed) made there from (key, stream_id) -- Additive in
    // the fused kernel, PackedShamir in the share kernels or staged in h->keyed_draws (packed_generate)
    const int64_t* draws = nullptr;
    bool keyed = false;
    const uint32_t* key = nullptr;
    uint32_t stream_id = 0;
    // the call's first batch (Additive: column) within a job: where its keyed draws and its part of the mask begin
    uint64_t first = 0;
    // one of shares64 / shares32 is the [n][B] output (int32 rows: PackedShamir, and keyed Additive up to modulus 2^31)
    int64_t* shares64 = nullptr;
    int32_t* shares32 = nullptr;
    uint8_t* payload = nullptr;   // the n encoded rows back to back, payload_row_bytes[n] their lengths (host)
    uint64_t payload_cap = 0;
    uint64_t* payload_row_bytes = nullptr;
    bool packed() const { return ss->kind == SDA_SHARING_PACKED_SHAMIR; }
    uint64_t batches() const { return packed() ? (dimension + ss->secret_count - 1) / ss->secret_count : dimension; }
};

// Step 1: what the schemes and the mode must satisfy, before anything is queued.
sda_status participant_checks(const ParticipantCall& c) {
    const sda_sharing_scheme* ss = c.ss;
    const bool packed = c.packed();
    if (!packed && ss->kind != SDA_SHARING_ADDITIVE) return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    if (!packed && c.shares32 && !c.keyed)
        return fail(SDA_ERR_UNSUPPORTED, "int32 shares need a PackedShamir scheme: an additive scheme's first n - 1 "
                                         "shares are the caller's draws, copied unchecked");
    if (c.mode != SDA_REVEAL_EXACT && c.mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
    if (packed) return check_packed(ss);
    if (ss->share_count == 0) return fail(SDA_ERR_PRECONDITION, "share_count - 1 underflows (additive.rs:42)");
    if (ss->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    if (c.shares32 && ss->modulus > (int64_t)1 << 31)
        return fail(SDA_ERR_UNSUPPORTED, "int32 shares of an additive scheme need modulus <= 2^31: its first n - 1 "
                                         "shares are draws in [0, modulus), which need not fit int32");
    return SDA_OK;
}

// What step 2 leaves: the masked secrets, how they were made, and what the pending rejection check needs.
struct MaskStep {
    const int64_t* masked = nullptr;  // the call's secrets (no mask, or none of them), else h->pipe
    uint32_t route = 1;               // sda_participant_last_launch's mask_route
    bool pending = false;             // ChaCha's fused mask add: its rejection count is still to be read (participant_mask_settle)
    int64_t* cmask = nullptr;         // the mask itself, and its cw seed words, in h->pipe behind the masked secrets
    uint32_t* cseed = nullptr;
    uint32_t cw = 0;
};

// Step 2: SecretMasker::mask (participate.rs:53-54), queued on c.st.
sda_status participant_mask(sda_engine* h, const ParticipantCall& c, MaskStep* m) {
    const sda_masking_scheme* ms = c.ms;
    const uint64_t D = c.dimension;
    hipStream_t st = c.st;
    *m = MaskStep();
    m->masked = c.secrets;
    // chacha.rs:26 assert_eq!(self.dimension, secrets.len()): before any draw, and for an empty secrets vector too
    if (ms->kind == SDA_MASKING_CHACHA && ms->dimension != D)
        return fail(SDA_ERR_PRECONDITION, "assertion failed: dimension == secrets.len()");
    if (ms->kind == SDA_MASKING_NONE || !D) return SDA_OK;
    if (ms->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    if (sda_status e = ensure(&h->pipe, &h->pipe_bytes, 2 * rup(D * 8) + 256)) return e;
    int64_t* dm = static_cast<int64_t*>(h->pipe);
    if (ms->kind == SDA_MASKING_FULL && c.mask_key) {
        // full.rs:25-31 in one kernel: element d of the call is element first k + d of the job's mask
        const uint64_t k = c.packed() ? c.ss->secret_count : 1;
        HIP_TRY(sda::launch_full_mask_keyed(c.mask_key, c.mask_stream_id, c.first * k, c.secrets, D, ms->modulus, dm,
                                            c.mask64, c.mask32, st));
        m->route = 5;
    } else if (ms->kind == SDA_MASKING_FULL) {
        if (!c.full_masks) return fail(SDA_ERR_INVALID_ARGUMENT, "Full masking needs the drawn masks");
        HIP_TRY(sda::launch_addsub_trem(c.secrets, c.full_masks, +1, D, dm, ms->modulus, st));      // full.rs:28-31
        m->route = 2;
    } else if (ms->kind == SDA_MASKING_CHACHA) {
        const uint64_t want = (ms->seed_bitsize + 31) / 32;
        if (c.seed_words != want || (c.seed_words && !c.seed))
            return fail(SDA_ERR_PRECONDITION, "expected %llu seed words", (unsigned long long)want);
        int64_t* dmask = dm + rup(D * 8) / 8;
        uint32_t* dseed = reinterpret_cast<uint32_t*>(dmask + rup(D * 8) / 8);
        const uint32_t w = (uint32_t)(c.seed_words < 8 ? c.seed_words : 8);
        if (w) HIP_TRY(hipMemcpyAsync(dseed, c.seed, w * 4, hipMemcpyHostToDevice, st));
        // chacha.rs:36-45: masked = (secrets + draw) % m over one stream
        if (chacha_fast_path(ms->modulus)) {
            if (sda_status e = ensure(&h->work, &h->work_bytes, sda::chacha_work_bytes(D, 0))) return e;
            sda::ChachaLaunchInfo info;
            HIP_TRY(sda::launch_chacha_mask_add_async(ms->modulus, D, dseed, w, c.secrets, dm, h->work, st, h->rej_host,
                                                      &info));
            record_chacha(h, info);
            m->pending = true;
            m->route = 3;
        } else {
            if (sda_status e = chacha_combine(h, ms->modulus, D, dseed, w, 1, dmask, st)) return e;
            HIP_TRY(sda::launch_addsub_trem(c.secrets, dmask, +1, D, dm, ms->modulus, st));
            m->route = 4;
        }
        m->cmask = dmask, m->cseed = dseed, m->cw = w;
    } else {
        return fail(SDA_ERR_INVALID_ARGUMENT, "unknown masking scheme kind");
    }
    m->masked = dm;
    return SDA_OK;
}

// The pending mask's rejection count, read after one wait: a nonzero count -- probability < 2^-28 per draw -- redoes
// the mask exactly and sets *redone, and the caller then redoes every later step.
sda_status participant_mask_settle(sda_engine* h, const ParticipantCall& c, const MaskStep& m, bool* redone) {
    *redone = false;
    if (!m.pending) return SDA_OK;
    HIP_TRY(hipStreamSynchronize(c.st));
    if (!*h->rej_host) return SDA_OK;
    if (sda_status e = chacha_combine(h, c.ms->modulus, c.dimension, m.cseed, m.cw, 1, m.cmask, c.st)) return e;
    // the record stays the mask add's, with the redo's fix-up count (or its log overflow)
    if (h->last.chacha.path != sda::kChachaOverflow) {
        h->last.chacha.path = sda::kChachaMaskAdd;
        h->last.chacha.grid_y = 1;
    }
    HIP_TRY(sda::launch_addsub_trem(c.secrets, m.cmask, +1, c.dimension, const_cast<int64_t*>(m.masked), c.ms->modulus,
                                    c.st));
    *redone = true;
    return SDA_OK;
}

// Step 3: ShareGenerator::generate (participate.rs:75-76) over `masked`, shares [n][B], then the per-clerk payload
// encoding (participate.rs:79-98 -> sodium.rs:36-41); sealing stays on the host.
sda_status participant_generate_encode(sda_engine* h, const ParticipantCall& c, const int64_t* masked) {
    const sda_sharing_scheme* ss = c.ss;
    const uint64_t D = c.dimension, n = ss->share_count, B = c.batches();
    if (B) {
        if (c.packed()) {
            sda::PackedGenArgs ga{masked, D, 1, c.draws, c.shares64, c.mode == SDA_REVEAL_CANONICAL};
            ga.out32 = c.shares32;           // as sda_packed_generate32_dev: scratch + narrowing at n + 1 = 81
            if (c.keyed) {                   // batch b takes draws b t + j of (key, stream_id) at bound p - 1
                ga.key = c.key;
                ga.stream_id = c.stream_id;
                ga.first_batch = c.first;
            }
            if (sda_status e = packed_generate(h, ss, ga, c.st)) return e;
        } else if (c.keyed) {
            HIP_TRY(sda::launch_additive_generate_keyed(c.key, c.stream_id, c.first, masked, D, n, ss->modulus,
                                                        c.shares64, c.shares32, B, c.st));
        } else {
            HIP_TRY(sda::launch_additive_generate(masked, D, c.draws, n, c.shares64, ss->modulus, c.st));
        }
    }
    if (!c.payload) return SDA_OK;
    return c.shares32 ? encode_rows(h, c.shares32, n, B, B, c.payload, c.payload_cap, c.payload_row_bytes, c.st, "payload_cap")
                      : encode_rows(h, c.shares64, n, B, B, c.payload, c.payload_cap, c.payload_row_bytes, c.st, "payload_cap");
}

// The recipient's mask payload (participate.rs:56-72) of a job's Full mask: the call's mask row, as it was drawn.
sda_status encode_full_mask(sda_engine* h, const ParticipantCall& c, uint8_t* dst, uint64_t cap, uint64_t* len,
                            const char* cap_name) {
    const uint64_t D = c.dimension;
    return c.mask32 ? encode_rows(h, c.mask32, 1, D, D, dst, cap, len, c.st, cap_name)
                    : encode_rows(h, c.mask64, 1, D, D, dst, cap, len, c.st, cap_name);
}

// The three steps in order on `stream`, behind the four sda_participant_share*_dev calls and sda_participant_job_dev.
sda_status participant_share(sda_engine* h, ParticipantCall& c, void* stream) {
    if (!h || !c.ms || !c.ss || (c.dimension && (!c.secrets || (!c.shares64 && !c.shares32))) ||
        (c.payload && !c.payload_row_bytes) || (c.keyed && !c.key))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    c.st = pick(h, stream);
    if (sda_status e = participant_checks(c)) return e;
    MaskStep m;
    if (sda_status e = participant_mask(h, c, &m)) return e;
    if (c.batches() && !c.draws && !c.keyed) return fail(SDA_ERR_INVALID_ARGUMENT, "need the randomness draws");
    if (c.payload && c.ss->share_count > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 clerks");
    if (sda_status e = participant_generate_encode(h, c, m.masked)) return e;
    bool redone = false;
    if (sda_status e = participant_mask_settle(h, c, m, &redone)) return e;
    if (redone)
        if (sda_status e = participant_generate_encode(h, c, m.masked)) return e;
    // sda_participant_last_launch: the handle's record only once this call returns SDA_OK
    if (c.dimension)
        h->last.participant = {m.route, c.packed() ? (c.keyed ? 4u : 3u) : (c.keyed ? 2u : 1u), redone ? 2u : 1u};
    return ok();
}

// What both job forms settle before any work: the schemes' kinds, the payload bounds and the width of the rows.
struct ParticipantJobSetup {
    sda::ParticipantJobShape shape;
    uint64_t row_bound = 0, mask_bound = 0;   // sda_participant_job_payload_bound
    bool packed = false, full = false, chacha = false;
    uint64_t k = 1, units = 0;                // secrets of a batch (Additive: 1); the job's batches (Additive: columns)
    uint32_t share_bytes = 8, mask_bytes = 0; // of a share / a Full mask value in handle scratch
    uint32_t mask_route = 0;                  // sda_participant_job_last_launch
};

sda_status participant_job_setup(const sda_masking_scheme* ms, const sda_sharing_scheme* ss, uint64_t D,
                                 uint32_t mask_stream_id, uint32_t share_stream_id, ParticipantJobSetup* s) {
    if (ms->kind != SDA_MASKING_NONE && ms->kind != SDA_MASKING_FULL && ms->kind != SDA_MASKING_CHACHA)
        return fail(SDA_ERR_INVALID_ARGUMENT, "unknown masking scheme kind");
    if (ss->kind != SDA_SHARING_ADDITIVE && ss->kind != SDA_SHARING_PACKED_SHAMIR)
        return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    s->packed = ss->kind == SDA_SHARING_PACKED_SHAMIR;
    s->full = ms->kind == SDA_MASKING_FULL;
    s->chacha = ms->kind == SDA_MASKING_CHACHA;
    if (ss->share_count > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 clerks");
    // the key contract: one (key, stream_id) pair must not serve the mask and the shares
    if (s->full && mask_stream_id == share_stream_id)
        return fail(SDA_ERR_INVALID_ARGUMENT, "mask_stream_id and share_stream_id must differ");
    s->shape = {ms->kind, ms->modulus, (ms->seed_bitsize + 31) / 32, s->packed, ss->modulus,
                s->packed ? ss->secret_count : 1, ss->share_count};
    if (!sda::participant_job_bound(s->shape, D, &s->row_bound, &s->mask_bound))
        return fail(SDA_ERR_INVALID_ARGUMENT, "the payload bound does not fit 64 bits");
    s->k = s->packed ? std::max<uint64_t>(ss->secret_count, 1) : 1;
    s->units = D / s->k + (D % s->k ? 1 : 0);
    // int32 rows wherever they fit by construction (sda_participant_share32_keyed_dev's rule)
    s->share_bytes = s->packed || ss->modulus <= (int64_t)1 << 31 ? 4 : 8;
    s->mask_bytes = s->full ? (ms->modulus <= (int64_t)1 << 31 ? 4 : 8) : 0;
    s->mask_route = s->full ? (s->mask_bytes == 8 ? 1u : 2u) : s->chacha ? 3u : 0u;
    return SDA_OK;
}

// A job's call: every draw keyed, a Full mask drawn in the masking kernel.  The rows come from job_rows.
ParticipantCall job_call(const ParticipantJobSetup& s, const sda_masking_scheme* ms, const sda_sharing_scheme* ss,
                         int32_t mode, const uint32_t* key, uint32_t mask_stream_id, uint32_t share_stream_id) {
    ParticipantCall c{ms, ss, nullptr, 0, mode};
    c.keyed = true, c.key = key, c.stream_id = share_stream_id;
    if (s.full) c.mask_key = key, c.mask_stream_id = mask_stream_id;
    return c;
}

// chacha.rs:48-50: the mask is the seed words `as i64`; their encoding (sodium.rs:36-41) made on the host
std::vector<uint8_t> encode_seed_words(const uint32_t* seed, uint64_t words) {
    std::vector<uint8_t> out;
    out.reserve(words * sda::kSeedWordBytes);
    for (uint64_t i = 0; i < words; ++i) {
        uint64_t z = (uint64_t)seed[i] << 1;                // zigzag of a value >= 0
        do {
            const uint8_t b = (uint8_t)(z & 127);
            z >>= 7;
            out.push_back(z ? (uint8_t)(b | 128) : b);
        } while (z);
    }
    return out;
}

// The call's (a tile's) share rows [n][B] and the Full mask row [c->dimension] behind them, in h->job_shares.
sda_status job_rows(sda_engine* h, const ParticipantJobSetup& s, uint64_t B, ParticipantCall* c) {
    uint64_t shares, mask;
    if (__builtin_mul_overflow(s.shape.n, B, &shares) || __builtin_mul_overflow(shares, (uint64_t)s.share_bytes, &shares) ||
        __builtin_mul_overflow(c->dimension, (uint64_t)s.mask_bytes, &mask) || shares > (uint64_t)1 << 62 ||
        mask > (uint64_t)1 << 62)
        return fail(SDA_ERR_OUT_OF_MEMORY, "the share rows do not fit the address space");
    if (sda_status e = ensure(&h->job_shares, &h->job_shares_bytes, rup(shares) + rup(mask) + 256)) return e;
    char* base = static_cast<char*>(h->job_shares);
    c->shares32 = s.share_bytes == 4 ? reinterpret_cast<int32_t*>(base) : nullptr;
    c->shares64 = s.share_bytes == 4 ? nullptr : reinterpret_cast<int64_t*>(base);
    c->mask32 = s.mask_bytes == 4 ? reinterpret_cast<int32_t*>(base + rup(shares)) : nullptr;
    c->mask64 = s.mask_bytes == 8 ? reinterpret_cast<int64_t*>(base + rup(shares)) : nullptr;
    return SDA_OK;
}

// The host job's tiles of whole batches (Additive: columns).  Tile i + 1's secrets go up on the copy stream while tile i
// computes and tile i - 1's payloads come down; each half of both buffers is [secrets | clerk payloads | mask payload].
struct JobTiles {
    sda_engine* h;
    const ParticipantJobSetup& s;
    const sda::ParticipantTilePlan plan;
    const ParticipantCall call;               // the job's call: a tile's differs in its secrets, rows and payloads
    const int64_t* secrets;                   // host
    const int64_t* masked_all;                // ChaCha: the whole vector's masked secrets on the device, else NULL
    uint8_t* const* clerk_payloads;           // the caller's blobs
    uint8_t* mask_payload;
    std::vector<uint64_t> lens;               // the clerks' running offsets; the caller's arrays are set at the end
    uint64_t mlen;
    uint32_t mask_route = 1;                  // of the tiles' own masking step
    size_t sec_b = 0, pay_b = 0, mpay_b = 0;
    uint8_t *hp[2] = {nullptr, nullptr}, *dv[2] = {nullptr, nullptr};
    std::vector<uint64_t> row_bytes[2];
    uint64_t mask_bytes[2] = {0, 0};

    struct Tile {
        uint64_t u0, units, s0, ds;           // its first batch and their number, its first secret and their number
        int b;                                // its half of the buffers
    };
    Tile tile(uint64_t i) const {
        const uint64_t u0 = i * plan.tile, u1 = std::min(plan.units, u0 + plan.tile), s0 = u0 * s.k;
        return {u0, u1 - u0, s0, std::min(call.dimension, u1 * s.k) - s0, (int)(i & 1)};   // the last batch may be short
    }
    sda_status run() {
        const uint64_t n = s.shape.n, te = std::min(call.dimension, plan.tile * s.k);    // secrets of a full tile
        sec_b = s.chacha ? 0 : rup(te * 8);
        pay_b = rup(n * plan.tile * sda::participant_share_bytes_bound(s.shape) + 64);
        mpay_b = s.full ? rup(te * sda::participant_mask_bytes_bound(s.shape) + 64) : 0;
        const size_t half = sec_b + pay_b + mpay_b;
        if (plan.tiles) {
            if (sda_status e = host_stream_ensure(h, half, 0)) return e;
            for (int b = 0; b < 2; ++b)
                if (!h->d2h_done[b]) HIP_TRY(hipEventCreateWithFlags(&h->d2h_done[b], hipEventDisableTiming));
        }
        for (int b = 0; b < 2; ++b) {
            hp[b] = static_cast<uint8_t*>(h->hs_pin) + b * rup(half);
            dv[b] = static_cast<uint8_t*>(h->hs_dev) + b * rup(half);
            row_bytes[b].assign(n + 1, 0);
        }
        const bool up = !s.chacha;
        if (up && plan.tiles)
            if (sda_status e = upload(0)) return e;
        for (uint64_t i = 0; i < plan.tiles; ++i) {
            // the other half's secrets: tile i - 1 has computed (every tile ends with the wait for its payload sizes)
            if (up && i + 1 < plan.tiles)
                if (sda_status e = upload(i + 1)) return e;
            if (sda_status e = compute(i)) return e;
            if (i >= 1)
                if (sda_status e = drain(i - 1)) return e;
        }
        return plan.tiles ? drain(plan.tiles - 1) : SDA_OK;
    }
    sda_status upload(uint64_t i) {
        const Tile t = tile(i);
        memcpy(hp[t.b], secrets + t.s0, t.ds * 8);
        HIP_TRY(hipMemcpyAsync(dv[t.b], hp[t.b], t.ds * 8, hipMemcpyHostToDevice, h->copy_stream));
        HIP_TRY(hipEventRecord(h->h2d_done[t.b], h->copy_stream));
        return SDA_OK;
    }
    // tile i: mask (unless the whole vector's was made), shares and payloads, and the payloads' copy down queued
    sda_status compute(uint64_t i) {
        const Tile ti = tile(i);
        const int b = ti.b;
        if (!s.chacha) HIP_TRY(hipStreamWaitEvent(h->stream, h->h2d_done[b], 0));
        ParticipantCall t = call;
        t.dimension = ti.ds, t.first = ti.u0;
        if (sda_status e = job_rows(h, s, ti.units, &t)) return e;
        // this half's payload buffers: tile i - 2 was drained while tile i - 1 computed
        uint8_t* dpay = dv[b] + sec_b;
        t.payload = dpay, t.payload_cap = pay_b, t.payload_row_bytes = row_bytes[b].data();
        const int64_t* masked = masked_all ? masked_all + ti.s0 : nullptr;
        if (!masked) {
            t.secrets = reinterpret_cast<const int64_t*>(dv[b]);
            MaskStep m;
            if (sda_status e = participant_mask(h, t, &m)) return e;
            masked = m.masked;
            mask_route = m.route;
        }
        if (sda_status e = participant_generate_encode(h, t, masked)) return e;
        mask_bytes[b] = 0;
        if (s.full && ti.ds)
            if (sda_status e = encode_full_mask(h, t, dpay + pay_b, mpay_b, &mask_bytes[b], "the mask payload's tile"))
                return e;
        // both encodes have been waited for: the copy stream may read the payloads now
        uint64_t total = 0;
        for (uint64_t c = 0; c < s.shape.n; ++c) total += row_bytes[b][c];
        if (total) HIP_TRY(hipMemcpyAsync(hp[b] + sec_b, dpay, total, hipMemcpyDeviceToHost, h->copy_stream));
        if (mask_bytes[b])
            HIP_TRY(hipMemcpyAsync(hp[b] + sec_b + pay_b, dpay + pay_b, mask_bytes[b], hipMemcpyDeviceToHost,
                                   h->copy_stream));
        HIP_TRY(hipEventRecord(h->d2h_done[b], h->copy_stream));
        return SDA_OK;
    }
    sda_status drain(uint64_t i) {                          // tile i's payloads: pinned memory -> the caller's blobs
        const int b = (int)(i & 1);
        HIP_TRY(hipEventSynchronize(h->d2h_done[b]));
        const uint8_t* src = hp[b] + sec_b;
        for (uint64_t c = 0; c < s.shape.n; ++c) {
            if (row_bytes[b][c]) memcpy(clerk_payloads[c] + lens[c], src, row_bytes[b][c]);
            lens[c] += row_bytes[b][c];
            src += row_bytes[b][c];
        }
        if (mask_bytes[b]) memcpy(mask_payload + mlen, hp[b] + sec_b + pay_b, mask_bytes[b]);
        mlen += mask_bytes[b];
        return SDA_OK;
    }
};

}  // namespace

extern "C" {

// participate.rs:53-76 (+ the encoding step of Encryptor::encrypt, sodium.rs:36-41) on device.
sda_status sda_participant_share_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                     uint64_t seed_words, const int64_t* full_masks, const sda_sharing_scheme* ss,
                                     const int64_t* secrets, uint64_t dimension, const int64_t* draws,
                                     int32_t mode, int64_t* shares_out, uint8_t* payload, uint64_t payload_cap,
                                     uint64_t* payload_row_bytes, void* stream) {
    SDA_ENTRY;
    ParticipantCall c{ms, ss, secrets, dimension, mode, nullptr, seed, seed_words, full_masks};
    c.draws = draws, c.shares64 = shares_out;
    c.payload = payload, c.payload_cap = payload_cap, c.payload_row_bytes = payload_row_bytes;
    return participant_share(h, c, stream);
}

// The same with the shares as int32 rows, from sda_packed_generate32_dev's kernels into the int32 encoder.
sda_status sda_participant_share32_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                       uint64_t seed_words, const int64_t* full_masks, const sda_sharing_scheme* ss,
                                       const int64_t* secrets, uint64_t dimension, const int64_t* draws, int32_t mode,
                                       int32_t* shares_out, uint8_t* payload, uint64_t payload_cap,
                                       uint64_t* payload_row_bytes, void* stream) {
    SDA_ENTRY;
    ParticipantCall c{ms, ss, secrets, dimension, mode, nullptr, seed, seed_words, full_masks};
    c.draws = draws, c.shares32 = shares_out;
    c.payload = payload, c.payload_cap = payload_cap, c.payload_row_bytes = payload_row_bytes;
    return participant_share(h, c, stream);
}

// The two calls above with the share-generation draws made on the device from (key, stream_id).
sda_status sda_participant_share_keyed_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                           uint64_t seed_words, const int64_t* full_masks,
                                           const sda_sharing_scheme* ss, const int64_t* secrets, uint64_t dimension,
                                           const uint32_t* key, uint32_t stream_id, int32_t mode, int64_t* shares_out,
                                           uint8_t* payload, uint64_t payload_cap, uint64_t* payload_row_bytes,
                                           void* stream) {
    SDA_ENTRY;
    ParticipantCall c{ms, ss, secrets, dimension, mode, nullptr, seed, seed_words, full_masks};
    c.keyed = true, c.key = key, c.stream_id = stream_id, c.shares64 = shares_out;
    c.payload = payload, c.payload_cap = payload_cap, c.payload_row_bytes = payload_row_bytes;
    return participant_share(h, c, stream);
}

sda_status sda_participant_share32_keyed_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                             uint64_t seed_words, const int64_t* full_masks,
                                             const sda_sharing_scheme* ss, const int64_t* secrets, uint64_t dimension,
                                             const uint32_t* key, uint32_t stream_id, int32_t mode,
                                             int32_t* shares_out, uint8_t* payload, uint64_t payload_cap,
                                             uint64_t* payload_row_bytes, void* stream) {
    SDA_ENTRY;
    ParticipantCall c{ms, ss, secrets, dimension, mode, nullptr, seed, seed_words, full_masks};
    c.keyed = true, c.key = key, c.stream_id = stream_id, c.shares32 = shares_out;
    c.payload = payload, c.payload_cap = payload_cap, c.payload_row_bytes = payload_row_bytes;
    return participant_share(h, c, stream);
}

// ---------------- participant job: mask, mask payload, shares and clerk payloads in one call ----------------
// participate.rs:53-98 without the sealing: the pipeline's steps with the Full mask drawn in the masking kernel, the
// shares in handle scratch and the recipient's mask payload encoded next to the clerks'.
sda_status sda_participant_job_payload_bound(const sda_masking_scheme* ms, const sda_sharing_scheme* ss,
                                             uint64_t dimension, uint64_t* clerk_row_bound, uint64_t* mask_bound) {
    SDA_ENTRY;
    if (!ms || !ss || !clerk_row_bound || !mask_bound) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    ParticipantJobSetup s;
    if (sda_status e = participant_job_setup(ms, ss, dimension, 0, 1, &s)) return e;
    *clerk_row_bound = s.row_bound;
    *mask_bound = s.mask_bound;
    return ok();
}

sda_status sda_participant_job_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                   uint64_t seed_words, const sda_sharing_scheme* ss, const int64_t* secrets,
                                   uint64_t dimension, const uint32_t* key, uint32_t mask_stream_id,
                                   uint32_t share_stream_id, int32_t mode, uint8_t* payload, uint64_t payload_cap,
                                   uint64_t* payload_row_bytes, uint8_t* mask_payload, uint64_t mask_payload_cap,
                                   uint64_t* mask_payload_len, void* stream) {
    SDA_ENTRY;
    const uint64_t D = dimension;
    if (!h || !ms || !ss || !key || !mask_payload_len || (ss->share_count && !payload_row_bytes) || (D && !secrets))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    ParticipantJobSetup s;
    if (sda_status e = participant_job_setup(ms, ss, D, mask_stream_id, share_stream_id, &s)) return e;
    const uint64_t n = ss->share_count;
    uint64_t all_rows;
    if (__builtin_mul_overflow(n, s.row_bound, &all_rows))
        return fail(SDA_ERR_INVALID_ARGUMENT, "the payload bound does not fit 64 bits");
    if (payload_cap < all_rows || mask_payload_cap < s.mask_bound) {
        for (uint64_t c = 0; c < n; ++c) payload_row_bytes[c] = s.row_bound;
        *mask_payload_len = s.mask_bound;
        return fail(SDA_ERR_INVALID_ARGUMENT, "payload_cap or mask_payload_cap is below the bound of "
                                              "sda_participant_job_payload_bound");
    }
    if ((all_rows && !payload) || (s.mask_bound && !mask_payload) || (s.chacha && seed_words && !seed))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick(h, stream);
    ParticipantCall c = job_call(s, ms, ss, mode, key, mask_stream_id, share_stream_id);
    c.secrets = secrets, c.dimension = D, c.seed = seed, c.seed_words = seed_words;
    c.payload = payload, c.payload_cap = payload_cap, c.payload_row_bytes = payload_row_bytes;
    if (sda_status e = job_rows(h, s, s.units, &c)) return e;
    RecordsGuard records(h);                                // a failing return below: every record stays the previous call's
    uint64_t mask_len = 0;
    if (sda_status e = participant_share(h, c, stream)) return e;
    if (s.chacha && seed_words != s.shape.seed_words)
        return fail(SDA_ERR_PRECONDITION, "expected %llu seed words", (unsigned long long)s.shape.seed_words);
    // the recipient's mask payload (participate.rs:56-72)
    if (s.full && D)
        if (sda_status e = encode_full_mask(h, c, mask_payload, mask_payload_cap, &mask_len, "mask_payload_cap")) return e;
    if (s.chacha && seed_words) {
        const std::vector<uint8_t> bytes = encode_seed_words(seed, seed_words);
        mask_len = bytes.size();
        hipError_t he = hipMemcpyAsync(mask_payload, bytes.data(), bytes.size(), hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);             // `bytes` goes out of scope
        if (he != hipSuccess) {
            (void)hipGetLastError();
            return fail(SDA_ERR_DEVICE, "the mask payload's copy failed: %s", hipGetErrorString(he));
        }
    }
    *mask_payload_len = mask_len;
    if (D) h->last.participant_job = {s.mask_route, h->last.participant.share_route, s.share_bytes, 1};
    records.keep();
    return ok();
}

sda_status sda_participant_job(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed, uint64_t seed_words,
                               const sda_sharing_scheme* ss, const int64_t* secrets, uint64_t dimension,
                               const uint32_t* key, uint32_t mask_stream_id, uint32_t share_stream_id, int32_t mode,
                               uint8_t* const* clerk_payloads, const uint64_t* clerk_caps, uint64_t* clerk_lens,
                               uint8_t* mask_payload, uint64_t mask_cap, uint64_t* mask_len) {
    SDA_ENTRY;
    const uint64_t D = dimension;
    if (!h || !ms || !ss || !key || !mask_len || (D && !secrets) ||
        (ss->share_count && (!clerk_payloads || !clerk_caps || !clerk_lens)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    ParticipantJobSetup s;
    if (sda_status e = participant_job_setup(ms, ss, D, mask_stream_id, share_stream_id, &s)) return e;
    const uint64_t n = ss->share_count;
    bool small = mask_cap < s.mask_bound;
    for (uint64_t c = 0; c < n; ++c) small = small || clerk_caps[c] < s.row_bound;
    if (small) {
        for (uint64_t c = 0; c < n; ++c) clerk_lens[c] = s.row_bound;
        *mask_len = s.mask_bound;
        return fail(SDA_ERR_INVALID_ARGUMENT, "a clerk_caps entry or mask_cap is below the bound of "
                                              "sda_participant_job_payload_bound");
    }
    if ((s.mask_bound && !mask_payload) || (s.chacha && seed_words && !seed))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint64_t c = 0; c < n; ++c)
        if (s.row_bound && !clerk_payloads[c])
            return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument (clerk payload %llu)", (unsigned long long)c);
    HIP_TRY(hipSetDevice(h->device));
    (void)pick(h, h->stream);
    RecordsGuard records(h);                    // a failing return below: every record stays the previous call's
    auto drained = [&](sda_status e) {          // and nothing of this call stays queued
        if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
        (void)hipStreamSynchronize(h->stream);
        return e;
    };
    ParticipantCall c = job_call(s, ms, ss, mode, key, mask_stream_id, share_stream_id);
    c.dimension = D, c.st = h->stream, c.seed = seed, c.seed_words = seed_words;
    // the checks once for every tile (the job's own rows pass the int32 rules by construction)
    if (s.chacha || D)
        if (sda_status e = participant_checks(c)) return e;
    uint64_t mlen = 0;
    // ChaCha: the masked secrets over the whole vector first, by the masking step (the rejection count is read here,
    // before the first tile); the tiles then share and encode them
    const int64_t* masked_all = nullptr;
    sda_engine::ParticipantLaunchInfo rec = {1, s.packed ? 4u : 2u, 1};
    if (s.chacha) {
        DevArena a;
        if (sda_status e = stage(h, rup(D * 8 + 8), &a)) return e;
        int64_t* dsec = a.take<int64_t>(D + 1);
        if (D) HIP_TRY(hipMemcpyAsync(dsec, secrets, D * 8, hipMemcpyHostToDevice, h->stream));
        c.secrets = dsec;
        MaskStep m;
        bool redone = false;
        if (sda_status e = participant_mask(h, c, &m)) return drained(e);
        if (sda_status e = participant_mask_settle(h, c, m, &redone)) return drained(e);
        if (seed_words != s.shape.seed_words)
            return drained(fail(SDA_ERR_PRECONDITION, "expected %llu seed words", (unsigned long long)s.shape.seed_words));
        masked_all = m.masked;
        rec.mask_route = m.route, rec.passes = redone ? 2 : 1;
        const std::vector<uint8_t> bytes = encode_seed_words(seed, seed_words);
        if (!bytes.empty()) memcpy(mask_payload, bytes.data(), bytes.size());
        mlen = bytes.size();
    }
    const char* ov = getenv("SDA_PARTICIPANT_TILE_BATCHES");
    const uint64_t override_units = ov && *ov && atoll(ov) > 0 ? (uint64_t)atoll(ov) : 0;
    JobTiles tiles{h, s, sda::participant_job_tiles(s.shape, D, s.share_bytes, host_stage_bytes(), override_units), c,
                   secrets, masked_all, clerk_payloads, mask_payload, std::vector<uint64_t>(n, 0), mlen};
    if (sda_status e = tiles.run()) return drained(e);
    for (uint64_t i = 0; i < n; ++i) clerk_lens[i] = tiles.lens[i];
    *mask_len = tiles.mlen;
    if (D) {
        if (!s.chacha) rec.mask_route = tiles.mask_route;
        h->last.participant = rec;
        h->last.participant_job = {s.mask_route, rec.share_route, s.share_bytes, tiles.plan.tiles};
    }
    if (sda_status e = finish(h)) return e;
    records.keep();
    return SDA_OK;
}

sda_status sda_participant_job_last_launch(sda_engine* h, uint32_t* mask_route, uint32_t* share_route,
                                           uint32_t* share_bytes, uint64_t* tiles) {
    SDA_ENTRY;
    if (!h || !mask_route || !share_route || !share_bytes || !tiles) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for
    const sda_engine::ParticipantJobLaunchInfo& r = h->last.participant_job;
    *mask_route = r.mask_route;
    *share_route = r.share_route;
    *share_bytes = r.share_bytes;
    *tiles = r.tiles;
    return ok();
}

}  // extern "C"
