// engine_check.cpp -- the packed-Shamir share consistency check's entry points (include/sda_engine.h):
// sda_packed_check_dev / sda_packed_check32_dev on device shares, sda_secret_check on host rows, and their record --
// and the checked reveal's on the same arguments plus `out`: sda_packed_reveal_checked_dev / 32, the host form
// sda_secret_reconstruct_checked and its record.  Argument checks follow the reveal entry points on the same
// arguments; the arithmetic is packed_check.hip's and packed_repair.hip's.
#include "engine_internal.h"

using namespace sda_host;

namespace {

// what a call hands back once it has succeeded (a failing call writes nothing)
struct CheckOutputs {
    uint64_t *redundancy, *bad_batches, *first_bad, *blame;
    uint64_t n_idx;
    void zero(uint64_t r) const {
        *redundancy = r;
        *bad_batches = 0;
        *first_bad = UINT64_MAX;
        for (uint64_t j = 0; j < n_idx; ++j) blame[j] = 0;
    }
};

uint32_t check_log_cap() {                                 // SDA_CHECK_LOG_CAP, read per call
    const char* e = getenv("SDA_CHECK_LOG_CAP");
    if (!e || !*e) return sda::kCheckLogCap;
    const unsigned long long v = strtoull(e, nullptr, 10);
    return v < sda::kCheckLogCap ? (uint32_t)v : sda::kCheckLogCap;
}

// SDA_OK with zero counts and nothing launched; a given device verdict buffer of `words` entries is zero-filled
sda_status nothing_to_check(const CheckOutputs& o, uint64_t r, uint16_t* verdict, uint64_t words, hipStream_t st) {
    if (verdict && words) {
        HIP_TRY(hipMemsetAsync(verdict, 0, words * sizeof(uint16_t), st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    o.zero(r);
    return SDA_OK;
}

// The check of a validated call (PackedShamir, n_idx >= k + t, at most 1023 shares and 65535 vectors) on stream st.
sda_status run_check(sda_engine* h, const sda_sharing_scheme* s, const sda::PackedCheckArgs& ca, const uint64_t* indices,
                     uint64_t n_idx, const CheckOutputs& o, hipStream_t st) {
    if (sda_status e = ensure(&h->chk_buf, &h->chk_buf_bytes, sda::packed_check_buf_bytes())) return e;
    const uint64_t k = s->secret_count, B = (ca.dimension + k - 1) / k;
    std::vector<uint64_t> blame(n_idx, 0);
    sda::PackedCheckResult res{};
    const hipError_t e = sda::launch_packed_check(ca, indices, (uint32_t)n_idx, (uint32_t)k,
                                                  (uint32_t)s->privacy_threshold, (uint32_t)s->modulus,
                                                  (uint32_t)s->omega_secrets, (uint32_t)s->omega_shares, h->chk_tab,
                                                  h->chk_buf, check_log_cap(), st, blame.data(), &res);
    if (e == hipErrorInvalidValue) return fail(SDA_ERR_UNSUPPORTED, "the share check needs distinct clerk indices");
    HIP_TRY(e);
    if (!res.launched) return nothing_to_check(o, res.plan.redundancy, ca.verdict, ca.n_vectors * B, st);
    *o.redundancy = res.plan.redundancy;
    *o.bad_batches = res.bad;
    *o.first_bad = res.first_bad;
    for (uint64_t j = 0; j < n_idx; ++j) o.blame[j] = blame[j];
    h->last.check.path = res.plan.path;
    h->last.check.bucket = res.plan.bucket;
    h->last.check.located = res.located;
    h->last.check.overflowed = res.overflowed ? 1 : 0;
    return SDA_OK;
}

// Both device entry points, T the share type: sda_packed_reconstruct_dev's checks in its order.
template <typename T>
sda_status packed_check(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension, const uint64_t* indices,
                        uint64_t n_idx, uint64_t n_vectors, const T* shares, uint16_t* verdict, const CheckOutputs& o,
                        void* stream) {
    if (!h || !s) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (!o.redundancy || !o.bad_batches || !o.first_bad || (n_idx && !o.blame))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (s->kind == SDA_SHARING_ADDITIVE) {                  // every share is needed: no redundancy to check
        if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
        HIP_TRY(hipSetDevice(h->device));
        if (sda_status e = nothing_to_check(o, 0, verdict, n_vectors * dimension, pick(h, stream))) return e;
        return ok();
    }
    if (s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (sda_status st = check_packed(s)) return st;
    const uint64_t kt = s->privacy_threshold + s->secret_count;
    if (dimension == 0) {                                   // batched.rs:77-81: no batch, no check
        o.zero(n_idx > kt ? n_idx - kt : 0);
        return ok();
    }
    if (n_idx < kt) return fail(SDA_ERR_NOT_ENOUGH_SHARES, "Not enough shares to reconstruct");
    if (n_idx > sda::kRevealMaxShares)
        return fail(SDA_ERR_UNSUPPORTED, "more than %u clerk shares per batch", sda::kRevealMaxShares);
    if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
    if (n_vectors && (!shares || !indices)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    if (n_vectors == 0) {
        o.zero(n_idx - kt);
        return ok();
    }
    sda::PackedCheckArgs ca{nullptr, nullptr, dimension, n_vectors, verdict};
    if constexpr (sizeof(T) == 4) ca.shares32 = shares; else ca.shares = shares;
    if (sda_status e = run_check(h, s, ca, indices, n_idx, o, pick(h, stream))) return e;
    return ok();
}

// The checked reveal of a validated call (PackedShamir, n_idx >= k + t, at most 1023 shares and 65535 vectors, at
// least one batch and one vector) on stream st, as packed_repair_plan decides it.
sda_status run_reveal_checked(sda_engine* h, const sda_sharing_scheme* s, const sda::PackedRepairArgs& ra,
                              const uint64_t* indices, uint64_t n_idx, const CheckOutputs& o, hipStream_t st) {
    if (sda_status e = ensure(&h->chk_buf, &h->chk_buf_bytes, sda::packed_check_buf_bytes())) return e;
    const uint32_t k = (uint32_t)s->secret_count, t = (uint32_t)s->privacy_threshold, p = (uint32_t)s->modulus;
    const uint32_t ws = (uint32_t)s->omega_secrets, wn = (uint32_t)s->omega_shares, n = (uint32_t)n_idx;
    const uint64_t words = ra.n_vectors * ((ra.dimension + k - 1) / k);
    const sda::PackedRepairPlan pl = sda::packed_repair_plan(n, k, t);
    const hipError_t te = sda::ensure_repair_table(h->rep_tab, indices, n, k, t, p, ws, wn);
    if (te == hipErrorInvalidValue) return fail(SDA_ERR_UNSUPPORTED, "the checked reveal needs distinct clerk indices");
    HIP_TRY(te);
    const uint32_t cap = check_log_cap();
    std::vector<uint64_t> blame(n_idx, 0);
    sda::PackedRepairResult res{0, UINT64_MAX, 0, false};
    // the verdict words the fix-up reads when the caller keeps none: zeros, then the located positions
    uint16_t* ver = ra.verdict;
    auto own_verdict = [&]() -> sda_status {
        if (ver) return SDA_OK;
        if (sda_status e = ensure(&h->rep_ver, &h->rep_ver_bytes, words * sizeof(uint16_t))) return e;
        ver = static_cast<uint16_t*>(h->rep_ver);
        HIP_TRY(hipMemsetAsync(ver, 0, words * sizeof(uint16_t), st));
        return SDA_OK;
    };
    if (pl.path == sda::kRepairFused) {
        HIP_TRY(sda::launch_packed_repair(ra, n, k, t, p, h->rep_tab, h->chk_buf, cap, st, &res));
        if (res.bad && pl.locate) {
            if (sda_status e = own_verdict()) return e;
            HIP_TRY(sda::launch_packed_repair_fix(ra, ver, n, k, t, p, h->rep_tab, h->chk_buf, cap, true, false, st,
                                                  blame.data(), &res));
        }
    } else {
        if (pl.redundancy) {                                // the share check locates in the same call: ahead of it
            if (sda_status e = own_verdict()) return e;
            const sda::PackedCheckArgs ca{ra.shares, ra.shares32, ra.dimension, ra.n_vectors, ver};
            sda::PackedCheckResult cr{};
            HIP_TRY(sda::launch_packed_check(ca, indices, n, k, t, p, ws, wn, h->chk_tab, h->chk_buf, cap, st,
                                             blame.data(), &cr));
            res.bad = cr.bad;
            res.first_bad = cr.first_bad;
        } else if (ra.verdict) {
            HIP_TRY(hipMemsetAsync(ra.verdict, 0, words * sizeof(uint16_t), st));
        }
        sda::PackedRevealArgs rv{ra.shares, ra.dimension, ra.n_vectors, ra.out};
        rv.shares32 = ra.shares32;
        if (sda_status e = packed_reveal(h, s, rv, indices, n_idx, SDA_REVEAL_CANONICAL, st)) return e;
        if (res.bad)
            HIP_TRY(sda::launch_packed_repair_fix(ra, ver, n, k, t, p, h->rep_tab, h->chk_buf, cap, false, true, st,
                                                  blame.data(), &res));
        else
            HIP_TRY(hipStreamSynchronize(st));
    }
    *o.redundancy = pl.redundancy;
    *o.bad_batches = res.bad;
    *o.first_bad = res.first_bad;
    for (uint64_t j = 0; j < n_idx; ++j) o.blame[j] = blame[j];
    h->last.repair.path = pl.path;
    h->last.repair.bucket = pl.bucket;
    h->last.repair.fixed = res.fixed;
    h->last.repair.overflowed = res.overflowed ? 1 : 0;
    return SDA_OK;
}

// Both device entry points of the checked reveal, T the share type: packed_check's checks in its order, `out` where
// the reveal checks it; an Additive scheme has nothing to correct and no packed reveal.
template <typename T>
sda_status packed_reveal_checked(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                 const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors, const T* shares,
                                 uint16_t* verdict, int64_t* out, const CheckOutputs& o, void* stream) {
    if (!h || !s) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (!o.redundancy || !o.bad_batches || !o.first_bad || (n_idx && !o.blame))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (s->kind == SDA_SHARING_ADDITIVE) return fail(SDA_ERR_UNSUPPORTED, "an Additive scheme has no checked reveal");
    if (s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (sda_status st = check_packed(s)) return st;
    const uint64_t kt = s->privacy_threshold + s->secret_count;
    if (dimension == 0) {                                   // batched.rs:77-81: no batch, no check
        o.zero(n_idx > kt ? n_idx - kt : 0);
        return ok();
    }
    if (n_idx < kt) return fail(SDA_ERR_NOT_ENOUGH_SHARES, "Not enough shares to reconstruct");
    if (n_idx > sda::kRevealMaxShares)
        return fail(SDA_ERR_UNSUPPORTED, "more than %u clerk shares per batch", sda::kRevealMaxShares);
    if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
    if (n_vectors && (!out || !shares || !indices)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    if (n_vectors == 0) {
        o.zero(n_idx - kt);
        return ok();
    }
    sda::PackedRepairArgs ra{nullptr, nullptr, dimension, n_vectors, verdict, out};
    if constexpr (sizeof(T) == 4) ra.shares32 = shares; else ra.shares = shares;
    if (sda_status e = run_reveal_checked(h, s, ra, indices, n_idx, o, pick(h, stream))) return e;
    return ok();
}

// sda_secret_reconstruct's checks of the host rows of a PackedShamir call with at least one batch, in its order.
sda_status check_host_rows(const sda_sharing_scheme* s, uint64_t B, const uint64_t* indices,
                           const int64_t* const* rows, const uint64_t* lens, uint64_t n_rows) {
    const uint64_t kt = s->privacy_threshold + s->secret_count;
    if (n_rows && (!rows || !lens || !indices)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    const bool enough = n_rows >= kt;
    for (uint64_t i = 0; i < n_rows; ++i)
        if (lens[i] < (enough ? B : 1))
            return fail(SDA_ERR_PRECONDITION, "index out of bounds: row %llu has %llu < %llu batches",
                        (unsigned long long)i, (unsigned long long)lens[i], (unsigned long long)(enough ? B : 1));
    if (!enough)
        return fail(SDA_ERR_NOT_ENOUGH_SHARES, "Not enough shares to reconstruct (%llu < %llu)",
                    (unsigned long long)n_rows, (unsigned long long)kt);
    if (n_rows > sda::kRevealMaxShares)
        return fail(SDA_ERR_UNSUPPORTED, "more than %u clerk shares per batch", sda::kRevealMaxShares);
    for (uint64_t i = 0; i < n_rows; ++i)
        if (!rows[i]) return fail(SDA_ERR_INVALID_ARGUMENT, "row %llu is NULL", (unsigned long long)i);
    return SDA_OK;
}

}  // namespace

extern "C" {

sda_status sda_packed_check_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors, const int64_t* shares,
                                void* verdict, uint64_t* redundancy, uint64_t* bad_batches, uint64_t* first_bad,
                                uint64_t* blame, void* stream) {
    SDA_ENTRY;
    return packed_check(h, s, dimension, indices, n_idx, n_vectors, shares, static_cast<uint16_t*>(verdict),
                        CheckOutputs{redundancy, bad_batches, first_bad, blame, n_idx}, stream);
}

sda_status sda_packed_check32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                  const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors, const int32_t* shares,
                                  void* verdict, uint64_t* redundancy, uint64_t* bad_batches, uint64_t* first_bad,
                                  uint64_t* blame, void* stream) {
    SDA_ENTRY;
    return packed_check(h, s, dimension, indices, n_idx, n_vectors, shares, static_cast<uint16_t*>(verdict),
                        CheckOutputs{redundancy, bad_batches, first_bad, blame, n_idx}, stream);
}

// sda_secret_reconstruct's checks in its order (no output buffer here), then the device form on the staged rows
sda_status sda_secret_check(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension, const uint64_t* indices,
                            const int64_t* const* rows, const uint64_t* lens, uint64_t n_rows, void* verdict,
                            uint64_t* redundancy, uint64_t* bad_batches, uint64_t* first_bad, uint64_t* blame) {
    SDA_ENTRY;
    if (!h || !s || !redundancy || !bad_batches || !first_bad || (n_rows && !blame))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    const CheckOutputs o{redundancy, bad_batches, first_bad, blame, n_rows};
    if (s->kind == SDA_SHARING_ADDITIVE) {
        // additive.rs:56-72 through combine_rows' checks: the dimension is row 0's length
        if (n_rows && (!rows || !lens)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
        const uint64_t dim = n_rows ? lens[0] : 0;
        int64_t m;
        if (dim && s->modulus == 0) return modulus_abs(s->modulus, &m);
        for (uint64_t i = 0; i < n_rows; ++i)
            if (lens[i] != dim) return fail(SDA_ERR_MISMATCHING_DIMENSION, "Mismatching dimension (row %llu has %llu elements, expected %llu)",
                                            (unsigned long long)i, (unsigned long long)lens[i], (unsigned long long)dim);
        if (dim && n_rows)
            if (sda_status st = modulus_abs(s->modulus, &m)) return st;
        if (verdict) memset(verdict, 0, dim * sizeof(uint16_t));
        o.zero(0);
        return ok();
    }
    if (s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    if (sda_status st = check_packed(s)) return st;
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t k = s->secret_count, kt = s->privacy_threshold + k;
    const uint64_t B = (dimension + k - 1) / k;             // batched.rs:77
    if (B == 0) {                                           // no batch => no error checks run
        o.zero(n_rows > kt ? n_rows - kt : 0);
        return ok();
    }
    if (sda_status st = check_host_rows(s, B, indices, rows, lens, n_rows)) return st;
    (void)pick(h, h->stream);                               // host entry points run on the engine's own stream
    DevArena a;
    if (sda_status e = stage(h, rup(n_rows * B * 8) + rup(B * 2), &a)) return e;
    int64_t* din = a.take<int64_t>(n_rows * B);
    uint16_t* dver = a.take<uint16_t>(B);
    for (uint64_t i = 0; i < n_rows; ++i)                   // batched.rs:83-85: clerk i's batches
        HIP_TRY(hipMemcpyAsync(din + i * B, rows[i], B * 8, hipMemcpyHostToDevice, h->stream));
    // the counts go to locals first: the verdict copy below may still fail
    uint64_t r = 0, bad = 0, first = UINT64_MAX;
    std::vector<uint64_t> bl(n_rows, 0);
    const CheckOutputs tmp{&r, &bad, &first, bl.data(), n_rows};
    const sda_engine::CheckLaunchInfo before = h->last.check;
    sda::PackedCheckArgs ca{din, nullptr, dimension, 1, verdict ? dver : nullptr};
    if (sda_status e = run_check(h, s, ca, indices, n_rows, tmp, h->stream)) return e;
    if (verdict) {
        std::vector<uint16_t> hv(B);
        hipError_t ce = hipMemcpyAsync(hv.data(), dver, B * 2, hipMemcpyDeviceToHost, h->stream);
        if (ce == hipSuccess) ce = hipStreamSynchronize(h->stream);
        if (ce != hipSuccess) h->last.check = before;
        HIP_TRY(ce);
        memcpy(verdict, hv.data(), B * 2);
    }
    *redundancy = r;
    *bad_batches = bad;
    *first_bad = first;
    for (uint64_t j = 0; j < n_rows; ++j) blame[j] = bl[j];
    return ok();
}

sda_status sda_packed_reveal_checked_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                         const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                         const int64_t* shares, int64_t* out, void* verdict, uint64_t* redundancy,
                                         uint64_t* bad_batches, uint64_t* first_bad, uint64_t* blame, void* stream) {
    SDA_ENTRY;
    return packed_reveal_checked(h, s, dimension, indices, n_idx, n_vectors, shares, static_cast<uint16_t*>(verdict),
                                 out, CheckOutputs{redundancy, bad_batches, first_bad, blame, n_idx}, stream);
}

sda_status sda_packed_reveal_checked32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                           const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                           const int32_t* shares, int64_t* out, void* verdict, uint64_t* redundancy,
                                           uint64_t* bad_batches, uint64_t* first_bad, uint64_t* blame,
                                           void* stream) {
    SDA_ENTRY;
    return packed_reveal_checked(h, s, dimension, indices, n_idx, n_vectors, shares, static_cast<uint16_t*>(verdict),
                                 out, CheckOutputs{redundancy, bad_batches, first_bad, blame, n_idx}, stream);
}

// sda_secret_check's checks in its order (out where sda_secret_reconstruct has its own), then the device form on the
// staged rows; everything reaches the caller's memory only once the call has succeeded
sda_status sda_secret_reconstruct_checked(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                          const uint64_t* indices, const int64_t* const* rows, const uint64_t* lens,
                                          uint64_t n_rows, void* verdict, uint64_t* redundancy, uint64_t* bad_batches,
                                          uint64_t* first_bad, uint64_t* blame, int64_t* out) {
    SDA_ENTRY;
    if (!h || !s || !redundancy || !bad_batches || !first_bad || (n_rows && !blame) || (dimension && !out))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    const CheckOutputs o{redundancy, bad_batches, first_bad, blame, n_rows};
    if (s->kind == SDA_SHARING_ADDITIVE) return fail(SDA_ERR_UNSUPPORTED, "an Additive scheme has no checked reveal");
    if (s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    if (sda_status st = check_packed(s)) return st;
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t k = s->secret_count, kt = s->privacy_threshold + k;
    const uint64_t B = (dimension + k - 1) / k;             // batched.rs:77
    if (B == 0) {                                           // no batch => no error checks run
        o.zero(n_rows > kt ? n_rows - kt : 0);
        return ok();
    }
    if (sda_status st = check_host_rows(s, B, indices, rows, lens, n_rows)) return st;
    (void)pick(h, h->stream);                               // host entry points run on the engine's own stream
    DevArena a;
    if (sda_status e = stage(h, rup(n_rows * B * 8) + rup(B * 2) + rup(dimension * 8), &a)) return e;
    int64_t* din = a.take<int64_t>(n_rows * B);
    uint16_t* dver = a.take<uint16_t>(B);
    int64_t* dout = a.take<int64_t>(dimension);
    for (uint64_t i = 0; i < n_rows; ++i)                   // batched.rs:83-85: clerk i's batches
        HIP_TRY(hipMemcpyAsync(din + i * B, rows[i], B * 8, hipMemcpyHostToDevice, h->stream));
    uint64_t r = 0, bad = 0, first = UINT64_MAX;
    std::vector<uint64_t> bl(n_rows, 0);
    const CheckOutputs tmp{&r, &bad, &first, bl.data(), n_rows};
    const sda_engine::RepairLaunchInfo before = h->last.repair;
    const sda::PackedRepairArgs ra{din, nullptr, dimension, 1, dver, dout};
    if (sda_status e = run_reveal_checked(h, s, ra, indices, n_rows, tmp, h->stream)) return e;
    std::vector<uint16_t> hv(B);
    std::vector<int64_t> ho(dimension);
    hipError_t ce = hipMemcpyAsync(hv.data(), dver, B * 2, hipMemcpyDeviceToHost, h->stream);
    if (ce == hipSuccess) ce = hipMemcpyAsync(ho.data(), dout, dimension * 8, hipMemcpyDeviceToHost, h->stream);
    if (ce == hipSuccess) ce = hipStreamSynchronize(h->stream);
    if (ce != hipSuccess) h->last.repair = before;
    HIP_TRY(ce);
    if (verdict) memcpy(verdict, hv.data(), B * 2);
    memcpy(out, ho.data(), dimension * 8);
    *redundancy = r;
    *bad_batches = bad;
    *first_bad = first;
    for (uint64_t j = 0; j < n_rows; ++j) blame[j] = bl[j];
    return ok();
}

sda_status sda_packed_reveal_checked_last_launch(sda_engine* h, uint32_t* path, uint32_t* bucket, uint64_t* fixed,
                                                 uint32_t* overflowed) {
    SDA_ENTRY;
    if (!h || !path || !bucket || !fixed || !overflowed) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *path = h->last.repair.path;
    *bucket = h->last.repair.bucket;
    *fixed = h->last.repair.fixed;
    *overflowed = h->last.repair.overflowed;
    return ok();
}

sda_status sda_packed_check_last_launch(sda_engine* h, uint32_t* path, uint32_t* bucket, uint64_t* located,
                                        uint32_t* overflowed) {
    SDA_ENTRY;
    if (!h || !path || !bucket || !located || !overflowed) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *path = h->last.check.path;
    *bucket = h->last.check.bucket;
    *located = h->last.check.located;
    *overflowed = h->last.check.overflowed;
    return ok();
}

}  // extern "C"
