// engine_check.cpp -- the packed-Shamir share consistency check's entry points (include/sda_engine.h):
// sda_packed_check_dev / sda_packed_check32_dev on device shares, sda_secret_check on host rows, and their record --
// and the checked reveal's on the same arguments plus `out`: sda_packed_reveal_checked_dev / 32, the host form
// sda_secret_reconstruct_checked and its record.  The two families share one argument front (validate), one host
// form (host_form) and one device table (sda::ensure_check_table); run_check and run_reveal_checked are the two
// algorithms, and the arithmetic is packed_check.hip's and packed_repair.hip's.
#include "engine_internal.h"

using namespace sda_host;

namespace {

// what a call hands back once it has succeeded (a failing call writes nothing)
struct CheckOutputs {
    uint64_t *redundancy, *bad_batches, *first_bad, *blame;
    uint64_t n_idx;
    bool complete() const { return redundancy && bad_batches && first_bad && (!n_idx || blame); }
    void commit(uint64_t r, const sda::PackedCheckResult& res, const uint64_t* bl) const {
        *redundancy = r;
        *bad_batches = res.bad;
        *first_bad = res.first_bad;
        for (uint64_t j = 0; j < n_idx; ++j) blame[j] = bl ? bl[j] : 0;
    }
    void zero(uint64_t r) const { commit(r, sda::PackedCheckResult{}, nullptr); }
};

// the counts of a run before they reach the caller: what follows the run may still fail
struct Counts {
    uint64_t redundancy = 0;
    sda::PackedCheckResult res;
    std::vector<uint64_t> blame;
    explicit Counts(uint64_t n_idx) : blame(n_idx, 0) {}
};

uint32_t check_log_cap() {                                 // SDA_CHECK_LOG_CAP, read per call
    const char* e = getenv("SDA_CHECK_LOG_CAP");
    if (!e || !*e) return sda::kCheckLogCap;
    const unsigned long long v = strtoull(e, nullptr, 10);
    return v < sda::kCheckLogCap ? (uint32_t)v : sda::kCheckLogCap;
}

// nothing to check and nothing launched: a given device verdict buffer of `words` entries is zero-filled
sda_status zero_verdict(uint16_t* verdict, uint64_t words, hipStream_t st) {
    if (verdict && words) {
        HIP_TRY(hipMemsetAsync(verdict, 0, words * sizeof(uint16_t), st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return SDA_OK;
}

// What both algorithms start from: the counter block, the (scheme, clerk set)'s table -- repeated clerk points are
// refused with the family's own message `repeated` -- and the geometry of the call's launches.
sda_status prepare(sda_engine* h, const sda_sharing_scheme* s, const sda::PackedCheckArgs& a, const uint64_t* indices,
                   uint64_t n_idx, const char* repeated, sda::CheckGeom* g) {
    if (sda_status e = ensure(&h->chk_buf, &h->chk_buf_bytes, sda::packed_check_buf_bytes())) return e;
    const uint32_t k = (uint32_t)s->secret_count, t = (uint32_t)s->privacy_threshold, p = (uint32_t)s->modulus;
    const hipError_t te = sda::ensure_check_table(h->chk_tab, indices, (uint32_t)n_idx, k, t, p,
                                                  (uint32_t)s->omega_secrets, (uint32_t)s->omega_shares);
    if (te == hipErrorInvalidValue) return fail(SDA_ERR_UNSUPPORTED, "%s", repeated);
    HIP_TRY(te);
    *g = sda::check_geom(a, (uint32_t)n_idx, k, t, p, h->chk_tab, h->chk_buf, check_log_cap());
    return SDA_OK;
}

// The check of a validated call (PackedShamir, n_idx >= k + t, at most 1023 shares and 65535 vectors, at least one
// batch and one vector) on stream st.
sda_status run_check(sda_engine* h, const sda_sharing_scheme* s, const sda::PackedCheckArgs& ca, const uint64_t* indices,
                     uint64_t n_idx, Counts* c, hipStream_t st) {
    sda::CheckGeom g;
    if (sda_status e = prepare(h, s, ca, indices, n_idx, "the share check needs distinct clerk indices", &g)) return e;
    const sda::PackedCheckPlan pl = sda::packed_check_plan(g.n_idx, g.k, g.kt - g.k);
    c->redundancy = pl.redundancy;
    HIP_TRY(sda::launch_packed_check(ca, g, st, c->blame.data(), &c->res));
    if (!c->res.launched) return zero_verdict(ca.verdict, ca.n_vectors * g.B, st);
    h->last.check.path = pl.path;
    h->last.check.bucket = pl.bucket;
    h->last.check.located = c->res.located;
    h->last.check.overflowed = c->res.overflowed ? 1 : 0;
    return SDA_OK;
}

// The checked reveal of a call validated as run_check's, on stream st, as packed_repair_plan decides it.
sda_status run_reveal_checked(sda_engine* h, const sda_sharing_scheme* s, const sda::PackedRepairArgs& ra,
                              const uint64_t* indices, uint64_t n_idx, Counts* c, hipStream_t st) {
    sda::CheckGeom g;
    if (sda_status e = prepare(h, s, ra, indices, n_idx, "the checked reveal needs distinct clerk indices", &g)) return e;
    const uint64_t words = ra.n_vectors * g.B;
    const sda::PackedRepairPlan pl = sda::packed_repair_plan(g.n_idx, g.k, g.kt - g.k);
    sda::PackedCheckResult& res = c->res;
    uint64_t* blame = c->blame.data();
    c->redundancy = pl.redundancy;
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
        HIP_TRY(sda::launch_packed_repair(ra, g, st, &res));
        if (res.bad && pl.locate) {
            if (sda_status e = own_verdict()) return e;
            HIP_TRY(sda::launch_packed_repair_fix(ra, ver, g, true, false, st, blame, &res));
        }
    } else {
        if (pl.redundancy) {                                // the share check locates in the same call: ahead of it
            if (sda_status e = own_verdict()) return e;
            sda::PackedCheckArgs ca = ra;
            ca.verdict = ver;
            HIP_TRY(sda::launch_packed_check(ca, g, st, blame, &res));
        } else if (ra.verdict) {
            HIP_TRY(hipMemsetAsync(ra.verdict, 0, words * sizeof(uint16_t), st));
        }
        sda::PackedRevealArgs rv{ra.shares, ra.dimension, ra.n_vectors, ra.out};
        rv.shares32 = ra.shares32;
        if (sda_status e = packed_reveal(h, s, rv, indices, n_idx, SDA_REVEAL_CANONICAL, st)) return e;
        if (res.bad)
            HIP_TRY(sda::launch_packed_repair_fix(ra, ver, g, false, true, st, blame, &res));
        else
            HIP_TRY(hipStreamSynchronize(st));
    }
    h->last.repair.path = pl.path;
    h->last.repair.bucket = pl.bucket;
    h->last.repair.fixed = res.fixed;
    h->last.repair.overflowed = res.overflowed ? 1 : 0;
    return SDA_OK;
}

// What a decoded reveal hands back beside the check's outputs.
struct DecodeExtra {
    uint64_t *radius, *undecoded;
    bool complete() const { return radius && undecoded; }
};

sda_status decode_scope(uint64_t n_idx, uint64_t k) {
    if (n_idx > sda::kDecodeMaxShares)
        return fail(SDA_ERR_UNSUPPORTED, "the decoded reveal takes at most %u clerk shares per batch", sda::kDecodeMaxShares);
    if (k > sda::kDecodeMaxK)
        return fail(SDA_ERR_UNSUPPORTED, "the decoded reveal takes at most %u secrets per batch", sda::kDecodeMaxK);
    return SDA_OK;
}

// The decoded reveal of a call validated as run_check's and inside decode_scope, on stream st, as packed_decode_plan
// decides it: the checked reveal's fused first pass, then the decode pass over what it logged.  wrong: device uint32
// [n_vectors][B] or nullptr.
// mask (device, `dimension` i64 values; the recipient pipeline's call, one vector of i64 rows): out holds
// (secret - mask) mod p instead of the secrets -- subtracted in the first pass's write-back, or, with `unfused`
// (scratch of `dimension` values), by launch_recipient_unmask behind the plain first pass.  The decode pass corrects a
// residue by a difference mod p, so it runs behind either as it is.
sda_status run_reveal_decoded(sda_engine* h, const sda_sharing_scheme* s, const sda::PackedRepairArgs& ra, uint32_t* wrong,
                              const uint64_t* indices, uint64_t n_idx, Counts* c, uint64_t* undecoded, hipStream_t st,
                              const int64_t* mask = nullptr, int64_t* unfused = nullptr) {
    sda::CheckGeom g;
    if (sda_status e = prepare(h, s, ra, indices, n_idx, "the decoded reveal needs distinct clerk indices", &g)) return e;
    const sda::PackedDecodePlan pl = sda::packed_decode_plan(g.n_idx, g.k, g.kt - g.k);
    if (pl.decode)
        HIP_TRY(sda::ensure_decode_table(h->dec_tab, indices, g.n_idx, g.k, g.kt - g.k, g.M.p, (uint32_t)s->omega_secrets,
                                         (uint32_t)s->omega_shares));
    sda::PackedCheckResult& res = c->res;
    sda::PackedDecodeResult dres;
    c->redundancy = pl.redundancy;
    if (wrong) HIP_TRY(hipMemsetAsync(wrong, 0, ra.n_vectors * g.B * sizeof(uint32_t), st));
    if (!mask) {
        HIP_TRY(sda::launch_packed_repair(ra, g, st, &res));
    } else if (!unfused) {
        HIP_TRY(sda::launch_recipient_repair(ra, mask, g, st, &res));
    } else {
        sda::PackedRepairArgs plain = ra;
        plain.out = unfused;
        HIP_TRY(sda::launch_packed_repair(plain, g, st, &res));
        HIP_TRY(sda::launch_recipient_unmask(unfused, mask, ra.dimension, g.M, ra.out, st));
    }
    const bool second = res.bad && pl.decode;
    if (second)
        HIP_TRY(sda::launch_packed_decode(ra, wrong, g, static_cast<const uint32_t*>(h->dec_tab.dev), st,
                                          c->blame.data(), &res, &dres));
    *undecoded = second ? dres.undecoded : res.bad;
    h->last.decode.path = second ? sda::kDecodeDecoded : sda::kDecodeFirstPass;
    h->last.decode.bucket = pl.bucket;
    h->last.decode.decoded = dres.decoded;
    h->last.decode.fixed = second ? res.fixed : 0;
    h->last.decode.max_errors = dres.max_errors;
    h->last.decode.overflowed = second && res.overflowed ? 1 : 0;
    return SDA_OK;
}

// The argument ladder of the four device entry points: sda_packed_reconstruct_dev's checks in its order.
// additive_clean: an Additive scheme needs every share, so it has no redundancy to check and the call is done with
// zero counts (the share check); otherwise it is refused (no packed reveal to correct).  need_out: `out` is checked
// where the reveal checks it.  *run: the call goes on to its algorithm; else the status returned is the call's.
sda_status validate(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension, const uint64_t* indices,
                    uint64_t n_idx, uint64_t n_vectors, const void* shares, uint16_t* verdict, bool additive_clean,
                    bool need_out, const int64_t* out, const CheckOutputs& o, void* stream, bool* run) {
    *run = false;
    if (!h || !s) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (!o.complete()) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (s->kind == SDA_SHARING_ADDITIVE) {
        if (!additive_clean) return fail(SDA_ERR_UNSUPPORTED, "an Additive scheme has no checked reveal");
        if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
        HIP_TRY(hipSetDevice(h->device));
        if (sda_status e = zero_verdict(verdict, n_vectors * dimension, pick(h, stream))) return e;
        o.zero(0);
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
    if (n_vectors && ((need_out && !out) || !shares || !indices)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    if (n_vectors == 0) {
        o.zero(n_idx - kt);
        return ok();
    }
    *run = true;
    return SDA_OK;
}

// The four device entry points, T the share type; out == nullptr: the share check, else the checked reveal.
template <typename T>
sda_status device_form(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension, const uint64_t* indices,
                       uint64_t n_idx, uint64_t n_vectors, const T* shares, void* verdict, bool reveal, int64_t* out,
                       const CheckOutputs& o, void* stream) {
    bool run;
    const sda_status vs = validate(h, s, dimension, indices, n_idx, n_vectors, shares, static_cast<uint16_t*>(verdict),
                                   !reveal, reveal, out, o, stream, &run);
    if (!run) return vs;
    sda::PackedRepairArgs ra{{nullptr, nullptr, dimension, n_vectors, static_cast<uint16_t*>(verdict)}, out};
    if constexpr (sizeof(T) == 4) ra.shares32 = shares; else ra.shares = shares;
    Counts c(n_idx);
    if (sda_status e = reveal ? run_reveal_checked(h, s, ra, indices, n_idx, &c, pick(h, stream))
                              : run_check(h, s, ra, indices, n_idx, &c, pick(h, stream)))
        return e;
    o.commit(c.redundancy, c.res, c.blame.data());
    return ok();
}

// Both device forms of the decoded reveal, T the share type: the checked reveal's ladder, then the decoder's scope.
template <typename T>
sda_status decoded_device_form(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension, const uint64_t* indices,
                               uint64_t n_idx, uint64_t n_vectors, const T* shares, int64_t* out, void* verdict,
                               void* wrong, const CheckOutputs& o, const DecodeExtra& x, void* stream) {
    if (h && s && !x.complete()) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (h && s && o.complete() && s->kind == SDA_SHARING_ADDITIVE)
        return fail(SDA_ERR_UNSUPPORTED, "an Additive scheme has no decoded reveal");
    bool run;
    const sda_status vs = validate(h, s, dimension, indices, n_idx, n_vectors, shares, static_cast<uint16_t*>(verdict),
                                   false, true, out, o, stream, &run);
    if (!run) {
        if (vs == SDA_OK) {                                 // no batch or no vector: zero counts
            *x.radius = *o.redundancy / 2;
            *x.undecoded = 0;
        }
        return vs;
    }
    if (sda_status e = decode_scope(n_idx, s->secret_count)) return e;
    if (wrong && (reinterpret_cast<uintptr_t>(wrong) & 3))
        return fail(SDA_ERR_INVALID_ARGUMENT, "wrong must be 4-byte aligned");
    sda::PackedRepairArgs ra{{nullptr, nullptr, dimension, n_vectors, static_cast<uint16_t*>(verdict)}, out};
    if constexpr (sizeof(T) == 4) ra.shares32 = shares; else ra.shares = shares;
    Counts c(n_idx);
    uint64_t undecoded = 0;
    if (sda_status e = run_reveal_decoded(h, s, ra, static_cast<uint32_t*>(wrong), indices, n_idx, &c, &undecoded,
                                          pick(h, stream)))
        return e;
    o.commit(c.redundancy, c.res, c.blame.data());
    *x.radius = c.redundancy / 2;
    *x.undecoded = undecoded;
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

// Both host forms from where the scheme is no Additive one: sda_secret_reconstruct's checks in its order, the rows
// staged (batched.rs:83-85: clerk i's batches) with B verdict words and `extra` more bytes behind them, then
// run(rows, verdict words, extra bytes, &counts) on the engine's own stream.  The verdict words come back when the
// caller keeps them or, with `verdict_always`, in any case; the extra bytes go to extra_out.  Everything reaches the
// caller's memory only once the call has succeeded, and a failing read-back puts `rec`, the family's launch record,
// back as it was before the run.
template <typename Rec, typename Run>
sda_status host_form(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension, const uint64_t* indices,
                     const int64_t* const* rows, const uint64_t* lens, uint64_t n_rows, void* verdict,
                     bool verdict_always, void* extra_out, size_t extra, Rec& rec, const CheckOutputs& o, Run run) {
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
    if (sda_status e = stage(h, rup(n_rows * B * 8) + rup(B * 2) + rup(extra), &a)) return e;
    int64_t* din = a.take<int64_t>(n_rows * B);
    uint16_t* dver = a.take<uint16_t>(B);
    char* dextra = a.take<char>(extra);
    for (uint64_t i = 0; i < n_rows; ++i)
        HIP_TRY(hipMemcpyAsync(din + i * B, rows[i], B * 8, hipMemcpyHostToDevice, h->stream));
    Counts c(n_rows);
    const Rec before = rec;
    const bool keep_verdict = verdict || verdict_always;
    if (sda_status e = run(din, keep_verdict ? dver : nullptr, dextra, &c)) return e;
    if (keep_verdict || extra) {
        std::vector<uint16_t> hv(B);
        std::vector<char> hx(extra);
        hipError_t ce = hipSuccess;
        if (keep_verdict) ce = hipMemcpyAsync(hv.data(), dver, B * 2, hipMemcpyDeviceToHost, h->stream);
        if (ce == hipSuccess && extra) ce = hipMemcpyAsync(hx.data(), dextra, extra, hipMemcpyDeviceToHost, h->stream);
        if (ce == hipSuccess) ce = hipStreamSynchronize(h->stream);
        if (ce != hipSuccess) rec = before;
        HIP_TRY(ce);
        if (verdict) memcpy(verdict, hv.data(), B * 2);
        if (extra) memcpy(extra_out, hx.data(), extra);
    }
    o.commit(c.redundancy, c.res, c.blame.data());
    return ok();
}

}  // namespace

sda_status sda_host::reveal_decoded_masked(sda_engine* h, const sda_sharing_scheme* s, const sda::PackedRepairArgs& ra,
                                           const int64_t* mask, int64_t* unfused, const uint64_t* indices,
                                           uint64_t n_idx, DecodedReveal* d, hipStream_t st) {
    Counts c(n_idx);
    uint64_t undecoded = 0;
    if (sda_status e = run_reveal_decoded(h, s, ra, d->wrong, indices, n_idx, &c, &undecoded, st, mask, unfused)) return e;
    d->redundancy = c.redundancy;
    d->bad_batches = c.res.bad;
    d->first_bad = c.res.first_bad;
    d->undecoded = undecoded;
    d->blame = c.blame;
    return SDA_OK;
}

extern "C" {

sda_status sda_packed_check_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors, const int64_t* shares,
                                void* verdict, uint64_t* redundancy, uint64_t* bad_batches, uint64_t* first_bad,
                                uint64_t* blame, void* stream) {
    SDA_ENTRY;
    return device_form(h, s, dimension, indices, n_idx, n_vectors, shares, verdict, false, nullptr,
                       CheckOutputs{redundancy, bad_batches, first_bad, blame, n_idx}, stream);
}

sda_status sda_packed_check32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                  const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors, const int32_t* shares,
                                  void* verdict, uint64_t* redundancy, uint64_t* bad_batches, uint64_t* first_bad,
                                  uint64_t* blame, void* stream) {
    SDA_ENTRY;
    return device_form(h, s, dimension, indices, n_idx, n_vectors, shares, verdict, false, nullptr,
                       CheckOutputs{redundancy, bad_batches, first_bad, blame, n_idx}, stream);
}

// An Additive scheme's rows are checked as sda_secret_reconstruct checks them; the rest is host_form's
sda_status sda_secret_check(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension, const uint64_t* indices,
                            const int64_t* const* rows, const uint64_t* lens, uint64_t n_rows, void* verdict,
                            uint64_t* redundancy, uint64_t* bad_batches, uint64_t* first_bad, uint64_t* blame) {
    SDA_ENTRY;
    const CheckOutputs o{redundancy, bad_batches, first_bad, blame, n_rows};
    if (!h || !s || !o.complete()) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
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
    return host_form(h, s, dimension, indices, rows, lens, n_rows, verdict, false, nullptr, 0, h->last.check, o,
                     [&](const int64_t* din, uint16_t* dver, char*, Counts* c) {
                         const sda::PackedCheckArgs ca{din, nullptr, dimension, 1, dver};
                         return run_check(h, s, ca, indices, n_rows, c, h->stream);
                     });
}

sda_status sda_packed_reveal_checked_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                         const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                         const int64_t* shares, int64_t* out, void* verdict, uint64_t* redundancy,
                                         uint64_t* bad_batches, uint64_t* first_bad, uint64_t* blame, void* stream) {
    SDA_ENTRY;
    return device_form(h, s, dimension, indices, n_idx, n_vectors, shares, verdict, true, out,
                       CheckOutputs{redundancy, bad_batches, first_bad, blame, n_idx}, stream);
}

sda_status sda_packed_reveal_checked32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                           const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                           const int32_t* shares, int64_t* out, void* verdict, uint64_t* redundancy,
                                           uint64_t* bad_batches, uint64_t* first_bad, uint64_t* blame,
                                           void* stream) {
    SDA_ENTRY;
    return device_form(h, s, dimension, indices, n_idx, n_vectors, shares, verdict, true, out,
                       CheckOutputs{redundancy, bad_batches, first_bad, blame, n_idx}, stream);
}

// `out` is checked where sda_secret_reconstruct has its own check; an Additive scheme has no packed reveal to correct
sda_status sda_secret_reconstruct_checked(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                          const uint64_t* indices, const int64_t* const* rows, const uint64_t* lens,
                                          uint64_t n_rows, void* verdict, uint64_t* redundancy, uint64_t* bad_batches,
                                          uint64_t* first_bad, uint64_t* blame, int64_t* out) {
    SDA_ENTRY;
    const CheckOutputs o{redundancy, bad_batches, first_bad, blame, n_rows};
    if (!h || !s || !o.complete() || (dimension && !out)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (s->kind == SDA_SHARING_ADDITIVE) return fail(SDA_ERR_UNSUPPORTED, "an Additive scheme has no checked reveal");
    return host_form(h, s, dimension, indices, rows, lens, n_rows, verdict, true, out, dimension * 8, h->last.repair, o,
                     [&](const int64_t* din, uint16_t* dver, char* dout, Counts* c) {
                         const sda::PackedRepairArgs ra{{din, nullptr, dimension, 1, dver},
                                                        reinterpret_cast<int64_t*>(dout)};
                         return run_reveal_checked(h, s, ra, indices, n_rows, c, h->stream);
                     });
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

sda_status sda_packed_reveal_decoded_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                         const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                         const int64_t* shares, int64_t* out, void* verdict, void* wrong,
                                         uint64_t* redundancy, uint64_t* radius, uint64_t* bad_batches,
                                         uint64_t* first_bad, uint64_t* undecoded, uint64_t* blame, void* stream) {
    SDA_ENTRY;
    return decoded_device_form(h, s, dimension, indices, n_idx, n_vectors, shares, out, verdict, wrong,
                               CheckOutputs{redundancy, bad_batches, first_bad, blame, n_idx},
                               DecodeExtra{radius, undecoded}, stream);
}

sda_status sda_packed_reveal_decoded32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                           const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                           const int32_t* shares, int64_t* out, void* verdict, void* wrong,
                                           uint64_t* redundancy, uint64_t* radius, uint64_t* bad_batches,
                                           uint64_t* first_bad, uint64_t* undecoded, uint64_t* blame, void* stream) {
    SDA_ENTRY;
    return decoded_device_form(h, s, dimension, indices, n_idx, n_vectors, shares, out, verdict, wrong,
                               CheckOutputs{redundancy, bad_batches, first_bad, blame, n_idx},
                               DecodeExtra{radius, undecoded}, stream);
}

// sda_secret_reconstruct_checked's front; the B `wrong` words travel behind `out` in host_form's extra bytes
sda_status sda_secret_reconstruct_decoded(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                          const uint64_t* indices, const int64_t* const* rows, const uint64_t* lens,
                                          uint64_t n_rows, void* verdict, void* wrong, uint64_t* redundancy,
                                          uint64_t* radius, uint64_t* bad_batches, uint64_t* first_bad,
                                          uint64_t* undecoded, uint64_t* blame, int64_t* out) {
    SDA_ENTRY;
    const CheckOutputs o{redundancy, bad_batches, first_bad, blame, n_rows};
    if (!h || !s || !o.complete() || !radius || !undecoded || (dimension && !out))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (s->kind == SDA_SHARING_ADDITIVE) return fail(SDA_ERR_UNSUPPORTED, "an Additive scheme has no decoded reveal");
    const uint64_t k = s->secret_count ? s->secret_count : 1, B = (dimension + k - 1) / k;
    const size_t out_bytes = rup(dimension * 8), extra = out_bytes + (wrong ? B * 4 : 0);
    std::vector<char> back(extra);
    uint64_t und = 0;
    const sda_status st =
        host_form(h, s, dimension, indices, rows, lens, n_rows, verdict, false, back.data(), extra, h->last.decode, o,
                  [&](const int64_t* din, uint16_t* dver, char* dextra, Counts* c) {
                      if (sda_status e = decode_scope(n_rows, s->secret_count)) return e;
                      const sda::PackedRepairArgs ra{{din, nullptr, dimension, 1, dver},
                                                     reinterpret_cast<int64_t*>(dextra)};
                      return run_reveal_decoded(h, s, ra, wrong ? reinterpret_cast<uint32_t*>(dextra + out_bytes) : nullptr,
                                                indices, n_rows, c, &und, h->stream);
                  });
    if (st != SDA_OK) return st;
    if (extra) {
        memcpy(out, back.data(), dimension * 8);
        if (wrong) memcpy(wrong, back.data() + out_bytes, B * 4);
    }
    *radius = *redundancy / 2;
    *undecoded = und;
    return st;
}

sda_status sda_packed_decode_last_launch(sda_engine* h, uint32_t* path, uint32_t* bucket, uint64_t* decoded,
                                         uint64_t* fixed, uint32_t* max_errors, uint32_t* overflowed) {
    SDA_ENTRY;
    if (!h || !path || !bucket || !decoded || !fixed || !max_errors || !overflowed)
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *path = h->last.decode.path;
    *bucket = h->last.decode.bucket;
    *decoded = h->last.decode.decoded;
    *fixed = h->last.decode.fixed;
    *max_errors = h->last.decode.max_errors;
    *overflowed = h->last.decode.overflowed;
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
