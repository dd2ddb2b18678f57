// engine_recipient.cpp -- the fused recipient pipeline of the C ABI (include/sda_engine.h):
// sda_recipient_reveal and the recipient job, on device-resident inputs and on host ones, and the robust forms of
// both, which reveal with the decoded reveal (engine_check.cpp) and unmask in its write-back.
#include "engine_internal.h"

using namespace sda_host;

namespace {

// `%= modulus` over len values (full.rs:45, additive.rs:67): with a value to fold, a modulus of 0 panics.
sda_status fold_checks(uint64_t len, int64_t modulus) {
    int64_t m;
    return len ? modulus_abs(modulus, &m) : SDA_OK;
}

// The mask combine of receive.rs:101-117 over n_masks rows of mask_width values: its panics, and *mask_len, the
// length of the mask it returns.  The host form runs it before its own share-shape checks (the reference combines
// the masks before it reconstructs), the pipeline as its first step.
sda_status mask_combine_checks(const sda_masking_scheme* ms, uint64_t n_masks, uint64_t mask_width,
                               uint64_t* mask_len) {
    *mask_len = 0;
    if (ms->kind == SDA_MASKING_NONE) {
        if (n_masks && mask_width) return fail(SDA_ERR_PRECONDITION, "assertion failed: masks.iter().all(|mask| mask.len() == 0)");
    } else if (ms->kind == SDA_MASKING_FULL) {
        *mask_len = n_masks ? mask_width : 0;               // full.rs:38-40
        if (sda_status e = fold_checks(*mask_len, ms->modulus)) return e;
    } else if (ms->kind == SDA_MASKING_CHACHA) {
        *mask_len = ms->dimension;                          // chacha.rs:58
        if (mask_width == 0 || mask_width > 8) return fail(SDA_ERR_UNSUPPORTED, "device seeds must be 1..8 words");
        if (*mask_len && n_masks && ms->modulus <= 0)       // chacha.rs:69 gen_range(0, m)
            return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    } else {
        return fail(SDA_ERR_INVALID_ARGUMENT, "unknown masking scheme kind");
    }
    return SDA_OK;
}

// None masking on host rows or blobs (none.rs:23): every mask must be empty.
sda_status no_mask_checks(const uint64_t* mask_lens, uint64_t n_masks) {
    for (uint64_t i = 0; i < n_masks; ++i)
        if (mask_lens[i]) return fail(SDA_ERR_PRECONDITION, "assertion failed: masks.iter().all(|mask| mask.len() == 0)");
    return SDA_OK;
}

// Where a recipient call's masks come from, stated once: a tag and the fields that belong to it.
struct MaskSource {
    enum Kind {
        kRows,        // rows: [n][width] on the device, Full i64 values or ChaCha seed words
        kReady,       // Full: rows is the folded mask, one row of `width` values used as it is
        kSeedBlobs    // ChaCha: the n seed blobs (seed_bytes, seed_off) to decode, width = sda::kSeedWords
    } kind = kRows;
    uint64_t n = 0, width = 0;
    const void* rows = nullptr;
    const uint8_t* seed_bytes = nullptr;
    const uint64_t* seed_off = nullptr;
    // the one Full row is the ChaCha mask a multi-device handle combined (combine_mask_multi): recorded as mask_kind 4
    bool multi_combined = false;
};
// Where its clerk results come from.
struct ShareSource {
    enum Kind {
        kRows,        // rows: [n_idx][len] i64 on the device
        kBlobs        // the n_idx payloads (bytes, off), laid out as sda_clerk_decode_combine_dev takes them; what they
                      // decode to tells the share length (n_idx may be 0)
    } kind = kRows;
    const int64_t* rows = nullptr;
    uint64_t len = 0;
    const uint8_t* bytes = nullptr;
    const uint64_t* off = nullptr;
};
// One recipient call (receive.rs:80-157 + :14-20): the schemes, the output and the two sources.
struct RecipientCall {
    sda_masking_scheme ms;
    const sda_sharing_scheme* ss;
    uint64_t dimension;
    const uint64_t* indices;
    uint64_t n_idx;
    int64_t output_modulus;
    int32_t mode;
    int64_t* out;                   // device
    uint64_t out_cap;
    hipStream_t st;
    MaskSource mask;
    ShareSource shares;
    // a robust call (sda_recipient_*_decoded*): the packed branch reveals with the decoded reveal into `out` itself and
    // leaves its counts here; `mode` is not read
    DecodedReveal* dec = nullptr;
};

// A pipeline call that returned SDA_OK: its output length, and the record the caller commits when its call succeeds.
struct RecipientDone {
    uint64_t len = 0;
    sda_engine::RecipientLaunchInfo rec;
    sda_engine::RecipientDecodedLaunchInfo dec;             // a robust call's own record
};

// Scratch in h->pipe: [mask | masked | compacted shares], carved once per call -- before the clerk payloads of an
// Additive scheme are decoded into `masked`, whose length is then bounded by blob 0's bytes only, else once the output
// length is known.
struct PipeScratch {
    int64_t *mask = nullptr, *masked = nullptr, *compact = nullptr;
    sda_status carve(sda_engine* h, uint64_t masked_cap, uint64_t mask_cap, uint64_t compact_bytes) {
        if (sda_status e = ensure(&h->pipe, &h->pipe_bytes, rup(mask_cap * 8) + rup(masked_cap * 8) + rup(compact_bytes) + 256))
            return e;
        mask = static_cast<int64_t*>(h->pipe);
        masked = mask + rup(mask_cap * 8) / 8;
        compact = masked + rup(masked_cap * 8) / 8;
        return SDA_OK;
    }
};

// A multi-device handle spreads the ChaCha mask combine (receive.rs:113-116, the dominant cost at configs[4]) over its
// devices -- seeds split, one RCCL reduce onto device 0 (engine_host.cpp) -- and runs the rest of the pipeline on
// device 0 with the combined mask as one Full mask row: (0 + c) % m = c for the canonical c, so the unmask sees the
// same mask.  Only where the reference would not panic in the mask combine (m > 0).
bool multi_mask(const sda_engine* h, const sda_masking_scheme* ms, uint64_t n_masks) {
    return ms->kind == SDA_MASKING_CHACHA && is_multi(h) && n_masks && ms->dimension && ms->modulus > 0;
}
// `seeds`: the [n_masks][w] key words on the host.  Leaves the combined row in h->hs_dev and makes it c's mask.
sda_status combine_mask_multi(sda_engine* h, const std::vector<uint32_t>& seeds, uint32_t w, uint64_t n_masks,
                              RecipientCall* c) {
    const uint64_t D = c->ms.dimension;
    if (sda_status e = host_stream_ensure(h, 0, D * 8)) return e;
    if (sda_status e = chacha_combine_multi(h, c->ms.modulus, D, seeds, w, n_masks, static_cast<int64_t*>(h->hs_dev)))
        return e;
    c->ms = {SDA_MASKING_FULL, c->ms.modulus, 0, 0};
    c->mask = {MaskSource::kRows, 1, D, h->hs_dev, nullptr, nullptr, true};
    return SDA_OK;
}

// receive.rs:80-157 + :14-20 on the sources `c` names.
sda_status recipient_pipeline(sda_engine* h, const RecipientCall& c, RecipientDone* done) {
    const sda_masking_scheme* ms = &c.ms;
    const sda_sharing_scheme* ss = c.ss;
    const uint64_t n_idx = c.n_idx, dimension = c.dimension;
    const bool blobs = c.shares.kind == ShareSource::kBlobs;
    hipStream_t st = c.st;
    *done = RecipientDone();
    PipeScratch sc;
    // Checks in the reference's order: mask combine (receive.rs:101-117), reconstruct (:120-146), unmask (:149-152).
    // ---- 1. mask combine: its length and panics ----
    uint64_t mask_len = 0;
    if (sda_status e = mask_combine_checks(ms, c.mask.n, c.mask.width, &mask_len)) return e;
    // ChaCha seed payloads: the key words of every seed, zero padded, decoded into handle scratch.  Queued here, in
    // front of the wait the clerk results' lengths take, so that the offsets' copy and the kernel hide under it and
    // the mask combine finds its seeds ready.
    const uint32_t* seeds = c.mask.kind == MaskSource::kRows ? static_cast<const uint32_t*>(c.mask.rows) : nullptr;
    if (c.mask.kind == MaskSource::kSeedBlobs && c.mask.n && ms->kind == SDA_MASKING_CHACHA && mask_len) {
        const size_t words = rup(c.mask.n * sda::kSeedWords * 4);
        if (sda_status e = ensure(&h->job_work, &h->job_work_bytes, words + rup((c.mask.n + 1) * 8))) return e;
        uint32_t* dseeds = static_cast<uint32_t*>(h->job_work);
        HIP_TRY(sda::launch_recipient_seeds(c.mask.seed_bytes, c.mask.seed_off, c.mask.n,
                                            reinterpret_cast<uint64_t*>(static_cast<char*>(h->job_work) + words),
                                            dseeds, st));
        seeds = dseeds;
    }
    // ---- 2. reconstruct: masked output length and errors ----
    uint64_t D;
    uint64_t share_len = c.shares.len, stride = c.shares.len;  // stride: of the i64 clerk rows the packed reveal reads
    sda::VarintPlan plan;                                    // PackedShamir clerk payloads: the count pass's plan
    bool irregular = false;
    if (ss->kind == SDA_SHARING_ADDITIVE && blobs) {
        // additive.rs:56-72 is combiner.rs:16-28: the clerk's decode -> combine writes `masked`, and its one wait
        // tells the length.  Row 0 is folded (`%= modulus`, additive.rs:66-67) before :64 reads a later row's length.
        const uint64_t cap = n_idx ? c.shares.off[1] - c.shares.off[0] : 0;             // one value per byte at most
        if (sda_status e = fold_checks(cap, ss->modulus)) return e;
        const bool own_mask = ms->kind != SDA_MASKING_NONE && c.mask.kind != MaskSource::kReady;
        if (sda_status e = sc.carve(h, cap, own_mask ? std::min(mask_len, cap) : 0, 0)) return e;
        if (sda_status e = decode_combine(h, ss->modulus, c.shares.bytes, c.shares.off, n_idx, sc.masked, cap, &D, st))
            return e == SDA_ERR_WRONG_DIMENSION ? fail(SDA_ERR_MISMATCHING_DIMENSION, "Mismatching dimension") : e;
    } else if (ss->kind == SDA_SHARING_ADDITIVE) {
        D = n_idx ? share_len : 0;                           // additive.rs:56-60
        if (sda_status e = fold_checks(D, ss->modulus)) return e;
    } else if (ss->kind == SDA_SHARING_PACKED_SHAMIR) {
        if (sda_status e = check_packed(ss)) return e;
        if (!c.dec && c.mode != SDA_REVEAL_EXACT && c.mode != SDA_REVEAL_CANONICAL)
            return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
        const uint64_t B = (dimension + ss->secret_count - 1) / ss->secret_count;
        if (blobs) {
            // the count pass's one wait supplies the lengths of the reference's checks: ragged rows are read over
            // [0, B) (batched.rs:83-85), so the shortest decides, and the longest is the rows' stride
            share_len = stride = 0;
            if (B && n_idx) {
                std::vector<uint64_t> counts(n_idx);
                if (sda_status e = codec_count(h, c.shares.bytes, c.shares.off, n_idx, &plan, counts.data(), &irregular, st))
                    return e;
                share_len = *std::min_element(counts.begin(), counts.end());
                stride = *std::max_element(counts.begin(), counts.end());
            }
        }
        if (B) {                                             // batched.rs:77-81: no batch => no check
            const bool enough = n_idx >= ss->privacy_threshold + ss->secret_count;
            if (n_idx && share_len < (enough ? B : 1))      // batched.rs:84 indexes [batch_index]
                return fail(SDA_ERR_PRECONDITION, "index out of bounds: clerk vector shorter than the batch count");
            if (!enough) return fail(SDA_ERR_NOT_ENOUGH_SHARES, "Not enough shares to reconstruct");  // packed_shamir.rs:75
            if (n_idx > sda::kRevealMaxShares)
                return fail(SDA_ERR_UNSUPPORTED, "more than %u clerk shares per batch", sda::kRevealMaxShares);
            if (c.dec && n_idx > sda::kDecodeMaxShares)
                return fail(SDA_ERR_UNSUPPORTED, "the decoded reveal takes at most %u clerk shares per batch",
                            sda::kDecodeMaxShares);
        }
        D = dimension;
    } else {
        return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    }
    // ---- 3. unmask ----
    if (ms->kind != SDA_MASKING_NONE && mask_len != D)     // chacha.rs:83 / full.rs:58 assert_eq!
        return fail(SDA_ERR_PRECONDITION, "assertion failed: mask.len() == masked_secrets.len() (%llu vs %llu)",
                    (unsigned long long)mask_len, (unsigned long long)D);
    if (c.out_cap < D) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    if (D == 0) return ok();
    int64_t q = 1;
    if (ms->kind != SDA_MASKING_NONE)
        if (sda_status e = modulus_abs(ms->modulus, &q)) return e;
    const bool packed = ss->kind == SDA_SHARING_PACKED_SHAMIR;
    const uint64_t B = packed ? (dimension + ss->secret_count - 1) / ss->secret_count : 0;
    const bool compact = packed && stride != B;
    // A robust call writes c.out from the reveal itself; only its unfused route (SDA_RECIPIENT_FUSE_UNMASK=0, read
    // per call) parks the secrets in `masked` first.
    const char* fuse = getenv("SDA_RECIPIENT_FUSE_UNMASK");
    const bool masked_call = ms->kind != SDA_MASKING_NONE;
    const bool unfused = c.dec && masked_call && fuse && strcmp(fuse, "0") == 0;
    if (!sc.masked)                                         // (a payload job's Additive reconstruction has run)
        if (sda_status e = sc.carve(h, c.dec && !unfused ? 0 : D, D, compact ? n_idx * B * 8 : 0)) return e;
    sda_engine::RecipientLaunchInfo& rec = done->rec;
    rec.mask_kind = c.mask.multi_combined ? 4 : ms->kind == SDA_MASKING_NONE ? 1 : ms->kind == SDA_MASKING_FULL ? 2 : 3;
    rec.compact = compact;
    rec.unmask_launches = 1;
    // 1. masks (receive.rs:101-117)
    const int64_t* mask = sc.mask;
    if (ms->kind == SDA_MASKING_FULL && c.mask.kind == MaskSource::kReady) {
        mask = static_cast<const int64_t*>(c.mask.rows);    // folded by the caller: (0 + c) % m = c
    } else if (ms->kind == SDA_MASKING_FULL) {
        if (sda_status e = modulus_abs(ms->modulus, &q)) return e;
        HIP_TRY(sda::launch_combine_exact(static_cast<const int64_t*>(c.mask.rows), c.mask.n, D, c.mask.width, sc.mask,
                                          q, st, false, &h->last.combine));
    }
    PendingChacha pc;                                       // ChaCha: its rejection count is checked at the end
    if (ms->kind == SDA_MASKING_CHACHA)
        if (sda_status e = chacha_combine_begin(h, ms->modulus, D, seeds, (uint32_t)c.mask.width, c.mask.n, sc.mask, st, &pc))
            return e;
    // 2. reconstruct (receive.rs:120-146)
    if (!packed && !blobs) {
        int64_t m;
        if (sda_status e = modulus_abs(ss->modulus, &m)) return e;
        HIP_TRY(sda::launch_combine_exact(c.shares.rows, n_idx, D, share_len, sc.masked, m, st, false, &h->last.combine));
    } else if (packed) {
        const int64_t* rows = c.shares.rows;
        if (blobs) {                                        // i64 rows of the longest blob's length in handle scratch
            if (sda_status e = ensure(&h->codec_mat, &h->codec_mat_bytes, n_idx * stride * 8 + 8)) return e;
            int64_t* decoded = static_cast<int64_t*>(h->codec_mat);
            HIP_TRY(sda::launch_varint_decode(c.shares.bytes, n_idx, plan, h->codec_work, decoded, stride, stride,
                                              irregular, st));
            rows = decoded;
        }
        if (compact) {                                      // batched.rs:83-85 reads [clerk][0..B)
            HIP_TRY(hipMemcpy2DAsync(sc.compact, B * 8, rows, stride * 8, B * 8, n_idx, hipMemcpyDeviceToDevice, st));
            rows = sc.compact;
        }
        if (c.dec) {
            // The decoded reveal (engine_check.cpp) in place of the packed reveal, the mask subtracted in its first
            // pass's write-back: the scope checks have made both moduli the sharing prime, so the output is the one
            // residue (secret - mask) mod p, and the decode pass's correction mod p commutes with that subtraction.
            // The mask combine is queued ahead on the same stream.  A ChaCha mask that turns out to have had rejected
            // draws is fixed (chacha_combine_end) and the reveal passes run again over the same inputs.
            const sda::PackedRepairArgs da{{rows, nullptr, dimension, 1, c.dec->verdict}, c.out};
            const int64_t* m = masked_call ? mask : nullptr;
            int64_t* park = unfused ? sc.masked : nullptr;
            if (sda_status e = reveal_decoded_masked(h, ss, da, m, park, c.indices, n_idx, c.dec, st)) return e;
            done->dec = {masked_call ? (unfused ? 2u : 1u) : 0u, 1u, compact ? 1u : 0u};
            if (pc.pending) {
                bool changed = false;                       // (the reveal's own wait has drained the stream)
                if (sda_status e = chacha_combine_end(h, pc, st, &changed)) return e;
                const char* redo = getenv("SDA_RECIPIENT_REDO");
                if (changed || (redo && atoi(redo) == 1)) {
                    if (sda_status e = reveal_decoded_masked(h, ss, da, m, park, c.indices, n_idx, c.dec, st)) return e;
                    done->dec.reveal_runs = 2;
                }
            }
            if (unfused) HIP_TRY(hipStreamSynchronize(st)); // the unmask pass may still run: the call returns counts
            rec.reveal_mode = 2;
            rec.unmask_launches = unfused ? done->dec.reveal_runs : 0;
            done->len = D;
            return SDA_OK;
        }
        sda::PackedRevealArgs ra{rows, dimension, 1, sc.masked};
        // The output is positive(unmask(reveal)).  When the masking modulus (or no mask) and output_modulus are
        // both the sharing prime, that is the canonical residue of (reveal - mask) mod p, which depends only on
        // the reveal's residue: tss' signed representatives (EXACT, 2.1x the canonical reveal's time) cannot
        // change a byte of it, so the canonical reveal runs.  Duplicate clerk points (no Lagrange form) fall
        // back to EXACT.  SDA_RECIPIENT_EXACT=1 keeps EXACT (A/B and test knob).
        const int64_t p = ss->modulus;
        const char* keep = getenv("SDA_RECIPIENT_EXACT");
        const bool residue_only = c.output_modulus == p && (ms->kind == SDA_MASKING_NONE || q == p) &&
                                  !(keep && atoi(keep) == 1);
        const int32_t run_mode = (c.mode == SDA_REVEAL_EXACT && residue_only) ? SDA_REVEAL_CANONICAL : c.mode;
        bool refused = false;
        sda_status e = packed_reveal(h, ss, ra, c.indices, n_idx, run_mode, st, &refused);
        rec.reveal_mode = run_mode == SDA_REVEAL_CANONICAL ? 2 : 1;
        if (refused && run_mode != c.mode) {
            e = packed_reveal(h, ss, ra, c.indices, n_idx, c.mode, st);
            rec.reveal_mode = 1;
            rec.fell_back = 1;
        }
        if (e) return e;
    }
    // 3. unmask (receive.rs:149-152) + RecipientOutput::positive (:14-20), one pass
    HIP_TRY(sda::launch_unmask_positive(sc.masked, ms->kind == SDA_MASKING_NONE ? nullptr : mask, D, q,
                                        c.output_modulus, c.out, st));
    if (pc.pending) {            // the mask's rejection count: fix the mask and unmask again if it had any
        HIP_TRY(hipStreamSynchronize(st));
        bool changed = false;
        if (sda_status e = chacha_combine_end(h, pc, st, &changed)) return e;
        if (changed) {
            HIP_TRY(sda::launch_unmask_positive(sc.masked, sc.mask, D, q, c.output_modulus, c.out, st));
            rec.unmask_launches = 2;
        }
    }
    done->len = D;
    return SDA_OK;
}

// The `_dev` forms: the pipeline on the caller's buffers, its record the handle's when it launched something.
sda_status recipient_dev_call(sda_engine* h, const RecipientCall& c, uint64_t* out_len) {
    *out_len = 0;
    RecipientDone done;
    if (sda_status e = recipient_pipeline(h, c, &done)) return e;
    if (done.len) h->last.recipient = done.rec;
    if (done.len && c.dec) h->last.recipient_decoded = done.dec;
    *out_len = done.len;
    return ok();
}

// The host forms: the pipeline into staging (c.out, any capacity), then the caller's capacity, the copy back and the
// wait.  A call whose output does not fit has not committed its record.
sda_status recipient_host_call(sda_engine* h, const RecipientCall& c, int64_t* out, uint64_t out_cap, uint64_t* out_len) {
    RecipientDone done;
    if (sda_status e = recipient_pipeline(h, c, &done)) return e;
    if (out_cap < done.len) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    if (done.len) {
        h->last.recipient = done.rec;
        if (c.dec) h->last.recipient_decoded = done.dec;
        HIP_TRY(hipMemcpyAsync(out, c.out, done.len * 8, hipMemcpyDeviceToHost, h->stream));
    }
    *out_len = done.len;
    return finish(h);
}

// What a robust call hands back beside `out`: the per-batch words (host or device, either may be NULL) and the
// decoded reveal's counts.  Nothing is written before the call has succeeded.
struct DecodedOutputs {
    void *verdict, *wrong;
    uint64_t *redundancy, *radius, *bad_batches, *first_bad, *undecoded, *blame;
    uint64_t n_idx;
    bool complete() const {
        return redundancy && radius && bad_batches && first_bad && undecoded && (!n_idx || blame);
    }
    // len == 0: no batch, no check (batched.rs:77-81) -- sda_secret_reconstruct_decoded's counts for it
    void commit(const DecodedReveal& d, const sda_sharing_scheme* ss, uint64_t len) const {
        const uint64_t kt = ss->privacy_threshold + ss->secret_count;
        *redundancy = len ? d.redundancy : (n_idx > kt ? n_idx - kt : 0);
        *radius = *redundancy / 2;
        *bad_batches = len ? d.bad_batches : 0;
        *first_bad = len ? d.first_bad : UINT64_MAX;
        *undecoded = len ? d.undecoded : 0;
        for (uint64_t j = 0; j < n_idx; ++j) blame[j] = len && j < d.blame.size() ? d.blame[j] : 0;
    }
};

// Where a robust call is defined, checked on the schemes alone: the decoded reveal's output is canonical, so unmask +
// positive() must be one subtraction mod the sharing prime.  wrong_dev: the device form's `wrong` buffer.
sda_status decoded_scope(const sda_masking_scheme* ms, const sda_sharing_scheme* ss, int64_t output_modulus,
                         const void* wrong_dev) {
    if (ss->kind == SDA_SHARING_ADDITIVE) return fail(SDA_ERR_UNSUPPORTED, "an Additive scheme has no decoded reveal");
    if (ss->kind == SDA_SHARING_PACKED_SHAMIR) {
        if (ss->secret_count > sda::kDecodeMaxK)
            return fail(SDA_ERR_UNSUPPORTED, "the decoded reveal takes at most %u secrets per batch", sda::kDecodeMaxK);
        if (output_modulus != ss->modulus)
            return fail(SDA_ERR_UNSUPPORTED, "the robust recipient job needs output_modulus == the sharing prime");
        if ((ms->kind == SDA_MASKING_FULL || ms->kind == SDA_MASKING_CHACHA) &&
            (ms->modulus < 0 ? (uint64_t)0 - (uint64_t)ms->modulus : (uint64_t)ms->modulus) != (uint64_t)ss->modulus)
            return fail(SDA_ERR_UNSUPPORTED, "the robust recipient job needs a masking modulus equal to the sharing prime");
    }
    if (wrong_dev && (reinterpret_cast<uintptr_t>(wrong_dev) & 3))
        return fail(SDA_ERR_INVALID_ARGUMENT, "wrong must be 4-byte aligned");
    return SDA_OK;
}

// sda_recipient_job_dev, and with `dec` (and the outputs `dout` its counts go to) sda_recipient_job_decoded_dev: the
// same call with the decoded reveal in the pipeline, behind the scope checks that make its output defined.
sda_status job_dev(sda_engine* h, const sda_masking_scheme* ms, const int64_t* mask, uint64_t mask_len,
                   const uint8_t* seed_bytes, const uint64_t* seed_off, uint64_t n_seeds, const sda_sharing_scheme* ss,
                   uint64_t dimension, const uint64_t* indices, const uint8_t* clerk_bytes, const uint64_t* clerk_off,
                   uint64_t n_idx, int64_t output_modulus, int32_t mode, int64_t* out, uint64_t out_cap,
                   uint64_t* out_len, void* stream, DecodedReveal* dec, const DecodedOutputs* dout) {
    if (!h || !ms || !ss || !out_len || (dec && (!dout->complete() || (dimension && !out))))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    const bool full = ms->kind == SDA_MASKING_FULL;
    if (full) n_seeds = 0;                                  // the seed arguments belong to ChaCha and None
    if ((n_idx && (!clerk_bytes || !clerk_off || !indices)) || (n_seeds && (!seed_bytes || !seed_off)) ||
        (full && mask_len && !mask))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (dec)
        if (sda_status e = decoded_scope(ms, ss, output_modulus, dec->wrong)) return e;
    HIP_TRY(hipSetDevice(h->device));
    RecipientCall c{*ms, ss, dimension, indices, n_idx, output_modulus, mode, out, out_cap, pick(h, stream)};
    if (n_seeds)
        if (sda_status e = check_blob_buffer(seed_bytes, seed_off, n_seeds)) return e;
    if (n_idx)
        if (sda_status e = check_blob_buffer(clerk_bytes, clerk_off, n_idx)) return e;
    c.shares = {ShareSource::kBlobs, nullptr, 0, clerk_bytes, clerk_off};
    c.mask.n = n_seeds;
    if (full) {                                             // one row, already folded: full.rs:38-51 has run
        c.mask = {MaskSource::kReady, mask_len ? 1u : 0u, mask_len, mask};
    } else if (ms->kind == SDA_MASKING_CHACHA) {
        c.mask = {MaskSource::kSeedBlobs, n_seeds, sda::kSeedWords, nullptr, seed_bytes, seed_off};
    } else {                                                // none.rs:23: a blob with a byte decodes to a value
        for (uint64_t i = 0; i < n_seeds; ++i) c.mask.width |= seed_off[i + 1] - seed_off[i];
    }
    RecordsGuard records(h);
    c.dec = dec;
    if (sda_status e = recipient_dev_call(h, c, out_len)) return e;
    if (dec) dout->commit(*dec, ss, *out_len);
    if (*out_len)
        h->last.recipient_job = {ms->kind == SDA_MASKING_NONE ? 0u : full ? 1u : 3u,
                                 ss->kind == SDA_SHARING_ADDITIVE ? 1u : 2u,
                                 ms->kind == SDA_MASKING_CHACHA ? (uint32_t)n_seeds : 0u};
    records.keep();
    return ok();
}


// sda_recipient_job, and with `dec` sda_recipient_job_decoded (dout: HOST verdict / wrong and the counts).
sda_status job_host(sda_engine* h, const sda_masking_scheme* ms, const uint8_t* const* mask_blobs,
                    const uint64_t* mask_lens, uint64_t n_masks, const sda_sharing_scheme* ss, uint64_t dimension,
                    const uint64_t* indices, const uint8_t* const* clerk_blobs, const uint64_t* clerk_lens,
                    uint64_t n_idx, int64_t output_modulus, int32_t mode, int64_t* out, uint64_t out_cap,
                    uint64_t* out_len, DecodedReveal* dec, const DecodedOutputs* dout) {
    if (!h || !ms || !ss || !out_len || (n_masks && (!mask_blobs || !mask_lens)) ||
        (n_idx && (!clerk_blobs || !clerk_lens || !indices)) || (dec && (!dout->complete() || (dimension && !out))))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint64_t i = 0; i < n_masks; ++i)
        if (mask_lens[i] && !mask_blobs[i])
            return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument (mask blob %llu)", (unsigned long long)i);
    for (uint64_t i = 0; i < n_idx; ++i)
        if (clerk_lens[i] && !clerk_blobs[i])
            return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument (clerk blob %llu)", (unsigned long long)i);
    if (dec)
        if (sda_status e = decoded_scope(ms, ss, output_modulus, nullptr)) return e;
    *out_len = 0;
    HIP_TRY(hipSetDevice(h->device));
    (void)pick(h, h->stream);
    RecordsGuard records(h);                                // a failing return below: every record stays the previous call's
    // 1. the mask combine's inputs and panics (receive.rs:101-117), before anything of the clerk results is looked at
    // (a robust call's capacity is checked where the pipeline checks it, ahead of the check table)
    RecipientCall c{*ms, ss, dimension, indices, n_idx, output_modulus, mode, nullptr, dec ? out_cap : (uint64_t)-1,
                    h->stream};
    c.mask.n = n_masks;
    const bool chacha = ms->kind == SDA_MASKING_CHACHA;
    uint32_t mask_route = 0;
    if (ms->kind == SDA_MASKING_FULL) {
        // full.rs:38-51 is combiner.rs:16-28: the blobs stream through the clerk's decode -> combine, a group of
        // them in HBM at a time, and the folded mask stays on the device
        int64_t* acc = nullptr;
        uint64_t len = 0;
        if (sda_status e = host_decode_combine(h, ms->modulus, mask_blobs, mask_lens, n_masks, nullptr, 0, &len, &acc))
            return e == SDA_ERR_WRONG_DIMENSION ? fail(SDA_ERR_PRECONDITION, "assertion failed: mask.len() == dimension")
                                                : e;
        c.mask = {MaskSource::kReady, len ? 1u : 0u, len, acc};
        mask_route = 2;
    } else if (chacha) {
        c.mask = {MaskSource::kSeedBlobs, n_masks, sda::kSeedWords};
        uint64_t mask_len;
        if (sda_status e = mask_combine_checks(ms, n_masks, c.mask.width, &mask_len)) return e;
        mask_route = 3;
    } else {
        if (sda_status e = no_mask_checks(mask_lens, n_masks)) return e;
    }
    uint64_t seed_total = 0, clerk_total = 0;
    if (chacha)
        for (uint64_t i = 0; i < n_masks; ++i) seed_total += mask_lens[i];
    for (uint64_t i = 0; i < n_idx; ++i) clerk_total += clerk_lens[i];
    std::vector<uint64_t> seed_off, clerk_off;
    uint8_t* dseed_bytes = nullptr;
    // A multi-device handle combines its ChaCha mask as sda_recipient_reveal does: the key words are decoded on the
    // device and read back (32 bytes a seed) for combine_mask_multi.
    const bool multi = multi_mask(h, ms, n_masks);
    if (multi) {
        DevArena a;
        if (sda_status e = stage(h, rup(seed_total + 32) + rup(n_masks * sda::kSeedWords * 4) + rup((n_masks + 1) * 8), &a))
            return e;
        if (sda_status e = upload_blobs(h, mask_blobs, mask_lens, n_masks, &a, &dseed_bytes, &seed_off)) return e;
        uint32_t* dwords = a.take<uint32_t>(n_masks * sda::kSeedWords);
        uint64_t* doff = a.take<uint64_t>(n_masks + 1);
        std::vector<uint32_t> seeds(n_masks * sda::kSeedWords);
        HIP_TRY(sda::launch_recipient_seeds(dseed_bytes, seed_off.data(), n_masks, doff, dwords, h->stream));
        HIP_TRY(hipMemcpyAsync(seeds.data(), dwords, seeds.size() * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (sda_status e = combine_mask_multi(h, seeds, sda::kSeedWords, n_masks, &c)) return e;
        mask_route = 4;
    }
    // 2. one upload of the seed and clerk payloads
    const uint64_t outn = ss->kind == SDA_SHARING_ADDITIVE ? (n_idx ? clerk_lens[0] : 0) : dimension;
    const bool up_seeds = chacha && !multi && n_masks;
    DevArena a;
    // a robust call's B verdict and wrong words travel behind `out`
    const uint64_t kk = ss->secret_count ? ss->secret_count : 1, Bw = dec ? (dimension + kk - 1) / kk : 0;
    if (sda_status e = stage(h, (up_seeds ? rup(seed_total + 32) : 0) + rup(clerk_total + 32) + rup(outn * 8 + 8) +
                                    rup(Bw * 2) + rup(Bw * 4), &a))
        return e;
    if (up_seeds) {
        if (sda_status e = upload_blobs(h, mask_blobs, mask_lens, n_masks, &a, &dseed_bytes, &seed_off)) return e;
        c.mask.seed_bytes = dseed_bytes;
        c.mask.seed_off = seed_off.data();
    }
    uint8_t* dclerk = nullptr;
    if (sda_status e = upload_blobs(h, clerk_blobs, clerk_lens, n_idx, &a, &dclerk, &clerk_off)) return e;
    c.shares = {ShareSource::kBlobs, nullptr, 0, dclerk, clerk_off.data()};
    c.out = a.take<int64_t>(outn + 1);
    if (dec) {
        c.dec = dec;
        if (dout->verdict) dec->verdict = a.take<uint16_t>(Bw);
        if (dout->wrong) dec->wrong = a.take<uint32_t>(Bw);
    }
    // 3. the pipeline, the clerk results decoded where it reconstructs
    if (sda_status e = recipient_host_call(h, c, out, out_cap, out_len)) return e;
    if (dec) {
        if (*out_len && dec->verdict) HIP_TRY(hipMemcpy(dout->verdict, dec->verdict, Bw * 2, hipMemcpyDeviceToHost));
        if (*out_len && dec->wrong) HIP_TRY(hipMemcpy(dout->wrong, dec->wrong, Bw * 4, hipMemcpyDeviceToHost));
        dout->commit(*dec, ss, *out_len);
    }
    if (*out_len)
        h->last.recipient_job = {mask_route, ss->kind == SDA_SHARING_ADDITIVE ? 1u : 2u, chacha ? (uint32_t)n_masks : 0u};
    records.keep();
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
    RecipientCall c{*ms, ss, dimension, indices, n_idx, output_modulus, mode, out, out_cap, pick(h, stream)};
    c.mask = {MaskSource::kRows, n_masks, mask_width, mask_in};
    c.shares = {ShareSource::kRows, shares, share_len};
    return recipient_dev_call(h, c, out_len);
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
    // host-side shape checks in the reference's order -- the mask combine (receive.rs:101-117) before the
    // reconstruction (:120-146) -- then one upload
    uint64_t width = 0;
    std::vector<uint32_t> seeds;
    if (ms->kind == SDA_MASKING_FULL) {
        width = n_masks ? mask_lens[0] : 0;
        for (uint64_t i = 0; i < n_masks; ++i) {
            if (mask_lens[i] == width) continue;
            // full.rs:45-46 folds row 0 (`%= 0` panics) before :43 reads row i
            if (sda_status e = fold_checks(width, ms->modulus)) return e;
            return fail(SDA_ERR_PRECONDITION, "assertion failed: mask.len() == dimension");
        }
    } else if (ms->kind == SDA_MASKING_CHACHA) {
        uint32_t w;
        seeds = pack_seeds(mask_rows, mask_lens, n_masks, &w);        // key = first 8 words, zero padded
        width = w;
    } else {
        if (sda_status e = no_mask_checks(mask_lens, n_masks)) return e;
    }
    if (ms->kind == SDA_MASKING_FULL || ms->kind == SDA_MASKING_CHACHA) {
        uint64_t mask_len;
        if (sda_status e = mask_combine_checks(ms, n_masks, width, &mask_len)) return e;
    }
    uint64_t share_len = n_idx ? share_lens[0] : 0;
    for (uint64_t i = 0; i < n_idx; ++i) {
        if (share_lens[i] == share_len) continue;
        if (ss->kind == SDA_SHARING_ADDITIVE) {
            // additive.rs:66-67 folds row 0 (`%= 0` panics) before :64 reads row i
            if (sda_status e = fold_checks(share_len, ss->modulus)) return e;
            return fail(SDA_ERR_MISMATCHING_DIMENSION, "Mismatching dimension");
        }
        share_len = share_lens[i] < share_len ? share_lens[i] : share_len;   // packed: reads [0, B) of each
    }
    const uint64_t outn = ss->kind == SDA_SHARING_ADDITIVE ? share_len : dimension;
    RecipientCall c{*ms, ss, dimension, indices, n_idx, output_modulus, mode, nullptr, (uint64_t)-1, h->stream};
    const bool multi = multi_mask(h, ms, n_masks);
    if (multi)
        if (sda_status e = combine_mask_multi(h, seeds, (uint32_t)width, n_masks, &c)) return e;
    DevArena a;
    if (sda_status e = stage(h, rup(n_idx * share_len * 8 + 8) + rup(n_masks * width * 8 + 8) + rup(outn * 8 + 8), &a))
        return e;
    int64_t* dsh = a.take<int64_t>(n_idx * share_len + 1);
    void* dmask = a.take<int64_t>(n_masks * width + 1);
    c.out = a.take<int64_t>(outn + 1);
    for (uint64_t i = 0; i < n_idx; ++i)
        if (share_len) HIP_TRY(hipMemcpyAsync(dsh + i * share_len, share_rows[i], share_len * 8, hipMemcpyHostToDevice, h->stream));
    if (ms->kind == SDA_MASKING_FULL)
        for (uint64_t i = 0; i < n_masks; ++i)
            if (width) HIP_TRY(hipMemcpyAsync(static_cast<int64_t*>(dmask) + i * width, mask_rows[i], width * 8,
                                              hipMemcpyHostToDevice, h->stream));
    if (ms->kind == SDA_MASKING_CHACHA && !seeds.empty() && !multi)
        HIP_TRY(hipMemcpyAsync(dmask, seeds.data(), seeds.size() * 4, hipMemcpyHostToDevice, h->stream));
    if (!multi) c.mask = {MaskSource::kRows, n_masks, ms->kind == SDA_MASKING_NONE ? 0 : width, dmask};
    c.shares = {ShareSource::kRows, dsh, share_len};
    return recipient_host_call(h, c, out, out_cap, out_len);
}

// ---------------- recipient job: the same pipeline from the opened payloads ----------------
// receive.rs:98-157 + positive() with the decode of receive.rs:101-146 (Decryptor::decrypt, sodium.rs:82-90) on the
// device too.
sda_status sda_recipient_job_dev(sda_engine* h, const sda_masking_scheme* ms, const int64_t* mask, uint64_t mask_len,
                                 const uint8_t* seed_bytes, const uint64_t* seed_off, uint64_t n_seeds,
                                 const sda_sharing_scheme* ss, uint64_t dimension, const uint64_t* indices,
                                 const uint8_t* clerk_bytes, const uint64_t* clerk_off, uint64_t n_idx,
                                 int64_t output_modulus, int32_t mode, int64_t* out, uint64_t out_cap,
                                 uint64_t* out_len, void* stream) {
    SDA_ENTRY;
    return job_dev(h, ms, mask, mask_len, seed_bytes, seed_off, n_seeds, ss, dimension, indices, clerk_bytes, clerk_off,
                   n_idx, output_modulus, mode, out, out_cap, out_len, stream, nullptr, nullptr);
}

sda_status sda_recipient_job(sda_engine* h, const sda_masking_scheme* ms, const uint8_t* const* mask_blobs,
                             const uint64_t* mask_lens, uint64_t n_masks, const sda_sharing_scheme* ss,
                             uint64_t dimension, const uint64_t* indices, const uint8_t* const* clerk_blobs,
                             const uint64_t* clerk_lens, uint64_t n_idx, int64_t output_modulus, int32_t mode,
                             int64_t* out, uint64_t out_cap, uint64_t* out_len) {
    SDA_ENTRY;
    return job_host(h, ms, mask_blobs, mask_lens, n_masks, ss, dimension, indices, clerk_blobs, clerk_lens, n_idx,
                    output_modulus, mode, out, out_cap, out_len, nullptr, nullptr);
}
// ---------------- robust recipient job: the same calls over the decoded reveal ----------------
sda_status
sda_recipient_job_decoded(sda_engine* h, const sda_masking_scheme* ms, const uint8_t* const* mask_blobs,
                                     const uint64_t* mask_lens, uint64_t n_masks, const sda_sharing_scheme* ss,
                                     uint64_t dimension, const uint64_t* indices, const uint8_t* const* clerk_blobs,
                                     const uint64_t* clerk_lens, uint64_t n_idx, int64_t output_modulus, int64_t* out,
                                     uint64_t out_cap, uint64_t* out_len, void* verdict, void* wrong,
                                     uint64_t* redundancy, uint64_t* radius, uint64_t* bad_batches,
                                     uint64_t* first_bad, uint64_t* undecoded, uint64_t* blame) {
    SDA_ENTRY;
    DecodedReveal dec;
    const DecodedOutputs dout{verdict, wrong, redundancy, radius, bad_batches, first_bad, undecoded, blame, n_idx};
    return job_host(h, ms, mask_blobs, mask_lens, n_masks, ss, dimension, indices, clerk_blobs, clerk_lens, n_idx,
                    output_modulus, SDA_REVEAL_CANONICAL, out, out_cap, out_len, &dec, &dout);
}

sda_status
sda_recipient_job_decoded_dev(sda_engine* h, const sda_masking_scheme* ms, const int64_t* mask,
                                         uint64_t mask_len, const uint8_t* seed_bytes, const uint64_t* seed_off,
                                         uint64_t n_seeds, const sda_sharing_scheme* ss, uint64_t dimension,
                                         const uint64_t* indices, const uint8_t* clerk_bytes, const uint64_t* clerk_off,
                                         uint64_t n_idx, int64_t output_modulus, int64_t* out, uint64_t out_cap,
                                         uint64_t* out_len, void* verdict, void* wrong, uint64_t* redundancy,
                                         uint64_t* radius, uint64_t* bad_batches, uint64_t* first_bad,
                                         uint64_t* undecoded, uint64_t* blame, void* stream) {
    SDA_ENTRY;
    DecodedReveal dec;
    dec.verdict = static_cast<uint16_t*>(verdict);
    dec.wrong = static_cast<uint32_t*>(wrong);
    const DecodedOutputs dout{verdict, wrong, redundancy, radius, bad_batches, first_bad, undecoded, blame, n_idx};
    return job_dev(h, ms, mask, mask_len, seed_bytes, seed_off, n_seeds, ss, dimension, indices, clerk_bytes, clerk_off,
                   n_idx, output_modulus, SDA_REVEAL_CANONICAL, out, out_cap, out_len, stream, &dec, &dout);
}

sda_status sda_recipient_reveal_decoded_dev(sda_engine* h, const sda_masking_scheme* ms, const void* mask_in,
                                            uint64_t n_masks, uint64_t mask_width, const sda_sharing_scheme* ss,
                                            uint64_t dimension, const uint64_t* indices, const int64_t* shares,
                                            uint64_t n_idx, uint64_t share_len, int64_t output_modulus, int64_t* out,
                                            uint64_t out_cap, uint64_t* out_len, void* verdict, void* wrong,
                                            uint64_t* redundancy, uint64_t* radius, uint64_t* bad_batches,
                                            uint64_t* first_bad, uint64_t* undecoded, uint64_t* blame, void* stream) {
    SDA_ENTRY;
    const DecodedOutputs dout{verdict, wrong, redundancy, radius, bad_batches, first_bad, undecoded, blame, n_idx};
    if (!h || !ms || !ss || !out_len || !dout.complete() || (dimension && !out) || (n_idx && (!shares || !indices)) ||
        (n_masks && mask_width && !mask_in))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (sda_status e = decoded_scope(ms, ss, output_modulus, wrong)) return e;
    HIP_TRY(hipSetDevice(h->device));
    DecodedReveal dec;
    dec.verdict = static_cast<uint16_t*>(verdict);
    dec.wrong = static_cast<uint32_t*>(wrong);
    RecipientCall c{*ms, ss, dimension, indices, n_idx, output_modulus, SDA_REVEAL_CANONICAL, out, out_cap, pick(h, stream)};
    c.mask = {MaskSource::kRows, n_masks, mask_width, mask_in};
    c.shares = {ShareSource::kRows, shares, share_len};
    c.dec = &dec;
    RecordsGuard records(h);
    if (sda_status e = recipient_dev_call(h, c, out_len)) return e;
    dout.commit(dec, ss, *out_len);
    records.keep();
    return ok();
}

sda_status sda_recipient_decoded_last_launch(sda_engine* h, uint32_t* unmask_route, uint32_t* reveal_runs,
                                             uint32_t* compact) {
    SDA_ENTRY;
    if (!h || !unmask_route || !reveal_runs || !compact) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    const sda_engine::RecipientDecodedLaunchInfo& r = h->last.recipient_decoded;
    *unmask_route = r.unmask_route;
    *reveal_runs = r.reveal_runs;
    *compact = r.compact;
    return ok();
}

sda_status sda_recipient_job_last_launch(sda_engine* h, uint32_t* mask_route, uint32_t* share_route,
                                         uint32_t* seeds_decoded) {
    SDA_ENTRY;
    if (!h || !mask_route || !share_route || !seeds_decoded) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for
    const sda_engine::RecipientJobLaunchInfo& r = h->last.recipient_job;
    *mask_route = r.mask_route;
    *share_route = r.share_route;
    *seeds_decoded = r.seeds_decoded;
    return ok();
}

}  // extern "C"
