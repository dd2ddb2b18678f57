// engine_pipelines.cpp -- the fused recipient and participant pipelines of the C ABI (include/sda_engine.h).
#include "engine_internal.h"

using namespace sda_host;

// ---------------- fused role pipelines ----------------
namespace {

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
        if (*mask_len) {                                    // full.rs:45 `%= modulus`
            int64_t q0;
            if (sda_status e = modulus_abs(ms->modulus, &q0)) return e;
        }
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

// The payload source of a recipient job (sda_recipient_job / sda_recipient_job_dev): opened payload bytes on the
// device, laid out as sda_clerk_decode_combine_dev takes them, that recipient_pipeline reads in place of mask_in
// and of shares.  Each part stands alone (the host form on a multi-device handle combines its ChaCha mask first and
// passes the clerk results only).
struct RecipientPayloads {
    const int64_t* combined_mask = nullptr;   // Full: the folded mask, mask_width values as one row, used as it is
    const uint8_t* seed_bytes = nullptr;      // ChaCha: the n_masks seed blobs (mask_width = sda::kSeedWords)
    const uint64_t* seed_off = nullptr;
    const uint8_t* clerk_bytes = nullptr;     // the n_idx clerk results; share_len is then what they decode to
    const uint64_t* clerk_off = nullptr;
    bool shares = false;                      // the clerk results come from clerk_bytes (n_idx may be 0)
};

// The checks every `_dev` call makes of a (bytes, blob_off) pair before anything reads it.
sda_status check_blob_buffer(const uint8_t* bytes, const uint64_t* blob_off, uint64_t n_blobs) {
    if (n_blobs == 0) return SDA_OK;
    if (((uintptr_t)bytes & 15) != 0) return fail(SDA_ERR_INVALID_ARGUMENT, "byte buffer must be 16-byte aligned");
    for (uint64_t b = 0; b < n_blobs; ++b)
        if (blob_off[b + 1] < blob_off[b]) return fail(SDA_ERR_INVALID_ARGUMENT, "blob offsets must be non-decreasing");
    return SDA_OK;
}

// Every *_last_launch record a recipient call can write, on every device of the handle: a call that fails after
// the code it reuses has run puts them back.
struct LaunchRecords {
    struct One {
        sda::ChachaLaunchInfo chacha;
        bool chacha_split;
        sda::CodecLaunchInfo codec;
        sda::CombineLaunchInfo combine;
        sda_engine::RecipientLaunchInfo recipient;
        sda_engine::RecipientJobLaunchInfo job;
    };
    std::vector<One> saved;
    explicit LaunchRecords(sda_engine* h) {
        for (size_t g = 0; g < n_devices(h); ++g) {
            const sda_engine* d = dev_of(h, g);
            saved.push_back({d->chacha_last, d->chacha_split, d->codec_last, d->combine_last, d->recipient_last,
                             d->recipient_job_last});
        }
    }
    void restore(sda_engine* h) const {
        for (size_t g = 0; g < saved.size(); ++g) {
            sda_engine* d = dev_of(h, g);
            d->chacha_last = saved[g].chacha;
            d->chacha_split = saved[g].chacha_split;
            d->codec_last = saved[g].codec;
            d->combine_last = saved[g].combine;
            d->recipient_last = saved[g].recipient;
            d->recipient_job_last = saved[g].job;
        }
    }
};

// receive.rs:80-157 + :14-20 on device-resident inputs (see sda_recipient_reveal_dev); with `pay`, on the opened
// payloads (see sda_recipient_job_dev).
sda_status recipient_pipeline(sda_engine* h, const sda_masking_scheme* ms, const void* mask_in, uint64_t n_masks,
                              uint64_t mask_width, const sda_sharing_scheme* ss, uint64_t dimension,
                              const uint64_t* indices, const int64_t* shares, uint64_t n_idx, uint64_t share_len,
                              int64_t output_modulus, int32_t mode, int64_t* out, uint64_t out_cap,
                              uint64_t* out_len, hipStream_t st, const RecipientPayloads* pay = nullptr) {
    *out_len = 0;
    const bool pay_shares = pay && pay->shares, pay_seeds = pay && pay->seed_off && n_masks;
    // Scratch in h->pipe: [mask | masked | compacted shares], carved once per call -- before the clerk payloads of
    // an Additive scheme are decoded into `masked`, whose length is then bounded by blob 0's bytes only, else once
    // the output length is known
    int64_t *dmask = nullptr, *dmasked = nullptr, *dcompact = nullptr;
    auto carve = [&](uint64_t masked_cap, uint64_t mask_cap, uint64_t compact_bytes) -> sda_status {
        if (sda_status e = ensure(&h->pipe, &h->pipe_bytes,
                                  rup(mask_cap * 8) + rup(masked_cap * 8) + rup(compact_bytes) + 256))
            return e;
        dmask = static_cast<int64_t*>(h->pipe);
        dmasked = dmask + rup(mask_cap * 8) / 8;
        dcompact = dmasked + rup(masked_cap * 8) / 8;
        return SDA_OK;
    };
    // Checks in the reference's order: mask combine (receive.rs:101-117), reconstruct (:120-146),
    // unmask (:149-152).
    // ---- 1. mask combine: its length and panics ----
    uint64_t mask_len = 0;
    if (sda_status e = mask_combine_checks(ms, n_masks, mask_width, &mask_len)) return e;
    // ChaCha seed payloads: the key words of every seed, zero padded, decoded into handle scratch.  Queued here, in
    // front of the wait the clerk results' lengths take, so that the offsets' copy and the kernel hide under it and
    // the mask combine finds its seeds ready.
    uint32_t* dseeds = nullptr;
    if (pay_seeds && ms->kind == SDA_MASKING_CHACHA && mask_len) {
        const size_t words = rup(n_masks * sda::kSeedWords * 4);
        if (sda_status e = ensure(&h->job_work, &h->job_work_bytes, words + rup((n_masks + 1) * 8))) return e;
        dseeds = static_cast<uint32_t*>(h->job_work);
        HIP_TRY(sda::launch_recipient_seeds(pay->seed_bytes, pay->seed_off, n_masks,
                                            reinterpret_cast<uint64_t*>(static_cast<char*>(h->job_work) + words),
                                            dseeds, st));
    }
    // ---- 2. reconstruct: masked output length and errors ----
    uint64_t D;
    uint64_t stride = share_len;                             // of the i64 clerk rows the packed reveal reads
    sda::VarintPlan plan;                                    // PackedShamir clerk payloads: the count pass's plan
    bool irregular = false;
    if (ss->kind == SDA_SHARING_ADDITIVE && pay_shares) {
        // additive.rs:56-72 is combiner.rs:16-28: the clerk's decode -> combine writes `masked`, and its one wait
        // tells the length.  Row 0 is folded (`%= modulus`, additive.rs:66-67) before :64 reads a later row's length.
        const uint64_t cap = n_idx ? pay->clerk_off[1] - pay->clerk_off[0] : 0;       // one value per byte at most
        if (cap) {
            int64_t m0;
            if (sda_status e = modulus_abs(ss->modulus, &m0)) return e;
        }
        if (sda_status e = carve(cap, ms->kind == SDA_MASKING_NONE || pay->combined_mask ? 0 : std::min(mask_len, cap), 0))
            return e;
        if (sda_status e = decode_combine(h, ss->modulus, pay->clerk_bytes, pay->clerk_off, n_idx, dmasked, cap, &D, st))
            return e == SDA_ERR_WRONG_DIMENSION ? fail(SDA_ERR_MISMATCHING_DIMENSION, "Mismatching dimension") : e;
    } else if (ss->kind == SDA_SHARING_ADDITIVE) {
        D = n_idx ? share_len : 0;                           // additive.rs:56-60
        if (D) {                                             // additive.rs:67 `%= modulus`
            int64_t m0;
            if (sda_status e = modulus_abs(ss->modulus, &m0)) return e;
        }
    } else if (ss->kind == SDA_SHARING_PACKED_SHAMIR) {
        if (sda_status e = check_packed(ss)) return e;
        if (mode != SDA_REVEAL_EXACT && mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
        const uint64_t B = (dimension + ss->secret_count - 1) / ss->secret_count;
        if (pay_shares) {
            // the count pass's one wait supplies the lengths of the reference's checks: ragged rows are read over
            // [0, B) (batched.rs:83-85), so the shortest decides, and the longest is the rows' stride
            share_len = stride = 0;
            if (B && n_idx) {
                std::vector<uint64_t> counts(n_idx);
                if (sda_status e = codec_count(h, pay->clerk_bytes, pay->clerk_off, n_idx, &plan, counts.data(),
                                               &irregular, st))
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
    const bool compact = packed && stride != B;
    if (!dmasked)                                           // (a payload job's Additive reconstruction has run)
        if (sda_status e = carve(D, D, compact ? n_idx * B * 8 : 0)) return e;
    // sda_recipient_last_launch: collected here, the handle's record only once this call returns SDA_OK
    sda_engine::RecipientLaunchInfo rec;
    rec.mask_kind = ms->kind == SDA_MASKING_NONE ? 1 : ms->kind == SDA_MASKING_FULL ? 2 : 3;
    rec.compact = compact;
    rec.unmask_launches = 1;
    // 1. masks (receive.rs:101-117)
    const int64_t* mask = dmask;
    if (ms->kind == SDA_MASKING_FULL && pay && pay->combined_mask) {
        mask = pay->combined_mask;                          // folded by the caller: (0 + c) % m = c
    } else if (ms->kind == SDA_MASKING_FULL) {
        if (sda_status e = modulus_abs(ms->modulus, &q)) return e;
        HIP_TRY(sda::launch_combine_exact(static_cast<const int64_t*>(mask_in), n_masks, D, mask_width, dmask, q, st,
                                          false, &h->combine_last));
    }
    PendingChacha pc;                                       // ChaCha: its rejection count is checked at the end
    if (ms->kind == SDA_MASKING_CHACHA) {
        const uint32_t* seeds = dseeds ? dseeds : static_cast<const uint32_t*>(mask_in);
        if (sda_status e = chacha_combine_begin(h, ms->modulus, D, seeds, (uint32_t)mask_width, n_masks, dmask, st, &pc))
            return e;
    }
    // 2. reconstruct (receive.rs:120-146)
    if (!packed && !pay_shares) {
        int64_t m;
        if (sda_status e = modulus_abs(ss->modulus, &m)) return e;
        HIP_TRY(sda::launch_combine_exact(shares, n_idx, D, share_len, dmasked, m, st, false, &h->combine_last));
    } else if (packed) {
        if (pay_shares) {                                   // i64 rows of the longest blob's length in handle scratch
            if (sda_status e = ensure(&h->codec_mat, &h->codec_mat_bytes, n_idx * stride * 8 + 8)) return e;
            int64_t* rows = static_cast<int64_t*>(h->codec_mat);
            HIP_TRY(sda::launch_varint_decode(pay->clerk_bytes, n_idx, plan, h->codec_work, rows, stride, stride,
                                              irregular, st));
            shares = rows;
        }
        const int64_t* src = shares;
        if (compact) {                                      // batched.rs:83-85 reads [clerk][0..B)
            int64_t* c = dcompact;
            HIP_TRY(hipMemcpy2DAsync(c, B * 8, shares, stride * 8, B * 8, n_idx, hipMemcpyDeviceToDevice, st));
            src = c;
        }
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
        bool refused = false;
        sda_status e = packed_reveal(h, ss, ra, indices, n_idx, run_mode, st, &refused);
        rec.reveal_mode = run_mode == SDA_REVEAL_CANONICAL ? 2 : 1;
        if (refused && run_mode != mode) {
            e = packed_reveal(h, ss, ra, indices, n_idx, mode, st);
            rec.reveal_mode = 1;
            rec.fell_back = 1;
        }
        if (e) return e;
    }
    // 3. unmask (receive.rs:149-152) + RecipientOutput::positive (:14-20), one pass
    HIP_TRY(sda::launch_unmask_positive(dmasked, ms->kind == SDA_MASKING_NONE ? nullptr : mask, D, q,
                                        output_modulus, out, st));
    if (pc.pending) {            // the mask's rejection count: fix the mask and unmask again if it had any
        HIP_TRY(hipStreamSynchronize(st));
        bool changed = false;
        if (sda_status e = chacha_combine_end(h, pc, st, &changed)) return e;
        if (changed) {
            HIP_TRY(sda::launch_unmask_positive(dmasked, dmask, D, q, output_modulus, out, st));
            rec.unmask_launches = 2;
        }
    }
    h->recipient_last = rec;
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
    // host-side shape checks in the reference's order -- the mask combine (receive.rs:101-117) before the
    // reconstruction (:120-146) -- then one upload
    uint64_t width = 0;
    std::vector<uint32_t> seeds;
    if (ms->kind == SDA_MASKING_FULL) {
        width = n_masks ? mask_lens[0] : 0;
        for (uint64_t i = 0; i < n_masks; ++i) {
            if (mask_lens[i] == width) continue;
            if (width) {                                    // full.rs:45-46 folds row 0 (`%= 0` panics) before :43 reads row i
                int64_t q0;
                if (sda_status e = modulus_abs(ms->modulus, &q0)) return e;
            }
            return fail(SDA_ERR_PRECONDITION, "assertion failed: mask.len() == dimension");
        }
    } else if (ms->kind == SDA_MASKING_CHACHA) {
        uint32_t w;
        seeds = pack_seeds(mask_rows, mask_lens, n_masks, &w);        // key = first 8 words, zero padded
        width = w;
    } else {
        for (uint64_t i = 0; i < n_masks; ++i)
            if (mask_lens[i]) return fail(SDA_ERR_PRECONDITION, "assertion failed: masks.iter().all(|mask| mask.len() == 0)");
    }
    if (ms->kind == SDA_MASKING_FULL || ms->kind == SDA_MASKING_CHACHA) {
        uint64_t mask_len;
        if (sda_status e = mask_combine_checks(ms, n_masks, width, &mask_len)) return e;
    }
    uint64_t share_len = n_idx ? share_lens[0] : 0;
    for (uint64_t i = 0; i < n_idx; ++i) {
        if (share_lens[i] == share_len) continue;
        if (ss->kind == SDA_SHARING_ADDITIVE) {
            if (share_len) {                                // additive.rs:66-67 folds row 0 (`%= 0` panics) before :64 reads row i
                int64_t m0;
                if (sda_status e = modulus_abs(ss->modulus, &m0)) return e;
            }
            return fail(SDA_ERR_MISMATCHING_DIMENSION, "Mismatching dimension");
        }
        share_len = share_lens[i] < share_len ? share_lens[i] : share_len;   // packed: reads [0, B) of each
    }
    const uint64_t outn = ss->kind == SDA_SHARING_ADDITIVE ? share_len : dimension;
    // A multi-device handle spreads the mask combine (receive.rs:113-116, the dominant cost at configs[4]) over its
    // devices -- seeds split, one RCCL reduce onto device 0 (engine_host.cpp) -- and runs the rest of the
    // pipeline on device 0 with the combined mask as one Full mask row: (0 + c) % m = c for the canonical c, so
    // the unmask sees the same mask.  Only where the reference would not panic in the mask combine (m > 0).
    const sda_masking_scheme full_row = {SDA_MASKING_FULL, ms->modulus, 0, 0};
    const bool multi_mask = ms->kind == SDA_MASKING_CHACHA && is_multi(h) && n_masks && ms->dimension &&
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
    const sda_engine::RecipientLaunchInfo before = h->recipient_last;
    if (sda_status e = multi_mask
                           ? recipient_pipeline(h, &full_row, h->hs_dev, 1, ms->dimension, ss, dimension, indices, dsh,
                                                n_idx, share_len, output_modulus, mode, dout, (uint64_t)-1, &len, h->stream)
                           : recipient_pipeline(h, ms, dmask, n_masks, ms->kind == SDA_MASKING_NONE ? 0 : width, ss,
                                                dimension, indices, dsh, n_idx, share_len, output_modulus, mode, dout,
                                                (uint64_t)-1, &len, h->stream))
        return e;
    if (out_cap < len) {
        h->recipient_last = before;              // the call fails: the record stays the previous call's
        return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    }
    if (multi_mask && len) h->recipient_last.mask_kind = 4;   // the pipeline saw the combined row as a Full mask
    if (len) HIP_TRY(hipMemcpyAsync(out, dout, len * 8, hipMemcpyDeviceToHost, h->stream));
    *out_len = len;
    return finish(h);
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
    if (!h || !ms || !ss || !out_len) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    const bool full = ms->kind == SDA_MASKING_FULL;
    if (full) n_seeds = 0;                                  // the seed arguments belong to ChaCha and None
    if ((n_idx && (!clerk_bytes || !clerk_off || !indices)) || (n_seeds && (!seed_bytes || !seed_off)) ||
        (full && mask_len && !mask))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick(h, stream);
    if (sda_status e = check_blob_buffer(seed_bytes, seed_off, n_seeds)) return e;
    if (sda_status e = check_blob_buffer(clerk_bytes, clerk_off, n_idx)) return e;
    RecipientPayloads pay;
    pay.clerk_bytes = clerk_bytes;
    pay.clerk_off = clerk_off;
    pay.shares = true;
    uint64_t n_masks = n_seeds, width = 0;
    if (full) {                                             // one row, already folded: full.rs:38-51 has run
        n_masks = mask_len ? 1 : 0;
        width = mask_len;
        pay.combined_mask = mask;
    } else if (ms->kind == SDA_MASKING_CHACHA) {
        width = sda::kSeedWords;
        pay.seed_bytes = seed_bytes;
        pay.seed_off = seed_off;
    } else {                                                // none.rs:23: a blob with a byte decodes to a value
        for (uint64_t i = 0; i < n_seeds; ++i) width |= seed_off[i + 1] - seed_off[i];
    }
    const LaunchRecords before(h);
    if (sda_status e = recipient_pipeline(h, ms, nullptr, n_masks, width, ss, dimension, indices, nullptr, n_idx, 0,
                                          output_modulus, mode, out, out_cap, out_len, st, &pay)) {
        before.restore(h);
        return e;
    }
    if (*out_len)
        h->recipient_job_last = {ms->kind == SDA_MASKING_NONE ? 0u : full ? 1u : 3u,
                                 ss->kind == SDA_SHARING_ADDITIVE ? 1u : 2u,
                                 ms->kind == SDA_MASKING_CHACHA ? (uint32_t)n_seeds : 0u};
    return ok();
}

sda_status sda_recipient_job(sda_engine* h, const sda_masking_scheme* ms, const uint8_t* const* mask_blobs,
                             const uint64_t* mask_lens, uint64_t n_masks, const sda_sharing_scheme* ss,
                             uint64_t dimension, const uint64_t* indices, const uint8_t* const* clerk_blobs,
                             const uint64_t* clerk_lens, uint64_t n_idx, int64_t output_modulus, int32_t mode,
                             int64_t* out, uint64_t out_cap, uint64_t* out_len) {
    SDA_ENTRY;
    if (!h || !ms || !ss || !out_len || (n_masks && (!mask_blobs || !mask_lens)) ||
        (n_idx && (!clerk_blobs || !clerk_lens || !indices)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    for (uint64_t i = 0; i < n_masks; ++i)
        if (mask_lens[i] && !mask_blobs[i])
            return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument (mask blob %llu)", (unsigned long long)i);
    for (uint64_t i = 0; i < n_idx; ++i)
        if (clerk_lens[i] && !clerk_blobs[i])
            return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument (clerk blob %llu)", (unsigned long long)i);
    *out_len = 0;
    HIP_TRY(hipSetDevice(h->device));
    (void)pick(h, h->stream);
    const LaunchRecords before(h);
    auto failed = [&](sda_status e) {                       // the call fails: every record stays the previous call's
        before.restore(h);
        return e;
    };
    // 1. the mask combine's inputs and panics (receive.rs:101-117), before anything of the clerk results is looked at
    RecipientPayloads pay;
    uint64_t pipe_masks = n_masks, width = 0;
    const void* mask_in = nullptr;
    const sda_masking_scheme* pipe_ms = ms;
    const sda_masking_scheme full_row = {SDA_MASKING_FULL, ms->modulus, 0, 0};
    const bool chacha = ms->kind == SDA_MASKING_CHACHA;
    uint32_t mask_route = 0;
    if (ms->kind == SDA_MASKING_FULL) {
        // full.rs:38-51 is combiner.rs:16-28: the blobs stream through the clerk's decode -> combine, a group of
        // them in HBM at a time, and the folded mask stays on the device
        int64_t* acc = nullptr;
        uint64_t len = 0;
        if (sda_status e = host_decode_combine(h, ms->modulus, mask_blobs, mask_lens, n_masks, nullptr, 0, &len, &acc)) {
            before.restore(h);
            return e == SDA_ERR_WRONG_DIMENSION ? fail(SDA_ERR_PRECONDITION, "assertion failed: mask.len() == dimension")
                                                : e;
        }
        pay.combined_mask = acc;
        pipe_masks = len ? 1 : 0;
        width = len;
        mask_route = 2;
    } else if (chacha) {
        width = sda::kSeedWords;
        uint64_t mask_len;
        if (sda_status e = mask_combine_checks(ms, n_masks, width, &mask_len)) return e;
        mask_route = 3;
    } else {
        for (uint64_t i = 0; i < n_masks; ++i)
            if (mask_lens[i]) return fail(SDA_ERR_PRECONDITION, "assertion failed: masks.iter().all(|mask| mask.len() == 0)");
    }
    uint64_t seed_total = 0, clerk_total = 0;
    if (chacha)
        for (uint64_t i = 0; i < n_masks; ++i) seed_total += mask_lens[i];
    for (uint64_t i = 0; i < n_idx; ++i) clerk_total += clerk_lens[i];
    std::vector<uint64_t> seed_off, clerk_off;
    uint8_t* dseed_bytes = nullptr;
    // A multi-device handle spreads the ChaCha mask combine over its devices exactly as sda_recipient_reveal does:
    // the key words are decoded on the device, read back (32 bytes a seed), split, reduced onto device 0, and the
    // pipeline sees the combined mask as one Full row.
    const bool multi_mask = chacha && is_multi(h) && n_masks && ms->dimension && ms->modulus > 0;
    if (multi_mask) {
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
        if (sda_status e = host_stream_ensure(h, 0, ms->dimension * 8)) return e;
        if (sda_status e = chacha_combine_multi(h, ms->modulus, ms->dimension, seeds, sda::kSeedWords, n_masks,
                                                static_cast<int64_t*>(h->hs_dev)))
            return failed(e);
        pipe_ms = &full_row;
        mask_in = h->hs_dev;
        pipe_masks = 1;
        width = ms->dimension;
        mask_route = 4;
    }
    // 2. one upload of the seed and clerk payloads
    const uint64_t outn = ss->kind == SDA_SHARING_ADDITIVE ? (n_idx ? clerk_lens[0] : 0) : dimension;
    const bool up_seeds = chacha && !multi_mask && n_masks;
    DevArena a;
    if (sda_status e = stage(h, (up_seeds ? rup(seed_total + 32) : 0) + rup(clerk_total + 32) + rup(outn * 8 + 8), &a))
        return failed(e);
    if (up_seeds) {
        if (sda_status e = upload_blobs(h, mask_blobs, mask_lens, n_masks, &a, &dseed_bytes, &seed_off)) return failed(e);
        pay.seed_bytes = dseed_bytes;
        pay.seed_off = seed_off.data();
    }
    uint8_t* dclerk = nullptr;
    if (sda_status e = upload_blobs(h, clerk_blobs, clerk_lens, n_idx, &a, &dclerk, &clerk_off)) return failed(e);
    pay.clerk_bytes = dclerk;
    pay.clerk_off = clerk_off.data();
    pay.shares = true;
    int64_t* dout = a.take<int64_t>(outn + 1);
    // 3. the pipeline, the clerk results decoded where it reconstructs
    uint64_t len = 0;
    if (sda_status e = recipient_pipeline(h, pipe_ms, mask_in, pipe_masks, width, ss, dimension, indices, nullptr, n_idx,
                                          0, output_modulus, mode, dout, (uint64_t)-1, &len, h->stream, &pay))
        return failed(e);
    if (out_cap < len) {
        before.restore(h);
        return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
    }
    if (len) {
        if (multi_mask) h->recipient_last.mask_kind = 4;    // the pipeline saw the combined row as a Full mask
        h->recipient_job_last = {mask_route, ss->kind == SDA_SHARING_ADDITIVE ? 1u : 2u,
                                 chacha ? (uint32_t)n_masks : 0u};
        HIP_TRY(hipMemcpyAsync(out, dout, len * 8, hipMemcpyDeviceToHost, h->stream));
    }
    *out_len = len;
    return finish(h);
}

sda_status sda_recipient_job_last_launch(sda_engine* h, uint32_t* mask_route, uint32_t* share_route,
                                         uint32_t* seeds_decoded) {
    SDA_ENTRY;
    if (!h || !mask_route || !share_route || !seeds_decoded) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for
    const sda_engine::RecipientJobLaunchInfo& r = h->recipient_job_last;
    *mask_route = r.mask_route;
    *share_route = r.share_route;
    *seeds_decoded = r.seeds_decoded;
    return ok();
}

// The participant pipeline behind sda_participant_share_dev, sda_participant_share32_dev and their keyed forms.
// One of shares64 / shares32 is the [n][B] output (shares32: int32 rows, encoded by the int32 encoder; PackedShamir,
// and keyed Additive up to modulus 2^31).  kd (the keyed forms): `draws` is NULL and the share-generation draws
// come from (kd->key, kd->stream_id) -- Additive in the fused kernel, PackedShamir through the keyed launch
// (packed_generate: in the share kernels, or staged in h->keyed_draws where those do not serve the scheme).
// job (the participant job, keyed): where a Full mask comes from and where the call's secrets lie within the job.
struct ParticipantJobArgs {
    // Full masking: `full_masks` is NULL and the mask is drawn in the masking kernel (mask_keyed.hip) from
    // (mask_key, mask_stream_id); its `dimension` values go to mask64, or to mask32 as int32 when that is given
    const uint32_t* mask_key = nullptr;
    uint32_t mask_stream_id = 0;
    int64_t* mask64 = nullptr;
    int32_t* mask32 = nullptr;
    // the call's first batch (Additive: column) within the job: the first_batch / first_column of the keyed share
    // generation, and times the batch size the first element of the mask
    uint64_t first = 0;
    // the masking step alone (the host job under ChaCha masking, whose tiles then share and encode): nothing is
    // generated or encoded, and *masked_out = the D masked secrets in handle scratch (h->pipe), complete for work
    // queued on the call's stream after it (the rejection check and its redo have run)
    const int64_t** masked_out = nullptr;
};
static sda_status participant_share(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                    uint64_t seed_words, const int64_t* full_masks, const sda_sharing_scheme* ss,
                                    const int64_t* secrets, uint64_t dimension, const int64_t* draws, int32_t mode,
                                    int64_t* shares64, int32_t* shares32, uint8_t* payload, uint64_t payload_cap,
                                    uint64_t* payload_row_bytes, void* stream, const KeyedDraws* kd = nullptr,
                                    const ParticipantJobArgs* job = nullptr) {
    const bool mask_only = job && job->masked_out;
    if (!h || !ms || !ss || (dimension && (!secrets || (!shares64 && !shares32 && !mask_only))) ||
        (payload && !payload_row_bytes) || (kd && !kd->key))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick(h, stream);
    const uint64_t D = dimension;
    const bool packed = ss->kind == SDA_SHARING_PACKED_SHAMIR;
    const uint64_t first = job ? job->first : 0;
    if (!packed && ss->kind != SDA_SHARING_ADDITIVE) return fail(SDA_ERR_INVALID_ARGUMENT, "unknown sharing scheme kind");
    if (!packed && shares32 && !kd)
        return fail(SDA_ERR_UNSUPPORTED, "int32 shares need a PackedShamir scheme: an additive scheme's first n - 1 "
                                         "shares are the caller's draws, copied unchecked");
    if (mode != SDA_REVEAL_EXACT && mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
    if (packed) {
        if (sda_status e = check_packed(ss)) return e;
    } else {
        if (ss->share_count == 0) return fail(SDA_ERR_PRECONDITION, "share_count - 1 underflows (additive.rs:42)");
        if (ss->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
        if (shares32 && ss->modulus > (int64_t)1 << 31)
            return fail(SDA_ERR_UNSUPPORTED, "int32 shares of an additive scheme need modulus <= 2^31: its first n - 1 "
                                             "shares are draws in [0, modulus), which need not fit int32");
    }
    // 1. SecretMasker::mask (participate.rs:53-54)
    const int64_t* masked = secrets;
    // ChaCha on the fast path: the masked secrets come straight out of the ChaCha kernel and its rejection
    // count is checked at the end of the call (a nonzero count -- probability < 2^-28 per draw -- redoes
    // the mask exactly, then every later step)
    bool mask_pending = false;
    // sda_participant_last_launch: collected here, the handle's record only once this call returns SDA_OK
    sda_engine::ParticipantLaunchInfo rec;
    rec.mask_route = 1;
    rec.share_route = packed ? (kd ? 4 : 3) : (kd ? 2 : 1);
    rec.passes = 1;
    int64_t* cmask = nullptr;
    uint32_t* cseed = nullptr;
    uint32_t cw = 0;
    // chacha.rs:26 assert_eq!(self.dimension, secrets.len()): before any draw, and for an empty secrets vector too
    if (ms->kind == SDA_MASKING_CHACHA && ms->dimension != D)
        return fail(SDA_ERR_PRECONDITION, "assertion failed: dimension == secrets.len()");
    if (ms->kind != SDA_MASKING_NONE && D) {
        if (ms->modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
        if (sda_status e = ensure(&h->pipe, &h->pipe_bytes, 2 * rup(D * 8) + 256)) return e;
        int64_t* dm = static_cast<int64_t*>(h->pipe);
        if (ms->kind == SDA_MASKING_FULL && job && job->mask_key) {
            // full.rs:25-31 in one kernel: element d of the call is element first k + d of the job's mask
            HIP_TRY(sda::launch_full_mask_keyed(job->mask_key, job->mask_stream_id,
                                                first * (packed ? ss->secret_count : 1), secrets, D, ms->modulus, dm,
                                                job->mask64, job->mask32, st));
            rec.mask_route = 5;
        } else if (ms->kind == SDA_MASKING_FULL) {
            if (!full_masks) return fail(SDA_ERR_INVALID_ARGUMENT, "Full masking needs the drawn masks");
            HIP_TRY(sda::launch_addsub_trem(secrets, full_masks, +1, D, dm, ms->modulus, st));      // full.rs:28-31
            rec.mask_route = 2;
        } else if (ms->kind == SDA_MASKING_CHACHA) {
            const uint64_t want = (ms->seed_bitsize + 31) / 32;
            if (seed_words != want || (seed_words && !seed))
                return fail(SDA_ERR_PRECONDITION, "expected %llu seed words", (unsigned long long)want);
            int64_t* dmask = dm + rup(D * 8) / 8;
            uint32_t* dseed = reinterpret_cast<uint32_t*>(dmask + rup(D * 8) / 8);
            const uint32_t w = (uint32_t)(seed_words < 8 ? seed_words : 8);
            if (w) HIP_TRY(hipMemcpyAsync(dseed, seed, w * 4, hipMemcpyHostToDevice, st));
            // chacha.rs:36-45: masked = (secrets + draw) % m over one stream
            if (chacha_fast_path(ms->modulus)) {
                if (sda_status e = ensure(&h->work, &h->work_bytes, sda::chacha_work_bytes(D, 0))) return e;
                sda::ChachaLaunchInfo info;
                HIP_TRY(sda::launch_chacha_mask_add_async(ms->modulus, D, dseed, w, secrets, dm, h->work, st,
                                                          h->rej_host, &info));
                record_chacha(h, info);
                mask_pending = true;
                rec.mask_route = 3;
            } else {
                if (sda_status e = chacha_combine(h, ms->modulus, D, dseed, w, 1, dmask, st)) return e;
                HIP_TRY(sda::launch_addsub_trem(secrets, dmask, +1, D, dm, ms->modulus, st));
                rec.mask_route = 4;
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
    if (B && !draws && !kd) return fail(SDA_ERR_INVALID_ARGUMENT, "need the randomness draws");
    if (payload && n > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 clerks");
    auto share_and_encode = [&]() -> sda_status {
        if (mask_only) return SDA_OK;
        if (B) {
            if (packed) {
                sda::PackedGenArgs ga{masked, D, 1, draws, shares64, mode == SDA_REVEAL_CANONICAL};
                ga.out32 = shares32;             // as sda_packed_generate32_dev: scratch + narrowing at n + 1 = 81
                if (kd) {                        // batch b takes draws b t + j of (key, stream_id) at bound p - 1
                    ga.key = kd->key;
                    ga.stream_id = kd->stream_id;
                    ga.first_batch = first;
                }
                if (sda_status e = packed_generate(h, ss, ga, st)) return e;
            } else if (kd) {
                HIP_TRY(sda::launch_additive_generate_keyed(kd->key, kd->stream_id, first, masked, D, n, ss->modulus,
                                                            shares64, shares32, B, st));
            } else {
                HIP_TRY(sda::launch_additive_generate(masked, D, draws, n, shares64, ss->modulus, st));
            }
        }
        // 3. per-clerk payload encoding (participate.rs:79-98 -> sodium.rs:36-41); sealing stays on the host
        if (payload) {
            if (sda_status e = shares32 ? encode_rows(h, shares32, n, B, B, payload, payload_cap, payload_row_bytes, st,
                                                      "payload_cap")
                                        : encode_rows(h, shares64, n, B, B, payload, payload_cap, payload_row_bytes, st,
                                                      "payload_cap"))
                return e;
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
            rec.passes = 2;
        }
    }
    if (D) h->participant_last = rec;
    if (mask_only) *job->masked_out = masked;
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

// The two calls above with the share-generation draws made on the device from (key, stream_id).
sda_status sda_participant_share_keyed_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                           uint64_t seed_words, const int64_t* full_masks,
                                           const sda_sharing_scheme* ss, const int64_t* secrets, uint64_t dimension,
                                           const uint32_t* key, uint32_t stream_id, int32_t mode, int64_t* shares_out,
                                           uint8_t* payload, uint64_t payload_cap, uint64_t* payload_row_bytes,
                                           void* stream) {
    SDA_ENTRY;
    const KeyedDraws kd{key, stream_id};
    return participant_share(h, ms, seed, seed_words, full_masks, ss, secrets, dimension, nullptr, mode, shares_out,
                             nullptr, payload, payload_cap, payload_row_bytes, stream, &kd);
}

sda_status sda_participant_share32_keyed_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                             uint64_t seed_words, const int64_t* full_masks,
                                             const sda_sharing_scheme* ss, const int64_t* secrets, uint64_t dimension,
                                             const uint32_t* key, uint32_t stream_id, int32_t mode,
                                             int32_t* shares_out, uint8_t* payload, uint64_t payload_cap,
                                             uint64_t* payload_row_bytes, void* stream) {
    SDA_ENTRY;
    const KeyedDraws kd{key, stream_id};
    return participant_share(h, ms, seed, seed_words, full_masks, ss, secrets, dimension, nullptr, mode, nullptr,
                             shares_out, payload, payload_cap, payload_row_bytes, stream, &kd);
}

// ---------------- participant job: mask, mask payload, shares and clerk payloads in one call ----------------
// participate.rs:53-98 without the sealing: participant_share with the Full mask drawn in its masking kernel, the
// shares in handle scratch and the recipient's mask payload encoded next to the clerks'.
}  // extern "C"

namespace {

// Every *_last_launch record a participant job's reused code writes (on ordinals[0], where it runs): a call that
// fails puts them back.
struct ParticipantRecords {
    sda::ChachaLaunchInfo chacha;
    bool chacha_split;
    sda_engine::ParticipantLaunchInfo participant;
    sda_engine::ParticipantJobLaunchInfo job;
    uint32_t keyed_path;
    uint64_t keyed_staged_bytes;
    explicit ParticipantRecords(const sda_engine* h)
        : chacha(h->chacha_last), chacha_split(h->chacha_split), participant(h->participant_last),
          job(h->participant_job_last), keyed_path(h->keyed_path), keyed_staged_bytes(h->keyed_staged_bytes) {}
    void restore(sda_engine* h) const {
        h->chacha_last = chacha;
        h->chacha_split = chacha_split;
        h->participant_last = participant;
        h->participant_job_last = job;
        h->keyed_path = keyed_path;
        h->keyed_staged_bytes = keyed_staged_bytes;
    }
};

// What both job forms settle before any work: the schemes' kinds, the payload bounds and the width of the rows.
struct ParticipantJobSetup {
    sda::ParticipantJobShape shape;
    uint64_t row_bound = 0, mask_bound = 0;   // sda_participant_job_payload_bound
    bool packed = false, full = false, chacha = false;
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
    // int32 rows wherever they fit by construction (sda_participant_share32_keyed_dev's rule)
    s->share_bytes = s->packed || ss->modulus <= (int64_t)1 << 31 ? 4 : 8;
    s->mask_bytes = s->full ? (ms->modulus <= (int64_t)1 << 31 ? 4 : 8) : 0;
    s->mask_route = s->full ? (s->mask_bytes == 8 ? 1u : 2u) : s->chacha ? 3u : 0u;
    return SDA_OK;
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

// The call's (a tile's) share rows [n][B] and the Full mask row [D] behind them, in h->job_shares.
struct JobRows {
    int64_t* sh64 = nullptr;
    int32_t* sh32 = nullptr;
    int64_t* mask64 = nullptr;
    int32_t* mask32 = nullptr;
};
sda_status job_rows(sda_engine* h, const ParticipantJobSetup& s, uint64_t n, uint64_t B, uint64_t D, JobRows* r) {
    uint64_t shares, mask;
    if (__builtin_mul_overflow(n, B, &shares) || __builtin_mul_overflow(shares, (uint64_t)s.share_bytes, &shares) ||
        __builtin_mul_overflow(D, (uint64_t)s.mask_bytes, &mask) || shares > (uint64_t)1 << 62 || mask > (uint64_t)1 << 62)
        return fail(SDA_ERR_OUT_OF_MEMORY, "the share rows do not fit the address space");
    if (sda_status e = ensure(&h->job_shares, &h->job_shares_bytes, rup(shares) + rup(mask) + 256)) return e;
    char* base = static_cast<char*>(h->job_shares);
    (s.share_bytes == 4 ? (void)(r->sh32 = reinterpret_cast<int32_t*>(base))
                        : (void)(r->sh64 = reinterpret_cast<int64_t*>(base)));
    if (s.mask_bytes == 4) r->mask32 = reinterpret_cast<int32_t*>(base + rup(shares));
    if (s.mask_bytes == 8) r->mask64 = reinterpret_cast<int64_t*>(base + rup(shares));
    return SDA_OK;
}

}  // namespace

extern "C" {

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
    const uint64_t k = s.packed ? std::max<uint64_t>(ss->secret_count, 1) : 1;
    const uint64_t B = D / k + (D % k ? 1 : 0);
    JobRows rows;
    if (sda_status e = job_rows(h, s, n, B, D, &rows)) return e;
    const ParticipantRecords before(h);
    const KeyedDraws kd{key, share_stream_id};
    ParticipantJobArgs job;
    if (s.full) {
        job.mask_key = key;
        job.mask_stream_id = mask_stream_id;
        job.mask64 = rows.mask64;
        job.mask32 = rows.mask32;
    }
    uint64_t mask_len = 0;
    sda_status e = participant_share(h, ms, seed, seed_words, nullptr, ss, secrets, D, nullptr, mode, rows.sh64,
                                     rows.sh32, payload, payload_cap, payload_row_bytes, stream, &kd, &job);
    if (!e && s.chacha && seed_words != s.shape.seed_words)
        e = fail(SDA_ERR_PRECONDITION, "expected %llu seed words", (unsigned long long)s.shape.seed_words);
    // the recipient's mask payload (participate.rs:56-72)
    if (!e && s.full && D)
        e = rows.mask32 ? encode_rows(h, rows.mask32, 1, D, D, mask_payload, mask_payload_cap, &mask_len, st,
                                      "mask_payload_cap")
                        : encode_rows(h, rows.mask64, 1, D, D, mask_payload, mask_payload_cap, &mask_len, st,
                                      "mask_payload_cap");
    if (!e && s.chacha && seed_words) {
        const std::vector<uint8_t> bytes = encode_seed_words(seed, seed_words);
        mask_len = bytes.size();
        hipError_t he = hipMemcpyAsync(mask_payload, bytes.data(), bytes.size(), hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);             // `bytes` goes out of scope
        if (he != hipSuccess) {
            (void)hipGetLastError();
            e = fail(SDA_ERR_DEVICE, "the mask payload's copy failed: %s", hipGetErrorString(he));
        }
    }
    if (e) {
        before.restore(h);
        return e;
    }
    *mask_payload_len = mask_len;
    if (D) h->participant_job_last = {s.mask_route, h->participant_last.share_route, s.share_bytes, 1};
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
    const ParticipantRecords before(h);
    auto failed = [&](sda_status e) {           // nothing of this call stays queued, every record stays the previous call's
        if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
        (void)hipStreamSynchronize(h->stream);
        before.restore(h);
        return e;
    };
    const KeyedDraws kd{key, share_stream_id};
    std::vector<uint64_t> lens(n, 0);           // the clerks' running offsets; the caller's arrays are set at the end
    uint64_t mlen = 0;
    // ChaCha: the masked secrets over the whole vector first, by participant_share's masking step (the rejection
    // count is read there, before the first tile); the tiles then share and encode them as an unmasked job
    const int64_t* masked_all = nullptr;
    const sda_masking_scheme no_mask = {SDA_MASKING_NONE, 0, 0, 0};
    sda_engine::ParticipantLaunchInfo mask_rec;
    if (s.chacha) {
        DevArena a;
        if (sda_status e = stage(h, rup(D * 8 + 8), &a)) return e;
        int64_t* dsec = a.take<int64_t>(D + 1);
        if (D) HIP_TRY(hipMemcpyAsync(dsec, secrets, D * 8, hipMemcpyHostToDevice, h->stream));
        ParticipantJobArgs mj;
        mj.masked_out = &masked_all;
        if (sda_status e = participant_share(h, ms, seed, seed_words, nullptr, ss, dsec, D, nullptr, mode, nullptr,
                                             nullptr, nullptr, 0, nullptr, h->stream, &kd, &mj))
            return failed(e);
        if (seed_words != s.shape.seed_words)
            return failed(fail(SDA_ERR_PRECONDITION, "expected %llu seed words", (unsigned long long)s.shape.seed_words));
        mask_rec = h->participant_last;
        const std::vector<uint8_t> bytes = encode_seed_words(seed, seed_words);
        if (!bytes.empty()) memcpy(mask_payload, bytes.data(), bytes.size());
        mlen = bytes.size();
    }
    // Tiles of whole batches (Additive: columns).  Tile i + 1's secrets go up on the copy stream while tile i computes
    // and tile i - 1's payloads come down; each half of the pinned and of the device buffer is [secrets | clerk
    // payloads | mask payload].
    const char* ov = getenv("SDA_PARTICIPANT_TILE_BATCHES");
    const uint64_t override_units = ov && *ov && atoll(ov) > 0 ? (uint64_t)atoll(ov) : 0;
    const sda::ParticipantTilePlan plan =
        sda::participant_job_tiles(s.shape, D, s.share_bytes, host_stage_bytes(), override_units);
    const uint64_t k = s.packed ? std::max<uint64_t>(ss->secret_count, 1) : 1;
    const uint64_t te = std::min(D, plan.tile * k);         // secrets of a full tile
    const size_t sec_b = s.chacha ? 0 : rup(te * 8);
    const size_t pay_b = rup(n * plan.tile * sda::participant_share_bytes_bound(s.shape) + 64);
    const size_t mpay_b = s.full ? rup(te * sda::participant_mask_bytes_bound(s.shape) + 64) : 0;
    const size_t half = sec_b + pay_b + mpay_b;
    auto run_tiles = [&]() -> sda_status {
        if (plan.tiles) {
            if (sda_status e = host_stream_ensure(h, half, 0)) return e;
            for (int b = 0; b < 2; ++b)
                if (!h->d2h_done[b]) HIP_TRY(hipEventCreateWithFlags(&h->d2h_done[b], hipEventDisableTiming));
        }
        uint8_t* hp[2] = {static_cast<uint8_t*>(h->hs_pin), static_cast<uint8_t*>(h->hs_pin) + rup(half)};
        uint8_t* dv[2] = {static_cast<uint8_t*>(h->hs_dev), static_cast<uint8_t*>(h->hs_dev) + rup(half)};
        std::vector<uint64_t> row_bytes[2] = {std::vector<uint64_t>(n + 1, 0), std::vector<uint64_t>(n + 1, 0)};
        uint64_t mask_bytes[2] = {0, 0};
        auto tile_range = [&](uint64_t i, uint64_t* u0, uint64_t* s0, uint64_t* ds) {
            *u0 = i * plan.tile;
            *s0 = *u0 * k;
            *ds = std::min(D, std::min(plan.units, *u0 + plan.tile) * k) - *s0;   // the last batch may be short
        };
        auto upload = [&](uint64_t i) -> sda_status {
            uint64_t u0, s0, ds;
            tile_range(i, &u0, &s0, &ds);
            const int b = (int)(i & 1);
            memcpy(hp[b], secrets + s0, ds * 8);
            HIP_TRY(hipMemcpyAsync(dv[b], hp[b], ds * 8, hipMemcpyHostToDevice, h->copy_stream));
            HIP_TRY(hipEventRecord(h->h2d_done[b], h->copy_stream));
            return SDA_OK;
        };
        auto drain = [&](uint64_t i) -> sda_status {            // tile i's payloads: pinned memory -> the caller's blobs
            const int b = (int)(i & 1);
            HIP_TRY(hipEventSynchronize(h->d2h_done[b]));
            const uint8_t* src = hp[b] + sec_b;
            for (uint64_t c = 0; c < n; ++c) {
                if (row_bytes[b][c]) memcpy(clerk_payloads[c] + lens[c], src, row_bytes[b][c]);
                lens[c] += row_bytes[b][c];
                src += row_bytes[b][c];
            }
            if (mask_bytes[b]) memcpy(mask_payload + mlen, hp[b] + sec_b + pay_b, mask_bytes[b]);
            mlen += mask_bytes[b];
            return SDA_OK;
        };
        if (!s.chacha && plan.tiles)
            if (sda_status e = upload(0)) return e;
        for (uint64_t i = 0; i < plan.tiles; ++i) {
            uint64_t u0, s0, ds;
            tile_range(i, &u0, &s0, &ds);
            const int b = (int)(i & 1);
            // the other half's secrets: tile i - 1 has computed (every tile ends with the wait for its payload sizes)
            if (!s.chacha && i + 1 < plan.tiles)
                if (sda_status e = upload(i + 1)) return e;
            if (!s.chacha) HIP_TRY(hipStreamWaitEvent(h->stream, h->h2d_done[b], 0));
            const uint64_t tb = std::min(plan.units, u0 + plan.tile) - u0;
            JobRows rows;
            if (sda_status e = job_rows(h, s, n, tb, ds, &rows)) return e;
            ParticipantJobArgs job;
            job.first = u0;
            if (s.full) {
                job.mask_key = key;
                job.mask_stream_id = mask_stream_id;
                job.mask64 = rows.mask64;
                job.mask32 = rows.mask32;
            }
            const int64_t* tsec = s.chacha ? masked_all + s0 : reinterpret_cast<const int64_t*>(dv[b]);
            uint8_t* dpay = dv[b] + sec_b;
            // this half's payload buffers: tile i - 2 was drained while tile i - 1 computed
            if (sda_status e = participant_share(h, s.chacha ? &no_mask : ms, seed, seed_words, nullptr, ss, tsec, ds, nullptr,
                                                 mode, rows.sh64, rows.sh32, dpay, pay_b, row_bytes[b].data(), h->stream,
                                                 &kd, &job))
                return e;
            mask_bytes[b] = 0;
            if (s.full && ds)
                if (sda_status e = rows.mask32 ? encode_rows(h, rows.mask32, 1, ds, ds, dpay + pay_b, mpay_b, &mask_bytes[b],
                                                             h->stream, "the mask payload's tile")
                                               : encode_rows(h, rows.mask64, 1, ds, ds, dpay + pay_b, mpay_b, &mask_bytes[b],
                                                             h->stream, "the mask payload's tile"))
                    return e;
            // both encodes have been waited for: the copy stream may read the payloads now
            uint64_t total = 0;
            for (uint64_t c = 0; c < n; ++c) total += row_bytes[b][c];
            if (total) HIP_TRY(hipMemcpyAsync(hp[b] + sec_b, dpay, total, hipMemcpyDeviceToHost, h->copy_stream));
            if (mask_bytes[b])
                HIP_TRY(hipMemcpyAsync(hp[b] + sec_b + pay_b, dpay + pay_b, mask_bytes[b], hipMemcpyDeviceToHost,
                                       h->copy_stream));
            HIP_TRY(hipEventRecord(h->d2h_done[b], h->copy_stream));
            if (i >= 1)
                if (sda_status e = drain(i - 1)) return e;
        }
        if (plan.tiles)
            if (sda_status e = drain(plan.tiles - 1)) return e;
        return SDA_OK;
    };
    if (sda_status e = run_tiles()) return failed(e);
    for (uint64_t c = 0; c < n; ++c) clerk_lens[c] = lens[c];
    *mask_len = mlen;
    if (D) {
        if (s.chacha) {                         // the tiles ran as an unmasked job: the mask step's routes stand
            h->participant_last.mask_route = mask_rec.mask_route;
            h->participant_last.passes = mask_rec.passes;
        }
        h->participant_job_last = {s.mask_route, h->participant_last.share_route, s.share_bytes, plan.tiles};
    }
    return finish(h);
}

sda_status sda_participant_job_last_launch(sda_engine* h, uint32_t* mask_route, uint32_t* share_route,
                                           uint32_t* share_bytes, uint64_t* tiles) {
    SDA_ENTRY;
    if (!h || !mask_route || !share_route || !share_bytes || !tiles) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // a host-side record, final when the call that made it returned: nothing to wait for
    const sda_engine::ParticipantJobLaunchInfo& r = h->participant_job_last;
    *mask_route = r.mask_route;
    *share_route = r.share_route;
    *share_bytes = r.share_bytes;
    *tiles = r.tiles;
    return ok();
}

}  // extern "C"
