// engine_dev.cpp -- the device-resident (`_dev`) entry points of the C ABI (include/sda_engine.h): raw device
// pointers in and out, on the caller's stream.  The packed-Shamir launch helpers that the pipelines and the host path
// share are defined here.
#include "engine_internal.h"

namespace sda_host __attribute__((visibility("hidden"))) {

sda_status packed_generate(sda_engine* h, const sda_sharing_scheme* s, sda::PackedGenArgs ga, hipStream_t st) {
    const uint32_t k = (uint32_t)s->secret_count, t = (uint32_t)s->privacy_threshold, n = (uint32_t)s->share_count;
    if (sda_status e = ensure(&h->gen_log, &h->gen_log_bytes, sda::packed_gen_log_bytes())) return e;
    // the launcher plans the call with the same function: the scratch sized here is the scratch its kernels use
    const sda::PackedGenPlan pl = sda::packed_gen_plan(ga, k, t, n, (uint32_t)s->modulus);
    if (const size_t tmp = pl.narrow_bytes) {
        if (sda_status e = ensure(&h->gen32_tmp, &h->gen32_tmp_bytes, tmp + 64)) return e;
        ga.scratch = static_cast<int64_t*>(h->gen32_tmp);
        ga.flag = ga.scratch + tmp / sizeof(int64_t);          // launch_narrow32's overflow word: never set here
    }
    if (pl.draw_bytes) {      // keyed, staged in handle-owned scratch (path 2; path 1 makes them in the share kernels)
        if (sda_status e = ensure(&h->keyed_draws, &h->keyed_draws_bytes, rup(pl.draw_bytes + 8))) return e;
        ga.draw_scratch = static_cast<int64_t*>(h->keyed_draws);
    }
    HIP_TRY(sda::launch_packed_generate(ga, k, t, n, (uint32_t)s->modulus, (uint32_t)s->omega_secrets,
                                        (uint32_t)s->omega_shares, h->gen_tab, h->gen_log, st, &h->gen_log_used));
    if (pl.keyed_path && ga.dimension && ga.n_vectors) {        // sda_packed_keyed_last_launch
        h->last.keyed_path = pl.keyed_path;
        h->last.keyed_staged_bytes = pl.draw_bytes;
    }
    return SDA_OK;
}

sda_status packed_reveal(sda_engine* h, const sda_sharing_scheme* s, const sda::PackedRevealArgs& ra,
                         const uint64_t* indices, uint64_t n_idx, int32_t mode, hipStream_t st, bool* refused) {
    if (refused) *refused = false;
    if (sda_status e = ensure(&h->gen_log, &h->gen_log_bytes, sda::packed_gen_log_bytes())) return e;
    const hipError_t e = sda::launch_packed_reveal(ra, indices, (uint32_t)n_idx, (uint32_t)s->secret_count,
                                                   (uint32_t)s->privacy_threshold, (uint32_t)s->modulus,
                                                   (uint32_t)s->omega_secrets, (uint32_t)s->omega_shares, mode,
                                                   h->rev_tab, h->gen_log, st, &h->gen_log_used);
    if (e == hipErrorInvalidValue && mode == SDA_REVEAL_CANONICAL) {
        if (refused) *refused = true;
        return fail(SDA_ERR_UNSUPPORTED, "canonical reveal needs distinct clerk indices");
    }
    HIP_TRY(e);
    return SDA_OK;
}

}  // namespace sda_host

using namespace sda_host;

// The four combine entry points: T is the share rows' element type, `accumulate` continues the recurrence from
// inout.  The accumulate forms have nothing to do for n == 0 (inout stays); the plain forms launch (out = 0).
template <typename T>
static sda_status combine_dev(sda_engine* h, int64_t modulus, const T* shares, uint64_t n, uint64_t dim,
                              uint64_t row_stride, int64_t* out, void* stream, bool accumulate) {
    if (!h || (dim && (!out || (n && !shares)))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n > 1 && row_stride < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "row_stride < dim");
    int64_t m;
    if (sda_status st = modulus_abs(modulus, &m)) return st;
    HIP_TRY(hipSetDevice(h->device));
    if (accumulate && n == 0) return ok();
    const uint64_t stride = n > 1 ? row_stride : dim;
    if constexpr (sizeof(T) == 8)
        HIP_TRY(sda::launch_combine_exact(shares, n, dim, stride, out, m, pick(h, stream), accumulate, &h->last.combine));
    else
        HIP_TRY(sda::launch_combine_wide32(shares, n, dim, stride, out, m, pick(h, stream), accumulate,
                                           &h->last.combine));
    return ok();
}

// Both reconstruct entry points, T the share type; the NULL-argument check is the int32 one's alone, as it has been.
template <typename T>
static sda_status packed_reconstruct(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                     const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors, const T* shares,
                                     int64_t* out, int32_t mode, void* stream) {
    if (!h || !s || s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (sda_status st = check_packed(s)) return st;
    if (mode != SDA_REVEAL_EXACT && mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
    if (dimension == 0) return ok();                        // batched.rs:77-81: no batch, no check
    if (n_idx < s->privacy_threshold + s->secret_count)
        return fail(SDA_ERR_NOT_ENOUGH_SHARES, "Not enough shares to reconstruct");
    if (n_idx > sda::kRevealMaxShares)
        return fail(SDA_ERR_UNSUPPORTED, "more than %u clerk shares per batch", sda::kRevealMaxShares);
    if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
    if (sizeof(T) == 4 && n_vectors && (!out || !shares || !indices)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    sda::PackedRevealArgs ra{nullptr, dimension, n_vectors, out};
    if constexpr (sizeof(T) == 4) ra.shares32 = shares; else ra.shares = shares;
    if (sda_status e = packed_reveal(h, s, ra, indices, n_idx, mode, pick(h, stream))) return e;
    return ok();
}

extern "C" {

// ---------------- device-resident entry points ----------------
sda_status sda_combine_dev(sda_engine* h, int64_t modulus, const int64_t* shares, uint64_t n, uint64_t dim,
                           uint64_t row_stride, int64_t* out, void* stream) {
    SDA_ENTRY;
    return combine_dev(h, modulus, shares, n, dim, row_stride, out, stream, false);
}

sda_status sda_combine_accumulate_dev(sda_engine* h, int64_t modulus, const int64_t* shares, uint64_t n,
                                      uint64_t dim, uint64_t row_stride, int64_t* inout, void* stream) {
    SDA_ENTRY;
    return combine_dev(h, modulus, shares, n, dim, row_stride, inout, stream, true);
}

// int32 share rows (|v| < 2^31: every shipped configuration): half the bytes per share; the kernels sign-extend
// and run the i64 recurrence, so the result is that of the widened rows for any modulus
sda_status sda_combine32_dev(sda_engine* h, int64_t modulus, const int32_t* shares, uint64_t n, uint64_t dim,
                             uint64_t row_stride, int64_t* out, void* stream) {
    SDA_ENTRY;
    return combine_dev(h, modulus, shares, n, dim, row_stride, out, stream, false);
}

sda_status sda_combine32_accumulate_dev(sda_engine* h, int64_t modulus, const int32_t* shares, uint64_t n,
                                        uint64_t dim, uint64_t row_stride, int64_t* inout, void* stream) {
    SDA_ENTRY;
    return combine_dev(h, modulus, shares, n, dim, row_stride, inout, stream, true);
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
                                      &h->last.combine));
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
                                       m, pick(h, stream), &h->last.combine));
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
    if (sda_status st = packed_generate(h, s, ga, pick(h, stream))) return st;
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
    if (sda_status st = packed_generate(h, s, ga, pick(h, stream))) return st;
    return ok();
}

sda_status sda_packed_reconstruct_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                      const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                      const int64_t* shares, int64_t* out, int32_t mode, void* stream) {
    SDA_ENTRY;
    return packed_reconstruct(h, s, dimension, indices, n_idx, n_vectors, shares, out, mode, stream);
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
    if (sda_status st = packed_generate(h, s, ga, pick(h, stream))) return st;
    return ok();
}

sda_status sda_packed_reconstruct32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                        const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                        const int32_t* shares, int64_t* out, int32_t mode, void* stream) {
    SDA_ENTRY;
    return packed_reconstruct(h, s, dimension, indices, n_idx, n_vectors, shares, out, mode, stream);
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

}  // extern "C"

// Both keyed Additive entry points: the header's checks in its order, then the fused kernel (additive_keyed.hip).
template <typename Out>
static sda_status additive_generate_keyed(sda_engine* h, int64_t modulus, uint64_t share_count, const int64_t* secrets,
                                          uint64_t dimension, const uint32_t* key, uint32_t stream_id,
                                          uint64_t first_column, Out* out, uint64_t out_stride, void* stream) {
    if (!h || !key || (dimension && (!secrets || !out)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL handle, key or needed buffer");
    if (share_count == 0) return fail(SDA_ERR_PRECONDITION, "share_count - 1 underflows (additive.rs:42)");
    if (modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    if (out_stride < dimension) return fail(SDA_ERR_INVALID_ARGUMENT, "out_stride is smaller than the dimension");
    uint64_t end, elems;
    if (share_count > 1 && (__builtin_add_overflow(first_column, dimension, &end) ||
                            __builtin_mul_overflow(end, share_count - 1, &elems)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "(first_column + dimension) * (share_count - 1) wraps past 2^64");
    if (sizeof(Out) == 4 && modulus > (int64_t)1 << 31)
        return fail(SDA_ERR_UNSUPPORTED, "int32 shares need modulus <= 2^31: a draw in [0, modulus) need not fit int32");
    if (dimension == 0) return ok();
    HIP_TRY(hipSetDevice(h->device));
    int64_t* o64 = nullptr;
    int32_t* o32 = nullptr;
    if constexpr (sizeof(Out) == 4) o32 = out; else o64 = out;
    HIP_TRY(sda::launch_additive_generate_keyed(key, stream_id, first_column, secrets, dimension, share_count, modulus,
                                                o64, o32, out_stride, pick(h, stream)));
    return ok();
}

// Both keyed packed entry points: the unkeyed entry points' checks in their order, then the key and the wrap.
template <typename Out>
static sda_status packed_generate_keyed(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets,
                                        uint64_t dimension, uint64_t n_vectors, const uint32_t* key,
                                        uint32_t stream_id, uint64_t first_batch, Out* out, int32_t mode,
                                        void* stream) {
    if (!h || !s || s->kind != SDA_SHARING_PACKED_SHAMIR) return fail(SDA_ERR_INVALID_ARGUMENT, "need a PackedShamir scheme");
    if (mode != SDA_REVEAL_EXACT && mode != SDA_REVEAL_CANONICAL) return fail(SDA_ERR_INVALID_ARGUMENT, "bad mode");
    if (sda_status st = check_packed(s)) return st;
    if (n_vectors > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 vectors per launch");
    if (dimension && n_vectors && (!out || !secrets)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!key) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL key");
    const uint64_t k = s->secret_count, t = s->privacy_threshold, B = dimension / k + (dimension % k ? 1 : 0);
    uint64_t end, elems;                                       // n_vectors B <= 65535 * 2^64 / k may itself wrap
    if (t && (__builtin_mul_overflow(n_vectors, B, &end) || __builtin_add_overflow(end, first_batch, &end) ||
              __builtin_mul_overflow(end, t, &elems)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "(first_batch + n_vectors * B) * t wraps past 2^64");
    HIP_TRY(hipSetDevice(h->device));
    sda::PackedGenArgs ga{secrets, dimension, n_vectors, nullptr, nullptr, mode == SDA_REVEAL_CANONICAL};
    if constexpr (sizeof(Out) == 4) ga.out32 = out; else ga.out = out;
    ga.key = key;
    ga.stream_id = stream_id;
    ga.first_batch = first_batch;
    if (sda_status st = packed_generate(h, s, ga, pick(h, stream))) return st;
    return ok();
}

extern "C" {

sda_status sda_packed_generate_keyed_dev(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets,
                                         uint64_t dimension, uint64_t n_vectors, const uint32_t* key,
                                         uint32_t stream_id, uint64_t first_batch, int64_t* out, int32_t mode,
                                         void* stream) {
    SDA_ENTRY;
    return packed_generate_keyed(h, s, secrets, dimension, n_vectors, key, stream_id, first_batch, out, mode, stream);
}

sda_status sda_packed_generate_keyed32_dev(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets,
                                           uint64_t dimension, uint64_t n_vectors, const uint32_t* key,
                                           uint32_t stream_id, uint64_t first_batch, int32_t* out, int32_t mode,
                                           void* stream) {
    SDA_ENTRY;
    return packed_generate_keyed(h, s, secrets, dimension, n_vectors, key, stream_id, first_batch, out, mode, stream);
}

sda_status sda_packed_keyed_last_launch(sda_engine* h, uint32_t* path, uint64_t* staged_bytes) {
    SDA_ENTRY;
    if (!h || !path || !staged_bytes) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *path = h->last.keyed_path;
    *staged_bytes = h->last.keyed_staged_bytes;
    return ok();
}

sda_status sda_additive_generate_keyed_dev(sda_engine* h, int64_t modulus, uint64_t share_count, const int64_t* secrets,
                                           uint64_t dimension, const uint32_t* key, uint32_t stream_id,
                                           uint64_t first_column, int64_t* out, uint64_t out_stride, void* stream) {
    SDA_ENTRY;
    return additive_generate_keyed(h, modulus, share_count, secrets, dimension, key, stream_id, first_column, out,
                                   out_stride, stream);
}

sda_status sda_additive_generate_keyed32_dev(sda_engine* h, int64_t modulus, uint64_t share_count,
                                             const int64_t* secrets, uint64_t dimension, const uint32_t* key,
                                             uint32_t stream_id, uint64_t first_column, int32_t* out,
                                             uint64_t out_stride, void* stream) {
    SDA_ENTRY;
    return additive_generate_keyed(h, modulus, share_count, secrets, dimension, key, stream_id, first_column, out,
                                   out_stride, stream);
}

sda_status sda_chacha_mask_combine_dev(sda_engine* h, int64_t modulus, uint64_t dimension, const uint32_t* seeds,
                                       uint64_t w, uint64_t n_seeds, int64_t* out, void* stream) {
    SDA_ENTRY;
    if (!h || (dimension && !out) || (n_seeds && w && !seeds)) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    // chacha.rs:69 gen_range(0, m) runs once per seed and element: no seed, no draw, whatever the modulus
    if (dimension && n_seeds && modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    if (w == 0 || w > 8) return fail(SDA_ERR_INVALID_ARGUMENT, "seed width must be 1..8 words");
    HIP_TRY(hipSetDevice(h->device));
    if (dimension && n_seeds == 0 && modulus <= 0) {        // chacha.rs:58 vec![0; self.dimension]: no kernel sees m
        HIP_TRY(hipMemsetAsync(out, 0, dimension * 8, pick(h, stream)));
        return ok();
    }
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

}  // extern "C"

// sda_full_mask_keyed_dev and its 32 form: the checks in sda_draws_dev's order, then mask_keyed.hip's kernel.
template <typename MaskOut>
static sda_status full_mask_keyed(sda_engine* h, int64_t modulus, const int64_t* secrets, uint64_t D,
                                  const uint32_t* key, uint32_t stream_id, uint64_t first, int64_t* masked_out,
                                  MaskOut* mask_out, void* stream) {
    if (!h || !key || (D && (!secrets || !masked_out || !mask_out)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL handle, key or needed buffer");
    if (modulus <= 0) return fail(SDA_ERR_PRECONDITION, "Rng.gen_range called with low >= high");
    if (D && first + (D - 1) < first) return fail(SDA_ERR_INVALID_ARGUMENT, "first + count wraps past 2^64");
    if (sizeof(MaskOut) == 4 && modulus > (int64_t)1 << 31)
        return fail(SDA_ERR_UNSUPPORTED, "an int32 mask needs modulus <= 2^31: a mask value lies in [0, modulus)");
    if (D == 0) return ok();
    HIP_TRY(hipSetDevice(h->device));
    int64_t* m64 = nullptr;
    int32_t* m32 = nullptr;
    if constexpr (sizeof(MaskOut) == 4) m32 = mask_out; else m64 = mask_out;
    HIP_TRY(sda::launch_full_mask_keyed(key, stream_id, first, secrets, D, modulus, masked_out, m64, m32,
                                        pick(h, stream)));
    return ok();
}

extern "C" {

sda_status sda_full_mask_keyed_dev(sda_engine* h, int64_t modulus, const int64_t* secrets, uint64_t dimension,
                                   const uint32_t* key, uint32_t stream_id, uint64_t first, int64_t* masked_out,
                                   int64_t* mask_out, void* stream) {
    SDA_ENTRY;
    return full_mask_keyed(h, modulus, secrets, dimension, key, stream_id, first, masked_out, mask_out, stream);
}

sda_status sda_full_mask_keyed32_dev(sda_engine* h, int64_t modulus, const int64_t* secrets, uint64_t dimension,
                                     const uint32_t* key, uint32_t stream_id, uint64_t first, int64_t* masked_out,
                                     int32_t* mask_out, void* stream) {
    SDA_ENTRY;
    return full_mask_keyed(h, modulus, secrets, dimension, key, stream_id, first, masked_out, mask_out, stream);
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
