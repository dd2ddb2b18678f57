// engine_codec.cpp -- the host side of the share payload codec (varint encode / decode, the clerk's decode +
// combine over device-resident blobs) and the snapshot transposition of the C ABI (include/sda_engine.h).
#include "engine_internal.h"

using namespace sda_host;

// ---------------- share payload codec (sodium.rs:36-41 / :82-88) ----------------
template <typename T>
sda_status sda_host::encode_rows(sda_engine* h, const T* vals, uint64_t rows, uint64_t len, uint64_t stride,
                                 uint8_t* dst, uint64_t dst_cap, uint64_t* row_bytes, hipStream_t st,
                                 const char* cap_name) {
    constexpr bool wide = sizeof(T) == 8;
    if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes,
                              wide ? sda::varint_encode_work_bytes(rows, len) : sda::varint_encode32_work_bytes(rows, len)))
        return e;
    hipError_t e;
    if constexpr (wide) e = sda::launch_varint_encode(vals, rows, len, stride, dst, dst_cap, h->codec_work, row_bytes, st);
    else e = sda::launch_varint_encode32(vals, rows, len, stride, dst, dst_cap, h->codec_work, row_bytes, st);
    if (e == hipErrorInvalidValue) return fail(SDA_ERR_INVALID_ARGUMENT, "%s too small", cap_name);
    HIP_TRY(e);
    return SDA_OK;
}
template sda_status sda_host::encode_rows(sda_engine*, const int64_t*, uint64_t, uint64_t, uint64_t, uint8_t*, uint64_t,
                                          uint64_t*, hipStream_t, const char*);
template sda_status sda_host::encode_rows(sda_engine*, const int32_t*, uint64_t, uint64_t, uint64_t, uint8_t*, uint64_t,
                                          uint64_t*, hipStream_t, const char*);

// The argument checks and the launch of sda_varint_encode_dev and sda_varint_encode32_dev.
template <typename T>
static sda_status encode_dev(sda_engine* h, const T* vals, uint64_t rows, uint64_t len, uint64_t stride, uint8_t* dst,
                             uint64_t dst_cap, uint64_t* row_bytes, void* stream) {
    if (!h || !row_bytes || (rows && len && (!vals || !dst))) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (rows > 65535) return fail(SDA_ERR_UNSUPPORTED, "at most 65535 rows per call");
    if (stride < len) return fail(SDA_ERR_INVALID_ARGUMENT, "stride < len");
    HIP_TRY(hipSetDevice(h->device));
    if (sda_status e = encode_rows(h, vals, rows, len, stride, dst, dst_cap, row_bytes, pick(h, stream), "dst_cap"))
        return e;
    return ok();
}

// Shared with the recipient job (engine_recipient.cpp): declared in engine_internal.h.
namespace sda_host {

sda_status check_blob_buffer(const uint8_t* bytes, const uint64_t* blob_off, uint64_t n_blobs) {
    if (((uintptr_t)bytes & 15) != 0) return fail(SDA_ERR_INVALID_ARGUMENT, "byte buffer must be 16-byte aligned");
    for (uint64_t b = 0; b < n_blobs; ++b)
        if (blob_off[b + 1] < blob_off[b]) return fail(SDA_ERR_INVALID_ARGUMENT, "blob offsets must be non-decreasing");
    return SDA_OK;
}

// Plan + count N device-resident blobs; counts[n] on the host.
sda_status codec_count(sda_engine* h, const uint8_t* bytes, const uint64_t* blob_off, uint64_t n_blobs,
                       sda::VarintPlan* plan, uint64_t* counts, bool* irregular, hipStream_t st,
                       bool sub_counts, bool* long_any) {
    if (sda_status e = check_blob_buffer(bytes, blob_off, n_blobs)) return e;
    sda::varint_plan(blob_off, n_blobs, plan);
    if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes,
                              sda::varint_decode_work_bytes(plan->regions, n_blobs)))
        return e;
    HIP_TRY(sda::launch_varint_count(bytes, blob_off, n_blobs, *plan, h->codec_work, counts, irregular, st,
                                     sub_counts, long_any));
    return SDA_OK;
}

// decode + combiner.rs:16-28 over device-resident blobs; out (device) gets out_len = count of blob 0.  With a job:
// out is the job's state, continued in place from prior_dim columns when job->first > 0, and the result is encoded
// into job->payload -- behind the combine, before the call's one wait, on the slot path (route 1), else once the
// counts are known (route 2).
sda_status decode_combine(sda_engine* h, int64_t m, const uint8_t* bytes, const uint64_t* blob_off, uint64_t n_blobs,
                          int64_t* out, uint64_t out_cap, uint64_t* out_len, hipStream_t st,
                          const ClerkJob* job) {
    const bool cont = job && job->first > 0;
    const uint64_t prior = cont ? job->prior_dim : 0, first = cont ? job->first : 0;
    *out_len = prior;
    if (job && job->payload_len) *job->payload_len = 0;
    // sda_codec_last_launch: NONE until this call returns SDA_OK; `info` collects each decision where it is taken
    h->last.codec = sda::CodecLaunchInfo();
    sda::CodecLaunchInfo info;
    // sda_clerk_job_last_launch: written by conclude() when the call ends well after launching something
    sda_engine::ClerkJobLaunchInfo rec;
    rec.continued = cont;
    // the result on the host-length encoder, or the record alone when no payload is asked for
    auto conclude = [&](uint64_t dim, bool launched) -> sda_status {
        if (!job) return SDA_OK;
        if (job->payload && dim) {
            uint64_t nbytes = 0;
            const sda_status e = encode_rows(h, (const int64_t*)out, 1, dim, dim, job->payload, job->payload_cap, &nbytes,
                                             st, "payload_cap");
            *job->payload_len = nbytes;                             // the count needed when payload_cap is too small
            if (e) return e;
            rec.encode_route = 2;
            rec.encode_chunks = sda::varint_encode_chunks(dim);
            launched = true;
        } else if (job->payload) {
            rec.encode_route = 2;
        }
        if (launched) h->last.clerk_job = rec;
        return SDA_OK;
    };
    if (cont) {
        if (prior > out_cap) return fail(SDA_ERR_INVALID_ARGUMENT, "prior_dim %llu > state_cap %llu",
                                         (unsigned long long)prior, (unsigned long long)out_cap);
        int64_t mm;                                                 // row 0 was folded by an earlier call
        if (prior)
            if (sda_status e = modulus_abs(m, &mm)) return e;
    }
    if (n_blobs == 0) {                                             // combiner.rs:17: empty input; the finish call
        if (sda_status e = conclude(prior, false)) return e;
        return ok();
    }
    // SDA_CODEC_PATH=fused (A/B and test knob) runs the column-tile decode+combine, which reads the payload
    // once instead of writing and re-reading an int32 matrix but measured slower (VALU-bound: 3.4 ms per
    // 1000 x 1M launch vs 2.2 + 0.7 ms, profiles/r02d/ab_codec_fused.txt); the default is the matrix path.
    // The fused kernel has no accumulating form: a continuing call asked for it takes the matrix path.
    const char* path = getenv("SDA_CODEC_PATH");
    const bool want_fused = path && strcmp(path, "fused") == 0;
    const bool force_fused = want_fused && !cont, force_matrix = !force_fused;
    const char* env = getenv("SDA_CODEC_NARROW");                    // "0": A/B and test knob
    const bool narrow_ok = !(env && atoi(env) == 0);
    sda::VarintPlan plan;
    std::vector<uint64_t> counts(n_blobs);
    // the reference's checks once the counts are known: `% 0` on row 0 before a later row's "Wrong dimension";
    // a continuing call's blob 0 is an ordinary row of the established dimension
    auto check = [&](uint64_t dim, int64_t* mm) -> sda_status {
        if (!cont && dim && m == 0) return modulus_abs(m, mm);      // blob 0 is folded first (combiner.rs:20-25)
        for (uint64_t i = cont ? 0 : 1; i < n_blobs; ++i)
            if (counts[i] != dim)
                return fail(SDA_ERR_WRONG_DIMENSION,
                            "Wrong dimension (participation %llu decodes to %llu shares, expected %llu)",
                            (unsigned long long)(first + i), (unsigned long long)counts[i], (unsigned long long)dim);
        if (dim) {
            if (sda_status e = modulus_abs(m, mm)) return e;
        }
        if (out_cap < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
        return SDA_OK;
    };
    // Default: decode once into int32 slots per 16 KiB region (no count pass), then the exact combine
    // over the slots.  SDA_CODEC_PATH=matrix (A/B and test knob) takes the count pass + dense int32
    // matrix path; any element longer than 5 bytes or outside int32 (malformed or raw i64 payloads)
    // falls back to it as well.
    if (narrow_ok && !want_fused && !(path && strcmp(path, "matrix") == 0)) {
        if (sda_status e = check_blob_buffer(bytes, blob_off, n_blobs)) return e;
        sda::varint_plan(blob_off, n_blobs, &plan);
        if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes,
                                  sda::varint_decode_work_bytes(plan.regions, n_blobs)))
            return e;
        // the slots are sized by the bytes, the tile plan by the dimension (<= the bytes of blob 0)
        const uint64_t dim_max = cont ? prior : blob_off[1] - blob_off[0];
        if (sda_status e = ensure(&h->codec_mat, &h->codec_mat_bytes, sda::varint_slot_bytes(plan, n_blobs, dim_max)))
            return e;
        sda::SlotJob sj;
        if (job) {
            sj.continued = cont;
            sj.prior_dim = prior;
            if (job->payload) {                // its own workspace: codec_work holds the counts until the wait
                if (sda_status e = ensure(&h->job_work, &h->job_work_bytes, sda::varint_encode_work_bytes(1, dim_max)))
                    return e;
                sj.payload = job->payload;
                sj.payload_cap = job->payload_cap;
                sj.enc_work = h->job_work;
            }
        }
        // everything is queued before the host sees a count: the combine itself exits when a flag is set
        // or blob 0's count exceeds out_cap, and the checks below then report it in the reference's order
        const bool m_ok = m != 0 && m != INT64_MIN;
        uint32_t flags = 0;
        HIP_TRY(sda::launch_varint_decode_slots_combine(bytes, blob_off, n_blobs, plan, h->codec_work, h->codec_mat,
                                                        out, out_cap, m_ok ? (m < 0 ? -m : m) : 0, counts.data(),
                                                        &flags, st, &info, job ? &sj : nullptr));
        if (!(flags & 1u)) {
            const uint64_t dim = cont ? prior : counts[0];
            int64_t mm = 1;
            if (sda_status e = check(dim, &mm)) return e;
            *out_len = dim;
            h->last.codec = info;
            if (!job) return SDA_OK;
            if (job->payload && dim && !sj.encoded) return conclude(dim, true);      // not reached: dim > 0 queues it
            if (job->payload) {
                rec.encode_route = 1;
                rec.encode_chunks = sj.enc_chunks;
                *job->payload_len = dim ? sj.payload_bytes : 0;
                if (dim && sj.payload_bytes > job->payload_cap)
                    return fail(SDA_ERR_INVALID_ARGUMENT, "payload_cap too small (%llu bytes needed)",
                                (unsigned long long)sj.payload_bytes);
            }
            h->last.clerk_job = rec;
            return SDA_OK;
        }
        info = sda::CodecLaunchInfo();                 // the slot attempt wrote nothing: the count pass takes over
        info.fell_back = sda::kCodecSlotWide;
    }
    bool irregular = false, long_elems = false;
    if (sda_status e = codec_count(h, bytes, blob_off, n_blobs, &plan, counts.data(), &irregular, st, !force_matrix,
                                   &long_elems))
        return e;
    const uint64_t dim = cont ? prior : counts[0];
    int64_t mm;
    if (sda_status e = check(dim, &mm)) return e;
    *out_len = dim;
    if (dim == 0) {
        if (sda_status e = conclude(0, true)) return e;
        return ok();
    }
    if (force_fused && irregular) info.fell_back |= sda::kCodecFusedIrregular;
    if (!irregular && force_fused) {
        // one pass over the payload: no [N][dim] matrix (the matrix buffer holds the tile plan)
        if (sda_status e = ensure(&h->codec_mat, &h->codec_mat_bytes, sda::varint_tile_plan_bytes(n_blobs, dim)))
            return e;
        HIP_TRY(sda::launch_varint_decode_combine(bytes, n_blobs, plan, h->codec_work,
                                                  static_cast<uint64_t*>(h->codec_mat), dim, out, mm, long_elems, st,
                                                  &info));
        h->last.codec = info;
        return conclude(dim, true);
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
            HIP_TRY(sda::launch_combine_exact32(mat32, n_blobs, dim, dim, out, mm, st, cont, &h->last.combine));
            info.path = sda::kCodecMatrix32;
            h->last.codec = info;
            return conclude(dim, true);
        }
        info.fell_back |= sda::kCodecNarrowWide;
    }
    int64_t* mat = static_cast<int64_t*>(h->codec_mat);
    HIP_TRY(sda::launch_varint_decode(bytes, n_blobs, plan, h->codec_work, mat, dim, dim, irregular, st, &info));
    HIP_TRY(sda::launch_combine_exact(mat, n_blobs, dim, dim, out, mm, st, cont, &h->last.combine));
    info.path = sda::kCodecMatrix64;
    h->last.codec = info;
    return conclude(dim, true);
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

}  // namespace sda_host

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
    // blob groups streamed through pinned double buffers, decoded and combined on device (engine_host.cpp)
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
    if (sda_status e = check_blob_buffer(bytes, blob_off, n_blobs)) return e;
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

// The clerk's arithmetic step (clerk.rs:63-107 between the sealed boxes): decode, combine -- continued from `state`
// when first_participation > 0 -- and the recipient's payload, one call with one wait.
sda_status sda_clerk_job_dev(sda_engine* h, int64_t modulus, const uint8_t* bytes, const uint64_t* blob_off,
                             uint64_t n_blobs, uint64_t first_participation, uint64_t prior_dim, int64_t* state,
                             uint64_t state_cap, uint64_t* dim_out, uint8_t* payload, uint64_t payload_cap,
                             uint64_t* payload_len, void* stream) {
    SDA_ENTRY;
    if (!h || !dim_out || (payload && !payload_len) || (n_blobs && (!bytes || !blob_off)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    if (first_participation && prior_dim && !state) return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    const ClerkJob job = {first_participation, prior_dim, payload, payload_cap, payload_len};
    if (sda_status e = decode_combine(h, modulus, bytes, blob_off, n_blobs, state, state_cap, dim_out,
                                      pick(h, stream), &job))
        return e;
    return ok();
}

sda_status sda_clerk_job(sda_engine* h, const sda_sharing_scheme* s, const uint8_t* const* blobs,
                         const uint64_t* blob_lens, uint64_t n_blobs, int64_t* out, uint64_t out_cap,
                         uint64_t* out_len, uint8_t* payload, uint64_t payload_cap, uint64_t* payload_len) {
    SDA_ENTRY;
    if (!h || !s || !out_len || !payload_len || (n_blobs && (!blobs || !blob_lens)))
        return fail(SDA_ERR_INVALID_ARGUMENT, "NULL argument");
    *out_len = 0;
    *payload_len = 0;
    for (uint64_t i = 0; i < n_blobs; ++i)
        if (blob_lens[i] && !blobs[i]) return fail(SDA_ERR_INVALID_ARGUMENT, "blob %llu is NULL", (unsigned long long)i);
    HIP_TRY(hipSetDevice(h->device));
    (void)pick(h, h->stream);
    // the streamed decode -> combine of sda_clerk_decode_combine; its accumulator stays on the device
    int64_t* acc = nullptr;
    if (sda_status st = host_decode_combine(h, s->modulus, blobs, blob_lens, n_blobs, out, out_cap, out_len, &acc))
        return st;
    const uint64_t dim = *out_len;
    if (dim == 0) return ok();
    // the recipient's payload from the accumulator: about 4.9 bytes per field share cross PCIe instead of 8
    DevArena a;
    if (sda_status st = stage(h, rup(dim * 10 + 16), &a)) return st;
    uint8_t* db = a.take<uint8_t>(dim * 10 + 16);
    uint64_t nbytes = 0;
    if (sda_status st = encode_rows(h, (const int64_t*)acc, 1, dim, dim, db, dim * 10 + 16, &nbytes, h->stream, "payload"))
        return st;
    *payload_len = nbytes;
    if (!payload || nbytes > payload_cap)
        return fail(SDA_ERR_INVALID_ARGUMENT, "payload_cap too small (%llu bytes needed)", (unsigned long long)nbytes);
    HIP_TRY(hipMemcpyAsync(payload, db, nbytes, hipMemcpyDeviceToHost, h->stream));
    if (sda_status st = finish(h)) return st;
    h->last.clerk_job = {0u, 2u, sda::varint_encode_chunks(dim)};
    return SDA_OK;
}

sda_status sda_varint_encode_dev(sda_engine* h, const int64_t* vals, uint64_t rows, uint64_t len, uint64_t stride,
                                 uint8_t* dst, uint64_t dst_cap, uint64_t* row_bytes, void* stream) {
    SDA_ENTRY;
    return encode_dev(h, vals, rows, len, stride, dst, dst_cap, row_bytes, stream);
}

sda_status sda_varint_encode32_dev(sda_engine* h, const int32_t* vals, uint64_t rows, uint64_t len, uint64_t stride,
                                   uint8_t* dst, uint64_t dst_cap, uint64_t* row_bytes, void* stream) {
    SDA_ENTRY;
    return encode_dev(h, vals, rows, len, stride, dst, dst_cap, row_bytes, stream);
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
    // sda_snapshot_last_launch: collected here, the handle's record only once this call returns SDA_OK
    sda::SnapshotLaunchInfo info;
    info.chunk_bytes = chunk;
    for (uint64_t c = 0; c < n; ++c)
        for (uint64_t p = 0; p < P; ++p) {
            const uint64_t len = part_off[p * n + c + 1] - part_off[p * n + c];
            if (!len) continue;
            blobs.push_back({part_off[p * n + c], clerk_base[c] + clerk_off[c * (P + 1) + p], len});
            cstart.push_back(cstart.back() + (len + chunk - 1) / chunk);
            info.shifts |= 1u << ((blobs.back().src - blobs.back().dst) & 15);
        }
    info.blobs = blobs.size();
    info.chunks = cstart.back();
    if (blobs.empty()) {
        h->last.snapshot = info;
        return ok();
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = pick(h, stream);
    const size_t b0 = rup(blobs.size() * sizeof(sda::SnapshotCopy));
    if (sda_status e = ensure(&h->snap, &h->snap_bytes, b0 + rup(cstart.size() * 8))) return e;
    char* plan = static_cast<char*>(h->snap);
    HIP_TRY(hipMemcpyAsync(plan, blobs.data(), blobs.size() * sizeof(sda::SnapshotCopy), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(plan + b0, cstart.data(), cstart.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(sda::launch_snapshot_transpose(src, dst, reinterpret_cast<const sda::SnapshotCopy*>(plan),
                                           reinterpret_cast<const uint64_t*>(plan + b0), blobs.size(),
                                           cstart.back(), st, &info.grid));
    HIP_TRY(hipStreamSynchronize(st));                             // the host plan vectors go out of scope
    h->last.snapshot = info;
    return ok();
}

}  // extern "C"
