/*
 * sda_engine.h -- C ABI of the MI355X (gfx950) SDA secret-sharing engine.
 *
 * This is the drop-in boundary for the reference client's sharing and masking
 * traits (baajur/sda, client/src/crypto/{sharing,masking}/mod.rs).  A Rust FFI
 * shim implements the six traits on top of these entry points
 * and is selected in the factories at client/src/crypto/sharing/mod.rs:35-96
 * and client/src/crypto/masking/mod.rs:33-94.
 *
 * Conventions
 *   - sda_share_combine, the Full sda_mask_combine, the Additive sda_secret_reconstruct and
 *     sda_clerk_decode_combine stream their inputs through pinned double buffers in row tiles of
 *     SDA_HOST_STAGE_MB (default 256) MiB, so a job larger than HBM runs (bit-identical to one pass).
 *     The other host entry points (packed and additive generate, packed reconstruct, ChaCha mask
 *     combine, sda_recipient_reveal) stage their whole job -- or, on a multi-device handle, each
 *     device's share of it -- in device memory, and return OUT_OF_MEMORY past it.
 *   - Elements are i64 (client/src/crypto/mod.rs:33-36); arithmetic follows
 *     Rust: truncated `%`, wrapping `+` (release builds).
 *   - The caller owns every buffer.  Host entry points are synchronous (they
 *     return when results are in host memory), like the Rust trait calls.
 *   - Entry points suffixed `_dev` take DEVICE pointers and a hipStream_t
 *     (passed as void*; NULL = the HIP null stream, the same convention as the
 *     ROCm math libraries); they only enqueue work, except for the few host
 *     values they return: the ChaCha combine waits for its rejection log (a few
 *     bytes) mid-call; the recipient and participant pipelines with ChaCha
 *     masking, and the varint encode (row sizes), wait for their stream at the
 *     end of the call instead, so no GPU idle gap opens inside them.
 *   - Randomness is explicit.  Where the reference draws from OsRng the caller
 *     passes the drawn values (or, for ChaCha masking, the seed words) -- or, through the `_keyed` entry
 *     points and sda_draws_dev, one 256-bit OS-RNG key that the device expands into the draws.  Keyed
 *     Additive generation (sda_additive_generate_keyed_dev, sda_participant_share_keyed_dev and their 32 forms)
 *     makes the draws inside the share kernel: they never exist as a buffer.
 *   - Every function returns an sda_status; 0 = OK.  The codes 1..6 map 1:1 to
 *     the reference's error strings; sda_last_error_message() gives details.
 *   - A handle may be used from one thread at a time (the Rust trait objects
 *     are not Sync either); distinct handles are independent.  The handle's
 *     scratch buffers are shared by its calls: a `_dev` call on a different
 *     stream than the handle's previous call first makes its stream wait (an
 *     event recorded when the previous call returned, no host sync) for the
 *     work queued by the previous one, so calls on one handle never race
 *     however the caller mixes streams.  The previous call's stream is not
 *     touched again: it may be destroyed once that call has returned.
 */
#ifndef SDA_ENGINE_H
#define SDA_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDA_ENGINE_ABI_VERSION 1

typedef enum {
    SDA_OK = 0,
    SDA_ERR_BATCH_INPUT_WRONG_LENGTH = 1,     /* "Batch input wrong length"          additive.rs:33      */
    SDA_ERR_PACKED_SHARING_FAILED = 2,        /* "Sharing failed for packed secret sharing scheme" packed_shamir.rs:41 */
    SDA_ERR_WRONG_DIMENSION = 3,              /* "Wrong dimension"                   combiner.rs:21      */
    SDA_ERR_MISMATCHING_DIMENSION = 4,        /* "Mismatching dimension"             additive.rs:64      */
    SDA_ERR_INPUTS_MUST_HAVE_SAME_LENGTH = 5, /* "Inputs must have same length"      packed_shamir.rs:74 */
    SDA_ERR_NOT_ENOUGH_SHARES = 6,            /* "Not enough shares to reconstruct"  packed_shamir.rs:75 */
    SDA_ERR_PRECONDITION = 64,   /* where the reference panics (assert!/assert_eq!, chacha.rs:26 ...)   */
    SDA_ERR_INVALID_ARGUMENT = 65, /* null handle/pointer, buffer too small                              */
    SDA_ERR_UNSUPPORTED = 66,    /* scheme parameters outside the engine's domain       */
    SDA_ERR_DEVICE = 67,         /* HIP runtime / kernel failure                                        */
    SDA_ERR_OUT_OF_MEMORY = 68
} sda_status;

/* protocol/src/crypto.rs:79-114  LinearSecretSharingScheme */
typedef enum { SDA_SHARING_ADDITIVE = 0, SDA_SHARING_PACKED_SHAMIR = 1 } sda_sharing_kind;
typedef struct {
    int32_t kind;                /* sda_sharing_kind                                  */
    uint64_t share_count;        /* Additive.share_count / PackedShamir.share_count   */
    int64_t modulus;             /* Additive.modulus     / PackedShamir.prime_modulus */
    uint64_t secret_count;       /* PackedShamir only                                 */
    uint64_t privacy_threshold;  /* PackedShamir only                                 */
    int64_t omega_secrets;       /* PackedShamir only                                 */
    int64_t omega_shares;        /* PackedShamir only                                 */
} sda_sharing_scheme;

/* protocol/src/crypto.rs:43-64  LinearMaskingScheme */
typedef enum { SDA_MASKING_NONE = 0, SDA_MASKING_FULL = 1, SDA_MASKING_CHACHA = 2 } sda_masking_kind;
typedef struct {
    int32_t kind;                /* sda_masking_kind                    */
    int64_t modulus;             /* Full.modulus / ChaCha.modulus       */
    uint64_t dimension;          /* ChaCha.dimension                    */
    uint64_t seed_bitsize;       /* ChaCha.seed_bitsize                 */
} sda_masking_scheme;

/* Packed-Shamir reveal representation. */
typedef enum {
    SDA_REVEAL_EXACT = 0,        /* bit-exact signed representatives of tss reconstruct (Newton) */
    SDA_REVEAL_CANONICAL = 1     /* canonical residues in [0,p) (Lagrange weights); equal mod p  */
} sda_reveal_mode;

typedef struct sda_engine sda_engine;

/* ---------------- lifecycle / diagnostics ---------------- */
int sda_abi_version(void);
sda_status sda_engine_create(int device_ordinal, sda_engine** out);
void sda_engine_destroy(sda_engine* h);
sda_status sda_engine_synchronize(sda_engine* h);
/* One handle over n_devices devices ("1-8 GPUs are used internally").  The host entry
 * points split their work over the devices and still return when the result is in host memory:
 *   sda_share_combine / Full sda_mask_combine / Additive sda_secret_reconstruct: by columns (each device
 *     walks every row in order over its slice: exact, signed inputs included, no exchange);
 *   ChaCha sda_mask_combine: by seeds, one RCCL ncclReduce(SUM, int64) onto ordinals[0] + the device
 *     finalize (RCCL is loaded on first use; moduli above 2^62, or repeated ordinals, run on ordinals[0]);
 *   sda_share_generate / PackedShamir sda_secret_reconstruct: by batches (Additive generate: by columns).
 * The `_dev` entry points run on ordinals[0].  Ordinals may repeat (several slices on one device: a
 * rehearsal of the split on fewer GPUs).  n_devices = 1 gives a one-device handle whose ChaCha mask
 * combine still reduces through a one-rank RCCL communicator. */
sda_status sda_engine_create_multi(const int* ordinals, int n_devices, sda_engine** out);
int sda_engine_device_count(const sda_engine* h);     /* devices the host entry points use; 0 for NULL */
const char* sda_last_error_message(void);          /* thread-local; never NULL */
const char* sda_status_string(int status);         /* reference error string for 1..6 */

/* ---------------- derived scheme sizes: protocol/src/crypto.rs:117-155 ---------------- */
uint64_t sda_scheme_input_size(const sda_sharing_scheme* s);              /* :120-126 */
uint64_t sda_scheme_output_size(const sda_sharing_scheme* s);             /* :129-135 */
uint64_t sda_scheme_privacy_threshold(const sda_sharing_scheme* s);       /* :138-144 */
uint64_t sda_scheme_reconstruction_threshold(const sda_sharing_scheme* s);/* :147-153 */
/* number of batches per clerk vector: ceil(dimension / input_size) (batched.rs:21-23) */
uint64_t sda_share_length(const sda_sharing_scheme* s, uint64_t dimension);

/* ---------------- trait mirrors (host buffers, synchronous) ---------------- */

/* ShareGenerator::generate  (sharing/mod.rs:14-17; batched.rs:19-53)
 *   secrets[dimension];  draws: the values OsRng produced, in draw order:
 *     Additive     [dimension][share_count-1]   gen_range(0, modulus)   additive.rs:42-44
 *     PackedShamir [B][privacy_threshold]       tss Range(0, p-1) sample
 *   out: [share_count][B] clerk-major, B = sda_share_length(s, dimension). */
sda_status sda_share_generate(sda_engine* h, const sda_sharing_scheme* s,
                              const int64_t* secrets, uint64_t dimension,
                              const int64_t* draws, uint64_t n_draws,
                              int64_t* out, uint64_t out_cap);

/* sda_share_generate with its draws made on the device (sda_draws_dev's rule, below) instead of passed in:
 *   Additive:     draw [d][j] is element d*(n-1)+j, bound = modulus
 *   PackedShamir: draw [b][j] is element b*t+j,     bound = prime_modulus - 1
 * of (key, stream_id).  key: HOST, 8 words, fresh from the OS RNG for this call (see sda_draws_dev).  Every scheme
 * check, status and the output layout are sda_share_generate's, and the result is identical to sda_share_generate
 * fed with sda_draws of the same key, stream_id and bound.  On a multi-device handle the work splits as
 * sda_share_generate's does and each device makes its own slice of the draws, so the result does not depend on
 * the device count. */
sda_status sda_share_generate_keyed(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets,
                                    uint64_t dimension, const uint32_t* key, uint32_t stream_id,
                                    int64_t* out, uint64_t out_cap);

/* ShareCombiner::combine  (sharing/mod.rs:23-25; combiner.rs:16-28)
 *   rows[i] has lens[i] elements (a Vec<Vec<i64>>).  out_len = lens[0] (0 if n_rows == 0). */
sda_status sda_share_combine(sda_engine* h, const sda_sharing_scheme* s,
                             const int64_t* const* rows, const uint64_t* lens, uint64_t n_rows,
                             int64_t* out, uint64_t out_cap, uint64_t* out_len);

/* SecretReconstructor::reconstruct  (sharing/mod.rs:31-33; additive.rs:56-72; batched.rs:69-97)
 *   indexed shares = (indices[i], rows[i][lens[i]]);  dimension = factory argument (mod.rs:76). */
sda_status sda_secret_reconstruct(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                  const uint64_t* indices, const int64_t* const* rows,
                                  const uint64_t* lens, uint64_t n_rows,
                                  int64_t* out, uint64_t out_cap, uint64_t* out_len);

/* SecretMasker::mask  (masking/mod.rs:13-15)
 *   None:   mask_len = 0, masked = secrets                        (none.rs:14-19)
 *   Full:   full_masks[dimension] = the OsRng draws; mask = them  (full.rs:22-35)
 *   ChaCha: seed[seed_words] = the OsRng seed words; mask = seed as i64 (chacha.rs:25-53)
 *   mask_out needs room for dimension (Full) or seed_words (ChaCha) values. */
sda_status sda_secret_mask(sda_engine* h, const sda_masking_scheme* s,
                           const int64_t* secrets, uint64_t dimension,
                           const uint32_t* seed, uint64_t seed_words,
                           const int64_t* full_masks,
                           int64_t* mask_out, uint64_t mask_cap, uint64_t* mask_len,
                           int64_t* masked_out);

/* sda_secret_mask for Full masking with the mask drawn on the device: mask element d is element d of
 * (key, stream_id) at bound = modulus (sda_draws_dev's rule); mask_out = those draws, *mask_len = dimension,
 * masked_out = (secrets + mask) % modulus as full.rs:28-32.  key: HOST, 8 words, fresh from the OS RNG for this
 * call.  Kinds None and ChaCha return SDA_ERR_INVALID_ARGUMENT (None draws nothing, ChaCha expands its own seed:
 * use sda_secret_mask); a modulus <= 0 is SDA_ERR_PRECONDITION as in sda_secret_mask. */
sda_status sda_secret_mask_keyed(sda_engine* h, const sda_masking_scheme* s, const int64_t* secrets,
                                 uint64_t dimension, const uint32_t* key, uint32_t stream_id,
                                 int64_t* mask_out, uint64_t mask_cap, uint64_t* mask_len,
                                 int64_t* masked_out);

/* MaskCombiner::combine  (masking/mod.rs:21-23)
 *   Full: rows are masks (full.rs:38-50); ChaCha: rows are seeds-as-i64 (chacha.rs:57-76) -- no row gives
 *   `dimension` zeros for any modulus (nothing is drawn), a modulus <= 0 with a row is SDA_ERR_PRECONDITION;
 *   None: every row must be empty, out_len = 0 (none.rs:22-25). */
sda_status sda_mask_combine(sda_engine* h, const sda_masking_scheme* s,
                            const int64_t* const* rows, const uint64_t* lens, uint64_t n_rows,
                            int64_t* out, uint64_t out_cap, uint64_t* out_len);

/* SecretUnmasker::unmask  (masking/mod.rs:29-31; chacha.rs:80-91; full.rs:55-66; none.rs:28-32)
 *   For ChaCha, `mask` is the COMBINED mask (the recipient's mask_combiner output). */
sda_status sda_secret_unmask(sda_engine* h, const sda_masking_scheme* s,
                             const int64_t* mask, uint64_t mask_len,
                             const int64_t* masked, uint64_t masked_len,
                             int64_t* out, uint64_t out_cap, uint64_t* out_len);

/* RecipientOutput::positive  (receive.rs:14-20) */
sda_status sda_recipient_positive(sda_engine* h, int64_t modulus, const int64_t* values,
                                  uint64_t n, int64_t* out);

/* ---------------- device-resident entry points (HBM-resident inputs) ---------------- */

/* Exact clerk combine of a dense [n][dim] matrix with row stride `row_stride` elements:
 * out[j] = combiner.rs:22-25 applied over rows 0..n-1 in order. */
sda_status sda_combine_dev(sda_engine* h, int64_t modulus, const int64_t* shares,
                           uint64_t n, uint64_t dim, uint64_t row_stride,
                           int64_t* out, void* stream);

/* The same recurrence continued from inout[dim] (a previous combine result, |r| < m, or zeros):
 * a clerk job streamed through HBM in row tiles is bit-identical to one pass over all rows. */
sda_status sda_combine_accumulate_dev(sda_engine* h, int64_t modulus, const int64_t* shares,
                                      uint64_t n, uint64_t dim, uint64_t row_stride,
                                      int64_t* inout, void* stream);

/* int32 share rows as an input type of the combine: shares [n][dim] int32, `row_stride` in int32 elements.
 * Every shipped configuration has |share| < m <= 2^31, so half of an i64 row is sign extension; these entry
 * points read half the bytes.  The rows are sign-extended and run through the same recurrence: the i64 result
 * is bit-identical to widening the rows and calling sda_combine_dev / sda_combine_accumulate_dev, for every
 * modulus.  Argument checks, the n == 0 behaviour and the stream ordering are those of the i64 entry points;
 * accumulate calls of the two widths may alternate on one `inout`. */
sda_status sda_combine32_dev(sda_engine* h, int64_t modulus, const int32_t* shares, uint64_t n, uint64_t dim,
                             uint64_t row_stride, int64_t* out, void* stream);
sda_status sda_combine32_accumulate_dev(sda_engine* h, int64_t modulus, const int32_t* shares, uint64_t n,
                                        uint64_t dim, uint64_t row_stride, int64_t* inout, void* stream);

/* dst[n][dim] (int32, row stride dst_stride) = (int32_t)src[n][dim] (i64, row stride src_stride), on the
 * device.  flag: device int64[1], zeroed by the caller; set to 1 (never cleared) when some element lies
 * outside [-2^31, 2^31 - 1] -- dst is then not a copy of src.  No condition on any modulus: the values only
 * have to fit. */
sda_status sda_narrow32_dev(sda_engine* h, const int64_t* src, uint64_t n, uint64_t dim, uint64_t src_stride,
                            int32_t* dst, uint64_t dst_stride, int64_t* flag, void* stream);

/* Counters of the row-tile stream of i64 host rows (sda_share_combine, the Full sda_mask_combine, the Additive
 * sda_secret_reconstruct), cumulative since the handle was created, summed over a multi-device handle's
 * devices: tiles staged as int32 rows (every value of the tile fitted; SDA_HOST_NARROW) and as
 * i64 rows, and the bytes of their host -> device copies.  Any pointer may be NULL.
 * sda_clerk_decode_combine's stream is not counted. */
sda_status sda_host_stream_stats(const sda_engine* h, uint64_t* tiles_i32, uint64_t* tiles_i64,
                                 uint64_t* bytes_h2d);

/* Diagnostic (read-only): how many batches the handle's most recent packed-Shamir generate or reconstruct
 * launch handed to its generic fix-up kernel (raw i64 inputs outside (-p, p), or a lazy-truncation / sign-bit
 * trap).  A value above 65536 (the log's capacity) means the launch recomputed every batch.
 * 0 when that launch logged nothing by construction (the workspace kernels of the wide schemes, the canonical
 * Lagrange reveal) or when no packed launch has run.  Waits for the handle's last call to finish and copies 4
 * bytes per device; summed over a multi-device handle's devices. */
sda_status sda_packed_fixup_count(sda_engine* h, uint64_t* batches);

/* Diagnostic (read-only): how the handle's most recent ChaCha launch ran -- a mask combine (sda_mask_combine,
 * sda_chacha_mask_combine_dev, the recipient pipeline's mask) or a participant's mask (sda_secret_mask,
 * sda_participant_share_dev).  A call of dimension 0 launches nothing and leaves the record.
 *   path    0  no ChaCha launch yet
 *           1  fast path, direct: one chunk, the kernel stores the results
 *           2  fast path, chunked: grid_y chunks of seeds merged with atomics
 *           3  fast path, stream-K over grid_y workgroups
 *           4  single-stream mask add (sda_participant_share_dev's masked secrets)
 *           5  exact stream path
 *           6  fast path whose rejection log overflowed, rerun on the stream path
 *   grid_y  the number of chunks (1 for paths 1 and 4), or the stream-K grid size; 0 for path 5; for path 6
 *           that of the fast attempt
 *   fixups  fix-up kernel launches, one per stream with a rejected draw below the dimension (a pipeline's
 *           late resolve included; after a participant's redo, those of the redone mask)
 * Host-side records: nothing is waited for or copied.  On a multi-device handle whose last mask combine split
 * its seeds over the devices, path and grid_y are the first device's and fixups is summed over the devices.
 * No pointer may be NULL. */
sda_status sda_chacha_last_launch(sda_engine* h, uint32_t* path, uint64_t* grid_y, uint64_t* fixups);

/* Diagnostic (read-only): how the handle's most recent sda_clerk_decode_combine_dev or sda_clerk_job_dev produced
 * its result.  The record is NONE from the call's entry until it returns SDA_OK, so a failed call leaves NONE; the
 * host streaming entry points (sda_clerk_decode_combine, sda_clerk_job) keep no record and leave NONE as well, and
 * so does a job whose payloads decode to no element after its count pass (nothing is launched), and a
 * sda_clerk_job_dev call without blobs (the finish call).  One failing call writes it: a sda_clerk_job_dev whose
 * payload_cap was too small has completed its decode -> combine, and the record describes that.
 *   path       0  NONE
 *              1  SLOTS          one decode into int32 slots per 16 KiB region + the combine over the slots
 *              2  SLOTS_GROUPED  the same, `passes` groups of blobs through one reused slot buffer (SDA_CODEC_GROUP)
 *              3  FUSED          the column-tile decode -> combine (SDA_CODEC_PATH=fused)
 *              4  FUSED_MULTI    its multi-round variant (the job has an element of >= 6 bytes)
 *              5  MATRIX32       count pass + int32 matrix + combine
 *              6  MATRIX64       count pass + i64 matrix + combine
 *   width      columns per lane of the slot combine (1, 2 or 4: SDA_SLOT_CPL) for paths 1 and 2; blobs the fused
 *              kernel prefetches ahead (2, 4 or 8: SDA_DC_DEPTH; always 2 for path 4) for paths 3 and 4; else 0
 *   fell_back  bits: 1  the slot attempt raised its wide flag (an element longer than 5 bytes or outside int32, or
 *                       more than 4096 elements in a region) and was abandoned for the count pass
 *                    2  fused was asked for but a blob is irregular (a run of >= 11 continuation bytes)
 *                    4  the int32 matrix decode met a value outside int32 and was abandoned for the i64 one
 *                    8  the sequential decoder ran (irregular blobs)
 *   passes     path 2: the blob groups; else the grid slices of at most 65,535 blobs of the decode pass that
 *              produced the result (paths 3 and 4: of the tile plan, the fused kernel's grid being column tiles)
 * A host-side record: nothing is waited for or copied.  No pointer may be NULL. */
sda_status sda_codec_last_launch(sda_engine* h, uint32_t* path, uint32_t* width, uint32_t* fell_back,
                                 uint64_t* passes);

/* Diagnostic (read-only): which share-combine kernel the handle launched most recently and on what grid -- by any
 * entry point that ends in one: sda_combine_dev / sda_combine32_dev and their _accumulate forms, sda_combine_split_dev,
 * sda_combine_split_replay_dev, the host entry points' streamed tiles (the last tile's launch), the matrix paths of
 * the clerk's decode -> combine (sda_clerk_decode_combine_dev, sda_clerk_job_dev), the recipient pipeline.  A call that launches nothing (dim == 0, an accumulate,
 * split or replay with n == 0) leaves the record, and so does a launch the runtime refuses (the call then returns
 * SDA_ERR_DEVICE).  The ChaCha stream path's internal combine is not recorded here (sda_chacha_last_launch describes
 * that launch).
 *   kind        0  no combine launch yet
 *               1  combine_exact_kernel
 *               2  combine_replay_kernel (pass 2 of the participation split)
 *   elem_bytes  the row element: 8 (i64) or 4 (int32)
 *   vec         columns per lane: 1, 2 or 4 -- the widest the column count, row stride and pointers line up for
 *   rows        rows loaded per batch: 2, 4 or 8
 *   variant     bits: 1  m <= 2^62 (the kernel without the wrapping-add slow path)
 *                     2  continues from the output's values (accumulate, split)
 *                     4  raises the participation split's flags
 *                     8  software-pipelined (off with SDA_COMBINE_PIPE=0)
 *   grid        workgroups launched
 *   wlo, nwide  the balanced grid: every workgroup owns wlo lanes, the first nwide of them 8 more; 0, 0 on the plain
 *               grid of 256-lane workgroups
 *   per_cu      resident workgroups per CU the runtime reported for the kernel, as handed to the balanced grid's
 *               sizing; 0 when that grid was not considered (a kernel that is not pipelined, SDA_COMBINE_BALANCE=0)
 * A host-side record: nothing is waited for or copied.  A multi-device handle reports its first device's record.
 * No pointer may be NULL. */
sda_status sda_combine_last_launch(sda_engine* h, uint32_t* kind, uint32_t* elem_bytes, uint32_t* vec, uint32_t* rows,
                                   uint32_t* variant, uint64_t* grid, uint32_t* wlo, uint32_t* nwide,
                                   uint32_t* per_cu);

/* Diagnostic (read-only): what the handle's most recent sda_snapshot_transpose_dev planned and launched.  Every
 * successful call with a dst writes the record; a sizing query (dst == NULL) and a failed call leave it as it was.
 * Before any such call every field is 0.
 *   blobs        the non-empty blobs of the copy plan (empty blobs are dropped on the host)
 *   chunks       the chunks those blobs were cut into: the sum of ceil(len / chunk_bytes)
 *   grid         workgroups launched; 0 when every blob was empty (nothing is launched)
 *   chunk_bytes  the bytes of one chunk of the copy kernel as built
 *   shifts       bit s is set when some planned blob has (source offset - destination offset) mod 16 == s: the
 *                kernel's 16 load variants this call reached
 * A snapshot of empty blobs alone reports (0, 0, 0, chunk_bytes, 0).  A host-side record: nothing is waited for or
 * copied.  No pointer may be NULL. */
sda_status sda_snapshot_last_launch(sda_engine* h, uint64_t* blobs, uint64_t* chunks, uint64_t* grid,
                                    uint64_t* chunk_bytes, uint32_t* shifts);

/* Diagnostic (read-only): the decisions the handle's most recent sda_recipient_reveal / sda_recipient_reveal_dev
 * took.  A call writes the record when it returns SDA_OK with an output of at least one element; a failed call and
 * a call whose output is empty leave it as it was.  Before any such call every field is 0.
 *   mask_kind        1  no masking
 *                    2  Full: the mask rows were combined by the pipeline
 *                    3  ChaCha: the seeds were expanded and combined by the pipeline
 *                    4  ChaCha on a multi-device handle: the mask combine was split over the devices and the
 *                       pipeline ran with the combined row
 *   reveal_mode      0  Additive: the clerk rows were combined
 *                    1  PackedShamir, the exact reveal (tss' signed representatives)
 *                    2  PackedShamir, the canonical reveal -- asked for, or substituted for an EXACT request
 *                       whose output cannot depend on the representative (masking and output modulus both the
 *                       sharing prime; SDA_RECIPIENT_EXACT=1 keeps EXACT)
 *   fell_back        1 when that substituted canonical reveal was refused (repeated clerk indices) and the
 *                    exact reveal ran instead
 *   compact          1 when the clerk vectors were longer than the batch count and their first B values were
 *                    copied into a dense matrix first
 *   unmask_launches  1, or 2 when the ChaCha mask had rejected draws: it was fixed and the unmask redone
 * A host-side record: nothing is waited for or copied.  No pointer may be NULL. */
sda_status sda_recipient_last_launch(sda_engine* h, uint32_t* mask_kind, uint32_t* reveal_mode, uint32_t* fell_back,
                                     uint32_t* compact, uint32_t* unmask_launches);

/* Diagnostic (read-only): the routes the handle's most recent sda_participant_share_dev, _share32_dev or keyed form
 * took.  A call of dimension > 0 writes the record when it returns SDA_OK; a failed call and a call of dimension 0
 * leave it as it was.  Before any such call every field is 0.
 *   mask_route   1  no masking
 *                2  Full: one add of the caller's masks
 *                3  ChaCha, the fused single-stream mask add (sda_chacha_last_launch path 4)
 *                4  ChaCha, the mask expanded by the combine's dispatch (a modulus off the fast path, or
 *                   SDA_CHACHA_PATH=stream), then one add
 *                5  Full, the mask drawn in the masking kernel (a participant job)
 *   share_route  1  Additive from the caller's draws
 *                2  Additive, draws made in the kernel (keyed)
 *                3  PackedShamir from the caller's draws
 *                4  PackedShamir keyed (sda_packed_keyed_last_launch tells in-kernel from staged draws)
 *   passes       1, or 2 when route 3's mask had a rejected draw: the mask and every later step were redone
 * A host-side record: nothing is waited for or copied.  No pointer may be NULL. */
sda_status sda_participant_last_launch(sda_engine* h, uint32_t* mask_route, uint32_t* share_route, uint32_t* passes);

/* Multi-GPU finalize: `sums` are the int64 sums (RCCL-reduced; |sum| <= 2^63 - 1, signed allowed)
 * of per-GPU combine results; out = their canonical residue in [0, m).  Exact w.r.t. the reference
 * when all combined inputs were non-negative. */
sda_status sda_combine_finalize_dev(sda_engine* h, int64_t modulus, const int64_t* sums,
                                    uint64_t dim, int64_t* out, void* stream);

/* ---- participation split of the clerk combine over G ranks ----
 * The reference's result (combiner.rs:16-28) is order dependent when inputs are negative (Additive
 * last shares are signed, additive.rs:46), so rank g (rows of participations g's contiguous range):
 *  1. sda_combine_split_dev: the exact recurrence continued from inout (zeros before the first row
 *     tile), which also sets flags[0] = 1 if an input is < 0 and flags[1] = 1 if an input lies outside
 *     [-(2^63 - m), 2^63 - m] (the reference's `r + v` may wrap there: no split reproduces that, refuse
 *     the split).  flags: device int64[2], zeroed by the caller, only ever set to 1.
 *  2. no rank flagged a negative input: all-reduce(SUM) the G results, sda_combine_finalize_dev.
 *  3. otherwise: all-gather the G results into gathered[G][dim]; sda_combine_split_prefix_dev gives
 *     c_in (canonical sum of ranks < g), total (canonical sum of all) and the initial code;
 *     sda_combine_split_replay_dev replays this rank's row tiles from c_in (state in/out) recording the
 *     last sign event in code (0 none, 2g+1 reset, 2g+2 set); all-reduce(MAX) the codes over the ranks;
 *     sda_combine_split_resolve_dev writes the reference's signed result. */
sda_status sda_combine_split_dev(sda_engine* h, int64_t modulus, const int64_t* shares, uint64_t n,
                                 uint64_t dim, uint64_t row_stride, int64_t* inout, int64_t* flags,
                                 void* stream);
sda_status sda_combine_split_prefix_dev(sda_engine* h, int64_t modulus, const int64_t* gathered,
                                        uint64_t world, uint64_t rank, uint64_t dim, int64_t* c_in,
                                        int64_t* total, int32_t* code, void* stream);
sda_status sda_combine_split_replay_dev(sda_engine* h, int64_t modulus, const int64_t* shares, uint64_t n,
                                        uint64_t dim, uint64_t row_stride, uint64_t rank, int64_t* state,
                                        int32_t* code, void* stream);
sda_status sda_combine_split_resolve_dev(sda_engine* h, int64_t modulus, const int64_t* total,
                                         const int32_t* code, uint64_t dim, int64_t* out, void* stream);

/* Packed-Shamir share generation for `n_vectors` participant vectors at once:
 * secrets [n_vectors][dimension], draws [n_vectors][B][t], out [n_vectors][n][B]. */
sda_status sda_packed_generate_dev(sda_engine* h, const sda_sharing_scheme* s,
                                   const int64_t* secrets, uint64_t dimension, uint64_t n_vectors,
                                   const int64_t* draws, int64_t* out, void* stream);

/* The same with a representation mode: SDA_REVEAL_EXACT = tss' signed shares (as above),
 * SDA_REVEAL_CANONICAL = their canonical residues in [0, p).  Canonical shares are equal to the
 * reference's mod p, so combine -> reveal -> unmask -> positive() ends in the identical output
 * when the masking modulus is the sharing prime. */
sda_status sda_packed_generate_mode_dev(sda_engine* h, const sda_sharing_scheme* s,
                                        const int64_t* secrets, uint64_t dimension, uint64_t n_vectors,
                                        const int64_t* draws, int64_t* out, int32_t mode, void* stream);

/* Packed-Shamir reveal: shares [n_vectors][n_idx][B] at clerk `indices` (host array),
 * out [n_vectors][dimension].  All n_idx shares are used (batched.rs:75); n_idx <= 1023. */
sda_status sda_packed_reconstruct_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                      const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                      const int64_t* shares, int64_t* out, int32_t mode, void* stream);

/* ---- int32 share rows through the packed-Shamir data flow ----
 * check_packed admits only primes p < 2^31 and every share is a `% p` result, so |share| <= p - 1 < 2^31: half
 * of an i64 share is sign extension.  With these two entry points the device-resident chain generate ->
 * sda_combine32_dev -> sda_narrow32_dev (of the n clerk results) -> reveal stays in int32 rows end to end, and so
 * does the participant's generate -> sda_varint_encode32_dev (or sda_participant_share32_dev) -> clerk decode
 * (INTEGRATION.md).  Argument checks, error codes, the 65,535-vector and 1,023-share limits, the stream ordering
 * on the handle and sda_packed_fixup_count afterwards are those of the i64 entry points; on a multi-device handle
 * they run on ordinals[0].  out / shares need only 4-byte alignment and any B works; the fast stores need a
 * 16-byte aligned out and even B (16 bytes per lane from B % 4 == 0), as the i64 kernels do.
 *
 * sda_packed_generate_mode_dev with int32 shares: out [n_vectors][n][B] int32, dense.  Bit-identical to
 * (int32_t) of the i64 entry point's output, for every scheme in the engine's domain, both modes, raw i64
 * secrets included (shares are `% p` results, p < 2^31: they always fit, so there is no flag).
 * Schemes with n + 1 <= 27 and the workspace kernels (k + t + 1 > 64, n + 1 > 81) write int32 directly.  At
 * n + 1 = 81 the register kernels write i64 shares into scratch owned by the handle (n_vectors * n * B * 8
 * bytes, kept and reused until the handle is destroyed) and a narrowing pass writes out: when that scratch
 * cannot be allocated the call returns SDA_ERR_OUT_OF_MEMORY and out is untouched. */
sda_status sda_packed_generate32_dev(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets,
                                     uint64_t dimension, uint64_t n_vectors, const int64_t* draws,
                                     int32_t* out, int32_t mode, void* stream);

/* sda_packed_reconstruct_dev from int32 shares [n_vectors][n_idx][B]: out (i64) is bit-identical to widening
 * the shares and calling the i64 entry point -- shares outside (-p, p) that fit int32 included (fix-up). */
sda_status sda_packed_reconstruct32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                        const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                        const int32_t* shares, int64_t* out, int32_t mode, void* stream);

/* ---- share consistency check with faulty-clerk location ----
 * A packed-Shamir sharing polynomial has degree below L = k + t + 1, and a reveal interpolates through the inserted
 * point (1, 0) and ALL n_idx clerk shares: from more than k + t shares some are redundant, and a wrong one still
 * gives an aggregate with status SDA_OK.  These calls read the shares a reveal would read and tell whether they
 * agree.  Points: x_0 = 1, y_0 = 0; x_j = omega_shares^(indices[j-1] + 1), y_j = the residue mod p of share j
 * (any i64 value is reduced exactly; signed and canonical representatives are the same share).  With
 * r = n_idx - (k + t), the redundancy:
 *   a batch is consistent iff one polynomial of degree < L passes through all n_idx + 1 points;
 *   with r >= 2 a bad batch is located at position j (1 <= j <= n_idx) iff the points without point j are
 *   consistent (at most one such j exists); with r < 2 nothing is located; point 0 is never a suspect.
 * Verdict per batch (uint16_t): 0 consistent, j located at position j (1-based into indices), 0xFFFF inconsistent
 * and not located.
 *
 * shares [n_vectors][n_idx][B] as sda_packed_reconstruct_dev takes them, B = ceil(dimension / k).  verdict: device
 * uint16_t [n_vectors][B], 2-byte aligned, or NULL (declared void*: every binding maps it without a 16-bit type).  Host outputs (all required; blame may be NULL when n_idx == 0): *redundancy = r,
 * *bad_batches, *first_bad = the smallest bad vec * B + b (UINT64_MAX when nothing is bad), blame[j-1] = the batches
 * located at position j (unlocated ones: bad_batches - sum of blame).
 * The checks, their order and their statuses are those of sda_packed_reconstruct_dev on the same arguments (NULL
 * arguments where the int32 reveal checks them; SDA_ERR_NOT_ENOUGH_SHARES included); repeated indices return
 * SDA_ERR_UNSUPPORTED, as a CANONICAL reveal does.  An Additive scheme (B = dimension), r == 0, dimension == 0 and
 * n_vectors == 0 return SDA_OK with zero counts and launch nothing; a given verdict buffer is zero-filled.  The call
 * drains its stream before it returns (it reads the counts); a failing call writes nothing.  Stream ordering on the
 * handle is that of every `_dev` call; on a multi-device handle the call runs on ordinals[0].
 * SDA_CHECK_LOG_CAP (read per call, 0 .. 65536, default 65536): the entries of the bad-batch log used; more bad
 * batches than that and the location pass walks every batch of the call (same results, slower). */
sda_status sda_packed_check_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                const int64_t* shares, void* verdict, uint64_t* redundancy,
                                uint64_t* bad_batches, uint64_t* first_bad, uint64_t* blame, void* stream);
sda_status sda_packed_check32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                  const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                  const int32_t* shares, void* verdict, uint64_t* redundancy,
                                  uint64_t* bad_batches, uint64_t* first_bad, uint64_t* blame, void* stream);
/* The same check of host share rows, as sda_secret_reconstruct takes them (one vector; verdict: HOST [B] or NULL).
 * Checks and statuses are those of sda_secret_reconstruct, ragged rows included; an Additive scheme returns SDA_OK
 * with zero counts (verdict, when given, holds share_lens[0] zeros for n_idx > 0). */
sda_status sda_secret_check(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                            const uint64_t* indices, const int64_t* const* share_rows, const uint64_t* share_lens,
                            uint64_t n_idx, void* verdict, uint64_t* redundancy, uint64_t* bad_batches,
                            uint64_t* first_bad, uint64_t* blame);
/* How the last check on this handle that launched something ran (written when it returns SDA_OK; host-side only; all
 * zeros before): path 1 a register kernel / 2 the looped kernel (33 .. 1023 shares); bucket 8 / 16 / 32 shares, 0
 * on the looped path; located = batches the location pass walked (the bad ones, or every batch when the log
 * overflowed; 0 when r < 2 or nothing was bad); overflowed = more bad batches than the log held. */
sda_status sda_packed_check_last_launch(sda_engine* h, uint32_t* path, uint32_t* bucket, uint64_t* located,
                                        uint32_t* overflowed);

/* ---- checked reveal: the check and the CANONICAL reveal in one pass, a located wrong share corrected ----
 * Inputs as sda_packed_check_dev takes them; out [n_vectors][dimension] i64 as sda_packed_reconstruct_dev writes it
 * (never NULL), verdict and the host outputs as the check gives them.  Per batch, with the check's verdict:
 *   0 (consistent)          the k secrets of sda_packed_reconstruct_dev(..., SDA_REVEAL_CANONICAL) on the same
 *                           arguments, bit for bit;
 *   j (located at j)        the CANONICAL reveal of the n_idx - 1 shares without position j, whether j is one of the
 *                           first k + t positions or a later one: one clerk's wrong share costs nothing;
 *   0xFFFF (not located)    the CANONICAL reveal from the first k + t shares in the order given.  Such a batch is
 *                           flagged garbage, as it is in sda_packed_reconstruct_dev; the rule is this one so that it
 *                           is the same on every path.  Fall back to dropping a clerk and revealing from the rest
 *                           (INTEGRATION.md).
 * Output is always canonical, in [0, p): tss defines no signed representative for a corrected set, so there is no
 * EXACT form.  The tail batch is cut at `dimension`; raw i64 shares outside (-p, p) are reduced exactly, as in the
 * check.  r == 0 is the plain canonical reveal with zero counts; r == 1 detects and flags only.
 * The checks, their order and their statuses are those of sda_packed_check_dev, with out == NULL where the reveal
 * checks it (SDA_ERR_INVALID_ARGUMENT); repeated indices return SDA_ERR_UNSUPPORTED; an Additive scheme returns
 * SDA_ERR_UNSUPPORTED (nothing to correct, no packed reveal).  dimension == 0 and n_vectors == 0 return SDA_OK with
 * zero counts and launch nothing.  A failing call writes nothing; the call drains its stream before it returns.
 * Schemes with at most 32 shares and k <= 8 run one fused kernel over the shares (one memset, one kernel, one small
 * copy and one wait when every batch is consistent; bad batches add the location pass, a fix-up over them and the
 * blame copy); all others run the check, the CANONICAL reveal and the fix-up one after the other: there a consistent
 * batch is what sda_packed_reconstruct_dev CANONICAL returns, which past 32 shares follows tss' wrapping i64 steps for
 * raw shares within 2^62 of the i64 limits.  The call shares the check's counter block and bad-batch log, and
 * SDA_CHECK_LOG_CAP. */
sda_status sda_packed_reveal_checked_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                         const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                         const int64_t* shares, int64_t* out, void* verdict, uint64_t* redundancy,
                                         uint64_t* bad_batches, uint64_t* first_bad, uint64_t* blame, void* stream);
sda_status sda_packed_reveal_checked32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                           const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                           const int32_t* shares, int64_t* out, void* verdict, uint64_t* redundancy,
                                           uint64_t* bad_batches, uint64_t* first_bad, uint64_t* blame, void* stream);
/* The same from host share rows, as sda_secret_check takes them (one vector; verdict: HOST [B] or NULL; out: HOST
 * [dimension], required when dimension > 0).  Checks and statuses are those of sda_secret_check, ragged rows included,
 * except that an Additive scheme returns SDA_ERR_UNSUPPORTED. */
sda_status sda_secret_reconstruct_checked(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                          const uint64_t* indices, const int64_t* const* share_rows,
                                          const uint64_t* share_lens, uint64_t n_idx, void* verdict,
                                          uint64_t* redundancy, uint64_t* bad_batches, uint64_t* first_bad,
                                          uint64_t* blame, int64_t* out);
/* How the last checked reveal on this handle that launched something ran (written when it returns SDA_OK; host-side
 * only; all zeros before): path 1 the fused register kernel / 2 the composed path; bucket 8 / 16 / 32 shares on the
 * fused path, else 0; fixed = the batches the fix-up kernel rewrote (fused: those located among the first k + t
 * positions; composed: every bad batch); overflowed = more bad batches than the log held. */
sda_status sda_packed_reveal_checked_last_launch(sda_engine* h, uint32_t* path, uint32_t* bucket, uint64_t* fixed,
                                                 uint32_t* overflowed);

/* ---- decoded reveal: the CANONICAL reveal with up to floor(r / 2) wrong clerk shares per batch corrected ----
 * The n_idx + 1 points of a batch (the share check's: x_0 = 1, y_0 = 0, then x_j = omega_shares^(indices[j-1] + 1),
 * y_j = share j mod p) are a word of a Reed-Solomon code of minimum distance r + 1, r = n_idx - (k + t), so up to
 * e_max = floor(r / 2) wrong shares per batch are uniquely correctable.  Per batch:
 *   consistent          one polynomial of degree < L = k + t + 1 passes through all n_idx + 1 points (the check's);
 *   decoded with E      E a set of positions in 1 .. n_idx, 1 <= |E| <= e_max, the points without E are consistent
 *                       and no smaller such set exists.  At most one such E exists (two would give two codewords at
 *                       distance <= 2 e_max <= r).  Point 0 is never in E: a word whose nearest codeword disagrees
 *                       with (1, 0) is undecodable;
 *   undecodable         otherwise.
 *                       verdict (uint16_t)   wrong (uint32_t, bit j-1 = position j)   secrets written
 *   consistent          0                    0                  sda_packed_reconstruct_dev CANONICAL of all shares,
 *                                                               bit for bit
 *   decoded with E      |E|                  the bits of E      the CANONICAL reveal of the n_idx - |E| shares without E
 *   undecodable         0xFFFF               0                  the CANONICAL reveal from the first k + t shares (the
 *                                                               checked reveal's rule: flagged garbage)
 * With |E| = 1 this is the share check's "located at j": every batch sda_packed_reveal_checked_dev answers with 0 or
 * j gets the same secrets here, E = {j}.  r < 2 behaves as the checked reveal does (r == 0: the plain canonical
 * reveal, zero counts; r == 1: detect and flag).  Output is always canonical, in [0, p); raw i64 shares outside
 * (-p, p) are reduced exactly.
 * Inputs and out as sda_packed_reveal_checked_dev takes them.  verdict: device uint16_t [n_vectors][B] or NULL; wrong:
 * device uint32_t [n_vectors][B], 4-byte aligned, or NULL, independent of verdict.  Host outputs (all required; blame
 * may be NULL when n_idx == 0): *redundancy = r, *radius = e_max, *bad_batches and *first_bad as the check gives
 * them, *undecoded = the batches with verdict 0xFFFF, blame[j-1] = the batches whose E contains position j (the sum
 * of blame is the sum of |E| over the call).
 * Scope: PackedShamir, n_idx <= 32 and k <= 8 (the fused checked reveal's); beyond either SDA_ERR_UNSUPPORTED.  An
 * Additive scheme and repeated indices return SDA_ERR_UNSUPPORTED.  All other checks, their order and their statuses
 * are those of sda_packed_reveal_checked_dev; wrong not 4-byte aligned is SDA_ERR_INVALID_ARGUMENT.  dimension == 0
 * and n_vectors == 0 return SDA_OK with zero counts and launch nothing.  A failing call writes nothing; the call
 * drains its stream before it returns; stream ordering and the multi-device rule are those of every `_dev` call.
 * Two passes: the checked reveal's fused first pass, then, when something is bad and e_max >= 1, one decode pass over
 * the logged batches (one lane per batch: syndromes, Berlekamp-Massey, root search, Forney).
 * SDA_CHECK_LOG_CAP applies as in the check: on overflow the decode pass walks every batch, with the same results. */
sda_status sda_packed_reveal_decoded_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                         const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                         const int64_t* shares, int64_t* out, void* verdict, void* wrong,
                                         uint64_t* redundancy, uint64_t* radius, uint64_t* bad_batches,
                                         uint64_t* first_bad, uint64_t* undecoded, uint64_t* blame, void* stream);
sda_status sda_packed_reveal_decoded32_dev(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                           const uint64_t* indices, uint64_t n_idx, uint64_t n_vectors,
                                           const int32_t* shares, int64_t* out, void* verdict, void* wrong,
                                           uint64_t* redundancy, uint64_t* radius, uint64_t* bad_batches,
                                           uint64_t* first_bad, uint64_t* undecoded, uint64_t* blame, void* stream);
/* The same from host share rows, as sda_secret_reconstruct_checked takes them (one vector; verdict: HOST uint16_t [B]
 * or NULL; wrong: HOST uint32_t [B] or NULL; out: HOST [dimension], required when dimension > 0).  Checks and statuses
 * are those of sda_secret_reconstruct_checked, ragged rows included, then the scope above. */
sda_status sda_secret_reconstruct_decoded(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                          const uint64_t* indices, const int64_t* const* share_rows,
                                          const uint64_t* share_lens, uint64_t n_idx, void* verdict, void* wrong,
                                          uint64_t* redundancy, uint64_t* radius, uint64_t* bad_batches,
                                          uint64_t* first_bad, uint64_t* undecoded, uint64_t* blame, int64_t* out);
/* How the last decoded reveal on this handle that launched something ran (written when it returns SDA_OK; host-side
 * only; all zeros before): path 1 the first pass alone (nothing bad, or e_max == 0) / 2 the decode pass too; bucket
 * 8 / 16 / 32 shares; decoded = the batches the decode pass walked (the bad ones, or every batch when the log
 * overflowed); fixed = the batches whose out it rewrote (E meets the first k + t positions); max_errors = the largest
 * |E| of the call; overflowed = more bad batches than the log held. */
sda_status sda_packed_decode_last_launch(sda_engine* h, uint32_t* path, uint32_t* bucket, uint64_t* decoded,
                                         uint64_t* fixed, uint32_t* max_errors, uint32_t* overflowed);

/* Additive share generation: secrets [dimension], draws [dimension][n-1], out [n][dimension]. */
sda_status sda_additive_generate_dev(sda_engine* h, int64_t modulus, uint64_t share_count,
                                     const int64_t* secrets, uint64_t dimension,
                                     const int64_t* draws, int64_t* out, void* stream);

/* ChaCha mask expansion + combine (chacha.rs:57-76) over n_seeds seeds of w words
 * (seeds [n_seeds][w] u32, device), out [dimension].  Exact including gen_range rejections
 * (fix-up pass; moduli with a high rejection rate expand each stream exactly instead) and the
 * reference's wrapping i64 sum for moduli above 2^62 (the result is then signed and
 * order-dependent, as in the reference).  Waits for its rejection log before returning.  n_seeds == 0 gives
 * `dimension` zeros for any modulus; a modulus <= 0 with a seed is SDA_ERR_PRECONDITION. */
sda_status sda_chacha_mask_combine_dev(sda_engine* h, int64_t modulus, uint64_t dimension,
                                       const uint32_t* seeds, uint64_t w, uint64_t n_seeds,
                                       int64_t* out, void* stream);

/* ---------------- device-side draws (DESIGN.md "Device draws") ----------------
 * The reference draws every share-generation and Full-mask value from OsRng, one gen_range at a time.  These entry
 * points expand one 256-bit key with ChaCha20 on the device instead.  Element i (an absolute 64-bit index), retry
 * round r = 0, 1, ...:
 *   state = "expand 32-byte k" | key[0..7] | (i >> 3) low word, high word | stream_id | r
 *   o = ChaCha20 core(state) (20 rounds + feed-forward);  j = i & 7;  v = (o[2j] << 32) | o[2j+1]
 *   zone = (2^64 - 1) - (2^64 - 1) % bound          (rand 0.3's gen_range rule, as the ChaCha mask kernels)
 *   v < zone: the draw is v % bound; otherwise round r + 1 (same block counter and position); at r = 63 the
 *   draw is v % bound unconditionally (reached with probability below 2^-64).
 * An element depends only on (key, stream_id, i, bound): any sub-range, device split or launch shape gives the
 * same values.  KEY CONTRACT: key is 8 words in HOST memory, fresh from the OS RNG; a (key, stream_id) pair must
 * never serve two different jobs -- within one job, distinct element ranges or distinct stream_ids of one key are
 * independent streams.  The key travels as a kernel argument and is never stored in device memory.
 * Checks, in this order: a NULL handle, key or needed buffer -> SDA_ERR_INVALID_ARGUMENT; bound <= 0 ->
 * SDA_ERR_PRECONDITION ("Rng.gen_range called with low >= high"); first + count wrapping past 2^64 ->
 * SDA_ERR_INVALID_ARGUMENT; count == 0 -> SDA_OK, nothing launched.
 *
 * out[p] = draw(first + p), p < count, uniform on [0, bound).  out: device (8-byte aligned).  Only enqueues. */
sda_status sda_draws_dev(sda_engine* h, const uint32_t* key, uint32_t stream_id, uint64_t first,
                         uint64_t count, int64_t bound, int64_t* out, void* stream);
/* The same into host memory (synchronous; the draws pass through the handle's staging scratch).  out_cap < count
 * -> SDA_ERR_INVALID_ARGUMENT. */
sda_status sda_draws(sda_engine* h, const uint32_t* key, uint32_t stream_id, uint64_t first,
                     uint64_t count, int64_t bound, int64_t* out, uint64_t out_cap);

/* Full masking (full.rs:22-35) with the mask drawn inside the masking kernel: for d < dimension,
 *   mask_out[d]   = draw(first + d) of (key, stream_id) at bound = modulus, and
 *   masked_out[d] = (secrets[d] + mask_out[d]) % modulus, a wrapping add and Rust's truncated `%` (full.rs:28-31),
 * so mask_out is bit-identical to sda_draws_dev(key, stream_id, first, dimension, modulus) and masked_out to what
 * sda_secret_mask returns with that mask, in one pass that reads the secrets once and writes each output once.
 * `first` lets a caller split one job's secrets over calls, devices or streams: any split gives the same values.
 * secrets, masked_out and mask_out are device buffers (8-byte aligned; the 32 form's mask_out 4-byte aligned) that
 * do not overlap.  Only enqueues; runs on ordinals[0] of a multi-device handle.  sda_draws_dev's KEY CONTRACT
 * applies verbatim.
 * The 32 form writes the mask as int32 values, equal to (int32_t) of the i64 form's: with modulus <= 2^31 every
 * mask value lies in [0, modulus) and fits.
 * Checks, in this order: a NULL handle, key or needed buffer -> SDA_ERR_INVALID_ARGUMENT; modulus <= 0 ->
 * SDA_ERR_PRECONDITION ("Rng.gen_range called with low >= high"); first + dimension wrapping past 2^64 ->
 * SDA_ERR_INVALID_ARGUMENT; the 32 form with modulus > 2^31 -> SDA_ERR_UNSUPPORTED; dimension == 0 -> SDA_OK,
 * nothing launched.  A refused call writes nothing. */
sda_status sda_full_mask_keyed_dev(sda_engine* h, int64_t modulus, const int64_t* secrets, uint64_t dimension,
                                   const uint32_t* key, uint32_t stream_id, uint64_t first, int64_t* masked_out,
                                   int64_t* mask_out, void* stream);
sda_status sda_full_mask_keyed32_dev(sda_engine* h, int64_t modulus, const int64_t* secrets, uint64_t dimension,
                                     const uint32_t* key, uint32_t stream_id, uint64_t first, int64_t* masked_out,
                                     int32_t* mask_out, void* stream);

/* Additive share generation with the draws made inside the kernel: column d < dimension of
 * `secrets` (device) is absolute column c = first_column + d of the job and takes draws c (n - 1) + j, j < n - 1,
 * of (key, stream_id) at bound = modulus (n = share_count), so
 *   out[j * out_stride + d] = draw(c (n - 1) + j)                      for j < n - 1, and
 *   out[(n - 1) * out_stride + d] = the fold of additive.rs:47 over them in order from the raw secret,
 * which is bit-identical to sda_draws_dev(key, stream_id, first_column (n - 1), dimension (n - 1), modulus) fed to
 * sda_additive_generate_dev, without the draws ever being a buffer.  n = 1 draws nothing and writes the secrets
 * unreduced.  first_column lets a caller split one job's columns over calls, devices or streams: any split gives
 * the same shares.  out: device, rows out_stride elements apart (columns past `dimension` of a row are not
 * written).  Only enqueues; runs on ordinals[0] of a multi-device handle.  sda_draws_dev's KEY CONTRACT applies
 * verbatim.
 * The 32 form writes int32 rows (4-byte alignment is enough, any dimension), equal to (int32_t) of the i64 form's:
 * with modulus <= 2^31 every draw lies in [0, m) and the last share in (-m, m), so each share fits by construction.
 * Checks, in this order: a NULL handle, key or needed buffer -> SDA_ERR_INVALID_ARGUMENT; share_count == 0 ->
 * SDA_ERR_PRECONDITION (share_count - 1 underflows); modulus <= 0 -> SDA_ERR_PRECONDITION ("Rng.gen_range called
 * with low >= high"); out_stride < dimension -> SDA_ERR_INVALID_ARGUMENT; (first_column + dimension) *
 * (share_count - 1) wrapping past 2^64 -> SDA_ERR_INVALID_ARGUMENT; the 32 form with modulus > 2^31 ->
 * SDA_ERR_UNSUPPORTED; dimension == 0 -> SDA_OK, nothing launched.  A refused call writes nothing. */
sda_status sda_additive_generate_keyed_dev(sda_engine* h, int64_t modulus, uint64_t share_count,
                                           const int64_t* secrets, uint64_t dimension, const uint32_t* key,
                                           uint32_t stream_id, uint64_t first_column, int64_t* out,
                                           uint64_t out_stride, void* stream);
sda_status sda_additive_generate_keyed32_dev(sda_engine* h, int64_t modulus, uint64_t share_count,
                                             const int64_t* secrets, uint64_t dimension, const uint32_t* key,
                                             uint32_t stream_id, uint64_t first_column, int32_t* out,
                                             uint64_t out_stride, void* stream);

/* Packed-Shamir share generation with the draws made inside the share kernels: the keyed form of
 * sda_packed_generate_mode_dev.  With B = ceil(dimension / k) batches per vector, batch b of vector v is absolute
 * batch first_batch + v B + b of the job and takes draws (first_batch + v B + b) t + j, j < t, of (key, stream_id)
 * at bound p - 1 as its randomness, so out [n_vectors][n][B] is bit-identical to
 * sda_draws_dev(key, stream_id, first_batch t, n_vectors B t, p - 1) fed to sda_packed_generate_mode_dev (the 32
 * form: to sda_packed_generate32_dev), in both modes, and sda_packed_fixup_count afterwards reports the same count
 * as after that unkeyed call.  first_batch lets a caller split one job's batches over calls, devices or streams: any
 * split gives the same shares.  Schemes the register kernels serve with n + 1 <= 27 make the draws in the share
 * kernel's tile and never write them to device memory; every other scheme (n + 1 >= 81, k + t + 1 > 64, the
 * workspace kernels) gets them from the draws kernel in scratch owned by the handle (n_vectors * B * t * 8 bytes,
 * kept and reused until the handle is destroyed) ahead of the unkeyed kernels.  Only enqueues; runs on ordinals[0]
 * of a multi-device handle.  sda_draws_dev's KEY CONTRACT applies verbatim.
 * Checks, in this order: those of sda_packed_generate_mode_dev / sda_packed_generate32_dev (scheme kind, mode,
 * the scheme's domain, the 65,535-vector limit, a NULL needed buffer); a NULL key -> SDA_ERR_INVALID_ARGUMENT;
 * (first_batch + n_vectors * B) * t wrapping past 2^64 -> SDA_ERR_INVALID_ARGUMENT; on the staged path, scratch
 * that cannot be allocated -> SDA_ERR_OUT_OF_MEMORY with out untouched.  A refused call writes nothing. */
sda_status sda_packed_generate_keyed_dev(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets,
                                         uint64_t dimension, uint64_t n_vectors, const uint32_t* key,
                                         uint32_t stream_id, uint64_t first_batch, int64_t* out, int32_t mode,
                                         void* stream);
sda_status sda_packed_generate_keyed32_dev(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets,
                                           uint64_t dimension, uint64_t n_vectors, const uint32_t* key,
                                           uint32_t stream_id, uint64_t first_batch, int32_t* out, int32_t mode,
                                           void* stream);
/* How the last keyed packed-Shamir launch on the handle got its draws (the two entry points above, the keyed
 * participant calls, sda_share_generate_keyed on its first device): *path = 0 none yet, 1 made in the share
 * kernels, 2 staged; *staged_bytes = the draw bytes that crossed HBM (0 on path 1).  A host-side record: calls
 * that launch nothing (dimension or n_vectors 0) and refused calls leave it as it was. */
sda_status sda_packed_keyed_last_launch(sda_engine* h, uint32_t* path, uint64_t* staged_bytes);

/* ---------------- share payload codec ----------------
 * Encryptor::encrypt encodes shares with integer-encoding 1.0 VarInt before sealing
 * (client/src/crypto/encryption/sodium.rs:36-41); Decryptor::decrypt decodes after opening
 * (:82-88): zigzag + LEB128, a run of >= 11 continuation bytes forms one 11-byte element and a
 * truncated final varint yields its partial value.  The sealed box itself stays on the host. */

/* Encryptor::encrypt's encoding step: out[*out_len] bytes (at most 10 per value). */
sda_status sda_varint_encode(sda_engine* h, const int64_t* vals, uint64_t n,
                             uint8_t* out, uint64_t out_cap, uint64_t* out_len);
/* Decryptor::decrypt's decoding step for one opened blob. */
sda_status sda_varint_decode(sda_engine* h, const uint8_t* bytes, uint64_t n_bytes,
                             int64_t* out, uint64_t out_cap, uint64_t* out_len);
/* Clerk job after the sealed-box opens (clerk.rs:79-86): decode every participation's blob,
 * then ShareCombiner::combine -- "Wrong dimension" if a blob decodes to a different length. */
sda_status sda_clerk_decode_combine(sda_engine* h, const sda_sharing_scheme* s,
                                    const uint8_t* const* blobs, const uint64_t* blob_lens,
                                    uint64_t n_blobs, int64_t* out, uint64_t out_cap,
                                    uint64_t* out_len);
/* Device forms.  `bytes`: device, 16-byte aligned, readable up to blob_off[n_blobs] rounded up to
 * 16 plus 16 bytes; blob i = bytes[blob_off[i], blob_off[i+1]) with blob_off a HOST array.
 * decode: out [n_blobs][out_stride] (device), counts[n_blobs] (host) = values per blob. */
sda_status sda_varint_decode_dev(sda_engine* h, const uint8_t* bytes, const uint64_t* blob_off,
                                 uint64_t n_blobs, int64_t* out, uint64_t out_stride,
                                 uint64_t* counts, void* stream);
/* decode + exact combine (combiner.rs:16-28); out (device) gets *out_len values. */
sda_status sda_clerk_decode_combine_dev(sda_engine* h, int64_t modulus, const uint8_t* bytes,
                                        const uint64_t* blob_off, uint64_t n_blobs,
                                        int64_t* out, uint64_t out_cap, uint64_t* out_len,
                                        void* stream);
/* encode rows [rows][stride] (first len values of each) back to back into dst (device);
 * row_bytes[rows] (host) = bytes per row. */
sda_status sda_varint_encode_dev(sda_engine* h, const int64_t* vals, uint64_t rows, uint64_t len,
                                 uint64_t stride, uint8_t* dst, uint64_t dst_cap,
                                 uint64_t* row_bytes, void* stream);
/* The same from int32 rows (a share below 2^31 in magnitude, e.g. sda_packed_generate32_dev's output): stride is
 * in int32 elements and vals needs only 4-byte alignment.  The bytes written and row_bytes are identical to
 * sign-extending the rows and calling sda_varint_encode_dev (an element takes at most 5 bytes); argument checks,
 * status codes, the 65,535-row limit, the stream ordering on the handle and the wait for the row sizes are those
 * of sda_varint_encode_dev.  A dst_cap below the total returns SDA_ERR_INVALID_ARGUMENT and writes nothing. */
sda_status sda_varint_encode32_dev(sda_engine* h, const int32_t* vals, uint64_t rows, uint64_t len,
                                   uint64_t stride, uint8_t* dst, uint64_t dst_cap,
                                   uint64_t* row_bytes, void* stream);

/* The clerk's whole arithmetic step (process_clerking_job, client/src/clerk.rs:63-107, between opening the
 * participations' sealed boxes and sealing the result): decode every blob, combine, and encode the combined
 * shares as the recipient's payload -- one call, one wait, and continuable tile by tile so that a job's
 * participations need not fit in HBM together.  bytes and blob_off are as for sda_clerk_decode_combine_dev.
 *   Fresh call (first_participation == 0; prior_dim is ignored): state[0 .. dim) and *dim_out are what
 *     sda_clerk_decode_combine_dev writes to out and *out_len, with its checks, their order and its statuses.
 *   Continuing call (first_participation > 0): state holds the prior_dim values earlier calls left for
 *     participations [0, first_participation).  Every blob of this call, its blob 0 included, must decode to
 *     exactly prior_dim values, else SDA_ERR_WRONG_DIMENSION naming participation first_participation + i.  With
 *     prior_dim > 0 a modulus of 0 or INT64_MIN fails first (row 0 was folded by an earlier call); prior_dim >
 *     state_cap is SDA_ERR_INVALID_ARGUMENT.  combiner.rs:16-28's recurrence continues from state in place:
 *     after any split of the blobs into calls, state is bit-identical to one sda_clerk_decode_combine_dev over
 *     all of them (signed shares make the recurrence order-dependent).  *dim_out = prior_dim.
 *   Continuing call with n_blobs == 0: state is left alone; with a payload this is the job's finish call, and
 *     the retry after a payload buffer that was too small.
 *   payload != NULL (device): state[0 .. dim) encoded as Encryptor::encrypt encodes it (sodium.rs:36-41), the
 *     bytes sda_varint_encode_dev(state, 1, dim, dim, ...) writes; *payload_len = their count.  A payload_cap
 *     below it returns SDA_ERR_INVALID_ARGUMENT with no payload byte written, *payload_len the count needed, and
 *     state, *dim_out and sda_codec_last_launch's record those of the completed combine: finish with an
 *     n_blobs == 0 call.  payload == NULL: no encode (an intermediate tile); payload_len may then be NULL.
 *   Every other failing call leaves state and payload exactly as they were.
 * The decode paths and their dispatch are sda_clerk_decode_combine_dev's, and sda_codec_last_launch and
 * sda_combine_last_launch report these calls as they report that one (a continuing call's matrix paths combine
 * with the accumulate variant), except that a continuing call under SDA_CODEC_PATH=fused takes the count pass and
 * the matrix path (the fused kernel has no accumulating form).  On the slot path the payload is encoded behind the
 * combine by kernels that read the dimension on the device, before the call's single wait.  Runs on ordinals[0] of
 * a multi-device handle; stream ordering on the handle is that of every _dev call. */
sda_status sda_clerk_job_dev(sda_engine* h, int64_t modulus, const uint8_t* bytes, const uint64_t* blob_off,
                             uint64_t n_blobs, uint64_t first_participation, uint64_t prior_dim,
                             int64_t* state, uint64_t state_cap, uint64_t* dim_out,
                             uint8_t* payload, uint64_t payload_cap, uint64_t* payload_len, void* stream);
/* The same job from host memory (the Rust clerk's call): the blobs stream as in sda_clerk_decode_combine, the
 * accumulator is encoded on the device and the payload (about 4.9 bytes per field share instead of 8) is copied
 * to payload (host).  out (host) may be NULL; else it gets the *out_len combined shares as
 * sda_clerk_decode_combine writes them.  Errors are that call's; a payload_cap below the payload's size (or a
 * NULL payload) returns SDA_ERR_INVALID_ARGUMENT with *payload_len the count needed. */
sda_status sda_clerk_job(sda_engine* h, const sda_sharing_scheme* s, const uint8_t* const* blobs,
                         const uint64_t* blob_lens, uint64_t n_blobs, int64_t* out, uint64_t out_cap,
                         uint64_t* out_len, uint8_t* payload, uint64_t payload_cap, uint64_t* payload_len);
/* Diagnostic (read-only): how the handle's most recent sda_clerk_job_dev / sda_clerk_job ran.  Written when such a
 * call returns SDA_OK after launching something; a failed call and a call that launches nothing (no blobs and
 * nothing to encode) leave it as it was.  Before any such call every field is 0.
 *   continued      0  a fresh call; 1  a continuing one
 *   encode_route   0  no payload was asked for
 *                  1  the device-length encode, queued behind the combine before the call's single wait
 *                  2  the host-length encode after the counts were read (the count-pass paths, the finish call,
 *                     sda_clerk_job)
 *   encode_chunks  the chunks of the encode's grid: route 1 sizes it by the host's bound on the dimension (blob
 *                  0's bytes, or prior_dim), route 2 by the dimension; 0 when nothing was encoded
 * A host-side record: nothing is waited for or copied.  No pointer may be NULL. */
sda_status sda_clerk_job_last_launch(sda_engine* h, uint32_t* continued, uint32_t* encode_route,
                                     uint64_t* encode_chunks);

/* ---------------- snapshot transposition ----------------
 * Replaces AggregationsStore::iter_snapshot_clerk_jobs_data (server/src/stores.rs:86-101; the Mongo
 * store's $unwind/$group at server-store-mongodb/src/aggregations.rs:164-195): the snapshot's
 * participations [participation][clerk] regrouped as clerking jobs [clerk][participation], each
 * clerk's blobs in snapshot order.  Blobs are opaque bytes (sealed boxes or opened payloads).
 *   src (device, 16-byte aligned, readable 32 bytes past part_off[P*n]): participation p's payload
 *     for clerk c = src[part_off[p*n + c], part_off[p*n + c + 1]); part_off is a HOST array [P*n + 1].
 *   dst (device, 16-byte aligned): clerk c's job starts at dst + clerk_base[c] (16-byte aligned) and
 *     its blob p = [clerk_off[c*(P+1) + p], clerk_off[c*(P+1) + p + 1]) relative to that start, followed
 *     by >= 16 readable bytes -- exactly the (bytes, blob_off) pair sda_clerk_decode_combine_dev takes.
 *   clerk_base [n], clerk_off [n][P+1] (HOST, written); *dst_len = bytes of dst used.
 *   dst == NULL: sizing query (offsets and *dst_len only, nothing launched).
 *   Runs on `stream` and returns once the copy has completed (the copy plan is uploaded per call). */
sda_status sda_snapshot_transpose_dev(sda_engine* h, const uint8_t* src, const uint64_t* part_off,
                                      uint64_t n_participations, uint64_t n_clerks, uint8_t* dst,
                                      uint64_t dst_cap, uint64_t* dst_len, uint64_t* clerk_base,
                                      uint64_t* clerk_off, void* stream);

/* ---------------- fused role pipelines ---------------- */

/* Recipient reveal (receive.rs:80-157) + RecipientOutput::positive (:14-20) as one device
 * pipeline: mask combine -> reconstruct -> fused unmask+positive, no host round trip between.
 *   mask_in: Full = masks [n_masks][mask_width] i64; ChaCha = seeds [n_masks][mask_width] u32
 *            (1..8 words); None = n_masks rows of width 0.
 *   shares [n_idx][share_len] at clerk `indices` (host array); dimension = the reconstructor's
 *   factory argument (vector_dimension); output_modulus = aggregation.modulus for positive().
 *   Errors as the reference: Not enough shares (6), Mismatching dimension (4), assert -> 64.
 *   With ChaCha masking the call drains its stream before returning: the mask's gen_range rejection
 *   count is read then (the rare rejected draws are fixed and the unmask redone). */
sda_status sda_recipient_reveal_dev(sda_engine* h, const sda_masking_scheme* ms, const void* mask_in,
                                    uint64_t n_masks, uint64_t mask_width, const sda_sharing_scheme* ss,
                                    uint64_t dimension, const uint64_t* indices, const int64_t* shares,
                                    uint64_t n_idx, uint64_t share_len, int64_t output_modulus,
                                    int32_t mode, int64_t* out, uint64_t out_cap, uint64_t* out_len,
                                    void* stream);
/* Host form: mask rows as MaskCombiner::combine takes them (Full masks / ChaCha seeds-as-i64),
 * share rows as SecretReconstructor::reconstruct takes them.  On a multi-device handle the ChaCha mask
 * combine is split over the devices (as sda_mask_combine), the rest runs on ordinals[0]. */
sda_status sda_recipient_reveal(sda_engine* h, const sda_masking_scheme* ms,
                                const int64_t* const* mask_rows, const uint64_t* mask_lens, uint64_t n_masks,
                                const sda_sharing_scheme* ss, uint64_t dimension, const uint64_t* indices,
                                const int64_t* const* share_rows, const uint64_t* share_lens, uint64_t n_idx,
                                int64_t output_modulus, int32_t mode,
                                int64_t* out, uint64_t out_cap, uint64_t* out_len);

/* Participant (participate.rs:53-76): SecretMasker::mask -> ShareGenerator::generate -> per-clerk
 * payload encoding (sodium.rs:36-41) on device.  seed: host words (ChaCha); full_masks: device [D]
 * (Full); secrets [D], draws (as sda_share_generate) and shares_out [n][B] are device buffers.
 * mode: packed shares as tss' signed values (SDA_REVEAL_EXACT) or canonical residues
 * (SDA_REVEAL_CANONICAL, see sda_packed_generate_mode_dev); ignored for Additive.
 * payload (device, may be NULL): the n clerk payloads back to back, payload_row_bytes[n] (host).
 * With ChaCha masking, or with payloads, the call drains its stream before returning (the mask's
 * rejection count; the payload sizes). */
sda_status sda_participant_share_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                     uint64_t seed_words, const int64_t* full_masks,
                                     const sda_sharing_scheme* ss, const int64_t* secrets, uint64_t dimension,
                                     const int64_t* draws, int32_t mode, int64_t* shares_out, uint8_t* payload,
                                     uint64_t payload_cap, uint64_t* payload_row_bytes, void* stream);

/* sda_participant_share_dev with the shares as int32 rows: shares_out [n][B] int32, dense (4-byte alignment is
 * enough), generated by what sda_packed_generate32_dev launches and encoded by sda_varint_encode32_dev's kernels,
 * so a share stays 4 bytes wide from share generation to the clerk's sda_clerk_decode_combine_dev.  shares_out is
 * bit-identical to (int32_t) of the i64 pipeline's shares, payload and payload_row_bytes are byte-identical to
 * the i64 pipeline's, in both modes and for every packed scheme in the engine's domain.  Masking (the ChaCha
 * rejection check and its redo of every later step included), sda_chacha_last_launch, sda_packed_fixup_count,
 * payload == NULL and the waits are those of sda_participant_share_dev.
 * PackedShamir only: an Additive scheme returns SDA_ERR_UNSUPPORTED, because its first n - 1 shares are the
 * caller's draws copied verbatim and the engine does not range-check them, so they need not fit int32
 * (sda_participant_share32_keyed_dev, whose draws are the engine's own, takes Additive).
 * At n + 1 = 81 the SDA_ERR_OUT_OF_MEMORY contract of sda_packed_generate32_dev applies (n * B * 8 bytes of
 * handle-owned scratch; shares_out and payload are untouched when it cannot be allocated). */
sda_status sda_participant_share32_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                       uint64_t seed_words, const int64_t* full_masks,
                                       const sda_sharing_scheme* ss, const int64_t* secrets, uint64_t dimension,
                                       const int64_t* draws, int32_t mode, int32_t* shares_out, uint8_t* payload,
                                       uint64_t payload_cap, uint64_t* payload_row_bytes, void* stream);

/* sda_participant_share_dev with the share-generation draws made on the device from (key, stream_id) instead of
 * passed in (key: HOST, 8 words; sda_draws_dev's KEY CONTRACT applies verbatim).  shares_out, payload and
 * payload_row_bytes are bit-identical to sda_participant_share_dev fed with sda_draws_dev(key, stream_id, 0, count,
 * bound) -- Additive: count = D (n - 1), bound = modulus, made inside the share kernel
 * (sda_additive_generate_keyed_dev with first_column 0); PackedShamir: count = B t, bound = p - 1, made as
 * sda_packed_generate_keyed_dev with first_batch 0 makes them (sda_packed_keyed_last_launch tells where).
 * Everything else is sda_participant_share_dev's:
 * the masking (full_masks is still passed in, because the mask must also reach the recipient: make it with
 * sda_draws_dev under another stream_id), the ChaCha rejection redo (share generation runs again and, under the
 * same key, makes the same shares), the payload encode, the waits, sda_chacha_last_launch and
 * sda_packed_fixup_count.  A NULL key -> SDA_ERR_INVALID_ARGUMENT. */
sda_status sda_participant_share_keyed_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                           uint64_t seed_words, const int64_t* full_masks,
                                           const sda_sharing_scheme* ss, const int64_t* secrets,
                                           uint64_t dimension, const uint32_t* key, uint32_t stream_id,
                                           int32_t mode, int64_t* shares_out, uint8_t* payload,
                                           uint64_t payload_cap, uint64_t* payload_row_bytes, void* stream);

/* sda_participant_share32_dev likewise.  Unlike the unkeyed form it takes an Additive scheme with modulus <= 2^31:
 * the engine makes the first n - 1 shares itself, in [0, m), and the last is a `% m` result, so every share fits
 * int32 by construction and flows on to sda_combine32_dev, sda_varint_encode32_dev and the clerk's int32 decode.
 * An Additive modulus above 2^31 -> SDA_ERR_UNSUPPORTED (a draw need not fit int32). */
sda_status sda_participant_share32_keyed_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                             uint64_t seed_words, const int64_t* full_masks,
                                             const sda_sharing_scheme* ss, const int64_t* secrets,
                                             uint64_t dimension, const uint32_t* key, uint32_t stream_id,
                                             int32_t mode, int32_t* shares_out, uint8_t* payload,
                                             uint64_t payload_cap, uint64_t* payload_row_bytes, void* stream);

/* ---------------- participant job: mask, mask payload, shares and every clerk payload in one call ----------------
 * participate.rs:53-98 between the secrets and the sealed boxes: SecretMasker::mask, the recipient's mask payload
 * (:56-72), ShareGenerator::generate and one payload per clerk (:79-98), each payload being the bytes
 * Encryptor::encrypt encodes before it seals (sodium.rs:36-41).  Sealing stays on the host.  Every random value comes
 * from one key (sda_draws_dev's KEY CONTRACT applies verbatim): the Full mask is elements [0, D) of
 * (key, mask_stream_id) at bound = the masking modulus, drawn inside the masking kernel (sda_full_mask_keyed_dev),
 * and the share-generation draws are those of sda_participant_share_keyed_dev under (key, share_stream_id).
 *
 * CONTRACT.  The clerk payloads and their sizes are byte-identical to sda_participant_share_keyed_dev(ms, seed,
 * seed_words, full_masks = sda_draws_dev(key, mask_stream_id, 0, D, ms->modulus), ss, secrets, D, key,
 * share_stream_id, mode, ...)'s payload and payload_row_bytes; the mask payload is sda_varint_encode of the mask that
 * full.rs / chacha.rs return (Full: those draws; ChaCha: the seed words `as i64`; None: empty).  The shares live in
 * handle scratch as int32 rows wherever they fit by construction -- a PackedShamir scheme, or an Additive scheme with
 * modulus <= 2^31 (sda_participant_share32_keyed_dev's rules) -- else as i64 rows, and a Full mask as int32 values
 * when its modulus <= 2^31.  Masking, the ChaCha rejection check and its redo, the scheme checks and their statuses
 * are those of sda_participant_share_dev; ChaCha masking also needs seed_words == (seed_bitsize + 31) / 32 when
 * dimension is 0.  With Full masking mask_stream_id == share_stream_id -> SDA_ERR_INVALID_ARGUMENT (the key
 * contract).  More than 65,535 clerks -> SDA_ERR_UNSUPPORTED.
 *
 * CAPACITIES.  sda_participant_job_payload_bound gives the worst case in bytes of one clerk's payload and of the mask
 * payload, from the moduli alone: a share lies in (-m, m) and a mask value in [0, m), so a value takes at most the
 * bytes of 2 (m - 1) -- 5 for every modulus up to 2^34 -- and a ChaCha seed word 5.  (One Additive clerk's share is
 * the masked secret as it stands: the masking modulus bounds it, and without masking it takes up to 10 bytes.)  Both
 * job forms require every capacity to be at least its bound, else they return SDA_ERR_INVALID_ARGUMENT before any
 * work with every length set to its bound: nothing is ever half-written for want of space.  Needs no device. */
sda_status sda_participant_job_payload_bound(const sda_masking_scheme* ms, const sda_sharing_scheme* ss,
                                             uint64_t dimension, uint64_t* clerk_row_bound, uint64_t* mask_bound);

/* Device form.  secrets [dimension]: device; seed (ChaCha) and key: HOST words.  payload (device, payload_cap >=
 * share_count * clerk_row_bound bytes): the clerk payloads back to back, payload_row_bytes[share_count] (host) their
 * sizes; mask_payload (device, mask_payload_cap >= mask_bound): the mask payload, *mask_payload_len (host) its size
 * (0 without masking: nothing is drawn).  The ChaCha seed words are encoded on the host and copied.
 * A failing call leaves caller memory and every *_last_launch record as they were.  The call drains its stream
 * before returning, as sda_participant_share_dev with a payload does.  Runs on ordinals[0] of a multi-device handle. */
sda_status sda_participant_job_dev(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed,
                                   uint64_t seed_words, const sda_sharing_scheme* ss, const int64_t* secrets,
                                   uint64_t dimension, const uint32_t* key, uint32_t mask_stream_id,
                                   uint32_t share_stream_id, int32_t mode, uint8_t* payload, uint64_t payload_cap,
                                   uint64_t* payload_row_bytes, uint8_t* mask_payload, uint64_t mask_payload_cap,
                                   uint64_t* mask_payload_len, void* stream);

/* Host form.  secrets [dimension], clerk_payloads[c] (clerk_caps[c] >= clerk_row_bound bytes) and mask_payload
 * (mask_cap >= mask_bound) are host memory; clerk_lens[c] and *mask_len get the sizes.  Every output byte equals the
 * device form's.  The job runs in tiles of whole batches (Additive: columns): a tile's secrets go up on the handle's
 * copy stream while the previous tile computes and the one before it comes down, each clerk's bytes of a tile are
 * appended to that clerk's blob, and device memory is bounded by the tile, not by share_count * B.  Tile [b0, b1)
 * draws its mask from element b0 k on and its shares from first_batch (first_column) b0, so the bytes do not depend
 * on the tiling.  The tile size follows SDA_HOST_STAGE_MB; SDA_PARTICIPANT_TILE_BATCHES (read per call; an A/B and
 * test knob) sets it in batches.  With ChaCha masking the masked secrets are made over the whole vector first (8
 * dimension bytes of handle scratch twice over) and its rejection count is read before the first tile.  Runs on
 * ordinals[0] of a multi-device handle. */
sda_status sda_participant_job(sda_engine* h, const sda_masking_scheme* ms, const uint32_t* seed, uint64_t seed_words,
                               const sda_sharing_scheme* ss, const int64_t* secrets, uint64_t dimension,
                               const uint32_t* key, uint32_t mask_stream_id, uint32_t share_stream_id, int32_t mode,
                               uint8_t* const* clerk_payloads, const uint64_t* clerk_caps, uint64_t* clerk_lens,
                               uint8_t* mask_payload, uint64_t mask_cap, uint64_t* mask_len);

/* Diagnostic (read-only): what the handle's most recent sda_participant_job / sda_participant_job_dev ran.  Written
 * when such a call of dimension > 0 returns SDA_OK; before any such call every field is 0.
 *   mask_route   0  no masking
 *                1  Full, the mask drawn in the masking kernel as i64 values
 *                2  Full, the same as int32 values (modulus <= 2^31)
 *                3  ChaCha
 *   share_route  as sda_participant_last_launch reports it (2 Additive keyed, 4 PackedShamir keyed)
 *   share_bytes  4 or 8: the width of the share rows in handle scratch
 *   tiles        the tiles of the host form; 1 for the device form
 * sda_participant_last_launch describes the reused pipeline (its mask_route 5: a Full mask drawn in the masking
 * kernel).  A host-side record: nothing is waited for or copied.  No pointer may be NULL. */
sda_status sda_participant_job_last_launch(sda_engine* h, uint32_t* mask_route, uint32_t* share_route,
                                           uint32_t* share_bytes, uint64_t* tiles);

/* ---------------- recipient job: the recipient pipeline from the opened payloads ----------------
 * receive.rs:98-157 + positive() with the decode of every mask blob and clerk result (Decryptor::decrypt,
 * sodium.rs:82-90, receive.rs:101-146) done by the engine as well: the recipient hands over the opened payload
 * bytes, as the clerk does to sda_clerk_job.
 *
 * CONTRACT.  For any input, sda_recipient_job returns what sda_recipient_reveal returns when it is called with each
 * blob's sda_varint_decode output as the corresponding row: the status, the reference's message, *out_len and every
 * output value.  Blobs of different lengths are the normal case, and sda_recipient_reveal's rules for ragged rows
 * apply as they stand: Full mask blobs that decode to different lengths fail with full.rs:43's assertion
 * (SDA_ERR_PRECONDITION; row 0's `% 0` panic comes first), Additive clerk results of different lengths with
 * "Mismatching dimension" (4), PackedShamir clerk results are read over [0, B), a ChaCha seed is its first 8
 * values `as u32`, zero padded, and with no masking every blob must be empty.  A failing call writes nothing to
 * out and leaves every *_last_launch record of the handle as it was. */

/* Host form.  mask_blobs[i] (mask_lens[i] bytes) is participation i's opened mask payload -- a Full mask or a
 * ChaCha seed --, clerk_blobs[i] (clerk_lens[i] bytes) the opened result of clerk indices[i].
 *   Full masks stream through the decode -> combine of sda_clerk_decode_combine (full.rs:38-51 is combiner.rs:16-28's
 *   recurrence), a group of blobs in HBM at a time, so a mask set larger than HBM runs; seed blobs and clerk
 *   results are uploaded once.  On a multi-device handle the ChaCha mask combine is split over the devices as
 *   sda_recipient_reveal splits it (the decoded key words, 32 bytes a seed, are read back for that), and
 *   sda_recipient_last_launch then reports mask_kind 4; the rest runs on ordinals[0]. */
sda_status sda_recipient_job(sda_engine* h, const sda_masking_scheme* ms,
                             const uint8_t* const* mask_blobs, const uint64_t* mask_lens, uint64_t n_masks,
                             const sda_sharing_scheme* ss, uint64_t dimension, const uint64_t* indices,
                             const uint8_t* const* clerk_blobs, const uint64_t* clerk_lens, uint64_t n_idx,
                             int64_t output_modulus, int32_t mode,
                             int64_t* out, uint64_t out_cap, uint64_t* out_len);

/* Device form.  (seed_bytes, seed_off, n_seeds) and (clerk_bytes, clerk_off, n_idx) are laid out as
 * sda_clerk_decode_combine_dev takes its (bytes, blob_off, n_blobs): device bytes, 16-byte aligned and readable 16
 * bytes past the last blob, HOST offsets [n + 1], non-decreasing.
 *   Full masking: mask (device) is the already combined mask of mask_len values, read as it is.  That is the state
 *     sda_clerk_job_dev(h, ms->modulus, ..., payload = NULL) leaves after folding the mask payloads in any number
 *     of tiles (full.rs:38-51 is the clerk's recurrence), so a mask set larger than HBM is folded tile by tile and
 *     revealed with one call; SDA_ERR_WRONG_DIMENSION (3) from that fold stands for full.rs:43's assertion.
 *     mask_len == 0 is the empty mask of zero participations.  The unmask asserts mask_len == the output length,
 *     as sda_recipient_reveal_dev does.  The seed arguments are ignored.
 *   ChaCha masking: the seeds arrive as n_seeds blobs and their key words are decoded on the device; mask and
 *     mask_len are ignored.
 *   No masking: every blob passed must be empty.
 *   Additive clerk results are reconstructed by the clerk's decode -> combine straight into the pipeline's scratch
 *   (no [n_idx][D] matrix of i64 rows exists); PackedShamir results are counted, decoded into i64 rows of the
 *   longest result's length in handle scratch and revealed as sda_recipient_reveal_dev reveals them.
 *   sda_codec_last_launch, sda_combine_last_launch, sda_chacha_last_launch and sda_recipient_last_launch report
 *   what that reused code ran.
 * The call reads mask and the byte buffers only, and a failing call leaves all caller memory untouched.  It makes
 * one host wait before the reveal and the unmask are queued (the decode -> combine's, or the count pass's); with
 * ChaCha masking it drains its stream before returning, as sda_recipient_reveal_dev does.  Runs on ordinals[0] of
 * a multi-device handle; stream ordering on the handle is that of every _dev call. */
sda_status sda_recipient_job_dev(sda_engine* h, const sda_masking_scheme* ms,
                                 const int64_t* mask, uint64_t mask_len,
                                 const uint8_t* seed_bytes, const uint64_t* seed_off, uint64_t n_seeds,
                                 const sda_sharing_scheme* ss, uint64_t dimension, const uint64_t* indices,
                                 const uint8_t* clerk_bytes, const uint64_t* clerk_off, uint64_t n_idx,
                                 int64_t output_modulus, int32_t mode,
                                 int64_t* out, uint64_t out_cap, uint64_t* out_len, void* stream);

/* Diagnostic (read-only): where the handle's most recent sda_recipient_job / sda_recipient_job_dev took its inputs
 * from.  Written when such a call returns SDA_OK with a non-empty output, as sda_recipient_last_launch is; before
 * any such call every field is 0.
 *   mask_route     0  no masking
 *                  1  Full, the caller's combined mask (sda_recipient_job_dev)
 *                  2  Full, the blobs streamed through decode -> combine (sda_recipient_job)
 *                  3  ChaCha, the seeds decoded on the device
 *                  4  as 3, then the mask combine split over the handle's devices
 *   share_route    1  Additive: decode -> combine
 *                  2  PackedShamir: count pass + i64 rows
 *   seeds_decoded  the blobs the seed kernel handled
 * A host-side record: nothing is waited for or copied.  No pointer may be NULL. */
sda_status sda_recipient_job_last_launch(sda_engine* h, uint32_t* mask_route, uint32_t* share_route,
                                         uint32_t* seeds_decoded);

/* ---------------- robust recipient job: the recipient pipeline over the decoded reveal ----------------
 * The recipient job with sda_packed_reveal_decoded_dev as its reveal: up to e_max = floor(r / 2) wrong clerk results
 * per batch (r = n_idx - (k + t); truncated to a wrong value, stale, reduced by another modulus, ...) are located,
 * blamed on their clerks and corrected inside the one call, and a batch with more is flagged, never returned as
 * if it were right.  sda_recipient_job itself reveals from whatever it is given and returns SDA_OK.
 *
 * CONTRACT.  With p = ss->modulus, B = ceil(dimension / k) and clerk row i = sda_varint_decode(clerk_blobs[i]) read
 * over [0, B) (sda_recipient_reveal_decoded_dev: row i of `shares`), the call reveals what
 * sda_secret_reconstruct_decoded reveals from those rows -- the secrets s, verdict, wrong, *redundancy, *radius,
 * *bad_batches, *first_bad, *undecoded and blame[n_idx], bit for bit -- and returns
 *     out[i] = (s_i - mask_i) mod p  in [0, p),   i < dimension,
 * where mask is the combined mask exactly as sda_recipient_job / sda_recipient_job_dev / sda_recipient_reveal_dev
 * builds or takes it (no masking: mask_i = 0) and every i64 mask value is reduced exactly.  The output is DEFINED as
 * that residue, not through the reference's wrapping `-` (full.rs:58-66, chacha.rs:83-91) followed by positive(): a
 * corrected batch has no counterpart in the reference.  For every mask an engine call produces (values in (-p, p))
 * the two agree.  Consequences:
 *   - with no more than e_max wrong results in any batch, out equals sda_recipient_job's output on the uncorrupted
 *     payloads, *undecoded == 0, and blame counts the batches in which each clerk was wrong;
 *   - on consistent results, out equals sda_recipient_job's output on the same payloads, in either mode, and every
 *     count is zero.
 * SCOPE.  Defined only where the decoded reveal's canonical output is the whole answer; everything else is refused
 * with SDA_ERR_UNSUPPORTED on the schemes alone, right after the NULL checks and before any data is looked at:
 *   an Additive sharing scheme ("Additive"); k > 8 ("secrets per batch"); output_modulus != p ("output_modulus");
 *   Full or ChaCha masking with |ms->modulus| != p ("masking modulus").
 * After them come sda_recipient_job's own checks in its order, with its statuses and messages (the mask combine's,
 * the scheme's, the count pass's, index out of bounds, Not enough shares), except that more than 32 clerk results
 * are refused (SDA_ERR_UNSUPPORTED) where the job refuses more than 1023.  Repeated clerk indices are refused
 * (SDA_ERR_UNSUPPORTED) when the check table is built: after the length and out_cap checks, before anything is
 * written.  dimension == 0 returns SDA_OK, *out_len = 0 and sda_secret_reconstruct_decoded's counts for it
 * (*redundancy = max(n_idx, k + t) - (k + t), *first_bad = UINT64_MAX, the rest 0) and launches nothing; r == 0 and
 * r == 1 behave as the decoded reveal does (nothing is correctable, a bad batch is flagged 0xFFFF and undecoded).
 * A failing call writes nothing to out, verdict, wrong or any host output and leaves every *_last_launch record of
 * the handle as it was.  A multi-device handle behaves as in sda_recipient_job.
 *
 * verdict: uint16 [B] or NULL, wrong: uint32 [B] or NULL, independently; both as sda_packed_reveal_decoded_dev
 * writes them for one vector.  redundancy, radius, bad_batches, first_bad and undecoded may not be NULL, nor blame
 * when n_idx > 0.  The reused code fills sda_packed_decode_last_launch, sda_codec_last_launch,
 * sda_chacha_last_launch, sda_combine_last_launch, sda_recipient_last_launch (reveal_mode 2; unmask_launches counts
 * the separate unmask passes, 0 on routes 0 and 1 below) and sda_recipient_job_last_launch as it does today.
 *
 * ChaCha masking: the mask combine is queued ahead of the reveal, whose write-back reads the finished mask.  Should
 * the combine report rejected draws (probability about 2^-33 a draw at these moduli), the mask is fixed and the
 * reveal passes run again over the same inputs.
 * Knobs, read per call: SDA_RECIPIENT_FUSE_UNMASK=0 runs the plain first pass into scratch and unmasks in a pass of
 * its own (route 2); SDA_RECIPIENT_REDO=1 takes the rerun branch of a ChaCha call as if its mask had changed. */

/* Host form: sda_recipient_job's arguments without `mode`; verdict and wrong are HOST buffers. */
sda_status
sda_recipient_job_decoded(sda_engine* h, const sda_masking_scheme* ms,
                          const uint8_t* const* mask_blobs, const uint64_t* mask_lens, uint64_t n_masks,
                          const sda_sharing_scheme* ss, uint64_t dimension, const uint64_t* indices,
                          const uint8_t* const* clerk_blobs, const uint64_t* clerk_lens, uint64_t n_idx,
                          int64_t output_modulus, int64_t* out, uint64_t out_cap, uint64_t* out_len,
                          void* verdict, void* wrong, uint64_t* redundancy, uint64_t* radius,
                          uint64_t* bad_batches, uint64_t* first_bad, uint64_t* undecoded, uint64_t* blame);

/* Device form: sda_recipient_job_dev's arguments without `mode`; verdict and wrong are DEVICE buffers (wrong 4-byte
 * aligned, else SDA_ERR_INVALID_ARGUMENT).  The call drains its stream before returning: it returns counts. */
sda_status
sda_recipient_job_decoded_dev(sda_engine* h, const sda_masking_scheme* ms,
                              const int64_t* mask, uint64_t mask_len,
                              const uint8_t* seed_bytes, const uint64_t* seed_off, uint64_t n_seeds,
                              const sda_sharing_scheme* ss, uint64_t dimension, const uint64_t* indices,
                              const uint8_t* clerk_bytes, const uint64_t* clerk_off, uint64_t n_idx,
                              int64_t output_modulus, int64_t* out, uint64_t out_cap, uint64_t* out_len,
                              void* verdict, void* wrong, uint64_t* redundancy, uint64_t* radius,
                              uint64_t* bad_batches, uint64_t* first_bad, uint64_t* undecoded, uint64_t* blame,
                              void* stream);

/* The clerk results as device i64 rows [n_idx][share_len]: sda_recipient_reveal_dev's arguments without `mode`, the
 * outputs of the device form above.  Drains its stream before returning. */
sda_status sda_recipient_reveal_decoded_dev(sda_engine* h, const sda_masking_scheme* ms, const void* mask_in,
                                            uint64_t n_masks, uint64_t mask_width, const sda_sharing_scheme* ss,
                                            uint64_t dimension, const uint64_t* indices, const int64_t* shares,
                                            uint64_t n_idx, uint64_t share_len, int64_t output_modulus,
                                            int64_t* out, uint64_t out_cap, uint64_t* out_len,
                                            void* verdict, void* wrong, uint64_t* redundancy, uint64_t* radius,
                                            uint64_t* bad_batches, uint64_t* first_bad, uint64_t* undecoded,
                                            uint64_t* blame, void* stream);

/* Diagnostic (read-only): how the handle's most recent robust recipient call ran.  Written when such a call returns
 * SDA_OK with a non-empty output, as sda_recipient_last_launch is; before any such call every field is 0.
 *   unmask_route  0  no masking: the reveal wrote out itself
 *                 1  the mask subtracted in the first pass's write-back (recipient_repair_kernel)
 *                 2  a separate unmask pass behind the plain first pass (SDA_RECIPIENT_FUSE_UNMASK=0)
 *   reveal_runs   1, or 2 when the reveal passes ran again behind a ChaCha mask that changed
 *   compact       as in sda_recipient_last_launch: the clerk rows were longer than B and compacted first
 * A host-side record: nothing is waited for or copied.  No pointer may be NULL. */
sda_status sda_recipient_decoded_last_launch(sda_engine* h, uint32_t* unmask_route, uint32_t* reveal_runs,
                                             uint32_t* compact);

/* Synthetic benchmark input: dst[r*cols + c] = lo + splitmix64(seed, r, c) % (hi - lo). */
sda_status sda_synth_fill_dev(sda_engine* h, int64_t* dst, uint64_t rows, uint64_t cols,
                              uint64_t seed, int64_t lo, int64_t hi, void* stream);

/* HBM for the resident hot-path buffers (no reference counterpart: the reference's buffers are Rust
 * Vec<i64> on the host, batched.rs:25-28).  `bytes` of device memory on `device`, one virtual range
 * mapped from physical chunks of SDA_HBM_CHUNK_MB (default 64) MiB, so its backing never depends on how
 * fragmented the driver's free VRAM is.  The request is rounded up to whole chunks, and
 * belongs to a size class (n chunks: n up to 4, then 4..7 x 2^e, at most 25 % more): the buffer reserves
 * its class's virtual range and maps the chunks asked for.
 * sda_hbm_free does not wait: the buffer returns to a per-process pool, still mapped, and a later
 * sda_hbm_alloc of the same size class gets it back (after a device-wide sync if none has completed since
 * the free; extra chunks, if it needs more, are mapped at the range's never-mapped tail).  The pool holds
 * at most SDA_HBM_POOL_MB (default 32768) MiB per device: an allocation that finds no pooled buffer of its
 * class trims the oldest pooled buffers down to that bound, and trims the whole pool and retries once when
 * the device is out of memory.  Trimming syncs the device and releases the physical chunks; the virtual
 * range stays reserved and is never mapped again (DESIGN.md §2 gives the cause).  NULL is a no-op; a
 * pointer not returned by sda_hbm_alloc, or freed twice, is INVALID_ARGUMENT.  Thread-safe; no lock is
 * held across a device sync. */
sda_status sda_hbm_alloc(int device, uint64_t bytes, void** out);
sda_status sda_hbm_free(void* ptr);
/* Release pooled buffers of `device` (oldest first) until at most keep_bytes stay pooled.
 * Destroying the last live engine handle of a device trims that device's pool to 0. */
sda_status sda_hbm_trim(int device, uint64_t keep_bytes);
/* Bytes of `device` handed out and pooled (mapped chunks), and retired (virtual ranges kept reserved
 * after a trim; a steady stream of jobs whose buffers fit the pool retires none); any pointer may be
 * NULL. */
sda_status sda_hbm_stats(int device, uint64_t* live_bytes, uint64_t* pooled_bytes, uint64_t* retired_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SDA_ENGINE_H */
