//! Raw declarations of `include/sda_engine.h` (ABI version 1), one to one: same names, same argument
//! order, same integer widths.  `tests/test_rust_ffi.py` parses this `extern "C"` block and the C header
//! and fails on any difference.  UNCOMPILED here (the image has no cargo / rustc).
#![allow(non_camel_case_types, dead_code)]

use libc::{c_char, c_int, c_void};

pub const SDA_ENGINE_ABI_VERSION: c_int = 1;

/// `sda_status` (include/sda_engine.h); 1..=6 are the reference's error strings.
pub type SdaStatus = c_int;
pub const SDA_OK: SdaStatus = 0;
pub const SDA_ERR_BATCH_INPUT_WRONG_LENGTH: SdaStatus = 1;      // additive.rs:33
pub const SDA_ERR_PACKED_SHARING_FAILED: SdaStatus = 2;         // packed_shamir.rs:41
pub const SDA_ERR_WRONG_DIMENSION: SdaStatus = 3;               // combiner.rs:21
pub const SDA_ERR_MISMATCHING_DIMENSION: SdaStatus = 4;         // additive.rs:64
pub const SDA_ERR_INPUTS_MUST_HAVE_SAME_LENGTH: SdaStatus = 5;  // packed_shamir.rs:74
pub const SDA_ERR_NOT_ENOUGH_SHARES: SdaStatus = 6;             // packed_shamir.rs:75
pub const SDA_ERR_PRECONDITION: SdaStatus = 64;                 // where the reference panics
pub const SDA_ERR_INVALID_ARGUMENT: SdaStatus = 65;
pub const SDA_ERR_UNSUPPORTED: SdaStatus = 66;
pub const SDA_ERR_DEVICE: SdaStatus = 67;
pub const SDA_ERR_OUT_OF_MEMORY: SdaStatus = 68;

pub const SDA_SHARING_ADDITIVE: i32 = 0;
pub const SDA_SHARING_PACKED_SHAMIR: i32 = 1;
pub const SDA_MASKING_NONE: i32 = 0;
pub const SDA_MASKING_FULL: i32 = 1;
pub const SDA_MASKING_CHACHA: i32 = 2;
pub const SDA_REVEAL_EXACT: i32 = 0;
pub const SDA_REVEAL_CANONICAL: i32 = 1;

/// `sda_sharing_scheme`: protocol/src/crypto.rs:79-114 LinearSecretSharingScheme.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SdaSharingScheme {
    pub kind: i32,
    pub share_count: u64,
    pub modulus: i64,
    pub secret_count: u64,
    pub privacy_threshold: u64,
    pub omega_secrets: i64,
    pub omega_shares: i64,
}

/// `sda_masking_scheme`: protocol/src/crypto.rs:43-64 LinearMaskingScheme.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SdaMaskingScheme {
    pub kind: i32,
    pub modulus: i64,
    pub dimension: u64,
    pub seed_bitsize: u64,
}

/// Opaque `sda_engine`.
#[repr(C)]
pub struct SdaEngine {
    _private: [u8; 0],
}

#[link(name = "sda_engine")]
extern "C" {
    // ---- lifecycle / diagnostics ----
    pub fn sda_abi_version() -> c_int;
    pub fn sda_engine_create(device_ordinal: c_int, out: *mut *mut SdaEngine) -> SdaStatus;
    pub fn sda_engine_destroy(h: *mut SdaEngine);
    pub fn sda_engine_synchronize(h: *mut SdaEngine) -> SdaStatus;
    pub fn sda_engine_create_multi(ordinals: *const c_int, n_devices: c_int, out: *mut *mut SdaEngine) -> SdaStatus;
    pub fn sda_engine_device_count(h: *const SdaEngine) -> c_int;
    pub fn sda_last_error_message() -> *const c_char;
    pub fn sda_status_string(status: c_int) -> *const c_char;

    // ---- derived scheme sizes: protocol/src/crypto.rs:117-155 ----
    pub fn sda_scheme_input_size(s: *const SdaSharingScheme) -> u64;
    pub fn sda_scheme_output_size(s: *const SdaSharingScheme) -> u64;
    pub fn sda_scheme_privacy_threshold(s: *const SdaSharingScheme) -> u64;
    pub fn sda_scheme_reconstruction_threshold(s: *const SdaSharingScheme) -> u64;
    pub fn sda_share_length(s: *const SdaSharingScheme, dimension: u64) -> u64;

    // ---- trait mirrors (host buffers, synchronous) ----
    pub fn sda_share_generate(h: *mut SdaEngine, s: *const SdaSharingScheme, secrets: *const i64, dimension: u64,
                              draws: *const i64, n_draws: u64, out: *mut i64, out_cap: u64) -> SdaStatus;
    pub fn sda_share_generate_keyed(h: *mut SdaEngine, s: *const SdaSharingScheme, secrets: *const i64,
                                    dimension: u64, key: *const u32, stream_id: u32, out: *mut i64, out_cap: u64)
                                    -> SdaStatus;
    pub fn sda_share_combine(h: *mut SdaEngine, s: *const SdaSharingScheme, rows: *const *const i64,
                             lens: *const u64, n_rows: u64, out: *mut i64, out_cap: u64, out_len: *mut u64)
                             -> SdaStatus;
    pub fn sda_secret_reconstruct(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64,
                                  indices: *const u64, rows: *const *const i64, lens: *const u64, n_rows: u64,
                                  out: *mut i64, out_cap: u64, out_len: *mut u64) -> SdaStatus;
    pub fn sda_secret_mask(h: *mut SdaEngine, s: *const SdaMaskingScheme, secrets: *const i64, dimension: u64,
                           seed: *const u32, seed_words: u64, full_masks: *const i64, mask_out: *mut i64,
                           mask_cap: u64, mask_len: *mut u64, masked_out: *mut i64) -> SdaStatus;
    pub fn sda_secret_mask_keyed(h: *mut SdaEngine, s: *const SdaMaskingScheme, secrets: *const i64, dimension: u64,
                                 key: *const u32, stream_id: u32, mask_out: *mut i64, mask_cap: u64,
                                 mask_len: *mut u64, masked_out: *mut i64) -> SdaStatus;
    pub fn sda_mask_combine(h: *mut SdaEngine, s: *const SdaMaskingScheme, rows: *const *const i64,
                            lens: *const u64, n_rows: u64, out: *mut i64, out_cap: u64, out_len: *mut u64)
                            -> SdaStatus;
    pub fn sda_secret_unmask(h: *mut SdaEngine, s: *const SdaMaskingScheme, mask: *const i64, mask_len: u64,
                             masked: *const i64, masked_len: u64, out: *mut i64, out_cap: u64, out_len: *mut u64)
                             -> SdaStatus;
    pub fn sda_recipient_positive(h: *mut SdaEngine, modulus: i64, values: *const i64, n: u64, out: *mut i64)
                                  -> SdaStatus;

    // ---- device-resident entry points ----
    pub fn sda_combine_dev(h: *mut SdaEngine, modulus: i64, shares: *const i64, n: u64, dim: u64, row_stride: u64,
                           out: *mut i64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_combine_accumulate_dev(h: *mut SdaEngine, modulus: i64, shares: *const i64, n: u64, dim: u64,
                                      row_stride: u64, inout: *mut i64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_combine32_dev(h: *mut SdaEngine, modulus: i64, shares: *const i32, n: u64, dim: u64, row_stride: u64,
                             out: *mut i64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_combine32_accumulate_dev(h: *mut SdaEngine, modulus: i64, shares: *const i32, n: u64, dim: u64,
                                        row_stride: u64, inout: *mut i64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_narrow32_dev(h: *mut SdaEngine, src: *const i64, n: u64, dim: u64, src_stride: u64, dst: *mut i32,
                            dst_stride: u64, flag: *mut i64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_host_stream_stats(h: *const SdaEngine, tiles_i32: *mut u64, tiles_i64: *mut u64,
                                 bytes_h2d: *mut u64) -> SdaStatus;
    pub fn sda_packed_fixup_count(h: *mut SdaEngine, batches: *mut u64) -> SdaStatus;
    pub fn sda_chacha_last_launch(h: *mut SdaEngine, path: *mut u32, grid_y: *mut u64, fixups: *mut u64)
                                  -> SdaStatus;
    pub fn sda_codec_last_launch(h: *mut SdaEngine, path: *mut u32, width: *mut u32, fell_back: *mut u32,
                                 passes: *mut u64) -> SdaStatus;
    pub fn sda_combine_last_launch(h: *mut SdaEngine, kind: *mut u32, elem_bytes: *mut u32, vec: *mut u32,
                                   rows: *mut u32, variant: *mut u32, grid: *mut u64, wlo: *mut u32,
                                   nwide: *mut u32, per_cu: *mut u32) -> SdaStatus;
    pub fn sda_snapshot_last_launch(h: *mut SdaEngine, blobs: *mut u64, chunks: *mut u64, grid: *mut u64,
                                    chunk_bytes: *mut u64, shifts: *mut u32) -> SdaStatus;
    pub fn sda_recipient_last_launch(h: *mut SdaEngine, mask_kind: *mut u32, reveal_mode: *mut u32,
                                     fell_back: *mut u32, compact: *mut u32, unmask_launches: *mut u32) -> SdaStatus;
    pub fn sda_participant_last_launch(h: *mut SdaEngine, mask_route: *mut u32, share_route: *mut u32,
                                       passes: *mut u32) -> SdaStatus;
    pub fn sda_combine_finalize_dev(h: *mut SdaEngine, modulus: i64, sums: *const i64, dim: u64, out: *mut i64,
                                    stream: *mut c_void) -> SdaStatus;
    pub fn sda_combine_split_dev(h: *mut SdaEngine, modulus: i64, shares: *const i64, n: u64, dim: u64,
                                 row_stride: u64, inout: *mut i64, flags: *mut i64, stream: *mut c_void)
                                 -> SdaStatus;
    pub fn sda_combine_split_prefix_dev(h: *mut SdaEngine, modulus: i64, gathered: *const i64, world: u64,
                                        rank: u64, dim: u64, c_in: *mut i64, total: *mut i64, code: *mut i32,
                                        stream: *mut c_void) -> SdaStatus;
    pub fn sda_combine_split_replay_dev(h: *mut SdaEngine, modulus: i64, shares: *const i64, n: u64, dim: u64,
                                        row_stride: u64, rank: u64, state: *mut i64, code: *mut i32,
                                        stream: *mut c_void) -> SdaStatus;
    pub fn sda_combine_split_resolve_dev(h: *mut SdaEngine, modulus: i64, total: *const i64, code: *const i32,
                                         dim: u64, out: *mut i64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_packed_generate_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, secrets: *const i64,
                                   dimension: u64, n_vectors: u64, draws: *const i64, out: *mut i64,
                                   stream: *mut c_void) -> SdaStatus;
    pub fn sda_packed_generate_mode_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, secrets: *const i64,
                                        dimension: u64, n_vectors: u64, draws: *const i64, out: *mut i64,
                                        mode: i32, stream: *mut c_void) -> SdaStatus;
    pub fn sda_packed_reconstruct_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64,
                                      indices: *const u64, n_idx: u64, n_vectors: u64, shares: *const i64,
                                      out: *mut i64, mode: i32, stream: *mut c_void) -> SdaStatus;
    pub fn sda_packed_generate32_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, secrets: *const i64,
                                     dimension: u64, n_vectors: u64, draws: *const i64, out: *mut i32, mode: i32,
                                     stream: *mut c_void) -> SdaStatus;
    pub fn sda_packed_reconstruct32_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64,
                                        indices: *const u64, n_idx: u64, n_vectors: u64, shares: *const i32,
                                        out: *mut i64, mode: i32, stream: *mut c_void) -> SdaStatus;
    // share consistency check of a reveal's input; verdict: u16 [n_vectors][B] on the device (host [B] for
    // sda_secret_check) or NULL
    pub fn sda_packed_check_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64, indices: *const u64,
                                n_idx: u64, n_vectors: u64, shares: *const i64, verdict: *mut c_void,
                                redundancy: *mut u64, bad_batches: *mut u64, first_bad: *mut u64, blame: *mut u64,
                                stream: *mut c_void) -> SdaStatus;
    pub fn sda_packed_check32_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64,
                                  indices: *const u64, n_idx: u64, n_vectors: u64, shares: *const i32,
                                  verdict: *mut c_void, redundancy: *mut u64, bad_batches: *mut u64,
                                  first_bad: *mut u64, blame: *mut u64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_secret_check(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64, indices: *const u64,
                            share_rows: *const *const i64, share_lens: *const u64, n_idx: u64, verdict: *mut c_void,
                            redundancy: *mut u64, bad_batches: *mut u64, first_bad: *mut u64, blame: *mut u64)
                            -> SdaStatus;
    pub fn sda_packed_check_last_launch(h: *mut SdaEngine, path: *mut u32, bucket: *mut u32, located: *mut u64,
                                        overflowed: *mut u32) -> SdaStatus;
    // checked reveal: the check's arguments plus out (i64 [n_vectors][dimension] on the device; host [dimension]
    // for sda_secret_reconstruct_checked)
    pub fn sda_packed_reveal_checked_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64,
                                         indices: *const u64, n_idx: u64, n_vectors: u64, shares: *const i64,
                                         out: *mut i64, verdict: *mut c_void, redundancy: *mut u64,
                                         bad_batches: *mut u64, first_bad: *mut u64, blame: *mut u64,
                                         stream: *mut c_void) -> SdaStatus;
    pub fn sda_packed_reveal_checked32_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64,
                                           indices: *const u64, n_idx: u64, n_vectors: u64, shares: *const i32,
                                           out: *mut i64, verdict: *mut c_void, redundancy: *mut u64,
                                           bad_batches: *mut u64, first_bad: *mut u64, blame: *mut u64,
                                           stream: *mut c_void) -> SdaStatus;
    pub fn sda_secret_reconstruct_checked(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64,
                                          indices: *const u64, share_rows: *const *const i64,
                                          share_lens: *const u64, n_idx: u64, verdict: *mut c_void,
                                          redundancy: *mut u64, bad_batches: *mut u64, first_bad: *mut u64,
                                          blame: *mut u64, out: *mut i64) -> SdaStatus;
    pub fn sda_packed_reveal_checked_last_launch(h: *mut SdaEngine, path: *mut u32, bucket: *mut u32,
                                                 fixed: *mut u64, overflowed: *mut u32) -> SdaStatus;
    // decoded reveal: the checked reveal's arguments plus wrong (u32 [n_vectors][B] on the device, host [B] for
    // sda_secret_reconstruct_decoded, or NULL), the radius and the undecodable count
    pub fn sda_packed_reveal_decoded_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64,
                                         indices: *const u64, n_idx: u64, n_vectors: u64, shares: *const i64,
                                         out: *mut i64, verdict: *mut c_void, wrong: *mut c_void,
                                         redundancy: *mut u64, radius: *mut u64, bad_batches: *mut u64,
                                         first_bad: *mut u64, undecoded: *mut u64, blame: *mut u64,
                                         stream: *mut c_void) -> SdaStatus;
    pub fn sda_packed_reveal_decoded32_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64,
                                           indices: *const u64, n_idx: u64, n_vectors: u64, shares: *const i32,
                                           out: *mut i64, verdict: *mut c_void, wrong: *mut c_void,
                                           redundancy: *mut u64, radius: *mut u64, bad_batches: *mut u64,
                                           first_bad: *mut u64, undecoded: *mut u64, blame: *mut u64,
                                           stream: *mut c_void) -> SdaStatus;
    pub fn sda_secret_reconstruct_decoded(h: *mut SdaEngine, s: *const SdaSharingScheme, dimension: u64,
                                          indices: *const u64, share_rows: *const *const i64,
                                          share_lens: *const u64, n_idx: u64, verdict: *mut c_void,
                                          wrong: *mut c_void, redundancy: *mut u64, radius: *mut u64,
                                          bad_batches: *mut u64, first_bad: *mut u64, undecoded: *mut u64,
                                          blame: *mut u64, out: *mut i64) -> SdaStatus;
    pub fn sda_packed_decode_last_launch(h: *mut SdaEngine, path: *mut u32, bucket: *mut u32, decoded: *mut u64,
                                         fixed: *mut u64, max_errors: *mut u32, overflowed: *mut u32) -> SdaStatus;
    pub fn sda_additive_generate_dev(h: *mut SdaEngine, modulus: i64, share_count: u64, secrets: *const i64,
                                     dimension: u64, draws: *const i64, out: *mut i64, stream: *mut c_void)
                                     -> SdaStatus;
    pub fn sda_chacha_mask_combine_dev(h: *mut SdaEngine, modulus: i64, dimension: u64, seeds: *const u32, w: u64,
                                       n_seeds: u64, out: *mut i64, stream: *mut c_void) -> SdaStatus;

    // ---- device-side draws: one OS-RNG key per call, expanded with ChaCha20 on the device ----
    pub fn sda_draws_dev(h: *mut SdaEngine, key: *const u32, stream_id: u32, first: u64, count: u64, bound: i64,
                         out: *mut i64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_draws(h: *mut SdaEngine, key: *const u32, stream_id: u32, first: u64, count: u64, bound: i64,
                     out: *mut i64, out_cap: u64) -> SdaStatus;
    // Additive share generation with the draws made inside the kernel; the 32 form writes int32 rows (m <= 2^31)
    pub fn sda_additive_generate_keyed_dev(h: *mut SdaEngine, modulus: i64, share_count: u64, secrets: *const i64,
                                           dimension: u64, key: *const u32, stream_id: u32, first_column: u64,
                                           out: *mut i64, out_stride: u64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_additive_generate_keyed32_dev(h: *mut SdaEngine, modulus: i64, share_count: u64, secrets: *const i64,
                                             dimension: u64, key: *const u32, stream_id: u32, first_column: u64,
                                             out: *mut i32, out_stride: u64, stream: *mut c_void) -> SdaStatus;
    // Packed-Shamir share generation with the draws made in the share kernels (staged in handle-owned scratch for
    // the schemes those kernels do not serve); the record tells which: path 1 in-kernel, 2 staged
    pub fn sda_packed_generate_keyed_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, secrets: *const i64,
                                         dimension: u64, n_vectors: u64, key: *const u32, stream_id: u32,
                                         first_batch: u64, out: *mut i64, mode: i32, stream: *mut c_void)
                                         -> SdaStatus;
    pub fn sda_packed_generate_keyed32_dev(h: *mut SdaEngine, s: *const SdaSharingScheme, secrets: *const i64,
                                           dimension: u64, n_vectors: u64, key: *const u32, stream_id: u32,
                                           first_batch: u64, out: *mut i32, mode: i32, stream: *mut c_void)
                                           -> SdaStatus;
    pub fn sda_packed_keyed_last_launch(h: *mut SdaEngine, path: *mut u32, staged_bytes: *mut u64) -> SdaStatus;

    // ---- share payload codec (sodium.rs:36-41, :82-88) ----
    pub fn sda_varint_encode(h: *mut SdaEngine, vals: *const i64, n: u64, out: *mut u8, out_cap: u64,
                             out_len: *mut u64) -> SdaStatus;
    pub fn sda_varint_decode(h: *mut SdaEngine, bytes: *const u8, n_bytes: u64, out: *mut i64, out_cap: u64,
                             out_len: *mut u64) -> SdaStatus;
    pub fn sda_clerk_decode_combine(h: *mut SdaEngine, s: *const SdaSharingScheme, blobs: *const *const u8,
                                    blob_lens: *const u64, n_blobs: u64, out: *mut i64, out_cap: u64,
                                    out_len: *mut u64) -> SdaStatus;
    pub fn sda_varint_decode_dev(h: *mut SdaEngine, bytes: *const u8, blob_off: *const u64, n_blobs: u64,
                                 out: *mut i64, out_stride: u64, counts: *mut u64, stream: *mut c_void)
                                 -> SdaStatus;
    pub fn sda_clerk_decode_combine_dev(h: *mut SdaEngine, modulus: i64, bytes: *const u8, blob_off: *const u64,
                                        n_blobs: u64, out: *mut i64, out_cap: u64, out_len: *mut u64,
                                        stream: *mut c_void) -> SdaStatus;
    pub fn sda_varint_encode_dev(h: *mut SdaEngine, vals: *const i64, rows: u64, len: u64, stride: u64,
                                 dst: *mut u8, dst_cap: u64, row_bytes: *mut u64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_varint_encode32_dev(h: *mut SdaEngine, vals: *const i32, rows: u64, len: u64, stride: u64,
                                   dst: *mut u8, dst_cap: u64, row_bytes: *mut u64, stream: *mut c_void) -> SdaStatus;
    // The clerk's whole arithmetic step (clerk.rs:63-107): decode, combine (continued from `state` when
    // first_participation > 0) and the recipient's payload in one call; sda_clerk_job is the host-memory form
    pub fn sda_clerk_job_dev(h: *mut SdaEngine, modulus: i64, bytes: *const u8, blob_off: *const u64, n_blobs: u64,
                             first_participation: u64, prior_dim: u64, state: *mut i64, state_cap: u64,
                             dim_out: *mut u64, payload: *mut u8, payload_cap: u64, payload_len: *mut u64,
                             stream: *mut c_void) -> SdaStatus;
    pub fn sda_clerk_job(h: *mut SdaEngine, s: *const SdaSharingScheme, blobs: *const *const u8,
                         blob_lens: *const u64, n_blobs: u64, out: *mut i64, out_cap: u64, out_len: *mut u64,
                         payload: *mut u8, payload_cap: u64, payload_len: *mut u64) -> SdaStatus;
    pub fn sda_clerk_job_last_launch(h: *mut SdaEngine, continued: *mut u32, encode_route: *mut u32,
                                     encode_chunks: *mut u64) -> SdaStatus;

    // ---- snapshot transposition (server/src/stores.rs:86-101) ----
    pub fn sda_snapshot_transpose_dev(h: *mut SdaEngine, src: *const u8, part_off: *const u64,
                                      n_participations: u64, n_clerks: u64, dst: *mut u8, dst_cap: u64,
                                      dst_len: *mut u64, clerk_base: *mut u64, clerk_off: *mut u64,
                                      stream: *mut c_void) -> SdaStatus;

    // ---- fused role pipelines ----
    pub fn sda_recipient_reveal_dev(h: *mut SdaEngine, ms: *const SdaMaskingScheme, mask_in: *const c_void,
                                    n_masks: u64, mask_width: u64, ss: *const SdaSharingScheme, dimension: u64,
                                    indices: *const u64, shares: *const i64, n_idx: u64, share_len: u64,
                                    output_modulus: i64, mode: i32, out: *mut i64, out_cap: u64,
                                    out_len: *mut u64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_recipient_reveal(h: *mut SdaEngine, ms: *const SdaMaskingScheme, mask_rows: *const *const i64,
                                mask_lens: *const u64, n_masks: u64, ss: *const SdaSharingScheme, dimension: u64,
                                indices: *const u64, share_rows: *const *const i64, share_lens: *const u64,
                                n_idx: u64, output_modulus: i64, mode: i32, out: *mut i64, out_cap: u64,
                                out_len: *mut u64) -> SdaStatus;
    pub fn sda_participant_share_dev(h: *mut SdaEngine, ms: *const SdaMaskingScheme, seed: *const u32,
                                     seed_words: u64, full_masks: *const i64, ss: *const SdaSharingScheme,
                                     secrets: *const i64, dimension: u64, draws: *const i64, mode: i32,
                                     shares_out: *mut i64, payload: *mut u8, payload_cap: u64,
                                     payload_row_bytes: *mut u64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_participant_share32_dev(h: *mut SdaEngine, ms: *const SdaMaskingScheme, seed: *const u32,
                                       seed_words: u64, full_masks: *const i64, ss: *const SdaSharingScheme,
                                       secrets: *const i64, dimension: u64, draws: *const i64, mode: i32,
                                       shares_out: *mut i32, payload: *mut u8, payload_cap: u64,
                                       payload_row_bytes: *mut u64, stream: *mut c_void) -> SdaStatus;
    // the two calls above with the share-generation draws made on the device from (key, stream_id); the 32 form
    // takes an Additive scheme with modulus <= 2^31
    pub fn sda_participant_share_keyed_dev(h: *mut SdaEngine, ms: *const SdaMaskingScheme, seed: *const u32,
                                           seed_words: u64, full_masks: *const i64, ss: *const SdaSharingScheme,
                                           secrets: *const i64, dimension: u64, key: *const u32, stream_id: u32,
                                           mode: i32, shares_out: *mut i64, payload: *mut u8, payload_cap: u64,
                                           payload_row_bytes: *mut u64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_participant_share32_keyed_dev(h: *mut SdaEngine, ms: *const SdaMaskingScheme, seed: *const u32,
                                             seed_words: u64, full_masks: *const i64, ss: *const SdaSharingScheme,
                                             secrets: *const i64, dimension: u64, key: *const u32, stream_id: u32,
                                             mode: i32, shares_out: *mut i32, payload: *mut u8, payload_cap: u64,
                                             payload_row_bytes: *mut u64, stream: *mut c_void) -> SdaStatus;

    // ---- recipient job: the recipient pipeline from the opened payloads ----
    pub fn sda_recipient_job(h: *mut SdaEngine, ms: *const SdaMaskingScheme, mask_blobs: *const *const u8,
                             mask_lens: *const u64, n_masks: u64, ss: *const SdaSharingScheme, dimension: u64,
                             indices: *const u64, clerk_blobs: *const *const u8, clerk_lens: *const u64, n_idx: u64,
                             output_modulus: i64, mode: i32, out: *mut i64, out_cap: u64, out_len: *mut u64)
        -> SdaStatus;
    pub fn sda_recipient_job_dev(h: *mut SdaEngine, ms: *const SdaMaskingScheme, mask: *const i64, mask_len: u64,
                                 seed_bytes: *const u8, seed_off: *const u64, n_seeds: u64,
                                 ss: *const SdaSharingScheme, dimension: u64, indices: *const u64,
                                 clerk_bytes: *const u8, clerk_off: *const u64, n_idx: u64, output_modulus: i64,
                                 mode: i32, out: *mut i64, out_cap: u64, out_len: *mut u64, stream: *mut c_void)
        -> SdaStatus;
    pub fn sda_recipient_job_last_launch(h: *mut SdaEngine, mask_route: *mut u32, share_route: *mut u32,
                                         seeds_decoded: *mut u32) -> SdaStatus;

    // ---- robust recipient job: the same calls over the decoded reveal (wrong clerk results corrected) ----
    pub fn sda_recipient_job_decoded(h: *mut SdaEngine, ms: *const SdaMaskingScheme, mask_blobs: *const *const u8,
                                     mask_lens: *const u64, n_masks: u64, ss: *const SdaSharingScheme,
                                     dimension: u64, indices: *const u64, clerk_blobs: *const *const u8,
                                     clerk_lens: *const u64, n_idx: u64, output_modulus: i64, out: *mut i64,
                                     out_cap: u64, out_len: *mut u64, verdict: *mut c_void, wrong: *mut c_void,
                                     redundancy: *mut u64, radius: *mut u64, bad_batches: *mut u64,
                                     first_bad: *mut u64, undecoded: *mut u64, blame: *mut u64) -> SdaStatus;
    pub fn sda_recipient_job_decoded_dev(h: *mut SdaEngine, ms: *const SdaMaskingScheme, mask: *const i64,
                                         mask_len: u64, seed_bytes: *const u8, seed_off: *const u64, n_seeds: u64,
                                         ss: *const SdaSharingScheme, dimension: u64, indices: *const u64,
                                         clerk_bytes: *const u8, clerk_off: *const u64, n_idx: u64,
                                         output_modulus: i64, out: *mut i64, out_cap: u64, out_len: *mut u64,
                                         verdict: *mut c_void, wrong: *mut c_void, redundancy: *mut u64,
                                         radius: *mut u64, bad_batches: *mut u64, first_bad: *mut u64,
                                         undecoded: *mut u64, blame: *mut u64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_recipient_reveal_decoded_dev(h: *mut SdaEngine, ms: *const SdaMaskingScheme, mask_in: *const c_void,
                                            n_masks: u64, mask_width: u64, ss: *const SdaSharingScheme,
                                            dimension: u64, indices: *const u64, shares: *const i64, n_idx: u64,
                                            share_len: u64, output_modulus: i64, out: *mut i64, out_cap: u64,
                                            out_len: *mut u64, verdict: *mut c_void, wrong: *mut c_void,
                                            redundancy: *mut u64, radius: *mut u64, bad_batches: *mut u64,
                                            first_bad: *mut u64, undecoded: *mut u64, blame: *mut u64,
                                            stream: *mut c_void) -> SdaStatus;
    pub fn sda_recipient_decoded_last_launch(h: *mut SdaEngine, unmask_route: *mut u32, reveal_runs: *mut u32,
                                             compact: *mut u32) -> SdaStatus;

    // ---- participant job: mask, mask payload, shares and every clerk payload in one call ----
    pub fn sda_full_mask_keyed_dev(h: *mut SdaEngine, modulus: i64, secrets: *const i64, dimension: u64,
                                   key: *const u32, stream_id: u32, first: u64, masked_out: *mut i64,
                                   mask_out: *mut i64, stream: *mut c_void) -> SdaStatus;
    pub fn sda_full_mask_keyed32_dev(h: *mut SdaEngine, modulus: i64, secrets: *const i64, dimension: u64,
                                     key: *const u32, stream_id: u32, first: u64, masked_out: *mut i64,
                                     mask_out: *mut i32, stream: *mut c_void) -> SdaStatus;
    pub fn sda_participant_job_payload_bound(ms: *const SdaMaskingScheme, ss: *const SdaSharingScheme,
                                             dimension: u64, clerk_row_bound: *mut u64, mask_bound: *mut u64)
        -> SdaStatus;
    pub fn sda_participant_job_dev(h: *mut SdaEngine, ms: *const SdaMaskingScheme, seed: *const u32,
                                   seed_words: u64, ss: *const SdaSharingScheme, secrets: *const i64,
                                   dimension: u64, key: *const u32, mask_stream_id: u32, share_stream_id: u32,
                                   mode: i32, payload: *mut u8, payload_cap: u64, payload_row_bytes: *mut u64,
                                   mask_payload: *mut u8, mask_payload_cap: u64, mask_payload_len: *mut u64,
                                   stream: *mut c_void) -> SdaStatus;
    pub fn sda_participant_job(h: *mut SdaEngine, ms: *const SdaMaskingScheme, seed: *const u32, seed_words: u64,
                               ss: *const SdaSharingScheme, secrets: *const i64, dimension: u64, key: *const u32,
                               mask_stream_id: u32, share_stream_id: u32, mode: i32,
                               clerk_payloads: *const *mut u8, clerk_caps: *const u64, clerk_lens: *mut u64,
                               mask_payload: *mut u8, mask_cap: u64, mask_len: *mut u64) -> SdaStatus;
    pub fn sda_participant_job_last_launch(h: *mut SdaEngine, mask_route: *mut u32, share_route: *mut u32,
                                           share_bytes: *mut u32, tiles: *mut u64) -> SdaStatus;

    // ---- synthetic benchmark input ----
    pub fn sda_synth_fill_dev(h: *mut SdaEngine, dst: *mut i64, rows: u64, cols: u64, seed: u64, lo: i64, hi: i64,
                              stream: *mut c_void) -> SdaStatus;

    // ---- HBM for resident buffers (fixed-size physical chunks) ----
    pub fn sda_hbm_alloc(device: c_int, bytes: u64, out: *mut *mut c_void) -> SdaStatus;
    pub fn sda_hbm_free(ptr: *mut c_void) -> SdaStatus;
    pub fn sda_hbm_trim(device: c_int, keep_bytes: u64) -> SdaStatus;
    pub fn sda_hbm_stats(device: c_int, live_bytes: *mut u64, pooled_bytes: *mut u64, retired_bytes: *mut u64)
        -> SdaStatus;
}
