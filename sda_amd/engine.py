"""ctypes binding of libsda_engine.so (include/sda_engine.h).

This is the Python-side consumer of the C ABI: the parity tests and bench.py call the MI355X
engine only through it.  There is deliberately no CPU fallback: if the shared library is
missing or a call fails, an exception is raised.

Trait mirrors (reference: client/src/crypto/{sharing,masking}/mod.rs):
    share_generate     ShareGenerator::generate        (sharing/mod.rs:14-17)
    share_combine      ShareCombiner::combine          (sharing/mod.rs:23-25)
    secret_reconstruct SecretReconstructor::reconstruct (sharing/mod.rs:31-33)
    secret_mask        SecretMasker::mask              (masking/mod.rs:13-15)
    mask_combine       MaskCombiner::combine           (masking/mod.rs:21-23)
    secret_unmask      SecretUnmasker::unmask          (masking/mod.rs:29-31)
    positive           RecipientOutput::positive       (receive.rs:14-20)
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import sys
from typing import Optional, Sequence

import numpy as np

from . import schemes as S

# SDA_ENGINE_LIB: developer override (A/B builds of the same ABI); the default is the in-tree build.
LIB_PATH = os.environ.get("SDA_ENGINE_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsda_engine.so")

OK = 0
ERR_BATCH_INPUT_WRONG_LENGTH = 1
ERR_PACKED_SHARING_FAILED = 2
ERR_WRONG_DIMENSION = 3
ERR_MISMATCHING_DIMENSION = 4
ERR_INPUTS_MUST_HAVE_SAME_LENGTH = 5
ERR_NOT_ENOUGH_SHARES = 6
ERR_PRECONDITION = 64
ERR_INVALID_ARGUMENT = 65
ERR_UNSUPPORTED = 66
ERR_DEVICE = 67
ERR_OUT_OF_MEMORY = 68

REVEAL_EXACT = 0
REVEAL_CANONICAL = 1

# sda_chacha_last_launch's path codes
CHACHA_NONE = 0
CHACHA_DIRECT = 1
CHACHA_CHUNKED = 2
CHACHA_STREAM_K = 3
CHACHA_MASK_ADD = 4
CHACHA_STREAM = 5
CHACHA_OVERFLOW = 6

# sda_codec_last_launch's path codes and fell_back bits
CODEC_NONE = 0
CODEC_SLOTS = 1
CODEC_SLOTS_GROUPED = 2
CODEC_FUSED = 3
CODEC_FUSED_MULTI = 4
CODEC_MATRIX32 = 5
CODEC_MATRIX64 = 6
CODEC_FB_SLOT_WIDE = 1
CODEC_FB_FUSED_IRREGULAR = 2
CODEC_FB_NARROW_WIDE = 4
CODEC_FB_SEQUENTIAL = 8

# sda_combine_last_launch's kind codes and variant bits
COMBINE_NONE = 0
COMBINE_EXACT = 1
COMBINE_REPLAY = 2
COMBINE_SMALL_M = 1
COMBINE_ACC = 2
COMBINE_FLAG = 4
COMBINE_PIPE = 8
CombineLaunch = collections.namedtuple("CombineLaunch",
                                       "kind elem_bytes vec rows variant grid wlo nwide per_cu")

# sda_recipient_last_launch's mask_kind and reveal_mode codes
RECIPIENT_MASK_NONE_YET = 0
RECIPIENT_MASK_NONE = 1
RECIPIENT_MASK_FULL = 2
RECIPIENT_MASK_CHACHA = 3
RECIPIENT_MASK_COMBINED_ROW = 4
RECIPIENT_REVEAL_ADDITIVE = 0
RECIPIENT_REVEAL_EXACT = 1
RECIPIENT_REVEAL_CANONICAL = 2
RecipientLaunch = collections.namedtuple("RecipientLaunch", "mask_kind reveal_mode fell_back compact unmask_launches")

# sda_participant_last_launch's route codes
PARTICIPANT_MASK_NONE = 1
PARTICIPANT_MASK_FULL_ADD = 2
PARTICIPANT_MASK_CHACHA_FUSED = 3
PARTICIPANT_MASK_CHACHA_COMBINE_ADD = 4
PARTICIPANT_MASK_FULL_KEYED = 5
PARTICIPANT_SHARE_ADDITIVE = 1
PARTICIPANT_SHARE_ADDITIVE_KEYED = 2
PARTICIPANT_SHARE_PACKED = 3
PARTICIPANT_SHARE_PACKED_KEYED = 4
ParticipantLaunch = collections.namedtuple("ParticipantLaunch", "mask_route share_route passes")

# sda_recipient_job_last_launch's route codes
RECIPIENT_JOB_MASK_NONE = 0
RECIPIENT_JOB_MASK_FULL_COMBINED = 1
RECIPIENT_JOB_MASK_FULL_STREAMED = 2
RECIPIENT_JOB_MASK_CHACHA = 3
RECIPIENT_JOB_MASK_CHACHA_SPLIT = 4
RECIPIENT_JOB_SHARE_ADDITIVE = 1
RECIPIENT_JOB_SHARE_PACKED = 2
RecipientJobLaunch = collections.namedtuple("RecipientJobLaunch", "mask_route share_route seeds_decoded")

# sda_participant_job_last_launch's mask_route codes (share_route: the PARTICIPANT_SHARE_* codes)
PARTICIPANT_JOB_MASK_NONE = 0
PARTICIPANT_JOB_MASK_FULL64 = 1
PARTICIPANT_JOB_MASK_FULL32 = 2
PARTICIPANT_JOB_MASK_CHACHA = 3
ParticipantJobLaunch = collections.namedtuple("ParticipantJobLaunch", "mask_route share_route share_bytes tiles")

# Share consistency check (sda_packed_check_dev): a batch's verdict is 0 (consistent), the 1-based position of the one
# share that does not agree, or CHECK_UNLOCATED; sda_packed_check_last_launch's path codes
CHECK_UNLOCATED = 0xFFFF
CHECK_NO_BAD = (1 << 64) - 1
CHECK_PATH_REGISTERS = 1
CHECK_PATH_LOOPED = 2
ShareCheck = collections.namedtuple("ShareCheck", "redundancy bad_batches first_bad blame")
CheckLaunch = collections.namedtuple("CheckLaunch", "path bucket located overflowed")
# Checked reveal (sda_packed_reveal_checked_dev): sda_packed_reveal_checked_last_launch's path codes and record
REPAIR_PATH_FUSED = 1
REPAIR_PATH_COMPOSED = 2
RepairLaunch = collections.namedtuple("RepairLaunch", "path bucket fixed overflowed")

# Decoded reveal (sda_packed_reveal_decoded_dev): its counts, sda_packed_decode_last_launch's path codes and record
DECODE_PATH_FIRST_PASS = 1
DECODE_PATH_DECODED = 2
DECODE_UNDECODABLE = 0xFFFF
ShareDecode = collections.namedtuple("ShareDecode", "redundancy radius bad_batches first_bad undecoded blame")
DecodeLaunch = collections.namedtuple("DecodeLaunch", "path bucket decoded fixed max_errors overflowed")
# Robust recipient job (sda_recipient_job_decoded): sda_recipient_decoded_last_launch's unmask_route codes and record
RECIPIENT_UNMASK_NONE = 0
RECIPIENT_UNMASK_FUSED = 1
RECIPIENT_UNMASK_SEPARATE = 2
RecipientDecodedLaunch = collections.namedtuple("RecipientDecodedLaunch", "unmask_route reveal_runs compact")

# Elements one workgroup of the draws kernel produces (csrc/kernels.h kDrawsTile): the sizes at which
# sda_draws_dev's grid gains a workgroup
DRAWS_TILE = 2048

# Columns one workgroup of the fused Additive kernel owns (csrc/kernels.h kAdditiveKeyedTile): the dimensions at
# which sda_additive_generate_keyed_dev's grid gains a workgroup
ADDITIVE_KEYED_TILE = 512

_i64p = C.POINTER(C.c_int64)
_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)
_vp = C.c_void_p
_st = C.c_int

# (name, restype, argtypes) for every symbol declared in include/sda_engine.h
SIGNATURES = [
    ("sda_abi_version", C.c_int, []),
    ("sda_engine_create", _st, [C.c_int, C.POINTER(_vp)]),
    ("sda_engine_destroy", None, [_vp]),
    ("sda_engine_create_multi", _st, [C.POINTER(C.c_int), C.c_int, C.POINTER(_vp)]),
    ("sda_engine_device_count", C.c_int, [_vp]),
    ("sda_engine_synchronize", _st, [_vp]),
    ("sda_last_error_message", C.c_char_p, []),
    ("sda_status_string", C.c_char_p, [C.c_int]),
    ("sda_scheme_input_size", C.c_uint64, [C.POINTER(S.SharingSchemeC)]),
    ("sda_scheme_output_size", C.c_uint64, [C.POINTER(S.SharingSchemeC)]),
    ("sda_scheme_privacy_threshold", C.c_uint64, [C.POINTER(S.SharingSchemeC)]),
    ("sda_scheme_reconstruction_threshold", C.c_uint64, [C.POINTER(S.SharingSchemeC)]),
    ("sda_share_length", C.c_uint64, [C.POINTER(S.SharingSchemeC), C.c_uint64]),
    ("sda_share_generate", _st, [_vp, C.POINTER(S.SharingSchemeC), _i64p, C.c_uint64, _i64p, C.c_uint64,
                                 _i64p, C.c_uint64]),
    ("sda_share_combine", _st, [_vp, C.POINTER(S.SharingSchemeC), C.POINTER(_i64p), _u64p, C.c_uint64,
                                _i64p, C.c_uint64, _u64p]),
    ("sda_secret_reconstruct", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.POINTER(_i64p),
                                     _u64p, C.c_uint64, _i64p, C.c_uint64, _u64p]),
    ("sda_secret_mask", _st, [_vp, C.POINTER(S.MaskingSchemeC), _i64p, C.c_uint64, _u32p, C.c_uint64, _i64p,
                              _i64p, C.c_uint64, _u64p, _i64p]),
    ("sda_mask_combine", _st, [_vp, C.POINTER(S.MaskingSchemeC), C.POINTER(_i64p), _u64p, C.c_uint64, _i64p,
                               C.c_uint64, _u64p]),
    ("sda_secret_unmask", _st, [_vp, C.POINTER(S.MaskingSchemeC), _i64p, C.c_uint64, _i64p, C.c_uint64, _i64p,
                                C.c_uint64, _u64p]),
    ("sda_recipient_positive", _st, [_vp, C.c_int64, _i64p, C.c_uint64, _i64p]),
    ("sda_combine_dev", _st, [_vp, C.c_int64, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp]),
    ("sda_combine_finalize_dev", _st, [_vp, C.c_int64, _vp, C.c_uint64, _vp, _vp]),
    ("sda_combine_accumulate_dev", _st, [_vp, C.c_int64, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp]),
    ("sda_combine32_dev", _st, [_vp, C.c_int64, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp]),
    ("sda_combine32_accumulate_dev", _st, [_vp, C.c_int64, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp]),
    ("sda_narrow32_dev", _st, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _vp, _vp]),
    ("sda_host_stream_stats", _st, [_vp, _u64p, _u64p, _u64p]),
    ("sda_packed_fixup_count", _st, [_vp, _u64p]),
    ("sda_chacha_last_launch", _st, [_vp, _u32p, _u64p, _u64p]),
    ("sda_codec_last_launch", _st, [_vp, _u32p, _u32p, _u32p, _u64p]),
    ("sda_combine_last_launch", _st, [_vp, _u32p, _u32p, _u32p, _u32p, _u32p, _u64p, _u32p, _u32p, _u32p]),
    ("sda_snapshot_last_launch", _st, [_vp, _u64p, _u64p, _u64p, _u64p, _u32p]),
    ("sda_recipient_last_launch", _st, [_vp, _u32p, _u32p, _u32p, _u32p, _u32p]),
    ("sda_participant_last_launch", _st, [_vp, _u32p, _u32p, _u32p]),
    ("sda_combine_split_dev", _st, [_vp, C.c_int64, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp, _vp]),
    ("sda_combine_split_prefix_dev", _st, [_vp, C.c_int64, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp, _vp,
                                           _vp]),
    ("sda_combine_split_replay_dev", _st, [_vp, C.c_int64, _vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                           _vp, _vp, _vp]),
    ("sda_combine_split_resolve_dev", _st, [_vp, C.c_int64, _vp, _vp, C.c_uint64, _vp, _vp]),
    ("sda_packed_generate_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), _vp, C.c_uint64, C.c_uint64, _vp, _vp,
                                      _vp]),
    ("sda_packed_generate_mode_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), _vp, C.c_uint64, C.c_uint64, _vp,
                                           _vp, C.c_int32, _vp]),
    ("sda_packed_reconstruct_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.c_uint64,
                                         C.c_uint64, _vp, _vp, C.c_int32, _vp]),
    ("sda_packed_generate32_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), _vp, C.c_uint64, C.c_uint64, _vp,
                                        _vp, C.c_int32, _vp]),
    ("sda_packed_reconstruct32_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.c_uint64,
                                           C.c_uint64, _vp, _vp, C.c_int32, _vp]),
    ("sda_packed_check_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.c_uint64, C.c_uint64,
                                   _vp, _vp, _u64p, _u64p, _u64p, _u64p, _vp]),
    ("sda_packed_check32_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.c_uint64, C.c_uint64,
                                     _vp, _vp, _u64p, _u64p, _u64p, _u64p, _vp]),
    ("sda_secret_check", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.POINTER(_i64p), _u64p,
                               C.c_uint64, _vp, _u64p, _u64p, _u64p, _u64p]),
    ("sda_packed_check_last_launch", _st, [_vp, _u32p, _u32p, _u64p, _u32p]),
    ("sda_packed_reveal_checked_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.c_uint64,
                                            C.c_uint64, _vp, _vp, _vp, _u64p, _u64p, _u64p, _u64p, _vp]),
    ("sda_packed_reveal_checked32_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.c_uint64,
                                              C.c_uint64, _vp, _vp, _vp, _u64p, _u64p, _u64p, _u64p, _vp]),
    ("sda_secret_reconstruct_checked", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.POINTER(_i64p),
                                             _u64p, C.c_uint64, _vp, _u64p, _u64p, _u64p, _u64p, _i64p]),
    ("sda_packed_reveal_checked_last_launch", _st, [_vp, _u32p, _u32p, _u64p, _u32p]),
    ("sda_packed_reveal_decoded_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.c_uint64,
                                            C.c_uint64, _vp, _vp, _vp, _vp, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p,
                                            _vp]),
    ("sda_packed_reveal_decoded32_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.c_uint64,
                                              C.c_uint64, _vp, _vp, _vp, _vp, _u64p, _u64p, _u64p, _u64p, _u64p,
                                              _u64p, _vp]),
    ("sda_secret_reconstruct_decoded", _st, [_vp, C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.POINTER(_i64p),
                                             _u64p, C.c_uint64, _vp, _vp, _u64p, _u64p, _u64p, _u64p, _u64p, _u64p,
                                             _i64p]),
    ("sda_packed_decode_last_launch", _st, [_vp, _u32p, _u32p, _u64p, _u64p, _u32p, _u32p]),
    ("sda_additive_generate_dev", _st, [_vp, C.c_int64, C.c_uint64, _vp, C.c_uint64, _vp, _vp, _vp]),
    ("sda_chacha_mask_combine_dev", _st, [_vp, C.c_int64, C.c_uint64, _vp, C.c_uint64, C.c_uint64, _vp, _vp]),
    ("sda_draws_dev", _st, [_vp, _u32p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int64, _vp, _vp]),
    ("sda_draws", _st, [_vp, _u32p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int64, _i64p, C.c_uint64]),
    ("sda_share_generate_keyed", _st, [_vp, C.POINTER(S.SharingSchemeC), _i64p, C.c_uint64, _u32p, C.c_uint32,
                                       _i64p, C.c_uint64]),
    ("sda_secret_mask_keyed", _st, [_vp, C.POINTER(S.MaskingSchemeC), _i64p, C.c_uint64, _u32p, C.c_uint32, _i64p,
                                    C.c_uint64, _u64p, _i64p]),
    ("sda_synth_fill_dev", _st, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, _vp]),
    ("sda_hbm_alloc", _st, [C.c_int, C.c_uint64, C.POINTER(_vp)]),
    ("sda_hbm_free", _st, [_vp]),
    ("sda_hbm_trim", _st, [C.c_int, C.c_uint64]),
    ("sda_hbm_stats", _st, [C.c_int, _u64p, _u64p, _u64p]),
    ("sda_varint_encode", _st, [_vp, _i64p, C.c_uint64, _u8p, C.c_uint64, _u64p]),
    ("sda_varint_decode", _st, [_vp, _u8p, C.c_uint64, _i64p, C.c_uint64, _u64p]),
    ("sda_clerk_decode_combine", _st, [_vp, C.POINTER(S.SharingSchemeC), C.POINTER(_u8p), _u64p, C.c_uint64,
                                       _i64p, C.c_uint64, _u64p]),
    ("sda_varint_decode_dev", _st, [_vp, _vp, _u64p, C.c_uint64, _vp, C.c_uint64, _u64p, _vp]),
    ("sda_clerk_decode_combine_dev", _st, [_vp, C.c_int64, _vp, _u64p, C.c_uint64, _vp, C.c_uint64, _u64p, _vp]),
    ("sda_varint_encode_dev", _st, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _u64p, _vp]),
    ("sda_clerk_job_dev", _st, [_vp, C.c_int64, _vp, _u64p, C.c_uint64, C.c_uint64, C.c_uint64, _vp, C.c_uint64,
                                _u64p, _vp, C.c_uint64, _u64p, _vp]),
    ("sda_clerk_job", _st, [_vp, C.POINTER(S.SharingSchemeC), C.POINTER(_u8p), _u64p, C.c_uint64, _i64p, C.c_uint64,
                            _u64p, _u8p, C.c_uint64, _u64p]),
    ("sda_clerk_job_last_launch", _st, [_vp, _u32p, _u32p, _u64p]),
    ("sda_varint_encode32_dev", _st, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _u64p, _vp]),
    ("sda_snapshot_transpose_dev", _st, [_vp, _vp, _u64p, C.c_uint64, C.c_uint64, _vp, C.c_uint64, _u64p, _u64p,
                                         _u64p, _vp]),
    ("sda_recipient_reveal_dev", _st, [_vp, C.POINTER(S.MaskingSchemeC), _vp, C.c_uint64, C.c_uint64,
                                       C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, _vp, C.c_uint64, C.c_uint64,
                                       C.c_int64, C.c_int32, _vp, C.c_uint64, _u64p, _vp]),
    ("sda_recipient_reveal", _st, [_vp, C.POINTER(S.MaskingSchemeC), C.POINTER(_i64p), _u64p, C.c_uint64,
                                   C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.POINTER(_i64p), _u64p,
                                   C.c_uint64, C.c_int64, C.c_int32, _i64p, C.c_uint64, _u64p]),
    ("sda_recipient_job", _st, [_vp, C.POINTER(S.MaskingSchemeC), C.POINTER(_u8p), _u64p, C.c_uint64,
                                C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.POINTER(_u8p), _u64p, C.c_uint64,
                                C.c_int64, C.c_int32, _i64p, C.c_uint64, _u64p]),
    ("sda_recipient_job_dev", _st, [_vp, C.POINTER(S.MaskingSchemeC), _vp, C.c_uint64, _vp, _u64p, C.c_uint64,
                                    C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, _vp, _u64p, C.c_uint64,
                                    C.c_int64, C.c_int32, _vp, C.c_uint64, _u64p, _vp]),
    ("sda_recipient_job_last_launch", _st, [_vp, _u32p, _u32p, _u32p]),
    ("sda_recipient_job_decoded", _st, [_vp, C.POINTER(S.MaskingSchemeC), C.POINTER(_u8p), _u64p, C.c_uint64,
                                        C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, C.POINTER(_u8p), _u64p,
                                        C.c_uint64, C.c_int64, _i64p, C.c_uint64, _u64p, _vp, _vp, _u64p, _u64p,
                                        _u64p, _u64p, _u64p, _u64p]),
    ("sda_recipient_job_decoded_dev", _st, [_vp, C.POINTER(S.MaskingSchemeC), _vp, C.c_uint64, _vp, _u64p, C.c_uint64,
                                            C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, _vp, _u64p, C.c_uint64,
                                            C.c_int64, _vp, C.c_uint64, _u64p, _vp, _vp, _u64p, _u64p, _u64p, _u64p,
                                            _u64p, _u64p, _vp]),
    ("sda_recipient_reveal_decoded_dev", _st, [_vp, C.POINTER(S.MaskingSchemeC), _vp, C.c_uint64, C.c_uint64,
                                               C.POINTER(S.SharingSchemeC), C.c_uint64, _u64p, _vp, C.c_uint64,
                                               C.c_uint64, C.c_int64, _vp, C.c_uint64, _u64p, _vp, _vp, _u64p, _u64p,
                                               _u64p, _u64p, _u64p, _u64p, _vp]),
    ("sda_recipient_decoded_last_launch", _st, [_vp, _u32p, _u32p, _u32p]),
    ("sda_participant_share_dev", _st, [_vp, C.POINTER(S.MaskingSchemeC), _u32p, C.c_uint64, _vp,
                                        C.POINTER(S.SharingSchemeC), _vp, C.c_uint64, _vp, C.c_int32, _vp, _vp,
                                        C.c_uint64, _u64p, _vp]),
    ("sda_participant_share32_dev", _st, [_vp, C.POINTER(S.MaskingSchemeC), _u32p, C.c_uint64, _vp,
                                          C.POINTER(S.SharingSchemeC), _vp, C.c_uint64, _vp, C.c_int32, _vp, _vp,
                                          C.c_uint64, _u64p, _vp]),
    ("sda_additive_generate_keyed_dev", _st, [_vp, C.c_int64, C.c_uint64, _vp, C.c_uint64, _u32p, C.c_uint32,
                                              C.c_uint64, _vp, C.c_uint64, _vp]),
    ("sda_additive_generate_keyed32_dev", _st, [_vp, C.c_int64, C.c_uint64, _vp, C.c_uint64, _u32p, C.c_uint32,
                                                C.c_uint64, _vp, C.c_uint64, _vp]),
    ("sda_packed_generate_keyed_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), _vp, C.c_uint64, C.c_uint64, _u32p,
                                            C.c_uint32, C.c_uint64, _vp, C.c_int32, _vp]),
    ("sda_packed_generate_keyed32_dev", _st, [_vp, C.POINTER(S.SharingSchemeC), _vp, C.c_uint64, C.c_uint64, _u32p,
                                              C.c_uint32, C.c_uint64, _vp, C.c_int32, _vp]),
    ("sda_packed_keyed_last_launch", _st, [_vp, _u32p, _u64p]),
    ("sda_participant_share_keyed_dev", _st, [_vp, C.POINTER(S.MaskingSchemeC), _u32p, C.c_uint64, _vp,
                                              C.POINTER(S.SharingSchemeC), _vp, C.c_uint64, _u32p, C.c_uint32,
                                              C.c_int32, _vp, _vp, C.c_uint64, _u64p, _vp]),
    ("sda_participant_share32_keyed_dev", _st, [_vp, C.POINTER(S.MaskingSchemeC), _u32p, C.c_uint64, _vp,
                                                C.POINTER(S.SharingSchemeC), _vp, C.c_uint64, _u32p, C.c_uint32,
                                                C.c_int32, _vp, _vp, C.c_uint64, _u64p, _vp]),
    ("sda_full_mask_keyed_dev", _st, [_vp, C.c_int64, _vp, C.c_uint64, _u32p, C.c_uint32, C.c_uint64, _vp, _vp, _vp]),
    ("sda_full_mask_keyed32_dev", _st, [_vp, C.c_int64, _vp, C.c_uint64, _u32p, C.c_uint32, C.c_uint64, _vp, _vp,
                                        _vp]),
    ("sda_participant_job_payload_bound", _st, [C.POINTER(S.MaskingSchemeC), C.POINTER(S.SharingSchemeC), C.c_uint64,
                                                _u64p, _u64p]),
    ("sda_participant_job_dev", _st, [_vp, C.POINTER(S.MaskingSchemeC), _u32p, C.c_uint64,
                                      C.POINTER(S.SharingSchemeC), _vp, C.c_uint64, _u32p, C.c_uint32, C.c_uint32,
                                      C.c_int32, _vp, C.c_uint64, _u64p, _vp, C.c_uint64, _u64p, _vp]),
    ("sda_participant_job", _st, [_vp, C.POINTER(S.MaskingSchemeC), _u32p, C.c_uint64, C.POINTER(S.SharingSchemeC),
                                  _i64p, C.c_uint64, _u32p, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(_u8p),
                                  _u64p, _u64p, _u8p, C.c_uint64, _u64p]),
    ("sda_participant_job_last_launch", _st, [_vp, _u32p, _u32p, _u32p, _u64p]),
]

_libs = {}


def load_library(path: Optional[str] = None):
    """Load the in-tree engine library (or another build of it at `path`, for an in-process A/B of two builds);
    raises if it has not been built."""
    path = path or LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise RuntimeError(f"MI355X engine not built: {path} is missing (run `make` / __graft_entry__.build())")
        lib = C.CDLL(path)
        for name, res, args in SIGNATURES:
            if path != LIB_PATH and not hasattr(lib, name):
                continue                    # an older build in an A/B: it lacks the entry points added since
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _libs[path] = lib
    return _libs[path]


class SdaError(Exception):
    """A non-OK sda_status.  `.status` is the code; for 1..6 str(e) starts with the reference's string."""

    def __init__(self, status: int, message: str):
        self.status = status
        super().__init__(message)


def _check(st: int):
    if st != OK:
        lib = load_library()
        detail = lib.sda_last_error_message().decode()
        base = lib.sda_status_string(st).decode()
        raise SdaError(st, f"{base}: {detail}" if detail and detail != base else base)


def _arr(a, dtype=np.int64):
    return np.ascontiguousarray(np.asarray(a, dtype=dtype))


def _ptr(a, t=_i64p):
    return a.ctypes.data_as(t)


def _rows(rows):
    arrs = [_arr(r) for r in rows]
    n = len(arrs)
    ptrs = (_i64p * max(n, 1))(*[_ptr(a) for a in arrs])
    lens = (C.c_uint64 * max(n, 1))(*[a.size for a in arrs])
    return arrs, ptrs, lens, n


def participant_job_payload_bound(masking, sharing, dimension, lib_path: Optional[str] = None):
    """(clerk_row_bound, mask_bound): the most bytes one clerk's payload and the mask payload of a participant job
    over `dimension` secrets take (sda_participant_job_payload_bound).  Needs the library but no device."""
    ms, ss = masking.c(), sharing.c()
    row, mask = C.c_uint64(), C.c_uint64()
    _check(load_library(lib_path).sda_participant_job_payload_bound(C.byref(ms), C.byref(ss), dimension,
                                                                    C.byref(row), C.byref(mask)))
    return int(row.value), int(mask.value)


class _HbmBlock:
    """One sda_hbm_alloc buffer, exposed through __cuda_array_interface__ so torch.as_tensor wraps it
    without a copy; torch keeps this object alive as long as the tensor, and its release frees the buffer."""

    _TYPESTR = {"torch.int64": "<i8", "torch.int32": "<i4", "torch.uint8": "|u1", "torch.float64": "<f8",
                "torch.float32": "<f4"}

    def __init__(self, lib, device, shape, dtype, nbytes):
        typestr = self._TYPESTR.get(str(dtype))
        if typestr is None:
            raise ValueError(f"hbm_empty: unsupported dtype {dtype}")
        self.lib = lib
        p = _vp()
        _check(lib.sda_hbm_alloc(device, nbytes, C.byref(p)))
        self.ptr = p.value
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (self.ptr, False),
                                         "version": 2, "strides": None}

    def __del__(self):
        # sda_hbm_free does not wait for the device (the buffer is only pooled); at interpreter shutdown the
        # HIP runtime may already be gone, and the process exit releases everything anyway
        if getattr(self, "ptr", None) and not sys.is_finalizing():
            self.lib.sda_hbm_free(self.ptr)
        self.ptr = None


class Engine:
    """One engine handle = one HIP device + one stream (sda_engine_create), or, with `devices`, one handle over
    several devices (sda_engine_create_multi): the host trait calls then split over them; the `_dev` entry points
    run on devices[0].  `lib_path` names another build of the library than the in-tree one."""

    def __init__(self, device: int = 0, devices: Optional[Sequence[int]] = None, lib_path: Optional[str] = None):
        # torch (when the caller uses it) ships its own HIP runtime; it has to open the device before
        # the engine's ROCm runtime does, or torch later reports "No HIP GPUs are available"
        t = sys.modules.get("torch")
        if t is not None and t.cuda.is_available():
            t.cuda.init()
        self.lib = load_library(lib_path)
        h = _vp()
        if devices is None:
            _check(self.lib.sda_engine_create(device, C.byref(h)))
        else:
            devs = (C.c_int * max(len(devices), 1))(*devices)
            _check(self.lib.sda_engine_create_multi(devs, len(devices), C.byref(h)))
            device = int(devices[0])
        self.h = h
        self.device = device

    def device_count(self) -> int:
        """Devices the handle's host calls use (sda_engine_device_count)."""
        return int(self.lib.sda_engine_device_count(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.sda_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------- trait mirrors ----------------
    def share_generate(self, scheme, secrets, draws) -> np.ndarray:
        s = scheme.c()
        sec = _arr(secrets)
        dr = _arr(draws).reshape(-1)
        B = self.lib.sda_share_length(C.byref(s), sec.size)
        n = scheme.output_size()
        out = np.zeros(max(n * B, 1), np.int64)
        _check(self.lib.sda_share_generate(self.h, C.byref(s), _ptr(sec), sec.size, _ptr(dr), dr.size, _ptr(out),
                                           out.size))
        return out[: n * B].reshape(n, B)

    def share_combine(self, scheme, rows: Sequence) -> np.ndarray:
        s = scheme.c()
        arrs, ptrs, lens, n = _rows(rows)
        cap = arrs[0].size if arrs else 0
        out = np.zeros(max(cap, 1), np.int64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_share_combine(self.h, C.byref(s), ptrs, lens, n, _ptr(out), out.size, C.byref(olen)))
        return out[: olen.value]

    def secret_reconstruct(self, scheme, dimension: int, indexed_shares) -> np.ndarray:
        s = scheme.c()
        idx = _arr([i for i, _ in indexed_shares], np.uint64)
        arrs, ptrs, lens, n = _rows([r for _, r in indexed_shares])
        cap = max(dimension, arrs[0].size if arrs else 0, 1)
        out = np.zeros(cap, np.int64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_secret_reconstruct(self.h, C.byref(s), dimension, _ptr(idx, _u64p), ptrs, lens, n,
                                               _ptr(out), out.size, C.byref(olen)))
        return out[: olen.value]

    def secret_mask(self, scheme, secrets, seed: Optional[Sequence[int]] = None, full_masks=None):
        s = scheme.c()
        sec = _arr(secrets)
        sd = _arr(seed if seed is not None else [], np.uint32)
        fm = _arr(full_masks) if full_masks is not None else None
        mask = np.zeros(max(sec.size, sd.size, 1), np.int64)
        masked = np.zeros(max(sec.size, 1), np.int64)
        mlen = C.c_uint64(0)
        _check(self.lib.sda_secret_mask(self.h, C.byref(s), _ptr(sec), sec.size, _ptr(sd, _u32p), sd.size,
                                        _ptr(fm) if fm is not None else None, _ptr(mask), mask.size,
                                        C.byref(mlen), _ptr(masked)))
        return mask[: mlen.value], masked[: sec.size]

    # ---------------- device-side draws (one OS-RNG key per call, expanded on the device) ----------------
    @staticmethod
    def _key(key):
        k = _arr(key, np.uint32)
        if k.size != 8:
            raise ValueError("a draws key is 8 uint32 words")
        return k

    def draws_dev(self, key, stream_id, first, count, bound, out_ptr, stream=None):
        """out[p] = draw(first + p), p < count, uniform on [0, bound), into device memory (sda_draws_dev).  A
        (key, stream_id) pair must never serve two different jobs."""
        k = self._key(key)
        _check(self.lib.sda_draws_dev(self.h, _ptr(k, _u32p), stream_id, first, count, bound, out_ptr, stream))

    def draws(self, key, stream_id, first, count, bound) -> np.ndarray:
        """The same draws into host memory (sda_draws)."""
        k = self._key(key)
        out = np.zeros(max(count, 1), np.int64)
        _check(self.lib.sda_draws(self.h, _ptr(k, _u32p), stream_id, first, count, bound, _ptr(out), out.size))
        return out[:count]

    def share_generate_keyed(self, scheme, secrets, key, stream_id=0) -> np.ndarray:
        """share_generate with its draws made on the device from (key, stream_id) (sda_share_generate_keyed)."""
        s = scheme.c()
        sec = _arr(secrets)
        k = self._key(key)
        B = self.lib.sda_share_length(C.byref(s), sec.size)
        n = scheme.output_size()
        out = np.zeros(max(n * B, 1), np.int64)
        _check(self.lib.sda_share_generate_keyed(self.h, C.byref(s), _ptr(sec), sec.size, _ptr(k, _u32p), stream_id,
                                                 _ptr(out), out.size))
        return out[: n * B].reshape(n, B)

    def secret_mask_keyed(self, scheme, secrets, key, stream_id=0):
        """Full secret_mask with the mask drawn on the device from (key, stream_id) (sda_secret_mask_keyed);
        returns (mask, masked)."""
        s = scheme.c()
        sec = _arr(secrets)
        k = self._key(key)
        mask = np.zeros(max(sec.size, 1), np.int64)
        masked = np.zeros(max(sec.size, 1), np.int64)
        mlen = C.c_uint64(0)
        _check(self.lib.sda_secret_mask_keyed(self.h, C.byref(s), _ptr(sec), sec.size, _ptr(k, _u32p), stream_id,
                                              _ptr(mask), mask.size, C.byref(mlen), _ptr(masked)))
        return mask[: mlen.value], masked[: sec.size]

    def mask_combine(self, scheme, rows: Sequence) -> np.ndarray:
        s = scheme.c()
        arrs, ptrs, lens, n = _rows(rows)
        cap = max(getattr(scheme, "dimension", 0), arrs[0].size if arrs else 0, 1)
        out = np.zeros(cap, np.int64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_mask_combine(self.h, C.byref(s), ptrs, lens, n, _ptr(out), out.size, C.byref(olen)))
        return out[: olen.value]

    def secret_unmask(self, scheme, values) -> np.ndarray:
        s = scheme.c()
        mask, masked = _arr(values[0]), _arr(values[1])
        out = np.zeros(max(masked.size, 1), np.int64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_secret_unmask(self.h, C.byref(s), _ptr(mask), mask.size, _ptr(masked), masked.size,
                                          _ptr(out), out.size, C.byref(olen)))
        return out[: olen.value]

    def positive(self, modulus: int, values) -> np.ndarray:
        v = _arr(values)
        out = np.zeros(max(v.size, 1), np.int64)
        _check(self.lib.sda_recipient_positive(self.h, modulus, _ptr(v), v.size, _ptr(out)))
        return out[: v.size]

    # ---------------- share payload codec (sodium.rs:36-41 / :82-88) ----------------
    def varint_encode(self, values) -> bytes:
        v = _arr(values)
        out = (C.c_uint8 * max(10 * v.size, 1))()
        olen = C.c_uint64(0)
        _check(self.lib.sda_varint_encode(self.h, _ptr(v), v.size, out, len(out), C.byref(olen)))
        return bytes(out[: olen.value])

    def varint_decode(self, data: bytes) -> np.ndarray:
        src = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        out = np.zeros(max(len(data), 1), np.int64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_varint_decode(self.h, src, len(data), _ptr(out), out.size, C.byref(olen)))
        return out[: olen.value]

    def clerk_decode_combine_packed(self, scheme, payload: np.ndarray, blob_off) -> np.ndarray:
        """sda_clerk_decode_combine over blobs that sit back to back in one host uint8 array (blob i =
        payload[blob_off[i]:blob_off[i + 1]]), passed as pointers into it: no per-blob copy on the Python side."""
        s = scheme.c()
        pay = np.ascontiguousarray(payload, dtype=np.uint8)
        off = _arr(blob_off, np.uint64)
        n = off.size - 1
        base = pay.ctypes.data
        ptrs = (_u8p * max(n, 1))(*[C.cast(base + int(o), _u8p) for o in off[:-1]])
        lens = (C.c_uint64 * max(n, 1))(*[int(off[i + 1] - off[i]) for i in range(n)])
        cap = int(max(np.diff(off).max(initial=0), 1))
        out = np.zeros(cap, np.int64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_clerk_decode_combine(self.h, C.byref(s), ptrs, lens, n, _ptr(out), out.size, C.byref(olen)))
        return out[: olen.value]

    def clerk_decode_combine(self, scheme, blobs: Sequence[bytes]) -> np.ndarray:
        """clerk.rs:79-86 after the sealed-box opens: decode each participation, combine."""
        s = scheme.c()
        bufs = [(C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0") for b in blobs]
        n = len(bufs)
        ptrs = (_u8p * max(n, 1))(*[C.cast(b, _u8p) for b in bufs])
        lens = (C.c_uint64 * max(n, 1))(*[len(b) for b in blobs])
        cap = max([len(b) for b in blobs] + [1])
        out = np.zeros(cap, np.int64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_clerk_decode_combine(self.h, C.byref(s), ptrs, lens, n, _ptr(out), out.size,
                                                 C.byref(olen)))
        return out[: olen.value]

    def clerk_job(self, scheme, blobs: Sequence[bytes], want_out=True, payload_cap=None):
        """clerk.rs:63-107 between the sealed boxes, from host memory: decode each participation, combine, and
        encode the combined shares for the recipient.  Returns (out or None, payload bytes); payload_cap defaults
        to 10 bytes per byte of the longest blob.  A too-small payload_cap raises SdaError with `.payload_len`."""
        s = scheme.c()
        bufs = [(C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0") for b in blobs]
        n = len(bufs)
        ptrs = (_u8p * max(n, 1))(*[C.cast(b, _u8p) for b in bufs])
        lens = (C.c_uint64 * max(n, 1))(*[len(b) for b in blobs])
        cap = max([len(b) for b in blobs] + [1])
        out = np.zeros(cap, np.int64) if want_out else None
        pcap = 10 * cap if payload_cap is None else payload_cap
        pay = np.zeros(max(pcap, 1), np.uint8)
        olen, plen = C.c_uint64(0), C.c_uint64(0)
        try:
            _check(self.lib.sda_clerk_job(self.h, C.byref(s), ptrs, lens, n, _ptr(out) if want_out else None, cap,
                                          C.byref(olen), _ptr(pay, _u8p), pcap, C.byref(plen)))
        except SdaError as e:
            e.payload_len = int(plen.value)
            raise
        return (out[: olen.value] if want_out else None), pay[: plen.value].tobytes()

    # ---------------- fused role pipelines ----------------
    def recipient_reveal(self, masking, mask_rows, sharing, dimension: int, indexed_shares, output_modulus: int,
                         mode=REVEAL_EXACT) -> np.ndarray:
        """receive.rs:80-157 + positive() (:14-20) as one device pipeline."""
        ms, ss = masking.c(), sharing.c()
        marrs, mptrs, mlens, nm = _rows(mask_rows)
        idx = _arr([i for i, _ in indexed_shares], np.uint64)
        sarrs, sptrs, slens, ns = _rows([r for _, r in indexed_shares])
        cap = max(dimension, sarrs[0].size if sarrs else 0, 1)
        out = np.zeros(cap, np.int64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_recipient_reveal(self.h, C.byref(ms), mptrs, mlens, nm, C.byref(ss), dimension,
                                             _ptr(idx, _u64p), sptrs, slens, ns, output_modulus, mode, _ptr(out),
                                             out.size, C.byref(olen)))
        return out[: olen.value]

    @staticmethod
    def _blobs(blobs):
        bufs = [(C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0") for b in blobs]
        n = len(bufs)
        ptrs = (_u8p * max(n, 1))(*[C.cast(b, _u8p) for b in bufs])
        lens = (C.c_uint64 * max(n, 1))(*[len(b) for b in blobs])
        return bufs, ptrs, lens, n

    def recipient_job(self, masking, mask_blobs: Sequence[bytes], sharing, dimension: int, indexed_blobs,
                      output_modulus: int, mode=REVEAL_EXACT) -> np.ndarray:
        """recipient_reveal from the opened payloads: mask_blobs are the participations' mask payloads (Full masks or
        ChaCha seeds), indexed_blobs the (clerk index, opened clerk result) pairs; the engine decodes them."""
        ms, ss = masking.c(), sharing.c()
        mbufs, mptrs, mlens, nm = self._blobs(mask_blobs)
        idx = _arr([i for i, _ in indexed_blobs], np.uint64)
        sbufs, sptrs, slens, ns = self._blobs([b for _, b in indexed_blobs])
        cap = max(dimension, len(indexed_blobs[0][1]) if indexed_blobs else 0, 1)
        out = np.zeros(cap, np.int64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_recipient_job(self.h, C.byref(ms), mptrs, mlens, nm, C.byref(ss), dimension,
                                          _ptr(idx, _u64p), sptrs, slens, ns, output_modulus, mode, _ptr(out),
                                          out.size, C.byref(olen)))
        return out[: olen.value]

    def recipient_job_decoded(self, masking, mask_blobs: Sequence[bytes], sharing, dimension: int, indexed_blobs,
                              output_modulus: int, want_verdict=True, want_wrong=True):
        """recipient_job with the decoded reveal inside (sda_recipient_job_decoded): up to radius wrong clerk results
        per batch are corrected.  Returns (out, ShareDecode, verdict, wrong) as secret_reconstruct_decoded does, out
        being (secret - mask) mod p in [0, p)."""
        ms, ss = masking.c(), sharing.c()
        mbufs, mptrs, mlens, nm = self._blobs(mask_blobs)
        idx = _arr([i for i, _ in indexed_blobs], np.uint64)
        sbufs, sptrs, slens, ns = self._blobs([b for _, b in indexed_blobs])
        k = max(int(getattr(sharing, "secret_count", 1) or 1), 1)
        nb = (dimension + k - 1) // k
        verdict = np.full(max(nb, 1), 0xAAAA, np.uint16) if want_verdict else None
        wrong = np.full(max(nb, 1), 0xAAAAAAAA, np.uint32) if want_wrong else None
        out = np.zeros(max(dimension, 1), np.int64)
        olen = C.c_uint64(0)
        r, rad, bad, first, und = (C.c_uint64() for _ in range(5))
        blame = np.zeros(max(ns, 1), np.uint64)
        _check(self.lib.sda_recipient_job_decoded(self.h, C.byref(ms), mptrs, mlens, nm, C.byref(ss), dimension,
                                                  _ptr(idx, _u64p), sptrs, slens, ns, output_modulus, _ptr(out),
                                                  dimension, C.byref(olen),
                                                  verdict.ctypes.data if want_verdict else None,
                                                  wrong.ctypes.data if want_wrong else None, C.byref(r), C.byref(rad),
                                                  C.byref(bad), C.byref(first), C.byref(und), _ptr(blame, _u64p)))
        res = ShareDecode(int(r.value), int(rad.value), int(bad.value), int(first.value), int(und.value),
                          [int(x) for x in blame[:ns]])
        return (out[: olen.value], res, verdict[:nb] if want_verdict else None, wrong[:nb] if want_wrong else None)

    def recipient_decoded_last_launch(self):
        """RecipientDecodedLaunch(unmask_route, reveal_runs, compact) of the handle's last robust recipient call with
        a non-empty output (sda_recipient_decoded_last_launch): all zeros before the first."""
        route, runs, compact = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(self.lib.sda_recipient_decoded_last_launch(self.h, C.byref(route), C.byref(runs), C.byref(compact)))
        return RecipientDecodedLaunch(int(route.value), int(runs.value), int(compact.value))

    def synchronize(self):
        _check(self.lib.sda_engine_synchronize(self.h))

    def hbm_empty(self, shape, dtype=None):
        """An uninitialised torch tensor on this engine's device, in an sda_hbm_alloc buffer (fixed-size
        physical chunks, DESIGN.md "HBM backing"); the buffer is released when the tensor is."""
        import torch
        dtype = dtype or torch.int64
        shape = tuple(int(s) for s in shape)
        count = 1
        for s in shape:
            count *= s
        nbytes = max(count * torch.empty((), dtype=dtype).element_size(), 1)
        return torch.as_tensor(_HbmBlock(self.lib, self.device, shape, dtype, nbytes),
                               device=torch.device("cuda", self.device))

    def hbm_trim(self, keep_bytes: int = 0):
        """Release this device's pooled sda_hbm_alloc buffers down to keep_bytes (sda_hbm_trim)."""
        _check(self.lib.sda_hbm_trim(self.device, keep_bytes))

    def hbm_stats(self):
        """(live, pooled, retired) bytes of this device's sda_hbm_alloc buffers (sda_hbm_stats)."""
        v = [C.c_uint64() for _ in range(3)]
        _check(self.lib.sda_hbm_stats(self.device, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    # ---------------- device-resident entry points (raw device pointers, hipStream_t) ----------------
    def combine_dev(self, modulus, shares_ptr, n, dim, row_stride, out_ptr, stream=None):
        _check(self.lib.sda_combine_dev(self.h, modulus, shares_ptr, n, dim, row_stride, out_ptr, stream))

    def combine_accumulate_dev(self, modulus, shares_ptr, n, dim, row_stride, inout_ptr, stream=None):
        _check(self.lib.sda_combine_accumulate_dev(self.h, modulus, shares_ptr, n, dim, row_stride, inout_ptr,
                                                   stream))

    # int32 share rows (row_stride in int32 elements; i64 results, bit-identical to the widened rows)
    def combine32_dev(self, modulus, shares_ptr, n, dim, row_stride, out_ptr, stream=None):
        _check(self.lib.sda_combine32_dev(self.h, modulus, shares_ptr, n, dim, row_stride, out_ptr, stream))

    def combine32_accumulate_dev(self, modulus, shares_ptr, n, dim, row_stride, inout_ptr, stream=None):
        _check(self.lib.sda_combine32_accumulate_dev(self.h, modulus, shares_ptr, n, dim, row_stride, inout_ptr,
                                                     stream))

    def narrow32_dev(self, src_ptr, n, dim, src_stride, dst_ptr, dst_stride, flag_ptr, stream=None):
        """dst (int32) = src (i64) on the device; flag_ptr: device int64[1], zeroed by the caller, set to 1
        when a value does not fit (sda_narrow32_dev)."""
        _check(self.lib.sda_narrow32_dev(self.h, src_ptr, n, dim, src_stride, dst_ptr, dst_stride, flag_ptr, stream))

    def host_stream_stats(self):
        """(tiles_i32, tiles_i64, bytes_h2d) of the host rows' tile stream since the handle was created
        (sda_host_stream_stats)."""
        v = [C.c_uint64() for _ in range(3)]
        _check(self.lib.sda_host_stream_stats(self.h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def packed_fixup_count(self) -> int:
        """Batches the last packed generate / reconstruct launch sent to its generic fix-up kernel; 0 after a
        launch that logs nothing (workspace kernels, canonical Lagrange reveal) (sda_packed_fixup_count)."""
        v = C.c_uint64()
        _check(self.lib.sda_packed_fixup_count(self.h, C.byref(v)))
        return int(v.value)

    def chacha_last_launch(self):
        """(path, grid_y, fixups) of the handle's last ChaCha launch: path is one of the CHACHA_* codes, grid_y
        the chunks or the stream-K grid size, fixups the fix-up kernel launches (sda_chacha_last_launch)."""
        path, grid_y, fixups = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(self.lib.sda_chacha_last_launch(self.h, C.byref(path), C.byref(grid_y), C.byref(fixups)))
        return int(path.value), int(grid_y.value), int(fixups.value)

    def codec_last_launch(self):
        """(path, width, fell_back, passes) of the handle's last clerk_decode_combine_dev: path is one of the CODEC_*
        codes, width the slot combine's columns per lane or the fused kernel's prefetch depth, fell_back the
        CODEC_FB_* bits, passes the blob groups or grid slices (sda_codec_last_launch)."""
        path, width, fb, passes = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(self.lib.sda_codec_last_launch(self.h, C.byref(path), C.byref(width), C.byref(fb), C.byref(passes)))
        return int(path.value), int(width.value), int(fb.value), int(passes.value)

    def clerk_job_last_launch(self):
        """(continued, encode_route, encode_chunks) of the handle's last clerk_job_dev / clerk_job that launched
        something: encode_route 0 no payload, 1 the device-length encode queued before the call's wait, 2 the
        host-length encode after the counts were read (sda_clerk_job_last_launch)."""
        cont, route, chunks = C.c_uint32(), C.c_uint32(), C.c_uint64()
        _check(self.lib.sda_clerk_job_last_launch(self.h, C.byref(cont), C.byref(route), C.byref(chunks)))
        return int(cont.value), int(route.value), int(chunks.value)

    def combine_last_launch(self):
        """CombineLaunch(kind, elem_bytes, vec, rows, variant, grid, wlo, nwide, per_cu) of the handle's last
        share-combine launch: kind is one of the COMBINE_* codes, vec the columns per lane, rows the rows per batch,
        variant the COMBINE_SMALL_M / _ACC / _FLAG / _PIPE bits, (grid, wlo, nwide) the workgroups and the balanced
        grid's widths (0, 0 on the plain grid), per_cu the occupancy that grid was sized with
        (sda_combine_last_launch)."""
        v = [C.c_uint32() for _ in range(5)] + [C.c_uint64()] + [C.c_uint32() for _ in range(3)]
        _check(self.lib.sda_combine_last_launch(self.h, *[C.byref(x) for x in v]))
        return CombineLaunch(*[int(x.value) for x in v])

    def snapshot_last_launch(self):
        """(blobs, chunks, grid, chunk_bytes, shifts) of the handle's last snapshot_transpose_dev with a dst: the
        non-empty blobs planned, their chunks, the workgroups launched, the kernel's chunk size and the set of
        (src - dst) mod 16 the blobs had, bit s for shift s (sda_snapshot_last_launch)."""
        v = [C.c_uint64() for _ in range(4)] + [C.c_uint32()]
        _check(self.lib.sda_snapshot_last_launch(self.h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def recipient_last_launch(self):
        """RecipientLaunch(mask_kind, reveal_mode, fell_back, compact, unmask_launches) of the handle's last
        recipient_reveal / recipient_reveal_dev with a non-empty output: the RECIPIENT_MASK_* and RECIPIENT_REVEAL_*
        codes, whether a substituted canonical reveal fell back to the exact one, whether the clerk vectors were
        compacted, and the unmask launches (2 after a late ChaCha resolve) (sda_recipient_last_launch)."""
        v = [C.c_uint32() for _ in range(5)]
        _check(self.lib.sda_recipient_last_launch(self.h, *[C.byref(x) for x in v]))
        return RecipientLaunch(*[int(x.value) for x in v])

    def participant_last_launch(self):
        """ParticipantLaunch(mask_route, share_route, passes) of the handle's last participant_share*_dev of
        dimension > 0: the PARTICIPANT_MASK_* and PARTICIPANT_SHARE_* codes, and 2 passes when a rejecting ChaCha
        mask was redone (sda_participant_last_launch)."""
        v = [C.c_uint32() for _ in range(3)]
        _check(self.lib.sda_participant_last_launch(self.h, *[C.byref(x) for x in v]))
        return ParticipantLaunch(*[int(x.value) for x in v])

    def recipient_job_last_launch(self):
        """RecipientJobLaunch(mask_route, share_route, seeds_decoded) of the handle's last recipient_job /
        recipient_job_dev with a non-empty output: the RECIPIENT_JOB_MASK_* and RECIPIENT_JOB_SHARE_* codes and the
        seed blobs the seed kernel decoded (sda_recipient_job_last_launch)."""
        v = [C.c_uint32() for _ in range(3)]
        _check(self.lib.sda_recipient_job_last_launch(self.h, *[C.byref(x) for x in v]))
        return RecipientJobLaunch(*[int(x.value) for x in v])

    def participant_job_last_launch(self):
        """ParticipantJobLaunch(mask_route, share_route, share_bytes, tiles) of the handle's last participant_job /
        participant_job_dev of dimension > 0: the PARTICIPANT_JOB_MASK_* and PARTICIPANT_SHARE_* codes, the width of
        the share rows in handle scratch and the host form's tiles (sda_participant_job_last_launch)."""
        v = [C.c_uint32() for _ in range(3)]
        tiles = C.c_uint64()
        _check(self.lib.sda_participant_job_last_launch(self.h, *[C.byref(x) for x in v], C.byref(tiles)))
        return ParticipantJobLaunch(*[int(x.value) for x in v], int(tiles.value))

    @staticmethod
    def participant_job_payload_bound(masking, sharing, dimension):
        """The module's participant_job_payload_bound."""
        return participant_job_payload_bound(masking, sharing, dimension)

    def participant_job(self, masking, sharing, secrets, key, mask_stream_id, share_stream_id, seed=None,
                        mode=REVEAL_EXACT, clerk_caps=None, mask_cap=None):
        """The participant's whole job on host buffers (sda_participant_job): returns (clerk_payloads, mask_payload)
        as bytes -- what Encryptor::encrypt seals for each clerk and for the recipient.  clerk_caps / mask_cap
        override the capacities (default: the payload bound); a failing call raises SdaError carrying `.clerk_lens`
        and `.mask_len` as the call left them."""
        ms, ss = masking.c(), sharing.c()
        sec = _arr(secrets)
        sd = _arr(seed if seed is not None else [], np.uint32)
        k = self._key(key) if key is not None else None
        n = sharing.output_size()
        row, mb = self.participant_job_payload_bound(masking, sharing, sec.size)
        caps = _arr(clerk_caps if clerk_caps is not None else [row] * n, np.uint64)
        mcap = mb if mask_cap is None else mask_cap
        bufs = [np.zeros(max(int(c), 1), np.uint8) for c in caps]
        ptrs = (_u8p * max(n, 1))(*[_ptr(b, _u8p) for b in bufs])
        lens = np.zeros(max(n, 1), np.uint64)
        mbuf = np.zeros(max(mcap, 1), np.uint8)
        mlen = C.c_uint64(0)
        try:
            _check(self.lib.sda_participant_job(self.h, C.byref(ms), _ptr(sd, _u32p), sd.size, C.byref(ss), _ptr(sec),
                                                sec.size, _ptr(k, _u32p) if k is not None else None, mask_stream_id,
                                                share_stream_id, mode, ptrs, _ptr(caps, _u64p) if n else None,
                                                _ptr(lens, _u64p), _ptr(mbuf, _u8p), mcap, C.byref(mlen)))
        except SdaError as e:
            e.clerk_lens, e.mask_len = [int(x) for x in lens[:n]], int(mlen.value)
            raise
        return [bufs[c][: int(lens[c])].tobytes() for c in range(n)], mbuf[: mlen.value].tobytes()

    def packed_keyed_last_launch(self):
        """(path, staged_bytes) of the handle's last keyed packed-Shamir launch: path 0 none yet, 1 the draws were
        made in the share kernels, 2 staged in device scratch; staged_bytes the draw bytes that crossed HBM
        (sda_packed_keyed_last_launch)."""
        path, staged = C.c_uint32(), C.c_uint64()
        _check(self.lib.sda_packed_keyed_last_launch(self.h, C.byref(path), C.byref(staged)))
        return int(path.value), int(staged.value)

    def combine_finalize_dev(self, modulus, sums_ptr, dim, out_ptr, stream=None):
        _check(self.lib.sda_combine_finalize_dev(self.h, modulus, sums_ptr, dim, out_ptr, stream))

    # participation split of the combine (sda_amd.distributed; include/sda_engine.h "participation split")
    def combine_split_dev(self, modulus, shares_ptr, n, dim, row_stride, inout_ptr, flags_ptr, stream=None):
        _check(self.lib.sda_combine_split_dev(self.h, modulus, shares_ptr, n, dim, row_stride, inout_ptr, flags_ptr,
                                              stream))

    def combine_split_prefix_dev(self, modulus, gathered_ptr, world, rank, dim, c_in_ptr, total_ptr, code_ptr,
                                 stream=None):
        _check(self.lib.sda_combine_split_prefix_dev(self.h, modulus, gathered_ptr, world, rank, dim, c_in_ptr,
                                                     total_ptr, code_ptr, stream))

    def combine_split_replay_dev(self, modulus, shares_ptr, n, dim, row_stride, rank, state_ptr, code_ptr,
                                 stream=None):
        _check(self.lib.sda_combine_split_replay_dev(self.h, modulus, shares_ptr, n, dim, row_stride, rank,
                                                     state_ptr, code_ptr, stream))

    def combine_split_resolve_dev(self, modulus, total_ptr, code_ptr, dim, out_ptr, stream=None):
        _check(self.lib.sda_combine_split_resolve_dev(self.h, modulus, total_ptr, code_ptr, dim, out_ptr, stream))

    def packed_generate_dev(self, scheme, secrets_ptr, dimension, n_vectors, draws_ptr, out_ptr, stream=None):
        s = scheme.c()
        _check(self.lib.sda_packed_generate_dev(self.h, C.byref(s), secrets_ptr, dimension, n_vectors, draws_ptr,
                                                out_ptr, stream))

    def packed_generate_mode_dev(self, scheme, secrets_ptr, dimension, n_vectors, draws_ptr, out_ptr, mode,
                                 stream=None):
        s = scheme.c()
        _check(self.lib.sda_packed_generate_mode_dev(self.h, C.byref(s), secrets_ptr, dimension, n_vectors,
                                                     draws_ptr, out_ptr, mode, stream))

    def packed_reconstruct_dev(self, scheme, dimension, indices, n_vectors, shares_ptr, out_ptr,
                               mode=REVEAL_EXACT, stream=None):
        s = scheme.c()
        idx = _arr(indices, np.uint64)
        _check(self.lib.sda_packed_reconstruct_dev(self.h, C.byref(s), dimension, _ptr(idx, _u64p), idx.size,
                                                   n_vectors, shares_ptr, out_ptr, mode, stream))

    # int32 share rows: out / shares are device int32 [n_vectors][n][B]; the values are those of the i64 twins
    def packed_generate32_dev(self, scheme, secrets_ptr, dimension, n_vectors, draws_ptr, out_ptr, mode,
                              stream=None):
        s = scheme.c()
        _check(self.lib.sda_packed_generate32_dev(self.h, C.byref(s), secrets_ptr, dimension, n_vectors, draws_ptr,
                                                  out_ptr, mode, stream))

    def packed_reconstruct32_dev(self, scheme, dimension, indices, n_vectors, shares_ptr, out_ptr,
                                 mode=REVEAL_EXACT, stream=None):
        s = scheme.c()
        idx = _arr(indices, np.uint64)
        _check(self.lib.sda_packed_reconstruct32_dev(self.h, C.byref(s), dimension, _ptr(idx, _u64p), idx.size,
                                                     n_vectors, shares_ptr, out_ptr, mode, stream))

    # share consistency check of a reveal's input (include/sda_engine.h "share consistency check")
    def _packed_check(self, fn, scheme, dimension, indices, n_vectors, shares_ptr, verdict_ptr, stream):
        s = scheme.c()
        idx = _arr(indices, np.uint64)
        r, bad, first = C.c_uint64(), C.c_uint64(), C.c_uint64()
        blame = np.zeros(max(idx.size, 1), np.uint64)
        _check(fn(self.h, C.byref(s), dimension, _ptr(idx, _u64p), idx.size, n_vectors, shares_ptr, verdict_ptr,
                  C.byref(r), C.byref(bad), C.byref(first), _ptr(blame, _u64p), stream))
        return ShareCheck(int(r.value), int(bad.value), int(first.value), [int(x) for x in blame[: idx.size]])

    def packed_check_dev(self, scheme, dimension, indices, n_vectors, shares_ptr, verdict_ptr=None, stream=None):
        """Do the i64 shares [n_vectors][n_idx][B] a reveal would read agree?  Returns ShareCheck(redundancy,
        bad_batches, first_bad, blame); verdict_ptr: device uint16 [n_vectors][B] or None (sda_packed_check_dev).
        Waits for its stream."""
        return self._packed_check(self.lib.sda_packed_check_dev, scheme, dimension, indices, n_vectors, shares_ptr,
                                  verdict_ptr, stream)

    def packed_check32_dev(self, scheme, dimension, indices, n_vectors, shares_ptr, verdict_ptr=None, stream=None):
        """packed_check_dev over int32 shares (sda_packed_check32_dev)."""
        return self._packed_check(self.lib.sda_packed_check32_dev, scheme, dimension, indices, n_vectors, shares_ptr,
                                  verdict_ptr, stream)

    def secret_check(self, scheme, dimension: int, indexed_shares, want_verdict=True):
        """The check of host share rows, as secret_reconstruct takes them (sda_secret_check): (ShareCheck, verdict)
        with verdict a uint16 array of one entry per batch, or None."""
        s = scheme.c()
        idx = _arr([i for i, _ in indexed_shares], np.uint64)
        arrs, ptrs, lens, n = _rows([r for _, r in indexed_shares])
        k = max(int(getattr(scheme, "secret_count", 1) or 1), 1)
        nb = max((dimension + k - 1) // k, arrs[0].size if arrs else 0, 1)
        verdict = np.full(nb, 0xAAAA, np.uint16) if want_verdict else None
        r, bad, first = C.c_uint64(), C.c_uint64(), C.c_uint64()
        blame = np.zeros(max(n, 1), np.uint64)
        _check(self.lib.sda_secret_check(self.h, C.byref(s), dimension, _ptr(idx, _u64p), ptrs, lens, n,
                                         verdict.ctypes.data if want_verdict else None,
                                         C.byref(r), C.byref(bad), C.byref(first), _ptr(blame, _u64p)))
        res = ShareCheck(int(r.value), int(bad.value), int(first.value), [int(x) for x in blame[:n]])
        if not want_verdict:
            return res, None
        packed = getattr(s, "kind", 0) == 1
        return res, verdict[: (dimension + k - 1) // k if packed else (arrs[0].size if arrs else 0)]

    def packed_check_last_launch(self):
        """CheckLaunch(path, bucket, located, overflowed) of the handle's last share check that launched something
        (sda_packed_check_last_launch): all zeros before the first."""
        path, bucket, located, over = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
        _check(self.lib.sda_packed_check_last_launch(self.h, C.byref(path), C.byref(bucket), C.byref(located),
                                                     C.byref(over)))
        return CheckLaunch(int(path.value), int(bucket.value), int(located.value), int(over.value))

    # checked reveal (include/sda_engine.h "checked reveal"): the check's arguments plus out
    def _packed_reveal_checked(self, fn, scheme, dimension, indices, n_vectors, shares_ptr, out_ptr, verdict_ptr,
                               stream):
        s = scheme.c()
        idx = _arr(indices, np.uint64)
        r, bad, first = C.c_uint64(), C.c_uint64(), C.c_uint64()
        blame = np.zeros(max(idx.size, 1), np.uint64)
        _check(fn(self.h, C.byref(s), dimension, _ptr(idx, _u64p), idx.size, n_vectors, shares_ptr, out_ptr,
                  verdict_ptr, C.byref(r), C.byref(bad), C.byref(first), _ptr(blame, _u64p), stream))
        return ShareCheck(int(r.value), int(bad.value), int(first.value), [int(x) for x in blame[: idx.size]])

    def packed_reveal_checked_dev(self, scheme, dimension, indices, n_vectors, shares_ptr, out_ptr,
                                  verdict_ptr=None, stream=None):
        """The canonical reveal of i64 shares [n_vectors][n_idx][B] into out_ptr (device i64 [n_vectors][dimension])
        with the share check in the same pass and a located wrong share corrected; returns the check's ShareCheck
        (sda_packed_reveal_checked_dev).  Waits for its stream."""
        return self._packed_reveal_checked(self.lib.sda_packed_reveal_checked_dev, scheme, dimension, indices,
                                           n_vectors, shares_ptr, out_ptr, verdict_ptr, stream)

    def packed_reveal_checked32_dev(self, scheme, dimension, indices, n_vectors, shares_ptr, out_ptr,
                                    verdict_ptr=None, stream=None):
        """packed_reveal_checked_dev over int32 shares (sda_packed_reveal_checked32_dev)."""
        return self._packed_reveal_checked(self.lib.sda_packed_reveal_checked32_dev, scheme, dimension, indices,
                                           n_vectors, shares_ptr, out_ptr, verdict_ptr, stream)

    def secret_reconstruct_checked(self, scheme, dimension: int, indexed_shares, want_verdict=True):
        """The checked reveal of host share rows, as secret_check takes them (sda_secret_reconstruct_checked):
        (secrets, ShareCheck, verdict) with verdict a uint16 array of one entry per batch, or None."""
        s = scheme.c()
        idx = _arr([i for i, _ in indexed_shares], np.uint64)
        arrs, ptrs, lens, n = _rows([r for _, r in indexed_shares])
        k = max(int(getattr(scheme, "secret_count", 1) or 1), 1)
        nb = (dimension + k - 1) // k
        verdict = np.full(max(nb, 1), 0xAAAA, np.uint16) if want_verdict else None
        out = np.zeros(max(dimension, 1), np.int64)
        r, bad, first = C.c_uint64(), C.c_uint64(), C.c_uint64()
        blame = np.zeros(max(n, 1), np.uint64)
        _check(self.lib.sda_secret_reconstruct_checked(self.h, C.byref(s), dimension, _ptr(idx, _u64p), ptrs, lens, n,
                                                       verdict.ctypes.data if want_verdict else None, C.byref(r),
                                                       C.byref(bad), C.byref(first), _ptr(blame, _u64p), _ptr(out)))
        res = ShareCheck(int(r.value), int(bad.value), int(first.value), [int(x) for x in blame[:n]])
        return out[:dimension], res, verdict[:nb] if want_verdict else None

    def packed_reveal_checked_last_launch(self):
        """RepairLaunch(path, bucket, fixed, overflowed) of the handle's last checked reveal that launched something
        (sda_packed_reveal_checked_last_launch): all zeros before the first."""
        path, bucket, fixed, over = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
        _check(self.lib.sda_packed_reveal_checked_last_launch(self.h, C.byref(path), C.byref(bucket), C.byref(fixed),
                                                              C.byref(over)))
        return RepairLaunch(int(path.value), int(bucket.value), int(fixed.value), int(over.value))

    # decoded reveal (include/sda_engine.h "decoded reveal"): the checked reveal's arguments plus wrong
    def _packed_reveal_decoded(self, fn, scheme, dimension, indices, n_vectors, shares_ptr, out_ptr, verdict_ptr,
                               wrong_ptr, stream):
        s = scheme.c()
        idx = _arr(indices, np.uint64)
        r, rad, bad, first, und = (C.c_uint64() for _ in range(5))
        blame = np.zeros(max(idx.size, 1), np.uint64)
        _check(fn(self.h, C.byref(s), dimension, _ptr(idx, _u64p), idx.size, n_vectors, shares_ptr, out_ptr,
                  verdict_ptr, wrong_ptr, C.byref(r), C.byref(rad), C.byref(bad), C.byref(first), C.byref(und),
                  _ptr(blame, _u64p), stream))
        return ShareDecode(int(r.value), int(rad.value), int(bad.value), int(first.value), int(und.value),
                           [int(x) for x in blame[: idx.size]])

    def packed_reveal_decoded_dev(self, scheme, dimension, indices, n_vectors, shares_ptr, out_ptr,
                                  verdict_ptr=None, wrong_ptr=None, stream=None):
        """The canonical reveal of i64 shares [n_vectors][n_idx][B] into out_ptr (device i64 [n_vectors][dimension])
        with up to radius = redundancy // 2 wrong shares per batch corrected; verdict_ptr: device uint16
        [n_vectors][B] (|E|, 0xFFFF undecodable) or None; wrong_ptr: device uint32 [n_vectors][B] (the bits of E) or
        None.  Returns ShareDecode(redundancy, radius, bad_batches, first_bad, undecoded, blame)
        (sda_packed_reveal_decoded_dev).  Waits for its stream."""
        return self._packed_reveal_decoded(self.lib.sda_packed_reveal_decoded_dev, scheme, dimension, indices,
                                           n_vectors, shares_ptr, out_ptr, verdict_ptr, wrong_ptr, stream)

    def packed_reveal_decoded32_dev(self, scheme, dimension, indices, n_vectors, shares_ptr, out_ptr,
                                    verdict_ptr=None, wrong_ptr=None, stream=None):
        """packed_reveal_decoded_dev over int32 shares (sda_packed_reveal_decoded32_dev)."""
        return self._packed_reveal_decoded(self.lib.sda_packed_reveal_decoded32_dev, scheme, dimension, indices,
                                           n_vectors, shares_ptr, out_ptr, verdict_ptr, wrong_ptr, stream)

    def secret_reconstruct_decoded(self, scheme, dimension: int, indexed_shares, want_verdict=True, want_wrong=True):
        """The decoded reveal of host share rows, as secret_reconstruct_checked takes them
        (sda_secret_reconstruct_decoded): (secrets, ShareDecode, verdict, wrong) with verdict a uint16 and wrong a
        uint32 array of one entry per batch, or None."""
        s = scheme.c()
        idx = _arr([i for i, _ in indexed_shares], np.uint64)
        arrs, ptrs, lens, n = _rows([r for _, r in indexed_shares])
        k = max(int(getattr(scheme, "secret_count", 1) or 1), 1)
        nb = (dimension + k - 1) // k
        verdict = np.full(max(nb, 1), 0xAAAA, np.uint16) if want_verdict else None
        wrong = np.full(max(nb, 1), 0xAAAAAAAA, np.uint32) if want_wrong else None
        out = np.zeros(max(dimension, 1), np.int64)
        r, rad, bad, first, und = (C.c_uint64() for _ in range(5))
        blame = np.zeros(max(n, 1), np.uint64)
        _check(self.lib.sda_secret_reconstruct_decoded(self.h, C.byref(s), dimension, _ptr(idx, _u64p), ptrs, lens, n,
                                                       verdict.ctypes.data if want_verdict else None,
                                                       wrong.ctypes.data if want_wrong else None, C.byref(r),
                                                       C.byref(rad), C.byref(bad), C.byref(first), C.byref(und),
                                                       _ptr(blame, _u64p), _ptr(out)))
        res = ShareDecode(int(r.value), int(rad.value), int(bad.value), int(first.value), int(und.value),
                          [int(x) for x in blame[:n]])
        return (out[:dimension], res, verdict[:nb] if want_verdict else None, wrong[:nb] if want_wrong else None)

    def packed_decode_last_launch(self):
        """DecodeLaunch(path, bucket, decoded, fixed, max_errors, overflowed) of the handle's last decoded reveal that
        launched something (sda_packed_decode_last_launch): all zeros before the first."""
        path, bucket, over, mx = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        decoded, fixed = C.c_uint64(), C.c_uint64()
        _check(self.lib.sda_packed_decode_last_launch(self.h, C.byref(path), C.byref(bucket), C.byref(decoded),
                                                      C.byref(fixed), C.byref(mx), C.byref(over)))
        return DecodeLaunch(int(path.value), int(bucket.value), int(decoded.value), int(fixed.value), int(mx.value),
                            int(over.value))

    def packed_generate_keyed_dev(self, scheme, secrets_ptr, dimension, n_vectors, key, stream_id, out_ptr, mode,
                                  first_batch=0, stream=None):
        """packed_generate_mode_dev with the draws made on the device (sda_packed_generate_keyed_dev): batch b of
        vector v takes draws (first_batch + v B + b) t + j of (key, stream_id) at bound p - 1.  key=None passes a
        NULL key (the status tests)."""
        s = scheme.c()
        k = self._key(key) if key is not None else None
        _check(self.lib.sda_packed_generate_keyed_dev(self.h, C.byref(s), secrets_ptr, dimension, n_vectors,
                                                      _ptr(k, _u32p) if k is not None else None, stream_id,
                                                      first_batch, out_ptr, mode, stream))

    def packed_generate_keyed32_dev(self, scheme, secrets_ptr, dimension, n_vectors, key, stream_id, out_ptr, mode,
                                    first_batch=0, stream=None):
        """packed_generate_keyed_dev with out as device int32 [n_vectors][n][B]."""
        s = scheme.c()
        k = self._key(key) if key is not None else None
        _check(self.lib.sda_packed_generate_keyed32_dev(self.h, C.byref(s), secrets_ptr, dimension, n_vectors,
                                                        _ptr(k, _u32p) if k is not None else None, stream_id,
                                                        first_batch, out_ptr, mode, stream))

    def additive_generate_dev(self, modulus, share_count, secrets_ptr, dimension, draws_ptr, out_ptr, stream=None):
        _check(self.lib.sda_additive_generate_dev(self.h, modulus, share_count, secrets_ptr, dimension, draws_ptr,
                                                  out_ptr, stream))

    def additive_generate_keyed_dev(self, modulus, share_count, secrets_ptr, dimension, key, stream_id, out_ptr,
                                    out_stride, first_column=0, stream=None):
        """Additive shares with the draws made inside the kernel (sda_additive_generate_keyed_dev): column d takes
        draws (first_column + d) * (share_count - 1) + j of (key, stream_id); out is device i64, rows out_stride
        apart.  key=None passes a NULL key (the status tests)."""
        k = self._key(key) if key is not None else None
        _check(self.lib.sda_additive_generate_keyed_dev(self.h, modulus, share_count, secrets_ptr, dimension,
                                                        _ptr(k, _u32p) if k is not None else None, stream_id,
                                                        first_column, out_ptr, out_stride, stream))

    def additive_generate_keyed32_dev(self, modulus, share_count, secrets_ptr, dimension, key, stream_id, out_ptr,
                                      out_stride, first_column=0, stream=None):
        """additive_generate_keyed_dev with out as device int32 rows (modulus <= 2^31)."""
        k = self._key(key) if key is not None else None
        _check(self.lib.sda_additive_generate_keyed32_dev(self.h, modulus, share_count, secrets_ptr, dimension,
                                                          _ptr(k, _u32p) if k is not None else None, stream_id,
                                                          first_column, out_ptr, out_stride, stream))

    def full_mask_keyed_dev(self, modulus, secrets_ptr, dimension, key, stream_id, masked_ptr, mask_ptr, first=0,
                            mask32=False, stream=None):
        """Full masking with the mask drawn in the kernel (sda_full_mask_keyed_dev): mask[d] = draw(first + d) of
        (key, stream_id) at bound = modulus, masked[d] = (secrets[d] + mask[d]) % modulus; all device pointers, the
        mask as int32 values with mask32 (modulus <= 2^31).  key=None passes a NULL key (the status tests)."""
        k = self._key(key) if key is not None else None
        fn = self.lib.sda_full_mask_keyed32_dev if mask32 else self.lib.sda_full_mask_keyed_dev
        _check(fn(self.h, modulus, secrets_ptr, dimension, _ptr(k, _u32p) if k is not None else None, stream_id,
                  first, masked_ptr, mask_ptr, stream))

    def participant_job_dev(self, masking, sharing, secrets_ptr, dimension, key, mask_stream_id, share_stream_id,
                            payload_ptr, payload_cap, mask_payload_ptr, mask_payload_cap, seed=None,
                            mode=REVEAL_EXACT, stream=None):
        """The participant's whole job on device buffers (sda_participant_job_dev); returns (payload_row_bytes [n],
        mask_payload_len).  A failing call raises SdaError carrying `.row_bytes` and `.mask_len` as the call left
        them.  key=None passes a NULL key (the status tests)."""
        ms, ss = masking.c(), sharing.c()
        sd = _arr(seed if seed is not None else [], np.uint32)
        k = self._key(key) if key is not None else None
        n = sharing.output_size()
        rb = np.zeros(max(n, 1), np.uint64)
        mlen = C.c_uint64(0)
        try:
            _check(self.lib.sda_participant_job_dev(self.h, C.byref(ms), _ptr(sd, _u32p), sd.size, C.byref(ss),
                                                    secrets_ptr, dimension, _ptr(k, _u32p) if k is not None else None,
                                                    mask_stream_id, share_stream_id, mode, payload_ptr, payload_cap,
                                                    _ptr(rb, _u64p), mask_payload_ptr, mask_payload_cap,
                                                    C.byref(mlen), stream))
        except SdaError as e:
            e.row_bytes, e.mask_len = rb[:n].copy(), int(mlen.value)
            raise
        return rb[:n], int(mlen.value)

    def chacha_mask_combine_dev(self, modulus, dimension, seeds_ptr, w, n_seeds, out_ptr, stream=None):
        _check(self.lib.sda_chacha_mask_combine_dev(self.h, modulus, dimension, seeds_ptr, w, n_seeds, out_ptr,
                                                    stream))

    def synth_fill_dev(self, dst_ptr, rows, cols, seed, lo, hi, stream=None):
        _check(self.lib.sda_synth_fill_dev(self.h, dst_ptr, rows, cols, seed, lo, hi, stream))

    def varint_decode_dev(self, bytes_ptr, blob_off, out_ptr, out_stride, stream=None) -> np.ndarray:
        off = _arr(blob_off, np.uint64)
        n = off.size - 1
        counts = np.zeros(max(n, 1), np.uint64)
        _check(self.lib.sda_varint_decode_dev(self.h, bytes_ptr, _ptr(off, _u64p), n, out_ptr, out_stride,
                                              _ptr(counts, _u64p), stream))
        return counts[:n]

    def clerk_decode_combine_dev(self, modulus, bytes_ptr, blob_off, out_ptr, out_cap, stream=None) -> int:
        off = _arr(blob_off, np.uint64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_clerk_decode_combine_dev(self.h, modulus, bytes_ptr, _ptr(off, _u64p), off.size - 1,
                                                     out_ptr, out_cap, C.byref(olen), stream))
        return olen.value

    def clerk_job_dev(self, modulus, bytes_ptr, blob_off, state_ptr, state_cap, first_participation=0, prior_dim=0,
                      payload_ptr=None, payload_cap=0, stream=None):
        """The clerk's decode -> combine -> payload as one call, continued from the state of participations
        [0, first_participation) over prior_dim columns when first_participation > 0; blob_off empty or [0] with a
        payload is the finish call.  Returns (dim, payload_len); payload_ptr None: an intermediate tile, no encode.
        A failing call raises SdaError carrying `.dim` and `.payload_len` as the call left them."""
        off = _arr(blob_off if len(blob_off) else [0], np.uint64)
        dim, plen = C.c_uint64(0), C.c_uint64(0)
        try:
            _check(self.lib.sda_clerk_job_dev(self.h, modulus, bytes_ptr, _ptr(off, _u64p), off.size - 1,
                                              first_participation, prior_dim, state_ptr, state_cap, C.byref(dim),
                                              payload_ptr, payload_cap, C.byref(plen), stream))
        except SdaError as e:
            e.dim, e.payload_len = int(dim.value), int(plen.value)
            raise
        return int(dim.value), int(plen.value)

    def varint_encode_dev(self, vals_ptr, rows, length, stride, dst_ptr, dst_cap, stream=None) -> np.ndarray:
        rb = np.zeros(max(rows, 1), np.uint64)
        _check(self.lib.sda_varint_encode_dev(self.h, vals_ptr, rows, length, stride, dst_ptr, dst_cap,
                                              _ptr(rb, _u64p), stream))
        return rb[:rows]

    def varint_encode32_dev(self, vals_ptr, rows, length, stride, dst_ptr, dst_cap, stream=None) -> np.ndarray:
        """varint_encode_dev from int32 rows (stride in int32 elements): the bytes of the sign-extended rows."""
        rb = np.zeros(max(rows, 1), np.uint64)
        _check(self.lib.sda_varint_encode32_dev(self.h, vals_ptr, rows, length, stride, dst_ptr, dst_cap,
                                                _ptr(rb, _u64p), stream))
        return rb[:rows]

    def snapshot_transpose_dev(self, src_ptr, part_off, n_participations, n_clerks, dst_ptr=None, dst_cap=0,
                               stream=None):
        """AggregationsStore::iter_snapshot_clerk_jobs_data (server/src/stores.rs:86-101) on device.

        part_off: [P*n + 1] offsets of the [participation][clerk] blobs in src.  Returns
        (dst_len, clerk_base [n], clerk_off [n][P+1]); dst_ptr None = sizing query."""
        off = _arr(part_off, np.uint64)
        P, n = n_participations, n_clerks
        if off.size != P * n + 1:
            raise ValueError("part_off must have n_participations * n_clerks + 1 entries")
        base = np.zeros(max(n, 1), np.uint64)
        coff = np.zeros(max(n * (P + 1), 1), np.uint64)
        dlen = C.c_uint64(0)
        _check(self.lib.sda_snapshot_transpose_dev(self.h, src_ptr, _ptr(off, _u64p), P, n, dst_ptr, dst_cap,
                                                   C.byref(dlen), _ptr(base, _u64p), _ptr(coff, _u64p), stream))
        return dlen.value, base[:n], coff[:n * (P + 1)].reshape(n, P + 1)

    def recipient_reveal_dev(self, masking, mask_ptr, n_masks, mask_width, sharing, dimension, indices, shares_ptr,
                             share_len, output_modulus, out_ptr, out_cap, mode=REVEAL_EXACT, stream=None) -> int:
        ms, ss = masking.c(), sharing.c()
        idx = _arr(indices, np.uint64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_recipient_reveal_dev(self.h, C.byref(ms), mask_ptr, n_masks, mask_width, C.byref(ss),
                                                 dimension, _ptr(idx, _u64p), shares_ptr, idx.size, share_len,
                                                 output_modulus, mode, out_ptr, out_cap, C.byref(olen), stream))
        return olen.value

    def recipient_job_dev(self, masking, sharing, dimension, indices, clerk_ptr, clerk_off, output_modulus, out_ptr,
                          out_cap, mask_ptr=None, mask_len=0, seed_ptr=None, seed_off=(), mode=REVEAL_EXACT,
                          stream=None) -> int:
        """recipient_reveal_dev from the opened payloads on the device: (clerk_ptr, clerk_off) and, for ChaCha
        masking, (seed_ptr, seed_off) are (bytes, offsets) pairs as clerk_decode_combine_dev takes them; for Full
        masking (mask_ptr, mask_len) is the combined mask, e.g. the state clerk_job_dev left over the mask payloads."""
        ms, ss = masking.c(), sharing.c()
        idx = _arr(indices, np.uint64)
        coff = _arr(clerk_off if len(clerk_off) else [0], np.uint64)
        soff = _arr(seed_off if len(seed_off) else [0], np.uint64)
        olen = C.c_uint64(0)
        _check(self.lib.sda_recipient_job_dev(self.h, C.byref(ms), mask_ptr, mask_len, seed_ptr, _ptr(soff, _u64p),
                                              soff.size - 1, C.byref(ss), dimension, _ptr(idx, _u64p), clerk_ptr,
                                              _ptr(coff, _u64p), coff.size - 1, output_modulus, mode, out_ptr,
                                              out_cap, C.byref(olen), stream))
        return olen.value

    def _decoded_counts(self, n_idx):
        cs = [C.c_uint64() for _ in range(5)]
        blame = np.zeros(max(n_idx, 1), np.uint64)
        done = lambda: ShareDecode(*[int(c.value) for c in cs], [int(x) for x in blame[:n_idx]])
        return [C.byref(c) for c in cs] + [_ptr(blame, _u64p)], done

    def recipient_reveal_decoded_dev(self, masking, mask_ptr, n_masks, mask_width, sharing, dimension, indices,
                                     shares_ptr, share_len, output_modulus, out_ptr, out_cap, verdict_ptr=None,
                                     wrong_ptr=None, stream=None):
        """recipient_reveal_dev with the decoded reveal inside (sda_recipient_reveal_decoded_dev): verdict_ptr device
        uint16 [B] or None, wrong_ptr device uint32 [B] or None.  Returns (out_len, ShareDecode).  Waits for its
        stream."""
        ms, ss = masking.c(), sharing.c()
        idx = _arr(indices, np.uint64)
        olen = C.c_uint64(0)
        counts, done = self._decoded_counts(idx.size)
        _check(self.lib.sda_recipient_reveal_decoded_dev(self.h, C.byref(ms), mask_ptr, n_masks, mask_width,
                                                         C.byref(ss), dimension, _ptr(idx, _u64p), shares_ptr,
                                                         idx.size, share_len, output_modulus, out_ptr, out_cap,
                                                         C.byref(olen), verdict_ptr, wrong_ptr, *counts, stream))
        return olen.value, done()

    def recipient_job_decoded_dev(self, masking, sharing, dimension, indices, clerk_ptr, clerk_off, output_modulus,
                                  out_ptr, out_cap, mask_ptr=None, mask_len=0, seed_ptr=None, seed_off=(),
                                  verdict_ptr=None, wrong_ptr=None, stream=None):
        """recipient_job_dev with the decoded reveal inside (sda_recipient_job_decoded_dev); the inputs as
        recipient_job_dev takes them, verdict_ptr / wrong_ptr as recipient_reveal_decoded_dev.  Returns
        (out_len, ShareDecode).  Waits for its stream."""
        ms, ss = masking.c(), sharing.c()
        idx = _arr(indices, np.uint64)
        coff = _arr(clerk_off if len(clerk_off) else [0], np.uint64)
        soff = _arr(seed_off if len(seed_off) else [0], np.uint64)
        olen = C.c_uint64(0)
        counts, done = self._decoded_counts(idx.size)
        _check(self.lib.sda_recipient_job_decoded_dev(self.h, C.byref(ms), mask_ptr, mask_len, seed_ptr,
                                                      _ptr(soff, _u64p), soff.size - 1, C.byref(ss), dimension,
                                                      _ptr(idx, _u64p), clerk_ptr, _ptr(coff, _u64p), coff.size - 1,
                                                      output_modulus, out_ptr, out_cap, C.byref(olen), verdict_ptr,
                                                      wrong_ptr, *counts, stream))
        return olen.value, done()

    def participant_share_dev(self, masking, sharing, secrets_ptr, dimension, draws_ptr, shares_ptr, seed=None,
                              full_masks_ptr=None, payload_ptr=None, payload_cap=0, mode=REVEAL_EXACT, stream=None):
        """participate.rs:53-76 (+ payload encoding) on device; returns per-clerk payload byte counts."""
        ms, ss = masking.c(), sharing.c()
        sd = _arr(seed if seed is not None else [], np.uint32)
        n = sharing.output_size()
        rb = np.zeros(max(n, 1), np.uint64)
        _check(self.lib.sda_participant_share_dev(self.h, C.byref(ms), _ptr(sd, _u32p), sd.size, full_masks_ptr,
                                                  C.byref(ss), secrets_ptr, dimension, draws_ptr, mode, shares_ptr,
                                                  payload_ptr, payload_cap, _ptr(rb, _u64p), stream))
        return rb[:n]

    def participant_share32_dev(self, masking, sharing, secrets_ptr, dimension, draws_ptr, shares_ptr, seed=None,
                                full_masks_ptr=None, payload_ptr=None, payload_cap=0, mode=REVEAL_EXACT,
                                stream=None):
        """participant_share_dev with shares_ptr as device int32 [n][B] (PackedShamir only) and the payload from
        the int32 encoder; returns per-clerk payload byte counts."""
        ms, ss = masking.c(), sharing.c()
        sd = _arr(seed if seed is not None else [], np.uint32)
        n = sharing.output_size()
        rb = np.zeros(max(n, 1), np.uint64)
        _check(self.lib.sda_participant_share32_dev(self.h, C.byref(ms), _ptr(sd, _u32p), sd.size, full_masks_ptr,
                                                    C.byref(ss), secrets_ptr, dimension, draws_ptr, mode,
                                                    shares_ptr, payload_ptr, payload_cap, _ptr(rb, _u64p), stream))
        return rb[:n]

    def participant_share_keyed_dev(self, masking, sharing, secrets_ptr, dimension, key, stream_id, shares_ptr,
                                    seed=None, full_masks_ptr=None, payload_ptr=None, payload_cap=0,
                                    mode=REVEAL_EXACT, stream=None):
        """participant_share_dev with the share-generation draws made on the device from (key, stream_id)
        (sda_participant_share_keyed_dev); returns per-clerk payload byte counts."""
        ms, ss = masking.c(), sharing.c()
        sd = _arr(seed if seed is not None else [], np.uint32)
        k = self._key(key)
        n = sharing.output_size()
        rb = np.zeros(max(n, 1), np.uint64)
        _check(self.lib.sda_participant_share_keyed_dev(self.h, C.byref(ms), _ptr(sd, _u32p), sd.size, full_masks_ptr,
                                                        C.byref(ss), secrets_ptr, dimension, _ptr(k, _u32p), stream_id,
                                                        mode, shares_ptr, payload_ptr, payload_cap, _ptr(rb, _u64p),
                                                        stream))
        return rb[:n]

    def participant_share32_keyed_dev(self, masking, sharing, secrets_ptr, dimension, key, stream_id, shares_ptr,
                                      seed=None, full_masks_ptr=None, payload_ptr=None, payload_cap=0,
                                      mode=REVEAL_EXACT, stream=None):
        """participant_share_keyed_dev with shares_ptr as device int32 [n][B] (PackedShamir, and Additive up to
        modulus 2^31) and the payload from the int32 encoder."""
        ms, ss = masking.c(), sharing.c()
        sd = _arr(seed if seed is not None else [], np.uint32)
        k = self._key(key)
        n = sharing.output_size()
        rb = np.zeros(max(n, 1), np.uint64)
        _check(self.lib.sda_participant_share32_keyed_dev(self.h, C.byref(ms), _ptr(sd, _u32p), sd.size,
                                                          full_masks_ptr, C.byref(ss), secrets_ptr, dimension,
                                                          _ptr(k, _u32p), stream_id, mode, shares_ptr, payload_ptr,
                                                          payload_cap, _ptr(rb, _u64p), stream))
        return rb[:n]
