"""The decisions of the two role pipelines (sda_amd/csrc/engine_recipient.cpp, engine_participant.cpp), restated once
in Python: what sda_recipient_last_launch and sda_participant_last_launch must report for a call, and the status of
every early return, in the order the host code takes them.  No GPU, no product import beyond the scheme descriptors.

tests/pipeline_matrix_cases.py builds its cases on these functions, tests/test_pipeline_matrix_plan.py holds the case
tables against them, tests/test_gpu_pipeline_matrix.py asserts them on the device.
"""
from sda_amd import schemes as S

I64_MIN, I64_MAX = -(2**63), 2**63 - 1
U64_MAX = 2**64 - 1
EXACT, CANONICAL = 0, 1
REVEAL_MAX_SHARES = 1023                  # kernels.h kRevealMaxShares

# include/sda_engine.h sda_status
OK = 0
MISMATCHING_DIMENSION = 4
NOT_ENOUGH_SHARES = 6
PRECONDITION = 64
INVALID_ARGUMENT = 65
UNSUPPORTED = 66

# sda_recipient_last_launch
MASK_NONE_YET, MASK_NONE, MASK_FULL, MASK_CHACHA, MASK_COMBINED_ROW = 0, 1, 2, 3, 4
REVEAL_ADDITIVE, REVEAL_EXACT, REVEAL_CANONICAL = 0, 1, 2
# sda_participant_last_launch
ROUTE_MASK_NONE, ROUTE_FULL_ADD, ROUTE_CHACHA_FUSED, ROUTE_CHACHA_COMBINE_ADD = 1, 2, 3, 4
ROUTE_ADDITIVE, ROUTE_ADDITIVE_KEYED, ROUTE_PACKED, ROUTE_PACKED_KEYED = 1, 2, 3, 4

ENTRIES = ("dev", "dev32", "keyed", "keyed32")          # sda_participant_share{,32}{,_keyed}_dev


def is_packed(ss):
    return isinstance(ss, S.PackedShamir)


def mask_kind(ms):
    return MASK_NONE if isinstance(ms, S.NoMasking) else MASK_FULL if isinstance(ms, S.FullMasking) else MASK_CHACHA


def batches(ss, dimension):
    return (dimension + ss.secret_count - 1) // ss.secret_count if is_packed(ss) else 0


# ---------------------------------------------------------------- ChaCha
def chacha_needs_stream_path(m):
    """chacha.hip chacha_needs_stream_path, for m != 0 (the host never asks it about 0)."""
    um = m % 2**64
    return um > 2**62 or U64_MAX % um + 1 > 2**36


def chacha_fast_path(m, env_path=None):
    """engine.cpp chacha_fast_path."""
    return not chacha_needs_stream_path(m) and env_path != "stream"


def chacha_pending(ms, n_masks, env_path=None):
    """engine.cpp chacha_combine_begin: the recipient's ChaCha mask is resolved after the reveal was queued."""
    return isinstance(ms, S.ChaChaMasking) and chacha_fast_path(ms.modulus, env_path) and n_masks > 0


# ---------------------------------------------------------------- recipient
def residue_only(ms, ss, output_modulus, env_exact=None):
    """engine_recipient.cpp `residue_only`: q is |masking modulus|."""
    p = ss.prime_modulus
    keep = env_exact is not None and env_exact.strip().lstrip("+-").isdigit() and int(env_exact) == 1
    return output_modulus == p and (isinstance(ms, S.NoMasking) or abs(ms.modulus) == p) and not keep


def run_mode(ms, ss, output_modulus, mode, env_exact=None):
    """engine_recipient.cpp `run_mode`."""
    return CANONICAL if mode == EXACT and residue_only(ms, ss, output_modulus, env_exact) else mode


def has_duplicates(indices):
    return len(set(indices)) != len(indices)


def fell_back(ms, ss, output_modulus, mode, indices, env_exact=None):
    """The canonical reveal refuses repeated clerk points; a substituted one then reruns as asked (EXACT)."""
    return run_mode(ms, ss, output_modulus, mode, env_exact) != mode and has_duplicates(indices)


def compact(ss, dimension, share_len):
    """engine_recipient.cpp `compact`."""
    return is_packed(ss) and share_len != batches(ss, dimension)


def recipient_record(ms, ss, dimension, indices, share_len, output_modulus, mode, env_exact=None, late_resolve=False,
                     multi_mask=False):
    """(mask_kind, reveal_mode, fell_back, compact, unmask_launches) of a recipient call that returns SDA_OK with a
    non-empty output.  late_resolve: the pending ChaCha mask had a rejected draw.  multi_mask: the host form on a
    multi-device handle combined the ChaCha mask before the pipeline."""
    if is_packed(ss):
        fb = fell_back(ms, ss, output_modulus, mode, indices, env_exact)
        rm = mode if fb else run_mode(ms, ss, output_modulus, mode, env_exact)
        reveal = REVEAL_CANONICAL if rm == CANONICAL else REVEAL_EXACT
    else:
        fb, reveal = False, REVEAL_ADDITIVE
    return (MASK_COMBINED_ROW if multi_mask else mask_kind(ms), reveal, int(fb),
            int(compact(ss, dimension, share_len)), 2 if late_resolve else 1)


def multi_mask(ms, n_masks):
    """sda_recipient_reveal on a handle from sda_engine_create_multi: `multi_mask`."""
    return isinstance(ms, S.ChaChaMasking) and n_masks > 0 and ms.dimension > 0 and ms.modulus > 0


def _modulus_abs(m):
    """engine.cpp modulus_abs."""
    if m == 0:
        return (PRECONDITION, "divisor of zero")
    if m == I64_MIN:
        return (UNSUPPORTED, "i64::MIN")
    return None


def check_packed(ss):
    """engine.cpp check_packed, for the schemes the matrix uses (all inside the domain)."""
    k, t, n, p = ss.secret_count, ss.privacy_threshold(), ss.share_count, ss.prime_modulus
    def pow_of(x, b):
        while x > 1 and x % b == 0:
            x //= b
        return x == 1

    if k == 0 or not pow_of(k + t + 1, 2) or not pow_of(n + 1, 3) or p < 3 or p % 2 == 0 or p >= 2**31:
        return (UNSUPPORTED, "domain")
    if n < k + t:
        return (PRECONDITION, "share_count")
    return None


def mask_combine_status(ms, n_masks, mask_width):
    """engine_recipient.cpp mask_combine_checks -> (status or None, mask_len)."""
    if isinstance(ms, S.NoMasking):
        if n_masks and mask_width:
            return (PRECONDITION, "masks.iter().all"), 0
        return None, 0
    if isinstance(ms, S.FullMasking):
        mask_len = mask_width if n_masks else 0
        return (_modulus_abs(ms.modulus) if mask_len else None), mask_len
    if mask_width == 0 or mask_width > 8:
        return (UNSUPPORTED, "1..8 words"), ms.dimension
    if ms.dimension and n_masks and ms.modulus <= 0:
        return (PRECONDITION, "gen_range"), ms.dimension
    return None, ms.dimension


def recipient_status(ms, n_masks, mask_width, ss, dimension, n_idx, share_len, output_modulus, mode, out_cap):
    """recipient_pipeline's early returns, in its order -> ((status, message class) or None, out_len)."""
    st, mask_len = mask_combine_status(ms, n_masks, mask_width)
    if st:
        return st, 0
    if not is_packed(ss):
        D = share_len if n_idx else 0
        if D and _modulus_abs(ss.modulus):
            return _modulus_abs(ss.modulus), 0
    else:
        if check_packed(ss):
            return check_packed(ss), 0
        if mode not in (EXACT, CANONICAL):
            return (INVALID_ARGUMENT, "bad mode"), 0
        B = batches(ss, dimension)
        if B:
            enough = n_idx >= ss.privacy_threshold() + ss.secret_count
            if n_idx and share_len < (B if enough else 1):
                return (PRECONDITION, "index out of bounds"), 0
            if not enough:
                return (NOT_ENOUGH_SHARES, "Not enough shares"), 0
            if n_idx > REVEAL_MAX_SHARES:
                return (UNSUPPORTED, "clerk shares per batch"), 0
        D = dimension
    if not isinstance(ms, S.NoMasking) and mask_len != D:
        return (PRECONDITION, "mask.len() == masked_secrets.len()"), 0
    if out_cap < D:
        return (INVALID_ARGUMENT, "output buffer too small"), 0
    if D == 0:
        return None, 0
    if not isinstance(ms, S.NoMasking) and _modulus_abs(ms.modulus):
        return _modulus_abs(ms.modulus), 0
    return None, D


def recipient_host_status(ms, mask_lens, ss, dimension, share_lens, output_modulus, mode, out_cap):
    """sda_recipient_reveal's own shape checks, then recipient_pipeline's."""
    n_masks, n_idx = len(mask_lens), len(share_lens)
    if isinstance(ms, S.FullMasking):
        width = mask_lens[0] if n_masks else 0
        if any(l != width for l in mask_lens):
            if width and _modulus_abs(ms.modulus):
                return _modulus_abs(ms.modulus), 0
            return (PRECONDITION, "mask.len() == dimension"), 0
    elif isinstance(ms, S.ChaChaMasking):
        width = max(1, min(8, max(mask_lens, default=0)))           # engine.cpp pack_seeds
    else:
        if any(mask_lens):
            return (PRECONDITION, "masks.iter().all"), 0
        width = 0
    st, _ = mask_combine_status(ms, n_masks, width)
    if st:
        return st, 0
    share_len = share_lens[0] if n_idx else 0
    if any(l != share_len for l in share_lens):
        if not is_packed(ss):
            if share_len and _modulus_abs(ss.modulus):
                return _modulus_abs(ss.modulus), 0
            return (MISMATCHING_DIMENSION, "Mismatching dimension"), 0
        share_len = min(share_lens)
    st, D = recipient_status(ms, n_masks, width, ss, dimension, n_idx, share_len, output_modulus, mode, U64_MAX)
    if st:
        return st, 0
    if out_cap < D:
        return (INVALID_ARGUMENT, "output buffer too small"), 0
    return None, D


# ---------------------------------------------------------------- participant
def mask_route(ms, env_path=None):
    if isinstance(ms, S.NoMasking):
        return ROUTE_MASK_NONE
    if isinstance(ms, S.FullMasking):
        return ROUTE_FULL_ADD
    return ROUTE_CHACHA_FUSED if chacha_fast_path(ms.modulus, env_path) else ROUTE_CHACHA_COMBINE_ADD


def share_route(ss, entry):
    keyed = entry in ("keyed", "keyed32")
    if is_packed(ss):
        return ROUTE_PACKED_KEYED if keyed else ROUTE_PACKED
    return ROUTE_ADDITIVE_KEYED if keyed else ROUTE_ADDITIVE


def participant_record(ms, ss, entry, env_path=None, late_resolve=False):
    """(mask_route, share_route, passes) of a participant call of dimension > 0 that returns SDA_OK."""
    return (mask_route(ms, env_path), share_route(ss, entry), 2 if late_resolve else 1)


def participant_status(ms, ss, entry, dimension, seed_words, mode, has_seed=True, has_full_masks=True,
                       has_draws=True, payload_cap=None, payload_need=0):
    """participant_share's early returns, in its order (the NULL-argument row aside) -> (status, class) or None."""
    packed = is_packed(ss)
    if not packed and entry == "dev32":
        return (UNSUPPORTED, "int32 shares need a PackedShamir scheme")
    if mode not in (EXACT, CANONICAL):
        return (INVALID_ARGUMENT, "bad mode")
    if packed:
        if check_packed(ss):
            return check_packed(ss)
    else:
        if ss.share_count == 0:
            return (PRECONDITION, "share_count - 1 underflows")
        if ss.modulus <= 0:
            return (PRECONDITION, "gen_range")
        if entry == "keyed32" and ss.modulus > 2**31:
            return (UNSUPPORTED, "modulus <= 2^31")
    D = dimension
    if isinstance(ms, S.ChaChaMasking) and ms.dimension != D:         # chacha.rs:26, an empty vector included
        return (PRECONDITION, "dimension == secrets.len()")
    if not isinstance(ms, S.NoMasking) and D:
        if ms.modulus <= 0:
            return (PRECONDITION, "gen_range")
        if isinstance(ms, S.FullMasking):
            if not has_full_masks:
                return (INVALID_ARGUMENT, "Full masking needs the drawn masks")
        else:
            if seed_words != ms.seed_words() or (seed_words and not has_seed):
                return (PRECONDITION, "seed words")
    B = batches(ss, D) if packed else D
    if B and not has_draws and entry in ("dev", "dev32"):
        return (INVALID_ARGUMENT, "need the randomness draws")
    if payload_cap is not None and payload_cap < payload_need:
        return (INVALID_ARGUMENT, "payload_cap")
    return None
