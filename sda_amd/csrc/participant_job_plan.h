// participant_job_plan.h -- the payload bound and the tile plan of the participant job (sda_participant_job,
// sda_participant_job_dev; engine_participant.cpp).  Header-only and HIP-free, so a plain C++ program can test it
// under a host sanitizer (tests/host_c).
#pragma once
#include <stdint.h>

#include <algorithm>

namespace sda {

// bytes of the payload codec's encoding of v (sodium.rs:36-41: zigzag, then 7 bits a byte)
inline uint32_t varint_len(int64_t v) {
    uint64_t z = ((uint64_t)v << 1) ^ (uint64_t)(v >> 63);
    uint32_t n = 1;
    for (; z >= 128; z >>= 7) ++n;
    return n;
}

// the most bytes a value of (-m, m) takes: the zigzag of m - 1 is 2 (m - 1), of -(m - 1) one less.  m <= 0 (no
// bound on the value): any i64, 10 bytes.
inline uint32_t varint_bound_mod(int64_t m) {
    if (m <= 0) return 10;
    uint64_t z = 2 * (uint64_t)(m - 1);                     // m <= 2^63 - 1: no wrap
    uint32_t n = 1;
    for (; z >= 128; z >>= 7) ++n;
    return n;
}

constexpr uint32_t kSeedWordBytes = 5;                      // a seed word `as i64` lies in [0, 2^32): zigzag < 2^33

// What decides the bytes of a participant job's payloads.  mask_kind: 0 None, 1 Full, 2 ChaCha (the values of
// sda_masking_kind); packed: PackedShamir, else Additive.
struct ParticipantJobShape {
    int mask_kind;
    int64_t mask_modulus;
    uint64_t seed_words;          // ChaCha: (seed_bitsize + 31) / 32
    bool packed;
    int64_t share_modulus;        // Additive: modulus; PackedShamir: prime_modulus
    uint64_t k;                   // secrets per batch (Additive: 1)
    uint64_t n;                   // clerks
};

// worst-case bytes of one share: every share lies in (-m, m) -- a PackedShamir share is a residue or tss' signed
// value of it, an Additive draw lies in [0, m) and the last share is a `% m` result -- except with one Additive
// clerk, whose share is the masked secret as it stands (additive.rs:47 folds over no draw): then the masking
// modulus bounds it, and without masking nothing does.
inline uint32_t participant_share_bytes_bound(const ParticipantJobShape& s) {
    if (!s.packed && s.n == 1) return s.mask_kind == 0 ? 10u : varint_bound_mod(s.mask_modulus);
    return varint_bound_mod(s.share_modulus);
}

// worst-case bytes of one mask value: a Full mask value lies in [0, m)
inline uint32_t participant_mask_bytes_bound(const ParticipantJobShape& s) {
    return s.mask_kind == 1 ? varint_bound_mod(s.mask_modulus) : 0u;
}

// *clerk_row = the most bytes one clerk's payload of a job over D secrets takes, *mask = the same for the
// recipient's mask payload; false when a bound does not fit 64 bits.
inline bool participant_job_bound(const ParticipantJobShape& s, uint64_t D, uint64_t* clerk_row, uint64_t* mask) {
    const uint64_t k = s.packed ? std::max<uint64_t>(s.k, 1) : 1;
    const uint64_t B = D / k + (D % k ? 1 : 0);
    *clerk_row = *mask = 0;
    if (__builtin_mul_overflow(B, (uint64_t)participant_share_bytes_bound(s), clerk_row)) return false;
    if (s.mask_kind == 1) return !__builtin_mul_overflow(D, (uint64_t)participant_mask_bytes_bound(s), mask);
    if (s.mask_kind == 2) return !__builtin_mul_overflow(s.seed_words, (uint64_t)kSeedWordBytes, mask);
    return true;
}

// The host job's tiles: whole batches (Additive: columns), `tile` of them at a time over `units` in all.  Tile i is
// units [i tile, min(units, (i + 1) tile)), i.e. secrets [u0 k, min(D, u1 k)).
struct ParticipantTilePlan {
    uint64_t units = 0, tile = 0, tiles = 0;
    uint64_t unit_bytes = 0;      // device bytes one unit takes in a tile
};
// stage_bytes: the budget of one tile (SDA_HOST_STAGE_MB); override_units > 0 replaces the tile size it gives
// (SDA_PARTICIPANT_TILE_BATCHES).  share_bytes: 4 or 8, the width of the share rows.
inline ParticipantTilePlan participant_job_tiles(const ParticipantJobShape& s, uint64_t D, uint32_t share_bytes,
                                                 uint64_t stage_bytes, uint64_t override_units) {
    ParticipantTilePlan p;
    const uint64_t k = s.packed ? std::max<uint64_t>(s.k, 1) : 1;
    p.units = D / k + (D % k ? 1 : 0);
    // secrets up and masked secrets (k i64 each), the mask row and its payload, n share values and their payloads
    p.unit_bytes = k * (16 + 8 + participant_mask_bytes_bound(s)) +
                   s.n * ((uint64_t)share_bytes + participant_share_bytes_bound(s));
    p.tile = override_units ? override_units : std::max<uint64_t>(1, stage_bytes / p.unit_bytes);
    p.tile = std::min(p.tile, std::max<uint64_t>(p.units, 1));
    p.tiles = (p.units + p.tile - 1) / p.tile;
    return p;
}

}  // namespace sda
