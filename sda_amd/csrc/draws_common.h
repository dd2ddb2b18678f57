// draws_common.h -- the draw rule's device code, shared by the kernels that expand it (draws.hip,
// additive_keyed.hip, mask_keyed.hip, packed_gen.hip's keyed kernels): the ChaCha20 block with state words 14 = stream_id and 15 = retry round, and one lane's
// block of 8 draws with its per-element retry rounds.  draws.hip states the rule.
#pragma once
#include "kernels.h"

namespace sda {

namespace {

constexpr uint32_t C0 = 0x61707865u, C1 = 0x3320646Eu, C2 = 0x79622D32u, C3 = 0x6B206574u;
constexpr uint32_t kLastRound = 63;            // the retry round whose value is taken unconditionally
constexpr int kPad = 9;                        // LDS row stride (u64) of a lane's 8 results

struct DrawKey { uint32_t k[8]; };

__device__ __forceinline__ uint32_t rotl(uint32_t x, int r) { return __builtin_amdgcn_alignbit(x, x, 32 - r); }

#define SDA_DQR(a, b, c, d)                   \
    a += b; d ^= a; d = rotl(d, 16);          \
    c += d; b ^= c; b = rotl(b, 12);          \
    a += b; d ^= a; d = rotl(d, 8);           \
    c += d; b ^= c; b = rotl(b, 7);

// core(state) with state words 14 = stream_id, 15 = round
__device__ __forceinline__ void draw_block(const DrawKey& K, uint64_t counter, uint32_t stream_id, uint32_t round,
                                           uint32_t (&o)[16]) {
    const uint32_t* key = K.k;
    uint32_t x0 = C0, x1 = C1, x2 = C2, x3 = C3;
    uint32_t x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3];
    uint32_t x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7];
    uint32_t x12 = (uint32_t)counter, x13 = (uint32_t)(counter >> 32), x14 = stream_id, x15 = round;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        SDA_DQR(x0, x4, x8, x12); SDA_DQR(x1, x5, x9, x13); SDA_DQR(x2, x6, x10, x14); SDA_DQR(x3, x7, x11, x15);
        SDA_DQR(x0, x5, x10, x15); SDA_DQR(x1, x6, x11, x12); SDA_DQR(x2, x7, x8, x13); SDA_DQR(x3, x4, x9, x14);
    }
    o[0] = x0 + C0; o[1] = x1 + C1; o[2] = x2 + C2; o[3] = x3 + C3;
    o[4] = x4 + key[0]; o[5] = x5 + key[1]; o[6] = x6 + key[2]; o[7] = x7 + key[3];
    o[8] = x8 + key[4]; o[9] = x9 + key[5]; o[10] = x10 + key[6]; o[11] = x11 + key[7];
    o[12] = x12 + (uint32_t)counter; o[13] = x13 + (uint32_t)(counter >> 32);
    o[14] = x14 + stream_id; o[15] = x15 + round;
}
#undef SDA_DQR

// v % bound: the 64-bit Barrett `%` of modarith.h, for every bound in [1, 2^63)
__device__ __forceinline__ uint64_t draw_mod(uint64_t v, const Mod64& M) { return umod64(v, M); }

// res[q] = draw(8 blk + q), q < 8: the eight draws of block `blk`
__device__ __forceinline__ void draw_eight(const DrawKey& key, uint64_t blk, uint32_t stream_id, const Mod64& M,
                                           uint64_t zone, uint64_t (&res)[8]) {
    uint32_t rej = 0;                                        // bit q: element q still waits for an accepted value
    {
        uint32_t o[16];
        draw_block(key, blk, stream_id, 0u, o);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint64_t v = ((uint64_t)o[2 * q] << 32) | o[2 * q + 1];   // high word first
            rej |= v < zone ? 0u : (1u << q);                // the one accept/retry decision, for every bound
            res[q] = draw_mod(v, M);
        }
    }
    // Retries, per element: round r of block `blk` serves every element of the lane still waiting at r, each
    // at its own position.  Rare for the shipped moduli (< 2^-32 per draw below 2^32), about one element in
    // three for bounds near 2^64 / 3; elements outside the caller's range retry too and are never stored.
    for (uint32_t r = 1; rej != 0 && r <= kLastRound; ++r) {
        uint32_t o[16];
        draw_block(key, blk, stream_id, r, o);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint64_t v = ((uint64_t)o[2 * q] << 32) | o[2 * q + 1];
            if ((rej >> q) & 1u) {
                res[q] = draw_mod(v, M);
                if (v < zone) rej &= ~(1u << q);             // at r == kLastRound the value stands either way
            }
        }
    }
}

}  // namespace

}  // namespace sda
