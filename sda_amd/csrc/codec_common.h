// codec_common.h -- what the two halves of the share payload codec (codec_decode.hip, codec_encode.hip) share.
#pragma once
#include <stdlib.h>

#include "kernels.h"

namespace sda {

namespace {

constexpr int kThreads = 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // one 16-byte word of payload

// Inclusive prefix sum over the 64 lanes of a wave with DPP (row shifts, then the row broadcasts of
// gfx9): six VALU adds, no LDS round trips.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);   // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);   // row_bcast:15
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);   // row_bcast:31
    return x;
}

}  // namespace

}  // namespace sda
