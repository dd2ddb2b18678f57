// draws.hip -- the engine's own uniform draws: ChaCha20 in counter mode under a caller-supplied key.
//
// Where the reference draws from OsRng (additive.rs:42-44, tss' packed `share`, full.rs:25-27) there is no
// stream to reproduce; what must hold is that every draw is uniform on [0, bound), independent and derived
// from OS entropy.  The caller draws one 256-bit key per call and the device expands it (DESIGN.md "Device
// draws").  Element i (an absolute 64-bit index) at retry round r = 0, 1, ...:
//   state = "expand 32-byte k" | key[0..7] | block counter i >> 3 (low, high word) | stream_id | r
//   o = core(state) (20 rounds + feed-forward); j = i & 7; v = (o[2j] << 32) | o[2j + 1]  (high word first)
//   v < zone = u64::MAX - u64::MAX % bound (rand 0.3's gen_range rule): the draw is v % bound;
//   otherwise round r + 1, same block counter and position; round 63 is taken unconditionally.
// An element depends only on (key, stream_id, i, bound): any sub-range, device split or launch shape gives
// the same values.  chacha.hip's block function keeps state words 14 and 15 at zero (rand 0.3's stream), so
// draws_common.h carries its own with the two extra words, shared with additive_keyed.hip.
//
// One lane expands one block (8 draws).  The grid is laid out in absolute block indices from first >> 3, so
// `first` need not be a multiple of 8: the first and last block's elements outside [first, first + count)
// are computed and never stored.  A workgroup's 2048 results go through LDS so that lane t stores element
// t + 256 j: each store instruction writes 512 contiguous bytes, once, nontemporal.
#include "draws_common.h"

namespace sda {

namespace {

static_assert(kDrawsTile == 256 * 8, "one lane per block of 8 draws, 256 lanes per workgroup");

// out[p] = draw(first + p), p < count.  Workgroup x owns blocks blk0 + 256 x + lane (blk0 = first >> 3); wg0 is
// the grid slice's first workgroup (launch_draws slices grids past 2^30 workgroups).
__global__ __launch_bounds__(256) void draws_kernel(DrawKey key, uint32_t stream_id, uint64_t first, uint64_t count,
                                                    uint64_t wg0, Mod64 M, uint64_t zone,
                                                    unsigned long long* __restrict__ out) {
    __shared__ unsigned long long st[256 * kPad];
    const uint32_t tid = threadIdx.x;
    const uint64_t wg = wg0 + blockIdx.x;
    const uint64_t blk = (first >> 3) + wg * 256 + tid;      // cannot wrap: the host checked first + count
    uint64_t res[8];
    draw_eight(key, blk, stream_id, M, zone, res);
#pragma unroll
    for (int q = 0; q < 8; ++q) st[tid * kPad + q] = res[q];
    __syncthreads();
    // element e0 + idx of the workgroup's 2048; e0 may lie up to 7 below `first`, and e0 + idx - first is the
    // output position once e0 + idx >= first (compared as offsets from e0: no wrap at either end of the range)
    const uint64_t e0 = ((first >> 3) + wg * 256) << 3;
    const uint64_t lead = wg == 0 ? first - e0 : 0;          // elements of this tile before `first` (0..7)
    const uint64_t p0 = wg == 0 ? 0 : e0 - first;            // output position of the tile's first kept element
    const uint64_t left = count - p0;                        // p0 < count: the grid holds no tile past the range
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t idx = j * 256 + tid;
        if (idx >= lead && idx - lead < left)
            __builtin_nontemporal_store(st[(idx >> 3) * kPad + (idx & 7)], out + p0 + (idx - lead));
    }
}

}  // namespace

hipError_t launch_draws(const uint32_t* key_host, uint32_t stream_id, uint64_t first, uint64_t count, int64_t bound,
                        int64_t* out, hipStream_t s) {
    if (count == 0) return hipSuccess;
    DrawKey key;
    for (int q = 0; q < 8; ++q) key.k[q] = key_host[q];
    const Mod64 M = make_mod64(bound);
    const uint64_t zone = UINT64_MAX - UINT64_MAX % (uint64_t)bound;
    const uint64_t n_blk = ((first + (count - 1)) >> 3) - (first >> 3) + 1;   // blocks that hold a kept element
    const uint64_t n_wg = (n_blk + 255) / 256;
    constexpr uint64_t kSlice = 1ull << 30;                                    // workgroups per launch
    for (uint64_t wg0 = 0; wg0 < n_wg; wg0 += kSlice) {
        const uint64_t g = n_wg - wg0 < kSlice ? n_wg - wg0 : kSlice;
        hipLaunchKernelGGL(draws_kernel, dim3((unsigned)g), dim3(256), 0, s, key, stream_id, first, count, wg0, M, zone,
                           reinterpret_cast<unsigned long long*>(out));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sda
