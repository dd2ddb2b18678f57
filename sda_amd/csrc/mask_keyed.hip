// mask_keyed.hip -- Full masking (full.rs:22-35) with the mask drawn in the kernel.
//
// For p < count: mask[p] = draw(first + p) of the draw rule (draws.hip) under (key, stream_id) at bound = m, and
// masked[p] = (secrets[p] + mask[p]) % m with a wrapping add and Rust's truncated `%` (full.rs:28-31).  The mask
// must reach the recipient, so it is an output too -- as i64, or as int32 where m <= 2^31 (every value lies in
// [0, m)) -- but it is written once and never read back: the kernel reads 8 bytes an element and writes 8 + (8 or
// 4), where launch_draws + launch_addsub_trem move 8 + 24.
//
// The layout is draws.hip's: one lane expands one block (8 draws), the grid is laid out in absolute block indices
// from first >> 3, so `first` need not be a multiple of 8, and a workgroup's 2048 results go through LDS so that
// lane t handles element t + 256 j: each load and each store instruction covers 256 contiguous values.
// Every output value is written once, nontemporal.
#include "draws_common.h"

namespace sda {

namespace {

static_assert(kDrawsTile == 256 * 8, "one lane per block of 8 draws, 256 lanes per workgroup");

// Workgroup x owns blocks blk0 + 256 x + lane (blk0 = first >> 3); wg0 is the grid slice's first workgroup
// (launch_full_mask_keyed slices grids past 2^30 workgroups).
template <typename MaskOut>
__global__ __launch_bounds__(256) void full_mask_keyed_kernel(DrawKey key, uint32_t stream_id, uint64_t first,
                                                              uint64_t count, uint64_t wg0, Mod64 M, uint64_t zone,
                                                              const int64_t* __restrict__ secrets,
                                                              int64_t* __restrict__ masked,
                                                              MaskOut* __restrict__ mask) {
    __shared__ unsigned long long st[256 * kPad];
    const uint32_t tid = threadIdx.x;
    const uint64_t wg = wg0 + blockIdx.x;
    // element e0 + idx of the workgroup's 2048; e0 may lie up to 7 below `first`, and e0 + idx - first is the
    // position once e0 + idx >= first (compared as offsets from e0: no wrap at either end of the range)
    const uint64_t e0 = ((first >> 3) + wg * 256) << 3;
    const uint64_t lead = wg == 0 ? first - e0 : 0;          // elements of this tile before `first` (0..7)
    const uint64_t p0 = wg == 0 ? 0 : e0 - first;            // position of the tile's first kept element
    const uint64_t left = count - p0;                        // p0 < count: the grid holds no tile past the range
    const uint64_t blk = (first >> 3) + wg * 256 + tid;      // cannot wrap: the host checked first + count
    uint64_t res[8];
    draw_eight(key, blk, stream_id, M, zone, res);
    // the lane's eight secrets, asked for once the ChaCha state's registers are free (the kernel keeps the draws
    // kernel's 8 waves per SIMD): their latency hides under the LDS exchange and the other waves' rounds
    int64_t sec[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t idx = j * 256 + tid;
        sec[j] = idx >= lead && idx - lead < left ? __builtin_nontemporal_load(secrets + p0 + (idx - lead)) : 0;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) st[tid * kPad + q] = res[q];
    __syncthreads();
    const bool small_m = M.m <= (1ull << 62);                // [0, m) + (-m, m) cannot wrap
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t idx = j * 256 + tid;
        if (idx >= lead && idx - lead < left) {
            const uint64_t p = p0 + (idx - lead);
            const int64_t x = (int64_t)st[(idx >> 3) * kPad + (idx & 7)];
            __builtin_nontemporal_store((MaskOut)x, mask + p);
            __builtin_nontemporal_store(add_trem(x, sec[j], M, small_m), masked + p);
        }
    }
}

template <typename MaskOut>
hipError_t launch(const uint32_t* key_host, uint32_t stream_id, uint64_t first, const int64_t* secrets, uint64_t count,
                  int64_t modulus, int64_t* masked, MaskOut* mask, hipStream_t s) {
    DrawKey key;
    for (int q = 0; q < 8; ++q) key.k[q] = key_host[q];
    const Mod64 M = make_mod64(modulus);
    const uint64_t zone = UINT64_MAX - UINT64_MAX % (uint64_t)modulus;
    const uint64_t n_blk = ((first + (count - 1)) >> 3) - (first >> 3) + 1;   // blocks that hold a kept element
    const uint64_t n_wg = (n_blk + 255) / 256;
    constexpr uint64_t kSlice = 1ull << 30;                                    // workgroups per launch
    for (uint64_t wg0 = 0; wg0 < n_wg; wg0 += kSlice) {
        const uint64_t g = n_wg - wg0 < kSlice ? n_wg - wg0 : kSlice;
        hipLaunchKernelGGL(full_mask_keyed_kernel<MaskOut>, dim3((unsigned)g), dim3(256), 0, s, key, stream_id, first,
                           count, wg0, M, zone, secrets, masked, mask);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_full_mask_keyed(const uint32_t* key_host, uint32_t stream_id, uint64_t first, const int64_t* secrets,
                                  uint64_t count, int64_t modulus, int64_t* masked, int64_t* mask64, int32_t* mask32,
                                  hipStream_t s) {
    if (count == 0) return hipSuccess;
    return mask32 ? launch(key_host, stream_id, first, secrets, count, modulus, masked, mask32, s)
                  : launch(key_host, stream_id, first, secrets, count, modulus, masked, mask64, s);
}

}  // namespace sda
