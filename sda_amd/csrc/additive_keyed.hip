// additive_keyed.hip -- Additive share generation (additive.rs:32-51) with the draws made in the kernel.
//
// Column d of a call (absolute column c = first_column + d) owns draws c (n - 1) .. c (n - 1) + n - 2 of the draw
// rule (draws.hip): share j < n - 1 of the column is draw c (n - 1) + j, and the last share is the fold of
// additive.rs:47 over them in order, last = (last - x_j) % m from the raw secret, with a wrapping subtraction.
// The draws never exist in device memory as a buffer: the kernel reads the secrets and writes the n share rows,
// 8 D (n + 1) bytes as i64 and 4 D (2 + n) as int32, where sda_draws_dev + additive_generate_kernel move
// 8 D (3 n - 1).
//
// A workgroup is one wave and owns kAdditiveKeyedTile columns, i.e. the contiguous element range
// [C (n - 1), (C + w)(n - 1)) of the draw stream.  It walks that range in chunks of 64 ChaCha blocks (512
// elements) laid out in absolute block indices, one block per lane, so the LDS footprint does not depend on n:
//   * the chunk's first and last block may hold elements of a neighbouring workgroup's columns (or of no column
//     of the call): they are computed and never used;
//   * a chunk's 512 results go to LDS (draws.hip's padded layout); then lane l folds column l, l + 64, ... of the
//     chunk (the secret is read when a column starts in the chunk; a column cut by the chunk's end hands its
//     running value to the next chunk through an LDS word), and the draws are stored row by row: consecutive
//     lanes write consecutive columns of one share row, so a store instruction covers runs of
//     min(64, 512 / (n - 1)) contiguous values.  A chunk that holds at most two columns (every chunk from
//     n - 1 > 510 on) is stored in element order instead.
// Every store is nontemporal and every output value is written once.
#include "draws_common.h"

namespace sda {

namespace {

constexpr uint32_t kLanes = 64;                // one wave per workgroup
constexpr uint32_t kChunk = kLanes * 8;        // elements per chunk: one ChaCha block per lane
constexpr uint32_t kCarry = kLanes * kPad;     // LDS words kCarry, kCarry + 1: the fold handed to the next chunk
static_assert(kAdditiveKeyedTile % kLanes == 0, "a tile is a whole number of lane rounds");

// (col, j) += delta elements of the stream; j < n1 before and after, delta <= kChunk
__device__ __forceinline__ void advance(uint64_t& col, uint64_t& j, uint32_t delta, uint64_t n1) {
    const uint64_t room = n1 - j;              // elements left in the column, >= 1
    if (delta < room) {
        j += delta;
        return;
    }
    delta -= (uint32_t)room;                   // room <= delta <= kChunk
    col += 1;
    if (delta >= n1) {                         // n1 <= delta < kChunk: 32-bit division
        const uint32_t q = delta / (uint32_t)n1;
        col += q;
        delta -= q * (uint32_t)n1;
    }
    j = delta;
}

// out[j * out_stride + d] = draw((first_column + d)(n - 1) + j), j < n - 1; out[(n - 1) * out_stride + d] = the fold.
// Workgroup x owns columns (wg0 + x) * kAdditiveKeyedTile ... of the call; wg0 is the grid slice's first workgroup.
template <typename Out>
__global__ __launch_bounds__(kLanes) void additive_generate_keyed_kernel(
    DrawKey key, uint32_t stream_id, uint64_t first_column, const int64_t* __restrict__ secrets, uint64_t dimension,
    uint64_t n, uint64_t wg0, Mod64 M, uint64_t zone, Out* __restrict__ out, uint64_t out_stride) {
    __shared__ unsigned long long st[kLanes * kPad + 2];
    const uint32_t tid = threadIdx.x;
    const uint64_t c0 = (wg0 + blockIdx.x) * kAdditiveKeyedTile;      // the tile's first column, < dimension
    const uint64_t left = dimension - c0;
    const uint32_t cw = left < kAdditiveKeyedTile ? (uint32_t)left : kAdditiveKeyedTile;
    const uint64_t n1 = n - 1;
    secrets += c0;
    out += c0;
    if (n1 == 0) {                             // no draws: the fold over an empty list is the raw secret
        for (uint32_t l = tid; l < cw; l += kLanes) __builtin_nontemporal_store((Out)secrets[l], out + l);
        return;
    }
    // absolute element range of the tile; the host checked that (first_column + dimension) * n1 does not wrap
    const uint64_t E0 = (first_column + c0) * n1;
    const uint64_t E1 = E0 + (uint64_t)cw * n1;
    const uint64_t blk_end = ((E1 - 1) >> 3) + 1;
    const int64_t m = (int64_t)M.m;
    const bool small_m = M.m <= (1ull << 62);  // (-m, m) - [0, m) cannot wrap
    Out* last_row = out + n1 * out_stride;
    uint64_t ca = 0, ja = 0;                   // tile column and draw index of the chunk's first kept element
    uint32_t it = 0;
    for (uint64_t cb = E0 >> 3; cb < blk_end; cb += kLanes, ++it) {
        if (cb + tid < blk_end) {
            uint64_t res[8];
            draw_eight(key, cb + tid, stream_id, M, zone, res);
#pragma unroll
            for (int q = 0; q < 8; ++q) st[tid * kPad + q] = res[q];
        }
        __syncthreads();
        const uint64_t ce0 = cb << 3;                                  // the chunk's first element
        const uint32_t off = ce0 < E0 ? (uint32_t)(E0 - ce0) : 0u;     // its elements before the tile (first chunk)
        const uint64_t rem = E1 - (ce0 + off);                         // elements of the tile from here on, >= 1
        const uint32_t len = rem < kChunk - off ? (uint32_t)rem : kChunk - off;   // kept elements of the chunk
        uint64_t cl = ca, jl = ja;                                     // the last kept element
        advance(cl, jl, len - 1, n1);
        const uint32_t nc = (uint32_t)(cl - ca) + 1;                   // columns with an element in the chunk
        const uint32_t n1w = (uint32_t)n1, jaw = (uint32_t)ja;         // exact wherever a product below is used
        // ---- fold: lane l takes the chunk's columns l, l + 64, ... ----
        for (uint32_t l = tid; l < nc; l += kLanes) {
            const uint64_t js = l == 0 ? ja : 0;
            const uint64_t je = l == nc - 1 ? jl + 1 : n1;
            const uint32_t cnt = (uint32_t)(je - js);
            uint32_t pos = off + (l == 0 ? 0u : l * n1w - jaw);        // LDS position of (column, js); < kChunk
            int64_t last = js == 0 ? secrets[ca + l] : (int64_t)st[kCarry + (it & 1)];
            {                                  // the column's first step of the chunk: `last` may be a raw secret
                const int64_t x = (int64_t)st[(pos >> 3) * kPad + (pos & 7)];
                const int64_t v = (int64_t)((uint64_t)last - (uint64_t)x);
                last = small_m && last > -m && last < m ? (v <= -m ? v + m : v) : trem64(v, M);
                ++pos;
            }
            if (small_m) {                     // last in (-m, m) from here on: v in (-2m, m), one adjust is the `%`
#pragma unroll 4
                for (uint32_t k = 1; k < cnt; ++k, ++pos) {
                    const int64_t v = last - (int64_t)st[(pos >> 3) * kPad + (pos & 7)];
                    last = v <= -m ? v + m : v;
                }
            } else {
                for (uint32_t k = 1; k < cnt; ++k, ++pos) {
                    const int64_t x = (int64_t)st[(pos >> 3) * kPad + (pos & 7)];
                    last = trem64((int64_t)((uint64_t)last - (uint64_t)x), M);
                }
            }
            if (je == n1)
                __builtin_nontemporal_store((Out)last, last_row + ca + l);
            else
                st[kCarry + ((it + 1) & 1)] = (unsigned long long)last;
        }
        // ---- the draws, row by row ----
        if (nc > 2) {                          // then a whole column lies inside the chunk: n1 <= kChunk - 2
            const uint32_t total = nc * n1w;
            const uint32_t dq = kLanes / nc, dr = kLanes % nc;
            uint32_t j = tid / nc, l = tid - j * nc;
            for (uint32_t idx = tid; idx < total; idx += kLanes) {
                const int32_t rel = (int32_t)(l * n1w + j) - (int32_t)jaw;   // element offset from the first kept one
                if (rel >= 0 && (uint32_t)rel < len) {
                    const uint32_t pos = off + (uint32_t)rel;
                    __builtin_nontemporal_store((Out)(int64_t)st[(pos >> 3) * kPad + (pos & 7)],
                                                out + (uint64_t)j * out_stride + ca + l);
                }
                j += dq;
                l += dr;
                if (l >= nc) {
                    l -= nc;
                    ++j;
                }
            }
        } else {
            const uint64_t room = n1 - ja;     // elements of the first column from (ca, ja) on
            for (uint32_t idx = tid; idx < len; idx += kLanes) {
                const bool second = idx >= room;
                const uint64_t j = second ? idx - room : ja + idx;
                const uint32_t pos = off + idx;
                __builtin_nontemporal_store((Out)(int64_t)st[(pos >> 3) * kPad + (pos & 7)],
                                            out + j * out_stride + ca + (second ? 1u : 0u));
            }
        }
        advance(ca, ja, len, n1);
        __syncthreads();
    }
}

template <typename Out>
hipError_t launch(const uint32_t* key_host, uint32_t stream_id, uint64_t first_column, const int64_t* secrets,
                  uint64_t D, uint64_t n, int64_t modulus, Out* out, uint64_t out_stride, hipStream_t s) {
    DrawKey key;
    for (int q = 0; q < 8; ++q) key.k[q] = key_host[q];
    const Mod64 M = make_mod64(modulus);
    const uint64_t zone = UINT64_MAX - UINT64_MAX % (uint64_t)modulus;
    const uint64_t n_wg = (D + kAdditiveKeyedTile - 1) / kAdditiveKeyedTile;
    constexpr uint64_t kSlice = 1ull << 30;                                    // workgroups per launch
    for (uint64_t wg0 = 0; wg0 < n_wg; wg0 += kSlice) {
        const uint64_t g = n_wg - wg0 < kSlice ? n_wg - wg0 : kSlice;
        hipLaunchKernelGGL(additive_generate_keyed_kernel<Out>, dim3((unsigned)g), dim3(kLanes), 0, s, key, stream_id,
                           first_column, secrets, D, n, wg0, M, zone, out, out_stride);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_additive_generate_keyed(const uint32_t* key_host, uint32_t stream_id, uint64_t first_column,
                                          const int64_t* secrets, uint64_t D, uint64_t n, int64_t modulus,
                                          int64_t* out64, int32_t* out32, uint64_t out_stride, hipStream_t s) {
    if (D == 0) return hipSuccess;
    return out32 ? launch(key_host, stream_id, first_column, secrets, D, n, modulus, out32, out_stride, s)
                 : launch(key_host, stream_id, first_column, secrets, D, n, modulus, out64, out_stride, s);
}

}  // namespace sda
