// codec_encode.hip -- share payload codec on gfx950: the payload encoder.  The byte
// format and its reference (sodium.rs:36-41, integer-encoding 1.0 VarInt) are described at the head of
// codec_decode.hip.
//
// Rows of i64 or int32 (a field share below 2^31) become one byte stream, the rows back to back:
//   size     per [row][chunk] block of elements, its encoded bytes;
//   offsets  per row, the exclusive scan of its chunks' bytes and its total; then the rows' bases;
//   write    per chunk, the bytes, built in LDS and stored 16 bytes at a time.
// One size body and one write body serve both element types; a traits struct per type (Enc64, Enc32) holds what
// differs.  From int32 an element takes at most 5 bytes, so the zigzag, the size and the byte image stay in 32-bit
// registers, an element touches at most two LDS dwords, and the chunk's LDS image is 5 bytes per element, not 10.
// The same bodies also run with the row's length read from a device word (the job_encode_* kernels): the clerk job's
// payload is queued behind a combine whose dimension the host has not seen yet (sda_clerk_job_dev).
#include "codec_common.h"

namespace sda {

namespace {

constexpr uint32_t kEncChunk = 2048;          // elements per encode block
#ifndef SDA_ENC_EPL
#define SDA_ENC_EPL 2
#endif
constexpr uint32_t kEncEpl = SDA_ENC_EPL;     // write pass: adjacent elements per lane per round (even)
#ifndef SDA_ENC32_CHUNK
#define SDA_ENC32_CHUNK 2048                  // A/B against 4096: DESIGN.md §4.5
#endif
constexpr uint32_t kEnc32Chunk = SDA_ENC32_CHUNK;   // elements per int32 encode block
constexpr uint32_t kEnc32Epl = 4;             // adjacent elements per lane per round: one 16-byte load
static_assert(kEnc32Chunk % (kEnc32Epl * kThreads) == 0 && kEnc32Chunk * 5 / 16 <= kEncChunk * 10 / 16,
              "int32 encode chunk: whole rounds, and an LDS image no larger than the i64 kernel's");
typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// inverse of leb_pack8: 7-bit groups of z -> bytes (group i in byte i), continuation bits not set
__device__ __forceinline__ uint64_t leb_spread8(uint64_t z) {
    uint64_t x = z & 0x00FFFFFFFFFFFFFFull;
    x = (x & 0x000000000FFFFFFFull) | ((x & 0x00FFFFFFF0000000ull) << 4);
    x = (x & 0x00003FFF00003FFFull) | ((x & 0x0FFFC0000FFFC000ull) << 2);
    x = (x & 0x007F007F007F007Full) | ((x & 0x3F803F803F803F80ull) << 1);
    return x;
}

// i64 rows: an element of up to 10 bytes
struct Enc64 {
    typedef int64_t Elem;
    typedef uint64_t Zig;
    typedef i64x2 Vec;                        // the 16-byte load
    typedef uint64_t Acc;                     // a chunk's byte count in the size pass
    static constexpr uint32_t kChunk = kEncChunk, kEpl = kEncEpl;
    static constexpr uint32_t kBufQuads = (kEncChunk * 10 + 32) / 16;      // lead < 16, + the shifted tail dwords
    static __device__ __forceinline__ Zig zigzag(Elem v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }
    static __device__ __forceinline__ uint32_t size(Zig z) {
        const int bits = 64 - __builtin_clzll(z | 1);
        return (uint32_t)((bits + 6) / 7);
    }
    // The element's 8 + 2 bytes shifted to their byte offset: 2-4 ds_or_b32, no per-byte stores.
    static __device__ __forceinline__ void deposit(uint32_t* buf, uint32_t off, Zig z, uint32_t n) {
        // bytes 0..7: groups 0..7, continuation bit on every byte but the element's last;
        // bytes 8, 9 (n > 8): groups 8 and 9
        const uint32_t nc = n - 1;
        const uint64_t cont = nc >= 8 ? 0x8080808080808080ull : (0x8080808080808080ull & ((1ull << (8 * nc)) - 1));
        const uint64_t W = leb_spread8(z) | cont;
        const uint32_t g8 = (uint32_t)(z >> 56) & 0x7Fu, g9 = (uint32_t)(z >> 63);
        const uint32_t E = n > 8 ? (g8 | (n > 9 ? 0x80u : 0u) | (g9 << 8)) : 0u;
        const uint32_t sh = (off & 3) * 8, dw = off >> 2;
        const uint32_t o0 = (uint32_t)W << sh;
        const uint32_t o1 = (uint32_t)(W >> (32 - sh));                          // sh = 0: W's high word
        const uint32_t o2 = (uint32_t)(((((uint64_t)E) << 32) | (uint32_t)(W >> 32)) >> (32 - sh));
        const uint32_t o3 = sh ? E >> (32 - sh) : 0u;
        atomicOr(&buf[dw], o0);                                                  // ds_or_b32
        if (o1) atomicOr(&buf[dw + 1], o1);
        if (o2) atomicOr(&buf[dw + 2], o2);
        if (o3) atomicOr(&buf[dw + 3], o3);
    }
};

// int32 rows: an element of up to 5 bytes
struct Enc32 {
    typedef int32_t Elem;
    typedef uint32_t Zig;
    typedef i32x4 Vec;
    typedef uint32_t Acc;                     // <= 5 * kEnc32Chunk
    static constexpr uint32_t kChunk = kEnc32Chunk, kEpl = kEnc32Epl;
    static constexpr uint32_t kBufQuads = (kEnc32Chunk * 5 + 15 + 15) / 16;     // lead <= 15, rounded up to a quad
    static __device__ __forceinline__ Zig zigzag(Elem v) { return ((uint32_t)v << 1) ^ (uint32_t)(v >> 31); }
    static __device__ __forceinline__ uint32_t size(Zig z) { return (uint32_t)(32 - __builtin_clz(z | 1) + 6) / 7; }
    // Groups 0..3 spread into one dword, group 4 in a fifth byte; the 40 bits shifted to the byte offset are one
    // or two ds_or_b32.  A dword past the element's last byte is never touched (o1 == 0 is skipped).
    static __device__ __forceinline__ void deposit(uint32_t* buf, uint32_t off, Zig zz, uint32_t n) {
        // bytes 0..3: groups 0..3, continuation bit on every byte but the element's last; byte 4: group 4
        uint32_t x = zz & 0x0FFFFFFFu;
        x = (x & 0x00003FFFu) | ((x & 0x0FFFC000u) << 2);
        x = (x & 0x007F007Fu) | ((x & 0x3F803F80u) << 1);
        const uint32_t nc = n - 1;
        const uint32_t lo = x | (nc >= 4 ? 0x80808080u : (0x80808080u & ((1u << (8 * nc)) - 1)));
        const uint32_t hi = zz >> 28;                                // 0 unless n == 5
        const uint32_t sh = (off & 3) * 8, dw = off >> 2;
        const uint32_t o0 = lo << sh;
        const uint32_t o1 = sh ? __builtin_amdgcn_alignbit(hi, lo, 32 - sh) : hi;
        atomicOr(&buf[dw], o0);                                      // ds_or_b32
        if (o1) atomicOr(&buf[dw + 1], o1);
    }
};

// A full chunk whose first element is 16-byte aligned is read with one 16-byte load per lane (a wave moves 1 KiB
// per load instruction).  A row of int32 starts 0, 4, 8 or 12 bytes off a 16-byte boundary (stride and base are
// only 4-byte aligned), and every chunk of the row shares that offset (the chunk is a multiple of 4 elements):
// only offset 0 takes the 16-byte loads.  So the row's own alignment is tested, which is every chunk's.
template <class Tr>
__device__ __forceinline__ bool enc_vec_ok(const typename Tr::Elem* rowp, uint64_t e0, uint64_t len) {
    static_assert(Tr::kChunk * sizeof(typename Tr::Elem) % 16 == 0, "a chunk is a whole number of 16-byte loads");
    return e0 + Tr::kChunk <= len && ((uintptr_t)rowp & 15) == 0;
}

// sizes of each [row][chunk] block of elements
template <class Tr>
__device__ __forceinline__ void varint_size_body(const typename Tr::Elem* __restrict__ vals, uint64_t len,
                                                 uint64_t stride, uint32_t chunks,
                                                 uint64_t* __restrict__ chunk_bytes) {
    typedef typename Tr::Vec Vec;
    typedef typename Tr::Acc Acc;
    constexpr uint32_t kVec = sizeof(Vec) / sizeof(typename Tr::Elem);     // elements per 16-byte load
    const uint32_t c = blockIdx.x, row = blockIdx.y;
    const uint64_t e0 = (uint64_t)c * Tr::kChunk;
    const typename Tr::Elem* rowp = vals + (uint64_t)row * stride;
    Acc n = 0;
    if (enc_vec_ok<Tr>(rowp, e0, len)) {        // 16-byte loads (order is irrelevant here)
#pragma unroll
        for (uint32_t q = 0; q < Tr::kChunk / (kVec * kThreads); ++q) {
            const Vec x = __builtin_nontemporal_load(reinterpret_cast<const Vec*>(rowp + e0) + q * kThreads + threadIdx.x);
#pragma unroll
            for (uint32_t j = 0; j < kVec; ++j) n += Tr::size(Tr::zigzag(x[j]));
        }
    } else {
#pragma unroll
        for (uint32_t q = 0; q < Tr::kChunk / kThreads; ++q) {
            const uint64_t e = e0 + q * kThreads + threadIdx.x;
            if (e < len) n += Tr::size(Tr::zigzag(rowp[e]));
        }
    }
    __shared__ Acc red[kThreads / 64];
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        Acc s = 0;
        for (int i = 0; i < kThreads / 64; ++i) s += red[i];
        chunk_bytes[(uint64_t)row * chunks + c] = s;
    }
}

// write: rounds of coalesced loads (round q: lane t owns the kEpl adjacent elements e0 + R q + kEpl t + j,
// R = kEpl * 256; 16-byte loads when the chunk allows it), one block-wide scan of the lane sizes per round, each
// element's bytes ORed into a zeroed LDS image of the chunk's output (Tr::deposit), the image aligned to the
// chunk's global byte offset mod 16 so that the interior leaves as 16-byte stores; the two partial 16-byte words
// at the ends (shared with the neighbouring chunks) are written byte-wise.
// Chunk (c, row) starts at dst + row_base[row] + chunk_off (the exclusive scan of the row's chunk_bytes);
// nothing is written when *too_big (the rows do not fit dst_cap).
template <class Tr, bool NT>
__device__ __forceinline__ void varint_write_body(const typename Tr::Elem* __restrict__ vals, uint64_t len,
                                                  uint64_t stride, uint32_t chunks,
                                                  const uint64_t* __restrict__ chunk_off,
                                                  const uint64_t* __restrict__ row_base,
                                                  const uint32_t* __restrict__ too_big, uint8_t* __restrict__ dst) {
    typedef typename Tr::Vec Vec;
    constexpr uint32_t kVec = sizeof(Vec) / sizeof(typename Tr::Elem), kEpl = Tr::kEpl;
    constexpr uint32_t kRounds = Tr::kChunk / (kEpl * kThreads);
    const uint32_t c = blockIdx.x, row = blockIdx.y;
    if (*too_big) return;
    const uint64_t e0 = (uint64_t)c * Tr::kChunk;
    __shared__ uint4 buf4[Tr::kBufQuads];
    __shared__ uint32_t wsum[kThreads / 64];
    uint32_t* buf = reinterpret_cast<uint32_t*>(buf4);
    const uint8_t* b8 = reinterpret_cast<const uint8_t*>(buf4);
    uint8_t* gdst = dst + row_base[row] + chunk_off[(uint64_t)row * chunks + c];
    const uint32_t lead = (uint32_t)((uintptr_t)gdst & 15);
    for (uint32_t k = threadIdx.x; k < Tr::kBufQuads; k += kThreads) buf4[k] = make_uint4(0, 0, 0, 0);
    const typename Tr::Elem* rowp = vals + (uint64_t)row * stride;
    typename Tr::Zig z[kRounds][kEpl];
    if (enc_vec_ok<Tr>(rowp, e0, len)) {
#pragma unroll
        for (uint32_t q = 0; q < kRounds; ++q)
#pragma unroll
            for (uint32_t j = 0; j < kEpl / kVec; ++j) {
                const Vec x = __builtin_nontemporal_load(
                    reinterpret_cast<const Vec*>(rowp + e0 + kEpl * (q * kThreads + threadIdx.x)) + j);
#pragma unroll
                for (uint32_t i = 0; i < kVec; ++i) z[q][kVec * j + i] = Tr::zigzag(x[i]);
            }
    } else {
#pragma unroll
        for (uint32_t q = 0; q < kRounds; ++q)
#pragma unroll
            for (uint32_t j = 0; j < kEpl; ++j) {
                const uint64_t e = e0 + kEpl * (q * kThreads + threadIdx.x) + j;
                // only the load under the lane branch: a zigzag there would wait for each load in turn
                z[q][j] = Tr::zigzag(e < len ? rowp[e] : 0);
            }
    }
    uint32_t base = lead;
#pragma unroll
    for (uint32_t q = 0; q < kRounds; ++q) {
        const uint64_t e = e0 + kEpl * (q * kThreads + threadIdx.x);
        uint32_t ns[kEpl], pre[kEpl], np = 0;
#pragma unroll
        for (uint32_t j = 0; j < kEpl; ++j) {
            ns[j] = e + j < len ? Tr::size(z[q][j]) : 0u;
            pre[j] = np;
            np += ns[j];
        }
        const uint32_t incl = wave_incl_scan(np);
        __syncthreads();                                     // wsum of the previous q consumed (and, at
        if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;    // q = 0, the zeroed image visible)
        __syncthreads();
        uint32_t off0 = base + incl - np, total = 0;
        for (uint32_t w = 0; w < kThreads / 64; ++w) {
            if (w < (threadIdx.x >> 6)) off0 += wsum[w];
            total += wsum[w];
        }
        base += total;
#pragma unroll
        for (uint32_t h = 0; h < kEpl; ++h)
            if (ns[h]) Tr::deposit(buf, off0 + pre[h], z[q][h], ns[h]);
    }
    __syncthreads();
    const uint32_t end = base;                               // lead + chunk bytes
    uint4* d128 = reinterpret_cast<uint4*>(gdst - lead);
    uint8_t* d8 = gdst - lead;
    const uint32_t nq = (end + 15) / 16;
    for (uint32_t k = threadIdx.x; k < nq; k += kThreads) {
        const uint32_t lo = k * 16, hi = lo + 16;
        if (lo >= lead && hi <= end) {
            if constexpr (NT)
                __builtin_nontemporal_store(reinterpret_cast<const u32x4*>(buf4)[k], reinterpret_cast<u32x4*>(d128) + k);
            else d128[k] = buf4[k];
        } else {
            for (uint32_t i = lo; i < hi; ++i)
                if (i >= lead && i < end) d8[i] = b8[i];
        }
    }
}

__global__ __launch_bounds__(kThreads) void varint_size_kernel(const int64_t* __restrict__ vals, uint64_t len,
                                                               uint64_t stride, uint32_t chunks,
                                                               uint64_t* __restrict__ chunk_bytes) {
    varint_size_body<Enc64>(vals, len, stride, chunks, chunk_bytes);
}
__global__ __launch_bounds__(kThreads) void varint_size32_kernel(const int32_t* __restrict__ vals, uint64_t len,
                                                                 uint64_t stride, uint32_t chunks,
                                                                 uint64_t* __restrict__ chunk_bytes) {
    varint_size_body<Enc32>(vals, len, stride, chunks, chunk_bytes);
}
template <bool NT>
__global__ __launch_bounds__(kThreads) void varint_write_kernel(const int64_t* __restrict__ vals, uint64_t len,
                                                                uint64_t stride, uint32_t chunks,
                                                                const uint64_t* __restrict__ chunk_off,
                                                                const uint64_t* __restrict__ row_base,
                                                                const uint32_t* __restrict__ too_big,
                                                                uint8_t* __restrict__ dst) {
    varint_write_body<Enc64, NT>(vals, len, stride, chunks, chunk_off, row_base, too_big, dst);
}
template <bool NT>
__global__ __launch_bounds__(kThreads) void varint_write32_kernel(const int32_t* __restrict__ vals, uint64_t len,
                                                                  uint64_t stride, uint32_t chunks,
                                                                  const uint64_t* __restrict__ chunk_off,
                                                                  const uint64_t* __restrict__ row_base,
                                                                  const uint32_t* __restrict__ too_big,
                                                                  uint8_t* __restrict__ dst) {
    varint_write_body<Enc32, NT>(vals, len, stride, chunks, chunk_off, row_base, too_big, dst);
}

// exclusive scan of chunk_bytes per row (one block per row) + row base; row_bytes = total
// One workgroup: rows placed back to back -- row_base = exclusive scan of row_bytes; *too_big = the total
// exceeds cap (the write pass then writes nothing and the host reports it).
__device__ __forceinline__ void varint_rows_body(const uint64_t* __restrict__ row_bytes, uint64_t rows, uint64_t cap,
                                                 uint64_t* __restrict__ row_base, uint32_t* __restrict__ too_big) {
    __shared__ uint64_t part[kThreads];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < rows; base += kThreads) {
        const uint64_t r = base + threadIdx.x;
        const uint64_t v = r < rows ? row_bytes[r] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < kThreads; o <<= 1) {
            const uint64_t add = threadIdx.x >= (uint32_t)o ? part[threadIdx.x - o] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (r < rows) row_base[r] = carry + part[threadIdx.x] - v;
        carry += part[kThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *too_big = carry > cap ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void varint_rows_kernel(const uint64_t* __restrict__ row_bytes, uint64_t rows,
                                                               uint64_t cap, uint64_t* __restrict__ row_base,
                                                               uint32_t* __restrict__ too_big) {
    varint_rows_body(row_bytes, rows, cap, row_base, too_big);
}

__device__ __forceinline__ void varint_offsets_body(const uint64_t* __restrict__ chunk_bytes, uint32_t chunks,
                                                    const uint64_t* __restrict__ row_base,
                                                    uint64_t* __restrict__ chunk_off, uint64_t* __restrict__ row_bytes) {
    const uint32_t row = blockIdx.x;
    __shared__ uint64_t part[kThreads];
    uint64_t carry = row_base ? row_base[row] : 0, total = 0;
    for (uint32_t base = 0; base < chunks; base += kThreads) {
        const uint32_t c = base + threadIdx.x;
        const uint64_t v = c < chunks ? chunk_bytes[(uint64_t)row * chunks + c] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < kThreads; o <<= 1) {
            const uint64_t add = threadIdx.x >= (uint32_t)o ? part[threadIdx.x - o] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (c < chunks) chunk_off[(uint64_t)row * chunks + c] = carry + part[threadIdx.x] - v;
        carry += part[kThreads - 1];
        total += part[kThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0 && row_bytes) row_bytes[row] = total;
}
__global__ __launch_bounds__(kThreads) void varint_offsets_kernel(const uint64_t* __restrict__ chunk_bytes,
                                                                  uint32_t chunks, const uint64_t* __restrict__ row_base,
                                                                  uint64_t* __restrict__ chunk_off,
                                                                  uint64_t* __restrict__ row_bytes) {
    varint_offsets_body(chunk_bytes, chunks, row_base, chunk_off, row_bytes);
}

// ---- the length on the device (sda_clerk_job_dev: the encode queued behind a combine whose dimension the host has
// not seen).  The row's length is a device word, valid only while the job's flag word is clear and the length fits
// the row's capacity; otherwise every pass exits without a store.  The grids and the workspace follow the host's
// bound on the length: a chunk at or past the real length reports 0 bytes and its write pass stores nothing.
struct DevLen {
    const uint64_t* len;       // the row's element count
    const uint32_t* flags;     // the job's flag word: nonzero = no result
    uint64_t cap;              // elements the row can hold
    __device__ __forceinline__ bool get(uint64_t* n) const {
        if (*flags) return false;
        *n = *len;
        return *n <= cap;
    }
};
__global__ __launch_bounds__(kThreads) void job_encode_size_kernel(const int64_t* __restrict__ vals, DevLen dl,
                                                                      uint32_t chunks,
                                                                      uint64_t* __restrict__ chunk_bytes) {
    uint64_t len;
    if (!dl.get(&len)) return;
    varint_size_body<Enc64>(vals, len, len, chunks, chunk_bytes);
}
__global__ __launch_bounds__(kThreads) void job_encode_offsets_kernel(const uint64_t* __restrict__ chunk_bytes,
                                                                         DevLen dl, uint32_t chunks,
                                                                         uint64_t* __restrict__ chunk_off,
                                                                         uint64_t* __restrict__ row_bytes) {
    uint64_t len;
    if (!dl.get(&len)) return;
    varint_offsets_body(chunk_bytes, chunks, nullptr, chunk_off, row_bytes);
}
// *total = the payload's bytes, next to the job's flag word for the call's one copy
__global__ __launch_bounds__(kThreads) void job_encode_rows_kernel(const uint64_t* __restrict__ row_bytes, DevLen dl,
                                                                      uint64_t cap, uint64_t* __restrict__ row_base,
                                                                      uint32_t* __restrict__ too_big,
                                                                      uint64_t* __restrict__ total) {
    uint64_t len;
    if (!dl.get(&len)) return;
    varint_rows_body(row_bytes, 1, cap, row_base, too_big);
    if (threadIdx.x == 0) *total = row_bytes[0];
}
template <bool NT>
__global__ __launch_bounds__(kThreads) void job_encode_write_kernel(const int64_t* __restrict__ vals, DevLen dl,
                                                                       uint32_t chunks,
                                                                       const uint64_t* __restrict__ chunk_off,
                                                                       const uint64_t* __restrict__ row_base,
                                                                       const uint32_t* __restrict__ too_big,
                                                                       uint8_t* __restrict__ dst) {
    uint64_t len;
    if (!dl.get(&len) || (uint64_t)blockIdx.x * Enc64::kChunk >= len) return;
    varint_write_body<Enc64, NT>(vals, len, len, chunks, chunk_off, row_base, too_big, dst);
}

}  // namespace

// Layout of the device workspace for the encode passes: [chunk_bytes | chunk_off] per (row, chunk), then
// [row_base | row_bytes] per row, then the flag.
struct EncodeWork {
    uint64_t* chunk_bytes; uint64_t* chunk_off; uint64_t* row_base; uint64_t* row_bytes; uint32_t* too_big;
};
static EncodeWork carve_encode(void* work, uint64_t rows, uint64_t chunks) {
    EncodeWork w;
    w.chunk_bytes = static_cast<uint64_t*>(work);
    w.chunk_off = w.chunk_bytes + rows * chunks;
    w.row_base = w.chunk_off + rows * chunks;
    w.row_bytes = w.row_base + rows;
    w.too_big = reinterpret_cast<uint32_t*>(w.row_bytes + rows);
    return w;
}
static size_t encode_work_bytes(uint64_t rows, uint64_t len, uint32_t chunk) {
    const uint64_t chunks = (len + chunk - 1) / chunk;
    return 2 * rows * (chunks ? chunks : 1) * 8 + 2 * rows * 8 + 1024 + 256;
}
size_t varint_encode_work_bytes(uint64_t rows, uint64_t len) { return encode_work_bytes(rows, len, kEncChunk); }
size_t varint_encode32_work_bytes(uint64_t rows, uint64_t len) { return encode_work_bytes(rows, len, kEnc32Chunk); }

// size -> offsets -> rows -> write (Tr's kernels), then the call's one wait: the row sizes' copy.
template <class Tr, class SizeKernel, class WriteKernel>
static hipError_t launch_encode(SizeKernel size_kernel, WriteKernel write_nt, WriteKernel write_cached,
                                const typename Tr::Elem* vals, uint64_t rows, uint64_t len, uint64_t stride,
                                uint8_t* dst, uint64_t dst_cap, void* work, uint64_t* row_bytes_host, hipStream_t s) {
    const uint64_t chunks = (len + Tr::kChunk - 1) / Tr::kChunk;
    if (rows == 0) return hipSuccess;
    if (chunks == 0) {
        for (uint64_t r = 0; r < rows; ++r) row_bytes_host[r] = 0;
        return hipSuccess;
    }
    const EncodeWork w = carve_encode(work, rows, chunks);
    const dim3 grid((unsigned)chunks, (unsigned)rows), block(kThreads);
    hipError_t e;
    hipLaunchKernelGGL(size_kernel, grid, block, 0, s, vals, len, stride, (uint32_t)chunks, w.chunk_bytes);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // per row: its chunks' offsets and its total; then the rows back to back -- all on the device, so the
    // only host wait is the row sizes' copy at the end
    hipLaunchKernelGGL(varint_offsets_kernel, dim3((unsigned)rows), block, 0, s, (const uint64_t*)w.chunk_bytes,
                       (uint32_t)chunks, (const uint64_t*)nullptr, w.chunk_off, w.row_bytes);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(varint_rows_kernel, dim3(1), block, 0, s, (const uint64_t*)w.row_bytes, rows, dst_cap,
                       w.row_base, w.too_big);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // nontemporal payload stores: encode -5.5 % in-process (3.770 -> 3.563 ms at 1000 x 1M, profiles/r06ad);
    // SDA_ENC_NT=0 (read per call) keeps cached stores for A/B
    const char* nt = getenv("SDA_ENC_NT");
    hipLaunchKernelGGL(nt && nt[0] == '0' ? write_cached : write_nt, grid, block, 0, s, vals, len, stride,
                       (uint32_t)chunks, (const uint64_t*)w.chunk_off, (const uint64_t*)w.row_base,
                       (const uint32_t*)w.too_big, dst);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(row_bytes_host, w.row_bytes, rows * 8, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    uint64_t acc = 0;
    for (uint64_t r = 0; r < rows; ++r) acc += row_bytes_host[r];
    return acc > dst_cap ? hipErrorInvalidValue : hipSuccess;     // nothing was written (too_big)
}

hipError_t launch_varint_encode(const int64_t* vals, uint64_t rows, uint64_t len, uint64_t stride, uint8_t* dst,
                                uint64_t dst_cap, void* work, uint64_t* row_bytes_host, hipStream_t s) {
    return launch_encode<Enc64>(varint_size_kernel, varint_write_kernel<true>, varint_write_kernel<false>, vals, rows,
                                len, stride, dst, dst_cap, work, row_bytes_host, s);
}

// The same from int32 rows: the same work-buffer layout with chunks of kEnc32Chunk elements.
hipError_t launch_varint_encode32(const int32_t* vals, uint64_t rows, uint64_t len, uint64_t stride, uint8_t* dst,
                                  uint64_t dst_cap, void* work, uint64_t* row_bytes_host, hipStream_t s) {
    return launch_encode<Enc32>(varint_size32_kernel, varint_write32_kernel<true>, varint_write32_kernel<false>, vals,
                                rows, len, stride, dst, dst_cap, work, row_bytes_host, s);
}

// One i64 row whose length is the device word *len_dev (sda_clerk_job_dev): size -> offsets -> rows -> write, only
// queued.  bound >= the length the word can hold when the job is clean (the grids and `work`,
// varint_encode_work_bytes(1, bound) bytes); *total_dev gets the payload's bytes unless the job's flag word is set
// or the length exceeds vals_cap, and nothing is written to dst when they exceed dst_cap.
hipError_t launch_varint_encode_devlen(const int64_t* vals, uint64_t vals_cap, const uint64_t* len_dev,
                                       const uint32_t* flags_dev, uint64_t bound, uint8_t* dst, uint64_t dst_cap,
                                       void* work, uint64_t* total_dev, hipStream_t s, uint64_t* chunks_out) {
    const uint64_t chunks = (bound + kEncChunk - 1) / kEncChunk;
    if (chunks_out) *chunks_out = chunks;
    if (chunks == 0) return hipSuccess;
    if (chunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const EncodeWork w = carve_encode(work, 1, chunks);
    const DevLen dl = {len_dev, flags_dev, vals_cap};
    const dim3 grid((unsigned)chunks), block(kThreads);
    hipError_t e;
    hipLaunchKernelGGL(job_encode_size_kernel, grid, block, 0, s, vals, dl, (uint32_t)chunks, w.chunk_bytes);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(job_encode_offsets_kernel, dim3(1), block, 0, s, (const uint64_t*)w.chunk_bytes, dl,
                       (uint32_t)chunks, w.chunk_off, w.row_bytes);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(job_encode_rows_kernel, dim3(1), block, 0, s, (const uint64_t*)w.row_bytes, dl, dst_cap,
                       w.row_base, w.too_big, total_dev);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const char* nt = getenv("SDA_ENC_NT");                          // as launch_encode
    hipLaunchKernelGGL(nt && nt[0] == '0' ? job_encode_write_kernel<false> : job_encode_write_kernel<true>, grid,
                       block, 0, s, vals, dl, (uint32_t)chunks, (const uint64_t*)w.chunk_off,
                       (const uint64_t*)w.row_base, (const uint32_t*)w.too_big, dst);
    return hipGetLastError();
}
uint64_t varint_encode_chunks(uint64_t len) { return (len + kEncChunk - 1) / kEncChunk; }

}  // namespace sda
