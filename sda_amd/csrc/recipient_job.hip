// recipient_job.hip -- the recipient's ChaCha seed payloads (sda_recipient_job / sda_recipient_job_dev).
//
//   client/src/receive.rs:101-117  every mask blob is opened and decoded (Decryptor::decrypt, sodium.rs:82-90)
//   client/src/crypto/masking/chacha.rs:62-64  seed.iter().map(|&x| x as u32) feeds ChaChaRng::from_seed, whose
//     key is the first 8 words, zero padded
//
// A seed blob is a handful of varints (seed_bitsize / 32 of them), so a 16 KiB decode region per blob would be all
// overhead: one lane walks one blob by the codec's rules (codec_decode.hip's sequential walk: zigzag + LEB128, a run
// of >= 11 continuation bytes forms one element, a truncated last varint yields its partial value), stops after the
// 8 values the key can hold and stores them `as u32`, zero padded, as the [n_seeds][8] matrix the ChaCha mask
// combine takes with w = 8 (pack_seeds: a shorter seed is its zero-padded key).
#include "kernels.h"

namespace sda {

namespace {

constexpr uint32_t kThreads = 256;

__global__ __launch_bounds__(kThreads) void recipient_seed_kernel(const uint8_t* __restrict__ bytes,
                                                                  const uint64_t* __restrict__ blob_off,
                                                                  uint64_t n_seeds, uint32_t* __restrict__ words) {
    const uint64_t b = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (b >= n_seeds) return;
    uint64_t r = blob_off[b];
    const uint64_t e = blob_off[b + 1];
    uint32_t key[kSeedWords];
#pragma unroll
    for (uint32_t c = 0; c < kSeedWords; ++c) {       // unrolled: key[] stays in registers
        uint32_t v = 0;
        if (r < e) {
            uint64_t z = 0;
            unsigned shift = 0;
            while (r < e) {
                const uint8_t by = bytes[r++];
                z |= (uint64_t)(by & 0x7f) << (shift & 63);
                shift += 7;
                if (!(by & 0x80) || shift > 70) break;
            }
            v = (uint32_t)((z >> 1) ^ (0 - (z & 1)));   // zigzag, then `as u32`
        }
        key[c] = v;
    }
    uint4* dst = reinterpret_cast<uint4*>(words + b * kSeedWords);
    dst[0] = make_uint4(key[0], key[1], key[2], key[3]);
    dst[1] = make_uint4(key[4], key[5], key[6], key[7]);
}

}  // namespace

hipError_t launch_recipient_seeds(const uint8_t* bytes, const uint64_t* blob_off_host, uint64_t n_seeds,
                                  uint64_t* blob_off_dev, uint32_t* words, hipStream_t s) {
    if (n_seeds == 0) return hipSuccess;
    const uint64_t grid = (n_seeds + kThreads - 1) / kThreads;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = hipMemcpyAsync(blob_off_dev, blob_off_host, (n_seeds + 1) * 8, hipMemcpyHostToDevice, s)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(recipient_seed_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, bytes,
                       (const uint64_t*)blob_off_dev, n_seeds, words);
    return hipGetLastError();
}

}  // namespace sda
