// recipient_repair.hip -- the decoded reveal's first pass inside the recipient job (sda_recipient_job_decoded and its
// device forms): packed_repair.hip's fused check + basis reveal over i64 clerk rows, with the recipient's unmask and
// positive() taken in the same write-back.
//
// Where the masking modulus and the output modulus are both the sharing prime p, positive(unmask(secret)) is the one
// residue (secret - mask) mod p in [0, p).  The first pass has the k secrets of its 256 batches parked in LDS for the
// coalesced write-back, so the mask is subtracted there: one more 8- or 16-byte load per store, and no separate pass
// that reads 16 D bytes and writes 8 D.  The decode pass behind it (packed_decode.hip) reads out[e] as a residue and
// subtracts lam[e][j-1] err_j mod p, which commutes with the mask's subtraction, so it runs as it is.
#include "check_launch.h"
#include "repair_body.h"
#include "repair_plan.h"

namespace sda {
using namespace packed;

namespace {

template <int NMAX>
__global__ __launch_bounds__(256) void recipient_repair_kernel(const int64_t* __restrict__ shares, uint64_t B,
                                                               uint64_t D, int64_t* __restrict__ out,
                                                               const int64_t* __restrict__ mask, uint32_t n_idx,
                                                               uint32_t kt, uint32_t k,
                                                               const uint32_t* __restrict__ tab, uint32_t ks, MontP M,
                                                               uint16_t* __restrict__ verdict,
                                                               unsigned long long* __restrict__ cnt, uint32_t cap) {
    extern __shared__ int64_t lds_o[];
    const FlushSubMask epi{mask + (uint64_t)blockIdx.y * D, M};
    repair_body<int64_t, NMAX>(shares, B, D, out, n_idx, kt, k, tab, ks, M, verdict, cnt, cap, lds_o, epi);
}

// The same residue as a pass of its own (the unfused route): out[i] = (secrets[i] - mask[i]) mod p, secrets in [0, p).
__global__ __launch_bounds__(256) void recipient_unmask_kernel(const int64_t* __restrict__ secrets,
                                                               const int64_t* __restrict__ mask, uint64_t D, MontP M,
                                                               int64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D) return;
    const FlushSubMask epi{mask, M};
    out[i] = epi.sub(secrets[i], mask[i]);
}

}  // namespace

hipError_t launch_recipient_repair(const PackedRepairArgs& a, const int64_t* mask, const CheckGeom& g, hipStream_t s,
                                   PackedCheckResult* res) {
    const PackedRepairPlan pl = packed_repair_plan(g.n_idx, g.k, g.kt - g.k);
    if (pl.path != kRepairFused || !a.shares || a.shares32 || !mask) return hipErrorInvalidValue;
    *res = PackedCheckResult{};
    res->launched = true;
    const dim3 grid((unsigned)((g.B + 255) / 256), (unsigned)a.n_vectors);
    const size_t lds = (size_t)256 * g.k * sizeof(int64_t);
    return first_pass(g, s, [&] {
        return with_bucket(pl.bucket, [&](auto nmax) {
            hipLaunchKernelGGL(recipient_repair_kernel<nmax>, grid, dim3(256), lds, s, a.shares, g.B, g.D, a.out, mask,
                               g.n_idx, g.kt, g.k, g.tab, g.ks, g.M, a.verdict, g.cnt, g.cap);
        });
    }, res);
}

hipError_t launch_recipient_unmask(const int64_t* secrets, const int64_t* mask, uint64_t D, const MontP& M,
                                   int64_t* out, hipStream_t s) {
    if (D == 0) return hipSuccess;
    hipLaunchKernelGGL(recipient_unmask_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, s, secrets, mask, D, M,
                       out);
    return hipGetLastError();
}

}  // namespace sda
