// packed_decode.hip -- decoded reveal: the decode pass of sda_packed_reveal_decoded_dev, which corrects up to
// e_max = r / 2 wrong clerk shares per batch (r = n_idx - (k + t), the redundancy).
//
// The call's first pass is the checked reveal's fused kernel (packed_repair.hip): out holds the reveal of every batch
// from its first kt = k + t shares, the bad batches are counted and logged.  packed_decode_kernel then walks the
// logged batches, one lane per batch (with `all`, the log overflowed, every batch of the call).  A lane
//   reads the batch's n_idx residues and forms RMAX power-sum syndromes against the decode table (decode_tables.h;
//     one row of RMAX words per position, the words for syndromes r .. RMAX - 1 zero),
//   runs decode_core.h's decoder: Berlekamp-Massey, the root search over the clerk positions, Forney,
//   and for a decoded batch with error set E takes  out[e] -= lam[e][j-1] err_j  for every j in E with j <= kt, the
//     checked reveal's correction summed over E (lam: the basis Lagrange rows of ensure_check_table's table).  Wrong
//     shares among the check positions leave the basis reveal right as it stands.
// verdict = |E| and wrong = the bits of E go to the caller's buffers; an undecodable batch keeps the first pass's
// 0xFFFF and its reveal from the first kt shares.  Point 0, the inserted (1, 0), is not among the positions searched:
// a word whose nearest codeword disagrees with it has a root there, comes up one root short and is undecodable.
//
// Counters (check_common.h's block): [2] batches whose out was rewritten, [3] undecodable batches, blame word
// kDecodeMaxErrWord the largest |E|; blame[j-1] counts the batches whose E holds j.  A wave keeps its blame counts in
// registers (lane j - 1 holds position j's) across its batches and adds them once at the end: with whole wrong rows
// every batch adds to the same few words.
#include "check_launch.h"
#include "decode_core.h"
#include "decode_plan.h"
#include "decode_tables.h"

namespace sda {
using namespace packed;

namespace {

// no clerk position has blame word 1023 (at most kRevealMaxShares = 1023 shares), and first_pass zeroes it
constexpr uint32_t kDecodeMaxErrWord = kCheckHdr + kCheckBlameCap - 1;
static_assert(kRevealMaxShares <= kCheckBlameCap - 1, "the last blame word is free");

template <class ST, int RMAX>
__device__ __forceinline__ void decode_body(const ST* __restrict__ shares, uint64_t B, uint64_t D,
                                            int64_t* __restrict__ out, uint32_t n_idx, uint32_t kt, uint32_t k,
                                            const uint32_t* __restrict__ lam, uint32_t ks,
                                            const uint32_t* __restrict__ dtab, const MontP& M,
                                            uint16_t* __restrict__ verdict, uint32_t* __restrict__ wrong,
                                            unsigned long long* __restrict__ cnt, uint64_t total, int all) {
    const uint32_t p = M.p, r = n_idx - kt, e_max = r / 2;
    const int64_t P = (int64_t)p;
    const Mod64 PM = make_mod64(P);
    const decode::MontField F0 = decode::make_field(p, M.pinv, M.r2);
    const unsigned long long* list = cnt + kCheckHdr + kCheckBlameCap;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t basis_bits = (1u << kt) - 1u;           // kt <= n_idx - 2 <= 30
    uint32_t my_blame = 0, fixed = 0, undecoded = 0, max_err = 0;
    // wave-uniform trip count: every lane of a wave reaches the ballots
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < total; i0 += stride) {
        const uint64_t i = i0 + lane;
        uint32_t mask = 0;
        if (i < total) {
            const uint64_t gb = all ? i : list[i];
            const uint64_t vec = gb / B, b = gb - vec * B;
            const ST* sh = shares + vec * (uint64_t)n_idx * B + b;
            decode::Decoder<decode::MontField, RMAX> dec;
            static_for<0, RMAX>([&](auto c) { dec.S[c] = 0; });
            // The table is read with vector loads (every lane the same address, a row's RMAX words 16-byte aligned:
            // a broadcast): as uniform loads a row would hold RMAX scalar registers, and the kernel spills them.
            const uint32_t* dvec = dtab;
            asm volatile("" : "+v"(dvec));
            const uint32_t* xinv = dvec + (size_t)RMAX * n_idx;
            const uint32_t* xs = xinv + n_idx;
            const uint32_t* vinv = xs + n_idx;
            for (uint32_t j = 0; j < n_idx; ++j) {
                const uint32_t y = canon_any(sh[(uint64_t)j * B], p, P, PM);
                const uint32_t* row = static_cast<const uint32_t*>(__builtin_assume_aligned(dvec + (size_t)j * RMAX, 16));
                static_for<0, RMAX>([&](auto c) {
                    dec.S[c] = addm(dec.S[c], mont_mul(row[c], y, M), p);
                });
            }
            uint32_t nz = 0;
            static_for<0, RMAX>([&](auto c) { nz |= dec.S[c]; });
            if (nz) {                                       // consistent batches are only met on a full walk
                // r and the field's one as per-batch vector values: left uniform, the unrolled steps' `i < r` tests
                // are hoisted out of the batch loop as RMAX lane masks and the first steps run on scalar registers,
                // and both spill SGPRs
                uint32_t rv, onev;
                asm volatile("v_mov_b32 %0, %1" : "=v"(rv) : "s"(r));
                asm volatile("v_mov_b32 %0, %1" : "=v"(onev) : "s"(F0.r1));
                const decode::MontField F{p, M.pinv, M.r2, onev};
                static_for<0, RMAX>([&](auto c) { dec.S[c] = F.enter(dec.S[c]); });
                const uint32_t nu = dec.locator(F, rv);
                uint32_t roots = 0;
                if (nu <= e_max)
                    for (uint32_t j = 0; j < n_idx; ++j)
                        if (dec.locator_at(F, xinv[j]) == 0) { mask |= 1u << j; ++roots; }
                if (nu > e_max || roots != nu) {
                    mask = 0;
                    ++undecoded;
                } else {
                    const uint32_t lim = b * k < D ? (uint32_t)(D - b * k < k ? D - b * k : k) : 0u;
                    int64_t* dst = out + vec * D + b * k;
                    uint32_t todo = mask & basis_bits;
                    if (todo) {
                        dec.evaluator(F, nu);
                        ++fixed;
                    }
                    while (todo) {
                        const uint32_t j = (uint32_t)__ffs((int)todo) - 1;
                        todo &= todo - 1;
                        const uint32_t err = F.leave(dec.error_value(F, p, xs[j], xinv[j], vinv[j]));
                        for (uint32_t e = 0; e < lim; ++e)
                            dst[e] = (int64_t)subm((uint32_t)dst[e], mont_mul(lam[(size_t)e * ks + j], err, M), p);
                    }
                    if (verdict) verdict[gb] = (uint16_t)nu;
                    if (wrong) wrong[gb] = mask;
                    max_err = max(max_err, nu);
                }
            }
        }
        for (uint32_t j = 0; j < n_idx; ++j) {
            const uint64_t hit = __ballot((mask >> j) & 1u);
            if (lane == j) my_blame += (uint32_t)__popcll((unsigned long long)hit);
        }
    }
    if (lane < n_idx && my_blame) atomicAdd(cnt + kCheckHdr + lane, (unsigned long long)my_blame);
    for (int off = 32; off; off >>= 1) {
        fixed += (uint32_t)__shfl_xor((int)fixed, off);
        undecoded += (uint32_t)__shfl_xor((int)undecoded, off);
        max_err = max(max_err, (uint32_t)__shfl_xor((int)max_err, off));
    }
    if (lane == 0) {
        if (fixed) atomicAdd(cnt + 2, (unsigned long long)fixed);
        if (undecoded) atomicAdd(cnt + 3, (unsigned long long)undecoded);
        if (max_err) atomicMax(cnt + kDecodeMaxErrWord, (unsigned long long)max_err);
    }
}

template <int RMAX>
__global__ __launch_bounds__(256) void packed_decode_kernel(const int64_t* __restrict__ shares, uint64_t B, uint64_t D,
                                                            int64_t* __restrict__ out, uint32_t n_idx, uint32_t kt,
                                                            uint32_t k, const uint32_t* __restrict__ lam, uint32_t ks,
                                                            const uint32_t* __restrict__ dtab, MontP M,
                                                            uint16_t* __restrict__ verdict,
                                                            uint32_t* __restrict__ wrong,
                                                            unsigned long long* __restrict__ cnt, uint64_t total,
                                                            int all) {
    decode_body<int64_t, RMAX>(shares, B, D, out, n_idx, kt, k, lam, ks, dtab, M, verdict, wrong, cnt, total, all);
}

template <int RMAX>
__global__ __launch_bounds__(256) void packed_decode32_kernel(const int32_t* __restrict__ shares, uint64_t B,
                                                              uint64_t D, int64_t* __restrict__ out, uint32_t n_idx,
                                                              uint32_t kt, uint32_t k, const uint32_t* __restrict__ lam,
                                                              uint32_t ks, const uint32_t* __restrict__ dtab, MontP M,
                                                              uint16_t* __restrict__ verdict,
                                                              uint32_t* __restrict__ wrong,
                                                              unsigned long long* __restrict__ cnt, uint64_t total,
                                                              int all) {
    decode_body<int32_t, RMAX>(shares, B, D, out, n_idx, kt, k, lam, ks, dtab, M, verdict, wrong, cnt, total, all);
}

// f(std::integral_constant<int, rmax>) for the instantiations of decode_plan.h; false, and no call, for anything else
template <class F>
bool with_rmax(uint32_t rmax, F&& f) {
    if (rmax == 4) f(std::integral_constant<int, 4>{});
    else if (rmax == 8) f(std::integral_constant<int, 8>{});
    else if (rmax == 12) f(std::integral_constant<int, 12>{});
    else if (rmax == 16) f(std::integral_constant<int, 16>{});
    else if (rmax == 32) f(std::integral_constant<int, 32>{});
    else return false;
    return true;
}

template <class ST>
bool decode_launch_t(const PackedDecodePlan& pl, const PackedRepairArgs& a, const ST* sh, uint32_t* wrong,
                     const CheckGeom& g, const uint32_t* dtab, uint64_t total, int all, hipStream_t s) {
    const uint64_t blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    const uint32_t* lam = g.tab + (size_t)(g.n_idx - g.kt) * g.ks;
    return with_rmax(pl.rmax, [&](auto rmax) {
        auto kernel = [&] {
            if constexpr (sizeof(ST) == 4) return packed_decode32_kernel<rmax>; else return packed_decode_kernel<rmax>;
        }();
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, sh, g.B, g.D, a.out, g.n_idx, g.kt, g.k, lam, g.ks, dtab,
                           g.M, a.verdict, wrong, g.cnt, total, all);
    });
}

}  // namespace

hipError_t ensure_decode_table(DeviceTable& tab, const uint64_t* indices, uint32_t n_idx, uint32_t k, uint32_t t,
                               uint32_t p, uint32_t omega_secrets, uint32_t omega_shares) {
    const PackedDecodePlan pl = packed_decode_plan(n_idx, k, t);
    if (!pl.decode) return hipErrorInvalidValue;
    std::vector<uint8_t> key(sizeof(uint32_t) * 6 + sizeof(uint64_t) * n_idx);
    const uint32_t kv[6] = {n_idx, k, t, p, omega_secrets, omega_shares};
    memcpy(key.data(), kv, sizeof(kv));
    memcpy(key.data() + sizeof(kv), indices, sizeof(uint64_t) * n_idx);
    if (tab.key == key) return hipSuccess;
    const DecodeTable T = make_decode_table(indices, n_idx, k, t, p, omega_secrets, omega_shares, pl.rmax);
    if (T.duplicate) return hipErrorInvalidValue;
    return ensure_table(tab, key, T.words.data(), T.words.size() * sizeof(uint32_t));
}

hipError_t launch_packed_decode(const PackedRepairArgs& a, uint32_t* wrong, const CheckGeom& g, const uint32_t* dtab,
                                hipStream_t s, uint64_t* blame_host, PackedCheckResult* res, PackedDecodeResult* dres) {
    const PackedDecodePlan pl = packed_decode_plan(g.n_idx, g.k, g.kt - g.k);
    if (!pl.decode || pl.path != kDecodeDecoded) return hipErrorInvalidValue;
    const uint64_t total = bad_total(g, a.n_vectors, res);
    const bool launched = a.shares32 ? decode_launch_t(pl, a, a.shares32, wrong, g, dtab, total, res->overflowed, s)
                                     : decode_launch_t(pl, a, a.shares, wrong, g, dtab, total, res->overflowed, s);
    if (!launched) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    std::vector<uint64_t> back(kCheckHdr + kCheckBlameCap, 0);
    if ((e = hipMemcpyAsync(back.data(), g.cnt, back.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s)) != hipSuccess)
        return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    res->fixed = back[2];
    dres->decoded = total;
    dres->undecoded = back[3];
    dres->max_errors = (uint32_t)back[kDecodeMaxErrWord];
    for (uint32_t j = 0; j < g.n_idx; ++j) blame_host[j] = back[kCheckHdr + j];
    return hipSuccess;
}

}  // namespace sda
