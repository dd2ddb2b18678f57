// packed_repair.hip -- checked reveal: the share consistency check and the CANONICAL reveal in one pass over the
// shares, with a located wrong share corrected (sda_packed_reveal_checked_dev).
//
// The check is systematic (packed_check.hip): the first kt = k + t shares of a batch fix its polynomial and r parity
// rows test the others.  Once a batch is consistent, its reveal from all n_idx shares equals its reveal from the kt
// basis shares alone, so packed_repair_kernel computes, from one load of the batch,
//   syndrome_c = share_{kt+c} + sum_{s < kt} w[c][s] share_s,  c < r        (bad iff some syndrome != 0)
//   secret_e   = sum_{s < kt} lam[e][s] share_s,               e < k        (make_repair_tables' basis rows)
// and reports a bad batch exactly as the check does.  What the basis reveal means for a bad batch:
//   located at a check position j > kt   the basis is clean: already the reveal without share j
//   not located                          the reveal from the first kt shares: flagged garbage, the rule on every path
//   located at a basis position j <= kt  share j carries an error err with syndrome_0 = err w[0][j-1], so
//                                        err = syndrome_0 winv[j-1]  and  secret_e -= lam[e][j-1] err
// The last is packed_repair_fix_kernel's work, behind packed_check_locate_kernel, launched only when something is bad.
// Schemes past the fused kernel (repair_plan.h) run the share check and the CANONICAL reveal as they are, and the
// fix-up then recomputes every bad batch from its basis before it corrects.
//
// Device table (u32 words, Montgomery form, rows of KS = kt rounded up to even words, pad word 0) -- the one
// ensure_check_table (packed_check.hip) keeps for both families, built by make_check_table (packed_common.h):
//   rows [0, r)       the check's parity rows w[c][s]
//   rows [r, r + k)   lam[e][s]
//   row  r + k        winv[s] (zeros when r == 0)
#include "check_launch.h"
#include "repair_body.h"
#include "repair_plan.h"

namespace sda {
using namespace packed;

namespace {

// The first pass is repair_body (repair_body.h) with the secrets stored as they are.
template <int NMAX>
__global__ __launch_bounds__(256) void packed_repair_kernel(const int64_t* __restrict__ shares, uint64_t B, uint64_t D,
                                                            int64_t* __restrict__ out, uint32_t n_idx, uint32_t kt,
                                                            uint32_t k, const uint32_t* __restrict__ tab, uint32_t ks,
                                                            MontP M, uint16_t* __restrict__ verdict,
                                                            unsigned long long* __restrict__ cnt, uint32_t cap) {
    extern __shared__ int64_t lds_o[];
    repair_body<int64_t, NMAX>(shares, B, D, out, n_idx, kt, k, tab, ks, M, verdict, cnt, cap, lds_o, FlushAsIs{});
}

template <int NMAX>
__global__ __launch_bounds__(256) void packed_repair32_kernel(const int32_t* __restrict__ shares, uint64_t B,
                                                              uint64_t D, int64_t* __restrict__ out, uint32_t n_idx,
                                                              uint32_t kt, uint32_t k,
                                                              const uint32_t* __restrict__ tab, uint32_t ks, MontP M,
                                                              uint16_t* __restrict__ verdict,
                                                              unsigned long long* __restrict__ cnt, uint32_t cap) {
    extern __shared__ int64_t lds_o[];
    repair_body<int32_t, NMAX>(shares, B, D, out, n_idx, kt, k, tab, ks, M, verdict, cnt, cap, lds_o, FlushAsIs{});
}

// One lane per bad batch -- the `total` logged ones, or with `all` every batch of the call (the log overflowed).  A
// batch located at a basis position (1 <= verdict <= kt) is corrected; syndrome_0 is recomputed from the batch's
// kt + 1 shares.  Without `recompute` (fused path) the others are right as they stand; with it (composed path) every
// batch whose verdict is not 0 is first revealed again from its basis.  cnt[2] counts the batches rewritten.
template <class ST>
__device__ __forceinline__ void repair_fix_body(const ST* __restrict__ shares, uint64_t B, uint64_t D,
                                                int64_t* __restrict__ out, uint32_t n_idx, uint32_t kt, uint32_t k,
                                                const uint32_t* __restrict__ tab, uint32_t ks, const MontP& M,
                                                const uint16_t* __restrict__ verdict,
                                                unsigned long long* __restrict__ cnt, uint64_t total, int all,
                                                int recompute) {
    const uint32_t p = M.p, r = n_idx - kt;
    const int64_t P = (int64_t)p;
    const Mod64 PM = make_mod64(P);
    const uint32_t* lam = tab + (size_t)r * ks;
    const uint32_t* winv = lam + (size_t)k * ks;
    const unsigned long long* list = cnt + kCheckHdr + kCheckBlameCap;
    uint32_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t gb = all ? i : list[i];
        const uint32_t v = verdict[gb];
        const bool basis = v >= 1 && v <= kt;
        if (recompute ? v == 0 : !basis) continue;
        const uint64_t vec = gb / B, b = gb - vec * B;
        const uint32_t lim = b * k < D ? (uint32_t)(D - b * k < k ? D - b * k : k) : 0u;
        const ST* sh = shares + vec * (uint64_t)n_idx * B + b;
        int64_t* dst = out + vec * D + b * k;
        auto share = [&](uint32_t s) { return canon_any(sh[(uint64_t)s * B], p, P, PM); };
        uint32_t err = 0;
        if (basis) {                                      // located: r >= 2, so share kt exists
            uint32_t s0 = share(kt);
            for (uint32_t s = 0; s < kt; ++s) s0 = addm(s0, mont_mul(tab[s], share(s), M), p);
            err = mont_mul(winv[v - 1], s0, M);
        }
        for (uint32_t e = 0; e < lim; ++e) {
            const uint32_t* le = lam + (size_t)e * ks;
            uint32_t acc = 0;
            if (recompute)
                for (uint32_t s = 0; s < kt; ++s) acc = addm(acc, mont_mul(le[s], share(s), M), p);
            else
                acc = (uint32_t)dst[e];
            if (basis) acc = subm(acc, mont_mul(le[v - 1], err, M), p);
            dst[e] = (int64_t)acc;
        }
        ++mine;
    }
    for (int off = 32; off; off >>= 1) mine += (uint32_t)__shfl_xor((int)mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(cnt + 2, (unsigned long long)mine);
}

__global__ __launch_bounds__(256) void packed_repair_fix_kernel(const int64_t* __restrict__ shares, uint64_t B,
                                                                uint64_t D, int64_t* __restrict__ out, uint32_t n_idx,
                                                                uint32_t kt, uint32_t k,
                                                                const uint32_t* __restrict__ tab, uint32_t ks, MontP M,
                                                                const uint16_t* __restrict__ verdict,
                                                                unsigned long long* __restrict__ cnt, uint64_t total,
                                                                int all, int recompute) {
    repair_fix_body(shares, B, D, out, n_idx, kt, k, tab, ks, M, verdict, cnt, total, all, recompute);
}

__global__ __launch_bounds__(256) void packed_repair32_fix_kernel(const int32_t* __restrict__ shares, uint64_t B,
                                                                  uint64_t D, int64_t* __restrict__ out,
                                                                  uint32_t n_idx, uint32_t kt, uint32_t k,
                                                                  const uint32_t* __restrict__ tab, uint32_t ks,
                                                                  MontP M, const uint16_t* __restrict__ verdict,
                                                                  unsigned long long* __restrict__ cnt, uint64_t total,
                                                                  int all, int recompute) {
    repair_fix_body(shares, B, D, out, n_idx, kt, k, tab, ks, M, verdict, cnt, total, all, recompute);
}


// The fused first pass for share type ST: the bucket's kernel inside first_pass (one wait).
template <class ST>
hipError_t repair_launch_t(const PackedRepairPlan& pl, const PackedRepairArgs& a, const ST* sh, const CheckGeom& g,
                           hipStream_t s, PackedCheckResult* res) {
    const dim3 grid((unsigned)((g.B + 255) / 256), (unsigned)a.n_vectors);
    const size_t lds = (size_t)256 * g.k * sizeof(int64_t);
    return first_pass(g, s, [&] {
        return with_bucket(pl.bucket, [&](auto nmax) {
            auto kernel = [&] {
                if constexpr (sizeof(ST) == 4) return packed_repair32_kernel<nmax>; else return packed_repair_kernel<nmax>;
            }();
            hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, sh, g.B, g.D, a.out, g.n_idx, g.kt, g.k, g.tab, g.ks,
                               g.M, a.verdict, g.cnt, g.cap);
        });
    }, res);
}

}  // namespace

hipError_t launch_packed_repair(const PackedRepairArgs& a, const CheckGeom& g, hipStream_t s, PackedCheckResult* res) {
    const PackedRepairPlan pl = packed_repair_plan(g.n_idx, g.k, g.kt - g.k);
    if (pl.path != kRepairFused) return hipErrorInvalidValue;
    *res = PackedCheckResult{};
    res->launched = true;
    return a.shares32 ? repair_launch_t(pl, a, a.shares32, g, s, res) : repair_launch_t(pl, a, a.shares, g, s, res);
}

hipError_t launch_packed_repair_fix(const PackedRepairArgs& a, uint16_t* verdict, const CheckGeom& g, bool locate,
                                    bool recompute, hipStream_t s, uint64_t* blame_host, PackedCheckResult* res) {
    const uint64_t total = bad_total(g, a.n_vectors, res);
    const int all = res->overflowed ? 1 : 0;
    hipError_t e;
    if (locate) {
        PackedCheckArgs ca = a;
        ca.verdict = verdict;
        if ((e = launch_packed_check_locate(ca, g, total, res->overflowed, s)) != hipSuccess) return e;
    }
    const uint64_t blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
    if (a.shares32)
        hipLaunchKernelGGL(packed_repair32_fix_kernel, grid, dim3(256), 0, s, a.shares32, g.B, g.D, a.out, g.n_idx, g.kt,
                           g.k, g.tab, g.ks, g.M, verdict, g.cnt, total, all, recompute ? 1 : 0);
    else
        hipLaunchKernelGGL(packed_repair_fix_kernel, grid, dim3(256), 0, s, a.shares, g.B, g.D, a.out, g.n_idx, g.kt,
                           g.k, g.tab, g.ks, g.M, verdict, g.cnt, total, all, recompute ? 1 : 0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    std::vector<uint64_t> back(kCheckHdr + g.n_idx, 0);
    if ((e = hipMemcpyAsync(back.data(), g.cnt, back.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s)) != hipSuccess)
        return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    res->fixed = back[2];
    if (locate)
        for (uint32_t j = 0; j < g.n_idx; ++j) blame_host[j] = back[kCheckHdr + j];
    return hipSuccess;
}

}  // namespace sda
