// packed_check.hip -- packed-Shamir share consistency check with faulty-clerk location (sda_packed_check_dev).
//
// A sharing polynomial has degree below L = k + t + 1, so of the m = n_idx + 1 points of a batch -- the inserted
// (1, 0) and the n_idx clerk shares -- the first L fix it and the other r = n_idx - (k + t) are redundant.  The check
// is the systematic one (packed_common.h, make_check_weights): parity row c < r is
//   syndrome_c = share_{kt+c} + sum_{s < kt} w[c][s] share_s  (mod p),   kt = k + t,
// and a batch is consistent iff every syndrome is 0.  A single error e in share j gives syndrome = e x column j of
// the parity matrix H = [W | I]; any two columns of H are independent when r >= 2 (the code is MDS), so at most one
// position explains a bad batch, and packed_check_locate_kernel finds it: one wave per bad batch, lane j tests
// "syndrome is a multiple of column j" by cross-multiplication (no inverse).
//
// Device table (u32 words, Montgomery form): w[c][s] at c * KS + s, KS = kt rounded up to even, the pad word 0 (the
// kernels take the products of a row in pairs that share one REDC, as reveal_canon_body does) -- the first r rows of
// the table ensure_check_table keeps for both families (packed_common.h, make_check_table).
//
// The counter block, check_report and the register tuple of a batch are check_common.h's, the first pass and the
// bucket dispatch check_launch.h's (shared with the checked reveal, packed_repair.hip).
#include "check_launch.h"
#include "check_plan.h"

namespace sda {
using namespace packed;

namespace {

// One lane = one batch, its n_idx <= NMAX shares in registers: every load is issued before the first wait, each
// share becomes its canonical residue as it lands (raw i64 shares outside (-p, p): reduced exactly in registers,
// reloaded; rare), then r rows of kt Montgomery MACs, two products per REDC (2 p^2 < p R).
template <class ST, int NMAX>
__device__ __forceinline__ void check_body(const ST* __restrict__ shares, uint64_t B, uint32_t n_idx, uint32_t kt,
                                           const uint32_t* __restrict__ tab, uint32_t ks, const MontP& M,
                                           uint16_t* __restrict__ verdict, unsigned long long* __restrict__ cnt,
                                           uint32_t cap) {
    // lanes past the last batch read the last batch again (check_report drops them)
    const uint32_t wave0 = wave_first_thread();
    const uint64_t b0 = (uint64_t)blockIdx.x * 256, rest = B - b0;
    const ST* sh = shares + ((uint64_t)blockIdx.y * n_idx * B + b0) + (threadIdx.x < rest ? threadIdx.x : (uint32_t)rest - 1);
    const uint32_t p = M.p;
    const ShareTuple<NMAX> S = load_residues<ST, NMAX>(sh, B, n_idx, p);
    const uint32_t r = n_idx - kt;
    uint32_t nz = 0;
    for (uint32_t c = 0; c < r; ++c)
        nz |= addm(row_mac<NMAX>(tab + (size_t)c * ks, S, kt, M), S[(kt + c) & (NMAX - 1)], p);     // kt + c < n_idx <= NMAX
    check_report(nz != 0, wave0, B, verdict, cnt, cap);
}

template <int NMAX>
__global__ __launch_bounds__(256) void packed_check_kernel(const int64_t* __restrict__ shares, uint64_t B,
                                                           uint32_t n_idx, uint32_t kt,
                                                           const uint32_t* __restrict__ tab, uint32_t ks, MontP M,
                                                           uint16_t* __restrict__ verdict,
                                                           unsigned long long* __restrict__ cnt, uint32_t cap) {
    check_body<int64_t, NMAX>(shares, B, n_idx, kt, tab, ks, M, verdict, cnt, cap);
}

template <int NMAX>
__global__ __launch_bounds__(256) void packed_check32_kernel(const int32_t* __restrict__ shares, uint64_t B,
                                                             uint32_t n_idx, uint32_t kt,
                                                             const uint32_t* __restrict__ tab, uint32_t ks, MontP M,
                                                             uint16_t* __restrict__ verdict,
                                                             unsigned long long* __restrict__ cnt, uint32_t cap) {
    check_body<int32_t, NMAX>(shares, B, n_idx, kt, tab, ks, M, verdict, cnt, cap);
}

// 33 ... 1023 shares: the parity rows in groups of 8 accumulators; a group reads the kt basis shares of the batch
// once (the first group from HBM, the others from cache) and the weights with uniform loads from the global table.
template <class ST>
__device__ __forceinline__ void check_loop_body(const ST* __restrict__ shares, uint64_t B, uint32_t n_idx, uint32_t kt,
                                                const uint32_t* __restrict__ tab, uint32_t ks, const MontP& M,
                                                uint16_t* __restrict__ verdict, unsigned long long* __restrict__ cnt,
                                                uint32_t cap) {
    constexpr int G = 8;
    // lanes past the last batch read the last batch again (check_report drops them)
    const uint32_t wave0 = wave_first_thread();
    const uint64_t b0 = (uint64_t)blockIdx.x * 256, rest = B - b0;
    const ST* sh = shares + ((uint64_t)blockIdx.y * n_idx * B + b0) + (threadIdx.x < rest ? threadIdx.x : (uint32_t)rest - 1);
    auto share = [&](uint32_t i) { return sh[(uint64_t)i * B]; };
    const uint32_t p = M.p, r = n_idx - kt;
    const int64_t P = (int64_t)p;
    const Mod64 PM = make_mod64(P);
    uint32_t nz = 0;
    for (uint32_t c0 = 0; c0 < r; c0 += G) {
        uint32_t acc[G];
        static_for<0, G>([&](auto u) { acc[u] = 0; });
        for (uint32_t i = 0; i < kt; i += 2) {
            const uint32_t s0 = canon_any(share(i), p, P, PM);
            const uint32_t s1 = i + 1 < kt ? canon_any(share(i + 1), p, P, PM) : 0u;
            static_for<0, G>([&](auto u) {
                const uint32_t* w = tab + (size_t)min(c0 + (uint32_t)u, r - 1) * ks + i;      // rows past r: row r - 1 again
                acc[u] = addm(acc[u], red1(redc_lazy((uint64_t)w[0] * s0 + (uint64_t)w[1] * s1, M), p), p);
            });
        }
        static_for<0, G>([&](auto u) {
            if (c0 + (uint32_t)u < r)
                nz |= addm(acc[u], canon_any(share(kt + c0 + (uint32_t)u), p, P, PM), p);
        });
    }
    check_report(nz != 0, wave0, B, verdict, cnt, cap);
}

__global__ __launch_bounds__(256) void packed_check_loop_kernel(const int64_t* __restrict__ shares, uint64_t B,
                                                                uint32_t n_idx, uint32_t kt,
                                                                const uint32_t* __restrict__ tab, uint32_t ks, MontP M,
                                                                uint16_t* __restrict__ verdict,
                                                                unsigned long long* __restrict__ cnt, uint32_t cap) {
    check_loop_body(shares, B, n_idx, kt, tab, ks, M, verdict, cnt, cap);
}

__global__ __launch_bounds__(256) void packed_check32_loop_kernel(const int32_t* __restrict__ shares, uint64_t B,
                                                                  uint32_t n_idx, uint32_t kt,
                                                                  const uint32_t* __restrict__ tab, uint32_t ks,
                                                                  MontP M, uint16_t* __restrict__ verdict,
                                                                  unsigned long long* __restrict__ cnt, uint32_t cap) {
    check_loop_body(shares, B, n_idx, kt, tab, ks, M, verdict, cnt, cap);
}

// Location (r >= 2): one wave per bad batch -- the `total` logged ones, or with `all` every batch of the launch (the
// log overflowed; consistent batches are recognised and skipped).  The wave computes syndrome c as a sum over its
// lanes (lane l holds share l; shares past 64 are re-read) and lane j tests position j0 + j against it as the rows
// go by:  a basis position j < kt needs  s_c w[0][j] == s_0 w[c][j]  for every c (column j of W has no zero entry);
// a check position kt + c' needs s_c != 0 exactly at c = c'.  At most one position passes.  The located batch gets
// its verdict, and the wave adds to blame[] once per run of equal positions (a whole wrong row is one long run).
template <class ST>
__device__ __forceinline__ void check_locate_body(const ST* __restrict__ shares, uint64_t B, uint32_t n_idx,
                                                  uint32_t kt, const uint32_t* __restrict__ tab, uint32_t ks,
                                                  const MontP& M, uint16_t* __restrict__ verdict,
                                                  unsigned long long* __restrict__ cnt, uint64_t total, int all) {
    const uint32_t lane = threadIdx.x, p = M.p, r = n_idx - kt;
    const int64_t P = (int64_t)p;
    const Mod64 PM = make_mod64(P);
    const unsigned long long* list = cnt + kCheckHdr + kCheckBlameCap;
    uint32_t run_pos = 0;                         // wave-uniform: the current run of located positions (1-based)
    unsigned long long run = 0;
    auto flush = [&]() {
        if (run && lane == 0) atomicAdd(cnt + kCheckHdr + (run_pos - 1), run);
        run = 0;
    };
    for (uint64_t wv = blockIdx.x; wv < total; wv += gridDim.x) {
        const uint64_t gb = all ? wv : list[wv];
        const uint64_t vec = gb / B, b = gb - vec * B;
        const ST* sh = shares + vec * (uint64_t)n_idx * B + b;
        const uint32_t own = lane < n_idx ? canon_any(sh[(uint64_t)lane * B], p, P, PM) : 0u;
        uint32_t found = 0;
        for (uint32_t j0 = 0; j0 < n_idx && !found; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool basis = j < kt;
            const uint32_t w0j = basis ? tab[j] : 0u;
            bool ok = j < n_idx, any = false;
            uint32_t s0 = 0;
            for (uint32_t c = 0; c < r; ++c) {
                const uint32_t* w = tab + (size_t)c * ks;
                uint32_t part = 0;
                for (uint32_t i = lane; i < kt; i += 64)
                    part = addm(part, mont_mul(w[i], i < 64 ? own : canon_any(sh[(uint64_t)i * B], p, P, PM), M), p);
                const uint32_t ci = kt + c;
                if ((ci & 63) == lane) part = addm(part, ci < 64 ? own : canon_any(sh[(uint64_t)ci * B], p, P, PM), p);
                for (int off = 32; off; off >>= 1) part = addm(part, (uint32_t)__shfl_xor((int)part, off), p);
                if (c == 0) s0 = part;
                any = any || part != 0;
                if (basis) ok = ok && mont_mul(w0j, part, M) == mont_mul(w[j], s0, M);
                else ok = ok && ((part != 0) == (j - kt == c));
            }
            if (!any) break;                      // consistent (full pass only)
            const uint64_t mask = __ballot(ok);
            if (mask) found = j0 + (uint32_t)__ffsll((unsigned long long)mask);
        }
        if (found) {
            if (verdict && lane == 0) verdict[gb] = (uint16_t)found;
            if (found != run_pos) {
                flush();
                run_pos = found;
            }
            ++run;
        }
    }
    flush();
}

__global__ __launch_bounds__(64) void packed_check_locate_kernel(const int64_t* __restrict__ shares, uint64_t B,
                                                                 uint32_t n_idx, uint32_t kt,
                                                                 const uint32_t* __restrict__ tab, uint32_t ks, MontP M,
                                                                 uint16_t* __restrict__ verdict,
                                                                 unsigned long long* __restrict__ cnt, uint64_t total,
                                                                 int all) {
    check_locate_body(shares, B, n_idx, kt, tab, ks, M, verdict, cnt, total, all);
}

__global__ __launch_bounds__(64) void packed_check32_locate_kernel(const int32_t* __restrict__ shares, uint64_t B,
                                                                   uint32_t n_idx, uint32_t kt,
                                                                   const uint32_t* __restrict__ tab, uint32_t ks,
                                                                   MontP M, uint16_t* __restrict__ verdict,
                                                                   unsigned long long* __restrict__ cnt, uint64_t total,
                                                                   int all) {
    check_locate_body(shares, B, n_idx, kt, tab, ks, M, verdict, cnt, total, all);
}

// The location pass over `total` logged batches, or with `all` over every batch of the launch.
template <class ST>
hipError_t check_locate_launch_t(const ST* sh, uint16_t* verdict, const CheckGeom& g, uint64_t total, bool all,
                                 hipStream_t s) {
    const unsigned waves = (unsigned)(total < 8192 ? total : 8192);
    auto kernel = [] {
        if constexpr (sizeof(ST) == 4) return packed_check32_locate_kernel; else return packed_check_locate_kernel;
    }();
    hipLaunchKernelGGL(kernel, dim3(waves), dim3(64), 0, s, sh, g.B, g.n_idx, g.kt, g.tab, g.ks, g.M, verdict, g.cnt,
                       total, all ? 1 : 0);
    return hipGetLastError();
}

// The launches of one call for share type ST: the first pass with the kernel the plan names (one wait), then the
// location pass over what it logged (a second wait) when something is bad and r >= 2.
template <class ST>
hipError_t check_launch_t(const PackedCheckPlan& pl, const PackedCheckArgs& a, const ST* sh, const CheckGeom& g,
                          hipStream_t s, uint64_t* blame_host, PackedCheckResult* res) {
    constexpr bool I32 = sizeof(ST) == 4;
    const dim3 grid((unsigned)((g.B + 255) / 256), (unsigned)a.n_vectors);
    auto run = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, sh, g.B, g.n_idx, g.kt, g.tab, g.ks, g.M, a.verdict, g.cnt,
                           g.cap);
    };
    hipError_t e = first_pass(g, s, [&] {
        if (pl.path == kCheckLooped) {
            if constexpr (I32) run(packed_check32_loop_kernel); else run(packed_check_loop_kernel);
            return true;
        }
        return with_bucket(pl.bucket, [&](auto nmax) {
            if constexpr (I32) run(packed_check32_kernel<nmax>); else run(packed_check_kernel<nmax>);
        });
    }, res);
    if (e != hipSuccess || !pl.locate || res->bad == 0) return e;
    res->located = bad_total(g, a.n_vectors, res);
    if ((e = check_locate_launch_t(sh, a.verdict, g, res->located, res->overflowed, s)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(blame_host, g.cnt + kCheckHdr, (size_t)g.n_idx * sizeof(uint64_t), hipMemcpyDeviceToHost,
                            s)) != hipSuccess)
        return e;
    return hipStreamSynchronize(s);
}

}  // namespace

size_t packed_check_buf_bytes() { return (size_t)(kCheckHdr + kCheckBlameCap + kCheckLogCap) * sizeof(uint64_t); }

hipError_t ensure_check_table(DeviceTable& tab, const uint64_t* indices, uint32_t n_idx, uint32_t k, uint32_t t,
                              uint32_t p, uint32_t omega_secrets, uint32_t omega_shares) {
    std::vector<uint8_t> key(sizeof(uint32_t) * 6 + sizeof(uint64_t) * n_idx);
    const uint32_t kv[6] = {n_idx, k, t, p, omega_secrets, omega_shares};
    memcpy(key.data(), kv, sizeof(kv));
    memcpy(key.data() + sizeof(kv), indices, sizeof(uint64_t) * n_idx);
    if (tab.key == key) return hipSuccess;
    const CheckTable T = make_check_table(indices, n_idx, k, t, p, omega_secrets, omega_shares);
    if (T.duplicate) return hipErrorInvalidValue;         // repeated points have no systematic form
    return ensure_table(tab, key, T.words.data(), T.words.size() * sizeof(uint32_t));
}

CheckGeom check_geom(const PackedCheckArgs& a, uint32_t n_idx, uint32_t k, uint32_t t, uint32_t p,
                     const DeviceTable& tab, void* buf, uint32_t log_cap) {
    const uint32_t kt = k + t;
    return {(a.dimension + k - 1) / k, a.dimension, n_idx, kt, k, (kt + 1) & ~1u, make_mont(p),
            static_cast<const uint32_t*>(tab.dev), static_cast<unsigned long long*>(buf),
            log_cap < kCheckLogCap ? log_cap : kCheckLogCap};
}

hipError_t launch_packed_check_locate(const PackedCheckArgs& a, const CheckGeom& g, uint64_t total, bool all,
                                      hipStream_t s) {
    return a.shares32 ? check_locate_launch_t(a.shares32, a.verdict, g, total, all, s)
                      : check_locate_launch_t(a.shares, a.verdict, g, total, all, s);
}

hipError_t launch_packed_check(const PackedCheckArgs& a, const CheckGeom& g, hipStream_t s, uint64_t* blame_host,
                               PackedCheckResult* res) {
    const PackedCheckPlan pl = packed_check_plan(g.n_idx, g.k, g.kt - g.k);
    *res = PackedCheckResult{};
    if (pl.path == kCheckNothing) return hipSuccess;
    res->launched = true;
    return a.shares32 ? check_launch_t(pl, a, a.shares32, g, s, blame_host, res)
                      : check_launch_t(pl, a, a.shares, g, s, blame_host, res);
}

}  // namespace sda
