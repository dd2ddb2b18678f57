#pragma once
// check_launch.h -- host pieces shared by the launchers of the share check (packed_check.hip) and the checked reveal
// (packed_repair.hip): the dispatch over the register buckets, the first pass around either family's kernel, and what
// a pass over the bad batches walks.
#include <type_traits>

#include "check_common.h"

namespace sda {

// f(std::integral_constant<int, bucket>) for the 8 / 16 / 32 share buckets of check_plan.h and repair_plan.h; false,
// and no call, for anything else
template <class F>
bool with_bucket(uint32_t bucket, F&& f) {
    if (bucket == 8) f(std::integral_constant<int, 8>{});
    else if (bucket == 16) f(std::integral_constant<int, 16>{});
    else if (bucket == 32) f(std::integral_constant<int, 32>{});
    else return false;
    return true;
}

// The first pass of a call and its one wait: the counters and blame words zeroed, launch() -- it enqueues the pass's
// kernel on s, or returns false when it has none --, the two head words copied back.
template <class L>
hipError_t first_pass(const CheckGeom& g, hipStream_t s, L&& launch, PackedCheckResult* res) {
    hipError_t e = hipMemsetAsync(g.cnt, 0, (size_t)(packed::kCheckHdr + packed::kCheckBlameCap) * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    if (!launch()) return hipErrorInvalidValue;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    uint64_t head[2] = {0, 0};
    if ((e = hipMemcpyAsync(head, g.cnt, sizeof(head), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    res->bad = head[0];
    res->first_bad = ~head[1];                              // 0 (no max taken) -> UINT64_MAX
    return hipSuccess;
}

// The batches a pass over the bad ones walks: the res->bad logged ones, or, the log overflowed (res->overflowed is
// set here), every batch of the call.
inline uint64_t bad_total(const CheckGeom& g, uint64_t n_vectors, PackedCheckResult* res) {
    res->overflowed = res->bad > g.cap;
    return res->overflowed ? g.B * n_vectors : res->bad;
}

}  // namespace sda
