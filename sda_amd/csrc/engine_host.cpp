// engine_host.cpp -- the streaming, multi-device host path behind the host-buffer entry points of the C ABI
// (include/sda_engine.h), RCCL loaded at run time, and sda_engine_create_multi.
#include "engine_internal.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <mutex>
#include <thread>

#include "host_pack.h"

// ---------------- streaming, multi-device host path ----------------
// The host entry points take the reference's host buffers (a Vec<Vec<i64>> of rows, clerk.rs:79-86) and
// return when the result is in host memory.  A clerk job may be larger than HBM, so rows never sit in one
// device buffer: each device streams them in row tiles through two pinned host buffers and two device tiles
// (host_stage_bytes() each).  Tile i is packed on the host (host threads copying the rows' column slice into
// pinned memory) while tile i - 1 uploads on the copy stream and tile i - 2's combine runs on the compute
// stream; the combine continues the recurrence across tiles (launch_combine_exact, accumulate), so the
// result is bit-identical to one pass over all rows.
//
// Half-width tiles (SDA_HOST_NARROW, host_narrow()): a tile is first packed as int32 (pack_rows32); when every
// value fits -- |v| < m <= 2^31 in every shipped configuration -- it ships and combines as int32 rows
// (launch_combine_wide32, accumulate) in half of its buffers: half the bytes over PCIe.  A tile with a value
// that does not fit is repacked as i64, and the rest of that column chunk's tiles ship as i64 without trying,
// so raw i64 rows cost at most one wasted pack per chunk.  sda_host_stream_stats counts both kinds.
//
// A handle over G devices (sda_engine_create_multi) splits the host calls:
//   - combine (ShareCombiner, Full MaskCombiner, Additive reconstruct): by COLUMNS.  Device g walks every
//     row, in order, over its column slice and writes that slice of the result: exact for signed inputs in
//     one pass with no exchange.  A participation split would have to stream a signed
//     job's rows over PCIe twice (DESIGN.md §5's two-pass split), and the rows come from the host anyway.
//   - ChaCha MaskCombiner: by SEEDS (the expansion is compute-bound, the rows are a few words).  Each device
//     sums its seeds' canonical draws; one RCCL ncclReduce(SUM, int64) over xGMI onto device 0 and the
//     device finalize give the reference's result (every draw is >= 0; headroom G (m - 1) <= 2^63 - 1 is
//     checked).  Moduli above 2^62 (the reference's own sum wraps there) and handles whose ordinals repeat
//     run on device 0 alone.
//   - packed share generate / reconstruct: by BATCHES; additive share generate: by columns.
namespace sda_host __attribute__((visibility("hidden"))) {

static long long env_ll(const char* name, long long dflt) {
    const char* e = getenv(name);
    return e && *e ? atoll(e) : dflt;
}

// host threads for packing rows into pinned memory, over all the handle's devices (SDA_HOST_THREADS; default:
// the CPUs, at most 16 per device)
static int host_threads(size_t devices = 1) {
    const long long t = env_ll("SDA_HOST_THREADS", 0);
    if (t > 0) return (int)std::min<long long>(t, 1024);
    const unsigned hc = std::thread::hardware_concurrency();
    return (int)std::max<unsigned>(1u, std::min<unsigned>(hc ? hc : 1u, 16u * (unsigned)devices));
}

// bytes of one staging tile (SDA_HOST_STAGE_MB, default 256 MiB; at least 1 MiB)
uint64_t host_stage_bytes() {
    const long long mb = env_ll("SDA_HOST_STAGE_MB", 256);
    return (uint64_t)std::max<long long>(mb, 1) << 20;
}

// (the tile packing -- pack_rows, pack_rows32 -- is host_pack.h: HIP-free, tested under a host sanitizer)
using sda::pack_rows;
using sda::pack_rows32;

// SDA_HOST_NARROW (read per call): 1 ships every tile whose values fit as int32 rows -- half the bytes over
// PCIe and into the combine --, 0 ships every tile as i64.  The results are bit-identical.
static bool host_narrow() { return env_ll("SDA_HOST_NARROW", 1) != 0; }

sda_status host_stream_ensure(sda_engine* h, size_t tile_bytes, size_t acc_bytes) {
    if (!h->copy_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(hipEventCreateWithFlags(&h->h2d_done[b], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&h->tile_free[b], hipEventDisableTiming));
        }
    }
    if (h->hs_pin_bytes < 2 * rup(tile_bytes)) {
        if (h->hs_pin) (void)hipHostFree(h->hs_pin);
        h->hs_pin = nullptr;
        h->hs_pin_bytes = 0;
        HIP_TRY(hipHostMalloc(&h->hs_pin, 2 * rup(tile_bytes), hipHostMallocDefault));
        h->hs_pin_bytes = 2 * rup(tile_bytes);
    }
    const size_t dev_need = 2 * rup(tile_bytes) + rup(acc_bytes);
    if (h->hs_dev_bytes < dev_need) {
        dev_free(h->hs_dev);
        h->hs_dev = nullptr;
        h->hs_dev_bytes = 0;
        if (sda_status e = dev_alloc(&h->hs_dev, dev_need)) return e;
        h->hs_dev_bytes = dev_need;
    }
    return SDA_OK;
}

// combiner.rs:22-25 (|m| > 0) over the column slice [lo, lo + w) of n_rows host rows on h's device, streamed
// in row tiles (section comment); the w results land in out_host.  A row slice wider than a tile is taken in
// column chunks, each a full pass over the rows.
static sda_status stream_combine_slice(sda_engine* h, int64_t m, const int64_t* const* rows, uint64_t n_rows,
                                       uint64_t lo, uint64_t w, int64_t* out_host, int threads) {
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t stage = host_stage_bytes();
    const bool narrow = host_narrow();
    const uint64_t wc_max = std::max<uint64_t>(2, stage / 8 / 2 * 2);
    for (uint64_t c0 = 0; c0 < w; c0 += wc_max) {
        const uint64_t wc = std::min(wc_max, w - c0);
        const uint64_t R = std::max<uint64_t>(1, stage / (wc * 8));
        const size_t tile = (size_t)(std::min(R, std::max<uint64_t>(n_rows, 1)) * wc * 8);
        if (sda_status e = host_stream_ensure(h, tile, wc * 8)) return e;
        int64_t* dt[2] = {static_cast<int64_t*>(h->hs_dev), static_cast<int64_t*>(h->hs_dev) + rup(tile) / 8};
        int64_t* acc = static_cast<int64_t*>(h->hs_dev) + 2 * rup(tile) / 8;
        int64_t* hp[2] = {static_cast<int64_t*>(h->hs_pin), static_cast<int64_t*>(h->hs_pin) + rup(tile) / 8};
        uint64_t i = 0;
        bool try32 = narrow;                     // until a tile of this column chunk has to ship wide
        for (uint64_t r0 = 0; r0 < n_rows; r0 += R, ++i) {
            const uint64_t Ri = std::min(R, n_rows - r0);
            const int b = (int)(i & 1);
            if (i >= 2) HIP_TRY(hipEventSynchronize(h->h2d_done[b]));        // tile i - 2 has left hp[b]
            if (try32) try32 = pack_rows32(reinterpret_cast<int32_t*>(hp[b]), rows, r0, Ri, lo + c0, wc, threads);
            if (!try32) pack_rows(hp[b], rows, r0, Ri, lo + c0, wc, threads);
            const size_t bytes = (size_t)(Ri * wc * (try32 ? 4 : 8));
            if (i >= 2) HIP_TRY(hipStreamWaitEvent(h->copy_stream, h->tile_free[b], 0));   // ... and dt[b]
            HIP_TRY(hipMemcpyAsync(dt[b], hp[b], bytes, hipMemcpyHostToDevice, h->copy_stream));
            HIP_TRY(hipEventRecord(h->h2d_done[b], h->copy_stream));
            HIP_TRY(hipStreamWaitEvent(h->stream, h->h2d_done[b], 0));
            if (try32)
                HIP_TRY(sda::launch_combine_wide32(reinterpret_cast<const int32_t*>(dt[b]), Ri, wc, wc, acc, m,
                                                   h->stream, i > 0, &h->last.combine));
            else
                HIP_TRY(sda::launch_combine_exact(dt[b], Ri, wc, wc, acc, m, h->stream, i > 0, &h->last.combine));
            HIP_TRY(hipEventRecord(h->tile_free[b], h->stream));
            ++(try32 ? h->hs_tiles32 : h->hs_tiles64);
            h->hs_bytes_h2d += bytes;
        }
        HIP_TRY(hipMemcpyAsync(out_host + c0, acc, wc * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return SDA_OK;
}

// run fn(g) for every device of the handle, one host thread per device (fn(0) on the caller's thread); the first
// failing device's status and message are returned
template <typename F>
static sda_status for_devices(sda_engine* h, F fn) {
    const size_t G = n_devices(h);
    if (G == 1) return fn(0);
    std::vector<sda_status> st(G, SDA_OK);
    std::vector<std::string> msg(G);
    std::vector<std::thread> ts;
    for (size_t g = 1; g < G; ++g)
        ts.emplace_back([&, g] {
            st[g] = fn(g);
            if (st[g]) msg[g] = last_error();
        });
    st[0] = fn(0);
    if (st[0]) msg[0] = last_error();
    for (auto& t : ts) t.join();
    for (size_t g = 0; g < G; ++g)
        if (st[g]) return fail(st[g], "device %d: %s", h->sub[g]->device, msg[g].c_str());
    return SDA_OK;
}

// even-aligned column split (sda_amd/distributed.py column_slice): [lo, lo + w) of dim for part g of G
static void column_slice(uint64_t dim, size_t g, size_t G, uint64_t* lo, uint64_t* w) {
    const uint64_t pairs = (dim + 1) / 2, base = pairs / G, extra = pairs % G;
    const uint64_t start = g * base + std::min<uint64_t>(g, extra), count = base + (g < extra ? 1 : 0);
    *lo = std::min(dim, 2 * start);
    *w = std::min(dim, 2 * (start + count)) - *lo;
}

// contiguous near-equal split of n items (shard_range)
static void shard(uint64_t n, size_t g, size_t G, uint64_t* start, uint64_t* count) {
    const uint64_t base = n / G, extra = n % G;
    *start = g * base + std::min<uint64_t>(g, extra);
    *count = base + (g < extra ? 1 : 0);
}

// combiner.rs:16-28 over host rows (validated by combine_rows): one device streams all columns, G devices
// a column slice each
sda_status host_combine(sda_engine* h, int64_t m, const int64_t* const* rows, uint64_t n_rows, uint64_t dim,
                        int64_t* out) {
    const size_t G = n_devices(h);
    const int T = std::max(1, host_threads(G) / (int)G);
    return for_devices(h, [&](size_t g) -> sda_status {
        uint64_t lo, w;
        column_slice(dim, g, G, &lo, &w);
        if (w == 0) return SDA_OK;
        return stream_combine_slice(dev_of(h, g), m, rows, n_rows, lo, w, out + lo, T);
    });
}

// ---- RCCL, loaded when a multi-device handle first reduces (single-device users never load it) ----
struct Rccl {
    bool ok = false;
    std::string err;
    ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t,
                           hipStream_t) = nullptr;
    ncclResult_t (*group_start)() = nullptr;
    ncclResult_t (*group_end)() = nullptr;
    const char* (*error_string)(ncclResult_t) = nullptr;
};

static Rccl& rccl() {
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) {
            r.err = dlerror() ? dlerror() : "dlopen(librccl.so.1) failed";
            return;
        }
        r.comm_init_all = reinterpret_cast<decltype(r.comm_init_all)>(dlsym(lib, "ncclCommInitAll"));
        r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(lib, "ncclCommDestroy"));
        r.reduce = reinterpret_cast<decltype(r.reduce)>(dlsym(lib, "ncclReduce"));
        r.group_start = reinterpret_cast<decltype(r.group_start)>(dlsym(lib, "ncclGroupStart"));
        r.group_end = reinterpret_cast<decltype(r.group_end)>(dlsym(lib, "ncclGroupEnd"));
        r.error_string = reinterpret_cast<decltype(r.error_string)>(dlsym(lib, "ncclGetErrorString"));
        r.ok = r.comm_init_all && r.comm_destroy && r.reduce && r.group_start && r.group_end && r.error_string;
        if (!r.ok) r.err = "librccl.so.1 lacks an entry point";
    });
    return r;
}

#define NCCL_TRY(expr)                                                                                  \
    do {                                                                                                \
        ncclResult_t _r = (expr);                                                                       \
        if (_r != ncclSuccess)                                                                          \
            return fail(SDA_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, rccl().error_string(_r), __FILE__, \
                        __LINE__);                                                                      \
    } while (0)

static bool distinct_devices(const sda_engine* h) {
    for (size_t a = 0; a < h->sub.size(); ++a)
        for (size_t b = a + 1; b < h->sub.size(); ++b)
            if (h->sub[a]->device == h->sub[b]->device) return false;
    return true;
}

static sda_status ensure_comms(sda_engine* h) {
    if (h->comms) return SDA_OK;
    Rccl& r = rccl();
    if (!r.ok) return fail(SDA_ERR_DEVICE, "RCCL unavailable: %s", r.err.c_str());
    const size_t G = n_devices(h);
    std::vector<int> devs(G);
    for (size_t g = 0; g < G; ++g) devs[g] = dev_of(h, g)->device;
    std::vector<ncclComm_t> comms(G, nullptr);
    NCCL_TRY(r.comm_init_all(comms.data(), (int)G, devs.data()));
    h->comms = new void*[G];
    for (size_t g = 0; g < G; ++g) h->comms[g] = comms[g];
    return SDA_OK;
}

void destroy_comms(sda_engine* h) {
    if (!h->comms) return;
    for (size_t g = 0; g < n_devices(h); ++g)
        if (h->comms[g]) (void)rccl().comm_destroy(static_cast<ncclComm_t>(h->comms[g]));
    delete[] h->comms;
    h->comms = nullptr;
}

// chacha.rs:57-76 over host seed words [n][w], the combined mask (D values) left in dst on device 0 (ordered on
// h->stream; the other devices are idle again at return): seeds split over the devices, one RCCL reduce onto
// device 0 (section comment).  dst must not lie in device 0's staging arena or work buffer.
sda_status chacha_combine_multi(sda_engine* h, int64_t m, uint64_t D, const std::vector<uint32_t>& seeds, uint32_t w,
                                uint64_t n, int64_t* dst) {
    // (a one-device handle from sda_engine_create_multi takes the split path too: a one-rank reduce)
    const size_t G = n_devices(h);
    const bool split = is_multi(h) && distinct_devices(h) && n >= G && !sda::chacha_needs_stream_path(m) &&
                       (unsigned __int128)G * (uint64_t)(m - 1) <= (unsigned __int128)INT64_MAX;
    const size_t parts = split ? G : 1;
    std::vector<int64_t*> partial(parts, nullptr);
    sda_status st = for_devices(h, [&](size_t g) -> sda_status {
        if (g >= parts) return SDA_OK;
        sda_engine* d = dev_of(h, g);
        HIP_TRY(hipSetDevice(d->device));
        uint64_t s0 = 0, cnt = n;
        if (split) shard(n, g, G, &s0, &cnt);
        DevArena a;
        if (sda_status e = stage(d, rup(cnt * w * 4 + 4) + rup(D * 8), &a)) return e;
        uint32_t* dseeds = a.take<uint32_t>(cnt * w + 1);
        partial[g] = split ? a.take<int64_t>(D) : dst;
        if (cnt) HIP_TRY(hipMemcpyAsync(dseeds, seeds.data() + s0 * w, cnt * w * 4, hipMemcpyHostToDevice, d->stream));
        return chacha_combine(d, m, D, dseeds, w, cnt, partial[g], d->stream);
    });
    if (st) return st;
    HIP_TRY(hipSetDevice(h->device));
    if (!split) return SDA_OK;
    h->last.chacha_split = true;                      // every device recorded its part (sda_chacha_last_launch)
    if (sda_status e = ensure_comms(h)) return e;
    Rccl& r = rccl();
    NCCL_TRY(r.group_start());
    for (size_t g = 0; g < G; ++g) {
        sda_engine* d = dev_of(h, g);
        ncclResult_t rr = r.reduce(partial[g], partial[g], D, ncclInt64, ncclSum, 0,
                                   static_cast<ncclComm_t>(h->comms[g]), d->stream);
        if (rr != ncclSuccess) {
            (void)r.group_end();
            return fail(SDA_ERR_DEVICE, "ncclReduce: %s", r.error_string(rr));
        }
    }
    NCCL_TRY(r.group_end());
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(sda::launch_mod_canonical(partial[0], D, dst, m, h->stream));
    for (size_t g = 1; g < G; ++g) HIP_TRY(hipStreamSynchronize(dev_of(h, g)->stream));   // reduce sent
    return SDA_OK;
}

// the same, the combined mask copied to out_host (MaskCombiner::combine)
sda_status host_chacha_combine(sda_engine* h, int64_t m, uint64_t D, const std::vector<uint32_t>& seeds, uint32_t w,
                               uint64_t n, int64_t* out_host) {
    HIP_TRY(hipSetDevice(h->device));
    if (sda_status e = host_stream_ensure(h, 0, D * 8)) return e;          // dst: the host path's accumulator
    int64_t* dst = static_cast<int64_t*>(h->hs_dev);
    if (sda_status e = chacha_combine_multi(h, m, D, seeds, w, n, dst)) return e;
    HIP_TRY(hipMemcpyAsync(out_host, dst, D * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SDA_OK;
}

// The clerk's job after the sealed-box opens (clerk.rs:79-86): decode every participation's payload
// (sodium.rs:82-88), then combiner.rs:16-28 over the decoded rows in participation order.  Blobs go in groups
// of at most host_stage_bytes() of payload: a host thread packs group g + 1 into pinned buffer (g + 1) mod 2
// while group g uploads and is decoded (int64 rows: any payload, malformed ones included) and combined on the
// compute stream, the recurrence continued across groups -- so a job larger than HBM runs, bit-identical to
// one pass.  The payload crosses PCIe instead of the decoded rows: 4.9 bytes per field share instead of 8.
// Errors in the reference's order: `% 0` folds row 0 before row 1's length is checked, then "Wrong dimension"
// at the first participation whose length differs from participation 0's.  One device (ordinals[0] of a
// multi-device handle): a participation's columns are not locatable in its bytes before it is decoded.
sda_status host_decode_combine(sda_engine* h, int64_t m, const uint8_t* const* blobs, const uint64_t* lens, uint64_t n,
                               int64_t* out, uint64_t out_cap, uint64_t* out_len, int64_t** acc_dev) {
    *out_len = 0;
    if (acc_dev) *acc_dev = nullptr;
    const bool to_host = out || !acc_dev;       // the accumulator alone is wanted: no copy, no capacity check
    h->last.codec = sda::CodecLaunchInfo();     // this path keeps no record: a stale one must not be read
    if (n == 0) return SDA_OK;                                        // combiner.rs:17: empty input
    const uint64_t stage = host_stage_bytes();
    struct Group { uint64_t b0, nb, bytes; };
    std::vector<Group> groups;
    for (uint64_t i = 0; i < n;) {
        Group g{i, 0, 0};
        while (i < n && (g.nb == 0 || g.bytes + lens[i] <= stage)) g.bytes += lens[i++], ++g.nb;
        groups.push_back(g);
    }
    uint64_t biggest = 0;
    for (auto& g : groups) biggest = std::max(biggest, g.bytes);
    const size_t slot = rup(biggest + 32);                           // 16-byte aligned, 16+ readable bytes past
    if (sda_status e = host_stream_ensure(h, slot, 0)) return e;
    uint8_t* hp[2] = {static_cast<uint8_t*>(h->hs_pin), static_cast<uint8_t*>(h->hs_pin) + rup(slot)};
    uint8_t* dbytes[2] = {static_cast<uint8_t*>(h->hs_dev), static_cast<uint8_t*>(h->hs_dev) + rup(slot)};
    const int T = host_threads();
    auto pack = [&](const Group& g, uint8_t* dst, std::vector<uint64_t>* off) {
        off->assign(g.nb + 1, 0);
        for (uint64_t i = 0; i < g.nb; ++i) (*off)[i + 1] = (*off)[i] + lens[g.b0 + i];
        std::vector<std::thread> ts;
        const uint64_t per = (g.nb + T - 1) / T;
        for (int t = 0; t < T && (uint64_t)t * per < g.nb; ++t)
            ts.emplace_back([&, t] {
                for (uint64_t i = (uint64_t)t * per; i < g.nb && i < (uint64_t)(t + 1) * per; ++i)
                    if (lens[g.b0 + i]) memcpy(dst + (*off)[i], blobs[g.b0 + i], lens[g.b0 + i]);
            });
        for (auto& t : ts) t.join();
        memset(dst + (*off)[g.nb], 0, 32);
    };
    std::vector<uint64_t> off[2], counts;
    pack(groups[0], hp[0], &off[0]);
    uint64_t dim = 0, stride = 0;
    int64_t mm = 1;
    int64_t* acc = nullptr;
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        const Group& g = groups[gi];
        const int b = (int)(gi & 1);
        HIP_TRY(hipMemcpyAsync(dbytes[b], hp[b], off[b][g.nb] + 32, hipMemcpyHostToDevice, h->copy_stream));
        HIP_TRY(hipEventRecord(h->h2d_done[b], h->copy_stream));
        HIP_TRY(hipStreamWaitEvent(h->stream, h->h2d_done[b], 0));
        // pack the next group while this one decodes (its pinned buffer's previous upload has to be done)
        std::thread next;
        if (gi + 1 < groups.size()) {
            if (gi >= 1) HIP_TRY(hipEventSynchronize(h->h2d_done[b ^ 1]));
            next = std::thread(pack, std::cref(groups[gi + 1]), hp[b ^ 1], &off[b ^ 1]);
        }
        struct Join { std::thread& t; ~Join() { if (t.joinable()) t.join(); } } join{next};
        // rows of this group as int64 [nb][stride]; participation 0 has at most one element per byte
        if (gi == 0) stride = std::max<uint64_t>(lens[0], 1);
        if (sda_status e = ensure(&h->codec_mat, &h->codec_mat_bytes, g.nb * stride * 8 + 8)) return e;
        sda::VarintPlan plan;
        sda::varint_plan(off[b].data(), g.nb, &plan);
        if (sda_status e = ensure(&h->codec_work, &h->codec_work_bytes, sda::varint_decode_work_bytes(plan.regions, g.nb)))
            return e;
        counts.assign(g.nb, 0);
        bool too_long = false;
        int64_t* mat = static_cast<int64_t*>(h->codec_mat);
        HIP_TRY(sda::launch_varint_decode_one_wait(dbytes[b], off[b].data(), g.nb, plan, h->codec_work, mat, stride,
                                                   counts.data(), &too_long, h->stream));
        if (gi == 0) {
            dim = counts[0];
            if (dim && m == 0) return modulus_abs(m, &mm);         // row 0 is folded first (combiner.rs:20-25)
            if (dim) {
                if (sda_status e = modulus_abs(m, &mm)) return e;
            }
            if (to_host && out_cap < dim) return fail(SDA_ERR_INVALID_ARGUMENT, "output buffer too small");
            if (dim) {
                if (sda_status e = ensure(&h->work, &h->work_bytes, dim * 8)) return e;
                acc = static_cast<int64_t*>(h->work);
            }
        }
        for (uint64_t i = 0; i < g.nb; ++i)
            if (counts[i] != dim)
                return fail(SDA_ERR_WRONG_DIMENSION, "Wrong dimension (participation %llu decodes to %llu shares, expected %llu)",
                            (unsigned long long)(g.b0 + i), (unsigned long long)counts[i], (unsigned long long)dim);
        if (dim)
            HIP_TRY(sda::launch_combine_exact(mat, g.nb, dim, stride, acc, mm, h->stream, gi > 0, &h->last.combine));
        if (gi == 0) stride = std::max<uint64_t>(dim, 1);            // later groups: rows of exactly dim values
    }
    if (dim && to_host) HIP_TRY(hipMemcpyAsync(out, acc, dim * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *out_len = dim;
    if (acc_dev) *acc_dev = acc;
    return SDA_OK;
}

// additive.rs:32-51 per column (batched.rs:19-53 with input_size 1): columns split over the devices;
// out [n][D] clerk-major
sda_status host_additive_generate(sda_engine* h, int64_t m, uint64_t n, const int64_t* secrets, uint64_t D,
                                  const int64_t* draws, int64_t* out, const KeyedDraws* kd) {
    const size_t G = n_devices(h);
    return for_devices(h, [&](size_t g) -> sda_status {
        uint64_t lo, w;
        column_slice(D, g, G, &lo, &w);
        if (w == 0) return SDA_OK;
        sda_engine* d = dev_of(h, g);
        HIP_TRY(hipSetDevice(d->device));
        DevArena a;
        // keyed: the fused kernel draws in registers (additive_keyed.hip), so no draws are staged
        if (sda_status e = stage(d, rup(w * 8) + (kd ? 0 : rup(w * (n - 1) * 8 + 8)) + rup(n * w * 8), &a)) return e;
        int64_t* dsec = a.take<int64_t>(w);
        int64_t* ddr = kd ? nullptr : a.take<int64_t>(w * (n - 1) + 1);
        int64_t* dout = a.take<int64_t>(n * w);
        HIP_TRY(hipMemcpyAsync(dsec, secrets + lo, w * 8, hipMemcpyHostToDevice, d->stream));
        if (kd) {             // column lo + c of the call takes draws (lo + c) * (n - 1) + j: first_column = lo
            HIP_TRY(sda::launch_additive_generate_keyed(kd->key, kd->stream_id, lo, dsec, w, n, m, dout, nullptr, w,
                                                        d->stream));
        } else {
            if (n > 1)
                HIP_TRY(hipMemcpyAsync(ddr, draws + lo * (n - 1), w * (n - 1) * 8, hipMemcpyHostToDevice, d->stream));
            HIP_TRY(sda::launch_additive_generate(dsec, w, ddr, n, dout, m, d->stream));
        }
        HIP_TRY(hipMemcpy2DAsync(out + lo, D * 8, dout, w * 8, w * 8, n, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        return SDA_OK;
    });
}

// packed_shamir.rs:40-43 per batch (batched.rs:19-53): batches split over the devices; out [n][B]
sda_status host_packed_generate(sda_engine* h, const sda_sharing_scheme* s, const int64_t* secrets, uint64_t D,
                                const int64_t* draws, int64_t* out, const KeyedDraws* kd) {
    const uint64_t k = s->secret_count, t = s->privacy_threshold, n = s->share_count, B = (D + k - 1) / k;
    const size_t G = n_devices(h);
    return for_devices(h, [&](size_t g) -> sda_status {
        uint64_t b0, nb;
        shard(B, g, G, &b0, &nb);
        if (nb == 0) return SDA_OK;
        sda_engine* d = dev_of(h, g);
        HIP_TRY(hipSetDevice(d->device));
        const uint64_t s0 = b0 * k, ds = std::min(D, (b0 + nb) * k) - s0;   // the last batch may be short (padded)
        DevArena a;
        // keyed: the launch makes the draws itself (packed_generate), so no draws slice is staged in the arena
        if (sda_status e = stage(d, rup(ds * 8) + (kd ? 0 : rup(nb * t * 8 + 8)) + rup(n * nb * 8), &a)) return e;
        int64_t* dsec = a.take<int64_t>(ds);
        int64_t* ddr = kd ? nullptr : a.take<int64_t>(nb * t + 1);
        int64_t* dout = a.take<int64_t>(n * nb);
        HIP_TRY(hipMemcpyAsync(dsec, secrets + s0, ds * 8, hipMemcpyHostToDevice, d->stream));
        if (t && !kd)
            HIP_TRY(hipMemcpyAsync(ddr, draws + b0 * t, nb * t * 8, hipMemcpyHostToDevice, d->stream));
        sda::PackedGenArgs ga{dsec, ds, 1, ddr, dout};
        if (kd) {             // batch b0 + b of the call takes draws (b0 + b) t + j: first_batch = b0
            ga.key = kd->key;
            ga.stream_id = kd->stream_id;
            ga.first_batch = b0;
        }
        if (sda_status e = packed_generate(d, s, ga, d->stream)) return e;
        HIP_TRY(hipMemcpy2DAsync(out + b0, B * 8, dout, nb * 8, nb * 8, n, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        return SDA_OK;
    });
}

// packed_shamir.rs:73-77 per batch (batched.rs:69-97), exact: batches split over the devices; out [dimension]
sda_status host_packed_reconstruct(sda_engine* h, const sda_sharing_scheme* s, uint64_t dimension,
                                   const uint64_t* indices, const int64_t* const* rows, uint64_t n_rows, int64_t* out) {
    const uint64_t k = s->secret_count, B = (dimension + k - 1) / k;
    const size_t G = n_devices(h);
    return for_devices(h, [&](size_t g) -> sda_status {
        uint64_t b0, nb;
        shard(B, g, G, &b0, &nb);
        if (nb == 0) return SDA_OK;
        sda_engine* d = dev_of(h, g);
        HIP_TRY(hipSetDevice(d->device));
        const uint64_t s0 = b0 * k, ds = std::min(dimension, (b0 + nb) * k) - s0;
        DevArena a;
        if (sda_status e = stage(d, rup(n_rows * nb * 8) + rup(ds * 8), &a)) return e;
        int64_t* din = a.take<int64_t>(n_rows * nb);
        int64_t* dout = a.take<int64_t>(ds);
        for (uint64_t i = 0; i < n_rows; ++i)        // batched.rs:83-85: clerk i's batches [b0, b0 + nb)
            HIP_TRY(hipMemcpyAsync(din + i * nb, rows[i] + b0, nb * 8, hipMemcpyHostToDevice, d->stream));
        sda::PackedRevealArgs ra{din, ds, 1, dout};
        if (sda_status e = packed_reveal(d, s, ra, indices, n_rows, SDA_REVEAL_EXACT, d->stream)) return e;
        HIP_TRY(hipMemcpyAsync(out + s0, dout, ds * 8, hipMemcpyDeviceToHost, d->stream));
        HIP_TRY(hipStreamSynchronize(d->stream));
        return SDA_OK;
    });
}

}  // namespace sda_host

using namespace sda_host;

extern "C" {

sda_status sda_engine_create_multi(const int* ordinals, int n_devices_, sda_engine** out) {
    SDA_ENTRY;
    if (!out) return fail(SDA_ERR_INVALID_ARGUMENT, "out is NULL");
    *out = nullptr;
    if (!ordinals || n_devices_ < 1 || n_devices_ > 64)
        return fail(SDA_ERR_INVALID_ARGUMENT, "need 1..64 device ordinals");
    sda_engine* h = nullptr;
    if (sda_status e = sda_engine_create(ordinals[0], &h)) return e;
    if (n_devices_ == 1) {                       // a one-device handle that still reduces through RCCL
        h->sub.push_back(h);
        *out = h;
        return ok();
    }
    h->sub.push_back(h);
    for (int g = 1; g < n_devices_; ++g) {
        sda_engine* d = nullptr;
        if (sda_status e = sda_engine_create(ordinals[g], &d)) {
            const std::string msg = last_error();
            sda_engine_destroy(h);
            return fail(e, "device %d: %s", ordinals[g], msg.c_str());
        }
        h->sub.push_back(d);
    }
    HIP_TRY(hipSetDevice(h->device));
    *out = h;
    return ok();
}

int sda_engine_device_count(const sda_engine* h) { return h ? (int)n_devices(h) : 0; }

}  // extern "C"
