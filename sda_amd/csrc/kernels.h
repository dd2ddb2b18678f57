// kernels.h -- internal launchers (not part of the C ABI).  Each returns hipSuccess or the
// launch error; all of them only enqueue on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "modarith.h"
#include "reveal_plan.h"
#include "check_plan.h"
#include "repair_plan.h"
#include "decode_plan.h"

namespace sda {

// ---- combine.hip ----
// Which combine kernel a launch ran and on what grid (sda_combine_last_launch reports the handle's last one).
// Filled where each decision is taken: launch_vec for the combine_exact_kernel instantiation and its grid, the
// replay launcher for its own, each once the runtime has accepted the launch.  A launcher that launches nothing
// (dim == 0; the split and replay with n == 0) or whose launch is refused leaves *info untouched.  Every call site in engine.cpp passes the handle's record; chacha.hip's stream path
// (launch_chacha_streams_combine) passes none: its combine is part of a ChaCha launch, which
// sda_chacha_last_launch describes.
enum CombineKind : uint32_t {
    kCombineNone = 0,         // no combine launch yet
    kCombineExact = 1,        // combine_exact_kernel
    kCombineReplay = 2,       // combine_replay_kernel
};
enum CombineVariant : uint32_t {  // the kernels' bool template arguments
    kCombineSmallM = 1,       // SMALL_M: m <= 2^62
    kCombineAcc = 2,          // ACC: continues from `out`
    kCombineFlag = 4,         // FLAG: pass 1 of the participation split
    kCombinePipe = 8,         // PIPE: software-pipelined
};
struct CombineLaunchInfo {
    uint32_t kind = kCombineNone;
    uint32_t elem_bytes = 0;  // 8 (i64 rows) or 4 (int32 rows)
    uint32_t vec = 0;         // columns per lane: 1, 2 or 4
    uint32_t rows = 0;        // rows per batch (the UNROLL argument): 2, 4 or 8
    uint32_t variant = 0;     // CombineVariant bits
    uint64_t grid = 0;        // workgroups launched
    uint32_t wlo = 0;         // balanced grid (combine_grid): lanes per workgroup, + 8 in the first nwide ones;
    uint32_t nwide = 0;       // 0, 0 on the plain grid of 256-lane workgroups
    uint32_t per_cu = 0;      // the occupancy handed to combine_grid; 0 when the balanced grid was not considered
};
// Exact clerk combine: out[j] = fold over rows of (r + v) % m  (combiner.rs:22-25).
// accumulate: continue from the values in `out` (a previous result, |r| < m) instead of 0.
hipError_t launch_combine_exact(const int64_t* in, uint64_t n, uint64_t dim, uint64_t stride,
                                int64_t* out, int64_t modulus, hipStream_t s, bool accumulate = false,
                                CombineLaunchInfo* info = nullptr);
// The same recurrence over int32 rows (decoded field shares: the clerk's decode -> combine).
hipError_t launch_combine_exact32(const int32_t* in, uint64_t n, uint64_t dim, uint64_t stride,
                                  int64_t* out, int64_t modulus, hipStream_t s, bool accumulate = false,
                                  CombineLaunchInfo* info = nullptr);
// int32 share rows as an input type of the combine (sda_combine32_dev, the half-width host stream): 16-byte
// loads (4 columns per lane), software-pipelined on the balanced grid where the rows line up, else the
// kernels above.  Sign-extends and runs the i64 recurrence: exact for every modulus.
hipError_t launch_combine_wide32(const int32_t* in, uint64_t n, uint64_t dim, uint64_t stride, int64_t* out,
                                 int64_t modulus, hipStream_t s, bool accumulate = false,
                                 CombineLaunchInfo* info = nullptr);
// dst[n][dim] (int32, row stride dst_stride) = (int32_t)src[n][dim] (row stride src_stride); flag[0] = 1 when
// a value lies outside int32 (never cleared).
hipError_t launch_narrow32(const int64_t* src, uint64_t n, uint64_t dim, uint64_t src_stride, int32_t* dst,
                           uint64_t dst_stride, int64_t* flag, hipStream_t s);
// Canonical residue of the int64 sums of the ranks' results (multi-GPU finalize; signed sums allowed).
hipError_t launch_mod_canonical(const int64_t* sums, uint64_t dim, int64_t* out, int64_t modulus,
                                hipStream_t s);
// Participation split.  Pass 1: the exact recurrence continued from inout that also sets
// flags[0] = 1 (an input < 0) / flags[1] = 1 (an input outside [-(2^63 - m), 2^63 - m]).
hipError_t launch_combine_split(const int64_t* in, uint64_t n, uint64_t dim, uint64_t stride, int64_t* inout,
                                int64_t modulus, int64_t* flags, hipStream_t s, CombineLaunchInfo* info = nullptr);
// Pass 2 (signed inputs): replay the canonical trajectory from state (c_in), recording the last sign
// event in code (reset_code = 2 rank + 1 on a reset, + 1 on a set; unchanged without an event).
hipError_t launch_combine_replay(const int64_t* in, uint64_t n, uint64_t dim, uint64_t stride, int64_t* state,
                                 int32_t* code, int32_t reset_code, int64_t modulus, hipStream_t s,
                                 CombineLaunchInfo* info = nullptr);
hipError_t launch_split_prefix(const int64_t* gathered, uint64_t world, uint64_t rank, uint64_t dim, int64_t* c_in,
                               int64_t* total, int32_t* code, int64_t modulus, hipStream_t s);
hipError_t launch_split_resolve(const int64_t* total, const int32_t* code, uint64_t dim, int64_t* out,
                                int64_t modulus, hipStream_t s);

// ---- elementwise.hip ----
hipError_t launch_additive_generate(const int64_t* secrets, uint64_t D, const int64_t* draws,
                                    uint64_t n, int64_t* out, int64_t modulus, hipStream_t s);
// out[i] = (a[i] + sign * b[i]) % m   (sign = +1: mask, -1: unmask)
hipError_t launch_addsub_trem(const int64_t* a, const int64_t* b, int sign, uint64_t D,
                              int64_t* out, int64_t modulus, hipStream_t s);
hipError_t launch_positive(const int64_t* v, uint64_t D, int64_t* out, int64_t modulus,
                           hipStream_t s);
// out = positive((ms - mask) % q, pos_m); mask == nullptr: no unmask; pos_m == 0: no positive()
hipError_t launch_unmask_positive(const int64_t* ms, const int64_t* mask, uint64_t D, int64_t q, int64_t pos_m,
                                  int64_t* out, hipStream_t s);
hipError_t launch_synth_fill(int64_t* dst, uint64_t rows, uint64_t cols, uint64_t seed,
                             int64_t lo, int64_t hi, hipStream_t s);

// ---- packed_gen.hip / packed_reveal.hip ----
// Engine-owned device copy of a precomputed, data-independent table (twiddles, Newton inverses,
// Lagrange weights).  Rebuilt and uploaded only when its key (the parameters it depends on) changes.
struct DeviceTable {
    std::vector<uint8_t> key;
    void* dev = nullptr;
    size_t cap = 0;
    void* ws = nullptr;           // packed_wide.hip: per-lane transform workspace (grows, never shrinks)
    size_t ws_cap = 0;
    uint32_t flags = 0;           // per-table launch choices (packed_gen.hip: bit 0 = sign-bit kernel)
};
hipError_t ensure_table(DeviceTable& t, const std::vector<uint8_t>& key, const void* host, size_t bytes);
void free_table(DeviceTable& t);

struct PackedGenArgs {
    const int64_t* secrets; uint64_t dimension; uint64_t n_vectors;
    const int64_t* draws; int64_t* out;
    bool canonical = false;       // shares as canonical residues in [0, p) instead of tss' signed values
    // int32 shares (sda_packed_generate32_dev): out32 != nullptr replaces out, [n_vectors][n][B] int32.  Native
    // kernels up to n + 1 = 27 and on the workspace path; the n + 1 = 81 register kernels write i64 into
    // `scratch` (PackedGenPlan::narrow_bytes bytes, 16-byte aligned) and launch_narrow32 narrows it (`flag`: its
    // device word).
    int32_t* out32 = nullptr;
    int64_t* scratch = nullptr;
    int64_t* flag = nullptr;
    // keyed (sda_packed_generate_keyed_dev): key != nullptr replaces `draws`.  Batch b of vector v takes draws
    // (first_batch + v B + b) t + j, j < t, of launch_draws' rule under (key, stream_id) at bound p - 1 (key: HOST,
    // 8 words; the caller has checked that (first_batch + n_vectors B) t does not wrap).  Schemes on the register
    // path with n + 1 <= 27 make them in the share kernels; the others get launch_draws into draw_scratch
    // (PackedGenPlan::draw_bytes bytes) ahead of the unkeyed kernels.  keyed_fuse = false stages every scheme.
    const uint32_t* key = nullptr;
    uint32_t stream_id = 0;
    uint64_t first_batch = 0;
    int64_t* draw_scratch = nullptr;
    bool keyed_fuse = true;
};
// How one share-gen call runs.  packed_gen_plan decides it once: the engine sizes the call's scratch from it and
// launch_packed_generate dispatches from it, so the two cannot disagree.
struct PackedGenPlan {
    uint64_t B;                   // batches per vector
    bool pair;                    // pair store: even B and a 16-byte aligned caller buffer (out32, else out) -- also
                                  // when the i64 kernels write `scratch` for an int32 caller (narrow_bytes)
    bool lazy;                    // p >= kLazyTruncMinP: exact shares with pair stores take the lazy-truncation kernels
    bool registers;               // the register kernels (gen_register_path), else packed_wide.hip's workspace kernels
    uint32_t keyed_path;          // 0 unkeyed; 1 draws made in the share kernels; 2 staged through draw_scratch, after
                                  // which the call runs as the unkeyed one it has become (sda_packed_keyed_last_launch)
    size_t draw_bytes;            // draw_scratch the staged call needs: n_vectors B t 8 (0 on paths 0 and 1)
    size_t narrow_bytes;          // nonzero: int32 shares from the n + 1 = 81 register kernels, i64 into this much
                                  // `scratch`, then launch_narrow32
};
PackedGenPlan packed_gen_plan(const PackedGenArgs& a, uint32_t k, uint32_t t, uint32_t n, uint32_t p);
// A/B knob: SDA_XCD_ORDER=0 runs the streaming kernels in natural workgroup order (xcd.h).
bool xcd_order_enabled();
// Batches whose inputs fall outside (-p, p) are logged by the fast kernel and recomputed by a
// generic exact fix-up kernel.  `log_buf` is device memory of packed_gen_log_bytes() bytes.
constexpr uint32_t kGenLogCap = 1u << 16;
struct GenFixupLog {
    unsigned int* count;
    uint64_t* list;        // vec * B + batch
    uint32_t cap;
};
size_t packed_gen_log_bytes();
// *logged (host, optional; both launchers): whether this launch zeroed `log_buf`'s count and ran kernels that
// log into it -- false for the workspace kernels and the canonical Lagrange reveal (sda_packed_fixup_count).
hipError_t launch_packed_generate(const PackedGenArgs& a, uint32_t k, uint32_t t, uint32_t n, uint32_t p,
                                  uint32_t omega_secrets, uint32_t omega_shares, DeviceTable& tab, void* log_buf,
                                  hipStream_t s, bool* logged = nullptr);
struct PackedRevealArgs {
    const int64_t* shares; uint64_t dimension; uint64_t n_vectors; int64_t* out;
    const int32_t* shares32 = nullptr;   // int32 shares (sda_packed_reconstruct32_dev): replaces `shares`
};
// Past these sizes (k + t + 1 > 64, n + 1 > 81, more than kRevealMaxPoints - 1 shares: reveal_plan.h) the packed
// calls take packed_wide.hip's workspace kernels, up to the engine's domain limits below.
constexpr uint32_t kWideMaxL = 1024;       // k + t + 1
constexpr uint32_t kWideMaxN3 = 729;       // n + 1
constexpr uint32_t kRevealMaxShares = 1023;
hipError_t launch_packed_generate_wide(const PackedGenArgs& a, uint32_t k, uint32_t t, uint32_t n, uint32_t p,
                                       uint32_t omega_secrets, uint32_t omega_shares, DeviceTable& tab,
                                       hipStream_t s);
// Runs the call as packed_reveal_plan (reveal_plan.h) decides it.  Returns hipErrorInvalidValue for CANONICAL mode
// with duplicate clerk points: nothing is launched and `tab` keeps its key.  `log_buf`: device memory of
// packed_gen_log_bytes() bytes (batches the exact kernel hands to its fix-up).
hipError_t launch_packed_reveal(const PackedRevealArgs& a, const uint64_t* indices, uint32_t n_idx, uint32_t k,
                                uint32_t t, uint32_t p, uint32_t omega_secrets, uint32_t omega_shares, int mode,
                                DeviceTable& tab, void* log_buf, hipStream_t s, bool* logged = nullptr);
hipError_t launch_packed_reveal_wide(const PackedRevealArgs& a, const uint64_t* indices, uint32_t n_idx, uint32_t k,
                                     uint32_t p, uint32_t omega_secrets, uint32_t omega_shares, int mode,
                                     DeviceTable& tab, hipStream_t s);

// ---- packed_check.hip / packed_repair.hip ----
// Share consistency check of a reveal's input (sda_packed_check_dev): the shares as PackedRevealArgs lays them out and
// the per-batch verdicts.  The checked reveal (sda_packed_reveal_checked_dev) takes the same plus `out`.
struct PackedCheckArgs {
    const int64_t* shares; const int32_t* shares32;   // one of the two
    uint64_t dimension; uint64_t n_vectors;
    uint16_t* verdict;        // device [n_vectors][B], or nullptr
};
struct PackedRepairArgs : PackedCheckArgs {
    int64_t* out;             // device [n_vectors][dimension]
};
// The counts of one call of either family.
struct PackedCheckResult {
    uint64_t bad = 0, first_bad = UINT64_MAX;   // bad batches; the smallest bad vec * B + b, UINT64_MAX for none
    uint64_t located = 0;     // batches the location pass walked: the bad ones, or on overflow every batch
    uint64_t fixed = 0;       // batches packed_repair_fix_kernel rewrote
    bool overflowed = false;  // more bad batches than the log holds
    bool launched = false;    // false: no redundancy -- the check ran nothing and the counts are zero
};
constexpr uint32_t kCheckLogCap = 1u << 16;
size_t packed_check_buf_bytes();
// The table of a (scheme, indices) pair, n_idx >= k + t, for both families: the check's parity rows, the basis
// Lagrange rows and the inverse weights (packed_common.h, make_check_table, gives the layout).  hipErrorInvalidValue
// for repeated clerk points: nothing is uploaded and `tab` keeps its key and contents.
hipError_t ensure_check_table(DeviceTable& tab, const uint64_t* indices, uint32_t n_idx, uint32_t k, uint32_t t,
                              uint32_t p, uint32_t omega_secrets, uint32_t omega_shares);
// What every launch of one call shares.  tab: ensure_check_table's words at row stride ks; cnt: the counter block,
// device memory of packed_check_buf_bytes() bytes, of whose log `cap` = min(log_cap, kCheckLogCap) entries are used.
struct CheckGeom {
    uint64_t B, D;            // batches per vector, the dimension
    uint32_t n_idx, kt, k, ks;
    MontP M;
    const uint32_t* tab;
    unsigned long long* cnt;
    uint32_t cap;
};
CheckGeom check_geom(const PackedCheckArgs& a, uint32_t n_idx, uint32_t k, uint32_t t, uint32_t p,
                     const DeviceTable& tab, void* buf, uint32_t log_cap);
// Runs the check as packed_check_plan (check_plan.h) decides it and waits for it: *res and blame_host[n_idx] (written
// only when the location pass ran) are final on return.  At least one batch and one vector, n_idx >= k + t.
hipError_t launch_packed_check(const PackedCheckArgs& a, const CheckGeom& g, hipStream_t s, uint64_t* blame_host,
                               PackedCheckResult* res);
// The location pass alone, over `total` logged batches of g.cnt or with `all` over every batch: a.verdict (when given)
// gets the located positions and the blame words their counts.  Only enqueues.
hipError_t launch_packed_check_locate(const PackedCheckArgs& a, const CheckGeom& g, uint64_t total, bool all,
                                      hipStream_t s);
// The fused first pass (packed_repair_plan: kRepairFused) and its one wait: out holds the reveal of every batch from
// its first k + t shares, a.verdict (when given) the provisional verdicts, *res the counts.
hipError_t launch_packed_repair(const PackedRepairArgs& a, const CheckGeom& g, hipStream_t s, PackedCheckResult* res);
// The same first pass over i64 rows with the recipient's mask (device [n_vectors][dimension], 8-byte aligned)
// subtracted in its write-back (recipient_repair.hip): out[i] = (secret_i - mask_i) mod p in [0, p), every i64 mask
// value reduced exactly.  launch_recipient_unmask is that subtraction as a pass of its own over secrets in [0, p)
// (only enqueues).
hipError_t launch_recipient_repair(const PackedRepairArgs& a, const int64_t* mask, const CheckGeom& g, hipStream_t s,
                                   PackedCheckResult* res);
hipError_t launch_recipient_unmask(const int64_t* secrets, const int64_t* mask, uint64_t D, const MontP& M,
                                   int64_t* out, hipStream_t s);
// What follows a pass that counted res->bad > 0 bad batches into g.cnt, and its wait.  `verdict`: never nullptr (the
// caller's buffer, or zeroed scratch when it gave none).  locate: the location pass first (fused path; the composed
// path's share check has run it).  recompute: every bad batch is first revealed again from its first k + t shares
// (composed path: out holds the reveal from all shares); a batch located at a basis position is corrected either way.
// Fills res->fixed, res->overflowed and, with locate, blame_host[n_idx].
hipError_t launch_packed_repair_fix(const PackedRepairArgs& a, uint16_t* verdict, const CheckGeom& g, bool locate,
                                    bool recompute, hipStream_t s, uint64_t* blame_host, PackedCheckResult* res);

// ---- packed_decode.hip ----
// The decoded reveal's table of a (scheme, indices) pair with r = n_idx - (k + t) >= 2 inside packed_decode_plan's
// scope (decode_tables.h gives the layout).  hipErrorInvalidValue for repeated clerk points, as ensure_check_table.
hipError_t ensure_decode_table(DeviceTable& tab, const uint64_t* indices, uint32_t n_idx, uint32_t k, uint32_t t,
                               uint32_t p, uint32_t omega_secrets, uint32_t omega_shares);
struct PackedDecodeResult {
    uint64_t decoded = 0;     // batches the decode pass walked: the bad ones, or on overflow every batch
    uint64_t undecoded = 0;   // bad batches left at verdict 0xFFFF
    uint32_t max_errors = 0;  // the largest error set of the call
};
// The decode pass behind launch_packed_repair when it counted res->bad > 0 bad batches into g.cnt, and its wait: every
// decodable bad batch gets its corrected secrets in a.out, its |E| in a.verdict and its error set in `wrong` (device
// uint32 [n_vectors][B]; either may be nullptr).  dtab: ensure_decode_table's words.  Fills res->fixed,
// res->overflowed, *dres and blame_host[n_idx].
hipError_t launch_packed_decode(const PackedRepairArgs& a, uint32_t* wrong, const CheckGeom& g, const uint32_t* dtab,
                                hipStream_t s, uint64_t* blame_host, PackedCheckResult* res, PackedDecodeResult* dres);

// ---- codec_decode.hip (share payload codec: sodium.rs:36-41 / :82-88, integer-encoding 1.0 VarInt) ----
// Host-side plan of the decode: blobs are split into 4 KiB regions aligned to the (16-byte
// aligned) byte buffer; a region shared by two blobs appears once per blob.
struct VarintPlan {
    std::vector<uint64_t> blob_region;   // [n_blobs + 1] first region of each blob (prefix sum)
    uint64_t regions = 0;
    uint64_t max_regions = 0;            // regions of the largest blob (grid.x)
};
void varint_plan(const uint64_t* blob_off, uint64_t n_blobs, VarintPlan* plan);
// How the clerk's decode -> combine produced its result (sda_codec_last_launch reports the handle's last one).
// The launchers below fill the part they decide (the slot combine's columns per lane and groups, the fused
// kernel's prefetch depth and variant, the grid slices of a decode pass, the sequential decoder); the engine's
// decode_combine() adds the path it settled on and the attempts it abandoned.
enum CodecPath : uint32_t {
    kCodecNone = 0,           // no decode -> combine yet (or the last one failed, or ran the host streaming path)
    kCodecSlots = 1,          // slot decode + slot_combine_kernel, the whole job in one pass
    kCodecSlotsGrouped = 2,   // the same through one reused slot buffer, `passes` groups of blobs
    kCodecFused = 3,          // varint_decode_combine_kernel<DEPTH, false>
    kCodecFusedMulti = 4,     // varint_decode_combine_kernel<2, true> (an element of >= 6 bytes)
    kCodecMatrix32 = 5,       // count pass + int32 matrix + combine
    kCodecMatrix64 = 6,       // count pass + i64 matrix + combine
};
enum CodecFellBack : uint32_t {
    kCodecSlotWide = 1,       // the slot attempt raised its wide flag and was abandoned
    kCodecFusedIrregular = 2, // fused was asked for but a blob is irregular
    kCodecNarrowWide = 4,     // the int32 matrix decode met a value outside int32 and was abandoned
    kCodecSequential = 8,     // varint_sequential_kernel decoded the irregular blobs
};
struct CodecLaunchInfo {
    uint32_t path = kCodecNone;
    uint32_t width = 0;       // columns per lane of the slot combine (1/2/4) or the fused kernel's DEPTH (2/4/8)
    uint32_t fell_back = 0;   // CodecFellBack bits
    uint64_t passes = 0;      // blob groups (grouped slot path), else <= 65,535-blob grid slices of the decode pass
};
size_t varint_decode_work_bytes(size_t regions, uint64_t n_blobs);
// element count of every blob (synchronous: copies n_blobs counts to the host); long_any: some element
// has >= 6 bytes (sub_counts: also the 256-byte sub-chunk counts of the fused decode -> combine)
hipError_t launch_varint_count(const uint8_t* bytes, const uint64_t* blob_off_host, uint64_t n_blobs,
                               const VarintPlan& plan, void* work, uint64_t* counts_host, bool* irregular_any,
                               hipStream_t s, bool sub_counts = false, bool* long_any = nullptr);
// decode every blob into out + blob * out_stride (after launch_varint_count on the same work)
hipError_t launch_varint_decode(const uint8_t* bytes, uint64_t n_blobs, const VarintPlan& plan, void* work,
                                int64_t* out, uint64_t out_stride, uint64_t len, bool irregular_any,
                                hipStream_t s, CodecLaunchInfo* info = nullptr);
// the same decode into int32 (regular blobs only: the caller checked irregular_any == false); *wide_host
// (synchronous) tells whether some value did not fit, in which case out holds garbage
// sda_varint_decode_dev in one pass of launches: count, scan, a device capacity check (some blob
// decodes to more than out_stride values: nothing is written, *too_long), decode; counts_host[n_blobs]
// and the flag are read at the end of the call (its only wait).
hipError_t launch_varint_decode_one_wait(const uint8_t* bytes, const uint64_t* blob_off_host, uint64_t n_blobs,
                                        const VarintPlan& plan, void* work, int64_t* out, uint64_t out_stride,
                                        uint64_t* counts_host, bool* too_long, hipStream_t s);
hipError_t launch_varint_decode_narrow(const uint8_t* bytes, uint64_t n_blobs, const VarintPlan& plan, void* work,
                                       int32_t* out, uint64_t out_stride, bool* wide_host, hipStream_t s,
                                       CodecLaunchInfo* info = nullptr);
// The clerk's fused decode -> combine (after launch_varint_count with sub_counts on the same work; regular
// blobs of equal element count dim): out[dim] = combiner.rs:16-28 over the decoded blobs in order, each
// payload read once.  tile_plan: device scratch of varint_tile_plan_bytes(n_blobs, dim).  *info (optional, this
// launcher and the decode launchers around it): the part of the record each decides (CodecLaunchInfo); the
// fused kernel's grid is over column tiles, so its `passes` are the grid slices of its tile plan.
uint64_t varint_tile_plan_bytes(uint64_t n_blobs, uint64_t dim);
uint64_t varint_fused_tiles(uint64_t dim);
hipError_t launch_varint_decode_combine(const uint8_t* bytes, uint64_t n_blobs, const VarintPlan& plan, void* work,
                                        uint64_t* tile_plan, uint64_t dim, int64_t* out, int64_t modulus,
                                        bool multi, hipStream_t s, CodecLaunchInfo* info = nullptr);
// The clerk's decode -> combine over region slots (no count pass), in one pass of launches: the payload is
// decoded once into int32 slots per 16 KiB region (slot buffer: varint_slot_bytes), region counts are
// scanned, and combiner.rs:16-28 runs over the slots into out -- unless *flags_host comes back nonzero
// (bit 0: an element longer than 5 bytes or not a field share: use the matrix path; bit 1: the blobs
// decode to different lengths), or blob 0's count exceeds out_cap, or modulus (|m|) is 0: then out is
// untouched.  counts_host[n_blobs] and *flags_host are read at the end of the call (its only wait).
// *job (sda_clerk_job_dev; nullptr: the call above exactly): what a clerk job adds to the pass of launches.
//   continued: `out` holds the state of earlier calls over prior_dim columns and the recurrence continues from it
//     in place; every blob, blob 0 included, has to decode to prior_dim values (else flag bit 1, out untouched),
//     and prior_dim replaces blob 0's bytes as the bound of the grids and of varint_slot_bytes' dim.
//   payload != nullptr: the result is encoded behind the combine (launch_varint_encode_devlen: nothing is stored
//     when a flag is set or the dimension exceeds out_cap); enc_work holds varint_encode_work_bytes(1, bound).
//     Back on the host: encoded = the encode was queued (not for modulus 0 or a bound of 0), enc_chunks its
//     grid, payload_bytes the payload's size (above payload_cap: nothing was written to payload).
// Counts, flags and payload_bytes come back in the call's one copy.
struct SlotJob {
    bool continued = false;
    uint64_t prior_dim = 0;
    uint8_t* payload = nullptr;
    uint64_t payload_cap = 0;
    void* enc_work = nullptr;
    bool encoded = false;
    uint64_t enc_chunks = 0, payload_bytes = 0;
};
size_t varint_slot_bytes(const VarintPlan& plan, uint64_t n_blobs, uint64_t dim);
hipError_t launch_varint_decode_slots_combine(const uint8_t* bytes, const uint64_t* blob_off_host, uint64_t n_blobs,
                                              const VarintPlan& plan, void* work, void* slot_buf, int64_t* out,
                                              uint64_t out_cap, int64_t modulus, uint64_t* counts_host,
                                              uint32_t* flags_host, hipStream_t s, CodecLaunchInfo* info = nullptr,
                                              SlotJob* job = nullptr);
// ---- codec_encode.hip (the same codec's encoder: one size body and one write body over i64 or int32 rows) ----
size_t varint_encode_work_bytes(uint64_t rows, uint64_t len);
// encode rows [rows][stride] (first len elements) back to back into dst; row_bytes_host gets each
// row's byte count (synchronous).  hipErrorInvalidValue if dst_cap is too small.
hipError_t launch_varint_encode(const int64_t* vals, uint64_t rows, uint64_t len, uint64_t stride, uint8_t* dst,
                                uint64_t dst_cap, void* work, uint64_t* row_bytes_host, hipStream_t s);
// The same from int32 rows (stride in int32 elements, vals 4-byte aligned): the bytes of the sign-extended rows.
size_t varint_encode32_work_bytes(uint64_t rows, uint64_t len);
hipError_t launch_varint_encode32(const int32_t* vals, uint64_t rows, uint64_t len, uint64_t stride, uint8_t* dst,
                                  uint64_t dst_cap, void* work, uint64_t* row_bytes_host, hipStream_t s);
// One i64 row whose length the host has not seen (sda_clerk_job_dev): the same four passes, only queued, reading
// the length from *len_dev.  They store nothing when *flags_dev is nonzero or the length exceeds vals_cap; the
// grids and `work` (varint_encode_work_bytes(1, bound) bytes, not the decode's workspace) follow `bound`, which
// the length does not exceed in a clean job.  *total_dev (device) = the payload's bytes; above dst_cap, dst is
// left alone.  *chunks_out (host, optional) = the grid's chunks.
hipError_t launch_varint_encode_devlen(const int64_t* vals, uint64_t vals_cap, const uint64_t* len_dev,
                                       const uint32_t* flags_dev, uint64_t bound, uint8_t* dst, uint64_t dst_cap,
                                       void* work, uint64_t* total_dev, hipStream_t s, uint64_t* chunks_out = nullptr);
uint64_t varint_encode_chunks(uint64_t len);       // chunks of the i64 encoder's grid for a row of len values

// ---- chacha.hip ----
// Combine of n_seeds ChaCha mask streams (chacha.rs:57-76), two implementations:
//  * fast path: counter mode, canonical sums, rejections logged and fixed up.  `work` must hold
//    chacha_work_bytes(D, n_seeds).  Valid when !chacha_needs_stream_path(m); sets *overflow (and writes
//    nothing) when more rejections occur than its log holds -- rerun on the stream path.
//  * stream path: the draws of a tile of streams expanded exactly (any rejection rate) into rows,
//    then the exact sequential combine recurrence (wrapping i64 add for m > 2^62, as the reference).
//    `work` must hold chacha_stream_work_bytes(D, n_seeds, m).  Host-synchronous per tile.
// How a ChaCha launch ran (sda_chacha_last_launch reports the handle's last one).  The fast path's plan is
// recorded where it is decided (chacha_fast_enqueue); the engine adds the stream path and the fix-up count.
enum ChachaPath : uint32_t {
    kChachaNone = 0,          // no ChaCha launch yet
    kChachaDirect = 1,        // fast path, one chunk: chacha_combine_kernel<*, DIRECT> stores the results
    kChachaChunked = 2,       // fast path, grid_y chunks of seeds merged with atomics
    kChachaStreamK = 3,       // fast path, chacha_combine_sk_kernel over grid_y workgroups
    kChachaMaskAdd = 4,       // one stream's masked secrets (chacha_mask_add_kernel)
    kChachaStream = 5,        // exact stream path
    kChachaOverflow = 6,      // fast path whose rejection log overflowed: rerun on the stream path
};
struct ChachaLaunchInfo {
    uint32_t path = kChachaNone;
    uint64_t grid_y = 0;      // chunks (direct, mask add: 1) or the stream-K grid size G; 0 on the stream path
    uint64_t fixups = 0;      // chacha_fix_kernel launches: one per stream with a rejection below D
};
size_t chacha_work_bytes(uint64_t dimension, uint64_t n_seeds);
bool chacha_needs_stream_path(int64_t modulus);
size_t chacha_stream_work_bytes(uint64_t dimension, uint64_t n_seeds, int64_t modulus);
hipError_t launch_chacha_mask_combine(int64_t modulus, uint64_t dimension, const uint32_t* seeds,
                                      uint32_t w, uint64_t n_seeds, int64_t* out, void* work,
                                      hipStream_t s, bool* overflow, int* fixups_out,
                                      ChachaLaunchInfo* info = nullptr);
// The same fast path in two halves, for pipelines that keep queueing work behind it: _async enqueues
// the combine (canonical draws' sums in out, before any fix-up) and copies its rejection count to
// count_host (PINNED host memory, valid once the stream has drained); resolve_ then applies the
// fix-ups for that count (host-synchronous, rare) or sets *overflow (rerun on the stream path).  The
// caller redoes whatever it queued on `out` when the count was nonzero.  *info (optional, every launcher
// below): the plan of the launch, its fixups 0 until a resolve_ counts them (fixups_out).
hipError_t launch_chacha_mask_combine_async(int64_t modulus, uint64_t dimension, const uint32_t* seeds, uint32_t w,
                                            uint64_t n_seeds, int64_t* out, void* work, hipStream_t s,
                                            unsigned long long* count_host, ChachaLaunchInfo* info = nullptr);
// One stream's masked secrets in one pass (chacha.rs:36-45): masked = (secrets + draw) % m, the rejection
// count to count_host (pinned).  A nonzero count means `masked` used rejected draws: the caller redoes
// the mask exactly (launch_chacha_mask_combine, then the add).
hipError_t launch_chacha_mask_add_async(int64_t modulus, uint64_t dimension, const uint32_t* seed, uint32_t w,
                                        const int64_t* secrets, int64_t* masked, void* work, hipStream_t s,
                                        unsigned long long* count_host, ChachaLaunchInfo* info = nullptr);
hipError_t resolve_chacha_mask_combine(int64_t modulus, uint64_t dimension, const uint32_t* seeds, uint32_t w,
                                       uint64_t n_seeds, int64_t* out, void* work, hipStream_t s,
                                       unsigned long long n_rej, bool* overflow, int* fixups_out);
hipError_t launch_chacha_streams_combine(int64_t modulus, uint64_t dimension, const uint32_t* seeds, uint32_t w,
                                         uint64_t n_seeds, int64_t* out, void* work, hipStream_t s);
// mask[i] = gen_range draw i of one stream (chacha.rs:36-39); `work`: chacha_stream_work_bytes(D, 1, m)
hipError_t launch_chacha_stream(int64_t modulus, uint64_t dimension, const uint32_t* seed, uint32_t w,
                                int64_t* mask, void* work, hipStream_t s);

// ---- draws.hip ----
// Elements one workgroup of the draws kernel produces (256 lanes x one ChaCha block of 8 draws); sda_amd/engine.py
// restates it as DRAWS_TILE for the tests' shapes.
constexpr uint32_t kDrawsTile = 2048;
// out[p] = draw(first + p), p < count (device), uniform on [0, bound): ChaCha20 under key_host[8] (HOST words,
// passed as a kernel argument) with state words 14 = stream_id, 15 = retry round (draws.hip gives the rule).
// The caller has checked bound >= 1 and that first + count does not wrap.
hipError_t launch_draws(const uint32_t* key_host, uint32_t stream_id, uint64_t first, uint64_t count, int64_t bound,
                        int64_t* out, hipStream_t s);

// ---- additive_keyed.hip ----
// Columns one workgroup of the fused Additive kernel owns; sda_amd/engine.py restates it as ADDITIVE_KEYED_TILE.
constexpr uint32_t kAdditiveKeyedTile = 512;
// Additive share generation with the draws made in the kernel: column d < D of `secrets` (device) takes draws
// (first_column + d)(n - 1) + j, j < n - 1, of launch_draws' rule at bound = modulus, and share j of it goes to
// out[j * out_stride + d] -- out64, or out32 (int32 rows) when that is given.  The caller has checked n >= 1,
// modulus >= 1 (out32: modulus <= 2^31), out_stride >= D and that (first_column + D)(n - 1) does not wrap.
hipError_t launch_additive_generate_keyed(const uint32_t* key_host, uint32_t stream_id, uint64_t first_column,
                                          const int64_t* secrets, uint64_t D, uint64_t n, int64_t modulus,
                                          int64_t* out64, int32_t* out32, uint64_t out_stride, hipStream_t s);

// ---- mask_keyed.hip ----
// Full masking with the mask drawn in the kernel: for p < count, mask[p] = draw(first + p) of launch_draws' rule at
// bound = modulus -- into mask64, or mask32 (int32 values) when that is given -- and masked[p] =
// (secrets[p] + mask[p]) % modulus as launch_addsub_trem computes it.  All device buffers.  The caller has checked
// modulus >= 1 (mask32: modulus <= 2^31) and that first + count does not wrap.
hipError_t launch_full_mask_keyed(const uint32_t* key_host, uint32_t stream_id, uint64_t first, const int64_t* secrets,
                                  uint64_t count, int64_t modulus, int64_t* masked, int64_t* mask64, int32_t* mask32,
                                  hipStream_t s);

// ---- snapshot.hip ----
// One blob of the snapshot transposition: len bytes from src offset to dst offset.
struct SnapshotCopy {
    uint64_t src, dst, len;
};
uint64_t snapshot_chunk_bytes();
// What the last snapshot transposition on a handle planned and launched (sda_snapshot_last_launch).  The host
// plan (sda_snapshot_transpose_dev) fills blobs, chunks, chunk_bytes and shifts; the launcher reports its grid.
struct SnapshotLaunchInfo {
    uint64_t blobs = 0;        // non-empty blobs planned
    uint64_t chunks = 0;       // their chunks (total_chunks)
    uint64_t grid = 0;         // workgroups launched
    uint64_t chunk_bytes = 0;  // snapshot_chunk_bytes()
    uint32_t shifts = 0;       // bit s: some planned blob has (src - dst) & 15 == s
};
// blobs[n_blobs] (each len >= 1), chunk_start[n_blobs + 1] = exclusive prefix of ceil(len / chunk);
// src/dst 16-byte aligned, src readable 32 bytes past the last blob's end.  *grid (when given): the workgroups
// of the launch the runtime accepted, 0 when there was nothing to launch; a refused launch leaves it.
hipError_t launch_snapshot_transpose(const uint8_t* src, uint8_t* dst, const SnapshotCopy* blobs,
                                     const uint64_t* chunk_start, uint64_t n_blobs, uint64_t total_chunks,
                                     hipStream_t s, uint64_t* grid = nullptr);

// ---- recipient_job.hip ----
// The ChaCha seed payloads of a recipient job: blob b = bytes[blob_off[b], blob_off[b + 1]) is walked by the
// codec's rules and its first kSeedWords values are stored `as u32`, zero padded, into words[b][kSeedWords]
// (16-byte aligned) -- the seed matrix of the ChaCha mask combine at w = kSeedWords.  blob_off_dev: device scratch
// of (n_seeds + 1) * 8 bytes the host offsets are uploaded to.  Queued on s; no wait.
constexpr uint32_t kSeedWords = 8;     // ChaChaRng's key
hipError_t launch_recipient_seeds(const uint8_t* bytes, const uint64_t* blob_off_host, uint64_t n_seeds,
                                  uint64_t* blob_off_dev, uint32_t* words, hipStream_t s);

}  // namespace sda
