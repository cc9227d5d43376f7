// hj_internal.h -- device data layout and kernel launchers of the MI355X
// hash join.  Not part of the public ABI (that is include/hj.h).
//
// Hash table = open addressing with linear probing (north_star), replacing the
// reference's bucket-chained heads + SoA linked list (join_v1.mlir:25-39,
// :213-249).  Two slot layouts:
//
//   wide   : 16-B slot {u64 key, u64 payload}; EMPTY key = INT64_MIN.
//            R rows whose key IS INT64_MIN go to a side list (payload only)
//            and are matched by a side loop whose cost is proportional to
//            the output it produces.
//   narrow : 8-B slot (u32 key << 32 | u32 row id), the reference's i32 key /
//            i32 row-id types (join_v1.mlir:546-549, :604-605).  Row ids are
//            < 2^31, so the all-ones word can never be a real slot: EMPTY.
//
// Both: power-of-two capacity >= 2 * |R| (load factor <= 0.5), slot index =
// top bits of a Fibonacci multiplicative hash, one 64-bit atomicCAS claims a
// slot; duplicate build keys each take their own slot (the reference visits
// every chain node, join_v2.mlir:363-384, so duplicates must all match).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hj_gen.h"

namespace hj {

constexpr unsigned long long kEmptyKey64 = 0x8000000000000000ull;
constexpr unsigned long long kEmptySlot32 = ~0ull;

// Wave64 scans by DPP: row shifts 1, 2, 4, 8 inside each row of 16 lanes,
// then row broadcasts of lane 15 (into rows 1, 3) and lane 31 (into rows 2,
// 3).  A handful of VALU cycles per step, where __shfl_up / __shfl_xor are a
// ds_bpermute (an LDS round trip) each; a wave scanning alone on a
// workgroup's critical path (the partition pass's bin scan, the join's
// output claim) waits for six of them in a row (micro/dpp_micro.hip).
// A lane a DPP step reads from outside the row / mask contributes 0.
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned dpp_or0(unsigned x) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xf, false);
}
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned long long dpp_or0(unsigned long long x) {
    const unsigned lo = dpp_or0<CTRL, ROWS>((unsigned)x), hi = dpp_or0<CTRL, ROWS>((unsigned)(x >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
// inclusive prefix sum over the wave's 64 lanes (all lanes active)
template <typename T>
__device__ __forceinline__ T wave_incl_add_t(T x) {
    x += dpp_or0<0x111, 0xf>(x);   // row_shr:1
    x += dpp_or0<0x112, 0xf>(x);   // row_shr:2
    x += dpp_or0<0x114, 0xf>(x);   // row_shr:4
    x += dpp_or0<0x118, 0xf>(x);   // row_shr:8
    x += dpp_or0<0x142, 0xa>(x);   // row_bcast:15
    x += dpp_or0<0x143, 0xc>(x);   // row_bcast:31
    return x;
}
__device__ __forceinline__ unsigned wave_incl_add(unsigned x) { return wave_incl_add_t(x); }
__device__ __forceinline__ unsigned long long wave_incl_add64(unsigned long long x) { return wave_incl_add_t(x); }
// maximum over the wave's 64 lanes, in every lane (all lanes active)
__device__ __forceinline__ unsigned wave_max_all(unsigned x) {
    auto mx = [](unsigned a, unsigned b) { return a > b ? a : b; };
    x = mx(x, dpp_or0<0x111, 0xf>(x));
    x = mx(x, dpp_or0<0x112, 0xf>(x));
    x = mx(x, dpp_or0<0x114, 0xf>(x));
    x = mx(x, dpp_or0<0x118, 0xf>(x));
    x = mx(x, dpp_or0<0x142, 0xa>(x));
    x = mx(x, dpp_or0<0x143, 0xc>(x));
    return (unsigned)__builtin_amdgcn_readlane((int)x, 63);
}

struct alignas(16) Slot64 {
    unsigned long long key;
    unsigned long long pay;
};

// Device-side table descriptor, passed by value to kernels.
struct TableDev {
    void *slots;                     // Slot64[cap] or u64[cap]
    unsigned long long mask;         // cap - 1
    int shift;                       // 64 - log2(cap)
    unsigned long long *side;        // wide: payloads of INT64_MIN-key rows
    unsigned long long *meta;        // [0] side count, [1] dup-seen flag, [3] slow-tile count, [8..] cursors
};

enum Layout : int { kWide = 0, kNarrow = 1 };

// Source forms of a relation on the device.
// (3 and 4 are the radix passes' own; kKeyRow64, radix_partition only: an
// int64 key column whose payload is the row's index -- the lookup probe's S)
enum SrcForm : int { kCols64 = 0, kPacked64 = 1, kCol32 = 2, kKeyRow64 = 5 };

struct SrcDev {
    const void *key;    // int64 column, packed {key,pay} tuples or int32 column
    const void *pay;    // int64 column (kCols64 only)
    long long n;
    long long row_base; // kCol32: row id = row_base + row
    int form;
};

struct OutDev {
    void *r;            // int64 or int32 column (R payload / row id)
    void *s;            // int64 or int32 column (S payload / row id)
    long long cap;      // rows the caller allocated
    unsigned long long *counter;  // device u64: total match count (all rows, even past cap)
};

// CUs of the current device (hj_radix.hip): asked once per process, then
// remembered -- the devices of one process are taken to be alike
int cu_count();

// launchers (hipError_t of the launch; all asynchronous on `st`)
hipError_t launch_init(const TableDev &t, int layout, unsigned long long cap, hipStream_t st);
hipError_t launch_build(const TableDev &t, int layout, const SrcDev &src, hipStream_t st);
// slow: >= probe_tiles(src.n) words (tiles handed to the general path; the
// count lives in meta[3])
size_t probe_tiles(long long n);
// slow_cap: entries of `slow` (tiles beyond it are never written; the
// callers size it from probe_tiles so that cannot happen)
// marks (launch_probe, launch_probe_outer): non-null for the build-side outer
// probes -- tiles that stay on the fast path set the bits of the slots they
// matched (launch_marks_clear before, launch_unmatched_build after)
hipError_t launch_probe(const TableDev &t, int layout, const SrcDev &src, const OutDev &out,
                        bool count_only, unsigned *slow, size_t slow_cap, hipStream_t st, unsigned *marks = nullptr);
// semi- (anti: anti-) join probe of the global table: out.r = S keys (may be
// null), out.s = S payloads, out.cap == 0 counts only; one launch, no
// general path, meta[1] untouched
hipError_t launch_probe_exists(const TableDev &t, int layout, const SrcDev &src, const OutDev &out, bool anti,
                               hipStream_t st);
// positional lookup over the global table: for S row j, out.r[j] = the
// smallest (signed) payload of the R rows with its key or null_pay, cnt[j] =
// their number (either may be null); out.counter += the S rows with a
// partner.  src: a key column (kCols64 -- its pay is not read -- or kCol32).
// One launch; reads meta[0..1], writes no build state.
hipError_t launch_probe_lookup(const TableDev &t, int layout, const SrcDev &src, const OutDev &out, int *cnt,
                               unsigned long long null_pay, hipStream_t st);
// The as-of probes' order (hj.h "As-of probe"; KIND = HJ_ASOF_* direction |
// strict, a template argument of both kernels): payloads and bounds compare as
// signed int64.  A running best starts at asof_start (the identity of the
// kind's max / min) beside a found bit that alone says whether the set was
// empty: INT64_MIN and INT64_MAX are payloads like any other.
template <int KIND>
__device__ __forceinline__ bool asof_admits(long long p, long long b) {
    if constexpr (KIND == 0) return p <= b;        // backward
    else if constexpr (KIND == 1) return p >= b;   // forward
    else if constexpr (KIND == 2) return p < b;    // backward, strict
    else return p > b;                             // forward, strict
}
template <int KIND>
constexpr long long asof_start = (KIND & 1) ? 0x7fffffffffffffffll : -0x7fffffffffffffffll - 1;
// folds payload p into `best` under bound b; true if p was a candidate
template <int KIND>
__device__ __forceinline__ bool asof_fold(long long p, long long b, long long &best) {
    if (!asof_admits<KIND>(p, b)) return false;
    if constexpr (KIND & 1) best = p < best ? p : best;
    else best = p > best ? p : best;
    return true;
}
// as-of probe over the global table (k_probe_asof): for S row j, out.r[j] =
// the largest payload <= bound[j] (kind HJ_ASOF_*: or the smallest >= it,
// strictly or not) of the R rows with its key, or null_pay; out.counter += the
// S rows with a candidate.  src as launch_probe_lookup's; bound: S's own
// element width (int64 / int32, sign-extended).  Two launches, the first
// zeroing out.counter (kernels only, n == 0 too); reads meta[0..1] and the side
// list, writes no build state.
hipError_t launch_probe_asof(const TableDev &t, int layout, int kind, const SrcDev &src, const void *bound,
                             const OutDev &out, unsigned long long null_pay, hipStream_t st);
// The expand probe's scan (hj_kernels.hip; both strategies): cnt[0..n) are the
// per-row partner counts (launch_probe_lookup's / radix_lookup's cnt column),
// width = cnt, or max(1, cnt) when outer.  off[j] = the widths before row j,
// off[n] = *count = M: exactly n + 1 words, for n == 0 too.  Three launches
// (tile sums, one workgroup over the tile sums, per-tile scan + prefix), no
// workgroup waits on another.  sums: expand_scan_tiles(n) u64.
size_t expand_scan_tiles(long long n);
hipError_t launch_expand_scan(const int *cnt, long long n, bool outer, unsigned long long *sums, long long *off,
                              unsigned long long *count, hipStream_t st);
// The expand probe's fill over the global table (k_probe_expand): the payloads
// of S row j's partners at out_r[off[j] ..), in chain order, null_pay where an
// outer row has none; only positions < cap are written (cap <= 0: no launch).
// src as launch_probe_lookup's.  Reads meta[0..1], writes no build state.
hipError_t launch_probe_expand(const TableDev &t, int layout, const SrcDev &src, const long long *off, void *out_r,
                               long long cap, bool outer, unsigned long long null_pay, hipStream_t st);
// The group probe's result columns (any may be null: neither computed nor
// stored) and its per-slot accumulators of the global table.  Element types by
// layout: wide -- every column int64; narrow -- r, cnt, mn, mx int32 and sum
// int64 (the S value is the row id).
struct GroupOut {
    void *r, *cnt, *sum, *mn, *mx;
    long long cap;                // rows the caller allocated (0: count only)
    unsigned long long *counter;  // device u64: result rows (all of them, even past cap)
    unsigned long long null_val;  // min / max of an empty group
    int all;                      // 0: only the groups with a partner, 1: every R row
};
struct GroupAcc {                 // slots + 1 entries each (the last: the wide INT64_MIN side list's)
    void *cnt;                    // u64 (wide) / u32 (narrow); always present
    unsigned long long *sum;      // null: not asked for
    void *mn, *mx;                // i64 (wide) / i32 (narrow); null: not asked for
};
// group probe over the global table: k_group_init (the accumulators' fill, a
// kernel), k_probe_group (S's rows add into the accumulators of the first slot
// holding their key; src.pay may be null when sum, mn and mx all are) and
// k_emit_groups (one row per R row, compacted through out.counter, which the
// caller zeroed).  Reads the table, the side list and meta[0..1]; writes none.
hipError_t launch_group(const TableDev &t, int layout, const SrcDev &src, const GroupAcc &acc, const GroupOut &out,
                        hipStream_t st);
// Hash aggregate (GROUP BY key) of src over the global table, which the call
// fills itself: launch_init, k_aggregate_init (the accumulators' fill; it also
// zeroes out.counter), k_aggregate (each 2048-row tile
// collapsed in LDS, then one insert-or-find and one atomic per accumulator and
// distinct key of the tile) and k_emit_aggregate (one row per occupied slot,
// compacted through out.counter).  t: 2^bits >= 2 *
// src.n slots; acc as launch_group's (slots + 1 entries; the last is the wide
// INT64_MIN key's).  out.r receives the KEY; out.all and out.null_val are not
// read.  src.pay may be null when acc.sum, acc.mn and acc.mx all are.  The
// table is left holding the keys, not a build: meta[0..1] are zeroed.
hipError_t launch_aggregate(const TableDev &t, int layout, const SrcDev &src, const GroupAcc &acc, const GroupOut &out,
                            hipStream_t st);
// probe-side outer join over the global table: launch_probe's pairs plus
// (null_pay, S payload) for every S row without a partner; out.cap == 0
// counts only; slow / slow_cap as launch_probe's
hipError_t launch_probe_outer(const TableDev &t, int layout, const SrcDev &src, const OutDev &out,
                              unsigned long long null_pay, unsigned *slow, size_t slow_cap, hipStream_t st,
                              unsigned *marks = nullptr);
// build-side outer join over the global table: launch_marks_clear, then
// launch_probe (RIGHT OUTER) or launch_probe_outer (FULL OUTER) with marks,
// then launch_unmatched_build of the same src, out, slow and slow_cap: the
// tiles stage 1 handed to the general path are marked too, and the R rows no
// row of src matches are appended as (R payload, null_s).  marks:
// mark_words(slots) 32-bit words: one bit per slot, then the "src held
// INT64_MIN" word.  out.cap == 0 counts only.
size_t mark_words(unsigned long long slots);
hipError_t launch_marks_clear(const TableDev &t, unsigned *marks, hipStream_t st);
hipError_t launch_unmatched_build(const TableDev &t, int layout, const SrcDev &src, const OutDev &out,
                                  unsigned long long null_s, unsigned *marks, const unsigned *slow, size_t slow_cap,
                                  hipStream_t st);

// ---------------------------------------------------------------- radix join
// (hj_radix.hip) partitions both relations by the top bits of the key hash
// until a partition's build rows fit one workgroup's LDS table, then joins
// partition pairs in LDS.  A pass writes rows into fixed-size buckets (one
// partition per bucket, bucket chaining): no histogram pass, no global scan.
// The radix join's key hash: partitions, passes' bins and LDS slots are its
// bit fields from the top down (odd multiplier: a bijection of the key).
__host__ __device__ __forceinline__ unsigned long long radix_hash(unsigned long long k) {
    return k * 0x9E3779B97F4A7C15ull;
}

struct RadixPlan {
    int passes;       // 1..3 partition passes
    int bits[3];      // fan-out bits per pass (<= 9 each)
    int pbl[3];       // log2 rows per bucket written by each pass
    int total_bits;   // P = 2^total_bits partitions
    int skip = 0;     // top hash bits above the partition bits (the owning GPU of a folded routing)
};

// One pass's output: packed rows in buckets of 2^pbl rows; bucket j holds
// bfill[j] rows of partition bbin[j].  After the pass the rows are listed
// as RUNS of <= 64 consecutive rows of one bucket (row << 7 | count; a
// bucket of f rows gives ceil(f / 64) runs), grouped by partition: p owns
// runs[rstart[p] .. rstart[p+1]).  Consumers map one wave to one run, so a
// partly filled bucket idles at most one wave's tail.
constexpr int kRunLog = 6;
// readable entries past max_runs in a run list: the joins load a wave's
// entries in one scalar load of up to 4, past the list's end included
constexpr int kRunPad = 8;
constexpr int kPassPbl = 10;   // 1024-row buckets for intermediate passes (9: 1 % slower C3 step)
constexpr int kFinalPbl = 9;   // 512-row buckets for the join's input (8 / 9 / 10+9 measured: profiles/r01_bucket_sizes.txt)
struct BucketSet {
    void *rows;                    // >= max_buckets << pbl rows
    unsigned *bbin, *bfill;        // >= max_buckets
    unsigned long long *runs;      // >= max_runs + kRunPad (readable)
    unsigned long long *rstart;    // >= P + 1 (P of the pass writing the set)
    unsigned max_buckets;          // bbin / bfill entries
    unsigned long long max_rows;   // rows entries
    unsigned long long max_runs;   // runs entries (max_rows / 64 + max_buckets covers any fill)
};

struct RadixWork {                 // scratch shared by the partition passes
    BucketSet tmp;                 // ping set of multi-pass plans
    unsigned *nb;                  // device bucket counter
    unsigned long long *pcur;      // >= P + 1: chunk-map scratch
    unsigned long long *rcur;      // >= P + 1: run placement cursors
    unsigned *tile_start;          // >= P + 1
    unsigned *tile_owner;          // >= radix_tiles(n, P)
    void *tdesc;                   // >= radix_tiles(n, P) * 16 B: bucketed-pass tile descriptors
    unsigned *wstart;              // >= 1025: per-workgroup bucket id ranges of a pass
    unsigned long long *scan_sums; // >= P / 8192 + 2
    unsigned long long *scan_state;// >= P / 1024 + 4, zero between calls (the one-launch scan's tile words)
    // 2 x (kRawCntWords): a small pass's raw run counts by pass parity, when
    // the next pass's plan launch scans them itself (null: a scan launch)
    unsigned long long *raw_cnt = nullptr;
    unsigned *work_start = nullptr;   // >= radix_work_words: the joins' work map and deferred-item lists
    void *work_desc = nullptr;        // >= radix_join_items * radix_item_desc_bytes(): their item descriptors
};
constexpr unsigned long long kRawCntWords = 4097;   // kPlanSegs + 1 (hj_radix.hip)

struct RadixNeed {                 // sizes of one bucket set
    unsigned long long buckets, rows;
};

// force_bits > 0: fixed 2^bits partitions; wide: int64 rows (else i32 rows, twice the rows per partition)
RadixPlan radix_plan(long long n_build, int force_bits = 0, bool wide = true);
// Bucket capacity of the final set (`final_set`) or the ping set of plan pl for n rows.
// routed_src > 0: the rows arrive routed from that many sources
// (radix_partition_routed), one run list entry per (source, bin) at least.
RadixNeed radix_need(long long n, const RadixPlan &pl, bool final_set, int routed_src = 0);
unsigned long long radix_tiles(long long n, int max_nseg);
unsigned long long radix_join_items(const RadixPlan &pl, unsigned long long s_runs);
// words of RadixWork::work_start: work map (P + 1 + items), then two
// deferred-item lists (count + items each: the fast join's, the grouped join's)
unsigned long long radix_work_words(const RadixPlan &pl, unsigned long long s_runs);
// Partitioned rows are packed: 16 B {key, pay} (wide) or 8 B key << 32 | row id (narrow).
hipError_t radix_partition(const SrcDev &src, bool wide, const RadixPlan &pl, const RadixWork &ws,
                           const BucketSet &out, hipStream_t st);
size_t radix_item_desc_bytes();
struct JoinOpts {                                 // radix_join's modes
    unsigned long long *dup_flag = nullptr;       // set when the build keys of a built partition repeat
    const unsigned long long *sample = nullptr;   // the build side's {rows, repeats} from radix_sample (device memory; null = "unique")
    bool count_only = false;                      // out.r / out.s are not written
    bool stream = false;                          // the probe side is many times the build side (C2): int64 rows take the larger-sub-chunk shape
    int nparts = -1;                              // >= 0: join that many partitions (r.rstart / s.rstart views of a sub-range), not the plan's 2^total_bits
};
// The kernel that joins follows from (wide, opt.stream, opt.sample) alone:
// join_kernel_choice.  ws.work_start / ws.work_desc are sized for s.max_runs;
// the work-map launch zeroes out.counter.
hipError_t radix_join(bool wide, const RadixPlan &pl, const RadixWork &ws, const BucketSet &r, const BucketSet &s,
                      const OutDev &out, const JoinOpts &opt, hipStream_t st);
// Semi- (anti: anti-) join of the partitioned relations: the S rows with /
// without a partner in r.  out.r (may be null) and out.s receive the S keys
// and payloads (int64, or int32 for narrow rows), out.cap == 0 counts only.
// The work map is radix_join's (no deferred lists); for anti every non-empty
// S partition is an item, build rows or not.  Reads r, writes neither it nor
// the repeat flag.
hipError_t radix_exists(bool wide, bool anti, const RadixPlan &pl, const RadixWork &ws, const BucketSet &r,
                        const BucketSet &s, const OutDev &out, hipStream_t st);
// Positional lookup over the partitioned relations (k_join_lookup).  s was
// partitioned with each row's index in S as its payload (kKeyRow64, or kCol32
// with row_base 0), n = |S|: for S row j, out.r[j] = the smallest (signed)
// payload of the R rows with its key or null_pay, cnt[j] = their number
// (int64 / int32 payloads by width; either output may be null), out.counter =
// the S rows with a partner.  out.cap is ignored: every store is bounded by n.
// radix_exists' anti work map (every non-empty S partition is an item), so
// each row index is written exactly once and nothing needs a prefill.  Reads
// r, writes neither it nor the repeat flag.
hipError_t radix_lookup(bool wide, unsigned long long null_pay, long long n, const RadixPlan &pl, const RadixWork &ws,
                        const BucketSet &r, const BucketSet &s, const OutDev &out, int *cnt, hipStream_t st);
// As-of probe over the partitioned relations (k_join_asof): s partitioned as
// for radix_lookup (each row carries its index in S), n = |S|, bound the S
// column of n bounds in input order (int64 / int32 by width).  For S row j,
// out.r[j] = the best payload under kind (HJ_ASOF_*) and bound[j] among the R
// rows with its key, or null_pay; out.counter = the S rows with a candidate.
// radix_lookup's work map: every row index is written exactly once, nothing
// needs a prefill.  Reads r, writes neither it nor the repeat flag.
hipError_t radix_asof(bool wide, int kind, unsigned long long null_pay, long long n, const void *bound,
                      const RadixPlan &pl, const RadixWork &ws, const BucketSet &r, const BucketSet &s,
                      const OutDev &out, hipStream_t st);
// Expand probe over the partitioned relations: s partitioned as for
// radix_lookup (each row carries its index in S), n = |S|.  One work map
// (radix_lookup's: every non-empty S partition is an item) serves both
// stages: k_join_lookup with the count column alone fills cnt[0..n), then
// launch_expand_scan writes off[0..n] and out.counter = M, then (out.cap > 0)
// k_join_expand stores the payloads of row j's partners at out.r[off[j] ..)
// below out.cap, null_pay where an outer row has none.  sums:
// expand_scan_tiles(n) u64.  Reads r, writes neither it nor the repeat flag.
hipError_t radix_expand(bool wide, bool outer, unsigned long long null_pay, long long n, const RadixPlan &pl,
                        const RadixWork &ws, const BucketSet &r, const BucketSet &s, const OutDev &out, int *cnt,
                        long long *off, unsigned long long *sums, hipStream_t st);
// Group probe over the partitioned relations (k_join_group): one row per R row
// with the count, wrapping sum and signed extremes of the S payloads of its
// key.  The two bucket sets exchanged as in radix_unmatched_build: S's rows are
// aggregated per key in the LDS table, R's rows look their key up and are
// compacted through out.counter (zeroed by the work map).  The map cuts R's
// runs (ws must cover r.max_runs: every build sizes it so); out.all keeps the
// R partitions without S rows.  Reads r and s, writes neither nor the repeat flag.
hipError_t radix_group(bool wide, const RadixPlan &pl, const RadixWork &ws, const BucketSet &r, const BucketSet &s,
                       const GroupOut &out, hipStream_t st);
// Hash aggregate over ONE partitioned relation s (k_join_aggregate): one row
// (key in out.r, count, wrapping sum, signed extremes of the payloads) per
// distinct key, compacted through out.counter (zeroed by the work map); one
// item per non-empty partition, exact whatever a partition holds (an item with
// more distinct keys than its LDS table admits is re-run in sub-splits).
// out.all and out.null_val are not read.  Reads s, writes nothing of it.
hipError_t radix_aggregate(bool wide, const RadixPlan &pl, const RadixWork &ws, const BucketSet &s, const GroupOut &out,
                           hipStream_t st);
// The outer join's second stage, after radix_join over the same r and s (and
// out): the S rows without a partner in r are appended behind the pairs as
// (null_pay, S payload) -- radix_exists' anti probe whose work map leaves
// out.counter as the join left it.  out.cap == 0 counts only.
hipError_t radix_unmatched(bool wide, unsigned long long null_pay, const RadixPlan &pl, const RadixWork &ws,
                           const BucketSet &r, const BucketSet &s, const OutDev &out, hipStream_t st);
// The build-side outer join's last stage, after radix_join (and, FULL OUTER,
// radix_unmatched) over the same r, s and out: the R rows without a partner
// in s are appended as (R payload, null_s).  The same anti stage with the two
// bucket sets exchanged -- s's keys go into the LDS table, r's rows are
// tested and emitted -- over a work map that cuts R's runs into items and
// keeps every non-empty R partition live, S rows or not.  ws.work_start /
// ws.work_desc must cover r.max_runs too (every build sizes them for it).
hipError_t radix_unmatched_build(bool wide, unsigned long long null_s, const RadixPlan &pl, const RadixWork &ws,
                                 const BucketSet &r, const BucketSet &s, const OutDev &out, hipStream_t st);
// Folded routing's send side: rows (int64 columns or packed tuples) grouped
// by the top rbits (<= 9) of radix_hash into out_tuples, exact and contiguous
// per bin, bins in order; counts[2^rbits] their sizes.  One EXACT partition
// pass (k_pass's tiles, line tails and loads) behind a key histogram; hist
// and scan_sums: radix_route_scratch(n, rbits) and exclusive_scan_sums(that)
// u64 each.
size_t radix_route_scratch(long long n, int rbits);
hipError_t radix_route(const SrcDev &src, int rbits, void *out_tuples, unsigned long long *counts,
                       unsigned long long *hist, unsigned long long *scan_sums, hipStream_t st);
// Folded multi-GPU routing: `tuples` (packed int64 {key, payload}) were
// routed by the top pl.skip + pl.bits[0] bits of radix_hash, so they arrive
// already split into the plan's first-pass segments: for each of nsrc sources
// in order, that source's rows of segments 0 .. nseg-1 (cnt[s * nseg + b]
// rows each).  Runs the plan's second pass only (pl.passes == 2) into `out`.
hipError_t radix_partition_routed(const void *tuples, long long n, const unsigned long long *cnt, int nsrc, int nseg,
                                  const RadixPlan &pl, const RadixWork &ws, const BucketSet &out, hipStream_t st);
// Before R's partition: zeroes the radix build's four state words (the side
// count, the repeat flag and the sample) with a kernel.  Not hipMemsetAsync:
// as a node of a captured graph that 32-byte fill was replayed with a stale
// 16-byte pattern (words seen on an MI355X: {garbage, -9, garbage + rows,
// -9 + repeats} where -9 was the caller's own fill value of another tensor),
// which turned the repeat flag on and the kernel choice round.  A kernel's
// arguments travel in its node.
hipError_t radix_state_clear(unsigned long long *meta4, hipStream_t st);
// After R's partition: sample up to 64 build partitions for repeated keys,
// adding {rows sampled, rows whose key repeated} into sample[0..1] (zeroed by
// the caller).  Deterministic for given data.
hipError_t radix_sample(bool wide, const RadixPlan &pl, const BucketSet &r, unsigned long long *sample,
                        hipStream_t st);
// The exact "build keys repeat" answer for the whole build side r (the
// plan's 2^total_bits partitions): k_join_b's DETECT build over one item per
// non-empty partition (a work map rebuilt from r.rstart alone), the
// partitions it cannot take by k_join's list-mode build (repeats inside each
// of its build rounds); sets *dup_flag.  The joins themselves only flag
// repeats of partitions they built (k_join_b: that a probe row met).
hipError_t radix_detect(bool wide, const RadixPlan &pl, const RadixWork &ws, const BucketSet &r,
                        unsigned long long *dup_flag, const unsigned long long *sample, hipStream_t st);
// HJ_JOIN_KERNEL_* of the radix join for this shape and sample (host mirror
// of the device-side choice)
int join_kernel_choice(bool wide, bool stream, unsigned long long rows, unsigned long long repeats);

// Routing fan-out limit: k_part_scatter (> 512 parts) keeps 12 B of LDS
// counters per part, k_part_hist 4 B (<= 96 KiB of the 160 KiB).
constexpr int kMaxRouteParts = 8192;
constexpr int kMaxRouteSources = 64;   // ranks a folded routing's receiver takes rows from
// rbits > 0: parts = the top rbits of radix_hash (nparts = 2^rbits), else an
// fmix64 multiply-shift onto [0, nparts) independent of the radix bits.
hipError_t launch_partition(const SrcDev &src, int nparts, void *out_tuples,
                            unsigned long long *counts, unsigned long long *cursors,
                            hipStream_t st, int rbits = 0);

// exclusive scan of a u64 array in place (hj_radix.hip); sums >= exclusive_scan_sums(len)
hipError_t exclusive_scan_u64(unsigned long long *v, unsigned long long len, unsigned long long *sums,
                              hipStream_t st);
size_t exclusive_scan_sums(unsigned long long len);

// selection (hj_kernels.hip): tiles >= select_tiles(n) + 1 words, sums >= exclusive_scan_sums(tiles)
size_t select_tiles(long long n);
hipError_t launch_select_f32(const float *in, long long n, int op, float c, float *out, long long *out_row,
                             long long cap, unsigned long long *count, unsigned long long *tiles,
                             unsigned long long *sums, hipStream_t st);
hipError_t launch_select_i64(const long long *in, long long n, int op, long long c, long long *out,
                             long long *out_row, long long cap, unsigned long long *count, unsigned long long *tiles,
                             unsigned long long *sums, hipStream_t st);
// copy floors (hj_dev_stream_copy): shape 0 persistent (cus workgroups), 1 flat
hipError_t launch_stream_copy(const void *in, void *out, long long rows, int shape, int cus, hipStream_t st);
// the partition pass's write pattern (buckets of bucket_bytes: 4-16 KiB) vs a
// flat write of the same bytes into a fresh buffer (>= cus x 256 buckets):
// *ratio = pattern time / flat time, ~1.0 at a good physical placement,
// 1.25-1.35 at a bad one (hj_kernels.hip)
hipError_t placement_probe(void *buf, size_t bytes, size_t bucket_bytes, int cus, float *ratio);

// nested-loop.mlir result rows (hj_kernels.hip)
hipError_t launch_key_col_i32(const int *t, long long rows, long long ld, int *out, hipStream_t st);
hipError_t launch_gather_rows_i32(const int *x, long long ldx, int cx, const int *y, long long ldy, int cy,
                                  const int *px, const int *py, const unsigned long long *count, long long cap,
                                  int *out, long long ldo, hipStream_t st);

// ------------------------------------------------------------ composite keys
// (hj_keys.hip) exact range packing of up to four int32 / int64 key columns
// into one int64 key (hj.h "Composite keys").  The plan lives in one device
// block; every kernel reads it there, so a captured sequence replayed over new
// data follows the new data's plan.
constexpr int kKeysMaxCols = 4;
constexpr int kKeysBlock = 256;        // threads per workgroup of the streaming kernels
constexpr int kKeysTile = 2048;        // rows per workgroup and loop step (observe, pack and unpack alike)
constexpr int kKeysGridPerCu = 8;      // the grid is capped at this many workgroups per CU; the loop strides past it
struct KeyPlan {
    long long mn[kKeysMaxCols], mx[kKeysMaxCols];   // observed signed extremes (reset: INT64_MAX / INT64_MIN)
    unsigned long long rows;                        // rows observed
    unsigned long long oor;                         // rows packed with a value outside [lo, hi]
    // the sealed plan
    long long lo[kKeysMaxCols], hi[kKeysMaxCols];
    unsigned long long span[kKeysMaxCols];          // (u64)hi - (u64)lo
    unsigned long long mask[kKeysMaxCols];          // the low bits[c] bits set (0 for a 0-bit column)
    int bits[kKeysMaxCols];
    int shift[kKeysMaxCols];                        // 0 for a 0-bit column: such a column is masked out, never shifted by 64
    int total;                                      // the sum of bits
    int range;                                      // 1: total > 64, pack and unpack write nothing
};
struct KeyCols {                                    // column pointers, by value in the kernel arguments
    const void *p[kKeysMaxCols];
};
struct KeyOutCols {
    void *p[kKeysMaxCols];                          // null: the column is not written
};
// w64: bit c set = column c is int64 (else int32, sign-extended).  All launch
// kernels only; n == 0 launches nothing.
hipError_t keys_reset(KeyPlan *plan, hipStream_t st);
hipError_t keys_observe(KeyPlan *plan, int ncols, unsigned w64, const KeyCols &cols, long long n, hipStream_t st);
hipError_t keys_seal(KeyPlan *plan, int ncols, hipStream_t st);
// out: n keys, or with pay (tuples) 2n words {key, pay}
hipError_t keys_pack(KeyPlan *plan, int ncols, unsigned w64, const KeyCols &cols, const long long *pay, long long n,
                     unsigned long long *out, bool tuples, hipStream_t st);
hipError_t keys_unpack(const KeyPlan *plan, int ncols, unsigned w64, const unsigned long long *key, long long n,
                       const KeyOutCols &out, hipStream_t st);

// ---------------------------------------------------------------- key filter
// (hj_filter.hip) a split-block Bloom filter of a build side's keys (hj.h "Key
// filter"): nblocks blocks of eight uint32 words; a key owns one bit in each
// word of one block.  The placement is one function for the kernels and the
// host (hj_filter_place).
constexpr int kFilterBlock = 256;      // threads per workgroup
constexpr int kFilterTile = 2048;      // rows per workgroup and loop step (insert, count and write alike)
constexpr int kFilterGridPerCu = 8;    // the grid is capped at this many workgroups per CU; the loop strides past it
HJ_HD uint64_t filter_hash(int64_t key) { return fmix64((uint64_t)key ^ 0x9E3779B97F4A7C15ull); }
HJ_HD uint64_t filter_block(uint64_t h, uint64_t nblocks) { return ((h >> 32) * nblocks) >> 32; }   // nblocks < 2^31
HJ_HD uint32_t filter_mask(uint32_t lo, int w) {   // the bit of word w (0..7) for a key whose hash's low word is lo
    constexpr uint32_t salt[8] = {0x47b6137bu, 0x44974d91u, 0x8824ad5bu, 0xa2b7289du,
                                  0x705495c7u, 0x2df1424bu, 0x9efc4947u, 0x5c6bfb31u};
    return 1u << ((uint32_t)(lo * salt[w]) >> 27);
}
struct FilterWork {                    // apply's workspace, owned by the filter object
    unsigned long long *tiles;         // >= filter_tiles(n) + 1 words
    unsigned long long *sums;          // >= exclusive_scan_sums(filter_tiles(n) + 1) words
    unsigned char *bitmap;             // >= filter_bitmap_bytes(n) bytes
};
size_t filter_tiles(long long n);
size_t filter_bitmap_bytes(long long n);
// All launch kernels only.  form: kCols64 (int64 column), kPacked64 (16-byte
// {key, pay} tuples) or kCol32 (int32 column, sign-extended).
hipError_t filter_clear(unsigned *words, long long nblocks, hipStream_t st);
hipError_t filter_insert(unsigned *words, long long nblocks, int form, const void *key, long long n, hipStream_t st);
hipError_t filter_merge(unsigned *words, const unsigned *other, long long nblocks, hipStream_t st);
// kind 0: the rows whose key passes, 1: the others; compacted in input order.
// out_key: int64 keys / 16-byte tuples / int32 keys by form; out_pay: kCols64
// only; out_row: int64 source positions (kCol32: int32 row ids row_base + row).
// Every output may be null; nothing is written at or past cap; *count = all
// qualifying rows.  n == 0 writes the count alone.
hipError_t filter_apply(const unsigned *words, long long nblocks, int form, int kind, const void *key,
                        const long long *pay, long long n, long long row_base, void *out_key, void *out_pay,
                        void *out_row, long long cap, unsigned long long *count, const FilterWork &ws,
                        hipStream_t st);

// ---------------------------------------------------------------- star probe
// (hj_kernels.hip, k_star) n probe rows against up to kStarMaxDims global
// tables of one layout in one kernel (hj.h "Star probe").  Kinds = HJ_STAR_*.
constexpr int kStarMaxDims = 4;
enum StarKind : int { kStarInner = 0, kStarLeft = 1, kStarAnti = 2 };
struct StarDim {
    TableDev t;
    const void *key;                 // this dimension's key column of the probe rows (int64 / int32 by layout)
    void *out;                       // its payload column (int64 / int32; null: not asked for)
    unsigned long long null_pay;     // LEFT: the payload of a row without a partner
    int kind;
    int lds_off;                     // set by star_place: byte offset of the table's copy in dynamic LDS, < 0: global
};
struct StarArgs {                    // by value in the kernel arguments
    StarDim d[kStarMaxDims];
    long long n, row_base, cap;
    void *out_row;                   // int64 positions / int32 row ids (null: not asked for)
    unsigned long long *count;
    unsigned long long *tiles;       // the workspace's tile counts, then offsets
    unsigned char *bitmap;           // the workspace's result bytes
    int first;                       // set by launch_star: the first dimension the launch walks (-1: none)
};
struct StarPlan {                    // host facts of one launch_star
    int launches;
    unsigned grid;                   // of the probe launch (decision, or the keep-all launch)
    long long tiles;
    int lds_dims;                    // bit d: the probe launch reads dimension d's table from LDS
    long long lds_bytes;             // those tables together: its dynamic LDS
};
// Raises the maximum dynamic LDS of every k_star instantiation on the current
// device to kLdsPerCu (a launch above 64 KiB needs it; never under capture).
hipError_t star_prepare();
// Kernels only.  ws: >= filter_tiles(n) + 1 tile words, exclusive_scan_sums of
// that, filter_tiles(n) * kFilterBlock bitmap bytes (the key filter's shape).
// Placement (the probe launch: the decision, or the keep-all launch): the
// tables it walks in ascending size while their sum stays <= kLdsPerCu and
// each is <= kLdsTableBytes; then a persistent grid of as many workgroups as
// that LDS lets a CU hold, else one workgroup per tile.  The write launch walks
// the survivors alone: global tables, one workgroup per tile.
hipError_t launch_star(int layout, int ndims, StarArgs a, const FilterWork &ws, StarPlan *plan, hipStream_t st);
// Star aggregate (hj_kernels.hip, k_star_agg; hj.h "Star aggregate"): GROUP BY
// over the star probe's qualifying rows in one pass.  d[].out is not read.
// The star query's fact side (hj.h "Star query", hj_star_fact): predicates on
// fact columns, the value's second operand and the group key's fact fields.
// Every column has the call's layout (int64 / int32, sign-extended).
constexpr int kStarMaxPreds = 4, kStarMaxFactGroups = 2;
enum StarValueOp : int { kStarValueA = 0, kStarValueAdd = 1, kStarValueSub = 2, kStarValueMul = 3 };
struct StarFact {
    const void *pcol[kStarMaxPreds]; // predicate p admits row j iff (plo <= pcol[j] <= phi) != (pkind == 1)
    long long plo[kStarMaxPreds], phi[kStarMaxPreds];
    int pkind[kStarMaxPreds];
    int npreds;
    int vop;                         // v(j) = sval[j] <vop> vb[j], wrapping int64
    const void *vb;                  // null: vop is kStarValueA, or none of sum / min / max
    const void *fcol[kStarMaxFactGroups];   // the key's fact field f: (fcol[j] - fbase) << fshift
    long long fbase[kStarMaxFactGroups];
    int fshift[kStarMaxFactGroups];
    int nfact;
};
struct StarAggArgs {                 // by value in the kernel arguments
    StarDim d[kStarMaxDims];
    long long gbase[kStarMaxDims];   // the group key's field of dimension d: (payload - gbase) << gshift
    int gshift[kStarMaxDims];        // < 0: the dimension is not part of the key
    int order[kStarMaxDims];         // set by launch_star_aggregate: the walk order, nwalk entries
    int nwalk;
    const void *sval;                // the value column (int64 / int32 by layout); null: none of sum / min / max
    long long n;
    TableDev gt;                     // the group table: wide, 2^k slots; side is not read
    GroupAcc acc;                    // its accumulators (wide), slots + 1 entries
    unsigned long long *counter;     // set by launch_star_aggregate: out.counter, whose bit 63 is the overflow flag
};
struct StarQueryArgs : StarAggArgs { // the FACT instantiations' arguments; the others take StarAggArgs as before
    StarFact f;
};
// Kernels only: the group table's fill, k_aggregate_init (it zeroes
// out.counter), k_star_agg (n > 0) and k_emit_aggregate<kWide>.  Placement by
// star_place, as launch_star's, over the tables the pass walks (INNER, ANTI,
// grouped LEFT), the budget being min(kLdsPerCu, 160 KiB - the kernel's static
// LDS).  out.r is the group key column; every out column is int64.
// star_prepare covers it.
// fact (the star query): the pass is the FACT instantiation over *fact;
// ndims == 0 is then legal: no dimension is walked, no table read, no LDS asked
// for beside the static one.  Null: the star aggregate's own instantiation.
hipError_t launch_star_aggregate(int layout, int ndims, StarAggArgs a, const GroupOut &out, StarPlan *plan,
                                 hipStream_t st, const StarFact *fact = nullptr);
// launches of exclusive_scan_u64 over len words (hj_radix.hip)
int exclusive_scan_launches(unsigned long long len);

hipError_t launch_gen_pkfk(unsigned long long seed, long long NR, unsigned long long hit_thr,
                           long long r0, long long nr, long long *rkey, long long *rpay,
                           long long s0, long long ns, long long *skey, long long *spay,
                           hipStream_t st);
hipError_t launch_gen_zipf(unsigned long long seed, const ZipfParams &z, long long s0, long long ns, long long *skey,
                           long long *spay, hipStream_t st);
hipError_t launch_gen_uniform_i64(unsigned long long seed, unsigned long long stream_id,
                                  long long lo, long long hi, long long i0, long long n,
                                  long long *key, long long *pay, hipStream_t st);
hipError_t launch_gen_uniform_i32(unsigned long long seed, unsigned long long stream_id,
                                  int lo, int hi, long long i0, long long n, int *key,
                                  hipStream_t st);

}  // namespace hj
