// hj_capi.cpp -- the C ABI of libhj.so (declared in include/hj.h).
//
// Host side of the join, C++ over HIP.  It replaces the reference's host
// functions inside join_v1.mlir / join_v2.mlir (@allocateHashTable,
// @initializeHashTable, @buildTable, @countRows, @probeRelation: join_v2.mlir:
// 25-199) and the @main data path (:607-730).  The reference lowers every
// gpu.launch_func to stream create -> module load -> launch -> unload ->
// synchronize -> destroy (join_v2.ll:133-172); here one context keeps its
// workspace and every device phase is an asynchronous launch on the caller's
// stream.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <functional>
#include <thread>
#include <type_traits>
#include <vector>

#include "hj.h"
#include "hj_internal.h"

using hj::kNarrow;
using hj::kWide;

namespace {

thread_local std::string g_err;

int fail(int code, const char *file, int line, const std::string &msg) {
    g_err = std::string(file) + ":" + std::to_string(line) + ": " + msg;
    if (code == HJ_ERR_HIP || code == HJ_ERR_NOMEM) std::fprintf(stderr, "hj: %s\n", g_err.c_str());
    return code;
}

#define HJ_FAIL(code, msg) return fail((code), __FILE__, __LINE__, (msg))
#define HJ_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(HJ_ERR_HIP, __FILE__, __LINE__, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
// A radix call that fails may leave the one-launch scan's tile words set
// (they are zeroed only on allocation, and every completed scan clears
// them): reset them on the stream before reporting the failure.
#define HJ_RADIX(ctx, st, expr)                                                                    \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            if ((ctx)->scan_state.p) (void)hipMemsetAsync((ctx)->scan_state.p, 0, (ctx)->scan_state.bytes, (st)); \
            return fail(HJ_ERR_HIP, __FILE__, __LINE__, std::string(#expr) + ": " + hipGetErrorString(e_)); \
        }                                                                                          \
    } while (0)
#define HJ_TRY(expr)              \
    do {                          \
        int r_ = (expr);          \
        if (r_ != HJ_OK) return r_; \
    } while (0)

int ceil_log2(unsigned long long x) {
    int b = 0;
    while ((1ull << b) < x) ++b;
    return b;
}

// Table capacity for n build rows: power of two >= 2n (load factor <= 0.5),
// at least 16 slots.
int table_bits(int64_t n) {
    const unsigned long long want = 2ull * (unsigned long long)(n > 0 ? n : 1);
    int b = ceil_log2(want);
    return b < 4 ? 4 : b;
}

// HJ_TRACE=1: synchronise and log every phase to stderr (diagnostics).
bool trace_on() {
    static const bool on = getenv("HJ_TRACE") != nullptr;
    return on;
}
void trace(const char *what, hipStream_t st, long long n = -1) {
    if (!trace_on()) return;
    const hipError_t e = hipStreamSynchronize(st);
    std::fprintf(stderr, "hj trace: %s n=%lld -> %s\n", what, n, hipGetErrorString(e));
}

enum Ev { kEvInit0, kEvInit1, kEvBuild1, kEvProbe0, kEvProbeMid, kEvProbe1, kEvPart0, kEvPart1, kEvCount };

// Build sides at least this large use the radix-partitioned join (LDS
// tables); smaller ones a global linear-probing table (HJ_STRATEGY_AUTO).
constexpr int64_t kRadixMinRows = 1ll << 21;
// AUTO with a smaller build side whose global table outgrows one XCD's L2
// (>= 2^18 rows = 8 MiB of slots) also radix-partitions R at build time
// (~20 us); a probe side of >= 2^24 rows then takes the radix join: the
// global probe of a MALL-resident table is latency-bound (~40 G rows/s,
// C2 26.4 ms) while partition + LDS join streams (C2 19.7 ms).
constexpr int64_t kDualMinBuildRows = 1ll << 18;
constexpr int64_t kRadixProbeMinRows = 1ll << 24;
// A probe side KNOWN before the build (hj_ctx_probe_hint) takes the radix
// join alone from these many rows on: 2^22 for build sides of >= 2^20 rows,
// else 2^24 (round 6, profiles/r06/r06sc_strategy_cross.txt: 2^20 x 2^22
// radix 0.204 ms, global 0.233; 2^19 x 2^21 global 0.134, radix 0.166).
// Without a hint the dual build keeps kRadixProbeMinRows: its global table
// is already paid for, and its global probe beats partitioning S below 2^24.
inline int64_t radix_probe_min_rows(int64_t n_build) { return n_build >= (1ll << 20) ? 1ll << 22 : kRadixProbeMinRows; }

struct Buf {
    void *p = nullptr;
    size_t bytes = 0;
};

// Device buffers of one radix bucket set (hj::BucketSet).
struct SetBufs {
    Buf rows, bbin, bfill, runs, rstart;
    unsigned max_buckets = 0;
    unsigned long long max_rows = 0;
    unsigned long long max_runs = 0;
};

}  // namespace

struct hj_ctx {
    int device = 0;
    void *table = nullptr;
    size_t table_bytes = 0;
    unsigned long long *side = nullptr;   // wide-layout side list (INT64_MIN keys)
    size_t side_rows = 0;
    unsigned *marks = nullptr;            // build-side outer probes: one bit per slot + the INT64_MIN word (hj::mark_words)
    size_t mark_words = 0;
    unsigned long long *meta = nullptr;   // [0] side count, [1] dup flag, [8..] partition cursors
    size_t meta_words = 0;
    // current table
    int layout = -1;
    int bits = 0;
    int64_t n_build = 0;
    int strategy = HJ_STRATEGY_AUTO;   // requested
    int radix_bits = 0;                // 0: planner chooses
    int used = 0;                      // HJ_STRATEGY_GLOBAL / _RADIX of the current build
    bool dual = false;                 // global build whose R is ALSO radix-partitioned (probe-time choice)
    int64_t probe_hint = -1;           // expected probe rows (hj_ctx_probe_hint; < 0 unknown)
    int probe_used = -1;               // strategy of the last probe (-1: none since the build)
    // radix-join workspace (hj_radix.hip)
    hj::RadixPlan plan;
    SetBufs rset, sset, tset;   // R and S final partitions, ping set of multi-pass plans
    Buf nb, pcur, rcur, tile_start, tile_owner, tdesc, wstart, work_start, work_desc, scan_sums, scan_state, raw_cnt;
    Buf slow;   // global-table probe: tiles for the general path
    Buf acc_cnt, acc_sum, acc_min, acc_max;   // global-table group probe: per-slot accumulators (hj::GroupAcc)
    Buf exp_cnt, exp_sums;                    // expand probe: per-row int32 partner counts, the scan's tile sums
    Buf rows_kx, rows_ky, rows_px, rows_py;   // row materialisation: key columns, pair row ids
    Buf sel_tiles, sel_sums;                  // selection: per-tile counts (then offsets), scan sums
    Buf route_hist, route_sums;               // folded routing: (bin, workgroup) slot bases, scan sums
    // timing: the records go to event set `cur`.  Accumulating mode
    // (hj_ctx_timing_accumulate) moves to the next set of a ring at every
    // build and reads a set back only when the ring comes round to it again
    // or the totals are asked for, so back-to-back build + probe steps need
    // no host synchronisation between them.
    static constexpr int kEvSets = 64;
    struct EvSet {
        hipEvent_t ev[kEvCount];
        bool rec[4] = {false, false, false, false};
        bool rec_mid = false;
    };
    bool timing = false;
    bool ev_ready = false;   // set 0 created
    int ev_made = 0;         // sets created (1, or all of them once accumulating was asked for)
    bool acc = false;        // accumulating
    int cur = 0;
    EvSet sets[kEvSets];
    double tot[6] = {0, 0, 0, 0, 0, 0};
    long long tot_sets = 0;
    EvSet &evs() { return sets[cur]; }
    // host memref path.  One host thread at a time per context: every host
    // entry point holds host_mu (they share the staging buffers, dcount and
    // host_stream).
    std::mutex host_mu;
    hipStream_t host_stream = nullptr;
    static constexpr int kDbufs = 10;
    void *dbuf[kDbufs] = {};
    size_t dbuf_bytes[kDbufs] = {};
    unsigned long long *dcount = nullptr;
    // count -> probe reuse (join_v1.mlir:110-176: @countRows leaves its table
    // for @probeRelation).  hj_count_* uploads both relations into dbuf[6],
    // dbuf[7], builds, and COUNTS (no pairs); it keeps the built table, the
    // staged probe side and a content digest of each input memref.  The next
    // hj_probe_* digests its memrefs on the host (no upload) and, when both
    // digests match, only probes into M-row buffers and downloads.  Any other
    // build on the context invalidates it.
    struct Digest {
        unsigned long long a = 0, b = 0;
        bool operator==(const Digest &o) const { return a == o.a && b == o.b; }
    };
    struct Memo {
        bool valid = false;
        int layout = -1;
        int64_t nr = 0, ns = 0;
        Digest dr, ds;   // R (keys, payloads), S (keys, payloads)
        int64_t m = 0;
        int reuse = 0;   // HJ_REUSE_* the count ran under
        // HJ_REUSE_EXACT: the count's inputs, compacted (keys, then payloads)
        std::vector<unsigned char> cr, cs;
        // drop the memo; the EXACT-mode copies (GBs at 2^28 rows) give
        // their memory back unless `keep` (a count about to refill them)
        void invalidate(bool keep = false) {
            valid = false;
            if (keep) {
                cr.clear();
                cs.clear();
            } else {
                std::vector<unsigned char>().swap(cr);
                std::vector<unsigned char>().swap(cs);
            }
        }
    } memo;
    long long memo_hits = 0;
    // the last radix probe's shape, for hj_ctx_join_kernel (the kernel itself
    // follows from these and the build-time sample in meta[2..3])
    bool join_ran = false, join_wide = false, join_stream = false;
    bool exists_ran = false;   // the last probe was a radix semi- / anti-join (HJ_JOIN_KERNEL_EXISTS)
    bool lookup_ran = false;   // the last probe was a radix lookup (HJ_JOIN_KERNEL_LOOKUP)
    bool asof_ran = false;     // the last probe was a radix as-of probe (HJ_JOIN_KERNEL_ASOF)
    bool group_ran = false;    // the last probe was a radix group probe (HJ_JOIN_KERNEL_GROUP)
    bool expand_ran = false;   // the last probe was a radix expand (HJ_JOIN_KERNEL_EXPAND)
    bool agg_ran = false;      // an aggregate (hj_dev_aggregate_*) ran since the last build: layout < 0, and used,
                               // plan, bits and n_build describe it
    bool routed = false;   // the current build came from hj_dev_build_routed_i64 (plan.skip owner bits)
    bool dup_checked = false;   // hj_ctx_build_has_duplicates ran its DETECT build for this build
    bool host_building = false;  // host_join's build is running (do_build keeps the memo's input copies)
};

namespace {

int set_device(hj_ctx *c) {
    HJ_HIP(hipSetDevice(c->device));
    return HJ_OK;
}

int ensure_meta(hj_ctx *c, size_t words) {
    if (c->meta_words >= words) return HJ_OK;
    if (c->meta) HJ_HIP(hipFree(c->meta));
    c->meta = nullptr;
    size_t w = words < 64 ? 64 : words;
    if (hipMalloc(&c->meta, w * sizeof(unsigned long long)) != hipSuccess) HJ_FAIL(HJ_ERR_NOMEM, "hipMalloc meta");
    HJ_HIP(hipMemset(c->meta, 0, w * sizeof(unsigned long long)));
    c->meta_words = w;
    return HJ_OK;
}

// with_build = false: the slots alone (an aggregate reads neither the side list nor the mark bitmap)
int ensure_table(hj_ctx *c, int64_t n, int layout, bool with_build = true) {
    const int bits = table_bits(n);
    const size_t need = (size_t(1) << bits) * (layout == kWide ? 16 : 8);
    if (c->table_bytes < need) {
        if (c->table) HJ_HIP(hipFree(c->table));
        c->table = nullptr;
        c->table_bytes = 0;
        if (hipMalloc(&c->table, need) != hipSuccess) HJ_FAIL(HJ_ERR_NOMEM, "hipMalloc table " + std::to_string(need));
        c->table_bytes = need;
    }
    if (!with_build) return ensure_meta(c, 64);
    if (layout == kWide && c->side_rows < (size_t)(n > 0 ? n : 1)) {
        if (c->side) HJ_HIP(hipFree(c->side));
        c->side = nullptr;
        const size_t rows = (size_t)(n > 0 ? n : 1);
        if (hipMalloc(&c->side, rows * 8) != hipSuccess) HJ_FAIL(HJ_ERR_NOMEM, "hipMalloc side list");
        c->side_rows = rows;
    }
    // (with the table, so a reserved context's build-side outer probe allocates nothing)
    const size_t mw = hj::mark_words(1ull << bits);
    if (c->mark_words < mw) {
        if (c->marks) HJ_HIP(hipFree(c->marks));
        c->marks = nullptr;
        c->mark_words = 0;
        if (hipMalloc(&c->marks, mw * sizeof(unsigned)) != hipSuccess) HJ_FAIL(HJ_ERR_NOMEM, "hipMalloc mark bitmap");
        c->mark_words = mw;
    }
    return ensure_meta(c, 64);
}

hj::TableDev table_dev(const hj_ctx *c) {
    hj::TableDev t;
    t.slots = c->table;
    t.mask = (1ull << c->bits) - 1ull;
    t.shift = 64 - c->bits;
    t.side = c->side;
    t.meta = c->meta;
    return t;
}

void record(hj_ctx *c, int ev, hipStream_t st) {
    if (c->timing && c->ev_ready) (void)hipEventRecord(c->evs().ev[ev], st);
}

// ms of one event set's phases: init, build, probe, routing partition,
// probe-side partitioning, join (-1: not recorded)
int set_ms(hj_ctx::EvSet &s, float ms[8]) {
    for (int i = 0; i < 8; ++i) ms[i] = -1.0f;
    auto el = [&](int a, int b, float *out) -> int {
        HJ_HIP(hipEventSynchronize(s.ev[b]));
        HJ_HIP(hipEventElapsedTime(out, s.ev[a], s.ev[b]));
        return HJ_OK;
    };
    if (s.rec[0]) HJ_TRY(el(kEvInit0, kEvInit1, &ms[0]));
    if (s.rec[1]) HJ_TRY(el(kEvInit1, kEvBuild1, &ms[1]));
    if (s.rec[2]) HJ_TRY(el(kEvProbe0, kEvProbe1, &ms[2]));
    if (s.rec[3]) HJ_TRY(el(kEvPart0, kEvPart1, &ms[3]));
    if (s.rec[2]) {
        if (s.rec_mid) {
            HJ_TRY(el(kEvProbe0, kEvProbeMid, &ms[4]));
            HJ_TRY(el(kEvProbeMid, kEvProbe1, &ms[5]));
        } else {
            ms[4] = 0.0f;
            ms[5] = ms[2];
        }
    }
    return HJ_OK;
}

// accumulating mode: add set k's phases to the totals and forget them
int fold_set(hj_ctx *c, int k) {
    hj_ctx::EvSet &s = c->sets[k];
    if (!(s.rec[0] || s.rec[1] || s.rec[2] || s.rec[3])) return HJ_OK;
    float ms[8];
    HJ_TRY(set_ms(s, ms));
    for (int i = 0; i < 6; ++i)
        if (ms[i] > 0.0f) c->tot[i] += ms[i];
    ++c->tot_sets;
    s.rec[0] = s.rec[1] = s.rec[2] = s.rec[3] = s.rec_mid = false;
    return HJ_OK;
}

// a build starts a step: accumulating, it records into the ring's next set
// (summing what that set held first: a ring's length of steps ago)
int timing_advance(hj_ctx *c) {
    if (!c->acc || !c->timing) return HJ_OK;
    c->cur = (c->cur + 1) % hj_ctx::kEvSets;
    return fold_set(c, c->cur);
}

int ensure_buf(Buf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return HJ_OK;
    if (b.p) HJ_HIP(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    if (hipMalloc(&b.p, bytes) != hipSuccess) HJ_FAIL(HJ_ERR_NOMEM, "hipMalloc radix workspace " + std::to_string(bytes));
    b.bytes = bytes;
    return HJ_OK;
}

void free_buf(Buf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

// Placement of the bucket sets' row buffers (the partition passes' only
// destinations).  The passes write each tile's rows as one line into each of
// ~512 open buckets per workgroup, and into some physical placements of a
// buffer that pattern runs 25-35 % slower than a flat write (a property of
// the allocation, bimodal: 4-10 of 12 fresh 6 GiB buffers on one box,
// profiles/r05/r05t_place_micro.txt; the same pass into two such buffers: 1.46
// vs 1.76 ms).  A large row buffer is therefore probed when it is allocated
// (hj::placement_probe: the pass's pattern against a flat write, ~2 ms) and
// redrawn while it is slow: up to kPlaceDraws allocations.  Rejected draws
// are held (so the allocator cannot hand the same memory back), at most
// kPlaceHeld of them at once -- a further reject frees the oldest held one --
// and another draw is taken only while free memory is at least kPlaceSpare
// times the buffer (the same rule as hashjoin.join.placed_rows); the best draw
// is kept and the rest freed.  A buffer whose draws stopped before a good one
// is a give-up, counted (and why) in hj_placement_stats_ex and in every bench
// line.  HJ_PLACEMENT_PROBE=0 turns it off.
// (smaller buffers, and 4-KiB buckets (i32 rows' final sets), probe too short
// a pattern to judge: REF-B's sets were rejected 9 draws in 10 at unchanged
// pass times, profiles/r05/r05y_*)
constexpr size_t kPlaceMinBytes = size_t(1) << 30;
constexpr size_t kPlaceMinBucket = size_t(8) << 10;
constexpr int kPlaceDraws = 24;   // (a box where 86 % of draws were slow: r05_final)
constexpr int kPlaceHeld = 2;     // rejected draws held at once
constexpr size_t kPlaceSpare = 3; // another draw while free memory >= 3 x the buffer
std::atomic<float> g_place_good{1.12f};   // pattern / flat at a good placement: 0.98-1.05
struct PlaceStats {
    long long probes = 0, rejected = 0, gave_up = 0, gave_up_low_mem = 0, held_max = 0;
    double worst_kept = 0.0, last_kept = 0.0;
};
PlaceStats g_place;
std::mutex g_place_mu;

bool placement_probe_on() {
    static const bool on = [] {
        const char *e = getenv("HJ_PLACEMENT_PROBE");
        return !(e && e[0] == '0');
    }();
    return on;
}

int ensure_rows(Buf &b, size_t bytes, size_t bucket_bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return HJ_OK;
    if (bytes < kPlaceMinBytes || bucket_bytes < kPlaceMinBucket || !placement_probe_on()) return ensure_buf(b, bytes);
    free_buf(b);
    const int cus = hj::cu_count();
    const float good = g_place_good.load();
    std::vector<Buf> held;   // rejected draws still held (oldest first)
    Buf best;
    float best_r = 1e30f;
    int draws = 0;
    long long rejected = 0, held_max = 0;
    bool low_mem = false;
    for (; draws < kPlaceDraws; ++draws) {
        if (draws > 0) {
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < kPlaceSpare * bytes) {
                (void)hipGetLastError();
                low_mem = true;
                break;
            }
        }
        Buf cand;
        if (hipMalloc(&cand.p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            low_mem = true;
            break;
        }
        cand.bytes = bytes;
        float r = 0.0f;
        if (hj::placement_probe(cand.p, bytes, bucket_bytes, cus, &r) != hipSuccess) {
            (void)hipGetLastError();
            r = 0.0f;   // no verdict: take it
        }
        Buf rej;
        if (r < best_r) {
            rej = best;
            best = cand;
            best_r = r;
        } else {
            rej = cand;
        }
        if (rej.p) {
            ++rejected;
            held.push_back(rej);
            if ((int)held.size() > kPlaceHeld) {
                free_buf(held.front());
                held.erase(held.begin());
            }
            if ((long long)held.size() > held_max) held_max = (long long)held.size();
        }
        if (best_r <= good) {
            ++draws;
            break;
        }
    }
    for (Buf &x : held) free_buf(x);
    if (!best.p) HJ_FAIL(HJ_ERR_NOMEM, "hipMalloc radix rows " + std::to_string(bytes));
    b = best;
    const bool gave_up = best_r > good;
    {
        std::lock_guard<std::mutex> lk(g_place_mu);
        g_place.probes += draws;
        g_place.rejected += rejected;
        if (gave_up) {
            ++g_place.gave_up;
            if (low_mem) ++g_place.gave_up_low_mem;
        }
        if (held_max > g_place.held_max) g_place.held_max = held_max;
        g_place.last_kept = best_r;
        if (best_r > g_place.worst_kept) g_place.worst_kept = best_r;
    }
    if (trace_on() || (gave_up && low_mem))
        std::fprintf(stderr, "hj %s: rows placement %zu B: %d draw(s), kept pattern/flat %.3f%s\n",
                     trace_on() ? "trace" : "note", bytes, draws, (double)best_r,
                     gave_up ? (low_mem ? " (gave up: free memory below 3x the buffer)" : " (gave up: draws spent)") : "");
    return HJ_OK;
}

int ensure_set(SetBufs &sb, const hj::RadixNeed &need, size_t esz, size_t P, int pbl) {
    if (need.buckets > 0xFFFFFFF0ull) HJ_FAIL(HJ_ERR_CAPACITY, "radix partition: too many buckets");
    HJ_TRY(ensure_rows(sb.rows, (size_t)need.rows * esz, esz << pbl));
    HJ_TRY(ensure_buf(sb.bbin, (size_t)need.buckets * 4));
    HJ_TRY(ensure_buf(sb.bfill, (size_t)need.buckets * 4));
    HJ_TRY(ensure_buf(sb.rstart, (P + 1) * 8));
    // capacity actually held (buffers may be larger than this need)
    size_t cap = sb.bbin.bytes / 4;
    if (sb.bfill.bytes / 4 < cap) cap = sb.bfill.bytes / 4;
    sb.max_buckets = (unsigned)(cap < 0xFFFFFFF0ull ? cap : 0xFFFFFFF0ull);
    sb.max_rows = sb.rows.bytes / esz;
    // a bucket of f rows lists ceil(f / 64) runs: <= rows / 64 + buckets
    HJ_TRY(ensure_buf(sb.runs, (size_t)((sb.max_rows >> hj::kRunLog) + sb.max_buckets + hj::kRunPad) * 8));
    sb.max_runs = sb.runs.bytes / 8 - hj::kRunPad;
    return HJ_OK;
}

hj::BucketSet bucket_set(SetBufs &sb) {
    hj::BucketSet b;
    b.rows = sb.rows.p;
    b.bbin = (unsigned *)sb.bbin.p;
    b.bfill = (unsigned *)sb.bfill.p;
    b.runs = (unsigned long long *)sb.runs.p;
    b.rstart = (unsigned long long *)sb.rstart.p;
    b.max_buckets = sb.max_buckets;
    b.max_rows = sb.max_rows;
    b.max_runs = sb.max_runs;
    return b;
}

// Partition scratch for n rows under plan pl (shared by R and S), plus the
// relation's own final set.  routed_src > 0: the rows come routed from that
// many sources (the run lists then hold an entry per (source, bin) at least).
int ensure_radix_scratch(hj_ctx *c, SetBufs &fin, int64_t n, bool wide, const hj::RadixPlan &pl, int routed_src = 0) {
    const size_t P = size_t(1) << pl.total_bits, esz = wide ? 16 : 8;   // (packed partitioned rows)
    HJ_TRY(ensure_set(fin, hj::radix_need(n, pl, true, routed_src), esz, P, hj::kFinalPbl));
    if (pl.passes > 1) HJ_TRY(ensure_set(c->tset, hj::radix_need(n, pl, false, routed_src), esz, P, hj::kPassPbl));
    HJ_TRY(ensure_buf(c->nb, 16));
    HJ_TRY(ensure_buf(c->pcur, (P + 1) * 8));
    HJ_TRY(ensure_buf(c->rcur, (P + 1) * 8));
    HJ_TRY(ensure_buf(c->tile_start, (P + 1) * 4));
    HJ_TRY(ensure_buf(c->tile_owner, (size_t)hj::radix_tiles(n, (int)P) * 4));
    HJ_TRY(ensure_buf(c->tdesc, (size_t)hj::radix_tiles(n, (int)P) * 16));
    HJ_TRY(ensure_buf(c->wstart, 1025 * 4));
    // work map: P + 1 chunk starts, then the item -> partition owner list
    const size_t items = (size_t)hj::radix_join_items(pl, fin.max_runs);
    // work_start (P + 1) + work_owner (items) + two deferred-item lists (1 + items each)
    HJ_TRY(ensure_buf(c->work_start, (size_t)hj::radix_work_words(pl, fin.max_runs) * 4));
    HJ_TRY(ensure_buf(c->work_desc, items * hj::radix_item_desc_bytes()));
    HJ_TRY(ensure_buf(c->scan_sums, ((P + 1) / 8192 + 2) * 8));
    HJ_TRY(ensure_buf(c->raw_cnt, 2 * hj::kRawCntWords * 8));
    {
        // the one-launch scan's tile words: zero on allocation, and every
        // scan leaves them zero
        const size_t had = c->scan_state.bytes;
        HJ_TRY(ensure_buf(c->scan_state, ((P + 1) / 1024 + 4) * 8));
        if (c->scan_state.bytes != had) HJ_HIP(hipMemset(c->scan_state.p, 0, c->scan_state.bytes));
    }
    return HJ_OK;
}

hj::RadixWork radix_work(hj_ctx *c) {
    hj::RadixWork w;
    w.tmp = bucket_set(c->tset);
    w.nb = (unsigned *)c->nb.p;
    w.pcur = (unsigned long long *)c->pcur.p;
    w.rcur = (unsigned long long *)c->rcur.p;
    w.tile_start = (unsigned *)c->tile_start.p;
    w.tile_owner = (unsigned *)c->tile_owner.p;
    w.tdesc = c->tdesc.p;
    w.wstart = (unsigned *)c->wstart.p;
    w.scan_sums = (unsigned long long *)c->scan_sums.p;
    w.scan_state = (unsigned long long *)c->scan_state.p;
    w.raw_cnt = (unsigned long long *)c->raw_cnt.p;
    w.work_start = (unsigned *)c->work_start.p;
    w.work_desc = c->work_desc.p;
    return w;
}

int choose_strategy(const hj_ctx *c, int64_t n_build) {
    if (c->strategy == HJ_STRATEGY_GLOBAL || c->strategy == HJ_STRATEGY_RADIX) return c->strategy;
    if (n_build >= kRadixMinRows) return HJ_STRATEGY_RADIX;
    if (n_build >= kDualMinBuildRows && c->probe_hint >= radix_probe_min_rows(n_build)) return HJ_STRATEGY_RADIX;
    return HJ_STRATEGY_GLOBAL;
}

// One relation as the radix passes take it: plain, or (counts set) packed
// tuples that arrive routed, split by source and first-pass bin.
struct RadixSrc {
    hj::SrcDev src;
    const uint64_t *counts = nullptr;   // routed: [nsrc][nbins] rows
    int nsrc = 0, nbins = 0;
};

int radix_partition_src(hj_ctx *c, const RadixSrc &in, SetBufs &fin, hipStream_t st) {
    if (in.counts)
        HJ_RADIX(c, st, hj::radix_partition_routed(in.src.key, in.src.n, (const unsigned long long *)in.counts, in.nsrc,
                                                   in.nbins, c->plan, radix_work(c), bucket_set(fin), st));
    else
        HJ_RADIX(c, st, hj::radix_partition(in.src, c->layout == kWide, c->plan, radix_work(c), bucket_set(fin), st));
    return HJ_OK;
}

// A build starts on the context: a new timing step, and what the last build and its probes left is reset.
int begin_build(hj_ctx *c, int layout, int64_t n, int used, bool dual, bool routed, const hj::RadixPlan &plan) {
    HJ_TRY(set_device(c));
    HJ_TRY(ensure_meta(c, 64));
    HJ_TRY(timing_advance(c));
    c->layout = layout;
    c->n_build = n;
    c->used = used;
    c->dual = dual;
    c->routed = routed;
    c->plan = plan;
    c->probe_used = -1;
    c->join_ran = c->exists_ran = c->lookup_ran = c->asof_ran = c->group_ran = c->expand_ran = c->agg_ran = c->dup_checked = false;
    // (hj_count_*'s kept table is gone; a host join's own build keeps the
    // EXACT copies it has just taken of its inputs)
    if (c->host_building) c->memo.valid = false;
    else c->memo.invalidate();
    return HJ_OK;
}

// The radix build under c->plan: R partitioned by the top key-hash bits
// (tables are built per partition in LDS at probe time) and sampled.  The
// build phase ends here unless a global table follows (dual).
int radix_build(hj_ctx *c, const RadixSrc &in, hipStream_t st) {
    const bool wide = c->layout == kWide;
    HJ_TRY(ensure_radix_scratch(c, c->rset, in.src.n, wide, c->plan, in.nsrc));
    record(c, kEvInit0, st);
    // meta[0] side count, [1] dup flag, [2..3] the build-side sample (zeroed by
    // a kernel: a memset node of a captured build was replayed with a stale pattern)
    HJ_HIP(hj::radix_state_clear(c->meta, st));
    record(c, kEvInit1, st);
    trace("build: workspace", st, in.src.n);
    HJ_TRY(radix_partition_src(c, in, c->rset, st));
    // repeated build keys, sampled: decides the join kernel (radix_join)
    HJ_HIP(hj::radix_sample(wide, c->plan, bucket_set(c->rset), c->meta + 2, st));
    trace("build: R partitioned", st, (long long)c->plan.total_bits);
    if (!c->dual) {
        record(c, kEvBuild1, st);
        c->evs().rec[0] = c->evs().rec[1] = c->timing;
    }
    return HJ_OK;
}

int do_build(hj_ctx *c, int layout, const hj::SrcDev &src, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (src.n < 0 || (src.n > 0 && !src.key) || (src.form == hj::kCols64 && src.n > 0 && !src.pay))
        HJ_FAIL(HJ_ERR_ARG, "bad build relation");
    if (layout == kNarrow && src.n > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "i32 row ids: build side must have < 2^31 rows");
    const int used = choose_strategy(c, src.n);
    // (a known probe side settled the strategy in choose_strategy: no dual)
    const bool dual = used == HJ_STRATEGY_GLOBAL && c->strategy == HJ_STRATEGY_AUTO && src.n >= kDualMinBuildRows &&
                      c->probe_hint < 0;
    const bool radix = used == HJ_STRATEGY_RADIX || dual;
    HJ_TRY(begin_build(c, layout, src.n, used, dual, false,
                       radix ? hj::radix_plan(src.n, c->radix_bits, layout == kWide) : c->plan));
    if (radix) {
        HJ_TRY(radix_build(c, RadixSrc{src}, st));
        if (!dual) return HJ_OK;
    }
    HJ_TRY(ensure_table(c, src.n, layout));
    c->bits = table_bits(src.n);
    const hj::TableDev t = table_dev(c);
    if (!dual) record(c, kEvInit0, st);   // (dual: the build phase starts at R's partition)
    HJ_HIP(hj::launch_init(t, layout, 1ull << c->bits, st));
    if (!dual) record(c, kEvInit1, st);
    HJ_HIP(hj::launch_build(t, layout, src, st));
    record(c, kEvBuild1, st);
    c->evs().rec[0] = c->evs().rec[1] = c->timing;
    return HJ_OK;
}

// One probe of the current build, after the entry point's argument checks.
enum ProbeKind { kProbeInner, kProbeCount, kProbeSemi, kProbeAnti, kProbeOuter, kProbeBuild, kProbeFull, kProbeLookup,
                 kProbeGroup, kProbeExpand, kProbeAsof };
struct ProbeReq {
    RadixSrc in;       // S; routed: bins [bin0, bin0 + in.nbins) of the build's first pass
    int bin0 = 0;
    hj::OutDev out;    // inner, outer, build, full: R and S payloads; semi / anti: S keys (may be null) and S payloads;
                       // lookup: out.r the per-row R payload (may be null), out.s unused, out.cap = |S|
    int *out_cnt = nullptr;   // lookup: the per-row partner count (may be null)
    ProbeKind kind = kProbeInner;
    unsigned long long null_pay = 0;   // outer, full, lookup: the R payload of an S row without a partner (outer, full: out.cap == 0 counts only)
    unsigned long long null_s = 0;     // build, full: the S payload of an R row without a partner
    hj::GroupOut grp{};                // group: the result columns, the kind and the null value (its counter is out.counter)
    long long *out_off = nullptr;      // expand: the n + 1 offsets (out.r the values, may be null with out.cap == 0)
    bool expand_outer = false;         // expand: a row without a partner gets one null_pay entry
    const void *bound = nullptr;       // asof: S's bound column (int64 / int32 by layout; out.r the per-row result)
    int asof_kind = 0;                 // asof: HJ_ASOF_* direction | strict
};

// The global-table group probe's accumulators for a table of 2^bits slots (and
// the side list's entry): the count always, the others when asked for.
int ensure_group_acc(hj_ctx *c, int bits, int layout, bool sum, bool mn, bool mx) {
    const size_t entries = (size_t(1) << bits) + 1, small = layout == kWide ? 8 : 4;
    HJ_TRY(ensure_buf(c->acc_cnt, entries * small));
    if (sum) HJ_TRY(ensure_buf(c->acc_sum, entries * 8));
    if (mn) HJ_TRY(ensure_buf(c->acc_min, entries * small));
    if (mx) HJ_TRY(ensure_buf(c->acc_max, entries * small));
    return HJ_OK;
}

// The expand probe's workspace for n probe rows: the count column and the scan's tile sums.
int ensure_expand(hj_ctx *c, int64_t n) {
    HJ_TRY(ensure_buf(c->exp_cnt, (size_t)(n > 0 ? n : 0) * sizeof(int)));
    return ensure_buf(c->exp_sums, hj::expand_scan_tiles(n) * sizeof(unsigned long long));
}

int run_probe(hj_ctx *c, const ProbeReq &q, hipStream_t st) {
    HJ_TRY(set_device(c));
    const hj::SrcDev &src = q.in.src;
    const bool exists = q.kind == kProbeSemi || q.kind == kProbeAnti;
    // outer / full: S's null rows behind the pairs; build / full: then R's
    const bool s_nulls = q.kind == kProbeOuter || q.kind == kProbeFull;
    const bool r_nulls = q.kind == kProbeBuild || q.kind == kProbeFull;
    const bool radix = c->used == HJ_STRATEGY_RADIX || (c->dual && src.n >= kRadixProbeMinRows);
    c->probe_used = radix ? HJ_STRATEGY_RADIX : HJ_STRATEGY_GLOBAL;
    c->join_ran = c->exists_ran = c->lookup_ran = c->asof_ran = c->group_ran = c->expand_ran = false;
    if (q.kind == kProbeExpand) HJ_TRY(ensure_expand(c, src.n));
    if (!radix) {
        // (expand: the scan's last launch stores the counter, nothing reads it before; asof: its launcher zeroes it by a kernel)
        if (q.kind != kProbeExpand && q.kind != kProbeAsof) HJ_HIP(hipMemsetAsync(q.out.counter, 0, sizeof(uint64_t), st));
        record(c, kEvProbe0, st);
        if (q.kind == kProbeExpand) {
            // counts (the lookup's kernel without its payload column), their scan, the fill
            const hj::OutDev cnt_out{nullptr, nullptr, src.n, q.out.counter};
            HJ_HIP(hj::launch_probe_lookup(table_dev(c), c->layout, src, cnt_out, (int *)c->exp_cnt.p, 0ull, st));
            HJ_HIP(hj::launch_expand_scan((const int *)c->exp_cnt.p, src.n, q.expand_outer,
                                          (unsigned long long *)c->exp_sums.p, q.out_off, q.out.counter, st));
            HJ_HIP(hj::launch_probe_expand(table_dev(c), c->layout, src, q.out_off, q.out.r, q.out.cap, q.expand_outer,
                                           q.null_pay, st));
        } else if (exists) {
            HJ_HIP(hj::launch_probe_exists(table_dev(c), c->layout, src, q.out, q.kind == kProbeAnti, st));
        } else if (q.kind == kProbeLookup) {
            HJ_HIP(hj::launch_probe_lookup(table_dev(c), c->layout, src, q.out, q.out_cnt, q.null_pay, st));
        } else if (q.kind == kProbeAsof) {
            HJ_HIP(hj::launch_probe_asof(table_dev(c), c->layout, q.asof_kind, src, q.bound, q.out, q.null_pay, st));
        } else if (q.kind == kProbeGroup) {
            HJ_TRY(ensure_group_acc(c, c->bits, c->layout, q.grp.sum, q.grp.mn, q.grp.mx));
            const hj::GroupAcc acc{c->acc_cnt.p, q.grp.sum ? (unsigned long long *)c->acc_sum.p : nullptr,
                                   q.grp.mn ? c->acc_min.p : nullptr, q.grp.mx ? c->acc_max.p : nullptr};
            HJ_HIP(hj::launch_group(table_dev(c), c->layout, src, acc, q.grp, st));
        } else {
            const size_t slow_cap = hj::probe_tiles(src.n);
            HJ_TRY(ensure_buf(c->slow, slow_cap * sizeof(unsigned)));
            // build / full: stage 1 marks the slots its fast path matched (a bitmap cleared per call)
            unsigned *marks = r_nulls ? c->marks : nullptr;
            if (r_nulls) HJ_HIP(hj::launch_marks_clear(table_dev(c), marks, st));
            if (s_nulls)
                HJ_HIP(hj::launch_probe_outer(table_dev(c), c->layout, src, q.out, q.null_pay, (unsigned *)c->slow.p,
                                              slow_cap, st, marks));
            else
                HJ_HIP(hj::launch_probe(table_dev(c), c->layout, src, q.out,
                                        q.kind == kProbeCount || (r_nulls && q.out.cap == 0), (unsigned *)c->slow.p,
                                        slow_cap, st, marks));
            // then the handed-over tiles are marked, and the unmarked rows emitted behind stage 1's
            if (r_nulls)
                HJ_HIP(hj::launch_unmatched_build(table_dev(c), c->layout, src, q.out, q.null_s, marks,
                                                  (const unsigned *)c->slow.p, slow_cap, st));
        }
    } else {
        // (the work-map kernel zeroes the counter: no memset launch)
        const bool wide = c->layout == kWide;
        trace("probe: enter", st, src.n);
        HJ_TRY(ensure_radix_scratch(c, c->sset, src.n, wide, c->plan, q.in.nsrc));
        trace("probe: workspace", st, (long long)c->sset.max_buckets);
        record(c, kEvProbe0, st);
        if ((q.kind == kProbeLookup || q.kind == kProbeExpand || q.kind == kProbeAsof || (q.kind == kProbeGroup && !src.pay && src.form == hj::kCols64)) && wide) {
            // S's rows carry their index through the passes: the key column alone is read
            // (a group probe without a value column: no aggregate reads the payload)
            RadixSrc in = q.in;
            in.src.form = hj::kKeyRow64;
            in.src.pay = nullptr;
            HJ_TRY(radix_partition_src(c, in, c->sset, st));
        } else {
            HJ_TRY(radix_partition_src(c, q.in, c->sset, st));
        }
        trace("probe: S partitioned", st, src.n);
        record(c, kEvProbeMid, st);
        hj::BucketSet r = bucket_set(c->rset);
        hj::JoinOpts o;
        if (q.in.counts) {
            // bins [bin0, bin0 + nbins): partitions [bin0, bin0 + nbins) << bits[1] of R
            r.rstart += (size_t)q.bin0 << c->plan.bits[1];
            o.nparts = q.in.nbins << c->plan.bits[1];
        }
        if (exists) {
            HJ_RADIX(c, st, hj::radix_exists(wide, q.kind == kProbeAnti, c->plan, radix_work(c), r, bucket_set(c->sset),
                                             q.out, st));
            c->exists_ran = true;
        } else if (q.kind == kProbeLookup) {
            HJ_RADIX(c, st, hj::radix_lookup(wide, q.null_pay, src.n, c->plan, radix_work(c), r, bucket_set(c->sset),
                                             q.out, q.out_cnt, st));
            c->lookup_ran = true;
        } else if (q.kind == kProbeAsof) {
            HJ_RADIX(c, st, hj::radix_asof(wide, q.asof_kind, q.null_pay, src.n, q.bound, c->plan, radix_work(c), r,
                                           bucket_set(c->sset), q.out, st));
            c->asof_ran = true;
        } else if (q.kind == kProbeExpand) {
            HJ_RADIX(c, st, hj::radix_expand(wide, q.expand_outer, q.null_pay, src.n, c->plan, radix_work(c), r,
                                             bucket_set(c->sset), q.out, (int *)c->exp_cnt.p, q.out_off,
                                             (unsigned long long *)c->exp_sums.p, st));
            c->expand_ran = true;
        } else if (q.kind == kProbeGroup) {
            HJ_RADIX(c, st, hj::radix_group(wide, c->plan, radix_work(c), r, bucket_set(c->sset), q.grp, st));
            c->group_ran = true;
        } else {
            // the kernel: a function of (row width, size ratio, build-time sample)
            o.dup_flag = c->meta + 1;
            o.sample = c->meta + 2;
            o.count_only = q.kind == kProbeCount || ((s_nulls || r_nulls) && q.out.cap == 0);
            o.stream = src.n >= 8 * c->n_build;
            HJ_RADIX(c, st, hj::radix_join(wide, c->plan, radix_work(c), r, bucket_set(c->sset), q.out, o, st));
            c->join_ran = true;
            c->join_wide = wide;
            c->join_stream = o.stream;
            // outer: the S rows without a partner, over the same S partition, behind the pairs
            if (s_nulls)
                HJ_RADIX(c, st, hj::radix_unmatched(wide, q.null_pay, c->plan, radix_work(c), r, bucket_set(c->sset),
                                                    q.out, st));
            // build / full: the R rows without a partner, the same stage with the bucket sets exchanged
            // (never after a routed bin-range probe: r is the whole of R's partition here)
            if (r_nulls)
                HJ_RADIX(c, st, hj::radix_unmatched_build(wide, q.null_s, c->plan, radix_work(c), r,
                                                          bucket_set(c->sset), q.out, st));
        }
        trace("probe: joined", st, q.out.cap);
    }
    record(c, kEvProbe1, st);
    c->evs().rec[2] = c->timing;
    c->evs().rec_mid = radix && c->timing;   // kEvProbeMid split the phase (partition | join)
    return HJ_OK;
}

int do_probe(hj_ctx *c, int layout, const hj::SrcDev &src, void *out_r, void *out_s, int64_t cap,
             uint64_t *d_count, bool count_only, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (c->layout != layout) HJ_FAIL(HJ_ERR_STATE, "probe without a matching build");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (src.n < 0 || (src.n > 0 && !src.key)) HJ_FAIL(HJ_ERR_ARG, "bad probe relation");
    if (!count_only && (cap < 0 || (cap > 0 && (!out_r || !out_s)))) HJ_FAIL(HJ_ERR_ARG, "bad output");
    ProbeReq q;
    q.in.src = src;
    q.out = hj::OutDev{out_r, out_s, count_only ? 0 : cap, (unsigned long long *)d_count};
    q.kind = count_only ? kProbeCount : kProbeInner;
    return run_probe(c, q, st);
}

// Semi- / anti-join probe (hj_dev_exists_*): the table, R's partition, the
// side list and the repeat flag meta[1] are only read (meta[1] not even that).
int do_exists(hj_ctx *c, int layout, int kind, const hj::SrcDev &src, void *out_key, void *out_s, int64_t cap,
              uint64_t *d_count, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (kind != HJ_EXISTS_SEMI && kind != HJ_EXISTS_ANTI)
        HJ_FAIL(HJ_ERR_ARG, "kind must be HJ_EXISTS_SEMI or HJ_EXISTS_ANTI");
    if (c->layout != layout) HJ_FAIL(HJ_ERR_STATE, "probe without a matching build");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (src.n < 0 || (src.n > 0 && !src.key)) HJ_FAIL(HJ_ERR_ARG, "bad probe relation");
    if (cap < 0 || (cap > 0 && !out_s) || (cap == 0 && !out_s && out_key)) HJ_FAIL(HJ_ERR_ARG, "bad output");
    ProbeReq q;
    q.in.src = src;
    q.out = hj::OutDev{out_key, out_s, cap, (unsigned long long *)d_count};
    q.kind = kind == HJ_EXISTS_ANTI ? kProbeAnti : kProbeSemi;
    return run_probe(c, q, st);
}

// Positional lookup (hj_dev_lookup_*): one (payload, count) per S row at the
// row's own index.  Reads what do_exists reads and the repeat flag.
int do_lookup(hj_ctx *c, int layout, const hj::SrcDev &src, unsigned long long null_pay, void *out_r, int32_t *out_cnt,
              uint64_t *d_count, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (c->layout != layout) HJ_FAIL(HJ_ERR_STATE, "probe without a matching build");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (src.n < 0 || (src.n > 0 && !src.key)) HJ_FAIL(HJ_ERR_ARG, "bad probe relation");
    if (src.n > 0 && !out_r && !out_cnt)
        HJ_FAIL(HJ_ERR_ARG, "both outputs null (hj_dev_exists_* counts the rows with a partner)");
    if (c->n_build > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "int32 counts: the build side must have < 2^31 rows");
    if (layout == kNarrow && src.n > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "i32 row ids: probe side must have < 2^31 rows");
    ProbeReq q;
    q.in.src = src;
    q.out = hj::OutDev{out_r, nullptr, src.n, (unsigned long long *)d_count};
    q.out_cnt = out_cnt;
    q.kind = kProbeLookup;
    q.null_pay = null_pay;
    return run_probe(c, q, st);
}

// As-of probe (hj_dev_asof_*): per S row the nearest R payload at or before
// (after) the row's bound.  do_lookup's order of checks behind the kind's.
// Reads what do_lookup reads.
int do_asof(hj_ctx *c, int layout, int kind, const hj::SrcDev &src, const void *sbound, unsigned long long null_pay,
            void *out_r, uint64_t *d_count, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (kind < 0 || kind > (HJ_ASOF_FORWARD | HJ_ASOF_STRICT))
        HJ_FAIL(HJ_ERR_ARG, "kind must be HJ_ASOF_BACKWARD or HJ_ASOF_FORWARD, with or without HJ_ASOF_STRICT");
    if (c->layout != layout) HJ_FAIL(HJ_ERR_STATE, "probe without a matching build");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (src.n < 0 || (src.n > 0 && !src.key)) HJ_FAIL(HJ_ERR_ARG, "bad probe relation");
    if (src.n > 0 && !sbound) HJ_FAIL(HJ_ERR_ARG, "null bound column");
    if (src.n > 0 && !out_r) HJ_FAIL(HJ_ERR_ARG, "null output");
    if (layout == kNarrow && src.n > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "i32 row ids: probe side must have < 2^31 rows");
    ProbeReq q;
    q.in.src = src;
    q.out = hj::OutDev{out_r, nullptr, src.n, (unsigned long long *)d_count};
    q.kind = kProbeAsof;
    q.null_pay = null_pay;
    q.bound = sbound;
    q.asof_kind = kind;
    return run_probe(c, q, st);
}

// Expand probe (hj_dev_expand_*): every partner of S row j at out_r[out_off[j] ..
// out_off[j + 1]).  do_lookup's order of checks behind the kind's.  Reads what
// do_lookup reads.
int do_expand(hj_ctx *c, int layout, int kind, const hj::SrcDev &src, unsigned long long null_pay, int64_t *out_off,
              void *out_r, int64_t cap, uint64_t *d_count, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (kind != HJ_EXPAND_INNER && kind != HJ_EXPAND_OUTER)
        HJ_FAIL(HJ_ERR_ARG, "kind must be HJ_EXPAND_INNER or HJ_EXPAND_OUTER");
    if (c->layout != layout) HJ_FAIL(HJ_ERR_STATE, "probe without a matching build");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (src.n < 0 || (src.n > 0 && !src.key)) HJ_FAIL(HJ_ERR_ARG, "bad probe relation");
    if (!out_off) HJ_FAIL(HJ_ERR_ARG, "null offsets (n + 1 int64 words)");
    if (cap < 0 || (cap > 0 && !out_r) || (cap == 0 && out_r)) HJ_FAIL(HJ_ERR_ARG, "bad output");
    if (c->n_build > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "int32 counts: the build side must have < 2^31 rows");
    if (layout == kNarrow && src.n > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "i32 row ids: probe side must have < 2^31 rows");
    ProbeReq q;
    q.in.src = src;
    q.out = hj::OutDev{out_r, nullptr, cap, (unsigned long long *)d_count};
    q.out_off = (long long *)out_off;
    q.expand_outer = kind == HJ_EXPAND_OUTER;
    q.kind = kProbeExpand;
    q.null_pay = null_pay;
    return run_probe(c, q, st);
}

// Group probe (hj_dev_group_*): one row per R row with the aggregates of the S
// rows of its key.  do_probe_full's order of checks; rel_err: the entry point
// found its relation bad.  Any column may be null; out_cap == 0 with all five
// null is the count-only form.  Reads what an inner probe reads.
int do_group(hj_ctx *c, int layout, int kind, const hj::SrcDev &src, const char *rel_err, unsigned long long null_val,
             void *out_r, void *out_cnt, void *out_sum, void *out_min, void *out_max, int64_t cap, uint64_t *d_count,
             hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (kind != HJ_GROUP_MATCHED && kind != HJ_GROUP_ALL)
        HJ_FAIL(HJ_ERR_ARG, "kind must be HJ_GROUP_MATCHED or HJ_GROUP_ALL");
    if (c->layout != layout) HJ_FAIL(HJ_ERR_STATE, "probe without a matching build");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (rel_err) HJ_FAIL(HJ_ERR_ARG, rel_err);
    if (src.n < 0 || (src.n > 0 && !src.key)) HJ_FAIL(HJ_ERR_ARG, "bad probe relation");
    const bool any = out_r || out_cnt || out_sum || out_min || out_max;
    if (cap < 0 || (cap > 0 && !any) || (cap == 0 && any)) HJ_FAIL(HJ_ERR_ARG, "bad output");
    ProbeReq q;
    q.in.src = src;
    q.out = hj::OutDev{nullptr, nullptr, cap, (unsigned long long *)d_count};
    q.kind = kProbeGroup;
    q.grp = hj::GroupOut{out_r, out_cnt, out_sum, out_min, out_max, cap, (unsigned long long *)d_count, null_val,
                         kind == HJ_GROUP_ALL ? 1 : 0};
    return run_probe(c, q, st);
}

// Hash aggregate (hj_dev_aggregate_*): GROUP BY key over one relation.  It
// takes the workspace as a build does (begin_build: a new timing step, the host
// memo dropped) and leaves no build: layout stays -1, so every probe answers
// HJ_ERR_STATE until the next build, while used / plan / bits describe the
// aggregate.  AUTO goes by n alone.  The radix plan is made for n rows; i32
// rows are planned as if there were twice as many, one bit finer than a join's
// plan: k_join_aggregate's table admits 2400 keys per partition whatever the
// row width, the narrow join plan averages 4096 rows.
int aggregate_strategy(const hj_ctx *c, int64_t n) {
    if (c->strategy == HJ_STRATEGY_GLOBAL || c->strategy == HJ_STRATEGY_RADIX) return c->strategy;
    return n >= kRadixMinRows ? HJ_STRATEGY_RADIX : HJ_STRATEGY_GLOBAL;
}
hj::RadixPlan aggregate_plan(const hj_ctx *c, int64_t n, bool wide) {
    return hj::radix_plan(wide ? n : 2 * n, c->radix_bits, wide);
}
int ensure_aggregate(hj_ctx *c, int64_t n, int layout, int used, bool sum, bool mn, bool mx) {
    if (used == HJ_STRATEGY_RADIX)
        return ensure_radix_scratch(c, c->sset, n, layout == kWide, aggregate_plan(c, n, layout == kWide));
    HJ_TRY(ensure_table(c, n, layout, false));
    return ensure_group_acc(c, table_bits(n), layout, sum, mn, mx);
}

int do_aggregate(hj_ctx *c, int layout, const hj::SrcDev &src, const char *rel_err, void *out_key, void *out_cnt,
                 void *out_sum, void *out_min, void *out_max, int64_t cap, uint64_t *d_count, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (rel_err) HJ_FAIL(HJ_ERR_ARG, rel_err);
    if (src.n < 0 || (src.n > 0 && !src.key)) HJ_FAIL(HJ_ERR_ARG, "bad relation");
    const bool any = out_key || out_cnt || out_sum || out_min || out_max;
    if (cap < 0 || (cap > 0 && !any) || (cap == 0 && any)) HJ_FAIL(HJ_ERR_ARG, "bad output");
    HJ_TRY(set_device(c));
    const bool wide = layout == kWide;
    const int used = aggregate_strategy(c, src.n);
    // (the build is dropped before the workspace is touched: sizing it may free
    // the table a global build lives in, and may then fail)
    HJ_TRY(begin_build(c, -1, src.n, used, false, false,
                       used == HJ_STRATEGY_RADIX ? aggregate_plan(c, src.n, wide) : c->plan));
    c->evs().rec[0] = c->evs().rec[1] = c->evs().rec[3] = false;   // (no init, build or routing phase in this step)
    c->evs().rec[2] = c->evs().rec_mid = false;
    HJ_TRY(ensure_aggregate(c, src.n, layout, used, out_sum, out_min, out_max));
    c->agg_ran = true;
    const hj::GroupOut grp{out_key, out_cnt, out_sum, out_min, out_max, cap, (unsigned long long *)d_count, 0ull, 0};
    if (used != HJ_STRATEGY_RADIX) {
        c->bits = table_bits(src.n);
        // (the accumulators' fill zeroes the counter: no memset launch)
        record(c, kEvProbe0, st);
        const hj::GroupAcc acc{c->acc_cnt.p, out_sum ? (unsigned long long *)c->acc_sum.p : nullptr,
                               out_min ? c->acc_min.p : nullptr, out_max ? c->acc_max.p : nullptr};
        HJ_HIP(hj::launch_aggregate(table_dev(c), layout, src, acc, grp, st));
    } else {
        // (the work-map kernel zeroes the counter: no memset launch)
        record(c, kEvProbe0, st);
        hj::SrcDev in = src;
        if (wide && !src.pay && src.form == hj::kCols64) {
            // no aggregate reads the payload: the key column alone is read (the rows carry their index)
            in.form = hj::kKeyRow64;
        }
        HJ_RADIX(c, st, hj::radix_partition(in, wide, c->plan, radix_work(c), bucket_set(c->sset), st));
        trace("aggregate: partitioned", st, src.n);
        record(c, kEvProbeMid, st);
        HJ_RADIX(c, st, hj::radix_aggregate(wide, c->plan, radix_work(c), bucket_set(c->sset), grp, st));
        trace("aggregate: done", st, cap);
    }
    record(c, kEvProbe1, st);
    c->evs().rec[2] = c->timing;
    c->evs().rec_mid = used == HJ_STRATEGY_RADIX && c->timing;
    return HJ_OK;
}

// Probe-side outer join (hj_dev_probe_outer_*): do_probe's checks; out_cap == 0
// with both outputs null is the count-only form.  Reads what an inner probe reads.
int do_probe_outer(hj_ctx *c, int layout, const hj::SrcDev &src, unsigned long long null_pay, void *out_r, void *out_s,
                   int64_t cap, uint64_t *d_count, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (c->layout != layout) HJ_FAIL(HJ_ERR_STATE, "probe without a matching build");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (src.n < 0 || (src.n > 0 && !src.key)) HJ_FAIL(HJ_ERR_ARG, "bad probe relation");
    if (cap < 0 || (cap > 0 && (!out_r || !out_s)) || (cap == 0 && (out_r || out_s))) HJ_FAIL(HJ_ERR_ARG, "bad output");
    ProbeReq q;
    q.in.src = src;
    q.out = hj::OutDev{out_r, out_s, cap, (unsigned long long *)d_count};
    q.kind = kProbeOuter;
    q.null_pay = null_pay;
    return run_probe(c, q, st);
}

// Build-side and full outer join (hj_dev_probe_full_*): do_probe_outer's checks
// behind the kind's; rel_err: the entry point found its relation bad (reported
// in do_probe_outer's order, after the state and the count pointer).
int do_probe_full(hj_ctx *c, int layout, int kind, const hj::SrcDev &src, const char *rel_err,
                  unsigned long long null_r, unsigned long long null_s, void *out_r, void *out_s, int64_t cap,
                  uint64_t *d_count, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (kind != HJ_OUTER_BUILD && kind != HJ_OUTER_FULL)
        HJ_FAIL(HJ_ERR_ARG, "kind must be HJ_OUTER_BUILD or HJ_OUTER_FULL");
    if (c->layout != layout) HJ_FAIL(HJ_ERR_STATE, "probe without a matching build");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (rel_err) HJ_FAIL(HJ_ERR_ARG, rel_err);
    if (src.n < 0 || (src.n > 0 && !src.key)) HJ_FAIL(HJ_ERR_ARG, "bad probe relation");
    if (cap < 0 || (cap > 0 && (!out_r || !out_s)) || (cap == 0 && (out_r || out_s))) HJ_FAIL(HJ_ERR_ARG, "bad output");
    ProbeReq q;
    q.in.src = src;
    q.out = hj::OutDev{out_r, out_s, cap, (unsigned long long *)d_count};
    q.kind = kind == HJ_OUTER_FULL ? kProbeFull : kProbeBuild;
    q.null_pay = null_r;
    q.null_s = null_s;
    return run_probe(c, q, st);
}

int do_partition(hj_ctx *c, const hj::SrcDev &src, int nparts, int64_t *out, uint64_t *d_counts, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (nparts < 1 || nparts > hj::kMaxRouteParts) HJ_FAIL(HJ_ERR_ARG, "nparts must be in [1, 8192]");
    if (src.n < 0 || (src.n > 0 && (!src.key || !out))) HJ_FAIL(HJ_ERR_ARG, "bad partition input");
    if (!d_counts) HJ_FAIL(HJ_ERR_ARG, "null counts");
    HJ_TRY(set_device(c));
    HJ_TRY(ensure_meta(c, 8 + (size_t)nparts));
    record(c, kEvPart0, st);
    HJ_HIP(hj::launch_partition(src, nparts, out, (unsigned long long *)d_counts, c->meta + 8, st));
    record(c, kEvPart1, st);
    c->evs().rec[3] = c->timing;
    return HJ_OK;
}

hj::SrcDev src_cols64(const int64_t *k, const int64_t *p, int64_t n) {
    hj::SrcDev s;
    s.key = k;
    s.pay = p;
    s.n = n;
    s.row_base = 0;
    s.form = hj::kCols64;
    return s;
}
hj::SrcDev src_packed(const int64_t *t, int64_t n) {
    hj::SrcDev s;
    s.key = t;
    s.pay = nullptr;
    s.n = n;
    s.row_base = 0;
    s.form = hj::kPacked64;
    return s;
}
hj::SrcDev src_col32(const int32_t *k, int64_t n, int64_t row_base) {
    hj::SrcDev s;
    s.key = k;
    s.pay = nullptr;
    s.n = n;
    s.row_base = row_base;
    s.form = hj::kCol32;
    return s;
}

// ---------------------------------------------------------------- host path
std::mutex g_default_mu;
std::atomic<int> g_reuse{HJ_REUSE_DIGEST};   // hj_host_set_reuse
std::map<int, hj_ctx *> g_default;

hj_ctx *default_ctx() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::lock_guard<std::mutex> lk(g_default_mu);
    auto it = g_default.find(dev);
    if (it != g_default.end()) return it->second;
    hj_ctx *c = hj_ctx_create(dev);
    if (c) g_default[dev] = c;
    return c;
}

// nested-loop.mlir (:29-192, @main :195-289) as a hash join plus a row
// gather.  Roles as %table_1_or_2_as_inner (:247): the larger table is the
// outer X (ties: t1), the smaller the inner Y; every pair X[i][0] == Y[j][0]
// yields the row [X[i][0 .. cx), Y[j][1 .. cy)].  Y is the build side (i32
// keys, payload = row id), X probes; pair row ids are staged in ctx buffers
// and k_gather_rows_i32 writes the rows (<= cap of them; *d_count = M).
struct RowTables {
    const int32_t *t1;
    int64_t r1, c1, ld1;
    const int32_t *t2;
    int64_t r2, c2, ld2;
};

int do_join_rows(hj_ctx *c, const RowTables &a, int32_t *out, int64_t ldo, int64_t cap, uint64_t *d_count,
                 bool count_only, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (a.r1 < 0 || a.r2 < 0 || a.c1 < 1 || a.c2 < 1 || a.ld1 < a.c1 || a.ld2 < a.c2)
        HJ_FAIL(HJ_ERR_ARG, "bad table shape");
    if ((a.r1 > 0 && !a.t1) || (a.r2 > 0 && !a.t2)) HJ_FAIL(HJ_ERR_ARG, "null table");
    if (a.r1 > 0x7fffffffll || a.r2 > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "i32 row ids: tables must have < 2^31 rows");
    const bool t2_outer = a.r1 < a.r2;   // nested-loop.mlir:247
    const int32_t *x = t2_outer ? a.t2 : a.t1, *y = t2_outer ? a.t1 : a.t2;
    const int64_t rx = t2_outer ? a.r2 : a.r1, cx = t2_outer ? a.c2 : a.c1, ldx = t2_outer ? a.ld2 : a.ld1;
    const int64_t ry = t2_outer ? a.r1 : a.r2, cy = t2_outer ? a.c1 : a.c2, ldy = t2_outer ? a.ld1 : a.ld2;
    const int64_t oc = cx + cy - 1;
    if (!count_only && (cap < 0 || (cap > 0 && (!out || ldo < oc)))) HJ_FAIL(HJ_ERR_ARG, "bad row output");
    HJ_TRY(set_device(c));
    HJ_TRY(ensure_buf(c->rows_kx, (size_t)(rx > 0 ? rx : 1) * 4));
    HJ_TRY(ensure_buf(c->rows_ky, (size_t)(ry > 0 ? ry : 1) * 4));
    int32_t *kx = (int32_t *)c->rows_kx.p, *ky = (int32_t *)c->rows_ky.p;
    HJ_HIP(hj::launch_key_col_i32(x, rx, ldx, kx, st));
    HJ_HIP(hj::launch_key_col_i32(y, ry, ldy, ky, st));
    HJ_TRY(do_build(c, kNarrow, src_col32(ky, ry, 0), st));
    if (count_only) return do_probe(c, kNarrow, src_col32(kx, rx, 0), nullptr, nullptr, 0, d_count, true, st);
    HJ_TRY(ensure_buf(c->rows_px, (size_t)(cap > 0 ? cap : 1) * 4));
    HJ_TRY(ensure_buf(c->rows_py, (size_t)(cap > 0 ? cap : 1) * 4));
    int32_t *px = (int32_t *)c->rows_px.p, *py = (int32_t *)c->rows_py.p;
    // R payload = Y row, S payload = X row
    HJ_TRY(do_probe(c, kNarrow, src_col32(kx, rx, 0), py, px, cap, d_count, false, st));
    HJ_HIP(hj::launch_gather_rows_i32(x, ldx, (int)cx, y, ldy, (int)cy, px, py, (const unsigned long long *)d_count,
                                      cap, out, ldo, st));
    return HJ_OK;
}

// Experiments/selection.mlir (:34-155) generalised: survivors of v <op> c,
// order-preserving, optional source row ids.
template <class V>
int do_select(hj_ctx *c, const V *in, int64_t n, int op, V value, V *out, int64_t *out_row, int64_t cap,
              uint64_t *d_count, hipStream_t st) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (n < 0 || (n > 0 && !in)) HJ_FAIL(HJ_ERR_ARG, "bad selection input");
    if (op < HJ_CMP_LT || op > HJ_CMP_NE) HJ_FAIL(HJ_ERR_ARG, "unknown comparison");
    if (cap < 0 || (cap > 0 && !out)) HJ_FAIL(HJ_ERR_ARG, "bad selection output");
    HJ_TRY(set_device(c));
    const size_t nt = hj::select_tiles(n) + 1;
    HJ_TRY(ensure_buf(c->sel_tiles, nt * 8));
    HJ_TRY(ensure_buf(c->sel_sums, hj::exclusive_scan_sums(nt) * 8));
    hipError_t e;
    if constexpr (std::is_same<V, float>::value)
        e = hj::launch_select_f32(in, n, op, value, out, (long long *)out_row, cap, (unsigned long long *)d_count,
                                  (unsigned long long *)c->sel_tiles.p, (unsigned long long *)c->sel_sums.p, st);
    else
        e = hj::launch_select_i64((const long long *)in, n, op, (long long)value, (long long *)out,
                                  (long long *)out_row, cap, (unsigned long long *)d_count,
                                  (unsigned long long *)c->sel_tiles.p, (unsigned long long *)c->sel_sums.p, st);
    HJ_HIP(e);
    return HJ_OK;
}

int dbuf(hj_ctx *c, int i, size_t bytes, void **p) {
    if (bytes == 0) bytes = 16;
    if (c->dbuf_bytes[i] < bytes) {
        if (c->dbuf[i]) HJ_HIP(hipFree(c->dbuf[i]));
        c->dbuf[i] = nullptr;
        c->dbuf_bytes[i] = 0;
        if (hipMalloc(&c->dbuf[i], bytes) != hipSuccess) HJ_FAIL(HJ_ERR_NOMEM, "hipMalloc staging");
        c->dbuf_bytes[i] = bytes;
    }
    *p = c->dbuf[i];
    return HJ_OK;
}

// Copy a strided host memref (aligned + offset, size, stride) into device
// buffer `dst` (contiguous).  shared.cpp reads through the aligned pointer
// (shared.cpp:40, :67, :148); we additionally honour offset and stride.
// (a plain pageable copy: a page-locked staging mirror of d2h below ran the
// count's 537-MB upload slower, 20-21 -> 25-26 ms, profiles/r05/r05zi_*)
template <class T>
int upload(void *dst, const T *aligned, int64_t off, int64_t size, int64_t stride, hipStream_t st) {
    if (size <= 0) return HJ_OK;
    if (!aligned) HJ_FAIL(HJ_ERR_ARG, "null memref");
    const T *base = aligned + off;
    if (stride == 1) {
        HJ_HIP(hipMemcpyAsync(dst, base, sizeof(T) * (size_t)size, hipMemcpyHostToDevice, st));
        HJ_HIP(hipStreamSynchronize(st));
        return HJ_OK;
    }
    std::vector<T> tmp((size_t)size);
    for (int64_t i = 0; i < size; ++i) tmp[(size_t)i] = base[i * stride];
    HJ_HIP(hipMemcpyAsync(dst, tmp.data(), sizeof(T) * (size_t)size, hipMemcpyHostToDevice, st));
    HJ_HIP(hipStreamSynchronize(st));
    return HJ_OK;
}

int host_stream(hj_ctx *c) {
    if (!c->host_stream) HJ_HIP(hipStreamCreateWithFlags(&c->host_stream, hipStreamNonBlocking));
    if (!c->dcount) {
        if (hipMalloc(&c->dcount, 64) != hipSuccess) HJ_FAIL(HJ_ERR_NOMEM, "hipMalloc counter");
    }
    return HJ_OK;
}

// ---- content digests of host memrefs (count -> probe reuse)
// 128 bits from four multiply-rotate lanes over the elements' bytes (lane j
// takes every 4th 8-B word), cut into up to 8 chunks hashed on host threads;
// a changed element changes its lane's state, which no later word undoes
// except by a crafted value.  Memory-bound: ~2^29 B (two 2^24-row int64
// relations) in ~10 ms, overlapped with the upload in hj_count_*.
typedef hj_ctx::Digest Digest;
inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t dstep(uint64_t h, uint64_t w) { return rotl64((h ^ w) * 0x9E3779B97F4A7C15ull, 31); }
inline uint64_t fmix(uint64_t k) {
    k ^= k >> 33;
    k *= 0xFF51AFD7ED558CCDull;
    k ^= k >> 33;
    k *= 0xC4CEB9FE1A85EC53ull;
    return k ^ (k >> 33);
}

Digest digest_mem(const void *aligned, int64_t off, int64_t size, int64_t stride, int esz) {
    Digest d;
    d.a = fmix((uint64_t)size * 16 + (uint64_t)esz);
    d.b = fmix(d.a ^ 0x5EEDull);
    if (size <= 0 || !aligned) return d;
    const char *base = (const char *)aligned + off * esz;
    const int64_t bytes = size * esz;
    const unsigned hw = std::thread::hardware_concurrency();
    unsigned T = (unsigned)(bytes >> 22) + 1;   // >= 4 MiB per thread
    if (T > 8) T = 8;
    if (hw && T > hw) T = hw;
    std::vector<Digest> part(T);
    auto work = [&](unsigned t) {
        const int64_t e0 = size * t / T, e1 = size * (t + 1) / T;
        uint64_t h[4] = {0x243F6A8885A308D3ull, 0x13198A2E03707344ull, 0xA4093822299F31D0ull, 0x082EFA98EC4E6C89ull};
        if (stride == 1) {
            const char *p = base + e0 * esz;
            const size_t n = (size_t)(e1 - e0) * (size_t)esz;
            size_t i = 0;
            for (; i + 32 <= n; i += 32) {
                uint64_t w[4];
                std::memcpy(w, p + i, 32);
                for (int j = 0; j < 4; ++j) h[j] = dstep(h[j], w[j]);
            }
            uint64_t w[4] = {0, 0, 0, 0};
            std::memcpy(w, p + i, n - i);
            for (int j = 0; j < 4; ++j) h[j] = dstep(h[j], w[j] ^ (uint64_t)(n - i));
        } else {
            for (int64_t e = e0; e < e1; ++e) {
                uint64_t w = 0;
                std::memcpy(&w, base + e * stride * esz, (size_t)esz);
                h[e & 3] = dstep(h[e & 3], w);
            }
        }
        part[t].a = fmix(h[0]) ^ fmix(h[1] + 0x9E3779B97F4A7C15ull);
        part[t].b = fmix(h[2]) ^ fmix(h[3] + 0x9E3779B97F4A7C15ull);
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
    for (unsigned t = 0; t < T; ++t) {
        d.a = fmix(d.a ^ part[t].a) + t;
        d.b = fmix(d.b ^ part[t].b) + t;
    }
    return d;
}

// ---- exact copies (HJ_REUSE_EXACT): the count keeps the inputs' bytes,
// compacted; the probe compares its memrefs with them (same threading as
// digest_mem: up to 8 host threads, >= 4 MiB each).
template <class F>
void chunked(int64_t size, int esz, F &&work) {
    const unsigned hw = std::thread::hardware_concurrency();
    unsigned T = (unsigned)((size * esz) >> 22) + 1;
    if (T > 8) T = 8;
    if (hw && T > hw) T = hw;
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back(work, size * t / T, size * (t + 1) / T);
    work((int64_t)0, size / T);
    for (auto &x : th) x.join();
}

void gather_mem(const void *aligned, int64_t off, int64_t size, int64_t stride, int esz, unsigned char *dst) {
    if (size <= 0 || !aligned) return;
    const char *base = (const char *)aligned + off * esz;
    chunked(size, esz, [&](int64_t e0, int64_t e1) {
        if (stride == 1) std::memcpy(dst + e0 * esz, base + e0 * esz, (size_t)(e1 - e0) * (size_t)esz);
        else
            for (int64_t e = e0; e < e1; ++e) std::memcpy(dst + e * esz, base + e * stride * esz, (size_t)esz);
    });
}

bool same_mem(const void *aligned, int64_t off, int64_t size, int64_t stride, int esz, const unsigned char *ref) {
    if (size <= 0) return true;
    if (!aligned) return false;
    const char *base = (const char *)aligned + off * esz;
    std::atomic<bool> diff{false};
    chunked(size, esz, [&](int64_t e0, int64_t e1) {
        bool d = false;
        if (stride == 1) d = std::memcmp(ref + e0 * esz, base + e0 * esz, (size_t)(e1 - e0) * (size_t)esz) != 0;
        else
            for (int64_t e = e0; e < e1 && !d; ++e) d = std::memcmp(ref + e * esz, base + e * stride * esz, (size_t)esz) != 0;
        if (d) diff = true;
    });
    return !diff;
}

// One host relation of the memref ABI: a key column and (int64 rows) an
// optional payload column (null: payload = row id, the reference's rowId,
// join_v1.mlir:255).
struct HostRel {
    const void *k;
    int64_t k_off, k_stride;
    const void *p;
    int64_t p_off, p_stride;
    int64_t n;
};

void copy_rel(const HostRel &r, int esz, std::vector<unsigned char> &out) {
    const size_t col = (size_t)(r.n > 0 ? r.n : 0) * (size_t)esz;
    out.resize(col * (r.p ? 2 : 1));
    gather_mem(r.k, r.k_off, r.n, r.k_stride, esz, out.data());
    if (r.p) gather_mem(r.p, r.p_off, r.n, r.p_stride, esz, out.data() + col);
}

bool same_rel(const HostRel &r, int esz, const std::vector<unsigned char> &ref) {
    const size_t col = (size_t)(r.n > 0 ? r.n : 0) * (size_t)esz;
    if (ref.size() != col * (r.p ? 2 : 1)) return false;
    return same_mem(r.k, r.k_off, r.n, r.k_stride, esz, ref.data()) &&
           (!r.p || same_mem(r.p, r.p_off, r.n, r.p_stride, esz, ref.data() + col));
}

Digest digest_rel(const HostRel &r, int esz) {
    Digest d = digest_mem(r.k, r.k_off, r.n, r.k_stride, esz);
    if (r.p) {
        const Digest e = digest_mem(r.p, r.p_off, r.n, r.p_stride, esz);
        d.a = fmix(d.a ^ e.a);
        d.b = fmix(d.b ^ e.b) + 1;
    }
    return d;
}

// Relation r into device buffer dst (keys, then int64 payloads: given or
// row ids); the device source of the join.
int upload_rel(hj_ctx *c, int layout, const HostRel &r, void *dst, hj::SrcDev *src) {
    hipStream_t st = c->host_stream;
    if (layout == kNarrow) {
        HJ_TRY(upload<int32_t>(dst, (const int32_t *)r.k, r.k_off, r.n, r.k_stride, st));
        *src = src_col32((const int32_t *)dst, r.n, 0);
        return HJ_OK;
    }
    void *dp = (char *)dst + 8 * (size_t)r.n;
    HJ_TRY(upload<int64_t>(dst, (const int64_t *)r.k, r.k_off, r.n, r.k_stride, st));
    if (r.p) {
        HJ_TRY(upload<int64_t>(dp, (const int64_t *)r.p, r.p_off, r.n, r.p_stride, st));
    } else if (r.n > 0) {
        std::vector<int64_t> iota((size_t)r.n);
        for (int64_t i = 0; i < r.n; ++i) iota[(size_t)i] = i;
        HJ_TRY(upload<int64_t>(dp, iota.data(), 0, r.n, 1, st));
    }
    *src = src_cols64((const int64_t *)dst, (const int64_t *)dp, r.n);
    return HJ_OK;
}

// Probe into dbuf[2] / dbuf[3] sized optimistically (|S| rows, or the known
// M), once more at the exact M when that was too small; *m = M.
int host_probe_all(hj_ctx *c, int layout, const hj::SrcDev &probe, size_t esz, int64_t guess, int64_t *m) {
    hipStream_t st = c->host_stream;
    int64_t cap = guess > 0 ? guess : 1;
    uint64_t cnt = 0;
    for (int pass = 0; pass < 2; ++pass) {
        void *o_r, *o_s;
        HJ_TRY(dbuf(c, 2, esz * (size_t)cap, &o_r));
        HJ_TRY(dbuf(c, 3, esz * (size_t)cap, &o_s));
        HJ_TRY(do_probe(c, layout, probe, o_r, o_s, cap, (uint64_t *)c->dcount, false, st));
        HJ_HIP(hipMemcpyAsync(&cnt, c->dcount, 8, hipMemcpyDeviceToHost, st));
        HJ_HIP(hipStreamSynchronize(st));
        if (cnt >> 63) HJ_FAIL(HJ_ERR_CAPACITY, "probe: internal work list overflow (count flagged)");
        if ((int64_t)cnt <= cap) break;
        cap = (int64_t)cnt;   // exact M known: second pass fits
    }
    *m = (int64_t)cnt;
    return HJ_OK;
}

// Joins a std::thread on every exit path.
struct Joiner {
    std::thread t;
    ~Joiner() {
        if (t.joinable()) t.join();
    }
};

// Host-memref join (the reference's @main data path, join_v2.mlir:627-696).
//   kHostCount: upload, build, COUNT (no pairs); remember the inputs'
//               digests (computed while uploading) -- @countRows.
//   kHostProbe: if both memrefs digest as the last count's, probe the kept
//               table with the staged probe side into M-row buffers (no
//               upload, no build) -- @probeRelation; else the whole join.
//               The digests run on host threads WHILE the kept table is
//               probed and, through `deliver`, the pairs are downloaded into
//               the caller's outputs (speculatively: changed inputs then get
//               the whole join, whose pairs are delivered again).
//   kHostJoin:  the whole join (one-memref-out C interface), no memo.
// Pairs land in dbuf[2], dbuf[3] (not for kHostCount); *m = M.
enum HostMode { kHostCount, kHostProbe, kHostJoin };
typedef std::function<int(const void *, const void *, int64_t)> Deliver;
int host_join(hj_ctx *c, int layout, const HostRel &r, const HostRel &s, HostMode mode, int64_t *m, void **d_or,
              void **d_os, const Deliver *deliver = nullptr, bool *delivered = nullptr) {
    if (r.n < 0 || s.n < 0) HJ_FAIL(HJ_ERR_ARG, "negative memref size");
    HJ_TRY(set_device(c));
    HJ_TRY(host_stream(c));
    hipStream_t st = c->host_stream;
    const int esz = layout == kWide ? 8 : 4;
    hj_ctx::Memo &mm = c->memo;
    const int reuse = g_reuse.load();
    // a memo an EXACT count left on this context after the mode moved on:
    // its input copies (GBs at 2^28 rows) go now (hj_host_set_reuse frees
    // those of the default contexts at once; user contexts' here)
    if (mm.reuse == HJ_REUSE_EXACT && reuse != HJ_REUSE_EXACT && (!mm.cr.empty() || !mm.cs.empty())) mm.invalidate();
    Digest dr, ds;
    bool same_r = false, same_s = false;   // HJ_REUSE_EXACT: byte-equal to the count's inputs
    if (delivered) *delivered = false;
    if (mode == kHostProbe && mm.valid && mm.reuse == reuse && reuse != HJ_REUSE_OFF && mm.layout == layout &&
        mm.nr == r.n && mm.ns == s.n) {
        int rc = HJ_OK;
        int64_t mp = 0;
        bool sent = false;
        {
            Joiner dig_r, dig_s;
            if (reuse == HJ_REUSE_EXACT) {
                dig_r.t = std::thread([&] { same_r = same_rel(r, esz, mm.cr); });
                dig_s.t = std::thread([&] { same_s = same_rel(s, esz, mm.cs); });
            } else {
                dig_r.t = std::thread([&] { dr = digest_rel(r, esz); });
                dig_s.t = std::thread([&] { ds = digest_rel(s, esz); });
            }
            const hj::SrcDev src = layout == kWide
                                       ? src_cols64((const int64_t *)c->dbuf[7], (const int64_t *)c->dbuf[7] + s.n, s.n)
                                       : src_col32((const int32_t *)c->dbuf[7], s.n, 0);
            rc = host_probe_all(c, layout, src, (size_t)esz, mm.m, &mp);
            if (rc == HJ_OK && deliver && mp == mm.m) {
                const int d = (*deliver)(c->dbuf[2], c->dbuf[3], mp);   // (1: outputs of another size, not sent)
                sent = d == HJ_OK;
                if (d < 0) rc = d;
            }
        }
        if (rc != HJ_OK) return rc;
        if (reuse == HJ_REUSE_EXACT ? (same_r && same_s) : (dr == mm.dr && ds == mm.ds)) {
            ++c->memo_hits;
            *m = mp;
            *d_or = c->dbuf[2];
            *d_os = c->dbuf[3];
            if (delivered) *delivered = sent;
            return HJ_OK;
        }
    }
    mm.invalidate(mode == kHostCount && reuse == HJ_REUSE_EXACT);
    const size_t rb = (size_t)(layout == kWide ? 16 : 4) * (size_t)r.n;
    const size_t sb = (size_t)(layout == kWide ? 16 : 4) * (size_t)s.n;
    void *dr_buf, *ds_buf;
    HJ_TRY(dbuf(c, 6, rb, &dr_buf));
    HJ_TRY(dbuf(c, 7, sb, &ds_buf));
    hj::SrcDev rsrc, ssrc;
    {
        Joiner dig;
        if (mode == kHostCount && reuse == HJ_REUSE_DIGEST) dig.t = std::thread([&] {   // overlapped with the upload
            dr = digest_rel(r, esz);
            ds = digest_rel(s, esz);
        });
        else if (mode == kHostCount && reuse == HJ_REUSE_EXACT) dig.t = std::thread([&] {
            copy_rel(r, esz, mm.cr);
            copy_rel(s, esz, mm.cs);
        });
        HJ_TRY(upload_rel(c, layout, r, dr_buf, &rsrc));
        HJ_TRY(upload_rel(c, layout, s, ds_buf, &ssrc));
    }
    c->host_building = true;
    const int64_t hint = c->probe_hint;
    c->probe_hint = s.n;
    const int brc = do_build(c, layout, rsrc, st);
    c->probe_hint = hint;
    c->host_building = false;
    HJ_TRY(brc);
    if (mode != kHostCount) {
        HJ_TRY(host_probe_all(c, layout, ssrc, (size_t)esz, s.n, m));
        *d_or = c->dbuf[2];
        *d_os = c->dbuf[3];
        return HJ_OK;
    }
    uint64_t cnt = 0;
    HJ_TRY(do_probe(c, layout, ssrc, nullptr, nullptr, 0, (uint64_t *)c->dcount, true, st));
    HJ_HIP(hipMemcpyAsync(&cnt, c->dcount, 8, hipMemcpyDeviceToHost, st));
    HJ_HIP(hipStreamSynchronize(st));
    // (a flagged count is an error, never a row count -- and never memoised)
    if (cnt >> 63) HJ_FAIL(HJ_ERR_CAPACITY, "count: internal work list overflow (count flagged)");
    mm.layout = layout;
    mm.nr = r.n;
    mm.ns = s.n;
    mm.dr = dr;
    mm.ds = ds;
    mm.m = (int64_t)cnt;
    mm.reuse = reuse;
    mm.valid = reuse != HJ_REUSE_OFF;
    *m = (int64_t)cnt;
    *d_or = *d_os = nullptr;
    return HJ_OK;
}

HostRel rel32(const int32_t *k, int64_t off, int64_t n, int64_t stride) { return HostRel{k, off, stride, nullptr, 0, 1, n}; }
HostRel rel64(const int64_t *k, int64_t k_off, int64_t k_stride, const int64_t *p, int64_t p_off, int64_t p_stride,
              int64_t n) {
    return HostRel{k, k_off, k_stride, p, p_off, p_stride, n};
}

// ---- device -> pageable host memory through page-locked staging.  A plain
// hipMemcpy into a pageable buffer (the caller's memref) ran at ~17 GB/s
// (bench host_memref: 2 x 134 MB in 16 ms); here 32-MiB chunks are DMA'd into
// one of two page-locked buffers while the host copies the previous chunk out
// with up to 8 threads (chunked).  The staging pairs are process-wide, taken
// from a free list (concurrent host joins each take their own pair); a pair's
// events belong to the device that was current when it was made, so a pair
// is only handed out again on that device (an event recorded on
// another device's stream is an invalid handle).
constexpr size_t kStageChunk = size_t(32) << 20;
constexpr size_t kStageMin = size_t(16) << 20;   // below this: one plain copy
struct Staging {
    void *p[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    int dev = -1;
};
std::mutex g_stage_mu;
std::vector<Staging *> g_stage_free;

Staging *stage_take() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        for (size_t i = 0; i < g_stage_free.size(); ++i) {
            if (g_stage_free[i]->dev != dev) continue;
            Staging *s = g_stage_free[i];
            g_stage_free.erase(g_stage_free.begin() + (std::ptrdiff_t)i);
            return s;
        }
    }
    Staging *s = new Staging;
    s->dev = dev;
    bool ok = true;
    for (int i = 0; i < 2 && ok; ++i) {
        ok = hipHostMalloc(&s->p[i], kStageChunk, hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&s->ev[i], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        for (int i = 0; i < 2; ++i) {
            if (s->p[i]) (void)hipHostFree(s->p[i]);
            if (s->ev[i]) (void)hipEventDestroy(s->ev[i]);
        }
        delete s;
        return nullptr;
    }
    return s;
}

void stage_give(Staging *s) {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    g_stage_free.push_back(s);
}

int d2h(void *dst, const void *src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return HJ_OK;
    Staging *sg = bytes >= kStageMin ? stage_take() : nullptr;
    if (!sg) {
        HJ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
        HJ_HIP(hipStreamSynchronize(st));
        return HJ_OK;
    }
    const size_t nch = (bytes + kStageChunk - 1) / kStageChunk;
    auto len_of = [&](size_t i) { return i + 1 < nch ? kStageChunk : bytes - i * kStageChunk; };
    auto issue = [&](size_t i) -> hipError_t {
        hipError_t e = hipMemcpyAsync(sg->p[i & 1], (const char *)src + i * kStageChunk, len_of(i),
                                      hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipEventRecord(sg->ev[i & 1], st);
        return e;
    };
    hipError_t e = issue(0);
    for (size_t i = 0; i < nch && e == hipSuccess; ++i) {
        // chunk i + 1 lands in the buffer chunk i - 1 was copied out of
        if (i + 1 < nch) e = issue(i + 1);
        if (e == hipSuccess) e = hipEventSynchronize(sg->ev[i & 1]);
        if (e != hipSuccess) break;
        char *out = (char *)dst + i * kStageChunk;
        const char *in = (const char *)sg->p[i & 1];
        chunked((int64_t)len_of(i), 1, [&](int64_t a, int64_t b) { std::memcpy(out + a, in + a, (size_t)(b - a)); });
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(st);   // (nothing left in flight into the staging)
    stage_give(sg);
    HJ_HIP(e);
    return HJ_OK;
}

// Device column -> strided host memref.
template <class T>
int download(T *aligned, int64_t off, int64_t size, int64_t stride, const void *src, hipStream_t st) {
    if (size <= 0) return HJ_OK;
    if (!aligned) HJ_FAIL(HJ_ERR_ARG, "null output memref");
    T *base = aligned + off;
    if (stride == 1) return d2h(base, src, sizeof(T) * (size_t)size, st);
    std::vector<T> tmp((size_t)size);
    HJ_TRY(d2h(tmp.data(), src, sizeof(T) * (size_t)size, st));
    for (int64_t i = 0; i < size; ++i) base[i * stride] = tmp[(size_t)i];
    return HJ_OK;
}

// Interleave two device columns into a malloc'ed memref<?x2xT> descriptor.
template <class T, class D>
int fill_result(D *res, const void *d_r, const void *d_s, int64_t m, hipStream_t st) {
    std::memset(res, 0, sizeof(D));
    T *buf = (T *)std::malloc(sizeof(T) * 2 * (size_t)(m > 0 ? m : 1));
    if (!buf) HJ_FAIL(HJ_ERR_NOMEM, "malloc result");
    if (m > 0) {
        std::vector<T> a((size_t)m), b((size_t)m);
        int rc = d2h(a.data(), d_r, sizeof(T) * (size_t)m, st);
        if (rc == HJ_OK) rc = d2h(b.data(), d_s, sizeof(T) * (size_t)m, st);
        if (rc != HJ_OK) {
            std::free(buf);   // (the descriptor stays empty: allocated == NULL)
            return rc;
        }
        for (int64_t i = 0; i < m; ++i) {
            buf[2 * i] = a[(size_t)i];
            buf[2 * i + 1] = b[(size_t)i];
        }
    }
    res->allocated = buf;
    res->aligned = buf;
    res->offset = 0;
    res->sizes[0] = m;
    res->sizes[1] = 2;
    res->strides[0] = 2;
    res->strides[1] = 1;
    return HJ_OK;
}

}  // namespace

namespace {

// Upload a strided 2-D host memref (aligned + offset, sizes, strides) as a
// contiguous row-major rows x cols block.
int upload2(void *dst, const int32_t *aligned, int64_t off, int64_t rows, int64_t cols, int64_t s0, int64_t s1,
            hipStream_t st) {
    if (rows <= 0 || cols <= 0) return HJ_OK;
    if (!aligned) HJ_FAIL(HJ_ERR_ARG, "null memref");
    const int32_t *base = aligned + off;
    if (s1 == 1 && s0 == cols) {
        HJ_HIP(hipMemcpyAsync(dst, base, sizeof(int32_t) * (size_t)(rows * cols), hipMemcpyHostToDevice, st));
    } else {
        std::vector<int32_t> tmp((size_t)(rows * cols));
        for (int64_t i = 0; i < rows; ++i)
            for (int64_t j = 0; j < cols; ++j) tmp[(size_t)(i * cols + j)] = base[i * s0 + j * s1];
        HJ_HIP(hipMemcpyAsync(dst, tmp.data(), sizeof(int32_t) * tmp.size(), hipMemcpyHostToDevice, st));
        HJ_HIP(hipStreamSynchronize(st));
        return HJ_OK;
    }
    HJ_HIP(hipStreamSynchronize(st));
    return HJ_OK;
}

// Host-memref row join: tables copied in, rows materialised on the device
// into staging buffer dbuf[4] (M x oc, contiguous); *m = M, *oc_out = columns.
int host_join_rows(hj_ctx *c, const int32_t *a1, int64_t o1, int64_t r1, int64_t c1, int64_t s10, int64_t s11,
                   const int32_t *a2, int64_t o2, int64_t r2, int64_t c2, int64_t s20, int64_t s21, bool count_only,
                   int64_t *m, int64_t *oc_out, void **d_out) {
    if (r1 < 0 || r2 < 0 || c1 < 1 || c2 < 1) HJ_FAIL(HJ_ERR_ARG, "bad memref shape");
    HJ_TRY(set_device(c));
    HJ_TRY(host_stream(c));
    hipStream_t st = c->host_stream;
    void *d1, *d2;
    HJ_TRY(dbuf(c, 0, sizeof(int32_t) * (size_t)(r1 * c1), &d1));
    HJ_TRY(dbuf(c, 1, sizeof(int32_t) * (size_t)(r2 * c2), &d2));
    HJ_TRY(upload2(d1, a1, o1, r1, c1, s10, s11, st));
    HJ_TRY(upload2(d2, a2, o2, r2, c2, s20, s21, st));
    const RowTables t{(const int32_t *)d1, r1, c1, c1, (const int32_t *)d2, r2, c2, c2};
    *oc_out = c1 + c2 - 1;
    uint64_t cnt = 0;
    HJ_TRY(do_join_rows(c, t, nullptr, 0, 0, (uint64_t *)c->dcount, true, st));
    HJ_HIP(hipMemcpyAsync(&cnt, c->dcount, 8, hipMemcpyDeviceToHost, st));
    HJ_HIP(hipStreamSynchronize(st));
    *m = (int64_t)cnt;
    if (count_only) return HJ_OK;
    HJ_TRY(dbuf(c, 4, sizeof(int32_t) * (size_t)(*m > 0 ? *m * *oc_out : 1), d_out));
    HJ_TRY(do_join_rows(c, t, (int32_t *)*d_out, *oc_out, *m, (uint64_t *)c->dcount, false, st));
    HJ_HIP(hipStreamSynchronize(st));
    return HJ_OK;
}

}  // namespace

extern "C" {

int hj_abi_version(void) { return HJ_ABI_VERSION; }

int hj_device_info(int device, int64_t out[8]) {
    if (!out) HJ_FAIL(HJ_ERR_ARG, "null output");
    hipDeviceProp_t p;
    HJ_HIP(hipGetDeviceProperties(&p, device));
    out[0] = p.multiProcessorCount;
    out[1] = p.memoryClockRate;   // kHz
    out[2] = p.memoryBusWidth;    // bits
    out[3] = p.l2CacheSize;
    out[4] = (int64_t)p.totalGlobalMem;
    out[5] = p.clockRate;         // kHz
    out[6] = (int64_t)p.maxSharedMemoryPerMultiProcessor;
    // HBM3E: 4 transfers per reported memory clock (MI355X reports 2.0 GHz
    // and 8192 bits: 8 Gb/s per pin, 8.19 TB/s -- the 8.0 TB/s spec)
    out[7] = (int64_t)(4.0 * (double)p.memoryClockRate * 1e3 * (double)p.memoryBusWidth / 8.0 / 1e6);   // MB/s
    return HJ_OK;
}

int hj_host_set_reuse(int mode) {
    if (mode != HJ_REUSE_DIGEST && mode != HJ_REUSE_EXACT && mode != HJ_REUSE_OFF) HJ_FAIL(HJ_ERR_ARG, "bad reuse mode");
    const int prev = g_reuse.exchange(mode);
    if (prev == HJ_REUSE_EXACT && mode != HJ_REUSE_EXACT) {
        // the EXACT copies can no longer be used: give their memory back
        // (the default contexts' now -- g_default_mu held throughout, so
        // hj_ctx_destroy, which takes a context out of g_default before it
        // frees anything, cannot free one under us; user contexts drop
        // theirs at their next host join)
        std::lock_guard<std::mutex> lk(g_default_mu);
        for (auto &kv : g_default) {
            std::lock_guard<std::mutex> host_lk(kv.second->host_mu);
            kv.second->memo.invalidate();
        }
    }
    return prev;
}

int64_t hj_host_memo_hits(void) {
    hj_ctx *c = default_ctx();
    if (!c) return HJ_ERR_HIP;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    return c->memo_hits;
}
const char *hj_last_error(void) { return g_err.c_str(); }

hj_ctx *hj_ctx_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        fail(HJ_ERR_HIP, __FILE__, __LINE__, "no HIP device visible");
        return nullptr;
    }
    if (device < 0 || device >= n) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "device index out of range");
        return nullptr;
    }
    hj_ctx *c = new hj_ctx();
    c->device = device;
    if (set_device(c) != HJ_OK || ensure_meta(c, 64) != HJ_OK) {
        delete c;
        return nullptr;
    }
    return c;
}

void hj_ctx_destroy(hj_ctx *c) {
    if (!c) return;
    {   // out of the default registry first (hj_host_set_reuse walks it)
        std::lock_guard<std::mutex> lk(g_default_mu);
        for (auto it = g_default.begin(); it != g_default.end(); ++it)
            if (it->second == c) {
                g_default.erase(it);
                break;
            }
    }
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->table) (void)hipFree(c->table);
    if (c->side) (void)hipFree(c->side);
    if (c->marks) (void)hipFree(c->marks);
    if (c->meta) (void)hipFree(c->meta);
    if (c->dcount) (void)hipFree(c->dcount);
    for (int i = 0; i < hj_ctx::kDbufs; ++i)
        if (c->dbuf[i]) (void)hipFree(c->dbuf[i]);
    if (c->host_stream) (void)hipStreamDestroy(c->host_stream);
    for (SetBufs *sb : {&c->rset, &c->sset, &c->tset})
        for (Buf *b : {&sb->rows, &sb->bbin, &sb->bfill, &sb->runs, &sb->rstart}) free_buf(*b);
    for (Buf *b : {&c->nb, &c->pcur, &c->rcur, &c->tile_start, &c->tile_owner, &c->tdesc, &c->wstart, &c->work_start, &c->work_desc, &c->scan_sums, &c->scan_state, &c->raw_cnt,
                   &c->slow, &c->acc_cnt, &c->acc_sum, &c->acc_min, &c->acc_max, &c->exp_cnt, &c->exp_sums, &c->rows_kx, &c->rows_ky, &c->rows_px, &c->rows_py, &c->sel_tiles, &c->sel_sums,
                   &c->route_hist, &c->route_sums})
        free_buf(*b);
    for (int k = 0; k < c->ev_made; ++k)
        for (int i = 0; i < kEvCount; ++i) (void)hipEventDestroy(c->sets[k].ev[i]);
    delete c;
}

int hj_ctx_reserve(hj_ctx *c, int64_t max_build_rows, int key_bits) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (max_build_rows < 0 || (key_bits != 32 && key_bits != 64)) HJ_FAIL(HJ_ERR_ARG, "bad reserve arguments");
    HJ_TRY(set_device(c));
    HJ_TRY(ensure_meta(c, 64));
    if (choose_strategy(c, max_build_rows) == HJ_STRATEGY_GLOBAL) {
        HJ_TRY(ensure_table(c, max_build_rows, key_bits == 64 ? kWide : kNarrow));
        if (c->strategy != HJ_STRATEGY_AUTO || max_build_rows < kDualMinBuildRows) return HJ_OK;
    }
    const hj::RadixPlan pl = hj::radix_plan(max_build_rows, c->radix_bits, key_bits == 64);
    return ensure_radix_scratch(c, c->rset, max_build_rows, key_bits == 64, pl);
}

int64_t hj_ctx_table_capacity(const hj_ctx *c) {
    if (!c || (c->layout < 0 && !c->agg_ran)) return 0;
    if (c->used == HJ_STRATEGY_RADIX) return (int64_t)(1ll << c->plan.total_bits);   // partitions
    return (int64_t)(1ll << c->bits);
}

int hj_ctx_radix_plan(const hj_ctx *c, int *passes, int bits[3]) {
    if (!c || !passes || !bits) HJ_FAIL(HJ_ERR_ARG, "null argument");
    const bool radix = (c->layout >= 0 || c->agg_ran) && (c->used == HJ_STRATEGY_RADIX || c->dual);
    *passes = radix ? c->plan.passes : 0;
    for (int i = 0; i < 3; ++i) bits[i] = radix ? c->plan.bits[i] : 0;
    return HJ_OK;
}

int hj_ctx_build_has_duplicates(hj_ctx *c) {
    if (!c || c->layout < 0) HJ_FAIL(HJ_ERR_STATE, "no table built");
    HJ_TRY(set_device(c));
    unsigned long long v = 0;
    HJ_HIP(hipDeviceSynchronize());
    HJ_HIP(hipMemcpy(&v, c->meta + 1, 8, hipMemcpyDeviceToHost));
    if (!v && c->used == HJ_STRATEGY_RADIX && !c->dup_checked) {
        // the joins flag only the repeats of partitions they built (k_join_b:
        // only those a probe row met): the exact answer, once per build, is a
        // DETECT build over every partition of R (the work map is rebuilt from
        // R alone; the last join's map is not needed again)
        hipStream_t st = nullptr;   // the default stream
        HJ_RADIX(c, st, hj::radix_detect(c->layout == kWide, c->plan, radix_work(c), bucket_set(c->rset),
                                         /*dup_flag*/ c->meta + 1, /*sample*/ c->meta + 2, st));
        HJ_HIP(hipDeviceSynchronize());
        HJ_HIP(hipMemcpy(&v, c->meta + 1, 8, hipMemcpyDeviceToHost));
        c->dup_checked = true;
    }
    return v ? 1 : 0;
}

int hj_ctx_join_kernel(hj_ctx *c) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (c->agg_ran) return c->used == HJ_STRATEGY_RADIX ? HJ_JOIN_KERNEL_AGGREGATE : 0;
    if (c->exists_ran && c->layout >= 0) return HJ_JOIN_KERNEL_EXISTS;
    if (c->lookup_ran && c->layout >= 0) return HJ_JOIN_KERNEL_LOOKUP;
    if (c->asof_ran && c->layout >= 0) return HJ_JOIN_KERNEL_ASOF;
    if (c->group_ran && c->layout >= 0) return HJ_JOIN_KERNEL_GROUP;
    if (c->expand_ran && c->layout >= 0) return HJ_JOIN_KERNEL_EXPAND;
    if (!c->join_ran || c->layout < 0) return 0;
    HJ_TRY(set_device(c));
    unsigned long long v[2] = {0, 0};
    HJ_HIP(hipDeviceSynchronize());
    HJ_HIP(hipMemcpy(v, c->meta + 2, sizeof(v), hipMemcpyDeviceToHost));
    return hj::join_kernel_choice(c->join_wide, c->join_stream, v[0], v[1]);
}

int hj_ctx_set_timing(hj_ctx *c, int enable) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    HJ_TRY(set_device(c));
    if (enable && !c->ev_ready) {
        for (int i = 0; i < kEvCount; ++i) HJ_HIP(hipEventCreate(&c->sets[0].ev[i]));
        c->ev_ready = true;
        c->ev_made = 1;
    }
    c->timing = enable != 0;
    return HJ_OK;
}

int hj_ctx_timing_accumulate(hj_ctx *c, int enable) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (enable) HJ_TRY(hj_ctx_set_timing(c, 1));
    if (enable && c->ev_made < hj_ctx::kEvSets) {
        for (int k = c->ev_made; k < hj_ctx::kEvSets; ++k) {
            for (int i = 0; i < kEvCount; ++i) HJ_HIP(hipEventCreate(&c->sets[k].ev[i]));
            c->ev_made = k + 1;
        }
    }
    if (enable) c->acc = true;
    if (!c->acc) return HJ_OK;
    // a fresh start: nothing recorded so far counts
    for (auto &s : c->sets) s.rec[0] = s.rec[1] = s.rec[2] = s.rec[3] = s.rec_mid = false;
    for (double &t : c->tot) t = 0.0;
    c->tot_sets = 0;
    if (!enable) {
        // (the sets stay created; set `cur` keeps taking the records)
        c->acc = false;
    }
    return HJ_OK;
}

int hj_ctx_timing_totals(hj_ctx *c, float ms[8], long long *sets) {
    if (!c || !ms || !sets) HJ_FAIL(HJ_ERR_ARG, "null argument");
    if (!c->acc) HJ_FAIL(HJ_ERR_STATE, "timing totals need hj_ctx_timing_accumulate(c, 1)");
    HJ_TRY(set_device(c));
    for (int k = 1; k <= hj_ctx::kEvSets; ++k) HJ_TRY(fold_set(c, (c->cur + k) % hj_ctx::kEvSets));
    for (int i = 0; i < 8; ++i) ms[i] = i < 6 ? (float)c->tot[i] : -1.0f;
    *sets = c->tot_sets;
    for (double &t : c->tot) t = 0.0;
    c->tot_sets = 0;
    return HJ_OK;
}

int hj_ctx_last_timing_ex(hj_ctx *c, float ms[8]) {
    if (!c || !ms) HJ_FAIL(HJ_ERR_ARG, "null argument");
    for (int i = 0; i < 8; ++i) ms[i] = -1.0f;
    if (!c->ev_ready) return HJ_OK;
    HJ_TRY(set_device(c));
    return set_ms(c->evs(), ms);
}

int hj_ctx_last_timing(hj_ctx *c, float ms[4]) {
    float ex[8];
    HJ_TRY(hj_ctx_last_timing_ex(c, ex));
    for (int i = 0; i < 4; ++i) ms[i] = ex[i];
    return HJ_OK;
}

int hj_ctx_set_strategy(hj_ctx *c, int strategy) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (strategy != HJ_STRATEGY_AUTO && strategy != HJ_STRATEGY_GLOBAL && strategy != HJ_STRATEGY_RADIX)
        HJ_FAIL(HJ_ERR_ARG, "unknown strategy");
    c->strategy = strategy;
    return HJ_OK;
}

int hj_ctx_set_radix_bits(hj_ctx *c, int bits) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (bits < 0 || bits > 24) HJ_FAIL(HJ_ERR_ARG, "radix bits must be in [0, 24]");
    c->radix_bits = bits;
    return HJ_OK;
}


int hj_ctx_strategy_used(const hj_ctx *c) {
    if (c && c->agg_ran) return c->used;
    if (!c || c->layout < 0) return 0;
    return c->probe_used >= 0 ? c->probe_used : c->used;
}

int hj_ctx_probe_hint(hj_ctx *c, int64_t probe_rows) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    c->probe_hint = probe_rows < 0 ? -1 : probe_rows;
    return HJ_OK;
}

int hj_ctx_reserve_probe(hj_ctx *c, int64_t max_probe_rows, int key_bits) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (max_probe_rows < 0 || (key_bits != 32 && key_bits != 64)) HJ_FAIL(HJ_ERR_ARG, "bad reserve arguments");
    if (c->layout < 0 || (c->used != HJ_STRATEGY_RADIX && !c->dual)) return HJ_OK;   // the global table needs none
    HJ_TRY(set_device(c));
    return ensure_radix_scratch(c, c->sset, max_probe_rows, key_bits == 64, c->plan);
}

int hj_ctx_reserve_group(hj_ctx *c, int64_t max_build_rows, int key_bits) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (max_build_rows < 0 || (key_bits != 32 && key_bits != 64)) HJ_FAIL(HJ_ERR_ARG, "bad reserve arguments");
    // (the radix group probe works in the build's and hj_ctx_reserve_probe's workspace)
    if (choose_strategy(c, max_build_rows) != HJ_STRATEGY_GLOBAL) return HJ_OK;
    HJ_TRY(set_device(c));
    return ensure_group_acc(c, table_bits(max_build_rows), key_bits == 64 ? kWide : kNarrow, true, true, true);
}

int hj_ctx_reserve_expand(hj_ctx *c, int64_t max_probe_rows, int key_bits) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (max_probe_rows < 0 || (key_bits != 32 && key_bits != 64)) HJ_FAIL(HJ_ERR_ARG, "bad reserve arguments");
    // (the counts are int32 and the tile sums u64 whatever the key width; both strategies use them)
    HJ_TRY(set_device(c));
    return ensure_expand(c, max_probe_rows);
}

int hj_ctx_reserve_aggregate(hj_ctx *c, int64_t max_rows, int key_bits) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (max_rows < 0 || (key_bits != 32 && key_bits != 64)) HJ_FAIL(HJ_ERR_ARG, "bad reserve arguments");
    if (key_bits == 32 && max_rows > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "i32 row ids: at most 2^31 - 1 rows");
    HJ_TRY(set_device(c));
    HJ_TRY(ensure_meta(c, 64));
    const int layout = key_bits == 64 ? kWide : kNarrow;
    const int used = aggregate_strategy(c, max_rows);
    // (a current build that lives in the global table is dropped when the table is replaced or lost)
    const size_t table_bytes = c->table_bytes;
    int rc = ensure_aggregate(c, max_rows, layout, used, true, true, true);
    // AUTO sends the inputs below kRadixMinRows rows to the global table: size that too
    if (rc == HJ_OK && c->strategy == HJ_STRATEGY_AUTO && used == HJ_STRATEGY_RADIX)
        rc = ensure_aggregate(c, kRadixMinRows - 1, layout, HJ_STRATEGY_GLOBAL, true, true, true);
    if (c->table_bytes != table_bytes && (c->used == HJ_STRATEGY_GLOBAL || c->dual)) c->layout = -1;
    return rc;
}

// ------------------------------------------------------------ device phases
int hj_dev_build_i64(hj_ctx *c, const int64_t *rkey, const int64_t *rpay, int64_t n, void *stream) {
    return do_build(c, kWide, src_cols64(rkey, rpay, n), (hipStream_t)stream);
}
int hj_dev_count_i64(hj_ctx *c, const int64_t *skey, int64_t n, uint64_t *d_count, void *stream) {
    hj::SrcDev s = src_cols64(skey, skey, n);   // payload unused when counting
    return do_probe(c, kWide, s, nullptr, nullptr, 0, d_count, true, (hipStream_t)stream);
}
int hj_dev_probe_i64(hj_ctx *c, const int64_t *skey, const int64_t *spay, int64_t n, int64_t *out_r,
                     int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream) {
    if (n > 0 && !spay) HJ_FAIL(HJ_ERR_ARG, "null probe payload");
    return do_probe(c, kWide, src_cols64(skey, spay, n), out_r, out_s, out_cap, d_count, false,
                    (hipStream_t)stream);
}
int hj_dev_build_tuples_i64(hj_ctx *c, const int64_t *tuples, int64_t n, void *stream) {
    return do_build(c, kWide, src_packed(tuples, n), (hipStream_t)stream);
}
int hj_dev_probe_tuples_i64(hj_ctx *c, const int64_t *tuples, int64_t n, int64_t *out_r, int64_t *out_s,
                            int64_t out_cap, uint64_t *d_count, void *stream) {
    return do_probe(c, kWide, src_packed(tuples, n), out_r, out_s, out_cap, d_count, false, (hipStream_t)stream);
}
int hj_dev_build_i32(hj_ctx *c, const int32_t *rkey, int64_t n, int64_t row_base, void *stream) {
    if (row_base < 0 || row_base + n > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "i32 row ids out of range");
    return do_build(c, kNarrow, src_col32(rkey, n, row_base), (hipStream_t)stream);
}
int hj_dev_count_i32(hj_ctx *c, const int32_t *skey, int64_t n, uint64_t *d_count, void *stream) {
    return do_probe(c, kNarrow, src_col32(skey, n, 0), nullptr, nullptr, 0, d_count, true, (hipStream_t)stream);
}
int hj_dev_probe_i32(hj_ctx *c, const int32_t *skey, int64_t n, int64_t row_base, int32_t *out_r, int32_t *out_s,
                     int64_t out_cap, uint64_t *d_count, void *stream) {
    if (row_base < 0 || row_base + n > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "i32 row ids out of range");
    return do_probe(c, kNarrow, src_col32(skey, n, row_base), out_r, out_s, out_cap, d_count, false,
                    (hipStream_t)stream);
}

int hj_dev_exists_i64(hj_ctx *c, int kind, const int64_t *skey, const int64_t *spay, int64_t n, int64_t *out_key,
                      int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream) {
    // (the count-only form reads no payload: any readable column stands in)
    if (n > 0 && !spay && (out_cap != 0 || out_s)) HJ_FAIL(HJ_ERR_ARG, "null probe payload");
    return do_exists(c, kWide, kind, src_cols64(skey, spay ? spay : skey, n), out_key, out_s, out_cap, d_count,
                     (hipStream_t)stream);
}
int hj_dev_exists_tuples_i64(hj_ctx *c, int kind, const int64_t *tuples, int64_t n, int64_t *out_key, int64_t *out_s,
                             int64_t out_cap, uint64_t *d_count, void *stream) {
    return do_exists(c, kWide, kind, src_packed(tuples, n), out_key, out_s, out_cap, d_count, (hipStream_t)stream);
}
int hj_dev_exists_i32(hj_ctx *c, int kind, const int32_t *skey, int64_t n, int64_t row_base, int32_t *out_key,
                      int32_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream) {
    if (row_base < 0 || row_base + n > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "i32 row ids out of range");
    return do_exists(c, kNarrow, kind, src_col32(skey, n, row_base), out_key, out_s, out_cap, d_count,
                     (hipStream_t)stream);
}

int hj_dev_lookup_i64(hj_ctx *c, const int64_t *skey, int64_t n, int64_t null_pay, int64_t *out_r, int32_t *out_cnt,
                      uint64_t *d_count, void *stream) {
    // (the key column stands in for the payload column, which no lookup kernel reads)
    return do_lookup(c, kWide, src_cols64(skey, skey, n), (unsigned long long)null_pay, out_r, out_cnt, d_count,
                     (hipStream_t)stream);
}
int hj_dev_lookup_i32(hj_ctx *c, const int32_t *skey, int64_t n, int32_t null_row, int32_t *out_r, int32_t *out_cnt,
                      uint64_t *d_count, void *stream) {
    return do_lookup(c, kNarrow, src_col32(skey, n, 0), (unsigned long long)(long long)null_row, out_r, out_cnt,
                     d_count, (hipStream_t)stream);
}

int hj_dev_asof_i64(hj_ctx *c, int kind, const int64_t *skey, const int64_t *sbound, int64_t n, int64_t null_pay,
                    int64_t *out_r, uint64_t *d_count, void *stream) {
    // (the key column stands in for the payload column, which no as-of kernel reads)
    return do_asof(c, kWide, kind, src_cols64(skey, skey, n), sbound, (unsigned long long)null_pay, out_r, d_count,
                   (hipStream_t)stream);
}
int hj_dev_asof_i32(hj_ctx *c, int kind, const int32_t *skey, const int32_t *sbound, int64_t n, int32_t null_row,
                    int32_t *out_r, uint64_t *d_count, void *stream) {
    return do_asof(c, kNarrow, kind, src_col32(skey, n, 0), sbound, (unsigned long long)(long long)null_row, out_r,
                   d_count, (hipStream_t)stream);
}

int hj_dev_expand_i64(hj_ctx *c, int kind, const int64_t *skey, int64_t n, int64_t null_pay, int64_t *out_off,
                      int64_t *out_r, int64_t out_cap, uint64_t *d_count, void *stream) {
    // (the key column stands in for the payload column, which no expand kernel reads)
    return do_expand(c, kWide, kind, src_cols64(skey, skey, n), (unsigned long long)null_pay, out_off, out_r, out_cap,
                     d_count, (hipStream_t)stream);
}
int hj_dev_expand_i32(hj_ctx *c, int kind, const int32_t *skey, int64_t n, int32_t null_row, int64_t *out_off,
                      int32_t *out_r, int64_t out_cap, uint64_t *d_count, void *stream) {
    return do_expand(c, kNarrow, kind, src_col32(skey, n, 0), (unsigned long long)(long long)null_row, out_off, out_r,
                     out_cap, d_count, (hipStream_t)stream);
}

int hj_dev_group_i64(hj_ctx *c, int kind, const int64_t *skey, const int64_t *sval, int64_t n, int64_t null_val,
                     int64_t *out_r, int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                     int64_t out_cap, uint64_t *d_count, void *stream) {
    // (a null value column is kept null: no kernel reads it when no aggregate of it is asked for)
    const bool no_val = n > 0 && !sval && (out_sum || out_min || out_max);
    return do_group(c, kWide, kind, src_cols64(skey, sval, n), no_val ? "null probe value column" : nullptr,
                    (unsigned long long)null_val, out_r, out_cnt, out_sum, out_min, out_max, out_cap, d_count,
                    (hipStream_t)stream);
}
int hj_dev_group_tuples_i64(hj_ctx *c, int kind, const int64_t *tuples, int64_t n, int64_t null_val, int64_t *out_r,
                            int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max, int64_t out_cap,
                            uint64_t *d_count, void *stream) {
    return do_group(c, kWide, kind, src_packed(tuples, n), nullptr, (unsigned long long)null_val, out_r, out_cnt,
                    out_sum, out_min, out_max, out_cap, d_count, (hipStream_t)stream);
}
int hj_dev_group_i32(hj_ctx *c, int kind, const int32_t *skey, int64_t n, int64_t row_base, int32_t null_row,
                     int32_t *out_r, int32_t *out_cnt, int64_t *out_sum, int32_t *out_min, int32_t *out_max,
                     int64_t out_cap, uint64_t *d_count, void *stream) {
    const bool bad_ids = n > 0x7fffffffll || row_base < 0 || row_base + n > 0x7fffffffll;
    return do_group(c, kNarrow, kind, src_col32(skey, n, bad_ids ? 0 : row_base),
                    bad_ids ? "i32 row ids out of range" : nullptr, (unsigned long long)(uint32_t)null_row, out_r,
                    out_cnt, out_sum, out_min, out_max, out_cap, d_count, (hipStream_t)stream);
}

int hj_dev_aggregate_i64(hj_ctx *c, const int64_t *key, const int64_t *val, int64_t n, int64_t *out_key,
                         int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max, int64_t out_cap,
                         uint64_t *d_count, void *stream) {
    // (a null value column is kept null: no kernel reads it when no aggregate of it is asked for)
    // (n == 0 reads nothing: an empty column may be null)
    const bool no_val = n > 0 && !val && (out_sum || out_min || out_max);
    return do_aggregate(c, kWide, src_cols64(key, val, n), no_val ? "null value column" : nullptr, out_key, out_cnt,
                        out_sum, out_min, out_max, out_cap, d_count, (hipStream_t)stream);
}
int hj_dev_aggregate_tuples_i64(hj_ctx *c, const int64_t *tuples, int64_t n, int64_t *out_key, int64_t *out_cnt,
                                int64_t *out_sum, int64_t *out_min, int64_t *out_max, int64_t out_cap,
                                uint64_t *d_count, void *stream) {
    return do_aggregate(c, kWide, src_packed(tuples, n), nullptr, out_key, out_cnt, out_sum, out_min, out_max, out_cap,
                        d_count, (hipStream_t)stream);
}
int hj_dev_aggregate_i32(hj_ctx *c, const int32_t *key, int64_t n, int64_t row_base, int32_t *out_key,
                         int32_t *out_cnt, int64_t *out_sum, int32_t *out_min, int32_t *out_max, int64_t out_cap,
                         uint64_t *d_count, void *stream) {
    const bool bad_ids = n > 0x7fffffffll || row_base < 0 || row_base + n > 0x7fffffffll;
    return do_aggregate(c, kNarrow, src_col32(key, n, bad_ids ? 0 : row_base),
                        bad_ids ? "i32 row ids out of range" : nullptr, out_key, out_cnt, out_sum, out_min, out_max,
                        out_cap, d_count, (hipStream_t)stream);
}

// (the null context is reported before any other argument, as the header says)
int hj_dev_probe_outer_i64(hj_ctx *c, const int64_t *skey, const int64_t *spay, int64_t n, int64_t null_pay,
                           int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    // (the count-only form reads no payload: any readable column stands in)
    if (n > 0 && !spay && (out_cap != 0 || out_r || out_s)) HJ_FAIL(HJ_ERR_ARG, "null probe payload");
    return do_probe_outer(c, kWide, src_cols64(skey, spay ? spay : skey, n), (unsigned long long)null_pay, out_r, out_s,
                          out_cap, d_count, (hipStream_t)stream);
}
int hj_dev_probe_outer_tuples_i64(hj_ctx *c, const int64_t *tuples, int64_t n, int64_t null_pay, int64_t *out_r,
                                  int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream) {
    return do_probe_outer(c, kWide, src_packed(tuples, n), (unsigned long long)null_pay, out_r, out_s, out_cap, d_count,
                          (hipStream_t)stream);
}
int hj_dev_probe_outer_i32(hj_ctx *c, const int32_t *skey, int64_t n, int64_t row_base, int32_t null_row,
                           int32_t *out_r, int32_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (row_base < 0 || row_base + n > 0x7fffffffll) HJ_FAIL(HJ_ERR_ARG, "i32 row ids out of range");
    return do_probe_outer(c, kNarrow, src_col32(skey, n, row_base), (unsigned long long)(uint32_t)null_row, out_r,
                          out_s, out_cap, d_count, (hipStream_t)stream);
}

int hj_dev_probe_full_i64(hj_ctx *c, int kind, const int64_t *skey, const int64_t *spay, int64_t n, int64_t null_r,
                          int64_t null_s, int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count,
                          void *stream) {
    // (the count-only form reads no payload: any readable column stands in)
    const bool no_pay = n > 0 && !spay && (out_cap != 0 || out_r || out_s);
    return do_probe_full(c, kWide, kind, src_cols64(skey, spay ? spay : skey, n), no_pay ? "null probe payload" : nullptr,
                         (unsigned long long)null_r, (unsigned long long)null_s, out_r, out_s, out_cap, d_count,
                         (hipStream_t)stream);
}
int hj_dev_probe_full_tuples_i64(hj_ctx *c, int kind, const int64_t *tuples, int64_t n, int64_t null_r, int64_t null_s,
                                 int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream) {
    return do_probe_full(c, kWide, kind, src_packed(tuples, n), nullptr, (unsigned long long)null_r,
                         (unsigned long long)null_s, out_r, out_s, out_cap, d_count, (hipStream_t)stream);
}
int hj_dev_probe_full_i32(hj_ctx *c, int kind, const int32_t *skey, int64_t n, int64_t row_base, int32_t null_row_r,
                          int32_t null_row_s, int32_t *out_r, int32_t *out_s, int64_t out_cap, uint64_t *d_count,
                          void *stream) {
    const bool bad_ids = row_base < 0 || row_base + n > 0x7fffffffll;
    return do_probe_full(c, kNarrow, kind, src_col32(skey, n, bad_ids ? 0 : row_base),
                         bad_ids ? "i32 row ids out of range" : nullptr, (unsigned long long)(uint32_t)null_row_r,
                         (unsigned long long)(uint32_t)null_row_s, out_r, out_s, out_cap, d_count, (hipStream_t)stream);
}

int hj_dev_partition_i64(hj_ctx *c, const int64_t *key, const int64_t *pay, int64_t n, int nparts,
                         int64_t *out_tuples, uint64_t *d_counts, void *stream) {
    if (n > 0 && !pay) HJ_FAIL(HJ_ERR_ARG, "null payload");
    return do_partition(c, src_cols64(key, pay, n), nparts, out_tuples, d_counts, (hipStream_t)stream);
}
int hj_dev_partition_tuples_i64(hj_ctx *c, const int64_t *tuples, int64_t n, int nparts, int64_t *out_tuples,
                                uint64_t *d_counts, void *stream) {
    return do_partition(c, src_packed(tuples, n), nparts, out_tuples, d_counts, (hipStream_t)stream);
}

int hj_route_plan(int64_t n_build_global, int nranks, int *sub_bits) {
    if (!sub_bits) HJ_FAIL(HJ_ERR_ARG, "null argument");
    *sub_bits = 0;
    if (nranks < 1 || nranks > hj::kMaxRouteSources || (nranks & (nranks - 1)) || n_build_global < 0)
        return HJ_OK;
    const int g = ceil_log2((unsigned long long)nranks);
    const int64_t local = (n_build_global + nranks - 1) / nranks;
    if (local < kRadixMinRows || g >= 9) return HJ_OK;
    const int t = hj::radix_plan(local, 0, true).total_bits;
    const int b1 = 9 - g < t - 1 ? 9 - g : t - 1;
    if (b1 >= 1 && t - b1 <= 9) *sub_bits = b1;
    return HJ_OK;
}

int hj_dev_route_i64(hj_ctx *c, const int64_t *key, const int64_t *pay, int64_t n, int nranks, int sub_bits,
                     int64_t *out_tuples, uint64_t *d_counts, void *stream) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (n > 0 && (!key || !pay || !out_tuples)) HJ_FAIL(HJ_ERR_ARG, "bad route input");
    if (!d_counts) HJ_FAIL(HJ_ERR_ARG, "null counts");
    if (nranks < 1 || (nranks & (nranks - 1)) || sub_bits < 1) HJ_FAIL(HJ_ERR_ARG, "nranks: a power of two; sub_bits >= 1");
    const int rbits = ceil_log2((unsigned long long)nranks) + sub_bits;
    if (rbits > 9) HJ_FAIL(HJ_ERR_ARG, "nranks << sub_bits must be <= 512");
    hipStream_t st = (hipStream_t)stream;
    HJ_TRY(set_device(c));
    const size_t hw = hj::radix_route_scratch(n, rbits);
    HJ_TRY(ensure_buf(c->route_hist, hw * 8));
    HJ_TRY(ensure_buf(c->route_sums, hj::exclusive_scan_sums(hw) * 8));
    record(c, kEvPart0, st);
    HJ_HIP(hj::radix_route(src_cols64(key, pay, n), rbits, out_tuples, (unsigned long long *)d_counts,
                           (unsigned long long *)c->route_hist.p, (unsigned long long *)c->route_sums.p, st));
    record(c, kEvPart1, st);
    c->evs().rec[3] = c->timing;
    return HJ_OK;
}

int hj_dev_build_routed_i64(hj_ctx *c, const int64_t *tuples, int64_t n, const uint64_t *d_counts, int nsrc,
                            int nranks, int sub_bits, void *stream) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (n < 0 || (n > 0 && !tuples) || !d_counts) HJ_FAIL(HJ_ERR_ARG, "bad routed build relation");
    if (nsrc < 1 || nsrc > hj::kMaxRouteSources || nranks < 1 || (nranks & (nranks - 1)) || sub_bits < 1 ||
        sub_bits > 9)
        HJ_FAIL(HJ_ERR_ARG, "bad routed layout");
    // (what hj_dev_route_i64 can have produced: owner and bin bits from 9 hash bits)
    if (ceil_log2((unsigned long long)nranks) + sub_bits > 9) HJ_FAIL(HJ_ERR_ARG, "nranks << sub_bits must be <= 512");
    // this rank's plan: the routing's bins are its first pass (skip = the
    // owner bits above them), one local pass of <= 9 bits below them
    hj::RadixPlan pl = hj::radix_plan(n, 0, true);
    int t = pl.total_bits;
    if (t < sub_bits + 1) t = sub_bits + 1;
    if (t > sub_bits + 9) t = sub_bits + 9;
    pl.passes = 2;
    pl.bits[0] = sub_bits;
    pl.bits[1] = t - sub_bits;
    pl.bits[2] = 0;
    pl.pbl[0] = 10;   // (sizes the ping set, whose run arrays list the routed rows)
    pl.pbl[1] = hj::kFinalPbl;
    pl.pbl[2] = 0;
    pl.total_bits = t;
    pl.skip = ceil_log2((unsigned long long)nranks);
    HJ_TRY(begin_build(c, kWide, n, HJ_STRATEGY_RADIX, false, true, pl));
    return radix_build(c, RadixSrc{src_packed(tuples, n), d_counts, nsrc, 1 << sub_bits}, (hipStream_t)stream);
}

int hj_dev_probe_routed_i64(hj_ctx *c, const int64_t *tuples, int64_t n, const uint64_t *d_counts, int nsrc,
                            int bin0, int nbins, int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count,
                            void *stream) {
    if (!c) HJ_FAIL(HJ_ERR_ARG, "null context");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (c->layout != kWide || c->used != HJ_STRATEGY_RADIX || !c->routed)
        HJ_FAIL(HJ_ERR_STATE, "probe_routed needs a routed build");
    if (n < 0 || (n > 0 && !tuples) || !d_counts) HJ_FAIL(HJ_ERR_ARG, "bad routed probe relation");
    if (out_cap < 0 || (out_cap > 0 && (!out_r || !out_s))) HJ_FAIL(HJ_ERR_ARG, "bad output");
    const int F = 1 << c->plan.bits[0];
    if (nsrc < 1 || nsrc > hj::kMaxRouteSources || bin0 < 0 || nbins < 1 || bin0 + nbins > F)
        HJ_FAIL(HJ_ERR_ARG, "bad routed layout");
    ProbeReq q;
    q.in = RadixSrc{src_packed(tuples, n), d_counts, nsrc, nbins};
    q.bin0 = bin0;
    q.out = hj::OutDev{out_r, out_s, out_cap, (unsigned long long *)d_count};
    return run_probe(c, q, (hipStream_t)stream);
}

int hj_partition_of(int64_t key, int nparts) {
    if (nparts < 1) return -1;
    unsigned long long k = (unsigned long long)key;
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (int)(((k >> 32) * (unsigned long long)(unsigned)nparts) >> 32);
}

int hj_dev_gen_pkfk_i64(uint64_t seed, int64_t NR, uint64_t hit_threshold, int64_t r0, int64_t nr, int64_t *rkey,
                        int64_t *rpay, int64_t s0, int64_t ns, int64_t *skey, int64_t *spay, void *stream) {
    if (NR <= 0 || nr < 0 || ns < 0) HJ_FAIL(HJ_ERR_ARG, "bad generator sizes");
    HJ_HIP(hj::launch_gen_pkfk(seed, NR, hit_threshold, r0, nr, (long long *)rkey, (long long *)rpay, s0, ns,
                               (long long *)skey, (long long *)spay, (hipStream_t)stream));
    return HJ_OK;
}
int hj_zipf_params(int64_t NR, double theta, double out[4]) {
    if (NR < 1 || !(theta > 0.0 && theta < 1.0) || !out) HJ_FAIL(HJ_ERR_ARG, "zipf: NR >= 1 and 0 < theta < 1");
    // zeta(n, theta) = sum_{k=1..n} k^-theta: exact below 2^20 terms, then
    // Euler-Maclaurin for the tail (relative error < 1e-12 at n = 2^28)
    const int64_t m = NR < (1ll << 20) ? NR : (1ll << 20);
    double z = 0.0;
    for (int64_t k = m; k >= 1; --k) z += std::pow((double)k, -theta);
    if (NR > m) {
        const double a = (double)m, b = (double)NR, e = 1.0 - theta;
        z += (std::pow(b, e) - std::pow(a, e)) / e + 0.5 * (std::pow(b, -theta) - std::pow(a, -theta)) -
             theta / 12.0 * (std::pow(b, -theta - 1.0) - std::pow(a, -theta - 1.0));
    }
    double z2 = 1.0 + std::pow(2.0, -theta);
    out[0] = z;
    out[1] = (1.0 - std::pow(2.0 / (double)NR, 1.0 - theta)) / (1.0 - z2 / z);
    out[2] = 1.0 / (1.0 - theta);
    out[3] = std::pow(0.5, theta);
    return HJ_OK;
}

int hj_dev_gen_zipf_i64(uint64_t seed, int64_t NR, double theta, int64_t s0, int64_t ns, int64_t *skey,
                        int64_t *spay, void *stream) {
    double p[4];
    HJ_TRY(hj_zipf_params(NR, theta, p));
    if (ns < 0) HJ_FAIL(HJ_ERR_ARG, "bad generator sizes");
    hj::ZipfParams z;
    z.zetan = p[0];
    z.eta = p[1];
    z.alpha = p[2];
    z.half_pow_theta = p[3];
    z.n = (unsigned long long)NR;
    HJ_HIP(hj::launch_gen_zipf(seed, z, s0, ns, (long long *)skey, (long long *)spay, (hipStream_t)stream));
    return HJ_OK;
}

int hj_dev_gen_uniform_i64(uint64_t seed, uint64_t stream_id, int64_t lo, int64_t hi, int64_t i0, int64_t n,
                           int64_t *key, int64_t *pay, void *stream) {
    if (hi < lo || n < 0) HJ_FAIL(HJ_ERR_ARG, "bad generator range");
    HJ_HIP(hj::launch_gen_uniform_i64(seed, stream_id, lo, hi, i0, n, (long long *)key, (long long *)pay,
                                      (hipStream_t)stream));
    return HJ_OK;
}
int hj_dev_gen_uniform_i32(uint64_t seed, uint64_t stream_id, int32_t lo, int32_t hi, int64_t i0, int64_t n,
                           int32_t *key, void *stream) {
    if (hi < lo || n < 0) HJ_FAIL(HJ_ERR_ARG, "bad generator range");
    HJ_HIP(hj::launch_gen_uniform_i32(seed, stream_id, lo, hi, i0, n, key, (hipStream_t)stream));
    return HJ_OK;
}

// ------------------------------------------------------- host memref ABI
int64_t hj_count_i32(int32_t *, int32_t *r_align, int64_t r_off, int64_t r_size, int64_t r_stride, int32_t *,
                     int32_t *s_align, int64_t s_off, int64_t s_size, int64_t s_stride) {
    hj_ctx *c = default_ctx();
    if (!c) return HJ_ERR_HIP;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    int64_t m = 0;
    void *a, *b;
    int rc = host_join(c, kNarrow, rel32(r_align, r_off, r_size, r_stride), rel32(s_align, s_off, s_size, s_stride),
                       kHostCount, &m, &a, &b);
    return rc == HJ_OK ? m : rc;
}

int32_t hj_probe_i32(int32_t *, int32_t *r_align, int64_t r_off, int64_t r_size, int64_t r_stride, int32_t *,
                     int32_t *s_align, int64_t s_off, int64_t s_size, int64_t s_stride, int32_t *,
                     int32_t *or_align, int64_t or_off, int64_t or_size, int64_t or_stride, int32_t *,
                     int32_t *os_align, int64_t os_off, int64_t os_size, int64_t os_stride) {
    hj_ctx *c = default_ctx();
    if (!c) return HJ_ERR_HIP;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    int64_t m = 0;
    void *d_or = nullptr, *d_os = nullptr;
    const Deliver put = [&](const void *a, const void *b, int64_t mm) -> int {
        if (or_size != mm || os_size != mm) return 1;
        HJ_TRY(download<int32_t>(or_align, or_off, mm, or_stride, a, c->host_stream));
        return download<int32_t>(os_align, os_off, mm, os_stride, b, c->host_stream);
    };
    bool sent = false;
    HJ_TRY(host_join(c, kNarrow, rel32(r_align, r_off, r_size, r_stride), rel32(s_align, s_off, s_size, s_stride),
                     kHostProbe, &m, &d_or, &d_os, or_size == os_size ? &put : nullptr, &sent));
    if (sent) return HJ_OK;
    if (or_size != m || os_size != m) HJ_FAIL(HJ_ERR_CAPACITY, "output memrefs must have exactly M rows");
    HJ_TRY(download<int32_t>(or_align, or_off, m, or_stride, d_or, c->host_stream));
    HJ_TRY(download<int32_t>(os_align, os_off, m, os_stride, d_os, c->host_stream));
    return HJ_OK;
}

int64_t hj_count_i64(int64_t *, int64_t *rk, int64_t rk_off, int64_t rk_size, int64_t rk_stride, int64_t *,
                     int64_t *rp, int64_t rp_off, int64_t rp_size, int64_t rp_stride, int64_t *, int64_t *sk,
                     int64_t sk_off, int64_t sk_size, int64_t sk_stride, int64_t *, int64_t *sp, int64_t sp_off,
                     int64_t sp_size, int64_t sp_stride) {
    if (rk_size != rp_size || sk_size != sp_size) HJ_FAIL(HJ_ERR_ARG, "key/payload sizes differ");
    hj_ctx *c = default_ctx();
    if (!c) return HJ_ERR_HIP;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    int64_t m = 0;
    void *a, *b;
    int rc = host_join(c, kWide, rel64(rk, rk_off, rk_stride, rp, rp_off, rp_stride, rk_size),
                       rel64(sk, sk_off, sk_stride, sp, sp_off, sp_stride, sk_size), kHostCount, &m, &a, &b);
    return rc == HJ_OK ? m : rc;
}

int32_t hj_probe_i64(int64_t *, int64_t *rk, int64_t rk_off, int64_t rk_size, int64_t rk_stride, int64_t *,
                     int64_t *rp, int64_t rp_off, int64_t rp_size, int64_t rp_stride, int64_t *, int64_t *sk,
                     int64_t sk_off, int64_t sk_size, int64_t sk_stride, int64_t *, int64_t *sp, int64_t sp_off,
                     int64_t sp_size, int64_t sp_stride, int64_t *, int64_t *or_align, int64_t or_off,
                     int64_t or_size, int64_t or_stride, int64_t *, int64_t *os_align, int64_t os_off,
                     int64_t os_size, int64_t os_stride) {
    if (rk_size != rp_size || sk_size != sp_size) HJ_FAIL(HJ_ERR_ARG, "key/payload sizes differ");
    hj_ctx *c = default_ctx();
    if (!c) return HJ_ERR_HIP;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    int64_t m = 0;
    void *d_or = nullptr, *d_os = nullptr;
    const Deliver put = [&](const void *a, const void *b, int64_t mm) -> int {
        if (or_size != mm || os_size != mm) return 1;
        HJ_TRY(download<int64_t>(or_align, or_off, mm, or_stride, a, c->host_stream));
        return download<int64_t>(os_align, os_off, mm, os_stride, b, c->host_stream);
    };
    bool sent = false;
    HJ_TRY(host_join(c, kWide, rel64(rk, rk_off, rk_stride, rp, rp_off, rp_stride, rk_size),
                     rel64(sk, sk_off, sk_stride, sp, sp_off, sp_stride, sk_size), kHostProbe, &m, &d_or, &d_os,
                     or_size == os_size ? &put : nullptr, &sent));
    if (sent) return HJ_OK;
    if (or_size != m || os_size != m) HJ_FAIL(HJ_ERR_CAPACITY, "output memrefs must have exactly M rows");
    HJ_TRY(download<int64_t>(or_align, or_off, m, or_stride, d_or, c->host_stream));
    HJ_TRY(download<int64_t>(os_align, os_off, m, os_stride, d_os, c->host_stream));
    return HJ_OK;
}

// ------------------------------------------------------ MLIR C-interface
void _mlir_ciface_hj_join_i32(hj_memref2_i32 *res, hj_memref1_i32 *r, hj_memref1_i32 *s) {
    if (!res) return;
    std::memset(res, 0, sizeof(*res));
    if (!r || !s) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "null memref descriptor");
        return;
    }
    hj_ctx *c = default_ctx();
    if (!c) return;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    int64_t m = 0;
    void *d_or = nullptr, *d_os = nullptr;
    if (host_join(c, kNarrow, rel32(r->aligned, r->offset, r->sizes[0], r->strides[0]),
                  rel32(s->aligned, s->offset, s->sizes[0], s->strides[0]), kHostJoin, &m, &d_or, &d_os) != HJ_OK)
        return;
    fill_result<int32_t>(res, d_or, d_os, m, c->host_stream);
}

void _mlir_ciface_hj_join_i64(hj_memref2_i64 *res, hj_memref1_i64 *r, hj_memref1_i64 *s) {
    if (!res) return;
    std::memset(res, 0, sizeof(*res));
    if (!r || !s) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "null memref descriptor");
        return;
    }
    hj_ctx *c = default_ctx();
    if (!c) return;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    int64_t m = 0;
    void *d_or = nullptr, *d_os = nullptr;
    if (host_join(c, kWide, rel64(r->aligned, r->offset, r->strides[0], nullptr, 0, 1, r->sizes[0]),
                  rel64(s->aligned, s->offset, s->strides[0], nullptr, 0, 1, s->sizes[0]), kHostJoin, &m, &d_or,
                  &d_os) != HJ_OK)
        return;
    fill_result<int64_t>(res, d_or, d_os, m, c->host_stream);
}

void _mlir_ciface_hj_join_kp_i64(hj_memref2_i64 *res, hj_memref1_i64 *rk, hj_memref1_i64 *rp, hj_memref1_i64 *sk,
                                 hj_memref1_i64 *sp) {
    if (!res) return;
    std::memset(res, 0, sizeof(*res));
    if (!rk || !rp || !sk || !sp || rk->sizes[0] != rp->sizes[0] || sk->sizes[0] != sp->sizes[0]) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "bad key/payload memrefs");
        return;
    }
    hj_ctx *c = default_ctx();
    if (!c) return;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    int64_t m = 0;
    void *d_or = nullptr, *d_os = nullptr;
    if (host_join(c, kWide, rel64(rk->aligned, rk->offset, rk->strides[0], rp->aligned, rp->offset, rp->strides[0],
                                  rk->sizes[0]),
                  rel64(sk->aligned, sk->offset, sk->strides[0], sp->aligned, sp->offset, sp->strides[0], sk->sizes[0]),
                  kHostJoin, &m, &d_or, &d_os) != HJ_OK)
        return;
    fill_result<int64_t>(res, d_or, d_os, m, c->host_stream);
}

// ------------------------------------------------- nested-loop.mlir rows
int hj_dev_count_rows_i32(hj_ctx *c, const int32_t *t1, int64_t r1, int64_t c1, int64_t ld1, const int32_t *t2,
                          int64_t r2, int64_t c2, int64_t ld2, uint64_t *d_count, void *stream) {
    HJ_HIP(hipMemsetAsync(d_count, 0, sizeof(uint64_t), (hipStream_t)stream));
    return do_join_rows(c, RowTables{t1, r1, c1, ld1, t2, r2, c2, ld2}, nullptr, 0, 0, d_count, true,
                        (hipStream_t)stream);
}

int hj_dev_join_rows_i32(hj_ctx *c, const int32_t *t1, int64_t r1, int64_t c1, int64_t ld1, const int32_t *t2,
                         int64_t r2, int64_t c2, int64_t ld2, int32_t *out, int64_t ldo, int64_t out_cap,
                         uint64_t *d_count, void *stream) {
    return do_join_rows(c, RowTables{t1, r1, c1, ld1, t2, r2, c2, ld2}, out, ldo, out_cap, d_count, false,
                        (hipStream_t)stream);
}

int64_t hj_count_rows_i32(int32_t *, int32_t *a1, int64_t o1, int64_t r1, int64_t c1, int64_t s10, int64_t s11,
                          int32_t *, int32_t *a2, int64_t o2, int64_t r2, int64_t c2, int64_t s20, int64_t s21) {
    hj_ctx *c = default_ctx();
    if (!c) return HJ_ERR_HIP;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    int64_t m = 0, oc = 0;
    void *d = nullptr;
    const int rc = host_join_rows(c, a1, o1, r1, c1, s10, s11, a2, o2, r2, c2, s20, s21, true, &m, &oc, &d);
    return rc == HJ_OK ? m : rc;
}

int64_t hj_join_rows_i32(int32_t *, int32_t *a1, int64_t o1, int64_t r1, int64_t c1, int64_t s10, int64_t s11,
                         int32_t *, int32_t *a2, int64_t o2, int64_t r2, int64_t c2, int64_t s20, int64_t s21,
                         int32_t *, int32_t *ao, int64_t oo, int64_t ro, int64_t co, int64_t so0, int64_t so1) {
    hj_ctx *c = default_ctx();
    if (!c) return HJ_ERR_HIP;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    int64_t m = 0, oc = 0;
    void *d = nullptr;
    HJ_TRY(host_join_rows(c, a1, o1, r1, c1, s10, s11, a2, o2, r2, c2, s20, s21, false, &m, &oc, &d));
    if (co != oc) HJ_FAIL(HJ_ERR_ARG, "result memref must have c1 + c2 - 1 columns");
    if (ro < m) HJ_FAIL(HJ_ERR_CAPACITY, "result memref has fewer rows than the join");
    if (m > 0) {
        if (!ao) HJ_FAIL(HJ_ERR_ARG, "null result memref");
        std::vector<int32_t> tmp((size_t)(m * oc));
        HJ_HIP(hipMemcpyAsync(tmp.data(), d, sizeof(int32_t) * tmp.size(), hipMemcpyDeviceToHost, c->host_stream));
        HJ_HIP(hipStreamSynchronize(c->host_stream));
        int32_t *base = ao + oo;
        for (int64_t i = 0; i < m; ++i)
            for (int64_t j = 0; j < oc; ++j) base[i * so0 + j * so1] = tmp[(size_t)(i * oc + j)];
    }
    return m;
}

void _mlir_ciface_hj_join_rows_i32(hj_memref2_i32 *res, hj_memref2_i32 *t1, hj_memref2_i32 *t2) {
    if (!res) return;
    std::memset(res, 0, sizeof(*res));
    if (!t1 || !t2) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "null memref descriptor");
        return;
    }
    hj_ctx *c = default_ctx();
    if (!c) return;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    int64_t m = 0, oc = 0;
    void *d = nullptr;
    if (host_join_rows(c, t1->aligned, t1->offset, t1->sizes[0], t1->sizes[1], t1->strides[0], t1->strides[1],
                       t2->aligned, t2->offset, t2->sizes[0], t2->sizes[1], t2->strides[0], t2->strides[1], false,
                       &m, &oc, &d) != HJ_OK)
        return;
    int32_t *h = (int32_t *)std::malloc(sizeof(int32_t) * (size_t)(m > 0 ? m * oc : 1));
    if (!h) {
        fail(HJ_ERR_NOMEM, __FILE__, __LINE__, "malloc result");
        return;
    }
    if (m > 0) {
        if (hipMemcpyAsync(h, d, sizeof(int32_t) * (size_t)(m * oc), hipMemcpyDeviceToHost, c->host_stream) !=
                hipSuccess ||
            hipStreamSynchronize(c->host_stream) != hipSuccess) {
            std::free(h);
            fail(HJ_ERR_HIP, __FILE__, __LINE__, "copy result");
            return;
        }
    }
    res->allocated = res->aligned = h;
    res->offset = 0;
    res->sizes[0] = m;
    res->sizes[1] = oc;
    res->strides[0] = oc;
    res->strides[1] = 1;
}

// ------------------------------------------------------------- selection
int hj_dev_select_f32(hj_ctx *c, const float *in, int64_t n, int cmp, float value, float *out, int64_t *out_row,
                      int64_t out_cap, uint64_t *d_count, void *stream) {
    return do_select<float>(c, in, n, cmp, value, out, out_row, out_cap, d_count, (hipStream_t)stream);
}

int hj_dev_select_i64(hj_ctx *c, const int64_t *in, int64_t n, int cmp, int64_t value, int64_t *out,
                      int64_t *out_row, int64_t out_cap, uint64_t *d_count, void *stream) {
    return do_select<int64_t>(c, in, n, cmp, value, out, out_row, out_cap, d_count, (hipStream_t)stream);
}

int hj_dev_stream_copy(const void *in, void *out, int64_t rows, int shape, void *stream) {
    if (shape != HJ_COPY_PERSISTENT && shape != HJ_COPY_FLAT) HJ_FAIL(HJ_ERR_ARG, "bad copy shape");
    if (rows < 0) HJ_FAIL(HJ_ERR_ARG, "negative row count");
    if (rows > 0 && (!in || !out || (((uintptr_t)in | (uintptr_t)out) & 15)))
        HJ_FAIL(HJ_ERR_ARG, "copy buffers must be non-null and 16-B aligned");
    const int cus = hj::cu_count();
    HJ_HIP(hj::launch_stream_copy(in, out, rows, shape, cus, (hipStream_t)stream));
    return HJ_OK;
}

int64_t hj_select_f32(float *, float *in, int64_t in_off, int64_t in_size, int64_t in_stride, float value, float *,
                      float *out, int64_t out_off, int64_t out_size, int64_t out_stride) {
    hj_ctx *c = default_ctx();
    if (!c) return HJ_ERR_HIP;
    std::lock_guard<std::mutex> host_lk(c->host_mu);
    if (in_size < 0 || out_size < 0) HJ_FAIL(HJ_ERR_ARG, "negative memref size");
    HJ_TRY(set_device(c));
    HJ_TRY(host_stream(c));
    hipStream_t st = c->host_stream;
    void *din, *dout;
    HJ_TRY(dbuf(c, 0, sizeof(float) * (size_t)in_size, &din));
    HJ_TRY(dbuf(c, 1, sizeof(float) * (size_t)(in_size > 0 ? in_size : 1), &dout));
    HJ_TRY(upload<float>(din, in, in_off, in_size, in_stride, st));
    HJ_TRY(do_select<float>(c, (const float *)din, in_size, HJ_CMP_LT, value, (float *)dout, nullptr, in_size,
                            (uint64_t *)c->dcount, st));
    uint64_t m = 0;
    HJ_HIP(hipMemcpyAsync(&m, c->dcount, 8, hipMemcpyDeviceToHost, st));
    HJ_HIP(hipStreamSynchronize(st));
    if ((int64_t)m > out_size) HJ_FAIL(HJ_ERR_CAPACITY, "result memref smaller than the selection");
    HJ_TRY(download<float>(out, out_off, (int64_t)m, out_stride, dout, st));
    return (int64_t)m;
}

void hj_free_result(void *allocated) { std::free(allocated); }

}  // extern "C"

// --------------------------------------------------------- composite keys
// A key codec: the column set and, on the device, the plan block every
// hj_keys.hip kernel reads.  The host keeps only the call order (sealed or
// not); what was observed lives on the device alone.
struct hj_keycodec {
    int device = 0;
    int ncols = 0;
    unsigned w64 = 0;            // bit c: column c is int64
    hj::KeyPlan *plan = nullptr; // device
    bool sealed = false;
};

namespace {

int keys_cols(const hj_keycodec *kc, const void *const cols[], int64_t n, hj::KeyCols *out) {
    if (n < 0) HJ_FAIL(HJ_ERR_ARG, "negative row count");
    for (int c = 0; c < hj::kKeysMaxCols; ++c) out->p[c] = nullptr;
    if (n == 0) return HJ_OK;
    if (!cols) HJ_FAIL(HJ_ERR_ARG, "bad column set: null column array");
    for (int c = 0; c < kc->ncols; ++c) {
        if (!cols[c]) HJ_FAIL(HJ_ERR_ARG, "bad column set: null column");
        out->p[c] = cols[c];
    }
    return HJ_OK;
}

}  // namespace

extern "C" {

hj_keycodec *hj_keycodec_create(int device, int ncols, const int col_bits[]) {
    // the arguments first, before anything touches a device
    if (ncols < 1 || ncols > HJ_KEYS_MAX_COLS) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "key codec: ncols must be 1.." + std::to_string(HJ_KEYS_MAX_COLS));
        return nullptr;
    }
    if (!col_bits) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "key codec: null col_bits");
        return nullptr;
    }
    unsigned w64 = 0;
    for (int c = 0; c < ncols; ++c) {
        if (col_bits[c] != 32 && col_bits[c] != 64) {
            fail(HJ_ERR_ARG, __FILE__, __LINE__, "key codec: col_bits must be 32 or 64");
            return nullptr;
        }
        w64 |= (col_bits[c] == 64 ? 1u : 0u) << c;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        fail(HJ_ERR_HIP, __FILE__, __LINE__, "no HIP device visible");
        return nullptr;
    }
    if (device < 0 || device >= n) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "device index out of range");
        return nullptr;
    }
    hj_keycodec *kc = new hj_keycodec();
    kc->device = device;
    kc->ncols = ncols;
    kc->w64 = w64;
    // the reset state, written by the reset kernel and waited for here: the
    // first call may come on any stream
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc((void **)&kc->plan, sizeof(hj::KeyPlan));
    if (e == hipSuccess) e = hj::keys_reset(kc->plan, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        fail(e == hipErrorOutOfMemory ? HJ_ERR_NOMEM : HJ_ERR_HIP, __FILE__, __LINE__,
             std::string("key codec: ") + hipGetErrorString(e));
        if (kc->plan) (void)hipFree(kc->plan);
        delete kc;
        return nullptr;
    }
    return kc;
}

void hj_keycodec_destroy(hj_keycodec *kc) {
    if (!kc) return;
    (void)hipSetDevice(kc->device);
    (void)hipDeviceSynchronize();
    if (kc->plan) (void)hipFree(kc->plan);
    delete kc;
}

int hj_dev_keycodec_reset(hj_keycodec *kc, void *stream) {
    if (!kc) HJ_FAIL(HJ_ERR_ARG, "null codec");
    HJ_HIP(hipSetDevice(kc->device));
    HJ_HIP(hj::keys_reset(kc->plan, (hipStream_t)stream));
    kc->sealed = false;
    return HJ_OK;
}

int hj_dev_keycodec_observe(hj_keycodec *kc, const void *const cols[], int64_t n, void *stream) {
    if (!kc) HJ_FAIL(HJ_ERR_ARG, "null codec");
    hj::KeyCols kcols;
    HJ_TRY(keys_cols(kc, cols, n, &kcols));
    if (kc->sealed) HJ_FAIL(HJ_ERR_STATE, "key codec: observe after seal (reset first)");
    HJ_HIP(hipSetDevice(kc->device));
    HJ_HIP(hj::keys_observe(kc->plan, kc->ncols, kc->w64, kcols, n, (hipStream_t)stream));
    return HJ_OK;
}

int hj_dev_keycodec_seal(hj_keycodec *kc, void *stream) {
    if (!kc) HJ_FAIL(HJ_ERR_ARG, "null codec");
    HJ_HIP(hipSetDevice(kc->device));
    HJ_HIP(hj::keys_seal(kc->plan, kc->ncols, (hipStream_t)stream));
    kc->sealed = true;
    return HJ_OK;
}

int hj_dev_keycodec_pack(hj_keycodec *kc, const void *const cols[], int64_t n, int64_t *out_key, void *stream) {
    if (!kc) HJ_FAIL(HJ_ERR_ARG, "null codec");
    hj::KeyCols kcols;
    HJ_TRY(keys_cols(kc, cols, n, &kcols));
    if (n > 0 && !out_key) HJ_FAIL(HJ_ERR_ARG, "null output");
    if (!kc->sealed) HJ_FAIL(HJ_ERR_STATE, "key codec: pack before seal");
    HJ_HIP(hipSetDevice(kc->device));
    HJ_HIP(hj::keys_pack(kc->plan, kc->ncols, kc->w64, kcols, nullptr, n, (unsigned long long *)out_key, false,
                         (hipStream_t)stream));
    return HJ_OK;
}

int hj_dev_keycodec_pack_tuples(hj_keycodec *kc, const void *const cols[], const int64_t *pay, int64_t n,
                                int64_t *out_tuples, void *stream) {
    if (!kc) HJ_FAIL(HJ_ERR_ARG, "null codec");
    hj::KeyCols kcols;
    HJ_TRY(keys_cols(kc, cols, n, &kcols));
    if (n > 0 && !pay) HJ_FAIL(HJ_ERR_ARG, "bad column set: null payload column");
    if (n > 0 && !out_tuples) HJ_FAIL(HJ_ERR_ARG, "null output");
    if (!kc->sealed) HJ_FAIL(HJ_ERR_STATE, "key codec: pack before seal");
    HJ_HIP(hipSetDevice(kc->device));
    HJ_HIP(hj::keys_pack(kc->plan, kc->ncols, kc->w64, kcols, (const long long *)pay, n,
                         (unsigned long long *)out_tuples, true, (hipStream_t)stream));
    return HJ_OK;
}

int hj_dev_keycodec_unpack(hj_keycodec *kc, const int64_t *key, int64_t n, void *const out_cols[], void *stream) {
    if (!kc) HJ_FAIL(HJ_ERR_ARG, "null codec");
    if (n < 0) HJ_FAIL(HJ_ERR_ARG, "negative row count");
    if (n > 0 && !key) HJ_FAIL(HJ_ERR_ARG, "bad column set: null key column");
    if (n > 0 && !out_cols) HJ_FAIL(HJ_ERR_ARG, "null output");
    if (!kc->sealed) HJ_FAIL(HJ_ERR_STATE, "key codec: unpack before seal");
    hj::KeyOutCols o;
    for (int c = 0; c < hj::kKeysMaxCols; ++c) o.p[c] = n > 0 && c < kc->ncols ? out_cols[c] : nullptr;
    HJ_HIP(hipSetDevice(kc->device));
    HJ_HIP(hj::keys_unpack(kc->plan, kc->ncols, kc->w64, (const unsigned long long *)key, n, o, (hipStream_t)stream));
    return HJ_OK;
}

int hj_keycodec_info(hj_keycodec *kc, int *total_bits, int bits[4], int64_t lo[4], int64_t hi[4],
                     uint64_t *rows_observed, uint64_t *rows_out_of_range) {
    if (!kc) HJ_FAIL(HJ_ERR_ARG, "null codec");
    if (!kc->sealed) HJ_FAIL(HJ_ERR_STATE, "key codec: info before seal");
    hj::KeyPlan p;
    HJ_HIP(hipSetDevice(kc->device));
    HJ_HIP(hipDeviceSynchronize());
    HJ_HIP(hipMemcpy(&p, kc->plan, sizeof(p), hipMemcpyDeviceToHost));
    if (total_bits) *total_bits = p.total;
    for (int c = 0; c < hj::kKeysMaxCols; ++c) {
        if (bits) bits[c] = p.bits[c];
        if (lo) lo[c] = p.lo[c];
        if (hi) hi[c] = p.hi[c];
    }
    if (rows_observed) *rows_observed = p.rows;
    if (rows_out_of_range) *rows_out_of_range = p.oor;
    if (p.range) {
        std::string w;
        for (int c = 0; c < kc->ncols; ++c) w += (c ? " + " : "") + std::to_string(p.bits[c]);
        HJ_FAIL(HJ_ERR_RANGE, "key codec: the columns' joint range needs " + w + " = " + std::to_string(p.total) +
                                  " bits, more than 64");
    }
    return HJ_OK;
}

}  // extern "C"

// -------------------------------------------------------------- key filter
// A key filter: the words (its own or the caller's) and apply's workspace --
// tile counts, scan sums and the row bitmap in ONE grow-only allocation.
struct hj_filter {
    int device = 0;
    int64_t nblocks = 0;
    unsigned *words = nullptr;   // device, nblocks * 8 words
    bool owns = false;
    void *work = nullptr;        // device
    int64_t work_rows = -1;      // rows the workspace admits
    hj::FilterWork ws{nullptr, nullptr, nullptr};
};

namespace {

constexpr int64_t kFilterMaxBlocks = (int64_t(1) << 31) - 1;

int filter_work(hj_filter *f, int64_t rows) {
    if (rows <= f->work_rows) return HJ_OK;
    const size_t nt = hj::filter_tiles(rows) + 1;
    const size_t tiles_b = (nt * 8 + 15) & ~size_t(15), sums_b = (hj::exclusive_scan_sums(nt) * 8 + 15) & ~size_t(15);
    const size_t map_b = hj::filter_bitmap_bytes(rows) + 16;
    HJ_HIP(hipSetDevice(f->device));
    if (f->work) HJ_HIP(hipFree(f->work));   // (waits for the device: nothing in flight reads the old one)
    f->work = nullptr;
    f->work_rows = -1;
    if (hipMalloc(&f->work, tiles_b + sums_b + map_b) != hipSuccess) {
        (void)hipGetLastError();
        HJ_FAIL(HJ_ERR_NOMEM, "key filter: hipMalloc of the apply workspace for " + std::to_string(rows) + " rows");
    }
    f->ws.tiles = (unsigned long long *)f->work;
    f->ws.sums = (unsigned long long *)((char *)f->work + tiles_b);
    f->ws.bitmap = (unsigned char *)f->work + tiles_b + sums_b;
    f->work_rows = rows;
    return HJ_OK;
}

int filter_insert(hj_filter *f, int form, const void *key, int64_t n, void *stream) {
    if (!f) HJ_FAIL(HJ_ERR_ARG, "null filter");
    if (n < 0 || (n > 0 && !key)) HJ_FAIL(HJ_ERR_ARG, "bad relation: null keys or a negative row count");
    HJ_HIP(hipSetDevice(f->device));
    HJ_HIP(hj::filter_insert(f->words, f->nblocks, form, key, n, (hipStream_t)stream));
    return HJ_OK;
}

// any_out: some output pointer is non-null; rel_err: what is wrong with the relation (null: nothing)
int filter_apply(hj_filter *f, int form, int kind, const void *key, const int64_t *pay, int64_t n, int64_t row_base,
                 const char *rel_err, void *out_key, void *out_pay, void *out_row, int64_t cap, uint64_t *d_count,
                 void *stream) {
    if (!f) HJ_FAIL(HJ_ERR_ARG, "null filter");
    if (kind != HJ_FILTER_PASS && kind != HJ_FILTER_REJECT) HJ_FAIL(HJ_ERR_ARG, "unknown filter kind");
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (n < 0 || (n > 0 && !key)) HJ_FAIL(HJ_ERR_ARG, "bad relation: null keys or a negative row count");
    if (rel_err) HJ_FAIL(HJ_ERR_ARG, std::string("bad relation: ") + rel_err);
    const bool any_out = out_key || out_pay || out_row;
    if (cap < 0) HJ_FAIL(HJ_ERR_ARG, "negative output capacity");
    if (cap > 0 && !any_out) HJ_FAIL(HJ_ERR_ARG, "out_cap > 0 with every output null (the count form is out_cap == 0)");
    if (cap == 0 && any_out) HJ_FAIL(HJ_ERR_ARG, "out_cap == 0 with an output (the count form takes none)");
    HJ_TRY(filter_work(f, n));
    HJ_HIP(hipSetDevice(f->device));
    HJ_HIP(hj::filter_apply(f->words, f->nblocks, form, kind, key, (const long long *)pay, n, row_base, out_key,
                            out_pay, out_row, cap, (unsigned long long *)d_count, f->ws, (hipStream_t)stream));
    return HJ_OK;
}

}  // namespace

extern "C" {

int64_t hj_filter_blocks_for(int64_t n_keys, int bits_per_key) {
    if (n_keys < 0 || bits_per_key < 4 || bits_per_key > 64) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "key filter: n_keys >= 0 and bits_per_key in 4..64");
        return HJ_ERR_ARG;
    }
    const unsigned __int128 bits = (unsigned __int128)n_keys * (unsigned)bits_per_key;
    const unsigned __int128 blocks = (bits + 255) / 256;
    if (blocks > (unsigned __int128)kFilterMaxBlocks) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "key filter: more than 2^31 - 1 blocks");
        return HJ_ERR_ARG;
    }
    return blocks ? (int64_t)blocks : 1;
}

int hj_filter_place(int64_t key, int64_t nblocks, int64_t *block, uint32_t mask[8]) {
    if (nblocks < 1 || nblocks > kFilterMaxBlocks) HJ_FAIL(HJ_ERR_ARG, "key filter: nblocks must be in [1, 2^31)");
    const uint64_t h = hj::filter_hash(key);
    if (block) *block = (int64_t)hj::filter_block(h, (uint64_t)nblocks);
    if (mask)
        for (int w = 0; w < 8; ++w) mask[w] = hj::filter_mask((uint32_t)h, w);
    return HJ_OK;
}

hj_filter *hj_filter_create(int device, int64_t nblocks, void *d_words) {
    // the arguments first, before anything touches a device
    if (nblocks < 1 || nblocks > kFilterMaxBlocks) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "key filter: nblocks must be in [1, 2^31)");
        return nullptr;
    }
    if (((uintptr_t)d_words) & 31) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "key filter: the words buffer must be 32-byte aligned");
        return nullptr;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        fail(HJ_ERR_HIP, __FILE__, __LINE__, "no HIP device visible");
        return nullptr;
    }
    if (device < 0 || device >= n) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "device index out of range");
        return nullptr;
    }
    hj_filter *f = new hj_filter();
    f->device = device;
    f->nblocks = nblocks;
    f->words = (unsigned *)d_words;
    if (!d_words) {
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipMalloc((void **)&f->words, (size_t)nblocks * 32);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            fail(e == hipErrorOutOfMemory ? HJ_ERR_NOMEM : HJ_ERR_HIP, __FILE__, __LINE__,
                 std::string("key filter: ") + hipGetErrorString(e));
            delete f;
            return nullptr;
        }
        f->owns = true;
    }
    return f;
}

void hj_filter_destroy(hj_filter *f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    (void)hipDeviceSynchronize();
    if (f->owns && f->words) (void)hipFree(f->words);
    if (f->work) (void)hipFree(f->work);
    delete f;
}

int hj_filter_words(hj_filter *f, void **d_words, int64_t *nblocks) {
    if (!f) HJ_FAIL(HJ_ERR_ARG, "null filter");
    if (d_words) *d_words = f->words;
    if (nblocks) *nblocks = f->nblocks;
    return HJ_OK;
}

int hj_filter_reserve(hj_filter *f, int64_t max_rows) {
    if (!f) HJ_FAIL(HJ_ERR_ARG, "null filter");
    if (max_rows < 0) HJ_FAIL(HJ_ERR_ARG, "negative row count");
    return filter_work(f, max_rows);
}

int hj_dev_filter_clear(hj_filter *f, void *stream) {
    if (!f) HJ_FAIL(HJ_ERR_ARG, "null filter");
    HJ_HIP(hipSetDevice(f->device));
    HJ_HIP(hj::filter_clear(f->words, f->nblocks, (hipStream_t)stream));
    return HJ_OK;
}

int hj_dev_filter_insert_i64(hj_filter *f, const int64_t *key, int64_t n, void *stream) {
    return filter_insert(f, hj::kCols64, key, n, stream);
}

int hj_dev_filter_insert_tuples_i64(hj_filter *f, const int64_t *tuples, int64_t n, void *stream) {
    return filter_insert(f, hj::kPacked64, tuples, n, stream);
}

int hj_dev_filter_insert_i32(hj_filter *f, const int32_t *key, int64_t n, void *stream) {
    return filter_insert(f, hj::kCol32, key, n, stream);
}

int hj_dev_filter_merge(hj_filter *f, const hj_filter *other, void *stream) {
    if (!f) HJ_FAIL(HJ_ERR_ARG, "null filter");
    if (!other) HJ_FAIL(HJ_ERR_ARG, "key filter: null filter to merge in");
    if (other->nblocks != f->nblocks || other->device != f->device)
        HJ_FAIL(HJ_ERR_ARG, "key filter: merge of filters of different geometry (" + std::to_string(f->nblocks) +
                                " and " + std::to_string(other->nblocks) + " blocks) or devices");
    HJ_HIP(hipSetDevice(f->device));
    HJ_HIP(hj::filter_merge(f->words, other->words, f->nblocks, (hipStream_t)stream));
    return HJ_OK;
}

int hj_dev_filter_apply_i64(hj_filter *f, int kind, const int64_t *skey, const int64_t *spay, int64_t n,
                            int64_t *out_key, int64_t *out_pay, int64_t *out_row, int64_t out_cap, uint64_t *d_count,
                            void *stream) {
    const bool no_pay = n > 0 && out_pay && !spay;
    return filter_apply(f, hj::kCols64, kind, skey, spay, n, 0, no_pay ? "null payload column" : nullptr, out_key,
                        out_pay, out_row, out_cap, d_count, stream);
}

int hj_dev_filter_apply_tuples_i64(hj_filter *f, int kind, const int64_t *tuples, int64_t n, int64_t *out_tuples,
                                   int64_t *out_row, int64_t out_cap, uint64_t *d_count, void *stream) {
    return filter_apply(f, hj::kPacked64, kind, tuples, nullptr, n, 0, nullptr, out_tuples, nullptr, out_row, out_cap,
                        d_count, stream);
}

int hj_dev_filter_apply_i32(hj_filter *f, int kind, const int32_t *skey, int64_t n, int64_t row_base,
                            int32_t *out_key, int32_t *out_row, int64_t out_cap, uint64_t *d_count, void *stream) {
    const bool bad_ids = n >= 0 && (row_base < 0 || row_base > INT32_MAX - n);
    return filter_apply(f, hj::kCol32, kind, skey, nullptr, n, bad_ids ? 0 : row_base,
                        bad_ids ? "row ids past 2^31 - 1" : nullptr, out_key, nullptr, out_row, out_cap, d_count,
                        stream);
}

}  // extern "C"

// -------------------------------------------------------------- star probe
// A star probe object: the compaction workspace (tile counts, scan sums, one
// result byte per lane: the key filter's shape) in ONE grow-only allocation,
// and the host facts of the last call.  The contexts it probes are only read.
struct hj_star {
    int device = 0;
    void *work = nullptr;        // device
    int64_t work_rows = -1;      // rows the workspace admits
    hj::FilterWork ws{nullptr, nullptr, nullptr};
    hj::StarPlan plan{0, 0u, 0, 0, 0};
    // the star aggregate's group table (wide) with its accumulators and two meta words, ONE grow-only allocation
    void *groups = nullptr;      // device
    int group_bits = 0;          // capacity 2^group_bits (0: no reserve yet)
};

namespace {

static_assert(HJ_STAR_INNER == hj::kStarInner && HJ_STAR_LEFT == hj::kStarLeft && HJ_STAR_ANTI == hj::kStarAnti &&
                  HJ_STAR_MAX_DIMS == hj::kStarMaxDims,
              "hj.h's star constants are the kernels'");

int star_work(hj_star *s, int64_t rows) {
    if (rows <= s->work_rows) return HJ_OK;
    const size_t nt = hj::filter_tiles(rows) + 1;
    const size_t tiles_b = (nt * 8 + 15) & ~size_t(15), sums_b = (hj::exclusive_scan_sums(nt) * 8 + 15) & ~size_t(15);
    const size_t map_b = hj::filter_tiles(rows) * hj::kFilterBlock + 16;
    HJ_HIP(hipSetDevice(s->device));
    if (s->work) HJ_HIP(hipFree(s->work));   // (waits for the device: nothing in flight reads the old one)
    s->work = nullptr;
    s->work_rows = -1;
    if (hipMalloc(&s->work, tiles_b + sums_b + map_b) != hipSuccess) {
        (void)hipGetLastError();
        HJ_FAIL(HJ_ERR_NOMEM, "star probe: hipMalloc of the workspace for " + std::to_string(rows) + " rows");
    }
    s->ws.tiles = (unsigned long long *)s->work;
    s->ws.sums = (unsigned long long *)((char *)s->work + tiles_b);
    s->ws.bitmap = (unsigned char *)s->work + tiles_b + sums_b;
    s->work_rows = rows;
    return HJ_OK;
}

// The checks every star entry point makes first, in hj.h's order.  what: its name in the messages; least: the fewest
// dimensions it takes; grouped: it takes gshift, whose checks sit between the device's and the layout's.
int star_check_dims(const std::string &what, int layout, int ndims, int least, const hj_star *s, hj_ctx *const dims[],
                    const int kinds[], const void *skeys, const void *null_pay, const int gshift[], bool grouped) {
    if (!s) HJ_FAIL(HJ_ERR_ARG, "null star");
    if (ndims < least || ndims > HJ_STAR_MAX_DIMS)
        HJ_FAIL(HJ_ERR_ARG,
                what + ": ndims must be in " + std::to_string(least) + ".." + std::to_string(HJ_STAR_MAX_DIMS));
    if (ndims > 0 && (!dims || !kinds || !skeys || !null_pay || (grouped && !gshift)))
        HJ_FAIL(HJ_ERR_ARG, what + ": null dims, kinds, skeys" +
                                (grouped ? ", null-value or gshift array" : " or null-value array"));
    for (int d = 0; d < ndims; ++d) {
        const std::string who = what + ": dimension " + std::to_string(d);
        const hj_ctx *c = dims[d];
        if (!c) HJ_FAIL(HJ_ERR_ARG, who + ": null context");
        if (kinds[d] != HJ_STAR_INNER && kinds[d] != HJ_STAR_LEFT && kinds[d] != HJ_STAR_ANTI)
            HJ_FAIL(HJ_ERR_ARG, who + ": kind must be HJ_STAR_INNER, HJ_STAR_LEFT or HJ_STAR_ANTI");
        if (c->device != s->device) HJ_FAIL(HJ_ERR_ARG, who + ": a context of another device");
        if (grouped) {
            if (gshift[d] < -1 || gshift[d] > 63) HJ_FAIL(HJ_ERR_ARG, who + ": gshift must be -1 or in 0..63");
            if (kinds[d] == HJ_STAR_ANTI && gshift[d] >= 0)
                HJ_FAIL(HJ_ERR_ARG, who + ": an ANTI dimension has no payload to group by");
        }
        if (c->layout != layout) HJ_FAIL(HJ_ERR_STATE, who + ": no build of this layout");
        if (c->used != HJ_STRATEGY_GLOBAL && !c->dual)
            HJ_FAIL(HJ_ERR_STATE, who + ": a radix-only build has no global table (build it under HJ_STRATEGY_GLOBAL)");
    }
    return HJ_OK;
}

int star_check_rows(const uint64_t *d_count, int64_t n, int ndims, const void *const skeys[]) {
    if (!d_count) HJ_FAIL(HJ_ERR_ARG, "null count pointer");
    if (n < 0) HJ_FAIL(HJ_ERR_ARG, "bad probe relation: a negative row count");
    for (int d = 0; d < ndims; ++d)
        if (n > 0 && !skeys[d]) HJ_FAIL(HJ_ERR_ARG, "bad probe relation: dimension " + std::to_string(d) + " has null keys");
    return HJ_OK;
}

int star_check_cap(int64_t cap, bool any_out) {
    if (cap < 0) HJ_FAIL(HJ_ERR_ARG, "negative output capacity");
    if (cap > 0 && !any_out) HJ_FAIL(HJ_ERR_ARG, "out_cap > 0 with every output null (the count form is out_cap == 0)");
    if (cap == 0 && any_out) HJ_FAIL(HJ_ERR_ARG, "out_cap == 0 with an output (the count form takes none)");
    return HJ_OK;
}

void star_fill_dims(hj::StarDim (&sd)[HJ_STAR_MAX_DIMS], int ndims, hj_ctx *const dims[], const int kinds[],
                    const void *const skeys[], const unsigned long long null_pay[], void *const out_pay[]) {
    for (int d = 0; d < ndims; ++d)
        sd[d] = hj::StarDim{table_dev(dims[d]), skeys[d], out_pay ? out_pay[d] : nullptr, null_pay[d], kinds[d], -1};
}

// An _i32 entry point's null rows as the kernels' 64-bit null payloads, sign-extended into v; null stays null.
const unsigned long long *widen_nulls(const int32_t null_row[], int ndims, unsigned long long (&v)[HJ_STAR_MAX_DIMS]) {
    for (int d = 0; null_row && d < ndims && d < HJ_STAR_MAX_DIMS; ++d)
        v[d] = (unsigned long long)(long long)null_row[d];
    return null_row ? v : nullptr;
}

// Both entry points behind their casts: the checks in hj.h's order, then the launches.
int do_star(hj_star *s, int layout, int ndims, hj_ctx *const dims[], const int kinds[], const void *const skeys[],
            const unsigned long long null_pay[], int64_t n, int64_t row_base, void *const out_pay[], void *out_row,
            int64_t cap, uint64_t *d_count, void *stream) {
    HJ_TRY(star_check_dims("star probe", layout, ndims, 1, s, dims, kinds, skeys, null_pay, nullptr, false));
    HJ_TRY(star_check_rows(d_count, n, ndims, skeys));
    bool any_out = out_row != nullptr;
    for (int d = 0; d < ndims; ++d) {
        void *o = out_pay ? out_pay[d] : nullptr;
        if (o && kinds[d] == HJ_STAR_ANTI)
            HJ_FAIL(HJ_ERR_ARG, "star probe: dimension " + std::to_string(d) + ": an ANTI dimension has no payload column");
        any_out |= o != nullptr;
    }
    HJ_TRY(star_check_cap(cap, any_out));
    if (layout == kNarrow && (row_base < 0 || row_base > INT32_MAX - n)) HJ_FAIL(HJ_ERR_ARG, "row ids past 2^31 - 1");
    HJ_TRY(star_work(s, n));
    HJ_HIP(hipSetDevice(s->device));
    hj::StarArgs a{};
    star_fill_dims(a.d, ndims, dims, kinds, skeys, null_pay, out_pay);
    a.n = n;
    a.row_base = row_base;
    a.cap = cap;
    a.out_row = out_row;
    a.count = (unsigned long long *)d_count;
    HJ_HIP(hj::launch_star(layout, ndims, a, s->ws, &s->plan, (hipStream_t)stream));
    return HJ_OK;
}

// The group table's parts inside hj_star::groups: slots, then count, sum, min and max of slots + 1 entries, then meta.
struct StarGroups {
    hj::TableDev t;
    hj::GroupAcc acc;
};
size_t star_groups_bytes(int bits) {
    const size_t cap = size_t(1) << bits;
    return cap * 16 + 4 * (cap + 1) * 8 + 64;
}
StarGroups star_groups(const hj_star *s) {
    const size_t cap = size_t(1) << s->group_bits, col = (cap + 1) * 8;
    char *p = (char *)s->groups;
    StarGroups g;
    g.t.slots = p;
    g.t.mask = cap - 1;
    g.t.shift = 64 - s->group_bits;
    g.t.side = nullptr;
    g.acc.cnt = p + cap * 16;
    g.acc.sum = (unsigned long long *)(p + cap * 16 + col);
    g.acc.mn = p + cap * 16 + 2 * col;
    g.acc.mx = p + cap * 16 + 3 * col;
    g.t.meta = (unsigned long long *)(p + cap * 16 + 4 * col);
    return g;
}

// The star aggregate's and the star query's entry points behind their casts: the checks in hj.h's order, then the
// launches.  query: hj_dev_star_query_* (ndims == 0 is legal, `fact` may be given); else fact is null.
int do_star_aggregate(hj_star *s, int layout, int ndims, hj_ctx *const dims[], const int kinds[],
                      const void *const skeys[], const unsigned long long null_pay[], const int gshift[],
                      const int64_t gbase[], const void *sval, int64_t n, void *out_key, void *out_cnt, void *out_sum,
                      void *out_min, void *out_max, int64_t cap, uint64_t *d_count, void *stream,
                      const hj_star_fact *fact = nullptr, bool query = false) {
    const std::string what = query ? "star query" : "star aggregate";
    HJ_TRY(star_check_dims(what, layout, ndims, query ? 0 : 1, s, dims, kinds, skeys, null_pay, gshift, true));
    if (fact) {
        if (fact->npreds < 0 || fact->npreds > HJ_STAR_MAX_PREDS)
            HJ_FAIL(HJ_ERR_ARG, "star query: fact.npreds must be in 0.." + std::to_string(HJ_STAR_MAX_PREDS));
        for (int p = 0; p < fact->npreds; ++p)
            if (fact->pkind[p] != HJ_PRED_IN && fact->pkind[p] != HJ_PRED_OUT)
                HJ_FAIL(HJ_ERR_ARG, "star query: fact.pkind[" + std::to_string(p) + "] must be HJ_PRED_IN or HJ_PRED_OUT");
        if (fact->vop < HJ_VALUE_A || fact->vop > HJ_VALUE_MUL)
            HJ_FAIL(HJ_ERR_ARG, "star query: fact.vop must be HJ_VALUE_A, _ADD, _SUB or _MUL");
        if (fact->nfact < 0 || fact->nfact > HJ_STAR_MAX_FACT_GROUPS)
            HJ_FAIL(HJ_ERR_ARG, "star query: fact.nfact must be in 0.." + std::to_string(HJ_STAR_MAX_FACT_GROUPS));
        for (int f = 0; f < fact->nfact; ++f)
            if (fact->fshift[f] < 0 || fact->fshift[f] > 63)
                HJ_FAIL(HJ_ERR_ARG, "star query: fact.fshift[" + std::to_string(f) + "] must be in 0..63");
    }
    if (!s->groups) HJ_FAIL(HJ_ERR_STATE, what + ": no group table (call hj_star_reserve_groups first)");
    HJ_TRY(star_check_rows(d_count, n, ndims, skeys));
    if (fact && n > 0) {
        for (int p = 0; p < fact->npreds; ++p)
            if (!fact->pcol[p]) HJ_FAIL(HJ_ERR_ARG, "bad probe relation: fact.pcol[" + std::to_string(p) + "] is null");
        for (int f = 0; f < fact->nfact; ++f)
            if (!fact->fcol[f]) HJ_FAIL(HJ_ERR_ARG, "bad probe relation: fact.fcol[" + std::to_string(f) + "] is null");
    }
    const bool vals = out_sum || out_min || out_max;
    if (vals && !sval && n > 0) HJ_FAIL(HJ_ERR_ARG, what + ": sum, min or max without a value column");
    if (fact && fact->vop != HJ_VALUE_A && vals && !fact->vb && n > 0)
        HJ_FAIL(HJ_ERR_ARG, "star query: fact.vb is null under a vop other than HJ_VALUE_A with sum, min or max asked for");
    HJ_TRY(star_check_cap(cap, out_key || out_cnt || vals));
    HJ_HIP(hipSetDevice(s->device));
    const StarGroups g = star_groups(s);
    hj::StarAggArgs a{};
    star_fill_dims(a.d, ndims, dims, kinds, skeys, null_pay, nullptr);
    for (int d = 0; d < HJ_STAR_MAX_DIMS; ++d) {
        a.gshift[d] = d < ndims ? gshift[d] : -1;
        a.gbase[d] = d < ndims && gbase ? gbase[d] : 0;
    }
    a.sval = vals ? sval : nullptr;
    a.n = n;
    a.gt = g.t;
    a.acc = hj::GroupAcc{g.acc.cnt, out_sum ? g.acc.sum : nullptr, out_min ? g.acc.mn : nullptr,
                         out_max ? g.acc.mx : nullptr};
    // the fact side; one that asks for nothing (and a dimension to walk) is the star aggregate's own kernel
    bool fact_pass = ndims == 0;
    hj::StarFact ff{};
    if (fact) {
        static_assert(hj::kStarMaxPreds == HJ_STAR_MAX_PREDS && hj::kStarMaxFactGroups == HJ_STAR_MAX_FACT_GROUPS &&
                      hj::kStarValueMul == HJ_VALUE_MUL, "hj.h and hj_internal.h agree");
        ff.npreds = fact->npreds;
        for (int p = 0; p < fact->npreds; ++p) {
            ff.pcol[p] = fact->pcol[p];
            ff.plo[p] = fact->plo[p];
            ff.phi[p] = fact->phi[p];
            ff.pkind[p] = fact->pkind[p];
        }
        ff.vop = vals ? fact->vop : HJ_VALUE_A;
        ff.vb = ff.vop != HJ_VALUE_A ? fact->vb : nullptr;
        ff.nfact = fact->nfact;
        for (int f = 0; f < fact->nfact; ++f) {
            ff.fcol[f] = fact->fcol[f];
            ff.fshift[f] = fact->fshift[f];
            ff.fbase[f] = fact->fbase[f];
        }
        fact_pass |= fact->npreds > 0 || ff.vop != HJ_VALUE_A || fact->nfact > 0;
    }
    const hj::GroupOut out{out_key, out_cnt, out_sum, out_min, out_max, cap, (unsigned long long *)d_count, 0ull, 0};
    HJ_HIP(hj::launch_star_aggregate(layout, ndims, a, out, &s->plan, (hipStream_t)stream,
                                     fact_pass ? &ff : nullptr));
    return HJ_OK;
}

}  // namespace

extern "C" {

hj_star *hj_star_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        fail(HJ_ERR_HIP, __FILE__, __LINE__, "no HIP device visible");
        return nullptr;
    }
    if (device < 0 || device >= n) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "device index out of range");
        return nullptr;
    }
    // (here, not in a call: a launch above 64 KiB of dynamic LDS needs the attribute, and a call may be under capture)
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hj::star_prepare();
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fail(HJ_ERR_HIP, __FILE__, __LINE__, std::string("star probe: ") + hipGetErrorString(e));
        return nullptr;
    }
    hj_star *s = new hj_star();
    s->device = device;
    return s;
}

void hj_star_destroy(hj_star *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    if (s->work) (void)hipFree(s->work);
    if (s->groups) (void)hipFree(s->groups);
    delete s;
}

int hj_star_reserve_groups(hj_star *s, int64_t max_groups) {
    if (!s) HJ_FAIL(HJ_ERR_ARG, "null star");
    if (max_groups < 0 || max_groups > (int64_t(1) << 40)) HJ_FAIL(HJ_ERR_ARG, "bad group count");
    int bits = ceil_log2(2ull * (unsigned long long)max_groups);
    if (bits < 11) bits = 11;   // at least one emit tile of slots
    if (bits <= s->group_bits) return HJ_OK;
    HJ_HIP(hipSetDevice(s->device));
    if (s->groups) HJ_HIP(hipFree(s->groups));   // (waits for the device: nothing in flight reads the old one)
    s->groups = nullptr;
    s->group_bits = 0;
    if (hipMalloc(&s->groups, star_groups_bytes(bits)) != hipSuccess) {
        (void)hipGetLastError();
        HJ_FAIL(HJ_ERR_NOMEM, "star aggregate: hipMalloc of the group table for " + std::to_string(max_groups) + " groups");
    }
    s->group_bits = bits;
    return HJ_OK;
}

int64_t hj_star_group_capacity(const hj_star *s) {
    if (!s) {
        fail(HJ_ERR_ARG, __FILE__, __LINE__, "null star");
        return HJ_ERR_ARG;
    }
    return s->groups ? int64_t(1) << s->group_bits : 0;
}

int hj_dev_star_aggregate_i64(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[],
                              const int64_t *const skeys[], const int64_t null_pay[], const int gshift[],
                              const int64_t gbase[], const int64_t *sval, int64_t n, int64_t *out_key, int64_t *out_cnt,
                              int64_t *out_sum, int64_t *out_min, int64_t *out_max, int64_t out_cap, uint64_t *d_count,
                              void *stream) {
    return do_star_aggregate(s, kWide, ndims, dims, kinds, (const void *const *)skeys,
                             (const unsigned long long *)null_pay, gshift, gbase, sval, n, out_key, out_cnt, out_sum,
                             out_min, out_max, out_cap, d_count, stream);
}

int hj_dev_star_aggregate_i32(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[],
                              const int32_t *const skeys[], const int32_t null_row[], const int gshift[],
                              const int64_t gbase[], const int32_t *sval, int64_t n, int64_t *out_key, int64_t *out_cnt,
                              int64_t *out_sum, int64_t *out_min, int64_t *out_max, int64_t out_cap, uint64_t *d_count,
                              void *stream) {
    unsigned long long w[HJ_STAR_MAX_DIMS] = {};
    return do_star_aggregate(s, kNarrow, ndims, dims, kinds, (const void *const *)skeys,
                             widen_nulls(null_row, ndims, w), gshift, gbase, sval, n, out_key, out_cnt, out_sum,
                             out_min, out_max, out_cap, d_count, stream);
}

int hj_dev_star_query_i64(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[],
                          const int64_t *const skeys[], const int64_t null_pay[], const int gshift[],
                          const int64_t gbase[], const hj_star_fact *fact, const int64_t *sval, int64_t n,
                          int64_t *out_key, int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                          int64_t out_cap, uint64_t *d_count, void *stream) {
    return do_star_aggregate(s, kWide, ndims, dims, kinds, (const void *const *)skeys,
                             (const unsigned long long *)null_pay, gshift, gbase, sval, n, out_key, out_cnt, out_sum,
                             out_min, out_max, out_cap, d_count, stream, fact, true);
}

int hj_dev_star_query_i32(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[],
                          const int32_t *const skeys[], const int32_t null_row[], const int gshift[],
                          const int64_t gbase[], const hj_star_fact *fact, const int32_t *sval, int64_t n,
                          int64_t *out_key, int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                          int64_t out_cap, uint64_t *d_count, void *stream) {
    unsigned long long w[HJ_STAR_MAX_DIMS] = {};
    return do_star_aggregate(s, kNarrow, ndims, dims, kinds, (const void *const *)skeys,
                             widen_nulls(null_row, ndims, w), gshift, gbase, sval, n, out_key, out_cnt, out_sum,
                             out_min, out_max, out_cap, d_count, stream, fact, true);
}

int hj_star_reserve(hj_star *s, int64_t max_rows) {
    if (!s) HJ_FAIL(HJ_ERR_ARG, "null star");
    if (max_rows < 0) HJ_FAIL(HJ_ERR_ARG, "negative row count");
    return star_work(s, max_rows);
}

int hj_star_last_plan(const hj_star *s, int *launches, int *grid, int64_t *tiles, int *lds_dims, int64_t *lds_bytes) {
    if (!s) HJ_FAIL(HJ_ERR_ARG, "null star");
    if (launches) *launches = s->plan.launches;
    if (grid) *grid = (int)s->plan.grid;
    if (tiles) *tiles = s->plan.tiles;
    if (lds_dims) *lds_dims = s->plan.lds_dims;
    if (lds_bytes) *lds_bytes = s->plan.lds_bytes;
    return HJ_OK;
}

int hj_dev_star_i64(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[], const int64_t *const skeys[],
                    const int64_t null_pay[], int64_t n, int64_t *const out_pay[], int64_t *out_row, int64_t out_cap,
                    uint64_t *d_count, void *stream) {
    return do_star(s, kWide, ndims, dims, kinds, (const void *const *)skeys, (const unsigned long long *)null_pay, n, 0,
                   (void *const *)out_pay, out_row, out_cap, d_count, stream);
}

int hj_dev_star_i32(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[], const int32_t *const skeys[],
                    const int32_t null_row[], int64_t n, int64_t row_base, int32_t *const out_pay[], int32_t *out_row,
                    int64_t out_cap, uint64_t *d_count, void *stream) {
    unsigned long long w[HJ_STAR_MAX_DIMS] = {};
    return do_star(s, kNarrow, ndims, dims, kinds, (const void *const *)skeys, widen_nulls(null_row, ndims, w), n,
                   row_base, (void *const *)out_pay, out_row, out_cap, d_count, stream);
}

}  // extern "C"

void hj_placement_stats(long long *probes, long long *rejected, double *last_kept, double *worst_kept) {
    std::lock_guard<std::mutex> lk(g_place_mu);
    if (probes) *probes = g_place.probes;
    if (rejected) *rejected = g_place.rejected;
    if (last_kept) *last_kept = g_place.last_kept;
    if (worst_kept) *worst_kept = g_place.worst_kept;
}

void hj_placement_stats_ex(long long out[5], double *last_kept, double *worst_kept) {
    std::lock_guard<std::mutex> lk(g_place_mu);
    if (out) {
        out[0] = g_place.probes;
        out[1] = g_place.rejected;
        out[2] = g_place.gave_up;
        out[3] = g_place.gave_up_low_mem;
        out[4] = g_place.held_max;
    }
    if (last_kept) *last_kept = g_place.last_kept;
    if (worst_kept) *worst_kept = g_place.worst_kept;
}

double hj_placement_set_good(double ratio) {
    const float prev = g_place_good.load();
    if (ratio > 0.0) g_place_good.store((float)ratio);
    return (double)prev;
}

int hj_placement_check(const void *buf, int64_t bytes, double *ratio) {
    if (!buf || bytes <= 0 || !ratio) HJ_FAIL(HJ_ERR_ARG, "placement check: null buffer / ratio or no bytes");
    *ratio = 0.0;
    const int cus = hj::cu_count();
    float r = 0.0f;
    const hipError_t e = hj::placement_probe(const_cast<void *>(buf), (size_t)bytes, size_t(16) << hj::kPassPbl, cus, &r);
    if (e == hipErrorInvalidValue) HJ_FAIL(HJ_ERR_ARG, "placement check: buffer below 4 MiB per CU");
    HJ_HIP(e);
    *ratio = r;
    return HJ_OK;
}
