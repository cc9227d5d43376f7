/*
 * hj.h -- C ABI of the MI355X-native hash-join operator (libhj.so).
 *
 * Drop-in boundary for the reference's join program (deveshv-99/mlir-HashJoin,
 * SURVEY 8(b)).  Three layers, all plain C (pointers + sizes, no torch types):
 *
 *  1. Host memref ABI.  The reference's host functions take ranked 1-D
 *     memrefs, which MLIR's -finalize-memref-to-llvm / -convert-func-to-llvm
 *     expand into five scalars (allocated, aligned, offset, size, stride);
 *     see join_v1.ll:1262-1265 and shared_stuff/shared.cpp:35,59,83,129-132.
 *     hj_count_* / hj_probe_* use exactly that expansion, so a .mlir module
 *     declares them `func.func private` and links libhj.so through
 *     mlir-cpu-runner --shared-libs (run_test.sh:33), the way it links
 *     shared.so today (join_v1.mlir:651-658).
 *
 *  2. MLIR C-interface (`llvm.emit_c_interface`) one-memref-out joins:
 *     _mlir_ciface_hj_join_*(result*, R*, S*) -- the "two-memref-in /
 *     one-memref-out" entry point of north_star.  The result buffer is
 *     malloc'ed (allocated == aligned) so MLIR's memref.dealloc (free) or
 *     hj_free_result() releases it.
 *
 *  3. Device-resident phases (hj_dev_*): the hot path.  Inputs and outputs
 *     are device pointers, every call is asynchronous on the given HIP stream
 *     (NULL = default stream) and launches kernels only (no allocation, no
 *     synchronisation) once hj_ctx_reserve() has sized the workspace, so the
 *     sequence can be captured into a hipGraph.
 *
 * Semantics (all layers): an equi-join of R and S on the key column; the
 * output is the multiset {(R.pay[i], S.pay[j]) : R.key[i] == S.key[j]} --
 * every pair, duplicates on either side included, exactly the nested-loop
 * definition of shared_stuff/shared.cpp:154-165 (payload = row id in the
 * reference types).  Row order is unspecified (the reference's is decided by
 * atomics too); compare after sorting, as shared.cpp:168-171 does.
 *
 * Errors: functions returning int return HJ_OK (0) or a negative HJ_ERR_*;
 * hj_last_error() gives "file:line: message" of the last failure on this
 * thread.  The reference has no error channel besides check()'s 1/0/-1
 * (shared.cpp:158-171).
 */
#ifndef HJ_H_
#define HJ_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HJ_ABI_VERSION 1

#define HJ_OK 0
#define HJ_ERR_ARG (-1)      /* bad argument / size mismatch */
#define HJ_ERR_HIP (-2)      /* HIP runtime error (see hj_last_error) */
#define HJ_ERR_NOMEM (-3)    /* device or host allocation failed */
#define HJ_ERR_STATE (-4)    /* call order: probe before build, wrong layout */
#define HJ_ERR_CAPACITY (-5) /* output memref smaller than the join result */
#define HJ_ERR_RANGE (-6)        /* the columns' joint range needs more than 64 bits */

typedef struct hj_ctx hj_ctx;

int hj_abi_version(void);
const char *hj_last_error(void);
/* Device facts for the roofline: [0] CUs, [1] memory clock (kHz), [2] memory
 * bus width (bits), [3] L2 bytes (one XCD), [4] HBM bytes, [5] shader clock
 * (kHz), [6] LDS bytes per CU, [7] peak HBM MB/s = 4 x memory clock x bus
 * bytes (HBM3E: 4 transfers per reported clock). */
int hj_device_info(int device, int64_t out[8]);

/* ------------------------------------------------------------------ context
 * One context = one device + its hash-table workspace.  Replaces the
 * reference's @allocateHashTable (join_v2.mlir:25-39: gpu.alloc of heads and
 * linked list) -- allocation is hoisted out of the per-join path. */
hj_ctx *hj_ctx_create(int device);
void hj_ctx_destroy(hj_ctx *ctx);
/* Size the workspace for builds of up to max_build_rows rows with 32- or
 * 64-bit keys (key_bits = 32 | 64). */
int hj_ctx_reserve(hj_ctx *ctx, int64_t max_build_rows, int key_bits);
/* Probe-side workspace of the radix strategy (no-op for the global table). */
int hj_ctx_reserve_probe(hj_ctx *ctx, int64_t max_probe_rows, int key_bits);
/* Join strategy.  GLOBAL: one linear-probing table in HBM (build = 64-bit CAS
 * per row, probe = random slot reads).  RADIX: both relations radix-
 * partitioned by the key hash until a partition's build rows fit an LDS
 * table; partitions are joined in LDS.  AUTO picks RADIX for large build
 * sides.  The result multiset is identical. */
#define HJ_STRATEGY_AUTO 0
#define HJ_STRATEGY_GLOBAL 1
#define HJ_STRATEGY_RADIX 2
int hj_ctx_set_strategy(hj_ctx *ctx, int strategy);
/* RADIX: partition into exactly 2^bits partitions (1..24; 0 = planner's
 * choice, ~4096 build rows per partition).  For tests and tuning. */
int hj_ctx_set_radix_bits(hj_ctx *ctx, int bits);
/* Strategy of the last probe since the current build (else of the build):
 * HJ_STRATEGY_GLOBAL / _RADIX, 0 if none.  Under HJ_STRATEGY_AUTO a build side
 * of [2^18, 2^21) rows gets the global table AND a radix partition; a probe
 * side of >= 2^24 rows then takes the radix join. */
int hj_ctx_strategy_used(const hj_ctx *ctx);
/* The probe side's expected rows, given before the build (< 0: unknown, the
 * default).  AUTO with a [2^18, 2^21)-row build side then builds ONE
 * strategy instead of both: radix from 2^24 hinted probe rows on (2^22 for
 * build sides of >= 2^20 rows), else the global table (2^20 x 2^20: 0.21 ->
 * 0.15 ms per join; 2^20 x 2^22: 0.24 -> 0.20).  A later, larger probe still joins correctly, through
 * the global table.  HashJoin.join and the host memref entry points set it. */
int hj_ctx_probe_hint(hj_ctx *ctx, int64_t probe_rows);
/* GLOBAL: slot capacity of the table (power of two, >= 2 x build rows);
 * RADIX: number of partitions. */
int64_t hj_ctx_table_capacity(const hj_ctx *ctx);
/* RADIX: partition passes of the current build (1..3) and their fan-out bits
 * (bits[0..passes-1]); returns 0 passes for GLOBAL / no build. */
int hj_ctx_radix_plan(const hj_ctx *ctx, int *passes, int bits[3]);
/* 1 if the build side repeats a key, 0 if not (synchronises); INT64_MIN is a
 * key like any other here too: two build rows that hold it repeat it.  Known after
 * the build (GLOBAL) or after the first probe (RADIX: a repeat that a probe
 * row met is flagged by the join; the first call after a join whose kernel
 * was k_join_b checks every partition of the build side on the device,
 * including those no probe row reached and, after routed probes in several
 * bin ranges, every range). */
int hj_ctx_build_has_duplicates(hj_ctx *ctx);
/* Per-phase kernel timing with HIP events on the caller's stream. */
int hj_ctx_set_timing(hj_ctx *ctx, int enable);
/* ms of the last init, build, probe/count and partition launches (synchronises). */
int hj_ctx_last_timing(hj_ctx *ctx, float ms[4]);
/* Same plus the probe's split: [4] probe-side partitioning (RADIX, else 0),
 * [5] probe/join kernel; [6], [7] reserved (-1). */
int hj_ctx_last_timing_ex(hj_ctx *ctx, float ms[8]);
/* Accumulating timing (enable = 1; turns timing on): every build starts a
 * new event set of a 64-set ring and a set is read back only when the ring
 * comes round to it, so back-to-back build + probe steps run with no host
 * synchronisation between them (a probe repeated without a build replaces
 * that set's probe times).  Enabling again, or 0, drops what was recorded.
 * hj_ctx_timing_totals sums every recorded set (synchronises on them) into
 * ms[0..5] as hj_ctx_last_timing_ex orders them, *sets = how many, and
 * starts the totals again; HJ_ERR_STATE unless accumulating. */
int hj_ctx_timing_accumulate(hj_ctx *ctx, int enable);
int hj_ctx_timing_totals(hj_ctx *ctx, float ms[8], long long *sets);
/* RADIX: the join kernel of the last probe, whichever entry point ran it
 * (hj_dev_probe_*, hj_dev_probe_outer_*, hj_dev_probe_full_*, hj_dev_count_*, hj_dev_exists_*, hj_dev_lookup_*, hj_dev_asof_*, hj_dev_expand_*, and after a routed build
 * hj_dev_probe_routed_i64 too).  A pure function of the row
 * width, the probe / build size ratio (>= 8: the probe-heavy shape) and the
 * build side's repeated keys, sampled at build time over up to 64 partitions
 * -- never of an earlier join's statistics: HJ_JOIN_KERNEL_BUCKETED
 * (k_join_b), _STREAM (k_join_u, probe-heavy shape), _GROUPED (k_join_grp
 * over every item: most build keys repeated; i32 and, since round 5, int64
 * rows); 0 if the last probe was no radix join.  Items those kernels defer
 * (INT64_MIN build keys, oversized partitions) run k_join afterwards.
 * (_LINEAR, k_join_u outside the stream shape, and _GENERAL, k_join over
 * every int64 item, are no longer chosen since round 5.)  Synchronises. */
#define HJ_JOIN_KERNEL_BUCKETED 1
#define HJ_JOIN_KERNEL_LINEAR 2
#define HJ_JOIN_KERNEL_STREAM 3
#define HJ_JOIN_KERNEL_GROUPED 4
#define HJ_JOIN_KERNEL_GENERAL 5
/* k_join_exists: the last probe was a radix semi- / anti-join (hj_dev_exists_*) */
#define HJ_JOIN_KERNEL_EXISTS 6
/* k_join_lookup: the last probe was a radix positional lookup (hj_dev_lookup_*) */
#define HJ_JOIN_KERNEL_LOOKUP 7
/* k_join_group: the last probe was a radix group probe (hj_dev_group_*) */
#define HJ_JOIN_KERNEL_GROUP 8
/* k_join_aggregate: the last call was a radix hash aggregate (hj_dev_aggregate_*) */
#define HJ_JOIN_KERNEL_AGGREGATE 9
/* k_join_expand: the last probe was a radix expand (hj_dev_expand_*) */
#define HJ_JOIN_KERNEL_EXPAND 10
/* k_join_asof: the last probe was a radix as-of probe (hj_dev_asof_*) */
#define HJ_JOIN_KERNEL_ASOF 11   /* k_join_asof */
int hj_ctx_join_kernel(hj_ctx *ctx);

/* ------------------------------------------------------------ device phases
 * build:  @initializeHashTable + @buildTable   (join_v2.mlir:54-108)
 * count:  @countRows                           (join_v2.mlir:110-147)
 * probe:  @probeRelation                       (join_v2.mlir:149-199)
 * d_count (device uint64): set to M, the exact number of result rows, even
 * when M > out_cap (rows past out_cap are dropped; re-run with a larger
 * output).  The counter is zeroed by the call.  Bit 63 set means an internal
 * work list overflowed (a sizing bug, never expected): the result is invalid
 * and the host entry points return HJ_ERR_CAPACITY for it. */

/* 64-bit key / 64-bit payload column pairs (north_star types). */
int hj_dev_build_i64(hj_ctx *ctx, const int64_t *rkey, const int64_t *rpay, int64_t n, void *stream);
int hj_dev_count_i64(hj_ctx *ctx, const int64_t *skey, int64_t n, uint64_t *d_count, void *stream);
int hj_dev_probe_i64(hj_ctx *ctx, const int64_t *skey, const int64_t *spay, int64_t n,
                     int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream);
/* Same with rows as packed 16-B {key, payload} tuples (the exchange format). */
int hj_dev_build_tuples_i64(hj_ctx *ctx, const int64_t *tuples, int64_t n, void *stream);
int hj_dev_probe_tuples_i64(hj_ctx *ctx, const int64_t *tuples, int64_t n,
                            int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream);

/* Reference types: i32 keys, payload = row id (global thread index in
 * join_v1.mlir:255), (rowR, rowS) i32 output (join_v1.mlir:604-605).
 * row_base is added to row ids (0 for the reference). */
int hj_dev_build_i32(hj_ctx *ctx, const int32_t *rkey, int64_t n, int64_t row_base, void *stream);
int hj_dev_count_i32(hj_ctx *ctx, const int32_t *skey, int64_t n, uint64_t *d_count, void *stream);
int hj_dev_probe_i32(hj_ctx *ctx, const int32_t *skey, int64_t n, int64_t row_base,
                     int32_t *out_r, int32_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream);

/* Semi- and anti-join probes (EXISTS / NOT EXISTS) over the table an ordinary
 * hj_dev_build_* left: one build serves inner, semi and anti probes in any
 * order.  For the built relation R and the probe relation S,
 *   HJ_EXISTS_SEMI: the S rows j for which some i has R.key[i] == S.key[j];
 *   HJ_EXISTS_ANTI: the S rows for which no such i exists.
 * Every S row is in exactly one of the two results and at most once, however
 * often its key repeats in R; two S rows with equal keys are two rows.
 * INT64_MIN is a key like any other (it matches iff R holds an INT64_MIN
 * key).  R empty: semi is empty, anti is S.  S empty: both are empty.  Row
 * order is unspecified, as for the inner join.
 * out_s receives the S payload (i32: the row id row_base + row); out_key is
 * optional (NULL skips it), else it receives the S key at the same index, so
 * a semi-join's survivors can feed the next build or probe without a gather.
 * out_cap == 0 with both outputs NULL is the count-only form (spay may be
 * NULL then).  d_count = M, the exact number of qualifying rows, even when
 * M > out_cap: rows past out_cap are dropped and nothing is written at or
 * past index out_cap; bit 63 as above.
 * Errors as hj_dev_probe_*: HJ_ERR_ARG (null context, bad relation, bad
 * output, a kind other than the two), HJ_ERR_STATE (no build of that layout).
 * Asynchronous on the stream, kernels only once hj_ctx_reserve /
 * hj_ctx_reserve_probe sized the workspace (graph-capturable); the strategy
 * is chosen as for hj_dev_probe_* and hj_ctx_strategy_used, the probe timing
 * and hj_ctx_join_kernel (HJ_JOIN_KERNEL_EXISTS after a radix one) report the
 * call.  The built table, R's partition, the side list and the "build keys
 * repeat" flag are left untouched: an inner probe afterwards returns what it
 * returned before, and hj_ctx_build_has_duplicates keeps its answer. */
#define HJ_EXISTS_SEMI 0
#define HJ_EXISTS_ANTI 1
int hj_dev_exists_i64(hj_ctx *ctx, int kind, const int64_t *skey, const int64_t *spay, int64_t n, int64_t *out_key,
                      int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_exists_tuples_i64(hj_ctx *ctx, int kind, const int64_t *tuples, int64_t n, int64_t *out_key,
                             int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_exists_i32(hj_ctx *ctx, int kind, const int32_t *skey, int64_t n, int64_t row_base, int32_t *out_key,
                      int32_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream);

/* Positional lookup probe (the SINGLE and MARK joins of a query engine's
 * join-kind list; a dimension lookup, an id -> index mapping, Series.map) over
 * the table an ordinary hj_dev_build_* left: one result per probe row, at the
 * row's own position.  For the built relation R and the probe relation S of n
 * rows, with j the row's position in S as passed in,
 *   out_cnt[j] = the number of R rows i with R.key[i] == S.key[j];
 *   out_r[j]   = the smallest (signed) R payload among those rows, or
 *                null_pay (i32: null_row), written verbatim, when there is none.
 * i32 payloads are R's row ids (hj_dev_build_i32's row_base + row), so the
 * smallest is the first partner in R's order; "smallest" makes the result
 * deterministic and equal across strategies and kernels, and with a unique
 * build key it is simply the partner.  A caller that needs SINGLE-join
 * strictness checks out_cnt or hj_ctx_build_has_duplicates.
 * Every position 0 .. n-1 of each output that was passed is written exactly
 * once and nothing at or past n; there is no out_cap.  Either output may be
 * NULL (MARK only, or payload only); both NULL with n > 0 is HJ_ERR_ARG --
 * hj_dev_exists_*'s count-only form answers that.  d_count = the number of S
 * rows with at least one partner (the semi-join count), zeroed by the call;
 * bit 63 as above.
 * INT64_MIN is a key like any other: an INT64_MIN probe key counts R's
 * INT64_MIN rows and takes their smallest payload.  R empty: every row is
 * (null_pay, 0).  S empty: nothing is written, d_count = 0.
 * Errors in hj_dev_probe_outer_*'s order: a null context (HJ_ERR_ARG); no
 * build of that layout (HJ_ERR_STATE); a null count pointer, a bad relation,
 * both outputs null (HJ_ERR_ARG); a current build of more than INT32_MAX rows
 * (HJ_ERR_ARG: counts are int32); for i32, n > INT32_MAX (HJ_ERR_ARG).
 * Asynchronous on the stream, kernels and memsets only once hj_ctx_reserve /
 * hj_ctx_reserve_probe sized the workspace (graph-capturable).  The strategy
 * is chosen exactly as for hj_dev_probe_* (the AUTO dual build included) and
 * hj_ctx_strategy_used reports it; the probe timing works as for
 * hj_dev_exists_* (RADIX: [4] the partition of S, whose rows carry their
 * index through the passes, [5] the rest) and hj_ctx_join_kernel returns
 * HJ_JOIN_KERNEL_LOOKUP after a radix lookup.  The table, R's partition, the
 * side list, the "build keys repeat" flag and the full outer probes' mark
 * bitmap are left untouched: lookup, inner, semi, anti, outer, build and full
 * probes of one build may follow each other in any order and each returns
 * what it returned before.  Valid after hj_dev_build_routed_i64 too, over
 * unrouted rows, like hj_dev_exists_i64.
 * Cost: GLOBAL stores both columns in whole contiguous
 * runs; RADIX joins S in hash order, so each output column passed costs one
 * scattered store per row -- pass only the column that is needed.
 * There is no tuples form -- a packed S payload has no meaning where the
 * result is addressed by position -- and no routed bin-range form: a bin
 * range sees only part of S, so the positions of the rest would stay
 * unwritten. */
int hj_dev_lookup_i64(hj_ctx *ctx, const int64_t *skey, int64_t n, int64_t null_pay,
                      int64_t *out_r, int32_t *out_cnt, uint64_t *d_count, void *stream);
int hj_dev_lookup_i32(hj_ctx *ctx, const int32_t *skey, int64_t n, int32_t null_row,
                      int32_t *out_r, int32_t *out_cnt, uint64_t *d_count, void *stream);

/* As-of probe (pandas merge_asof(by=key, on=time), the ASOF JOIN of DuckDB,
 * ClickHouse and kdb+, "the last quote before each trade") over the table an
 * ordinary hj_dev_build_* left: per probe row, among the build rows with its
 * key, the one whose payload is the nearest at or before (or at or after) the
 * row's own bound.  For the built relation R and the probe relation S of n
 * rows, with j the row's position in S as passed in, let
 * P(j) = { R.pay[i] : R.key[i] == S.key[j] }; then
 *   HJ_ASOF_BACKWARD: out_r[j] = max { p in P(j) : p <= sbound[j] };
 *   HJ_ASOF_FORWARD:  out_r[j] = min { p in P(j) : p >= sbound[j] };
 *   | HJ_ASOF_STRICT: p < sbound[j]  /  p > sbound[j]  instead.
 * Payloads and bounds are compared as signed int64.  i32: the payload is R's
 * row id (hj_dev_build_i32's row_base + row), zero-extended, and the bound is
 * sign-extended -- "the last R row with this key at or before row b".
 * A row without a candidate gets null_pay (i32: null_row), written verbatim.
 * Validity comes from the set being empty, never from a sentinel: INT64_MIN and
 * INT64_MAX are payloads and bounds like any other, and the strict kinds are
 * true strict compares, not bound -+ 1 (strict backward with bound INT64_MIN
 * and strict forward with bound INT64_MAX have no candidate).
 * Every position 0 .. n-1 of out_r is written exactly once and nothing at or
 * past n; out_r is required when n > 0.  d_count = the number of S rows that
 * got a candidate, zeroed by the call; bit 63 as above (no as-of path sets it).
 * The result is a function of the data alone -- a max or a min of a set -- and
 * bit-equal across strategies, kernels and runs; repeated build keys need no
 * tie rule.  INT64_MIN is a key like any other, on both sides.  R empty: every
 * row is null_pay and d_count = 0.  S empty: nothing is written.
 * Errors in hj_dev_lookup_*'s order: a null context (HJ_ERR_ARG); a kind
 * outside {0, 1, 2, 3} (HJ_ERR_ARG); no build of that layout (HJ_ERR_STATE); a
 * null count pointer, a null skey or sbound with n > 0, a null out_r with
 * n > 0, n < 0 (HJ_ERR_ARG); for i32, n > INT32_MAX (HJ_ERR_ARG).
 * Asynchronous on the stream, kernels ONLY once hj_ctx_reserve /
 * hj_ctx_reserve_probe sized the workspace (the counter is zeroed by a kernel
 * on both strategies, not by a memset): capturable as a linear graph, a build
 * in front of the probe included.  The strategy is chosen exactly as for
 * hj_dev_probe_* (the AUTO dual build included) and hj_ctx_strategy_used
 * reports it; the probe timing works as for hj_dev_lookup_* (RADIX: [4] S's
 * one partition, whose rows carry their index through the passes, [5] the
 * rest) and hj_ctx_join_kernel returns HJ_JOIN_KERNEL_ASOF after a radix one.
 * Nothing the build left is written -- not the table, R's partition, the side
 * list, the "build keys repeat" flag or the mark bitmap: as-of, lookup, expand,
 * group, inner, semi, anti, outer, build and full probes of one build may
 * follow each other in any order and each returns what it returned before, and
 * hj_ctx_build_has_duplicates keeps its answer.  Valid after
 * hj_dev_build_routed_i64 too, over unrouted rows.
 * Cost: the lookup's, plus one read of the bound per row
 * -- contiguous beside the key on GLOBAL, scattered on RADIX, which joins S in
 * hash order.  Every copy of a build key sits in a slot of its own of one probe
 * chain that each probe of the key walks whole: fine at a handful of versions
 * per key, the expand probe's weak spot at thousands.
 * There is no tuples form and no routed bin-range form, for the reasons the
 * lookup gives. */
#define HJ_ASOF_BACKWARD 0   /* out_r[j] = max { p in P(j) : p <= sbound[j] } */
#define HJ_ASOF_FORWARD  1   /* out_r[j] = min { p in P(j) : p >= sbound[j] } */
#define HJ_ASOF_STRICT   2   /* flag, ORed into the kind: p < sbound[j]  /  p > sbound[j] */
int hj_dev_asof_i64(hj_ctx *ctx, int kind, const int64_t *skey, const int64_t *sbound, int64_t n, int64_t null_pay,
                    int64_t *out_r, uint64_t *d_count, void *stream);
int hj_dev_asof_i32(hj_ctx *ctx, int kind, const int32_t *skey, const int32_t *sbound, int64_t n, int32_t null_row,
                    int32_t *out_r, uint64_t *d_count, void *stream);

/* Expand probe (the join as a CSR: merge(how="inner" | "left") in the left
 * frame's order, a ragged id -> rows lookup, neighbour lists, an inverted
 * index, explode) over the table an ordinary hj_dev_build_* left: EVERY
 * partner of every probe row, at a place known from the row's position.  For
 * the built relation R and the probe relation S of n rows, with j the row's
 * position in S as passed in, let c(j) = the number of R rows i with
 * R.key[i] == S.key[j] and
 *   HJ_EXPAND_INNER: w(j) = c(j);
 *   HJ_EXPAND_OUTER: w(j) = max(1, c(j)) -- a row without a partner gets one
 *                    null entry.
 * out_off (required, n + 1 int64 words): out_off[j] = the sum of w(i) over
 * i < j, out_off[n] = M.  Exactly these n + 1 words are written; n == 0 writes
 * out_off[0] = 0.
 * out_r[out_off[j] .. out_off[j + 1]) holds the R payloads of row j's partners
 * (i32: R's row ids, hj_dev_build_i32's row_base + row), each partner exactly
 * once, a repeated build key one entry per copy; OUTER with c(j) == 0 gives
 * the single entry null_pay (i32: null_row), written verbatim.
 * The order INSIDE one segment is unspecified (compare after sorting within
 * segments); everything else is a function of the data alone and bit-equal
 * across strategies, kernels and runs -- with a build side that repeats no key
 * the whole of out_r is.
 * d_count = M exactly, even when M > out_cap: entries at positions >= out_cap
 * are dropped, nothing is written at or past out_cap, every position < out_cap
 * holds its defined value, and the offsets are always complete; bit 63 as
 * above (no expand path sets it).  out_cap == 0 with out_r NULL is the count
 * form (offsets and M only); out_cap > 0 with out_r NULL is HJ_ERR_ARG, and so
 * is out_cap == 0 with out_r non-NULL.
 * INT64_MIN is a key like any other, on both sides.  R empty: INNER gives
 * M = 0 and all offsets 0, OUTER n null entries with out_off[j] = j.
 * Errors in hj_dev_lookup_*'s order: a null context (HJ_ERR_ARG); a kind other
 * than the two (HJ_ERR_ARG); no build of that layout (HJ_ERR_STATE); a null
 * count pointer, a bad relation, a null out_off, bad outputs (HJ_ERR_ARG); a
 * current build of more than INT32_MAX rows (HJ_ERR_ARG: the per-row counts
 * are int32); for i32, n > INT32_MAX (HJ_ERR_ARG); HJ_ERR_NOMEM when the
 * workspace does not fit.  The workspace -- one int32 count per probe row and
 * one uint64 per 2048 of them -- lives in the context, grow-only, allocated by
 * the call or ahead by hj_ctx_reserve_expand.
 * Asynchronous on the stream, kernels ONLY once hj_ctx_reserve /
 * hj_ctx_reserve_probe / hj_ctx_reserve_expand sized the workspace (the
 * counter is written by a kernel, not by a memset): capturable as a linear
 * graph.  Three stages: the per-row counts (the lookup's kernels without their
 * payload column), a scan of them in three launches in which no workgroup
 * waits on another, and a fill that walks each row's partners again and stores
 * them at out_off[j] + k; RADIX partitions S ONCE and both stages share that
 * partition and its work map.  The strategy is chosen exactly as for
 * hj_dev_probe_* (the AUTO dual build included) and hj_ctx_strategy_used
 * reports it; the probe timing works as for hj_dev_lookup_* (RADIX: [4] S's
 * one partition, [5] everything after) and hj_ctx_join_kernel returns
 * HJ_JOIN_KERNEL_EXPAND after a radix expand.  Nothing the build left is
 * written -- not the table, R's partition, the side list, the "build keys
 * repeat" flag or the mark bitmap: expand, lookup, group, inner, semi, anti,
 * outer, build and full probes of one build may follow each other in any order
 * and each returns what it returned before.  Valid after
 * hj_dev_build_routed_i64 too, over unrouted rows.
 * Cost: a probe row with c partners issues its c stores
 * one after the other from one lane, and RADIX keeps every copy of a build key
 * in a slot of its own of one probe chain -- fine at PK-FK fan-out, far from
 * the grouped inner join's cooperative write path on a build side with ~100
 * copies per key.
 * There is no tuples form and no routed bin-range form, for the reasons the
 * lookup gives. */
#define HJ_EXPAND_INNER 0   /* w(j) = c(j) */
#define HJ_EXPAND_OUTER 1   /* w(j) = max(1, c(j)): a row without a partner gets one null entry */
int hj_dev_expand_i64(hj_ctx *ctx, int kind, const int64_t *skey, int64_t n, int64_t null_pay,
                      int64_t *out_off, int64_t *out_r, int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_expand_i32(hj_ctx *ctx, int kind, const int32_t *skey, int64_t n, int32_t null_row,
                      int64_t *out_off, int32_t *out_r, int64_t out_cap, uint64_t *d_count, void *stream);
/* Sizes the expand probe's count column and scan sums for probe sides of up to
 * max_probe_rows rows (key_bits 32 / 64), so that hj_dev_expand_* allocates
 * nothing. */
int hj_ctx_reserve_expand(hj_ctx *ctx, int64_t max_probe_rows, int key_bits);

/* Group probe (the group join of a query engine: join, then aggregate per
 * build row -- SELECT r.id, count(*), sum(s.v), min(s.v), max(s.v) ... GROUP
 * BY r.id, TPC-H Q13's shape, a segment reduction) over the table an ordinary
 * hj_dev_build_* left.  For the built relation R and the probe relation S with
 * a value column, let G(i) = {j : S.key[j] == R.key[i]}; then for R row i
 *   cnt(i) = |G(i)|,
 *   sum(i) = the sum of S.val[j] over G(i) in two's-complement int64 (it wraps),
 *   min(i) / max(i) = the signed extremes of S.val over G(i).
 * The result holds one row (R.pay[i], cnt, sum, min, max) per R row, every
 * column aligned at the same index:
 *   HJ_GROUP_MATCHED: only the R rows with cnt > 0;
 *   HJ_GROUP_ALL:     every R row; an empty group gives cnt = 0, sum = 0 and
 *                     min = max = null_val (i32: null_row) written verbatim.
 * Every copy of a repeated build key is a row of its own and carries the whole
 * group's aggregates (what join-then-group-by-R-row gives); two S rows with
 * equal keys are two contributions.  Row order is unspecified; the result is
 * otherwise a function of the data alone -- integer add, min and max commute --
 * and bit-equal across strategies, kernels and runs.  INT64_MIN is a key like
 * any other, INT64_MIN and INT64_MAX are values like any other: validity comes
 * from cnt, never from a sentinel.  R empty: M = 0.  S empty: MATCHED gives
 * M = 0, ALL every R row as an empty group.
 * i32: the S value is the row id row_base + row, as in every i32 entry point,
 * so out_min / out_max are the first and last partner's row and out_sum is an
 * int64 sum of row ids (defined, rarely wanted); n > INT32_MAX is HJ_ERR_ARG.
 * Any output column may be NULL and is then neither computed nor stored; sval
 * may be NULL when none of sum / min / max is asked for.  out_cap == 0 with all
 * five outputs NULL is the count-only form; out_cap > 0 with all five NULL is
 * HJ_ERR_ARG, and so is out_cap == 0 with any of them non-NULL.  d_count = M,
 * the exact number of result rows, even when M > out_cap: rows past out_cap
 * are dropped and nothing is written at or past index out_cap in any column;
 * bit 63 as above.
 * Errors in hj_dev_probe_full_*'s order: a null context (HJ_ERR_ARG); a kind
 * other than the two (HJ_ERR_ARG); no build of that layout (HJ_ERR_STATE); a
 * null count pointer, a bad relation, bad outputs (HJ_ERR_ARG).  GLOBAL keeps
 * per-slot accumulators beside the table (at most 32 B per slot, allocated by
 * the call, grow-only, or ahead by hj_ctx_reserve_group): HJ_ERR_NOMEM when
 * they do not fit.
 * Asynchronous on the stream, kernels (and the counter's one-word memset) only
 * once hj_ctx_reserve / hj_ctx_reserve_probe / hj_ctx_reserve_group sized the
 * workspace (graph-capturable).  The strategy is chosen exactly as for
 * hj_dev_probe_* (the AUTO dual build included) and hj_ctx_strategy_used
 * reports it; the probe timing works as for hj_dev_exists_* (RADIX: [4] S's
 * partition, [5] the rest) and hj_ctx_join_kernel returns HJ_JOIN_KERNEL_GROUP
 * after a radix one.  Nothing the build left is written -- not the table, R's
 * partition, the side list, the "build keys repeat" flag or the mark bitmap:
 * group, lookup, inner, semi, anti, outer, build and full probes of one build
 * may follow each other in any order and each returns what it returned before.
 * Valid after hj_dev_build_routed_i64 over unrouted rows, as
 * hj_dev_probe_full_i64 is; there is no routed bin-range form (a bin range
 * sees part of S). */
#define HJ_GROUP_MATCHED 0
#define HJ_GROUP_ALL 1
int hj_dev_group_i64(hj_ctx *ctx, int kind, const int64_t *skey, const int64_t *sval, int64_t n, int64_t null_val,
                     int64_t *out_r, int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                     int64_t out_cap, uint64_t *d_count, void *stream);
/* rows as packed 16-B {key, value} tuples */
int hj_dev_group_tuples_i64(hj_ctx *ctx, int kind, const int64_t *tuples, int64_t n, int64_t null_val,
                            int64_t *out_r, int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                            int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_group_i32(hj_ctx *ctx, int kind, const int32_t *skey, int64_t n, int64_t row_base, int32_t null_row,
                     int32_t *out_r, int32_t *out_cnt, int64_t *out_sum, int32_t *out_min, int32_t *out_max,
                     int64_t out_cap, uint64_t *d_count, void *stream);
/* Sizes the GLOBAL group probe's accumulators for builds of up to
 * max_build_rows rows of key_bits (32 / 64) keys, so that hj_dev_group_*
 * allocates nothing (a no-op where such a build would take the radix join). */
int hj_ctx_reserve_group(hj_ctx *ctx, int64_t max_build_rows, int key_bits);

/* Hash aggregate (GROUP BY key over ONE relation, and DISTINCT):
 *   SELECT key, count(*), sum(v), min(v), max(v) FROM S GROUP BY key
 * For the relation S with a value column, let G(k) = {j : S.key[j] == k}; the
 * result holds one row (key, cnt, sum, min, max) per DISTINCT key k of S, every
 * column aligned at the same index:
 *   cnt = |G(k)|,
 *   sum = the sum of S.val[j] over G(k) in two's-complement int64 (it wraps),
 *   min / max = the signed extremes of S.val over G(k).
 * M is the number of distinct keys.  Row order is unspecified; the result is
 * otherwise a function of the data alone -- integer add, min and max commute --
 * and bit-equal across strategies, kernels and runs.  INT64_MIN is a key like
 * any other (the wide table's empty word, and whatever word a layout uses as
 * "empty", never shows), INT64_MIN and INT64_MAX are values like any other;
 * i32 keys -1, INT32_MIN and 0 are ordinary keys.
 * i32: the value is the row id row_base + row, as in every i32 entry point, so
 * out_min / out_max are the key's first and last row, out_cnt its multiplicity
 * and out_sum an int64 sum of row ids; n > INT32_MAX (or row ids past it) is
 * HJ_ERR_ARG.
 * Any output column may be NULL and is then neither computed nor stored; val
 * may be NULL when none of sum / min / max is asked for (only the key column
 * is read then), and val == NULL with one of them passed is HJ_ERR_ARG (n == 0
 * reads nothing and takes a null column).  With
 * only out_key passed the call is DISTINCT.  out_cap == 0 with all five outputs
 * NULL is the count-only form (d_count = the number of distinct keys); out_cap
 * > 0 with all five NULL is HJ_ERR_ARG, and so is out_cap == 0 with any of them
 * non-NULL.  d_count = M exactly, even when M > out_cap: rows past out_cap are
 * dropped (which ones is unspecified) and nothing is written at or past index
 * out_cap in any column; bit 63 as above (no aggregate path sets it).  n == 0:
 * M = 0 and nothing is written.
 * Errors, in this order: a null context (HJ_ERR_ARG); a null count pointer, a
 * bad relation, bad outputs (HJ_ERR_ARG); HJ_ERR_NOMEM when the workspace does
 * not fit.
 * The call needs NO prior build.  It takes the context's workspace the way a
 * build does -- a new timing step, the host memo dropped -- and leaves NO build
 * behind: every hj_dev_probe_* / _count_* / _exists_* / _lookup_* / _group_*
 * after it returns HJ_ERR_STATE until the next hj_dev_build_*, and so does
 * hj_ctx_build_has_duplicates; a build and its probes after an aggregate work
 * exactly as on a fresh context.  Until that build hj_ctx_strategy_used,
 * hj_ctx_radix_plan and hj_ctx_table_capacity describe the aggregate, and
 * hj_ctx_join_kernel returns HJ_JOIN_KERNEL_AGGREGATE after a radix one, 0
 * after a global one.  Timing follows the probes: the whole call is the probe
 * phase ([2]); RADIX: [4] the input's partition, [5] the rest.
 * Strategy: hj_ctx_set_strategy and hj_ctx_set_radix_bits are honoured; AUTO
 * goes by n alone -- RADIX from 2^21 rows on, else GLOBAL (it does not know
 * the number of distinct keys).  GLOBAL: a table of >= 2n slots with per-slot
 * accumulators; each 2048-row tile is collapsed in LDS before it touches the
 * table, so a hot key costs one global atomic per tile.  RADIX: the input is
 * partitioned once (i32 rows one bit finer than a join's plan) and each
 * partition aggregated in one LDS table that persists over the partition's
 * rows; a partition with more distinct keys than the table admits is re-run
 * in sub-splits and is exact all the same.
 * Asynchronous on the stream: kernels only (the counter is zeroed by one of
 * them, not by a memset) -- no allocation, no synchronisation -- once
 * hj_ctx_reserve_aggregate sized the workspace (graph-capturable as a linear
 * graph). */
int hj_dev_aggregate_i64(hj_ctx *ctx, const int64_t *key, const int64_t *val, int64_t n,
                         int64_t *out_key, int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                         int64_t out_cap, uint64_t *d_count, void *stream);
/* rows as packed 16-B {key, value} tuples */
int hj_dev_aggregate_tuples_i64(hj_ctx *ctx, const int64_t *tuples, int64_t n,
                                int64_t *out_key, int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                                int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_aggregate_i32(hj_ctx *ctx, const int32_t *key, int64_t n, int64_t row_base,
                         int32_t *out_key, int32_t *out_cnt, int64_t *out_sum, int32_t *out_min, int32_t *out_max,
                         int64_t out_cap, uint64_t *d_count, void *stream);
/* Sizes the workspace for hj_dev_aggregate_* calls of up to max_rows rows of
 * key_bits (32 / 64) keys under the context's strategy and radix bits, every
 * column asked for, so that those calls allocate nothing.  AUTO: both the
 * radix workspace for max_rows and the global table for the inputs below 2^21
 * rows.  Where it has to replace the global table, a current build in that
 * table is dropped (probes answer HJ_ERR_STATE until the next build): reserve
 * before building, as with hj_ctx_reserve. */
int hj_ctx_reserve_aggregate(hj_ctx *ctx, int64_t max_rows, int key_bits);

/* Probe-side outer join (LEFT OUTER with the probe relation on the left) over
 * the table an ordinary hj_dev_build_* left: one build serves inner, semi,
 * anti and outer probes in any order.  For the built relation R and the probe
 * relation S the result is the multiset
 *   {(R.pay[i], S.pay[j]) : R.key[i] == S.key[j]}            (the inner join)
 *   u {(null_pay, S.pay[j]) : no i has R.key[i] == S.key[j]}  (the null rows),
 * so every S row appears at least once: M = sum over j of max(1, matches(j))
 * >= |S|, with equality iff no S row has two partners.  Row order is
 * unspecified; matched and null rows may interleave.
 * null_pay (i32: null_row, with row ids row_base + row as hj_dev_probe_i32's)
 * is written verbatim into out_r; the caller picks a value R's payloads (row
 * ids) do not take -- -1 is the natural one for row ids.
 * INT64_MIN is a key like any other: an INT64_MIN probe key pairs with every
 * INT64_MIN build row, or yields one null row if R holds none.  R empty:
 * every S row comes out as a null row.  S empty: M = 0.
 * d_count = the exact M even when M > out_cap: rows past out_cap are dropped
 * (which ones is unspecified) and nothing is written at or past index out_cap
 * in either output; bit 63 as above.  out_cap == 0 with both outputs NULL is
 * the count-only form (spay may be NULL then); with out_cap > 0 both outputs
 * are required.
 * Errors as hj_dev_probe_*: HJ_ERR_ARG (null context -- checked first --, bad
 * relation, bad output), HJ_ERR_STATE (no build of that layout).
 * Asynchronous on the stream, kernels only once hj_ctx_reserve /
 * hj_ctx_reserve_probe sized the workspace (graph-capturable).  The strategy
 * is chosen exactly as for hj_dev_probe_* (the AUTO dual build included) and
 * hj_ctx_strategy_used reports it.  The probe timing covers the whole call;
 * RADIX: [4] is the one partition of S, [5] everything after it (the join's
 * kernels, then the unmatched-rows stage over the same partition), and
 * hj_ctx_join_kernel reports the kernel that produced the pairs, as after
 * hj_dev_probe_*.  The built table, R's partition and the side list are left
 * untouched and hj_ctx_build_has_duplicates answers what it would after
 * hj_dev_probe_* of the same S: inner, semi, anti and outer probes of one
 * build may follow each other in any order and each returns what it returned
 * before.  Valid after hj_dev_build_routed_i64 too, over unrouted rows, like
 * hj_dev_probe_i64. */
int hj_dev_probe_outer_i64(hj_ctx *ctx, const int64_t *skey, const int64_t *spay, int64_t n, int64_t null_pay,
                           int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_probe_outer_tuples_i64(hj_ctx *ctx, const int64_t *tuples, int64_t n, int64_t null_pay,
                                  int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_probe_outer_i32(hj_ctx *ctx, const int32_t *skey, int64_t n, int64_t row_base, int32_t null_row,
                           int32_t *out_r, int32_t *out_s, int64_t out_cap, uint64_t *d_count, void *stream);

/* Build-side and full outer join (RIGHT OUTER / FULL OUTER with the probe
 * relation S on the left) over the table an ordinary hj_dev_build_* left: the
 * kinds that keep the BUILD relation's rows, so the smaller relation can stay
 * the build side and a full outer join needs one build.  The result is the
 * multiset
 *   {(R.pay[i], S.pay[j]) : R.key[i] == S.key[j]}            (the inner join)
 *   u {(R.pay[i], null_s) : no j has S.key[j] == R.key[i]}    (R's null rows)
 *   u {(null_r, S.pay[j]) : no i has R.key[i] == S.key[j]}    (S's null rows, HJ_OUTER_FULL only);
 * M is the sum of the three sizes.  Row order is unspecified and the three
 * kinds of rows may interleave.  null_r and null_s (i32: null_row_r,
 * null_row_s; row ids as hj_dev_probe_i32's) are written verbatim; null_r is
 * ignored for HJ_OUTER_BUILD.
 * "Without a partner" refers to the S of THIS call: nothing carries over
 * between calls.  Each unmatched R row comes out once; every copy of a
 * repeated build key is a row of its own, and all copies of a key that some
 * S row holds are matched.  INT64_MIN is a key like any other: INT64_MIN
 * build rows are unmatched iff S holds no INT64_MIN key, and (FULL) INT64_MIN
 * probe rows are null rows iff R holds none.  R empty: BUILD gives M = 0,
 * FULL every S row as a null row.  S empty: every R row as (pay, null_s).
 * d_count = the exact M even when M > out_cap: rows past out_cap are dropped
 * (which ones is unspecified) and nothing is written at or past index out_cap
 * in either output; bit 63 as above.  out_cap == 0 with both outputs NULL is
 * the count-only form (spay may be NULL then).
 * Errors in hj_dev_probe_outer_*'s order: a null context first, then a kind
 * other than the two (both HJ_ERR_ARG); no build of that layout
 * (HJ_ERR_STATE); a null count pointer, a bad relation, bad outputs
 * (HJ_ERR_ARG).
 * Asynchronous on the stream, kernels and memsets only once hj_ctx_reserve /
 * hj_ctx_reserve_probe sized the workspace (graph-capturable).  The strategy
 * is chosen exactly as for hj_dev_probe_* (the AUTO dual build included) and
 * hj_ctx_strategy_used reports it.  The probe timing covers the whole call;
 * RADIX: [4] is the one partition of S, [5] everything after it;
 * hj_ctx_join_kernel reports the kernel that produced the pairs.  GLOBAL: a
 * mark bitmap (one bit per slot, allocated with the table) is cleared, set
 * where the probe finds its matches and scanned inside the call.  The table, R's partition, the side
 * list and the "build keys repeat" flag are left as hj_dev_probe_* of the
 * same S leaves them: inner, semi, anti, outer, build and full probes of one
 * build may follow each other in any order, each returns what it returned
 * before, and hj_ctx_build_has_duplicates keeps its answer.
 * Valid after hj_dev_build_routed_i64 too, over unrouted rows.  Routed
 * bin-range probes (hj_dev_probe_routed_i64) have no full form: an R row's
 * partner may lie in a bin that has not arrived. */
#define HJ_OUTER_BUILD 1 /* inner pairs + R rows without a partner (RIGHT OUTER, S on the left) */
#define HJ_OUTER_FULL 2  /* inner pairs + S rows without a partner + R rows without a partner */
int hj_dev_probe_full_i64(hj_ctx *ctx, int kind, const int64_t *skey, const int64_t *spay, int64_t n, int64_t null_r,
                          int64_t null_s, int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count,
                          void *stream);
int hj_dev_probe_full_tuples_i64(hj_ctx *ctx, int kind, const int64_t *tuples, int64_t n, int64_t null_r,
                                 int64_t null_s, int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count,
                                 void *stream);
int hj_dev_probe_full_i32(hj_ctx *ctx, int kind, const int32_t *skey, int64_t n, int64_t row_base, int32_t null_row_r,
                          int32_t null_row_s, int32_t *out_r, int32_t *out_s, int64_t out_cap, uint64_t *d_count,
                          void *stream);

/* ---------------------------------------------------------- Composite keys
 * Exact range packing of up to four key columns into ONE int64 key, so that
 * `ON a.x = b.x AND a.y = b.y` and `GROUP BY a, b` run through every entry
 * point above unchanged.  A key codec is an object of its own, independent of
 * hj_ctx; it owns one small device block (a few hundred bytes) holding the
 * plan.  Columns are signed int32 or int64 (col_bits[c] = 32 | 64), ncols is
 * 1 .. HJ_KEYS_MAX_COLS.
 *
 * Call order: reset -> observe (once per relation that will be packed) ->
 * seal -> pack / unpack.  A freshly created codec is in the reset state.
 *   reset    forgets every observation, the seal and the out-of-range count (a
 *            kernel, not a memset).
 *   observe  folds the n rows of the given columns into the per-column signed
 *            minimum lo[c] and maximum hi[c] (int32 columns sign-extended) and
 *            adds n to rows_observed.  Any number of calls; n == 0 reads
 *            nothing and accepts null column pointers (and a null cols).
 *   seal     one tiny kernel computes the plan on the device:
 *              span    = (uint64)hi[c] - (uint64)lo[c]
 *              bits[c] = 0 if span == 0, else 64 - clz(span)
 *              shift[c] = bits[c+1] + ... + bits[ncols-1]   (column 0 is the highest field)
 *              total   = the sum of bits[c]; total > 64 sets the range flag.
 *            With no row observed at all every width is 0 and lo = hi = 0.
 *            Sealing a sealed codec recomputes the same plan.
 *   pack     key = OR over the columns with bits[c] > 0 of
 *                  ((uint64)(v[c] - lo[c]) << shift[c]).
 *            A 0-bit column contributes nothing and is never shifted: the pair
 *            (constant, full-range int64) gives bits = {0, 64}, shift = {64, 0},
 *            and two full-range int32 columns give bits = {32, 32}; both total
 *            exactly 64 and both are legal.
 *              - pack is injective on the observed box [lo, hi];
 *              - the UNSIGNED order of the packed keys equals the lexicographic
 *                order of the column tuples;
 *              - any 64-bit pattern can occur, the INT64_MIN word included --
 *                the joins and the aggregate treat that word as an ordinary key.
 *            Exactly n words are written (pack_tuples: 2n, the 16-B rows
 *            {key, pay[row]} of the hj_dev_*_tuples_i64 entry points) and
 *            nothing past them.
 *   unpack   the exact inverse on the observed box: out_cols[c][row] =
 *            lo[c] + ((key >> shift[c]) & (2^bits[c] - 1)), int32 columns
 *            written as int32; a NULL entry of out_cols is skipped.
 * Values outside the sealed range (a relation that was not observed is
 * packed): a row with some v[c] outside [lo[c], hi[c]] is counted in
 * rows_out_of_range and its key is unspecified; the call stays memory-safe
 * and every other row's key is exact.
 * Range flag set (total > 64): pack and unpack launch and write nothing (they
 * read the flag on the device), and hj_keycodec_info returns HJ_ERR_RANGE with
 * the widths filled in, so the caller sees which column is to blame.  The
 * joint range is never joined approximately; there is no hash-and-verify
 * fallback.
 * Errors, in this order: a null codec; a bad column set (null cols, or a null
 * column with n > 0), a null output, n < 0 -- each HJ_ERR_ARG with the message
 * in hj_last_error; then the call order, tracked on the host (it is call
 * order, not data): observe after a seal and before a reset, and pack or
 * unpack before a seal, are HJ_ERR_STATE.  hj_keycodec_create checks ncols and
 * col_bits BEFORE it touches a device and returns NULL with a message.
 * Every hj_dev_keycodec_* call is asynchronous on the stream (NULL = default
 * stream), launches kernels only, allocates nothing and never synchronises.
 * Column pointers travel by value in the kernel arguments; the plan is read
 * from the device block.  The sequence reset, observe, observe, seal, pack,
 * pack is capturable as a LINEAR graph and, replayed over new data in the
 * same buffers, yields the new data's plan and keys.
 * hj_keycodec_info synchronises the device and reads the sealed plan back
 * (HJ_ERR_STATE before a seal): the sum of the widths, per column the width
 * and the observed [lo, hi], the rows observed and the rows packed out of
 * range since the reset; entries past ncols are 0; any pointer may be NULL. */
#define HJ_KEYS_MAX_COLS 4
typedef struct hj_keycodec hj_keycodec;
hj_keycodec *hj_keycodec_create(int device, int ncols, const int col_bits[]);
void hj_keycodec_destroy(hj_keycodec *kc);
int hj_dev_keycodec_reset(hj_keycodec *kc, void *stream);
int hj_dev_keycodec_observe(hj_keycodec *kc, const void *const cols[], int64_t n, void *stream);
int hj_dev_keycodec_seal(hj_keycodec *kc, void *stream);
int hj_dev_keycodec_pack(hj_keycodec *kc, const void *const cols[], int64_t n, int64_t *out_key, void *stream);
int hj_dev_keycodec_pack_tuples(hj_keycodec *kc, const void *const cols[], const int64_t *pay, int64_t n,
                                int64_t *out_tuples, void *stream);
int hj_dev_keycodec_unpack(hj_keycodec *kc, const int64_t *key, int64_t n, void *const out_cols[], void *stream);
int hj_keycodec_info(hj_keycodec *kc, int *total_bits, int bits[4], int64_t lo[4], int64_t hi[4],
                     uint64_t *rows_observed, uint64_t *rows_out_of_range);

/* --------------------------------------------------------------- Key filter
 * A runtime filter of a build side's keys, applied to a probe side BEFORE the
 * expensive step (the radix passes, the multi-GPU shuffle): a split-block
 * Bloom filter with no false negatives.  An object of its own, independent of
 * hj_ctx.  Nothing in the library turns it on by itself.
 *
 * Format (fixed: the device equals a host model bit for bit).  nblocks blocks
 * of 32 bytes, each 8 uint32 words; a key sets / tests ONE bit in each word of
 * ONE block.  For a key k (int32 keys are sign-extended to int64 first, so an
 * i32 filter and an i64 filter of the same values are the same filter):
 *     h     = fmix64((uint64)k ^ 0x9E3779B97F4A7C15)    (MurmurHash3's finalizer)
 *     hi    = h >> 32;  lo = (uint32)h
 *     block = (hi * (uint64)nblocks) >> 32               (1 <= nblocks < 2^31)
 *     SALT  = {0x47b6137b, 0x44974d91, 0x8824ad5b, 0xa2b7289d,
 *              0x705495c7, 0x2df1424b, 0x9efc4947, 0x5c6bfb31}
 *     mask[w] = 1u << ((uint32)(lo * SALT[w]) >> 27)     (w = 0..7, 32-bit wrapping multiply)
 * Insert ORs mask[w] into word w of the block; a key passes iff all eight
 * bits are set.  The xor constant keeps the block index independent of
 * hj_partition_of (fmix64(k)'s top word): one owner's keys still spread over
 * the whole filter.  hj_filter_place is this function on the host.
 * Sizing: hj_filter_blocks_for(n_keys, bits_per_key) = max(1, ceil(n_keys *
 * bits_per_key / 256)), bits_per_key in 4..64 (< 0 on bad arguments or past
 * 2^31 - 1 blocks).  False positives at 8 / 12 / 16 / 24 bits per key: about
 * 3.3 % / 0.55 % / 0.13 % / 0.016 %.
 *
 * Guarantees:
 *   - the filter's words are a function of nblocks and the SET of inserted
 *     keys alone: order, repeats, the number of insert calls and the form
 *     (columns, tuples, i32) do not matter;
 *   - a key that was inserted, or merged in, always passes;
 *   - INT64_MIN is an ordinary key;
 *   - a cleared filter passes nothing.
 *
 * hj_filter_create: d_words == NULL -- the filter allocates and owns nblocks *
 * 32 bytes, contents undefined until the first clear; d_words != NULL -- the
 * caller's device buffer of that size, 32-byte aligned, is used in place and
 * never freed (so a caller can all-reduce the words with bitwise OR as a
 * tensor).  nblocks outside [1, 2^31) or a misaligned buffer is checked before
 * any device is touched: NULL with a message in hj_last_error.
 * hj_filter_words returns the words' device pointer and nblocks.
 * clear  zeroes the words (a kernel, not a memset).
 * insert ORs the keys of an int64 column, of 16-byte {key, pay} tuples or of
 *        an int32 column in.  n == 0 reads nothing and accepts a null pointer.
 * merge  f |= other; both filters must have the same nblocks and device.
 * apply  compacts the qualifying rows IN INPUT ORDER: kind HJ_FILTER_PASS the
 *        rows whose key passes (they may have a partner), HJ_FILTER_REJECT the
 *        rows whose key fails (they certainly have none).  Every output is
 *        optional: out_key / out_pay (out_tuples) receive the rows, out_row the
 *        source position -- for i32 the row id row_base + row, so the survivors
 *        of an i32 probe can be mapped back.  spay may be NULL when out_pay is.
 *        *d_count = M, the number of qualifying rows, exactly, even when M >
 *        out_cap; nothing is written at or past out_cap.  out_cap == 0 with
 *        every output NULL is the count form; out_cap > 0 with every output
 *        NULL, or out_cap == 0 with an output, is HJ_ERR_ARG.  The counter is
 *        written by a kernel; n == 0 writes nothing else and gives 0.
 * Errors, in this order: a null filter (HJ_ERR_ARG, "null filter"); a kind
 * other than the two; a null count pointer, a bad relation (null keys with n >
 * 0, a null spay with out_pay, i32 row ids past 2^31 - 1), bad outputs, n < 0;
 * for merge a geometry mismatch; HJ_ERR_NOMEM when apply's workspace (tile
 * counts, scan sums, one bit per row) does not fit.
 * Every hj_dev_filter_* call is asynchronous on the stream (NULL = default
 * stream).  hj_filter_reserve sizes apply's workspace for max_rows rows
 * (grow-only); after it the calls launch kernels only -- no allocation, no
 * synchronisation -- and clear, insert, insert, apply capture as a LINEAR
 * graph that, replayed, follows new data in the same buffers.  An apply of
 * more rows than reserved grows the workspace first (it waits for the device
 * and cannot be captured). */
#define HJ_FILTER_PASS 0   /* the rows whose key passes (may have a partner) */
#define HJ_FILTER_REJECT 1 /* the rows whose key fails (certainly have none) */
typedef struct hj_filter hj_filter;
int64_t hj_filter_blocks_for(int64_t n_keys, int bits_per_key);
int hj_filter_place(int64_t key, int64_t nblocks, int64_t *block, uint32_t mask[8]);
hj_filter *hj_filter_create(int device, int64_t nblocks, void *d_words);
void hj_filter_destroy(hj_filter *f);
int hj_filter_words(hj_filter *f, void **d_words, int64_t *nblocks);
int hj_filter_reserve(hj_filter *f, int64_t max_rows);
int hj_dev_filter_clear(hj_filter *f, void *stream);
int hj_dev_filter_insert_i64(hj_filter *f, const int64_t *key, int64_t n, void *stream);
int hj_dev_filter_insert_tuples_i64(hj_filter *f, const int64_t *tuples, int64_t n, void *stream);
int hj_dev_filter_insert_i32(hj_filter *f, const int32_t *key, int64_t n, void *stream);
int hj_dev_filter_merge(hj_filter *f, const hj_filter *other, void *stream);
int hj_dev_filter_apply_i64(hj_filter *f, int kind, const int64_t *skey, const int64_t *spay, int64_t n,
                            int64_t *out_key, int64_t *out_pay, int64_t *out_row, int64_t out_cap, uint64_t *d_count,
                            void *stream);
int hj_dev_filter_apply_tuples_i64(hj_filter *f, int kind, const int64_t *tuples, int64_t n, int64_t *out_tuples,
                                   int64_t *out_row, int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_filter_apply_i32(hj_filter *f, int kind, const int32_t *skey, int64_t n, int64_t row_base,
                            int32_t *out_key, int32_t *out_row, int64_t out_cap, uint64_t *d_count, void *stream);

/* --------------------------------------------------------------- Star probe
 * One pass of n probe rows (a fact table) over 1..HJ_STAR_MAX_DIMS built
 * relations (its dimensions): per dimension d a key column skeys[d] of the
 * probe rows and a context dims[d] holding an ordinary build in its GLOBAL
 * table.  The rows that qualify under EVERY dimension are returned in input
 * order with each dimension's payload beside them.  The key columns are read
 * once for the decision, the tables are walked in one kernel, and only the M
 * surviving rows are written.  An object of its own, like hj_filter: it owns
 * the compaction workspace and only reads the contexts.
 *
 * For dimension d let R_d be the relation built in dims[d], c_d(j) the number
 * of R_d rows whose key equals skeys[d][j] and p_d(j) the smallest signed
 * payload among them (i32: the smallest row id) -- exactly hj_dev_lookup_*'s
 * out_cnt and out_r.  Kinds, per dimension:
 *   HJ_STAR_INNER  row j needs c_d(j) > 0.  With out_pay[d] == NULL this is
 *                  the semi-join form.
 *   HJ_STAR_LEFT   row j always stays; its payload is p_d(j), or null_pay[d]
 *                  written verbatim when c_d(j) == 0.
 *   HJ_STAR_ANTI   row j needs c_d(j) == 0.  It has no payload column: a
 *                  non-null out_pay[d] is HJ_ERR_ARG.
 * Row j qualifies iff every dimension admits it.  With o the number of
 * qualifying rows before j:
 *     out_row[o]    = j                        (i32: row_base + j)
 *     out_pay[d][o] = p_d(j), or null_pay[d] when c_d(j) == 0
 *     *d_count      = M, the number of qualifying rows, exactly, even when M >
 *                     out_cap.
 * Nothing is written at or past out_cap in any column, and every position
 * below min(M, out_cap) holds its defined value.  Every output is optional
 * (out_pay itself may be NULL: no payload column).  out_cap == 0 with every
 * output NULL is the count form; out_cap > 0 with every output NULL, or
 * out_cap == 0 with any output, is HJ_ERR_ARG.
 * The result is a function of the data alone: bit-equal across runs and
 * across the table placements below.
 *   - INT64_MIN is a key like any other on both sides (the wide layout answers
 *     it from the side list, as the lookup does).
 *   - An empty R_d: INNER gives M = 0, LEFT all nulls, ANTI admits every row.
 *   - n == 0 writes nothing but the counter.
 *   - The same context may appear in two dimensions.
 * The contexts are only read: the table, the side list, the mark bitmap, the
 * state words, the strategy of the last probe, the timing sets and the "build
 * keys repeat" flag are left untouched, and every other probe of those builds
 * returns afterwards what it returned before.
 *
 * dims, kinds, skeys, null_pay (null_row) and out_pay are HOST arrays of ndims
 * entries read at call time; their values travel in the kernel arguments.  All
 * dimensions of one call share a layout: int64 builds for hj_dev_star_i64,
 * hj_dev_build_i32 builds for hj_dev_star_i32.
 * The dimensions are walked in the caller's order and a row that one of them
 * dropped is looked up in no further one: put the most selective first.
 * There is no radix form: it would have to partition the probe rows once per
 * key column.  A radix-only build (HJ_STRATEGY_RADIX, or AUTO from 2^21 rows)
 * is HJ_ERR_STATE; AUTO's dual build (2^18..2^21 rows) is valid, its global
 * table exists.
 *
 * Errors, in this order: a null star (HJ_ERR_ARG, "null star", before any
 * device is touched); ndims outside 1..HJ_STAR_MAX_DIMS or a null dims, kinds,
 * skeys or null-value array (HJ_ERR_ARG); per dimension in index order a null
 * context, a kind outside the three, a context of another device (HJ_ERR_ARG),
 * no build of that layout, a build with no global table (HJ_ERR_STATE, the
 * message names the dimension); a null count pointer; n < 0 or a null key
 * column with n > 0; bad outputs as above; for i32 row ids past 2^31 - 1 (all
 * HJ_ERR_ARG); HJ_ERR_NOMEM when the workspace does not fit.
 *
 * Launches.  Asynchronous on the stream (NULL = default stream).  Two kernels
 * around a scan: the decision launch leaves one result byte per lane and a
 * count per 2048-row tile, exclusive_scan turns the counts into offsets, the
 * write launch stores the survivors (the count form stores the counter alone).
 * When no dimension can drop a row (every kind LEFT) a row's position is its
 * index: ONE probe launch stores everything positionally, clipped at out_cap,
 * and M = n.  The probe launch (the decision, or the keep-all launch) sees
 * every row: the tables it walks go to LDS in ascending size while their sum
 * stays <= 128 KiB and each is <= 64 KiB, and the others are read from global
 * memory in the same kernel; the plan is a function of the tables' capacities
 * at call time.  The write launch sees the survivors alone and reads every
 * table from global memory.
 * hj_star_reserve sizes the workspace for max_rows probe rows (grow-only);
 * after it the calls launch kernels only -- the counter is written by a
 * kernel, never a memset -- and the dimensions' builds followed by the star
 * probe capture as a LINEAR graph that, replayed, follows new data in the same
 * buffers.  A call of more rows than reserved grows the workspace first (it
 * waits for the device and cannot be captured).
 * hj_star_last_plan: host facts of the last hj_dev_star_* call, no
 * synchronisation: the kernel launches, the grid of the probe launch (the
 * decision, or the keep-all launch), its tiles, bit d of lds_dims set =
 * dimension d's table was probed from LDS, the LDS bytes of those tables. */
#define HJ_STAR_MAX_DIMS 4
#define HJ_STAR_INNER 0 /* the row needs a partner in this dimension */
#define HJ_STAR_LEFT 1  /* the row stays; null_pay[d] where it has none */
#define HJ_STAR_ANTI 2  /* the row needs to have no partner; no payload column */
typedef struct hj_star hj_star;
hj_star *hj_star_create(int device);
void hj_star_destroy(hj_star *s);
int hj_star_reserve(hj_star *s, int64_t max_rows);
int hj_star_last_plan(const hj_star *s, int *launches, int *grid, int64_t *tiles, int *lds_dims, int64_t *lds_bytes);
int hj_dev_star_i64(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[], const int64_t *const skeys[],
                    const int64_t null_pay[], int64_t n, int64_t *const out_pay[], int64_t *out_row,
                    int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_star_i32(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[], const int32_t *const skeys[],
                    const int32_t null_row[], int64_t n, int64_t row_base, int32_t *const out_pay[], int32_t *out_row,
                    int64_t out_cap, uint64_t *d_count, void *stream);

/* ------------------------------------------------------------ Star aggregate
 * GROUP BY over a star probe's qualifying rows in ONE pass of the fact table:
 * the rows every dimension admits are grouped by dimension payloads and one
 * fact column is aggregated per group.  No per-row result reaches memory: the
 * key columns are read once, the value column for the qualifying rows only,
 * and the group table is all that is written.
 *
 * dims, kinds, skeys, the null array, c_d(j), p_d(j), the three kinds, which
 * rows qualify, INT64_MIN keys, empty builds, the same context passed twice,
 * radix-only builds (HJ_ERR_STATE) and the contexts being only read: all as
 * "Star probe" above.
 *
 * Group key.  Let P_d(j) be p_d(j) when c_d(j) > 0, else (LEFT only) the
 * dimension's null value; i32: both sign-extended to int64.  A qualifying row
 * j has the group key
 *     g(j) = sum over the dimensions with gshift[d] >= 0 of
 *            ((uint64)(P_d(j) - gbase[d]) << gshift[d])          (mod 2^64)
 * gshift[d] is -1 (the dimension takes no part in the key) or 0..63; gbase ==
 * NULL means all zeros.  This is the composite keys' pack formula with lo =
 * gbase and shift = gshift: a sealed codec over the grouped payload columns
 * supplies both arrays and its unpack turns out_key back into the columns.
 * The arithmetic wraps, so g is defined for every input; keeping the fields
 * apart is the caller's business.  With every gshift at -1 all qualifying rows
 * form one group with key 0.  With no qualifying row there is no group (M =
 * 0): GROUP BY semantics, not a scalar aggregate's one row.
 *
 * Result.  One row (key, cnt, sum, min, max) per distinct g over the
 * qualifying rows, every column int64 in both forms: exactly what
 * hj_dev_aggregate_i64 returns over the columns (g(j), sval[j]) of the
 * qualifying rows.  sum wraps, min / max are signed extremes, i32 sval is
 * sign-extended; INT64_MIN and INT64_MAX are values like any other, and a
 * group key that comes out as the INT64_MIN word is a key like any other.  Row
 * order is unspecified; the rest is a function of the data alone, bit-equal
 * across runs and table placements.
 * Any output may be NULL and is then neither computed nor stored.  sval may be
 * NULL when none of sum / min / max is passed; sval == NULL with one of them is
 * HJ_ERR_ARG.  n == 0 takes null columns.  out_cap == 0 with all five outputs
 * NULL is the count form; out_cap > 0 with all five NULL, or out_cap == 0 with
 * any of them, is HJ_ERR_ARG.  *d_count = G, the number of distinct groups,
 * exactly, even when G > out_cap; nothing is written at or past out_cap.
 *
 * Group table.  The star object owns it: a wide (int64-key) table with the
 * group probe's accumulators beside it, for both forms.
 * hj_star_reserve_groups sizes it (grow-only) to the smallest power of two >=
 * max(2 * max_groups, 2048) slots; hj_star_group_capacity returns that (0
 * before the first reserve).  A call before any reserve is HJ_ERR_STATE.
 * G <= max_groups never overflows.  G > max_groups gives either the exact
 * result or bit 63 of *d_count with the result invalid (nothing is stored) --
 * never a wrong result without the bit, and never an unbounded walk: the
 * insert-or-find is a counted loop of at most `capacity` steps, and the flag it
 * sets is read at the start of every tile and ends the pass.
 *
 * Errors, in this order: a null star (HJ_ERR_ARG, "null star", before any
 * device is touched); ndims outside 1..HJ_STAR_MAX_DIMS or a null dims, kinds,
 * skeys, null-value array or gshift (HJ_ERR_ARG); per dimension in index order
 * a null context, a kind outside the three, a context of another device, a
 * gshift outside -1..63, an ANTI dimension with gshift >= 0 (it has no
 * payload) (all HJ_ERR_ARG), then no build of that layout, or no global table
 * (HJ_ERR_STATE naming the dimension); no group reserve (HJ_ERR_STATE); a null
 * count pointer; n < 0 or a null key column with n > 0; the sval rule; the
 * output rules (HJ_ERR_ARG); HJ_ERR_NOMEM (hj_star_reserve_groups).
 *
 * Launches.  Asynchronous on the stream and, after hj_star_reserve_groups,
 * kernels only -- no memset, no allocation, no synchronisation: the group
 * table's fill, the accumulators' fill (it zeroes the counter), one pass over
 * the fact rows (n > 0) and the emit.  The dimensions' builds followed by this
 * call capture as a LINEAR graph that, replayed, follows new data in the same
 * buffers.  There is no per-row workspace: hj_star_reserve is not needed.
 * The pass walks the dimensions that can drop a row (INNER, ANTI) in the
 * caller's order -- a grouped one once, for its smallest payload -- then, for
 * the surviving rows alone, the grouped LEFT ones; a LEFT dimension with
 * gshift -1 is never read.  The tables it walks go to LDS in ascending size
 * as the star probe's do, into what a CU's 160 KiB leave beside the kernel's
 * own 18 KiB collapse table and into no more than 128 KiB.
 * hj_star_last_plan reports this call like a star probe: the launches, the
 * pass's grid and tiles, the LDS-resident dimensions and their bytes. */
int hj_star_reserve_groups(hj_star *s, int64_t max_groups);
int64_t hj_star_group_capacity(const hj_star *s);
int hj_dev_star_aggregate_i64(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[],
                              const int64_t *const skeys[], const int64_t null_pay[], const int gshift[],
                              const int64_t gbase[], const int64_t *sval, int64_t n, int64_t *out_key, int64_t *out_cnt,
                              int64_t *out_sum, int64_t *out_min, int64_t *out_max, int64_t out_cap, uint64_t *d_count,
                              void *stream);
int hj_dev_star_aggregate_i32(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[],
                              const int32_t *const skeys[], const int32_t null_row[], const int gshift[],
                              const int64_t gbase[], const int32_t *sval, int64_t n, int64_t *out_key, int64_t *out_cnt,
                              int64_t *out_sum, int64_t *out_min, int64_t *out_max, int64_t out_cap, uint64_t *d_count,
                              void *stream);

/* ---------------------------------------------------------------- Star query
 * The star aggregate with the fact row's own part of a star-schema query in
 * the same pass: predicates on fact columns, a value that is an expression of
 * two fact columns, and group fields taken from fact columns.  Nothing is
 * written per row and no column is read for a row that already failed.
 *
 * hj_star_fact is a HOST struct read at call time; its values travel in the
 * kernel arguments as dims / kinds / gshift do.  Every fact column of a call
 * (pcol, vb, fcol, as sval and skeys) has the call's layout: int64 for _i64,
 * int32 for _i32.  Columns may alias each other, sval or a key column: all are
 * only read.  The arguments are hj_dev_star_aggregate_*'s with `fact` after
 * gbase.
 *
 * Which rows qualify.  Row j qualifies iff every predicate admits it AND every
 * dimension admits it (the star aggregate's rule, unchanged).  Predicate p
 * admits row j iff plo[p] <= pcol[p][j] <= phi[p] under HJ_PRED_IN, iff
 * pcol[p][j] < plo[p] or pcol[p][j] > phi[p] under HJ_PRED_OUT.  The compares
 * are SIGNED int64 compares; int32 column values are sign-extended first.  plo
 * / phi are int64 in both forms: bounds outside int32 are legal and mean
 * "always" or "never".  plo = INT64_MIN, phi = INT64_MAX admits every row
 * under IN and none under OUT; plo > phi is an empty range: no row under IN,
 * every row under OUT.  INT64_MIN and INT64_MAX are column values like any
 * other.
 *
 * The value.  v(j) = sval[j] <vop> vb[j] in two's-complement int64: it wraps,
 * MUL is the low 64 bits.  int32 columns are sign-extended first, so i32 MUL /
 * ADD / SUB never wrap.  sum / min / max are over v.  vb is read only when vop
 * != HJ_VALUE_A and one of sum / min / max is asked for, and only for
 * qualifying rows.
 *
 * The group key.  The star aggregate's g(j) plus, for each f < nfact,
 *     ((uint64)(fcol[f][j] - fbase[f]) << fshift[f])             (mod 2^64)
 * fshift is 0..63; a fact group that takes no part is simply not listed.
 * Keeping the fields apart is the caller's business, as for gshift.  fcol is
 * read for qualifying rows only.
 *
 * The result is exactly what hj_dev_star_aggregate_i64 returns over the
 * qualifying rows with that value and that key.  Carried over unchanged: the
 * output rules and the count form, *d_count and its bit 63 on group-table
 * overflow, hj_star_reserve_groups, the contexts being only read, bit-equality
 * across runs and placements, and the launches being kernels only, a linear
 * graph under capture (bounds, shifts and bases travel in the captured
 * arguments).
 *
 * fact == NULL is no predicate, HJ_VALUE_A and no fact group: the call then
 * equals hj_dev_star_aggregate_* bit for bit (it runs the same kernel).
 *
 * ndims == 0 is legal here (and only here: hj_dev_star_aggregate_* keeps its
 * 1..4); dims, kinds, skeys, the null array and gshift may then be NULL.  This
 * is a filtered GROUP BY over the fact columns alone.  With nothing grouped all
 * qualifying rows form one group with key 0; with no qualifying row M = 0.  No
 * table is read and the pass asks for no dynamic LDS.
 *
 * hj_star_last_plan reports the call as it reports a star aggregate: 4
 * launches, or 3 when n == 0.
 *
 * Errors, in this order (extending the star aggregate's): a null star
 * (HJ_ERR_ARG, "null star", before any device is touched); ndims outside
 * 0..HJ_STAR_MAX_DIMS, or with ndims > 0 a null dims, kinds, skeys, null-value
 * array or gshift; per dimension as the star aggregate; the fact descriptor,
 * each HJ_ERR_ARG naming the field and index: npreds outside
 * 0..HJ_STAR_MAX_PREDS, a pkind outside the two, vop outside 0..3, nfact
 * outside 0..HJ_STAR_MAX_FACT_GROUPS, an fshift outside 0..63; no group
 * reserve (HJ_ERR_STATE); a null count pointer; n < 0; with n > 0 a null key
 * column, then a null pcol[p], then a null fcol[f]; the sval rule; vop !=
 * HJ_VALUE_A with sum / min / max asked for and vb == NULL (n > 0); the output
 * rules.  n == 0 takes null columns everywhere. */
#define HJ_STAR_MAX_PREDS 4
#define HJ_STAR_MAX_FACT_GROUPS 2
#define HJ_PRED_IN  0   /* the row needs plo <= col[j] <= phi            */
#define HJ_PRED_OUT 1   /* the row needs col[j] < plo or col[j] > phi    */
#define HJ_VALUE_A   0  /* v(j) = sval[j]                                */
#define HJ_VALUE_ADD 1  /* v(j) = sval[j] + vb[j]   (wrapping int64)     */
#define HJ_VALUE_SUB 2  /* v(j) = sval[j] - vb[j]                        */
#define HJ_VALUE_MUL 3  /* v(j) = sval[j] * vb[j]                        */
typedef struct {
    int npreds;
    const void *pcol[HJ_STAR_MAX_PREDS];
    int64_t plo[HJ_STAR_MAX_PREDS], phi[HJ_STAR_MAX_PREDS];
    int pkind[HJ_STAR_MAX_PREDS];
    int vop;
    const void *vb;
    int nfact;
    const void *fcol[HJ_STAR_MAX_FACT_GROUPS];
    int fshift[HJ_STAR_MAX_FACT_GROUPS];
    int64_t fbase[HJ_STAR_MAX_FACT_GROUPS];
} hj_star_fact;
int hj_dev_star_query_i64(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[],
                          const int64_t *const skeys[], const int64_t null_pay[], const int gshift[],
                          const int64_t gbase[], const hj_star_fact *fact, const int64_t *sval, int64_t n,
                          int64_t *out_key, int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                          int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_star_query_i32(hj_star *s, int ndims, hj_ctx *const dims[], const int kinds[],
                          const int32_t *const skeys[], const int32_t null_row[], const int gshift[],
                          const int64_t gbase[], const hj_star_fact *fact, const int32_t *sval, int64_t n,
                          int64_t *out_key, int64_t *out_cnt, int64_t *out_sum, int64_t *out_min, int64_t *out_max,
                          int64_t out_cap, uint64_t *d_count, void *stream);

/* Radix partition of rows into nparts (1..8192) groups by a key hash independent of
 * the table's slot hash: out_tuples (2*n int64) receives packed {key, pay}
 * tuples grouped by partition in order 0..nparts-1, d_counts (nparts uint64)
 * the group sizes.  Multi-GPU routing step (north_star: "build-side
 * partitioning ... probe tuples routed by the same radix"). */
int hj_dev_partition_i64(hj_ctx *ctx, const int64_t *key, const int64_t *pay, int64_t n, int nparts,
                         int64_t *out_tuples, uint64_t *d_counts, void *stream);
int hj_dev_partition_tuples_i64(hj_ctx *ctx, const int64_t *tuples, int64_t n, int nparts,
                                int64_t *out_tuples, uint64_t *d_counts, void *stream);
/* Owning partition of one key (host-side, same function as the kernels). */
int hj_partition_of(int64_t key, int nparts);

/* Folded routing (north_star: "probe tuples routed by the same radix"): a
 * row's owner AND its receiver's first radix-pass bin are the top
 * log2(nranks) + sub_bits bits of the radix join's own key hash, so the
 * received tuples are already first-pass partitioned and the receiver runs
 * one local pass fewer per relation (R and S).
 * hj_route_plan: sub_bits for a join of n_build_global build rows over nranks
 * ranks (a power of two, <= 64); *sub_bits = 0 when the fold does not apply
 * (small or non-radix local build sides, other rank counts): route with
 * hj_dev_partition_* then.  The same value on every rank. */
int hj_route_plan(int64_t n_build_global, int nranks, int *sub_bits);
/* out_tuples (2n int64): packed {key, pay} grouped by part = owner << sub_bits
 * | bin (<= 512 parts), parts in order; d_counts (nranks << sub_bits uint64):
 * part sizes.  One exact partition pass (line-tailed, like a radix pass) after
 * a key histogram. */
int hj_dev_route_i64(hj_ctx *ctx, const int64_t *key, const int64_t *pay, int64_t n, int nranks, int sub_bits,
                     int64_t *out_tuples, uint64_t *d_counts, void *stream);
/* Build from routed tuples: nsrc (1..64) sources' rows one after another,
 * each source's grouped by bin 0 .. 2^sub_bits - 1; d_counts (device, nsrc x
 * 2^sub_bits uint64, row s = source s's bin sizes).  nranks, sub_bits as
 * routed (nranks << sub_bits <= 512, else HJ_ERR_ARG).  Any counts are
 * joined exactly, empty sources and (source, bin) pairs of a few rows
 * included: the workspace is sized for rows / 64 + nsrc * 2^sub_bits listed
 * runs.
 * The build is an ordinary radix build of this owner's rows: besides
 * hj_dev_probe_routed_i64, hj_dev_probe_i64 / _tuples_i64, hj_dev_count_i64
 * and hj_dev_exists_i64 / _tuples_i64 over unrouted rows are valid after it
 * and return the join with the built rows (they run both local passes on
 * their probe side). */
int hj_dev_build_routed_i64(hj_ctx *ctx, const int64_t *tuples, int64_t n, const uint64_t *d_counts, int nsrc,
                            int nranks, int sub_bits, void *stream);
/* Probe routed tuples of bins [bin0, bin0 + nbins) only (the part of the probe
 * side that has arrived), laid out as for the build; d_counts nsrc x nbins.
 * Output as hj_dev_probe_i64. */
int hj_dev_probe_routed_i64(hj_ctx *ctx, const int64_t *tuples, int64_t n, const uint64_t *d_counts, int nsrc,
                            int bin0, int nbins, int64_t *out_r, int64_t *out_s, int64_t out_cap, uint64_t *d_count,
                            void *stream);

/* Deterministic synthetic relations (counter-based, so any slice of a
 * global relation can be generated independently on any GPU). */
int hj_dev_gen_pkfk_i64(uint64_t seed, int64_t NR, uint64_t hit_threshold,
                        int64_t r0, int64_t nr, int64_t *rkey, int64_t *rpay,
                        int64_t s0, int64_t ns, int64_t *skey, int64_t *spay, void *stream);
/* Zipf(theta) probe keys over the PK-FK build side of the same seed: S.key =
 * R.key[row(rank)], rank ~ Zipf(theta) over [0, NR) (Gray et al. inverse
 * CDF), S.pay = global row.  hj_zipf_params returns
 * {zeta(NR, theta), eta, alpha, 0.5^theta} (host, for the oracle). */
int hj_zipf_params(int64_t NR, double theta, double out[4]);
int hj_dev_gen_zipf_i64(uint64_t seed, int64_t NR, double theta, int64_t s0, int64_t ns, int64_t *skey,
                        int64_t *spay, void *stream);
int hj_dev_gen_uniform_i64(uint64_t seed, uint64_t stream_id, int64_t lo, int64_t hi,
                           int64_t i0, int64_t n, int64_t *key, int64_t *pay, void *stream);
int hj_dev_gen_uniform_i32(uint64_t seed, uint64_t stream_id, int32_t lo, int32_t hi,
                           int64_t i0, int64_t n, int32_t *key, void *stream);

/* nested-loop.mlir result rows (:29-192, @main :195-289).  Row-major int32
 * tables with the key in column 0 and row strides ld1 / ld2 (elements).
 * Roles as %table_1_or_2_as_inner (:247): the larger table is the outer X
 * (ties: t1), the smaller the inner Y; every pair X[i][0] == Y[j][0] yields
 * the row [X[i][0 .. cx), Y[j][1 .. cy)] (cx + cy - 1 columns).  Executed as
 * a hash join (build Y, probe X) plus a row gather.  d_count = M; rows past
 * out_cap are dropped.  Rows are in no particular order (as the reference's
 * atomic block offsets). */
int hj_dev_count_rows_i32(hj_ctx *ctx, const int32_t *t1, int64_t r1, int64_t c1, int64_t ld1, const int32_t *t2,
                          int64_t r2, int64_t c2, int64_t ld2, uint64_t *d_count, void *stream);
int hj_dev_join_rows_i32(hj_ctx *ctx, const int32_t *t1, int64_t r1, int64_t c1, int64_t ld1, const int32_t *t2,
                         int64_t r2, int64_t c2, int64_t ld2, int32_t *out, int64_t ldo, int64_t out_cap,
                         uint64_t *d_count, void *stream);

/* Selection (Experiments/selection.mlir:34-155): the elements v of `in`
 * with `v <cmp> value`, compacted in input order into out[0 .. min(M,
 * out_cap)), their source indices into out_row (optional, may be NULL);
 * d_count = M.  Float compares are ordered: NaN never passes (the reference
 * uses `cmpf olt`). */
#define HJ_CMP_LT 0
#define HJ_CMP_LE 1
#define HJ_CMP_GT 2
#define HJ_CMP_GE 3
#define HJ_CMP_EQ 4
#define HJ_CMP_NE 5
int hj_dev_select_f32(hj_ctx *ctx, const float *in, int64_t n, int cmp, float value, float *out, int64_t *out_row,
                      int64_t out_cap, uint64_t *d_count, void *stream);
int hj_dev_select_i64(hj_ctx *ctx, const int64_t *in, int64_t n, int cmp, int64_t value, int64_t *out,
                      int64_t *out_row, int64_t out_cap, uint64_t *d_count, void *stream);

/* Copy floor (measurement helper, no reference counterpart: SURVEY 8(d)
 * asks every figure to be set against the box's own HBM rate).  Copies
 * `rows` 16-B rows from `in` to `out` (device pointers, 16-B aligned) with
 * non-temporal loads and stores, in one of two shapes:
 *   HJ_COPY_PERSISTENT: one 1024-thread workgroup per CU over a contiguous
 *     range of 4096-row tiles, next tile's loads in flight (the radix
 *     partition passes' loop shape);
 *   HJ_COPY_FLAT: one row per thread over a grid of 256-thread workgroups
 *     (the fastest streamed copy this chip runs).
 * Asynchronous on `stream`; HJ_ERR_ARG for a bad shape or misaligned
 * pointer. */
#define HJ_COPY_PERSISTENT 0
#define HJ_COPY_FLAT 1
int hj_dev_stream_copy(const void *in, void *out, int64_t rows, int shape, void *stream);

/* Placement of the radix bucket sets' row buffers (diagnostics, no reference
 * counterpart).  A row buffer of >= 1 GiB (buckets >= 8 KiB) is probed when allocated: the
 * partition pass's write pattern against a flat write of the same bytes
 * (some physical placements run the pattern 25-35 % slower), redrawn up to 24
 * times while slow, best draw kept; HJ_PLACEMENT_PROBE=0 in the environment
 * turns the probe off.  Process-wide counts since load: draws probed, draws
 * rejected, and the pattern/flat ratio of the last and of the worst kept
 * buffer (0 when none was probed).  Any pointer may be null. */
void hj_placement_stats(long long *probes, long long *rejected, double *last_kept, double *worst_kept);
/* Since round 6 a probe holds at most 2 rejected draws at once (a further
 * reject frees the oldest) and draws again only while free memory is >= 3x
 * the buffer.  out[0] draws probed, [1] rejected, [2] buffers that kept a
 * slow draw (gave up), [3] of those, gave up because free memory ran short,
 * [4] most rejected draws held at once; ratios as hj_placement_stats. */
void hj_placement_stats_ex(long long out[5], double *last_kept, double *worst_kept);
/* The pattern/flat ratio a draw must reach to be kept at once (default
 * 1.12); returns the previous value, ratio <= 0 only reads it.  A knob for
 * tests (a low ratio makes every draw a reject). */
double hj_placement_set_good(double ratio);
/* The same probe on a caller's device buffer of >= 4 MiB per CU (its
 * contents are overwritten): *ratio = pass-pattern time / flat-write time
 * (~1.0 good placement, 1.25-1.35 slow).  Synchronous on the default stream.
 * The Python host side draws the routed-tuple buffers of hj_dev_route_i64
 * with it (hashjoin.HashJoin.route). */
int hj_placement_check(const void *buf, int64_t bytes, double *ratio);

/* Out-of-core join of HOST-resident int64 key/payload columns (relations
 * larger than HBM; the reference leaves the partitioned join out,
 * projectDescription.md:23-24).  When R does not fit device_budget bytes
 * (0 = 80 % of free HBM), R and S are routed by hj_partition_of into groups
 * that do, through the GPU in chunks; each group is built on the GPU and its
 * S side streamed through the probe with copies overlapping the probe.
 * Pairs (R.pay, S.pay) go to out_r/out_s (host); returns M (rows past
 * out_cap dropped) or < 0. */
int64_t hj_host_join_ooc_i64(hj_ctx *ctx, const int64_t *rkey, const int64_t *rpay, int64_t nr, const int64_t *skey,
                             const int64_t *spay, int64_t ns, int64_t *out_r, int64_t *out_s, int64_t out_cap,
                             uint64_t device_budget);

/* ------------------------------------------------------- host memref ABI
 * Two-phase, reference-shaped (mirrors @countRows -> alloc -> @probeRelation,
 * join_v2.mlir:672-688).  Each memref is the 5-scalar expansion; offset and
 * stride of every memref are honoured.  hj_probe_* returns HJ_OK, or
 * HJ_ERR_CAPACITY when the output memrefs' size differs from the join's row
 * count.
 *
 * Count -> probe reuse: the reference's @countRows leaves its table for
 * @probeRelation (join_v1.mlir:110-176).  hj_count_* uploads both relations,
 * BUILDS and COUNTS (no pairs are materialised) and keeps the built table and
 * the staged probe side.  A following hj_probe_* with inputs of the same
 * sizes probes that kept table (no upload, no build) when the inputs are
 * judged unchanged since the count, under the process-wide reuse mode:
 *   HJ_REUSE_DIGEST (default): a 128-bit content digest of every input
 *     memref, taken by the count and again by the probe on host threads
 *     (four multiply-rotate lanes, hj_capi.cpp digest_mem), matches.  The
 *     digest is NOT cryptographic: inputs crafted to collide with the counted
 *     ones would be joined as the counted ones.
 *   HJ_REUSE_EXACT: every input byte equals the count's (the count keeps a
 *     compacted host copy of its inputs -- host memory of the inputs' size --
 *     and the probe compares with memcmp on host threads).
 *   HJ_REUSE_OFF: nothing is kept; every hj_probe_* runs the whole join.
 * Anything else (changed inputs, another mode, another build in between)
 * runs the whole join.  Reused or not, the result is the join of the inputs
 * passed to hj_probe_*.
 * Output delivery is speculative: while the verdict is computed the kept
 * table's pairs are already written into the caller's output memrefs (when
 * their size equals the count's M); if the inputs turn out changed, the fresh
 * join's pairs are written over them.  On any error return the contents of
 * the output memrefs are undefined.  hj_host_memo_hits() counts the reuses.
 *
 * Threading: these host-memref entry points (and the ciface / rows /
 * selection ones below) use one default context per device; each call holds
 * that context's lock, so concurrent callers are serialised, never mixed. */
#define HJ_REUSE_DIGEST 0
#define HJ_REUSE_EXACT 1
#define HJ_REUSE_OFF 2
/* Set the reuse mode; returns the previous one, or HJ_ERR_ARG. */
int hj_host_set_reuse(int mode);
int64_t hj_host_memo_hits(void);
int64_t hj_count_i32(int32_t *r_alloc, int32_t *r_align, int64_t r_off, int64_t r_size, int64_t r_stride,
                     int32_t *s_alloc, int32_t *s_align, int64_t s_off, int64_t s_size, int64_t s_stride);
int32_t hj_probe_i32(int32_t *r_alloc, int32_t *r_align, int64_t r_off, int64_t r_size, int64_t r_stride,
                     int32_t *s_alloc, int32_t *s_align, int64_t s_off, int64_t s_size, int64_t s_stride,
                     int32_t *or_alloc, int32_t *or_align, int64_t or_off, int64_t or_size, int64_t or_stride,
                     int32_t *os_alloc, int32_t *os_align, int64_t os_off, int64_t os_size, int64_t os_stride);
/* int64 key/payload column pairs (Rkey, Rpay, Skey, Spay). */
int64_t hj_count_i64(int64_t *rk_alloc, int64_t *rk_align, int64_t rk_off, int64_t rk_size, int64_t rk_stride,
                     int64_t *rp_alloc, int64_t *rp_align, int64_t rp_off, int64_t rp_size, int64_t rp_stride,
                     int64_t *sk_alloc, int64_t *sk_align, int64_t sk_off, int64_t sk_size, int64_t sk_stride,
                     int64_t *sp_alloc, int64_t *sp_align, int64_t sp_off, int64_t sp_size, int64_t sp_stride);
int32_t hj_probe_i64(int64_t *rk_alloc, int64_t *rk_align, int64_t rk_off, int64_t rk_size, int64_t rk_stride,
                     int64_t *rp_alloc, int64_t *rp_align, int64_t rp_off, int64_t rp_size, int64_t rp_stride,
                     int64_t *sk_alloc, int64_t *sk_align, int64_t sk_off, int64_t sk_size, int64_t sk_stride,
                     int64_t *sp_alloc, int64_t *sp_align, int64_t sp_off, int64_t sp_size, int64_t sp_stride,
                     int64_t *or_alloc, int64_t *or_align, int64_t or_off, int64_t or_size, int64_t or_stride,
                     int64_t *os_alloc, int64_t *os_align, int64_t os_off, int64_t os_size, int64_t os_stride);

/* nested-loop.mlir rows over host 2-D memrefs (7 scalars each: allocated,
 * aligned, offset, sizes[2], strides[2]).  hj_join_rows_i32 writes the M rows
 * into the result memref (>= M rows, c1 + c2 - 1 columns) and returns M, or
 * < 0 (HJ_ERR_CAPACITY when the result has fewer than M rows). */
int64_t hj_count_rows_i32(int32_t *t1_alloc, int32_t *t1_align, int64_t t1_off, int64_t t1_rows, int64_t t1_cols,
                          int64_t t1_s0, int64_t t1_s1, int32_t *t2_alloc, int32_t *t2_align, int64_t t2_off,
                          int64_t t2_rows, int64_t t2_cols, int64_t t2_s0, int64_t t2_s1);
int64_t hj_join_rows_i32(int32_t *t1_alloc, int32_t *t1_align, int64_t t1_off, int64_t t1_rows, int64_t t1_cols,
                         int64_t t1_s0, int64_t t1_s1, int32_t *t2_alloc, int32_t *t2_align, int64_t t2_off,
                         int64_t t2_rows, int64_t t2_cols, int64_t t2_s0, int64_t t2_s1, int32_t *o_alloc,
                         int32_t *o_align, int64_t o_off, int64_t o_rows, int64_t o_cols, int64_t o_s0,
                         int64_t o_s1);

/* selection.mlir's query over host memrefs: in[i] < value (olt) compacted
 * into the result memref; returns M, or < 0 (HJ_ERR_CAPACITY if the result
 * memref is shorter than M). */
int64_t hj_select_f32(float *in_alloc, float *in_align, int64_t in_off, int64_t in_size, int64_t in_stride,
                      float value, float *out_alloc, float *out_align, int64_t out_off, int64_t out_size,
                      int64_t out_stride);

/* ------------------------------------------------------ MLIR C-interface
 * Descriptor structs of memref<?xT> / memref<?x2xT> (MLIR's StridedMemRefType
 * layout: allocated, aligned, offset, sizes[rank], strides[rank]). */
typedef struct { int32_t *allocated; int32_t *aligned; int64_t offset; int64_t sizes[1]; int64_t strides[1]; } hj_memref1_i32;
typedef struct { int64_t *allocated; int64_t *aligned; int64_t offset; int64_t sizes[1]; int64_t strides[1]; } hj_memref1_i64;
typedef struct { int32_t *allocated; int32_t *aligned; int64_t offset; int64_t sizes[2]; int64_t strides[2]; } hj_memref2_i32;
typedef struct { int64_t *allocated; int64_t *aligned; int64_t offset; int64_t sizes[2]; int64_t strides[2]; } hj_memref2_i64;

/* memref<?xi32> R, S -> memref<?x2xi32> rows (rowR, rowS): the reference's
 * whole @main join (join_v2.mlir:607-730) as one call. */
void _mlir_ciface_hj_join_i32(hj_memref2_i32 *result, hj_memref1_i32 *r, hj_memref1_i32 *s);
/* memref<?xi64> R, S keys (payload = row id) -> memref<?x2xi64> (rowR, rowS). */
void _mlir_ciface_hj_join_i64(hj_memref2_i64 *result, hj_memref1_i64 *r, hj_memref1_i64 *s);
/* key/payload column pairs -> memref<?x2xi64> (R.pay, S.pay). */
void _mlir_ciface_hj_join_kp_i64(hj_memref2_i64 *result, hj_memref1_i64 *rkey, hj_memref1_i64 *rpay,
                                 hj_memref1_i64 *skey, hj_memref1_i64 *spay);
/* memref<?x?xi32> tables -> memref<?x?xi32> rows of nested-loop.mlir
 * (exactly M rows, malloc'ed). */
void _mlir_ciface_hj_join_rows_i32(hj_memref2_i32 *result, hj_memref2_i32 *t1, hj_memref2_i32 *t2);
/* Release a result buffer of the ciface joins (== free(allocated)). */
void hj_free_result(void *allocated);

#ifdef __cplusplus
}
#endif

#endif /* HJ_H_ */
