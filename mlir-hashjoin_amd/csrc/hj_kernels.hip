// hj_kernels.hip -- hand-written CDNA4 (gfx950) kernels of the hash join.
//
// Reference kernels replaced (kernel inventory):
//   initializeHT  join_v1.mlir:180-202  -> k_init    (slot fill, 16 B/lane)
//   build         join_v1.mlir:213-277  -> k_build   (linear probing, 64-bit CAS)
//   count         join_v1.mlir:288-425  -> k_probe<WRITE=false>
//   probe v1/v2   join_v1.mlir:436-521, join_v2.mlir:450-604
//                                       -> k_probe<WRITE=true>: ILP slot
//                                          reads, ballot-compacted output,
//                                          one global cursor add per block
// plus the exists probes (k_probe_exists), the positional lookup probe
// (k_probe_lookup), the star probe (k_star: up to four tables per probe row),
// the as-of probe (k_probe_asof), the expand probe's scan and global-table fill
// (k_expand_sums, k_expand_scan_sums, k_expand_offsets, k_probe_expand),
// the outer probe (k_probe_outer),
// the build-side outer stages (k_probe_mark, k_emit_unmatched),
// the group probe (k_group_init, k_probe_group, k_emit_groups),
// the hash aggregate (k_aggregate, k_emit_aggregate), the star aggregate
// (k_star_agg: the star probe's walks in front of the aggregate's collapse),
// the radix partition used by the
// multi-GPU exchange, the selection, the counter-based generators of the
// benchmark inputs and the copy floors.
//
// Wave64 throughout: 256-thread blocks (4 waves), all per-lane work
// independent, no warp-32 idioms.  Integer/byte work: no MFMA.
//
// Written once, used by several kernels / launchers:
//   TableView        the table in global memory or staged in LDS (k_probe, k_probe_exists, k_probe_lookup, k_probe_asof, k_probe_expand, k_probe_outer)
//   wave_incl_add    every wave prefix sum (hj_internal.h: DPP, no LDS round trips)
//   with_layout_form the (layout, form) -> template-argument dispatch of the launchers
//   probe_grid       the tile probes' grid and LDS bytes
//   k_probe_slow     the general path of k_probe and (with the null value) of k_probe_outer
//   cu_count         the CU count (hj_radix.hip)
// k_probe and k_probe_exists still each spell out their row load, chain walk
// and ballot compaction, and the three count kernels their block sum: as
// shared functions these compiled to other instruction streams (DESIGN.md,
// "Refactor check (global-table kernels)").  A fix to one copy belongs in
// the other too.
#include <type_traits>

#include "hj_internal.h"
#include "hj_gen.h"

namespace hj {
namespace {

constexpr int kBlock = 256;
constexpr int kBuildItems = 4;   // rows per thread in build (CAS ILP)
constexpr int kProbeItems = 8;   // rows per thread in probe (tile = 2048 rows)
constexpr int kPartItems = 8;    // rows per thread in partition

__device__ __forceinline__ unsigned long long slot_of(unsigned long long k, int shift) {
    return (k * 0x9E3779B97F4A7C15ull) >> shift;   // Fibonacci hashing, top bits
}

// ------------------------------------------------------------------ sources
struct Tuple {
    unsigned long long k, p;
};

template <int FORM>
__device__ __forceinline__ Tuple load_src(const SrcDev &s, long long row);

template <>
__device__ __forceinline__ Tuple load_src<kCols64>(const SrcDev &s, long long row) {
    return {((const unsigned long long *)s.key)[row], ((const unsigned long long *)s.pay)[row]};
}
template <>
__device__ __forceinline__ Tuple load_src<kPacked64>(const SrcDev &s, long long row) {
    const ulonglong2 v = ((const ulonglong2 *)s.key)[row];
    return {v.x, v.y};
}
template <>
__device__ __forceinline__ Tuple load_src<kCol32>(const SrcDev &s, long long row) {
    return {(unsigned long long)(unsigned)((const int *)s.key)[row],
            (unsigned long long)(s.row_base + row)};
}

// ------------------------------------------------------------------ layouts
template <int L>
struct Lay;

template <>
struct Lay<kWide> {
    using slot_t = Slot64;
    using out_t = long long;
    static constexpr unsigned long long kEmptyWord = kEmptyKey64;
    static __device__ __forceinline__ unsigned long long *word(slot_t *sl, unsigned long long h) { return &sl[h].key; }
    static __device__ __forceinline__ unsigned long long cas_val(unsigned long long k, unsigned long long) { return k; }
    static __device__ __forceinline__ unsigned long long word_key(unsigned long long w) { return w; }
    static __device__ __forceinline__ void after_claim(slot_t *sl, unsigned long long h, unsigned long long p) { sl[h].pay = p; }
    static __device__ __forceinline__ bool empty(const slot_t &s) { return s.key == kEmptyKey64; }
    static __device__ __forceinline__ unsigned long long key(const slot_t &s) { return s.key; }
    static __device__ __forceinline__ unsigned long long pay(const slot_t &s) { return s.pay; }
    static __device__ __forceinline__ bool null_key(unsigned long long k) { return k == kEmptyKey64; }
};

template <>
struct Lay<kNarrow> {
    using slot_t = unsigned long long;
    using out_t = int;
    static constexpr unsigned long long kEmptyWord = kEmptySlot32;
    static __device__ __forceinline__ unsigned long long *word(slot_t *sl, unsigned long long h) { return &sl[h]; }
    static __device__ __forceinline__ unsigned long long cas_val(unsigned long long k, unsigned long long p) { return (k << 32) | (p & 0xffffffffull); }
    static __device__ __forceinline__ unsigned long long word_key(unsigned long long w) { return w >> 32; }
    static __device__ __forceinline__ void after_claim(slot_t *, unsigned long long, unsigned long long) {}
    static __device__ __forceinline__ bool empty(const slot_t &s) { return s == kEmptySlot32; }
    static __device__ __forceinline__ unsigned long long key(const slot_t &s) { return s >> 32; }
    static __device__ __forceinline__ unsigned long long pay(const slot_t &s) { return s & 0xffffffffull; }
    static __device__ __forceinline__ bool null_key(unsigned long long) { return false; }
};

template <int N, typename T>
__device__ __forceinline__ T pick(const T (&a)[N], int i) {   // static-index select: no scratch
    T r = a[0];
#pragma unroll
    for (int j = 1; j < N; ++j) r = (i == j) ? a[j] : r;
    return r;
}
// The same select with the indices as template arguments, for k_probe_slow's
// outer instantiations: under pick() the compiler keeps the writing general
// path's K and P in scratch (144 B per lane, one indexed load per row); with
// no loop index ever applied to the arrays they stay in registers.  The inner
// instantiations keep pick(): their machine code is held as it was.
template <int J, int N, typename T>
__device__ __forceinline__ T pick_c(const T (&a)[N], int i) {
    if constexpr (J == N - 1) {
        return a[J];
    } else {
        const T r = pick_c<J + 1>(a, i);
        return i == J ? a[J] : r;
    }
}

// ------------------------------------------------------------------ init
// initializeHT (join_v2.mlir:203-225) sets heads[:] = -1; here every slot is
// set EMPTY with 16-B stores, and the side count / dup flag are reset.
template <int L>
__global__ __launch_bounds__(kBlock) void k_init(TableDev t, unsigned long long n16) {
    const ulonglong2 v = (L == kWide) ? make_ulonglong2(kEmptyKey64, 0ull)
                                      : make_ulonglong2(kEmptySlot32, kEmptySlot32);
    ulonglong2 *p = (ulonglong2 *)t.slots;
    const unsigned long long base = (unsigned long long)blockIdx.x * (kBlock * 4) + threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned long long j = base + (unsigned long long)i * kBlock;
        if (j < n16) p[j] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) t.meta[threadIdx.x] = 0ull;
}

// ------------------------------------------------------------------ build
// build + @insertNodeInHashTable (join_v2.mlir:236-300): the reference takes
// a node with atomicAdd(freeIndex) -- one address hit by every thread -- and
// prepends it with atomicExch on the bucket head.  Here each row claims its
// own slot with one 64-bit CAS at its hash position (linear probing on
// failure).  The first CAS of all kBuildItems rows is issued before any
// result is consumed, so each lane has that many atomics in flight.
// A failed CAS that returns the row's own key proves the build side has a
// duplicate key (both rows walk the same probe sequence, so the later one
// must fail on the earlier one's slot); that sets meta[1], and probes then
// keep walking past matches.  Without duplicates a probe stops at its match.
// INT64_MIN keys sit in the side list, not in a slot: the row that finds the
// list non-empty is the repeat (hj_ctx_build_has_duplicates answers for them too).
template <int L, int FORM>
__global__ __launch_bounds__(kBlock) void k_build(TableDev t, SrcDev src) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    slot_t *sl = (slot_t *)t.slots;
    const long long base = (long long)blockIdx.x * (kBlock * kBuildItems) + threadIdx.x;
    unsigned long long k[kBuildItems], p[kBuildItems], h[kBuildItems], o[kBuildItems];
    bool v[kBuildItems];
#pragma unroll
    for (int i = 0; i < kBuildItems; ++i) {
        const long long row = base + (long long)i * kBlock;
        v[i] = row < src.n;
        Tuple tp = v[i] ? load_src<FORM>(src, row) : Tuple{0ull, 0ull};
        k[i] = tp.k;
        p[i] = tp.p;
    }
    bool dup = false;
#pragma unroll
    for (int i = 0; i < kBuildItems; ++i) {
        if (v[i] && LY::null_key(k[i])) {   // wide only: INT64_MIN keys -> side list
            const unsigned long long idx = atomicAdd(&t.meta[0], 1ull);
            t.side[idx] = p[i];
            dup |= idx != 0ull;             // a second INT64_MIN row repeats a key like any other
            v[i] = false;
        }
        h[i] = slot_of(k[i], t.shift);
        o[i] = v[i] ? atomicCAS(LY::word(sl, h[i]), LY::kEmptyWord, LY::cas_val(k[i], p[i]))
                    : LY::kEmptyWord;
    }
#pragma unroll
    for (int i = 0; i < kBuildItems; ++i) {
        if (!v[i]) continue;
        unsigned long long hh = h[i], old = o[i];
        while (old != LY::kEmptyWord) {
            dup |= (LY::word_key(old) == k[i]);
            hh = (hh + 1) & t.mask;
            old = atomicCAS(LY::word(sl, hh), LY::kEmptyWord, LY::cas_val(k[i], p[i]));
        }
        LY::after_claim(sl, hh, p[i]);
    }
    // one store per block: same-address stores from every thread that saw a
    // repeated key serialise at the memory side (the radix join's flag cost
    // 3.5 ms at 2^28 uniform keys before it was made per workgroup)
    if (__syncthreads_or(dup ? 1 : 0) && threadIdx.x == 0)
        __hip_atomic_store(&t.meta[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------ probe tiles
// A probe tile is kProbeItems * kBlock rows: tile q = rows [q * kTile, ...).
constexpr int kProbeTile = kBlock * kProbeItems;
#ifndef HJ_LDS_TABLE_BYTES
#define HJ_LDS_TABLE_BYTES 65536
#endif
// global tables up to this size are probed from LDS (k_probe<..., LDS>);
// kLdsPerCu: the LDS the copies of one CU's workgroups may take together
constexpr int kLdsTableBytes = HJ_LDS_TABLE_BYTES;
constexpr int kLdsPerCu = 128 * 1024;
// the LDS a CU has, and a bound on k_star_agg's static LDS (its collapse table
// and a few words): its table copies are planned into what is left of the CU
// beside that, and into no more than kLdsPerCu
constexpr int kLdsCu = 160 * 1024;
constexpr int kStarAggStaticLds = 19 * 1024;

template <int L, int FORM>
__device__ __forceinline__ bool probe_row(const SrcDev &src, unsigned long long q, int i, Tuple &tp) {
    const long long row = (long long)q * kProbeTile + (long long)i * kBlock + threadIdx.x;
    if (row >= src.n) return false;
    tp = load_src<FORM>(src, row);
    return true;
}

// The table as the tile probes read it: from global memory, or (LDS) from
// the copy that every workgroup makes once in s_tab, its dynamic LDS.
template <int L, bool LDS>
struct TableView {
    using slot_t = typename Lay<L>::slot_t;
    const slot_t *sl;
    __device__ __forceinline__ TableView(const TableDev &t, ulonglong2 *s_tab) {
        if constexpr (LDS) {
            const unsigned long long n16 = (t.mask + 1) * sizeof(slot_t) / 16;
            const ulonglong2 *g16 = (const ulonglong2 *)t.slots;
            for (unsigned long long j = threadIdx.x; j < n16; j += kBlock) s_tab[j] = g16[j];
            __syncthreads();
            sl = (const slot_t *)s_tab;
        } else {
            sl = (const slot_t *)t.slots;
        }
    }
    __device__ __forceinline__ slot_t at(unsigned long long h) const { return sl[h]; }
};

// ------------------------------------------------------------------ slot marks
// The build-side outer probes' mark bitmap (one bit per slot, "some S row of
// this call matched it"; see "build-side outer probe" below).  mark_first
// sets slot h's bit and says whether this call was the first to: the word is
// read before the atomic OR, which is skipped when the bit is already set --
// at PK-FK fan-in all S rows of a build key but the first issue no atomic.
__device__ __forceinline__ bool mark_first(unsigned *marks, unsigned long long h) {
    unsigned *w = marks + (h >> 5);
    const unsigned bit = 1u << (unsigned)(h & 31ull);
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) return false;
    return !(atomicOr(w, bit) & bit);
}
// Marks the matched slots MH[i] (bits of `found`) of a tile the fast path
// keeps: the 8 words are read before any atomic is issued.
template <int N>
__device__ __forceinline__ void mark_found(unsigned *marks, unsigned found, const unsigned long long (&MH)[N]) {
    unsigned W[N];
#pragma unroll
    for (int i = 0; i < N; ++i)
        if ((found >> i) & 1u) W[i] = __hip_atomic_load(marks + (MH[i] >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const unsigned bit = 1u << (unsigned)(MH[i] & 31ull);
        if (((found >> i) & 1u) && !(W[i] & bit)) atomicOr(marks + (MH[i] >> 5), bit);
    }
}

// ------------------------------------------------------------------ probe
// count (join_v1.mlir:288-425, join_v2.mlir:311-439) and probe
// (join_v1.mlir:436-521, join_v2.mlir:450-604) in one kernel family.
//
// Each thread owns kProbeItems rows of a 2048-row tile (coalesced loads).
//
// Fast path (duplicate-free build side, no INT64_MIN probe key in the tile):
// every row's first slot load is issued before any is resolved, so a lane
// has kProbeItems random reads in flight (the table read is latency-bound:
// one dependent read per lane at a time left HBM idle); rows still open
// after their first slot walk the chain.  A row matches at most once, so
// the output is compacted with wave ballots in row-slot-major order: each
// store instruction writes one contiguous run per wave, after ONE global
// cursor add per tile.
//
// General path (duplicates or null keys): a flattened per-lane loop (one
// slot load per iteration; a lane moves to its next row when the current is
// resolved) with matches staged in LDS through a wave-aggregated cursor (the
// v2 idea, join_v2.mlir:525-538), one cursor add per tile and a coalesced
// flush; more than kStage matches spill straight to global (the v2 overflow
// path, :539-549).  The cursor counts every match, so a caller whose
// capacity was too small still learns the exact M (rows past cap dropped).
//
// LDS (small tables, <= kLdsTableBytes): each workgroup first copies the
// whole table into LDS and the fast path reads its slots there (TableView:
// the copy and the slot read, for this kernel and k_probe_exists); the probes
// of a table that fits one XCD's L2 were random L2 reads (~82-96 G/s), well
// below the rate the probe side streams at (profiles/r06/r06sr_small_build_sides.txt).
//
// MARKS: empty, or one unsigned * -- the build-side outer probes' mark bitmap:
// a tile that stays on the fast path sets the bit of every slot a row matched
// (one per found row: a tile with a multi-match row has left), so only the
// tiles handed to the general path need k_probe_mark afterwards.  A pack, so
// the instantiations without it keep their kernel arguments and machine code.
template <int L, int FORM, bool WRITE, bool LDS = false, typename... MARKS>
__global__ __launch_bounds__(kBlock) void k_probe(TableDev t, SrcDev src, OutDev out, unsigned *slow,
                                                  unsigned long long slow_cap, MARKS... marks) {
    static_assert(sizeof...(MARKS) <= 1, "at most the mark bitmap");
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using out_t = typename LY::out_t;
    constexpr int NW = kBlock / 64;
    __shared__ unsigned long long st_base;
    __shared__ unsigned long long wsum[NW];
    __shared__ unsigned s_cw[kProbeItems * NW];
    extern __shared__ ulonglong2 s_tab[];

    const TableView<L, LDS> tab(t, s_tab);
    const bool unique = (__hip_atomic_load(&t.meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long nt = (unsigned long long)((src.n + kProbeTile - 1) / kProbeTile);
    // A tile handed to the general path (to_slow) leaves the body by
    // `continue` and so skips the barrier at its end.  That is safe only
    // because nothing between the loop head and the last `continue` touches
    // s_cw, st_base or wsum: the row loads, the chain walks and tab.at() use
    // registers and the table alone.  Code moved above that point must keep it so.
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long K[kProbeItems], P[kProbeItems];
        bool V[kProbeItems];
        bool has_null = false;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            Tuple tp{0ull, 0ull};
            V[i] = probe_row<L, FORM>(src, q, i, tp);
            K[i] = tp.k;
            P[i] = tp.p;
            has_null |= V[i] && LY::null_key(K[i]);
        }
        // general path (k_probe_slow takes the tile): a null probe key, or
        // -- with repeated build keys -- a row with more than one match
        auto to_slow = [&]() {
            if (threadIdx.x == 0) {
                const unsigned long long j = atomicAdd(&t.meta[3], 1ull);
                if (j < slow_cap) slow[j] = (unsigned)q;   // (sized so it always is; else k_probe_slow flags the count)
            }
        };
        if (__syncthreads_or(has_null ? 1 : 0)) {
            to_slow();
            continue;
        }
        slot_t S[kProbeItems];
        unsigned long long H[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            H[i] = slot_of(K[i], t.shift);
            if (V[i]) S[i] = tab.at(H[i]);
        }
        unsigned found = 0;
        unsigned long long RP[kProbeItems];
        [[maybe_unused]] unsigned long long MH[kProbeItems];   // MARKS: the matched slots
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            RP[i] = 0;
            if constexpr (sizeof...(MARKS) == 1) MH[i] = 0;
            if (!V[i]) continue;
            // duplicate-free table: the chain ends at the match or at EMPTY
            // (a two-exit loop with nothing else in it)
            slot_t sv = S[i];
            unsigned long long hh = H[i];
            while (!LY::empty(sv) && LY::key(sv) != K[i]) {
                hh = (hh + 1) & t.mask;
                sv = tab.at(hh);
            }
            if (!LY::empty(sv)) {
                found |= 1u << i;
                RP[i] = LY::pay(sv);
                if constexpr (sizeof...(MARKS) == 1) MH[i] = hh;
            }
        }
        if (!unique) {
            // repeated build keys: a matched row walks on to EMPTY; a second
            // copy of its key sends the tile to the general path (a few
            // repeated keys used to send every tile there: i32 2^12 random
            // build keys, 3.2 ms against 0.6 without a repeat,
            // profiles/r06/r06lu_lds_table_probe_ab.txt)
            bool multi = false;
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) {
                if (!((found >> i) & 1u)) continue;
                unsigned long long hh = slot_of(K[i], t.shift);
                slot_t sv = tab.at(hh);
                while (!LY::empty(sv) && LY::key(sv) != K[i]) {   // (back to the first copy)
                    hh = (hh + 1) & t.mask;
                    sv = tab.at(hh);
                }
                hh = (hh + 1) & t.mask;
                sv = tab.at(hh);
                while (!LY::empty(sv) && !multi) {
                    multi = LY::key(sv) == K[i];
                    hh = (hh + 1) & t.mask;
                    sv = tab.at(hh);
                }
            }
            if (__syncthreads_or(multi ? 1 : 0)) {
                to_slow();
                continue;
            }
        }
        if constexpr (sizeof...(MARKS) == 1) mark_found((marks, ...), found, MH);
        if constexpr (!WRITE) {
            unsigned long long c = (unsigned long long)__popc(found);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
            if (lane == 0) wsum[wv] = c;
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned long long tot = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) tot += wsum[w];
                if (tot) atomicAdd(out.counter, tot);
            }
        } else {
            const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
            unsigned lpre[kProbeItems];
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) {
                const unsigned long long bal = __ballot((found >> i) & 1u);
                lpre[i] = (unsigned)__popcll(bal & lt);
                if (lane == 0) s_cw[i * NW + wv] = (unsigned)__popcll(bal);
            }
            __syncthreads();
            if (wv == 0) {   // exclusive scan of the kProbeItems * NW runs (<= 64)
                static_assert(kProbeItems * NW <= 64, "one lane per run");
                const unsigned v = lane < kProbeItems * NW ? s_cw[lane] : 0u;
                const unsigned x = wave_incl_add(v);
                if (lane < kProbeItems * NW) s_cw[lane] = x - v;
                if (lane == 63) st_base = x ? atomicAdd(out.counter, (unsigned long long)x) : 0ull;
            }
            __syncthreads();
            out_t *orr = (out_t *)out.r;
            out_t *oss = (out_t *)out.s;
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) {
                if (!((found >> i) & 1u)) continue;
                const unsigned long long gi = st_base + s_cw[i * NW + wv] + lpre[i];
                if (gi < (unsigned long long)out.cap) {
                    orr[gi] = (out_t)RP[i];
                    oss[gi] = (out_t)P[i];
                }
            }
        }
        __syncthreads();   // s_cw / st_base / wsum reused by the next tile
    }
}

// General path over the tiles k_probe handed over (slow[0 .. meta[3])):
// persistent workgroups, one tile at a time.
// NULLV: empty (the inner join), or one unsigned long long -- k_probe_outer's
// general path: a row whose walk ended without a match emits (null, S.pay).
// A pack, not a flag plus an argument: the inner instantiations keep their
// kernel arguments, and with them their machine code, as they were.
template <int L, int FORM, bool WRITE, typename... NULLV>
__global__ __launch_bounds__(kBlock) void k_probe_slow(TableDev t, SrcDev src, OutDev out, const unsigned *slow,
                                                       unsigned long long slow_cap, NULLV... null_pay) {
    constexpr bool OUTER = sizeof...(NULLV) == 1;
    static_assert(sizeof...(NULLV) <= 1, "at most the null value");
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using out_t = typename LY::out_t;
    constexpr int kStage = 1024;
    constexpr int NW = kBlock / 64;
    __shared__ out_t st_r[WRITE ? kStage : 1];
    __shared__ out_t st_s[WRITE ? kStage : 1];
    __shared__ unsigned st_n;
    __shared__ unsigned long long st_base;
    __shared__ unsigned long long wsum[NW];

    const slot_t *sl = (const slot_t *)t.slots;
    const bool unique = (__hip_atomic_load(&t.meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull);
    const unsigned long long ntiles = t.meta[3] < slow_cap ? t.meta[3] : slow_cap;
    // an undersized slow list would drop tiles: report it through the count
    // (bit 63, never a real M) rather than return a short result
    if (blockIdx.x == 0 && threadIdx.x == 0 && t.meta[3] > slow_cap) atomicOr(out.counter, 1ull << 63);
    for (unsigned long long j = blockIdx.x; j < ntiles; j += gridDim.x) {
        if (threadIdx.x == 0) st_n = 0u;
        const unsigned id = slow[j];
        unsigned long long K[kProbeItems], P[kProbeItems];
        bool V[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            Tuple tp{0ull, 0ull};
            V[i] = probe_row<L, FORM>(src, id, i, tp);
            K[i] = tp.k;
            P[i] = tp.p;
        }
        __syncthreads();   // st_n visible

        unsigned long long cnt = 0;
        auto emit = [&](unsigned long long rv, unsigned long long sv) {
            if constexpr (!WRITE) {
                ++cnt;
            } else {
                const unsigned idx = atomicAdd(&st_n, 1u);
                if (idx < (unsigned)kStage) {
                    st_r[idx] = (out_t)rv;
                    st_s[idx] = (out_t)sv;
                } else {
                    const unsigned long long g = atomicAdd(out.counter, 1ull);
                    if (g < (unsigned long long)out.cap) {
                        ((out_t *)out.r)[g] = (out_t)rv;
                        ((out_t *)out.s)[g] = (out_t)sv;
                    }
                }
            }
        };

        int it = -1;
        bool have = false;
        [[maybe_unused]] bool hit = false;   // OUTER: the current row has matched
        unsigned long long k = 0, p = 0, hh = 0;
        while (true) {
            while (!have) {
                if (++it >= kProbeItems) break;
                if constexpr (OUTER) {
                    if (!pick_c<0>(V, it)) continue;
                    k = pick_c<0>(K, it);
                    p = pick_c<0>(P, it);
                } else {
                    if (!pick(V, it)) continue;
                    k = pick(K, it);
                    p = pick(P, it);
                }
                if (LY::null_key(k)) {   // wide: INT64_MIN probe key matches every side row
                    const unsigned long long ns = t.meta[0];
                    for (unsigned long long q = 0; q < ns; ++q) emit(t.side[q], p);
                    if constexpr (OUTER)
                        if (ns == 0ull) emit(null_pay..., p);
                    continue;
                }
                hh = slot_of(k, t.shift);
                have = true;
                if constexpr (OUTER) hit = false;
            }
            if (!have) break;
            const slot_t s = sl[hh];
            if (LY::empty(s)) {
                if constexpr (OUTER)
                    if (!hit) emit(null_pay..., p);
                have = false;
            } else {
                if (LY::key(s) == k) {
                    emit(LY::pay(s), p);
                    if constexpr (OUTER) hit = true;
                    if (unique) have = false;
                }
                hh = (hh + 1) & t.mask;
            }
        }

        if constexpr (WRITE) {
            __syncthreads();
            const unsigned nb = st_n;
            const unsigned nl = nb < (unsigned)kStage ? nb : (unsigned)kStage;
            if (threadIdx.x == 0) st_base = nl ? atomicAdd(out.counter, (unsigned long long)nl) : 0ull;
            __syncthreads();
            const unsigned long long gb = st_base;
            out_t *orr = (out_t *)out.r;
            out_t *oss = (out_t *)out.s;
            for (unsigned q = threadIdx.x; q < nl; q += kBlock) {
                const unsigned long long g = gb + q;
                if (g < (unsigned long long)out.cap) {
                    orr[g] = st_r[q];
                    oss[g] = st_s[q];
                }
            }
        } else {
            unsigned long long c = cnt;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
            if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned long long tot = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) tot += wsum[w];
                if (tot) atomicAdd(out.counter, tot);
            }
        }
        __syncthreads();   // st_n / staging reused by the next tile
    }
}

// ------------------------------------------------------------------ exists probe
// Semi- / anti-join probe (EXISTS / NOT EXISTS): the S rows that have / have
// no partner in the built table.  k_probe's shape -- 2048-row tiles, every
// row's first slot load issued before any is resolved, the LDS copy of small
// tables (TableView), ballot compaction in row-slot-major order after ONE
// cursor add per tile (k_probe<WRITE>'s, statement for statement: keep the
// two equal) -- without its general path: a row yields at most one output element
// whatever the build side repeats, so a chain walk ends at the first equal
// key or at EMPTY, meta[1] is never read and no tile is handed on.  A wide
// INT64_MIN probe key matches iff the side list holds a row (meta[0]).
// out.r: the S keys (optional, may be null), out.s: the S payloads; anti
// inverts `found` before the ballots.  out.cap == 0 is the count-only form
// (nothing is written; kind, count-only and out.r are wave-uniform runtime
// branches: one instantiation per layout, form and table placement).
template <int L, int FORM, bool LDS>
__global__ __launch_bounds__(kBlock) void k_probe_exists(TableDev t, SrcDev src, OutDev out, unsigned anti) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using out_t = typename LY::out_t;
    constexpr int NW = kBlock / 64;
    __shared__ unsigned long long st_base;
    __shared__ unsigned s_cw[kProbeItems * NW];
    extern __shared__ ulonglong2 s_tab[];

    const TableView<L, LDS> tab(t, s_tab);
    const bool side_rows = L == kWide && t.meta[0] != 0ull;   // the build side holds an INT64_MIN key
    const unsigned flip = anti ? (1u << kProbeItems) - 1u : 0u;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long nt = (unsigned long long)((src.n + kProbeTile - 1) / kProbeTile);
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long K[kProbeItems], P[kProbeItems], H[kProbeItems];
        unsigned valid = 0, walk = 0, found = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            Tuple tp{0ull, 0ull};
            if (probe_row<L, FORM>(src, q, i, tp)) {
                valid |= 1u << i;
                if (LY::null_key(tp.k)) found |= side_rows ? 1u << i : 0u;
                else walk |= 1u << i;
            }
            K[i] = tp.k;
            P[i] = tp.p;
        }
        slot_t S[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            H[i] = slot_of(K[i], t.shift);
            if ((walk >> i) & 1u) S[i] = tab.at(H[i]);
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((walk >> i) & 1u)) continue;
            slot_t sv = S[i];
            unsigned long long hh = H[i];
            while (!LY::empty(sv) && LY::key(sv) != K[i]) {
                hh = (hh + 1) & t.mask;
                sv = tab.at(hh);
            }
            if (!LY::empty(sv)) found |= 1u << i;
        }
        found = (found ^ flip) & valid;
        const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
        unsigned lpre[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const unsigned long long bal = __ballot((found >> i) & 1u);
            lpre[i] = (unsigned)__popcll(bal & lt);
            if (lane == 0) s_cw[i * NW + wv] = (unsigned)__popcll(bal);
        }
        __syncthreads();
        if (wv == 0) {   // exclusive scan of the kProbeItems * NW runs (<= 64)
            static_assert(kProbeItems * NW <= 64, "one lane per run");
            const unsigned v = lane < kProbeItems * NW ? s_cw[lane] : 0u;
            const unsigned x = wave_incl_add(v);
            if (lane < kProbeItems * NW) s_cw[lane] = x - v;
            if (lane == 63) st_base = x ? atomicAdd(out.counter, (unsigned long long)x) : 0ull;
        }
        __syncthreads();
        out_t *okk = (out_t *)out.r;
        out_t *oss = (out_t *)out.s;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((found >> i) & 1u)) continue;
            const unsigned long long gi = st_base + s_cw[i * NW + wv] + lpre[i];
            if (gi < (unsigned long long)out.cap) {
                oss[gi] = (out_t)P[i];
                if (okk) okk[gi] = (out_t)K[i];
            }
        }
        __syncthreads();   // s_cw / st_base reused by the next tile
    }
}

// The key of row `row` alone (k_probe_lookup, k_probe_mark: no payload column is read).
template <int FORM>
__device__ __forceinline__ unsigned long long load_key(const SrcDev &s, long long row);
template <>
__device__ __forceinline__ unsigned long long load_key<kCols64>(const SrcDev &s, long long row) {
    return ((const unsigned long long *)s.key)[row];
}
template <>
__device__ __forceinline__ unsigned long long load_key<kPacked64>(const SrcDev &s, long long row) {
    return ((const unsigned long long *)s.key)[2 * row];
}
template <>
__device__ __forceinline__ unsigned long long load_key<kCol32>(const SrcDev &s, long long row) {
    return (unsigned long long)(unsigned)((const int *)s.key)[row];
}

// ------------------------------------------------------------------ lookup probe
// Positional lookup (SINGLE / MARK join): for S row j, out.r[j] = the smallest
// (signed) payload among the R rows with its key, or null_pay; cnt[j] = how
// many there are.  k_probe_exists' shape -- 2048-row tiles, every row's first
// slot load issued before any is resolved, TableView -- over S's KEYS alone
// (load_key), without its compaction: row slot i of thread x stores to its own
// row index, so there are no ballots, no scan and no cursor, and every store
// instruction writes one contiguous run per wave.  The chain walk ends at the
// first equal key when the build's repeat flag (meta[1]) is clear, else it
// goes on to EMPTY, counting and taking the minimum.  A wide INT64_MIN probe
// key answers from the side list: its count is meta[0] and its minimum is
// taken once per workgroup (only when the list holds a row).  Either output
// may be null (wave-uniform branches).  The rows with a partner are summed per
// lane and added to out.counter once per workgroup, after its last tile.
// LDS: the next tile's keys are loaded ahead (see load_keys below).
template <int L, int FORM, bool LDS>
__global__ __launch_bounds__(kBlock) void k_probe_lookup(TableDev t, SrcDev src, OutDev out, int *cnt,
                                                         unsigned long long null_pay) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using out_t = typename LY::out_t;
    constexpr int NW = kBlock / 64;
    constexpr long long kMaxPay = 0x7fffffffffffffffll;
    __shared__ long long s_side_min;
    __shared__ unsigned s_hits[NW];
    extern __shared__ ulonglong2 s_tab[];

    const TableView<L, LDS> tab(t, s_tab);
    const bool unique = (__hip_atomic_load(&t.meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull);
    const unsigned long long side_n = L == kWide ? t.meta[0] : 0ull;   // INT64_MIN build rows
    long long side_min = (long long)null_pay;
    if (side_n != 0ull) {   // (uniform)
        if (threadIdx.x == 0) s_side_min = kMaxPay;
        __syncthreads();
        long long m = kMaxPay;
        for (unsigned long long j = threadIdx.x; j < side_n; j += kBlock) {
            const long long p = (long long)t.side[j];
            m = p < m ? p : m;
        }
        atomicMin(&s_side_min, m);
        __syncthreads();
        side_min = s_side_min;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long nt = (unsigned long long)((src.n + kProbeTile - 1) / kProbeTile);
    out_t *orr = (out_t *)out.r;
    unsigned hits = 0;
    // the keys of tile q (bits of the result: the rows the source holds)
    auto load_keys = [&](unsigned long long q, unsigned long long (&K)[kProbeItems]) {
        unsigned valid = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const long long row = (long long)q * kProbeTile + (long long)i * kBlock + threadIdx.x;
            K[i] = 0ull;
            if (row < src.n) {
                valid |= 1u << i;
                K[i] = load_key<FORM>(src, row);
            }
        }
        return valid;
    };
    // LDS: a persistent loop of few waves per CU (the table copies fill the
    // LDS), so the next tile's keys are loaded before this tile's walks and
    // stores -- loads issued behind a tile's stores would wait for them.  A
    // global table runs one workgroup per tile: nothing to load ahead.
    [[maybe_unused]] unsigned long long KN[kProbeItems];
    [[maybe_unused]] unsigned valid_n = 0;
    if constexpr (LDS) {
        if (blockIdx.x < nt) valid_n = load_keys(blockIdx.x, KN);
    }
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long K[kProbeItems], H[kProbeItems];
        long long RP[kProbeItems];
        unsigned C[kProbeItems];
        unsigned valid, walk = 0;
        if constexpr (LDS) {
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) K[i] = KN[i];
            valid = valid_n;
            if (q + gridDim.x < nt) valid_n = load_keys(q + gridDim.x, KN);
        } else {
            valid = load_keys(q, K);
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            C[i] = 0u;
            RP[i] = kMaxPay;
            if (!((valid >> i) & 1u)) continue;
            if (LY::null_key(K[i])) {
                C[i] = (unsigned)side_n;
                RP[i] = side_min;
            } else {
                walk |= 1u << i;
            }
        }
        slot_t S[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            H[i] = slot_of(K[i], t.shift);
            if ((walk >> i) & 1u) S[i] = tab.at(H[i]);
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((walk >> i) & 1u)) continue;
            slot_t sv = S[i];
            unsigned long long hh = H[i];
            while (!LY::empty(sv)) {
                if (LY::key(sv) == K[i]) {
                    const long long p = (long long)LY::pay(sv);
                    RP[i] = p < RP[i] ? p : RP[i];
                    ++C[i];
                    if (unique) break;
                }
                hh = (hh + 1) & t.mask;
                sv = tab.at(hh);
            }
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((valid >> i) & 1u)) continue;
            const long long row = (long long)q * kProbeTile + (long long)i * kBlock + threadIdx.x;
            if (orr) orr[row] = (out_t)(C[i] ? RP[i] : (long long)null_pay);
            if (cnt) cnt[row] = (int)C[i];
            hits += C[i] ? 1u : 0u;
        }
    }
    const unsigned x = wave_incl_add(hits);
    if (lane == 63) s_hits[wv] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += s_hits[w];
        if (sum) atomicAdd(out.counter, sum);
    }
}

// ------------------------------------------------------------------ star probe
// Star probe (hj.h "Star probe"): n probe rows against up to four built tables
// in ONE kernel; the rows every dimension admits are kept in input order with
// each dimension's smallest payload beside them.  k_probe_lookup's tile shape
// -- 2048-row tiles, row slot i of thread x is row q * 2048 + i * 256 + x,
// every row's first slot load of a dimension issued before any is resolved --
// with the dimension loop unrolled (ND) around it.  Each table is read from its
// copy in dynamic LDS (StarDim::lds_off >= 0, made once per workgroup) or from
// global memory: a wave-uniform branch per dimension and tile.  A persistent grid
// strides over the tiles; the next tile's first key column (kStarWrite: its
// result byte) is loaded ahead, as k_probe_lookup's LDS variant does.
//
// MODE kStarDecide: walks the dimensions that can drop a row (INNER, ANTI) in
//   the caller's order.  A row that failed one loads no further key and walks
//   no further table; existence alone decides, so a walk ends at the first
//   equal key whatever the repeat flag says.  Leaves each lane's eight result
//   bits as one byte (bitmap[q * 256 + x], bit i) and the tile's count: the
//   key filter's workspace shape, scanned by exclusive_scan_u64.
// MODE kStarWrite: reads the byte, places the survivors in row order (per-slot
//   wave prefix sums, one (slot, wave) scan per tile) and, for them alone and
//   only for the dimensions whose payload column was passed, loads the key,
//   walks again for the smallest payload (to the first equal key when the
//   table's meta[1] is clear, else on to EMPTY) and stores below cap.  It is
//   launched with one workgroup per tile and no table copy (launch_star).
// kStarWrite and kStarAll drop no row, so they load every walked dimension's
// keys of a tile before the first walk.
// MODE kStarAll: no dimension can drop a row (every kind LEFT), so row j's
//   position is j: one launch stores payloads and row ids positionally below
//   cap and the count n.
// A wide INT64_MIN probe key answers from the side list: it exists when
// meta[0] != 0, and its minimum is taken once per workgroup and dimension.
// Reads the tables, the side lists and meta[0..1]; writes no build state.
enum StarMode : int { kStarDecide = 0, kStarWrite = 1, kStarAll = 2 };
// Teams of kBlock threads per workgroup at most.  A persistent launch runs
// kStarTeams: its table copies fill the LDS, so the workgroups per CU are few,
// and a second team doubles the waves that hide each other's load latency
// behind the same copies.  The write launch runs one (launch_star).
constexpr int kStarTeams = 2;

// A probe key in registers: 64 bits, or the 32 of an i32 column (zero-extended where it meets a slot's key).
template <int L>
using star_key_t = std::conditional_t<L == kWide, unsigned long long, unsigned>;
template <int L>
__device__ __forceinline__ star_key_t<L> star_key(const void *col, long long row) {
    if constexpr (L == kWide) return ((const unsigned long long *)col)[row];
    else return (unsigned)((const int *)col)[row];
}

// One dimension's walk for the rows in `rows` (bits over the lane's row slots)
// whose keys are K: found = the rows with a partner and, MIN, RP = their
// smallest payload.  LDS: the table's copy at dm.lds_off in s_tab is read, else
// dm.t.slots -- a template argument, so that the slot loads are LDS reads and
// global loads (one walk with the pointer selected at run time compiled to
// flat loads); star_walk below takes the wave-uniform branch between the two.
template <int L, bool MIN, bool LDS>
__device__ __forceinline__ unsigned star_walk_t(const StarDim &dm, unsigned rows,
                                                const star_key_t<L> (&K)[kProbeItems], unsigned long long side_n,
                                                long long side_min, bool unique, long long (&RP)[kProbeItems]) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    extern __shared__ ulonglong2 s_tab[];
    const slot_t *sl = LDS ? (const slot_t *)(s_tab + (dm.lds_off >> 4)) : (const slot_t *)dm.t.slots;
    auto at = [&](unsigned long long h) -> slot_t { return sl[h]; };
    unsigned walk = 0, found = 0;
#pragma unroll
    for (int i = 0; i < kProbeItems; ++i) {
        if (!((rows >> i) & 1u)) continue;
        if (LY::null_key(K[i])) {
            if (side_n != 0ull) {
                found |= 1u << i;
                RP[i] = side_min;
            }
        } else {
            walk |= 1u << i;
        }
    }
    slot_t S[kProbeItems];
    unsigned long long H[kProbeItems];
#pragma unroll
    for (int i = 0; i < kProbeItems; ++i) {
        H[i] = slot_of(K[i], dm.t.shift);
        if ((walk >> i) & 1u) S[i] = at(H[i]);
    }
#pragma unroll
    for (int i = 0; i < kProbeItems; ++i) {
        if (!((walk >> i) & 1u)) continue;
        slot_t sv = S[i];
        unsigned long long hh = H[i];
        long long best = 0x7fffffffffffffffll;
        bool f = false;
        while (!LY::empty(sv)) {
            if (LY::key(sv) == K[i]) {
                f = true;
                if (MIN) {
                    const long long p = (long long)LY::pay(sv);
                    best = p < best ? p : best;
                }
                if (!MIN || unique) break;
            }
            hh = (hh + 1) & dm.t.mask;
            sv = at(hh);
        }
        if (f) {
            found |= 1u << i;
            RP[i] = best;
        }
    }
    return found;
}
template <int L, bool MIN>
__device__ __forceinline__ unsigned star_walk(const StarDim &dm, unsigned rows,
                                              const star_key_t<L> (&K)[kProbeItems], unsigned long long side_n,
                                              long long side_min, bool unique, long long (&RP)[kProbeItems]) {
    if (dm.lds_off >= 0) return star_walk_t<L, MIN, true>(dm, rows, K, side_n, side_min, unique, RP);   // (uniform)
    return star_walk_t<L, MIN, false>(dm, rows, K, side_n, side_min, unique, RP);
}

// The skeleton k_star and k_star_agg share.  The one difference between them:
// k_star unrolls its dimension loops over ND and so holds walks, unique, side_n
// and side_min in registers; k_star_agg walks a.order[] with a run-time index
// under #pragma unroll 1 and therefore keeps them in LDS.
//
// The workgroup's copy of dm's table into s_tab at dm.lds_off, when the host planned one (it plans a copy only for
// a dimension the launch walks).
template <int L>
__device__ __forceinline__ void star_copy_table(const StarDim &dm) {
    extern __shared__ ulonglong2 s_tab[];
    if (dm.lds_off >= 0) {
        ulonglong2 *dst = s_tab + (dm.lds_off >> 4);
        const unsigned long long n16 = (dm.t.mask + 1) * sizeof(typename Lay<L>::slot_t) / 16;
        const ulonglong2 *g16 = (const ulonglong2 *)dm.t.slots;
        for (unsigned long long j = threadIdx.x; j < n16; j += blockDim.x) dst[j] = g16[j];
    }
}
// The workgroup's minimum over a side list of side_n payloads into *slot (LDS, preset to the largest payload).
__device__ __forceinline__ void star_side_min(const TableDev &t, unsigned long long side_n, long long *slot) {
    long long m = 0x7fffffffffffffffll;
    for (unsigned long long j = threadIdx.x; j < side_n; j += blockDim.x) {
        const long long p = (long long)t.side[j];
        m = p < m ? p : m;
    }
    atomicMin(slot, m);
}
// Tile geometry: the row of thread tid's slot i in tile q, and its slots of tile q below n.
__device__ __forceinline__ long long star_row(unsigned long long q, int i, int tid) {
    return (long long)q * kProbeTile + (long long)i * kBlock + tid;
}
__device__ __forceinline__ unsigned star_valid(unsigned long long q, int tid, long long n) {
    unsigned v = 0;
#pragma unroll
    for (int i = 0; i < kProbeItems; ++i) v |= star_row(q, i, tid) < n ? 1u << i : 0u;
    return v;
}
// A column's keys of tile q for the slots in `rows`.  The column is a pointer (k_star_agg) or the dimension whose
// key column it is (k_star), and the row comes from the kernel's row_of, a lambda over star_row that holds tid by
// reference: dm->key and tid are then read per slot, inside the slot's branch, which is what the kernels' own
// loops did.  Handed over by value they are read once ahead of the eight branches, the column's base address is
// kept live across them, and the kernels' register counts and spills move (some occupancies with them).
__device__ __forceinline__ const void *star_col(const void *col) { return col; }
__device__ __forceinline__ const void *star_col(const StarDim *dm) { return dm->key; }
template <int L, class Col, class Row>
__device__ __forceinline__ void star_load_keys(Col col, unsigned long long q, unsigned rows,
                                               star_key_t<L> (&K)[kProbeItems], const Row &row_of) {
#pragma unroll
    for (int i = 0; i < kProbeItems; ++i) K[i] = (rows >> i) & 1u ? star_key<L>(star_col(col), row_of(q, i)) : star_key_t<L>(0);
}
// A team = kBlock threads = one tile at a time; the teams of a workgroup share the table copies.  They take tiles
// qb .. qb + teams - 1 together, qb from first() on in steps of step(), the grid's teams: every team of a workgroup
// runs the same number of steps (its barriers), a team past the last tile an empty one.
struct StarTeam {
    int tid, team, teams;
    __device__ __forceinline__ unsigned long long first() const { return (unsigned long long)blockIdx.x * teams; }
    __device__ __forceinline__ unsigned long long step() const { return (unsigned long long)gridDim.x * teams; }
};
__device__ __forceinline__ StarTeam star_team() {
    return {(int)(threadIdx.x & (kBlock - 1)), (int)(threadIdx.x / kBlock), (int)(blockDim.x / kBlock)};
}

template <int L, int ND, int MODE>
__global__ __launch_bounds__(kBlock * kStarTeams) void k_star(StarArgs a) {
    using LY = Lay<L>;
    using out_t = typename LY::out_t;
    constexpr int NW = kBlock / 64;
    constexpr long long kMaxPay = 0x7fffffffffffffffll;
    __shared__ long long s_side_min[kStarMaxDims];
    __shared__ unsigned s_cw[kProbeItems * NW];

    // the dimensions this launch walks, their tables' copies and side lists
    bool walks[ND], unique[ND];
    unsigned long long side_n[ND];
    long long side_min[ND];
    const StarTeam tm = star_team();
    const int tid = tm.tid, team = tm.team;
    if (threadIdx.x < kStarMaxDims) s_side_min[threadIdx.x] = kMaxPay;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const StarDim &dm = a.d[d];
        walks[d] = MODE == kStarDecide ? dm.kind != kStarLeft : dm.out != nullptr;
        star_copy_table<L>(dm);
        unique[d] = true;
        side_n[d] = 0ull;
        if (walks[d]) {
            if (MODE != kStarDecide)
                unique[d] = __hip_atomic_load(&dm.t.meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull;
            if (L == kWide) side_n[d] = dm.t.meta[0];
        }
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        side_min[d] = kMaxPay;
        if (MODE == kStarDecide || side_n[d] == 0ull) continue;   // (uniform)
        star_side_min(a.d[d].t, side_n[d], &s_side_min[d]);
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < ND; ++d)
        if (MODE != kStarDecide && side_n[d] != 0ull) side_min[d] = s_side_min[d];

    const int lane = tid & 63, wv = tid >> 6;
    const unsigned long long nt = (unsigned long long)((a.n + kProbeTile - 1) / kProbeTile);
    auto row_of = [&](unsigned long long q, int i) { return star_row(q, i, tid); };
    // loaded ahead: the first walked dimension's keys of the next tile (kStarWrite: the next tile's result byte)
    [[maybe_unused]] star_key_t<L> KN[kProbeItems] = {};
    [[maybe_unused]] unsigned byte_n = 0;
    const unsigned long long step = tm.step(), q0 = tm.first() + team;
    if (q0 < nt) {
        if constexpr (MODE == kStarWrite) {
            byte_n = a.bitmap[q0 * kBlock + tid];
        } else {
#pragma unroll
            for (int d = 0; d < ND; ++d)
                if (d == a.first) star_load_keys<L>(&a.d[d], q0, star_valid(q0, tid, a.n), KN, row_of);
        }
    }
    [[maybe_unused]] unsigned par = 0;
    for (unsigned long long qb = tm.first(); qb < nt; qb += step) {
        const unsigned long long q = qb + team, qn = q + step;
        const bool active = q < nt;
        unsigned alive;
        [[maybe_unused]] star_key_t<L> KF[kProbeItems];
        if constexpr (MODE == kStarWrite) {
            alive = active ? byte_n : 0u;
            if (qn < nt) byte_n = a.bitmap[qn * kBlock + tid];
        } else {
            alive = active ? star_valid(q, tid, a.n) : 0u;
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) KF[i] = KN[i];
            if (qn < nt) {
#pragma unroll
                for (int d = 0; d < ND; ++d)
                    if (d == a.first) star_load_keys<L>(&a.d[d], qn, star_valid(qn, tid, a.n), KN, row_of);
            }
        }
        if constexpr (MODE == kStarDecide) {
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                if (!walks[d]) continue;   // (uniform)
                star_key_t<L> K[kProbeItems];
                long long RP[kProbeItems];
                if (d == a.first) {
#pragma unroll
                    for (int i = 0; i < kProbeItems; ++i) K[i] = KF[i];
                } else {
                    star_load_keys<L>(&a.d[d], q, alive, K, row_of);
                }
                const unsigned found = star_walk<L, false>(a.d[d], alive, K, side_n[d], kMaxPay, true, RP);
                alive &= a.d[d].kind == kStarInner ? found : ~found;
            }
            if (active) a.bitmap[q * kBlock + tid] = (unsigned char)alive;
            unsigned c = (unsigned)__popc(alive);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            // one barrier per step: the wave counts alternate between two sets, and nobody reaches the set's
            // next writes (two steps on) before everybody has passed the barrier in between
            unsigned *cw = s_cw + (par * kStarTeams + team) * NW;
            par ^= 1u;
            if (lane == 0) cw[wv] = c;
            __syncthreads();
            if (tid == 0 && active) {
                unsigned s = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) s += cw[w];
                a.tiles[q] = s;
            }
        } else {
            // the rows' output positions: row order = (slot, wave, lane)
            unsigned long long O[kProbeItems];
            if constexpr (MODE == kStarWrite) {
                const unsigned long long tb = a.tiles[q];
                if (tb >= (unsigned long long)a.cap || a.tiles[q + 1] == tb) continue;   // (uniform) nothing of this tile is stored
                unsigned lpre[kProbeItems];
#pragma unroll
                for (int i = 0; i < kProbeItems; ++i) {
                    const unsigned c = (alive >> i) & 1u;
                    const unsigned xs = wave_incl_add(c);
                    lpre[i] = xs - c;
                    if (lane == 63) s_cw[i * NW + wv] = xs;
                }
                __syncthreads();
                if (tid == 0) {
                    unsigned run = 0;
#pragma unroll
                    for (int j = 0; j < kProbeItems * NW; ++j) {
                        const unsigned v = s_cw[j];
                        s_cw[j] = run;
                        run += v;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < kProbeItems; ++i) O[i] = tb + s_cw[i * NW + wv] + lpre[i];
                __syncthreads();   // s_cw is the next tile's too
            } else {
#pragma unroll
                for (int i = 0; i < kProbeItems; ++i) O[i] = (unsigned long long)row_of(q, i);
            }
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i)
                if (O[i] >= (unsigned long long)a.cap) alive &= ~(1u << i);
            if (a.out_row) {
#pragma unroll
                for (int i = 0; i < kProbeItems; ++i)
                    if ((alive >> i) & 1u) ((out_t *)a.out_row)[O[i]] = (out_t)(a.row_base + row_of(q, i));
            }
            // no row is dropped from here on: every dimension's keys are loaded before the first walk
            star_key_t<L> KA[ND][kProbeItems];
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                if (!walks[d]) continue;   // (uniform)
                if (MODE == kStarAll && d == a.first) {
#pragma unroll
                    for (int i = 0; i < kProbeItems; ++i) KA[d][i] = KF[i];
                } else {
                    star_load_keys<L>(&a.d[d], q, alive, KA[d], row_of);
                }
            }
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                if (!walks[d]) continue;   // (uniform)
                long long RP[kProbeItems];
                const unsigned found = star_walk<L, true>(a.d[d], alive, KA[d], side_n[d], side_min[d], unique[d], RP);
                out_t *o = (out_t *)a.d[d].out;
#pragma unroll
                for (int i = 0; i < kProbeItems; ++i)
                    if ((alive >> i) & 1u) o[O[i]] = (out_t)((found >> i) & 1u ? RP[i] : (long long)a.d[d].null_pay);
            }
        }
    }
    if (MODE != kStarDecide && blockIdx.x == 0 && threadIdx.x == 0)
        *a.count = MODE == kStarWrite ? a.tiles[nt] : (unsigned long long)a.n;
    if (MODE == kStarDecide && blockIdx.x == 0 && threadIdx.x == 0) a.tiles[nt] = 0ull;
}

// The star probe's counter without a write launch: the count form (*src, the
// scan's total), n == 0 and the keep-all count form (imm).  A kernel, not a
// memset: see k_counter_clear below.
__global__ __launch_bounds__(64) void k_star_total(const unsigned long long *src, unsigned long long imm,
                                                   unsigned long long *count) {
    if (threadIdx.x == 0) *count = src ? *src : imm;
}

// ------------------------------------------------------------------ as-of probe
// As-of probe: for S row j, out.r[j] = the largest payload <= bound[j] (KIND:
// the smallest >= it; strictly or not -- asof_admits) among the R rows with its
// key, or null_pay.  k_probe_lookup's shape -- 2048-row tiles over S's keys
// alone, every row's first slot load issued before any is resolved, TableView,
// stores at the row's own index, LDS: the next tile loaded ahead -- with one
// more input column, the bounds, read contiguously beside the keys in S's own
// element width (int64, or int32 sign-extended).  The chain walk keeps the
// running best of the payloads the bound admits and a found bit (the best
// alone says nothing: INT64_MIN and INT64_MAX are payloads); it ends at the
// first equal key when the build's repeat flag (meta[1]) is clear, whether or
// not that one qualifies, else it goes on to EMPTY.  A wide INT64_MIN probe
// key answers from the side list, which holds payloads and is scanned by each
// such row itself, every row having its own bound (rare, and all such rows'
// partners sit in that one list).  KIND is a template argument: the walk holds
// one compare and one select.  The rows with a candidate are summed per lane
// and added to out.counter once per workgroup, after its last tile.
// out.counter is zeroed by k_counter_clear in front, not by a memset: as a node
// of a captured build + probe sequence the one-word memset was replayed with a
// stale pattern (the counter came back as 0x2929292929292929 + the count on an
// MI355X; radix_state_clear met the same with its fill).  A kernel's arguments
// travel in its node.
__global__ __launch_bounds__(64) void k_counter_clear(unsigned long long *counter) {
    if (threadIdx.x == 0) *counter = 0ull;
}
template <int L>
__device__ __forceinline__ long long load_bound(const void *b, long long row) {
    if constexpr (L == kWide) return ((const long long *)b)[row];
    else return (long long)((const int *)b)[row];
}
template <int L, int FORM, bool LDS, int KIND>
__global__ __launch_bounds__(kBlock) void k_probe_asof(TableDev t, SrcDev src, const void *bound, OutDev out,
                                                       unsigned long long null_pay) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using out_t = typename LY::out_t;
    constexpr int NW = kBlock / 64;
    __shared__ unsigned s_hits[NW];
    extern __shared__ ulonglong2 s_tab[];

    const TableView<L, LDS> tab(t, s_tab);
    const bool unique = (__hip_atomic_load(&t.meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull);
    const unsigned long long side_n = L == kWide ? t.meta[0] : 0ull;   // INT64_MIN build rows
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long nt = (unsigned long long)((src.n + kProbeTile - 1) / kProbeTile);
    out_t *orr = (out_t *)out.r;
    unsigned hits = 0;
    // the keys and bounds of tile q (bits of the result: the rows the source holds)
    auto load_rows = [&](unsigned long long q, unsigned long long (&K)[kProbeItems], long long (&B)[kProbeItems]) {
        unsigned valid = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const long long row = (long long)q * kProbeTile + (long long)i * kBlock + threadIdx.x;
            K[i] = 0ull;
            B[i] = 0ll;
            if (row < src.n) {
                valid |= 1u << i;
                K[i] = load_key<FORM>(src, row);
                B[i] = load_bound<L>(bound, row);
            }
        }
        return valid;
    };
    // (LDS: the next tile's rows are loaded ahead, as k_probe_lookup's keys are)
    [[maybe_unused]] unsigned long long KN[kProbeItems];
    [[maybe_unused]] long long BN[kProbeItems];
    [[maybe_unused]] unsigned valid_n = 0;
    if constexpr (LDS) {
        if (blockIdx.x < nt) valid_n = load_rows(blockIdx.x, KN, BN);
    }
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long K[kProbeItems], H[kProbeItems];
        long long B[kProbeItems], RP[kProbeItems];
        unsigned valid, walk = 0, found = 0;
        if constexpr (LDS) {
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) {
                K[i] = KN[i];
                B[i] = BN[i];
            }
            valid = valid_n;
            if (q + gridDim.x < nt) valid_n = load_rows(q + gridDim.x, KN, BN);
        } else {
            valid = load_rows(q, K, B);
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            RP[i] = asof_start<KIND>;
            if (!((valid >> i) & 1u)) continue;
            if (LY::null_key(K[i])) {
                for (unsigned long long j = 0; j < side_n; ++j)
                    if (asof_fold<KIND>((long long)t.side[j], B[i], RP[i])) found |= 1u << i;
            } else {
                walk |= 1u << i;
            }
        }
        slot_t S[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            H[i] = slot_of(K[i], t.shift);
            if ((walk >> i) & 1u) S[i] = tab.at(H[i]);
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((walk >> i) & 1u)) continue;
            slot_t sv = S[i];
            unsigned long long hh = H[i];
            while (!LY::empty(sv)) {
                if (LY::key(sv) == K[i]) {
                    if (asof_fold<KIND>((long long)LY::pay(sv), B[i], RP[i])) found |= 1u << i;
                    if (unique) break;
                }
                hh = (hh + 1) & t.mask;
                sv = tab.at(hh);
            }
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((valid >> i) & 1u)) continue;
            const long long row = (long long)q * kProbeTile + (long long)i * kBlock + threadIdx.x;
            const bool f = (found >> i) & 1u;
            orr[row] = (out_t)(f ? RP[i] : (long long)null_pay);
            hits += f ? 1u : 0u;
        }
    }
    const unsigned x = wave_incl_add(hits);
    if (lane == 63) s_hits[wv] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += s_hits[w];
        if (sum) atomicAdd(out.counter, sum);
    }
}

// ------------------------------------------------------------------ expand probe
// Every partner of S row j at out_r[off[j] .. off[j + 1]): a CSR.  Three
// stages share one per-row int32 count column (k_probe_lookup without its
// payload output, or k_join_lookup): the scan below turns the counts into the
// int64 offsets, then a fill kernel (k_probe_expand here, k_join_expand of the
// radix join) walks each row's chain again and stores at off[j] + k.
//
// The scan is reduce-then-scan in three launches, so that no workgroup ever
// waits on another: k_expand_sums (one u64 sum per tile of kExpandTile
// counts), k_expand_scan_sums (ONE workgroup turns the tile sums into their
// exclusive prefix, kExpandFan of them per step with a running carry) and
// k_expand_offsets (each tile's own exclusive scan plus its prefix; the last
// thread of the last tile also writes off[n] = M and the call's counter).
// width(c) = c for the inner kind, max(1, c) for the outer one (outer = 1).
constexpr int kExpandItems = 8;
constexpr int kExpandTile = kBlock * kExpandItems;
constexpr int kExpandFan = 1024;

__device__ __forceinline__ unsigned long long expand_width(int c, unsigned outer) {
    return c ? (unsigned long long)(unsigned)c : (unsigned long long)outer;
}
// exclusive prefix of v over the workgroup's NT threads and its total (all threads call)
template <int NT>
__device__ __forceinline__ unsigned long long block_excl_add64(unsigned long long v, unsigned long long *wsum,
                                                               unsigned long long &total) {
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long inc = wave_incl_add64(v);
    __syncthreads();   // wsum's previous readers are done
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    unsigned long long before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const unsigned long long s = wsum[w];
        before += w < wv ? s : 0ull;
        tot += s;
    }
    total = tot;
    return before + inc - v;
}
// a thread's kExpandItems consecutive widths of tile blockIdx.x (0 past n) and their sum
__device__ __forceinline__ unsigned long long expand_load(const int *cnt, long long n, unsigned outer,
                                                          unsigned long long (&w)[kExpandItems]) {
    const long long base = (long long)blockIdx.x * kExpandTile + (long long)threadIdx.x * kExpandItems;
    unsigned long long s = 0;
    if (base + kExpandItems <= n) {   // (cnt is the context's own buffer: 16-B aligned at every tile's thread base)
        const int4 a = ((const int4 *)(cnt + base))[0], b = ((const int4 *)(cnt + base))[1];
        const int c[kExpandItems] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int i = 0; i < kExpandItems; ++i) w[i] = expand_width(c[i], outer);
    } else {
#pragma unroll
        for (int i = 0; i < kExpandItems; ++i) w[i] = base + i < n ? expand_width(cnt[base + i], outer) : 0ull;
    }
#pragma unroll
    for (int i = 0; i < kExpandItems; ++i) s += w[i];
    return s;
}
__global__ __launch_bounds__(kBlock) void k_expand_sums(const int *cnt, long long n, unsigned outer,
                                                        unsigned long long *sums) {
    __shared__ unsigned long long wsum[kBlock / 64];
    unsigned long long w[kExpandItems], total;
    const unsigned long long s = expand_load(cnt, n, outer, w);
    block_excl_add64<kBlock>(s, wsum, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(kExpandFan) void k_expand_scan_sums(unsigned long long *sums, unsigned long long nt) {
    __shared__ unsigned long long wsum[kExpandFan / 64];
    unsigned long long carry = 0;
    for (unsigned long long b = 0; b < nt; b += kExpandFan) {
        const unsigned long long i = b + threadIdx.x;
        const unsigned long long v = i < nt ? sums[i] : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_excl_add64<kExpandFan>(v, wsum, total);
        if (i < nt) sums[i] = carry + ex;
        carry += total;
    }
}
__global__ __launch_bounds__(kBlock) void k_expand_offsets(const int *cnt, long long n, unsigned outer,
                                                           const unsigned long long *sums, long long *off,
                                                           unsigned long long *count) {
    __shared__ unsigned long long wsum[kBlock / 64];
    unsigned long long w[kExpandItems], total;
    const unsigned long long s = expand_load(cnt, n, outer, w);
    unsigned long long run = sums[blockIdx.x] + block_excl_add64<kBlock>(s, wsum, total);
    const long long base = (long long)blockIdx.x * kExpandTile + (long long)threadIdx.x * kExpandItems;
#pragma unroll
    for (int i = 0; i < kExpandItems; ++i) {
        if (base + i < n) off[base + i] = (long long)run;
        run += w[i];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == kBlock - 1) {   // (rows past n added 0: run is M)
        off[n] = (long long)run;
        *count = run;
    }
}

// The global table's fill: k_probe_lookup's tile shape over S's keys alone --
// 2048-row tiles, every row's first slot load (and its offset) issued before
// any walk, TableView -- where row j walks its chain to EMPTY (to the first
// equal key when the build's repeat flag meta[1] is clear) and stores every
// equal key's payload at pos++, pos starting at off[j], while pos < cap.  A
// wide INT64_MIN probe key copies the side list's meta[0] payloads.  Outer: a
// row that stored nothing writes null_pay.  No cursor, no atomics, no counter:
// every position is a function of the scan.  outer and cap are kernel
// arguments (wave-uniform); only `pos < cap` is a lane's own.
template <int L, int FORM, bool LDS>
__global__ __launch_bounds__(kBlock) void k_probe_expand(TableDev t, SrcDev src, const long long *off, void *out_r,
                                                         unsigned long long cap, unsigned outer,
                                                         unsigned long long null_pay) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using out_t = typename LY::out_t;
    extern __shared__ ulonglong2 s_tab[];

    const TableView<L, LDS> tab(t, s_tab);
    const bool unique = (__hip_atomic_load(&t.meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull);
    const unsigned long long side_n = L == kWide ? t.meta[0] : 0ull;   // INT64_MIN build rows
    out_t *orr = (out_t *)out_r;
    const unsigned long long nt = (unsigned long long)((src.n + kProbeTile - 1) / kProbeTile);
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long K[kProbeItems], H[kProbeItems], P[kProbeItems];
        unsigned valid = 0, walk = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const long long row = (long long)q * kProbeTile + (long long)i * kBlock + threadIdx.x;
            K[i] = 0ull;
            P[i] = 0ull;
            if (row < src.n) {
                valid |= 1u << i;
                K[i] = load_key<FORM>(src, row);
                P[i] = (unsigned long long)off[row];
                if (!LY::null_key(K[i])) walk |= 1u << i;
            }
        }
        slot_t S[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            H[i] = slot_of(K[i], t.shift);
            if ((walk >> i) & 1u) S[i] = tab.at(H[i]);
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((valid >> i) & 1u)) continue;
            unsigned long long pos = P[i];
            if ((walk >> i) & 1u) {
                slot_t sv = S[i];
                unsigned long long hh = H[i];
                while (!LY::empty(sv)) {
                    if (LY::key(sv) == K[i]) {
                        if (pos < cap) orr[pos] = (out_t)LY::pay(sv);
                        ++pos;
                        if (unique) break;
                    }
                    hh = (hh + 1) & t.mask;
                    sv = tab.at(hh);
                }
            } else {
                for (unsigned long long j = 0; j < side_n; ++j, ++pos)
                    if (pos < cap) orr[pos] = (out_t)t.side[j];
            }
            if (outer && pos == P[i] && pos < cap) orr[pos] = (out_t)null_pay;
        }
    }
}

// ------------------------------------------------------------------ outer probe
// Probe-side outer join (LEFT OUTER with S on the left): every pair of the
// inner join, plus (null_pay, S.pay) for every S row without a partner.
// k_probe's shape and its two paths -- 2048-row tiles, every row's first slot
// load issued before any is resolved, TableView, one cursor add per tile; a
// tile with an INT64_MIN probe key or (repeated build keys) a row with more
// than one match goes to the general path, k_probe_slow with the null value,
// which emits the null row when a walk ends without a match.
// What the fast path does not need is k_probe's compaction: every valid row
// of a tile that stays here emits exactly one element, (RP, P) or (null, P),
// the valid rows are a prefix of the tile, so the tile's count is known from
// src.n alone and row slot i of thread x writes at cursor + i * kBlock + x:
// no ballots, no scan, whole-wave contiguous stores.  out.cap == 0 is the
// count-only form (the walks still run when build keys repeat: they decide
// which tiles leave).  The chain walks are k_probe's, statement for statement.
// MARKS: as k_probe's (the full outer probe).
template <int L, int FORM, bool LDS, typename... MARKS>
__global__ __launch_bounds__(kBlock) void k_probe_outer(TableDev t, SrcDev src, OutDev out, unsigned *slow,
                                                        unsigned long long slow_cap, unsigned long long null_pay,
                                                        MARKS... marks) {
    static_assert(sizeof...(MARKS) <= 1, "at most the mark bitmap");
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using out_t = typename LY::out_t;
    __shared__ unsigned long long st_base;
    extern __shared__ ulonglong2 s_tab[];

    const TableView<L, LDS> tab(t, s_tab);
    const bool unique = (__hip_atomic_load(&t.meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull);
    const unsigned long long nt = (unsigned long long)((src.n + kProbeTile - 1) / kProbeTile);
    // (as in k_probe: a tile handed on leaves by `continue` past the closing
    // barrier, and nothing before the last `continue` touches st_base)
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long K[kProbeItems], P[kProbeItems];
        bool V[kProbeItems];
        bool has_null = false;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            Tuple tp{0ull, 0ull};
            V[i] = probe_row<L, FORM>(src, q, i, tp);
            K[i] = tp.k;
            P[i] = tp.p;
            has_null |= V[i] && LY::null_key(K[i]);
        }
        auto to_slow = [&]() {
            if (threadIdx.x == 0) {
                const unsigned long long j = atomicAdd(&t.meta[3], 1ull);
                if (j < slow_cap) slow[j] = (unsigned)q;   // (sized so it always is; else k_probe_slow flags the count)
            }
        };
        if (__syncthreads_or(has_null ? 1 : 0)) {
            to_slow();
            continue;
        }
        slot_t S[kProbeItems];
        unsigned long long H[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            H[i] = slot_of(K[i], t.shift);
            if (V[i]) S[i] = tab.at(H[i]);
        }
        unsigned found = 0;
        unsigned long long RP[kProbeItems];
        [[maybe_unused]] unsigned long long MH[kProbeItems];   // MARKS: the matched slots
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            RP[i] = null_pay;
            if constexpr (sizeof...(MARKS) == 1) MH[i] = 0;
            if (!V[i]) continue;
            slot_t sv = S[i];
            unsigned long long hh = H[i];
            while (!LY::empty(sv) && LY::key(sv) != K[i]) {
                hh = (hh + 1) & t.mask;
                sv = tab.at(hh);
            }
            if (!LY::empty(sv)) {
                found |= 1u << i;
                RP[i] = LY::pay(sv);
                if constexpr (sizeof...(MARKS) == 1) MH[i] = hh;
            }
        }
        if (!unique) {
            // repeated build keys: a matched row walks on to EMPTY; a second
            // copy of its key sends the tile to the general path
            bool multi = false;
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) {
                if (!((found >> i) & 1u)) continue;
                unsigned long long hh = slot_of(K[i], t.shift);
                slot_t sv = tab.at(hh);
                while (!LY::empty(sv) && LY::key(sv) != K[i]) {   // (back to the first copy)
                    hh = (hh + 1) & t.mask;
                    sv = tab.at(hh);
                }
                hh = (hh + 1) & t.mask;
                sv = tab.at(hh);
                while (!LY::empty(sv) && !multi) {
                    multi = LY::key(sv) == K[i];
                    hh = (hh + 1) & t.mask;
                    sv = tab.at(hh);
                }
            }
            if (__syncthreads_or(multi ? 1 : 0)) {
                to_slow();
                continue;
            }
        }
        if constexpr (sizeof...(MARKS) == 1) mark_found((marks, ...), found, MH);
        // the tile's valid rows: [q * kProbeTile, min(src.n, (q + 1) * kProbeTile)), never none
        const unsigned long long left = (unsigned long long)src.n - q * kProbeTile;
        const unsigned long long rows = left < (unsigned long long)kProbeTile ? left : (unsigned long long)kProbeTile;
        if (threadIdx.x == 0) st_base = atomicAdd(out.counter, rows);
        if (out.cap != 0) {   // (uniform)
            __syncthreads();
            out_t *orr = (out_t *)out.r;
            out_t *oss = (out_t *)out.s;
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) {
                if (!V[i]) continue;
                const unsigned long long gi = st_base + (unsigned long long)(i * kBlock) + threadIdx.x;
                if (gi < (unsigned long long)out.cap) {
                    orr[gi] = (out_t)RP[i];
                    oss[gi] = (out_t)P[i];
                }
            }
            __syncthreads();   // st_base reused by the next tile
        }
    }
}

// ------------------------------------------------------------------ build-side outer probe
// RIGHT / FULL OUTER with S on the left: behind the pairs (k_probe) or the
// pairs and S's null rows (k_probe_outer), the R rows no S row of this call
// matched come out as (R.pay, null_s), found through a mark bitmap, one bit
// per slot, zeroed on the stream before every call:
//   stage 1          k_probe / k_probe_outer with the MARKS pack: a tile that
//                    stays on the fast path marks the slots its rows matched
//                    where the walk found them (no second read of S, no
//                    second walk);
//   k_probe_mark     the tiles stage 1 handed to the general path (the slow
//                    list: an INT64_MIN probe key, or a multi-match row):
//                    every S key walks its chain and sets the bit of each
//                    slot that holds it;
//   k_emit_unmatched scans the slot array and emits occupied, unmarked slots.
// marks[words] (the word behind the bitmap) is "an S row held INT64_MIN":
// the side list's rows are matched iff it is set.
//
// k_probe_mark: k_probe_exists' shape -- 2048-row tiles, a lane's 8 first-slot
// loads in flight before any is resolved -- over S's KEYS alone (load_key: no
// payload column is read), persistent workgroups over slow[0 .. meta[3]) as
// k_probe_slow's.  Bits are set through mark_first.
// Duplicate-free build (meta[1] == 0): the walk ends at the first equal key.
// Repeated build keys: every copy must end up marked.  All walks for key k
// start at the same slot and pass k's copies c1, c2, ... in the same order.
// A walk that is FIRST to set a copy's bit (its atomic OR returned the bit
// clear) goes on towards EMPTY; a walk that finds a copy's bit already set
// (by the read, or by the OR's return value) stops there.  Why every copy is
// still marked: the bit of copy c_i can only be set by a walk for k, and the
// walk that set it first does not stop at c_i, so it reaches c_{i+1} and
// either sets that bit first and goes on, or finds it set by another walk
// that, by the same rule, went on.  By induction from c1 (the first walk to
// reach it sets it) every copy up to EMPTY is marked when the kernel ends,
// and k_emit_unmatched is a later launch on the stream.  A hot build key of
// c copies is thus walked to its end once per first-setter, not once per S row.
// (Stage 1's fast path never sets a bit of a repeated key: a row matching one
// sends its tile here.)
template <int L, int FORM>
__global__ __launch_bounds__(kBlock) void k_probe_mark(TableDev t, SrcDev src, unsigned *marks,
                                                       unsigned long long words, const unsigned *slow,
                                                       unsigned long long slow_cap) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    const slot_t *sl = (const slot_t *)t.slots;
    const bool unique = (__hip_atomic_load(&t.meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull);
    // (a slow list too short is flagged in the count by k_probe_slow)
    const unsigned long long nt = t.meta[3] < slow_cap ? t.meta[3] : slow_cap;
    for (unsigned long long j = blockIdx.x; j < nt; j += gridDim.x) {
        const unsigned long long q = slow[j];
        unsigned long long K[kProbeItems], H[kProbeItems];
        unsigned walk = 0;
        bool has_null = false;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const long long row = (long long)q * kProbeTile + (long long)i * kBlock + threadIdx.x;
            K[i] = 0ull;
            if (row < src.n) {
                K[i] = load_key<FORM>(src, row);
                if (LY::null_key(K[i])) has_null = true;
                else walk |= 1u << i;
            }
        }
        slot_t S[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            H[i] = slot_of(K[i], t.shift);
            if ((walk >> i) & 1u) S[i] = sl[H[i]];
        }
        if constexpr (L == kWide) {
            // (read first: one store per call and lane at most, none once the word is set)
            if (has_null && __hip_atomic_load(&marks[words], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
                __hip_atomic_store(&marks[words], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((walk >> i) & 1u)) continue;
            slot_t sv = S[i];
            unsigned long long hh = H[i];
            while (!LY::empty(sv)) {
                // unique: the only copy; else only the first setter goes on (see above)
                if (LY::key(sv) == K[i] && (!mark_first(marks, hh) || unique)) break;
                hh = (hh + 1) & t.mask;
                sv = sl[hh];
            }
        }
    }
}

// k_emit_unmatched: 2048-slot tiles of the slot array (wide: one 16-B load
// per slot), the mark word of a slot read beside it (a wave's 64 slots share
// two words); occupied and unmarked slots are compacted with wave ballots in
// row-slot-major order after ONE cursor add per tile (k_probe_exists'
// compaction) and written as (pay, null_s), each element under out.cap;
// out.cap == 0 counts only (uniform).  Wide: workgroup 0 then appends the side
// list's payloads when no S row held INT64_MIN.
template <int L>
__global__ __launch_bounds__(kBlock) void k_emit_unmatched(TableDev t, OutDev out, const unsigned *marks,
                                                           unsigned long long words, unsigned long long null_s) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using out_t = typename LY::out_t;
    constexpr int NW = kBlock / 64;
    __shared__ unsigned long long st_base;
    __shared__ unsigned s_cw[kProbeItems * NW];
    const slot_t *sl = (const slot_t *)t.slots;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long cap = t.mask + 1ull;
    const unsigned long long nt = (cap + kProbeTile - 1) / kProbeTile;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    out_t *orr = (out_t *)out.r;
    out_t *oss = (out_t *)out.s;
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long P[kProbeItems];
        unsigned found = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const unsigned long long j = q * kProbeTile + (unsigned long long)(i * kBlock) + threadIdx.x;
            P[i] = 0ull;
            if (j < cap) {
                const slot_t sv = sl[j];
                const unsigned m = marks[j >> 5];
                P[i] = LY::pay(sv);
                if (!LY::empty(sv) && !((m >> (unsigned)(j & 31ull)) & 1u)) found |= 1u << i;
            }
        }
        unsigned lpre[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const unsigned long long bal = __ballot((found >> i) & 1u);
            lpre[i] = (unsigned)__popcll(bal & lt);
            if (lane == 0) s_cw[i * NW + wv] = (unsigned)__popcll(bal);
        }
        __syncthreads();
        if (wv == 0) {   // exclusive scan of the kProbeItems * NW runs (<= 64)
            static_assert(kProbeItems * NW <= 64, "one lane per run");
            const unsigned v = lane < kProbeItems * NW ? s_cw[lane] : 0u;
            const unsigned x = wave_incl_add(v);
            if (lane < kProbeItems * NW) s_cw[lane] = x - v;
            if (lane == 63) st_base = x ? atomicAdd(out.counter, (unsigned long long)x) : 0ull;
        }
        __syncthreads();
        if (out.cap != 0) {   // (uniform)
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) {
                if (!((found >> i) & 1u)) continue;
                const unsigned long long gi = st_base + s_cw[i * NW + wv] + lpre[i];
                if (gi < (unsigned long long)out.cap) {
                    orr[gi] = (out_t)P[i];
                    oss[gi] = (out_t)null_s;
                }
            }
        }
        __syncthreads();   // s_cw / st_base reused by the next tile
    }
    if constexpr (L == kWide) {
        if (blockIdx.x != 0) return;
        const unsigned long long ns = t.meta[0];
        if (ns == 0ull || marks[words] != 0u) return;   // (uniform)
        if (threadIdx.x == 0) st_base = atomicAdd(out.counter, ns);
        __syncthreads();
        if (out.cap == 0) return;
        for (unsigned long long j = threadIdx.x; j < ns; j += kBlock) {
            const unsigned long long gi = st_base + j;
            if (gi < (unsigned long long)out.cap) {
                orr[gi] = (out_t)t.side[j];
                oss[gi] = (out_t)null_s;
            }
        }
    }
}

// ------------------------------------------------------------------ group probe
// Join, then aggregate per build row: per-slot accumulators beside the slot
// array (GroupAcc: separate arrays of slots + 1 entries, so an aggregate nobody
// asked for does not exist; the last entry is the wide side list's), three
// launches and no scratch.
//   k_group_init   the fill: count and sum 0, min the largest and max the
//                  smallest value of the type.
//   k_probe_group  k_probe_exists' shape over S's keys and values: each row
//                  walks to the FIRST slot of its chain holding its key and
//                  issues its atomics there (results unused: non-returning),
//                  only for the aggregates asked for.  A row without a partner
//                  does nothing.  A wide INT64_MIN key adds into the last
//                  entry when the side list holds a row.
//   k_emit_groups  k_emit_unmatched's shape over the slots: an occupied slot
//                  finds the accumulators of its key's first copy -- itself
//                  when the repeat flag meta[1] is clear, else the first equal
//                  key on the walk from the key's home slot -- applies the
//                  kind and writes the columns passed; workgroup 0 appends the
//                  side list's rows with the last entry's aggregates.
// Element types: Lay<L>::out_t for r, count, min and max, int64 for the sum.
template <int L>
struct GroupTypes;
template <>
struct GroupTypes<kWide> {
    using cnt_t = unsigned long long;
    using ext_t = long long;
    static constexpr ext_t kMin = (ext_t)0x8000000000000000ull, kMax = 0x7fffffffffffffffll;
};
template <>
struct GroupTypes<kNarrow> {
    using cnt_t = unsigned;
    using ext_t = int;
    static constexpr ext_t kMin = (ext_t)0x80000000u, kMax = 0x7fffffff;
};

template <int L>
__device__ __forceinline__ void group_fill(const GroupAcc &acc, unsigned long long n) {
    using GT = GroupTypes<L>;
    typename GT::cnt_t *cnt = (typename GT::cnt_t *)acc.cnt;
    typename GT::ext_t *mn = (typename GT::ext_t *)acc.mn, *mx = (typename GT::ext_t *)acc.mx;
    const unsigned long long stride = (unsigned long long)gridDim.x * kBlock;
    for (unsigned long long j = (unsigned long long)blockIdx.x * kBlock + threadIdx.x; j < n; j += stride) {
        cnt[j] = 0;
        if (acc.sum) acc.sum[j] = 0ull;
        if (mn) mn[j] = GT::kMax;
        if (mx) mx[j] = GT::kMin;
    }
}
template <int L>
__global__ __launch_bounds__(kBlock) void k_group_init(GroupAcc acc, unsigned long long n) {
    group_fill<L>(acc, n);
}

template <int L, int FORM>
__global__ __launch_bounds__(kBlock) void k_probe_group(TableDev t, SrcDev src, GroupAcc acc) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using GT = GroupTypes<L>;
    typename GT::cnt_t *cnt = (typename GT::cnt_t *)acc.cnt;
    typename GT::ext_t *mn = (typename GT::ext_t *)acc.mn, *mx = (typename GT::ext_t *)acc.mx;
    const slot_t *sl = (const slot_t *)t.slots;
    const bool vals = acc.sum || mn || mx;   // (uniform) else only the key is read
    const bool side_rows = L == kWide && t.meta[0] != 0ull;   // the build side holds an INT64_MIN key
    const unsigned long long nt = (unsigned long long)((src.n + kProbeTile - 1) / kProbeTile);
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long K[kProbeItems], V[kProbeItems], H[kProbeItems];
        unsigned walk = 0, found = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const long long row = (long long)q * kProbeTile + (long long)i * kBlock + threadIdx.x;
            K[i] = V[i] = 0ull;
            if (row < src.n) {
                if (vals) {
                    const Tuple tp = load_src<FORM>(src, row);
                    K[i] = tp.k;
                    V[i] = tp.p;
                } else {
                    K[i] = load_key<FORM>(src, row);
                }
                if (LY::null_key(K[i])) found |= side_rows ? 1u << i : 0u;
                else walk |= 1u << i;
            }
        }
        slot_t S[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            H[i] = LY::null_key(K[i]) ? t.mask + 1ull : slot_of(K[i], t.shift);
            if ((walk >> i) & 1u) S[i] = sl[H[i]];
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((walk >> i) & 1u)) continue;
            slot_t sv = S[i];
            unsigned long long hh = H[i];
            while (!LY::empty(sv) && LY::key(sv) != K[i]) {
                hh = (hh + 1) & t.mask;
                sv = sl[hh];
            }
            H[i] = hh;
            if (!LY::empty(sv)) found |= 1u << i;
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((found >> i) & 1u)) continue;
            atomicAdd(cnt + H[i], (typename GT::cnt_t)1);
            if (acc.sum) atomicAdd(acc.sum + H[i], V[i]);
            if (mn) atomicMin(mn + H[i], (typename GT::ext_t)V[i]);
            if (mx) atomicMax(mx + H[i], (typename GT::ext_t)V[i]);
        }
    }
}

template <int L>
__global__ __launch_bounds__(kBlock) void k_emit_groups(TableDev t, GroupAcc acc, GroupOut out) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using out_t = typename LY::out_t;
    using GT = GroupTypes<L>;
    constexpr int NW = kBlock / 64;
    __shared__ unsigned long long st_base;
    __shared__ unsigned s_cw[kProbeItems * NW];
    const typename GT::cnt_t *cnt = (const typename GT::cnt_t *)acc.cnt;
    const typename GT::ext_t *mn = (const typename GT::ext_t *)acc.mn, *mx = (const typename GT::ext_t *)acc.mx;
    const slot_t *sl = (const slot_t *)t.slots;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long cap = t.mask + 1ull;
    const unsigned long long nt = (cap + kProbeTile - 1) / kProbeTile;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    const bool unique = (__hip_atomic_load(&t.meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull);
    out_t *orr = (out_t *)out.r, *ocnt = (out_t *)out.cnt, *omin = (out_t *)out.mn, *omax = (out_t *)out.mx;
    long long *osum = (long long *)out.sum;
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long P[kProbeItems], F[kProbeItems];
        typename GT::cnt_t C[kProbeItems];
        unsigned found = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const unsigned long long j = q * kProbeTile + (unsigned long long)(i * kBlock) + threadIdx.x;
            P[i] = 0ull;
            F[i] = 0ull;
            C[i] = 0;
            if (j < cap) {
                const slot_t sv = sl[j];
                if (!LY::empty(sv)) {
                    P[i] = LY::pay(sv);
                    unsigned long long f = j;
                    if (!unique) {   // the first copy of the key: the walk from its home slot
                        const unsigned long long k = LY::key(sv);
                        f = slot_of(k, t.shift);
                        while (f != j && LY::key(sl[f]) != k) f = (f + 1) & t.mask;
                    }
                    F[i] = f;
                    C[i] = cnt[f];
                    if (out.all || C[i] != 0) found |= 1u << i;
                }
            }
        }
        unsigned lpre[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const unsigned long long bal = __ballot((found >> i) & 1u);
            lpre[i] = (unsigned)__popcll(bal & lt);
            if (lane == 0) s_cw[i * NW + wv] = (unsigned)__popcll(bal);
        }
        __syncthreads();
        if (wv == 0) {   // exclusive scan of the kProbeItems * NW runs (<= 64)
            static_assert(kProbeItems * NW <= 64, "one lane per run");
            const unsigned v = lane < kProbeItems * NW ? s_cw[lane] : 0u;
            const unsigned x = wave_incl_add(v);
            if (lane < kProbeItems * NW) s_cw[lane] = x - v;
            if (lane == 63) st_base = x ? atomicAdd(out.counter, (unsigned long long)x) : 0ull;
        }
        __syncthreads();
        if (out.cap != 0) {   // (uniform)
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) {
                if (!((found >> i) & 1u)) continue;
                const unsigned long long gi = st_base + s_cw[i * NW + wv] + lpre[i];
                if (gi < (unsigned long long)out.cap) {
                    const bool some = C[i] != 0;
                    if (orr) orr[gi] = (out_t)P[i];
                    if (ocnt) ocnt[gi] = (out_t)C[i];
                    if (osum) osum[gi] = (long long)acc.sum[F[i]];
                    if (omin) omin[gi] = some ? (out_t)mn[F[i]] : (out_t)out.null_val;
                    if (omax) omax[gi] = some ? (out_t)mx[F[i]] : (out_t)out.null_val;
                }
            }
        }
        __syncthreads();   // s_cw / st_base reused by the next tile
    }
    if constexpr (L == kWide) {
        if (blockIdx.x != 0) return;
        const unsigned long long ns = t.meta[0];
        if (ns == 0ull) return;   // (uniform)
        const typename GT::cnt_t c = cnt[cap];
        if (!out.all && c == 0) return;
        if (threadIdx.x == 0) st_base = atomicAdd(out.counter, ns);
        __syncthreads();
        if (out.cap == 0) return;
        for (unsigned long long j = threadIdx.x; j < ns; j += kBlock) {
            const unsigned long long gi = st_base + j;
            if (gi < (unsigned long long)out.cap) {
                if (orr) orr[gi] = (out_t)t.side[j];
                if (ocnt) ocnt[gi] = (out_t)c;
                if (osum) osum[gi] = (long long)acc.sum[cap];
                if (omin) omin[gi] = c ? (out_t)mn[cap] : (out_t)out.null_val;
                if (omax) omax[gi] = c ? (out_t)mx[cap] : (out_t)out.null_val;
            }
        }
    }
}

// ------------------------------------------------------------------ hash aggregate
// GROUP BY key over one relation (launch_aggregate): the table holds each
// distinct key once and the group probe's accumulators (GroupAcc) sit beside
// it.  The table's fill and k_aggregate_init (k_group_init's fill, and the
// output counter's zero: a captured one-word memset node in front of these
// launches was replayed with a stale byte pattern at 70 000 rows; the cause is
// not known; a kernel's arguments travel in its node), then
//   k_aggregate       persistent workgroups over 2048-row tiles.  A tile is
//                     first collapsed in a kAggSlots-slot LDS table (key,
//                     count and the partials asked for: LDS atomics behind a
//                     CAS that ends at EMPTY or at the key itself, at most
//                     kAggWalk steps from the key's home slot -- slots are
//                     never freed inside a tile, so every row of a key takes
//                     the same way).  A row whose walk ends on neither goes to
//                     the global table itself.  Every occupied LDS slot is
//                     then flushed once: insert-or-find in the global table (a
//                     CAS on the slot's key word; narrow: key << 32, which is
//                     never the all-ones EMPTY word, so -1 is a key like any
//                     other) and one non-returning atomic per accumulator that
//                     carries the tile's partial.  A hot key costs one global
//                     atomic per tile instead of one per row.  Wide INT64_MIN
//                     keys (the table's EMPTY word) are collapsed in LDS words
//                     of their own and flushed into the last entry.
//   k_emit_aggregate  k_emit_groups' scan over the slots, emitting the slot's
//                     key and its own accumulators (no first-copy walk: the
//                     table holds each key once); workgroup 0 appends the
//                     INT64_MIN entry when its count is non-zero.
// 18 KiB of LDS (int64 rows) per workgroup: eight workgroups fit a CU.
constexpr int kAggSlotsLog = 9, kAggSlots = 1 << kAggSlotsLog, kAggWalk = 8;

template <int L>
__global__ __launch_bounds__(kBlock) void k_aggregate_init(GroupAcc acc, unsigned long long n,
                                                           unsigned long long *counter) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *counter = 0ull;
    group_fill<L>(acc, n);
}

// the slot of key K in the global table, claimed if the key is new
template <int L>
__device__ __forceinline__ unsigned long long agg_slot(typename Lay<L>::slot_t *sl, const TableDev &t,
                                                       unsigned long long K) {
    using LY = Lay<L>;
    const unsigned long long w = L == kWide ? K : K << 32;
    unsigned long long h = slot_of(K, t.shift);
    while (true) {
        // (read first: a repeated key finds itself without an atomic)
        unsigned long long old = __hip_atomic_load(LY::word(sl, h), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == LY::kEmptyWord) old = atomicCAS(LY::word(sl, h), LY::kEmptyWord, w);
        if (old == LY::kEmptyWord || old == w) return h;
        h = (h + 1) & t.mask;
    }
}

template <int L>
__device__ __forceinline__ void acc_add(const GroupAcc &acc, unsigned long long h, typename GroupTypes<L>::cnt_t c,
                                        unsigned long long s, typename GroupTypes<L>::ext_t lo,
                                        typename GroupTypes<L>::ext_t hi) {
    using GT = GroupTypes<L>;
    atomicAdd((typename GT::cnt_t *)acc.cnt + h, c);
    if (acc.sum) atomicAdd(acc.sum + h, s);
    if (acc.mn) atomicMin((typename GT::ext_t *)acc.mn + h, lo);
    if (acc.mx) atomicMax((typename GT::ext_t *)acc.mx + h, hi);
}

// One tile's collapse table in LDS, shared by k_aggregate and k_star_agg: keys,
// counts and the partials asked for (AggWant), and the wide INT64_MIN key's
// words of their own (n_*).  agg_tile_clear, a barrier, agg_tile_add per row, a
// barrier, agg_tile_flush, a barrier.
template <int L>
struct AggTile {
    using ext_t = typename GroupTypes<L>::ext_t;
    static constexpr unsigned long long kE = L == kWide ? kEmptyKey64 : ~0ull;   // (a zero-extended i32 key is never all ones)
    unsigned long long key[kAggSlots];
    unsigned long long sum[kAggSlots];
    ext_t mn[kAggSlots], mx[kAggSlots];
    unsigned cnt[kAggSlots];
    unsigned long long n_sum;
    ext_t n_min, n_max;
    unsigned n_cnt;
};
struct AggWant {
    bool sum, mn, mx;
};

template <int L>
__device__ __forceinline__ void agg_tile_clear(AggTile<L> &lt, AggWant w, int tid, int nthreads) {
    using GT = GroupTypes<L>;
    for (int j = tid; j < kAggSlots; j += nthreads) {
        lt.key[j] = AggTile<L>::kE;
        lt.cnt[j] = 0u;
        if (w.sum) lt.sum[j] = 0ull;
        if (w.mn) lt.mn[j] = GT::kMax;
        if (w.mx) lt.mx[j] = GT::kMin;
    }
    if (tid == 0) {
        lt.n_cnt = 0u;
        lt.n_sum = 0ull;
        lt.n_min = GT::kMax;
        lt.n_max = GT::kMin;
    }
}

// one row (K, V) into the tile's table; false: the walk ended on neither EMPTY nor K, the row goes to the global table itself
template <int L>
__device__ __forceinline__ bool agg_tile_add(AggTile<L> &lt, AggWant w, unsigned long long K, unsigned long long V) {
    using ext_t = typename GroupTypes<L>::ext_t;
    constexpr unsigned long long kE = AggTile<L>::kE;
    if (Lay<L>::null_key(K)) {
        atomicAdd(&lt.n_cnt, 1u);
        if (w.sum) atomicAdd(&lt.n_sum, V);
        if (w.mn) atomicMin(&lt.n_min, (ext_t)V);
        if (w.mx) atomicMax(&lt.n_max, (ext_t)V);
        return true;
    }
    unsigned h = (unsigned)slot_of(K, 64 - kAggSlotsLog);
    bool in = false;
    for (int step = 0; step < kAggWalk; ++step) {
        unsigned long long e = __hip_atomic_load(&lt.key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (e == kE) e = atomicCAS(&lt.key[h], kE, K);
        if (e == kE || e == K) {
            in = true;
            break;
        }
        h = (h + 1u) & (unsigned)(kAggSlots - 1);
    }
    if (!in) return false;
    atomicAdd(&lt.cnt[h], 1u);
    if (w.sum) atomicAdd(&lt.sum[h], V);
    if (w.mn) atomicMin(&lt.mn[h], (ext_t)V);
    if (w.mx) atomicMax(&lt.mx[h], (ext_t)V);
    return true;
}

// every occupied slot once into the global accumulators at slot(key) (~0: no slot, the partial is dropped -- the
// bounded insert's overflow); the INT64_MIN words into entry null_entry
template <int L, typename SLOT>
__device__ __forceinline__ void agg_tile_flush(const AggTile<L> &lt, AggWant w, const GroupAcc &acc,
                                               unsigned long long null_entry, int tid, int nthreads, SLOT slot) {
    using GT = GroupTypes<L>;
    using cnt_t = typename GT::cnt_t;
    for (int j = tid; j < kAggSlots; j += nthreads) {
        const unsigned long long k = lt.key[j];
        if (k == AggTile<L>::kE) continue;
        const unsigned long long h = slot(k);
        if (h == ~0ull) continue;
        acc_add<L>(acc, h, (cnt_t)lt.cnt[j], w.sum ? lt.sum[j] : 0ull, w.mn ? lt.mn[j] : GT::kMax,
                   w.mx ? lt.mx[j] : GT::kMin);
    }
    if (L == kWide && tid == 0 && lt.n_cnt != 0u) acc_add<L>(acc, null_entry, (cnt_t)lt.n_cnt, lt.n_sum, lt.n_min, lt.n_max);
}

template <int L, int FORM>
__global__ __launch_bounds__(kBlock) void k_aggregate(TableDev t, SrcDev src, GroupAcc acc) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using GT = GroupTypes<L>;
    using ext_t = typename GT::ext_t;
    using cnt_t = typename GT::cnt_t;
    __shared__ AggTile<L> lt;
    slot_t *sl = (slot_t *)t.slots;
    const AggWant w{acc.sum != nullptr, acc.mn != nullptr, acc.mx != nullptr};
    const bool vals = w.sum || w.mn || w.mx;   // (uniform) else only the key is read
    const unsigned long long nt = (unsigned long long)((src.n + kProbeTile - 1) / kProbeTile);
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long K[kProbeItems], V[kProbeItems];
        unsigned ok = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const long long row = (long long)q * kProbeTile + (long long)i * kBlock + threadIdx.x;
            K[i] = V[i] = 0ull;
            if (row < src.n) {
                if (vals) {
                    const Tuple tp = load_src<FORM>(src, row);
                    K[i] = tp.k;
                    V[i] = tp.p;
                } else {
                    K[i] = load_key<FORM>(src, row);
                }
                ok |= 1u << i;
            }
        }
        agg_tile_clear(lt, w, (int)threadIdx.x, kBlock);
        __syncthreads();
        // ---- the tile's rows into the LDS table
        unsigned direct = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((ok >> i) & 1u)) continue;
            if (!agg_tile_add(lt, w, K[i], V[i])) direct |= 1u << i;
        }
        // ---- the rows the LDS table did not admit: the global table, one by one
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((direct >> i) & 1u)) continue;
            acc_add<L>(acc, agg_slot<L>(sl, t, K[i]), (cnt_t)1, V[i], (ext_t)V[i], (ext_t)V[i]);
        }
        __syncthreads();
        // ---- one flush per occupied LDS slot
        agg_tile_flush(lt, w, acc, t.mask + 1ull, (int)threadIdx.x, kBlock,
                       [&](unsigned long long k) { return agg_slot<L>(sl, t, k); });
        __syncthreads();   // the LDS table is cleared for the next tile
    }
}

template <int L>
__global__ __launch_bounds__(kBlock) void k_emit_aggregate(TableDev t, GroupAcc acc, GroupOut out) {
    using LY = Lay<L>;
    using slot_t = typename LY::slot_t;
    using out_t = typename LY::out_t;
    using GT = GroupTypes<L>;
    constexpr int NW = kBlock / 64;
    __shared__ unsigned long long st_base;
    __shared__ unsigned s_cw[kProbeItems * NW];
    const typename GT::cnt_t *cnt = (const typename GT::cnt_t *)acc.cnt;
    const typename GT::ext_t *mn = (const typename GT::ext_t *)acc.mn, *mx = (const typename GT::ext_t *)acc.mx;
    const slot_t *sl = (const slot_t *)t.slots;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long cap = t.mask + 1ull;
    const unsigned long long nt = (cap + kProbeTile - 1) / kProbeTile;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    out_t *okey = (out_t *)out.r, *ocnt = (out_t *)out.cnt, *omin = (out_t *)out.mn, *omax = (out_t *)out.mx;
    long long *osum = (long long *)out.sum;
    for (unsigned long long q = blockIdx.x; q < nt; q += gridDim.x) {
        unsigned long long KY[kProbeItems];
        unsigned found = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const unsigned long long j = q * kProbeTile + (unsigned long long)(i * kBlock) + threadIdx.x;
            KY[i] = 0ull;
            if (j < cap) {
                const slot_t sv = sl[j];
                if (!LY::empty(sv)) {
                    KY[i] = LY::key(sv);
                    found |= 1u << i;
                }
            }
        }
        unsigned lpre[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            const unsigned long long bal = __ballot((found >> i) & 1u);
            lpre[i] = (unsigned)__popcll(bal & lt);
            if (lane == 0) s_cw[i * NW + wv] = (unsigned)__popcll(bal);
        }
        __syncthreads();
        if (wv == 0) {   // exclusive scan of the kProbeItems * NW runs (<= 64)
            static_assert(kProbeItems * NW <= 64, "one lane per run");
            const unsigned v = lane < kProbeItems * NW ? s_cw[lane] : 0u;
            const unsigned x = wave_incl_add(v);
            if (lane < kProbeItems * NW) s_cw[lane] = x - v;
            if (lane == 63) st_base = x ? atomicAdd(out.counter, (unsigned long long)x) : 0ull;
        }
        __syncthreads();
        if (out.cap != 0) {   // (uniform)
#pragma unroll
            for (int i = 0; i < kProbeItems; ++i) {
                if (!((found >> i) & 1u)) continue;
                const unsigned long long gi = st_base + s_cw[i * NW + wv] + lpre[i];
                if (gi < (unsigned long long)out.cap) {
                    const unsigned long long j = q * kProbeTile + (unsigned long long)(i * kBlock) + threadIdx.x;
                    if (okey) okey[gi] = (out_t)KY[i];
                    if (ocnt) ocnt[gi] = (out_t)cnt[j];
                    if (osum) osum[gi] = (long long)acc.sum[j];
                    if (omin) omin[gi] = (out_t)mn[j];
                    if (omax) omax[gi] = (out_t)mx[j];
                }
            }
        }
        __syncthreads();   // s_cw / st_base reused by the next tile
    }
    if constexpr (L == kWide) {
        if (blockIdx.x != 0 || threadIdx.x != 0) return;
        const typename GT::cnt_t c = cnt[cap];
        if (c == 0) return;
        const unsigned long long gi = atomicAdd(out.counter, 1ull);
        if (gi < (unsigned long long)out.cap) {
            if (okey) okey[gi] = (out_t)kEmptyKey64;
            if (ocnt) ocnt[gi] = (out_t)c;
            if (osum) osum[gi] = (long long)acc.sum[cap];
            if (omin) omin[gi] = (out_t)mn[cap];
            if (omax) omax[gi] = (out_t)mx[cap];
        }
    }
}

// ------------------------------------------------------------------ star aggregate
// GROUP BY over a star probe's survivors in one pass (hj.h "Star aggregate"):
// k_star's tiles, teams, table copies and key prefetch in front of
// k_aggregate's collapse.  Nothing per row reaches memory: no result byte, no
// tile count, no scan and no write launch.  Per tile
//   1. a.order[0 .. a.nwalk) is walked with one loop body (the index is
//      wave-uniform, so the dimension's fields are scalar loads of the kernel
//      arguments and one set of eight keys is live): first the dimensions that
//      can drop a row (INNER, ANTI) in the caller's order, a row that failed
//      one loading no further key, then the grouped LEFT ones, for the
//      survivors alone.  A LEFT dimension outside the key is never read.  A
//      grouped dimension's walk takes the smallest payload (to the first equal
//      key when the table's meta[1] is clear, else on to EMPTY; the side list's
//      minimum for a wide INT64_MIN key); an ungrouped one ends at the first
//      equal key.  Each grouped payload is folded into the row's group key
//      g += (P - gbase) << gshift as it arrives.
//   2. sval is loaded for the survivors, and only when sum / min / max is asked
//      for.
//   3. the survivors are collapsed in the LDS table (AggTile<kWide>: the group
//      table is wide in both forms) and flushed with the bounded insert below.
// The teams of a workgroup share ONE collapse table: beside per-team tables
// (36 KiB) two 64-KiB table copies would no longer fit a CU's 160 KiB, and the
// teams already meet at a barrier every step.  All of a workgroup's threads
// clear and flush it.
// Overflow: bit 63 of *a.counter (zeroed by k_aggregate_init in front) is the
// flag.  agg_slot_bounded sets it when a counted walk of the whole table found
// neither the key nor EMPTY; thread 0 reads it at the start of every tile and
// the workgroup leaves the loop behind the tile's first barrier.  The emit adds
// its counts below the bit and stores nothing, its positions being >= 2^63.

// agg_slot as a COUNTED loop: at most capacity steps, then the flag and ~0.
// Every 256 steps it looks at the flag, so a full table costs one long walk,
// not one per row.
__device__ __forceinline__ unsigned long long agg_slot_bounded(Slot64 *sl, const TableDev &t, unsigned long long K,
                                                               unsigned long long *flag) {
    unsigned long long h = slot_of(K, t.shift);
    for (unsigned long long step = 0; step <= t.mask; ++step) {
        unsigned long long old = __hip_atomic_load(&sl[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == kEmptyKey64) old = atomicCAS(&sl[h].key, kEmptyKey64, K);
        if (old == kEmptyKey64 || old == K) return h;
        if ((step & 255ull) == 255ull &&
            (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 63) != 0ull)
            return ~0ull;
        h = (h + 1) & t.mask;
    }
    atomicOr(flag, 1ull << 63);
    return ~0ull;
}

// FACT (hj.h "Star query"): the fact row's own part of the query, in front of
// and behind the walks; the instantiations without it are the star aggregate's
// code unchanged.  Per tile
//   0. the predicates a.f.pcol[0 .. npreds) in the caller's order, one loop
//      body (one set of eight values live): the column is loaded for the rows
//      still alive and compared as signed int64.  A row that failed loads no
//      further predicate column and no key, and walks no table.
//   1. the walks, over what is left.
//   2. sval, then a.f.vb when the value is an expression, for the survivors.
//   2a. each a.f.fcol for the survivors, folded into the group key.
//   3. unchanged.
// With a predicate the column loaded ahead for the next tile is pcol[0] (every
// row of the tile reads it; the first walked dimension's keys are then read by
// the predicates' survivors alone).  ndims == 0 runs ND = 1 with nwalk == 0 and
// a LEFT, ungrouped dummy dimension the prologue skips.
template <int L, int ND, bool FACT = false>
__global__ __launch_bounds__(kBlock * kStarTeams) void k_star_agg(
    std::conditional_t<FACT, StarQueryArgs, StarAggArgs> a) {
    constexpr long long kMaxPay = 0x7fffffffffffffffll;
    __shared__ AggTile<kWide> lt;
    __shared__ long long s_side_min[kStarMaxDims];
    __shared__ unsigned long long s_side_n[kStarMaxDims];
    __shared__ unsigned s_unique[kStarMaxDims];
    __shared__ unsigned s_stop;
    static_assert(sizeof(AggTile<kWide>) + 128 <= kStarAggStaticLds, "the placement plan's bound on the static LDS");

    const StarTeam tm = star_team();
    const int tid = tm.tid, team = tm.team;
    const AggWant w{a.acc.sum != nullptr, a.acc.mn != nullptr, a.acc.mx != nullptr};
    const bool vals = w.sum || w.mn || w.mx;   // (uniform) else sval is not read
    Slot64 *gsl = (Slot64 *)a.gt.slots;
    if (threadIdx.x < kStarMaxDims) {
        s_side_min[threadIdx.x] = kMaxPay;
        s_side_n[threadIdx.x] = 0ull;
        s_unique[threadIdx.x] = 1u;
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const StarDim &dm = a.d[d];
        const bool grouped = a.gshift[d] >= 0;
        if (dm.kind == kStarLeft && !grouped) continue;   // (uniform) never walked
        star_copy_table<L>(dm);
        const unsigned long long side_n = L == kWide ? dm.t.meta[0] : 0ull;
        if (threadIdx.x == 0) {
            s_side_n[d] = side_n;
            if (grouped)
                s_unique[d] = __hip_atomic_load(&dm.t.meta[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ull ? 1u : 0u;
        }
        if (!grouped || side_n == 0ull) continue;   // (uniform)
        star_side_min(dm.t, side_n, &s_side_min[d]);
    }
    __syncthreads();

    const unsigned long long nt = (unsigned long long)((a.n + kProbeTile - 1) / kProbeTile);
    auto row_of = [&](unsigned long long q, int i) { return star_row(q, i, tid); };
    // loaded ahead: the first walked dimension's keys of the next tile (FACT with a predicate: its first column)
    bool pred_first = false;   // (uniform)
    const void *first_col = a.nwalk > 0 ? a.d[a.order[0]].key : nullptr;
    if constexpr (FACT) {
        pred_first = a.f.npreds > 0;
        if (pred_first) first_col = a.f.pcol[0];
    }
    star_key_t<L> KN[kProbeItems] = {};
    const unsigned long long step = tm.step(), q0 = tm.first() + team;
    if (q0 < nt && first_col) star_load_keys<L>(first_col, q0, star_valid(q0, tid, a.n), KN, row_of);
    for (unsigned long long qb = tm.first(); qb < nt; qb += step) {
        const unsigned long long q = qb + team, qn = q + step;
        if (threadIdx.x == 0)
            s_stop = (unsigned)(__hip_atomic_load(a.counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 63);
        agg_tile_clear(lt, w, (int)threadIdx.x, (int)blockDim.x);
        unsigned alive = q < nt ? star_valid(q, tid, a.n) : 0u;
        star_key_t<L> KF[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) KF[i] = KN[i];
        if (qn < nt && first_col) star_load_keys<L>(first_col, qn, star_valid(qn, tid, a.n), KN, row_of);
        unsigned long long G[kProbeItems] = {};
        if constexpr (FACT) {
#pragma unroll 1
            for (int p = 0; p < a.f.npreds; ++p) {
                star_key_t<L> K[kProbeItems];
                if (p == 0) {
#pragma unroll
                    for (int i = 0; i < kProbeItems; ++i) K[i] = KF[i];
                } else {
                    star_load_keys<L>(a.f.pcol[p], q, alive, K, row_of);
                }
                const long long lo = a.f.plo[p], hi = a.f.phi[p];
                const bool outside = a.f.pkind[p] != 0;   // (uniform)
                unsigned pass = 0;
#pragma unroll
                for (int i = 0; i < kProbeItems; ++i) {
                    const long long x = L == kWide ? (long long)K[i] : (long long)(int)K[i];
                    pass |= ((x >= lo && x <= hi) != outside) ? 1u << i : 0u;
                }
                alive &= pass;
            }
        }
#pragma unroll 1
        for (int j = 0; j < a.nwalk; ++j) {
            const int d = a.order[j];   // (uniform)
            const StarDim &dm = a.d[d];
            const int gs = a.gshift[d];
            star_key_t<L> K[kProbeItems];
            long long RP[kProbeItems];
            if (j == 0 && !pred_first) {
#pragma unroll
                for (int i = 0; i < kProbeItems; ++i) K[i] = KF[i];
            } else {
                star_load_keys<L>(dm.key, q, alive, K, row_of);
            }
            const unsigned found = star_walk<L, true>(dm, alive, K, s_side_n[d], s_side_min[d], gs < 0 || s_unique[d] != 0u, RP);
            if (dm.kind == kStarInner) alive &= found;
            else if (dm.kind == kStarAnti) alive &= ~found;
            if (gs >= 0) {
                const long long base = a.gbase[d];
#pragma unroll
                for (int i = 0; i < kProbeItems; ++i) {
                    if (!((alive >> i) & 1u)) continue;
                    long long p = (long long)dm.null_pay;
                    if ((found >> i) & 1u) p = L == kWide ? RP[i] : (long long)(int)RP[i];
                    G[i] += ((unsigned long long)p - (unsigned long long)base) << gs;
                }
            }
        }
        unsigned long long V[kProbeItems];
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            V[i] = 0ull;
            if (vals && ((alive >> i) & 1u)) {
                if constexpr (L == kWide) V[i] = ((const unsigned long long *)a.sval)[row_of(q, i)];
                else V[i] = (unsigned long long)(long long)((const int *)a.sval)[row_of(q, i)];
            }
        }
        if constexpr (FACT) {
            auto fact_word = [&](const void *col, int i) {   // a fact column's value of row slot i, sign-extended
                if constexpr (L == kWide) return ((const unsigned long long *)col)[row_of(q, i)];
                else return (unsigned long long)(long long)((const int *)col)[row_of(q, i)];
            };
            if (vals && a.f.vop != kStarValueA) {   // (uniform)
                const int op = a.f.vop;
#pragma unroll
                for (int i = 0; i < kProbeItems; ++i) {
                    if (!((alive >> i) & 1u)) continue;
                    const unsigned long long b = fact_word(a.f.vb, i);
                    V[i] = op == kStarValueAdd ? V[i] + b : op == kStarValueSub ? V[i] - b : V[i] * b;
                }
            }
#pragma unroll 1
            for (int f = 0; f < a.f.nfact; ++f) {
                const void *col = a.f.fcol[f];
                const unsigned long long base = (unsigned long long)a.f.fbase[f];
                const int fs = a.f.fshift[f];
#pragma unroll
                for (int i = 0; i < kProbeItems; ++i) {
                    if (!((alive >> i) & 1u)) continue;
                    G[i] += (fact_word(col, i) - base) << fs;
                }
            }
        }
        __syncthreads();   // the table is clear, s_stop is everybody's
        if (s_stop != 0u) break;   // (uniform)
        unsigned direct = 0;
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((alive >> i) & 1u)) continue;
            if (!agg_tile_add(lt, w, G[i], V[i])) direct |= 1u << i;
        }
#pragma unroll
        for (int i = 0; i < kProbeItems; ++i) {
            if (!((direct >> i) & 1u)) continue;
            const unsigned long long h = agg_slot_bounded(gsl, a.gt, G[i], a.counter);
            if (h != ~0ull) acc_add<kWide>(a.acc, h, 1ull, V[i], (long long)V[i], (long long)V[i]);
        }
        __syncthreads();
        agg_tile_flush(lt, w, a.acc, a.gt.mask + 1ull, (int)threadIdx.x, (int)blockDim.x,
                       [&](unsigned long long k) { return agg_slot_bounded(gsl, a.gt, k, a.counter); });
        __syncthreads();   // the table is cleared, s_stop rewritten for the next tile
    }
}

// ------------------------------------------------------------------ partition
// Radix partition by a hash independent of the slot hash (fmix64 top word,
// multiply-shift onto [0, P)), so a partition's keys still spread over its
// local table.  Used to route R and S rows to their owning GPU.  rbits > 0:
// the top rbits of the radix join's own key hash instead (P = 2^rbits) --
// the folded routing, whose parts are (owner, first-pass bin) pairs.
__device__ __forceinline__ unsigned part_of(unsigned long long k, unsigned P, int rbits) {
    if (rbits > 0) return (unsigned)(radix_hash(k) >> (64 - rbits));
    return (unsigned)(((fmix64(k) >> 32) * (unsigned long long)P) >> 32);
}

// Parts at most this many: LDS counter updates are aggregated per wave (one
// atomic per distinct part and wave instead of one per lane: with 1-8 parts
// every lane of a wave hits the same few counters).
constexpr unsigned kAggParts = 16;

// Wave-aggregated cnt[d] += 1 for every lane with `valid`; returns the lane's
// rank among the lanes of its wave and part, offset by the counter's old
// value.  All 64 lanes must call it (ballots).
__device__ __forceinline__ unsigned agg_add(unsigned *cnt, unsigned d, bool valid) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    unsigned long long todo = __ballot(valid);
    unsigned rank = 0u;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned dl = __shfl(d, leader, 64);
        const bool mine = valid && d == dl;
        const unsigned long long m = __ballot(mine);
        unsigned b = 0u;
        if ((int)lane == leader) b = atomicAdd(&cnt[dl], (unsigned)__popcll(m));
        b = __shfl(b, leader, 64);
        if (mine) rank = b + (unsigned)__popcll(m & lt);
        todo &= ~m;
    }
    return rank;
}

template <int FORM>
__global__ __launch_bounds__(kBlock) void k_part_hist(SrcDev src, unsigned P, int rbits, unsigned long long *counts) {
    extern __shared__ unsigned lds_hist[];
    for (unsigned i = threadIdx.x; i < P; i += kBlock) lds_hist[i] = 0u;
    __syncthreads();
    // grid-stride over 2048-row chunks: one flush of the block's counts at
    // the end (a flush per chunk put ~10^5 atomics on each part's counter)
    for (long long base = (long long)blockIdx.x * (kBlock * kPartItems) + threadIdx.x; base - threadIdx.x < src.n;
         base += (long long)gridDim.x * (kBlock * kPartItems)) {
#pragma unroll
        for (int i = 0; i < kPartItems; ++i) {
            const long long row = base + (long long)i * kBlock;
            const bool v = row < src.n;
            const unsigned d = v ? part_of(load_src<FORM>(src, row).k, P, rbits) : 0u;
            if (P <= kAggParts) (void)agg_add(lds_hist, d, v);
            else if (v) atomicAdd(&lds_hist[d], 1u);
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < P; i += kBlock)
        if (lds_hist[i]) atomicAdd(&counts[i], (unsigned long long)lds_hist[i]);
}

__global__ void k_part_offsets(const unsigned long long *counts, unsigned P, unsigned long long *cursors) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        unsigned long long acc = 0;
        for (unsigned i = 0; i < P; ++i) {
            cursors[i] = acc;
            acc += counts[i];
        }
    }
}

template <int FORM>
__global__ __launch_bounds__(kBlock) void k_part_scatter(SrcDev src, unsigned P, int rbits, ulonglong2 *out,
                                                         unsigned long long *cursors) {
    extern __shared__ unsigned lds[];   // [0,P) local counts -> ranks, [P,3P) u64 bases
    unsigned *cnt = lds;
    unsigned long long *bases = (unsigned long long *)(lds + ((P + 1) & ~1u));
    for (unsigned i = threadIdx.x; i < P; i += kBlock) cnt[i] = 0u;
    __syncthreads();
    const long long base = (long long)blockIdx.x * (kBlock * kPartItems) + threadIdx.x;
    unsigned long long k[kPartItems], p[kPartItems];
    unsigned pid[kPartItems];
#pragma unroll
    for (int i = 0; i < kPartItems; ++i) {
        const long long row = base + (long long)i * kBlock;
        if (row < src.n) {
            Tuple tp = load_src<FORM>(src, row);
            k[i] = tp.k;
            p[i] = tp.p;
            pid[i] = part_of(tp.k, P, rbits);
            atomicAdd(&cnt[pid[i]], 1u);
        } else {
            pid[i] = ~0u;
            k[i] = p[i] = 0ull;
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < P; i += kBlock) {
        const unsigned c = cnt[i];
        bases[i] = c ? atomicAdd(&cursors[i], (unsigned long long)c) : 0ull;
        cnt[i] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPartItems; ++i) {
        if (pid[i] == ~0u) continue;
        const unsigned r = atomicAdd(&cnt[pid[i]], 1u);
        out[bases[pid[i]] + r] = make_ulonglong2(k[i], p[i]);
    }
}

// Staged scatter for up to kRouteMaxParts parts: one 8192-row tile per
// workgroup is counting-sorted by part in LDS and every part's run is then
// written by consecutive lanes to consecutive addresses.  k_part_scatter
// writes each row to its own rank slot (lanes of a wave hit unrelated
// addresses and most 128-B lines are written in pieces, each a
// read-modify-write in HBM: profiles/r01_micro_write_alignment.txt).
// Two shapes: up to 512 parts, 8192-row tiles (152 KiB of LDS: one
// workgroup per CU, whose load and store phases then alternate on the CU);
// 4..64 parts (the multi-GPU owner routing: one part per rank), 2048-row
// tiles in 37 KiB, four workgroups per CU overlapping each other's phases:
// 8 parts 4.22 -> 2.78 ms and 64 parts 6.11 -> 3.33 ms per 2^28 rows
// (profiles/r02_route_tiles.txt).  1-2 parts keep the large tile (2-5 %
// faster there); a 128-part small tile (38 KiB) and a 4096-row tile for
// 65..256 parts measured no better than the large one.
constexpr int kRouteTile = 8192;
constexpr int kRouteThreads = 1024;
constexpr int kRouteMaxParts = 512;
constexpr int kRouteTileS = 2048;
constexpr int kRouteThreadsS = 256;
constexpr int kRouteMaxPartsS = 64;

template <int FORM, int TILE, int NT, int MAXP>
__global__ __launch_bounds__(NT) void k_route_scatter(SrcDev src, unsigned P, int rbits, ulonglong2 *out,
                                                      unsigned long long *cursors) {
    constexpr int IT = TILE / NT;
    static_assert(MAXP % 64 == 0 && TILE % NT == 0 && IT % 2 == 0, "route tile shape");
    __shared__ ulonglong2 stage[TILE];
    __shared__ unsigned short sp[TILE];
    __shared__ unsigned cnt[MAXP], start[MAXP];
    __shared__ unsigned long long base[MAXP];
    for (unsigned i = threadIdx.x; i < P; i += NT) cnt[i] = 0u;
    __syncthreads();
    const long long lo = (long long)blockIdx.x * TILE;
    ulonglong2 row[IT];
    unsigned pr[IT];   // part << 16 | rank, or ~0
    if constexpr (FORM == kCols64) {
        // two consecutive rows per lane: one 16-B load from each column
        const unsigned long long *kc = (const unsigned long long *)src.key, *pc = (const unsigned long long *)src.pay;
        const bool al = ((((uintptr_t)kc) | ((uintptr_t)pc)) & 15) == 0;
#pragma unroll
        for (int i = 0; i < IT / 2; ++i) {
            const long long r = lo + 2ll * (i * NT + threadIdx.x);
            if (al && r + 1 < src.n) {
                const ulonglong2 k2 = *(const ulonglong2 *)(kc + r), p2 = *(const ulonglong2 *)(pc + r);
                row[2 * i] = make_ulonglong2(k2.x, p2.x);
                row[2 * i + 1] = make_ulonglong2(k2.y, p2.y);
                pr[2 * i] = pr[2 * i + 1] = 0u;
            } else {
                const bool v0 = r < src.n, v1 = r + 1 < src.n;
                row[2 * i] = v0 ? make_ulonglong2(kc[r], pc[r]) : make_ulonglong2(0ull, 0ull);
                row[2 * i + 1] = v1 ? make_ulonglong2(kc[r + 1], pc[r + 1]) : make_ulonglong2(0ull, 0ull);
                pr[2 * i] = v0 ? 0u : ~0u;
                pr[2 * i + 1] = v1 ? 0u : ~0u;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const long long r = lo + (long long)i * NT + threadIdx.x;
            const bool v = r < src.n;
            const Tuple tp = v ? load_src<FORM>(src, r) : Tuple{0ull, 0ull};
            row[i] = make_ulonglong2(tp.k, tp.p);
            pr[i] = v ? 0u : ~0u;
        }
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const bool v = pr[i] != ~0u;
        const unsigned d = v ? part_of(row[i].x, P, rbits) : 0u;
        if (P <= kAggParts) {
            const unsigned r = agg_add(cnt, d, v);
            if (v) pr[i] = (d << 16) | r;
        } else if (v) {
            pr[i] = (d << 16) | atomicAdd(&cnt[d], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {   // wave 0: stage offsets; one cursor atomic per non-empty part
        const unsigned lane = threadIdx.x;
        constexpr int PER = MAXP / 64;
        unsigned c[PER], sum = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const unsigned d = lane * PER + j;
            c[j] = d < P ? cnt[d] : 0u;
            sum += c[j];
        }
        unsigned run = wave_incl_add(sum) - sum;   // (the whole of wave 0 is here)
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const unsigned d = lane * PER + j;
            if (d < P) {
                start[d] = run;
                base[d] = c[j] ? atomicAdd(&cursors[d], (unsigned long long)c[j]) : 0ull;
            }
            run += c[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        if (pr[i] == ~0u) continue;
        const unsigned d = pr[i] >> 16, pos = start[d] + (pr[i] & 0xffffu);
        stage[pos] = row[i];
        sp[pos] = (unsigned short)d;
    }
    __syncthreads();
    const long long rem = src.n - lo;
    const unsigned tn = rem < TILE ? (unsigned)rem : (unsigned)TILE;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
        const unsigned j = (unsigned)i * NT + threadIdx.x;
        if (j >= tn) continue;
        const unsigned d = sp[j];
        out[base[d] + (j - start[d])] = stage[j];
    }
}

// ------------------------------------------------------------------ datagen
__global__ __launch_bounds__(kBlock) void k_gen_pkfk(unsigned long long seed, long long NR,
                                                     unsigned long long hit_thr, long long r0, long long nr,
                                                     long long *rkey, long long *rpay, long long s0, long long ns,
                                                     long long *skey, long long *spay) {
    const unsigned long long salt = pkfk_salt(seed);
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < nr) {
        const unsigned long long g = (unsigned long long)(r0 + i);
        rkey[i] = pkfk_rkey(salt, g);
        rpay[i] = (long long)g;
    }
    if (i < ns) {
        const unsigned long long g = (unsigned long long)(s0 + i);
        skey[i] = pkfk_skey(seed, salt, NR, hit_thr, g);
        spay[i] = (long long)g;
    }
}

__global__ __launch_bounds__(kBlock) void k_gen_uniform_i64(unsigned long long seed, unsigned long long sid,
                                                            long long lo, long long hi, long long i0, long long n,
                                                            long long *key, long long *pay) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned long long range = (unsigned long long)(hi - lo) + 1ull;
    const unsigned long long g = (unsigned long long)(i0 + i);
    const unsigned long long r = rand64(seed, sid, g);
    key[i] = lo + (long long)(range ? r % range : r);
    if (pay) pay[i] = (long long)g;
}

__global__ __launch_bounds__(kBlock) void k_gen_uniform_i32(unsigned long long seed, unsigned long long sid,
                                                            int lo, int hi, long long i0, long long n, int *key) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned long long range = (unsigned long long)((long long)hi - (long long)lo) + 1ull;
    const unsigned long long r = rand64(seed, sid, (unsigned long long)(i0 + i));
    key[i] = (int)((long long)lo + (long long)(r % range));
}

__global__ __launch_bounds__(kBlock) void k_gen_zipf(unsigned long long seed, ZipfParams z, long long s0, long long ns,
                                                     long long *skey, long long *spay) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= ns) return;
    const unsigned long long g = (unsigned long long)(s0 + i);
    skey[i] = zipf_skey(seed, z, g);
    spay[i] = (long long)g;
}

// ------------------------------------------------------------------ rows
// nested-loop.mlir's result rows (:160-188) materialised from join pairs.
// Key column (column 0) of a row-major int32 table with row stride ld.
__global__ __launch_bounds__(kBlock) void k_key_col_i32(const int *t, long long rows, long long ld, int *out) {
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i < rows) out[i] = t[i * ld];
}

// out[m] = [X[px[m]][0 .. cx), Y[py[m]][1 .. cy)] for m < min(*count, cap):
// one lane per output element, so the stores are coalesced and the row
// gathers are the only scattered accesses.
__global__ __launch_bounds__(kBlock) void k_gather_rows_i32(const int *x, long long ldx, int cx, const int *y,
                                                            long long ldy, int cy, const int *px, const int *py,
                                                            const unsigned long long *count, long long cap,
                                                            int *out, long long ldo) {
    const int oc = cx + cy - 1;
    const unsigned long long m_all = *count;
    const long long m = (long long)(m_all < (unsigned long long)cap ? m_all : (unsigned long long)cap);
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < m * oc; e += (long long)gridDim.x * kBlock) {
        const long long r = e / oc;
        const int c = (int)(e - r * oc);
        out[r * ldo + c] = c < cx ? x[(long long)px[r] * ldx + c] : y[(long long)py[r] * ldy + (c - cx + 1)];
    }
}

// ------------------------------------------------------------------ selection
// Experiments/selection.mlir (:34-155): keep the elements that pass
// `v <op> c`, compacted.  Order-preserving here (the reference orders blocks
// by an atomic): count per tile, exclusive scan of the counts, then each tile
// writes its survivors in element order.  A lane reads 16 B per load: slot j
// of lane t holds elements j*64*NW*W + t*W .. +W (W = 16 B / sizeof(V)), so
// element order is (slot, wave, lane, w) and positions come from per-lane
// counts, a wave prefix sum and one (slot, wave) scan per tile.
// Float compares are ordered (NaN never passes), like the reference's olt.
constexpr int kSelSlots = 4;

template <typename V>
__device__ __forceinline__ bool sel_pass(V v, int op, V c) {
    switch (op) {
        case 0: return v < c;
        case 1: return v <= c;
        case 2: return v > c;
        case 3: return v >= c;
        case 4: return v == c;
        default: return v < c || v > c;   // ordered not-equal
    }
}

template <typename V>
struct SelVec {
    static constexpr int W = 16 / sizeof(V);
    static constexpr long long kTile = (long long)kBlock * kSelSlots * W;
    V v[W];
};

// Slot j of this lane: W elements at e0 (vector load when whole and aligned).
template <typename V>
__device__ __forceinline__ void sel_load(const V *in, long long n, long long e0, bool vec_ok, SelVec<V> &x) {
    constexpr int W = SelVec<V>::W;
    if (vec_ok && e0 + W <= n) {
        const uint4 u = *(const uint4 *)(in + e0);
        __builtin_memcpy(x.v, &u, 16);
    } else {
#pragma unroll
        for (int w = 0; w < W; ++w) x.v[w] = e0 + w < n ? in[e0 + w] : V(0);
    }
}

template <typename V>
__global__ __launch_bounds__(kBlock) void k_sel_count(const V *in, long long n, int op, V c, bool vec_ok,
                                                      unsigned long long *tile_cnt) {
    constexpr int W = SelVec<V>::W;
    __shared__ unsigned ws[kBlock / 64];
    const long long base = (long long)blockIdx.x * SelVec<V>::kTile + (long long)threadIdx.x * W;
    unsigned k = 0;
#pragma unroll
    for (int j = 0; j < kSelSlots; ++j) {
        SelVec<V> x;
        const long long e0 = base + (long long)j * kBlock * W;
        sel_load(in, n, e0, vec_ok, x);
#pragma unroll
        for (int w = 0; w < W; ++w) k += (e0 + w < n && sel_pass(x.v[w], op, c)) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k += __shfl_down(k, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) t += ws[w];
        tile_cnt[blockIdx.x] = t;
    }
}

template <typename V>
__global__ __launch_bounds__(kBlock) void k_sel_write(const V *in, long long n, int op, V c, bool vec_ok,
                                                      const unsigned long long *tile_off, unsigned ntiles, V *out,
                                                      long long *out_row, long long cap,
                                                      unsigned long long *count) {
    constexpr int W = SelVec<V>::W;
    constexpr int NW = kBlock / 64;
    __shared__ unsigned s_cw[kSelSlots * NW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * SelVec<V>::kTile + (long long)threadIdx.x * W;
    SelVec<V> x[kSelSlots];
    unsigned pass[kSelSlots], lpre[kSelSlots];
#pragma unroll
    for (int j = 0; j < kSelSlots; ++j) {
        const long long e0 = base + (long long)j * kBlock * W;
        sel_load(in, n, e0, vec_ok, x[j]);
        pass[j] = 0;
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (e0 + w < n && sel_pass(x[j].v[w], op, c)) pass[j] |= 1u << w;
        // lane prefix within the wave for this slot (every lane gets here)
        const unsigned k = (unsigned)__popc(pass[j]);
        const unsigned xs = wave_incl_add(k);
        lpre[j] = xs - k;
        if (lane == 63) s_cw[j * NW + wv] = xs;
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // (slot, wave) runs in element order: kSelSlots * NW = 16 entries
        unsigned run = 0;
#pragma unroll
        for (int q = 0; q < kSelSlots * NW; ++q) {
            const unsigned v = s_cw[q];
            s_cw[q] = run;
            run += v;
        }
    }
    __syncthreads();
    const unsigned long long tb = tile_off[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kSelSlots; ++j) {
        unsigned long long g = tb + s_cw[j * NW + wv] + lpre[j];
        const long long e0 = base + (long long)j * kBlock * W;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (!((pass[j] >> w) & 1u)) continue;
            if (g < (unsigned long long)cap) {
                out[g] = x[j].v[w];
                if (out_row) out_row[g] = e0 + w;
            }
            ++g;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = tile_off[ntiles];
}

inline unsigned grid_for(long long n, int per_block) {
    return (unsigned)((n + per_block - 1) / per_block);
}

// The (layout, form) pairs the library has kernels for, as compile-time
// constants: f(integral_constant<int, L>, integral_constant<int, FORM>);
// any other pair is hipErrorInvalidValue and instantiates nothing.
// with_form64: the two int64 forms alone (the partition takes no others).
template <int V>
using int_c = std::integral_constant<int, V>;
template <typename F>
hipError_t with_form64(int form, F &&f) {
    if (form == kCols64) return f(int_c<kCols64>{});
    if (form == kPacked64) return f(int_c<kPacked64>{});
    return hipErrorInvalidValue;
}
template <typename F>
hipError_t with_layout_form(int layout, int form, F &&f) {
    if (layout == kWide) return with_form64(form, [&](auto fm) { return f(int_c<kWide>{}, fm); });
    if (layout == kNarrow && form == kCol32) return f(int_c<kNarrow>{}, int_c<kCol32>{});
    return hipErrorInvalidValue;
}

// Grid of the tile probes (k_probe, k_probe_exists) over n rows.  A table of
// <= kLdsTableBytes: every workgroup copies it into LDS once (tbytes of
// dynamic LDS) and strides over the tiles, as many workgroups as LDS lets a
// CU hold; a larger one: one workgroup per tile.
struct ProbeGrid {
    bool lds;
    size_t tbytes;
    unsigned grid;
};
ProbeGrid probe_grid(const TableDev &t, int layout, long long n) {
    const unsigned tiles = grid_for(n, kProbeTile);
    const size_t tbytes = (size_t)(t.mask + 1) * (layout == kWide ? 16 : 8);
    const bool lds = tbytes <= (size_t)kLdsTableBytes && tbytes >= 16;
    unsigned per_cu = lds ? (unsigned)(kLdsPerCu / tbytes) : 1u;
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    const unsigned most = (unsigned)cu_count() * per_cu;
    return {lds, tbytes, lds && most < tiles ? most : tiles};
}

}  // namespace

// ---------------------------------------------------------------- launchers
hipError_t launch_init(const TableDev &t, int layout, unsigned long long cap, hipStream_t st) {
    const unsigned long long bytes = cap * (layout == kWide ? 16ull : 8ull);
    const unsigned long long n16 = bytes / 16ull;
    const unsigned g = grid_for((long long)n16, kBlock * 4);
    if (layout == kWide) hipLaunchKernelGGL(k_init<kWide>, dim3(g), dim3(kBlock), 0, st, t, n16);
    else hipLaunchKernelGGL(k_init<kNarrow>, dim3(g), dim3(kBlock), 0, st, t, n16);
    return hipGetLastError();
}

hipError_t launch_build(const TableDev &t, int layout, const SrcDev &src, hipStream_t st) {
    if (src.n <= 0) return hipSuccess;
    const unsigned g = grid_for(src.n, kBlock * kBuildItems);
    return with_layout_form(layout, src.form, [&](auto l, auto f) {
        hipLaunchKernelGGL((k_build<decltype(l)::value, decltype(f)::value>), dim3(g), dim3(kBlock), 0, st, t, src);
        return hipGetLastError();
    });
}

size_t probe_tiles(long long n) {
    // plain tiles: one slow-list entry per 2048-row tile at most
    return (size_t)(n > 0 ? (n + kProbeTile - 1) / kProbeTile : 0) + 1;
}

hipError_t launch_probe(const TableDev &t, int layout, const SrcDev &src, const OutDev &out,
                        bool count_only, unsigned *slow, size_t slow_cap, hipStream_t st, unsigned *marks) {
    if (src.n <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(&t.meta[3], 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const unsigned long long cap = slow_cap;
    const ProbeGrid pg = probe_grid(t, layout, src.n);
    // the general path's persistent workgroups: eight per CU, a tile each at most
    const unsigned tiles = grid_for(src.n, kProbeTile), most = (unsigned)(cu_count() * 8);
    const unsigned gs = tiles < most ? tiles : most;
    return with_layout_form(layout, src.form, [&](auto l, auto f) {
        constexpr int L = decltype(l)::value, F = decltype(f)::value;
        const auto fast = count_only ? (pg.lds ? k_probe<L, F, false, true> : k_probe<L, F, false, false>)
                                     : (pg.lds ? k_probe<L, F, true, true> : k_probe<L, F, true, false>);
        const auto rest = count_only ? k_probe_slow<L, F, false> : k_probe_slow<L, F, true>;
        if (marks) {
            const auto fm = count_only ? (pg.lds ? k_probe<L, F, false, true, unsigned *> : k_probe<L, F, false, false, unsigned *>)
                                       : (pg.lds ? k_probe<L, F, true, true, unsigned *> : k_probe<L, F, true, false, unsigned *>);
            hipLaunchKernelGGL(fm, dim3(pg.grid), dim3(kBlock), pg.lds ? pg.tbytes : 0, st, t, src, out, slow, cap, marks);
        } else
            hipLaunchKernelGGL(fast, dim3(pg.grid), dim3(kBlock), pg.lds ? pg.tbytes : 0, st, t, src, out, slow, cap);
        hipLaunchKernelGGL(rest, dim3(gs), dim3(kBlock), 0, st, t, src, out, (const unsigned *)slow, cap);
        return hipGetLastError();
    });
}

hipError_t launch_probe_exists(const TableDev &t, int layout, const SrcDev &src, const OutDev &out, bool anti,
                               hipStream_t st) {
    if (src.n <= 0) return hipSuccess;
    const ProbeGrid pg = probe_grid(t, layout, src.n);
    const unsigned a = anti ? 1u : 0u;
    return with_layout_form(layout, src.form, [&](auto l, auto f) {
        constexpr int L = decltype(l)::value, F = decltype(f)::value;
        const auto k = pg.lds ? k_probe_exists<L, F, true> : k_probe_exists<L, F, false>;
        hipLaunchKernelGGL(k, dim3(pg.grid), dim3(kBlock), pg.lds ? pg.tbytes : 0, st, t, src, out, a);
        return hipGetLastError();
    });
}

hipError_t launch_probe_lookup(const TableDev &t, int layout, const SrcDev &src, const OutDev &out, int *cnt,
                               unsigned long long null_pay, hipStream_t st) {
    if (src.n <= 0) return hipSuccess;
    const ProbeGrid pg = probe_grid(t, layout, src.n);
    // (a key column only: the int64 column form or the i32 one)
    auto launch = [&](auto l, auto f) {
        constexpr int L = decltype(l)::value, F = decltype(f)::value;
        const auto k = pg.lds ? k_probe_lookup<L, F, true> : k_probe_lookup<L, F, false>;
        hipLaunchKernelGGL(k, dim3(pg.grid), dim3(kBlock), pg.lds ? pg.tbytes : 0, st, t, src, out, cnt, null_pay);
        return hipGetLastError();
    };
    if (layout == kWide && src.form == kCols64) return launch(int_c<kWide>{}, int_c<kCols64>{});
    if (layout == kNarrow && src.form == kCol32) return launch(int_c<kNarrow>{}, int_c<kCol32>{});
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------- star probe
namespace {
static_assert(kFilterTile == kProbeTile && kFilterBlock == kBlock, "the star probe shares the key filter's workspace shape");
// Every star kernel there is: f(layout, ndims, variant, kernel) for each (layout, ND, variant), the first three
// as int_c.  The variants are k_star's modes and, behind them, k_star_agg without and with FACT.  star_prepare and
// star_launch both go through here, so an instantiation is named once and none can miss its attribute.
enum : int { kStarAgg = 3, kStarQuery = 4 };
template <int V>
using star_args_t =
    std::conditional_t<V == kStarQuery, StarQueryArgs, std::conditional_t<V == kStarAgg, StarAggArgs, StarArgs>>;
template <int... V, class F>
void for_ints(F &&f) {
    (f(int_c<V>{}), ...);
}
template <class F>
void for_each_star_kernel(F &&f) {
    for_ints<kWide, kNarrow>([&](auto l) {
        for_ints<1, 2, 3, 4>([&](auto nd) {
            for_ints<kStarDecide, kStarWrite, kStarAll, kStarAgg, kStarQuery>([&](auto v) {
                constexpr int L = decltype(l)::value, ND = decltype(nd)::value, V = decltype(v)::value;
                static_assert(ND <= kStarMaxDims);
                if constexpr (V <= kStarAll) f(l, nd, v, k_star<L, ND, V>);
                else f(l, nd, v, k_star_agg<L, ND, V == kStarQuery>);
            });
        });
    });
}
// (the launchers have checked layout and ndims: exactly one instantiation matches)
template <int V>
void star_launch(int layout, int ndims, unsigned grid, unsigned threads, size_t lds, hipStream_t st,
                 const star_args_t<V> &a) {
    for_each_star_kernel([&](auto l, auto nd, auto v, auto k) {
        if constexpr (decltype(v)::value == V)
            if (l == layout && nd == ndims) hipLaunchKernelGGL(k, dim3(grid), dim3(threads), lds, st, a);
    });
}

// The placement plan of a persistent launch that walks dimensions walk[0 .. nwalk): their tables ascending by
// size (ties in walk order) get a copy in dynamic LDS while each is an LDS table's size at most and they fit the
// budget together.  Assigns lds_off in dimension order, -1 where there is no copy.
struct StarPlacement {
    int lds_dims;
    size_t lds_bytes;
};
StarPlacement star_place(int layout, int ndims, StarDim (&dims)[kStarMaxDims], const int *walk, int nwalk,
                         size_t budget) {
    const size_t sb = layout == kWide ? 16 : 8;
    size_t bytes[kStarMaxDims];
    int order[kStarMaxDims];
    for (int j = 0; j < nwalk; ++j) {
        const int d = walk[j];
        bytes[d] = (size_t)(dims[d].t.mask + 1) * sb;
        int k = j;
        for (; k > 0 && bytes[order[k - 1]] > bytes[d]; --k) order[k] = order[k - 1];
        order[k] = d;
    }
    StarPlacement p{0, 0};
    for (int j = 0; j < nwalk; ++j) {
        const size_t b = bytes[order[j]];
        if (b > (size_t)kLdsTableBytes || p.lds_bytes + b > budget) break;
        p.lds_dims |= 1 << order[j];
        p.lds_bytes += b;
    }
    size_t off = 0;
    for (int d = 0; d < kStarMaxDims; ++d) {
        dims[d].lds_off = -1;
        if (d < ndims && ((p.lds_dims >> d) & 1)) {
            dims[d].lds_off = (int)off;
            off += bytes[d];
        }
    }
    return p;
}

// The persistent grid over `tiles` tiles.  With table copies: workgroups of kStarTeams teams, per CU as many as
// lds_cu / (lds_bytes + static_lds) and the wave slots (8 teams) admit.  Without: one team each, plain_per_cu per
// CU, or one workgroup per tile when that is 0.
struct StarGrid {
    unsigned grid, teams;
};
StarGrid star_grid(unsigned tiles, size_t lds_bytes, size_t lds_cu, size_t static_lds, unsigned plain_per_cu) {
    unsigned teams = 1, per_cu = plain_per_cu;
    if (lds_bytes) {
        teams = kStarTeams;   // (4 workgroups x 2 teams x 4 waves are a CU's 32 wave slots)
        per_cu = (unsigned)(lds_cu / (lds_bytes + static_lds));
        if (per_cu * teams > 8) per_cu = 8 / teams;
        if (per_cu < 1) per_cu = 1;
    }
    if (per_cu == 0) return {tiles, teams};
    const unsigned most = (unsigned)cu_count() * per_cu, want = (tiles + teams - 1) / teams;
    return {most < want ? most : want, teams};
}
}  // namespace

hipError_t star_prepare() {
    hipError_t e = hipSuccess;
    for_each_star_kernel([&](auto, auto, auto, auto k) {
        if (e != hipSuccess) return;
        e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsPerCu);
    });
    return e;
}

hipError_t launch_star_aggregate(int layout, int ndims, StarAggArgs a, const GroupOut &out, StarPlan *plan,
                                 hipStream_t st, const StarFact *fact) {
    if (ndims < (fact ? 0 : 1) || ndims > kStarMaxDims || (layout != kWide && layout != kNarrow))
        return hipErrorInvalidValue;
    if (ndims == 0) {   // the ND = 1 instantiation over a dimension that is never walked
        a.d[0] = StarDim{};
        a.d[0].kind = kStarLeft;
        a.gshift[0] = -1;
    }
    const unsigned long long cap = a.gt.mask + 1ull, entries = cap + 1ull;
    a.counter = out.counter;
    hipError_t e = launch_init(a.gt, kWide, cap, st);
    if (e != hipSuccess) return e;
    const unsigned most = (unsigned)(cu_count() * 8);
    const unsigned fl = grid_for((long long)entries, kBlock), gi = fl < most ? fl : most;
    hipLaunchKernelGGL(k_aggregate_init<kWide>, dim3(gi), dim3(kBlock), 0, st, a.acc, entries, out.counter);
    *plan = StarPlan{3, 0u, 0, 0, 0};
    if (a.n > 0) {
        // the walk order: the dimensions that can drop a row in the caller's order, then the grouped LEFT ones
        a.nwalk = 0;
        for (int d = 0; d < ndims; ++d)
            if (a.d[d].kind != kStarLeft) a.order[a.nwalk++] = d;
        for (int d = 0; d < ndims; ++d)
            if (a.d[d].kind == kStarLeft && a.gshift[d] >= 0) a.order[a.nwalk++] = d;
        // placement: the budget is what the CU has left beside the kernel's static LDS and no more than kLdsPerCu
        const size_t budget = (size_t)(kLdsCu - kStarAggStaticLds < kLdsPerCu ? kLdsCu - kStarAggStaticLds : kLdsPerCu);
        const StarPlacement p = star_place(layout, ndims, a.d, a.order, a.nwalk, budget);
        // without copies eight workgroups per CU (the collapse table alone, as k_aggregate's)
        const unsigned tiles = grid_for(a.n, kProbeTile);
        const StarGrid g = star_grid(tiles, p.lds_bytes, (size_t)kLdsCu, (size_t)kStarAggStaticLds, 8);
        if (fact) {
            StarQueryArgs qa{};
            static_cast<StarAggArgs &>(qa) = a;
            qa.f = *fact;
            star_launch<kStarQuery>(layout, ndims ? ndims : 1, g.grid, kBlock * g.teams, p.lds_bytes, st, qa);
        } else {
            star_launch<kStarAgg>(layout, ndims, g.grid, kBlock * g.teams, p.lds_bytes, st, a);
        }
        *plan = StarPlan{4, g.grid, (long long)tiles, p.lds_dims, (long long)p.lds_bytes};
    }
    const unsigned tl = grid_for((long long)cap, kProbeTile), g = tl < most ? tl : most;
    hipLaunchKernelGGL(k_emit_aggregate<kWide>, dim3(g), dim3(kBlock), 0, st, a.gt, a.acc, out);
    return hipGetLastError();
}

hipError_t launch_star(int layout, int ndims, StarArgs a, const FilterWork &ws, StarPlan *plan, hipStream_t st) {
    if (ndims < 1 || ndims > kStarMaxDims || (layout != kWide && layout != kNarrow)) return hipErrorInvalidValue;
    a.tiles = ws.tiles;
    a.bitmap = ws.bitmap;
    *plan = StarPlan{1, 0u, 0, 0, 0};
    bool drops = false;
    for (int d = 0; d < ndims; ++d) drops |= a.d[d].kind != kStarLeft;
    // no tile to walk: the counter alone (keep-all: M = n whatever the tables hold)
    if (a.n <= 0 || (!drops && a.cap <= 0)) {
        hipLaunchKernelGGL(k_star_total, dim3(1), dim3(64), 0, st, (const unsigned long long *)nullptr,
                           (unsigned long long)(a.n > 0 ? a.n : 0), a.count);
        return hipGetLastError();
    }
    // placement: the tables the probe launch walks (the decision's INNER and
    // ANTI dimensions; keep-all: the ones with a payload column)
    int walk[kStarMaxDims], nwalk = 0;
    for (int d = 0; d < ndims; ++d)
        if (drops ? a.d[d].kind != kStarLeft : a.d[d].out != nullptr) walk[nwalk++] = d;
    const StarPlacement p = star_place(layout, ndims, a.d, walk, nwalk, (size_t)kLdsPerCu);
    // the probe launch: as many workgroups of kStarTeams teams as its table
    // copies let a CU hold stride over the tiles; without a copy, one workgroup
    // of one team per tile.  The write
    // launch walks the survivors alone: no copies (a copy per workgroup costs
    // what the walks of a few rows do not give back) and one workgroup per tile.
    const unsigned tiles = grid_for(a.n, kProbeTile);
    const StarGrid g = star_grid(tiles, p.lds_bytes, (size_t)kLdsPerCu, 0, 0);
    *plan = StarPlan{0, g.grid, (long long)tiles, p.lds_dims, (long long)p.lds_bytes};
    auto launch = [&](auto m) {
        constexpr int mode = decltype(m)::value;
        constexpr bool write = mode == kStarWrite;
        StarArgs b = a;
        b.first = -1;
        for (int d = 0; d < ndims; ++d) {
            const bool walks = mode == kStarDecide ? b.d[d].kind != kStarLeft : b.d[d].out != nullptr;
            if (write) b.d[d].lds_off = -1;
            if (walks && b.first < 0) b.first = d;
        }
        star_launch<mode>(layout, ndims, write ? tiles : g.grid, kBlock * (write ? 1u : g.teams),
                          write ? 0 : p.lds_bytes, st, b);
        ++plan->launches;
        return hipGetLastError();
    };
    if (!drops) return launch(int_c<kStarAll>{});
    hipError_t e = launch(int_c<kStarDecide>{});
    if (e != hipSuccess) return e;
    e = exclusive_scan_u64(ws.tiles, (unsigned long long)tiles + 1, ws.sums, st);
    if (e != hipSuccess) return e;
    plan->launches += exclusive_scan_launches((unsigned long long)tiles + 1);
    if (a.cap > 0) return launch(int_c<kStarWrite>{});
    hipLaunchKernelGGL(k_star_total, dim3(1), dim3(64), 0, st, (const unsigned long long *)(ws.tiles + tiles), 0ull,
                       a.count);
    ++plan->launches;
    return hipGetLastError();
}

hipError_t launch_probe_asof(const TableDev &t, int layout, int kind, const SrcDev &src, const void *bound,
                             const OutDev &out, unsigned long long null_pay, hipStream_t st) {
    hipLaunchKernelGGL(k_counter_clear, dim3(1), dim3(64), 0, st, out.counter);
    if (src.n <= 0) return hipGetLastError();
    const ProbeGrid pg = probe_grid(t, layout, src.n);
    // (a key column only, as the lookup's; one instantiation per kind: the walk holds no kind branch)
    auto launch = [&](auto l, auto f, auto k_) {
        constexpr int L = decltype(l)::value, F = decltype(f)::value, K = decltype(k_)::value;
        const auto k = pg.lds ? k_probe_asof<L, F, true, K> : k_probe_asof<L, F, false, K>;
        hipLaunchKernelGGL(k, dim3(pg.grid), dim3(kBlock), pg.lds ? pg.tbytes : 0, st, t, src, bound, out, null_pay);
        return hipGetLastError();
    };
    auto by_kind = [&](auto l, auto f) {
        switch (kind) {
        case 0: return launch(l, f, int_c<0>{});
        case 1: return launch(l, f, int_c<1>{});
        case 2: return launch(l, f, int_c<2>{});
        case 3: return launch(l, f, int_c<3>{});
        default: return hipErrorInvalidValue;
        }
    };
    if (layout == kWide && src.form == kCols64) return by_kind(int_c<kWide>{}, int_c<kCols64>{});
    if (layout == kNarrow && src.form == kCol32) return by_kind(int_c<kNarrow>{}, int_c<kCol32>{});
    return hipErrorInvalidValue;
}

size_t expand_scan_tiles(long long n) { return n > 0 ? (size_t)((n + kExpandTile - 1) / kExpandTile) : 1; }

hipError_t launch_expand_scan(const int *cnt, long long n, bool outer, unsigned long long *sums, long long *off,
                              unsigned long long *count, hipStream_t st) {
    // (n == 0: one workgroup over no rows writes off[0] = 0 and the counter)
    const long long rows = n > 0 ? n : 0;
    const unsigned tiles = (unsigned)expand_scan_tiles(rows);
    const unsigned o = outer ? 1u : 0u;
    hipLaunchKernelGGL(k_expand_sums, dim3(tiles), dim3(kBlock), 0, st, cnt, rows, o, sums);
    hipLaunchKernelGGL(k_expand_scan_sums, dim3(1), dim3(kExpandFan), 0, st, sums, (unsigned long long)tiles);
    hipLaunchKernelGGL(k_expand_offsets, dim3(tiles), dim3(kBlock), 0, st, cnt, rows, o,
                       (const unsigned long long *)sums, off, count);
    return hipGetLastError();
}

hipError_t launch_probe_expand(const TableDev &t, int layout, const SrcDev &src, const long long *off, void *out_r,
                               long long cap, bool outer, unsigned long long null_pay, hipStream_t st) {
    if (src.n <= 0 || cap <= 0) return hipSuccess;
    const ProbeGrid pg = probe_grid(t, layout, src.n);
    auto launch = [&](auto l, auto f) {
        constexpr int L = decltype(l)::value, F = decltype(f)::value;
        const auto k = pg.lds ? k_probe_expand<L, F, true> : k_probe_expand<L, F, false>;
        hipLaunchKernelGGL(k, dim3(pg.grid), dim3(kBlock), pg.lds ? pg.tbytes : 0, st, t, src, off, out_r,
                           (unsigned long long)cap, outer ? 1u : 0u, null_pay);
        return hipGetLastError();
    };
    if (layout == kWide && src.form == kCols64) return launch(int_c<kWide>{}, int_c<kCols64>{});
    if (layout == kNarrow && src.form == kCol32) return launch(int_c<kNarrow>{}, int_c<kCol32>{});
    return hipErrorInvalidValue;
}

hipError_t launch_probe_outer(const TableDev &t, int layout, const SrcDev &src, const OutDev &out,
                              unsigned long long null_pay, unsigned *slow, size_t slow_cap, hipStream_t st,
                              unsigned *marks) {
    if (src.n <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(&t.meta[3], 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    const unsigned long long cap = slow_cap;
    const ProbeGrid pg = probe_grid(t, layout, src.n);
    // the general path's persistent workgroups, as launch_probe's
    const unsigned tiles = grid_for(src.n, kProbeTile), most = (unsigned)(cu_count() * 8);
    const unsigned gs = tiles < most ? tiles : most;
    return with_layout_form(layout, src.form, [&](auto l, auto f) {
        constexpr int L = decltype(l)::value, F = decltype(f)::value;
        const auto fast = pg.lds ? k_probe_outer<L, F, true> : k_probe_outer<L, F, false>;
        const auto rest = out.cap == 0 ? k_probe_slow<L, F, false, unsigned long long>
                                       : k_probe_slow<L, F, true, unsigned long long>;
        if (marks) {
            const auto fm = pg.lds ? k_probe_outer<L, F, true, unsigned *> : k_probe_outer<L, F, false, unsigned *>;
            hipLaunchKernelGGL(fm, dim3(pg.grid), dim3(kBlock), pg.lds ? pg.tbytes : 0, st, t, src, out, slow, cap,
                               null_pay, marks);
        } else
            hipLaunchKernelGGL(fast, dim3(pg.grid), dim3(kBlock), pg.lds ? pg.tbytes : 0, st, t, src, out, slow, cap,
                               null_pay);
        hipLaunchKernelGGL(rest, dim3(gs), dim3(kBlock), 0, st, t, src, out, (const unsigned *)slow, cap, null_pay);
        return hipGetLastError();
    });
}

size_t mark_words(unsigned long long cap) { return (size_t)(cap >> 5 ? cap >> 5 : 1) + 1; }

hipError_t launch_marks_clear(const TableDev &t, unsigned *marks, hipStream_t st) {
    return hipMemsetAsync(marks, 0, mark_words(t.mask + 1ull) * sizeof(unsigned), st);
}

hipError_t launch_unmatched_build(const TableDev &t, int layout, const SrcDev &src, const OutDev &out,
                                  unsigned long long null_s, unsigned *marks, const unsigned *slow, size_t slow_cap,
                                  hipStream_t st) {
    const unsigned long long cap = t.mask + 1ull, words = mark_words(cap) - 1;
    if (src.n > 0) {
        // the handed-over tiles' persistent workgroups, as k_probe_slow's
        const unsigned tl = grid_for(src.n, kProbeTile), mx = (unsigned)(cu_count() * 8);
        const unsigned g = tl < mx ? tl : mx;
        const hipError_t e = with_layout_form(layout, src.form, [&](auto l, auto f) {
            hipLaunchKernelGGL((k_probe_mark<decltype(l)::value, decltype(f)::value>), dim3(g), dim3(kBlock), 0, st, t,
                               src, marks, words, slow, (unsigned long long)slow_cap);
            return hipGetLastError();
        });
        if (e != hipSuccess) return e;
    }
    // the scan's persistent workgroups: eight per CU, a tile each at most
    const unsigned tiles = grid_for((long long)cap, kProbeTile), most = (unsigned)(cu_count() * 8);
    const unsigned g = tiles < most ? tiles : most;
    if (layout == kWide)
        hipLaunchKernelGGL(k_emit_unmatched<kWide>, dim3(g), dim3(kBlock), 0, st, t, out, (const unsigned *)marks, words,
                           null_s);
    else if (layout == kNarrow)
        hipLaunchKernelGGL(k_emit_unmatched<kNarrow>, dim3(g), dim3(kBlock), 0, st, t, out, (const unsigned *)marks,
                           words, null_s);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_group(const TableDev &t, int layout, const SrcDev &src, const GroupAcc &acc, const GroupOut &out,
                        hipStream_t st) {
    if (layout != kWide && layout != kNarrow) return hipErrorInvalidValue;
    const unsigned long long cap = t.mask + 1ull, entries = cap + 1ull;
    // the fill's and the scan's persistent workgroups: eight per CU at most
    const unsigned most = (unsigned)(cu_count() * 8);
    const unsigned fl = grid_for((long long)entries, kBlock), gi = fl < most ? fl : most;
    if (layout == kWide) hipLaunchKernelGGL(k_group_init<kWide>, dim3(gi), dim3(kBlock), 0, st, acc, entries);
    else hipLaunchKernelGGL(k_group_init<kNarrow>, dim3(gi), dim3(kBlock), 0, st, acc, entries);
    if (src.n > 0) {
        const unsigned tiles = grid_for(src.n, kProbeTile);
        const hipError_t e = with_layout_form(layout, src.form, [&](auto l, auto f) {
            hipLaunchKernelGGL((k_probe_group<decltype(l)::value, decltype(f)::value>), dim3(tiles), dim3(kBlock), 0, st,
                               t, src, acc);
            return hipGetLastError();
        });
        if (e != hipSuccess) return e;
    }
    const unsigned tl = grid_for((long long)cap, kProbeTile), g = tl < most ? tl : most;
    if (layout == kWide) hipLaunchKernelGGL(k_emit_groups<kWide>, dim3(g), dim3(kBlock), 0, st, t, acc, out);
    else hipLaunchKernelGGL(k_emit_groups<kNarrow>, dim3(g), dim3(kBlock), 0, st, t, acc, out);
    return hipGetLastError();
}

hipError_t launch_aggregate(const TableDev &t, int layout, const SrcDev &src, const GroupAcc &acc, const GroupOut &out,
                            hipStream_t st) {
    if (layout != kWide && layout != kNarrow) return hipErrorInvalidValue;
    const unsigned long long cap = t.mask + 1ull, entries = cap + 1ull;
    hipError_t e = launch_init(t, layout, cap, st);
    if (e != hipSuccess) return e;
    // the fill's, the tiles' and the scan's persistent workgroups: eight per CU at most (their LDS)
    const unsigned most = (unsigned)(cu_count() * 8);
    const unsigned fl = grid_for((long long)entries, kBlock), gi = fl < most ? fl : most;
    if (layout == kWide)
        hipLaunchKernelGGL(k_aggregate_init<kWide>, dim3(gi), dim3(kBlock), 0, st, acc, entries, out.counter);
    else hipLaunchKernelGGL(k_aggregate_init<kNarrow>, dim3(gi), dim3(kBlock), 0, st, acc, entries, out.counter);
    if (src.n > 0) {
        const unsigned tiles = grid_for(src.n, kProbeTile), ga = tiles < most ? tiles : most;
        e = with_layout_form(layout, src.form, [&](auto l, auto f) {
            hipLaunchKernelGGL((k_aggregate<decltype(l)::value, decltype(f)::value>), dim3(ga), dim3(kBlock), 0, st, t,
                               src, acc);
            return hipGetLastError();
        });
        if (e != hipSuccess) return e;
    }
    const unsigned tl = grid_for((long long)cap, kProbeTile), g = tl < most ? tl : most;
    if (layout == kWide) hipLaunchKernelGGL(k_emit_aggregate<kWide>, dim3(g), dim3(kBlock), 0, st, t, acc, out);
    else hipLaunchKernelGGL(k_emit_aggregate<kNarrow>, dim3(g), dim3(kBlock), 0, st, t, acc, out);
    return hipGetLastError();
}

hipError_t launch_partition(const SrcDev &src, int nparts, void *out_tuples,
                            unsigned long long *counts, unsigned long long *cursors, hipStream_t st, int rbits) {
    const unsigned P = (unsigned)nparts;
    if (rbits > 0 && (rbits > 13 || P != (1u << rbits))) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(unsigned long long) * P, st);
    if (e != hipSuccess) return e;
    if (src.n <= 0) return hipGetLastError();
    return with_form64(src.form, [&](auto f) {
        constexpr int F = decltype(f)::value;
        const unsigned g = grid_for(src.n, kBlock * kPartItems);
        const unsigned most = (unsigned)cu_count() * 8u;
        const unsigned gh = g < most ? g : most;
        const size_t lds_h = sizeof(unsigned) * P;
        const size_t lds_s = sizeof(unsigned) * ((P + 1) & ~1u) + sizeof(unsigned long long) * P;
        ulonglong2 *rows = (ulonglong2 *)out_tuples;
        hipLaunchKernelGGL(k_part_hist<F>, dim3(gh), dim3(kBlock), lds_h, st, src, P, rbits, counts);
        hipLaunchKernelGGL(k_part_offsets, dim3(1), dim3(64), 0, st, counts, P, cursors);
        if (P >= 4u && P <= (unsigned)kRouteMaxPartsS)
            hipLaunchKernelGGL((k_route_scatter<F, kRouteTileS, kRouteThreadsS, kRouteMaxPartsS>),
                               dim3(grid_for(src.n, kRouteTileS)), dim3(kRouteThreadsS), 0, st, src, P, rbits, rows, cursors);
        else if (P <= (unsigned)kRouteMaxParts)
            hipLaunchKernelGGL((k_route_scatter<F, kRouteTile, kRouteThreads, kRouteMaxParts>),
                               dim3(grid_for(src.n, kRouteTile)), dim3(kRouteThreads), 0, st, src, P, rbits, rows, cursors);
        else
            hipLaunchKernelGGL(k_part_scatter<F>, dim3(g), dim3(kBlock), lds_s, st, src, P, rbits, rows, cursors);
        return hipGetLastError();
    });
}

hipError_t launch_gen_pkfk(unsigned long long seed, long long NR, unsigned long long hit_thr,
                           long long r0, long long nr, long long *rkey, long long *rpay,
                           long long s0, long long ns, long long *skey, long long *spay, hipStream_t st) {
    const long long n = nr > ns ? nr : ns;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gen_pkfk, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, seed, NR, hit_thr, r0, nr,
                       rkey, rpay, s0, ns, skey, spay);
    return hipGetLastError();
}

hipError_t launch_gen_zipf(unsigned long long seed, const ZipfParams &z, long long s0, long long ns, long long *skey,
                           long long *spay, hipStream_t st) {
    if (ns <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gen_zipf, dim3(grid_for(ns, kBlock)), dim3(kBlock), 0, st, seed, z, s0, ns, skey, spay);
    return hipGetLastError();
}

hipError_t launch_gen_uniform_i64(unsigned long long seed, unsigned long long sid, long long lo, long long hi,
                                  long long i0, long long n, long long *key, long long *pay, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gen_uniform_i64, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, seed, sid, lo, hi, i0, n,
                       key, pay);
    return hipGetLastError();
}

hipError_t launch_gen_uniform_i32(unsigned long long seed, unsigned long long sid, int lo, int hi, long long i0,
                                  long long n, int *key, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gen_uniform_i32, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, seed, sid, lo, hi, i0, n,
                       key);
    return hipGetLastError();
}

hipError_t launch_key_col_i32(const int *t, long long rows, long long ld, int *out, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_key_col_i32, dim3(grid_for(rows, kBlock)), dim3(kBlock), 0, st, t, rows, ld, out);
    return hipGetLastError();
}

hipError_t launch_gather_rows_i32(const int *x, long long ldx, int cx, const int *y, long long ldy, int cy,
                                  const int *px, const int *py, const unsigned long long *count, long long cap,
                                  int *out, long long ldo, hipStream_t st) {
    if (cap <= 0) return hipSuccess;
    const long long elems = cap * (long long)(cx + cy - 1);
    unsigned g = grid_for(elems, kBlock * 4);
    if (g > 65536u) g = 65536u;   // grid-stride beyond
    hipLaunchKernelGGL(k_gather_rows_i32, dim3(g), dim3(kBlock), 0, st, x, ldx, cx, y, ldy, cy, px, py, count, cap,
                       out, ldo);
    return hipGetLastError();
}

static size_t select_tiles_of(long long n, long long tile) { return (size_t)(n > 0 ? (n + tile - 1) / tile : 0); }

size_t select_tiles(long long n) {   // upper bound over element types (int64 tiles hold fewer elements)
    return select_tiles_of(n, SelVec<long long>::kTile);
}

template <typename V>
static hipError_t launch_select_t(const V *in, long long n, int op, V c, V *out, long long *out_row, long long cap,
                                  unsigned long long *count, unsigned long long *tiles, unsigned long long *sums,
                                  hipStream_t st) {
    const unsigned nt = (unsigned)select_tiles_of(n, SelVec<V>::kTile);
    if (nt == 0) return hipMemsetAsync(count, 0, sizeof(unsigned long long), st);
    const bool vec_ok = (((uintptr_t)in) & 15) == 0;
    hipLaunchKernelGGL((k_sel_count<V>), dim3(nt), dim3(kBlock), 0, st, in, n, op, c, vec_ok, tiles);
    hipError_t e = hipMemsetAsync(tiles + nt, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    e = exclusive_scan_u64(tiles, (unsigned long long)nt + 1, sums, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_sel_write<V>), dim3(nt), dim3(kBlock), 0, st, in, n, op, c, vec_ok,
                       (const unsigned long long *)tiles, nt, out, out_row, cap, count);
    return hipGetLastError();
}

hipError_t launch_select_f32(const float *in, long long n, int op, float c, float *out, long long *out_row,
                             long long cap, unsigned long long *count, unsigned long long *tiles,
                             unsigned long long *sums, hipStream_t st) {
    return launch_select_t<float>(in, n, op, c, out, out_row, cap, count, tiles, sums, st);
}

hipError_t launch_select_i64(const long long *in, long long n, int op, long long c, long long *out,
                             long long *out_row, long long cap, unsigned long long *count, unsigned long long *tiles,
                             unsigned long long *sums, hipStream_t st) {
    return launch_select_t<long long>(in, n, op, c, out, out_row, cap, count, tiles, sums, st);
}

// ------------------------------------------------------------ copy floors
// The box's own streamed-copy rate, so a bench line can say how far each
// phase is from it.  16-B rows, non-temporal
// loads and stores (the partition passes' access flavour).
typedef unsigned long long cp_u64;
typedef __attribute__((ext_vector_type(2))) unsigned long long cp_v2;

__device__ __forceinline__ cp_v2 cp_ld(const cp_v2 *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void cp_st(cp_v2 *p, cp_v2 v) { __builtin_nontemporal_store(v, p); }

// one row per thread over the whole grid (n / 256 workgroups): the chip's
// best copy shape (6.2-6.4 TB/s, profiles/r04_copy_and_interleave.txt)
__global__ __launch_bounds__(256) void k_copy_flat(const cp_v2 *__restrict__ in, cp_v2 *__restrict__ out, cp_u64 n) {
    const cp_u64 i = (cp_u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) cp_st(out + i, cp_ld(in + i));
}

// the partition passes' loop shape: one 1024-thread workgroup per CU walks a
// contiguous range of 4096-row tiles with the next tile's loads in flight
// during this tile's stores
constexpr int kCpNT = 1024, kCpIT = 4;
__global__ __launch_bounds__(kCpNT) void k_copy_persistent(const cp_v2 *__restrict__ in, cp_v2 *__restrict__ out,
                                                           cp_u64 n) {
    constexpr cp_u64 T = (cp_u64)kCpNT * kCpIT;
    const cp_u64 tiles = n / T;
    const cp_u64 t0 = (cp_u64)blockIdx.x * tiles / gridDim.x, t1 = (cp_u64)(blockIdx.x + 1) * tiles / gridDim.x;
    cp_v2 r[kCpIT], q[kCpIT];
    if (t0 < t1)
#pragma unroll
        for (int i = 0; i < kCpIT; ++i) r[i] = cp_ld(in + t0 * T + (cp_u64)i * kCpNT + threadIdx.x);
    for (cp_u64 t = t0; t < t1; ++t) {
        if (t + 1 < t1)
#pragma unroll
            for (int i = 0; i < kCpIT; ++i) q[i] = cp_ld(in + (t + 1) * T + (cp_u64)i * kCpNT + threadIdx.x);
#pragma unroll
        for (int i = 0; i < kCpIT; ++i) cp_st(out + t * T + (cp_u64)i * kCpNT + threadIdx.x, r[i]);
#pragma unroll
        for (int i = 0; i < kCpIT; ++i) r[i] = q[i];
    }
    // rows past the last whole tile (n % T): the last workgroup, one per thread
    if (blockIdx.x == gridDim.x - 1)
        for (cp_u64 i = tiles * T + threadIdx.x; i < n; i += kCpNT) cp_st(out + i, cp_ld(in + i));
}

hipError_t launch_stream_copy(const void *in, void *out, long long rows, int shape, int cus, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    const cp_v2 *s = (const cp_v2 *)in;
    cp_v2 *d = (cp_v2 *)out;
    if (shape == 0)
        hipLaunchKernelGGL(k_copy_persistent, dim3(cus > 0 ? cus : 1), dim3(kCpNT), 0, st, s, d, (cp_u64)rows);
    else
        hipLaunchKernelGGL(k_copy_flat, dim3(grid_for(rows, 256)), dim3(256), 0, st, s, d, (cp_u64)rows);
    return hipGetLastError();
}

// ------------------------------------------------------- placement probe
// The partition passes write, per 4096-row tile, one 128-B line into each of
// ~512 open 1024-row buckets of the workgroup's own bucket range.  Into some
// physical placements of the destination buffer that pattern runs 25-35 %
// slower than a flat write of the same bytes; it is a property of the
// allocation (bimodal, reproducible per buffer, the flat write and flat read
// never vary, contiguous allocations are slow more often:
// profiles/r05/r05t_place_micro.txt, r05u_*).  placement_probe writes the
// pass's pattern (synthetic rows, every workgroup in its own range) and a flat
// stream of the same bytes into a fresh buffer; ratio = pattern / flat.
// (nb = 128 / 256 / 512 open buckets per workgroup: nb / 128 lines per
// thread group of 8 lanes per tile; buckets of 2^lpb_log 128-B lines)
__global__ __launch_bounds__(1024) void k_place_pattern(cp_v2 *__restrict__ out, unsigned tpw, cp_u64 wrows,
                                                        unsigned nb, unsigned lpb_log) {
    const unsigned w = blockIdx.x, tid = threadIdx.x;
    const cp_u64 base = (cp_u64)w * wrows;
    const cp_v2 val = {(cp_u64)w, 1ull};
    const unsigned lmask = (1u << lpb_log) - 1u;
    for (unsigned t = 0; t < tpw; ++t)
        for (unsigned i = 0; i < nb / 128u; ++i) {
            const unsigned j = i * 128u + (tid >> 3);   // the line's bin
            cp_st(out + base + ((((cp_u64)(t >> lpb_log) * nb + j) << lpb_log) + (t & lmask)) * 8u + (tid & 7u), val);
        }
}

__global__ __launch_bounds__(256) void k_place_flat(cp_v2 *__restrict__ out, cp_u64 n) {
    const cp_u64 i = (cp_u64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) cp_st(out + i, cp_v2{i, 2ull});
}

hipError_t placement_probe(void *buf, size_t bytes, size_t bucket_bytes, int cus, float *ratio) {
    *ratio = 0.0f;
    if (cus <= 0 || !buf) return hipErrorInvalidValue;
    // 128-B lines per bucket (a power of two, 8 .. 128)
    unsigned lpb_log = 3;
    while (lpb_log < 7 && (size_t(128) << (lpb_log + 1)) <= bucket_bytes) ++lpb_log;
    const cp_u64 bv2 = (cp_u64)8 << lpb_log;   // 16-B units per bucket
    // every workgroup's range: whole buckets, >= two per bin (512 bins; 256 /
    // 128 in smaller buffers)
    const cp_u64 wrows = ((cp_u64)(bytes / 16) / (cp_u64)cus) / bv2 * bv2;
    const cp_u64 buckets = wrows / bv2;
    const unsigned nb = buckets >= 1024 ? 512u : buckets >= 512 ? 256u : 128u;
    if (buckets < 256) return hipErrorInvalidValue;
    // tiles per workgroup: a bin's buckets (t >> lpb_log) stay inside the range
    const cp_u64 tw = (buckets / nb - 1) << lpb_log;
    const unsigned tpw = (unsigned)(tw > 512 ? 512 : tw);
    const cp_u64 flat = (cp_u64)tpw * 8u * nb * (cp_u64)cus;   // the same rows, streamed
    cp_v2 *out = (cp_v2 *)buf;
    hipEvent_t e[4];
    hipError_t err = hipSuccess;
    int made = 0;
    for (; made < 4 && err == hipSuccess; ++made) err = hipEventCreate(&e[made]);
    float best_p = 1e30f, best_f = 1e30f;
    for (int rep = 0; rep < 3 && err == hipSuccess; ++rep) {
        // rep 0 warms up (first touch of the pages), reps 1-2 are kept
        err = hipEventRecord(e[0], 0);
        hipLaunchKernelGGL(k_place_pattern, dim3(cus), dim3(1024), 0, 0, out, tpw, wrows, nb, lpb_log);
        if (err == hipSuccess) err = hipEventRecord(e[1], 0);
        hipLaunchKernelGGL(k_place_flat, dim3((unsigned)((flat + 255) / 256)), dim3(256), 0, 0, out, flat);
        if (err == hipSuccess) err = hipEventRecord(e[2], 0);
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipEventSynchronize(e[2]);
        float tp = 0.0f, tf = 0.0f;
        if (err == hipSuccess) err = hipEventElapsedTime(&tp, e[0], e[1]);
        if (err == hipSuccess) err = hipEventElapsedTime(&tf, e[1], e[2]);
        if (rep > 0 && err == hipSuccess) {
            if (tp < best_p) best_p = tp;
            if (tf < best_f) best_f = tf;
        }
    }
    for (int i = 0; i < made; ++i) (void)hipEventDestroy(e[i]);
    if (err == hipSuccess) *ratio = best_f > 0.0f ? best_p / best_f : 0.0f;
    return err;
}

}  // namespace hj
