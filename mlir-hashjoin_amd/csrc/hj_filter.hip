// hj_filter.hip -- the key filter: a split-block Bloom filter of a build
// side's keys (include/hj.h "Key filter").  nblocks blocks of 32 bytes, eight
// uint32 words each; a key sets or tests one bit in each word of ONE block, so
// a test reads one 32-byte sector and an insert touches one.
//
// Kernels.  k_filter_clear and k_filter_merge are 16-byte streams over the
// words.  k_filter_insert, k_filter_count and k_filter_write have hj_keys.hip's
// stream shape: a bounded grid (kFilterGridPerCu workgroups per CU) strides
// over tiles of kFilterTile rows, a lane owns groups of W consecutive rows
// (W = 2 for an int64 column, 4 for an int32 column, 1 for 16-byte {key, pay}
// tuples) read with one 16-byte non-temporal load per group when the column
// is 16-byte aligned and the group whole, else row by row; a tile's key loads
// are all issued before the first is used.
//
// Insert: per key the block and the eight masks, ORed in as four 64-bit
// no-return agent-scope atomics (words 2j and 2j + 1 pair into one).  Two
// forms, template READ_FIRST: issue the four always, or read the block first
// (two 16-byte loads) and issue an atomic only for a pair that still lacks a
// bit -- insert only ever sets bits and the clear is an earlier kernel, so a
// stale read can only show a bit as missing and cost a redundant atomic.
// kFilterInsertReadFirst (below) names the form the library launches;
// micro/filter_micro.hip times both.
//
// Apply = launch_select_t's shape: k_filter_count leaves every tile's number
// of qualifying rows in tile_cnt (and a zero behind them), exclusive_scan_u64
// turns them into offsets, k_filter_write compacts in row order (per-lane
// counts, a wave prefix sum, one (group, wave) scan per tile) and writes the
// counter.  Two forms, template BITMAP: the write launch tests the filter
// again, or the count launch leaves each lane's eight result bits as one byte
// of the workspace (tile * 256 + thread) and the write launch reads that byte
// and never touches the filter.  kFilterApplyBitmap names the form kept.
#include <type_traits>

#include "hj_internal.h"

namespace hj {

// The forms the library launches ("Key filter": the measurements).
constexpr bool kFilterInsertReadFirst = true;
constexpr bool kFilterApplyBitmap = true;

namespace {

typedef unsigned long long u64;
typedef long long i64;
typedef __attribute__((ext_vector_type(2))) unsigned long long fv2;   // 16 B of int64
typedef __attribute__((ext_vector_type(4))) int fi4;                  // 16 B of int32
typedef __attribute__((ext_vector_type(4))) unsigned fu4;             // 16 B of filter words

constexpr int kRowsPerLane = kFilterTile / kFilterBlock;   // 8
constexpr int kWaves = kFilterBlock / 64;

template <int FORM>
struct FilterShape {
    static constexpr int W = FORM == kCols64 ? 2 : (FORM == kCol32 ? 4 : 1);   // rows per 16-byte load
    static constexpr int G = kRowsPerLane / W;                                 // groups per lane and tile
};

// The W keys (sign-extended) of one lane's group at row r0, and for tuples the
// payload: one 16-byte load when the column is 16-byte aligned and the group
// whole, else one guarded load per row (rows at or past n read nothing).
template <int FORM>
__device__ __forceinline__ void filter_load(const void *col, bool vec_ok, i64 r0, i64 n,
                                            i64 (&k)[FilterShape<FORM>::W], i64 &tpay) {
    constexpr int W = FilterShape<FORM>::W;
    const bool whole = r0 + W <= n;
    tpay = 0;
    if constexpr (FORM == kCols64) {
        const i64 *p = (const i64 *)col + r0;
        if (vec_ok && whole) {
            const fv2 u = __builtin_nontemporal_load((const fv2 *)p);
            k[0] = (i64)u.x;
            k[1] = (i64)u.y;
        } else {
#pragma unroll
            for (int w = 0; w < W; ++w) k[w] = r0 + w < n ? __builtin_nontemporal_load(p + w) : 0;
        }
    } else if constexpr (FORM == kCol32) {
        const int *p = (const int *)col + r0;
        if (vec_ok && whole) {
            const fi4 u = __builtin_nontemporal_load((const fi4 *)p);
#pragma unroll
            for (int w = 0; w < W; ++w) k[w] = (i64)u[w];
        } else {
#pragma unroll
            for (int w = 0; w < W; ++w) k[w] = r0 + w < n ? (i64)__builtin_nontemporal_load(p + w) : 0;
        }
    } else {
        const i64 *p = (const i64 *)col + 2 * r0;
        if (vec_ok && whole) {
            const fv2 u = __builtin_nontemporal_load((const fv2 *)p);
            k[0] = (i64)u.x;
            tpay = (i64)u.y;
        } else if (whole) {
            k[0] = __builtin_nontemporal_load(p);
            tpay = __builtin_nontemporal_load(p + 1);
        } else {
            k[0] = 0;
        }
    }
}

// One column value of a lane's group (apply's payload column): as filter_load's int64 path.
__device__ __forceinline__ void filter_load_pay(const i64 *pay, bool vec_ok, i64 r0, i64 n, i64 (&v)[2]) {
    const i64 *p = pay + r0;
    if (vec_ok && r0 + 2 <= n) {
        const fv2 u = __builtin_nontemporal_load((const fv2 *)p);
        v[0] = (i64)u.x;
        v[1] = (i64)u.y;
    } else {
#pragma unroll
        for (int w = 0; w < 2; ++w) v[w] = r0 + w < n ? __builtin_nontemporal_load(p + w) : 0;
    }
}

struct Place {
    u64 block;
    unsigned lo;
};
__device__ __forceinline__ Place place_of(i64 key, u64 nblocks) {
    const u64 h = filter_hash(key);
    return Place{filter_block(h, nblocks), (unsigned)h};
}

// Does the block hold all eight bits of the key whose low hash word is lo?
__device__ __forceinline__ bool block_has(const fu4 &a, const fu4 &b, unsigned lo) {
    unsigned miss = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        miss |= ~a[w] & filter_mask(lo, w);
        miss |= ~b[w] & filter_mask(lo, w + 4);
    }
    return miss == 0;
}

__global__ __launch_bounds__(kFilterBlock) void k_filter_clear(fu4 *words16, u64 n16) {
    const fu4 z = {0u, 0u, 0u, 0u};
    for (u64 i = (u64)blockIdx.x * kFilterBlock + threadIdx.x; i < n16; i += (u64)gridDim.x * kFilterBlock)
        words16[i] = z;
}

__global__ __launch_bounds__(kFilterBlock) void k_filter_merge(fu4 *dst, const fu4 *src, u64 n16) {
    for (u64 i = (u64)blockIdx.x * kFilterBlock + threadIdx.x; i < n16; i += (u64)gridDim.x * kFilterBlock) {
        const fu4 a = dst[i], b = __builtin_nontemporal_load(src + i);
        dst[i] = a | b;
    }
}

template <int FORM, bool READ_FIRST>
__global__ __launch_bounds__(kFilterBlock) void k_filter_insert(unsigned *words, u64 nblocks, const void *key,
                                                                bool vec_ok, i64 n) {
    constexpr int W = FilterShape<FORM>::W, G = FilterShape<FORM>::G;
    for (i64 base = (i64)blockIdx.x * kFilterTile; base < n; base += (i64)gridDim.x * kFilterTile) {
        i64 k[G][W], unused;
#pragma unroll
        for (int g = 0; g < G; ++g)
            filter_load<FORM>(key, vec_ok, base + ((i64)g * kFilterBlock + threadIdx.x) * W, n, k[g], unused);
        Place pl[G][W];
        fu4 cur[READ_FIRST ? G : 1][READ_FIRST ? W : 1][2];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 r0 = base + ((i64)g * kFilterBlock + threadIdx.x) * W;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                pl[g][w] = place_of(k[g][w], nblocks);
                if (READ_FIRST && r0 + w < n) {
                    const fu4 *b = (const fu4 *)(words + pl[g][w].block * 8);
                    cur[READ_FIRST ? g : 0][READ_FIRST ? w : 0][0] = b[0];
                    cur[READ_FIRST ? g : 0][READ_FIRST ? w : 0][1] = b[1];
                }
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 r0 = base + ((i64)g * kFilterBlock + threadIdx.x) * W;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                if (r0 + w >= n) continue;
                u64 *b = (u64 *)(words + pl[g][w].block * 8);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u64 m = (u64)filter_mask(pl[g][w].lo, 2 * j) | ((u64)filter_mask(pl[g][w].lo, 2 * j + 1) << 32);
                    if (READ_FIRST) {
                        const fu4 &c = cur[READ_FIRST ? g : 0][READ_FIRST ? w : 0][j >> 1];
                        const u64 have = (u64)c[(j & 1) * 2] | ((u64)c[(j & 1) * 2 + 1] << 32);
                        if ((~have & m) == 0) continue;
                    }
                    (void)__hip_atomic_fetch_or(b + j, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
}

// The rows of one lane's tile share that qualify, as bits in (group, w) order
// (bit g * W + w): tested against the filter.  kind: HJ_FILTER_PASS keeps the
// rows whose key passes, HJ_FILTER_REJECT the others.
template <int FORM>
__device__ __forceinline__ unsigned filter_test_tile(const unsigned *words, u64 nblocks, int kind, i64 base, i64 n,
                                                     const i64 (&k)[FilterShape<FORM>::G][FilterShape<FORM>::W]) {
    constexpr int W = FilterShape<FORM>::W, G = FilterShape<FORM>::G;
    fu4 blk[G][W][2];
    unsigned lo[G][W];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const i64 r0 = base + ((i64)g * kFilterBlock + threadIdx.x) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const Place pl = place_of(k[g][w], nblocks);
            lo[g][w] = pl.lo;
            const fu4 *b = (const fu4 *)(words + pl.block * 8);
            const fu4 z = {0u, 0u, 0u, 0u};
            const bool in = r0 + w < n;
            blk[g][w][0] = in ? b[0] : z;
            blk[g][w][1] = in ? b[1] : z;
        }
    }
    unsigned bits = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const i64 r0 = base + ((i64)g * kFilterBlock + threadIdx.x) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const bool has = block_has(blk[g][w][0], blk[g][w][1], lo[g][w]);
            if (r0 + w < n && has == (kind == 0)) bits |= 1u << (g * W + w);
        }
    }
    return bits;
}

// tile_cnt[t] = qualifying rows of tile t, tile_cnt[ntiles] = 0 (the scan's last word).
template <int FORM, bool BITMAP>
__global__ __launch_bounds__(kFilterBlock) void k_filter_count(const unsigned *words, u64 nblocks, int kind,
                                                               const void *key, bool vec_ok, i64 n, u64 *tile_cnt,
                                                               u64 ntiles, unsigned char *bitmap) {
    constexpr int W = FilterShape<FORM>::W, G = FilterShape<FORM>::G;
    __shared__ unsigned ws[kWaves];
    if (blockIdx.x == 0 && threadIdx.x == 0) tile_cnt[ntiles] = 0;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const i64 base = (i64)t * kFilterTile;
        i64 k[G][W], unused;
#pragma unroll
        for (int g = 0; g < G; ++g)
            filter_load<FORM>(key, vec_ok, base + ((i64)g * kFilterBlock + threadIdx.x) * W, n, k[g], unused);
        const unsigned bits = filter_test_tile<FORM>(words, nblocks, kind, base, n, k);
        if (BITMAP) bitmap[t * kFilterBlock + threadIdx.x] = (unsigned char)bits;
        unsigned c = (unsigned)__popc(bits);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned s = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) s += ws[w];
            tile_cnt[t] = s;
        }
        __syncthreads();
    }
}

struct FilterOut {
    void *key;    // int64 / int32 keys, or 16-byte tuples
    void *pay;    // int64 payloads (kCols64 only)
    void *row;    // int64 source positions; kCol32: int32 row ids
};

template <int FORM, bool BITMAP>
__global__ __launch_bounds__(kFilterBlock) void k_filter_write(const unsigned *words, u64 nblocks, int kind,
                                                               const void *key, const i64 *pay, unsigned vec, i64 n,
                                                               i64 row_base, const u64 *tile_off, u64 ntiles,
                                                               const unsigned char *bitmap, FilterOut out, i64 cap,
                                                               u64 *count) {
    constexpr int W = FilterShape<FORM>::W, G = FilterShape<FORM>::G;
    __shared__ unsigned s_cw[G * kWaves];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool need_key = !BITMAP || out.key != nullptr;
    const bool need_pay = FORM == kCols64 && out.pay != nullptr;
    for (u64 t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const i64 base = (i64)t * kFilterTile;
        i64 k[G][W], tp[G], pv[FORM == kCols64 ? G : 1][2];
        unsigned bits = BITMAP ? (unsigned)bitmap[t * kFilterBlock + threadIdx.x] : 0u;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 r0 = base + ((i64)g * kFilterBlock + threadIdx.x) * W;
            if (need_key) {
                filter_load<FORM>(key, vec & 1u, r0, n, k[g], tp[g]);
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) k[g][w] = 0;
                tp[g] = 0;
            }
            if constexpr (FORM == kCols64) {
                if (need_pay)
                    filter_load_pay(pay, (vec >> 1) & 1u, r0, n, pv[g]);
                else
                    pv[g][0] = pv[g][1] = 0;
            }
        }
        if (!BITMAP) bits = filter_test_tile<FORM>(words, nblocks, kind, base, n, k);
        unsigned lpre[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const unsigned c = (unsigned)__popc((bits >> (g * W)) & ((1u << W) - 1u));
            const unsigned xs = wave_incl_add(c);
            lpre[g] = xs - c;
            if (lane == 63) s_cw[g * kWaves + wv] = xs;
        }
        __syncthreads();
        if (threadIdx.x == 0) {   // (group, wave) runs in row order
            unsigned run = 0;
#pragma unroll
            for (int q = 0; q < G * kWaves; ++q) {
                const unsigned v = s_cw[q];
                s_cw[q] = run;
                run += v;
            }
        }
        __syncthreads();
        const u64 tb = tile_off[t];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            u64 o = tb + s_cw[g * kWaves + wv] + lpre[g];
            const i64 r0 = base + ((i64)g * kFilterBlock + threadIdx.x) * W;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                if (!((bits >> (g * W + w)) & 1u)) continue;
                if (o < (u64)cap) {
                    if constexpr (FORM == kCols64) {
                        if (out.key) ((i64 *)out.key)[o] = k[g][w];
                        if (out.pay) ((i64 *)out.pay)[o] = pv[g][w];
                        if (out.row) ((i64 *)out.row)[o] = r0 + w;
                    } else if constexpr (FORM == kCol32) {
                        if (out.key) ((int *)out.key)[o] = (int)k[g][w];
                        if (out.row) ((int *)out.row)[o] = (int)(row_base + r0 + w);
                    } else {
                        if (out.key) {
                            ((i64 *)out.key)[2 * o] = k[g][w];
                            ((i64 *)out.key)[2 * o + 1] = tp[g];
                        }
                        if (out.row) ((i64 *)out.row)[o] = r0 + w;
                    }
                }
                ++o;
            }
        }
        __syncthreads();   // s_cw is the next tile's too
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = tile_off[ntiles];
}

__global__ __launch_bounds__(64) void k_filter_zero_count(u64 *count) {
    if (threadIdx.x == 0) *count = 0;
}

unsigned capped_grid(u64 work_groups) {
    const u64 cap = (u64)cu_count() * kFilterGridPerCu;
    return (unsigned)(work_groups < cap ? (work_groups ? work_groups : 1) : cap);
}

inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

template <typename F>
hipError_t with_filter_form(int form, F &&f) {
    switch (form) {
        case kCols64: f(std::integral_constant<int, kCols64>()); break;
        case kPacked64: f(std::integral_constant<int, kPacked64>()); break;
        case kCol32: f(std::integral_constant<int, kCol32>()); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

template <bool READ_FIRST>
hipError_t filter_insert_t(unsigned *words, long long nblocks, int form, const void *key, long long n,
                           hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const unsigned grid = capped_grid(filter_tiles(n));
    return with_filter_form(form, [&](auto fc) {
        hipLaunchKernelGGL((k_filter_insert<decltype(fc)::value, READ_FIRST>), dim3(grid), dim3(kFilterBlock), 0, st,
                           words, (u64)nblocks, key, aligned16(key), (i64)n);
    });
}

template <bool BITMAP>
hipError_t filter_apply_t(const unsigned *words, long long nblocks, int form, int kind, const void *key,
                          const long long *pay, long long n, long long row_base, void *out_key, void *out_pay,
                          void *out_row, long long cap, unsigned long long *count, const FilterWork &ws,
                          hipStream_t st) {
    if (n <= 0) {
        hipLaunchKernelGGL(k_filter_zero_count, dim3(1), dim3(64), 0, st, count);
        return hipGetLastError();
    }
    const u64 nt = filter_tiles(n);
    const unsigned grid = capped_grid(nt);
    const unsigned vec = (aligned16(key) ? 1u : 0u) | (aligned16(pay) ? 2u : 0u);
    hipError_t e = with_filter_form(form, [&](auto fc) {
        hipLaunchKernelGGL((k_filter_count<decltype(fc)::value, BITMAP>), dim3(grid), dim3(kFilterBlock), 0, st, words,
                           (u64)nblocks, kind, key, (vec & 1u) != 0, (i64)n, ws.tiles, nt, ws.bitmap);
    });
    if (e != hipSuccess) return e;
    e = exclusive_scan_u64(ws.tiles, nt + 1, ws.sums, st);
    if (e != hipSuccess) return e;
    const FilterOut out{out_key, out_pay, out_row};
    return with_filter_form(form, [&](auto fc) {
        hipLaunchKernelGGL((k_filter_write<decltype(fc)::value, BITMAP>), dim3(grid), dim3(kFilterBlock), 0, st, words,
                           (u64)nblocks, kind, key, (const i64 *)pay, vec, (i64)n, (i64)row_base,
                           (const u64 *)ws.tiles, nt, (const unsigned char *)ws.bitmap, out, (i64)cap, count);
    });
}

size_t filter_tiles(long long n) { return (size_t)(n > 0 ? (n + kFilterTile - 1) / kFilterTile : 0); }

size_t filter_bitmap_bytes(long long n) { return kFilterApplyBitmap ? filter_tiles(n) * kFilterBlock : 0; }

hipError_t filter_clear(unsigned *words, long long nblocks, hipStream_t st) {
    const u64 n16 = (u64)nblocks * 2;
    hipLaunchKernelGGL(k_filter_clear, dim3(capped_grid((n16 + kFilterBlock - 1) / kFilterBlock)), dim3(kFilterBlock),
                       0, st, (fu4 *)words, n16);
    return hipGetLastError();
}

hipError_t filter_merge(unsigned *words, const unsigned *other, long long nblocks, hipStream_t st) {
    const u64 n16 = (u64)nblocks * 2;
    hipLaunchKernelGGL(k_filter_merge, dim3(capped_grid((n16 + kFilterBlock - 1) / kFilterBlock)), dim3(kFilterBlock),
                       0, st, (fu4 *)words, (const fu4 *)other, n16);
    return hipGetLastError();
}

hipError_t filter_insert(unsigned *words, long long nblocks, int form, const void *key, long long n,
                         hipStream_t st) {
    return filter_insert_t<kFilterInsertReadFirst>(words, nblocks, form, key, n, st);
}

hipError_t filter_apply(const unsigned *words, long long nblocks, int form, int kind, const void *key,
                        const long long *pay, long long n, long long row_base, void *out_key, void *out_pay,
                        void *out_row, long long cap, unsigned long long *count, const FilterWork &ws,
                        hipStream_t st) {
    return filter_apply_t<kFilterApplyBitmap>(words, nblocks, form, kind, key, pay, n, row_base, out_key, out_pay,
                                              out_row, cap, count, ws, st);
}

}  // namespace hj
