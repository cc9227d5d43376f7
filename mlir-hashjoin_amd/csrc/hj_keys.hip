// hj_keys.hip -- composite keys: exact range packing of up to four int32 /
// int64 key columns into one int64 key (include/hj.h "Composite keys").
//
// Five kernels.  k_keys_reset and k_keys_seal are single-workgroup kernels over
// the plan block (hj::KeyPlan, device memory).  k_keys_observe, k_keys_pack
// and k_keys_unpack are bandwidth-bound streams of one shape: a bounded grid
// (kKeysGridPerCu workgroups per CU) strides over tiles of kKeysTile rows; a
// lane owns groups of W consecutive rows (W = 2 when every column is int64,
// else 4), so that a column whose base is 16-byte aligned is read with 16-byte
// loads and the keys of a group leave in 16-byte non-temporal stores (the
// 16-byte {key, pay} rows of pack_tuples are first turned round in the wave's
// own piece of LDS, so that a store instruction writes 1 KiB in a row).  A
// column that is only element-aligned (a torch slice such as col[1:]) takes
// the element path -- the same rows per lane, one load per row -- and so does
// the ragged last group.  The column count and widths are uniform across the
// grid: the count is a template parameter and the widths a scalar mask, so
// neither costs the row path anything.  The plan is read from the device
// block (uniform loads), the column pointers travel in the kernel arguments.
#include <type_traits>

#include "hj_internal.h"

namespace hj {
namespace {

typedef unsigned long long u64;
typedef long long i64;
typedef __attribute__((ext_vector_type(2))) unsigned long long kv2;   // 16 B of int64
typedef __attribute__((ext_vector_type(4))) int ki4;                  // 16 B of int32

constexpr int kVecPay = 4, kVecOut = 5;   // bits of the alignment mask beside the columns' 0..3

// The W rows of one lane's group at row r0 of a column, sign-extended: one or
// two 16-byte loads when the column is 16-byte aligned and the group whole,
// else one guarded load per row (rows at or past n read nothing and give 0).
template <int W, bool NT>
__device__ __forceinline__ void keys_load(const void *col, bool is64, bool vec_ok, i64 r0, i64 n, i64 (&v)[W]) {
    const bool whole = r0 + W <= n;
    if (W == 2 || is64) {
        const i64 *p = (const i64 *)col + r0;
        if (vec_ok && whole) {
#pragma unroll
            for (int h = 0; h < W / 2; ++h) {
                const kv2 u = NT ? __builtin_nontemporal_load((const kv2 *)p + h) : *((const kv2 *)p + h);
                v[2 * h] = (i64)u.x;
                v[2 * h + 1] = (i64)u.y;
            }
        } else {
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = r0 + w < n ? (NT ? __builtin_nontemporal_load(p + w) : p[w]) : 0;
        }
    } else {
        const int *p = (const int *)col + r0;
        if (vec_ok && whole) {
            const ki4 u = NT ? __builtin_nontemporal_load((const ki4 *)p) : *(const ki4 *)p;
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = (i64)u[w];
        } else {
#pragma unroll
            for (int w = 0; w < W; ++w) v[w] = r0 + w < n ? (i64)(NT ? __builtin_nontemporal_load(p + w) : p[w]) : 0;
        }
    }
}

__global__ __launch_bounds__(64) void k_keys_reset(KeyPlan *plan) {
    if (threadIdx.x != 0) return;
    for (int c = 0; c < kKeysMaxCols; ++c) {
        plan->mn[c] = INT64_MAX;
        plan->mx[c] = INT64_MIN;
        plan->lo[c] = plan->hi[c] = 0;
        plan->span[c] = plan->mask[c] = 0;
        plan->bits[c] = plan->shift[c] = 0;
    }
    plan->rows = plan->oor = 0;
    plan->total = plan->range = 0;
}

// Per lane, then wave (shuffles), then workgroup (LDS); ONE signed 64-bit
// atomicMin and atomicMax per column and workgroup.
template <int NC, int W>
__global__ __launch_bounds__(kKeysBlock) void k_keys_observe(KeyPlan *plan, KeyCols cols, unsigned w64, unsigned vec,
                                                             i64 n) {
    constexpr int G = kKeysTile / (kKeysBlock * W);
    __shared__ i64 smn[kKeysBlock / 64][NC], smx[kKeysBlock / 64][NC];
    i64 mn[NC], mx[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) mn[c] = INT64_MAX, mx[c] = INT64_MIN;
    for (i64 base = (i64)blockIdx.x * kKeysTile; base < n; base += (i64)gridDim.x * kKeysTile) {
        i64 v[G][NC][W];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 r0 = base + ((i64)g * kKeysBlock + threadIdx.x) * W;
#pragma unroll
            for (int c = 0; c < NC; ++c) keys_load<W, false>(cols.p[c], (w64 >> c) & 1, (vec >> c) & 1, r0, n, v[g][c]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 r0 = base + ((i64)g * kKeysBlock + threadIdx.x) * W;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const bool in = r0 + w < n;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const i64 x = v[g][c][w];
                    mn[c] = in && x < mn[c] ? x : mn[c];
                    mx[c] = in && x > mx[c] ? x : mx[c];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const i64 a = __shfl_xor(mn[c], o, 64), b = __shfl_xor(mx[c], o, 64);
            mn[c] = a < mn[c] ? a : mn[c];
            mx[c] = b > mx[c] ? b : mx[c];
        }
        if ((threadIdx.x & 63) == 0) smn[threadIdx.x >> 6][c] = mn[c], smx[threadIdx.x >> 6][c] = mx[c];
    }
    __syncthreads();
    if (threadIdx.x < NC) {
        const int c = threadIdx.x;
        i64 a = smn[0][c], b = smx[0][c];
#pragma unroll
        for (int k = 1; k < kKeysBlock / 64; ++k) {
            a = smn[k][c] < a ? smn[k][c] : a;
            b = smx[k][c] > b ? smx[k][c] : b;
        }
        atomicMin(&plan->mn[c], a);
        atomicMax(&plan->mx[c], b);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&plan->rows, (u64)n);
}

__global__ __launch_bounds__(64) void k_keys_seal(KeyPlan *plan, int ncols) {
    if (threadIdx.x != 0) return;
    const bool any = plan->rows > 0;
    for (int c = 0; c < kKeysMaxCols; ++c) {
        const bool live = any && c < ncols;
        const i64 lo = live ? plan->mn[c] : 0, hi = live ? plan->mx[c] : 0;
        const u64 span = (u64)hi - (u64)lo;
        const int bits = span ? 64 - __clzll((i64)span) : 0;
        plan->lo[c] = lo;
        plan->hi[c] = hi;
        plan->span[c] = span;
        plan->bits[c] = bits;
        plan->mask[c] = bits == 64 ? ~0ull : (1ull << bits) - 1;
    }
    int below = 0;   // the widths of the columns after c
    for (int c = kKeysMaxCols - 1; c >= 0; --c) {
        plan->shift[c] = plan->bits[c] ? below : 0;   // a 0-bit column is masked out, never shifted (by up to 64)
        below += plan->bits[c];
    }
    plan->total = below;
    plan->range = below > 64 ? 1 : 0;
}

// The plan's per-column words, uniform across the grid.
template <int NC>
struct KeysPlanRegs {
    u64 lo[NC], span[NC], mask[NC];
    int shift[NC];
    __device__ __forceinline__ explicit KeysPlanRegs(const KeyPlan *__restrict__ plan) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            lo[c] = (u64)plan->lo[c];
            span[c] = plan->span[c];
            mask[c] = plan->mask[c];
            shift[c] = plan->shift[c];
        }
    }
};

// out: n keys, or (TUPLES) n 16-byte rows {key, pay}.  oor: the plan's
// out-of-range counter (a pointer of its own: the plan itself is read-only here).
template <int NC, int W, bool TUPLES>
__global__ __launch_bounds__(kKeysBlock) void k_keys_pack(const KeyPlan *__restrict__ plan, u64 *oor, KeyCols cols,
                                                          const i64 *pay, unsigned w64, unsigned vec, i64 n, u64 *out) {
    constexpr int G = kKeysTile / (kKeysBlock * W);
    if (plan->range) return;   // the joint range needs more than 64 bits: nothing is written
    const KeysPlanRegs<NC> pl(plan);
    __shared__ unsigned sbad[kKeysBlock / 64];
    __shared__ kv2 stage[TUPLES ? kKeysBlock * W : 1];   // TUPLES: 64 W tuples per wave (below)
    unsigned bad = 0;
    for (i64 base = (i64)blockIdx.x * kKeysTile; base < n; base += (i64)gridDim.x * kKeysTile) {
        i64 v[G][NC][W], pv[G][W];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 r0 = base + ((i64)g * kKeysBlock + threadIdx.x) * W;
#pragma unroll
            for (int c = 0; c < NC; ++c) keys_load<W, true>(cols.p[c], (w64 >> c) & 1, (vec >> c) & 1, r0, n, v[g][c]);
            if (TUPLES) keys_load<W, true>(pay, true, (vec >> kVecPay) & 1, r0, n, pv[g]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 r0 = base + ((i64)g * kKeysBlock + threadIdx.x) * W;
            u64 k[W];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                bool outside = false;
                k[w] = 0;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const u64 d = (u64)v[g][c][w] - pl.lo[c];
                    outside |= d > pl.span[c];
                    k[w] |= (d & pl.mask[c]) << pl.shift[c];
                }
                bad += outside && r0 + w < n ? 1u : 0u;
            }
            const bool vec_st = ((vec >> kVecOut) & 1) && r0 + W <= n;
            if (TUPLES) {
                // A lane's W rows are W 16-byte tuples 16 W bytes apart from the next lane's: stored
                // from where they are, every store instruction would write a 16-byte piece of each
                // 16 W bytes (measured: 3.4 TB/s).  The wave turns its 64 W tuples round in its own
                // piece of LDS, so that store s writes rows 64 s .. 64 s + 63 of the wave, 1 KiB in a row.
                kv2 *ws = stage + (threadIdx.x >> 6) * 64 * W;
                const int lane = threadIdx.x & 63;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    kv2 t;
                    t.x = k[w];
                    t.y = (u64)pv[g][w];
                    ws[lane * W + w] = t;
                }
                __builtin_amdgcn_wave_barrier();   // the wave's own LDS operations complete in order
                const i64 wr0 = base + ((i64)g * kKeysBlock + (threadIdx.x & ~63)) * W;   // the wave's first row
#pragma unroll
                for (int s = 0; s < W; ++s) {
                    const i64 row = wr0 + 64 * s + lane;
                    const kv2 t = ws[64 * s + lane];
                    if (row < n) {
                        if ((vec >> kVecOut) & 1) {
                            __builtin_nontemporal_store(t, (kv2 *)out + row);
                        } else {
                            __builtin_nontemporal_store(t.x, out + 2 * row);
                            __builtin_nontemporal_store(t.y, out + 2 * row + 1);
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
            } else if (vec_st) {
#pragma unroll
                for (int h = 0; h < W / 2; ++h) {
                    kv2 t;
                    t.x = k[2 * h];
                    t.y = k[2 * h + 1];
                    __builtin_nontemporal_store(t, (kv2 *)(out + r0) + h);
                }
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (r0 + w < n) __builtin_nontemporal_store(k[w], out + r0 + w);
            }
        }
    }
    // rows outside the sealed range: one add per workgroup, and only when there are any
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
    if ((threadIdx.x & 63) == 0) sbad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0;
#pragma unroll
        for (int k = 0; k < kKeysBlock / 64; ++k) t += sbad[k];
        if (t) atomicAdd(oor, (u64)t);
    }
}

template <int NC, int W>
__global__ __launch_bounds__(kKeysBlock) void k_keys_unpack(const KeyPlan *__restrict__ plan, const u64 *key,
                                                            KeyOutCols out, unsigned w64, unsigned vec, i64 n) {
    constexpr int G = kKeysTile / (kKeysBlock * W);
    if (plan->range) return;
    const KeysPlanRegs<NC> pl(plan);
    for (i64 base = (i64)blockIdx.x * kKeysTile; base < n; base += (i64)gridDim.x * kKeysTile) {
        i64 k[G][W];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 r0 = base + ((i64)g * kKeysBlock + threadIdx.x) * W;
            keys_load<W, true>(key, true, (vec >> kVecPay) & 1, r0, n, k[g]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const i64 r0 = base + ((i64)g * kKeysBlock + threadIdx.x) * W;
            const bool whole = r0 + W <= n;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (!out.p[c]) continue;
                u64 x[W];
#pragma unroll
                for (int w = 0; w < W; ++w) x[w] = pl.lo[c] + (((u64)k[g][w] >> pl.shift[c]) & pl.mask[c]);
                const bool vec_st = ((vec >> c) & 1) && whole;
                if (W == 2 || ((w64 >> c) & 1)) {
                    u64 *o = (u64 *)out.p[c] + r0;
                    if (vec_st) {
#pragma unroll
                        for (int h = 0; h < W / 2; ++h) {
                            kv2 t;
                            t.x = x[2 * h];
                            t.y = x[2 * h + 1];
                            __builtin_nontemporal_store(t, (kv2 *)o + h);
                        }
                    } else {
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            if (r0 + w < n) __builtin_nontemporal_store(x[w], o + w);
                    }
                } else {
                    int *o = (int *)out.p[c] + r0;
                    if (vec_st) {
                        ki4 t;
#pragma unroll
                        for (int w = 0; w < W; ++w) t[w] = (int)x[w];
                        __builtin_nontemporal_store(t, (ki4 *)o);
                    } else {
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            if (r0 + w < n) __builtin_nontemporal_store((int)x[w], o + w);
                    }
                }
            }
        }
    }
}

unsigned keys_grid(i64 n) {
    const i64 tiles = (n + kKeysTile - 1) / kKeysTile, cap = (i64)cu_count() * kKeysGridPerCu;
    return (unsigned)(tiles < cap ? tiles : cap);
}

inline unsigned aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0 ? 1u : 0u; }

constexpr unsigned kAll64[kKeysMaxCols + 1] = {0, 1, 3, 7, 15};

// f(NC, W) for the runtime column count and "every column is int64"
template <typename F>
hipError_t keys_dispatch(int ncols, bool all64, F &&f) {
#define HJ_KEYS_CASE(NC)                                                                  \
    case NC:                                                                              \
        if (all64)                                                                        \
            f(std::integral_constant<int, NC>(), std::integral_constant<int, 2>());       \
        else                                                                              \
            f(std::integral_constant<int, NC>(), std::integral_constant<int, 4>());       \
        break;
    switch (ncols) {
        HJ_KEYS_CASE(1)
        HJ_KEYS_CASE(2)
        HJ_KEYS_CASE(3)
        HJ_KEYS_CASE(4)
        default: return hipErrorInvalidValue;
    }
#undef HJ_KEYS_CASE
    return hipGetLastError();
}

}  // namespace

hipError_t keys_reset(KeyPlan *plan, hipStream_t st) {
    hipLaunchKernelGGL(k_keys_reset, dim3(1), dim3(64), 0, st, plan);
    return hipGetLastError();
}

hipError_t keys_seal(KeyPlan *plan, int ncols, hipStream_t st) {
    hipLaunchKernelGGL(k_keys_seal, dim3(1), dim3(64), 0, st, plan, ncols);
    return hipGetLastError();
}

hipError_t keys_observe(KeyPlan *plan, int ncols, unsigned w64, const KeyCols &cols, long long n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    unsigned vec = 0;
    for (int c = 0; c < ncols; ++c) vec |= aligned16(cols.p[c]) << c;
    const unsigned grid = keys_grid(n);
    return keys_dispatch(ncols, w64 == kAll64[ncols], [&](auto nc, auto w) {
        hipLaunchKernelGGL((k_keys_observe<decltype(nc)::value, decltype(w)::value>), dim3(grid), dim3(kKeysBlock), 0,
                           st, plan, cols, w64, vec, (i64)n);
    });
}

hipError_t keys_pack(KeyPlan *plan, int ncols, unsigned w64, const KeyCols &cols, const long long *pay, long long n,
                     unsigned long long *out, bool tuples, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    unsigned vec = (aligned16(pay) << kVecPay) | (aligned16(out) << kVecOut);
    for (int c = 0; c < ncols; ++c) vec |= aligned16(cols.p[c]) << c;
    const unsigned grid = keys_grid(n);
    return keys_dispatch(ncols, w64 == kAll64[ncols], [&](auto nc, auto w) {
        constexpr int NC = decltype(nc)::value, W = decltype(w)::value;
        if (tuples)
            hipLaunchKernelGGL((k_keys_pack<NC, W, true>), dim3(grid), dim3(kKeysBlock), 0, st, plan, &plan->oor, cols,
                               pay, w64, vec, (i64)n, out);
        else
            hipLaunchKernelGGL((k_keys_pack<NC, W, false>), dim3(grid), dim3(kKeysBlock), 0, st, plan, &plan->oor, cols,
                               pay, w64, vec, (i64)n, out);
    });
}

hipError_t keys_unpack(const KeyPlan *plan, int ncols, unsigned w64, const unsigned long long *key, long long n,
                       const KeyOutCols &out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    unsigned vec = aligned16(key) << kVecPay;
    for (int c = 0; c < ncols; ++c) vec |= aligned16(out.p[c]) << c;
    const unsigned grid = keys_grid(n);
    return keys_dispatch(ncols, w64 == kAll64[ncols], [&](auto nc, auto w) {
        hipLaunchKernelGGL((k_keys_unpack<decltype(nc)::value, decltype(w)::value>), dim3(grid), dim3(kKeysBlock), 0,
                           st, plan, key, out, w64, vec, (i64)n);
    });
}

}  // namespace hj
