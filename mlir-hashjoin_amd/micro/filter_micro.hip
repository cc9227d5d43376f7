// filter_micro.hip -- the two forms of the key filter's insert and apply, timed
// side by side (csrc/hj_filter.hip names the one the library launches).
//   insert: always issue the four 64-bit atomic ORs / read the block first and
//           issue only the ORs that still lack a bit; unique keys and keys that
//           repeat 16 times, 2^20 and 2^24 keys at 16 bits per key.
//   apply:  the write launch tests the filter again / the count launch leaves one
//           bit per row; PASS, all three outputs, half the rows pass; 2^26 and
//           2^28 rows against filters of 2 MiB, 32 MiB and 512 MiB.
// Includes the kernels' source, links libhj.so for the scan and the CU count.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../include -I../csrc -o filter_micro filter_micro.hip \
//        -L../lib -lhj   (and the library's directory in the run-time search path)
// Prints one JSON line per measurement: 2 warm-up runs, then 7 timed; median [min, max] in ms.
#include "../csrc/hj_filter.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1);} } while (0)
typedef unsigned long long u64;
constexpr u64 kGold = 0x9E3779B97F4A7C15ull;

// build keys: row i -> kGold * (i / rep); probe keys: odd rows hit a build key, even rows miss
__global__ void k_gen_build(long long *k, u64 n, u64 rep) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) k[i] = (long long)(kGold * (i / rep));
}
__global__ void k_gen_probe(long long *k, long long *p, u64 n, u64 nbuild) {
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) {
        const u64 h = hj::fmix64(i);
        k[i] = (long long)(kGold * ((i & 1) ? h % nbuild : nbuild + i));
        p[i] = (long long)i;
    }
}

static void timed(const char *what, const std::function<void()> &run, const std::function<void()> &before) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int it = 0; it < 9; ++it) {
        before();
        CK(hipEventRecord(e0, nullptr));
        run();
        CK(hipEventRecord(e1, nullptr));
        CK(hipEventSynchronize(e1));
        float t;
        CK(hipEventElapsedTime(&t, e0, e1));
        if (it >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    printf("%s \"ms\": {\"median\": %.4f, \"min\": %.4f, \"max\": %.4f}}\n", what, ms[ms.size() / 2], ms.front(), ms.back());
    fflush(stdout);
}

int main(int argc, char **argv) {
    const bool big = argc < 2 || atoi(argv[1]) != 0;   // 0: the small sizes only
    char buf[512];
    // ---- insert
    for (int lg : {20, 24}) {
        for (u64 rep : {1ull, 16ull}) {
            const u64 n = 1ull << lg, nblocks = (n / rep) * 16 / 256;
            long long *keys;
            unsigned *words;
            CK(hipMalloc(&keys, n * 8));
            CK(hipMalloc(&words, nblocks * 32));
            k_gen_build<<<4096, 256>>>(keys, n, rep);
            for (int form = 0; form < 2; ++form) {
                snprintf(buf, sizeof buf, "{\"op\": \"insert\", \"form\": \"%s\", \"keys\": %llu, \"repeat\": %llu, \"filter_bytes\": %llu,",
                         form ? "read-first" : "always", n, rep, nblocks * 32);
                auto before = [&] { CK(hj::filter_clear(words, (long long)nblocks, nullptr)); };
                auto run = [&] {
                    CK(form ? hj::filter_insert_t<true>(words, (long long)nblocks, hj::kCols64, keys, (long long)n, nullptr)
                            : hj::filter_insert_t<false>(words, (long long)nblocks, hj::kCols64, keys, (long long)n, nullptr));
                };
                timed(buf, run, before);
            }
            CK(hipFree(keys));
            CK(hipFree(words));
        }
    }
    // ---- apply
    for (int lg : {26, 28}) {
        if (lg == 28 && !big) continue;
        const u64 n = 1ull << lg;
        long long *sk, *sp, *ok, *op, *orow;
        u64 *count;
        for (long long **p : {&sk, &sp, &ok, &op, &orow}) CK(hipMalloc(p, n * 8));
        CK(hipMalloc(&count, 8));
        const size_t nt = hj::filter_tiles((long long)n) + 1;
        hj::FilterWork ws;
        CK(hipMalloc(&ws.tiles, nt * 8));
        CK(hipMalloc(&ws.sums, hj::exclusive_scan_sums(nt) * 8));
        CK(hipMalloc(&ws.bitmap, nt * hj::kFilterBlock));
        for (u64 mib : {2ull, 32ull, 512ull}) {
            const u64 nblocks = (mib << 20) / 32, nbuild = nblocks * 256 / 16;
            long long *rk;
            unsigned *words;
            CK(hipMalloc(&rk, nbuild * 8));
            CK(hipMalloc(&words, nblocks * 32));
            k_gen_build<<<4096, 256>>>(rk, nbuild, 1);
            k_gen_probe<<<4096, 256>>>(sk, sp, n, nbuild);
            CK(hj::filter_clear(words, (long long)nblocks, nullptr));
            CK(hj::filter_insert(words, (long long)nblocks, hj::kCols64, rk, (long long)nbuild, nullptr));
            for (int form = 0; form < 2; ++form) {
                auto run = [&] {
                    CK(form ? hj::filter_apply_t<true>(words, (long long)nblocks, hj::kCols64, 0, sk, sp, (long long)n, 0, ok, op,
                                                       orow, (long long)n, count, ws, nullptr)
                            : hj::filter_apply_t<false>(words, (long long)nblocks, hj::kCols64, 0, sk, sp, (long long)n, 0, ok, op,
                                                        orow, (long long)n, count, ws, nullptr));
                };
                run();
                u64 m = 0;
                CK(hipMemcpy(&m, count, 8, hipMemcpyDeviceToHost));
                snprintf(buf, sizeof buf, "{\"op\": \"apply\", \"form\": \"%s\", \"rows\": %llu, \"filter_bytes\": %llu, \"kept\": %llu,",
                         form ? "bitmap" : "test-twice", n, nblocks * 32, m);
                timed(buf, run, [] {});
            }
            CK(hipFree(rk));
            CK(hipFree(words));
        }
        for (void *p : {(void *)sk, (void *)sp, (void *)ok, (void *)op, (void *)orow, (void *)count, (void *)ws.tiles, (void *)ws.sums,
                        (void *)ws.bitmap})
            CK(hipFree(p));
    }
    return 0;
}
