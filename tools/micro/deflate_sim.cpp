// deflate_sim.cpp -- deflate.hip's member routine (fqtool_amd/csrc/deflate_core.h) run on the host:
// 256 real threads and a pthread barrier stand in for the workgroup, heap blocks of the exact sizes
// for its LDS, token array, source and slot, so a sanitizer sees every access (CPU only).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tools/micro/deflate_sim.cpp -o tools/micro/deflate_sim
//   tools/micro/deflate_sim IN LEVEL OUT.gz      (then e.g. `gzip -dc OUT.gz | cmp - IN`)
#include <stdint.h>
#include <pthread.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#define __host__
#define __device__
#define __global__
struct Dim3 { unsigned x; };
static thread_local Dim3 threadIdx;
struct uint4 { uint32_t x, y, z, w; };
static pthread_barrier_t g_bar;
static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
static inline uint32_t atomicAdd(uint32_t* p, uint32_t v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t atomicXor(uint32_t* p, uint32_t v) { return __atomic_fetch_xor(p, v, __ATOMIC_SEQ_CST); }
#include "../../fqtool_amd/csrc/deflate_core.h"
int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = fopen(argv[1], "rb");
    std::vector<uint8_t> in;
    { uint8_t b[65536]; size_t k; while ((k = fread(b, 1, sizeof b, f)) > 0) in.insert(in.end(), b, b + k); }
    fclose(f);
    const int level = atoi(argv[2]);
    const size_t n = in.size(), nmem = (n + 65279) / 65280;
    uint8_t* lds = (uint8_t*)aligned_alloc(16, FQ_DL_TOTAL);
    uint32_t* tok = (uint32_t*)malloc(65280 * 4);
    std::vector<std::vector<uint8_t>> outs(nmem);
    pthread_barrier_init(&g_bar, nullptr, 256);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < 256; ++t)
        th.emplace_back([&, t] {
            threadIdx.x = t;
            for (size_t m = 0; m < nmem; ++m) {
                static uint8_t* dst;
                if (t == 0) dst = (uint8_t*)malloc(65536);
                __syncthreads();
                const uint32_t len = (uint32_t)std::min<size_t>(65280, n - m * 65280);
                // the source copied to an exact-size block so that reads past it are caught
                static uint8_t* src;
                if (t == 0) { src = (uint8_t*)aligned_alloc(16, (len + 15) / 16 * 16 + 16); memcpy(src, in.data() + m * 65280, len); }
                __syncthreads();
                const uint32_t sz = fq_deflate_member(lds, src, len, level, tok, dst);
                __syncthreads();
                if (t == 0) { outs[m].assign(dst, dst + sz); free(dst); free(src); }
                __syncthreads();
            }
        });
    for (auto& x : th) x.join();
    FILE* o = fopen(argv[3], "wb");
    size_t total = 0;
    for (auto& v : outs) { fwrite(v.data(), 1, v.size(), o); total += v.size(); }
    fclose(o);
    free(lds);
    free(tok);
    printf("%zu -> %zu (%.4f)\n", n, total, n ? (double)total / n : 0.0);
    return 0;
}
