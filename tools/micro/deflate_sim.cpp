// deflate_sim.cpp -- deflate.hip's member routine (fqtool_amd/csrc/deflate_core.h) run on the host:
// 256 real threads and a pthread barrier stand in for the workgroup, heap blocks of the exact sizes
// for its LDS, token array, source and slot, so a sanitizer sees every access (CPU only).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tools/micro/deflate_sim.cpp -o tools/micro/deflate_sim
//   tools/micro/deflate_sim IN LEVEL OUT.gz      (then e.g. `gzip -dc OUT.gz | cmp - IN`)
// Span mode: the multi-span kernels' two walks (one workgroup walking every member) over a table of
// up to 6 spans, the scratch holding MEMBERS slots:
//   tools/micro/deflate_sim --spans LEVEL MEMBERS OUT SPAN...      SPAN = FILE:WORD:CAP, or - (no span)
// FILE's bytes are the text (at most CAP are loaded), WORD is the span's length word (clamped to CAP
// by the walks), and the span's buffer is a heap block of exactly fq_deflate_bound(CAP) bytes, which
// the members are compacted into in place.  Writes OUT.<k> (span k's stream) and prints
// "span <k> <total>" per span and "overflow <0|1>" (1: the error word's bit 1 was set).
#include <stdint.h>
#include <pthread.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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
static inline int atomicOr(int* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t atomicXor(uint32_t* p, uint32_t v) { return __atomic_fetch_xor(p, v, __ATOMIC_SEQ_CST); }
#include "../../fqtool_amd/csrc/deflate_core.h"

static std::vector<uint8_t> read_file(const char* path) {
    std::vector<uint8_t> in;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    uint8_t b[65536];
    size_t k;
    while ((k = fread(b, 1, sizeof b, f)) > 0) in.insert(in.end(), b, b + k);
    fclose(f);
    return in;
}

static int spans_main(int argc, char** argv) {
    if (argc < 6 || argc > 5 + FQ_DEFL_SPANS) return 2;
    const int level = atoi(argv[2]);
    const unsigned long long members = strtoull(argv[3], nullptr, 10);
    const std::string out = argv[4];
    fq_span_table t{};
    unsigned long long words[FQ_DEFL_SPANS] = {};
    size_t alloc[FQ_DEFL_SPANS] = {};
    for (int k = 0; k < argc - 5; ++k) {
        const std::string a = argv[5 + k];
        if (a == "-") continue;
        const size_t c2 = a.rfind(':'), c1 = a.rfind(':', c2 - 1);
        if (c2 == std::string::npos || c1 == std::string::npos) return 2;
        const std::vector<uint8_t> in = read_file(a.substr(0, c1).c_str());
        words[k] = strtoull(a.c_str() + c1 + 1, nullptr, 10);
        t.cap[k] = strtoull(a.c_str() + c2 + 1, nullptr, 10);
        alloc[k] = t.cap[k] + 31 * ((t.cap[k] + FQ_DEFL_MEMBER_IN - 1) / FQ_DEFL_MEMBER_IN);
        t.text[k] = (uint8_t*)malloc(std::max<size_t>(1, alloc[k]));  // (16-byte aligned, as the device buffers)
        if (!in.empty()) memcpy(t.text[k], in.data(), std::min<size_t>(in.size(), t.cap[k]));
        t.n[k] = &words[k];
    }
    uint8_t* lds = (uint8_t*)aligned_alloc(16, FQ_DL_TOTAL);
    uint32_t* tok = (uint32_t*)malloc(65280 * 4);
    uint8_t* slots = (uint8_t*)malloc(std::max<size_t>(1, members) * FQ_DEFL_SLOT);
    uint32_t* sizes = (uint32_t*)malloc(std::max<size_t>(1, members) * sizeof(uint32_t));
    unsigned long long* part = (unsigned long long*)malloc(256 * sizeof(unsigned long long));
    unsigned long long totals[FQ_DEFL_SPANS];
    for (auto& x : totals) x = ~0ull;  // (every total must be written)
    int err = 0;
    pthread_barrier_init(&g_bar, nullptr, 256);
    std::vector<std::thread> th;
    for (unsigned i = 0; i < 256; ++i)
        th.emplace_back([&, i] {
            threadIdx.x = i;
            fq_deflate_spans_walk(lds, t, members, level, tok, slots, sizes, 0, 1);
            __syncthreads();  // (the kernel boundary)
            fq_compact_spans_walk(part, t, members, slots, sizes, totals, &err, 0, 1);
        });
    for (auto& x : th) x.join();
    int rc = 0;
    for (int k = 0; k < FQ_DEFL_SPANS; ++k) {
        if (totals[k] == ~0ull || totals[k] > alloc[k]) {
            fprintf(stderr, "span %d: total %llu not written or past the buffer\n", k, totals[k]);
            rc = 1;
            continue;
        }
        printf("span %d %llu\n", k, totals[k]);
        FILE* o = fopen((out + "." + std::to_string(k)).c_str(), "wb");
        if (totals[k]) fwrite(t.text[k], 1, totals[k], o);
        fclose(o);
    }
    printf("overflow %d\n", (err & 2) ? 1 : 0);
    for (int k = 0; k < FQ_DEFL_SPANS; ++k) free(t.text[k]);
    free(lds), free(tok), free(slots), free(sizes), free(part);
    return rc;
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "--spans")) return spans_main(argc, argv);
    if (argc < 4) return 2;
    const std::vector<uint8_t> in = read_file(argv[1]);
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
