// deflate_spans_bench.hip -- per-pack cost of the routed egress's compression (deflate.hip), timed
// with HIP events: one multi-span launch (fq_launch_deflate_spans) against one fq_launch_deflate per
// open stream, on the same texts, capacities and scratch.  The capacities are the engine's
// (fq_egress_bound of a pack of PAIRS pairs whose mates span TEXT bytes), the streams' real sizes
// are given as shares of one mate's text, as in a failed + unpaired1/2 run.
//   hipcc -std=c++17 -O3 --offload-arch=gfx950 tools/micro/deflate_spans_bench.hip -Lfqtool_amd/lib -lfqengine
//         -Wl,-rpath,'$ORIGIN/../../fqtool_amd/lib' -o tools/micro/deflate_spans_bench
//   tools/micro/deflate_spans_bench [PAIRS=262144] [LEVEL=4] [REPEAT=5] [SHARES=0.85,0.85,0,0.03,0.03,0.24]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fqtool_amd/csrc/engine_internal.h"

#define CHECK(x)                                                                              \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); \
            return 1;                                                                         \
        }                                                                                     \
    } while (0)

// FASTQ records of 150 bases: a counted name, uniform bases, qualities from a skewed set
static std::vector<char> fastq_text(size_t bytes, uint64_t seed) {
    std::vector<char> t;
    t.reserve(bytes + 400);
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&] {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return x;
    };
    const char q[16] = {'F', 'F', 'F', 'F', 'F', 'F', 'F', 'F', 'F', 'F', ':', ':', ':', ',', ',', '#'};
    for (size_t i = 0; t.size() < bytes; ++i) {
        char name[64];
        const int n = std::snprintf(name, sizeof name, "@SIM:1:FCX:1:%zu:%zu:%zu 1:N:0:ATCACG\n", i / 100000, i % 100000, i * 7 % 9973);
        t.insert(t.end(), name, name + n);
        for (int k = 0; k < 150; ++k) t.push_back("ACGT"[rnd() & 3]);
        t.push_back('\n'), t.push_back('+'), t.push_back('\n');
        for (int k = 0; k < 150; ++k) t.push_back(q[rnd() & 15]);
        t.push_back('\n');
    }
    t.resize(bytes);
    return t;
}

int main(int argc, char** argv) {
    const size_t pairs = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 262144;
    const int level = argc > 2 ? std::atoi(argv[2]) : 4;
    const int repeat = argc > 3 ? std::atoi(argv[3]) : 5;
    double share[FQ_EG_STREAMS] = {0.85, 0.85, 0, 0.03, 0.03, 0.24};
    if (argc > 4) {
        const char* p = argv[4];
        for (int k = 0; k < FQ_EG_STREAMS && *p; ++k) {
            char* end;
            share[k] = std::strtod(p, &end);
            p = *end ? end + 1 : end;
        }
    }
    const size_t text = pairs * 340;  // one mate's input text
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    hipStream_t s;
    CHECK(hipStreamCreate(&s));
    size_t cap[FQ_EG_STREAMS], n[FQ_EG_STREAMS], sum_cap = 0, open = 0;
    char* d_text[FQ_EG_STREAMS] = {};
    std::vector<std::vector<char>> host(FQ_EG_STREAMS);
    unsigned long long *d_n, *d_len;
    CHECK(hipMalloc(&d_n, FQ_EG_STREAMS * sizeof(unsigned long long)));
    CHECK(hipMalloc(&d_len, FQ_EG_STREAMS * sizeof(unsigned long long)));
    unsigned long long h_n[FQ_EG_STREAMS];
    for (int k = 0; k < FQ_EG_STREAMS; ++k) {
        cap[k] = share[k] > 0 ? fq_egress_bound(k, text, text, pairs) : 0;
        n[k] = (size_t)(share[k] * (double)text);
        if (n[k] > cap[k]) n[k] = cap[k];
        h_n[k] = n[k];
        if (!cap[k]) continue;
        ++open;
        sum_cap += cap[k];
        host[k] = fastq_text(n[k], 11 + (uint64_t)k);
        CHECK(hipMalloc(&d_text[k], fq_deflate_bound(cap[k])));
    }
    CHECK(hipMemcpy(d_len, h_n, sizeof h_n, hipMemcpyHostToDevice));
    // the scratch the engine makes for such a pack: the FAILED bound plus a member per open stream
    fq_deflate_scratch sc;
    const size_t largest = fq_egress_bound(FQ_EG_FAILED, text, text, pairs);
    CHECK(fq_deflate_scratch_ensure(sc, largest + open * FQ_BGZF_IN, prop.multiProcessorCount));
    std::printf("pairs %zu, level %d, %zu open streams, text per mate %zu B; sizes", pairs, level, open, text);
    for (int k = 0; k < FQ_EG_STREAMS; ++k) std::printf(" %zu", n[k]);
    std::printf("; sum of the capacities %zu B, scratch %zu members on %d CUs\n", sum_cap, sc.members, sc.cus);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    unsigned long long out_spans[FQ_EG_STREAMS] = {}, out_single[FQ_EG_STREAMS] = {};
    for (int mode = 0; mode < 2; ++mode) {
        for (int r = 0; r < repeat; ++r) {
            for (int k = 0; k < FQ_EG_STREAMS; ++k)
                if (cap[k] && n[k]) CHECK(hipMemcpyAsync(d_text[k], host[k].data(), n[k], hipMemcpyHostToDevice, s));
            CHECK(hipMemcpyAsync(d_n, d_len, sizeof h_n, hipMemcpyDeviceToDevice, s));
            CHECK(hipEventRecord(e0, s));
            if (mode == 0) {
                fq_deflate_span sp[FQ_EG_STREAMS] = {};
                for (int k = 0; k < FQ_EG_STREAMS; ++k)
                    if (cap[k]) sp[k] = fq_deflate_span{d_text[k], d_n + k, cap[k]};
                CHECK(fq_launch_deflate_spans(sc, sp, level, d_n, nullptr, s));
            } else {
                for (int k = 0; k < FQ_EG_STREAMS; ++k)
                    if (cap[k])
                        CHECK(fq_launch_deflate(sc, d_text[k], d_n + k, cap[k], level, d_text[k], fq_deflate_bound(cap[k]), d_n + k, s));
            }
            CHECK(hipEventRecord(e1, s));
            CHECK(hipStreamSynchronize(s));
            float ms = 0;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            CHECK(hipMemcpy(mode ? out_single : out_spans, d_n, sizeof h_n, hipMemcpyDeviceToHost));
            unsigned long long in = 0, out = 0;
            for (int k = 0; k < FQ_EG_STREAMS; ++k) in += n[k], out += (mode ? out_single : out_spans)[k];
            std::printf("%s run %d: %.3f ms, %llu -> %llu B (%.1f GB/s of text)\n", mode ? "one launch per stream" : "multi-span launch ",
                        r, ms, in, out, (double)in / ms * 1e-6);
        }
    }
    // (the hash inserts of a sub-block race, so the two forms' streams differ by a few bytes; an empty
    // stream must be empty in both)
    bool same = true;
    for (int k = 0; k < FQ_EG_STREAMS; ++k) {
        const unsigned long long a = out_spans[k], b = out_single[k], d = a > b ? a - b : b - a;
        same = same && (a == 0) == (b == 0) && d <= a / 1000;
    }
    std::printf("stream sizes of both forms %s\n", same ? "agree within 0.1 %" : "DIFFER");
    fq_deflate_scratch_free(sc);
    return same ? 0 : 1;
}
