// ora.hip -- overrepresented-sequence counting of --ora on gfx950: the per-sequence counts and
// per-cycle distributions of the four Stats objects (Stats::statRead, reference
// src/stats.cpp:277-293), counted per pack by two passes around the pack's main kernels:
//   pre   the original reads (before UMI trim and -c), into pre-R1 / pre-R2;
//   post  the reads that reach the post-filter statRead, rebuilt from the pack's records and the
//         planes (which -c has corrected in place by then), into post-R1 / post-R2.
// Each Stats samples every `sampling`-th read of ITS OWN stream.  The handle keeps the four running
// statRead counts in device memory; the pre pass picks its reads arithmetically from them, the post
// pass from them plus an exclusive prefix count (hipCUB, both Stats packed in one 64-bit scan) of
// the reads that reach post-R1 / post-R2 before each pair.  The counts advance on the device in
// stream order, so nothing is read back to the host between packs.
//
// A workgroup is one wave and takes 64 consecutive pairs: every lane decides whether its reads are
// sampled, and the wave then scans the sampled ones one after another, all 64 lanes on one read
// (ora_core.h): the bytes staged in LDS, lanes on the window starts, hits as ballot masks,
// increments as 64-bit global atomics spread over the lanes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <string>

#include "../../include/fqengine.h"
#include "engine_internal.h"
#include "ora_core.h"

using namespace fqora;
using fqkstat::kstat_row;

struct fq_ora {
    int device = 0;
    int cus = 0;
    int sampling = 0;
    int eval[2] = {0, 0};
    ora_set set[2] = {};                  // device pointers
    void* set_mem[2][4] = {};             // bytes, off, len, slots of each set
    size_t words = 0;                     // of the four blocks
    size_t blk_off[4] = {0, 0, 0, 0};     // [pre-R1 | pre-R2 | post-R1 | post-R2]
    unsigned long long* blk = nullptr;
    unsigned long long* counts = nullptr; // the four Stats' statRead calls so far
    fq_read_result* res = nullptr;        // records of packs whose caller wants none
    size_t res_cap = 0;
    unsigned long long* reach = nullptr;  // per pair: reaches post-R1 | reaches post-R2 << 32
    unsigned long long* before = nullptr; // its exclusive prefix sum
    void* tmp = nullptr;
    size_t scan_cap = 0, tmp_bytes = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // pre start/end, post start/end
    bool timed_pre = false, timed_post = false;
    std::string err;
};

namespace {

// longest read a wave stages (a merged read of two 4096-byte rows): team_bytes(kMaxLen) is 41 KiB,
// inside the 64 KiB of LDS a kernel gets by default
constexpr int kMaxLen = 8192;

struct Wave {
    static constexpr int W = 64;
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ uint64_t ballot(bool p) const { return __ballot(p); }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// an accepted hit: the count from lane 0, the distribution's cycles over the lanes
struct Hit {
    unsigned long long* blk;
    int eval;
    __device__ __forceinline__ void operator()(int seq, int j, int step) {
        unsigned long long* cell = blk + (size_t)seq * (size_t)(1 + eval);
        if (threadIdx.x == 0) atomicAdd(cell, 1ull);
        const int end = j + step < eval ? j + step : eval;
        for (int p = j + (int)threadIdx.x; p < end; p += Wave::W) atomicAdd(cell + 1 + p, 1ull);
    }
};

struct PassArgs {
    ora_set set[2];
    unsigned long long* blk[2];
    const unsigned long long* counts;  // the pass's two
    int sampling, max_len;
};

__device__ __forceinline__ ora_post_items post_items(const fq_batch& b, int paired, int merge_enabled, int discard_unmerged,
                                                     const fq_read_result* res, long long idx, int l1, int l2) {
    ora_post_items it;
    if (paired) fqkstat::visit_post_pair(merge_enabled, discard_unmerged, res[2 * (size_t)idx], res[2 * (size_t)idx + 1], l1, l2, it);
    else fqkstat::visit_post_single(res[(size_t)idx], l1, it);
    return it;
}

// reach[i] = pair i reaches post-R1 | reaches post-R2 << 32
__global__ void ora_reach_kernel(fq_batch b, int paired, int merge_enabled, int discard_unmerged, const fq_read_result* res,
                                 unsigned long long* reach) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= b.n) return;
    const int l1 = b.len1[idx], l2 = paired ? b.len2[idx] : 0;
    unsigned long long v = 0;
    if (l1 <= b.stride && l2 <= b.stride) {
        const ora_post_items it = post_items(b, paired, merge_enabled, discard_unmerged, res, idx, l1, l2);
        v = (it.a.kind ? 1ull : 0ull) | (it.b.kind ? 1ull << 32 : 0ull);
    }
    reach[idx] = v;
}

// the statRead counts after the pack
__global__ void ora_advance_kernel(unsigned long long* counts, int n, int paired, const unsigned long long* reach,
                                   const unsigned long long* before) {
    if (threadIdx.x || blockIdx.x) return;
    if (!reach) {
        counts[0] += (unsigned long long)n;
        if (paired) counts[1] += (unsigned long long)n;
        return;
    }
    const unsigned long long t = before[n - 1] + reach[n - 1];
    counts[2] += t & 0xFFFFFFFFull;
    counts[3] += t >> 32;
}

// Both passes.  Round r of workgroup g takes pairs (r * gridDim + g) * 64 + lane.
template <bool POST>
__global__ __launch_bounds__(64) void ora_kernel(fq_batch b, int paired, int merge_enabled, int discard_unmerged,
                                                 const fq_read_result* res, const unsigned long long* before, PassArgs a,
                                                 int rounds) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sh[];
    const ora_team_mem mem(sh, a.max_len);
    const Wave wave;
    const unsigned long long c0 = a.counts[0], c1 = a.counts[1];
    const unsigned long long s = (unsigned long long)a.sampling;
    for (int r = 0; r < rounds; ++r) {
        const long long first = ((long long)r * gridDim.x + blockIdx.x) * Wave::W;
        if (first >= b.n) break;
        const long long idx = first + threadIdx.x;
        ora_item it[2] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
        bool take[2] = {false, false};
        if (idx < b.n) {
            const int l1 = b.len1[idx], l2 = paired ? b.len2[idx] : 0;
            // (a read longer than its row fails the pack in the main kernels; it is not read here)
            const bool ok = l1 <= b.stride && l2 <= b.stride;
            if (!POST) {
                if (ok) it[0] = ora_item{1, 0, l1, 0, 0};
                if (ok && paired) it[1] = ora_item{2, 0, l2, 0, 0};
                take[0] = (c0 + (unsigned long long)idx) % s == 0;
                take[1] = paired && (c1 + (unsigned long long)idx) % s == 0;
            } else if (ok) {
                const ora_post_items pi = post_items(b, paired, merge_enabled, discard_unmerged, res, idx, l1, l2);
                const unsigned long long bf = before[idx];
                it[0] = pi.a, it[1] = pi.b;
                take[0] = (c0 + (bf & 0xFFFFFFFFull)) % s == 0;
                take[1] = (c1 + (bf >> 32)) % s == 0;
            }
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            if (a.set[st].ntab == 0) continue;  // an empty set, or no step of its lengths: nothing can hit
            const ora_item mine = it[st];
            uint64_t todo = __ballot(take[st] && mine.kind != 0);
            Hit hit{a.blk[st], a.set[st].eval_len};
            while (todo) {  // (at most 64 turns)
                const int L = (int)__builtin_ctzll(todo);
                todo &= todo - 1;
                const int kind = __shfl(mine.kind, L), st1 = __shfl(mine.st1, L), n1 = __shfl(mine.n1, L);
                const int st2 = __shfl(mine.st2, L), n2 = __shfl(mine.n2, L);
                const int len = kind == 3 ? n1 + n2 : n1;
                if (len > a.max_len) continue;
                if (kind == 2) {
                    stage_row(wave, mem.s, kstat_row(b.seq2, b.stride, first + L), st1, n1);
                } else {
                    stage_row(wave, mem.s, kstat_row(b.seq1, b.stride, first + L), st1, n1);
                    if (kind == 3) stage_revcomp(wave, mem.s + n1, kstat_row(b.seq2, b.stride, first + L), st2, n2);
                }
                __syncthreads();
                scan_read(wave, mem, len, a.set[st], hit);
                __syncthreads();
            }
        }
    }
}

int ora_fail(fq_ora* h, hipError_t e, const char* what) {
    h->err = std::string(what) + ": " + hipGetErrorString(e);
    return FQ_E_HIP;
}

#define ORA_TRY(h, call)                                      \
    do {                                                      \
        hipError_t _e = (call);                               \
        if (_e != hipSuccess) return ora_fail(h, _e, #call);  \
    } while (0)

int ensure_scan(fq_ora* h, size_t n, hipStream_t s) {
    if (n <= h->scan_cap) return FQ_OK;
    ORA_TRY(h, hipStreamSynchronize(s));  // (a pass in flight may still read the old buffers)
    for (void* p : {(void*)h->reach, (void*)h->before, h->tmp})
        if (p) (void)hipFree(p);
    h->reach = h->before = nullptr;
    h->tmp = nullptr;
    h->scan_cap = 0;
    const size_t cap = n < 4096 ? 4096 : n;
    size_t tb = 0;
    ORA_TRY(h, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                (int)cap));
    ORA_TRY(h, hipMalloc(&h->reach, cap * sizeof(unsigned long long)));
    ORA_TRY(h, hipMalloc(&h->before, cap * sizeof(unsigned long long)));
    ORA_TRY(h, hipMalloc(&h->tmp, tb ? tb : 8));
    h->tmp_bytes = tb;
    h->scan_cap = cap;
    return FQ_OK;
}

template <bool POST>
int launch_pass(fq_ora* h, const fq_batch& b, const fq_params& p, const fq_read_result* res, hipStream_t s) {
    PassArgs a;
    const int max_len = (POST && p.paired && p.merge_enabled) ? 2 * b.stride : b.stride;
    if (max_len > kMaxLen) return h->err = "row stride too large for the overrepresented-sequence passes", FQ_E_INVALID;
    for (int st = 0; st < 2; ++st) {
        a.set[st] = h->set[st];
        a.blk[st] = h->blk + h->blk_off[(POST ? 2 : 0) + st];
    }
    a.counts = h->counts + (POST ? 2 : 0);
    a.sampling = h->sampling;
    a.max_len = max_len;
    if (POST) {
        const int rc = ensure_scan(h, (size_t)b.n, s);
        if (rc != FQ_OK) return rc;
        hipLaunchKernelGGL(ora_reach_kernel, dim3((unsigned)((b.n + 255) / 256)), dim3(256), 0, s, b, p.paired,
                           p.merge_enabled, p.discard_unmerged, res, h->reach);
        ORA_TRY(h, hipGetLastError());
        size_t tb = h->tmp_bytes;
        ORA_TRY(h, hipcub::DeviceScan::ExclusiveSum(h->tmp, tb, h->reach, h->before, b.n, s));
    }
    const int cus = h->cus;
    const long long need = ((long long)b.n + Wave::W - 1) / Wave::W;
    long long grid = need < (long long)cus * 16 ? need : (long long)cus * 16;
    if (grid < 1) grid = 1;
    const int rounds = (int)((need + grid - 1) / grid);
    hipLaunchKernelGGL((ora_kernel<POST>), dim3((unsigned)grid), dim3(Wave::W), team_bytes(max_len), s, b, p.paired,
                       p.merge_enabled, p.discard_unmerged, res, POST ? h->before : nullptr, a, rounds);
    ORA_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(ora_advance_kernel, dim3(1), dim3(1), 0, s, h->counts, b.n, p.paired, POST ? h->reach : nullptr,
                       POST ? h->before : nullptr);
    ORA_TRY(h, hipGetLastError());
    return FQ_OK;
}

// a host array on the device
template <class T>
hipError_t upload(const std::vector<T>& v, void** out) {
    *out = nullptr;
    hipError_t e = hipMalloc(out, v.empty() ? 8 : v.size() * sizeof(T));
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

}  // namespace

int fq_ora_pre(fq_ora* h, const fq_batch& b, const fq_params& p, hipStream_t s) {
    if (b.n <= 0) return FQ_OK;
    ORA_TRY(h, hipEventRecord(h->ev[0], s));
    const int rc = launch_pass<false>(h, b, p, nullptr, s);
    if (rc != FQ_OK) return rc;
    ORA_TRY(h, hipEventRecord(h->ev[1], s));
    h->timed_pre = true;
    h->timed_post = false;
    return FQ_OK;
}

int fq_ora_post(fq_ora* h, const fq_batch& b, const fq_params& p, const fq_read_result* res, hipStream_t s) {
    if (b.n <= 0) return FQ_OK;
    if (!res) return h->err = "the post-filter overrepresented-sequence pass needs the pack's records", FQ_E_INVALID;
    ORA_TRY(h, hipEventRecord(h->ev[2], s));
    const int rc = launch_pass<true>(h, b, p, res, s);
    if (rc != FQ_OK) return rc;
    ORA_TRY(h, hipEventRecord(h->ev[3], s));
    h->timed_post = true;
    return FQ_OK;
}

int fq_ora_records(fq_ora* h, size_t n, hipStream_t s, fq_read_result** out) {
    if (n > h->res_cap) {
        ORA_TRY(h, hipStreamSynchronize(s));  // (a pass in flight may still read the old buffer)
        if (h->res) (void)hipFree(h->res);
        h->res = nullptr;
        h->res_cap = 0;
        const size_t cap = n < 4096 ? 4096 : n;
        ORA_TRY(h, hipMalloc(&h->res, cap * sizeof(fq_read_result)));
        h->res_cap = cap;
    }
    *out = h->res;
    return FQ_OK;
}

const char* fq_ora_error(const fq_ora* h) { return h ? h->err.c_str() : ""; }

int fq_ora_device(const fq_ora* h, int* device) {
    if (!h || !device) return FQ_E_INVALID;
    *device = h->device;
    return FQ_OK;
}

extern "C" {

int fq_ora_create(int device, int32_t sampling, int32_t eval_len1, int32_t eval_len2, const uint8_t* seq1,
                  const uint32_t* off1, int32_t n1, const uint8_t* seq2, const uint32_t* off2, int32_t n2, fq_ora** out) {
    if (!out || sampling < 1 || eval_len1 < 3 || eval_len2 < 3 || n1 < 0 || n2 < 0) return FQ_E_INVALID;
    if ((n1 > 0 && (!seq1 || !off1)) || (n2 > 0 && (!seq2 || !off2))) return FQ_E_INVALID;
    *out = nullptr;
    ora_image im[2];
    const uint32_t none[1] = {0};
    if (!ora_build(seq1, n1 ? off1 : none, n1, eval_len1, im[0]) || !ora_build(seq2, n2 ? off2 : none, n2, eval_len2, im[1]))
        return FQ_E_INVALID;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return FQ_E_NO_DEVICE;
    fq_ora* h = new fq_ora();
    h->device = device;
    h->sampling = sampling;
    h->eval[0] = eval_len1, h->eval[1] = eval_len2;
    auto bail = [&](int rc) {
        fq_ora_destroy(h);
        return rc;
    };
    if (hipSetDevice(device) != hipSuccess) return bail(FQ_E_HIP);
    if (hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->cus < 1)
        return bail(FQ_E_HIP);
    for (int st = 0; st < 2; ++st) {
        if (upload(im[st].bytes, &h->set_mem[st][0]) != hipSuccess || upload(im[st].off, &h->set_mem[st][1]) != hipSuccess ||
            upload(im[st].len, &h->set_mem[st][2]) != hipSuccess || upload(im[st].slots, &h->set_mem[st][3]) != hipSuccess)
            return bail(FQ_E_NOMEM);
        h->set[st] = im[st].set;
        h->set[st].bytes = (const uint8_t*)h->set_mem[st][0];
        h->set[st].off = (const uint32_t*)h->set_mem[st][1];
        h->set[st].len = (const uint16_t*)h->set_mem[st][2];
        h->set[st].slots = (const ora_slot*)h->set_mem[st][3];
    }
    const size_t w1 = (size_t)n1 * (size_t)(1 + eval_len1), w2 = (size_t)n2 * (size_t)(1 + eval_len2);
    h->blk_off[0] = 0, h->blk_off[1] = w1, h->blk_off[2] = w1 + w2, h->blk_off[3] = 2 * w1 + w2;
    h->words = 2 * (w1 + w2);
    if (hipMalloc(&h->blk, (h->words ? h->words : 1) * sizeof(unsigned long long)) != hipSuccess) return bail(FQ_E_NOMEM);
    if (hipMalloc(&h->counts, 4 * sizeof(unsigned long long)) != hipSuccess) return bail(FQ_E_NOMEM);
    for (hipEvent_t& e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) return bail(FQ_E_HIP);
    if (fq_ora_reset(h) != FQ_OK) return bail(FQ_E_HIP);
    *out = h;
    return FQ_OK;
}

int fq_ora_destroy(fq_ora* h) {
    if (!h) return FQ_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (auto& m : h->set_mem)
        for (void* p : m)
            if (p) (void)hipFree(p);
    for (void* p : {(void*)h->blk, (void*)h->counts, (void*)h->res, (void*)h->reach, (void*)h->before, h->tmp})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
    return FQ_OK;
}

int fq_ora_reset(fq_ora* h) {
    if (!h) return FQ_E_INVALID;
    ORA_TRY(h, hipSetDevice(h->device));
    ORA_TRY(h, hipDeviceSynchronize());
    ORA_TRY(h, hipMemset(h->blk, 0, (h->words ? h->words : 1) * sizeof(unsigned long long)));
    ORA_TRY(h, hipMemset(h->counts, 0, 4 * sizeof(unsigned long long)));
    ORA_TRY(h, hipDeviceSynchronize());
    return FQ_OK;
}

size_t fq_ora_words(const fq_ora* h) { return h ? h->words : 0; }

int fq_ora_read(fq_ora* h, uint64_t* host, size_t words) {
    if (!h || (!host && h->words) || words < h->words) return FQ_E_INVALID;
    ORA_TRY(h, hipSetDevice(h->device));
    ORA_TRY(h, hipDeviceSynchronize());
    if (h->words) ORA_TRY(h, hipMemcpy(host, h->blk, h->words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return FQ_OK;
}

double fq_ora_last_kernel_ms(const fq_ora* h) {
    if (!h || !h->timed_pre) return 0.0;
    float a = 0.f, b = 0.f;
    if (hipEventSynchronize(h->ev[1]) != hipSuccess || hipEventElapsedTime(&a, h->ev[0], h->ev[1]) != hipSuccess) return 0.0;
    if (h->timed_post &&
        (hipEventSynchronize(h->ev[3]) != hipSuccess || hipEventElapsedTime(&b, h->ev[2], h->ev[3]) != hipSuccess))
        return 0.0;
    return (double)a + (double)b;
}

}  // extern "C"
