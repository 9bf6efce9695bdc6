// kstat.hip -- k-mer counting of --kmer on gfx950: the KmerCount tables of the four Stats objects
// (Stats::statRead, reference src/stats.cpp:245,266-274), counted per pack by two passes around
// the pack's main kernels:
//   pre   the original reads (before UMI trim and -c), into pre-R1 / pre-R2;
//   post  the reads that reach the post-filter statRead, rebuilt from the pack's records and the
//         planes (which -c has corrected in place by then), into post-R1 / post-R2.
// One lane walks one read (pair) with 16-byte chunk loads of the tiled planes (a wave's load of
// one chunk is contiguous runs of 512 bytes); the per-read routine is kstat_core.h.
//
// Where the increments go:
//   k <= kLdsMaxK  a private copy of the pass's two tables per workgroup in LDS, 32-bit cells
//                  (2 * 4^k * 4 bytes: 2 KiB at k = 4 ... 128 KiB at k = 7 of the CU's 160 KiB),
//                  flushed to the uint64 tables with one atomic per non-zero cell;
//   k >  kLdsMaxK  (k = 8 would need 512 KiB) 64-bit atomics on the global tables, results unused.
// A lane adds a run of equal keys (homopolymers) with one atomic.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/fqengine.h"
#include "engine_internal.h"
#include "kstat_core.h"

using namespace fqkstat;

struct fq_kstat {
    int device = 0;
    int k = 0;
    size_t tw = 0;                       // 4^k: words per table
    unsigned long long* tab = nullptr;   // [pre-R1 | pre-R2 | post-R1 | post-R2]
    fq_read_result* res = nullptr;       // records of packs whose caller wants none
    size_t res_cap = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // pre start/end, post start/end
    bool timed_pre = false, timed_post = false;
    std::string err;
};

namespace {

constexpr int kLdsMaxK = 7;

// one increment target of a lane: equal consecutive keys are added together
template <bool LDS>
struct Bin {
    uint32_t* sh;               // LDS copy of the table (LDS)
    unsigned long long* glob;   // the table (!LDS)
    uint32_t key, n;
    __device__ __forceinline__ void operator()(uint32_t k2) {
        if (n && k2 == key) {
            ++n;
            return;
        }
        flush();
        key = k2;
        n = 1;
    }
    __device__ __forceinline__ void flush() {
        if (!n) return;
        if (LDS) atomicAdd(&sh[key], n);
        else atomicAdd(&glob[key], (unsigned long long)n);
        n = 0;
    }
};

template <bool LDS>
__device__ __forceinline__ void flush_lds(uint32_t* sh, unsigned long long* t, size_t cells) {
    if (!LDS) return;
    __syncthreads();
    for (size_t i = threadIdx.x; i < cells; i += blockDim.x) {
        const uint32_t v = sh[i];
        if (v) {
            atomicAdd(&t[i], (unsigned long long)v);
            sh[i] = 0;
        }
    }
    __syncthreads();
}

// Both passes: POST = false counts the original reads into t[0, tw) (R1) and t[tw, 2 tw) (R2);
// POST = true counts what the records say reached the post-filter statRead.
// A workgroup takes reads round by round (round r: reads (r * gridDim + blockIdx) * blockDim + lane)
// and flushes its LDS cells every `flush_rounds` rounds.  Bound: a read adds fewer than `stride`
// increments to a table, a merged read fewer than 2 * stride, so one round adds fewer than
// blockDim * 2 * stride to any cell, and the host sets flush_rounds = (2^32 - 1) / (blockDim * 2 *
// stride) (>= 1 for every stride the 16-bit lengths allow): no 32-bit cell can wrap, however many
// bases the pack holds.
template <bool LDS, bool POST>
__global__ void kstat_kernel(fq_batch b, int paired, int merge_enabled, int discard_unmerged, const fq_read_result* res,
                             int k, unsigned long long* t, size_t tw, int rounds, int flush_rounds) {
    extern __shared__ uint32_t sh[];
    if (LDS) {
        for (size_t i = threadIdx.x; i < 2 * tw; i += blockDim.x) sh[i] = 0;
        __syncthreads();
    }
    Bin<LDS> b1{sh, t, 0, 0}, b2{sh + (LDS ? tw : 0), t + tw, 0, 0};
    for (int r = 0; r < rounds; ++r) {
        const long long idx = ((long long)r * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
        if (idx < b.n) {
            const int l1 = b.len1[idx];
            const int l2 = paired ? b.len2[idx] : 0;
            // (a read longer than its row fails the pack in the main kernels; it is not read here)
            if (l1 <= b.stride && l2 <= b.stride) {
                kstat_row s1(b.seq1, b.stride, idx);
                if (!POST) {
                    count_row(s1, 0, l1, k, b1);
                    if (paired) {
                        kstat_row s2(b.seq2, b.stride, idx);
                        count_row(s2, 0, l2, k, b2);
                    }
                } else if (paired) {
                    kstat_row s2(b.seq2, b.stride, idx);
                    const fq_read_result r1 = res[2 * (size_t)idx], r2 = res[2 * (size_t)idx + 1];
                    post_pair(merge_enabled, discard_unmerged, r1, r2, s1, l1, s2, l2, k, b1, b2);
                } else {
                    const fq_read_result r1 = res[(size_t)idx];
                    post_single(r1, s1, l1, k, b1);
                }
                b1.flush();
                b2.flush();
            }
        }
        if (LDS && (r + 1) % flush_rounds == 0 && r + 1 < rounds) flush_lds<LDS>(sh, t, 2 * tw);
    }
    flush_lds<LDS>(sh, t, 2 * tw);
}

int kstat_fail(fq_kstat* h, hipError_t e, const char* what) {
    h->err = std::string(what) + ": " + hipGetErrorString(e);
    return FQ_E_HIP;
}

#define KSTAT_TRY(h, call)                                      \
    do {                                                        \
        hipError_t _e = (call);                                 \
        if (_e != hipSuccess) return kstat_fail(h, _e, #call);  \
    } while (0)

template <bool POST>
int launch_pass(fq_kstat* h, const fq_batch& b, const fq_params& p, const fq_read_result* res, hipStream_t s) {
    const bool lds = h->k <= kLdsMaxK;
    // as many waves per CU as the LDS copies allow, up to the CU's 32: k = 7 one workgroup of 16
    // waves (128 KiB), k = 6 four of 8 waves (4 x 32 KiB), smaller tables eight of 4 waves
    const int threads = h->k == kLdsMaxK ? 1024 : h->k == kLdsMaxK - 1 ? 512 : 256;
    const size_t shmem = lds ? 2 * h->tw * sizeof(uint32_t) : 0;
    const long long need = ((long long)b.n + threads - 1) / threads;
    long long grid = need;
    if (lds) {
        int cus = 0;
        KSTAT_TRY(h, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
        const long long per_cu = h->k == kLdsMaxK ? 1 : h->k == kLdsMaxK - 1 ? 4 : 8;
        grid = need < cus * per_cu ? need : cus * per_cu;
    }
    if (grid < 1) grid = 1;
    const int rounds = (int)((need + grid - 1) / grid);
    const unsigned long long per_round = (unsigned long long)threads * 2ull * (unsigned long long)b.stride;
    unsigned long long fr = 0xFFFFFFFFull / per_round;
    if (fr < 1) return h->err = "row stride too large for the k-mer tables", FQ_E_INVALID;
    const int flush_rounds = fr > 0x7FFFFFFFull ? 0x7FFFFFFF : (int)fr;
    unsigned long long* t = h->tab + (POST ? 2 * h->tw : 0);
    if (lds)
        hipLaunchKernelGGL((kstat_kernel<true, POST>), dim3((unsigned)grid), dim3(threads), shmem, s, b, p.paired,
                           p.merge_enabled, p.discard_unmerged, res, h->k, t, h->tw, rounds, flush_rounds);
    else
        hipLaunchKernelGGL((kstat_kernel<false, POST>), dim3((unsigned)grid), dim3(threads), 0, s, b, p.paired,
                           p.merge_enabled, p.discard_unmerged, res, h->k, t, h->tw, rounds, flush_rounds);
    KSTAT_TRY(h, hipGetLastError());
    return FQ_OK;
}

}  // namespace

int fq_kstat_pre(fq_kstat* h, const fq_batch& b, const fq_params& p, hipStream_t s) {
    if (b.n <= 0) return FQ_OK;
    KSTAT_TRY(h, hipEventRecord(h->ev[0], s));
    const int rc = launch_pass<false>(h, b, p, nullptr, s);
    if (rc != FQ_OK) return rc;
    KSTAT_TRY(h, hipEventRecord(h->ev[1], s));
    h->timed_pre = true;
    h->timed_post = false;
    return FQ_OK;
}

int fq_kstat_post(fq_kstat* h, const fq_batch& b, const fq_params& p, const fq_read_result* res, hipStream_t s) {
    if (b.n <= 0) return FQ_OK;
    if (!res) return h->err = "the post-filter k-mer pass needs the pack's records", FQ_E_INVALID;
    KSTAT_TRY(h, hipEventRecord(h->ev[2], s));
    const int rc = launch_pass<true>(h, b, p, res, s);
    if (rc != FQ_OK) return rc;
    KSTAT_TRY(h, hipEventRecord(h->ev[3], s));
    h->timed_post = true;
    return FQ_OK;
}

int fq_kstat_records(fq_kstat* h, size_t n, hipStream_t s, fq_read_result** out) {
    if (n > h->res_cap) {
        KSTAT_TRY(h, hipStreamSynchronize(s));  // (a pass in flight may still read the old buffer)
        if (h->res) (void)hipFree(h->res);
        h->res = nullptr;
        h->res_cap = 0;
        const size_t cap = n < 4096 ? 4096 : n;
        KSTAT_TRY(h, hipMalloc(&h->res, cap * sizeof(fq_read_result)));
        h->res_cap = cap;
    }
    *out = h->res;
    return FQ_OK;
}

const char* fq_kstat_error(const fq_kstat* h) { return h ? h->err.c_str() : ""; }

int fq_kstat_device(const fq_kstat* h, int* device) {
    if (!h || !device) return FQ_E_INVALID;
    *device = h->device;
    return FQ_OK;
}

extern "C" {

int fq_kstat_create(int device, int32_t k, fq_kstat** out) {
    if (!out || k < FQ_KSTAT_MIN_K || k > FQ_KSTAT_MAX_K) return FQ_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return FQ_E_NO_DEVICE;
    fq_kstat* h = new fq_kstat();
    h->device = device;
    h->k = k;
    h->tw = (size_t)1 << (2 * k);
    auto bail = [&](int rc) {
        fq_kstat_destroy(h);
        return rc;
    };
    if (hipSetDevice(device) != hipSuccess) return bail(FQ_E_HIP);
    if (hipMalloc(&h->tab, 4 * h->tw * sizeof(unsigned long long)) != hipSuccess) return bail(FQ_E_NOMEM);
    for (hipEvent_t& e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) return bail(FQ_E_HIP);
    if (k == kLdsMaxK) {  // above the 64 KiB a kernel gets by default
        const int bytes = (int)(2 * h->tw * sizeof(uint32_t));
        if (hipFuncSetAttribute((const void*)kstat_kernel<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) !=
                hipSuccess ||
            hipFuncSetAttribute((const void*)kstat_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) !=
                hipSuccess)
            return bail(FQ_E_HIP);
    }
    if (fq_kstat_reset(h) != FQ_OK) return bail(FQ_E_HIP);
    *out = h;
    return FQ_OK;
}

int fq_kstat_destroy(fq_kstat* h) {
    if (!h) return FQ_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->tab) (void)hipFree(h->tab);
    if (h->res) (void)hipFree(h->res);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
    return FQ_OK;
}

int fq_kstat_reset(fq_kstat* h) {
    if (!h) return FQ_E_INVALID;
    KSTAT_TRY(h, hipSetDevice(h->device));
    KSTAT_TRY(h, hipDeviceSynchronize());
    KSTAT_TRY(h, hipMemset(h->tab, 0, 4 * h->tw * sizeof(unsigned long long)));
    KSTAT_TRY(h, hipDeviceSynchronize());
    return FQ_OK;
}

int fq_kstat_k(const fq_kstat* h) { return h ? h->k : 0; }

size_t fq_kstat_words(const fq_kstat* h) { return h ? 4 * h->tw : 0; }

int fq_kstat_read(fq_kstat* h, uint64_t* host, size_t words) {
    if (!h || !host || words < 4 * h->tw) return FQ_E_INVALID;
    KSTAT_TRY(h, hipSetDevice(h->device));
    KSTAT_TRY(h, hipDeviceSynchronize());
    KSTAT_TRY(h, hipMemcpy(host, h->tab, 4 * h->tw * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return FQ_OK;
}

double fq_kstat_last_kernel_ms(const fq_kstat* h) {
    if (!h || !h->timed_pre) return 0.0;
    float a = 0.f, b = 0.f;
    if (hipEventSynchronize(h->ev[1]) != hipSuccess || hipEventElapsedTime(&a, h->ev[0], h->ev[1]) != hipSuccess) return 0.0;
    if (h->timed_post &&
        (hipEventSynchronize(h->ev[3]) != hipSuccess || hipEventElapsedTime(&b, h->ev[2], h->ev[3]) != hipSuccess))
        return 0.0;
    return (double)a + (double)b;
}

}  // extern "C"
