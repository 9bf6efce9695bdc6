// ingest.hip -- the device ingest kernels of text packs and raw windows (include/fqengine.h "device
// ingest" and "pack cuts"; the per-record routines are ingest_core.h's):
//   * index_flags_kernel: the index filter's per-record FQ_BF_* flags from the records' names, one
//     lane per record; the lists (offsets, then bytes) are staged in LDS when they fit in 32 KiB
//     and read from device memory otherwise;
//   * phred64_kernel: the quality lines of the pack's records rewritten in the device copy of the
//     text, one thread per (record, 16-byte chunk);
//   * cuts_kernel: the cut table of a pack's plain pair egress, one wave per piece, from the egress's
//     per-record sizes and their exclusive scan.
// As in text.hip, PCIe bounds the path these run on, not the kernels.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "ingest_core.h"

namespace {

constexpr uint32_t kListLdsBytes = 32 * 1024;

// the lists in the blob (fq_index_lists): off1[n1 + 1] | off2[n2 + 1] | bytes1 | bytes2
__device__ __forceinline__ void lists_of(const uint32_t* blob, uint32_t n1, uint32_t n2, uint32_t len1, fqingest::List& l1,
                                         fqingest::List& l2) {
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(blob + n1 + n2 + 2);
    l1 = fqingest::List{bytes, blob, (int)n1};
    l2 = fqingest::List{bytes + len1, blob + n1 + 1, (int)n2};
}

template <bool LDS>
__global__ __launch_bounds__(256) void index_flags_kernel(fq_index_lists f, const char* __restrict__ text1,
                                                          const fq_text_rec* __restrict__ rec1, const char* __restrict__ text2,
                                                          const fq_text_rec* __restrict__ rec2, int n, uint8_t* __restrict__ flags) {
    __shared__ uint32_t staged[LDS ? kListLdsBytes / 4 : 1];
    const uint32_t* blob = f.blob;
    if (LDS) {
        const uint32_t words = (f.blob_bytes + 3) / 4;  // (the blob is allocated in whole words)
        for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) staged[w] = f.blob[w];
        __syncthreads();
        blob = staged;
    }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fqingest::List l1, l2;
    lists_of(blob, f.n1, f.n2, f.len1, l1, l2);
    const fq_text_rec r1 = rec1[i];
    fq_text_rec r2{};
    if (text2) r2 = rec2[i];
    flags[i] = fqingest::index_flag(l1, l2, f.threshold, text1, r1, text2, &r2);
}

__global__ __launch_bounds__(256) void phred64_kernel(char* __restrict__ text, const fq_text_rec* __restrict__ rec, int n,
                                                      int nch) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = t / nch;
    if (r >= n) return;
    const int j0 = 16 * (int)(t - r * nch);
    const fq_text_rec R = rec[r];
    const int m = min(16, (int)R.len - j0);
    uint8_t* q = reinterpret_cast<uint8_t*>(text) + R.qual_off + j0;
    for (int b = 0; b < m; ++b) q[b] = fqingest::phred64_to_33(q[b]);
}

__global__ __launch_bounds__(64) void cuts_kernel(const uint32_t* __restrict__ size0, const uint32_t* __restrict__ off0,
                                                  const uint32_t* __restrict__ size1, const uint32_t* __restrict__ off1,
                                                  uint32_t n, unsigned long long every, unsigned long long first,
                                                  uint32_t pieces, fq_cut* __restrict__ out) {
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    if (j >= pieces) return;
    uint32_t lo, hi;
    fqingest::cut_range(every, first, n, j, lo, hi);
    uint32_t passed = 0;
    for (uint32_t base = lo; base < hi; base += 64) {  // (a wave-uniform trip count: every lane votes)
        const uint32_t i = base + lane;
        passed += (uint32_t)__popcll(__ballot(i < hi && size0[i] != 0));
    }
    if (lane) return;
    fq_cut c{};
    c.bytes[0] = fqingest::cut_offset(size0, off0, n, hi) - fqingest::cut_offset(size0, off0, n, lo);
    if (size1) c.bytes[1] = fqingest::cut_offset(size1, off1, n, hi) - fqingest::cut_offset(size1, off1, n, lo);
    c.items = hi - lo;
    c.passed = passed;
    out[j] = c;
}

}  // namespace

hipError_t fq_launch_index_flags(const fq_index_lists& f, const char* d_text1, const fq_text_rec* d_rec1, const char* d_text2,
                                 const fq_text_rec* d_rec2, int n, uint8_t* d_flags, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const dim3 g((n + 255) / 256), b(256);
    if (f.blob_bytes <= kListLdsBytes)
        hipLaunchKernelGGL(index_flags_kernel<true>, g, b, 0, s, f, d_text1, d_rec1, d_text2, d_rec2, n, d_flags);
    else
        hipLaunchKernelGGL(index_flags_kernel<false>, g, b, 0, s, f, d_text1, d_rec1, d_text2, d_rec2, n, d_flags);
    return hipGetLastError();
}

hipError_t fq_launch_phred64(char* d_text, const fq_text_rec* d_rec, int n, int stride, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int nch = stride >> 4;
    const long long threads = (long long)n * nch;
    hipLaunchKernelGGL(phred64_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, d_text, d_rec, n, nch);
    return hipGetLastError();
}

hipError_t fq_launch_cuts(const uint32_t* d_size0, const uint32_t* d_off0, const uint32_t* d_size1, const uint32_t* d_off1, int n,
                          uint64_t every, uint64_t first, uint32_t pieces, fq_cut* d_cuts, hipStream_t s) {
    if (n <= 0 || !pieces) return hipSuccess;
    hipLaunchKernelGGL(cuts_kernel, dim3(pieces), dim3(64), 0, s, d_size0, d_off0, d_size1, d_off1, (uint32_t)n,
                       (unsigned long long)every, (unsigned long long)first, pieces, d_cuts);
    return hipGetLastError();
}
