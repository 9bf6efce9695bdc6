// deflate.hip -- BGZF members compressed on the device (include/fqengine.h, "device BGZF").
//
// Two kernels: fq_deflate_kernel compresses each member of the text (65280 input bytes, the last
// one shorter) with one 256-thread workgroup into a fixed 64 KiB slot of a scratch buffer
// (deflate_core.h has the routine); fq_compact_kernel prefix-sums the member sizes and moves the
// members into one contiguous stream, and writes its length.  The text's length is read on the
// device (the engine knows only a bound of it when it enqueues the kernels), so the grids are
// sized by that bound and workgroups beyond the real length leave at once.
// fq_deflate_spans_kernel / fq_compact_spans_kernel do the same for up to six texts at once (a
// routed pack's streams): one global member index runs over all of them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "engine_internal.h"
#include "deflate_core.h"

__global__ __launch_bounds__(FQ_DEFL_THREADS) void fq_deflate_kernel(const uint8_t* text, const unsigned long long* d_n,
                                                                     unsigned long long cap, int level, uint32_t* tok,
                                                                     uint8_t* slots, uint32_t* sizes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fq_defl_lds[];
    unsigned long long n = *d_n;
    if (n > cap) n = cap;
    const unsigned long long nmem = (n + FQ_BGZF_IN - 1) / FQ_BGZF_IN;
    uint32_t* mytok = tok + (size_t)blockIdx.x * FQ_BGZF_IN;
    for (unsigned long long m = blockIdx.x; m < nmem; m += gridDim.x) {
        const unsigned long long at = m * FQ_BGZF_IN;
        const uint32_t len = (uint32_t)std::min<unsigned long long>(FQ_BGZF_IN, n - at);
        const uint32_t sz = fq_deflate_member(fq_defl_lds, text + at, len, level, mytok, slots + m * FQ_DEFL_SLOT);
        if (threadIdx.x == 0) sizes[m] = sz;
    }
}

__global__ __launch_bounds__(256) void fq_compact_kernel(const unsigned long long* d_n, unsigned long long cap,
                                                         const uint8_t* slots, const uint32_t* sizes, uint8_t* dst,
                                                         unsigned long long dst_cap, unsigned long long* d_total) {
    __shared__ unsigned long long part[256];
    const uint32_t tid = threadIdx.x;
    unsigned long long n = *d_n;
    if (n > cap) n = cap;
    const unsigned long long nmem = (n + FQ_BGZF_IN - 1) / FQ_BGZF_IN;
    if (nmem == 0 && blockIdx.x == 0 && tid == 0) *d_total = 0;
    for (unsigned long long m = blockIdx.x; m < nmem; m += gridDim.x) {
        const unsigned long long end = fq_compact_member(part, slots, sizes, 0, m, dst, dst_cap);
        if (m == nmem - 1 && tid == 0) *d_total = end;
    }
}

// ---- several spans by one launch (the routed egress's streams) -------------------------------------
// The table goes to the kernels by value; every workgroup reads the length words and derives the same
// layout, then takes every gridDim.x-th member of all spans (deflate_core.h has both walks).
static_assert(FQ_DEFL_SPANS == FQ_EG_STREAMS && FQ_DEFL_MEMBER_IN == FQ_BGZF_IN, "deflate_core.h restates fqengine.h");

__global__ __launch_bounds__(FQ_DEFL_THREADS) void fq_deflate_spans_kernel(fq_span_table t, unsigned long long members, int level,
                                                                           uint32_t* tok, uint8_t* slots, uint32_t* sizes) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fq_defl_lds[];
    fq_deflate_spans_walk(fq_defl_lds, t, members, level, tok + (size_t)blockIdx.x * FQ_BGZF_IN, slots, sizes, blockIdx.x,
                          gridDim.x);
}

__global__ __launch_bounds__(256) void fq_compact_spans_kernel(fq_span_table t, unsigned long long members, const uint8_t* slots,
                                                               const uint32_t* sizes, unsigned long long* totals, int* err) {
    __shared__ unsigned long long part[256];
    fq_compact_spans_walk(part, t, members, slots, sizes, totals, err, blockIdx.x, gridDim.x);
}

static size_t members_of(size_t bytes) { return (bytes + FQ_BGZF_IN - 1) / FQ_BGZF_IN; }

void fq_deflate_scratch_free(fq_deflate_scratch& sc) {
    if (sc.tok) (void)hipFree(sc.tok);
    if (sc.slots) (void)hipFree(sc.slots);
    if (sc.sizes) (void)hipFree(sc.sizes);
    if (sc.total) (void)hipFree(sc.total);
    sc = fq_deflate_scratch();
}

hipError_t fq_deflate_scratch_ensure(fq_deflate_scratch& sc, size_t max_bytes, int cus) {
    const size_t members = std::max<size_t>(1, members_of(max_bytes));
    if (members <= sc.members) return hipSuccess;
    hipError_t e = hipFuncSetAttribute((const void*)fq_deflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FQ_DL_TOTAL);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)fq_deflate_spans_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FQ_DL_TOTAL);
    if (e != hipSuccess) return e;
    fq_deflate_scratch_free(sc);  // (hipFree waits for the device: no launch still uses the old buffers)
    const int grid = (int)std::min<size_t>(members, (size_t)2 * std::max(1, cus));
    if ((e = hipMalloc(&sc.tok, (size_t)grid * FQ_BGZF_IN * sizeof(uint32_t))) != hipSuccess) return e;
    if ((e = hipMalloc(&sc.slots, members * FQ_DEFL_SLOT)) != hipSuccess) return e;
    if ((e = hipMalloc(&sc.sizes, members * sizeof(uint32_t))) != hipSuccess) return e;
    if ((e = hipMalloc(&sc.total, FQ_EG_STREAMS * sizeof(unsigned long long))) != hipSuccess) return e;
    sc.members = members;
    sc.grid = grid;
    sc.cus = std::max(1, cus);
    return hipSuccess;
}

hipError_t fq_launch_deflate(const fq_deflate_scratch& sc, const void* d_text, const unsigned long long* d_n, size_t cap_bytes,
                             int level, void* d_dst, size_t dst_cap, unsigned long long* d_total, hipStream_t s) {
    const size_t members = members_of(cap_bytes);
    if (members > sc.members || level < 1 || level > 9) return hipErrorInvalidValue;
    if (members == 0) return hipMemsetAsync(d_total, 0, sizeof(unsigned long long), s);
    const int grid = (int)std::min<size_t>(members, (size_t)sc.grid);
    hipLaunchKernelGGL(fq_deflate_kernel, dim3(grid), dim3(FQ_DEFL_THREADS), FQ_DL_TOTAL, s, (const uint8_t*)d_text, d_n,
                       (unsigned long long)cap_bytes, level, sc.tok, sc.slots, sc.sizes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int cgrid = (int)std::min<size_t>(members, (size_t)4 * sc.cus);
    hipLaunchKernelGGL(fq_compact_kernel, dim3(cgrid), dim3(256), 0, s, d_n, (unsigned long long)cap_bytes, sc.slots, sc.sizes,
                       (uint8_t*)d_dst, (unsigned long long)dst_cap, sc.total);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // (d_total may be the word d_n points to: it is replaced only after both kernels have read it)
    return hipMemcpyAsync(d_total, sc.total, sizeof(unsigned long long), hipMemcpyDeviceToDevice, s);
}

hipError_t fq_launch_deflate_spans(const fq_deflate_scratch& sc, const fq_deflate_span* spans, int level,
                                   unsigned long long* d_totals, int* d_err, hipStream_t s) {
    if (level < 1 || level > 9 || !sc.members) return hipErrorInvalidValue;
    fq_span_table t{};
    size_t bound = 0;  // members the capacities allow
    for (int k = 0; k < FQ_EG_STREAMS; ++k) {
        if (!spans[k].d_n || !spans[k].d_text || !spans[k].cap_bytes) continue;
        t.text[k] = (uint8_t*)spans[k].d_text;
        t.n[k] = spans[k].d_n;
        t.cap[k] = spans[k].cap_bytes;
        bound += members_of(spans[k].cap_bytes);
    }
    if (bound == 0) return hipMemsetAsync(d_totals, 0, FQ_EG_STREAMS * sizeof(unsigned long long), s);
    const size_t most = std::min(bound, sc.members);
    const int grid = (int)std::min<size_t>(most, (size_t)sc.grid);
    hipLaunchKernelGGL(fq_deflate_spans_kernel, dim3(grid), dim3(FQ_DEFL_THREADS), FQ_DL_TOTAL, s, t,
                       (unsigned long long)sc.members, level, sc.tok, sc.slots, sc.sizes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int cgrid = (int)std::min<size_t>(most, (size_t)4 * sc.cus);
    hipLaunchKernelGGL(fq_compact_spans_kernel, dim3(cgrid), dim3(256), 0, s, t, (unsigned long long)sc.members, sc.slots,
                       sc.sizes, sc.total, d_err);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // (d_totals may be the spans' length words: they are replaced only after both kernels have read them)
    return hipMemcpyAsync(d_totals, sc.total, FQ_EG_STREAMS * sizeof(unsigned long long), hipMemcpyDeviceToDevice, s);
}

struct fq_deflate {
    int device = 0;
    size_t max_bytes = 0;
    fq_deflate_scratch sc;
    uint8_t* d_buf = nullptr;  // the text in, the stream out (fq_deflate_bound(max_bytes))
    unsigned long long* d_n = nullptr;
    hipStream_t stream = nullptr;
};

extern "C" {

size_t fq_deflate_bound(size_t n) { return n + 31 * members_of(n); }

int fq_deflate_code_lengths(const uint32_t* freq, int32_t n_sym, int32_t max_len, uint8_t* len) {
    if (!freq || !len || n_sym < 1 || n_sym > 288 || max_len < 1 || max_len > 15) return FQ_E_INVALID;
    unsigned long long sum = 0;
    for (int i = 0; i < n_sym; ++i) sum += freq[i];
    if (sum * (unsigned)max_len >= (1ull << 32)) return FQ_E_INVALID;  // (the builder's weights are 32-bit)
    std::vector<uint32_t> ws(fq_huff_ws_words(n_sym, max_len));
    return fq_huff_code_lengths(freq, n_sym, max_len, len, ws.data()) == 0 ? FQ_OK : FQ_E_INVALID;
}

int fq_deflate_destroy(fq_deflate* d) {
    if (!d) return FQ_OK;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    fq_deflate_scratch_free(d->sc);
    if (d->d_buf) (void)hipFree(d->d_buf);
    if (d->d_n) (void)hipFree(d->d_n);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
    return FQ_OK;
}

int fq_deflate_create(int device, size_t max_bytes, fq_deflate** out) {
    if (!out) return FQ_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FQ_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return FQ_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return FQ_E_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FQ_E_NO_DEVICE;
    if (max_bytes >= ((size_t)1 << 40)) return FQ_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FQ_E_HIP;
    fq_deflate* d = new fq_deflate();
    d->device = device;
    d->max_bytes = max_bytes;
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess ||
        fq_deflate_scratch_ensure(d->sc, max_bytes, prop.multiProcessorCount) != hipSuccess ||
        hipMalloc(&d->d_buf, std::max<size_t>(16, fq_deflate_bound(max_bytes))) != hipSuccess ||
        hipMalloc(&d->d_n, sizeof(unsigned long long)) != hipSuccess) {
        fq_deflate_destroy(d);
        return FQ_E_HIP;
    }
    *out = d;
    return FQ_OK;
}

int fq_deflate_bgzf(fq_deflate* d, const void* text, size_t n, int32_t level, void* out, size_t out_cap, size_t* out_bytes) {
    if (!d || !out_bytes || (n && (!text || !out))) return FQ_E_INVALID;
    *out_bytes = 0;
    if (n > d->max_bytes || level < 1 || level > 9 || out_cap < fq_deflate_bound(n)) return FQ_E_INVALID;
    if (n == 0) return FQ_OK;
    if (hipSetDevice(d->device) != hipSuccess) return FQ_E_HIP;
    const unsigned long long nn = n;
    unsigned long long total = 0;
    // the stream is compacted over the text: the members are in their slots before compaction starts
    if (hipMemcpyAsync(d->d_buf, text, n, hipMemcpyHostToDevice, d->stream) != hipSuccess ||
        hipMemcpyAsync(d->d_n, &nn, sizeof nn, hipMemcpyHostToDevice, d->stream) != hipSuccess ||
        fq_launch_deflate(d->sc, d->d_buf, d->d_n, n, level, d->d_buf, fq_deflate_bound(n), d->d_n, d->stream) != hipSuccess ||
        hipMemcpyAsync(&total, d->d_n, sizeof total, hipMemcpyDeviceToHost, d->stream) != hipSuccess ||
        hipStreamSynchronize(d->stream) != hipSuccess)
        return FQ_E_HIP;
    if (total > out_cap || total > fq_deflate_bound(n)) return FQ_E_HIP;
    if (hipMemcpy(out, d->d_buf, total, hipMemcpyDeviceToHost) != hipSuccess) return FQ_E_HIP;
    *out_bytes = (size_t)total;
    return FQ_OK;
}

}  // extern "C"
