// inflate.hip -- BGZF members inflated on the device (include/fqengine.h, "device inflate").
//
// fq_inflate_kernel: one wave64 per workgroup, one member per wave at a time (inflate_core.h has
// the routine); fq_inflate_spans_kernel is the same for the raw stream's BGZF windows.  The grid is four workgroups per CU (the output window lives in LDS, ~38 KiB a
// wave) and strides over the members.  The host side validates every descriptor before anything
// is copied or launched, so the kernel sees only payloads inside the compressed buffer and output
// ranges inside the output buffer; what the payload bytes say is the kernel's to survive.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "engine_internal.h"
#include "inflate_core.h"

static_assert(FQ_INFLATE_MAX == FQ_INFLATE_MAX_BYTES, "fqengine.h and inflate_core.h disagree");
static_assert(FQ_INFL_OK == FQ_IS_OK && FQ_INFL_DATA == FQ_IS_DATA && FQ_INFL_LONG == FQ_IS_LONG &&
                  FQ_INFL_SHORT == FQ_IS_SHORT && FQ_INFL_CRC == FQ_IS_CRC,
              "fqengine.h and inflate_core.h disagree");
static_assert(sizeof(fq_inflate_member) == 32, "fq_inflate_member layout");

__global__ __launch_bounds__(64) void fq_inflate_kernel(const uint8_t* comp, fq_inflate_member* m, const unsigned long long* out_off,
                                                        uint32_t n, uint8_t* out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fq_infl_lds[];
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        // (the host checked the limits; clamped again so that no descriptor can widen an access)
        const uint32_t in_len = std::min<uint32_t>(m[i].in_len, FQ_INFLATE_MAX);
        const uint32_t isize = std::min<uint32_t>(m[i].isize, FQ_INFLATE_MAX);
        uint32_t produced = 0;
        const uint32_t st = fq_inflate_one(fq_infl_lds, comp + m[i].in_off, in_len, isize, m[i].crc, out + out_off[i], produced);
        if (threadIdx.x == 0) {
            m[i].status = st;
            m[i].produced = produced;
        }
    }
}

// The raw stream's BGZF windows: the members of both mates in one table, claimed in table order from
// a device counter (lane 0 takes the next index and broadcasts it), so the two mates share one grid
// and one tail.  Same LDS and registers per wave as fq_inflate_kernel.
__global__ __launch_bounds__(64) void fq_inflate_spans_kernel(fq_inflate_spans a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fq_infl_lds[];
    for (;;) {
        uint32_t i = 0;
        if (threadIdx.x == 0) i = atomicAdd(&a.ctl[0], 1u);
        i = fq_uni(i);
        if (i >= a.n) break;
        const fq_raw_bgzf_desc d = a.desc[i];
        const uint32_t mate = fq_uni(d.mate) & 1u;
        // (the host checked the limits; clamped again so that no descriptor can widen an access)
        const uint32_t in_len = std::min<uint32_t>(fq_uni(d.in_len), FQ_INFLATE_MAX);
        const uint32_t isize = std::min<uint32_t>(fq_uni(d.isize), FQ_INFLATE_MAX);
        uint32_t produced = 0;
        const uint32_t st = fq_inflate_one(fq_infl_lds, a.comp[mate] + fq_uni(d.in_off), in_len, isize, fq_uni(d.crc),
                                           a.out[mate] + fq_uni(d.out_off), produced);
        if (st != FQ_IS_OK && threadIdx.x == 0) atomicAdd(&a.ctl[1 + mate], 1u);
    }
}

hipError_t fq_inflate_spans_prepare() {
    return hipFuncSetAttribute((const void*)fq_inflate_spans_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FQ_IL_TOTAL);
}

hipError_t fq_launch_inflate_spans(const fq_inflate_spans& a, int cus, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const int grid = (int)std::min<size_t>(a.n, (size_t)4 * std::max(1, cus));
    hipLaunchKernelGGL(fq_inflate_spans_kernel, dim3(grid), dim3(64), FQ_IL_TOTAL, s, a);
    return hipGetLastError();
}

struct fq_inflate {
    int device = 0;
    int cus = 1;
    size_t max_in = 0, max_out = 0, max_members = 0;
    uint8_t* d_comp = nullptr;
    uint8_t* d_out = nullptr;
    fq_inflate_member* d_m = nullptr;
    unsigned long long* d_off = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_ms = 0;
    std::vector<fq_inflate_member> hm;
    std::vector<unsigned long long> hoff;
};

extern "C" {

int fq_inflate_destroy(fq_inflate* h) {
    if (!h) return FQ_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->d_comp) (void)hipFree(h->d_comp);
    if (h->d_out) (void)hipFree(h->d_out);
    if (h->d_m) (void)hipFree(h->d_m);
    if (h->d_off) (void)hipFree(h->d_off);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return FQ_OK;
}

int fq_inflate_create(int device, size_t max_in, size_t max_out, size_t max_members, fq_inflate** out) {
    if (!out) return FQ_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FQ_E_NO_DEVICE;
    if (device < 0 || device >= ndev) return FQ_E_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return FQ_E_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FQ_E_NO_DEVICE;
    const size_t lim = (size_t)1 << 40;
    if (max_in >= lim || max_out >= lim || max_members >= ((size_t)1 << 31)) return FQ_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FQ_E_HIP;
    fq_inflate* h = new fq_inflate();
    h->device = device;
    h->cus = std::max(1, prop.multiProcessorCount);
    h->max_in = max_in;
    h->max_out = max_out;
    h->max_members = max_members;
    const size_t nm = std::max<size_t>(1, max_members);
    if (hipFuncSetAttribute((const void*)fq_inflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FQ_IL_TOTAL) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
        hipMalloc(&h->d_comp, std::max<size_t>(16, max_in)) != hipSuccess ||
        hipMalloc(&h->d_out, std::max<size_t>(16, max_out)) != hipSuccess ||
        hipMalloc(&h->d_m, nm * sizeof(fq_inflate_member)) != hipSuccess ||
        hipMalloc(&h->d_off, nm * sizeof(unsigned long long)) != hipSuccess) {
        fq_inflate_destroy(h);
        return FQ_E_HIP;
    }
    *out = h;
    return FQ_OK;
}

int fq_inflate_members(fq_inflate* h, const void* comp, size_t comp_bytes, fq_inflate_member* m, size_t n, void* out,
                       size_t out_cap, size_t* n_bad) {
    if (!h || !n_bad || (n && !m)) return FQ_E_INVALID;
    *n_bad = 0;
    if (n > h->max_members || comp_bytes > h->max_in || (comp_bytes && !comp)) return FQ_E_INVALID;
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        if (m[i].in_len > FQ_INFLATE_MAX || m[i].isize > FQ_INFLATE_MAX) return FQ_E_INVALID;
        if (m[i].in_off > comp_bytes || m[i].in_len > comp_bytes - m[i].in_off) return FQ_E_INVALID;
        total += m[i].isize;
    }
    if (total > h->max_out || total > out_cap || (total && !out)) return FQ_E_INVALID;
    if (n == 0) return FQ_OK;
    h->hm.assign(m, m + n);
    h->hoff.resize(n);
    unsigned long long at = 0;
    for (size_t i = 0; i < n; ++i) {
        h->hoff[i] = at;
        at += m[i].isize;
        h->hm[i].status = FQ_INFL_DATA;
        h->hm[i].produced = 0;
    }
    if (hipSetDevice(h->device) != hipSuccess) return FQ_E_HIP;
    const int grid = (int)std::min<size_t>(n, (size_t)4 * h->cus);
    if ((comp_bytes && hipMemcpyAsync(h->d_comp, comp, comp_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess) ||
        hipMemcpyAsync(h->d_m, h->hm.data(), n * sizeof(fq_inflate_member), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(h->d_off, h->hoff.data(), n * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipEventRecord(h->ev0, h->stream) != hipSuccess)
        return FQ_E_HIP;
    hipLaunchKernelGGL(fq_inflate_kernel, dim3(grid), dim3(64), FQ_IL_TOTAL, h->stream, (const uint8_t*)h->d_comp, h->d_m,
                       (const unsigned long long*)h->d_off, (uint32_t)n, h->d_out);
    if (hipGetLastError() != hipSuccess || hipEventRecord(h->ev1, h->stream) != hipSuccess ||
        hipMemcpyAsync(h->hm.data(), h->d_m, n * sizeof(fq_inflate_member), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        (total && hipMemcpyAsync(out, h->d_out, total, hipMemcpyDeviceToHost, h->stream) != hipSuccess) ||
        hipStreamSynchronize(h->stream) != hipSuccess)
        return FQ_E_HIP;
    float ms = 0;
    h->last_ms = hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess ? (double)ms : 0.0;
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) {
        m[i].status = h->hm[i].status;
        m[i].produced = std::min(h->hm[i].produced, m[i].isize);
        bad += m[i].status != FQ_INFL_OK;
    }
    *n_bad = bad;
    return FQ_OK;
}

// the member chain of a BGZF image from its headers, by the rules of the tool's reader (fastq.cpp,
// BgzfSource::walk): RFC 1952 header with FEXTRA and the 'BC' subfield, optional FNAME / FCOMMENT /
// FHCRC, the members covering the bytes exactly
static bool fq_bgzf_walk(const uint8_t* p, size_t size, std::vector<fq_inflate_member>& ms) {
    auto le16 = [](const uint8_t* q) { return (uint32_t)q[0] | (uint32_t)q[1] << 8; };
    auto le32 = [&](const uint8_t* q) { return le16(q) | le16(q + 2) << 16; };
    for (size_t o = 0; o < size;) {
        const uint8_t* hd = p + o;
        if (size - o < 28 || hd[0] != 0x1f || hd[1] != 0x8b || hd[2] != 8 || !(hd[3] & 4) || (hd[3] & 0xe0)) return false;
        const size_t xlen = le16(hd + 10);
        if (12 + xlen > size - o) return false;
        size_t bsize = 0;
        for (size_t x = 12; x + 4 <= 12 + xlen;) {
            const size_t slen = le16(hd + x + 2);
            if (hd[x] == 'B' && hd[x + 1] == 'C' && slen == 2 && x + 6 <= 12 + xlen) bsize = le16(hd + x + 4) + 1;
            x += 4 + slen;
        }
        size_t q = 12 + xlen;
        auto skipz = [&]() {
            while (o + q < size && hd[q]) ++q;
            ++q;
        };
        if (hd[3] & 8) skipz();   // FNAME
        if (hd[3] & 16) skipz();  // FCOMMENT
        if (hd[3] & 2) q += 2;    // FHCRC
        if (!bsize || bsize > size - o || q + 8 > bsize) return false;
        fq_inflate_member mb;
        std::memset(&mb, 0, sizeof mb);
        mb.in_off = o + q;
        mb.in_len = (uint32_t)(bsize - q - 8);
        mb.crc = le32(hd + bsize - 8);
        mb.isize = le32(hd + bsize - 4);
        ms.push_back(mb);
        o += bsize;
    }
    return !ms.empty();
}

int fq_inflate_bgzf(fq_inflate* h, const void* bgzf, size_t n, void* out, size_t out_cap, size_t* out_bytes,
                    int64_t* first_bad) {
    if (!h || !bgzf || !out_bytes || !first_bad) return FQ_E_INVALID;
    *out_bytes = 0;
    *first_bad = -1;
    std::vector<fq_inflate_member> ms;
    if (!fq_bgzf_walk((const uint8_t*)bgzf, n, ms)) return FQ_E_INVALID;
    size_t bad = 0;
    const int rc = fq_inflate_members(h, bgzf, n, ms.data(), ms.size(), out, out_cap, &bad);
    if (rc != FQ_OK) return rc;
    size_t total = 0;
    for (size_t i = 0; i < ms.size(); ++i) {
        total += ms[i].isize;
        if (ms[i].status != FQ_INFL_OK && *first_bad < 0) *first_bad = (int64_t)i;
    }
    *out_bytes = total;
    return FQ_OK;
}

double fq_inflate_last_kernel_ms(const fq_inflate* h) { return h ? h->last_ms : 0.0; }

}  // extern "C"
