// engine.hip -- the C-ABI (include/fqengine.h) over the gfx950 kernels.
//
// No CPU fallback: creation fails with FQ_E_NO_DEVICE unless a gfx950 device is present.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <deque>
#include <mutex>
#include <unordered_map>
#include <vector>
#include <sys/mman.h>
#include <string>

// profiling only (FQ_PROF_NO_EGRESS=1): raw packs copy no output text back and report none, to
// time the pipeline without its device-to-host leg (the outputs are empty)
static bool prof_no_egress() {
    static const bool on = std::getenv("FQ_PROF_NO_EGRESS") != nullptr;
    return on;
}

#include "engine_internal.h"
#include "ingest_core.h"

// Tile list the fast kernel hands to the general kernel (one per concurrently running launch).
struct Scratch {
    int* slow_tiles = nullptr;
    int* slow_count = nullptr;  // [0] the list's length, [1] the fast kernel's tile claim counter
    size_t slow_cap = 0;
    int* tile_ctr() const { return slow_count + 1; }
};

// One in-flight pack of the asynchronous pipeline (fq_engine_submit / fq_engine_poll): its own
// device copy of the batch, result records and hand-off list, and the events that order
//   H2D (stream in) -> kernels (compute stream) -> D2H of the records (stream out).
struct Slot {
    uint8_t* d_rows = nullptr;  // 4 planes of fq_batch_bytes(max_batch, max_stride)
    uint16_t* d_lens = nullptr;  // 2 x max_batch
    uint8_t* d_flags = nullptr;  // max_batch per-pair FQ_BF_* flags
    fq_read_result* d_res = nullptr;
    Scratch scratch;
    hipEvent_t ev_in = nullptr, ev_kern = nullptr, ev_done = nullptr;
    // FASTQ-text packs (fq_engine_submit_text): per mate text, records, output text, sizes, offsets
    char* d_text[2] = {nullptr, nullptr};
    char* d_out[2] = {nullptr, nullptr};
    size_t text_cap[2] = {0, 0};
    fq_text_rec* d_trec[2] = {nullptr, nullptr};
    uint32_t* d_tsize[2] = {nullptr, nullptr};
    uint32_t* d_toff[2] = {nullptr, nullptr};
    size_t trec_cap = 0;
    void* d_scan = nullptr;
    size_t scan_bytes = 0;
    unsigned long long* d_total = nullptr;  // [2]
    unsigned long long* h_total = nullptr;  // pinned [2]
    fq_text_out* text_out = nullptr;        // the pending text pack's output descriptor
    // routed egress (fq_engine_submit_text_routed): per open stream sizes, cursors and output text
    uint32_t* d_egsize[FQ_EG_STREAMS] = {};
    uint32_t* d_egoff[FQ_EG_STREAMS] = {};
    char* d_eg[FQ_EG_STREAMS] = {};
    size_t eg_cap[FQ_EG_STREAMS] = {};
    size_t eg_recs[FQ_EG_STREAMS] = {};
    unsigned long long* d_egtotal = nullptr;  // [FQ_EG_STREAMS]
    unsigned long long* h_egtotal = nullptr;  // pinned
    fq_egress_out* eg_out = nullptr;          // the pending routed pack's output descriptor
    fq_raw_egress_out* reg_out = nullptr;     // ... of a routed raw pack: its adapter entries too (from d_ad)
    // raw windows (fq_engine_raw_*): line index, block counts / bases, indexing state, adapter entries
    uint32_t* d_lines[2] = {nullptr, nullptr};
    uint32_t* d_bcnt[2] = {nullptr, nullptr};
    uint32_t* d_bbase[2] = {nullptr, nullptr};
    fq_raw_state* d_rstate = nullptr;  // [2]
    fq_raw_state* h_rstate = nullptr;  // pinned [2]
    char* d_ad[2] = {nullptr, nullptr};
    size_t ad_cap = 0;
    bool raw_ready = false;
    hipEvent_t ev_idx = nullptr;
    fq_raw_out* raw_out = nullptr;  // the pending raw pack's output descriptor
    uint64_t raw_n[2] = {0, 0};     // the window's raw bytes
    // BGZF windows (fq_engine_raw_enqueue_bgzf; made at the first one): each mate's compressed bytes,
    // the members' table (pinned copy and device copy), the claim counter and bad-member counts
    uint8_t* d_bcomp[2] = {nullptr, nullptr};
    size_t bcomp_cap[2] = {0, 0};
    fq_raw_bgzf_desc* h_bdesc = nullptr;  // pinned [2 * FQ_RAW_BGZF_MEMBERS]
    fq_raw_bgzf_desc* d_bdesc = nullptr;
    uint32_t* d_bctl = nullptr;           // [4]
    hipEvent_t ev_b0 = nullptr, ev_b1 = nullptr;  // FQ_ENGINE_TIMING: around the inflate
    bool b_timed = false;
    int* d_err = nullptr;  // this pack's device error word (cleared at submit, set by its kernels)
    int* h_err = nullptr;  // pinned: d_err as of this pack's kernels
    bool busy = false;      // events recorded and not yet waited for
    // raw packs: the output text is copied back once its size is known (issue_copies)
    bool copy_pending = false;
    char* copy_dst[2] = {nullptr, nullptr};
    size_t copy_cap[2] = {0, 0};
    // pack cuts (fq_engine_next_cuts): the pack's table on the device, where it goes on the host
    fq_cut* d_cuts = nullptr;
    size_t cuts_cap = 0;
};

// A submitted pack, in submission order, until fq_engine_poll reports it.
struct Pending {
    uint64_t seq_no;
    int slot;
    bool done;  // its slot's events completed (the slot may already serve a later pack)
    int err;
};

static const int kSlots = 3;     // host packs: H2D(k+1) || kernels(k) || D2H(k-1)
static const int kRawSlots = 8;  // raw windows: up to 3 enqueued + 5 launched, copies queued each way

struct fq_engine {
    fq_params p;
    int device = 0;
    int cus = 0;
    char arch[64] = {0};
    int32_t max_batch = 0, max_stride = 0;
    hipStream_t stream = nullptr;
    unsigned long long* acc = nullptr;      // accumulator in use
    unsigned long long* own_acc = nullptr;  // the engine's own buffer
    unsigned long long* xfix = nullptr;     // the fast kernels' exotic-byte Stats moves (fq_xfix_words)
    size_t acc_words = 0;
    int* err = nullptr;
    // host-memory path: pipeline slots and their streams
    Slot slots[kRawSlots];  // (host packs use the first kSlots)
    std::deque<Pending> pending;
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool fast = false;  // pe_fast kernel usable for these params
    Scratch scratch;    // hand-off list of fq_engine_process_device
    bool timed = false;
    // raw stream (fq_engine_raw_*): window / carry capacity, index stream, windows not yet launched
    bool raw = false;
    uint64_t raw_wcap = 0, raw_ccap = 0;
    uint32_t raw_nblocks = 0;
    hipStream_t s_idx = nullptr;
    std::deque<int> raw_queued;
    int raw_prev_slot = -1;
    fq_dup* dup = nullptr;    // duplication table fed by every pack (-d)
    fq_kstat* kstat = nullptr;  // k-mer tables fed by every pack (--kmer)
    fq_ora* ora = nullptr;      // overrepresented-sequence counts fed by every pack (--ora)
    // device BGZF (fq_engine_set_gz_out): level 1..9, 0 = off; the compressor's scratch, one per
    // engine (its launches all run on the compute stream, one after another)
    int gz_level = 0;
    fq_deflate_scratch gz;
    // routed egress (fq_engine_set_egress): the streams that have a writer
    bool eg_on = false;
    uint32_t eg_open = 0;
    // UMI description of the routed egress (fq_engine_set_umi)
    bool umi_on = false;
    fq_umi umi{};
    // device ingest: the index filter's lists (fq_engine_set_index_filter), --phred64
    bool idx_on = false;
    uint32_t* d_idx = nullptr;
    fq_index_lists idx{};
    bool phred64 = false;
    // pack cuts (fq_engine_set_cuts), and the table armed for the next pack (fq_engine_next_cuts)
    uint64_t cut_every = 0;
    bool cut_armed = false;
    uint64_t cut_first = 0;
    fq_cut* cut_host = nullptr;
    uint32_t cut_cap = 0;
    uint64_t calls = 0;       // order of process / process_device packs for the table
    std::string last_error;
};

static std::string g_create_error;

// FQ_ENGINE_TIMING=1: creation steps and the raw stream's one-time set-up on stderr (profiling)
static bool engine_timing() {
    static const bool on = std::getenv("FQ_ENGINE_TIMING") != nullptr;
    return on;
}
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Raw-window copies of the engines that share one GPU (and so one PCIe link) run one after another
// in call order: each engine's host-to-device copies wait for the last one another engine enqueued
// on the device (and likewise its device-to-host copies).  Left to share the link, the copies of a
// window that is due would finish only with those of the windows enqueued behind it on the other
// engines (the raw stream launches windows in order), so several engines on one GPU ran slower than
// one.  Engines on different GPUs never wait for each other.
struct LinkChain {
    std::mutex m;
    hipEvent_t in = nullptr, out = nullptr;  // the last copies enqueued on the device
    const fq_engine *in_owner = nullptr, *out_owner = nullptr;
};
static LinkChain& link_chain(int device) {
    static LinkChain chains[64];
    return chains[device & 63];
}

static int fail(fq_engine* e, int code, const std::string& msg) {
    if (e) e->last_error = msg;
    else g_create_error = msg;
    return code;
}

static int hip_fail(fq_engine* e, hipError_t err, const char* what) {
    return fail(e, FQ_E_HIP, std::string(what) + ": " + hipGetErrorString(err));
}

#define HIP_TRY(e, call)                                       \
    do {                                                       \
        hipError_t _err = (call);                              \
        if (_err != hipSuccess) return hip_fail(e, _err, #call); \
    } while (0)

static int validate_params(const fq_params* p, std::string& why) {
    if (p->max_cycles < 1 || p->max_cycles > FQ_MAX_CYCLES_LIMIT) return why = "max_cycles must be in [1, 4096]", FQ_E_INVALID;
    if (p->insert_size_max < 0 || p->insert_size_max > 100000) return why = "bad insert_size_max", FQ_E_INVALID;
    if (p->cut_front && p->cut_front_window < 1) return why = "cut_front window must be >= 1", FQ_E_INVALID;
    if (p->cut_right && p->cut_right_window < 1) return why = "cut_right window must be >= 1", FQ_E_INVALID;
    if (p->cut_tail && p->cut_tail_window < 1) return why = "cut_tail window must be >= 1", FQ_E_INVALID;
    if (p->polyg_enabled && p->polyg_one_mismatch_per < 1) return why = "polyG one-mismatch-per must be >= 1", FQ_E_INVALID;
    if (p->polyx_enabled && p->polyx_one_mismatch_per < 1) return why = "polyX one-mismatch-per must be >= 1", FQ_E_INVALID;
    if (p->adapter1_len < 0 || p->adapter1_len > FQ_MAX_ADAPTER || p->adapter2_len < 0 ||
        p->adapter2_len > FQ_MAX_ADAPTER)
        return why = "bad adapter length", FQ_E_INVALID;
    return FQ_OK;
}

static int ensure_scratch(fq_engine* e, Scratch& sc, size_t ntiles, bool sync_device) {
    if (!sc.slow_count) HIP_TRY(e, hipMalloc(&sc.slow_count, 2 * sizeof(int)));
    if (ntiles <= sc.slow_cap) return FQ_OK;
    // the old list may still be read by a launch in flight
    if (sync_device) HIP_TRY(e, hipDeviceSynchronize());
    if (sc.slow_tiles) HIP_TRY(e, hipFree(sc.slow_tiles));
    sc.slow_tiles = nullptr;
    sc.slow_cap = 0;
    HIP_TRY(e, hipMalloc(&sc.slow_tiles, ntiles * sizeof(int)));
    sc.slow_cap = ntiles;
    return FQ_OK;
}

static void free_scratch(Scratch& sc) {
    if (sc.slow_tiles) (void)hipFree(sc.slow_tiles);
    if (sc.slow_count) (void)hipFree(sc.slow_count);
    sc = Scratch();
}

static void free_slot(Slot& s) {
    if (s.d_rows) (void)hipFree(s.d_rows);
    if (s.d_lens) (void)hipFree(s.d_lens);
    if (s.d_flags) (void)hipFree(s.d_flags);
    if (s.d_cuts) (void)hipFree(s.d_cuts);
    if (s.d_res) (void)hipFree(s.d_res);
    for (int m = 0; m < 2; ++m) {
        if (s.d_text[m]) (void)hipFree(s.d_text[m]);
        if (s.d_out[m]) (void)hipFree(s.d_out[m]);
        if (s.d_trec[m]) (void)hipFree(s.d_trec[m]);
        if (s.d_tsize[m]) (void)hipFree(s.d_tsize[m]);
        if (s.d_toff[m]) (void)hipFree(s.d_toff[m]);
    }
    if (s.d_scan) (void)hipFree(s.d_scan);
    if (s.d_total) (void)hipFree(s.d_total);
    if (s.h_total) (void)hipHostFree(s.h_total);
    for (int k = 0; k < FQ_EG_STREAMS; ++k) {
        if (s.d_egsize[k]) (void)hipFree(s.d_egsize[k]);
        if (s.d_egoff[k]) (void)hipFree(s.d_egoff[k]);
        if (s.d_eg[k]) (void)hipFree(s.d_eg[k]);
    }
    if (s.d_egtotal) (void)hipFree(s.d_egtotal);
    if (s.h_egtotal) (void)hipHostFree(s.h_egtotal);
    for (int m = 0; m < 2; ++m) {
        if (s.d_lines[m]) (void)hipFree(s.d_lines[m]);
        if (s.d_bcnt[m]) (void)hipFree(s.d_bcnt[m]);
        if (s.d_bbase[m]) (void)hipFree(s.d_bbase[m]);
        if (s.d_ad[m]) (void)hipFree(s.d_ad[m]);
    }
    if (s.d_rstate) (void)hipFree(s.d_rstate);
    if (s.h_rstate) (void)hipHostFree(s.h_rstate);
    if (s.ev_idx) (void)hipEventDestroy(s.ev_idx);
    for (int m = 0; m < 2; ++m)
        if (s.d_bcomp[m]) (void)hipFree(s.d_bcomp[m]);
    if (s.h_bdesc) (void)hipHostFree(s.h_bdesc);
    if (s.d_bdesc) (void)hipFree(s.d_bdesc);
    if (s.d_bctl) (void)hipFree(s.d_bctl);
    if (s.ev_b0) (void)hipEventDestroy(s.ev_b0);
    if (s.ev_b1) (void)hipEventDestroy(s.ev_b1);
    if (s.d_err) (void)hipFree(s.d_err);
    if (s.h_err) (void)hipHostFree(s.h_err);
    if (s.ev_in) (void)hipEventDestroy(s.ev_in);
    if (s.ev_kern) (void)hipEventDestroy(s.ev_kern);
    if (s.ev_done) (void)hipEventDestroy(s.ev_done);
    free_scratch(s.scratch);
    s = Slot();
}

static int alloc_slot(fq_engine* e, Slot& s) {
    if (s.d_rows) return FQ_OK;
    const size_t rows = (size_t)4 * fq_batch_bytes(e->max_batch, e->max_stride);
    HIP_TRY(e, hipMalloc(&s.d_rows, rows));
    HIP_TRY(e, hipMalloc(&s.d_lens, (size_t)2 * e->max_batch * sizeof(uint16_t)));
    HIP_TRY(e, hipMalloc(&s.d_flags, (size_t)e->max_batch + 1));
    HIP_TRY(e, hipMalloc(&s.d_res, (size_t)2 * e->max_batch * sizeof(fq_read_result)));
    HIP_TRY(e, hipMalloc(&s.d_err, sizeof(int)));
    HIP_TRY(e, hipHostMalloc((void**)&s.h_err, sizeof(int), hipHostMallocDefault));
    *s.h_err = 0;
    HIP_TRY(e, hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming));
    HIP_TRY(e, hipEventCreateWithFlags(&s.ev_kern, hipEventDisableTiming));
    HIP_TRY(e, hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
    return FQ_OK;
}

extern "C" {

int fq_engine_create(const fq_params* params, int device, int32_t max_batch, int32_t max_stride, fq_engine** out) {
    if (!params || !out || max_batch < 0 || max_stride < 0 || (max_stride & 15))
        return fail(nullptr, FQ_E_INVALID, "fq_engine_create: bad arguments (stride must be a multiple of 16)");
    *out = nullptr;
    std::string why;
    if (validate_params(params, why) != FQ_OK) return fail(nullptr, FQ_E_INVALID, why);
    // FQ_ENGINE_TIMING=1: the creation's steps on stderr (profiling: start-up of the tool)
    const bool timing = engine_timing();
    const auto t0 = std::chrono::steady_clock::now();
    auto stamp = [&](const char* what) {
        if (timing)
            std::fprintf(stderr, "fq_engine_create: %s at %.4f s\n", what,
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, FQ_E_NO_DEVICE, "no HIP device visible (the engine has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(nullptr, FQ_E_NO_DEVICE, "device id out of range");
    stamp("runtime up (hipGetDeviceCount)");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return fail(nullptr, FQ_E_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, FQ_E_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", engine is built for gfx950");
    fq_engine* e = new fq_engine();
    e->p = *params;
    e->device = device;
    e->cus = prop.multiProcessorCount;
    std::snprintf(e->arch, sizeof e->arch, "%s", prop.gcnArchName);
    e->max_batch = max_batch;
    e->max_stride = max_stride;
    e->acc_words = fq_acc_words(params->insert_size_max, params->max_cycles);
    auto bail = [&](int rc) {
        g_create_error = e->last_error;
        fq_engine_destroy(e);
        return rc;
    };
    hipError_t he;
    if ((he = hipSetDevice(device)) != hipSuccess) return bail(hip_fail(e, he, "hipSetDevice"));
    for (hipStream_t* s : {&e->stream, &e->s_in, &e->s_out})
        if ((he = hipStreamCreateWithFlags(s, hipStreamNonBlocking)) != hipSuccess)
            return bail(hip_fail(e, he, "hipStreamCreate"));
    if ((he = hipMalloc(&e->own_acc, e->acc_words * 8)) != hipSuccess) return bail(hip_fail(e, he, "hipMalloc acc"));
    e->acc = e->own_acc;
    if ((he = hipMalloc(&e->err, sizeof(int))) != hipSuccess) return bail(hip_fail(e, he, "hipMalloc err"));
    if ((he = hipMemset(e->acc, 0, e->acc_words * 8)) != hipSuccess) return bail(hip_fail(e, he, "hipMemset"));
    const size_t xw = fq_xfix_words(params->max_cycles);
    if ((he = hipMalloc(&e->xfix, xw * 8)) != hipSuccess) return bail(hip_fail(e, he, "hipMalloc xfix"));
    if ((he = hipMemset(e->xfix, 0, xw * 8)) != hipSuccess) return bail(hip_fail(e, he, "hipMemset"));
    if ((he = hipMemset(e->err, 0, sizeof(int))) != hipSuccess) return bail(hip_fail(e, he, "hipMemset"));
    stamp("streams and accumulators");
    // the first pipeline slot up front, so an engine that cannot hold one pack fails here
    if (max_batch > 0 && max_stride > 0 && alloc_slot(e, e->slots[0]) != FQ_OK) return bail(FQ_E_HIP);
    stamp("first slot");
    if ((he = hipEventCreate(&e->ev0)) != hipSuccess) return bail(hip_fail(e, he, "hipEventCreate"));
    if ((he = hipEventCreate(&e->ev1)) != hipSuccess) return bail(hip_fail(e, he, "hipEventCreate"));
    if (fq_pack_kernel_lds_bytes(e->p) > 160 * 1024)
        return bail(fail(e, FQ_E_INVALID, "insert_size_max too large for the LDS-privatised accumulators"));
    if ((he = fq_pack_kernel_set_lds(e->p)) != hipSuccess) return bail(hip_fail(e, he, "hipFuncSetAttribute"));
    const char* force_general = std::getenv("FQ_ENGINE_GENERAL_ONLY");
    e->fast = fq_pe_fast_supported(e->p) && !(force_general && force_general[0] == '1');
    stamp("general kernel attributes");
    if (e->fast) {
        if ((he = fq_pe_fast_prepare()) != hipSuccess) return bail(hip_fail(e, he, "hipFuncSetAttribute fast"));
    }
    stamp("fast kernel attributes");
    *out = e;
    return FQ_OK;
}

int fq_engine_destroy(fq_engine* e) {
    if (!e) return FQ_OK;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    {
        LinkChain& lc = link_chain(e->device);  // (its events are about to go)
        std::lock_guard<std::mutex> g(lc.m);
        if (lc.in_owner == e) lc.in = nullptr, lc.in_owner = nullptr;
        if (lc.out_owner == e) lc.out = nullptr, lc.out_owner = nullptr;
    }
    if (e->own_acc) (void)hipFree(e->own_acc);
    if (e->xfix) (void)hipFree(e->xfix);
    if (e->err) (void)hipFree(e->err);
    if (e->d_idx) (void)hipFree(e->d_idx);
    for (Slot& s : e->slots) free_slot(s);
    free_scratch(e->scratch);
    fq_deflate_scratch_free(e->gz);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    for (hipStream_t s : {e->stream, e->s_in, e->s_out, e->s_idx})
        if (s) (void)hipStreamDestroy(s);
    delete e;
    return FQ_OK;
}

static int grid_for(const fq_engine* e, int n) {
    const size_t lds = fq_pack_kernel_lds_bytes(e->p);
    int per_cu = (int)((160 * 1024) / (lds ? lds : 1));
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    const int cap = e->cus * per_cu;
    const int need = (n + kPackThreads - 1) / kPackThreads;
    return need < cap ? (need > 0 ? need : 1) : cap;
}

// Enqueues the kernels of one batch on stream s.  `sc` is the hand-off list of this launch; it
// must not be shared with a launch that can run concurrently (different stream).
static int launch(fq_engine* e, const fq_batch& db, fq_read_result* dres, hipStream_t s, Scratch& sc, bool timed,
                  bool sync_device_on_grow, uint64_t order, int* derr) {
    if (db.n <= 0) return FQ_OK;
    if (e->dup) {  // Duplicate::statPair / statRead run on the untrimmed reads (src/peprocessor.cpp:279-281)
        const int rc = fq_dup_pack(e->dup, db, e->p.paired, order, s);
        if (rc != FQ_OK) return fail(e, rc, std::string("duplication analysis: ") + fq_dup_error(e->dup));
    }
    if (e->kstat) {  // the pre-filter k-mers, before -c rewrites the planes (src/peprocessor.cpp:276-277)
        int rc = FQ_OK;
        if (!dres) rc = fq_kstat_records(e->kstat, (size_t)db.n * (e->p.paired ? 2 : 1), s, &dres);
        if (rc == FQ_OK) rc = fq_kstat_pre(e->kstat, db, e->p, s);
        if (rc != FQ_OK) return fail(e, rc, std::string("k-mer statistics: ") + fq_kstat_error(e->kstat));
    }
    if (e->ora) {  // likewise the pre-filter overrepresented sequences
        int rc = FQ_OK;
        if (!dres) rc = fq_ora_records(e->ora, (size_t)db.n * (e->p.paired ? 2 : 1), s, &dres);
        if (rc == FQ_OK) rc = fq_ora_pre(e->ora, db, e->p, s);
        if (rc != FQ_OK) return fail(e, rc, std::string("overrepresented sequences: ") + fq_ora_error(e->ora));
    }
    // (index-filtered pairs are handed to the general kernel one by one)
    if (e->fast) {
        // hand-off list: pair / read indices, reserved a tile's worth (<= 64) at a time, at most
        // one reservation per tile, so at most n + 64 slots (holes included)
        const size_t nitems = (size_t)db.n + 64 + 1;
        int rc = ensure_scratch(e, sc, nitems, sync_device_on_grow);
        if (rc != FQ_OK) return rc;
        HIP_TRY(e, hipMemsetAsync(sc.slow_count, 0, 2 * sizeof(int), s));  // (both counters, every launch)
        if (timed) HIP_TRY(e, hipEventRecord(e->ev0, s));
        HIP_TRY(e, fq_launch_pe_fast(e->p, db, dres, e->acc, sc.slow_tiles, sc.slow_count, sc.tile_ctr(), e->xfix, e->cus, s));
        HIP_TRY(e, fq_launch_xfix_fold(e->acc + fq_acc_stats_offset(e->p.insert_size_max, e->p.max_cycles, 0), e->xfix,
                                       e->p.max_cycles, s));
        // (the hand-off list's length is known on the device only: as many workgroups as the
        // batch could need, at the occupancy the kernel's LDS allows; empty ones exit at once)
        HIP_TRY(e, fq_launch_pack_kernel(e->p, db, dres, e->acc, derr, grid_for(e, db.n), s, sc.slow_tiles,
                                         sc.slow_count));
    } else {
        if (timed) HIP_TRY(e, hipEventRecord(e->ev0, s));
        HIP_TRY(e, fq_launch_pack_kernel(e->p, db, dres, e->acc, derr, grid_for(e, db.n), s));
    }
    if (timed) {
        HIP_TRY(e, hipEventRecord(e->ev1, s));
        e->timed = true;
    }
    if (e->kstat) {  // the post-filter k-mers, from the records the kernels above have written
        const int rc = fq_kstat_post(e->kstat, db, e->p, dres, s);
        if (rc != FQ_OK) return fail(e, rc, std::string("k-mer statistics: ") + fq_kstat_error(e->kstat));
    }
    if (e->ora) {  // and the post-filter overrepresented sequences
        const int rc = fq_ora_post(e->ora, db, e->p, dres, s);
        if (rc != FQ_OK) return fail(e, rc, std::string("overrepresented sequences: ") + fq_ora_error(e->ora));
    }
    return FQ_OK;
}

static int check_err(fq_engine* e) {
    int h = 0;
    HIP_TRY(e, hipMemcpy(&h, e->err, sizeof(int), hipMemcpyDeviceToHost));
    if (h) {
        HIP_TRY(e, hipMemset(e->err, 0, sizeof(int)));
        return fail(e, FQ_E_TOO_LONG, "a read is longer than max_cycles or the row stride");
    }
    return FQ_OK;
}

// gz on: an output buffer takes the BGZF stream of its text in place
static size_t out_alloc(const fq_engine* e, size_t bytes) { return e->gz_level ? fq_deflate_bound(bytes) : bytes; }

// Raw packs' copies back, exactly sized: a pack's kernels end by copying its output sizes to the
// host (on the compute stream, event ev_kern); once they are in, its text + adapter entries are
// copied back on the out stream (in submission order; the link chain orders the copies of engines
// sharing a GPU).  Copying the capacity bound instead carried the gap left by trimmed and dropped
// records and, with -m, mate 1's whole input-sized bound for its few entry bytes (the e2e C4 leg's
// copies back took 1.44x the C3 leg's).  upto = a slot: waits for the sizes of the packs up to
// and including that slot's; -1: issues what is ready, stopping at the first pack whose sizes are
// not in; -2: waits for all.
static int issue_copies(fq_engine* e, int upto) {
    for (Pending& q : e->pending) {
        if (q.done) continue;
        Slot& s = e->slots[q.slot];
        if (s.copy_pending) {
            if (upto == -1) {
                const hipError_t st = hipEventQuery(s.ev_kern);
                if (st == hipErrorNotReady) break;
                if (st != hipSuccess) return hip_fail(e, st, "hipEventQuery");
            } else {
                HIP_TRY(e, hipEventSynchronize(s.ev_kern));
            }
            s.copy_pending = false;
            LinkChain& lc = link_chain(e->device);
            std::lock_guard<std::mutex> g(lc.m);
            if (lc.out && lc.out_owner != e) HIP_TRY(e, hipStreamWaitEvent(e->s_out, lc.out, 0));
            for (int k = 0; k < FQ_EG_STREAMS && s.eg_out; ++k) {  // a routed pack: each open stream's text
                // (a total above the caller's capacity copies nothing and fails the pack at retire)
                const size_t bytes = (size_t)s.h_egtotal[k];
                if (bytes && s.eg_out->text[k] && bytes <= s.eg_out->cap[k] && bytes <= out_alloc(e, s.eg_cap[k]))
                    HIP_TRY(e, hipMemcpyAsync(s.eg_out->text[k], s.d_eg[k], bytes, hipMemcpyDeviceToHost, e->s_out));
            }
            for (int m = 0; m < 2 && s.reg_out; ++m) {  // a routed raw pack: its trimmed-adapter entries
                const unsigned long long ad = s.h_total[2 + m];
                if (ad && ad != ~0ull && s.reg_out->adapters[m] && ad <= s.reg_out->adapter_cap[m])
                    HIP_TRY(e, hipMemcpyAsync(s.reg_out->adapters[m], s.d_ad[m], (size_t)ad, hipMemcpyDeviceToHost, e->s_out));
            }
            for (int m = 0; m < 2 && !prof_no_egress() && !s.eg_out; ++m) {
                if (!s.copy_dst[m]) continue;
                const unsigned long long ad = s.h_total[2 + m];  // (~0: the entries overflowed, reported at retire)
                const size_t bytes = std::min<size_t>(s.copy_cap[m], (size_t)s.h_total[m] + (ad == ~0ull ? 0 : (size_t)ad));
                if (bytes) HIP_TRY(e, hipMemcpyAsync(s.copy_dst[m], s.d_out[m], bytes, hipMemcpyDeviceToHost, e->s_out));
            }
            HIP_TRY(e, hipEventRecord(s.ev_done, e->s_out));
            lc.out = s.ev_done, lc.out_owner = e;
        }
        if (q.slot == upto) break;
    }
    return FQ_OK;
}

// Waits for slot k's pack (if any) and records its completion in the pending list.
static int retire_slot(fq_engine* e, int k) {
    Slot& s = e->slots[k];
    if (!s.busy) return FQ_OK;
    if (s.copy_pending) {
        const int rc = issue_copies(e, k);
        if (rc != FQ_OK) return rc;
    }
    HIP_TRY(e, hipEventSynchronize(s.ev_done));
    s.busy = false;
    for (Pending& q : e->pending)
        if (q.slot == k && !q.done) {
            q.done = true;
            q.err = *s.h_err;
        }
    if (s.text_out) {  // a text pack: its output sizes are in now
        s.text_out->bytes[0] = s.h_total[0];
        s.text_out->bytes[1] = s.h_total[1];
        s.text_out = nullptr;
    }
    if (s.eg_out) {  // a routed pack: its streams' sizes
        fq_egress_out* o = s.eg_out;
        fq_raw_egress_out* ro = s.reg_out;
        s.eg_out = nullptr;
        s.reg_out = nullptr;
        for (int k = 0; k < FQ_EG_STREAMS; ++k) {
            o->bytes[k] = s.h_egtotal[k];
            if (o->bytes[k] > o->cap[k] || o->bytes[k] > out_alloc(e, s.eg_cap[k])) {
                o->bytes[k] = 0;
                return fail(e, FQ_E_INVALID, "routed pack: a stream exceeds its buffer");
            }
        }
        for (int m = 0; m < 2 && ro; ++m) {
            ro->adapter_bytes[m] = s.h_total[2 + m];
            if (ro->adapter_bytes[m] == ~0ull || ro->adapter_bytes[m] > ro->adapter_cap[m]) {
                ro->adapter_bytes[m] = 0;
                return fail(e, FQ_E_INVALID, "routed raw pack: adapter entries exceed their buffer");
            }
        }
    }
    if (s.raw_out) {  // a raw pack: its trimmed-adapter entries follow the output text
        fq_raw_out* o = s.raw_out;
        s.raw_out = nullptr;
        for (int m = 0; m < 2; ++m) {
            o->adapter_bytes[m] = s.h_total[2 + m];
            if (o->adapter_bytes[m] == ~0ull) return fail(e, FQ_E_INVALID, "raw pack: adapter entries exceed the output copy");
            if (prof_no_egress()) o->adapter_bytes[m] = o->text.bytes[m] = 0;
        }
    }
    return FQ_OK;
}

// a text pack's output is at most its input plus the final line terminator an input may lack
static const size_t kTextSlack = 16;
// -m: mate 0's output is the merged stream, at most both mates' input plus a merged name's tag
// ("_merged_<m1>_<m2>", < 24 bytes) per pair
static size_t merged_cap(uint64_t text1, uint64_t text2, size_t pairs) {
    return (size_t)text1 + (size_t)text2 + 24 * pairs + kTextSlack;
}

// gz on: the scratch covers the largest text (growing it waits for the device)
static int ensure_gz(fq_engine* e, size_t text_bytes) {
    if (!e->gz_level) return FQ_OK;
    HIP_TRY(e, fq_deflate_scratch_ensure(e->gz, text_bytes, e->cus));
    return FQ_OK;
}
// mate m's output text (its length in d_total[m], at most cap bytes) -> BGZF members in place
static int launch_gz(fq_engine* e, Slot& s, int m, size_t cap) {
    HIP_TRY(e, fq_launch_deflate(e->gz, s.d_out[m], s.d_total + m, cap, e->gz_level, s.d_out[m], fq_deflate_bound(cap),
                                 s.d_total + m, e->stream));
    return FQ_OK;
}

// the output text of a text / raw pack: out1 (+ out2), or (-m) the merged stream into mate 0's buffer
static int launch_text_out(fq_engine* e, Slot& s, int n) {
    const bool pe = e->p.paired;
    if (pe && e->p.merge_enabled) {
        HIP_TRY(e, fq_launch_merge_out(s.d_text[0], s.d_text[1], s.d_trec[0], s.d_trec[1], s.d_res, n, e->p.discard_unmerged,
                                       s.d_tsize[0], s.d_toff[0], s.d_scan, s.scan_bytes, s.d_out[0], s.d_total, e->stream));
        HIP_TRY(e, hipMemsetAsync(s.d_total + 1, 0, sizeof(unsigned long long), e->stream));
        return FQ_OK;
    }
    for (int m = 0; m < (pe ? 2 : 1); ++m)
        HIP_TRY(e, fq_launch_text_out(s.d_text[m], s.d_trec[m], s.d_res, n, pe ? 1 : 0, m, s.d_tsize[m], s.d_toff[m],
                                      s.d_scan, s.scan_bytes, s.d_out[m], s.d_total + m, e->stream));
    if (!pe) HIP_TRY(e, hipMemsetAsync(s.d_total + 1, 0, sizeof(unsigned long long), e->stream));
    return FQ_OK;
}

// device buffers of a text pack (grown on demand; growing frees the old ones, which waits for the
// device, so steady-state packs of similar size reuse them)
static int ensure_text(fq_engine* e, Slot& s, const fq_text_batch* tb) {
    const bool pe = e->p.paired;
    const bool mrg = pe && e->p.merge_enabled;
    for (int m = 0; m < (pe ? 2 : 1); ++m) {
        size_t need = tb->text_bytes[m] + kTextSlack;
        // (-m: mate 0's output buffer takes the merged stream; the sizes go together)
        if (mrg && m == 0) need = merged_cap(tb->text_bytes[0], tb->text_bytes[1], (size_t)tb->n);
        if (need > s.text_cap[m]) {
            s.raw_ready = false;  // (the raw-window buffers are re-made by ensure_raw)
            if (s.d_text[m]) (void)hipFree(s.d_text[m]);
            if (s.d_out[m]) (void)hipFree(s.d_out[m]);
            s.d_text[m] = s.d_out[m] = nullptr;
            s.text_cap[m] = 0;
            const size_t cap = need + need / 8;
            HIP_TRY(e, hipMalloc(&s.d_text[m], cap));
            HIP_TRY(e, hipMalloc(&s.d_out[m], out_alloc(e, cap)));
            s.text_cap[m] = cap;
        }
        const int rc = ensure_gz(e, s.text_cap[m]);
        if (rc != FQ_OK) return rc;
    }
    if ((size_t)tb->n > s.trec_cap || !s.d_total) {
        s.raw_ready = false;
        const size_t cap = (size_t)tb->n + (size_t)tb->n / 8 + 1;
        for (int m = 0; m < 2; ++m) {
            if (s.d_trec[m]) (void)hipFree(s.d_trec[m]);
            if (s.d_tsize[m]) (void)hipFree(s.d_tsize[m]);
            if (s.d_toff[m]) (void)hipFree(s.d_toff[m]);
            s.d_trec[m] = nullptr;
            s.d_tsize[m] = s.d_toff[m] = nullptr;
        }
        if (s.d_scan) (void)hipFree(s.d_scan);
        s.d_scan = nullptr;
        s.trec_cap = 0;
        for (int m = 0; m < 2; ++m) {
            HIP_TRY(e, hipMalloc(&s.d_trec[m], cap * sizeof(fq_text_rec)));
            HIP_TRY(e, hipMalloc(&s.d_tsize[m], cap * sizeof(uint32_t)));
            HIP_TRY(e, hipMalloc(&s.d_toff[m], cap * sizeof(uint32_t)));
        }
        s.scan_bytes = fq_text_scan_temp_bytes((int)cap);
        HIP_TRY(e, hipMalloc(&s.d_scan, s.scan_bytes ? s.scan_bytes : 1));
        if (!s.d_total) HIP_TRY(e, hipMalloc(&s.d_total, 4 * sizeof(unsigned long long)));
        if (!s.h_total) HIP_TRY(e, hipHostMalloc((void**)&s.h_total, 4 * sizeof(unsigned long long), hipHostMallocDefault));
        s.trec_cap = cap;
    }
    return FQ_OK;
}

// ---- device ingest and pack cuts (ingest.hip) -------------------------------------------------

// the setters' call-time rule: nothing pending or enqueued, not inside a raw stream
static int idle_for(fq_engine* e, const char* what) {
    if (!e->pending.empty() || !e->raw_queued.empty()) return fail(e, FQ_E_INVALID, std::string(what) + " with packs in flight");
    if (e->raw) return fail(e, FQ_E_INVALID, std::string(what) + " inside a raw stream");
    return FQ_OK;
}

int fq_engine_set_index_filter(fq_engine* e, const fq_index_filter* f) {
    if (!e) return FQ_E_INVALID;
    const int rc = idle_for(e, "fq_engine_set_index_filter");
    if (rc != FQ_OK) return rc;
    std::vector<uint32_t> blob;
    fq_index_lists L{};
    if (f) {
        if (f->threshold < 0 || f->reserved) return fail(e, FQ_E_INVALID, "fq_engine_set_index_filter: threshold must be >= 0, reserved 0");
        uint64_t len[2] = {0, 0};
        for (int m = 0; m < 2; ++m) {
            const int32_t n = f->n[m];
            if (n < 0 || (n > 0 && (!f->off[m] || f->off[m][0] != 0)))
                return fail(e, FQ_E_INVALID, "fq_engine_set_index_filter: a list needs n >= 0 and n + 1 offsets from 0");
            for (int32_t i = 0; i < n; ++i)
                if (f->off[m][i + 1] < f->off[m][i] || f->off[m][i + 1] - f->off[m][i] > 65535u)
                    return fail(e, FQ_E_INVALID, "fq_engine_set_index_filter: offsets must not decrease, entries hold at most 65535 bytes");
            len[m] = n ? f->off[m][n] : 0;
            if (len[m] && !f->list[m]) return fail(e, FQ_E_INVALID, "fq_engine_set_index_filter: missing list bytes");
        }
        const uint64_t head = 4ull * ((uint64_t)f->n[0] + (uint64_t)f->n[1] + 2), total = head + len[0] + len[1];
        if (total >= (1ull << 31)) return fail(e, FQ_E_INVALID, "fq_engine_set_index_filter: the lists exceed 2 GiB");
        blob.assign((size_t)((total + 3) / 4), 0u);
        uint32_t* o = blob.data();
        for (int m = 0; m < 2; ++m) {
            for (int32_t i = 0; i <= f->n[m]; ++i) o[i] = f->n[m] ? f->off[m][i] : 0u;
            o += f->n[m] + 1;
        }
        uint8_t* b = reinterpret_cast<uint8_t*>(o);
        if (len[0]) std::memcpy(b, f->list[0], (size_t)len[0]);
        if (len[1]) std::memcpy(b + len[0], f->list[1], (size_t)len[1]);
        L.blob_bytes = (uint32_t)total;
        L.n1 = (uint32_t)f->n[0], L.n2 = (uint32_t)f->n[1];
        L.len1 = (uint32_t)len[0];
        L.threshold = f->threshold;
    }
    HIP_TRY(e, hipSetDevice(e->device));
    if (e->d_idx) (void)hipFree(e->d_idx);  // (nothing is in flight: no kernel reads the old lists)
    e->d_idx = nullptr;
    e->idx_on = false;
    e->idx = fq_index_lists{};
    if (f) {
        HIP_TRY(e, hipMalloc(&e->d_idx, blob.size() * sizeof(uint32_t)));
        HIP_TRY(e, hipMemcpy(e->d_idx, blob.data(), blob.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        L.blob = e->d_idx;
        e->idx = L;
        e->idx_on = true;
    }
    return FQ_OK;
}

int fq_engine_set_phred64(fq_engine* e, int on) {
    if (!e) return FQ_E_INVALID;
    const int rc = idle_for(e, "fq_engine_set_phred64");
    if (rc != FQ_OK) return rc;
    if (on != 0 && on != 1) return fail(e, FQ_E_INVALID, "fq_engine_set_phred64: on must be 0 or 1");
    e->phred64 = on != 0;
    return FQ_OK;
}

size_t fq_cuts_bound(uint64_t every, uint64_t n) { return every ? (size_t)(n / every + 2) : 0; }
size_t fq_cuts_count(uint64_t every, uint64_t first_item, uint32_t n) {
    return every ? (size_t)fqingest::cut_count(every, first_item, n) : 0;
}

int fq_engine_set_cuts(fq_engine* e, uint64_t every) {
    if (!e) return FQ_E_INVALID;
    const int rc = idle_for(e, "fq_engine_set_cuts");
    if (rc != FQ_OK) return rc;
    if (every && e->p.paired && e->p.merge_enabled) return fail(e, FQ_E_INVALID, "fq_engine_set_cuts: the merged stream (-m) takes no cuts");
    if (every && e->gz_level) return fail(e, FQ_E_INVALID, "fq_engine_set_cuts: no cuts while device BGZF output is on");
    e->cut_every = every;
    e->cut_armed = false;
    return FQ_OK;
}

int fq_engine_next_cuts(fq_engine* e, uint64_t first_item, fq_cut* cuts, uint32_t cap) {
    if (!e) return FQ_E_INVALID;
    if (!e->cut_every) return fail(e, FQ_E_INVALID, "fq_engine_next_cuts without fq_engine_set_cuts");
    if (!cuts || !cap) return fail(e, FQ_E_INVALID, "fq_engine_next_cuts: missing table");
    e->cut_armed = true;
    e->cut_first = first_item;
    e->cut_host = cuts;
    e->cut_cap = cap;
    return FQ_OK;
}

// a plain pack of n records against the armed table, before anything is launched
static int check_cuts(fq_engine* e, int n) {
    if (e->cut_armed && (size_t)e->cut_cap < fq_cuts_bound(e->cut_every, (uint64_t)n))
        return fail(e, FQ_E_INVALID, "pack cuts: the table is below fq_cuts_bound");
    return FQ_OK;
}

// the ingest kernels of a text / raw pack whose text and records are in the slot, in front of its
// tile kernels: the index filter's flags (which the device batch then carries), --phred64
static int launch_ingest(fq_engine* e, Slot& s, int n, int stride, fq_batch& db) {
    const bool pe = e->p.paired;
    if (e->idx_on) {
        HIP_TRY(e, fq_launch_index_flags(e->idx, s.d_text[0], s.d_trec[0], pe ? s.d_text[1] : nullptr, pe ? s.d_trec[1] : nullptr,
                                         n, s.d_flags, e->stream));
        db.flags = s.d_flags;
    }
    if (e->phred64)
        for (int m = 0; m < (pe ? 2 : 1); ++m) HIP_TRY(e, fq_launch_phred64(s.d_text[m], s.d_trec[m], n, stride, e->stream));
    return FQ_OK;
}

// the armed cut table of the pack launch_text_out has just sized, into the slot's device table
// (*pieces entries, which the caller copies to e->cut_host behind the kernels)
static int launch_cuts(fq_engine* e, Slot& s, int n, uint32_t* pieces) {
    *pieces = (uint32_t)fq_cuts_count(e->cut_every, e->cut_first, (uint32_t)n);
    if ((size_t)*pieces > s.cuts_cap) {
        if (s.d_cuts) (void)hipFree(s.d_cuts);
        s.d_cuts = nullptr;
        s.cuts_cap = 0;
        const size_t cap = (size_t)*pieces + (size_t)*pieces / 8 + 1;
        HIP_TRY(e, hipMalloc(&s.d_cuts, cap * sizeof(fq_cut)));
        s.cuts_cap = cap;
    }
    const bool pe = e->p.paired;
    HIP_TRY(e, fq_launch_cuts(s.d_tsize[0], s.d_toff[0], pe ? s.d_tsize[1] : nullptr, pe ? s.d_toff[1] : nullptr, n, e->cut_every,
                              e->cut_first, *pieces, s.d_cuts, e->stream));
    return FQ_OK;
}

static int validate_host_batch(fq_engine* e, const fq_batch* hb) {
    const bool pe = e->p.paired;
    if (hb->n < 0 || hb->n > e->max_batch || hb->stride <= 0 || hb->stride > e->max_stride || (hb->stride & 15))
        return fail(e, FQ_E_INVALID, "batch exceeds the engine's max_batch/max_stride (or stride % 16 != 0)");
    if (!hb->seq1 || !hb->qual1 || !hb->len1 || (pe && (!hb->seq2 || !hb->qual2 || !hb->len2)))
        return fail(e, FQ_E_INVALID, "missing batch arrays");
    // -c hands the host the overlap offset of a corrected pair in a 16-bit signed record field
    if (e->p.correction_enabled && hb->stride > 32768)
        return fail(e, FQ_E_INVALID, "-c takes reads of at most 32767 bases (the record's overlap offset is 16-bit)");
    // (read lengths are checked on the device: a read longer than max_cycles or the stride sets
    // the pack's error word, which fq_engine_poll reports as FQ_E_TOO_LONG)
    return FQ_OK;
}

int fq_engine_submit(fq_engine* e, const fq_batch* hb, fq_read_result* results, uint64_t seq_no) {
    if (!e || !hb || !results) return FQ_E_INVALID;
    int rc = validate_host_batch(e, hb);
    if (rc != FQ_OK) return rc;
    if (hb->n == 0) {  // nothing to move: complete at once, in order
        e->pending.push_back(Pending{seq_no, -1, true, 0});
        return FQ_OK;
    }
    HIP_TRY(e, hipSetDevice(e->device));
    // the slot after the newest pack's (round robin), once its previous pack has drained
    int k = 0;
    for (auto it = e->pending.rbegin(); it != e->pending.rend(); ++it)
        if (it->slot >= 0) {
            k = (it->slot + 1) % kSlots;
            break;
        }
    if ((rc = retire_slot(e, k)) != FQ_OK) return rc;
    Slot& s = e->slots[k];
    if ((rc = alloc_slot(e, s)) != FQ_OK) return rc;
    const bool pe = e->p.paired;
    const size_t rowbytes = fq_batch_bytes(hb->n, hb->stride);
    const size_t plane = fq_batch_bytes(e->max_batch, e->max_stride);
    fq_batch db{};
    db.n = hb->n;
    db.stride = hb->stride;
    db.seq1 = s.d_rows;
    db.qual1 = s.d_rows + plane;
    db.len1 = s.d_lens;
    db.seq2 = pe ? s.d_rows + 2 * plane : nullptr;
    db.qual2 = pe ? s.d_rows + 3 * plane : nullptr;
    db.len2 = pe ? s.d_lens + e->max_batch : nullptr;
    // H2D on the copy-in stream (overlaps the previous pack's kernels when the host batch is pinned)
    HIP_TRY(e, hipMemcpyAsync((void*)db.seq1, hb->seq1, rowbytes, hipMemcpyHostToDevice, e->s_in));
    HIP_TRY(e, hipMemcpyAsync((void*)db.qual1, hb->qual1, rowbytes, hipMemcpyHostToDevice, e->s_in));
    HIP_TRY(e, hipMemcpyAsync((void*)db.len1, hb->len1, (size_t)hb->n * 2, hipMemcpyHostToDevice, e->s_in));
    if (pe) {
        HIP_TRY(e, hipMemcpyAsync((void*)db.seq2, hb->seq2, rowbytes, hipMemcpyHostToDevice, e->s_in));
        HIP_TRY(e, hipMemcpyAsync((void*)db.qual2, hb->qual2, rowbytes, hipMemcpyHostToDevice, e->s_in));
        HIP_TRY(e, hipMemcpyAsync((void*)db.len2, hb->len2, (size_t)hb->n * 2, hipMemcpyHostToDevice, e->s_in));
    }
    if (hb->flags) {
        db.flags = s.d_flags;
        HIP_TRY(e, hipMemcpyAsync((void*)db.flags, hb->flags, (size_t)hb->n, hipMemcpyHostToDevice, e->s_in));
    }
    HIP_TRY(e, hipEventRecord(s.ev_in, e->s_in));
    // kernels on the compute stream (one accumulator: the packs' kernels run in order)
    HIP_TRY(e, hipStreamWaitEvent(e->stream, s.ev_in, 0));
    HIP_TRY(e, hipMemsetAsync(s.d_err, 0, sizeof(int), e->stream));
    if ((rc = launch(e, db, s.d_res, e->stream, s.scratch, false, false, seq_no, s.d_err)) != FQ_OK) return rc;
    HIP_TRY(e, hipEventRecord(s.ev_kern, e->stream));
    // D2H of the records (and of the error flag) on the copy-out stream
    HIP_TRY(e, hipStreamWaitEvent(e->s_out, s.ev_kern, 0));
    const size_t nres = (size_t)hb->n * (pe ? 2 : 1);
    if (nres)
        HIP_TRY(e, hipMemcpyAsync(results, s.d_res, nres * sizeof(fq_read_result), hipMemcpyDeviceToHost, e->s_out));
    HIP_TRY(e, hipMemcpyAsync(s.h_err, s.d_err, sizeof(int), hipMemcpyDeviceToHost, e->s_out));
    HIP_TRY(e, hipEventRecord(s.ev_done, e->s_out));
    s.busy = true;
    e->pending.push_back(Pending{seq_no, k, false, 0});
    return FQ_OK;
}

int fq_engine_submit_text(fq_engine* e, const fq_text_batch* tb, fq_read_result* results, fq_text_out* out,
                          uint64_t seq_no) {
    if (!e || !tb || !results || !out) return FQ_E_INVALID;
    const bool pe = e->p.paired;
    if (tb->n < 0 || tb->n > e->max_batch || tb->stride <= 0 || tb->stride > e->max_stride || (tb->stride & 15))
        return fail(e, FQ_E_INVALID, "text pack exceeds the engine's max_batch/max_stride (or stride % 16 != 0)");
    if (e->p.correction_enabled || e->p.umi_front1 > 0 || e->p.umi_front2 > 0 || e->umi_on ||
        (e->p.merge_enabled && e->p.discard_unmerged))
        return fail(e, FQ_E_INVALID, "text packs take no -c, UMI or --discard_unmerged options");
    for (int m = 0; m < (pe ? 2 : 1); ++m)
        if (tb->n > 0 && (!tb->text[m] || !tb->rec[m] || !out->text[m]))
            return fail(e, FQ_E_INVALID, "missing text pack arrays");
    const bool mrg = pe && e->p.merge_enabled;
    int rc = check_cuts(e, tb->n);
    if (rc != FQ_OK) return rc;
    const bool cut = e->cut_armed;
    out->bytes[0] = out->bytes[1] = 0;
    if (tb->n == 0) {
        e->cut_armed = false;  // (no records: no pieces)
        e->pending.push_back(Pending{seq_no, -1, true, 0});
        return FQ_OK;
    }
    HIP_TRY(e, hipSetDevice(e->device));
    int k = 0;
    for (auto it = e->pending.rbegin(); it != e->pending.rend(); ++it)
        if (it->slot >= 0) {
            k = (it->slot + 1) % kSlots;
            break;
        }
    if ((rc = retire_slot(e, k)) != FQ_OK) return rc;
    Slot& s = e->slots[k];
    if ((rc = alloc_slot(e, s)) != FQ_OK) return rc;
    if ((rc = ensure_text(e, s, tb)) != FQ_OK) return rc;
    const size_t plane = fq_batch_bytes(e->max_batch, e->max_stride);
    fq_batch db{};
    db.n = tb->n;
    db.stride = tb->stride;
    db.seq1 = s.d_rows;
    db.qual1 = s.d_rows + plane;
    db.len1 = s.d_lens;
    db.seq2 = pe ? s.d_rows + 2 * plane : nullptr;
    db.qual2 = pe ? s.d_rows + 3 * plane : nullptr;
    db.len2 = pe ? s.d_lens + e->max_batch : nullptr;
    // H2D of the text spans and records on the copy-in stream
    for (int m = 0; m < (pe ? 2 : 1); ++m) {
        HIP_TRY(e, hipMemcpyAsync(s.d_text[m], tb->text[m], tb->text_bytes[m], hipMemcpyHostToDevice, e->s_in));
        HIP_TRY(e, hipMemcpyAsync(s.d_trec[m], tb->rec[m], (size_t)tb->n * sizeof(fq_text_rec), hipMemcpyHostToDevice,
                                  e->s_in));
    }
    HIP_TRY(e, hipEventRecord(s.ev_in, e->s_in));
    HIP_TRY(e, hipStreamWaitEvent(e->stream, s.ev_in, 0));
    // the ingest kernels, planes from the text, the pack's kernels, then the output text
    if ((rc = launch_ingest(e, s, tb->n, tb->stride, db)) != FQ_OK) return rc;
    for (int m = 0; m < (pe ? 2 : 1); ++m)
        HIP_TRY(e, fq_launch_text_tiles(s.d_text[m], s.d_trec[m], tb->n, tb->stride, const_cast<uint8_t*>(m ? db.seq2 : db.seq1),
                                        const_cast<uint8_t*>(m ? db.qual2 : db.qual1), const_cast<uint16_t*>(m ? db.len2 : db.len1),
                                        e->stream));
    HIP_TRY(e, hipMemsetAsync(s.d_err, 0, sizeof(int), e->stream));
    if ((rc = launch(e, db, s.d_res, e->stream, s.scratch, false, false, seq_no, s.d_err)) != FQ_OK) return rc;
    if ((rc = launch_text_out(e, s, tb->n)) != FQ_OK) return rc;
    uint32_t pieces = 0;
    if (cut && (rc = launch_cuts(e, s, tb->n, &pieces)) != FQ_OK) return rc;
    size_t tback[2] = {0, 0};
    for (int m = 0; m < (mrg ? 1 : pe ? 2 : 1); ++m) {
        tback[m] = mrg ? merged_cap(tb->text_bytes[0], tb->text_bytes[1], (size_t)tb->n) : tb->text_bytes[m] + kTextSlack;
        if (e->gz_level && (rc = launch_gz(e, s, m, tback[m])) != FQ_OK) return rc;
    }
    const size_t nres = (size_t)tb->n * (pe ? 2 : 1);
    if (e->gz_level) {
        // gz: a bound of the stream would be more than the text, so the sizes come back first and
        // the copy back is exactly the members, as for raw packs (issue_copies)
        HIP_TRY(e, hipMemsetAsync(s.d_total + 2, 0, 2 * sizeof(unsigned long long), e->stream));  // (no adapter entries)
        HIP_TRY(e, hipMemcpyAsync(results, s.d_res, nres * sizeof(fq_read_result), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipMemcpyAsync(s.h_total, s.d_total, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipMemcpyAsync(s.h_err, s.d_err, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipEventRecord(s.ev_kern, e->stream));
        for (int m = 0; m < 2; ++m) {
            const bool has = m < (mrg ? 1 : pe ? 2 : 1);
            s.copy_dst[m] = has ? out->text[m] : nullptr;
            s.copy_cap[m] = has ? fq_deflate_bound(tback[m]) : 0;
        }
        s.copy_pending = true;
        s.busy = true;
        s.text_out = out;
        e->pending.push_back(Pending{seq_no, k, false, 0});
        return issue_copies(e, -1);
    }
    HIP_TRY(e, hipEventRecord(s.ev_kern, e->stream));
    // D2H: records, output sizes and text (the text up to its input span: an upper bound of the
    // output, no device-to-host round trip for the exact size), the error word
    HIP_TRY(e, hipStreamWaitEvent(e->s_out, s.ev_kern, 0));
    HIP_TRY(e, hipMemcpyAsync(results, s.d_res, nres * sizeof(fq_read_result), hipMemcpyDeviceToHost, e->s_out));
    HIP_TRY(e, hipMemcpyAsync(s.h_total, s.d_total, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->s_out));
    if (cut) {  // (cuts and device BGZF exclude each other: the table always goes back here)
        HIP_TRY(e, hipMemcpyAsync(e->cut_host, s.d_cuts, (size_t)pieces * sizeof(fq_cut), hipMemcpyDeviceToHost, e->s_out));
        e->cut_armed = false;
    }
    for (int m = 0; m < (mrg ? 1 : pe ? 2 : 1); ++m)
        HIP_TRY(e, hipMemcpyAsync(out->text[m], s.d_out[m], tback[m], hipMemcpyDeviceToHost, e->s_out));
    HIP_TRY(e, hipMemcpyAsync(s.h_err, s.d_err, sizeof(int), hipMemcpyDeviceToHost, e->s_out));
    HIP_TRY(e, hipEventRecord(s.ev_done, e->s_out));
    s.busy = true;
    s.text_out = out;
    e->pending.push_back(Pending{seq_no, k, false, 0});
    return FQ_OK;
}

// ---- routed egress ---------------------------------------------------------------------------

// a FAILED record: its input plus a blank and the longest tag ("paired_read_is_failing", 22 bytes)
static const size_t kFailedTag = 24;

size_t fq_egress_bound(int32_t stream, uint64_t text_bytes1, uint64_t text_bytes2, uint64_t n) {
    const bool pe = text_bytes2 != 0;
    switch (stream) {
        case FQ_EG_OUT1: case FQ_EG_UNPAIRED1: return (size_t)text_bytes1 + kTextSlack;
        case FQ_EG_OUT2: case FQ_EG_UNPAIRED2: return (size_t)text_bytes2 + kTextSlack;
        case FQ_EG_MERGED: return merged_cap(text_bytes1, text_bytes2, (size_t)n);
        case FQ_EG_FAILED: return (size_t)text_bytes1 + (size_t)text_bytes2 + kFailedTag * (size_t)n * (pe ? 2 : 1) + kTextSlack;
        default: return 0;
    }
}

// what the UMI tag can add to stream s (include/fqengine.h)
size_t fq_egress_bound_umi(int32_t stream, uint64_t text_bytes1, uint64_t text_bytes2, uint64_t n, const fq_umi* u) {
    const size_t base = fq_egress_bound(stream, text_bytes1, text_bytes2, n);
    if (!u || !base) return base;
    const bool pe = text_bytes2 != 0;
    const size_t L = (size_t)std::max<int32_t>(u->length, 0);
    // records of the stream, and how often one mate's name can recur in its tags
    const size_t recs = (size_t)n * ((stream == FQ_EG_MERGED || stream == FQ_EG_FAILED) && pe ? 2 : 1);
    const size_t per = recs / (n ? (size_t)n : 1);
    switch (u->location) {
        case 3: case 4: return base + recs * (12 + 2 * L);
        case 6: return base + recs * (14 + 4 * L);
        case 1: return base + recs * 6 + per * (size_t)text_bytes1;
        case 2: return base + recs * 6 + per * (size_t)text_bytes2;
        default: return base + recs * 7 + per * ((size_t)text_bytes1 + (size_t)text_bytes2);
    }
}

// gz on: what the open streams of one pack hold together (include/fqengine.h, "device BGZF"), as the
// bytes to size the compressor's scratch for: a member more per open stream for the short last ones
static size_t egress_gz_scratch_bytes(const fq_engine* e, uint64_t text1, uint64_t text2, uint64_t n) {
    return fq_egress_bound_umi(FQ_EG_FAILED, text1, text2, n, e->umi_on ? &e->umi : nullptr) +
           (size_t)__builtin_popcount(e->eg_open) * FQ_BGZF_IN;
}

// the description against the engine's params (Options::umi_front)
static bool umi_matches(const fq_params& p, const fq_umi& u) {
    const int front = u.not_trim ? 0 : u.length + u.skip;
    const bool r1 = u.location == 3 || u.location == 6, r2 = (u.location == 4 || u.location == 6) && p.paired;
    return p.umi_front1 == (r1 ? front : 0) && p.umi_front2 == (r2 ? front : 0);
}

int fq_engine_set_umi(fq_engine* e, const fq_umi* u) {
    if (!e) return FQ_E_INVALID;
    if (!e->pending.empty() || !e->raw_queued.empty()) return fail(e, FQ_E_INVALID, "fq_engine_set_umi with packs in flight");
    if (e->raw) return fail(e, FQ_E_INVALID, "fq_engine_set_umi inside a raw stream");
    if (u) {
        if (u->location < 1 || u->location > 6 || u->length < 0 || u->skip < 0 || u->length > 65535 || u->skip > 65535)
            return fail(e, FQ_E_INVALID, "fq_engine_set_umi: location must be 1..6, length and skip 0..65535");
        if ((u->location == 3 || u->location == 4 || u->location == 6) && u->length == 0)
            return fail(e, FQ_E_INVALID, "fq_engine_set_umi: the UMI length can not be zero in read 1 / 2");
        if (u->drop_comment > 1 || u->not_trim > 1 || u->reserved[0] || u->reserved[1])
            return fail(e, FQ_E_INVALID, "fq_engine_set_umi: flags must be 0 or 1, reserved 0");
        if (!umi_matches(e->p, *u))
            return fail(e, FQ_E_INVALID, "fq_engine_set_umi: the description disagrees with the params' umi_front1/2");
    }
    for (Slot& s : e->slots) s.raw_ready = false;  // (raw slots carry the open streams' buffers at their bounds)
    e->umi_on = u != nullptr;
    e->umi = u ? *u : fq_umi{};
    return FQ_OK;
}

// the routed calls take UMI params only with a description set (which set_umi checked against them)
static bool umi_refused(const fq_engine* e) { return !e->umi_on && (e->p.umi_front1 > 0 || e->p.umi_front2 > 0); }
static const fq_umi* umi_of(const fq_engine* e) { return e->umi_on ? &e->umi : nullptr; }

int fq_engine_set_egress(fq_engine* e, const fq_egress* eg) {
    if (!e) return FQ_E_INVALID;
    if (!e->pending.empty() || !e->raw_queued.empty()) return fail(e, FQ_E_INVALID, "fq_engine_set_egress with packs in flight");
    if (eg && (eg->open >> FQ_EG_STREAMS)) return fail(e, FQ_E_INVALID, "fq_engine_set_egress: unknown stream bits");
    if (e->raw) return fail(e, FQ_E_INVALID, "fq_engine_set_egress inside a raw stream");
    for (Slot& s : e->slots) s.raw_ready = false;  // (raw slots carry the open streams' buffers)
    e->eg_on = eg != nullptr;
    e->eg_open = eg ? eg->open : 0;
    return FQ_OK;
}

// the routed pack's per-stream device buffers (grown on demand, as ensure_text's)
static int ensure_egress_caps(fq_engine* e, Slot& s, uint64_t text1, uint64_t text2, size_t n);
static int ensure_egress(fq_engine* e, Slot& s, const fq_text_batch* tb) {
    return ensure_egress_caps(e, s, tb->text_bytes[0], e->p.paired ? tb->text_bytes[1] : 0, (size_t)tb->n);
}
static int ensure_egress_caps(fq_engine* e, Slot& s, uint64_t text1, uint64_t text2, size_t n) {
    if (!s.d_egtotal) HIP_TRY(e, hipMalloc(&s.d_egtotal, FQ_EG_STREAMS * sizeof(unsigned long long)));
    if (!s.h_egtotal)
        HIP_TRY(e, hipHostMalloc((void**)&s.h_egtotal, FQ_EG_STREAMS * sizeof(unsigned long long), hipHostMallocDefault));
    const size_t recs = n + n / 8 + 1;
    for (int k = 0; k < FQ_EG_STREAMS; ++k) {
        if (!((e->eg_open >> k) & 1u)) continue;
        if (n > s.eg_recs[k]) {
            if (s.d_egsize[k]) (void)hipFree(s.d_egsize[k]);
            if (s.d_egoff[k]) (void)hipFree(s.d_egoff[k]);
            s.d_egsize[k] = s.d_egoff[k] = nullptr;
            s.eg_recs[k] = 0;
            HIP_TRY(e, hipMalloc(&s.d_egsize[k], recs * sizeof(uint32_t)));
            HIP_TRY(e, hipMalloc(&s.d_egoff[k], recs * sizeof(uint32_t)));
            s.eg_recs[k] = recs;
        }
        const size_t need = fq_egress_bound_umi(k, text1, text2, (uint64_t)n, umi_of(e));
        if (need > s.eg_cap[k]) {
            if (s.d_eg[k]) (void)hipFree(s.d_eg[k]);
            s.d_eg[k] = nullptr;
            s.eg_cap[k] = 0;
            const size_t cap = need + need / 8;
            HIP_TRY(e, hipMalloc(&s.d_eg[k], out_alloc(e, cap)));
            s.eg_cap[k] = cap;
        }
    }
    return ensure_gz(e, egress_gz_scratch_bytes(e, text1, text2, (uint64_t)n));
}

// gz on: every open stream's text (d_egtotal[q] bytes, at most bound[q]) -> BGZF members in place by
// one pair of launches, d_egtotal[q] = their bytes; a pack whose members exceed the scratch sets bit 1
// of the slot's error word
static int launch_gz_streams(fq_engine* e, Slot& s, const size_t (&bound)[FQ_EG_STREAMS]) {
    fq_deflate_span sp[FQ_EG_STREAMS] = {};
    for (int q = 0; q < FQ_EG_STREAMS; ++q)
        if ((e->eg_open >> q) & 1u) sp[q] = fq_deflate_span{s.d_eg[q], s.d_egtotal + q, std::min(bound[q], s.eg_cap[q])};
    HIP_TRY(e, fq_launch_deflate_spans(e->gz, sp, e->gz_level, s.d_egtotal, s.d_err, e->stream));
    return FQ_OK;
}

int fq_engine_submit_text_routed(fq_engine* e, const fq_text_batch* tb, fq_read_result* results, fq_egress_out* out,
                                 uint64_t seq_no) {
    if (!e || !tb || !results || !out) return FQ_E_INVALID;
    const bool pe = e->p.paired;
    const int mates = pe ? 2 : 1;
    if (!e->eg_on) return fail(e, FQ_E_INVALID, "routed text pack without fq_engine_set_egress");
    if (e->raw) return fail(e, FQ_E_INVALID, "routed text pack inside a raw stream");
    if (e->cut_armed) return fail(e, FQ_E_INVALID, "routed text packs take no pack cuts");
    if (tb->n < 0 || tb->n > e->max_batch || tb->stride <= 0 || tb->stride > e->max_stride || (tb->stride & 15))
        return fail(e, FQ_E_INVALID, "text pack exceeds the engine's max_batch/max_stride (or stride % 16 != 0)");
    if (umi_refused(e)) return fail(e, FQ_E_INVALID, "routed text packs take no UMI options");
    if (e->p.correction_enabled && tb->stride > 32768)
        return fail(e, FQ_E_INVALID, "-c takes reads of at most 32767 bases (the record's overlap offset is 16-bit)");
    for (int m = 0; m < mates; ++m)
        if (tb->n > 0 && (!tb->text[m] || !tb->rec[m])) return fail(e, FQ_E_INVALID, "missing text pack arrays");
    // every open stream needs a buffer of at least its bound, before anything is launched or copied
    // (gz on: the bound of its BGZF stream)
    size_t bound[FQ_EG_STREAMS] = {};
    for (int k = 0; k < FQ_EG_STREAMS; ++k) {
        out->bytes[k] = 0;
        if (!((e->eg_open >> k) & 1u)) continue;
        const size_t need = fq_egress_bound_umi(k, tb->text_bytes[0], pe ? tb->text_bytes[1] : 0, (uint64_t)tb->n, umi_of(e));
        if (e->umi_on && need > 0xFFFFFFFFull) return fail(e, FQ_E_INVALID, "routed text pack: a UMI-tagged stream's bound exceeds the 32-bit cursors (submit smaller packs)");
        if (!out->text[k] || out->cap[k] < out_alloc(e, need))
            return fail(e, FQ_E_INVALID, "routed text pack: an open stream's buffer is missing or below fq_egress_bound");
        bound[k] = need;
    }
    if (tb->n == 0) {
        e->pending.push_back(Pending{seq_no, -1, true, 0});
        return FQ_OK;
    }
    HIP_TRY(e, hipSetDevice(e->device));
    int k = 0;
    for (auto it = e->pending.rbegin(); it != e->pending.rend(); ++it)
        if (it->slot >= 0) {
            k = (it->slot + 1) % kSlots;
            break;
        }
    int rc = retire_slot(e, k);
    if (rc != FQ_OK) return rc;
    Slot& s = e->slots[k];
    if ((rc = alloc_slot(e, s)) != FQ_OK) return rc;
    if ((rc = ensure_text(e, s, tb)) != FQ_OK) return rc;
    if ((rc = ensure_egress(e, s, tb)) != FQ_OK) return rc;
    const size_t plane = fq_batch_bytes(e->max_batch, e->max_stride);
    fq_batch db{};
    db.n = tb->n;
    db.stride = tb->stride;
    db.seq1 = s.d_rows;
    db.qual1 = s.d_rows + plane;
    db.len1 = s.d_lens;
    db.seq2 = pe ? s.d_rows + 2 * plane : nullptr;
    db.qual2 = pe ? s.d_rows + 3 * plane : nullptr;
    db.len2 = pe ? s.d_lens + e->max_batch : nullptr;
    for (int m = 0; m < mates; ++m) {
        HIP_TRY(e, hipMemcpyAsync(s.d_text[m], tb->text[m], tb->text_bytes[m], hipMemcpyHostToDevice, e->s_in));
        HIP_TRY(e, hipMemcpyAsync(s.d_trec[m], tb->rec[m], (size_t)tb->n * sizeof(fq_text_rec), hipMemcpyHostToDevice,
                                  e->s_in));
    }
    HIP_TRY(e, hipEventRecord(s.ev_in, e->s_in));
    HIP_TRY(e, hipStreamWaitEvent(e->stream, s.ev_in, 0));
    if ((rc = launch_ingest(e, s, tb->n, tb->stride, db)) != FQ_OK) return rc;
    for (int m = 0; m < mates; ++m)
        HIP_TRY(e, fq_launch_text_tiles(s.d_text[m], s.d_trec[m], tb->n, tb->stride, const_cast<uint8_t*>(m ? db.seq2 : db.seq1),
                                        const_cast<uint8_t*>(m ? db.qual2 : db.qual1), const_cast<uint16_t*>(m ? db.len2 : db.len1),
                                        e->stream));
    HIP_TRY(e, hipMemsetAsync(s.d_err, 0, sizeof(int), e->stream));
    if ((rc = launch(e, db, s.d_res, e->stream, s.scratch, false, false, seq_no, s.d_err)) != FQ_OK) return rc;
    // the six streams: corrected pairs (-c, PE) read their rows back from the planes
    fq_egress_args a{};
    fq_egress_streams st{};
    const bool planes = pe && e->p.correction_enabled;
    for (int m = 0; m < mates; ++m) {
        a.text[m] = s.d_text[m];
        a.rec[m] = s.d_trec[m];
        a.seq[m] = planes ? (m ? db.seq2 : db.seq1) : nullptr;
        a.qual[m] = planes ? (m ? db.qual2 : db.qual1) : nullptr;
    }
    a.res = s.d_res;
    a.n = tb->n, a.stride = tb->stride, a.paired = pe ? 1 : 0;
    a.merge = pe && e->p.merge_enabled, a.discard = e->p.discard_unmerged;
    a.open = e->eg_open;
    a.umi = umi_of(e);
    for (int q = 0; q < FQ_EG_STREAMS; ++q) st.size[q] = s.d_egsize[q], st.off[q] = s.d_egoff[q], st.out[q] = s.d_eg[q];
    st.total = s.d_egtotal;
    HIP_TRY(e, fq_launch_egress(a, st, s.d_scan, s.scan_bytes, e->stream));
    if (e->gz_level && (rc = launch_gz_streams(e, s, bound)) != FQ_OK) return rc;
    // records, sizes and the error word behind the kernels; each stream's text (gz: its members)
    // follows once the sizes are in (issue_copies)
    const size_t nres = (size_t)tb->n * mates;
    HIP_TRY(e, hipMemcpyAsync(results, s.d_res, nres * sizeof(fq_read_result), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(s.h_egtotal, s.d_egtotal, FQ_EG_STREAMS * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              e->stream));
    HIP_TRY(e, hipMemcpyAsync(s.h_err, s.d_err, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipEventRecord(s.ev_kern, e->stream));
    s.copy_dst[0] = s.copy_dst[1] = nullptr;
    s.copy_cap[0] = s.copy_cap[1] = 0;
    s.copy_pending = true;
    s.busy = true;
    s.eg_out = out;
    e->pending.push_back(Pending{seq_no, k, false, 0});
    return issue_copies(e, -1);
}

// ---- raw FASTQ streams -----------------------------------------------------------------------

// the raw-window buffers of slot s (the text-pack buffers at raw capacity plus the line index)
static int ensure_raw(fq_engine* e, Slot& s) {
    if (s.raw_ready) return FQ_OK;
    const bool pe = e->p.paired;
    const size_t text = (size_t)e->raw_nblocks * 4096;
    const size_t recs = (size_t)e->max_batch + 1;
    const size_t cap_lines = 4 * recs + 8;
    for (int m = 0; m < 2; ++m) {
        if (s.d_text[m]) (void)hipFree(s.d_text[m]);
        if (s.d_out[m]) (void)hipFree(s.d_out[m]);
        if (s.d_trec[m]) (void)hipFree(s.d_trec[m]);
        if (s.d_tsize[m]) (void)hipFree(s.d_tsize[m]);
        if (s.d_toff[m]) (void)hipFree(s.d_toff[m]);
        s.d_text[m] = s.d_out[m] = nullptr;
        s.d_trec[m] = nullptr;
        s.d_tsize[m] = s.d_toff[m] = nullptr;
        for (uint32_t** q : {&s.d_lines[m], &s.d_bcnt[m], &s.d_bbase[m]})
            if (*q) {
                (void)hipFree(*q);
                *q = nullptr;
            }
        if (s.d_ad[m]) (void)hipFree(s.d_ad[m]);
        s.d_ad[m] = nullptr;
        if (m == 1 && !pe) continue;
        HIP_TRY(e, hipMalloc(&s.d_text[m], text));
        // (+ the adapter entries' slack; -m: mate 0's takes the merged stream of both mates' text)
        const size_t out = pe && m == 0 && e->p.merge_enabled ? merged_cap(text, text, recs) + 3 * recs + 64 : text + 4 * recs + 64;
        HIP_TRY(e, hipMalloc(&s.d_out[m], out_alloc(e, out)));
        const int rc = ensure_gz(e, out);
        if (rc != FQ_OK) return rc;
        HIP_TRY(e, hipMalloc(&s.d_trec[m], recs * sizeof(fq_text_rec)));
        HIP_TRY(e, hipMalloc(&s.d_tsize[m], recs * sizeof(uint32_t)));
        HIP_TRY(e, hipMalloc(&s.d_toff[m], recs * sizeof(uint32_t)));
        HIP_TRY(e, hipMalloc(&s.d_lines[m], cap_lines * sizeof(uint32_t)));
        HIP_TRY(e, hipMalloc(&s.d_bcnt[m], (size_t)e->raw_nblocks * sizeof(uint32_t)));
        HIP_TRY(e, hipMalloc(&s.d_bbase[m], (size_t)e->raw_nblocks * sizeof(uint32_t)));

    }
    if (e->eg_on) {  // routed raw packs: every open stream at the window's capacity, the entries apart
        const int rc = ensure_egress_caps(e, s, text, pe ? text : 0, recs);
        if (rc != FQ_OK) return rc;
        for (int m = 0; m < (pe ? 2 : 1); ++m) HIP_TRY(e, hipMalloc(&s.d_ad[m], text + 3 * recs + 64));
        s.ad_cap = text + 3 * recs + 64;
    }
    s.text_cap[0] = s.text_cap[1] = 0;  // (not the text-pack sizes: ensure_text re-allocates)
    s.trec_cap = 0;
    if (s.d_scan) (void)hipFree(s.d_scan);
    s.scan_bytes = std::max(fq_raw_scan_temp_bytes((int)e->raw_nblocks, (int)recs), fq_text_scan_temp_bytes((int)recs));
    HIP_TRY(e, hipMalloc(&s.d_scan, s.scan_bytes));
    if (!s.d_total) HIP_TRY(e, hipMalloc(&s.d_total, 4 * sizeof(unsigned long long)));
    if (!s.h_total) HIP_TRY(e, hipHostMalloc((void**)&s.h_total, 4 * sizeof(unsigned long long), hipHostMallocDefault));
    if (!s.d_rstate) HIP_TRY(e, hipMalloc(&s.d_rstate, 2 * sizeof(fq_raw_state)));
    if (!s.h_rstate) HIP_TRY(e, hipHostMalloc((void**)&s.h_rstate, 2 * sizeof(fq_raw_state), hipHostMallocDefault));
    if (!s.ev_idx) HIP_TRY(e, hipEventCreateWithFlags(&s.ev_idx, hipEventDisableTiming));
    s.raw_ready = true;
    return FQ_OK;
}

int fq_engine_raw_begin(fq_engine* e, uint64_t window_cap, uint64_t carry_cap) {
    if (!e) return FQ_E_INVALID;
    if (!e->pending.empty() || !e->raw_queued.empty()) return fail(e, FQ_E_INVALID, "fq_engine_raw_begin with packs in flight");
    // (-c and --discard_unmerged: only with an egress set, whose packs fq_engine_raw_launch_routed writes)
    // (UMI: with an egress and a UMI description set)
    if ((e->umi_on && !e->eg_on) || (!(e->umi_on && e->eg_on) && (e->p.umi_front1 > 0 || e->p.umi_front2 > 0)) ||
        (!e->eg_on && (e->p.correction_enabled || (e->p.merge_enabled && e->p.discard_unmerged))))
        return fail(e, FQ_E_INVALID, "raw streams take no -c, UMI or --discard_unmerged options");
    if (e->p.correction_enabled && e->max_stride > 32768)
        return fail(e, FQ_E_INVALID, "-c takes reads of at most 32767 bases (the record's overlap offset is 16-bit)");
    const double tb = engine_timing() ? now_s() : 0;
    struct Stamp {
        double t;
        ~Stamp() {
            if (t > 0) std::fprintf(stderr, "fq_engine_raw_begin: %.2f ms\n", 1e3 * (now_s() - t));
        }
    } stamp{tb};
    carry_cap = (carry_cap + 4095) / 4096 * 4096;
    if (!window_cap || carry_cap + window_cap + 4096 >= (1ull << 31) || e->max_batch <= 0)
        return fail(e, FQ_E_INVALID, "raw window / carry capacity out of range");
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipDeviceSynchronize());
    if (!e->s_idx) HIP_TRY(e, hipStreamCreateWithFlags(&e->s_idx, hipStreamNonBlocking));
    const uint32_t nb = (uint32_t)((carry_cap + window_cap + 64 + 4095) / 4096);
    if (!e->raw || nb != e->raw_nblocks || carry_cap != e->raw_ccap)
        for (Slot& s : e->slots) s.raw_ready = false;
    e->raw = true;
    e->raw_wcap = window_cap;
    e->raw_ccap = carry_cap;
    e->raw_nblocks = nb;
    e->raw_prev_slot = -1;
    e->raw_queued.clear();
    return FQ_OK;
}

static int raw_index(fq_engine* e, int k, const uint64_t* n, const uint32_t* d_infl_bad);

int fq_engine_raw_enqueue(fq_engine* e, const fq_raw_window* w) {
    if (!e || !w) return FQ_E_INVALID;
    if (!e->raw) return fail(e, FQ_E_INVALID, "fq_engine_raw_enqueue before fq_engine_raw_begin");
    if (e->raw_queued.size() >= 3) return fail(e, FQ_E_INVALID, "three raw windows are already waiting for fq_engine_raw_launch");
    const bool pe = e->p.paired;
    for (int m = 0; m < (pe ? 2 : 1); ++m)
        if (w->n[m] > e->raw_wcap || (w->n[m] && !w->bytes[m])) return fail(e, FQ_E_INVALID, "raw window exceeds its capacity");
    HIP_TRY(e, hipSetDevice(e->device));
    const int k = (e->raw_prev_slot + 1) % kRawSlots;
    int rc = retire_slot(e, k);
    if (rc != FQ_OK) return rc;
    Slot& s = e->slots[k];
    const bool fresh = !s.raw_ready;
    const double ts = fresh && engine_timing() ? now_s() : 0;
    if ((rc = alloc_slot(e, s)) != FQ_OK) return rc;
    if ((rc = ensure_raw(e, s)) != FQ_OK) return rc;
    if (ts > 0) std::fprintf(stderr, "fq_engine_raw_enqueue: slot %d set up in %.2f ms\n", k, 1e3 * (now_s() - ts));
    {
        LinkChain& lc = link_chain(e->device);
        std::lock_guard<std::mutex> g(lc.m);
        if (lc.in && lc.in_owner != e) HIP_TRY(e, hipStreamWaitEvent(e->s_in, lc.in, 0));
        for (int m = 0; m < (pe ? 2 : 1); ++m)
            if (w->n[m])
                HIP_TRY(e, hipMemcpyAsync(s.d_text[m] + e->raw_ccap, w->bytes[m], w->n[m], hipMemcpyHostToDevice, e->s_in));
        HIP_TRY(e, hipEventRecord(s.ev_in, e->s_in));
        lc.in = s.ev_in, lc.in_owner = e;
    }
    HIP_TRY(e, hipStreamWaitEvent(e->s_idx, s.ev_in, 0));
    s.b_timed = false;
    return raw_index(e, k, w->n, nullptr);
}

// the index of slot k's window of n[m] bytes on the index stream, and the window enqueued
static int raw_index(fq_engine* e, int k, const uint64_t* n, const uint32_t* d_infl_bad) {
    Slot& s = e->slots[k];
    const bool pe = e->p.paired;
    s.raw_n[0] = n[0];
    s.raw_n[1] = pe ? n[1] : 0;
    fq_raw_text_args a{};
    const Slot* ps = e->raw_prev_slot >= 0 ? &e->slots[e->raw_prev_slot] : nullptr;
    for (int m = 0; m < 2; ++m) {
        a.text[m] = s.d_text[m];
        a.prev_text[m] = ps ? ps->d_text[m] : nullptr;
        a.raw_bytes[m] = (uint32_t)s.raw_n[m];
        a.bcnt[m] = s.d_bcnt[m];
        a.bbase[m] = s.d_bbase[m];
        a.lines[m] = s.d_lines[m];
        a.rec[m] = s.d_trec[m];
    }
    a.prev_state = ps ? ps->d_rstate : nullptr;
    a.state = s.d_rstate;
    a.infl_bad = d_infl_bad;
    a.carry_cap = (uint32_t)e->raw_ccap;
    a.nblocks = e->raw_nblocks;
    a.cap_lines = (uint32_t)(4 * ((size_t)e->max_batch + 1) + 8);
    a.cap_records = e->max_batch + 1;
    a.max_len = std::min(e->max_stride, e->p.max_cycles);
    HIP_TRY(e, fq_launch_raw_index(a, pe ? 2 : 1, e->max_batch, s.d_scan, s.scan_bytes, e->s_idx));
    HIP_TRY(e, hipMemcpyAsync(s.h_rstate, s.d_rstate, 2 * sizeof(fq_raw_state), hipMemcpyDeviceToHost, e->s_idx));
    HIP_TRY(e, hipEventRecord(s.ev_idx, e->s_idx));
    e->raw_queued.push_back(k);
    e->raw_prev_slot = k;
    return FQ_OK;
}

// the BGZF-window buffers of slot s: the members' table, and room for comp[m] bytes of each mate
static int ensure_bgzf(fq_engine* e, Slot& s, const uint64_t* comp) {
    if (!s.d_bdesc) {
        const size_t tab = (size_t)2 * FQ_RAW_BGZF_MEMBERS * sizeof(fq_raw_bgzf_desc);
        HIP_TRY(e, fq_inflate_spans_prepare());
        HIP_TRY(e, hipHostMalloc((void**)&s.h_bdesc, tab, hipHostMallocDefault));
        HIP_TRY(e, hipMalloc(&s.d_bdesc, tab));
        HIP_TRY(e, hipMalloc(&s.d_bctl, 4 * sizeof(uint32_t)));
        if (engine_timing()) {
            HIP_TRY(e, hipEventCreate(&s.ev_b0));
            HIP_TRY(e, hipEventCreate(&s.ev_b1));
        }
    }
    for (int m = 0; m < (e->p.paired ? 2 : 1); ++m) {
        if (comp[m] <= s.bcomp_cap[m]) continue;
        // (grown with some room, never beyond the window capacity, which bounds comp[m])
        const size_t cap = (size_t)std::min<uint64_t>(e->raw_wcap, std::max<uint64_t>(comp[m] + comp[m] / 4, 1u << 20));
        if (s.d_bcomp[m]) (void)hipFree(s.d_bcomp[m]);
        s.d_bcomp[m] = nullptr;
        s.bcomp_cap[m] = 0;
        HIP_TRY(e, hipMalloc(&s.d_bcomp[m], std::max<size_t>(cap, 16)));
        s.bcomp_cap[m] = cap;
    }
    return FQ_OK;
}

// FQ_BGZF_CLAIM=len (profiling): the members are claimed largest payload first, not in stream order
static bool bgzf_claim_by_len() {
    static const bool on = [] {
        const char* v = std::getenv("FQ_BGZF_CLAIM");
        return v && std::strcmp(v, "len") == 0;
    }();
    return on;
}

int fq_engine_raw_enqueue_bgzf(fq_engine* e, const fq_raw_bgzf_window* w) {
    if (!e || !w) return FQ_E_INVALID;
    if (!e->raw) return fail(e, FQ_E_INVALID, "fq_engine_raw_enqueue_bgzf before fq_engine_raw_begin");
    if (e->raw_queued.size() >= 3) return fail(e, FQ_E_INVALID, "three raw windows are already waiting for fq_engine_raw_launch");
    const bool pe = e->p.paired;
    const int mates = pe ? 2 : 1;
    if (e->raw_ccap < 65536) return fail(e, FQ_E_INVALID, "BGZF windows need a carry capacity of at least 65536 bytes");
    uint64_t n[2] = {0, 0}, comp[2] = {0, 0};
    for (int m = 0; m < mates; ++m) {
        if (w->members[m] > FQ_RAW_BGZF_MEMBERS) return fail(e, FQ_E_INVALID, "BGZF window: too many members");
        if (w->comp_bytes[m] > e->raw_wcap || (w->comp_bytes[m] && !w->comp[m]) || (w->members[m] && !w->m[m]))
            return fail(e, FQ_E_INVALID, "BGZF window: compressed bytes exceed the window capacity");
        if (w->skip[m] > e->raw_ccap) return fail(e, FQ_E_INVALID, "BGZF window: skip exceeds the carry capacity");
        uint64_t total = 0;
        for (uint32_t i = 0; i < w->members[m]; ++i) {
            const fq_inflate_member& mb = w->m[m][i];
            if (mb.in_len > FQ_INFLATE_MAX || mb.isize > FQ_INFLATE_MAX) return fail(e, FQ_E_INVALID, "BGZF window: member exceeds FQ_INFLATE_MAX");
            if (mb.in_off > w->comp_bytes[m] || mb.in_len > w->comp_bytes[m] - mb.in_off)
                return fail(e, FQ_E_INVALID, "BGZF window: a payload lies outside the compressed bytes");
            total += mb.isize;
        }
        if (w->n[m] > e->raw_wcap || total < (uint64_t)w->skip[m] + w->n[m] || total - w->skip[m] > e->raw_wcap)
            return fail(e, FQ_E_INVALID, "BGZF window: the members do not match skip and n, or exceed the window capacity");
        n[m] = w->n[m];
        comp[m] = w->comp_bytes[m];
    }
    HIP_TRY(e, hipSetDevice(e->device));
    const int k = (e->raw_prev_slot + 1) % kRawSlots;
    int rc = retire_slot(e, k);
    if (rc != FQ_OK) return rc;
    Slot& s = e->slots[k];
    if ((rc = alloc_slot(e, s)) != FQ_OK) return rc;
    if ((rc = ensure_raw(e, s)) != FQ_OK) return rc;
    if ((rc = ensure_bgzf(e, s, comp)) != FQ_OK) return rc;
    // the table in claim order: the mates interleaved in stream order (each mate's members in the
    // proportion of its count), so that both mates' outputs fill at the same rate
    uint32_t nd = 0;
    {
        uint32_t at[2] = {0, 0}, off[2] = {0, 0};
        const uint32_t c0 = w->members[0], c1 = pe ? w->members[1] : 0;
        while (at[0] < c0 || at[1] < c1) {
            // mate 1 goes next while it is behind mate 0 in its share of the members
            const int m = at[1] < c1 && (at[0] >= c0 || (uint64_t)at[1] * c0 < (uint64_t)at[0] * c1) ? 1 : 0;
            const fq_inflate_member& mb = w->m[m][at[m]++];
            fq_raw_bgzf_desc& d = s.h_bdesc[nd++];
            d.in_off = (uint32_t)mb.in_off;
            d.in_len = mb.in_len;
            d.isize = mb.isize;
            d.crc = mb.crc;
            d.out_off = off[m];
            d.mate = (uint32_t)m;
            d.pad[0] = d.pad[1] = 0;
            off[m] += mb.isize;
        }
        if (bgzf_claim_by_len())
            std::stable_sort(s.h_bdesc, s.h_bdesc + nd, [](const fq_raw_bgzf_desc& x, const fq_raw_bgzf_desc& y) { return x.in_len > y.in_len; });
    }
    {
        LinkChain& lc = link_chain(e->device);
        std::lock_guard<std::mutex> g(lc.m);
        if (lc.in && lc.in_owner != e) HIP_TRY(e, hipStreamWaitEvent(e->s_in, lc.in, 0));
        for (int m = 0; m < mates; ++m)
            if (comp[m]) HIP_TRY(e, hipMemcpyAsync(s.d_bcomp[m], w->comp[m], comp[m], hipMemcpyHostToDevice, e->s_in));
        if (nd) HIP_TRY(e, hipMemcpyAsync(s.d_bdesc, s.h_bdesc, (size_t)nd * sizeof(fq_raw_bgzf_desc), hipMemcpyHostToDevice, e->s_in));
        HIP_TRY(e, hipEventRecord(s.ev_in, e->s_in));
        lc.in = s.ev_in, lc.in_owner = e;
    }
    HIP_TRY(e, hipStreamWaitEvent(e->s_idx, s.ev_in, 0));
    HIP_TRY(e, hipMemsetAsync(s.d_bctl, 0, 4 * sizeof(uint32_t), e->s_idx));
    fq_inflate_spans a{};
    for (int m = 0; m < mates; ++m) {
        a.comp[m] = s.d_bcomp[m];
        a.out[m] = reinterpret_cast<uint8_t*>(s.d_text[m]) + e->raw_ccap - w->skip[m];
    }
    a.desc = s.d_bdesc;
    a.n = nd;
    a.ctl = s.d_bctl;
    s.b_timed = s.ev_b0 != nullptr;
    if (s.b_timed) HIP_TRY(e, hipEventRecord(s.ev_b0, e->s_idx));
    HIP_TRY(e, fq_launch_inflate_spans(a, e->cus, e->s_idx));
    if (s.b_timed) HIP_TRY(e, hipEventRecord(s.ev_b1, e->s_idx));
    return raw_index(e, k, n, s.d_bctl + 1);
}

// the oldest enqueued window's index, once its copy back has landed
static void raw_result_of(const fq_engine* e, const Slot& s, fq_raw_result* r) {
    const int mates = e->p.paired ? 2 : 1;
    std::memset(r, 0, sizeof *r);
    const int n = s.h_rstate[0].n;
    r->pairs = n;
    for (int m = 0; m < mates; ++m) {
        const fq_raw_state& st = s.h_rstate[m];
        // (after an overflow every byte of the carry and the window is still to be read)
        r->carry[m] = st.overflow ? (uint64_t)st.carry_in + s.raw_n[m] : (uint64_t)(st.avail - st.consumed);
        r->text_bytes[m] = st.consumed;
        r->max_len = std::max(r->max_len, st.max_len);
        if (st.overflow || st.first_bad == n) r->stop = 1;
    }
    for (int m = 0; m < mates; ++m)
        if (s.h_rstate[m].infl_bad) r->stop = FQ_RAW_STOP_INFLATE;
}

// FQ_ENGINE_TIMING: an indexed BGZF window's inflate, by the events around its launch (once)
static void report_inflate(Slot& s) {
    if (!s.b_timed) return;
    s.b_timed = false;
    float ms = 0;
    if (hipEventElapsedTime(&ms, s.ev_b0, s.ev_b1) == hipSuccess)
        std::fprintf(stderr, "fq_engine_raw: BGZF window of %llu + %llu bytes inflated in %.3f ms\n", (unsigned long long)s.raw_n[0],
                     (unsigned long long)s.raw_n[1], (double)ms);
}

int fq_engine_raw_wait(fq_engine* e, fq_raw_result* r) {
    if (!e) return FQ_E_INVALID;
    if (e->raw_queued.empty()) return fail(e, FQ_E_INVALID, "fq_engine_raw_wait without an enqueued window");
    HIP_TRY(e, hipSetDevice(e->device));
    Slot& s = e->slots[e->raw_queued.front()];
    HIP_TRY(e, hipEventSynchronize(s.ev_idx));
    if (r) raw_result_of(e, s, r);
    report_inflate(s);
    return FQ_OK;
}

int fq_engine_raw_launch(fq_engine* e, fq_raw_result* r, fq_raw_out* out, uint64_t seq_no) {
    if (!e || !r || !out) return FQ_E_INVALID;
    if (e->raw_queued.empty()) return fail(e, FQ_E_INVALID, "fq_engine_raw_launch without an enqueued window");
    if (e->gz_level && out->results) return fail(e, FQ_E_INVALID, "raw pack: records-only egress while gz output is on");
    // (its two streams cannot hold what -c and --discard_unmerged write: fq_engine_raw_launch_routed)
    if (e->p.correction_enabled || (e->p.merge_enabled && e->p.discard_unmerged) || e->umi_on)
        return fail(e, FQ_E_INVALID, "raw streams take no -c, UMI or --discard_unmerged options");
    if (e->phred64 && out->results) return fail(e, FQ_E_INVALID, "raw pack: records-only egress while --phred64 is on the device");
    if (e->cut_armed && out->results) return fail(e, FQ_E_INVALID, "raw pack: records-only egress takes no pack cuts");
    HIP_TRY(e, hipSetDevice(e->device));
    const int k = e->raw_queued.front();
    Slot& s = e->slots[k];
    HIP_TRY(e, hipEventSynchronize(s.ev_idx));  // (returns at once after fq_engine_raw_wait)
    report_inflate(s);
    const bool pe = e->p.paired;
    const int mates = pe ? 2 : 1;
    raw_result_of(e, s, r);
    const int n = r->pairs;
    // (a table below its bound is refused before the launch and leaves the window enqueued)
    int rc = check_cuts(e, std::max(n, 0));
    if (rc != FQ_OK) return rc;
    const bool cut = e->cut_armed;
    e->raw_queued.pop_front();
    out->text.bytes[0] = out->text.bytes[1] = 0;
    out->adapter_bytes[0] = out->adapter_bytes[1] = 0;
    if (n <= 0) {
        e->cut_armed = false;  // (no records: no pieces)
        e->pending.push_back(Pending{seq_no, -1, true, 0});
        return FQ_OK;
    }
    const bool recs_only = out->results != nullptr;  // (records-only egress: the caller formats)
    for (int m = 0; m < mates; ++m)
        if (recs_only ? !out->rec[m] : !out->text.text[m]) return fail(e, FQ_E_INVALID, "raw pack: missing output buffer");
    const size_t plane = fq_batch_bytes(e->max_batch, e->max_stride);
    fq_batch db{};
    db.n = n;
    db.stride = std::max(16, (r->max_len + 15) & ~15);
    db.seq1 = s.d_rows;
    db.qual1 = s.d_rows + plane;
    db.len1 = s.d_lens;
    db.seq2 = pe ? s.d_rows + 2 * plane : nullptr;
    db.qual2 = pe ? s.d_rows + 3 * plane : nullptr;
    db.len2 = pe ? s.d_lens + e->max_batch : nullptr;
    HIP_TRY(e, hipStreamWaitEvent(e->stream, s.ev_idx, 0));
    // (--phred64: only the taken records' quality lines; the carry, which the next window's index
    // copies from this text, lies behind them and is converted with the window that takes it)
    if ((rc = launch_ingest(e, s, n, db.stride, db)) != FQ_OK) return rc;
    for (int m = 0; m < mates; ++m)
        HIP_TRY(e, fq_launch_text_tiles(s.d_text[m], s.d_trec[m], n, db.stride, const_cast<uint8_t*>(m ? db.seq2 : db.seq1),
                                        const_cast<uint8_t*>(m ? db.qual2 : db.qual1), const_cast<uint16_t*>(m ? db.len2 : db.len1),
                                        e->stream));
    HIP_TRY(e, hipMemsetAsync(s.d_err, 0, sizeof(int), e->stream));
    if ((rc = launch(e, db, s.d_res, e->stream, s.scratch, false, false, seq_no, s.d_err)) != FQ_OK) return rc;
    HIP_TRY(e, hipMemsetAsync(s.d_total, 0, 4 * sizeof(unsigned long long), e->stream));
    if (recs_only) {  // the records and their line offsets back, no output text
        HIP_TRY(e, hipEventRecord(s.ev_kern, e->stream));
        HIP_TRY(e, hipStreamWaitEvent(e->s_out, s.ev_kern, 0));
        HIP_TRY(e, hipMemcpyAsync(out->results, s.d_res, (size_t)n * mates * sizeof(fq_read_result), hipMemcpyDeviceToHost,
                                  e->s_out));
        for (int m = 0; m < mates; ++m)
            HIP_TRY(e, hipMemcpyAsync(out->rec[m], s.d_trec[m], (size_t)n * sizeof(fq_text_rec), hipMemcpyDeviceToHost, e->s_out));
        HIP_TRY(e, hipMemcpyAsync(s.h_total, s.d_total, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->s_out));
        HIP_TRY(e, hipMemcpyAsync(s.h_err, s.d_err, sizeof(int), hipMemcpyDeviceToHost, e->s_out));
        HIP_TRY(e, hipEventRecord(s.ev_done, e->s_out));
        s.busy = true;
        s.text_out = &out->text;
        s.raw_out = out;
        e->pending.push_back(Pending{seq_no, k, false, 0});
        return FQ_OK;
    }
    // each mate's copy back: its output text (<= the input it spans) and the adapter entries after
    // it (per record, output + entry <= input + 3 bytes)
    // (-m: mate 0's output is the merged stream, mate 1's is empty: only its adapter entries)
    const bool mrg = pe && e->p.merge_enabled;
    size_t back[2] = {0, 0};
    for (int m = 0; m < mates; ++m) back[m] = (size_t)r->text_bytes[m] + kTextSlack + 3 * (size_t)n;
    if (mrg) back[0] = merged_cap(r->text_bytes[0], r->text_bytes[1], (size_t)n) + 3 * (size_t)n;
    if ((rc = launch_text_out(e, s, n)) != FQ_OK) return rc;
    // (the cut table before the adapter entries, which reuse the sizes' and offsets' buffers)
    if (cut) {
        uint32_t pieces = 0;
        if ((rc = launch_cuts(e, s, n, &pieces)) != FQ_OK) return rc;
        HIP_TRY(e, hipMemcpyAsync(e->cut_host, s.d_cuts, (size_t)pieces * sizeof(fq_cut), hipMemcpyDeviceToHost, e->stream));
        e->cut_armed = false;
    }
    // gz: each mate's text becomes BGZF members in place (d_total[m]: their bytes); the entries
    // follow them as they follow the text (members + entries <= the bound of text + entries)
    for (int m = 0; m < mates && e->gz_level; ++m) {
        if ((rc = launch_gz(e, s, m, back[m])) != FQ_OK) return rc;
        back[m] = fq_deflate_bound(back[m]);
    }
    for (int m = 0; m < mates; ++m) {
        if (e->p.adapter_trimming)
            HIP_TRY(e, fq_launch_raw_adapters(s.d_text[m], s.d_trec[m], s.d_res, n, pe ? 1 : 0, m, s.d_tsize[m], s.d_toff[m],
                                              s.d_scan, s.scan_bytes, s.d_out[m], s.d_total + m, back[m], s.d_total + 2 + m,
                                              e->stream));
    }
    // the output sizes (and the error word) behind the kernels; the text follows once they are in
    HIP_TRY(e, hipMemcpyAsync(s.h_total, s.d_total, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(s.h_err, s.d_err, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipEventRecord(s.ev_kern, e->stream));
    for (int m = 0; m < 2; ++m) {
        s.copy_dst[m] = m < mates ? out->text.text[m] : nullptr;
        s.copy_cap[m] = m < mates ? back[m] : 0;
    }
    s.copy_pending = true;
    s.busy = true;
    s.text_out = &out->text;
    s.raw_out = out;
    e->pending.push_back(Pending{seq_no, k, false, 0});
    return issue_copies(e, -1);
}

int fq_engine_raw_launch_routed(fq_engine* e, fq_raw_result* r, fq_raw_egress_out* out, uint64_t seq_no) {
    if (!e || !r || !out) return FQ_E_INVALID;
    if (!e->eg_on) return fail(e, FQ_E_INVALID, "routed raw pack without fq_engine_set_egress");
    if (e->raw_queued.empty()) return fail(e, FQ_E_INVALID, "fq_engine_raw_launch_routed without an enqueued window");
    if (e->cut_armed) return fail(e, FQ_E_INVALID, "routed raw packs take no pack cuts");
    HIP_TRY(e, hipSetDevice(e->device));
    const int k = e->raw_queued.front();
    Slot& s = e->slots[k];
    HIP_TRY(e, hipEventSynchronize(s.ev_idx));  // (returns at once after fq_engine_raw_wait)
    report_inflate(s);
    const bool pe = e->p.paired;
    const int mates = pe ? 2 : 1;
    raw_result_of(e, s, r);
    const int n = r->pairs;
    // every open stream (and, with -a, each mate's entries) needs a buffer of at least its bound; a
    // refusal leaves the window enqueued
    // (gz on: the bound of its BGZF stream)
    size_t bound[FQ_EG_STREAMS] = {};
    for (int q = 0; q < FQ_EG_STREAMS; ++q) {
        out->eg.bytes[q] = 0;
        if (!((e->eg_open >> q) & 1u) || n <= 0) continue;
        const size_t need = fq_egress_bound_umi(q, r->text_bytes[0], pe ? r->text_bytes[1] : 0, (uint64_t)n, umi_of(e));
        if (e->umi_on && need > 0xFFFFFFFFull) return fail(e, FQ_E_INVALID, "routed raw pack: a UMI-tagged stream's bound exceeds the 32-bit cursors (use smaller windows and max_batch)");
        if (!out->eg.text[q] || out->eg.cap[q] < out_alloc(e, need))
            return fail(e, FQ_E_INVALID, "routed raw pack: an open stream's buffer is missing or below fq_egress_bound");
        bound[q] = need;
    }
    for (int m = 0; m < 2; ++m) {
        out->adapter_bytes[m] = 0;
        if (m >= mates || n <= 0 || !e->p.adapter_trimming) continue;
        if (!out->adapters[m] || out->adapter_cap[m] < (size_t)r->text_bytes[m] + 3 * (size_t)n + kTextSlack)
            return fail(e, FQ_E_INVALID, "routed raw pack: an adapter-entry buffer is missing or too small");
    }
    e->raw_queued.pop_front();
    if (n <= 0) {
        e->pending.push_back(Pending{seq_no, -1, true, 0});
        return FQ_OK;
    }
    const size_t plane = fq_batch_bytes(e->max_batch, e->max_stride);
    fq_batch db{};
    db.n = n;
    db.stride = std::max(16, (r->max_len + 15) & ~15);
    db.seq1 = s.d_rows;
    db.qual1 = s.d_rows + plane;
    db.len1 = s.d_lens;
    db.seq2 = pe ? s.d_rows + 2 * plane : nullptr;
    db.qual2 = pe ? s.d_rows + 3 * plane : nullptr;
    db.len2 = pe ? s.d_lens + e->max_batch : nullptr;
    HIP_TRY(e, hipStreamWaitEvent(e->stream, s.ev_idx, 0));
    int rc = launch_ingest(e, s, n, db.stride, db);
    if (rc != FQ_OK) return rc;
    for (int m = 0; m < mates; ++m)
        HIP_TRY(e, fq_launch_text_tiles(s.d_text[m], s.d_trec[m], n, db.stride, const_cast<uint8_t*>(m ? db.seq2 : db.seq1),
                                        const_cast<uint8_t*>(m ? db.qual2 : db.qual1), const_cast<uint16_t*>(m ? db.len2 : db.len1),
                                        e->stream));
    HIP_TRY(e, hipMemsetAsync(s.d_err, 0, sizeof(int), e->stream));
    if ((rc = launch(e, db, s.d_res, e->stream, s.scratch, false, false, seq_no, s.d_err)) != FQ_OK) return rc;
    HIP_TRY(e, hipMemsetAsync(s.d_total, 0, 4 * sizeof(unsigned long long), e->stream));
    fq_egress_args a{};
    fq_egress_streams st{};
    const bool planes = pe && e->p.correction_enabled;
    for (int m = 0; m < mates; ++m) {
        a.text[m] = s.d_text[m];
        a.rec[m] = s.d_trec[m];
        a.seq[m] = planes ? (m ? db.seq2 : db.seq1) : nullptr;
        a.qual[m] = planes ? (m ? db.qual2 : db.qual1) : nullptr;
    }
    a.res = s.d_res;
    a.n = n, a.stride = db.stride, a.paired = pe ? 1 : 0;
    a.merge = pe && e->p.merge_enabled, a.discard = e->p.discard_unmerged;
    a.open = e->eg_open;
    a.umi = umi_of(e);
    for (int q = 0; q < FQ_EG_STREAMS; ++q) st.size[q] = s.d_egsize[q], st.off[q] = s.d_egoff[q], st.out[q] = s.d_eg[q];
    st.total = s.d_egtotal;
    HIP_TRY(e, fq_launch_egress(a, st, s.d_scan, s.scan_bytes, e->stream));
    if (e->gz_level && (rc = launch_gz_streams(e, s, bound)) != FQ_OK) return rc;
    // the trimmed-adapter entries per mate, uncompressed, into their own buffer (corrected pairs: the corrected bytes)
    for (int m = 0; m < mates && e->p.adapter_trimming; ++m)
        HIP_TRY(e, fq_launch_egress_adapters(a, m, s.d_tsize[m], s.d_toff[m], s.d_scan, s.scan_bytes, s.d_ad[m],
                                             (unsigned long long)s.ad_cap, s.d_total + 2 + m, e->stream));
    HIP_TRY(e, hipMemcpyAsync(s.h_egtotal, s.d_egtotal, FQ_EG_STREAMS * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                              e->stream));
    HIP_TRY(e, hipMemcpyAsync(s.h_total, s.d_total, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipMemcpyAsync(s.h_err, s.d_err, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipEventRecord(s.ev_kern, e->stream));
    s.copy_dst[0] = s.copy_dst[1] = nullptr;
    s.copy_cap[0] = s.copy_cap[1] = 0;
    s.copy_pending = true;
    s.busy = true;
    s.eg_out = &out->eg;
    s.reg_out = out;
    e->pending.push_back(Pending{seq_no, k, false, 0});
    return issue_copies(e, -1);
}

int fq_engine_raw_end(fq_engine* e) {
    if (!e) return FQ_E_INVALID;
    if (!e->raw) return FQ_OK;
    HIP_TRY(e, hipSetDevice(e->device));
    if (e->s_idx) HIP_TRY(e, hipStreamSynchronize(e->s_idx));  // (the index stream waits for the copies)
    e->raw_queued.clear();
    e->raw_prev_slot = -1;
    e->raw = false;
    return FQ_OK;
}

int fq_engine_set_gz_out(fq_engine* e, int32_t level) {
    if (!e) return FQ_E_INVALID;
    if (level < 0 || level > 9) return fail(e, FQ_E_INVALID, "fq_engine_set_gz_out: level must be 0 (off) or 1..9");
    if (!e->pending.empty() || !e->raw_queued.empty())
        return fail(e, FQ_E_INVALID, "fq_engine_set_gz_out with packs in flight");
    if (level && e->cut_every) return fail(e, FQ_E_INVALID, "fq_engine_set_gz_out: no device BGZF output while pack cuts are on");
    if ((level != 0) != (e->gz_level != 0)) {
        // the output buffers are sized for the stream's bound while gz is on: re-made on next use
        for (Slot& s : e->slots) {
            s.text_cap[0] = s.text_cap[1] = 0;
            for (int k = 0; k < FQ_EG_STREAMS; ++k) s.eg_cap[k] = 0;  // (ensure_egress_caps re-makes the streams' buffers)
            s.raw_ready = false;
        }
        if (!level) {
            HIP_TRY(e, hipSetDevice(e->device));
            HIP_TRY(e, hipDeviceSynchronize());
            fq_deflate_scratch_free(e->gz);
        }
    }
    e->gz_level = level;
    return FQ_OK;
}

int fq_host_register(const void* p, size_t bytes) {
    if (!p || !bytes) return FQ_E_INVALID;
    return hipHostRegister(const_cast<void*>(p), bytes, hipHostRegisterReadOnly) == hipSuccess ? FQ_OK : FQ_E_HIP;
}

int fq_host_unregister(const void* p) {
    if (!p) return FQ_E_INVALID;
    return hipHostUnregister(const_cast<void*>(p)) == hipSuccess ? FQ_OK : FQ_E_HIP;
}

int fq_engine_poll(fq_engine* e, int wait, uint64_t* seq_no) {
    if (!e) return FQ_E_INVALID;
    if (e->pending.empty()) return 0;
    HIP_TRY(e, hipSetDevice(e->device));
    int rc0 = issue_copies(e, -1);  // (raw packs whose sizes are in: their copies back start now)
    if (rc0 != FQ_OK) return rc0;
    Pending& q = e->pending.front();
    if (!q.done) {
        Slot& s = e->slots[q.slot];
        if (s.copy_pending && !wait) return 0;
        if (!wait) {
            const hipError_t st = hipEventQuery(s.ev_done);
            if (st == hipErrorNotReady) return 0;
            if (st != hipSuccess) return hip_fail(e, st, "hipEventQuery");
        }
        int rc = retire_slot(e, q.slot);
        if (rc != FQ_OK) return rc;
    }
    const Pending done = q;
    e->pending.pop_front();
    if (seq_no) *seq_no = done.seq_no;
    if (done.err & 2) return fail(e, FQ_E_INVALID, "device BGZF: the pack's members exceed the compressor's scratch");
    if (done.err) return fail(e, FQ_E_TOO_LONG, "a read is longer than max_cycles or the row stride");
    return 1;
}

int fq_engine_pending(const fq_engine* e) { return e ? (int)e->pending.size() : FQ_E_INVALID; }

int fq_engine_process(fq_engine* e, const fq_batch* hb, fq_read_result* results) {
    if (!e || !hb || !results) return FQ_E_INVALID;
    if (!e->pending.empty()) return fail(e, FQ_E_INVALID, "fq_engine_process with submitted packs not yet polled");
    int rc = fq_engine_submit(e, hb, results, 0);
    if (rc != FQ_OK) return rc;
    rc = fq_engine_poll(e, 1, nullptr);
    return rc == 1 ? FQ_OK : rc;
}

int fq_engine_process_device(fq_engine* e, const fq_batch* db, fq_read_result* dres, void* stream) {
    if (!e || !db) return FQ_E_INVALID;
    if (db->n < 0 || db->stride <= 0 || (db->stride & 15) || !db->seq1 || !db->qual1 || !db->len1 ||
        (e->p.paired && (!db->seq2 || !db->qual2 || !db->len2)))
        return fail(e, FQ_E_INVALID, "bad device batch");
    if (e->p.correction_enabled && db->stride > 32768)
        return fail(e, FQ_E_INVALID, "-c takes reads of at most 32767 bases (the record's overlap offset is 16-bit)");
    HIP_TRY(e, hipSetDevice(e->device));
    // NULL is the HIP default stream
    return launch(e, *db, dres, (hipStream_t)stream, e->scratch, true, true, e->calls++, e->err);
}

size_t fq_engine_acc_words(const fq_engine* e) { return e ? e->acc_words : 0; }

int fq_engine_set_dup(fq_engine* e, fq_dup* d) {
    if (!e) return FQ_E_INVALID;
    if (d) {
        int dev = -1;
        if (fq_dup_device(d, &dev) != FQ_OK || dev != e->device)
            return fail(e, FQ_E_INVALID, "the duplication table is on another device");
    }
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipDeviceSynchronize());  // packs in flight finish with the old table
    e->dup = d;
    return FQ_OK;
}

int fq_engine_set_kstat(fq_engine* e, fq_kstat* h) {
    if (!e) return FQ_E_INVALID;
    if (h) {
        int dev = -1;
        if (fq_kstat_device(h, &dev) != FQ_OK || dev != e->device)
            return fail(e, FQ_E_INVALID, "the k-mer tables are on another device");
    }
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipDeviceSynchronize());  // packs in flight finish with the old tables
    e->kstat = h;
    return FQ_OK;
}

int fq_engine_set_ora(fq_engine* e, fq_ora* h) {
    if (!e) return FQ_E_INVALID;
    if (h) {
        int dev = -1;
        if (fq_ora_device(h, &dev) != FQ_OK || dev != e->device)
            return fail(e, FQ_E_INVALID, "the overrepresented-sequence counts are on another device");
    }
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipDeviceSynchronize());  // packs in flight finish with the old handle
    e->ora = h;
    return FQ_OK;
}

int fq_engine_acc_device_ptr(fq_engine* e, uint64_t** dptr) {
    if (!e || !dptr) return FQ_E_INVALID;
    *dptr = reinterpret_cast<uint64_t*>(e->acc);
    return FQ_OK;
}

int fq_engine_read_acc(fq_engine* e, uint64_t* host, size_t words) {
    if (!e || !host || words < e->acc_words) return FQ_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipDeviceSynchronize());
    HIP_TRY(e, hipMemcpy(host, e->acc, e->acc_words * 8, hipMemcpyDeviceToHost));
    return check_err(e);
}

int fq_engine_set_acc_buffer(fq_engine* e, uint64_t* device_acc) {
    if (!e) return FQ_E_INVALID;
    e->acc = device_acc ? reinterpret_cast<unsigned long long*>(device_acc) : e->own_acc;
    return FQ_OK;
}

int fq_engine_reset_acc(fq_engine* e) {
    if (!e) return FQ_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->device));
    HIP_TRY(e, hipMemsetAsync(e->acc, 0, e->acc_words * 8, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return FQ_OK;
}

int fq_engine_sync(fq_engine* e) {
    if (!e) return FQ_E_INVALID;
    HIP_TRY(e, hipSetDevice(e->device));
    const int rc = issue_copies(e, -2);  // (the copies back of every raw pack launched)
    if (rc != FQ_OK) return rc;
    HIP_TRY(e, hipDeviceSynchronize());
    return check_err(e);
}

const char* fq_engine_last_error(const fq_engine* e) { return e ? e->last_error.c_str() : g_create_error.c_str(); }

int fq_engine_device_info(const fq_engine* e, int* device, char* arch, size_t arch_len) {
    if (!e) return FQ_E_INVALID;
    if (device) *device = e->device;
    if (arch && arch_len) std::snprintf(arch, arch_len, "%s", e->arch);
    return FQ_OK;
}

// Page-locked host memory as anonymous transparent-huge-page memory, populated, then registered
// with every device (portable): 0.06 s per GiB to set up and 0.04 s to release, against 0.23 s
// and 0.13 s for hipHostMalloc (tools/micro/h2d.hip on MI355X), and DMA at the same 57 GB/s.
// The mapping length of each block is kept for fq_host_free; hipHostMalloc is the fallback.
namespace {
std::mutex g_host_mu;
std::unordered_map<void*, size_t> g_host_maps;  // registered anonymous mappings -> length
}  // namespace

int fq_host_alloc(size_t bytes, void** out) {
    if (!out) return FQ_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FQ_E_NO_DEVICE;
    const size_t huge = (size_t)2 << 20;
    const size_t len = ((bytes ? bytes : 1) + huge - 1) / huge * huge;
    void* m = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m != MAP_FAILED) {
        (void)madvise(m, len, MADV_HUGEPAGE);
        std::memset(m, 0, len);  // populate (registration pins what is there)
        if (hipHostRegister(m, len, hipHostRegisterPortable) == hipSuccess) {
            std::lock_guard<std::mutex> g(g_host_mu);
            g_host_maps[m] = len;
            *out = m;
            return FQ_OK;
        }
        munmap(m, len);
    }
    if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) {
        *out = nullptr;
        return FQ_E_NOMEM;
    }
    return FQ_OK;
}

int fq_host_free(void* p) {
    if (!p) return FQ_OK;
    size_t len = 0;
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        auto it = g_host_maps.find(p);
        if (it != g_host_maps.end()) {
            len = it->second;
            g_host_maps.erase(it);
        }
    }
    if (len) {
        const bool ok = hipHostUnregister(p) == hipSuccess;
        munmap(p, len);
        return ok ? FQ_OK : FQ_E_HIP;
    }
    return hipHostFree(p) == hipSuccess ? FQ_OK : FQ_E_HIP;
}

int fq_synth_fill_device(const fq_batch* db, uint64_t seed, uint64_t first_index, int32_t read_len, void* stream) {
    if (!db || read_len <= 0 || read_len > db->stride || !db->seq1 || !db->qual1 || !db->len1)
        return FQ_E_INVALID;
    hipError_t he = fq_launch_synth(*db, seed, first_index, read_len, (hipStream_t)stream);
    return he == hipSuccess ? FQ_OK : FQ_E_HIP;
}

double fq_engine_last_kernel_ms(const fq_engine* e) {
    if (!e || !e->timed) return 0.0;
    float ms = 0.f;
    if (hipEventSynchronize(e->ev1) != hipSuccess) return 0.0;
    if (hipEventElapsedTime(&ms, e->ev0, e->ev1) != hipSuccess) return 0.0;
    return ms;
}

}  // extern "C"
