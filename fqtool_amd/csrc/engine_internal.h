// engine_internal.h -- launch entry points shared between the engine's translation units.
#pragma once

// largest fq_params.max_cycles an engine accepts (reads beyond it fail the pack with FQ_E_TOO_LONG)
#define FQ_MAX_CYCLES_LIMIT 4096

#include <hip/hip_runtime.h>

#include "../../include/fqengine.h"

// General kernel workgroup: 8 waves (one LDS histogram copy per workgroup, 2 workgroups per CU
// at <= 160 cycles: 16 waves per CU; it uses ~70 VGPRs, so registers allow more)
constexpr int kPackThreads = 512;
size_t fq_pack_kernel_lds_bytes(const fq_params& p);
hipError_t fq_pack_kernel_set_lds(const fq_params& p);
// General kernel (any bytes, any length <= max_cycles, merge): all pairs, or only the pairs
// (single-end: reads) whose indices are listed in tiles[0 .. *ntiles) when tiles != nullptr.
hipError_t fq_launch_pack_kernel(const fq_params& p, const fq_batch& b, fq_read_result* res, unsigned long long* acc,
                                 int* err, int grid, hipStream_t stream, const int* tiles = nullptr,
                                 const int* ntiles = nullptr);
// Fast kernels (pe_fast.hip); the indices of pairs / reads they cannot take are appended to
// slow_tiles (room for one per pair / read).
bool fq_pe_fast_supported(const fq_params& p);
hipError_t fq_pe_fast_prepare();
hipError_t fq_launch_pe_fast(const fq_params& p, const fq_batch& b, fq_read_result* res, unsigned long long* acc,
                             int* slow_tiles, int* slow_count, int* tile_ctr, unsigned long long* xfix, int grid,
                             hipStream_t stream);
// the fast kernels' exotic-byte Stats moves: a zeroed buffer of fq_xfix_words(max_cycles) words per
// engine, folded into the accumulator's Stats blocks (acc_stats: their first word) after each launch
size_t fq_xfix_words(int32_t max_cycles);
hipError_t fq_launch_xfix_fold(unsigned long long* acc_stats, unsigned long long* xfix, int32_t max_cycles, hipStream_t s);
// the same kernels built for rows of up to 320 bytes (pe_fast_long.hip; fq_launch_pe_fast
// forwards batches with stride > 160 to it, except -m)
hipError_t fq_pe_fast_long_prepare();
hipError_t fq_launch_pe_fast_long(const fq_params& p, const fq_batch& b, fq_read_result* res, unsigned long long* acc,
                                  int* slow_tiles, int* slow_count, int* tile_ctr, unsigned long long* xfix, int grid,
                                  hipStream_t stream);
hipError_t fq_launch_synth(const fq_batch& b, uint64_t seed, uint64_t first_index, int read_len, hipStream_t stream);
// Duplication analysis of one pack into a table (dup.hip); order_base orders the pack's reads
// against other packs (the pack's sequence number).
int fq_dup_pack(fq_dup* d, const fq_batch& b, int paired, unsigned long long order_base, hipStream_t s);
const char* fq_dup_error(const fq_dup* d);
int fq_dup_device(const fq_dup* d, int* device);
// k-mer statistics of one pack (kstat.hip): the pre pass reads the original planes, so it goes
// before the main kernels (-c rewrites the planes in place); the post pass reads the records, so
// it goes after the last kernel that writes them.  fq_kstat_records lends a record buffer of n
// entries to a pack whose caller wants no records.
int fq_kstat_pre(fq_kstat* h, const fq_batch& b, const fq_params& p, hipStream_t s);
int fq_kstat_post(fq_kstat* h, const fq_batch& b, const fq_params& p, const fq_read_result* res, hipStream_t s);
int fq_kstat_records(fq_kstat* h, size_t n, hipStream_t s, fq_read_result** out);
const char* fq_kstat_error(const fq_kstat* h);
int fq_kstat_device(const fq_kstat* h, int* device);
// overrepresented sequences of one pack (ora.hip): two passes placed like the k-mer ones, and a
// record buffer lent likewise
int fq_ora_pre(fq_ora* h, const fq_batch& b, const fq_params& p, hipStream_t s);
int fq_ora_post(fq_ora* h, const fq_batch& b, const fq_params& p, const fq_read_result* res, hipStream_t s);
int fq_ora_records(fq_ora* h, size_t n, hipStream_t s, fq_read_result** out);
const char* fq_ora_error(const fq_ora* h);
int fq_ora_device(const fq_ora* h, int* device);
// FASTQ-text packs (text.hip): tile planes built from the text; output text of the passing records
hipError_t fq_launch_text_tiles(const char* d_text, const fq_text_rec* d_rec, int n, int stride, uint8_t* seq,
                                uint8_t* qual, uint16_t* lens, hipStream_t s);
size_t fq_text_scan_temp_bytes(int n);
hipError_t fq_launch_text_out(const char* d_text, const fq_text_rec* d_rec, const fq_read_result* d_res, int n, int paired,
                              int m, uint32_t* d_size, uint32_t* d_off, void* d_temp, size_t temp_bytes, char* d_out,
                              unsigned long long* d_total, hipStream_t s);
// -m: the merged output stream of a PE text pack (text.hip), into d_out (mate 0's output)
hipError_t fq_launch_merge_out(const char* d_text1, const char* d_text2, const fq_text_rec* d_rec1,
                               const fq_text_rec* d_rec2, const fq_read_result* d_res, int n, int discard,
                               uint32_t* d_size, uint32_t* d_off, void* d_temp, size_t temp_bytes, char* d_out,
                               unsigned long long* d_total, hipStream_t s);
// Routed egress of a text pack (text.hip, the per-pair routine of egress_core.h): every open stream's
// output text, st.total[s] = its bytes (0 for a stream that is not open)
struct fq_egress_args {
    const char* text[2];
    const fq_text_rec* rec[2];
    const fq_read_result* res;
    const uint8_t* seq[2];   // the tile planes when -c ran (corrected pairs are read from them), else null
    const uint8_t* qual[2];
    int n, stride, paired, merge, discard;
    uint32_t open;
    const fq_umi* umi;       // the UMI description (fq_engine_set_umi), or null
};
struct fq_egress_streams {
    uint32_t* size[FQ_EG_STREAMS];  // n each, open streams only
    uint32_t* off[FQ_EG_STREAMS];
    char* out[FQ_EG_STREAMS];
    unsigned long long* total;      // [FQ_EG_STREAMS]
};
hipError_t fq_launch_egress(const fq_egress_args& a, const fq_egress_streams& st, void* d_temp, size_t temp_bytes,
                            hipStream_t s);
// trimmed-adapter entries of mate m of a routed raw pack (the format of fq_launch_raw_adapters), from
// d_out's start; a corrected pair's bytes come from the planes.  *d_total = their bytes, ~0 (nothing
// written) if they exceed cap
hipError_t fq_launch_egress_adapters(const fq_egress_args& a, int m, uint32_t* d_size, uint32_t* d_off, void* d_temp,
                                     size_t temp_bytes, char* d_out, unsigned long long cap, unsigned long long* d_total,
                                     hipStream_t s);
// Device ingest (ingest.hip).  The index filter's lists as the engine keeps them on the device: one
// blob of whole 32-bit words, off1[n1 + 1] | off2[n2 + 1] | list 1's bytes | list 2's bytes
struct fq_index_lists {
    const uint32_t* blob;
    uint32_t blob_bytes;
    uint32_t n1, n2;
    uint32_t len1;  // list 1's bytes (list 2's follow them)
    int threshold;
};
// the pack's per-record FQ_BF_* flags (d_text2 / d_rec2 null: single end)
hipError_t fq_launch_index_flags(const fq_index_lists& f, const char* d_text1, const fq_text_rec* d_rec1, const char* d_text2,
                                 const fq_text_rec* d_rec2, int n, uint8_t* d_flags, hipStream_t s);
// --phred64: the records' quality lines rewritten in place (stride: the pack's, >= every record's length)
hipError_t fq_launch_phred64(char* d_text, const fq_text_rec* d_rec, int n, int stride, hipStream_t s);
// the cut table of a pack's plain pair egress, from fq_launch_text_out's sizes and offsets of each
// mate (d_size1 / d_off1 null: single end)
hipError_t fq_launch_cuts(const uint32_t* d_size0, const uint32_t* d_off0, const uint32_t* d_size1, const uint32_t* d_off1, int n,
                          uint64_t every, uint64_t first, uint32_t pieces, fq_cut* d_cuts, hipStream_t s);
// Device BGZF (deflate.hip): scratch of the compressor, shared by the launches of one stream (they
// run one after another): a token array per resident workgroup, a 64 KiB slot and a size per member
struct fq_deflate_scratch {
    uint32_t* tok = nullptr;
    uint8_t* slots = nullptr;
    uint32_t* sizes = nullptr;
    unsigned long long* total = nullptr;  // [FQ_EG_STREAMS]
    size_t members = 0;  // members the slots hold
    int grid = 0;        // workgroups the token arrays serve
    int cus = 0;
};
// grows the scratch to texts of max_bytes (freeing the old buffers waits for the device)
hipError_t fq_deflate_scratch_ensure(fq_deflate_scratch& sc, size_t max_bytes, int cus);
void fq_deflate_scratch_free(fq_deflate_scratch& sc);
// d_text[0, min(*d_n, cap_bytes)) -> BGZF members at d_dst (which may be d_text: the members are
// compacted only after all are compressed), their bytes to *d_total (which may be d_n)
hipError_t fq_launch_deflate(const fq_deflate_scratch& sc, const void* d_text, const unsigned long long* d_n, size_t cap_bytes,
                             int level, void* d_dst, size_t dst_cap, unsigned long long* d_total, hipStream_t s);
// The same for up to FQ_EG_STREAMS texts of one pack by one pair of launches (a routed pack's
// streams, whose real sizes only the device knows): spans[k] with d_n null is not there.  Each text
// becomes its members in place (its buffer holds fq_deflate_bound(cap_bytes)), d_totals[k] = their
// bytes, 0 for an empty or absent span; d_totals may be the array the d_n point into.  The members of
// all spans share the scratch: should they exceed sc.members, nothing is compacted, every total is 0
// and bit 1 of *d_err is set (d_err may be null).
struct fq_deflate_span {
    void* d_text;
    const unsigned long long* d_n;
    size_t cap_bytes;
};
hipError_t fq_launch_deflate_spans(const fq_deflate_scratch& sc, const fq_deflate_span* spans, int level,
                                   unsigned long long* d_totals, int* d_err, hipStream_t s);
// Raw FASTQ streams (raw.hip): per (window, mate) device state of the record indexing
struct fq_raw_state {
    uint32_t text_start;  // buffer offset of the window's text (the carried bytes first)
    uint32_t carry_in;    // bytes carried over from the previous window
    uint32_t avail;       // carry_in + the window's raw bytes
    uint32_t overflow;    // the carry did not fit (nothing is indexed)
    int32_t first_bad;    // lowest index of a complete record that is not plain (INT_MAX: none)
    int32_t complete;     // records whose four lines are in the text (capped by the record capacity)
    int32_t max_len;      // longest sequence of the plain records
    uint32_t total_lines;
    uint32_t consumed;    // text bytes taken by the pack's records
    int32_t n;            // records (pairs) of the pack
    uint32_t infl_bad;    // members of this or an earlier BGZF window that did not inflate (overflow is set)
    uint32_t pad;
};
struct fq_raw_text_args {
    char* text[2];
    const char* prev_text[2];
    const fq_raw_state* prev_state;  // previous window's states, nullptr at the start of the stream
    fq_raw_state* state;             // [2]
    uint32_t raw_bytes[2];
    const uint32_t* infl_bad;        // [2]: a BGZF window's members that did not inflate, nullptr for a plain window
    uint32_t carry_cap;              // the raw bytes land at this buffer offset
    uint32_t nblocks;                // 4 KiB blocks of the buffer
    uint32_t* bcnt[2];
    uint32_t* bbase[2];
    uint32_t* lines[2];
    uint32_t cap_lines;
    int cap_records;
    fq_text_rec* rec[2];
    int max_len;                     // longest sequence the engine takes (longer: not plain)
};
size_t fq_raw_scan_temp_bytes(int nblocks, int n);
hipError_t fq_launch_raw_index(const fq_raw_text_args& a, int mates, int cap_batch, void* d_temp, size_t temp_bytes,
                               hipStream_t s);
// BGZF windows of the raw stream (inflate.hip): one launch inflates both mates' members.  The table
// is in claim order: the waves take its entries one after another from ctl[0], and count the members
// of mate m that are not FQ_INFL_OK in ctl[1 + m] (all three cleared on the stream before the launch).
struct fq_raw_bgzf_desc {
    uint32_t in_off;   // the payload's offset in comp[mate]
    uint32_t in_len;
    uint32_t isize;
    uint32_t crc;
    uint32_t out_off;  // the member's offset in out[mate]
    uint32_t mate;
    uint32_t pad[2];
};
struct fq_inflate_spans {
    const uint8_t* comp[2];
    uint8_t* out[2];
    const fq_raw_bgzf_desc* desc;
    uint32_t n;
    uint32_t* ctl;  // [3]
};
hipError_t fq_inflate_spans_prepare();
hipError_t fq_launch_inflate_spans(const fq_inflate_spans& a, int cus, hipStream_t s);
// trimmed-adapter entries of mate m appended to its output text (at *d_text_total, within cap bytes
// of d_out; *d_total = the entries' bytes, ~0 if they would not fit)
hipError_t fq_launch_raw_adapters(const char* d_text, const fq_text_rec* d_rec, const fq_read_result* d_res, int n,
                                  int paired, int m, uint32_t* d_size, uint32_t* d_off, void* d_temp, size_t temp_bytes,
                                  char* d_out, const unsigned long long* d_text_total, unsigned long long cap,
                                  unsigned long long* d_total, hipStream_t s);
