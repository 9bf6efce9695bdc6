/*
 * fqengine.h -- C-ABI drop-in boundary of the MI355X FASTQ preprocessing engine.
 *
 * The reference (Wsc000123/fqtool, a fastp fork) has no plugin/FFI API; its hot path is the
 * per-pack worker call
 *     bool PairEndProcessor::processPairEnd(ReadPairPack*, ThreadConfig*)
 *         (reference src/peprocessor.h:61, body src/peprocessor.cpp:261-508)
 *     void SingleEndProcessor::processSingleEnd(ReadPack*, ThreadConfig*)
 *         (reference src/seprocessor.cpp:290-388)
 * which mutates the reads of one pack in place and accumulates into the worker's
 * ThreadConfig (Stats x4 + FilterResult, src/threadconfig.cpp:3-20) and the processor's
 * insert-size histogram (src/peprocessor.cpp:510-523).
 *
 * This header replaces that seam with plain pointers and sizes (no C++ / torch types):
 *   - fq_params       : POD snapshot of every derived Options field the loop body reads
 *                        (src/options.h:15-386 after Options::update, src/options.cpp:24-58)
 *   - fq_batch        : one pack of reads as SoA uint8 seq/qual planes (chunk-interleaved
 *                        tiles, see below) + uint16 lengths
 *                        (replaces ReadPairPack / ReadPack, src/peprocessor.h:28-31)
 *   - fq_read_result  : per-read trim window + filter code + adapter/merge descriptors, i.e.
 *                        everything the in-place std::string mutations of the loop body produce
 *   - accumulator     : flat uint64 block = Stats x4 + FilterResult counters + insert histogram,
 *                        sum-reducible (RCCL ncclSum/ncclUint64 across GPUs)
 * Every entry point returns 0 on success and a negative FQ_E* code on failure; nothing
 * throws across the ABI. The engine never falls back to a CPU path: without a usable gfx950
 * device fq_engine_create fails with FQ_E_NO_DEVICE.
 */
#ifndef FQENGINE_H
#define FQENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FQ_ABI_VERSION 3

/* ---- status codes ------------------------------------------------------------------- */
#define FQ_OK 0
#define FQ_E_INVALID (-1)    /* bad argument / unsupported parameter combination           */
#define FQ_E_NO_DEVICE (-2)  /* no HIP device, or not gfx950                                */
#define FQ_E_HIP (-3)        /* a HIP runtime call failed (message in fq_engine_last_error)  */
#define FQ_E_TOO_LONG (-4)   /* a read is longer than the engine's configured max_cycles     */
#define FQ_E_NOMEM (-5)

/* ---- filter result codes: reference src/common.h:9-30 -------------------------------- */
#define FQ_PASS_FILTER 0
#define FQ_FAIL_POLY_X 4
#define FQ_FAIL_OVERLAP 8
#define FQ_FAIL_N_BASE 12
#define FQ_FAIL_LENGTH 16
#define FQ_FAIL_TOO_LONG 17
#define FQ_FAIL_QUALITY 20
#define FQ_FAIL_COMPLEXITY 24
#define FQ_FILTER_RESULT_TYPES 32

#define FQ_MAX_ADAPTER 128 /* longest --adapter_of_read{1,2} accepted                       */

/*
 * Derived options, already in the form the reference's loop body consumes them.
 * The host (fqtool_amd/host/options.cpp) fills this exactly as Options::update does,
 * including the reference quirks:
 *   - low_qual_limit already has +33 added (src/options.cpp:26),
 *   - low_qual_base_limit = int(lowQualityRatio * 151) (src/options.cpp:44 runs before the
 *     read-length evaluation, src/main.cpp:124-129),
 *   - polyg_* are the EFFECTIVE (compareReq, maxMismatch, oneMismatchPer) triple: the PE call
 *     at src/peprocessor.cpp:297 passes (maxMismatch, allowedOneMismatchForEach, minLen) into
 *     PolyX::trimPolyG(r1, r2, compareReq, maxMismatch, allowedOneMismatchForEach, fr)
 *     (src/polyx.h:28), the SE call at src/seprocessor.cpp:317 passes them in order.
 */
typedef struct fq_params {
    int32_t paired; /* 1 = PairEndProcessor, 0 = SingleEndProcessor */

    /* Filter::trimAndCut, src/filter.cpp:69-189 */
    int32_t trim_front1, trim_tail1, trim_front2, trim_tail2; /* -f -t -F -T */
    int32_t cut_front, cut_right, cut_tail;                   /* enable flags */
    int32_t cut_front_window, cut_right_window, cut_tail_window;
    int32_t cut_front_quality, cut_right_quality, cut_tail_quality; /* mean quality, no +33 */

    /* PolyX::trimPolyG, src/polyx.cpp:14-38 (effective argument order, see above) */
    int32_t polyg_enabled;
    int32_t polyg_compare_req, polyg_max_mismatch, polyg_one_mismatch_per;

    /* PolyX::trimPolyX, src/polyx.cpp:45-101 */
    int32_t polyx_enabled;
    int32_t polyx_mask; /* bit b set <=> base "ATCGN"[b] is in --base_to_trim */
    int32_t polyx_compare_req, polyx_max_mismatch, polyx_one_mismatch_per;

    /* adapters: src/peprocessor.cpp:301-326, src/seprocessor.cpp:321-323 */
    int32_t adapter_trimming; /* -a */
    int32_t adapter1_len, adapter2_len; /* 0 = not provided (adapterSeqR{1,2}Provided) */
    uint8_t adapter1[FQ_MAX_ADAPTER];
    uint8_t adapter2[FQ_MAX_ADAPTER];

    /* OverlapAnalysis::analyze, src/overlapanalysis.cpp:7-72 */
    int32_t overlap_diff_limit; /* --max_diff_for_overlap, default 5 */
    int32_t overlap_require;    /* --min_overlap_len, default 30 */
    int32_t insert_size_max;    /* 512, src/options.cpp:17 */

    /* -b / -B, src/peprocessor.cpp:342-349 */
    int32_t max_len1, max_len2;

    /* -m, src/peprocessor.cpp:351-385 */
    int32_t merge_enabled, discard_unmerged;

    /* Filter::passFilter, src/filter.cpp:3-52 */
    int32_t qual_filter_enabled;
    int32_t low_qual_limit;      /* -Q + 33 */
    int32_t low_qual_base_limit; /* int(-U * 151) */
    int32_t n_base_limit;        /* -N */
    double avg_qual_limit;       /* -e */
    int32_t length_filter_enabled, min_len, max_len; /* -l --min_length --max_length */
    int32_t complexity_enabled;  /* -y */
    double complexity_threshold; /* -Y */

    /* engine sizing */
    int32_t max_cycles; /* per-cycle Stats buffer length; reads longer than this are rejected */

    /* -c: BaseCorrector::correctByOverlapAnalysis (src/basecorrector.cpp:14-70), PE only, run
     * between the insert-size statistics and adapter trimming (src/peprocessor.cpp:310-312).
     * The engine corrects the bases/qualities of the DEVICE batch planes in place. */
    int32_t correction_enabled;
    /* -u with the UMI in the read (UmiProcessor::process, src/umiprocessor.cpp:10-79): after the
     * pre-filter statistics each mate loses min(umi_front, len - 1) leading bases
     * (Read::trimFront, src/read.h:203-208); 0 = no UMI trim.  The UMI tag itself only changes
     * the read names and is the host's business. */
    int32_t umi_front1, umi_front2;
    int32_t reserved[4];
} fq_params;

/* One pack of reads.  Each plane (seq1, qual1, seq2, qual2) holds every read's row of `stride`
 * bytes in CHUNK-INTERLEAVED TILES: reads are grouped in tiles of FQ_TILE_READS consecutive reads,
 * and inside a tile the 16-byte chunk k of all its reads is stored together, so
 *     byte j of read i  is at  plane[fq_batch_offset(stride, i, j)]
 *                          =  (i / 32) * 32 * stride + (j / 16) * 512 + (i % 32) * 16 + j % 16.
 * One wave-wide load of chunk k of 32 (or 64) reads is then one (or two) 512-byte contiguous runs
 * instead of 64 rows touched 16 bytes at a time.  A plane spans fq_batch_bytes(n, stride) bytes
 * (whole tiles; the padding rows are never read as reads).  Bytes j >= len[i] of a row are
 * ignored.  Packers: fq_batch_offset / fq_batch_put_row below. */
#define FQ_TILE_READS 32
#define FQ_CHUNK 16
typedef struct fq_batch {
    int32_t n;      /* number of pairs (PE) or reads (SE) */
    int32_t stride; /* bytes per row, multiple of 16, >= every len */
    const uint8_t* seq1;
    const uint8_t* qual1;
    const uint16_t* len1;
    const uint8_t* seq2; /* PE only, else NULL */
    const uint8_t* qual2;
    const uint16_t* len2;
    /* optional per-pair (per-read in SE) FQ_BF_* flags, n bytes; NULL = all zero */
    const uint8_t* flags;
} fq_batch;

/* fq_batch.flags: the pair (read) was dropped by Filter::filterByIndex
 * (src/filter.cpp:209-232, called at src/peprocessor.cpp:283 / src/seprocessor.cpp:304): only the
 * pre-filter statistics count it, its record carries FQ_RF_INDEX_FILTERED and nothing else. */
#define FQ_BF_INDEX_FILTERED 0x01

static inline size_t fq_batch_offset(int32_t stride, int64_t i, int32_t j) {
    return (size_t)(i / FQ_TILE_READS) * FQ_TILE_READS * (size_t)stride +
           (size_t)(j / FQ_CHUNK) * (FQ_TILE_READS * FQ_CHUNK) + (size_t)(i % FQ_TILE_READS) * FQ_CHUNK +
           (size_t)(j % FQ_CHUNK);
}
static inline size_t fq_batch_bytes(int64_t n, int32_t stride) {
    return (size_t)((n + FQ_TILE_READS - 1) / FQ_TILE_READS) * FQ_TILE_READS * (size_t)stride;
}
/* copy `len` bytes of `src` into read i's row of a plane (len <= stride) */
static inline void fq_batch_put_row(uint8_t* plane, int32_t stride, int64_t i, const uint8_t* src, int32_t len) {
    int32_t j;
    for (j = 0; j < len; j += FQ_CHUNK) {
        const int32_t m = len - j < FQ_CHUNK ? len - j : FQ_CHUNK;
        const size_t o = fq_batch_offset(stride, i, j);
        int32_t k;
        for (k = 0; k < m; ++k) plane[o + k] = src[j + k];
    }
}
/* copy read i's first `len` row bytes out of a plane */
static inline void fq_batch_get_row(const uint8_t* plane, int32_t stride, int64_t i, uint8_t* dst, int32_t len) {
    int32_t j;
    for (j = 0; j < len; j += FQ_CHUNK) {
        const int32_t m = len - j < FQ_CHUNK ? len - j : FQ_CHUNK;
        const size_t o = fq_batch_offset(stride, i, j);
        int32_t k;
        for (k = 0; k < m; ++k) dst[j + k] = plane[o + k];
    }
}

/* fq_read_result.flags */
#define FQ_RF_NULL 0x01      /* trimAndCut returned NULL (src/filter.cpp:78,100,124,160,183) */
#define FQ_RF_AD_OVERLAP 0x02 /* trimmed by AdapterTrimmer::trimByOverlapAnalysis */
#define FQ_RF_AD_SEQ 0x04    /* trimmed by AdapterTrimmer::trimBySequence */
#define FQ_RF_AD_NEG 0x08    /* trimBySequence matched at pos<0: recorded adapter = adapter[ad_pos:] */
#define FQ_RF_MERGED 0x10    /* (read-1 record) pair was merged (-m) */
#define FQ_RF_OVERLAP 0x20   /* (read-1 record) OverlapAnalysis reported overlapped for this pair */
#define FQ_RF_CORRECTED 0x40 /* -c corrected bases of this read (see fq_read_result) */
#define FQ_RF_INDEX_FILTERED 0x80 /* the pair/read was dropped by the index filter (FQ_BF_INDEX_FILTERED) */

/*
 * Everything the loop body's in-place std::string edits leave behind, per read (16 bytes).
 * The surviving read is original[start .. start+len).  For adapter bookkeeping
 * (FilterResult::addAdapterTrimmed, src/filterresult.cpp:138-177) the host rebuilds the
 * recorded adapter string from (ad_pos, ad_len): original[ad_pos .. ad_pos+ad_len), or, with
 * FQ_RF_AD_NEG, adapter[ad_pos .. ad_pos+ad_len).  For a merged pair (FQ_RF_MERGED, read-1
 * record) the merged read is r1[0:m_len1] + revcomp(r2)[ol : ol+m_len2] with ol = len2 - m_len2
 * (src/overlapanalysis.cpp:74-104); the read-1 record's code is the merged read's code.
 * Base correction (-c, FQ_RF_CORRECTED on either mate's record): the read-2 record carries the
 * correcting overlap, m_len1 = (int16_t) offset, m_len2 = overlap length, reserved = read 2's length
 * at correction time; both reads' windows start at their final `start`.  The corrected bytes are
 * those BaseCorrector::correctByOverlapAnalysis rewrites for that overlap (src/basecorrector.cpp:
 * 14-70), which a host re-applies to its copy of the text (fq_correct_pair_text below).
 */
typedef struct fq_read_result {
    uint16_t start;
    uint16_t len;
    uint8_t code;  /* Filter::passFilter result, FQ_PASS_FILTER ... */
    uint8_t flags; /* FQ_RF_* */
    uint16_t ad_pos;
    uint16_t ad_len;
    uint16_t m_len1;
    uint16_t m_len2;
    uint16_t reserved;
} fq_read_result;

/* util::complement, reference src/util.h:438-451 */
static inline char fq_complement(char c) {
    switch (c) {
        case 'A': case 'a': return 'T';
        case 'T': case 't': return 'A';
        case 'C': case 'c': return 'G';
        case 'G': case 'g': return 'C';
        default: return 'N';
    }
}

/* Re-applies the edits of BaseCorrector::correctByOverlapAnalysis (src/basecorrector.cpp:14-70)
 * for a FQ_RF_CORRECTED pair to a host copy of its text: s1/q1 = read 1 from its record's start,
 * s2/q2 = read 2 from its record's start, (offset, ol, len2) from the read-2 record
 * ((int16_t) m_len1, m_len2, reserved).  The engine took the same decisions on the device. */
static inline void fq_correct_pair_text(char* s1, char* q1, char* s2, char* q2, int offset, int ol, int len2) {
    const int start1 = offset > 0 ? offset : 0;
    const int start2 = len2 - (offset < 0 ? -offset : 0) - 1;
    const char good = (char)(33 + 30), bad = (char)(33 + 14); /* util::num2qual(30), (14) */
    int i;
    for (i = 0; i < ol; ++i) {
        const int p1 = start1 + i, p2 = start2 - i;
        if (s1[p1] == fq_complement(s2[p2])) continue;
        if ((signed char)q1[p1] >= good && (signed char)q2[p2] <= bad) {
            s2[p2] = fq_complement(s1[p1]);
            q2[p2] = q1[p1];
        } else if ((signed char)q2[p2] >= good && (signed char)q1[p1] <= bad) {
            s1[p1] = fq_complement(s2[p2]);
            q1[p1] = q2[p2];
        }
    }
}

/*
 * Flat accumulator (uint64 words).  Layout (indices into the uint64 array):
 *   FQ_ACC_FILTER + code          FilterResult::mFilterReadStats[32]
 *   FQ_ACC_ADAPTER_READS/BASES    FilterResult::mTrimmedAdapterReads/Bases
 *   FQ_ACC_POLYX_READS + b        FilterResult::mTrimmedPolyXReads[5]  (b in A,T,C,G,N order)
 *   FQ_ACC_POLYX_BASES + b        FilterResult::mTrimmedPolyXBases[5]
 *   FQ_ACC_MERGED_PAIRS           ThreadConfig::addMergedPairs
 *   FQ_ACC_INSERT + isize         PairEndProcessor::mInsertSizeHist[insert_size_max + 1]
 *   fq_acc_stats_offset(k)        Stats block k in {0 pre-R1, 1 pre-R2, 2 post-R1, 3 post-R2}:
 *        +FQ_ST_READS, +FQ_ST_LENGTH_SUM, +FQ_ST_Q20, +FQ_ST_Q30 then, from +FQ_ST_CYCLES,
 *        [max_cycles][16] = per cycle 8 base-class counts (mCycleBaseContents[b][c], b = byte&7)
 *        followed by 8 base-class quality sums (mCycleBaseQuality[b][c]).
 *   fq_acc_tail_offset + FQ_ACC_TAIL_*  the -c counters.
 * All counters are sums, so N engines (GPUs) combine by element-wise uint64 addition.
 */
#define FQ_ACC_FILTER 0
#define FQ_ACC_ADAPTER_READS 32
#define FQ_ACC_ADAPTER_BASES 33
#define FQ_ACC_POLYX_READS 34
#define FQ_ACC_POLYX_BASES 39
#define FQ_ACC_MERGED_PAIRS 44
#define FQ_ACC_INSERT 48
/* after the four Stats blocks (fq_acc_tail_offset): -c counters */
#define FQ_ACC_TAIL_CORRECTED_READS 0 /* FilterResult::mCorrectedReads                        */
#define FQ_ACC_TAIL_CORRECTED_BASES 1 /* sum of FilterResult::mCorrectionMatrix (CorrectedBases) */
#define FQ_ACC_TAIL_WORDS 16
#define FQ_ST_READS 0
#define FQ_ST_LENGTH_SUM 1
#define FQ_ST_Q20 2
#define FQ_ST_Q30 3
#define FQ_ST_CYCLES 16
#define FQ_ST_PER_CYCLE 16

static inline size_t fq_acc_stats_words(int32_t max_cycles) {
    return (size_t)FQ_ST_CYCLES + (size_t)max_cycles * FQ_ST_PER_CYCLE;
}
static inline size_t fq_acc_stats_offset(int32_t insert_size_max, int32_t max_cycles, int k) {
    size_t base = (size_t)FQ_ACC_INSERT + (size_t)(insert_size_max + 1);
    base = (base + 15) & ~(size_t)15;
    return base + (size_t)k * fq_acc_stats_words(max_cycles);
}
static inline size_t fq_acc_tail_offset(int32_t insert_size_max, int32_t max_cycles) {
    return fq_acc_stats_offset(insert_size_max, max_cycles, 4);
}
static inline size_t fq_acc_words(int32_t insert_size_max, int32_t max_cycles) {
    return fq_acc_tail_offset(insert_size_max, max_cycles) + FQ_ACC_TAIL_WORDS;
}

/* ---- engine ------------------------------------------------------------------------- */
typedef struct fq_engine fq_engine;

/* fq_engine_create: validates params, selects `device` (hipSetDevice), allocates the device
 * accumulator and staging buffers for packs of up to max_batch reads/pairs with rows of up to
 * max_stride bytes.  Fails with FQ_E_NO_DEVICE when no gfx950 device is present. */
int fq_engine_create(const fq_params* params, int device, int32_t max_batch, int32_t max_stride,
                     fq_engine** out);
int fq_engine_destroy(fq_engine* e);

/* Host-memory pack (the CLI path): H2D copy, kernels, D2H of the per-read results.
 * `results` has n entries (SE) or 2n entries (PE: [2i] = read 1, [2i+1] = read 2).
 * Synchronous; replaces one call of processPairEnd / processSingleEnd. */
int fq_engine_process(fq_engine* e, const fq_batch* host_batch, fq_read_result* results);

/* Device-resident pack (inputs already in HBM): enqueues the kernels on `stream`
 * (a hipStream_t; NULL = the HIP default stream) and returns without synchronising.
 * `device_results` may be NULL when the caller needs only the accumulators.
 * The engine's hand-off list (pairs / reads the fast kernels pass to the general kernel) is
 * shared by these calls: use one stream at a time per engine (concurrent streams need one
 * engine each). */
int fq_engine_process_device(fq_engine* e, const fq_batch* device_batch,
                             fq_read_result* device_results, void* stream);

/* ---- asynchronous host-pack pipeline ---------------------------------------------------
 * Replaces the reference's concurrent workers over disjoint packs (consumePack on -w threads,
 * src/peprocessor.cpp:546-566) with an in-order device pipeline per engine:
 * fq_engine_submit enqueues one host pack -- H2D on a copy-in stream, the kernels on the compute
 * stream, D2H of its records into `results` on a copy-out stream -- and returns without waiting.
 * Up to 3 packs are in flight per engine (a further submit first waits for the oldest pack's
 * device slot to drain).  The host batch arrays and `results` must stay valid and untouched
 * until fq_engine_poll has reported `seq_no`.  With pinned host memory (fq_host_alloc) pack
 * k+1's H2D overlaps pack k's kernels and pack k-1's D2H.
 * fq_engine_poll reports packs in submission order: it returns 1 and sets *seq_no when the
 * oldest pending pack is complete (its records are in its `results`), 0 when nothing is pending
 * or (wait == 0) the oldest pack is still running, and a negative FQ_E_* code on failure.
 * One thread submits and polls a given engine; fq_engine_process must not be mixed with
 * packs still pending. */
int fq_engine_submit(fq_engine* e, const fq_batch* host_batch, fq_read_result* results, uint64_t seq_no);
int fq_engine_poll(fq_engine* e, int wait, uint64_t* seq_no);
int fq_engine_pending(const fq_engine* e); /* packs submitted and not yet reported */

/* ---- FASTQ-text packs: GPU-side ingest and egress ------------------------------------------
 * Replaces the host's tile packing and output formatting (Read::toString + the writers' input,
 * src/read.h:166-168, src/peprocessor.cpp:457-491, src/seprocessor.cpp:337-350) for the plain
 * output case: the pack's records go over as the bytes of the input FASTQ (a span of the mapped
 * file or of the read arena, pageable or pinned) plus one fq_text_rec per record; the device builds
 * the tiled batch planes from the text, runs the pack's kernels, and writes the output FASTQ text
 * of the records that pass (both mates of a pair for PE, to out1 / out2, in input order, each
 * record "name\nseq[start, start+len)\nstrand\nqual[start, start+len)\n" as the reference writes
 * it) into `out`.  With -m (merge_enabled, PE, no --discard_unmerged) every pair's output is the
 * merged stream (src/peprocessor.cpp:351-385: the merged read, name "_merged_<m1>_<m2>" spliced in
 * before the first space, when it merged and passes; otherwise each read that passes), written to
 * out->text[0] (which must then hold text_bytes[0] + text_bytes[1] + 24 * n + 16 bytes), and
 * out->bytes[1] is 0.  Only for options whose outputs are out1 (+ out2) or that merged stream: no
 * -c, UMI, split, failed or unpaired outputs, no --discard_unmerged; the
 * routed egress below (fq_engine_set_egress, fq_engine_submit_text_routed) writes -c, failed,
 * unpaired and --discard_unmerged runs' streams, the index filter and --phred64 are attached with
 * fq_engine_set_index_filter / fq_engine_set_phred64 (device ingest, below), and the host routes
 * everything else (split outputs) through fq_engine_submit.  Records and text must stay valid until fq_engine_poll reports the pack; then
 * `results` holds the records as from fq_engine_submit and out->bytes[m] the bytes of out->text[m].
 * out->text[m] must hold at least the mate's text_bytes + 16 (a record's output is never longer
 * than its input text, except by the final line terminator that the input may lack). */
typedef struct fq_text_rec {
    uint32_t name_off;   /* offsets from the mate's text pointer: the name line (without its terminator), */
    uint32_t seq_off;    /* the sequence, */
    uint32_t strand_off; /* the strand line, */
    uint32_t qual_off;   /* the quality line */
    uint16_t name_len, strand_len, len, pad;
} fq_text_rec;
typedef struct fq_text_batch {
    int32_t n;      /* records (PE: pairs) */
    int32_t stride; /* row stride of the planes the device builds (multiple of 16, >= every len) */
    const char* text[2];
    uint64_t text_bytes[2];
    const fq_text_rec* rec[2]; /* rec[1]: PE only */
} fq_text_batch;
typedef struct fq_text_out {
    char* text[2];      /* host buffers (pinned for full speed) of at least text_bytes[m] */
    uint64_t bytes[2];  /* set when the pack is reported by fq_engine_poll */
} fq_text_out;
int fq_engine_submit_text(fq_engine* e, const fq_text_batch* tb, fq_read_result* results, fq_text_out* out,
                          uint64_t seq_no);

/* ---- raw FASTQ streams: record indexing on the GPU ------------------------------------------
 * Replaces the reader too (FqReader::read over its 1 MiB buffers and FqReaderPair::read,
 * src/fqreader.cpp:90-195, :254-267) for the plain part of an input, on top of the text-pack
 * path above.  The caller hands each mate's input bytes over in consecutive windows of any size
 * (fq_engine_raw_enqueue; page-locked or registered host memory, fq_host_register, makes the copy
 * asynchronous).  On the device each window's text is the previous window's bytes after its last
 * taken record followed by the new bytes; the line terminators ('\n' and '\r') are indexed and
 * record i is lines 4i .. 4i+3 while records are "plain": all four lines end in '\n' and are
 * non-empty, the first starts with '@', quality and sequence are equally long, name/strand lines
 * are < 65536 bytes and the sequence <= the engine's max_stride and max_cycles.  On plain records
 * the reference reader is exactly "four lines per record" (no '@' search, no "\r\n" folding at its
 * buffer ends, no length error).  A window's pack is the leading plain records (PE: pairs, the
 * minimum over the mates), up to max_batch; fq_engine_raw_launch runs it as a text pack.
 *   fq_raw_result.stop != 0: a complete record that is not plain follows the pack (or the carry
 *   overflowed): the caller continues with its own reader at each mate's stream offset
 *   (end of the window's bytes) - carry[m].  The same applies when the input ended (every mate's
 *   last window enqueued) with carry left, or a window takes no pairs.
 * Protocol: fq_engine_raw_begin; enqueue window 0; then for k = 0, 1, ...: enqueue window k+1
 * (optional), fq_engine_raw_launch (window k: waits for its index), poll as for other packs.  At
 * most three windows are enqueued and not launched, and eight windows are in the engine (enqueued,
 * launched or not yet polled: a ninth enqueue waits for the oldest pack's copies); a window's
 * host bytes (of either enqueue call) may be reused once fq_engine_raw_wait or the launch of that
 * window has returned: its copies are done by then.  Options as for text
 * packs (-m writes the merged stream into out->text.text[0], which must then hold both mates' window
 * and carry bytes + 28 * max_batch + 64; no -c, UMI, --discard_unmerged: those go
 * through fq_engine_raw_launch_routed below; the index filter and --phred64 as for text packs).
 * The trimmed-adapter strings (FilterResult::addAdapterTrimmed, src/filterresult.cpp:138-157) come
 * back after the output text, at out->text.text[m] + out->text.bytes[m], adapter_bytes[m] bytes of
 * entries "u16 ad_len (little endian), u8 neg, then ad_len bytes of the read (neg 0) or u16
 * ad_pos (neg 1: the string is adapter[ad_pos, ad_pos + ad_len) of the mate's adapter parameter)";
 * one copy back per mate, of the pack's text_bytes[m] + 3 * pairs + 16 bytes (a record's output
 * plus its entry is at most its input + 3 bytes).
 * Several engines on one GPU (one PCIe link): a window's host-to-device copies wait for the last
 * ones any other engine of the process enqueued on that device, and a pack's copies back likewise,
 * so copies run one after another in call order at the link's full rate; a caller dealing one
 * stream's windows over such engines enqueues (and launches) them in stream order.  Engines on
 * different GPUs never wait for each other. */
typedef struct fq_raw_window {
    const char* bytes[2]; /* mate m's next input bytes (bytes[1]: PE only) */
    uint64_t n[2];        /* their count, <= the window capacity given to fq_engine_raw_begin */
} fq_raw_window;
typedef struct fq_raw_result {
    int32_t pairs;      /* records (PE: pairs) in the window's pack */
    int32_t stop;       /* nonzero: the GPU path cannot continue after this pack (see above) */
    int32_t max_len;    /* longest sequence of the pack */
    int32_t pad;
    uint64_t carry[2];  /* mate m's bytes after the pack's last record (they stay on the device) */
    uint64_t text_bytes[2]; /* mate m's text bytes the pack's records span */
} fq_raw_result;
typedef struct fq_raw_out {
    fq_text_out text;          /* text[m]: >= carry capacity + window bytes + 4 * max_batch + 16 */
    uint64_t adapter_bytes[2]; /* set by fq_engine_poll: entries after the output text */
    /* Records-only egress (all set, or all null): instead of the output text the pack's records
     * come back -- results[2i + m] (PE) / results[i] as from fq_engine_submit, and rec[m][i] the
     * record's line offsets in the window buffer [carry capacity - carry | window bytes] (the
     * window's bytes at offset carry capacity, the previous pack's unconsumed bytes just before),
     * so a caller that kept its page-locked window bytes (and the carry in front of them) formats
     * the output itself; text.bytes and adapter_bytes are 0.  80 bytes per pair cross PCIe instead
     * of the ~input-sized text. */
    fq_read_result* results;   /* >= pairs * 2 (PE) / reads */
    fq_text_rec* rec[2];       /* >= max_batch each (rec[1]: PE) */
} fq_raw_out;
int fq_engine_raw_begin(fq_engine* e, uint64_t window_cap, uint64_t carry_cap);
int fq_engine_raw_enqueue(fq_engine* e, const fq_raw_window* w);
int fq_engine_raw_launch(fq_engine* e, fq_raw_result* r, fq_raw_out* out, uint64_t seq_no);
/* Waits until the oldest enqueued (not launched) window is indexed and reports its pack's pairs,
 * stop, carry and text bytes as fq_engine_raw_launch of it will (r may be null); that launch then
 * does not wait.  A caller ordering launches over several engines waits here, on each engine's own
 * thread, before it takes its turn (no counterpart in the reference: its reader is one thread). */
int fq_engine_raw_wait(fq_engine* e, fq_raw_result* r);
/* Leaves raw mode: waits for the copies and indexing of windows enqueued and never launched (their
 * host bytes may then be reused) and drops them; launched packs are polled as usual.  The engine
 * takes other packs, or a new fq_engine_raw_begin once nothing is in flight. */
int fq_engine_raw_end(fq_engine* e);

/* A window whose bytes are BGZF members, inflated on the device (inflate.hip, "device inflate"
 * below) straight into the window's place: only the compressed bytes cross PCIe.  The call stands
 * where fq_engine_raw_enqueue stands in the protocol, and the two may be mixed window by window;
 * wait, launch, poll and end are unchanged.  Mate m's members inflate back to back, the first at
 * `skip` bytes before the window's first byte (they land in the tail of the carry region, which the
 * carried bytes then overwrite), so the window is inflated bytes [skip, skip + n) of the members; a
 * window may start and end inside a member, and what the last member holds past skip + n is ignored
 * (the next window brings that member again).  The device buffers for the compressed bytes are made
 * at the first such call.
 * Refused (FQ_E_INVALID, nothing copied or launched, the engine stays usable): a call outside a raw
 * stream or with three windows waiting; members[m] > FQ_RAW_BGZF_MEMBERS; a member whose in_len or
 * isize exceeds FQ_INFLATE_MAX or whose payload is not within comp[m][0, comp_bytes[m]);
 * comp_bytes[m] above the window capacity; skip[m] above the carry capacity, or a carry capacity
 * below 65536; sum(isize) < skip + n, or sum(isize) - skip above the window capacity.
 * A member that is not FQ_INFL_OK: fq_engine_raw_wait and the launch of that window report
 * stop = FQ_RAW_STOP_INFLATE, pairs = 0 and carry[m] = the carried bytes + n[m] (nothing of the
 * window is taken: the caller resumes with its own reader at window end - carry, which reports the
 * error); windows enqueued behind it report the same and are dropped by fq_engine_raw_end. */
#define FQ_RAW_BGZF_MEMBERS 8192           /* members per mate and window */
#define FQ_RAW_STOP_INFLATE 2              /* fq_raw_result.stop: a member of the window was not FQ_INFL_OK */
struct fq_inflate_member;
typedef struct fq_raw_bgzf_window {
    const void* comp[2];            /* mate m's compressed bytes (page-locked: asynchronous copy) */
    uint64_t comp_bytes[2];         /* <= the window capacity of fq_engine_raw_begin */
    const struct fq_inflate_member* m[2];  /* in_off relative to comp[m]; status / produced are ignored */
    uint32_t members[2];            /* <= FQ_RAW_BGZF_MEMBERS */
    uint32_t skip[2];               /* leading inflated bytes that are not part of the window */
    uint64_t n[2];                  /* the window's bytes: inflated bytes [skip, skip + n) */
} fq_raw_bgzf_window;
int fq_engine_raw_enqueue_bgzf(fq_engine* e, const fq_raw_bgzf_window* w);

/* Page-locked host memory for packs and records (portable across devices; transparent huge
 * pages registered with the runtime, hipHostMalloc as fallback).  FQ_E_NO_DEVICE without a HIP
 * device: callers then use ordinary memory. */
int fq_host_alloc(size_t bytes, void** out);
int fq_host_free(void* p);
/* Page-lock an existing host range (e.g. of a read-only file mapping, page-aligned) so copies
 * from it are asynchronous DMA; fq_host_unregister releases it. */
int fq_host_register(const void* p, size_t bytes);
int fq_host_unregister(const void* p);

/* Accumulators */
size_t fq_engine_acc_words(const fq_engine* e);
int fq_engine_acc_device_ptr(fq_engine* e, uint64_t** dptr); /* for an RCCL all-reduce */
int fq_engine_read_acc(fq_engine* e, uint64_t* host_acc, size_t words);
/* Use a caller-owned, zero-initialised device buffer of fq_engine_acc_words() uint64 words as
 * the accumulator (e.g. a torch tensor that is then all-reduced over RCCL); NULL restores the
 * engine's own buffer. */
int fq_engine_set_acc_buffer(fq_engine* e, uint64_t* device_acc);
int fq_engine_reset_acc(fq_engine* e);
int fq_engine_sync(fq_engine* e);

/* Last error message of this engine (or of the last failed create when e == NULL). */
const char* fq_engine_last_error(const fq_engine* e);

/* Device id the engine runs on; gfx arch name of that device. */
int fq_engine_device_info(const fq_engine* e, int* device, char* arch, size_t arch_len);

/* ---- synthetic workload ------------------------------------------------ *
 * Fills a device-resident PE (seq2 != NULL) or SE batch with the seeded synthetic reads of
 * the benchmark configs: counter-based (splitmix64 keyed on seed and global read index), so
 * shards generate independently; `first_index` is the global index of the batch's first
 * pair/read.  Lengths are written too.  Asynchronous on `stream`. */
int fq_synth_fill_device(const fq_batch* device_batch, uint64_t seed, uint64_t first_index,
                         int32_t read_len, void* stream);

/* ---- duplication analysis (-d) ----------------------------------------------------------
 * Duplicate::statRead / statPair / statAll, reference src/duplicate.cpp:46-166.  A table lives
 * on one device and outlives engines (the tool re-creates engines when reads grow); an engine
 * with a table attached adds every later pack's reads to it, on its compute stream, in input
 * order (packs are ordered by their seq_no; fq_engine_process / process_device use a per-engine
 * call counter).  Tables of engines that processed interleaved packs of one input merge exactly
 * (fq_dup_merge), since each key remembers the order of its first read.  fq_dup_stat returns
 * statAll's histogram and GC sums (hist_size bins; a key seen more than hist_size times counts in
 * the last bin; exactly hist_size lands past the reference's array and is not reported) and
 * totals[0] = reads counted, totals[1] = duplicates (Rate = totals[1] / totals[0]). */
typedef struct fq_dup fq_dup;
int fq_dup_create(int device, int32_t keylen, fq_dup** out); /* keylen 1..31 (-dup_ana_key_len) */
int fq_dup_destroy(fq_dup* d);
int fq_dup_reset(fq_dup* d);
int fq_engine_set_dup(fq_engine* e, fq_dup* d); /* NULL detaches; d must be on the engine's device */
int fq_dup_merge(fq_dup* dst, const fq_dup* src);
int fq_dup_stat(fq_dup* d, int32_t hist_size, uint64_t* hist, uint64_t* gc_sum, uint64_t* totals);

/* ---- adapter-detection k-mers (Evaluator::evaluateAdapterSeq, src/evaluator.cpp:229-426) ------
 * A read set uploaded once (read i = seq[off[i] .. off[i+1]), n + 1 offsets).  For every read,
 * every window [pos, pos + keylen) of uppercase A/C/G/T bases with
 * first <= pos <= len - keylen - shift_tail is one k-mer (key = 2-bit codes A0 T1 C2 G3, first
 * base most significant, as Evaluator::seq2int).  fq_kmer_count fills counts[4^keylen];
 * fq_kmer_find lists where `seed` occurs as (read << 32 | pos), in no particular order, up to
 * cap entries (*n_out = all occurrences). */
typedef struct fq_kmer_set fq_kmer_set;
int fq_kmer_open(int device, const uint8_t* seq, const uint32_t* off, int32_t n, fq_kmer_set** out);
int fq_kmer_close(fq_kmer_set* s);
int fq_kmer_count(fq_kmer_set* s, int32_t keylen, int32_t first, int32_t shift_tail, uint32_t* counts);
int fq_kmer_find(fq_kmer_set* s, int32_t keylen, int32_t first, int32_t shift_tail, uint32_t seed, uint64_t* occ,
                 size_t cap, size_t* n_out);

/* ---- k-mer statistics (--kmer --kmer_length k) ------------------------------------------------
 * The KmerCount tables of the four Stats objects (Stats::statRead, reference src/stats.cpp:245,
 * 266-274): every window of k consecutive bytes that are all upper-case A/T/C/G is one k-mer, key
 * = 2-bit codes A0 T1 C2 G3, first base most significant (Evaluator::seq2int); a read shorter than
 * k has none.  A handle lives on one device and outlives engines, as a duplication table does; an
 * engine with a handle attached counts every later pack on its compute stream, through every entry
 * point: the original reads (before the UMI trim and -c, index-filtered pairs included) into the
 * pre tables, before the pack's main kernels, and after them the reads that reach the post-filter
 * statRead -- original[start, start + len) of passing reads as -c left them, or with -m the
 * merged read (its k-mers span the junction) in post-R1 -- into the post tables.  The handle holds
 * four tables of 4^k uint64 counters, [pre-R1 | pre-R2 | post-R1 | post-R2] (512 MiB at k = 12);
 * they are sums, so the tables of several engines combine by element-wise addition.  Nothing else
 * changes: records and accumulators are the same with and without a handle.  A process_device pack
 * without device_results keeps its records in a buffer of the handle.
 * fq_kstat_create refuses (FQ_E_INVALID) k outside FQ_KSTAT_MIN_K..FQ_KSTAT_MAX_K: the tables and
 * the reports grow as 4^k (the reference itself crashes at its nominal maximum of 16).
 * fq_kstat_last_kernel_ms: device-event time of the last pack's two k-mer passes, milliseconds. */
#define FQ_KSTAT_MIN_K 4
#define FQ_KSTAT_MAX_K 12
typedef struct fq_kstat fq_kstat;
int fq_kstat_create(int device, int32_t k, fq_kstat** out);
int fq_kstat_destroy(fq_kstat* h);
int fq_kstat_reset(fq_kstat* h);                 /* waits for the device, then zeroes the tables */
int fq_kstat_k(const fq_kstat* h);
size_t fq_kstat_words(const fq_kstat* h);        /* 4 * 4^k */
int fq_engine_set_kstat(fq_engine* e, fq_kstat* h); /* NULL detaches; h must be on the engine's device */
int fq_kstat_read(fq_kstat* h, uint64_t* host, size_t words); /* waits for the device, then copies */
double fq_kstat_last_kernel_ms(const fq_kstat* h);

/* ---- overrepresented sequences (--ora --ora_sample s) -------------------------------------------
 * The counts and per-cycle distributions of the four Stats objects (Stats::statRead, reference
 * src/stats.cpp:277-293).  A hot set is the caller's (Evaluator::computeOverRepSeq): set 1 serves
 * the read-1 Stats with evalLen1, set 2 the read-2 Stats with evalLen2; a set is its sequences'
 * bytes back to back, sequence i = seq[off[i], off[i + 1]) (n + 1 offsets), raw bytes compared as
 * they are, all distinct; n = 0 (seq and off may be NULL) is a valid empty set.
 * Every Stats samples the reads whose number in ITS stream is a multiple of `sampling`: for the pre
 * Stats a read's index over all packs so far, for the post Stats the number of reads that reached
 * it before.  The handle keeps these four running counts on the device and advances them in stream
 * order, so a handle is fed by ONE engine's packs in input order (unlike the k-mer tables, two
 * handles' results do not add up to one stream's).  A sampled read of length len is scanned for
 * each step of {10, 20, 40, 100, min(150, evalLen - 2)}: window j < len - step equal to a hot
 * sequence adds 1 to its count and to its distribution at cycles [j, min(j + step, evalLen)), and
 * the scan goes on at j + step + 1.  The passes sit where the k-mer passes do (pre: the original
 * reads, before the main kernels; post: what the records say reached the post-filter statRead, a
 * merged read in post-R1), through every entry point; records and accumulators do not change.
 * fq_ora_read: four blocks [pre-R1 | pre-R2 | post-R1 | post-R2], block of set s = n_s x (1 +
 * evalLen_s) uint64: per sequence, in the caller's order, its count and then its distribution.
 * fq_ora_create refuses (FQ_E_INVALID) sampling < 1, an evalLen < 3 (the reference throws there),
 * a sequence above 65535 bytes and a set with a repeated member.  Rows of more than 4096 bytes
 * fail the pack.  fq_ora_reset zeroes the blocks and the four running counts.
 * fq_ora_last_kernel_ms: device-event time of the last pack's two passes, milliseconds. */
typedef struct fq_ora fq_ora;
int fq_ora_create(int device, int32_t sampling, int32_t eval_len1, int32_t eval_len2, const uint8_t* seq1,
                  const uint32_t* off1, int32_t n1, const uint8_t* seq2, const uint32_t* off2, int32_t n2, fq_ora** out);
int fq_ora_destroy(fq_ora* h);
int fq_ora_reset(fq_ora* h);                  /* waits for the device */
size_t fq_ora_words(const fq_ora* h);
int fq_engine_set_ora(fq_engine* e, fq_ora* h); /* NULL detaches; h must be on the engine's device */
int fq_ora_read(fq_ora* h, uint64_t* host, size_t words); /* waits for the device, then copies */
double fq_ora_last_kernel_ms(const fq_ora* h);

/* ---- device BGZF: output text compressed on the GPU ---------------------------------------------
 * A span of text in device memory is cut into members of FQ_BGZF_IN input bytes (the last one
 * shorter; no bytes, no member).  Each member is a complete BGZF member laid out as the host
 * writer's: the 18-byte header "1f 8b 08 04 00000000 XFL ff 0600 'B' 'C' 0200 BSIZE-1", one
 * deflate block (dynamic Huffman over an LZ77 parse, or stored when that is not smaller), CRC32
 * and ISIZE.  XFL is 4 in members the device wrote and 0 in the host writer's, which is how a file
 * tells which side compressed a member (BGZF readers do not look at it).  A member is never
 * larger than its input + 31, so a stream of n bytes never exceeds fq_deflate_bound(n).
 * level 1..9 selects the search effort (1-3: the hash table of earlier positions and runs;
 * 4-9: also a second look-up among the nearest 256 positions); every level gives a valid stream.
 * fq_deflate_bgzf refuses (FQ_E_INVALID, nothing written) n > max_bytes, a level outside 1..9 and
 * out_cap < fq_deflate_bound(n).
 * fq_engine_set_gz_out (only while no pack is pending or enqueued, else FQ_E_INVALID) with level
 * 1..9 makes text packs (fq_engine_submit_text) and raw packs (fq_engine_raw_launch) compress
 * their output text on the device, on the compute stream behind the text kernel: out->text[m]
 * then receives BGZF members and out->bytes[m] is their byte count (-m: the merged stream in
 * text[0] likewise); raw packs' adapter entries still follow, uncompressed, at text[m] + bytes[m].
 * The caller's out->text[m] must then hold fq_deflate_bound(x), x being the size documented for
 * the plain case (text packs: text_bytes + 16, -m: both + 24 * n + 16; raw packs: carry capacity
 * + window bytes + 4 * max_batch + 16, -m: both mates' + 28 * max_batch + 64); the copy back is
 * exactly the members (text packs too: their sizes come back first, as raw packs').  Records-only
 * egress (out->results set) is refused while gz is on.  Level 0 (the default) turns it off;
 * fq_engine_submit and fq_engine_process* are unaffected.  The device scratch is allocated with
 * the slots' output buffers, nothing while gz is off.
 * Routed packs (fq_engine_submit_text_routed, fq_engine_raw_launch_routed, below) are compressed
 * likewise: behind the egress kernel one pair of launches compresses every open stream of the pack,
 * out->text[s] receives stream s's members and out->bytes[s] their byte count (0 for a stream
 * nothing was routed to: no bytes, no member), and the copies back are exactly the members.  The
 * caller's cap[s] must then be at least fq_deflate_bound(fq_egress_bound_umi(s, ...)), else the call
 * is refused (FQ_E_INVALID) before anything is launched or copied (a raw window stays enqueued).  A
 * routed raw pack's adapter entries stay uncompressed in adapters[m].
 * The streams' real sizes are known only on the device, and their bounds add up to several times the
 * pack's input (FAILED and MERGED may each take both mates), so the compressor's scratch is sized by
 * what the six streams can hold together.  Per pair the egress writes every read to at most one
 * stream: a read is its input record (name, bases, strand line, qualities and four terminators, of
 * which an input may lack the last), plus a blank and a failure tag of at most 22 bytes in FAILED,
 * plus its UMI tag; a merged pair is written once, with mate 1's name and strand line, at most both
 * mates' bases and a "_merged_<m1>_<m2>" tag of less than 24 bytes.  That is FAILED's own bound with
 * every read in it, so over all streams
 *     sum of bytes[s] before compression <= fq_egress_bound_umi(FQ_EG_FAILED, text_bytes1, text_bytes2, n, u)
 * and the members number at most ceil(that / FQ_BGZF_IN) plus one per open stream (each stream's
 * last member may be short).  Should a pack ever exceed the scratch, no member is taken for a write:
 * fq_engine_poll fails the pack with FQ_E_INVALID and every bytes[s] is 0.
 * fq_deflate_code_lengths runs the kernels' own length builder on the host (optimal length-limited
 * code lengths by package-merge: 0 for unused symbols; n_sym <= 288, max_len <= 15, the sum of
 * freq times max_len below 2^32, else FQ_E_INVALID). */
#define FQ_BGZF_IN 65280
size_t fq_deflate_bound(size_t n);      /* n + 31 * ceil(n / 65280): every member stored; 0 for 0; no device needed */
int fq_deflate_code_lengths(const uint32_t* freq, int32_t n_sym, int32_t max_len, uint8_t* len);
                                        /* the kernels' own length builder, run on the host (checks, tests); no device needed */
typedef struct fq_deflate fq_deflate;
int fq_deflate_create(int device, size_t max_bytes, fq_deflate** out);  /* FQ_E_NO_DEVICE as fq_engine_create */
int fq_deflate_destroy(fq_deflate* d);
int fq_deflate_bgzf(fq_deflate* d, const void* text, size_t n, int32_t level,
                    void* out, size_t out_cap, size_t* out_bytes);     /* host pointers, synchronous */
int fq_engine_set_gz_out(fq_engine* e, int32_t level);                  /* 0 (default): off */

/* ---- routed egress: every output stream of a text pack written on the GPU -----------------------
 * The text packs above write out1 / out2 or the merged stream only.  An engine with an egress set
 * routes each pair of a text pack as the loop bodies do (src/peprocessor.cpp:351-429,
 * src/seprocessor.cpp:337-350; fqtool_amd/host/processor.cpp format_range) over six streams:
 *   single end: a passing read -> OUT1; any other -> FAILED, tagged with its failure
 *     (" failed_too_short" ... after the name, Read::toStringWithTag, src/read.h:170-178);
 *   paired end: index-filtered pairs write nothing; with -m a merged pair that passes -> MERGED
 *     (a merged pair that fails writes nothing) and, without --discard_unmerged, an unmerged pair's
 *     passing reads -> MERGED; every other pair: both pass -> OUT1 and OUT2; only read 1 passes ->
 *     with UNPAIRED1 open r1 -> UNPAIRED1 and r2 -> FAILED, else r1 -> FAILED tagged
 *     "paired_read_is_failing" and r2 -> FAILED; only read 2 passes -> with UNPAIRED1 open (the
 *     reference tests the left writer, src/peprocessor.cpp:417) r2 -> UNPAIRED2 and r1 -> FAILED
 *     tagged with read 2's code (:420), else r1 -> FAILED and r2 -> FAILED tagged
 *     "paired_read_is_failing".  FAILED holds both mates in pair order.
 * A read is its record's window, or the whole read when its record is FQ_RF_NULL.  A stream whose
 * bit is clear in fq_egress.open has no writer: what is routed there is dropped, and UNPAIRED1's bit
 * is the "left writer" of the rules above.  With an egress set, fq_engine_submit_text_routed also
 * takes -c (a pair with FQ_RF_CORRECTED on either record takes its sequence and quality bytes, the
 * merged read's included, from the corrected rows of the tile planes; names and strand lines always
 * come from the text) and -m --discard_unmerged; UMI is taken once a UMI description is set
 * (fq_engine_set_umi below) and refused without one.
 * fq_engine_set_egress (only while no pack is pending or enqueued, else FQ_E_INVALID): NULL (the
 * default) turns the routed egress off; fq_engine_submit_text, fq_engine_raw_begin and
 * fq_engine_raw_launch write and refuse as before (fq_engine_raw_begin takes -c and
 * --discard_unmerged once an egress is set, for fq_engine_raw_launch_routed below), and the routed
 * calls are refused (FQ_E_INVALID) while no egress is set.  With device BGZF on (fq_engine_set_gz_out)
 * they write every open stream as BGZF members and the capacities below become those of the members,
 * fq_deflate_bound(fq_egress_bound(...)) ("device BGZF" above).
 * fq_egress_bound (no device needed) is the capacity stream s needs for a pack of n records whose
 * mates span text_bytes1 / text_bytes2 (0 for single end) bytes of input text: a record's output is
 * its input (plus the final line terminator an input may lack); a FAILED record adds a blank and a
 * tag of at most 23 bytes; MERGED is both mates' text plus a merged name's tag per pair, as for the
 * text packs above.  fq_engine_submit_text_routed refuses (FQ_E_INVALID, before anything is launched
 * or copied) an open stream without a buffer or with cap[s] below that bound.  The copies back are
 * the exact byte counts: the sizes come back first, then each stream's text; bytes[s] is set when
 * fq_engine_poll reports the pack (0 for a stream that is not open). */
enum { FQ_EG_OUT1 = 0, FQ_EG_OUT2 = 1, FQ_EG_MERGED = 2, FQ_EG_UNPAIRED1 = 3, FQ_EG_UNPAIRED2 = 4, FQ_EG_FAILED = 5,
       FQ_EG_STREAMS = 6 };
typedef struct fq_egress {
    uint32_t open;      /* bit s set: stream s has a writer */
    uint32_t reserved;  /* 0 */
} fq_egress;
typedef struct fq_egress_out {
    char* text[FQ_EG_STREAMS];     /* host buffers (pinned for full speed) of the open streams */
    uint64_t cap[FQ_EG_STREAMS];   /* their capacities, >= fq_egress_bound */
    uint64_t bytes[FQ_EG_STREAMS]; /* set when the pack is reported by fq_engine_poll */
} fq_egress_out;
size_t fq_egress_bound(int32_t stream, uint64_t text_bytes1, uint64_t text_bytes2, uint64_t n);
int fq_engine_set_egress(fq_engine* e, const fq_egress* eg);
int fq_engine_submit_text_routed(fq_engine* e, const fq_text_batch* tb, fq_read_result* results, fq_egress_out* out,
                                 uint64_t seq_no);
/* The same through the raw stream.  With an egress set, fq_engine_raw_begin also takes -c and
 * -m --discard_unmerged, and each window's pack is launched with fq_engine_raw_launch_routed in
 * fq_engine_raw_launch's place (which keeps refusing those options): the six streams as above, the
 * bounds taken over the pack's fq_raw_result.text_bytes and pairs (the window's and carry's bytes
 * and max_batch bound them before the launch), and the trimmed-adapter entries per mate, in
 * fq_engine_raw_launch's entry format, in buffers of their own: adapters[m] of at least
 * text_bytes[m] + 3 * pairs + 16 bytes when adapter_trimming is on; a corrected pair's entry holds
 * the corrected bytes.  A refusal (FQ_E_INVALID: a missing or small buffer) comes before anything is
 * launched and leaves the window enqueued.  fq_engine_set_egress is refused inside a raw stream. */
typedef struct fq_raw_egress_out {
    fq_egress_out eg;
    char* adapters[2];         /* mate m's entries (adapters[1]: PE only) */
    uint64_t adapter_cap[2];
    uint64_t adapter_bytes[2]; /* set when the pack is reported by fq_engine_poll */
} fq_raw_egress_out;
int fq_engine_raw_launch_routed(fq_engine* e, fq_raw_result* r, fq_raw_egress_out* out, uint64_t seq_no);
/* UMI (-u) on the routed egress.  The params' umi_front1/2 only cut the reads; the tag
 * UmiProcessor::process builds and addTagToName puts into both mates' names (src/umiprocessor.cpp:10-89;
 * fqtool_amd/host/processor.cpp umi_tag / tagged_name) is text, and the routed egress writes it once
 * the engine has the description: location 1..6 (index1, index2, read1, read2, per_index, per_read),
 * the UMI's length, the bases skipped after it, --umi_drop_comment and --umi_not_trim.  The tag is
 * " OX:Z:" + umi and, when there is a quality part, " BZ:Z:" + qual: Read::firstIndex of the name(s)
 * at locations 1, 2 and 5 (joined with '-' for a pair at 5), the first min(len, length) bases and
 * their qualities at 3, 4 and 6 (location 4's quality part is bounded by read 1's length; location 6
 * joins both reads' parts with '-', read 2's quality part taken after read 2's cut and bounded by
 * read 1's cut length); always from the input text, also for a -c corrected pair.  A tag without a umi
 * part is not added, nor is any at locations 2 and 4 on single-end input.  The tag goes in at the
 * name's first blank (the rest is dropped with drop_comment) or at its end; the failure tag and the
 * merged read's "_merged_<m1>_<m2>" then apply to the tagged name.  A FQ_RF_NULL read is written
 * whole minus its UMI cut, min(length + skip, len - 1) bases.
 * fq_engine_set_umi (only while no pack is pending or enqueued, and not inside a raw stream, else
 * FQ_E_INVALID): NULL (the default) detaches the description and every call refuses UMI as before.
 * A description is refused (FQ_E_INVALID) with a location outside 1..6, a length or skip that is
 * negative or above 65535, length 0 at locations 3 / 4 / 6, a flag other than 0 / 1, or when the engine's umi_front1/2 are not what it implies:
 * length + skip for read 1 at locations 3 and 6, for read 2 (paired) at 4 and 6, else 0, and 0 with
 * not_trim.  With a description and an egress set, fq_engine_submit_text_routed, fq_engine_raw_begin
 * and fq_engine_raw_launch_routed take UMI; fq_engine_submit_text and fq_engine_raw_launch keep
 * refusing, and fq_engine_raw_begin refuses a description without an egress.
 * fq_egress_bound_umi is the capacity the routed calls then check every open stream's buffer against
 * (refusing before anything is launched, as for fq_egress_bound, which it equals for u == NULL):
 *     fq_egress_bound(s, ...) + recs * add + names
 * with recs = n records in OUT1 / OUT2 / UNPAIRED1 / UNPAIRED2 and 2 n (paired) in MERGED and FAILED,
 * which may hold both mates (their own tags are in fq_egress_bound already);
 * add = 12 + 2 * length at locations 3 and 4 (" OX:Z:", " BZ:Z:" and the two parts), 14 + 4 * length
 * at 6 (two '-' more), names = 0; at locations 1 and 2 add = 6 (" OX:Z:") and names = (recs / n) *
 * text_bytes1 (text_bytes2 at location 2), at location 5 add = 7 (a '-' more) and names = (recs / n) *
 * (text_bytes1 + text_bytes2), since an index is part of a mate's name and the mate's text bytes
 * bound all its names.  A stream whose bound passes 2^32 - 1 is refused (the cursors are 32-bit).
 * The adapter entries of a routed raw pack are unchanged: an entry is at most 3 bytes plus bytes of
 * the read at the record's ad_pos, which counts from the untrimmed read and so already lies past the
 * UMI cut, so text_bytes[m] + 3 * pairs + 16 still bounds them. */
typedef struct fq_umi {
    int32_t location;      /* 1..6 */
    int32_t length, skip;
    uint8_t drop_comment, not_trim, reserved[2];
} fq_umi;
int fq_engine_set_umi(fq_engine* e, const fq_umi* u);
size_t fq_egress_bound_umi(int32_t stream, uint64_t text_bytes1, uint64_t text_bytes2, uint64_t n, const fq_umi* u);

/* ---- device ingest: the index filter and --phred64 on text packs and the raw stream ---------------
 * Index filter (--enable_index_filter; Filter::filterByIndex, src/filter.cpp:191-232, which runs on
 * the input names before the UMI step, src/peprocessor.cpp:283-290).  With a filter attached every
 * text-pack and raw-stream entry point (fq_engine_submit_text, fq_engine_submit_text_routed,
 * fq_engine_raw_launch, fq_engine_raw_launch_routed) runs one more kernel before the pack's main
 * kernels: it writes the pack's per-record FQ_BF_* flags, which the device batch then carries as a
 * host pack's fq_batch.flags would:
 *     flags[i] = match(list 1, firstIndex(name1)) || (paired && match(list 2, firstIndex(name2)))
 * firstIndex is Read::firstIndex (src/read.h:106-123) of the record's name line as it stands in the
 * text.  match is Filter::match: an entry matches when its mismatches with the index over
 * min(entry length, index length) bytes are <= threshold, so an empty index or an empty entry matches
 * whenever the list has an entry at all, and an empty list never matches.  Single end uses list 1
 * only.  A list is its entries' bytes back to back, entry i = list[m][off[m][i], off[m][i + 1])
 * (n[m] + 1 offsets), raw bytes compared as they are; n[m] = 0 (list and off may be NULL) is the empty
 * list.  The engine keeps a device copy, so the caller's arrays may go after the call.
 * fq_engine_set_index_filter (only while no pack is pending or enqueued, and not inside a raw stream,
 * else FQ_E_INVALID): NULL (the default) detaches the filter.  Refused (FQ_E_INVALID): a negative
 * threshold or n, offsets that do not start at 0 or decrease, an entry above 65535 bytes, reserved
 * not 0.  fq_engine_submit and fq_engine_process* keep taking the caller's fq_batch.flags.
 * --phred64 (Read::convertPhred64To33, src/read.h:71-75: q = max(33, (signed char)q - 31), so bytes
 * >= 128 become 33).  fq_engine_set_phred64 (the same call-time rules; on = 0 / 1) makes the same
 * entry points rewrite the quality line of every record of the pack in the device copy of the text,
 * in place, before the tile planes are built: planes, Stats, the output text, UMI BZ:Z: parts and
 * adapter entries all read that copy.  On the raw stream only a window's taken records are
 * converted: the carried bytes belong to records not yet taken (each is converted exactly once, in
 * the window that takes it), and a caller that resumes with its own reader does so on the
 * unconverted input.  The records-only egress (fq_raw_out.results) is refused while it is on: its
 * caller formats from host windows that were never converted. */
typedef struct fq_index_filter {
    const uint8_t* list[2];  /* list 1 / list 2 (paired end), entries back to back */
    const uint32_t* off[2];  /* n[m] + 1 offsets into list[m] */
    int32_t n[2];
    int32_t threshold;       /* --max_diff_for_match, >= 0 */
    int32_t reserved;        /* 0 */
} fq_index_filter;
int fq_engine_set_index_filter(fq_engine* e, const fq_index_filter* f);
int fq_engine_set_phred64(fq_engine* e, int on);

/* ---- pack cuts: where the reference's packs end inside a text pack (split outputs, -s / -S) -------
 * The reference closes and opens split files only between its own packs of --max_item_in_pack reads
 * (ThreadConfig::markProcessed, src/threadconfig.cpp:88-137).  An engine with cuts on describes, for
 * a pack whose first record has global index first_item (the records taken by all earlier packs of
 * the input), the pieces the pack falls into when it is cut in front of every record whose global
 * index is a multiple of `every`: fq_cuts_count(every, first_item, n) pieces, piece j holding the
 * pack's records of global index [(first_item / every + j) * every, ... + every).  Per piece:
 * bytes[m] = the output bytes of stream m (OUT1 / OUT2; single end: bytes[1] = 0) its records wrote,
 * so the pieces' bytes[m] add up to out->bytes[m] and piece j's text starts where piece j - 1's
 * ends; items = its records; passed = its records that were written (a pair both of whose reads
 * pass, a passing read in single end).  A piece may be empty of passing records (bytes 0).
 * fq_engine_set_cuts (only while no pack is pending or enqueued, and not inside a raw stream, else
 * FQ_E_INVALID): every = 0 (the default) turns cuts off; refused with -m (the merged stream is not a
 * split output) and while device BGZF is on (fq_engine_set_gz_out, which in turn is refused while
 * cuts are on).  fq_engine_next_cuts arms the table for the next pack of fq_engine_submit_text or
 * fq_engine_raw_launch only: `cuts` (host memory, cap entries) is filled when fq_engine_poll reports
 * that pack, and must stay valid until then.  The pack's call refuses (FQ_E_INVALID, before anything
 * is launched; a raw window stays enqueued, the table stays armed) cap < fq_cuts_bound(every, n), n
 * being the pack's records, and the records-only egress; the routed calls refuse while a table is
 * armed.  A pack submitted without fq_engine_next_cuts gets no table.  fq_cuts_bound and
 * fq_cuts_count need no device. */
typedef struct fq_cut {
    uint64_t bytes[2];
    uint32_t items;
    uint32_t passed;
} fq_cut;
size_t fq_cuts_bound(uint64_t every, uint64_t n);                           /* n / every + 2 (0 for every = 0) */
size_t fq_cuts_count(uint64_t every, uint64_t first_item, uint32_t n);      /* pieces of such a pack (0 for n = 0) */
int fq_engine_set_cuts(fq_engine* e, uint64_t every);
int fq_engine_next_cuts(fq_engine* e, uint64_t first_item, fq_cut* cuts, uint32_t cap);

/* ---- device inflate: BGZF input members inflated on the GPU ---------------------------------------
 * The mirror of device BGZF.  Every BGZF member is an independent raw deflate stream (RFC 1951)
 * whose compressed size, ISIZE and CRC32 stand in its header and trailer, so the place of its
 * bytes in the output is known before anything is inflated: one wave64 inflates one member
 * (stored, fixed and dynamic blocks, any number of them), checks the produced length against
 * ISIZE and the CRC32 of the produced bytes, and reports per member the first failure it met:
 *   FQ_INFL_DATA   the payload is no valid deflate stream, or ends before its last block does
 *   FQ_INFL_LONG   it would inflate to more than isize bytes (the byte past isize is not written)
 *   FQ_INFL_SHORT  its last block ended after fewer than isize bytes
 *   FQ_INFL_CRC    length right, CRC32 wrong
 * The payload may be any bytes at all: reads are bounded by in_len, writes by isize, distances by
 * the bytes produced so far in the member.  The device is stricter than zlib about
 * incomplete code-length sets only (of those it takes none but a distance set with no code or with
 * a single one-bit code; zlib also lets a one-symbol literal/length code through); it never accepts
 * what zlib rejects, and bytes after the last block's end are ignored as zlib's inflate() ignores them.
 * fq_inflate_create sizes the handle's device buffers for calls of up to max_in payload bytes,
 * max_out output bytes and max_members members; the handle owns one non-blocking stream, and one
 * thread uses it at a time.
 * fq_inflate_members refuses (FQ_E_INVALID, nothing written, no launch) a member whose in_len or
 * isize exceeds FQ_INFLATE_MAX or whose payload does not lie within comp[0, comp_bytes), totals
 * above the handle's limits, and out_cap below the sum of isize.  Otherwise member i's bytes land
 * at out + isize[0] + ... + isize[i - 1], status and produced are set in every member, and *n_bad
 * counts the members that are not FQ_INFL_OK (FQ_OK is returned all the same: bad data is a result,
 * not a failure of the call).
 * fq_inflate_bgzf walks the member chain of a whole BGZF file image itself (RFC 1952 header with
 * the 'BC' extra subfield; the members must cover the n bytes exactly, else FQ_E_INVALID), inflates
 * all members, and sets *out_bytes to the sum of ISIZE and *first_bad to the index of the first
 * member that is not OK (-1: none; the bytes before that member's range are good). */
#define FQ_INFLATE_MAX 65536          /* largest in_len and isize the device takes per member */
enum { FQ_INFL_OK = 0, FQ_INFL_DATA = 1, FQ_INFL_LONG = 2, FQ_INFL_SHORT = 3, FQ_INFL_CRC = 4 };
typedef struct fq_inflate_member {
    uint64_t in_off;    /* the member's deflate payload: offset in `comp` ... */
    uint32_t in_len;    /* ... and length (<= FQ_INFLATE_MAX) */
    uint32_t isize;     /* bytes it must inflate to (<= FQ_INFLATE_MAX; 0 is legal: the EOF member) */
    uint32_t crc;       /* CRC32 they must have */
    uint32_t status;    /* out: FQ_INFL_* (the first failure met) */
    uint32_t produced;  /* out: bytes written for this member (== isize when OK, <= isize always) */
    uint32_t pad;
} fq_inflate_member;
typedef struct fq_inflate fq_inflate;
int fq_inflate_create(int device, size_t max_in, size_t max_out, size_t max_members, fq_inflate** out);
                                      /* FQ_E_NO_DEVICE as fq_deflate_create */
int fq_inflate_destroy(fq_inflate* h);
/* host pointers, synchronous; member i's bytes land at out + sum of isize[0..i).
 * *n_bad = members whose status is not OK; their output ranges hold `produced` bytes, then unspecified bytes */
int fq_inflate_members(fq_inflate* h, const void* comp, size_t comp_bytes, fq_inflate_member* m, size_t n,
                       void* out, size_t out_cap, size_t* n_bad);
/* a whole BGZF chain: walks the headers itself */
int fq_inflate_bgzf(fq_inflate* h, const void* bgzf, size_t n, void* out, size_t out_cap,
                    size_t* out_bytes, int64_t* first_bad /* member index, -1: none */);
/* the inflate kernel's time in the handle's last call (HIP events around the launch), milliseconds */
double fq_inflate_last_kernel_ms(const fq_inflate* h);

/* Kernel timing of the engine's last process_device call (HIP events on the launch stream),
 * in milliseconds; 0 when unavailable. */
double fq_engine_last_kernel_ms(const fq_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* FQENGINE_H */
