// kstat_core.h -- the per-read k-mer counting of --kmer (Stats::statRead, reference
// src/stats.cpp:245,266-274 with Evaluator::seq2int, src/evaluator.cpp:3-49), shared by the device
// kernels (kstat.hip) and host code (tools/micro/kstat_sim.cpp).
//
// A read contributes every window of k consecutive bytes that are all one of 'A' 'T' 'C' 'G'
// (upper case only); the key is base 4 with A0 T1 C2 G3, first base most significant.  The
// reference's rolling update and its fresh computation give the same key, so a window's key is
// the low 2k bits of the rolling value once the last k bytes were all valid.
//
// Reads live in the chunk-interleaved tile planes of include/fqengine.h; a row is walked with one
// 16-byte load per chunk.  Every routine takes `emit(key)`: the caller decides where the
// increment goes (an LDS cell, a global cell, a host array).
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/fqengine.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQ_KSTAT_HD __host__ __device__ __forceinline__
#else
#define FQ_KSTAT_HD inline
#endif
#if defined(__clang__)
#define FQ_KSTAT_UNROLL _Pragma("unroll")
#else
#define FQ_KSTAT_UNROLL
#endif

namespace fqkstat {

// A0 T1 C2 G3, anything else (N, lower case, IUPAC) -1.  The four letters lie in 64..95 and differ
// in bits 1-2 ((c >> 1) & 3: A0 C1 T2 G3), which 0xD8 maps to the reference's order.
FQ_KSTAT_HD int code2(uint8_t c) {
    const uint32_t letters = (1u << ('A' & 31)) | (1u << ('C' & 31)) | (1u << ('G' & 31)) | (1u << ('T' & 31));
    const bool ok = ((uint32_t)c ^ 0x40u) < 32u && ((letters >> (c & 31)) & 1u);
    return ok ? (int)((0xD8u >> (c & 6)) & 3u) : -1;
}

// util::complement as the merge applies it (include/fqengine.h fq_complement)
FQ_KSTAT_HD uint8_t comp(uint8_t c) {
    switch (c) {
        case 'A': case 'a': return 'T';
        case 'T': case 't': return 'A';
        case 'C': case 'c': return 'G';
        case 'G': case 'g': return 'C';
        default: return 'N';
    }
}

// Read idx's row of a tiled plane: byte j is at base[(j / 16) * 512 + j % 16]
struct kstat_row {
    const uint8_t* base;  // byte 0 of the row's chunk 0
    FQ_KSTAT_HD kstat_row(const uint8_t* plane, int stride, int64_t idx)
        : base(plane + (size_t)(idx / FQ_TILE_READS) * FQ_TILE_READS * (size_t)stride +
               (size_t)(idx % FQ_TILE_READS) * FQ_CHUNK) {}
    // the row's 16-byte chunk c as four words (one 16-byte load)
    FQ_KSTAT_HD void chunk(int c, uint32_t (&w)[4]) const {
        const uint8_t* p = base + (size_t)c * (FQ_TILE_READS * FQ_CHUNK);
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
#else
        memcpy(w, p, 16);
#endif
    }
};

// the rolling key of one read
struct kstat_roll {
    uint32_t key, mask;
    int run, k;
    FQ_KSTAT_HD explicit kstat_roll(int k_) : key(0), mask(k_ >= 16 ? 0xFFFFFFFFu : (1u << (2 * k_)) - 1u), run(0), k(k_) {}
    template <class Emit>
    FQ_KSTAT_HD void push(uint8_t c, Emit& emit) {
        const int v = code2(c);
        if (v < 0) {
            run = 0;
            return;
        }
        key = ((key << 2) | (uint32_t)v) & mask;
        if (++run >= k) emit(key);
    }
};

// row[start, start + len) into the rolling key, chunk by chunk: the 16 bytes of a chunk are taken
// out of its four words with constant shifts (the loop is unrolled), the chunk's bytes outside the
// range are skipped
template <class Emit>
FQ_KSTAT_HD void feed(kstat_roll& roll, const kstat_row& r, int start, int len, Emit& emit) {
    if (len <= 0) return;
    const int end = start + len;
    for (int c = start >> 4; c * 16 < end; ++c) {
        uint32_t w[4];
        r.chunk(c, w);
        const int lo = start - c * 16, hi = end - c * 16;
        FQ_KSTAT_UNROLL
        for (int b = 0; b < 16; ++b)
            if (b >= lo && b < hi) roll.push((uint8_t)(w[b >> 2] >> ((b & 3) * 8)), emit);
    }
}

// the complements of row[start + len - 1], ..., row[start], in that order
template <class Emit>
FQ_KSTAT_HD void feed_revcomp(kstat_roll& roll, const kstat_row& r, int start, int len, Emit& emit) {
    if (len <= 0) return;
    const int end = start + len;
    for (int c = (end - 1) >> 4; c >= start >> 4; --c) {
        uint32_t w[4];
        r.chunk(c, w);
        const int lo = start - c * 16, hi = end - c * 16;
        FQ_KSTAT_UNROLL
        for (int b = 15; b >= 0; --b)
            if (b >= lo && b < hi) roll.push(comp((uint8_t)(w[b >> 2] >> ((b & 3) * 8))), emit);
    }
}

// the k-mers of row[start, start + len)
template <class Emit>
FQ_KSTAT_HD void count_row(const kstat_row& r, int start, int len, int k, Emit& emit) {
    if (len < k) return;
    kstat_roll roll(k);
    feed(roll, r, start, len, emit);
}

// the k-mers of a merged read (OverlapAnalysis::merge, src/overlapanalysis.cpp:74-104):
// a[st1, st1 + m1) followed by revcomp(b[st2, st2 + n2))[ol, ol + m2) with ol = n2 - m2, i.e. the
// complements of b[st2 + m2 - 1], ..., b[st2]; windows span the junction
template <class Emit>
FQ_KSTAT_HD void count_merged(const kstat_row& a, int st1, int m1, const kstat_row& b, int st2, int m2, int k, Emit& emit) {
    if (m1 + m2 < k) return;
    kstat_roll roll(k);
    feed(roll, a, st1, m1, emit);
    feed_revcomp(roll, b, st2, m2, emit);
}

// Which reads of a processed pair reach the post-filter statRead, from its records (reference
// src/peprocessor.cpp:351-403): with -m a merged pair counts its merged read in post-R1 when that
// passes; a pair that did not overlap counts each passing mate on its own unless unmerged pairs
// are discarded; without -m both mates count when both pass.  A mate that trimAndCut dropped
// (FQ_RF_NULL) keeps the pair out, index-filtered pairs never get here.  Windows that do not lie
// inside the read (a record of a pack that failed) are skipped, never read.
// The visitor takes them in the reference's order: v.row1(start, len) / v.merged(st1, m1, st2, m2)
// go to post-R1, v.row2(start, len) to post-R2 (ora_core.h walks the same reads).
template <class Visit>
FQ_KSTAT_HD void visit_post_pair(int merge_enabled, int discard_unmerged, const fq_read_result& r1, const fq_read_result& r2,
                                 int l1, int l2, Visit& v) {
    if ((r1.flags | r2.flags) & (FQ_RF_NULL | FQ_RF_INDEX_FILTERED)) return;
    if ((int)r1.start + (int)r1.len > l1 || (int)r2.start + (int)r2.len > l2) return;
    if (merge_enabled) {
        if (r1.flags & FQ_RF_MERGED) {
            if (r1.code != FQ_PASS_FILTER || r1.m_len1 > r1.len || r1.m_len2 > r2.len) return;
            v.merged(r1.start, r1.m_len1, r2.start, r1.m_len2);
        } else if (!discard_unmerged) {
            if (r1.code == FQ_PASS_FILTER) v.row1(r1.start, r1.len);
            if (r2.code == FQ_PASS_FILTER) v.row2(r2.start, r2.len);
        }
        return;
    }
    if (r1.code != FQ_PASS_FILTER || r2.code != FQ_PASS_FILTER) return;
    v.row1(r1.start, r1.len);
    v.row2(r2.start, r2.len);
}

// single end (reference src/seprocessor.cpp:339-345)
template <class Visit>
FQ_KSTAT_HD void visit_post_single(const fq_read_result& r, int l, Visit& v) {
    if (r.flags & (FQ_RF_NULL | FQ_RF_INDEX_FILTERED)) return;
    if (r.code != FQ_PASS_FILTER || (int)r.start + (int)r.len > l) return;
    v.row1(r.start, r.len);
}

// the k-mers of those reads: emit1 / emit2 take the post-R1 / post-R2 keys
template <class Emit1, class Emit2>
struct kstat_post_count {
    const kstat_row& s1;
    const kstat_row& s2;
    int k;
    Emit1& emit1;
    Emit2& emit2;
    FQ_KSTAT_HD void row1(int start, int len) { count_row(s1, start, len, k, emit1); }
    FQ_KSTAT_HD void row2(int start, int len) { count_row(s2, start, len, k, emit2); }
    FQ_KSTAT_HD void merged(int st1, int m1, int st2, int m2) { count_merged(s1, st1, m1, s2, st2, m2, k, emit1); }
};

template <class Emit1, class Emit2>
FQ_KSTAT_HD void post_pair(int merge_enabled, int discard_unmerged, const fq_read_result& r1, const fq_read_result& r2,
                           const kstat_row& s1, int l1, const kstat_row& s2, int l2, int k, Emit1& emit1, Emit2& emit2) {
    kstat_post_count<Emit1, Emit2> v{s1, s2, k, emit1, emit2};
    visit_post_pair(merge_enabled, discard_unmerged, r1, r2, l1, l2, v);
}

template <class Emit>
FQ_KSTAT_HD void post_single(const fq_read_result& r, const kstat_row& s, int l, int k, Emit& emit) {
    kstat_post_count<Emit, Emit> v{s, s, k, emit, emit};
    visit_post_single(r, l, v);
}

}  // namespace fqkstat
