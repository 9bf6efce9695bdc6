// deflate_core.h -- the BGZF member compressor of deflate.hip: the Huffman length builder and the
// other single-thread pieces as __host__ __device__ functions (the host runs them for checks), and
// the per-member workgroup routine, the compaction of a member, and the index arithmetic and walks
// of the multi-span kernels.  Included by deflate.hip only, after <hip/hip_runtime.h>
// (tools/micro/deflate_sim.cpp compiles it for the host).
//
// One 256-thread workgroup compresses one member (<= 65280 input bytes, whole in LDS):
//   1. matches: the member is walked in sub-blocks of 256 positions, one position per thread.  In
//      each sub-block every thread first looks its 4-byte hash up in the LDS table (which then holds
//      only positions of earlier sub-blocks: look up before insert), then all threads insert their
//      positions, then (level >= 4) a second look-up finds a position of the same sub-block.  A run
//      candidate (distance 1) is always tried.  A candidate q is used only if 0 < p - q <= 32768 and
//      the bytes at q and p really agree, so whatever the table holds is harmless; the table is
//      cleared per member.  The longest match of every position goes to a per-workgroup array in
//      device memory (4 bytes per position).
//   2. parse: the member is cut into 256 chunks of 255 bytes, one per thread; each thread parses its
//      chunk greedily on its own (matches never cross a chunk end, so no thread waits for another),
//      writes its tokens over the match array in place and counts symbols into LDS histograms.
//   3. code lengths (package-merge, one thread per tree), the code-length alphabet, canonical codes.
//   4. bits: each thread sums the bit lengths of its tokens, a workgroup prefix sum gives its bit
//      offset, and it ORs its codes into the LDS image of the block (over the input, which is dead
//      by then unless the block is stored).
//   5. CRC32 per chunk, shifted to its place in the member (multiplication by x^(8 * bytes after
//      the chunk) modulo the CRC polynomial) and XORed together.
// Every loop is bounded by a constant or by the member's length, never by table contents.
#pragma once
#include <stdint.h>

#include "crc_core.h"  // fq_crc_mul, fq_crc_xpow8, fq_crc_bytes

#define FQ_DEFL_THREADS 256
#define FQ_DEFL_CHUNK 255          // bytes each thread parses (256 * 255 = 65280)
#define FQ_DEFL_MIN_MATCH 4
#define FQ_DEFL_WINDOW 32768
#define FQ_DEFL_HASH_BITS 12
#define FQ_DEFL_NLIT 286
#define FQ_DEFL_NDIST 30
#define FQ_DEFL_NCL 19
#define FQ_DEFL_SLOT 65536         // scratch bytes per member (a member is <= 65280 + 31)

// ---- LDS layout (bytes) --------------------------------------------------------------------
#define FQ_DL_IN 0                                // input, later the block's bit image
#define FQ_DL_IN_BYTES 65296
#define FQ_DL_HASH (FQ_DL_IN + FQ_DL_IN_BYTES)    // u16[4096]; later the length builders' workspace
#define FQ_DL_HASH_BYTES 8192
#define FQ_DL_LFREQ (FQ_DL_HASH + FQ_DL_HASH_BYTES)  // u32[288]
#define FQ_DL_DFREQ (FQ_DL_LFREQ + 1152)          // u32[32]
#define FQ_DL_LCODE (FQ_DL_DFREQ + 128)           // u16[288]
#define FQ_DL_DCODE (FQ_DL_LCODE + 576)           // u16[32]
#define FQ_DL_LLEN (FQ_DL_DCODE + 64)             // u8[288]
#define FQ_DL_DLEN (FQ_DL_LLEN + 288)             // u8[32]
#define FQ_DL_CLFREQ (FQ_DL_DLEN + 32)            // u32[20]
#define FQ_DL_CLCODE (FQ_DL_CLFREQ + 80)          // u16[20]
#define FQ_DL_CLLEN (FQ_DL_CLCODE + 40)           // u8[24]
#define FQ_DL_SEQ (FQ_DL_CLLEN + 24)              // u16[320]: code-length symbol | extra << 8
#define FQ_DL_SCAN (FQ_DL_SEQ + 640)              // u32[256]
#define FQ_DL_MISC (FQ_DL_SCAN + 1024)            // u32[16]
#define FQ_DL_TOTAL (FQ_DL_MISC + 64)
// two workgroups per CU of the 160 KiB LDS
static_assert(FQ_DL_TOTAL <= 80 * 1024, "deflate workgroup must leave room for two per CU");

enum { FQ_DM_CRC = 0, FQ_DM_HBITS, FQ_DM_HLIT, FQ_DM_HDIST, FQ_DM_HCLEN, FQ_DM_NSEQ, FQ_DM_BAD };

// ---- several spans of one launch: the member index arithmetic -------------------------------------
// The multi-span kernels (deflate.hip fq_deflate_spans_kernel / fq_compact_spans_kernel) number the
// members of up to FQ_DEFL_SPANS texts with one global index g: span k's members are
// [base[k], base[k + 1]), base[FQ_DEFL_SPANS] is their count.  Member g is compressed into scratch
// slot g and compacted to its own span's buffer at the sum of the sizes of slots [first, g).
// (No array here is indexed with a run-time value: on the device that would put it in scratch memory.)
#define FQ_DEFL_SPANS 6            // = FQ_EG_STREAMS, the routed egress's streams
#define FQ_DEFL_MEMBER_IN 65280    // = FQ_BGZF_IN
struct fq_defl_layout {
    unsigned long long len[FQ_DEFL_SPANS];       // each span's bytes, clamped to its capacity
    unsigned long long base[FQ_DEFL_SPANS + 1];
};
struct fq_defl_place {
    int span;                  // -1: g is no member
    unsigned long long first;  // global index of the span's first member
    unsigned long long at;     // byte offset of the member's input in its span
    uint32_t len;              // its input bytes (1..65280)
    bool last;                 // the span's last member
};

// n[k]: span k's length word as read, cap[k]: its capacity (0 for a span that is not there)
__host__ __device__ inline void fq_defl_spans_layout(const unsigned long long (&n)[FQ_DEFL_SPANS],
                                                     const unsigned long long (&cap)[FQ_DEFL_SPANS], fq_defl_layout& L) {
    unsigned long long b = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < FQ_DEFL_SPANS; ++k) {
        L.len[k] = n[k] < cap[k] ? n[k] : cap[k];
        L.base[k] = b;
        b += (L.len[k] + FQ_DEFL_MEMBER_IN - 1) / FQ_DEFL_MEMBER_IN;
    }
    L.base[FQ_DEFL_SPANS] = b;
}

__host__ __device__ inline fq_defl_place fq_defl_spans_place(const fq_defl_layout& L, unsigned long long g) {
    fq_defl_place p{-1, 0, 0, 0, false};
    if (g >= L.base[FQ_DEFL_SPANS]) return p;
    unsigned long long len = 0, next = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < FQ_DEFL_SPANS; ++k) {
        // (an empty span has base[k] == base[k + 1] and is never chosen)
        const bool in = g >= L.base[k] && g < L.base[k + 1];
        p.span = in ? k : p.span;
        p.first = in ? L.base[k] : p.first;
        len = in ? L.len[k] : len;
        next = in ? L.base[k + 1] : next;
    }
    p.at = (g - p.first) * FQ_DEFL_MEMBER_IN;
    const unsigned long long rest = len - p.at;
    p.len = (uint32_t)(rest < FQ_DEFL_MEMBER_IN ? rest : FQ_DEFL_MEMBER_IN);
    p.last = g + 1 == next;
    return p;
}

// ---- Huffman code lengths: package-merge ------------------------------------------------------
// 32-bit words of workspace fq_huff_code_lengths needs for n_sym symbols and max_len levels
__host__ __device__ inline uint32_t fq_huff_ws_words(int n_sym, int max_len) {
    const uint32_t n = (uint32_t)n_sym;
    return 3 * n + (n + 1) / 2 + (uint32_t)max_len * ((2 * n + 31) / 32);
}

// Optimal length-limited prefix code lengths (package-merge, Larmore & Hirschberg 1990, in the
// compact form that keeps one leaf/package bit per item and level).  freq[n_sym] -> len[n_sym]:
// 0 for unused symbols, 1..max_len for used ones; one used symbol gets length 1.  Sorts the used
// symbols itself (insertion sort, by frequency then symbol).  The sum of the frequencies times
// max_len must fit 32 bits.  Returns 0, or -1 when the used symbols cannot be coded in max_len
// bits or the result fails the Kraft check (sum 2^-len == 1 for two or more used symbols).
// Loops: n^2 for the sort, max_len * 2n for the merge, max_len * 2n for the walk back.
__host__ __device__ inline int fq_huff_code_lengths(const uint32_t* freq, int n_sym, int max_len, uint8_t* len,
                                                    uint32_t* ws) {
    uint32_t* w = ws;                       // leaf weights, ascending
    uint32_t* pa = ws + n_sym;              // packages of the previous level
    uint32_t* pb = ws + 2 * n_sym;          // packages being made
    uint16_t* sym = (uint16_t*)(ws + 3 * n_sym);
    uint32_t* flags = ws + 3 * n_sym + (n_sym + 1) / 2;
    const int fw = (2 * n_sym + 31) / 32;   // flag words per level
    int n = 0;
    for (int s = 0; s < n_sym; ++s) {
        len[s] = 0;
        const uint32_t f = freq[s];
        if (!f) continue;
        int i = n++;
        for (; i > 0 && w[i - 1] > f; --i) {
            w[i] = w[i - 1];
            sym[i] = sym[i - 1];
        }
        w[i] = f;
        sym[i] = (uint16_t)s;
    }
    if (n == 0) return 0;
    if (n == 1) {
        len[sym[0]] = 1;
        return 0;
    }
    if (max_len < 1 || max_len > 15 || n > (1 << max_len)) return -1;
    const int kmax = 2 * n - 2;
    int np = 0;  // packages in pa
    int cnt_last = 0;
    for (int j = 0; j < max_len; ++j) {
        uint32_t* fl = flags + j * fw;
        for (int i = 0; i < fw; ++i) fl[i] = 0;
        int li = 0, pi = 0, items = 0, nq = 0;
        uint32_t carry = 0;
        for (; items < kmax && (li < n || pi < np); ++items) {
            uint32_t x;
            if (li < n && (pi >= np || w[li] <= pa[pi])) {
                x = w[li++];
            } else {
                x = pa[pi++];
                fl[items >> 5] |= 1u << (items & 31);
            }
            if (items & 1) pb[nq++] = carry + x;
            else carry = x;
        }
        cnt_last = items;
        uint32_t* t = pa;
        pa = pb;
        pb = t;
        np = nq;
    }
    if (cnt_last < kmax) return -1;
    // walk back: of the k items taken at a level, the leaves are the first c leaves, each one bit
    // longer; the packages were made of the first 2 * (k - c) items of the level before
    int k = kmax;
    for (int j = max_len - 1; j >= 0 && k > 0; --j) {
        const uint32_t* fl = flags + j * fw;
        int pk = 0;
        for (int i = 0; i < k; ++i) pk += (fl[i >> 5] >> (i & 31)) & 1;
        const int c = k - pk;
        for (int s = 0; s < c; ++s) ++len[sym[s]];
        k = 2 * pk;
    }
    uint32_t kraft = 0;
    for (int s = 0; s < n; ++s) {
        const int l = len[sym[s]];
        if (l < 1 || l > max_len) return -1;
        kraft += 1u << (max_len - l);
    }
    return kraft == (1u << max_len) ? 0 : -1;
}

// canonical codes of the lengths (RFC 1951 3.2.2), bit-reversed: deflate packs codes from the
// most significant bit while everything else goes in from the least significant
__host__ __device__ inline void fq_huff_codes(const uint8_t* len, int n_sym, uint16_t* code) {
    uint32_t count[16], next[16];
    for (int i = 0; i < 16; ++i) count[i] = 0;
    for (int s = 0; s < n_sym; ++s) ++count[len[s]];
    count[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) {
        c = (c + count[b - 1]) << 1;
        next[b] = c;
    }
    for (int s = 0; s < n_sym; ++s) {
        const int l = len[s];
        uint32_t r = 0;
        if (l) {
            const uint32_t v = next[l]++;
            for (int b = 0; b < l; ++b) r |= ((v >> b) & 1u) << (l - 1 - b);
        }
        code[s] = (uint16_t)r;
    }
}

// length 3..258 -> code 257..285, extra bits and their value
__host__ __device__ inline void fq_len_code(uint32_t len, uint32_t& code, uint32_t& ebits, uint32_t& eval) {
    const uint32_t l = len - 3;
    if (len == 258) {
        code = 285, ebits = 0, eval = 0;
    } else if (l < 8) {
        code = 257 + l, ebits = 0, eval = 0;
    } else {
        const uint32_t e = (31 - __builtin_clz(l)) - 2;
        code = 261 + 4 * e + ((l >> e) & 3);
        ebits = e;
        eval = l & ((1u << e) - 1);
    }
}

// distance - 1 (0..32767) -> code 0..29, extra bits and their value
__host__ __device__ inline void fq_dist_code(uint32_t d, uint32_t& code, uint32_t& ebits, uint32_t& eval) {
    if (d < 4) {
        code = d, ebits = 0, eval = 0;
    } else {
        const uint32_t e = (31 - __builtin_clz(d)) - 1;
        code = 2 * e + 2 + ((d >> e) & 1);
        ebits = e;
        eval = d & ((1u << e) - 1);
    }
}

// The code lengths of both trees as the code-length alphabet's symbols (RFC 1951 3.2.7: 16 repeats
// the previous length 3..6 times, 17 / 18 are runs of 3..10 / 11..138 zeros), seq[i] = symbol |
// extra << 8, and the symbols' frequencies.  Returns the number of entries (<= hlit + hdist).
__host__ __device__ inline int fq_cl_sequence(const uint8_t* llen, int hlit, const uint8_t* dlen, int hdist, uint16_t* seq,
                                              uint32_t* clfreq) {
    for (int i = 0; i < FQ_DEFL_NCL; ++i) clfreq[i] = 0;
    const int total = hlit + hdist;
    int ns = 0;
    for (int i = 0; i < total;) {
        const int v = i < hlit ? llen[i] : dlen[i - hlit];
        int run = 1;
        while (i + run < total && (i + run < hlit ? llen[i + run] : dlen[i + run - hlit]) == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int r = run < 138 ? run : 138;
                seq[ns++] = (uint16_t)(18 | (r - 11) << 8);
                ++clfreq[18];
                run -= r;
            }
            if (run >= 3) {
                seq[ns++] = (uint16_t)(17 | (run - 3) << 8);
                ++clfreq[17];
                run = 0;
            }
        } else {
            seq[ns++] = (uint16_t)v;
            ++clfreq[v];
            --run;
            while (run >= 3) {
                const int r = run < 6 ? run : 6;
                seq[ns++] = (uint16_t)(16 | (r - 3) << 8);
                ++clfreq[16];
                run -= r;
            }
        }
        for (; run > 0; --run) {
            seq[ns++] = (uint16_t)v;
            ++clfreq[v];
        }
    }
    return ns;
}

// ---- the workgroup routine ----------------------------------------------------------------------
// bits ORed into the LDS image from a bit position on (32-bit words; neighbours share the words at
// their ends, hence the atomic OR)
struct fq_bitput {
    uint32_t* img;
    uint32_t word;
    uint32_t fill;
    uint64_t acc;
    __device__ inline void start(uint32_t* image, uint32_t bitpos) {
        img = image;
        word = bitpos >> 5;
        fill = bitpos & 31;
        acc = 0;
    }
    __device__ inline void put(uint32_t v, uint32_t nbits) {  // nbits <= 28
        acc |= (uint64_t)v << fill;
        fill += nbits;
        if (fill >= 32) {
            atomicOr(&img[word], (uint32_t)acc);
            ++word;
            acc >>= 32;
            fill -= 32;
        }
    }
    __device__ inline void flush() {
        if (fill) atomicOr(&img[word], (uint32_t)acc);
        fill = 0;
        acc = 0;
    }
};

__device__ inline uint32_t fq_defl_load4(const uint8_t* in, uint32_t p) {
    return (uint32_t)in[p] | (uint32_t)in[p + 1] << 8 | (uint32_t)in[p + 2] << 16 | (uint32_t)in[p + 3] << 24;
}

// candidate q for position p (v = the 4 bytes at p): the match length if it beats best
__device__ inline void fq_defl_try(const uint8_t* in, uint32_t p, uint32_t q, uint32_t v, uint32_t maxl, uint32_t& best_len,
                                   uint32_t& best_dist) {
    if (q >= p || p - q > FQ_DEFL_WINDOW) return;
    if (fq_defl_load4(in, q) != v) return;
    uint32_t l = 4;
    while (l < maxl && in[q + l] == in[p + l]) ++l;  // (maxl <= 255; q + l < p + l < the member's end)
    if (l > best_len || (l == best_len && p - q < best_dist)) best_len = l, best_dist = p - q;
}

// Compresses src[0, n) (0 < n <= 65280) into one BGZF member at dst (a FQ_DEFL_SLOT-byte slot)
// and returns its size (the same value in every thread).  tok: 65280 words of this workgroup's own.
__device__ inline uint32_t fq_deflate_member(uint8_t* lds, const uint8_t* src, uint32_t n, int level, uint32_t* tok,
                                             uint8_t* dst) {
    const uint32_t tid = threadIdx.x;
    uint8_t* in = lds + FQ_DL_IN;
    uint32_t* in32 = (uint32_t*)(lds + FQ_DL_IN);
    uint16_t* hash = (uint16_t*)(lds + FQ_DL_HASH);
    uint32_t* lfreq = (uint32_t*)(lds + FQ_DL_LFREQ);
    uint32_t* dfreq = (uint32_t*)(lds + FQ_DL_DFREQ);
    uint16_t* lcode = (uint16_t*)(lds + FQ_DL_LCODE);
    uint16_t* dcode = (uint16_t*)(lds + FQ_DL_DCODE);
    uint8_t* llen = lds + FQ_DL_LLEN;
    uint8_t* dlen = lds + FQ_DL_DLEN;
    uint32_t* clfreq = (uint32_t*)(lds + FQ_DL_CLFREQ);
    uint16_t* clcode = (uint16_t*)(lds + FQ_DL_CLCODE);
    uint8_t* cllen = lds + FQ_DL_CLLEN;
    uint16_t* seq = (uint16_t*)(lds + FQ_DL_SEQ);
    uint32_t* scan = (uint32_t*)(lds + FQ_DL_SCAN);
    uint32_t* misc = (uint32_t*)(lds + FQ_DL_MISC);

    __syncthreads();  // (the previous member's last LDS reads)
    // the input into LDS (16 bytes a thread where the source allows), the rest of the LDS cleared
    if (((uintptr_t)src & 15) == 0) {
        const uint32_t n16 = n >> 4;
        const uint4* s4 = (const uint4*)src;
        uint4* d4 = (uint4*)in;
        for (uint32_t i = tid; i < n16; i += FQ_DEFL_THREADS) d4[i] = s4[i];
        for (uint32_t i = (n16 << 4) + tid; i < n; i += FQ_DEFL_THREADS) in[i] = src[i];
    } else {
        for (uint32_t i = tid; i < n; i += FQ_DEFL_THREADS) in[i] = src[i];
    }
    if (tid < 16) in[n + tid] = 0;  // (n + 16 <= FQ_DL_IN_BYTES)
    for (uint32_t i = tid; i < (FQ_DL_TOTAL - FQ_DL_HASH) / 4; i += FQ_DEFL_THREADS) ((uint32_t*)(lds + FQ_DL_HASH))[i] = 0;
    __syncthreads();

    // 1. matches
    const uint32_t rounds = (n + FQ_DEFL_THREADS - 1) / FQ_DEFL_THREADS;
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t p = r * FQ_DEFL_THREADS + tid;
        const uint32_t cend = (p / FQ_DEFL_CHUNK + 1) * FQ_DEFL_CHUNK;
        const uint32_t limit = cend < n ? cend : n;  // matches end with the chunk
        const bool ins = p + 4 <= n;
        const bool look = p + FQ_DEFL_MIN_MATCH <= limit;
        uint32_t v = 0, h = 0, c1 = 0;
        if (ins) {
            v = fq_defl_load4(in, p);
            h = (v * 2654435761u) >> (32 - FQ_DEFL_HASH_BITS);
            c1 = hash[h];
        }
        __syncthreads();
        if (ins) hash[h] = (uint16_t)p;
        __syncthreads();
        if (p < n) {
            uint32_t best_len = 0, best_dist = 0;
            if (look) {
                const uint32_t maxl = limit - p;
                fq_defl_try(in, p, c1, v, maxl, best_len, best_dist);
                if (level >= 4) fq_defl_try(in, p, hash[h], v, maxl, best_len, best_dist);
                if (p > 0) fq_defl_try(in, p, p - 1, v, maxl, best_len, best_dist);
                // a short match far away costs more bits than its literals
                if ((best_len == 4 && best_dist > 1024) || (best_len == 5 && best_dist > 8192)) best_len = 0;
            }
            tok[p] = best_len ? (best_len << 16 | (best_dist - 1)) : 0;
        }
    }
    __syncthreads();

    // 2. parse this thread's chunk, tokens in place (token j is written at or before the position
    // being read), symbol counts into the histograms
    const uint32_t cs = tid * FQ_DEFL_CHUNK;
    const uint32_t ce = cs + FQ_DEFL_CHUNK < n ? cs + FQ_DEFL_CHUNK : n;
    uint32_t ntok = 0;
    {
        uint32_t p = cs;
        for (uint32_t it = 0; it < FQ_DEFL_CHUNK && p < ce; ++it) {
            const uint32_t m = tok[p];
            const uint32_t l = m >> 16;
            uint32_t t;
            if (l >= FQ_DEFL_MIN_MATCH && p + l <= ce) {
                uint32_t c, eb, ev;
                fq_len_code(l, c, eb, ev);
                atomicAdd(&lfreq[c], 1u);
                fq_dist_code(m & 0xffff, c, eb, ev);
                atomicAdd(&dfreq[c], 1u);
                t = m;
                p += l;
            } else {
                t = in[p];
                atomicAdd(&lfreq[t], 1u);
                p += 1;
            }
            tok[cs + ntok] = t;
            ++ntok;
        }
    }
    if (tid == 0) atomicAdd(&lfreq[256], 1u);
    // 5. CRC32 of the chunk, moved to its place in the member
    if (cs < n) {
        const uint32_t c = fq_crc_bytes(in + cs, ce - cs);
        atomicXor(&misc[FQ_DM_CRC], fq_crc_mul(fq_crc_xpow8(n - ce), c));
    }
    __syncthreads();

    // 3. code lengths and codes: literal/length tree (thread 0), distance tree (thread 64)
    if (tid == 0) {
        if (fq_huff_code_lengths(lfreq, FQ_DEFL_NLIT, 15, llen, (uint32_t*)(lds + FQ_DL_HASH)) != 0) misc[FQ_DM_BAD] = 1;
        fq_huff_codes(llen, FQ_DEFL_NLIT, lcode);
    }
    if (tid == 64) {
        // (as zlib: at least two distance codes, so the tree is complete for every inflater)
        int used = 0;
        for (int i = 0; i < FQ_DEFL_NDIST; ++i) used += dfreq[i] != 0;
        if (used < 2) {
            if (!dfreq[0]) dfreq[0] = 1, ++used;
            if (used < 2) dfreq[1] = 1;
        }
        if (fq_huff_code_lengths(dfreq, FQ_DEFL_NDIST, 15, dlen, (uint32_t*)(lds + FQ_DL_HASH + 5120)) != 0)
            misc[FQ_DM_BAD] = 1;
        fq_huff_codes(dlen, FQ_DEFL_NDIST, dcode);
    }
    __syncthreads();
    if (tid == 0) {
        int hlit = FQ_DEFL_NLIT, hdist = FQ_DEFL_NDIST;
        while (hlit > 257 && !llen[hlit - 1]) --hlit;
        while (hdist > 1 && !dlen[hdist - 1]) --hdist;
        const int ns = fq_cl_sequence(llen, hlit, dlen, hdist, seq, clfreq);
        int used = 0;
        for (int i = 0; i < FQ_DEFL_NCL; ++i) used += clfreq[i] != 0;
        if (used < 2) clfreq[clfreq[0] ? 18 : 0] = 1;
        if (fq_huff_code_lengths(clfreq, FQ_DEFL_NCL, 7, cllen, (uint32_t*)(lds + FQ_DL_HASH)) != 0) misc[FQ_DM_BAD] = 1;
        fq_huff_codes(cllen, FQ_DEFL_NCL, clcode);
        const uint8_t order[FQ_DEFL_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int hclen = FQ_DEFL_NCL;
        while (hclen > 4 && !cllen[order[hclen - 1]]) --hclen;
        uint32_t hbits = 3 + 5 + 5 + 4 + 3 * hclen;
        for (int i = 0; i < ns; ++i) {
            const uint32_t s = seq[i] & 0xff;
            hbits += cllen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
        }
        misc[FQ_DM_HBITS] = hbits;
        misc[FQ_DM_HLIT] = hlit;
        misc[FQ_DM_HDIST] = hdist;
        misc[FQ_DM_HCLEN] = hclen;
        misc[FQ_DM_NSEQ] = ns;
    }
    // 4. bit lengths of this thread's tokens, prefix sum
    // (llen / dlen are final since the barrier above; thread 0 only reads them)
    uint32_t bits = 0;
    for (uint32_t j = 0; j < ntok; ++j) {
        const uint32_t t = tok[cs + j];
        if (t >> 16) {
            uint32_t c, eb, ev;
            fq_len_code(t >> 16, c, eb, ev);
            bits += llen[c] + eb;
            fq_dist_code(t & 0xffff, c, eb, ev);
            bits += dlen[c] + eb;
        } else {
            bits += llen[t];
        }
    }
    scan[tid] = bits;
    __syncthreads();
    for (uint32_t off = 1; off < FQ_DEFL_THREADS; off <<= 1) {
        const uint32_t a = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += a;
        __syncthreads();
    }
    const uint32_t hbits = misc[FQ_DM_HBITS];
    const uint32_t total_bits = hbits + scan[FQ_DEFL_THREADS - 1] + llen[256];
    const uint32_t dyn_bytes = (total_bits + 7) >> 3;
    const uint32_t crc = misc[FQ_DM_CRC];
    const bool stored = misc[FQ_DM_BAD] != 0 || dyn_bytes >= n + 5;  // (so dyn_bytes <= 65284 < 65536 - 26)
    const uint32_t payload = stored ? n + 5 : dyn_bytes;
    const uint32_t member = 18 + payload + 8;
    const uint32_t mybit = hbits + scan[tid] - bits;
    __syncthreads();
    if (stored) {
        if (tid < 5) {
            const uint32_t nl = n & 0xffff, nn = ~n & 0xffff;
            const uint8_t hd[5] = {1, (uint8_t)nl, (uint8_t)(nl >> 8), (uint8_t)nn, (uint8_t)(nn >> 8)};
            dst[18 + tid] = hd[tid];
        }
        for (uint32_t i = tid; i < n; i += FQ_DEFL_THREADS) dst[23 + i] = in[i];
    } else {
        const uint32_t words = (dyn_bytes + 3) / 4 + 1;  // (<= FQ_DL_IN_BYTES / 4)
        for (uint32_t i = tid; i < words; i += FQ_DEFL_THREADS) in32[i] = 0;
        __syncthreads();
        fq_bitput bp;
        if (tid == 0) {
            bp.start(in32, 0);
            bp.put(1, 1);  // BFINAL
            bp.put(2, 2);  // dynamic Huffman
            const int hclen = (int)misc[FQ_DM_HCLEN];
            bp.put(misc[FQ_DM_HLIT] - 257, 5);
            bp.put(misc[FQ_DM_HDIST] - 1, 5);
            bp.put(hclen - 4, 4);
            const uint8_t order[FQ_DEFL_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            for (int i = 0; i < hclen; ++i) bp.put(cllen[order[i]], 3);
            const int ns = (int)misc[FQ_DM_NSEQ];
            for (int i = 0; i < ns; ++i) {
                const uint32_t s = seq[i] & 0xff, x = seq[i] >> 8;
                bp.put(clcode[s], cllen[s]);
                if (s >= 16) bp.put(x, s == 16 ? 2 : s == 17 ? 3 : 7);
            }
            // (the header ends at bit hbits = this thread's token offset)
        } else {
            bp.start(in32, mybit);
        }
        for (uint32_t j = 0; j < ntok; ++j) {
            const uint32_t t = tok[cs + j];
            if (t >> 16) {
                uint32_t c, eb, ev;
                fq_len_code(t >> 16, c, eb, ev);
                bp.put(lcode[c] | ev << llen[c], llen[c] + eb);
                fq_dist_code(t & 0xffff, c, eb, ev);
                bp.put(dcode[c] | ev << dlen[c], dlen[c] + eb);
            } else {
                bp.put(lcode[t], llen[t]);
            }
        }
        if (tid == FQ_DEFL_THREADS - 1) bp.put(lcode[256], llen[256]);  // (empty chunks start at the tokens' end)
        bp.flush();
        __syncthreads();
        for (uint32_t i = tid; i < dyn_bytes; i += FQ_DEFL_THREADS) dst[18 + i] = in[i];
    }
    if (tid < 18) {
        const uint32_t bs = member - 1;
        const uint8_t hd[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 4, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bs, (uint8_t)(bs >> 8)};
        dst[tid] = hd[tid];
    }
    if (tid >= 32 && tid < 40) {
        const uint32_t k = tid - 32;
        dst[18 + payload + k] = (uint8_t)((k < 4 ? crc : n) >> (8 * (k & 3)));
    }
    return member;
}

// ---- compaction -------------------------------------------------------------------------------------
// Moves member g (scratch slot g, sizes[g] bytes) to its place in its stream: dst + the sizes of the
// slots [first, g), first being the slot of the stream's first member.  Returns the stream offset
// past the member (the same value in every thread).  A member that would not fit dst_cap (or whose
// size is no member's) is not written.  part: 256 words of the workgroup's LDS.
__device__ inline unsigned long long fq_compact_member(unsigned long long* part, const uint8_t* slots, const uint32_t* sizes,
                                                       unsigned long long first, unsigned long long g, uint8_t* dst,
                                                       unsigned long long dst_cap) {
    const uint32_t tid = threadIdx.x;
    unsigned long long sum = 0;
    for (unsigned long long i = first + tid; i < g; i += 256) sum += sizes[i];
    part[tid] = sum;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    const unsigned long long off = part[0];
    __syncthreads();
    const uint32_t sz = sizes[g];
    const uint8_t* src = slots + g * FQ_DEFL_SLOT;
    if (sz <= FQ_DEFL_SLOT && off + sz <= dst_cap) {
        // 4 bytes a thread once the destination is aligned (the slot is; the stream offset is not)
        const uint32_t lead = (uint32_t)((4 - ((uintptr_t)(dst + off) & 3)) & 3);
        const uint32_t head = sz < lead ? sz : lead;
        if (tid < head) dst[off + tid] = src[tid];
        const uint32_t words = (sz - head) / 4;
        uint32_t* d4 = (uint32_t*)(dst + off + head);
        for (uint32_t i = tid; i < words; i += 256) {
            const uint8_t* q = src + head + 4 * i;
            d4[i] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        }
        const uint32_t done = head + 4 * words;
        if (tid < sz - done) dst[off + done + tid] = src[done + tid];
    }
    return off + sz;
}

// ---- several spans by one launch: the two walks ----------------------------------------------------
// members: the slots the scratch holds.  A member beyond them is skipped by both walks, and the
// compaction then compacts nothing at all, writes 0 for every total and sets bit 1 of *err, so that
// nothing of a pack with a skipped member is ever taken for a stream.
struct fq_span_table {
    uint8_t* text[FQ_DEFL_SPANS];                // the text in, the stream out (fq_deflate_bound(cap) bytes)
    const unsigned long long* n[FQ_DEFL_SPANS];  // its length word (null: no such span)
    unsigned long long cap[FQ_DEFL_SPANS];
};

__device__ inline void fq_span_layout(const fq_span_table& t, fq_defl_layout& L) {
    unsigned long long n[FQ_DEFL_SPANS], cap[FQ_DEFL_SPANS];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < FQ_DEFL_SPANS; ++k) {
        n[k] = t.n[k] ? *t.n[k] : 0;
        cap[k] = t.n[k] ? t.cap[k] : 0;
    }
    fq_defl_spans_layout(n, cap, L);
}

__device__ inline uint8_t* fq_span_text(const fq_span_table& t, int span) {
    uint8_t* p = nullptr;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < FQ_DEFL_SPANS; ++k) p = k == span ? t.text[k] : p;
    return p;
}

// workgroup `block` of `nblocks`: its members compressed into their slots (lds: FQ_DL_TOTAL bytes,
// tok: this workgroup's token array)
__device__ inline void fq_deflate_spans_walk(uint8_t* lds, const fq_span_table& t, unsigned long long members, int level,
                                             uint32_t* tok, uint8_t* slots, uint32_t* sizes, unsigned block, unsigned nblocks) {
    fq_defl_layout L;
    fq_span_layout(t, L);
    // (32-bit indices: the slots' bytes, 64 KiB each, bound their count far below 2^32)
    const uint32_t nmem = (uint32_t)(L.base[FQ_DEFL_SPANS] < members ? L.base[FQ_DEFL_SPANS] : members);
    for (uint32_t g = block; g < nmem; g += nblocks) {
        // (the layout is derived anew per member: six scalar loads, instead of its 13 words kept in
        // registers across the member routine, which spilled scalar registers)
        fq_span_layout(t, L);
        const fq_defl_place p = fq_defl_spans_place(L, g);
        const uint32_t sz = fq_deflate_member(lds, fq_span_text(t, p.span) + p.at, p.len, level, tok,
                                              slots + (size_t)g * FQ_DEFL_SLOT);
        if (threadIdx.x == 0) sizes[g] = sz;
    }
}

// ... its members moved to their streams, each span's total written by the workgroup that moves
// its last member (an empty or absent span's by workgroup 0); part: 256 words of LDS
__device__ inline void fq_compact_spans_walk(unsigned long long* part, const fq_span_table& t, unsigned long long members,
                                             const uint8_t* slots, const uint32_t* sizes, unsigned long long* totals, int* err,
                                             unsigned block, unsigned nblocks) {
    const uint32_t tid = threadIdx.x;
    fq_defl_layout L;
    fq_span_layout(t, L);
    const unsigned long long nmem = L.base[FQ_DEFL_SPANS];
    const bool over = nmem > members;
    if (block == 0 && tid == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < FQ_DEFL_SPANS; ++k)
            if (over || L.len[k] == 0) totals[k] = 0;
        if (over && err) atomicOr(err, 2);
    }
    if (over) return;
    for (unsigned long long g = block; g < nmem; g += nblocks) {
        const fq_defl_place p = fq_defl_spans_place(L, g);
        unsigned long long cap = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < FQ_DEFL_SPANS; ++k) cap = k == p.span ? t.cap[k] : cap;
        // (the span's buffer: fq_deflate_bound(cap))
        const unsigned long long dst_cap = cap + 31 * ((cap + FQ_DEFL_MEMBER_IN - 1) / FQ_DEFL_MEMBER_IN);
        const unsigned long long end = fq_compact_member(part, slots, sizes, p.first, g, fq_span_text(t, p.span), dst_cap);
        if (p.last && tid == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 0; k < FQ_DEFL_SPANS; ++k)
                if (k == p.span) totals[k] = end;
        }
    }
}
