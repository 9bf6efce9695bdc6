// inflate_core.h -- the BGZF member inflater of inflate.hip (RFC 1951 in full: stored, fixed and
// dynamic blocks), written once for the device and for the host simulation
// (tools/micro/inflate_sim.cpp, which runs this text under AddressSanitizer).
//
// One wave64 inflates one member (payload and output both <= 64 KiB).  The routine is a wave
// program: everything outside an FQ_LANES block is wave-uniform (the bit buffer, the positions, the
// decoded symbols: the compiler keeps them in SGPRs), and the lane-parallel parts (window loads,
// table fills, literal runs, match copies, CRC, copy-out) stand in FQ_LANES blocks.  On the device
// FQ_LANES(l) runs its body once with l = the lane; the simulation defines it as a loop over the 64
// lanes.  The two agree because no FQ_LANES block reads a byte that another lane writes in the same
// block (match copies are cut so that a step's sources all lie before its destinations).
//
// Where things live:
//   input    read from device memory 256 bytes at a time, 4 bytes a lane, into one VGPR (the
//            window); the bit buffer takes its 32-bit words from it with v_readlane, so a refill
//            costs no memory round trip.  Bytes at or past in_len read as zero, and consuming any
//            of them is a data error.
//   output   the last 32 KiB (deflate's largest distance) in LDS, as a ring: a match copy is an LDS
//            read and an LDS write of the same wave, ordered by fq_wave_sync, and whenever the ring
//            holds 16 KiB that device memory does not have yet, those bytes are written out,
//            coalesced, and their CRC32 is taken on the way.  With the tables that is ~38 KiB a wave:
//            four waves a CU, one per SIMD, 1024 members in flight on the chip (a 64 MB batch has
//            ~1000).
//   tables   per wave in LDS: a 10-bit first-level table for the literal/length code and one for the
//            distance code (symbol | length << 9; 0 = not a short code), and for the longer codes
//            the canonical-order symbol list with the per-length counts (the spill: walked bit by
//            bit, at most 15 steps).
//
// Hostile input: every read of `in` is guarded by in_len, every write of the output by isize, every
// distance by the bytes produced so far; code-length sets are checked (Kraft sum) before a table is
// filled; every loop iteration consumes at least one input bit or produces at least one output byte,
// and running past the input ends the member, so a member ends in bounded time.
#pragma once
#include <stdint.h>

#include "crc_core.h"

#define FQ_INFLATE_MAX_BYTES 65536u
#define FQ_INFL_ROOT 10u        // first-level bits of the literal/length and distance tables
#define FQ_INFL_CLROOT 7u       // the code-length code is at most 7 bits: its table is complete
#define FQ_INFL_NOSYM 0xffffu

enum { FQ_IS_OK = 0, FQ_IS_DATA = 1, FQ_IS_LONG = 2, FQ_IS_SHORT = 3, FQ_IS_CRC = 4 };

// ---- LDS layout (bytes), one wave ----------------------------------------------------------
#define FQ_INFL_WIN 32768u                            // the output window: deflate's largest distance
#define FQ_INFL_DRAIN 16384u                          // the window goes to device memory when it holds this much
#define FQ_IL_OUT 0                                   // the last FQ_INFL_WIN bytes of output, a ring
#define FQ_IL_LTAB (FQ_IL_OUT + FQ_INFL_WIN)          // u16[1024]
#define FQ_IL_DTAB (FQ_IL_LTAB + 2048)                // u16[1024]
#define FQ_IL_CLTAB (FQ_IL_DTAB + 2048)               // u16[128]
#define FQ_IL_LENS (FQ_IL_CLTAB + 256)                // u8[320]: literal/length lengths, then distance
#define FQ_IL_LSORT (FQ_IL_LENS + 320)                // u16[288]
#define FQ_IL_DSORT (FQ_IL_LSORT + 576)               // u16[32]
#define FQ_IL_CLSORT (FQ_IL_DSORT + 64)               // u16[32]
#define FQ_IL_LCNT (FQ_IL_CLSORT + 64)                // u32[16]
#define FQ_IL_DCNT (FQ_IL_LCNT + 64)                  // u32[16]
#define FQ_IL_CLCNT (FQ_IL_DCNT + 64)                 // u32[16]
#define FQ_IL_FIRST (FQ_IL_CLCNT + 64)                // u32[32]: first code, first list index per length
#define FQ_IL_CLLEN (FQ_IL_FIRST + 128)               // u8[32]
#define FQ_IL_TOTAL (FQ_IL_CLLEN + 32)
static_assert(4 * FQ_IL_TOTAL <= 160 * 1024, "four inflate waves per CU: one per SIMD");

// ---- the cross-lane operations (the simulation defines its own before including this) -------
#ifndef FQ_INFL_HOST_SIM
#define FQ_LANES(l) for (uint32_t l = threadIdx.x & 63u, fq_once_ = 1; fq_once_; fq_once_ = 0)
#define FQ_LANEVAR(T, name) T name
#define FQ_LV(name, l) (*((void)(l), &(name)))
// lane k's value of a lane variable (k wave-uniform)
#define FQ_LANE_GET(name, k) ((uint32_t)__builtin_amdgcn_readlane((int)(name), (int)(k)))
// a value that is the same in every lane, moved to a scalar register
__device__ inline uint32_t fq_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// orders the wave's LDS and device-memory accesses: what any lane wrote before is visible to every
// lane after (the workgroup is this one wave)
__device__ inline void fq_wave_sync() { __syncthreads(); }
__device__ inline uint32_t fq_wave_xor(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o, 64);
    return fq_uni(v);
}
__device__ inline void fq_lds_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
#endif

// ---- bit reader ----------------------------------------------------------------------------
struct fq_infl_rd {
    const uint8_t* in;
    uint32_t in_len;
    uint32_t wbase;  // payload offset of the window's first byte
    uint32_t next;   // payload offset of the next 32-bit word the bit buffer takes
    uint64_t bb;     // bit buffer, the next bit in bit 0
    uint32_t bc;     // bits in it
    FQ_LANEVAR(uint32_t, win);  // bytes [wbase + 4 * lane, + 4) of the payload, zero past in_len
};

// the next word to take is at payload offset pos (the bit buffer empty, the window reloaded)
__device__ inline void fq_infl_seek(fq_infl_rd& r, uint32_t pos) {
    r.next = pos;
    r.wbase = pos - 256u;
    r.bb = 0;
    r.bc = 0;
}

// at least 32 bits in the buffer
__device__ inline void fq_infl_fill(fq_infl_rd& r) {
    if (r.bc >= 32) return;
    if (r.next - r.wbase >= 256u) {
        r.wbase = r.next;
        FQ_LANES(l) {
            const uint32_t p = r.wbase + 4 * l;
            uint32_t w = 0;
            for (uint32_t k = 0; k < 4; ++k)
                if (p + k < r.in_len) w |= (uint32_t)r.in[p + k] << (8 * k);
            FQ_LV(r.win, l) = w;
        }
    }
    const uint32_t w = FQ_LANE_GET(r.win, (r.next - r.wbase) >> 2);
    r.bb |= (uint64_t)w << r.bc;
    r.bc += 32;
    r.next += 4;
}

__device__ inline uint32_t fq_infl_bits(fq_infl_rd& r, uint32_t n) {  // n <= 16 <= bc
    const uint32_t v = (uint32_t)r.bb & ((1u << n) - 1);
    r.bb >>= n;
    r.bc -= n;
    return v;
}

// bits were consumed that the payload does not have
__device__ inline bool fq_infl_overrun(const fq_infl_rd& r) { return r.next * 8 - r.bc > r.in_len * 8; }

// ---- code tables ---------------------------------------------------------------------------
// The decoding tables of the code whose lengths are lens[0, n) (each <= 15): cnt[len] = codes of
// that length, sorted[] = the symbols in canonical order, tab[1 << root] = the first-level table.
// Returns 1, with no table usable, when the set is over-subscribed, or incomplete (unless few_ok
// and it has no code at all, or one code of length 1: the distance code's exceptions).
__device__ inline int fq_infl_build(const uint8_t* lens, uint32_t n, uint32_t root, bool few_ok, uint16_t* tab, uint32_t* cnt,
                                    uint16_t* sorted, uint32_t* first) {
    fq_wave_sync();  // (the lengths written, the old tables no longer read)
    FQ_LANES(l) {
        if (l < 16) cnt[l] = 0;
        for (uint32_t i = l; i < (1u << root) / 2; i += 64) ((uint32_t*)tab)[i] = 0;
    }
    fq_wave_sync();
    FQ_LANES(l) {
        for (uint32_t s = l; s < n; s += 64) {
            const uint32_t v = lens[s];
            if (v) fq_lds_add(&cnt[v], 1u);
        }
    }
    fq_wave_sync();
    int32_t left = 1;
    uint32_t code = 0, off = 0;
    for (uint32_t len = 1; len <= 15; ++len) {
        const uint32_t c = fq_uni(cnt[len]);
        left = (left << 1) - (int32_t)c;
        if (left < 0) return 1;  // over-subscribed
        FQ_LANES(l) {
            if (l == 0) {
                first[len] = code;
                first[16 + len] = off;
            }
        }
        code = (code + c) << 1;
        off += c;
    }
    if (left > 0 && !(few_ok && (off == 0 || (off == 1 && fq_uni(cnt[1]) == 1)))) return 1;  // incomplete
    fq_wave_sync();
    FQ_LANES(l) {
        for (uint32_t s = l; s < n; s += 64) {
            const uint32_t v = lens[s];
            if (!v) continue;
            uint32_t rank = 0;  // symbols before s with the same length
            for (uint32_t i = 0; i < s; ++i) rank += lens[i] == v;
            const uint32_t c = first[v] + rank;
            sorted[first[16 + v] + rank] = (uint16_t)s;  // (< the number of used symbols <= n)
            if (v <= root) {
                uint32_t rev = 0;
                for (uint32_t b = 0; b < v; ++b) rev |= ((c >> b) & 1u) << (v - 1 - b);
                // (codes of a set that passed the Kraft check are prefix-free: no entry is written twice)
                for (uint32_t j = rev; j < (1u << root); j += 1u << v) tab[j] = (uint16_t)(s | v << 9);
            }
        }
    }
    fq_wave_sync();
    return 0;
}

// the next symbol (needs 15 bits in the buffer; consumes 1..15), FQ_INFL_NOSYM for bits that are no code
__device__ inline uint32_t fq_infl_sym(fq_infl_rd& r, const uint16_t* tab, uint32_t root, const uint32_t* cnt,
                                       const uint16_t* sorted) {
    const uint32_t e = fq_uni(tab[(uint32_t)r.bb & ((1u << root) - 1)]);
    if (e) {
        fq_infl_bits(r, e >> 9);
        return e & 511u;
    }
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= 15; ++len) {
        code |= (uint32_t)(r.bb >> (len - 1)) & 1u;
        const uint32_t c = fq_uni(cnt[len]);
        if (code >= first && code - first < c) {
            fq_infl_bits(r, len);
            return fq_uni(sorted[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    fq_infl_bits(r, 15);
    return FQ_INFL_NOSYM;
}

// ---- the member routine -----------------------------------------------------------------------
// Inflates in[0, in_len) (in_len, isize <= 65536) into dst[0, produced), produced <= isize, and
// returns the FQ_IS_* status (the first failure met): the same values in every lane.
// lds: FQ_IL_TOTAL bytes of this wave's own, 16-byte aligned.
__device__ inline uint32_t fq_inflate_one(uint8_t* lds, const uint8_t* in, uint32_t in_len, uint32_t isize, uint32_t crc,
                                             uint8_t* dst, uint32_t& produced) {
    uint8_t* out = lds + FQ_IL_OUT;
    uint16_t* ltab = (uint16_t*)(lds + FQ_IL_LTAB);
    uint16_t* dtab = (uint16_t*)(lds + FQ_IL_DTAB);
    uint16_t* cltab = (uint16_t*)(lds + FQ_IL_CLTAB);
    uint8_t* lens = lds + FQ_IL_LENS;
    uint16_t* lsort = (uint16_t*)(lds + FQ_IL_LSORT);
    uint16_t* dsort = (uint16_t*)(lds + FQ_IL_DSORT);
    uint16_t* clsort = (uint16_t*)(lds + FQ_IL_CLSORT);
    uint32_t* lcnt = (uint32_t*)(lds + FQ_IL_LCNT);
    uint32_t* dcnt = (uint32_t*)(lds + FQ_IL_DCNT);
    uint32_t* clcnt = (uint32_t*)(lds + FQ_IL_CLCNT);
    uint32_t* first = (uint32_t*)(lds + FQ_IL_FIRST);
    uint8_t* cllen = lds + FQ_IL_CLLEN;

    fq_wave_sync();  // (the previous member's last LDS reads)
    fq_infl_rd r;
    r.in = in;
    r.in_len = in_len;
    FQ_LANES(l) { FQ_LV(r.win, l) = 0; }
    fq_infl_seek(r, 0);
    uint32_t st = FQ_IS_OK;
    const uint32_t wm = FQ_INFL_WIN - 1;
    uint32_t pos = 0;             // bytes of output produced: byte p is out[p & wm] while pos - p <= FQ_INFL_WIN
    uint32_t drained = 0;         // of which in device memory (pos - drained stays below FQ_INFL_WIN - 322)
    uint32_t nlit = 0;            // literals waiting in lit (lane k holds the k-th)
    FQ_LANEVAR(uint32_t, lit);
    FQ_LANEVAR(uint32_t, crcacc);  // this lane's share of the CRC32 of dst[0, drained)
    FQ_LANES(l) {
        FQ_LV(lit, l) = 0;
        FQ_LV(crcacc, l) = 0;
    }

// out[drained, pos) to device memory, its CRC32 into crcacc: each lane sums its own run of the bytes
// (an odd number of them, so that the lanes' LDS reads spread over the banks), bitwise, and moves the
// sum to its place in a member of isize bytes (crc_core.h), which is what it is worth if the member
// turns out to be isize bytes long; otherwise nobody looks at it
#ifndef FQ_INFL_NO_CRC  // (profiling only: the kernel's time without the CRC32)
#define FQ_INFL_CRC_PART()                                                                       \
    do {                                                                                         \
        const uint32_t chunk = ((pos - drained + 63) / 64) | 1u;                                 \
        FQ_LANES(l) {                                                                            \
            const uint32_t cs = drained + l * chunk;                                             \
            if (cs < pos) {                                                                      \
                const uint32_t ce = cs + chunk < pos ? cs + chunk : pos;                         \
                uint32_t c = 0xffffffffu;                                                        \
                for (uint32_t i = cs; i < ce; ++i) {                                             \
                    c ^= out[i & wm];                                                            \
                    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1))); \
                }                                                                                \
                if (ce <= isize) FQ_LV(crcacc, l) ^= fq_crc_mul(fq_crc_xpow8(isize - ce), ~c);   \
            }                                                                                    \
        }                                                                                        \
    } while (0)
#else
#define FQ_INFL_CRC_PART() do { } while (0)
#endif
#define FQ_INFL_DRAIN_ALL()                                                              \
    do {                                                                                 \
        fq_wave_sync();                                                                  \
        FQ_INFL_CRC_PART();                                                              \
        FQ_LANES(l) {                                                                    \
            for (uint32_t i = drained + l; i < pos; i += 64) dst[i] = out[i & wm];       \
        }                                                                                \
        drained = pos;                                                                   \
        fq_wave_sync();                                                                  \
    } while (0)
// the waiting literals into the window (after which a match of 258 bytes still fits it)
#define FQ_INFL_FLUSH()                                                  \
    do {                                                                 \
        if (pos - drained >= FQ_INFL_DRAIN) FQ_INFL_DRAIN_ALL();         \
        FQ_LANES(l) {                                                    \
            if (l < nlit) out[(pos + l) & wm] = (uint8_t)FQ_LV(lit, l);  \
        }                                                                \
        pos += nlit;                                                     \
        nlit = 0;                                                        \
    } while (0)

    for (;;) {  // blocks (each consumes at least 3 bits)
        fq_infl_fill(r);
        const uint32_t bfinal = fq_infl_bits(r, 1);
        const uint32_t type = fq_infl_bits(r, 2);
        if (fq_infl_overrun(r) || type == 3) {
            st = FQ_IS_DATA;
            break;
        }
        if (type == 0) {
            fq_infl_bits(r, r.bc & 7);  // to the byte boundary
            fq_infl_fill(r);
            const uint32_t len = fq_infl_bits(r, 16);
            const uint32_t nlen = fq_infl_bits(r, 16);
            const uint32_t at = r.next - (r.bc >> 3);  // payload offset of the block's bytes
            if (fq_infl_overrun(r) || len != (~nlen & 0xffffu) || at + len > in_len) {
                st = FQ_IS_DATA;
                break;
            }
            FQ_INFL_FLUSH();
            if (pos + len > isize) {
                st = FQ_IS_LONG;
                break;
            }
            for (uint32_t done = 0; done < len;) {  // through the window, a drain's worth at a time
                if (pos - drained >= FQ_INFL_DRAIN) FQ_INFL_DRAIN_ALL();
                const uint32_t step = len - done < FQ_INFL_DRAIN ? len - done : FQ_INFL_DRAIN;
                FQ_LANES(l) {
                    for (uint32_t i = l; i < step; i += 64) out[(pos + i) & wm] = in[at + done + i];
                }
                pos += step;
                done += step;
            }
            fq_infl_seek(r, at + len);
        } else {
            uint32_t nl, nd;
            if (type == 1) {
                nl = 288;
                nd = 32;
                fq_wave_sync();  // (the tables' last readers)
                FQ_LANES(l) {
                    for (uint32_t s = l; s < 320; s += 64) lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
                }
            } else {
                fq_infl_fill(r);
                nl = fq_infl_bits(r, 5) + 257;
                nd = fq_infl_bits(r, 5) + 1;
                const uint32_t ncl = fq_infl_bits(r, 4) + 4;
                if (nl > 286 || nd > 30) {
                    st = FQ_IS_DATA;
                    break;
                }
                fq_wave_sync();
                FQ_LANES(l) {
                    if (l < 32) cllen[l] = 0;
                }
                fq_wave_sync();
                // the code-length code's lengths come in this order, 5 bits each here:
                // 16 17 18 0 8 7 9 6 10 5 11 4 | 12 3 13 2 14 1 15
                const uint64_t ord_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 |
                                        6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
                const uint64_t ord_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
                for (uint32_t i = 0; i < ncl; ++i) {
                    fq_infl_fill(r);
                    const uint32_t v = fq_infl_bits(r, 3);
                    const uint32_t o = (uint32_t)(i < 12 ? ord_lo >> (5 * i) : ord_hi >> (5 * (i - 12))) & 31u;
                    FQ_LANES(l) {
                        if (l == 0) cllen[o] = (uint8_t)v;
                    }
                }
                if (fq_infl_overrun(r) || fq_infl_build(cllen, 19, FQ_INFL_CLROOT, false, cltab, clcnt, clsort, first)) {
                    st = FQ_IS_DATA;
                    break;
                }
                const uint32_t total = nl + nd;
                uint32_t i = 0, prev = 0;
                while (i < total) {  // (each turn consumes at least one bit)
                    fq_infl_fill(r);
                    const uint32_t s = fq_infl_sym(r, cltab, FQ_INFL_CLROOT, clcnt, clsort);
                    if (fq_infl_overrun(r) || s > 18) {
                        st = FQ_IS_DATA;
                        break;
                    }
                    uint32_t rep = 1, val = s;
                    if (s == 16) {
                        if (i == 0) {
                            st = FQ_IS_DATA;
                            break;
                        }
                        rep = 3 + fq_infl_bits(r, 2);
                        val = prev;
                    } else if (s == 17) {
                        rep = 3 + fq_infl_bits(r, 3);
                        val = 0;
                    } else if (s == 18) {
                        rep = 11 + fq_infl_bits(r, 7);
                        val = 0;
                    }
                    if (i + rep > total) {
                        st = FQ_IS_DATA;
                        break;
                    }
                    FQ_LANES(l) {
                        for (uint32_t k = l; k < rep; k += 64) lens[i + k] = (uint8_t)val;
                    }
                    i += rep;
                    prev = val;
                }
                if (st != FQ_IS_OK) break;
                if (fq_infl_overrun(r)) {
                    st = FQ_IS_DATA;
                    break;
                }
            }
            if (fq_infl_build(lens, nl, FQ_INFL_ROOT, false, ltab, lcnt, lsort, first) || fq_uni(lens[256]) == 0 ||
                fq_infl_build(lens + nl, nd, FQ_INFL_ROOT, true, dtab, dcnt, dsort, first)) {
                st = FQ_IS_DATA;
                break;
            }
            for (;;) {  // symbols (each turn consumes at least one bit)
                fq_infl_fill(r);
                const uint32_t s = fq_infl_sym(r, ltab, FQ_INFL_ROOT, lcnt, lsort);
                if (fq_infl_overrun(r)) {
                    st = FQ_IS_DATA;
                    break;
                }
                if (s < 256) {
                    if (pos + nlit >= isize) {
                        st = FQ_IS_LONG;
                        break;
                    }
                    FQ_LANES(l) {
                        if (l == nlit) FQ_LV(lit, l) = s;
                    }
                    if (++nlit == 64) FQ_INFL_FLUSH();
                    continue;
                }
                if (s == 256) break;
                if (s > 285) {  // 286, 287, or no code
                    st = FQ_IS_DATA;
                    break;
                }
                const uint32_t lc = s - 257;
                uint32_t len;
                if (lc < 8) {
                    len = 3 + lc;
                } else if (lc == 28) {
                    len = 258;
                } else {
                    const uint32_t e = (lc >> 2) - 1;
                    len = 3 + ((4 + (lc & 3)) << e) + fq_infl_bits(r, e);
                }
                fq_infl_fill(r);
                const uint32_t dc = fq_infl_sym(r, dtab, FQ_INFL_ROOT, dcnt, dsort);
                if (dc > 29) {  // 30, 31, or no code
                    st = FQ_IS_DATA;
                    break;
                }
                uint32_t dist;
                if (dc < 4) {
                    dist = 1 + dc;
                } else {
                    const uint32_t e = (dc >> 1) - 1;
                    dist = 1 + ((2 + (dc & 1)) << e) + fq_infl_bits(r, e);
                }
                if (fq_infl_overrun(r)) {
                    st = FQ_IS_DATA;
                    break;
                }
                FQ_INFL_FLUSH();
                if (dist > pos) {
                    st = FQ_IS_DATA;
                    break;
                }
                if (pos + len > isize) {
                    st = FQ_IS_LONG;
                    break;
                }
                const uint32_t from = pos - dist;
                if (dist >= len || dist >= 64) {
                    // a step's 64 sources end before its first destination
                    for (uint32_t c = 0; c < len; c += 64) {
                        fq_wave_sync();
                        FQ_LANES(l) {
                            if (c + l < len) out[(pos + c + l) & wm] = out[(from + c + l) & wm];
                        }
                    }
                } else {
                    // the period out[from, pos) repeated: every source lies before pos
                    fq_wave_sync();
                    FQ_LANES(l) {
                        for (uint32_t i = l; i < len; i += 64) out[(pos + i) & wm] = out[(from + i % dist) & wm];
                    }
                }
                pos += len;
            }
            if (st != FQ_IS_OK) break;
        }
        if (bfinal) break;
    }
    FQ_INFL_FLUSH();
    FQ_INFL_DRAIN_ALL();
#undef FQ_INFL_FLUSH
#undef FQ_INFL_DRAIN_ALL
#undef FQ_INFL_CRC_PART
    if (st == FQ_IS_OK && pos != isize) st = FQ_IS_SHORT;  // (pos <= isize always)
#ifndef FQ_INFL_NO_CRC
    if (st == FQ_IS_OK) {
        uint32_t x = 0;
        FQ_LANES(l) { x ^= FQ_LV(crcacc, l); }
        x = fq_wave_xor(x);
        if (x != crc) st = FQ_IS_CRC;
    }
#endif
    produced = pos;
    return st;
}
