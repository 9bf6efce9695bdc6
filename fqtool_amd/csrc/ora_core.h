// ora_core.h -- the per-read counting of --ora (overrepresented sequences; Stats::statRead, reference
// src/stats.cpp:277-293), shared by the device kernels (ora.hip) and host code
// (tools/micro/ora_sim.cpp).
//
// A sampled read is scanned once per step of {10, 20, 40, 100, min(150, evalLen - 2)}: window j
// (j < len - step: the last full window is never taken) is looked up in the hot set; on a hit the
// sequence counts once, its distribution counts cycles [j, min(j + step, evalLen)), and the next
// window examined starts at j + step + 1.
//
// The routine is written for a team of W lanes (a wave on the device, one lane on the host) over
// the read's bytes staged in memory the team shares: lanes take the window starts, every candidate
// of the step's hash table (keyed on the window's leading bytes) is compared byte by byte with the
// stored sequence, the step's hits become a bit mask over j, and the greedy j + step + 1 rule is a
// team-uniform walk over that mask.  `hit(seq, j, step)` is called team-uniformly; the caller
// decides where the increments go.  Every loop is bounded by the read's length, the number of
// steps or a table's size, never by a table's contents.
#pragma once

#include <stdint.h>

#include "kstat_core.h"

#include <algorithm>
#include <string>
#include <vector>

#define FQ_ORA_HD FQ_KSTAT_HD

namespace fqora {

constexpr int kMaxSteps = 5;
constexpr int kLeadBytes = 10;  // a window's hash covers its first min(step, kLeadBytes) bytes

// One step's hash table: open addressing with linear probing over `size` (a power of two, more
// than twice the step's sequences, so an empty slot always ends a probe) slots of
// {sequence index or -1, hash of its leading bytes}.
struct ora_slot {
    int32_t seq;
    uint32_t hash;
};
struct ora_table {
    int32_t step;
    uint32_t size;
    uint32_t first;  // slots[first, first + size)
};
// A hot set as the kernels read it: sequence i = bytes[off[i], off[i] + len[i]), back to back, one
// table per step that some sequence's length equals.
struct ora_set {
    int32_t nseq;
    int32_t eval_len;
    int32_t ntab;
    ora_table tab[kMaxSteps];
    const uint8_t* bytes;
    const uint32_t* off;  // nseq starts; the lengths are in len
    const uint16_t* len;
    const ora_slot* slots;
};

FQ_ORA_HD uint32_t lead_hash(const uint8_t* p, int n) {  // FNV-1a
    uint32_t h = 2166136261u;
    for (int i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

// the hot sequence equal to p[0, t.step), or -1
FQ_ORA_HD int lookup(const ora_set& s, const ora_table& t, const uint8_t* p) {
    const int step = t.step;
    const uint32_t h = lead_hash(p, step < kLeadBytes ? step : kLeadBytes);
    const ora_slot* slots = s.slots + t.first;
    uint32_t at = h & (t.size - 1);
    for (uint32_t probe = 0; probe < t.size; ++probe, at = (at + 1) & (t.size - 1)) {
        const ora_slot e = slots[at];
        if (e.seq < 0) return -1;
        if (e.hash != h) continue;
        const uint8_t* q = s.bytes + s.off[e.seq];
        int i = 0;
        while (i < step && q[i] == p[i]) ++i;
        if (i == step) return e.seq;
    }
    return -1;
}

// shared memory of one team for reads of up to max_len bytes: the staged bytes, the hit of every
// window start, the step's mask
FQ_ORA_HD size_t stage_bytes(int max_len) { return ((size_t)max_len + 15) & ~(size_t)15; }
FQ_ORA_HD size_t mask_words(int max_len) { return ((size_t)max_len + 63) / 64; }
FQ_ORA_HD size_t team_bytes(int max_len) {
    return stage_bytes(max_len) + 4 * stage_bytes(max_len) + 8 * mask_words(max_len);
}
struct ora_team_mem {
    uint8_t* s;      // stage_bytes(max_len)
    int32_t* ids;    // one per window start
    uint64_t* mask;  // mask_words(max_len)
    FQ_ORA_HD ora_team_mem(void* base, int max_len)
        : s((uint8_t*)base),
          ids((int32_t*)((uint8_t*)base + stage_bytes(max_len))),
          mask((uint64_t*)((uint8_t*)base + 5 * stage_bytes(max_len))) {}
};

// byte j of a tiled row
FQ_ORA_HD uint8_t row_byte(const fqkstat::kstat_row& r, int j) {
    return r.base[(size_t)(j >> 4) * (FQ_TILE_READS * FQ_CHUNK) + (size_t)(j & 15)];
}

// row[start, start + len) to dst[0, len)
template <class Team>
FQ_ORA_HD void stage_row(const Team& tm, uint8_t* dst, const fqkstat::kstat_row& r, int start, int len) {
    for (int p = tm.lane(); p < len; p += Team::W) dst[p] = row_byte(r, start + p);
}

// the reverse complement's part of a merged read (kstat_core.h count_merged): the complements of
// b[st2 + m2 - 1], ..., b[st2] to dst[0, m2)
template <class Team>
FQ_ORA_HD void stage_revcomp(const Team& tm, uint8_t* dst, const fqkstat::kstat_row& b, int st2, int m2) {
    for (int p = tm.lane(); p < m2; p += Team::W) dst[p] = fqkstat::comp(row_byte(b, st2 + m2 - 1 - p));
}

// One sampled read, staged at m.s[0, len).  The team calls this together, after a sync that made
// the staged bytes visible, and syncs again before it stages the next read.
template <class Team, class Hit>
FQ_ORA_HD void scan_read(const Team& tm, const ora_team_mem& m, int len, const ora_set& set, Hit& hit) {
    for (int t = 0; t < set.ntab; ++t) {
        const ora_table tab = set.tab[t];
        const int step = tab.step;
        const int nwin = len - step;  // j < len - step
        if (nwin <= 0) continue;
        for (int j0 = 0; j0 < nwin; j0 += Team::W) {
            const int j = j0 + tm.lane();
            int id = -1;
            if (j < nwin) {
                id = lookup(set, tab, m.s + j);
                m.ids[j] = id;
            }
            const uint64_t b = tm.ballot(id >= 0);
            if (tm.lane() == 0) {
                const int w = j0 >> 6, sh = j0 & 63;
                m.mask[w] = (sh ? m.mask[w] : 0) | (b << sh);
            }
        }
        tm.sync();
        for (int j = 0; j < nwin;) {
            const uint64_t bits = m.mask[j >> 6] >> (j & 63);
            if (!bits) {
                j = ((j >> 6) + 1) << 6;
                continue;
            }
            j += (int)__builtin_ctzll(bits);
            hit(m.ids[j], j, step);
            j += step + 1;
        }
        tm.sync();
    }
}

// Which reads of a pack feed which Stats, for the two passes: `emit(stat, kind, st1, n1, st2, n2)`
// with stat 0 the R1-side Stats of the pass and 1 the R2-side, kind 1 a window of row 1, 2 a window
// of row 2 (st1, n1), 3 a merged read row1[st1, st1 + n1) + revcomp(row2[st2, st2 + n2)).
struct ora_item {
    int32_t kind, st1, n1, st2, n2;
};
struct ora_post_items {
    ora_item a, b;  // post-R1, post-R2 (kind 0: none)
    FQ_ORA_HD ora_post_items() {
        a.kind = a.st1 = a.n1 = a.st2 = a.n2 = 0;
        b.kind = b.st1 = b.n1 = b.st2 = b.n2 = 0;
    }
    FQ_ORA_HD void row1(int start, int len) { a.kind = 1, a.st1 = start, a.n1 = len; }
    FQ_ORA_HD void row2(int start, int len) { b.kind = 2, b.st1 = start, b.n1 = len; }
    FQ_ORA_HD void merged(int st1, int m1, int st2, int m2) { a.kind = 3, a.st1 = st1, a.n1 = m1, a.st2 = st2, a.n2 = m2; }
};

// ---- host: a set's device image -----------------------------------------------------------------
struct ora_image {
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off;
    std::vector<uint16_t> len;
    std::vector<ora_slot> slots;
    ora_set set{};  // pointers unset
};

// The steps of Stats::statRead for one evaluated length, ascending and distinct
inline std::vector<int> ora_steps(int eval_len) {
    std::vector<int> st = {10, 20, 40, 100, eval_len - 2 < 150 ? eval_len - 2 : 150};
    for (size_t i = 1; i < st.size(); ++i)
        for (size_t j = i; j > 0 && st[j] < st[j - 1]; --j) std::swap(st[j], st[j - 1]);
    std::vector<int> out;
    for (int v : st)
        if (out.empty() || out.back() != v) out.push_back(v);
    return out;
}

// seq i = data[off[i], off[i + 1]); returns false when a sequence is longer than 65535 bytes or
// appears twice (a set has distinct members)
inline bool ora_build(const uint8_t* data, const uint32_t* off, int nseq, int eval_len, ora_image& im) {
    im = ora_image();
    im.set.nseq = nseq;
    im.set.eval_len = eval_len;
    for (int i = 0; i < nseq; ++i) {
        const uint32_t n = off[i + 1] - off[i];
        if (off[i + 1] < off[i] || n > 65535u) return false;
        im.off.push_back((uint32_t)im.bytes.size());
        im.len.push_back((uint16_t)n);
        im.bytes.insert(im.bytes.end(), data + off[i], data + off[i + 1]);
    }
    for (int step : ora_steps(eval_len)) {
        if (step < 1) continue;  // (no window has that length)
        std::vector<int> members;
        for (int i = 0; i < nseq; ++i)
            if (im.len[i] == step) members.push_back(i);
        if (members.empty()) continue;  // a step that matches no hot length can never hit
        uint32_t size = 4;
        while (size < 2 * members.size() + 2) size *= 2;
        ora_table t{step, size, (uint32_t)im.slots.size()};
        im.slots.resize(im.slots.size() + size, ora_slot{-1, 0});
        ora_slot* sl = im.slots.data() + t.first;
        for (int i : members) {
            const uint8_t* p = im.bytes.data() + im.off[i];
            const uint32_t h = lead_hash(p, step < kLeadBytes ? step : kLeadBytes);
            uint32_t at = h & (size - 1);
            for (; sl[at].seq >= 0; at = (at + 1) & (size - 1))
                if (sl[at].hash == h && std::equal(p, p + step, im.bytes.data() + im.off[sl[at].seq])) return false;
            sl[at] = ora_slot{i, h};
        }
        im.set.tab[im.set.ntab++] = t;
    }
    return true;
}

}  // namespace fqora
