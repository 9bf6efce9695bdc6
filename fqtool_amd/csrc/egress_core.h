// egress_core.h -- the per-pair routing of the routed egress (fq_engine_set_egress), shared by the
// device kernels (text.hip) and host code (tools/micro/egress_sim.cpp).
//
// It restates the loop bodies' appends as the host formats them (fqtool_amd/host/processor.cpp
// format_range; reference src/peprocessor.cpp:351-429, src/seprocessor.cpp:337-350) over six output
// streams.  Per pair (single end: per read) `route` decides which reads go where and with which tag,
// `sizes` gives the bytes each stream receives and `write` puts them at the stream's cursor; a
// stream without a writer (its bit clear in `open`) receives nothing.  A read is written as
// Read::toString / toStringWithTag (src/read.h:166-178):
//     name [" " tag] "\n" seq[start, start + len) "\n" strand "\n" qual[start, start + len) "\n"
// with (start, len) of its record, or the whole read for a FQ_RF_NULL record.  Name and strand lines
// come from the text; sequence and quality bytes come from the text, or (`planes`: a pair -c
// corrected) from the read's row of the chunk-interleaved tile planes, where the kernels left the
// corrected bytes: byte j of a row is at row[(j / 16) * 512 + j % 16].
//
// With a UMI description (-u; fq_engine_set_umi) the names carry the UMI tag as UmiProcessor::process
// and addTagToName build it (src/umiprocessor.cpp:10-89; host umi_tag / tagged_name): `umi_tag`
// describes the tag of a pair as up to four slices of the input text, `Name` splits a name at its
// first blank, and a FQ_RF_NULL read is the whole read minus the UMI cut (Mate::cut).  The tag's
// bases and qualities are always the input text's (UMI runs before -c).  Without a description
// (location 0) every routine behaves as it did before.
#pragma once

#include <stdint.h>

#include "../../include/fqengine.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQ_EG_HD __host__ __device__ __forceinline__
#else
#define FQ_EG_HD inline
#endif

namespace fqegress {

// a tag: none, Filter::passFilter's code (FilterResult's failed_type text), or the mate's failure
enum { TAG_NONE = -1, TAG_MATE_FAILING = 256 };

// the tag's text (" " + text follows the name; an unknown code gives the blank alone)
FQ_EG_HD const char* tag_text(int tag, int& len) {
#define FQ_EG_TAG(s) (len = (int)sizeof(s) - 1, s)
    switch (tag) {
        case TAG_MATE_FAILING: return FQ_EG_TAG("paired_read_is_failing");
        case 0: return FQ_EG_TAG("passed");
        case 4: return FQ_EG_TAG("failed_polyx_filter");
        case 8: return FQ_EG_TAG("failed_bad_overlap");
        case 12: return FQ_EG_TAG("failed_too_many_n_bases");
        case 16: return FQ_EG_TAG("failed_too_short");
        case 17: return FQ_EG_TAG("failed_too_long");
        case 20: return FQ_EG_TAG("failed_quality_filter");
        case 24: return FQ_EG_TAG("failed_low_complexity");
        default: return FQ_EG_TAG("");
    }
#undef FQ_EG_TAG
}

// the UMI description (fq_umi); location 0: no UMI
struct Umi {
    int location, length, skip, drop_comment, not_trim;
};

// Read::trimFront of the UMI step (src/read.h:203-208): min(k, len - 1) bases
FQ_EG_HD int umi_cut(int k, int len) { return (k > 0 && len > 0) ? (k < len - 1 ? k : len - 1) : 0; }

// the leading bases the UMI step cuts off mate k, before clamping (Options::umi_front)
FQ_EG_HD int umi_front(const Umi& u, int k, bool paired) {
    if (u.not_trim) return 0;
    const bool r1 = u.location == 3 || u.location == 6, r2 = u.location == 4 || u.location == 6;
    return (k == 0 ? r1 : (r2 && paired)) ? u.length + u.skip : 0;
}

// one mate's record of a pair
struct Mate {
    const char* text;     // the mate's text
    fq_text_rec R;
    fq_read_result r;
    const uint8_t* seq;   // byte 0 of the read's row (chunk 0) in the sequence plane, or null
    const uint8_t* qual;  // ... in the quality plane
    int cut;              // UMI: the bases a FQ_RF_NULL read lost to the UMI cut (else 0)
    FQ_EG_HD int start() const { return (r.flags & FQ_RF_NULL) ? cut : (int)r.start; }
    FQ_EG_HD int len() const { return (r.flags & FQ_RF_NULL) ? (int)R.len - cut : (int)r.len; }
};

FQ_EG_HD size_t row_at(int j) { return (size_t)(j / FQ_CHUNK) * (FQ_TILE_READS * FQ_CHUNK) + (size_t)(j % FQ_CHUNK); }
FQ_EG_HD char seq_at(const Mate& m, bool planes, int j) {
    return planes ? (char)m.seq[row_at(j)] : m.text[m.R.seq_off + j];
}
FQ_EG_HD char qual_at(const Mate& m, bool planes, int j) {
    return planes ? (char)m.qual[row_at(j)] : m.text[m.R.qual_off + j];
}

// what a pair writes: up to two reads in this order (the merged read counts as one, of mate 0)
struct Plan {
    int n;
    int stream[2];
    int mate[2];
    int tag[2];
    bool merged;  // the one item is the merged read
};

// (no array here is indexed with a run-time value: on the device that would put it in scratch memory)
FQ_EG_HD void plan_add(Plan& p, uint32_t open, int stream, int mate, int tag) {
    if (!((open >> stream) & 1u)) return;
    if (p.n == 0) p.stream[0] = stream, p.mate[0] = mate, p.tag[0] = tag;
    else p.stream[1] = stream, p.mate[1] = mate, p.tag[1] = tag;
    ++p.n;
}

FQ_EG_HD bool passing(const fq_read_result& r) { return !(r.flags & FQ_RF_NULL) && r.code == FQ_PASS_FILTER; }

// single end (src/seprocessor.cpp:337-350)
FQ_EG_HD Plan route_single(uint32_t open, const fq_read_result& r) {
    Plan p{};
    if (r.flags & FQ_RF_INDEX_FILTERED) return p;
    if (passing(r)) plan_add(p, open, FQ_EG_OUT1, 0, TAG_NONE);
    else plan_add(p, open, FQ_EG_FAILED, 0, r.code);
    return p;
}

// paired end (src/peprocessor.cpp:351-429)
FQ_EG_HD Plan route_pair(uint32_t open, bool merge, bool discard, const fq_read_result& a, const fq_read_result& b) {
    Plan p{};
    if (a.flags & FQ_RF_INDEX_FILTERED) return p;
    const bool nn1 = !(a.flags & FQ_RF_NULL), nn2 = !(b.flags & FQ_RF_NULL);
    if (merge && nn1 && nn2) {
        if (a.flags & FQ_RF_MERGED) {
            if (a.code == FQ_PASS_FILTER) {
                plan_add(p, open, FQ_EG_MERGED, 0, TAG_NONE);
                p.merged = p.n > 0;
            }
            return p;
        }
        if (!discard) {
            if (a.code == FQ_PASS_FILTER) plan_add(p, open, FQ_EG_MERGED, 0, TAG_NONE);
            if (b.code == FQ_PASS_FILTER) plan_add(p, open, FQ_EG_MERGED, 1, TAG_NONE);
            return p;
        }
    }
    const bool p1 = passing(a), p2 = passing(b);
    const bool left = (open >> FQ_EG_UNPAIRED1) & 1u;  // (the reference tests the left writer in both branches, :417)
    if (p1 && p2) {
        plan_add(p, open, FQ_EG_OUT1, 0, TAG_NONE);
        plan_add(p, open, FQ_EG_OUT2, 1, TAG_NONE);
    } else if (p1) {
        if (left) {
            plan_add(p, open, FQ_EG_UNPAIRED1, 0, TAG_NONE);
            plan_add(p, open, FQ_EG_FAILED, 1, b.code);
        } else {
            plan_add(p, open, FQ_EG_FAILED, 0, TAG_MATE_FAILING);
            plan_add(p, open, FQ_EG_FAILED, 1, b.code);
        }
    } else if (p2) {
        if (left) {  // read 2 first, and read 1's tag is read 2's code (sic, :420)
            plan_add(p, open, FQ_EG_UNPAIRED2, 1, TAG_NONE);
            plan_add(p, open, FQ_EG_FAILED, 0, b.code);
        } else {
            plan_add(p, open, FQ_EG_FAILED, 0, a.code);
            plan_add(p, open, FQ_EG_FAILED, 1, TAG_MATE_FAILING);
        }
    }
    return p;
}

// util::complement as the merge applies it (include/fqengine.h fq_complement)
FQ_EG_HD char comp(char c) {
    switch (c) {
        case 'A': case 'a': return 'T';
        case 'T': case 't': return 'A';
        case 'C': case 'c': return 'G';
        case 'G': case 'g': return 'C';
        default: return 'N';
    }
}

FQ_EG_HD int dec_digits(int v) {
    int d = 1;
    while (v >= 10) {
        v /= 10;
        ++d;
    }
    return d;
}

FQ_EG_HD char* put_dec(char* d, int v) {
    const int nd = dec_digits(v);
    for (int k = nd - 1; k >= 0; --k) {
        d[k] = (char)('0' + v % 10);
        v /= 10;
    }
    return d + nd;
}

// the name's first space (or -1)
FQ_EG_HD int first_space(const char* s, int n) {
    for (int k = 0; k < n; ++k)
        if (s[k] == ' ') return k;
    return -1;
}

// bytes [p, p + n) of the input text
struct Slice {
    const char* p;
    int n;
};

// Read::firstIndex (src/read.h:106-123; host first_index) of the mate's name: the scan runs backwards
// from len - 3, a '+' moves the end to the byte before it, the first ':' met ends the scan;
// substr(i + 1, end - i) stops at the name's end
FQ_EG_HD Slice first_index(const char* nm, int n) {
    Slice s{nm, 0};
    if (n < 5) return s;
    int end = n;
    for (int i = n - 3; i >= 0; --i) {
        const char c = nm[i];
        if (c == '+') end = i - 1;
        if (c == ':') {
            const int rest = n - (i + 1);
            s.p = nm + i + 1;
            s.n = end - i < rest ? end - i : rest;
            return s;
        }
    }
    return s;
}
FQ_EG_HD Slice first_index(const Mate& m) { return first_index(m.text + m.R.name_off, (int)m.R.name_len); }

// a pair's UMI tag: " OX:Z:" a ["-" b] and, when there is a quality part, " BZ:Z:" c ["-" d]; n: its
// bytes (0: no tag, the names stay as they are)
struct Tag {
    int n;
    Slice a, b, c, d;
    bool dash, qdash;
};

FQ_EG_HD int min2(int x, int y) { return x < y ? x : y; }

// UmiProcessor::process (src/umiprocessor.cpp:10-79; host umi_tag), quirks included: location 4's
// quality part is bounded by read 1's length, location 6's read 2 quality part is taken after read
// 2's cut and bounded by read 1's cut length; single end has no tag at locations 2 and 4
FQ_EG_HD Tag umi_tag(const Umi& u, bool paired, const Mate* m) {
    Tag t{};
    const int L = u.length;
    const int len1 = (int)m[0].R.len, len2 = paired ? (int)m[1].R.len : 0;
    switch (u.location) {
        case 1: t.a = first_index(m[0]); break;
        case 2:
            if (paired) t.a = first_index(m[1]);
            break;
        case 3:
            t.a = Slice{m[0].text + m[0].R.seq_off, min2(len1, L)};
            t.c = Slice{m[0].text + m[0].R.qual_off, min2(len1, L)};
            break;
        case 4:
            if (paired) {
                t.a = Slice{m[1].text + m[1].R.seq_off, min2(len2, L)};
                t.c = Slice{m[1].text + m[1].R.qual_off, min2(min2(len1, L), len2)};
            }
            break;
        case 5:
            t.a = first_index(m[0]);
            if (paired) t.dash = true, t.b = first_index(m[1]);
            break;
        case 6:
            t.a = Slice{m[0].text + m[0].R.seq_off, min2(len1, L)};
            t.c = Slice{m[0].text + m[0].R.qual_off, min2(len1, L)};
            if (paired) {
                const int cut1 = u.not_trim ? 0 : umi_cut(L + u.skip, len1), cut2 = u.not_trim ? 0 : umi_cut(L + u.skip, len2);
                t.dash = t.qdash = true;
                t.b = Slice{m[1].text + m[1].R.seq_off, min2(len2, L)};
                t.d = Slice{m[1].text + m[1].R.qual_off + cut2, min2(min2(len1 - cut1, L), len2 - cut2)};
            }
            break;
        default: break;
    }
    const int umi = t.a.n + (t.dash ? 1 + t.b.n : 0), qua = t.c.n + (t.qdash ? 1 + t.d.n : 0);
    t.n = umi == 0 ? 0 : 6 + umi + (qua ? 6 + qua : 0);
    return t;
}

// a name as addTagToName (src/umiprocessor.cpp:81-89; host tagged_name) splits it: the tag goes after
// `head` bytes (up to the first blank, or the whole name), then the name's last `tail` bytes (the
// comment from its blank on; none with --umi_drop_comment).  Without a tag: the whole name, no tail.
struct Name {
    int head, tail;
};

FQ_EG_HD Name split_name(const Mate& m, const Tag& t, bool drop_comment) {
    Name nm{(int)m.R.name_len, 0};
    if (t.n == 0) return nm;
    const int sp = first_space(m.text + m.R.name_off, m.R.name_len);
    if (sp < 0) return nm;
    nm.head = sp;
    nm.tail = drop_comment ? 0 : (int)m.R.name_len - sp;
    return nm;
}

FQ_EG_HD uint32_t read_bytes(const Mate& m, int tag, const Tag& t = Tag{}, bool drop_comment = false) {
    const Name nm = split_name(m, t, drop_comment);
    uint32_t z = (uint32_t)(nm.head + t.n + nm.tail) + m.R.strand_len + 2u * (uint32_t)m.len() + 4u;
    if (tag != TAG_NONE) {
        int tl;
        tag_text(tag, tl);
        z += 1u + (uint32_t)tl;
    }
    return z;
}

// OverlapAnalysis::merge (src/overlapanalysis.cpp:74-104): name "_merged_<m1>_<m2>" spliced in
// before the name's first space (the byte before the space is dropped, as the reference does; a
// name without a space becomes the tag alone).  A UMI-tagged name's first space is its tag's: the
// merged tag goes before the UMI tag, and the byte before it is dropped.
FQ_EG_HD uint32_t merged_bytes(const Mate& m1, const Tag& t = Tag{}, bool drop_comment = false) {
    const int a = m1.r.m_len1, b = m1.r.m_len2;
    const uint32_t tag = 9u + (uint32_t)dec_digits(a) + (uint32_t)dec_digits(b);
    uint32_t name;
    if (t.n) {
        const Name nm = split_name(m1, t, drop_comment);
        name = (uint32_t)(nm.head - (nm.head > 0 ? 1 : 0) + t.n + nm.tail) + tag;
    } else {
        const int sp = first_space(m1.text + m1.R.name_off, m1.R.name_len);
        name = sp < 0 ? tag : (uint32_t)m1.R.name_len - (sp > 0 ? 1u : 0u) + tag;
    }
    return name + m1.R.strand_len + 2u * (uint32_t)(a + b) + 4u;
}

FQ_EG_HD void copy_bytes(char* d, const char* s, int n) {
    for (int b = 0; b < n; ++b) d[b] = s[b];
}

// the UMI tag's bytes
FQ_EG_HD char* put_umi(char* d, const Tag& t) {
    const char ox[6] = {' ', 'O', 'X', ':', 'Z', ':'}, bz[6] = {' ', 'B', 'Z', ':', 'Z', ':'};
    copy_bytes(d, ox, 6);
    d += 6;
    copy_bytes(d, t.a.p, t.a.n);
    d += t.a.n;
    if (t.dash) {
        *d++ = '-';
        copy_bytes(d, t.b.p, t.b.n);
        d += t.b.n;
    }
    if (t.c.n + (t.qdash ? 1 + t.d.n : 0)) {
        copy_bytes(d, bz, 6);
        d += 6;
        copy_bytes(d, t.c.p, t.c.n);
        d += t.c.n;
        if (t.qdash) {
            *d++ = '-';
            copy_bytes(d, t.d.p, t.d.n);
            d += t.d.n;
        }
    }
    return d;
}

FQ_EG_HD char* put_read(char* d, const Mate& m, bool planes, int tag, const Tag& t = Tag{}, bool drop_comment = false) {
    if (t.n) {
        const Name nm = split_name(m, t, drop_comment);
        copy_bytes(d, m.text + m.R.name_off, nm.head);
        d = put_umi(d + nm.head, t);
        copy_bytes(d, m.text + m.R.name_off + m.R.name_len - nm.tail, nm.tail);
        d += nm.tail;
    } else {
        copy_bytes(d, m.text + m.R.name_off, m.R.name_len);
        d += m.R.name_len;
    }
    if (tag != TAG_NONE) {
        int tl;
        const char* t = tag_text(tag, tl);
        *d++ = ' ';
        copy_bytes(d, t, tl);
        d += tl;
    }
    *d++ = '\n';
    const int s = m.start(), n = m.len();
    if (planes) {
        for (int j = 0; j < n; ++j) d[j] = (char)m.seq[row_at(s + j)];
    } else {
        copy_bytes(d, m.text + m.R.seq_off + s, n);
    }
    d += n;
    *d++ = '\n';
    copy_bytes(d, m.text + m.R.strand_off, m.R.strand_len);
    d += m.R.strand_len;
    *d++ = '\n';
    if (planes) {
        for (int j = 0; j < n; ++j) d[j] = (char)m.qual[row_at(s + j)];
    } else {
        copy_bytes(d, m.text + m.R.qual_off + s, n);
    }
    d += n;
    *d++ = '\n';
    return d;
}

FQ_EG_HD char* put_merged(char* d, const Mate& m1, const Mate& m2, bool planes, const Tag& t = Tag{},
                          bool drop_comment = false) {
    const int a = m1.r.m_len1, b = m1.r.m_len2;
    const char* nm = m1.text + m1.R.name_off;
    const Name sn = split_name(m1, t, drop_comment);
    const int sp = t.n ? sn.head : first_space(nm, m1.R.name_len);
    if (sp > 0) {
        copy_bytes(d, nm, sp - 1);
        d += sp - 1;
    }
    const char tag[8] = {'_', 'm', 'e', 'r', 'g', 'e', 'd', '_'};
    copy_bytes(d, tag, 8);
    d = put_dec(d + 8, a);
    *d++ = '_';
    d = put_dec(d, b);
    if (t.n) {
        d = put_umi(d, t);
        copy_bytes(d, nm + m1.R.name_len - sn.tail, sn.tail);
        d += sn.tail;
    } else if (sp >= 0) {
        copy_bytes(d, nm + sp, m1.R.name_len - sp);
        d += m1.R.name_len - sp;
    }
    *d++ = '\n';
    // sequence: r1's window [0, a), then r2's window [0, b) reverse-complemented
    const int s1 = m1.start(), s2 = m2.start();
    for (int j = 0; j < a; ++j) d[j] = seq_at(m1, planes, s1 + j);
    d += a;
    for (int j = 0; j < b; ++j) d[j] = comp(seq_at(m2, planes, s2 + b - 1 - j));
    d += b;
    *d++ = '\n';
    copy_bytes(d, m1.text + m1.R.strand_off, m1.R.strand_len);
    d += m1.R.strand_len;
    *d++ = '\n';
    for (int j = 0; j < a; ++j) d[j] = qual_at(m1, planes, s1 + j);
    d += a;
    for (int j = 0; j < b; ++j) d[j] = qual_at(m2, planes, s2 + b - 1 - j);
    d += b;
    *d++ = '\n';
    return d;
}

// a pack as the routines see it: per mate the text, its records and (when -c ran) the tile planes
struct Pack {
    const char* text[2];
    const fq_text_rec* rec[2];
    const fq_read_result* res;  // [2i], [2i + 1] for pairs, [i] single end
    const uint8_t* seq[2];      // null: no corrected rows to read
    const uint8_t* qual[2];
    int n, stride, paired, merge, discard;
    uint32_t open;
    Umi umi;                    // location 0: none
};

// pair i's mates, its plan, and whether its sequence and quality bytes come from the planes
// (UMI: the pack has a UMI description, whose cut a FQ_RF_NULL read keeps)
template <bool UMI = false>
FQ_EG_HD Plan load(const Pack& pk, int64_t i, Mate (&m)[2], bool& planes) {
    const int mates = pk.paired ? 2 : 1;
    uint8_t flags = 0;
    bool fits = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 2; ++k) {
        if (k >= mates) break;
        m[k].text = pk.text[k];
        m[k].R = pk.rec[k][i];
        m[k].r = pk.res[(size_t)mates * (size_t)i + (size_t)k];
        const size_t row = (size_t)(i / FQ_TILE_READS) * FQ_TILE_READS * (size_t)pk.stride + (size_t)(i % FQ_TILE_READS) * FQ_CHUNK;
        m[k].seq = pk.seq[k] ? pk.seq[k] + row : nullptr;
        m[k].qual = pk.qual[k] ? pk.qual[k] + row : nullptr;
        m[k].cut = UMI ? umi_cut(umi_front(pk.umi, k, pk.paired != 0), (int)m[k].R.len) : 0;
        flags |= m[k].r.flags;
        fits = fits && m[k].seq && m[k].qual && (int)m[k].R.len <= pk.stride;
    }
    planes = (flags & FQ_RF_CORRECTED) && fits;
    return pk.paired ? route_pair(pk.open, pk.merge != 0, pk.discard != 0, m[0].r, m[1].r) : route_single(pk.open, m[0].r);
}

// bytes the pair adds to each stream
FQ_EG_HD void sizes(const Plan& p, const Mate* m, uint32_t (&z)[FQ_EG_STREAMS], const Tag& t = Tag{},
                    bool drop_comment = false) {
    for (int s = 0; s < FQ_EG_STREAMS; ++s) z[s] = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 2; ++k) {
        if (k >= p.n) break;
        Mate mk = m[0];
        if (p.mate[k]) mk = m[1];
        const uint32_t v = p.merged ? merged_bytes(m[0], t, drop_comment) : read_bytes(mk, p.tag[k], t, drop_comment);
        for (int s = 0; s < FQ_EG_STREAMS; ++s) z[s] += s == p.stream[k] ? v : 0u;
    }
}

// writes them at the streams' cursors d[s] (advanced past what was written)
FQ_EG_HD void write(const Plan& p, const Mate* m, bool planes, char* (&d)[FQ_EG_STREAMS], const Tag& t = Tag{},
                    bool drop_comment = false) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 2; ++k) {
        if (k >= p.n) break;
        Mate mk = m[0];
        if (p.mate[k]) mk = m[1];
        char* at = nullptr;
        for (int s = 0; s < FQ_EG_STREAMS; ++s) at = s == p.stream[k] ? d[s] : at;
        at = p.merged ? put_merged(at, m[0], m[1], planes, t, drop_comment) : put_read(at, mk, planes, p.tag[k], t, drop_comment);
        for (int s = 0; s < FQ_EG_STREAMS; ++s) d[s] = s == p.stream[k] ? at : d[s];
    }
}

}  // namespace fqegress
