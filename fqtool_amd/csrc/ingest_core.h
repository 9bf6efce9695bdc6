// ingest_core.h -- the per-record routines of the device ingest (include/fqengine.h: the index
// filter, --phred64 and the pack cuts of split outputs), shared by the device kernels (ingest.hip)
// and host code (tools/micro/ingest_sim.cpp).
//
//   * index_flag: Filter::filterByIndex (reference src/filter.cpp:191-232; the host's index_match /
//     prepare_pack in fqtool_amd/host/processor.cpp) on the records' input names: Read::firstIndex
//     of the name (egress_core.h first_index) against the lists.
//   * phred64_to_33: Read::convertPhred64To33 (src/read.h:71-75), char arithmetic.
//   * cut_piece: piece j of a pack cut at every record whose global index is a multiple of `every`
//     (the reference's packs of --max_item_in_pack reads, between which alone it closes and opens
//     split files: ThreadConfig::markProcessed, src/threadconfig.cpp:88-137), from the egress's
//     per-record sizes and their exclusive scan.
#pragma once

#include <stdint.h>

#include "../../include/fqengine.h"
#include "egress_core.h"

namespace fqingest {

// a list of the index filter: entry i = bytes[off[i], off[i + 1])
struct List {
    const uint8_t* bytes;
    const uint32_t* off;
    int n;
};

// Filter::match: some entry differs from the index in at most `threshold` of their first
// min(entry length, index length) bytes
FQ_EG_HD bool match(const List& l, const char* idx, int ilen, int threshold) {
    for (int e = 0; e < l.n; ++e) {
        const uint32_t a = l.off[e];
        const int elen = (int)(l.off[e + 1] - a);
        const int m = elen < ilen ? elen : ilen;
        const uint8_t* s = l.bytes + a;
        int diff = 0;
        for (int k = 0; k < m; ++k)
            if (s[k] != (uint8_t)idx[k] && ++diff > threshold) break;
        if (diff <= threshold) return true;
    }
    return false;
}

// the FQ_BF_* flags of record i: text2 / rec2 are null for single end
FQ_EG_HD uint8_t index_flag(const List& l1, const List& l2, int threshold, const char* text1, const fq_text_rec& r1,
                            const char* text2, const fq_text_rec* r2) {
    const fqegress::Slice a = fqegress::first_index(text1 + r1.name_off, (int)r1.name_len);
    bool hit = match(l1, a.p, a.n, threshold);
    if (!hit && text2) {
        const fqegress::Slice b = fqegress::first_index(text2 + r2->name_off, (int)r2->name_len);
        hit = match(l2, b.p, b.n, threshold);
    }
    return hit ? (uint8_t)FQ_BF_INDEX_FILTERED : (uint8_t)0;
}

FQ_EG_HD uint8_t phred64_to_33(uint8_t q) {
    const int v = (int)(signed char)q - (64 - 33);
    return (uint8_t)(v < 33 ? 33 : v);
}

// pieces of a pack of n records whose first has global index `first`
FQ_EG_HD uint32_t cut_count(uint64_t every, uint64_t first, uint32_t n) {
    return n ? (uint32_t)((first + n - 1) / every - first / every) + 1u : 0u;
}

// records [lo, hi) of piece j
FQ_EG_HD void cut_range(uint64_t every, uint64_t first, uint32_t n, uint32_t j, uint32_t& lo, uint32_t& hi) {
    const uint64_t base = first / every * every;  // global index of the reference pack piece 0 lies in
    const uint64_t a = base + (uint64_t)j * every, b = a + every;
    lo = a > first ? (uint32_t)(a - first) : 0u;
    hi = b - first < n ? (uint32_t)(b - first) : n;
}

// output bytes of stream m before record i (i == n: all of them)
FQ_EG_HD uint64_t cut_offset(const uint32_t* size, const uint32_t* off, uint32_t n, uint32_t i) {
    return i < n ? (uint64_t)off[i] : (uint64_t)off[n - 1] + size[n - 1];
}

}  // namespace fqingest
