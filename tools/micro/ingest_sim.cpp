// ingest_sim.cpp -- the device ingest's per-record routines (fqtool_amd/csrc/ingest_core.h) run on the
// host as ingest.hip's kernels run them: one loop iteration per lane's record (index filter), per
// (record, 16-byte chunk) (--phred64) and per piece (pack cuts), over heap copies of the lists, the
// text and the sizes of exactly their sizes, so a sanitizer sees every access the kernels would make
// (CPU only).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/micro/ingest_sim.cpp -o tools/micro/ingest_sim
//   tools/micro/ingest_sim IN OUT
//   IN:  int32 {magic 0x494E4731, paired, n, stride, threshold, n1, n2, phred64}, uint64 {every, first_item},
//        list 1's n1 + 1 uint32 offsets, list 2's n2 + 1, list 1's bytes, list 2's bytes,
//        per mate {uint64 text bytes, the text, n fq_text_rec},
//        per mate n uint32: the bytes each record adds to the mate's output stream (text_size_kernel's).
//   OUT: n flag bytes, per mate its text after the --phred64 pass (as it came with phred64 0),
//        uint32 pieces, then the pieces' fq_cut entries (every 0: no pieces).
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fqtool_amd/csrc/ingest_core.h"

using namespace fqingest;

template <class T>
static T* heap(size_t n) {  // (never a zero-byte block: its address must still be valid to hold)
    return (T*)malloc(n ? n * sizeof(T) : 1);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[8];
    uint64_t cutp[2];
    if (fread(h, 4, 8, f) != 8 || h[0] != 0x494E4731 || fread(cutp, 8, 2, f) != 2) return 2;
    const int paired = h[1], n = h[2], stride = h[3], threshold = h[4], n1 = h[5], n2 = h[6], phred64 = h[7];
    const uint64_t every = cutp[0], first = cutp[1];
    if (n < 0 || stride <= 0 || (stride & 15) || threshold < 0 || n1 < 0 || n2 < 0) return 2;
    const int mates = paired ? 2 : 1;
    uint32_t* off[2] = {heap<uint32_t>((size_t)n1 + 1), heap<uint32_t>((size_t)n2 + 1)};
    const int ln[2] = {n1, n2};
    uint8_t* bytes[2];
    for (int m = 0; m < 2; ++m)
        if (fread(off[m], 4, (size_t)ln[m] + 1, f) != (size_t)ln[m] + 1) return 2;
    for (int m = 0; m < 2; ++m) {
        const size_t len = off[m][ln[m]];
        bytes[m] = heap<uint8_t>(len);
        if (len && fread(bytes[m], 1, len, f) != len) return 2;
    }
    char* text[2] = {nullptr, nullptr};
    fq_text_rec* rec[2] = {nullptr, nullptr};
    uint64_t tbytes[2] = {0, 0};
    for (int m = 0; m < mates; ++m) {
        if (fread(&tbytes[m], 8, 1, f) != 1) return 2;
        text[m] = heap<char>(tbytes[m]);
        rec[m] = heap<fq_text_rec>((size_t)n);
        if (tbytes[m] && fread(text[m], 1, tbytes[m], f) != tbytes[m]) return 2;
        if (n && fread(rec[m], sizeof(fq_text_rec), (size_t)n, f) != (size_t)n) return 2;
    }
    uint32_t* size[2] = {nullptr, nullptr};
    uint32_t* offs[2] = {nullptr, nullptr};
    for (int m = 0; m < mates; ++m) {
        size[m] = heap<uint32_t>((size_t)n);
        offs[m] = heap<uint32_t>((size_t)n);
        if (n && fread(size[m], 4, (size_t)n, f) != (size_t)n) return 2;
        uint32_t at = 0;
        for (int i = 0; i < n; ++i) {  // (the egress's exclusive scan)
            offs[m][i] = at;
            at += size[m][i];
        }
    }
    fclose(f);

    // index_flags_kernel: one lane per record
    uint8_t* flags = heap<uint8_t>((size_t)n);
    const List l1{bytes[0], off[0], n1}, l2{bytes[1], off[1], n2};
    for (int i = 0; i < n; ++i)
        flags[i] = index_flag(l1, l2, threshold, text[0], rec[0][i], paired ? text[1] : nullptr, paired ? &rec[1][i] : nullptr);

    // phred64_kernel: one thread per (record, 16-byte chunk)
    if (phred64) {
        const int nch = stride >> 4;
        for (int m = 0; m < mates; ++m)
            for (long long t = 0; t < (long long)n * nch; ++t) {
                const long long r = t / nch;
                const int j0 = 16 * (int)(t - r * nch);
                const fq_text_rec R = rec[m][r];
                const int k = (int)R.len - j0 < 16 ? (int)R.len - j0 : 16;
                uint8_t* q = reinterpret_cast<uint8_t*>(text[m]) + R.qual_off + j0;
                for (int b = 0; b < k; ++b) q[b] = phred64_to_33(q[b]);
            }
    }

    // cuts_kernel: one wave per piece, the lanes striding over its records
    const uint32_t pieces = every ? cut_count(every, first, (uint32_t)n) : 0u;
    fq_cut* cuts = heap<fq_cut>(pieces);
    for (uint32_t j = 0; j < pieces; ++j) {
        uint32_t lo, hi;
        cut_range(every, first, (uint32_t)n, j, lo, hi);
        fq_cut c{};
        for (uint32_t base = lo; base < hi; base += 64)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t i = base + lane;
                c.passed += i < hi && size[0][i] != 0;
            }
        c.bytes[0] = cut_offset(size[0], offs[0], (uint32_t)n, hi) - cut_offset(size[0], offs[0], (uint32_t)n, lo);
        if (paired) c.bytes[1] = cut_offset(size[1], offs[1], (uint32_t)n, hi) - cut_offset(size[1], offs[1], (uint32_t)n, lo);
        c.items = hi - lo;
        cuts[j] = c;
    }

    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    if (n) fwrite(flags, 1, (size_t)n, g);
    for (int m = 0; m < mates; ++m)
        if (tbytes[m]) fwrite(text[m], 1, tbytes[m], g);
    fwrite(&pieces, 4, 1, g);
    if (pieces) fwrite(cuts, sizeof(fq_cut), pieces, g);
    fclose(g);
    for (int m = 0; m < 2; ++m) {
        free(off[m]);
        free(bytes[m]);
        free(text[m]);
        free(rec[m]);
        free(size[m]);
        free(offs[m]);
    }
    free(flags);
    free(cuts);
    return 0;
}
