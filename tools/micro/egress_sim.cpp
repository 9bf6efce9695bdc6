// egress_sim.cpp -- the routed egress's per-pair routine (fqtool_amd/csrc/egress_core.h) run on the
// host as text.hip's kernels run it: one loop iteration per lane's pair, a size pass, an exclusive
// sum per open stream, a write pass into heap buffers of exactly each stream's total, over heap
// copies of the text and tile planes of exactly their sizes, so a sanitizer sees every access the
// kernels would make (CPU only).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/micro/egress_sim.cpp -o tools/micro/egress_sim
//   tools/micro/egress_sim IN OUT   IN: int32 {magic 0x45475231, paired, merge_enabled, discard_unmerged,
//                                   correction_enabled, open mask, n, stride}, per mate {uint64 text bytes, the text,
//                                   n fq_text_rec}, then the fq_read_result records (n, or 2n for pairs).
//                                   With correction_enabled the planes hold the rows as -c leaves them
//                                   (fq_correct_pair_text applied to the FQ_RF_CORRECTED pairs).
//                                   Magic 0x45475532: five more int32 follow the eight, the UMI description
//                                   {location 1..6, length, skip, drop_comment, not_trim} (fq_umi), and the
//                                   routine runs as the UMI instantiation of the kernels does.
//                                   OUT: uint64 bytes[6], then the six streams' text.
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fqtool_amd/csrc/egress_core.h"

using namespace fqegress;

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[8];
    if (fread(h, 4, 8, f) != 8 || (h[0] != 0x45475231 && h[0] != 0x45475532)) return 2;
    const bool with_umi = h[0] == 0x45475532;
    int32_t uh[5] = {0, 0, 0, 0, 0};
    if (with_umi && (fread(uh, 4, 5, f) != 5 || uh[0] < 1 || uh[0] > 6 || uh[1] < 0 || uh[2] < 0)) return 2;
    const int paired = h[1], merge = h[2], discard = h[3], correction = h[4], n = h[6], stride = h[7];
    const uint32_t open = (uint32_t)h[5];
    if (n < 0 || stride <= 0 || (stride & 15) || (open >> FQ_EG_STREAMS)) return 2;
    const int mates = paired ? 2 : 1;
    char* text[2] = {nullptr, nullptr};
    fq_text_rec* rec[2] = {nullptr, nullptr};
    uint64_t tbytes[2] = {0, 0};
    for (int m = 0; m < mates; ++m) {
        if (fread(&tbytes[m], 8, 1, f) != 1) return 2;
        text[m] = (char*)malloc(tbytes[m] ? tbytes[m] : 1);
        rec[m] = (fq_text_rec*)malloc(n ? (size_t)n * sizeof(fq_text_rec) : 1);
        if (tbytes[m] && fread(text[m], 1, tbytes[m], f) != tbytes[m]) return 2;
        if (n && fread(rec[m], sizeof(fq_text_rec), (size_t)n, f) != (size_t)n) return 2;
    }
    const size_t nres = (size_t)n * mates;
    fq_read_result* res = (fq_read_result*)malloc(nres ? nres * sizeof(fq_read_result) : 1);
    if (nres && fread(res, sizeof(fq_read_result), nres, f) != nres) return 2;
    fclose(f);

    // the tile planes as the pack's kernels leave them
    const size_t pbytes = fq_batch_bytes(n, stride);
    uint8_t* plane[4] = {nullptr, nullptr, nullptr, nullptr};  // seq1, qual1, seq2, qual2
    if (correction && paired) {
        for (int k = 0; k < 4; ++k) {
            plane[k] = (uint8_t*)malloc(pbytes ? pbytes : 1);
            memset(plane[k], 0xEE, pbytes);
        }
        for (int i = 0; i < n; ++i) {
            std::string s[2], q[2];
            bool fits = true;
            for (int m = 0; m < 2; ++m) {
                const fq_text_rec& R = rec[m][i];
                s[m].assign(text[m] + R.seq_off, R.len);
                q[m].assign(text[m] + R.qual_off, R.len);
                fits = fits && R.len <= stride;
            }
            if (!fits) continue;  // (the engine fails such a pack)
            const fq_read_result &a = res[2 * (size_t)i], &b = res[2 * (size_t)i + 1];
            if ((a.flags | b.flags) & FQ_RF_CORRECTED)
                fq_correct_pair_text(&s[0][0] + a.start, &q[0][0] + a.start, &s[1][0] + b.start, &q[1][0] + b.start,
                                     (int16_t)b.m_len1, b.m_len2, b.reserved);
            for (int m = 0; m < 2; ++m) {
                fq_batch_put_row(plane[2 * m], stride, i, (const uint8_t*)s[m].data(), (int)s[m].size());
                fq_batch_put_row(plane[2 * m + 1], stride, i, (const uint8_t*)q[m].data(), (int)q[m].size());
            }
        }
    }

    Pack pk{};
    for (int m = 0; m < mates; ++m) {
        pk.text[m] = text[m], pk.rec[m] = rec[m];
        pk.seq[m] = plane[2 * m], pk.qual[m] = plane[2 * m + 1];
    }
    pk.res = res;
    pk.n = n, pk.stride = stride, pk.paired = paired, pk.merge = paired && merge, pk.discard = discard, pk.open = open;
    pk.umi = Umi{uh[0], uh[1], uh[2], uh[3], uh[4]};
    // (the tag is derived anew in each pass, as the two kernels do)
    auto tag_of = [&](const Plan& p, const Mate* m) { return with_umi && p.n ? umi_tag(pk.umi, paired != 0, m) : Tag{}; };
    auto load_pair = [&](int i, Mate(&m)[2], bool& planes) { return with_umi ? load<true>(pk, i, m, planes) : load(pk, i, m, planes); };

    // size pass, exclusive sums, exact buffers, write pass
    std::vector<uint32_t> size[FQ_EG_STREAMS], off[FQ_EG_STREAMS];
    uint64_t total[FQ_EG_STREAMS] = {0, 0, 0, 0, 0, 0};
    for (int s = 0; s < FQ_EG_STREAMS; ++s) size[s].assign((size_t)n, 0), off[s].assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        Mate m[2];
        bool planes;
        const Plan p = load_pair(i, m, planes);
        uint32_t z[FQ_EG_STREAMS];
        sizes(p, m, z, tag_of(p, m), uh[3] != 0);
        for (int s = 0; s < FQ_EG_STREAMS; ++s) {
            if (z[s] && !((open >> s) & 1u)) return 3;  // nothing may go to a stream without a writer
            size[s][(size_t)i] = z[s];
        }
    }
    char* out[FQ_EG_STREAMS];
    for (int s = 0; s < FQ_EG_STREAMS; ++s) {
        for (int i = 0; i < n; ++i) off[s][(size_t)i] = (uint32_t)total[s], total[s] += size[s][(size_t)i];
        out[s] = (char*)malloc(total[s] ? total[s] : 1);
    }
    for (int i = 0; i < n; ++i) {
        Mate m[2];
        bool planes;
        const Plan p = load_pair(i, m, planes);
        if (!p.n) continue;
        char* d[FQ_EG_STREAMS];
        for (int s = 0; s < FQ_EG_STREAMS; ++s) d[s] = ((open >> s) & 1u) ? out[s] + off[s][(size_t)i] : nullptr;
        write(p, m, planes, d, tag_of(p, m), uh[3] != 0);
        for (int s = 0; s < FQ_EG_STREAMS; ++s)  // each cursor ends where the size pass said
            if (((open >> s) & 1u) && d[s] != out[s] + off[s][(size_t)i] + size[s][(size_t)i]) return 4;
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(total, 8, FQ_EG_STREAMS, o) != FQ_EG_STREAMS) return 2;
    for (int s = 0; s < FQ_EG_STREAMS; ++s)
        if (total[s] && fwrite(out[s], 1, total[s], o) != total[s]) return 2;
    fclose(o);
    for (int s = 0; s < FQ_EG_STREAMS; ++s) free(out[s]);
    for (int k = 0; k < 4; ++k) free(plane[k]);
    for (int m = 0; m < 2; ++m) free(text[m]), free(rec[m]);
    free(res);
    return 0;
}
