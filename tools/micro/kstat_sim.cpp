// kstat_sim.cpp -- kstat.hip's per-read routines (fqtool_amd/csrc/kstat_core.h) run on the host:
// one loop iteration per lane's read over heap planes of exactly fq_batch_bytes, increments into
// heap tables of exactly 4^k counters, so a sanitizer sees every access the kernels would make
// (CPU only).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/micro/kstat_sim.cpp -o tools/micro/kstat_sim
//   tools/micro/kstat_sim IN OUT   IN: int32 {magic 0x4b535431, k, paired, merge_enabled, discard_unmerged, n, stride,
//                                  has_records}, uint16 len1[n] (, len2[n]), the rows seq1[n][stride] (, seq2), then
//                                  the fq_read_result records (n, or 2n for pairs; without them only the pre tables
//                                  are counted).  OUT: the four tables, 4 * 4^k uint64.
//   tools/micro/kstat_sim --self   hostile packs made here (lengths 0 .. k + 1 and around the chunk boundaries, a bad
//                                  byte at every position, merged junctions, records with windows outside the read)
//                                  against a plain per-window count; exit status 1 on a difference.
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fqtool_amd/csrc/kstat_core.h"

using namespace fqkstat;

struct Pack {
    int k = 0, paired = 0, merge = 0, discard = 0, n = 0, stride = 0;
    std::vector<uint16_t> len[2];
    std::vector<std::string> seq[2];
    std::vector<fq_read_result> res;
};

struct Inc {
    uint64_t* t;
    void operator()(uint32_t key) { ++t[key]; }
};

// what the two kernels of a pack do, read by read
static std::vector<uint64_t> run(const Pack& p) {
    const size_t tw = (size_t)1 << (2 * p.k);
    uint64_t* tab = (uint64_t*)calloc(4 * tw, 8);
    const size_t bytes = fq_batch_bytes(p.n, p.stride);
    uint8_t* plane[2] = {(uint8_t*)malloc(bytes ? bytes : 1), (uint8_t*)malloc(bytes ? bytes : 1)};
    for (int m = 0; m < (p.paired ? 2 : 1); ++m) {
        memset(plane[m], 0xEE, bytes);
        for (int i = 0; i < p.n; ++i)
            fq_batch_put_row(plane[m], p.stride, i, (const uint8_t*)p.seq[m][i].data(), (int)p.seq[m][i].size());
    }
    for (int post = 0; post < 2; ++post) {
        if (post && p.res.empty()) break;
        // each table on its own heap block, as the kernels' b1 / b2 see them
        uint64_t* t1 = (uint64_t*)calloc(tw, 8);
        uint64_t* t2 = (uint64_t*)calloc(tw, 8);
        Inc b1{t1}, b2{t2};
        for (int64_t idx = 0; idx < p.n; ++idx) {
            const int l1 = p.len[0][idx], l2 = p.paired ? p.len[1][idx] : 0;
            if (l1 > p.stride || l2 > p.stride) continue;
            kstat_row s1(plane[0], p.stride, idx);
            if (!post) {
                count_row(s1, 0, l1, p.k, b1);
                if (p.paired) {
                    kstat_row s2(plane[1], p.stride, idx);
                    count_row(s2, 0, l2, p.k, b2);
                }
            } else if (p.paired) {
                kstat_row s2(plane[1], p.stride, idx);
                post_pair(p.merge, p.discard, p.res[2 * idx], p.res[2 * idx + 1], s1, l1, s2, l2, p.k, b1, b2);
            } else {
                post_single(p.res[idx], s1, l1, p.k, b1);
            }
        }
        for (size_t i = 0; i < tw; ++i) tab[(2 * post) * tw + i] = t1[i], tab[(2 * post + 1) * tw + i] = t2[i];
        free(t1);
        free(t2);
    }
    free(plane[0]);
    free(plane[1]);
    std::vector<uint64_t> out(tab, tab + 4 * tw);
    free(tab);
    return out;
}

// ---- --self: a plain count, window by window ---------------------------------------------------
static void plain(std::vector<uint64_t>& t, size_t base, const std::string& s, int k) {
    for (int i = 0; i + k <= (int)s.size(); ++i) {
        uint64_t key = 0;
        bool ok = true;
        for (int j = 0; j < k && ok; ++j) {
            const char* at = strchr("ATCG", s[i + j]);
            ok = s[i + j] && at;
            if (ok) key = key * 4 + (uint64_t)(at - "ATCG");
        }
        if (ok) ++t[base + key];
    }
}

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}
static std::string rand_seq(int n, bool hostile) {
    std::string s((size_t)n, 'A');
    for (char& c : s) c = hostile && rnd() % 11 == 0 ? "NnacgtRYK."[rnd() % 10] : "ACGT"[rnd() % 4];
    return s;
}

static int self_test() {
    int bad = 0;
    for (int k : {4, 5, 7, 8, 12}) {
        for (int stride : {160, 320}) {
            Pack p;
            p.k = k, p.paired = 1, p.stride = stride;
            std::vector<std::string> reads;
            for (int L = 0; L <= k + 1; ++L) reads.push_back(rand_seq(L, false));
            for (int L : {15, 16, 17, 31, 32, 33, 47, 48, 49, stride - 1, stride}) reads.push_back(rand_seq(L, false));
            const std::string base = rand_seq(2 * k, false);
            for (int pos = 0; pos < 2 * k; ++pos)
                for (char c : {'N', 'a', 'R'}) {
                    std::string s = base;
                    s[(size_t)pos] = c;
                    reads.push_back(s);
                }
            for (int i = 0; i < 40; ++i) reads.push_back(rand_seq((int)(rnd() % (stride + 1)), true));
            p.n = (int)reads.size();
            for (int m = 0; m < 2; ++m)
                for (int i = 0; i < p.n; ++i) {
                    const std::string& s = reads[(size_t)((i * (m ? 7 : 1) + 3 * m) % p.n)];
                    p.seq[m].push_back(s);
                    p.len[m].push_back((uint16_t)s.size());
                }
            for (int mode = 0; mode < 3; ++mode) {  // no -m, -m, -m --discard_unmerged
                if (k == 12 && (mode != 1 || stride != 160)) continue;  // (0.5 GiB of tables: once)
                p.merge = mode > 0, p.discard = mode > 1;
                p.res.assign((size_t)2 * p.n, fq_read_result{});
                std::vector<uint64_t> want((size_t)4 << (2 * k), 0);
                const size_t tw = (size_t)1 << (2 * k);
                for (int i = 0; i < p.n; ++i) {
                    const std::string &a = p.seq[0][i], &b = p.seq[1][i];
                    plain(want, 0, a, k);
                    plain(want, tw, b, k);
                    fq_read_result& r1 = p.res[2 * (size_t)i];
                    fq_read_result& r2 = p.res[2 * (size_t)i + 1];
                    const int la = (int)a.size(), lb = (int)b.size();
                    r1.start = (uint16_t)(la ? rnd() % (la + 1) : 0), r1.len = (uint16_t)(rnd() % (la - r1.start + 1));
                    r2.start = (uint16_t)(lb ? rnd() % (lb + 1) : 0), r2.len = (uint16_t)(rnd() % (lb - r2.start + 1));
                    const uint32_t what = rnd() % 16;
                    if (what == 0) r1.flags |= FQ_RF_NULL;
                    if (what == 1) r2.flags |= FQ_RF_NULL;
                    if (what == 2) r1.flags = r2.flags = FQ_RF_INDEX_FILTERED;
                    if (what == 3) r1.code = FQ_FAIL_QUALITY;
                    if (what == 4) r2.code = FQ_FAIL_LENGTH;
                    if (what == 5) r1.len = (uint16_t)(la + 1 + rnd() % 50);  // a window outside the read: skipped
                    const bool merged = p.merge && what >= 8 && what < 12;
                    if (merged) {
                        r1.flags |= FQ_RF_MERGED | FQ_RF_OVERLAP;
                        r1.m_len1 = (uint16_t)(rnd() % (r1.len + 1));
                        r1.m_len2 = (uint16_t)(rnd() % (r2.len + 1));
                        r2.code = r1.code;
                    }
                    if ((r1.flags | r2.flags) & (FQ_RF_NULL | FQ_RF_INDEX_FILTERED)) continue;
                    if (r1.start + r1.len > la || r2.start + r2.len > lb) continue;
                    const std::string w1 = a.substr(r1.start, r1.len), w2 = b.substr(r2.start, r2.len);
                    if (merged) {
                        if (r1.code != FQ_PASS_FILTER) continue;
                        std::string rc(w2.rbegin(), w2.rend());
                        for (char& c : rc) c = fq_complement(c);
                        plain(want, 2 * tw, w1.substr(0, r1.m_len1) + rc.substr(w2.size() - r1.m_len2, r1.m_len2), k);
                    } else if (p.merge) {
                        if (p.discard) continue;
                        if (r1.code == FQ_PASS_FILTER) plain(want, 2 * tw, w1, k);
                        if (r2.code == FQ_PASS_FILTER) plain(want, 3 * tw, w2, k);
                    } else if (r1.code == FQ_PASS_FILTER && r2.code == FQ_PASS_FILTER) {
                        plain(want, 2 * tw, w1, k);
                        plain(want, 3 * tw, w2, k);
                    }
                }
                const std::vector<uint64_t> got = run(p);
                if (got != want) {
                    ++bad;
                    fprintf(stderr, "kstat_sim --self: k %d stride %d mode %d differs\n", k, stride, mode);
                }
            }
        }
    }
    printf("kstat_sim --self: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--self")) return self_test();
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[8];
    if (fread(h, 4, 8, f) != 8 || h[0] != 0x4b535431) return 2;
    Pack p;
    p.k = h[1], p.paired = h[2], p.merge = h[3], p.discard = h[4], p.n = h[5], p.stride = h[6];
    if (p.k < FQ_KSTAT_MIN_K || p.k > FQ_KSTAT_MAX_K || p.n < 0 || p.stride <= 0 || (p.stride & 15)) return 2;
    const int mates = p.paired ? 2 : 1;
    for (int m = 0; m < mates; ++m) {
        p.len[m].resize((size_t)p.n);
        if (p.n && fread(p.len[m].data(), 2, (size_t)p.n, f) != (size_t)p.n) return 2;
    }
    std::vector<char> row((size_t)p.stride);
    for (int m = 0; m < mates; ++m)
        for (int i = 0; i < p.n; ++i) {
            if (fread(row.data(), 1, row.size(), f) != row.size()) return 2;
            p.seq[m].emplace_back(row.data(), (size_t)(p.len[m][i] <= p.stride ? p.len[m][i] : p.stride));
        }
    if (h[7]) {
        p.res.resize((size_t)p.n * mates);
        if (p.n && fread(p.res.data(), sizeof(fq_read_result), p.res.size(), f) != p.res.size()) return 2;
    }
    fclose(f);
    const std::vector<uint64_t> t = run(p);
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(t.data(), 8, t.size(), o) != t.size()) return 2;
    fclose(o);
    return 0;
}
