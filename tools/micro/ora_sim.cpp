// ora_sim.cpp -- ora.hip's per-read routine (fqtool_amd/csrc/ora_core.h) run on the host: a team of
// one lane per sampled read over heap planes of exactly fq_batch_bytes, a heap block of exactly
// team_bytes(max_len) as the team's shared memory, the sets' images and the four result blocks on
// the heap at their exact sizes, so a sanitizer sees every access the kernels would make (CPU only).
// The passes around it (which reads are sampled, from the running counts and the prefix count of
// the reads that reach the post Stats) are restated here as ora.hip's kernels do them.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/micro/ora_sim.cpp -o tools/micro/ora_sim
//   tools/micro/ora_sim IN OUT   IN: int32 {magic 0x4f524131, sampling, evalLen1, evalLen2, paired, merge_enabled,
//                                discard_unmerged, n, stride, has_records, nseq1, nseq2}, uint64 counts[4] (the four
//                                Stats' statRead calls before the pack), per set uint32 off[nseq + 1] and its bytes,
//                                uint16 len1[n] (, len2[n]), the rows seq1[n][stride] (, seq2), then the
//                                fq_read_result records (n, or 2n for pairs; without them only the pre blocks are
//                                counted).  OUT: the four blocks [pre-R1 | pre-R2 | post-R1 | post-R2], then the
//                                four counts after the pack.
//   tools/micro/ora_sim --self   hostile packs made here (planted hot sequences back to back and overlapping, bad
//                                bytes, every length around the steps and the chunk edges, merged junctions, records
//                                with windows outside the read) against the reference's loop written out plainly
//                                over std::map; exit status 1 on a difference.
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../fqtool_amd/csrc/ora_core.h"

using namespace fqora;
using fqkstat::kstat_row;

struct Pack {
    int sampling = 1, eval[2] = {151, 151}, paired = 0, merge = 0, discard = 0, n = 0, stride = 0;
    uint64_t counts[4] = {0, 0, 0, 0};
    std::vector<std::string> set[2];
    std::vector<uint16_t> len[2];
    std::vector<std::string> seq[2];
    std::vector<fq_read_result> res;
};

struct One {  // the team of the host: one lane
    static constexpr int W = 1;
    int lane() const { return 0; }
    uint64_t ballot(bool p) const { return p ? 1 : 0; }
    void sync() const {}
};

struct Inc {
    uint64_t* blk;
    int eval;
    void operator()(int seq, int j, int step) {
        uint64_t* cell = blk + (size_t)seq * (size_t)(1 + eval);
        ++cell[0];
        const int end = j + step < eval ? j + step : eval;
        for (int p = j; p < end; ++p) ++cell[1 + p];
    }
};

static bool image_of(const std::vector<std::string>& seqs, int eval, ora_image& im) {
    std::string data;
    std::vector<uint32_t> off{0};
    for (const std::string& s : seqs) {
        data += s;
        off.push_back((uint32_t)data.size());
    }
    if (!ora_build((const uint8_t*)data.data(), off.data(), (int)seqs.size(), eval, im)) return false;
    im.set.bytes = im.bytes.data();
    im.set.off = im.off.data();
    im.set.len = im.len.data();
    im.set.slots = im.slots.data();
    return true;
}

// what the kernels of a pack do, pair by pair; false: a set the engine refuses
static bool run(const Pack& p, std::vector<uint64_t>& out) {
    ora_image im[2];
    if (!image_of(p.set[0], p.eval[0], im[0]) || !image_of(p.set[1], p.eval[1], im[1])) return false;
    const size_t w[2] = {p.set[0].size() * (size_t)(1 + p.eval[0]), p.set[1].size() * (size_t)(1 + p.eval[1])};
    const size_t bytes = fq_batch_bytes(p.n, p.stride);
    uint8_t* plane[2] = {(uint8_t*)malloc(bytes ? bytes : 1), (uint8_t*)malloc(bytes ? bytes : 1)};
    for (int m = 0; m < (p.paired ? 2 : 1); ++m) {
        memset(plane[m], 0xEE, bytes);
        for (int i = 0; i < p.n; ++i)
            fq_batch_put_row(plane[m], p.stride, i, (const uint8_t*)p.seq[m][i].data(), (int)p.seq[m][i].size());
    }
    uint64_t counts[4] = {p.counts[0], p.counts[1], p.counts[2], p.counts[3]};
    out.clear();
    const One team;
    for (int post = 0; post < 2; ++post) {
        uint64_t* blk[2] = {(uint64_t*)calloc(w[0] ? w[0] : 1, 8), (uint64_t*)calloc(w[1] ? w[1] : 1, 8)};
        if (!post || !p.res.empty()) {
            const int max_len = post && p.paired && p.merge ? 2 * p.stride : p.stride;
            void* shared = malloc(team_bytes(max_len));
            const ora_team_mem mem(shared, max_len);
            uint64_t before[2] = {0, 0};  // the exclusive prefix counts of the post pass
            for (int64_t idx = 0; idx < p.n; ++idx) {
                const int l1 = p.len[0][idx], l2 = p.paired ? p.len[1][idx] : 0;
                const bool ok = l1 <= p.stride && l2 <= p.stride;
                ora_item it[2] = {{0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
                bool take[2] = {false, false};
                if (!post) {
                    if (ok) it[0] = ora_item{1, 0, l1, 0, 0};
                    if (ok && p.paired) it[1] = ora_item{2, 0, l2, 0, 0};
                    take[0] = (counts[0] + (uint64_t)idx) % (uint64_t)p.sampling == 0;
                    take[1] = p.paired && (counts[1] + (uint64_t)idx) % (uint64_t)p.sampling == 0;
                } else if (ok) {
                    ora_post_items pi;
                    if (p.paired)
                        fqkstat::visit_post_pair(p.merge, p.discard, p.res[2 * (size_t)idx], p.res[2 * (size_t)idx + 1], l1, l2, pi);
                    else
                        fqkstat::visit_post_single(p.res[(size_t)idx], l1, pi);
                    it[0] = pi.a, it[1] = pi.b;
                    take[0] = (counts[2] + before[0]) % (uint64_t)p.sampling == 0;
                    take[1] = (counts[3] + before[1]) % (uint64_t)p.sampling == 0;
                    before[0] += it[0].kind != 0, before[1] += it[1].kind != 0;
                }
                for (int st = 0; st < 2; ++st) {
                    if (im[st].set.ntab == 0 || !take[st] || !it[st].kind) continue;
                    const ora_item x = it[st];
                    const int len = x.kind == 3 ? x.n1 + x.n2 : x.n1;
                    if (len > max_len) continue;
                    if (x.kind == 2) {
                        stage_row(team, mem.s, kstat_row(plane[1], p.stride, idx), x.st1, x.n1);
                    } else {
                        stage_row(team, mem.s, kstat_row(plane[0], p.stride, idx), x.st1, x.n1);
                        if (x.kind == 3) stage_revcomp(team, mem.s + x.n1, kstat_row(plane[1], p.stride, idx), x.st2, x.n2);
                    }
                    Inc hit{blk[st], p.eval[st]};
                    scan_read(team, mem, len, im[st].set, hit);
                }
            }
            if (!post) {
                counts[0] += (uint64_t)p.n;
                if (p.paired) counts[1] += (uint64_t)p.n;
            } else {
                counts[2] += before[0], counts[3] += before[1];
            }
            free(shared);
        }
        for (int st = 0; st < 2; ++st) {
            out.insert(out.end(), blk[st], blk[st] + w[st]);
            free(blk[st]);
        }
    }
    free(plane[0]);
    free(plane[1]);
    out.insert(out.end(), counts, counts + 4);
    return true;
}

// ---- --self: Stats::statRead's loop as the reference has it -------------------------------------
struct Plain {
    int sampling, eval;
    uint64_t reads = 0;
    std::map<std::string, std::vector<uint64_t>> m;  // sequence -> count, distribution
    Plain(int s, int e, const std::vector<std::string>& set) : sampling(s), eval(e) {
        for (const std::string& q : set) m[q].assign((size_t)(1 + e), 0);
    }
    void stat(const std::string& s) {
        if (reads % (uint64_t)sampling == 0) {
            const std::set<int> steps = {10, 20, 40, 100, eval - 2 < 150 ? eval - 2 : 150};
            const int len = (int)s.size();
            for (int step : steps)
                for (int j = 0; j < len - step; ++j) {
                    auto it = m.find(s.substr((size_t)j, (size_t)step));
                    if (it == m.end()) continue;
                    ++it->second[0];
                    for (int p = j; p < step + j && p < eval; ++p) ++it->second[(size_t)(1 + p)];
                    j += step;
                }
        }
        ++reads;
    }
    void dump(const std::vector<std::string>& set, std::vector<uint64_t>& out) const {
        for (const std::string& q : set) out.insert(out.end(), m.at(q).begin(), m.at(q).end());
    }
};

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
    for (int eval : {151, 150, 42, 22, 12, 3}) {
        for (int stride : {160, 320}) {
            Pack p;
            p.paired = 1, p.stride = stride, p.eval[0] = eval, p.eval[1] = eval == 151 ? 100 : eval;
            const int fifth = eval - 2 < 150 ? eval - 2 : 150;
            // hot sequences of every step's length (some with bad bytes, some sharing their leading bytes),
            // and of a length no step has
            for (int st = 0; st < 2; ++st) {
                std::set<std::string> hot;
                for (int len : {10, 10, 20, 20, 40, 100, fifth, fifth, 33})
                    if (len >= 1 && len <= stride) hot.insert(rand_seq(len, len % 20 == 0));
                const std::string lead = rand_seq(12, false);
                for (int i = 0; i < 6; ++i) hot.insert(lead + rand_seq(8, false));
                if (st == 1 && stride == 320) hot.clear();  // an empty R2 set
                p.set[st].assign(hot.begin(), hot.end());
            }
            std::vector<std::string> reads;
            for (int L = 0; L <= 12; ++L) reads.push_back(rand_seq(L, false));
            for (int L : {15, 16, 17, 31, 32, 33, 47, 48, 49, stride - 1, stride}) reads.push_back(rand_seq(L, true));
            for (int st = 0; st < 2; ++st)
                for (const std::string& h : p.set[st]) {
                    const int n = (int)h.size();
                    for (int extra : {0, 1, 2})  // len == step, step + 1, step + 2: 0, 1 and 2 windows
                        if (n + extra <= stride) reads.push_back(h + rand_seq(extra, false));
                    if (2 * n + 2 <= stride) {
                        reads.push_back(h + h + "AC");                    // back to back: the second is skipped
                        reads.push_back(h + "T" + h + "AC");              // one byte between: both count
                        reads.push_back(rand_seq(stride - 2 * n - 2, false) + h + "G" + h + "C");
                    }
                }
            for (int i = 0; i < 60; ++i) {  // several hot sequences in one read, at random places
                std::string s = rand_seq((int)(rnd() % (stride + 1)), true);
                for (int k = 0; k < 3; ++k) {
                    const std::vector<std::string>& set = p.set[k & 1].empty() ? p.set[0] : p.set[k & 1];
                    const std::string& h = set[rnd() % set.size()];
                    if (h.size() <= s.size()) s.replace(rnd() % (s.size() - h.size() + 1), h.size(), h);
                }
                reads.push_back(s);
            }
            p.n = (int)reads.size();
            for (int m = 0; m < 2; ++m) {
                p.seq[m].clear(), p.len[m].clear();
                for (int i = 0; i < p.n; ++i) {
                    const std::string& s = reads[(size_t)((i * (m ? 7 : 1) + 3 * m) % p.n)];
                    p.seq[m].push_back(s);
                    p.len[m].push_back((uint16_t)s.size());
                }
            }
            for (int mode = 0; mode < 3; ++mode)  // no -m, -m, -m --discard_unmerged
                for (int sampling : {1, 3, 100}) {
                    p.merge = mode > 0, p.discard = mode > 1, p.sampling = sampling;
                    for (uint64_t& c : p.counts) c = rnd() % 200;
                    p.res.assign((size_t)2 * p.n, fq_read_result{});
                    Plain pl[4] = {Plain(sampling, p.eval[0], p.set[0]), Plain(sampling, p.eval[1], p.set[1]),
                                   Plain(sampling, p.eval[0], p.set[0]), Plain(sampling, p.eval[1], p.set[1])};
                    for (int t = 0; t < 4; ++t) pl[t].reads = p.counts[t];
                    for (int i = 0; i < p.n; ++i) {
                        const std::string &a = p.seq[0][i], &b = p.seq[1][i];
                        pl[0].stat(a);
                        pl[1].stat(b);
                        fq_read_result& r1 = p.res[2 * (size_t)i];
                        fq_read_result& r2 = p.res[2 * (size_t)i + 1];
                        const int la = (int)a.size(), lb = (int)b.size();
                        const uint32_t what = rnd() % 16;
                        r1.start = (uint16_t)(what & 1 && la ? rnd() % 4 % (la + 1) : 0), r1.len = (uint16_t)(la - r1.start - (what & 2 && la - r1.start ? 1 : 0));
                        r2.start = (uint16_t)(what & 4 && lb ? rnd() % 4 % (lb + 1) : 0), r2.len = (uint16_t)(lb - r2.start);
                        if (what == 0) r1.flags |= FQ_RF_NULL;
                        if (what == 1) r2.flags |= FQ_RF_NULL;
                        if (what == 2) r1.flags = r2.flags = FQ_RF_INDEX_FILTERED;
                        if (what == 3) r1.code = FQ_FAIL_QUALITY;
                        if (what == 4) r2.code = FQ_FAIL_LENGTH;
                        if (what == 5) r1.len = (uint16_t)(la + 1 + rnd() % 50);  // a window outside the read: skipped
                        const bool merged = p.merge && what >= 8 && what < 12;
                        if (merged) {
                            r1.flags |= FQ_RF_MERGED | FQ_RF_OVERLAP;
                            r1.m_len1 = (uint16_t)(r1.len - (what == 9 && r1.len ? 1 : 0));
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
                            pl[2].stat(w1.substr(0, r1.m_len1) + rc.substr(w2.size() - r1.m_len2, r1.m_len2));
                        } else if (p.merge) {
                            if (p.discard) continue;
                            if (r1.code == FQ_PASS_FILTER) pl[2].stat(w1);
                            if (r2.code == FQ_PASS_FILTER) pl[3].stat(w2);
                        } else if (r1.code == FQ_PASS_FILTER && r2.code == FQ_PASS_FILTER) {
                            pl[2].stat(w1);
                            pl[3].stat(w2);
                        }
                    }
                    std::vector<uint64_t> want, got;
                    for (int t = 0; t < 4; ++t) pl[t].dump(p.set[t & 1], want);
                    for (int t = 0; t < 4; ++t) want.push_back(pl[t].reads);
                    uint64_t hits = 0;
                    for (int t = 0; t < 4; ++t)
                        for (const auto& e : pl[t].m) hits += e.second[0];
                    if (!run(p, got) || got != want || (sampling == 1 && eval > 12 && !hits)) {
                        ++bad;
                        fprintf(stderr, "ora_sim --self: evalLen %d stride %d mode %d sampling %d differs\n", eval, stride, mode,
                                sampling);
                    }
                }
        }
    }
    printf("ora_sim --self: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--self")) return self_test();
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[12];
    if (fread(h, 4, 12, f) != 12 || h[0] != 0x4f524131) return 2;
    Pack p;
    p.sampling = h[1], p.eval[0] = h[2], p.eval[1] = h[3], p.paired = h[4], p.merge = h[5], p.discard = h[6];
    p.n = h[7], p.stride = h[8];
    if (p.sampling < 1 || p.eval[0] < 3 || p.eval[1] < 3 || p.n < 0 || p.stride <= 0 || (p.stride & 15) || h[10] < 0 || h[11] < 0)
        return 2;
    if (fread(p.counts, 8, 4, f) != 4) return 2;
    for (int st = 0; st < 2; ++st) {
        std::vector<uint32_t> off((size_t)h[10 + st] + 1);
        if (fread(off.data(), 4, off.size(), f) != off.size()) return 2;
        std::string data(off.back(), '\0');
        if (!data.empty() && fread(&data[0], 1, data.size(), f) != data.size()) return 2;
        for (size_t i = 0; i + 1 < off.size(); ++i) p.set[st].push_back(data.substr(off[i], off[i + 1] - off[i]));
    }
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
    if (h[9]) {
        p.res.resize((size_t)p.n * mates);
        if (p.n && fread(p.res.data(), sizeof(fq_read_result), p.res.size(), f) != p.res.size()) return 2;
    }
    fclose(f);
    std::vector<uint64_t> t;
    if (!run(p, t)) return 3;
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(t.data(), 8, t.size(), o) != t.size()) return 2;
    fclose(o);
    return 0;
}
