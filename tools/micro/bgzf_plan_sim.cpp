// bgzf_plan_sim.cpp -- the BGZF window planner (fqtool_amd/host/bgzf_plan.h) over a member table,
// under AddressSanitizer / UBSan (tests/test_bgzf_plan_cpu.py).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tools/micro/bgzf_plan_sim.cpp -o tools/micro/bgzf_plan_sim
//   bgzf_plan_sim TABLE CALL CAP MEMBER_CAP WANT
// TABLE: one line "data clen isize crc" per member (decimal).  Prints "fits 0|1", then, if it fits,
// one line "start n first end skip comp_off comp_bytes" per window, each asked for WANT bytes at
// the end of the one before, until the stream's end.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../../fqtool_amd/host/bgzf_plan.h"

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: bgzf_plan_sim TABLE CALL CAP MEMBER_CAP WANT\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<BgzfChainMember> ms;
    unsigned long long data;
    unsigned clen, isize, crc;
    while (std::fscanf(f, "%llu %u %u %u", &data, &clen, &isize, &crc) == 4) ms.push_back(BgzfChainMember{data, clen, isize, crc});
    std::fclose(f);
    const uint64_t call = std::strtoull(argv[2], nullptr, 10), cap = std::strtoull(argv[3], nullptr, 10);
    const uint64_t want = std::strtoull(argv[5], nullptr, 10);
    const BgzfPlanner pl(ms, call, cap, (uint32_t)std::strtoul(argv[4], nullptr, 10));
    const bool fits = pl.fits();
    std::printf("fits %d\n", fits ? 1 : 0);
    if (!fits) return 0;
    for (uint64_t s = 0; s < pl.size();) {
        BgzfWindowPlan w;
        if (!pl.next(s, want, w) || w.n == 0) {
            std::fprintf(stderr, "no window at %" PRIu64 " although the chain fits\n", s);
            return 1;
        }
        std::printf("%" PRIu64 " %" PRIu64 " %zu %zu %u %" PRIu64 " %" PRIu64 "\n", w.start, w.n, w.first, w.end, w.skip, w.comp_off,
                    w.comp_bytes);
        s = w.start + w.n;
    }
    BgzfWindowPlan w;  // at the end, and for a reader that wants nothing: the empty window
    if (!pl.next(pl.size(), want, w) || w.n || w.first != w.end || !pl.next(0, 0, w) || w.n || w.first != w.end) return 1;
    return 0;
}
