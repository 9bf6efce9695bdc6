// tile_claim_sim.cpp -- the fast kernels' tile hand-out (fqtool_amd/csrc/tile_claim.h) run by W
// simulated waves, under AddressSanitizer / UBSan (tests/test_tile_claim_cpu.py).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/micro/tile_claim_sim.cpp -o tools/micro/tile_claim_sim
//   tile_claim_sim W NTILES SEED
// Every wave runs the kernel's loop (its strided tiles below T0, then claims from one counter), the
// waves advancing in the order of their clocks with seeded random tile durations, so the claims
// interleave as they would on the device.  Fails (exit 1) unless every tile of [0, NTILES) was run
// exactly once and none beyond; prints the makespan next to the fixed stride's for the same durations.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <utility>
#include <vector>

#include "../../fqtool_amd/csrc/tile_claim.h"

namespace {
uint64_t rng_state;
uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: tile_claim_sim W NTILES SEED\n");
        return 2;
    }
    const int W = std::atoi(argv[1]), ntiles = std::atoi(argv[2]);
    rng_state = std::strtoull(argv[3], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    if (W < 1 || ntiles < 0) return 2;
    // a tile's duration: 900 .. 1100, one in 16 up to twice that; every 7th wave runs 3 % slower
    std::vector<uint32_t> dur((size_t)ntiles);
    for (auto& d : dur) {
        d = 900 + rnd() % 201;
        if (rnd() % 16 == 0) d += rnd() % 1000;
    }
    auto cost = [&](int w, int t) -> uint64_t { return dur[(size_t)t] + (w % 7 == 0 ? dur[(size_t)t] * 3 / 100 : 0); };

    const int T0 = fq_static_end(ntiles, W);
    if (T0 < 0 || T0 > ntiles || T0 % W != 0) {
        std::fprintf(stderr, "fq_static_end(%d, %d) = %d\n", ntiles, W, T0);
        return 1;
    }
    std::vector<uint8_t> runs((size_t)ntiles, 0);
    int counter = 0, beyond = 0;
    auto claim = [&]() { return fq_claimed_tile(T0, counter++); };
    // (clock, wave) -> the wave's next tile; the wave with the earliest clock acts next
    typedef std::pair<uint64_t, int> Ev;
    std::priority_queue<Ev, std::vector<Ev>, std::greater<Ev>> q;
    std::vector<int> next((size_t)W);
    for (int w = 0; w < W; ++w) {
        next[(size_t)w] = w >= T0 ? claim() : w;
        q.push(Ev(0, w));
    }
    uint64_t makespan = 0;
    while (!q.empty()) {
        const Ev e = q.top();
        q.pop();
        const int w = e.second, t = next[(size_t)w];
        if (t >= ntiles) {  // the wave's loop ends
            if (e.first > makespan) makespan = e.first;
            continue;
        }
        if (t < 0) {
            ++beyond;
            continue;
        }
        ++runs[(size_t)t];
        const int nx = fq_next_tile(t, T0, W);
        next[(size_t)w] = nx >= 0 ? nx : claim();
        q.push(Ev(e.first + cost(w, t), w));
    }
    int bad = beyond;
    for (int t = 0; t < ntiles; ++t) bad += runs[(size_t)t] != 1;
    // the fixed stride over the same durations
    uint64_t fixed = 0;
    for (int w = 0; w < W && w < ntiles; ++w) {
        uint64_t c = 0;
        for (int t = w; t < ntiles; t += W) c += cost(w, t);
        if (c > fixed) fixed = c;
    }
    std::printf("W %d ntiles %d T0 %d claims %d makespan %" PRIu64 " fixed %" PRIu64 " bad %d\n", W, ntiles, T0, counter, makespan,
                fixed, bad);
    return bad ? 1 : 0;
}
