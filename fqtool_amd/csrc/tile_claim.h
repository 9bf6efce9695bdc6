// How the fast kernels' persistent grid hands tiles to its W waves: a static body and a claimed tail.
// Tiles [0, T0) keep the fixed stride (wave w takes w, w + W, ...), which needs no communication;
// tiles [T0, ntiles) are claimed from a device counter, kClaimTiles at a time, so a wave whose tiles
// were cheap (short polyG tails, few exact overlap checks, a fast CU) takes more of the launch's end
// and the launch does not wait for its slowest waves with most SIMDs empty.  Which wave runs a tile
// changes no output: the accumulator is integer sums and the records are written by pair index.
// Plain arithmetic, shared by the kernels (pe_fast.hip) and the host-side model
// (tools/micro/tile_claim_sim.cpp).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FQ_TC_FN __host__ __device__ inline
#else
#define FQ_TC_FN inline
#endif

// the claimed tail is 1 / kTailDiv of the tiles (at least one round of the grid)
constexpr int kTailDiv = 8;
// tiles per claim (a power of two: a claimed run's end is a mask test).  The claims are same-address
// atomics, which the device serves at some 6 ns each whoever asks: one per tile cannot keep up with
// the 4,096 waves of the headline launch (a tile takes a wave about 24 us), four tiles per claim can.
constexpr int kClaimTiles = 4;
static_assert(kTailDiv >= 1 && kClaimTiles >= 1 && (kClaimTiles & (kClaimTiles - 1)) == 0, "tile claim constants");

// T0: the first claimed tile.  A multiple of W, so the strided part is whole rounds; 0 for a batch
// of less than two rounds.
FQ_TC_FN int fq_static_end(int ntiles, int W) {
    const int want = ntiles / kTailDiv > W ? ntiles / kTailDiv : W;
    const int D = ntiles < want ? ntiles : want;
    return (ntiles - D) / W * W;
}

// the first tile of claim c (c = the counter's value before the wave's increment)
FQ_TC_FN int fq_claimed_tile(int T0, int c) { return T0 + kClaimTiles * c; }

// The tile a wave runs after tile t without asking the counter, or -1 when it has to claim: the next
// round of the strided part, or the next tile of its claimed run.
FQ_TC_FN int fq_next_tile(int t, int T0, int W) {
    if (t + W < T0) return t + W;
    if (kClaimTiles > 1 && t >= T0 && ((t + 1 - T0) & (kClaimTiles - 1)) != 0) return t + 1;
    return -1;
}
