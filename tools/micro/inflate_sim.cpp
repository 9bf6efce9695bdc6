// inflate_sim.cpp -- inflate.hip's member routine (fqtool_amd/csrc/inflate_core.h) run on the host:
// the wave's lane-parallel blocks become loops over the 64 lanes (no such block reads what another
// lane writes in it, so the order of the lanes does not matter), lane variables become arrays, and
// heap blocks of the exact sizes stand for the wave's LDS, the member's payload and its output, so
// a sanitizer sees every access the kernel would make (CPU only).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread tools/micro/inflate_sim.cpp -o tools/micro/inflate_sim
//   tools/micro/inflate_sim IN.bgzf [OUT]   one line per member: index status produced crc32-of-the-produced-bytes
//                                           (OUT: every member's isize bytes, 0xA5 after the produced ones)
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __host__
#define __device__
#define FQ_INFL_HOST_SIM
#define FQ_LANES(l) for (uint32_t l = 0; l < 64; ++l)
#define FQ_LANEVAR(T, name) T name[64]
#define FQ_LV(name, l) name[l]
#define FQ_LANE_GET(name, k) name[k]
static inline uint32_t fq_uni(uint32_t v) { return v; }
static inline void fq_wave_sync() {}
static inline uint32_t fq_wave_xor(uint32_t v) { return v; }  // (the lane loop has summed already)
static inline void fq_lds_add(uint32_t* p, uint32_t v) { *p += v; }
#include "../../fqtool_amd/csrc/inflate_core.h"

static uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
static uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    { uint8_t b[65536]; size_t k; while ((k = fread(b, 1, sizeof b, f)) > 0) file.insert(file.end(), b, b + k); }
    fclose(f);
    FILE* o = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    uint8_t* lds = (uint8_t*)aligned_alloc(16, FQ_IL_TOTAL);
    memset(lds, 0xEE, FQ_IL_TOTAL);  // (whatever an earlier workgroup left)
    size_t idx = 0;
    for (size_t at = 0; at < file.size(); ++idx) {
        const uint8_t* h = file.data() + at;
        // the members the tests write: 18-byte header with the BC subfield first
        if (file.size() - at < 28 || h[0] != 0x1f || h[1] != 0x8b || h[3] != 4 || le16(h + 10) != 6 || h[12] != 'B' || h[13] != 'C') return 3;
        const size_t bsize = le16(h + 16) + 1;
        if (bsize < 26 || bsize > file.size() - at) return 3;
        const uint32_t in_len = (uint32_t)(bsize - 26), crc = le32(h + bsize - 8), isize = le32(h + bsize - 4);
        if (isize > FQ_INFLATE_MAX_BYTES) return 4;  // (the host side refuses these before any launch)
        // exact-size blocks: a read past the payload or a write past isize is caught
        uint8_t* in = (uint8_t*)malloc(in_len ? in_len : 1);
        memcpy(in, h + 18, in_len);
        uint8_t* dst = (uint8_t*)malloc(isize ? isize : 1);
        memset(dst, 0xA5, isize ? isize : 1);
        uint32_t produced = 0;
        const uint32_t st = fq_inflate_one(lds, in_len ? in : in + 1, in_len, isize, crc, isize ? dst : dst + 1, produced);
        if (produced > isize) return 5;
        printf("%zu %u %u %08x\n", idx, st, produced, fq_crc_bytes(dst, produced));
        if (o) fwrite(dst, 1, isize, o);
        free(in);
        free(dst);
        at += bsize;
    }
    if (o) fclose(o);
    free(lds);
    return 0;
}
