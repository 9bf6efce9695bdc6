// crc_core.h -- CRC32 (reflected, polynomial 0xedb88320) pieces shared by deflate_core.h and
// inflate_core.h: a chunk's CRC, and the multiplication that moves it to its place in a longer
// message, so that chunks can be summed in parallel and XORed together.
#pragma once
#include <stdint.h>

// a(x) * b(x) modulo the polynomial, operands bit-reflected (x^0 is bit 31)
__host__ __device__ inline uint32_t fq_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
// x^(8 * bytes) modulo the polynomial (bytes < 2^17)
__host__ __device__ inline uint32_t fq_crc_xpow8(uint32_t bytes) {
    uint32_t r = 0x80000000u;  // x^0
    uint32_t b = 0x00800000u;  // x^8
    for (int i = 0; i < 17; ++i) {
        if ((bytes >> i) & 1) r = fq_crc_mul(r, b);
        b = fq_crc_mul(b, b);
    }
    return r;
}
__host__ __device__ inline uint32_t fq_crc_bytes(const uint8_t* p, uint32_t n) {
    uint32_t c = 0xffffffffu;
    for (uint32_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1)));
    }
    return ~c;
}
