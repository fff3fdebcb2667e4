// Device helpers of otto_deflate.hip (SPEC-DEFLATE, include/otto_deflate.h): the symbol arithmetic of RFC 1951 section
// 3.2.5 without tables, CRC-32 by bits and the joining of partial CRCs. No device intrinsics, so tools/deflate_host_main.cpp
// runs the same functions on the CPU under the sanitizers (tests/test_deflate_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OTTO_DEFLATE_HD __host__ __device__ __forceinline__
#else
#define OTTO_DEFLATE_HD static inline
#endif

namespace otto {

// ---- RFC 1951 section 3.2.5 ---------------------------------------------------------------------------------------------
// match length 3..258 -> literal/length symbol 257..285, number of extra bits, their value
OTTO_DEFLATE_HD void df_len_symbol(uint32_t length, uint32_t* sym, uint32_t* ebits, uint32_t* eval) {
    const uint32_t l = length - 3u;
    if (length >= 258u) { *sym = 285u, *ebits = 0u, *eval = 0u; return; }
    if (l < 8u) { *sym = 257u + l, *ebits = 0u, *eval = 0u; return; }
    const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
    *sym = 257u + 4u * (e + 1u) + ((l >> e) & 3u);
    *ebits = e;
    *eval = l & ((1u << e) - 1u);
}
// distance 1..32768 -> distance symbol 0..29, number of extra bits, their value
OTTO_DEFLATE_HD void df_dist_symbol(uint32_t dist, uint32_t* sym, uint32_t* ebits, uint32_t* eval) {
    const uint32_t d = dist - 1u;
    if (d < 4u) { *sym = d, *ebits = 0u, *eval = 0u; return; }
    const uint32_t k = 31u - (uint32_t)__builtin_clz(d), e = k - 1u;
    *sym = 2u * k + ((d >> e) & 1u);
    *ebits = e;
    *eval = d & ((1u << e) - 1u);
}
OTTO_DEFLATE_HD uint32_t df_len_extra(uint32_t sym) { return sym >= 265u && sym < 285u ? (sym - 261u) >> 2 : 0u; }
OTTO_DEFLATE_HD uint32_t df_dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }

// ---- CRC-32 (reflected, polynomial 0xEDB88320) ----------------------------------------------------------------------------
OTTO_DEFLATE_HD uint32_t df_crc_byte(uint32_t c, uint32_t b) {
    c ^= b;
    for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    return c;
}
// a * b modulo the polynomial; bit 31 is the coefficient of x^0
OTTO_DEFLATE_HD uint32_t df_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
    }
    return p;
}
// x^e modulo the polynomial
OTTO_DEFLATE_HD uint32_t df_crc_xpow(uint64_t e) {
    uint32_t p = 0x80000000u, sq = 0x40000000u;
    for (; e; e >>= 1) {
        if (e & 1u) p = df_crc_mul(sq, p);
        sq = df_crc_mul(sq, sq);
    }
    return p;
}
// CRC of A||B from crc(A), crc(B) and the length of B: crc(A) * x^(8 len(B)) + crc(B)
OTTO_DEFLATE_HD uint32_t df_crc_shift(uint32_t crc_a, uint64_t len_b) { return df_crc_mul(df_crc_xpow(8u * len_b), crc_a); }

}  // namespace otto
