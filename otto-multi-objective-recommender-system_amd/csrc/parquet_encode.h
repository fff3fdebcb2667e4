// Scalar element encoders of SPEC-PQWRITE (include/otto_pqwrite.h), as host/device functions: the kernels of
// otto_pqwrite.hip run them, tools/pqwrite_host_main.cpp runs the same code on the CPU under the sanitizers.
//
// Every writer goes through a sink, an object with one member `void or32(uint32_t word, uint32_t bits)` that ORs `bits`
// into 32-bit word `word` of a zeroed little-endian image. The kernels' sink is an LDS array (atomicOr); the host
// program's is a byte buffer of the exact size, so a bit set past the end is seen by the sanitizer. A writer never hands
// a sink a bit that lies outside the bytes its length function counts.
#pragma once
#include <stdint.h>
#include "../../include/otto_pqwrite.h"

#if defined(__HIPCC__)
#define OTTO_PQE_HD __host__ __device__ __forceinline__
#else
#define OTTO_PQE_HD static inline
#endif

// number of bits of v: 0 for 0, 64 for a value with bit 63 set
OTTO_PQE_HD uint32_t pqe_bit_length(uint64_t v) {
    uint32_t n = 0;
    if (v >> 32) n = 32, v >>= 32;
    if (v >> 16) n += 16, v >>= 16;
    if (v >> 8) n += 8, v >>= 8;
    if (v >> 4) n += 4, v >>= 4;
    if (v >> 2) n += 2, v >>= 2;
    if (v >> 1) n += 1, v >>= 1;
    return n + (uint32_t)v;
}

OTTO_PQE_HD uint64_t pqe_zigzag(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }

// bytes of the ULEB128 of v: 1 .. 10
OTTO_PQE_HD uint32_t pqe_uleb_len(uint64_t v) {
    const uint32_t b = pqe_bit_length(v);
    return b ? (b + 6u) / 7u : 1u;
}

template <typename Sink>
OTTO_PQE_HD void pqe_put_byte(Sink& s, uint32_t pos, uint32_t byte) {
    s.or32(pos >> 2, (byte & 0xFFu) << (8u * (pos & 3u)));
}

// ULEB128 of v at byte `pos`; returns the byte behind it
template <typename Sink>
OTTO_PQE_HD uint32_t pqe_put_uleb(Sink& s, uint32_t pos, uint64_t v) {
    while (v >= 0x80u) {
        pqe_put_byte(s, pos++, (uint32_t)(v & 0x7Fu) | 0x80u);
        v >>= 7;
    }
    pqe_put_byte(s, pos++, (uint32_t)v);
    return pos;
}

// the low `w` (0 .. 64) bits of v at bit `bitpos`, LSB first: at most three words
template <typename Sink>
OTTO_PQE_HD void pqe_put_bits(Sink& s, uint32_t bitpos, uint64_t v, uint32_t w) {
    if (w == 0) return;
    if (w < 64u) v &= (1ull << w) - 1ull;
    const uint32_t word = bitpos >> 5, sh = bitpos & 31u;
    const uint64_t a = v << sh;
    const uint32_t c = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
    if ((uint32_t)a) s.or32(word, (uint32_t)a);
    if ((uint32_t)(a >> 32)) s.or32(word + 1u, (uint32_t)(a >> 32));
    if (c) s.or32(word + 2u, c);
}

// The stored value of a column is in the domain of the delta encoding: [0, 2^31) for INT32, [0, 2^62) for INT64
OTTO_PQE_HD bool pqe_in_domain(int64_t v, uint32_t phys_bytes) {
    return v >= 0 && v < (phys_bytes == 4u ? (1ll << 31) : (1ll << 62));
}

// ---- a page's header: block size, miniblocks per block, number of values, first value ------------------------------------
OTTO_PQE_HD uint32_t pqe_page_header_len(uint32_t n, int64_t first) {
    return 2u + 1u + pqe_uleb_len(n) + pqe_uleb_len(pqe_zigzag(n ? first : 0));
}

template <typename Sink>
OTTO_PQE_HD uint32_t pqe_put_page_header(Sink& s, uint32_t pos, uint32_t n, int64_t first) {
    pos = pqe_put_uleb(s, pos, OTTO_PQW_BLOCK);
    pos = pqe_put_uleb(s, pos, OTTO_PQW_MINIBLOCKS);
    pos = pqe_put_uleb(s, pos, n);
    return pqe_put_uleb(s, pos, pqe_zigzag(n ? first : 0));
}

// ---- a block: zigzag ULEB128 of the minimum delta, four width bytes, the miniblocks --------------------------------------
// widths: byte j is the width of miniblock j, 0 for a miniblock that holds no delta
OTTO_PQE_HD uint32_t pqe_block_header_len(int64_t min_delta) { return pqe_uleb_len(pqe_zigzag(min_delta)) + OTTO_PQW_MINIBLOCKS; }

OTTO_PQE_HD uint32_t pqe_block_bytes(int64_t min_delta, uint32_t widths) {
    const uint32_t sum = (widths & 0xFFu) + ((widths >> 8) & 0xFFu) + ((widths >> 16) & 0xFFu) + (widths >> 24);
    return pqe_block_header_len(min_delta) + sum * (OTTO_PQW_MINI_VALUES / 8u);
}

// the widths a block record may hold: none above 64 (then pqe_block_bytes is at most OTTO_PQW_BLOCK_BYTES_MAX)
OTTO_PQE_HD bool pqe_widths_ok(uint32_t widths) {
    return (widths & 0xFFu) <= 64u && ((widths >> 8) & 0xFFu) <= 64u && ((widths >> 16) & 0xFFu) <= 64u && (widths >> 24) <= 64u;
}

template <typename Sink>
OTTO_PQE_HD uint32_t pqe_put_block_header(Sink& s, uint32_t pos, int64_t min_delta, uint32_t widths) {
    pos = pqe_put_uleb(s, pos, pqe_zigzag(min_delta));
    for (uint32_t j = 0; j < OTTO_PQW_MINIBLOCKS; ++j) pqe_put_byte(s, pos++, (widths >> (8u * j)) & 0xFFu);
    return pos;
}

// bit position, counted from the byte the block's miniblocks start at, of delta `e` (0 .. 127) of the block
OTTO_PQE_HD uint32_t pqe_delta_bitpos(uint32_t e, uint32_t widths) {
    const uint32_t j = e / OTTO_PQW_MINI_VALUES;
    uint32_t before = 0;
    for (uint32_t k = 0; k < j; ++k) before += (widths >> (8u * k)) & 0xFFu;
    return before * OTTO_PQW_MINI_VALUES + (e % OTTO_PQW_MINI_VALUES) * ((widths >> (8u * j)) & 0xFFu);
}

// the miniblock packer: delta `e` of the block, as its distance `rel` from the block's minimum, into the block image whose
// miniblocks start at byte `body`
template <typename Sink>
OTTO_PQE_HD void pqe_pack_delta(Sink& s, uint32_t body, uint32_t e, uint64_t rel, uint32_t widths) {
    pqe_put_bits(s, body * 8u + pqe_delta_bitpos(e, widths), rel, (widths >> (8u * (e / OTTO_PQW_MINI_VALUES))) & 0xFFu);
}
