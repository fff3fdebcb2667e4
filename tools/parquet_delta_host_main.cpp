// The DELTA_BINARY_PACKED helpers of csrc/parquet_decode.h on the CPU: one page body walked by pq_delta_walk and unpacked
// the way k_pq_delta_sum, k_pq_delta_scan and k_pq_delta_out of csrc/otto_parquet.hip do it (a pass that sums every block, a
// scan over the sums, a pass that scans inside each block; 64 values at a time through the two half-wave cursors), with the
// body and the block records allocated at their exact sizes. Stand-alone, so it can be built with the sanitizers
// (tests/test_parquet_delta_cpu.py: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined).
//
//   parquet_delta_host_main < cases  ->  one line per case
//
// A case on stdin: `<physical bytes: 4 or 8> <num_values> <the body in hex, - for an empty one>`. Its line on stdout: the
// values as unsigned decimals modulo 2^(8 x physical bytes), `-` for none, or `REFUSED <PQ_E_* code>`.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "parquet_decode.h"

struct Block {
    int64_t widths, min_delta;
    uint64_t base;
};

// the 64 values i0 .. i0 + 63 of a block, as pq_delta_chunk of otto_parquet.hip gives them to the 64 lanes
static void chunk(const uint8_t* b, const Block& k, int mv, int64_t i0, int64_t in_block, pq_delta_cursor* cur, uint64_t* out) {
    const pq_delta_cursor lo = *cur;
    pq_delta_advance(b, k.widths, mv, cur);
    const pq_delta_cursor hi = *cur;
    pq_delta_advance(b, k.widths, mv, cur);
    for (int lane = 0; lane < 64; ++lane) {
        const pq_delta_cursor c = lane < 32 ? lo : hi;
        out[lane] = i0 + lane >= in_block ? 0 : (uint64_t)k.min_delta + pq_delta_field(b, c.off, c.k + (lane & 31), b[k.widths + c.j]);
    }
}

int main() {
    unsigned phys;
    long long n;
    static char hex[1 << 22];
    while (scanf("%u %lld %4194303s", &phys, &n, hex) == 3) {
        if ((phys != 4 && phys != 8) || n < 0) return 2;
        const size_t len = strcmp(hex, "-") == 0 ? 0 : strlen(hex) / 2;
        uint8_t* body = new uint8_t[len];                     // exact size: a read past the body is the sanitizer's
        for (size_t i = 0; i < len; ++i) {
            unsigned v;
            if (sscanf(hex + 2 * i, "%2x", &v) != 1) return 2;
            body[i] = (uint8_t)v;
        }
        const int64_t slots = n > 1 ? (n - 1 + 127) / 128 : 0;
        Block* blocks = new Block[(size_t)slots];
        pq_delta_head h = {};
        const int st = pq_delta_walk(body, 0, (int64_t)len, n, (int)phys, &h, (int64_t*)blocks, (int)(sizeof(Block) / 8));
        if (st != PQ_OK) {
            printf("REFUSED %d\n", st);
        } else {
            uint64_t* out = new uint64_t[(size_t)n];
            uint64_t lanes[64];
            for (int64_t b = 0; b < h.n_blocks; ++b) {        // k_pq_delta_sum
                const int64_t left = n - 1 - b * h.B, in_block = left < h.B ? left : h.B;
                pq_delta_cursor cur = {blocks[b].widths + h.M, 0, 0};
                uint64_t sum = 0;
                for (int64_t i0 = 0; i0 < in_block; i0 += 64) {
                    chunk(body, blocks[b], h.mv, i0, in_block, &cur, lanes);
                    for (int l = 0; l < 64; ++l) sum += lanes[l];
                }
                blocks[b].base = sum;
            }
            uint64_t carry = (uint64_t)h.first;               // k_pq_delta_scan
            if (n > 0) out[0] = carry;
            for (int64_t b = 0; b < h.n_blocks; ++b) {
                const uint64_t s = blocks[b].base;
                blocks[b].base = carry;
                carry += s;
            }
            for (int64_t b = 0; b < h.n_blocks; ++b) {        // k_pq_delta_out
                const int64_t left = n - 1 - b * h.B, in_block = left < h.B ? left : h.B;
                pq_delta_cursor cur = {blocks[b].widths + h.M, 0, 0};
                uint64_t run = blocks[b].base;
                for (int64_t i0 = 0; i0 < in_block; i0 += 64) {
                    chunk(body, blocks[b], h.mv, i0, in_block, &cur, lanes);
                    for (int l = 0; l < 64 && i0 + l < in_block; ++l) {
                        run += lanes[l];
                        out[1 + b * h.B + i0 + l] = run;
                    }
                }
            }
            if (n == 0) printf("-");
            for (int64_t i = 0; i < n; ++i)
                printf(i ? " %" PRIu64 : "%" PRIu64, phys == 4 ? (uint64_t)(uint32_t)out[i] : out[i]);
            printf("\n");
            delete[] out;
        }
        delete[] blocks;
        delete[] body;
    }
    return 0;
}
