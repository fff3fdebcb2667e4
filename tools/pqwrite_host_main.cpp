// The element encoders of csrc/parquet_encode.h on the CPU: the body of one DELTA_BINARY_PACKED page, sized and packed the
// way k_pqw_plan, k_pqw_scan and k_pqw_emit of csrc/otto_pqwrite.hip do it (a pass that sizes every block, then a pass that
// ORs the fields into a zeroed image), with every buffer allocated at its exact size. Stand-alone, so it can be built with the
// sanitizers (tests/test_parquet_write_cpu.py: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined).
//
//   pqwrite_host_main < cases  ->  one line per case
//
// A case on stdin: `<stored bytes: 4 or 8> <n>` and then n decimal stored values. Its line on stdout: the body in hex
// (`-` for an empty one cannot happen: a body has at least 5 bytes), or `DOMAIN <row>` for the smallest row whose value
// lies outside the delta domain.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "parquet_encode.h"

// the image as bytes: a word may hang over the end, the bits that would land there are 0 by the writers' contract
struct ByteSink {
    uint8_t* p;
    void or32(uint32_t word, uint32_t bits) {
        for (uint32_t k = 0; k < 4; ++k) {
            const uint8_t b = (uint8_t)(bits >> (8 * k));
            if (b) p[(size_t)word * 4 + k] |= b;
        }
    }
};

struct Block {
    int64_t m;
    uint32_t widths, bytes, off;
};

int main() {
    unsigned phys;
    long long n;
    while (scanf("%u %lld", &phys, &n) == 2) {
        if ((phys != 4 && phys != 8) || n < 0) return 2;
        int64_t* v = new int64_t[(size_t)n];
        long long bad = -1;
        for (long long i = 0; i < n; ++i) {
            if (scanf("%" SCNd64, &v[i]) != 1) return 2;
            if (bad < 0 && !pqe_in_domain(v[i], phys)) bad = i;
        }
        if (bad >= 0) {
            printf("DOMAIN %lld\n", bad);
            delete[] v;
            continue;
        }
        // plan: the figures of every block
        const long long nd_all = n > 0 ? n - 1 : 0;
        std::vector<Block> blocks;
        uint32_t run = pqe_page_header_len((uint32_t)n, n ? v[0] : 0);
        for (long long d0 = 0; d0 < nd_all; d0 += OTTO_PQW_BLOCK) {
            const int nd = nd_all - d0 < OTTO_PQW_BLOCK ? (int)(nd_all - d0) : OTTO_PQW_BLOCK;
            int64_t m = INT64_MAX;
            for (int e = 0; e < nd; ++e) {
                const int64_t d = (int64_t)((uint64_t)v[d0 + e + 1] - (uint64_t)v[d0 + e]);
                if (d < m) m = d;
            }
            uint32_t widths = 0;
            for (int e = 0; e < nd; ++e) {
                const uint64_t rel = (uint64_t)v[d0 + e + 1] - (uint64_t)v[d0 + e] - (uint64_t)m;
                const uint32_t j = (uint32_t)e / OTTO_PQW_MINI_VALUES, w = pqe_bit_length(rel);
                if (w > ((widths >> (8 * j)) & 0xFFu)) widths = (widths & ~(0xFFu << (8 * j))) | w << (8 * j);
            }
            const uint32_t bytes = pqe_block_bytes(m, widths);
            blocks.push_back(Block{m, widths, bytes, run});
            run += bytes;
        }
        // emit: every field into the zeroed image
        uint8_t* body = new uint8_t[run]();
        ByteSink sink = {body};
        uint32_t pos = pqe_put_page_header(sink, 0, (uint32_t)n, n ? v[0] : 0);
        for (size_t b = 0; b < blocks.size(); ++b) {
            const Block& k = blocks[b];
            const long long d0 = (long long)b * OTTO_PQW_BLOCK;
            const int nd = nd_all - d0 < OTTO_PQW_BLOCK ? (int)(nd_all - d0) : OTTO_PQW_BLOCK;
            if (pos != k.off) return 3;
            const uint32_t start = pqe_put_block_header(sink, k.off, k.m, k.widths);
            for (int e = 0; e < nd; ++e)
                pqe_pack_delta(sink, start, (uint32_t)e, (uint64_t)v[d0 + e + 1] - (uint64_t)v[d0 + e] - (uint64_t)k.m, k.widths);
            pos = k.off + k.bytes;
        }
        if (pos != run) return 3;
        for (uint32_t i = 0; i < run; ++i) printf("%02x", body[i]);
        printf("\n");
        delete[] body;
        delete[] v;
    }
    return 0;
}
