// The device helpers of csrc/deflate.h on the CPU: the length and distance symbols of every match length 3..258 and every
// distance 1..32,768 against the tables of RFC 1951 section 3.2.5, and the CRC-32 of 64 pieces joined by x^(8 len) products
// (as k_deflate_plan joins its lanes' pieces) against the CRC taken byte after byte. Stand-alone, so it can be built with
// the sanitizers (tests/test_deflate_cpu.py: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined).
//
//   deflate_host_main  ->  "OK" and exit code 0, or the first values that differ
#include <cstdint>
#include <cstdio>
#include <vector>

#include "deflate.h"

using namespace otto;

static const int LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const int LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const int DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                  4097, 6145, 8193, 12289, 16385, 24577};
static const int DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

static uint32_t crc_serial(const std::vector<uint8_t>& x) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint8_t b : x) c = df_crc_byte(c, b);
    return ~c;
}

int main() {
    for (uint32_t length = 3; length <= 258; ++length) {
        int s = 28;
        if (length != 258)
            for (s = 27; LEN_BASE[s] > (int)length; --s) {}
        uint32_t sym, bits, val;
        df_len_symbol(length, &sym, &bits, &val);
        if (sym != 257u + s || bits != (uint32_t)LEN_EXTRA[s] || val != length - LEN_BASE[s] || df_len_extra(sym) != bits) {
            printf("length %u: symbol %u, %u extra bits, value %u\n", length, sym, bits, val);
            return 1;
        }
    }
    for (uint32_t dist = 1; dist <= 32768; ++dist) {
        int s = 29;
        for (; DIST_BASE[s] > (int)dist; --s) {}
        uint32_t sym, bits, val;
        df_dist_symbol(dist, &sym, &bits, &val);
        if (sym != (uint32_t)s || bits != (uint32_t)DIST_EXTRA[s] || val != dist - DIST_BASE[s] || df_dist_extra(sym) != bits) {
            printf("distance %u: symbol %u, %u extra bits, value %u\n", dist, sym, bits, val);
            return 1;
        }
    }
    const std::vector<uint8_t> check = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
    if (crc_serial(check) != 0xCBF43926u) {
        printf("CRC-32 of 123456789 is %08x\n", crc_serial(check));
        return 1;
    }
    uint64_t state = 1;
    for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 1000u, 65535u, 65536u}) {
        std::vector<uint8_t> x(n);
        for (auto& v : x) v = (uint8_t)((state = state * 6364136223846793005ull + 1442695040888963407ull) >> 56);
        const uint32_t piece = (n + 63u) / 64u;
        uint32_t crc = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t lo = lane * piece < n ? lane * piece : n, hi = lo + piece < n ? lo + piece : n;
            uint32_t c = 0xFFFFFFFFu;
            for (uint32_t i = lo; i < hi; ++i) c = df_crc_byte(c, x[i]);
            crc ^= hi > lo ? df_crc_shift(~c, n - hi) : 0u;
        }
        if (crc != crc_serial(x)) {
            printf("n = %u: joined %08x, serial %08x\n", n, crc, crc_serial(x));
            return 1;
        }
    }
    printf("OK\n");
    return 0;
}
