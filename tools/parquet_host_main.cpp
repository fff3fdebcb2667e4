// SPEC-PARQUET (include/otto_parquet.h) on the CPU with the element decoders the kernels run (csrc/parquet_decode.h): the
// Snappy tag parser and its checks, the varint reader, the hybrid run headers, the bit extraction, the level count and the
// run walk with its per-tile checkpoints. Stand-alone, so it can be built with the sanitizers (tests/test_parquet_cpu.py:
// g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined); every buffer is allocated at exactly its
// stated size, so a read or write outside an extent is an error there.
//
//   parquet_host_main snappy DECLARED FILE [DECLARED FILE ...]
//     -> per stream "ERR <code>"  or  "OK <hex of the output>"
//   parquet_host_main decode FILE TABLE
//     TABLE: "n_pages n_cols", n_cols lines "elem phys zext rows", n_pages lines of the OTTO_PQ_FIELDS of a page record
//     (offsets relative to FILE, as otto_amd/parquet.py walks them)
//     -> "ERR <page> <code>"  or  "OK" and one line per column: its elements as unsigned numbers
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "parquet_decode.h"

static bool read_file(const char* path, uint8_t** out, int64_t* n) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::perror(path);
        return false;
    }
    std::fseek(f, 0, SEEK_END);
    *n = (int64_t)std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    *out = new uint8_t[(size_t)(*n ? *n : 1)];
    const bool ok = !*n || std::fread(*out, 1, (size_t)*n, f) == (size_t)*n;
    std::fclose(f);
    return ok;
}

// the loop of pq_snappy_wave (otto_parquet.hip), one byte at a time; dst holds exactly dst_len bytes
static int snappy(const uint8_t* src, int64_t n, uint8_t* dst, int64_t dst_len) {
    int64_t ip = 0, op = 0;
    int st = pq_snappy_preamble(src, &ip, n, dst_len);
    if (st != PQ_OK) return st;
    while (ip < n) {
        pq_snappy_elem e;
        st = pq_snappy_tag(src, &ip, n, &e);
        if (st != PQ_OK) return st;
        st = pq_snappy_check(e, ip, n, op, dst_len);
        if (st != PQ_OK) return st;
        if (e.kind == 0) {
            std::memcpy(dst + op, src + ip, e.len);
            ip += e.len;
        } else {
            const int64_t s0 = op - (int64_t)e.offset;
            for (int64_t i = 0; i < (int64_t)e.len; ++i) dst[op + i] = dst[s0 + i % (int64_t)e.offset];
        }
        op += e.len;
    }
    return op == dst_len ? PQ_OK : PQ_E_SNAPPY_SHORT;
}

static int run_snappy(int argc, char** argv) {
    for (int i = 2; i + 1 < argc; i += 2) {
        const int64_t declared = std::atoll(argv[i]);
        uint8_t* src = nullptr;
        int64_t n = 0;
        if (!read_file(argv[i + 1], &src, &n)) return 2;
        uint8_t* exact = new uint8_t[(size_t)(n ? n : 1)];      // the input at exactly its size
        std::memcpy(exact, src, (size_t)n);
        delete[] src;
        uint8_t* dst = new uint8_t[(size_t)(declared ? declared : 1)];
        const int st = snappy(exact, n, dst, declared);
        if (st != PQ_OK) {
            std::printf("ERR %d\n", st);
        } else {
            std::printf("OK ");
            for (int64_t k = 0; k < declared; ++k) std::printf("%02x", dst[k]);
            std::printf("\n");
        }
        delete[] dst;
        delete[] exact;
    }
    return 0;
}

struct Body {
    uint8_t* p = nullptr;
    int64_t len = 0;
    int64_t start = -1;
};

static int run_decode(const char* file, const char* table) {
    uint8_t* bytes = nullptr;
    int64_t n_bytes = 0;
    if (!read_file(file, &bytes, &n_bytes)) return 2;
    std::FILE* t = std::fopen(table, "r");
    if (!t) {
        std::perror(table);
        return 2;
    }
    long long n_pages = 0, n_cols = 0;
    if (std::fscanf(t, "%lld %lld", &n_pages, &n_cols) != 2) return 2;
    std::vector<long long> elem((size_t)n_cols), phys((size_t)n_cols), zext((size_t)n_cols), rows((size_t)n_cols);
    std::vector<std::vector<uint64_t>> out((size_t)n_cols);
    for (long long c = 0; c < n_cols; ++c) {
        if (std::fscanf(t, "%lld %lld %lld %lld", &elem[c], &phys[c], &zext[c], &rows[c]) != 4) return 2;
        out[(size_t)c].assign((size_t)rows[c], 0);
    }
    std::vector<long long> rec((size_t)(n_pages * OTTO_PQ_FIELDS));
    for (auto& v : rec)
        if (std::fscanf(t, "%lld", &v) != 1) return 2;
    std::fclose(t);
    std::vector<Body> body((size_t)n_pages);
    long long bad_page = -1;
    int bad = PQ_OK;
    for (long long p = 0; p < n_pages && bad == PQ_OK; ++p) {
        const long long* r = &rec[(size_t)(p * OTTO_PQ_FIELDS)];
        const long long type = r[OTTO_PQ_PAGE_TYPE], c = r[OTTO_PQ_COL_SLOT], nv = r[OTTO_PQ_NUM_VALUES];
        const long long lev = type == 3 ? r[OTTO_PQ_DEF_LEN] + r[OTTO_PQ_REP_LEN] : 0;
        if (r[OTTO_PQ_SRC_OFF] < 0 || r[OTTO_PQ_SRC_OFF] + r[OTTO_PQ_COMP_SIZE] > n_bytes || lev > r[OTTO_PQ_COMP_SIZE] ||
            lev > r[OTTO_PQ_UNCOMP_SIZE]) {
            std::fprintf(stderr, "page %lld outside the file\n", p);
            return 3;
        }
        Body& b = body[(size_t)p];
        int st = PQ_OK;
        if (r[OTTO_PQ_IS_COMPRESSED]) {
            b.len = r[OTTO_PQ_UNCOMP_SIZE] - lev;
            b.p = new uint8_t[(size_t)(b.len ? b.len : 1)];
            const int64_t sn = r[OTTO_PQ_COMP_SIZE] - lev;
            uint8_t* src = new uint8_t[(size_t)(sn ? sn : 1)];
            std::memcpy(src, bytes + r[OTTO_PQ_SRC_OFF] + lev, (size_t)sn);
            st = snappy(src, sn, b.p, b.len);
            delete[] src;
        } else {
            b.len = r[OTTO_PQ_COMP_SIZE] - lev;
            b.p = new uint8_t[(size_t)(b.len ? b.len : 1)];
            std::memcpy(b.p, bytes + r[OTTO_PQ_SRC_OFF] + lev, (size_t)b.len);
            if (r[OTTO_PQ_COMP_SIZE] != r[OTTO_PQ_UNCOMP_SIZE]) st = PQ_E_SIZE;
        }
        const bool plain = type == 2 || r[OTTO_PQ_ENCODING] == 0;
        std::vector<int64_t> marks((size_t)(2 * ((nv + OTTO_PQ_TILE - 1) / OTTO_PQ_TILE) + 2), 0);
        int width = 0;
        if (st == PQ_OK && type == 2) {
            b.start = 0;
            if (b.len != nv * phys[c]) st = PQ_E_SIZE;
        } else if (st == PQ_OK) {
            st = pq_v1_values_start(b.p, b.len, type == 0 && r[OTTO_PQ_DEF_LEN] == -1, nv, &b.start);
            if (st == PQ_OK && plain && b.len - b.start != nv * phys[c]) st = PQ_E_SIZE;
            if (st == PQ_OK && !plain) st = pq_walk_runs(b.p, b.start, b.len, nv, marks.data(), &width);
        }
        if (st == PQ_OK && type != 2) {                    // k_pq_decode, tile by tile from the checkpoints
            const long long d = r[OTTO_PQ_DICT_SLOT];
            if (r[OTTO_PQ_OUT_ROW] < 0 || r[OTTO_PQ_OUT_ROW] + nv > rows[c] || (!plain && (d < 0 || d >= p))) {
                std::fprintf(stderr, "page %lld: rows or dictionary slot outside the table\n", p);
                return 3;
            }
            for (int64_t lo = 0; lo < nv && st == PQ_OK; lo += OTTO_PQ_TILE) {
                const int64_t hi = lo + OTTO_PQ_TILE < nv ? lo + OTTO_PQ_TILE : nv;
                if (plain) {
                    for (int64_t v = lo; v < hi; ++v)
                        out[(size_t)c][(size_t)(r[OTTO_PQ_OUT_ROW] + v)] =
                            (uint64_t)pq_widen(pq_load_le(b.p, b.start + v * phys[c], (int)phys[c]), (int)phys[c], zext[c] != 0);
                    continue;
                }
                const Body& dict = body[(size_t)d];
                const int64_t dn = rec[(size_t)(d * OTTO_PQ_FIELDS + OTTO_PQ_NUM_VALUES)];
                int64_t pos = marks[(size_t)(2 * (lo / OTTO_PQ_TILE))], seen = marks[(size_t)(2 * (lo / OTTO_PQ_TILE) + 1)];
                while (seen < hi && st == PQ_OK) {
                    pq_run run;
                    if (!pq_run_header(b.p, &pos, b.len, width, &run)) {
                        st = PQ_E_RUNS;
                        break;
                    }
                    const int64_t last = seen + (int64_t)run.count;
                    for (int64_t v = seen > lo ? seen : lo; v < (last < hi ? last : hi); ++v) {
                        const uint32_t idx = run.packed ? pq_bits(b.p, run.data, b.len, v - seen, width) : run.value;
                        if ((int64_t)idx >= dn) {
                            st = PQ_E_INDEX;
                            break;
                        }
                        out[(size_t)c][(size_t)(r[OTTO_PQ_OUT_ROW] + v)] =
                            (uint64_t)pq_widen(pq_load_le(dict.p, (int64_t)idx * phys[c], (int)phys[c]), (int)phys[c], zext[c] != 0);
                    }
                    seen = last;
                }
            }
        }
        if (st != PQ_OK) {
            bad = st;
            bad_page = p;
        }
    }
    for (auto& b : body) delete[] b.p;
    delete[] bytes;
    if (bad != PQ_OK) {
        std::printf("ERR %lld %d\n", bad_page, bad);
        return 0;
    }
    std::printf("OK\n");
    for (long long c = 0; c < n_cols; ++c) {
        const uint64_t mask = elem[c] == 8 ? ~0ull : (1ull << (8 * elem[c])) - 1;
        for (size_t i = 0; i < out[(size_t)c].size(); ++i) std::printf(i ? " %llu" : "%llu", (unsigned long long)(out[(size_t)c][i] & mask));
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "snappy") && argc % 2 == 0) return run_snappy(argc, argv);
    if (argc == 4 && !std::strcmp(argv[1], "decode")) return run_decode(argv[2], argv[3]);
    std::fprintf(stderr, "usage: %s snappy DECLARED FILE [DECLARED FILE ...] | decode FILE TABLE\n", argv[0]);
    return 2;
}
