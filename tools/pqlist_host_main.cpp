// SPEC-PQLIST (include/otto_pqlist.h) on the CPU with the scalar pieces the kernels run (csrc/pqlist_levels.h over
// csrc/parquet_decode.h): the page extents, the walk of both level streams with its per-tile checkpoints, the expansion of a
// tile from its checkpoints, the check of every entry, the counts, the bases and the stores, in the order of
// otto_pqlist_levels. Stand-alone, so it can be built with the sanitizers (tests/test_pqlist_cpu.py: g++ -O1 -g
// -fsanitize=address,undefined -fno-sanitize-recover=undefined); every page body, checkpoint array and output is allocated
// at exactly its stated size, so a read or write outside an extent is an error there.
//
//   pqlist_host_main FILE TABLE
//     TABLE: "n_pages n_rows value_base", then n_pages lines of the OTTO_PL_FIELDS of a page record (offsets relative to FILE,
//     the V1 bodies decoded, as otto_amd/parquet.py lays them out)
//     -> "ERR <page> <code>"  or  "OK", the n_rows + 1 offsets, the n_rows null flags, and per page "level_bytes values rows"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pqlist_levels.h"

struct Page {
    uint8_t* body = nullptr;                                // exactly BODY_LEN bytes
    long long len = 0, type = 0, rep_len = 0, def_len = 0, num = 0, flags = 0, chunk_rows = 0, chunk_pages = 0;
    pl_extents f = {};
    std::vector<int64_t> marks;                             // 4 per tile
    long long rows = 0, vals = 0;
};

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s FILE TABLE\n", argv[0]);
        return 2;
    }
    std::FILE* fb = std::fopen(argv[1], "rb");
    std::FILE* t = std::fopen(argv[2], "r");
    if (!fb || !t) {
        std::perror(!fb ? argv[1] : argv[2]);
        return 2;
    }
    std::fseek(fb, 0, SEEK_END);
    const long long n_bytes = std::ftell(fb);
    std::fseek(fb, 0, SEEK_SET);
    std::vector<uint8_t> bytes((size_t)n_bytes);
    if (n_bytes && std::fread(bytes.data(), 1, (size_t)n_bytes, fb) != (size_t)n_bytes) return 2;
    std::fclose(fb);
    long long n_pages = 0, n_rows = 0, value_base = 0;
    if (std::fscanf(t, "%lld %lld %lld", &n_pages, &n_rows, &value_base) != 3) return 2;
    std::vector<Page> pages((size_t)n_pages);
    for (long long p = 0; p < n_pages; ++p) {
        long long r[OTTO_PL_FIELDS];
        for (auto& v : r)
            if (std::fscanf(t, "%lld", &v) != 1) return 2;
        Page& g = pages[(size_t)p];
        if (r[OTTO_PL_BODY_OFF] < 0 || r[OTTO_PL_BODY_LEN] < 0 || r[OTTO_PL_BODY_OFF] + r[OTTO_PL_BODY_LEN] > n_bytes) {
            std::fprintf(stderr, "page %lld outside the file\n", p);
            return 3;
        }
        g.len = r[OTTO_PL_BODY_LEN];
        g.body = new uint8_t[(size_t)(g.len ? g.len : 1)];
        std::memcpy(g.body, bytes.data() + r[OTTO_PL_BODY_OFF], (size_t)g.len);
        g.type = r[OTTO_PL_PAGE_TYPE], g.rep_len = r[OTTO_PL_REP_LEN], g.def_len = r[OTTO_PL_DEF_LEN], g.num = r[OTTO_PL_NUM_VALUES];
        g.flags = r[OTTO_PL_FLAGS], g.chunk_rows = r[OTTO_PL_CHUNK_ROWS], g.chunk_pages = r[OTTO_PL_CHUNK_PAGES];
        g.marks.assign((size_t)(4 * ((g.num + OTTO_PQ_TILE - 1) / OTTO_PQ_TILE)), 0);
    }
    std::fclose(t);
    long long bad_page = -1;
    int bad = 0;
    auto refuse = [&](long long p, int code) {              // the smallest page, inside it the smallest code: atomicMin of page << 8 | code
        if (bad == 0 || p < bad_page || (p == bad_page && code < bad)) bad_page = p, bad = code;
    };
    // k_pl_walk
    for (long long p = 0; p < n_pages; ++p) {
        Page& g = pages[(size_t)p];
        int st = pl_page_extents(g.body, g.len, (int)g.type, g.rep_len, g.def_len, &g.f);
        if (!st) st = pl_walk_stream(g.body, g.f.rep_pos, g.f.rep_end, 1, g.num, g.marks.data());
        if (!st) st = pl_walk_stream(g.body, g.f.def_pos, g.f.def_end, pl_def_width((int)g.flags), g.num, g.marks.data() + 2);
        g.f.ok = st == 0;
        if (st) refuse(p, st);
    }
    // k_pl_tiles, both passes: pass 0 counts and checks, pass 1 stores
    std::vector<int64_t> off((size_t)(n_rows + 1), -1);
    std::vector<uint8_t> null((size_t)n_rows, 0xEE);
    for (int pass = 0; pass < 2; ++pass) {
        long long row = 0, val = 0;                          // the bases of the scans: running sums in page order
        for (long long p = 0; p < n_pages; ++p) {
            Page& g = pages[(size_t)p];
            if (!g.f.ok) continue;
            const int D = pl_def_max((int)g.flags), outer = (int)g.flags & OTTO_PL_F_OUTER_OPTIONAL;
            long long rows = 0, vals = 0;
            for (int64_t lo = 0; lo < g.num; lo += OTTO_PQ_TILE) {
                const int64_t hi = lo + OTTO_PQ_TILE < g.num ? lo + OTTO_PQ_TILE : g.num;
                std::vector<uint8_t> s_rep((size_t)(hi - lo), 0xEE), s_def((size_t)(hi - lo), 0xEE);      // exactly the tile's entries
                const int64_t* mk = g.marks.data() + 4 * (lo / OTTO_PQ_TILE);
                pl_expand(g.body, mk[0], mk[1], g.f.rep_end, 1, lo, hi, s_rep.data(), 0, 1);
                pl_expand(g.body, mk[2], mk[3], g.f.def_end, pl_def_width((int)g.flags), lo, hi, s_def.data(), 0, 1);
                for (int64_t i = lo; i < hi; ++i) {
                    const int r = s_rep[(size_t)(i - lo)], d = s_def[(size_t)(i - lo)];
                    if (pass == 0) {
                        const int e = pl_entry_check(r, d, (int)g.flags, i == 0 && (g.flags & OTTO_PL_F_CHUNK_FIRST));
                        if (e) refuse(p, e);
                    } else if (r == 0 && row + rows < n_rows) {
                        off[(size_t)(row + rows)] = value_base + val + vals;
                        null[(size_t)(row + rows)] = (uint8_t)(outer && d == 0);
                    }
                    rows += r == 0;
                    vals += d == D;
                }
            }
            g.rows = rows, g.vals = vals;
            row += rows, val += vals;
        }
        if (pass == 0) {                                     // k_pl_pages
            off[(size_t)n_rows] = value_base + val;
            for (long long p = 0; p < n_pages; ++p) {
                const Page& g = pages[(size_t)p];
                if (!(g.flags & OTTO_PL_F_CHUNK_FIRST)) continue;
                long long rows = 0;
                for (long long q = p; q < p + g.chunk_pages && q < n_pages; ++q) rows += pages[(size_t)q].rows;
                if (rows != g.chunk_rows && (bad == 0 || bad == OTTO_PL_E_ROWS)) refuse(p, OTTO_PL_E_ROWS);      // only without another violation
            }
        }
    }
    if (bad) {
        std::printf("ERR %lld %d\n", bad_page, bad);
    } else {
        std::printf("OK\n");
        for (size_t i = 0; i < off.size(); ++i) std::printf(i ? " %lld" : "%lld", (long long)off[i]);
        std::printf("\n");
        for (size_t i = 0; i < null.size(); ++i) std::printf(i ? " %d" : "%d", (int)null[i]);
        std::printf("\n");
        for (const Page& g : pages) std::printf("%lld %lld %lld\n", (long long)g.f.def_end, g.vals, g.rows);
    }
    for (Page& g : pages) delete[] g.body;
    return 0;
}
