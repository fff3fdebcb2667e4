// Level decode of Parquet list columns for MI355X (gfx950): the repetition / definition levels of a three-level LIST column
// -> row offsets and null flags. C-ABI and SPEC-PQLIST in include/otto_pqlist.h; the scalar pieces
// (page extents, run walk, expansion, the check of one entry) are the host/device functions of pqlist_levels.h over the run
// headers of parquet_decode.h, which tools/pqlist_host_main.cpp runs on the CPU under the sanitizers.
//
//   k_pl_walk    one lane per page: the V1 length prefixes (or the V2 header lengths), then every run header of both level
//                streams, each checked against the stream's extent; one (header byte, first entry) checkpoint per stream
//                and OTTO_PQ_TILE entries, and where the values start.
//   k_pl_tiles   one wave per tile of OTTO_PQ_TILE entries: both streams are expanded from the tile's checkpoints into
//                2 KiB of LDS (the two streams have unrelated run boundaries; side by side in LDS an entry's two levels
//                meet in one lane), then 16 steps of 64 entries check the levels and ballot rep == 0 and def == D.
//                Pass 0 leaves the tile's row and value counts; pass 1, behind the scans, stores off / null of the rows
//                that start in the tile from the popcounts below the lane.
//   scan.h       two exclusive scans of the tile counts: bases in page order, which is chunk and file order.
//   k_pl_pages   one lane per page: level bytes, values and rows of the page for the host; the row count of every chunk
//                against its row group's; off[n_rows].
#include <vector>

#include "common.h"
#include "wave.h"
#include "scan.h"
#include "pqlist_levels.h"

namespace otto {

constexpr int PL_THREADS = 256;
constexpr int PL_WAVES = PL_THREADS / WAVE;
constexpr int PL_TILE = OTTO_PQ_TILE;

struct PlPage {
    int64_t body, body_len, rep_len, def_len, num, tile0, chunk_rows, chunk_pages;
    int32_t type, flags;
};

using PlInfo = pl_extents;                                 // k_pl_walk's verdict on a page; offsets relative to its body

struct PlWs {
    unsigned long long* err;      // page << 8 | reason of the smallest violating page, ~0 without one
    PlPage* pages;                // [n_pages]
    PlInfo* infos;                // [n_pages]
    int64_t* marks;               // [4 * tiles]  rep (byte, entry), def (byte, entry)
    uint64_t* n_row;              // [tiles]
    uint64_t* n_val;              // [tiles]
    uint64_t* row_base;           // [tiles + 1]
    uint64_t* val_base;           // [tiles + 1]
    uint64_t* partial;            // scan.h
    int64_t* page_out;            // [3 * n_pages]
};

static size_t pl_layout(int64_t n_pages, int64_t tiles, char* base, PlWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    PlWs t;
    t.err = (unsigned long long*)take(8);
    t.pages = (PlPage*)take((size_t)n_pages * sizeof(PlPage));
    t.infos = (PlInfo*)take((size_t)n_pages * sizeof(PlInfo));
    t.marks = (int64_t*)take((size_t)tiles * 32);
    t.n_row = (uint64_t*)take((size_t)tiles * 8);
    t.n_val = (uint64_t*)take((size_t)tiles * 8);
    t.row_base = (uint64_t*)take((size_t)(tiles + 1) * 8);
    t.val_base = (uint64_t*)take((size_t)(tiles + 1) * 8);
    t.partial = (uint64_t*)take(scan_partial_bytes(tiles));
    t.page_out = (int64_t*)take((size_t)n_pages * 24);
    if (w) *w = t;
    return o;
}

static const char* pl_reason(int64_t r) {
    static const char* const names[] = {"no violation", "level lengths run past the page body", "malformed run header in a level stream",
                                        "level stream ends before num_values entries", "level stream runs past num_values entries",
                                        "a level above its maximum", "repetition level 1 on an entry without an element",
                                        "a null element", "the column chunk opens with repetition level 1",
                                        "the count of rows differs from the row group's num_rows"};
    return r >= 0 && r <= OTTO_PL_E_ROWS ? names[r] : "?";
}

__global__ __launch_bounds__(WAVE) void k_pl_walk(const uint8_t* __restrict__ bytes, const PlPage* __restrict__ pages, int64_t n_pages,
                                                  PlInfo* __restrict__ infos, int64_t* __restrict__ marks, unsigned long long* err) {
    const int64_t p = (int64_t)blockIdx.x * WAVE + threadIdx.x;
    if (p >= n_pages) return;
    const PlPage pg = pages[p];
    const uint8_t* b = bytes + pg.body;
    PlInfo f = {};
    int st = pl_page_extents(b, pg.body_len, pg.type, pg.rep_len, pg.def_len, &f);
    if (!st) st = pl_walk_stream(b, f.rep_pos, f.rep_end, 1, pg.num, marks + 4 * pg.tile0);
    if (!st) st = pl_walk_stream(b, f.def_pos, f.def_end, pl_def_width(pg.flags), pg.num, marks + 4 * pg.tile0 + 2);
    f.ok = st == 0;
    if (st) atomicMin(err, (unsigned long long)p << 8 | (unsigned long long)st);
    infos[p] = f;
}

template <int PASS>
__global__ __launch_bounds__(PL_THREADS) void k_pl_tiles(const uint8_t* __restrict__ bytes, const PlPage* __restrict__ pages, int64_t n_pages,
                                                         int64_t n_tiles, const PlInfo* __restrict__ infos, const int64_t* __restrict__ marks,
                                                         uint64_t* __restrict__ n_row, uint64_t* __restrict__ n_val,
                                                         const uint64_t* __restrict__ row_base, const uint64_t* __restrict__ val_base,
                                                         int64_t* __restrict__ off, uint8_t* __restrict__ null, int64_t n_rows,
                                                         int64_t value_base, unsigned long long* err) {
    __shared__ uint8_t s_lev[PL_WAVES][2][PL_TILE];
    const int64_t tile = (int64_t)blockIdx.x * PL_WAVES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;                             // wave-uniform
    const int lane = (int)lane_id();
    int64_t lo_p = 0, hi_p = n_pages - 1;                    // the last page whose first tile is <= tile
    while (lo_p < hi_p) {
        const int64_t mid = (lo_p + hi_p + 1) >> 1;
        if (pages[mid].tile0 <= tile) lo_p = mid; else hi_p = mid - 1;
    }
    const int64_t p = lo_p;
    const PlPage pg = pages[p];
    const PlInfo f = infos[p];
    if (!f.ok) {
        if (PASS == 0 && lane == 0) n_row[tile] = n_val[tile] = 0;
        return;
    }
    const uint8_t* b = bytes + pg.body;
    const int64_t t = tile - pg.tile0;
    const int64_t lo = t * PL_TILE, hi = lo + PL_TILE < pg.num ? lo + PL_TILE : pg.num;
    const int D = pl_def_max(pg.flags), outer = pg.flags & OTTO_PL_F_OUTER_OPTIONAL;
    uint8_t* s_rep = s_lev[threadIdx.x >> 6][0];
    uint8_t* s_def = s_lev[threadIdx.x >> 6][1];
    const int64_t* mk = marks + 4 * tile;
    pl_expand(b, mk[0], mk[1], f.rep_end, 1, lo, hi, s_rep, lane, WAVE);
    pl_expand(b, mk[2], mk[3], f.def_end, pl_def_width(pg.flags), lo, hi, s_def, lane, WAVE);
    wave_lds_sync();
    const unsigned long long below = (1ull << lane) - 1;
    int64_t rows = 0, vals = 0;
    int bad = 255;
    for (int64_t i0 = lo; i0 < hi; i0 += WAVE) {
        const int64_t i = i0 + lane;
        const bool live = i < hi;
        const int r = live ? s_rep[i - lo] : 1, d = live ? s_def[i - lo] : 0;
        const unsigned long long m_row = __ballot(live && r == 0), m_val = __ballot(live && d == D);
        if (PASS == 0) {
            if (live) {
                const int e = pl_entry_check(r, d, pg.flags, i == 0 && (pg.flags & OTTO_PL_F_CHUNK_FIRST));
                if (e && e < bad) bad = e;
            }
        } else if (live && r == 0) {
            const int64_t row = (int64_t)row_base[tile] + rows + __popcll(m_row & below);
            if (row < n_rows) {                              // a chunk with too many rows is k_pl_pages' refusal
                off[row] = value_base + (int64_t)val_base[tile] + vals + __popcll(m_val & below);
                null[row] = (uint8_t)(outer && d == 0);
            }
        }
        rows += __popcll(m_row);
        vals += __popcll(m_val);
    }
    if (PASS == 0) {
        bad = wave_reduce<Min>(bad);
        if (lane == 0) {
            n_row[tile] = (uint64_t)rows;
            n_val[tile] = (uint64_t)vals;
            if (bad != 255) atomicMin(err, (unsigned long long)p << 8 | (unsigned long long)bad);
        }
    }
}

struct PlCount {
    const uint64_t* c;
    __device__ uint64_t operator()(int64_t i) const { return c[i]; }
};

__global__ __launch_bounds__(WAVE) void k_pl_pages(const PlPage* __restrict__ pages, int64_t n_pages, int64_t n_tiles,
                                                   const PlInfo* __restrict__ infos, const uint64_t* __restrict__ row_base,
                                                   const uint64_t* __restrict__ val_base, int64_t* __restrict__ page_out,
                                                   int64_t* __restrict__ off, int64_t n_rows, int64_t value_base, unsigned long long* err) {
    const int64_t p = (int64_t)blockIdx.x * WAVE + threadIdx.x;
    if (p == 0) off[n_rows] = value_base + (int64_t)val_base[n_tiles];
    if (p >= n_pages) return;
    const PlPage pg = pages[p];
    const int64_t t0 = pg.tile0, t1 = p + 1 < n_pages ? pages[p + 1].tile0 : n_tiles;
    page_out[3 * p] = infos[p].def_end;
    page_out[3 * p + 1] = (int64_t)(val_base[t1] - val_base[t0]);
    page_out[3 * p + 2] = (int64_t)(row_base[t1] - row_base[t0]);
    if (pg.flags & OTTO_PL_F_CHUNK_FIRST) {
        const int64_t q = p + pg.chunk_pages;                // the host has checked q <= n_pages
        const int64_t tq = q < n_pages ? pages[q].tile0 : n_tiles;
        if ((int64_t)(row_base[tq] - row_base[t0]) != pg.chunk_rows) {
            // a page refused for its levels counts no rows: the row count is held against the row group's only in a call
            // without another violation (the walk and pass 0 are complete; only this kernel's own refusals can still arrive)
            const unsigned long long cur = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == ~0ull || (cur & 0xFF) == OTTO_PL_E_ROWS) atomicMin(err, (unsigned long long)p << 8 | (unsigned long long)OTTO_PL_E_ROWS);
        }
    }
}

static int pl_plan(const otto_pqlist_job* j, std::vector<PlPage>* out, int64_t* n_tiles) {
    OTTO_REQUIRE(j, "otto_pqlist: null job");
    OTTO_REQUIRE(j->n_pages >= 0 && j->n_pages < (1ll << 24), "otto_pqlist: n_pages must be in [0, 2^24)");
    OTTO_REQUIRE(j->n_pages == 0 || j->h_pages, "otto_pqlist: null page table");
    OTTO_REQUIRE(j->n_bytes >= 0 && j->n_bytes < (1ll << 31), "otto_pqlist: n_bytes must be in [0, 2^31)");
    OTTO_REQUIRE(j->n_rows >= 0 && j->n_rows < (1ll << 40) && j->value_base >= 0, "otto_pqlist: n_rows must be in [0, 2^40), value_base >= 0");
    out->resize((size_t)j->n_pages);
    int64_t tiles = 0, rows = 0, left = 0;                  // left: pages the open chunk still has to come
    for (int64_t p = 0; p < j->n_pages; ++p) {
        const int64_t* r = j->h_pages + p * OTTO_PL_FIELDS;
        const int64_t body = r[OTTO_PL_BODY_OFF], len = r[OTTO_PL_BODY_LEN], type = r[OTTO_PL_PAGE_TYPE], nv = r[OTTO_PL_NUM_VALUES];
        const int64_t flags = r[OTTO_PL_FLAGS], rl = r[OTTO_PL_REP_LEN], dl = r[OTTO_PL_DEF_LEN];
        OTTO_REQUIRE(type == 0 || type == 3, "otto_pqlist: page %lld: page type %lld", (long long)p, (long long)type);
        OTTO_REQUIRE(body >= 0 && len >= 0 && body + len <= j->n_bytes, "otto_pqlist: page %lld: body outside the %lld bytes", (long long)p,
                     (long long)j->n_bytes);
        OTTO_REQUIRE(nv >= 0 && nv < (1ll << 31), "otto_pqlist: page %lld: num_values %lld", (long long)p, (long long)nv);
        OTTO_REQUIRE((flags & ~7ll) == 0, "otto_pqlist: page %lld: flags %lld", (long long)p, (long long)flags);
        if (type == 3) {
            OTTO_REQUIRE(rl >= 0 && dl >= 0 && rl + dl <= len, "otto_pqlist: page %lld: %s", (long long)p, pl_reason(OTTO_PL_E_PREFIX));
        } else {
            OTTO_REQUIRE(rl == 0 && dl == 0, "otto_pqlist: page %lld: level lengths of a V1 page", (long long)p);
        }
        OTTO_REQUIRE(((flags & OTTO_PL_F_CHUNK_FIRST) != 0) == (left == 0), "otto_pqlist: page %lld: chunk boundaries disagree with CHUNK_PAGES",
                     (long long)p);
        PlPage& g = (*out)[(size_t)p];
        g = PlPage{body, len, rl, dl, nv, tiles, 0, 0, (int32_t)type, (int32_t)flags};
        if (flags & OTTO_PL_F_CHUNK_FIRST) {
            g.chunk_rows = r[OTTO_PL_CHUNK_ROWS];
            g.chunk_pages = r[OTTO_PL_CHUNK_PAGES];
            OTTO_REQUIRE(g.chunk_rows >= 0 && g.chunk_pages >= 1 && p + g.chunk_pages <= j->n_pages, "otto_pqlist: page %lld: chunk of %lld pages, %lld rows",
                         (long long)p, (long long)g.chunk_pages, (long long)g.chunk_rows);
            rows += g.chunk_rows;
            left = g.chunk_pages;
        }
        left -= 1;
        tiles += (nv + PL_TILE - 1) / PL_TILE;
    }
    OTTO_REQUIRE(rows == j->n_rows, "otto_pqlist: n_rows %lld, the chunks declare %lld", (long long)j->n_rows, (long long)rows);
    *n_tiles = tiles;
    return 0;
}

}  // namespace otto

using namespace otto;

extern "C" const char* otto_pqlist_reason(int32_t code) { return pl_reason(code); }

extern "C" int64_t otto_pqlist_workspace(const otto_pqlist_job* job) {
    std::vector<PlPage> pages;
    int64_t tiles = 0;
    if (pl_plan(job, &pages, &tiles) != 0) return -22;
    return (int64_t)pl_layout(job->n_pages, tiles, nullptr, nullptr);
}

extern "C" int otto_pqlist_levels(const otto_pqlist_job* job, int64_t* h_err) {
    OTTO_REQUIRE(h_err, "otto_pqlist_levels: null h_err");
    h_err[0] = -1;
    h_err[1] = 0;
    std::vector<PlPage> pages;
    int64_t tiles = 0;
    OTTO_TRY(pl_plan(job, &pages, &tiles));
    const otto_pqlist_job& j = *job;
    OTTO_REQUIRE(j.d_off && (j.n_rows == 0 || j.d_null), "otto_pqlist_levels: null output");
    OTTO_REQUIRE(j.n_pages == 0 || (j.d_bytes && j.h_page_out), "otto_pqlist_levels: null argument");
    PlWs w;
    const int64_t need = (int64_t)pl_layout(j.n_pages, tiles, (char*)j.d_work, &w);
    OTTO_REQUIRE(j.d_work && ((uintptr_t)j.d_work & 255) == 0 && j.work_bytes >= need, "otto_pqlist_levels: workspace of %lld 256-byte aligned bytes needed",
                 (long long)need);
    hipStream_t s = (hipStream_t)j.stream;
    OTTO_HIP(hipMemsetAsync(w.err, 0xFF, 8, s));
    if (j.n_pages > 0) {
        OTTO_HIP(hipMemcpyAsync(w.pages, pages.data(), (size_t)j.n_pages * sizeof(PlPage), hipMemcpyHostToDevice, s));
        k_pl_walk<<<(unsigned)((j.n_pages + WAVE - 1) / WAVE), WAVE, 0, s>>>(j.d_bytes, w.pages, j.n_pages, w.infos, w.marks, w.err);
        OTTO_HIP(hipGetLastError());
    }
    const unsigned grid = (unsigned)((tiles + PL_WAVES - 1) / PL_WAVES);
    if (grid > 0) {
        k_pl_tiles<0><<<grid, PL_THREADS, 0, s>>>(j.d_bytes, w.pages, j.n_pages, tiles, w.infos, w.marks, w.n_row, w.n_val, w.row_base, w.val_base,
                                                  j.d_off, j.d_null, j.n_rows, j.value_base, w.err);
        OTTO_HIP(hipGetLastError());
    }
    OTTO_TRY(device_scan(PlCount{w.n_row}, tiles, w.row_base, w.partial, s));
    OTTO_TRY(device_scan(PlCount{w.n_val}, tiles, w.val_base, w.partial, s));
    k_pl_pages<<<(unsigned)(j.n_pages / WAVE + 1), WAVE, 0, s>>>(w.pages, j.n_pages, tiles, w.infos, w.row_base, w.val_base, w.page_out, j.d_off,
                                                              j.n_rows, j.value_base, w.err);
    OTTO_HIP(hipGetLastError());
    if (grid > 0) {
        k_pl_tiles<1><<<grid, PL_THREADS, 0, s>>>(j.d_bytes, w.pages, j.n_pages, tiles, w.infos, w.marks, w.n_row, w.n_val, w.row_base, w.val_base,
                                                  j.d_off, j.d_null, j.n_rows, j.value_base, w.err);
        OTTO_HIP(hipGetLastError());
    }
    unsigned long long herr = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, w.err, 8, hipMemcpyDeviceToHost, s));
    if (j.n_pages > 0) OTTO_HIP(hipMemcpyAsync(j.h_page_out, w.page_out, (size_t)j.n_pages * 24, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (herr != ~0ull) {
        h_err[0] = (int64_t)(herr >> 8);
        h_err[1] = (int64_t)(herr & 0xFF);
        OTTO_REQUIRE(false, "otto_pqlist_levels: page %lld: %s", (long long)h_err[0], pl_reason(h_err[1]));
    }
    return 0;
}
