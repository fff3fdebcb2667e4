// Device-side Parquet encode for MI355X (gfx950): device columns -> the bodies of PLAIN and DELTA_BINARY_PACKED data pages.
// C-ABI and SPEC-PQWRITE in include/otto_pqwrite.h. Reference code this replaces: the pyarrow encode
// behind DataFrame.to_parquet of src/covisitation/covisitation.py and src/utilities/split_dataset_writer_parquet.py. Host
// restatement: tests/parquet_write_restatement.py; the element encoders are those of parquet_encode.h.
//
// The work is cut into units, numbered page after page: a delta page of n values has max(1, ceil((n - 1) / 128)) units, one
// per block of 128 deltas (the first also writes the page's header; a page of 0 or 1 values has that unit alone), a PLAIN
// page one per OTTO_PQW_PLAIN_TILE values. One wave owns a unit in both kernels, so nothing but wave_lds_sync orders the LDS
// traffic; a workgroup is four such waves that share nothing. A wave of k_pqw_plan takes a run of consecutive units (PqwWalk):
// the page of the first is found by a binary search, the later ones by stepping; a wave of k_pqw_emit takes every n-th unit.
//   k_pqw_plan   a block's values into LDS in whole lines (lane l takes value l, l + 64), two deltas per lane, so a miniblock
//                is 16 lanes: the minimum over the wave, an OR over each 16 lanes -> widths -> bytes, into the block record
//   k_pqw_scan   one wave per page: the header's length, the exclusive scan of the block sizes, the page's bytes
//   k_pqw_emit   the block's image in LDS (every field ORed into zeroed words), stored in 8-byte pieces; a PLAIN tile is
//                copied value by value at the stored width
#include <algorithm>
#include <vector>

#include "common.h"
#include "parquet_encode.h"
#include "wave.h"
#include "../../include/otto_pqwrite.h"

namespace otto {

constexpr int PQW_THREADS = 256, PQW_WAVES = PQW_THREADS / WAVE;
constexpr int PQW_CUS = 256;                                 // a grid is at most the workgroups that are resident together: a wave's share is one run or one stride
constexpr int PQW_PLAN_PER_CU = 8, PQW_EMIT_PER_CU = 6;      // workgroups per CU at the kernels' 8 and 6 waves per SIMD (profiles/pqwrite/kernel_resources.txt)
constexpr unsigned long long PQW_NO_ERR = ~0ull;
constexpr uint64_t PQW_MAGIC = 0x31544952575150ull;         // "PQWRIT1"
constexpr int PQW_STAGE_WORDS = 272;                         // 17 bytes of page header + 1,038 of a block, and the spare words
static_assert(OTTO_PQW_BLOCK == 2 * WAVE, "a lane owns two deltas");
static_assert(PQW_STAGE_WORDS * 4 >= 17 + OTTO_PQW_BLOCK_BYTES_MAX + 8 + 8, "the image of a block, read in 8-byte pieces");

struct PqwCol {
    const void* p;
    int32_t elem_bytes, kind, encoding, phys_bytes;
};
struct PqwPageRec {
    int64_t first_row;
    int32_t n, col;
};
struct PqwHead {                   // the first 64 bytes of the workspace
    unsigned long long err_domain, err_plan;
    uint64_t magic, hash, n_units, n_pages, pad[2];
};

struct PqwWs {
    PqwHead* head;
    PqwCol* cols;
    PqwPageRec* pages;
    int64_t* unit0;                // [n_pages + 1] first unit of a page, the number of units last
    int64_t* page_bytes;           // [n_pages]
    int64_t* page_dst;             // [n_pages]
    int64_t* rec_m;                // [n_units] block records: minimum delta,
    uint32_t* rec_w;               //           the four widths,
    uint32_t* rec_bytes;           //           bytes of the block,
    uint32_t* rec_off;             //           its first byte in the page's body
};

static size_t pqw_layout(int64_t n_cols, int64_t n_pages, int64_t n_units, char* base, PqwWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    PqwWs t;
    t.head = (PqwHead*)take(sizeof(PqwHead));
    t.cols = (PqwCol*)take((size_t)n_cols * sizeof(PqwCol));
    t.pages = (PqwPageRec*)take((size_t)n_pages * sizeof(PqwPageRec));
    t.unit0 = (int64_t*)take((size_t)(n_pages + 1) * 8);
    t.page_bytes = (int64_t*)take((size_t)n_pages * 8);
    t.page_dst = (int64_t*)take((size_t)n_pages * 8);
    t.rec_m = (int64_t*)take((size_t)n_units * 8);
    t.rec_w = (uint32_t*)take((size_t)n_units * 4);
    t.rec_bytes = (uint32_t*)take((size_t)n_units * 4);
    t.rec_off = (uint32_t*)take((size_t)n_units * 4);
    if (w) *w = t;
    return o;
}

// the stored value of row `row`: integers extended to 64 bits through their stored 32 or 64, a float as its bit pattern
__device__ __forceinline__ int64_t pqw_load(const PqwCol& c, int64_t row) {
    switch (c.elem_bytes) {
        case 1: return c.kind == OTTO_PQW_SIGNED ? (int64_t)((const int8_t*)c.p)[row] : (int64_t)((const uint8_t*)c.p)[row];
        case 2: return c.kind == OTTO_PQW_SIGNED ? (int64_t)((const int16_t*)c.p)[row] : (int64_t)((const uint16_t*)c.p)[row];
        case 4: return (int64_t)((const int32_t*)c.p)[row];
        default: return ((const int64_t*)c.p)[row];
    }
}

// the page of unit u: the last p with unit0[p] <= u (pages without units are stepped over)
__device__ __forceinline__ int64_t pqw_page_of(const int64_t* __restrict__ unit0, int64_t n_pages, int64_t u) {
    int64_t lo = 0, hi = n_pages;                            // unit0[lo] <= u < unit0[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (unit0[mid] <= u) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The units of one wave. RUN: a run of consecutive units, so that the page is searched for once and then stepped to and the
// rows a wave reads follow one another (k_pqw_plan, where PLAIN units cost nothing). Else every n_waves-th unit, which spreads
// the PLAIN tiles, 16 blocks' worth of bytes each, evenly over the waves (k_pqw_emit). Every member is uniform over the wave.
template <bool RUN>
struct PqwWalk {
    const PqwCol* cols;
    const PqwPageRec* pages;
    const int64_t* unit0;
    int64_t u, u_hi, p, p_u0, p_end, stride, n_pages;
    PqwPageRec pg;
    PqwCol c;

    __device__ __forceinline__ PqwWalk(const PqwCol* cols_, const PqwPageRec* pages_, const int64_t* unit0_, int64_t n_pages_, int64_t n_units)
        : cols(cols_), pages(pages_), unit0(unit0_), n_pages(n_pages_) {
        const int64_t n_waves = (int64_t)gridDim.x * PQW_WAVES, me = (int64_t)blockIdx.x * PQW_WAVES + (threadIdx.x >> 6);
        const int64_t chunk = (n_units + n_waves - 1) / n_waves;
        u = RUN ? me * chunk : me;
        u_hi = RUN && u + chunk < n_units ? u + chunk : n_units;
        stride = RUN ? 1 : n_waves;
        p = -1;
        p_end = 0;
        if (u < u_hi) {
            p = pqw_page_of(unit0, n_pages, u);
            load_page();
        }
    }
    __device__ __forceinline__ void load_page() {
        p_u0 = unit0[p];
        p_end = unit0[p + 1];
        pg = pages[p];
        c = cols[pg.col];
    }
    // false when the run is over; else u is the unit, p / pg / c its page
    __device__ __forceinline__ bool valid() const { return u < u_hi; }
    __device__ __forceinline__ void step() {
        u += stride;
        if (u < u_hi && u >= p_end) {                        // u < n_units = unit0[n_pages], so either search ends at a page
            if (RUN) {
                do ++p; while (u >= unit0[p + 1]);
            } else {
                p = pqw_page_of(unit0, n_pages, u);
            }
            load_page();
        }
    }
};

__device__ __forceinline__ unsigned long long pqw_err_key(int64_t row, int32_t col) { return (unsigned long long)row << 16 | (unsigned)col; }

struct PqwLdsSink {
    uint32_t* w;
    __device__ __forceinline__ void or32(uint32_t i, uint32_t v) { atomicOr(&w[i], v); }
};

// What a lane knows of its block after the values are in x[0 .. nd]: its two relative deltas and the block's figures
struct PqwBlock {
    int64_t m;
    uint32_t widths;
    uint64_t rel0, rel1;
};

// deltas 2 * lane and 2 * lane + 1 of the nd (1 .. 128) deltas of x[0 .. nd]; m and the widths by reduction
__device__ __forceinline__ PqwBlock pqw_block_figures(const int64_t* x, int nd) {
    const int lane = (int)lane_id();
    const int e0 = 2 * lane, e1 = e0 + 1;
    const bool v0 = e0 < nd, v1 = e1 < nd;
    const int64_t a = x[v0 ? e0 : 0], b = x[v0 ? e0 + 1 : 0], c = x[v1 ? e1 + 1 : 0];
    const int64_t d0 = (int64_t)((uint64_t)b - (uint64_t)a), d1 = (int64_t)((uint64_t)c - (uint64_t)b);
    long long mn = v0 ? (long long)d0 : INT64_MAX;
    if (v1 && d1 < mn) mn = d1;
    mn = wave_reduce<Min>(mn);
    PqwBlock r;
    r.m = (int64_t)mn;
    r.rel0 = v0 ? (uint64_t)d0 - (uint64_t)mn : 0ull;
    r.rel1 = v1 ? (uint64_t)d1 - (uint64_t)mn : 0ull;
    unsigned long long any = r.rel0 | r.rel1;
    for (int o = 8; o > 0; o >>= 1) any |= __shfl_xor(any, o, 64);          // stays inside the 16 lanes of a miniblock
    const uint32_t w = pqe_bit_length(any);
    r.widths = 0;
    for (int j = 0; j < OTTO_PQW_MINIBLOCKS; ++j) r.widths |= (uint32_t)__shfl((int)w, 16 * j, 64) << (8 * j);
    return r;
}

// the nd + 1 values of a block into x, lane l the values l, l + 64, l + 128; a delta-domain violation goes to *err
__device__ __forceinline__ void pqw_stage_values(const PqwCol& c, int32_t col, int64_t row0, int nd, int64_t* x, unsigned long long* err) {
    for (int i = (int)lane_id(); i <= nd; i += WAVE) {
        const int64_t v = pqw_load(c, row0 + i);
        x[i] = v;
        if (err && !pqe_in_domain(v, (uint32_t)c.phys_bytes)) atomicMin(err, pqw_err_key(row0 + i, col));
    }
    wave_lds_sync();
}

__global__ __launch_bounds__(PQW_THREADS) void k_pqw_plan(const PqwCol* __restrict__ cols, const PqwPageRec* __restrict__ pages,
                                                          const int64_t* __restrict__ unit0, int64_t n_pages, int64_t n_units,
                                                          int64_t* __restrict__ rec_m, uint32_t* __restrict__ rec_w,
                                                          uint32_t* __restrict__ rec_bytes, unsigned long long* err) {
    __shared__ int64_t X[PQW_WAVES][OTTO_PQW_BLOCK + 2];
    const int wave = (int)(threadIdx.x >> 6);
    int64_t* x = X[wave];
    for (PqwWalk<true> k(cols, pages, unit0, n_pages, n_units); k.valid(); k.step()) {
        const int64_t u = k.u;
        const PqwPageRec& pg = k.pg;
        const PqwCol& c = k.c;
        if (c.encoding != OTTO_PQW_DELTA) continue;
        const int64_t b = u - k.p_u0;
        const int64_t left = (int64_t)pg.n - 1 - b * OTTO_PQW_BLOCK;
        const int nd = left < 0 ? 0 : left > OTTO_PQW_BLOCK ? OTTO_PQW_BLOCK : (int)left;
        if (nd == 0) {                                       // a page of 0 or 1 values: k_pqw_scan looks at the first value
            if (lane_id() == 0) rec_m[u] = 0, rec_w[u] = 0, rec_bytes[u] = 0;
            continue;
        }
        pqw_stage_values(c, pg.col, pg.first_row + b * OTTO_PQW_BLOCK, nd, x, err);
        const PqwBlock f = pqw_block_figures(x, nd);
        if (lane_id() == 0) rec_m[u] = f.m, rec_w[u] = f.widths, rec_bytes[u] = pqe_block_bytes(f.m, f.widths);
        wave_lds_sync();                                     // x is rewritten by the next unit
    }
}

__global__ __launch_bounds__(PQW_THREADS) void k_pqw_scan(const PqwCol* __restrict__ cols, const PqwPageRec* __restrict__ pages,
                                                          const int64_t* __restrict__ unit0, int64_t n_pages,
                                                          const uint32_t* __restrict__ rec_bytes, uint32_t* __restrict__ rec_off,
                                                          int64_t* __restrict__ page_bytes, unsigned long long* err) {
    const int lane = (int)lane_id();
    for (int64_t p = (int64_t)blockIdx.x * PQW_WAVES + (threadIdx.x >> 6); p < n_pages; p += (int64_t)gridDim.x * PQW_WAVES) {
        const PqwPageRec pg = pages[p];
        const PqwCol c = cols[pg.col];
        if (c.encoding != OTTO_PQW_DELTA) {
            if (lane == 0) page_bytes[p] = (int64_t)pg.n * c.phys_bytes;
            continue;
        }
        const int64_t first = pg.n ? pqw_load(c, pg.first_row) : 0;
        if (lane == 0 && pg.n && !pqe_in_domain(first, (uint32_t)c.phys_bytes)) atomicMin(err, pqw_err_key(pg.first_row, pg.col));
        uint32_t run = pqe_page_header_len((uint32_t)pg.n, first);
        const int64_t u0 = unit0[p], u1 = unit0[p + 1];
        for (int64_t base = u0; base < u1; base += WAVE) {
            const int64_t u = base + lane;
            const uint32_t bytes = u < u1 ? rec_bytes[u] : 0u;
            const uint32_t incl = wave_incl_scan<uint32_t>(bytes);
            if (u < u1) rec_off[u] = run + incl - bytes;
            run += (uint32_t)__shfl((int)incl, 63, 64);
        }
        if (lane == 0) page_bytes[p] = run;
    }
}

__global__ __launch_bounds__(PQW_THREADS) void k_pqw_emit(const PqwCol* __restrict__ cols, const PqwPageRec* __restrict__ pages,
                                                          const int64_t* __restrict__ unit0, int64_t n_pages, int64_t n_units,
                                                          const int64_t* __restrict__ rec_m, const uint32_t* __restrict__ rec_w,
                                                          const uint32_t* __restrict__ rec_bytes, const uint32_t* __restrict__ rec_off,
                                                          const int64_t* __restrict__ page_bytes, const int64_t* __restrict__ page_dst,
                                                          uint8_t* __restrict__ out, unsigned long long* err) {
    __shared__ int64_t X[PQW_WAVES][OTTO_PQW_BLOCK + 2];
    __shared__ uint64_t S[PQW_WAVES][PQW_STAGE_WORDS / 2];
    const int lane = (int)lane_id();
    const int wave = (int)(threadIdx.x >> 6);
    int64_t* x = X[wave];
    uint32_t* stage = reinterpret_cast<uint32_t*>(S[wave]);
    for (PqwWalk<false> k(cols, pages, unit0, n_pages, n_units); k.valid(); k.step()) {
        const int64_t u = k.u;
        const PqwPageRec& pg = k.pg;
        const PqwCol& c = k.c;
        const int64_t b = u - k.p_u0;
        const int64_t pbytes = page_bytes[k.p];
        uint8_t* dst = out + page_dst[k.p];
        if (c.encoding != OTTO_PQW_DELTA) {                  // a tile of a PLAIN page: [at, at + cnt) of its values
            const int64_t at = b * OTTO_PQW_PLAIN_TILE;
            const int64_t rest = (int64_t)pg.n - at;
            const int cnt = rest > OTTO_PQW_PLAIN_TILE ? OTTO_PQW_PLAIN_TILE : (int)rest;
            if (cnt <= 0 || (at + cnt) * c.phys_bytes > pbytes) {            // uniform over the wave
                if (lane == 0) atomicMin(err, (unsigned long long)u);
                continue;
            }
            if (c.phys_bytes == 4) {
                for (int i = lane; i < cnt; i += WAVE) {
                    const int32_t v = (int32_t)pqw_load(c, pg.first_row + at + i);
                    __builtin_memcpy(dst + (at + i) * 4, &v, 4);
                }
            } else {
                for (int i = lane; i < cnt; i += WAVE) {
                    const int64_t v = pqw_load(c, pg.first_row + at + i);
                    __builtin_memcpy(dst + (at + i) * 8, &v, 8);
                }
            }
            continue;
        }
        // a block of a delta page. Every store lands in [off - lead, off - lead + total) of the page's body; the refusal
        // (uniform over the wave) keeps that inside the body whatever the workspace holds
        const int64_t left = (int64_t)pg.n - 1 - b * OTTO_PQW_BLOCK;
        const int nd = left < 0 ? 0 : left > OTTO_PQW_BLOCK ? OTTO_PQW_BLOCK : (int)left;
        const int64_t m = rec_m[u];
        const uint32_t widths = rec_w[u], bytes = rec_bytes[u], off = rec_off[u];
        if (nd || (b == 0 && pg.n)) pqw_stage_values(c, pg.col, pg.first_row + b * OTTO_PQW_BLOCK, nd, x, nullptr);
        const int64_t first = pg.n ? x[0] : 0;
        const uint32_t lead = b == 0 ? pqe_page_header_len((uint32_t)pg.n, first) : 0u;
        const uint32_t total = lead + bytes;
        bool ok = pqe_widths_ok(widths) && bytes == (nd ? pqe_block_bytes(m, widths) : 0u) && off >= lead &&
                  (int64_t)off + bytes <= pbytes && (b != 0 || off == lead);
        for (int j = 0; j < OTTO_PQW_MINIBLOCKS; ++j)        // no width where no delta is
            if (j * OTTO_PQW_MINI_VALUES >= nd && ((widths >> (8 * j)) & 0xFFu)) ok = false;
        if (!ok) {
            if (lane == 0) atomicMin(err, (unsigned long long)u);
            wave_lds_sync();
            continue;
        }
        const uint32_t words = (total + 3u) / 4u + 2u;       // the image, and the two words a field may reach into
        for (uint32_t i = lane; i < words + 1u && i < PQW_STAGE_WORDS; i += WAVE) stage[i] = 0;
        wave_lds_sync();
        PqwLdsSink sink = {stage};
        if (lane == 0) {
            uint32_t pos = 0;
            if (b == 0) pos = pqe_put_page_header(sink, pos, (uint32_t)pg.n, first);
            if (nd) pqe_put_block_header(sink, pos, m, widths);
        }
        if (nd) {
            const int e0 = 2 * lane, e1 = e0 + 1;
            const uint32_t body = lead + pqe_block_header_len(m);
            if (e0 < nd) pqe_pack_delta(sink, body, (uint32_t)e0, (uint64_t)x[e0 + 1] - (uint64_t)x[e0] - (uint64_t)m, widths);
            if (e1 < nd) pqe_pack_delta(sink, body, (uint32_t)e1, (uint64_t)x[e1 + 1] - (uint64_t)x[e1] - (uint64_t)m, widths);
        }
        wave_lds_sync();
        uint8_t* q = dst + off - lead;
        for (uint32_t i = (uint32_t)lane * 8u; i < total; i += WAVE * 8u) {
            const uint64_t v = S[wave][i >> 3];
            if (i + 8u <= total) {
                __builtin_memcpy(q + i, &v, 8);
            } else {
                for (uint32_t k = 0; i + k < total; ++k) q[i + k] = (uint8_t)(v >> (8u * k));
            }
        }
        wave_lds_sync();                                     // x and the stage are rewritten by the next unit
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
struct PqwPlan {
    std::vector<PqwCol> cols;
    std::vector<PqwPageRec> pages;
    std::vector<int64_t> unit0;
    int64_t n_units = 0;
    uint64_t hash = 0;
};

static uint64_t pqw_fnv(uint64_t h, const void* p, size_t n) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    return h;
}

// every rule of the header that the host can check; the unit numbering; the hash that ties a workspace to a job
static int pqw_check(const char* what, const otto_pqw_job* job, PqwPlan* plan) {
    OTTO_REQUIRE(job, "%s: null job", what);
    OTTO_REQUIRE(job->n_columns >= 1 && job->n_columns <= OTTO_PQW_MAX_COLUMNS && job->columns, "%s: n_columns must be in [1, %d] (got %lld)", what,
                 OTTO_PQW_MAX_COLUMNS, (long long)job->n_columns);
    OTTO_REQUIRE(job->n_pages >= 0 && (job->n_pages == 0 || job->pages), "%s: negative n_pages or null page table", what);
    plan->cols.resize((size_t)job->n_columns);
    for (int64_t j = 0; j < job->n_columns; ++j) {
        const otto_pqw_column& c = job->columns[j];
        OTTO_REQUIRE(c.elem_bytes == 1 || c.elem_bytes == 2 || c.elem_bytes == 4 || c.elem_bytes == 8, "%s: column %lld: elem_bytes %d", what,
                     (long long)j, c.elem_bytes);
        OTTO_REQUIRE(c.kind == OTTO_PQW_SIGNED || c.kind == OTTO_PQW_UNSIGNED || (c.kind == OTTO_PQW_FLOAT && c.elem_bytes >= 4),
                     "%s: column %lld: kind %d with %d-byte elements", what, (long long)j, c.kind, c.elem_bytes);
        OTTO_REQUIRE(c.encoding == OTTO_PQW_PLAIN || (c.encoding == OTTO_PQW_DELTA && c.kind != OTTO_PQW_FLOAT),
                     "%s: column %lld: encoding %d (PLAIN 0 for any column, DELTA_BINARY_PACKED 5 for integers)", what, (long long)j, c.encoding);
        OTTO_REQUIRE(c.n_rows >= 0 && (c.n_rows == 0 || c.d_data), "%s: column %lld: negative n_rows or null d_data", what, (long long)j);
        plan->cols[(size_t)j] = PqwCol{c.d_data, c.elem_bytes, c.kind, c.encoding, c.elem_bytes == 8 ? 8 : 4};
    }
    plan->pages.resize((size_t)job->n_pages);
    plan->unit0.resize((size_t)job->n_pages + 1);
    int64_t units = 0;
    for (int64_t p = 0; p < job->n_pages; ++p) {
        const otto_pqw_page& g = job->pages[p];
        OTTO_REQUIRE(g.column >= 0 && g.column < job->n_columns, "%s: page %lld: column slot %d", what, (long long)p, g.column);
        OTTO_REQUIRE(g.n_values >= 0 && g.n_values <= OTTO_PQW_MAX_PAGE_VALUES, "%s: page %lld: n_values %d is not in [0, %d]", what, (long long)p,
                     g.n_values, OTTO_PQW_MAX_PAGE_VALUES);
        OTTO_REQUIRE(g.first_row >= 0 && g.first_row + g.n_values <= job->columns[g.column].n_rows, "%s: page %lld: rows [%lld, %lld) leave the column's %lld",
                     what, (long long)p, (long long)g.first_row, (long long)(g.first_row + g.n_values), (long long)job->columns[g.column].n_rows);
        plan->pages[(size_t)p] = PqwPageRec{g.first_row, g.n_values, g.column};
        plan->unit0[(size_t)p] = units;
        if (job->columns[g.column].encoding == OTTO_PQW_DELTA)
            units += g.n_values <= 1 ? 1 : ((int64_t)g.n_values - 1 + OTTO_PQW_BLOCK - 1) / OTTO_PQW_BLOCK;
        else
            units += ((int64_t)g.n_values + OTTO_PQW_PLAIN_TILE - 1) / OTTO_PQW_PLAIN_TILE;
    }
    plan->unit0[(size_t)job->n_pages] = units;
    plan->n_units = units;
    uint64_t h = 0xCBF29CE484222325ull;
    h = pqw_fnv(h, plan->cols.data(), plan->cols.size() * sizeof(PqwCol));
    h = pqw_fnv(h, plan->pages.data(), plan->pages.size() * sizeof(PqwPageRec));
    plan->hash = h;
    return 0;
}

static int pqw_check_work(const char* what, const otto_pqw_job* job, const PqwPlan& plan, PqwWs* w) {
    const int64_t need = (int64_t)pqw_layout(job->n_columns, job->n_pages, plan.n_units, nullptr, nullptr);
    OTTO_REQUIRE(job->d_work, "%s: null d_work", what);
    OTTO_REQUIRE(job->work_bytes >= need, "%s: workspace too small (%lld < %lld)", what, (long long)job->work_bytes, (long long)need);
    pqw_layout(job->n_columns, job->n_pages, plan.n_units, (char*)job->d_work, w);
    return 0;
}

static unsigned pqw_grid(int64_t waves, int per_cu) {
    const int64_t g = (waves + PQW_WAVES - 1) / PQW_WAVES, most = (int64_t)PQW_CUS * per_cu;
    return (unsigned)(g < 1 ? 1 : g > most ? most : g);
}

}  // namespace otto

using namespace otto;

extern "C" int64_t otto_pqw_workspace(const otto_pqw_job* job) {
    PqwPlan plan;
    OTTO_TRY(pqw_check("otto_pqw_workspace", job, &plan));
    return (int64_t)pqw_layout(job->n_columns, job->n_pages, plan.n_units, nullptr, nullptr);
}

extern "C" int otto_pqw_plan(const otto_pqw_job* job, int64_t* h_page_bytes) {
    PqwPlan plan;
    PqwWs w;
    OTTO_TRY(pqw_check("otto_pqw_plan", job, &plan));
    OTTO_REQUIRE(h_page_bytes || job->n_pages == 0, "otto_pqw_plan: null h_page_bytes");
    OTTO_TRY(pqw_check_work("otto_pqw_plan", job, plan, &w));
    hipStream_t s = (hipStream_t)job->stream;
    const int64_t np = job->n_pages;
    PqwHead head = {PQW_NO_ERR, PQW_NO_ERR, PQW_MAGIC, plan.hash, (uint64_t)plan.n_units, (uint64_t)np, {0, 0}};
    OTTO_HIP(hipMemcpyAsync(w.head, &head, sizeof(head), hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.cols, plan.cols.data(), plan.cols.size() * sizeof(PqwCol), hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.unit0, plan.unit0.data(), plan.unit0.size() * 8, hipMemcpyHostToDevice, s));
    unsigned long long herr = PQW_NO_ERR;
    if (np) {
        OTTO_HIP(hipMemcpyAsync(w.pages, plan.pages.data(), plan.pages.size() * sizeof(PqwPageRec), hipMemcpyHostToDevice, s));
        if (plan.n_units) {
            k_pqw_plan<<<pqw_grid(plan.n_units, PQW_PLAN_PER_CU), PQW_THREADS, 0, s>>>(w.cols, w.pages, w.unit0, np, plan.n_units, w.rec_m, w.rec_w, w.rec_bytes,
                                                                      &w.head->err_domain);
            OTTO_HIP(hipGetLastError());
        }
        k_pqw_scan<<<pqw_grid(np, PQW_PLAN_PER_CU), PQW_THREADS, 0, s>>>(w.cols, w.pages, w.unit0, np, w.rec_bytes, w.rec_off, w.page_bytes, &w.head->err_domain);
        OTTO_HIP(hipGetLastError());
        OTTO_HIP(hipMemcpyAsync(h_page_bytes, w.page_bytes, (size_t)np * 8, hipMemcpyDeviceToHost, s));
        OTTO_HIP(hipMemcpyAsync(&herr, &w.head->err_domain, 8, hipMemcpyDeviceToHost, s));
    }
    OTTO_HIP(hipStreamSynchronize(s));
    if (herr != PQW_NO_ERR) {
        OTTO_HIP(hipMemsetAsync(w.head, 0xFF, sizeof(PqwHead), s));         // the workspace holds no plan
        OTTO_HIP(hipStreamSynchronize(s));
        const int col = (int)(herr & 0xFFFFu);
        set_error("otto_pqw_plan: column %d, row %lld: a value outside the domain of DELTA_BINARY_PACKED, [0, 2^%d)", col, (long long)(herr >> 16),
                  plan.cols[(size_t)col].phys_bytes == 4 ? 31 : 62);
        return -22;
    }
    return 0;
}

extern "C" int otto_pqw_emit(const otto_pqw_job* job, const int64_t* h_page_dst, uint8_t* d_out, int64_t out_bytes) {
    PqwPlan plan;
    PqwWs w;
    OTTO_TRY(pqw_check("otto_pqw_emit", job, &plan));
    OTTO_REQUIRE(h_page_dst || job->n_pages == 0, "otto_pqw_emit: null h_page_dst");
    OTTO_REQUIRE(out_bytes >= 0 && (d_out || out_bytes == 0), "otto_pqw_emit: null d_out or negative out_bytes");
    OTTO_TRY(pqw_check_work("otto_pqw_emit", job, plan, &w));
    hipStream_t s = (hipStream_t)job->stream;
    const int64_t np = job->n_pages;
    PqwHead head;
    std::vector<int64_t> bytes((size_t)np);
    OTTO_HIP(hipMemcpyAsync(&head, w.head, sizeof(head), hipMemcpyDeviceToHost, s));
    if (np) OTTO_HIP(hipMemcpyAsync(bytes.data(), w.page_bytes, (size_t)np * 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    OTTO_REQUIRE(head.magic == PQW_MAGIC && head.hash == plan.hash && head.n_units == (uint64_t)plan.n_units && head.n_pages == (uint64_t)np &&
                     head.err_domain == PQW_NO_ERR,
                 "otto_pqw_emit: the workspace does not hold the plan otto_pqw_plan wrote for this job");
    std::vector<int64_t> order;
    for (int64_t p = 0; p < np; ++p) {
        OTTO_REQUIRE(bytes[(size_t)p] >= 0 && bytes[(size_t)p] <= (int64_t)OTTO_PQW_MAX_PAGE_VALUES * 9 + 32,
                     "otto_pqw_emit: the workspace does not hold the plan otto_pqw_plan wrote for this job");
        OTTO_REQUIRE(h_page_dst[p] >= 0 && h_page_dst[p] <= out_bytes && bytes[(size_t)p] <= out_bytes - h_page_dst[p],
                     "otto_pqw_emit: page %lld: bytes [%lld, %lld) leave out_bytes %lld; nothing written", (long long)p, (long long)h_page_dst[p],
                     (long long)(h_page_dst[p] + bytes[(size_t)p]), (long long)out_bytes);
        if (bytes[(size_t)p]) order.push_back(p);
    }
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return h_page_dst[a] < h_page_dst[b]; });
    for (size_t i = 1; i < order.size(); ++i) {
        const int64_t a = order[i - 1], b = order[i];
        OTTO_REQUIRE(h_page_dst[a] + bytes[(size_t)a] <= h_page_dst[b], "otto_pqw_emit: the extents of pages %lld and %lld overlap; nothing written",
                     (long long)a, (long long)b);
    }
    if (np == 0 || plan.n_units == 0) return 0;
    // the tables the kernel reads rows by come from the job again, so only checked figures are taken from the workspace
    OTTO_HIP(hipMemcpyAsync(w.cols, plan.cols.data(), plan.cols.size() * sizeof(PqwCol), hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.pages, plan.pages.data(), plan.pages.size() * sizeof(PqwPageRec), hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.unit0, plan.unit0.data(), plan.unit0.size() * 8, hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.page_bytes, bytes.data(), (size_t)np * 8, hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.page_dst, h_page_dst, (size_t)np * 8, hipMemcpyHostToDevice, s));
    k_pqw_emit<<<pqw_grid(plan.n_units, PQW_EMIT_PER_CU), PQW_THREADS, 0, s>>>(w.cols, w.pages, w.unit0, np, plan.n_units, w.rec_m, w.rec_w, w.rec_bytes, w.rec_off,
                                                              w.page_bytes, w.page_dst, d_out, &w.head->err_plan);
    OTTO_HIP(hipGetLastError());
    unsigned long long herr = PQW_NO_ERR;
    OTTO_HIP(hipMemcpyAsync(&herr, &w.head->err_plan, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (herr != PQW_NO_ERR) {
        OTTO_HIP(hipMemsetAsync(&w.head->err_plan, 0xFF, 8, s));
        OTTO_HIP(hipStreamSynchronize(s));
        set_error("otto_pqw_emit: unit %llu: the workspace does not hold the plan otto_pqw_plan wrote for these inputs", herr);
        return -22;
    }
    return 0;
}
