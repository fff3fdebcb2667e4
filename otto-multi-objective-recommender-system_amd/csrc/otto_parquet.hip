// Device-side Parquet decode for MI355X (gfx950): the page bodies of the split files, as they lie in the file -> the
// session / aid / ts / type columns. C-ABI and SPEC-PARQUET in include/otto_parquet.h; the scalar
// element decoders are the host/device functions of parquet_decode.h.
//
//   k_pq_snappy  one wave per compressed page. The wave keeps a window of the input in LDS; every lane parses the same
//                tag from it (the element is wave-uniform), then the 64 lanes carry the element out: a literal is a
//                coalesced copy input -> output, a copy reads the output this wave wrote earlier. That read is ordered
//                behind the stores by waiting for them (s_waitcnt vmcnt(0) inside a workgroup-scope fence: the wave's
//                loads and stores go through one L1), and only when the copy's source reaches into bytes stored since
//                the last wait -- no LDS window of the output, since offsets reach back 64 KiB and more.
//   k_pq_runs    one lane per data page: the V1 definition levels (ones == num_values), the bit-width byte and every
//                run header of the page, checked against the page's extent; one (header byte, first value) checkpoint
//                per OTTO_PQ_TILE values. A bit-packed run covers >= 8 values per header, so the walk touches a small
//                part of the page.
//   k_pq_decode  one wave per tile of OTTO_PQ_TILE values: walks the runs from the tile's checkpoint (wave-uniform), the
//                lanes extract the indices of a run side by side, gather from the chunk's dictionary page and store with
//                the cast. PLAIN pages are a straight casting copy in the same kernel. The dictionary is read through
//                the cache: a tile gathers 1024 entries, staging a dictionary of up to 1 MiB in LDS per tile would
//                read more than it saves.
//
// DELTA_BINARY_PACKED pages take no tile of k_pq_decode and are skipped by k_pq_runs; they run four kernels of their own, so
// that nothing but the block headers of a page is walked serially:
//   k_pq_delta_walk  one lane per delta page: the levels, the header, every block header and miniblock extent
//                    (pq_delta_walk); one (width bytes, min_delta) record per block.
//   k_pq_delta_sum   one wave per block: unpacks the fields 64 at a time and reduces min_delta + field over the block's
//                    values, modulo 2^64.
//   k_pq_delta_scan  one wave per delta page: exclusive scan of the block sums, 64 blocks at a time, plus the first value
//                    -> the value in front of every block; stores the page's first value.
//   k_pq_delta_out   one wave per block: unpacks again, a wave inclusive scan plus the block's base, stored with the cast.
// The host cannot see a page's block size (the body may be compressed): the block records of a page are sized for blocks of
// 128, the smallest accepted, and the last two kernels start one wave per such slot; waves past the page's real block
// count leave at once.
#include <vector>

#include "common.h"
#include "wave.h"
#include "parquet_decode.h"
#include "../../include/otto_parquet.h"

namespace otto {

constexpr int PQ_THREADS = 256;
constexpr int PQ_WAVES = PQ_THREADS / WAVE;
constexpr int PQ_WIN = 1024;                                // bytes of input a wave keeps in LDS
constexpr int PQ_TILE = OTTO_PQ_TILE;

struct PqStream {                                           // one Snappy stream; n < 0: nothing to do
    int64_t src, n, dst, dst_len;
};

struct PqPage {
    int64_t body, body_len;                                 // the decoded body: offset in the workspace bodies (in_work) or in d_bytes
    int64_t num_values, out_row, tile0, mark0;              // first tile / first checkpoint of the page
    int32_t in_work, type, plain, levels, col, dict;        // plain: 1 PLAIN, 0 dictionary indices, 2 DELTA_BINARY_PACKED
};

struct PqDelta {                                            // one delta page: its slots among the block records
    int64_t page, blk0;
};

struct PqBlock {
    int64_t widths, min_delta;                              // byte of the block's width bytes inside the body
    uint64_t base;                                          // k_pq_delta_sum: the block's sum; k_pq_delta_scan: the value in front of it
};

struct PqCol {
    void* out;
    int32_t elem, phys, zext, pad;
};

struct PqWs {
    unsigned long long* err;      // page << 8 | reason of the smallest violating page, ~0 without one
    PqPage* pages;                // [n_pages]
    PqStream* streams;            // [n_pages]
    PqCol* cols;                  // [64]
    int32_t* sstat;               // [n_pages]  status of the page's Snappy stream
    int64_t* vstart;              // [n_pages]  where the values start in the body, -1: the page is not decoded
    int64_t* marks;               // [2 * tiles]
    uint8_t* bodies;              // the decompressed bodies, each 16-byte aligned
    PqDelta* dpages;              // [n_delta]
    pq_delta_head* dheads;        // [n_delta]  written by k_pq_delta_walk
    PqBlock* blocks;              // [block slots]
};

constexpr int PQ_MAX_COLS = 64;

static inline size_t pq_align(size_t b) { return (b + 255) & ~(size_t)255; }

static size_t pq_layout(int64_t n_pages, int64_t tiles, int64_t body_bytes, int64_t n_delta, int64_t slots, char* base, PqWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += pq_align(bytes); return p; };
    PqWs t;
    t.err = (unsigned long long*)take(8);
    t.pages = (PqPage*)take((size_t)n_pages * sizeof(PqPage));
    t.streams = (PqStream*)take((size_t)n_pages * sizeof(PqStream));
    t.cols = (PqCol*)take(PQ_MAX_COLS * sizeof(PqCol));
    t.sstat = (int32_t*)take((size_t)n_pages * 4);
    t.vstart = (int64_t*)take((size_t)n_pages * 8);
    t.marks = (int64_t*)take((size_t)tiles * 16);
    t.bodies = (uint8_t*)take((size_t)body_bytes);
    t.dpages = (PqDelta*)take((size_t)n_delta * sizeof(PqDelta));       // nothing without delta pages
    t.dheads = (pq_delta_head*)take((size_t)n_delta * sizeof(pq_delta_head));
    t.blocks = (PqBlock*)take((size_t)slots * sizeof(PqBlock));
    if (w) *w = t;
    return o;
}

// Carries out one Snappy stream with the 64 lanes of the calling wave; src[0 .. n) -> dst[0 .. dst_len). win: PQ_WIN bytes
// of LDS of the wave's own. Every value that steers the loop is wave-uniform.
__device__ int pq_snappy_wave(const uint8_t* __restrict__ src, int64_t n, uint8_t* dst, int64_t dst_len, uint8_t* win) {
    const int lane = (int)lane_id();
    int64_t wbase = 0, wend = 0;
    auto fill = [&](int64_t at) {
        wave_lds_sync();                                     // the earlier reads of the window are done
        wbase = at;
        wend = at + PQ_WIN < n ? at + PQ_WIN : n;
        for (int64_t i = lane; i < wend - wbase; i += WAVE) win[i] = src[at + i];
        wave_lds_sync();
    };
    fill(0);
    int64_t ip = 0, op = 0, waited = 0;                      // waited: the output below it was stored before the last wait
    int st = pq_snappy_preamble(win, &ip, wend, dst_len);
    if (st != PQ_OK) return st;
    while (ip < n) {
        if (ip + 5 > wend && wend < n) fill(ip);
        int64_t rel = ip - wbase;
        pq_snappy_elem e;
        st = pq_snappy_tag(win, &rel, wend - wbase, &e);
        if (st != PQ_OK) return st;
        e.kind = __builtin_amdgcn_readfirstlane(e.kind);
        e.len = __builtin_amdgcn_readfirstlane(e.len);
        e.offset = __builtin_amdgcn_readfirstlane(e.offset);
        ip = wbase + rel;
        st = pq_snappy_check(e, ip, n, op, dst_len);
        if (st != PQ_OK) return st;
        const int64_t len = (int64_t)e.len;
        if (e.kind == 0) {
            for (int64_t i = lane; i < len; i += WAVE) dst[op + i] = src[ip + i];
            ip += len;
        } else {
            const int64_t off = (int64_t)e.offset, s0 = op - off;
            if (s0 + (len < off ? len : off) > waited) {     // the source holds bytes this wave stored since the last wait
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                __builtin_amdgcn_s_waitcnt(0x0F70);          // vmcnt(0): the stores have landed
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                waited = op;
            }
            if (off >= len) {
                for (int64_t i = lane; i < len; i += WAVE) dst[op + i] = dst[s0 + i];
            } else {                                         // overlapping: the pattern of `off` bytes repeats
                for (int64_t i = lane; i < len; i += WAVE) dst[op + i] = dst[s0 + i % off];
            }
        }
        op += len;
    }
    return op == dst_len ? PQ_OK : PQ_E_SNAPPY_SHORT;
}

__global__ __launch_bounds__(PQ_THREADS) void k_pq_snappy(const uint8_t* __restrict__ bytes, const PqStream* __restrict__ streams,
                                                          int64_t n_streams, uint8_t* out, int32_t* __restrict__ status,
                                                          unsigned long long* err) {
    __shared__ uint8_t s_win[PQ_WAVES][PQ_WIN];
    const int64_t i = (int64_t)blockIdx.x * PQ_WAVES + (threadIdx.x >> 6);
    if (i >= n_streams) return;                              // wave-uniform
    const PqStream s = streams[i];
    int st = PQ_OK;
    if (s.n >= 0) st = pq_snappy_wave(bytes + s.src, s.n, out + s.dst, s.dst_len, s_win[threadIdx.x >> 6]);
    if (lane_id() == 0) {
        status[i] = st;
        if (st != PQ_OK && err) atomicMin(err, (unsigned long long)i << 8 | (unsigned long long)st);
    }
}

__device__ __forceinline__ const uint8_t* pq_body(const PqPage& pg, const uint8_t* bytes, const uint8_t* bodies) {
    return (pg.in_work ? bodies : bytes) + pg.body;
}

__global__ __launch_bounds__(WAVE) void k_pq_runs(const uint8_t* __restrict__ bytes, const uint8_t* __restrict__ bodies,
                                                  const PqPage* __restrict__ pages, const PqCol* __restrict__ cols, int64_t n_pages,
                                                  const int32_t* __restrict__ sstat, int64_t* __restrict__ vstart,
                                                  int64_t* __restrict__ marks, unsigned long long* err) {
    const int64_t p = (int64_t)blockIdx.x * WAVE + threadIdx.x;
    if (p >= n_pages) return;
    const PqPage pg = pages[p];
    if (pg.plain == 2) return;                               // k_pq_delta_walk's page
    int64_t start = -1;
    int st = sstat[p];
    if (st == PQ_OK) {
        start = 0;
        if (pg.type != 2) {
            const uint8_t* b = pq_body(pg, bytes, bodies);
            if (pg.dict >= 0 && sstat[pg.dict] != PQ_OK) st = -1;             // reported by the dictionary page
            if (st == PQ_OK) st = pq_v1_values_start(b, pg.body_len, pg.levels != 0, pg.num_values, &start);
            if (st == PQ_OK) {
                if (pg.plain) {
                    if (pg.body_len - start != pg.num_values * cols[pg.col].phys) st = PQ_E_SIZE;
                } else {
                    int width = 0;
                    st = pq_walk_runs(b, start, pg.body_len, pg.num_values, marks + 2 * pg.mark0, &width);
                }
            }
        }
        if (st > PQ_OK) atomicMin(err, (unsigned long long)p << 8 | (unsigned long long)st);
        if (st != PQ_OK) start = -1;
    }
    vstart[p] = start;
}

// ---- delta pages ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_pq_delta_walk(const uint8_t* __restrict__ bytes, const uint8_t* __restrict__ bodies,
                                                        const PqPage* __restrict__ pages, const PqCol* __restrict__ cols,
                                                        const PqDelta* __restrict__ dpages, int64_t n_delta,
                                                        const int32_t* __restrict__ sstat, int64_t* __restrict__ vstart,
                                                        pq_delta_head* __restrict__ heads, PqBlock* __restrict__ blocks,
                                                        unsigned long long* err) {
    const int64_t d = (int64_t)blockIdx.x * WAVE + threadIdx.x;
    if (d >= n_delta) return;
    const int64_t p = dpages[d].page;
    const PqPage pg = pages[p];
    int64_t start = -1;
    pq_delta_head h = {};
    if (sstat[p] == PQ_OK) {
        const uint8_t* b = pq_body(pg, bytes, bodies);
        int st = pq_v1_values_start(b, pg.body_len, pg.levels != 0, pg.num_values, &start);
        if (st == PQ_OK) {                                   // a PqBlock opens with the two int64 of pq_delta_walk's record
            st = pq_delta_walk(b, start, pg.body_len, pg.num_values, cols[pg.col].phys, &h, (int64_t*)(blocks + dpages[d].blk0),
                               (int)(sizeof(PqBlock) / 8));
        }
        if (st != PQ_OK) {
            atomicMin(err, (unsigned long long)p << 8 | (unsigned long long)st);
            start = -1;
        }
    }
    vstart[p] = start;
    heads[d] = h;
}

// The delta page that owns block slot `slot` (the last one whose first slot is <= slot; a page without slots is never the
// last such one, since the page behind it starts at the same slot) -> its index among the delta pages
__device__ __forceinline__ int64_t pq_delta_of_slot(const PqDelta* __restrict__ dpages, int64_t n_delta, int64_t slot) {
    int64_t lo = 0, hi = n_delta - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (dpages[mid].blk0 <= slot) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The 64 values i0 + lane of one block, i0 a multiple of 64: min_delta + field where the value exists (i < in_block), else 0.
// cur: the cursor at value i0, moved to i0 + 64. Wave-uniform but for the lane's own half.
__device__ __forceinline__ uint64_t pq_delta_chunk(const uint8_t* b, const PqBlock& k, int mv, int64_t i0, int64_t in_block,
                                                   pq_delta_cursor* cur) {
    const int lane = (int)lane_id();
    const pq_delta_cursor lo = *cur;
    pq_delta_advance(b, k.widths, mv, cur);
    const pq_delta_cursor hi = *cur;
    pq_delta_advance(b, k.widths, mv, cur);
    const pq_delta_cursor c = lane < 32 ? lo : hi;
    if (i0 + lane >= in_block) return 0;
    return (uint64_t)k.min_delta + pq_delta_field(b, c.off, c.k + (lane & 31), b[k.widths + c.j]);
}

// what the three block kernels share: the slot's page and block, or false when the slot is not a block of a clean page
struct PqDeltaBlock {
    PqPage pg;
    pq_delta_head h;
    const uint8_t* b;
    int64_t blk, in_block;
    PqBlock* rec;
};
__device__ __forceinline__ bool pq_delta_block(const uint8_t* bytes, const uint8_t* bodies, const PqPage* pages, const PqDelta* dpages,
                                               int64_t n_delta, const int64_t* vstart, const pq_delta_head* heads, PqBlock* blocks,
                                               int64_t slot, PqDeltaBlock* o) {
    const int64_t d = pq_delta_of_slot(dpages, n_delta, slot);
    const PqDelta dp = dpages[d];
    if (vstart[dp.page] < 0) return false;
    o->h = heads[d];
    o->blk = slot - dp.blk0;
    if (o->blk >= o->h.n_blocks) return false;
    o->pg = pages[dp.page];
    o->b = pq_body(o->pg, bytes, bodies);
    const int64_t left = o->h.n - 1 - o->blk * o->h.B;
    o->in_block = left < o->h.B ? left : o->h.B;
    o->rec = blocks + slot;
    return true;
}

__global__ __launch_bounds__(PQ_THREADS) void k_pq_delta_sum(const uint8_t* __restrict__ bytes, const uint8_t* __restrict__ bodies,
                                                             const PqPage* __restrict__ pages, const PqDelta* __restrict__ dpages,
                                                             int64_t n_delta, int64_t n_slots, const int64_t* __restrict__ vstart,
                                                             const pq_delta_head* __restrict__ heads, PqBlock* __restrict__ blocks) {
    const int64_t slot = (int64_t)blockIdx.x * PQ_WAVES + (threadIdx.x >> 6);
    if (slot >= n_slots) return;                             // wave-uniform
    PqDeltaBlock o;
    if (!pq_delta_block(bytes, bodies, pages, dpages, n_delta, vstart, heads, blocks, slot, &o)) return;
    const PqBlock k = *o.rec;
    pq_delta_cursor cur = {k.widths + o.h.M, 0, 0};
    uint64_t sum = 0;
    for (int64_t i0 = 0; i0 < o.in_block; i0 += WAVE) sum += pq_delta_chunk(o.b, k, o.h.mv, i0, o.in_block, &cur);
    sum = wave_reduce<Sum>(sum);
    if (lane_id() == 0) o.rec->base = sum;
}

__global__ __launch_bounds__(WAVE) void k_pq_delta_scan(const PqPage* __restrict__ pages, const PqCol* __restrict__ cols,
                                                        const PqDelta* __restrict__ dpages, const int64_t* __restrict__ vstart,
                                                        const pq_delta_head* __restrict__ heads, PqBlock* __restrict__ blocks) {
    const int64_t d = blockIdx.x;
    const PqDelta dp = dpages[d];
    if (vstart[dp.page] < 0) return;
    const pq_delta_head h = heads[d];
    if (h.n == 0) return;
    const int lane = (int)lane_id();
    const PqPage pg = pages[dp.page];
    const PqCol col = cols[pg.col];
    if (lane == 0) pq_store(col.out, pg.out_row, col.elem, pq_widen((uint64_t)h.first, col.phys, col.zext != 0));
    uint64_t carry = (uint64_t)h.first;
    for (int64_t b0 = 0; b0 < h.n_blocks; b0 += WAVE) {
        const int64_t b = b0 + lane;
        const uint64_t v = b < h.n_blocks ? blocks[dp.blk0 + b].base : 0;
        const uint64_t incl = wave_incl_scan<uint64_t>(v);
        if (b < h.n_blocks) blocks[dp.blk0 + b].base = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
}

__global__ __launch_bounds__(PQ_THREADS) void k_pq_delta_out(const uint8_t* __restrict__ bytes, const uint8_t* __restrict__ bodies,
                                                             const PqPage* __restrict__ pages, const PqCol* __restrict__ cols,
                                                             const PqDelta* __restrict__ dpages, int64_t n_delta, int64_t n_slots,
                                                             const int64_t* __restrict__ vstart, const pq_delta_head* __restrict__ heads,
                                                             PqBlock* __restrict__ blocks) {
    const int64_t slot = (int64_t)blockIdx.x * PQ_WAVES + (threadIdx.x >> 6);
    if (slot >= n_slots) return;                             // wave-uniform
    PqDeltaBlock o;
    if (!pq_delta_block(bytes, bodies, pages, dpages, n_delta, vstart, heads, blocks, slot, &o)) return;
    const PqBlock k = *o.rec;
    const PqCol col = cols[o.pg.col];
    const int lane = (int)lane_id();
    const int64_t row0 = o.pg.out_row + 1 + o.blk * o.h.B;   // value 0 of the page is k_pq_delta_scan's
    pq_delta_cursor cur = {k.widths + o.h.M, 0, 0};
    uint64_t carry = k.base;
    for (int64_t i0 = 0; i0 < o.in_block; i0 += WAVE) {
        const uint64_t incl = wave_incl_scan<uint64_t>(pq_delta_chunk(o.b, k, o.h.mv, i0, o.in_block, &cur));
        if (i0 + lane < o.in_block) pq_store(col.out, row0 + i0 + lane, col.elem, pq_widen(carry + incl, col.phys, col.zext != 0));
        carry += __shfl(incl, 63, 64);
    }
}

__device__ __forceinline__ uint64_t pq_value(const uint8_t* p, int64_t i, int phys) {
    if (phys == 8) {
        uint64_t v;
        __builtin_memcpy(&v, p + i * 8, 8);
        return v;
    }
    uint32_t v;
    __builtin_memcpy(&v, p + i * 4, 4);
    return v;
}

__global__ __launch_bounds__(PQ_THREADS) void k_pq_decode(const uint8_t* __restrict__ bytes, const uint8_t* __restrict__ bodies,
                                                          const PqPage* __restrict__ pages, const PqCol* __restrict__ cols,
                                                          int64_t n_pages, int64_t n_tiles, const int64_t* __restrict__ vstart,
                                                          const int64_t* __restrict__ marks, unsigned long long* err) {
    const int64_t tile = (int64_t)blockIdx.x * PQ_WAVES + (threadIdx.x >> 6);
    if (tile >= n_tiles) return;                             // wave-uniform
    const int lane = (int)lane_id();
    int64_t lo_p = 0, hi_p = n_pages - 1;                    // the last page whose first tile is <= tile
    while (lo_p < hi_p) {
        const int64_t mid = (lo_p + hi_p + 1) >> 1;
        if (pages[mid].tile0 <= tile) lo_p = mid; else hi_p = mid - 1;
    }
    const int64_t p = lo_p;
    const PqPage pg = pages[p];
    const int64_t start = vstart[p];
    if (start < 0 || pg.type == 2) return;
    const PqCol col = cols[pg.col];
    const uint8_t* b = pq_body(pg, bytes, bodies);
    const int64_t t = tile - pg.tile0;
    const int64_t lo = t * PQ_TILE, hi = lo + PQ_TILE < pg.num_values ? lo + PQ_TILE : pg.num_values;
    if (pg.plain) {
        for (int64_t v = lo + lane; v < hi; v += WAVE)
            pq_store(col.out, pg.out_row + v, col.elem, pq_widen(pq_value(b + start, v, col.phys), col.phys, col.zext != 0));
        return;
    }
    const PqPage dp = pages[pg.dict];
    if (vstart[pg.dict] < 0) return;
    const uint8_t* d = pq_body(dp, bytes, bodies);
    const int width = b[start];
    int64_t pos = marks[2 * (pg.mark0 + t)], seen = marks[2 * (pg.mark0 + t) + 1];
    bool bad = false;
    while (seen < hi) {
        pq_run r;
        if (!pq_run_header(b, &pos, pg.body_len, width, &r)) break;             // k_pq_runs has walked these headers
        const int64_t last = seen + (int64_t)r.count;
        const int64_t a = seen > lo ? seen : lo, z = last < hi ? last : hi;
        for (int64_t v = a + lane; v < z; v += WAVE) {
            const uint32_t idx = r.packed ? pq_bits(b, r.data, pg.body_len, v - seen, width) : r.value;
            if ((int64_t)idx >= dp.num_values) {
                bad = true;
            } else {
                pq_store(col.out, pg.out_row + v, col.elem, pq_widen(pq_value(d, idx, col.phys), col.phys, col.zext != 0));
            }
        }
        seen = last;
    }
    if (bad) atomicMin(err, (unsigned long long)p << 8 | (unsigned long long)PQ_E_INDEX);
}

// The host's check of the table and the device records it becomes. Returns the bytes of decompressed bodies and the
// number of tiles; -22 with the error set on a record that would read or write outside its buffers.
struct PqPlan {
    std::vector<PqPage> pages;
    std::vector<PqStream> streams;
    std::vector<PqDelta> deltas;
    int64_t tiles = 0, body_bytes = 0, slots = 0;           // slots: block records, one per 128 deltas of every delta page
};

static int pq_plan(const int64_t* h_pages, int64_t n_pages, int64_t n_bytes, const int64_t* h_cols, int32_t n_cols, PqPlan* plan) {
    OTTO_REQUIRE(n_pages >= 0 && n_pages < (1ll << 24), "otto_parquet: n_pages must be in [0, 2^24)");
    OTTO_REQUIRE(n_pages == 0 || h_pages, "otto_parquet: null page table");
    plan->pages.resize((size_t)n_pages);
    plan->streams.resize((size_t)n_pages);
    for (int64_t p = 0; p < n_pages; ++p) {
        const int64_t* r = h_pages + p * OTTO_PQ_FIELDS;
        const int64_t src = r[OTTO_PQ_SRC_OFF], comp = r[OTTO_PQ_COMP_SIZE], uncomp = r[OTTO_PQ_UNCOMP_SIZE];
        const int64_t type = r[OTTO_PQ_PAGE_TYPE], enc = r[OTTO_PQ_ENCODING], nv = r[OTTO_PQ_NUM_VALUES];
        const int64_t col = r[OTTO_PQ_COL_SLOT], dict = r[OTTO_PQ_DICT_SLOT];
        int64_t lev = 0;
        OTTO_REQUIRE(type == 0 || type == 2 || type == 3, "otto_parquet: page %lld: page type %lld", (long long)p, (long long)type);
        OTTO_REQUIRE(enc == 0 || enc == 2 || enc == 8 || (enc == 5 && type != 2), "otto_parquet: page %lld: encoding %lld", (long long)p,
                     (long long)enc);
        OTTO_REQUIRE(src >= 0 && comp >= 0 && uncomp >= 0 && comp < (1ll << 31) && uncomp < (1ll << 31) && nv >= 0 && nv < (1ll << 31),
                     "otto_parquet: page %lld: negative or oversized extent", (long long)p);
        OTTO_REQUIRE(n_bytes < 0 || src + comp <= n_bytes, "otto_parquet: page %lld: body outside the %lld bytes", (long long)p,
                     (long long)n_bytes);
        OTTO_REQUIRE(col >= 0 && (n_cols < 0 || col < n_cols), "otto_parquet: page %lld: column slot %lld", (long long)p, (long long)col);
        if (type == 3) {
            lev = r[OTTO_PQ_DEF_LEN] + r[OTTO_PQ_REP_LEN];
            OTTO_REQUIRE(r[OTTO_PQ_DEF_LEN] >= 0 && r[OTTO_PQ_REP_LEN] >= 0 && lev <= comp && lev <= uncomp,
                         "otto_parquet: page %lld: level lengths outside the page", (long long)p);
        } else {
            OTTO_REQUIRE(r[OTTO_PQ_REP_LEN] == 0 && (r[OTTO_PQ_DEF_LEN] == 0 || (type == 0 && r[OTTO_PQ_DEF_LEN] == -1)),
                         "otto_parquet: page %lld: level lengths of a V1 page", (long long)p);
        }
        PqPage& g = plan->pages[(size_t)p];
        PqStream& s = plan->streams[(size_t)p];
        g.num_values = nv;
        g.out_row = r[OTTO_PQ_OUT_ROW];
        g.type = (int32_t)type;
        g.plain = type == 2 || enc == 0 ? 1 : enc == 5 ? 2 : 0;
        g.levels = type == 0 && r[OTTO_PQ_DEF_LEN] == -1;
        g.col = (int32_t)col;
        g.dict = -1;
        g.tile0 = plan->tiles;
        g.mark0 = plan->tiles;
        if (r[OTTO_PQ_IS_COMPRESSED]) {
            g.in_work = 1;
            g.body = plan->body_bytes;
            g.body_len = uncomp - lev;
            s = PqStream{src + lev, comp - lev, g.body, g.body_len};
            plan->body_bytes += (g.body_len + 15) & ~(int64_t)15;
        } else {
            OTTO_REQUIRE(comp == uncomp, "otto_parquet: page %lld: %s (%lld stored, %lld declared)", (long long)p, pq_reason(PQ_E_SIZE),
                         (long long)comp, (long long)uncomp);
            g.in_work = 0;
            g.body = src + lev;
            g.body_len = comp - lev;
            s = PqStream{0, -1, 0, 0};
        }
        if (type == 2) {
            OTTO_REQUIRE(dict == -1, "otto_parquet: page %lld: a dictionary page names a dictionary", (long long)p);
            if (h_cols) {
                OTTO_REQUIRE(g.body_len == nv * h_cols[col * OTTO_PQ_COL_FIELDS + OTTO_PQ_COL_PHYS],
                             "otto_parquet: page %lld: %s (dictionary of %lld values in %lld bytes)", (long long)p, pq_reason(PQ_E_SIZE),
                             (long long)nv, (long long)g.body_len);
            }
        } else {
            if (g.plain == 0) {
                OTTO_REQUIRE(dict >= 0 && dict < p && plan->pages[(size_t)dict].type == 2 && plan->pages[(size_t)dict].col == g.col,
                             "otto_parquet: page %lld: dictionary slot %lld", (long long)p, (long long)dict);
                g.dict = (int32_t)dict;
            }
            if (h_cols) {
                OTTO_REQUIRE(g.out_row >= 0 && g.out_row + nv <= h_cols[col * OTTO_PQ_COL_FIELDS + OTTO_PQ_COL_ROWS],
                             "otto_parquet: page %lld: rows %lld + %lld outside the column's %lld", (long long)p, (long long)g.out_row,
                             (long long)nv, (long long)h_cols[col * OTTO_PQ_COL_FIELDS + OTTO_PQ_COL_ROWS]);
            }
            if (g.plain == 2) {                               // no tile of k_pq_decode: the delta kernels' page
                plan->deltas.push_back(PqDelta{p, plan->slots});
                plan->slots += (nv > 1 ? nv - 1 + 127 : 0) / 128;
            } else {
                plan->tiles += (nv + PQ_TILE - 1) / PQ_TILE;
            }
        }
    }
    return 0;
}

}  // namespace otto

using namespace otto;

extern "C" const char* otto_parquet_reason(int32_t code) { return pq_reason(code); }

extern "C" int64_t otto_parquet_workspace(const int64_t* h_pages, int64_t n_pages) {
    PqPlan plan;
    if (pq_plan(h_pages, n_pages, -1, nullptr, -1, &plan) != 0) return -22;
    return (int64_t)pq_layout(n_pages, plan.tiles, plan.body_bytes, (int64_t)plan.deltas.size(), plan.slots, nullptr, nullptr);
}

extern "C" int otto_parquet_decode(const uint8_t* d_bytes, int64_t n_bytes, const int64_t* h_pages, int64_t n_pages, const int64_t* h_cols,
                                   int32_t n_cols, int32_t phases, void* d_work, int64_t work_bytes, int64_t* h_err, void* stream) {
    OTTO_REQUIRE(h_err, "otto_parquet_decode: null h_err");
    h_err[0] = -1;
    h_err[1] = 0;
    OTTO_REQUIRE(n_bytes >= 0 && n_bytes < (1ll << 31), "otto_parquet_decode: n_bytes must be in [0, 2^31)");
    OTTO_REQUIRE(n_cols >= 0 && n_cols <= PQ_MAX_COLS && (n_cols == 0 || h_cols), "otto_parquet_decode: n_cols must be in [0, %d]", PQ_MAX_COLS);
    OTTO_REQUIRE((phases & ~3) == 0 && phases != 0, "otto_parquet_decode: phases must be 1, 2 or 3");
    PqCol hc[PQ_MAX_COLS] = {};
    for (int c = 0; c < n_cols; ++c) {
        const int64_t* r = h_cols + c * OTTO_PQ_COL_FIELDS;
        const int64_t elem = r[OTTO_PQ_COL_ELEM], phys = r[OTTO_PQ_COL_PHYS];
        OTTO_REQUIRE(elem == 1 || elem == 2 || elem == 4 || elem == 8, "otto_parquet_decode: column %d: element size %lld", c, (long long)elem);
        OTTO_REQUIRE(phys == 4 || phys == 8, "otto_parquet_decode: column %d: physical size %lld", c, (long long)phys);
        OTTO_REQUIRE(r[OTTO_PQ_COL_ROWS] >= 0 && (r[OTTO_PQ_COL_ROWS] == 0 || r[OTTO_PQ_COL_OUT]), "otto_parquet_decode: column %d: null output", c);
        OTTO_REQUIRE((r[OTTO_PQ_COL_OUT] & (elem - 1)) == 0, "otto_parquet_decode: column %d: misaligned output", c);
        hc[c] = PqCol{(void*)(uintptr_t)r[OTTO_PQ_COL_OUT], (int32_t)elem, (int32_t)phys, (int32_t)(r[OTTO_PQ_COL_ZEXT] != 0), 0};
    }
    PqPlan plan;
    OTTO_TRY(pq_plan(h_pages, n_pages, n_bytes, h_cols, n_cols, &plan));
    if (n_pages == 0) return 0;
    OTTO_REQUIRE(d_bytes && d_work, "otto_parquet_decode: null argument");
    OTTO_REQUIRE(((uintptr_t)d_bytes & 15) == 0 && ((uintptr_t)d_work & 255) == 0, "otto_parquet_decode: d_bytes must be 16-byte, d_work 256-byte aligned");
    PqWs w;
    const int64_t n_delta = (int64_t)plan.deltas.size();
    const int64_t need = (int64_t)pq_layout(n_pages, plan.tiles, plan.body_bytes, n_delta, plan.slots, (char*)d_work, &w);
    OTTO_REQUIRE(work_bytes >= need, "otto_parquet_decode: workspace too small (%lld < %lld)", (long long)work_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    OTTO_HIP(hipMemsetAsync(w.err, 0xFF, 8, s));
    OTTO_HIP(hipMemcpyAsync(w.pages, plan.pages.data(), (size_t)n_pages * sizeof(PqPage), hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.streams, plan.streams.data(), (size_t)n_pages * sizeof(PqStream), hipMemcpyHostToDevice, s));
    OTTO_HIP(hipMemcpyAsync(w.cols, hc, sizeof(hc), hipMemcpyHostToDevice, s));
    if (n_delta > 0) OTTO_HIP(hipMemcpyAsync(w.dpages, plan.deltas.data(), (size_t)n_delta * sizeof(PqDelta), hipMemcpyHostToDevice, s));
    if (phases & OTTO_PQ_PHASE_SNAPPY) {
        k_pq_snappy<<<(unsigned)((n_pages + PQ_WAVES - 1) / PQ_WAVES), PQ_THREADS, 0, s>>>(d_bytes, w.streams, n_pages, w.bodies, w.sstat, w.err);
        OTTO_HIP(hipGetLastError());
    }
    if (phases & OTTO_PQ_PHASE_DECODE) {
        k_pq_runs<<<(unsigned)((n_pages + WAVE - 1) / WAVE), WAVE, 0, s>>>(d_bytes, w.bodies, w.pages, w.cols, n_pages, w.sstat, w.vstart,
                                                                          w.marks, w.err);
        OTTO_HIP(hipGetLastError());
        if (plan.tiles > 0) {
            k_pq_decode<<<(unsigned)((plan.tiles + PQ_WAVES - 1) / PQ_WAVES), PQ_THREADS, 0, s>>>(d_bytes, w.bodies, w.pages, w.cols, n_pages,
                                                                                                plan.tiles, w.vstart, w.marks, w.err);
            OTTO_HIP(hipGetLastError());
        }
        if (n_delta > 0) {
            k_pq_delta_walk<<<(unsigned)((n_delta + WAVE - 1) / WAVE), WAVE, 0, s>>>(d_bytes, w.bodies, w.pages, w.cols, w.dpages, n_delta, w.sstat,
                                                                                   w.vstart, w.dheads, w.blocks, w.err);
            OTTO_HIP(hipGetLastError());
            const unsigned grid = (unsigned)((plan.slots + PQ_WAVES - 1) / PQ_WAVES);
            if (grid > 0) {
                k_pq_delta_sum<<<grid, PQ_THREADS, 0, s>>>(d_bytes, w.bodies, w.pages, w.dpages, n_delta, plan.slots, w.vstart, w.dheads, w.blocks);
                OTTO_HIP(hipGetLastError());
            }
            k_pq_delta_scan<<<(unsigned)n_delta, WAVE, 0, s>>>(w.pages, w.cols, w.dpages, w.vstart, w.dheads, w.blocks);
            OTTO_HIP(hipGetLastError());
            if (grid > 0) {
                k_pq_delta_out<<<grid, PQ_THREADS, 0, s>>>(d_bytes, w.bodies, w.pages, w.cols, w.dpages, n_delta, plan.slots, w.vstart, w.dheads,
                                                           w.blocks);
                OTTO_HIP(hipGetLastError());
            }
        }
    }
    unsigned long long herr = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, w.err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (herr != ~0ull) {
        h_err[0] = (int64_t)(herr >> 8);
        h_err[1] = (int64_t)(herr & 0xFF);
        OTTO_REQUIRE(false, "otto_parquet_decode: page %lld: %s", (long long)h_err[0], pq_reason((int)h_err[1]));
    }
    return 0;
}

extern "C" int64_t otto_parquet_snappy_workspace(int64_t n_streams) {
    return (int64_t)(pq_align((size_t)(n_streams > 0 ? n_streams : 0) * sizeof(PqStream)) + pq_align((size_t)(n_streams > 0 ? n_streams : 0) * 4));
}

extern "C" int otto_parquet_snappy(const uint8_t* d_bytes, int64_t n_bytes, const int64_t* h_src_off, const int64_t* h_src_len,
                                   const int64_t* h_dst_off, const int64_t* h_dst_len, int64_t n_streams, uint8_t* d_out, int64_t out_bytes,
                                   int32_t* h_status, void* d_work, int64_t work_bytes, void* stream) {
    OTTO_REQUIRE(n_streams >= 0 && n_streams < (1ll << 24), "otto_parquet_snappy: n_streams must be in [0, 2^24)");
    OTTO_REQUIRE(n_bytes >= 0 && n_bytes < (1ll << 31) && out_bytes >= 0, "otto_parquet_snappy: n_bytes must be in [0, 2^31)");
    if (n_streams == 0) return 0;
    OTTO_REQUIRE(h_src_off && h_src_len && h_dst_off && h_dst_len && h_status && d_work, "otto_parquet_snappy: null argument");
    OTTO_REQUIRE((n_bytes == 0 || d_bytes) && (out_bytes == 0 || d_out), "otto_parquet_snappy: null buffer");
    OTTO_REQUIRE(work_bytes >= otto_parquet_snappy_workspace(n_streams), "otto_parquet_snappy: workspace too small");
    std::vector<PqStream> st((size_t)n_streams);
    for (int64_t i = 0; i < n_streams; ++i) {
        OTTO_REQUIRE(h_src_off[i] >= 0 && h_src_len[i] >= 0 && h_src_off[i] + h_src_len[i] <= n_bytes,
                     "otto_parquet_snappy: stream %lld: input extent outside the %lld bytes", (long long)i, (long long)n_bytes);
        OTTO_REQUIRE(h_dst_off[i] >= 0 && h_dst_len[i] >= 0 && h_dst_len[i] < (1ll << 31) && h_dst_off[i] + h_dst_len[i] <= out_bytes,
                     "otto_parquet_snappy: stream %lld: output extent outside the %lld bytes", (long long)i, (long long)out_bytes);
        st[(size_t)i] = PqStream{h_src_off[i], h_src_len[i], h_dst_off[i], h_dst_len[i]};
    }
    hipStream_t s = (hipStream_t)stream;
    PqStream* d_st = (PqStream*)d_work;
    int32_t* d_status = (int32_t*)((char*)d_work + pq_align((size_t)n_streams * sizeof(PqStream)));
    OTTO_HIP(hipMemcpyAsync(d_st, st.data(), (size_t)n_streams * sizeof(PqStream), hipMemcpyHostToDevice, s));
    k_pq_snappy<<<(unsigned)((n_streams + PQ_WAVES - 1) / PQ_WAVES), PQ_THREADS, 0, s>>>(d_bytes, d_st, n_streams, d_out, d_status, nullptr);
    OTTO_HIP(hipGetLastError());
    OTTO_HIP(hipMemcpyAsync(h_status, d_status, (size_t)n_streams * 4, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    return 0;
}
