// Scalar pieces of SPEC-PQLIST (include/otto_pqlist.h), as host/device functions over the run headers and the bit extraction
// of parquet_decode.h: the kernels of otto_pqlist.hip run them, tools/pqlist_host_main.cpp runs the same code on the CPU
// under the sanitizers.
//
// As in parquet_decode.h every function works on p[0 .. end): nothing at or past `end` is read, whatever the bytes say.
#pragma once
#include "parquet_decode.h"
#include "../../include/otto_pqlist.h"

// Where the two level streams of a page lie inside its body; offsets relative to the body
struct pl_extents {
    int64_t rep_end, def_pos, def_end;                      // def_end = the bytes of the levels
    int32_t rep_pos, ok;
};

OTTO_PQ_HD int pl_def_max(int flags) { return 1 + (flags & OTTO_PL_F_OUTER_OPTIONAL) + ((flags >> 1) & 1); }
OTTO_PQ_HD int pl_def_width(int flags) { return pl_def_max(flags) == 1 ? 1 : 2; }

// The V1 length prefixes of the body b[0 .. len) (type 0), or the header's two lengths (type 3) -> the extents, or
// OTTO_PL_E_PREFIX when they run past the body
OTTO_PQ_HD int pl_page_extents(const uint8_t* b, int64_t len, int type, int64_t rep_len, int64_t def_len, pl_extents* f) {
    f->ok = 0;
    if (type == 0) {
        if (len < 4) return OTTO_PL_E_PREFIX;
        const int64_t rl = (int64_t)pq_load_le(b, 0, 4);
        if (8 + rl > len) return OTTO_PL_E_PREFIX;
        const int64_t dl = (int64_t)pq_load_le(b, 4 + rl, 4);
        if (8 + rl + dl > len) return OTTO_PL_E_PREFIX;
        f->rep_pos = 4;
        f->rep_end = 4 + rl;
        f->def_pos = 8 + rl;
        f->def_end = 8 + rl + dl;
    } else {
        if (rep_len < 0 || def_len < 0 || rep_len + def_len > len) return OTTO_PL_E_PREFIX;
        f->rep_pos = 0;
        f->rep_end = rep_len;
        f->def_pos = rep_len;
        f->def_end = rep_len + def_len;
    }
    return 0;
}

// One level stream at p[pos .. end), n entries of `width` bits: every run header, checked; mark[4 t], mark[4 t + 1] = the
// header byte and the first entry of the run that holds entry t * OTTO_PQ_TILE (the other stream's pair lies at + 2).
OTTO_PQ_HD int pl_walk_stream(const uint8_t* p, int64_t pos, int64_t end, int width, int64_t n, int64_t* mark) {
    int64_t seen = 0, next = 0;
    while (seen < n) {
        if (pos >= end) return OTTO_PL_E_SHORT;
        const int64_t at = pos;
        pq_run r;
        if (!pq_run_header(p, &pos, end, width, &r)) return OTTO_PL_E_RUNS;
        const int64_t last = seen + (int64_t)r.count;
        if (r.packed) {                                      // the entries the page needs from the run must lie inside the stream
            const int64_t need = (last < n ? last : n) - seen;
            if (r.data + (need * width + 7) / 8 > end) return OTTO_PL_E_SHORT;
            if (last - n >= 8) return OTTO_PL_E_LONG;
        } else if (last > n) {
            return OTTO_PL_E_LONG;
        }
        while (next < n && next < last) {
            mark[4 * (next / OTTO_PQ_TILE)] = at;
            mark[4 * (next / OTTO_PQ_TILE) + 1] = seen;
            next += OTTO_PQ_TILE;
        }
        seen = last;
    }
    return pos == end ? 0 : OTTO_PL_E_LONG;
}

// Entries [lo, hi) of a walked stream -> dst[0 .. hi - lo), from the checkpoint (pos, seen). `lane` of `lanes` callers
// share the work: each takes every lanes-th entry of a run (a wave: lane_id() of 64; the host: 0 of 1).
OTTO_PQ_HD void pl_expand(const uint8_t* b, int64_t pos, int64_t seen, int64_t end, int width, int64_t lo, int64_t hi, uint8_t* dst,
                          int lane, int lanes) {
    while (seen < hi) {
        pq_run r;
        if (!pq_run_header(b, &pos, end, width, &r)) break;                     // the walk has been over these headers
        const int64_t last = seen + (int64_t)r.count;
        const int64_t a = seen > lo ? seen : lo, z = last < hi ? last : hi;
        for (int64_t v = a + lane; v < z; v += lanes)
            dst[v - lo] = (uint8_t)(r.packed ? pq_bits(b, r.data, end, v - seen, width) : r.value > 255u ? 255u : r.value);
        seen = last;
    }
}

// The refusal of one entry (0: none), in the order of SPEC-PQLIST. chunk_first: the entry is the first of its column chunk.
OTTO_PQ_HD int pl_entry_check(int r, int d, int flags, bool chunk_first) {
    const int D = pl_def_max(flags), elem = (flags >> 1) & 1;
    if (r > 1 || d > D) return OTTO_PL_E_LEVEL;
    if (r == 1 && d < D - elem) return OTTO_PL_E_REP_EMPTY;
    if (elem && d == D - 1) return OTTO_PL_E_NULL_ELEM;
    if (chunk_first && r == 1) return OTTO_PL_E_CHUNK_REP;
    return 0;
}
