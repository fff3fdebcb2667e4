// Scalar element decoders of SPEC-PARQUET (include/otto_parquet.h), as host/device functions: the kernels of
// otto_parquet.hip run them, tools/parquet_host_main.cpp runs the same code on the CPU under the sanitizers.
//
// Every function works on p[0 .. end): nothing at or past `end` is read, whatever the bytes say, and every length a
// stream states is checked against `end` before it is used.
#pragma once
#include <stdint.h>
#include "../../include/otto_parquet.h"

#if defined(__HIPCC__)
#define OTTO_PQ_HD __host__ __device__ __forceinline__
#else
#define OTTO_PQ_HD static inline
#endif

enum { PQ_OK = 0, PQ_E_SNAPPY_TRUNC, PQ_E_SNAPPY_OFFSET, PQ_E_SNAPPY_OVERRUN, PQ_E_SNAPPY_PREAMBLE, PQ_E_SNAPPY_SHORT,
       PQ_E_LEVELS, PQ_E_NULL, PQ_E_WIDTH, PQ_E_RUNS, PQ_E_INDEX, PQ_E_SIZE, PQ_E_DELTA_VARINT, PQ_E_DELTA_SHAPE, PQ_E_DELTA_COUNT,
       PQ_E_DELTA_WIDTH, PQ_E_DELTA_TRUNC, PQ_E_DELTA_TRAILING, PQ_N_REASONS };

static inline const char* pq_reason(int r) {
    static const char* const names[PQ_N_REASONS] = {
        "no violation", "snappy: stream cut short inside an element", "snappy: copy offset is 0 or reaches before the output",
        "snappy: output runs past the declared uncompressed size", "snappy: preamble disagrees with the declared uncompressed size",
        "snappy: stream ends before the declared uncompressed size", "definition levels run past the page",
        "a null (definition level 0)", "dictionary index width above 32 bits", "index runs cut short, empty or short of num_values",
        "dictionary index not below the dictionary's size", "decoded size differs from the page header",
        "delta: a varint of more than 10 bytes or 64 bits", "delta: block shape (values per block, miniblocks per block) is not accepted",
        "delta: the header's value count differs from the page's", "delta: miniblock width above the physical type's bits",
        "delta: the stream runs past the page body", "delta: bytes behind the last miniblock"};
    return r >= 0 && r < PQ_N_REASONS ? names[r] : "?";
}

// ULEB128 of at most 32 bits at p[*pos .. end): false when it is cut short, longer than 5 bytes or overflows 32 bits
OTTO_PQ_HD bool pq_varint32(const uint8_t* p, int64_t* pos, int64_t end, uint32_t* out) {
    uint32_t v = 0;
    int64_t i = *pos;
    for (int shift = 0; shift < 35; shift += 7) {
        if (i >= end) return false;
        const uint32_t b = p[i++];
        if (shift == 28 && (b & 0xF0u)) return false;
        v |= (b & 0x7Fu) << shift;
        if (!(b & 0x80u)) {
            *pos = i;
            *out = v;
            return true;
        }
    }
    return false;
}

// `k` little-endian bytes at p[pos ..), k in 0..8; the caller has checked pos + k <= end
OTTO_PQ_HD uint64_t pq_load_le(const uint8_t* p, int64_t pos, int k) {
    uint64_t v = 0;
    for (int i = 0; i < k; ++i) v |= (uint64_t)p[pos + i] << (8 * i);
    return v;
}

// One Snappy element. kind 0: a literal of `len` bytes that start at p[*ip] after the call; kind 1: a copy of `len`
// bytes from `offset` bytes behind the output position. *ip moves past the tag and its length / offset bytes only.
struct pq_snappy_elem {
    uint32_t kind, len, offset;
};
OTTO_PQ_HD int pq_snappy_tag(const uint8_t* p, int64_t* ip, int64_t end, pq_snappy_elem* e) {
    int64_t i = *ip;
    if (i >= end) return PQ_E_SNAPPY_TRUNC;
    const uint32_t tag = p[i++];
    const uint32_t low = tag & 3u;
    if (low == 0) {
        uint32_t len = tag >> 2;
        if (len >= 60) {
            const int extra = (int)len - 59;              // 1 .. 4 bytes of length - 1
            if (i + extra > end) return PQ_E_SNAPPY_TRUNC;
            len = (uint32_t)pq_load_le(p, i, extra);
            i += extra;
            if (len == 0xFFFFFFFFu) return PQ_E_SNAPPY_OVERRUN;
        }
        e->kind = 0;
        e->len = len + 1;
        e->offset = 0;
    } else if (low == 1) {
        if (i + 1 > end) return PQ_E_SNAPPY_TRUNC;
        e->kind = 1;
        e->len = 4 + ((tag >> 2) & 7u);
        e->offset = (tag >> 5) << 8 | p[i];
        i += 1;
    } else {
        const int nb = low == 2 ? 2 : 4;
        if (i + nb > end) return PQ_E_SNAPPY_TRUNC;
        e->kind = 1;
        e->len = 1 + (tag >> 2);
        e->offset = (uint32_t)pq_load_le(p, i, nb);
        i += nb;
    }
    *ip = i;
    return PQ_OK;
}

// The checks of one element BEFORE any of its bytes is touched: ip is the position after pq_snappy_tag, op the bytes
// produced so far
OTTO_PQ_HD int pq_snappy_check(const pq_snappy_elem& e, int64_t ip, int64_t end, int64_t op, int64_t dst_len) {
    if (e.kind == 0) {
        if (ip + (int64_t)e.len > end) return PQ_E_SNAPPY_TRUNC;
    } else if (e.offset == 0 || (int64_t)e.offset > op) {
        return PQ_E_SNAPPY_OFFSET;
    }
    if (op + (int64_t)e.len > dst_len) return PQ_E_SNAPPY_OVERRUN;
    return PQ_OK;
}

// The preamble: the uncompressed length, which must be the one the page header (the caller) declares
OTTO_PQ_HD int pq_snappy_preamble(const uint8_t* p, int64_t* ip, int64_t end, int64_t dst_len) {
    uint32_t n = 0;
    if (!pq_varint32(p, ip, end, &n)) return PQ_E_SNAPPY_TRUNC;
    return (int64_t)n == dst_len ? PQ_OK : PQ_E_SNAPPY_PREAMBLE;
}

// One run header of the RLE / bit-packed hybrid at p[*pos .. end) for values of `width` bits. After the call *pos is
// the first byte behind the run. packed: `count` values (a multiple of 8) in count * width / 8 bytes at `data`; else
// `count` copies of `value`, which is stored in ceil(width / 8) bytes.
struct pq_run {
    uint32_t packed, count, value;
    int64_t data;
};
OTTO_PQ_HD bool pq_run_header(const uint8_t* p, int64_t* pos, int64_t end, int width, pq_run* r) {
    uint32_t h = 0;
    int64_t i = *pos;
    if (!pq_varint32(p, &i, end, &h)) return false;
    r->packed = h & 1u;
    r->data = i;
    r->value = 0;
    if (r->packed) {
        const int64_t groups = (int64_t)(h >> 1);
        if (groups == 0 || groups > (1 << 26)) return false;
        r->count = (uint32_t)(groups * 8);
        int64_t bytes = groups * width;
        if (i + bytes > end) {                            // writers may cut the padding of the last group
            bytes = end - i;
        }
        i += bytes;
    } else {
        r->count = h >> 1;
        if (r->count == 0) return false;
        const int vb = (width + 7) / 8;
        if (i + vb > end) return false;
        r->value = (uint32_t)pq_load_le(p, i, vb);
        i += vb;
    }
    *pos = i;
    return true;
}

// value `k` of a bit-packed run whose bytes start at p[data]; width in 0..32; bytes at or past `end` read as 0
OTTO_PQ_HD uint32_t pq_bits(const uint8_t* p, int64_t data, int64_t end, int64_t k, int width) {
    if (width == 0) return 0;
    const int64_t bit = k * width;
    int64_t b = data + (bit >> 3);
    const int sh = (int)(bit & 7);
    uint64_t v = 0;
    for (int i = 0; i < 5; ++i, ++b)
        if (b < end) v |= (uint64_t)p[b] << (8 * i);
    return (uint32_t)((v >> sh) & (width == 32 ? 0xFFFFFFFFull : ((1ull << width) - 1)));
}

// The V1 definition levels (max level 1) at p[pos .. end): RLE hybrid of width 1. Counts the first num_values levels
// that are 1 into *ones. false: the runs are malformed or hold fewer than num_values levels.
OTTO_PQ_HD bool pq_count_defined(const uint8_t* p, int64_t pos, int64_t end, int64_t num_values, int64_t* ones) {
    int64_t seen = 0, n1 = 0;
    while (seen < num_values) {
        pq_run r;
        if (!pq_run_header(p, &pos, end, 1, &r)) return false;
        int64_t take = (int64_t)r.count < num_values - seen ? (int64_t)r.count : num_values - seen;
        if (!r.packed) {
            if (r.value > 1) return false;
            n1 += r.value ? take : 0;
        } else {
            for (int64_t k = 0; k < take; ++k) n1 += pq_bits(p, r.data, end, k, 1);
        }
        seen += take;
    }
    *ones = n1;
    return true;
}

// Where the values of a data page start inside its decoded body p[0 .. end) and the page's verdict on its levels.
// has_levels: a V1 page of an OPTIONAL column (4-byte length, then the level runs).
OTTO_PQ_HD int pq_v1_values_start(const uint8_t* p, int64_t end, bool has_levels, int64_t num_values, int64_t* start) {
    *start = 0;
    if (!has_levels) return PQ_OK;
    if (end < 4) return PQ_E_LEVELS;
    const int64_t len = (int64_t)pq_load_le(p, 0, 4);
    if (4 + len > end) return PQ_E_LEVELS;
    int64_t ones = 0;
    if (!pq_count_defined(p, 4, 4 + len, num_values, &ones)) return PQ_E_LEVELS;
    if (ones != num_values) return PQ_E_NULL;
    *start = 4 + len;
    return PQ_OK;
}

// The index runs of a dictionary-coded page at p[pos .. end): the bit-width byte, then hybrid runs. Walks every run
// header once; every OTTO_PQ_TILE values it records where the run that holds value t * OTTO_PQ_TILE starts:
// mark[2 t] = the byte of its header, mark[2 t + 1] = the index of its first value. n_marks = ceil(num_values / TILE).
OTTO_PQ_HD int pq_walk_runs(const uint8_t* p, int64_t pos, int64_t end, int64_t num_values, int64_t* mark, int* width_out) {
    if (num_values == 0) return PQ_OK;
    if (pos >= end) return PQ_E_RUNS;
    const int width = p[pos++];
    *width_out = width;
    if (width > 32) return PQ_E_WIDTH;
    int64_t seen = 0, next = 0;
    while (seen < num_values) {
        const int64_t at = pos;
        pq_run r;
        if (!pq_run_header(p, &pos, end, width, &r)) return PQ_E_RUNS;
        const int64_t last = seen + (int64_t)r.count;
        if (r.packed) {                                   // the values the page needs from the run must lie inside it
            const int64_t need = (last < num_values ? last : num_values) - seen;
            if (r.data + (need * width + 7) / 8 > end) return PQ_E_RUNS;
        }
        while (next < num_values && next < last) {
            mark[2 * (next / OTTO_PQ_TILE)] = at;
            mark[2 * (next / OTTO_PQ_TILE) + 1] = seen;
            next += OTTO_PQ_TILE;
        }
        seen = last;
    }
    return PQ_OK;
}

// sign or zero extension of a PLAIN value of `size` (4 or 8) bytes to 64 bits; the store truncates
OTTO_PQ_HD int64_t pq_widen(uint64_t raw, int size, bool zero_extend) {
    if (size == 8) return (int64_t)raw;
    return zero_extend ? (int64_t)(uint32_t)raw : (int64_t)(int32_t)(uint32_t)raw;
}
OTTO_PQ_HD void pq_store(void* out, int64_t row, int elem, int64_t v) {
    if (elem == 1) ((uint8_t*)out)[row] = (uint8_t)v;
    else if (elem == 2) ((uint16_t*)out)[row] = (uint16_t)v;
    else if (elem == 4) ((uint32_t*)out)[row] = (uint32_t)v;
    else ((uint64_t*)out)[row] = (uint64_t)v;
}

// ---- DELTA_BINARY_PACKED (SPEC-PARQUET, "Delta pages") ----------------------------------------------------------------------

// ULEB128 of at most 64 bits at p[*pos .. end): PQ_E_DELTA_TRUNC when it is cut short, PQ_E_DELTA_VARINT when it is longer
// than 10 bytes or its tenth byte carries bits above 2^64
OTTO_PQ_HD int pq_varint64(const uint8_t* p, int64_t* pos, int64_t end, uint64_t* out) {
    uint64_t v = 0;
    int64_t i = *pos;
    for (int shift = 0; shift < 70; shift += 7) {
        if (i >= end) return PQ_E_DELTA_TRUNC;
        const uint64_t b = p[i++];
        if (shift == 63 && (b & 0xFEu)) return PQ_E_DELTA_VARINT;
        v |= (b & 0x7Fu) << shift;
        if (!(b & 0x80u)) {
            *pos = i;
            *out = v;
            return PQ_OK;
        }
    }
    return PQ_E_DELTA_VARINT;
}
OTTO_PQ_HD int64_t pq_unzigzag(uint64_t u) { return (int64_t)((u >> 1) ^ (0 - (u & 1))); }

// The header of a delta page: values per block, miniblocks per block, values per miniblock, the value count, the first value
struct pq_delta_head {
    int32_t B, M, mv, pad;
    int64_t n, first, n_blocks;
};

// Walks a delta stream at p[pos .. end) once: the header, then every block header (min_delta, the M width bytes) and the
// extent of every miniblock the page's values need, each checked against `end` before it is used. Block b's record opens at
// blk[stride * b]: the byte of its width bytes, then its min_delta; at most ceil((num_values - 1) / 128) records are
// written, which covers every accepted block shape. phys: 4 or 8, the bytes of the physical type.
OTTO_PQ_HD int pq_delta_walk(const uint8_t* p, int64_t pos, int64_t end, int64_t num_values, int phys, pq_delta_head* h, int64_t* blk,
                             int stride) {
    uint64_t B = 0, M = 0, n = 0, first = 0;
    int st = pq_varint64(p, &pos, end, &B);
    if (st == PQ_OK) st = pq_varint64(p, &pos, end, &M);
    if (st == PQ_OK) st = pq_varint64(p, &pos, end, &n);
    if (st == PQ_OK) st = pq_varint64(p, &pos, end, &first);
    if (st != PQ_OK) return st;
    if (B < 128 || B > 65536 || B % 128 || M < 1 || B % M || (B / M) % 32) return PQ_E_DELTA_SHAPE;
    if (n != (uint64_t)num_values) return PQ_E_DELTA_COUNT;
    const int64_t mv = (int64_t)(B / M), nd = num_values > 0 ? num_values - 1 : 0;
    h->B = (int32_t)B;
    h->M = (int32_t)M;
    h->mv = (int32_t)mv;
    h->pad = 0;
    h->n = num_values;
    h->first = pq_unzigzag(first);
    h->n_blocks = (nd + (int64_t)B - 1) / (int64_t)B;
    for (int64_t b = 0; b < h->n_blocks; ++b) {
        uint64_t md = 0;
        st = pq_varint64(p, &pos, end, &md);
        if (st != PQ_OK) return st;
        if (pos + (int64_t)M > end) return PQ_E_DELTA_TRUNC;
        blk[stride * b] = pos;
        blk[stride * b + 1] = pq_unzigzag(md);
        const int64_t left = nd - b * (int64_t)B, in_block = left < (int64_t)B ? left : (int64_t)B;
        const int64_t need = (in_block + mv - 1) / mv;      // miniblocks behind these have no bytes, their width bytes are not looked at
        const int64_t widths = pos;
        pos += (int64_t)M;
        for (int64_t j = 0; j < need; ++j) {
            const int64_t w = p[widths + j];
            if (w > 8 * phys) return PQ_E_DELTA_WIDTH;
            if (pos + mv / 8 * w > end) return PQ_E_DELTA_TRUNC;
            pos += mv / 8 * w;
        }
    }
    return pos == end ? PQ_OK : PQ_E_DELTA_TRAILING;
}

// field `k` of a miniblock whose bytes start at p[data], width in 0..64. Reads the bytes that hold the field's bits and no
// other: they lie inside the miniblock, which pq_delta_walk has checked against the body's end.
OTTO_PQ_HD uint64_t pq_delta_field(const uint8_t* p, int64_t data, int64_t k, int width) {
    if (width == 0) return 0;
    const int64_t bit = k * width;
    const int64_t b0 = data + (bit >> 3);
    const int sh = (int)(bit & 7);
    const int nb = (sh + width + 7) >> 3;                    // 1 .. 9 bytes
    uint64_t v = 0;
    for (int i = 0; i < nb && i < 8; ++i) v |= (uint64_t)p[b0 + i] << (8 * i);
    v >>= sh;
    if (nb == 9) v |= (uint64_t)p[b0 + 8] << (64 - sh);      // sh >= 1 here
    return width == 64 ? v : v & ((1ull << width) - 1);
}

// Where the 32 values that start at value `u32 * 32` of a block lie: a cursor that moves through the block's miniblocks
// 32 values at a time (a miniblock holds a multiple of 32). j: the miniblock, off: its first byte, k: values of it behind.
struct pq_delta_cursor {
    int64_t off;
    int32_t j, k;
};
OTTO_PQ_HD void pq_delta_advance(const uint8_t* p, int64_t widths, int mv, pq_delta_cursor* c) {
    c->k += 32;
    if (c->k == mv) {
        c->off += (int64_t)(mv / 8) * p[widths + c->j];
        c->j += 1;
        c->k = 0;
    }
}
