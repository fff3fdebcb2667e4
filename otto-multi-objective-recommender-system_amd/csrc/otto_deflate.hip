// Device-side DEFLATE for MI355X (gfx950): a device buffer of bytes -> concatenated gzip members, one per block of at most
// 64 KiB. C-ABI and SPEC-DEFLATE in include/otto_deflate.h. Reference code this replaces: the zlib
// call behind to_csv(..., compression='gzip') of src/ranker/inference.py, src/covisitation/inference.py and
// src/recbole/inference.py. Host restatement: tests/deflate_restatement.py.
//
// One wave owns a block in both kernels, so nothing but wave_lds_sync orders the LDS traffic.
//   k_deflate_plan  CRC-32 (a contiguous piece per lane, joined by x^(8 len) products); the match finder in batches of 64
//                   positions (hash table of 4,096 positions and both histograms in LDS), the greedy selection on ballot
//                   masks, the tokens to the workspace in whole words; code lengths (rank sort, two-queue Huffman by lane
//                   0), the run-length coded header as bits, the dynamic-or-stored choice, the member's size
//   device_scan     (scan.h) -> the byte offset of every member, the total last
//   k_deflate_emit  canonical codes into LDS; every piece of the member (gzip header, Huffman header, tokens, stored
//                   bytes, trailer) goes through one bit appender: a field of up to 64 bits per lane, placed by a wave
//                   prefix sum of the field widths, OR-ed into an LDS image of the next output words, flushed in whole
//                   32-bit words. A word inside the member is stored plain, a word shared with a neighbour is OR-ed.
#include "common.h"
#include "deflate.h"
#include "scan.h"
#include "wave.h"
#include "../../include/otto_deflate.h"

namespace otto {

constexpr int DF_BLOCK_MAX = OTTO_DEFLATE_BLOCK_MAX;
constexpr int DF_MIN_MATCH = OTTO_DEFLATE_MIN_MATCH;
constexpr int DF_HASH_BYTES = OTTO_DEFLATE_HASH_BYTES;
constexpr int DF_HASH_BITS = OTTO_DEFLATE_HASH_BITS;
constexpr int DF_MAX_MATCH = 258, DF_MAX_DIST = 32768;
constexpr int DF_LL = 286, DF_D = 30, DF_CL = 19;
constexpr int DF_SYMS = 320;                                 // literal/length symbols at 0, distance symbols at DF_DOFF
constexpr int DF_DOFF = 288;
constexpr int DF_HDR_WORDS = 160;                            // 17 + 19 * 3 + 316 * 14 bits at the most = 4,498
constexpr int DF_REC_BYTES = 1024;                           // per block: DfMeta, the code lengths, the header bits
static_assert(OTTO_DEFLATE_BATCH == WAVE, "a batch of the match finder is one position per lane");
static_assert(DF_MIN_MATCH >= 3 && DF_HASH_BYTES <= 8, "RFC 1951; the hash reads one 64-bit value");

enum { DF_EMPTY = 0, DF_DYNAMIC = 1, DF_STORED = 2 };
constexpr unsigned long long DF_NO_ERR = ~0ull;

struct DfMeta {
    uint32_t form, crc, ntok, hdr_bits;
    uint32_t size;                                           // bytes of the member
    uint32_t bits;                                           // of the dynamic stream
    uint32_t pad[2];
};
static_assert(sizeof(DfMeta) + DF_SYMS + DF_HDR_WORDS * 4 <= DF_REC_BYTES, "the record of a block");

struct DfWs {
    unsigned long long* err;
    uint64_t* off;                // [blocks + 1] exclusive scan of size, the total last
    uint32_t* size;               // [blocks]
    uint64_t* partial;
    uint8_t* rec;                 // [blocks] records of DF_REC_BYTES
    uint32_t* tok;                // [blocks * block_bytes]
};

static int64_t df_blocks(int64_t n, int32_t bb) { return n == 0 ? 1 : (n + bb - 1) / bb; }

static size_t df_layout(int64_t n, int32_t bb, char* base, DfWs* w) {
    const int64_t nb = df_blocks(n, bb);
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    DfWs t;
    t.err = (unsigned long long*)take(8);
    t.off = (uint64_t*)take((size_t)(nb + 1) * 8);
    t.size = (uint32_t*)take((size_t)nb * 4);
    t.partial = (uint64_t*)take(scan_partial_bytes(nb));
    t.rec = (uint8_t*)take((size_t)nb * DF_REC_BYTES);
    t.tok = (uint32_t*)take((size_t)nb * (size_t)bb * 4);
    if (w) *w = t;
    return o;
}

struct LoadSize {
    const uint32_t* a;
    __device__ uint64_t operator()(int64_t i) const { return a[i]; }
};

// a token: a literal byte, or bit 31 | (distance - 1) << 9 | length
__device__ __forceinline__ uint32_t df_match_token(uint32_t length, uint32_t dist) { return 0x80000000u | (dist - 1u) << 9 | length; }

// number of leading bytes x[a ...] and x[b ...] share, at most limit
// 8 bytes of x at any address, little-endian (gfx950 serves an unaligned global load)
__device__ __forceinline__ uint64_t df_load8(const uint8_t* __restrict__ x) {
    uint64_t v;
    __builtin_memcpy(&v, x, 8);
    return v;
}

__device__ __forceinline__ uint32_t df_common(const uint8_t* __restrict__ x, uint32_t a, uint32_t b, uint32_t limit) {
    uint32_t i = 0;
    for (; i + 8u <= limit; i += 8u) {                       // a < b and b + limit is inside the block
        const uint64_t d = df_load8(x + a + i) ^ df_load8(x + b + i);
        if (d) return i + ((uint32_t)__builtin_ctzll(d) >> 3);
    }
    while (i < limit && x[a + i] == x[b + i]) ++i;
    return i;
}

// ---- Huffman code lengths (SPEC-DEFLATE) --------------------------------------------------------------------------------
struct DfHuffLds {
    uint32_t c[DF_LL];            // the counts, halved while the limit is exceeded
    uint32_t node_w[DF_LL];
    uint16_t order[DF_LL], leaf_parent[DF_LL], node_parent[DF_LL], depth[DF_LL];
};

// cnt[0, n) -> len[0, n), by one wave
__device__ void df_huff_lengths(const uint32_t* cnt, int n, int limit, uint8_t* len, DfHuffLds& h) {
    const int lane = (int)lane_id();
    int used = 0, only = 0;
    for (int s = lane; s < n; s += WAVE) {
        h.c[s] = cnt[s];
        len[s] = 0;
        if (cnt[s]) ++used, only = s;
    }
    const int m = wave_reduce<Sum>(used);
    wave_lds_sync();
    if (m == 0) return;
    if (m == 1) {
        if (used) len[only] = 1;
        wave_lds_sync();
        return;
    }
#pragma unroll 1
    for (int round = 0; round < 32; ++round) {               // 17 halvings make every count 1: depth <= 9
        for (int s = lane; s < n; s += WAVE) {
            const uint32_t cs = h.c[s];
            if (!cs) continue;
            const uint32_t key = cs << 9 | (uint32_t)s;
            int rank = 0;
            for (int t = 0; t < n; ++t) {
                const uint32_t ct = h.c[t];
                rank += ct != 0 && (ct << 9 | (uint32_t)t) < key;
            }
            h.order[rank] = (uint16_t)s;
        }
        wave_lds_sync();
        if (lane == 0) {
            int li = 0, ni = 0;
            for (int j = 0; j < m - 1; ++j) {
                uint32_t w = 0;
                for (int r = 0; r < 2; ++r) {
                    const uint32_t lw = li < m ? h.c[h.order[li]] : 0u;
                    if (li < m && (ni >= j || lw <= h.node_w[ni])) {
                        w += lw;
                        h.leaf_parent[li++] = (uint16_t)j;
                    } else {
                        w += h.node_w[ni];
                        h.node_parent[ni++] = (uint16_t)j;
                    }
                }
                h.node_w[j] = w;
            }
            h.depth[m - 2] = 0;
            for (int j = m - 3; j >= 0; --j) h.depth[j] = (uint16_t)(h.depth[h.node_parent[j]] + 1);
        }
        wave_lds_sync();
        int deepest = 0;
        for (int i = lane; i < m; i += WAVE) {
            const int d = h.depth[h.leaf_parent[i]] + 1;
            len[h.order[i]] = (uint8_t)d;
            deepest = d > deepest ? d : deepest;
        }
        deepest = wave_reduce<Max>(deepest);
        wave_lds_sync();
        if (deepest <= limit) return;
        for (int s = lane; s < n; s += WAVE) h.c[s] = (h.c[s] + 1u) >> 1;
        wave_lds_sync();
    }
}

// canonical codes (RFC 1951 section 3.2.2) of len[0, n), bit-reversed for the LSB-first stream; next[] is scratch of 16
__device__ void df_canonical(const uint8_t* len, int n, uint16_t* rev, uint32_t* next) {
    const int lane = (int)lane_id();
    if (lane < 16) next[lane] = 0;
    wave_lds_sync();
    for (int s = lane; s < n; s += WAVE)
        if (len[s]) atomicAdd(&next[len[s] & 15], 1u);
    wave_lds_sync();
    if (lane == 0) {
        uint32_t code = 0, before = 0;
        for (int b = 1; b < 16; ++b) {
            code = (code + before) << 1;
            before = next[b];
            next[b] = code;
        }
    }
    wave_lds_sync();
    for (int s = lane; s < n; s += WAVE) {
        const uint32_t l = len[s] & 15u;
        uint32_t r = 0;
        if (l) {
            uint32_t code = next[l];
            for (int t = 0; t < s; ++t) code += len[t] == l;
            r = __brev(code) >> (32u - l);
        }
        rev[s] = (uint16_t)r;
    }
    wave_lds_sync();
}

__device__ __constant__ uint8_t DF_CLEN_ORDER[DF_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct DfPlanLds {
    uint32_t table[1 << DF_HASH_BITS];                       // position + 1, 0 = empty
    uint32_t cnt[DF_SYMS];
    uint8_t len[DF_SYMS];
    DfHuffLds huff;
    uint32_t cl_cnt[DF_CL + 1];
    uint8_t cl_len[DF_CL + 1];
    uint16_t cl_rev[DF_CL + 1];
    uint32_t next[16];
    uint16_t rl[DF_LL + DF_D];                               // symbol | extra value << 5
    uint32_t hdr[DF_HDR_WORDS];
    uint32_t n_rl, hdr_bits;
};

__global__ __launch_bounds__(WAVE) void k_deflate_plan(const uint8_t* __restrict__ in, int64_t n, int bb, uint32_t* __restrict__ tok_all,
                                                       uint8_t* __restrict__ rec_all, uint32_t* __restrict__ size_out) {
    __shared__ DfPlanLds L;
    const int lane = (int)lane_id();
    const int64_t blk = blockIdx.x;
    const int64_t b0 = blk * bb;
    const uint32_t m = (uint32_t)(n - b0 < bb ? n - b0 : bb);          // bytes of this block
    const uint8_t* __restrict__ x = in + b0;
    uint32_t* __restrict__ tok = tok_all + blk * bb;
    uint8_t* rec = rec_all + blk * DF_REC_BYTES;
    DfMeta* meta = reinterpret_cast<DfMeta*>(rec);
    if (m == 0) {                                            // only n == 0
        if (lane == 0) {
            DfMeta e = {DF_EMPTY, 0u, 0u, 0u, 20u, 0u, {0u, 0u}};
            *meta = e;
            size_out[blk] = 20u;
        }
        return;
    }
    for (int i = lane; i < (1 << DF_HASH_BITS); i += WAVE) L.table[i] = 0;
    for (int i = lane; i < DF_SYMS; i += WAVE) L.cnt[i] = 0, L.len[i] = 0;        // the four lengths no alphabet owns go to the record too
    for (int i = lane; i < DF_HDR_WORDS; i += WAVE) L.hdr[i] = 0;
    wave_lds_sync();

    // CRC-32: lane l takes bytes [l * piece, (l + 1) * piece)
    uint32_t crc;
    {
        const uint32_t piece = (m + WAVE - 1) / WAVE;
        const uint32_t lo = (uint32_t)lane * piece < m ? (uint32_t)lane * piece : m;
        const uint32_t hi = lo + piece < m ? lo + piece : m;
        uint32_t c = 0xFFFFFFFFu;
        uint32_t i = lo;
        for (; i + 8u <= hi; i += 8u) {
            const uint64_t v = df_load8(x + i);
#pragma unroll
            for (int j = 0; j < 8; ++j) c = df_crc_byte(c, (uint32_t)(v >> (8 * j)) & 0xFFu);
        }
        for (; i < hi; ++i) c = df_crc_byte(c, x[i]);
        c = hi > lo ? df_crc_shift(~c, m - hi) : 0u;
        crc = c;                                             // the pieces join by xor
        for (int o = 32; o > 0; o >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, o, 64);
    }

    // the match finder and the greedy selection
    uint32_t frontier = 0, ntok = 0;
#pragma unroll 1
    for (uint32_t base = 0; base < m; base += WAVE) {
        const uint32_t p = base + (uint32_t)lane;
        const bool valid = p < m, hashable = p + DF_HASH_BYTES <= m;
        uint32_t first = 0, slot = 0, seen = 0;
        if (hashable) {
            uint64_t v = 0;
            if (p + 8u <= m) {
                v = df_load8(x + p) & (~0ull >> (64 - 8 * DF_HASH_BYTES));
            } else {
#pragma unroll
                for (int i = 0; i < DF_HASH_BYTES; ++i) v |= (uint64_t)x[p + i] << (8 * i);
            }
            first = (uint32_t)(v & 0xFFu);
            slot = (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> (64 - DF_HASH_BITS));
            seen = L.table[slot];
        } else if (valid) {
            first = x[p];
        }
        wave_lds_sync();
        if (hashable) atomicMax(&L.table[slot], p + 1u);
        wave_lds_sync();
        uint32_t mlen = 0, dist = 0;
        if (valid && p >= frontier) {
            const uint32_t limit = m - p < DF_MAX_MATCH ? m - p : DF_MAX_MATCH;
            if (p >= 1u) mlen = df_common(x, p - 1u, p, limit), dist = 1u;
            if (seen && p - (seen - 1u) <= DF_MAX_DIST) {
                const uint32_t l2 = df_common(x, seen - 1u, p, limit);
                if (l2 > mlen) mlen = l2, dist = p - (seen - 1u);
            }
            if (mlen < DF_MIN_MATCH) mlen = 0;
        }
        const uint64_t matches = __ballot(mlen > 0);
        const uint32_t nvalid = m - base < WAVE ? m - base : WAVE;
        uint32_t cur = frontier > base ? frontier - base : 0u;
        uint64_t reach = 0;                                  // the lanes a token starts at
        while (cur < nvalid) {
            const uint64_t from = ~0ull << cur;
            const uint64_t rest = matches & from;
            const uint32_t stop = rest ? (uint32_t)__builtin_ctzll(rest) : nvalid;      // literals in [cur, stop)
            const uint64_t below = stop >= 64u ? ~0ull : (1ull << stop) - 1ull;
            reach |= from & below;
            if (!rest) { cur = nvalid; break; }
            reach |= 1ull << stop;
            cur = stop + (uint32_t)__shfl((int)mlen, (int)stop, 64);
        }
        if (base + cur > frontier) frontier = base + cur;
        if ((reach >> lane) & 1ull) {
            const uint32_t at = ntok + (uint32_t)__popcll(reach & ((1ull << lane) - 1ull));
            if (mlen) {
                uint32_t s, e, v;
                df_len_symbol(mlen, &s, &e, &v);
                atomicAdd(&L.cnt[s], 1u);
                df_dist_symbol(dist, &s, &e, &v);
                atomicAdd(&L.cnt[DF_DOFF + s], 1u);
                tok[at] = df_match_token(mlen, dist);
            } else {
                atomicAdd(&L.cnt[first], 1u);
                tok[at] = first;
            }
        }
        ntok += (uint32_t)__popcll(reach);
    }
    if (lane == 0) L.cnt[256] = 1;
    wave_lds_sync();

    df_huff_lengths(L.cnt, DF_LL, 15, L.len, L.huff);
    df_huff_lengths(L.cnt + DF_DOFF, DF_D, 15, L.len + DF_DOFF, L.huff);

    // HLIT, HDIST
    int hl = 0, hd = 0;
    for (int s = lane; s < DF_LL; s += WAVE)
        if (L.len[s]) hl = s + 1;
    if (lane < DF_D && L.len[DF_DOFF + lane]) hd = lane + 1;
    const int hlit = max(wave_reduce<Max>(hl), 257), hdist = max(wave_reduce<Max>(hd), 1);

    // run-length tokens of the joint sequence, by lane 0
    if (lane < DF_CL + 1) L.cl_cnt[lane] = 0;
    wave_lds_sync();
    if (lane == 0) {
        const int total = hlit + hdist;
        auto seq = [&](int i) -> uint32_t { return i < hlit ? L.len[i] : L.len[DF_DOFF + i - hlit]; };
        int i = 0, k = 0;
        while (i < total) {
            const uint32_t v = seq(i);
            int r = 1;
            while (i + r < total && seq(i + r) == v) ++r;
            uint32_t sym, val;
            int t;
            if (v == 0 && r >= 11) t = r < 138 ? r : 138, sym = 18, val = (uint32_t)t - 11u;
            else if (v == 0 && r >= 3) t = r, sym = 17, val = (uint32_t)t - 3u;         // r <= 10 here
            else if (v != 0 && i > 0 && seq(i - 1) == v && r >= 3) t = r < 6 ? r : 6, sym = 16, val = (uint32_t)t - 3u;
            else t = 1, sym = v, val = 0;
            L.rl[k++] = (uint16_t)(sym | val << 5);
            L.cl_cnt[sym] += 1;
            i += t;
        }
        L.n_rl = (uint32_t)k;
    }
    wave_lds_sync();
    df_huff_lengths(L.cl_cnt, DF_CL, 7, L.cl_len, L.huff);
    df_canonical(L.cl_len, DF_CL, L.cl_rev, L.next);

    // the header as bits, by lane 0
    if (lane == 0) {
        uint64_t acc = 0;
        uint32_t fill = 0, words = 0, bits = 0;
        auto put = [&](uint32_t value, uint32_t width) {
            acc |= (uint64_t)value << fill;
            fill += width;
            bits += width;
            if (fill >= 32u) {
                L.hdr[words++] = (uint32_t)acc;
                acc >>= 32;
                fill -= 32u;
            }
        };
        int hclen = 4;
        for (int i = 0; i < DF_CL; ++i)
            if (L.cl_len[DF_CLEN_ORDER[i]] && i + 1 > hclen) hclen = i + 1;
        put(1u, 1), put(2u, 2), put((uint32_t)hlit - 257u, 5), put((uint32_t)hdist - 1u, 5), put((uint32_t)hclen - 4u, 4);
        for (int i = 0; i < hclen; ++i) put(L.cl_len[DF_CLEN_ORDER[i]], 3);
        const uint32_t n_rl = L.n_rl;
        for (uint32_t k = 0; k < n_rl; ++k) {
            const uint32_t sym = L.rl[k] & 31u, val = L.rl[k] >> 5;
            put(L.cl_rev[sym], L.cl_len[sym]);
            if (sym >= 16u) put(val, sym == 16u ? 2u : sym == 17u ? 3u : 7u);
        }
        if (fill) L.hdr[words] = (uint32_t)acc;
        L.hdr_bits = bits;
    }
    wave_lds_sync();

    // bits of the dynamic form
    uint32_t bits = 0;
    for (int s = lane; s < DF_LL; s += WAVE) bits += L.cnt[s] * (L.len[s] + df_len_extra((uint32_t)s));
    if (lane < DF_D) bits += L.cnt[DF_DOFF + lane] * (L.len[DF_DOFF + lane] + df_dist_extra((uint32_t)lane));
    bits = wave_reduce<Sum>(bits) + L.hdr_bits;
    const uint32_t dynamic_bytes = (bits + 7u) >> 3, stored_bytes = m + (m > 65535u ? 10u : 5u);
    const bool dynamic = dynamic_bytes < stored_bytes;
    const uint32_t size = 10u + (dynamic ? dynamic_bytes : stored_bytes) + 8u;
    if (lane == 0) {
        DfMeta e = {dynamic ? (uint32_t)DF_DYNAMIC : (uint32_t)DF_STORED, crc, ntok, L.hdr_bits, size, bits, {(uint32_t)hlit, (uint32_t)hdist}};
        *meta = e;
        size_out[blk] = size;
    }
    uint32_t* rec_len = reinterpret_cast<uint32_t*>(rec + sizeof(DfMeta));               // 320 bytes as 80 words
    for (int i = lane; i < DF_SYMS / 4; i += WAVE) rec_len[i] = reinterpret_cast<const uint32_t*>(L.len)[i];
    uint32_t* rec_hdr = reinterpret_cast<uint32_t*>(rec + sizeof(DfMeta) + DF_SYMS);
    for (int i = lane; i < DF_HDR_WORDS; i += WAVE) rec_hdr[i] = L.hdr[i];
}

// ---- emit ---------------------------------------------------------------------------------------------------------------
constexpr int DF_STAGE_WORDS = 132;                          // 31 bits carried + 64 fields of 64 bits, and a spare word

struct DfEmitLds {
    uint32_t stage[DF_STAGE_WORDS];
    uint8_t len[DF_SYMS];
    uint16_t ll_rev[DF_DOFF], d_rev[32];
    uint32_t next[16];
};

// The bit appender of one wave. stage[i] is output word word0 + i; `fill` bits of it are taken.
struct DfAppender {
    uint32_t* stage;
    uint32_t* out32;
    uint64_t word0;
    uint32_t fill;
    uint64_t lo, hi;                                         // the member's bytes [lo, hi)

    __device__ __forceinline__ void store(uint64_t w, uint32_t v) {
        const uint64_t b = w * 4u;
        if (b >= lo && b + 4u <= hi) out32[w] = v;
        else if (b + 4u > lo && b < hi) atomicOr(&out32[w], v);     // the bits outside the member are 0
    }
    // every lane appends `width` (<= 64) bits of `value` (no bit set at or above width), lane 0 first
    __device__ __forceinline__ void append(uint64_t value, uint32_t width) {
        const int lane = (int)lane_id();
        width = width > 64u ? 64u : width;
        const uint32_t incl = wave_incl_scan<uint32_t>(width);
        const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
        if (width) {
            const uint32_t pos = fill + incl - width, w = pos >> 5, s = pos & 31u;
            const uint64_t a = value << s;
            const uint32_t c = s ? (uint32_t)(value >> (64u - s)) : 0u;
            if ((uint32_t)a) atomicOr(&stage[w], (uint32_t)a);
            if ((uint32_t)(a >> 32)) atomicOr(&stage[w + 1], (uint32_t)(a >> 32));
            if (c) atomicOr(&stage[w + 2], c);
        }
        fill += total;
        wave_lds_sync();
        const uint32_t full = fill >> 5;                     // whole words: at most (31 + 64 * 64) >> 5 = 128
        uint32_t v0 = 0, v1 = 0;
        if ((uint32_t)lane < full) v0 = stage[lane];
        if ((uint32_t)lane + 64u < full) v1 = stage[lane + 64];
        const uint32_t carry = stage[full];
        wave_lds_sync();
        if ((uint32_t)lane < full) store(word0 + lane, v0);
        if ((uint32_t)lane + 64u < full) store(word0 + 64u + lane, v1);
        for (uint32_t i = lane; i <= full; i += WAVE) stage[i] = i == 0 ? carry : 0u;
        word0 += full;
        fill &= 31u;
        wave_lds_sync();
    }
    __device__ __forceinline__ void finish() {
        if (fill && lane_id() == 0) store(word0, stage[0]);
    }
};

__global__ __launch_bounds__(WAVE) void k_deflate_emit(const uint8_t* __restrict__ in, int64_t n, int bb, const uint32_t* __restrict__ tok_all,
                                                       const uint8_t* __restrict__ rec_all, const uint64_t* __restrict__ off, int64_t blocks,
                                                       uint8_t* out, uint64_t total, unsigned long long* err) {
    __shared__ DfEmitLds L;
    const int lane = (int)lane_id();
    const int64_t blk = blockIdx.x;
    const int64_t b0 = blk * bb;
    const uint32_t m = (uint32_t)(n - b0 < bb ? n - b0 : bb);
    const uint8_t* __restrict__ x = in + b0;
    const uint32_t* __restrict__ tok = tok_all + blk * bb;
    const uint8_t* rec = rec_all + blk * DF_REC_BYTES;
    const DfMeta meta = *reinterpret_cast<const DfMeta*>(rec);
    const uint64_t o_lo = off[blk], o_hi = off[blk + 1];
    // Every store lands in [o_lo, o_hi); the refusal (uniform over the wave) keeps that inside [0, total), whatever the
    // workspace holds. The sizes a form can have bound the appender's work as well.
    const uint32_t stored_bytes = m + (m > 65535u ? 10u : 5u);
    bool ok = off[blocks] == total && o_lo <= o_hi && o_hi <= total && o_hi - o_lo == meta.size && meta.ntok <= m;
    if (meta.form == DF_EMPTY) ok = ok && m == 0 && meta.size == 20u;
    else if (meta.form == DF_STORED) ok = ok && m > 0 && meta.size == 18u + stored_bytes;
    else ok = ok && meta.form == DF_DYNAMIC && m > 0 && meta.hdr_bits <= DF_HDR_WORDS * 32u && meta.hdr_bits <= meta.bits &&
              meta.size == 18u + ((meta.bits + 7u) >> 3) && meta.size < 18u + stored_bytes;
    if (!ok) {
        if (lane == 0) atomicMin(err, (unsigned long long)blk);
        return;
    }
    for (int i = lane; i < DF_STAGE_WORDS; i += WAVE) L.stage[i] = 0;
    wave_lds_sync();
    DfAppender ap = {L.stage, reinterpret_cast<uint32_t*>(out), o_lo >> 2, (uint32_t)(o_lo & 3u) * 8u, o_lo, o_hi};
    ap.append(lane == 0 ? 0x0000000000088B1Full : 0xFF00ull, lane == 0 ? 64u : lane == 1 ? 16u : 0u);
    if (meta.form == DF_EMPTY) {
        ap.append(0x0003ull, lane == 0 ? 16u : 0u);
    } else if (meta.form == DF_STORED) {
        for (uint32_t lo = 0; lo < m; lo += 65535u) {
            const uint32_t piece = m - lo < 65535u ? m - lo : 65535u;
            const uint64_t field = lane == 0 ? (lo + piece == m ? 1u : 0u) : lane == 1 ? piece : (~piece & 0xFFFFu);
            ap.append(lane < 3 ? field : 0ull, lane == 0 ? 8u : lane < 3 ? 16u : 0u);
            for (uint32_t q = 0; q < piece; q += WAVE * 8u) {
                const uint32_t at = q + (uint32_t)lane * 8u;
                const uint32_t have = at < piece ? (piece - at < 8u ? piece - at : 8u) : 0u;
                uint64_t v = 0;
                for (uint32_t i = 0; i < have; ++i) v |= (uint64_t)x[lo + at + i] << (8u * i);
                ap.append(v, have * 8u);
            }
        }
    } else {
        const uint32_t* rec_len = reinterpret_cast<const uint32_t*>(rec + sizeof(DfMeta));
        for (int i = lane; i < DF_SYMS / 4; i += WAVE) reinterpret_cast<uint32_t*>(L.len)[i] = rec_len[i] & 0x0F0F0F0Fu;
        wave_lds_sync();
        df_canonical(L.len, DF_LL, L.ll_rev, L.next);
        df_canonical(L.len + DF_DOFF, DF_D, L.d_rev, L.next);
        const uint32_t* rec_hdr = reinterpret_cast<const uint32_t*>(rec + sizeof(DfMeta) + DF_SYMS);
        for (uint32_t base = 0; base < meta.hdr_bits; base += WAVE * 32u) {
            const uint32_t at = base + (uint32_t)lane * 32u;
            const uint32_t width = at < meta.hdr_bits ? (meta.hdr_bits - at < 32u ? meta.hdr_bits - at : 32u) : 0u;
            uint32_t v = width ? rec_hdr[at >> 5] : 0u;
            if (width < 32u) v &= (1u << width) - 1u;
            ap.append(v, width);
        }
        // the tokens and, as the last item, end-of-block
        for (uint32_t base = 0; base <= meta.ntok; base += WAVE) {
            const uint32_t t = base + (uint32_t)lane;
            uint64_t v = 0;
            uint32_t width = 0;
            if (t < meta.ntok) {
                const uint32_t k = tok[t];
                if (k >> 31) {
                    uint32_t length = k & 511u, dist = ((k >> 9) & 32767u) + 1u, s, e, ev;
                    length = length < 3u ? 3u : length > 258u ? 258u : length;
                    df_len_symbol(length, &s, &e, &ev);
                    v = L.ll_rev[s], width = L.len[s];
                    v |= (uint64_t)ev << width, width += e;
                    df_dist_symbol(dist, &s, &e, &ev);
                    v |= (uint64_t)L.d_rev[s] << width, width += L.len[DF_DOFF + s];
                    v |= (uint64_t)ev << width, width += e;
                } else {
                    v = L.ll_rev[k & 255u], width = L.len[k & 255u];
                }
            } else if (t == meta.ntok) {
                v = L.ll_rev[256], width = L.len[256];
            }
            ap.append(v, width);
        }
    }
    // zero bits up to the next byte, then CRC-32 and ISIZE
    const uint32_t pad = (32u - ap.fill) & 7u;
    ap.append(lane == 1 ? meta.crc : lane == 2 ? m : 0u, lane == 0 ? pad : lane < 3 ? 32u : 0u);
    ap.finish();
    // a plan and an input that do not belong together end somewhere else than the member does
    if (lane == 0 && (ap.word0 * 4u + (ap.fill >> 3)) != o_hi) atomicMin(err, (unsigned long long)blk);
}

static int df_check_args(const char* what, const uint8_t* d_in, int64_t n, int32_t bb, const void* d_work, int64_t work_bytes) {
    OTTO_REQUIRE(bb >= 1 && bb <= DF_BLOCK_MAX, "%s: block_bytes must be in [1, %d] (got %d)", what, DF_BLOCK_MAX, bb);
    OTTO_REQUIRE(n >= 0, "%s: negative n", what);
    OTTO_REQUIRE(df_blocks(n, bb) < (1ll << 31), "%s: more than 2^31 - 1 blocks", what);
    OTTO_REQUIRE((n == 0 || d_in) && d_work, "%s: null argument", what);
    OTTO_REQUIRE(work_bytes >= otto_deflate_workspace(n, bb), "%s: workspace too small (%lld < %lld)", what, (long long)work_bytes,
                 (long long)otto_deflate_workspace(n, bb));
    return 0;
}

}  // namespace otto

using namespace otto;

extern "C" int64_t otto_deflate_bound(int64_t n, int32_t block_bytes) {
    if (n < 0 || block_bytes < 1 || block_bytes > DF_BLOCK_MAX) return -1;
    return n + df_blocks(n, block_bytes) * (18 + (block_bytes > 65535 ? 10 : 5));
}

extern "C" int64_t otto_deflate_workspace(int64_t n, int32_t block_bytes) {
    if (n < 0 || block_bytes < 1 || block_bytes > DF_BLOCK_MAX) return -1;
    return (int64_t)df_layout(n, block_bytes, nullptr, nullptr);
}

extern "C" int otto_deflate_plan(const uint8_t* d_in, int64_t n, int32_t block_bytes, int64_t* h_total, void* d_work, int64_t work_bytes,
                                 void* stream) {
    OTTO_REQUIRE(h_total, "otto_deflate_plan: null h_total");
    *h_total = 0;
    OTTO_TRY(df_check_args("otto_deflate_plan", d_in, n, block_bytes, d_work, work_bytes));
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = df_blocks(n, block_bytes);
    DfWs w;
    df_layout(n, block_bytes, (char*)d_work, &w);
    k_deflate_plan<<<(unsigned)blocks, WAVE, 0, s>>>(d_in, n, block_bytes, w.tok, w.rec, w.size);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(LoadSize{w.size}, blocks, w.off, w.partial, s));
    uint64_t total = 0;
    OTTO_HIP(hipMemcpyAsync(&total, w.off + blocks, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    *h_total = (int64_t)total;
    return 0;
}

extern "C" int otto_deflate_emit(const uint8_t* d_in, int64_t n, int32_t block_bytes, uint8_t* d_out, int64_t out_bytes, void* d_work,
                                 int64_t work_bytes, void* stream) {
    OTTO_TRY(df_check_args("otto_deflate_emit", d_in, n, block_bytes, d_work, work_bytes));
    OTTO_REQUIRE(out_bytes >= 0 && d_out, "otto_deflate_emit: null d_out or negative out_bytes");
    OTTO_REQUIRE(((uintptr_t)d_out & 15) == 0, "otto_deflate_emit: d_out must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = df_blocks(n, block_bytes);
    DfWs w;
    df_layout(n, block_bytes, (char*)d_work, &w);
    uint64_t total = 0;
    OTTO_HIP(hipMemcpyAsync(&total, w.off + blocks, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    OTTO_REQUIRE(total >= 20u * (uint64_t)blocks && total <= (uint64_t)otto_deflate_bound(n, block_bytes),
                 "otto_deflate_emit: the workspace does not hold the plan otto_deflate_plan wrote for this input");
    OTTO_REQUIRE(total <= (uint64_t)out_bytes, "otto_deflate_emit: %llu bytes of members do not fit out_bytes %lld; nothing written",
                 (unsigned long long)total, (long long)out_bytes);
    OTTO_HIP(hipMemsetAsync(w.err, 0xFF, 8, s));
    OTTO_HIP(hipMemsetAsync(d_out, 0, (size_t)total, s));
    k_deflate_emit<<<(unsigned)blocks, WAVE, 0, s>>>(d_in, n, block_bytes, w.tok, w.rec, w.off, blocks, d_out, total, w.err);
    OTTO_HIP(hipGetLastError());
    unsigned long long herr = 0;
    OTTO_HIP(hipMemcpyAsync(&herr, w.err, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    OTTO_REQUIRE(herr == DF_NO_ERR, "otto_deflate_emit: block %llu: the workspace does not hold the plan otto_deflate_plan wrote for this input",
                 herr);
    return 0;
}
