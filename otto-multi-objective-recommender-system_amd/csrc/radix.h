// Stable 8-bit LSD radix sort of (key u64, value u32 [, byte u8]) rows, for the translation units that run it
// (otto_events.hip: events, aid pairs, feature ranks; otto_blend.hip: the join's rows with their model column).
//
// One pass = block histograms of 4096-key tiles (k_rs_hist) -> exclusive scan over (digit, block) -> scatter with STABLE
// in-block ranks (k_rs_scatter): a wave finds the lanes that hold its digit with 8 ballots (no LDS traffic), a per-wave
// running count per digit (LDS, plain read-modify-write by the first lane of each digit group) orders the wave's 16
// chunks, and the waves of a block are ordered by a 256-thread prefix over the per-wave counts.
//
// A digit that is constant over the whole input makes its pass the identity. Who finds that out is the caller's choice:
//   SkipOnHost    the host has read the key bits back (key_bits_fold, below) and launches the varying digits only;
//   SkipOnDevice  the kernels read the key bits themselves: the histogram returns at once and the scatter copies. Every
//                 pass is launched and the host needs no read-back before the passes.
#pragma once
#include "common.h"
#include "scan.h"
#include "wave.h"

namespace otto {

constexpr int RS_THREADS = 256;
constexpr int RS_ITEMS = 16;
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;      // 4096 keys per block and pass
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_SUB = 4;                            // tiles a workgroup takes one after the other (one counter row per workgroup)
constexpr int64_t RS_SPAN = (int64_t)RS_TILE * RS_SUB;
inline int64_t rs_blocks(int64_t n) { return (n + RS_SPAN - 1) / RS_SPAN; }

// ---------------------------------------------------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------------------------------------------------
struct RadixWs {         // carved from the caller's workspace
    uint64_t* key[2];
    uint32_t* val[2];
    uint8_t* byt[2];     // null without the byte column
    uint32_t* counts;    // [256 * nb]
    uint64_t* offs;      // [max(256 * nb, n) + 1]: scan of the counts; the callers' own scans over the n rows go here too
    uint64_t* partial;   // scan scratch
};

// Lays the buffers of a sort of n rows out from `base` (null: sizes only) in 256-byte aligned pieces; returns the bytes taken.
inline size_t radix_ws_layout(int64_t n, bool byte_column, char* base, RadixWs* w) {
    const int64_t nb = rs_blocks(n);
    const size_t scan_n = (size_t)(256 * nb > n ? 256 * nb : n) + 1;
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    RadixWs t;
    for (int i = 0; i < 2; ++i) t.key[i] = (uint64_t*)take((size_t)n * 8);
    for (int i = 0; i < 2; ++i) t.val[i] = (uint32_t*)take((size_t)n * 4);
    for (int i = 0; i < 2; ++i) t.byt[i] = byte_column ? (uint8_t*)take((size_t)n) : nullptr;
    t.counts = (uint32_t*)take((size_t)256 * nb * 4);
    t.offs = (uint64_t*)take(scan_n * 8);
    t.partial = (uint64_t*)take(scan_partial_bytes((int64_t)scan_n));
    if (w) *w = t;
    return o;
}

// ---------------------------------------------------------------------------------------------------------------------
// key bits: which digits vary at all
// ---------------------------------------------------------------------------------------------------------------------
// Folds every thread's (OR, AND) of its keys through the wave and the 256-thread workgroup into bits[0] (OR of all keys;
// starts at 0) and bits[1] (AND of all keys; starts at ~0). Bit b differs somewhere in the input iff set in bits[0] ^ bits[1].
__device__ __forceinline__ void key_bits_fold(unsigned long long vo, unsigned long long va, unsigned long long* bits) {
    __shared__ unsigned long long s_or[4], s_and[4];
    vo = wave_reduce<Or>(vo);
    va = wave_reduce<And>(va);
    if (lane_id() == 0) { s_or[threadIdx.x >> 6] = vo; s_and[threadIdx.x >> 6] = va; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicOr(&bits[0], s_or[0] | s_or[1] | s_or[2] | s_or[3]);
        atomicAnd(&bits[1], s_and[0] & s_and[1] & s_and[2] & s_and[3]);
    }
}

struct SkipOnHost {
    __device__ bool varies(int) const { return true; }          // a constant digit is never launched
};
struct SkipOnDevice {
    const unsigned long long* bits;                              // the two words of key_bits_fold
    __device__ bool varies(int shift) const { return (((bits[0] ^ bits[1]) >> shift) & 255ull) != 0; }
};

// ---------------------------------------------------------------------------------------------------------------------
// one pass
// ---------------------------------------------------------------------------------------------------------------------
template <class SKIP>
__global__ __launch_bounds__(RS_THREADS) void k_rs_hist(const uint64_t* key, int64_t n, int shift, int64_t nb, uint32_t* counts, SKIP skip) {
    __shared__ uint32_t s_h[256];
    if (!skip.varies(shift)) return;                 // the scatter of this pass copies; the counts are not read
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RS_SPAN;
    for (int sub = 0; sub < RS_SUB; ++sub) {
#pragma unroll
        for (int c = 0; c < RS_ITEMS; ++c) {
            const int64_t i = base + (int64_t)sub * RS_TILE + (int64_t)c * RS_THREADS + threadIdx.x;
            if (i < n) atomicAdd(&s_h[(key[i] >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    counts[(int64_t)threadIdx.x * nb + blockIdx.x] = s_h[threadIdx.x];
}

struct CountAt {
    const uint32_t* c;
    __device__ uint64_t operator()(int64_t i) const { return c[i]; }
};

// Scatter of one pass. Ranks: stable in-wave rank of a key among the wave's keys of the same digit (8 ballots), per-wave digit
// counters in LDS. The tile is then REORDERED IN LDS by digit and written out in that order: consecutive lanes hold
// consecutive positions of a digit run, so a wave-instruction touches a handful of cache lines instead of up to 64 (the
// direct form -- every lane storing its key at base[digit] + rank -- ran at ~1.5 TB/s of traffic).
// BYTE: the rows carry the byte column byt too; without it the column's registers and LDS staging do not exist.
template <bool BYTE, class SKIP>
__global__ __launch_bounds__(RS_THREADS) void k_rs_scatter(const uint64_t* key, const uint32_t* val, const uint8_t* byt, int64_t n, int shift,
                                                           int64_t nb, const uint64_t* offs, uint64_t* key_out, uint32_t* val_out,
                                                           uint8_t* byt_out, SKIP skip) {
    __shared__ uint16_t s_wcnt[RS_WAVES][256];      // per wave: keys of digit d, then the wave's first position of d in the tile (< 4096)
    __shared__ uint32_t s_scan[RS_THREADS / 64 + 1];
    __shared__ long long s_delta[256];              // global position of digit d's run minus its position in the tile
    __shared__ uint64_t s_k[RS_TILE];
    __shared__ uint32_t s_v[RS_TILE];
    __shared__ uint8_t s_b[BYTE ? RS_TILE : 1];
    if (!skip.varies(shift)) {                       // constant digit: the pass is the identity
        const int64_t base = (int64_t)blockIdx.x * RS_SPAN;
        for (int64_t i = base + threadIdx.x; i < base + RS_SPAN && i < n; i += RS_THREADS) {
            key_out[i] = key[i];
            val_out[i] = val[i];
            if constexpr (BYTE) byt_out[i] = byt[i];
        }
        return;
    }
    const int w = threadIdx.x >> 6;
    const unsigned lane = lane_id();
    unsigned long long gbase = offs[(int64_t)threadIdx.x * nb + blockIdx.x];     // thread d: where the workgroup's next key of digit d goes
    for (int sub = 0; sub < RS_SUB; ++sub) {
        const int64_t tile_base = (int64_t)blockIdx.x * RS_SPAN + (int64_t)sub * RS_TILE;
        if (tile_base >= n) break;
        for (int q = 0; q < RS_WAVES; ++q) s_wcnt[q][threadIdx.x] = 0;
        __syncthreads();
        const int64_t wave_base = tile_base + (int64_t)w * (RS_TILE / RS_WAVES);
        uint64_t k[RS_ITEMS];
        uint32_t v[RS_ITEMS], lr[RS_ITEMS];
        uint8_t b[BYTE ? RS_ITEMS : 1];
        const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
        for (int c = 0; c < RS_ITEMS; ++c) {
            const int64_t i = wave_base + (int64_t)c * 64 + lane;
            const bool valid = i < n;
            k[c] = valid ? key[i] : ~0ull;
            v[c] = valid ? val[i] : 0u;
            if constexpr (BYTE) b[c] = valid ? byt[i] : (uint8_t)0;
        }
#pragma unroll
        for (int c = 0; c < RS_ITEMS; ++c) {
            const bool valid = wave_base + (int64_t)c * 64 + lane < n;
            const uint32_t dig = (uint32_t)(k[c] >> shift) & 255u;
            uint64_t m = __ballot(valid);
#pragma unroll
            for (int bit_i = 0; bit_i < 8; ++bit_i) {
                const bool bit = (dig >> bit_i) & 1u;
                const uint64_t bb = __ballot(bit);
                m &= bit ? bb : ~bb;
            }
            const int leader = valid ? __ffsll((unsigned long long)m) - 1 : (int)lane;
            uint32_t prev = 0;
            if (valid && (int)lane == leader) {
                prev = s_wcnt[w][dig];
                s_wcnt[w][dig] = (uint16_t)(prev + (uint32_t)__popcll(m));
            }
            prev = (uint32_t)__shfl((int)prev, leader, 64);
            lr[c] = prev + (uint32_t)__popcll(m & lt);
            wave_lds_sync();                         // the next chunk's leaders read what this chunk's wrote
        }
        __syncthreads();
        {
            // digit threadIdx.x: position of its run in the tile (exclusive scan over the digits), every wave's share of it
            uint32_t tot = 0, cnt[RS_WAVES];
#pragma unroll
            for (int q = 0; q < RS_WAVES; ++q) { cnt[q] = s_wcnt[q][threadIdx.x]; tot += cnt[q]; }
            uint32_t all;
            uint32_t run = block_excl_scan<uint32_t, RS_THREADS>(tot, s_scan, &all);
            s_delta[threadIdx.x] = (long long)gbase - (long long)run;
            gbase += tot;
#pragma unroll
            for (int q = 0; q < RS_WAVES; ++q) { s_wcnt[q][threadIdx.x] = (uint16_t)run; run += cnt[q]; }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < RS_ITEMS; ++c) {
            if (wave_base + (int64_t)c * 64 + lane < n) {
                const uint32_t p = s_wcnt[w][(uint32_t)(k[c] >> shift) & 255u] + lr[c];      // < RS_TILE
                s_k[p] = k[c];
                s_v[p] = v[c];
                if constexpr (BYTE) s_b[p] = b[c];
            }
        }
        __syncthreads();
        const int64_t left = n - tile_base;
        const uint32_t tile_n = left < (int64_t)RS_TILE ? (uint32_t)left : (uint32_t)RS_TILE;
#pragma unroll
        for (int c = 0; c < RS_ITEMS; ++c) {
            const uint32_t p = (uint32_t)c * RS_THREADS + threadIdx.x;
            if (p < tile_n) {
                const uint64_t kk = s_k[p];
                const long long g = s_delta[(uint32_t)(kk >> shift) & 255u] + (long long)p;  // in [0, n): offs is the scan of the counts
                key_out[g] = kk;
                val_out[g] = s_v[p];
                if constexpr (BYTE) byt_out[g] = s_b[p];
            }
        }
        __syncthreads();                             // the next tile reuses the staging arrays
    }
}

// The LSD passes over the rows in buffers *cur_io of w; on return *cur_io names the buffers that hold the sorted rows.
// `launch`: a digit with no bit set in it is skipped without a launch. SkipOnHost callers pass the bits that vary
// (OR ^ AND of the keys). SkipOnDevice callers pass ~0: all eight passes are launched, an even number, so the sorted rows
// end in the buffers they started in.
template <bool BYTE, class SKIP>
int radix_passes(const RadixWs& w, int64_t n, uint64_t launch, SKIP skip, int* cur_io, hipStream_t s) {
    const int64_t nb = rs_blocks(n);
    int cur = *cur_io;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 8 * pass;
        if (((launch >> shift) & 255ull) == 0) continue;        // constant digit: the pass would be the identity
        k_rs_hist<SKIP><<<(unsigned)nb, RS_THREADS, 0, s>>>(w.key[cur], n, shift, nb, w.counts, skip);
        OTTO_HIP(hipGetLastError());
        OTTO_TRY(device_scan(CountAt{w.counts}, 256 * nb, w.offs, w.partial, s));
        k_rs_scatter<BYTE, SKIP><<<(unsigned)nb, RS_THREADS, 0, s>>>(w.key[cur], w.val[cur], w.byt[cur], n, shift, nb, w.offs,
                                                                    w.key[cur ^ 1], w.val[cur ^ 1], w.byt[cur ^ 1], skip);
        OTTO_HIP(hipGetLastError());
        cur ^= 1;
    }
    *cur_io = cur;
    return 0;
}

}  // namespace otto
