// Device-side event ingest for MI355X (gfx950): stable (session, ts) sort of the event frame, CSR session offsets and
// the event-type string map. C-ABI in include/otto_events.h. Reference code this replaces: the
// pandas sort_values(['session', 'ts']) of src/ranker/aid_feature_engineering.py:40, the ms -> s division of :37 and the
// type map of src/utilities/dataset_writer_pickle.py:29-33; host restatement otto_amd/events.py:frame_to_events.
//
// Sort: 8-bit LSD radix sort (radix.h) of (session << 32 | seconds, input index) pairs; the host reads the key bits back
// and skips the digits that are constant over the whole input.
#include "common.h"
#include "radix.h"
#include "sort.h"
#include "../../include/otto_events.h"

namespace otto {

struct SortWs : RadixWs {
    unsigned long long* orand;   // [2]: OR and AND of all keys; [2]: error counter of the type map
};

static size_t ws_layout(int64_t n, char* base, SortWs* w) {
    const size_t o = radix_ws_layout(n, false, base, w);
    if (w) w->orand = (unsigned long long*)(base + o);
    return o + align256((size_t)64);
}

__global__ __launch_bounds__(256) void k_make_keys(const uint32_t* session, const int64_t* ts, int64_t n, int64_t ts_div, uint64_t* key,
                                                   uint32_t* idx, unsigned long long* orand, unsigned long long* bad) {
    unsigned long long vo = 0, va = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t t = ts[i];
        const int64_t sec = t / ts_div;              // truncates: a stamp in (-ts_div, 0) would pass as second 0
        if (t < 0 || sec > 0x7FFFFFFFll) atomicAdd(bad, 1ull);
        const uint64_t k = ((uint64_t)session[i] << 32) | (uint64_t)(uint32_t)sec;
        key[i] = k;
        idx[i] = (uint32_t)i;
        vo |= k;
        va &= k;
    }
    key_bits_fold(vo, va, orand);
}

__global__ __launch_bounds__(256) void k_orand(const uint64_t* key, int64_t n, unsigned long long* orand) {
    unsigned long long vo = 0, va = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint64_t k = key[i];
        vo |= k;
        va &= k;
    }
    key_bits_fold(vo, va, orand);
}

struct HeadFlag {      // 1 where a new session starts in the sorted key stream
    const uint64_t* key;
    __device__ uint64_t operator()(int64_t i) const { return (i == 0 || (key[i] >> 32) != (key[i - 1] >> 32)) ? 1ull : 0ull; }
};

__global__ void k_emit_sorted(const uint64_t* key, const uint32_t* idx, int64_t n, const uint32_t* aid, const uint8_t* type,
                              const uint64_t* head_pos, uint32_t* out_aid, int32_t* out_ts, uint8_t* out_type, uint32_t* out_order,
                              int64_t* sess_off, uint32_t* sess_id) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = key[i];
        const uint32_t src = idx[i];
        out_aid[i] = aid[src];
        out_type[i] = type[src];
        out_ts[i] = (int32_t)(uint32_t)k;
        if (out_order) out_order[i] = src;
        if (i == 0 || (k >> 32) != (key[i - 1] >> 32)) {
            const uint64_t p = head_pos[i];
            sess_off[p] = i;
            sess_id[p] = (uint32_t)(k >> 32);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) sess_off[head_pos[n]] = n;
}

template <typename OFF>
__global__ void k_type_strings(const OFF* off, const uint8_t* bytes, int64_t n, uint8_t* out, unsigned long long* bad) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = (int64_t)off[i], len = (int64_t)off[i + 1] - o;
        uint8_t t = 255;
        if (len >= 2) {
            const uint8_t c0 = bytes[o], c1 = bytes[o + 1];
            if (c0 == 'c' && c1 == 'l' && len == 6) t = 0;          // clicks
            else if (c0 == 'c' && c1 == 'a' && len == 5) t = 1;     // carts
            else if (c0 == 'o' && c1 == 'r' && len == 6) t = 2;     // orders
        }
        if (t == 255) atomicAdd(bad, 1ull);
        out[i] = t;
    }
}

}  // namespace otto

using namespace otto;

// sort.h: shared with the aid-pair and feature builders
int otto_sort_pairs_in_ws(uint64_t* d_keys, int64_t n, void* d_ws, uint64_t** d_keys_sorted, uint32_t** d_vals_sorted, hipStream_t s) {
    SortWs w;
    ws_layout(n, (char*)d_ws, &w);
    OTTO_REQUIRE(d_keys == w.key[0], "keys must have been written into the workspace's first key buffer");
    unsigned long long init[2] = {0ull, ~0ull};
    OTTO_HIP(hipMemcpyAsync(w.orand, init, sizeof init, hipMemcpyHostToDevice, s));
    const int grid = (int)((n + 255) / 256 < 256 * 16 ? (n + 255) / 256 : 256 * 16);
    k_orand<<<grid, 256, 0, s>>>(w.key[0], n, w.orand);
    OTTO_HIP(hipGetLastError());
    unsigned long long h[2];
    OTTO_HIP(hipMemcpyAsync(h, w.orand, sizeof h, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    int cur = 0;
    OTTO_TRY(radix_passes<false>(w, n, h[0] ^ h[1], SkipOnHost{}, &cur, s));
    *d_keys_sorted = w.key[cur];
    *d_vals_sorted = w.val[cur];
    return 0;
}
void otto_sort_ws_buffers(int64_t n, void* d_ws, uint64_t** key0, uint32_t** val0, uint64_t** scan_out, uint64_t** scan_partial) {
    SortWs w;
    ws_layout(n, (char*)d_ws, &w);
    *key0 = w.key[0]; *val0 = w.val[0]; *scan_out = w.offs; *scan_partial = w.partial;
}

extern "C" int64_t otto_events_sort_workspace(int64_t n) {
    if (n <= 0) return 256;
    return (int64_t)ws_layout(n, nullptr, nullptr);
}

extern "C" int otto_events_sort(const uint32_t* d_session, const int64_t* d_ts, const uint32_t* d_aid, const uint8_t* d_type, int64_t n,
                                int64_t ts_div, uint32_t* d_out_aid, int32_t* d_out_ts, uint8_t* d_out_type, uint32_t* d_out_order,
                                int64_t* d_sess_off, uint32_t* d_sess_id, int64_t* h_n_sessions, void* d_ws, int64_t ws_bytes,
                                void* stream) {
    OTTO_REQUIRE(h_n_sessions && d_sess_off, "otto_events_sort: null argument");
    OTTO_REQUIRE(n >= 0 && n < (1ll << 32), "n must be in [0, 2^32)");
    OTTO_REQUIRE(ts_div >= 1, "ts_div must be >= 1");
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        *h_n_sessions = 0;
        OTTO_HIP(hipMemsetAsync(d_sess_off, 0, 8, s));
        return 0;
    }
    OTTO_REQUIRE(d_session && d_ts && d_aid && d_type && d_out_aid && d_out_ts && d_out_type && d_sess_id && d_ws, "otto_events_sort: null argument");
    OTTO_REQUIRE(ws_bytes >= otto_events_sort_workspace(n), "workspace too small (%lld < %lld)", (long long)ws_bytes,
                 (long long)otto_events_sort_workspace(n));
    SortWs w;
    ws_layout(n, (char*)d_ws, &w);
    unsigned long long init[4] = {0ull, ~0ull, 0ull, 0ull};
    OTTO_HIP(hipMemcpyAsync(w.orand, init, sizeof init, hipMemcpyHostToDevice, s));
    const int grid = (int)((n + 255) / 256 < 256 * 16 ? (n + 255) / 256 : 256 * 16);
    k_make_keys<<<grid, 256, 0, s>>>(d_session, d_ts, n, ts_div, w.key[0], w.val[0], w.orand, w.orand + 2);
    OTTO_HIP(hipGetLastError());
    unsigned long long h[4];
    OTTO_HIP(hipMemcpyAsync(h, w.orand, sizeof h, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    OTTO_REQUIRE(h[2] == 0, "%llu timestamps are negative or beyond 2^31 - 1 seconds after dividing by %lld", h[2], (long long)ts_div);
    const uint64_t varying = h[0] ^ h[1];                       // bits that differ somewhere in the input
    int cur = 0;
    OTTO_TRY(radix_passes<false>(w, n, varying, SkipOnHost{}, &cur, s));
    OTTO_TRY(device_scan(HeadFlag{w.key[cur]}, n, w.offs, w.partial, s));
    k_emit_sorted<<<grid, 256, 0, s>>>(w.key[cur], w.val[cur], n, d_aid, d_type, w.offs, d_out_aid, d_out_ts, d_out_type, d_out_order,
                                       d_sess_off, d_sess_id);
    OTTO_HIP(hipGetLastError());
    uint64_t ns = 0;
    OTTO_HIP(hipMemcpyAsync(&ns, w.offs + n, 8, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    *h_n_sessions = (int64_t)ns;
    return 0;
}

extern "C" int otto_events_type_from_strings(const void* d_offsets, int32_t offsets_are_64, const uint8_t* d_bytes, int64_t n,
                                             uint8_t* d_out_type, void* stream) {
    OTTO_REQUIRE(n >= 0, "n < 0");
    if (n == 0) return 0;
    OTTO_REQUIRE(d_offsets && d_bytes && d_out_type, "otto_events_type_from_strings: null argument");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* bad = nullptr;
    OTTO_TRY(device_scratch(SCRATCH_EVENTS, 8, (void**)&bad, s));
    OTTO_HIP(hipMemsetAsync(bad, 0, 8, s));
    const int grid = (int)((n + 255) / 256 < 256 * 16 ? (n + 255) / 256 : 256 * 16);
    if (offsets_are_64) k_type_strings<int64_t><<<grid, 256, 0, s>>>((const int64_t*)d_offsets, d_bytes, n, d_out_type, bad);
    else k_type_strings<int32_t><<<grid, 256, 0, s>>>((const int32_t*)d_offsets, d_bytes, n, d_out_type, bad);
    unsigned long long hb = 0;
    hipError_t e = hipMemcpyAsync(&hb, bad, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    OTTO_HIP(e);
    OTTO_REQUIRE(hb == 0, "%llu event type strings are none of clicks / carts / orders", hb);
    return 0;
}
