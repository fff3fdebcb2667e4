// GRU4Rec session model for MI355X (gfx950): epoch plan, recurrent encoder, back-propagation through time, Adam. C-ABI and
// SPEC-GRU4REC in include/otto_gru.h.
//
//   k_plan_check   offsets and aids, the smallest offending index of each kind by integer atomicMin.
//   k_plan_keys    one thread per event: its session by binary search, key = hash(seed, epoch, p) >> 1 for a sample, bit 63
//                  for an event that is none (it sorts behind every sample); value = p. The stable radix sort of radix.h
//                  orders them, so equal keys stay in the order of p.
//   k_plan_emit    one thread per sample: sequence bounds, target, negative.
//   k_gru_len_keys / one radix pass / a scan   the batch in descending length (stable, so the order is a function of the
//                  batch alone), the first step row of every sequence.
//   k_gru_transpose  W_ih, W_hh, W_d transposed into the workspace: in the forward products a thread's hidden unit is the
//                  fastest index of what it reads.
//   k_gru_tile     one workgroup of 2H threads per OTTO_GRU_TILE sequences; thread (j, half) owns hidden unit j of eight
//                  sequences. Forward: x_t and h_t of the tile in LDS ([k][sequence], so a thread's eight operands are two
//                  16-byte reads that all lanes of a half share), weights from L2. TRAIN: the step's h, r, z, n, W_hn h
//                  go to the step row of the stash, then the dense layer, the loss, and the walk back with dh in registers;
//                  the pre-activation gradients replace r, z, n, W_hn h in the stash.
//   k_gru_atb      C = A^T B over the step rows (or the batch rows), 32 x 32 outputs per workgroup, OTTO_GRU_CHUNK rows per
//                  workgroup; k_gru_atb_sum adds the chunks' partials in chunk order.
//   k_gru_dx       the input gradient of every step row: gi W_ih.
//   k_co_*         the item gradient: one key per contribution (step rows, targets, negatives), sorted by row id; a head
//                  flag, its scan, and one thread per (listed row, column) that adds the run in contribution order.
//   k_gru_final    loss sum and the bias gradient, in a fixed two-level order.
//   k_gru_adam / k_gru_adam_rows   SPEC UPDATE.
// No float atomic anywhere; no kernel waits for another workgroup.
#include "common.h"
#include "radix.h"
#include "../../include/otto_gru.h"

#include <math.h>
#include <string.h>

namespace otto {
namespace {

constexpr int GT = 256;
constexpr int TS = OTTO_GRU_TILE;                                // sequences of a tile
constexpr int NS = 8;                                            // sequences of one thread
constexpr int64_t CHUNK = OTTO_GRU_CHUNK;
static_assert(TS == 2 * NS, "a tile is two halves of NS sequences");

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + GT - 1) / GT); }
inline unsigned capped_blocks(int64_t n) { const int64_t b = (n + GT - 1) / GT; return (unsigned)(b < 1 ? 1 : b > 8192 ? 8192 : b); }

__device__ __forceinline__ uint64_t order_key(uint64_t seed, uint64_t epoch, uint64_t p) {
    return mix64(mix64(seed ^ (epoch * 0xD1342543DE82EF95ull)) ^ (p * 0xA0761D6478BD642Full)) >> 1;
}

// ---------------------------------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------------------------------
struct PlanCtrl {                                                // the first 256 bytes of the plan's workspace
    unsigned long long err_off, err_aid;                         // smallest offending index, ~0 without one
    unsigned long long key_bits[2];                              // key_bits_fold
    unsigned long long n;                                        // samples
};

__global__ __launch_bounds__(GT) void k_plan_check(const int32_t* __restrict__ aid, const int64_t* __restrict__ off, int64_t E, int64_t S,
                                                   int64_t n_aids, PlanCtrl* ctrl) {
    const int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (i <= S) {
        const int64_t o = off[i];
        if ((i == 0 && o != 0) || (i < S && o > off[i + 1]) || (i == S && o != E)) atomicMin(&ctrl->err_off, (unsigned long long)i);
    }
    if (i < E) {
        const int32_t a = aid[i];
        if (a < 0 || a >= n_aids) atomicMin(&ctrl->err_aid, (unsigned long long)i);
    }
}

__global__ __launch_bounds__(GT) void k_plan_keys(const int64_t* __restrict__ off, int64_t E, int64_t S, uint64_t seed, uint64_t epoch,
                                                  uint64_t* key, uint32_t* val, PlanCtrl* ctrl) {
    const int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x;
    unsigned long long vo = 0, va = ~0ull;
    bool sample = false;
    if (i < E) {
        sample = i > off[segment_of(off, S, i)];
        const uint64_t k = sample ? order_key(seed, epoch, (uint64_t)i) : 1ull << 63;
        key[i] = k;
        val[i] = (uint32_t)i;
        vo = va = k;
    }
    const unsigned long long m = __ballot(sample);
    if (lane_id() == 0 && m) atomicAdd(&ctrl->n, (unsigned long long)__popcll(m));
    key_bits_fold(vo, va, ctrl->key_bits);
}

__global__ __launch_bounds__(GT) void k_plan_emit(const uint32_t* __restrict__ val, int64_t N, const int32_t* __restrict__ aid,
                                                  const int64_t* __restrict__ off, int64_t E, int64_t S, int64_t n_aids, int L, uint64_t seed,
                                                  uint64_t epoch, int32_t* p_out, int32_t* lo_out, int32_t* len_out, int32_t* tgt_out,
                                                  int32_t* neg_out) {
    const int64_t q = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (q >= N) return;
    const int64_t p = val[q];
    if (p >= E) return;                                          // never: the values are event indices
    const int64_t lo = off[segment_of(off, S, p)];
    int64_t len = p - lo;
    len = len > L ? L : len < 0 ? 0 : len;
    const int32_t t = aid[p];
    p_out[q] = (int32_t)p;
    lo_out[q] = (int32_t)(p - len);
    len_out[q] = (int32_t)len;
    tgt_out[q] = t;
    neg_out[q] = (int32_t)bpr_negative(seed, epoch, (uint64_t)p, t, n_aids);
}

struct PlanWs {
    PlanCtrl* ctrl;
    RadixWs r;
};

size_t plan_layout(int64_t E, char* base, PlanWs* w) {
    PlanWs t;
    t.ctrl = (PlanCtrl*)base;
    const size_t o = align256(sizeof(PlanCtrl));
    const size_t total = o + radix_ws_layout(E, false, base ? base + o : nullptr, &t.r);
    if (w) *w = t;
    return total;
}

int plan_check(const otto_gru_plan_job* j) {
    OTTO_REQUIRE(j, "otto_gru_plan: null job");
    OTTO_REQUIRE(j->n_events >= 0 && j->n_events < (1ll << 31) - 1, "otto_gru_plan: n_events must be in [0, 2^31 - 1) (got %lld)", (long long)j->n_events);
    OTTO_REQUIRE(j->n_sessions >= 0 && j->n_sessions < (1ll << 31) - 1, "otto_gru_plan: n_sessions must be in [0, 2^31 - 1) (got %lld)", (long long)j->n_sessions);
    OTTO_REQUIRE(j->n_aids >= 1 && j->n_aids < (1ll << 31) - 1, "otto_gru_plan: n_aids must be in [1, 2^31 - 1) (got %lld)", (long long)j->n_aids);
    OTTO_REQUIRE(j->max_len >= 1 && j->max_len <= OTTO_GRU_MAX_LEN, "otto_gru_plan: max_len must be in [1, %d] (got %d)", OTTO_GRU_MAX_LEN, j->max_len);
    OTTO_REQUIRE(j->reserved == 0, "otto_gru_plan: reserved must be 0");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// encode / grad
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t row_of(int32_t a, int64_t n_aids) { return (uint32_t)a < (uint64_t)n_aids ? (int64_t)a + 1 : 0; }
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// the length a sequence is run with: 0 unless it lies inside the events and within L
__device__ __forceinline__ int run_len(int32_t lo, int32_t len, int64_t E, int L) {
    return (len < 0 || len > L || lo < 0 || (int64_t)lo + len > E) ? 0 : len;
}

__global__ __launch_bounds__(GT) void k_gru_len_keys(const int32_t* __restrict__ lo, const int32_t* __restrict__ len, int64_t B, int64_t E, int L,
                                                     uint64_t* key, uint32_t* val) {
    const int64_t b = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (b >= B) return;
    key[b] = (uint64_t)(L - run_len(lo[b], len[b], E, L));       // ascending key = descending length
    val[b] = (uint32_t)b;
}

struct LenAt {
    const uint64_t* key;
    int L;
    __device__ uint64_t operator()(int64_t i) const { return (uint64_t)L - key[i]; }
};

__global__ __launch_bounds__(GT) void k_gru_transpose(const float* __restrict__ W_ih, const float* __restrict__ W_hh, const float* __restrict__ W_d,
                                                      int De, int H, float* wt_ih, float* wt_hh, float* wt_d) {
    const int i = blockIdx.x * GT + threadIdx.x;
    const int n_ih = 3 * H * De, n_hh = 3 * H * H, n_d = De * H;
    if (i < n_ih) {
        const int m = i / De, k = i % De;
        wt_ih[k * 3 * H + m] = W_ih[i];
    } else if (i < n_ih + n_hh) {
        const int q = i - n_ih, m = q / H, k = q % H;
        wt_hh[k * 3 * H + m] = W_hh[q];
    } else if (i < n_ih + n_hh + n_d) {
        const int q = i - n_ih - n_hh, e = q / H, k = q % H;
        wt_d[k * De + e] = W_d[q];
    }
}

struct TileArgs {
    const float* E;
    const float* wt_ih;          // [De, 3H]
    const float* wt_hh;          // [H, 3H]
    const float* wt_d;           // [H, De]
    const float* W_hh;           // [3H, H]
    const float* W_d;            // [De, H]
    const float* b_d;
    int64_t n_aids;
    const int32_t* aid;
    const int32_t* seq_lo;
    const int32_t* target;
    const int32_t* neg;
    int64_t B;
    int L;
    const uint64_t* lkey;        // [B] L - length, sorted
    const uint32_t* order;       // [B] batch index of every sorted position
    const uint64_t* step_off;    // [B + 1] first step row of every sorted position (TRAIN)
    float* o;                    // [B, De] by batch index, or null
    float* stash;                // [rows, 5H]: h, r, z, n, W_hn h  ->  h, da_r, da_z, da_n, da_hn
    int32_t* xrow;               // [rows] item row of the step's input; -row - 1 at a sequence's first step
    float* hT;                   // [B, H] by sorted position
    float* dO;                   // [B, De]
    float* cO;                   // [B, De] c * o: what the target's row receives, and minus what the negative's does
    float* lossv;                // [B]
    float inv_b;
};

// acc[i] += sum over k of W[k * ldw + col] * in[k * TS + s0 + i]
template <int K>
__device__ __forceinline__ void tile_mac(float (&acc)[NS], const float* __restrict__ W, int ldw, int col, const float* in, int s0) {
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const float w = W[k * ldw + col];
        const float4 a = *reinterpret_cast<const float4*>(in + k * TS + s0);
        const float4 b = *reinterpret_cast<const float4*>(in + k * TS + s0 + 4);
        acc[0] += w * a.x; acc[1] += w * a.y; acc[2] += w * a.z; acc[3] += w * a.w;
        acc[4] += w * b.x; acc[5] += w * b.y; acc[6] += w * b.z; acc[7] += w * b.w;
    }
}

template <int De, int H, bool TRAIN>
__global__ __launch_bounds__(2 * H) void k_gru_tile(TileArgs a) {
    constexpr int T = 2 * H;
    constexpr int XG = De > 3 * H ? De : 3 * H;
    __shared__ __attribute__((aligned(16))) float xs[De * TS];               // x_t, later dO
    __shared__ __attribute__((aligned(16))) float hs[H * TS];                // h_t
    __shared__ __attribute__((aligned(16))) float gs[(TRAIN ? XG : De) * TS];  // o, later the step's gh
    __shared__ int s_len[TS], s_lo[TS], s_orig[TS];
    __shared__ long long s_row0[TS], s_prow[TS], s_nrow[TS];
    __shared__ float s_c[TS];
    const int tid = threadIdx.x, j = tid % H, s0 = (tid / H) * NS;
    const int64_t pos0 = (int64_t)blockIdx.x * TS;
    if (tid < TS) {
        const int64_t pos = pos0 + tid;
        const bool valid = pos < a.B;
        const int64_t orig = valid ? (int64_t)a.order[pos] : -1;
        const bool ok = valid && orig < a.B;
        int len = ok ? a.L - (int)a.lkey[pos] : 0;
        len = len < 0 ? 0 : len > a.L ? a.L : len;
        s_len[tid] = len;
        s_orig[tid] = ok ? (int)orig : -1;
        s_lo[tid] = ok ? a.seq_lo[orig] : 0;
        if constexpr (TRAIN) {
            s_row0[tid] = ok ? (long long)a.step_off[pos] : 0;
            s_prow[tid] = ok ? row_of(a.target[orig], a.n_aids) : 0;
            s_nrow[tid] = ok ? row_of(a.neg[orig], a.n_aids) : 0;
        }
    }
    for (int i = tid; i < H * TS; i += T) hs[i] = 0.0f;
    __syncthreads();
    int maxlen = 0;
#pragma unroll
    for (int s = 0; s < TS; ++s) maxlen = s_len[s] > maxlen ? s_len[s] : maxlen;

    // ---- forward
    for (int t = 0; t < maxlen; ++t) {
        for (int i = tid; i < De * TS; i += T) {
            const int s = i / De, e = i % De;
            float x = 0.0f;
            if (s_len[s] > t) x = a.E[row_of(a.aid[s_lo[s] + t], a.n_aids) * De + e];
            xs[e * TS + s] = x;
        }
        if constexpr (TRAIN) {
            if (tid < TS && s_len[tid] > t) {
                const int32_t row = (int32_t)row_of(a.aid[s_lo[tid] + t], a.n_aids);
                a.xrow[s_row0[tid] + t] = t == 0 ? -row - 1 : row;
            }
        }
        __syncthreads();
        float r[NS] = {}, z[NS] = {}, ni[NS] = {}, nh[NS] = {};
        tile_mac<De>(r, a.wt_ih, 3 * H, j, xs, s0);
        tile_mac<De>(z, a.wt_ih, 3 * H, H + j, xs, s0);
        tile_mac<De>(ni, a.wt_ih, 3 * H, 2 * H + j, xs, s0);
        tile_mac<H>(r, a.wt_hh, 3 * H, j, hs, s0);
        tile_mac<H>(z, a.wt_hh, 3 * H, H + j, hs, s0);
        tile_mac<H>(nh, a.wt_hh, 3 * H, 2 * H + j, hs, s0);
        __syncthreads();                                         // every read of h_t-1 is done
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int s = s0 + i;
            if (s_len[s] > t) {
                const float rr = sigmoidf(r[i]), zz = sigmoidf(z[i]);
                const float nn = tanhf(ni[i] + rr * nh[i]);
                const float hn = (1.0f - zz) * nn + zz * hs[j * TS + s];
                hs[j * TS + s] = hn;
                if constexpr (TRAIN) {
                    float* st = a.stash + (s_row0[s] + t) * (5 * H);
                    st[j] = hn; st[H + j] = rr; st[2 * H + j] = zz; st[3 * H + j] = nn; st[4 * H + j] = nh[i];
                }
            }
        }
    }
    __syncthreads();

    // ---- dense layer: o = W_d h_T + b_d
    for (int c = tid; c < De * 2; c += T) {
        const int e = c % De, q0 = (c / De) * NS;
        float acc[NS] = {};
        tile_mac<H>(acc, a.wt_d, De, e, hs, q0);
        const float bias = a.b_d[e];
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const float v = acc[i] + bias;
            if constexpr (TRAIN) gs[e * TS + q0 + i] = v;
            if (a.o && s_orig[q0 + i] >= 0) a.o[(int64_t)s_orig[q0 + i] * De + e] = v;
        }
    }
    if constexpr (!TRAIN) return;

    // ---- loss: x = <o, E[target]> - <o, E[negative]>, c = d loss / d x / B
    if constexpr (TRAIN) {
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (pos0 + s0 + i < a.B) a.hT[(pos0 + s0 + i) * H + j] = hs[j * TS + s0 + i];
        __syncthreads();
        if (tid < TS) {
            float c = 0.0f;
            if (s_orig[tid] >= 0) {
                const float* ep = a.E + s_prow[tid] * De;
                const float* en = a.E + s_nrow[tid] * De;
                float x = 0.0f;
                for (int e = 0; e < De; ++e) x += gs[e * TS + tid] * (ep[e] - en[e]);
                const float sg = sigmoidf(x);
                a.lossv[pos0 + tid] = -logf(1e-10f + sg);
                c = -(sg * (1.0f - sg)) / (1e-10f + sg) * a.inv_b;
            }
            s_c[tid] = c;
        }
        __syncthreads();
        for (int i = tid; i < De * TS; i += T) {
            const int s = i / De, e = i % De;
            float d = 0.0f;
            if (s_orig[s] >= 0) {
                d = s_c[s] * (a.E[s_prow[s] * De + e] - a.E[s_nrow[s] * De + e]);
                a.dO[(pos0 + s) * De + e] = d;
                a.cO[(pos0 + s) * De + e] = s_c[s] * gs[e * TS + s];
            }
            xs[e * TS + s] = d;
        }
        __syncthreads();
        float dh[NS] = {};
        tile_mac<De>(dh, a.W_d, H, j, xs, s0);                   // dh_T = W_d^T dO
        __syncthreads();

        // ---- back through time
        for (int t = maxlen - 1; t >= 0; --t) {
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                const int s = s0 + i;
                float dar = 0.0f, daz = 0.0f, dahn = 0.0f;
                if (s_len[s] > t) {
                    float* st = a.stash + (s_row0[s] + t) * (5 * H);
                    const float hp = t > 0 ? st[j - 5 * H] : 0.0f;
                    const float rr = st[H + j], zz = st[2 * H + j], nn = st[3 * H + j], hn = st[4 * H + j];
                    const float dn = dh[i] * (1.0f - zz), dz = dh[i] * (hp - nn);
                    const float dan = dn * (1.0f - nn * nn);
                    daz = dz * zz * (1.0f - zz);
                    dar = dan * hn * rr * (1.0f - rr);
                    dahn = dan * rr;
                    dh[i] = dh[i] * zz;
                    st[H + j] = dar; st[2 * H + j] = daz; st[3 * H + j] = dan; st[4 * H + j] = dahn;
                }
                gs[j * TS + s] = dar; gs[(H + j) * TS + s] = daz; gs[(2 * H + j) * TS + s] = dahn;
            }
            __syncthreads();
            tile_mac<3 * H>(dh, a.W_hh, H, j, gs, s0);           // dh_t-1 += W_hh^T gh; a finished sequence adds zeros
            __syncthreads();
        }
    }
}

// C[m, n] = sum over the rows r of A(r, m) * B(r, n)
enum { ATB_IH = 0, ATB_HH = 1, ATB_D = 2 };
struct AtbArgs {
    int mode;
    const float* stash;
    const int32_t* xrow;
    const float* E;
    const float* dO;
    const float* hT;
    const uint64_t* rows_dev;    // the number of rows, on the device (null: rows_host)
    int64_t rows_host;
    int Md, Nd, De, H;
    float* partial;              // [chunks, Md, Nd]
};

__device__ __forceinline__ int64_t atb_rows(const AtbArgs& a) { return a.rows_dev ? (int64_t)*a.rows_dev : a.rows_host; }

__global__ __launch_bounds__(GT) void k_gru_atb(AtbArgs a) {
    __shared__ float As[32][33], Bs[32][33];
    const int64_t R = atb_rows(a), r_beg = (int64_t)blockIdx.y * CHUNK;
    if (r_beg >= R) return;
    const int64_t r_end = r_beg + CHUNK < R ? r_beg + CHUNK : R;
    const int nt = a.Nd / 32, m0 = ((int)blockIdx.x / nt) * 32, n0 = ((int)blockIdx.x % nt) * 32;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, H5 = 5 * a.H;
    float acc[2][2] = {};
    for (int64_t r0 = r_beg; r0 < r_end; r0 += 32) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int idx = tid + GT * q, rr = idx >> 5, cc = idx & 31;
            const int64_t r = r0 + rr;
            float av = 0.0f, bv = 0.0f;
            if (r < r_end) {
                const int m = m0 + cc, n = n0 + cc;
                if (a.mode == ATB_IH) {
                    const int32_t xr = a.xrow[r];
                    av = a.stash[r * H5 + a.H + m];
                    bv = a.E[(int64_t)(xr < 0 ? -xr - 1 : xr) * a.De + n];
                } else if (a.mode == ATB_HH) {
                    av = a.stash[r * H5 + a.H + m + (m >= 2 * a.H ? a.H : 0)];
                    bv = a.xrow[r] < 0 ? 0.0f : a.stash[(r - 1) * H5 + n];      // a first step has h_0 = 0 in front of it
                } else {
                    av = a.dO[r * a.De + m];
                    bv = a.hT[r * a.H + n];
                }
            }
            As[rr][cc] = av;
            Bs[rr][cc] = bv;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < 32; ++k) {
            const float a0 = As[k][2 * ty], a1 = As[k][2 * ty + 1], b0 = Bs[k][2 * tx], b1 = Bs[k][2 * tx + 1];
            acc[0][0] += a0 * b0; acc[0][1] += a0 * b1; acc[1][0] += a1 * b0; acc[1][1] += a1 * b1;
        }
        __syncthreads();
    }
    float* out = a.partial + (int64_t)blockIdx.y * a.Md * a.Nd;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) out[(int64_t)(m0 + 2 * ty + u) * a.Nd + n0 + 2 * tx + v] = acc[u][v];
}

// out = the partials of the chunks that hold rows, added in chunk order
__global__ __launch_bounds__(GT) void k_gru_atb_sum(AtbArgs a, float* out) {
    const int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x, MN = (int64_t)a.Md * a.Nd;
    if (i >= MN) return;
    const int64_t R = atb_rows(a), chunks = (R + CHUNK - 1) / CHUNK;
    float s = 0.0f;
    for (int64_t c = 0; c < chunks; ++c) s += a.partial[c * MN + i];
    out[i] = s;
}

// dX[r, e] = sum over k of gi[r, k] * W_ih[k, e] for every step row
template <int De>
__global__ __launch_bounds__(GT) void k_gru_dx(const float* __restrict__ stash, const float* __restrict__ W_ih, const uint64_t* n_rows, int H,
                                               float* dX) {
    extern __shared__ __attribute__((aligned(16))) float gsx[];  // [3H][32]
    constexpr int NR = De / 8;                                   // rows of one thread: 256 / De threads side by side cover 32
    const int64_t M = (int64_t)*n_rows, r0 = (int64_t)blockIdx.x * 32;
    if (r0 >= M) return;
    const int K = 3 * H, tid = threadIdx.x;
    for (int i = tid; i < 32 * K; i += GT) {
        const int rr = i / K, k = i % K;
        gsx[k * 32 + rr] = r0 + rr < M ? stash[(r0 + rr) * (5 * H) + H + k] : 0.0f;
    }
    __syncthreads();
    const int e = tid % De, q0 = (tid / De) * NR;
    float acc[NR] = {};
    for (int k = 0; k < K; ++k) {
        const float w = W_ih[k * De + e];
#pragma unroll
        for (int i = 0; i < NR; ++i) acc[i] += w * gsx[k * 32 + q0 + i];
    }
#pragma unroll
    for (int i = 0; i < NR; ++i)
        if (r0 + q0 + i < M) dX[(r0 + q0 + i) * De + e] = acc[i];
}

// ---- item gradient: contributions [0, RL) step rows, [RL, RL + B) targets, [RL + B, RL + 2B) negatives
struct CoArgs {
    const uint64_t* n_steps;     // device: step rows in use
    int64_t RL, B, n2, n_rows;   // B * L; the batch; RL + 2B; n_aids + 1 (the key of a contribution that is dropped)
    const int32_t* xrow;
    const uint32_t* order;
    const int32_t* target;
    const int32_t* neg;
    const float* dX;
    const float* cO;
    int De;
};

__global__ __launch_bounds__(GT) void k_co_keys(CoArgs a, uint64_t* key, uint32_t* val) {
    const int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (i >= a.n2) return;
    int64_t row = 0;
    if (i < a.RL) {
        if (i < (int64_t)*a.n_steps) { const int32_t xr = a.xrow[i]; row = xr < 0 ? -xr - 1 : xr; }
    } else {
        const bool tgt = i < a.RL + a.B;
        const int64_t orig = a.order[i - a.RL - (tgt ? 0 : a.B)];
        if (orig < a.B) row = row_of((tgt ? a.target : a.neg)[orig], a.n_rows - 1);
    }
    key[i] = row > 0 && row < a.n_rows ? (uint64_t)row : (uint64_t)a.n_rows;      // PAD receives nothing
    val[i] = (uint32_t)i;
}

__global__ __launch_bounds__(GT) void k_co_heads(const uint64_t* __restrict__ key, int64_t n2, int64_t n_rows, uint8_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (i < n2) flag[i] = key[i] < (uint64_t)n_rows && (i == 0 || key[i - 1] != key[i]);
}

__global__ __launch_bounds__(GT) void k_co_start(const uint8_t* __restrict__ flag, const uint64_t* __restrict__ pos, int64_t n2, uint64_t* start,
                                                 int64_t cap, int64_t* count) {
    const int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (i == 0) *count = (int64_t)pos[n2] < cap ? (int64_t)pos[n2] : cap;
    if (i < n2 && flag[i]) start[pos[i]] = (uint64_t)i;           // pos[i] < n2
}

__global__ __launch_bounds__(GT) void k_co_sum(CoArgs a, const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                               const uint64_t* __restrict__ start, const int64_t* count, int64_t cap, int32_t* ids, float* rows) {
    const int64_t cnt = *count < cap ? *count : cap, total = cnt * a.De;
    for (int64_t idx = (int64_t)blockIdx.x * GT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * GT) {
        const int64_t q = idx / a.De;
        const int e = (int)(idx % a.De);
        const int64_t i0 = (int64_t)start[q];
        if (i0 >= a.n2) continue;
        const uint64_t id = key[i0];
        float acc = 0.0f;
        for (int64_t i = i0; i < a.n2 && key[i] == id; ++i) {    // contribution order: the sort is stable
            const int64_t c = val[i];
            float v = 0.0f;
            if (c < a.RL) v = a.dX[c * a.De + e];
            else if (c < a.RL + a.B) v = a.cO[(c - a.RL) * a.De + e];
            else if (c < a.n2) v = -a.cO[(c - a.RL - a.B) * a.De + e];
            acc += v;
        }
        rows[idx] = acc;
        if (e == 0) ids[q] = (int32_t)id;
    }
}

// loss sum (double) and b_d's gradient: four interleaved parts per column, 256 per loss, folded in index order
__global__ __launch_bounds__(GT) void k_gru_final(const float* __restrict__ lossv, const float* __restrict__ dO, int64_t B, int De, double* loss_sum,
                                                  float* gb) {
    __shared__ double s_l[GT];
    __shared__ float s_b[4][64];
    const int tid = threadIdx.x, e = tid & 63, part = tid >> 6;
    double l = 0.0;
    for (int64_t b = tid; b < B; b += GT) l += (double)lossv[b];
    s_l[tid] = l;
    float g = 0.0f;
    if (e < De)
        for (int64_t b = part; b < B; b += 4) g += dO[b * De + e];
    s_b[part][e] = g;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < GT; ++i) s += s_l[i];
        *loss_sum = s;
    }
    if (tid < De) gb[tid] = ((s_b[0][tid] + s_b[1][tid]) + s_b[2][tid]) + s_b[3][tid];
}

struct GruWs {
    RadixWs rl;                  // the length sort; rl.offs holds the step offsets afterwards
    float *wt_ih, *wt_hh, *wt_d;
    float* stash;
    int32_t* xrow;
    float *hT, *dO, *cO, *lossv, *dX;
    float *part_ih, *part_hh, *part_d;
    RadixWs rc;                  // the contribution sort
    uint8_t* flag;
    uint64_t* start;
};

size_t gru_layout(int64_t B, int L, int De, int H, bool grad, char* base, GruWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    GruWs t;
    memset(&t, 0, sizeof t);
    o += radix_ws_layout(B, false, base, &t.rl);
    t.wt_ih = (float*)take((size_t)3 * H * De * 4);
    t.wt_hh = (float*)take((size_t)3 * H * H * 4);
    t.wt_d = (float*)take((size_t)De * H * 4);
    if (grad) {
        const size_t RL = (size_t)B * L, n2 = RL + 2 * (size_t)B;
        const size_t chunks = (RL + CHUNK - 1) / CHUNK, chunks_d = ((size_t)B + CHUNK - 1) / CHUNK;
        t.stash = (float*)take(RL * 5 * H * 4);
        t.xrow = (int32_t*)take(RL * 4);
        t.hT = (float*)take((size_t)B * H * 4);
        t.dO = (float*)take((size_t)B * De * 4);
        t.cO = (float*)take((size_t)B * De * 4);
        t.lossv = (float*)take((size_t)B * 4);
        t.dX = (float*)take(RL * De * 4);
        t.part_ih = (float*)take(chunks * 3 * H * De * 4);
        t.part_hh = (float*)take(chunks * 3 * H * H * 4);
        t.part_d = (float*)take(chunks_d * De * H * 4);
        o += radix_ws_layout((int64_t)n2, false, base ? base + o : nullptr, &t.rc);
        t.flag = (uint8_t*)take(n2);
        t.start = (uint64_t*)take((n2 + 1) * 8);
    }
    if (w) *w = t;
    return o;
}

int gru_check(const otto_gru_job* j, const char* who) {
    OTTO_REQUIRE(j, "%s: null job", who);
    OTTO_REQUIRE(j->De == 32 || j->De == 64, "%s: De must be 32 or 64 (got %d)", who, j->De);
    OTTO_REQUIRE(j->H == 32 || j->H == 64 || j->H == 128, "%s: H must be 32, 64 or 128 (got %d)", who, j->H);
    OTTO_REQUIRE(j->B >= 0 && j->B <= OTTO_GRU_MAX_BATCH, "%s: B must be in [0, %d] (got %lld)", who, OTTO_GRU_MAX_BATCH, (long long)j->B);
    OTTO_REQUIRE(j->max_len >= 1 && j->max_len <= OTTO_GRU_MAX_LEN, "%s: max_len must be in [1, %d] (got %d)", who, OTTO_GRU_MAX_LEN, j->max_len);
    OTTO_REQUIRE(j->n_aids >= 1 && j->n_aids < (1ll << 31) - 1, "%s: n_aids must be in [1, 2^31 - 1) (got %lld)", who, (long long)j->n_aids);
    OTTO_REQUIRE(j->n_events >= 0 && j->n_events < (1ll << 31), "%s: n_events must be in [0, 2^31) (got %lld)", who, (long long)j->n_events);
    OTTO_REQUIRE(j->reserved == 0, "%s: reserved must be 0", who);
    return 0;
}

template <bool TRAIN>
int launch_tile(int De, int H, unsigned tiles, const TileArgs& a, hipStream_t s) {
#define OTTO_GRU_CASE(D, HH) \
    if (De == D && H == HH) { k_gru_tile<D, HH, TRAIN><<<tiles, 2 * HH, 0, s>>>(a); OTTO_HIP(hipGetLastError()); return 0; }
    OTTO_GRU_CASE(32, 32) OTTO_GRU_CASE(32, 64) OTTO_GRU_CASE(32, 128)
    OTTO_GRU_CASE(64, 32) OTTO_GRU_CASE(64, 64) OTTO_GRU_CASE(64, 128)
#undef OTTO_GRU_CASE
    set_error("otto_gru: De = %d, H = %d is not built", De, H);
    return -22;
}

int atb(AtbArgs a, int64_t max_rows, float* out, hipStream_t s) {
    const int64_t chunks = (max_rows + CHUNK - 1) / CHUNK;
    k_gru_atb<<<dim3((unsigned)((a.Md / 32) * (a.Nd / 32)), (unsigned)chunks), GT, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    k_gru_atb_sum<<<blocks_for((int64_t)a.Md * a.Nd), GT, 0, s>>>(a, out);
    OTTO_HIP(hipGetLastError());
    return 0;
}

// forward (grad = false) or forward + backward of one batch
int gru_run(const otto_gru_job& j, bool grad, const char* who) {
    OTTO_TRY(gru_check(&j, who));
    const int64_t B = j.B;
    const int De = j.De, H = j.H, L = j.max_len;
    hipStream_t s = (hipStream_t)j.stream;
    if (grad) {
        OTTO_REQUIRE(j.d_gW_ih && j.d_gW_hh && j.d_gW_d && j.d_gb_d && j.d_count && j.d_loss_sum, "%s: null gradient output", who);
        if (B == 0) {                                            // nothing to learn from: zero gradients, an empty list
            OTTO_HIP(hipMemsetAsync(j.d_gW_ih, 0, (size_t)3 * H * De * 4, s));
            OTTO_HIP(hipMemsetAsync(j.d_gW_hh, 0, (size_t)3 * H * H * 4, s));
            OTTO_HIP(hipMemsetAsync(j.d_gW_d, 0, (size_t)De * H * 4, s));
            OTTO_HIP(hipMemsetAsync(j.d_gb_d, 0, (size_t)De * 4, s));
            OTTO_HIP(hipMemsetAsync(j.d_count, 0, 8, s));
            OTTO_HIP(hipMemsetAsync(j.d_loss_sum, 0, 8, s));
            return 0;
        }
    }
    if (B == 0) return 0;
    OTTO_REQUIRE(j.d_E && j.d_W_ih && j.d_W_hh && j.d_W_d && j.d_b_d, "%s: null parameter", who);
    OTTO_REQUIRE(j.d_seq_lo && j.d_seq_len && (j.n_events == 0 || j.d_aid), "%s: null input", who);
    OTTO_REQUIRE(grad || j.d_o, "%s: null output", who);
    const int64_t RL = B * L, n2 = RL + 2 * B;
    if (grad) {
        OTTO_REQUIRE(j.d_target && j.d_neg, "%s: null target or negative", who);
        const int64_t need_cap = n2 < j.n_aids ? n2 : j.n_aids;
        OTTO_REQUIRE(j.d_ids && j.d_rows && j.cap >= need_cap, "%s: the export list needs room for %lld rows (cap = %lld)", who,
                     (long long)need_cap, (long long)j.cap);
    }
    OTTO_REQUIRE(j.d_work && ((uintptr_t)j.d_work & 255) == 0, "%s: a 256-byte aligned workspace is needed", who);
    const int64_t need = (int64_t)gru_layout(B, L, De, H, grad, nullptr, nullptr);
    OTTO_REQUIRE(j.work_bytes >= need, "%s: workspace too small (%lld < %lld)", who, (long long)j.work_bytes, (long long)need);
    GruWs w;
    gru_layout(B, L, De, H, grad, (char*)j.d_work, &w);

    k_gru_transpose<<<blocks_for(3 * H * De + 3 * H * H + De * H), GT, 0, s>>>(j.d_W_ih, j.d_W_hh, j.d_W_d, De, H, w.wt_ih, w.wt_hh, w.wt_d);
    OTTO_HIP(hipGetLastError());
    k_gru_len_keys<<<blocks_for(B), GT, 0, s>>>(j.d_seq_lo, j.d_seq_len, B, j.n_events, L, w.rl.key[0], w.rl.val[0]);
    OTTO_HIP(hipGetLastError());
    int cur = 0;
    OTTO_TRY((radix_passes<false>(w.rl, B, 0xFFull, SkipOnHost{}, &cur, s)));        // lengths fit one digit
    if (grad) OTTO_TRY(device_scan(LenAt{w.rl.key[cur], L}, B, w.rl.offs, w.rl.partial, s));
    const uint64_t* n_steps = w.rl.offs + B;

    TileArgs a;
    memset(&a, 0, sizeof a);
    a.E = j.d_E; a.wt_ih = w.wt_ih; a.wt_hh = w.wt_hh; a.wt_d = w.wt_d; a.W_hh = j.d_W_hh; a.W_d = j.d_W_d; a.b_d = j.d_b_d;
    a.n_aids = j.n_aids; a.aid = j.d_aid; a.seq_lo = j.d_seq_lo; a.target = j.d_target; a.neg = j.d_neg; a.B = B; a.L = L;
    a.lkey = w.rl.key[cur]; a.order = w.rl.val[cur]; a.step_off = w.rl.offs; a.o = j.d_o;
    a.stash = w.stash; a.xrow = w.xrow; a.hT = w.hT; a.dO = w.dO; a.cO = w.cO; a.lossv = w.lossv; a.inv_b = 1.0f / (float)B;
    const unsigned tiles = (unsigned)((B + TS - 1) / TS);
    if (!grad) return launch_tile<false>(De, H, tiles, a, s);
    OTTO_TRY(launch_tile<true>(De, H, tiles, a, s));

    AtbArgs g;
    memset(&g, 0, sizeof g);
    g.stash = w.stash; g.xrow = w.xrow; g.E = j.d_E; g.dO = w.dO; g.hT = w.hT; g.De = De; g.H = H;
    g.mode = ATB_IH; g.rows_dev = n_steps; g.Md = 3 * H; g.Nd = De; g.partial = w.part_ih;
    OTTO_TRY(atb(g, RL, j.d_gW_ih, s));
    g.mode = ATB_HH; g.Nd = H; g.partial = w.part_hh;
    OTTO_TRY(atb(g, RL, j.d_gW_hh, s));
    g.mode = ATB_D; g.rows_dev = nullptr; g.rows_host = B; g.Md = De; g.Nd = H; g.partial = w.part_d;
    OTTO_TRY(atb(g, B, j.d_gW_d, s));

    const unsigned dx_blocks = (unsigned)((RL + 31) / 32);
    const size_t dx_lds = (size_t)3 * H * 32 * 4;
    if (De == 32) k_gru_dx<32><<<dx_blocks, GT, dx_lds, s>>>(w.stash, j.d_W_ih, n_steps, H, w.dX);
    else k_gru_dx<64><<<dx_blocks, GT, dx_lds, s>>>(w.stash, j.d_W_ih, n_steps, H, w.dX);
    OTTO_HIP(hipGetLastError());

    CoArgs c;
    c.n_steps = n_steps; c.RL = RL; c.B = B; c.n2 = n2; c.n_rows = j.n_aids + 1; c.xrow = w.xrow; c.order = a.order;
    c.target = j.d_target; c.neg = j.d_neg; c.dX = w.dX; c.cO = w.cO; c.De = De;
    k_co_keys<<<blocks_for(n2), GT, 0, s>>>(c, w.rc.key[0], w.rc.val[0]);
    OTTO_HIP(hipGetLastError());
    uint64_t digits = 1;
    while (digits <= (uint64_t)c.n_rows) digits <<= 1;           // the keys are 1 .. n_rows
    int ccur = 0;
    OTTO_TRY((radix_passes<false>(w.rc, n2, digits - 1, SkipOnHost{}, &ccur, s)));
    k_co_heads<<<blocks_for(n2), GT, 0, s>>>(w.rc.key[ccur], n2, c.n_rows, w.flag);
    OTTO_HIP(hipGetLastError());
    OTTO_TRY(device_scan(FlagAt{w.flag}, n2, w.rc.offs, w.rc.partial, s));
    k_co_start<<<blocks_for(n2), GT, 0, s>>>(w.flag, w.rc.offs, n2, w.start, j.cap, j.d_count);
    OTTO_HIP(hipGetLastError());
    const int64_t most = (n2 < j.cap ? n2 : j.cap) * De;
    k_co_sum<<<capped_blocks(most), GT, 0, s>>>(c, w.rc.key[ccur], w.rc.val[ccur], w.start, j.d_count, j.cap, j.d_ids, j.d_rows);
    OTTO_HIP(hipGetLastError());
    k_gru_final<<<1, GT, 0, s>>>(w.lossv, w.dO, B, De, j.d_loss_sum, j.d_gb_d);
    OTTO_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// apply
// ---------------------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
struct AdamArgs {
    float* p[4];
    float* m[4];
    float* v[4];
    const float* g[4];
    int64_t end[4];              // running ends of the four tensors in the launch's index space
    float omb1, b2, omb2, eps, step_size, bc2_sqrt;
    // the rows of the item table
    float *E, *mE, *vE;
    const int32_t* ids;
    const float* rows;
    const int64_t* count;
    int64_t cap, n_aids;
    int De;
    float row_step_size;
};

__global__ __launch_bounds__(GT) void k_gru_adam(AdamArgs a) {
    const int64_t i = (int64_t)blockIdx.x * GT + threadIdx.x;
    if (i >= a.end[3]) return;
    const int q = i < a.end[0] ? 0 : i < a.end[1] ? 1 : i < a.end[2] ? 2 : 3;
    const int64_t k = i - (q ? a.end[q - 1] : 0);
    const float g = a.g[q][k];
    float m = a.m[q][k], v = a.v[q][k];
    m = m + (g - m) * a.omb1;
    v = v * a.b2 + (a.omb2 * g) * g;
    a.m[q][k] = m;
    a.v[q][k] = v;
    a.p[q][k] = a.p[q][k] + (-a.step_size) * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
}

__global__ __launch_bounds__(GT) void k_gru_adam_rows(AdamArgs a) {
    const int64_t cnt = *a.count < a.cap ? *a.count : a.cap, total = cnt * a.De;
    for (int64_t idx = (int64_t)blockIdx.x * GT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * GT) {
        const int64_t id = a.ids[idx / a.De];
        if (id < 1 || id > a.n_aids) continue;                   // PAD and anything that is no row
        const int64_t k = id * a.De + idx % a.De;
        const float g = a.rows[idx];
        // torch/optim/_functional.py sparse_adam. Not shared with adam1 of otto_mf.hip: this kernel is compiled with fp
        // contraction off and adam1 with it on, and one inline function would take one of the two states for both
        float m = a.mE[k], v = a.vE[k];
        m = m + (g - m) * a.omb1;
        v = v + (g * g - v) * a.omb2;
        a.mE[k] = m;
        a.vE[k] = v;
        a.E[k] = a.E[k] + (-a.row_step_size) * (m / (sqrtf(v) + a.eps));
    }
}

}  // namespace
}  // namespace otto

using namespace otto;

extern "C" int64_t otto_gru_plan_workspace(const otto_gru_plan_job* job) {
    if (plan_check(job) != 0) return -22;
    return (int64_t)plan_layout(job->n_events, nullptr, nullptr);
}

extern "C" int otto_gru_plan(const otto_gru_plan_job* job, int64_t* h_n, int64_t* h_err) {
    OTTO_REQUIRE(h_n && h_err, "otto_gru_plan: null h_n or h_err");
    *h_n = 0;
    h_err[0] = -1;
    h_err[1] = 0;
    OTTO_TRY(plan_check(job));
    const otto_gru_plan_job& j = *job;
    const int64_t E = j.n_events, S = j.n_sessions;
    OTTO_REQUIRE(j.d_sess_off, "otto_gru_plan: null sess_off");
    OTTO_REQUIRE(E == 0 || j.d_aid, "otto_gru_plan: null aid");
    OTTO_REQUIRE(j.d_work && ((uintptr_t)j.d_work & 255) == 0, "otto_gru_plan: a 256-byte aligned workspace is needed");
    const int64_t need = (int64_t)plan_layout(E, nullptr, nullptr);
    OTTO_REQUIRE(j.work_bytes >= need, "otto_gru_plan: workspace too small (%lld < %lld)", (long long)j.work_bytes, (long long)need);
    hipStream_t s = (hipStream_t)j.stream;
    PlanWs w;
    plan_layout(E, (char*)j.d_work, &w);
    OTTO_HIP(hipMemsetAsync(w.ctrl, 0, sizeof(PlanCtrl), s));
    OTTO_HIP(hipMemsetAsync(&w.ctrl->err_off, 0xFF, 16, s));     // both error words
    OTTO_HIP(hipMemsetAsync(&w.ctrl->key_bits[1], 0xFF, 8, s));  // the AND of the keys starts at all ones
    k_plan_check<<<blocks_for((E > S + 1 ? E : S + 1)), GT, 0, s>>>(j.d_aid, j.d_sess_off, E, S, j.n_aids, w.ctrl);
    OTTO_HIP(hipGetLastError());
    if (E > 0 && S > 0) {
        k_plan_keys<<<blocks_for(E), GT, 0, s>>>(j.d_sess_off, E, S, j.seed, j.epoch, w.r.key[0], w.r.val[0], w.ctrl);
        OTTO_HIP(hipGetLastError());
    }
    PlanCtrl h;
    OTTO_HIP(hipMemcpyAsync(&h, w.ctrl, sizeof h, hipMemcpyDeviceToHost, s));
    OTTO_HIP(hipStreamSynchronize(s));
    if (h.err_off != ~0ull) {
        h_err[0] = (int64_t)h.err_off;
        h_err[1] = 1;
        OTTO_REQUIRE(false, "otto_gru_plan: sess_off[%lld] breaks the offsets (0, non-decreasing, n_events)", (long long)h_err[0]);
    }
    if (h.err_aid != ~0ull) {
        h_err[0] = (int64_t)h.err_aid;
        h_err[1] = 2;
        OTTO_REQUIRE(false, "otto_gru_plan: event %lld: aid outside [0, n_aids)", (long long)h_err[0]);
    }
    const int64_t N = (int64_t)h.n;
    if (N == 0) return 0;
    OTTO_REQUIRE(N <= E, "otto_gru_plan: %lld samples of %lld events", (long long)N, (long long)E);
    OTTO_REQUIRE(j.d_p && j.d_seq_lo && j.d_seq_len && j.d_target && j.d_neg, "otto_gru_plan: null output");
    int cur = 0;                                                 // all eight passes are launched, an even number: the sorted rows end in buffer 0
    OTTO_TRY((radix_passes<false>(w.r, E, ~0ull, SkipOnDevice{w.ctrl->key_bits}, &cur, s)));
    k_plan_emit<<<blocks_for(N), GT, 0, s>>>(w.r.val[0], N, j.d_aid, j.d_sess_off, E, S, j.n_aids, j.max_len, j.seed, j.epoch, j.d_p, j.d_seq_lo,
                                             j.d_seq_len, j.d_target, j.d_neg);
    OTTO_HIP(hipGetLastError());
    *h_n = N;
    return 0;
}

extern "C" int64_t otto_gru_workspace(const otto_gru_job* job, int32_t grad) {
    if (gru_check(job, "otto_gru_workspace") != 0) return -22;
    return (int64_t)gru_layout(job->B, job->max_len, job->De, job->H, grad != 0, nullptr, nullptr);
}

extern "C" int otto_gru_encode(const otto_gru_job* job) {
    OTTO_REQUIRE(job, "otto_gru_encode: null job");
    return gru_run(*job, false, "otto_gru_encode");
}

extern "C" int otto_gru_grad(const otto_gru_job* job) {
    OTTO_REQUIRE(job, "otto_gru_grad: null job");
    return gru_run(*job, true, "otto_gru_grad");
}

extern "C" int otto_gru_apply(const otto_gru_apply_job* job) {
    OTTO_REQUIRE(job, "otto_gru_apply: null job");
    const otto_gru_apply_job& j = *job;
    OTTO_REQUIRE(j.De == 32 || j.De == 64, "otto_gru_apply: De must be 32 or 64 (got %d)", j.De);
    OTTO_REQUIRE(j.H == 32 || j.H == 64 || j.H == 128, "otto_gru_apply: H must be 32, 64 or 128 (got %d)", j.H);
    OTTO_REQUIRE(j.n_aids >= 1 && j.n_aids < (1ll << 31) - 1, "otto_gru_apply: n_aids must be in [1, 2^31 - 1) (got %lld)", (long long)j.n_aids);
    OTTO_REQUIRE(j.t >= 1, "otto_gru_apply: t is the 1-based step (got %lld)", (long long)j.t);
    OTTO_REQUIRE(j.cap >= 0 && j.d_count, "otto_gru_apply: null count");
    OTTO_REQUIRE(j.d_E && j.d_mE && j.d_vE, "otto_gru_apply: null item table or moments");
    for (int q = 0; q < 4; ++q) OTTO_REQUIRE(j.d_W[q] && j.d_m[q] && j.d_v[q] && j.d_g[q], "otto_gru_apply: null tensor %d", q);
    hipStream_t s = (hipStream_t)j.stream;
    AdamArgs a;
    memset(&a, 0, sizeof a);
    const int64_t sizes[4] = {(int64_t)3 * j.H * j.De, (int64_t)3 * j.H * j.H, (int64_t)j.De * j.H, j.De};
    int64_t run = 0;
    for (int q = 0; q < 4; ++q) {
        a.p[q] = j.d_W[q]; a.m[q] = j.d_m[q]; a.v[q] = j.d_v[q]; a.g[q] = j.d_g[q];
        run += sizes[q];
        a.end[q] = run;
    }
    // torch evaluates the bias corrections in double on the host and hands them to float32 kernels
    const double bc1 = 1.0 - pow(j.beta1, (double)j.t), bc2 = 1.0 - pow(j.beta2, (double)j.t);
    a.omb1 = (float)(1.0 - j.beta1); a.b2 = (float)j.beta2; a.omb2 = (float)(1.0 - j.beta2); a.eps = (float)j.eps;
    a.step_size = (float)(j.lr / bc1);
    a.bc2_sqrt = (float)sqrt(bc2);
    a.row_step_size = (float)(j.lr * sqrt(bc2) / bc1);
    a.E = j.d_E; a.mE = j.d_mE; a.vE = j.d_vE; a.ids = j.d_ids; a.rows = j.d_rows; a.count = j.d_count; a.cap = j.cap;
    a.n_aids = j.n_aids; a.De = j.De;
    k_gru_adam<<<blocks_for(run), GT, 0, s>>>(a);
    OTTO_HIP(hipGetLastError());
    if (j.cap > 0) {
        OTTO_REQUIRE(j.d_ids && j.d_rows, "otto_gru_apply: null list");
        k_gru_adam_rows<<<capped_blocks(j.cap * j.De), GT, 0, s>>>(a);
        OTTO_HIP(hipGetLastError());
    }
    return 0;
}
