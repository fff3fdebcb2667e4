/*
 * otto_gru.h -- C-ABI of the GRU4Rec session model: the epoch plan, the recurrent encoder, back-propagation through time
 * and the two Adam updates. The package's first dense, recurrent workload.
 *
 * Reference code replaced: src/recbole/trainer.py:8-9,38 (any model of recbole.model.sequential_recommender built by name,
 * trained by RecBole's Trainer) and the sequential branch of src/recbole/inference.py:58-72 (the session's aids padded to
 * 20, passed as aid_list / item_length to full_sort_predict). RecBole is not installed and not vendored:
 * the model follows RecBole 1.1.1's GRU4Rec as its published source reads, the arithmetic below is build-defined and
 * parity with RecBole is not claimed. Host restatement: tests/gru_restatement.py, itself checked against torch.nn.GRU
 * with autograd on the CPU (tests/test_gru_cpu.py).
 *
 * SPEC-GRU4REC (normative)
 * ------------------------
 * MODEL. Item table E float32 [n_aids + 1, De]; row 0 is PAD: all zero, never updated, never drawn as a negative; aid a
 * lives in row a + 1. One GRU layer without biases, W_ih [3H, De], W_hh [3H, H], gate rows in torch's order r, z, n:
 *     r = sigma(W_ir x + W_hr h)      z = sigma(W_iz x + W_hz h)      n = tanh(W_in x + r * (W_hn h))
 *     h' = (1 - z) * n + z * h        h_0 = 0
 * and a dense layer o = W_d h_T + b_d, W_d [De, H], b_d [De]. De in {32, 64}, H in {32, 64, 128}; anything else is
 * refused. All arithmetic is float32 with exact expf / tanhf / logf (no tables, no fast-math intrinsics); sigma(x) =
 * 1 / (1 + expf(-x)). The order of the sums is free, but fixed for a given input (DETERMINISM, below).
 *
 * SAMPLES. Events aid int32 [E], sessions sess_off int64 [S + 1] (sess_off[0] = 0, non-decreasing, sess_off[S] = E).
 * For a session with events [lo, hi) every p in lo + 1 .. hi - 1 is one sample, named by the global event index p:
 * target aid[p], input sequence aid[max(lo, p - L) .. p - 1] (seq_lo = max(lo, p - L), seq_len = p - seq_lo), 1 <= L <=
 * OTTO_GRU_MAX_LEN. Sessions of length 0 or 1 give no sample. Only the real steps are run (RecBole runs the padded tail
 * and gathers the state at item_length - 1; for a causal GRU that is the same value).
 *
 * EPOCH ORDER. key(seed, epoch, p) = mix64(mix64(seed ^ epoch * 0xD1342543DE82EF95) ^ p * 0xA0761D6478BD642F) >> 1 (mix64
 * of csrc/common.h, all products modulo 2^64). The samples are ordered by (key, p); batch q is positions [qB, (q + 1)B)
 * of that order. No draw depends on the grid or on how the epoch is cut into launches.
 *
 * LOSS. BPR, one negative per sample: neg = bpr_negative(seed, epoch, p, target, n_aids) of oracle/mf_oracle.py (uniform
 * over the aids by multiply-high, redrawn up to 16 times while equal to the target, then (target + 1) % n_aids), that
 * is rows 1 .. n_aids. x = <o, E[target + 1]> - <o, E[neg + 1]>, loss = -logf(1e-10 + sigma(x)), meaned over the batch
 * (1e-10 is the gamma of RecBole's BPRLoss).
 *
 * GRADIENTS. The exact derivatives of the batch-mean loss with respect to E, W_ih, W_hh, W_d and b_d through every time
 * step. A row of E collects what it receives as an input at any step, as a target and as a negative, within one sample
 * and across samples; the item gradient leaves as a coalesced list (ids int32 ascending without repeats, rows float32
 * [., De], a device count).
 *
 * UPDATE. W_ih, W_hh, W_d, b_d: torch.optim.Adam without amsgrad and weight decay,
 *     m = m + (g - m) * (1 - b1);  v = v * b2 + (1 - b2) * g * g;
 *     p = p - (lr / (1 - b1^t)) * (m / (sqrtf(v) / sqrt(1 - b2^t) + eps)),      t the 1-based global step.
 * E: Adam on the rows of the list only, the arithmetic of otto_mf_step_sparse_adam (_adam_rows of oracle/mf_oracle.py);
 * a row that is not in the list keeps its value and its moments bit for bit, row 0 always.
 *
 * DETERMINISM. otto_gru_grad called twice on the same inputs returns the same bytes: partial weight gradients of the
 * workgroups are summed in a fixed order and the rows of the item gradient in the order of their contribution index; no
 * float atomic is used anywhere.
 *
 * Departures from RecBole, on purpose: its sampler also avoids the items of the session's history, this one only the
 * target; it runs dense Adam over the whole item table (on 1.86 M x 64 that is four full tables read and written per
 * step), this one updates the rows present in the batch.
 *
 * Not built (refused by the Python side's argument checks): loss_type CE, dropout_prob != 0, num_layers > 1, the other
 * sequential models (SASRec and the rest), several GPUs, loading a RecBole .pth.
 *
 * Kernels (csrc/otto_gru.hip). PLAN: a check kernel (offsets, aids), one key per event (events that are no sample sort
 * behind every sample), the stable radix sort of radix.h, an emit kernel. ENCODE / GRAD: the batch is ordered by
 * descending length with one radix pass, so that the OTTO_GRU_TILE sequences of a workgroup stop together; k_gru_tile
 * walks the time steps of its tile with x_t and h_t in LDS and the transposed weights read from L2 (2H threads: hidden
 * unit j, half of the tile), keeps h, r, z, n and W_hn h of every step in the workspace, takes the loss and walks back,
 * leaving the pre-activation gradients where r, z, n stood. The three weight gradients are then products over the step
 * rows, cut into chunks of OTTO_GRU_CHUNK rows whose partial results are added in chunk order; the input gradients
 * are one more product and are coalesced by a sort over (row id, contribution). No kernel waits for another workgroup;
 * every loop is bounded by a length of the plan, by a count clipped to its capacity, or by a compile-time capacity.
 *
 * Conventions as in otto_tfidf.h: 0 / negative code + otto_last_error(); the caller owns every buffer; d_* are device
 * pointers, h_* host pointers; all arguments travel in one record and the caller's hipStream_t rides in it; nothing is
 * allocated per call. otto_gru_plan synchronises the stream once; encode, grad and apply only enqueue.
 */
#ifndef OTTO_GRU_H
#define OTTO_GRU_H

#include <stdint.h>

#define OTTO_GRU_MAX_LEN 50             /* RecBole's MAX_ITEM_LIST_LENGTH */
#define OTTO_GRU_TILE 16                /* sequences of one workgroup of k_gru_tile */
#define OTTO_GRU_CHUNK 2048             /* step rows whose weight-gradient partial one workgroup sums */
#define OTTO_GRU_MAX_BATCH (1 << 20)

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const int32_t* d_aid;       /* E */
    const int64_t* d_sess_off;  /* S + 1 */
    int64_t n_events;           /* E, 0 .. 2^31 - 2 */
    int64_t n_sessions;         /* S, 0 .. 2^31 - 2 */
    int64_t n_aids;             /* 1 .. 2^31 - 2 */
    int32_t max_len;            /* L, 1 .. OTTO_GRU_MAX_LEN */
    int32_t reserved;           /* 0 */
    uint64_t seed, epoch;
    int32_t* d_p;               /* E each: the first *h_n entries are written */
    int32_t* d_seq_lo;
    int32_t* d_seq_len;
    int32_t* d_target;          /* aids, not rows */
    int32_t* d_neg;
    void* d_work;
    int64_t work_bytes;
    void* stream;
} otto_gru_plan_job;

/* Bytes of scratch the plan needs (d_work and work_bytes are not looked at), or -22. Host only. */
int64_t otto_gru_plan_workspace(const otto_gru_plan_job* job);
/* SPEC-GRU4REC SAMPLES + EPOCH ORDER + the negatives. *h_n = the number of samples. h_err: two int64. Broken offsets
 * (sess_off[0] != 0, a decreasing pair, sess_off[S] != E): -22, h_err = {the smallest offending offset index, 1}; else an
 * aid outside [0, n_aids): -22, h_err = {the smallest offending event index, 2}; else h_err = {-1, 0}. After a refusal
 * no output has been written. Synchronises the stream once. */
int otto_gru_plan(const otto_gru_plan_job* job, int64_t* h_n, int64_t* h_err);

typedef struct {
    const float* d_E;           /* [n_aids + 1, De] */
    const float* d_W_ih;        /* [3H, De] */
    const float* d_W_hh;        /* [3H, H] */
    const float* d_W_d;         /* [De, H] */
    const float* d_b_d;         /* [De] */
    int64_t n_aids;
    int32_t De, H;
    const int32_t* d_aid;       /* E; an aid outside [0, n_aids) is read as PAD, never followed */
    int64_t n_events;
    const int32_t* d_seq_lo;    /* B; a sequence that leaves [0, E) or is longer than max_len is run as empty */
    const int32_t* d_seq_len;   /* B */
    const int32_t* d_target;    /* B; grad only */
    const int32_t* d_neg;       /* B; grad only */
    int64_t B;                  /* 0 .. OTTO_GRU_MAX_BATCH */
    int32_t max_len;            /* 1 .. OTTO_GRU_MAX_LEN */
    int32_t reserved;           /* 0 */
    float* d_o;                 /* [B, De]; encode writes it, grad too unless NULL */
    float* d_gW_ih;             /* grad only, from here on: the four dense gradients */
    float* d_gW_hh;
    float* d_gW_d;
    float* d_gb_d;
    int32_t* d_ids;             /* [cap] */
    float* d_rows;              /* [cap, De] */
    int64_t cap;                /* >= min(B * (max_len + 2), n_aids) */
    int64_t* d_count;           /* one int64: rows in the list */
    double* d_loss_sum;         /* one double: the SUM of the samples' losses */
    void* d_work;
    int64_t work_bytes;
    void* stream;
} otto_gru_job;

/* Bytes of scratch encode (grad = 0) or grad (grad = 1) needs for job's B, max_len, De, H, or -22. Host only. */
int64_t otto_gru_workspace(const otto_gru_job* job, int32_t grad);
/* The forward pass and nothing else: o = W_d h_T + b_d of every sequence. Enqueues only. */
int otto_gru_encode(const otto_gru_job* job);
/* Forward, loss, BPTT of one batch (SPEC GRADIENTS; every gradient is of the batch MEAN). Enqueues only. */
int otto_gru_grad(const otto_gru_job* job);

typedef struct {
    float* d_E;                 /* [n_aids + 1, De], with its moments */
    float* d_mE;
    float* d_vE;
    int64_t n_aids;
    int32_t De, H;
    float* d_W[4];              /* W_ih, W_hh, W_d, b_d */
    float* d_m[4];
    float* d_v[4];
    const float* d_g[4];        /* their gradients */
    const int32_t* d_ids;       /* the list otto_gru_grad wrote */
    const float* d_rows;
    int64_t cap;
    const int64_t* d_count;     /* read on the device */
    double lr, beta1, beta2, eps;
    int64_t t;                  /* 1-based global step */
    void* stream;
} otto_gru_apply_job;

/* SPEC-GRU4REC UPDATE. An id outside [1, n_aids] is skipped. Enqueues only. */
int otto_gru_apply(const otto_gru_apply_job* job);

#ifdef __cplusplus
}
#endif
#endif
