/*
 * otto_rows.h -- C-ABI of the rows -> resident top-k step: the (aid_x, aid_y, wgt) rows of the covisitation part files, as
 * otto_parquet.h decodes them, back into the padded arrays CovisBuilder.finalize returns and otto_cand_lookup takes
 * (DESIGN.md section 2g). The inverse of engine.topk_to_device_rows.
 *
 * Reference code replaced: the pandas groupby / dict building in front of every consumer of the part files
 * (src/covisitation/inference.py:87-111, src/ranker/covisitation_candidate_generation.py:49-73,
 * src/ranker/regular_candidate_generation.py:75-101). Host restatement: tests/parts_restatement.py.
 *
 * SPEC-ROWS (normative)
 * ---------------------
 * Inputs. aid_x, aid_y int32 and wgt float32 of n_rows rows, aid_x non-decreasing; n_aids >= 0; 1 <= k <= 64.
 * Outputs. y int32 [n_aids, k], w float32 [n_aids, k], n int32 [n_aids]. The rows of one aid_x value are a run; the row at
 * position r of the run of aid a goes to y[a, r] / w[a, r] (aid_y and the bits of wgt); n[a] is the run's length. Every other
 * slot is y = -1, w = 0; aids without rows get n = 0.
 *
 * Refused, in this order for one row: OTTO_ROWS_E_AID_X aid_x outside [0, n_aids); OTTO_ROWS_E_AID_Y aid_y outside
 * [0, n_aids); OTTO_ROWS_E_ORDER aid_x[i] < aid_x[i-1]; OTTO_ROWS_E_RUN the row's position in its run is >= k (a run
 * longer than k: its row k is the offending one). A refusal returns -22, h_err[0] = the smallest offending row, h_err[1] =
 * that row's first reason in the order above; otto_last_error() carries the text. Nothing is stored outside the three
 * outputs; their contents are then unspecified. Without a refusal h_err = {-1, 0}.
 *
 * Kernel. k_rows_topk, one wave per 64 consecutive rows. A row is a head where its aid_x differs from the previous row's; a
 * ballot of the head flags gives every lane its run's start inside the wave. Only the run that began before the wave's
 * first row looks back: that walk is wave-uniform and at most k steps (a longer one is the OTTO_ROWS_E_RUN refusal). The
 * lane at a run's last row writes n. The padding is written by fills in front of the kernel.
 *
 * Conventions as in otto_pqwrite.h: 0 / negative code + otto_last_error(); the caller owns every buffer; d_* are device
 * pointers, h_* host pointers; all arguments travel in one record and the caller's hipStream_t rides in it (the calling
 * guarantees -- side stream, late inputs, reused scratch -- are tested in tests/test_parts_gpu.py). The call synchronises
 * the stream once, to read the error word.
 */
#ifndef OTTO_ROWS_H
#define OTTO_ROWS_H

#include <stdint.h>

#define OTTO_ROWS_MAX_K 64
#define OTTO_ROWS_E_AID_X 1
#define OTTO_ROWS_E_AID_Y 2
#define OTTO_ROWS_E_ORDER 3
#define OTTO_ROWS_E_RUN 4

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const int32_t* d_aid_x;    /* n_rows, non-decreasing */
    const int32_t* d_aid_y;    /* n_rows */
    const float* d_wgt;        /* n_rows */
    int64_t n_rows;            /* >= 0 */
    int32_t* d_y;              /* n_aids * k */
    float* d_w;                /* n_aids * k */
    int32_t* d_n;              /* n_aids */
    int64_t n_aids;            /* 0 .. 2^31 - 1 */
    int32_t k;                 /* 1 .. OTTO_ROWS_MAX_K */
    int32_t reserved;          /* 0 */
    void* d_work;
    int64_t work_bytes;
    void* stream;              /* the caller's hipStream_t; every launch and copy goes there */
} otto_rows_job;

/* Bytes of scratch otto_rows_topk needs for this job (d_work and work_bytes are not looked at), or -22 for a job that
 * breaks a rule above. Host only: enqueues nothing. */
int64_t otto_rows_workspace(const otto_rows_job* job);

/* SPEC-ROWS. h_err: two int64 (above). Synchronises the stream once. */
int otto_rows_topk(const otto_rows_job* job, int64_t* h_err);

#ifdef __cplusplus
}
#endif
#endif
