/*
 * otto_knn.h -- C-ABI of the exact nearest-neighbour table over aid embeddings (SPEC-KNN).
 *
 * What this replaces in the reference: the Annoy index over fastText vectors that the candidate scripts query once per
 * session (src/covisitation/inference.py:58-69,166,223, src/ranker/regular_candidate_generation.py:58-70,157,338,
 * src/ranker/fasttext_candidate_generator.py:75-98). Here the table is exact (brute force on the f32 matrix cores) and
 * is built once per embedding table; its lists are not expected to reproduce an approximate index over other vectors.
 *
 * Conventions of otto_covis.h: 0 or a negative OTTO_E* code plus otto_last_error; caller-owned device buffers;
 * all work on the caller's stream; nothing is allocated inside.
 * otto_knn_workspace, the one function without a stream parameter, runs on the host and enqueues nothing.
 *
 * Per query aid a = d_rows[r] (d_rows == NULL: a = r, n_rows == N): all b != a with valid[b] != 0, ordered by
 * (key asc, b asc), the first k:
 *     OTTO_KNN_EUCLIDEAN  key = sum_i (a_i - b_i)^2            dist = sqrt(max(key, 0))
 *     OTTO_KNN_ANGULAR    key = 2 - 2 cos(a, b), 2 if a norm is 0   dist = sqrt(max(key, 0))
 *     OTTO_KNN_DOT        key = -<a, b>                         dist = <a, b>
 * d_ids [n_rows, k] int32 (-1 padded), d_dist [n_rows, k] float32 (+inf padded), d_n [n_rows] int32 (0 for a query aid
 * with valid == 0). fp32 throughout, exact-f32 MFMA contraction; the order is that of the fp32 keys the kernel
 * computes (euclidean: |b|^2 - 2<a,b>, the row constant |a|^2 is added for dist only), exact fp32 ties to the smaller id.
 * Self is excluded by id, not by distance.
 *
 * A d_rows entry outside [0, N) is detected on the device: its row comes back empty and the call returns OTTO_EINVAL
 * after the stream has drained. The call synchronises the stream once to read that error word.
 */
#ifndef OTTO_KNN_H
#define OTTO_KNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTTO_KNN_EUCLIDEAN 0
#define OTTO_KNN_ANGULAR 1
#define OTTO_KNN_DOT 2
#define OTTO_KNN_MAX_K 64

/* bytes of d_workspace the table call needs; 0 for arguments it would refuse */
int64_t otto_knn_workspace(int64_t n_rows, int64_t N, int32_t d, int32_t k, int32_t metric);

/* d_E float32 [N, d] row-major, d in {8, 16, 32, 64, 128}; d_valid uint8 [N] or NULL; d_rows int32 [n_rows] or NULL;
 * 1 <= k <= OTTO_KNN_MAX_K. */
int otto_knn_table(const float* d_E, int64_t N, int32_t d, const uint8_t* d_valid, const int32_t* d_rows, int64_t n_rows,
                   int32_t k, int32_t metric, int32_t* d_ids, float* d_dist, int32_t* d_n, void* d_workspace,
                   int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
