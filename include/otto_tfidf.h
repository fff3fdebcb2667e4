/*
 * otto_tfidf.h -- C-ABI of the TF-IDF similarity model: the sparse bag-of-aids matrix of the sessions, its transpose, and the
 * cosine top-k between sparse rows. The package's only sparse linear algebra.
 *
 * Reference code replaced: src/tfidf/inference.py:33-37,89-91 (TfidfVectorizer().fit_transform over ' '.join(str(aid)),
 * cosine_similarity(dense_output=False), per-row argsort). Host restatement: tests/tfidf_restatement.py. The reference's
 * indexing defect and the reading built here: SURVEY.md App. E.
 *
 * SPEC-TFIDF (normative)
 * ----------------------
 * Every floating-point operation below is one IEEE-754 binary64 operation, rounded to nearest even, never fused with
 * another; where an order is named, that order is part of the result.
 *
 * COUNT / FILL. Inputs: tok_aid int32 [E], doc_off int64 [D + 1] (doc_off[0] = 0, non-decreasing, doc_off[D] = E: the
 * tokens of document d are [doc_off[d], doc_off[d + 1])), n_aids, min_aid >= 0. A token with aid < min_aid is dropped
 * (min_aid = 10 is the effect of scikit-learn's default token_pattern on decimal aids: one-character tokens never enter
 * the vocabulary; min_aid = 0 keeps everything). The document-term matrix has one entry per (document, distinct kept
 * aid): row_off int64 [D + 1] is the scan of the entries per document, col int32 [nnz] the aids, ascending inside each
 * row, tf int32 [nnz] the number of tokens of that aid in the document, df int32 [n_aids] the number of documents that
 * hold the aid (0 below min_aid). Documents of any length are taken. A token whose aid lies outside [0, n_aids) is
 * refused: -22, h_err[0] = the smallest such token index (h_err[0] = -1 otherwise).
 *
 * WEIGHTS. For every entry i of row r, in column order: w_i = tf_i * idf[col_i]; ss = 0.0, then ss = ss + w_i * w_i for
 * i ascending; norm = sqrt(ss); val_i = w_i / norm, or 0.0 for every entry of a row whose norm is 0. idf float64 [n_cols]
 * is an INPUT (the Python side computes log((1 + D) / (1 + df)) + 1 with NumPy from the device's df, so one libm serves
 * the product and the restatement). With idf == NULL the call takes w_i = val_i as it stands and writes the re-normalised
 * row back in place (tf is not read): the step the aid direction needs after the transpose.
 *
 * TRANSPOSE. CSR (off int64 [R + 1], idx int32 [nnz], val float64 [nnz]) of an R x C matrix -> CSR (t_off int64 [C + 1],
 * t_idx, t_val) of its transpose; every output row's indices ascend; the values are bit copies.
 *
 * COSINE TOP-K. Inputs: A (CSR, R x C, column indices ascending inside each row, rows of unit norm or zero), AT = its
 * transpose (CSR, C x R, with values), queries int32 [nq] (row ids of A; repeats allowed), 1 <= k <= OTTO_TFIDF_MAX_K,
 * exclude_self in {0, 1}. For a query q and every row j that shares a column with q,
 *     s(q, j) = fold over the shared columns c IN ASCENDING ORDER of  s = s + A[q, c] * A[j, c],  starting from s = 0.0.
 * Kept: the rows with s > 0 (and j != q when exclude_self is set), ordered by (s descending, j ascending), the first k.
 * Outputs: ids int32 [nq, k] padded with -1, sim float64 [nq, k] padded with 0.0, n int32 [nq] the number kept.
 * A query id outside [0, R) is found on the device: its output row comes back empty (n = 0), every other row is
 * complete, and the call returns -22 after the stream has drained, with h_err[0] = the smallest offending position in
 * queries (h_err[0] = -1 otherwise). A and AT are trusted to be each other's transpose (they come from the calls
 * above); an index of theirs outside its range is skipped, never followed.
 *
 * Not built (refused by the Python side's argument checks): sublinear_tf, norm = 'l1', use_idf = False, max_df / min_df /
 * max_features, n-grams.
 *
 * Kernels (csrc/otto_tfidf.hip). COUNT / FILL: keys (document << 32 | aid) of the kept tokens, the stable radix sort of
 * radix.h, head flags and their scan -- no per-workgroup tile, so no document is too long. TRANSPOSE: the same sort over
 * (column << 32 | row). WEIGHTS: one wave per row, the sum of squares folded in column order. COSINE: a plan kernel (one
 * wave per query) bounds the query's candidates by the sum of the AT row lengths over its columns and files it in the
 * small tier (bound <= OTTO_TFIDF_SMALL_CAP: one wave, accumulators in an LDS hash table of 2 * OTTO_TFIDF_SMALL_CAP
 * slots) or the large tier (one 256-thread workgroup, accumulators in a dense float64 [R] array of the workspace, one per
 * resident workgroup, cleared by the workgroup itself before its first query). Both tiers take q's columns one at a
 * time in ascending order, add the column's postings to the accumulators (within one column every row occurs once, so
 * no two lanes meet), and put a barrier between two columns: that is SPEC's order, without atomics on the sums. No
 * kernel waits for another workgroup; every loop is bounded by a length read from the offsets or by the table's
 * capacity.
 *
 * Conventions as in otto_rows.h / otto_pqwrite.h: 0 / negative code + otto_last_error(); the caller owns every buffer;
 * d_* are device pointers, h_* host pointers; all arguments travel in one record and the caller's hipStream_t rides in it
 * (the calling guarantees -- side stream, late inputs, reused scratch -- are tested in tests/test_tfidf_gpu.py). count,
 * transpose and cosine_topk synchronise the stream once each, to read their counters and error words; fill and weights
 * only enqueue.
 */
#ifndef OTTO_TFIDF_H
#define OTTO_TFIDF_H

#include <stdint.h>

#define OTTO_TFIDF_MAX_K 64
#define OTTO_TFIDF_SMALL_CAP 512        /* candidate bound up to which a query runs in the one-wave LDS tier */
#define OTTO_TFIDF_MAX_GROUPS 128       /* resident workgroups of the large tier, each with a dense accumulator row */
#define OTTO_TFIDF_SMALL_GRID 1024      /* workgroups (of four one-query waves) the small tier launches at most */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const int32_t* d_tok_aid;  /* E */
    const int64_t* d_doc_off;  /* D + 1 */
    int64_t n_tokens;          /* E, 0 .. 2^31 - 1 */
    int64_t n_docs;            /* D, 0 .. 2^31 - 2 */
    int64_t n_aids;            /* 0 .. 2^31 - 1 */
    int32_t min_aid;           /* >= 0 */
    int32_t reserved;          /* 0 */
    int64_t* d_row_off;        /* D + 1; count writes it, fill reads nothing of it */
    int32_t* d_df;             /* n_aids; count writes it */
    int32_t* d_col;            /* nnz; fill writes it */
    int32_t* d_tf;             /* nnz; fill writes it */
    int64_t nnz;               /* what count returned (fill writes no entry past it) */
    void* d_work;              /* fill reads what count left here: the same bytes, untouched in between */
    int64_t work_bytes;
    void* stream;              /* the caller's hipStream_t; every launch and copy goes there */
} otto_tfidf_fit_job;

/* Bytes of scratch count and fill need (d_work and work_bytes are not looked at), or -22. Host only. */
int64_t otto_tfidf_fit_workspace(const otto_tfidf_fit_job* job);
/* SPEC-TFIDF COUNT. *h_nnz = the number of entries. h_err: one int64 (above). Synchronises the stream once. */
int otto_tfidf_count(const otto_tfidf_fit_job* job, int64_t* h_nnz, int64_t* h_err);
/* SPEC-TFIDF FILL, after a count of the same job on the same stream. Enqueues only. */
int otto_tfidf_fill(const otto_tfidf_fit_job* job);

typedef struct {
    const int64_t* d_row_off;  /* n_rows + 1 */
    const int32_t* d_col;      /* nnz; each < n_cols */
    const int32_t* d_tf;       /* nnz; NULL with d_idf == NULL */
    const double* d_idf;       /* n_cols, or NULL: re-normalise d_val in place */
    double* d_val;             /* nnz */
    int64_t n_rows;
    int64_t n_cols;
    void* stream;
} otto_tfidf_weights_job;

/* SPEC-TFIDF WEIGHTS. Needs no scratch. Enqueues only. */
int otto_tfidf_weights(const otto_tfidf_weights_job* job);

typedef struct {
    const int64_t* d_off;      /* n_rows + 1 */
    const int32_t* d_idx;      /* nnz; each in [0, n_cols) */
    const double* d_val;       /* nnz */
    int64_t n_rows;            /* 0 .. 2^31 - 1 */
    int64_t n_cols;            /* 0 .. 2^31 - 1 */
    int64_t nnz;               /* 0 .. 2^32 - 1 */
    int64_t* d_t_off;          /* n_cols + 1 */
    int32_t* d_t_idx;          /* nnz */
    double* d_t_val;           /* nnz */
    void* d_work;
    int64_t work_bytes;
    void* stream;
} otto_tfidf_transpose_job;

int64_t otto_tfidf_transpose_workspace(const otto_tfidf_transpose_job* job);
/* SPEC-TFIDF TRANSPOSE. h_err[0] = the smallest entry whose index lies outside [0, n_cols) (-22), else -1. Synchronises
 * the stream once. */
int otto_tfidf_transpose(const otto_tfidf_transpose_job* job, int64_t* h_err);

typedef struct {
    const int64_t* d_a_off;    /* A: n_rows + 1 */
    const int32_t* d_a_idx;
    const double* d_a_val;
    const int64_t* d_t_off;    /* AT: n_cols + 1 */
    const int32_t* d_t_idx;
    const double* d_t_val;
    int64_t n_rows;            /* R, 0 .. 2^31 - 1 */
    int64_t n_cols;            /* C, 0 .. 2^31 - 1 */
    const int32_t* d_queries;  /* nq */
    int64_t n_queries;         /* 0 .. 2^31 - 1 */
    int32_t k;                 /* 1 .. OTTO_TFIDF_MAX_K */
    int32_t exclude_self;      /* 0 or 1 */
    int32_t* d_ids;            /* nq * k */
    double* d_sim;             /* nq * k */
    int32_t* d_n;              /* nq */
    void* d_work;
    int64_t work_bytes;
    void* stream;
} otto_tfidf_cosine_job;

int64_t otto_tfidf_cosine_workspace(const otto_tfidf_cosine_job* job);
/* SPEC-TFIDF COSINE TOP-K. h_err: one int64 (above). Synchronises the stream once. */
int otto_tfidf_cosine_topk(const otto_tfidf_cosine_job* job, int64_t* h_err);

#ifdef __cplusplus
}
#endif
#endif
