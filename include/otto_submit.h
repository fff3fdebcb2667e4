/*
 * otto_submit.h -- C-ABI of the two ends of the output path: the submission text (per-session top lists -> the bytes of the
 * `session_type,labels` CSV) and the most-frequent-aid statistics (event columns -> per-type counts and their top k).
 * DESIGN.md section 3j.
 *
 * Reference code replaced: the row loops and DataFrame.to_csv of src/ranker/inference.py:403-408,566-572 and
 * src/covisitation/inference.py:387-391,437-447; src/baseline/frequency_statistics.py. Host restatement:
 * tests/submit_restatement.py.
 *
 * SPEC-SUBMIT (normative)
 * -----------------------
 * Input: T in 1..3 tables over one list of S sessions. Table t has a type code c_t in {0, 1, 2} (suffix `_clicks`,
 * `_carts`, `_orders`), rows d_top_aid_t int32 [S] of stride ld >= k (1 <= k <= OTTO_SUBMIT_MAX_K) and d_n_t int32 [S];
 * d_session_id int32 [S] is shared. Line (s, t) has the index t * S + s (interleave == 0: one block per table, the blend
 * script's order) or s * T + t (interleave != 0: the covisitation script's T lines per session). With n = d_n_t[s]:
 *
 *   n >= 0:  <session>_<suffix>,<aid_0> <aid_1> ... <aid_{n-1}>\n      decimal, no sign, no leading zeros; 0 is `0`
 *   n == 0:  <session>_<suffix>,\n                                     (pandas writes the empty field bare)
 *   n <  0:  no line at all, and the session is not examined            (recency_predictions marks the other branch so)
 *
 * The bytes are those of pandas.DataFrame({'session_type', 'labels'}).to_csv(index=False) without its header line.
 * Entries of a row at and past n are never read as values: -1 padding there is no error.
 * Violations: n > k, a negative session id, a negative aid among the first n. They are found on the device; the call
 * returns -22 after the stream has drained and otto_last_error() names the smallest violating line index. A violating
 * line has length 0 in the offsets.
 *
 * Byte offsets are int64 throughout: a full test set is about 0.9 GB, and k = 64 passes 2^31.
 *
 * Frequency lists: ties of the count are ordered by ascending aid. That is this project's choice; the reference's
 * sort_values(ascending=False) leaves ties in an unpinned order.
 *
 * Conventions as in otto_jsonl.h: 0 / negative code + otto_last_error(); caller owns every buffer; d_* are device
 * pointers, h_* host pointers (h_d_* a host array of device pointers); launches go to the caller's hipStream_t.
 * otto_submit_workspace, the one function without a stream parameter, runs on the host and enqueues nothing.
 */
#ifndef OTTO_SUBMIT_H
#define OTTO_SUBMIT_H

#include <stdint.h>

#define OTTO_SUBMIT_MAX_K 64       /* OTTO_FOREST_MAX_K */
#define OTTO_SUBMIT_MAX_TABLES 3
#define OTTO_SUBMIT_LINES 32       /* consecutive lines one workgroup of otto_submit_format owns */

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of scratch otto_submit_measure / otto_submit_format need for S sessions and T tables: 12 bytes per line */
int64_t otto_submit_workspace(int64_t S, int32_t T);

/* Lengths of all S * T lines (one lane per (line, slot)) and their exclusive scan, int64 [S * T + 1], into the
 * workspace; *h_bytes = the total. S == 0 is legal: *h_bytes = 0. Synchronises the stream once. */
int otto_submit_measure(int32_t T, const int32_t* const* h_d_top_aid, const int32_t* const* h_d_n, const int32_t* h_type,
                        const int32_t* d_session_id, int64_t S, int32_t k, int64_t ld, int32_t interleave, int64_t* h_bytes,
                        void* d_work, int64_t work_bytes, void* stream);

/* Write the lines to d_out[first_byte .. first_byte + total), total as otto_submit_measure returned it for the same
 * inputs and the same workspace on this stream (the workspace must be untouched in between). d_out is 16-byte aligned,
 * first_byte >= 0 is any value: a header or an earlier block may precede. first_byte + total > out_bytes is -22 and
 * nothing is written. No byte outside [first_byte, first_byte + total) is written for any input, and a workspace that
 * does not hold the offsets of these inputs is -22. Synchronises the stream once, at the end. */
int otto_submit_format(int32_t T, const int32_t* const* h_d_top_aid, const int32_t* const* h_d_n, const int32_t* h_type,
                       const int32_t* d_session_id, int64_t S, int32_t k, int64_t ld, int32_t interleave, uint8_t* d_out,
                       int64_t out_bytes, int64_t first_byte, void* d_work, int64_t work_bytes, void* stream);

/* d_count u32 [3, n_aids] += the events of this call: d_count[type * n_aids + aid] += 1, one integer atomic per event.
 * The caller zeroes d_count before the first call; train and then test give the reference's "all" lists. An aid >= n_aids
 * or a type > 2 is -22 (the smallest such event index is named; the counts are then unspecified). E == 0 is legal.
 * Synchronises the stream once. */
int otto_freq_count(const uint32_t* d_aid, const uint8_t* d_type, int64_t E, int64_t n_aids, uint32_t* d_count, void* stream);

/* The k (<= OTTO_SUBMIT_MAX_K) most frequent aids of d_count u32 [3, n_aids], by (count descending, aid ascending):
 * row 0 all types together (the sum of the three rows, formed in 64 bits at selection time), rows 1..3 clicks, carts,
 * orders. d_top_aid i32 [4, k] (-1 padded), d_top_count i64 [4, k] (0 padded), d_n i32 [4]: aids of count 0 are never
 * listed, so d_n[r] may be < k. Does not synchronise the stream. */
int otto_freq_topk(const uint32_t* d_count, int64_t n_aids, int32_t k, int32_t* d_top_aid, int64_t* d_top_count, int32_t* d_n,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
