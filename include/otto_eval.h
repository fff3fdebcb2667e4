/*
 * otto_eval.h -- C-ABI of the validation split, the ground-truth labels and the recall@20 hit counts (SPEC-EVAL,
 * DESIGN.md section 3f).
 *
 * What this replaces in the reference: src/validation.py (the per-session cutoff, :71-85, and get_labels, :9-52) and the
 * recall loops of src/ranker/inference.py:176-180, 248-250, 317-322, src/ranker/lgb_trainer.py:190-197 and
 * src/ranker/covisitation_candidate_generation.py:159-164.
 *
 * Conventions of otto_blend.h: 0 or a negative OTTO_E* code plus otto_last_error; caller-owned buffers; the caller
 * supplies the workspace, sized by the *_workspace function (256-byte aligned); no allocation per call (error words,
 * list lengths and totals live in a 256-byte per-device scratch the library keeps); all device work on the caller's
 * stream; a call synchronises the stream at most once, stated per function. Everything is integer work.
 * The functions without a stream parameter (the two *_workspace sizes) run on the host and enqueue nothing.
 *
 * SPEC-EVAL.
 *
 * Events: aid int32 >= 0, ts int32, typ uint8 in {0 clicks, 1 carts, 2 orders}, sess_off int64 [S+1] (session s owns
 * events [sess_off[s], sess_off[s+1]), n = its length), events of a session in (ts, original order) order. S < 2^31.
 * A typ outside 0..2 is refused with OTTO_EINVAL, detected on the device; no input is ever written.
 *
 * 1. last_click[s] = the largest in-session index i with typ == 0, or -1.
 *    cutoff[s] = 0 when n == 2; 0 when last_click <= 0; else ((h >> 32) * last_click) >> 32 with
 *        h = mix64(mix64(seed) ^ (s * 0xA0761D6478BD642F)),   all in uint64, s = the session's position,
 *        mix64(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                  z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)     (the BPR sampler's hash)
 *    so it is uniform in [0, last_click). The reference raises for a click-free session with n != 2; here its cutoff is
 *    0 and the number of such sessions comes back in *h_n_without_click.
 *    Any caller-made cutoff with 0 <= cutoff[s] < max(n, 1) is valid for the split; anything else is OTTO_EINVAL.
 *
 * 2. Split at cutoff: events 0..cutoff[s] of every session are kept (none when n == 0), in order, with their own
 *    sess_off. Labels are over the tail cutoff[s]+1 .. n-1, as three CSR lists (off int64 [S+1], aid int32):
 *    clicks = the aid of the earliest click of the tail (length 0 or 1); carts = the distinct aids with typ == 1 in
 *    ascending order; orders = the same for typ == 2. No limit on session or tail length.
 *
 * 3. Hits of one event type. Label session j carries labels label_aid[label_off[j] .. label_off[j+1]) (any order,
 *    duplicates allowed) and the id label_session[j] (ascending and distinct; NULL: the id is j). Prediction row p is
 *    either padded (d_pred_off == NULL: d_pred_aid [P, k], 1 <= k <= 64, the first d_pred_n[p] entries, all k when
 *    d_pred_n == NULL) or CSR (d_pred_aid[d_pred_off[p] .. d_pred_off[p+1]), any length). It belongs to session
 *    d_pred_session[p] (ascending and distinct), or to label session p when d_pred_session == NULL (then P == S).
 *    Only the first cap entries of a row count (cap <= 0: all); a negative entry is padding and is skipped.
 *    A d_pred_session that is no label session is OTTO_EINVAL. A label session without a row has 0 hits.
 *        hits[j]  = |distinct(row[:cap]) n distinct(labels)|        denom[j] = min(number of labels as listed, 20)
 *    h_totals = {sum hits, sum denom, sum hits where mask, sum denom where mask} (the last two 0 without a mask).
 */
#ifndef OTTO_EVAL_H
#define OTTO_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* d_last_click int32 [S]. OTTO_EINVAL for a typ outside 0..2. Synchronises the stream once. */
int otto_eval_last_click(const uint8_t* d_typ, const int64_t* d_sess_off, int64_t S, int32_t* d_last_click, void* stream);

/* d_cutoff int32 [S]; *h_n_without_click = sessions without a click and n != 2 (host pointer, may be NULL).
 * OTTO_EINVAL for a typ outside 0..2. Synchronises the stream once. */
int otto_eval_cutoffs(const uint8_t* d_typ, const int64_t* d_sess_off, int64_t S, uint64_t seed, int32_t* d_cutoff,
                      int64_t* h_n_without_click, void* stream);

/* bytes of workspace the two split calls need for S sessions holding n_events events */
int64_t otto_eval_split_workspace(int64_t S, int64_t n_events);

/* Count pass and scans. Writes the four CSR offset arrays, each int64 [S+1]: d_out_sess_off (kept events),
 * d_click_off, d_cart_off, d_order_off; h_counts[4] (host) = their totals: kept events, click, cart, order labels.
 * OTTO_EINVAL (outputs undefined) for a typ outside 0..2 or a cutoff outside [0, max(n, 1)).
 * Synchronises the stream once. */
int otto_eval_split_count(const int32_t* d_aid, const uint8_t* d_typ, const int64_t* d_sess_off, int64_t S, int64_t n_events,
                          const int32_t* d_cutoff, int64_t* d_out_sess_off, int64_t* d_click_off, int64_t* d_cart_off,
                          int64_t* d_order_off, int64_t* h_counts, void* d_workspace, int64_t workspace_bytes, void* stream);

/* Emit pass: the same inputs and the four offset arrays otto_eval_split_count wrote; writes the kept events
 * (d_out_aid, d_out_ts, d_out_typ: h_counts[0] entries) and the label aids (h_counts[1..3] entries). The workspace
 * need not be the one of the count pass. No synchronisation. */
int otto_eval_split(const int32_t* d_aid, const int32_t* d_ts, const uint8_t* d_typ, const int64_t* d_sess_off, int64_t S, int64_t n_events,
                    const int32_t* d_cutoff, const int64_t* d_out_sess_off, const int64_t* d_click_off,
                    const int64_t* d_cart_off, const int64_t* d_order_off, int32_t* d_out_aid, int32_t* d_out_ts,
                    uint8_t* d_out_typ, int32_t* d_click_aid, int32_t* d_cart_aid, int32_t* d_order_aid, void* d_workspace,
                    int64_t workspace_bytes, void* stream);

/* bytes of workspace otto_eval_hits needs for S label sessions */
int64_t otto_eval_hits_workspace(int64_t S);

/* d_hits / d_denom int32 [S]; h_totals int64 [4] (host); d_mask uint8 [S] or NULL. OTTO_EINVAL (outputs undefined) for a
 * foreign prediction session or ids that are not ascending and distinct. Synchronises the stream once. */
int otto_eval_hits(const int32_t* d_label_session, const int64_t* d_label_off, const int32_t* d_label_aid, int64_t S,
                   const int32_t* d_pred_aid, const int32_t* d_pred_n, const int64_t* d_pred_off, int32_t k, int64_t P,
                   const int32_t* d_pred_session, int32_t cap, const uint8_t* d_mask, int32_t* d_hits, int32_t* d_denom,
                   int64_t* h_totals, void* d_workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
