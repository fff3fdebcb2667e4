/*
 * otto_jsonl.h -- C-ABI of the device-side JSONL ingest: the raw session files (train.jsonl / test.jsonl) -> the event
 * columns otto_events_sort takes.
 *
 * Reference code replaced: create_dataframe of utilities/dataset_writer_pickle.py:11-65 (pd.read_json(lines=True) and a
 * Python loop over every event); host restatement: tests/jsonl_restatement.py.
 *
 * SPEC-JSONL (normative)
 * ----------------------
 * Input is a byte buffer holding whole lines. Lines end in '\n'; the last line of a buffer may lack it. `ws` is any run
 * of space, tab and '\r'. A line of ws only is skipped. Every other line must match exactly
 *
 *   ws { ws "session" ws : ws INT ws , ws "events" ws : ws [ ws ( EVENT ( ws , ws EVENT )* ws )? ] ws } ws
 *   EVENT  := { ws MEMBER ws , ws MEMBER ws , ws MEMBER ws }     the three keys "aid", "ts", "type", each once, any order
 *   MEMBER := "aid" ws : ws INT | "ts" ws : ws INT | "type" ws : ws ( "clicks" | "carts" | "orders" )
 *   INT    := 0 | [1-9][0-9]*         session, aid <= 2^32 - 1;  ts <= 2^63 - 1
 *
 * The top-level key order is fixed (session, then events: the dataset's own order and DataFrame.to_json(lines=True)'s).
 * Violations: a sign, fraction, exponent, leading zero, overflow or escape; any other key, type string or byte (bytes
 * >= 0x80 and a BOM included); a duplicate or missing key; a trailing or missing comma; nesting; a line cut short by the
 * end of the buffer.
 *
 * A "piece" is one of three spans: a line's leading ws (the whole of a blank line); the header, from the line's '{' up
 * to the first event or, without events, to the line end; one event, from its '{' up to the next event's '{' or the line
 * end. The line end is the position of the '\n' or the end of the buffer, so the last piece of a line holds the closing
 * "]}" and the trailing ws. A piece longer than OTTO_JSONL_MAX_PIECE bytes is a violation too: it bounds how far a thread
 * reads past its tile.
 *
 * Outputs, in file order: per event session u32, aid u32, ts i64 (as written, not divided), type u8 (0 clicks / 1 carts /
 * 2 orders); per non-blank line sess_id u32 [S]; the CSR sess_off i64 [S + 1]. A line with "events":[] is a session row
 * without events (the reference's loop drops it from the frame, and so does otto_events_sort).
 *
 * On a violation the call returns -22 after the stream has drained; otto_last_error() names the 1-based number of the
 * smallest violating line (line0 + the newlines before it + 1) and a short reason; the outputs' contents are then
 * unspecified. No read leaves [0, n_bytes) for any input whatever, and no write leaves the stated capacities.
 *
 * Conventions as in otto_events.h: 0 / negative code + otto_last_error(); caller owns every buffer; d_* are device
 * pointers, h_* host pointers; launches go to the caller's hipStream_t. d_bytes must be 16-byte aligned.
 * otto_jsonl_workspace, the one function without a stream parameter, runs on the host and enqueues nothing.
 */
#ifndef OTTO_JSONL_H
#define OTTO_JSONL_H

#include <stdint.h>

#define OTTO_JSONL_MAX_PIECE 256   /* longest legal piece, bytes; also the halo a tile's workgroup reads past its tile */
#define OTTO_JSONL_TILE 4096       /* bytes of input per workgroup */

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of scratch otto_jsonl_count / otto_jsonl_parse need for n_bytes of input: O(n_bytes / OTTO_JSONL_TILE) */
int64_t otto_jsonl_workspace(int64_t n_bytes);

/* h_counts[0] = S, the non-blank lines, h_counts[1] = E, the events, of d_bytes[0 .. n_bytes), n_bytes in [0, 2^31):
 * the capacities otto_jsonl_parse needs. Counts only -- nothing is validated; on an input that otto_jsonl_parse refuses
 * the two numbers are still the ones that call works with. Synchronises the stream once. */
int otto_jsonl_count(const uint8_t* d_bytes, int64_t n_bytes, int64_t* h_counts, void* d_work, int64_t work_bytes, void* stream);

/* Parse and validate d_bytes[0 .. n_bytes) by SPEC-JSONL. line0: the number of lines that precede the buffer in its file
 * (error messages only).
 *   out: d_session u32[cap_events], d_aid u32[cap_events], d_ts i64[cap_events], d_type u8[cap_events]: first E valid;
 *        d_sess_off i64[cap_sessions + 1]: first S + 1 valid; d_sess_id u32[cap_sessions]: first S valid;
 *        h_counts[0] = S, h_counts[1] = E.
 * S > cap_sessions or E > cap_events is -22 (nothing is written past a capacity). n_bytes == 0 is legal: S = E = 0 and
 * sess_off[0] = 0. Synchronises the stream once. */
int otto_jsonl_parse(const uint8_t* d_bytes, int64_t n_bytes, int64_t line0, int64_t cap_sessions, int64_t cap_events,
                     uint32_t* d_session, uint32_t* d_aid, int64_t* d_ts, uint8_t* d_type, int64_t* d_sess_off,
                     uint32_t* d_sess_id, int64_t* h_counts, void* d_work, int64_t work_bytes, void* stream);

/* *h_newlines = the number of '\n' in the n_bytes of input of the last otto_jsonl_count / otto_jsonl_parse call that ran
 * with this workspace on this stream (what a chunked reader adds to line0 for its next chunk). */
int otto_jsonl_newlines(const void* d_work, int64_t work_bytes, int64_t n_bytes, int64_t* h_newlines, void* stream);

#ifdef __cplusplus
}
#endif
#endif
