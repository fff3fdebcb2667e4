// Byte-level piece parsers of SPEC-JSONL (include/otto_jsonl.h), as host/device functions: the kernels of otto_jsonl.hip
// run them on a tile staged in LDS, tools/jsonl_host_main.cpp runs the same code on the CPU under the sanitizers.
//
// Every function works on p[0 .. n): `begin` is the first byte of the piece, n the end of the buffer in p's index space.
// No byte at or past min(n, begin + OTTO_JSONL_MAX_PIECE + 1) is read, none before `begin` except by jsonl_piece_kind,
// which looks back over at most OTTO_JSONL_MAX_PIECE bytes and never below 0.
#pragma once
#include <stdint.h>
#include "../../include/otto_jsonl.h"

#if defined(__HIPCC__)
#define OTTO_JSONL_HD __host__ __device__ __forceinline__
#else
#define OTTO_JSONL_HD static inline
#endif

enum { JSONL_NONE = 0, JSONL_LEAD = 1, JSONL_HEADER = 2, JSONL_EVENT = 3 };                 // piece kinds
enum { JSONL_OK = 0, JSONL_E_BYTE, JSONL_E_NUMBER, JSONL_E_RANGE, JSONL_E_KEY, JSONL_E_TYPE, JSONL_E_TRUNC, JSONL_E_LONG,
       JSONL_N_REASONS };

static inline const char* jsonl_reason(int r) {
    static const char* const names[JSONL_N_REASONS] = {
        "no violation", "unexpected byte", "malformed number (sign, fraction, exponent or leading zero)", "number out of range",
        "unknown, duplicate or missing key", "unknown event type", "line cut short by the end of the buffer",
        "piece longer than OTTO_JSONL_MAX_PIECE bytes"};
    return r >= 0 && r < JSONL_N_REASONS ? names[r] : "?";
}

OTTO_JSONL_HD bool jsonl_is_ws(int b) { return b == ' ' || b == '\t' || b == '\r'; }

// Which piece starts at p[pos], pos in [0, n). A '{' whose preceding non-ws byte is the line start opens a header, any
// other '{' an event; a line start that holds neither '{' nor '\n' opens the leading ws. Within a valid line no string
// holds a brace, and each parser below refuses a '{' anywhere but at the end of its span, so the pieces found here tile
// every line that the parsers accept. A ws run longer than MAX_PIECE makes the piece that holds it a violation, so the
// look-back may stop there.
OTTO_JSONL_HD int jsonl_piece_kind(const uint8_t* p, int64_t pos, int64_t n) {
    (void)n;
    const int b = p[pos];
    if (b == '{') {
        int64_t j = pos - 1;
        const int64_t stop = pos - OTTO_JSONL_MAX_PIECE > 0 ? pos - OTTO_JSONL_MAX_PIECE : 0;
        while (j >= stop && jsonl_is_ws(p[j])) --j;
        return (j < 0 || p[j] == '\n') ? JSONL_HEADER : JSONL_EVENT;
    }
    if (b != '\n' && (pos == 0 || p[pos - 1] == '\n')) return JSONL_LEAD;
    return JSONL_NONE;
}

// jsonl_piece_kind for a caller that holds the byte b = p[pos] and the byte in front of it (prev; '\n' at pos 0): memory
// is touched only for a '{' behind ws
OTTO_JSONL_HD int jsonl_piece_kind_after(const uint8_t* p, int64_t pos, int64_t n, int prev, int b) {
    if (b == '\n') return JSONL_NONE;
    if (b == '{') return jsonl_is_ws(prev) ? jsonl_piece_kind(p, pos, n) : prev == '\n' ? JSONL_HEADER : JSONL_EVENT;
    return prev == '\n' ? JSONL_LEAD : JSONL_NONE;
}

struct jsonl_cur {
    const uint8_t* p;
    int64_t i, limit;
    bool eof;          // limit is the end of the buffer
    int err;
};

OTTO_JSONL_HD jsonl_cur jsonl_open(const uint8_t* p, int64_t begin, int64_t n) {
    jsonl_cur c;
    c.p = p;
    c.i = begin;
    c.eof = n - begin <= OTTO_JSONL_MAX_PIECE + 1;
    c.limit = c.eof ? n : begin + OTTO_JSONL_MAX_PIECE + 1;
    c.err = JSONL_OK;
    return c;
}
OTTO_JSONL_HD int jsonl_peek(const jsonl_cur& c) { return c.i < c.limit ? (int)c.p[c.i] : -1; }
OTTO_JSONL_HD void jsonl_fail(jsonl_cur& c, int reason) {
    if (c.err == JSONL_OK) c.err = c.i < c.limit ? reason : (c.eof ? JSONL_E_TRUNC : JSONL_E_LONG);
}
OTTO_JSONL_HD void jsonl_ws(jsonl_cur& c) {
    while (c.i < c.limit && jsonl_is_ws(c.p[c.i])) ++c.i;
}
OTTO_JSONL_HD void jsonl_expect(jsonl_cur& c, int ch, int reason) {
    if (c.err) return;
    if (jsonl_peek(c) == ch) ++c.i;
    else jsonl_fail(c, reason);
}
// ws ch ws
OTTO_JSONL_HD void jsonl_punct(jsonl_cur& c, int ch) {
    jsonl_ws(c);
    jsonl_expect(c, ch, JSONL_E_BYTE);
    jsonl_ws(c);
}
// the rest of a literal, closing quote included
OTTO_JSONL_HD void jsonl_lit(jsonl_cur& c, const char* s, int len, int reason) {
    for (int k = 0; k < len; ++k) jsonl_expect(c, s[k], reason);
}
OTTO_JSONL_HD uint64_t jsonl_int(jsonl_cur& c, uint64_t max) {
    if (c.err) return 0;
    int b = jsonl_peek(c);
    if (b < '0' || b > '9') {
        jsonl_fail(c, b == '-' || b == '+' || b == '.' ? JSONL_E_NUMBER : JSONL_E_BYTE);
        return 0;
    }
    ++c.i;
    uint64_t v = (uint64_t)(b - '0');
    const bool zero = b == '0';
    for (;;) {
        b = jsonl_peek(c);
        if (b < '0' || b > '9') break;
        if (zero) { jsonl_fail(c, JSONL_E_NUMBER); return 0; }        // leading zero
        const uint64_t d = (uint64_t)(b - '0');
        if (v > (max - d) / 10) { jsonl_fail(c, JSONL_E_RANGE); return 0; }
        v = v * 10 + d;
        ++c.i;
    }
    if (b == '.' || b == 'e' || b == 'E') jsonl_fail(c, JSONL_E_NUMBER);
    return v;
}
// ws, then the line end: '\n' or the end of the buffer
OTTO_JSONL_HD void jsonl_eol(jsonl_cur& c) {
    jsonl_ws(c);
    if (c.err) return;
    if (c.i < c.limit) {
        if (c.p[c.i] != '\n') jsonl_fail(c, JSONL_E_BYTE);
    } else if (!c.eof) {
        jsonl_fail(c, JSONL_E_LONG);
    }
}
// ] ws } ws line end
OTTO_JSONL_HD void jsonl_close(jsonl_cur& c) {
    jsonl_expect(c, ']', JSONL_E_BYTE);
    jsonl_punct(c, '}');
    jsonl_eol(c);
}
OTTO_JSONL_HD int jsonl_done(const jsonl_cur& c, int64_t begin) {
    if (c.err) return c.err;
    return c.i - begin > OTTO_JSONL_MAX_PIECE ? JSONL_E_LONG : JSONL_OK;
}

// the leading ws of a line, up to its '{' or, on a blank line, to the line end
OTTO_JSONL_HD int jsonl_parse_lead(const uint8_t* p, int64_t begin, int64_t n) {
    jsonl_cur c = jsonl_open(p, begin, n);
    jsonl_ws(c);
    if (jsonl_peek(c) != '{') jsonl_eol(c);
    return jsonl_done(c, begin);
}

// { ws "session" ws : ws INT ws , ws "events" ws : ws [ ws, then the first event's '{' or ] ws } ws line end
OTTO_JSONL_HD int jsonl_parse_header(const uint8_t* p, int64_t begin, int64_t n, uint32_t* session) {
    jsonl_cur c = jsonl_open(p, begin, n);
    jsonl_expect(c, '{', JSONL_E_BYTE);
    jsonl_ws(c);
    jsonl_expect(c, '"', JSONL_E_BYTE);
    jsonl_lit(c, "session\"", 8, JSONL_E_KEY);
    jsonl_punct(c, ':');
    *session = (uint32_t)jsonl_int(c, 0xFFFFFFFFull);
    jsonl_punct(c, ',');
    jsonl_expect(c, '"', JSONL_E_BYTE);
    jsonl_lit(c, "events\"", 7, JSONL_E_KEY);
    jsonl_punct(c, ':');
    jsonl_expect(c, '[', JSONL_E_BYTE);
    jsonl_ws(c);
    if (!c.err && jsonl_peek(c) != '{') jsonl_close(c);
    return jsonl_done(c, begin);
}

// { ws MEMBER ws , ws MEMBER ws , ws MEMBER ws } ws, then , ws and the next event's '{', or ] ws } ws line end
OTTO_JSONL_HD int jsonl_parse_event(const uint8_t* p, int64_t begin, int64_t n, uint32_t* aid, int64_t* ts, uint8_t* type) {
    jsonl_cur c = jsonl_open(p, begin, n);
    jsonl_expect(c, '{', JSONL_E_BYTE);
    int seen = 0;
    for (int m = 0; m < 3 && !c.err; ++m) {
        jsonl_ws(c);
        jsonl_expect(c, '"', m ? JSONL_E_BYTE : JSONL_E_KEY);
        const int k = jsonl_peek(c);
        int key;
        if (k == 'a') { key = 1; jsonl_lit(c, "aid\"", 4, JSONL_E_KEY); }
        else if (k == 't') {
            ++c.i;
            if (jsonl_peek(c) == 's') { key = 2; jsonl_lit(c, "s\"", 2, JSONL_E_KEY); }
            else { key = 4; jsonl_lit(c, "ype\"", 4, JSONL_E_KEY); }
        } else { key = 0; jsonl_fail(c, JSONL_E_KEY); }
        if (!c.err && (seen & key)) jsonl_fail(c, JSONL_E_KEY);            // duplicate
        seen |= key;
        jsonl_punct(c, ':');
        if (key == 1) *aid = (uint32_t)jsonl_int(c, 0xFFFFFFFFull);
        else if (key == 2) *ts = (int64_t)jsonl_int(c, 0x7FFFFFFFFFFFFFFFull);
        else if (key == 4) {
            jsonl_expect(c, '"', JSONL_E_BYTE);
            const int t = jsonl_peek(c);
            if (t == 'c') {
                ++c.i;
                if (jsonl_peek(c) == 'l') { *type = 0; jsonl_lit(c, "licks\"", 6, JSONL_E_TYPE); }
                else { *type = 1; jsonl_lit(c, "arts\"", 5, JSONL_E_TYPE); }
            } else { *type = 2; jsonl_lit(c, "orders\"", 7, JSONL_E_TYPE); }
        }
        jsonl_punct(c, m < 2 ? ',' : '}');
    }
    if (!c.err) {
        if (jsonl_peek(c) == ',') {
            ++c.i;
            jsonl_ws(c);
            if (jsonl_peek(c) != '{') jsonl_fail(c, JSONL_E_BYTE);
        } else {
            jsonl_close(c);
        }
    }
    return jsonl_done(c, begin);
}
