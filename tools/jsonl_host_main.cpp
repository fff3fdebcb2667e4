// SPEC-JSONL (include/otto_jsonl.h) on the CPU with the piece functions the kernels run (csrc/jsonl_parse.h): reads a file,
// finds every piece the way k_jsonl_parse does (jsonl_piece_kind at every byte), parses the pieces one after the other and
// prints the arrays or the smallest violating line. Stand-alone, so it can be built with the sanitizers
// (tests/test_jsonl_cpu.py: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined); the buffer is
// allocated at exactly the file's size, so a read outside [0, n_bytes) is an error there.
//
//   jsonl_host_main LINE0 FILE...
//   -> per file "ERR <line> <reason>"  or  "OK <S> <E>" and six lines: sess_id, sess_off, session, aid, ts, type
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jsonl_parse.h"

template <typename T>
static void print_row(const std::vector<T>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %lld" : "%lld", (long long)v[i]);
    std::printf("\n");
}

static int run(const char* path, long long line0) {
    std::FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::perror(path);
        return 2;
    }
    std::fseek(f, 0, SEEK_END);
    const int64_t n = (int64_t)std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    uint8_t* p = n ? new uint8_t[(size_t)n] : nullptr;
    if (n && std::fread(p, 1, (size_t)n, f) != (size_t)n) {
        std::fprintf(stderr, "short read\n");
        return 2;
    }
    std::fclose(f);

    std::vector<int64_t> sess_id, sess_off, session, aid, ts, type;
    long long newlines = 0, bad_line = -1;
    int bad_reason = JSONL_OK;
    for (int64_t pos = 0; pos < n; ++pos) {
        if (p[pos] == '\n') {
            ++newlines;
            continue;
        }
        const int kind = jsonl_piece_kind(p, pos, n);
        if (kind != jsonl_piece_kind_after(p, pos, n, pos ? p[pos - 1] : '\n', p[pos])) {       // the form the kernels call
            std::fprintf(stderr, "%s: the two piece classifiers differ at byte %lld\n", path, (long long)pos);
            return 3;
        }
        int reason = JSONL_OK;
        if (kind == JSONL_LEAD) {
            reason = jsonl_parse_lead(p, pos, n);
        } else if (kind == JSONL_HEADER) {
            uint32_t s = 0;
            reason = jsonl_parse_header(p, pos, n, &s);
            sess_id.push_back(s);
            sess_off.push_back((int64_t)aid.size());
        } else if (kind == JSONL_EVENT) {
            uint32_t a = 0;
            int64_t t = 0;
            uint8_t y = 0;
            reason = jsonl_parse_event(p, pos, n, &a, &t, &y);
            session.push_back(sess_id.empty() ? 0 : sess_id.back());
            aid.push_back(a);
            ts.push_back(t);
            type.push_back(y);
        }
        if (reason != JSONL_OK && bad_line < 0) {         // pieces come in file order: the first one is the smallest line
            bad_line = line0 + newlines + 1;
            bad_reason = reason;
        }
    }
    sess_off.push_back((int64_t)aid.size());
    delete[] p;
    if (bad_line >= 0) {
        std::printf("ERR %lld %s\n", bad_line, jsonl_reason(bad_reason));
        return 0;
    }
    std::printf("OK %zu %zu\n", sess_id.size(), aid.size());
    print_row(sess_id);
    print_row(sess_off);
    print_row(session);
    print_row(aid);
    print_row(ts);
    print_row(type);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s LINE0 FILE...\n", argv[0]);
        return 2;
    }
    const long long line0 = std::atoll(argv[1]);
    for (int i = 2; i < argc; ++i)
        if (int rc = run(argv[i], line0)) return rc;
    return 0;
}
