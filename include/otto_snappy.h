/*
 * otto_snappy.h -- C-ABI of the device-side Snappy encoder: extents of a device buffer -> one Snappy raw-format stream
 * each, the codec of the Parquet pages otto_amd/parquet_write.py writes with compression='snappy' and the counterpart of
 * the decoder of otto_parquet.h (otto_parquet_snappy). DESIGN.md section 2h.
 *
 * Reference code replaced: the Snappy call inside pyarrow behind DataFrame.to_parquet (default compression) of
 * src/covisitation/covisitation.py and src/utilities/split_dataset_writer_parquet.py. Host restatement:
 * tests/snappy_restatement.py, which reads the #defines below.
 *
 * SPEC-SNAPPY (normative)
 * -----------------------
 * Given the bytes x[0, n) of an extent, the bytes of its stream are fully determined.
 *
 * Stream. The ULEB128 of n, then the elements of the extent's fragments in order. A fragment is OTTO_SNAPPY_FRAGMENT =
 * 65,536 input bytes; the last may be short. Fragments are compressed without reference to one another, so every copy
 * offset is below 65,536 and the copy with a 4-byte offset is never written. n = 0 gives the single byte 00. n < 2^32.
 *
 * Matches (positions p count from the fragment's first byte, m its bytes). Every position with p + OTTO_SNAPPY_HASH_BYTES
 * <= m has the slot  ((v * 0x9E3779B97F4A7C15) mod 2^64) >> (64 - OTTO_SNAPPY_HASH_BITS),  v the little-endian value of
 * its first OTTO_SNAPPY_HASH_BYTES bytes. Positions are taken in batches of OTTO_SNAPPY_BATCH = 64 consecutive ones, the
 * first at p = 0. A table of 2^OTTO_SNAPPY_HASH_BITS entries, empty at the start of the fragment, holds per slot the
 * largest position of all EARLIER batches: a batch first reads the table for all its positions, then enters them.
 * The candidates of position p, in this order: p - 1, p - 4, p - 8 (each only if it is >= 0), then the table's entry of
 * its slot as its batch read it (if the position has a slot and the entry is not empty). The length of a candidate c is
 * the number of leading bytes that x[c ...] and x[p ...] share, capped at min(OTTO_SNAPPY_MAX_MATCH = 64, m - p); copies
 * may overlap. The longest candidate wins; on a tie the earliest in the order above. The selection is greedy from p = 0:
 * if the winner's length is at least OTTO_SNAPPY_MIN_MATCH the token is (length, distance p - c) and p advances by the
 * length; otherwise the token is the literal x[p] and p advances by 1. A match never reaches before its fragment's first
 * byte or past its last.
 *
 * Elements. A maximal run of consecutive literal tokens of a fragment becomes one literal element of len bytes: the tag
 * byte (len - 1) << 2 for len <= 60; the tag 60 << 2 and the byte len - 1 for len <= 256; otherwise the tag 61 << 2 and
 * len - 1 in two little-endian bytes; then the bytes. A match token (L, d) is exactly one copy element, because of the cap:
 * the 1-byte-offset form  01 | (L - 4) << 2 | (d >> 8) << 5,  d & 0xFF  when 4 <= L <= 11 and d < 2,048; otherwise the
 * 2-byte-offset form  02 | (L - 1) << 2,  d in two little-endian bytes.
 *
 * Bound. A stream is never longer than 32 + n + n / 6 (otto_snappy_bound): a literal element adds at most 3 bytes to the
 * bytes it carries and follows a copy or starts the fragment; a copy element is shorter than the bytes it stands for.
 *
 * Choice of the parameters (bytes of the stream of each column of tests/snappy_inputs.py columns(): the four chunk-writer
 * columns and the covisitation weights, about 40,000 rows each, synthetic; `python tests/snappy_restatement.py` prints it).
 * LDS is the hash table of one fragment's wave, 4 bytes per entry; a CU has 160 KiB and holds at most 32 waves.
 *   H / MIN_MATCH / bits / near   session      aid       ts     type      wgt    LDS      waves per CU
 *   raw bytes                      159980   159980   319960   159980   159980
 *   pyarrow Codec('snappy')         43279    94964   160080    17499    69104
 *   4 / 4 / 12 / 1,4,8              33639    95231   160707    16478    66880   16 KiB   10
 *   5 / 5 / 12 / 1,4,8              33640    94030   160875    15494    45732   16 KiB   10
 *   6 / 6 / 12 / 1,4,8              33640    96131   161160    15494    44177   16 KiB   10     <- chosen
 *   8 / 8 / 12 / 1,4,8              38283   106669   305853    15470    44403   16 KiB   10
 *   4 / 6 / 12 / 1,4,8              33640   104157   160729    16611    71882   16 KiB   10
 *   6 / 6 / 11 / 1,4,8              33640    99097   162167    15494    46163    8 KiB   20
 *   6 / 6 / 10 / 1,4,8              33640   102829   163966    15494    48104    4 KiB   32
 *   6 / 6 / 13 / 1,4,8              33640    93758   160613    15494    43838   32 KiB    5
 *   6 / 6 / 12 / 1                 117344    96201   162028    15497    44292   16 KiB   10
 * A 4-byte match at a hashed distance costs 3 bytes and breaks a literal run, which is why MIN_MATCH 4 loses on the float
 * column; 6 / 6 is the best setting for it and is the setting of SPEC-DEFLATE. The fixed distances 4 and 8 are the previous
 * value of a 4- and an 8-byte column: without them a column of slowly changing values finds nothing (last row). One more
 * table bit gains 1 % for twice the LDS. Ten waves per CU are 2.5 per SIMD; the plan kernel must not need more than
 * 512 / 3 = 168 VGPRs for the table to be what limits it (it needs 44: profiles/snappy/kernel_resources.txt).
 *
 * Conventions as in otto_submit.h: 0 / negative code + otto_last_error(); the caller owns every buffer; d_* are device
 * pointers, h_* host pointers. All arguments travel in one record, otto_snappy_job, and the caller's hipStream_t rides in
 * it, as in otto_pqw_job (include/otto_pqwrite.h says why); the guarantees of tests/contract_cases.py (side stream, late
 * inputs, reused scratch) are tested for these entry points in tests/test_snappy_gpu.py.
 */
#ifndef OTTO_SNAPPY_H
#define OTTO_SNAPPY_H

#include <stdint.h>

#define OTTO_SNAPPY_FRAGMENT 65536
#define OTTO_SNAPPY_MIN_MATCH 6
#define OTTO_SNAPPY_HASH_BYTES 6
#define OTTO_SNAPPY_HASH_BITS 12
#define OTTO_SNAPPY_BATCH 64
#define OTTO_SNAPPY_MAX_MATCH 64

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const uint8_t* d_in;       /* n_bytes bytes, any alignment */
    int64_t n_bytes;
    const int64_t* src_off;    /* host: stream i compresses d_in[src_off[i] .. + src_len[i]); extents may touch, overlap or leave gaps */
    const int64_t* src_len;    /* host: 0 <= src_len[i] < 2^32 */
    int64_t n_streams;         /* >= 0 */
    void* d_work;
    int64_t work_bytes;
    void* stream;              /* the caller's hipStream_t; every launch and copy goes there */
} otto_snappy_job;

/* the largest stream n bytes can give, 32 + n + n / 6; -1 for a negative n. Host only. */
int64_t otto_snappy_bound(int64_t n);

/* Bytes of scratch the two calls below need for this job (d_work and work_bytes are not looked at): about 1.4 bytes per input
 * byte for the elements, and a few words per fragment and per stream. -22 for a job that breaks a rule above: a null
 * array, a negative count, an extent outside [0, n_bytes) or of 2^32 bytes or more. Host only: enqueues nothing. */
int64_t otto_snappy_workspace(const otto_snappy_job* job);

/* h_stream_bytes[i] = the bytes of stream i. k_snappy_plan, one wave per fragment: the hash table in LDS, 64 positions per
 * batch, the greedy selection on ballot masks, the elements (a literal run or a copy each) and the fragment's size to the
 * workspace; then a scan of the fragment sizes and the size of every stream. Synchronises the stream once. */
int otto_snappy_plan(const otto_snappy_job* job, int64_t* h_stream_bytes);

/* Stream i goes to d_out[h_dst_off[i] .. + its bytes): any byte offsets, the gaps are the caller's. Extents that overlap or
 * leave [0, out_bytes) are -22 before anything is launched, and so are a workspace that does not hold the plan
 * otto_snappy_plan wrote for this very job (same d_in, same extents) and a source extent outside d_in. k_snappy_emit, one
 * wave per fragment: element offsets from a wave scan of the element sizes, literal bytes copied from the input. No global
 * atomic touches d_out, no byte outside a stream's extent is written for any input or workspace content, every byte inside
 * is written exactly once. The input must be the bytes the plan saw. Synchronises the stream. */
int otto_snappy_emit(const otto_snappy_job* job, const int64_t* h_dst_off, uint8_t* d_out, int64_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif
