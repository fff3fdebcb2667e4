/*
 * otto_parquet.h -- C-ABI of the device-side Parquet decode: the split files (DATA/splits/{train,val}.parquet, the 100k-session
 * part files of the chunk writers) -> the event columns otto_events_sort takes.
 *
 * Reference code replaced: the pyarrow / pandas host decode in front of every consumer of the split files
 * (src/ranker/aid_feature_engineering.py:21-36 reads them with pd.read_parquet). The host side (otto_amd/parquet.py) reads
 * the footer and the page headers only; the page bodies cross PCIe as they lie in the file and are unpacked here.
 *
 * SPEC-PARQUET (normative)
 * ------------------------
 * Accepted. Magic "PAR1" at both ends; a Thrift-compact FileMetaData; any number of row groups; requested columns that are
 * top-level primitive leaves with repetition REQUIRED or OPTIONAL (every other column, nested ones included, is skipped by
 * walking num_children); physical types INT32 and INT64; codecs UNCOMPRESSED and SNAPPY. Page types: DICTIONARY_PAGE with
 * encoding PLAIN or the legacy PLAIN_DICTIONARY; DATA_PAGE (V1: the levels are inside the compressed body, the definition
 * levels are RLE with a 4-byte length prefix); DATA_PAGE_V2 (the levels are outside the compressed body, their lengths come
 * from the header, is_compressed is honoured); INDEX_PAGE is skipped. Value encodings: PLAIN; RLE_DICTIONARY /
 * PLAIN_DICTIONARY (one bit-width byte, then RLE / bit-packed hybrid runs, widths 0 to 32, width 0 means every index is 0).
 * DELTA_BINARY_PACKED on data pages of INT32 / INT64 columns ("Delta pages" below). A column chunk may mix delta,
 * dictionary-coded and PLAIN data pages. Page CRCs are not checked.
 *
 * Float columns. The host side reads FLOAT and DOUBLE columns when asked to (floats=True): encodings PLAIN and dictionary,
 * the column record's element size equals the physical size, no zero extension, so every value is a bit copy. A delta-coded
 * page of such a column is refused on the host by name.
 *
 * Delta pages. Behind the levels the body holds ULEB128 B (values per block), ULEB128 M (miniblocks per block), ULEB128 n
 * (values) and the zigzag ULEB128 first value. Accepted: B a multiple of 128 with 128 <= B <= 65536, M >= 1, B % M == 0,
 * B / M a multiple of 32 (pyarrow writes 128, 4 for INT32 and 256, 4 for INT64; the project's writer 128, 4 for both). n must
 * equal the page's non-null value count; n == 0 is a page of its header alone, n == 1 ends behind the first value. The
 * n - 1 deltas come in blocks of B: a zigzag ULEB128 min_delta, M width bytes, then the miniblocks, each B / M fields of its
 * width packed LSB-first. A width above 8 x the physical size is refused. The last miniblock that holds a delta is stored
 * whole; miniblocks behind it have no bytes and their width bytes are ignored whatever they hold. A varint of more than 10
 * bytes, or one whose tenth byte carries bits above 2^64, is refused. Arithmetic: v[i] = v[i-1] + min_delta + field, modulo
 * 2^(8 x physical size); then the widening and the cast of "Output dtype" apply. Extent: the stream must end exactly at the
 * body's end; running past it and a single trailing byte are each refused with a reason of their own. No byte outside the
 * body is read -- a field is fetched through the bytes that hold its bits and no others -- and nothing outside the page's rows
 * of its column is written.
 *
 * Refused, each with an error that names the file, the column, the row group and, where it applies, the page ordinal and a
 * reason: an encrypted footer ("PARE"); any other physical type, codec or encoding (named in the message); a repeated or
 * nested requested column; a null (V2: num_nulls != 0, refused on the host; V1: the device counts the definition levels
 * equal to 1 and the count must equal num_values); a dictionary index >= the dictionary's size; a page whose decoded size
 * differs from its header; any Snappy violation; any violation of "Delta pages"; a row group whose requested columns disagree
 * on num_rows.
 *
 * Snappy. The preamble varint must equal the size the page header declares. Every element is checked BEFORE any of its
 * bytes is touched: the tag and its length / offset bytes and a literal's bytes against the compressed extent; the bytes
 * it produces against the declared uncompressed extent; a copy's offset against 0 < offset <= bytes produced so far. A
 * violation ends that stream with its status set; nothing outside the stream's own output extent is ever written. The
 * stream must end exactly at the declared size.
 *
 * Output dtype. Every value is widened to 64 bits (sign extension; zero extension for a 32-bit unsigned annotation) and
 * stored with two's-complement truncation to the element size the caller names (1, 2, 4 or 8 bytes): the cast happens in
 * the decode kernel's store. The host side picks the default the way pyarrow's to_numpy does.
 *
 * A refused file writes nothing the caller can see: the host side decodes into tensors of its own and hands them out only
 * after every batch of every file came back clean.
 *
 * The page table: n_pages records of OTTO_PQ_FIELDS int64, one per page, in file order within a column chunk, the
 * dictionary page of a chunk before the data pages that name it. Offsets are relative to d_bytes.
 *
 * Conventions as in otto_events.h: 0 / negative code + otto_last_error(); caller owns every buffer; d_* are device
 * pointers, h_* host pointers; launches go to the caller's hipStream_t. d_bytes must be 16-byte aligned.
 * The functions without a stream parameter (the two *_workspace sizes, otto_parquet_reason) run on the host and enqueue nothing.
 */
#ifndef OTTO_PARQUET_H
#define OTTO_PARQUET_H

#include <stdint.h>

#define OTTO_PQ_TILE 1024          /* output values per wave of the decode kernel; one run checkpoint per tile */

/* fields of a page record */
enum {
    OTTO_PQ_SRC_OFF = 0,           /* first byte of the page body (behind its header) */
    OTTO_PQ_COMP_SIZE,             /* compressed_page_size */
    OTTO_PQ_UNCOMP_SIZE,           /* uncompressed_page_size */
    OTTO_PQ_PAGE_TYPE,             /* 0 DATA_PAGE, 2 DICTIONARY_PAGE, 3 DATA_PAGE_V2 */
    OTTO_PQ_ENCODING,              /* 0 PLAIN, 5 DELTA_BINARY_PACKED (data pages), 8 RLE_DICTIONARY (the legacy 2 is taken as 8 on a
                                      data page, as 0 on a dictionary page) */
    OTTO_PQ_DEF_LEN,               /* V2: definition_levels_byte_length; V1: -1 = levels with a 4-byte prefix open the body, 0 = none */
    OTTO_PQ_REP_LEN,               /* V2: repetition_levels_byte_length; V1: 0 */
    OTTO_PQ_NUM_VALUES,
    OTTO_PQ_IS_COMPRESSED,         /* the body (V2: behind the levels) is a Snappy stream */
    OTTO_PQ_OUT_ROW,               /* row of the column's output that the page's first value goes to */
    OTTO_PQ_COL_SLOT,              /* index into the column records */
    OTTO_PQ_DICT_SLOT,             /* index of the chunk's dictionary page in this table, -1 without one */
    OTTO_PQ_FIELDS
};

/* fields of a column record */
enum {
    OTTO_PQ_COL_OUT = 0,           /* device pointer of the output column */
    OTTO_PQ_COL_ELEM,              /* bytes per output element: 1, 2, 4, 8 */
    OTTO_PQ_COL_ROWS,              /* rows the output holds */
    OTTO_PQ_COL_PHYS,              /* bytes per stored value: 4 (INT32), 8 (INT64) */
    OTTO_PQ_COL_ZEXT,              /* 1: a 32-bit unsigned annotation, widened with zeros */
    OTTO_PQ_COL_FIELDS
};

#define OTTO_PQ_PHASE_SNAPPY 1     /* phases of otto_parquet_decode (a measurement may run them apart) */
#define OTTO_PQ_PHASE_DECODE 2

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of scratch otto_parquet_decode needs for the page table: the decompressed bodies, the run checkpoints, the
 * device copies of the records, and ceil((num_values - 1) / 128) block records per delta page (the host cannot see B: a
 * body may be compressed). -22 (as a negative size) on a malformed table. */
int64_t otto_parquet_workspace(const int64_t* h_pages, int64_t n_pages);

/* Decode the pages of h_pages out of d_bytes[0 .. n_bytes), n_bytes in [0, 2^31), into the columns of h_cols
 * (n_cols records of OTTO_PQ_COL_FIELDS int64). Three kernels: k_pq_snappy, one wave per compressed page, into the
 * workspace; k_pq_runs, one lane per data page, validates the levels and the index runs and leaves one checkpoint per
 * OTTO_PQ_TILE values; k_pq_decode, one wave per tile, extracts, gathers and stores with the cast. Delta pages run four
 * kernels of their own: k_pq_delta_walk, one lane per page, validates the header and every block header and leaves one
 * record per block; k_pq_delta_sum, one wave per block, reduces the block's deltas; k_pq_delta_scan, one wave per page,
 * scans the block sums; k_pq_delta_out, one wave per block, scans inside the block and stores. Every record is checked
 * on the host before anything is launched: no page reads outside d_bytes or writes outside its column's rows.
 * h_err[0] = the table index of the smallest violating page, -1 without one; h_err[1] = its reason (otto_last_error()
 * carries the text); the call then returns -22 and the outputs' contents are unspecified. phases: OTTO_PQ_PHASE_* or'ed,
 * 3 for a decode; the decode phase alone expects the workspace of an earlier Snappy phase over the same table.
 * Synchronises the stream once. */
int otto_parquet_decode(const uint8_t* d_bytes, int64_t n_bytes, const int64_t* h_pages, int64_t n_pages, const int64_t* h_cols,
                        int32_t n_cols, int32_t phases, void* d_work, int64_t work_bytes, int64_t* h_err, void* stream);

/* bytes of scratch otto_parquet_snappy needs for n_streams */
int64_t otto_parquet_snappy_workspace(int64_t n_streams);

/* The decompressor alone (test seam): stream i is d_bytes[h_src_off[i] .. + h_src_len[i]) and must decompress to exactly
 * h_dst_len[i] bytes at d_out[h_dst_off[i] ..). h_status[i] = 0 or the violation (PQ_E_* of csrc/parquet_decode.h); a
 * violating stream leaves bytes of its own extent unspecified and every other byte of d_out untouched. An extent outside
 * d_bytes / d_out is -22 before anything is launched. Returns 0 whatever the streams hold. Synchronises the stream once. */
int otto_parquet_snappy(const uint8_t* d_bytes, int64_t n_bytes, const int64_t* h_src_off, const int64_t* h_src_len,
                        const int64_t* h_dst_off, const int64_t* h_dst_len, int64_t n_streams, uint8_t* d_out, int64_t out_bytes,
                        int32_t* h_status, void* d_work, int64_t work_bytes, void* stream);

/* the text of a violation code */
const char* otto_parquet_reason(int32_t code);

#ifdef __cplusplus
}
#endif
#endif
