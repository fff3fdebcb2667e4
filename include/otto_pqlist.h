/*
 * otto_pqlist.h -- C-ABI of the level decode of Parquet list columns: the repetition and definition levels of the
 * `ground_truth` column of DATA/splits/val_labels.parquet -> row offsets and null flags. The values
 * behind the levels are decoded by otto_parquet.h from level-free page records the caller builds out of what this call
 * reports per page.
 *
 * Reference code replaced: pd.read_parquet in front of the label merges of src/covisitation/inference.py:118-123,
 * src/ranker/lgb_trainer.py:54-75, src/ranker/xgb_trainer.py:54-75, src/ranker/covisitation_candidate_generation.py:78-83,
 * src/ranker/fasttext_candidate_generator.py:55-60. Host restatement: tests/pqlist_restatement.py.
 *
 * SPEC-PQLIST (normative)
 * -----------------------
 * Accepted schema. A top-level group (REQUIRED or OPTIONAL) with exactly one child group of repetition REPEATED, which has
 * exactly one primitive child (REQUIRED or OPTIONAL) of physical type INT32 or INT64: the three-level LIST form, under any
 * field names. Maximum repetition level 1; maximum definition level D = 1 + (outer OPTIONAL) + (element OPTIONAL) <= 3.
 * Every other nested form (a two-level list, a repeated primitive at top level, a map, a struct, a list of lists) is
 * refused by the host with a message that names the form.
 *
 * Pages. V1: the decoded body opens with the repetition levels, then the definition levels, each a 4-byte little-endian
 * length and that many bytes of the RLE / bit-packed hybrid of SPEC-PARQUET; the values follow. V2: the two level streams
 * lie in front of the (possibly compressed) values without a length; their lengths are in the header. Bit widths: 1 for
 * repetition, bits(D) for definition (1, 2, 2). BIT_PACKED level encoding is refused by the host. num_values of a page
 * counts level entries.
 *
 * Meaning. Entry i has rep[i] and def[i]. rep 0 starts a row. def == D carries a value. With an OPTIONAL outer group def 0
 * is a null list and def 1 an empty list; with a REQUIRED one def 0 is an empty list. With an OPTIONAL element def == D - 1
 * is a null element, which is refused. A row may continue across the pages of a column chunk (a page may open with rep 1);
 * it never crosses a column chunk. Row and value positions are therefore sums over the whole level stream of the call.
 *
 * Outputs. off int64 [n_rows + 1]: off[r] = value_base + the number of values in front of row r, off[n_rows] =
 * value_base + the number of values of the call. null uint8 [n_rows]: 1 for a null list (its span is empty). A row at or
 * past n_rows is not stored. Per page (h_page_out, three int64): the bytes of its levels inside the body (V1: 8 + both
 * lengths; V2: both lengths), its count of values, its count of rows.
 *
 * Refusals, reason codes in this order; the smallest page wins, inside it the smallest code:
 *   OTTO_PL_E_PREFIX      a V1 length prefix or a V2 level length that runs past the page body
 *   OTTO_PL_E_RUNS        a malformed run header in a level stream
 *   OTTO_PL_E_SHORT       a level stream that ends before num_values entries
 *   OTTO_PL_E_LONG        a level stream with bytes or entries behind num_values (a bit-packed run may pad up to 7)
 *   OTTO_PL_E_LEVEL       a level above its maximum
 *   OTTO_PL_E_REP_EMPTY   repetition level 1 on an entry whose definition level says "no element"
 *   OTTO_PL_E_NULL_ELEM   a null element
 *   OTTO_PL_E_CHUNK_REP   a column chunk whose first entry has repetition level 1
 *   OTTO_PL_E_ROWS        a column chunk whose count of rep-0 entries differs from the row group's num_rows (reported on
 *                         the chunk's first page, and only when the call holds no other violation: a page refused for
 *                         its levels counts no rows)
 * A refusal returns -22, h_err[0] = the page, h_err[1] = the reason; otto_last_error() carries the text. Nothing outside
 * a page's bytes is read, nothing outside off, null and the workspace is written; after a refusal the outputs are
 * unspecified. Without one h_err = {-1, 0}. A value stream whose count differs from the page's count of def == D entries is
 * refused by otto_parquet_decode, which is handed that count as the page's num_values.
 *
 * Kernels (otto_pqlist.hip). k_pl_walk: one lane per page walks the run headers of both streams, checks them against the
 * page's extent and leaves one (header byte, first entry) checkpoint per stream and OTTO_PQ_TILE entries. k_pl_tiles: one
 * wave per tile expands both streams from the checkpoints into LDS, checks every entry and ballots rep == 0 and def == D;
 * pass 0 leaves the tile's two counts, scan.h turns them into bases in page order, pass 1 stores off and null of the rows
 * that start in the tile. k_pl_pages: one lane per page, the per-page report and the row count of every chunk.
 *
 * Conventions as in otto_rows.h: 0 / negative code + otto_last_error(); the caller owns every buffer; d_* are device
 * pointers, h_* host pointers; all arguments travel in one record and the caller's hipStream_t rides in it (side stream,
 * late inputs and reused scratch are tested in tests/test_pqlist_gpu.py). The call synchronises the stream once.
 */
#ifndef OTTO_PQLIST_H
#define OTTO_PQLIST_H

#include <stdint.h>

/* one page record: OTTO_PL_FIELDS int64 */
#define OTTO_PL_BODY_OFF 0      /* the decoded body (V1) or the stored page body (V2) inside d_bytes */
#define OTTO_PL_BODY_LEN 1      /* V1: bytes of the decoded body; V2: rep_len + def_len */
#define OTTO_PL_PAGE_TYPE 2     /* 0 DATA_PAGE, 3 DATA_PAGE_V2 */
#define OTTO_PL_REP_LEN 3       /* V2 only, else 0 */
#define OTTO_PL_DEF_LEN 4       /* V2 only, else 0 */
#define OTTO_PL_NUM_VALUES 5    /* level entries, 0 .. 2^31 - 1 */
#define OTTO_PL_FLAGS 6         /* OTTO_PL_F_* */
#define OTTO_PL_CHUNK_ROWS 7    /* on a chunk's first page: num_rows of its row group */
#define OTTO_PL_CHUNK_PAGES 8   /* on a chunk's first page: the pages of the chunk, >= 1 */
#define OTTO_PL_FIELDS 9

#define OTTO_PL_F_OUTER_OPTIONAL 1
#define OTTO_PL_F_ELEM_OPTIONAL 2
#define OTTO_PL_F_CHUNK_FIRST 4

#define OTTO_PL_E_PREFIX 1
#define OTTO_PL_E_RUNS 2
#define OTTO_PL_E_SHORT 3
#define OTTO_PL_E_LONG 4
#define OTTO_PL_E_LEVEL 5
#define OTTO_PL_E_REP_EMPTY 6
#define OTTO_PL_E_NULL_ELEM 7
#define OTTO_PL_E_CHUNK_REP 8
#define OTTO_PL_E_ROWS 9

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const uint8_t* d_bytes;    /* the page bodies */
    int64_t n_bytes;           /* 0 .. 2^31 - 1 */
    const int64_t* h_pages;    /* n_pages * OTTO_PL_FIELDS, the data pages in file order */
    int64_t n_pages;           /* 0 .. 2^24 - 1 */
    int64_t* d_off;            /* n_rows + 1 */
    uint8_t* d_null;           /* n_rows */
    int64_t n_rows;            /* the sum of CHUNK_ROWS */
    int64_t value_base;        /* added to every offset */
    int64_t* h_page_out;       /* n_pages * 3 */
    void* d_work;
    int64_t work_bytes;
    void* stream;              /* the caller's hipStream_t; every launch and copy goes there */
} otto_pqlist_job;

/* Bytes of scratch otto_pqlist_levels needs for this job (d_work and work_bytes are not looked at), or -22 for a job that
 * breaks a rule above. Host only: enqueues nothing. */
int64_t otto_pqlist_workspace(const otto_pqlist_job* job);

/* SPEC-PQLIST. h_err: two int64 (above). Synchronises the stream once. */
int otto_pqlist_levels(const otto_pqlist_job* job, int64_t* h_err);

/* The text of an OTTO_PL_E_* code. */
const char* otto_pqlist_reason(int32_t code);

#ifdef __cplusplus
}
#endif
#endif
