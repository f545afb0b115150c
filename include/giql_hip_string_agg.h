/* giql_hip_string_agg.h -- STRING_AGG beside MERGE in libgiql_hip.so: the names of every merged region joined by a
 * separator (bedtools `merge -c 4 -o collapse`; docs/recipes/clustering.rst:267-279; merge.py:317-390 keeps any plain
 * aggregate beside MERGE under the per-cluster GROUP BY).
 *
 * An extension header of its own beside include/giql_hip.h, whose types it uses: the two entry points below are
 * exported by the same library and follow the same conventions (status codes, giql_hip_last_error, the stream
 * argument, THE LIFETIME OF A PLAN).  GIQL_HIP_ABI_VERSION is unchanged: no struct of giql_hip.h changed.
 *
 * Semantics (DuckDB's string_agg): NULL inputs are skipped; a region with no non-NULL input is NULL (out_nn = 0, an
 * empty slice of the output); an empty string is a value and brings its separator.  The members of a region are
 * joined in ascending `start`, then ascending row id: the merge's sort by start is stable in every form it takes and
 * carries the row ids.  No atomics anywhere: the same call returns the same bytes.
 *
 * Two steps, like giql_hip_take_utf8_plan_dev / _fill_dev -- the caller allocates the bytes in between:
 *
 * giql_hip_merge_str_dev = giql_hip_merge_agg_dev with n_aggs in 0..8, plus
 *   strs / n_strs (1..4)  one giql_str_agg per string aggregate (host array).  Per aggregate the call writes
 *                         out_offsets[0..*n_out] (Arrow offsets of the region strings), out_nn[r] (non-NULL inputs of
 *                         region r; 0 = the region's string is NULL), row_dst (below) and n_bytes = out_offsets[*n_out].
 *   out_order (s->n)      the row ids in the merge's order; region r owns out_count[r] consecutive entries.
 * row_dst is indexed by sorted position (the index into out_order): bits 0..30 the byte offset of the row's value in
 * the output, bit 31 "a separator precedes it" (at offset - sep_len), 0xFFFFFFFF a NULL row.  The caller owns row_dst,
 * so the pair keeps NO plan in the context.
 * One call yields at most 0x7FFFFFFF bytes per aggregate (int32 offsets, 31-bit row_dst): an aggregate past that gets
 * n_bytes = -1 and the call returns GIQL_ERR_CAPACITY naming it (an output of exactly 0x7FFFFFFF bytes is refused as
 * well when sep_len > 0: its last row_dst could read as the NULL mark).  The other outputs of the call are complete.
 * GIQL_ERR_INVALID names the aggregate, before anything is launched: n_strs outside 1..4, n_aggs outside 0..8,
 * sep_len outside 0..255, a NULL offsets / out_offsets / out_nn / row_dst / out_order (tables with rows).  An offset
 * pair that decreases (or is negative) is found by the length pass and reported as GIQL_ERR_INVALID; it is never
 * followed.  Begins a call: a plan held in the context is dropped, also when the table is empty (then *n_out = 0,
 * n_bytes = 0 and out_offsets[0] = 0 where out_offsets is given).
 *
 * giql_hip_concat_utf8_fill_dev writes the bytes: for every sorted position i < n whose row_dst[i] is not the NULL
 * mark, the value of row order[i] (offsets / data: the column, n_rows rows) at its offset and, where bit 31 is set,
 * the separator in front of it.  Every output byte is written exactly once.  sep: HOST pointer, sep_len (0..255)
 * bytes.  out_data: n_bytes bytes.  No workspace; an INNER or DISJOIN plan held in the context survives the call, a
 * CONTAINS plan does not (as giql_hip_take_utf8_fill_dev).  An order[i] >= n_rows, a decreasing offset pair or a
 * separator that would begin before out_data is GIQL_ERR_INVALID; such a row is neither read nor written. */
#ifndef GIQL_HIP_STRING_AGG_H
#define GIQL_HIP_STRING_AGG_H

#include "giql_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GIQL_STR_AGG_MAX      4
#define GIQL_STR_AGG_MAX_SEP  255
#define GIQL_STR_AGG_NULL_ROW 0xFFFFFFFFu

typedef struct giql_str_agg {
  const int32_t* offsets;   /* Arrow utf8 offsets, s->n + 1, device        */
  const uint8_t* valid;     /* device byte-per-row validity, or NULL       */
  int32_t sep_len;          /* 0..255                                      */
  int32_t* out_offsets;     /* device, capacity + 1                        */
  int64_t* out_nn;          /* device, capacity                            */
  uint32_t* row_dst;        /* device, s->n                                */
  int64_t n_bytes;          /* written by the call                         */
} giql_str_agg;

int giql_hip_merge_str_dev(giql_hip_ctx* ctx, const giql_side* s, int32_t n_chrom, int64_t distance,
                           const struct giql_pred* preds, int32_t n_preds, /* 0: plain MERGE */
                           const giql_agg* aggs, int32_t n_aggs,           /* host array, 0..8 */
                           giql_str_agg* strs, int32_t n_strs,             /* host array, 1..4 */
                           int32_t* out_chrom, int32_t* out_start, int32_t* out_end, int64_t* out_count,
                           int32_t* out_order, int64_t capacity, int64_t* n_out, void* stream);

int giql_hip_concat_utf8_fill_dev(giql_hip_ctx* ctx, const int32_t* offsets, const uint8_t* data, int64_t n_rows,
                                  const int32_t* order, const uint32_t* row_dst, int64_t n, const uint8_t* sep,
                                  int32_t sep_len, uint8_t* out_data, void* stream);

#ifdef __cplusplus
}
#endif
#endif
