/* giql_hip_coverage.h -- the coverage profile of one table in libgiql_hip.so: the segments between consecutive
 * breakpoints (distinct starts and ends) of a chromosome, each with the number of rows that cover it.  It is what
 *   SELECT disjoin_chrom, disjoin_start, disjoin_end, COUNT(*) FROM DISJOIN(t) GROUP BY disjoin_chrom, disjoin_start, disjoin_end
 * returns (`bedtools genomecov -bg`, Bioconductor `disjoin()`), computed from DISJOIN's breakpoint table without the
 * per-piece rows: one sort of 2n keys, scans, and at most 2n - 1 output rows.
 *
 * An extension header of its own beside include/giql_hip.h, whose types it uses: the entry point below is exported by
 * the same library and follows the same conventions (status codes, giql_hip_last_error, the stream argument, THE
 * LIFETIME OF A PLAN).  GIQL_HIP_ABI_VERSION is unchanged: no struct of giql_hip.h changed.
 *
 * giql_hip_coverage_dev
 *   side / n_chrom      the table, as for giql_hip_disjoin_plan_dev's target (self mode): start <= end on every row in
 *                       canonical coordinates, at most 2^29 - 1 rows.
 *   flags               0, or GIQL_COV_RUNS: maximal runs of abutting segments of equal depth become one row (the
 *                       reference's MERGE(interval, predicate := depth = PREV(depth)) over the segments of a
 *                       half-open table; abutting is judged on canonical coordinates for every encoding).
 *   chrom_out, start_out, end_out, depth_out
 *                       device arrays of `capacity` rows; depth_out may be NULL.  Start and end are in the side's
 *                       declared encoding.  Rows are ordered by (chromosome id, start).
 *   n_out               the rows written.
 * For consecutive breakpoints x < y of a chromosome the segment [x, y) exists when depth(x) = #{rows: start <= x < end}
 * is not 0, and carries that depth.  Zero-length rows cut and never count.  No segment crosses a chromosome.
 *
 * GIQL_ERR_CAPACITY: `capacity` is smaller than the row count (never more than 2n - 1); *n_out is set to the need and
 * nothing is written.  GIQL_ERR_INVALID: a row with start > end (DISJOIN's text), more than 2^29 - 1 rows, unknown
 * flags, a NULL output where rows exist.  n == 0: GIQL_OK, *n_out = 0.
 * Begins a call: a plan held in the context is dropped.  Workspace: the context's, 80 bytes per row beside the sort's
 * scratch.  Everything is enqueued on `stream`; the call returns after the stream has been synchronised. */
#ifndef GIQL_HIP_COVERAGE_H
#define GIQL_HIP_COVERAGE_H

#include "giql_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GIQL_COV_RUNS 1u /* merge abutting segments of equal depth */

int giql_hip_coverage_dev(giql_hip_ctx* ctx, const giql_side* side, int32_t n_chrom, uint32_t flags,
                          int32_t* chrom_out, int32_t* start_out, int32_t* end_out,
                          int64_t* depth_out, /* device, capacity rows; depth_out may be NULL */
                          int64_t capacity, int64_t* n_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
