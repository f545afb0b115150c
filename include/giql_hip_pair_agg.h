/* giql_hip_pair_agg.h -- aggregates over a join's pairs, per left row, in libgiql_hip.so: COUNT(col), SUM, MIN, MAX
 * of columns of B over the pairs (row_a[i], row_b[i]) a join produced, grouped by row_a (bedtools `map`;
 * `SELECT a.*, AVG(b.score) ... FROM a JOIN b ON a.interval INTERSECTS b.interval GROUP BY a.*`).
 *
 * An extension header of its own beside include/giql_hip.h, whose types it uses: the entry point below is exported by
 * the same library and follows the same conventions (status codes, giql_hip_last_error, the stream argument, THE
 * LIFETIME OF A PLAN).  GIQL_HIP_ABI_VERSION is unchanged: no struct of giql_hip.h changed.
 *
 * giql_hip_pair_agg_dev
 *   row_a, row_b (n_pairs)  device int32 row ids of A / B, in any order, duplicates allowed.
 *   n_a, n_b                the rows of A / B (0 .. 2^31 - 1).
 *   aggs / n_aggs (0..8)    host array of giql_agg.  data / valid are addressed by the B row id and hold n_b rows;
 *                           out / out_nn are device arrays of n_a entries, one per A row in A's input order.
 *                           GIQL_AGG_COUNT reads validity only: its data may be NULL (COUNT over a string column).
 *   pairs_out (n_a)         device int64: the pairs of the row.
 * A row of A without a pair gets pairs_out = 0, out_nn = 0 and out = 0.  NaN order, int64 / binary64 accumulation
 * and "no non-NULL input is NULL (out_nn = 0, out = 0)" are those of giql_hip_merge_agg_dev.
 *
 * The result is a function of the SET of pairs: a row's values are reduced in ascending row_b whatever order the pairs
 * arrive in, without atomics on values, so a float SUM has the same bits for every join form and on every run.
 *
 * Ids are not trusted: a row_a outside [0, n_a) or a row_b outside [0, n_b) -- negative included -- makes the call
 * return GIQL_ERR_INVALID; the id is found before anything is read through it and is never followed.  The outputs
 * are then undefined.
 *
 * n_pairs == 0: GIQL_OK, the outputs zeroed.  n_a == 0: GIQL_OK, nothing written.  GIQL_ERR_INVALID before anything
 * is launched: n_pairs >= 2^31, n_aggs outside 0..8, a NULL out, an unknown function or type, a NULL data for
 * anything but COUNT, a NULL pairs_out, row_a or row_b (where they would be used).
 * Begins a call: a plan held in the context is dropped.  Workspace: the context's, 16 bytes per pair for the two
 * (row_b, row_a) sort buffers plus 8 for the region arrays and 16 per aggregate and region.  Everything is enqueued
 * on `stream`; the call returns after the stream has been synchronised (the status word is read back). */
#ifndef GIQL_HIP_PAIR_AGG_H
#define GIQL_HIP_PAIR_AGG_H

#include "giql_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GIQL_PAIR_AGG_MAX 8

int giql_hip_pair_agg_dev(giql_hip_ctx* ctx, const int32_t* row_a, const int32_t* row_b, int64_t n_pairs,
                          int64_t n_a, int64_t n_b,
                          const giql_agg* aggs, int32_t n_aggs, /* host array, 0..8 */
                          int64_t* pairs_out,                   /* device [n_a]: pairs of the row */
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
