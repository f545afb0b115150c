/* giql_hip_pair_expr_agg.h -- aggregates of per-pair EXPRESSIONS over a join's pairs, per left row, in libgiql_hip.so:
 * giql_hip_pair_agg_dev (include/giql_hip_pair_agg.h) whose value source may be an expression program evaluated at
 * the pair (row_a[i], row_b[i]) instead of a column of B
 * (`SELECT a.*, SUM(LEAST(a.end, b.end) - GREATEST(a.start, b.start)) ... GROUP BY a.*`; what
 * `bedtools intersect -wo | groupby` computes).
 *
 * An extension header of its own beside include/giql_hip.h, whose types it uses: the entry point below is exported by
 * the same library and follows the same conventions (status codes, giql_hip_last_error, the stream argument, THE
 * LIFETIME OF A PLAN).  GIQL_HIP_ABI_VERSION is unchanged: no struct of giql_hip.h changed.
 *
 * giql_hip_pair_expr_agg_dev
 *   row_a, row_b, n_pairs, n_a, n_b, pairs_out   as giql_hip_pair_agg_dev.
 *   nodes / n_nodes (0..256)   host array of giql_operand: the postfix programs of giql_hip_eval_expr_dev (same node
 *                              kinds, GIQL_X_IF / GIQL_X_NULL included).  Columns of side A hold n_a rows and are read
 *                              at row_a[i], columns of side B hold n_b rows and are read at row_b[i].
 *   aggs / n_aggs (0..8)       host array of giql_pair_expr_agg: per aggregate the function and ONE value source --
 *       count == 0   a column of B: data / valid / type as giql_agg (GIQL_AGG_COUNT may give a NULL data);
 *       count >= 1   the program nodes[first, first + count) with its static result type in `type`: GIQL_T_I64 (the
 *                    value is the program's integer) or GIQL_T_F64 (a float value, or an integer one converted once,
 *                    as giql_hip_eval_expr_dev stores it).  data and valid are ignored.  A pair at which the program
 *                    is NULL is no input of the aggregate.
 *     out / out_nn are device arrays of n_a entries as in giql_agg: out is int64 for COUNT and for SUM / MIN / MAX of
 *     an integer source, binary64 for SUM / MIN / MAX of a float source.
 * Aggregates with the same source (the same column, or the same first / count / type) share one evaluation per pair.
 *
 * The programs are checked and statically typed on the host exactly as giql_hip_eval_expr_dev does it, before
 * anything is launched: GIQL_ERR_INVALID for a malformed program, a node range outside `nodes`, and a program that can
 * yield a float (a float column or literal, a `/`) under type GIQL_T_I64.
 *
 * Everything else is giql_hip_pair_agg_dev's: a row of A without a pair gets pairs_out = 0, out_nn = 0, out = 0; NaN
 * order, int64 / binary64 accumulation (an integer SUM wraps: the caller bounds n_pairs x max|value|) and "no non-NULL
 * input is NULL"; the result is a function of the SET of pairs -- a row's values are reduced in ascending row_b without
 * atomics on values, so a float SUM has the same bits for every join form and on every run; ids are not trusted: a
 * row_a outside [0, n_a) or a row_b outside [0, n_b) makes the call return GIQL_ERR_INVALID, and is found before any
 * program or column is read through it; n_pairs == 0: GIQL_OK, the outputs zeroed; n_a == 0: GIQL_OK, nothing
 * written; GIQL_ERR_INVALID before anything is launched for n_pairs >= 2^31, n_aggs outside 0..8, n_nodes outside
 * 0..256, a NULL out, an unknown function or type, a NULL data of a column source for anything but COUNT, a NULL
 * pairs_out, row_a or row_b (where they would be used).  Begins a call: a plan held in the context is dropped.
 *
 * Workspace: the context's; giql_hip_pair_agg_dev's (16 bytes per pair for the two sort buffers plus 8 for the region
 * arrays, 16 per aggregate and region) plus the 256 staged nodes (12 KiB).  NO per-pair value array: a program's value
 * goes from the interpreter into the reduction in registers.  Everything is enqueued on `stream`; the call returns
 * after the stream has been synchronised (the status word is read back). */
#ifndef GIQL_HIP_PAIR_EXPR_AGG_H
#define GIQL_HIP_PAIR_EXPR_AGG_H

#include "giql_hip_pair_agg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GIQL_PAIR_EXPR_AGG_MAX_NODES 256

typedef struct giql_pair_expr_agg {
  int32_t func, type;   /* GIQL_AGG_*; GIQL_T_* of data, or the program's result type    */
  const void* data;     /* column source: device column of n_b rows                      */
  const uint8_t* valid; /* column source: byte-per-row validity, NULL = all valid        */
  int32_t first, count; /* expression source: nodes [first, first + count); count == 0:  */
                        /* a column source                                               */
  void* out;            /* device, n_a x 8 bytes                                         */
  int64_t* out_nn;      /* device, n_a: non-NULL inputs of the row.  May be NULL         */
} giql_pair_expr_agg;

int giql_hip_pair_expr_agg_dev(giql_hip_ctx* ctx, const int32_t* row_a, const int32_t* row_b, int64_t n_pairs,
                               int64_t n_a, int64_t n_b,
                               const struct giql_operand* nodes, int32_t n_nodes, /* host array, 0..256 */
                               const giql_pair_expr_agg* aggs, int32_t n_aggs,    /* host array, 0..8 */
                               int64_t* pairs_out,                                /* device [n_a] */
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif
