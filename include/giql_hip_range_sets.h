/* giql_hip_range_sets.h -- the literal range sets of libgiql_hip.so: `interval <op> ANY('chr:lo-hi', ...)` over one
 * table (docs/dialect/quantifiers.rst; src/giql/expanders/intersects.py:243-270: an OR of one term per range,
 *   chrom = c AND <cmp on start> AND <cmp on end>, under SQL's three-valued logic).
 *
 * An extension header of its own beside include/giql_hip.h, whose types it uses: the entry point below is exported by
 * the same library and follows the same conventions (status codes, giql_hip_last_error, the stream argument, THE
 * LIFETIME OF A PLAN).  GIQL_HIP_ABI_VERSION is unchanged: no struct of giql_hip.h changed.
 *
 * chrom / start / end: the table's per-row int32 chromosome codes and its RAW int32 coordinate columns, n rows;
 * valid_*: one byte per row (0 = SQL NULL) or NULL = no NULLs.  All DEVICE pointers.  Each of the n_sets (1..8) sets
 * holds n_ranges (1..1024) ranges in HOST arrays, in any order, duplicates allowed: a chromosome code and the int64
 * bounds its term compares `start` and `end` with -- the caller has moved the table's coordinate encoding onto them, the
 * columns are compared as they lie in memory:
 *   GIQL_RANGE_INTERSECTS  start <  on_start AND end >  on_end     (on_start = the range's end, on_end = its start)
 *   GIQL_RANGE_CONTAINS    start <= on_start AND end >= on_end
 *   GIQL_RANGE_WITHIN      start >= on_start AND end <= on_end
 * Per set and row it writes the predicate's three-valued result as two bytes: out_value (1 = TRUE) and out_valid
 * (0 = NULL, out_value 0 then) -- a giql_operand of type GIQL_T_U8 with its validity for giql_hip_select_dev.  A row
 * whose code no range of the set carries is FALSE.  One streaming read of the three columns per set; per row one
 * binary search in the set's table (staged in LDS) and one compare, so the work grows with log n_ranges.  No
 * linearised axis: no GIQL_ERR_SPAN.  GIQL_ERR_INVALID before anything is launched: n outside [0, 2^31-16], n_sets /
 * n_ranges outside their bounds, an unknown op, a NULL array.  Begins a call: a plan held in the context is dropped,
 * also when n = 0 (tests/test_range_sets_gpu.py holds its cells of the plan-lifetime table). */
#ifndef GIQL_HIP_RANGE_SETS_H
#define GIQL_HIP_RANGE_SETS_H

#include "giql_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GIQL_RANGE_INTERSECTS 0
#define GIQL_RANGE_CONTAINS   1
#define GIQL_RANGE_WITHIN     2
#define GIQL_RANGE_MAX_SETS   8
#define GIQL_RANGE_MAX_RANGES 1024

typedef struct giql_range_set {
  int32_t op, n_ranges;      /* GIQL_RANGE_*; 1..GIQL_RANGE_MAX_RANGES                     */
  const int32_t* chrom;      /* host, n_ranges: chromosome code of each range             */
  const int64_t* on_start;   /* host, n_ranges: the bound `start` is compared with        */
  const int64_t* on_end;     /* host, n_ranges: the bound `end` is compared with          */
  uint8_t* out_value;        /* device, n bytes                                           */
  uint8_t* out_valid;        /* device, n bytes                                           */
} giql_range_set;

int giql_hip_range_set_any_dev(giql_hip_ctx* ctx, const int32_t* chrom, const int32_t* start, const int32_t* end,
                               const uint8_t* valid_chrom, const uint8_t* valid_start, const uint8_t* valid_end,
                               int64_t n, const giql_range_set* sets, int32_t n_sets, void* stream);

#ifdef __cplusplus
}
#endif
#endif
