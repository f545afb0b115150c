// eval_kernels.hip.h -- computed SELECT-list columns: the VALUE of an expression program per candidate pair,
// stored instead of the keep bit the residual filter derives from it (select_kernels.hip.h).
//
// The recipes behind it are bedtools' -wo / -wao (docs/recipes/bedtools-migration.rst, docs/recipes/intersect.rst):
// "(LEAST(a.end, b.end) - GREATEST(a.start, b.start)) AS overlap_bp" beside the pairs, and under a LEFT JOIN the
// same inside "CASE WHEN b.chrom IS NULL THEN 0 ELSE ... END".  The programs are the postfix programs of the select
// kernel, run by the same interpreter (sel_eval_prog), plus IF / NULL nodes for a searched CASE; a negative row id
// is the NULL row of its side (the padded row of giql_hip_left_pad_dev), so one pass serves the matched and the
// padded rows of a LEFT join.
//
// HBM-bound on paper: 8 B of ids read, every referenced column gathered once per candidate (the programs of one
// call run back to back on a candidate, so a gathered line is reused from cache), 8 B + 1 B written per candidate
// and output.  The interpreter's value stack lives in scratch; that traffic is the suspect where the measured time
// departs from the byte count ("Computed columns").
#pragma once
#include "select_kernels.hip.h"

namespace giql {

constexpr int EV_MAX_OUTS = 8;

// mirrors giql_expr_out of include/giql_hip.h
struct DevExprOut {
  int first, count;  // the program: nodes [first, first + count)
  int type;          // 1 i64, 3 f64 (GIQL_T_*): element type of data
  int pad;
  void* data;
  uint8_t* valid;    // may be null: the NULLs are counted only
};
struct DevExprOuts {
  DevExprOut o[EV_MAX_OUTS];
  int n;
};

// The select kernel's geometry: a block takes tiles of SEL_TILE candidates, a thread SEL_ITEMS of them at stride
// SEL_NT, so the id loads and the 8-byte stores of a wave are contiguous.  The grid is capped and strides over the
// tiles: the NULL counts then cost one atomic per wave and output that saw a NULL, whatever n is.
// A row id >= its side's row count raises GIQL_ERR_INVALID (the candidate's outputs read as NULL); a negative one is
// that side's NULL row -- sel_load reads nothing through it.
__global__ __launch_bounds__(SEL_NT) void k_eval_expr(DevExprOuts outs, const DevOperand* __restrict__ prog,
                                                      const int* __restrict__ idx_a, u32 n_rows_a,
                                                      const int* __restrict__ idx_b, u32 n_rows_b, u64 n, u32 n_tiles,
                                                      u64* __restrict__ n_null, DevMeta* meta) {
  u32 nulls[EV_MAX_OUTS];  // per wave; every lane of a wave holds the same counts (the unrolled k keeps them in registers)
#pragma unroll
  for (int k = 0; k < EV_MAX_OUTS; k++) nulls[k] = 0;
  bool bad = false;
  for (u32 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const u64 base = (u64)tile * SEL_TILE;
    for (int j = 0; j < SEL_ITEMS; j++) {
      const u64 i = base + (u64)j * SEL_NT + threadIdx.x;
      const bool live = i < n;
      int ia = 0, ib = 0;
      bool ok = live;
      if (live) {
        ia = idx_a ? idx_a[i] : (int)i;
        ib = idx_b ? idx_b[i] : (int)i;
        if ((ia >= 0 && (u32)ia >= n_rows_a) || (ib >= 0 && (u32)ib >= n_rows_b)) {
          bad = true;
          ok = false;
        }
      }
#pragma unroll
      for (int k = 0; k < EV_MAX_OUTS; k++) {
        if (k >= outs.n) break;  // (kernel argument: the same in every lane)
        const DevExprOut o = outs.o[k];
        bool is_null = false;
        if (live) {
          SelValue v;
          v.i = 0;
          v.f = 0.0;
          v.is_float = false;
          v.null = true;
          if (ok) v = sel_eval_prog(prog, o.first, o.count, ia, ib);
          is_null = v.null;
          if (o.type == 3) {
            const double x = v.null ? 0.0 : (v.is_float ? v.f : (double)v.i);
            reinterpret_cast<double*>(o.data)[i] = x;
          } else {
            reinterpret_cast<i64*>(o.data)[i] = v.null ? 0 : v.i;
          }
          if (o.valid) o.valid[i] = v.null ? 0 : 1;
        }
        nulls[k] += (u32)__popcll(__ballot(is_null));
      }
    }
  }
  if (lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < EV_MAX_OUTS; k++)
      if (k < outs.n && nulls[k]) atomicAdd((unsigned long long*)&n_null[k], (unsigned long long)nulls[k]);
  }
  if (bad) atomicMin(&meta->status, -1);
}

}  // namespace giql
