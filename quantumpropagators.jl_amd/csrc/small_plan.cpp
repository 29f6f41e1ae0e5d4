// The plan of the persistent small-system kernels (small_plan.h).  Pure host code: no HIP header, no device query.
#include "small_plan.h"

#include "qprop_internal.h"

namespace qp {

static_assert(kSmallThreads * kSmallEpt == 8192, "Tuning::small_nnz default = one register slot set (x2 for the 32-slot variants)");

bool small_plan(int64_t n, int64_t maxrow, SmallPlan* p, int max_slots) {
  if (n < 1 || n > kSmallLdsRows) return false;
  for (int t = 1; t <= 64; t <<= 1) {
    const int64_t ngrp = kSmallThreads / t;
    const int64_t rows = (n + ngrp - 1) / ngrp;
    int64_t ent = 1;
    while (ent * t < maxrow) ent <<= 1;   // compile-time variants: 1, 2, 4, 8, 16 (Arnoldi: also 32)
    int64_t rows_p2 = 1;
    while (rows_p2 < rows) rows_p2 <<= 1;
    if (rows_p2 * ent <= max_slots) {   // smallest t: fewest cross-lane reduction levels
      p->lanes = t;
      p->ent = (int)ent;
      p->rows_per_group = (int)rows_p2;
      int to = 1;
      while (to < 64 && (int64_t)kSmallThreads / (2 * to) >= n) to <<= 1;
      p->obs_lanes = to;
      return true;
    }
  }
  return false;
}

}  // namespace qp

extern "C" {

int qp_small_plan_host(int64_t n, int64_t maxrow, int max_slots, int64_t out[4]) {
  if (!out || maxrow < 0 || max_slots < 1) return qp::fail(QP_E_BAD_ARG, "qp_small_plan_host: bad arguments");
  qp::SmallPlan p;
  const bool taken = qp::small_plan(n, maxrow, &p, max_slots);
  out[0] = taken ? 1 : 0;
  out[1] = taken ? p.lanes : 0;
  out[2] = taken ? p.ent : 0;
  out[3] = taken ? p.rows_per_group : 0;
  return QP_OK;
}

}  // extern "C"
