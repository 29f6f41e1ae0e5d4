// Pure-host planning unit: HOW an operator runs, decided on plain host data -- the device format (choose_format), the lattice
// completion of open-boundary grids (lattice_fill), the strip-walk plans of a Hermitian-packed lattice (plan_walk, with the shape
// parser walk_shape_reason), the column-blocked mirror of an operator with irregular columns (plan_colblock), the batched path's
// row order and LDS tiles with the kernel's operand table (plan_spmm_order, plan_spmm_tiles, spmm_tile_table).  No HIP, no handle
// type, no device query: the union pattern, the layout, knob values and the CU count in, numbers and vectors out
// (operator_plans.cpp); engine_plans.hip uploads the results.  Index work: exact, and compiled as ordinary C++ by the sanitizer
// harness (tests/sanitize_host_index.cpp), whose table tests/operator_plan_cases.h pins the numbers.
#pragma once

#include <string>
#include <vector>

#include "operator_layout.h"
#include "walk_geometry.h"

// the union pattern of an operator (borrowed)
struct UnionPattern {
  int64_t nrows = 0, ncols = 0;
  const UnionRowptr& ur;
  const UnionCols& uc;
};
// what the planners read of the context's knobs (device.h: Tuning; engine_host.h: plan_knobs)
struct PlanKnobs {
  int hrb_walk = 1, walk_min_blocks = 3072, lattice_fill = 1, colblock = 1, cb_log2w = 0, spmm_strip = 0;
};

// ---- the walk's stencil shape --------------------------------------------------------------------------------------------
// read off one row's sorted list of column distances (kernels_walk.hip):
//   [-L_1]? [-L_0]? [-K g .. -g] [-d_nn .. -d_1] [0]? [d_1 .. d_nn] [g .. K g] [L_0]? [L_1]?
// near distances of at most kWalkHalo rows, far distances the multiples of one strip step g >= 64 rows, optionally one or two
// more pairs +-L beyond them (xl: the plane distance of a three-dimensional grid, and its double for a fourth-order stencil;
// the volume distance of a four-dimensional one).
struct WalkShape {
  int nn = 0, K = 0, z0 = 0, xl = 0, fd = 0;   // fd = 1: diagonal far neighbours g - 1, g, g + 1 (nine-point stencils)
  int64_t g = 0, glong = 0, glong1 = 0;   // glong: the longest distance; glong1: the shorter long one when there are two
  int near[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
// 0 = a shape the walk has a kernel for; else the QP_WALK_* code of what broke it (include/qprop.h), with the offending
// numbers in *why
int walk_shape_reason(const std::vector<int64_t>& dl, WalkShape& w, std::string* why);
inline bool parse_walk_shape(const std::vector<int64_t>& dl, WalkShape& w) { return walk_shape_reason(dl, w, nullptr) == QP_WALK_OK; }

// ---- strip-walk plans (walk_geometry.h: WalkPlan) --------------------------------------------------------------------------
struct WalkPlans {
  int reason = QP_WALK_OK;           // QP_WALK_*: why there is no plan
  std::string text;
  qp::WalkPlan one, two;             // (edge_map: the caller's device copies of the lists below)
  std::vector<int32_t> edge, edge2;  // the blocks outside [W0, R1) of either plan
};
WalkPlans plan_walk(const UnionPattern& A, const HostLayout& L);

// the device format for `requested` (QP_FMT_AUTO: chosen); -1: QP_FMT_HRB requested for a non-Hermitian operator
int choose_format(const UnionPattern& A, int requested, bool hermitian, const PlanKnobs& k);

// completes the rows of an open-boundary lattice with explicit zeros, in place; ur_before / uc_before take the pattern as it was,
// and only when something was completed
void lattice_fill(const PlanKnobs& k, int64_t n, int64_t ncols, UnionRowptr& ur, UnionCols& uc, UnionRowptr* ur_before = nullptr,
                  UnionCols* uc_before = nullptr);

// ---- column-blocked mirror (device.h: ColBlockPlan) ---------------------------------------------------------------------
struct ColBlockHost {
  qp::ColBlockShape shape;      // valid = 0: no mirror (the vectors are empty)
  double line_share = -1.0;     // share of a row block's gathers that pull a line of their own (sampled); < 0: not sampled
  std::vector<int32_t> segptr;
  std::vector<uint16_t> rowoff;
  std::vector<uint32_t> cols;
  std::vector<int64_t> map;
};
ColBlockHost plan_colblock(const UnionPattern& A, const HostLayout& L, const PlanKnobs& k, int cu);

// ---- batched path: row order of the row kernel, LDS tiles (device.h: SpmmTiles) -------------------------------------------
struct SpmmOrder {
  std::vector<int32_t> order;   // empty: the natural order
  int64_t g = 0, sw = 0;        // what was detected: inner dimension and strip width
};
SpmmOrder plan_spmm_order(const UnionPattern& A, int batch, int knob);

struct SpmmTilesHost {
  qp::SpmmTileShape shape;
  std::vector<int32_t> tiles, rest;   // first row of every tile; the rows outside the tiles.  tiles empty: the row kernel alone
  int64_t g = 0, sw = 0;
};
SpmmTilesHost plan_spmm_tiles(const UnionPattern& A, int knob);

struct SpmmTileTable {
  int T = 0;                   // staged rows: 16 + 8 K + 8 NN
  std::vector<int32_t> tab;    // kSpmmTileTab entries (layout_constants.h)
};
SpmmTileTable spmm_tile_table(const qp::SpmmTileShape& shape, int64_t g);
