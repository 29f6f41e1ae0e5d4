// Internal header of the device layer of the plans that decide HOW an operator is run (engine_plans.hip), called from the
// operator build (engine_operator.hip).  The decisions themselves are the pure-host planning unit's (operator_plans.h); what an
// operator's arrays ARE is the pure-host layout unit's business (operator_layout.h, included by engine.h).
#pragma once

#include "engine.h"
#include "operator_plans.h"

// what the planners read of an operator and of its context's knobs
inline UnionPattern union_pattern_of(const qp_operator* op) { return UnionPattern{op->A.nrows, op->A.ncols, op->u_rowptr, op->u_col}; }
inline PlanKnobs plan_knobs(const qp::Tuning& t) { return PlanKnobs{t.hrb_walk, t.walk_min_blocks, t.lattice_fill, t.colblock, t.cb_log2w, t.spmm_strip}; }

int choose_format(qp_operator* op, int requested, bool hermitian);
int build_walk_plan(qp_operator* op);
int build_colblock(qp_operator* op);
