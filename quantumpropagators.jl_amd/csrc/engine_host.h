// Internal header of the host index work that decides HOW an operator is run (engine_plans.hip: format choice, lattice
// completion, strip-walk plan, column-blocked mirror), called from the operator build (engine_operator.hip).  What an
// operator's arrays ARE is the pure-host layout unit's business (operator_layout.h, included by engine.h).
#pragma once

#include "engine.h"

struct WalkShape;
int choose_format(qp_operator* op, int requested, bool hermitian);
void lattice_fill(const qp::Tuning& tun, int64_t n, int64_t ncols, qp::HostVec<int64_t>& ur, qp::HostVec<int32_t>& uc,
                  qp::HostVec<int64_t>* ur_before = nullptr, qp::HostVec<int32_t>* uc_before = nullptr);
int build_walk_plan(qp_operator* op);
int build_colblock(qp_operator* op);
