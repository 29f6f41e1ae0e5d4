// Pure-host planning unit of cheby!: what the host decides on plain data before it touches the device -- the accumulator
// schedule and the step's scalars, the ORDER OF LAUNCHES of one step with the vector every term gathers, reads and writes
// (ChebySequence), the boundary / adjacent / interior partition of a split term (plan_split), the gate of the persistent
// small-system kernel and the verdict of check_normalization.  No HIP, no handle type: numbers and vectors in, numbers and
// vectors out (cheby_plan.cpp); engine_cheby.hip and engine_sharded.hip map slots to pointers, upload and launch.  Compiled as
// ordinary C++ by tests/cheby_plan_host.cpp, whose table tests/cheby_plan_cases.h pins the sequences and the partitions.
#pragma once

#include <cstdint>
#include <vector>

#include "layout_constants.h"
#include "small_plan.h"

// which terms of a cheby! touch the Psi accumulator (include/qprop.h, qp_acc_defer)
void acc_schedule(const double* a, int n_coeffs, bool defer, qp_acc_defer* out);
// @assert abs(dt) ~ abs(wrk.dt)   (isapprox, rtol = sqrt(eps))   src/cheby.jl:157
bool cheby_dt_matches(double dt, double wrk_dt);
struct ChebyScalars {   // src/cheby.jl:156, :158-162, :211
  double beta;
  qp::cplx c, phase;
  ChebyScalars(double Delta, double E_min, double dt);
};

// ---- the launches of one step ---------------------------------------------------------------------------------------------
// The vectors of a step by name: Psi's own buffer, the workspace's three term vectors and its accumulator.  (The row-partitioned
// step has two: Psi = X0, A = X1.)
enum class ChebySlot : int { None = 0, Psi, A, C, D, Acc };
constexpr int kChebySlots = 6;

struct ChebyTerm {   // one fused term: v_m = c (H x - beta x) + v0 -> vout, Psi's accumulator acc_in -> acc_out
  int m = 0;
  ChebySlot x = ChebySlot::None, v0 = ChebySlot::None, vout = ChebySlot::None;   // x holds v_{m-1}, v0 holds v_{m-2} (term 1: none)
  ChebySlot acc_in = ChebySlot::None, acc_out = ChebySlot::None;                 // both None: the schedule skips the accumulator
  double a_prev = 0.0;   // the coefficient of v_0 while the accumulator has not been written
  double a = 0.0;        // a[m]
  double c_scale = 1.0;  // the step's c is doubled after term 1 (src/cheby.jl:184)
  int apply_phase = 0;   // the last term only
  bool check = false;    // carries the partials of check_normalization (the reference checks terms i >= 3 only: m >= 2)
  const qp_acc_defer* defer = nullptr;
};
struct ChebyLaunch {
  int m = 0;            // first term of the launch
  bool pair = false;    // terms m and m + 1 in one pass over the matrix values (kernels_walk2.hip): t[0] and t[1]
  ChebyTerm t[2];
};

// Term m gathers the vector term m - 1 wrote.  A one-term launch writes v_m over v_{m-2} in place (term 1: into A); a pair writes
// v_m and v_{m+1} to the two vectors no term of the launch reads -- the neighbouring strip columns still gather from x and v0 -- so
// a step that takes pairs rotates four vectors (Psi, A, C, D) instead of two.  Psi's buffer is an output only for the last update
// of the accumulator, only while it is not being gathered and only in a step that takes no pairs; otherwise the result lands in
// Acc and the caller copies it.  A pair is proposed for m > 1 when the schedule lets at most one of the two terms update the
// accumulator; the launcher may still refuse it at run time (no kernel instance).
class ChebySequence {
 public:
  // can a step of this kind take pairs at all?  (the caller adds what only it knows: the vectors C and D, the operator's plan)
  static bool pairs_possible(int n_coeffs, bool check_normalization, bool panel) { return !panel && !check_normalization && n_coeffs - 1 >= 3; }
  ChebySequence(const double* a, int n_coeffs, bool defer, bool pairs_allowed, bool check_normalization, bool panel);
  bool next(ChebyLaunch* L);   // the launch to issue now; false: the step is complete
  // the pair next() just gave was not launched: the next launch is its first term alone, no pair is proposed again in this step,
  // and the accumulator is as if the proposal had never been made
  void refuse();
  ChebySlot result() const { return st_.result; }   // after the last launch: where the new Psi is (the caller copies unless Psi)

 private:
  struct State {
    int m = 1;
    bool pairs = false;
    bool updated = false;   // has any term written the accumulator yet?
    ChebySlot cur = ChebySlot::Psi, prev = ChebySlot::None, spare[2] = {ChebySlot::C, ChebySlot::D}, result = ChebySlot::None;
  };
  ChebyTerm term(int m, ChebySlot x, ChebySlot v0, ChebySlot vout, ChebySlot acc_out);
  const double* a_;
  int nterms_;
  bool check_;
  std::vector<qp_acc_defer> sched_;
  State st_, undo_;
};

// ---- boundary / interior split of one fused term (qp_split_create) ---------------------------------------------------------
// What the partition reads of the operator's one-term walk plan (walk_geometry.h: WalkPlan); valid = 0: no walk
struct SplitWalk {
  int valid = 0, K = 0, fd = 0;
  int64_t g = 0, glong = 0, W0 = 0, R1 = 0;
};
struct SplitPlan {
  std::vector<int32_t> boundary;   // blocks with a send row or a row that reads a ghost column (column >= nrows), ascending
  std::vector<int32_t> interior;   // the others: n_plain plain blocks, then the adjacent ones -- they gather from boundary rows or
  int64_t n_plain = 0;             //   boundary rows gather from them, and only they wait for the boundary launch of the term before
  std::vector<int32_t> mirror;     // 64 * n_boundary + 1: slab slot (index in send_rows) of a boundary block's row, or -1
  unsigned wait_from_wg = 0;       // interior workgroups at or beyond this position poll ...
  unsigned n_waiting_wg = 0;       // ... and how many of them there are
  // The interior as a strip walk.  The boundary blocks of a row-partitioned lattice are a prefix and a suffix of the local rows;
  // the walk takes the interior blocks from which no walked row block, with its ring of +-K strip steps and its one-block halo,
  // reaches a boundary block: [max(W0, lo + reach), min(R1, hi - reach)); `edge`: the rest of the interior, in its order
  bool walk = false;
  int64_t W0 = 0, R1 = 0;
  std::vector<int32_t> edge;
};
// u_rowptr / u_col: the union pattern of the nrows local rows; rows_per_wg: row blocks per workgroup of the per-block kernels.
// QP_E_BAD_ARG (through qp::fail) for a send row out of range or listed twice.
int plan_split(int64_t nrows, const int64_t* u_rowptr, const int32_t* u_col, const int64_t* send_rows, int64_t nsend,
               int rows_per_wg, const SplitWalk& walk, SplitPlan* out);

// ---- small gates and verdicts -------------------------------------------------------------------------------------------
// does the persistent small-system kernel take a Chebychev time grid of an operator with these numbers, and with which plan?
// (small_nnz: the knob; cheby_small_candidate: the part that needs no pass over the rows)
inline bool cheby_small_candidate(int64_t nnz, int nops, int small_nnz) { return small_nnz > 0 && nnz <= 2 * (int64_t)small_nnz && nops <= 64; }
bool cheby_small_gate(int64_t nnz, int nops, int64_t n, int64_t maxrow, int small_nnz, qp::SmallPlan* plan);
// check_normalization: triples {Re<v1,t>, Im<v1,t>, |v1|^2} of terms 1 .. nterms -> the first term (as the reference counts: m + 1)
// whose map norm is not within 1 + limit (a NaN is not), or 0      src/cheby.jl:195
int cheby_normalization_verdict(const double* triples, int nterms, double limit);
