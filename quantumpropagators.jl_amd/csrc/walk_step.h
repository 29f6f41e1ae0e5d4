// What the one-term strip walk (kernels_walk_impl.h: hrb_walk_kernel) and the two-term walk (kernels_walk2_impl.h:
// hrb_walk2_kernel) share as code: the address of a row's value plane and the layout of a wavefront's near windows in LDS.
//
// The step itself -- halo map, window publish / read, the slot-ordered row sum, the driver over the two register sets -- is
// still written out in hrb_walk_kernel and in both phases of hrb_walk2_kernel, in one order that tests/test_gpu_walk2_forms.py
// and tests/test_gpu_parity.py hold together bit for bit against the per-block kernel.  It was moved into this header as
// __forceinline__ functions over always-inline accessors and measured: the results kept their bits, but the compiler's register
// figures moved in 348 of the 354 kernel instances and the headline step and a long-pair lattice left the parent's run-to-run
// spread (+0.9 % and +0.75 %).  Only the two pieces below leave the assembly of every instance as it was.
// profiles/walk_step_core.txt has the forms that were tried, piece by piece, and their figures: start there before trying again.
#pragma once

#include "kernel_common.h"

namespace qp {

// position of slot 0 of row r in the upper value array (r inside the run; rows of one 64-row block are contiguous).  The kernels
// reach it through their `vpos` lambdas: called directly it moved the instruction counts of 15 instances.
__device__ __forceinline__ int64_t walk_vpos(const WalkPlan& P, int64_t r) {
  return P.U0 + ((r >> 6) - P.R0) * (int64_t)P.ustride + (r & 63);
}

// The near windows of one wavefront in LDS, in double2 elements: the window of x (16 + 64 + 16), then NN value windows
// (16 + 64).  Element e of a block's window sits at [kWalkHalo + e], e = -16 .. 79.  The far-value FIFOs behind them are each
// kernel's own (WalkLds: m entries deep for far slot m; Walk2Lds: K + m).
template <int NN>
struct WalkWindows {
  static constexpr int XW = kRB + 2 * kWalkHalo, AW = kRB + kWalkHalo;
  static constexpr int kWin = XW + NN * AW;
};

}  // namespace qp
