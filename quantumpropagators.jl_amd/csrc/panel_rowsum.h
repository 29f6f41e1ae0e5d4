// The row sum of the batched panel kernels (kernels_spmm.hip), lane = one state of the panel: csr_spmm_kernel (per staged chunk),
// spmm_row_scalar_entries (spmm_rows_smem_kernel and the rest rows of spmm_tile_kernel) and spmm_rows_kernel (per 64-entry chunk) call
// panel_row_sum; spmm_tile_kernel keeps its compile-time 24-entry skeleton and calls the group primitive only (the comment there says
// why).  gfx950, wave64.
//
// The order of the arithmetic is part of every panel result's bits ("the same bits under every knob"), and it is this one rule:
//
//     entry k goes to acc[k & 1] while k < (len & ~3); the last len & 3 entries go into acc0; entries ascend; the result is acc0 + acc1
//
// (complex FMAs, cfma; the caller adds acc0 + acc1 once at the end of the row).  A caller that takes a row in chunks keeps the rule
// as long as every chunk but the row's last holds a multiple of four entries.  What is NOT shared: where an entry's value and its
// panel operand come from -- two accessors a(k) and x(k), small lambdas at the call site -- and every kernel's addressing, staging,
// barriers and epilogue; how many gathers a call site keeps in flight is a parameter.
#pragma once

#include "kernel_common.h"

namespace qp {

__device__ __forceinline__ double readlane_f64(double v, int l) {   // l wave-uniform
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// Entries k .. k + GG - 1, GG = 4 or 8: the operands x(k + u) are requested first, XB at a time, then the FMAs alternate acc0, acc1,
// acc0, acc1 ... in entry order.  XB = GG: GG gathers in flight; XB = 4 under GG = 8: the same order of the sums with half the
// registers (the tile kernel, whose operands come from LDS).  VF: the values a(k + u) are requested together with the operands
// (scalar or LDS loads, under way while the gathers are); without it each is taken at its FMA (the tile kernel: a v_readlane, nothing
// to wait for, and no SGPRs held across the LDS reads).
template <int GG, int XB = GG, bool VF = true, class AV, class XV>
__device__ __forceinline__ void panel_group(double2& acc0, double2& acc1, int k, const AV& a, const XV& x) {
  static_assert((GG == 4 || GG == 8) && (XB == 4 || XB == GG), "groups of four or eight entries, operands four or GG at a time");
#pragma unroll
  for (int h = 0; h < GG; h += XB) {
    double2 xs[XB], as[XB];
#pragma unroll
    for (int u = 0; u < XB; ++u) {
      xs[u] = x(k + h + u);
      if (VF) as[u] = a(k + h + u);
    }
#pragma unroll
    for (int u = 0; u < XB; u += 2) {
      cfma(acc0, VF ? as[u] : a(k + h + u), xs[u]);
      cfma(acc1, VF ? as[u + 1] : a(k + h + u + 1), xs[u + 1]);
    }
  }
}

// cnt entries (a run-time count) by the rule above: groups of G while G entries are left -- G = 8, or G = 4 where eight gathers in
// flight would cost a kernel its occupancy (csr_spmm_kernel) --, after groups of eight one group of four, then the last one to three
// entries into acc0.  (The bound is written k + (G - 1): with (k + G) - 1 the compiler forms another induction variable, and the
// rest rows of the tile kernel, whose registers are capped, come out with a stack frame.)
template <int G = 8, class AV, class XV>
__device__ __forceinline__ void panel_row_sum(double2& acc0, double2& acc1, int cnt, const AV& a, const XV& x) {
  static_assert(G == 4 || G == 8, "groups of four or eight entries");
  int k = 0;
  for (; k + (G - 1) < cnt; k += G) panel_group<G>(acc0, acc1, k, a, x);
  if constexpr (G == 8)
    if (k + 3 < cnt) {
      panel_group<4>(acc0, acc1, k, a, x);
      k += 4;
    }
  for (; k < cnt; ++k) cfma(acc0, a(k), x(k));
}

}  // namespace qp
