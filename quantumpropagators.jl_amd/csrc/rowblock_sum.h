// The row sum of one 64-row block by one wavefront (lane = row), shared by every row-block mat-vec outside the strip walk:
// rbcsr_spmv_kernel and the upper section of hrb_spmv_kernel (kernels.hip), rbcsr_coded_spmv_kernel (kernels_coded.hip) and
// arnoldi_matvec_dots_kernel (kernels_arnoldi.hip).  arnoldi_onepass_kernel (kernels_onepass.hip) shares the reduction below only:
// it keeps the quad loop written out, in the same order (the comment there says why).  gfx950, wave64.
//
// The order of the arithmetic is part of every stored-operator result's bits ("bit-identical across formats"): per quad of slots
// the column section, the four values, the four gathers, then four complex FMAs into s0, s1, s0, s1 in slot order; the caller
// adds s0 + s1 once at the end of the row.  It is written here once -- plain and through the value dictionary -- together with
// the lane-transposed reduction of the two Arnoldi kernels.  What is NOT shared is policy: every call site passes the unroll
// depth and the cache policies it was measured with.
#pragma once

#include "kernel_common.h"

namespace qp {

// nq quads of a block's (upper) section.  v: the block's value plane at this lane (slot k at v + 64 k); NTC / NTV: nontemporal
// loads of the column section / of the values (the Hermitian-packed kernel re-reads its values through the L2: NTV = false).
template <bool NTC, bool NTV, int UNR, class VT>
__device__ __forceinline__ void rowblock_quads(double2& s0, double2& s1, const char* colbytes, int64_t cm, const VT* v, int nq,
                                               int lane, int rowc, const double2* x) {
#pragma unroll UNR
  for (int q = 0; q < nq; ++q) {
    const int4 c = ld_cols<NTC>(colbytes, cm, q, lane, rowc);
    const double2 a0 = ld_val<NTV>(v + (size_t)(4 * q + 0) * 64);
    const double2 a1 = ld_val<NTV>(v + (size_t)(4 * q + 1) * 64);
    const double2 a2 = ld_val<NTV>(v + (size_t)(4 * q + 2) * 64);
    const double2 a3 = ld_val<NTV>(v + (size_t)(4 * q + 3) * 64);
    const double2 x0 = x[c.x];
    const double2 x1 = x[c.y];
    const double2 x2 = x[c.z];
    const double2 x3 = x[c.w];
    cfma(s0, a0, x0);
    cfma(s1, a1, x1);
    cfma(s0, a2, x2);
    cfma(s1, a3, x3);
  }
}

// ---- the value dictionary (device.h: CodedVals): one byte per slot + the block's table of at most 256 distinct values ----
// The block's table into the wavefront's LDS window tw (256 entries): the look-ups then go through the LDS crossbar, not
// through the vector L1 that the gathers of x keep busy (profiles/r05/value_dictionary.txt: 21 table reads per row through
// the L1 cost 8.5 of 45 us per term).  tp: the block's entry of tptr (offset << 9 | length).  Ends in the wavefront's sync; a
// caller that reuses the window syncs BEFORE the call as well.
template <class TT>
__device__ __forceinline__ void coded_stage_table(TT* tw, const TT* tab, int64_t tp, int lane) {
  const TT* tb = tab + (tp >> 9);
  const int tlen = (int)(tp & 511);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i * 64 < tlen) tw[i * 64 + lane] = tb[min(i * 64 + lane, tlen - 1)];   // (wave-uniform condition)
  wave_lds_sync();
}
// rowblock_quads with the four values of a quad looked up in tw by the four codes of one nontemporal dword (cq: the block's
// codes at this lane, quad q at cq + 64 q); the table holds the numbers the value plane would hold: the same bits
template <int UNR, class TT>
__device__ __forceinline__ void rowblock_quads_coded(double2& s0, double2& s1, const char* colbytes, int64_t cm, const unsigned* cq,
                                                     const TT* tw, int nq, int lane, int rowc, const double2* x) {
#pragma unroll UNR
  for (int q = 0; q < nq; ++q) {
    const unsigned cw = __builtin_nontemporal_load(cq + (size_t)q * 64);
    const int4 c = ld_cols<true>(colbytes, cm, q, lane, rowc);
    const double2 x0 = x[c.x];
    const double2 x1 = x[c.y];
    const double2 x2 = x[c.z];
    const double2 x3 = x[c.w];
    const double2 a0 = ld_val<false>(tw + (cw & 255u));
    const double2 a1 = ld_val<false>(tw + ((cw >> 8) & 255u));
    const double2 a2 = ld_val<false>(tw + ((cw >> 16) & 255u));
    const double2 a3 = ld_val<false>(tw + (cw >> 24));
    cfma(s0, a0, x0);
    cfma(s1, a1, x1);
    cfma(s0, a2, x2);
    cfma(s1, a3, x3);
  }
}

// ---- NV per-lane doubles summed over the lanes of a wavefront ----
// One cross-lane tree per value would be 80 dependent chains at NV = 80; instead the lanes transpose eight values at a time
// through a wavefront-private LDS tile (row = lane, nine doubles wide: conflict-free both ways): lane l then owns value l % 8
// and adds the entries of the eight lanes 8 (l / 8) .. 8 (l / 8) + 7 in order -- all 64 lanes busy, reads independent of one
// another --, and one row shift folds the eight parts into four: red_parts[wave][p][id], p < 4.  val(id): the lane's value id (called
// with constants once unrolled).  The caller's last stage (__syncthreads, then wavefronts x parts in a fixed order) and the
// slot a value takes in the partials are its own.
template <int NV, int WS, class F>
__device__ __forceinline__ void lane_transposed_sums(double (&red_tile)[WS][64 * 9], double (&red_parts)[WS][4][NV], int wave, int lane,
                                                     F val) {
  static_assert(NV % 8 == 0, "the lane transpose takes eight values at a time");
  double* __restrict__ tile = red_tile[wave];
  const int tv = lane & 7, tp = lane >> 3;
#pragma unroll
  for (int ch = 0; ch < NV / 8; ++ch) {
#pragma unroll
    for (int i = 0; i < 8; ++i) tile[lane * 9 + i] = val(8 * ch + i);
    wave_lds_sync();
    double sum = tile[(tp * 8) * 9 + tv];
#pragma unroll
    for (int i = 1; i < 8; ++i) sum += tile[(tp * 8 + i) * 9 + tv];
    sum += dpp_take<0x118, 0xf>(sum);   // row_shr:8: part 2 r + 1 (lanes 8 .. 15 of a row) += part 2 r
    if (tp & 1) red_parts[wave][tp >> 1][8 * ch + tv] = sum;
    wave_lds_sync();                    // this chunk's reads before the next chunk's writes
  }
}

}  // namespace qp
