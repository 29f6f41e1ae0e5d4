// Row-block mat-vec through the value-dictionary mirror (device.h: CodedVals) -- gfx950, wave64.
//
// The operator's values are a few distinct numbers (a spin chain's couplings and its handful of diagonal energies, a grid's
// hopping amplitudes; the reference's generators are sums of such terms, src/generators.jl:634-645): every 64-row block carries
// one byte per stored entry and a table of the distinct values it holds.  One wavefront per row block, lane = row, exactly as
// rbcsr_spmv_kernel (kernels.hip): per quad of slots one 4-byte load of the four codes (256 B per wavefront instead of 4 KiB of
// complex values), the column section as stored, then four table reads -- from the block's table of at most 256 entries, which the
// wavefront copies into its LDS window first -- and the four gathers.  The partial sums
// alternate between two accumulators in slot order as in rbcsr_spmv_kernel and the table holds the numbers the value plane
// would hold, so the result is bit-identical to the uncoded path.
#include <type_traits>

#include "kernel_common.h"
#include "rowblock_sum.h"

namespace qp {

template <class Op, class TT, int WS>   // TT: double2, or double for an all-real operator; WS row blocks per workgroup
__global__ __launch_bounds__(64 * WS) void rbcsr_coded_spmv_kernel(const int64_t* __restrict__ bptr,
                                                                    const int64_t* __restrict__ cmeta,
                                                                    const char* __restrict__ colbytes,
                                                                    const unsigned* __restrict__ codes4,
                                                                    const int64_t* __restrict__ tptr,
                                                                    const TT* __restrict__ tab,
                                                                    const double2* __restrict__ x, int64_t nblocks,
                                                                    int64_t nrows, Op op,
                                                                    const int32_t* __restrict__ block_map, SyncArgs sy) {
  static_assert(WS == kThreads / 64 || std::is_same<Op, ChebyOp>::value,
                "block_sum (Op::begin of the folded norm, finish_check) sums kThreads / 64 wavefronts");
  __shared__ double2 lds[WS];
  __shared__ TT tabs[WS][256];
  const unsigned wg = xcd_remap(blockIdx.x, gridDim.x);
  sync_wait(sy, wg);
  op.begin_issue();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int64_t idx = (int64_t)wg * WS + wave;   // position in the row set
  double2 chk = make_double2(0.0, 0.0);
  double nrm = 0.0;
  int64_t row = nrows;
  typename Op::Pre pre;
  double2 s0 = make_double2(0.0, 0.0), s1 = make_double2(0.0, 0.0);
  if (idx < nblocks) {
    const int64_t b = block_map ? (int64_t)block_map[idx] : idx;
    const int64_t base = bptr[b];
    const int nq = (int)((bptr[b + 1] - base) >> 8);   // slots / 4
    const unsigned* __restrict__ cq = codes4 + (base >> 2) + lane;
    const int64_t cm = cmeta[b];
    row = b * kRB + lane;
    const int64_t rowc = row < nrows ? row : nrows - 1;
    pre = op.pre(rowc);
    TT* __restrict__ tw = tabs[wave];
    coded_stage_table(tw, tab, tptr[b], lane);
    rowblock_quads_coded<4>(s0, s1, colbytes, cm, cq, tw, nq, lane, (int)rowc, x);
  }
  op.begin(lds);
  if (row < nrows) op.row(row, make_double2(s0.x + s1.x, s0.y + s1.y), pre, chk, nrm, idx * kRB + lane);
  finish_check(op, chk, nrm, lds);
  sync_signal(sy);
}

template <class Op, int WS>
static int launch_coded(hipStream_t s, const DevMatrix& A, const double2* x, const Op& op, int64_t nblk, const int32_t* bmap,
                        const SyncArgs& sy) {
  const CodedVals& C = *A.cv;
  const dim3 grid((unsigned)((nblk + WS - 1) / WS));
  const unsigned* codes4 = reinterpret_cast<const unsigned*>(C.codes);
  with_values(C.use_real ? C.tab_r : nullptr, C.tab, [&](auto* tab) {
    hipLaunchKernelGGL((rbcsr_coded_spmv_kernel<Op, pointee_t<decltype(tab)>, WS>), grid, dim3(64 * WS), 0, s, A.bptr, A.cmeta,
                       reinterpret_cast<const char*>(A.cols), codes4, C.tptr, tab, x, nblk, A.nrows, op, bmap, sy);
  });
  QP_HIP(hipGetLastError());
  return QP_OK;
}

// wide: eight row blocks per workgroup (the plain fused term of a whole operator or of an interior launch: no per-workgroup
// check partials, no completion signal, no mirror map -- launch_spmv decides); the wait threshold is given in workgroups of four
int launch_rbcsr_coded_cheby(hipStream_t s, const DevMatrix& A, const double2* x, const ChebyEpi& e, int64_t nblk,
                             const int32_t* bmap, const SyncArgs& sy, bool wide) {
  ChebyOp op{e};
  if (wide) {
    SyncArgs sy8 = sy;
    sy8.wait_from_wg = sy.wait_from_wg / 2;
    return launch_coded<ChebyOp, 8>(s, A, x, op, nblk, bmap, sy8);
  }
  return launch_coded<ChebyOp, kThreads / 64>(s, A, x, op, nblk, bmap, sy);
}

int launch_rbcsr_coded_plain(hipStream_t s, const DevMatrix& A, const double2* x, const PlainEpi& e, int64_t nblk,
                             const int32_t* bmap, const SyncArgs& sy) {
  PlainOp op{e};
  return launch_coded<PlainOp, kThreads / 64>(s, A, x, op, nblk, bmap, sy);
}

}  // namespace qp
