// Two-term strip walk (kernels_walk2_impl.h): host side (the launch, cut by walk_geometry.cpp; dispatch over the kernel shapes) and the translation unit of the
// shapes with four near distances -- the headline's (4, 4).
#include "kernels_walk2_impl.h"

namespace qp {

QP_WALK2_DEFINE(walk2_launch_nn4, 4)

// Term m + 1 of the blocks outside the two-term region, after the pair's walk: one edge block per wavefront on the latency-arranged
// per-block path (kernels_walk_impl.h: hrb_edge_block -- three dependent rounds of loads, the per-block kernel's sums).  One
// wavefront per workgroup: the launch is a chain of load latencies, and spread over every compute unit it is shortest (N = 2^20,
// 320 blocks: 29.89 us per term of the step against 29.97 - 30.06 with four per workgroup).  The block comes from the plan's bounds
// (walk_edge_block), not from edge_map: one dependent load less.  No LDS, no hand-off: the launch follows the walk in stream order.
template <class VT>
__global__ __launch_bounds__(64) void hrb_walk2_edge_kernel(const VT* __restrict__ uvals, const double2* __restrict__ x, WalkPlan P,
                                                             HrbArrays H, int64_t nrows, ChebyOp op2) {
  const int64_t idx = blockIdx.x;
  if (idx >= P.n_edge) return;
  hrb_edge_block<VT>(H, uvals, x, walk_edge_block(P.W0, P.R1, idx), (int)threadIdx.x, nrows, op2);
}

int launch_hrb_walk2_edge_cheby(hipStream_t s, const DevMatrix& A, const WalkPlan& P2, const double2* x, const ChebyEpi& e2) {
  if (P2.n_edge <= 0) return QP_OK;
  const HrbArrays H = hrb_arrays(A);
  const ChebyOp op2{e2};
  const unsigned grid = (unsigned)P2.n_edge;
  if (A.vals_r)
    hipLaunchKernelGGL(hrb_walk2_edge_kernel<double>, dim3(grid), dim3(64), 0, s, A.vals_r, x, P2, H, A.nrows, op2);
  else
    hipLaunchKernelGGL(hrb_walk2_edge_kernel<double2>, dim3(grid), dim3(64), 0, s, A.vals, x, P2, H, A.nrows, op2);
  QP_HIP(hipGetLastError());
  return QP_OK;
}

// Both terms of a pair on the two-term region of `P2` (walk_geometry.h: walk2_shape_supported; the plan's edge list = every block
// outside the region) + term m of the edge list.  *launched = false: not taken (the caller issues two one-term launches).
// The caller follows up with term m + 1 of the edge list (launch_hrb_walk2_edge_cheby above).
int launch_hrb_walk2_cheby(hipStream_t s, const DevMatrix& A, const WalkPlan& P2, const double2* x, const ChebyEpi& e1,
                           const ChebyEpi& e2, const Tuning& tun, Walk2Rule rule, bool* launched) {
  *launched = false;
  if (A.format != QP_FMT_HRB) return QP_OK;
  if (!e1.v0 || e1.check_partials || e2.check_partials || e1.mirror || e2.mirror || e1.xloc != x) return QP_OK;
  // the cut and the cache policy of the value stream: walk_geometry.cpp
  const Walk2Cut C = walk2_cut_of(rule, P2, walk_matrix(A), walk_knobs(tun), device_cu_count());
  if (!C.taken) return QP_OK;
  const Walk2Geom& G = C.G;
  const int ntm = C.ntm;
  const HrbArrays H = hrb_arrays(A);
  ChebyOp op1{e1}, op2{e2};
  bool ok = false;
  switch (P2.nn) {
#define QP_WALK2_CASE(NN_)                                                                                   \
  case NN_:                                                                                                  \
    ok = A.vals_r ? walk2_launch_nn##NN_##_f64(s, A.vals_r, x, P2, G, H, A.nrows, op1, op2, ntm)                \
                  : walk2_launch_nn##NN_##_c128(s, A.vals, x, P2, G, H, A.nrows, op1, op2, ntm);                \
    break;
    QP_WALK2_CASE(1)
    QP_WALK2_CASE(2)
    QP_WALK2_CASE(3)
    QP_WALK2_CASE(4)
#undef QP_WALK2_CASE
    default: break;
  }
  if (!ok) return QP_OK;
  QP_HIP(hipGetLastError());
  *launched = true;
  return QP_OK;
}

}  // namespace qp
