// Strip walk of the fused Chebyshev term: host side (the launch, cut by walk_geometry.cpp; dispatch over the kernel shapes) and the translation
// unit of the complex-valued shapes with 3-4 near distances -- the headline's (4, 4).  The kernel itself: kernels_walk_impl.h.
#include "kernels_walk_impl.h"

namespace qp {

bool walk_launch_c128_hi(hipStream_t s, dim3 grid, const double2* uvals, const double2* x, const WalkPlan& P, const WalkGeom& G,
                         const HrbArrays& H, int64_t nrows, const ChebyOp& op, int ntm, const SyncArgs& sy) {
  return launch_shape<double2, 0>(s, grid, uvals, x, P, G, H, nrows, op, ntm, sy);
}

int launch_hrb_walk_cheby(hipStream_t s, const DevMatrix& A, const double2* x, const ChebyEpi& e, const Tuning& tun,
                          bool* launched, const RowSet* rs) {
  *launched = false;
  const WalkPlan* P = (rs && rs->walk) ? rs->walk : A.walk;
  const SyncArgs sy = rs ? rs->sync : SyncArgs();
  const int reserve = rs ? rs->reserve_cu : 0;
  if (!P || !P->valid || A.format != QP_FMT_HRB) return QP_OK;
#ifdef QP_DEVELOPER
  const bool no_edges = (tun.walk_dbg & 2) != 0;   // measurement only, developer builds only: the edge blocks are skipped, results are WRONG
#else
  const bool no_edges = false;
#endif
  // how the launch is cut into wavefronts, segments and edge work: walk_geometry.cpp
  const WalkCut C = walk_cut(*P, walk_matrix(A), walk_knobs(tun), device_cu_count(), reserve, rs != nullptr, no_edges);
  if (!C.taken) return QP_OK;
  const WalkGeom& G = C.G;
  const int ntm = C.ntm;
  const HrbArrays H = hrb_arrays(A);
  ChebyOp op{e};
  const dim3 grid(C.grid);
  WalkPlan Pl = *P;
  if (no_edges) Pl.n_edge = 0;
  const bool hi = Pl.nn >= 3 && !Pl.xl;   // which translation unit holds the shape
  const bool xlu = Pl.xl && !(Pl.xl == 1 && Pl.K == 1);
  const bool ok = Pl.fd ? (A.vals_r ? walk_launch_f64_fd(s, grid, A.vals_r, x, Pl, G, H, A.nrows, op, ntm, sy)
                                    : walk_launch_c128_fd(s, grid, A.vals, x, Pl, G, H, A.nrows, op, ntm, sy))
                  : A.vals_r ? (xlu  ? walk_launch_f64_xl(s, grid, A.vals_r, x, Pl, G, H, A.nrows, op, ntm, sy)
                              : hi ? walk_launch_f64_hi(s, grid, A.vals_r, x, Pl, G, H, A.nrows, op, ntm, sy)
                                   : walk_launch_f64_lo(s, grid, A.vals_r, x, Pl, G, H, A.nrows, op, ntm, sy))
                           : (xlu  ? walk_launch_c128_xl(s, grid, A.vals, x, Pl, G, H, A.nrows, op, ntm, sy)
                              : hi ? walk_launch_c128_hi(s, grid, A.vals, x, Pl, G, H, A.nrows, op, ntm, sy)
                                   : walk_launch_c128_lo(s, grid, A.vals, x, Pl, G, H, A.nrows, op, ntm, sy));
  if (!ok) return QP_OK;
  QP_HIP(hipGetLastError());
  *launched = true;
  return QP_OK;
}

}  // namespace qp
