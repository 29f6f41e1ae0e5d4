// The cut of the strip walks (walk_geometry.h).  Pure host code: no HIP header, no device query -- the chip's size is an argument.
#include "walk_geometry.h"

#include <algorithm>

namespace qp {

double walk_value_bytes(const WalkPlan& P, const WalkMatrix& M) {
  return (double)(P.z0 + P.nn + P.K * (1 + 2 * P.fd) + P.xl) * kRB * (double)M.nblocks * (M.real_vals ? 8.0 : 16.0);
}
double walk_footprint_bytes(const WalkPlan& P, const WalkMatrix& M) { return walk_value_bytes(P, M) + 64.0 * (double)M.nrows; }
bool walk_resident(const WalkPlan& P, const WalkMatrix& M) { return walk_footprint_bytes(P, M) <= 230e6; }

WalkCut walk_cut(const WalkPlan& P, const WalkMatrix& M, const WalkKnobs& k, int cu, int reserve_cu, bool row_set, bool no_edges) {
  WalkCut C;
  const int64_t nW = P.R1 - P.W0;
  if (nW < k.walk_min_blocks || nW < P.S) return C;
  WalkGeom& G = C.G;
  const int64_t J = (nW * kRB + P.g - 1) / P.g;                 // steps of the longest strip column
  // wavefronts.  While the operator and the vectors sit in the Infinity Cache, 768 wavefronts as 192 workgroups of four
  // (one per CU on three quarters of the chip) draw what it delivers: the set-up of a walk (8 + 10 loads) is paid less
  // often than with the 2048 that fill every SIMD twice, and the edge blocks run beside the walk on the free compute
  // units (profiles/r03/kbench_walk_development.txt: N = 2^20 31.9 us per term; 1280 as workgroups of eight 33.4, 2048 36.5)
  // ... and beyond it the matrix values are streamed nontemporally: they are read once per term, and what the
  // Infinity Cache then keeps from one term to the next is the vectors
  const bool resident = walk_resident(P, M);
  // beyond it: every CU but the few the edge workgroups take (8 x (256 - 24) = 1856 for the headline lattice), so that
  // the edge blocks run BESIDE the walk there too; 2048 with the edge blocks inside the walk's wavefronts when that would
  // leave more than an eighth of the chip to them (profiles/r03/kbench_walk_development.txt: 2^21 rows 71.4 -> 68.5 us,
  // 2^22 126.0 -> 121.8, 2^23 275 -> 278)
  const int ws = resident ? 4 : kWalkWaves;            // wavefronts per workgroup (two 4-wavefront workgroups fit a CU)
  const int64_t wg_slots = (int64_t)std::max(cu - reserve_cu, 8) * (kWalkWaves / ws);  // workgroups the walk may hold at once
  const int64_t edge_wgs = (P.n_edge + ws - 1) / ws;
  const int waves_beside = (int)(ws * std::max<int64_t>(0, wg_slots - edge_wgs)) / P.S * P.S;
  const int waves = k.walk_waves > 0 ? k.walk_waves
                    : resident ? (M.real_vals ? 1024 : 768)   // (real copy, half the value bytes per step: 1024; N = 2^20: 26.6 -> 24.3 us)
                    : ((row_set || waves_beside >= 7 * kWalkWaves * cu / 8) ? std::max(waves_beside, P.S) : kWalkWaves * cu);
  C.ws = ws;
  C.ntm = k.walk_nt >= 0 ? k.walk_nt : (resident ? 0 : 1);
  const int64_t nseg_target = std::max<int64_t>(1, waves / P.S);
  // edge blocks as workgroups of their own while every workgroup of the launch still finds room on the chip at once
  const bool edge_beside = !no_edges && (k.walk_dbg & 4) == 0 &&
                           (nseg_target * P.S + ws - 1) / ws + edge_wgs <= wg_slots;
  G.n_edge_wg = edge_beside ? (int)edge_wgs : 0;
  G.edge_steps = (no_edges || edge_beside) ? 0 : kWalkEdgeSteps;
  G.edge_last = (k.walk_dbg & 1) ? 1 : 0;
  G.edge_segs = (no_edges || edge_beside) ? 0 : (int)std::min<int64_t>(nseg_target, (P.n_edge + P.S - 1) / P.S);
  G.xlast = M.ncols - 1;
  G.L = (int)std::max<int64_t>(G.edge_steps + 1, (J + (int64_t)G.edge_segs * G.edge_steps + nseg_target - 1) / nseg_target);
  G.nseg = (int)((J + (int64_t)G.edge_segs * G.edge_steps + G.L - 1) / G.L);
  while ((int64_t)G.nseg * G.L - (int64_t)std::min(G.edge_segs, G.nseg) * G.edge_steps < J) ++G.nseg;   // (tiny operators)
  G.edge_segs = std::min(G.edge_segs, G.nseg);
  const int64_t ntask = (int64_t)G.nseg * P.S;
  G.n_walk_wg = (int)((ntask + ws - 1) / ws);
  G.ntask = G.n_walk_wg * ws;
  C.grid = (unsigned)(G.n_edge_wg + G.n_walk_wg);
  C.taken = true;
  return C;
}

// what both cuts of the two-term walk share: the chunks of a strip step, the strip steps of the two-term region, the segments the
// wavefront budget allows (one wavefront per SIMD unless walk_waves says otherwise).  false: no two-term kernel for this plan
static bool walk2_cut_columns(const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu, Walk2Cut& C) {
  if (!P2.valid || !walk2_shape_supported(P2.nn, P2.K, P2.z0) || P2.xl || P2.fd || P2.g % kRB) return false;
  Walk2Geom& G = C.G;
  const int dmax = P2.near[P2.nn - 1];
  G.W = kRB - 2 * dmax;
  if (G.W < 16) return false;
  G.S2 = (int)((P2.g + G.W - 1) / G.W);
  C.Jz = ((P2.R1 - P2.W0) * (int64_t)kRB + P2.g - 1) / P2.g;
  const int64_t waves = k.walk_waves > 0 ? k.walk_waves : (int64_t)kWalk2Waves * cu;   // one per SIMD
  C.nseg_target = std::max<int64_t>(1, waves / G.S2);
  G.xlast = M.ncols - 1;
  G.vend = (P2.R1 + (int64_t)P2.K * P2.S) * (int64_t)kRB;      // the one-term plan's run end
  return true;
}
static void walk2_cut_grid(Walk2Geom& G) {
  const int64_t ntask = std::max<int64_t>((int64_t)G.nseg * G.S2, 1);
  G.n_walk_wg = (int)((ntask + kWalk2Waves - 1) / kWalk2Waves);
  G.ntask = G.n_walk_wg * kWalk2Waves;
}

Walk2Cut walk2_cut(const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu) {
  Walk2Cut C;
  if (!walk2_cut_columns(P2, M, k, cu, C)) return C;
  Walk2Geom& G = C.G;
  G.L = (int)((C.Jz + C.nseg_target - 1) / C.nseg_target);
  G.nseg = (int)((C.Jz + G.L - 1) / G.L);
  walk2_cut_grid(G);
  // value loads with the default cache policy once the values are well beyond the Infinity Cache: the chunks overlap by 2 d_max rows and
  // a chunk's packed value halo is its neighbour's stream -- streamed nontemporally, each of those lines comes from memory twice
  // (N = 2^22: 103.6 -> 99.8 us per term, 2^24: 399 -> 363); while most of the values still fit the cache the nontemporal stream
  // leaves it to the vectors (2^21: 56.8 -> 54.6)
  C.ntm = k.walk_nt >= 0 ? k.walk_nt : (walk_value_bytes(P2, M) <= 300e6 ? 1 : 0);
  C.taken = true;
  return C;
}

bool walk2_wanted(const WalkPlan& P1, const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu) {
  if (!P2.valid || k.walk_pair == 0 || !P1.valid) return false;
  if (P1.R1 - P1.W0 < k.walk_min_blocks) return false;
  if (k.walk_pair == 1) return true;
  if (walk_resident(P2, M)) return false;
  const Walk2Cut C = walk2_cut(P2, M, k, cu);
  return C.taken && C.Jz / C.nseg_target >= 24;
}

Walk2Cut walk2_cut_resident(const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu) {
  Walk2Cut C;
  if (!walk2_cut_columns(P2, M, k, cu, C)) return C;
  Walk2Geom& G = C.G;
  // wavefront i < n_edge takes edge block i first (wavefronts of segment i / S2): those segments are shorter -- WalkGeom's balance,
  // walk_cut's formulas with the two-term region's steps
  const int dbg_steps = (k.walk_dbg >> kWalkDbgEdgeStepsShift) & 7;
  G.edge_steps = dbg_steps ? dbg_steps - 1 : kWalk2EdgeSteps;
  G.edge_segs = G.edge_steps ? (int)std::min<int64_t>(C.nseg_target, (P2.n_edge + G.S2 - 1) / G.S2) : 0;
  const int64_t J = C.Jz + (int64_t)G.edge_segs * G.edge_steps;
  G.L = (int)std::max<int64_t>(G.edge_steps + 1, (J + C.nseg_target - 1) / C.nseg_target);
  G.nseg = (int)((J + G.L - 1) / G.L);
  while ((int64_t)G.nseg * G.L - (int64_t)std::min(G.edge_segs, G.nseg) * G.edge_steps < C.Jz) ++G.nseg;   // (tiny operators)
  G.edge_segs = std::min(G.edge_segs, G.nseg);
  walk2_cut_grid(G);
  C.ntm = k.walk_nt >= 0 ? k.walk_nt : 0;      // the values stay in the cache from term to term: default policy, as walk_cut
  C.taken = true;
  return C;
}

bool walk2_wanted_resident(const WalkPlan& P1, const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu) {
  if (!P2.valid || !P1.valid || k.walk_pair == 0 || k.walk_pair == 1) return false;
  if (P1.R1 - P1.W0 < k.walk_min_blocks) return false;
  const Walk2Cut C = walk2_cut_resident(P2, M, k, cu);
  if (k.walk_pair == 2) return C.taken;
  // not for the real copy of the values: a pair saves half as many bytes there and pays the same run-in and follow-up launch
  // (N = 2^20: one-term walk 24.7 us per term, resident pair cut 28.3)
  if (M.real_vals) return false;
  return walk_resident(P2, M) && C.taken && C.Jz / C.nseg_target >= kWalk2ResidentMinSteps;
}

Walk2Rule walk2_rule(const WalkPlan& P1, const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu) {
  if (k.walk_pair == 2) return walk2_wanted_resident(P1, P2, M, k, cu) ? kWalk2Resident : kWalk2None;
  if (walk2_wanted(P1, P2, M, k, cu)) return kWalk2Streamed;
  return kWalk2ResidentAuto && walk2_wanted_resident(P1, P2, M, k, cu) ? kWalk2Resident : kWalk2None;
}

Walk2Cut walk2_cut_of(Walk2Rule rule, const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu) {
  return rule == kWalk2Resident ? walk2_cut_resident(P2, M, k, cu) : rule == kWalk2Streamed ? walk2_cut(P2, M, k, cu) : Walk2Cut();
}

}  // namespace qp
