// Strip walks of a Hermitian-packed lattice operator (kernels_walk_impl.h, kernels_walk2_impl.h): the plan, the launch geometry
// the kernels take as arguments, and the CUT -- how a launch is divided into wavefronts, segments and edge work -- as pure
// functions of plain numbers.  No HIP: the launchers (kernels_walk.hip, kernels_walk2.hip), qp_operator_walk2_info and the
// sanitizer harness (tests/sanitize_host_index.cpp, which checks on the CPU that every strip step belongs to exactly one
// segment) all call the same functions.
#pragma once

#include <cstdint>

#include "layout_constants.h"

namespace qp {

// ---- strip walk over a lattice operator (Hermitian-packed format) -----------------------------------------------
// A run of row blocks [R0, R1) that all carry the same stencil: upper section
//   [z0 slots at distance 0 (the diagonal)] [nn near distances 0 < d_1 < ... < d_nn <= 16] [K far distances m g, m = 1..K]
//   [pads], lower section its mirror image [-K g ... -g] [-d_nn ... -d_1]; S = ceil(g / 64) column chunks per strip step.  Inside the run the position of
// every value is a formula (U0 + (b - R0) ustride + 64 slot + lane), and a wavefront that WALKS down one strip column --
// row blocks b, b + S, b + 2 S, ... -- finds everything a block needs beyond its own streams in what it loaded for the
// blocks before: the gathered elements x[r + m g] are the row-local elements of the blocks m steps ahead / behind (a ring
// of 2 K + 1 registers, one new load per step), the conj-transposed values of the far lower entries are the far upper
// values it streamed m steps ago (a FIFO in LDS), the near gathers and the near conj-transposed values are lane shifts
// of the block's own element / values, staged through a per-wavefront LDS window with a halo of the neighbouring block.
// Blocks outside [W0, R1) (W0 = R0 + K S: the first blocks whose history lies inside the run; the periodic wrap-around,
// a ragged end) are listed in edge_map and take the per-block code path in the same launch.
constexpr int kWalkMaxNear = 8;
constexpr int kWalkHalo = 16;      // largest near distance
struct WalkPlan {
  int valid = 0;
  int nn = 0, K = 0, z0 = 0;  // shape of the stencil (see above)
  int S = 0;                  // 64-row column chunks per strip step: ceil(g / 64)
  int xl = 0;                 // 1: one more pair of distances +- glong beyond the ring's reach (loaded directly); 2: two, +- glong1 and +- glong
  int64_t glong = 0;          // the longest distance of the stencil
  int64_t glong1 = 0;         // xl = 2: the shorter long distance, K g < glong1 < glong
  int fd = 0;                 // 1: diagonal far neighbours -- the far distances of strip step m are m g - 1, m g, m g + 1 (three slots per step)
  int64_t g = 0;              // rows per strip step (the far distances are g, 2 g, .., K g); need not be a multiple of 64
  int near[kWalkMaxNear] = {0};
  int64_t R0 = 0, R1 = 0, W0 = 0;
  int64_t U0 = 0;             // bptr[R0]
  int ustride = 0;            // stored upper values per row block (64 x padded width)
  int32_t* edge_map = nullptr;   // device: the blocks outside [W0, R1)
  int64_t n_edge = 0;
};

// entry `idx` of a plan's edge list (operator_plans.cpp builds edge_map from this): the blocks below W0, then those from R1 on.
// (constexpr: host and device code alike)
constexpr int64_t walk_edge_block(int64_t W0, int64_t R1, int64_t idx) { return idx < W0 ? idx : R1 + (idx - W0); }

// is there a strip-walk kernel instance for this stencil shape?  (The dispatch of kernels_walk_impl.h: launch_shape instantiates
// exactly these; inline here so that the host planners -- and their sanitizer build, tests/sanitize_host_index.cpp -- see the same list.)
// near distances 1..4 of at most 16 rows, far reach 1..4 strip steps, with or without a diagonal
// ... and, with one or two long pairs beyond the ring (xl = 1, 2), near 1..2 and one or two far distances
// ... and, with diagonal far neighbours (fd = 1: m g - 1, m g, m g + 1), near 1..2, one strip step and at most one long pair
inline bool walk_shape_supported(int nn, int K, int z0, int xl = 0, int fd = 0) {
  if (fd) return fd == 1 && (xl == 0 || xl == 1) && K == 1 && nn >= 1 && nn <= 2 && (z0 == 0 || z0 == 1);
  if (xl) return (xl == 1 || xl == 2) && nn >= 1 && nn <= 2 && (K == 1 || K == 2) && (z0 == 0 || z0 == 1);
  return nn >= 1 && nn <= 4 && K >= 1 && K <= 4 && (z0 == 0 || z0 == 1);
}
// the two-term strip walk (kernels_walk2.hip): both terms of a pair (m, m + 1) on the two-term region of plan `P2`, term m of its edge list
inline bool walk2_shape_supported(int nn, int K, int z0) {
  return (z0 == 0 || z0 == 1) && nn >= 1 && nn <= 4 && K >= 1 && K <= 4;
}

// ---- kernel arguments (member order and types are the kernels' ABI) ------------------------------------------------
struct WalkGeom {
  int L = 0;           // steps per wavefront
  int nseg = 0;        // segments of L steps per strip column
  int n_walk_wg = 0;
  int ntask = 0;       // wavefronts of the walk (n_walk_wg x wavefronts per workgroup)
  // Edge blocks (outside the walkable run), two schemes:
  //  * beside the walk (n_edge_wg > 0): workgroups of their own at the head of the grid, one block per wavefront, while
  //    every workgroup of the launch still finds room on the chip at once -- the walk is cut so that it does (768
  //    wavefronts inside the Infinity Cache, 8 per CU on all but the CUs the edge workgroups take beyond it);
  //  * inside the walk (n_edge_wg == 0; knob walk_waves / walk_dbg): edge block i goes to wavefront i, BEFORE its walk
  //    (edge_last: after), and the segments of those wavefronts are `edge_steps` steps shorter -- a block on the per-block
  //    path is three dependent rounds of loads, a step of the walk about one -- so that every wavefront finishes at
  //    about the same time.  (As leading workgroups of a launch that fills every CU they cost 5-6 us: whichever compute
  //    units ran them started their walk that much later.)
  int edge_segs = 0;   // segments 0 .. edge_segs - 1 are the shorter ones
  int edge_steps = 0;
  int edge_last = 0;
  int64_t xlast = 0;   // last element of x (columns of a row-partitioned operator run beyond its rows: the halo slabs)
  int n_edge_wg = 0;
};

struct Walk2Geom {
  int L = 0, nseg = 0, ntask = 0, n_walk_wg = 0;
  int S2 = 0;          // column chunks per strip step: ceil(g / W)
  int W = 0;           // rows of a chunk that form z: 64 - 2 d_max
  int64_t xlast = 0;   // last element of x
  int64_t vend = 0;    // first row beyond the lattice run (values at the run's strides exist below it)
  // the one-term walk's balance (WalkGeom): wavefront i < n_edge takes edge block i before its walk, and segments
  // 0 .. edge_segs - 1 -- theirs -- are `edge_steps` steps shorter.  0: every segment has L steps (walk2_cut)
  int edge_segs = 0;
  int edge_steps = 0;
};

constexpr int kWalkWaves = 8;       // most wavefronts (adjacent strip columns) per workgroup; the launch may use fewer (knob walk_wg)
constexpr int kWalk2Waves = 4;      // two-term walk: wavefronts per workgroup = per compute unit: one per SIMD
constexpr int kWalkEdgeSteps = 4;   // strip walk: a wavefront that also takes an edge block walks this many steps less (a block on the per-block path is three dependent rounds of loads; a step of the walk takes about one)
constexpr int kWalkReserveCu = 8;   // compute units an interior strip walk leaves to the boundary launch and the collective's kernel (was a knob while it was being measured: docs/history/)

// ---- the cut ----------------------------------------------------------------------------------------------------------
// what a cut reads of the operator and of the context's knobs (device.h: walk_matrix, walk_knobs)
struct WalkMatrix {
  int64_t nblocks = 0, nrows = 0, ncols = 0;
  bool real_vals = false;    // the kernels stream the real copy of the values (8 bytes per value instead of 16)
};
struct WalkKnobs {
  int walk_waves = 0, walk_nt = -1, walk_dbg = 0, walk_min_blocks = 3072, walk_pair = -1;
};

// bytes of matrix values a term streams (the pad slots of the quad-padded upper sections are never read), and with the vectors:
// the operator "fits the Infinity Cache" while the footprint is at most 230e6 bytes
double walk_value_bytes(const WalkPlan& P, const WalkMatrix& M);
double walk_footprint_bytes(const WalkPlan& P, const WalkMatrix& M);
bool walk_resident(const WalkPlan& P, const WalkMatrix& M);

struct WalkCut {
  bool taken = false;   // false: the plan is too small for the walk (the caller takes the per-block kernel)
  int ws = 0;           // wavefronts per workgroup: 4 or 8
  int ntm = 0;          // nontemporal accesses (template parameter NTM of hrb_walk_kernel)
  unsigned grid = 0;    // workgroups: edge workgroups first, then the walk's
  WalkGeom G;
};
// One-term walk of plan `P` on a chip of `cu` compute units of which `reserve_cu` stay free; `row_set`: the launch covers a
// row set (interior of a split term); `no_edges`: developer builds' measurement knob (edge blocks skipped).
WalkCut walk_cut(const WalkPlan& P, const WalkMatrix& M, const WalkKnobs& k, int cu, int reserve_cu, bool row_set, bool no_edges);

struct Walk2Cut {
  bool taken = false;   // false: no two-term kernel for this plan (shape, or fewer than 16 rows of a chunk would form z)
  int ntm = 0;
  int64_t Jz = 0;            // strip steps of the two-term region
  int64_t nseg_target = 0;   // segments per strip column the wavefront budget allows
  Walk2Geom G;
};
Walk2Cut walk2_cut(const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu);

// Does a whole-operator cheby! take the two-term walk of `P2` (P1: the operator's one-term plan) with walk2_cut?  Beyond the Infinity
// Cache only (inside it: walk2_wanted_resident below), and only when a wavefront's strip column is long enough for
// the 2 K steps a segment runs in before its first z to be a small part of it.
bool walk2_wanted(const WalkPlan& P1, const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu);

// ---- the two-term walk of an operator INSIDE the Infinity Cache -------------------------------------------------------
// What a pair costs there beyond its value stream is the run-in (2 K steps per segment) and the edge blocks its wavefronts take
// first.  So the cut gives the wavefronts with an edge block shorter segments (Walk2Geom::edge_segs / edge_steps), and the value
// loads keep the default cache policy.  Measured at N = 2^20 (profiles/walk2_resident.txt), us per term.  Against each other, in
// regions of 20 steps: one wavefront per SIMD 30.9, 760 wavefronts 34.5, 608 38.7 (fewer only lengthen the launch); edge_steps
// 0 / 2 / 3 / 4: 31.9 / 31.3 / 30.9 / 31.5; nontemporal values 34.5; walk2_cut with its nontemporal values 35.4.  Against the
// one-term walk, in regions of 60 steps (the figures that agree with bench.py's 100): 29.9 against 30.75 (the short regions give the
// pair about 1 us more and the one-term walk 0.2 less; why is not known).  The real copy of the values: 28.3 against 24.7 -- not taken.
constexpr int kWalk2EdgeSteps = 3;           // steps a segment with an edge block is shorter
constexpr bool kWalk2ResidentAuto = true;    // the automatic rule (walk_pair = -1) takes walk2_wanted_resident's verdict (bench.py: + 5.9 %)
// automatic rule: a wavefront's share of the strip column, at least.  Measured at ONE point only -- 19 steps, the (4, 4) lattice at
// N = 2^20, 2 K = 8 of run-in; nothing between 4 (2^18) and 19 steps and no other shape was measured: 16 keeps the rule to what was
constexpr int kWalk2ResidentMinSteps = 16;
// knob walk_dbg (measurements only), beyond the one-term walk's bits 1, 2, 4:
constexpr int kWalkDbgPairFollowUpPerBlock = 8;   // term m + 1 of a pair's edge blocks by the per-block kernel (row set) instead of hrb_walk2_edge_kernel
constexpr int kWalkDbgEdgeStepsShift = 4;         // bits 16 | 32 | 64 = n > 0: walk2_cut_resident with edge_steps = n - 1
Walk2Cut walk2_cut_resident(const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu);
// The automatic rule inside the cache: the operator is resident, its values are complex (M.real_vals: measured, a loss), its shape
// has a pair kernel, and a wavefront's segment is at
// least kWalk2ResidentMinSteps long (the headline lattice at N = 2^20 on 256 compute units: 19; at 2^16: 1).  walk_pair = 2
// forces it at any size; 0 and 1 never take it.
bool walk2_wanted_resident(const WalkPlan& P1, const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu);

// Which cut a whole-operator cheby! takes its pairs with -- kWalk2None: one-term launches; kWalk2Streamed: walk2_cut (walk2_wanted,
// walk_pair = 1); kWalk2Resident: walk2_cut_resident (walk2_wanted_resident, walk_pair = 2) -- and that cut
enum Walk2Rule { kWalk2None = 0, kWalk2Streamed = 1, kWalk2Resident = 2 };
Walk2Rule walk2_rule(const WalkPlan& P1, const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu);
Walk2Cut walk2_cut_of(Walk2Rule rule, const WalkPlan& P2, const WalkMatrix& M, const WalkKnobs& k, int cu);

}  // namespace qp
