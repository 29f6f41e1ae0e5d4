// The two-term strip walk's cut and rule for operators INSIDE the Infinity Cache (csrc/walk_geometry.cpp: walk2_cut_resident,
// walk2_wanted_resident, walk2_rule) on the CPU: built from walk_geometry.cpp alone by tests/test_walk2_resident_host.py.
//  * the cut, swept over chip sizes, wavefront budgets, edge steps and three lattice plans, against hrb_walk2_kernel's own segment
//    formulas: every strip step of the two-term region in exactly one segment (the shortened ones included), the launch holds
//    every segment's wavefronts, edge_segs <= nseg, L > edge_steps;
//  * the rule on named inputs;
//  * walk2_cut / walk2_wanted (pinned by tests/walk_geometry_cases.h) untouched: no shortened segments, the headline not wanted.
// The plans are written down from the layout rules (a periodic lattice's first and last K S row blocks wrap around and are edge
// blocks of the one-term plan; the two-term region is K S blocks shorter at either end), as tests/walk_geometry_cases.h does.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "walk_geometry.h"

using namespace qp;

static int g_fail = 0;
#define REQUIRE(cond, ...)                       \
  do {                                           \
    if (!(cond)) {                               \
      std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                  \
      std::printf("\n");                         \
      ++g_fail;                                  \
    }                                            \
  } while (0)

struct Lattice {
  const char* name;
  int nn, K, z0;
  long long g;
  int near[4];
  long long nblocks;
  int real;
};

// one-term plan P1 and two-term plan P2 of a periodic lattice of `nblocks` row blocks
static void plans_of(const Lattice& l, WalkPlan& P1, WalkPlan& P2, WalkMatrix& M) {
  WalkPlan P;
  P.valid = 1;
  P.nn = l.nn;
  P.K = l.K;
  P.z0 = l.z0;
  P.g = l.g;
  P.S = (int)((l.g + kRB - 1) / kRB);
  for (int i = 0; i < l.nn; ++i) P.near[i] = l.near[i];
  const long long ks = (long long)l.K * P.S;
  P.R0 = ks;
  P.R1 = l.nblocks - ks;
  P.W0 = P.R0 + ks;
  P.n_edge = l.nblocks - (P.R1 - P.W0);
  P1 = P;
  P2 = P;
  P2.W0 = P1.W0 + ks;
  P2.R1 = P1.R1 - ks;
  P2.n_edge = l.nblocks - (P2.R1 - P2.W0);
  M.nblocks = l.nblocks;
  M.nrows = M.ncols = l.nblocks * kRB;
  M.real_vals = l.real != 0;
}

static const Lattice kHeadline20 = {"headline (4, 4) g = 1024, N = 2^20", 4, 4, 0, 1024, {1, 2, 3, 4}, 16384, 0};
static const Lattice kHeadline20Real = {"headline, real copy, N = 2^20", 4, 4, 0, 1024, {1, 2, 3, 4}, 16384, 1};
static const Lattice kHeadline22 = {"headline, N = 2^22", 4, 4, 0, 1024, {1, 2, 3, 4}, 65536, 0};
static const Lattice kHeadline15 = {"(4, 4) g = 1024, N = 2^15", 4, 4, 0, 1024, {1, 2, 3, 4}, 512, 0};
static const Lattice kHeadline16 = {"(4, 4) g = 1024, N = 2^16", 4, 4, 0, 1024, {1, 2, 3, 4}, 1024, 0};
static const Lattice kSmall44 = {"(4, 4) g = 128, N = 2^15", 4, 4, 0, 128, {1, 2, 3, 4}, 512, 0};
static const Lattice kSmall22 = {"(2, 2) + diagonal g = 64, N = 2^13, real copy", 2, 2, 1, 64, {1, 2, 0, 0}, 128, 1};

static long long g_all_short = 0, g_some_short = 0;   // cuts whose every segment is shortened / whose first segments only

static long long sweep_cut(const Lattice& l) {
  WalkPlan P1, P2;
  WalkMatrix M;
  plans_of(l, P1, P2, M);
  long long cuts = 0;
  for (int cu : {8, 64, 256})
    for (int waves : {0, 1, 64, 4096})
      for (int dbg_steps = 0; dbg_steps <= 7; ++dbg_steps) {
        WalkKnobs k;
        k.walk_waves = waves;
        k.walk_min_blocks = 16;
        k.walk_pair = 2;
        k.walk_dbg = dbg_steps << kWalkDbgEdgeStepsShift;
        const Walk2Cut C = walk2_cut_resident(P2, M, k, cu);
        REQUIRE(C.taken, "%s cu %d waves %d", l.name, cu, waves);
        const Walk2Geom& G = C.G;
        const int want_steps = dbg_steps ? dbg_steps - 1 : kWalk2EdgeSteps;
        REQUIRE(G.edge_steps == want_steps, "%s: edge_steps %d", l.name, G.edge_steps);
        REQUIRE(C.ntm == 0, "%s: resident values are loaded with the default policy", l.name);
        REQUIRE(G.W == kRB - 2 * l.near[l.nn - 1] && G.S2 == (l.g + G.W - 1) / G.W, "%s: W %d S2 %d", l.name, G.W, G.S2);
        REQUIRE(G.ntask == kWalk2Waves * G.n_walk_wg && (long long)G.ntask >= (long long)G.nseg * G.S2, "%s cu %d waves %d: ntask %d nseg %d S2 %d",
                l.name, cu, waves, G.ntask, G.nseg, G.S2);
        REQUIRE(G.edge_segs >= 0 && G.edge_segs <= G.nseg, "%s cu %d waves %d: edge_segs %d nseg %d", l.name, cu, waves, G.edge_segs, G.nseg);
        REQUIRE(G.L > G.edge_steps, "%s cu %d waves %d: L %d edge_steps %d", l.name, cu, waves, G.L, G.edge_steps);
        REQUIRE(G.xlast == M.ncols - 1 && G.vend == (P2.R1 + (long long)P2.K * P2.S) * kRB, "%s: xlast / vend", l.name);
        // the kernel's formulas (kernels_walk2_impl.h), every task of the launch
        const long long Jz = ((P2.R1 - P2.W0) * (long long)kRB + P2.g - 1) / P2.g;
        REQUIRE(C.Jz == Jz, "%s: Jz", l.name);
        std::vector<int> hit((size_t)Jz, 0);
        for (int task = 0; task < G.ntask; ++task) {
          const int seg = task / G.S2, col = task - seg * G.S2;
          if (seg >= G.nseg || col != 0) continue;
          const long long j0 = (long long)seg * G.L - (long long)std::min(seg, G.edge_segs) * G.edge_steps;
          const long long j1 = std::min<long long>((long long)(seg + 1) * G.L - (long long)std::min(seg + 1, G.edge_segs) * G.edge_steps, Jz);
          REQUIRE(j0 >= 0, "%s: j0 %lld", l.name, j0);
          for (long long j = j0; j < j1; ++j) hit[(size_t)j]++;
        }
        long long bad = 0;
        for (long long j = 0; j < Jz; ++j) bad += hit[(size_t)j] != 1;
        REQUIRE(bad == 0, "%s cu %d waves %d edge_steps %d: %lld of %lld strip steps not in exactly one segment (L %d nseg %d edge_segs %d)",
                l.name, cu, waves, G.edge_steps, bad, Jz, G.L, G.nseg, G.edge_segs);
        // the wavefronts with an edge block on their first round are those of the shortened segments (as far as the budget goes)
        if (G.edge_steps > 0 && P2.n_edge <= (long long)G.nseg * G.S2)
          REQUIRE((long long)G.edge_segs * G.S2 >= P2.n_edge, "%s: edge_segs %d cover %lld edge blocks", l.name, G.edge_segs, (long long)P2.n_edge);
        if (waves == 1) REQUIRE(P2.n_edge > G.ntask, "%s: walk_waves = 1 gives a wavefront several edge blocks", l.name);
        if (G.edge_steps > 0) ++(G.edge_segs == G.nseg ? g_all_short : g_some_short);
        // the streamed cut of the same inputs has no shortened segments
        k.walk_pair = 1;
        const Walk2Cut C1 = walk2_cut(P2, M, k, cu);
        REQUIRE(C1.taken && C1.G.edge_segs == 0 && C1.G.edge_steps == 0, "%s: walk2_cut moved", l.name);
        ++cuts;
      }
  return cuts;
}

struct RuleCase {
  const char* name;
  const Lattice* l;
  int walk_pair, walk_min_blocks, cu;
  int want_resident;   // walk2_wanted_resident
  int want_rule;       // walk2_rule
};

int main() {
  long long cuts = 0;
  for (const Lattice* l : {&kHeadline20, &kSmall44, &kSmall22}) cuts += sweep_cut(*l);
  REQUIRE(g_all_short > 0 && g_some_short > 0, "the sweep reaches both forms: %lld cuts with every segment shortened, %lld with the first ones", g_all_short, g_some_short);
  std::printf("resident cut: %lld cuts of 3 lattice plans hold the kernel's segment formulas (%lld with every segment shortened)\n", cuts, g_all_short);

  const RuleCase rules[] = {
      {"headline 2^20 on 256 compute units", &kHeadline20, -1, 3072, 256, 1, kWalk2ResidentAuto ? kWalk2Resident : kWalk2None},
      {"headline 2^20, real copy: measured slower than the one-term walk, not wanted", &kHeadline20Real, -1, 3072, 256, 0, kWalk2None},
      {"headline 2^20, real copy, walk_pair = 2", &kHeadline20Real, 2, 3072, 256, 1, kWalk2Resident},
      {"(4, 4) g = 1024 at 2^15", &kHeadline15, -1, 3072, 256, 0, kWalk2None},
      {"(4, 4) g = 1024 at 2^15, walk_min_blocks = 16", &kHeadline15, -1, 16, 256, 0, kWalk2None},
      {"(4, 4) g = 1024 at 2^16, walk_min_blocks = 16", &kHeadline16, -1, 16, 256, 0, kWalk2None},
      {"(4, 4) g = 128 at 2^15, walk_min_blocks = 16", &kSmall44, -1, 16, 256, 0, kWalk2None},
      {"(2, 2) g = 64 at 2^13, walk_min_blocks = 16", &kSmall22, -1, 16, 256, 0, kWalk2None},
      {"headline 2^22: the streamed rule's", &kHeadline22, -1, 3072, 256, 0, kWalk2Streamed},
      {"headline 2^20, walk_pair = 0", &kHeadline20, 0, 3072, 256, 0, kWalk2None},
      {"headline 2^22, walk_pair = 0", &kHeadline22, 0, 3072, 256, 0, kWalk2None},
      {"(4, 4) g = 128 at 2^15, walk_pair = 0", &kSmall44, 0, 16, 256, 0, kWalk2None},
      {"headline 2^20, walk_pair = 1: the streamed cut", &kHeadline20, 1, 3072, 256, 0, kWalk2Streamed},
      {"(4, 4) g = 128 at 2^15, walk_pair = 2", &kSmall44, 2, 16, 256, 1, kWalk2Resident},
      {"(4, 4) g = 128 at 2^15, walk_pair = 2 below walk_min_blocks", &kSmall44, 2, 3072, 256, 0, kWalk2None},
      {"headline 2^22, walk_pair = 2", &kHeadline22, 2, 3072, 256, 1, kWalk2Resident},
  };
  int nrules = 0;
  for (const RuleCase& r : rules) {
    WalkPlan P1, P2;
    WalkMatrix M;
    plans_of(*r.l, P1, P2, M);
    WalkKnobs k;
    k.walk_pair = r.walk_pair;
    k.walk_min_blocks = r.walk_min_blocks;
    REQUIRE((int)walk2_wanted_resident(P1, P2, M, k, r.cu) == r.want_resident, "%s: walk2_wanted_resident", r.name);
    REQUIRE((int)walk2_rule(P1, P2, M, k, r.cu) == r.want_rule, "%s: walk2_rule", r.name);
    const Walk2Cut C = walk2_cut_of(walk2_rule(P1, P2, M, k, r.cu), P2, M, k, r.cu);
    REQUIRE(C.taken == (r.want_rule != kWalk2None), "%s: the rule's cut", r.name);
    if (r.want_rule == kWalk2Streamed) REQUIRE(C.G.edge_steps == 0, "%s: the streamed cut has no shortened segments", r.name);
    ++nrules;
  }
  // the streamed rule itself keeps the headline out (tests/walk_geometry_cases.h pins the same)
  {
    WalkPlan P1, P2;
    WalkMatrix M;
    plans_of(kHeadline20, P1, P2, M);
    WalkKnobs k;
    REQUIRE(!walk2_wanted(P1, P2, M, k, 256), "walk2_wanted moved");
    const Walk2Cut C = walk2_cut(P2, M, k, 256);
    REQUIRE(C.G.L == 19 && C.G.nseg == 53 && C.G.ntask == 1008 && C.G.n_walk_wg == 252 && C.ntm == 1, "walk2_cut moved");
    REQUIRE(walk_resident(P2, M), "the headline operator at 2^20 is resident");
  }
  std::printf("resident rule: %d named cases match the table\n", nrules);
  if (g_fail) {
    std::printf("%d failures\n", g_fail);
    return 1;
  }
  std::printf("resident walk2 geometry clean\n");
  return 0;
}
