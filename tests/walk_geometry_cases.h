// Launch geometry of the strip walks (csrc/walk_geometry.cpp) on named inputs: what walk_cut / walk2_cut / walk2_wanted must return.
// Included by tests/sanitize_host_index.cpp.
//
// How the expected values were produced: NOT by the functions under test.  The launcher bodies of the commit before the cut
// moved into walk_geometry.cpp (kernels_walk.hip: launch_hrb_walk_cheby from `nW` to `G.ntask`; kernels_walk2.hip:
// launch_hrb_walk2_cheby from the shape check to `ntm`; engine_cheby.hip: walk2_wanted) were copied verbatim into a scratch program
// with device_cu_count() replaced by the row's CU count, run on the inputs below, and its output pasted here.  The same program
// tried 1.5 million tiny plans: the `while` loop "for tiny operators" was entered for none of them (nseg L >= J + edge_segs
// edge_steps holds by the ceiling that defines nseg), so the tiny-operator row covers the regime it was written for -- L clamped to
// edge_steps + 1, edge_segs clipped to nseg -- and the loop stays in the code as it was.
// Figures the sources document, for orientation: inside the Infinity Cache the walk is cut into at most 768 wavefronts (1024 for
// the real copy); the headline lattice beyond it has 192 edge blocks = 24 workgroups of eight, which leaves 8 x (256 - 24) = 1856;
// its two-term chunks form z on W = 56 rows, S2 = 19 chunks per 1024-row strip step.
struct CutCase {
  const char* name;
  int two;   // 0: one-term walk (walk_cut), 1: two-term walk (walk2_cut, walk2_wanted; the one-term plan is the region grown by K S blocks at either end)
  struct { int nn, K, z0, S, xl, fd; long long g; int near[4]; long long R0, R1, W0, n_edge; } p;
  struct { long long nblocks, nrows, ncols; int real; } m;
  struct { int walk_waves, walk_nt, walk_dbg, walk_min_blocks; } k;
  int cu, reserve_cu, row_set, no_edges;
  // expected
  int taken, ws, ntm;
  unsigned grid;
  struct { int L, nseg, n_walk_wg, ntask, edge_segs, edge_steps, edge_last; long long xlast; int n_edge_wg; } g1;
  struct { int L, nseg, ntask, n_walk_wg, S2, W; long long xlast, vend; } g2;
  int wanted;   // walk2_wanted with walk_pair = -1
};
static const CutCase kCutCases[] = {
  {"headline 2^20 complex: resident, 768 wavefronts", 0, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,16320,128,192}, {16384,1048576,1048576,0}, {0,-1,0,3072}, 256,0,0,0,
   1, 4, 0, 232, {22,46,184,736,0,0,0,1048575,48}, {}, 0},
  {"headline 2^20 real copy: resident, 1024 wavefronts", 0, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,16320,128,192}, {16384,1048576,1048576,1}, {0,-1,0,3072}, 256,0,0,0,
   1, 4, 0, 304, {16,64,256,1024,0,0,0,1048575,48}, {}, 0},
  {"headline 2^22: beyond the cache, edges beside, 8 x (256 - 24) = 1856", 0, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,65472,128,192}, {65536,4194304,4194304,0}, {0,-1,0,3072}, 256,0,0,0,
   1, 8, 1, 252, {36,114,228,1824,0,0,0,4194303,24}, {}, 0},
  {"g = 2048 at 2^22: beyond the cache, edges inside the walk, 2048", 0, {4,4,0,32,0,0,2048, {1,2,3,4}, 128,65408,256,384}, {65536,4194304,4194304,0}, {0,-1,0,3072}, 256,0,0,0,
   1, 8, 1, 256, {33,64,256,2048,12,4,0,4194303,0}, {}, 0},
  {"row set of a split term at 2^21 local rows, reserve_cu = 8", 0, {4,4,0,16,0,0,1024, {1,2,3,4}, 0,32768,145,290}, {32768,2097152,2105344,0}, {0,-1,0,3072}, 256,8,1,0,
   1, 8, 1, 241, {20,102,204,1632,0,0,0,2105343,37}, {}, 0},
  {"g = 1000 (no multiple of 64), diagonal, two near, two far", 0, {2,2,1,16,0,0,1000, {1,2,0,0}, 32,7780,64,97}, {7813,500000,500000,0}, {0,-1,0,3072}, 256,0,0,0,
   1, 4, 0, 205, {11,45,180,720,0,0,0,499999,25}, {}, 0},
  {"headline 2^22, walk_waves = 2048", 0, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,65472,128,192}, {65536,4194304,4194304,0}, {2048,-1,0,3072}, 256,0,0,0,
   1, 8, 1, 252, {33,126,252,2016,12,4,0,4194303,0}, {}, 0},
  {"headline 2^20, walk_waves = 64, walk_nt = 1", 0, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,16320,128,192}, {16384,1048576,1048576,0}, {64,1,0,3072}, 256,0,0,0,
   1, 4, 1, 64, {253,4,16,64,0,0,0,1048575,48}, {}, 0},
  {"headline 2^20, walk_dbg = 5: edges inside, after the walk", 0, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,16320,128,192}, {16384,1048576,1048576,0}, {0,-1,5,3072}, 256,0,0,0,
   1, 4, 0, 188, {23,47,188,752,12,4,1,1048575,0}, {}, 0},
  {"headline 2^22 on 64 compute units", 0, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,65472,128,192}, {65536,4194304,4194304,0}, {0,-1,0,3072}, 64,0,0,0,
   1, 8, 1, 64, {130,32,64,512,12,4,0,4194303,0}, {}, 0},
  {"headline 2^17: fewer walkable blocks than walk_min_blocks, not taken", 0, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,1984,128,192}, {2048,131072,131072,0}, {0,-1,0,3072}, 256,0,0,0,
   0, 0, 0, 0, {0,0,0,0,0,0,0,0,0}, {}, 0},
  {"long pair and diagonal far neighbours at 2^21 (footprint counts 3 far slots + the long one)", 0, {2,1,1,4,1,1,256, {1,2,0,0}, 1024,31744,2048,3072}, {32768,2097152,2097152,0}, {0,-1,0,3072}, 256,0,0,0,
   1, 8, 1, 250, {19,499,250,2000,499,4,0,2097151,0}, {}, 0},
  {"tiny operator (8 walkable blocks): L clamped to edge_steps + 1, edge_segs clipped to nseg", 0, {1,1,1,1,0,0,64, {1,0,0,0}, 0,9,1,30}, {38,2432,2432,0}, {256,-1,4,8}, 256,0,0,0,
   1, 4, 0, 7, {5,26,7,28,26,4,0,2431,0}, {}, 0},
  {"developer knob walk_dbg = 2: edge blocks skipped", 0, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,16320,128,192}, {16384,1048576,1048576,0}, {0,-1,2,3072}, 256,0,0,1,
   1, 4, 0, 184, {22,46,184,736,0,0,0,1048575,0}, {}, 0},
  {"two-term (4, 4) headline 2^22: W = 56, S2 = 19", 1, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,65408,192,320}, {65536,4194304,4194304,0}, {0,-1,0,3072}, 256,0,0,0,
   1, 0, 0, 252, {}, {77,53,1008,252,19,56,4194303,4190208}, 1},
  {"two-term (4, 4) headline 2^21: values within 300e6 bytes", 1, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,32640,192,320}, {32768,2097152,2097152,0}, {0,-1,0,3072}, 256,0,0,0,
   1, 0, 1, 247, {}, {39,52,988,247,19,56,2097151,2093056}, 1},
  {"two-term (1, 1) with a diagonal, g = 4096, real copy", 1, {1,1,1,64,0,0,4096, {1,0,0,0}, 64,65408,192,192}, {65536,4194304,4194304,1}, {0,-1,0,3072}, 256,0,0,0,
   1, 0, 1, 252, {}, {68,15,1008,252,67,62,4194303,4190208}, 1},
  {"two-term (2, 3), d_max = 16, g = 512 at 2^23", 1, {2,3,0,8,0,0,512, {1,16,0,0}, 24,131024,72,120}, {131072,8388608,8388608,0}, {0,-1,0,3072}, 256,0,0,0,
   1, 0, 0, 256, {}, {256,64,1024,256,16,32,8388607,8387072}, 1},
  {"two-term (4, 4) headline 2^22, walk_waves = 1856, walk_nt = 0", 1, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,65408,192,320}, {65536,4194304,4194304,0}, {1856,0,0,3072}, 256,0,0,0,
   1, 0, 0, 452, {}, {43,95,1808,452,19,56,4194303,4190208}, 1},
  {"two-term (4, 4) headline 2^20: resident, not wanted", 1, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,16256,192,320}, {16384,1048576,1048576,0}, {0,-1,0,3072}, 256,0,0,0,
   1, 0, 1, 252, {}, {19,53,1008,252,19,56,1048575,1044480}, 0},
  {"two-term (4, 4) at 20000 blocks: beyond the cache, 23 steps per wavefront, not wanted", 1, {4,4,0,16,0,0,1024, {1,2,3,4}, 64,19872,192,320}, {20000,1280000,1280000,0}, {0,-1,0,3072}, 256,0,0,0,
   1, 0, 1, 247, {}, {24,52,988,247,19,56,1279999,1275904}, 0},
};
