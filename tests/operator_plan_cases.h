// The plans of csrc/operator_plans.cpp on named inputs: what the walk's shape parser says about a row's column distances, and the
// whole plans -- device format, lattice completion, strip-walk plans, column-blocked mirror, the batched path's row order, tiles and
// operand table -- of named operators.  Included by tests/sanitize_host_index.cpp.
//
// How the expected values were produced: NOT by the functions under test.  The commit before the plans became a unit of their own
// (csrc/engine_plans.hip: walk_shape_reason, build_walk_plan, build_colblock, choose_format, lattice_fill, operator_spmm_order,
// operator_spmm_tiles, all on a qp_operator) was checked out into a scratch directory and built against the same host stand-in of
// the HIP runtime, with the printing code of this harness (`--print-plan-cases`: check_shape_table, plan_record, check_plan_table)
// beside it; the rows below are its output on the inputs below.  Its stand-in device reported the row's CU count (256, 64 or 8) for
// that run; in the harness the rows at 64 and 8 call plan_colblock, the only plan that reads the count, with the number.
// No value depends on a standard-library distribution: the lattices carry constant values, the random columns come from the
// linear congruential generator written out in the harness (lcg_csr).
struct ShapeCase {
  const char* name;
  int n;
  long long d[20];   // the row's column distances, ascending
  // expected
  int code;          // QP_WALK_* (include/qprop.h)
  const char* text;  // the reason, verbatim ("" for an accepted list)
  int nn, K, z0, xl, fd;   // the WalkShape of an accepted list (zeros otherwise)
  long long g, glong, glong1;
  int near[4];
};
static const ShapeCase kShapeCases[] = {
  {"z = 2", 2, {-64,64}, 6, "2 entries per row (the walk takes 3 to 19)", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"z = 20", 20, {-10,-9,-8,-7,-6,-5,-4,-3,-2,-1,1,2,3,4,5,6,7,8,9,10}, 6, "20 entries per row (the walk takes 3 to 19)", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"65 without -65", 5, {-64,-1,0,1,65}, 7, "column distance -64 has no mirror image 64 in the row", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"plain band", 5, {-2,-1,0,1,2}, 8, "no column distance of at least 64 rows: a band of half-width 2 has no strip step", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"near distance 32", 7, {-1024,-32,-1,0,1,32,1024}, 10, "near column distance 32 exceeds the 16-row halo of the walk's window", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"five near", 13, {-64,-5,-4,-3,-2,-1,0,1,2,3,4,5,64}, 11, "5 near column distances per side (the walk takes 1 to 4)", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"far only", 5, {-128,-64,0,64,128}, 9, "no near column distance (the walk's kernels take 1 to 4 within 16 rows)", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"seven far", 17, {-448,-384,-320,-256,-192,-128,-64,-1,0,1,64,128,192,256,320,384,448}, 12, "7 far column distances per side (the walk takes up to 4 multiples of one stride, or up to 2 plus one or two long pairs)", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"two strides", 11, {-1000,-700,-300,-64,-1,0,1,64,300,700,1000}, 13, "far column distance 300 is no multiple of the strip step 64 (two incommensurate strides)", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"multiples 1 3 7 9 of 64", 11, {-576,-448,-192,-64,-1,0,1,64,192,448,576}, 12, "far column distances are multiples of 64 but not the consecutive ones 1 .. K, K <= 4 (largest: 576)", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"65 beside the far reach 64", 7, {-65,-64,-1,0,1,64,65}, 14, "distance 65 is a diagonal neighbour of the far reach 64 (windows on the ring's far steps are not built; the per-block kernel is as fast)", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"three near beside diagonal far neighbours", 13, {-66,-65,-64,-3,-2,-1,0,1,2,3,64,65,66}, 14, "no kernel instance for 3 near distances beside diagonal far neighbours (they come with at most 2 near and one long pair)", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"three near with a long pair", 11, {-5000,-64,-3,-2,-1,0,1,2,3,64,5000}, 14, "no kernel instance for 3 near and 1 far distances with long pairs (they come with at most 2 near, 2 far)", 0,0,0,0,0, 0,0,0, {0,0,0,0}},
  {"(4,4) with diagonal", 17, {-256,-192,-128,-64,-4,-3,-2,-1,0,1,2,3,4,64,128,192,256}, 0, "", 4,4,1,0,0, 64,0,0, {1,2,3,4}},
  {"(4,4)", 16, {-256,-192,-128,-64,-4,-3,-2,-1,1,2,3,4,64,128,192,256}, 0, "", 4,4,0,0,0, 64,0,0, {1,2,3,4}},
  {"(2,2) with diagonal", 9, {-128,-64,-2,-1,0,1,2,64,128}, 0, "", 2,2,1,0,0, 64,0,0, {1,2,0,0}},
  {"(2,2)", 8, {-128,-64,-2,-1,1,2,64,128}, 0, "", 2,2,0,0,0, 64,0,0, {1,2,0,0}},
  {"(1,1) with diagonal", 5, {-64,-1,0,1,64}, 0, "", 1,1,1,0,0, 64,0,0, {1,0,0,0}},
  {"(1,1)", 4, {-64,-1,1,64}, 0, "", 1,1,0,0,0, 64,0,0, {1,0,0,0}},
  {"g = 1000, near 1 and 7", 9, {-2000,-1000,-7,-1,0,1,7,1000,2000}, 0, "", 2,2,1,0,0, 1000,0,0, {1,7,0,0}},
  {"nine-point fd", 9, {-66,-65,-64,-1,0,1,64,65,66}, 0, "", 1,1,1,0,1, 65,0,0, {1,0,0,0}},
  {"fd + long pair", 11, {-4096,-66,-65,-64,-1,0,1,64,65,66,4096}, 0, "", 1,1,1,1,1, 65,4096,0, {1,0,0,0}},
  {"one long pair", 7, {-4096,-64,-1,0,1,64,4096}, 0, "", 1,1,1,1,0, 64,4096,0, {1,0,0,0}},
  {"two long pairs", 9, {-8192,-4096,-64,-1,0,1,64,4096,8192}, 0, "", 1,1,1,2,0, 64,8192,4096, {1,0,0,0}},
};

// One row per named operator (tests/sanitize_host_index.cpp: kPlanInputs gives its generator, requested format and knobs) and CU count.
// s: format, n_lattice_fill, walk reason code | the one-term plan, then the two-term plan: valid nn K z0 S xl glong glong1 fd g R0 R1 W0
//    U0 ustride n_edge near[0..3] | mirror: valid log2w P rpt max_seg ntiles nnz | row order at 64 states: g sw | tiles: valid ntiles
//    nrest g sw T nd K NN
// line_share: cb_line_share, printed %a
// h: 64-bit FNV-1a of the edge lists of the two walk plans | the mirror's segptr, rowoff, cols, map | the row order | tiles, rest, the
//    kernel's operand table (0: no such array)
// text: the walk's reason, verbatim
constexpr int kPlanScalars = 61, kPlanHashes = 10;
struct PlanCase {
  const char* name;
  int cu;
  long long s[kPlanScalars];
  double line_share;
  unsigned long long h[kPlanHashes];
  const char* text;
};
static const PlanCase kPlanCases[] = {
  {"(4,4) lattice g 64, N 4096", 256, {3,0,0,1,4,4,0,1,0,0,0,0,64,4,60,8,3328,512,12,1,2,3,4,1,4,4,0,1,0,0,0,0,64,4,56,12,3328,512,20,1,2,3,4,0,17,0,2,0,0,0,0,0,1,224,512,64,64,80,16,4,4}, 0x0p+0, {0x4fee431bc58e4023ull,0x8ad0e5d1806c5343ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0xd042b0c835aa8bc3ull,0xa056aff156929b83ull,0x186aad300463cf03ull}, ""},
  {"(1,1) lattice g 64, N 5000, open ends", 256, {3,0,0,1,1,1,0,1,0,0,0,0,64,1,77,2,256,256,4,1,0,0,0,1,1,1,0,1,0,0,0,0,64,1,76,3,256,256,6,1,0,0,0,0,17,0,2,0,0,0,0,0,1,288,392,64,64,32,4,1,1}, 0x0p+0, {0xc0da965363f60351ull,0x315b5397cb6ea1dfull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x6ec68600c3b593c3ull,0x37cf37366de97353ull,0x23e41b6e88f4f944ull}, ""},
  {"(2,2) lattice g 100, N 16461", 256, {3,0,0,1,2,2,0,2,0,0,0,0,100,4,254,8,2048,256,12,1,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,1,975,861,100,100,48,8,2,2}, 0x0p+0, {0xe4d5e59c89ca6607ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x056372c8a2df7b62ull,0x30218af585d6af0full,0x8f215a14e007cf97ull}, ""},
  {"nine-point lattice g 64, N 16461", 256, {3,0,10,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, "near column distance 63 exceeds the 16-row halo of the walk's window"},
  {"nine-point lattice g 65, N 16461", 256, {3,0,0,1,1,1,0,2,0,0,0,1,65,2,256,4,1024,256,6,1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x09f335a53cf1fe6eull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"near distance 32, N 4096, packed", 256, {3,0,10,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,1024,256,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x259769b984ba7183ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, "near column distance 32 exceeds the 16-row halo of the walk's window"},
  {"band of five, N 4096, packed", 256, {3,0,8,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, "no column distance of at least 64 rows: a band of half-width 5 has no strip step"},
  {"(4,4) lattice g 1024, N 2^15", 256, {3,0,0,1,4,4,0,16,0,0,0,0,1024,64,448,128,49408,512,192,1,2,3,4,1,4,4,0,16,0,0,0,0,1024,64,384,192,49408,512,320,1,2,3,4,0,17,0,2,0,0,0,1024,64,1,1536,8192,1024,128,80,16,4,4}, 0x0p+0, {0xf396be4a7b04a8c3ull,0x2d3a5ecf4a499803ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0xfb408ebf35cf8583ull,0x5736d3af40271783ull,0x267d899d1a430983ull,0x42442b8de832835full}, ""},
  {"chain of blocks g 64, N 2048", 256, {3,0,0,1,1,1,0,1,0,0,0,0,64,1,31,2,256,256,3,1,0,0,0,1,1,1,0,1,0,0,0,0,64,1,30,3,256,256,5,1,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x8447c58c6fc21c9dull,0x61fd082c5a0b5dc1ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"64 x 64 periodic grid", 256, {3,0,0,1,1,1,0,1,0,0,0,0,64,1,63,2,256,256,3,1,0,0,0,1,1,1,0,1,0,0,0,0,64,1,62,3,256,256,5,1,0,0,0,0,17,0,2,0,0,0,0,0,1,224,512,64,64,32,4,1,1}, 0x0p+0, {0x839d46973679aebdull,0x40ab6a587eac3401ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0xd042b0c835aa8bc3ull,0xa056aff156929b83ull,0x23e41b6e88f4f944ull}, ""},
  {"256 x 16 periodic grid", 256, {3,0,0,1,1,1,0,4,0,0,0,0,256,4,60,8,1024,256,12,1,0,0,0,1,1,1,0,4,0,0,0,0,256,4,56,12,1024,256,20,1,0,0,0,0,17,0,2,0,0,0,0,0,1,128,2048,256,128,32,4,1,1}, 0x0p+0, {0x4fee431bc58e4023ull,0x8ad0e5d1806c5343ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x16a51d43703a9883ull,0xfbad9a09e0f98183ull,0xb630ad8907eaddb5ull}, ""},
  {"256 x 16 periodic grid, strips of 8", 256, {3,0,0,1,1,1,0,4,0,0,0,0,256,4,60,8,1024,256,12,1,0,0,0,1,1,1,0,4,0,0,0,0,256,4,56,12,1024,256,20,1,0,0,0,0,17,0,2,0,0,0,256,8,1,128,2048,256,8,32,4,1,1}, 0x0p+0, {0x4fee431bc58e4023ull,0x8ad0e5d1806c5343ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x19a356368b2a9783ull,0xea551e9f2d57bf83ull,0xfbad9a09e0f98183ull,0xb630ad8907eaddb5ull}, ""},
  {"open 96 x 64 grid", 256, {3,126,0,1,1,1,1,2,0,0,0,0,96,2,94,4,512,256,6,1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,1,336,768,96,96,32,5,1,1}, 0x0p+0, {0x3aaed7945213f612ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x191a30dcea9d3663ull,0x1aa563552397b303ull,0xa1c71282fb6b16fcull}, ""},
  {"open 96 x 64 grid, default knobs", 256, {1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"12-spin chain", 256, {2,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"12-spin chain, packed", 256, {3,0,5,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, "the longest run of row blocks whose rows all carry one list of column distances is 0 blocks (of 64): not a lattice"},
  {"ragged 4096 x 4096", 256, {2,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"random columns N 4096, mirror forced", 256, {2,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,6,64,2,35,32,32737,0,0,0,0,0,0,0,0,0,0,0}, 0x1.b94ee11a846c1p-1, {0x0000000000000000ull,0x0000000000000000ull,0xaba753150d9c4536ull,0xdb033064ec1ea86full,0xf4b7662741881654ull,0x47cd5f93e56f9258ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"random columns N 4096, mirror forced", 64, {2,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,6,64,2,35,32,32737,0,0,0,0,0,0,0,0,0,0,0}, 0x1.b94ee11a846c1p-1, {0x0000000000000000ull,0x0000000000000000ull,0xaba753150d9c4536ull,0xdb033064ec1ea86full,0xf4b7662741881654ull,0x47cd5f93e56f9258ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"random columns N 4096, mirror forced", 8, {2,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,6,64,2,35,32,32737,0,0,0,0,0,0,0,0,0,0,0}, 0x1.b94ee11a846c1p-1, {0x0000000000000000ull,0x0000000000000000ull,0xaba753150d9c4536ull,0xdb033064ec1ea86full,0xf4b7662741881654ull,0x47cd5f93e56f9258ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"random columns N 4096, mirror forced, CSR", 256, {1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,6,64,2,35,32,32737,0,0,0,0,0,0,0,0,0,0,0}, 0x1.b94ee11a846c1p-1, {0x0000000000000000ull,0x0000000000000000ull,0xaba753150d9c4536ull,0xdb033064ec1ea86full,0xf4b7662741881654ull,0xb52756c0fb145b26ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"random columns N 4096, mirror forced, CSR", 64, {1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,6,64,2,35,32,32737,0,0,0,0,0,0,0,0,0,0,0}, 0x1.b94ee11a846c1p-1, {0x0000000000000000ull,0x0000000000000000ull,0xaba753150d9c4536ull,0xdb033064ec1ea86full,0xf4b7662741881654ull,0xb52756c0fb145b26ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"random columns N 4096, mirror forced, CSR", 8, {1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,6,64,2,35,32,32737,0,0,0,0,0,0,0,0,0,0,0}, 0x1.b94ee11a846c1p-1, {0x0000000000000000ull,0x0000000000000000ull,0xaba753150d9c4536ull,0xdb033064ec1ea86full,0xf4b7662741881654ull,0xb52756c0fb145b26ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"random columns N 2^18, mirror forced", 256, {2,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,12,64,2,15,2048,524287,0,0,0,0,0,0,0,0,0,0,0}, 0x1.ff57p-1, {0x0000000000000000ull,0x0000000000000000ull,0x936d2f8fc60d08afull,0xbfba4187eca1b6c6ull,0x0a63f672c105abd7ull,0x10b6a2ae6282244dull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"random columns N 2^18, mirror forced", 64, {2,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,12,64,2,15,2048,524287,0,0,0,0,0,0,0,0,0,0,0}, 0x1.ff57p-1, {0x0000000000000000ull,0x0000000000000000ull,0x936d2f8fc60d08afull,0xbfba4187eca1b6c6ull,0x0a63f672c105abd7ull,0x10b6a2ae6282244dull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"random columns N 2^18, mirror forced", 8, {2,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x1.ff57p-1, {0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"long pair 16384, N 2^16: walkable decides", 256, {3,0,0,1,1,1,0,1,1,16384,0,0,64,256,768,512,65792,256,768,1,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x159956ee5456f883ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
  {"long pair 16384, N 2^16: walk off", 256, {2,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,17,0,2,0,0,0,0,0,0,0,0,0,0,0,0,0,0}, 0x0p+0, {0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull,0x0000000000000000ull}, ""},
};
