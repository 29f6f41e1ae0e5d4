// AddressSanitizer / UBSan harness for the library's HOST INDEX WORK: everything qp_operator_create does on the
// host before a kernel ever runs -- union pattern, Hermitian check, format choice, lattice completion, strip-walk plan, column
// encodings (int32 / int16 / stencil / block map), Hermitian packing with transposed positions, column-blocked mirror, value
// dictionary -- and the decoders of qp_operator_get_csr, compiled from the library's own sources (csrc/engine_core.hip,
// csrc/engine_operator.hip, csrc/engine_plans.hip here; csrc/operator_layout.cpp, csrc/operator_plans.cpp, csrc/walk_geometry.cpp and
// csrc/host_numerics.cpp beside it as ordinary C++) with g++ against tests/hip_host_shim (device memory = heap memory, so the
// sanitizer checks every copy into a "device" array against its allocation) and driven by a fuzz over the shapes that have bitten:
// tall (5681 x 358: the round-4 GPU memory fault), wide, 1 row, fewer than 64 rows, empty rows, lattices, grids, spin chains.
// Checked per case: the get_csr round trip reproduces the input exactly; EVERY stored slot of every row block -- real entries,
// pads, the lanes beyond the last row -- decodes to a column inside the matrix; every pad carries the value zero in every term;
// every transposed position of a Hermitian-packed operator is -1 (pad) or inside the value array.
// For every operator with a strip-walk plan, the CUT of its launches (csrc/walk_geometry.cpp, the pure-host unit the launchers call) is
// swept over chip sizes and knobs and checked against the kernels' own segment formulas: every strip step belongs to exactly one
// segment, every edge block is reached, the launch fits the chip; and a table of named inputs (tests/walk_geometry_cases.h) pins
// the numbers.
// The plans themselves (csrc/operator_plans.cpp, the pure-host unit engine_plans.hip uploads from): the batched path's row order, tiles
// and LDS operand table are checked BY CONSTRUCTION over every knob value (permutation, partition, every operand slot names the
// entry's column); every verdict of the walk's shape parser and the whole plans of named operators are pinned by
// tests/operator_plan_cases.h (`--print-plan-cases` prints that table's rows from the tree it is built against).
// Built and run by tests/test_cabi_host.py::test_host_index_work_under_sanitizers (CPU only).
// `--digest`: per case one line with the format, the scalar fields of the layout structs and a 64-bit FNV-1a hash over the
// declared extent of every "device" array the operator owns -- two builds of the library lay operators out bit-identically iff
// their outputs agree; the lazily built plans of the batched path (row order at 8 and 64 states, tiles, operand table) included.  For this mode build WITHOUT the sanitizers and with -DQP_SHIM_ZERO_ALLOC (bytes the build never writes
// then compare equal).  The values depend on the standard library's distributions: compare, do not store.
// `--large`: the THREADED host build -- a fixed list of operators of 2^16 .. 2^18 rows that crosses every serial threshold of
// parallel_rows, with the digests, the call sites that really started threads, the error paths at size and the throwing-worker
// checks (tests/test_cabi_host.py::test_threaded_host_build: equal digests at every thread count, ThreadSanitizer, ASan/UBSan).
#include <atomic>
#include <cstdio>
#include <mutex>
#include <new>
#include <random>
#include <set>
#include <thread>

#include "../quantumpropagators.jl_amd/csrc/engine_core.hip"
#include "../quantumpropagators.jl_amd/csrc/engine_operator.hip"
#include "../quantumpropagators.jl_amd/csrc/engine_plans.hip"
#include "walk_geometry_cases.h"
#include "operator_plan_cases.h"

// ---- the call sites of parallel_rows that started at least two threads (csrc/operator_layout.h, QP_PARALLEL_ROWS_TRACE) -----
namespace {
std::mutex g_sites_lock;
std::set<std::pair<std::string, int>> g_sites;
}  // namespace
void qp_parallel_rows_threaded(const char* file, int line, size_t) {
  const char* base = std::strrchr(file, '/');
  std::lock_guard<std::mutex> hold(g_sites_lock);
  g_sites.insert({base ? base + 1 : file, line});
}

// ---- out of memory on a worker thread, on demand (uninstrumented builds: the sanitizers bring an operator new of their own) ----
#if !defined(__SANITIZE_ADDRESS__) && !defined(__SANITIZE_THREAD__)
#define QP_HARNESS_OWN_NEW 1
namespace {
std::atomic<int> g_new_failures{0};   // so many allocations made off the main thread fail
std::thread::id g_main_thread = std::this_thread::get_id();
}  // namespace
void* operator new(size_t n) {
  if (g_new_failures.load(std::memory_order_relaxed) > 0 && std::this_thread::get_id() != g_main_thread && g_new_failures.fetch_sub(1) > 0)
    throw std::bad_alloc();
  if (void* p = std::malloc(n ? n : 1)) return p;
  throw std::bad_alloc();
}
void operator delete(void* p) noexcept { std::free(p); }
void operator delete(void* p, size_t) noexcept { std::free(p); }
#endif

// ---- host stand-ins of the few launches the creation path makes (values only; no kernel runs in this build) ---------------
namespace qp {
static inline void cfma_h(double2& s, double2 a, double2 b) {
  s.x = std::fma(a.x, b.x, s.x);
  s.x = std::fma(-a.y, b.y, s.x);
  s.y = std::fma(a.x, b.y, s.y);
  s.y = std::fma(a.y, b.x, s.y);
}
int launch_combine_planes(hipStream_t, double2* vals, const double2* const* planes, const double2* coefs, int nplanes, int64_t n,
                          double* vals_r, Stats*) {
  for (int64_t p = 0; p < n; ++p) {
    double2 acc{0.0, 0.0};
    for (int l = 0; l < nplanes; ++l) cfma_h(acc, coefs[l], planes[l][p]);
    vals[p] = acc;
    if (vals_r) vals_r[p] = acc.x;
  }
  return QP_OK;
}
int launch_sparse_planes_update(hipStream_t, double2* vals, const double2* base, const int32_t* support, int64_t n_support,
                                const double2* support_vals, int nplanes, const double2* coefs, double* vals_r, Stats*) {
  for (int64_t i = 0; i < n_support; ++i) {
    double2 acc = base[support[i]];
    for (int l = 0; l < nplanes; ++l) cfma_h(acc, coefs[l], support_vals[(size_t)l * n_support + i]);
    vals[support[i]] = acc;
    if (vals_r) vals_r[support[i]] = acc.x;
  }
  return QP_OK;
}
int launch_real_part(hipStream_t, double* out, const double2* v, int64_t n, Stats*) {
  for (int64_t i = 0; i < n; ++i) out[i] = v[i].x;
  return QP_OK;
}
int launch_colblock_gather(hipStream_t, const ColBlockPlan& P, const double2* src, Stats*) {
  for (int64_t p = 0; p < P.nnz; ++p) {
    const int64_t m = P.map[p];
    const double2 v = m >= 0 ? src[m] : make_double2(src[-m - 1].x, -src[-m - 1].y);
    P.vals[p] = v;
    if (P.use_real && P.vals_r) P.vals_r[p] = v.x;
  }
  return QP_OK;
}
int launch_gather_csr_vals(hipStream_t, double2* out, const double2* vals, const int64_t* map, int64_t nnz, Stats*) {
  for (int64_t p = 0; p < nnz; ++p) out[p] = map[p] >= 0 ? vals[map[p]] : make_double2(vals[-map[p] - 1].x, -vals[-map[p] - 1].y);
  return QP_OK;
}
// (never reached by operator creation / get_csr; the linker wants them)
int launch_fill(hipStream_t, double2*, double2, int64_t, Stats*) { std::abort(); }
int launch_scal(hipStream_t, double2*, double2, int64_t, Stats*) { std::abort(); }
int launch_axpy(hipStream_t, double2, const double2*, double2*, int64_t, Stats*) { std::abort(); }
int launch_dot_partials(hipStream_t, const double2*, const double2*, double2*, int64_t, Stats*) { std::abort(); }
int launch_spmv_plain(hipStream_t, const DevMatrix&, const double2*, const PlainEpi&, Stats*) { std::abort(); }
}  // namespace qp

namespace {

struct Csr {
  int64_t nrows = 0, ncols = 0;
  std::vector<int64_t> rp;
  std::vector<int32_t> col;      // (int64 copies are made for qp_matrix_create, whose index arrays are the reference's Int64)
  std::vector<qp_c128> val;
};

#define REQUIRE(cond, ...)                                   \
  do {                                                       \
    if (!(cond)) {                                           \
      std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                     \
      std::fprintf(stderr, "\n");                            \
      std::exit(1);                                          \
    }                                                        \
  } while (0)

// the kernels' column decoder (csrc/kernel_common.h: ld_cols) restated on the host bytes: column of slot k, lane l of block b
int64_t decode_any(const char* bytes, int64_t meta, int64_t k, int l, int64_t rowc) {
  const char* p = bytes + (meta >> 2);
  const int mode = (int)(meta & 3);
  const int64_t q = k >> 2;
  const int j = (int)(k & 3);
  if (mode == 2) {
    int32_t d[4];
    std::memcpy(d, p + q * 16, 16);
    return rowc + d[j];
  }
  if (mode == 3) {
    const char* pq = p + (size_t)q * (16 + 4 * 64);
    int32_t cb[4];
    std::memcpy(cb, pq, 16);
    uint32_t lb;
    std::memcpy(&lb, pq + 16 + 4 * l, 4);
    return ((int64_t)cb[j] << 6) | ((lb >> (8 * j)) & 63u);
  }
  if (mode == 1) {
    int16_t d[4];
    std::memcpy(d, p + ((size_t)q * 64 + l) * 8, 8);
    return rowc + d[j];
  }
  int32_t c[4];
  std::memcpy(c, p + ((size_t)q * 64 + l) * 16, 16);
  return c[j];
}

int64_t n_cases = 0, n_walked = 0, n_hrb = 0, n_coded = 0, n_cb = 0, n_dense = 0;
bool g_digest = false;

// --digest: see the head of this file
void print_digest(qp_operator* op, const char* what) {
  uint64_t h = 1469598103934665603ull;
  auto bytes = [&](const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
  };
  std::string scalars;
  auto num = [&](long long v) { scalars += " " + std::to_string(v); };
  const DevMatrix& A = op->A;
  const size_t nb = (size_t)A.nblocks;
  for (long long v : {(long long)A.nrows, (long long)A.ncols, (long long)A.nnz, (long long)A.stored, (long long)A.nblocks, (long long)A.colbytes,
                      (long long)A.lanes_per_row, (long long)A.lcolbytes, (long long)A.lstored, (long long)op->planes.size(), (long long)op->sparse_from,
                      (long long)op->n_support, (long long)op->planes_real, (long long)op->n_lattice_fill, (long long)op->cv_reason})
    num(v);
  if (qp::csr_layout(A.format)) {
    bytes(A.rowptr, ((size_t)A.nrows + 1) * 8);
    bytes(A.cols, (size_t)A.nnz * 4);
  } else {
    bytes(A.bptr, (nb + 1) * 8);
    bytes(A.cmeta, nb * 8);
    bytes(A.cols, (size_t)A.colbytes);
  }
  if (A.format == QP_FMT_HRB) {
    bytes(A.lptr, (nb + 1) * 8);
    bytes(A.lcmeta, nb * 8);
    bytes(A.lcols, (size_t)A.lcolbytes);
    bytes(A.lpos, (size_t)A.lstored * 4);
  }
  for (const double2* p : op->planes) bytes(p, (size_t)A.stored * 16);
  if (op->sparse_from >= 0) {
    bytes(op->support, (size_t)op->n_support * 4);
    bytes(op->support_vals, (size_t)(op->nops - op->sparse_from) * (size_t)op->n_support * 16);
  }
  for (const qp::WalkPlan* P : {&op->walk, &op->walk2}) {
    for (long long v : {(long long)P->valid, (long long)P->nn, (long long)P->K, (long long)P->z0, (long long)P->S, (long long)P->xl, (long long)P->glong,
                        (long long)P->glong1, (long long)P->fd, (long long)P->g, (long long)P->R0, (long long)P->R1, (long long)P->W0, (long long)P->U0,
                        (long long)P->ustride, (long long)P->n_edge})
      num(v);
    for (int v : P->near) num(v);
    if (P->valid) bytes(P->edge_map, (size_t)P->n_edge * 4);
  }
  const qp::ColBlockPlan& B = op->cb;
  for (long long v : {(long long)B.valid, (long long)B.log2w, (long long)B.P, (long long)B.rpt, (long long)B.max_seg, (long long)B.ntiles, (long long)B.nnz, (long long)B.use_real}) num(v);
  if (B.valid) {
    bytes(B.segptr, (size_t)(B.ntiles * B.P + 1) * 4);
    bytes(B.rowoff, (size_t)(B.ntiles * B.P) * (size_t)(64 * B.rpt + 1) * 2);
    bytes(B.cols, (size_t)B.nnz * 4);
    bytes(B.map, (size_t)B.nnz * 8);
    bytes(B.vals, (size_t)B.nnz * 16);
  }
  const qp::CodedVals& C = op->cv;
  for (long long v : {(long long)C.valid, (long long)C.ntab, (long long)C.ntables, (long long)C.use_real}) num(v);
  if (C.valid) {
    bytes(C.codes, (size_t)A.stored);
    bytes(C.tptr, nb * 8);
    for (const double2* p : op->cv_tplanes) bytes(p, (size_t)C.ntab * 16);
  }
  if (A.format != QP_FMT_MATFREE) {   // the batched path's plans, built at the first batched step
    for (int batch : {8, 64}) {
      const int32_t* order = nullptr;
      if (operator_spmm_order(op, batch, &order) != QP_OK) std::abort();
      for (long long v : {(long long)(order != nullptr), (long long)op->m_order_g, (long long)op->m_order_sw}) num(v);
      if (order) bytes(order, (size_t)A.nrows * 4);
    }
    const qp::SpmmTiles* T = nullptr;
    if (operator_spmm_tiles(op, &T) != QP_OK) std::abort();
    const qp::SpmmTiles& M = op->m_tiles;
    for (long long v : {(long long)M.valid, (long long)M.ntiles, (long long)M.nrest, (long long)M.g, (long long)M.sw, (long long)M.T, (long long)M.shape.nd,
                        (long long)M.shape.K, (long long)M.shape.NN})
      num(v);
    bytes(M.shape.dfar, sizeof M.shape.dfar);
    bytes(M.shape.dnear, sizeof M.shape.dnear);
    if (T) {
      bytes(T->tiles, (size_t)T->ntiles * 4);
      bytes(T->rest, (size_t)T->nrest * 4);
      bytes(T->tab, (size_t)qp::kSpmmTileTab * 4);
    }
  }
  std::printf("digest %s | format %d |%s | %016llx\n", what, A.format, scalars.c_str(), (unsigned long long)h);
}

int64_t n_walk2 = 0, n_cuts = 0;

// ---- the cut of the one-term walk against the kernel's segment formulas -------------------------------------------------
// (csrc/kernels_walk_impl.h, hrb_walk_kernel: wrows, Jc, j0, j1 as the kernel computes them from P and G for wavefront (seg, col);
// a wavefront walks steps [j0, j1) iff seg < G.nseg and j0 < j1; edge blocks: workgroups of their own, one block per wavefront,
// when G.n_edge_wg > 0, else `for (idx = task; idx < P.n_edge; idx += G.ntask)` on every wavefront with task < P.n_edge)
void check_walk_cut(const qp::WalkPlan& P, const qp::WalkMatrix& M, const qp::WalkKnobs& k, int cu, int reserve, bool row_set, const char* what) {
  const qp::WalkCut C = qp::walk_cut(P, M, k, cu, reserve, row_set, false);
  if (!C.taken) {
    REQUIRE(P.R1 - P.W0 < k.walk_min_blocks || P.R1 - P.W0 < P.S, "%s: a plan of %lld walkable blocks was not taken", what, (long long)(P.R1 - P.W0));
    return;
  }
  ++n_cuts;
  const qp::WalkGeom& G = C.G;
#define CUT_REQUIRE(cond) REQUIRE(cond, "%s: walk_cut(cu %d, reserve %d, row set %d, walk_waves %d, walk_dbg %d): " #cond " [L %d nseg %d ntask %d n_walk_wg %d edge_segs %d edge_steps %d n_edge_wg %d ws %d]", \
                                  what, cu, reserve, (int)row_set, k.walk_waves, k.walk_dbg, G.L, G.nseg, G.ntask, G.n_walk_wg, G.edge_segs, G.edge_steps, G.n_edge_wg, C.ws)
  CUT_REQUIRE(C.ws == 4 || C.ws == 8);
  CUT_REQUIRE(G.ntask == G.n_walk_wg * C.ws && (int64_t)G.ntask >= (int64_t)G.nseg * P.S);
  CUT_REQUIRE(C.grid == (unsigned)(G.n_edge_wg + G.n_walk_wg));
  CUT_REQUIRE(G.L > G.edge_steps);
  CUT_REQUIRE(G.edge_segs <= G.nseg);
  CUT_REQUIRE(G.xlast == M.ncols - 1);
  const int64_t g = P.g;
  const int64_t wrows = (P.R1 - P.W0) * (int64_t)kRB;
  for (int col = 0; col < P.S; ++col) {
    const int Jc = (int64_t)col * kRB < wrows ? (int)((wrows - (int64_t)col * kRB + g - 1) / g) : 0;
    int next = 0;   // first step of the column no segment has taken yet
    for (int seg = 0; seg < G.nseg; ++seg) {
      const int j0 = seg * G.L - std::min(seg, G.edge_segs) * G.edge_steps;
      const int j1 = std::min((seg + 1) * G.L - std::min(seg + 1, G.edge_segs) * G.edge_steps, Jc);
      if (j0 < j1) {
        CUT_REQUIRE(j0 == next);
        next = j1;
      }
    }
    CUT_REQUIRE(next == Jc);
  }
  if (G.n_edge_wg > 0) {
    CUT_REQUIRE((int64_t)G.n_edge_wg * C.ws >= P.n_edge);
    CUT_REQUIRE((int64_t)G.n_edge_wg + G.n_walk_wg <= (int64_t)std::max(cu - reserve, 8) * (8 / C.ws));
  } else {
    std::vector<char> reached((size_t)P.n_edge, 0);
    for (int64_t task = 0; task < G.ntask && task < P.n_edge; ++task)
      for (int64_t idx = task; idx < P.n_edge; idx += G.ntask) reached[(size_t)idx] = 1;
    for (int64_t i = 0; i < P.n_edge; ++i) CUT_REQUIRE(reached[(size_t)i]);
  }
#undef CUT_REQUIRE
}

// ---- the cut of the two-term walk (csrc/kernels_walk2_impl.h, hrb_walk2_kernel: zb, ze, Jz, j0 = seg L, j1 = min(j0 + L, Jz) for seg < G.nseg) -----
void check_walk2_cut(const qp::WalkPlan& P2, const qp::WalkMatrix& M, const qp::WalkKnobs& k, int cu, const char* what) {
  const qp::Walk2Cut C = qp::walk2_cut(P2, M, k, cu);
  const qp::Walk2Geom& G = C.G;
#define CUT_REQUIRE(cond) REQUIRE(cond, "%s: walk2_cut(cu %d, walk_waves %d): " #cond " [W %d S2 %d L %d nseg %d ntask %d n_walk_wg %d]", what, cu, k.walk_waves, G.W, G.S2, G.L, G.nseg, G.ntask, G.n_walk_wg)
  CUT_REQUIRE(C.taken);
  ++n_cuts;
  CUT_REQUIRE(G.W >= 16 && G.W == kRB - 2 * P2.near[P2.nn - 1]);
  CUT_REQUIRE((int64_t)G.S2 * G.W >= P2.g);
  const int64_t zb = P2.W0 * (int64_t)kRB, ze = P2.R1 * (int64_t)kRB;
  const int Jz = (int)((ze - zb + P2.g - 1) / P2.g);
  CUT_REQUIRE(C.Jz == Jz);
  int next = 0;
  for (int seg = 0; seg < G.nseg; ++seg) {
    const int j0 = seg * G.L, j1 = std::min(j0 + G.L, Jz);
    CUT_REQUIRE(j0 == next && j0 < j1);
    next = j1;
  }
  CUT_REQUIRE(next == Jz);
  CUT_REQUIRE(G.ntask == 4 * G.n_walk_wg && (int64_t)G.ntask >= (int64_t)G.nseg * G.S2);
  CUT_REQUIRE(G.vend == (P2.R1 + (int64_t)P2.K * P2.S) * 64);
  CUT_REQUIRE(G.xlast == M.ncols - 1);
#undef CUT_REQUIRE
}

// every chip size and knob setting the launchers can meet, for one operator's plans (walk_min_blocks lowered: small plans are taken)
void check_walk_geometry(const qp_operator* op, const char* what) {
  const qp::WalkMatrix M = qp::walk_matrix(op->A);
  for (int cu : {8, 64, 256})
    for (int waves : {0, 64, 1856, 2048}) {
      qp::WalkKnobs k;
      k.walk_waves = waves;
      k.walk_min_blocks = 1;
      for (int dbg : {0, 1, 4})
        for (int reserve : {0, 8})
          for (int row_set = 0; row_set < 2; ++row_set) {
            k.walk_dbg = dbg;
            check_walk_cut(op->walk, M, k, cu, reserve, row_set != 0, what);
          }
      k.walk_dbg = 0;
      if (op->walk2.valid) check_walk2_cut(op->walk2, M, k, cu, what);
    }
  if (op->walk2.valid) ++n_walk2;
}

// the named inputs of tests/walk_geometry_cases.h: the same numbers as the launchers computed before the cut became a unit of its own
void check_cut_table() {
  int n_one = 0, n_two = 0;
  for (const CutCase& c : kCutCases) {
    qp::WalkPlan P;
    P.valid = 1;
    P.nn = c.p.nn, P.K = c.p.K, P.z0 = c.p.z0, P.S = c.p.S, P.xl = c.p.xl, P.fd = c.p.fd, P.g = c.p.g;
    for (int i = 0; i < 4; ++i) P.near[i] = c.p.near[i];
    P.R0 = c.p.R0, P.R1 = c.p.R1, P.W0 = c.p.W0, P.n_edge = c.p.n_edge;
    const qp::WalkMatrix M{c.m.nblocks, c.m.nrows, c.m.ncols, c.m.real != 0};
    const qp::WalkKnobs k{c.k.walk_waves, c.k.walk_nt, c.k.walk_dbg, c.k.walk_min_blocks, -1};
    if (!c.two) {
      ++n_one;
      const qp::WalkCut C = qp::walk_cut(P, M, k, c.cu, c.reserve_cu, c.row_set != 0, c.no_edges != 0);
      const qp::WalkGeom& G = C.G;
      REQUIRE((int)C.taken == c.taken, "cut table, %s: taken %d", c.name, (int)C.taken);
      if (!C.taken) continue;
      REQUIRE(C.ws == c.ws && C.ntm == c.ntm && C.grid == c.grid, "cut table, %s: ws %d ntm %d grid %u", c.name, C.ws, C.ntm, C.grid);
      REQUIRE(G.L == c.g1.L && G.nseg == c.g1.nseg && G.n_walk_wg == c.g1.n_walk_wg && G.ntask == c.g1.ntask && G.edge_segs == c.g1.edge_segs &&
                  G.edge_steps == c.g1.edge_steps && G.edge_last == c.g1.edge_last && G.xlast == c.g1.xlast && G.n_edge_wg == c.g1.n_edge_wg,
              "cut table, %s: L %d nseg %d n_walk_wg %d ntask %d edge_segs %d edge_steps %d edge_last %d xlast %lld n_edge_wg %d", c.name, G.L, G.nseg,
              G.n_walk_wg, G.ntask, G.edge_segs, G.edge_steps, G.edge_last, (long long)G.xlast, G.n_edge_wg);
    } else {
      ++n_two;
      const qp::Walk2Cut C = qp::walk2_cut(P, M, k, c.cu);
      const qp::Walk2Geom& G = C.G;
      REQUIRE((int)C.taken == c.taken && C.ntm == c.ntm, "cut table, %s: taken %d ntm %d", c.name, (int)C.taken, C.ntm);
      REQUIRE(G.L == c.g2.L && G.nseg == c.g2.nseg && G.ntask == c.g2.ntask && G.n_walk_wg == c.g2.n_walk_wg && (unsigned)G.n_walk_wg == c.grid && G.S2 == c.g2.S2 &&
                  G.W == c.g2.W && G.xlast == c.g2.xlast && G.vend == c.g2.vend,
              "cut table, %s: L %d nseg %d ntask %d n_walk_wg %d S2 %d W %d xlast %lld vend %lld", c.name, G.L, G.nseg, G.ntask, G.n_walk_wg, G.S2, G.W,
              (long long)G.xlast, (long long)G.vend);
      qp::WalkPlan P1 = P;   // the operator's one-term plan
      P1.W0 = P.W0 - (int64_t)P.K * P.S;
      P1.R1 = P.R1 + (int64_t)P.K * P.S;
      REQUIRE((int)qp::walk2_wanted(P1, P, M, k, c.cu) == c.wanted, "cut table, %s: wanted != %d", c.name, c.wanted);
    }
  }
  // the table's own numbers against the figures the sources document (head of tests/walk_geometry_cases.h)
  const CutCase* t = kCutCases;
  REQUIRE(t[0].g1.ntask <= 768 && t[0].ws == 4 && t[1].g1.ntask == 1024, "cut table: 768 / 1024 wavefronts inside the cache");
  REQUIRE(t[2].g1.n_edge_wg == 24 && t[2].ws == 8 && t[2].g1.ntask <= 8 * (256 - 24) && t[2].grid <= 256, "cut table: 8 x (256 - 24) = 1856 beyond the cache");
  REQUIRE(t[3].g1.n_edge_wg == 0 && t[3].g1.ntask == 2048, "cut table: 2048 with the edge blocks inside the walk");
  for (const CutCase& c : kCutCases)
    if (c.two && c.p.nn == 4 && c.p.g == 1024) REQUIRE(c.g2.W == 56 && c.g2.S2 == 19, "cut table, %s: W = 56, S2 = 19", c.name);
  REQUIRE(n_one >= 9 && n_two >= 3, "cut table: %d one-term and %d two-term cases", n_one, n_two);
  std::printf("walk geometry: %d named cases (%d one-term, %d two-term) match the table\n", n_one + n_two, n_one, n_two);
}

// how the terms reach qp_matrix_create (--large): the index base, real values as QP_VAL_F64, and `raw` -- the arrays really passed
// in, whose canonical form (columns ascending, repeated columns summed) the terms are
struct InputForm {
  int index_base = 0;
  bool f64 = false;
  const std::vector<Csr>* raw = nullptr;
};
struct Features {   // of the operator check_operator built last (--large prints and requires them)
  int built = 0, format = 0, walk = 0, walk2 = 0, cv = 0, cb = 0, sparse_from = -1, planes_real = 0;
  long long n_lattice_fill = 0, cb_tiles = 0, stored = 0, lstored = 0, nblocks = 0, relayouts = 0;
} g_last;
bool g_large = false;

void check_operator(qp_ctx* ctx, const std::vector<Csr>& terms, int ncoeffs, int format, const char* what, const InputForm& in = InputForm()) {
  std::vector<qp_matrix*> ms;
  g_last = Features();
  for (size_t l = 0; l < terms.size(); ++l) {
    const Csr& t = in.raw ? (*in.raw)[l] : terms[l];
    qp_matrix* m = nullptr;
    std::vector<int64_t> idx(t.col.size()), rp(t.rp.size());
    for (size_t p = 0; p < idx.size(); ++p) idx[p] = (int64_t)t.col[p] + in.index_base;
    for (size_t r = 0; r < rp.size(); ++r) rp[r] = t.rp[r] + in.index_base;
    std::vector<double> re;
    if (in.f64) {
      re.resize(t.val.size());
      for (size_t p = 0; p < re.size(); ++p) {
        REQUIRE(t.val[p].im == 0.0, "%s: QP_VAL_F64 input wants real values", what);
        re[p] = t.val[p].re;
      }
    }
    REQUIRE(qp_matrix_create(ctx, t.nrows, t.ncols, (int64_t)t.col.size(), rp.data(), idx.data(), in.f64 ? (const void*)re.data() : (const void*)t.val.data(),
                             in.f64 ? QP_VAL_F64 : QP_VAL_C128, QP_LAYOUT_CSR, in.index_base, QP_FMT_AUTO, &m) == QP_OK,
            "%s: qp_matrix_create: %s", what, qp::g_last_error.c_str());
    ms.push_back(m);
  }
  qp_operator* op = nullptr;
  const int rc = qp_operator_create(ctx, ms.data(), (int)ms.size(), ncoeffs, format, &op);
  if (rc != QP_OK) {   // a request the library refuses (e.g. HRB for a non-Hermitian operator) is fine; a crash is not
    for (auto m : ms) qp_matrix_destroy(m);
    return;
  }
  ++n_cases;
  const DevMatrix& A = op->A;
  const int64_t nrows = A.nrows, ncols = A.ncols;
  if (A.format == QP_FMT_HRB) ++n_hrb;
  if (A.format == QP_FMT_DENSE) ++n_dense;
  if (op->walk.valid) ++n_walked;
  if (op->cv.valid) ++n_coded;
  if (op->cb.valid) ++n_cb;
  if (g_digest) print_digest(op, what);
  g_last.built = 1, g_last.format = A.format, g_last.walk = op->walk.valid, g_last.walk2 = op->walk2.valid, g_last.cv = op->cv.valid, g_last.cb = op->cb.valid;
  g_last.sparse_from = op->sparse_from, g_last.planes_real = op->planes_real, g_last.n_lattice_fill = op->n_lattice_fill;
  g_last.cb_tiles = op->cb.valid ? (long long)op->cb.ntiles : 0, g_last.stored = A.stored, g_last.lstored = A.lstored, g_last.nblocks = A.nblocks;
  if (g_large)
    std::printf("features %s | format %d walk.valid %d walk2.valid %d n_lattice_fill %lld cv.valid %d cb.valid %d (tiles %lld) sparse_from %d planes_real %d | "
                "rows %lld blocks %lld stored %lld lower %lld\n",
                what, g_last.format, g_last.walk, g_last.walk2, g_last.n_lattice_fill, g_last.cv, g_last.cb, g_last.cb_tiles, g_last.sparse_from, g_last.planes_real,
                (long long)nrows, g_last.nblocks, g_last.stored, g_last.lstored);
  // ---- round trip: one term, unit coefficient -> the input bit for bit (more terms: the union pattern, values summed)
  {
    const int64_t nnz = A.nnz;
    std::vector<int64_t> rp((size_t)nrows + 1);
    std::vector<int32_t> col((size_t)std::max<int64_t>(nnz, 1));
    std::vector<qp_c128> val((size_t)std::max<int64_t>(nnz, 1));
    REQUIRE(qp_operator_get_csr(op, rp.data(), col.data(), val.data()) == QP_OK, "%s: get_csr: %s", what, qp::g_last_error.c_str());
    for (int64_t r = 0; r < nrows; ++r)
      for (int64_t p = rp[r]; p < rp[r + 1]; ++p) REQUIRE(col[p] >= 0 && col[p] < ncols, "%s: get_csr column %d of row %lld outside [0, %lld)", what, col[p], (long long)r, (long long)ncols);
    if (terms.size() == 1 && op->n_lattice_fill == 0 && A.format != QP_FMT_DENSE) {
      const Csr& t = terms[0];
      REQUIRE(nnz == (int64_t)t.col.size(), "%s: nnz %lld != %zu", what, (long long)nnz, t.col.size());
      for (int64_t r = 0; r <= nrows; ++r) REQUIRE(rp[r] == t.rp[r], "%s: rowptr[%lld]", what, (long long)r);
      for (int64_t p = 0; p < nnz; ++p)
        REQUIRE(col[p] == t.col[p] && val[p].re == t.val[p].re && val[p].im == t.val[p].im,   // (== : a conjugated zero is -0.0)
                "%s: entry %lld differs after the round trip: column %d value (%.17g, %.17g), passed in column %d value (%.17g, %.17g) [format %d, coded %d]", what,
                (long long)p, col[p], val[p].re, val[p].im, t.col[p], t.val[p].re, t.val[p].im, A.format, op->cv.valid);
    }
  }
  // ---- every stored slot of the row-block formats: a column inside the matrix, zero pads, valid transposed positions
  if (A.format == QP_FMT_RBCSR || A.format == QP_FMT_HRB) {
    const HostLayout& Lh = op->layout;
    const bool hrb = A.format == QP_FMT_HRB;
    const char* ub = reinterpret_cast<const char*>(A.cols);
    const char* lb = reinterpret_cast<const char*>(A.lcols);
    for (int64_t b = 0; b < A.nblocks; ++b) {
      const int64_t wu = (Lh.bptr[b + 1] - Lh.bptr[b]) / kRB;
      for (int64_t k = 0; k < wu; ++k)
        for (int l = 0; l < kRB; ++l) {
          const int64_t row = b * kRB + l, rowc = std::min(row, nrows - 1);   // (the kernels clamp the lanes beyond the last row)
          const int64_t c = decode_any(ub, Lh.cmeta[b], k, l, rowc);
          REQUIRE(c >= 0 && c < ncols, "%s: upper slot %lld of block %lld lane %d decodes to column %lld outside [0, %lld) (mode %d)", what,
                  (long long)k, (long long)b, l, (long long)c, (long long)ncols, (int)(Lh.cmeta[b] & 3));
          const int64_t nl = (hrb && row < nrows) ? Lh.nlow[row] : 0;
          const int64_t len = row < nrows ? op->u_rowptr[row + 1] - op->u_rowptr[row] - nl : 0;
          if (k >= len)   // a pad: inert in every term
            for (double2* plane : op->planes) {
              const double2 v = plane[Lh.bptr[b] + k * kRB + l];
              REQUIRE(v.x == 0.0 && v.y == 0.0, "%s: pad slot %lld of block %lld lane %d carries (%g, %g)", what, (long long)k, (long long)b, l, v.x, v.y);
            }
        }
      if (hrb) {
        const int64_t wl = (Lh.lptr[b + 1] - Lh.lptr[b]) / kRB;
        const bool stencil = (Lh.lcmeta[b] & 3) == 2;
        for (int64_t k = 0; k < wl; ++k)
          for (int l = 0; l < kRB; ++l) {
            const int64_t row = b * kRB + l, rowc = std::min(row, nrows - 1);
            int64_t c;
            if (stencil) {
              LowerStencilSlot e;
              std::memcpy(&e, lb + (Lh.lcmeta[b] >> 2) + (size_t)k * sizeof(e), sizeof(e));
              c = rowc + e.delta;
              const int64_t pos = (((c >> 6) == e.cb0) ? e.pb0 : e.pb1) + (c & 63);
              REQUIRE(pos >= 0 && pos < A.stored, "%s: stencil lower slot %lld of block %lld lane %d reads position %lld outside [0, %lld)", what,
                      (long long)k, (long long)b, l, (long long)pos, (long long)A.stored);
            } else {
              c = decode_any(lb, Lh.lcmeta[b], k, l, rowc);
              const int32_t pos = A.lpos[Lh.lptr[b] + (k >> 2) * (4 * kRB) + l * 4 + (k & 3)];
              REQUIRE(pos >= -1 && pos < A.stored, "%s: lower slot %lld of block %lld lane %d: position %d outside [-1, %lld)", what, (long long)k,
                      (long long)b, l, pos, (long long)A.stored);
            }
            REQUIRE(c >= 0 && c < ncols, "%s: lower slot %lld of block %lld lane %d decodes to column %lld outside [0, %lld)", what, (long long)k,
                    (long long)b, l, (long long)c, (long long)ncols);
          }
      }
    }
    if (op->walk.valid) {   // the walk's edge list names blocks of the operator
      for (int64_t i = 0; i < op->walk.n_edge; ++i)
        REQUIRE(op->walk.edge_map[i] >= 0 && op->walk.edge_map[i] < A.nblocks, "%s: edge block %d", what, op->walk.edge_map[i]);
      REQUIRE(op->walk.R0 >= 0 && op->walk.R1 <= A.nblocks && op->walk.W0 >= op->walk.R0, "%s: walk run [%lld, %lld)", what, (long long)op->walk.R0, (long long)op->walk.R1);
      check_walk_geometry(op, what);
    }
    if (op->cv.valid) {     // value dictionary: every code inside its block's table
      for (int64_t b = 0; b < A.nblocks; ++b) {
        const int64_t tp = op->cv.tptr[b], len = tp & 511, first = tp >> 9;
        REQUIRE(first >= 0 && first + len <= op->cv.ntab && len <= 256, "%s: table of block %lld", what, (long long)b);
        for (int64_t p = Lh.bptr[b]; p < Lh.bptr[b + 1]; ++p) REQUIRE(op->cv.codes[p] < len, "%s: code %d beyond the table of block %lld", what, op->cv.codes[p], (long long)b);
      }
    }
  }
  if (op->cb.valid) {       // column-blocked mirror: columns inside the matrix, map inside the value array
    for (int64_t p = 0; p < op->cb.nnz; ++p) {
      REQUIRE((int64_t)op->cb.cols[p] < ncols, "%s: mirror column %u", what, op->cb.cols[p]);
      const int64_t m = op->cb.map[p], pos = m >= 0 ? m : -m - 1;
      REQUIRE(pos < A.stored, "%s: mirror map %lld", what, (long long)m);
    }
  }
  // coefficients change: the refresh paths (combined plane, sparse control terms, tables) stay inside their arrays
  if (ncoeffs > 0) {
    std::vector<qp_c128> c((size_t)ncoeffs);
    for (int rep = 0; rep < 3; ++rep) {
      for (int i = 0; i < ncoeffs; ++i) c[(size_t)i] = qp_c128{0.25 * (rep + 1) - i, rep == 2 ? 0.5 : 0.0};
      REQUIRE(qp_operator_set_coeffs(op, c.data(), ncoeffs) == QP_OK, "%s: set_coeffs: %s", what, qp::g_last_error.c_str());
    }
    g_last.relayouts = op->n_relayouts;
    if (g_large) {   // (a complex coefficient has sent a Hermitian-packed operator back to plain row blocks: the second build's arrays)
      std::printf("features %s, after set_coeffs | format %d relayouts %lld\n", what, A.format, g_last.relayouts);
      print_digest(op, (std::string(what) + ", after set_coeffs").c_str());
    }
  }
  qp_operator_destroy(op);
  for (auto m : ms) qp_matrix_destroy(m);
}

Csr random_csr(std::mt19937_64& rng, int64_t nrows, int64_t ncols, int maxlen, int nvals, bool hermitian) {
  std::vector<std::vector<std::pair<int32_t, std::complex<double>>>> rows((size_t)nrows);
  std::vector<std::complex<double>> palette((size_t)nvals);
  std::normal_distribution<double> g;
  for (auto& v : palette) v = {g(rng), (rng() & 1) ? g(rng) : 0.0};
  for (int64_t r = 0; r < nrows; ++r) {
    const int len = (rng() % 7 == 0) ? 0 : (int)(rng() % (uint64_t)(maxlen + 1));
    for (int k = 0; k < len; ++k) {
      const int32_t c = (int32_t)(rng() % (uint64_t)ncols);
      std::complex<double> v = palette[rng() % palette.size()];
      if (hermitian) {
        if (c >= nrows || r >= ncols) continue;
        if (c == r) v = {v.real(), 0.0};
        rows[(size_t)r].push_back({c, v});
        if (c != r) rows[(size_t)c].push_back({(int32_t)r, std::conj(v)});
      } else {
        rows[(size_t)r].push_back({c, v});
      }
    }
  }
  Csr out;
  out.nrows = nrows;
  out.ncols = ncols;
  out.rp.assign((size_t)nrows + 1, 0);
  for (int64_t r = 0; r < nrows; ++r) {
    auto& rr = rows[(size_t)r];
    std::sort(rr.begin(), rr.end(), [](auto& a, auto& b) { return a.first < b.first; });
    // (duplicates: keep the first of a column; for the Hermitian case both triangles dropped the same ones by symmetry of the sort)
    int32_t last = -1;
    for (auto& e : rr)
      if (e.first != last) {
        out.col.push_back(e.first);
        out.val.push_back(qp_c128{e.second.real(), e.second.imag()});
        last = e.first;
      }
    out.rp[(size_t)r + 1] = (int64_t)out.col.size();
  }
  if (hermitian) {   // make the kept entries exactly conjugate-symmetric: rebuild the lower triangle from the upper one
    std::vector<std::vector<std::pair<int32_t, qp_c128>>> sym((size_t)nrows);
    for (int64_t r = 0; r < nrows; ++r)
      for (int64_t p = out.rp[r]; p < out.rp[r + 1]; ++p)
        if (out.col[p] >= r) {
          sym[(size_t)r].push_back({out.col[p], out.val[p]});
          if (out.col[p] != r) sym[(size_t)out.col[p]].push_back({(int32_t)r, qp_c128{out.val[p].re, -out.val[p].im}});
        }
    out.col.clear();
    out.val.clear();
    for (int64_t r = 0; r < nrows; ++r) {
      auto& rr = sym[(size_t)r];
      std::sort(rr.begin(), rr.end(), [](auto& a, auto& b) { return a.first < b.first; });
      for (auto& e : rr) {
        out.col.push_back(e.first);
        out.val.push_back(e.second);
      }
      out.rp[(size_t)r + 1] = (int64_t)out.col.size();
    }
  }
  return out;
}

// a Hermitian lattice: col = (i +- d) mod N for the given distances (the headline's generator), optional open ends
Csr lattice(std::mt19937_64& rng, int64_t N, const std::vector<int64_t>& dist, bool periodic, bool constant) {
  std::vector<std::vector<std::pair<int32_t, qp_c128>>> rows((size_t)N);
  std::normal_distribution<double> g;
  for (int64_t i = 0; i < N; ++i)
    for (int64_t d : dist) {
      int64_t j = i + d;
      if (j >= N) {
        if (!periodic) continue;
        j -= N;
      }
      if (j == i) continue;
      const qp_c128 v = constant ? qp_c128{-1.0, 0.0} : qp_c128{g(rng), g(rng)};
      rows[(size_t)i].push_back({(int32_t)j, v});
      rows[(size_t)j].push_back({(int32_t)i, qp_c128{v.re, -v.im}});
    }
  Csr out;
  out.nrows = out.ncols = N;
  out.rp.assign((size_t)N + 1, 0);
  for (int64_t r = 0; r < N; ++r) {
    auto& rr = rows[(size_t)r];
    std::sort(rr.begin(), rr.end(), [](auto& a, auto& b) { return a.first < b.first; });
    int32_t last = -1;
    for (auto& e : rr)
      if (e.first != last) {
        out.col.push_back(e.first);
        out.val.push_back(e.second);
        last = e.first;
      }
    out.rp[(size_t)r + 1] = (int64_t)out.col.size();
  }
  return out;
}

// transverse-field Ising chain (qubit-register structure: row XOR 2^i), few distinct values
Csr tfim(int n) {
  const int64_t N = (int64_t)1 << n;
  Csr out;
  out.nrows = out.ncols = N;
  out.rp.assign((size_t)N + 1, 0);
  for (int64_t r = 0; r < N; ++r) {
    std::vector<std::pair<int32_t, double>> rr;
    double diag = 0.0;
    for (int i = 0; i + 1 < n; ++i) diag -= (((r >> i) & 1) == ((r >> (i + 1)) & 1)) ? 1.0 : -1.0;
    rr.push_back({(int32_t)r, diag});
    for (int i = 0; i < n; ++i) rr.push_back({(int32_t)(r ^ ((int64_t)1 << i)), -1.0});
    std::sort(rr.begin(), rr.end());
    for (auto& e : rr) {
      out.col.push_back(e.first);
      out.val.push_back(qp_c128{e.second, 0.0});
    }
    out.rp[(size_t)r + 1] = (int64_t)out.col.size();
  }
  return out;
}

// ---- generators without a standard-library distribution (their operators' plans are pinned in tests/operator_plan_cases.h) ------
struct Lcg {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
};
// up to `maxlen` entries per row at columns drawn by the generator above (value 1)
Csr lcg_csr(uint64_t seed, int64_t nrows, int64_t ncols, int minlen, int maxlen) {
  Lcg g{seed};
  Csr out;
  out.nrows = nrows;
  out.ncols = ncols;
  out.rp.assign((size_t)nrows + 1, 0);
  std::vector<int32_t> row;
  for (int64_t r = 0; r < nrows; ++r) {
    row.clear();
    const int len = minlen + (int)(g.next() % (uint32_t)(maxlen - minlen + 1));
    for (int k = 0; k < len; ++k) row.push_back((int32_t)(g.next() % (uint64_t)ncols));
    std::sort(row.begin(), row.end());
    row.erase(std::unique(row.begin(), row.end()), row.end());
    for (int32_t c : row) {
      out.col.push_back(c);
      out.val.push_back(qp_c128{1.0, 0.0});
    }
    out.rp[(size_t)r + 1] = (int64_t)out.col.size();
  }
  return out;
}
// five-point stencil on an nx x ny grid with open boundaries, row = y nx + x
Csr open_grid(int64_t nx, int64_t ny) {
  Csr out;
  out.nrows = out.ncols = nx * ny;
  out.rp.assign((size_t)(nx * ny) + 1, 0);
  for (int64_t y = 0; y < ny; ++y)
    for (int64_t x = 0; x < nx; ++x) {
      const int64_t r = y * nx + x;
      auto put = [&](int64_t c, double v) {
        out.col.push_back((int32_t)c);
        out.val.push_back(qp_c128{v, 0.0});
      };
      if (y > 0) put(r - nx, -1.0);
      if (x > 0) put(r - 1, -1.0);
      put(r, 4.0);
      if (x + 1 < nx) put(r + 1, -1.0);
      if (y + 1 < ny) put(r + nx, -1.0);
      out.rp[(size_t)r + 1] = (int64_t)out.col.size();
    }
  return out;
}
Csr const_lattice(int64_t N, const std::vector<int64_t>& dist, bool periodic = true) {
  std::mt19937_64 unused(1);   // (constant values: the generator draws nothing)
  return lattice(unused, N, dist, periodic, true);
}

struct Pattern {   // a Csr's pattern as the planners take it
  UnionRowptr ur;
  UnionCols uc;
  int64_t nrows, ncols;
  explicit Pattern(const Csr& c) : ur(c.rp.begin(), c.rp.end()), uc(c.col.begin(), c.col.end()), nrows(c.nrows), ncols(c.ncols) {}
  UnionPattern view() const { return UnionPattern{nrows, ncols, ur, uc}; }
};

// ---- the batched path's plans, checked by construction (csrc/operator_plans.cpp: plan_spmm_order, plan_spmm_tiles, spmm_tile_table) ----
int64_t n_panel_orders = 0, n_panel_tiles = 0, n_panel_operands = 0;
// want_order / want_tiles: must SOME knob setting take the plan (1), must none (0)
void check_panel_plans(const Csr& csr, const char* what, int want_order, int want_tiles, int want_rest = -1, int want_T = 0) {
  const Pattern pat(csr);
  const UnionPattern A = pat.view();
  const int64_t n = A.nrows;
  int got_order = 0, got_tiles = 0;
  for (int knob : {-1, 0, 8, 64}) {
    for (int batch : {1, 8, 64, 130}) {
      const SpmmOrder O = plan_spmm_order(A, batch, knob);
      if (O.order.empty()) {
        REQUIRE(O.g == 0 && O.sw == 0, "%s: no row order but g %lld sw %lld", what, (long long)O.g, (long long)O.sw);
        continue;
      }
      got_order = 1;
      ++n_panel_orders;
      REQUIRE((int64_t)O.order.size() == n && O.g >= 256 && O.sw >= 1 && O.sw < O.g && O.g % O.sw == 0, "%s: row order of %zu rows, g %lld sw %lld", what,
              O.order.size(), (long long)O.g, (long long)O.sw);
      std::vector<char> seen((size_t)n, 0);
      for (int32_t r : O.order) {
        REQUIRE(r >= 0 && r < n && !seen[(size_t)r], "%s (strip %d, batch %d): row %d twice in the order, or outside the matrix", what, knob, batch, r);
        seen[(size_t)r] = 1;
      }
    }
    const SpmmTilesHost P = plan_spmm_tiles(A, knob);
    if (P.tiles.empty()) {
      REQUIRE(P.rest.empty() && P.g == 0 && P.sw == 0 && P.shape.nd == 0, "%s: an empty tile plan carries data", what);
      continue;
    }
    got_tiles = 1;
    ++n_panel_tiles;
    const qp::SpmmTileShape& sh = P.shape;
    const int64_t g = P.g;
    REQUIRE(16 * (int64_t)P.tiles.size() >= n / 2, "%s: %zu tiles cover less than half of %lld rows", what, P.tiles.size(), (long long)n);
    REQUIRE(g >= 64 && sh.nd >= 2 && sh.nd <= qp::kSpmmTileMaxEntries && sh.K >= 1 && sh.K <= 4 && sh.NN >= 0 && sh.NN <= 4, "%s: tile shape", what);
    std::vector<int64_t> D((size_t)sh.nd);   // the candidate distance list
    for (int k = 0; k < sh.nd; ++k) D[(size_t)k] = sh.dnear[k] != 0 ? (int64_t)sh.dnear[k] : (int64_t)sh.dfar[k] * g;
    std::vector<char> owner((size_t)n, 0);
    for (int32_t r0 : P.tiles)
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
          const int64_t r = (int64_t)r0 + i * g + j;
          REQUIRE(r0 >= 0 && r < n, "%s: tile %d row %lld outside the matrix", what, r0, (long long)r);
          REQUIRE(!owner[(size_t)r], "%s: row %lld in two tiles", what, (long long)r);
          owner[(size_t)r] = 1;
          REQUIRE(A.ur[r + 1] - A.ur[r] == sh.nd, "%s: tile row %lld has %lld entries, the candidate %d", what, (long long)r, (long long)(A.ur[r + 1] - A.ur[r]), sh.nd);
          for (int k = 0; k < sh.nd; ++k)
            REQUIRE((int64_t)A.uc[A.ur[r] + k] - r == D[(size_t)k], "%s: entry %d of tile row %lld is not at distance %lld", what, k, (long long)r, (long long)D[(size_t)k]);
        }
    for (int32_t r : P.rest) {
      REQUIRE(r >= 0 && r < n && !owner[(size_t)r], "%s: rest row %d is in a tile, listed twice or outside the matrix", what, r);
      owner[(size_t)r] = 1;
    }
    for (int64_t r = 0; r < n; ++r) REQUIRE(owner[(size_t)r], "%s: row %lld in neither a tile nor the rest", what, (long long)r);
    if (want_rest >= 0) REQUIRE((int)!P.rest.empty() == want_rest, "%s: %zu rest rows", what, P.rest.size());
    // the kernel's table (csrc/kernels_spmm.hip, spmm_tile_kernel: LDS byte offset tab[80 + 24 w + k] of wavefront w's entry k)
    const SpmmTileTable T = spmm_tile_table(sh, g);
    const std::vector<int32_t>& tab = T.tab;
    REQUIRE(T.T == 16 + 8 * sh.K + 8 * sh.NN && T.T <= qp::kSpmmTileSlots && (int)tab.size() == qp::kSpmmTileTab, "%s: T %d", what, T.T);
    if (want_T) REQUIRE(T.T == want_T, "%s: T %d, expected %d", what, T.T, want_T);
    for (int a = 0; a < T.T; ++a)
      for (int b = a + 1; b < T.T; ++b) REQUIRE(tab[(size_t)a] != tab[(size_t)b], "%s: staged slots %d and %d hold the same row %d", what, a, b, tab[(size_t)a]);
    const int base = qp::kSpmmTileSlots, per = qp::kSpmmTileMaxEntries;
    for (int w = 0; w < 16; ++w) {
      const int64_t own_row = (int64_t)(w / 4) * g + w % 4;
      for (int k = 0; k < sh.nd; ++k) {
        const int32_t off = tab[(size_t)(base + per * w + k)];
        REQUIRE(off >= 0 && off % 1024 == 0 && off < T.T * 1024, "%s: operand offset %d of wavefront %d entry %d", what, off, w, k);
        REQUIRE((int64_t)tab[(size_t)(off / 1024)] == own_row + D[(size_t)k], "%s: wavefront %d entry %d reads staged row %d, its column is row + %lld", what, w, k,
                tab[(size_t)(off / 1024)], (long long)(own_row + D[(size_t)k]));
        ++n_panel_operands;
      }
      REQUIRE((int64_t)tab[(size_t)(base + per * 16 + w)] == own_row, "%s: own row of wavefront %d", what, w);
      const int32_t own_off = tab[(size_t)(base + per * 16 + 16 + w)];
      REQUIRE(own_off >= 0 && own_off % 1024 == 0 && own_off < T.T * 1024 && (int64_t)tab[(size_t)(own_off / 1024)] == own_row, "%s: own-row offset %d of wavefront %d", what, own_off, w);
    }
  }
  REQUIRE(want_order < 0 || got_order == want_order, "%s: row order taken %d, expected %d", what, got_order, want_order);
  REQUIRE(want_tiles < 0 || got_tiles == want_tiles, "%s: tiles taken %d, expected %d", what, got_tiles, want_tiles);
}

// the open-boundary grid as the operator build completes it
Csr completed(const Csr& c, int min_blocks) {
  Pattern p(c);
  PlanKnobs k;
  k.walk_min_blocks = min_blocks;
  lattice_fill(k, p.nrows, p.ncols, p.ur, p.uc);
  REQUIRE((int64_t)p.uc.size() > (int64_t)c.col.size(), "lattice_fill left the %lld x %lld open grid as it was", (long long)c.nrows, (long long)c.ncols);
  Csr out;
  out.nrows = c.nrows;
  out.ncols = c.ncols;
  out.rp.assign(p.ur.begin(), p.ur.end());
  out.col.assign(p.uc.begin(), p.uc.end());
  out.val.assign(out.col.size(), qp_c128{0.0, 0.0});
  return out;
}

void check_panel_plan_cases() {
  std::mt19937_64 rng(7);
  for (const auto& st : std::vector<std::vector<int64_t>>{{1, 2, 3, 4, 64, 128, 192, 256}, {1, 64}, {1, 2, 100, 200}, {1, 63, 64, 65}, {1, 32, 1024}, {3, 17}, {20, 40}})
    for (int64_t N : {(int64_t)4096, (int64_t)5000, (int64_t)16384 + 77})
      for (int periodic = 0; periodic < 2; ++periodic) check_panel_plans(lattice(rng, N, st, periodic != 0, false), "lattice generator", -1, -1);
  check_panel_plans(const_lattice(4096, {1, 64}), "64 x 64 periodic grid", 0, 1);
  check_panel_plans(const_lattice(4096, {1, 256}), "256 x 16 periodic grid", 1, 1);
  check_panel_plans(completed(open_grid(96, 64), 16), "open 96 x 64 grid, completed", 0, 1, 1);
  check_panel_plans(const_lattice((int64_t)1 << 15, {1, 2, 3, 4, 1024, 2048, 3072, 4096}), "(4,4) lattice, g = 1024", 1, 1);
  check_panel_plans(const_lattice(4096, {1, 2, 3, 4, 64, 128, 192, 256}), "K = NN = 4 at g = 64", 0, 1, -1, qp::kSpmmTileSlots);
  check_panel_plans(tfim(12), "spin chain", 0, 0);
  check_panel_plans(lcg_csr(11, 4096, 4096, 0, 11), "ragged operator", 0, 0);
  std::printf("panel plans: %lld row orders are permutations, %lld tile plans partition their rows, %lld LDS operands name their entry's column\n",
              (long long)n_panel_orders, (long long)n_panel_tiles, (long long)n_panel_operands);
}

// ---- every verdict of the walk's shape parser (tests/operator_plan_cases.h) ------------------------------------------------------
std::string c_string(const std::string& s) {
  std::string out = "\"";
  for (char c : s) {
    if (c == '"' || c == '\\') out += '\\';
    out += c;
  }
  return out + "\"";
}
void check_shape_table(bool print) {
  int n_ok = 0, n_refused = 0;
  for (const ShapeCase& c : kShapeCases) {
    const std::vector<int64_t> dl(c.d, c.d + c.n);
    WalkShape w;
    std::string text;
    const int code = walk_shape_reason(dl, w, &text);
    if (code != QP_WALK_OK) w = WalkShape();
    (code == QP_WALK_OK ? n_ok : n_refused)++;
    if (print) {
      std::printf("  {%s, %d, {", c_string(c.name).c_str(), c.n);
      for (int k = 0; k < c.n; ++k) std::printf("%s%lld", k ? "," : "", c.d[k]);
      std::printf("}, %d, %s, %d,%d,%d,%d,%d, %lld,%lld,%lld, {%d,%d,%d,%d}},\n", code, c_string(text).c_str(), w.nn, w.K, w.z0, w.xl, w.fd, (long long)w.g,
                  (long long)w.glong, (long long)w.glong1, w.near[0], w.near[1], w.near[2], w.near[3]);
      continue;
    }
    REQUIRE(code == c.code && text == c.text, "shape table, %s: code %d \"%s\", expected %d \"%s\"", c.name, code, text.c_str(), c.code, c.text);
    REQUIRE(parse_walk_shape(dl, w) == (c.code == QP_WALK_OK), "shape table, %s: parse_walk_shape", c.name);
    if (code != QP_WALK_OK) continue;
    REQUIRE(w.nn == c.nn && w.K == c.K && w.z0 == c.z0 && w.xl == c.xl && w.fd == c.fd && w.g == c.g && w.glong == c.glong && w.glong1 == c.glong1 &&
                w.near[0] == c.near[0] && w.near[1] == c.near[1] && w.near[2] == c.near[2] && w.near[3] == c.near[3],
            "shape table, %s: nn %d K %d z0 %d xl %d fd %d g %lld glong %lld glong1 %lld near %d %d %d %d", c.name, w.nn, w.K, w.z0, w.xl, w.fd, (long long)w.g,
            (long long)w.glong, (long long)w.glong1, w.near[0], w.near[1], w.near[2], w.near[3]);
  }
  if (!print) std::printf("walk shapes: %d accepted and %d refused distance lists match the table\n", n_ok, n_refused);
}

// ---- named operators -> whole plans (tests/operator_plan_cases.h) ------------------------------------------------------------------
struct PlanInput {
  const char* name;
  Csr (*make)();
  int format;
  std::vector<std::pair<const char*, int>> knobs;
  bool sweep_cu;   // also at 8 and 64 compute units (the column-blocked mirror's tiles-per-wavefront gate reads the count)
};
const PlanInput kPlanInputs[] = {
    {"(4,4) lattice g 64, N 4096", [] { return const_lattice(4096, {1, 2, 3, 4, 64, 128, 192, 256}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"(1,1) lattice g 64, N 5000, open ends", [] { return const_lattice(5000, {1, 64}, false); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"(2,2) lattice g 100, N 16461", [] { return const_lattice(16461, {1, 2, 100, 200}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"nine-point lattice g 64, N 16461", [] { return const_lattice(16461, {1, 63, 64, 65}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"nine-point lattice g 65, N 16461", [] { return const_lattice(16461, {1, 64, 65, 66}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"near distance 32, N 4096, packed", [] { return const_lattice(4096, {1, 32, 1024}); }, QP_FMT_HRB, {{"walk_min_blocks", 8}}, false},
    {"band of five, N 4096, packed", [] { return const_lattice(4096, {1, 2, 3, 4, 5}); }, QP_FMT_HRB, {{"walk_min_blocks", 8}}, false},
    {"(4,4) lattice g 1024, N 2^15", [] { return const_lattice((int64_t)1 << 15, {1, 2, 3, 4, 1024, 2048, 3072, 4096}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"chain of blocks g 64, N 2048", [] { return const_lattice(2048, {1, 64}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"64 x 64 periodic grid", [] { return const_lattice(4096, {1, 64}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"256 x 16 periodic grid", [] { return const_lattice(4096, {1, 256}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"256 x 16 periodic grid, strips of 8", [] { return const_lattice(4096, {1, 256}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}, {"spmm_strip", 8}}, false},
    {"open 96 x 64 grid", [] { return open_grid(96, 64); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"open 96 x 64 grid, default knobs", [] { return open_grid(96, 64); }, QP_FMT_AUTO, {}, false},
    {"12-spin chain", [] { return tfim(12); }, QP_FMT_AUTO, {}, false},
    {"12-spin chain, packed", [] { return tfim(12); }, QP_FMT_HRB, {}, false},
    {"ragged 4096 x 4096", [] { return lcg_csr(11, 4096, 4096, 0, 11); }, QP_FMT_RBCSR, {}, false},
    {"random columns N 4096, mirror forced", [] { return lcg_csr(12, 4096, 4096, 8, 8); }, QP_FMT_RBCSR, {{"colblock", 2}, {"cb_log2w", 6}}, true},
    {"random columns N 4096, mirror forced, CSR", [] { return lcg_csr(12, 4096, 4096, 8, 8); }, QP_FMT_CSR, {{"colblock", 2}, {"cb_log2w", 6}}, true},
    {"random columns N 2^18, mirror forced", [] { return lcg_csr(13, (int64_t)1 << 18, (int64_t)1 << 18, 2, 2); }, QP_FMT_RBCSR, {{"colblock", 2}, {"cb_log2w", 12}}, true},
    {"long pair 16384, N 2^16: walkable decides", [] { return const_lattice((int64_t)1 << 16, {1, 64, 16384}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}}, false},
    {"long pair 16384, N 2^16: walk off", [] { return const_lattice((int64_t)1 << 16, {1, 64, 16384}); }, QP_FMT_AUTO, {{"walk_min_blocks", 8}, {"hrb_walk", 0}}, false},
};

struct PlanRecord {
  long long s[kPlanScalars];
  double line_share;
  unsigned long long h[kPlanHashes];
  std::string text;
};
uint64_t fnv(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
  return h;
}
// s: format, n_lattice_fill, walk reason | one-term plan, two-term plan: valid nn K z0 S xl glong glong1 fd g R0 R1 W0 U0 ustride n_edge
// near[0..3] | mirror: valid log2w P rpt max_seg ntiles nnz | row order at 64 states: g sw | tiles: valid ntiles nrest g sw T nd K NN
// h: edge lists of the two plans | mirror: segptr rowoff cols map | row order | tiles, rest, table
PlanRecord plan_record(qp_operator* op) {
  PlanRecord R{};
  int i = 0;
  auto put = [&](long long v) { R.s[i++] = v; };
  put(op->A.format), put(op->n_lattice_fill), put(op->walk_reason);
  R.text = op->walk_reason_text;
  int hi = 0;
  for (const qp::WalkPlan* P : {&op->walk, &op->walk2}) {
    for (long long v : {(long long)P->valid, (long long)P->nn, (long long)P->K, (long long)P->z0, (long long)P->S, (long long)P->xl, (long long)P->glong,
                        (long long)P->glong1, (long long)P->fd, (long long)P->g, (long long)P->R0, (long long)P->R1, (long long)P->W0, (long long)P->U0,
                        (long long)P->ustride, (long long)P->n_edge})
      put(v);
    for (int k = 0; k < 4; ++k) put(P->near[k]);
    R.h[hi++] = P->valid ? fnv(P->edge_map, (size_t)P->n_edge * 4) : 0;
  }
  const qp::ColBlockPlan& B = op->cb;
  for (long long v : {(long long)B.valid, (long long)B.log2w, (long long)B.P, (long long)B.rpt, (long long)B.max_seg, (long long)B.ntiles, (long long)B.nnz}) put(v);
  R.line_share = op->cb_line_share;
  R.h[hi++] = B.valid ? fnv(B.segptr, (size_t)(B.ntiles * B.P + 1) * 4) : 0;
  R.h[hi++] = B.valid ? fnv(B.rowoff, (size_t)(B.ntiles * B.P) * (size_t)(64 * B.rpt + 1) * 2) : 0;
  R.h[hi++] = B.valid ? fnv(B.cols, (size_t)B.nnz * 4) : 0;
  R.h[hi++] = B.valid ? fnv(B.map, (size_t)B.nnz * 8) : 0;
  const int32_t* order = nullptr;
  REQUIRE(operator_spmm_order(op, 64, &order) == QP_OK, "operator_spmm_order");
  put(op->m_order_g), put(op->m_order_sw);
  R.h[hi++] = order ? fnv(order, (size_t)op->A.nrows * 4) : 0;
  const qp::SpmmTiles* T = nullptr;
  REQUIRE(operator_spmm_tiles(op, &T) == QP_OK, "operator_spmm_tiles");
  const qp::SpmmTiles& M = op->m_tiles;
  for (long long v : {(long long)M.valid, (long long)M.ntiles, (long long)M.nrest, (long long)M.g, (long long)M.sw, (long long)M.T, (long long)M.shape.nd,
                      (long long)M.shape.K, (long long)M.shape.NN})
    put(v);
  R.h[hi++] = T ? fnv(T->tiles, (size_t)T->ntiles * 4) : 0;
  R.h[hi++] = T ? fnv(T->rest, (size_t)T->nrest * 4) : 0;
  R.h[hi++] = T ? fnv(T->tab, (size_t)qp::kSpmmTileTab * 4) : 0;
  REQUIRE(i == kPlanScalars && hi == kPlanHashes, "plan record: %d scalars, %d hashes", i, hi);
  return R;
}
// the mirror's part of the record on a chip of `cu` compute units: the planner itself, on the operator's pattern and layout
void colblock_record(const qp_operator* op, int cu, PlanRecord& R) {
  const ColBlockHost C = plan_colblock(union_pattern_of(op), op->layout, plan_knobs(op->ctx->tun), cu);
  const qp::ColBlockShape& B = C.shape;
  int i = 43;
  for (long long v : {(long long)B.valid, (long long)B.log2w, (long long)B.P, (long long)B.rpt, (long long)B.max_seg, (long long)B.ntiles, (long long)B.nnz}) R.s[i++] = v;
  if (C.line_share >= 0.0) R.line_share = C.line_share;
  R.h[2] = B.valid ? fnv(C.segptr.data(), C.segptr.size() * 4) : 0;
  R.h[3] = B.valid ? fnv(C.rowoff.data(), C.rowoff.size() * 2) : 0;
  R.h[4] = B.valid ? fnv(C.cols.data(), C.cols.size() * 4) : 0;
  R.h[5] = B.valid ? fnv(C.map.data(), C.map.size() * 8) : 0;
}

void check_plan_table(bool print) {
  int n_rows = 0;
  for (const PlanInput& in : kPlanInputs) {
    qp_ctx* ctx = nullptr;
    REQUIRE(qp_ctx_create(0, nullptr, &ctx) == QP_OK, "qp_ctx_create");
    for (const auto& kv : in.knobs) REQUIRE(qp_ctx_tuning_set(ctx, kv.first, kv.second) == QP_OK, "knob %s", kv.first);
    const Csr t = in.make();
    qp_matrix* m = nullptr;
    std::vector<int64_t> idx(t.col.begin(), t.col.end());
    REQUIRE(qp_matrix_create(ctx, t.nrows, t.ncols, (int64_t)t.col.size(), t.rp.data(), idx.data(), t.val.data(), QP_VAL_C128, QP_LAYOUT_CSR, 0, QP_FMT_AUTO, &m) == QP_OK,
            "%s: qp_matrix_create", in.name);
    qp_operator* op = nullptr;
    REQUIRE(qp_operator_create(ctx, &m, 1, 0, in.format, &op) == QP_OK, "%s: qp_operator_create: %s", in.name, qp::g_last_error.c_str());
    const PlanRecord built = plan_record(op);
    for (int cu : {256, 64, 8}) {
      if (cu != 256 && !in.sweep_cu) continue;
      PlanRecord R = built;
      colblock_record(op, cu, R);
      if (cu == 256) {   // the build asked the (stand-in) device, which has 256
        REQUIRE(std::memcmp(R.s, built.s, sizeof R.s) == 0 && std::memcmp(R.h, built.h, sizeof R.h) == 0 && R.line_share == built.line_share,
                "%s: the planner and the built operator disagree about the column-blocked mirror", in.name);
      }
      ++n_rows;
      if (print) {
        std::printf("  {%s, %d, {", c_string(in.name).c_str(), cu);
        for (int k = 0; k < kPlanScalars; ++k) std::printf("%s%lld", k ? "," : "", R.s[k]);
        std::printf("}, %a, {", R.line_share);
        for (int k = 0; k < kPlanHashes; ++k) std::printf("%s0x%016llxull", k ? "," : "", R.h[k]);
        std::printf("}, %s},\n", c_string(R.text).c_str());
        continue;
      }
      const PlanCase* want = nullptr;
      for (const PlanCase& c : kPlanCases)
        if (std::strcmp(c.name, in.name) == 0 && c.cu == cu) want = &c;
      REQUIRE(want, "plan table: no row for %s at %d compute units", in.name, cu);
      for (int k = 0; k < kPlanScalars; ++k) REQUIRE(R.s[k] == want->s[k], "plan table, %s at %d CUs: scalar %d is %lld, expected %lld", in.name, cu, k, R.s[k], want->s[k]);
      for (int k = 0; k < kPlanHashes; ++k) REQUIRE(R.h[k] == want->h[k], "plan table, %s at %d CUs: hash %d is %016llx, expected %016llx", in.name, cu, k, R.h[k], want->h[k]);
      REQUIRE(R.line_share == want->line_share && R.text == want->text, "plan table, %s at %d CUs: line share %a, reason \"%s\"", in.name, cu, R.line_share, R.text.c_str());
    }
    if (g_digest) print_digest(op, in.name);
    qp_operator_destroy(op);
    qp_matrix_destroy(m);
    qp_ctx_destroy(ctx);
  }
  if (!print) std::printf("operator plans: %d rows of named operators match the table\n", n_rows);
}

// ---- --large: the threaded host build (head of this file) ---------------------------------------------------------------------------
// values without a random number generator: binary fractions of a hash of (row, column), conjugate-symmetric, a real diagonal
qp_c128 arith_value(int64_t r, int64_t c, bool complex_vals) {
  const int64_t lo = std::min(r, c), hi = std::max(r, c);
  const uint32_t h = (uint32_t)((uint64_t)lo * 2654435761ull + (uint64_t)hi * 40503ull + 12345ull);
  const double re = ((double)((h >> 7) % 2001u) - 1000.0) / 1024.0;
  const double im = (complex_vals && r != c) ? ((double)((h >> 18) % 2001u) - 1000.0) / 1024.0 : 0.0;
  return qp_c128{re, r <= c ? im : -im};
}
Csr with_arith_values(Csr m, bool complex_vals) {
  for (int64_t r = 0; r < m.nrows; ++r)
    for (int64_t p = m.rp[(size_t)r]; p < m.rp[(size_t)r + 1]; ++p) m.val[(size_t)p] = arith_value(r, m.col[(size_t)p], complex_vals);
  return m;
}
// k columns per row drawn by the generator of lcg_csr, each with its transpose: a Hermitian operator whose gathers are irregular
Csr lcg_hermitian(uint64_t seed, int64_t n, int k) {
  Lcg g{seed};
  std::vector<std::vector<int32_t>> rows((size_t)n);
  for (int64_t r = 0; r < n; ++r)
    for (int j = 0; j < k; ++j) {
      const int64_t c = (int64_t)(g.next() % (uint64_t)n);
      if (c == r) continue;
      rows[(size_t)r].push_back((int32_t)c);
      rows[(size_t)c].push_back((int32_t)r);
    }
  Csr out;
  out.nrows = out.ncols = n;
  out.rp.assign((size_t)n + 1, 0);
  for (int64_t r = 0; r < n; ++r) {
    auto& row = rows[(size_t)r];
    std::sort(row.begin(), row.end());
    row.erase(std::unique(row.begin(), row.end()), row.end());
    for (int32_t c : row) {
      out.col.push_back(c);
      out.val.push_back(qp_c128{0.0, 0.0});
    }
    out.rp[(size_t)r + 1] = (int64_t)out.col.size();
  }
  return with_arith_values(std::move(out), true);
}
// a control term on few positions: the pairs (i, i + 1), (i + 1, i) for every `every`-th row i, value 1/2
Csr sparse_pairs(int64_t n, int64_t every) {
  Csr out;
  out.nrows = out.ncols = n;
  out.rp.assign((size_t)n + 1, 0);
  for (int64_t r = 0; r < n; ++r) {
    int64_t c = -1;
    if (r % every == 0 && r + 1 < n) c = r + 1;
    else if (r >= 1 && (r - 1) % every == 0) c = r - 1;
    if (c >= 0) {
      out.col.push_back((int32_t)c);
      out.val.push_back(qp_c128{0.5, 0.0});
    }
    out.rp[(size_t)r + 1] = (int64_t)out.col.size();
  }
  return out;
}
// the same matrix as the caller of a sparse() would pass it: every row's columns descending, and the first entry of every fifth
// row twice with half the value each (the halves are exact, their sum is the entry)
Csr scrambled(const Csr& c) {
  Csr out;
  out.nrows = c.nrows;
  out.ncols = c.ncols;
  out.rp.assign((size_t)c.nrows + 1, 0);
  for (int64_t r = 0; r < c.nrows; ++r) {
    const int64_t a = c.rp[(size_t)r], b = c.rp[(size_t)r + 1];
    const bool twice = r % 5 == 0 && b > a;
    const qp_c128 half{0.5 * c.val[(size_t)a].re, 0.5 * c.val[(size_t)a].im};
    if (twice) {
      out.col.push_back(c.col[(size_t)a]);
      out.val.push_back(half);
    }
    for (int64_t p = b - 1; p >= a; --p) {
      out.col.push_back(c.col[(size_t)p]);
      out.val.push_back(twice && p == a ? half : c.val[(size_t)p]);
    }
    out.rp[(size_t)r + 1] = (int64_t)out.col.size();
  }
  return out;
}

long long number_after(const std::string& text, const char* key) {
  const size_t at = text.rfind(key);
  REQUIRE(at != std::string::npos, "\"%s\" does not say \"%s\"", text.c_str(), key);
  return std::atoll(text.c_str() + at + std::strlen(key));
}
// refusals at size: two bad entries in different chunks of the threaded pass, whichever thread names one must name a bad one
void check_errors_at_size(qp_ctx* ctx) {
  const Csr t = const_lattice(((int64_t)1 << 16) + 192, {1, 64});
  const int64_t n = t.nrows, nnz = (int64_t)t.col.size(), b1 = 1000, b2 = n - 1000;
  std::vector<int64_t> idx(t.col.begin(), t.col.end());
  qp_matrix* m = nullptr;
  {
    std::vector<int64_t> rp = t.rp;   // rows b1 and b2 end before they begin; every other row stays monotone
    rp[(size_t)b1 + 1] = rp[(size_t)b1] - 1;
    rp[(size_t)b2 + 1] = rp[(size_t)b2] - 1;
    const int rc = qp_matrix_create(ctx, n, n, nnz, rp.data(), idx.data(), t.val.data(), QP_VAL_C128, QP_LAYOUT_CSR, 0, QP_FMT_AUTO, &m);
    REQUIRE(rc == QP_E_BAD_ARG && m == nullptr, "non-monotone rowptr at size: status %d", rc);
    const long long named = number_after(qp::g_last_error, "at row ");
    REQUIRE(named == b1 || named == b2, "non-monotone rowptr: \"%s\" names row %lld, the bad rows are %lld and %lld", qp::g_last_error.c_str(), named, (long long)b1, (long long)b2);
    std::printf("error path: rowptr not monotone at rows %lld and %lld of %lld -> QP_E_BAD_ARG naming row %lld\n", (long long)b1, (long long)b2, (long long)n, named);
  }
  for (int base = 0; base < 2; ++base) {
    const int64_t p1 = t.rp[(size_t)b1] + 1, p2 = t.rp[(size_t)b2] + 2;
    std::vector<int64_t> bad(idx), rp(t.rp);
    for (auto& v : bad) v += base;
    for (auto& v : rp) v += base;
    bad[(size_t)p1] = n + base;   // one past the last column
    bad[(size_t)p2] = base - 1;   // one before the first
    const int rc = qp_matrix_create(ctx, n, n, nnz, rp.data(), bad.data(), t.val.data(), QP_VAL_C128, QP_LAYOUT_CSR, base, QP_FMT_AUTO, &m);
    REQUIRE(rc == QP_E_BAD_ARG && m == nullptr, "column out of range at size (index base %d): status %d", base, rc);
    const long long named = number_after(qp::g_last_error, "out of range at ");
    REQUIRE(named == p1 || named == p2, "column out of range: \"%s\" names position %lld, the bad ones are %lld and %lld", qp::g_last_error.c_str(), named, (long long)p1, (long long)p2);
    std::printf("error path: columns out of range at positions %lld and %lld (index base %d) -> QP_E_BAD_ARG naming position %lld\n", (long long)p1, (long long)p2, base, named);
  }
}

// a chunk of parallel_rows that throws: the caller catches the exception -- one, whichever chunk was first -- after every other
// chunk has run to its end; the process goes on
void check_throwing_workers() {
  const unsigned hw = host_threads();
  if (hw < 2) {
    std::printf("throwing workers: skipped, one host thread\n");
    return;
  }
  const int64_t n = 1000, chunk = (n + hw - 1) / hw, nchunks = (n + chunk - 1) / chunk;
  int n_checked = 0;
  for (const std::vector<int64_t>& bad : std::vector<std::vector<int64_t>>{{0}, {n / 2}, {n - 1}, {0, n - 1}, {0, n / 2, n - 1}}) {
    std::set<int64_t> bad_chunks;
    for (int64_t r : bad) bad_chunks.insert(r / chunk);
    std::atomic<int64_t> completed{0};
    int caught = 0;
    try {
      parallel_rows(n, [&](int64_t a, int64_t b) {
        for (int64_t r : bad)
          if (a <= r && r < b) throw std::bad_alloc();
        completed.fetch_add(1);
      }, 0);
    } catch (const std::bad_alloc&) {
      ++caught;
    }
    REQUIRE(caught == 1, "throwing workers: %d exceptions reached the caller of a pass with %zu throwing chunks", caught, bad_chunks.size());
    REQUIRE(completed.load() == nchunks - (int64_t)bad_chunks.size(), "throwing workers: %lld of %lld chunks ran to their end, %zu threw", (long long)completed.load(),
            (long long)nchunks, bad_chunks.size());
    ++n_checked;
  }
  std::printf("throwing workers: %d passes of %lld chunks, std::bad_alloc caught by the caller once each, every other chunk joined\n", n_checked, (long long)nchunks);
}

// the same through the C ABI: a worker's scratch vector (the per-row sort of unsorted input) finds no memory -> QP_E_ALLOC
void check_worker_out_of_memory(qp_ctx* ctx) {
#ifdef QP_HARNESS_OWN_NEW
  if (host_threads() < 2) {
    std::printf("worker out of memory: skipped, one host thread\n");
    return;
  }
  const Csr raw = scrambled(lcg_csr(21, ((int64_t)1 << 16) + 129, 30011, 6, 8));
  std::vector<int64_t> idx(raw.col.begin(), raw.col.end());
  qp_matrix* m = nullptr;
  g_new_failures.store(1);
  int rc = qp_matrix_create(ctx, raw.nrows, raw.ncols, (int64_t)raw.col.size(), raw.rp.data(), idx.data(), raw.val.data(), QP_VAL_C128, QP_LAYOUT_CSR, 0, QP_FMT_AUTO, &m);
  const bool fired = g_new_failures.load() <= 0;
  g_new_failures.store(0);
  REQUIRE(fired, "worker out of memory: no allocation was made off the main thread");
  REQUIRE(rc == QP_E_ALLOC && m == nullptr, "worker out of memory: status %d (%s), expected QP_E_ALLOC", rc, qp::g_last_error.c_str());
  rc = qp_matrix_create(ctx, raw.nrows, raw.ncols, (int64_t)raw.col.size(), raw.rp.data(), idx.data(), raw.val.data(), QP_VAL_C128, QP_LAYOUT_CSR, 0, QP_FMT_AUTO, &m);
  REQUIRE(rc == QP_OK && m != nullptr, "worker out of memory: the next qp_matrix_create returned %d (%s)", rc, qp::g_last_error.c_str());
  qp_matrix_destroy(m);
  std::printf("worker out of memory: qp_matrix_create returned QP_E_ALLOC, the next one QP_OK\n");
#else
  (void)ctx;
  std::printf("worker out of memory: skipped in a sanitizer build\n");
#endif
}

int run_large(const char* only) {
  g_large = g_digest = true;
  std::printf("host threads %u\n", host_threads());
  auto fresh_ctx = [](std::initializer_list<std::pair<const char*, int>> knobs) {
    qp_ctx* c = nullptr;
    REQUIRE(qp_ctx_create(0, nullptr, &c) == QP_OK, "qp_ctx_create");
    for (const auto& kv : knobs) REQUIRE(qp_ctx_tuning_set(c, kv.first, kv.second) == QP_OK, "knob %s", kv.first);
    return c;
  };
  qp_ctx* ctx = fresh_ctx({});
  const int64_t N18 = ((int64_t)1 << 18) + 77, N16 = ((int64_t)1 << 16) + 192;   // 4098 row blocks; just past the row threshold
  const std::vector<int64_t> headline{1, 2, 3, 4, 1024, 2048, 3072, 4096};
  // (`--large NAME`: that part of the list alone; `--large -NAME`: the list without it -- the site list then shows what only it reaches)
  auto wanted = [&](const char* name) { return !only || (only[0] == '-' ? std::strcmp(only + 1, name) != 0 : std::strcmp(only, name) == 0); };
#define LARGE_REQUIRE(name, cond) REQUIRE(g_last.built && (cond), "%s: the operator lacks what it is on the list for: " #cond, name)
  if (wanted("banded")) {   // the headline lattice, complex values: Hermitian-packed with both walk plans, plain row blocks, and as chosen
    const std::vector<Csr> big{with_arith_values(const_lattice(N18, headline), true)};
    check_operator(ctx, big, 0, QP_FMT_HRB, "banded lattice 2^18+77, HRB");
    LARGE_REQUIRE("banded HRB", g_last.format == QP_FMT_HRB && g_last.walk && g_last.walk2 && g_last.nblocks >= 4096 && g_last.stored >= (1 << 20) && g_last.lstored >= (1 << 20));
    InputForm one_based;
    one_based.index_base = 1;
    check_operator(ctx, big, 0, QP_FMT_RBCSR, "banded lattice 2^18+77, RBCSR, index base 1", one_based);
    LARGE_REQUIRE("banded RBCSR", g_last.format == QP_FMT_RBCSR && g_last.nblocks >= 4096);
    check_operator(ctx, big, 0, QP_FMT_AUTO, "banded lattice 2^18+77, AUTO");
    LARGE_REQUIRE("banded AUTO", g_last.format == QP_FMT_HRB && g_last.walk && g_last.walk2);
  }
  if (wanted("grid")) {   // five-point open grid: lattice completion; all real, passed as QP_VAL_F64
    const std::vector<Csr> t{open_grid(512, 520)};
    InputForm f64;
    f64.f64 = true;
    REQUIRE((int64_t)t[0].col.size() >= (1 << 20), "open grid: %zu entries", t[0].col.size());
    check_operator(ctx, t, 0, QP_FMT_AUTO, "open 512 x 520 grid, QP_VAL_F64", f64);
    LARGE_REQUIRE("open grid", g_last.n_lattice_fill > 0 && g_last.walk && g_last.planes_real);
  }
  if (wanted("mirror")) {   // random columns, Hermitian: the column-blocked mirror (forced: it is chosen from 2^20 columns on), >= 512 tiles
    qp_ctx* c = fresh_ctx({{"colblock", 2}, {"cb_log2w", 12}});
    const std::vector<Csr> t{lcg_hermitian(13, (int64_t)1 << 17, 2)};
    check_operator(c, t, 0, QP_FMT_AUTO, "random columns 2^17, Hermitian, mirror");
    LARGE_REQUIRE("mirror", g_last.cb && g_last.cb_tiles >= 512);
    qp_ctx_destroy(c);
  }
  if (wanted("tall")) {   // few-valued, tall, rows passed unsorted and with repeated columns: the per-thread sort, the value dictionary
    const std::vector<Csr> t{lcg_csr(21, ((int64_t)1 << 16) + 129, 30011, 6, 8)}, raw{scrambled(t[0])};
    InputForm in;
    in.raw = &raw;
    check_operator(ctx, t, 0, QP_FMT_AUTO, "few-valued tall 65665 x 30011, unsorted and repeated columns", in);
    LARGE_REQUIRE("tall", g_last.cv && g_last.format == QP_FMT_RBCSR);
  }
  if (wanted("tfim")) {
    const std::vector<Csr> t{tfim(18)};
    check_operator(ctx, t, 0, QP_FMT_AUTO, "tfim(18)");
    LARGE_REQUIRE("tfim(18)", g_last.cv && g_last.planes_real);
  }
  if (wanted("terms")) {   // drift + a sparse control term; the complex coefficient of check_operator's third set_coeffs re-lays the packed operator out
    const std::vector<Csr> t{with_arith_values(const_lattice(N16, headline), true), sparse_pairs(N16, 16)};
    check_operator(ctx, t, 1, QP_FMT_AUTO, "banded lattice 2^16+192 + sparse control term");
    LARGE_REQUIRE("two terms", g_last.sparse_from == 1 && g_last.relayouts >= 1);
  }
  if (wanted("dense")) {   // a tall dense operator: the completion of the pattern on the host threads
    const std::vector<Csr> t{lcg_csr(22, ((int64_t)1 << 16) + 5, 3, 1, 3)};
    check_operator(ctx, t, 0, QP_FMT_DENSE, "dense 65541 x 3");
    LARGE_REQUIRE("dense", g_last.format == QP_FMT_DENSE && g_last.n_lattice_fill > 0);
  }
#undef LARGE_REQUIRE
  if (wanted("errors")) check_errors_at_size(ctx);
  if (wanted("throws")) check_throwing_workers();
  if (wanted("oom")) check_worker_out_of_memory(ctx);
  qp_ctx_destroy(ctx);
  for (const auto& s : g_sites) std::printf("threaded site %s:%d\n", s.first.c_str(), s.second);
  std::printf("large run clean: %lld operators on %u host threads, %zu call sites of parallel_rows started threads\n", (long long)n_cases, host_threads(), g_sites.size());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  g_digest = argc > 1 && std::strcmp(argv[1], "--digest") == 0;
  if (argc > 1 && std::strcmp(argv[1], "--print-plan-cases") == 0) {   // the rows of tests/operator_plan_cases.h
    check_shape_table(true);
    check_plan_table(true);
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "--large") == 0) return run_large(argc > 2 ? argv[2] : nullptr);
  qp_ctx* ctx = nullptr;
  if (qp_ctx_create(0, nullptr, &ctx) != QP_OK) {
    std::fprintf(stderr, "qp_ctx_create: %s\n", qp::g_last_error.c_str());
    return 2;
  }
  std::mt19937_64 rng(20261004);
  const int formats[] = {QP_FMT_AUTO, QP_FMT_RBCSR, QP_FMT_HRB, QP_FMT_CSR};
  // the shapes that have bitten, first
  const std::pair<int64_t, int64_t> shapes[] = {{5681, 358}, {358, 5681}, {1, 1}, {1, 70}, {70, 1}, {5, 5}, {63, 63}, {64, 64}, {65, 65},
                                                {127, 300}, {300, 127}, {1000, 1000}, {4097, 4097}, {200, 9000}};
  for (auto sh : shapes)
    for (int fmt : formats)
      for (int nvals : {2, 100000})
        for (int rep = 0; rep < 2; ++rep) {
          const bool herm = sh.first == sh.second && rep == 1;
          std::vector<Csr> terms{random_csr(rng, sh.first, sh.second, 11, nvals, herm)};
          char what[128];
          std::snprintf(what, sizeof what, "random %lld x %lld fmt %d nvals %d herm %d", (long long)sh.first, (long long)sh.second, fmt, nvals, (int)herm);
          check_operator(ctx, terms, 0, fmt, what);
        }
  // a row with a repeated column makes the stored count reach nrows x ncols although a position is missing -- the
  // duplicate is summed (Julia's sparse() semantics), the operator must not be taken for a complete dense one
  {
    Csr t;
    t.nrows = t.ncols = 3;
    t.rp = {0, 3, 6, 9};
    t.col = {0, 0, 1, 0, 1, 2, 0, 1, 2};
    for (int i = 0; i < 9; ++i) t.val.push_back(qp_c128{1.0 + i, 0.5});
    for (int fmt : {QP_FMT_AUTO, QP_FMT_DENSE, QP_FMT_RBCSR, QP_FMT_CSR}) {
      qp_matrix* m = nullptr;
      std::vector<int64_t> idx(t.col.begin(), t.col.end());
      REQUIRE(qp_matrix_create(ctx, 3, 3, 9, t.rp.data(), idx.data(), t.val.data(), QP_VAL_C128, QP_LAYOUT_CSR, 0, QP_FMT_AUTO, &m) == QP_OK, "dup: matrix");
      qp_operator* op = nullptr;
      REQUIRE(qp_operator_create(ctx, &m, 1, 0, fmt, &op) == QP_OK, "dup: operator (format %d): %s", fmt, qp::g_last_error.c_str());
      if (g_digest) print_digest(op, "dup");
      const int64_t nnz = op->A.nnz;
      std::vector<int64_t> rp(4);
      std::vector<int32_t> col((size_t)nnz);
      std::vector<qp_c128> val((size_t)nnz);
      REQUIRE(qp_operator_get_csr(op, rp.data(), col.data(), val.data()) == QP_OK, "dup: get_csr");
      // row 0: columns 0 (1 + 2 = 3, 0.5 + 0.5) and 1; a dense layout adds the explicit zero at (0, 2)
      REQUIRE(col[0] == 0 && val[0].re == 3.0 && val[0].im == 1.0 && col[1] == 1 && val[1].re == 3.0, "dup: row 0 is (%d: %g), (%d: %g)", col[0], val[0].re, col[1], val[1].re);
      if (op->A.format == QP_FMT_DENSE) REQUIRE(nnz == 9 && col[2] == 2 && val[2].re == 0.0 && val[2].im == 0.0, "dup: the missing position must be an explicit zero");
      else REQUIRE(nnz == 8, "dup: nnz %lld", (long long)nnz);
      qp_operator_destroy(op);
      qp_matrix_destroy(m);
      ++n_cases;
    }
  }
  // several terms with coefficients (lazy sum, sparse control terms, table recombination)
  for (int rep = 0; rep < 12; ++rep) {
    const int64_t n = 50 + (int64_t)(rng() % 3000);
    const int nt = 2 + (int)(rng() % 2);
    std::vector<Csr> terms;
    for (int t = 0; t < nt; ++t) terms.push_back(random_csr(rng, n, n, t == 0 ? 9 : 2, rep % 2 ? 3 : 100000, rep % 3 == 0));
    check_operator(ctx, terms, 1 + (int)(rng() % (uint64_t)(nt - 1 + 1)) % nt, formats[rep % 4], "several terms");
  }
  // lattices (strip-walk plans, lattice completion with open ends), sizes that walk (>= 3072 blocks needs N >= 196608: use the knob)
  qp_ctx_tuning_set(ctx, "walk_min_blocks", 8);
  const std::vector<std::vector<int64_t>> stencils = {{1, 2, 3, 4, 64, 128, 192, 256}, {1, 64}, {1, 2, 100, 200}, {1, 63, 64, 65}, {1, 32, 1024}, {1, 2, 16, 32, 512, 1024},
                                                      {3, 17}, {1, 2, 3, 4, 5}, {20, 40}};
  for (const auto& st : stencils)
    for (int64_t N : {(int64_t)4096, (int64_t)5000, (int64_t)16384 + 77})
      for (int periodic = 0; periodic < 2; ++periodic)
        for (int constant = 0; constant < 2; ++constant) {
          std::vector<Csr> terms{lattice(rng, N, st, periodic != 0, constant != 0)};
          char what[128];
          std::snprintf(what, sizeof what, "lattice N %lld first distance %lld periodic %d constant %d", (long long)N, (long long)st[0], periodic, constant);
          check_operator(ctx, terms, 0, QP_FMT_AUTO, what);
          check_operator(ctx, terms, 0, QP_FMT_HRB, what);
        }
  // spin chains: block-map encoding + value dictionary; the column-blocked mirror forced on an irregular operator
  for (int n : {5, 7, 10, 13}) {
    std::vector<Csr> terms{tfim(n)};
    check_operator(ctx, terms, 0, QP_FMT_AUTO, "tfim");
    check_operator(ctx, terms, 0, QP_FMT_HRB, "tfim hrb");
  }
  qp_ctx_tuning_set(ctx, "colblock", 2);
  qp_ctx_tuning_set(ctx, "cb_log2w", 8);
  for (int rep = 0; rep < 6; ++rep) {
    const int64_t nr = 300 + (int64_t)(rng() % 4000), nc = rep % 2 ? nr : 100 + (int64_t)(rng() % 6000);
    std::vector<Csr> terms{random_csr(rng, nr, nc, 12, 100000, false)};
    check_operator(ctx, terms, 0, rep % 3 == 0 ? QP_FMT_CSR : QP_FMT_RBCSR, "forced column-blocked mirror");
  }
  check_cut_table();
  check_panel_plan_cases();
  check_shape_table(false);
  check_plan_table(false);
  std::printf("walk geometry: %lld cuts of %lld one-term and %lld two-term plans keep every strip step in exactly one segment\n", (long long)n_cuts,
              (long long)n_walked, (long long)n_walk2);
  qp_ctx_destroy(ctx);
  std::printf("sanitizer run clean: %lld operators (%lld Hermitian-packed, %lld with a strip-walk plan, %lld with a value dictionary, %lld with a "
              "column-blocked mirror, %lld dense)\n",
              (long long)n_cases, (long long)n_hrb, (long long)n_walked, (long long)n_coded, (long long)n_cb, (long long)n_dense);
  return 0;
}
