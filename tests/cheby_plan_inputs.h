// Inputs of tests/cheby_plan_host.cpp that do not depend on the unit under test (csrc/cheby_plan.h): the coefficients of the named
// step sequences, the sparsity patterns and send sets of the split cases, and the hash of a list.  The program that printed the
// expected rows of tests/cheby_plan_cases.h from the commit before the unit existed included this header too, so both sides saw
// the same inputs.  No standard-library distribution: a linear congruential generator written out here.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace cpi {

struct Lcg {
  uint64_t s;
  explicit Lcg(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int64_t below(int64_t n) { return (int64_t)(next() % (uint64_t)n); }
};

// a_i of a step with n_coeffs coefficients: exactly representable, all different, alternating in sign
inline std::vector<double> coeffs(int n_coeffs) {
  std::vector<double> a((size_t)n_coeffs);
  for (int i = 0; i < n_coeffs; ++i) a[(size_t)i] = ((i % 2) ? -1.0 : 1.0) * (0.5 + 0.25 * i);
  return a;
}

inline uint64_t fnv(const int32_t* p, size_t n) {   // FNV-1a over the values, four bytes each, little end first
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i)
    for (int b = 0; b < 4; ++b) h = (h ^ (uint64_t)(((uint32_t)p[i] >> (8 * b)) & 255u)) * 1099511628211ull;
  return h;
}
inline uint64_t fnv(const std::vector<int32_t>& v) { return fnv(v.data(), v.size()); }

// ---- patterns: nrows local rows, columns ascending and unique per row; a column >= nrows is a ghost column -------------------
struct Pattern {
  int64_t nrows = 0;
  std::vector<int64_t> rowptr;
  std::vector<int32_t> col;
};
inline Pattern from_rows(int64_t nrows, std::vector<std::vector<int64_t>>& rows) {
  Pattern P;
  P.nrows = nrows;
  P.rowptr.push_back(0);
  for (auto& r : rows) {
    std::sort(r.begin(), r.end());
    r.erase(std::unique(r.begin(), r.end()), r.end());
    for (int64_t c : r) P.col.push_back((int32_t)c);
    P.rowptr.push_back((int64_t)P.col.size());
  }
  return P;
}
// `ghosts` > 0: every seventh row of the first and of the last 64 rows reads one or two of `ghosts` ghost columns
inline void add_ghosts(int64_t n, int ghosts, Lcg& g, std::vector<std::vector<int64_t>>& rows) {
  if (ghosts <= 0) return;
  for (int64_t r = 0; r < n; ++r)
    if ((r < 64 || r >= n - 64) && r % 7 == 0)
      for (int k = 0; k < 1 + (int)(r % 2); ++k) rows[(size_t)r].push_back(n + g.below(ghosts));
}
// band of half-width hw (clipped at the ends)
inline Pattern banded(int64_t n, int hw, int ghosts, uint64_t seed) {
  Lcg g(seed);
  std::vector<std::vector<int64_t>> rows((size_t)n);
  for (int64_t r = 0; r < n; ++r)
    for (int64_t c = std::max<int64_t>(0, r - hw); c <= std::min(n - 1, r + hw); ++c) rows[(size_t)r].push_back(c);
  add_ghosts(n, ghosts, g, rows);
  return from_rows(n, rows);
}
// rows of 0 .. 6 entries anywhere (every fifth row empty), symmetrised: what a boundary row reads also reads it
inline Pattern ragged(int64_t n, int ghosts, uint64_t seed) {
  Lcg g(seed);
  std::vector<std::vector<int64_t>> rows((size_t)n);
  for (int64_t r = 0; r < n; ++r) {
    if (r % 5 == 4) continue;
    const int len = (int)g.below(4);
    for (int k = 0; k < len; ++k) {
      const int64_t c = (g.below(3) == 0) ? g.below(n) : std::min(n - 1, std::max<int64_t>(0, r + g.below(41) - 20));
      if (c % 5 == 4) continue;
      rows[(size_t)r].push_back(c);
      rows[(size_t)c].push_back(r);
    }
  }
  add_ghosts(n, ghosts, g, rows);
  return from_rows(n, rows);
}
// periodic lattice: the diagonal, +-1 .. +-nn, +-g .. +-K g, +-glong (0: none), with the diagonal far neighbours m g +- 1 when fd
inline Pattern lattice(int64_t n, int nn, int K, int64_t gstep, int64_t glong, int fd, int ghosts, uint64_t seed) {
  Lcg g(seed);
  std::vector<int64_t> d = {0};
  for (int k = 1; k <= nn; ++k) d.push_back(k);
  for (int m = 1; m <= K; ++m)
    for (int e = -fd; e <= fd; ++e) d.push_back(m * gstep + e);
  if (glong) d.push_back(glong);
  std::vector<std::vector<int64_t>> rows((size_t)n);
  for (int64_t r = 0; r < n; ++r)
    for (int64_t x : d) {
      rows[(size_t)r].push_back(((r + x) % n + n) % n);
      rows[(size_t)r].push_back(((r - x) % n + n) % n);
    }
  add_ghosts(n, ghosts, g, rows);
  return from_rows(n, rows);
}

// ---- send sets: tests/split_term_cases.py restated --------------------------------------------------------------------------------
inline const char* const* send_set_names() {
  static const char* const names[] = {"none", "ends", "scattered", "last-row", "all", "one-interior", nullptr};
  return names;
}
inline std::vector<int64_t> send_set(const std::string& name, int64_t nrows) {
  std::vector<int64_t> s;
  const int64_t nblocks = (nrows + 63) / 64;
  if (name == "ends") {                 // the first and the last 40 rows (fewer than 80 rows: every row once)
    for (int64_t r = 0; r < std::min<int64_t>(40, nrows); ++r) s.push_back(r);
    for (int64_t r = std::max<int64_t>(nrows - 40, 40); r < nrows; ++r) s.push_back(r);
  } else if (name == "scattered") {     // row 7, then from the top down: lane 63 of every second block, lane 10 of blocks 4, 8, ..
    std::vector<int64_t> rows;
    for (int64_t k = 0; k < nblocks; k += 2)
      if (64 * k + 63 < nrows) rows.push_back(64 * k + 63);
    for (int64_t k = 4; k < nblocks; k += 4)
      if (64 * k + 10 < nrows) rows.push_back(64 * k + 10);
    std::sort(rows.begin(), rows.end());
    if (nrows > 7) s.push_back(7);
    for (size_t i = rows.size(); i-- > 0;) s.push_back(rows[i]);
  } else if (name == "last-row") {
    s.push_back(nrows - 1);
  } else if (name == "all") {           // every row, descending
    for (int64_t r = nrows - 1; r >= 0; --r) s.push_back(r);
  } else if (name == "one-interior") {  // lane 1 of every block but the middle one
    for (int64_t k = 0; k < nblocks; ++k)
      if (k != nblocks / 2 && 64 * k + 1 < nrows) s.push_back(64 * k + 1);
  }
  return s;
}

// ---- the named split inputs of the table -------------------------------------------------------------------------------------------
struct WalkScalars {   // of the operator's one-term walk plan; valid = 0: none
  int valid, K, fd;
  int64_t g, glong, W0, R1;
};
struct SplitInput {
  const char* name;
  Pattern P;
  std::vector<int64_t> send;
  WalkScalars walk;
};
inline std::vector<SplitInput> split_inputs() {
  std::vector<SplitInput> v;
  const WalkScalars none = {0, 0, 0, 0, 0, 0, 0};
  v.push_back({"banded-200-ghosts/scattered", banded(200, 3, 9, 1), send_set("scattered", 200), none});
  v.push_back({"banded-65/last-row", banded(65, 2, 0, 2), send_set("last-row", 65), none});
  v.push_back({"banded-2048-hw70/ends", banded(2048, 70, 0, 3), send_set("ends", 2048), none});
  v.push_back({"ragged-5000-ghosts/scattered", ragged(5000, 33, 4), send_set("scattered", 5000), none});
  v.push_back({"ragged-5000/one-interior", ragged(5000, 0, 5), send_set("one-interior", 5000), none});
  v.push_back({"ragged-2048-ghosts/none", ragged(2048, 12, 6), send_set("none", 2048), none});
  v.push_back({"ragged-63/all", ragged(63, 0, 7), send_set("all", 63), none});
  v.push_back({"lattice-2048-5point/ends", lattice(2048, 1, 1, 64, 0, 0, 0, 8), send_set("ends", 2048), {1, 1, 0, 64, 0, 1, 32}});
  v.push_back({"lattice-4096-5point-ghosts/ends", lattice(4096, 1, 1, 64, 0, 0, 40, 9), send_set("ends", 4096), {1, 1, 0, 64, 0, 1, 64}});
  v.push_back({"lattice-4096-K2-g128/ends", lattice(4096, 2, 2, 128, 0, 0, 0, 10), send_set("ends", 4096), {1, 2, 0, 128, 0, 4, 64}});
  v.push_back({"lattice-4096-g100-long700-fd/ends", lattice(4096, 1, 1, 100, 700, 1, 0, 11), send_set("ends", 4096), {1, 1, 1, 100, 700, 2, 62}});
  v.push_back({"lattice-4096-5point/scattered", lattice(4096, 1, 1, 64, 0, 0, 0, 12), send_set("scattered", 4096), {1, 1, 0, 64, 0, 1, 64}});
  v.push_back({"lattice-2048-K2-g128/last-row", lattice(2048, 1, 2, 128, 0, 0, 0, 13), send_set("last-row", 2048), {1, 2, 0, 128, 0, 4, 32}});
  return v;
}

// ---- the rows of tests/cheby_plan_cases.h ---------------------------------------------------------------------------------------------
// slots: 0 none, 1 Psi, 2 A, 3 C, 4 D, 5 Acc
struct TermRow {
  int x, v0, vout, acc_in, acc_out;
  double a_prev, a, c_scale;   // c_scale: the term's c over the step's first c
  int apply_phase, skip, n_defer;
  double a_d1, a_d2;
  int check;
};
struct SeqRow {   // one launch; m = 0 closes the sequence: t[0].x is the slot that holds the result
  const char* seq;
  int m, pair;
  TermRow t[2];
};
struct SplitRow {
  const char* name;
  long long n_boundary, n_interior;
  unsigned wait_from_wg, n_waiting_wg;
  int walk;
  long long W0, R1, n_edge;
  unsigned long long h_boundary, h_interior, h_mirror, h_edge;   // fnv of the four lists (h_edge of the empty list without a walk)
};
inline void print_term(const TermRow& t) {
  std::printf("{%d,%d,%d,%d,%d, %.17g,%.17g,%.17g, %d,%d,%d, %.17g,%.17g, %d}", t.x, t.v0, t.vout, t.acc_in, t.acc_out, t.a_prev, t.a,
              t.c_scale, t.apply_phase, t.skip, t.n_defer, t.a_d1, t.a_d2, t.check);
}
inline void print_seq_row(const SeqRow& r) {
  std::printf("  {\"%s\", %d, %d, {", r.seq, r.m, r.pair);
  print_term(r.t[0]);
  std::printf(", ");
  print_term(r.t[1]);
  std::printf("}},\n");
}
inline void print_split_row(const SplitRow& r) {
  std::printf("  {\"%s\", %lld, %lld, %uu, %uu, %d, %lld, %lld, %lld, 0x%016llxull, 0x%016llxull, 0x%016llxull, 0x%016llxull},\n", r.name,
              r.n_boundary, r.n_interior, r.wait_from_wg, r.n_waiting_wg, r.walk, r.W0, r.R1, r.n_edge, r.h_boundary, r.h_interior,
              r.h_mirror, r.h_edge);
}
// the named sequences: n_coeffs x deferred accumulator x pairs (0 off, 1 on, 2 on and refused at the first proposal), and
// check_normalization at n_coeffs = 5
struct SeqCase {
  std::string name;
  int n_coeffs, defer, pairs, check;
};
inline std::vector<SeqCase> seq_cases() {
  std::vector<SeqCase> v;
  static const char* const pn[] = {"off", "on", "refused1"};
  for (int n : {2, 3, 4, 5, 6, 7, 14, 26})
    for (int d : {1, 0})
      for (int p : {0, 1, 2}) v.push_back({"n" + std::to_string(n) + "-defer" + std::to_string(d) + "-pairs-" + pn[p], n, d, p, 0});
  for (int d : {1, 0})
    for (int p : {0, 1}) v.push_back({"n5-defer" + std::to_string(d) + "-pairs-" + pn[p] + "-check", 5, d, p, 1});
  return v;
}

}  // namespace cpi
