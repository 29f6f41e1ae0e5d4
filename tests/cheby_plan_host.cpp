// TEST INFRASTRUCTURE (tests/test_cabi_host.py::test_cheby_plan_host_under_sanitizers): the pure-host planning unit of cheby!
// (csrc/cheby_plan.cpp, with csrc/small_plan.cpp), compiled as ordinary C++ with g++ -fsanitize=address,undefined and checked
//   1. by construction: every step sequence of 2 .. 40 coefficients, replayed symbolically -- which v_k every vector holds, which
//      a_k v_k the accumulator holds -- with the semantics of one fused term (tests/cheby_term_ref.py: term_ref);
//   2. against the rows the commit before the unit existed produced (tests/cheby_plan_cases.h);
//   3. the split partition by construction on generated patterns, against brute-force restatements of its definitions
//      (tests/split_term_cases.py: partition);
//   4. the split partition against the parent's rows of the same table;
//   5. the small-system gate against its statement in tests/small_instances.py, and the verdict of check_normalization.
// `--print-cases` prints the rows of the table from this tree.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <string>

#include "cheby_plan.h"
#include "cheby_plan_inputs.h"
#include "cheby_plan_cases.h"

static std::string g_last_error;
namespace qp {
int fail(int status, const char* fmt, ...) {   // (the library's own: engine_core.hip)
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return status;
}
}  // namespace qp

#define REQUIRE(cond, ...)                                        \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                                   \
      std::printf("\n");                                          \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

// ---- a step as rows ------------------------------------------------------------------------------------------------------------------
static cpi::TermRow term_row(const ChebyTerm& t) {
  cpi::TermRow r{};
  if (t.m == 0) return r;
  r.x = (int)t.x; r.v0 = (int)t.v0; r.vout = (int)t.vout; r.acc_in = (int)t.acc_in; r.acc_out = (int)t.acc_out;
  r.a_prev = t.a_prev; r.a = t.a; r.c_scale = t.c_scale; r.apply_phase = t.apply_phase;
  r.skip = t.defer->skip ? 1 : 0;                 // (as the engine's set_defer hands them to the kernel)
  r.n_defer = t.defer->skip ? 0 : t.defer->n_defer;
  r.a_d1 = t.defer->a_d1; r.a_d2 = t.defer->a_d2;
  r.check = t.check ? 1 : 0;
  return r;
}
struct Proposal {
  int m;
  bool both_update;
};
struct Sequence {
  std::vector<cpi::SeqRow> rows;     // the launches issued, then the closing row with the result slot
  std::vector<Proposal> proposals;   // every pair next() proposed, refused ones included
};
// refuse_at: which proposal (1-based) the launcher refuses; 0: none
static Sequence run(const char* name, const std::vector<double>& a, bool defer, bool pairs, bool check, bool panel, int refuse_at) {
  Sequence S;
  ChebySequence seq(a.data(), (int)a.size(), defer, pairs, check, panel);
  ChebyLaunch L;
  while (seq.next(&L)) {
    if (L.pair) {
      S.proposals.push_back({L.m, !L.t[0].defer->skip && !L.t[1].defer->skip});
      if ((int)S.proposals.size() == refuse_at) {
        seq.refuse();
        continue;
      }
    }
    cpi::SeqRow r{};
    r.seq = name; r.m = L.m; r.pair = L.pair ? 1 : 0;
    r.t[0] = term_row(L.t[0]);
    if (L.pair) r.t[1] = term_row(L.t[1]);
    REQUIRE(L.t[0].m == L.m && (!L.pair || L.t[1].m == L.m + 1), "%s: term numbers", name);
    S.rows.push_back(r);
  }
  cpi::SeqRow end{};
  end.seq = name;
  end.t[0].x = (int)seq.result();
  S.rows.push_back(end);
  REQUIRE(!seq.next(&L), "%s: next() after the end", name);
  return S;
}
static bool same_term(const cpi::TermRow& p, const cpi::TermRow& q) {
  return p.x == q.x && p.v0 == q.v0 && p.vout == q.vout && p.acc_in == q.acc_in && p.acc_out == q.acc_out && p.a_prev == q.a_prev &&
         p.a == q.a && p.c_scale == q.c_scale && p.apply_phase == q.apply_phase && p.skip == q.skip && p.n_defer == q.n_defer &&
         p.a_d1 == q.a_d1 && p.a_d2 == q.a_d2 && p.check == q.check;
}

// ---- 1. rotation by construction ----------------------------------------------------------------------------------------------------
enum { NONE = 0, PSI = 1, SLOT_A = 2, SLOT_C = 3, SLOT_D = 4, ACC = 5 };
constexpr int JUNK = -1, IS_ACC = -2;   // what a slot holds: v_k (k >= 0), junk, or the accumulator
static int coeff_index(const std::vector<double>& a, double v) {
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i] == v) return (int)i;
  return -1;
}
static void replay(const char* what, const Sequence& S, const std::vector<double>& a, bool check, bool pairs_allowed, bool panel) {
  const int nterms = (int)a.size() - 1;
  int holds[6] = {JUNK, 0, JUNK, JUNK, JUNK, JUNK};
  std::multiset<std::pair<int, int>> acc;   // (coefficient index, vector index) summed so far
  int acc_slot = NONE;                      // where that sum is
  int next_m = 1, last_acc_out = NONE;
  auto apply = [&](const cpi::TermRow& t, int m) {
    REQUIRE(m == next_m, "%s: term %d issued, %d expected", what, m, next_m);
    ++next_m;
    REQUIRE(t.x != NONE && holds[t.x] == m - 1, "%s: term %d gathers slot %d holding %d", what, m, t.x, t.x ? holds[t.x] : -9);
    if (m == 1) REQUIRE(t.v0 == NONE, "%s: term 1 has a v0", what);
    else REQUIRE(t.v0 != NONE && holds[t.v0] == m - 2, "%s: term %d reads v0 from slot %d holding %d", what, m, t.v0, t.v0 ? holds[t.v0] : -9);
    REQUIRE(t.a == a[(size_t)m] && t.c_scale == (m == 1 ? 1.0 : 2.0), "%s: term %d scalars", what, m);
    REQUIRE(t.apply_phase == (m == nterms ? 1 : 0), "%s: term %d apply_phase", what, m);
    REQUIRE(t.check == ((check && m >= 2) ? 1 : 0), "%s: term %d check partials", what, m);
    REQUIRE((t.vout == NONE) == (m == nterms), "%s: term %d vout", what, m);
    const int kx = holds[t.x], k0 = t.v0 ? holds[t.v0] : JUNK;
    if (!t.skip) {   // r = (acc_in ? acc_in : a_prev (n_defer == 1 ? v0 : x)) + [a_d2 v0] + [a_d1 x] + a t -> acc_out
      REQUIRE(t.acc_out == ACC || t.acc_out == PSI, "%s: term %d acc_out %d", what, m, t.acc_out);
      if (t.acc_in != NONE) {
        REQUIRE(t.acc_in == acc_slot && holds[t.acc_in] == IS_ACC, "%s: term %d reads an accumulator that is not there", what, m);
      } else {
        REQUIRE(acc.empty(), "%s: term %d starts the accumulator anew and loses %zu terms", what, m, acc.size());
        REQUIRE(t.a_prev == a[0], "%s: term %d a_prev", what, m);
        acc.insert({0, t.n_defer == 1 ? k0 : kx});
      }
      REQUIRE(t.n_defer >= 0 && t.n_defer <= 2 && (t.n_defer == 0 || m >= 2), "%s: term %d n_defer", what, m);
      if (t.n_defer == 2) acc.insert({coeff_index(a, t.a_d2), k0});
      if (t.n_defer >= 1) acc.insert({coeff_index(a, t.a_d1), kx});
      acc.insert({m, m});
      if (acc_slot != NONE && acc_slot != t.acc_out) holds[acc_slot] = JUNK;   // (the sum moved: the old copy is stale)
      acc_slot = last_acc_out = t.acc_out;
    } else {
      REQUIRE(t.acc_in == NONE && t.acc_out == NONE, "%s: term %d skips the accumulator and names it", what, m);
    }
    if (t.vout != NONE) holds[t.vout] = m;
    if (!t.skip) holds[t.acc_out] = IS_ACC;
  };
  for (size_t i = 0; i + 1 < S.rows.size(); ++i) {
    const cpi::SeqRow& r = S.rows[i];
    // (what a launch gathers of the vectors that exist before it: x of its first term; a pair's second term gathers y, which the
    // launch itself produces -- y may be Psi's buffer, once nothing reads v_0 .. any more)
    const bool gathers_psi = r.t[0].x == PSI;
    if (!r.pair) {
      const cpi::TermRow& t = r.t[0];
      if (t.vout != NONE) REQUIRE(r.m == 1 ? t.vout == SLOT_A : t.vout == t.v0, "%s: term %d writes vout to slot %d", what, r.m, t.vout);
      if (gathers_psi) REQUIRE(t.vout != PSI && t.acc_out != PSI, "%s: term %d writes Psi's buffer while gathering it", what, r.m);
      apply(t, r.m);
    } else {
      const cpi::TermRow &t0 = r.t[0], &t1 = r.t[1];
      REQUIRE(t1.x == t0.vout && t1.v0 == t0.x, "%s: pair at %d: the second term's operands", what, r.m);
      for (int out : {t0.vout, t1.vout})
        if (out != NONE) REQUIRE(out != t0.x && out != t0.v0 && out != t1.v0 && out != ACC, "%s: pair at %d writes slot %d that the launch reads", what, r.m, out);
      REQUIRE(t0.vout != t1.vout, "%s: pair at %d writes one slot twice", what, r.m);
      REQUIRE(t0.acc_out != PSI && t1.acc_out != PSI, "%s: pair at %d writes the accumulator to Psi's buffer", what, r.m);
      if (gathers_psi) REQUIRE(t0.vout != PSI && t1.vout != PSI, "%s: pair at %d writes Psi's buffer while gathering it", what, r.m);
      apply(t0, r.m);
      apply(t1, r.m + 1);
    }
  }
  REQUIRE(next_m == nterms + 1, "%s: %d terms of %d", what, next_m - 1, nterms);
  const int result = S.rows.back().t[0].x;
  REQUIRE(result == last_acc_out && holds[result] == IS_ACC, "%s: the result slot %d is not the last acc_out %d", what, result, last_acc_out);
  REQUIRE((int)acc.size() == nterms + 1, "%s: the accumulator holds %zu terms", what, acc.size());
  int k = 0;
  for (const auto& e : acc) {
    REQUIRE(e.first == k && e.second == k, "%s: the accumulator holds a_%d v_%d", what, e.first, e.second);
    ++k;
  }
  for (const Proposal& p : S.proposals)
    REQUIRE(p.m > 1 && p.m + 1 <= nterms && nterms >= 3 && !check && !panel && pairs_allowed && !p.both_update, "%s: a pair proposed at m = %d", what, p.m);
}
static long check_rotation() {
  long nseq = 0;
  for (int n = 2; n <= 40; ++n) {
    const std::vector<double> a = cpi::coeffs(n);
    const int nterms = n - 1;
    for (int defer = 0; defer <= 1; ++defer)
      for (int check = 0; check <= 1; ++check) {
        char what[96];
        std::snprintf(what, sizeof what, "n_coeffs %d defer %d check %d", n, defer, check);
        const Sequence off = run(what, a, defer, false, check, false, 0);
        replay(what, off, a, check, false, false);
        REQUIRE(off.proposals.empty() && (int)off.rows.size() == nterms + 1, "%s: pairs off", what);
        // the rule of the row-partitioned loop, restated: x = X[(m + 1) % 2], out = X0 iff m > 1 && last && m even
        for (int m = 1; m <= nterms; ++m) {
          const cpi::TermRow& t = off.rows[(size_t)m - 1].t[0];
          const bool last = m == nterms;
          const int xs = (m % 2) ? PSI : SLOT_A, os = (m % 2) ? SLOT_A : PSI;
          const int out = (m > 1 && last && m % 2 == 0) ? PSI : ACC;
          REQUIRE(t.x == xs && t.v0 == (m == 1 ? NONE : os) && t.vout == (last ? NONE : os), "%s: term %d against the sharded rule", what, m);
          REQUIRE(t.acc_out == (t.skip ? NONE : out), "%s: term %d acc_out against the sharded rule", what, m);
          if (last) REQUIRE(off.rows.back().t[0].x == (nterms == 1 ? ACC : out), "%s: result against the sharded rule", what);
        }
        ++nseq;
        // the panel step: never in pairs
        const Sequence pan = run(what, a, defer, true, check, true, 0);
        REQUIRE(pan.proposals.empty() && pan.rows.size() == off.rows.size(), "%s: a panel step in pairs", what);
        // pairs allowed: every proposal accepted, then refused at the 1st, 2nd, 3rd and at the last proposal
        const Sequence on = run(what, a, defer, true, check, false, 0);
        replay(what, on, a, check, true, false);
        ++nseq;
        const int np = (int)on.proposals.size();
        if (check || nterms < 3 || !defer) REQUIRE(np == 0, "%s: %d pairs proposed", what, np);
        if (!check && defer && nterms >= 4) REQUIRE(np >= 1, "%s: no pair proposed", what);
        for (int k : {1, 2, 3, np}) {
          if (k < 1 || k > np) continue;
          const Sequence ref = run(what, a, defer, true, check, false, k);
          replay(what, ref, a, check, true, false);
          REQUIRE((int)ref.proposals.size() == k, "%s: a pair proposed after the refusal of proposal %d", what, k);
          // up to the refused proposal the accepted sequence, afterwards one term per launch
          size_t i = 0;
          for (; i < ref.rows.size() && ref.rows[i].m != 0 && ref.rows[i].m < ref.proposals.back().m; ++i)
            REQUIRE(ref.rows[i].pair == on.rows[i].pair && same_term(ref.rows[i].t[0], on.rows[i].t[0]), "%s: refusal %d changes launch %zu before it", what, k, i);
          for (; i + 1 < ref.rows.size(); ++i) REQUIRE(!ref.rows[i].pair, "%s: a pair after refusal %d", what, k);
          ++nseq;
        }
      }
  }
  return nseq;
}

// ---- 2. rotation against the parent -----------------------------------------------------------------------------------------------
static std::vector<cpi::SeqRow> table_sequences(std::vector<std::string>& names) {
  std::vector<cpi::SeqRow> rows;
  const std::vector<cpi::SeqCase> cases = cpi::seq_cases();
  names.reserve(cases.size());
  for (const cpi::SeqCase& c : cases) {
    names.push_back(c.name);
    const Sequence S = run(names.back().c_str(), cpi::coeffs(c.n_coeffs), c.defer != 0, c.pairs != 0, c.check != 0, false, c.pairs == 2 ? 1 : 0);
    rows.insert(rows.end(), S.rows.begin(), S.rows.end());
  }
  return rows;
}
static long check_sequence_table() {
  std::vector<std::string> names;
  const std::vector<cpi::SeqRow> rows = table_sequences(names);
  const size_t nt = sizeof(kSeqRows) / sizeof(kSeqRows[0]);
  REQUIRE(rows.size() == nt, "%zu launch rows, the table has %zu", rows.size(), nt);
  for (size_t i = 0; i < nt; ++i) {
    const cpi::SeqRow &g = rows[i], &w = kSeqRows[i];
    REQUIRE(std::strcmp(g.seq, w.seq) == 0 && g.m == w.m && g.pair == w.pair && same_term(g.t[0], w.t[0]) && same_term(g.t[1], w.t[1]),
            "row %zu (%s, m = %d) differs from the table's (%s, m = %d)", i, g.seq, g.m, w.seq, w.m);
  }
  return (long)names.size();
}

// ---- 3. split by construction -----------------------------------------------------------------------------------------------------
static SplitWalk split_walk(const cpi::WalkScalars& w) { return SplitWalk{w.valid, w.K, w.fd, w.g, w.glong, w.W0, w.R1}; }
static void check_split(const char* what, const cpi::Pattern& P, const std::vector<int64_t>& send, const SplitWalk& W, long* nwalks) {
  const int rows_per_wg = 4;
  SplitPlan S;
  REQUIRE(plan_split(P.nrows, P.rowptr.data(), P.col.data(), send.data(), (int64_t)send.size(), rows_per_wg, W, &S) == QP_OK, "%s: %s", what, g_last_error.c_str());
  const int64_t n = P.nrows, nb = (n + 63) / 64;
  // the definitions, by brute force
  std::vector<char> is_b((size_t)nb, 0), adj((size_t)nb, 0);
  std::vector<int64_t> slot((size_t)n, -1);
  for (size_t i = 0; i < send.size(); ++i) {
    slot[(size_t)send[i]] = (int64_t)i;
    is_b[(size_t)(send[i] / 64)] = 1;
  }
  for (int64_t r = 0; r < n; ++r)
    for (int64_t p = P.rowptr[(size_t)r]; p < P.rowptr[(size_t)r + 1]; ++p)
      if (P.col[(size_t)p] >= n) is_b[(size_t)(r / 64)] = 1;
  for (int64_t r = 0; r < n; ++r)
    for (int64_t p = P.rowptr[(size_t)r]; p < P.rowptr[(size_t)r + 1]; ++p) {
      const int64_t c = P.col[(size_t)p];
      if (c >= n) continue;
      if (is_b[(size_t)(r / 64)] && !is_b[(size_t)(c / 64)]) adj[(size_t)(c / 64)] = 1;   // a boundary row gathers from the block
      if (!is_b[(size_t)(r / 64)] && is_b[(size_t)(c / 64)]) adj[(size_t)(r / 64)] = 1;   // a row of the block gathers from a boundary row
    }
  std::vector<int32_t> bb, plain, adjacent;
  for (int64_t b = 0; b < nb; ++b) (is_b[(size_t)b] ? bb : adj[(size_t)b] ? adjacent : plain).push_back((int32_t)b);
  REQUIRE(S.boundary == bb, "%s: boundary blocks", what);
  REQUIRE(S.n_plain == (int64_t)plain.size() && S.interior.size() == plain.size() + adjacent.size(), "%s: interior counts", what);
  REQUIRE(std::equal(plain.begin(), plain.end(), S.interior.begin()) && std::equal(adjacent.begin(), adjacent.end(), S.interior.begin() + (long)plain.size()),
          "%s: interior order (plain ascending, then adjacent ascending)", what);
  std::vector<char> seen((size_t)nb, 0);
  for (int32_t b : S.boundary) seen[(size_t)b]++;
  for (int32_t b : S.interior) seen[(size_t)b]++;
  for (int64_t b = 0; b < nb; ++b) REQUIRE(seen[(size_t)b] == 1, "%s: block %lld listed %d times", what, (long long)b, (int)seen[(size_t)b]);
  REQUIRE(S.mirror.size() == 64 * bb.size() + 1 && S.mirror.back() == -1, "%s: mirror size", what);
  for (size_t k = 0; k < bb.size(); ++k)
    for (int l = 0; l < 64; ++l) {
      const int64_t r = 64 * (int64_t)bb[k] + l;
      REQUIRE(S.mirror[64 * k + (size_t)l] == (r < n ? (int32_t)slot[(size_t)r] : -1), "%s: mirror of row %lld", what, (long long)r);
    }
  const unsigned wait_from = (unsigned)(plain.size() / rows_per_wg), total = (unsigned)((S.interior.size() + rows_per_wg - 1) / rows_per_wg);
  REQUIRE(S.wait_from_wg == wait_from && S.n_waiting_wg == (total > wait_from ? total - wait_from : 0u), "%s: waiting workgroups", what);
  if (!W.valid) REQUIRE(!S.walk, "%s: a walk without a plan", what);
  if (!S.walk) {
    REQUIRE(S.edge.empty() && S.W0 == 0 && S.R1 == 0, "%s: walk fields without a walk", what);
    return;
  }
  ++*nwalks;
  const int64_t reach = (std::max<int64_t>((int64_t)W.K * W.g + W.fd, W.glong) + 63) / 64 + 1;
  REQUIRE(S.R1 - S.W0 >= 8 && S.W0 >= W.W0 && S.R1 <= W.R1, "%s: window [%lld, %lld)", what, (long long)S.W0, (long long)S.R1);
  for (int64_t b = S.W0; b < S.R1; ++b) {
    REQUIRE(!is_b[(size_t)b] && !adj[(size_t)b], "%s: walked block %lld is boundary or adjacent", what, (long long)b);
    for (int32_t x : bb) REQUIRE(std::llabs((long long)(b - x)) >= reach, "%s: walked block %lld within reach of boundary block %d", what, (long long)b, x);
  }
  std::vector<int32_t> edge;
  for (int32_t b : S.interior)
    if (b < S.W0 || b >= S.R1) edge.push_back(b);
  REQUIRE(S.edge == edge, "%s: edge list", what);
}
static void check_splits(long* nsplits, long* nwalks) {
  const SplitWalk none;
  for (int64_t n : {1, 63, 64, 65, 200, 2048, 5000})
    for (int kind = 0; kind < 2; ++kind)
      for (int ghosts : {0, 37}) {
        const cpi::Pattern P = kind ? cpi::ragged(n, ghosts, (uint64_t)(100 + n)) : cpi::banded(n, n >= 2048 ? 70 : 3, ghosts, (uint64_t)(200 + n));
        for (const char* const* s = cpi::send_set_names(); *s; ++s) {
          char what[96];
          std::snprintf(what, sizeof what, "%s %lld rows, %d ghosts, send set %s", kind ? "ragged" : "banded", (long long)n, ghosts, *s);
          check_split(what, P, cpi::send_set(*s, n), none, nwalks);
          ++*nsplits;
        }
      }
  struct Lat { int nn, K; int64_t g, glong; int fd; };
  for (int64_t n : {2048, 4096})
    for (const Lat& l : {Lat{1, 1, 64, 0, 0}, Lat{2, 2, 128, 0, 0}, Lat{1, 1, 100, 700, 1}, Lat{4, 4, 64, 0, 0}})
      for (int ghosts : {0, 37}) {
        const cpi::Pattern P = cpi::lattice(n, l.nn, l.K, l.g, l.glong, l.fd, ghosts, (uint64_t)(300 + n));
        const int64_t S = (l.g + 63) / 64;
        for (int trim = 0; trim <= 2; trim += 2) {   // the operator's own run: all blocks past the first K S, or two fewer at the end
          const SplitWalk W{1, l.K, l.fd, l.g, l.glong, l.K * S, n / 64 - trim};
          for (const char* const* s = cpi::send_set_names(); *s; ++s) {
            char what[128];
            std::snprintf(what, sizeof what, "lattice %lld rows K %d g %lld glong %lld fd %d, %d ghosts, send set %s", (long long)n, l.K, (long long)l.g, (long long)l.glong, l.fd, ghosts, *s);
            check_split(what, P, cpi::send_set(*s, n), W, nwalks);
            ++*nsplits;
          }
        }
      }
  // the two refusals, and that nothing was read past them
  const cpi::Pattern P = cpi::banded(200, 3, 9, 1);
  SplitPlan S;
  const int64_t beyond[] = {3, 200}, below[] = {-1}, twice[] = {5, 9, 5};
  REQUIRE(plan_split(200, P.rowptr.data(), P.col.data(), beyond, 2, 4, none, &S) == QP_E_BAD_ARG && g_last_error == "send row 200 out of range", "%s", g_last_error.c_str());
  REQUIRE(plan_split(200, P.rowptr.data(), P.col.data(), below, 1, 4, none, &S) == QP_E_BAD_ARG && g_last_error == "send row -1 out of range", "%s", g_last_error.c_str());
  REQUIRE(plan_split(200, P.rowptr.data(), P.col.data(), twice, 3, 4, none, &S) == QP_E_BAD_ARG && g_last_error == "send row 5 listed twice", "%s", g_last_error.c_str());
}

// ---- 4. split against the parent ----------------------------------------------------------------------------------------------------
static cpi::SplitRow split_row(const cpi::SplitInput& in) {
  SplitPlan S;
  REQUIRE(plan_split(in.P.nrows, in.P.rowptr.data(), in.P.col.data(), in.send.data(), (int64_t)in.send.size(), 4, split_walk(in.walk), &S) == QP_OK, "%s", in.name);
  cpi::SplitRow r{};
  r.name = in.name; r.n_boundary = (long long)S.boundary.size(); r.n_interior = (long long)S.interior.size();
  r.wait_from_wg = S.wait_from_wg; r.n_waiting_wg = S.n_waiting_wg;
  r.walk = S.walk ? 1 : 0; r.W0 = S.W0; r.R1 = S.R1; r.n_edge = (long long)S.edge.size();
  r.h_boundary = cpi::fnv(S.boundary); r.h_interior = cpi::fnv(S.interior); r.h_mirror = cpi::fnv(S.mirror); r.h_edge = cpi::fnv(S.edge);
  return r;
}
static long check_split_table() {
  const std::vector<cpi::SplitInput> in = cpi::split_inputs();
  const size_t nt = sizeof(kSplitRows) / sizeof(kSplitRows[0]);
  REQUIRE(in.size() == nt, "%zu split inputs, the table has %zu", in.size(), nt);
  for (size_t i = 0; i < nt; ++i) {
    const cpi::SplitRow g = split_row(in[i]), &w = kSplitRows[i];
    REQUIRE(std::strcmp(g.name, w.name) == 0 && g.n_boundary == w.n_boundary && g.n_interior == w.n_interior && g.wait_from_wg == w.wait_from_wg &&
                g.n_waiting_wg == w.n_waiting_wg && g.walk == w.walk && g.W0 == w.W0 && g.R1 == w.R1 && g.n_edge == w.n_edge &&
                g.h_boundary == w.h_boundary && g.h_interior == w.h_interior && g.h_mirror == w.h_mirror && g.h_edge == w.h_edge,
            "split row %zu (%s) differs from the table's", i, g.name);
  }
  return (long)nt;
}

// ---- 5. small gate and verdict --------------------------------------------------------------------------------------------------------
static long check_gate_and_verdict() {
  long n_gate = 0;
  const int small_nnz = 8192;   // tests/small_instances.py: SMALL_NNZ
  for (int knob : {0, small_nnz})
    for (int64_t nnz : {(int64_t)1, (int64_t)small_nnz, (int64_t)small_nnz + 1, (int64_t)2 * small_nnz, (int64_t)2 * small_nnz + 1})
      for (int nops : {1, 64, 65})
        for (int64_t n : {(int64_t)1, (int64_t)513, (int64_t)600, (int64_t)601, (int64_t)1025, (int64_t)2048, (int64_t)2049})
          for (int64_t maxrow : {(int64_t)1, (int64_t)3, (int64_t)5, (int64_t)9, (int64_t)17, (int64_t)65}) {
            // tests/small_instances.py: cheby_plan
            qp::SmallPlan want, got;
            bool taken = knob > 0 && nnz <= 2 * (int64_t)knob && nops <= 64;
            if (taken) {
              bool ok = nnz <= knob && qp::small_plan(n, maxrow, &want, 16);
              if (!ok && n <= 600) ok = qp::small_plan(n, maxrow, &want, 32);
              taken = ok;
            }
            const bool g = cheby_small_gate(nnz, nops, n, maxrow, knob, &got);
            REQUIRE(g == taken, "gate(nnz %lld nops %d n %lld maxrow %lld knob %d)", (long long)nnz, nops, (long long)n, (long long)maxrow, knob);
            REQUIRE(cheby_small_candidate(nnz, nops, knob) || !g, "gate without candidate");
            if (g) REQUIRE(got.lanes == want.lanes && got.ent == want.ent && got.rows_per_group == want.rows_per_group, "gate plan");
            ++n_gate;
          }
  qp::SmallPlan p;
  // nine entries per row need the 32-slot form, which 600 rows get and 601 do not; more than small_nnz entries need it too
  REQUIRE(!qp::small_plan(600, 9, &p, 16) && cheby_small_gate(5400, 1, 600, 9, small_nnz, &p) && p.ent * p.rows_per_group > 16, "600 rows");
  REQUIRE(!cheby_small_gate(5409, 1, 601, 9, small_nnz, &p), "601 rows");
  REQUIRE(cheby_small_gate(small_nnz, 64, 513, 3, small_nnz, &p) && !cheby_small_gate(small_nnz, 65, 513, 3, small_nnz, &p), "nops 64 / 65");
  REQUIRE(cheby_small_gate(2 * small_nnz, 1, 513, 3, small_nnz, &p) && !cheby_small_gate(2 * small_nnz + 1, 1, 513, 3, small_nnz, &p), "2 small_nnz");
  REQUIRE(!cheby_small_gate(small_nnz + 1, 1, 1025, 3, small_nnz, &p) && cheby_small_gate(small_nnz, 1, 1025, 3, small_nnz, &p), "small_nnz beyond 600 rows");
  // verdict: triples {Re, Im, |v1|^2} of terms 1 .. nterms; map norm = hypot(Re, Im) / (2 |v1|^2); term 1 is never looked at
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const int nterms = 6;
  const double limit = 1e-3;
  std::vector<double> t((size_t)3 * nterms);
  auto fill = [&] {
    for (int m = 1; m <= nterms; ++m) { t[3 * (size_t)(m - 1)] = 0.6; t[3 * (size_t)(m - 1) + 1] = 0.8; t[3 * (size_t)(m - 1) + 2] = 0.5; }   // map norm exactly 1
  };
  fill();
  REQUIRE(cheby_normalization_verdict(t.data(), nterms, limit) == 0, "verdict: all within");
  t[0] = 100.0;   // term 1: not checked
  REQUIRE(cheby_normalization_verdict(t.data(), nterms, limit) == 0, "verdict: term 1");
  for (int m = 2; m <= nterms; ++m) {
    fill();
    t[3 * (size_t)(m - 1) + 2] = 0.5 / (1.0 + 2 * limit);   // map norm 1 + 2 limit
    t[3 * (size_t)(nterms - 1)] = nan;                     // (a later bad term does not hide the first)
    REQUIRE(cheby_normalization_verdict(t.data(), nterms, limit) == m + 1, "verdict: term %d", m);
    fill();
    t[3 * (size_t)(m - 1) + 2] = 0.5 / (1.0 + 0.5 * limit);
    REQUIRE(cheby_normalization_verdict(t.data(), nterms, limit) == 0, "verdict: within the limit at term %d", m);
    for (int which = 0; which < 3; ++which) {
      fill();
      t[3 * (size_t)(m - 1) + (size_t)which] = nan;
      REQUIRE(cheby_normalization_verdict(t.data(), nterms, limit) == m + 1, "verdict: NaN at term %d", m);
    }
    fill();
    t[3 * (size_t)(m - 1) + 2] = 0.0;   // |v1| = 0: infinite map norm
    REQUIRE(cheby_normalization_verdict(t.data(), nterms, limit) == m + 1, "verdict: zero vector at term %d", m);
  }
  REQUIRE(cheby_normalization_verdict(t.data(), 1, limit) == 0, "verdict: one term");
  // dt against the workspace's, and the scalars
  REQUIRE(cheby_dt_matches(0.5, -0.5) && cheby_dt_matches(-0.5, 0.5 * (1 + 1e-9)) && !cheby_dt_matches(0.5, 0.5 * (1 + 1e-7)), "cheby_dt_matches");
  const ChebyScalars f(2.0, -1.0, 1.0), b(2.0, -1.0, -1.0);
  REQUIRE(f.beta == 0.0 && f.c == qp::cplx(0, -1) && b.c == qp::cplx(0, 1) && f.phase == qp::cplx(1, 0), "ChebyScalars");
  return n_gate;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--print-cases") == 0) {
    std::vector<std::string> names;
    std::printf("static const cpi::SeqRow kSeqRows[] = {\n");
    for (const cpi::SeqRow& r : table_sequences(names)) cpi::print_seq_row(r);
    std::printf("};\nstatic const cpi::SplitRow kSplitRows[] = {\n");
    for (const cpi::SplitInput& in : cpi::split_inputs()) cpi::print_split_row(split_row(in));
    std::printf("};\n");
    return 0;
  }
  const long nseq = check_rotation();
  std::printf("rotation: %ld sequences of 2 .. 40 coefficients replayed term by term\n", nseq);
  const long named = check_sequence_table();
  std::printf("rotation: %ld named sequences (%zu launch rows) match the table\n", named, sizeof(kSeqRows) / sizeof(kSeqRows[0]));
  long nsplits = 0, nwalks = 0;
  check_splits(&nsplits, &nwalks);
  std::printf("split: %ld partitions match their definitions, %ld of them with a walk window; 3 refusals in the library's words\n", nsplits, nwalks);
  std::printf("split: %ld named partitions match the table\n", check_split_table());
  std::printf("small gate: %ld argument sets match the statement; verdict and scalars checked\n", check_gate_and_verdict());
  std::printf("sanitizer run clean\n");
  return 0;
}
