// Pure-host planning of cheby! (cheby_plan.h): accumulator schedule, the launches of a step, the split partition, small gates.
#include "cheby_plan.h"

#include <algorithm>
#include <cmath>

using qp::cplx;
using qp::kRB;

// terms whose epilogue updates the Psi accumulator: every third one counted from the last
// (the epilogue of term m holds v_{m-2}, v_{m-1}, v_m of the row).  The first update must
// still see Psi = v_0, which term 2 overwrites in place, so it is forced to term <= 2.
void acc_schedule(const double* a, int n_coeffs, bool defer, qp_acc_defer* out) {
  const int nterms = n_coeffs - 1;
  std::vector<char> upd((size_t)nterms + 1, defer ? 0 : 1);
  if (defer) {
    int m0 = nterms;
    for (; m0 >= 1; m0 -= 3) upd[m0] = 1;
    if (m0 + 3 == 3) upd[1] = 1;
  }
  int last_upd = 0;
  for (int m = 1; m <= nterms; ++m) {
    qp_acc_defer& d = out[m - 1];
    d = qp_acc_defer{0, 0, 0.0, 0.0};
    if (upd[m]) {
      d.n_defer = m - last_upd - 1;
      d.a_d1 = (d.n_defer >= 1) ? a[m - 1] : 0.0;
      d.a_d2 = (d.n_defer == 2) ? a[m - 2] : 0.0;
      last_upd = m;
    } else {
      d.skip = 1;
    }
  }
}

bool cheby_dt_matches(double dt, double wrk_dt) {
  const double x = std::fabs(dt), y = std::fabs(wrk_dt);
  return std::fabs(x - y) <= 1.4901161193847656e-08 * std::max(x, y);
}

ChebyScalars::ChebyScalars(double Delta, double E_min, double dt)
    : beta((Delta / 2) + E_min),
      c((dt > 0) ? cplx(0, -2.0) / Delta : cplx(0, 2.0) / Delta),
      phase(std::exp(cplx(0, -1) * beta * dt)) {}

// ---- the launches of one step (src/cheby.jl:171-211) ----------------------------------------------------------------------
ChebySequence::ChebySequence(const double* a, int n_coeffs, bool defer, bool pairs_allowed, bool check_normalization, bool panel)
    : a_(a), nterms_(n_coeffs - 1), check_(check_normalization), sched_((size_t)n_coeffs - 1) {
  acc_schedule(a, n_coeffs, defer, sched_.data());
  st_.pairs = pairs_allowed && pairs_possible(n_coeffs, check_normalization, panel);
}

// term m is issued next: what it finds in the accumulator and what it leaves there
ChebyTerm ChebySequence::term(int m, ChebySlot x, ChebySlot v0, ChebySlot vout, ChebySlot acc_out) {
  const qp_acc_defer& d = sched_[(size_t)m - 1];
  const bool last = (m == nterms_), reads = st_.updated && !d.skip;
  const ChebyTerm t{m, x, v0, last ? ChebySlot::None : vout, reads ? ChebySlot::Acc : ChebySlot::None, d.skip ? ChebySlot::None : acc_out,
                    st_.updated ? 0.0 : a_[0], a_[m], (m == 1) ? 1.0 : 2.0, last ? 1 : 0, false, &d};
  st_.updated = st_.updated || !d.skip;
  return t;
}

bool ChebySequence::next(ChebyLaunch* L) {
  State& s = st_;
  const int m = s.m;
  if (m > nterms_) return false;
  L->m = m;
  L->pair = m > 1 && s.pairs && m + 1 <= nterms_ && !(sched_[(size_t)m - 1].skip == 0 && sched_[(size_t)m].skip == 0);
  if (L->pair) {
    // y = v_m -> spare[0], z = v_{m+1} -> spare[1]; afterwards the two vectors the pair read are the spare ones
    undo_ = s;
    L->t[0] = term(m, s.cur, s.prev, s.spare[0], ChebySlot::Acc);
    L->t[1] = term(m + 1, s.spare[0], s.cur, s.spare[1], ChebySlot::Acc);
    s.result = ChebySlot::Acc;
    std::swap(s.prev, s.spare[1]);   // prev = z, cur = y; spare = the two vectors the pair read
    std::swap(s.cur, s.spare[0]);
    std::swap(s.cur, s.prev);
    s.m = m + 2;
    return true;
  }
  // m = 1: v0 = Psi; Psi = a1 v0; v1 = c (H v0 - beta v0); Psi += a2 v1     :171-182
  // m > 1: v2 = c (H v1 - beta v1) + v0 (`prev` holds v0, overwritten in place by v2); Psi += a_i v2; rotate            :186-207
  const bool last = (m == nterms_);
  s.result = (m > 1 && last && s.cur != ChebySlot::Psi && !s.pairs) ? ChebySlot::Psi : ChebySlot::Acc;
  L->t[0] = term(m, s.cur, s.prev, m == 1 ? ChebySlot::A : s.prev, s.result);
  L->t[0].check = check_ && m >= 2;
  if (m == 1) {
    s.prev = ChebySlot::Psi;
    s.cur = ChebySlot::A;
  } else {
    std::swap(s.cur, s.prev);   // prev's buffer now holds v_m: it is gathered next
  }
  s.m = m + 1;
  return true;
}

void ChebySequence::refuse() {
  st_ = undo_;
  st_.pairs = false;
}

// ---- boundary / interior split -----------------------------------------------------------------------------------------
int plan_split(int64_t nrows, const int64_t* ur, const int32_t* uc, const int64_t* send_rows, int64_t nsend, int rows_per_wg,
               const SplitWalk& P, SplitPlan* out) {
  const int64_t nblocks = (nrows + kRB - 1) / kRB;
  std::vector<char> is_boundary((size_t)nblocks, 0);
  std::vector<int32_t> slot_of_row((size_t)nrows, -1);
  for (int64_t i = 0; i < nsend; ++i) {
    const int64_t r = send_rows[i];
    if (r < 0 || r >= nrows) return qp::fail(QP_E_BAD_ARG, "send row %lld out of range", (long long)r);
    if (slot_of_row[r] >= 0) return qp::fail(QP_E_BAD_ARG, "send row %lld listed twice", (long long)r);
    slot_of_row[r] = (int32_t)i;
    is_boundary[r / kRB] = 1;
  }
  for (int64_t r = 0; r < nrows; ++r)   // rows that read a ghost column must wait for the exchange
    if (ur[r + 1] > ur[r] && uc[ur[r + 1] - 1] >= nrows) is_boundary[r / kRB] = 1;
  std::vector<char> adjacent((size_t)nblocks, 0);
  for (int64_t r = 0; r < nrows; ++r) {
    const bool rb = is_boundary[r / kRB];
    for (int64_t p = ur[r]; p < ur[r + 1]; ++p) {
      const int64_t c = uc[p];
      if (c >= nrows) continue;
      const bool cb = is_boundary[c / kRB];
      if (rb && !cb) adjacent[c / kRB] = 1;
      if (!rb && cb) adjacent[r / kRB] = 1;
    }
  }
  SplitPlan& S = *out;
  S = SplitPlan();
  std::vector<int32_t> adj;
  for (int64_t b = 0; b < nblocks; ++b) {
    if (is_boundary[b]) S.boundary.push_back((int32_t)b);
    else if (adjacent[b]) adj.push_back((int32_t)b);
    else S.interior.push_back((int32_t)b);
  }
  S.n_plain = (int64_t)S.interior.size();
  S.interior.insert(S.interior.end(), adj.begin(), adj.end());
  S.wait_from_wg = (unsigned)(S.n_plain / rows_per_wg);
  const unsigned total = (unsigned)((S.interior.size() + rows_per_wg - 1) / rows_per_wg);
  S.n_waiting_wg = total > S.wait_from_wg ? total - S.wait_from_wg : 0;
  S.mirror.assign(S.boundary.size() * kRB + 1, -1);
  for (size_t k = 0; k < S.boundary.size(); ++k)
    for (int l = 0; l < kRB; ++l) {
      const int64_t r = (int64_t)S.boundary[k] * kRB + l;
      if (r < nrows) S.mirror[k * kRB + l] = slot_of_row[r];
    }
  if (P.valid) {
    int64_t lo = 0, hi = nblocks;
    while (lo < nblocks && is_boundary[lo]) ++lo;
    while (hi > lo && is_boundary[hi - 1]) --hi;
    bool contiguous = true;
    for (int64_t b = lo; b < hi && contiguous; ++b) contiguous = !is_boundary[b];
    const int64_t reach = (std::max<int64_t>((int64_t)P.K * P.g + P.fd, P.glong) + kRB - 1) / kRB + 1;
    const int64_t w0 = std::max(P.W0, lo + reach), r1 = std::min(P.R1, hi - reach);
    if (contiguous && r1 - w0 >= 8) {
      S.walk = true;
      S.W0 = w0;
      S.R1 = r1;
      for (int32_t b : S.interior)
        if (b < w0 || b >= r1) S.edge.push_back(b);
    }
  }
  return QP_OK;
}

// ---- small gates and verdicts -------------------------------------------------------------------------------------------
bool cheby_small_gate(int64_t nnz, int nops, int64_t n, int64_t maxrow, int small_nnz, qp::SmallPlan* plan) {
  if (!cheby_small_candidate(nnz, nops, small_nnz)) return false;
  // 16 register slots per lane where that is enough; otherwise 32 (the upper 16 values of a lane
  // live in LDS: 128 KB, which leaves room for vectors of up to 600 rows)
  bool ok = nnz <= small_nnz && qp::small_plan(n, maxrow, plan, qp::kSmallEpt);
  if (!ok && n <= 600) ok = qp::small_plan(n, maxrow, plan, 2 * qp::kSmallEpt);
  return ok;
}

int cheby_normalization_verdict(const double* triples, int nterms, double limit) {
  for (int m = 2; m <= nterms; ++m) {
    const double* t = &triples[3 * (m - 1)];
    const double map_norm = std::hypot(t[0], t[1]) / (2 * t[2]);   // :195
    if (!(map_norm <= 1.0 + limit)) return m + 1;   // (coefficient a[m + 1] of the reference's 1-based list)
  }
  return 0;
}
