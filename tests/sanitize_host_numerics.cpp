// AddressSanitizer / UBSan harness for the library's host numerics (csrc/host_numerics.cpp): Bessel
// coefficients, Hessenberg eigenvalues of every leading block, Leja ordering, Newton divided
// differences, the Newton polynomial and next start vector of a restart, CSC -> CSR and row partitions, on random inputs; the
// restart algebra also on a diagonal matrix against its scalar recurrence and on the named inputs of
// tests/newton_restart_cases.h, both bit for bit.  Built and run by
// tests/test_cabi_host.py::test_host_numerics_under_sanitizers with g++ (CPU only; GPU sanitizers are
// not available on the test pool).
#include <cstdio>
#include <cstdlib>
#include <random>
#include "qprop_internal.h"
#include "newton_restart_cases.h"
using qp::cplx;

// one restart through the two host functions; returns the new beta
static double restart(const cplx* H, int ldh, int m, const cplx* a, const cplx* leja, double radius, double beta, const double* nu,
                      std::vector<cplx>& P, std::vector<cplx>& R, std::vector<cplx>& Rn) {
  qp::newton_restart_poly(H, ldh, m, a, leja, radius, beta, P, R, Rn);
  return qp::newton_restart_next(H, ldh, m, leja[m - 1], radius, nu, P, R, Rn);
}
static bool same(const std::vector<cplx>& x, const std::vector<cplx>& y, int n) {
  for (int i = 0; i < n; ++i)
    if (!(x[i].real() == y[i].real() && x[i].imag() == y[i].imag())) return false;
  return true;
}
// the restart's slice [n_s, n_s + m) of a / leja on a random Hessenberg matrix: with and without nu, and with a wider leading
// dimension, which must not change a bit
static int random_restart(const std::vector<cplx>& H, int m, const cplx* a, const cplx* leja, double radius, std::mt19937_64& rng) {
  std::vector<cplx> P, R, Rn, P2, R2, Rn2;
  std::vector<double> nu(m + 1);
  for (auto& v : nu) v = 1.0 + 1e-6 * (double)(rng() % 1000);
  nu[rng() % (m + 1)] = 0.0;
  const int ldw = m + 4;
  std::vector<cplx> Hw((size_t)ldw * ldw, cplx(7.0, -7.0));   // (what lies below row m must never be read into the result)
  for (int c = 0; c < m + 1; ++c)
    for (int r = 0; r < m + 1; ++r) Hw[(size_t)c * ldw + r] = H[(size_t)c * (m + 1) + r];
  for (const double* v : {(const double*)nullptr, (const double*)nu.data()}) {
    const double b = restart(H.data(), m + 1, m, a, leja, radius, 0.75, v, P, R, Rn);
    const double bw = restart(Hw.data(), ldw, m, a, leja, radius, 0.75, v, P2, R2, Rn2);
    if ((int)P.size() != m + 1 || (int)R.size() != m + 1) return 20;
    if (!(b == bw) || !same(P, P2, m) || !same(R, R2, m + 1)) return 21;
    if (v)
      for (int i = 0; i <= m; ++i)
        if (nu[i] == 0.0 && (R[i] != cplx(0) || (i < m && P[i] != cplx(0)))) return 22;
  }
  return 0;
}
// H diagonal: the matrix recurrence must equal the scalar one r <- (h r - z r) / radius, p += a r run in the same order, bit for
// bit (adding exact zeros does not round), and R[1..m] must be exactly zero
static int diagonal_restart(int m, const cplx* a, const cplx* leja, double radius, std::mt19937_64& rng) {
  std::normal_distribution<double> g;
  const int ldh = m + 2;
  std::vector<cplx> H((size_t)ldh * ldh, cplx(0)), P, R, Rn;
  for (int i = 0; i <= m; ++i) H[(size_t)i * ldh + i] = cplx(g(rng), g(rng));
  const cplx h = H[0];
  const double beta0 = 1.0 + 0.001 * (double)(rng() % 1000);
  const double beta = restart(H.data(), ldh, m, a, leja, radius, beta0, nullptr, P, R, Rn);
  cplx r = beta0, p = a[0] * beta0;
  auto step = [&](cplx z) {
    cplx acc = 0;
    acc += h * r;
    r = (acc - z * r) / radius;
  };
  for (int k = 1; k <= m - 1; ++k) {
    step(leja[k - 1]);
    p += a[k] * r;
  }
  step(leja[m - 1]);
  const double ab = std::abs(r);
  double b2 = 0;
  b2 += ab * ab;
  const double beta_ref = std::sqrt(b2);
  r *= (1.0 / beta_ref);
  if (!(beta == beta_ref) || !(P[0].real() == p.real() && P[0].imag() == p.imag()) ||
      !(R[0].real() == r.real() && R[0].imag() == r.imag()))
    return 30;
  for (int i = 1; i <= m; ++i)
    if (R[i] != cplx(0) || (i < m && P[i] != cplx(0))) return 31;
  return 0;
}
// the named inputs of tests/newton_restart_cases.h, bit for bit
static int named_restarts() {
  const double* e = kNewtonRestartExpected;
  std::vector<cplx> P, R, Rn;
  int n = 0;
  for (const NewtonRestartCase& c : kNewtonRestartCases) {
    const NewtonRestartInputs in = newton_restart_inputs(c);
    const double beta = restart(in.Hess.data(), c.ldh, c.m, in.a.data() + c.n_s, in.leja.data() + c.n_s, c.radius, c.beta,
                                c.nu_mode ? in.nu.data() : nullptr, P, R, Rn);
    bool ok = true;
    for (int i = 0; i < c.m; ++i, e += 2) ok = ok && P[i].real() == e[0] && P[i].imag() == e[1];
    for (int i = 0; i <= c.m; ++i, e += 2) ok = ok && R[i].real() == e[0] && R[i].imag() == e[1];
    ok = ok && beta == *e++;
    if (!ok) {
      std::printf("newton restart: case '%s' does not match the table\n", c.name);
      return 40;
    }
    ++n;
  }
  if (e != kNewtonRestartExpected + sizeof(kNewtonRestartExpected) / sizeof(double)) return 41;
  std::printf("newton restart: %d named cases match the table\n", n);
  return 0;
}

int main() {
  std::mt19937_64 rng(1);
  std::normal_distribution<double> g;
  // cheby coefficients over a range of alpha
  for (double dt : {1e-14, 0.01, 0.5, 3.0, 40.0}) {
    auto a = qp::cheby_coeffs(20.0, dt, 1e-12);
    if (a.empty()) return 1;
  }
  // Hessenberg eigenvalues of all leading blocks, m = 1 .. 40
  for (int m = 1; m <= 40; ++m) {
    std::vector<cplx> H((size_t)(m + 1) * (m + 1));
    for (int c = 0; c < m + 1; ++c)
      for (int r = 0; r < m + 1; ++r) H[(size_t)c * (m + 1) + r] = (r <= c + 1) ? cplx(g(rng), g(rng)) : cplx(0);
    std::vector<cplx> ritz((size_t)m * (m + 1) / 2);
    if (qp::diagonalize_hessenberg(H.data(), m + 1, m, true, ritz.data()) != 0) return 2;
    // Leja ordering + Newton coefficients, several restarts
    std::vector<cplx> leja((size_t)8 * m + 8), a((size_t)8 * m + 8);
    int n = 0, n_a = 0;
    double radius = 0;
    for (auto& z : ritz) radius = std::max(radius, 1.2 * std::abs(z));
    for (int s = 0; s < 4; ++s) {
      std::vector<cplx> cand = ritz;
      qp::extend_leja(leja.data(), n, cand.data(), (int)cand.size(), m);
      n += m;
      int st = qp::extend_newton_coeffs(a.data(), n_a, leja.data(), QP_FUNC_EXPMI, nullptr, nullptr, n, radius);
      if (st != 0 && st != QP_E_DIVDIFF_UNDERFLOW) return 3;
      if (st != 0) break;
      n_a = n;
      // this restart's polynomial and next start vector, on the random matrix and on a diagonal one
      if (int rc = random_restart(H, m, a.data() + n - m, leja.data() + n - m, radius, rng)) return rc;
      if (int rc = diagonal_restart(m, a.data() + n - m, leja.data() + n - m, radius, rng)) return rc;
    }
  }
  if (int rc = named_restarts()) return rc;
  // CSC -> CSR and row partitions on random patterns (empty rows / columns included)
  for (int trial = 0; trial < 200; ++trial) {
    const int64_t nr = 1 + rng() % 50, nc = 1 + rng() % 50;
    std::vector<int64_t> colptr{1}, rowval;
    for (int64_t c = 0; c < nc; ++c) {
      std::vector<int64_t> rows;
      for (int64_t r = 0; r < nr; ++r)
        if (rng() % 5 == 0) rows.push_back(r + 1);
      rowval.insert(rowval.end(), rows.begin(), rows.end());
      colptr.push_back(colptr.back() + (int64_t)rows.size());
    }
    std::vector<qp_c128> nz(rowval.size() + 1, qp_c128{1.0, 2.0});
    std::vector<int64_t> rp(nr + 1);
    std::vector<int32_t> col(rowval.size() + 1);
    std::vector<qp_c128> vals(rowval.size() + 1);
    if (qp::csc_to_csr(nr, nc, colptr.data(), rowval.data(), nz.data(), 1, rp.data(), col.data(), vals.data()) != 0) return 4;
    for (int parts = 1; parts <= 9; ++parts)
      for (int bal = 0; bal < 2; ++bal) {
        std::vector<int64_t> b(parts + 1);
        qp::partition_rows(rp.data(), nr, parts, bal, b.data());
        if (b[0] != 0 || b[parts] != nr) return 5;
      }
  }
  std::puts("host numerics: sanitizer run clean");
  return 0;
}
namespace qp {
int fail(int status, const char* fmt, ...) { (void)fmt; return status; }
void set_error(const char*) {}
}
