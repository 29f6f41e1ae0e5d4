"""Extended-precision reference of ONE fused Chebyshev term (include/qprop.h, the comment above qp_cheby_term), the per-row error
bound the GPU tests hold every kernel family to (tests/test_gpu_cheby_term.py), and the mutations that show the bound can fail
(tests/test_cheby_term_ref.py).  NumPy in np.clongdouble (80-bit here) and nothing of the library or of oracle/qp_oracle.py:

    s = (A x)[i];  x_i = x[xoff + i];  t = c (s - beta x_i) (+ v0[i] if v0)
    skip:      no r
    otherwise: r = acc_in ? acc_in[i] : a_prev * (n_defer == 1 ? v0[i] : x_i)
               if n_defer == 2: r += a_d2 v0[i];   if n_defer >= 1: r += a_d1 x_i;     r += a t;   r = phase r

with the magnitudes the bound is relative to (every operand by its modulus: what the row could be without cancellation)

    T_i = |c| (sum_j |a_ij| |x_j| + |beta| |x_i|) + |v0_i|
    R_i = |phase| (|first operand of r| + |a_d2| |v0_i| + |a_d1| |x_i| + |a| T_i)

and the acceptance test  |got_i - ref_i| <= (S_i + K) 2^-52 magnitude_i,  S_i = stored entries of row i (the padded length where a
format pads or completes rows), K = 12.  Nothing in it is measured; u = 2^-53 is the unit roundoff, so 2^-52 = 2 u:

  the row sum    The kernels accumulate each component of s by FMAs, two per stored entry (ar xr, then -ai xi), in at least two
                 chains (s0 / s1 of the row-block kernels, T >= 2 lanes of the CSR kernel, 64 lanes of the dense one) that are added
                 afterwards: one chain takes at most ceil(S / 2) entries = S + 1 roundings, and at most 7 additions of partial sums
                 follow (s0 + s1; the six shuffle levels of a 64-lane reduction) -- additions of zeros are exact.  Every rounding is
                 relative to a partial sum no larger than P = sum_j (|ar xr| + |ai xi|) resp. Q = sum_j (|ar xi| + |ai xr|), and
                 P^2 + Q^2 <= 2 (sum_j |a_ij| |x_j|)^2.  So |ds| <= sqrt(2) (S + 8) u sum = 0.7072 (S + 8) 2^-52 sum
                 <= (S + 5.66) 2^-52 sum_j |a_ij| |x_j|.  (The column-blocked mirror rounds each product on its own -- a cmul, two
                 roundings per component -- and adds the S products of a row in one chain: S + 1 roundings, inside the count
                 above.  The Pauli-string kernel: S strings, the count of tests/test_gpu_pauli_edges.py -- S + 8 there with the two
                 roundings of its plain epilogue, S + 6 for the sum alone, which with the 5.84 below is still under S + 12.)
  d = s - beta x_i     one FMA per component:                                          0.5  (in 2^-52 |d|)
  c d            cmul: a product and an FMA per component, < sqrt(8) u |c| |d|:        1.42
  + v0           one addition per component, u |t|:                                    0.5
                 => |dt| <= (S + 5.66 + 2.42) 2^-52 T_i = (S + 8.08) 2^-52 T_i
  r              inherits |a| |dt|; a_prev * Psi (or nothing: acc_in is exact), the FMAs of a_d2, a_d1 and a: four roundings of
                 0.5 each, relative to partial sums inside R_i / |phase|;  the phase: one more cmul, 1.42
                 => |dr| <= (S + 8.08 + 3.42) 2^-52 R_i = (S + 11.5) 2^-52 R_i,   K = 12.
  (second-order terms are below 1e-13 of this for S < 1e3.)  The same K bounds t, with room to spare.

  The matrix-free Liouvillian has no stored row: its row sum is  M_L rho - rho M_R + A rho A^+  with n products per matrix product,
  M_L/R formed on the device from H and A^+ A (n products and two additions more); the longest chain has 2 n + 4 roundings, and the
  magnitude is taken from the dense factors by modulus (liouvillian_magnitude): S_i = 2 n + 4 there.

A wrong operand on ONE row (v0 for x_i, a dropped a_d2, a skipped phase, a neighbouring column) moves that row by a multiple of one
of the terms of its magnitude -- with coefficients of order one and S of order ten, thousands of times the bound.
tests/test_cheby_term_ref.py applies each such mutation to this reference and requires a row beyond the bound."""
import types

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS = LD(2.0) ** -52
K = 12
assert np.finfo(LD).nmant >= 63, "the reference needs an extended-precision long double"

# every mutation of term_from_sums (tests/test_cheby_term_ref.py); the three mutations of the matrix are applied to A by the test
MUTATIONS = ("xi_without_offset", "v0_before_c", "swap_deferred", "v0_for_xi_in_defer2", "no_phase", "phase_on_t",
             "a_prev_with_acc_in")


def defer_of(skip=0, n_defer=0, a_d1=0.0, a_d2=0.0):
    """The fields of a qp_acc_defer, for callers without the library."""
    return types.SimpleNamespace(skip=int(skip), n_defer=int(n_defer), a_d1=float(a_d1), a_d2=float(a_d2))


def row_sums(A, x):
    """(s, sabs): s_i = sum_j a_ij x_j in clongdouble over the STORED entries of the SciPy CSR matrix, sabs_i = sum_j |a_ij| |x_j|."""
    A = A.tocsr()
    nrows = A.shape[0]
    assert len(x) == A.shape[1]
    rows = np.repeat(np.arange(nrows), np.diff(A.indptr))
    xg = np.asarray(x, dtype=CLD)[A.indices]
    val = A.data.astype(CLD)
    s, sabs = np.zeros(nrows, dtype=CLD), np.zeros(nrows, dtype=LD)
    np.add.at(s, rows, val * xg)
    np.add.at(sabs, rows, np.abs(val) * np.abs(xg))
    return s, sabs


def term_from_sums(s, sabs, x, xoff, v0, acc_in, c, beta, a_prev, a, phase, defer, mutation=None):
    """(t, r, T, R) of the header formula from the row sums; r and R are None for a skipped term.  ``mutation``: one of MUTATIONS,
    a deliberately WRONG formula (the checker of the checker)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    n = len(s)
    x = np.asarray(x, dtype=CLD)
    assert 0 <= xoff and xoff + n <= len(x)
    xi = x[:n] if mutation == "xi_without_offset" else x[xoff:xoff + n]
    v0 = None if v0 is None else np.asarray(v0, dtype=CLD)
    acc_in = None if acc_in is None else np.asarray(acc_in, dtype=CLD)
    c, phase = CLD(c), CLD(phase)
    beta, a_prev, a = LD(beta), LD(a_prev), LD(a)
    d = s - beta * xi
    if mutation == "v0_before_c" and v0 is not None:
        t = c * (d + v0)
    else:
        t = c * d + (0 if v0 is None else v0)
    T = np.abs(c) * (sabs + np.abs(beta) * np.abs(xi)) + (0 if v0 is None else np.abs(v0))
    if defer is not None and defer.skip:
        return t, None, T, None
    n_defer = 0 if defer is None else int(defer.n_defer)
    a_d1, a_d2 = (LD(0), LD(0)) if defer is None else (LD(defer.a_d1), LD(defer.a_d2))
    if mutation == "swap_deferred":
        a_d1, a_d2 = a_d2, a_d1
    assert n_defer in (0, 1, 2) and (n_defer == 0 or v0 is not None or (n_defer == 1 and acc_in is not None))
    if acc_in is not None:
        first = a_prev * acc_in if mutation == "a_prev_with_acc_in" else acc_in
    else:
        first = a_prev * (v0 if n_defer == 1 else xi)
    r, R = first.copy(), np.abs(first)
    if n_defer == 2:
        r = r + a_d2 * v0
        R = R + np.abs(a_d2) * np.abs(v0)
    if n_defer >= 1:
        r = r + a_d1 * (v0 if (mutation == "v0_for_xi_in_defer2" and n_defer == 2) else xi)
        R = R + np.abs(a_d1) * np.abs(xi)
    r = r + a * (phase * t if mutation == "phase_on_t" else t)
    R = R + np.abs(a) * T
    if mutation not in ("no_phase", "phase_on_t"):
        r = phase * r
    return t, r, T, np.abs(phase) * R


def term_ref(A, x, xoff, v0, acc_in, c, beta, a_prev, a, phase, defer):
    """(t, r, T, R) of one fused term of the SciPy CSR matrix A (nrows x ncols) in clongdouble: the header formula, see above."""
    s, sabs = row_sums(A, x)
    return term_from_sums(s, sabs, x, xoff, v0, acc_in, c, beta, a_prev, a, phase, defer)


def bound(S, magnitude):
    """(S_i + K) 2^-52 magnitude_i; every magnitude must be positive (all operands nonzero: an empty row qualifies too)."""
    magnitude = np.asarray(magnitude, dtype=LD)
    assert np.all(magnitude > 0), "a row without magnitude: the case must have nonzero operands on every row"
    return (np.asarray(S, dtype=LD) + K) * EPS * magnitude


def beyond(got, ref, S, magnitude):
    """rows of ``got`` beyond the bound around ``ref``"""
    err = np.abs(np.asarray(got, dtype=CLD) - ref)
    return np.nonzero(~(err <= bound(S, magnitude)))[0]


def check_rows(got, ref, S, magnitude, what, quiet=False):
    """Every row under the bound; returns (and prints, for -s) the largest err / bound."""
    err = np.abs(np.asarray(got, dtype=CLD) - ref)
    bnd = bound(S, magnitude)
    ratio = err / bnd
    worst = int(np.argmax(ratio))
    if not quiet:
        print(f"[term rows] {what}: max err/bound {float(ratio[worst]):.4f} at row {worst} (block {worst >> 6}, lane {worst & 63})")
    bad = np.nonzero(~(err <= bnd))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rows beyond the bound, first {int(bad[0])} (block {int(bad[0]) >> 6}, lane {int(bad[0]) & 63}): "
                           f"err {float(err[bad[0]]):.3e} bound {float(bnd[bad[0]]):.3e}")
    return float(ratio[worst])


def liouvillian_magnitude(H, c_ops, x):
    """sum over the dense factors, by modulus, of what the matrix-free Liouvillian adds up for row i of vec(rho) (column-major):
    (|H| + sum |A^+| |A| / 2) |rho| + |rho| (the same) + sum |A| |rho| |A^+|  -- no smaller than sum_j |L_ij| |x_j| of the assembled
    superoperator, whose entries are sums of these factors."""
    n = H.shape[0]
    rho = np.abs(np.asarray(x, dtype=CLD)).reshape(n, n).T
    M = np.abs(np.asarray(H)).astype(LD)
    W = np.zeros((n, n), dtype=LD)
    for A in c_ops:
        aA = np.abs(np.asarray(A)).astype(LD)
        M = M + 0.5 * (aA.T @ aA)
        W = W + aA @ rho @ aA.T
    W = W + M @ rho + rho @ M
    return W.T.reshape(-1)
