"""Extended-precision reference for the Gram-Schmidt step of the Krylov engine (csrc/kernels_blas.hip: multidot_kernel,
multidot_reduce_kernel, mgs_solve_kernel, mgs_update_kernel; csrc/kernels_arnoldi.hip; csrc/mgs_common.h) on bases that are NOT
orthogonal.  The engine's low-synchronisation step turns the classical inner products c = V^H w and the Gram rows <v_i|v_k> into
the coefficients of sequential modified Gram-Schmidt by a triangular solve; on a basis the engine built itself every Gram entry
is a rounding residue and the solve's Gram term moves nothing.  ``make_basis`` gives it Gram entries of a chosen size, ``mgs`` is
the sequential recurrence of src/arnoldi.jl:84-87 in ``np.clongdouble`` (it shares nothing with the solve), and the bounds are
derived from absolute values -- nothing in them is measured.  ``banded`` is a small non-Hermitian operator whose product is
formed by slicing, in the same precision.  Test infrastructure, host only."""
import math

import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53                      # unit roundoff of the kernels' arithmetic
SEAMS = (0, 255, 256, 65535, 65536, 131071, 131072)   # first / last element of a workgroup, of a grid stride, of a round of rows
SEAM_WEIGHT = 30.0


def seam_elements(n):
    """The elements at which a grid-stride loop of the vector kernels changes lane, workgroup, stride or round, and the last one."""
    return sorted({e for e in SEAMS + (n - 1,) if 0 <= e < n})


def delta_for(J):
    """Size of the off-diagonal Gram entries for a basis of J + 1 vectors: as large as keeps the solve's magnitude recursion tame."""
    return 0.1 if J <= 20 else 0.05 if J <= 40 else 0.03


def seam_weight(n):
    """SEAM_WEIGHT where the vector is long enough to carry it.  k elements weighted s times the typical 1 / sqrt(n) add about
    s^2 sqrt(k) / n (random phases) to every Gram entry; that is to stay below 0.05, the size of the entries the basis is built to
    have -- else the weighted elements ARE the vectors, the Gram entries are of order one whatever delta is, and the solve's
    magnitude recursion (coef_bound) grows until the bound admits anything (n = 257, 88 vectors: 10^13 with weight 30).  So
    s = 30 from n = 36000 up, 10 at n = 4197, 2.7 at n = 257, where a single element is 1 / 257 of a dot product anyway --
    thirteen orders of magnitude above the dot bound with or without a weight."""
    k = len(seam_elements(n))
    return max(1.0, min(SEAM_WEIGHT, math.sqrt(0.05 * n / math.sqrt(k))))


def _weigh_seams(X, n):
    X[..., seam_elements(n)] *= seam_weight(n)


def make_basis(n, J, delta, seed):
    """V_0 .. V_J (rows of the returned complex128 array, unit norm): V = U (I + delta R), U orthonormal (QR of a random complex
    n x (J + 1) matrix), R strictly upper triangular with entries in the unit disk, so <V_i|V_k> = O(delta).  The entries at the
    seam elements are multiplied by seam_weight(n) before the vectors are normalised: a kernel that drops or doubles one element at
    a stride edge then moves a dot product by far more than 1 / n.  (Fewer elements than vectors, n = 1: random unit vectors --
    the identity the kernels rest on holds for any basis.)"""
    rng = np.random.default_rng(seed)
    k = J + 1
    A = rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))
    Q = np.linalg.qr(A)[0] if n >= k else A
    R = np.triu((rng.uniform(-1, 1, (k, k)) + 1j * rng.uniform(-1, 1, (k, k))) / math.sqrt(2.0), 1)
    V = np.ascontiguousarray((Q @ (np.eye(k) + delta * R)).T)
    _weigh_seams(V, n)
    V /= np.linalg.norm(V, axis=1)[:, None]
    return V


def make_vector(V, seed, mix=0.3):
    """A vector to orthogonalise against the rows of V: random, plus mix x a random combination of them (coefficients of order one
    for the solve to find), seams weighted like the basis."""
    rng = np.random.default_rng(seed)
    k, n = V.shape
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    _weigh_seams(w, n)
    w /= np.linalg.norm(w)
    w += mix * ((rng.standard_normal(k) + 1j * rng.standard_normal(k)) @ V)
    return w


def dot(a, b):
    """<a|b> in extended precision."""
    return np.sum(np.conj(np.asarray(a, dtype=CLD)) * np.asarray(b, dtype=CLD))


def gram(V):
    """G[i, k] = <V_i|V_k> of the rows of V, in extended precision."""
    V = np.asarray(V, dtype=CLD)
    return np.conj(V) @ V.T


def mgs(V, w):
    """Sequential modified Gram-Schmidt exactly as src/arnoldi.jl:84-87: h_i = <v_i|w>; w -= h_i v_i (no division: the basis need
    not be normalised).  Returns (h, w_out, |w_out|^2) in extended precision."""
    w = np.array(w, dtype=CLD)
    h = np.zeros(len(V), dtype=CLD)
    for i, v in enumerate(V):
        v = np.asarray(v, dtype=CLD)
        h[i] = np.sum(np.conj(v) * w)
        w -= h[i] * v
    return h, w, np.sum(w.real * w.real + w.imag * w.imag)


# ---------------------------------------------------------------------------------------------------------------------------
# bounds from absolute values
# ---------------------------------------------------------------------------------------------------------------------------
def n_path(n):
    """Longest chain of additions of a kernel dot product over n elements: ceil(n / 65536) per lane (the fused mat-vec has half
    as many rounds), 6 levels of the wavefront tree, 4 wavefronts, 256 partials (added in sequence where the host sums them)."""
    return -(-int(n) // 65536) + 6 + 4 + 256


def dot_bound(absa, absb, n):
    """|err| of a double-precision <a|b> over n elements: (n_path + 8) u sum_e |a_e| |b_e|."""
    return (n_path(n) + 8) * U * float(np.sum(np.asarray(absa, dtype=LD) * np.asarray(absb, dtype=LD)))


def coef_bound(cb, absG):
    """The solve's recursion on magnitudes: hb_i = cb_i + sum_{k<i} |G_ik| hb_k (absG: (J+1) x (J+1), its strict lower triangle)."""
    hb = np.zeros(len(cb), dtype=LD)
    for i in range(len(cb)):
        hb[i] = cb[i] + np.sum(absG[i, :i] * hb[:i])
    return hb


def update_bound(J, absw, absV, absh, hb):
    """Element by element: (J + 4) u (|w_e| + sum_i |h_i| |v_ie|) + sum_i hb_i |v_ie|."""
    absV = np.asarray(absV, dtype=LD)
    return (J + 4) * U * (np.asarray(absw, dtype=LD) + np.asarray(absh, dtype=LD) @ absV) + np.asarray(hb, dtype=LD) @ absV


def norm2_bound(absw, wb, n):
    """|sum of the kernel's |w|^2 partials - |w_ref|^2|: the element errors wb pushed through the squares, plus the summation."""
    absw, wb = np.asarray(absw, dtype=LD), np.asarray(wb, dtype=LD)
    return float(np.sum(2 * absw * wb + wb * wb) + (n_path(n) + 8) * U * np.sum((absw + wb) ** 2))


class Column:
    """Reference of one orthogonalisation column: w against V_0 .. V_j (rows of V), with every bound the tests assert.
    ``w_err``: an element-wise bound on what the kernel's w may differ from the reference's before the column starts (the
    mat-vec's rounding; None: w is given exactly).  ``rel_last``: relative error of the kernel's copy of the LAST basis vector
    (the engine normalises it on the device before it takes the column)."""

    def __init__(self, V, w, j=None, w_err=None, rel_last=0.0, G=None):
        """V: at least j + 1 rows (all of them when j is None); G: <V_i|V_k> where the caller has it (gram())."""
        j = len(V) - 1 if j is None else j
        V = np.asarray(V[: j + 1], dtype=CLD)
        n = V.shape[1]
        self.j, self.n = j, n
        absV, absw = np.abs(V), np.abs(np.asarray(w, dtype=CLD))
        G = gram(V) if G is None else np.asarray(G)[: j + 1, : j + 1]
        self.c = np.array([dot(v, w) for v in V])                    # classical inner products <V_i|w>
        self.g = G[:, j].copy()                                      # the fresh Gram row <V_i|V_j>
        self.cb = np.array([dot_bound(a, absw, n) for a in absV], dtype=LD)
        self.gb = np.array([dot_bound(a, absV[j], n) for a in absV], dtype=LD)
        if w_err is not None:
            self.cb += absV @ np.asarray(w_err, dtype=LD)
        if rel_last:
            self.cb[j] += rel_last * float(np.sum(absV[j] * absw))
        self.absG = np.abs(G)
        self.h, self.w_out, self.norm2 = mgs(V, w)
        self.hb = coef_bound(self.cb, self.absG)
        self.wb = update_bound(j, absw, absV, np.abs(self.h), self.hb)
        if w_err is not None:
            self.wb = self.wb + np.asarray(w_err, dtype=LD)
        if rel_last:
            self.wb = self.wb + rel_last * np.abs(self.h[j]) * absV[j]
        self.norm2_b = norm2_bound(np.abs(self.w_out), self.wb, n)

    # largest error / bound of a kernel result (0 / 0 counts as 0: a bound of zero admits only the exact value)
    @staticmethod
    def _ratio(err, bound):
        err, bound = np.atleast_1d(np.asarray(err, dtype=LD)), np.atleast_1d(np.asarray(bound, dtype=LD))
        out = np.where(err == 0, LD(0), err / np.where(bound > 0, bound, LD(1e-4000)))
        return float(out.max()) if out.size else 0.0

    def ratio_dots(self, reduced):
        """reduced = [c_0 .. c_j | g_0 .. g_j] as the multidot leaves it."""
        j = self.j
        red = np.asarray(reduced[: 2 * (j + 1)], dtype=CLD)
        return max(self._ratio(np.abs(red[: j + 1] - self.c), self.cb), self._ratio(np.abs(red[j + 1:] - self.g), self.gb))

    def ratio_coefs(self, h):
        return self._ratio(np.abs(np.asarray(h, dtype=CLD) - self.h), self.hb)

    def ratio_vector(self, w_out):
        return self._ratio(np.abs(np.asarray(w_out, dtype=CLD) - self.w_out), self.wb)

    def ratio_norm2(self, partials):
        s = np.sum(np.asarray(partials, dtype=CLD).real.astype(LD))
        return self._ratio(abs(s - self.norm2), self.norm2_b)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 emulation of the low-synchronisation step (what the kernels compute, in NumPy), with the defects a test must catch
# ---------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("conjugated_gram", "transposed_tri_index", "gram_row_from_row_above", "dropped_seam_element", "skipped_basis_vector")


def lowsync_emulation(V, w, defect=None):
    """c = V^H w, G = V^H V, forward substitution h_i = c_i - sum_{k<i} G_ik h_k over the packed strict lower triangle, update in
    MGS order; all in complex128.  Returns (reduced = [c | g], h, w_out).  ``defect`` plants one of DEFECTS."""
    V = np.asarray(V, dtype=np.complex128)
    w = np.asarray(w, dtype=np.complex128)
    j, n = len(V) - 1, V.shape[1]
    Vd = V
    if defect == "dropped_seam_element":        # a stride edge that is never read
        Vd = V.copy()
        Vd[:, seam_elements(n)[len(seam_elements(n)) // 2]] = 0.0
    c = np.conj(Vd) @ w
    G = np.conj(V) @ V.T                        # G[i, k] = <V_i|V_k>
    if defect == "conjugated_gram":
        G = np.conj(G)
    if defect == "gram_row_from_row_above":
        G = np.vstack([G[:j], G[j - 1: j]]) if j >= 1 else G
    tri = lambda i, k: i * (i - 1) // 2 + k     # noqa: E731  (mgs_common.h: tri_index)
    Gt = np.zeros(j * (j + 1) // 2 + 1, dtype=np.complex128)
    for i in range(1, j + 1):
        Gt[tri(i, 0): tri(i, 0) + i] = G[i, :i]
    h = c.copy()
    for i in range(1, j + 1):
        for k in range(i):
            h[i] -= Gt[tri(k, i) if defect == "transposed_tri_index" else tri(i, k)] * h[k]   # (tri(k, i) stays inside Gt)
    out = w.copy()
    for i in range(j + 1):
        if defect == "skipped_basis_vector" and i == j // 2:
            continue
        out = out - h[i] * V[i]
    return np.concatenate([c, np.conj(Vd) @ V[j]]), h, out


# ---------------------------------------------------------------------------------------------------------------------------
# a banded operator
# ---------------------------------------------------------------------------------------------------------------------------
FEW_VALUES = np.array([0.31 + 0.12j, -0.27 + 0.05j, 0.11 - 0.33j, -0.19 - 0.08j, 0.23 + 0.29j])


class Banded:
    """Non-Hermitian banded operator with open boundaries: A[r, r + d] = values[d][r] for every offset d and every row r with
    0 <= r + d < n.  ``csr()`` is what lib.Matrix takes; ``apply`` / ``abs_apply`` work by slicing in extended precision
    (scipy.sparse does not carry long double)."""

    def __init__(self, n, offsets, seed, real=False, few_values=False):
        rng = np.random.default_rng(seed)
        self.n = int(n)
        self.offsets = tuple(int(d) for d in offsets if abs(int(d)) < n)
        self.values = {}
        for d in self.offsets:
            m = self.n - abs(d)
            if few_values:
                v = FEW_VALUES[rng.integers(0, len(FEW_VALUES), m)]
                v = v.real.copy() if real else v
            elif real:
                v = rng.uniform(-0.4, 0.4, m)
            else:
                v = rng.uniform(-0.3, 0.3, m) + 1j * rng.uniform(-0.3, 0.3, m)
            self.values[d] = v
        self.max_row = len(self.offsets)

    def csr(self):
        import scipy.sparse as sp
        A = sp.diags([self.values[d] for d in self.offsets], list(self.offsets), shape=(self.n, self.n), format="csr")
        A.sort_indices()
        return A

    def _sum(self, x, vals):
        y = np.zeros(self.n, dtype=x.dtype)
        for d in self.offsets:
            v = vals(self.values[d])
            if d >= 0:
                y[: self.n - d] += v * x[d:]
            else:
                y[-d:] += v * x[: self.n + d]
        return y

    def apply(self, x):
        return self._sum(np.asarray(x, dtype=CLD), lambda v: v.astype(CLD))

    def abs_apply(self, x):
        """(|A| |x|)_r, real."""
        return self._sum(np.abs(np.asarray(x, dtype=CLD)), lambda v: np.abs(v.astype(CLD)))

    def row_bound(self, x, rel_x=0.0):
        """Element-wise bound on a double-precision A x against ``apply(x)``: every row is a chain of at most max_row complex
        multiply-adds on two accumulators, their sum and one scaling -- 2 (max_row + 4) u (|A| |x|)_r covers both components --
        plus rel_x (|A| |x|)_r for an x that the device holds with relative error rel_x."""
        return (2 * (self.max_row + 4) * U + rel_x) * self.abs_apply(x)


def banded(n, offsets, seed, real=False, few_values=False):
    return Banded(n, offsets, seed, real=real, few_values=few_values)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_krylov_columns.py (tests/test_krylov_ref.py runs the emulation over the same families)
# ---------------------------------------------------------------------------------------------------------------------------
# building blocks: (n, J).  n = 257: the tile of eight basis vectors of the multidot (7 | 8 | 9, 15 | 16 | 17), the rounds of four
# of the update (2 | 3 | 4, 6 | 7 | 8), the solve's second wavefront pass (J > 63) and the longest basis the solve has room for (87);
# n = 1; the vector kernels' stride of 65536 and their round of two strides, one element short and one over, and one and a half rounds
BLOCK_CASES = ([(257, J) for J in (0, 1, 2, 3, 4, 6, 7, 8, 9, 15, 16, 17, 40, 87)] + [(1, 3)] +
               [(n, J) for n in (65535, 65537, 131071, 131073, 196613) for J in (3, 8)])
J_TOO_LONG = 88                       # device.h: mgs_lowsync_fits -- 16 (3 * 89 + 88 * 89 / 2) bytes > 64 KiB
DTS = (0.37, -0.8)
# the engine's column: n = 4197 is 65 row blocks and a ragged 66th; J at every edge of the fused mat-vec's instances (3 | 4, 7 | 8,
# 11 | 12, 15 | 16, 19 | 20: the end of fusion), 35 | 36 (reduction + solve in the update's prologue | ticket path) and 87 | 88 (the
# low-synchronisation form | sequential passes)
COLUMN_N = 4197
COLUMN_J = (1, 3, 4, 7, 8, 11, 12, 15, 16, 19, 20, 35, 36, 40, 87, 88)
VARIANT_J = (3, 8, 19, 20, 36)        # real-valued and value-dictionary operators: one J per kernel family is enough
COLUMN_SIZES = (131071, 131073, 131072 + 3 * 512 + 77, 262144 + 300)   # rounds of 131072 rows: short of one, ragged after one and after two
SIZE_J = (3, 8)
OFFSETS = (-200, -70, -3, -1, 0, 1, 2, 64)
