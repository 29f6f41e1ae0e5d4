"""The inputs of the lazy-sum tests, built on the host alone: tests/test_gpu_lazy_sum.py runs them through qp_operator_create /
set_coeffs / set_scale in every device format, tests/test_lazy_sum_ref.py (no GPU) shows on the SAME inputs that the bound of
tests/lazy_sum_ref.py holds for the exact chain and catches every mutation.

N = 197 rows: three full 64-row blocks and a ragged one of five rows.  The terms live on a band of offsets 0, +-1, +-2, +-7, +-64;
each is Hermitian (so the same inputs serve the packed format) with a pattern of its own -- a random half of the offset pairs on a
random half of the rows -- and the union pattern is whatever the terms of a case cover.  Term 1 is all-empty when L >= 3, the last
term repeats the pattern of term 0 exactly when L >= 2, and term 0 is handed over with duplicate entries within its rows (the
library sums those, as Julia's sparse() does; two per position, so the sum is one rounding in any order).  Values: moduli in
[0.5, 1.5) with random phases (real on the diagonal), times 2^k per term, k in [-20, 20] -- a small term is protected by its own
magnitude, not by a global norm.  The real variant has real planes.

Term counts 1, 2, 31, 32, 33, 64, 65 around the 32 coefficients one launch carries, one drift term each (ncoeffs = L - 1), and three
more splits: L = 33 without drift, L = 33 all drift (only the scale moves), L = 65 with 25 coefficients (the border inside the
second chunk)."""
import dataclasses
import functools
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lazy_sum_ref as R  # noqa: E402

N = 197
OFFSETS = (0, 1, 2, 7, 64)
TERM_COUNTS = (1, 2, 31, 32, 33, 64, 65)
SPLITS = {"L33-no-drift": (33, 33), "L33-all-drift": (33, 0), "L65-border-in-chunk-2": (65, 25)}
COMPLEX_SCALE = 0.75 - 1.25j


@dataclasses.dataclass(frozen=True)
class Term:
    """raw CSR as handed to the library: sorted columns, duplicates kept"""
    rowptr: np.ndarray
    col: np.ndarray
    vals: np.ndarray


def raw_csr(n, rows, cols, vals):
    order = np.lexsort((cols, rows))
    rows, cols, vals = np.asarray(rows)[order], np.asarray(cols)[order], np.asarray(vals, dtype=np.complex128)[order]
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int64)
    return Term(rowptr, cols.astype(np.int64), vals)


def from_scipy(A):
    """a SciPy matrix as a Term (canonical: sorted, duplicates summed, explicit zeros kept)"""
    A = A.tocsr().astype(np.complex128)
    A.sum_duplicates()
    A.sort_indices()
    return Term(A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.copy())


def term_rows(t):
    return np.repeat(np.arange(len(t.rowptr) - 1), np.diff(t.rowptr))


def hermitian_entries(n, rows_upper, cols_upper, vals_upper):
    """(rows, cols, vals) of the upper entries (i <= j; real on the diagonal) and their conjugate mirror images"""
    r, c, v = np.asarray(rows_upper), np.asarray(cols_upper), np.asarray(vals_upper, dtype=np.complex128).copy()
    diag = r == c
    v[diag] = v[diag].real
    off = ~diag
    return np.concatenate([r, c[off]]), np.concatenate([c, r[off]]), np.concatenate([v, np.conj(v[off])])


def _values(rng, count, k, real):
    mod = rng.uniform(0.5, 1.5, count)
    v = mod * (rng.choice([-1.0, 1.0], count) if real else np.exp(2j * np.pi * rng.uniform(0.0, 1.0, count)))
    v = np.asarray(v, dtype=np.complex128)
    return np.ldexp(v.real, k) + 1j * np.ldexp(v.imag, k)


def _upper_pattern(rng, n=N, offsets=OFFSETS):
    offs = rng.choice(offsets, size=rng.integers(2, 4), replace=False)
    rows = np.sort(rng.choice(n, size=n // 2, replace=False))
    r = np.concatenate([rows[rows + d < n] for d in offs])
    c = np.concatenate([rows[rows + d < n] + d for d in offs])
    return r, c


def build_terms(L, real, seed, n=N):
    rng = np.random.default_rng(seed)
    terms = []
    first = None
    for l in range(L):
        k = int(rng.integers(-20, 21))
        if L >= 3 and l == 1:
            terms.append(raw_csr(n, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0)))
            continue
        r, c = _upper_pattern(rng, n)
        if l == 0:
            first = (r, c)
        if L >= 2 and l == L - 1:
            r, c = first
        rows, cols, vals = hermitian_entries(n, r, c, _values(rng, len(r), k, real))
        if l == 0:          # a second entry on every third upper position (and on its mirror image)
            r2, c2 = r[::3], c[::3]
            rows2, cols2, vals2 = hermitian_entries(n, r2, c2, _values(rng, len(r2), k, real))
            rows, cols, vals = np.concatenate([rows, rows2]), np.concatenate([cols, cols2]), np.concatenate([vals, vals2])
        terms.append(raw_csr(n, rows, cols, vals))
    return terms


def union_planes(terms, n, ncols=None):
    """(rowptr, col, planes): the union pattern as sorted CSR and every term's values on it (duplicates summed; L x P)"""
    ncols = n if ncols is None else ncols
    lin = [term_rows(t) * ncols + t.col for t in terms]
    pos = np.unique(np.concatenate(lin)) if sum(len(x) for x in lin) else np.zeros(0, dtype=np.int64)
    planes = np.zeros((len(terms), len(pos)), dtype=np.complex128)
    for l, t in enumerate(terms):
        np.add.at(planes[l], np.searchsorted(pos, lin[l]), t.vals)
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(pos // ncols, minlength=n)))).astype(np.int64)
    return rowptr, (pos % ncols).astype(np.int64), planes


def _coeffs(rng, count, cplx=False):
    c = rng.uniform(0.3, 2.0, count) * rng.choice([-1.0, 1.0], count)
    if cplx:
        c = c + 1j * rng.uniform(0.3, 2.0, count) * rng.choice([-1.0, 1.0], count)
    return np.asarray(c, dtype=np.complex128)


def move_list(L, ncoeffs, seed):
    """The fixed list of moves, [(kind, argument)] with kind "c" (set_coeffs) or "s" (set_scale): real coefficients; the last one
    changed; one coefficient of a term of index >= 32 changed (where there is one); scale 0.5, -2, 1; complex coefficients; a
    complex scale; scale 1 again (complex coefficients at scale 1: exact); real coefficients.  No "c" move without coefficients."""
    rng = np.random.default_rng(seed)
    moves = []
    drift = L - ncoeffs
    if ncoeffs:
        c1 = _coeffs(rng, ncoeffs)
        moves.append(("c", c1))
        c2 = c1.copy()
        c2[-1] = -0.625 * c2[-1] + 0.25
        moves.append(("c", c2))
        high = [j for j in range(ncoeffs - 1) if drift + j >= R.CHUNK]
        if high:
            c3 = c2.copy()
            c3[high[len(high) // 2]] *= -1.75
            moves.append(("c", c3))
    moves += [("s", 0.5), ("s", -2.0), ("s", 1.0)]
    if ncoeffs:
        moves.append(("c", _coeffs(rng, ncoeffs, cplx=True)))
    moves += [("s", COMPLEX_SCALE), ("s", 1.0)]
    if ncoeffs:
        moves.append(("c", _coeffs(rng, ncoeffs)))
    return moves


def states(ncoeffs, moves):
    """[(label, coeffs, scale)] after each move, from the library's initial state (coefficients 1, scale 1)"""
    coeffs, scale = np.ones(ncoeffs, dtype=np.complex128), 1.0 + 0.0j
    out = []
    for i, (kind, arg) in enumerate(moves):
        if kind == "c":
            coeffs = np.asarray(arg, dtype=np.complex128)
        else:
            scale = complex(arg)
        out.append((f"move {i} {kind}", coeffs.copy(), scale))
    return out


def all_real(coeffs, scale):
    return bool(complex(scale).imag == 0.0 and np.all(np.asarray(coeffs).imag == 0.0))


@dataclasses.dataclass
class Case:
    name: str
    L: int
    ncoeffs: int
    real: bool
    n: int
    terms: list
    rowptr: np.ndarray
    col: np.ndarray
    planes: np.ndarray
    moves: list

    @property
    def seed(self):
        return zlib.crc32(self.name.encode())

    @property
    def rows(self):
        return np.repeat(np.arange(self.n), np.diff(self.rowptr))

    def sample(self):
        return R.sample_positions(self.planes, self.rows >> 6, self.seed)

    def states(self):
        return states(self.ncoeffs, self.moves)


def _name(L, real, split=None):
    return (split if split else f"L{L}") + ("-real" if real else "")


BUILDERS = {}
for _L in TERM_COUNTS:
    BUILDERS[_name(_L, False)] = (_L, _L - 1, False)
for _split, (_L, _nc) in SPLITS.items():
    BUILDERS[_name(_L, False, _split)] = (_L, _nc, False)
for _L in (33, 65):
    BUILDERS[_name(_L, True)] = (_L, _L - 1, True)
CASE_NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    L, ncoeffs, real = BUILDERS[name]
    seed = zlib.crc32(name.encode())
    terms = build_terms(L, real, seed)
    rowptr, col, planes = union_planes(terms, N)
    c = Case(name, L, ncoeffs, real, N, terms, rowptr, col, planes, move_list(L, ncoeffs, seed + 1))
    assert planes.shape[0] == L and (not real or np.all(planes.imag == 0))
    assert L < 3 or not np.any(planes[1])
    assert L < 2 or np.array_equal(planes[0] != 0, planes[-1] != 0)
    return c
