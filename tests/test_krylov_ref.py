"""The reference of tests/test_gpu_krylov_columns.py checked on the host (tests/krylov_ref.py): a float64 emulation of the
low-synchronisation Gram-Schmidt step stays under the derived bounds on every family of bases the GPU tests use, each planted defect
exceeds them by at least 10^3 on the same inputs -- so the GPU tests would notice a kernel that has it --, the recurrence agrees
with the oracle's Arnoldi column, and the banded operator's sliced product agrees with its CSR."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import qp_oracle as qo  # noqa: E402
import krylov_ref as kr  # noqa: E402

# every (n, J, delta) family of the GPU tests: the building blocks' cases, the engine column's (the longest basis per size: the
# shorter ones are leading blocks of the same construction)
FAMILIES = sorted(set(kr.BLOCK_CASES) | {(kr.COLUMN_N, J) for J in kr.COLUMN_J} | {(n, max(kr.SIZE_J)) for n in kr.COLUMN_SIZES})
# (the defects in the Gram term need a Gram row above the last one; at n = 1 the vector is zero after the first projection)
DEFECT_FAMILIES = [(n, J) for n, J in FAMILIES if n >= 257 and J >= 2]


def _inputs(n, J):
    V = kr.make_basis(n, J, kr.delta_for(J), seed=100 + J)
    return V, kr.make_vector(V, seed=200 + J)


def _worst(col, result):
    red, h, out = result
    return col.ratio_dots(red), col.ratio_coefs(h), col.ratio_vector(out)


@pytest.mark.parametrize("n,J", FAMILIES)
def test_emulation_stays_under_the_bounds_and_every_defect_exceeds_them(n, J):
    V, w = _inputs(n, J)
    col = kr.Column(V, w)
    if n >= 257 and J >= 1:      # the construction: unit vectors, Gram entries of the size the basis was built for
        off = col.absG - np.diag(np.diag(col.absG))
        assert abs(float(col.absG[0, 0]) - 1.0) < 1e-14 and 0.02 < float(off.max()) < 0.25, float(off.max())
        assert float((col.hb / col.cb).max()) < 5e3      # the magnitude recursion stays tame: the bound means something
    dots, coefs, vec = _worst(col, kr.lowsync_emulation(V, w))
    print(f"n={n} J={J}: clean emulation error / bound: dots {dots:.3g}, coefficients {coefs:.3g}, vector {vec:.3g}")
    assert dots <= 1.0 and coefs <= 1.0 and vec <= 1.0
    if (n, J) in DEFECT_FAMILIES:
        for defect in kr.DEFECTS:
            worst = max(_worst(col, kr.lowsync_emulation(V, w, defect)))
            print(f"    {defect}: {worst:.3g}")
            assert worst >= 1e3, (defect, worst)


def test_seam_elements_and_weight():
    assert kr.seam_elements(1) == [0] and kr.seam_elements(257) == [0, 255, 256]
    assert kr.seam_elements(131073) == [0, 255, 256, 65535, 65536, 131071, 131072]
    assert kr.seam_elements(196613)[-1] == 196612
    assert kr.seam_weight(65535) == kr.SEAM_WEIGHT and kr.seam_weight(262444) == kr.SEAM_WEIGHT
    assert 2.5 < kr.seam_weight(257) < 3.0 and 9.0 < kr.seam_weight(4197) < 11.0 and kr.seam_weight(1) == 1.0
    V = kr.make_basis(65537, 3, 0.1, seed=3)
    share = np.abs(V[:, kr.seam_elements(65537)]) ** 2 * 65537
    assert share.mean() > 300, share.mean()       # a seam element carries hundreds of times an average element's share of a dot


def test_mgs_agrees_with_the_oracles_arnoldi_column():
    """On the orthonormal basis the oracle built: dt h = Hess[0..j, j], |w_out| = Hess[j+1, j] / dt, w_out / |w_out| = q_{j+1}."""
    rng = np.random.default_rng(4)
    n, m, dt = 60, 6, 0.37
    A = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    psi = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    psi /= np.linalg.norm(psi)
    Hess = np.zeros((m + 1, m + 1), dtype=complex)
    q = [np.zeros(n, dtype=complex) for _ in range(m + 1)]
    assert qo.arnoldi(Hess, q, m, psi, A, dt=dt) == m
    for j in range(m):
        h, w_out, n2 = kr.mgs(np.array(q[: j + 1]), A @ q[j])
        assert np.abs(dt * h - Hess[: j + 1, j]).max() < 1e-13
        assert abs(dt * np.sqrt(n2) - Hess[j + 1, j]) < 1e-13
        assert np.abs(w_out / np.sqrt(n2) - q[j + 1]).max() < 1e-13


@pytest.mark.parametrize("real,few_values", [(False, False), (True, False), (False, True)])
def test_banded_operator(real, few_values):
    n = 333
    op = kr.banded(n, kr.OFFSETS, seed=9, real=real, few_values=few_values)
    A = op.csr()
    assert A.shape == (n, n) and A.nnz == sum(n - abs(d) for d in kr.OFFSETS)
    assert (A.dtype == np.float64) == real
    assert abs(A - A.conj().T).max() > 0.1                       # not Hermitian
    if few_values:
        assert len(np.unique(A.data)) == len(kr.FEW_VALUES)
    rng = np.random.default_rng(10)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    y, ya = op.apply(x), op.abs_apply(x)
    assert y.dtype == kr.CLD
    assert np.abs(y - A @ x).max() < 1e-14 and np.abs(ya - abs(A) @ np.abs(x)).max() < 1e-14
    # the double-precision product is under the row bound, and a product that misses one diagonal is far above it
    assert float((np.abs(A @ x - y) / op.row_bound(x)).max()) <= 1.0
    B = A.tolil()
    B.setdiag(0, 64)
    assert float((np.abs(B.tocsr() @ x - y) / op.row_bound(x)).max()) > 1e3
    # open boundaries: row 0 reaches only forwards, the last row only backwards
    assert list(A[0].indices) == [0, 1, 2, 64] and list(A[n - 1].indices) == [n - 201, n - 71, n - 4, n - 2, n - 1]
