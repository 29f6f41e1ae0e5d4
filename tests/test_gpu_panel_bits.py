"""The batched panel kernels on the shared panel row sum (csrc/panel_rowsum.h: csr_spmm_kernel<8 | 16>, spmm_rows_smem_kernel and the
tile kernel's rest rows, spmm_rows_kernel<1, 2, 4, 8>, and the group primitive under spmm_tile_kernel's skeleton, all in
csrc/kernels_spmm.hip) give the bits they gave before the header existed: SHA-256 digests of panels after one batched Chebyshev step
on exact inputs (tests/exact_inputs.py), recorded from the build of the commit before it, in tests/golden/panel_bits_parent.json.
Nothing here writes that file.  tests/test_gpu_panel_irregular.py holds the kernels against each other; this file holds all of them
against the parent, which a change that moves them together does not pass.

Values and states are 31-bit integers scaled by a power of two: a product of two does not fit a double, so every complex FMA rounds,
and a wrong operand, a skipped entry, another order of the entries or another pairing of the two partial sums changes the digest.
The scale keeps every row's absolute sum below 1 (asserted), so with the window (Delta, E_min) = (4, -2) the terms stay bounded;
every output is asserted finite.  The Chebyshev coefficients come from the host (Bessel functions): their digest is recorded too
and asserted first, so a changed host routine reads as such and not as a kernel change.  dt = 2.75 gives an even (24), dt = 2.5 an odd
number (23) of coefficients.  Every case asserts from Op.spmm_tiles(b) / Op.spmm_walk(b) and the launch statistics (one launch and
one mat-vec per term with the panel's byte count, besides the gather of the CSR-ordered mirror in an operator's first step nothing
else) that the kernel it is about ran.

Irregular operator: N = 269 (prime), row i with LENS[i % 39] entries at columns (7 i + 53 j + 11) mod N (distinct: 53 is invertible
mod 269 and 131 < 269); LENS = 0 .. 25, 31, 32, 33, 63 .. 67, 127 .. 131: no entries, fewer than four, every remainder after groups of
eight and four, one full 64-entry chunk of the lane-per-entry kernel, one and two reloads.  N mod 8 = 5: the last wavefront of the
RW = 2, 4, 8 instances is partly filled.  In CSR and RBCSR format (the panel reads the CSR-ordered mirror of either).  Panels of
b = 3 (TS = 8), 9 (TS = 16, one partly filled tile), 17 (two state tiles), 64 (one slice), 65 (two slices, one state in the second).
One digest per (format, b, parity) from spmm_rows = 0, spmm_nt = 0; spmm_nt = 2 and, for b > 32, spmm_rows = 1 with spmm_rw in
{0, 1, 2, 4, 8} and spmm_nt in {0, 2} must give the same.

Tile kernel: open-boundary lattices of N = 4196 rows (4096 is the plan's floor; + 100: a ragged last strip step), B + B^H with B
holding the upper offsets (exactly Hermitian: tests/test_gpu_rowblock_bits.py scattered_hermitian()), without and with an exact real
diagonal: 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17 entries per interior row -- every branch of the tile kernel's 24-entry skeleton
(fewer than four entries, one group of four, 4 + 1 .. 3, one and two groups of eight, 8 + 4, each of those + 1).  b = 64 and 70,
spmm_rw = -1, spmm_strip = 0; taken == 1 and rest_rows > 0 (the edge rows run the scalar-entry row code inside the tile launch);
spmm_rw = 0 (the row kernel alone) must give the same digest."""
import contextlib
import functools
import json
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qprop_amd.lib as L  # noqa: E402
from exact_inputs import cmat, digest, seq  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(ROOT, "tests", "golden", "panel_bits_parent.json")
DELTA, E_MIN = 4.0, -2.0
DTS = {"even": 2.75, "odd": 2.5}      # 24 and 23 coefficients
KNOBS = ("spmm_rows", "spmm_rw", "spmm_strip", "spmm_nt")

N_IRR = 269
LENS = tuple(range(26)) + (31, 32, 33) + tuple(range(63, 68)) + tuple(range(127, 132))
FORMATS = {"csr": L.FMT_CSR, "rbcsr": L.FMT_RBCSR}
BATCHES = (3, 9, 17, 64, 65)

N_LAT = 4096 + 100
LATTICES = {      # name -> (upper offsets, exact real diagonal, entries of an interior row)
    "2": ((64,), False, 2), "3": ((64,), True, 3),
    "4": ((64, 128), False, 4), "5": ((1, 64), True, 5),
    "6": ((1, 2, 64), False, 6), "7": ((1, 2, 64), True, 7),
    "8": ((1, 2, 64, 128), False, 8), "9": ((1, 2, 64, 128), True, 9),
    "12": ((1, 2, 3, 4, 64, 128), False, 12), "13": ((1, 2, 3, 4, 64, 128), True, 13),
    "16": ((1, 2, 3, 4, 64, 128, 192, 256), False, 16), "17": ((1, 2, 3, 4, 64, 128, 192, 256), True, 17),
}
LATTICE_BATCHES = (64, 70)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


@contextlib.contextmanager
def knobs(ctx, **kw):
    saved = {k: ctx.tuning_get(k) for k in kw}
    try:
        for k, v in kw.items():
            ctx.tuning_set(k, v)
        yield
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def _assert_rows_below_one(H):
    rows = np.asarray(abs(H).sum(axis=1)).ravel()
    assert rows.max() < 1.0, rows.max()


@functools.lru_cache(maxsize=None)
def irregular():
    """|component| < 2^-9, at most 131 entries per row: absolute row sums below 131 sqrt(2) / 512 < 0.37"""
    assert len(LENS) == 39 and len(set(LENS)) == 39
    lens = [LENS[i % 39] for i in range(N_IRR)]
    cols = [np.sort((7 * i + 53 * np.arange(n) + 11) % N_IRR) for i, n in enumerate(lens)]
    assert all(len(np.unique(c)) == len(c) for c in cols)
    rp = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    vals = cmat(1, int(rp[-1]), 211, 39).reshape(-1)
    H = sp.csr_matrix((vals, np.concatenate(cols).astype(np.int32), rp), shape=(N_IRR, N_IRR))
    assert sorted(set(np.diff(H.indptr).tolist())) == sorted(LENS) and H.nnz == int(rp[-1])
    _assert_rows_below_one(H)
    return H


@functools.lru_cache(maxsize=None)
def lattice(name):
    """B + B^H (+ D): B[i, i + d] for the upper offsets d and i + d < N (open boundaries), |component| < 2^-5, at most 17 entries
    per row: absolute row sums below 17 sqrt(2) / 32 < 0.76"""
    offsets, diag, per_row = LATTICES[name]
    n = N_LAT
    B = sp.csr_matrix((n, n), dtype=np.complex128)
    for t, d in enumerate(offsets):
        B = B + sp.diags([cmat(1, n - d, 223 + 17 * t + d, 35).reshape(-1)], [d], shape=(n, n), format="csr")
    H = B + B.getH()
    if diag:
        H = H + sp.diags([np.ldexp(seq(n, 229), -35).astype(np.complex128)], [0], shape=(n, n), format="csr")
    H = sp.csr_matrix(H)
    H.sum_duplicates()
    H.sort_indices()
    assert abs(H - H.getH()).max() == 0.0 and np.diff(H.indptr)[n // 2] == per_row == np.diff(H.indptr).max()
    _assert_rows_below_one(H)
    return H


@functools.lru_cache(maxsize=None)
def panel(n, b):
    """exact panel [n, b] whose columns have norms of order one (a power-of-two scale: no library norm on the way)"""
    return cmat(n, b, 5 + n + b, 30 + int(round(np.log2(2 * n / 3) / 2)))


def coeffs_digest(c):
    return digest(np.asarray(c, dtype=np.float64).astype(np.complex128))


# ---- one step ---------------------------------------------------------------------------------------------------------------

def step_bits(ctx, Op, b, parity, want_tiles, **kn):
    """digest of the panel after one batched step under the given knobs, and the digest of the step's coefficients"""
    n, dt = Op.nrows, DTS[parity]
    with knobs(ctx, **kn):
        wrk = L.ChebyWrk(ctx, n * b, DELTA, E_MIN, dt)
        assert wrk.n_coeffs == {"even": 24, "odd": 23}[parity], wrk.n_coeffs
        assert np.array_equal(wrk.coeffs[:wrk.n_coeffs], L.cheby_coeffs(DELTA, dt))
        ti = Op.spmm_tiles(b)
        assert ti["taken"] == want_tiles, (kn, ti)
        if want_tiles:
            assert ti["rest_rows"] > 0 and ti["tiles"] * 16 + ti["rest_rows"] == n, ti
        else:
            assert Op.spmm_walk(b) == (0, 0), (kn, Op.spmm_walk(b))
        psi = L.State(ctx, data=np.ascontiguousarray(panel(n, b)).reshape(-1))
        ctx.reset_stats()
        L.cheby_batched(psi, Op, dt, wrk, b)
        st = ctx.stats()
        # one launch per term (+ the gather of the CSR-ordered mirror in the operator's first step), each counted as one mat-vec
        # of a panel: 20 bytes per entry, the row pointers, 80 bytes per element of the panel
        nterms = wrk.n_coeffs - 1
        assert st["n_matvec"] == nterms and st["n_kernel_launches"] in (nterms, nterms + 1), (kn, st)
        assert np.isclose(st["spmv_bytes"], nterms * (20.0 * Op.nnz + 4.0 * (n + 1) + 80.0 * n * b), rtol=1e-12, atol=0), (kn, st)
        out = psi.numpy()
        cd = coeffs_digest(wrk.coeffs[:wrk.n_coeffs])
        psi.close()
        wrk.close()
    assert np.all(np.isfinite(out.view(np.float64)))
    return digest(out), cd


def case_irregular(ctx, fmt, b, parity):
    """-> (digest of the state-tiled kernel, digest of the coefficients); every other variant asserted equal to the first"""
    H = irregular()
    with knobs(ctx, **{k: ctx.tuning_get(k) for k in KNOBS}):
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)], 0, FORMATS[fmt])
        assert Op.format == FORMATS[fmt] and Op.nrows == N_IRR and N_IRR % 8 == 5
        ref, cd = step_bits(ctx, Op, b, parity, 0, spmm_rows=0, spmm_nt=0)
        variants = [dict(spmm_rows=0, spmm_nt=2)]
        if b > 32:
            variants += [dict(spmm_rows=1, spmm_rw=rw, spmm_nt=nt) for rw in (0, 1, 2, 4, 8) for nt in (0, 2)]
        for kn in variants:
            got, _ = step_bits(ctx, Op, b, parity, 0, **kn)
            assert got == ref, (fmt, b, parity, kn)
        Op.close()
    return {"panel": ref, "coeffs": cd}


def case_lattice(ctx, name, b):
    """-> digests of one step at the even and at the odd term count through the tile kernel; the row kernel alone asserted equal"""
    H = lattice(name)
    out = {}
    with knobs(ctx, **{k: ctx.tuning_get(k) for k in KNOBS}):
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)])
        for parity in DTS:
            tiles, cd = step_bits(ctx, Op, b, parity, 1, spmm_rows=1, spmm_rw=-1, spmm_strip=0, spmm_nt=0)
            rows, _ = step_bits(ctx, Op, b, parity, 0, spmm_rows=1, spmm_rw=0, spmm_strip=-1, spmm_nt=0)
            assert rows == tiles, (name, b, parity)
            out[parity] = {"panel": tiles, "coeffs": cd}
        Op.close()
    return out


# name in the fixture -> (case function, arguments)
CASES = {}
CASES.update({f"irregular-{f}-b{b}-{p}": (case_irregular, (f, b, p)) for f in FORMATS for b in BATCHES for p in DTS})
CASES.update({f"lattice-{name}-b{b}": (case_lattice, (name, b)) for name in LATTICES for b in LATTICE_BATCHES})


def _check(got, want):
    for g, w in ((got, want),) if "coeffs" in got else ((got[p], want[p]) for p in DTS):
        assert g["coeffs"] == w["coeffs"], "the host's Chebyshev coefficients changed, not (only) a kernel"
        assert g["panel"] == w["panel"]


@pytest.mark.parametrize("parity", list(DTS))
@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_panel_row_kernels_bits(ctx, parent, fmt, b, parity):
    _check(case_irregular(ctx, fmt, b, parity), parent["cases"][f"irregular-{fmt}-b{b}-{parity}"])


@pytest.mark.parametrize("b", LATTICE_BATCHES)
@pytest.mark.parametrize("name", list(LATTICES))
def test_panel_tile_kernel_bits(ctx, parent, name, b):
    _check(case_lattice(ctx, name, b), parent["cases"][f"lattice-{name}-b{b}"])
