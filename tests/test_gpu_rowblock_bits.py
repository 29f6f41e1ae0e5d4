"""The row-block mat-vec family on the shared row-sum core (csrc/rowblock_sum.h: rbcsr_spmv_kernel and the upper section of
hrb_spmv_kernel in csrc/kernels.hip, rbcsr_coded_spmv_kernel, arnoldi_matvec_dots_kernel, and the reduction of
arnoldi_onepass_kernel) gives the bits it gave before the core existed: SHA-256 digests of outputs on exact inputs
(tests/exact_inputs.py), recorded from the build of the commit before it, in tests/golden/rowblock_bits_parent.json.  Nothing
here writes that file.

Values and vectors are 31-bit integers scaled by a power of two: a product of two does not fit a double, so every complex FMA
rounds, and a wrong operand, a skipped quad, another summation order or another pairing of the two partial sums changes the
digest.  Every case first asserts, from the statistics and the information getters, that the kernel it is about ran:
small_nnz = 0 keeps the persistent small-system kernels away, colblock = 0 the column-blocked mirror, hrb_walk = 0 the strip walk.

Shapes: the smallest that reach each branch of the shared code.
  rbcsr      n = 337 (row blocks of 1, 2, 3, 5, 5 quads and a last one of 17 rows with 4; odd and even quad counts against unroll
             2 and 4), complex and all-real (`double` instance); every column is within 32767 of its row, so these sections are int16
             deltas -- n = 70001 with columns 33000 and more away has the int32 sections; a band of 12 entries per row, n = 576:
             int16 / stencil sections, and stored > 512 blocks, so the plain Chebyshev term runs eight row blocks per workgroup.
             mul! in both forms, a Chebyshev step without and with the normalisation check, all of them for all eight values
             of rbcsr_variant & 7 on every one of these operators: one digest per output.
  hrb        a scattered Hermitian operator, n = 337 (lower sections by position), and a lattice of twelve offsets on 43 blocks
             and 17 rows (three quads per section: lower_stencil() and the shared upper loop, not the straight-line path);
             variants 0-8, 15, 31: one digest per output.
  coded      a 9-spin transverse-field chain with uniform couplings (tables shorter than 64 entries), with site-dependent dyadic
             couplings (a table of more than 64 entries: the second guarded copy of the staging), with a sigma_y term (complex table).
  arnoldi    arnoldi! with m = 20 (every JT instance in one sweep): n = 337 complex and real, the non-uniform chain (CODED), a
             band of 8 entries per row on n = 131072 + 197 (two rounds, idle wavefronts in the second, nontemporal loads).
  onepass    newton! with arnoldi_onepass = 2, m_max = 4, 8, 12, 16, 20 (eight wavefronts; two blocks in flight; one), on n = 337
             and on n = 3 * 65536 - 37 (three rounds of four wavefronts: the second block of the last pair inactive, the last
             block partly filled).  newton! hands out neither the Hessenberg matrix nor the basis: the state (a combination of
             every basis vector with coefficients computed from the Hessenberg matrix), the Newton coefficients and the Leja
             points (functions of the Hessenberg matrix alone) are digested in their place.
"""
import contextlib
import functools
import hashlib
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
import qprop_amd.synth as synth  # noqa: E402
from exact_inputs import cmat, digest  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(ROOT, "tests", "golden", "rowblock_bits_parent.json")
KEEP_AWAY = {"small_nnz": 0, "colblock": 0, "cheby_graph": 0}


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


# ---- operators -------------------------------------------------------------------------------------------------------------

def _csr(n, cols, seed, shift, real=False):
    """scipy CSR with the given columns per row (a list of int arrays, or rows x k) and exact values"""
    if isinstance(cols, np.ndarray):
        rp = np.arange(n + 1, dtype=np.int64) * cols.shape[1]
        col = np.sort(cols, axis=1).reshape(-1).astype(np.int32)
    else:
        rp = np.concatenate(([0], np.cumsum([len(c) for c in cols]))).astype(np.int64)
        col = np.concatenate([np.sort(c) for c in cols]).astype(np.int32)
    vals = cmat(1, int(rp[-1]), seed, shift, real=real).reshape(-1)
    return sp.csr_matrix((vals, col, rp), shape=(n, n))


@functools.lru_cache(maxsize=None)
def scattered(real=False):
    """n = 337 = 5 * 64 + 17, rows of block b with exactly (4, 8, 12, 20, 20, 16)[b] entries at scattered columns (337 is prime:
    53 j runs through distinct residues): blocks of 1, 2, 3, 5, 5 quads and the partly filled one of 4.  |entry| < 2^-4 per
    component: norm below 4."""
    n = 337
    cols = [(7 * i + 53 * np.arange((4, 8, 12, 20, 20, 16)[i // 64]) + 11) % n for i in range(n)]
    return _csr(n, cols, 101, 34, real=real)


def far_columns(n=70001):
    """eight entries per row, 33000 + 1111 j + 97 (i (j + 1) mod 13) rows away (mod n): distinct, no int16 delta reaches the first
    of them, and the distance changes from row to row (no stencil, no block map)"""
    i, j = np.arange(n, dtype=np.int64)[:, None], np.arange(8, dtype=np.int64)[None, :]
    return _csr(n, (i + 33000 + 1111 * j + 97 * ((i * (j + 1)) % 13)) % n, 103, 33)


@functools.lru_cache(maxsize=None)
def banded(n, k, seed):
    """k entries per row at distances -k / 2 .. k / 2 - 1 (mod n)"""
    return _csr(n, (np.arange(n, dtype=np.int64)[:, None] + (np.arange(k) - k // 2)[None, :]) % n, seed, 33)


def scattered_hermitian():
    """B + B^H with four scattered entries per row of B, n = 337: exactly Hermitian (the sums of two 31-bit integers are exact)"""
    n = 337
    B = _csr(n, [(5 * i + 71 * np.arange(4) + 3) % n for i in range(n)], 107, 34)
    H = (B + B.getH()).tocsr()
    H.sum_duplicates()
    H.sort_indices()
    return H


LATTICE_N = 43 * 64 + 17
LATTICE_OFFSETS = (1, 2, 3, 4, 5, 6, 16, 32, 48, 64, 80, 96)


def spin_chain(J, hz, h, hy=None):
    """Transverse-field chain of len(h) spins (open ends) with couplings per site: H = -sum J_i sz_i sz_i+1 - sum hz_i sz_i
    - sum h_i sx_i - sum hy_i sy_i (synth.tfim_csr with arrays for numbers, and the sigma_y term)."""
    n = len(h)
    N = 1 << n
    r = np.arange(N, dtype=np.int64)
    s = 1.0 - 2.0 * ((r[:, None] >> np.arange(n)[None, :]) & 1)
    diag = -(s[:, :-1] * s[:, 1:]) @ np.asarray(J, dtype=float) - s @ np.asarray(hz, dtype=float)
    rows = np.repeat(r, n + 1)
    cols = np.concatenate([r[:, None] ^ (1 << np.arange(n))[None, :], r[:, None]], axis=1).reshape(-1)
    flip = -np.asarray(h, dtype=float)[None, :] + 0j * s
    if hy is not None:
        flip = flip - 1j * np.asarray(hy, dtype=float)[None, :] * s       # <0|sy|1> = -i, <1|sy|0> = +i
    vals = np.concatenate([flip, diag[:, None].astype(complex)], axis=1).reshape(-1)
    H = sp.coo_matrix((vals, (rows, cols)), shape=(N, N)).tocsr()
    H.sort_indices()
    return H


# dyadic: the bond terms are multiples of 1 / 16, the fields odd multiples of 2^-14 below 1 / 32 in sum: the 64 rows of a block have
# 64 different diagonal energies, and with the nine flip amplitudes the block's table has 73 entries (+ the zero of the padding)
SITES = np.arange(9)
CHAINS = {
    "uniform": dict(J=np.ones(8), hz=np.full(9, 0.125), h=np.ones(9)),
    "dyadic": dict(J=(SITES[:8] + 8) / 16.0, hz=2.0 ** -(SITES + 6.0), h=(SITES + 3) / 16.0),
    "sigma_y": dict(J=(SITES[:8] + 8) / 16.0, hz=2.0 ** -(SITES + 6.0), h=(SITES + 3) / 16.0, hy=(SITES + 1) / 32.0),
}


def _chain_bound(c):
    return float(sum(np.abs(np.asarray(v)).sum() for v in c.values()))


def _largest_table(H):
    """distinct stored values of the fullest 64-row block"""
    return max(len(np.unique(H.data[H.indptr[b]:H.indptr[min(b + 64, H.shape[0])]])) for b in range(0, H.shape[0], 64))


def _operator(ctx, H, fmt, value_dict=0):
    with knobs(ctx, value_dict=value_dict):
        return L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)], 0, fmt)


def _state(n, seed, shift=None):
    """exact vector with a norm of order one (a power-of-two scale: no library norm on the way)"""
    if shift is None:
        shift = 30 + int(round(np.log2(2 * n / 3) / 2))
    return cmat(n, 1, seed, shift).reshape(-1)


# ---- outputs ----------------------------------------------------------------------------------------------------------------

def matvec_bits(ctx, op, window, dt, variants=(None,)):
    """digests of mul! (3 and 5 arguments), a Chebyshev step without and with the normalisation check, each the same for every
    value of rbcsr_variant in `variants`"""
    n = op.nrows
    x, y0, psi0 = _state(n, 5 + n), _state(n, 3 + n), _state(n, 7 + n)
    wrk = L.ChebyWrk(ctx, n, window[0], window[1], dt)
    assert 4 <= wrk.n_coeffs <= 24
    out = None
    for v in variants:
        with knobs(ctx, **({} if v is None else {"rbcsr_variant": v})):
            xs, ys = L.State(ctx, data=x), L.State(ctx, n=n)
            ctx.reset_stats()
            op.mul(xs, ys)
            got = {"mul3": digest(ys.numpy())}
            ys.upload(y0)
            op.mul(xs, ys, 0.75 - 0.25j, -0.375 + 0.125j)
            got["mul5"] = digest(ys.numpy())
            assert ctx.stats()["n_kernel_launches"] == 2 and ctx.stats()["n_matvec"] == 2, ctx.stats()
            for name, check in (("step", False), ("step_checked", True)):
                psi = L.State(ctx, data=psi0)
                ctx.reset_stats()
                L.cheby(psi, op, dt, wrk, check_normalization=check)
                assert ctx.stats()["n_matvec"] == wrk.n_coeffs - 1, ctx.stats()
                got[name] = digest(psi.numpy())
        assert out is None or got == out, (v, got, out)
        out = got
    return out


def arnoldi_bits(ctx, op, m=20, dt=0.5):
    """digests of the Hessenberg matrix and the basis of arnoldi! with m columns through the fused mat-vec + dot products"""
    n = op.nrows
    with knobs(ctx, arnoldi_mode=1, arnoldi_fuse_dots=1, arnoldi_onepass=0):
        q = L.Krylov(ctx, n, m + 1)
        Hess = np.zeros((m + 1, m + 1), dtype=complex, order="F")
        ctx.reset_stats()
        m_out = L.arnoldi(Hess, q, m, L.State(ctx, data=_state(n, 9 + n)), op, dt)
        st = ctx.stats()
        # two launches per column (mat-vec with the dot products, projection) and the norm of the last vector; with a separate
        # multidot launch it would be three per column
        assert m_out == m and st["n_matvec"] == m and 2 * m <= st["n_kernel_launches"] <= 2 * m + 2, (m_out, st)
        h = hashlib.sha256()
        for i in range(m + 1):
            h.update(np.ascontiguousarray(q.vec(i), dtype=np.complex128).tobytes())
        q.close()
        return {"hess": digest(Hess), "basis": h.hexdigest()}


def onepass_bits(ctx, op, m, dt=0.5):
    """digests after one newton! step through the one-pass sweep (tests/test_gpu_onepass.py: the same entry point, the same
    bound on the launches)"""
    n = op.nrows
    with knobs(ctx, arnoldi_onepass=2, arnoldi_mode=1):
        wrk = L.NewtonWrk(ctx, n, m_max=m)
        psi = L.State(ctx, data=_state(n, 13 + n))
        ctx.reset_stats()
        L.newton(psi, op, dt, wrk)
        sweeps = wrk.restarts + 1
        assert wrk.stats["sweeps_onepass"] == sweeps and wrk.stats["sweeps_onepass_redone"] == 0, wrk.stats
        assert wrk.stats["n_matvec"] >= m, wrk.stats
        assert ctx.stats()["n_kernel_launches"] <= 2 * (wrk.stats["n_matvec"] + sweeps) + 3 * sweeps + 2, ctx.stats()
        a, leja = wrk.coeffs()
        out = {"state": digest(psi.numpy()), "newton_coeffs": digest(a), "leja": digest(leja), "restarts": wrk.restarts}
        wrk.close()
        return out


# ---- cases ------------------------------------------------------------------------------------------------------------------

def _plain_rbcsr(ctx, H):
    op = _operator(ctx, H, L.FMT_RBCSR)
    assert op.format == L.FMT_RBCSR and op.value_encoding_info()["valid"] == 0 and op.colblock_info()["valid"] == 0
    return op


def case_rbcsr(ctx, which):
    with knobs(ctx, **KEEP_AWAY):
        if which == "far":
            op = _plain_rbcsr(ctx, far_columns())
            assert op.encoding_info()["upper"]["int32"] == op.layout_info()["blocks"]
            return matvec_bits(ctx, op, (8.0, -4.0), 0.5, variants=range(8))
        if which == "band":
            op = _plain_rbcsr(ctx, banded(576, 12, 109))
            lay = op.layout_info()
            assert lay["stored"] > 512 * lay["blocks"]            # the plain term runs eight row blocks per workgroup
            assert op.encoding_info()["upper"]["int32"] == 0
            return matvec_bits(ctx, op, (8.0, -4.0), 0.5, variants=range(8))
        op = _plain_rbcsr(ctx, scattered(real=which == "real"))
        lay = op.layout_info()
        assert lay["blocks"] == 6 and lay["stored"] == 256 * (1 + 2 + 3 + 5 + 5 + 4) + 64      # (+ a block of slack)
        return matvec_bits(ctx, op, (8.0, -4.0), 0.5, variants=range(8))


def case_hrb(ctx, which):
    with knobs(ctx, hrb_walk=0, **KEEP_AWAY):
        if which == "scattered":
            op = _operator(ctx, scattered_hermitian(), L.FMT_HRB)
            assert op.encoding_info()["lower"]["stencil"] == 0       # lower sections by position
            window = (8.0, -4.0)
        else:
            rp, col, vals = synth.hermitian_offsets_csr(LATTICE_N, offsets=LATTICE_OFFSETS)
            op = L.Operator(ctx, [L.Matrix(ctx, LATTICE_N, LATTICE_N, rp, col, vals)], 0, L.FMT_HRB)
            lay = op.layout_info()
            assert lay["blocks"] == 44 and min(lay["stencil_lower_blocks"], lay["stencil_upper_blocks"]) > 0.75 * lay["blocks"]
            # quads of every block's sections, from the pattern: three and three away from the wrap-around, no block with the two
            # and two of the straight-line path; the stored slots say that the layout has exactly these upper widths
            c2, rows = col.reshape(LATTICE_N, -1), np.arange(LATTICE_N)[:, None]
            uq, lq = ([-(-int(n[b:b + 64].max()) // 4) for b in range(0, LATTICE_N, 64)] for n in ((c2 > rows).sum(axis=1), (c2 < rows).sum(axis=1)))
            assert sum(u == 3 and lo == 3 for u, lo in zip(uq, lq)) >= 36 and (2, 2) not in zip(uq, lq), (uq, lq)
            assert lay["stored"] == 256 * sum(uq) + 64, (lay, uq)
            window = (20.0, -10.0)
        assert op.format == L.FMT_HRB
        assert op.walk_reason()[1] != "ok", op.walk_reason()       # hrb_walk = 0: the per-block kernel, not the strip walk
        return matvec_bits(ctx, op, window, 0.2, variants=(0, 1, 2, 3, 4, 5, 6, 7, 8, 15, 31))


def _coded_chain(ctx, which):
    H = spin_chain(**CHAINS[which])
    op = _operator(ctx, H, L.FMT_RBCSR, value_dict=1)
    info = op.value_encoding_info()
    assert op.format == L.FMT_RBCSR and info["valid"] == 1 and op.colblock_info()["valid"] == 0, info
    longest = _largest_table(H)      # (+ the zero of the padding slots: ten entries per row in twelve slots)
    assert (longest + 1 < 64) if which == "uniform" else (longest > 64), longest
    return op


def case_coded(ctx, which):
    with knobs(ctx, value_dict=1, **KEEP_AWAY):
        op = _coded_chain(ctx, which)
        b = _chain_bound(CHAINS[which])
        return matvec_bits(ctx, op, (2.2 * b, -1.1 * b), 2.0 / b)


def case_arnoldi(ctx, which):
    with knobs(ctx, value_dict=1 if which == "coded" else 0, **KEEP_AWAY):
        if which == "coded":
            op = _coded_chain(ctx, "dyadic")
        elif which == "two_rounds":
            op = _plain_rbcsr(ctx, banded(131072 + 197, 8, 113))
            assert op.layout_info()["stored"] * 16 > 8 * 1024 * 1024          # nontemporal matrix loads
        else:
            op = _plain_rbcsr(ctx, scattered(real=which == "real"))
        return arnoldi_bits(ctx, op)


ONEPASS_BIG_N = 3 * 65536 - 37


def case_onepass(ctx, which, m):
    with knobs(ctx, **KEEP_AWAY):
        if which == "three_rounds":
            op = _plain_rbcsr(ctx, banded(ONEPASS_BIG_N, 8, 127))
        else:
            op = _plain_rbcsr(ctx, scattered(real=which == "real"))
        return onepass_bits(ctx, op, m)


RBCSR = ["complex", "real", "far", "band"]
HRB = ["scattered", "lattice"]
CODED = ["uniform", "dyadic", "sigma_y"]
ARNOLDI = ["complex", "real", "coded", "two_rounds"]
ONEPASS = [("complex", m) for m in (4, 8, 12, 16, 20)] + [("three_rounds", m) for m in (4, 8, 12, 16, 20)] + [("real", 12)]

# name in the fixture -> (case function, arguments)
CASES = {}
CASES.update({f"rbcsr-{w}": (case_rbcsr, (w,)) for w in RBCSR})
CASES.update({f"hrb-{w}": (case_hrb, (w,)) for w in HRB})
CASES.update({f"coded-{w}": (case_coded, (w,)) for w in CODED})
CASES.update({f"arnoldi-{w}": (case_arnoldi, (w,)) for w in ARNOLDI})
CASES.update({f"onepass-{w}-m{m}": (case_onepass, (w, m)) for w, m in ONEPASS})


@pytest.mark.parametrize("which", RBCSR)
def test_rbcsr_spmv_bits(ctx, parent, which):
    assert case_rbcsr(ctx, which) == parent["cases"][f"rbcsr-{which}"]


@pytest.mark.parametrize("which", HRB)
def test_hrb_spmv_bits(ctx, parent, which):
    assert case_hrb(ctx, which) == parent["cases"][f"hrb-{which}"]


@pytest.mark.parametrize("which", CODED)
def test_rbcsr_coded_spmv_bits(ctx, parent, which):
    assert case_coded(ctx, which) == parent["cases"][f"coded-{which}"]


@pytest.mark.parametrize("which", ARNOLDI)
def test_arnoldi_matvec_dots_bits(ctx, parent, which):
    assert case_arnoldi(ctx, which) == parent["cases"][f"arnoldi-{which}"]


@pytest.mark.parametrize("which,m", ONEPASS)
def test_arnoldi_onepass_bits(ctx, parent, which, m):
    assert case_onepass(ctx, which, m) == parent["cases"][f"onepass-{which}-m{m}"]
