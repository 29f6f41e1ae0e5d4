"""Every way an Arnoldi sweep is enqueued and collected (csrc/engine_krylov.hip: the persistent small sweep, the multi-launch sweep
plain and folded, its columns announced by the stream's end, by events or by flags, the one-pass sweep and its redo in two-pass
form), at the smallest sizes that reach each: every newton! step against the oracle to the tolerance of tests/test_gpu_parity.py,
restart counts equal.  What can go wrong here is host orchestration -- waits, the hook, the breakdown, the final drain -- not a
kernel, so the systems are tiny and the knobs are crossed."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import qp_oracle as qo  # noqa: E402
import qprop_amd.lib as L  # noqa: E402
import qprop_amd.synth as synth  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10          # tests/test_gpu_parity.py: TOL
N = 37 * 37          # 1369: no multiple of 64 -- the last row block and the last grid-stride pass of the norm kernel are partly filled
DTS = (0.5, 0.5, -0.3)
NQ = 6               # qubits of the matrix-free operator (N = 64)
LAM = np.array([-3.0, 0.5, 2.0, 7.5])


@functools.lru_cache(maxsize=None)
def _system(name):
    """(matrix for the oracle, start vector, newton! keywords); read-only, shared by all tests."""
    if name == "liouvillian":                       # (a)
        A = sp.csr_matrix(synth.liouvillian_tridiag(37))
        psi0, kw = synth.random_state(N), {}
    elif name in ("four_eigenvalues", "eigenstate"):   # (b), (c): Krylov dimension 4 / 1
        rng = np.random.default_rng(5)
        d = LAM[rng.integers(0, 4, N)]
        A = sp.diags([d], [0], format="csr", dtype=complex)
        if name == "eigenstate":
            psi0 = (d == LAM[2]).astype(complex)
        else:
            psi0 = rng.standard_normal(N) + 1j * rng.standard_normal(N)
        psi0, kw = psi0 / np.linalg.norm(psi0), {"norm_min": 1e-9}
    else:                                           # (d) "pauli": applied from its strings on the device
        rq, cq, vq = synth.tfim_csr(NQ)
        A = sp.csr_matrix((vq, cq, rq), shape=(1 << NQ, 1 << NQ))
        psi0, kw = synth.random_state(1 << NQ, seed=78), {}
    psi0.setflags(write=False)
    return A, psi0, kw


@functools.lru_cache(maxsize=None)
def _oracle(name, m_max):
    """The oracle's state and restart count after every step of DTS, computed once."""
    A, psi0, kw = _system(name)
    owrk = qo.NewtonWrk(psi0, m_max=m_max)
    ref, out = psi0.copy(), []
    for dt in DTS:
        qo.newton(ref, A, dt, owrk, **kw)
        snap = ref.copy()
        snap.setflags(write=False)
        out.append((snap, owrk.restarts))
    return tuple(out)


RUNS = (("liouvillian", 6), ("liouvillian", 12), ("four_eigenvalues", 10), ("eigenstate", 10), ("pauli", 5))


def _operator(ctx, name, fmt=L.FMT_RBCSR):
    if name == "pauli":
        return L.PauliOperator(ctx, NQ, [synth.tfim_pauli_terms(NQ)])
    A = _system(name)[0]
    return L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)], 0, fmt) if fmt is not None else L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)])


def _steps(ctx, name, m_max, op=None):
    """newton! over DTS against the oracle after every step; returns per step (n_matvec of the context, statistics of the step)."""
    _, psi0, kw = _system(name)
    op = op if op is not None else _operator(ctx, name)
    wrk = L.NewtonWrk(ctx, len(psi0), m_max=m_max)
    psi = L.State(ctx, data=psi0)
    seen = []
    for k, (dt, (ref, restarts)) in enumerate(zip(DTS, _oracle(name, m_max))):
        ctx.reset_stats()
        L.newton(psi, op, dt, wrk, **kw)
        err = float(np.linalg.norm(psi.numpy() - ref))
        print(f"{name} m_max={m_max} step {k}: |dpsi|={err:.2e} restarts {wrk.restarts} (oracle {restarts}) {wrk.stats}")
        assert err < TOL, (name, m_max, k, err)
        assert wrk.restarts == restarts, (name, m_max, k, wrk.restarts, restarts)
        seen.append((ctx.stats()["n_matvec"], ctx.stats()["n_kernel_launches"], dict(wrk.stats)))
    return seen


@pytest.fixture()
def ctx():
    c = L.Context(0)
    yield c
    c.close()


KNOBS = ("small_nnz", "newton_pipeline", "arnoldi_mode", "arnoldi_fuse_dots", "arnoldi_onepass")


def _set(ctx, **knobs):
    for k, v in knobs.items():
        ctx.tuning_set(k, v)


# arnoldi_mode, arnoldi_fuse_dots (only the low-synchronisation sweep has the knob)
SCHEDULES = [(0, 1), (1, 0), (1, 1)]
# 0: never, 2: always, 3: always, and every one-pass sweep is done again in the two-pass form (the redo path of a norm drift, forced)
ONEPASS = [0, 2, 3]


@pytest.mark.parametrize("onepass", ONEPASS)
@pytest.mark.parametrize("mode,fuse", SCHEDULES)
def test_every_sweep_form_matches_the_oracle(ctx, mode, fuse, onepass):
    """small_nnz = 0 (so that these small systems take the multi-launch path at all) x newton_pipeline x Gram-Schmidt schedule x
    one-pass knob, on (a) a Liouvillian, m_max 6 and 12, (b) an operator of Krylov dimension 4 (breakdown: the later columns are
    discarded), (c) an eigenstate (the m == 1 shortcut), (d) a matrix-free Pauli-string operator (plain sweep, columns by events).
    The mat-vec count of every step must not depend on the pipeline, and a one-pass sweep that was asked for must have been taken."""
    saved = {k: ctx.tuning_get(k) for k in KNOBS}
    try:
        _set(ctx, small_nnz=0, arnoldi_mode=mode, arnoldi_fuse_dots=fuse, arnoldi_onepass=onepass)
        for name, m_max in RUNS:
            per_pipeline = {}
            for pipeline in (1, 0):
                _set(ctx, newton_pipeline=pipeline)
                seen = _steps(ctx, name, m_max)
                per_pipeline[pipeline] = [s[0] for s in seen]
                for _, _, stats in seen:
                    if name == "liouvillian" and onepass >= 2 and mode == 1:   # (the one-pass sweep belongs to the low-sync schedule)
                        assert stats["sweeps_onepass"] > 0, stats
                        assert stats["sweeps_onepass_redone"] == (stats["sweeps_onepass"] if onepass == 3 else 0), stats
                    if onepass == 0 or mode == 0 or name == "pauli":
                        assert stats["sweeps_onepass"] == 0, stats
            assert per_pipeline[1] == per_pipeline[0], (name, m_max, per_pipeline)
    finally:
        _set(ctx, **saved)


def test_persistent_small_sweep_ends_in_the_same_collector(ctx):
    """(a) with the default small_nnz: all columns in one launch, one download, no per-column waits -- with the hook's pipeline on
    and off (the hook is not run while such a sweep is collected: its columns arrive together).  The persistent kernel keeps
    m + 2 vectors in LDS (csrc/device.h: small_arnoldi_fits, 152 KiB): at N = 1369 that is m_max <= 5 (16 B x 7 x 1369 = 150 KiB;
    m_max = 6 needs 171 KiB), so m_max = 5 is the run that reaches it -- fewer launches than columns says so (the multi-launch
    sweep has more than two per column) -- and m_max = 12 is the same call falling through to the multi-launch sweep by itself."""
    saved = ctx.tuning_get("newton_pipeline")
    try:
        assert ctx.tuning_get("small_nnz") > 0
        op = _operator(ctx, "liouvillian", fmt=None)
        for pipeline in (1, 0):
            _set(ctx, newton_pipeline=pipeline)
            for n_matvec, launches, stats in _steps(ctx, "liouvillian", 5, op=op):
                assert launches < stats["n_matvec"], (launches, stats)      # one launch per sweep and the combine: fewer than columns
            for n_matvec, launches, stats in _steps(ctx, "liouvillian", 12, op=op):
                assert launches > 2 * stats["n_matvec"], (launches, stats)
    finally:
        _set(ctx, newton_pipeline=saved)


@pytest.mark.parametrize("mode,fuse", SCHEDULES)
def test_plain_arnoldi_call_not_extended_and_breakdown(ctx, mode, fuse):
    """arnoldi! as ritzvals calls it (extended = false, no hook: the folded sweep hands its last vector over as it is and ends at
    the stream's end) against the oracle's Hessenberg matrix, and the breakdown of (b) at column 4 with the later columns discarded."""
    saved = {k: ctx.tuning_get(k) for k in KNOBS}
    try:
        _set(ctx, small_nnz=0, arnoldi_mode=mode, arnoldi_fuse_dots=fuse)
        A, psi0, _ = _system("liouvillian")
        op = _operator(ctx, "liouvillian")
        m = 6
        for extended in (False, True):
            q = L.Krylov(ctx, N, m + 1)
            Hess = np.zeros((m + 1, m + 1), dtype=complex, order="F")
            m_out = L.arnoldi(Hess, q, m, L.State(ctx, data=psi0), op, 0.5, extended=extended)
            oHess = np.zeros((m + 1, m + 1), dtype=complex)
            oq = [np.zeros(N, dtype=complex) for _ in range(m + 1)]
            om = qo.arnoldi(oHess, oq, m, psi0.copy(), A, dt=0.5, extended=extended)
            assert m_out == om == m
            assert np.abs(Hess - oHess).max() < 1e-12, np.abs(Hess - oHess).max()   # (tests/test_gpu_parity.py: test_arnoldi_matches_oracle)
            # the last vector: normalised (extended) or as the projection left it
            assert np.linalg.norm(q.vec(m) - oq[m]) < 1e-11
        _, psib, kw = _system("four_eigenvalues")
        opb = _operator(ctx, "four_eigenvalues")
        q = L.Krylov(ctx, N, 11)
        Hess = np.zeros((11, 11), dtype=complex, order="F")
        m_out = L.arnoldi(Hess, q, 10, L.State(ctx, data=psib), opb, 0.7, norm_min=1e-9)
        assert m_out == 4 and np.all(Hess[:, 4:] == 0)
    finally:
        _set(ctx, **saved)
