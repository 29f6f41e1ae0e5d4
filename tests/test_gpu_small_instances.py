"""Every reachable instance `(ent, rows_per_group)` of the two persistent single-workgroup kernels (csrc/kernels_small.hip:
cheby_propagate_small_kernel, arnoldi_small_kernel) on the smallest operator that selects it and on a ragged variant -- the shared
table of tests/small_instances.py, which tests/test_small_plan_host.py holds against the reachable set.  Each case first asserts,
through qp_operator_small_plan (the engine's own decision), the instance it is named after; then the whole time grid / the whole
sweep is compared with the oracle and with the general (launch per kernel) path, and the launch count says which path ran."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import qp_oracle as qo  # noqa: E402
import qprop_amd.lib as L  # noqa: E402
import qprop_amd.propagator as P  # noqa: E402
import small_instances as si  # noqa: E402

pytestmark = pytest.mark.gpu

NSTEPS = 24
TLIST = np.linspace(0.0, 1.0, NSTEPS + 1)
ENVELOPE = dict(E_min=-4.0, E_max=4.0)      # the operators' rows sum to at most 2 (+ 0.6 x 0.5 per control) in absolute value
FORMATS = {"hrb": L.FMT_HRB, "rbcsr": L.FMT_RBCSR}


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


class general_loop:
    """small_nnz = 0: the launch-per-kernel path."""

    def __enter__(self):
        L.tuning_set("small_nnz", 0)

    def __exit__(self, *exc):
        L.tuning_set("small_nnz", si.SMALL_NNZ)


def _state(n, seed):
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    return psi / np.linalg.norm(psi)


def _controls(k):
    """k control amplitudes, given on the intervals of TLIST."""
    mid = 0.5 * (TLIST[1:] + TLIST[:-1])
    return [0.6 * np.sin((j + 2) * mid + 0.3) for j in range(k)]


@functools.lru_cache(maxsize=None)
def _cheby_inputs(name):
    """Drift + one control on the drift's pattern (so that the union pattern -- what the plan sees -- is the table's), a state, and
    the oracle's stored states of both directions: computed once per case, shared by the device formats."""
    c = si.BY_NAME[name]
    H0 = c.build()
    H1 = si.same_pattern(H0, 1000 + c.n)
    (amp,) = _controls(1)
    psi0 = _state(c.n, 7 + c.n)
    ref = {bw: qo.propagate(psi0, qo.Generator([H0, H1], [amp]), TLIST, "cheby", storage=True, backward=bw, **ENVELOPE) for bw in (False, True)}
    return H0, H1, amp, psi0, ref


def _plan_of(ctx, mats, ncoeffs, fmt, kind="cheby", m=1):
    """The engine's decision for the operator `propagate` is about to build from the same matrices."""
    op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A) for A in mats], ncoeffs, fmt)
    try:
        assert fmt == L.FMT_AUTO or op.format == fmt
        return op.small_plan(kind, m)
    finally:
        op.close()


def _launches(ctx, f):
    ctx.reset_stats()
    out = f()
    return out, ctx.stats()["n_kernel_launches"]


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("name", [c.name for c in si.CHEBY_CASES])
def test_cheby_instance(ctx, name, fmt):
    """24 steps, drift + control, forward and backward, Hermitian-packed (negative `map` entries: the conjugation bit of the packed
    word) and plain row blocks: every stored state within 1e-10 of the oracle (the project's bar, BASELINE.json), within 1e-13 of
    the general loop; the whole grid in fewer launches than it has steps (the general loop: at least one per term and step).
    Measured on an MI355X over all cases: at most 3.4e-15 from the oracle and 1.7e-16 from the general loop; at most 12 launches
    (operator build and evaluate! included) where the general loop takes 220 or more."""
    c = si.BY_NAME[name]
    H0, H1, amp, psi0, ref = _cheby_inputs(name)
    assert _plan_of(ctx, [H0, H1], 1, FORMATS[fmt]) == c.cheby
    gen = P.hamiltonian(H0, (H1, amp))
    kw = dict(method="cheby", storage=True, ctx=ctx, device_format=FORMATS[fmt], **ENVELOPE)
    for backward in (False, True):
        (out, st), n_launch = _launches(ctx, lambda: P.propagate(psi0, gen, TLIST, backward=backward, **kw))
        assert n_launch < NSTEPS, n_launch
        rout, rst = ref[backward]
        err_o = max(np.max(np.linalg.norm(st - rst, axis=0)), np.linalg.norm(out - rout))
        with general_loop():
            (out_g, st_g), n_general = _launches(ctx, lambda: P.propagate(psi0, gen, TLIST, backward=backward, **kw))
        assert n_general >= NSTEPS
        err_g = max(np.max(np.linalg.norm(st - st_g, axis=0)), np.linalg.norm(out - out_g))
        print(f"{name} {fmt} backward={backward}: oracle {err_o:.2e}, general loop {err_g:.2e}, launches {n_launch} / {n_general}")
        assert err_o < 1e-10
        assert err_g < 1e-13


def test_cheby_beyond_600_rows_has_no_32_slot_form(ctx):
    """1025 rows of 5 entries need 32 slots per lane: an Arnoldi sweep takes (8, 4), the Chebychev grid the general loop."""
    for name in ("e8r4-band5", "e8r4-ragged"):
        c = si.BY_NAME[name]
        H0 = c.build()
        assert c.cheby is None and _plan_of(ctx, [H0], 0, L.FMT_AUTO) is None
        assert _plan_of(ctx, [H0], 0, L.FMT_AUTO, "arnoldi", si.ARNOLDI_COLUMNS) == (1, 8, 4)
        psi0 = _state(c.n, 3)
        (out, st), n_launch = _launches(ctx, lambda: P.propagate(psi0, (H0,), TLIST, method="cheby", storage=True, ctx=ctx, **ENVELOPE))
        assert n_launch >= NSTEPS
        rout, rst = qo.propagate(psi0, H0, TLIST, "cheby", storage=True, **ENVELOPE)
        assert np.max(np.linalg.norm(st - rst, axis=0)) < 1e-10 and np.linalg.norm(out - rout) < 1e-10


# one instance with one row per lane group, one with two, one packed (32 slots: a lane's upper 16 values in LDS)
EDGE_CASES = ["e8r1-ragged", "e4r2-ragged", "e16r2-band9"]


def _both_paths(ctx, run):
    """run() on the persistent path (asserted by its launch count) and on the general loop."""
    small, n_launch = _launches(ctx, run)
    assert n_launch < NSTEPS, n_launch
    with general_loop():
        general, n_general = _launches(ctx, run)
    assert n_general > n_launch
    return small, general


@pytest.mark.parametrize("name", EDGE_CASES)
def test_cheby_setup_edges(ctx, name):
    """A lazy sum without drift (nops == ncoeffs), five control terms, the fewest coefficients cheby_coeffs returns (two: the first
    term is also the last), a single step, and set_scale(0.5): oracle 1e-10, general loop 1e-13."""
    c = si.BY_NAME[name]
    H0 = c.build()
    psi0 = _state(c.n, 11 + c.n)
    terms = [si.same_pattern(H0, 2000 + 10 * c.n + k, rho=0.6) for k in range(5)]
    amps = _controls(5)

    def check(gen, ogen, tlist=TLIST, envelope=ENVELOPE, **kw):
        for backward in (False, True):
            run = lambda: P.propagate(psi0, gen, tlist, method="cheby", storage=True, ctx=ctx, backward=backward, **envelope, **kw)   # noqa: E731
            (out, st), (out_g, st_g) = _both_paths(ctx, run)
            rout, rst = qo.propagate(psi0, ogen, tlist, "cheby", storage=True, backward=backward, **envelope, **kw)
            assert np.max(np.linalg.norm(st - rst, axis=0)) < 1e-10 and np.linalg.norm(out - rout) < 1e-10
            assert np.max(np.linalg.norm(st - st_g, axis=0)) < 1e-13 and np.linalg.norm(out - out_g) < 1e-13

    # no drift: two controlled terms and nothing else
    assert _plan_of(ctx, terms[:2], 2, L.FMT_AUTO) == c.cheby
    check(P.hamiltonian((terms[0], amps[0]), (terms[1], amps[1])), qo.Generator(terms[:2], amps[:2]))
    # drift + five control terms (rows sum to at most 2 + 5 x 0.6 x 0.6 in absolute value)
    assert _plan_of(ctx, [H0] + terms, 5, L.FMT_AUTO) == c.cheby
    check(P.hamiltonian(H0, *zip(terms, amps)), qo.Generator([H0] + terms, amps), envelope=dict(E_min=-6.0, E_max=6.0))
    # two coefficients: |a_2| = 2 J_1(Delta dt / 2) is already below the limit
    assert P.init_prop(psi0, (H0,), TLIST, "cheby", ctx=ctx, cheby_coeffs_limit=0.5, **ENVELOPE).wrk.n_coeffs == 2
    check((H0,), H0, cheby_coeffs_limit=0.5)
    # a single step
    check(P.hamiltonian(H0, (terms[0], amps[0][:1])), qo.Generator([H0, terms[0]], [amps[0][:1]]), tlist=TLIST[:2])
    # ScaledOperator: 0.5 H through the library's step loop
    op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H0)])
    op.set_scale(0.5)
    assert op.small_plan("cheby") == c.cheby
    dt = TLIST[1] - TLIST[0]
    outs = []
    for small in (True, False):
        L.tuning_set("small_nnz", si.SMALL_NNZ if small else 0)
        try:
            psi = L.State(ctx, data=psi0)
            ctx.reset_stats()
            _, st = L.propagate_steps(op, psi, L.ChebyWrk(ctx, c.n, 8.0, -4.0, dt), np.full(NSTEPS, dt), store_states=True)
            assert (ctx.stats()["n_kernel_launches"] < NSTEPS) == small
            outs.append(st)
        finally:
            L.tuning_set("small_nnz", si.SMALL_NNZ)
    owrk = qo.ChebyWrk(psi0, 8.0, -4.0, dt)
    ref = [psi0.copy()]
    for _ in range(NSTEPS):
        ref.append(qo.cheby(ref[-1].copy(), qo.ScaledOperator(0.5, qo.Operator([H0], [])), dt, owrk))
    assert np.max(np.linalg.norm(outs[0] - np.array(ref), axis=1)) < 1e-10
    assert np.max(np.linalg.norm(outs[0] - outs[1], axis=1)) < 1e-13


def _observables(n, seed):
    """A Hermitian observable on a band, a diagonal one, and a non-Hermitian one with empty rows."""
    rng = np.random.default_rng(seed)
    O1 = si.banded(n, min(n, 3), seed, rho=1.0)
    O2 = sp.diags([np.linspace(-1.0, 1.0, n)], [0], format="csr", dtype=complex)
    O3 = sp.lil_matrix(sp.random(n, n, density=min(1.0, 4.0 / n), random_state=seed, format="csr") * (1 + 0.5j))
    for r in rng.choice(n, size=max(1, n // 5), replace=False):
        O3[r, :] = 0
    O3 = sp.csr_matrix(O3)
    O3.eliminate_zeros()
    assert np.any(np.diff(O3.indptr) == 0) and abs(O3 - O3.getH()).max() > 0
    return [O1, O2, O3]


@pytest.mark.parametrize("name", EDGE_CASES + ["obs-n256", "obs-n257"])
def test_cheby_observables(ctx, name):
    """Three observables: <psi|O|psi> at every grid point against vdot(psi, O psi) of the stored states, 1e-12.  256 and 257 rows lie
    on either side of a change of the observables' lanes per row (two for up to 256 rows, one beyond)."""
    if name.startswith("obs-n"):
        n = int(name[5:])
        H0, want_plan = si.banded(n, 3, n), (1, 4, 1)
    else:
        c = si.BY_NAME[name]
        n, H0, want_plan = c.n, c.build(), c.cheby
    assert _plan_of(ctx, [H0], 0, L.FMT_AUTO) == want_plan
    psi0 = _state(n, 5 + n)
    obs = _observables(n, 40 + n)
    kw = dict(method="cheby", storage=True, ctx=ctx, **ENVELOPE)
    (_, ev), n_launch = _launches(ctx, lambda: P.propagate(psi0, (H0,), TLIST, observables=obs, **kw))
    assert n_launch < NSTEPS and ev.shape == (3, NSTEPS + 1)
    _, st = P.propagate(psi0, (H0,), TLIST, **kw)
    want = np.array([[np.vdot(st[:, i], O @ st[:, i]) for i in range(NSTEPS + 1)] for O in obs])
    assert np.max(np.abs(ev - want)) < 1e-12


@pytest.mark.parametrize("name", EDGE_CASES)
def test_cheby_normalization_failure_names_step_and_term(ctx, name):
    """A spectral envelope that misses the spectrum: the persistent kernel's "Incorrect normalization" names the same step and term
    as the general loop's for the same inputs; with the right envelope the check passes on both."""
    c = si.BY_NAME[name]
    H0, H1, amp, psi0, _ = _cheby_inputs(name)
    gen = P.hamiltonian(H0, (H1, amp))
    text = []
    for small in (True, False):
        L.tuning_set("small_nnz", si.SMALL_NNZ if small else 0)
        try:
            with pytest.raises(L.QPError, match="Incorrect normalization") as e:
                P.propagate(psi0, gen, TLIST, method="cheby", ctx=ctx, E_min=3.0, E_max=3.2, check_normalization=True)
            text.append(str(e.value))
            P.propagate(psi0, gen, TLIST, method="cheby", ctx=ctx, check_normalization=True, **ENVELOPE)
        finally:
            L.tuning_set("small_nnz", si.SMALL_NNZ)
    assert re.search(r"in step \d+, term \d+$", text[0]), text
    assert text[0] == text[1], text


# ---------------------------------------------------------------------------------------------------------------- Arnoldi

def _arnoldi(ctx, Op, n, m, psi, dt, extended, norm_min=1e-15):
    ctx.reset_stats()
    q = L.Krylov(ctx, n, m + 1)
    Hess = np.zeros((m + 1, m + 1), dtype=complex, order="F")
    m_out = L.arnoldi(Hess, q, m, L.State(ctx, data=psi), Op, dt, extended=extended, norm_min=norm_min)
    return m_out, Hess, [q.vec(i) for i in range(m + 1)], ctx.stats()["n_kernel_launches"]


def _arnoldi_both_and_oracle(ctx, A, Op, m, psi, dt, extended, small_expected=True, norm_min=1e-15):
    """One sweep on the default path (one launch when `small_expected`) and on the multi-launch path, both against the oracle:
    Hessenberg matrix 1e-12, basis vectors 1e-11 (the bars of test_arnoldi_persistent_small)."""
    n = A.shape[0]
    res = [_arnoldi(ctx, Op, n, m, psi, dt, extended, norm_min)]
    with general_loop():
        res.append(_arnoldi(ctx, Op, n, m, psi, dt, extended, norm_min))
    assert (res[0][3] == 1) == small_expected, res[0][3]
    assert res[1][3] > 1
    Href = np.zeros((m + 1, m + 1), dtype=complex)
    qref = [np.zeros(n, dtype=complex) for _ in range(m + 1)]
    m_ref = qo.arnoldi(Href, qref, m, psi, A, dt, extended=extended, norm_min=norm_min)
    for m_out, Hess, qs, _ in res:
        assert m_out == m_ref
        assert np.max(np.abs(Hess - Href)) < 1e-12
        for i in range(m_ref + (1 if extended else 0)):
            assert np.linalg.norm(qs[i] - qref[i]) < 1e-11, i
    return m_ref


@pytest.mark.parametrize("name", [c.name for c in si.CASES])
def test_arnoldi_instance(ctx, name):
    """A non-Hermitian operator on the case's pattern: the whole sweep in ONE launch, Hessenberg matrix and basis as the oracle's
    and as the multi-launch path's, extended and not, dt of either sign."""
    c = si.BY_NAME[name]
    A = si.same_pattern(c.build(), 3000 + c.n, hermitian=False, rho=3.0)
    m = si.arnoldi_columns(c.n)
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)])
    assert Op.small_plan("arnoldi", m) == c.arnoldi
    psi = _state(c.n, 9 + c.n) if c.n > 1 else np.ones(1, dtype=complex)
    for extended, dt in ((True, 0.4), (False, -0.7), (True, -0.4), (False, 0.7)):
        _arnoldi_both_and_oracle(ctx, A, Op, m, psi, dt, extended)


def test_arnoldi_lds_fit_boundary(ctx):
    """The basis of m + 1 vectors and the work vector must fit 152 KiB of LDS: at 1025 rows m = 7 is the last sweep that does
    (16 B x (8 + 9 x 1025) = 147 728 <= 155 648 < 164 128 = 16 B x (8 + 10 x 1025)).  It is taken; m = 8 runs the multi-launch
    path and still matches."""
    c = si.BY_NAME["e4r4-band3"]
    assert si.arnoldi_fits_lds(c.n, 7) and not si.arnoldi_fits_lds(c.n, 8)
    A = si.same_pattern(c.build(), 77, hermitian=False, rho=3.0)
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)])
    psi = _state(c.n, 78)
    assert Op.small_plan("arnoldi", 7) == c.arnoldi and Op.small_plan("arnoldi", 8) is None
    for extended in (True, False):
        _arnoldi_both_and_oracle(ctx, A, Op, 7, psi, 0.4, extended, small_expected=True)
        _arnoldi_both_and_oracle(ctx, A, Op, 8, psi, 0.4, extended, small_expected=False)


def test_arnoldi_breakdown_with_two_rows_per_group(ctx):
    """Krylov dimension 3 inside a (4, 2) instance: a start vector on three rows that only couple to one another -- one of them the
    last row, alone in the second row set.  The sweep stops at column 3 on both paths (src/arnoldi.jl:91-95)."""
    n = 513
    A = sp.lil_matrix(si.same_pattern(si.banded(n, 3, 91), 92, hermitian=False, rho=3.0))
    block = [5, 300, n - 1]
    for r in block:                      # cut the three rows out of the band ...
        A[r, :] = 0
        A[:, r] = 0
    rng = np.random.default_rng(93)
    for r in block:                      # ... and couple them to one another: three entries per row, as in the band
        for col in block:
            A[r, col] = rng.standard_normal() + 1j * rng.standard_normal()
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    assert np.diff(A.indptr).max() == 3
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)])
    assert Op.small_plan("arnoldi", 6) == (1, 4, 2)
    psi = np.zeros(n, dtype=complex)
    psi[block] = np.array([0.6, 0.48j, 0.64])
    for extended, dt in ((True, 0.4), (False, -0.7)):
        assert _arnoldi_both_and_oracle(ctx, A, Op, 6, psi, dt, extended, norm_min=1e-10) == 3
