"""Edge tests of the Pauli-string kernel (csrc/engine_pauli.hip): every instantiation the launcher can pick and every register /
group-table edge of the kernel, one application compared ROW BY ROW with an extended-precision reference that shares nothing with
the mask arithmetic (tests/pauli_ref.py), under the forward bound of a sum of S complex products

    |y_r - ref_r| <= (S + 8) 2^-52 (|alpha| A_r + |beta| |y0_r|),      A_r = sum_t |a_t| |x_partner(r, t)|,

(nothing measured: a wrong sign or partner on ONE string moves its row by ~ 2 |a_t| |x_p| >= ~ A_r / S, orders of magnitude above
it; no row is skipped).  Which instantiation a case reaches, by the launcher's rules (pauli_launch, pauli_tables):

    STAGE = true  (tables in LDS: <= 1024 groups and <= 2048 strings)
      GS = 1, FAST    field_only, identity_plus_field (with a walked zero-mask group), the set_coeffs walk at real coefficients
      GS = 1          single_z (walked zero-mask group), field_only_complex, seam_masks, low_only, high_k, the set_coeffs walk
      GS = 2          xx_yy_only (g_begin = 0)
      generic         one_block, two_blocks, top_qubits, triples (multi-string branch), mixed_sizes (one-string branch inside)
    STAGE = false (tables read from global memory)
      generic only    many_groups, many_groups_diag (by group count), many_strings, huge_diagonal (by string count; the diagonal
                      group beyond kPauliMaxStrings is WALKED as group 0)
    each with the plain epilogue (mul!) and, for the cheby! cases below, the ChebyOp epilogue.

The library reports no kernel name: that STAGE = false ran is known from the launcher's rule and the counts asserted here (and one
launch per application: no unfused fall-back), not observed."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import qp_oracle as qo  # noqa: E402
import qprop_amd.lib as L  # noqa: E402
import qprop_amd.synth as synth  # noqa: E402
from pauli_ref import PauliRef  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10
ALPHA = 0.7 - 0.2j
BETAS = (0.0, -0.4 + 1.1j)
MAX_GROUPS, MAX_STRINGS = 1024, 2048      # kPauliMaxGroups, kPauliMaxStrings (csrc/engine_pauli.hip)


@pytest.fixture()
def ctx():
    c = L.Context(0)
    yield c
    c.close()


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def _random_labels(n, count, rng):
    out = []
    while len(out) < count:      # distinct strings, none of them the identity
        m = L.pauli_masks("".join(rng.choice(list("IXYZ"), size=n, p=[0.55, 0.15, 0.15, 0.15])))
        if m != (0, 0) and m not in out:
            out.append(m)
    return out


def _distinct(rng, lo, hi, count):
    return [int(v) for v in rng.permutation(np.arange(lo, hi))[:count]]


def _zz_diagonal(n):
    return [(0, (1 << i) | (1 << (i + 1))) for i in range(n - 1)]


def case_strings(cid, real=False):
    """(n, [(amplitude, (xmask, zmask)), ...]) of a case of the issue's table.  Amplitudes random in [-1, 1], complex unless the
    case (or ``real``: the Hermitian generators of the cheby! / newton! tests) says real."""
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    div = 1.0

    def z(n):
        return int(rng.integers(0, 1 << n))

    if cid == "one_block":
        n, masks = 6, _random_labels(6, 20, rng) + [(0, 0)]
    elif cid == "two_blocks":
        n = 7
        masks = _random_labels(7, 19, rng) + [(64, z(7))]
    elif cid == "seam_masks":
        n = 9
        masks = [(xm, z(9)) for xm in (1, 32, 63, 64, 65, 96, 127, 128, 191, 256, 511)]
    elif cid == "single_z":
        n, masks = 8, [(0, 1 << 3)] + [(1 << i, 0) for i in range(8)]
    elif cid == "identity_plus_field":
        n, masks, real = 8, [(0, 0)] + [(1 << i, 0) for i in range(8)], True
    elif cid == "field_only":
        n, masks, real = 10, [(1 << i, 0) for i in range(10)], True
    elif cid == "field_only_complex":
        n, masks = 10, [(1 << i, 0) for i in range(10)]
    elif cid == "xx_yy_only":
        n = 10
        masks = [m for i in range(9) for m in ((3 << i, 0), (3 << i, 3 << i))]
    elif cid == "triples":
        n = 10
        masks = [(xm, z(10)) for xm in _distinct(rng, 1, 1024, 12) for _ in range(3)]
    elif cid == "mixed_sizes":
        n = 10
        sizes = (1, 2, 1, 5, 1, 3, 1, 1, 4, 1)
        masks = [(xm, z(10)) for xm, k in zip(_distinct(rng, 1, 1024, len(sizes)), sizes) for _ in range(k)]
    elif cid == "low_only":
        n = 9
        masks = [(xm, z(9)) for xm in _distinct(rng, 1, 64, 20)] + _zz_diagonal(9)
    elif cid.startswith("high_"):
        n, k = 11, int(cid[5:])
        xms = _distinct(rng, 64, 2048, k)
        xms[0] = (xms[0] // 64) * 64                 # one line without a lane permutation; the others have low bits with
        for i in range(1, k):                        # probability 63 / 64 -- at least one by construction below
            if xms[i] == xms[0]:
                xms[i] += 1
        if k > 1 and xms[1] % 64 == 0:
            xms[1] += 33
        masks = [(xm, z(11)) for xm in xms]
    elif cid == "top_qubits":
        n = 18
        masks = [(1 << 17, 0), (3 << 16, 3 << 16), ((1 << 17) | 33, 1 << 5), (0, (1 << 17) | 1), (64, 0), (63, 0), (127, 64),
                 (1 << 16, (1 << 17) | 2), ((3 << 16) | 64, 1 << 16)]
    elif cid in ("many_groups", "many_groups_diag"):
        n, real, div = 11, True, 40.0
        rng = np.random.default_rng(zlib.crc32(b"many_groups"))      # "the same" 1100 strings in both
        masks = [(xm, z(11)) for xm in _distinct(rng, 1, 2048, 1100)]
        if cid == "many_groups_diag":
            masks += _zz_diagonal(11) + [(0, 1 << i) for i in range(11)] + [(0, 5 << i) for i in range(9)]      # 10 + 11 + 9 = 30
    elif cid == "many_strings":
        n = 11
        masks = [(xm, zm) for xm in _distinct(rng, 1, 2048, 300) for zm in _distinct(rng, 0, 2048, 7)]
    elif cid == "huge_diagonal":
        n = 12
        masks = [(0, zm) for zm in _distinct(rng, 1, 4096, 2100)] + [(1 << i, 0) for i in range(12)]
    else:
        raise KeyError(cid)
    assert len(set(masks)) == len(masks), cid
    amps = [float(rng.uniform(-1, 1)) / div if real else complex(rng.uniform(-1, 1), rng.uniform(-1, 1)) / div for _ in masks]
    return n, list(zip(amps, masks))


MUL_CASES = ["one_block", "two_blocks", "seam_masks", "single_z", "identity_plus_field", "field_only", "field_only_complex",
             "xx_yy_only", "triples", "mixed_sizes", "low_only", "high_1", "high_7", "high_8", "high_9", "high_16", "high_17",
             "top_qubits", "many_groups", "many_groups_diag", "many_strings", "huge_diagonal"]
UNSTAGED = ("many_groups", "many_groups_diag", "many_strings", "huge_diagonal")
CHEBY_CASES = ["one_block", "two_blocks", "single_z", "field_only", "xx_yy_only", "many_groups", "many_groups_diag", "huge_diagonal"]


def _shape_of(strings):
    """(number of x-mask groups, strings of the zero-mask group) -- what the launcher's rules look at."""
    xs = [xm for _, (xm, _) in strings]
    return len(set(xs)), xs.count(0)


# ---- the row-wise check --------------------------------------------------------------------------------------------------------

def check_rows(y, ref, A, y0, beta, S, what):
    """Every row under the derived bound; returns (and prints, for -s) the largest err / bound."""
    err = np.abs(np.asarray(y, dtype=np.clongdouble) - ref)
    bound = (S + 8) * np.longdouble(2.0) ** -52 * (abs(ALPHA) * A + abs(beta) * np.abs(y0.astype(np.clongdouble)))
    assert np.all(bound > 0), what
    ratio = err / bound
    worst = int(np.argmax(ratio))
    print(f"[pauli rows] {what}: S={S} max err/bound {float(ratio[worst]):.4f} at row {worst} (block {worst >> 6}, lane {worst & 63})")
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rows beyond the bound, first {int(bad[0])} (block {int(bad[0]) >> 6}, lane {int(bad[0]) & 63}): "
                           f"err {float(err[bad[0]]):.3e} bound {float(bound[bad[0]]):.3e}")
    return float(ratio[worst])


def mul_and_check(ctx, op, n, strings, what, seed=1, one_launch=False):
    N = 1 << n
    H = PauliRef(n, strings)
    x0, y0 = synth.random_state(N, seed=seed), synth.random_state(N, seed=seed + 1)
    Hx, A = H.apply(x0), H.abs_apply(x0)
    x = L.State(ctx, data=x0)
    for beta in BETAS:
        y = L.State(ctx, data=y0)
        ctx.reset_stats()
        op.mul(x, y, alpha=ALPHA, beta=beta)
        if one_launch:
            assert ctx.stats()["n_kernel_launches"] == 1
        ref = np.clongdouble(beta) * y0.astype(np.clongdouble) + np.clongdouble(ALPHA) * Hx
        check_rows(y.numpy(), ref, A, y0, beta, len(strings), f"{what} beta={beta}")
        y.close()
    assert np.array_equal(x.numpy(), x0)
    x.close()


@pytest.mark.parametrize("cid", MUL_CASES)
def test_mul_rows_against_extended_precision(ctx, cid):
    """y = beta y0 + alpha H x0 through op.mul for beta = 0 and beta != 0, every row under the derived bound (module docstring)."""
    n, strings = case_strings(cid)
    if cid in UNSTAGED:      # the launch path the case was built for: counts beyond what the LDS tables hold, one launch per mul!
        groups, _ = _shape_of(strings)
        assert groups > MAX_GROUPS or len(strings) > MAX_STRINGS
    op = L.PauliOperator(ctx, n, [strings])
    assert op.format == L.FMT_MATFREE and op.nrows == 1 << n
    mul_and_check(ctx, op, n, strings, cid, one_launch=cid in UNSTAGED)
    op.close()


# ---- cheby! / newton! through the same instances (the ChebyOp epilogue is another instantiation of each kernel) ------------------

@pytest.mark.parametrize("cid", CHEBY_CASES)
def test_cheby_through_the_same_instances(ctx, cid):
    """Real amplitudes (a Hermitian generator): cheby! forward, forward, backward against the oracle driven by the extended-precision
    reference -- 2-norm below 1e-10 and a unit norm to 1e-12 as test_pauli_cheby_matches_oracle_and_stored_matrix; at most n_coeffs
    launches per step (the fused term).  many_groups also takes one newton! step (the plain epilogue inside the Arnoldi sweep)."""
    n, strings = case_strings(cid, real=True)
    N = 1 << n
    sa = float(sum(abs(a) for a, _ in strings))
    H = PauliRef(n, strings)
    op = L.PauliOperator(ctx, n, [strings])
    psi0 = synth.random_state(N, seed=n)
    dt = 6.0 / sa
    wrk = L.ChebyWrk(ctx, N, 2.1 * sa, -1.05 * sa, dt)
    owrk = qo.ChebyWrk(psi0, 2.1 * sa, -1.05 * sa, dt)
    assert wrk.n_coeffs == owrk.n_coeffs > 3
    psi = L.State(ctx, data=psi0)
    ref = psi0.copy()
    for sg in (1, 1, -1):
        ctx.reset_stats()
        L.cheby(psi, op, sg * dt, wrk)
        assert ctx.stats()["n_kernel_launches"] <= wrk.n_coeffs
        qo.cheby(ref, H, sg * dt, owrk)
        err = float(np.linalg.norm(psi.numpy() - ref))
        print(f"[pauli cheby] {cid} sign {sg}: |dpsi| = {err:.3e}")
        assert err < TOL, sg
    assert abs(np.linalg.norm(psi.numpy()) - 1.0) < 1e-12
    if cid == "many_groups":
        nw = L.NewtonWrk(ctx, N, m_max=12)
        onw = qo.NewtonWrk(ref, m_max=12)
        L.newton(psi, op, 2.0 / sa, nw)
        qo.newton(ref, H, 2.0 / sa, onw)
        assert np.linalg.norm(psi.numpy() - ref) < TOL and nw.restarts == onw.restarts
        nw.close()
    for h in (psi, wrk, op):
        h.close()


# ---- coefficients that move the host-side kernel choice ------------------------------------------------------------------------

def test_set_coeffs_moves_the_kernel_choice(ctx):
    """A lazy sum drift (ZZ + Z) + c1 (X_i) + c2 (Z_i), real amplitudes: set_coeffs walks the walked strings FAST <-> signed GS = 1
    <-> zero coefficients and the diagonal vector real <-> complex, in both directions; after every change one mul! under the
    row-wise bound (the reference is given the products c a in extended precision: their rounding on the host is inside the + 8)."""
    n = 9
    rng = np.random.default_rng(44)
    drift = [(float(rng.uniform(-1, 1)), m) for m in _zz_diagonal(n) + [(0, 1 << i) for i in range(n)]]
    xs = [(float(rng.uniform(-1, 1)), (1 << i, 0)) for i in range(n)]
    zs = [(float(rng.uniform(-1, 1)), (0, 1 << i)) for i in range(n)]
    op = L.PauliOperator(ctx, n, [drift, xs, zs], ncoeffs=2)
    for k, (c1, c2) in enumerate(((1, 1), (0.5 + 0.5j, 1), (0, 1), (1, 2j), (1, 0), (-1, 1))):
        op.set_coeffs([c1, c2])
        strings = (drift + [(np.clongdouble(c1) * a, m) for a, m in xs] + [(np.clongdouble(c2) * a, m) for a, m in zs])
        mul_and_check(ctx, op, n, strings, f"set_coeffs {c1}, {c2}", seed=50 + k)
    op.close()


# ---- graph replay of matrix-free operators -------------------------------------------------------------------------------------

def _graph_scenarios(ctx, knob):
    """The states after every step of scenario (a) and (b) with knob cheby_graph = ``knob``, and the graph launches counted."""
    n = 9
    N = 1 << n
    saved = ctx.tuning_get("cheby_graph")
    ctx.tuning_set("cheby_graph", knob)
    out = {"a": [], "b": []}
    try:
        ctx.reset_stats()
        # (a) two operators, one workspace, one state buffer; A stays alive
        sA, sB = synth.tfim_pauli_terms(n, h=1.0), synth.tfim_pauli_terms(n, h=0.3)
        A, B = L.PauliOperator(ctx, n, [sA]), L.PauliOperator(ctx, n, [sB])
        sa = float(sum(abs(a) for a, _ in sA))
        dt = 6.0 / sa
        wrk = L.ChebyWrk(ctx, N, 2.1 * sa, -1.05 * sa, dt)
        psi = L.State(ctx, data=synth.random_state(N, seed=71))
        for op in (A, A, A, B, B, B):
            L.cheby(psi, op, dt, wrk)
            out["a"].append(psi.numpy().copy())
        # (b) one operator, a controlled X term: 1 -> 0.5 + 0.5j (not Hermitian: a short step) -> 1
        zz = [(-1.0, m) for m in _zz_diagonal(n)] + [(-0.1, (0, 1 << i)) for i in range(n)]
        xs = [(-1.0, (1 << i, 0)) for i in range(n)]
        C = L.PauliOperator(ctx, n, [zz, xs], ncoeffs=1)
        sc = float(sum(abs(a) for a, _ in zz + xs))
        dtc = 1.0 / sc
        wrkc = L.ChebyWrk(ctx, N, 2.1 * sc, -1.05 * sc, dtc)
        phi = L.State(ctx, data=synth.random_state(N, seed=72))
        for c in (1.0, 0.5 + 0.5j, 1.0):
            C.set_coeffs([c])
            for _ in range(3):
                L.cheby(phi, C, dtc, wrkc)
                out["b"].append(phi.numpy().copy())
        out["graph_launches"] = ctx.stats()["n_graph_launches"]
        for h in (psi, phi, wrk, wrkc, A, B, C):
            h.close()
    finally:
        ctx.tuning_set("cheby_graph", saved)
    return out


def test_cheby_graph_with_matrix_free_operators(ctx):
    """Knob `cheby_graph` with matrix-free operators.  A captured step bakes in the Pauli launcher's host-side choice of kernel and
    of the real / complex diagonal vector, and the graph's key knows an operator by its stored arrays -- all NULL here: (a) two
    operators on one workspace and state, (b) a real -> complex -> real coefficient would replay a stale graph (wrong numbers, every
    pointer valid).  The fix taken: qp_cheby_step does not take the graph path for QP_FMT_MATFREE (the knob is off by default and
    measured no gain), so n_graph_launches stays 0 and every state is bit-identical to the run with the knob off."""
    plain = _graph_scenarios(ctx, 0)
    graph = _graph_scenarios(ctx, 1 << 20)
    assert plain["graph_launches"] == 0 and graph["graph_launches"] == 0
    for key in ("a", "b"):
        assert len(plain[key]) == len(graph[key]) == (6 if key == "a" else 9)
        for k, (p, g) in enumerate(zip(plain[key], graph[key])):
            assert np.array_equal(p, g), (key, k)
    n = 9
    sA, sB = synth.tfim_pauli_terms(n, h=1.0), synth.tfim_pauli_terms(n, h=0.3)
    sa = float(sum(abs(a) for a, _ in sA))
    dt = 6.0 / sa
    psi0 = synth.random_state(1 << n, seed=71)
    ref = psi0.copy()
    owrk = qo.ChebyWrk(psi0, 2.1 * sa, -1.05 * sa, dt)
    for strings in (sA, sA, sA, sB, sB, sB):
        qo.cheby(ref, PauliRef(n, strings), dt, owrk)
    assert np.linalg.norm(graph["a"][-1] - ref) < TOL
    assert not np.array_equal(graph["a"][2], graph["a"][3])


# ---- errors that must stay clean -----------------------------------------------------------------------------------------------

def test_errors_stay_clean(ctx):
    for nq in (5, 31):
        with pytest.raises(L.QPError):
            L.PauliOperator(ctx, nq, [[(1.0, (1, 0))]])
    n = 8
    N = 1 << n
    strings = synth.tfim_pauli_terms(n)
    sa = float(sum(abs(a) for a, _ in strings))
    op = L.PauliOperator(ctx, n, [strings])
    psi0 = synth.random_state(N, seed=81)
    dt = 6.0 / sa
    wrk = L.ChebyWrk(ctx, N, 2.1 * sa, -1.05 * sa, dt)
    assert wrk.n_coeffs > 3
    psi = L.State(ctx, data=psi0)
    with pytest.raises(L.QPError, match="check_normalization is not available"):
        L.cheby(psi, op, dt, wrk, check_normalization=True)
    assert np.array_equal(psi.numpy(), psi0)          # the refused step has not touched the state
    L.cheby(psi, op, dt, wrk)
    ref = qo.cheby(psi0.copy(), PauliRef(n, strings), dt, qo.ChebyWrk(psi0, 2.1 * sa, -1.05 * sa, dt))
    assert np.linalg.norm(psi.numpy() - ref) < TOL
    batch = 4
    panel = L.State(ctx, data=np.repeat(psi0, batch))
    with pytest.raises(L.QPError, match="no stored entries"):
        L.cheby_batched(panel, op, dt, L.ChebyWrk(ctx, N * batch, 2.1 * sa, -1.05 * sa, dt), batch)
