"""The Gram-Schmidt kernels of the Krylov engine on bases that are NOT orthogonal, and at the edges of their strides.

Every other test reaches the low-synchronisation step (csrc/kernels_blas.hip: multidot_kernel, multidot_reduce_kernel,
mgs_solve_kernel, mgs_update_kernel; csrc/kernels_arnoldi.hip; csrc/mgs_common.h) on a basis the engine built itself: orthonormal
to 1e-16, so that whatever computes, stores, conjugates, indexes or consumes a Gram entry wrongly moves the results by 1e-16.
Here the basis has Gram entries of 0.03 .. 0.2 (tests/krylov_ref.py: make_basis), the reference is sequential modified
Gram-Schmidt in extended precision, and what is asserted is a bound derived from absolute values (krylov_ref: dot_bound,
coef_bound, update_bound): every test prints its largest error / bound, and a defect in the Gram term is 10^11 or more above it
(tests/test_krylov_ref.py plants them).

  * the building blocks of the row-partitioned sweep, directly: multidot -> project column by column, normalize, combine;
  * the single-GPU forms of a column -- dots in the mat-vec's epilogue, reduction + solve in the update's prologue, the ticket
    path of the reduction kernel, sequential passes -- through extend_arnoldi on a basis whose Gram rows the building blocks
    recorded (include/qprop.h: qp_krylov_project), with the launch count saying which form ran."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import krylov_ref as kr  # noqa: E402
import qprop_amd.lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
LD, CLD, U = kr.LD, kr.CLD, kr.U
RED = 256            # csrc/device.h: kRedBlocks


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _ratio(err, bound):
    return kr.Column._ratio(err, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# multidot -> project, column by column
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,J", kr.BLOCK_CASES)
def test_multidot_and_project_on_a_nonorthogonal_basis(ctx, n, J):
    """Column jj = 0 .. J: w = V_{jj+1} (jj < J) or a vector with coefficients of order one (jj = J) against V_0 .. V_jj.  multidot:
    c_i = <V_i|w> and g_i = <V_i|V_jj> under the dot bound; project (which reads the Gram rows the earlier columns stored):
    hess_col[i] = dt h_i under the coefficient bound, the vector element by element, the 256 norm partials; both signs of dt."""
    V = kr.make_basis(n, J, kr.delta_for(J), seed=1000 + J)
    W = list(V[1:]) + [kr.make_vector(V, seed=2000 + J)]
    G = kr.gram(V)
    cols = [kr.Column(V, W[jj], j=jj, G=G) for jj in range(J + 1)]
    q = L.Krylov(ctx, n, J + 2)
    views = [q.view(i) for i in range(J + 2)]
    reduced, hess, npart = L.State(ctx, n=2 * (J + 1)), L.State(ctx, n=J + 1), L.State(ctx, n=RED)
    worst = dict(dots=0.0, coefs=0.0, vector=0.0, norm=0.0)
    for dt in kr.DTS:
        views[0].upload(V[0])
        for jj, col in enumerate(cols):
            views[jj + 1].upload(W[jj])
            q.multidot(jj, reduced)
            r_dots = col.ratio_dots(reduced.numpy())
            q.project(jj, dt, reduced, hess, npart)
            r_coefs = col.ratio_coefs(hess.numpy()[: jj + 1].astype(CLD) / LD(dt))
            r_vec = col.ratio_vector(q.vec(jj + 1))
            r_norm = col.ratio_norm2(npart.numpy())
            for k, v in zip(worst, (r_dots, r_coefs, r_vec, r_norm)):
                worst[k] = max(worst[k], v)
            assert r_dots <= 1.0 and r_coefs <= 1.0 and r_vec <= 1.0 and r_norm <= 1.0, (n, J, dt, jj, r_dots, r_coefs, r_vec, r_norm)
            if jj < J:
                views[jj + 1].upload(V[jj + 1])     # the projection has overwritten the next basis vector
    print(f"error/bound multidot+project n={n} J={J}: " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))


def test_project_refuses_a_basis_too_long_for_the_solve(ctx):
    """J = 88: the packed Gram triangle and the three columns of the solve no longer fit 64 KiB of LDS (csrc/device.h:
    mgs_lowsync_fits) -- a checked argument error, and nothing is launched."""
    J = kr.J_TOO_LONG
    q = L.Krylov(ctx, 257, J + 2)
    reduced, hess, npart = L.State(ctx, n=2 * (J + 1)), L.State(ctx, n=J + 1), L.State(ctx, n=RED)
    w = np.arange(257) + 1j
    q.view(J + 1).upload(w)
    ctx.reset_stats()
    with pytest.raises(L.QPArgumentError, match="too long for the low-synchronisation projection") as e:
        q.project(J, 0.37, reduced, hess, npart)
    assert e.value.status == 1      # QP_E_BAD_ARG
    assert ctx.stats()["n_kernel_launches"] == 0
    assert np.array_equal(q.vec(J + 1), w)


# ---------------------------------------------------------------------------------------------------------------------------
# normalize
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 257, 32769, 131073))
def test_normalize(ctx, n):
    """h = sqrt(sum of the 256 partials' real parts) -- a tree of 6 + 3 additions, the root, one product: (9 / 2 + 2) u < 8 u
    relative --, hess_norm = (dt h, h), the vector times 1 / h to 2 u per element (the reciprocal's and the product's rounding).
    norm_min > h: the raw norm is reported all the same and the vector keeps its bits."""
    rng = np.random.default_rng(n)
    w = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    w[kr.seam_elements(n)] *= kr.SEAM_WEIGHT
    part = rng.uniform(0.1, 3.0, RED) + 1j * rng.standard_normal(RED)      # (the imaginary parts are not part of the norm)
    h_ref = np.sqrt(np.sum(part.real.astype(LD)))
    q = L.Krylov(ctx, n, 2)
    view = q.view(1)
    npart, hn = L.State(ctx, data=part), L.State(ctx, n=2)
    worst = 0.0
    for dt in kr.DTS:
        view.upload(w)
        hn.fill(0.0)
        q.normalize(0, dt, 1e-15, npart, hn)
        out = hn.numpy()
        h = out[1].real
        assert abs(LD(h) - h_ref) <= 8 * U * h_ref, (h, h_ref)
        assert out[0] == dt * h and out[1].imag == 0.0
        r = _ratio(np.abs(q.vec(1).astype(CLD) - w.astype(CLD) / LD(h)), 2 * U * np.abs(w.astype(CLD)) / LD(h))
        worst = max(worst, r)
        assert r <= 1.0, (n, dt, r)
        view.upload(w)
        hn.fill(0.0)
        q.normalize(0, dt, 2.0 * h, npart, hn)       # a breakdown: below norm_min
        out = hn.numpy()
        assert out[1].real == h and out[0] == dt * h
        assert np.array_equal(q.vec(1), w)
    print(f"error/bound normalize n={n}: vector={worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------------------
# combine
# ---------------------------------------------------------------------------------------------------------------------------
COMBINE_NVEC = 66


@pytest.fixture(scope="module")
def combine_cache(ctx):
    yield {}


def _combine_basis(ctx, _combine_cache, n):
    """66 random vectors in a Krylov workspace and on the host, uploaded once per size (nothing writes them)."""
    if n not in _combine_cache:
        rng = np.random.default_rng(7 * n)
        Q = rng.standard_normal((COMBINE_NVEC, n)) + 1j * rng.standard_normal((COMBINE_NVEC, n))
        Q[:, kr.seam_elements(n)] *= kr.SEAM_WEIGHT
        q = L.Krylov(ctx, n, COMBINE_NVEC)
        for i in range(COMBINE_NVEC):
            q.view(i).upload(Q[i])
        Q.setflags(write=False)
        _combine_cache[n] = (q, Q)
    return _combine_cache[n]


@pytest.mark.parametrize("n", (1, 257, 65537))
@pytest.mark.parametrize("use_out", (0, 1))
@pytest.mark.parametrize("first", (0, 1))
@pytest.mark.parametrize("m", (1, 31, 32, 33, 64, 65))
def test_combine(ctx, combine_cache, m, first, use_out, n):
    """out = (use_out ? s0 out : 0) + sum_{k<m} c_k q_{first+k}: lists longer than kCoefBlock = 32 coefficients are chunked.
    Element-wise (m + 2) u (|s0| |out0_e| + sum_k |c_k| |q_ke|); the 256 norm partials against |out|^2 of what was stored."""
    q, Q = _combine_basis(ctx, combine_cache, n)
    rng = np.random.default_rng(1000 * m + 10 * first + use_out)
    coefs = rng.standard_normal(m) + 1j * rng.standard_normal(m)
    s0 = 0.7 - 1.1j
    out0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    ref = (CLD(s0) * out0.astype(CLD)) if use_out else np.zeros(n, dtype=CLD)
    mag = (abs(s0) * np.abs(out0.astype(CLD))) if use_out else np.zeros(n, dtype=LD)
    for k in range(m):
        qk = Q[first + k].astype(CLD)
        ref = ref + CLD(coefs[k]) * qk
        mag = mag + abs(coefs[k]) * np.abs(qk)
    out, npart = L.State(ctx, data=out0), L.State(ctx, n=RED)
    q.combine(out, use_out, s0, first, m, coefs, npart)
    got = out.numpy()
    r = _ratio(np.abs(got.astype(CLD) - ref), (m + 2) * U * mag)
    n2 = np.sum(np.abs(got.astype(CLD)) ** 2)
    parts = npart.numpy()
    r_norm = _ratio(abs(np.sum(parts.real.astype(LD)) - n2), (kr.n_path(n) + 8) * U * n2)
    print(f"error/bound combine n={n} m={m} first={first} use_out={use_out}: vector={r:.3g} norm={r_norm:.3g}")
    assert r <= 1.0 and r_norm <= 1.0 and np.all(parts.imag == 0.0)
    if use_out == 0:       # without norm partials: the same bits
        out2 = L.State(ctx, data=out0)
        q.combine(out2, 0, s0, first, m, coefs, None)
        assert np.array_equal(out2.numpy(), got)


# ---------------------------------------------------------------------------------------------------------------------------
# the single-GPU forms of a column, on the same bases
# ---------------------------------------------------------------------------------------------------------------------------
KNOBS = ("arnoldi_mode", "arnoldi_fuse_dots")
ALL_FORMS = ((1, 1), (1, 0), (0, 1))      # (arnoldi_mode, arnoldi_fuse_dots); the sequential passes have no second knob


def _expected_column_launches(J, mode, fuse, plain_matvec):
    """Kernel launches of one extend_arnoldi call: |q_J|^2 partials, the scaling, then column J (csrc/engine_krylov.hip:
    arnoldi_column; csrc/kernels_blas.hip: launch_mgs_lowsync)."""
    if mode == 1 and J < kr.J_TOO_LONG:
        fused = fuse == 1 and J <= 19                    # kernels_arnoldi.hip: kFusedMaxJ
        matvec_and_dots = 1 if fused else plain_matvec + 1
        return 2 + matvec_and_dots + (1 if J <= 35 else 2)     # update with the solve in its prologue | reduction (ticket) + update
    return 2 + plain_matvec + (J + 2)                     # sequential passes


def _engine_column(ctx, n, J, forms, real=False, few_values=False, dt=0.37):
    """Rows 0 .. J-1 of the Gram matrix recorded by the building blocks (V restored after each projection), then column J by
    extend_arnoldi in every form of `forms`: Hess[J, J-1] = dt |V_J|, Hess[0..J, J] and the new vector against banded.apply(V_J /
    |V_J|) followed by mgs.  The device normalises V_J itself: relative error (n_path + 8) u, carried through the bounds."""
    V = kr.make_basis(n, J, kr.delta_for(J), seed=3000 + J)
    A = kr.banded(n, kr.OFFSETS, seed=4000 + J, real=real, few_values=few_values)
    norm_J = np.sqrt(kr.dot(V[J], V[J]).real)
    rel = (kr.n_path(n) + 8) * U
    Vref = V.astype(CLD)
    Vref[J] /= norm_J
    col = kr.Column(Vref, A.apply(Vref[J]), w_err=A.row_bound(Vref[J], rel_x=rel), rel_last=rel)
    op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A.csr())], 0, L.FMT_RBCSR)
    if real:
        assert A.csr().dtype == np.float64
    if few_values:
        info = op.value_encoding_info()
        assert info["valid"] == 1, info       # the value-dictionary mirror: the CODED instances of the fused mat-vec
    xs, ys = L.State(ctx, data=V[J]), L.State(ctx, n=n)
    ctx.reset_stats()
    op.mul(xs, ys)
    plain_matvec = ctx.stats()["n_kernel_launches"]
    q = L.Krylov(ctx, n, J + 2)
    views = [q.view(i) for i in range(J + 2)]
    reduced, hess, npart = L.State(ctx, n=2 * (J + 1)), L.State(ctx, n=J + 1), L.State(ctx, n=RED)
    for i in range(J + 1):
        views[i].upload(V[i])
    for jj in range(J):
        q.multidot(jj, reduced)
        q.project(jj, dt, reduced, hess, npart)
        views[jj + 1].upload(V[jj + 1])
    saved = {k: ctx.tuning_get(k) for k in KNOBS}
    worst = {}
    try:
        for mode, fuse in forms:
            ctx.tuning_set("arnoldi_mode", mode)
            ctx.tuning_set("arnoldi_fuse_dots", fuse)
            views[J].upload(V[J])
            Hess = np.zeros((J + 2, J + 2), dtype=complex, order="F")
            ctx.reset_stats()
            assert L.extend_arnoldi(Hess, q, J + 1, op, dt)
            launches = ctx.stats()["n_kernel_launches"]
            r_sub = _ratio(abs(LD(Hess[J, J - 1].real) - dt * norm_J), rel * abs(dt) * norm_J)
            r_coefs = col.ratio_coefs(Hess[: J + 1, J].astype(CLD) / LD(dt))
            r_vec = col.ratio_vector(q.vec(J + 1))
            worst[(mode, fuse)] = (r_sub, r_coefs, r_vec)
            assert Hess[J, J - 1].imag == 0.0 and r_sub <= 1.0 and r_coefs <= 1.0 and r_vec <= 1.0, (n, J, mode, fuse, r_sub, r_coefs, r_vec)
            expected = _expected_column_launches(J, mode, fuse, plain_matvec)
            assert launches == expected, (n, J, mode, fuse, launches, expected)
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    tag = " real" if real else " few_values" if few_values else ""
    print(f"error/bound engine column n={n} J={J}{tag}: " +
          " ".join(f"mode={m},fuse={f}: subdiagonal={a:.3g} coefs={b:.3g} vector={c:.3g};" for (m, f), (a, b, c) in worst.items()))


@pytest.mark.parametrize("J", kr.COLUMN_J)
def test_engine_column_on_a_nonorthogonal_basis(ctx, J):
    """n = 4197 (one ragged row block), J at every edge of the column's forms, all three forms."""
    _engine_column(ctx, kr.COLUMN_N, J, ALL_FORMS)


@pytest.mark.parametrize("J", kr.VARIANT_J)
@pytest.mark.parametrize("variant", ("real", "few_values"))
def test_engine_column_real_and_value_dictionary_operators(ctx, variant, J):
    """The `double` instances (an all-real operator) and the CODED instances (a value dictionary) of the fused mat-vec."""
    _engine_column(ctx, kr.COLUMN_N, J, ALL_FORMS, real=variant == "real", few_values=variant == "few_values", dt=-0.8)


@pytest.mark.parametrize("J", kr.SIZE_J)
@pytest.mark.parametrize("n", kr.COLUMN_SIZES)
def test_engine_column_at_the_round_edges(ctx, n, J):
    """Rounds of 131072 rows (fused mat-vec; the update's ordered form, whose first iteration is the prefetched LAST round): one
    row short of a round, one over, a ragged round after one and after two full ones."""
    _engine_column(ctx, n, J, ((1, 1), (1, 0)))
