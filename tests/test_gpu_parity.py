"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle on
the same seeded inputs.  Tolerance for complex-fp64 results is ||delta psi||_2 < 1e-10
(BASELINE.json north_star; the reference's own bar in test/test_cheby.jl:47 and
test/test_newton.jl:65,125,175); index work is bit-exact."""
import os
import re
import sys

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import qp_oracle as qo  # noqa: E402
import qprop_amd.lib as L  # noqa: E402
import qprop_amd.synth as synth  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(params=[1, 0], ids=["lowsync_mgs", "sequential_mgs"])
def arnoldi_mode(request):
    """Both orthogonalisation schedules of the engine must meet the same parity bar."""
    L.tuning_set("arnoldi_mode", request.param)
    yield request.param
    L.tuning_set("arnoldi_mode", 1)


def _rand_state(N, rng):
    psi = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    return psi / np.linalg.norm(psi)


def _ragged(n, rng, max_len=9, empty_rows=True):
    lens = np.minimum(rng.integers(0 if empty_rows else 1, max_len + 1, n), n)
    rows = np.repeat(np.arange(n), lens)
    cols = np.concatenate([rng.choice(n, l, replace=False) for l in lens]) if lens.sum() else np.zeros(0, int)
    vals = rng.standard_normal(len(rows)) + 1j * rng.standard_normal(len(rows))
    A = sp.csr_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


# ---------------------------------------------------------------- index work / formats

@pytest.mark.parametrize("fmt", [L.FMT_RBCSR, L.FMT_CSR])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 1000])
def test_device_format_roundtrip_bit_exact(ctx, fmt, n):
    rng = np.random.default_rng(n)
    A = _ragged(n, rng)
    M = L.Matrix.from_scipy(ctx, A.tocsc())          # CSC in, like Julia
    rp, col, vals = M.get_csr()
    assert np.array_equal(rp, A.indptr) and np.array_equal(col, A.indices) and np.array_equal(vals, A.data)
    Op = L.Operator(ctx, [M], 0, fmt)
    assert Op.format == fmt
    rp, col, vals = Op.get_csr()
    assert np.array_equal(rp, A.indptr) and np.array_equal(col, A.indices) and np.array_equal(vals, A.data)


@pytest.mark.parametrize("fmt", [L.FMT_HRB, L.FMT_RBCSR, L.FMT_CSR])
def test_large_value_plane_roundtrip_bit_exact(ctx, fmt):
    """A value plane of more than 256 MiB goes to the device in 64-MiB chunks through two pinned buffers while the host threads lay
    out the next chunk (engine_operator.hip: upload_plane_staged), and `qp_matrix_create` copies and checks its arrays on the
    host threads: the read-back of every device format reproduces the input bit for bit (N = 2^21 + 77 rows, 16 entries per row --
    a ragged last row block and a last chunk that is not full)."""
    N = (1 << 21) + 77
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4, 1000, 2000, 3000, 4001))
    M = L.Matrix(ctx, N, N, rp, col, vals)
    r0, c0, v0 = M.get_csr()
    assert np.array_equal(r0, rp) and np.array_equal(c0, col) and np.array_equal(v0, vals)
    Op = L.Operator(ctx, [M], 0, fmt)
    assert Op.format == fmt
    r1, c1, v1 = Op.get_csr()
    assert np.array_equal(r1, rp) and np.array_equal(c1, col) and np.array_equal(v1, vals)
    psi0 = synth.random_state(N, seed=4)                     # ... and the mat-vec on it: mul! against SciPy
    x, y = L.State(ctx, data=psi0), L.State(ctx, data=psi0)
    Op.mul(x, y)
    assert np.linalg.norm(y.numpy() - synth.to_scipy(rp, col, vals, N) @ psi0) < 1e-12


def _ragged_hermitian(n, rng):
    A = _ragged(n, rng, max_len=5)
    A = (A + A.conj().T).tocsr()
    A.setdiag(rng.standard_normal(n))
    A.sort_indices()
    return A


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 200, 1000])
def test_hermitian_packed_roundtrip_bit_exact(ctx, n):
    """HRB stores only col >= row; the read-back must reproduce the full matrix bit for bit."""
    rng = np.random.default_rng(100 + n)
    A = _ragged_hermitian(n, rng)
    M = L.Matrix.from_scipy(ctx, A)
    Op = L.Operator(ctx, [M], 0, L.FMT_HRB)
    assert Op.format == L.FMT_HRB
    rp, col, vals = Op.get_csr()
    assert np.array_equal(rp, A.indptr) and np.array_equal(col, A.indices) and np.array_equal(vals, A.data)
    B = A.copy()
    if B.nnz > 1 and n > 2:
        B.data[0] += 1e-17j + 1e-3                 # break Hermiticity in one entry
        if abs(B - B.conj().T).max() > 0:
            assert L.Operator(ctx, [L.Matrix.from_scipy(ctx, B)]).format in (L.FMT_RBCSR, L.FMT_CSR)
            with pytest.raises(L.QPArgumentError, match="not exactly Hermitian"):
                L.Operator(ctx, [L.Matrix.from_scipy(ctx, B)], 0, L.FMT_HRB)


def test_hermitian_packed_operator_sum(ctx):
    """Lazy sum of Hermitian terms in HRB: real coefficients stay packed, a complex
    coefficient re-lays the operator out as RBCSR (slow path) with identical results."""
    rng = np.random.default_rng(23)
    N = 300
    mats = [_ragged_hermitian(N, rng) for _ in range(3)]
    psi, phi0 = _rand_state(N, rng), _rand_state(N, rng)
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A) for A in mats], 2, L.FMT_HRB)
    assert Op.format == L.FMT_HRB
    x = L.State(ctx, data=psi)
    for coeffs in ([0.3, -1.2], [1.0, 1.0], [0.7, 0.1 + 0.2j], [2.0, -0.5]):
        Op.set_coeffs(coeffs)
        ref = qo.Operator(mats, coeffs)
        y = L.State(ctx, data=phi0)
        Op.mul(x, y, 0.5 - 1j, 0.25j)
        assert np.linalg.norm(y.numpy() - ref.mul(psi, 0.5 - 1j, 0.25j, C=phi0.copy())) < 1e-12
        rp, col, vals = Op.get_csr()
        dense = sp.csr_matrix((vals, col, rp), shape=(N, N)).toarray()
        assert np.linalg.norm(dense - ref.toarray()) < 1e-12
    Op._refresh_info()
    assert Op.format in (L.FMT_RBCSR, L.FMT_CSR)   # left the packed format at the complex coefficient


@pytest.mark.parametrize("fmt", [L.FMT_HRB, L.FMT_RBCSR])
def test_column_delta_encoding_roundtrip_and_parity(ctx, fmt):
    """Row blocks whose columns are all within +-32767 of their row store int16 deltas, the
    others int32 columns; a matrix with both kinds of blocks must round-trip bit-exactly and
    multiply correctly (N > 2^16 so that far and wrap-around couplings overflow int16)."""
    N = 1 << 17
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 40000))   # 40000 > 32767: every block int32
    rp2, col2, vals2 = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 30000))  # interior int16, wrap blocks int32
    rng = np.random.default_rng(5)
    x = _rand_state(N, rng)
    for (a, b, c) in ((rp, col, vals), (rp2, col2, vals2)):
        Op = L.Operator(ctx, [L.Matrix(ctx, N, N, a, b, c)], 0, fmt)
        r_, c_, v_ = Op.get_csr()
        assert np.array_equal(r_, a) and np.array_equal(c_, b) and np.array_equal(v_, c)
        y = L.State(ctx, n=N)
        Op.mul(L.State(ctx, data=x), y)
        assert np.linalg.norm(y.numpy() - synth.to_scipy(a, b, c, N) @ x) < 1e-12


def test_operator_auto_format(ctx):
    rp, col, vals = synth.hermitian_offsets_csr(512, offsets=(1, 2, 3, 4, 16, 32, 48, 64))
    Op = L.Operator(ctx, [L.Matrix(ctx, 512, 512, rp, col, vals)])
    assert Op.format == L.FMT_HRB            # the synthetic H is exactly Hermitian and banded
    rs, cs, vs = synth.hermitian_offsets_csr(1 << 16, offsets=synth.scattered_offsets(1 << 16))
    assert L.Operator(ctx, [L.Matrix(ctx, 1 << 16, 1 << 16, rs, cs, vs)]).format == L.FMT_RBCSR   # no L2 locality
    assert L.Operator(ctx, [L.Matrix(ctx, 512, 512, rp, col, vals)], 0, L.FMT_RBCSR).format == L.FMT_RBCSR
    rng = np.random.default_rng(0)
    lens = np.ones(512, int)
    lens[::64] = 60     # one long row per block: padding would be ~30x
    rows = np.repeat(np.arange(512), lens)
    cols = np.concatenate([rng.choice(512, l, replace=False) for l in lens])
    A = sp.csr_matrix((np.ones(len(rows), complex), (rows, cols)), shape=(512, 512))
    assert L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)]).format == L.FMT_CSR


# ---------------------------------------------------------------- mul! / BLAS-1

@pytest.mark.parametrize("fmt", [L.FMT_RBCSR, L.FMT_CSR])
def test_operator_mul(ctx, fmt):
    """test/test_operator_linalg.jl:30-64 on the device: mul!(phi, Op, psi, a, b) for
    (1,0),(1,1),(2,1),(2,2), drift + 2 controls and no drift, ScaledOperator."""
    rng = np.random.default_rng(21)
    N = 300
    mats = [_ragged(N, rng, empty_rows=(i == 0)) for i in range(3)]
    psi, phi0 = _rand_state(N, rng), _rand_state(N, rng)
    dmats = [L.Matrix.from_scipy(ctx, A) for A in mats]
    for ops, dops, coeffs in ((mats, dmats, [0.3, -1.2 + 0.4j]), (mats[1:], dmats[1:], [0.7, 0.1 + 0.2j])):
        ref = qo.Operator(ops, coeffs)
        Op = L.Operator(ctx, dops, len(coeffs), fmt)
        Op.set_coeffs(coeffs)
        x = L.State(ctx, data=psi)
        for alpha, beta in ((1, 0), (1, 1), (2, 1), (2, 2), (0.5 - 1j, 0.25j)):
            y = L.State(ctx, data=phi0)
            Op.mul(x, y, alpha, beta)
            assert np.linalg.norm(y.numpy() - ref.mul(psi, alpha, beta, C=phi0.copy())) < 1e-12
        Op.set_scale(0.5j)
        y = L.State(ctx, data=phi0)
        Op.mul(x, y, 2, 1)
        assert np.linalg.norm(y.numpy() - qo.ScaledOperator(0.5j, ref).mul(psi, 2, 1, C=phi0.copy())) < 1e-12
        Op.set_scale(1.0)
        # device copy of the combined values == sum_l c_l H_l on the union pattern
        rp, col, vals = Op.get_csr()
        dense = sp.csr_matrix((vals, col, rp), shape=(N, N)).toarray()
        assert np.linalg.norm(dense - ref.toarray()) < 1e-12


def test_blas1(ctx):
    rng = np.random.default_rng(22)
    for n in (1, 255, 256, 70001):
        x, y = _rand_state(n, rng), _rand_state(n, rng)
        X, Y = L.State(ctx, data=x), L.State(ctx, data=y)
        assert abs(X.dot(Y) - np.vdot(x, y)) < 1e-13
        assert abs(X.norm() - np.linalg.norm(x)) < 1e-13
        Y.axpy(0.3 - 2j, X)
        y = y + (0.3 - 2j) * x
        assert np.linalg.norm(Y.numpy() - y) < 1e-13
        Y.scal(1j)
        assert np.linalg.norm(Y.numpy() - 1j * y) < 1e-13
        Y.copy_from(X)
        assert np.array_equal(Y.numpy(), x)
        Y.fill(2 - 1j)
        assert np.all(Y.numpy() == 2 - 1j)


# ---------------------------------------------------------------- Chebyshev

def _cheby_case(ctx, H_sp, psi0, Delta, E_min, dt, fmt, steps=1, check=False):
    N = len(psi0)
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H_sp)], 0, fmt)
    wrk = L.ChebyWrk(ctx, N, Delta, E_min, abs(dt))
    owrk = qo.ChebyWrk(psi0, Delta, E_min, abs(dt))
    owrk.coeffs, owrk.n_coeffs = wrk.coeffs.copy(), wrk.n_coeffs   # identical coefficients
    psi = L.State(ctx, data=psi0)
    ref = psi0.copy()
    for _ in range(steps):
        L.cheby(psi, Op, dt, wrk, check_normalization=check)
        qo.cheby(ref, H_sp, dt, owrk)
    return psi.numpy(), ref, wrk


@pytest.mark.parametrize("fmt", [L.FMT_HRB, L.FMT_RBCSR, L.FMT_CSR])
def test_cheby_dense_c1(ctx, fmt):
    """BASELINE config C1: N=128 dense random Hermitian, 200 time steps, vs oracle and
    vs exp(-i H t)."""
    rng = np.random.default_rng(31)
    N = 128
    H = synth.dense_hermitian(N, rho=5.0, rng=rng)
    ev = np.linalg.eigvalsh(H)
    psi0 = _rand_state(N, rng)
    dt = 0.1
    out, ref, wrk = _cheby_case(ctx, sp.csr_matrix(H), psi0, ev[-1] - ev[0], ev[0], dt, fmt, steps=200)
    assert np.linalg.norm(out - ref) < TOL
    V = np.linalg.eigh(H)[1]
    exact = V @ (np.exp(-1j * ev * dt * 200) * (V.conj().T @ psi0))
    assert np.linalg.norm(out - exact) < 1e-9
    assert abs(np.linalg.norm(out) - 1) < 1e-10


@pytest.mark.parametrize("fmt", [L.FMT_HRB, L.FMT_RBCSR, L.FMT_CSR])
@pytest.mark.parametrize("N", [256, 1000, 16384])
@pytest.mark.parametrize("dt", [1.0, -1.0])
def test_cheby_synthetic(ctx, fmt, N, dt):
    """Same generator as BASELINE config C2 at oracle-sized N; forward and backward."""
    offs = (1, 2, 3, 4, 16, 32, 48, 64) if N < 16384 else synth.BANDED_OFFSETS
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=offs)
    H = synth.to_scipy(rp, col, vals, N)
    psi0 = synth.random_state(N)
    out, ref, wrk = _cheby_case(ctx, H, psi0, 20.0, -10.0, dt, fmt, steps=3)
    assert wrk.n_coeffs == 32
    assert np.linalg.norm(out - ref) < TOL
    assert abs(np.linalg.norm(out) - 1) < 1e-11


@pytest.mark.parametrize("alpha", [1e-13, 0.4, 50.0])
def test_cheby_coefficient_count_edges(ctx, alpha):
    """n_coeffs = 2 (single fused term, result copied back), odd/even term counts."""
    N = 300
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 5, 7, 30))
    H = synth.to_scipy(rp, col, vals, N)
    psi0 = synth.random_state(N)
    dt = alpha / 10.0
    out, ref, wrk = _cheby_case(ctx, H, psi0, 20.0, -10.0, dt, L.FMT_AUTO, steps=2)
    if alpha < 1e-6:
        assert wrk.n_coeffs == 2     # a_2 = 2 J_1(alpha) <= 1e-12 is the first one kept-and-stopped
    assert np.linalg.norm(out - ref) < TOL


def test_cheby_errors(ctx):
    N = 128
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4))
    Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)])
    psi = L.State(ctx, data=synth.random_state(N))
    wrk = L.ChebyWrk(ctx, N, 20.0, -10.0, 1.0)
    with pytest.raises(L.QPAssertionError, match="wrk was initialized for dt"):   # src/cheby.jl:157
        L.cheby(psi, Op, 0.5, wrk)
    # src/cheby.jl:194-200: spectrum outside [E_min, E_min + Delta] -> "Incorrect normalization"
    # (the check is a Rayleigh quotient, so use a one-sided violation; the oracle trips too)
    wrk2 = L.ChebyWrk(ctx, N, 0.5, 3.0, 1.0)
    with pytest.raises(L.QPAssertionError, match="Incorrect normalization"):
        L.cheby(psi, Op, 1.0, wrk2, check_normalization=True)
    H = synth.to_scipy(rp, col, vals, N)
    with pytest.raises(AssertionError, match="Incorrect normalization"):
        qo.cheby(synth.random_state(N), H, 1.0, qo.ChebyWrk(synth.random_state(N), 0.5, 3.0, 1.0),
                 check_normalization=True)
    # and a correct radius passes the check
    psi.upload(synth.random_state(N))
    L.cheby(psi, Op, 1.0, wrk, check_normalization=True)
    assert abs(psi.norm() - 1) < 1e-11


def test_cheby_deterministic(ctx):
    """check_propagator's reinit test needs run-to-run reproducibility (1e-14); the
    kernels use no atomics, so results are bitwise identical."""
    N = 4096
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4, 16, 32, 48, 64))
    Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)])
    wrk = L.ChebyWrk(ctx, N, 20.0, -10.0, 1.0)
    outs = []
    for _ in range(2):
        psi = L.State(ctx, data=synth.random_state(N))
        L.cheby(psi, Op, 1.0, wrk)
        outs.append(psi.numpy())
    assert np.array_equal(outs[0], outs[1])


def test_cheby_term_row_partition(ctx):
    """The multi-GPU building block on one GPU: two row shards in local numbering (own
    columns + ghost slots, Hermitian-packed square part), each running qp_cheby_term on
    its rows; the "all-gather" of the send slabs goes through the host.  Must reproduce
    the unsharded step."""
    import qprop_amd.sharded as sharded
    N = 1000
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4, 16, 32, 48, 64))
    H = synth.to_scipy(rp, col, vals, N)
    psi0 = synth.random_state(N)
    Delta, E_min, dt = 20.0, -10.0, 1.0
    a = L.cheby_coeffs(Delta, dt)
    beta = Delta / 2 + E_min
    bounds = L.partition_rows(rp, 2)
    G = 2
    blocks = [(int(bounds[r]), int(bounds[r + 1])) for r in range(G)]
    wanted = [sharded.split_by_owner(sharded.remote_columns(col[rp[r0]:rp[r1]], r0, r1), bounds) for r0, r1 in blocks]
    send_lists = [np.unique(np.concatenate([w[o] for w in wanted if o in w])) for o in range(G)]
    M = max(len(s) for s in send_lists)
    shards = []
    for (r0, r1) in blocks:
        nloc = r1 - r0
        lcol = sharded.remap_columns(col[rp[r0]:rp[r1]], r0, r1, bounds, send_lists, M)
        Op = L.Operator(ctx, [L.Matrix(ctx, nloc, nloc + G * M, rp[r0:r1 + 1] - rp[r0], lcol, vals[rp[r0]:rp[r1]])])
        assert Op.format == L.FMT_HRB          # the local square part stays Hermitian-packed
        X = [L.State(ctx, n=nloc + G * M), L.State(ctx, n=nloc + G * M)]
        shards.append(dict(r0=r0, r1=r1, nloc=nloc, Op=Op, X=X, acc=L.State(ctx, n=nloc)))

    def exchange(k):
        slabs = np.zeros((G, M), dtype=complex)
        hosts = [sh["X"][k].numpy() for sh in shards]
        for o, sh in enumerate(shards):
            idx = send_lists[o] - sh["r0"]
            slabs[o, :len(idx)] = hosts[o][idx]
        for o, sh in enumerate(shards):
            hosts[o][sh["nloc"]:] = slabs.reshape(-1)
            sh["X"][k].upload(hosts[o])

    for sh in shards:
        h = np.zeros(sh["nloc"] + G * M, dtype=complex)
        h[:sh["nloc"]] = psi0[sh["r0"]:sh["r1"]]
        sh["X"][0].upload(h)
    exchange(0)
    c = -2j / Delta
    n = len(a)
    for m in range(1, n):
        xi, oi = (0, 1) if m % 2 == 1 else (1, 0)
        last = m == n - 1
        phase = np.exp(-1j * beta * dt) if last else 1.0
        for sh in shards:
            nloc = sh["nloc"]
            oloc = L.State(ctx, n=nloc, device_ptr=sh["X"][oi].ptr, keepalive=sh["X"][oi])
            if m == 1:
                L.cheby_term(sh["Op"], sh["X"][xi], 0, None, oloc, None, sh["acc"], c, beta, a[0], a[1], phase)
            else:
                L.cheby_term(sh["Op"], sh["X"][xi], 0, oloc, None if last else oloc, sh["acc"], sh["acc"], c, beta,
                             0.0, a[m], phase)
        if not last:
            exchange(oi)
        if m == 1:
            c = 2 * c
    out = np.concatenate([sh["acc"].numpy() for sh in shards])
    wrk = qo.ChebyWrk(psi0, Delta, E_min, dt)
    wrk.coeffs, wrk.n_coeffs = a, len(a)
    ref = qo.cheby(psi0.copy(), H, dt, wrk)
    assert np.linalg.norm(out - ref) < TOL


@pytest.mark.parametrize("fmt", [L.FMT_HRB, L.FMT_RBCSR, L.FMT_CSR])
@pytest.mark.parametrize("batch", [1, 5, 64, 70])
def test_cheby_batched_matches_oracle(ctx, fmt, batch):
    """BASELINE configs[4] at oracle size: a panel of `batch` states through the SpMM path
    equals `batch` independent oracle propagations; forward and backward; any device format
    (the CSR-ordered mirror is gathered from the device values, conj-transposed for HRB)."""
    N = 777
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4, 16, 32, 48, 64))
    H = synth.to_scipy(rp, col, vals, N)
    Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)], 0, fmt)
    states = np.stack([synth.random_state(N, seed=1000 + s) for s in range(batch)], axis=1)   # [N, batch]
    wrk = L.ChebyWrk(ctx, N * batch, 20.0, -10.0, 0.7)
    panel = L.State(ctx, data=states.reshape(-1))
    for dt in (0.7, 0.7, -0.7):
        L.cheby_batched(panel, Op, dt, wrk, batch)
    out = panel.numpy().reshape(N, batch)
    for s in range(batch):
        owrk = qo.ChebyWrk(states[:, s], 20.0, -10.0, 0.7)
        owrk.coeffs, owrk.n_coeffs = wrk.coeffs.copy(), wrk.n_coeffs
        ref = states[:, s].copy()
        for dt in (0.7, 0.7, -0.7):
            qo.cheby(ref, H, dt, owrk)
        assert np.linalg.norm(out[:, s] - ref) < TOL


def test_cheby_batched_tracks_coefficients(ctx):
    """The CSR mirror follows qp_operator_set_coeffs (device-side `evaluate!`)."""
    rng = np.random.default_rng(77)
    N, batch = 200, 8
    H0 = synth.dense_hermitian(N, rho=2.0, rng=rng)
    H1 = synth.dense_hermitian(N, rho=1.0, rng=rng)
    Op = L.Operator(ctx, [L.Matrix.from_dense(ctx, H0), L.Matrix.from_dense(ctx, H1)], 1)
    states = np.stack([_rand_state(N, rng) for _ in range(batch)], axis=1)
    wrk = L.ChebyWrk(ctx, N * batch, 12.0, -6.0, 0.2)
    panel = L.State(ctx, data=states.reshape(-1))
    ref = states.copy()
    for cval in (0.5, -1.0, 0.25):
        Op.set_coeffs([cval])
        L.cheby_batched(panel, Op, 0.2, wrk, batch)
        for s in range(batch):
            owrk = qo.ChebyWrk(ref[:, s], 12.0, -6.0, 0.2)
            owrk.coeffs, owrk.n_coeffs = wrk.coeffs.copy(), wrk.n_coeffs
            col_ = ref[:, s].copy()
            qo.cheby(col_, H0 + cval * H1, 0.2, owrk)
            ref[:, s] = col_
    assert np.linalg.norm(panel.numpy().reshape(N, batch) - ref) < TOL


# ---------------------------------------------------------------- Arnoldi / Newton / specrange

def test_arnoldi_matches_oracle(ctx, arnoldi_mode):
    rng = np.random.default_rng(41)
    N, m, dt = 500, 12, 0.37
    A = synth.sparse_random(N, 0.03, rng=rng)
    psi = _rand_state(N, rng)
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)])
    for extended in (True, False):
        q = L.Krylov(ctx, N, m + 1)
        Hess = np.zeros((m + 1, m + 1), dtype=complex, order="F")
        m_out = L.arnoldi(Hess, q, m, L.State(ctx, data=psi), Op, dt, extended=extended)
        Href = np.zeros((m + 1, m + 1), dtype=complex)
        qref = [np.empty(N, dtype=complex) for _ in range(m + 1)]
        m_ref = qo.arnoldi(Href, qref, m, psi, A, dt, extended=extended)
        assert m_out == m_ref == m
        assert np.max(np.abs(Hess - Href)) < 1e-12
        for i in range(m + 1):
            assert np.linalg.norm(q.vec(i) - qref[i]) < 1e-11
        if not extended:   # extend_arnoldi! by one column (src/arnoldi.jl:115-129)
            q2 = L.Krylov(ctx, N, m + 2)
            H2 = np.zeros((m + 1, m + 1), dtype=complex, order="F")
            L.arnoldi(H2, q2, m, L.State(ctx, data=psi), Op, dt, extended=False)
            assert L.extend_arnoldi(H2, q2, m + 1, Op, dt)
            Href2 = np.zeros((m + 1, m + 1), dtype=complex)
            qref2 = [np.empty(N, dtype=complex) for _ in range(m + 2)]
            qo.arnoldi(Href2, qref2, m, psi, A, dt, extended=False)
            qo.extend_arnoldi(Href2, qref2, m + 1, A, dt)
            assert np.max(np.abs(H2 - Href2)) < 1e-12


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real_copy"])
def test_arnoldi_fused_dots_matches_oracle_and_unfused(ctx, real):
    """Knob `arnoldi_fuse_dots` (kernels_arnoldi.hip): the mat-vec of an Arnoldi column also accumulates the column's dot
    products c_k = <q_k|w> and its Gram row -- 2 launches per column instead of 3 while j <= 19, the unfused pair beyond.
    Same Hessenberg matrix and basis as the oracle and as the unfused kernels (different summation order: 1e-12), on a
    ragged N whose row blocks do not fill the 2048 wavefronts of the launch, for complex values and for the real copy."""
    rng = np.random.default_rng(77)
    N, m, dt = 20000 + 37, 24, 0.21
    A = synth.sparse_random(N, 6.0 / N, rng=rng)
    if real:
        A = sp.csr_matrix(A.real.astype(complex))
    psi = _rand_state(N, rng)
    saved = {k: ctx.tuning_get(k) for k in ("small_nnz", "arnoldi_fuse_dots", "arnoldi_mode")}
    try:
        ctx.tuning_set("small_nnz", 0)
        ctx.tuning_set("arnoldi_mode", 1)
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)], 0, L.FMT_RBCSR)
        res = {}
        for fuse in (1, 0):
            ctx.tuning_set("arnoldi_fuse_dots", fuse)
            q = L.Krylov(ctx, N, m + 1)
            Hess = np.zeros((m + 1, m + 1), dtype=complex, order="F")
            ctx.sync()
            ctx.reset_stats()
            assert L.arnoldi(Hess, q, m, L.State(ctx, data=psi), Op, dt, extended=True) == m
            res[fuse] = (Hess, [q.vec(i) for i in range(m + 1)], ctx.stats()["n_kernel_launches"])
        Href = np.zeros((m + 1, m + 1), dtype=complex)
        qref = [np.empty(N, dtype=complex) for _ in range(m + 1)]
        assert qo.arnoldi(Href, qref, m, psi, A, dt, extended=True) == m
        for fuse in (1, 0):
            assert np.max(np.abs(res[fuse][0] - Href)) < 1e-12
            for i in range(m + 1):
                assert np.linalg.norm(res[fuse][1][i] - qref[i]) < 1e-11
        assert res[0][2] - res[1][2] == 20          # one launch less for each of the columns j = 0 .. 19
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)


def test_arnoldi_breakdown(ctx, arnoldi_mode):
    """Krylov dimension smaller than m: reduced m is returned (src/arnoldi.jl:91-95),
    also for negative dt."""
    N = 64
    d = np.arange(1, N + 1, dtype=float)
    A = sp.diags([d], [0], format="csr", dtype=complex)
    psi = np.zeros(N, dtype=complex)
    psi[[3, 10, 20]] = 1 / np.sqrt(3)        # Krylov dimension 3
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)])
    for dt in (1.0, -1.0):
        q = L.Krylov(ctx, N, 9)
        Hess = np.zeros((9, 9), dtype=complex, order="F")
        m_out = L.arnoldi(Hess, q, 8, L.State(ctx, data=psi), Op, dt, norm_min=1e-10)
        Href = np.zeros((9, 9), dtype=complex)
        qref = [np.empty(N, dtype=complex) for _ in range(9)]
        m_ref = qo.arnoldi(Href, qref, 8, psi, A, dt, norm_min=1e-10)
        assert m_out == m_ref == 3
        assert np.max(np.abs(Hess[:, :3] - Href[:, :3])) < 1e-9
        assert np.all(Hess[:, 3:] == 0)


def _newton_case(ctx, A, psi0, dt, m_max, func=None, **kw):
    N = len(psi0)
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, sp.csr_matrix(A))])
    wrk = L.NewtonWrk(ctx, N, m_max=m_max)
    psi = L.State(ctx, data=psi0)
    L.newton(psi, Op, dt, wrk, func=func, **kw)
    owrk = qo.NewtonWrk(psi0, m_max=m_max)
    pyf = {None: None, "exp": np.exp}.get(func, func)
    ref = qo.newton(psi0.copy(), A, dt, owrk, func=pyf, **kw)
    return psi.numpy(), ref, wrk, owrk


def test_newton_hermitian(ctx, arnoldi_mode):
    """test/test_newton.jl:7-67: N=1000 Hermitian rho=10, dt=0.5, m_max=5, 200 restarts."""
    rng = np.random.default_rng(42)
    N = 1000
    H = synth.dense_hermitian(N, rho=10.0, rng=rng)
    psi0 = _rand_state(N, rng)
    out, ref, wrk, owrk = _newton_case(ctx, H, psi0, 0.5, 5, max_restarts=200)
    ev, V = np.linalg.eigh(H)
    exact = V @ (np.exp(-1j * ev * 0.5) * (V.conj().T @ psi0))
    assert np.linalg.norm(out - exact) < TOL
    assert np.linalg.norm(out - ref) < TOL
    assert abs(wrk.restarts - owrk.restarts) <= 1
    assert abs(np.linalg.norm(out) - 1) < 1e-10


def test_newton_nonhermitian(ctx, arnoldi_mode):
    """test/test_newton.jl:70-127: non-Hermitian rho=10, m_max=50; backward too."""
    rng = np.random.default_rng(43)
    N = 1000
    H = synth.dense_nonhermitian(N, rho=10.0, rng=rng)
    psi0 = _rand_state(N, rng)
    for dt in (0.5, -0.5):
        out, ref, wrk, owrk = _newton_case(ctx, H, psi0, dt, 50, max_restarts=200)
        assert np.linalg.norm(out - sla.expm(-1j * H * dt) @ psi0) < TOL * max(1, np.linalg.norm(ref))
        assert np.linalg.norm(out - ref) < TOL * max(1, np.linalg.norm(ref))


@pytest.mark.parametrize("func", ["exp", "callback"])
def test_newton_liouvillian_custom_func(ctx, func):
    """test/test_newton.jl:130-177: sparse L (32^2), density 0.5, m_max=50,
    func = exp (built in, and through the C callback), max_restarts=20."""
    rng = np.random.default_rng(44)
    n = 32
    Lm = synth.sparse_random(n * n, 0.5, rho=10.0, rng=rng)
    psi0 = _rand_state(n, rng)
    rho0 = np.outer(psi0, psi0.conj()).reshape(-1, order="F")
    f = "exp" if func == "exp" else (lambda z: np.exp(z))
    N = n * n
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, Lm)])
    wrk = L.NewtonWrk(ctx, N, m_max=50)
    rho = L.State(ctx, data=rho0)
    L.newton(rho, Op, 0.5, wrk, func=f, max_restarts=20)
    assert np.linalg.norm(rho.numpy() - sla.expm(Lm.toarray() * 0.5) @ rho0) < TOL


def test_newton_c3_liouvillian(ctx, arnoldi_mode):
    """BASELINE config C3 at oracle size: tridiagonal-system Liouvillian (n=24 -> N=576),
    m_max=20, several restarts; vs oracle and dense exp."""
    Lm = synth.liouvillian_tridiag(24)
    N = Lm.shape[0]
    rho0 = synth.random_state(N)
    out, ref, wrk, owrk = _newton_case(ctx, Lm, rho0, 0.8, 20)
    assert np.linalg.norm(out - ref) < TOL
    assert np.linalg.norm(out - sla.expm(-1j * Lm.toarray() * 0.8) @ rho0) < TOL
    assert wrk.restarts >= 1 and abs(wrk.restarts - owrk.restarts) <= 1
    a, leja = wrk.coeffs()
    n = min(len(a), owrk.n_a)
    assert np.max(np.abs(leja[:n] - owrk.leja[:n])) < 1e-8   # same Leja ordering


def test_newton_eigenstate_and_errors(ctx):
    rng = np.random.default_rng(45)
    H = synth.dense_hermitian(50, rho=4.0, rng=rng)
    ev, V = np.linalg.eigh(H)
    Op = L.Operator(ctx, [L.Matrix.from_dense(ctx, H)])
    wrk = L.NewtonWrk(ctx, 50, m_max=10)
    psi = L.State(ctx, data=V[:, 3])
    L.newton(psi, Op, 0.7, wrk)                      # src/newton.jl:289-295
    assert wrk.restarts == 0
    assert np.linalg.norm(psi.numpy() - np.exp(-1j * ev[3] * 0.7) * V[:, 3]) < 1e-12
    with pytest.raises(L.QPArgumentError, match="m_max > 2"):   # src/newton.jl:38-40
        L.NewtonWrk(ctx, 50, m_max=2)
    psi = L.State(ctx, data=_rand_state(50, rng))
    with pytest.raises(L.QPAssertionError):                    # src/newton.jl:375
        L.newton(psi, Op, 50.0, L.NewtonWrk(ctx, 50, m_max=3), max_restarts=1)


def test_ritzvals_and_specrange(ctx, arnoldi_mode):
    """test/test_specrad.jl:47-144 on the device, vs oracle (same start vector) and
    vs exact eigenvalues."""
    rng = np.random.default_rng(46)
    N = 1000
    H = synth.sparse_random(N, 0.1, rho=10.0, hermitian=True, rng=rng)
    ev = np.linalg.eigvalsh(H.toarray())
    Delta = ev[-1] - ev[0]
    psi = _rand_state(N, rng)
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)])
    st = L.State(ctx, data=psi)
    r_dev = L.ritzvals(Op, st, 20, 60, prec=1e-3)
    r_ref = qo.ritzvals(H, psi, 20, 60, prec=1e-3)
    assert len(r_dev) == len(r_ref)
    assert np.max(np.abs(r_dev - r_ref)) < 1e-8
    assert abs(ev[0] - r_dev[0].real) / abs(ev[0]) < 0.02 and abs(ev[-1] - r_dev[-1].real) / abs(ev[-1]) < 0.02
    E_min, E_max = L.specrange_arnoldi(Op, st, prec=1e-4)
    o_min, o_max = qo.specrange(H, "arnoldi", state=psi, prec=1e-4)
    assert abs(E_min - o_min) < 1e-8 and abs(E_max - o_max) < 1e-8
    assert ev[0] - 0.05 * Delta <= E_min <= ev[0]
    assert ev[-1] <= E_max < ev[-1] + 0.05 * Delta


# ---------------------------------------------------------------- full-size properties

def test_full_size_properties(ctx):
    """BASELINE config C2 at full size (N = 2^20, 16 nnz/row): size-independent properties --
    unitarity (norm), forward/backward round trip, linearity, agreement of the three device formats --
    and, since two steps cost the C restatement of the reference's serial CSC path
    (oracle/cheby_ref.c) only a second or two, a direct comparison with it at the full size."""
    from oracle import ref_c
    N = 1 << 20
    rp, col, vals = synth.hermitian_offsets_csr(N)
    M = L.Matrix(ctx, N, N, rp, col, vals)
    psi0 = synth.random_state(N)
    wrk = L.ChebyWrk(ctx, N, 20.0, -10.0, 1.0)
    assert wrk.n_coeffs == 32
    cref = psi0.copy()
    for _ in range(2):    # Hermitian H: CSC(H) = conj CSR(H)
        ref_c.cheby_csc(rp, col.astype(np.int64), np.conj(vals), cref, wrk.coeffs, 20.0, -10.0, 1.0)
    del rp, col, vals
    res = {}
    for fmt in (L.FMT_HRB, L.FMT_RBCSR, L.FMT_CSR):
        Op = L.Operator(ctx, [M], 0, fmt)
        psi = L.State(ctx, data=psi0)
        L.cheby(psi, Op, 1.0, wrk)
        L.cheby(psi, Op, 1.0, wrk)
        res[fmt] = psi.numpy()
        assert abs(np.linalg.norm(res[fmt]) - 1) < 1e-11
        assert np.linalg.norm(res[fmt] - cref) < TOL, fmt          # the oracle at the full BASELINE size
        L.cheby(psi, Op, -1.0, wrk)
        L.cheby(psi, Op, -1.0, wrk)
        assert np.linalg.norm(psi.numpy() - psi0) < TOL
        if fmt == L.FMT_HRB:        # linearity: U(a x + b y) = a U x + b U y
            y0 = synth.random_state(N, seed=77)
            a, b = 0.6 - 0.3j, -0.2 + 0.9j
            Y = L.State(ctx, data=y0)
            L.cheby(Y, Op, 1.0, wrk)
            L.cheby(Y, Op, 1.0, wrk)
            Z = L.State(ctx, data=a * psi0 + b * y0)
            L.cheby(Z, Op, 1.0, wrk)
            L.cheby(Z, Op, 1.0, wrk)
            assert np.linalg.norm(Z.numpy() - (a * res[fmt] + b * Y.numpy())) < TOL
        Op.close()
    assert np.linalg.norm(res[L.FMT_RBCSR] - res[L.FMT_CSR]) < TOL
    assert np.linalg.norm(res[L.FMT_HRB] - res[L.FMT_RBCSR]) < TOL


def test_hrb_kernel_variants_bit_identical(ctx):
    """Knob rbcsr_variant of the Hermitian-packed kernel: nontemporal index loads, early row-local loads, unroll
    depth and (bit 3, the default) the straight-line path that issues all 32 loads of an all-stencil block before
    the first FMA change the schedule of the loads only -- every variant gives the same bits (variant 15 runs eight row blocks per
    workgroup, the others four).  N is not a multiple of 8 x 64 rows: a partly filled workgroup."""
    N = (1 << 15) + 192
    rp, col, vals = synth.hermitian_offsets_csr(N)        # lattice: stencil blocks except at the wrap-around
    Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)], 0, L.FMT_HRB)
    lay = Op.layout_info()
    assert lay["stencil_lower_blocks"] > 0.75 * lay["blocks"]      # all but the blocks next to the periodic wrap
    psi0 = synth.random_state(N)
    wrk = L.ChebyWrk(ctx, N, 20.0, -10.0, 1.0)
    outs = {}
    try:
        for v in (15, 31, 7, 3, 0, 8):
            ctx.tuning_set("rbcsr_variant", v)
            psi = L.State(ctx, data=psi0)
            L.cheby(psi, Op, 1.0, wrk)
            L.cheby(psi, Op, -1.0, wrk)
            L.cheby(psi, Op, 1.0, wrk)
            outs[v] = psi.numpy()
    finally:
        ctx.tuning_set("rbcsr_variant", 15)
    assert all(np.array_equal(outs[15], o) for o in outs.values())
    H = synth.to_scipy(rp, col, vals, N)
    ref = qo.cheby(psi0.copy(), H, 1.0, qo.ChebyWrk(psi0, 20.0, -10.0, 1.0))
    assert np.linalg.norm(outs[15] - ref) < TOL


def _with_diagonal(rp, col, vals, N):
    H = synth.to_scipy(rp, col, vals, N) + sp.diags(np.linspace(-1.0, 1.0, N)).astype(np.complex128)
    H = sp.csr_matrix(H)
    H.sort_indices()
    return H.indptr.astype(np.int64), H.indices.astype(np.int32), H.data.astype(np.complex128)


WALK_KNOBS = ("hrb_walk", "walk_waves", "walk_nt", "walk_dbg", "walk_min_blocks", "walk_pair")
WALK_DEFAULTS = {"hrb_walk": 1, "walk_waves": 0, "walk_nt": -1, "walk_dbg": 0, "walk_min_blocks": 3072, "walk_pair": -1}


@pytest.mark.parametrize("N,offsets,diag,real,shape", [
    ((1 << 15) + 192, synth.BANDED_OFFSETS, False, False, (4, 4, 0)),      # the headline lattice, a partly filled last block
    (1 << 16, (1, 2, 512, 1024), False, False, (2, 2, 0)),
    (1 << 15, (1, 3, 7, 256), False, False, (3, 1, 0)),
    (1 << 15, (2, 128, 256, 384), False, False, (1, 3, 0)),
    (1 << 16, synth.BANDED_OFFSETS, True, False, (4, 4, 1)),               # with a diagonal: 9 + 3 pad slots in the upper section
    (1 << 15, (1, 2, 3, 4, 192, 384, 576, 768), False, False, (4, 4, 0)),  # three row blocks per strip step
    (1 << 15, (1, 2, 512, 1024), True, True, (2, 2, 1)),                   # real couplings: the walk streams the fp64 copy
    (1 << 15, (1, 256), True, False, (1, 1, 1)),                           # the five-point lattice: hopping + on-site term
    (1 << 15, (1, 128), False, False, (1, 1, 0)),                          # (2 lower entries per row: padded lower sections)
    (1 << 15, (1, 2, 192), True, True, (2, 1, 1)),
    (1 << 15, (3, 128, 256), False, False, (1, 2, 0)),
    (1 << 15, (1, 2, 3, 4, 256, 512), True, False, (4, 2, 1)),
    (1 << 16, (2, 5, 9, 320, 640, 960), False, False, (3, 3, 0)),
    # strip steps that are no multiple of the 64-row block (a 100 x 327 lattice): the last column chunk is partly filled
    (32700, (1, 100), True, False, (1, 1, 1)),
    (1 << 15, (1, 2, 3, 4, 100, 200, 300, 400), False, False, (4, 4, 0)),
    (1 << 15, (1, 16, 65, 130), False, True, (2, 2, 0)),
    ((1 << 15) + 77, (2, 127, 254, 381), True, False, (1, 3, 1)),
    (1 << 16, (1, 5, 1000, 2000), False, False, (2, 2, 0)),
], ids=["16nnz", "8nnz", "near3far1", "near1far3", "16nnz+diag", "g192", "real+diag", "5point", "4nnz", "near2far1+diag",
        "near1far2", "near4far2+diag", "near3far3", "g100_5point", "g100_16nnz", "g65_real", "g127+diag_ragged", "g1000"])
def test_strip_walk_bit_identical_to_block_kernel(ctx, N, offsets, diag, real, shape):
    """The strip-walk kernel of a lattice operator (kernels_walk.hip: register ring of the gathered elements, FIFO of the
    far upper values and near windows in LDS, edge blocks on the per-block path) sums every row in the order of the
    per-block kernel: bit-identical results for every lattice shape that has a kernel instance, for every partition of
    the walk (wavefront count), edge-block placement and cache policy -- and within 1e-10 of the oracle."""
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=offsets)
    if real:
        vals = vals.real.astype(np.complex128)
    if diag:
        rp, col, vals = _with_diagonal(rp, col, vals, N)
    saved = {k: ctx.tuning_get(k) for k in WALK_KNOBS}
    try:
        ctx.tuning_set("walk_min_blocks", 16)
        Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)], 0, L.FMT_HRB)
        wi = Op.walk_info()
        assert wi["valid"] == 1 and (wi["near"], wi["far"], wi["diag"]) == shape
        assert wi["rows_per_step"] == [d for d in offsets if d >= 64][0]
        assert 0 < wi["edge_blocks"] < 0.6 * Op.layout_info()["blocks"]
        psi0 = synth.random_state(N)
        wrk = L.ChebyWrk(ctx, N, 24.0, -12.0, 1.0)

        def run(**knobs):
            for k, v in {**WALK_DEFAULTS, "walk_min_blocks": 16, **knobs}.items():
                ctx.tuning_set(k, v)
            psi = L.State(ctx, data=psi0)
            L.cheby(psi, Op, 1.0, wrk)
            L.cheby(psi, Op, -1.0, wrk)
            L.cheby(psi, Op, 1.0, wrk)
            return psi.numpy()

        base = run(hrb_walk=0)                                     # the per-block kernel
        for knobs in (dict(), dict(walk_waves=64), dict(walk_waves=2048), dict(walk_waves=4096),
                      dict(walk_dbg=4), dict(walk_dbg=5), dict(walk_dbg=4, walk_waves=256),
                      dict(walk_nt=1), dict(walk_nt=0, walk_waves=512), dict(walk_waves=96)):
            assert np.array_equal(base, run(**knobs)), knobs
        if shape == (4, 4, 0):                                     # the measurement variants of the headline shape
            for nt in (3, 5, 7):
                assert np.array_equal(base, run(walk_nt=nt)), nt
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    H = synth.to_scipy(rp, col, vals, N)
    ref = qo.cheby(psi0.copy(), H, 1.0, qo.ChebyWrk(psi0, 24.0, -12.0, 1.0))
    assert np.linalg.norm(base - ref) < TOL


def test_strip_walk_random_lattices_bit_identical(ctx):
    """Seeded sweep over lattice parameters at the edges of the walk plan: strip steps of one row block (g = 64) up to 40,
    near distances up to the LDS halo (16), sizes that are no multiple of g or of 64, few steps per wavefront, a diagonal
    or none, real or complex couplings -- whenever the operator gets a plan, the walk and the per-block kernel agree bit
    for bit (forward, backward, forward); shapes without a kernel instance must simply have no plan."""
    rng = np.random.default_rng(20261003)
    saved = {k: ctx.tuning_get(k) for k in WALK_KNOBS}
    n_walked = 0
    try:
        for trial in range(40):
            nn, K = int(rng.integers(1, 5)), int(rng.integers(1, 5))
            S = int(rng.choice([1, 2, 3, 5, 8, 16, 40]))
            g = 64 * S if trial % 2 == 0 else int(rng.integers(64, 64 * S + 64))     # every other trial: any stride
            near = sorted(rng.choice(np.arange(1, 17), nn, replace=False).tolist())
            nsteps = int(rng.integers(2 * K + 4, 2 * K + 40))
            N = g * nsteps + int(rng.choice([0, 0, 64, 17, 200]))
            offsets = tuple(near) + tuple(g * m for m in range(1, K + 1))
            if 2 * max(offsets) >= N:
                continue
            rp, col, vals = synth.hermitian_offsets_csr(N, offsets=offsets, seed=1000 + trial)
            diag = bool(rng.integers(0, 2))
            if bool(rng.integers(0, 4) == 0):
                vals = vals.real.astype(np.complex128)
            if diag:
                rp, col, vals = _with_diagonal(rp, col, vals, N)
            for k, v in {**WALK_DEFAULTS, "walk_min_blocks": 8}.items():
                ctx.tuning_set(k, v)
            Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)], 0, L.FMT_HRB)
            wi = Op.walk_info()
            if not wi["valid"]:
                Op.close()
                continue
            assert (wi["near"], wi["far"], wi["diag"], wi["rows_per_step"]) == (nn, K, int(diag), g)
            psi0 = synth.random_state(N, seed=trial)
            wrk = L.ChebyWrk(ctx, N, 26.0, -13.0, 0.9)
            outs = []
            for knobs in (dict(hrb_walk=0), dict(hrb_walk=1), dict(hrb_walk=1, walk_waves=int(rng.choice([16, 128, 1024, 4096])),
                                                                   walk_dbg=int(rng.choice([0, 1, 4, 5])), walk_nt=int(rng.integers(0, 2)),
                                                                   walk_pair=int(rng.choice([0, 1])))):
                for k, v in {**WALK_DEFAULTS, "walk_min_blocks": 8, **knobs}.items():
                    ctx.tuning_set(k, v)
                psi = L.State(ctx, data=psi0)
                L.cheby(psi, Op, 0.9, wrk)
                L.cheby(psi, Op, -0.9, wrk)
                L.cheby(psi, Op, 0.9, wrk)
                outs.append(psi.numpy())
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), (trial, offsets, N, diag)
            assert abs(np.linalg.norm(outs[1]) - 1.0) < 1e-11
            n_walked += 1
            Op.close()
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    assert n_walked >= 24


@pytest.mark.parametrize("nx,ny,flux,nnn,shape", [(100, 420, 0.2, False, (1, 1, 1)), (64, 700, 0.0, False, (1, 1, 1)),
                                                  (130, 330, 0.1, True, (2, 1, 1))], ids=["100x420", "64x700_real", "130x330_nnn"])
def test_lattice_fill_open_boundary_grid(ctx, nx, ny, flux, nnn, shape):
    """A finite-difference Hamiltonian on an nx x ny grid with open boundaries: the rows at the grid's x-edges lack a
    neighbour, so no run of row blocks has one distance list on every row.  Operator creation completes those rows with
    explicit zeros (knob lattice_fill, qp_operator_fill_info): the operator becomes the walk's lattice with strip step
    g = nx (no multiple of 64 here), the step agrees with the oracle, and with the unfilled operator to rounding."""
    H = synth.grid_hamiltonian_2d(nx, ny, flux=flux, next_nearest=nnn)
    N = nx * ny
    psi0 = synth.random_state(N)
    saved = {k: ctx.tuning_get(k) for k in ("walk_min_blocks", "lattice_fill")}
    outs = {}
    try:
        ctx.tuning_set("walk_min_blocks", 64)
        for fill in (1, 0):
            ctx.tuning_set("lattice_fill", fill)
            Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)])
            wi = Op.walk_info()
            if fill:
                # entries that the rows between the first and the last grid row lack: 2 per grid row (6 with second
                # neighbours along x), plus their transposes in the first and the last grid row
                per_row = 6 if nnn else 2
                assert Op.fill_info() == per_row * (ny - 2) + per_row
                assert wi["valid"] == 1 and (wi["near"], wi["far"], wi["diag"]) == shape and wi["rows_per_step"] == nx
                assert Op.format == L.FMT_HRB
                rp, col, val = Op.get_csr()
                assert rp[-1] == H.nnz + Op.fill_info()
                assert abs(synth.to_scipy(rp, col, val, N) - H).max() == 0.0
            else:
                assert Op.fill_info() == 0 and wi["valid"] == 0
            wrk = L.ChebyWrk(ctx, N, 12.0, -1.0, 0.7)
            psi = L.State(ctx, data=psi0)
            for dt in (0.7, 0.7, -0.7):
                L.cheby(psi, Op, dt, wrk)
            outs[fill] = psi.numpy()
            Op.close()
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    owrk = qo.ChebyWrk(psi0, 12.0, -1.0, 0.7)
    ref = psi0.copy()
    for dt in (0.7, 0.7, -0.7):
        qo.cheby(ref, H, dt, owrk)
    assert np.linalg.norm(outs[1] - ref) < TOL
    assert np.linalg.norm(outs[1] - outs[0]) < 1e-12
    # an operator that is a lattice except for a few foreign entries is left alone
    H2 = sp.lil_matrix(H)
    H2[N // 2 + 5, N // 2 + 37] = 0.5
    H2[N // 2 + 37, N // 2 + 5] = 0.5
    H2 = sp.csr_matrix(H2)
    H2.sort_indices()
    try:
        ctx.tuning_set("walk_min_blocks", 64)
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H2)])
        assert Op.fill_info() == 0
        Op.close()
    finally:
        ctx.tuning_set("walk_min_blocks", saved["walk_min_blocks"])


@pytest.mark.parametrize("dims,flux,uniform", [((64, 8, 40), 0.2, False), ((100, 6, 30), 0.0, False), ((70, 9, 24), 0.1, False),
                                               ((0, 0, 0), 0.0, True)], ids=["64x8x40", "100x6x30_real", "70x9x24", "uniform_offsets"])
def test_strip_walk_long_pair_three_dimensional_grids(ctx, dims, flux, uniform):
    """Distances +-1, +-nx, +-nx ny: the plane distance is not in the walk's ring of +-K strip steps (it is ny steps away);
    the kernel instances with a long pair (XL) load its operands directly.  A seven-point Hamiltonian on an open-boundary
    nx x ny x nz grid is completed at creation (the x-edge rows AND the y-edge lines of every plane) and then walks in steps
    of g = nx: bit-identical to the per-block kernel for several partitions of the walk, within 1e-10 of the oracle."""
    if uniform:          # translation-invariant lattice with the same distances (no completion needed)
        N = 1 << 15
        rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 128, 3000))
        H = synth.to_scipy(rp, col, vals, N)
        H = sp.csr_matrix(H + sp.diags(np.linspace(-1.0, 1.0, N)).astype(np.complex128))
        H.sort_indices()
        Delta, Emin = 24.0, -12.0
    else:
        H = synth.grid_hamiltonian_3d(*dims, flux=flux)
        N = H.shape[0]
        Delta, Emin = 14.0, -1.0
    psi0 = synth.random_state(N)
    saved = {k: ctx.tuning_get(k) for k in WALK_KNOBS}
    try:
        ctx.tuning_set("walk_min_blocks", 16)
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)])
        assert Op.format == L.FMT_HRB
        wi = Op.walk_info()
        assert wi["valid"] == 1 and wi["far"] == 1 and wi["diag"] == 1
        assert wi["long_distance"] == (3000 if uniform else dims[0] * dims[1])
        if not uniform:
            assert Op.fill_info() > 0 and wi["rows_per_step"] == dims[0]
            assert wi["first_block"] >= (dims[0] * dims[1]) // 64
        wrk = L.ChebyWrk(ctx, N, Delta, Emin, 0.6)

        def run(**knobs):
            for k, v in {**WALK_DEFAULTS, "walk_min_blocks": 16, **knobs}.items():
                ctx.tuning_set(k, v)
            psi = L.State(ctx, data=psi0)
            for dt in (0.6, -0.6, 0.6):
                L.cheby(psi, Op, dt, wrk)
            return psi.numpy()

        base = run(hrb_walk=0)
        for knobs in (dict(), dict(walk_waves=64), dict(walk_waves=1024), dict(walk_dbg=4), dict(walk_dbg=5, walk_waves=256),
                      dict(walk_nt=1), dict(walk_waves=96)):
            assert np.array_equal(base, run(**knobs)), knobs
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    owrk = qo.ChebyWrk(psi0, Delta, Emin, 0.6)
    ref = psi0.copy()
    for dt in (0.6, -0.6, 0.6):
        qo.cheby(ref, H, dt, owrk)
    assert np.linalg.norm(base - ref) < TOL


def _uniform_shape(case):
    """`uniform_n<near>k<far>z<diag>x<long pairs>[_fd][_real]`: the offsets of a translation-invariant lattice of that walk shape
    (strip step 128 rows, N = 2^15) and what walk_info() must say.  With these every kernel instance of the long-pair and
    diagonal-neighbour families is run, complex values and real copy (profiles/walk_step_core.txt lists which case reaches which)."""
    nn, K, z0, xl = (int(t) for t in re.fullmatch(r"uniform_n(\d+)k(\d+)z(\d+)x(\d+)(_fd)?(_real)?", case).groups()[:4])
    fd = "_fd" in case
    near = {1: (2,), 2: (1, 2)}[nn] if fd else {1: (1,), 2: (1, 3)}[nn]
    far = (127, 128, 129) if fd else tuple(128 * m for m in range(1, K + 1))
    longs = {0: (), 1: (2500,), 2: (1111, 2222)}[xl]
    return near + far + longs, dict(near=nn, far=K, diag=z0, longs=list(longs), step=128, fd=int(fd))


# (near, far, diag, long pairs) of the sixteen long-pair kernel shapes that the named cases leave out, complex values and real copy
XL_SHAPE_CASES = (["uniform_n%dk%dz%dx%d" % s for s in ((1, 1, 0, 1), (2, 1, 0, 1), (1, 2, 0, 1), (1, 2, 1, 1), (2, 2, 0, 1), (1, 1, 0, 2),
                                                        (2, 1, 0, 2), (2, 1, 1, 2), (1, 2, 0, 2), (1, 2, 1, 2))] +
                  ["uniform_n%dk%dz%dx%d_real" % s for s in ((1, 1, 0, 1), (2, 1, 0, 1), (2, 1, 1, 1), (1, 2, 0, 1), (1, 2, 1, 1), (2, 2, 0, 1),
                                                             (2, 2, 1, 1), (1, 1, 0, 2), (1, 1, 1, 2), (2, 1, 0, 2), (2, 1, 1, 2), (1, 2, 0, 2),
                                                             (1, 2, 1, 2), (2, 2, 0, 2))])


@pytest.mark.parametrize("case", ["grid_4th_order_72x10x20", "grid_4th_order_real_64x8x24", "uniform_k1_two_pairs", "uniform_k2_one_pair",
                                  "uniform_k2_two_pairs_no_diag"] + XL_SHAPE_CASES)
def test_strip_walk_two_long_pairs_and_two_far_distances(ctx, case):
    """The long-pair shapes beyond (one pair, one far distance): the fourth-order Laplacian of an open-boundary nx x ny x nz grid
    -- distances +-1, +-2, +-nx, +-2 nx, +-nx ny, +-2 nx ny: near 2, far 2, TWO long pairs, completed at creation like the
    seven-point one -- and translation-invariant lattices with one / two far distances and one / two pairs.  Bit-identical to
    the per-block kernel for several partitions of the walk, within 1e-10 of the oracle.  The uniform_n.k.z.x. cases (_uniform_shape)
    are the remaining long-pair shapes, one pair and one far distance included."""
    if case.startswith("grid"):
        dims = (72, 10, 20) if "72x10x20" in case else (64, 8, 24)     # (nx >= 64: the strip step)
        H = synth.grid_hamiltonian_3d(*dims, flux=0.0 if "real" in case else 0.15, order=4)
        N = H.shape[0]
        Delta, Emin = 16.0, -1.0
        want = dict(near=2, far=2, diag=1, longs=[dims[0] * dims[1], 2 * dims[0] * dims[1]], step=dims[0])
    else:
        N = 1 << 15
        offs, want = _uniform_shape(case) if case.startswith("uniform_n") else {
            "uniform_k1_two_pairs": ((1, 128, 1000, 3001), dict(near=1, far=1, diag=1, longs=[1000, 3001], step=128)),
            "uniform_k2_one_pair": ((1, 3, 100, 200, 2500), dict(near=2, far=2, diag=1, longs=[2500], step=100)),
            "uniform_k2_two_pairs_no_diag": ((2, 5, 192, 384, 1111, 2222), dict(near=2, far=2, diag=0, longs=[1111, 2222], step=192))}[case]
        rp, col, vals = synth.hermitian_offsets_csr(N, offsets=offs)
        if "real" in case:
            vals = vals.real.astype(np.complex128)
        H = synth.to_scipy(rp, col, vals, N)
        if want["diag"]:
            H = sp.csr_matrix(H + sp.diags(np.linspace(-1.0, 1.0, N)).astype(np.complex128))
        H.sort_indices()
        Delta, Emin = 24.0, -12.0
    psi0 = synth.random_state(N)
    saved = {k: ctx.tuning_get(k) for k in WALK_KNOBS}
    try:
        ctx.tuning_set("walk_min_blocks", 16)
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)])
        assert Op.format == L.FMT_HRB and Op.walk_reason()[1] == "ok"
        wi = Op.walk_info()
        assert wi["valid"] == 1 and (wi["near"], wi["far"], wi["diag"]) == (want["near"], want["far"], want["diag"])
        assert wi["long_distances"] == want["longs"] and wi["long_distance"] == want["longs"][-1] and wi["rows_per_step"] == want["step"]
        assert wi["far_diagonals"] == 0
        if case.startswith("grid"):
            assert Op.fill_info() > 0 and wi["first_block"] >= want["longs"][-1] // 64
        wrk = L.ChebyWrk(ctx, N, Delta, Emin, 0.6)

        def run(**knobs):
            for k, v in {**WALK_DEFAULTS, "walk_min_blocks": 16, **knobs}.items():
                ctx.tuning_set(k, v)
            psi = L.State(ctx, data=psi0)
            for dt in (0.6, -0.6, 0.6):
                L.cheby(psi, Op, dt, wrk)
            return psi.numpy()

        base = run(hrb_walk=0)
        for knobs in (dict(), dict(walk_waves=64), dict(walk_waves=1024), dict(walk_dbg=4), dict(walk_dbg=5, walk_waves=256),
                      dict(walk_nt=1), dict(walk_waves=96)):
            assert np.array_equal(base, run(**knobs)), knobs
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    owrk = qo.ChebyWrk(psi0, Delta, Emin, 0.6)
    ref = psi0.copy()
    for dt in (0.6, -0.6, 0.6):
        qo.cheby(ref, H, dt, owrk)
    assert np.linalg.norm(base - ref) < TOL


# (near, diag, long pairs) of the eight diagonal-neighbour kernel shapes that the named cases leave out (far = 1 always)
FD_SHAPE_CASES = (["uniform_n%dk1z%dx%d_fd" % s for s in ((2, 0, 0), (2, 1, 0), (1, 0, 1), (2, 0, 1), (2, 1, 1))] +
                  ["uniform_n%dk1z%dx%d_fd_real" % s for s in ((1, 0, 0), (2, 0, 0), (1, 0, 1), (1, 1, 1), (2, 0, 1), (2, 1, 1))])


@pytest.mark.parametrize("case", ["uniform_256", "uniform_100_no_diag", "uniform_real_two_near", "grid_96x50_tprime", "grid_128x40_tprime_real",
                                  "uniform_128_long_pair", "layers_72x10x20_tprime"] + FD_SHAPE_CASES)
def test_strip_walk_diagonal_far_neighbours(ctx, case):
    """Far distances with their diagonal neighbours, g - 1, g, g + 1 (nine-point stencil: next-nearest hopping on a two-dimensional
    grid): the gathered elements are the ring's elements one lane over (a DPP wavefront shift, the edge lane from a packed halo
    load), the conj-transposed values come out of the FIFO one lane over.  Bit-identical to the per-block kernel for several
    partitions of the walk (strip steps that are no multiple of 64 rows included), within 1e-10 of the oracle."""
    if case.startswith("layers"):      # planes with next-nearest hopping, coupled along z: one long pair beside the diagonals
        H = synth.grid_hamiltonian_3d(72, 10, 20, flux=0.2, diagonal=0.3)
        N = H.shape[0]
        Delta, Emin = 16.0, -1.0
        want = dict(near=1, diag=1, step=72, long=720)
    elif case.startswith("grid"):
        nx, ny = (96, 50) if "96x50" in case else (128, 40)
        H = synth.grid_hamiltonian_2d(nx, ny, flux=0.0 if "real" in case else 0.2, diagonal=0.3)
        N = H.shape[0]
        Delta, Emin = 12.0, -1.0
        want = dict(near=1, diag=1, step=nx)
    else:
        N = 1 << 15
        offs, want = _uniform_shape(case) if case.startswith("uniform_n") else {
                      "uniform_256": ((1, 255, 256, 257), dict(near=1, diag=1, step=256)),
                      "uniform_128_long_pair": ((2, 127, 128, 129, 3001), dict(near=1, diag=1, step=128, long=3001)),
                      "uniform_100_no_diag": ((3, 99, 100, 101), dict(near=1, diag=0, step=100)),
                      "uniform_real_two_near": ((1, 2, 511, 512, 513), dict(near=2, diag=1, step=512))}[case]
        rp, col, vals = synth.hermitian_offsets_csr(N, offsets=offs)
        if "real" in case:
            vals = vals.real.astype(np.complex128)
        H = synth.to_scipy(rp, col, vals, N)
        if want["diag"]:
            H = sp.csr_matrix(H + sp.diags(np.linspace(-1.0, 1.0, N)).astype(np.complex128))
        H.sort_indices()
        Delta, Emin = 24.0, -12.0
    psi0 = synth.random_state(N)
    saved = {k: ctx.tuning_get(k) for k in WALK_KNOBS}
    try:
        ctx.tuning_set("walk_min_blocks", 16)
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)])
        assert Op.format == L.FMT_HRB and Op.walk_reason()[1] == "ok"
        wi = Op.walk_info()
        assert wi["valid"] == 1 and wi["far_diagonals"] == 1 and wi["far"] == 1
        assert (wi["near"], wi["diag"], wi["rows_per_step"]) == (want["near"], want["diag"], want["step"])
        assert wi["long_distances"] == want.get("longs", [want["long"]] if "long" in want else [])
        if case.startswith("grid") or case.startswith("layers"):
            assert Op.fill_info() > 0
        wrk = L.ChebyWrk(ctx, N, Delta, Emin, 0.6)

        def run(**knobs):
            for k, v in {**WALK_DEFAULTS, "walk_min_blocks": 16, **knobs}.items():
                ctx.tuning_set(k, v)
            psi = L.State(ctx, data=psi0)
            for dt in (0.6, -0.6, 0.6):
                L.cheby(psi, Op, dt, wrk)
            return psi.numpy()

        base = run(hrb_walk=0)
        for knobs in (dict(), dict(walk_waves=64), dict(walk_waves=1024), dict(walk_dbg=4), dict(walk_dbg=5, walk_waves=256),
                      dict(walk_nt=1), dict(walk_waves=96)):
            assert np.array_equal(base, run(**knobs)), knobs
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    owrk = qo.ChebyWrk(psi0, Delta, Emin, 0.6)
    ref = psi0.copy()
    for dt in (0.6, -0.6, 0.6):
        qo.cheby(ref, H, dt, owrk)
    assert np.linalg.norm(base - ref) < TOL


def test_strip_walk_inside_a_replayed_graph(ctx):
    """Knob `cheby_graph` with an operator that takes the strip walk: the walk's launch (dynamic LDS above 64 KB, opted in
    per kernel instance and device) is captured and replayed like any other; same bits as the eager step, and the graph is
    re-recorded when a walk knob changes the launch shape."""
    N = 1 << 15
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4, 128, 256, 384, 512))
    saved = {k: ctx.tuning_get(k) for k in WALK_KNOBS + ("cheby_graph",)}
    try:
        for k, v in {**WALK_DEFAULTS, "walk_min_blocks": 16}.items():
            ctx.tuning_set(k, v)
        Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)], 0, L.FMT_HRB)
        assert Op.walk_info()["valid"] == 1
        psi0 = synth.random_state(N)
        wrk = L.ChebyWrk(ctx, N, 20.0, -10.0, 1.0)

        def run(graph, **knobs):
            for k, v in knobs.items():
                ctx.tuning_set(k, v)
            ctx.tuning_set("cheby_graph", 1 << 20 if graph else 0)
            psi = L.State(ctx, data=psi0)
            ctx.reset_stats()
            for _ in range(5):
                L.cheby(psi, Op, 1.0, wrk)
            return psi.numpy(), ctx.stats()["n_graph_launches"]

        eager, g0 = run(False)
        replay, g1 = run(True)
        assert g0 == 0 and g1 == 4 and np.array_equal(eager, replay)       # the first call arms the key, the second records
        other, g2 = run(True, walk_waves=96)                    # a different launch shape: new key, new graph
        assert g2 == 4 and np.array_equal(eager, other)
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)


def test_strip_walk_plan_only_for_lattices(ctx):
    """The walk plan is index work on the host: it exists only where one list of column distances repeats down a run of row
    blocks and has the walk's shape -- not for scattered or per-row random columns, not for near distances beyond the LDS
    halo, far distances that are not the multiples g, 2 g, .. of one stride g >= 64 (any such g will do; ONE or TWO further distances
    beyond them are the long pairs of a three-dimensional grid, with at most two near and two far distances), more than four near or far distances -- and it
    goes away when a complex coefficient forces the operator out of the Hermitian-packed format."""
    N = 1 << 15
    saved = ctx.tuning_get("walk_min_blocks")
    ctx.tuning_set("walk_min_blocks", 16)
    try:
        for offsets, want in (((1, 2, 512, 1024), 1), ((1, 2, 500, 1000), 1), ((1, 2, 500, 1100), 1), ((1, 2, 500, 1100, 1700), 1), ((1, 2, 500, 1100, 1700, 2300), 0), ((1, 2, 3, 500, 1100), 0), ((1, 2, 40, 80), 0), ((1, 17, 512, 1024), 0), ((1, 2, 512, 1536), 1), ((1, 2, 512, 1536, 2048), 1),
                              ((1, 2, 3, 512), 1), ((1, 512, 1024, 1536), 1), ((3, 5, 320, 640), 1), ((1, 2, 3, 4, 5, 6, 512, 1024), 0)):
            rp, col, vals = synth.hermitian_offsets_csr(N, offsets=offsets)
            Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)], 0, L.FMT_HRB)
            assert Op.walk_info()["valid"] == want, offsets
            Op.close()
        rp, col, vals = synth.hermitian_offsets_csr(N, offsets=synth.scattered_offsets(N, 4))
        assert L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)], 0, L.FMT_HRB).walk_info()["valid"] == 0
        rp, col, vals = synth.random_columns_csr(4096, n_pairs=4)
        assert L.Operator(ctx, [L.Matrix(ctx, 4096, 4096, rp, col, vals)], 0, L.FMT_HRB).walk_info()["valid"] == 0
        # two Hermitian terms, one coefficient: real -> packed + walk; complex -> plain row blocks, no walk, one re-layout
        rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 512, 1024))
        M = L.Matrix(ctx, N, N, rp, col, vals)
        Op = L.Operator(ctx, [M, M], 1)
        Op.set_coeffs([0.5])
        assert Op.format == L.FMT_HRB and Op.walk_info()["valid"] == 1
        b0 = Op.build_info()
        assert b0["relayouts"] == 0 and b0["build_ms"] > 0 and b0["format"] == L.FMT_HRB
        Op.set_coeffs([0.5 + 0.25j])
        b1 = Op.build_info()
        assert Op.format == L.FMT_RBCSR and Op.walk_info()["valid"] == 0
        assert b1["relayouts"] == 1 and b1["build_ms_total"] > b0["build_ms_total"] and b1["format"] == L.FMT_RBCSR
        psi0 = synth.random_state(N)
        psi = L.State(ctx, data=psi0)
        y = L.State(ctx, n=N)
        Op.mul(psi, y)
        H = synth.to_scipy(rp, col, vals, N)
        assert np.linalg.norm(y.numpy() - (1.5 + 0.25j) * (H @ psi0)) < TOL
    finally:
        ctx.tuning_set("walk_min_blocks", saved)


@pytest.mark.parametrize("window", [None, 1024])
@pytest.mark.parametrize("fmt", [L.FMT_AUTO, L.FMT_HRB, L.FMT_RBCSR, L.FMT_CSR])
def test_random_columns_matches_oracle(ctx, window, fmt):
    """An irregular H -- columns drawn per row, globally or inside 1024-row windows, 12-16 entries per
    row (no translation invariance: no stencil blocks, per-entry indices) -- through every device
    format against the oracle, forward and backward, plus the bit-exact device round trip."""
    N = 1 << 14
    rp, col, vals = synth.random_columns_csr(N, window=window, seed=4242)
    H = synth.to_scipy(rp, col, vals, N)
    assert abs(H - H.conj().T).max() == 0 and np.diff(rp).max() == 16 and np.diff(rp).min() >= 12
    Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)], 0, fmt)
    lay = Op.layout_info()
    if fmt == L.FMT_AUTO:
        # irregular blocks: the conj-transposed reads of the Hermitian packing would not coalesce, AUTO keeps
        # plain row blocks even where the window would fit L2 (profiles/r02/kbench_random_window.txt)
        assert Op.format == L.FMT_RBCSR
    if Op.format != L.FMT_CSR:
        assert lay["stencil_upper_blocks"] == 0 and lay["stencil_lower_blocks"] == 0   # nothing translation invariant to encode
    r2, c2, v2 = Op.get_csr()
    assert np.array_equal(r2, rp) and np.array_equal(c2, col) and np.array_equal(v2, vals)
    psi0 = synth.random_state(N, seed=99)
    wrk = L.ChebyWrk(ctx, N, 20.0, -10.0, 0.8)
    owrk = qo.ChebyWrk(psi0, 20.0, -10.0, 0.8)
    psi = L.State(ctx, data=psi0)
    ref = psi0.copy()
    for dt in (0.8, 0.8, -0.8):
        L.cheby(psi, Op, dt, wrk)
        ref = qo.cheby(ref, H, dt, owrk)
        assert np.linalg.norm(psi.numpy() - ref) < TOL


def test_random_columns_full_size_properties(ctx):
    """The irregular pattern at the BASELINE size (N = 2^20, columns anywhere): which encodings fire
    (none of the stencil ones; AUTO leaves the Hermitian packing, whose transposed values would not
    be in L2), unitarity, forward / backward round trip, and all device formats agree."""
    N = 1 << 20
    rp, col, vals = synth.random_columns_csr(N)
    M = L.Matrix(ctx, N, N, rp, col, vals)
    del rp, col, vals
    psi0 = synth.random_state(N)
    wrk = L.ChebyWrk(ctx, N, 20.0, -10.0, 1.0)
    res = {}
    for fmt in (L.FMT_AUTO, L.FMT_HRB, L.FMT_CSR):
        Op = L.Operator(ctx, [M], 0, fmt)
        if fmt == L.FMT_AUTO:
            assert Op.format == L.FMT_RBCSR
            lay = Op.layout_info()
            assert lay["stencil_upper_blocks"] == 0 and lay["index_bytes"] >= 4 * 15 * N
        psi = L.State(ctx, data=psi0)
        L.cheby(psi, Op, 1.0, wrk)
        res[fmt] = psi.numpy()
        assert abs(np.linalg.norm(res[fmt]) - 1) < 1e-11
        L.cheby(psi, Op, -1.0, wrk)
        assert np.linalg.norm(psi.numpy() - psi0) < TOL
        Op.close()
    assert np.linalg.norm(res[L.FMT_AUTO] - res[L.FMT_CSR]) < TOL and np.linalg.norm(res[L.FMT_HRB] - res[L.FMT_CSR]) < TOL


def test_newton_c3_full_size(ctx):
    """BASELINE configs[2] at full size: N = 2^18 non-Hermitian Liouvillian (n = 512), Newton
    with m_max = 20, one step against the NumPy oracle (a few seconds of CPU)."""
    Lm = synth.liouvillian_tridiag(512)
    N = Lm.shape[0]
    assert N == 1 << 18
    rho0 = synth.random_state(N)
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, Lm)])
    wrk = L.NewtonWrk(ctx, N, m_max=20)
    rho = L.State(ctx, data=rho0)
    L.newton(rho, Op, 0.5, wrk)
    owrk = qo.NewtonWrk(rho0, m_max=20)
    ref = qo.newton(rho0.copy(), Lm, 0.5, owrk)
    assert np.linalg.norm(rho.numpy() - ref) < TOL
    # SURVEY 7 allows the convergence test to fire one restart apart; on this fixed input it does not, and a systematic
    # extra restart (50 % more sweeps) must not pass unnoticed
    assert wrk.restarts == owrk.restarts, (wrk.restarts, owrk.restarts)


@pytest.mark.parametrize("n", [96, 200])
def test_newton_sweep_knobs_match_oracle(ctx, n):
    """The Arnoldi sweep as shipped since round 4 -- the projection kernel on the mat-vec's rows per XCD, reading rounds and
    basis vectors back to front, the matrix streamed nontemporal in the fused mat-vec (both were knobs until round 6: settled) --
    against the oracle: |delta psi| < 1e-10 after every step, the restart counts equal; n = 200 (N = 40000) has
    two rounds of row blocks per workgroup with a partly filled last one."""
    Lm = synth.liouvillian_tridiag(n)
    N = Lm.shape[0]
    rho0 = synth.random_state(N)
    saved = {}
    try:
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, Lm)])
        wrk = L.NewtonWrk(ctx, N, m_max=12)
        rho = L.State(ctx, data=rho0)
        owrk = qo.NewtonWrk(rho0, m_max=12)
        ref = rho0.copy()
        ctx.reset_stats()
        for step, dt in enumerate((0.5, 0.5, 0.5, -0.5, 0.3)):
            L.newton(rho, Op, dt, wrk)
            qo.newton(ref, Lm, dt, owrk)
            assert np.linalg.norm(rho.numpy() - ref) < TOL, step
            assert wrk.restarts == owrk.restarts, (step, wrk.restarts, owrk.restarts)
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)


def test_batched_c5_full_size_properties(ctx):
    """BASELINE configs[4] at full size: 64 states x N = 2^18.  Three columns of the panel against the C restatement of
    the reference's serial CSC path (oracle/cheby_ref.c, ~0.15 s of one core each) -- the oracle DIRECTLY at the full
    size, for the wave-per-row kernel and, with 8 states (one GPU's share of the panel split over 8), for the
    state-tiled kernel; every state must also equal the single-state kernel's result for that state (different
    kernel, same operator), norms are conserved and a backward step undoes a forward one."""
    from oracle import ref_c
    N, b = 1 << 18, 64
    rp, col, vals = synth.hermitian_offsets_csr(N)
    Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)])
    states = np.stack([synth.random_state(N, seed=500 + s) for s in range(b)], axis=1)
    coeffs = L.ChebyWrk(ctx, N, 20.0, -10.0, 1.0).coeffs
    cref = {}
    for s in (0, 5, 17, 63):                 # Hermitian H: CSC(H) = conj CSR(H)
        c = states[:, s].copy()
        ref_c.cheby_csc(rp, col.astype(np.int64), np.conj(vals), c, coeffs, 20.0, -10.0, 1.0)
        cref[s] = c
    del rp, col, vals
    p8 = L.State(ctx, data=np.ascontiguousarray(states[:, :8]).reshape(-1))       # 8 states: csr_spmm_kernel
    w8 = L.ChebyWrk(ctx, N * 8, 20.0, -10.0, 1.0)
    L.cheby_batched(p8, Op, 1.0, w8, 8)
    out8 = p8.numpy().reshape(N, 8)
    for s in (0, 5):
        assert np.linalg.norm(out8[:, s] - cref[s]) < TOL, s
    p8.close()
    w8.close()
    panel = L.State(ctx, data=states.reshape(-1))
    wrk = L.ChebyWrk(ctx, N * b, 20.0, -10.0, 1.0)
    L.cheby_batched(panel, Op, 1.0, wrk, b)
    out = panel.numpy().reshape(N, b)
    assert np.max(np.abs(np.linalg.norm(out, axis=0) - 1.0)) < 1e-11
    for s in (0, 17, 63):                    # the oracle at the full size, panel kernel (more than 32 states)
        assert np.linalg.norm(out[:, s] - cref[s]) < TOL, s
    w1 = L.ChebyWrk(ctx, N, 20.0, -10.0, 1.0)
    for s in (0, 17, 63):
        single = L.State(ctx, data=states[:, s].copy())
        L.cheby(single, Op, 1.0, w1)
        assert np.linalg.norm(single.numpy() - out[:, s]) < TOL
    L.cheby_batched(panel, Op, -1.0, wrk, b)
    assert np.linalg.norm(panel.numpy().reshape(N, b) - states) < 1e-9


# ---------------------------------------------------------------- persistent single-launch Arnoldi

@pytest.mark.parametrize("N,dense,m,per_row", [(3, True, 2, 0), (64, True, 10, 0), (55, False, 10, 5.0),
                                               (300, False, 12, 5.0), (500, False, 10, 4.0), (1000, False, 4, 1.5)])
def test_arnoldi_persistent_small(ctx, N, dense, m, per_row):
    """Register-resident operators run arnoldi! (src/arnoldi.jl:74-100) as one persistent
    launch: same Hessenberg matrix and Krylov vectors as the oracle and as the general
    (launch per kernel) path, extended or not, dt of either sign."""
    rng = np.random.default_rng(100 + N)
    A = synth.dense_nonhermitian(N, rho=3.0, rng=rng) if dense else synth.sparse_random(N, min(1.0, per_row / N), rho=3.0, rng=rng)
    A = sp.csr_matrix(A)
    psi = _rand_state(N, rng)
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)])
    for extended, dt in ((True, 0.4), (False, -0.7)):
        res = {}
        for small in (1, 0):
            L.tuning_set("small_nnz", 8192 if small else 0)
            try:
                ctx.reset_stats()
                q = L.Krylov(ctx, N, m + 1)
                Hess = np.zeros((m + 1, m + 1), dtype=complex, order="F")
                m_out = L.arnoldi(Hess, q, m, L.State(ctx, data=psi), Op, dt, extended=extended)
                res[small] = (m_out, Hess, [q.vec(i) for i in range(m + 1)], ctx.stats()["n_kernel_launches"])
            finally:
                L.tuning_set("small_nnz", 8192)
        assert res[1][3] == 1 and res[0][3] > m       # one launch vs several per column
        Href = np.zeros((m + 1, m + 1), dtype=complex)
        qref = [np.empty(N, dtype=complex) for _ in range(m + 1)]
        m_ref = qo.arnoldi(Href, qref, m, psi, A, dt, extended=extended)
        for m_out, Hess, qs, _ in res.values():
            assert m_out == m_ref
            assert np.max(np.abs(Hess - Href)) < 1e-12
            for i in range(m_ref + (1 if extended else 0)):
                assert np.linalg.norm(qs[i] - qref[i]) < 1e-11


def test_newton_persistent_small_liouvillian(ctx):
    """Newton on a small open-system Liouvillian (N = n^2 = 256): every Arnoldi sweep is one
    launch; result equals the general path and the oracle."""
    n = 16
    Lv = synth.liouvillian_tridiag(n)
    N = n * n
    rng = np.random.default_rng(9)
    rho0 = _rand_state(N, rng)
    outs = {}
    for small in (1, 0):
        L.tuning_set("small_nnz", 8192 if small else 0)
        try:
            out, ref, wrk, owrk = _newton_case(ctx, Lv, rho0, 0.5, 10)
        finally:
            L.tuning_set("small_nnz", 8192)
        assert np.linalg.norm(out - ref) < TOL
        outs[small] = out
    assert np.linalg.norm(outs[0] - outs[1]) < 1e-12


@pytest.mark.parametrize("fmt", [L.FMT_CSR, L.FMT_RBCSR, L.FMT_HRB])
@pytest.mark.parametrize("dt", [0.05, 0.3, 0.9, 2.0])
def test_cheby_deferred_accumulation_bit_identical(ctx, fmt, dt):
    """Psi += a_i v_i folded into every third term's epilogue (knob acc_defer, default on) runs
    the same FMA sequence as the term-by-term update of src/cheby.jl:182/:205: results are
    bit-identical for every residue of the number of terms mod 3."""
    N = 3000
    rp, col, val = synth.hermitian_offsets_csr(N, (1, 2, 7, 64), rho=6.0)
    H = synth.to_scipy(rp, col, val, N)
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)], fmt=fmt)
    psi0 = synth.random_state(N)
    seen = set()
    for shrink in (1.0, 0.8, 0.6):
        wrk = L.ChebyWrk(ctx, N, 14.0 * shrink, -7.0 * shrink, dt)
        seen.add((wrk.n_coeffs - 1) % 3)
        outs = []
        for knob in (1, 0):
            L.tuning_set("acc_defer", knob)
            try:
                psi = L.State(ctx, data=psi0)
                for _ in range(3):
                    L.cheby(psi, Op, dt, wrk)
                outs.append(psi.numpy())
            finally:
                L.tuning_set("acc_defer", 1)
        assert np.array_equal(outs[0], outs[1])
    assert len(seen) >= 2


@pytest.mark.parametrize("fmt", [L.FMT_RBCSR, L.FMT_HRB])
@pytest.mark.parametrize("N", [64 * 40, 64 * 40 + 17, 200])
def test_stencil_blocks_bit_identical(ctx, fmt, N):
    """Blocks whose rows all sit at the same distances from the diagonal are stored as stencil
    sections (one delta per slot per block instead of per-lane indices; for the Hermitian
    lower section also no transpose positions).  The decode is exact: device round trip and
    Cheby steps are bit-identical to the per-lane encodings (knob `stencil` = 0), with
    wrap-around rows, a partial last block and irregular rows mixed in."""
    offs = (1, 2, 7, 64, 130) if N > 300 else (1, 3)
    rp, col, val = synth.hermitian_offsets_csr(N, offs, rho=6.0)
    H = synth.to_scipy(rp, col, val, N).tolil()
    if N > 300:                               # irregular rows inside otherwise regular blocks
        H[700, 900] = 0.3 + 0.1j
        H[900, 700] = 0.3 - 0.1j
    H = sp.csr_matrix(H)
    H.sort_indices()
    psi0 = synth.random_state(N)
    outs, infos = [], []
    for knob in (1, 0):
        L.tuning_set("stencil", knob)
        try:
            Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)], fmt=fmt)
        finally:
            L.tuning_set("stencil", 1)
        infos.append(Op.layout_info())
        rp2, col2, val2 = Op.get_csr()
        assert np.array_equal(rp2, H.indptr) and np.array_equal(col2, H.indices) and np.array_equal(val2, H.data)
        wrk = L.ChebyWrk(ctx, N, 16.0, -8.0, 0.4)
        psi = L.State(ctx, data=psi0)
        for _ in range(3):
            L.cheby(psi, Op, 0.4, wrk)
        outs.append(psi.numpy())
    assert np.array_equal(outs[0], outs[1])
    on, off = infos
    assert off["stencil_upper_blocks"] == 0 and off["stencil_lower_blocks"] == 0
    if N > 300:
        assert 0 < on["stencil_upper_blocks"] < on["blocks"]          # interior blocks only
        assert on["index_bytes"] < 0.9 * off["index_bytes"]
        if fmt == L.FMT_HRB:
            assert 0 < on["stencil_lower_blocks"] < on["blocks"]
    ref = psi0.copy()
    owrk = qo.ChebyWrk(ref, 16.0, -8.0, 0.4)
    for _ in range(3):
        qo.cheby(ref, H, 0.4, owrk)
    assert np.linalg.norm(outs[0] - ref) < TOL


@pytest.mark.parametrize("fmt", [L.FMT_CSR, L.FMT_RBCSR, L.FMT_HRB])
@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_sparse_control_terms_update_only_their_positions(ctx, fmt, real):
    """evaluate! (src/generators.jl:757-766) with sparse trailing control terms -- a diagonal dipole operator next to a
    banded drift -- rewrites only the positions those terms touch (knob sparse_controls): the stored values after any
    sequence of coefficient / scale changes are those of the full combination, bit for bit (the real copy included: same
    cheby! results), for the sparse term last, two sparse terms, a dense control term before them; a dense term AFTER a
    sparse one switches the path off.  A complex coefficient on the packed format still re-lays the operator out."""
    N = 6000
    rng = np.random.default_rng(5)
    rp, col, val = synth.hermitian_offsets_csr(N, (1, 2, 7, 64), rho=6.0)
    H0 = synth.to_scipy(rp, col, val, N)
    rp, col, val = synth.hermitian_offsets_csr(N, (1, 2, 7, 64), rho=6.0, seed=77)
    Hd = 0.3 * synth.to_scipy(rp, col, val, N)                                   # a dense control term
    D1 = sp.diags([np.linspace(-1, 1, N)], [0], format="csr", dtype=complex)    # sparse: the diagonal
    D2 = sp.diags([rng.uniform(-1, 1, N - 2)], [2], format="csr", dtype=complex)
    D2 = (D2 + D2.getH()).tocsr()                                                # sparse: one off-diagonal pair
    if real:
        H0, Hd, D2 = (sp.csr_matrix(M.real.astype(complex)) for M in (H0, Hd, D2))
    psi0 = synth.random_state(N)
    moves = [("c", [0.5, -0.25, 0.1]), ("c", [0.5, -0.25, 0.7]), ("c", [0.5, 0.4, 0.7]), ("s", 0.5), ("c", [0.9, 0.4, -0.2]),
             ("c", [0.9, 0.4, -0.3]), ("s", 1.0)]
    if fmt != L.FMT_HRB and not real:
        moves.append(("c", [0.9, 0.4 + 0.1j, -0.3 + 0.2j]))
    for terms, expect_sparse in (([H0, Hd, D1, D2], True), ([H0, D1, Hd, D2], True), ([H0, D1, D2, Hd], False)):
        outs = []
        for knob in (1, 0):
            ctx.tuning_set("sparse_controls", knob)
            try:
                Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M) for M in terms], ncoeffs=3, fmt=fmt)
                res = []
                wrk = L.ChebyWrk(ctx, N, 30.0, -15.0, 0.3)
                for kind, arg in moves:
                    n0 = ctx.stats()["n_kernel_launches"]
                    Op.set_coeffs(arg) if kind == "c" else Op.set_scale(arg)
                    ev = Op.evaluate_info()
                    relaid = Op.format != fmt            # (a complex coefficient un-packed the operator: full combination from then on)
                    # the sparse path exists when the trailing control terms touch at most a quarter of the STORED values: 3 of the
                    # 12 padded slots per row in the row-block formats, but 3 of 11 entries as plain CSR (no padding) -- not there
                    # (as plain CSR the stored count differs and a shorter suffix of the control terms may still qualify: the
                    # library's own answer is taken there, and checked for consistency)
                    has_sparse = ev["first_sparse_term"] > 0
                    if fmt != L.FMT_CSR and not relaid:
                        assert has_sparse == expect_sparse, (kind, arg, ev)
                    if not expect_sparse or relaid:
                        assert not has_sparse, (kind, arg, ev)
                    assert ev["latest_update_sparse"] == (1 if (knob and has_sparse) else 0), (kind, arg, ev)
                    if has_sparse:
                        assert 0 < ev["positions"] <= 3 * N
                    res.append(Op.get_csr()[2])
                    x = L.State(ctx, data=psi0)
                    L.cheby(x, Op, 0.3, wrk)
                    res.append(x.numpy())
                outs.append(res)
                Op.close()
            finally:
                ctx.tuning_set("sparse_controls", 1)
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
        # the last state against the oracle
        kind_c = [m for m in moves if m[0] == "c"][-1][1]
        scale = [m for m in moves if m[0] == "s"][-1][1]
        Heff = scale * (terms[0] + sum(c * M for c, M in zip(kind_c, terms[1:])))
        ref = qo.cheby(psi0.copy(), sp.csr_matrix(Heff), 0.3, qo.ChebyWrk(psi0, 30.0, -15.0, 0.3))
        if np.all(np.imag(kind_c) == 0):          # (a complex coefficient makes H non-Hermitian: cheby! is then only compared between the two paths)
            assert np.linalg.norm(outs[0][-1] - ref) < TOL
    # the knob toggled on a LIVE operator: full combination in between, then sparse updates again with drift
    # coefficients equal to what the base was built for -- the base must be rebuilt, not trusted
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M) for M in (H0, Hd, D1, D2)], ncoeffs=3, fmt=fmt)
    ref = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M) for M in (H0, Hd, D1, D2)], ncoeffs=3, fmt=fmt)
    try:
        live = 1 if Op.evaluate_info()["first_sparse_term"] > 0 else 0
        assert live == 1 or fmt == L.FMT_CSR
        ctx.tuning_set("sparse_controls", 1)
        Op.set_coeffs([0.5, -0.25, 0.1])
        assert Op.evaluate_info()["latest_update_sparse"] == live
        ctx.tuning_set("sparse_controls", 0)
        Op.set_coeffs([0.9, 0.3, 0.2])              # full combination: `combined` now holds 0.9 Hd everywhere
        assert Op.evaluate_info()["latest_update_sparse"] == 0
        ctx.tuning_set("sparse_controls", 1)
        Op.set_coeffs([0.5, -0.4, 0.6])             # drift coefficient 0.5 again: equal to the stale base's
        assert Op.evaluate_info()["latest_update_sparse"] == live
        ctx.tuning_set("sparse_controls", 0)
        ref.set_coeffs([0.5, -0.4, 0.6])
        assert np.array_equal(Op.get_csr()[2], ref.get_csr()[2])
    finally:
        ctx.tuning_set("sparse_controls", 1)


@pytest.mark.parametrize("fmt", [L.FMT_CSR, L.FMT_RBCSR, L.FMT_HRB])
def test_real_valued_operator_streams_real_copy(ctx, fmt):
    """An operator whose terms and coefficients are all real is streamed from a real copy of
    its values (8 instead of 16 bytes per entry).  The real value enters the same complex FMA
    sequence with a zero imaginary part: mul!, cheby! and newton! are bit-identical to the
    complex path (knob `real_vals` = 0), and a complex coefficient switches back."""
    N = 2000
    rp, col, val = synth.hermitian_offsets_csr(N, (1, 2, 7, 64), rho=6.0)
    H0 = synth.to_scipy(rp, col, val.real.astype(complex), N)          # real symmetric
    H1 = sp.diags([np.linspace(-1, 1, N)], [0], format="csr", dtype=complex)
    psi0 = synth.random_state(N)
    outs = []
    for knob in (1, 0):
        L.tuning_set("real_vals", knob)
        try:
            Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H0), L.Matrix.from_scipy(ctx, H1)], ncoeffs=1, fmt=fmt)
            res = []
            for cval in (0.5, -0.25):
                Op.set_coeffs([cval])
                x, y = L.State(ctx, data=psi0), L.State(ctx, n=N)
                Op.mul(x, y, 0.7 - 0.2j, 0.0)
                res.append(y.numpy())
                wrk = L.ChebyWrk(ctx, N, 16.0, -8.0, 0.3)
                for _ in range(2):
                    L.cheby(x, Op, 0.3, wrk)
                res.append(x.numpy())
                nw = L.NewtonWrk(ctx, N, m_max=8)
                L.newton(x, Op, 0.1, nw)
                res.append(x.numpy())
            rp2, col2, val2 = Op.get_csr()
            res.append(val2)
            Op.set_coeffs([0.5 + 0.5j])          # complex coefficient: complex values again
            x, y = L.State(ctx, data=psi0), L.State(ctx, n=N)
            Op.mul(x, y)
            res.append(y.numpy())
            outs.append(res)
        finally:
            L.tuning_set("real_vals", 1)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    Hc = (H0 + 0.5 * H1).tocsr()
    assert np.linalg.norm(outs[0][0] - (0.7 - 0.2j) * (Hc @ psi0)) < 1e-12
    Hz = (H0 + (0.5 + 0.5j) * H1).tocsr()
    assert np.linalg.norm(outs[0][-1] - Hz @ psi0) < 1e-12


# ---------------------------------------------------------------- matrix-free Liouvillian (N4)

def _dense_open_system(n, rng, nterms=2, nc=2):
    Hs = [synth.dense_hermitian(n, rho=2.0 if l == 0 else 0.7, rng=rng) for l in range(nterms)]
    cops = [0.3 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(n) for _ in range(nc)]
    return Hs, cops


@pytest.fixture(params=[(4096, 0), (0, 4096), (0, 0)], ids=["fused-mfma-16", "mfma-32", "rocblas"])
def liouville_path(request):
    """The three implementations of the matrix-free application: the hand-written fp64 matrix-core
    kernels -- 16 x 16 tiles (n <= 320 by default) and 32 x 32 tiles (260 <= n <= 2048 by default) -- and the chain of rocBLAS zgemm calls."""
    L.tuning_set("liouville_fused_n", request.param[0])
    L.tuning_set("liouville_tile32_n", request.param[1])
    L.tuning_set("liouville_tile32_min_n", 0)
    yield request.param
    L.tuning_set("liouville_fused_n", 320)
    L.tuning_set("liouville_tile32_n", 2048)
    L.tuning_set("liouville_tile32_min_n", 260)


@pytest.mark.parametrize("convention", ["TDSE", "LvN"])
@pytest.mark.parametrize("n,nterms,nc", [(3, 1, 0), (8, 2, 1), (33, 2, 2), (36, 1, 2), (64, 0, 1), (100, 1, 3), (150, 1, 1),
                                         (300, 2, 2)])
def test_matrix_free_liouvillian_matches_superoperator(ctx, liouville_path, convention, n, nterms, nc):
    """qp_liouvillian_create applies liouvillian(H, c_ops; convention) (src/generators.jl:473-631)
    as GEMMs on the n x n density matrix; the n^2 x n^2 sparse superoperator built from the
    reference's kron formulas is the check: mul! (3- and 5-argument), dot, coefficient updates,
    scale, both conventions, H only / c_ops only."""
    rng = np.random.default_rng(1000 + n)
    Hs, cops = _dense_open_system(n, rng, nterms, nc)
    ncoeffs = max(nterms - 1, 0)
    Lmf = L.Liouvillian(ctx, Hs, cops, ncoeffs=ncoeffs, convention=convention)
    assert Lmf.shape == (n * n, n * n) and Lmf.format == L.FMT_MATFREE
    rho = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    x = np.ascontiguousarray(rho.T).reshape(-1)            # column-major vec(rho)
    y0 = rng.standard_normal(n * n) + 1j * rng.standard_normal(n * n)
    for cvals, scale in (([1.0] * ncoeffs, 1.0), ([0.4 - 0.3j] * ncoeffs, 1.0), ([0.4] * ncoeffs, 0.5 - 1.5j)):
        Lmf.set_coeffs(cvals) if ncoeffs else None
        Lmf.set_scale(scale)
        if n <= 64:       # the stored superoperator (n^4 entries per dense Lindblad operator)
            Lref = sp.csr_matrix((n * n, n * n), dtype=complex)
            for l, H in enumerate(Hs):
                c = 1.0 if l < nterms - ncoeffs else cvals[l - (nterms - ncoeffs)]
                Lref = Lref + c * synth.ham_to_superop(sp.csr_matrix(H), convention)
            for A in cops:
                Lref = Lref + synth.lindblad_to_superop(sp.csr_matrix(A), convention)
            ref = (scale * Lref).tocsr() @ x
        else:             # the same map written out on rho (checked against the kron form above for small n)
            s_h, s_d = (1.0, 1j) if convention == "TDSE" else (1j, 1.0)
            H = sum((1.0 if l < nterms - ncoeffs else cvals[l - (nterms - ncoeffs)]) * Hl for l, Hl in enumerate(Hs))
            out = s_h * (H @ rho - rho @ H)
            for A in cops:
                G = A.conj().T @ A
                out = out + s_d * (A @ rho @ A.conj().T - 0.5 * (G @ rho + rho @ G))
            ref = scale * np.ascontiguousarray(out.T).reshape(-1)
        xs, ys = L.State(ctx, data=x), L.State(ctx, n=n * n)
        Lmf.mul(xs, ys)
        tol = 1e-12 * max(1.0, np.linalg.norm(ref))
        assert np.linalg.norm(ys.numpy() - ref) < tol
        ys.upload(y0)
        Lmf.mul(xs, ys, 0.7 - 0.2j, -0.3 + 0.1j)
        assert np.linalg.norm(ys.numpy() - ((-0.3 + 0.1j) * y0 + (0.7 - 0.2j) * ref)) < tol
        assert abs(Lmf.dot(xs, xs) - np.vdot(x, ref)) < tol
    # explicit physics check (TDSE: i d rho/dt = L rho):  L rho = [H, rho] + i D(rho)
    if convention == "TDSE":
        Lmf.set_scale(1.0)
        if ncoeffs:
            Lmf.set_coeffs([1.0] * ncoeffs)
        H = sum(Hs) if Hs else np.zeros((n, n))
        want = H @ rho - rho @ H
        for A in cops:
            G = A.conj().T @ A
            want = want + 1j * (A @ rho @ A.conj().T - 0.5 * (G @ rho + rho @ G))
        xs, ys = L.State(ctx, data=x), L.State(ctx, n=n * n)
        Lmf.mul(xs, ys)
        assert np.linalg.norm(ys.numpy() - np.ascontiguousarray(want.T).reshape(-1)) < 1e-12 * max(1.0, np.linalg.norm(want))
    with pytest.raises(L.QPError):
        Lmf.get_csr()


@pytest.mark.parametrize("n,nc", [(516, 2), (774, 1), (1024, 1)])
def test_matrix_free_liouvillian_paths_agree_at_size(ctx, n, nc):
    """The sizes the 32 x 32 matrix-core kernel is meant for (one with partial edge tiles, one with more workgroups than
    the chip holds at once): its L rho against the 16 x 16 kernel's, the library chain's and the map written out on rho
    in NumPy, 5-argument form included; a physical rho keeps trace L rho = 0 and L rho Hermitian (i d rho/dt = L rho)."""
    rng = np.random.default_rng(4000 + n)
    Hs, cops = _dense_open_system(n, rng, 1, nc)
    Lmf = L.Liouvillian(ctx, Hs, cops, convention="TDSE")
    psi = rng.standard_normal((n, 3)) + 1j * rng.standard_normal((n, 3))
    rho = psi @ psi.conj().T
    rho /= np.trace(rho).real
    x = np.ascontiguousarray(rho.T).reshape(-1)
    y0 = rng.standard_normal(n * n) + 1j * rng.standard_normal(n * n)
    out = Hs[0] @ rho - rho @ Hs[0]
    for A in cops:
        G = A.conj().T @ A
        out = out + 1j * (A @ rho @ A.conj().T - 0.5 * (G @ rho + rho @ G))
    ref = np.ascontiguousarray(out.T).reshape(-1)
    xs = L.State(ctx, data=x)
    res = {}
    try:
        for name, fused, tile in (("mfma16", 4096, 0), ("mfma32", 0, 4096), ("library", 0, 0)):
            ctx.tuning_set("liouville_fused_n", fused)
            ctx.tuning_set("liouville_tile32_n", tile)
            ys = L.State(ctx, n=n * n)
            Lmf.mul(xs, ys)
            a = ys.numpy()
            ys.upload(y0)
            Lmf.mul(xs, ys, 0.7 - 0.2j, -0.3 + 0.1j)
            res[name] = (a, ys.numpy())
    finally:
        ctx.tuning_set("liouville_fused_n", 320)
        ctx.tuning_set("liouville_tile32_n", 2048)
    scale = np.linalg.norm(ref)
    for name, (a, b5) in res.items():
        assert np.linalg.norm(a - ref) < 1e-13 * scale, name
        assert np.linalg.norm(b5 - ((-0.3 + 0.1j) * y0 + (0.7 - 0.2j) * ref)) < 1e-13 * (scale + np.linalg.norm(y0)), name
    Lrho = res["mfma32"][0].reshape(n, n).T
    assert abs(np.trace(Lrho)) < 1e-12 * scale
    assert np.linalg.norm(Lrho + Lrho.conj().T) < 1e-12 * scale      # L rho = i d rho/dt is anti-Hermitian


def test_matrix_free_liouvillian_newton_and_cheby(ctx, liouville_path):
    """Newton on the matrix-free Liouvillian equals Newton on the sparse superoperator and the
    oracle (trace preserved, rho stays Hermitian); without dissipation the superoperator is
    Hermitian and cheby! applies (unfused epilogue)."""
    rng = np.random.default_rng(77)
    n = 24
    Hs, cops = _dense_open_system(n, rng, 1, 2)
    psi = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    psi /= np.linalg.norm(psi)
    rho0 = np.outer(psi, psi.conj())
    x0 = np.ascontiguousarray(rho0.T).reshape(-1)
    Lsp = (synth.ham_to_superop(sp.csr_matrix(Hs[0]), "TDSE") + sum(synth.lindblad_to_superop(sp.csr_matrix(A), "TDSE") for A in cops)).tocsr()
    Lmf = L.Liouvillian(ctx, Hs, cops, convention="TDSE")
    Lop = L.Operator(ctx, [L.Matrix.from_scipy(ctx, Lsp)])
    outs = []
    for Op in (Lmf, Lop):
        xs = L.State(ctx, data=x0)
        wrk = L.NewtonWrk(ctx, n * n, m_max=10)
        for _ in range(5):
            L.newton(xs, Op, 0.2, wrk)
        outs.append(xs.numpy())
    assert np.linalg.norm(outs[0] - outs[1]) < 1e-11
    ref = x0.copy()
    owrk = qo.NewtonWrk(ref, m_max=10)
    for _ in range(5):
        ref = qo.newton(ref, Lsp, 0.2, owrk)
    assert np.linalg.norm(outs[0] - ref) < TOL
    rho = outs[0].reshape(n, n).T
    assert abs(np.trace(rho) - 1.0) < 1e-10 and np.linalg.norm(rho - rho.conj().T) < 1e-10
    # closed system: Hermitian superoperator, Chebyshev
    Lc = L.Liouvillian(ctx, Hs, (), convention="TDSE")
    Lcs = synth.ham_to_superop(sp.csr_matrix(Hs[0]), "TDSE").tocsr()
    xs = L.State(ctx, data=x0)
    wrk = L.ChebyWrk(ctx, n * n, 12.0, -6.0, 0.3)
    for _ in range(3):
        L.cheby(xs, Lc, 0.3, wrk)
    ref = x0.copy()
    owrk = qo.ChebyWrk(ref, 12.0, -6.0, 0.3)
    for _ in range(3):
        qo.cheby(ref, Lcs, 0.3, owrk)
    assert np.linalg.norm(xs.numpy() - ref) < TOL
    U = np.linalg.matrix_power(__import__("scipy.linalg", fromlist=["expm"]).expm(-1j * 0.3 * Hs[0]), 3)
    assert np.linalg.norm(xs.numpy().reshape(n, n).T - U @ rho0 @ U.conj().T) < 1e-9


# ---------------------------------------------------------------- property test over random operators

from hypothesis import HealthCheck, given, settings, strategies as st   # noqa: E402


@st.composite
def _random_operator(draw):
    """Band-structured + randomly perturbed sparse matrices: regular stencil blocks, wrap-around,
    ragged and empty rows, real or complex values, Hermitian or not, any size."""
    n = draw(st.integers(1, 700))
    seed = draw(st.integers(0, 2 ** 31 - 1))
    hermitian = draw(st.booleans())
    real = draw(st.booleans())
    n_offsets = draw(st.integers(0, 5))
    n_random = draw(st.integers(0, 60))
    n_empty = draw(st.integers(0, 3))
    rng = np.random.default_rng(seed)
    A = sp.lil_matrix((n, n), dtype=complex)
    val = (lambda k: rng.standard_normal(k)) if real else (lambda k: rng.standard_normal(k) + 1j * rng.standard_normal(k))
    for d in rng.integers(0, max(1, n // 2 + 1), n_offsets):
        rows = np.arange(n)
        A[rows, (rows + int(d)) % n] = val(n)
    if n_random:
        A[rng.integers(0, n, n_random), rng.integers(0, n, n_random)] = val(n_random)
    for r in rng.integers(0, n, n_empty):
        A[int(r), :] = 0
    A = sp.csr_matrix(A)
    if hermitian:
        A = sp.csr_matrix(A + A.conj().T)
    A.eliminate_zeros()
    A.sort_indices()
    return A, hermitian, real, seed


@pytest.mark.parametrize("fmt", [L.FMT_AUTO, L.FMT_CSR, L.FMT_RBCSR, L.FMT_HRB])
@settings(max_examples=int(os.environ.get("QP_HYP_EXAMPLES", "25")), deadline=None,
          derandomize="QP_HYP_EXAMPLES" not in os.environ,      # fixed examples by default; set the variable to explore
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(_random_operator())
def test_random_operators_all_formats(ctx, fmt, m):
    """Whatever the structure: the device copy reads back bit for bit, mul! and one cheby! term
    (through cheby_term, no spectral assumptions) match SciPy / the formula, and the real copy,
    stencil and int16 encodings (all on by default) never change a result."""
    A, hermitian, real, seed = m
    n = A.shape[0]
    hermitian = (abs(A - A.conj().T) > 0).nnz == 0          # a random draw can be Hermitian by accident
    if fmt == L.FMT_HRB and not hermitian:
        with pytest.raises(L.QPError):
            L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)], fmt=fmt)
        return
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)], fmt=fmt)
    rp, col, vals = Op.get_csr()
    assert np.array_equal(rp, A.indptr) and np.array_equal(col, A.indices) and np.array_equal(vals, A.data)
    rng = np.random.default_rng(seed + 1)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    y0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    xs, ys = L.State(ctx, data=x), L.State(ctx, data=y0)
    Op.mul(xs, ys, 0.3 - 0.7j, 1.1 + 0.2j)
    ref = (1.1 + 0.2j) * y0 + (0.3 - 0.7j) * (A @ x)
    scale = max(1.0, np.linalg.norm(ref))
    assert np.linalg.norm(ys.numpy() - ref) < 1e-12 * scale
    v0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    acc = L.State(ctx, data=y0)
    vout = L.State(ctx, data=v0)
    c, beta, a = 0.2 - 0.4j, 0.3, 0.7
    L.cheby_term(Op, xs, 0, vout, vout, acc, acc, c, beta, 0.0, a, 1.0)
    t = c * (A @ x - beta * x) + v0
    assert np.linalg.norm(vout.numpy() - t) < 1e-12 * max(1.0, np.linalg.norm(t))
    assert np.linalg.norm(acc.numpy() - (y0 + a * t)) < 1e-12 * max(1.0, np.linalg.norm(y0 + a * t))


@pytest.mark.parametrize("pipeline", [1, 0])
def test_newton_breakdown_multilaunch_path(ctx, pipeline):
    """Krylov space exhausted (src/arnoldi.jl:91-95, src/newton.jl:277-279) on the multi-launch
    Arnoldi path (more entries than the persistent kernel takes), where newton! computes the
    eigenvalues of the leading blocks while the later columns are still being orthogonalised:
    the columns after the breakdown are discarded, m shrinks to the Krylov dimension for all
    later restarts, and the result is exact.  Also with the pipeline switched off."""
    N = 20000
    rng = np.random.default_rng(5)
    lam = np.array([-3.0, 0.5, 2.0, 7.5])
    d = lam[rng.integers(0, 4, N)]
    A = sp.diags([d], [0], format="csr", dtype=complex)      # four distinct eigenvalues: Krylov dimension 4
    psi0 = _rand_state(N, rng)
    L.tuning_set("newton_pipeline", pipeline)
    try:
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)])
        q = L.Krylov(ctx, N, 11)
        Hess = np.zeros((11, 11), dtype=complex, order="F")
        m_out = L.arnoldi(Hess, q, 10, L.State(ctx, data=psi0), Op, 0.7, norm_min=1e-9)
        assert m_out == 4 and np.all(Hess[:, 4:] == 0)
        out, ref, wrk, owrk = _newton_case(ctx, A, psi0, 0.7, 10, norm_min=1e-9)
        assert np.linalg.norm(out - np.exp(-0.7j * d) * psi0) < TOL
        assert np.linalg.norm(out - ref) < TOL
        assert wrk.restarts == owrk.restarts
    finally:
        L.tuning_set("newton_pipeline", 1)


def test_independent_handles_from_concurrent_threads():
    """SURVEY 8b threading contract: callers step many independent propagators from their own
    threads; every context owns its stream, there is no shared mutable state, so qp_* calls on
    different handles may run concurrently (ctypes releases the GIL) and each thread reproduces
    the single-threaded result bit for bit."""
    import threading
    N = 6000
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 17, 64, 200, 511, 900))
    Lm = synth.liouvillian_tridiag(20)
    nthreads = 4

    def work(seed, out, k):
        try:
            c = L.Context(0)
            op = L.Operator(c, [L.Matrix(c, N, N, rp, col, vals)])
            psi = L.State(c, data=synth.random_state(N, seed=seed))
            wrk = L.ChebyWrk(c, N, 20.0, -10.0, 0.7)
            for _ in range(25):
                L.cheby(psi, op, 0.7, wrk)
            lop = L.Operator(c, [L.Matrix.from_scipy(c, Lm)])
            rho = L.State(c, data=synth.random_state(Lm.shape[0], seed=seed + 100))
            nw = L.NewtonWrk(c, Lm.shape[0], m_max=12)
            for _ in range(4):
                L.newton(rho, lop, 0.4, nw)
            out[k] = (psi.numpy(), rho.numpy())
            c.close()
        except Exception as e:  # noqa: BLE001
            out[k] = e

    serial = [None] * nthreads
    for k in range(nthreads):
        work(1000 + k, serial, k)
    threaded = [None] * nthreads
    ts = [threading.Thread(target=work, args=(1000 + k, threaded, k)) for k in range(nthreads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in range(nthreads):
        assert not isinstance(serial[k], Exception), serial[k]
        assert not isinstance(threaded[k], Exception), threaded[k]
        assert np.array_equal(serial[k][0], threaded[k][0]) and np.array_equal(serial[k][1], threaded[k][1])
        assert abs(np.linalg.norm(serial[k][0]) - 1.0) < 1e-12


def test_newton_long_krylov_basis(ctx):
    """m_max = 120: beyond the Krylov length whose Gram triangle the low-synchronisation solve keeps
    in LDS (j <= 87), the later columns continue with the sequential Gram-Schmidt passes -- same
    result, one restart."""
    rng = np.random.default_rng(77)
    N = 1500
    H = synth.sparse_random(N, 24.0 / N, rho=6.0, hermitian=True, rng=rng)     # > 16384 entries: multi-launch path
    psi0 = _rand_state(N, rng)
    out, ref, wrk, owrk = _newton_case(ctx, H, psi0, 2.0, 120)
    import scipy.sparse.linalg as spla
    exact = spla.expm_multiply(-2.0j * sp.csc_matrix(H), psi0)
    assert np.linalg.norm(out - exact) < TOL and np.linalg.norm(out - ref) < TOL
    assert wrk.restarts == owrk.restarts


@pytest.mark.parametrize("batch", [40, 8])
def test_cheby_batched_streaming_variants_bit_identical(ctx, batch):
    """Knob of the batched kernel: the nontemporal variant (picked automatically for panels larger than the caches, forced here
    on a small one) changes the memory access pattern only -- every (row, state) element sees the same FMA sequence; panels of
    40 states (tiles of 16) and of 8 (one tile)."""
    N = 1500
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4, 16, 32, 48, 300))
    Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)])
    states = np.stack([synth.random_state(N, seed=2000 + s) for s in range(batch)], axis=1)
    outs = {}
    try:
        for nt in (0, 2):
            L.tuning_set("spmm_nt", nt)
            wrk = L.ChebyWrk(ctx, N * batch, 20.0, -10.0, 0.9)
            panel = L.State(ctx, data=states.reshape(-1))
            for dt in (0.9, -0.9, 0.9):
                L.cheby_batched(panel, Op, dt, wrk, batch)
            outs[nt] = panel.numpy()
    finally:
        L.tuning_set("spmm_nt", 1)
    assert np.array_equal(outs[0], outs[2])
    wrk = L.ChebyWrk(ctx, N * batch, 20.0, -10.0, 0.9)
    panel = L.State(ctx, data=states.reshape(-1))
    for dt in (0.9, -0.9, 0.9):
        L.cheby_batched(panel, Op, dt, wrk, batch)
    assert np.array_equal(panel.numpy(), outs[0])            # the tile does not change any value either
    assert np.max(np.abs(np.linalg.norm(outs[0].reshape(N, batch), axis=0) - 1.0)) < 1e-12


@pytest.mark.parametrize("batch", [40, 64, 70])
def test_cheby_batched_rows_kernel_and_row_walk_bit_identical(ctx, batch):
    """Panels of more than 32 states take the wave-per-row kernel (lane = state, matrix entries
    broadcast through SGPRs).  It sums a row in the order of the tiled kernel, and the strip-wise row
    walk (tensor-structured H: far offsets multiples of g = 256 here) is index work only: tiled kernel,
    natural order, automatic and forced strips, matrix entries through the scalar unit (the default) or one per
    lane with one to eight rows per wavefront all give the same bits, and the oracle's values."""
    N = 8192
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4, 256, 512, 768, 1024))
    Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)])
    H = synth.to_scipy(rp, col, vals, N)
    states = np.stack([synth.random_state(N, seed=3000 + s) for s in range(batch)], axis=1)
    outs, walks = {}, {}
    try:
        for rows, strip, rw in ((0, 0, 1), (1, -1, 1), (1, 0, 1), (1, 32, 1), (1, 64, 1), (1, 48, 1), (1, 32, 2), (1, 64, 4), (1, -1, 8), (1, -1, 0), (1, 0, 0), (1, 64, 0),
                                (1, 0, -1), (1, 32, -1)):
            ctx.tuning_set("spmm_rows", rows)
            ctx.tuning_set("spmm_strip", strip)
            ctx.tuning_set("spmm_rw", rw)
            wrk = L.ChebyWrk(ctx, N * batch, 20.0, -10.0, 0.7)
            panel = L.State(ctx, data=states.reshape(-1))
            for dt in (0.7, -0.7, 0.7):
                L.cheby_batched(panel, Op, dt, wrk, batch)
            outs[(rows, strip, rw)] = panel.numpy()
            if rw == 1:
                walks[(rows, strip)] = Op.spmm_walk(batch)
            if rw == -1:      # the LDS-staged tiles (the default): strip steps 4 .. 27 of 32 are interior, 6 x 64 tiles; the rest by the row kernel
                assert Op.spmm_tiles(batch) == {"taken": 1, "tiles": 384, "rest_rows": N - 16 * 384, "g": 256, "K": 4, "NN": 4}
            else:
                assert Op.spmm_tiles(batch)["taken"] == 0
    finally:
        ctx.tuning_set("spmm_rows", 1)
        ctx.tuning_set("spmm_strip", 0)
        ctx.tuning_set("spmm_rw", -1)
    ref = outs[(0, 0, 1)]
    for k, v in outs.items():
        assert np.array_equal(v, ref), k
    assert walks[(1, -1)] == (0, 0)
    assert walks[(1, 32)] == (256, 32) and walks[(1, 64)] == (256, 64)
    assert walks[(1, 48)] == (256, 32)          # strips divide the inner dimension
    owrk = qo.ChebyWrk(states[:, 0].copy(), 20.0, -10.0, 0.7)
    for s in (0, batch - 1):
        r = qo.cheby(states[:, s].copy(), H, 0.7, owrk)
        assert np.linalg.norm(ref.reshape(N, batch)[:, s] - r) < TOL


def test_spmm_row_walk_detection(ctx):
    """Which patterns get a strip-wise row walk: the BASELINE lattice (inner dimension 1024, strips of
    64 inner indices at 64 states); not a scattered pattern (no common inner dimension), not a
    plain band (no far offsets)."""
    N = 1 << 15
    for offs, want in ((synth.BANDED_OFFSETS, (1024, 64)), (synth.scattered_offsets(N), (0, 0)), ((1, 2, 3, 4, 5, 6, 7, 8), (0, 0))):
        rp, col, vals = synth.hermitian_offsets_csr(N, offsets=offs)
        Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)])
        assert Op.spmm_walk(64) == want, (offs, Op.spmm_walk(64))
        Op.close()


@pytest.mark.parametrize("N", [100, 128])
def test_newton_dense_128_persistent_arnoldi(ctx, N):
    """Config C1's size through newton!: 10000 / 16384 stored entries run the Arnoldi sweeps in the
    32-slot variants of the persistent single-workgroup kernel; same result as the multi-launch path
    (to rounding) and as the oracle."""
    rng = np.random.default_rng(N)
    H = synth.dense_hermitian(N, rho=5.0, rng=rng)
    psi0 = _rand_state(N, rng)
    out, ref, wrk, owrk = _newton_case(ctx, H, psi0, 0.3, 10)
    assert np.linalg.norm(out - ref) < TOL and wrk.restarts == owrk.restarts
    ev, V = np.linalg.eigh(H)
    assert np.linalg.norm(out - V @ (np.exp(-0.3j * ev) * (V.conj().T @ psi0))) < TOL
    st0 = ctx.stats()["n_kernel_launches"]
    L.newton(L.State(ctx, data=psi0), L.Operator(ctx, [L.Matrix.from_dense(ctx, H)]), 0.3, L.NewtonWrk(ctx, N, m_max=10))
    small_launches = ctx.stats()["n_kernel_launches"] - st0
    L.tuning_set("small_nnz", 0)
    try:
        out_g, _, _, _ = _newton_case(ctx, H, psi0, 0.3, 10)
        st1 = ctx.stats()["n_kernel_launches"]
        L.newton(L.State(ctx, data=psi0), L.Operator(ctx, [L.Matrix.from_dense(ctx, H)]), 0.3, L.NewtonWrk(ctx, N, m_max=10))
        general_launches = ctx.stats()["n_kernel_launches"] - st1
    finally:
        L.tuning_set("small_nnz", 8192)
    assert np.linalg.norm(out - out_g) < 1e-12
    assert small_launches * 3 < general_launches          # one launch per sweep instead of ~5 per column


def test_handles_destroyed_in_any_order():
    """C-ABI convention: finalizers run in no particular order, so a context may be destroyed before
    the handles made from it; their destroy calls still succeed and compute calls fail cleanly."""
    import ctypes as C
    c = L.Context(0)
    lib = c.lib
    N = 500
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 7, 30))
    op = L.Operator(c, [L.Matrix(c, N, N, rp, col, vals)])
    x, y = L.State(c, data=synth.random_state(N)), L.State(c, n=N)
    wrk = L.ChebyWrk(c, N, 20.0, -10.0, 0.5)
    kry = L.Krylov(c, N, 6)
    L.cheby(x, op, 0.5, wrk)
    c.sync()
    assert lib.qp_ctx_destroy(c._h) == 0                 # the context goes first ...
    assert lib.qp_ctx_destroy(c._h) == 0                 # ... (idempotent) ...
    st = lib.qp_mul(op._h, x._h, y._h, L.c128(1.0), L.c128(0.0))
    assert st != 0 and b"context" in lib.qp_last_error()  # ... compute calls say so ...
    for h in (kry, wrk, y, x, op):                        # ... and the children can still be destroyed
        h.close()
    c._h = C.c_void_p()                                   # nothing left for Context.close()


def test_host_register_pinned_transfers(ctx):
    """qp_host_register / qp_host_unregister: a caller-owned (pinned) array as the source / target of
    uploads and downloads -- same bytes as through pageable memory."""
    N = 1 << 18
    a = synth.random_state(N)
    pinned = L.host_register(a.copy())
    try:
        s = L.State(ctx, data=pinned)
        out = L.host_register(np.empty(N, dtype=np.complex128))
        try:
            s.download(out)
            assert np.array_equal(out, a) and np.array_equal(s.numpy(), a)
            s.upload(out * 2)
            assert np.array_equal(s.numpy(), 2 * a)
        finally:
            L.host_unregister(out)
    finally:
        L.host_unregister(pinned)
    with pytest.raises(L.QPError):
        L.host_unregister(np.empty(16, dtype=np.complex128))     # was never registered


def test_walk_reason_says_what_broke_the_plan(ctx):
    """qp_operator_walk_reason: the fused term's fast path is a cliff; an operator that falls off it is told why, with the
    offending numbers.  One operator per way of falling, plus the ones that walk."""
    import warnings
    ctx.tuning_set("walk_min_blocks", 64)
    try:
        N = 1 << 14

        def reason(offsets, fmt=L.FMT_AUTO, hermitian=True, coeff=None):
            rp, col, vals = synth.hermitian_offsets_csr(N, offsets=offsets)
            if not hermitian:
                vals = vals * (1.0 + 0.5 * (np.arange(len(vals)) % 3 == 0))
            op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)], 1 if coeff is not None else 0, fmt)
            if coeff is not None:
                op.set_coeffs([coeff])
            r = op.walk_reason()
            return op, r

        op, r = reason((1, 2, 3, 4, 256, 512, 768, 1024))
        assert r[0] == 0 and r[1] == "ok" and op.walk_info()["valid"] == 1
        op, r = reason((1, 17, 256))
        assert r[1] == "near_too_far" and "17" in r[2] and op.walk_info()["valid"] == 0
        op, r = reason((1, 2, 3, 4, 5, 256))
        assert r[1] == "too_many_near" and "5 near" in r[2]
        op, r = reason((1, 256, 512, 768, 1024, 1280))             # read as four strides + one long pair: no such kernel
        assert r[1] == "no_kernel_instance" and "long pair" in r[2]
        op, r = reason((1, 256, 512, 768, 1024, 1280, 1536))       # four strides + two long pairs: no such kernel either
        assert r[1] == "no_kernel_instance"
        op, r = reason((1, 256, 512, 768, 1024, 1280, 1536, 1792))
        assert r[1] == "too_many_far"
        op, r = reason((1, 256, 600))                              # one stride + one long pair (any distance): walks
        assert r[1] == "ok" and op.walk_info()["long_distance"] == 600 and op.walk_info()["long_distances"] == [600]
        op, r = reason((1, 256, 600, 1000))                        # ... + two long pairs: walks (round 4)
        assert r[1] == "ok" and op.walk_info()["long_distances"] == [600, 1000] and op.walk_info()["long_distance"] == 1000
        op, r = reason((1, 2, 256, 512, 2000, 4000))               # the thirteen-point stencil of a three-dimensional grid
        wi = op.walk_info()
        assert r[1] == "ok" and wi["near"] == 2 and wi["far"] == 2 and wi["long_distances"] == [2000, 4000]
        op, r = reason((1, 255, 256, 257))                         # nine-point stencil with diagonal neighbours: walks (round 4)
        wi = op.walk_info()
        assert r[1] == "ok" and wi["far_diagonals"] == 1 and wi["far"] == 1 and wi["rows_per_step"] == 256 and wi["upper_slots"] == 4
        op, r = reason((1, 256, 257))                              # one diagonal neighbour only, read as a long pair beside the ring: per-block kernel
        assert r[1] == "no_kernel_instance" and "diagonal neighbour" in r[2] and op.walk_info()["valid"] == 0
        op, r = reason((1, 2, 3, 255, 256, 257))
        assert r[1] == "no_kernel_instance" and "diagonal far neighbours" in r[2]
        op, r = reason((1, 256, 600, 1000, 1500))
        assert r[1] == "incommensurate_strides" and "256" in r[2]
        op, r = reason((1, 2, 3))
        assert r[1] == "no_far_distance"
        op, r = reason((256, 512))
        assert r[1] == "no_near_distance"
        op, r = reason((1, 2, 256), hermitian=False)
        assert r[1] == "not_hermitian"
        op, r = reason((1, 2, 256), fmt=L.FMT_RBCSR)
        assert r[1] in ("not_hermitian", "not_packed")          # (a forced plain format is not checked for Hermiticity)
        op, r = reason((1, 2, 256), coeff=1.0)
        assert r[1] == "ok"
        op.set_coeffs([1.0 + 0.5j])                              # a complex coefficient un-packs the operator
        assert op.walk_reason()[1] == "complex_coefficient" and op.build_info()["relayouts"] == 1
        ctx.tuning_set("walk_min_blocks", 3072)
        op, r = reason((1, 2, 256))
        assert r[1] == "too_few_blocks" and "3072" in r[2]
        ctx.tuning_set("hrb_walk", 0)
        ctx.tuning_set("walk_min_blocks", 64)
        op, r = reason((1, 2, 256))
        assert r[1] == "disabled"
        ctx.tuning_set("hrb_walk", 1)
        # the Python wrapper warns once, at the first cheby! of a large operator that fell off for a reason worth telling
        N2 = 64 * 80
        rp, col, vals = synth.hermitian_offsets_csr(N2, offsets=(1, 17, 256))
        opw = L.Operator(ctx, [L.Matrix(ctx, N2, N2, rp, col, vals)])
        wrk = L.ChebyWrk(ctx, N2, 20.0, -10.0, 0.1)
        psi = L.State(ctx, data=synth.random_state(N2))
        with warnings.catch_warnings(record=True) as got:
            warnings.simplefilter("always")
            L.cheby(psi, opw, 0.1, wrk)
            L.cheby(psi, opw, 0.1, wrk)
        msgs = [w for w in got if issubclass(w.category, L.QPPerformanceWarning)]
        assert len(msgs) == 1 and "near_too_far" in str(msgs[0].message)
    finally:
        ctx.tuning_set("walk_min_blocks", 3072)
        ctx.tuning_set("hrb_walk", 1)


def test_lattice_completion_only_where_it_buys_the_walk(ctx):
    """the explicit zeros of the lattice completion are for operators that END UP Hermitian-packed with a strip-walk
    plan.  A lattice-shaped operator that is not Hermitian (a non-Hermitian term on the grid's pattern), or a Hermitian one whose
    layout is forced to plain row blocks, keeps the pattern it was given: same nnz, get_csr() identical to the input -- and a
    non-finite vector entry next to a (would-be) stored zero stays what the reference's mat-vec makes of it."""
    nx, ny = 100, 80
    H = synth.grid_hamiltonian_2d(nx, ny, flux=0.2)
    N = nx * ny
    saved = {k: ctx.tuning_get(k) for k in ("walk_min_blocks",)}
    try:
        ctx.tuning_set("walk_min_blocks", 64)
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)])
        assert Op.fill_info() > 0 and Op.walk_info()["valid"] == 1          # Hermitian: completed and walked
        A = H.copy().tocsr()
        A.data = A.data * (1.0 + 0.25 * (np.arange(A.nnz) % 5 == 0))        # same pattern, no longer Hermitian
        for M, fmt in ((A, L.FMT_AUTO), (H, L.FMT_RBCSR), (H, L.FMT_CSR)):
            Op2 = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M)], 0, fmt)
            assert Op2.fill_info() == 0 and Op2.nnz == M.nnz and Op2.format != L.FMT_HRB
            rp, col, val = Op2.get_csr()
            assert np.array_equal(rp, M.indptr) and np.array_equal(col, M.indices) and np.array_equal(val, M.data)
            x = synth.random_state(N)
            x[nx * 5] = np.inf                                               # row nx*5 - 1 (an x-edge row) has no entry in this column
            y = L.State(ctx, n=N)
            Op2.mul(L.State(ctx, data=x), y)
            out = y.numpy()
            assert np.isfinite(out[nx * 5 - 1])                              # 0 * Inf = NaN if a zero had been stored there
            Op2.close()
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
