"""GPU tests of the batched panel kernels (csrc/kernels_spmm.hip: csr_spmm_kernel<8 | 16>, spmm_rows_smem_kernel, spmm_rows_kernel<1, 2,
4, 8>, spmm_tile_kernel with its rest rows, gather_csr_vals_kernel) on IRREGULAR operators -- tests/panel_cases.py: rows of every length
from 0 to 131 next to each other, union rows of three 64-entry chunks, sizes that are no multiple of any tile -- where every other
panel test runs a lattice whose rows all have one length.  All kernels must sum a row in one order (the same bits under every knob),
and every state of every panel must lie within 1e-10 of the oracle's `cheby!` (src/cheby.jl:150-213)."""
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
import panel_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-10
KNOBS = ("spmm_rows", "spmm_rw", "spmm_strip", "spmm_nt")
FORMATS = {"hrb": L.FMT_HRB, "rbcsr": L.FMT_RBCSR, "csr": L.FMT_CSR}
LADDER = dict(Delta=2.4, E_min=-1.2, dts=(3.0, 2.5))      # 20 and 19 Chebychev coefficients: an even and an odd number of terms
PAIR = dict(Delta=5.0, E_min=-2.5, dt=1.5, coeffs=(0.7, -0.3, 0.5j, 1.2))
WIDEST = 130

_oracle = {}        # per operator (and time step): the oracle's result for the widest panel; narrower panels are prefixes of it
_worst = [0.0]      # largest distance from the oracle over all cases of this file (printed with -s)


@pytest.fixture()
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def _panel_step(ctx, Op, states, dts, wrk, **knobs):
    """`dts` batched steps of the panel `states` [N, b] under the given knobs; returns the panel [N, b]."""
    for k, v in knobs.items():
        ctx.tuning_set(k, v)
    N, b = states.shape
    panel = L.State(ctx, data=np.ascontiguousarray(states).reshape(-1))
    for dt in dts:
        L.cheby_batched(panel, Op, dt, wrk, b)
    out = panel.numpy().reshape(N, b)
    panel.close()
    return out


def _check_oracle(got, ref, what):
    err = np.linalg.norm(got - ref[:, :got.shape[1]], axis=0)
    _worst[0] = max(_worst[0], float(err.max()))
    print(f"{what}: largest distance from the oracle {err.max():.3e} (state {int(err.argmax())}); over this file so far {_worst[0]:.3e}")
    assert np.all(err < TOL), f"{what}: state {int(err.argmax())} is {err.max():.3e} from the oracle"


def _ladder_oracle(name, H, dt):
    key = (name, dt)
    if key not in _oracle:
        _oracle[key] = pc.oracle_steps(H, pc.panel_states(H.shape[0], WIDEST), L.cheby_coeffs(LADDER["Delta"], dt), LADDER["Delta"],
                                       LADDER["E_min"], (dt, -dt, dt))
    return _oracle[key]


def _assert_csr_round_trip(Op, M):
    rp, col, val = Op.get_csr()
    assert np.array_equal(rp, M.indptr) and np.array_equal(col, M.indices) and np.array_equal(val, M.data)


# ---------------------------------------------------------------- a. every kernel at every row length

@pytest.mark.parametrize("batch", [1, 3, 8, 9, 16, 17, 33, 64, 65, 130])
@pytest.mark.parametrize("fmt", list(FORMATS), ids=list(FORMATS))
def test_panel_kernels_bit_identical_at_every_row_length(ctx, fmt, batch):
    """The default ladder (rows of 0 .. 25, 31 .. 33, 63 .. 67, 127 .. 131 entries, mixed within 79 of its 80 groups of 16 rows; N = 1266) from each
    device format: the state-tiled kernel (TS = 8 up to eight states, else 16) gives the reference bits; its nontemporal variant
    and, for panels of more than 32 states, the wave-per-row kernels -- matrix entries through the scalar unit (spmm_rw <= 0) or one
    per lane with 1, 2, 4, 8 rows per wavefront (64-entry chunks: rows of 65 .. 131 entries reload), with and without nontemporal
    streams, any strip knob -- give the same bits; no lattice: no tiles, no row walk.  Three steps (dt, -dt, dt) at an even and an
    odd number of terms; every state against the oracle."""
    M = pc.ladder()[0]
    N = M.shape[0]
    states = pc.panel_states(N, batch)
    saved = {k: ctx.tuning_get(k) for k in KNOBS}
    outs = {}
    try:
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M)], 0, FORMATS[fmt])
        assert Op.format == FORMATS[fmt]
        _assert_csr_round_trip(Op, M)
        assert Op.spmm_tiles(batch)["taken"] == 0 and Op.spmm_walk(batch) == (0, 0)
        variants = [dict(spmm_rows=0, spmm_nt=2)]
        if batch > 32:
            variants += [dict(spmm_rows=1, spmm_rw=rw, spmm_nt=nt) for rw in (-1, 0, 1, 2, 4, 8) for nt in (0, 2)]
            variants += [dict(spmm_rows=1, spmm_rw=3)]                                    # no such instance: RW = 1
            variants += [dict(spmm_rows=1, spmm_rw=0, spmm_strip=strip) for strip in (-1, 0, 32)]
        for dt in LADDER["dts"]:
            wrk = L.ChebyWrk(ctx, N * batch, LADDER["Delta"], LADDER["E_min"], dt)
            assert np.array_equal(wrk.coeffs, L.cheby_coeffs(LADDER["Delta"], dt)) and wrk.n_coeffs == {3.0: 20, 2.5: 19}[dt]
            steps = (dt, -dt, dt)
            ref = _panel_step(ctx, Op, states, steps, wrk, **{**saved, "spmm_rows": 0, "spmm_nt": 0})
            for knobs in variants:
                got = _panel_step(ctx, Op, states, steps, wrk, **{**saved, **knobs})
                assert np.array_equal(got, ref), (f"dt={dt} {knobs}: off by up to {np.max(np.abs(got - ref)):.3e}, in rows of "
                                                  f"{np.unique(np.diff(M.indptr)[np.any(got != ref, axis=1)]).tolist()} entries")
                if batch > 32:
                    assert Op.spmm_tiles(batch)["taken"] == 0 and Op.spmm_walk(batch) == (0, 0), knobs
            outs[dt] = ref
            wrk.close()
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    for dt in LADDER["dts"]:
        _check_oracle(outs[dt], _ladder_oracle("ladder", M, dt), f"ladder {fmt} b={batch} dt={dt}")


def test_rows_kernel_last_wavefront_at_an_odd_size(ctx):
    """The ladder with one more empty row (N = 1267: odd, 3 past a multiple of 4 and of 8): the last wavefront of the wave-per-row
    kernel holds 1 of 2, 3 of 4 and 3 of 8 rows, where N = 1266 gives a full one, 2 of 4 and 2 of 8."""
    M = pc.ladder(n_empty=pc.DEFAULT_EMPTY + 1)[0]
    N, batch, dt = M.shape[0], 65, LADDER["dts"][0]
    assert N == 1267 and N % 2 == 1 and N % 4 == 3 and N % 8 == 3
    states = pc.panel_states(N, batch)
    saved = {k: ctx.tuning_get(k) for k in KNOBS}
    try:
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M)], 0, L.FMT_RBCSR)
        _assert_csr_round_trip(Op, M)
        wrk = L.ChebyWrk(ctx, N * batch, LADDER["Delta"], LADDER["E_min"], dt)
        ref = _panel_step(ctx, Op, states, (dt, -dt, dt), wrk, **{**saved, "spmm_rows": 0, "spmm_nt": 0})
        for rw in (-1, 0, 1, 2, 4, 8):
            got = _panel_step(ctx, Op, states, (dt, -dt, dt), wrk, **{**saved, "spmm_rows": 1, "spmm_rw": rw})
            assert np.array_equal(got, ref), (rw, float(np.max(np.abs(got - ref))))
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    _check_oracle(ref, pc.oracle_steps(M, states, L.cheby_coeffs(LADDER["Delta"], dt), LADDER["Delta"], LADDER["E_min"], (dt, -dt, dt)),
                  "ladder of odd size")


# ---------------------------------------------------------------- b. automatic format

@pytest.mark.parametrize("batch", [8, 130])
def test_panel_on_the_ladder_in_the_automatic_format(ctx, batch):
    """The same ladder through FMT_AUTO, whichever format the build picks (a dense format sends the panel to the matrix-core kernel:
    no knob comparison here), against the oracle."""
    M = pc.ladder()[0]
    N = M.shape[0]
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M)])
    assert Op.format in (L.FMT_CSR, L.FMT_RBCSR, L.FMT_HRB, L.FMT_DENSE), Op.format
    if Op.format != L.FMT_DENSE:
        _assert_csr_round_trip(Op, M)
    states = pc.panel_states(N, batch)
    for dt in LADDER["dts"]:
        wrk = L.ChebyWrk(ctx, N * batch, LADDER["Delta"], LADDER["E_min"], dt)
        got = _panel_step(ctx, Op, states, (dt, -dt, dt), wrk)
        _check_oracle(got, _ladder_oracle("ladder", M, dt), f"ladder in the automatic format (chose format {Op.format}) b={batch} dt={dt}")
        wrk.close()


# ---------------------------------------------------------------- c. lazy sum, evaluate!, leaving the packed format

def _pair_oracle():
    if "pair" not in _oracle:
        M0, M1 = pc.ladder_pair()
        cur = pc.panel_states(M0.shape[0], 64)
        refs = []
        for c in PAIR["coeffs"]:
            cur = pc.oracle_steps((M0 + c * M1).tocsr(), cur, L.cheby_coeffs(PAIR["Delta"], PAIR["dt"]), PAIR["Delta"], PAIR["E_min"],
                                  (PAIR["dt"],))
            refs.append(cur)
        _oracle["pair"] = refs
    return _oracle["pair"]


@pytest.mark.parametrize("batch", [8, 64])
@pytest.mark.parametrize("fmt", ["hrb", "rbcsr"])
def test_panel_lazy_sum_follows_coefficients_and_the_relayout(ctx, fmt, batch):
    """H0 + c H1 of two ladders with different permutations (union rows of up to three 64-entry chunks, 143 distinct lengths), c = 0.7,
    -0.3, 0.5j, 1.2 in turn (evaluate!, src/generators.jl:757-766): after each set_coeffs one step of the panel at the default knobs and
    one with the state-tiled kernel -- same bits, and the oracle's values.  The CSR-ordered mirror is gathered anew from the
    device values each time (conj-transposed entries of non-stencil blocks when Hermitian-packed); the complex coefficient takes a
    packed operator to another format, which frees and rebuilds the mirror; the steps after it must still be right."""
    M0, M1 = pc.ladder_pair()
    N = M0.shape[0]
    saved = {k: ctx.tuning_get(k) for k in KNOBS}
    try:
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M0), L.Matrix.from_scipy(ctx, M1)], 1, FORMATS[fmt])
        assert Op.format == FORMATS[fmt] and Op.build_info()["relayouts"] == 0
        wrk = L.ChebyWrk(ctx, N * batch, PAIR["Delta"], PAIR["E_min"], PAIR["dt"])
        assert wrk.n_coeffs == 21
        cur_default = cur_tiled = pc.panel_states(N, batch)
        for step, c in enumerate(PAIR["coeffs"]):
            Op.set_coeffs([c])
            bi = Op.build_info()
            if fmt == "hrb" and step >= 2:      # a complex combination of Hermitian terms is not Hermitian: the packed format was left
                assert Op.format != L.FMT_HRB and bi["format"] == Op.format and bi["relayouts"] == 1, (c, Op.format, bi)
            else:
                assert Op.format == FORMATS[fmt] and bi["relayouts"] == 0, (c, Op.format, bi)
            if Op.format != L.FMT_DENSE:
                rp, col, val = Op.get_csr()
                H = (M0 + c * M1).tocsr()
                U = (abs(M0) + abs(M1)).tocsr()
                U.sort_indices()
                assert np.array_equal(rp, U.indptr) and np.array_equal(col, U.indices)
                assert abs(sp.csr_matrix((val, col, rp), shape=(N, N)) - H).max() < 1e-15
            cur_default = _panel_step(ctx, Op, cur_default, (PAIR["dt"],), wrk, **saved)
            cur_tiled = _panel_step(ctx, Op, cur_tiled, (PAIR["dt"],), wrk, **{**saved, "spmm_rows": 0})
            assert np.array_equal(cur_default, cur_tiled), (c, float(np.max(np.abs(cur_default - cur_tiled))))
            _check_oracle(cur_default, _pair_oracle()[step], f"lazy sum {fmt} (now format {Op.format}) b={batch} after c={c}")
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)


# ---------------------------------------------------------------- d. real and few-valued operator

@pytest.mark.parametrize("batch", [8, 64])
@pytest.mark.parametrize("fmt", ["hrb", "rbcsr"])
def test_panel_real_few_valued_operator(ctx, fmt, batch):
    """A ladder with real symmetric blocks of four distinct values: Hermitian-packed it streams the real copy of its values, as plain
    row blocks the value dictionary (csrc/kernels_coded.hip) replaces the value plane for the mat-vec; the panel's mirror must gather
    the right complex values either way."""
    M = pc.real_few_valued()[0]
    N = M.shape[0]
    saved = {k: ctx.tuning_get(k) for k in KNOBS}
    outs = {}
    try:
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M)], 0, FORMATS[fmt])
        vi = Op.value_encoding_info()
        real_copy = vi["plane_bytes"] == 8 * Op.layout_info()["stored"]
        print(f"real few-valued {fmt}: value dictionary {vi}, real copy {real_copy}")
        assert real_copy, vi
        assert vi["valid"] == (1 if fmt == "rbcsr" else 0), vi
        _assert_csr_round_trip(Op, M)
        states = pc.panel_states(N, batch)
        dt = LADDER["dts"][0]
        wrk = L.ChebyWrk(ctx, N * batch, LADDER["Delta"], LADDER["E_min"], dt)
        for rows in (0, 1):
            outs[rows] = _panel_step(ctx, Op, states, (dt, -dt, dt), wrk, **{**saved, "spmm_rows": rows})
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    assert np.array_equal(outs[0], outs[1])
    key = ("real", dt)
    if key not in _oracle:
        _oracle[key] = pc.oracle_steps(M, pc.panel_states(N, 64), L.cheby_coeffs(LADDER["Delta"], dt), LADDER["Delta"], LADDER["E_min"],
                                       (dt, -dt, dt))
    _check_oracle(outs[0], _oracle[key], f"real few-valued {fmt} b={batch}")


# ---------------------------------------------------------------- e. a lattice that needs completion

@pytest.mark.parametrize("batch", [64, 70])
def test_panel_on_an_open_boundary_grid_filled_and_not(ctx, batch):
    """The finite-difference Hamiltonian of a 128 x 40 grid with open boundaries (N = 5120): with lattice_fill the operator's rows
    are completed with explicit zeros, which the mirror holds, and the rows at the grid's edges are the tile kernel's rest rows;
    without it the rows have 3 .. 5 entries.  LDS tiles (where the plan takes them), scalar-entry rows and the state-tiled kernel
    give the same bits for each; both agree with the oracle, and with each other to rounding."""
    nx, ny = 128, 40
    H = synth.grid_hamiltonian_2d(nx, ny, flux=0.2)
    N = nx * ny
    # Gershgorin: every eigenvalue within the largest row sum of |off-diagonals| of some diagonal entry
    d = H.diagonal().real
    radius = np.asarray(abs(H).sum(axis=1)).ravel() - np.abs(H.diagonal())
    lo, hi = float(np.min(d - radius)), float(np.max(d + radius))
    Delta, E_min, dt = 1.05 * (hi - lo), lo - 0.025 * (hi - lo), 0.7
    states = pc.panel_states(N, batch)
    saved = {k: ctx.tuning_get(k) for k in KNOBS + ("walk_min_blocks", "lattice_fill")}
    spmm = {k: saved[k] for k in KNOBS}
    outs = {}
    try:
        ctx.tuning_set("walk_min_blocks", 64)
        for fill in (1, 0):
            ctx.tuning_set("lattice_fill", fill)
            Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)])
            assert (Op.fill_info() > 0) == (fill == 1), (fill, Op.fill_info())
            rp, col, val = Op.get_csr()
            assert rp[-1] == H.nnz + Op.fill_info() and abs(synth.to_scipy(rp, col, val, N) - H).max() == 0.0
            wrk = L.ChebyWrk(ctx, N * batch, Delta, E_min, dt)
            res = {}
            for name, knobs in (("tiles", dict(spmm_rows=1, spmm_rw=-1)), ("rows", dict(spmm_rows=1, spmm_rw=0)), ("tiled", dict(spmm_rows=0))):
                res[name] = _panel_step(ctx, Op, states, (dt, -dt, dt), wrk, **{**spmm, **knobs})
                if name == "tiles":
                    ti = Op.spmm_tiles(batch)
                    print(f"grid fill={fill} b={batch}: format {Op.format}, {Op.fill_info()} zeros added, tiles {ti}")
                    if ti["taken"]:
                        assert ti["tiles"] * 16 + ti["rest_rows"] == N and ti["rest_rows"] > 0, ti
            assert np.array_equal(res["tiles"], res["tiled"]) and np.array_equal(res["rows"], res["tiled"]), fill
            outs[fill] = res["tiled"]
            wrk.close()
            Op.close()
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
    key = ("grid", Delta, E_min)
    if key not in _oracle:
        _oracle[key] = pc.oracle_steps(H, pc.panel_states(N, 70), L.cheby_coeffs(Delta, dt), Delta, E_min, (dt, -dt, dt))
    for fill in (1, 0):
        _check_oracle(outs[fill], _oracle[key], f"open grid fill={fill} b={batch}")
    assert np.max(np.linalg.norm(outs[1] - outs[0], axis=0)) < 1e-12


# ---------------------------------------------------------------- f. seeded sweep

def test_panel_kernels_random_operators_bit_identical(ctx):
    """Seeded sweep (24 trials): random Hermitian sparse operators (N in [65, 1500], no multiple of 8; 0.5 to 90 entries per row on
    average, Poisson-distributed lengths, empty rows included), a random device format, panel width and knob setting: the bits of the
    state-tiled kernel without nontemporal streams, and every state within 1e-10 of the oracle."""
    rng = np.random.default_rng(20240607)
    saved = {k: ctx.tuning_get(k) for k in KNOBS}
    mean_lens = rng.permutation(np.geomspace(0.5, 90.0, 24))        # every decade of the range, in a seeded order
    try:
        for trial in range(24):
            N = int(rng.integers(65, 1501))
            N += (N % 8 == 0)
            mean_len = min(float(mean_lens[trial]), 0.4 * N)
            batch = int(rng.choice([2, 7, 8, 12, 32, 33, 40, 64, 100]))
            fmt = str(rng.choice(list(FORMATS)))
            knobs = dict(spmm_rows=int(rng.integers(0, 2)), spmm_rw=int(rng.choice([-1, 0, 1, 2, 4, 8])),
                         spmm_strip=int(rng.choice([-1, 0, 32])), spmm_nt=int(rng.integers(0, 3)))
            H = synth.sparse_random(N, mean_len / (2.0 * N), rho=2.0, hermitian=True, rng=rng)
            what = dict(trial=trial, N=N, nnz=int(H.nnz), longest_row=int(np.diff(H.indptr).max()), batch=batch, fmt=fmt, **knobs)
            assert H.nnz > 0 and abs(H - H.getH()).max() == 0.0, str(what)
            ev = np.linalg.eigvalsh(H.toarray())
            span = float(ev[-1] - ev[0])
            assert span > 0, str(what)
            Delta, E_min = 1.05 * span, float(ev[0]) - 0.025 * span
            dt = 2.0 * float(rng.uniform(2.0, 8.0)) / Delta               # Delta dt / 2 in [2, 8]: 17 to 29 terms
            Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)], 0, FORMATS[fmt])
            _assert_csr_round_trip(Op, H)
            states = pc.panel_states(N, batch)
            wrk = L.ChebyWrk(ctx, N * batch, Delta, E_min, dt)
            ref = _panel_step(ctx, Op, states, (dt, -dt), wrk, **{**saved, "spmm_rows": 0, "spmm_nt": 0})
            got = _panel_step(ctx, Op, states, (dt, -dt), wrk, **{**saved, **knobs})
            assert np.array_equal(got, ref), f"{what}: off by up to {np.max(np.abs(got - ref)):.3e}"
            one = _panel_step(ctx, Op, states, (dt,), wrk, **{**saved, **knobs})
            orc = pc.oracle_steps(H, states, wrk.coeffs, Delta, E_min, (dt,))
            _check_oracle(one, orc, f"sweep {what} terms={wrk.n_coeffs}")
            assert np.max(np.linalg.norm(got - states, axis=0)) < TOL, str(what)      # forward + backward = identity
            wrk.close()
            Op.close()
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)
