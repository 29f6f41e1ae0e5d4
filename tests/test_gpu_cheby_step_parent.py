"""A cheby! step issues the launches it issued before its term rotation, its split partition and its small gates became the
pure-host unit csrc/cheby_plan.{h,cpp}: per case the digest of the state after cheby!(dt), cheby!(-dt), cheby!(dt), what ONE more
step adds to the context's counters (launches, mat-vecs, steps, graph launches, bytes), and for the splits the numbers of
qp_split_info / qp_split_walk_info -- recorded on the MI355X from the build of the commit before, in
tests/golden/cheby_step_parent.json (written by tests/golden/make_cheby_step_parent.py, which imports the cases and the records
from this file; nothing here writes the fixture).  The CPU harness (tests/cheby_plan_host.cpp with tests/cheby_plan_cases.h) pins
the same decisions launch by launch and list by list; this file holds what they add up to on the device.

The smallest shapes that reach each path: the five-point lattice of a 64 x 256 periodic grid as HRB (strip walk, terms in pairs
or not, an odd and an even number of terms, the deferred accumulator on and off, check_normalization, the replayed hipGraph), a
200-row ragged CSR operator (per-row kernel), a 12-spin chain (RBCSR), a 64-state panel on the 64 x 64 periodic grid, qp_propagate
on an operator the small gate takes and on one just past it, the split getters, and the library's row-partitioned step (one rank,
a forced send set) against the Python loop of the same object, serial and overlapped."""
import contextlib
import json
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qprop_amd.lib as L  # noqa: E402
import qprop_amd.synth as synth  # noqa: E402
import cheby_term_cases as cases  # noqa: E402
import small_instances as si  # noqa: E402
import split_term_cases as sc  # noqa: E402
from exact_inputs import digest  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(ROOT, "tests", "golden", "cheby_step_parent.json")
COUNTERS = ("n_kernel_launches", "n_matvec", "n_cheby_steps", "n_graph_launches", "spmv_bytes")
WALK = {"hrb_walk": 1, "walk_min_blocks": 16, "walk_nt": -1, "walk_waves": 0, "small_nnz": 0, "cheby_graph": 0}


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


def _counters(ctx):
    s = ctx.stats()
    return {k: (float(s[k]).hex() if k == "spmv_bytes" else int(s[k])) for k in COUNTERS}


def _three_steps(ctx, step, psi):
    """digest after step(dt), step(-dt), step(dt); the counters of one more step(dt)"""
    for sign in (1, -1, 1):
        step(sign)
    out = psi.numpy()
    assert np.all(np.isfinite(out.view(np.float64)))
    ctx.reset_stats()
    step(1)
    ctx.sync()
    return {"digest": digest(out), "one_step": _counters(ctx)}


def _five_point():
    return cases.lattice(1 << 14, (1, 64), diag=True)


def lattice_step(ctx, walk_pair, dt, defer, check=False, graph=False):
    """the five-point lattice (N = 2^14, HRB, walk_min_blocks 16): 35 / 22 coefficients at Delta = 24 for dt = 1 / 0.35"""
    N = 1 << 14
    with knobs(ctx, **WALK, walk_pair=walk_pair, acc_defer=defer):
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, _five_point())], 0, L.FMT_HRB)
        assert Op.walk_info()["valid"] == 1 and Op.walk2_info()["valid"] == (1 if walk_pair == 1 else 0)
        wrk = L.ChebyWrk(ctx, N, 24.0, -12.0, dt)
        psi = L.State(ctx, data=synth.random_state(N))
        with knobs(ctx, cheby_graph=(1 << 20) if graph else 0):
            if graph:      # three identical calls: the first arms the key, the second records, the third replays
                ctx.reset_stats()
                for _ in range(3):
                    L.cheby(psi, Op, dt, wrk)
                assert ctx.stats()["n_graph_launches"] == 2
            rec = _three_steps(ctx, lambda s: L.cheby(psi, Op, s * dt, wrk, check_normalization=check), psi)
        rec["n_coeffs"] = int(wrk.n_coeffs)
        for h in (psi, wrk, Op):
            h.close()
    return rec


def operator_step(ctx, H, fmt, Delta, E_min, dt, **kn):
    n = H.shape[0]
    with knobs(ctx, small_nnz=0, cheby_graph=0, **kn):
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)], 0, fmt)
        wrk = L.ChebyWrk(ctx, n, Delta, E_min, dt)
        psi = L.State(ctx, data=synth.random_state(n, seed=11))
        rec = _three_steps(ctx, lambda s: L.cheby(psi, Op, s * dt, wrk), psi)
        rec["format"] = int(Op.format)
        for h in (psi, wrk, Op):
            h.close()
    return rec


def panel_step(ctx):
    n, b, dt = 4096, 64, 0.6
    rp, col, vals = synth.hermitian_offsets_csr(n, offsets=(1, 64), rho=6.0)
    with knobs(ctx, spmm_rows=1, spmm_rw=-1, spmm_strip=0):
        Op = L.Operator(ctx, [L.Matrix(ctx, n, n, rp, col, vals)])
        wrk = L.ChebyWrk(ctx, n * b, 14.0, -7.0, dt)
        panel = np.stack([synth.random_state(n, seed=300 + s) for s in range(b)], axis=1)
        psi = L.State(ctx, data=np.ascontiguousarray(panel).reshape(-1))
        rec = _three_steps(ctx, lambda s: L.cheby_batched(psi, Op, s * dt, wrk, b), psi)
        for h in (psi, wrk, Op):
            h.close()
    return rec


def propagate_grid(ctx, name):
    """qp_propagate, method 0, four steps with every state stored: an operator the small gate takes (e4r4-band3, 1025 rows of 3)
    and one just past it (e8r4-band5, 5 per row: beyond 600 rows there is no 32-slot form, the general loop runs)"""
    c = si.BY_NAME[name]
    A = c.build()
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)])
    assert Op.small_plan("cheby") == c.cheby
    wrk = L.ChebyWrk(ctx, c.n, 4.4, -2.2, 0.3)
    psi = L.State(ctx, data=synth.random_state(c.n, seed=5))
    ctx.reset_stats()
    _, states = L.propagate_steps(Op, psi, wrk, np.full(4, 0.3), store_states=True)
    rec = {"digest": digest(states), "final": digest(psi.numpy()), "counters": _counters(ctx), "small": int(c.cheby is not None)}
    for h in (psi, wrk, Op):
        h.close()
    return rec


SPLIT_OPERATORS = {
    "walk-5point-2048": lambda: (cases.lattice(2048, (1, 64), diag=True), dict(cases.KEEP, colblock=0, hrb_walk=1, walk_min_blocks=16, walk_pair=0)),
    "walk-5point-4096": lambda: (cases.lattice(4096, (1, 64), diag=True), dict(cases.KEEP, colblock=0, hrb_walk=1, walk_min_blocks=16, walk_pair=0)),
    "hrb-z16-rect": lambda: (cases.case("hrb-z16-rect").A, cases.case("hrb-z16-rect").knobs),
}
SPLIT_SENDS = ("ends", "scattered", "one-interior")


def split_getters(ctx, name):
    A, kn = SPLIT_OPERATORS[name]()
    rec = {}
    with knobs(ctx, **kn):
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, A)], 0, L.FMT_HRB)
        for send_set in SPLIT_SENDS:
            split = L.Split(Op, sc.SEND_SETS[send_set](A.shape[0], cases.G))
            rec[send_set] = {"info": [int(split.n_boundary), int(split.n_interior)], "walk": split.walk_info()}
            split.close()
        Op.close()
    return rec


STEP_CASES = {f"lattice-pair{p}-dt{dt}-defer{d}": (lambda ctx, p=p, dt=dt, d=d: lattice_step(ctx, p, dt, d))
              for p in (0, 1) for dt in (1.0, 0.35) for d in (1, 0)}
STEP_CASES["lattice-pair1-dt1.0-defer1-check"] = lambda ctx: lattice_step(ctx, 1, 1.0, 1, check=True)
STEP_CASES["lattice-graph"] = lambda ctx: lattice_step(ctx, -1, 1.0, 1, graph=True)
STEP_CASES["csr-ragged-200"] = lambda ctx: operator_step(ctx, si.ragged(200, 9, 77), L.FMT_CSR, 4.4, -2.2, 0.7, colblock=0)
STEP_CASES["spin-chain-12"] = lambda ctx: operator_step(ctx, synth.to_scipy(*synth.tfim_csr(12), 1 << 12), L.FMT_RBCSR, 55.0, -27.5, 0.1)
STEP_CASES["panel-64-states"] = panel_step
STEP_CASES["propagate-small"] = lambda ctx: propagate_grid(ctx, "e4r4-band3")
STEP_CASES["propagate-past-the-gate"] = lambda ctx: propagate_grid(ctx, "e8r4-band5")
for _name in SPLIT_OPERATORS:
    STEP_CASES[f"split-{_name}"] = lambda ctx, n=_name: split_getters(ctx, n)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)       # (a stream of its own: the capture path requires one)
    yield c
    c.close()


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_step_matches_parent(ctx, parent, name):
    got, want = json.loads(json.dumps(STEP_CASES[name](ctx))), parent[name]
    print(name, got)
    assert got == want, (name, got, want)


def test_fixture_reaches_what_it_is_named_for(parent):
    """the fixture itself: 35 and 22 coefficients (34 and 21 terms: an even and an odd number), the same bits with terms in pairs / without the deferred accumulator /
    with the check's extra launches / replayed, the gate separates the two grids, the splits walk or not"""
    assert set(parent) == set(STEP_CASES)
    for dt, n_coeffs in ((1.0, 35), (0.35, 22)):
        base = parent[f"lattice-pair0-dt{dt}-defer1"]
        assert base["n_coeffs"] == n_coeffs and base["one_step"]["n_matvec"] == n_coeffs - 1
        for other in (f"lattice-pair1-dt{dt}-defer1", f"lattice-pair0-dt{dt}-defer0", f"lattice-pair1-dt{dt}-defer0"):
            assert parent[other]["digest"] == base["digest"] and parent[other]["one_step"] == base["one_step"], other
    check = parent["lattice-pair1-dt1.0-defer1-check"]
    assert check["digest"] == parent["lattice-pair0-dt1.0-defer1"]["digest"]
    assert check["one_step"]["n_kernel_launches"] == 34 + 33 and check["one_step"]["n_matvec"] == 34      # a reduction behind terms 2 .. 34
    assert parent["lattice-graph"]["one_step"]["n_graph_launches"] == 1 and parent["lattice-graph"]["one_step"]["n_matvec"] == 34
    assert parent["csr-ragged-200"]["format"] == L.FMT_CSR and parent["spin-chain-12"]["format"] == L.FMT_RBCSR
    assert parent["propagate-small"]["small"] == 1 and parent["propagate-small"]["counters"]["n_matvec"] == 0
    assert parent["propagate-past-the-gate"]["small"] == 0 and parent["propagate-past-the-gate"]["counters"]["n_matvec"] == 4 * 11
    for name, blocks in (("walk-5point-2048", 32), ("walk-5point-4096", 64)):
        ends = parent[f"split-{name}"]["ends"]
        assert ends["info"] == [2, blocks - 2] and ends["walk"] == dict(valid=1, first_block=3, end_block=blocks - 3, edge_blocks=4)
        assert parent[f"split-{name}"]["scattered"]["walk"]["valid"] == 0 and parent[f"split-{name}"]["one-interior"]["info"] == [blocks - 1, 1]
    assert all(v["walk"]["valid"] == 0 for v in parent["split-hrb-z16-rect"].values())


# ---- the library's row-partitioned step against the Python loop of the same object ------------------------------------------------

@pytest.fixture(scope="module")
def pg():
    import torch
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    yield dist
    dist.destroy_process_group()


@pytest.mark.parametrize("defer", [1, 0])
@pytest.mark.parametrize("overlap", [False, True], ids=["serial", "overlapped"])
def test_native_sharded_step_equals_python_loop(pg, overlap, defer):
    """qp_sharded_cheby_step draws its terms from the same sequence as the single-GPU step; the Python loop of sharded.py states
    the rotation on its own.  One rank, the first and last 200 rows forced into the send set, odd and even numbers
    of terms, both time directions: state, ghost slots and mat-vec count equal, bit for bit."""
    import torch
    import qprop_amd.sharded as sharded
    N = 8192
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4, 16, 32, 48, 64))
    ctx = L.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    ctx.tuning_set("acc_defer", defer)
    send = np.concatenate([np.arange(0, 200), np.arange(N - 200, N)])
    psi0 = synth.random_state(N)
    parities = set()
    for dt in (1.0, 0.2):
        sh = sharded.ShardedCheby(ctx, rp, col, vals, N, 0, N, 20.0, -10.0, dt, exchange="halo", overlap=overlap, native=True,
                                  _debug_send_rows=send)
        assert sh.native is not None and (sh.split is not None) == overlap
        nterms = len(sh.coeffs) - 1
        parities.add(nterms % 2)
        results = []
        for native in (True, False):
            sh.set_state(psi0)
            ctx.reset_stats()
            sh.step(native=native)
            sh.step(backward=True, native=native)
            sh.step(native=native)
            torch.cuda.synchronize()
            sh.check()
            results.append((sh.local_state(), sh.be.read(sh.X[0], N, sh.ncols_local), ctx.stats()["n_matvec"]))
        assert np.array_equal(results[0][0], results[1][0]), (dt, "state")
        assert np.array_equal(results[0][1], results[1][1]), (dt, "ghost slots")
        assert results[0][2] == results[1][2] == 3 * nterms
        sh.close()
    assert parities == {0, 1}
    ctx.close()
