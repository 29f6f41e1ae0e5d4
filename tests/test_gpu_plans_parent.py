"""The plans an operator gets -- device format, lattice completion, strip-walk plans with their reason, column-blocked mirror, the
batched path's row order and LDS tiles -- are what they were before the planners became a pure-host unit of their own
(csrc/operator_plans.cpp, uploaded by csrc/engine_plans.hip): every number the C ABI's getters report for eight named operators,
recorded on the MI355X from the build of the commit before, in tests/golden/plans_parent.json (written by
tests/golden/make_plans_parent.py, which imports the operators and the record from this file; nothing here writes the fixture).
The CPU harness (tests/sanitize_host_index.cpp with tests/operator_plan_cases.h) pins the same plans array by array on a stand-in
device; this file holds them on the real one, whose CU count the column-blocked mirror's gate reads.

One panel comparison runs the uploaded tile table on the device: a 64-state batched Chebyshev step on the 64 x 64 periodic grid
through the LDS tiles, bit for bit against the row kernel (spmm_rw = 0) and against the parent's digest."""
import contextlib
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qprop_amd.lib as L  # noqa: E402
import qprop_amd.synth as synth  # noqa: E402
from exact_inputs import digest  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(ROOT, "tests", "golden", "plans_parent.json")


def _lattice(n, offsets):
    rp, col, vals = synth.hermitian_offsets_csr(n, offsets=offsets, rho=6.0)
    return synth.to_scipy(rp, col, vals, n)


def _spin_chain():
    rp, col, vals = synth.tfim_csr(12)
    return synth.to_scipy(rp, col, vals, 1 << 12)


def _random_columns():
    rp, col, vals = synth.random_columns_csr(4096, n_pairs=8)
    return synth.to_scipy(rp, col, vals, 4096)


# name -> (generator, requested format, knobs during the build); the smallest sizes that still reach each plan
OPERATORS = {
    "chain-of-blocks-2048": (lambda: _lattice(2048, (1, 64)), L.FMT_AUTO, {"walk_min_blocks": 8}),
    "lattice-4-4-g1024": (lambda: _lattice(1 << 15, (1, 2, 3, 4, 1024, 2048, 3072, 4096)), L.FMT_AUTO, {"walk_min_blocks": 8}),
    "grid-64x64-periodic": (lambda: _lattice(4096, (1, 64)), L.FMT_AUTO, {"walk_min_blocks": 8}),
    "grid-256x16-periodic": (lambda: _lattice(4096, (1, 256)), L.FMT_AUTO, {"walk_min_blocks": 8}),
    "grid-96x64-open-completed": (lambda: synth.grid_hamiltonian_2d(96, 64), L.FMT_AUTO, {"walk_min_blocks": 8}),
    "random-columns-forced-mirror": (_random_columns, L.FMT_RBCSR, {"colblock": 2, "cb_log2w": 6}),
    "spin-chain-12": (_spin_chain, L.FMT_AUTO, {}),
    "long-pair-16384-walkable": (lambda: _lattice(1 << 16, (1, 64, 16384)), L.FMT_AUTO, {"walk_min_blocks": 8}),
}


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


def plan_record(ctx, name):
    """everything the getters say about the plans of operator `name` (JSON types only)"""
    make, fmt, kn = OPERATORS[name]
    H = make()
    with knobs(ctx, **kn):
        Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)], 0, fmt)
        code, _, text = Op.walk_reason()
        rec = {"format": int(Op.format), "lattice_fill": int(Op.fill_info()), "walk": Op.walk_info(), "walk2": Op.walk2_info(),
               "walk_reason": [int(code), text], "colblock": Op.colblock_info(), "spmm_walk": {}, "spmm_tiles": {}}
        with knobs(ctx, walk_pair=1):      # (walk2_info reports the plan only where a step would take it: forced)
            rec["walk2_forced"] = Op.walk2_info()
        rec["colblock"]["own_line_share"] = float(rec["colblock"]["own_line_share"]).hex()
        for strip in (0, 8):
            with knobs(ctx, spmm_strip=strip):
                for b in (8, 64):
                    rec["spmm_walk"][f"strip{strip}-b{b}"] = list(Op.spmm_walk(b))
                rec["spmm_tiles"][f"strip{strip}"] = Op.spmm_tiles(64)
        Op.close()
    return json.loads(json.dumps(rec))


@functools.lru_cache(maxsize=None)
def _panel(n, b):
    return np.stack([synth.random_state(n, seed=300 + s) for s in range(b)], axis=1)


def panel_step(ctx):
    """a 64-state batched Chebyshev step on the 64 x 64 periodic grid: digests through the LDS tiles and through the row kernel"""
    n, b, dt = 4096, 64, 0.6
    H = OPERATORS["grid-64x64-periodic"][0]()
    out = {}
    Op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, H)])
    for path, rw, taken in (("tiles", -1, 1), ("rows", 0, 0)):
        with knobs(ctx, spmm_rows=1, spmm_rw=rw, spmm_strip=0):
            assert Op.spmm_tiles(b)["taken"] == taken, (path, Op.spmm_tiles(b))
            wrk = L.ChebyWrk(ctx, n * b, 14.0, -7.0, dt)
            psi = L.State(ctx, data=np.ascontiguousarray(_panel(n, b)).reshape(-1))
            L.cheby_batched(psi, Op, dt, wrk, b)
            res = psi.numpy()
            psi.close()
            wrk.close()
        assert np.all(np.isfinite(res.view(np.float64)))
        out[path] = digest(res)
    Op.close()
    return out


@pytest.mark.parametrize("name", list(OPERATORS))
def test_plans_match_parent(ctx, parent, name):
    got, want = plan_record(ctx, name), parent["operators"][name]
    for key in want:
        assert got[key] == want[key], (name, key, got[key], want[key])
    assert set(got) == set(want)


def test_plans_reach_what_they_are_named_for(parent):
    """the fixture itself: every named operator reaches the plan it stands for"""
    ops = parent["operators"]
    assert set(ops) == set(OPERATORS)
    assert ops["chain-of-blocks-2048"]["walk"]["valid"] == 1 and ops["chain-of-blocks-2048"]["walk"]["rows_per_step"] == 64
    assert ops["lattice-4-4-g1024"]["walk"]["valid"] == 1 and ops["lattice-4-4-g1024"]["walk2_forced"]["valid"] == 1
    assert ops["grid-64x64-periodic"]["spmm_tiles"]["strip0"]["taken"] == 1 and ops["grid-64x64-periodic"]["spmm_walk"]["strip8-b64"] == [0, 0]
    assert ops["grid-256x16-periodic"]["spmm_tiles"]["strip0"]["taken"] == 1 and ops["grid-256x16-periodic"]["spmm_walk"]["strip8-b64"] == [256, 8]
    assert ops["grid-96x64-open-completed"]["lattice_fill"] > 0 and ops["grid-96x64-open-completed"]["spmm_tiles"]["strip0"]["rest_rows"] > 0
    assert ops["random-columns-forced-mirror"]["colblock"]["valid"] == 1
    assert ops["spin-chain-12"]["walk"]["valid"] == 0 and ops["spin-chain-12"]["spmm_tiles"]["strip0"]["taken"] == 0
    assert ops["long-pair-16384-walkable"]["format"] == L.FMT_HRB and ops["long-pair-16384-walkable"]["walk"]["long_distance"] == 16384


def test_tile_table_on_the_device_matches_row_kernel_and_parent(ctx, parent):
    got = panel_step(ctx)
    assert got["tiles"] == got["rows"], "the LDS tiles and the row kernel disagree bit for bit"
    assert got["tiles"] == parent["panel_step"]["tiles"]
