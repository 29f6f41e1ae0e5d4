"""The two-term strip walk (csrc/kernels_walk2_impl.h, launched in pairs by cheby_step_launches of csrc/engine_cheby.hip) on every
kernel instance, every form a pair's two epilogues can take, every geometry of chunk, strip step and last block, and every cut of
the walk -- each step checked three ways:

    launches   the context's counters (reset before the step) show exactly the pairs of the launch table restated in
               tests/walk2_step_ref.py: n_pair_launches pairs, n_matvec = nterms, one kernel launch per one-term launch and two per
               pair (the walk, and the follow-up of the edge blocks' second term).  A pair the launcher refuses is not counted: it
               fails the test instead of passing as one-term launches;
    bits       Psi is bit-identical to the one-term strip walk (walk_pair = 0) and to the per-block kernel (hrb_walk = 0);
    rows       every row of Psi is within the derived bound of the extended-precision reference of the whole step
               (walk2_step_ref.step_ref / step_bound: nothing in the bound is measured).

The steps use coefficients of order one (walk2_step_ref.order_one_coeffs) written into the workspace, so that every term -- the
last pair included -- moves Psi by order one; tests/test_walk2_step_ref.py shows on these lattices that each plausible mistake of
a pair launch then lands beyond the bound.  Lattices, geometry cases and cuts: tests/walk2_cases.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qprop_amd.lib as L  # noqa: E402
import cheby_term_cases as cases  # noqa: E402
import walk2_cases as wc  # noqa: E402
import walk2_step_ref as W2  # noqa: E402
from cheby_term_cases import same_bits  # noqa: E402
from test_gpu_cheby_term import Guarded  # noqa: E402
from test_gpu_rowblock_bits import knobs  # noqa: E402

pytestmark = pytest.mark.gpu
PAIR = dict(wc.KNOBS, walk_waves=0, walk_nt=-1)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


class Rig:
    """one lattice on the device: operator, workspace, a guarded Psi, and the host references of the steps run on it"""

    def __init__(self, ctx, lat):
        self.ctx, self.lat = ctx, lat
        self.H = lat.matrix()
        self.S = cases.packed_lengths(self.H)
        self.psi0 = lat.psi()
        self.op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, self.H)], 0, L.FMT_HRB)
        self.wrk = L.ChebyWrk(ctx, lat.n, wc.DELTA, wc.E_MIN, wc.DT)
        self.psi = Guarded(ctx, lat.n)
        self.refs, self.base = {}, {}

    def close(self):
        for h in (self.psi, self.wrk, self.op):
            h.close()

    def reference(self, a, dt):
        key = (len(a), dt)
        if key not in self.refs:
            step = W2.step_ref(self.H, self.psi0, a, wc.DELTA, wc.E_MIN, dt)
            self.refs[key] = (step.Psi, W2.step_bound(self.H, self.S, step.v, a, wc.DELTA, wc.E_MIN, dt)[0])
        return self.refs[key]

    def step(self, a, dt, what, wrk=None, op=None, **kn):
        """one cheby!(psi0, dt) with the coefficients ``a`` under the knobs ``kn``: (Psi, the step's counters).  Psi lives inside
        guard zones: its buffer is one of the four vectors a step in pairs rotates, and has length N exactly."""
        wrk = self.wrk if wrk is None else wrk
        wrk.coeffs = np.ascontiguousarray(a, dtype=np.float64)
        wrk.n_coeffs = len(a)
        with knobs(self.ctx, **kn):
            self.psi.load(self.psi0)
            self.ctx.reset_stats()
            L.cheby(self.psi.view, self.op if op is None else op, dt, wrk)
            stats = self.ctx.stats()
            return self.psi.read(what), stats

    def check(self, a, dt, what, wrk=None, **kn):
        """a step in pairs under ``kn``: the launches of the table, the bits of the one-term paths, every row under the bound"""
        nterms = len(a) - 1
        table = W2.launch_table(nterms)
        got, stats = self.step(a, dt, what, wrk=wrk, **{**PAIR, **kn})
        assert stats["n_pair_launches"] == W2.n_pairs(table) == (nterms - 1) // 2, (what, W2.table_text(table), stats)
        assert stats["n_matvec"] == nterms and stats["n_kernel_launches"] == len(table) + W2.n_pairs(table), (what, stats)
        assert stats["n_cheby_steps"] == 1 and stats["n_graph_launches"] == 0, (what, stats)
        key = (nterms, dt)
        if key not in self.base:
            one, st1 = self.step(a, dt, what + " one-term walk", **{**PAIR, "walk_pair": 0})
            blk, st0 = self.step(a, dt, what + " per-block", **{**PAIR, "hrb_walk": 0})
            for st in (st1, st0):
                assert st["n_pair_launches"] == 0 and st["n_matvec"] == nterms == st["n_kernel_launches"], (what, st)
            assert same_bits(one, blk), f"{what}: the one-term walk and the per-block kernel differ"
            self.base[key] = one
        assert same_bits(got, self.base[key]), (f"{what}: not the bits of the one-term launches, "
                                                f"first row {int(np.nonzero(got != self.base[key])[0][0])}")
        ref, bound = self.reference(a, dt)
        return W2.check_rows(got, ref, bound, what, quiet=True)


def prove_plan(rig):
    """the plans are the ones the lattice is named for; the pair path is taken"""
    lat, op = rig.lat, rig.op
    plan = lat.plan()
    wi, w2 = op.walk_info(), op.walk2_info()
    assert wi["valid"] == 1 and (wi["near"], wi["far"], wi["diag"]) == lat.shape and wi["rows_per_step"] == lat.g, wi
    assert (wi["first_block"], wi["end_block"]) == plan["one"] and wi["long_distance"] == 0 and wi["far_diagonals"] == 0, (wi, plan)
    assert w2["valid"] == 1 and (w2["first_block"], w2["end_block"]) == plan["two"] and w2["edge_blocks"] == plan["edge2"], (w2, plan)
    assert wi["first_block"] < w2["first_block"] and w2["end_block"] < wi["end_block"]              # edge blocks on both sides
    assert (w2["end_block"] - w2["first_block"]) * 64 >= (2 * lat.K + 4) * lat.g
    assert w2["useful_rows_per_chunk"] == 64 - 2 * lat.dmax and w2["chunks_per_strip_step"] == lat.chunks(), w2
    stored = op.layout_info()["stored"]
    assert op.value_encoding_info()["plane_bytes"] == (8 if lat.real else 16) * stored              # the real copy is what streams
    return w2


# ---- every instance ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", wc.BUILDER_NAMES)
def test_every_instance(ctx, name):
    """NN 1-4 x K 1-4 x diagonal x complex values / real copy, each with temporal and nontemporal value loads (walk_nt 0 / 1):
    the 128 instances of hrb_walk2_kernel.  nterms = 8 and 9: every pair form but [S,U1L]."""
    lat = wc.BUILDERS[name]()
    with knobs(ctx, **PAIR):
        rig = Rig(ctx, lat)
        try:
            worst = 0.0
            for nt in (0, 1):
                with knobs(ctx, walk_nt=nt):
                    prove_plan(rig)
                    # nterms = 8 at the default cut (one strip step per wavefront here), 9 in three segments per strip column
                    for nterms, waves in ((8, 0), (9, 3 * lat.chunks())):
                        worst = max(worst, rig.check(W2.order_one_coeffs(nterms), wc.DT, f"{name} walk_nt {nt} nterms {nterms}", walk_nt=nt,
                                                     walk_waves=waves))
            if lat.real:      # ... and the bits of the same operator streamed as complex values (knob real_vals = 0)
                with knobs(ctx, real_vals=0):
                    opc = L.Operator(ctx, [L.Matrix.from_scipy(ctx, rig.H)], 0, L.FMT_HRB)
                    assert opc.value_encoding_info()["plane_bytes"] == 16 * opc.layout_info()["stored"] and opc.walk2_info()["valid"] == 1
                    a = W2.order_one_coeffs(9)
                    got, stats = rig.step(a, wc.DT, name + " complex copy", op=opc, **PAIR)
                    assert stats["n_pair_launches"] == 4 and same_bits(got, rig.base[9, wc.DT])
                    opc.close()
            print(f"[walk2 rows] test_every_instance {name} dmax {lat.dmax} N {lat.n}: max err/bound {worst:.5f}")
        finally:
            rig.close()


# ---- every pair form ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", wc.PAIR_FORM_LATTICES)
def test_every_pair_form(ctx, name):
    """nterms = 3 .. 14, both time directions: [S,U1L] (the only pair, its z not stored), [U1f,S] (the first update inside a pair),
    [S,U1], [S,U2], [U2,S], [S,S], [S,U2L].  Then ONE workspace through nterms = 5, 3, 8: the four-vector rotation of a step leaves
    nothing behind for the next."""
    lat = wc.BUILDERS[name]()
    with knobs(ctx, **PAIR):
        rig = Rig(ctx, lat)
        try:
            prove_plan(rig)
            seen, worst = set(), {}
            for nterms in W2.ORDER_ONE_NTERMS:
                a = W2.order_one_coeffs(nterms)
                table = W2.launch_table(nterms)
                for dt in (wc.DT, -wc.DT):
                    r = rig.check(a, dt, f"{name} nterms {nterms} dt {dt} {W2.table_text(table)}")
                    for form in W2.pair_forms(table):
                        worst[form] = max(worst.get(form, 0.0), r)
                seen |= W2.pair_forms(table)
            assert seen == {("S", "U1L"), ("S", "S"), ("U1f", "S"), ("S", "U2L"), ("S", "U1"), ("U2", "S"), ("S", "U2")}
            for form, r in sorted(worst.items()):
                print(f"[walk2 rows] test_every_pair_form {name} [{form[0]},{form[1]}]: max err/bound {r:.5f}")
            wrk = L.ChebyWrk(ctx, lat.n, wc.DELTA, wc.E_MIN, wc.DT)
            for nterms in (5, 3, 8):
                rig.check(W2.order_one_coeffs(nterms), wc.DT, f"{name} reused workspace nterms {nterms}", wrk=wrk)
            wrk.close()
        finally:
            rig.close()


# ---- geometry and cuts -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geo,shape", wc.GEOMETRY_CASES, ids=[f"{g}/{s}" for g, s in wc.GEOMETRY_CASES])
def test_geometry_and_cuts(ctx, geo, shape):
    """Chunks that tile the strip step exactly or leave a partly owned last chunk, d_max = 1 and 16, a partly filled last row
    block, a last strip step that is not whole, the headline's g = 1024 -- each cut into one step per wavefront, the whole run per
    wavefront, segments with a shorter last one, and a wavefront count that leaves the last workgroup idle lanes; nterms = 7 and 8.
    Psi sits between sentinel guard zones throughout (Rig.step): no store before or behind its N elements."""
    lat = wc.geometry_lattice(geo, shape)
    assert wc.geometry_property(geo, lat)
    with knobs(ctx, **PAIR):
        rig = Rig(ctx, lat)
        try:
            prove_plan(rig)
            J = lat.plan()["strip_steps"]
            worst = {}
            for cut, waves in wc.cuts(lat).items():
                with knobs(ctx, walk_waves=waves):
                    info = rig.op.walk2_info()
                assert info["valid"] == 1 and wc.cut_property(cut, info, J), (cut, waves, info)
                for nterms in (7, 8):
                    worst[cut] = max(worst.get(cut, 0.0), rig.check(W2.order_one_coeffs(nterms), wc.DT, f"{geo}/{shape} {cut} nterms {nterms}",
                                                                    walk_waves=waves))
            print(f"[walk2 rows] test_geometry_and_cuts {geo}/{shape} N {lat.n}: " + ", ".join(f"{c} {r:.5f}" for c, r in worst.items()))
        finally:
            rig.close()


# ---- no deferred accumulator, no pairs ----------------------------------------------------------------------------------------

def test_acc_defer_off_takes_no_pairs(ctx):
    """acc_defer = 0: every term updates the accumulator, and a pair is proposed only when at most one of its two terms does
    (csrc/cheby_plan.h) -- so the step takes one-term launches although the operator's two-term plan is valid.  The documented
    behaviour, pinned: no pair launch, the bits of the one-term walk."""
    lat = wc.BUILDERS["nn2k2d1-complex"]()
    with knobs(ctx, **PAIR):
        rig = Rig(ctx, lat)
        try:
            prove_plan(rig)
            for nterms in (8, 9):
                a = W2.order_one_coeffs(nterms)
                table = W2.launch_table(nterms, defer=False)
                assert W2.n_pairs(table) == 0 and len(table) == nterms
                with knobs(ctx, acc_defer=0):
                    assert rig.op.walk2_info()["valid"] == 1
                got, stats = rig.step(a, wc.DT, f"acc_defer 0 nterms {nterms}", **{**PAIR, "acc_defer": 0})
                assert stats["n_pair_launches"] == 0 and stats["n_matvec"] == nterms == stats["n_kernel_launches"], stats
                one, _ = rig.step(a, wc.DT, f"acc_defer 0 one-term walk nterms {nterms}", **{**PAIR, "acc_defer": 0, "walk_pair": 0})
                assert same_bits(got, one)
                ref, bound = rig.reference(a, wc.DT)
                W2.check_rows(got, ref, bound, f"acc_defer 0 nterms {nterms}", quiet=True)
        finally:
            rig.close()
