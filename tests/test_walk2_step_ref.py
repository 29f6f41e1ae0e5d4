"""The checker of the checker of the two-term strip walk (no GPU): the step reference of tests/walk2_step_ref.py agrees with the
oracle and its launch table with the library's schedule; on the lattices of the GPU tests (tests/walk2_cases.py) every mutation of
a pair launch puts a row beyond the derived bound with coefficients of order one -- and, in the LAST pair of a step with true
Chebyshev coefficients, none does: what bit-identity of Psi after a physical step cannot see."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import qp_oracle as qo  # noqa: E402
import cheby_term_cases as cases  # noqa: E402
import walk2_cases as wc  # noqa: E402
import walk2_step_ref as W2  # noqa: E402

# the launches of a step written out by hand ([..]: one pair launch; U<n>: updates the accumulator with n deferred vectors, S: skips it,
# f: the first update, L: the last term)
TABLE = {3: "U0f [S,U1L]", 4: "U0f [S,S] U2L", 5: "S [U1f,S] [S,U2L]", 6: "U0f [S,U1] [S,S] U2L", 7: "U0f [S,S] [U2,S] [S,U2L]",
         8: "S [U1f,S] [S,U2] [S,S] U2L"}
ALL_PAIR_FORMS = {("S", "U1L"), ("S", "S"), ("U1f", "S"), ("S", "U2L"), ("S", "U1"), ("U2", "S"), ("S", "U2")}
MUTATION_LATTICES = ("nn4k4d0-complex", "nn2k2d1-real", "nn1k1d1-complex")


def test_launch_table():
    for nterms, text in TABLE.items():
        assert W2.table_text(W2.launch_table(nterms)) == text, nterms
    for nterms in range(3, 41):
        table = W2.launch_table(nterms)
        assert [f.m for l in table for f in l] == list(range(1, nterms + 1))
        assert len(table[0]) == 1 and (len(table[-1]) == 1) == (nterms % 2 == 0)            # a lone last term or not: nterms mod 2
        assert (table[1][0].name, table[1][1].name.rstrip("L")) == {0: ("S", "U1"), 1: ("S", "S"), 2: ("U1f", "S")}[nterms % 3]
        assert W2.n_pairs(table) == (nterms - 1) // 2
        # without the deferred accumulator every term updates, and no two updating terms share a launch
        assert W2.n_pairs(W2.launch_table(nterms, defer=False)) == 0
    assert W2.n_pairs(W2.launch_table(2)) == 0 and W2.table_text(W2.launch_table(2)) == "S U1fL"
    assert W2.table_text(W2.launch_table(1)) == "U0fL"


def test_coefficient_sets_reach_every_pair_form():
    forms = set()
    for nterms in W2.ORDER_ONE_NTERMS:
        a = W2.order_one_coeffs(nterms)
        assert len(a) == nterms + 1 and np.all(a * 16 == np.round(a * 16)) and a.min() < 0 < a.max()
        forms |= W2.pair_forms(W2.launch_table(nterms))
    assert forms == ALL_PAIR_FORMS
    assert W2.pair_forms(W2.launch_table(8)) | W2.pair_forms(W2.launch_table(9)) == ALL_PAIR_FORMS - {("S", "U1L")}      # test_every_instance
    assert ("U1f", "S") not in W2.pair_forms(W2.launch_table(34)) | W2.pair_forms(W2.launch_table(21)) | W2.pair_forms(W2.launch_table(31))


def test_schedule_agrees_with_the_library():
    """qp_acc_schedule_host (host only: the library loads without a GPU) against the restatement, nterms = 2 .. 40"""
    import qprop_amd.lib as L
    for nterms in range(2, 41):
        a = np.arange(1.0, nterms + 2)
        for f, d in zip(W2.term_forms(nterms), L.acc_schedule(a)):
            assert bool(d.skip) == (not f.update), (nterms, f)
            if f.update:
                assert d.n_defer == f.n_defer and d.a_d1 == (a[f.m - 1] if f.n_defer >= 1 else 0.0) and d.a_d2 == (a[f.m - 2] if f.n_defer == 2 else 0.0)


def test_cases_are_what_they_are_named_for():
    lats = [wc.BUILDERS[n]() for n in wc.BUILDER_NAMES]
    assert len({(l.nn, l.K, l.diag, l.real) for l in lats}) == 64 and max(l.n for l in lats) == 2560
    assert {1, 16} <= {l.dmax for l in lats} and len({l.dmax for l in lats}) >= 8
    assert all(l.g == 64 and l.plan()["strip_steps"] == l.K + 16 for l in lats)
    reached, by_shape = set(), {}
    for geo, shape in wc.GEOMETRY_CASES:
        lat = wc.geometry_lattice(geo, shape)
        assert wc.geometry_property(geo, lat), (geo, shape)
        J, S2 = lat.plan()["strip_steps"], lat.chunks()
        for cut, waves in wc.cuts(lat).items():
            L, nseg = wc.cut_of(waves, J, S2)
            assert wc.cut_property(cut, dict(steps_per_wavefront=L, segments=nseg, chunks_per_strip_step=S2), J), (geo, shape, cut)
            reached.add(cut)
        # (the 12 strip steps of the g = 1024 lattice with K = 4 have no segment length that leaves a shorter last one)
        assert {"one_step_per_wavefront", "whole_run_per_wavefront"} <= set(wc.cuts(lat)) and len(wc.cuts(lat)) >= 3, (geo, shape)
        by_shape.setdefault(shape, set()).update(wc.cuts(lat))
    assert reached == set(wc.CUTS) and all(v == set(wc.CUTS) for v in by_shape.values()), by_shape
    assert {geo for geo, _ in wc.GEOMETRY_CASES} == set(wc.GEOMETRY)


def test_reference_agrees_with_the_oracle():
    """one small lattice, a unit state, true coefficients: the oracle rounds each of its terms in double precision -- 1e-13 in the
    max norm; the reference's own error bound (the derivation with 2^-63) is below 1 % of the double-precision bound"""
    lat = wc.BUILDERS["nn2k2d1-complex"]()
    H = lat.matrix()
    rng = np.random.default_rng(5)
    psi0 = rng.standard_normal(lat.n) + 1j * rng.standard_normal(lat.n)
    psi0 /= np.linalg.norm(psi0)
    for dt in (wc.DT, -wc.DT):
        owrk = qo.ChebyWrk(psi0, wc.DELTA, wc.E_MIN, abs(dt))
        a = np.array(owrk.coeffs[:owrk.n_coeffs], dtype=np.float64)
        want = qo.cheby(psi0.copy(), H, dt, owrk)
        step = W2.step_ref(H, psi0, a, wc.DELTA, wc.E_MIN, dt)
        assert float(np.max(np.abs(step.Psi - want))) < 1e-13
        plain = W2.scalars(wc.DELTA, wc.E_MIN, dt)[2] * sum(W2.LD(a[m]) * step.v[m] for m in range(len(a)))
        assert float(np.max(np.abs(step.Psi - plain))) < 1e-16            # the launch-by-launch accumulator is the plain sum
        S = cases.packed_lengths(H)
        bound, _ = W2.step_bound(H, S, step.v, a, wc.DELTA, wc.E_MIN, dt)
        own, _ = W2.step_bound(H, S, step.v, a, wc.DELTA, wc.E_MIN, dt, eps=W2.EPS_LD)
        assert float(np.max(own / bound)) < 0.01


@pytest.fixture(scope="module")
def lattices():
    out = {}
    for name in MUTATION_LATTICES:
        lat = wc.BUILDERS[name]()
        H = lat.matrix()
        out[name] = (lat, H, cases.packed_lengths(H), lat.psi())
    return out


def _applies(mutation, table, where="all"):
    pairs = [l for l in table if len(l) == 2]
    if where == "last":
        pairs = pairs[-1:]
    return {"a0_on_x_in_U1f": any(l[0].name == "U1f" for l in pairs),
            "swap_deferred_2nd": any(l[1].update and l[1].n_defer >= 1 for l in pairs),
            "z_stored_last": any(l[1].last for l in pairs)}.get(mutation, True)


@pytest.mark.parametrize("name", MUTATION_LATTICES)
@pytest.mark.parametrize("dt", [wc.DT, -wc.DT], ids=["forward", "backward"])
def test_every_mutation_lands_beyond_the_bound(lattices, name, dt):
    """coefficients of order one, nterms = 3 .. 14: wherever a mutation can sit (and each can, in some set), a row beyond the bound"""
    lat, H, S, psi = lattices[name]
    geom = lat.geometry()
    seen = {m: 0 for m in W2.MUTATIONS}
    for nterms in W2.ORDER_ONE_NTERMS:
        a = W2.order_one_coeffs(nterms)
        ref = W2.step_ref(H, psi, a, wc.DELTA, wc.E_MIN, dt)
        bound, _ = W2.step_bound(H, S, ref.v, a, wc.DELTA, wc.E_MIN, dt)
        for mutation in W2.MUTATIONS:
            mut = W2.step_ref(H, psi, a, wc.DELTA, wc.E_MIN, dt, mutation=mutation, geom=geom)
            assert (mut.applied > 0) == _applies(mutation, ref.table), (mutation, nterms)
            if not mut.applied:
                assert np.array_equal(mut.Psi, ref.Psi)
                continue
            seen[mutation] += 1
            ratio = np.abs(mut.Psi - ref.Psi) / bound
            assert float(ratio.max()) > 1.0, (mutation, nterms, float(ratio.max()))
            print(f"[mutation] {name} dt {dt} nterms {nterms} {mutation}: {int((ratio > 1).sum())} rows beyond, max {float(ratio.max()):.3g} x the bound")
    assert all(seen.values()), seen


def _true_coeffs(limit):
    """the oracle's cheby_coeffs (src/cheby.jl:25-39) for the first dt >= DT whose series has an odd number of terms: the last
    launch of the step is then a pair, [S,U2L] or [S,U1L], and every late mutation can sit in it"""
    for k in range(100):
        dt = wc.DT + 0.01 * k
        a = np.array(qo.cheby_coeffs(wc.DELTA, dt, limit), dtype=np.float64)
        if (len(a) - 1) % 2 == 1 and W2.launch_table(len(a) - 1)[-1][1].n_defer >= 1:
            return a, dt
    raise AssertionError(limit)


@pytest.mark.parametrize("name", MUTATION_LATTICES[:2])
def test_late_mutations_hide_behind_true_coefficients(lattices, name):
    """The last pair of a physical step.  True Chebyshev coefficients end at the truncation limit of the series, so a wrong y or z
    there reaches Psi times 1e-12 and less:
      * limit = 1e-12 (the library's default): every late mutation moves Psi by less than 1e-10 of its norm -- below the tolerance
        of every oracle comparison of the two-term walk in the suite.  It is NOT inside the per-row bound (5 to 7e4 times the bound
        on these lattices, printed and not asserted): the last coefficients, 3e-11 .. 5e-13, are still far above 2^-52 -- a row-wise
        check or a bit-for-bit comparison with another kernel sees it, a norm does not;
      * the same series carried to limit = 1e-17, where the last coefficients are below 2^-52: every late mutation is INSIDE the
        bound -- no check of Psi can see the last pair of such a step;
      * coefficients of order one, same numbers of terms: every one of them beyond the bound."""
    lat, H, S, psi = lattices[name]
    geom = lat.geometry()
    for limit in (1e-12, 1e-17):
        true, dt = _true_coeffs(limit)
        nterms = len(true) - 1
        assert nterms >= 15 and abs(true[-1]) < limit and abs(true[-2]) < 100 * limit
        ratios = {}
        for kind, a in (("order-one", W2.order_one_coeffs(nterms)), ("true", true)):
            ref = W2.step_ref(H, psi, a, wc.DELTA, wc.E_MIN, dt)
            bound, _ = W2.step_bound(H, S, ref.v, a, wc.DELTA, wc.E_MIN, dt)
            for mutation in W2.LATE_MUTATIONS:
                mut = W2.step_ref(H, psi, a, wc.DELTA, wc.E_MIN, dt, mutation=mutation, geom=geom, where="last")
                assert mut.applied == 1, mutation
                moved = np.abs(mut.Psi - ref.Psi)
                ratio = ratios[kind, mutation] = float((moved / bound).max())
                norm = float(np.linalg.norm(moved.astype(np.float64)) / np.linalg.norm(ref.Psi.astype(np.complex128)))
                print(f"[late] {name} limit {limit:g} nterms {nterms} {kind} coefficients, {mutation}: max {ratio:.3g} x the bound, "
                      f"{norm:.3g} of the norm")
                if kind == "order-one":
                    assert ratio > 1.0, (mutation, ratio)
                elif limit == 1e-12:
                    assert norm < 1e-10, (mutation, ratio, norm)
                else:
                    assert ratio <= 1.0, (mutation, ratio)
