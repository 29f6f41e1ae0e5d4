"""The checker of the checker (no GPU): the term-level reference of tests/cheby_term_ref.py replays a whole cheby! step and agrees
with the oracle, and on the inputs of every GPU case (tests/cheby_term_cases.py) each mutation of the formula puts at least one
row beyond the bound the GPU tests use -- the bound is tight enough that they could fail."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import qp_oracle as qo  # noqa: E402
import qprop_amd.lib as L  # noqa: E402
import cheby_term_ref as R  # noqa: E402
import cheby_term_cases as cases  # noqa: E402


def _ragged(n=200, seed=3):
    """Hermitian, rows of 1 to 13 entries, rows 17 and 150 empty"""
    rng = np.random.default_rng(seed)
    B = sp.lil_matrix((n, n), dtype=complex)
    for i in range(n):
        for j in rng.choice(n, int(rng.integers(0, 7)), replace=False):
            B[i, j] = complex(rng.standard_normal(), rng.standard_normal())
    H = sp.csr_matrix(B + B.conj().T)
    H = sp.lil_matrix(H)
    for i in (17, 150):
        H[i, :] = 0
        H[:, i] = 0
    H = sp.csr_matrix(H)
    H.eliminate_zeros()
    H.sort_indices()
    assert np.diff(H.indptr).min() == 0 and np.diff(H.indptr).max() > 8
    return H


@pytest.mark.parametrize("n_coeffs", range(2, 13))
def test_schedule_replayed_through_the_term_reference_is_the_oracle_step(n_coeffs):
    """The terms of a step without pairs (csrc/cheby_plan.cpp: ChebySequence, launched by cheby_step_launches of csrc/engine_cheby.hip) with the schedule of qp_acc_schedule_host, each evaluated by
    term_ref: v_1 = c (H v_0 - beta v_0), c doubled after the first term, v_m = c (H v_{m-1} - beta v_{m-1}) + v_{m-2}; the
    accumulator starts as a_0 v_0 inside the first update and takes the skipped terms' coefficients as a_d1 / a_d2; the phase on the
    last term.  Against oracle.qp_oracle.cheby (src/cheby.jl:171-211) to a few ulps of the unit state norm: 64 ulp = 1.4e-14 (the
    oracle rounds every one of its up to 11 terms in double precision, the replay in extended)."""
    H = _ragged()
    n = H.shape[0]
    rng = np.random.default_rng(n_coeffs)
    psi0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    psi0 /= np.linalg.norm(psi0)
    Delta, E_min = 2.2 * abs(H).sum(axis=1).max(), -1.1 * abs(H).sum(axis=1).max()
    # the longest time step, and the truncation limit with it, whose series has exactly n_coeffs coefficients (a short series of
    # a long step has coefficients of order one throughout: no term of the replay hides behind a tiny coefficient)
    dt = limit = None
    for cand in np.geomspace(8.0, 1e-3, 400) / Delta:
        for lim in (1e-1, 1e-3, 1e-6, 1e-9, 1e-12):
            if dt is None and len(L.cheby_coeffs(Delta, cand, lim)) == n_coeffs:
                dt, limit = float(cand), lim
    assert dt is not None, n_coeffs
    owrk = qo.ChebyWrk(psi0, Delta, E_min, dt, limit=limit)
    a = np.asarray(owrk.coeffs[:owrk.n_coeffs], dtype=np.float64)
    assert len(a) == n_coeffs
    want = qo.cheby(psi0.copy(), H, dt, owrk)
    sched = L.acc_schedule(a)
    beta = Delta / 2 + E_min
    c = -2j / Delta
    phase = np.exp(-1j * beta * dt)
    nterms = n_coeffs - 1
    cur, prev, acc = psi0.astype(R.CLD), None, None
    updated = False
    for m in range(1, nterms + 1):
        d = sched[m - 1]
        t, r, _, _ = R.term_ref(H, cur, 0, prev, acc if updated else None, c, beta, a[0], a[m], phase if m == nterms else 1.0, d)
        if r is not None:
            acc, updated = r, True
        if m == 1:
            c = 2 * c
        prev, cur = cur, t
    assert updated and sum(1 for d in sched if not d.skip) >= 1
    assert np.linalg.norm((acc - want.astype(R.CLD)).astype(complex)) < 64 * 2.0 ** -52


# ---- the mutation table -------------------------------------------------------------------------------------------------------

def _caught(c, form, ref, got):
    """does any output the form produces (vout unless the form has none, acc_out unless it skips) have a row beyond the bound?"""
    t, r, T, Rm = ref
    hit = False
    if form.vout != "none":
        hit |= R.beyond(got[0], t, c.S, T).size > 0
    if r is not None:
        hit |= R.beyond(got[1], r, c.S, Rm).size > 0
    return hit


def _matrix_mutations(c, x, s):
    """{name: mutated row sums}: one stored entry dropped / conjugated / gathered from the neighbouring column, on the row and the
    entry where |a| |x_j| is largest among the rows of the last row block (so it is no entry the power-of-two scales of x hide)"""
    Am = c.A
    n = Am.shape[0]
    rows = np.repeat(np.arange(n), np.diff(Am.indptr))
    xg = np.asarray(x, dtype=R.CLD)[Am.indices]
    w = np.abs(Am.data) * np.abs(xg).astype(float)
    cand = np.nonzero(rows >= (n - 1) // 64 * 64)[0]
    out = {}
    p = int(cand[np.argmax(w[cand])])
    i, a, xj = int(rows[p]), R.CLD(Am.data[p]), xg[p]
    out["entry_dropped"] = s.copy()
    out["entry_dropped"][i] -= a * xj
    out["neighbouring_column"] = s.copy()
    out["neighbouring_column"][i] += a * (R.CLD(x[(int(Am.indices[p]) + 1) % len(x)]) - xj)
    wi = np.abs(Am.data.imag) * np.abs(xg).astype(float)
    if wi[cand].max() > 0:      # (an all-real operator has no entry a conjugation changes)
        q = int(cand[np.argmax(wi[cand])])
        out["entry_conjugated"] = s.copy()
        out["entry_conjugated"][int(rows[q])] += (np.conj(R.CLD(Am.data[q])) - R.CLD(Am.data[q])) * xg[q]
    return out


def _relevant(mutation, form, xoff):
    if form.skip and mutation not in ("xi_without_offset", "v0_before_c"):
        return False
    return {"xi_without_offset": xoff != 0,
            "v0_before_c": form.v0,
            "swap_deferred": form.n_defer >= 1,
            "v0_for_xi_in_defer2": form.n_defer == 2,
            "no_phase": form.phase != 1.0,
            "phase_on_t": form.phase != 1.0,
            "a_prev_with_acc_in": form.acc_in}[mutation]


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_every_mutation_is_beyond_the_bound(name):
    """For every case, row offset and argument form of the GPU tests: the reference itself is (of course) inside its bound, every
    magnitude is positive, and each mutation that the form can show -- a wrong operand, coefficient or phase of the epilogue
    (cheby_term_ref.MUTATIONS), a dropped, conjugated or misplaced matrix entry -- moves at least one row of an output beyond it."""
    c = cases.case(name)
    x, v0, acc = c.vectors()
    assert np.all(x != 0) and np.all(v0 != 0) and np.all(acc != 0)
    sums = c.sums(x)
    mats = _matrix_mutations(c, x, sums[0]) if c.family not in ("pauli", "liouville") else {}
    assert c.family in ("pauli", "liouville") or {"entry_dropped", "neighbouring_column"} <= set(mats)
    seen = set()
    for xoff in c.xoffs:
        for form in cases.FORMS:
            ref = cases.reference(c, x, xoff, v0, acc, form, sums=sums)
            t, r, T, Rm = ref
            assert np.all(T > 0) and (r is None or np.all(Rm > 0))
            assert not _caught(c, form, ref, (t, r))
            # rounding the reference to double precision stays far inside the bound
            assert R.check_rows(t.astype(complex), t, c.S, T, "", quiet=True) < 0.2
            for mutation in R.MUTATIONS:
                if not _relevant(mutation, form, xoff):
                    continue
                got = cases.reference(c, x, xoff, v0, acc, form, sums=sums, mutation=mutation)
                assert _caught(c, form, ref, got), (name, xoff, form.name, mutation)
                seen.add(mutation)
            for mname, s_mut in mats.items():
                got = cases.reference(c, x, xoff, v0, acc, form, sums=(s_mut, sums[1]))
                assert _caught(c, form, ref, got), (name, xoff, form.name, mname)
                seen.add(mname)
    want = set(R.MUTATIONS) | set(mats)
    if len(c.xoffs) == 1:
        want.discard("xi_without_offset")
    assert seen == want, want - seen


def test_forms_cover_the_issue_list():
    f = cases.FORM_BY_NAME
    assert len(cases.FORMS) == 14 and sorted({n.split("-")[0] for n in f}) == [str(k) for k in range(1, 10)]
    assert not f["1-first"].v0 and not f["1-first"].acc_in and f["1-first"].vout == "new" and f["1-first"].phase == 1.0
    assert f["3-middle-out-of-place"].vout == "new" and f["3-middle-out-of-place"].acc_out == "new"
    assert f["6-skip"].skip and f["6-skip"].acc_out == "none" and f["6-skip-acc-given"].skip and f["6-skip-acc-given"].acc_out == "new"
    assert f["8-defer2-no-acc"].n_defer == 2 and not f["8-defer2-no-acc"].acc_in
    assert f["7-defer1-acc-no-v0"].n_defer == 1 and not f["7-defer1-acc-no-v0"].v0 and f["7-defer1-acc-no-v0"].acc_in
    assert abs(abs(cases.PH_UNIT) - 1) < 1e-15 and abs(abs(cases.PH_NONUNIT) - 1) > 0.2
    for T in (2, 4, 8, 16, 32, 64):
        for kind in ("complex", "real"):
            assert f"csr-T{T}-{kind}" in cases.BUILDERS and f"csr-T{T}-{kind}-rect" in cases.BUILDERS
