"""The checker of the lazy-sum tests, checked on the host (no GPU): on the very inputs tests/test_gpu_lazy_sum.py uploads
(tests/lazy_sum_cases.py), the exact FMA chain of tests/lazy_sum_ref.py -- what the kernels are expected to return bit for bit --
stays inside the derived bound at every position of every case and move, every mutation of the sum or of the effective
coefficients puts a position beyond it, and the descending-order mutation changes bits (the inputs are not accidentally exact)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lazy_sum_ref as R  # noqa: E402
import lazy_sum_cases as cases  # noqa: E402


def test_fma_exact_is_the_fraction_formula():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        a, b, c = (float(np.ldexp(rng.uniform(-2, 2), int(rng.integers(-40, 41)))) for _ in range(3))
        assert R.fma_exact(a, b, c) == R.fma_fraction(a, b, c)
    # a product that a double cannot hold and that cancels against the addend: one rounding, not two
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    assert R.fma_exact(a, b, -1.0) == -2.0 ** -60 and a * b - 1.0 == 0.0
    assert R.fma_exact(0.0, 3.0, 1.5) == 1.5 and R.fma_exact(2.0, 0.0, -1.5) == -1.5


def test_exact_products_rule():
    assert R.product_is_exact(1.0, [0.3 + 0.2j]) and R.product_is_exact(-2.0, [0.3]) and R.product_is_exact(0.5, [])
    assert not R.product_is_exact(0.5, [0.3 + 0.2j]) and not R.product_is_exact(0.75 - 1.25j, [0.3]) and not R.product_is_exact(3.0, [0.3])


def test_effective_coefficients():
    eff = R.effective(4, 2, [2.0, 3.0j], -2.0)
    assert np.array_equal(eff, np.array([-2.0, -2.0, -4.0, -6.0j]))
    assert np.array_equal(R.effective(3, 0, [], 0.5j), np.full(3, 0.5j))


def test_case_table():
    """term counts around the 32 coefficients of a launch, the three splits, two real cases; the structure the docstring promises"""
    assert [cases.BUILDERS[n][0] for n in cases.CASE_NAMES[:7]] == [1, 2, 31, 32, 33, 64, 65]
    c = cases.case("L65")
    assert c.n == 197 and c.rowptr[-1] == c.planes.shape[1] and len(np.unique(c.rows >> 6)) == 4
    offs = np.unique(np.abs(c.col - c.rows))
    assert set(offs) <= set(cases.OFFSETS) and len(offs) == 5
    t0 = c.terms[0]
    assert np.any((np.diff(t0.col) == 0) & (np.diff(cases.term_rows(t0)) == 0)), "term 0 must carry duplicate entries"
    k = np.array([np.log2(np.abs(p[p != 0]).max()) for p in c.planes if np.any(p)])
    assert k.max() - k.min() > 25, "the terms' magnitudes must be spread over many binades"
    s = c.sample()
    assert {0, c.planes.shape[1] - 1} <= set(s) and len(s) >= 64
    assert set(np.unique(c.rows[s] >> 6)) == {0, 1, 2, 3}
    assert all(np.any(c.planes[l, s] != 0) for l in range(c.L) if l != 1)
    kinds = [m[0] for m in c.moves]
    assert kinds == ["c", "c", "c", "s", "s", "s", "c", "s", "s", "c"]
    assert [m[0] for m in cases.case("L33-all-drift").moves] == ["s"] * 5


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_exact_chain_is_inside_the_bound(name):
    """Every position of every move: the reference alone passes its own test.  (On random inputs of this distribution the largest
    err / bound of the chain is about 0.2: profiles/lazy_sum_bounds.txt.)"""
    c = cases.case(name)
    everywhere = np.arange(c.planes.shape[1])
    worst = 0.0
    for label, coeffs, scale in c.states():
        eff = R.effective(c.L, c.ncoeffs, coeffs, scale)
        got = R.chain_exact(c.planes, eff, everywhere)
        v, M, T = R.combined_ref(c.planes, R.effective(c.L, c.ncoeffs, coeffs, scale, extended=True))
        worst = max(worst, R.check_positions(got, v, M, T, f"{name} {label}", quiet=True))
        if c.real and cases.all_real(coeffs, scale):
            assert np.all(got.imag == 0)
    print(f"[lazy sum] {name}: exact chain, max err/bound {worst:.4f}")
    assert worst < 1.0


def _applies(c, mutation):
    if mutation == "second_chunk_first_coefs":      # (all drift: every effective coefficient is the scale, whichever is read)
        return c.L > R.CHUNK and c.ncoeffs >= 1
    if mutation in R.CHUNK_MUTATIONS:
        return c.L > R.CHUNK
    if mutation in ("border_up", "border_down", "conj_coeff"):
        return c.ncoeffs >= 1
    if mutation == "drift_unscaled":
        return c.ncoeffs < c.L
    return True


@pytest.mark.parametrize("mutation", [m for m in R.MUTATIONS if m != "descending_order"])
@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_mutation_lands_beyond_the_bound(name, mutation):
    c = cases.case(name)
    if not _applies(c, mutation):
        return
    caught = 0
    previous = None
    for label, coeffs, scale in c.states():
        v, M, T = R.combined_ref(c.planes, R.effective(c.L, c.ncoeffs, coeffs, scale, extended=True))
        if mutation == "stale_real_copy":
            if previous is not None:
                caught += R.beyond(previous.real + 1j * v.imag, v, M, T).size
            previous = v
            continue
        eff_m = R.effective(c.L, c.ncoeffs, coeffs, scale, extended=True, mutation=mutation if mutation in R.EFF_MUTATIONS else None)
        wrong = R.combined_ref(c.planes, eff_m, mutation=mutation if mutation in R.CHUNK_MUTATIONS else None)[0]
        caught += R.beyond(wrong, v, M, T).size
    assert caught > 0, f"{name}: the bound does not see {mutation}"


@pytest.mark.parametrize("name", [n for n in cases.CASE_NAMES if cases.BUILDERS[n][0] >= 2])
def test_descending_order_changes_bits(name):
    c = cases.case(name)
    s = c.sample()
    label, coeffs, scale = c.states()[0]
    eff = R.effective(c.L, c.ncoeffs, coeffs, scale)
    up, down = R.chain_exact(c.planes, eff, s), R.chain_exact(c.planes, eff, s, descending=True)
    assert np.any(up != down), f"{name}: the sampled positions do not tell the summation order"
