"""Pins the extended-precision Pauli reference of the GPU edge tests (tests/pauli_ref.py: tensor-axis flips and per-axis factors)
against the Kronecker-built matrix (synth.pauli_sum_matrix): two constructions that share no code.  Host only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qprop_amd.synth as synth  # noqa: E402
from qprop_amd.lib import pauli_masks  # noqa: E402
import pauli_ref  # noqa: E402
import test_gpu_pauli_edges as E  # noqa: E402  (the case builders; importing opens no device)


def _strings(n, count, rng):
    out = []
    for _ in range(count):
        lab = "".join(rng.choice(list("IXYZ"), size=n, p=[0.4, 0.2, 0.2, 0.2]))
        out.append((complex(rng.uniform(-1, 1), rng.uniform(-1, 1)), pauli_masks(lab)))
    return out


@pytest.mark.parametrize("n", [6, 7, 9])
def test_reference_matches_the_kronecker_matrix(n):
    """30 random I/X/Y/Z strings with complex amplitudes on a normalised state: 1e-15 absolute in the max-norm -- double-precision
    rounding of the Kronecker side's 30-term row sums (amplitudes below 1.5, |x_r| of order 2^(-n/2)); measured 4.5e-16."""
    rng = np.random.default_rng(100 + n)
    strings = _strings(n, 30, rng)
    x = synth.random_state(1 << n, seed=n)
    want = synth.pauli_sum_matrix(n, strings) @ x
    got = pauli_ref.pauli_apply(n, strings, x)
    assert got.dtype == np.clongdouble
    assert np.abs(got - want).max() < 1e-15
    H = pauli_ref.PauliRef(n, strings)
    assert H.shape == (1 << n, 1 << n) and (H @ x).dtype == np.complex128
    assert np.abs(H @ x - want).max() < 1e-15


def test_single_factors_and_bit_order():
    """One factor at a time on a basis-like vector: qubit q is bit q of the row index; Y|0> = i|1>, Y|1> = -i|0>."""
    n = 6
    x = np.arange(1, 65, dtype=np.complex128)
    r = np.arange(64)
    for q in range(n):
        b = 1 << q
        up = (r // b) % 2 == 0                      # rows whose bit q is clear
        partner = np.where(up, r + b, r - b)
        assert np.array_equal(pauli_ref.pauli_apply(n, [(1.0, (b, 0))], x).astype(np.complex128), x[partner])
        assert np.array_equal(pauli_ref.pauli_apply(n, [(1.0, (0, b))], x).astype(np.complex128), np.where(up, x, -x))
        assert np.array_equal(pauli_ref.pauli_apply(n, [(1.0, (b, b))], x).astype(np.complex128), np.where(up, -1j, 1j) * x[partner])


def test_abs_apply_is_the_row_magnitude():
    """A_r = sum |a_t| |x_partner|: what the same strings with |a_t| and their Z factors dropped give on |x|."""
    n = 7
    rng = np.random.default_rng(5)
    strings = _strings(n, 12, rng)
    x = synth.random_state(1 << n, seed=3)
    bare = [(abs(np.clongdouble(a)), (xm, 0)) for a, (xm, _) in strings]
    want = pauli_ref.pauli_apply(n, bare, np.abs(x.astype(np.clongdouble))).real
    got = pauli_ref.pauli_abs_apply(n, strings, x)
    assert np.abs(got - want).max() < 1e-17
    assert np.all(got + 1e-18 >= np.abs(pauli_ref.pauli_apply(n, strings, x)))


def test_cases_have_the_shape_they_were_built_for():
    """The group tables behind the case ids of tests/test_gpu_pauli_edges.py, against the launcher's rules (host only)."""
    for cid in E.MUL_CASES:
        n, strings = E.case_strings(cid)
        assert all(xm < (1 << n) and zm < (1 << n) for _, (xm, zm) in strings)
        groups, ndiag0 = E._shape_of(strings)
        xs = sorted({xm for _, (xm, _) in strings})
        if cid in ("many_groups", "many_groups_diag"):
            assert groups > E.MAX_GROUPS and ndiag0 == (30 if cid == "many_groups_diag" else 0) and len(strings) <= E.MAX_STRINGS + 30
            assert all(isinstance(a, float) for a, _ in strings)
        elif cid == "many_strings":
            assert groups <= E.MAX_GROUPS and len(strings) > E.MAX_STRINGS
        elif cid == "huge_diagonal":
            assert ndiag0 > E.MAX_STRINGS and groups == 13
        else:
            assert groups <= E.MAX_GROUPS and len(strings) <= E.MAX_STRINGS
        if cid.startswith("high_"):
            assert len(xs) == int(cid[5:]) and xs[0] >= 64 and any(xm % 64 == 0 for xm in xs)
            assert len(xs) == 1 or any(xm % 64 for xm in xs)
        if cid == "low_only":
            assert xs[0] == 0 and xs[-1] < 64 and ndiag0 == 8
        if cid in ("field_only", "field_only_complex", "xx_yy_only", "triples", "mixed_sizes", "seam_masks"):
            assert ndiag0 == 0
        if cid in ("single_z", "identity_plus_field"):
            assert ndiag0 == 1
        if cid == "two_blocks":
            assert 64 in xs
    assert E.case_strings("many_groups")[1] == E.case_strings("many_groups_diag")[1][:1100]
