"""The fixtures of tests/panel_cases.py without a GPU: the generators keep the edges the device tests rely on (every row length,
mixed 16-row groups, sizes that are no multiple of a tile, empty rows, union rows of three 64-entry chunks), and the oracle is right
on them -- against the exact exponential, block by block for the ladder and dense for the lazy sums -- to 1e-12, two orders below
the 1e-10 that the device tests ask of the kernels."""
import os
import sys

import numpy as np
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import qp_oracle as qo  # noqa: E402
import panel_cases as pc  # noqa: E402

ORACLE_TOL = 1e-12      # measured 6.4e-14 (ladder) and 6.0e-14 (lazy sum, c = 0.5j): the reference's own error with a margin of 15 x


def test_default_ladder_has_every_row_length_and_mixed_groups():
    M, blocks, perm = pc.ladder()               # (asserts its own guarantees)
    N = M.shape[0]
    assert N == 1266 and N % 32 == 18 and N % 8 == 2 and M.nnz == sum(s * s for s in pc.DEFAULT_SIZES) == 96049
    lens = np.diff(M.indptr)
    assert set(lens.tolist()) == {0} | set(pc.DEFAULT_SIZES) and int(np.sum(lens == 0)) == pc.DEFAULT_EMPTY
    mixed, groups = pc.mixed_groups(M)
    assert groups == 80 and mixed >= 75, (mixed, groups)
    # the last wavefront of the wave-per-row kernel is partly filled for every RW > 1, the last workgroup of every kernel is
    assert N % 4 and N % 8 and N % 16 and N % 32
    # rows of every remainder after groups of four, below and beyond one group of eight and one chunk of 8 / 16 / 64 entries
    assert {int(v) % 4 for v in lens} == {0, 1, 2, 3} and {1, 2, 3, 7, 9, 17, 65, 129} <= set(lens.tolist())
    # scattered columns: no row's entries are one run of consecutive columns beyond the shortest blocks
    spans = np.array([M.indices[a:b].max() - M.indices[a:b].min() + 1 for a, b in zip(M.indptr[:-1], M.indptr[1:]) if b - a >= 8])
    assert np.all(spans > 4 * lens[lens >= 8])
    # the permutation maps block k's rows to rows of length sizes[k]
    off = 0
    for b in blocks:
        assert np.all(lens[perm[off:off + b.shape[0]]] == b.shape[0])
        assert np.max(np.abs(np.linalg.eigvalsh(b))) <= 1.0
        off += b.shape[0]


def test_ladder_pair_union_rows_span_three_chunks():
    M0, M1 = pc.ladder_pair()                   # (asserts: union rows beyond 128 entries, many lengths, every group mixed)
    assert M0.shape == M1.shape == (1266, 1266)
    assert abs(M0 - M0.getH()).max() == 0.0 and abs(M1 - M1.getH()).max() == 0.0
    U = (abs(M0) + abs(M1)).tocsr()
    lens = np.diff(U.indptr)
    assert 128 < lens.max() <= 2 * max(pc.DEFAULT_SIZES)
    assert np.any((lens > 64) & (lens <= 128)) and np.any(lens > 128)
    # the permutations differ: the terms do not share a pattern
    assert (abs(M0) > 0).multiply(abs(M1) > 0).nnz < M0.nnz // 4


def test_real_few_valued_ladder():
    M, blocks, perm = pc.real_few_valued()      # (asserts: real, at most four values, ladder guarantees, spectrum inside [-1, 1])
    assert M.shape == (1266, 1266) and len(set(M.data.real.tolist())) <= 4
    assert abs(M - M.T).max() == 0.0


def test_panel_states_are_prefixes():
    a, b = pc.panel_states(1266, 3), pc.panel_states(1266, 9)
    assert np.array_equal(a, b[:, :3])
    assert np.max(np.abs(np.linalg.norm(b, axis=0) - 1.0)) < 1e-14
    assert abs(np.vdot(b[:, 0], b[:, 1])) < 0.2          # different states, not copies


def test_term_counts_of_the_device_cases_are_odd_and_even():
    assert len(qo.cheby_coeffs(2.4, 3.0)) == 20 and len(qo.cheby_coeffs(2.4, 2.5)) == 19 and len(qo.cheby_coeffs(5.0, 1.5)) == 21


def test_oracle_matches_the_exact_exponential_on_the_ladder():
    M, blocks, perm = pc.ladder()
    states = pc.panel_states(M.shape[0], 4)
    coeffs = qo.cheby_coeffs(2.4, 3.0)
    assert len(coeffs) == 20
    got = pc.oracle_steps(M, states, coeffs, 2.4, -1.2, (3.0,))
    want = pc.exact_ladder_step(blocks, perm, pc.DEFAULT_EMPTY, states, 3.0)
    err = np.linalg.norm(got - want, axis=0)
    assert np.all(err < ORACLE_TOL), err
    # the empty rows: the state's elements there only pick up the phase of a zero eigenvalue, i.e. nothing
    empty = perm[-pc.DEFAULT_EMPTY:]
    assert np.max(np.abs(got[empty] - states[empty])) < 1e-14


def test_oracle_matches_the_exact_exponential_on_the_lazy_sums():
    M0, M1 = pc.ladder_pair()
    states = pc.panel_states(M0.shape[0], 2)
    coeffs = qo.cheby_coeffs(5.0, 1.5)
    assert len(coeffs) == 21
    D0, D1 = M0.toarray(), M1.toarray()
    for c in (0.7, -0.3, 0.2j, 0.5j, 1.2):
        H = (M0 + c * M1).tocsr()
        got = pc.oracle_steps(H, states, coeffs, 5.0, -2.5, (1.5,))
        want = sla.expm(-1.5j * (D0 + c * D1)) @ states
        err = np.linalg.norm(got - want, axis=0)
        assert np.all(err < ORACLE_TOL), (c, err)
        if np.imag(c) != 0:
            assert np.all(np.linalg.norm(want, axis=0) > 1.0)   # a complex combination: the step is not unitary
