"""Irregular operators for the batched panel kernels (csrc/kernels_spmm.hip), shared by tests/test_panel_cases_host.py (no GPU:
the generators' guarantees, the oracle against the exact exponential) and tests/test_gpu_panel_irregular.py (every kernel on the
device).  Every other stored-operator test of the panel path uses a periodic lattice whose rows all have one length; here rows of
every length from 0 to 131 sit next to each other, so the kernels' chunk loops, remainders, empty rows and partly filled
wavefronts all run.  NumPy / SciPy and the oracle only: no HIP, no library.  The
generators cache what they return: callers do not write to it."""
import functools
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import qp_oracle as qo  # noqa: E402
import qprop_amd.synth as synth  # noqa: E402

# every length up to 25 (all remainders after groups of four and eight; one, two and three chunks of the state-tiled kernel's 8 or 16
# entries and the lengths around them), 31 .. 33, and the chunk edges of the wave-per-row kernel (64, 128) with one to three entries
# before and past them
DEFAULT_SIZES = tuple(range(1, 26)) + (31, 32, 33, 63, 64, 65, 66, 67, 127, 128, 129, 131)
DEFAULT_EMPTY = 5
FEW_VALUES = (-0.04, 0.025, 0.05, -0.015)


def _permuted_direct_sum(blocks, n_empty, rng):
    """P (B_1 + B_2 + ... + 0_{n_empty}) P^T as CSR with every entry of every block stored, and the permutation: entry (i, j) of the
    direct sum is entry (perm[i], perm[j]) of the result."""
    N = sum(b.shape[0] for b in blocks) + n_empty
    perm = rng.permutation(N)
    rows, cols, vals = [], [], []
    off = 0
    for b in blocks:
        s = b.shape[0]
        i, j = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
        rows.append(perm[off + i.ravel()])
        cols.append(perm[off + j.ravel()])
        vals.append(np.asarray(b, dtype=np.complex128).ravel())
        off += s
    assert all(np.all(v != 0) for v in vals), "a block with a zero entry: the row would be shorter than its block"
    M = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))
    M.sort_indices()
    return M, perm


def mixed_groups(M, rows=16):
    """(groups of `rows` consecutive rows that hold rows of different lengths, all groups)."""
    lens = np.diff(M.indptr)
    groups = [lens[a:a + rows] for a in range(0, M.shape[0], rows)]
    return sum(1 for g in groups if len(set(g.tolist())) > 1), len(groups)


def _check_ladder(M, sizes, n_empty):
    N = M.shape[0]
    lens = np.diff(M.indptr)
    want = set(sizes) | ({0} if n_empty else set())
    assert set(lens.tolist()) == want, sorted(set(lens.tolist()) ^ want)
    assert all(int(np.sum(lens == s)) == s * sizes.count(s) for s in set(sizes))
    assert N % 8 and N % 16 and N % 32, N
    mixed, groups = mixed_groups(M)
    assert 2 * mixed >= groups, (mixed, groups)
    assert abs(M - M.getH()).max() == 0.0


@functools.lru_cache(maxsize=None)
def ladder(sizes=DEFAULT_SIZES, n_empty=DEFAULT_EMPTY, seed=7):
    """Row-length ladder: the direct sum of dense random complex Hermitian blocks, one per entry of `sizes`, each scaled to a
    spectrum inside [-1, 1], and `n_empty` zero rows / columns, conjugated by a seeded random permutation.  A block of size s gives
    s rows of exactly s entries.  Returns (CSR matrix, blocks, permutation)."""
    sizes = tuple(int(s) for s in sizes)
    rng = np.random.default_rng(seed)
    blocks = []
    for s in sizes:
        X = rng.standard_normal((s, s)) + 1j * rng.standard_normal((s, s))
        B = (X + X.conj().T) / 2
        B = B / (np.max(np.abs(np.linalg.eigvalsh(B))) * (1.0 + 1e-12))
        B = (B + B.conj().T) / 2            # (exactly Hermitian after the scaling, too)
        blocks.append(B)
    M, perm = _permuted_direct_sum(blocks, n_empty, rng)
    _check_ladder(M, sizes, n_empty)
    return M, blocks, perm


@functools.lru_cache(maxsize=None)
def ladder_pair(seed0=7, seed1=8):
    """Two default ladders with different permutations, for lazy sums H0 + c H1: the union pattern has rows of more than 128
    entries (three 64-entry chunks of the wave-per-row kernel) and far more distinct row lengths than either term."""
    M0, M1 = ladder(seed=seed0)[0], ladder(seed=seed1)[0]
    U = (abs(M0) + abs(M1)).tocsr()
    lens = np.diff(U.indptr)
    assert lens.max() > 128 and len(set(lens.tolist())) >= 2 * len(DEFAULT_SIZES), (int(lens.max()), len(set(lens.tolist())))
    assert mixed_groups(U)[0] == mixed_groups(U)[1]
    return M0, M1


@functools.lru_cache(maxsize=None)
def real_few_valued(sizes=DEFAULT_SIZES, n_empty=DEFAULT_EMPTY, seed=11, values=FEW_VALUES):
    """A ladder whose blocks are real symmetric with entries drawn from `values` (at most four non-zero reals): the operator takes
    the real copy of its values and, as plain row blocks, the value dictionary.  Returns (CSR matrix, blocks, permutation); the
    spectrum lies inside [-1, 1] (asserted)."""
    assert 0 < len(values) <= 4 and all(v != 0 for v in values)
    sizes = tuple(int(s) for s in sizes)
    rng = np.random.default_rng(seed)
    blocks = []
    for s in sizes:
        B = np.asarray(values, dtype=np.float64)[rng.integers(0, len(values), (s, s))]
        B = np.triu(B) + np.triu(B, 1).T
        ev = np.linalg.eigvalsh(B)
        assert -1.0 < ev[0] and ev[-1] < 1.0, (s, ev[0], ev[-1])
        blocks.append(B)
    M, perm = _permuted_direct_sum(blocks, n_empty, rng)
    _check_ladder(M, sizes, n_empty)
    assert np.all(M.data.imag == 0) and set(M.data.real.tolist()) <= set(values)
    return M, blocks, perm


def panel_states(N, batch):
    """[N, batch]: state s is synth.random_state(N, seed=5000 + s), so a panel of b states is a prefix of any wider one."""
    return np.stack([synth.random_state(N, seed=5000 + s) for s in range(batch)], axis=1)


def oracle_steps(H, states, coeffs, Delta, E_min, dts):
    """The oracle's cheby! (oracle/qp_oracle.py) state by state with the given coefficients (the GPU work area's, copied in as
    tests/test_gpu_parity.py: _cheby_case does), one step per entry of `dts`.  Returns [N, batch]."""
    out = np.empty_like(states)
    for s in range(states.shape[1]):
        psi = states[:, s].copy()
        wrk = qo.ChebyWrk(psi, Delta, E_min, abs(dts[0]))
        wrk.coeffs, wrk.n_coeffs = np.asarray(coeffs, dtype=np.float64).copy(), len(coeffs)
        for dt in dts:
            qo.cheby(psi, H, dt, wrk)
        out[:, s] = psi
    return out


def exact_ladder_step(blocks, perm, n_empty, states, dt):
    """exp(-i H dt) applied to [N, batch] states for the ladder of `blocks` / `perm`: block by block with scipy.linalg.expm."""
    import scipy.linalg as sla
    out = np.empty_like(states)
    off = 0
    for b in blocks:
        idx = perm[off:off + b.shape[0]]
        out[idx] = sla.expm(-1j * dt * b) @ states[idx]
        off += b.shape[0]
    idx = perm[off:off + n_empty]
    out[idx] = states[idx]
    return out
