"""The persistent single-workgroup kernels (csrc/kernels_small.hip) as the tests see them: a Python mirror of the plan
(csrc/small_plan.cpp) and of the two gates (csrc/cheby_plan.cpp: cheby_small_gate, csrc/engine_krylov.hip: small_sweep_fits), the
instances `(ent, rows_per_group)` that an operator of at most 2048 rows can reach under the default knobs, and ONE table of the
smallest operators that select each of them -- shared by tests/test_small_plan_host.py (no GPU: mirror against the library, the
table against the reachable set) and tests/test_gpu_small_instances.py (every case on the device).  NumPy / SciPy only."""
import collections

import numpy as np
import scipy.sparse as sp

THREADS = 512          # csrc/small_plan.h: kSmallThreads
SLOTS = 16             # kSmallEpt
SLOTS_WIDE = 32        # kSmallEptArnoldi, and the packed Chebychev form
LDS_ROWS = 2048        # kSmallLdsRows
LDS_BYTES = 152 * 1024  # kSmallLdsBytes
SMALL_NNZ = 8192       # csrc/device.h: Tuning::small_nnz
CHEBY_WIDE_ROWS = 600  # cheby_plan.cpp (cheby_small_gate): the 32-slot Chebychev form keeps 128 KB of values in LDS, which leaves room for 600 rows


def small_plan(n, maxrow, max_slots=SLOTS):
    """(lanes, ent, rows_per_group) or None -- csrc/small_plan.cpp: small_plan."""
    if n < 1 or n > LDS_ROWS:
        return None
    t = 1
    while t <= 64:
        ngrp = THREADS // t
        rows = -(-n // ngrp)
        ent = 1
        while ent * t < maxrow:
            ent *= 2
        rows_p2 = 1
        while rows_p2 < rows:
            rows_p2 *= 2
        if rows_p2 * ent <= max_slots:
            return (t, ent, rows_p2)
        t *= 2
    return None


def cheby_plan(n, nnz, maxrow, nops=1, small_nnz=SMALL_NNZ):
    """What qp_propagate (method 0) takes -- csrc/cheby_plan.cpp: cheby_small_gate."""
    if not (small_nnz > 0 and nnz <= 2 * small_nnz and nops <= 64):
        return None
    plan = small_plan(n, maxrow, SLOTS) if nnz <= small_nnz else None
    if plan is None and n <= CHEBY_WIDE_ROWS:
        plan = small_plan(n, maxrow, SLOTS_WIDE)
    return plan


def arnoldi_fits_lds(n, m):
    """csrc/small_plan.h: small_arnoldi_fits -- m + 1 basis vectors, the work vector and 8 scratch slots of 16 bytes."""
    return 16 * (THREADS // 64 + (m + 2) * n) <= LDS_BYTES


def arnoldi_plan(n, nnz, maxrow, m, small_nnz=SMALL_NNZ):
    """What an Arnoldi sweep of m columns takes -- csrc/engine_krylov.hip: small_sweep_fits."""
    if not (small_nnz > 0 and nnz <= small_nnz * (SLOTS_WIDE // SLOTS) and arnoldi_fits_lds(n, m)):
        return None
    return small_plan(n, maxrow, SLOTS) or small_plan(n, maxrow, SLOTS_WIDE)


def reachable(kind):
    """{(ent, rows_per_group): set of lanes} over every n <= 2049 and every longest row, the other rows empty or as long (nnz =
    maxrow and n * maxrow; anything between reaches no more than the first), one term, Arnoldi with a single column: the default
    knobs' reach.  The plan sees the longest row only through `ent * lanes < maxrow` with powers of two on the left, so it is
    constant on (2^k, 2^(k+1)]: both ends of every such interval are enough."""
    out = collections.defaultdict(set)
    for n in range(1, LDS_ROWS + 2):
        ends = sorted({1, n} | {v for k in range(12) for v in (2 ** k, 2 ** k + 1) if v <= n})
        for maxrow in ends:
            for nnz in (maxrow, n * maxrow):
                plan = cheby_plan(n, nnz, maxrow) if kind == "cheby" else arnoldi_plan(n, nnz, maxrow, 1)
                if plan:
                    out[plan[1:]].add(plan[0])
    return dict(out)


# every instance the two launchers' switches hold (csrc/kernels_small.hip): ent * rows_per_group <= 32
COMPILED = sorted((e, r) for e in (1, 2, 4, 8, 16, 32) for r in (1, 2, 4, 8, 16, 32) if e * r <= 32)
# ... and the ones the enumeration above reaches, pinned (tests/test_small_plan_host.py compares)
REACHABLE_CHEBY = sorted([(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (1, 2), (2, 2), (4, 2), (8, 2), (16, 2), (1, 4), (2, 4), (4, 4)])
REACHABLE_ARNOLDI = sorted(REACHABLE_CHEBY + [(8, 4)])


# ---------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------

def _hermitian_from_upper(n, rows, cols, rng, rho):
    """Hermitian CSR with the pattern {(i, j), (j, i)} of the given pairs (i <= j), random complex values (real on the diagonal),
    scaled so that every row's absolute sum -- Gershgorin -- is at most rho."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    v = rng.standard_normal(len(rows)) + 1j * rng.standard_normal(len(rows))
    diag = rows == cols
    v[diag] = v[diag].real
    off = ~diag
    A = sp.coo_matrix((np.concatenate([v, np.conj(v[off])]), (np.concatenate([rows, cols[off]]), np.concatenate([cols, rows[off]]))),
                      shape=(n, n)).tocsr()
    A.sort_indices()
    A = A * (rho / max(abs(A).sum(axis=1).max(), 1e-300))
    return sp.csr_matrix(A)


def banded(n, per_row, seed, rho=2.0):
    """Banded circulant, exactly `per_row` entries in every row: the diagonal when per_row is odd, and the distances 1 .. per_row // 2
    either way (all of them for per_row = n: dense)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    rows, cols = ([i], [i]) if per_row % 2 else ([], [])
    for d in range(1, per_row // 2 + 1):
        j = (i + d) % n
        if 2 * d == n:               # (the distance n / 2 is its own mirror image)
            keep = i < j
            rows.append(i[keep]), cols.append(j[keep])
        else:
            rows.append(np.minimum(i, j)), cols.append(np.maximum(i, j))
    A = _hermitian_from_upper(n, np.concatenate(rows), np.concatenate(cols), rng, rho)
    assert np.all(np.diff(A.indptr) == per_row), (n, per_row)
    return A


def dense(n, seed, rho=2.0):
    i, j = np.triu_indices(n)
    return _hermitian_from_upper(n, i, j, np.random.default_rng(seed), rho)


def ragged(n, maxrow, seed, n_empty=3, planted=None, rho=2.0):
    """Rows of every length: ONE row of `maxrow` entries (`planted`, default the last row -- alone in the last row set of its lane
    group when n is one more than a multiple of the group count), `n_empty` empty rows (as many as the planted row's columns leave
    room for), every other row shorter than the planted one (for maxrow = 1: the planted row and half of the others hold one diagonal entry)."""
    rng = np.random.default_rng(seed)
    r0 = n - 1 if planted is None else planted
    others = np.array([i for i in range(n) if i != r0])
    own = maxrow % 2 == 1 or maxrow > len(others)      # the planted row's own diagonal entry
    partners = rng.choice(others, size=maxrow - (1 if own else 0), replace=False)
    free = np.setdiff1d(others, partners)
    empty = rng.choice(free, size=min(n_empty, len(free)), replace=False)
    length = np.zeros(n, dtype=np.int64)
    pairs = set()

    def add(i, j):
        pairs.add((min(i, j), max(i, j)))
        length[i] += 1
        if i != j:
            length[j] += 1
    if own:
        add(r0, r0)
    for c in partners:
        add(r0, int(c))
    live = np.setdiff1d(others, empty)
    cap = max(maxrow - 1, 1)
    if maxrow == 1:
        for i in live[::2]:
            add(int(i), int(i))
    else:
        for _ in range(len(live) * maxrow // 3):
            i, j = (int(x) for x in rng.choice(live, size=2))
            if (min(i, j), max(i, j)) in pairs or length[i] >= cap or length[j] >= cap:
                continue
            add(i, j)
    rows, cols = zip(*sorted(pairs))
    A = _hermitian_from_upper(n, rows, cols, rng, rho)
    lens = np.diff(A.indptr)
    assert lens[r0] == maxrow and lens.max() == maxrow and (maxrow == 1 or np.sum(lens == maxrow) == 1), (n, maxrow)
    assert len(empty) == 0 or np.all(lens[empty] == 0)
    return A


def same_pattern(A, seed, hermitian=True, rho=0.5):
    """Other values on the pattern of A (a control term / a non-Hermitian operator that selects the same instance)."""
    rng = np.random.default_rng(seed)
    coo = sp.triu(A).tocoo()
    if hermitian:
        return _hermitian_from_upper(A.shape[0], coo.row, coo.col, rng, rho)
    B = A.copy().astype(complex)
    B.data = rng.standard_normal(len(B.data)) + 1j * rng.standard_normal(len(B.data))
    return sp.csr_matrix(B * (rho / max(abs(B).sum(axis=1).max(), 1e-300)))


# ---------------------------------------------------------------------------------------------------------------------
# the case table: the smallest operator per instance, and a ragged variant of each
# ---------------------------------------------------------------------------------------------------------------------
# name, builder, n, longest row, (lanes, ent, rows_per_group) of the Chebychev grid (None: the general loop), of an Arnoldi sweep
Case = collections.namedtuple("Case", "name build n maxrow cheby arnoldi")


def _case(name, build, n, maxrow, cheby, arnoldi):
    return Case(name, build, n, maxrow, cheby, arnoldi)


CASES = [
    # rows_per_group = 1: n = 1, then dense n = 2, 3, 5, 9 for ent = 2, 4, 8, 16; dense n = 65: four lanes per row, the 32-slot form
    _case("e1r1-n1", lambda: dense(1, 1), 1, 1, (1, 1, 1), (1, 1, 1)),
    _case("e2r1-dense2", lambda: dense(2, 2), 2, 2, (1, 2, 1), (1, 2, 1)),
    _case("e4r1-dense3", lambda: dense(3, 3), 3, 3, (1, 4, 1), (1, 4, 1)),
    _case("e8r1-dense5", lambda: dense(5, 5), 5, 5, (1, 8, 1), (1, 8, 1)),
    _case("e16r1-dense9", lambda: dense(9, 9), 9, 9, (1, 16, 1), (1, 16, 1)),
    _case("e32r1-dense65", lambda: dense(65, 65), 65, 65, (4, 32, 1), (4, 32, 1)),
    # rows_per_group = 2: n = 513 with 1, 2, 3, 5, 9 entries per row; 9 per row is the packed Chebychev (16, 2)
    _case("e1r2-band1", lambda: banded(513, 1, 11), 513, 1, (1, 1, 2), (1, 1, 2)),
    _case("e2r2-band2", lambda: banded(513, 2, 12), 513, 2, (1, 2, 2), (1, 2, 2)),
    _case("e4r2-band3", lambda: banded(513, 3, 13), 513, 3, (1, 4, 2), (1, 4, 2)),
    _case("e8r2-band5", lambda: banded(513, 5, 15), 513, 5, (1, 8, 2), (1, 8, 2)),
    _case("e16r2-band9", lambda: banded(513, 9, 19), 513, 9, (1, 16, 2), (1, 16, 2)),
    # rows_per_group = 4: n = 1025 with 1, 2, 3 entries per row; 5 per row: Arnoldi only (Chebychev: beyond 600 rows no 32-slot form)
    _case("e1r4-band1", lambda: banded(1025, 1, 21), 1025, 1, (1, 1, 4), (1, 1, 4)),
    _case("e2r4-band2", lambda: banded(1025, 2, 22), 1025, 2, (1, 2, 4), (1, 2, 4)),
    _case("e4r4-band3", lambda: banded(1025, 3, 23), 1025, 3, (1, 4, 4), (1, 4, 4)),
    _case("e8r4-band5", lambda: banded(1025, 5, 25), 1025, 5, None, (1, 8, 4)),
    # the ragged variants: one planted longest row (the last one), a few empty rows, n no multiple of the group count
    _case("e1r1-ragged", lambda: ragged(7, 1, 31), 7, 1, (1, 1, 1), (1, 1, 1)),
    _case("e2r1-ragged", lambda: ragged(6, 2, 32, n_empty=2), 6, 2, (1, 2, 1), (1, 2, 1)),
    _case("e4r1-ragged", lambda: ragged(9, 4, 33), 9, 4, (1, 4, 1), (1, 4, 1)),
    _case("e8r1-ragged", lambda: ragged(13, 7, 35), 13, 7, (1, 8, 1), (1, 8, 1)),
    _case("e16r1-ragged", lambda: ragged(21, 13, 39), 21, 13, (1, 16, 1), (1, 16, 1)),
    _case("e32r1-ragged", lambda: ragged(83, 71, 65), 83, 71, (4, 32, 1), (4, 32, 1)),
    _case("e1r2-ragged", lambda: ragged(513, 1, 41), 513, 1, (1, 1, 2), (1, 1, 2)),
    _case("e2r2-ragged", lambda: ragged(599, 2, 42), 599, 2, (1, 2, 2), (1, 2, 2)),
    _case("e4r2-ragged", lambda: ragged(513, 4, 43), 513, 4, (1, 4, 2), (1, 4, 2)),
    _case("e8r2-ragged", lambda: ragged(599, 7, 45), 599, 7, (1, 8, 2), (1, 8, 2)),
    _case("e16r2-ragged", lambda: ragged(513, 12, 49), 513, 12, (1, 16, 2), (1, 16, 2)),
    _case("e1r4-ragged", lambda: ragged(1025, 1, 51), 1025, 1, (1, 1, 4), (1, 1, 4)),
    _case("e2r4-ragged", lambda: ragged(1025, 2, 52), 1025, 2, (1, 2, 4), (1, 2, 4)),
    _case("e4r4-ragged", lambda: ragged(1025, 4, 53), 1025, 4, (1, 4, 4), (1, 4, 4)),
    _case("e8r4-ragged", lambda: ragged(1025, 6, 55), 1025, 6, None, (1, 8, 4)),
]
CHEBY_CASES = [c for c in CASES if c.cheby]
BY_NAME = {c.name: c for c in CASES}
ARNOLDI_COLUMNS = 6      # columns of the sweeps of the GPU cases (fewer where the operator has fewer rows)


def arnoldi_columns(n):
    return max(1, min(ARNOLDI_COLUMNS, n - 1))
