"""The inputs of the fused-term tests, built on the host alone: tests/test_gpu_cheby_term.py runs them through qp_cheby_term on
every kernel family, tests/test_cheby_term_ref.py (no GPU) shows on the SAME inputs that the row-wise bound of
tests/cheby_term_ref.py catches every mutation of the formula.

A case is an operator (SciPy CSR, nrows x ncols; the matrix-free ones carry their strings / dense factors), the format and knobs
that take it to its kernel, the per-row length S_i of the bound, and the row offsets it is run at.  Rectangular cases append
G = 3 * 64 + 5 ghost columns that some rows read (a rank's local rows of a partitioned operator) and run at xoff = 0, 64 and G, the
largest the argument check admits.  Operand vectors: moduli in [0.5, 1.5) with random phases -- nonzero everywhere, so every row has
a magnitude, the empty ones too -- scaled per 64 elements by powers of two between 2^-20 and 2^20: a small row is protected by its
own bound, not by a global norm.  Scalars of order 0.1 to 3 with mixed signs."""
import dataclasses
import functools
import os
import sys
import zlib

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qprop_amd.synth as synth  # noqa: E402
import cheby_term_ref as R  # noqa: E402
import test_gpu_rowblock_bits as rb  # noqa: E402
from pauli_ref import PauliRef  # noqa: E402
from test_gpu_colblock import _random_sparse  # noqa: E402
from test_gpu_pauli_edges import _random_labels  # noqa: E402
from test_gpu_walk2 import _with_diagonal  # noqa: E402

G = 3 * 64 + 5
XOFFS = (0, 64, G)

C, BETA, A_PREV, A, A_D1, A_D2 = 0.7 - 1.3j, -0.9, 1.7, -0.6, 2.3, -1.4
PH_UNIT, PH_NONUNIT = complex(np.exp(-0.7j)), 0.6 - 1.1j

# the guard zones of the GPU tests (tests/test_gpu_cheby_term.py: Guarded; tests/split_term_cases.py: check_slab)
GUARD = 256
SENTINEL = complex(-7.25e33, 3.5e-21)
JUNK = complex(4.5e-9, -8.75e17)          # what an output vector holds before the call


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.complex128), np.ascontiguousarray(b, dtype=np.complex128)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@dataclasses.dataclass(frozen=True)
class Form:
    """One argument form of qp_cheby_term.  vout: "none" | "v0" (in place) | "new"; acc_out: "none" | "acc_in" (in place) | "new";
    defer: None or (skip, n_defer, a_d1, a_d2)."""
    name: str
    v0: bool
    vout: str
    acc_in: bool
    acc_out: str
    phase: complex
    defer: tuple = None

    @property
    def skip(self):
        return self.defer is not None and self.defer[0] != 0

    @property
    def n_defer(self):
        return 0 if self.defer is None or self.skip else self.defer[1]

    def defer_ref(self):
        return None if self.defer is None else R.defer_of(*self.defer)


FORMS = [
    Form("1-first", False, "new", False, "new", 1.0),
    Form("2-middle-in-place", True, "v0", True, "acc_in", 1.0),
    Form("3-middle-out-of-place", True, "new", True, "new", 1.0),
    Form("4-last", True, "none", True, "acc_in", PH_UNIT),
    Form("4-last-non-unit-phase", True, "none", True, "acc_in", PH_NONUNIT),
    Form("5-single-term", False, "none", False, "new", PH_UNIT),
    Form("6-skip", True, "v0", False, "none", 1.0, (1, 0, 0.0, 0.0)),
    Form("6-skip-acc-given", True, "v0", True, "new", PH_NONUNIT, (1, 0, A_D1, A_D2)),
    Form("7-defer1-psi-is-v0", True, "v0", False, "new", 1.0, (0, 1, A_D1, 0.0)),
    Form("7-defer1-acc-and-v0", True, "v0", True, "acc_in", PH_NONUNIT, (0, 1, A_D1, 0.0)),
    Form("7-defer1-acc-no-v0", False, "new", True, "acc_in", 1.0, (0, 1, A_D1, 0.0)),
    Form("8-defer2-acc", True, "v0", True, "acc_in", PH_UNIT, (0, 2, A_D1, A_D2)),
    Form("8-defer2-no-acc", True, "new", False, "new", PH_NONUNIT, (0, 2, A_D1, A_D2)),
    Form("9-phase-one", True, "v0", True, "acc_in", 1.0 + 0.0j, (0, 0, 0.0, 0.0)),
]
FORM_BY_NAME = {f.name: f for f in FORMS}


def scaled_vector(n, seed):
    """moduli in [0.5, 1.5), random phases, times 2^k per 64 elements, k in [-20, 20]"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 1.5, n) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, n))
    k = rng.integers(-20, 21, (n + 63) // 64)
    return np.ldexp(v.real, np.repeat(k, 64)[:n]) + 1j * np.ldexp(v.imag, np.repeat(k, 64)[:n])


# ---- row lengths of the bound -----------------------------------------------------------------------------------------------

def _pad4_of_block_max(lengths):
    """per row: the longest row of its 64-row block, rounded up to whole quads (the width a row-block layout stores)"""
    n = len(lengths)
    out = np.empty(n, dtype=np.int64)
    for b in range(0, n, 64):
        out[b:b + 64] = (int(lengths[b:b + 64].max()) + 3) // 4 * 4
    return out


def row_lengths(A):
    return np.diff(A.indptr).astype(np.int64)


def rowblock_lengths(A):
    return _pad4_of_block_max(row_lengths(A))


def packed_lengths(A):
    """Hermitian-packed row blocks: an upper section (columns >= row) and a lower one, each padded on its own"""
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    upper = np.bincount(rows[A.indices >= rows], minlength=A.shape[0])
    lower = np.bincount(rows[A.indices < rows], minlength=A.shape[0])
    return _pad4_of_block_max(upper) + _pad4_of_block_max(lower)


# ---- operators --------------------------------------------------------------------------------------------------------------

def with_ghosts(A, rows, seed, per_row=2, values=None):
    """A (n x n) with G ghost columns appended; ``rows`` read ``per_row`` of them each, the first of them column n and the last
    column n + G - 1 (the ends of the ghost range are read)."""
    n = A.shape[0]
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, dtype=np.int64)
    r = np.repeat(rows, per_row)
    c = np.concatenate([n + np.sort(rng.choice(G, per_row, replace=False)) for _ in rows])
    c[0], c[-1] = n, n + G - 1
    if values is None:
        v = rng.uniform(-1.0, 1.0, len(r)) + (1j * rng.uniform(-1.0, 1.0, len(r)) if np.abs(A.data.imag).max() > 0 else 0.0)
    else:
        v = rng.choice(np.asarray(values), len(r))
    Gh = sp.coo_matrix((v.astype(np.complex128), (r, c)), shape=(n, n + G)).tocsr()
    out = (sp.hstack([A, sp.csr_matrix((n, G), dtype=np.complex128)], format="csr") + Gh).tocsr()
    out.sort_indices()
    assert out.shape == (n, n + G) and out[:, n:].nnz == len(r)
    return out


def csr_lanes(A):
    """the lane rule of build_csr_arrays (csrc/engine_operator.hip): T = 2; while (T < 64 && T < mean) T *= 2"""
    mean = A.nnz / A.shape[0]
    T = 2
    while T < 64 and T < mean:
        T *= 2
    return T


CSR_N = 337


def csr_operator(T, real, rect):
    """n = 337 (n T is no multiple of 256 for any T; the last row block has 17 rows), a mean row length of 0.75 T -- well inside
    (T / 2, T] --, rows of length 0, 1, T, 4 T, 4 T + 1 and 8 T - 1 (the edges of the four-chain loop `p + 3 T < p1` and of the
    remainder loop; 8 T - 1 capped at the number of columns: T = 64 has 337 square, its 511 fit the rectangular one), the last
    two of them the last two rows.  Columns drawn per row anywhere, ghost columns included."""
    n, nc = CSR_N, CSR_N + (G if rect else 0)
    rng = np.random.default_rng(1000 * T + 10 * real + rect)
    special = {0: 0, 1: 1, 100: T, 200: 4 * T, n - 2: 4 * T + 1, n - 1: min(8 * T - 1, nc)}
    total = int(round(0.75 * T * n))
    rest = total - sum(special.values())
    others = [i for i in range(n) if i not in special]
    base, extra = divmod(rest, len(others))
    assert 0 < base + 1 <= nc
    spread = min(base, max(1, T // 2))          # ragged: base - spread .. base + spread, the mean kept
    lens = dict(special)
    delta = rng.integers(-spread, spread + 1, len(others) // 2)
    delta = np.concatenate([delta, -delta, np.zeros(len(others) % 2, dtype=np.int64)])
    for k, i in enumerate(others):
        lens[i] = base + int(delta[k]) + (1 if k < extra else 0)
    rp = np.concatenate(([0], np.cumsum([lens[i] for i in range(n)]))).astype(np.int64)
    assert rp[-1] == total
    col = np.concatenate([np.sort(rng.choice(nc, lens[i], replace=False)) for i in range(n)]).astype(np.int32)
    if rect:
        col[rp[n] - 1] = nc - 1          # the last ghost column is read (the largest column of the sorted last row becomes it)
    vals = rng.uniform(-1.0, 1.0, total) + (0.0 if real else 1j * rng.uniform(-1.0, 1.0, total))
    Am = sp.csr_matrix((vals.astype(np.complex128), col, rp), shape=(n, nc))
    Am.sort_indices()
    assert Am.has_canonical_format and csr_lanes(Am) == T, (T, Am.nnz / n)
    return Am


def lattice(N, offsets, diag=False, real=False):
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=offsets)
    if real:
        vals = vals.real.astype(np.complex128)
    if diag:
        rp, col, vals = _with_diagonal(rp, col, vals, N)
    return sp.csr_matrix((vals, col, rp), shape=(N, N))


def dense_matrix(n, real):
    rng = np.random.default_rng(7 + real)
    M = rng.uniform(-1.0, 1.0, (n, n)) + (0.0 if real else 1j * rng.uniform(-1.0, 1.0, (n, n)))
    return sp.csr_matrix(M.astype(np.complex128))


def pauli_strings(n):
    rng = np.random.default_rng(zlib.crc32(f"term-pauli-{n}".encode()))
    masks = _random_labels(n, 3 * n, rng) + [(1 << i, 0) for i in range(n)] + [(3 << i, 3 << i) for i in range(n - 1)] + [(0, 1 << i) for i in range(n)]
    masks = list(dict.fromkeys(masks))
    return [(complex(rng.uniform(-1, 1), rng.uniform(-1, 1)), m) for m in masks]


@dataclasses.dataclass
class Case:
    name: str
    family: str          # csr | rbcsr | coded | colblock | hrb | walk | dense | pauli | liouville
    A: object            # SciPy CSR, nrows x ncols (the assembled superoperator for the Liouvillian; None for Pauli strings)
    fmt: str             # CSR | RBCSR | HRB | DENSE | MATFREE
    knobs: dict
    S: np.ndarray
    variants: tuple = (None,)       # values of rbcsr_variant the case runs with (None: the default)
    extra: dict = dataclasses.field(default_factory=dict)

    @property
    def nrows(self):
        return self.A.shape[0] if self.A is not None else 1 << self.extra["n"]

    @property
    def ncols(self):
        return self.A.shape[1] if self.A is not None else 1 << self.extra["n"]

    @property
    def xoffs(self):
        return XOFFS if self.ncols > self.nrows else (0,)

    @property
    def seed(self):
        return zlib.crc32(self.name.encode())

    def vectors(self):
        """x (ncols), v0, acc (nrows): the uploads of every form"""
        return scaled_vector(self.ncols, self.seed), scaled_vector(self.nrows, self.seed + 1), scaled_vector(self.nrows, self.seed + 2)

    def sums(self, x):
        """(s, sabs) of the reference: the row sums and the magnitudes they are bounded with"""
        if self.family == "pauli":
            H = PauliRef(self.extra["n"], self.extra["strings"])
            return H.apply(x), H.abs_apply(x)
        s, sabs = R.row_sums(self.A, x)
        if self.family == "liouville":
            W = R.liouvillian_magnitude(self.extra["H"], (), x)
            assert np.all(W >= sabs * (1 - 1e-15))
            sabs = W
        return s, sabs


KEEP = {"small_nnz": 0, "cheby_graph": 0}


def _csr_case(T, real, rect):
    Am = csr_operator(T, real, rect)
    name = f"csr-T{T}-{'real' if real else 'complex'}{'-rect' if rect else ''}"
    return Case(name, "csr", Am, "CSR", dict(KEEP, colblock=0), row_lengths(Am), extra={"T": T})


def _ghost_rows(n, every=3):
    return np.arange(0, n, every)


def _end_rows(n):
    """every third row of the first and of the last 64: ghost columns read at both ends, the stencil in between left alone"""
    return np.unique(np.concatenate([np.arange(0, min(64, n), 3), np.arange(max(n - 64, 0), n, 3)]))


def shallow():
    """n = 337, four scattered entries per row: one quad per row block, stored <= 512 blocks -- the launcher clears the deep-unroll
    bit of rbcsr_variant"""
    n = 337
    return rb._csr(n, [(5 * i + 71 * np.arange(4) + 3) % n for i in range(n)], 131, 34)


def _rbcsr_case(which, rect):
    Am = {"complex": lambda: rb.scattered(False), "real": lambda: rb.scattered(True), "far": rb.far_columns,
          "band": lambda: rb.banded(576, 12, 109), "shallow": shallow}[which]()
    if rect:      # (the shallow operator: ghost entries at the two ends only, or its stored width would cross 512 per block)
        Am = with_ghosts(Am, _end_rows(Am.shape[0]) if which == "shallow" else _ghost_rows(Am.shape[0]), 31)
    # rbcsr_variant 7 on an operator with stored > 512 blocks is the eight-blocks-per-workgroup launch, 4-6 the deep unroll in
    # workgroups of four, 0-3 the shallow unroll; on the shallow operator 7 and 4 run instances 3 and 0.  (far has 8 entries per
    # row: 512 per block and the layout's block of slack -- deep by the launcher's rule.)
    variants = {"complex": (7, 6, 2), "real": (7, 5), "far": (7, 0), "band": (7, 4), "shallow": (7, 4)}[which]
    return Case(f"rbcsr-{which}{'-rect' if rect else ''}", "rbcsr", Am, "RBCSR", dict(KEEP, colblock=0, value_dict=0),
                rowblock_lengths(Am), variants=variants, extra={"which": which, "rect": rect})


def _coded_case(which, rect):
    Am = rb.spin_chain(**rb.CHAINS[which])
    if rect:     # ghost entries with values the chain has already: the blocks' tables stay as short as they were
        Am = with_ghosts(Am, _ghost_rows(Am.shape[0], 2), 37, values=np.unique(Am.data)[:4])
    return Case(f"coded-{which}{'-rect' if rect else ''}", "coded", Am, "RBCSR", dict(KEEP, colblock=0, value_dict=1),
                rowblock_lengths(Am), extra={"which": which})


def _colblock_case(rpt, rect):
    """127 rows of 12 entries: more than the 1024 entries of a segment in the only 128-row tile, so tiles of 64 rows (rpt 1);
    200 rows of 4: tiles of 128 rows (rpt 2).  Rows 0, n / 2 and n - 1 are empty."""
    n, per_row = (127, 12) if rpt == 1 else (200, 4)
    nc = n + (G if rect else 0)
    Am = _random_sparse(n, nc, per_row, np.random.default_rng(41 + rpt + 2 * rect), empty_rows=(0, n // 2, n - 1))
    return Case(f"colblock-rpt{rpt}{'-rect' if rect else ''}", "colblock", Am, "RBCSR", dict(KEEP, colblock=2, cb_log2w=8, value_dict=0),
                row_lengths(Am), extra={"rows_per_tile": 64 * rpt})


Z16_N = 1000
Z16_OFFSETS = (1, 2, 3, 4, 16, 32, 48, 64)


def _hrb_case(which, rect):
    if which == "scattered":
        Am = rb.scattered_hermitian()
    elif which == "lattice12":
        Am = lattice(rb.LATTICE_N, rb.LATTICE_OFFSETS)
    else:      # z = 16: eight upper and eight lower entries per row, two quads per section -- the straight-line DEEP path
        Am = lattice(Z16_N, Z16_OFFSETS)
    if rect:
        Am = with_ghosts(Am, _end_rows(Am.shape[0]), 43)
    return Case(f"hrb-{which}{'-rect' if rect else ''}", "hrb", Am, "HRB", dict(KEEP, colblock=0, hrb_walk=0), packed_lengths(Am),
                variants=(15, 31), extra={"which": which})


def _walk_case(which, rect):
    if which == "5point":
        Am = lattice(1 << 14, (1, 64), diag=True)
    else:
        Am = lattice(1 << 15, (2, 16, 192, 384), diag=True)
    if rect:      # ghost columns read by rows of the first and the last row block only: the lattice in between stays walkable
        Am = with_ghosts(Am, _end_rows(Am.shape[0]), 47)
    return Case(f"walk-{which}{'-rect' if rect else ''}", "walk", Am, "HRB", dict(KEEP, colblock=0, hrb_walk=1, walk_min_blocks=16, walk_pair=0),
                packed_lengths(Am), variants=(15, 31) if rect else (15,), extra={"which": which})


def _dense_case(real):
    Am = dense_matrix(200, real)
    return Case(f"dense-{'real' if real else 'complex'}", "dense", Am, "DENSE", dict(KEEP), np.full(200, 200, dtype=np.int64))


def _pauli_case(n):
    strings = pauli_strings(n)
    return Case(f"pauli-{n}q", "pauli", None, "MATFREE", dict(KEEP), np.full(1 << n, len(strings), dtype=np.int64),
                extra={"n": n, "strings": strings})


def _liouville_case(n):
    H = synth.dense_hermitian(n, rho=2.0, rng=np.random.default_rng(50 + n))
    Lm = synth.ham_to_superop(H, "TDSE").tocsr()
    Lm.sum_duplicates()
    Lm.sort_indices()
    return Case(f"liouville-n{n}", "liouville", Lm, "MATFREE", dict(KEEP), np.full(n * n, 2 * n + 4, dtype=np.int64), extra={"H": H, "n_hilbert": n})


BUILDERS = {}
for _T in (2, 4, 8, 16, 32, 64):
    for _real in (False, True):
        for _rect in (False, True):
            BUILDERS[f"csr-T{_T}-{'real' if _real else 'complex'}{'-rect' if _rect else ''}"] = functools.partial(_csr_case, _T, _real, _rect)
for _rect in (False, True):
    _sfx = "-rect" if _rect else ""
    for _w in ("shallow", "complex", "real", "far", "band"):
        BUILDERS[f"rbcsr-{_w}{_sfx}"] = functools.partial(_rbcsr_case, _w, _rect)
    for _w in ("uniform", "dyadic", "sigma_y"):
        BUILDERS[f"coded-{_w}{_sfx}"] = functools.partial(_coded_case, _w, _rect)
    for _rpt in (1, 2):
        BUILDERS[f"colblock-rpt{_rpt}{_sfx}"] = functools.partial(_colblock_case, _rpt, _rect)
    for _w in ("scattered", "lattice12", "z16"):
        BUILDERS[f"hrb-{_w}{_sfx}"] = functools.partial(_hrb_case, _w, _rect)
    for _w in ("5point", "near2far2+diag"):
        BUILDERS[f"walk-{_w}{_sfx}"] = functools.partial(_walk_case, _w, _rect)
for _real in (False, True):
    BUILDERS[f"dense-{'real' if _real else 'complex'}"] = functools.partial(_dense_case, _real)
for _n in (6, 8):
    BUILDERS[f"pauli-{_n}q"] = functools.partial(_pauli_case, _n)
for _n in (8, 33):
    BUILDERS[f"liouville-n{_n}"] = functools.partial(_liouville_case, _n)
CASE_NAMES = list(BUILDERS)
# the operators qp_mul is checked on as well (tests/test_gpu_cheby_term.py: test_mul_rows_on_rectangular_operators)
MUL_CASE_NAMES = [n for n in CASE_NAMES if n.endswith("-rect") and n.split("-")[0] in ("csr", "rbcsr", "coded", "colblock")]


@functools.lru_cache(maxsize=4)
def case(name):
    c = BUILDERS[name]()
    assert c.name == name and len(c.S) == c.nrows
    return c


def reference(c, x, xoff, v0, acc, form, sums=None, mutation=None):
    """(t, r, T, R) of ``form`` on the case's operator at row offset xoff"""
    s, sabs = c.sums(x) if sums is None else sums
    return R.term_from_sums(s, sabs, x, xoff, v0 if form.v0 else None, acc if form.acc_in else None, C, BETA, A_PREV, A, form.phase,
                            form.defer_ref(), mutation=mutation)
