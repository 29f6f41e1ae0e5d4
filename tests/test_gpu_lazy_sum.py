"""The lazy operator sum -- evaluate! on the device, operator_refresh of csrc/engine_operator.hip: the stored values become
scale * (sum of the drift planes + sum_l c_l * control planes) -- beyond the 32 coefficients one launch carries (CoefBlock,
csrc/device.h), in every device format and in every mirror that follows the values.  After every move (set_coeffs / set_scale)
the values the library hands back (get_csr) are held, position by position, to the extended-precision reference of
tests/lazy_sum_ref.py under its derived bound (1.5 T_p + 2) 2^-52 M_p -- a position no term touches must be exactly zero -- and,
on a sample of positions, to the exact FMA chain in ascending term order BIT FOR BIT wherever scale * coeff is exact.  Nothing is
measured into the bound; tests/test_lazy_sum_ref.py shows on the same inputs (tests/lazy_sum_cases.py) that a dropped term, a lost
accumulate, a wrong chunk of coefficients, a shifted drift border, a stale real copy and the other summation order are all seen.

What reads the values is checked through them: mul! under the row bound of tests/cheby_term_ref.py for the real copy, the value
dictionary and the column-blocked mirror, the persistent small-system kernel against the oracle, the matrix-free Liouvillian at its
limit of 32 Hamiltonian terms.  Every test asserts through the library's own information calls (launch statistics, evaluate_info,
value_encoding_info, colblock_info, small_plan, build_info) that the path it is named after ran with the term count it names."""
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
import qprop_amd.propagator as P  # noqa: E402
import qprop_amd.synth as synth  # noqa: E402
import cheby_term_ref as RT  # noqa: E402
import lazy_sum_ref as R  # noqa: E402
import lazy_sum_cases as cases  # noqa: E402
import small_instances as si  # noqa: E402
from cheby_term_cases import row_lengths, rowblock_lengths, scaled_vector  # noqa: E402
from test_gpu_colblock import _random_sparse  # noqa: E402
from test_gpu_rowblock_bits import knobs  # noqa: E402

pytestmark = pytest.mark.gpu
FORMATS = {"CSR": L.FMT_CSR, "RBCSR": L.FMT_RBCSR, "HRB": L.FMT_HRB, "DENSE": L.FMT_DENSE, "AUTO": L.FMT_AUTO}
PLAIN = {"sparse_controls": 0, "value_dict": 0, "colblock": 0}      # the full combination alone: its launches can be counted


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def chunks(nterms):
    """launches of launch_combine_planes for nterms planes"""
    return -(-nterms // R.CHUNK)


def matrices(ctx, terms, n, ncols=None):
    return [L.Matrix(ctx, n, n if ncols is None else ncols, t.rowptr, t.col, t.vals) for t in terms]


def stored_values(op, rowptr, col, what):
    """(values at the positions of the union pattern, the SciPy matrix of get_csr).  The library's pattern must hold the union
    pattern; what it stores beyond it (a completed lattice, a completed dense operator) must be exactly zero."""
    n, nc = op.shape
    rp, cl, v = op.get_csr()
    A = sp.csr_matrix((v.copy(), cl.astype(np.int64), rp.copy()), shape=(n, nc))
    lin = np.repeat(np.arange(n), np.diff(rp)) * nc + cl
    assert np.all(np.diff(lin) > 0), f"{what}: get_csr is not sorted row by row"
    want = np.repeat(np.arange(n), np.diff(rowptr)) * nc + col
    at = np.searchsorted(lin, want)
    assert np.all(at < len(lin)) and np.array_equal(lin[np.minimum(at, len(lin) - 1)], want), f"{what}: a position of the union pattern is missing"
    extra = np.ones(len(lin), dtype=bool)
    extra[at] = False
    assert np.all(v[extra] == 0), f"{what}: a position outside the union pattern is not zero"
    return v[at], A


def check_values(op, c_planes, rowptr, col, nops, ncoeffs, coeffs, scale, sample, what, bits=True):
    """bound everywhere, bits on the sample (where the products are exact, and not on conjugated complex moves of a packed
    operator); returns (err / bound, the SciPy matrix)"""
    got, A = stored_values(op, rowptr, col, what)
    v, M, T = R.combined_ref(c_planes, R.effective(nops, ncoeffs, coeffs, scale, extended=True))
    worst = R.check_positions(got, v, M, T, what, quiet=True)
    packed_complex = op.format == L.FMT_HRB and not cases.all_real(coeffs, scale)
    if bits and R.product_is_exact(scale, coeffs) and not packed_complex:
        want = R.chain_exact(c_planes, R.effective(nops, ncoeffs, coeffs, scale), sample)
        bad = np.nonzero(got[sample] != want)[0]
        assert bad.size == 0, (f"{what}: {bad.size} of {len(sample)} sampled positions differ from the FMA chain in ascending term order, "
                               f"first position {int(sample[bad[0]])}: {got[sample[bad[0]]]!r} != {want[bad[0]]!r}")
    return worst, A


def apply_move(op, kind, arg):
    op.set_coeffs(arg) if kind == "c" else op.set_scale(arg)


# ---- the combined values in every format ------------------------------------------------------------------------------------

COMBINED = ([(f"L{n}", f) for n in cases.TERM_COUNTS for f in ("CSR", "RBCSR", "HRB", "DENSE")]
            + [(s, "RBCSR") for s in cases.SPLITS] + [("L33", "AUTO"), ("L33", "HRB-complex")])


@pytest.mark.parametrize("name,fmt", COMBINED, ids=[f"{n}-{f}" for n, f in COMBINED])
def test_combined_values(ctx, name, fmt):
    """Term counts 1, 2, 31, 32, 33, 64, 65 in CSR, row blocks, Hermitian-packed row blocks and the dense format; the three splits
    (no drift, all drift, the border inside the second chunk) in row blocks; one case left to FMT_AUTO with every knob at its
    default.  The moves of lazy_sum_cases.move_list; a packed operator gets the real ones only, except in the case "HRB-complex":
    there the complex coefficient takes it out of the packed format (re-laid out from the downloaded planes), its values stay
    inside the bound, and the later real moves are bit-exact again.  A full combination takes ceil(L / 32) launches."""
    c = cases.case(name)
    leave_packed = fmt == "HRB-complex"
    f = FORMATS["HRB" if leave_packed else fmt]
    sample = c.sample()
    worst = 0.0
    with knobs(ctx, **({} if fmt == "AUTO" else PLAIN)):
        op = L.Operator(ctx, matrices(ctx, c.terms, c.n), c.ncoeffs, f)
        assert len(op.ops) == c.L and (fmt == "AUTO" or op.format == f), (op.format, fmt)
        if f == L.FMT_HRB:
            assert op.build_info()["relayouts"] == 0
        coeffs, scale = np.ones(c.ncoeffs, dtype=np.complex128), 1.0 + 0.0j
        w, _ = check_values(op, c.planes, c.rowptr, c.col, c.L, c.ncoeffs, coeffs, scale, sample, f"{name} {fmt} as created")
        worst = max(worst, w)
        for i, (kind, arg) in enumerate(c.moves):
            new_c, new_s = (np.asarray(arg, dtype=np.complex128), scale) if kind == "c" else (coeffs, complex(arg))
            if f == L.FMT_HRB and not leave_packed and not cases.all_real(new_c, new_s):
                continue
            coeffs, scale = new_c, new_s
            was = op.format
            ctx.reset_stats()
            apply_move(op, kind, arg)
            launches = ctx.stats()["n_kernel_launches"]
            what = f"{name} {fmt} move {i} ({kind})"
            if fmt != "AUTO" and c.L >= 2 and op.format == was:
                assert launches == chunks(c.L), (what, launches)
            if leave_packed and not cases.all_real(coeffs, scale):
                assert op.format != L.FMT_HRB and op.build_info()["relayouts"] == 1, what
            elif fmt != "AUTO" and not leave_packed:
                assert op.format == f, what
            w, _ = check_values(op, c.planes, c.rowptr, c.col, c.L, c.ncoeffs, coeffs, scale, sample, what)
            worst = max(worst, w)
        if leave_packed:
            assert op.format != L.FMT_HRB and cases.all_real(coeffs, scale) and R.product_is_exact(scale, coeffs)
        op.close()
    print(f"[lazy sum] combined values {name} {fmt}: max err/bound {worst:.4f}")


# ---- the real copy ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["RBCSR", "CSR"])
@pytest.mark.parametrize("name", ["L33-real", "L65-real"])
def test_real_copy_follows_every_move(ctx, name, fmt):
    """Real planes, 33 and 65 terms: real -> complex coefficient -> real -> complex scale -> real.  The real copy (8 bytes per
    value, written by the LAST chunk of the combination only) must follow every move: y = A x under the row bound of
    tests/cheby_term_ref.py against the matrix get_csr returns, bit-identical with the knob real_vals at 0, and
    value_encoding_info reports 8 bytes per stored value on the all-real moves exactly."""
    c = cases.case(name)
    rng = np.random.default_rng(c.seed + 5)
    real1, real2, real3 = (cases._coeffs(rng, c.ncoeffs) for _ in range(3))
    cplx = real1.copy()
    cplx[c.ncoeffs // 2] = 0.5 - 0.75j
    cplx[-1] = -1.25 + 0.5j          # (a coefficient of the last chunk, and one of an earlier one)
    moves = [("c", real1), ("c", cplx), ("c", real2), ("s", cases.COMPLEX_SCALE), ("s", 1.0), ("c", real3)]
    x = scaled_vector(c.n, c.seed + 6)
    sample = c.sample()
    ys, worst = [], 0.0
    for knob in (1, 0):
        with knobs(ctx, real_vals=knob, **PLAIN):
            op = L.Operator(ctx, matrices(ctx, c.terms, c.n), c.ncoeffs, FORMATS[fmt])
            assert op.format == FORMATS[fmt] and len(op.ops) == c.L
            xs, out = L.State(ctx, data=x), L.State(ctx, n=c.n)
            res = []
            for (label, coeffs, scale), (kind, arg) in zip(cases.states(c.ncoeffs, moves), moves):
                apply_move(op, kind, arg)
                what = f"{name} {fmt} real_vals {knob} {label}"
                real = cases.all_real(coeffs, scale)
                stored = op.layout_info()["stored"]
                assert op.value_encoding_info()["plane_bytes"] == (8 if (real and knob) else 16) * stored, what
                w, A = check_values(op, c.planes, c.rowptr, c.col, c.L, c.ncoeffs, coeffs, scale, sample, what)
                ctx.reset_stats()
                op.mul(xs, out)
                assert ctx.stats()["n_kernel_launches"] == 1, what
                y = out.numpy()
                s, sabs = RT.row_sums(A, x)
                S = rowblock_lengths(A) if fmt == "RBCSR" else row_lengths(A)
                worst = max(worst, w, RT.check_rows(y, s, S, sabs, what, quiet=True))
                res.append(y)
            ys.append(res)
            for h in (xs, out, op):
                h.close()
    for a, b in zip(*ys):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{name} {fmt}: the real copy and the complex values give different bits"
    print(f"[lazy sum] real copy {name} {fmt}: max err/bound {worst:.4f}")


# ---- the sparse-control update ---------------------------------------------------------------------------------------------

SP_N = 197


def _band(rng, n, offsets, scale=1.0):
    r = np.concatenate([np.arange(n - d) for d in offsets])
    col = np.concatenate([np.arange(n - d) + d for d in offsets])
    v = scale * rng.uniform(0.5, 1.5, len(r)) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, len(r)))
    return cases.raw_csr(n, *cases.hermitian_entries(n, r, col, v))


def _sparse_control(rng, n, j, k):
    """a diagonal (even j) or one off-diagonal pair (odd j, distance 1, 2 or 7) on a window of rows of its own"""
    w = max(3, n // (k + 1))
    r0 = (j * w) % (n - w - 8)
    rows = np.arange(r0, r0 + w)
    d = 0 if j % 2 == 0 else (1, 2, 7)[(j // 2) % 3]
    v = np.ldexp(rng.uniform(0.5, 1.5, w), int(rng.integers(-8, 9))) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, w))
    return cases.raw_csr(n, *cases.hermitian_entries(n, rows, rows + d, v))


SPARSE_CASES = [(1, 1), (1, 31), (1, 32), (1, 33), (39, 3)]


@pytest.mark.parametrize("fmt", ["RBCSR", "HRB"])
@pytest.mark.parametrize("ndense,k", SPARSE_CASES, ids=[f"dense{d}-sparse{k}" for d, k in SPARSE_CASES])
def test_sparse_controls_many_terms(ctx, fmt, ndense, k):
    """A banded drift, ``ndense`` dense controls on the band, then k sparse controls (diagonals and single off-diagonal pairs on
    windows of rows): evaluate! rewrites only the positions of the sparse suffix, from a base that is the combination of the
    terms before it -- with 39 dense controls a base of 40 planes, combined in two chunks.  Moves: all coefficients; only sparse
    ones (the base is reused: ONE launch); a dense one -- coefficient 35, a plane of the second chunk, where there are that many
    -- (the base is rebuilt: its chunks + one launch); only sparse ones again.  After each the values equal the FMA chain on the
    sample, lie inside the bound everywhere, and are bit-identical with the knob sparse_controls at 0.  evaluate_info is the
    library's answer and is checked for consistency.  With k = 33 the library currently reports no sparse suffix at all (more than
    32 sparse trailing terms: find_sparse_controls gives up instead of taking the last 32) -- recorded, not required."""
    n = SP_N
    rng = np.random.default_rng(1000 * ndense + k)
    terms = [_band(rng, n, cases.OFFSETS)] + [_band(rng, n, cases.OFFSETS, 2.0 ** int(rng.integers(-6, 7))) for _ in range(ndense)]
    terms += [_sparse_control(rng, n, j, k) for j in range(k)]
    nops, ncoeffs = len(terms), len(terms) - 1
    rowptr, col, planes = cases.union_planes(terms, n)
    sample = R.sample_positions(planes, np.repeat(np.arange(n), np.diff(rowptr)) >> 6, 7 * k + ndense)
    c_all = cases._coeffs(rng, ncoeffs)
    c_sparse = c_all.copy()
    c_sparse[ndense:] = cases._coeffs(rng, k)
    c_dense = c_sparse.copy()
    c_dense[35 if ndense > 35 else 0] *= -0.75
    c_sparse2 = c_dense.copy()
    c_sparse2[-1] = 0.375
    c_sparse2[ndense] = -1.5
    moves = [("all", c_all), ("sparse", c_sparse), ("dense", c_dense), ("sparse", c_sparse2)]
    vals, worst = [], 0.0
    for knob in (1, 0):
        with knobs(ctx, sparse_controls=knob, value_dict=0, colblock=0):
            op = L.Operator(ctx, matrices(ctx, terms, n), ncoeffs, FORMATS[fmt])
            assert op.format == FORMATS[fmt] and len(op.ops) == nops
            ev = op.evaluate_info()
            sf = ev["first_sparse_term"]
            has_sparse = sf > 0
            if k <= 32:
                assert sf == 1 + ndense, ev          # (the windows keep the suffix under a quarter of the stored values)
                assert 0 < ev["positions"] <= op.layout_info()["stored"] // 4
            res = []
            for what_move, coeffs in moves:
                ctx.reset_stats()
                op.set_coeffs(coeffs)
                launches = ctx.stats()["n_kernel_launches"]
                what = f"sparse controls {fmt} dense {ndense} sparse {k} knob {knob} move {what_move}"
                ev = op.evaluate_info()
                assert ev["latest_update_sparse"] == (1 if (has_sparse and knob) else 0), (what, ev)
                if has_sparse and knob:
                    assert launches == (1 if what_move == "sparse" else chunks(sf) + 1), (what, launches)
                else:
                    assert launches == chunks(nops), (what, launches)
                w, _ = check_values(op, planes, rowptr, col, nops, ncoeffs, coeffs, 1.0, sample, what)
                worst = max(worst, w)
                res.append(stored_values(op, rowptr, col, what)[0])
            vals.append(res)
            op.close()
    for a, b in zip(*vals):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"{fmt} {ndense} {k}: the sparse update and the full combination differ"
    print(f"[lazy sum] sparse controls {fmt} dense {ndense} sparse {k}: max err/bound {worst:.4f}")


# ---- the value dictionary --------------------------------------------------------------------------------------------------

DICT_QUBITS = 8


def _pauli_terms(nq):
    masks = [m for i in range(nq) for m in ((1 << i, 0), (1 << i, 1 << i), (0, 1 << i))]          # X_i, Y_i, Z_i
    masks += [(0, 3 << i) for i in range(nq - 1)] + [(3 << i, 0) for i in range(nq - 1)]          # Z_i Z_i+1, X_i X_i+1
    return [synth.pauli_sum_matrix(nq, [(1.0, m)]) for m in masks]


def test_value_dictionary_many_terms(ctx):
    """An 8-qubit chain, N = 256: its 38 Pauli terms X_i, Y_i, Z_i, Z_i Z_i+1, X_i X_i+1 as 38 matrices in row blocks, 37 of them
    controls -- the dictionary's tables hold tuples of 38 values, combined in two chunks.  get_csr decodes through the table the
    mat-vec reads: the chain on the sample, the bound everywhere, after a real and after a complex move; mul! under the row bound
    and bit-identical with the knob value_dict at 0."""
    nq = DICT_QUBITS
    n = 1 << nq
    mats = _pauli_terms(nq)
    assert len(mats) == 38
    terms = [cases.from_scipy(M) for M in mats]
    nops, ncoeffs = len(terms), len(terms) - 1
    rowptr, col, planes = cases.union_planes(terms, n)
    sample = R.sample_positions(planes, np.repeat(np.arange(n), np.diff(rowptr)) >> 6, 38)
    rng = np.random.default_rng(38)
    moves = [cases._coeffs(rng, ncoeffs), cases._coeffs(rng, ncoeffs, cplx=True)]
    x = scaled_vector(n, 3838)
    ys, worst = [], 0.0
    for knob in (1, 0):
        with knobs(ctx, value_dict=knob, colblock=0, sparse_controls=0, small_nnz=0):
            op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M) for M in mats], ncoeffs, L.FMT_RBCSR)
            info = op.value_encoding_info()
            assert info["valid"] == knob and (not knob or info["table_entries"] > 0), info
            xs, out = L.State(ctx, data=x), L.State(ctx, n=n)
            res = []
            for i, coeffs in enumerate(moves):
                ctx.reset_stats()
                op.set_coeffs(coeffs)
                # the value plane and, where there is one, the tables: two chunks each
                assert ctx.stats()["n_kernel_launches"] == chunks(nops) * (2 if knob else 1), ctx.stats()
                what = f"value dictionary knob {knob} move {i}"
                w, A = check_values(op, planes, rowptr, col, nops, ncoeffs, coeffs, 1.0, sample, what)
                op.mul(xs, out)
                y = out.numpy()
                s, sabs = RT.row_sums(A, x)
                worst = max(worst, w, RT.check_rows(y, s, rowblock_lengths(A), sabs, what, quiet=True))
                res.append(y)
            ys.append(res)
            for h in (xs, out, op):
                h.close()
    for a, b in zip(*ys):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "the coded mat-vec and the plain one give different bits"
    print(f"[lazy sum] value dictionary, 38 terms: max err/bound {worst:.4f}")


# ---- the column-blocked mirror -------------------------------------------------------------------------------------------------

def test_colblock_mirror_many_terms(ctx):
    """N = 1100 (more than two column blocks of 2^9 columns), 33 random sparse terms, the mirror forced as
    tests/test_gpu_colblock.py forces it: the gather that follows a combination in two chunks.  real -> complex -> real; after
    each, the stored values inside the bound (the chain on the sample) and mul! through the mirror inside the row bound."""
    n, nterms = 1100, 33
    rng = np.random.default_rng(1100)
    # one entry per row on a random half of the rows per term: about 500 entries per (64-row, 512-column) cell of the union
    # pattern -- the mirror takes no cell beyond 1024 (csrc/operator_plans.cpp: plan_colblock)
    mats = [_random_sparse(n, n, 1, rng, empty_rows=rng.choice(n, n // 2, replace=False)) * 2.0 ** int(rng.integers(-10, 11))
            for _ in range(nterms)]
    terms = [cases.from_scipy(M) for M in mats]
    ncoeffs = nterms - 1
    rowptr, col, planes = cases.union_planes(terms, n)
    sample = R.sample_positions(planes, np.repeat(np.arange(n), np.diff(rowptr)) >> 6, 33)
    moves = [cases._coeffs(rng, ncoeffs), cases._coeffs(rng, ncoeffs, cplx=True), cases._coeffs(rng, ncoeffs)]
    x = scaled_vector(n, 1133)
    worst = 0.0
    with knobs(ctx, colblock=2, cb_log2w=9, sparse_controls=0):
        op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, M) for M in mats], ncoeffs, L.FMT_RBCSR)
        info = op.colblock_info()
        assert info["valid"] == 1 and info["column_blocks"] == 3 and info["log2_block_columns"] == 9 and len(op.ops) == nterms, info
        xs, out = L.State(ctx, data=x), L.State(ctx, n=n)
        for i, coeffs in enumerate(moves):
            ctx.reset_stats()
            op.set_coeffs(coeffs)
            assert ctx.stats()["n_kernel_launches"] == chunks(nterms) + 1, ctx.stats()      # (+ the mirror's gather)
            what = f"colblock mirror move {i}"
            w, A = check_values(op, planes, rowptr, col, nterms, ncoeffs, coeffs, 1.0, sample, what)
            op.mul(xs, out)
            s, sabs = RT.row_sums(A, x)
            worst = max(worst, w, RT.check_rows(out.numpy(), s, row_lengths(A), sabs, what, quiet=True))
        for h in (xs, out, op):
            h.close()
    print(f"[lazy sum] colblock mirror, 33 terms: max err/bound {worst:.4f}")


# ---- the persistent small-system kernel -------------------------------------------------------------------------------------

SMALL_STEPS = 6
SMALL_TLIST = np.linspace(0.0, 1.0, 25)[:SMALL_STEPS + 1]
SMALL_ENVELOPE = dict(E_min=-4.0, E_max=4.0)


@pytest.mark.parametrize("ncontrols", [32, 63, 64])
@pytest.mark.parametrize("name", ["e8r1-ragged", "e16r2-band9"])
def test_small_kernel_many_controls(ctx, name, ncontrols):
    """A drift plus 32, 63, 64 controls on the drift's pattern, on an instance of 16 register slots and on the packed one of 32
    (tests/small_instances.py): nops = 33 and 64 take the persistent kernel (its coef[nops] region in LDS, `tid < nops`, the
    in-register plane loop), nops = 65 the general loop (cheby_small_fits: nops <= 64).  Six steps, amplitudes given per interval and
    scaled so that the rows sum to at most 2 + 1.9 in absolute value (the envelope is [-4, 4]); stored states and the final state
    against the oracle at 1e-10, the persistent cases against the general loop at 1e-13 -- the bars of
    tests/test_gpu_small_instances.py -- forward and backward.  The launches counted are those of the time grid alone (the
    propagator is initialised first: the operator's build and its first evaluate! take ceil(nops / 32) launches of their own)."""
    c = si.BY_NAME[name]
    nops = ncontrols + 1
    H0 = c.build()
    ctrl = [si.same_pattern(H0, 5000 + 100 * c.n + j) for j in range(ncontrols)]
    mid = 0.5 * (SMALL_TLIST[1:] + SMALL_TLIST[:-1])
    amps = [(1.9 / (0.5 * ncontrols)) * np.sin((j + 2) * mid + 0.3 + 0.01 * j) for j in range(ncontrols)]
    rng = np.random.default_rng(c.n + ncontrols)
    psi0 = rng.standard_normal(c.n) + 1j * rng.standard_normal(c.n)
    psi0 /= np.linalg.norm(psi0)
    gen = P.hamiltonian(H0, *zip(ctrl, amps))
    assert len(gen.ops) == nops, "every control must keep its own term"
    ogen = qo.Generator([H0] + ctrl, amps)
    persistent = nops <= 64
    worst_o = worst_g = 0.0
    for backward in (False, True):
        rout, rst = qo.propagate(psi0, ogen, SMALL_TLIST, "cheby", storage=True, backward=backward, **SMALL_ENVELOPE)

        def run():
            p = P.init_prop(psi0, gen, SMALL_TLIST, "cheby", ctx=ctx, backward=backward, **SMALL_ENVELOPE)
            op = p._dgen.op
            plan = op.small_plan("cheby")
            assert len(op.ops) == nops
            ctx.reset_stats()
            st = P._propagate_fused(p, True, None)
            return plan, ctx.stats()["n_kernel_launches"], p.state.numpy(), st
        plan, launches, out, st = run()
        assert (plan == c.cheby) if persistent else (plan is None), (plan, c.cheby)
        assert (launches < SMALL_STEPS) == persistent, launches
        worst_o = max(worst_o, np.max(np.linalg.norm(st - rst, axis=0)), np.linalg.norm(out - rout))
        if persistent:
            L.tuning_set("small_nnz", 0)
            try:
                plan_g, launches_g, out_g, st_g = run()
            finally:
                L.tuning_set("small_nnz", si.SMALL_NNZ)
            assert plan_g is None and launches_g >= SMALL_STEPS
            worst_g = max(worst_g, np.max(np.linalg.norm(st - st_g, axis=0)), np.linalg.norm(out - out_g))
    print(f"[lazy sum] small kernel {name} nops {nops}: oracle {worst_o:.2e} (bar 1e-10), general loop {worst_g:.2e} (bar 1e-13)")
    assert worst_o < 1e-10
    assert worst_g < 1e-13


# ---- the matrix-free Liouvillian -----------------------------------------------------------------------------------------------

def _liouvillian_ref(Hs, eff, c_ops, x):
    """(L rho, magnitude) column-major in clongdouble, TDSE convention: [H, rho] + i sum (A rho A^+ - {A^+ A, rho} / 2) with
    H = sum eff_l H_l; the magnitude of tests/cheby_term_ref.py with |H| taken term by term, sum |eff_l| |H_l|"""
    n = Hs[0].shape[0]
    rho = np.asarray(x, dtype=RT.CLD).reshape(n, n).T
    H = sum(RT.CLD(e) * np.asarray(Hl, dtype=RT.CLD) for e, Hl in zip(eff, Hs))
    Hmag = sum(np.abs(RT.CLD(e)) * np.abs(np.asarray(Hl, dtype=RT.CLD)) for e, Hl in zip(eff, Hs))
    out = H @ rho - rho @ H
    for A in c_ops:
        A = np.asarray(A, dtype=RT.CLD)
        G = A.conj().T @ A
        out = out + RT.CLD(1j) * (A @ rho @ A.conj().T - (G @ rho + rho @ G) / 2)
    return out.T.reshape(-1), RT.liouvillian_magnitude(Hmag, c_ops, x)


def test_liouvillian_term_limit(ctx):
    """n = 6 (N = 36), two collapse operators: with 32 Hamiltonian terms, 31 of them controls, mul! after a real and after a complex
    move inside the Liouvillian row bound of tests/cheby_term_ref.py (S = 2 n + 4); with 33 terms creation is refused, and the
    context still runs the 32-term operator afterwards."""
    n, nterms = 6, 32
    rng = np.random.default_rng(632)
    Hs = [synth.dense_hermitian(n, rho=2.0 ** int(rng.integers(-6, 3)), rng=rng) for _ in range(nterms + 1)]
    c_ops = [0.3 * (rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))) / np.sqrt(n) for _ in range(2)]
    x = scaled_vector(n * n, 3636)
    S = np.full(n * n, 2 * n + 4, dtype=np.int64)
    op = L.Liouvillian(ctx, Hs[:nterms], c_ops, ncoeffs=nterms - 1, convention="TDSE")
    assert op.format == L.FMT_MATFREE and op.shape == (n * n, n * n)
    xs, out = L.State(ctx, data=x), L.State(ctx, n=n * n)
    worst = 0.0

    def check(coeffs, what):
        op.set_coeffs(coeffs)
        op.mul(xs, out)
        ref, mag = _liouvillian_ref(Hs[:nterms], R.effective(nterms, nterms - 1, coeffs, 1.0, extended=True), c_ops, x)
        return RT.check_rows(out.numpy(), ref, S, mag, what, quiet=True)
    worst = max(worst, check(cases._coeffs(rng, nterms - 1), "liouvillian 32 terms, real move"))
    worst = max(worst, check(cases._coeffs(rng, nterms - 1, cplx=True), "liouvillian 32 terms, complex move"))
    with pytest.raises(L.QPArgumentError, match="at most 32 Hamiltonian terms"):
        L.Liouvillian(ctx, Hs, c_ops, ncoeffs=nterms, convention="TDSE")
    worst = max(worst, check(cases._coeffs(rng, nterms - 1), "liouvillian 32 terms, after the refusal"))
    print(f"[lazy sum] liouvillian, 32 terms: max err/bound {worst:.4f}")
    for h in (xs, out, op):
        h.close()
