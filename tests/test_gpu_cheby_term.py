"""The contract of ONE fused Chebyshev term (include/qprop.h, the comment above qp_cheby_term; the row epilogue ChebyOpT::row of
csrc/kernel_common.h) on every kernel family that ends in it, through direct calls of L.cheby_term: every argument form the header
allows, row offsets into a longer gathered vector, outputs inside guard zones -- each output compared ROW BY ROW with the
extended-precision reference of tests/cheby_term_ref.py under its derived bound (S_i + K) 2^-52 magnitude_i.  Nothing is measured
into the bound; tests/test_cheby_term_ref.py shows on these very inputs (tests/cheby_term_cases.py) that a wrong operand,
coefficient, phase or matrix entry on one row lands beyond it.

Every case first proves its kernel path from the information getters, then from the statistics of every call (one launch and one
mat-vec per term; two launches for the matrix-free Liouvillian: the apply and cheby_epilogue_kernel):

    csr        csr_spmv_kernel<T>, T = 2 .. 64 lanes per row by the rule of build_csr_arrays (csrc/engine_operator.hip):
               T = 2; while (T < 64 && T < mean row length) T *= 2 -- the case computes T with the same expression from its
               operator and requires the T of its name; complex values and all-real ones (the `double` instance).  The library
               reports no lane count: that the instance ran is the launcher's rule, not observed.
    rbcsr      rbcsr_spmv_kernel: rbcsr_variant 7 on an operator with stored > 512 blocks is the eight-blocks-per-workgroup
               launch, 4-6 the deep unroll in workgroups of four, 0-3 (and every variant on an operator with stored <= 512
               blocks: four entries per row here) the shallow one; int16, int32 and stencil column sections by encoding_info.
    coded      rbcsr_coded_spmv_kernel (value_encoding_info valid), short, long and complex tables.
    colblock   the column-blocked mirror (colblock_info valid), tiles of 64 and of 128 rows.
    hrb        hrb_spmv_kernel with hrb_walk = 0: lower sections by position, lower stencil with the shared loop, the straight-line
               DEEP path (two quads per section); variant 15 (eight blocks per workgroup) and 31 (NEAR cross-lane gather).
    walk       the one-term strip walk (walk_info valid, walk_pair = 0).  At xoff != 0 the launcher declines it (the row-local
               operand is no longer the gathered vector's own rows: csrc/kernels.hip, `op.e.xloc == x`) and the per-block kernel
               runs, variant 31 with near_ok false -- again the launcher's rule: the statistics count one launch either way.
    dense      the dense row kernel; pauli: the fused Pauli-string kernel; liouville: apply + the unfused cheby_epilogue_kernel.

Guard zones: vout and acc_out are views into the middle of longer device buffers with 256 sentinel elements either side, which
must come back bit for bit after every call -- n = 337 has a last row block of 17 rows, n T of the CSR operators is no multiple of
the workgroup, and the rectangular cases shift the row-local operand.  Inputs that are not outputs come back as uploaded."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
from hypothesis import HealthCheck, given, settings, strategies as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qprop_amd.lib as L  # noqa: E402
import cheby_term_ref as R  # noqa: E402
import cheby_term_cases as cases  # noqa: E402
from cheby_term_cases import A, A_PREV, BETA, C, GUARD, JUNK, SENTINEL, same_bits  # noqa: E402
from test_gpu_rowblock_bits import knobs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


class Guarded:
    """n elements in the middle of a device buffer of n + 2 * GUARD, sentinels either side"""

    def __init__(self, ctx, n):
        self.n = n
        self.buf = L.State(ctx, n=n + 2 * GUARD)
        self.view = L.State(ctx, n=n, device_ptr=self.buf.ptr + 16 * GUARD, keepalive=self.buf)
        self.host = np.full(n + 2 * GUARD, SENTINEL)

    def load(self, data):
        self.host[GUARD:GUARD + self.n] = data
        self.buf.upload(self.host)

    def read(self, what):
        got = self.buf.numpy()
        assert same_bits(got[:GUARD], self.host[:GUARD]), f"{what}: a store BEFORE the vector"
        assert same_bits(got[GUARD + self.n:], self.host[GUARD + self.n:]), f"{what}: a store BEHIND the vector"
        return got[GUARD:GUARD + self.n].copy()

    def close(self):
        self.view.close()
        self.buf.close()


class Vectors:
    """the device vectors of one operator: guarded outputs, plain inputs"""

    def __init__(self, ctx, nrows):
        self.V, self.ACC = Guarded(ctx, nrows), Guarded(ctx, nrows)
        self.v0, self.acc_in = L.State(ctx, n=nrows), L.State(ctx, n=nrows)
        self.junk = np.full(nrows, JUNK)

    def close(self):
        for h in (self.V, self.ACC, self.v0, self.acc_in):
            h.close()


def run_form(ctx, op, xs, xoff, form, v0, acc, vec, launches, what):
    """One call of L.cheby_term in ``form``; (vout, acc_out) as downloaded (None where the form has none).  Asserted here: the
    launches, the sentinels, untouched outputs the form does not write, inputs that are not outputs."""
    V, ACC = vec.V, vec.ACC
    V.load(v0 if form.vout == "v0" else vec.junk)
    ACC.load(acc if form.acc_out == "acc_in" else vec.junk)
    v0_arg = acc_in_arg = None
    if form.v0:
        v0_arg = V.view if form.vout == "v0" else vec.v0.upload(v0)
    if form.acc_in:
        acc_in_arg = ACC.view if form.acc_out == "acc_in" else vec.acc_in.upload(acc)
    defer = None if form.defer is None else L.qp_acc_defer(*form.defer)
    ctx.reset_stats()
    L.cheby_term(op, xs, xoff, v0_arg, None if form.vout == "none" else V.view, acc_in_arg, None if form.acc_out == "none" else ACC.view,
                 C, BETA, A_PREV, A, form.phase, defer)
    stats = ctx.stats()
    assert stats["n_kernel_launches"] == launches and stats["n_matvec"] == 1, (what, stats)
    vout, accout = V.read(what + " vout"), ACC.read(what + " acc_out")
    if form.vout == "none":
        assert same_bits(vout, vec.junk), f"{what}: no vout, and the vector was written"
        vout = None
    if form.acc_out == "none" or form.skip:
        assert same_bits(accout, vec.junk if form.acc_out != "acc_in" else acc), f"{what}: a skipped term wrote the accumulator"
        accout = None
    if v0_arg is vec.v0:
        assert same_bits(vec.v0.numpy(), v0), f"{what}: v0 is not as uploaded"
    if acc_in_arg is vec.acc_in:
        assert same_bits(vec.acc_in.numpy(), acc), f"{what}: acc_in is not as uploaded"
    return vout, accout


def check_form(c_S, ref, got, what):
    """every row of every output of the form under the bound; the largest err / bound"""
    t, r, T, Rm = ref
    vout, accout = got
    worst = 0.0
    if vout is not None:
        worst = max(worst, R.check_rows(vout, t, c_S, T, what + " vout", quiet=True))
    assert (accout is None) == (r is None), what
    if accout is not None:
        worst = max(worst, R.check_rows(accout, r, c_S, Rm, what + " acc_out", quiet=True))
    return worst


# ---- operators and the proof of their path --------------------------------------------------------------------------------------

def build(ctx, c):
    if c.family == "pauli":
        return L.PauliOperator(ctx, c.extra["n"], [c.extra["strings"]])
    if c.family == "liouville":
        return L.Liouvillian(ctx, [c.extra["H"]], (), convention="TDSE")
    return L.Operator(ctx, [L.Matrix.from_scipy(ctx, c.A)], 0, getattr(L, "FMT_" + c.fmt))


def prove_path(ctx, c, op):
    """What the getters say about the kernel the case is for; the launches one term must take."""
    assert (op.nrows, op.ncols) == (c.nrows, c.ncols) and op.format == getattr(L, "FMT_" + c.fmt), (op.format, c.fmt)
    if c.family in ("pauli", "dense"):
        return 1
    if c.family == "liouville":
        return 2
    assert op.colblock_info()["valid"] == (1 if c.family == "colblock" else 0)
    if c.family == "csr":
        assert cases.csr_lanes(c.A) == c.extra["T"]
        return 1
    lay, enc = op.layout_info(), op.encoding_info()
    blocks = (c.nrows + 63) // 64
    assert lay["blocks"] == blocks
    if c.family in ("rbcsr", "coded", "colblock"):
        assert op.value_encoding_info()["valid"] == (1 if c.family == "coded" else 0), op.value_encoding_info()
        # the padded row lengths of the bound are the widths the layout stores (+ a block of slack)
        assert lay["stored"] == 64 * int(cases.rowblock_lengths(c.A)[::64].sum()) + 64, lay
    if c.family == "colblock":
        assert op.colblock_info()["rows_per_tile"] == c.extra["rows_per_tile"], op.colblock_info()
    if c.family == "rbcsr":
        which = c.extra["which"]
        deep = lay["stored"] > 512 * blocks
        assert deep == (which != "shallow"), lay      # (far: 8 entries per row = 512 per block, and the layout's block of slack)
        if which == "far":
            assert enc["upper"]["int32"] == blocks
        elif which == "band":
            assert enc["upper"]["int32"] == 0 and enc["upper"]["stencil"] + enc["upper"]["int16"] == blocks
        else:
            assert enc["upper"]["int16"] == blocks, enc
        if which == "shallow":
            assert lay["stored"] == 256 * (blocks + (3 if c.extra["rect"] else 0)) + 64, lay
    if c.family == "hrb":
        assert op.walk_reason()[1] != "ok", op.walk_reason()
        which = c.extra["which"]
        if which == "scattered":
            assert enc["lower"]["stencil"] == 0
        else:
            assert lay["stencil_lower_blocks"] > 0.6 * blocks and lay["stencil_upper_blocks"] > 0.6 * blocks, lay
            # quads per section from the pattern: three and three (the shared loop) / two and two (the straight-line path)
            sq = c.A[:, :c.nrows].tocsr()
            rows = np.repeat(np.arange(c.nrows), np.diff(sq.indptr))
            up = np.bincount(rows[sq.indices > rows], minlength=c.nrows)
            lo = np.bincount(rows[sq.indices < rows], minlength=c.nrows)
            want = 3 if which == "lattice12" else 2
            full = sum(1 for b in range(0, c.nrows - 63, 64)
                       if -(-int(up[b:b + 64].max()) // 4) == want and -(-int(lo[b:b + 64].max()) // 4) == want)
            assert full >= 0.6 * blocks, (full, blocks)
    if c.family == "walk":
        wi = op.walk_info()
        assert wi["valid"] == 1 and op.walk_reason()[1] == "ok", (wi, op.walk_reason())
        assert wi["end_block"] - wi["first_block"] > 0.5 * blocks, wi
    return 1


# ---- the contract on every kernel family -------------------------------------------------------------------------------------

def run_case(ctx, c, forms=cases.FORMS, xoffs=None):
    x, v0, acc = c.vectors()
    sums = c.sums(x)
    worst = {}
    with knobs(ctx, **c.knobs):
        op = build(ctx, c)
        launches = prove_path(ctx, c, op)
        xs = L.State(ctx, data=x)
        vec = Vectors(ctx, c.nrows)
        for variant in c.variants:
            with knobs(ctx, **({} if variant is None else {"rbcsr_variant": variant})):
                for xoff in (c.xoffs if xoffs is None else xoffs):
                    form2 = None
                    for form in forms:
                        what = f"{c.name} variant {variant} xoff {xoff} form {form.name}"
                        got = run_form(ctx, op, xs, xoff, form, v0, acc, vec, launches, what)
                        ref = cases.reference(c, x, xoff, v0, acc, form, sums=sums)
                        worst[what] = check_form(c.S, ref, got, what)
                        if form.name == "2-middle-in-place":
                            form2 = got
                        if form.name == "9-phase-one" and form2 is not None:
                            # phase = 1 + 0i: apply_phase is off -- the bits of form 2, which has no defer argument at all
                            assert same_bits(got[0], form2[0]) and same_bits(got[1], form2[1]), what
        assert same_bits(xs.numpy(), x), f"{c.name}: the gathered vector was written"
        vec.close()
        xs.close()
        op.close()
    top = max(worst, key=worst.get)
    print(f"[term rows] {c.name} ({c.family}): {len(worst)} calls, max err/bound {worst[top]:.4f} ({top})")
    return worst[top]


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_term_rows_against_extended_precision(ctx, name):
    """All argument forms (cheby_term_cases.FORMS: 1 first term, 2 middle term in place, 3 out of place, 4 last term with a unit
    and a non-unit phase, 5 single-term step, 6 skip without and with accumulators, 7 n_defer = 1 in its three operand
    combinations, 8 n_defer = 2 with and without acc_in, 9 phase 1 + 0i bit-identical to form 2) at every row offset of the case
    (0; 0, 64 and G for the rectangular ones) and every kernel variant it names: every row of vout and acc_out under
    (S_i + K) 2^-52 magnitude_i, K = 12 as derived in tests/cheby_term_ref.py; sentinels, untouched vectors and launch counts
    in run_form."""
    run_case(ctx, cases.case(name))


# ---- errors leave memory alone -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rbcsr-complex-rect", "csr-T8-complex-rect", "pauli-6q"])
def test_errors_leave_memory_alone(ctx, name):
    """Each refused call raises the documented error (csrc/engine_cheby.hip: cheby_term_args, qp_cheby_term) before anything is
    launched: no launch counted, every vector bit for bit as uploaded, the sentinels too."""
    c = cases.case(name)
    x, v0, acc = c.vectors()
    n = c.nrows
    with knobs(ctx, **c.knobs):
        op = build(ctx, c)
        prove_path(ctx, c, op)
        xs = L.State(ctx, data=x)
        vec = Vectors(ctx, n)
        longer = L.State(ctx, data=np.concatenate([v0, [1.0]]))
        inside_x = L.State(ctx, n=n, device_ptr=xs.ptr + 16 * (c.ncols - n), keepalive=xs)      # the last nrows elements of x
        one, two = L.qp_acc_defer(0, 1, cases.A_D1, 0.0), L.qp_acc_defer(0, 2, cases.A_D1, cases.A_D2)
        V, ACC = vec.V, vec.ACC
        vec.v0.upload(v0)
        vec.acc_in.upload(acc)
        top = c.ncols - n
        refused = [
            ("deferred accumulation needs v0", dict(v0=None, acc_in=vec.acc_in, defer=two)),
            ("deferred accumulation needs v0", dict(v0=None, acc_in=None, defer=two)),
            ("deferred accumulation needs v0", dict(v0=None, acc_in=None, defer=one)),
            ("deferred accumulation needs v0", dict(defer=L.qp_acc_defer(0, 3, 1.0, 1.0))),
            ("outputs must not overlap", dict(vout=inside_x)),
            ("outputs must not overlap", dict(acc_out=inside_x)),
            ("offset mismatch", dict(xoff=top + 1)),
            ("offset mismatch", dict(xoff=-1)),
            ("offset mismatch", dict(x=vec.v0, xoff=0) if c.ncols > n else dict(x=longer, xoff=0)),
            ("length mismatch", dict(v0=longer)),
            ("length mismatch", dict(vout=longer)),
            ("length mismatch", dict(acc_in=longer)),
            ("length mismatch", dict(acc_out=longer)),
            ("NULL argument", dict(acc_out=None)),
            ("NULL argument", dict(acc_out=None, defer=L.qp_acc_defer(0, 0, 0.0, 0.0))),
        ]
        for message, change in refused:
            V.load(vec.junk)
            ACC.load(vec.junk)
            args = dict(x=xs, xoff=0, v0=vec.v0, vout=V.view, acc_in=vec.acc_in, acc_out=ACC.view, defer=None)
            args.update(change)
            ctx.reset_stats()
            with pytest.raises(L.QPArgumentError, match=message):
                L.cheby_term(op, args["x"], args["xoff"], args["v0"], args["vout"], args["acc_in"], args["acc_out"], C, BETA, A_PREV, A,
                             cases.PH_NONUNIT, args["defer"])
            what = f"{name}: {message} {sorted(change)}"
            assert ctx.stats()["n_kernel_launches"] == 0, what
            assert same_bits(V.read(what), vec.junk) and same_bits(ACC.read(what), vec.junk), what
            assert same_bits(xs.numpy(), x) and same_bits(vec.v0.numpy(), v0) and same_bits(vec.acc_in.numpy(), acc), what
            assert same_bits(longer.numpy(), np.concatenate([v0, [1.0]])), what
        # ... and the same arguments without the fault are accepted: the operator still works
        got = run_form(ctx, op, xs, top, cases.FORM_BY_NAME["3-middle-out-of-place"], v0, acc, vec, 1, name)
        check_form(c.S, cases.reference(c, x, top, v0, acc, cases.FORM_BY_NAME["3-middle-out-of-place"]), got, name)
        for h in (inside_x, longer, vec, xs, op):
            h.close()


# ---- one property test -----------------------------------------------------------------------------------------------------------

@st.composite
def _random_rectangular(draw):
    n = draw(st.integers(1, 700))
    ghosts = draw(st.integers(0, 200))
    longest = draw(st.integers(1, 40))
    real = draw(st.booleans())
    seed = draw(st.integers(0, 2 ** 31 - 1))
    xoff = draw(st.integers(0, ghosts))
    form = draw(st.sampled_from([f for f in cases.FORMS if not f.name.startswith("9-")]))
    rng = np.random.default_rng(seed)
    nc = n + ghosts
    lens = np.minimum(rng.integers(0, longest + 1, n), nc)
    if draw(st.booleans()):
        lens[rng.integers(0, n, 3)] = 0
    rp = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    col = (np.concatenate([np.sort(rng.choice(nc, k, replace=False)) for k in lens]) if rp[-1] else np.zeros(0)).astype(np.int32)
    vals = rng.uniform(-1.0, 1.0, int(rp[-1])) + (0.0 if real else 1j * rng.uniform(-1.0, 1.0, int(rp[-1])))
    return sp.csr_matrix((vals.astype(np.complex128), col, rp), shape=(n, nc)), xoff, form, seed


@pytest.mark.parametrize("fmt", ["AUTO", "CSR", "RBCSR"])
@settings(max_examples=int(os.environ.get("QP_HYP_EXAMPLES", "25")), deadline=None,
          derandomize="QP_HYP_EXAMPLES" not in os.environ,      # fixed examples by default; set the variable to explore
          suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
@given(_random_rectangular())
def test_random_rectangular_operators_any_form(ctx, fmt, m):
    """Whatever the structure, the row offset and the form: every row under the bound, the sentinels intact.  S_i by the format the
    library took: the row's own length (CSR), the padded width of its row block (row blocks), ncols (dense)."""
    Am, xoff, form, seed = m
    n, nc = Am.shape
    if Am.nnz == 0:
        return
    op = L.Operator(ctx, [L.Matrix.from_scipy(ctx, Am)], 0, getattr(L, "FMT_" + fmt))
    S = {L.FMT_CSR: cases.row_lengths, L.FMT_RBCSR: cases.rowblock_lengths, L.FMT_HRB: cases.packed_lengths,
         L.FMT_DENSE: lambda M: np.full(n, nc, dtype=np.int64)}[op.format](Am)
    x, v0, acc = cases.scaled_vector(nc, seed + 1), cases.scaled_vector(n, seed + 2), cases.scaled_vector(n, seed + 3)
    xs, vec = L.State(ctx, data=x), Vectors(ctx, n)
    what = f"random {n} x {nc} format {op.format} xoff {xoff} form {form.name}"
    got = run_form(ctx, op, xs, xoff, form, v0, acc, vec, 1, what)
    s, sabs = R.row_sums(Am, x)
    ref = R.term_from_sums(s, sabs, x, xoff, v0 if form.v0 else None, acc if form.acc_in else None, C, BETA, A_PREV, A, form.phase,
                           form.defer_ref())
    check_form(S, ref, got, what)
    assert same_bits(xs.numpy(), x)
    for h in (vec, xs, op):
        h.close()


# ---- qp_mul on the same rectangular operators ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.MUL_CASE_NAMES)
def test_mul_rows_on_rectangular_operators(ctx, name):
    """mul!(y, A, x, alpha, beta) on the rectangular CSR, row-block, coded and column-blocked operators: every row under the bound of
    tests/test_gpu_pauli_edges.py, (S_i + 8) 2^-52 (|alpha| sum_j |a_ij| |x_j| + |beta| |y0_i|), against clongdouble, y inside guard
    zones."""
    c = cases.case(name)
    x, y0, _ = c.vectors()
    s, sabs = c.sums(x)
    n = c.nrows
    with knobs(ctx, **c.knobs):
        op = build(ctx, c)
        prove_path(ctx, c, op)
        xs, Y = L.State(ctx, data=x), Guarded(ctx, n)
        worst = 0.0
        for variant in c.variants:
            with knobs(ctx, **({} if variant is None else {"rbcsr_variant": variant})):
                for alpha, beta in ((1.0, 0.0), (2.0, 1.0), (0.5 - 1j, 0.25j)):
                    Y.load(y0)
                    ctx.reset_stats()
                    op.mul(xs, Y.view, alpha, beta)
                    assert ctx.stats()["n_kernel_launches"] == 1 and ctx.stats()["n_matvec"] == 1, ctx.stats()
                    what = f"{name} variant {variant} mul alpha {alpha} beta {beta}"
                    y = Y.read(what)
                    ref = R.CLD(beta) * y0.astype(R.CLD) + R.CLD(alpha) * s
                    mag = abs(alpha) * sabs + abs(beta) * np.abs(y0.astype(R.CLD))
                    err = np.abs(y.astype(R.CLD) - ref)
                    bnd = (c.S.astype(R.LD) + 8) * R.EPS * mag
                    assert np.all((mag > 0) | (sabs == 0))      # (beta = 0 on an empty row: the bound is zero, y_i must be exactly 0)
                    bad = np.nonzero(~(err <= bnd))[0]
                    assert bad.size == 0, f"{what}: {bad.size} rows beyond the bound, first {int(bad[0])}: err {float(err[bad[0]]):.3e} bound {float(bnd[bad[0]]):.3e}"
                    worst = max(worst, float(np.max(err[bnd > 0] / bnd[bnd > 0])))
        assert same_bits(xs.numpy(), x)
        print(f"[mul rows] {name}: max err/bound {worst:.4f}")
        for h in (Y, xs, op):
            h.close()
