"""The SPLIT fused Chebyshev term (qp_split_create, qp_cheby_term_split of csrc/engine_cheby.hip; launch_spmv with a RowSet,
csrc/kernels.hip; the mirror store of ChebyOpT::row and sync_wait / sync_signal, csrc/kernel_common.h) called directly on one GPU:
one term in two launches -- the boundary row blocks on a side stream, packing the new term vector into the exchange slab, the
interior row blocks on the context's stream -- on every row-block kernel family, with send sets and ghost columns chosen on the
host (tests/split_term_cases.py, whose helpers tests/test_split_term_cases_host.py shows to reject a wrong slot, a block taken twice
or not at all and a store past the slab).  Every output row is held to the derived bound (S_i + 12) 2^-52 magnitude_i of
tests/cheby_term_ref.py AND to the bits of qp_cheby_term on the same operator, knobs, vectors and form: one row, one sum, whichever
launch takes it.  No family is exempt from the bit identity: the row-block kernels run the same row-sum core (csrc/rowblock_sum.h)
under a block map as without one, and the strip walk adds a row's entries in the per-block kernel's order.

What is proven to run, and from what (the library reports neither the workgroup width nor the kernel instance of a launch; where
this says "launcher's rule" the instance follows from csrc/kernels.hip: launch_spmv, not from an observation):

    every case   prove_path of tests/test_gpu_cheby_term.py first: format, layout, column and value encodings by the getters.  The two
                 row sets: Split.n_boundary / n_interior (qp_split_info) equal partition() of the host module, so the block maps have
                 the expected lengths; that every block is in exactly one of them is shown by the outputs -- a row of a block not
                 taken keeps its junk bits, a block taken twice in the in-place form adds v0 twice.  Per call the statistics count
                 one launch per non-empty row set (two when both are non-empty) and ONE mat-vec.
    boundary     always workgroups of four row blocks, with the completion signal in the counter modes and the mirror whenever slab
                 and vout are given (launcher's rule: wide_ok is false with either).  That the mirror path ran is observed: slab[i]
                 has the bits of vout[send_rows[i]]; that a launch without vout or without slab stores nothing is observed too.
    rbcsr        rbcsr_spmv_kernel under a block map, double2 and `double` values: interior launch eight blocks per workgroup at
                 rbcsr_variant 7 on the deep operators (complex, real, far), wait threshold wait_from_wg / 2; workgroups of four at the
                 case's other variants (6, 2, 5, 0) and on the shallow operator (variants 7 and 4 run instances 3 and 0).
    coded        rbcsr_coded_spmv_kernel under a block map (value_encoding_info valid): interior eight per workgroup whatever
                 the variant, boundary four.
    hrb          hrb_spmv_kernel under a block map, hrb_walk = 0: interior eight per workgroup at variant 15, four at 31 (NEAR gather).
    walk         Split.walk_info (qp_split_walk_info): a plan of its own where the boundary blocks are a prefix and a suffix
                 (valid = 1, edge_blocks = n_interior - walked blocks, the walked range inside the interior and clear of the adjacent
                 blocks), none for scattered send rows.  With a plan, variant 15 and xoff = 0 the interior launch is the strip walk
                 (one launch in the statistics, its edge list the only part that waits); at xoff != 0 the launcher declines the walk
                 (`op.e.xloc == x`) and at variant 31 it is not asked: the per-block kernel over the interior block map.

Hand-off modes: split_mode 0 (events on both streams) and 1 (the in-launch counter).  Mode 2 takes the counter when at most 256
workgroups poll, which holds for every operator here (at most 1094 row blocks: 274 workgroups of four, of which the adjacent ones
poll -- at most 55 here), so in the single-call test it is mode 1; the chained test runs it by name.  A single call with
first = True waits for nothing (wait_target 0) but signals; the wait itself is exercised by test_split_term_chain, where term
m + 1's adjacent interior workgroups poll for term m's boundary launch.  split.check() after every call or chain: no wait timed out.
The polling bound stays at its default and no test disables the signal."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qprop_amd.lib as L  # noqa: E402
import cheby_term_cases as cases  # noqa: E402
import split_term_cases as sc  # noqa: E402
from cheby_term_cases import A, A_PREV, BETA, C, JUNK, same_bits  # noqa: E402
from test_gpu_cheby_term import Guarded, Vectors, build, check_form, prove_path, run_form  # noqa: E402
from test_gpu_rowblock_bits import knobs  # noqa: E402

pytestmark = pytest.mark.gpu
MODES = (0, 1)


@pytest.fixture(scope="module")
def tc():
    """(torch, context on torch's current stream, side stream)"""
    import torch
    torch.cuda.set_device(0)
    ctx = L.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    side = torch.cuda.Stream(device=torch.device("cuda", 0), priority=-1)
    yield torch, ctx, side
    ctx.close()


def join(torch, side):
    cur = torch.cuda.current_stream()
    side.wait_stream(cur)
    cur.wait_stream(side)


def variants_of(c):
    """the case's kernel variants; the walk cases also with 31 (the per-block kernel inside the row set)"""
    return (15, 31) if c.family == "walk" else c.variants


_SUMS = {}


def sums_of(c, x):
    """the row sums of the reference, computed once per operator and shared by every test of it"""
    if c.name not in _SUMS:
        _SUMS.clear()
        _SUMS[c.name] = c.sums(x)
    return _SUMS[c.name]


def expected_launches(part):
    return (1 if part.n_boundary else 0) + (1 if part.n_interior else 0)


def run_split_form(tc, op, split, part, xs, xoff, form, v0, acc, vec, SL, what, with_slab=True):
    """One call of L.cheby_term_split with first = True in ``form``; (vout, acc_out) as downloaded.  Asserted here: split.check(),
    the launches and the one mat-vec, the sentinels, untouched outputs, inputs that are not outputs, the slab."""
    torch, ctx, side = tc
    V, ACC = vec.V, vec.ACC
    V.load(v0 if form.vout == "v0" else vec.junk)
    ACC.load(acc if form.acc_out == "acc_in" else vec.junk)
    SL.load(np.full(SL.n, JUNK))
    v0_arg = acc_in_arg = None
    if form.v0:
        v0_arg = V.view if form.vout == "v0" else vec.v0.upload(v0)
    if form.acc_in:
        acc_in_arg = ACC.view if form.acc_out == "acc_in" else vec.acc_in.upload(acc)
    defer = None if form.defer is None else L.qp_acc_defer(*form.defer)
    join(torch, side)
    ctx.reset_stats()
    L.cheby_term_split(op, split, side.cuda_stream, True, xs, xoff, v0_arg, None if form.vout == "none" else V.view, acc_in_arg,
                       None if form.acc_out == "none" else ACC.view, SL.view if with_slab else None, C, BETA, A_PREV, A, form.phase, defer)
    split.check()
    stats = ctx.stats()
    assert stats["n_kernel_launches"] == expected_launches(part) and stats["n_matvec"] == 1, (what, stats)
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
    sc.check_slab(SL.buf.numpy(), vout if with_slab else None, part.send_rows, what)
    return vout, accout


def identical(a, b):
    return (a is None and b is None) or (a is not None and b is not None and same_bits(a, b))


# ---- the partition ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("send_set", list(sc.SEND_SETS))
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_partition_matches_host(tc, name, send_set):
    """Split.n_boundary / n_interior equal partition() of tests/split_term_cases.py; the walk plan of a split (host getters only):
    valid with `ends` send rows on walk-5point, edge_blocks = n_interior - (end_block - first_block), the walked range inside the
    interior and clear of the adjacent blocks; none with scattered send rows, with every block a boundary block, with a single
    interior block, and on every operator that has no plan of its own."""
    _, ctx, _ = tc
    c = cases.case(name)
    send = sc.SEND_SETS[send_set](c.nrows, cases.G)
    part = sc.partition(c.A, send)
    with knobs(ctx, **c.knobs):
        op = build(ctx, c)
        prove_path(ctx, c, op)
        split = L.Split(op, send)
        wi = split.walk_info()
        what = f"{name} {send_set}"
        sc.check_partition_counts(part, split.n_boundary, split.n_interior, wi, what)
        if c.family != "walk" or send_set in ("scattered", "all", "one-interior"):
            assert wi == dict(valid=0, first_block=0, end_block=0, edge_blocks=0), (what, wi)
        elif send_set == "ends":
            assert wi["valid"] == 1 and wi["end_block"] - wi["first_block"] >= 8, (what, wi)
            assert wi["edge_blocks"] == split.n_interior - (wi["end_block"] - wi["first_block"]), (what, wi)
            assert part.boundary.min() < wi["first_block"] and wi["end_block"] <= part.boundary.max(), (what, wi)
        split.close()
        op.close()


# ---- one split term, row by row ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("send_set", list(sc.SEND_SETS))
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_split_term_rows(tc, name, send_set):
    """Every Form of cheby_term_cases.FORMS x split_mode 0 and 1 x the case's kernel variants x its row offsets (0; 0, 64 and G on
    the rectangular operators -- on the walk case the offsets at which the launcher must leave the walk), one call with
    first = True each: split.check() OK; two launches (one where a row set is empty) and one mat-vec; sentinels, untouched
    outputs and inputs; every row of vout and acc_out under (S_i + 12) 2^-52 magnitude_i against the extended-precision reference;
    every output bit for bit that of L.cheby_term; slab[i] = vout[send_rows[i]] bit for bit inside a guarded buffer of
    nsend + 64 elements whose tail stays untouched, and the whole slab untouched for a form without vout.  One call per operator
    without a slab: the same outputs."""
    torch, ctx, side = tc
    c = cases.case(name)
    x, v0, acc = c.vectors()
    sums = sums_of(c, x)
    send = sc.SEND_SETS[send_set](c.nrows, cases.G)
    part = sc.partition(c.A, send)
    worst, calls = {}, 0
    with knobs(ctx, **c.knobs):
        op = build(ctx, c)
        launches = prove_path(ctx, c, op)
        split = L.Split(op, send)
        sc.check_partition_counts(part, split.n_boundary, split.n_interior, split.walk_info(), name)
        xs = L.State(ctx, data=x)
        vec = Vectors(ctx, c.nrows)
        SL = Guarded(ctx, len(send) + sc.SLAB_TAIL)
        for variant in variants_of(c):
            for xoff in c.xoffs:
                for form in cases.FORMS:
                    what = f"{name} {send_set} variant {variant} xoff {xoff} form {form.name}"
                    ref = cases.reference(c, x, xoff, v0, acc, form, sums=sums)
                    with knobs(ctx, **({} if variant is None else {"rbcsr_variant": variant})):
                        whole = run_form(ctx, op, xs, xoff, form, v0, acc, vec, launches, what + " unsplit")
                        worst[what] = check_form(c.S, ref, whole, what + " unsplit")
                        for mode in MODES:
                            with knobs(ctx, split_mode=mode):
                                got = run_split_form(tc, op, split, part, xs, xoff, form, v0, acc, vec, SL, f"{what} mode {mode}")
                            calls += 1
                            if not (identical(got[0], whole[0]) and identical(got[1], whole[1])):
                                check_form(c.S, ref, got, f"{what} mode {mode}")      # (names the row, if it is beyond the bound)
                                raise AssertionError(f"{what} mode {mode}: under the row bound, but not the bits of the unsplit term")
                        if form.name == "3-middle-out-of-place" and xoff == 0:
                            got = run_split_form(tc, op, split, part, xs, xoff, form, v0, acc, vec, SL, what + " no slab", with_slab=False)
                            assert identical(got[0], whole[0]) and identical(got[1], whole[1]), what + " no slab"
        assert same_bits(xs.numpy(), x), f"{name}: the gathered vector was written"
        for h in (SL, vec, xs, split, op):
            h.close()
    top = max(worst, key=worst.get)
    print(f"[split rows] {name} {send_set}: boundary {part.n_boundary} interior {len(part.plain)}+{len(part.adjacent)} blocks, {calls} split calls, "
          f"all bit-identical to the unsplit term, max err/bound {worst[top]:.4f} ({top})")


# ---- twelve terms, handed from call to call -------------------------------------------------------------------------------------

def _chain(tc, c, op, split, send, x0, coeffs, sched):
    """Twelve terms with the buffer rotation and accumulator schedule of ShardedCheby.step (qprop_amd/sharded.py), through the split
    entry point (``split`` given: the exchange emulated by a copy of the slab into the ghost slots on the side stream, no host
    synchronisation between the terms) or through L.cheby_term on one stream (the ghost copy by index_select of the send rows).
    Returns (X[0], X[1], acc) as downloaded: the result and the last term vector with their ghost slots."""
    torch, ctx, side = tc
    from qprop_amd.sharded import HipBackend
    be = HipBackend(ctx)
    n, nc, G = c.nrows, c.ncols, len(send)
    assert nc - n in (0, G)          # (a square operator has no ghost slot: the slab is packed, and nothing is copied)
    X = [be.zeros(nc), be.zeros(nc)]
    acc_t, slab_t = be.zeros(n), be.zeros(G)
    Xfull = [be.view(t, 0, nc) for t in X]
    Xloc = [be.view(t, 0, n) for t in X]
    accs, slab = be.view(acc_t, 0, n), be.view(slab_t, 0, G)
    send_idx = be.index(send)
    be.write(X[0], 0, x0)
    be.write(X[1], 0, np.full(nc, JUNK))
    be.write(acc_t, 0, np.full(n, JUNK))
    nterms = len(coeffs) - 1
    cc, updated = C, False
    if split is not None:
        join(torch, side)
    for m in range(1, nterms + 1):
        last = m == nterms
        xi, oi = (0, 1) if m % 2 == 1 else (1, 0)
        d = sched[m - 1]
        out = Xloc[0] if (m > 1 and last and xi == 1) else accs
        args = (Xfull[xi], 0, None if m == 1 else Xloc[oi], None if last else Xloc[oi], accs if (updated and not d.skip) else None,
                None if d.skip else out)
        scal = (cc, BETA, 0.0 if updated else float(coeffs[0]), float(coeffs[m]), cases.PH_UNIT if last else 1.0, d)
        if split is not None:
            L.cheby_term_split(op, split, side.cuda_stream, m == 1, *args, None if last else slab, *scal)
            if not last and nc > n:
                with torch.cuda.stream(side):
                    X[oi][2 * n: 2 * (n + G)].copy_(slab_t)
        else:
            L.cheby_term(op, *args, *scal)
            if not last and nc > n:
                torch.index_select(X[oi][: 2 * n].view(-1, 2), 0, send_idx, out=X[oi][2 * n: 2 * (n + G)].view(-1, 2))
        updated = updated or not d.skip
        if m == 1:
            cc = 2 * cc
    if split is not None:
        join(torch, side)
        split.check()
    torch.cuda.synchronize()
    assert out is Xloc[0]
    res = be.read(X[0], 0, nc), be.read(X[1], 0, nc), be.read(acc_t, 0, n)
    for h in Xfull + Xloc + [accs, slab]:
        h.close()
    return res


@pytest.mark.parametrize("split_mode", [0, 1, 2])
@pytest.mark.parametrize("name", sc.CHAIN_CASE_NAMES + sc.CHAIN_CASE_NAMES_WITH_INTERIOR)
def test_split_term_chain(tc, name, split_mode):
    """The hand-off between consecutive calls: twelve terms, `first` for term 1 only, v0 -> vout in place, the schedule of
    qp_acc_schedule_host, exactly G unordered send rows whose slab is copied on the SIDE stream into the ghost slots of the vector
    the next term gathers, no host synchronisation in between.  After joining the streams and split.check(): the result, the last
    term vector (with its ghost slots) and the accumulator are bit for bit those of the same twelve terms through L.cheby_term
    with the ghost copy by index_select on one stream; a second run of the split chain has equal bits.  Coefficients of moduli
    around one with C and BETA of the one-term test: twelve terms grow by some twenty orders of magnitude, far from overflow
    (asserted finite).  Every row of rbcsr-complex-rect and coded-uniform-rect reads a ghost column, so they have no interior block and
    nothing there waits: rbcsr-shallow-rect (ghost columns at the ends only) and the square rbcsr-complex and coded-uniform (no ghost
    slot to fill; the slab is still packed) run the same chain with interior blocks, all of them adjacent -- the wait in
    rbcsr_spmv_kernel, four and eight blocks per workgroup, and in rbcsr_coded_spmv_kernel."""
    torch, ctx, side = tc
    c = cases.case(name)
    n = c.nrows
    send = sc.chain_send_rows(n, cases.G)
    part = sc.partition(c.A, send)
    x0 = c.vectors()[0].copy()
    if c.ncols > n:
        x0[n:] = x0[send]      # the ghost slots of the first gathered vector: the send rows, as after the first exchange
    coeffs = np.array([0.9, -1.1, 0.8, 1.2, -0.7, 1.05, -0.95, 0.85, 1.15, -1.0, 0.75, 1.25, -0.9])
    sched = L.acc_schedule(coeffs)
    assert [d.skip for d in sched] != [0] * 12, "the schedule defers no update: qp_acc_defer is not exercised"
    with knobs(ctx, **c.knobs), knobs(ctx, rbcsr_variant=15 if c.fmt == "HRB" else 7):
        op = build(ctx, c)
        prove_path(ctx, c, op)
        split = L.Split(op, send)
        sc.check_partition_counts(part, split.n_boundary, split.n_interior, split.walk_info(), name)
        if c.family == "walk":
            assert split.walk_info()["valid"] == 1
        if name in sc.CHAIN_CASE_NAMES_WITH_INTERIOR:
            assert len(part.adjacent) >= 2
        whole = _chain(tc, c, op, None, send, x0, coeffs, sched)
        with knobs(ctx, split_mode=split_mode):
            ctx.reset_stats()
            first = _chain(tc, c, op, split, send, x0, coeffs, sched)
            stats = ctx.stats()
            second = _chain(tc, c, op, split, send, x0, coeffs, sched)
        assert stats["n_matvec"] == 12 and stats["n_kernel_launches"] == 12 * expected_launches(part), stats
        assert np.all(np.isfinite(whole[0].view(np.float64))) and np.abs(whole[0][:n]).max() > 0
        for k, what in enumerate(("the result (X[0])", "the last term vector (X[1]) and its ghost slots", "the accumulator")):
            assert same_bits(first[k], whole[k]), f"{name} mode {split_mode}: {what} differs from the unsplit chain"
            assert same_bits(second[k], first[k]), f"{name} mode {split_mode}: {what} differs between two runs"
        assert c.ncols == n or same_bits(whole[1][n:], whole[1][send]), "the ghost slots of the last term vector are not its send rows"
        split.close()
        op.close()


# ---- refused calls ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rbcsr-shallow-rect", "hrb-z16-rect"])
def test_split_errors_leave_memory_alone(tc, name):
    """Each refused call returns QP_E_BAD_ARG (csrc/engine_cheby.hip: qp_cheby_term_split, cheby_term_args) before anything is
    launched: no launch counted, every guarded vector and the slab bit for bit as uploaded; qp_split_create refuses a duplicate
    row, a row == nrows, a row < 0 and an operator in the CSR format.  Afterwards the same split still computes."""
    torch, ctx, side = tc
    c = cases.case(name)
    x, v0, acc = c.vectors()
    n, top = c.nrows, c.ncols - c.nrows
    send = sc.SEND_SETS["scattered"](n, cases.G)
    part = sc.partition(c.A, send)
    with knobs(ctx, **c.knobs):
        op, other = build(ctx, c), build(ctx, c)
        prove_path(ctx, c, op)
        split, split_of_other = L.Split(op, send), L.Split(other, send)
        xs, vec, SL = L.State(ctx, data=x), Vectors(ctx, n), Guarded(ctx, len(send) + sc.SLAB_TAIL)
        short = L.State(ctx, n=len(send) - 1, device_ptr=SL.view.ptr, keepalive=SL.buf)
        V, ACC = vec.V, vec.ACC
        vec.v0.upload(v0)
        vec.acc_in.upload(acc)
        refused = [
            ("bad arguments", dict(split=split_of_other)),
            ("slab too small", dict(slab=short)),
            ("bad arguments", dict(stream=None)),
            ("bad arguments", dict(acc_out=None)),
            ("bad arguments", dict(acc_out=None, defer=L.qp_acc_defer(0, 1, cases.A_D1, 0.0))),
            ("offset mismatch", dict(xoff=top + 1)),
            ("offset mismatch", dict(xoff=-1)),
        ]
        for message, change in refused:
            V.load(vec.junk)
            ACC.load(vec.junk)
            SL.load(np.full(SL.n, JUNK))
            a = dict(split=split, stream=side.cuda_stream, xoff=0, acc_out=ACC.view, slab=SL.view, defer=None)
            a.update(change)
            join(torch, side)
            ctx.reset_stats()
            with pytest.raises(L.QPArgumentError, match=message):
                L.cheby_term_split(op, a["split"], a["stream"], True, xs, a["xoff"], vec.v0, V.view, vec.acc_in, a["acc_out"], a["slab"],
                                   C, BETA, A_PREV, A, cases.PH_NONUNIT, a["defer"])
            what = f"{name}: {message} {sorted(change)}"
            torch.cuda.synchronize()
            assert ctx.stats()["n_kernel_launches"] == 0, what
            assert same_bits(V.read(what), vec.junk) and same_bits(ACC.read(what), vec.junk), what
            sc.check_slab(SL.buf.numpy(), None, send, what)
            assert same_bits(xs.numpy(), x) and same_bits(vec.v0.numpy(), v0) and same_bits(vec.acc_in.numpy(), acc), what
        for rows, message in (([5, 70, 5], "listed twice"), ([5, n], "out of range"), ([-1, 5], "out of range")):
            with pytest.raises(L.QPArgumentError, match=message):
                L.Split(op, np.array(rows, dtype=np.int64))
        with knobs(ctx, colblock=0):
            csr = L.Operator(ctx, [L.Matrix.from_scipy(ctx, c.A)], 0, L.FMT_CSR)
        assert csr.format == L.FMT_CSR
        with pytest.raises(L.QPArgumentError, match="row-block device format"):
            L.Split(csr, send)
        # ... and the split still works
        form = cases.FORM_BY_NAME["3-middle-out-of-place"]
        got = run_split_form(tc, op, split, part, xs, top, form, v0, acc, vec, SL, name)
        check_form(c.S, cases.reference(c, x, top, v0, acc, form), got, name)
        split.check()
        split_of_other.check()
        for h in (csr, short, SL, vec, xs, split, split_of_other, op, other):
            h.close()
