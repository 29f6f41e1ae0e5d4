"""The checker of the split-term tests checks (no GPU).  A host emulation of qp_cheby_term_split -- the model is term_split of
tests/np_backend.py: the boundary row blocks with the true gathered vector and the pack into the slab through the mirror table, the
interior row blocks with POISONED ghost slots, every row taken from the extended-precision reference rounded to double -- is driven
by the same three tables the device gets (boundary list, interior list, mirror).  Unmutated it passes the helpers of
tests/split_term_cases.py and the row bound of tests/cheby_term_ref.py in every argument form; with one table entry wrong it must
not.  The operators: hrb-z16 (square, 1000 rows: the last row block has 40 rows and is interior) and rbcsr-shallow-rect (337 rows
and ghost columns read at both ends; the last row block has 17 rows and is a boundary block), with the `scattered` send rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cheby_term_cases as cases  # noqa: E402
import split_term_cases as sc  # noqa: E402
from cheby_term_cases import GUARD, JUNK, SENTINEL  # noqa: E402
from np_backend import NumpyBackend, _Op  # noqa: E402
from test_gpu_cheby_term import check_form  # noqa: E402

OPERATORS = ("hrb-z16", "rbcsr-shallow-rect")
MUTATIONS = ("mirror-shifted-one-lane", "last-interior-block-left-out", "interior-block-twice-another-missing",
             "non-send-row-stores-to-slot-0", "slab-written-at-nsend", "interior-row-reads-ghost", "slab-filled-without-vout")


class Emulation:
    """one operator, its vectors, the two references (true and poisoned ghost slots) and the tables of its split"""

    def __init__(self, name, send_set="scattered"):
        self.c = c = cases.case(name)
        self.x, self.v0, self.acc = c.vectors()
        self.send_rows = sc.SEND_SETS[send_set](c.nrows, cases.G)
        self.part = sc.partition(c.A, self.send_rows)
        self.sums = c.sums(self.x)
        xp = self.x.copy()
        xp[c.nrows:] = np.nan
        self.sums_poisoned = c.sums(xp)

    def run(self, form, mutation=None):
        """(vout, acc_out, slab buffer with its guards, the reference) of one emulated call at xoff = 0"""
        c, p, n = self.c, self.part, self.c.nrows
        boundary, interior, mirror = p.boundary.copy(), p.interior.copy(), p.mirror.copy()
        nsend = len(self.send_rows)
        pack = form.vout != "none"
        late_store = None
        if mutation == "mirror-shifted-one-lane":
            mirror = np.roll(mirror, 1)
        elif mutation == "last-interior-block-left-out":
            interior = interior[interior != interior.max()]
        elif mutation == "interior-block-twice-another-missing":
            interior[1] = interior[0]
        elif mutation == "non-send-row-stores-to-slot-0":
            late_store = int(np.nonzero(mirror[:-1] < 0)[0][0])        # (the store that wins the race for the slot)
        elif mutation == "slab-written-at-nsend":
            mirror[int(np.nonzero(mirror[:-1] < 0)[0][0])] = nsend
        elif mutation == "interior-row-reads-ghost":
            reads = np.unique((np.nonzero(np.diff(c.A[:, n:].tocsr().indptr))[0]) // 64)
            moved = [b for b in reads if not np.any(self.send_rows // 64 == b)][-1]
            boundary, interior = boundary[boundary != moved], np.append(interior, moved)
            mirror = sc.mirror_of(boundary, self.send_rows, n)
        elif mutation == "slab-filled-without-vout":
            pack = True
        else:
            assert mutation is None
        ref = cases.reference(c, self.x, 0, self.v0, self.acc, form, sums=self.sums)
        poisoned = cases.reference(c, self.x, 0, self.v0, self.acc, form, sums=self.sums_poisoned)
        V = (self.v0 if form.vout == "v0" else np.full(n, JUNK)).copy()
        ACC = (self.acc if form.acc_out == "acc_in" else np.full(n, JUNK)).copy()
        slab = np.full(nsend + sc.SLAB_TAIL + 2 * GUARD, SENTINEL)
        slab[GUARD:GUARD + nsend + sc.SLAB_TAIL] = JUNK
        for blocks, (t, r, _, _), is_boundary in ((boundary, ref, True), (interior, poisoned, False)):
            t = t.astype(np.complex128)
            for k, b in enumerate(blocks):
                rows = np.arange(64 * b, min(64 * b + 64, n))
                if form.vout != "none":
                    V[rows] = t[rows]
                if r is not None:
                    ACC[rows] = r.astype(np.complex128)[rows]
                if is_boundary and pack:
                    slots = mirror[64 * k: 64 * k + len(rows)]
                    slab[GUARD + slots[slots >= 0]] = t[rows[slots >= 0]]
        if late_store is not None:
            slab[GUARD] = ref[0].astype(np.complex128)[64 * boundary[late_store // 64] + late_store % 64]
        return (None if form.vout == "none" else V), (None if r is None else ACC), slab, ref

    def check(self, form, mutation=None):
        what = f"{self.c.name} form {form.name} mutation {mutation}"
        vout, accout, slab, ref = self.run(form, mutation)
        check_form(self.c.S, ref, (vout, accout), what)
        sc.check_slab(slab, vout, self.send_rows, what)


@pytest.fixture(scope="module", params=OPERATORS)
def emu(request):
    return Emulation(request.param)


def test_the_operators_have_what_the_mutations_need(emu):
    p, n = emu.part, emu.c.nrows
    assert n % 64 != 0 and p.n_boundary >= 2 and p.n_interior >= 2
    assert np.any(p.mirror[:-1] < 0) and np.any(p.mirror >= 0)
    if emu.c.name == "hrb-z16":
        assert p.interior.max() == p.nblocks - 1          # the partial last row block is interior
    else:
        assert p.boundary.max() == p.nblocks - 1 and emu.c.ncols == n + cases.G
        assert np.all(p.mirror[64 * (p.n_boundary - 1) + n % 64:] == -1)      # lanes beyond nrows carry no slot


def test_the_unmutated_emulation_passes_in_every_form(emu):
    for form in cases.FORMS:
        emu.check(form)


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mutation_is_rejected(emu, mutation):
    if mutation == "interior-row-reads-ghost" and emu.c.ncols == emu.c.nrows:
        # a square operator has no ghost slot: there the poisoned reference IS the true one
        assert all(np.array_equal(a, b) for a, b in zip(emu.sums, emu.sums_poisoned))
        return
    form = cases.FORM_BY_NAME["4-last" if mutation == "slab-filled-without-vout" else "3-middle-out-of-place"]
    emu.check(form)
    with pytest.raises(AssertionError):
        emu.check(form, mutation)


def test_a_block_taken_twice_is_seen_in_place_as_well():
    """form 2 writes v0 -> vout in place: a block that is listed twice leaves another with its OLD v0, not with junk -- still rows
    beyond the bound"""
    emu = Emulation("hrb-z16")
    with pytest.raises(AssertionError, match="rows beyond the bound"):
        emu.check(cases.FORM_BY_NAME["2-middle-in-place"], "interior-block-twice-another-missing")


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_partition_agrees_with_the_numpy_backend(name):
    """partition() against make_split of tests/np_backend.py (written for the gloo tests) on every operator x send set of the GPU
    test: the same boundary and interior counts, the same rows; the three parts are disjoint and complete, the mirror is a
    bijection between the send rows and the slots."""
    c = cases.case(name)
    sets = dict(sc.SEND_SETS)
    if name in sc.CHAIN_CASE_NAMES + sc.CHAIN_CASE_NAMES_WITH_INTERIOR:
        sets["chain"] = sc.chain_send_rows
    be = NumpyBackend()
    for set_name, fn in sets.items():
        send = fn(c.nrows, cases.G)
        p = sc.partition(c.A, send)
        m = be.make_split(_Op(c.A), send)
        what = f"{name} {set_name}"
        sc.check_partition_counts(p, m.n_boundary, m.n_interior, what=what)
        assert np.array_equal(np.unique(m.brows // 64), p.boundary) and np.array_equal(np.unique(m.irows // 64), np.sort(p.interior)), what
        assert np.array_equal(np.sort(np.concatenate([p.boundary, p.adjacent, p.plain])), np.arange(p.nblocks)), what
        assert np.array_equal(p.interior, np.concatenate([p.plain, p.adjacent])), what
        slots = p.mirror[p.mirror >= 0]
        assert np.array_equal(np.sort(slots), np.arange(len(send))) and p.mirror[-1] == -1, what
        lanes = np.nonzero(p.mirror[:-1] >= 0)[0]
        assert np.array_equal(send[p.mirror[lanes]], 64 * p.boundary[lanes // 64] + lanes % 64), what
    if "chain" in sets:
        assert len(sets["chain"](c.nrows, cases.G)) == cases.G


def test_send_sets_are_what_their_names_say():
    n, G = 1000, cases.G
    nb = 16
    s = {k: f(n, G) for k, f in sc.SEND_SETS.items()}
    assert len(s["none"]) == 0 and list(s["last-row"]) == [n - 1]
    assert sorted(s["ends"]) == list(range(40)) + list(range(n - 40, n))
    assert list(s["all"]) == list(range(n - 1, -1, -1))
    blocks = s["scattered"] // 64
    assert sorted(set(blocks)) == list(range(0, nb, 2)) and 7 in s["scattered"]
    assert np.sum(blocks == 2) == 1 and np.sum(blocks == 4) == 2 and np.any(np.diff(s["scattered"]) > 0) and np.any(np.diff(s["scattered"]) < 0)
    assert sorted(set(s["one-interior"] // 64)) == [b for b in range(nb) if b != nb // 2]
    ch = sc.chain_send_rows(n, G)
    assert len(ch) == G == len(set(ch)) and set(ch // 64) <= {0, 1, nb - 2, nb - 1} and np.any(np.diff(ch) < 0)
