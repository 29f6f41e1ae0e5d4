"""Which instance of the persistent single-workgroup kernels a small system takes (csrc/small_plan.cpp, behind qp_small_plan_host):
the library against a Python mirror at every boundary, the set of instances an operator can reach under the default knobs, and the
case table of tests/test_gpu_small_instances.py against that set.  No GPU."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qprop_amd.lib as L  # noqa: E402
import small_instances as si  # noqa: E402


def _around_powers_of_two(top):
    out = {1, 2}
    p = 2
    while p <= top:
        out |= {p - 1, p, p + 1}
        p *= 2
    return sorted(v for v in out if v >= 0)


def test_plan_mirror_matches_the_library_at_every_boundary():
    """n on both sides of every change of the row-set count (512 rows per set for one lane per row, and its halvings for 2 .. 64
    lanes), of the 600-row rule and of the LDS limit; the longest row around every power of two up to 4096 (beyond 64 lanes x 32
    entries nothing fits); 16 and 32 slots.  Both answers of a pair must agree, taken or not."""
    ns = sorted({0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 600, 601,
                 767, 768, 769, 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049, 4096})
    taken = 0
    for n in ns:
        for maxrow in [0] + _around_powers_of_two(4096):
            for slots in (si.SLOTS, si.SLOTS_WIDE):
                got, want = L.small_plan(n, maxrow, slots), si.small_plan(n, maxrow, slots)
                assert got == want, (n, maxrow, slots, got, want)
                if got:
                    taken += 1
                    lanes, ent, rpg = got
                    # what the kernels rely on: every row has a lane group and a slot set, every entry of a row a slot
                    assert ent * rpg <= slots and lanes * ent >= maxrow and (si.THREADS // lanes) * rpg >= n
                    assert (ent, rpg) in si.COMPILED
    assert taken > 500
    assert L.small_plan(2049, 1) is None and L.small_plan(0, 1) is None and L.small_plan(2048, 1) == (1, 1, 4)


def test_reachable_instances_are_pinned_and_every_one_has_a_gpu_case():
    """The instances an operator of at most 2048 rows selects under the default knobs (small_nnz = 8192), by enumeration over the
    mirror of the two gates: 14 of the 21 compiled Chebychev instances, 15 Arnoldi ones, only ever with 1, 2 or 4 lanes per row.
    Each has a named case in the shared table whose own numbers select it -- by the mirror and by qp_small_plan_host --, and so
    does its ragged variant; and each is one of the instances the launchers' switches hold."""
    for kind, pinned in (("cheby", si.REACHABLE_CHEBY), ("arnoldi", si.REACHABLE_ARNOLDI)):
        reach = si.reachable(kind)
        assert sorted(reach) == pinned, (kind, sorted(reach))
        assert set().union(*reach.values()) == {1, 2, 4}
        assert set(pinned) <= set(si.COMPILED)
        # nothing with eight or more rows per lane group, nor the Chebychev (8, 4): compiled, never selected
        assert all(r < 8 for _, r in pinned)
    assert (8, 4) in si.REACHABLE_ARNOLDI and (8, 4) not in si.REACHABLE_CHEBY
    assert len(si.COMPILED) == 21 and len(si.REACHABLE_CHEBY) == 14 and len(si.REACHABLE_ARNOLDI) == 15

    covered = {"cheby": {}, "arnoldi": {}}
    for c in si.CASES:
        A = c.build()
        lens = np.diff(A.indptr)
        assert A.shape == (c.n, c.n) and lens.max() == c.maxrow and c.n <= 1025, c.name
        assert abs(A - A.getH()).max() == 0, c.name          # Hermitian: the packed device format takes it
        m = si.arnoldi_columns(c.n)
        for nops in (1, 2, 5):                               # (the terms of a lazy sum share the pattern: same plan)
            assert si.cheby_plan(c.n, A.nnz, c.maxrow, nops) == c.cheby, c.name
        assert si.arnoldi_plan(c.n, A.nnz, c.maxrow, m) == c.arnoldi, c.name
        # the library's plan for the slot count the gate ends up with
        for plan in (c.cheby, c.arnoldi):
            if plan:
                slots = si.SLOTS if plan[1] * plan[2] <= si.SLOTS else si.SLOTS_WIDE
                assert L.small_plan(c.n, c.maxrow, slots) == plan, c.name
                if slots == si.SLOTS_WIDE:
                    assert L.small_plan(c.n, c.maxrow, si.SLOTS) is None, c.name
        ragged = c.name.endswith("-ragged")
        if ragged:
            assert np.sum(lens == 0) >= 1 or c.n < 9, c.name
            assert c.n % (si.THREADS // (c.arnoldi[0])) != 0, c.name
        for kind, plan in (("cheby", c.cheby), ("arnoldi", c.arnoldi)):
            if plan:
                covered[kind].setdefault(plan[1:], set()).add("ragged" if ragged else "uniform")
        assert c.name.startswith(f"e{c.arnoldi[1]}r{c.arnoldi[2]}-"), c.name      # a case is named after its instance
    for kind, pinned in (("cheby", si.REACHABLE_CHEBY), ("arnoldi", si.REACHABLE_ARNOLDI)):
        assert sorted(covered[kind]) == pinned, (kind, sorted(covered[kind]))
        assert all(v == {"uniform", "ragged"} for v in covered[kind].values()), covered[kind]
