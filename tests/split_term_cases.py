"""The inputs and the assertion helpers of the split-term tests, on the host alone (plain data and NumPy):
tests/test_gpu_split_term.py runs them through qp_split_create / qp_cheby_term_split, tests/test_split_term_cases_host.py (no GPU)
shows with a host emulation that the same helpers reject a wrong slot, a block taken twice or not at all and a store past the slab.

partition(A, send_rows) restates, from the SciPy matrix alone, what qp_split_create (its partition: csrc/cheby_plan.cpp, plan_split) must decide about the
64-row blocks of a rank's local rows (nrows x ncols, a column >= nrows being a ghost column: an entry of another rank's rows):

    boundary   a block with a send row, or with a row whose largest column is a ghost column
    adjacent   an interior block one of whose rows reads a row of a boundary block, or one of whose rows a boundary block reads
    plain      every other interior block
    interior   the order of the interior launch: plain blocks, then adjacent ones, each ascending -- only the adjacent ones wait
               for the boundary launch of the term before
    mirror     per boundary block (ascending) and lane: the slab slot of the row (its index in send_rows), -1 for a row that is not
               sent or lies beyond nrows; one -1 more at the end

The send sets are functions of (nrows, G), G the ghost width of the rectangular cases (cheby_term_cases.G)."""
import dataclasses
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cheby_term_cases import GUARD, JUNK, SENTINEL, same_bits  # noqa: E402

RB = 64
SLAB_TAIL = 64          # elements of the slab buffer behind the nsend that are used

# the operators of the split tests: the row-block cases of cheby_term_cases, square and rectangular
FAMILIES = ("rbcsr-shallow", "rbcsr-complex", "rbcsr-real", "rbcsr-far", "coded-uniform", "coded-sigma_y", "hrb-scattered", "hrb-z16",
            "walk-5point")
CASE_NAMES = [f + sfx for f in FAMILIES for sfx in ("", "-rect")]
CHAIN_CASE_NAMES = ["rbcsr-complex-rect", "coded-uniform-rect", "hrb-z16-rect", "walk-5point-rect"]
# (every row block of the first two reads a ghost column: the chain of these has interior blocks in the rbcsr and coded kernels too)
CHAIN_CASE_NAMES_WITH_INTERIOR = ["rbcsr-shallow-rect", "rbcsr-complex", "coded-uniform"]


@dataclasses.dataclass
class Partition:
    nrows: int
    nblocks: int
    boundary: np.ndarray      # ascending
    adjacent: np.ndarray      # ascending
    plain: np.ndarray         # ascending
    interior: np.ndarray      # plain, then adjacent
    mirror: np.ndarray        # 64 * len(boundary) + 1
    send_rows: np.ndarray

    @property
    def n_boundary(self):
        return len(self.boundary)

    @property
    def n_interior(self):
        return len(self.interior)


def mirror_of(boundary, send_rows, nrows):
    slot = np.full(nrows, -1, dtype=np.int64)
    slot[send_rows] = np.arange(len(send_rows))
    mirror = np.full(RB * len(boundary) + 1, -1, dtype=np.int64)
    for k, b in enumerate(boundary):
        rows = np.arange(RB * b, min(RB * (b + 1), nrows))
        mirror[RB * k: RB * k + len(rows)] = slot[rows]
    return mirror


def partition(A, send_rows):
    A = A.tocsr()
    nrows, nblocks = A.shape[0], (A.shape[0] + RB - 1) // RB
    send_rows = np.asarray(send_rows, dtype=np.int64).reshape(-1)
    assert len(np.unique(send_rows)) == len(send_rows) and (len(send_rows) == 0 or (send_rows.min() >= 0 and send_rows.max() < nrows))
    row_of = np.repeat(np.arange(nrows), np.diff(A.indptr))
    col = A.indices.astype(np.int64)
    is_b = np.zeros(nblocks, dtype=bool)
    is_b[send_rows // RB] = True
    is_b[row_of[col >= nrows] // RB] = True
    local = col < nrows
    rblk, cblk = row_of[local] // RB, col[local] // RB
    adj = np.zeros(nblocks, dtype=bool)
    adj[cblk[is_b[rblk] & ~is_b[cblk]]] = True      # a boundary row gathers from the block
    adj[rblk[~is_b[rblk] & is_b[cblk]]] = True      # a row of the block gathers from a boundary row
    blocks = np.arange(nblocks)
    boundary, adjacent, plain = blocks[is_b], blocks[~is_b & adj], blocks[~is_b & ~adj]
    return Partition(nrows, nblocks, boundary, adjacent, plain, np.concatenate([plain, adjacent]),
                     mirror_of(boundary, send_rows, nrows), send_rows)


# ---- send sets ------------------------------------------------------------------------------------------------------------------

def _none(nrows, G):
    return np.zeros(0, dtype=np.int64)


def _ends(nrows, G):
    """the first and the last 40 rows: a contiguous prefix and suffix, what qp_split_create requires for a walk plan"""
    return np.concatenate([np.arange(40), np.arange(nrows - 40, nrows)])


def _scattered(nrows, G):
    """row 7 and the last row of every second block (63, 191, 319, ...: exactly one send row in the blocks 2, 6, 10, ...), a second
    row (lane 10) in the blocks 4, 8, ...; the odd blocks have none.  Row 7 first, the others from the top down: the slot neither
    rises nor falls with the row."""
    rows = [64 * k + 63 for k in range(0, (nrows + 63) // 64, 2) if 64 * k + 63 < nrows]
    rows += [64 * k + 10 for k in range(4, (nrows + 63) // 64, 4) if 64 * k + 10 < nrows]
    return np.array([7] + sorted(rows, reverse=True), dtype=np.int64)


def _last_row(nrows, G):
    return np.array([nrows - 1], dtype=np.int64)


def _all(nrows, G):
    """every row, DESCENDING: the slot is not monotone in the row, and no block is interior"""
    return np.arange(nrows - 1, -1, -1)


def _one_interior(nrows, G):
    """lane 1 of every block but the middle one"""
    nblocks = (nrows + 63) // 64
    return np.array([64 * k + 1 for k in range(nblocks) if k != nblocks // 2 and 64 * k + 1 < nrows], dtype=np.int64)


SEND_SETS = {"none": _none, "ends": _ends, "scattered": _scattered, "last-row": _last_row, "all": _all, "one-interior": _one_interior}


def chain_send_rows(nrows, G):
    """exactly G rows without order, drawn from the first two and the last two row blocks: what a rank sends is as long as a ghost
    range, and the blocks in between stay interior (where no row of theirs reads a ghost column)"""
    nblocks = (nrows + 63) // 64
    pool = np.concatenate([np.arange(0, 128), np.arange(64 * (nblocks - 2), nrows)])
    assert nblocks >= 5 and len(pool) >= G
    return np.random.default_rng(1234 + nrows).permutation(pool)[:G].astype(np.int64)


# ---- assertion helpers ------------------------------------------------------------------------------------------------------------

def check_partition_counts(part, n_boundary, n_interior, walk=None, what=""):
    """The getters of a split (qp_split_info, qp_split_walk_info) against the expected partition.  ``walk``: the walk_info dict;
    a valid plan needs a boundary that is a prefix and a suffix of the blocks, walks a range inside the interior and leaves
    n_interior - (end - first) edge blocks."""
    assert (n_boundary, n_interior) == (part.n_boundary, part.n_interior), (what, n_boundary, n_interior, part.n_boundary, part.n_interior)
    assert n_boundary + n_interior == part.nblocks, what
    if walk is None or not walk["valid"]:
        return
    first, end = walk["first_block"], walk["end_block"]
    inside = set(part.interior.tolist())
    contiguous = part.n_interior > 0 and part.interior.max() - part.interior.min() + 1 == part.n_interior
    assert contiguous, f"{what}: a walk plan although the interior is no contiguous run of blocks"
    assert first < end and all(b in inside for b in range(first, end)), (what, walk)
    assert walk["edge_blocks"] == n_interior - (end - first), (what, walk)
    # no walked block is adjacent to a boundary block: those wait, the walk does not
    assert not (set(range(first, end)) & set(part.adjacent.tolist())), (what, walk)


def check_slab(slab_with_guards, vout, send_rows, what=""):
    """The slab buffer as downloaded, GUARD sentinels either side of nsend + SLAB_TAIL elements that held JUNK before the call:
    slab[i] has the bits of vout[send_rows[i]], the tail and the sentinels are untouched; vout None (a form without vout, or a
    call without slab): nothing was written at all."""
    nsend = len(send_rows)
    got = np.asarray(slab_with_guards)
    assert len(got) == nsend + SLAB_TAIL + 2 * GUARD, what
    assert same_bits(got[:GUARD], np.full(GUARD, SENTINEL)), f"{what}: a store BEFORE the slab"
    assert same_bits(got[GUARD + nsend + SLAB_TAIL:], np.full(GUARD, SENTINEL)), f"{what}: a store BEHIND the slab buffer"
    body = got[GUARD:GUARD + nsend]
    tail = got[GUARD + nsend:GUARD + nsend + SLAB_TAIL]
    assert same_bits(tail, np.full(SLAB_TAIL, JUNK)), f"{what}: a store past the end of the slab (index >= nsend)"
    if vout is None:
        assert same_bits(body, np.full(nsend, JUNK)), f"{what}: the slab was written although the term has no vout"
        return
    want = np.asarray(vout)[np.asarray(send_rows, dtype=np.int64)]
    bad = np.nonzero(body.view(np.uint64).reshape(-1, 2) != np.ascontiguousarray(want).view(np.uint64).reshape(-1, 2))[0]
    assert bad.size == 0, f"{what}: {bad.size} slab slots do not hold their send row, first slot {int(bad[0])} (row {int(send_rows[bad[0]])})"
