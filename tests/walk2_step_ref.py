"""Extended-precision reference of a WHOLE cheby! call (src/cheby.jl:171-211), the per-row error bound the GPU tests of the two-term
strip walk hold Psi to (tests/test_gpu_walk2_forms.py), the launches of a step restated from the prose of csrc/cheby_plan.h, the
coefficient sets that make every term count, and the mutations that show the bound can fail (tests/test_walk2_step_ref.py).
NumPy in np.clongdouble on top of tests/cheby_term_ref.py; nothing of the library or of oracle/ is imported.

The step.  beta = Delta / 2 + E_min, c = -2i / Delta (dt > 0) or 2i / Delta, phase = exp(-i beta dt) -- the three in DOUBLE
precision, as ChebyScalars (csrc/cheby_plan.h) forms them; the reference takes those doubles as given --

    v_0 = psi;   v_1 = c (H v_0 - beta v_0);   v_m = 2 c (H v_{m-1} - beta v_{m-1}) + v_{m-2}   (m = 2 .. nterms = n_coeffs - 1)
    Psi = phase sum_m a_m v_m

The launches.  One fused term per launch, or terms m and m + 1 in one pair launch (x = v_{m-1}, p = v_{m-2}; y = v_m, z = v_{m+1}).
Every third term counted from the last updates Psi's accumulator and folds the coefficients of the terms skipped before it
(include/qprop.h: qp_acc_defer); the first update needs v_0, which lives two terms only, so when the count from the last would
begin at term 3 the first term updates too.  A pair is taken from term 2 on whenever two terms are left and at most one of them
updates.  launch_table(nterms) states this; step_ref walks it -- y, z, the accumulator with its deferred coefficients -- so a
mutation can be wrong in ONE place of ONE kind of launch.

The bound.  Nothing in it is measured.  tests/cheby_term_ref.py bounds one fused term on exact operands: a computed
t_i is within b_i = (S_i + 12) 2^-52 T_i of the exact one, T_i = |c_m| (sum_j |a_ij| |x_j| + |beta| |x_i|) + |v0_i| (c_1 = c, c_m = 2 c
afterwards; no v0 in term 1).  The device's term m starts from ITS v_{m-1} and v_{m-2}, which carry the errors E_{m-1} and
E_{m-2}; the term is linear in them, so row by row

    E_0 = 0  (psi is uploaded as it is),    E_m = b_m + |c_m| (|H| E_{m-1} + |beta| E_{m-1}) + E_{m-2},    b_m from the T_m of the exact v

(b_m on the device's operands differs in second order: (S + 12) 2^-52 times the propagated part, below 1e-13 of it).  A pair launch
forms the same two terms with the same row sums and epilogues -- that is what bit-identity with the one-term launches asserts --
so the recurrence does not depend on the launch table.  The accumulator: whatever the schedule, Psi's row is built as
a_0 v_0 (one product), then one FMA per component and term, in rising m (qp_acc_defer: r = first; r += a_d2 v_{m-2}; r += a_d1
v_{m-1}; r += a t) -- nterms + 1 roundings, rounding j relative to the partial sum it produces, which is no larger than
M_j = sum_{k <= j} |a_k| (|v_k| + E_k): 0.5 each in units of 2^-52 M_j (one rounding per real component with a real coefficient:
the complex error is at most u |r|).  Stores of the accumulator between updates are exact.  The last update multiplies by the
phase: a cmul, 1.42 (cheby_term_ref), and the phase itself is a double-precision exp of the library's libm, known to the
reference only within an ulp per component: 2 more, both relative to M_nterms.  With |phase| = 1:

    bound_i = sum_{m >= 1} |a_m| E_m,i  +  2^-52 (0.5 sum_{j = 0}^{nterms} M_j,i  +  3.42 M_nterms,i)

The same expressions with 2^-63 for 2^-52 bound the error of this reference itself (its row sums add S products one by one in
80-bit arithmetic: S + 1 roundings, inside S + 12): 2^-11 of the double-precision bound.

The growth of E_m is the worst case of the recurrence, |2 c| (|H| + |beta|) + 1 by modulus per term; the device's errors do not
line up like that, so the measured err / bound is far below the 0.1 of a single term and falls with nterms.  A wrong operand on one
row still moves Psi by a multiple of an a_m v_m, of order one with the coefficient sets below.

Coefficient sets.  order_one_coeffs(nterms): nterms + 1 exact dyadic values k / 16, moduli in [0.5, 1.5], mixed signs -- every
term moves Psi by order one.  True Chebyshev coefficients fall to the truncation limit at the end of the series: a wrong y or z
in the last pairs, times such an a_m, stays inside the bound (tests/test_walk2_step_ref.py asserts this: bit-identity of Psi after
a physical step says little about the last third of the step).

Mutations (MUTATIONS): step references that a pair kernel could plausibly be.  They need the geometry of the walk
(Geometry: rows of the two-term region, the strip step g, d_max, K):
    z_from_x_on_halo     rows of a 64-row chunk outside its W = 64 - 2 d_max owned lanes hold x where z's near gathers expect y
    far_z_one_step_late  the far matrix values of z's row sum are those of the row one strip step further down
    swap_deferred_2nd    a_d1 / a_d2 exchanged in the second epilogue of a pair (with one deferred vector: its coefficient is lost)
    a0_on_x_in_U1f       the first update inside a pair, [U1f,S]: a_0 times x = v_1 instead of p = v_0
    z_stored_last        the last term's z is stored although the term has no vout -- into the one output vector the launch does
                         have, y's, on the rows the walk owns, before the edge follow-up gathers y
    edge_2nd_from_x      the follow-up launch of the edge blocks gathers x instead of y
"""
import dataclasses

import numpy as np
import scipy.sparse as sp

import cheby_term_ref as R

LD, CLD, EPS, K_TERM = R.LD, R.CLD, R.EPS, R.K
EPS_LD = LD(2.0) ** -63
MUTATIONS = ("z_from_x_on_halo", "far_z_one_step_late", "swap_deferred_2nd", "a0_on_x_in_U1f", "z_stored_last", "edge_2nd_from_x")
# the mutations that can sit in the LAST pair of a step alone
LATE_MUTATIONS = ("z_from_x_on_halo", "far_z_one_step_late", "swap_deferred_2nd", "z_stored_last", "edge_2nd_from_x")


# ---- scalars and coefficients ------------------------------------------------------------------------------------------------

def scalars(Delta, E_min, dt):
    """(c, beta, phase) in double precision: src/cheby.jl:156-162, :211"""
    Delta, E_min, dt = float(Delta), float(E_min), float(dt)
    beta = Delta / 2 + E_min
    c = complex(0.0, -2.0) / Delta if dt > 0 else complex(0.0, 2.0) / Delta
    return c, beta, complex(np.exp(-1j * beta * dt))


def order_one_coeffs(nterms):
    """nterms + 1 dyadic values k / 16 with 8 <= |k| <= 24: exact in every format, no two neighbours equal, signs mixed"""
    rng = np.random.default_rng(1000 + nterms)
    k = rng.integers(8, 25, nterms + 1)
    for i in range(1, nterms + 1):                   # (a swap of two neighbours must show)
        if k[i] == k[i - 1]:
            k[i] = 8 + (k[i] - 8 + 5) % 17
    sign = np.where(rng.integers(0, 2, nterms + 1) == 1, 1.0, -1.0)
    sign[0], sign[1] = 1.0, -1.0
    a = sign * k / 16.0
    assert np.all(np.abs(a) >= 0.5) and np.all(np.abs(a) <= 1.5) and np.all(np.abs(a[1:]) != np.abs(a[:-1]))
    return a


ORDER_ONE_NTERMS = tuple(range(3, 15))


# ---- the launches of a step ---------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class TermForm:
    m: int
    update: bool      # does the term's epilogue write the accumulator?
    n_defer: int      # ... with how many skipped terms folded in
    first: bool       # the first update of the step (the accumulator does not exist yet: a_0 enters here)
    last: bool        # the last term: no vout, the phase

    @property
    def name(self):
        return (f"U{self.n_defer}" + ("f" if self.first else "") if self.update else "S") + ("L" if self.last else "")


def updating_terms(nterms, defer=True):
    if not defer:
        return set(range(1, nterms + 1))
    upd = set(range(nterms, 0, -3))
    if min(upd) == 3:
        upd.add(1)
    return upd


def term_forms(nterms, defer=True):
    upd = updating_terms(nterms, defer)
    forms, before = [], 0
    for m in range(1, nterms + 1):
        if m in upd:
            forms.append(TermForm(m, True, m - before - 1, before == 0, m == nterms))
            before = m
        else:
            forms.append(TermForm(m, False, 0, False, m == nterms))
    assert all(f.n_defer <= 2 for f in forms) and forms[-1].update
    return forms


def launch_table(nterms, defer=True, pairs=True):
    """the launches of a step, in order: tuples of one TermForm (a one-term launch) or two (a pair)"""
    forms = term_forms(nterms, defer)
    out, m = [], 1
    while m <= nterms:
        if pairs and nterms >= 3 and m > 1 and m + 1 <= nterms and not (forms[m - 1].update and forms[m].update):
            out.append((forms[m - 1], forms[m]))
            m += 2
        else:
            out.append((forms[m - 1],))
            m += 1
    return out


def table_text(table):
    return " ".join(f"[{l[0].name},{l[1].name}]" if len(l) == 2 else l[0].name for l in table)


def pair_forms(table):
    return {(l[0].name, l[1].name) for l in table if len(l) == 2}


def n_pairs(table):
    return sum(1 for l in table if len(l) == 2)


# ---- the geometry a mutation needs --------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Geometry:
    """rows [zb, ze) of the two-term region (whole 64-row blocks; everything else is an edge block), the strip step g, the largest
    near distance and the far reach of the lattice"""
    n: int
    g: int
    K: int
    dmax: int
    zb: int
    ze: int

    @property
    def W(self):
        return 64 - 2 * self.dmax

    def region(self):
        m = np.zeros(self.n, dtype=bool)
        m[self.zb:self.ze] = True
        return m

    def halo_entries(self, H):
        """H restricted to the entries (i, j) of region rows whose near neighbour j lies, in the 64-lane chunk that owns row i,
        outside the W owned lanes"""
        Hc = H.tocoo()
        i, j = Hc.row.astype(np.int64), Hc.col.astype(np.int64)
        lane = (i - self.zb) % self.g % self.W + self.dmax
        near = (np.abs(j - i) <= self.dmax) & (j != i)
        lane_j = lane + (j - i)
        keep = self.region()[i] & near & ((lane_j < self.dmax) | (lane_j >= 64 - self.dmax))
        return sp.csr_matrix((Hc.data[keep], (i[keep], j[keep])), shape=H.shape)

    def late_far_values(self, H):
        """H with the far entries (|j - i| a multiple of g) of the region's rows replaced by those of row i + g"""
        Hs = H.tocsr().copy()
        Hs.sort_indices()
        n = self.n
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(Hs.indptr))
        cols = Hs.indices.astype(np.int64)
        keys = rows * n + cols
        assert np.all(np.diff(keys) > 0)
        far = self.region()[rows] & (np.abs(cols - rows) >= self.g) & (np.abs(cols - rows) % self.g == 0) & (np.abs(cols - rows) <= self.K * self.g)
        src = ((rows[far] + self.g) % n) * n + (cols[far] + self.g) % n
        pos = np.searchsorted(keys, src)
        assert np.all(keys[pos] == src), "a lattice: the row one strip step down has the same far entries"
        data = Hs.data.copy()
        data[far] = Hs.data[pos]
        return sp.csr_matrix((data, Hs.indices, Hs.indptr), shape=H.shape)


# ---- the step -------------------------------------------------------------------------------------------------------------------

class Step:
    """what step_ref returns: v[m], T[m] (m >= 1), Psi, the launch table it walked"""


def _apply(H, x):
    return R.row_sums(H, x)[0]


def step_ref(H, psi, a, Delta, E_min, dt, defer=True, mutation=None, geom=None, where="all"):
    """Psi and every v_m of cheby!(psi, H, dt) with the coefficients ``a``, in clongdouble, walked launch by launch through
    launch_table.  ``mutation``: one of MUTATIONS, applied in every pair launch it can sit in (``where`` = "all") or in the last
    pair launch alone ("last"); needs ``geom``.  Returns a Step; Step.applied counts the launches the mutation changed."""
    assert mutation is None or (mutation in MUTATIONS and geom is not None), mutation
    a = np.asarray(a, dtype=np.float64)
    nterms = len(a) - 1
    c, beta, phase = scalars(Delta, E_min, dt)
    c1, c2, betaL, phaseL = CLD(c), CLD(2 * c), LD(beta), CLD(phase)
    aL = a.astype(LD)
    H = H.tocsr()
    v = [np.asarray(psi, dtype=CLD)]
    table = launch_table(nterms, defer)
    pair_launches = [l for l in table if len(l) == 2]
    out = Step()
    out.table, out.applied = table, 0
    acc = None
    region = geom.region() if geom is not None else None
    H_halo = geom.halo_entries(H) if mutation == "z_from_x_on_halo" else None
    H_late = geom.late_far_values(H) if mutation == "far_z_one_step_late" else None

    def term(x, p, cm):
        t = cm * (_apply(H, x) - betaL * x)
        return t if p is None else t + p

    def update(f, t, x, p, mut=None):
        """the epilogue of an updating term: qp_acc_defer"""
        nonlocal acc
        a_d1 = aL[f.m - 1] if f.n_defer >= 1 else LD(0)
        a_d2 = aL[f.m - 2] if f.n_defer == 2 else LD(0)
        if mut == "swap_deferred_2nd":
            a_d1, a_d2 = a_d2, a_d1
        if f.first:
            r = aL[0] * (p if f.n_defer == 1 else x)
            if mut == "a0_on_x_in_U1f":
                r = aL[0] * x
        else:
            r = acc.copy()
        if f.n_defer == 2:
            r = r + a_d2 * p
        if f.n_defer >= 1:
            r = r + a_d1 * x
        acc = r + aL[f.m] * t

    for launch in table:
        f = launch[0]
        m = f.m
        x, p = v[m - 1], (v[m - 2] if m >= 2 else None)
        if len(launch) == 1:
            t = term(x, p, c1 if m == 1 else c2)
            if f.update:
                update(f, t, x, p)
            v.append(t)
            continue
        f2 = launch[1]
        mut = mutation if (where == "all" or launch is pair_launches[-1]) else None
        y = term(x, p, c2)
        if f.update:
            applies = mut == "a0_on_x_in_U1f" and f.first and f.n_defer == 1
            out.applied += applies
            update(f, y, x, p, mut if applies else None)
        z = term(y, x, c2)
        if mut == "z_from_x_on_halo":
            z = c2 * (_apply(H, y) + _apply(H_halo, x - y) - betaL * y) + x
            out.applied += 1
        elif mut == "far_z_one_step_late":
            z = np.where(region, c2 * (_apply(H_late, y) - betaL * y) + x, z)
            out.applied += 1
        elif mut == "edge_2nd_from_x":
            z = np.where(region, z, c2 * (_apply(H, x) - betaL * x) + x)
            out.applied += 1
        elif mut == "z_stored_last" and f2.last:
            y_seen = np.where(region, z, y)               # what the edge follow-up gathers; its row-local operand y_i is its own
            z = np.where(region, z, c2 * (_apply(H, y_seen) - betaL * y) + x)
            out.applied += 1
        if f2.update:
            applies = mut == "swap_deferred_2nd" and f2.n_defer >= 1
            out.applied += applies
            update(f2, z, y, x, mut if applies else None)
        v.extend([y, z])
    out.v = v
    out.Psi = phaseL * acc
    return out


def magnitudes(H, v, Delta, E_min, dt):
    """T_m of cheby_term_ref for m = 1 .. nterms (index 0: None)"""
    c, beta, _ = scalars(Delta, E_min, dt)
    T = [None]
    for m in range(1, len(v)):
        x = v[m - 1]
        cm = abs(c) * (1 if m == 1 else 2)
        T.append(LD(cm) * (R.row_sums(H, x)[1] + LD(abs(beta)) * np.abs(x)) + (np.abs(v[m - 2]) if m >= 2 else 0))
    return T


def step_bound(H, S, v, a, Delta, E_min, dt, eps=EPS):
    """(bound on |Psi_device - Psi| per row, [E_m]) as derived in the module docstring; ``eps``: 2^-52 for the device, EPS_LD for this
    reference's own arithmetic"""
    c, beta, phase = scalars(Delta, E_min, dt)
    a = np.abs(np.asarray(a, dtype=np.float64)).astype(LD)
    nterms = len(a) - 1
    assert len(v) == nterms + 1
    T = magnitudes(H, v, Delta, E_min, dt)
    S = np.asarray(S, dtype=LD)
    absH = abs(H.tocsr())
    E = [np.zeros(len(v[0]), dtype=LD)]
    for m in range(1, nterms + 1):
        assert np.all(T[m] > 0), "a row without magnitude: the case must have nonzero operands on every row"
        cm = LD(abs(c) * (1 if m == 1 else 2))
        prop = cm * (R.row_sums(absH, E[m - 1])[1] + LD(abs(beta)) * E[m - 1]) + (E[m - 2] if m >= 2 else 0)
        E.append((S + K_TERM) * eps * T[m] + prop)
    M = np.zeros(len(v[0]), dtype=LD)
    terms = np.zeros(len(v[0]), dtype=LD)
    roundings = np.zeros(len(v[0]), dtype=LD)
    for m in range(nterms + 1):
        M = M + a[m] * (np.abs(v[m]) + E[m])
        terms = terms + a[m] * E[m]
        roundings = roundings + LD(0.5) * M
    return LD(abs(phase)) * (terms + eps * (roundings + LD(3.42) * M)), E


def check_rows(got, ref, bound, what, quiet=False):
    """Every row of Psi under the bound; returns (and prints, for -s) the largest err / bound."""
    err = np.abs(np.asarray(got, dtype=CLD) - ref)
    ratio = err / bound
    worst = int(np.argmax(ratio))
    if not quiet:
        print(f"[step rows] {what}: max err/bound {float(ratio[worst]):.5f} at row {worst} (block {worst >> 6}, lane {worst & 63})")
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rows beyond the bound, first {int(bad[0])} (block {int(bad[0]) >> 6}, lane {int(bad[0]) & 63}): "
                           f"err {float(err[bad[0]]):.3e} bound {float(bound[bad[0]]):.3e}")
    return float(ratio[worst])
