"""Reference of the lazy operator sum -- evaluate! on the device, operator_refresh of csrc/engine_operator.hip: the stored values
become  scale * (sum of the drift planes + sum_l c_l * control planes)  -- the bound the GPU tests hold every stored position to
(tests/test_gpu_lazy_sum.py), the same sum in the very order the kernels form it, and the mutations that show both checks can
fail (tests/test_lazy_sum_ref.py).  NumPy and `fractions` only; nothing of the library or of oracle/.

Effective coefficients, as operator_refresh forms them on the host: with drift = nops - ncoeffs,

    eff_l = scale                        l <  drift
    eff_l = scale * coeffs[l - drift]    l >= drift          (one complex product in double precision)

combined_ref(planes, eff), in np.clongdouble (80-bit here), per stored position p of the union pattern (planes[l][p] = a_l[p], zero
where term l has no entry):

    v_p = sum_l eff_l a_l[p]        M_p = sum_l |eff_l| |a_l[p]|        T_p = number of terms with a_l[p] != 0

and the acceptance test  |got_p - v_p| <= (1.5 T_p + 2) 2^-52 M_p.  Nothing in it is measured; u = 2^-53 is the unit roundoff:

  the sum        cfma of csrc/kernel_common.h is four explicit fma's, two per component (x: c.re a.re, then -c.im a.im; y: c.re a.im,
                 then c.im a.re), and combine_planes_kernel / sparse_planes_update_kernel add the terms in ascending term index.  An
                 FMA whose product is zero returns its addend: a term that does not touch the position rounds nothing.  So a
                 component takes at most 2 T_p roundings, each at most u times a partial sum of modulus at most M_p: per
                 component |d| <= 2 T u M, in modulus sqrt(2) as much: 2 sqrt(2) T u M = 1.42 T 2^-52 M.
  scale * coeff  one complex product on the host, at most sqrt(8) u relative per term (the reference multiplies the two doubles
                 in extended precision): 1.42 2^-52 M more.
                 => |d v_p| <= (1.42 T_p + 1.42) 2^-52 M_p, rounded up: (1.5 T_p + 2) 2^-52 M_p.
  (second-order terms are below 1e-13 of this for T < 1e3.)  A position that no term touches has M_p = 0 and must come back as
  exactly zero -- the pads of a row block, the zeros that complete a lattice or a dense operator: asserted, not skipped.

chain_exact(planes, eff, positions) is the same sum as the kernel forms it: x = y = 0, then for l = 0, 1, .. in ascending order

    x = fma(c.re, a.re, x);  x = fma(-c.im, a.im, x);  y = fma(c.re, a.im, y);  y = fma(c.im, a.re, y)        (c = eff_l, a = a_l[p])

with an exact FMA, float(Fraction(a) * Fraction(b) + Fraction(c)) -- the conversion of a Fraction rounds correctly (fma_exact
computes the same quotient from float.as_integer_ratio without the gcd's; the host test compares the two).  The library's claims
rest on this order: the sparse-control update "runs in the summation order of combine_planes_kernel" from a base that is the chain
of the earlier terms, and a chunk boundary of launch_combine_planes stores and reloads a double, which changes nothing.  So the
chain is expected to hold BIT FOR BIT at every term count, compared with == (a signed zero is no difference).  The comparison
applies to moves whose scale * coeff is exact (product_is_exact: a real scale that is a power of two with real coefficients, or
any coefficients at scale 1); for a general complex scale only the bound applies -- whether the host product is contracted into
an FMA is not pinned.

A Hermitian-packed operator hands the lower triangle back (get_csr) as conjugates of the stored upper entries.  With REAL
coefficients the chain of conjugated values is the conjugate of the chain (c.im = 0: the second FMA of x and of y adds a zero, and
y = fma(c.re, -a.im, -y') = -fma(c.re, a.im, y')), so the emulation on the CSR values as given is still exact there.

MUTATIONS are deliberately WRONG versions of all this (the checker of the checker): each, except the order one, must put a position
beyond the bound on every case it applies to; the order one must change bits."""
from fractions import Fraction

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
EPS = LD(2.0) ** -52
CHUNK = 32          # csrc/device.h: kCoefBlock, the coefficients one launch carries
assert np.finfo(LD).nmant >= 63, "the reference needs an extended-precision long double"

# wrong effective coefficients / wrong sums / a stale real copy / the other order
MUTATIONS = ("drop_term_32", "second_chunk_overwrites", "second_chunk_first_coefs", "border_up", "border_down", "drift_unscaled",
             "conj_coeff", "stale_real_copy", "descending_order")
CHUNK_MUTATIONS = ("drop_term_32", "second_chunk_overwrites", "second_chunk_first_coefs")
EFF_MUTATIONS = ("border_up", "border_down", "drift_unscaled", "conj_coeff")


def product_is_exact(scale, coeffs):
    """Is every scale * coeffs[j] exact in double precision by the rule of the module docstring?"""
    scale = complex(scale)
    if scale == 1.0:
        return True
    m = abs(scale.real)
    pow2 = scale.imag == 0.0 and m > 0 and np.frexp(m)[0] == 0.5
    return bool(pow2 and np.all(np.asarray(coeffs, dtype=np.complex128).imag == 0.0))


def effective(nops, ncoeffs, coeffs, scale, extended=False, mutation=None):
    """eff_l of the header.  extended: the products in clongdouble (the reference of the bound); otherwise in complex128, one
    product each as on the host (the chain's input).  ``mutation``: one of EFF_MUTATIONS."""
    assert mutation is None or mutation in EFF_MUTATIONS, mutation
    coeffs = np.asarray(coeffs, dtype=np.complex128).reshape(-1)
    assert len(coeffs) == ncoeffs and 0 <= ncoeffs <= nops
    drift = nops - ncoeffs
    if mutation == "conj_coeff":
        coeffs = np.conj(coeffs)
    padded = np.concatenate([coeffs, [1.0]])          # what an off-by-one border reads behind the last coefficient
    if mutation == "border_up":
        drift += 1
    if mutation == "border_down":
        drift -= 1
    typ = CLD if extended else np.complex128
    eff = np.empty(nops, dtype=typ)
    for l in range(nops):
        s = typ(1.0) if (mutation == "drift_unscaled" and l < drift) else typ(complex(scale))
        eff[l] = s if l < drift else s * typ(padded[l - drift])
    return eff


def combined_ref(planes, eff, mutation=None):
    """(v, M, T) of the header for planes (L x P complex128) and eff (L).  ``mutation``: one of CHUNK_MUTATIONS."""
    assert mutation is None or mutation in CHUNK_MUTATIONS, mutation
    planes = np.asarray(planes, dtype=np.complex128)
    L, P = planes.shape
    assert len(eff) == L
    e = np.asarray(eff, dtype=CLD)
    v, M, T = np.zeros(P, dtype=CLD), np.zeros(P, dtype=LD), np.zeros(P, dtype=np.int64)
    for l in range(L):
        a = planes[l].astype(CLD)
        M += np.abs(e[l]) * np.abs(a)
        T += planes[l] != 0
        if mutation == "drop_term_32" and l == CHUNK:
            continue
        if mutation == "second_chunk_overwrites" and l == CHUNK:
            v[:] = 0
        c = e[l - CHUNK] if (mutation == "second_chunk_first_coefs" and CHUNK <= l < 2 * CHUNK) else e[l]
        v += c * a
    return v, M, T


def bound(M, T):
    return (LD(1.5) * np.asarray(T, dtype=LD) + 2) * EPS * np.asarray(M, dtype=LD)


def beyond(got, v, M, T):
    """positions of ``got`` beyond the bound around v (a position without magnitude must be exactly zero: its bound is zero)"""
    err = np.abs(np.asarray(got, dtype=CLD) - v)
    return np.nonzero(~(err <= bound(M, T)))[0]


def check_positions(got, v, M, T, what, quiet=False):
    """Every position under the bound, the untouched ones exactly zero; returns (and prints, for -s) the largest err / bound."""
    got = np.asarray(got, dtype=np.complex128)
    err = np.abs(got.astype(CLD) - v)
    bnd = bound(M, T)
    zero = np.asarray(M) == 0
    nz = np.nonzero(zero & (got != 0))[0]
    assert nz.size == 0, f"{what}: {nz.size} positions that no term touches are not exactly zero, first {int(nz[0])}: {got[nz[0]]}"
    ratio = np.zeros(len(got), dtype=LD)
    ratio[~zero] = err[~zero] / bnd[~zero]
    worst = int(np.argmax(ratio)) if len(ratio) else 0
    top = float(ratio[worst]) if len(ratio) else 0.0
    if not quiet:
        print(f"[lazy sum] {what}: max err/bound {top:.4f} at position {worst} (T = {int(T[worst]) if len(T) else 0})")
    bad = np.nonzero(~(err <= bnd))[0]
    assert bad.size == 0, (f"{what}: {bad.size} positions beyond the bound, first {int(bad[0])} (T = {int(T[bad[0]])}): "
                           f"err {float(err[bad[0]]):.3e} bound {float(bnd[bad[0]]):.3e}")
    return top


def fma_fraction(a, b, c):
    """the definition: a * b + c, rounded once"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fma_exact(a, b, c):
    """fma_fraction without the gcd's: the denominators of float.as_integer_ratio are powers of two, and the true division of two
    Python integers rounds correctly."""
    if a == 0.0 or b == 0.0:
        return c                    # (an exact zero product: the addend comes back; compared with ==, its sign does not matter)
    na, da = a.as_integer_ratio()
    nb, db = b.as_integer_ratio()
    nc, dc = c.as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def chain_exact(planes, eff, positions, descending=False):
    """The kernels' sum at ``positions`` (complex128): the FMA chain of the header, ascending term index (descending: the mutation)."""
    planes = np.asarray(planes, dtype=np.complex128)
    eff = np.asarray(eff, dtype=np.complex128)
    L = planes.shape[0]
    order = range(L - 1, -1, -1) if descending else range(L)
    cre, cim = [float(z.real) for z in eff], [float(z.imag) for z in eff]
    out = np.empty(len(positions), dtype=np.complex128)
    for i, p in enumerate(positions):
        col = planes[:, p]
        x = y = 0.0
        for l in order:
            ar, ai = float(col[l].real), float(col[l].imag)
            if ar == 0.0 and ai == 0.0:
                continue
            x = fma_exact(cre[l], ar, x)
            x = fma_exact(-cim[l], ai, x)
            y = fma_exact(cre[l], ai, y)
            y = fma_exact(cim[l], ar, y)
        out[i] = complex(x, y)
    return out


def sample_positions(planes, block_of_position, seed, count=64):
    """``count`` positions fixed by seed: the first and the last, one of every row block, for every term one that it touches, the
    rest drawn from the positions that some term touches."""
    planes = np.asarray(planes)
    L, P = planes.shape
    rng = np.random.default_rng(seed)
    pick = [0, P - 1]
    block_of_position = np.asarray(block_of_position)
    for b in np.unique(block_of_position):
        pick.append(int(rng.choice(np.nonzero(block_of_position == b)[0])))
    for l in range(L):
        t = np.nonzero(planes[l] != 0)[0]
        if t.size:
            pick.append(int(rng.choice(t)))
    pick = list(dict.fromkeys(pick))
    live = np.setdiff1d(np.nonzero(np.any(planes != 0, axis=0))[0], pick)
    if len(pick) < count and live.size:
        pick += [int(p) for p in rng.choice(live, size=min(count - len(pick), live.size), replace=False)]
    return np.array(sorted(pick), dtype=np.int64)
