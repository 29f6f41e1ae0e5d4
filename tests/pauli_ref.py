"""Extended-precision reference for the Pauli-string operator (csrc/engine_pauli.hip) that shares nothing with the kernel's mask
arithmetic: ``sum_t a_t P_t x`` by tensor-axis operations on ``x.reshape((2,) * n)`` (qubit q is axis n - 1 - q: bit q of the row
index).  X is ``np.flip`` along the axis, Z multiplies the axis by [1, -1], Y is a flip times [-1j, 1j] -- no XOR, no popcount and no
Kronecker matrix (synth.pauli_sum_matrix takes 20 s for the 1100 strings this applies in a fraction of a second).

A string acts as  P x = W * flip_X(x)  with W the outer product of its per-axis factors ([1, -1] for Z, [-1j, 1j] for Y, 1 otherwise;
factors on different axes commute with the flips of the others), so the strings that flip the same axes share one flip: their W are
summed first (exact products of the amplitudes with +-1 / +-i, added in the working precision).  ``strings`` is what lib.PauliOperator
takes for one term of the lazy sum: [(amplitude, (xmask, zmask)), ...].  Test infrastructure, host only."""
import numpy as np


def _bits(mask, n):
    return [q for q in range(n) if (int(mask) >> q) & 1]


def _real_of(dtype):
    return np.zeros(1, dtype=dtype).real.dtype


class PauliRef:
    """``sum_t a_t P_t`` of an n-qubit register.  ``H @ x`` evaluates in extended precision and returns complex128 -- the form
    oracle.qp_oracle.cheby / newton take as ``H``; ``apply`` keeps the working precision, ``abs_apply`` is the row-wise magnitude."""

    def __init__(self, n, strings, dtype=np.clongdouble):
        self.n, self.dtype = int(n), dtype
        self.shape = (1 << self.n, 1 << self.n)
        self.nstrings = len(strings)
        n = self.n
        z = np.array([1, -1], dtype=dtype)
        y = np.array([-1j, 1j], dtype=dtype)
        groups = {}       # flipped axes -> [W (summed over the group's strings), sum |a_t|]
        for amp, (xm, zm) in strings:
            xq, zq = _bits(xm, n), _bits(zm, n)
            w = np.full((1,) * n, dtype(amp), dtype=dtype)      # (an extended-precision amplitude keeps its bits)
            for q in sorted(set(xq) | set(zq)):
                if q in zq:
                    shape = [1] * n
                    shape[n - 1 - q] = 2
                    w = w * (y if q in xq else z).reshape(shape)
            axes = tuple(n - 1 - q for q in xq)
            g = groups.setdefault(axes, [np.zeros((2,) * n, dtype=dtype), _real_of(dtype).type(0)])
            g[0] += w
            g[1] += abs(dtype(amp))
        self.groups = groups
        self._finish()

    def _finish(self):
        """Per group: W as a flat vector, and the flipped ROW-NUMBER tensor (np.flip of arange(N) along the group's axes) -- a flip
        of the state is then one gather through it (a flipped view of a (2,) * n tensor iterates two elements at a time)."""
        rows = np.arange(1 << self.n).reshape((2,) * self.n)
        self._flat = [(np.ascontiguousarray(w).reshape(-1), a, np.ascontiguousarray(np.flip(rows, axis=axes) if axes else rows).reshape(-1))
                      for axes, (w, a) in self.groups.items()]

    def apply(self, x):
        t = np.asarray(x, dtype=self.dtype).reshape(-1)
        out = np.zeros_like(t)
        for w, _, partner in self._flat:
            out += w * t[partner]
        return out

    def abs_apply(self, x):
        """A_r = sum_t |a_t| |x_partner(r, t)|: the X masks only."""
        t = np.abs(np.asarray(x, dtype=self.dtype).reshape(-1))
        out = np.zeros_like(t)
        for _, a, partner in self._flat:
            out += a * t[partner]
        return out

    def __matmul__(self, x):
        return self.apply(x).astype(np.complex128)


def pauli_apply(n, strings, x, dtype=np.clongdouble):
    """sum_t a_t P_t x in ``dtype``."""
    return PauliRef(n, strings, dtype).apply(x)


def pauli_abs_apply(n, strings, x, dtype=np.clongdouble):
    """sum_t |a_t| |x_{partner}| per row (real, in the precision of ``dtype``)."""
    return PauliRef(n, strings, dtype).abs_apply(x)
