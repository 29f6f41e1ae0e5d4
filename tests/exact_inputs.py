"""Exact inputs and output digests for the tests that hold a build's bits against digests recorded from an earlier build
(tests/test_gpu_zgemm_bits.py, tests/test_gpu_rowblock_bits.py, tests/test_gpu_panel_bits.py): 31-bit integers of a quadratic integer recurrence modulo a
prime, scaled by a power of two -- no random-number library, so a digest depends on the kernels alone.  The product of two such
values does not fit a double: every accumulate rounds, and a wrong operand or summation order changes the digest."""
import hashlib

import numpy as np

P = 2147483647      # 2^31 - 1


def seq(count, seed):
    """x_i = (1103515245 i^2 + 1664525 i + seed) mod P, centred: the integer recurrence x_{i+1} = x_i + d_i,
    d_{i+1} = d_i + 2 * 1103515245 (mod P) in closed form, vectorised.  Integers in (-2^30, 2^30) as float64."""
    i = np.arange(count, dtype=np.int64) % P
    x = ((i * i) % P * 1103515245 + i * 1664525 + seed) % P
    return (x - P // 2).astype(np.float64)


def cmat(rows, cols, seed, shift, real=False):
    """rows x cols, entries (integer) 2^-shift, |entry| < 2^(30 - shift)"""
    re = seq(rows * cols, seed).reshape(rows, cols)
    im = np.zeros_like(re) if real else seq(rows * cols, seed + 7919).reshape(rows, cols)
    return np.ldexp(re, -shift) + 1j * np.ldexp(im, -shift)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.complex128).tobytes()).hexdigest()
