"""The fp64 matrix-core kernels (csrc/zgemm_mfma.h: the 32 x 32 and 16 x 16 Liouvillian kernels of
csrc/engine_liouville.hip, the dense panel Chebyshev term of csrc/kernels_dense.hip) give the bits they gave before the
shared tile core existed: SHA-256 digests of their outputs, recorded from the build of the commit before it, in
tests/golden/zgemm_bits_parent.json.

The inputs are exact (tests/exact_inputs.py): 31-bit integers of a quadratic integer recurrence modulo a prime, scaled by a power
of two (no random-number library), so the digests depend on the kernels alone.  The products of two such values do not fit a double:
every accumulate rounds, and a wrong operand, pipeline slot, tail or summation order changes the digest, while the order in
which independent accumulators are issued cannot.  The Lindblad operators are few-bit integers, so that the one library GEMM
on the way (G = sum_k A_k^+ A_k at creation) is exact in any order.

The shapes are the smallest that reach each branch of the shared code (D = 6 pipeline slots; a wavefront takes the steady
branch from 2 D - 1 = 11 k-steps):
  Liouvillian 32 x 32   n = 20 short branch in every wave, one wave without k-steps, one partial tile; n = 45, nc = 2
                        n & 3 = 1 with the round-robin tail over 4 products, wave totals 12, 12, 12, 8, edge tiles; n = 96
                        steady loop and drain on whole tiles; n = 176 exactly 11 k-steps per wave in the batched launch
  Liouvillian 16 x 16   n = 3, 33, 50 (LvN once, at n = 33)
  dense panel           (33, 8) 16 x 16 tile, short branch, ncols & 3 = 1; (179, 5) 16 x 16, steady branch, ncols & 3 = 3;
                        (1540, 33) 16 x 32 tile; (3076, 33) 32 x 32 tile with edge rows and edge columns
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import qprop_amd.lib as L  # noqa: E402
from exact_inputs import cmat as _cmat, digest as _digest, seq as _seq  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(ROOT, "tests", "golden", "zgemm_bits_parent.json")


def _small_int_mat(n, seed):
    """few-bit entries: (integers in [-8, 8]) / 16, real and imaginary part"""
    re = np.round(_seq(n * n, seed) * 2.0 ** -27).reshape(n, n)
    im = np.round(_seq(n * n, seed + 104729) * 2.0 ** -27).reshape(n, n)
    return (re + 1j * im) / 16.0


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


def liouville_bits(ctx, n, nc, convention, fused_n, tile32_n):
    """digests of mul! in the 3- and the 5-argument form through the path the two knobs select: with tile32_min_n = 0 the
    32 x 32 kernel is taken for n <= tile32_n, else the 16 x 16 kernel for n <= fused_n (liouville_apply)"""
    knobs = {"liouville_fused_n": fused_n, "liouville_tile32_n": tile32_n, "liouville_tile32_min_n": 0}
    saved = {k: ctx.tuning_get(k) for k in knobs}
    try:
        for k, v in knobs.items():
            ctx.tuning_set(k, v)
        sh = 31 + int(np.ceil(np.log2(n))) // 2       # entries of H and rho of order n^-1/2
        H = _cmat(n, n, 11 + n, sh)
        H = H + H.conj().T
        cops = [_small_int_mat(n, 1000 * (k + 1) + n) for k in range(nc)]
        Lmf = L.Liouvillian(ctx, [H], cops, convention=convention)
        x = _cmat(n, n, 5 + n, sh).reshape(-1)
        y0 = _cmat(n, n, 3 + n, 31).reshape(-1)
        xs, ys = L.State(ctx, data=x), L.State(ctx, n=n * n)
        ctx.reset_stats()
        Lmf.mul(xs, ys)
        out = {"mul3": _digest(ys.numpy())}
        ys.upload(y0)
        Lmf.mul(xs, ys, 0.75 - 0.25j, -0.375 + 0.125j)
        out["mul5"] = _digest(ys.numpy())
        # a matrix-core path takes two launches per application (the batched A_k rho, then the sum), the library chain 2 + 2 nc
        assert nc >= 1 and ctx.stats()["n_kernel_launches"] == 4
        return out
    finally:
        for k, v in saved.items():
            ctx.tuning_set(k, v)


def dense_bits(ctx, N, batch, real):
    """digest of one batched Chebyshev step of a dense N x N operator on a panel of `batch` states"""
    sh = 31 + int(np.ceil(np.log2(N)))                # |H| < 1/2 in the Frobenius norm: inside the window [-1, 1]
    H = _cmat(N, N, 17 + N, sh, real=real)
    M = L.Matrix(ctx, N, N, np.arange(N + 1, dtype=np.int64) * N, np.tile(np.arange(N, dtype=np.int32), N), H.reshape(-1))
    op = L.Operator(ctx, [M])
    assert op.format == L.FMT_DENSE
    states = _cmat(N, batch, 23 + N, 31 + int(np.ceil(np.log2(N))) // 2)
    panel = L.State(ctx, data=states.reshape(-1))
    wrk = L.ChebyWrk(ctx, N * batch, 2.0, -1.0, 0.5)
    assert 4 <= wrk.n_coeffs <= 16
    ctx.reset_stats()
    L.cheby_batched(panel, op, 0.5, wrk, batch)
    assert ctx.stats()["n_matvec"] == wrk.n_coeffs - 1
    return {"step": _digest(panel.numpy())}


LIOUVILLE_32 = [(20, 1), (45, 2), (96, 1), (176, 1)]
LIOUVILLE_16 = [(3, "TDSE"), (33, "TDSE"), (33, "LvN"), (50, "TDSE")]
DENSE = [(33, 8), (179, 5), (1540, 33), (3076, 33)]


@pytest.mark.parametrize("n,nc", LIOUVILLE_32)
def test_liouville_tile32_bits(ctx, parent, n, nc):
    assert liouville_bits(ctx, n, nc, "TDSE", 0, 4096) == parent[f"liouville32-n{n}-nc{nc}"]


@pytest.mark.parametrize("n,convention", LIOUVILLE_16)
def test_liouville_tile16_bits(ctx, parent, n, convention):
    assert liouville_bits(ctx, n, 1, convention, 4096, 0) == parent[f"liouville16-n{n}-{convention}"]


@pytest.mark.parametrize("N,batch", DENSE)
@pytest.mark.parametrize("real", [True, False], ids=["realH", "complexH"])
def test_dense_panel_bits(ctx, parent, N, batch, real):
    assert dense_bits(ctx, N, batch, real) == parent[f"dense-N{N}-b{batch}-{'real' if real else 'complex'}"]
