#!/usr/bin/env python3
"""Fuzz the Pauli-string operator (csrc/engine_pauli.hip) against the NumPy oracle driven by the extended-precision tensor-axis
reference (tests/pauli_ref.py -- independent of the mask arithmetic, and fast enough for thousands of strings): random registers of
6-13 qubits, 1-3 terms of the lazy sum with random real coefficients and a scale, 1-60 random strings per term (any mix of I / X / Y / Z,
so that groups with one string, groups with many, a diagonal group with one or many strings or none all occur); one case in eight is
beyond what the kernel stages in LDS (1025-1400 distinct x masks, or 2049-2500 strings: the kernel that reads its tables from global
memory).  Forward and backward cheby! steps with coefficients changing in between, then a mul! with random alpha / beta -- in one
case of four with complex coefficients and scale (the signed / complex-diagonal kernels).  Test infrastructure: oracle/ is the checker.

    python tools/fuzz_pauli.py [n_cases] [seed]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import qp_oracle as qo  # noqa: E402
import qprop_amd.lib as L  # noqa: E402
import qprop_amd.synth as synth  # noqa: E402
from pauli_ref import PauliRef  # noqa: E402


def small_terms(rng, n, nops):
    p_id = float(rng.choice([0.3, 0.6, 0.85]))
    terms = []
    for _ in range(nops):
        strings = []
        for _ in range(int(rng.integers(1, 61 // nops + 1))):
            lab = "".join(rng.choice(list("IXYZ"), size=n, p=[p_id] + [(1 - p_id) / 3] * 3))
            if rng.integers(0, 4) == 0:          # a diagonal string
                lab = lab.replace("X", "Z").replace("Y", "I")
            strings.append((float(rng.uniform(-1, 1)), L.pauli_masks(lab)))
        terms.append(strings)
    return terms


def large_terms(rng, n, nops):
    """More groups (1025-1400 x masks, one or two strings each) or more strings (2049-2500 over a few hundred x masks, the zero mask
    among them at times) than the tables in LDS hold; amplitudes scaled so that the spectral bound stays of order ten."""
    N = 1 << n
    if rng.integers(0, 2):
        xms = rng.permutation(np.arange(1, N))[: int(rng.integers(1025, 1401))]
        masks = [(int(xm), int(rng.integers(0, N))) for xm in xms for _ in range(int(rng.integers(1, 3)))]
    else:
        count = int(rng.integers(2049, 2501))
        xms = rng.permutation(np.arange(0 if rng.integers(0, 2) else 1, N))[: int(rng.integers(200, 600))]
        masks = [(int(xms[int(rng.integers(0, len(xms)))]), int(rng.integers(0, N))) for _ in range(count)]
    terms = [[] for _ in range(nops)]
    for m in masks:
        terms[int(rng.integers(0, nops))].append((float(rng.uniform(-1, 1)) * 20.0 / len(masks), m))
    for strings in terms:
        if not strings:
            strings.append((0.25, (1, 0)))
    return terms


def combined(terms, scale, coeffs, nops):
    """The strings of scale * sum_l c_l H_l with their current amplitudes (extended precision products)."""
    out = []
    for l, strings in enumerate(terms):
        c = 1.0 if l < nops - len(coeffs) else coeffs[l - (nops - len(coeffs))]
        out += [(np.clongdouble(scale) * np.clongdouble(c) * np.clongdouble(a), m) for a, m in strings]
    return out


def main():
    ncases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    rng = np.random.default_rng(seed)
    ctx = L.Context(0)
    bad, worst = 0, 0.0
    for case in range(ncases):
        large = rng.integers(0, 8) == 0
        n = int(rng.integers(11, 14)) if large else int(rng.integers(6, 14))
        N = 1 << n
        nops = int(rng.integers(1, 4))
        ncoeffs = int(rng.integers(0, nops + 1))
        terms = large_terms(rng, n, nops) if large else small_terms(rng, n, nops)
        op = L.PauliOperator(ctx, n, terms, ncoeffs=ncoeffs)
        scale = float(rng.choice([1.0, -0.7, 2.0]))
        op.set_scale(scale)
        psi0 = synth.random_state(N, seed=case)
        psi = L.State(ctx, data=psi0)
        ref = psi0.copy()
        err = 0.0
        bound = abs(scale) * sum(1.5 * sum(abs(a) for a, _ in s_) for s_ in terms) + 1e-3
        dt = float(rng.uniform(2.0, 12.0)) / bound
        wrk = L.ChebyWrk(ctx, N, 2.1 * bound, -1.05 * bound, dt)
        owrk = qo.ChebyWrk(psi0, 2.1 * bound, -1.05 * bound, dt)
        coeffs = np.ones(ncoeffs)
        for step in range(3):
            coeffs = rng.uniform(-1.5, 1.5, ncoeffs)
            if ncoeffs:
                op.set_coeffs(coeffs)
            sg = 1 if rng.integers(0, 3) else -1
            L.cheby(psi, op, sg * dt, wrk)
            qo.cheby(ref, PauliRef(n, combined(terms, scale, coeffs, nops)), sg * dt, owrk)
            err = max(err, float(np.linalg.norm(psi.numpy() - ref)))
        cplx_leg = rng.integers(0, 4) == 0
        if cplx_leg:      # (mul! only: the generator is no longer Hermitian)
            scale = complex(rng.choice([1.0, -0.7, 2.0]), rng.choice([0.0, 0.5, -1.0]))
            op.set_scale(scale)
            if ncoeffs:
                coeffs = rng.uniform(-1.5, 1.5, ncoeffs) + 1j * rng.uniform(-1.5, 1.5, ncoeffs) * rng.integers(0, 2, ncoeffs)
                op.set_coeffs(coeffs)
        x0, y0 = synth.random_state(N, seed=1000 + case), synth.random_state(N, seed=2000 + case)
        x, y = L.State(ctx, data=x0), L.State(ctx, data=y0)
        al, be = complex(rng.normal(), rng.normal()), complex(rng.normal(), rng.normal()) * float(rng.integers(0, 2))
        op.mul(x, y, alpha=al, beta=be)
        want = be * y0 + al * (PauliRef(n, combined(terms, scale, coeffs, nops)) @ x0)
        err = max(err, float(np.linalg.norm(y.numpy() - want)) / max(1.0, bound))
        worst = max(worst, err)
        if not err < 1e-10:
            bad += 1
            print(f"case {case}: n={n} nops={nops} ncoeffs={ncoeffs} strings={[len(s_) for s_ in terms]} large={bool(large)} "
                  f"complex={bool(cplx_leg)} err={err:.3e}  BAD", flush=True)
        for h in (x, y, psi, wrk, op):
            h.close()
    print(f"{ncases} cases (seed {seed}), {bad} bad, worst error {worst:.3e}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
