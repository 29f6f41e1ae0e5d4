#!/usr/bin/env python3
"""GPU parity check of the term-pair step with the cut of cache-resident operators (csrc/walk_geometry.cpp: walk2_cut_resident --
the wavefronts that take an edge block first walk shorter segments; knob walk_pair = 2) and of the pair's follow-up kernel
(csrc/kernels_walk2.hip: hrb_walk2_edge_kernel -- term m + 1 of the edge blocks, one block per wavefront), at the smallest shapes
that reach every path (walk_min_blocks = 16):

    python tools/check_walk2_resident.py          # exit status 0 and "walk2 resident parity ok" when every check holds

For each shape, an even and an odd number of terms and walk_waves in {0, 1, 64} (1: a wavefront takes several edge blocks; 64: most
or all segments are shortened), three cheby! steps (+dt, -dt, +dt) must agree BIT FOR BIT with the per-block kernel (hrb_walk = 0),
the one-term walk (walk_pair = 0) and the streamed cut with the per-block follow-up (walk_pair = 1, walk_dbg = 8); the statistics
must count (nterms - 1) // 2 pair launches and nterms mat-vecs; the automatic rule must leave operators this small alone; one
shape is held against the oracle to 1e-10.  (A script, not a pytest file: tests/required_gpu_tests.txt lists the suite's GPU tests.
__graft_entry__.py: smoke() runs the compact form of the same check at N = 2^18.)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import qp_oracle as qo  # noqa: E402
import qprop_amd.lib as L  # noqa: E402
import qprop_amd.synth as synth  # noqa: E402

TOL = 1e-10
DEFAULTS = {"hrb_walk": 1, "walk_pair": -1, "walk_min_blocks": 3072, "walk_nt": -1, "walk_waves": 0, "walk_dbg": 0}
PAIR_FOLLOW_UP_PER_BLOCK = 8      # walk_dbg bit (csrc/walk_geometry.h: kWalkDbgPairFollowUpPerBlock)


def _lattice_44():
    N = 1 << 15
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4, 128, 256, 384, 512))
    return N, rp, col, vals


def _lattice_22_diag_real():
    import scipy.sparse as sp
    N = 1 << 13
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 64, 128))
    vals = vals.real.astype(np.complex128)
    H = sp.csr_matrix((vals, col, rp), shape=(N, N)) + sp.diags(np.random.default_rng(3).uniform(-1.0, 1.0, N)).astype(np.complex128)
    H = H.tocsr()
    H.sort_indices()
    return N, H.indptr.astype(np.int64), H.indices.astype(np.int32), H.data.astype(np.complex128)


def _open_grid():
    H = synth.grid_hamiltonian_2d(96, 64)
    return 96 * 64, H.indptr.astype(np.int64), H.indices.astype(np.int32), H.data.astype(np.complex128)


# has_pairs: the operator has a two-term plan.  The open grid's strip step is 96 rows, no multiple of 64: it has none (as
# tests/golden/plans_parent.json records), every setting below runs its one-term launches and the check holds that they agree.
SHAPES = {"near4far4_g128": (_lattice_44, True), "near2far2_g64+diag_real": (_lattice_22_diag_real, True), "grid96x64_open": (_open_grid, False)}


def check_shape(ctx, shape):
    make, has_pairs = SHAPES[shape]
    N, rp, col, vals = make()
    ctx.tuning_set("walk_min_blocks", 16)
    Op = L.Operator(ctx, [L.Matrix(ctx, N, N, rp, col, vals)])
    assert Op.walk_info()["valid"] == 1
    psi0 = synth.random_state(N)
    for dt in (1.0, 0.35):                 # 35 / 22 coefficients at Delta = 24: 34 and 21 terms, an even and an odd number
        wrk = L.ChebyWrk(ctx, N, 24.0, -12.0, dt)
        nterms = wrk.n_coeffs - 1
        assert nterms % 2 == (0 if dt == 1.0 else 1)

        def run(**knobs):
            for k, v in {**DEFAULTS, "walk_min_blocks": 16, **knobs}.items():
                ctx.tuning_set(k, v)
            info = Op.walk2_info()
            psi = L.State(ctx, data=psi0)
            ctx.reset_stats()
            L.cheby(psi, Op, dt, wrk)
            st = ctx.stats()
            L.cheby(psi, Op, -dt, wrk)
            L.cheby(psi, Op, dt, wrk)
            out = psi.numpy()
            psi.close()
            return out, info, st

        block, i0, _ = run(hrb_walk=0)                                            # the per-block kernel, one term per launch
        one, i1, s1 = run(walk_pair=0)                                            # the one-term strip walk
        assert i0["valid"] == 0 and i1["valid"] == 0 and s1["n_pair_launches"] == 0 and s1["n_matvec"] == nterms
        assert np.array_equal(block, one)
        old, io, so = run(walk_pair=1, walk_dbg=PAIR_FOLLOW_UP_PER_BLOCK)         # streamed cut, per-block follow-up
        assert io["valid"] == (1 if has_pairs else 0) and np.array_equal(block, old)
        for waves in (0, 1, 64):
            got, info, st = run(walk_pair=2, walk_waves=waves)
            assert info["valid"] == (1 if has_pairs else 0), (waves, info)
            assert st["n_pair_launches"] == ((nterms - 1) // 2 if has_pairs else 0) and st["n_matvec"] == nterms, (waves, st)
            assert np.array_equal(block, got), (dt, waves, float(np.max(np.abs(block - got))))
            if has_pairs:
                # a pair is two launches (the walk and the edge blocks' second term), term 1 one, an odd last term one
                assert st["n_kernel_launches"] >= 2 * st["n_pair_launches"] + 1 + (nterms - 1) % 2
                if waves == 1:            # one segment: its wavefronts take several edge blocks each
                    assert info["segments"] == 1 and info["edge_blocks"] > 4 * ((info["chunks_per_strip_step"] + 3) // 4)
        if has_pairs:
            got, info, _ = run(walk_pair=1)                                       # streamed cut, new follow-up kernel
            assert info["valid"] == 1 and np.array_equal(block, got)
        auto, ia, sa = run()                                                      # the automatic rule: not for operators this small
        assert ia["valid"] == 0 and sa["n_pair_launches"] == 0 and np.array_equal(block, auto)
        if shape == "near4far4_g128" and dt == 1.0:
            H = synth.to_scipy(rp, col, vals, N)
            ref = qo.cheby(psi0.copy(), H, 1.0, qo.ChebyWrk(psi0, 24.0, -12.0, 1.0))
            ref = qo.cheby(ref, H, -1.0, qo.ChebyWrk(psi0, 24.0, -12.0, 1.0))
            ref = qo.cheby(ref, H, 1.0, qo.ChebyWrk(psi0, 24.0, -12.0, 1.0))
            err = float(np.linalg.norm(block - ref))
            assert err < TOL, err
        wrk.close()
    for k, v in DEFAULTS.items():
        ctx.tuning_set(k, v)


def main():
    ctx = L.Context(0)
    try:
        for shape in SHAPES:
            check_shape(ctx, shape)
            print(f"{shape}: identical bits", flush=True)
    finally:
        ctx.close()
    print("walk2 resident parity ok")


if __name__ == "__main__":
    main()
