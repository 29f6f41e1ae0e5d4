"""Worker of tests/test_gpu_threaded_build.py: one process per host thread count (QP_HOST_THREADS is read once per process,
csrc/operator_layout.h: host_threads).  Builds four operators of 2^18 + 77 rows -- past the 2^16-row, 4096-block, 512-tile and
2^20-element thresholds of parallel_rows -- on the real device path (pinned host vectors, uploads) and prints one JSON record:
per operator the SHA-256 of the get_csr arrays, the layout / walk / mirror dictionaries, the SHA-256 of y = mul(x) and of the state
after one cheby step.  `--dump DIR` also writes every y to DIR/<name>.npy (the parent checks the one-thread child's against scipy).
The operators and the state come from the counter-based generators of qprop_amd.synth: the same bits in every process."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = (1 << 18) + 77
CONTROL_COEFF = 0.75
DELTA, E_MIN, DT = 24.0, -12.0, 0.5      # (Gershgorin: every operator below has its spectrum inside [-10.4, 10.4])


def lattice():
    import qprop_amd.synth as synth
    rp, col, vals = synth.hermitian_offsets_csr(N, rho=10.0)      # the headline offsets 1, 2, 3, 4, 1024, ..., 4096
    return synth.to_scipy(rp, col, vals, N)


def random_columns():
    import qprop_amd.synth as synth
    rp, col, vals = synth.random_columns_csr(N, n_pairs=4)
    return synth.to_scipy(rp, col, vals, N)


def control():
    """a control term on few positions: a real diagonal entry on every 16th row"""
    import scipy.sparse as sp
    rows = np.arange(0, N, 16, dtype=np.int64)
    return sp.csr_matrix((np.full(len(rows), 0.5, dtype=np.complex128), (rows, rows)), shape=(N, N))


def state():
    import qprop_amd.synth as synth
    return synth.random_state(N, seed=4242)


# name -> (terms, coefficients, requested format, knobs during the build)
def operators():
    import qprop_amd.lib as L
    return {
        "lattice-hrb": ([lattice], [], L.FMT_HRB, {}),
        "lattice-auto": ([lattice], [], L.FMT_AUTO, {}),
        "random-columns-mirror": ([random_columns], [], L.FMT_AUTO, {"colblock": 2, "cb_log2w": 14}),
        "lattice-plus-sparse-control": ([lattice, control], [CONTROL_COEFF], L.FMT_AUTO, {}),
    }


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    import qprop_amd.lib as L
    dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None
    ctx = L.Context(0)
    x0 = state()
    out = {"host_threads_requested": os.environ.get("QP_HOST_THREADS"), "operators": {}}
    for name, (terms, coeffs, fmt, knobs) in operators().items():
        saved = {k: ctx.tuning_get(k) for k in knobs}
        for k, v in knobs.items():
            ctx.tuning_set(k, v)
        mats = [L.Matrix.from_scipy(ctx, make()) for make in terms]
        op = L.Operator(ctx, mats, len(coeffs), fmt)
        if coeffs:
            op.set_coeffs(coeffs)
        rec = {"format": int(op.format), "csr": sha(*op.get_csr()), "layout": op.layout_info(), "walk": op.walk_info(), "colblock": op.colblock_info(),
               "first_sparse_term": op.evaluate_info()["first_sparse_term"]}
        rec["colblock"]["own_line_share"] = float(rec["colblock"]["own_line_share"]).hex()
        x = L.State(ctx, data=x0)
        y = L.State(ctx, n=N)
        op.mul(x, y)
        yh = y.numpy()
        rec["mul"] = sha(yh)
        if dump:
            np.save(os.path.join(dump, name + ".npy"), yh)
        wrk = L.ChebyWrk(ctx, N, DELTA, E_MIN, DT)
        L.cheby(x, op, DT, wrk)
        psi = x.numpy()
        assert np.all(np.isfinite(psi.view(np.float64))), name
        rec["cheby"] = sha(psi)
        for h in (wrk, x, y, op, *mats):
            h.close()
        for k, v in saved.items():
            ctx.tuning_set(k, v)
        out["operators"][name] = rec
    ctx.close()
    print("THREADED_BUILD " + json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
