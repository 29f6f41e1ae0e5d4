"""The threaded host build on the REAL device path: what qp_matrix_create / qp_operator_create lay out must not depend on how many
host threads parallel_rows (csrc/operator_layout.h) cuts its passes into.  The CPU harness (tests/sanitize_host_index.cpp --large,
tests/test_cabi_host.py::test_threaded_host_build) proves that array by array on a stand-in device, under ThreadSanitizer and
ASan/UBSan; there the pinned host vectors and the uploads are heap memory.  Here three fresh child processes
(tests/threaded_build_worker.py; QP_HOST_THREADS = 1, 5, 16 -- read once per process) build four operators of 2^18 + 77 rows on the
MI355X -- the headline lattice Hermitian-packed and as chosen, a random-column Hermitian operator with the column-blocked mirror,
a lattice plus a sparse control term -- and report digests of get_csr, of y = A x and of one Chebyshev step, with the layout, walk
and mirror dictionaries: the three records must be equal, and the one-thread child's y must be A x (scipy) to the bound of
test_gpu_parity.py::test_operator_mul."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import threaded_build_worker as W  # noqa: E402

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "threaded_build_worker.py")
THREADS = (1, 5, 16)


def _child(threads, dump=None):
    """one worker after another, each under its own time limit: a child that runs into it raises here and nothing more is started"""
    cmd = [sys.executable, WORKER] + (["--dump", str(dump)] if dump else [])
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=180, cwd=ROOT, env=dict(os.environ, QP_HOST_THREADS=str(threads)))
    assert run.returncode == 0, (threads, (run.stdout + run.stderr)[-3000:])
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("THREADED_BUILD ")]
    assert len(lines) == 1, (threads, run.stdout[-2000:])
    return json.loads(lines[0][len("THREADED_BUILD "):])


def test_threaded_build_is_the_same_on_every_thread_count(tmp_path):
    records = {}
    for t in THREADS:
        records[t] = _child(t, dump=tmp_path if t == 1 else None)
        assert records[t]["host_threads_requested"] == str(t)
    one = records[1]["operators"]
    assert set(one) == set(W.operators())
    # the operators are what they are here for
    import qprop_amd.lib as L
    assert one["lattice-hrb"]["format"] == L.FMT_HRB and one["lattice-hrb"]["walk"]["valid"] == 1
    assert one["lattice-auto"]["format"] == L.FMT_HRB and one["lattice-auto"]["walk"]["valid"] == 1
    assert one["lattice-hrb"]["layout"]["blocks"] >= 4096 and one["lattice-hrb"]["layout"]["stored"] >= 1 << 20
    assert one["random-columns-mirror"]["colblock"]["valid"] == 1 and one["random-columns-mirror"]["colblock"]["tiles"] >= 512
    assert one["lattice-plus-sparse-control"]["first_sparse_term"] == 1
    for t in THREADS[1:]:
        got = records[t]["operators"]
        for name in one:
            for key in one[name]:
                assert got[name][key] == one[name][key], f"{name}: {key} differs between {t} host threads and 1: {got[name][key]} != {one[name][key]}"
        assert got == one
    # y = A x of the one-thread child against scipy
    x = W.state()
    for name, (terms, coeffs, _, _) in W.operators().items():
        mats = [make() for make in terms]
        drift = len(mats) - len(coeffs)
        ref = np.zeros(W.N, dtype=np.complex128)
        for l, A in enumerate(mats):
            ref += (coeffs[l - drift] if l >= drift else 1.0) * (A @ x)
        y = np.load(os.path.join(tmp_path, name + ".npy"))
        err, bound = float(np.linalg.norm(y - ref)), 1e-12 * max(1.0, float(np.linalg.norm(ref)))
        print(f"{name}: |y - A x| = {err:.3e}, bound {bound:.3e}")
        assert err < bound, (name, err, bound)
