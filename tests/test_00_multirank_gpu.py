"""End-to-end multi-rank test of the product HIP path on ONE GPU: 2 and 3 processes share GPU
0 (collective staged through the host with gloo -- see tests/multirank_gpu_worker.py).  This
file sorts first on purpose: the children must be started before this process initialises the
GPU (a GPU-initialised parent must not fork+exec on the test pool)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _gpus():
    """GPUs on this box WITHOUT initialising one in this process (device_count does not, on this image)."""
    import torch
    return torch.cuda.device_count()


# "shared": all ranks on GPU 0, the exchange staged through the host (gloo / the callback communicator) -- what a one-GPU
# test box can run.  "rccl": ONE GPU PER RANK, the exchange on the library's own RCCL communicator (and torch's nccl group for
# the Python-driven schedule): the same worker, the same oracle comparison; runs by itself on any box with enough GPUs and
# skips with the reason on the others, so that the first multi-GPU box exercises real RCCL without anyone asking.
TRANSPORTS = ["shared", "rccl"]


def _transport_env(transport, world):
    if transport == "shared":
        return {}
    n = _gpus()
    if n < world:
        pytest.skip(f"transport=rccl needs one GPU per rank: {world} ranks, {n} GPU(s) on this box "
                    "(RCCL forms no multi-rank communicator on one device)")
    return {"QP_REAL_GPUS": "1"}


def _run(world, timeout=240, **env_extra):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", **env_extra)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "multirank_gpu_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    # (a rank that dies takes the others' barrier down with it: show the rank that failed FIRST, i.e. not with
    # the "connection closed by peer" of a survivor)
    bad = [(p.returncode, out) for p, out in zip(procs, outs) if p.returncode != 0]
    bad.sort(key=lambda t: "Connection closed by peer" in t[1])
    assert not bad, "\n-----\n".join(f"rc {rc}: {out[-1500:]}" for rc, out in bad[:3])
    assert all("err=" in out for out in outs)
    return outs


@pytest.mark.parametrize("transport", TRANSPORTS)
@pytest.mark.parametrize("world,overlap,exchange,uneven", [
    (2, "1", "auto", "0"),
    (2, "0", "auto", "0"),
    (3, "1", "auto", "1"),
    (2, "1", "allgather", "0"),
])
def test_multirank_hip_path_one_gpu(world, overlap, exchange, uneven, transport):
    outs = _run(world, QP_OVERLAP=overlap, QP_EXCHANGE=exchange, QP_UNEVEN=uneven, **_transport_env(transport, world))
    assert all(f"transport={transport}" in o for o in outs)


@pytest.mark.parametrize("transport", TRANSPORTS)
@pytest.mark.parametrize("world,overlap,exchange,uneven,p2p", [
    (2, "1", "auto", "0", "1"),        # neighbour lists (send/recv form of the exchange), overlap
    (3, "1", "auto", "1", "1"),        # three ranks, uneven blocks
    (3, "0", "auto", "1", "0"),        # all-gather form, serial schedule
    (2, "1", "allgather", "0", "0"),   # scattered H: the slice itself is the send buffer
])
def test_multirank_native_driver_one_gpu(world, overlap, exchange, uneven, p2p, transport):
    """qp_sharded_cheby_step (the whole partitioned cheby! in one library call) with 2 and 3 ranks
    sharing the GPU: the exchange is handed back through qp_comm_create_callback and staged through
    the host, everything else -- term loop, two streams, fused pack, neighbour slots -- is the code
    that runs with RCCL on one GPU per rank."""
    outs = _run(world, QP_OVERLAP=overlap, QP_EXCHANGE=exchange, QP_UNEVEN=uneven, QP_NATIVE="1", QP_P2P=p2p,
                **_transport_env(transport, world))
    assert all("native=yes" in o and f"transport={transport}" in o for o in outs)
    # what RCCL itself says the communicator is (qp_comm_info): `world` ranks on a real one, none on the callback stand-in
    assert all(f"rccl_ranks={world if transport == 'rccl' else 0}" in o for o in outs)


@pytest.mark.parametrize("transport", TRANSPORTS)
@pytest.mark.parametrize("world", [2, 3])
def test_multirank_newton_one_gpu(world, transport):
    """Row-partitioned newton! (all-reduced Arnoldi inner products) with ranks sharing the GPU / one GPU per rank over nccl."""
    _run(world, QP_METHOD="newton", **_transport_env(transport, world))


@pytest.mark.parametrize("transport", TRANSPORTS)
def test_c4_full_size_eight_ranks_one_gpu(transport):
    """BASELINE configs[3] at its size: N = 2^24 rows as 8 ranks x 2^21 rows sharing the one GPU, the library's
    one-call step with the exchange through the callback communicator (the same code that runs with RCCL on one
    GPU per rank): norms, forward / backward round trip, and the state after one step against the C oracle on
    2^18-row windows inside a rank, across a rank boundary and across the periodic wrap."""
    outs = _run(8, timeout=900, QP_METHOD="c4", **_transport_env(transport, 8))
    assert all("c4 N=2^24" in o and "exchange=halo" in o and "M=8192" in o for o in outs)
    assert sum("err=0.000e+00" not in o for o in outs) >= 3      # the windows were compared on the ranks that own them


@pytest.mark.parametrize("transport", TRANSPORTS)
def test_c4_full_size_eight_ranks_allgather_form_one_gpu(transport):
    """The same size in the ALL-GATHER form (the collective BASELINE's north_star names): a scattered H whose send list is every
    rank's whole 2^21-row slice, 32 MiB per rank and term through the exchange; the state after one step against the C
    oracle at full size (computed once, on rank 0), norm and forward / backward round trip.  (dt = 0.1, 11 coefficients:
    each term of this form moves 256 MB through the host-staged exchange.)"""
    outs = _run(8, timeout=1500, QP_METHOD="c4-allgather", **_transport_env(transport, 8))
    assert all("c4-allgather N=2^24" in o and "exchange=allgather" in o and f"M={1 << 21}" in o for o in outs)


def test_bench_eight_ranks_full_c4_flow_one_gpu():
    """The COMPLETE `bench.py --gpus 8` flow at config C4's size (2^21 rows per rank, N = 2^24), as the driver launches it,
    with the 8 ranks sharing the test GPU: conservative pass, native set-up + self-check, both schedules' trial, the timed
    steps, the strong point -- so that the first run on a real 8-GPU node exercises nothing for the first time but RCCL
    itself.  Must finish well inside the driver's patience (asserted: < 10 min)."""
    import json
    import time
    world = 8
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    t0 = time.time()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", QP_BENCH_ONE_GPU="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "2",
                                       "--warmup", "1", "--full"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=900))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    took = time.time() - t0
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, err[-3000:]
    assert took < 600, f"the full --gpus 8 flow took {took:.0f} s"
    lines = [ln for ln in outs[0][0].splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    # the printed line is the compact one the driver parses: below 4 KB, no long strings, the gate keys
    assert len(lines[0]) < 4096
    d = json.loads(lines[0])
    assert d["degraded"] is False and d["native_path"].startswith("ok") and d["n_gpus"] == 8 and d["scaling"] == "weak"
    assert d["config"]["N_total"] == 1 << 24 and d["config"]["rows_per_gpu"] == 1 << 21
    par = d["config"]["parallelism"]
    # (the line reports the faster of the conservative and the native measurement; the native path's schedule and driver are named either way)
    assert "row-partitioned x8" in par and "exchange=halo" in par and "schedule=" in par and "driver=native" in par and len(par) <= 160
    assert d["roofline"]["frac"] > 0 and d["roofline"]["bound"] == "hbm" and d["value"] > 0
    assert d["strong_point"]["N_total"] == 1 << 20 and d["strong_point"]["prop_steps_per_s"] > 0
    # the collective north_star names has a measured point of its own next to the halo headline
    ag = d["allgather_form"]
    assert ag["us_per_term"] > 0 and ag["blocks_per_s"] > 0 and "error" not in ag
    # (round 6: the denominator is the two-term walk's single-GPU time, 1.6 x faster than round 5's, while a rank still launches its
    # terms one by one: the predicted ratio for the halo form is ~5, the ranks' absolute rate is what it was)
    assert d["prediction"]["fixed_n24_speedup_8gpu_halo"] > 4.5 > d["prediction"]["fixed_n24_speedup_8gpu_allgather"]
    # the complete record next to the script
    assert d["extras_file"] == "bench_extras_c4_gpus8.json"
    with open(os.path.join(ROOT, d["extras_file"])) as f:
        full = json.load(f)
    assert full["config"]["blocks_of_2^20_rows_per_step"] == 16.0 and "schedule=auto: overlap" in full["config"]["parallelism"] and "driver=native" in full["config"]["parallelism"]
    sp_ = full["strong_scaling_point"]
    assert sp_["N_total"] == 1 << 20 and sp_["rows_per_gpu"] == 1 << 17 and sp_["prop_steps_per_s"] > 0
    xm = full["exchange_model"]
    assert xm["rows_sent_per_rank_per_term"] == 8192 and xm["peers"] == 2
    pred = full["scaling_prediction"]         # the 1 / 2 / 4 / 8 table the first real run is read against
    assert [r["gpus"] for r in pred["fixed_problem_N_2^24"]] == [1, 2, 4, 8]
    assert pred["fixed_problem_N_2^24"][-1]["speedup_halo_overlap"] > 4.5 > pred["fixed_problem_N_2^24"][-1]["speedup_allgather"]
    assert pred["us_per_term_one_term_walk_by_log2_rows"]["21"] > pred["us_per_term_by_log2_rows"]["21"] * 0.95


# ---------------------------------------------------------------------------------------------------------------------
# Restored in round 6 (commit 06cd45f of round 5 had dropped them by accident; tests/required_gpu_tests.txt + the CPU test
# tests/test_required_gpu_tests.py now fail the CPU suite if any of these names stops being collected).
# bench.py prints a compact line (< 4 KB) and writes the complete record next to the script: `_bench()` returns both.
# ---------------------------------------------------------------------------------------------------------------------

def _bench(world, argv, rc_expected=0, timeout=300, **env_extra):
    """`bench.py` as the driver launches it for N ranks (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment), in
    its test mode where the ranks share GPU 0 -> (compact line of rank 0, complete record from the sidecar, [(stdout, stderr)])."""
    import json
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0", QP_BENCH_ONE_GPU="1", **env_extra)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world)] + argv, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=timeout))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == rc_expected, f"rc {p.returncode}\n" + err[-3000:]
    lines = [ln for ln in outs[0][0].splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and not any(ln.startswith("{") for o, _ in outs[1:] for ln in o.splitlines())
    assert outs[0][0].rstrip().splitlines()[-1] == lines[0] and len(lines[0]) < 4096       # LAST line, and one the driver can parse
    d = json.loads(lines[0])
    with open(os.path.join(ROOT, d["extras_file"])) as f:
        full = json.load(f)
    return d, full, outs


def test_split_wait_timeout_is_reported_not_hung():
    """The in-launch hand-off boundary(m) -> interior(m + 1) polls a counter with a bounded spin.  Forced failure: the
    boundary launches do not signal (knob split_dbg -- developer flavour of the library only, csrc: make dev) and the bound
    is lowered to 2^10 polls (knob split_spin_log2): the interior launch comes back by itself, raises the split's
    host-visible flag, and the NEXT call on that split -- Python-driven term or the library's own step -- returns
    QP_E_INTERNAL instead of computing on with a stale vector; a fresh split on the same context works again."""
    dev = os.path.join(ROOT, "quantumpropagators.jl_amd", "lib", "libqprop_hip_dev.so")
    assert os.path.exists(dev), "lib/libqprop_hip_dev.so is missing: __graft_entry__.build() (make all dev) builds it"
    env = dict(os.environ, QPROP_HIP_LIB=dev, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dev_build_worker.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "dev-build time-out test ok" in r.stdout


def test_library_rccl_communicator_two_gpus():
    """The library's own multi-rank RCCL communicator (two-phase set-up, ncclSend / ncclRecv neighbour exchange,
    ncclAllGather, overlapped and serial schedules) against the oracle -- one GPU per rank, so this needs two
    GPUs and skips itself on the one-GPU test boxes.  qp_comm_info must report ncclCommCount = 2."""
    if _gpus() < 2:
        pytest.skip("needs 2 GPUs (RCCL forms no multi-rank communicator on one device)")
    outs = _run(2, QP_METHOD="rccl")
    assert all("rccl err=" in o and "rccl_ranks=2" in o for o in outs)


@pytest.mark.parametrize("world,driver", [(2, "native"), (3, "torch")])
def test_bench_multirank_flow_one_gpu(world, driver):
    """bench.py as the driver launches it for N > 1, in its test mode where the ranks share GPU 0 and the exchange is staged
    through the host: partition, self-check of the native step against the torch-driven one, barrier + max over ranks, one
    JSON line from rank 0 with the whole-job value, the complete record in the sidecar."""
    d, full, _ = _bench(world, ["--steps", "3", "--warmup", "1", "--log2n", "16", "--driver", driver, "--full"], timeout=240)
    assert d["extras_file"] == f"bench_extras_c4_gpus{world}_n16.json"
    assert d["degraded"] is False and d["native_path"].startswith("ok")
    assert d["n_gpus"] == world and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak"
    # every measured point names its exchange and the RCCL ranks it ran on (0 here: test mode has no RCCL; a real run with
    # rccl_ranks != n_gpus exits with status 4)
    assert d["exchange"] == "halo" and d["rccl_ranks"] == 0
    assert d["allgather_form"]["exchange"] == "allgather" and d["allgather_form"]["rccl_ranks"] == 0
    assert d["conservative_first"]["rccl_ranks"] == 0 if "conservative_first" in d else True
    blocks = full["config"]["blocks_of_2^20_rows_per_step"]
    assert blocks == world / 16.0                       # value counts 2^20-row blocks: N_total / 2^20 of them per step
    assert full["value"] > 0 and abs(full["value"] - blocks * full["config"]["global_steps_per_s"]) < 1e-9 * full["value"]
    assert abs(d["value"] - full["value"]) < 1e-5 * full["value"]
    assert d["config"]["N_total"] == world << 16 and d["cpu_baseline"] is None
    rf = full["roofline"]
    assert 0 < rf["frac"] <= 1.0 and rf["achieved"] <= rf["peak"]          # bytes of the shipped layout: a physical fraction
    assert 0 < d["roofline"]["frac"] <= 1.0 and d["roofline"]["bound"] == "hbm"
    assert rf["layout_bytes_per_launch"] < rf["csr_equivalent_bytes_per_launch"]
    assert abs(rf["effective_csr_equiv_gbs"] * rf["layout_bytes_per_launch"] - rf["achieved"] * rf["csr_equivalent_bytes_per_launch"]) \
        < 1e-6 * rf["achieved"] * rf["csr_equivalent_bytes_per_launch"]
    sp_ = full["strong_scaling_point"]
    if world == 2:                                      # N = 2^20 in total, split over the ranks
        assert sp_["N_total"] == 1 << 20 and sp_["rows_per_gpu"] == 1 << 19 and sp_["prop_steps_per_s"] > 0
        assert d["strong_point"]["N_total"] == 1 << 20 and d["strong_point"]["exchange"] == "halo" and d["strong_point"]["rccl_ranks"] == 0
    else:
        assert sp_ is None and "strong_point" not in d  # 3 does not divide 2^20
    xm = full["exchange_model"]       # the prediction the first real multi-GPU run is read against
    assert xm["rows_sent_per_rank_per_term"] > 0 and xm["peers"] >= 1 and xm["predicted_exchange_us_per_term"] > xm["startup_us_assumed"]
    assert xm["bytes_on_busiest_link_per_term"] == 16 * xm["rows_sent_per_rank_per_term"]
    par = full["config"]["parallelism"]
    # both measurements happened: the conservative one first, then the native / overlapped path under the watchdog;
    # the faster of the two is the reported value and the line names the other
    assert ("conservative schedule measured first" in par) != ("the native / overlapped path (" in par)
    assert f"row-partitioned x{world}" in par and "TEST MODE" in par
    assert "exchange=halo" in par                       # 2^16 rows per rank: banded H exchanges halos only
    assert "schedule=auto: overlap" in par and ("-> overlap" in par or "-> serial" in par)   # both schedules were timed
    assert ("driver=native (library step" in par) if driver == "native" else ("driver=torch.distributed" in par)
    assert f"row-partitioned x{world}" in d["config"]["parallelism"] and len(d["config"]["parallelism"]) <= 160


@pytest.mark.parametrize("mode", ["1", "raise"])
def test_bench_multirank_watchdog_reports_the_conservative_measurement(mode):
    """The safety net of `bench.py --gpus N`: the plain schedule (torch.distributed all-gather per term, no second
    stream) is measured first; if the native / overlapped path then hangs (simulated: it sleeps) or fails on a rank
    (simulated: the last rank raises, the others wait for it in a collective), the watchdog prints the kept line from
    rank 0, marked `"degraded": true` with `native_path` = "hung" / "failed", and every rank exits with status 3: the
    driver still gets a complete, valid measurement, and nobody can mistake the run for a clean one."""
    world = 2
    d, full, outs = _bench(world, ["--steps", "3", "--warmup", "1", "--log2n", "16", "--watchdog", "20"], rc_expected=3, timeout=240,
                           QP_BENCH_TEST_HANG=mode)
    assert d["extras_file"] == "bench_extras_c4_gpus2.json"
    par = full["config"]["parallelism"]
    assert d["degraded"] is True and d["native_path"] == ("hung" if mode == "1" else "failed")
    assert d["n_gpus"] == world and d["steps"] == 3 and d["value"] > 0 and 0 < d["roofline"]["frac"] <= 1
    assert d["exchange"] == "halo" and d["rccl_ranks"] == 0
    assert "schedule=serial" in par and "driver=torch.distributed" in par
    assert "conservative schedule (reported because the native / overlapped path did not finish)" in par
    assert "schedule=serial" in d["config"]["parallelism"] and "driver=torch.distributed" in d["config"]["parallelism"]
    assert "reporting the conservative measurement" in outs[0][1]


@pytest.mark.parametrize("world", [1, 2, 8])
def test_bench_c5_batch_split_flow_one_gpu(world):
    """`bench.py --config c5 --gpus N`: the 64-state panel of BASELINE configs[4] split over N ranks (here sharing GPU 0),
    H replicated, no communication; one JSON line from rank 0 with the job's state-steps per second."""
    d, full, _ = _bench(world, ["--config", "c5", "--steps", "2", "--warmup", "1", "--log2n", "14", "--cpu-steps", "0"], timeout=300)
    assert d["extras_file"] == "bench_extras_c5" + (f"_gpus{world}" if world > 1 else "") + ".json"
    assert d["n_gpus"] == world and d["unit"] == "state_step/s" and d["config"]["states_per_gpu"] == 64 // world
    assert abs(full["value"] - 64 * 2 / (full["ms_per_step"] * 2e-3)) < 1e-6 * full["value"]
    assert abs(d["value"] - full["value"]) < 1e-5 * full["value"]
    assert 0 < d["roofline"]["frac"] <= 1.0 and d["max_norm_drift"] < 1e-10
    assert ("csr_spmm_kernel" in full["config"]["kernel"]) == (64 // world <= 32)
    assert d["roofline"]["kernel"] == ("csr_spmm_kernel" if 64 // world <= 32 else "spmm_tile_kernel")      # (the lattice's interior rows in LDS-staged tiles)
    if world == 1:
        assert full["config"]["lds_tiles"]["taken"] == 1 and full["config"]["lds_tiles"]["tiles"] * 16 + full["config"]["lds_tiles"]["rest_rows"] == 1 << 14
    assert d["cpu_baseline"] is None                    # --cpu-steps 0; `--config c5 --full` carries one (test below)


def test_bench_c5_line_carries_a_cpu_baseline():
    """`bench.py --config c5` on one GPU (small size): `cpu_baseline` = oracle/cheby_ref.c on a sample of the panel's states
    (same H, same coefficients, serial CSC path), in the line's unit, and the sampled states of the GPU panel agree with it."""
    d, full, _ = _bench(1, ["--config", "c5", "--steps", "2", "--warmup", "1", "--log2n", "14", "--cpu-steps", "2", "--no-pmc", "--full"],
                        timeout=300)
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["unit"] == "state_step/s" and cb["value"] > 0
    assert cb["l2_diff_vs_gpu_after_sample"] < 1e-10 and "states" in cb["sample"]
    assert full["cpu_baseline"]["states_sampled"] >= 1


def test_batched_panel_split_over_ranks_matches_oracle():
    """SURVEY 8e "Batched" / BASELINE configs[4]: a 64-state panel split as 64 / R states per rank (H replicated, zero
    communication) and reassembled equals the oracle's cheby! of every state (1e-10) and, bit for bit, the unsplit panel
    where both take the same kernel (R = 1 vs 2: wave-per-row kernel; R = 4, 8: the state-tiled one)."""
    sys.path.insert(0, ROOT)
    import qprop_amd.lib as L
    import qprop_amd.synth as synth
    import qprop_amd.sharded as sharded
    from oracle import qp_oracle as qo
    N, batch = 4096, 64
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=(1, 2, 3, 4, 64, 128, 192, 256))
    H = synth.to_scipy(rp, col, vals, N)
    states = np.stack([synth.random_state(N, seed=500 + s) for s in range(batch)], axis=1)
    ref = np.empty_like(states)
    for s_ in range(batch):
        psi = states[:, s_].copy()
        w = qo.ChebyWrk(psi, 20.0, -10.0, 0.7)
        qo.cheby(psi, H, 0.7, w)
        qo.cheby(psi, H, 0.7, w)
        ref[:, s_] = psi
    ctx = L.Context(0)
    results = {}
    for R in (1, 2, 4, 8):
        b = batch // R
        got = np.empty_like(states)
        for r in range(R):                      # what rank r of R does (its own context, operator and panel share)
            c = L.Context(0)
            bs = sharded.BatchSplitCheby(c, rp, col, vals, N, batch, 20.0, -10.0, 0.7, rank=r, world=R)
            assert (bs.s0, bs.s1, bs.b) == (r * b, (r + 1) * b, b)
            bs.set_states(states)
            bs.step()
            bs.step()
            got[:, bs.s0:bs.s1] = bs.local_states()
            bs.close()
            c.close()
        results[R] = got
        assert np.max(np.linalg.norm(got - ref, axis=0)) < 1e-10, R
    assert np.array_equal(results[1], results[2]) and np.array_equal(results[4], results[8])
    ctx.close()


def test_bench_single_gpu_line_is_physical():
    """bench.py on one GPU (small size): `roofline.frac` prices the shipped layout's bytes and stays below 1, the
    contract's CSR figure is reported separately, and `traffic` is measured in the run (child processes under
    rocprofv3 --pmc), not read from a file."""
    d, full, _ = _bench(1, ["--steps", "5", "--warmup", "1", "--cpu-steps", "0", "--log2n", "17", "--no-extras", "--full"], timeout=900)
    assert d["extras_file"] == "bench_extras_c2_n17.json"
    rf = full["roofline"]
    assert d["n_gpus"] == 1 and d["config"]["N_total"] == 1 << 17
    assert abs(full["value"] - full["config"]["global_steps_per_s"] / 8) < 1e-9 * full["value"] and abs(d["value"] - full["value"]) < 1e-5 * full["value"]
    assert 0 < rf["frac"] <= 1.0 and abs(d["roofline"]["frac"] - rf["frac"]) < 1e-5
    assert rf["layout_bytes_per_launch"] < rf["csr_equivalent_bytes_per_launch"] == (20 * 16 + 84) * (1 << 17) + 4
    assert abs(d["roofline"]["bytes_per_launch"] - rf["layout_bytes_per_launch"]) < 1e-5 * rf["layout_bytes_per_launch"]
    assert rf["traffic_source"].startswith("measured in this run"), rf["traffic_source"]
    assert d["roofline"]["traffic_measured"] is True
    assert 0.3 * rf["layout_bytes_per_launch"] < rf["traffic"] < 3.0 * rf["layout_bytes_per_launch"]
    assert rf["traffic_detail"]["dispatches"][0] >= 31
    # a working set the Infinity Cache holds is labelled as such (the bound stays one of the contract's two words)
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["cache_resident"] is True


def test_bench_config_c4_on_one_gpu_is_the_fixed_problem():
    """`bench.py --gpus 1 --config c4`: config C4's N = 2^24 on ONE GPU, the denominator of ">= 6 x at 8 GPUs vs 1 at fixed
    problem" (BASELINE.md section 2); here with the size overridden, to check the flow: the rows are all on this GPU, the value
    counts 2^20-row blocks, and the timed region reports its quarters."""
    d, full, _ = _bench(1, ["--config", "c4", "--log2n", "18", "--steps", "8", "--warmup", "1", "--cpu-steps", "0", "--no-pmc", "--no-extras"],
                        timeout=600)
    assert d["extras_file"] == "bench_extras_c4_n18.json"
    assert d["n_gpus"] == 1 and d["config"]["N_total"] == 1 << 18 == d["config"]["rows_per_gpu"] and "configs[3]" in d["config"]["workload"]
    assert abs(full["value"] - 0.25 * full["config"]["global_steps_per_s"]) < 1e-9 * full["value"]
    rf = full["roofline"]
    assert len(rf["launch_us_segments"]) == 4 and rf["unstable"] in (False, True) and 0 < rf["frac"] <= 1.0
    assert list(d["roofline"])[:8] == ["bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_us"]     # the gate scalars lead


def test_bench_plain_run_is_the_headline_alone_and_dumps_its_state(tmp_path):
    """`bench.py` without `--full`, at the headline config (where `--full` adds the extra points, the CPU baselines, the PMC passes
    and the stream yardsticks), measures the headline and nothing else, times exactly --steps steps, and `--dump-outputs DIR`
    writes the state after the last timed step: the oracle's state after warmup + steps prop_steps from the same seeded input."""
    sys.path.insert(0, ROOT)
    import qprop_amd.synth as synth
    from oracle import qp_oracle as qo
    warmup, steps = 2, 3
    d, full, _ = _bench(1, ["--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)], timeout=300)
    assert d["extras_file"] == "bench_extras.json" and d["config"]["N_total"] == 1 << 20       # the default run, the headline config
    assert d["steps"] == steps and d["warmup"] == warmup and d["ms_per_step"] > 0
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-4 * d["value"]
    assert d["cpu_baseline"] is None and "points" not in d and full["extras"] is None and full["cpu_baseline_all_cores"] is None
    rf = full["roofline"]
    assert rf["traffic_source"].startswith("STATIC") and d["roofline"]["traffic_measured"] is False     # no rocprofv3 child runs
    assert rf["stream_read_gbs"] is None and rf["hbm_resident_frac"] is None
    N = 1 << 20
    got = np.load(tmp_path / "psi.npy")
    assert got.dtype == np.float64 and got.shape == (N, 2) and sorted(os.listdir(tmp_path)) == ["psi.npy"]
    rp, col, vals = synth.hermitian_offsets_csr(N, offsets=synth.BANDED_OFFSETS)
    H = synth.to_scipy(rp, col, vals, N)
    psi = synth.random_state(N, row_begin=0, row_end=N)
    wrk = qo.ChebyWrk(psi, 20.0, -10.0, 1.0)
    for _ in range(warmup + steps):
        psi = qo.cheby(psi, H, 1.0, wrk)
    assert np.linalg.norm(got[:, 0] + 1j * got[:, 1] - psi) < 1e-10


def test_bench_extras_points_are_physical():
    """The measurement functions behind bench.py's `extras` (tools/bench_points.py), at small sizes: every `frac` is a physical
    fraction of the 8 TB/s roofline (bytes the implementation moves / time) and names its byte model, the SURVEY 8d model of the
    Newton sweep is reported beside it under its own key, an open-boundary grid takes the strip walk after the lattice completion."""
    import qprop_amd.lib as L
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_points as bp
    ctx = L.Context(0)
    try:
        ctx.tuning_set("walk_min_blocks", 64)
        r = bp.measure_newton_c3(ctx, n=96, m=12, steps=3, warmup=3)
        assert 0 < r["frac"] <= 1.0 and r["frac"] == r["implementation_frac"] and r["frac_survey_8d_model"] > r["frac"]
        assert r["launches_per_column"] < 2.6 and r["model"] == "impl"
        g = bp.measure_cheby(ctx, grid=(128, 96), steps=2, warmup=1)
        assert 0 < g["frac"] <= 1.0 and g["kernel"] == "hrb_walk_kernel" and g["explicit_zeros_completing_the_lattice"] > 0
        assert g["model"] == "layout"
        g3 = bp.measure_cheby(ctx, grid=(64, 12, 40), steps=2, warmup=1)
        assert 0 < g3["frac"] <= 1.0 and g3["kernel"] == "hrb_walk_kernel" and g3["strip_walk"]["long_distance"] == 64 * 12
        b = bp.measure_cheby(ctx, pattern="banded", log2n=16, steps=2, warmup=1)
        assert 0 < b["frac"] <= 1.0
    finally:
        ctx.close()


def test_c_consumer_runs(tmp_path):
    """examples/c_abi_demo.c -- a plain-C program on the C ABI, no Python / torch in the process: its own
    checks (norm, Newton == Cheby, forward + backward = identity, the reference's dt assertion) pass."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_c_consumer import _build
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=180)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "C ABI demo ok" in r.stdout and "QP_E_DT_MISMATCH" in r.stdout
