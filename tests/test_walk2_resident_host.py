"""CPU-side checks of the two-term strip walk's cut and rule for operators inside the Infinity Cache (csrc/walk_geometry.cpp:
walk2_cut_resident, walk2_wanted_resident, walk2_rule): tests/walk2_resident_host.cpp, a stand-alone program built from the pure-host
geometry unit alone with g++ -fsanitize=address,undefined.  Nothing is loaded into Python."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resident_pair_cut_and_rule_on_the_host(tmp_path):
    """Over CU counts {8, 64, 256}, walk_waves {0, 1, 64, 4096}, every edge-step setting and the plans of three lattices: every
    strip step of the two-term region lies in exactly one segment by hrb_walk2_kernel's own formulas (shortened segments included),
    ntask = 4 n_walk_wg >= nseg S2, edge_segs <= nseg, L > edge_steps.  The rule on named inputs: the headline at N = 2^20 on 256
    compute units is wanted, the (4, 4) lattices of 2^15 - 2^16 rows are not, N = 2^22 stays with the streamed rule, walk_pair = 0
    never takes pairs.  walk2_cut / walk2_wanted return what tests/walk_geometry_cases.h pins."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    csrc = os.path.join(ROOT, "quantumpropagators.jl_amd", "csrc")
    exe = str(tmp_path / "walk2_resident_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", csrc, os.path.join(ROOT, "tests", "walk2_resident_host.cpp"), os.path.join(csrc, "walk_geometry.cpp"),
                            "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "resident walk2 geometry clean" in run.stdout
    cuts = re.search(r"resident cut: (\d+) cuts of 3 lattice plans hold the kernel's segment formulas \((\d+) with every segment shortened\)", run.stdout)
    assert cuts and int(cuts.group(1)) >= 3 * 4 * 3 * 4 and int(cuts.group(2)) >= 1, run.stdout
    rules = re.search(r"resident rule: (\d+) named cases match the table", run.stdout)
    assert rules and int(rules.group(1)) >= 12, run.stdout
