"""Plans whose single-launch main pass leaves CUs to the caller's side work (ccr::make_plan with the side hint, CCR_SIDE_CUS;
csrc/ccr_plan.hip) are host code -- tests/native/side_cus_plan_check.cpp walks the shapes of planner_check.cpp and prints what is read
here.  No GPU call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crowd-coachable-recommendations_amd")


def test_side_cus_plans_on_cpu(tmp_path):
    """256 CUs, every pinned count 0, 8 .. 64 and the planner's own choice over the shapes of planner_check.cpp: main_grid = grid -
    side_cus stays a multiple of 8; only one launch of a tile kernel leaves CUs free; without the hint, and wherever no CU is left free,
    the plan is the plan of CCR_SIDE_CUS=0 field for field; the walk of main_grid workgroups covers every (range, query block) cell
    exactly once and the ranges hold every tile once; the arrival counter lies in the flag line the search clears; the planner's own
    choice leaves the main pass at least 3/4 of the CUs and is 0 where its estimate of the main pass is shorter than the pack."""
    from ccrec_amd import _lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "side_cus_plan_check"
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = [hipcc, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "native", "side_cus_plan_check.cpp"), "-o", str(exe), "-L", libdir, "-lccr_hip", f"-Wl,-rpath,{libdir}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:]
    lines = run.stdout.strip().splitlines()
    last = lines[-1].split()
    assert lines[-1].endswith(", 0 violations") and int(last[0]) > 5000, lines[-1]
    assert int(lines[-1].split("(")[1].split()[0]) > 1000, lines[-1]   # the pin took effect on many plans
    # one query: the streaming kernel, never carved
    one = [ln for ln in lines if ln.startswith("one query: ")]
    assert one and one[0].startswith("one query: side_cus 0 main_grid 256 "), one
