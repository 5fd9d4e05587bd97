"""The rank and the tile cap of estimated thresholds as the planner picks them (ccr::make_plan, csrc/ccr_plan.hip: optimistic_rank,
tile_cap_for) are host code -- tests/native/tile_cap_plan_check.cpp walks a grid of shapes and prints the plans read here.  No GPU call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crowd-coachable-recommendations_amd")


def test_rank_and_tile_cap_of_the_planner_on_cpu(tmp_path):
    """Over 840 plans (every shape at the default knobs and with CCR_OPTIMISTIC=1): an estimated threshold has a rank of at least 17 -- below
    40 only where the plan leaves out the sampled tiles of a sample of forty tiles or more --, capacities sized for rank 40 at least, a
    cap within 4 .. 16 with cap x 5 >= rank (16 = no cap), a rank above 4 x cap -- five tiles settle it at least -- and at least ten
    sampled tiles that hold the rank under the cap; a plan without estimated thresholds has no cap.
    The flagship shape (2 681 468 x 768, 3 452 queries): k = 100 -> rank 18, cap 4 on the 1/32 sample (rank 40, cap 8 when every tile is
    scored); k = 1001 -> rank 42 on the 1/64 sample as before, cap 9.  CCR_OPT_RANK and CCR_TILE_CAP are honoured; a pinned cap is raised
    to what leaves the rank among the capped groups (cap 1 on ten tiles at rank 17: 2); seventeen sampled tiles keep rank 40, four
    sampled tiles are not estimated from."""
    from ccrec_amd import _lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "tile_cap_plan_check"
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = [hipcc, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "native", "tile_cap_plan_check.cpp"), "-o", str(exe), "-L", libdir, "-lccr_hip", f"-Wl,-rpath,{libdir}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:]
    lines = run.stdout.strip().splitlines()
    assert lines[-1].endswith(", 0 violations") and int(lines[-1].split()[0]) > 800 and int(lines[-1].split("(")[1].split()[0]) > 300, lines[-1]
    want = {
        "NQ k=100": "fused 1 rank 18 cap 4 sample 328 skip_sampled 1 phases 0/0",
        "NQ k=1001": "fused 1 rank 42 cap 9 sample 164 skip_sampled 0 phases 0/0",
        "NQ k=100, CCR_SKIP_SAMPLED=0": "fused 1 rank 40 cap 8 sample 328 skip_sampled 0 phases 0/0",
        "NQ k=100, CCR_TILE_CAP=16": "fused 1 rank 18 cap 16 sample 328 skip_sampled 1 phases 0/0",
        "NQ k=100, CCR_OPT_RANK=13 CCR_TILE_CAP=16": "fused 1 rank 13 cap 16 sample 164 skip_sampled 1 phases 0/0",
        "NQ k=100, CCR_OPT_RANK=40": "fused 1 rank 40 cap 8 sample 328 skip_sampled 1 phases 0/0",
        "17 sampled tiles, CCR_TILE_CAP=1": "fused 1 rank 17 cap 1 sample 17 skip_sampled 0 phases 0/0",
        "10 sampled tiles, CCR_TILE_CAP=1": "fused 1 rank 17 cap 2 sample 10 skip_sampled 0 phases 0/0",
        "17 sampled tiles": "fused 1 rank 40 cap 8 sample 17 skip_sampled 0 phases 0/0",
        "4 sampled tiles": "fused 1 rank 0 cap 16 sample 4 skip_sampled 0 phases 0/0",
    }
    for what, plan in want.items():
        got = [ln for ln in lines if ln.startswith(what + ": ")]
        assert got and got[0] == f"{what}: {plan}", (what, got)
