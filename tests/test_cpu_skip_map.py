"""The main pass that leaves out the sampled tiles (CCR_SKIP_SAMPLED): its map from virtual to real tiles (ccr::unsampled_tile) and
the plans that switch it on (ccr::make_plan, csrc/ccr_plan.hip) are host code -- tests/native/skip_map_check.cpp checks both.  No GPU call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crowd-coachable-recommendations_amd")


def test_skip_map_and_plans_on_cpu(tmp_path):
    """t(v) over a sweep of (tiles, stride, sampled tiles) -- s = 2, n = 1, n * s at and just below the tile count, NQ's (10475, 31, 328) --
    is strictly ascending, never a sampled tile and hits every other tile once; at the default knobs NQ at k = 100 leaves out the
    sampled tiles, the conservative, phased, streaming and forced-dense plans do not.  NQ at k = 1001 leaves them out when
    CCR_SKIP_SAMPLED=1 pins it; the planner's own choice scores every tile there, as measured (profiles/skip_sampled.md: the search
    was 0.36 ms slower with the skip, which the issue answers with "leave that k off the skip in the planner")."""
    from ccrec_amd import _lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "skip_map_check"
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = [hipcc, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "native", "skip_map_check.cpp"), "-o", str(exe), "-L", libdir, "-lccr_hip", f"-Wl,-rpath,{libdir}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.endswith(", 0 violations") and int(last.split()[0]) > 200, last
    lines = run.stdout.splitlines()
    for what, want in (("NQ k=100:", 1), ("NQ k=1001:", 0), ("NQ k=100, CCR_SKIP_SAMPLED=1:", 1), ("NQ k=1001, CCR_SKIP_SAMPLED=1:", 1)):
        assert [ln for ln in lines if ln.startswith(what)][0].endswith(f"skip_sampled {want}"), what
