"""Unequal query groups of the main pass (CCR_QSPLIT): the item map (ccr::main_item) and the plans that choose it (ccr::make_plan,
csrc/ccr_plan.hip) are host code -- tests/native/qsplit_map_check.cpp checks both.  No GPU call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crowd-coachable-recommendations_amd")


def test_qsplit_map_and_plans_on_cpu(tmp_path):
    """1 ... 40 query blocks in 2, 4 and 8 groups (a split wherever the groups leave blocks over), every range count up to 128, fewer
    tiles than ranges, as many and more, grids of 8 and 256 workgroups: every (range, block) cell is scored exactly once, every XCD set
    walks the same number of items and at most base + rem blocks, a shared block's item lies in a range its XCD walks anyway, and equal
    groups give the former formula item for item.  At the default knobs NQ (k = 100 and 1001) runs the wide tile in two unequal groups,
    6 980 queries keep the 256-tile, and phased, streaming and forced-dense plans and CCR_QSPLIT=0 keep equal groups."""
    from ccrec_amd import _lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "qsplit_map_check"
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = [hipcc, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "native", "qsplit_map_check.cpp"), "-o", str(exe), "-L", libdir, "-lccr_hip", f"-Wl,-rpath,{libdir}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout[-6000:])
    assert run.returncode == 0, run.stdout[-3000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.endswith(", 0 violations") and int(last.split()[0]) > 10000, last
    lines = run.stdout.splitlines()
    for what, want in (("NQ k=100:", 2), ("NQ k=1001:", 2), ("dim 768, 6980 queries:", 0), ("NQ k=100 conservative (phased):", 0),
                       ("NQ 40 queries (streaming):", 0), ("NQ forced dense:", 0), ("NQ k=100, CCR_QSPLIT=0:", 0), ("NQ k=1001, CCR_QSPLIT=0:", 0)):
        assert [ln for ln in lines if ln.startswith(what)][0].endswith(f", split {want}"), what
    assert " tile_q 256 " in [ln for ln in lines if ln.startswith("dim 768, 6980 queries:")][0]
    assert " tile_q 384 " in [ln for ln in lines if ln.startswith("NQ k=100:")][0]
