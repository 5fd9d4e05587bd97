"""Loss scaling, overflow skip and norm clipping of the fused AdamW step without a GPU: the numpy restatement (ccrec_amd/optim_ref.py:
grad_sumsq_partials, control_update, adamw_step_scaled -- the kernels' bit-exact oracle) against torch's own arithmetic on the CPU
(unscale by 1 / scale, clip_grad_norm_, torch.optim.AdamW; torch._amp_update_scale_ for the scale), LossScaler's state dict, the new
entry points' argument checks (they return before any device call) and the host-side logic (tests/native/optim_amp_plan_check.cpp).

Bars of the restatement against torch: those of tests/test_cpu_optim.py (four fp32 spacings at the largest magnitude of each stored
quantity), widened by what a relative difference eps_g between the two EFFECTIVE gradients allows.  torch rounds a gradient twice (unscale,
clip) and forms the norm in fp32; the restatement rounds it once, g * coef, under a norm summed in double from fp32 chunk sums.
  eps_g = OURS + THEIRS, in units of 2^-24 (half a spacing, the bound of one rounding):
    OURS = 19: a chunk sum is a tree of depth 16 (thread) + 6 (wave) + 2 (waves) over squares rounded once, 25 roundings on the sum of
           squares and half of that, 12.5, on its root; then one each for the root's conversion to fp32, norm * inv, norm + 1e-6, the
           division, inv * clip and g * coef: 18.5 (the double-precision sum adds 2^-53 per term, far below the half kept in reserve)
    THEIRS: measured in the test against the same gradient formed in float64 (the reference's own error)
  exp_avg    moves by at most eps_g * max |g|      (its weights (1 - b1) * b1^k sum to less than 1)
  exp_avg_sq moves by at most 2 * eps_g * (1 + eps_g) * max g^2
  p          moves by at most t * lr * 4 * eps_g after t <= 3 steps: with every |g| of a coordinate within the test's range, sqrt(v^) is
             at least 0.57 of the coordinate's largest |g| in its first three steps, so m^ / sqrt(v^) moves by less than 1.75 eps_g
             through m^ and as much through v^.
The test prints the observed error in spacings next to each bar (DESIGN 4.8o quotes both)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG

EPS_F32 = 2.0 ** -23
BETAS, EPS = (0.9, 0.999), 1e-8
OURS_HALF_SPACINGS = 19.0
SHAPES = ((33, 7), (4097,), (1,), (64, 64), (3,), (5000,), (255,), (8193,), (12, 5), (4096,))


@pytest.mark.parametrize("max_norm", [0.05, 1e3])       # the clip at work, and idle (the factor is exactly 1)
@pytest.mark.parametrize("scale", [65536.0, 1000.0])    # a power of two (the unscale is exact) and a scale whose reciprocal is rounded
def test_restatement_tracks_unscale_clip_and_torch_adamw(scale, max_norm):
    from ccrec_amd import optim_ref
    lr, wd, steps = 1e-3, 0.01, 3
    gen = torch.Generator().manual_seed(int(scale) + int(max_norm * 100))
    params = [torch.nn.Parameter(torch.randn(*s, generator=gen) * 0.05) for s in SHAPES]
    opt = torch.optim.AdamW(params, lr=lr, weight_decay=wd, foreach=False)
    state = [(p.detach().numpy().copy(), np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32)) for p in params]
    inv = torch.tensor(scale, dtype=torch.float32).double().reciprocal().float()      # GradScaler.unscale_'s inverse
    gmax, worst, clipped = 0.0, [0.0, 0.0, 0.0], 0
    for t in range(1, steps + 1):
        true = [torch.randn(*s, generator=gen) * 1e-2 for s in SHAPES]
        scaled = [g * scale for g in true]      # what backward() of the scaled loss leaves
        for p, g in zip(params, scaled):
            p.grad = g * inv
        total = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
        # THEIRS: torch's effective gradient against the same quantity in float64
        g64 = [g.double().numpy() / scale for g in scaled]
        norm64 = float(np.sqrt(sum(float((x * x).sum()) for x in g64)))
        clip64 = min(1.0, max_norm / (norm64 + 1e-6))
        theirs = max(float(np.abs(p.grad.double().numpy() - x * clip64).max() / np.abs(x * clip64).max()) for p, x in zip(params, g64))
        eps_g = OURS_HALF_SPACINGS * 2.0 ** -24 + theirs
        opt.step()
        ctl = optim_ref.control_update(optim_ref.grad_sumsq_partials([g.numpy() for g in scaled]), scale, 0, max_norm, 2.0, 0.5, 2000)
        assert ctl["skip"] == 0 and ctl["scale"] == np.float32(scale) and ctl["tracker"] == 1
        assert abs(float(ctl["norm"]) - float(total)) <= 2 * eps_g * float(total)
        clipped += float(ctl["coef"]) < float(inv)
        if max_norm >= 1e3:
            assert ctl["coef"] == np.float32(inv.item())
        gmax = max(gmax, max(float(np.abs(x * clip64).max()) for x in g64))      # of the effective (unscaled, clipped) gradients
        for i, p in enumerate(params):
            state[i] = optim_ref.adamw_step_scaled(*state[i][:1], scaled[i].numpy(), *state[i][1:], t, lr, wd, BETAS, EPS, ctl["coef"], 0)
            st = opt.state[p]
            got = (p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy())
            plain = (4 * EPS_F32 * float(np.abs(got[0]).max()), 4 * EPS_F32 * gmax, 4 * EPS_F32 * gmax * gmax)
            bars = (plain[0] + t * lr * 4 * eps_g, plain[1] + eps_g * gmax, plain[2] + 2 * eps_g * (1 + eps_g) * gmax * gmax)
            for k in range(3):
                err = float(np.abs(state[i][k] - got[k]).max())
                worst[k] = max(worst[k], err / (plain[k] / 4))
                assert err <= bars[k], (("p", "exp_avg", "exp_avg_sq")[k], t, i, err, bars[k])
    assert clipped == (steps if max_norm < 1 else 0)
    print(f"scaled restatement vs torch (unscale, clip_grad_norm_, AdamW), scale {scale:g}, max_norm {max_norm:g}: worst error in fp32 spacings "
          f"p {worst[0]:.3f} exp_avg {worst[1]:.3f} exp_avg_sq {worst[2]:.3f}; bars {4 + 0:.0f} + widening "
          f"(eps_g = {eps_g / EPS_F32:.2f} spacings, of which torch's own {theirs / EPS_F32:.2f})")


def test_skip_leaves_everything_and_coef_one_is_the_plain_step():
    from ccrec_amd import optim_ref
    rng = np.random.default_rng(0)
    p, g, m, v = (rng.standard_normal(1000).astype(np.float32) * s for s in (0.05, 1e-2, 1e-3, 1e-5))
    v = np.abs(v)
    for a, b in zip(optim_ref.adamw_step_scaled(p, g, m, v, 3, 1e-3, 0.01, BETAS, EPS, np.float32(0.25), 1), (p, m, v)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and a is not b
    for a, b in zip(optim_ref.adamw_step_scaled(p, g, m, v, 3, 1e-3, 0.01, BETAS, EPS, np.float32(1.0), 0), optim_ref.adamw_step(p, g, m, v, 3, 1e-3, 0.01, BETAS, EPS)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    half = optim_ref.adamw_step_scaled(p, g, m, v, 3, 1e-3, 0.01, BETAS, EPS, np.float32(0.5), 0)
    for a, b in zip(half, optim_ref.adamw_step(p, g * np.float32(0.5), m, v, 3, 1e-3, 0.01, BETAS, EPS)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_partials_follow_the_documented_order_and_every_overflow_skips():
    from ccrec_amd import optim_ref
    rng = np.random.default_rng(1)
    g = rng.standard_normal(4096 + 7).astype(np.float32)
    parts = optim_ref.grad_sumsq_partials([g, np.zeros(0, np.float32), g[:3]])
    assert parts.dtype == np.float32 and parts.shape == (3,)
    # chunk 0 by hand, one thread, wave and workgroup at a time
    sq = g[:4096] * g[:4096]
    threads = np.zeros(256, np.float32)
    for t in range(256):
        acc = np.float32(0.0)
        for k in range(4):
            for e in range(4):
                acc = acc + sq[1024 * k + 4 * t + e]
        threads[t] = acc
    waves = []
    for w in range(4):
        x = threads[64 * w:64 * w + 64].copy()
        for h in (32, 16, 8, 4, 2, 1):
            x = x[:h] + x[h:2 * h]
        waves.append(x[0])
    assert parts[0] == ((waves[0] + waves[1]) + waves[2]) + waves[3]
    tail = g[4096:] * g[4096:]
    assert parts[1] == ((tail[0] + tail[1]) + tail[2]) + tail[3] + ((tail[4] + tail[5]) + tail[6])      # thread 0's four, thread 1's three
    assert parts[2] == (sq[0] + sq[1]) + sq[2]
    assert abs(float(optim_ref.partials_sum(parts)) - float((g.astype(np.float64) ** 2).sum() + (g[:3].astype(np.float64) ** 2).sum())) < 1e-3
    # 300 partials: 256 slices of two, the slice sums in order
    many = rng.random(300).astype(np.float32)
    by_hand = 0.0
    for t in range(150):
        by_hand = by_hand + (float(many[2 * t]) + float(many[2 * t + 1]))
    assert optim_ref.partials_sum(many) == by_hand
    for bad in (np.inf, -np.inf, np.nan, 3e19):
        h = g.copy()
        h[-1] = bad
        ctl = optim_ref.control_update(optim_ref.grad_sumsq_partials([h]), 65536.0, 5, 1.0, 2.0, 0.5, 2000)
        assert ctl["skip"] == 1 and ctl["scale"] == 32768.0 and ctl["tracker"] == 0, bad
        assert optim_ref.control_update(optim_ref.grad_sumsq_partials([h]), None, 0, None, 2.0, 0.5, 2000)["skip"] == 1
    fine = optim_ref.grad_sumsq_partials([g])
    assert optim_ref.control_update(fine, None, 0, None, 2.0, 0.5, 1, ext_found_inf=1.0, ext_scale=8.0)["skip"] == 1
    ext = optim_ref.control_update(fine, None, 0, None, 2.0, 0.5, 1, ext_found_inf=0.0, ext_scale=8.0)
    assert ext["skip"] == 0 and ext["coef"] == np.float32(0.125) and ext["scale"] is None
    assert ext["norm"] == np.float32(np.sqrt(optim_ref.partials_sum(fine))) * np.float32(0.125)
    for no_clip in (None, 0.0, -1.0, np.inf):
        assert optim_ref.control_update(fine, 4.0, 0, no_clip, 2.0, 0.5, 7)["coef"] == np.float32(0.25)


def test_scale_update_rule_is_torchs_amp_update_scale():
    """Grow at the interval, back off, refuse a growth that would overflow -- step by step against torch._amp_update_scale_ on the CPU."""
    from ccrec_amd import optim_ref
    finite, overflow = np.array([1.0], np.float32), np.array([np.inf], np.float32)
    for init, growth, backoff, interval, flags in ((65536.0, 2.0, 0.5, 3, [0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0]),
                                                   (3e38, 2.0, 0.5, 2, [0, 0, 0, 0, 1, 0, 0, 0, 0]),
                                                   (1000.0, 1.7, 0.3, 1, [0, 0, 1, 0, 1, 1, 0])):
        scale_t, tracker_t = torch.tensor(init, dtype=torch.float32), torch.tensor(0, dtype=torch.int32)
        scale, tracker = np.float32(init), 0
        for found in flags:
            torch._amp_update_scale_(scale_t, tracker_t, torch.tensor(float(found)), growth, backoff, interval)
            ctl = optim_ref.control_update(overflow if found else finite, scale, tracker, None, growth, backoff, interval)
            scale, tracker = ctl["scale"], ctl["tracker"]
            assert ctl["skip"] == found and scale == scale_t.numpy() and tracker == int(tracker_t), (init, found, scale, scale_t, tracker, tracker_t)
        if init == 3e38:
            assert scale == np.float32(1.5e38) * np.float32(2.0)      # 3e38 * 2 refused twice; backed off to 1.5e38; grown once; refused again
    grown = optim_ref.control_update(finite, 3e38, 1, None, 2.0, 0.5, 2)
    assert grown["scale"] == np.float32(3e38) and grown["tracker"] == 0


def test_loss_scaler_state_dict_moves_to_torch_grad_scaler_and_back():
    from ccrec_amd import optim
    mine = optim.LossScaler(init_scale=1024.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=17)
    sd = mine.state_dict()
    assert set(sd) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    theirs = torch.amp.GradScaler("cpu")
    assert set(theirs.state_dict()) == set(sd)
    theirs.load_state_dict(sd)
    assert theirs.state_dict() == sd and theirs.get_scale() == 1024.0 and theirs.get_growth_interval() == 17
    src = torch.amp.GradScaler("cpu", init_scale=2.0 ** 12, growth_factor=1.5, backoff_factor=0.75, growth_interval=5).state_dict()
    src["_growth_tracker"] = 3
    back = optim.LossScaler()
    back.load_state_dict(src)
    assert back.state_dict() == src and back.get_scale() == 4096.0
    again = torch.amp.GradScaler("cpu")
    again.load_state_dict(back.state_dict())
    assert again.state_dict() == src
    mine.update()      # a no-op kept for the call sites
    with pytest.raises(ValueError):
        optim.LossScaler(growth_factor=1.0)
    with pytest.raises(TypeError, match="FusedAdamW"):
        mine.step(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]))


def test_constructor_takes_max_grad_norm_and_keeps_the_plain_path():
    from ccrec_amd import optim
    p = torch.nn.Parameter(torch.zeros(4, 4))
    opt = optim.FusedAdamW([p], max_grad_norm=1.0, _host_state_only=True)
    assert opt.max_grad_norm == 1.0 and opt.last_grad_norm is None and opt._step_supports_amp_scaling is True
    assert optim.FusedAdamW([p], _host_state_only=True).max_grad_norm is None
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            optim.FusedAdamW([p], max_grad_norm=bad, _host_state_only=True)
    opt.settle()      # nothing pending: no event, no wait
    assert opt._pending is None and opt._skip_host is None
    assert set(opt.param_groups[0]) == set(torch.optim.AdamW([p]).param_groups[0])      # max_grad_norm is no group key: state dicts still move


def test_library_version_exports_and_argument_checks_without_a_device():
    from ccrec_amd import _lib, ops
    new = {"ccr_grad_stats_workspace_bytes", "ccr_grad_stats", "ccr_adamw_control_update", "ccr_adamw_step_scaled"}
    assert _lib.AMP_OPTIM_VERSION == 110 and new <= set(_lib.EXPORTS) and callable(ops._require_optim_amp)
    header = open(os.path.join(ROOT, "include", "ccr_retrieval.h")).read()
    assert all(name + "(" in header for name in new) and "typedef struct ccr_adamw_control {" in header
    lib = _lib.load()
    assert lib.ccr_version() >= 110
    assert ctypes.sizeof(_lib.AdamwControl) == 64 and _lib.CONTROL_WORDS == {"coef": 0, "skip": 1, "norm": 2, "scale": 3, "growth_tracker": 4, "skipped_total": 5}
    assert lib.ccr_grad_stats_workspace_bytes(None, 0) == 0 and lib.ccr_grad_stats_workspace_bytes(None, 2) == -1
    segs = (_lib.AdamwSegment * 3)()
    fake = 1 << 20      # made-up addresses: none of these calls reaches a launch
    for s, n in zip(segs, (4096, 0, 4097)):
        s.param = s.grad = s.exp_avg = s.exp_avg_sq = fake
        s.n = n
    assert lib.ccr_grad_stats_workspace_bytes(segs, 3) == 4 * 3
    assert lib.ccr_grad_stats(None, 0, None, None) == _lib.CCR_OK
    assert lib.ccr_grad_stats(None, -1, None, None) == _lib.CCR_ERR_INVALID
    assert lib.ccr_grad_stats(segs, 3, None, None) == _lib.CCR_ERR_INVALID and b"partials is NULL" in lib.ccr_last_error()
    segs[2].n = -5
    assert lib.ccr_grad_stats(segs, 3, fake, None) == _lib.CCR_ERR_INVALID
    assert b"segment 2" in lib.ccr_last_error() and b"n < 0" in lib.ccr_last_error()
    assert lib.ccr_grad_stats_workspace_bytes(segs, 3) == -1
    assert lib.ccr_adamw_step_scaled(segs, 3, 0.1, 0.999, 0.001, 1e-8, fake, None) == _lib.CCR_ERR_INVALID
    segs[2].n = 0
    assert lib.ccr_adamw_step_scaled(segs, 3, 0.1, 0.999, 0.001, 1e-8, None, None) == _lib.CCR_ERR_INVALID and b"control is NULL" in lib.ccr_last_error()
    assert lib.ccr_adamw_step_scaled(None, 0, 0.1, 0.999, 0.001, 1e-8, fake, None) == _lib.CCR_OK      # nothing to launch
    assert lib.ccr_adamw_control_update(None, fake, 3, 1.0, 0, 2.0, 0.5, 2000, None, None, None) == _lib.CCR_ERR_INVALID
    assert lib.ccr_adamw_control_update(fake, None, 3, 1.0, 0, 2.0, 0.5, 2000, None, None, None) == _lib.CCR_ERR_INVALID
    assert lib.ccr_adamw_control_update(fake, fake, -1, 1.0, 0, 2.0, 0.5, 2000, None, None, None) == _lib.CCR_ERR_INVALID
    assert lib.ccr_adamw_control_update(fake, fake, 3, 1.0, 1, 2.0, 0.5, 2000, fake, None, None) == _lib.CCR_ERR_INVALID and b"own_scale" in lib.ccr_last_error()
    assert lib.ccr_adamw_control_update(fake, fake, 3, 1.0, 1, 2.0, 0.5, 0, None, None, None) == _lib.CCR_ERR_INVALID


def test_partial_index_and_workspace_logic_on_cpu(tmp_path):
    """tests/native/optim_amp_plan_check.cpp over csrc/ccr_optim_plan.h: the global chunk index of every partial across launch batches
    (the GPU test's lists, lists with empty segments, BERT-base), the workspace size, the control kernel's slices."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not (os.path.isabs(cxx) and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "optim_amp_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "native", "optim_amp_plan_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = run.stdout.strip().splitlines()
    assert lines[-1].endswith(", 0 violations") and int(lines[-1].split()[0]) > 1000, lines[-1]
    bert = [ln for ln in lines if ln.startswith("BERT-base:")][0]
    assert "199 tensors, 26823 partials, 107292 workspace bytes" in bert, bert
