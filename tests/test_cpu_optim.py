"""The fused AdamW step without a GPU: the numpy restatement (ccrec_amd/optim_ref.py: the kernel's bit-exact oracle) against
torch.optim.AdamW on the CPU, the reference's parameter groups and schedule, FusedAdamW's refusals and state-dict interchange, the C
entry point's argument checks (they return before any device call) and the host-side batching (tests/native/optim_plan_check.cpp).

Bars of the restatement against torch (foreach=False, CPU): four spacings of fp32 at the largest magnitude of each stored quantity --
4 * 2^-23 * max |p| for p, 4 * 2^-23 * max |g| for exp_avg, 4 * 2^-23 * max g^2 for exp_avg_sq.  Both compute the same real-valued update;
torch rounds it along another path (lerp, addcmul, a step size divided in double), so the two drift by roundings of the stored value
itself, whatever the learning rate."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG

EPS_F32 = 2.0 ** -23
LR_PEAK, STEPS = 2e-5, 40


def _schedule(opt):
    from ccrec_amd import optim
    return torch.optim.lr_scheduler.LambdaLR(opt, optim.linear_warmup_lambda(int(STEPS * 0.1), STEPS))


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("gscale", [1e-6, 1e-3, 1.0])
def test_restatement_tracks_torch_adamw_within_four_spacings(gscale, wd):
    """40 steps under the reference's warm-up schedule (it starts at lr = 0)."""
    from ccrec_amd import optim_ref
    g = torch.Generator().manual_seed(int(gscale * 1e6) + int(wd * 100))
    p0 = torch.randn(4099, generator=g) * 0.05
    grads = [torch.randn(4099, generator=g) * gscale for _ in range(STEPS)]
    tp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([tp], lr=LR_PEAK, weight_decay=wd, foreach=False)
    sched = _schedule(opt)
    p, m, v = p0.numpy().copy(), np.zeros(4099, np.float32), np.zeros(4099, np.float32)
    worst = [0.0, 0.0, 0.0]
    for t, gr in enumerate(grads, start=1):
        lr = opt.param_groups[0]["lr"]
        assert (t == 1) == (lr == 0.0)
        tp.grad = gr.clone()
        opt.step()
        sched.step()
        p, m, v = optim_ref.adamw_step(p, gr.numpy(), m, v, t, lr, wd, (0.9, 0.999), 1e-8)
        st = opt.state[tp]
        gmax = max(float(x.abs().max()) for x in grads[:t])
        bars = (4 * EPS_F32 * float(np.abs(p).max()), 4 * EPS_F32 * gmax, 4 * EPS_F32 * gmax * gmax)
        errs = (np.abs(p - tp.detach().numpy()).max(), np.abs(m - st["exp_avg"].numpy()).max(), np.abs(v - st["exp_avg_sq"].numpy()).max())
        for i in range(3):
            worst[i] = max(worst[i], errs[i] / bars[i])
            assert errs[i] <= bars[i], (("p", "m", "v")[i], t, errs[i], bars[i])
    print(f"restatement vs torch AdamW, g scale {gscale:g}, wd {wd:g}: worst error / bar p {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")


def test_restatement_at_lr_zero_keeps_p_and_moves_the_moments():
    from ccrec_amd import optim_ref
    rng = np.random.default_rng(0)
    p, g = rng.standard_normal(1000).astype(np.float32), rng.standard_normal(1000).astype(np.float32)
    m = v = np.zeros(1000, np.float32)
    for wd in (0.0, 0.01):
        p1, m1, v1 = optim_ref.adamw_step(p, g, m, v, 1, 0.0, wd, (0.9, 0.999), 1e-8)
        assert np.array_equal(p1.view(np.uint32), p.view(np.uint32))
        assert np.array_equal(m1, np.float32(1.0 - 0.9) * g) and np.array_equal(v1, (np.float32(1.0 - 0.999) * g) * g)
    decay, step_size, bc2 = optim_ref.segment_scalars(1, 0.0, 0.01, (0.9, 0.999))
    assert decay == 1.0 and step_size == 0.0 and bc2 == np.float32(np.sqrt(1.0 - 0.999))
    decay, step_size, bc2 = optim_ref.segment_scalars(1000, 2e-5, 0.01, (0.9, 0.999))
    assert decay == np.float32(1.0 - 2e-7) and step_size == np.float32(2e-5 / (1.0 - 0.9 ** 1000)) and bc2 == np.float32(np.sqrt(1.0 - 0.999 ** 1000))


def test_restatement_propagates_nan_and_infinities():
    from ccrec_amd import optim_ref
    p, m, v = np.ones(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32)
    g = np.array([0.0, np.inf, -np.inf, np.nan], np.float32)
    p1, m1, v1 = optim_ref.adamw_step(p, g, m, v, 1, 1e-3, 0.0, (0.9, 0.999), 1e-8)
    assert p1[0] == 1.0 and m1[0] == 0.0 and v1[0] == 0.0                   # g = 0: 0 / (0 + eps)
    assert np.isinf(m1[1]) and np.isinf(v1[1]) and np.isnan(p1[1])          # inf / inf
    assert m1[2] == -np.inf and v1[2] == np.inf and np.isnan(p1[2])
    assert np.isnan(m1[3]) and np.isnan(v1[3]) and np.isnan(p1[3])


def test_shadow_bits_are_torchs_round_to_nearest_even():
    from ccrec_amd import optim_ref
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-8, 5, 4096).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65520.0, 65519.99, 7e4, -7e4,
                                  6e-8, 2.9e-8, 3.0e-8, 1e-40, 3.3895e38, 3.4e38, np.inf, -np.inf], np.float32)])
    t = torch.from_numpy(x)
    assert np.array_equal(optim_ref.shadow_bits(x, "bf16"), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(optim_ref.shadow_bits(x, "fp16"), t.to(torch.float16).view(torch.int16).numpy().view(np.uint16))
    nan = np.array([np.nan, -np.nan], np.float32)
    assert ((optim_ref.shadow_bits(nan, 1) & 0x7FFF) > 0x7F80).all() and ((optim_ref.shadow_bits(nan, 2) & 0x7FFF) > 0x7C00).all()
    with pytest.raises(ValueError):
        optim_ref.shadow_bits(x, "fp8")


def _names(kind):
    if kind == "bert":
        from transformers import BertConfig, BertModel
        m = BertModel(BertConfig(vocab_size=50, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=64, max_position_embeddings=16))
    else:
        from transformers import DistilBertConfig, DistilBertModel
        m = DistilBertModel(DistilBertConfig(vocab_size=50, dim=64, n_layers=2, n_heads=1, hidden_dim=64, max_position_embeddings=16))
    return m


@pytest.mark.parametrize("kind", ["bert", "distilbert"])
def test_bert_mt_groups_follow_the_references_substring_rule(kind):
    from ccrec_amd import optim
    model = _names(kind)
    named = [("item_tower.cls_model." + n, p) for n, p in model.named_parameters()]
    decayed, plain = optim.bert_mt_groups(named, 0.01)
    assert decayed["weight_decay"] == 0.01 and plain["weight_decay"] == 0.0
    ids = {id(p): n for n, p in named}
    dn, pn = {ids[id(p)] for p in decayed["params"]}, {ids[id(p)] for p in plain["params"]}
    assert dn | pn == set(ids.values()) and not dn & pn
    assert all(n.endswith(".bias") or "LayerNorm." in n for n in pn), pn
    assert all(n.endswith(".weight") for n in dn)
    if kind == "bert":
        assert all("LayerNorm" not in n for n in dn) and any(n.endswith("attention.output.LayerNorm.weight") for n in pn)
        assert any(n.endswith("embeddings.LayerNorm.weight") for n in pn)
    else:      # DistilBERT's layer norms are sa_layer_norm / output_layer_norm: their weights do not match the rule and are decayed, as in the reference
        assert any(n.endswith("sa_layer_norm.weight") for n in dn) and any(n.endswith("output_layer_norm.weight") for n in dn)
        assert any(n.endswith("sa_layer_norm.bias") for n in pn) and any(n.endswith("embeddings.LayerNorm.weight") for n in pn)


def test_bert_mt_optimizer_is_the_references_dict_and_schedule():
    from transformers import get_linear_schedule_with_warmup
    from ccrec_amd import optim
    model = _names("bert")
    out = optim.bert_mt_optimizer(model.named_parameters(), lr=2e-5, weight_decay=0.01, max_epochs=25, _host_state_only=True)
    assert set(out) == {"optimizer", "lr_scheduler"} and set(out["lr_scheduler"]) == {"scheduler", "monitor"} and out["lr_scheduler"]["monitor"] == "loss"
    opt, sched = out["optimizer"], out["lr_scheduler"]["scheduler"]
    assert isinstance(opt, optim.FusedAdamW) and len(opt.param_groups) == 2
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0]
    ref = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=2e-5)
    ref_sched = get_linear_schedule_with_warmup(ref, num_warmup_steps=int(25 * 0.1), num_training_steps=25)
    assert opt.param_groups[0]["lr"] == 0.0      # the schedule starts at zero
    for _ in range(27):
        assert opt.param_groups[0]["lr"] == opt.param_groups[1]["lr"] == ref.param_groups[0]["lr"]
        opt._opt_called = ref._opt_called = True      # (no step() on host tensors: silence the schedulers' order warning)
        sched.step()
        ref_sched.step()


def test_param_group_keys_are_torch_adamws():
    from ccrec_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    mine = optim.FusedAdamW([p], lr=1e-3, _host_state_only=True)
    theirs = torch.optim.AdamW([p], lr=1e-3)
    assert set(mine.param_groups[0]) == set(theirs.param_groups[0])
    for key in ("lr", "betas", "eps", "weight_decay"):
        assert mine.param_groups[0][key] == theirs.param_groups[0][key]
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(mine, factor=0.5, patience=0)
    sched.step(1.0)
    sched.step(2.0)
    assert mine.param_groups[0]["lr"] == 5e-4


def test_constructor_refusals_name_what_and_why():
    from ccrec_amd import optim
    p = torch.nn.Parameter(torch.zeros(4, 4))
    for kwargs, word in (({"amsgrad": True}, "amsgrad"), ({"maximize": True}, "maximize"), ({"capturable": True}, "capturable"),
                         ({"differentiable": True}, "differentiable"), ({"foreach": True}, "foreach"), ({"fused": True}, "fused")):
        with pytest.raises(ValueError, match=word):
            optim.FusedAdamW([p], _host_state_only=True, **kwargs)
    with pytest.raises(ValueError, match="CUDA parameters only"):
        optim.FusedAdamW([p])
    with pytest.raises(ValueError, match="float16"):
        optim.FusedAdamW([torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))], _host_state_only=True)
    with pytest.raises(ValueError, match="not contiguous"):
        optim.FusedAdamW([torch.nn.Parameter(torch.zeros(4, 4).t()[:, :2])], _host_state_only=True)
    sparse = torch.nn.Parameter(torch.zeros(4, 4))
    sparse.grad = torch.zeros(4, 4).to_sparse()
    with pytest.raises(ValueError, match="sparse gradient"):
        optim.FusedAdamW([sparse], _host_state_only=True)
    with pytest.raises(ValueError, match="more than one device"):
        optim.FusedAdamW([p, torch.nn.Parameter(torch.zeros(2, device="meta"))], _host_state_only=True)
    with pytest.raises(ValueError, match="shadow_dtype"):
        optim.FusedAdamW([p], shadow_for=torch.nn.Linear(2, 2), shadow_dtype=torch.float32, _host_state_only=True)
    with pytest.raises(ValueError):      # torch's own argument checks still apply
        optim.FusedAdamW([p], lr=-1.0, _host_state_only=True)
    with pytest.raises(ValueError, match="state-dict work only"):
        optim.FusedAdamW([p], _host_state_only=True).step()


def test_state_dict_moves_to_torch_adamw_and_back():
    """CPU tensors, no step(): the state a torch AdamW built is loaded, handed on and handed back unchanged; flags the kernel does not cover
    are refused on the way in."""
    from ccrec_amd import optim
    g = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter(torch.randn(7, 3, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g)), torch.nn.Parameter(torch.randn(2, generator=g))]
    groups = lambda: [{"params": params[:2], "weight_decay": 0.01}, {"params": params[2:], "weight_decay": 0.0}]      # noqa: E731
    theirs = torch.optim.AdamW(groups(), lr=3e-4, betas=(0.8, 0.95), eps=1e-6)
    for _ in range(3):
        for p in params[:2]:      # the third never gets a gradient: it has no state
            p.grad = torch.randn(p.shape, generator=g)
        theirs.step()
    sd = theirs.state_dict()
    mine = optim.FusedAdamW(groups(), _host_state_only=True)
    mine.load_state_dict(sd)
    assert set(mine.state) == set(params[:2])
    for p in params[:2]:
        st, ref = mine.state[p], theirs.state[p]
        assert st["step"].dtype == torch.float32 and not st["step"].is_cuda and float(st["step"]) == 3.0
        assert torch.equal(st["exp_avg"], ref["exp_avg"]) and torch.equal(st["exp_avg_sq"], ref["exp_avg_sq"])
    assert mine.param_groups[0]["lr"] == 3e-4 and mine.param_groups[0]["betas"] == (0.8, 0.95) and mine.param_groups[1]["weight_decay"] == 0.0
    back = torch.optim.AdamW(groups(), lr=1.0)
    back.load_state_dict(mine.state_dict())
    for p in params[:2]:
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back.state[p][key], theirs.state[p][key])
    before = [p.detach().clone() for p in params]
    for p in params[:2]:
        p.grad = torch.ones_like(p)
    back.step()      # torch accepts every key it needs from FusedAdamW's groups
    assert float(back.state[params[0]]["step"]) == 4.0 and not torch.equal(params[0], before[0])
    bad = torch.optim.AdamW(groups(), lr=3e-4, amsgrad=True).state_dict()
    with pytest.raises(ValueError, match="amsgrad"):
        optim.FusedAdamW(groups(), _host_state_only=True).load_state_dict(bad)


def test_library_version_and_argument_checks_without_a_device():
    """ccr_adamw_step checks its whole list before the first launch: these calls return before any device call."""
    from ccrec_amd import _lib
    assert _lib.OPTIM_VERSION == 107 and _lib.MIN_VERSION == 101 and "ccr_adamw_step" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.ccr_version() >= 107
    assert ctypes.sizeof(_lib.AdamwSegment) == 64
    assert lib.ccr_adamw_step(None, 0, 0.1, 0.999, 0.001, 1e-8, None) == _lib.CCR_OK
    assert lib.ccr_adamw_step(None, -1, 0.1, 0.999, 0.001, 1e-8, None) == _lib.CCR_ERR_INVALID
    assert lib.ccr_adamw_step(None, 2, 0.1, 0.999, 0.001, 1e-8, None) == _lib.CCR_ERR_INVALID
    segs = (_lib.AdamwSegment * 2)()
    segs[1].n = -5
    assert lib.ccr_adamw_step(segs, 2, 0.1, 0.999, 0.001, 1e-8, None) == _lib.CCR_ERR_INVALID
    assert b"segment 1" in lib.ccr_last_error() and b"n < 0" in lib.ccr_last_error()
    segs[1].n = 8      # non-empty, NULL pointers
    assert lib.ccr_adamw_step(segs, 2, 0.1, 0.999, 0.001, 1e-8, None) == _lib.CCR_ERR_INVALID
    assert b"NULL" in lib.ccr_last_error()
    segs[1].n, segs[1].shadow_dtype = 0, 7
    assert lib.ccr_adamw_step(segs, 2, 0.1, 0.999, 0.001, 1e-8, None) == _lib.CCR_ERR_INVALID
    segs[1].shadow_dtype = 0      # two empty segments: nothing to launch
    assert lib.ccr_adamw_step(ctypes.byref(segs, ctypes.sizeof(_lib.AdamwSegment)), 1, 0.1, 0.999, 0.001, 1e-8, None) == _lib.CCR_OK


def test_batching_invariants_on_cpu(tmp_path):
    """tests/native/optim_plan_check.cpp over csrc/ccr_optim_plan.h: lists of 0, 1 and 1000 segments, n from 1 to 24 M, every alignment --
    every element covered exactly once, no chunk across a segment edge, the 16-byte path only on aligned pointers, argument bytes <= 4096,
    BERT-base's 199 tensors in at most 16 launches."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not (os.path.isabs(cxx) and os.path.exists(cxx)):
        pytest.skip("no C++ compiler")
    exe = tmp_path / "optim_plan_check"
    cmd = [cxx, "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "native", "optim_plan_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:]
    lines = run.stdout.strip().splitlines()
    assert lines[-1].endswith(", 0 violations") and int(lines[-1].split()[0]) > 1000, lines[-1]
    bert = [ln for ln in lines if ln.startswith("BERT-base:")][0]
    assert "199 tensors" in bert and int(bert.split(" launches")[0].split()[-1]) <= 16, bert
