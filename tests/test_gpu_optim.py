"""ccr_adamw_step (csrc/ccr_optim.hip) and optim.FusedAdamW on the GPU.  Every case compares p, exp_avg, exp_avg_sq and the 16-bit shadow
BIT FOR BIT with the numpy restatement (ccrec_amd/optim_ref.py); NaNs compare by position.  Every array of a case lies in an arena with at
least 64 canary elements behind (and in front of) it, and the canaries must survive.

The library is called through its C ABI (a host array of ccr_adamw_segment) for the kernel cases and through FusedAdamW for the optimizer's
own behaviour (schedules, state, versions, no host wait, one call per step)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG  # noqa: F401

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.999), 1e-8
CANARY_F32, CANARY_U16 = np.float32(-7.25e7), np.uint16(0x5A5A)
GUARD = 64
EPS_F32 = 2.0 ** -23


class _Arena:
    """One device buffer holding many arrays: each starts `skew` elements past a 256-byte boundary and has >= 64 canaries on both sides."""

    def __init__(self, dtype, canary):
        self.dtype, self.canary, self.spans, self.size = dtype, canary, [], GUARD

    def place(self, data, skew):
        at = self.size + skew
        self.spans.append((at, np.ascontiguousarray(data, dtype=self.dtype)))
        self.size = (at + len(data) + GUARD + 127) // 128 * 128
        return len(self.spans) - 1

    def upload(self):
        host = np.full(self.size, self.canary, dtype=self.dtype)
        self.free = np.ones(self.size, dtype=bool)
        for at, data in self.spans:
            host[at:at + len(data)] = data
            self.free[at:at + len(data)] = False
        as_torch = torch.from_numpy(host.view(np.int16) if self.dtype == np.uint16 else host)
        self.dev = as_torch.cuda()
        assert self.dev.data_ptr() % 256 == 0
        return self

    def ptr(self, i):
        return self.dev.data_ptr() + self.spans[i][0] * self.dev.element_size()

    def download(self):
        self.after = self.dev.cpu().numpy().view(self.dtype)
        bad = np.flatnonzero(self.after[self.free] != self.canary)
        assert bad.size == 0, f"{bad.size} canary elements overwritten (first at free slot {bad[0]})"

    def get(self, i):
        at, data = self.spans[i]
        return self.after[at:at + len(data)]


def _same_bits(got, want, what):
    """Equal bit patterns; where the expectation is NaN, a NaN."""
    kind = np.uint32 if want.dtype == np.float32 else np.uint16
    if want.dtype == np.float32:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
        got, want = np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want)
    bad = np.flatnonzero(got.view(kind) != want.view(kind))
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} elements differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}"


def _same_shadow(got_u16, p_ref, code, what):
    from ccrec_amd import optim_ref
    want = optim_ref.shadow_bits(p_ref, code)
    nan = np.isnan(p_ref)
    exp_mask = 0x7F80 if code == 1 else 0x7C00
    assert ((got_u16[nan] & 0x7FFF) > exp_mask).all(), f"{what}: a NaN parameter's shadow is not a NaN"
    _same_bits(np.where(nan, np.uint16(0), got_u16), np.where(nan, np.uint16(0), want), what)


def _case(n, seed, skews=(0, 0, 0, 0), shadow=0, shadow_skew=0, t=1, lr=2e-5, wd=0.01, gscale=1e-2, special=False):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.05).astype(np.float32)
    g = (rng.standard_normal(n) * gscale).astype(np.float32)
    m = (rng.standard_normal(n) * gscale * 0.1).astype(np.float32) if t > 1 else np.zeros(n, np.float32)
    v = ((rng.standard_normal(n) * gscale) ** 2 * 0.01).astype(np.float32) if t > 1 else np.zeros(n, np.float32)
    if special:      # gradients of exactly 0 (with and without history), 1e-12, 1e4, both infinities, a NaN
        vals = [0.0, 0.0, 1e-12, -1e-12, 1e4, -1e4, np.inf, -np.inf, np.nan]
        at = rng.choice(n, size=len(vals), replace=False)
        g[at] = np.array(vals, np.float32)
        m[at[1]] = v[at[1]] = 0.0
    return dict(p=p, g=g, m=m, v=v, skews=skews, shadow=shadow, shadow_skew=shadow_skew, t=t, lr=lr, wd=wd)


def _run(cases):
    """One ccr_adamw_step call over the cases; every output against the restatement, every canary checked."""
    from ccrec_amd import _lib, ops, optim_ref
    lib = ops._require_optim()
    arenas = {k: _Arena(np.float32, CANARY_F32) for k in "pgmv"}
    shadows = _Arena(np.uint16, CANARY_U16)
    for c in cases:
        c["slot"] = {k: arenas[k].place(c[k], s) for k, s in zip("pgmv", c["skews"])}
        c["sslot"] = shadows.place(np.full(len(c["p"]), 0x1111, np.uint16), c["shadow_skew"]) if c["shadow"] else None
    for a in arenas.values():
        a.upload()
    shadows.upload()
    segs = (_lib.AdamwSegment * len(cases))()
    for s, c in zip(segs, cases):
        s.param, s.grad, s.exp_avg, s.exp_avg_sq = (arenas[k].ptr(c["slot"][k]) for k in "pgmv")
        s.n = len(c["p"])
        s.decay, s.step_size, s.bc2_sqrt = (float(x) for x in optim_ref.segment_scalars(c["t"], c["lr"], c["wd"], BETAS))
        s.shadow, s.shadow_dtype = (shadows.ptr(c["sslot"]), c["shadow"]) if c["shadow"] else (None, 0)
    w1, b2, w2, eps = (float(x) for x in optim_ref.global_scalars(BETAS, EPS))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.ccr_adamw_step(segs, len(cases), w1, b2, w2, eps, stream), "ccr_adamw_step")
    torch.cuda.synchronize()
    for a in arenas.values():
        a.download()
    shadows.download()
    for i, c in enumerate(cases):
        p, m, v = optim_ref.adamw_step(c["p"], c["g"], c["m"], c["v"], c["t"], c["lr"], c["wd"], BETAS, EPS)
        what = f"segment {i} (n={len(p)}, skews {c['skews']}, shadow {c['shadow']})"
        _same_bits(arenas["p"].get(c["slot"]["p"]), p, what + " p")
        _same_bits(arenas["m"].get(c["slot"]["m"]), m, what + " exp_avg")
        _same_bits(arenas["v"].get(c["slot"]["v"]), v, what + " exp_avg_sq")
        _same_bits(arenas["g"].get(c["slot"]["g"]), c["g"], what + " grad (read only)")
        if c["shadow"]:
            _same_shadow(shadows.get(c["sslot"]), p, c["shadow"], what + " shadow")
        c["out"] = (p, m, v)
    return cases


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 1023, 4095, 4096, 4097, 8191, 8193])
def test_single_segments_at_every_vector_and_chunk_edge(n):
    """One segment per call, without a shadow and with either type: n around the 4-element vector, the 256-thread sweep and the
    4096-element chunk (one chunk - 1, one chunk, one chunk + 1, two chunks +- 1)."""
    for shadow in (0, 1, 2):
        _run([_case(n, seed=n + shadow, shadow=shadow, t=2)])


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_views_off_the_16_byte_boundary(skew):
    """All four arrays `skew` floats past a 16-byte boundary; only one of them; only the shadow off its 8-byte boundary: the 4-byte path,
    the same bits.  (n = 4100: more than one chunk, n % 4 == 0.)"""
    cases = [_case(4100, seed=skew, skews=(skew,) * 4, shadow=1, shadow_skew=skew, t=3)]
    for which in range(4):
        cases.append(_case(4100, seed=10 * skew + which, skews=tuple(skew if j == which else 0 for j in range(4)), shadow=2, t=3))
    cases.append(_case(4100, seed=50 + skew, shadow=1, shadow_skew=skew, t=3))
    cases.append(_case(4101, seed=60 + skew, shadow=2, shadow_skew=0, t=3))      # aligned, with a tail
    _run(cases)
    for c in cases:
        _run([c])


def test_three_hundred_segments_cross_every_launch_batch():
    """n = 1 .. 300 in one call: seven launches of up to 48 segments, every position of the prefix search; shadows and alignments mixed."""
    _run([_case(n, seed=1000 + n, skews=((n // 3) % 4, 0, 0, (n // 7) % 2), shadow=n % 3, shadow_skew=(n // 5) % 4, t=1 + n % 3) for n in range(1, 301)])


def test_more_chunks_than_the_capped_grid():
    """10.4 M elements in four segments = 2546 chunks on a grid capped at 2048 workgroups: the stride loop; one segment on odd addresses."""
    cases = [_case(4 * 1024 * 1024 + 1, seed=1, shadow=1, t=5), _case(4 * 1024 * 1024 + 3, seed=2, skews=(1, 1, 1, 1), shadow=2, shadow_skew=1, t=5),
             _case(2 * 1024 * 1024 + 2, seed=3, t=5), _case(17, seed=4, shadow=1, t=5)]
    assert sum((len(c["p"]) + 4095) // 4096 for c in cases) > 2048
    _run(cases)


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("lr", [0.0, 2e-5])
def test_step_counts_decay_lr_zero_and_special_gradients(lr, wd, t):
    """t in {1, 2, 1000}; wd 0 / 0.01; lr = 0 (p keeps its bits, exp_avg and exp_avg_sq move); gradients of exactly 0, +-1e-12, +-1e4,
    +-inf and NaN among ordinary ones, on both access paths."""
    cases = _run([_case(4097, seed=t + int(wd * 1000), shadow=1, t=t, lr=lr, wd=wd, special=True),
                  _case(1027, seed=t + 7, skews=(1, 0, 2, 0), shadow=2, shadow_skew=1, t=t, lr=lr, wd=wd, special=True)])
    for c in cases:
        p, m, v = c["out"]
        finite = np.isfinite(c["g"])
        assert not np.array_equal(m[finite], c["m"][finite]) and not np.array_equal(v[finite], c["v"][finite])
        if lr == 0.0:      # the restatement itself leaves p alone wherever the update is finite
            assert np.array_equal(p[finite].view(np.uint32), c["p"][finite].view(np.uint32))
        assert np.isnan(p[~finite]).all()


def test_mixed_shadows_and_row_blocks_of_one_buffer():
    """No shadow, bf16 and fp16 in one call, and three segments writing the row blocks of one [3 h, h] buffer per type: the buffer then
    holds torch.cat([q, k, v]).to(dtype), bit for bit."""
    from ccrec_amd import _lib, ops, optim_ref
    lib = ops._require_optim()
    h = 64
    g = torch.Generator().manual_seed(3)
    tensors = {}
    for dtype, code in ((torch.bfloat16, 1), (torch.float16, 2)):
        for name in "qkv":
            tensors[(code, name)] = [(torch.randn(h, h, generator=g) * s).cuda() for s in (0.05, 1e-2, 0.0, 0.0)]      # p, g, m, v
    plain = [(torch.randn(777, generator=g) * s).cuda() for s in (0.05, 1e-2, 0.0, 0.0)]
    stacked = {1: torch.full((3 * h + 1, h), 9.0, dtype=torch.bfloat16, device="cuda"), 2: torch.full((3 * h + 1, h), 9.0, dtype=torch.float16, device="cuda")}
    before = {key: [x.cpu().numpy().copy() for x in val] for key, val in tensors.items()}
    plain_before = [x.cpu().numpy().copy() for x in plain]
    segs = (_lib.AdamwSegment * 7)()
    order = [(code, name) for code in (1, 2) for name in "qkv"]
    scal = [float(x) for x in optim_ref.segment_scalars(1, 1e-3, 0.01, BETAS)]
    for s, key in zip(segs, order):
        p, gr, m, v = tensors[key]
        s.param, s.grad, s.exp_avg, s.exp_avg_sq, s.n = p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
        s.decay, s.step_size, s.bc2_sqrt = scal
        s.shadow, s.shadow_dtype = stacked[key[0]]["qkv".index(key[1]) * h:].data_ptr(), key[0]
    s = segs[6]
    s.param, s.grad, s.exp_avg, s.exp_avg_sq, s.n = plain[0].data_ptr(), plain[1].data_ptr(), plain[2].data_ptr(), plain[3].data_ptr(), 777
    s.decay, s.step_size, s.bc2_sqrt = scal
    s.shadow, s.shadow_dtype = None, 0
    w1, b2, w2, eps = (float(x) for x in optim_ref.global_scalars(BETAS, EPS))
    _lib.check(lib.ccr_adamw_step(segs, 7, w1, b2, w2, eps, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ccr_adamw_step")
    torch.cuda.synchronize()
    _same_bits(plain[0].cpu().numpy(), optim_ref.adamw_step(*plain_before, 1, 1e-3, 0.01, BETAS, EPS)[0], "the segment without a shadow")
    for code, dtype in ((1, torch.bfloat16), (2, torch.float16)):
        for name in "qkv":
            p0, g0, m0, v0 = before[(code, name)]
            want = optim_ref.adamw_step(p0, g0, m0, v0, 1, 1e-3, 0.01, BETAS, EPS)[0]
            _same_bits(tensors[(code, name)][0].cpu().numpy(), want, f"{name} of type {code}")
        cat = torch.cat([tensors[(code, n)][0] for n in "qkv"]).to(dtype)
        assert torch.equal(stacked[code][:3 * h].view(torch.int16), cat.view(torch.int16))
        assert (stacked[code][3 * h:] == 9.0).all()      # the row behind the three blocks is nobody's


# ------------------------------------------------------------------------------------------------------------------------ FusedAdamW
def _params(seed=0, shapes=((33, 7), (4097,), (1,), (64, 64))):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).cuda()) for s in shapes]


def _set_grads(params, step, gscale=1e-2, skip=()):
    g = torch.Generator().manual_seed(100 + step)
    for i, p in enumerate(params):
        grad = (torch.randn(*p.shape, generator=g) * gscale).cuda()
        p.grad = None if i in skip else grad


def test_forty_steps_under_the_linear_warmup_schedule():
    """FusedAdamW under transformers' get_linear_schedule_with_warmup (lr starts at 0), two groups (wd 0.01 / 0): bit for bit the restatement
    at every step, and within four fp32 spacings (of max |p|, max |g|, max g^2) of torch.optim.AdamW on the same GPU."""
    from transformers import get_linear_schedule_with_warmup
    from ccrec_amd import optim, optim_ref
    mine, theirs = _params(), _params()
    groups = lambda ps: [{"params": ps[:2], "weight_decay": 0.01}, {"params": ps[2:], "weight_decay": 0.0}]      # noqa: E731
    opt = optim.FusedAdamW(groups(mine), lr=2e-5)
    ref_opt = torch.optim.AdamW(groups(theirs), lr=2e-5, foreach=False)
    sched = get_linear_schedule_with_warmup(opt, num_warmup_steps=4, num_training_steps=40)
    ref_sched = get_linear_schedule_with_warmup(ref_opt, num_warmup_steps=4, num_training_steps=40)
    state = [(p.detach().cpu().numpy().copy(), np.zeros(p.numel(), np.float32).reshape(p.shape), np.zeros(p.numel(), np.float32).reshape(p.shape))
             for p in mine]
    gmax = [0.0] * len(mine)
    worst = [0.0, 0.0, 0.0]
    for t in range(1, 41):
        lr = opt.param_groups[0]["lr"]
        assert (t == 1) == (lr == 0.0) and lr == ref_opt.param_groups[0]["lr"]
        _set_grads(mine, t, gscale=10.0 ** -(t % 4))
        for p, q in zip(mine, theirs):
            q.grad = p.grad.clone()
        opt.step()
        ref_opt.step()
        sched.step()
        ref_sched.step()
        for i, p in enumerate(mine):
            wd = 0.01 if i < 2 else 0.0
            gr = p.grad.cpu().numpy()
            state[i] = optim_ref.adamw_step(state[i][0], gr, state[i][1], state[i][2], t, lr, wd, BETAS, EPS)
            st = opt.state[p]
            assert float(st["step"]) == t and not st["step"].is_cuda
            got = (p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())
            for k, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
                _same_bits(got[k], state[i][k], f"step {t} parameter {i} {name}")
            gmax[i] = max(gmax[i], float(np.abs(gr).max()))
            rst = ref_opt.state[theirs[i]]
            ref = (theirs[i].detach().cpu().numpy(), rst["exp_avg"].cpu().numpy(), rst["exp_avg_sq"].cpu().numpy())
            bars = (4 * EPS_F32 * float(np.abs(got[0]).max()), 4 * EPS_F32 * gmax[i], 4 * EPS_F32 * gmax[i] ** 2)
            for k in range(3):
                err = float(np.abs(got[k] - ref[k]).max())
                worst[k] = max(worst[k], err / bars[k])
                assert err <= bars[k], (t, i, k, err, bars[k])
    print(f"FusedAdamW vs torch AdamW (GPU), 40 steps: worst error / bar p {worst[0]:.3f} exp_avg {worst[1]:.3f} exp_avg_sq {worst[2]:.3f}")


def test_step_is_one_library_call_without_a_host_wait_and_bumps_versions(monkeypatch):
    """A parameter without a gradient is untouched: its bits, its step count, its _version.  Updated parameters' _version rises.  step()
    runs under torch.cuda.set_sync_debug_mode("error") -- the first step, which creates the state, included.  One ccr_adamw_step per step."""
    from ccrec_amd import _lib, optim
    params = _params(seed=2)
    opt = optim.FusedAdamW(params, lr=1e-3)
    lib = _lib.load()
    calls, real = [], lib.ccr_adamw_step
    monkeypatch.setattr(lib, "ccr_adamw_step", lambda *a: (calls.append(a[1]), real(*a))[1])
    frozen = params[2].detach().clone()
    for step in range(1, 4):
        _set_grads(params, step, skip=(2,))
        strided = torch.zeros(7, 33, device="cuda").t()      # a non-contiguous gradient is made contiguous for the call
        strided.copy_(params[0].grad)
        params[0].grad = strided
        assert not params[0].grad.is_contiguous()
        versions = [p._version for p in params]
        before = [p.detach().clone() for p in params]
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert calls == [3] * step      # one call per step, three segments
        for i, p in enumerate(params):
            if i == 2:
                assert p._version == versions[i] and torch.equal(p.detach(), frozen) and p not in opt.state
            else:
                assert p._version > versions[i] and not torch.equal(p.detach(), before[i])
                assert float(opt.state[p]["step"]) == step
    # the parameter joins later: its own step count starts at 1 (bias correction per tensor)
    _set_grads(params, 9)
    opt.step()
    assert float(opt.state[params[2]]["step"]) == 1.0 and float(opt.state[params[0]]["step"]) == 4.0 and calls[-1] == 4
    params[0].grad = params[0].grad.to_sparse()
    with pytest.raises(ValueError, match="sparse gradient"):
        opt.step()


def test_state_dict_round_trip_through_torch_adamw_continues_with_the_same_bits():
    from ccrec_amd import optim
    straight, hopped = _params(seed=4), _params(seed=4)
    opt_a = optim.FusedAdamW(straight, lr=1e-3, weight_decay=0.01)
    opt_b = optim.FusedAdamW(hopped, lr=1e-3, weight_decay=0.01)
    for step in range(1, 3):
        for ps, opt in ((straight, opt_a), (hopped, opt_b)):
            _set_grads(ps, step)
            opt.step()
    via = torch.optim.AdamW(hopped, lr=5.0)
    via.load_state_dict(opt_b.state_dict())
    assert via.param_groups[0]["lr"] == 1e-3 and float(via.state[hopped[0]]["step"]) == 2.0
    opt_c = optim.FusedAdamW(hopped, lr=7.0)
    opt_c.load_state_dict(via.state_dict())
    for step in range(3, 5):
        for ps, opt in ((straight, opt_a), (hopped, opt_c)):
            _set_grads(ps, step)
            opt.step()
    for p, q in zip(straight, hopped):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[p][key].view(torch.int32), opt_c.state[q][key].view(torch.int32))
        assert float(opt_c.state[q]["step"]) == 4.0
    # and torch's optimizer steps on from FusedAdamW's state
    _set_grads(hopped, 5)
    via.load_state_dict(opt_c.state_dict())
    via.step()
    assert float(via.state[hopped[0]]["step"]) == 5.0
