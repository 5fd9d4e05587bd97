"""Loss scaling, overflow skip and norm clipping inside the fused AdamW step on the GPU: ccr_grad_stats, ccr_adamw_control_update and
ccr_adamw_step_scaled (csrc/ccr_optim.hip) through their C ABI, and FusedAdamW(max_grad_norm=...), optim.LossScaler and a stock
torch.amp.GradScaler (torch's _step_supports_amp_scaling protocol) on top of them.  Everything is compared BIT FOR BIT with the numpy
restatement (ccrec_amd/optim_ref.py); NaNs compare by position.  Arrays of the C ABI cases lie in arenas with 64 canary elements around
each, and the canaries must survive."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG  # noqa: F401

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.999), 1e-8
CANARY_F32, CANARY_U16 = np.float32(-7.25e7), np.uint16(0x5A5A)
GUARD = 64
EDGE_SIZES = (1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8193)
LONG = 2049 * 4096 + 5      # more chunks (2050) than the capped grid (2048)


class _Arena:
    """One device buffer holding many arrays: each starts `skew` elements past a 256-byte boundary and has >= 64 canaries on both sides."""

    def __init__(self, dtype, canary):
        self.dtype, self.canary, self.spans, self.size = dtype, canary, [], GUARD

    def place(self, data, skew=0):
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
        self.before = host
        self.dev = torch.from_numpy(host.view(np.int16) if self.dtype == np.uint16 else host).cuda()
        assert self.dev.data_ptr() % 256 == 0
        return self

    def ptr(self, i):
        return self.dev.data_ptr() + self.spans[i][0] * self.dev.element_size()

    def download(self):
        self.after = self.dev.cpu().numpy().view(self.dtype)
        bad = np.flatnonzero(self.after[self.free] != self.canary)
        assert bad.size == 0, f"{bad.size} canary elements overwritten (first at free slot {bad[0]})"
        return self

    def get(self, i):
        at, data = self.spans[i]
        return self.after[at:at + len(data)]


def _same_bits(got, want, what):
    """Equal bit patterns; where the expectation is NaN, a NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    kind = np.uint32 if want.dtype == np.float32 else np.uint16
    if want.dtype == np.float32:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
        got, want = np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want)
    bad = np.flatnonzero(got.reshape(-1).view(kind) != want.reshape(-1).view(kind))
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} elements differ, first at {bad[0]}: got {got.reshape(-1)[bad[0]]!r}, "
                           f"want {want.reshape(-1)[bad[0]]!r}")


def _lib_and_stream():
    from ccrec_amd import _lib, ops
    lib = ops._require_optim_amp()
    return _lib, lib, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _grads(sizes, seed, gscale=1e-2):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * gscale).astype(np.float32) for n in sizes]


def _control_tensor(scale=0.0, tracker=0, coef=0.0, skip=0):
    host = torch.zeros(16, dtype=torch.float32)
    host[0], host[3] = coef, scale
    host.view(torch.int32)[1], host.view(torch.int32)[4] = skip, tracker
    return host.cuda()


def _read_control(control):
    host = control.cpu()
    ints = host.view(torch.int32)
    assert not host[6:].any(), "the reserved words stay zero"
    return dict(coef=host[0].numpy(), skip=int(ints[1]), norm=host[2].numpy(), scale=host[3].numpy(), tracker=int(ints[4]), skipped=int(ints[5]))


def _stats_and_control(gs, g_skews=None, p_skews=None, modes=()):
    """ccr_grad_stats over the gradients (their segments' other three pointers are one more, never-read array of the same size), the
    partials against the restatement, then ccr_adamw_control_update in each mode against control_update.  -> the reference partials.
    modes: (own scale or None, tracker, max_norm, growth, backoff, interval, ext_found_inf, ext_scale)"""
    from ccrec_amd import optim_ref
    _lib, lib, stream = _lib_and_stream()
    g_arena, other = _Arena(np.float32, CANARY_F32), _Arena(np.float32, CANARY_F32)
    g_skews = g_skews or [0] * len(gs)
    p_skews = p_skews or [0] * len(gs)
    for g, gs_, ps_ in zip(gs, g_skews, p_skews):
        g_arena.place(g, gs_)
        other.place(np.zeros(len(g), np.float32), ps_)
    g_arena.upload(), other.upload()
    segs = (_lib.AdamwSegment * len(gs))()
    for i, s in enumerate(segs):
        s.grad = g_arena.ptr(i)
        s.param = s.exp_avg = s.exp_avg_sq = other.ptr(i)
        s.n, s.decay, s.step_size, s.bc2_sqrt = len(gs[i]), 1.0, 0.0, 1.0
    want = optim_ref.grad_sumsq_partials(gs)
    need = lib.ccr_grad_stats_workspace_bytes(segs, len(gs))
    assert need == 4 * len(want)
    parts = _Arena(np.float32, CANARY_F32)
    parts.place(np.full(len(want), 7.0, np.float32))
    parts.upload()
    _lib.check(lib.ccr_grad_stats(segs, len(gs), ctypes.c_void_p(parts.ptr(0)), stream), "ccr_grad_stats")
    controls = []
    for scale, tracker, max_norm, growth, backoff, interval, found, ext_scale in modes:
        control = _control_tensor(scale or 0.0, tracker)
        ext = [None if x is None else torch.tensor(float(x), dtype=torch.float32, device="cuda") for x in (ext_scale, found)]
        _lib.check(lib.ccr_adamw_control_update(ctypes.c_void_p(control.data_ptr()), ctypes.c_void_p(parts.ptr(0)), len(want), max_norm or 0.0,
                                                1 if scale else 0, growth, backoff, interval, *[None if t is None else ctypes.c_void_p(t.data_ptr()) for t in ext],
                                                stream), "ccr_adamw_control_update")
        controls.append((control, ext))
    torch.cuda.synchronize()
    _same_bits(parts.download().get(0), want, "partials")
    _same_bits(g_arena.download().get(0), gs[0], "the gradients are read only")
    other.download()
    for (control, _), (scale, tracker, max_norm, growth, backoff, interval, found, ext_scale) in zip(controls, modes):
        ref = optim_ref.control_update(want, scale, tracker, max_norm, growth, backoff, interval, ext_found_inf=found, ext_scale=ext_scale)
        got = _read_control(control)
        what = f"control block, mode {(scale, tracker, max_norm, interval, found, ext_scale)}"
        assert got["skip"] == ref["skip"] and got["skipped"] == ref["skip"], (what, got, ref)
        _same_bits(got["norm"], ref["norm"], what + " norm")
        if not ref["skip"]:
            _same_bits(got["coef"], ref["coef"], what + " coef")
        if scale:
            _same_bits(got["scale"], ref["scale"], what + " scale")
            assert got["tracker"] == ref["tracker"], (what, got, ref)
        else:
            assert got["scale"] == 0.0 and got["tracker"] == tracker      # not its own scale: left alone
    return want


MODES = ((65536.0, 0, 1.0, 2.0, 0.5, 2000, None, None),      # own scale, clipping
         (65536.0, 2, 1e-3, 2.0, 0.5, 3, None, None),        # ... growing at the interval, the clip at work
         (3e38, 0, None, 2.0, 0.5, 1, None, None),           # ... a growth that would overflow is refused
         (None, 0, None, 2.0, 0.5, 1, None, None),           # nothing: coef 1
         (None, 5, 0.5, 2.0, 0.5, 1, 0.0, 1024.0),           # a GradScaler's scale and found_inf = 0
         (None, 5, 0.5, 2.0, 0.5, 1, 1.0, 1024.0),           # ... found_inf = 1: skip
         (None, 0, 2.0, 2.0, 0.5, 1, 0.0, None))             # found_inf alone (the gradients were unscaled already)


def test_partials_and_control_at_every_vector_and_chunk_edge():
    want = _stats_and_control(_grads(EDGE_SIZES, 1), modes=MODES)
    assert len(want) == 9 + 2 + 3


@pytest.mark.parametrize("skew", [1, 2, 3])
def test_partials_of_views_off_the_16_byte_boundary(skew):
    """The gradient `skew` floats off; only the parameter off (the segment's flag, hence the 4-byte path on an aligned gradient): the same
    partials as the aligned arrays give."""
    gs = _grads(EDGE_SIZES, 2)
    aligned = _stats_and_control(gs)
    for g_skews, p_skews in (([skew] * len(gs), None), (None, [skew] * len(gs)), ([(skew + i) % 4 for i in range(len(gs))], None)):
        _same_bits(_stats_and_control(gs, g_skews, p_skews, modes=MODES[:1]), aligned, f"skews {g_skews} / {p_skews}")


def test_partial_index_continues_across_three_launch_batches():
    sizes = [1 + (i * 977) % 9000 for i in range(100)]
    want = _stats_and_control(_grads(sizes, 3), g_skews=[i % 4 for i in range(100)], modes=MODES[:2])
    assert len(want) == sum((n + 4095) // 4096 for n in sizes) > 100


def test_one_segment_with_more_chunks_than_the_capped_grid():
    want = _stats_and_control(_grads([LONG, 5], 4), modes=MODES[:1] + MODES[3:4])
    assert len(want) == 2050 + 1


# ---------------------------------------------------------------------------------------------------------------- the scaled step
def _case(n, seed, skews=(0, 0, 0, 0), shadow=0, shadow_skew=0, t=2, lr=1e-3, wd=0.01, gscale=1e-2):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.05).astype(np.float32)
    g = (rng.standard_normal(n) * gscale).astype(np.float32)
    m = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    v = ((rng.standard_normal(n) * 1e-2) ** 2 * 0.01).astype(np.float32)
    return dict(p=p, g=g, m=m, v=v, skews=skews, shadow=shadow, shadow_skew=shadow_skew, t=t, lr=lr, wd=wd)


def _mixed_cases(seed):
    cases = [_case(n, seed + n, shadow=i % 3) for i, n in enumerate(EDGE_SIZES)]
    cases += [_case(4100, seed + 50 + k, skews=(k, k, k, k), shadow=1 + k % 2, shadow_skew=k) for k in (1, 2, 3)]
    cases += [_case(4101, seed + 60, skews=(0, 1, 0, 0), shadow=2), _case(777, seed + 61, shadow=1, shadow_skew=1)]
    cases += [_case(1 + (i * 131) % 600, seed + 100 + i, shadow=i % 3) for i in range(90)]      # 106 segments: three launches
    return cases


def _place(cases):
    from ccrec_amd import optim_ref
    _lib, lib, stream = _lib_and_stream()
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
    return arenas, shadows, segs


def _download(arenas, shadows):
    torch.cuda.synchronize()
    for a in arenas.values():
        a.download()
    shadows.download()


def _scalars():
    from ccrec_amd import optim_ref
    return tuple(float(x) for x in optim_ref.global_scalars(BETAS, EPS))


def test_scaled_step_with_coef_one_stores_the_plain_steps_bits():
    """p, exp_avg, exp_avg_sq and both shadow types, every access path, three launches."""
    _lib, lib, stream = _lib_and_stream()
    plain, scaled = _mixed_cases(7), _mixed_cases(7)
    a_plain, s_plain, segs_plain = _place(plain)
    a_scaled, s_scaled, segs_scaled = _place(scaled)
    control = _control_tensor(coef=1.0, skip=0)
    _lib.check(lib.ccr_adamw_step(segs_plain, len(plain), *_scalars(), stream), "ccr_adamw_step")
    _lib.check(lib.ccr_adamw_step_scaled(segs_scaled, len(scaled), *_scalars(), ctypes.c_void_p(control.data_ptr()), stream), "ccr_adamw_step_scaled")
    _download(a_plain, s_plain), _download(a_scaled, s_scaled)
    for k in "pgmv":
        assert np.array_equal(a_plain[k].after.view(np.uint32), a_scaled[k].after.view(np.uint32)), k
        if k != "g":
            assert not np.array_equal(a_plain[k].after.view(np.uint32), a_plain[k].before.view(np.uint32))
    assert np.array_equal(s_plain.after, s_scaled.after) and not np.array_equal(s_plain.after, s_plain.before)


def test_skipped_step_stores_nothing():
    """skip = 1 (and a NaN multiplier, which any store would show): p, exp_avg, exp_avg_sq and the shadows keep every byte."""
    _lib, lib, stream = _lib_and_stream()
    cases = _mixed_cases(8)
    arenas, shadows, segs = _place(cases)
    control = _control_tensor(coef=float("nan"), skip=1)
    _lib.check(lib.ccr_adamw_step_scaled(segs, len(cases), *_scalars(), ctypes.c_void_p(control.data_ptr()), stream), "ccr_adamw_step_scaled")
    _download(arenas, shadows)
    for k in "pgmv":
        assert np.array_equal(arenas[k].after.view(np.uint32), arenas[k].before.view(np.uint32)), k
    assert np.array_equal(shadows.after, shadows.before)


@pytest.mark.parametrize("side", ["below", "above"])
def test_clipping_just_below_and_just_above_max_norm(side):
    """Scale 65536, the gradients pre-multiplied by it; max_norm 0.1 % above / below the unscaled norm.  stats -> control -> scaled step,
    every stored value against the restatement."""
    from ccrec_amd import optim_ref
    _lib, lib, stream = _lib_and_stream()
    scale = 65536.0
    cases = _mixed_cases(9)
    for c in cases:
        c["g"] = c["g"] * np.float32(scale)
    partials = optim_ref.grad_sumsq_partials([c["g"] for c in cases])
    norm = float(np.sqrt(optim_ref.partials_sum(partials))) / scale
    max_norm = float(np.float32(norm * (1.001 if side == "below" else 0.999)))
    ref = optim_ref.control_update(partials, scale, 0, max_norm, 2.0, 0.5, 2000)
    assert ref["skip"] == 0 and (ref["coef"] == np.float32(1.0 / scale) if side == "below" else ref["coef"] < np.float32(1.0 / scale))
    arenas, shadows, segs = _place(cases)
    control = _control_tensor(scale=scale)
    ws = torch.empty(len(partials), dtype=torch.float32, device="cuda")
    assert lib.ccr_grad_stats_workspace_bytes(segs, len(cases)) == 4 * len(partials)
    _lib.check(lib.ccr_grad_stats(segs, len(cases), ctypes.c_void_p(ws.data_ptr()), stream), "ccr_grad_stats")
    _lib.check(lib.ccr_adamw_control_update(ctypes.c_void_p(control.data_ptr()), ctypes.c_void_p(ws.data_ptr()), len(partials), max_norm, 1, 2.0, 0.5, 2000,
                                            None, None, stream), "ccr_adamw_control_update")
    _lib.check(lib.ccr_adamw_step_scaled(segs, len(cases), *_scalars(), ctypes.c_void_p(control.data_ptr()), stream), "ccr_adamw_step_scaled")
    _download(arenas, shadows)
    got = _read_control(control)
    _same_bits(ws.cpu().numpy(), partials, "partials")
    _same_bits(got["coef"], ref["coef"], "coef")
    _same_bits(got["norm"], ref["norm"], "norm")
    assert got["skip"] == 0 and got["scale"] == scale and got["tracker"] == 1
    for i, c in enumerate(cases):
        p, m, v = optim_ref.adamw_step_scaled(c["p"], c["g"], c["m"], c["v"], c["t"], c["lr"], c["wd"], BETAS, EPS, ref["coef"], 0)
        what = f"segment {i} (n={len(p)})"
        _same_bits(arenas["p"].get(c["slot"]["p"]), p, what + " p")
        _same_bits(arenas["m"].get(c["slot"]["m"]), m, what + " exp_avg")
        _same_bits(arenas["v"].get(c["slot"]["v"]), v, what + " exp_avg_sq")
        if c["shadow"]:
            _same_bits(shadows.get(c["sslot"]), optim_ref.shadow_bits(p, c["shadow"]), what + " shadow")


# --------------------------------------------------------------------------------------------------- FusedAdamW, LossScaler, GradScaler
LR, WD, MAX_NORM = 1e-3, 0.01, 0.05


def _odd_view(n, skew, fill=0.0):
    """A contiguous fp32 CUDA tensor of n elements `skew` floats past a 16-byte boundary."""
    base = torch.full((n + 8,), fill, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 16 == 0
    return base[skew:skew + n]


def _make_params(sizes, seed, odd=()):
    gen = torch.Generator().manual_seed(seed)
    params = []
    for i, n in enumerate(sizes):
        value = torch.randn(n, generator=gen) * 0.05
        if i in odd:
            store = _odd_view(n, 1 + i % 3)
            store.copy_(value)
            params.append(torch.nn.Parameter(store))
        else:
            params.append(torch.nn.Parameter(value.cuda()))
    return params


def _host_grads(sizes, step, seed=0):
    rng = np.random.default_rng(1000 * seed + step)
    return [(rng.standard_normal(n) * 1e-2).astype(np.float32) for n in sizes]


def _give(params, grads, odd=()):
    for i, (p, g) in enumerate(zip(params, grads)):
        if i in odd:
            p.grad = _odd_view(len(g), 1 + i % 3)
            p.grad.copy_(torch.from_numpy(g))
        else:
            p.grad = torch.from_numpy(g).cuda()


class _Sim:
    """The restatement of a run: per-tensor (p, m, v), the step count, the scale and its tracker."""

    def __init__(self, params, scale, growth=2.0, backoff=0.5, interval=2000):
        self.state = [(p.detach().cpu().numpy().copy(), np.zeros(p.numel(), np.float32), np.zeros(p.numel(), np.float32)) for p in params]
        self.t, self.scale, self.tracker, self.rule = 0, np.float32(scale), 0, (growth, backoff, interval)

    def step(self, scaled_grads):
        from ccrec_amd import optim_ref
        ctl = optim_ref.control_update(optim_ref.grad_sumsq_partials(scaled_grads), self.scale, self.tracker, MAX_NORM, *self.rule)
        self.scale, self.tracker = ctl["scale"], ctl["tracker"]
        if not ctl["skip"]:
            self.t += 1
        self.state = [optim_ref.adamw_step_scaled(p, g, m, v, max(self.t, 1), LR, WD, BETAS, EPS, ctl["coef"], ctl["skip"])
                      for (p, m, v), g in zip(self.state, scaled_grads)]
        return ctl

    def check(self, params, opt, what):
        for i, (p, (rp, rm, rv)) in enumerate(zip(params, self.state)):
            _same_bits(p.detach().cpu().numpy(), rp, f"{what}: parameter {i}")
            if p in opt.state:
                _same_bits(opt.state[p]["exp_avg"].cpu().numpy(), rm, f"{what}: exp_avg {i}")
                _same_bits(opt.state[p]["exp_avg_sq"].cpu().numpy(), rv, f"{what}: exp_avg_sq {i}")


SKIP_SIZES = {"first": ([4097, 33], (), (0, 0)), "tail_last": ([33, 4099], (), (1, 4098)), "non_vec4": ([600, 4100, 7], (1,), (1, 2222)),
              "third_batch_last": ([1 + (i * 131) % 600 for i in range(100)], (), (99, (99 * 131) % 600))}


SKIP_CASES = [(where, bad) for where in SKIP_SIZES for bad in (np.inf, -np.inf, np.nan)] + [("first", 3e19)]      # 3e19 alone, once


@pytest.mark.parametrize("where,bad", SKIP_CASES, ids=[f"{w}:{b}" for w, b in SKIP_CASES])
def test_an_overflow_anywhere_skips_the_step_halves_the_scale_and_takes_the_count_back(where, bad):
    """A good step, a step with one bad gradient element (the first element; the last element of a scalar tail; inside a segment on odd
    addresses; the last segment of the third launch batch -- +inf, -inf, NaN, and a finite 3e19 whose square passes fp32), a good step:
    skip = 1, nothing moves, the scale is halved, the counts go back after settle(), and the next step has the restatement's bits at the
    count the skipped step would have had."""
    from ccrec_amd import optim
    sizes, odd, (ti, ei) = SKIP_SIZES[where]
    params = _make_params(sizes, 5, odd)
    opt = optim.FusedAdamW(params, lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    scaler = optim.LossScaler(init_scale=65536.0)
    sim = _Sim(params, 65536.0)
    for step in (1, 2, 3):
        grads = [g * sim.scale for g in _host_grads(sizes, step)]
        if step == 2:
            if bad == 3e19:
                grads = [np.zeros_like(g) for g in grads]      # alone: every other gradient is zero
            grads[ti][ei] = bad
        before = [p.detach().clone() for p in params]
        moments = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params] if step > 1 else None
        _give(params, grads, odd)
        ctl = sim.step(grads)
        scaler.step(opt)
        scaler.update()
        block = _read_control(scaler._control)
        assert block["skip"] == ctl["skip"] == (1 if step == 2 else 0)
        _same_bits(block["scale"], ctl["scale"], f"step {step} scale")
        if step == 2:
            assert block["scale"] == 32768.0 and block["tracker"] == 0 and block["skipped"] == 1
            for p, old, (m, v) in zip(params, before, moments):
                assert torch.equal(p.detach().view(torch.int32), old.view(torch.int32))
                assert torch.equal(opt.state[p]["exp_avg"].view(torch.int32), m.view(torch.int32))
                assert torch.equal(opt.state[p]["exp_avg_sq"].view(torch.int32), v.view(torch.int32))
            assert all(float(opt.state[p]["step"]) == 2.0 for p in params)      # not settled yet: one ahead
            opt.settle()
            assert all(float(opt.state[p]["step"]) == 1.0 for p in params)
            opt.settle()      # idempotent
            assert all(float(opt.state[p]["step"]) == 1.0 for p in params)
        else:
            _same_bits(opt.last_grad_norm.cpu().numpy(), ctl["norm"], f"step {step} norm")
        sim.check(params, opt, f"{where} step {step}")
    opt.settle()
    assert sim.t == 2 and all(float(opt.state[p]["step"]) == 2.0 for p in params)
    assert scaler.get_scale() == 32768.0 and scaler.get_skipped_steps() == 1 and scaler.state_dict()["_growth_tracker"] == 1


def test_twelve_steps_with_two_overflows_under_loss_scaler_and_under_torchs_grad_scaler(monkeypatch):
    """Overflows at steps 4 and 9, growth every 3 unskipped steps: LossScaler and a stock torch.amp.GradScaler (through the protocol) give
    the restatement's bits and each other's, and neither step() calls Tensor.item or Tensor.cpu."""
    from ccrec_amd import optim
    sizes = [33 * 7, 4097, 1, 64 * 64, 8193]
    rule = dict(growth=2.0, backoff=0.5, interval=3)
    runs = {}
    for driver in ("loss_scaler", "grad_scaler"):
        params = _make_params(sizes, 6)
        opt = optim.FusedAdamW([{"params": params[:2], "weight_decay": WD}, {"params": params[2:], "weight_decay": WD}], lr=LR, max_grad_norm=MAX_NORM)
        sim = _Sim(params, 1024.0, **rule)
        if driver == "loss_scaler":
            scaler = optim.LossScaler(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
        else:
            scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
            scaler.scale(torch.zeros((), device="cuda"))      # (creates its device scalars)
        skips = []
        for step in range(1, 13):
            grads = [g * sim.scale for g in _host_grads(sizes, step, seed=2)]
            if step in (4, 9):
                grads[step % 5][-1] = np.inf if step == 4 else np.nan
            _give(params, grads)
            ctl = sim.step(grads)
            skips.append(ctl["skip"])
            with monkeypatch.context() as guard:
                def refuse(*a, **k):
                    raise AssertionError("a host read of a device tensor inside step()")
                guard.setattr(torch.Tensor, "item", refuse)
                guard.setattr(torch.Tensor, "cpu", refuse)
                scaler.step(opt)
            scaler.update()
            sim.check(params, opt, f"{driver} step {step}")
            _same_bits(opt.last_grad_norm.cpu().numpy(), ctl["norm"], f"{driver} step {step} norm")
            assert scaler.get_scale() == float(sim.scale), (driver, step, scaler.get_scale(), sim.scale)
        opt.settle()
        assert skips == [0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0] and sim.t == 10
        assert all(float(opt.state[p]["step"]) == 10.0 for p in params)
        assert sim.scale == 1024.0 * 2 / 2 * 2 / 2 * 2      # grown after 3, halved at 4, grown after 7, halved at 9, grown after 12
        runs[driver] = [p.detach().clone() for p in params] + [opt.state[p][k].clone() for p in params for k in ("exp_avg", "exp_avg_sq")]
        if driver == "loss_scaler":
            assert scaler.state_dict() == {"scale": float(sim.scale), "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 3, "_growth_tracker": 0}
        assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")
    for a, b in zip(runs["loss_scaler"], runs["grad_scaler"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_max_grad_norm_alone_clips_like_the_restatement_and_a_plain_optimizer_stays_one_call(monkeypatch):
    """max_grad_norm without any scaler: coef = the clip factor, last_grad_norm = the norm; the same parameters under a plain FusedAdamW make
    one ccr_adamw_step call per step and never touch the new entry points, the event or the pinned word."""
    from ccrec_amd import _lib, optim, optim_ref
    sizes = [4097, 33, 5]
    params, plain = _make_params(sizes, 8), _make_params(sizes, 8)
    opt = optim.FusedAdamW(params, lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    plain_opt = optim.FusedAdamW(plain, lr=LR, weight_decay=WD)
    lib = _lib.load()
    calls = []
    for name in ("ccr_adamw_step", "ccr_grad_stats", "ccr_adamw_control_update", "ccr_adamw_step_scaled"):
        monkeypatch.setattr(lib, name, (lambda real, name: lambda *a: (calls.append(name), real(*a))[1])(getattr(lib, name), name))
    state = [(p.detach().cpu().numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)) for p, n in zip(params, sizes)]
    for t in (1, 2):
        grads = _host_grads(sizes, t, seed=3)
        _give(params, grads)
        _give(plain, grads)
        ctl = optim_ref.control_update(optim_ref.grad_sumsq_partials(grads), None, 0, MAX_NORM, 2.0, 0.5, 1)
        assert ctl["skip"] == 0 and ctl["coef"] < 1.0
        del calls[:]
        opt.step()
        assert calls == ["ccr_grad_stats", "ccr_adamw_control_update", "ccr_adamw_step_scaled"]
        del calls[:]
        plain_opt.step()
        assert calls == ["ccr_adamw_step"] and plain_opt._pending is None and plain_opt._skip_host is None and plain_opt._control is None
        _same_bits(opt.last_grad_norm.cpu().numpy(), ctl["norm"], "last_grad_norm")
        assert opt.last_grad_norm.is_cuda and opt.last_grad_norm.dim() == 0
        state = [optim_ref.adamw_step_scaled(p, g, m, v, t, LR, WD, BETAS, EPS, ctl["coef"], 0) for (p, m, v), g in zip(state, grads)]
        for p, (rp, _, _) in zip(params, state):
            _same_bits(p.detach().cpu().numpy(), rp, f"step {t}")


def test_maintained_16_bit_weights_stay_current_and_equal_the_rounded_masters_after_a_skipped_step():
    """shadow_for = a two-layer BERT, fp16: a good step, then a step with an infinite gradient.  The skipped step leaves the masters and the
    encoder's maintained set alone; the set is still reported current and holds exactly what a rebuild from the masters would."""
    from transformers import BertConfig, BertModel
    from ccrec_amd import fused_bert, optim
    torch.manual_seed(0)
    model = BertModel(BertConfig(vocab_size=600, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                                 max_position_embeddings=128)).cuda()
    dtype = torch.float16
    opt = optim.FusedAdamW(model.parameters(), lr=LR, weight_decay=WD, shadow_for=model, shadow_dtype=dtype, max_grad_norm=1.0)
    scaler = optim.LossScaler(init_scale=65536.0)
    enc = fused_bert.for_model(model)
    assert enc is not None and enc.adopted_current(dtype)
    gen = torch.Generator().manual_seed(1)
    named = list(model.named_parameters())
    for step in (1, 2):
        for name, p in named:
            p.grad = (torch.randn(p.shape, generator=gen) * 1e-2 * 65536.0).cuda()
        if step == 2:
            next(p for n, p in named if n.endswith("layer.1.intermediate.dense.weight")).grad[3, 5] = float("inf")
        before = [p.detach().clone() for _, p in named]
        kept = {(i, name): getattr(layer, name).clone() for i, layer in enumerate(enc._layers[dtype]) for name in fused_bert._LAYER_16BIT}
        scaler.step(opt)
        opt.settle()
        assert _read_control(scaler._control)["skip"] == step - 1
        assert enc.adopted_current(dtype) and enc.refresh(dtype) is False
        moved = [not torch.equal(p.detach(), old) for (_, p), old in zip(named, before)]
        assert all(moved) if step == 1 else not any(moved)
        fresh = enc._build_layers(dtype)
        for i, (mine, want) in enumerate(zip(enc._layers[dtype], fresh)):
            for name in fused_bert._LAYER_16BIT:
                assert torch.equal(getattr(mine, name).view(torch.int16), getattr(want, name).view(torch.int16)), (step, i, name)
                assert torch.equal(getattr(mine, name).view(torch.int16), kept[(i, name)].view(torch.int16)) == (step == 2), (step, i, name)
    assert all(float(opt.state[p]["step"]) == 1.0 for _, p in named)
