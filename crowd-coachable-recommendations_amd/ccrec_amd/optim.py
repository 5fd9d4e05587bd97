"""FusedAdamW: torch.optim.AdamW's update as ONE multi-tensor kernel call per step (ccr_adamw_step, csrc/ccr_optim.hip) that can also keep
the 16-bit weight set of every FusedBertEncoder under a module current, so neither the training forwards nor the next ranking step's
inference forward cast a weight again.

The reference fine-tunes with torch.optim.AdamW under transformers' linear warm-up schedule (src/ccrec/models/bert_mt.py:115-146);
bert_mt_optimizer builds the same two parameter groups and the same schedule around FusedAdamW.

    opt = FusedAdamW(tower.parameters(), lr=2e-5, weight_decay=0.01)                                  # drop-in: same groups, same state dict
    opt = FusedAdamW(tower.parameters(), lr=2e-5, shadow_for=tower, shadow_dtype=torch.bfloat16)    # ... and the encoder's 16-bit weights

Arithmetic: optim_ref (fp32 throughout, per-tensor scalars formed in double from the tensor's own step count); within a few fp32 spacings
of torch.optim.AdamW per stored value (tests/test_cpu_optim.py).  Not covered, refused by name: amsgrad, maximize, capturable, differentiable,
parameters that are not contiguous fp32 CUDA tensors of one device, sparse gradients.

Loss scaling and clipping (fp16 training; opt-in, DESIGN 4.8o "Loss scaling, overflow skip and norm clipping"): max_grad_norm=, a stock
torch.amp.GradScaler (through torch's own _step_supports_amp_scaling protocol) or this module's LossScaler make step() three library calls
-- ccr_grad_stats reads every gradient once, ccr_adamw_control_update turns the sums into {multiplier, skip, norm, scale} in device
memory, ccr_adamw_step_scaled applies them -- with no host read of the device anywhere.  Without any of the three, step() is the one
call it was.  clip_grad_norm_ and GradScaler.unscale_ on p.grad before step() still work as with any optimizer.

    opt = FusedAdamW(params, lr=2e-5, max_grad_norm=1.0);  scaler = LossScaler()
    scaler.scale(loss).backward();  scaler.step(opt);  scaler.update()"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, ops

_SHADOW_CODES = {torch.bfloat16: 1, torch.float16: 2}
NO_DECAY = ("bias", "LayerNorm.bias", "LayerNorm.weight")      # the reference's substring rule (bert_mt.py:117)


def _refuse(what, why):
    raise ValueError(f"FusedAdamW: {what}: {why}")


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's constructor, param_groups keys and state (`step` an fp32 scalar CPU tensor, `exp_avg`, `exp_avg_sq`): LambdaLR,
    get_linear_schedule_with_warmup and ReduceLROnPlateau drive it unchanged and state_dict() loads into torch.optim.AdamW and back.

    shadow_for (a module): every encoder under it that the layer kernels cover (fused_bert.for_model) hands over a maintained 16-bit weight
    set in shadow_dtype (FusedBertEncoder.adopt_weights); each step writes the new projection weights and biases into it in the same pass and
    marks it current, and the other type's copies are dropped.

    max_grad_norm (a float): torch.nn.utils.clip_grad_norm_'s rule over the gradients of one step(), inside the step; last_grad_norm is the
    norm as a 0-dim device tensor (None before the first such step).

    Step counts stay on the host, so a step that the device skipped (an overflow under loss scaling) is learned late: settle() -- run by the
    next step(), by state_dict() and on request -- waits for the skipped step's flag and takes the skipped step off the counters of exactly
    the tensors it covered.  A raw read of state[p]["step"] between a step and the next settle may therefore be one ahead."""

    _step_supports_amp_scaling = True      # torch.amp.GradScaler.step then sets grad_scale / found_inf on the optimizer and calls step()

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None, shadow_for=None, shadow_dtype=torch.bfloat16, max_grad_norm=None,
                 _host_state_only=False):
        if amsgrad:
            _refuse("amsgrad=True", "the kernel keeps no running maximum of exp_avg_sq")
        if maximize:
            _refuse("maximize=True", "the kernel descends; negate the objective")
        if capturable:
            _refuse("capturable=True", "the step count lives on the host (hipGraph capture is not covered)")
        if differentiable:
            _refuse("differentiable=True", "the kernel writes through raw pointers, outside autograd")
        if foreach or fused:
            _refuse("foreach=True / fused=True", "this optimizer is its own multi-tensor kernel; leave both unset")
        if isinstance(lr, torch.Tensor):
            _refuse("a tensor lr", "the step's scalars are formed on the host; pass a float")
        # torch's own argument checks and its exact set of param_groups keys (a state dict then moves both ways)
        proto = torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, dict(proto.defaults))
        self._host_state_only = bool(_host_state_only)
        devices = set()
        for gi, group in enumerate(self.param_groups):
            names = group.get("param_names")
            for pi, p in enumerate(group["params"]):
                who = f"parameter {names[pi]!r}" if names else f"parameter {pi} of group {gi} {tuple(p.shape)}"
                if p.dtype != torch.float32:
                    _refuse(who, f"dtype {p.dtype} (fp32 master weights only)")
                if p.is_sparse or p.layout != torch.strided:
                    _refuse(who, "a sparse parameter")
                if not p.is_contiguous():
                    _refuse(who, "not contiguous (the kernel walks flat memory)")
                if p.grad is not None and p.grad.is_sparse:
                    _refuse(who, "a sparse gradient")
                if not p.is_cuda and not self._host_state_only:
                    _refuse(who, f"on {p.device} (CUDA parameters only: there is no CPU fallback)")
                devices.add(p.device)
        if len(devices) > 1:
            _refuse("parameters on more than one device", ", ".join(sorted(str(d) for d in devices)))
        self._segments, self._n_segments = None, 0      # numpy [n, 8] uint64 = ccr_adamw_segment [n], reused by every step
        self._step_base = torch.zeros(256, dtype=torch.float32)      # every parameter's `step`: views into one host vector (_step_slot)
        self._step_np, self._step_used = self._step_base.numpy(), 0
        self._step_slots = {}          # id(parameter) -> (its index in the vector, the view that is its state's `step`)
        self._shadow = {}              # id(parameter) -> (the tensor it lives in, its address, the type's code)
        self._shadow_tensors = []      # the 16-bit tensors written behind autograd's back: their versions are bumped with the parameters'
        self._encoders = []
        self.shadow_dtype = None
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            _refuse(f"max_grad_norm={max_grad_norm!r}", "a positive number, or None for no clipping")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self._control = None           # this optimizer's own ccr_adamw_control (a LossScaler brings its own), as 16 fp32 words on the device
        self._partials = None          # ccr_grad_stats' workspace
        self._skip_host = None         # a pinned int32 word: the last scaled step's skip flag lands here
        self._pending = None           # (event recorded behind that copy, the step slots the step covered)
        if shadow_for is not None:
            self._attach_shadows(shadow_for, shadow_dtype)

    # ------------------------------------------------------------------------------------------------------------------ shadows
    def _attach_shadows(self, module, dtype):
        from . import fused_bert
        if dtype not in _SHADOW_CODES:
            _refuse(f"shadow_dtype {dtype}", "torch.bfloat16 or torch.float16")
        if self._host_state_only:
            _refuse("shadow_for", "needs CUDA parameters")
        code, mine = _SHADOW_CODES[dtype], {id(p) for g in self.param_groups for p in g["params"]}
        refused = []      # why the encoders under the module that fused_bert knows by class were turned down
        for m in module.modules():
            reason = fused_bert.shadow_unsupported_reason(m)
            if reason is not None:      # (not covered, or covered for inference only)
                if not isinstance(fused_bert._describe(m), str):
                    refused.append(f"{type(m).__name__}: {reason}")
                continue
            enc = fused_bert.for_model(m)
            layers = enc.adopt_weights(dtype)
            arch = fused_bert._describe(m)

            def put(p, tensor, first_row=0):
                if p is None or id(p) not in mine:
                    return      # not this optimizer's: nobody moves it between two signatures, and a change from outside is seen by the encoder
                row = tensor[first_row:first_row + p.shape[0]]
                assert row.is_contiguous() and row.numel() == p.numel() and tensor.device == p.device, (tuple(p.shape), tuple(tensor.shape))
                self._shadow[id(p)] = (tensor, row.data_ptr(), code)

            for mod, l in zip(arch.stack.layer, layers):
                q, k, v, so, _, ff, out, _ = arch.layer_parts(mod)
                hidden = q.weight.shape[0]
                for j, lin in enumerate((q, k, v)):
                    put(lin.weight, l.wqkv, j * hidden)
                    put(lin.bias, l.bqkv, j * hidden)
                for lin, w, b in ((so, l.wo, l.bo), (ff, l.wi, l.bi), (out, l.wo2, l.bo2)):
                    put(lin.weight, w)
                    put(lin.bias, b)
                self._shadow_tensors += [l.wqkv, l.bqkv, l.wo, l.bo, l.wi, l.bi, l.wo2, l.bo2]
            self._encoders.append((enc, enc.adopted_masters()))
        if not self._encoders:
            _refuse("shadow_for", "no encoder under the module is one the layer kernels cover (fused_bert.unsupported_reason) and can train "
                    "(fused_bert.shadow_unsupported_reason)" + "".join(f"; {r}" for r in refused))
        self.shadow_dtype = dtype

    # --------------------------------------------------------------------------------------------------------------------- state
    def settle(self):
        """Wait for the last scaled step's skip flag; if the device skipped that step, its tensors' step counts go back by one.  (Nothing
        to do, and no wait, after a plain step.)"""
        pending, self._pending = self._pending, None
        if pending is None:
            return
        event, slots = pending
        event.synchronize()
        if int(self._skip_host.numpy()[0]) != 0:
            self._step_np[slots] -= 1.0

    _settle = settle

    def state_dict(self):
        self.settle()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        self.settle()
        super().load_state_dict(state_dict)
        for group in self.param_groups:      # (a torch.optim.AdamW state dict carries its own flags)
            self._check_group(group)
        for state in self.state.values():    # a fused / capturable torch optimizer keeps `step` on the device: one read here, none per step
            step = state.get("step")
            if isinstance(step, torch.Tensor) and (step.is_cuda or step.dtype != torch.float32):
                state["step"] = step.detach().to(device="cpu", dtype=torch.float32)
            elif step is not None and not isinstance(step, torch.Tensor):
                state["step"] = torch.tensor(float(step), dtype=torch.float32)

    @staticmethod
    def _check_group(group):
        for flag, why in (("amsgrad", "the kernel keeps no running maximum"), ("maximize", "the kernel descends"),
                          ("capturable", "the step count lives on the host"), ("differentiable", "the kernel writes outside autograd")):
            if group.get(flag):
                _refuse(f"{flag}=True in a parameter group", why)
        if group.get("decoupled_weight_decay") is False:
            _refuse("decoupled_weight_decay=False in a parameter group", "this is AdamW: the decay multiplies the parameter")

    # ---------------------------------------------------------------------------------------------------------------------- step
    def _step_slot(self, p, state):
        """`step` of every parameter is a 0-dim view into ONE host fp32 vector, so a step advances and reads all counters with two numpy
        calls instead of two tensor operations per parameter.  A `step` that is not that view (a fresh state, load_state_dict, a user's
        own tensor) is copied into its slot first."""
        slot = self._step_slots.get(id(p))
        if slot is None:
            if self._step_used == self._step_base.numel():      # grow: the states' old views fail the identity test below and move over
                self._step_base = torch.cat([self._step_base, torch.zeros_like(self._step_base)])
                self._step_np = self._step_base.numpy()
                self._step_slots = {key: (i, self._step_base[i]) for key, (i, _) in self._step_slots.items()}
            slot = self._step_slots[id(p)] = (self._step_used, self._step_base[self._step_used])
            self._step_used += 1
        i, view = slot
        have = state.get("step")
        if have is not view:
            self._step_np[i] = 0.0 if have is None else float(have)
            state["step"] = view
        return i

    def _control_block(self, device):
        if self._control is None:
            self._control = torch.zeros(16, dtype=torch.float32, device=device)
        return self._control

    def _scaled_calls(self, lib, device, n, slots, calls, base, stream, own):
        """The step under a control block: statistics over all n segments, the control kernel, the skip flag on its way to the host, then
        the scaled step.  own: a LossScaler's (block, growth, backoff, interval), else None -- then torch's GradScaler may have left
        grad_scale / found_inf on this optimizer (grad_scale None: the gradients are unscaled already)."""
        f32 = torch.float32
        ext_scale, ext_inf = (None, None) if own else (getattr(self, "grad_scale", None), getattr(self, "found_inf", None))
        for name, t in (("grad_scale", ext_scale), ("found_inf", ext_inf)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype is f32 and t.device == device and t.numel() == 1):
                _refuse(name, f"an fp32 tensor of one element on {device} (torch.amp.GradScaler's), not {t!r}")
        control = own[0] if own else self._control_block(device)
        segments = ctypes.c_void_p(base)
        need = int(lib.ccr_grad_stats_workspace_bytes(segments, n))
        if need < 0:
            _lib.check(_lib.CCR_ERR_INVALID, "ccr_grad_stats_workspace_bytes")
        if self._partials is None or self._partials.numel() * 4 < need or self._partials.device != device:
            self._partials = torch.empty(max(need // 4, 1024), dtype=f32, device=device)
        if self._skip_host is None:
            self._skip_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        growth, backoff, interval = own[1:] if own else (1.0, 1.0, 1)
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
        _lib.check(lib.ccr_grad_stats(segments, n, ptr(self._partials), stream), "ccr_grad_stats")
        _lib.check(lib.ccr_adamw_control_update(ptr(control), ptr(self._partials), need // 4, self.max_grad_norm or 0.0, 1 if own else 0,
                                                growth, backoff, interval, ptr(ext_scale), ptr(ext_inf), stream), "ccr_adamw_control_update")
        # the skip flag leaves before the step kernel is queued: the host learns of a skip as early as the device knows
        self._skip_host.copy_(control.view(torch.int32)[_lib.CONTROL_WORDS["skip"]:_lib.CONTROL_WORDS["skip"] + 1], non_blocking=True)
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(device))
        self._pending = (event, slots)
        for (b1, b2, eps), (first, count) in calls.items():
            if count:
                _lib.check(lib.ccr_adamw_step_scaled(ctypes.c_void_p(base + 64 * first), count, 1.0 - b1, b2, 1.0 - b2, eps, ptr(control), stream),
                           "ccr_adamw_step_scaled")
        self.last_grad_norm = control[_lib.CONTROL_WORDS["norm"]]

    @torch.no_grad()
    def step(self, closure=None, *, _loss_scaler=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._host_state_only:
            _refuse("step()", "built over host tensors for state-dict work only")
        self.settle()
        scaled = _loss_scaler is not None or self.max_grad_norm is not None or hasattr(self, "grad_scale") or hasattr(self, "found_inf")
        lib = ops._require_optim_amp() if scaled else ops._require_optim()
        f32, strided = torch.float32, torch.strided
        words, slots, decays, hyper, codes = [], [], [], [], []      # per segment: six 64-bit words, step slot, decay, (lr, b1, b2), shadow type
        calls = {}          # (beta1, beta2, eps) -> [first segment, count]: one library call each (one, unless the groups disagree)
        updated, keep_alive, device = [], [], None
        shadow_of = self._shadow
        for group in sorted(self.param_groups, key=lambda g: (float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]))):      # (stable)
            self._check_group(group)
            lr, wd, eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
            b1, b2 = float(group["betas"][0]), float(group["betas"][1])
            decay, hyp = 1.0 - lr * wd, (lr, b1, b2)
            run = calls.setdefault((b1, b2, eps), [len(updated), 0])
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.layout is not strided:
                    _refuse(f"parameter {tuple(p.shape)}", "a sparse gradient")
                if g.dtype is not f32 or g.device != p.device:
                    _refuse(f"parameter {tuple(p.shape)}", f"gradient of {g.dtype} on {g.device}")
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep_alive.append(g)
                state = self.state[p]
                if len(state) == 0:
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                if not (m.is_contiguous() and v.is_contiguous()):
                    m, v = state["exp_avg"], state["exp_avg_sq"] = m.contiguous(), v.contiguous()
                slots.append(self._step_slot(p, state))
                shadow = shadow_of.get(id(p))
                words += (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), shadow[1] if shadow else 0, p.numel())
                codes.append(shadow[2] if shadow else 0)
                decays.append(decay)
                hyper.append(hyp)
                updated.append(p)
                run[1] += 1
        n = len(updated)
        if n == 0:
            return loss
        device = updated[0].device
        # the counters advance, the per-tensor scalars follow from each tensor's own count (in double; rounded to fp32 once, on assignment)
        self._step_np[slots] += 1.0
        ts = self._step_np[slots].tolist()
        scalars = {}
        step_sizes, bc2 = [], []
        for t, (lr, b1, b2) in zip(ts, hyper):
            sc = scalars.get((t, lr, b1, b2))
            if sc is None:
                sc = scalars[(t, lr, b1, b2)] = (lr / (1.0 - b1 ** int(t)), math.sqrt(1.0 - b2 ** int(t)))
            step_sizes.append(sc[0])
            bc2.append(sc[1])
        if self._segments is None or self._segments.shape[0] < n:
            self._segments = np.zeros((max(n, 16), 8), dtype=np.uint64)      # ccr_adamw_segment [n]: eight 64-bit words each
        seg, self._n_segments = self._segments, n
        seg[:n, :6] = np.array(words, dtype=np.uint64).reshape(n, 6)
        floats = seg.view(np.float32)
        floats[:n, 12], floats[:n, 13], floats[:n, 14] = decays, step_sizes, bc2
        seg.view(np.int32)[:n, 15] = codes
        # is every maintained weight set current now?  (taken before the parameters' versions move)
        current = [enc.adopted_current(masters=masters) for enc, masters in self._encoders]
        stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        base = seg.ctypes.data
        with torch.cuda.device(device):
            if scaled:
                self._scaled_calls(lib, device, n, slots, calls, base, stream, _loss_scaler)
            else:
                for (b1, b2, eps), (first, count) in calls.items():
                    if count:
                        _lib.check(lib.ccr_adamw_step(ctypes.c_void_p(base + 64 * first), count, 1.0 - b1, b2, 1.0 - b2, eps, stream), "ccr_adamw_step")
        # the kernel wrote through raw pointers: tell autograd (and FusedBertEncoder, which reads _version).  A step that the device skipped
        # wrote nothing -- the 16-bit weights still equal the rounded masters and stay marked current -- but the host does not know yet, so
        # the version counters move although nothing changed.
        torch.autograd.graph.increment_version(updated + self._shadow_tensors)
        for (enc, masters), was_current in zip(self._encoders, current):
            enc.adopted_stepped(was_current, masters)
        del keep_alive
        return loss


class LossScaler:
    """Dynamic loss scaling for ONE FusedAdamW with torch.amp.GradScaler's call sites, rule and state dict, kept entirely on the device:
    the scale, the growth tracker and the overflow test live in a ccr_adamw_control block, the step reads every gradient once for the
    statistics and once for the update, and nothing is read on the host.

        scaler.scale(loss).backward();  scaler.step(opt);  scaler.update()

    An overflow -- a NaN, an infinity or a gradient whose square passes fp32's range -- skips the step and multiplies the scale by
    backoff_factor; growth_interval unskipped steps in a row multiply it by growth_factor (refused if that would be infinite)."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        if not (growth_factor > 1.0 and 0.0 < backoff_factor < 1.0 and int(growth_interval) >= 1 and init_scale > 0.0):
            raise ValueError(f"LossScaler: init_scale={init_scale}, growth_factor={growth_factor} (> 1), backoff_factor={backoff_factor} "
                             f"(in (0, 1)), growth_interval={growth_interval} (>= 1)")
        self._init_scale, self._init_tracker = float(init_scale), 0
        self._growth_factor, self._backoff_factor, self._growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._control = None      # 16 fp32 words on the device = ccr_adamw_control, made on first use on the loss's / the parameters' device
        self._optimizer = None

    def _block(self, device):
        if self._control is None:
            host = torch.zeros(16, dtype=torch.float32)
            host[_lib.CONTROL_WORDS["scale"]] = self._init_scale
            host.view(torch.int32)[_lib.CONTROL_WORDS["growth_tracker"]] = self._init_tracker
            self._control = host.to(device)
        elif self._control.device != torch.device(device):
            raise ValueError(f"LossScaler: its scale lives on {self._control.device}, asked for on {device}")
        return self._control

    def scale(self, loss):
        """loss * scale, the scale read from the device by the multiply itself."""
        return loss * self._block(loss.device)[_lib.CONTROL_WORDS["scale"]]

    def step(self, optimizer, closure=None):
        """optimizer.step() under this scaler's block: unscale, overflow test, clip (the optimizer's max_grad_norm) and scale update inside
        the optimizer's three library calls.  Returns what optimizer.step() returns."""
        if not isinstance(optimizer, FusedAdamW):
            raise TypeError(f"LossScaler.step: a FusedAdamW, not {type(optimizer).__name__} (use torch.amp.GradScaler for other optimizers)")
        if closure is not None:
            raise ValueError("LossScaler.step: a closure cannot be rerun after the loss was scaled")
        if self._optimizer is None:
            self._optimizer = optimizer
        elif self._optimizer is not optimizer:
            raise ValueError("LossScaler.step: this scaler serves one FusedAdamW (its growth tracker counts that optimizer's steps)")
        device = next(p.device for g in optimizer.param_groups for p in g["params"])
        return optimizer.step(_loss_scaler=(self._block(device), self._growth_factor, self._backoff_factor, self._growth_interval))

    def update(self, new_scale=None):
        """Nothing to do: step() has updated the scale on the device.  (Kept for GradScaler's call sites.)"""
        if new_scale is not None:
            raise ValueError("LossScaler.update: set a scale with load_state_dict")

    def get_scale(self):
        """The current scale as a float.  This READS THE DEVICE ON THE HOST (a wait for the stream), like GradScaler.get_scale()."""
        return self._init_scale if self._control is None else float(self._control[_lib.CONTROL_WORDS["scale"]].item())

    def get_skipped_steps(self):
        """Steps skipped so far; a host read of the device like get_scale()."""
        return 0 if self._control is None else int(self._control.view(torch.int32)[_lib.CONTROL_WORDS["skipped_total"]].item())

    def state_dict(self):
        """torch.amp.GradScaler's keys (one host read of the block): loads into a GradScaler and back."""
        tracker = self._init_tracker
        if self._control is not None:
            tracker = int(self._control.view(torch.int32)[_lib.CONTROL_WORDS["growth_tracker"]].item())
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": tracker}

    def load_state_dict(self, state_dict):
        self._init_scale, self._init_tracker = float(state_dict["scale"]), int(state_dict["_growth_tracker"])
        self._growth_factor, self._backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        if self._control is not None:
            self._control[_lib.CONTROL_WORDS["scale"]] = self._init_scale
            self._control.view(torch.int32)[_lib.CONTROL_WORDS["growth_tracker"]] = self._init_tracker


def bert_mt_groups(named_parameters, weight_decay):
    """The reference's two parameter groups (bert_mt.py:116-131): a name containing "bias", "LayerNorm.bias" or "LayerNorm.weight" is not
    decayed, every other parameter is (DistilBERT's sa_layer_norm.weight among them, as there)."""
    named = list(named_parameters)
    return [{"params": [p for n, p in named if not any(nd in n for nd in NO_DECAY)], "weight_decay": weight_decay},
            {"params": [p for n, p in named if any(nd in n for nd in NO_DECAY)], "weight_decay": 0.0}]


def linear_warmup_lambda(num_warmup_steps, num_training_steps):
    """transformers.get_linear_schedule_with_warmup's factor: 0 -> 1 over the warm-up, then linearly to 0 at num_training_steps."""
    def factor(step):
        if step < num_warmup_steps:
            return float(step) / float(max(1, num_warmup_steps))
        return max(0.0, float(num_training_steps - step) / float(max(1, num_training_steps - num_warmup_steps)))
    return factor


def bert_mt_optimizer(named_parameters, lr, weight_decay, max_epochs, **fused_adamw_args):
    """The reference's configure_optimizers (bert_mt.py:115-146) around FusedAdamW: the same two groups, the linear schedule with
    int(0.1 * max_epochs) warm-up steps over int(max_epochs) -- it starts at lr = 0 -- and the same dict.  fused_adamw_args: shadow_for,
    shadow_dtype, betas, eps."""
    optimizer = FusedAdamW(bert_mt_groups(named_parameters, weight_decay), lr=lr, weight_decay=weight_decay, **fused_adamw_args)
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, linear_warmup_lambda(int(max_epochs * 0.1), int(max_epochs)))
    return {"optimizer": optimizer, "lr_scheduler": {"scheduler": scheduler, "monitor": "loss"}}
