"""The fused AdamW step restated on the CPU (numpy only, no GPU, no library): the bit-exact oracle of csrc/ccr_optim.hip.

Every element-wise operation is one fp32 operation rounded to nearest -- numpy's float32 arithmetic: no contraction, a correctly rounded
divide and square root -- in exactly the kernel's order; the per-tensor scalars are formed in double from the tensor's own 1-based step
count t and rounded once to fp32 (segment_scalars: what FusedAdamW hands the library).

    p1 = p * decay                      decay     = fp32(1 - lr * wd)
    m' = m + w1 * (g - m)               w1        = fp32(1 - beta1)
    v' = v * b2 + (w2 * g) * g          b2, w2    = fp32(beta2), fp32(1 - beta2)
    d  = sqrt(v') / bc2_sqrt + eps      bc2_sqrt  = fp32(sqrt(1 - beta2 ** t))
    p' = p1 - step_size * (m' / d)      step_size = fp32(lr / (1 - beta1 ** t))
    shadow = p' rounded to nearest even in bf16 / fp16

torch.optim.AdamW computes the same update with other roundings (lerp, addcmul, a step size divided in double); the two agree within a
few fp32 spacings of each stored quantity (tests/test_cpu_optim.py)."""
import math

import numpy as np

SHADOW_NONE, SHADOW_BF16, SHADOW_FP16 = 0, 1, 2
_F = np.float32


def global_scalars(betas, eps):
    """-> (1 - beta1, beta2, 1 - beta2, eps) as fp32: the step's tensor-independent scalars."""
    b1, b2 = float(betas[0]), float(betas[1])
    return _F(1.0 - b1), _F(b2), _F(1.0 - b2), _F(float(eps))


def segment_scalars(t, lr, wd, betas):
    """-> (decay, step_size, bc2_sqrt) as fp32 for a tensor at its t-th step (t >= 1), formed in double."""
    t, lr, wd = int(t), float(lr), float(wd)
    assert t >= 1, t
    b1, b2 = float(betas[0]), float(betas[1])
    return _F(1.0 - lr * wd), _F(lr / (1.0 - b1 ** t)), _F(math.sqrt(1.0 - b2 ** t))


def adamw_step(p, g, m, v, t, lr, wd, betas, eps):
    """One step on fp32 arrays of one shape -> (p', m', v'), new arrays; NaN and infinities propagate as IEEE arithmetic has them."""
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    decay, step_size, bc2_sqrt = segment_scalars(t, lr, wd, betas)
    w1, b2, w2, eps = global_scalars(betas, eps)
    with np.errstate(all="ignore"):
        p1 = p * decay
        m1 = m + w1 * (g - m)
        v1 = v * b2 + (w2 * g) * g
        d = np.sqrt(v1) / bc2_sqrt + eps
        p2 = p1 - step_size * (m1 / d)
    assert p2.dtype == m1.dtype == v1.dtype == np.float32
    return p2, m1, v1


def shadow_bits(p, dtype):
    """The 16-bit copy of fp32 p as uint16 bit patterns: dtype "bf16" / SHADOW_BF16 or "fp16" / SHADOW_FP16, round to nearest even.
    (NaN stays NaN; its payload is not specified.)"""
    p = np.ascontiguousarray(p, dtype=np.float32)
    if dtype in ("bf16", "bfloat16", SHADOW_BF16):
        u = p.view(np.uint32).astype(np.uint64)
        r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
        nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
        return np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)
    if dtype in ("fp16", "float16", "half", SHADOW_FP16):
        with np.errstate(all="ignore"):
            return p.astype(np.float16).view(np.uint16)
    raise ValueError(f"shadow_bits: dtype {dtype!r} (bf16 or fp16)")


# ------------------------------------------------------------------- loss scaling, overflow skip, norm clipping (library version 110)
CHUNK, STATS_THREADS, CONTROL_THREADS = 4096, 256, 256


def grad_sumsq_partials(g_list):
    """ccr_grad_stats: one fp32 sum of squares per 4096-element chunk of every non-empty gradient, the chunks counted through the list.
    The order is the kernel's on either access path: the element at offset j of its chunk belongs to thread (j // 4) % 256, which adds its
    squares (each rounded to fp32) in increasing j to a sum that starts at +0; a wave's 64 sums fold as x[i] + x[i + h] for
    h = 32, 16, 8, 4, 2, 1; the four wave sums add as ((w0 + w1) + w2) + w3.  (A chunk's missing elements count as +0, which leaves a sum
    of squares as it is.)"""
    out = []
    with np.errstate(all="ignore"):
        for g in g_list:
            g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
            if g.size == 0:
                continue
            chunks = (g.size + CHUNK - 1) // CHUNK
            padded = np.zeros(chunks * CHUNK, np.float32)
            padded[:g.size] = g
            sq = (padded * padded).reshape(chunks, CHUNK // (4 * STATS_THREADS), STATS_THREADS, 4)      # [chunk, sweep, thread, element]
            acc = np.zeros((chunks, STATS_THREADS), np.float32)
            for k in range(sq.shape[1]):
                for e in range(4):
                    acc = acc + sq[:, k, :, e]
            acc = acc.reshape(chunks, STATS_THREADS // 64, 64)
            for h in (32, 16, 8, 4, 2, 1):
                acc = acc[:, :, :h] + acc[:, :, h:2 * h]
            w = acc[:, :, 0]
            out.append(((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])
            assert out[-1].dtype == np.float32
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def partials_sum(partials):
    """ccr_adamw_control_update's sum of the partials, a double: index order within 256 equal contiguous slices of ceil(n / 256) partials,
    then the slice sums in slice order (for n <= 256 that is plain index order)."""
    partials = np.asarray(partials, dtype=np.float32).reshape(-1)
    n = partials.size
    per = (n + CONTROL_THREADS - 1) // CONTROL_THREADS
    padded = np.zeros(CONTROL_THREADS * per, np.float64)
    padded[:n] = partials
    padded = padded.reshape(CONTROL_THREADS, per)
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        mine = np.zeros(CONTROL_THREADS, np.float64)
        for i in range(per):
            mine = mine + padded[:, i]
        for t in range(CONTROL_THREADS):
            s = s + mine[t]
    return s


def control_update(partials, scale, tracker, max_norm, growth, backoff, interval, ext_found_inf=None, ext_scale=None):
    """ccr_adamw_control_update -> dict(coef, skip, norm, scale, tracker).  scale: the block's own loss scale (updated by torch's
    _amp_update_scale_ rule), or None: no scaling of its own.  ext_scale / ext_found_inf: a stock GradScaler's values; with ext_scale the
    own scale must be None.  max_norm None, <= 0 or infinite: no clipping (the factor is exactly 1)."""
    assert ext_scale is None or scale is None
    s = partials_sum(partials)
    with np.errstate(all="ignore"):
        inv = _F(1.0)
        if ext_scale is not None:
            inv = _F(1.0 / float(_F(ext_scale)))
        elif scale is not None:
            inv = _F(1.0 / float(_F(scale)))
        skip = bool(not np.isfinite(s)) or (ext_found_inf is not None and float(ext_found_inf) != 0.0)
        norm = _F(np.sqrt(s)) * inv
        clip = _F(1.0)
        max_norm = _F(0.0 if max_norm is None else max_norm)
        if max_norm > 0 and not np.isinf(max_norm):
            ratio = max_norm / (norm + _F(1e-6))
            clip = ratio if ratio < 1 else _F(1.0)
        coef = inv * clip
        new_scale, tracker = (None if scale is None else _F(scale)), int(tracker)
        if scale is not None:
            if skip:
                new_scale, tracker = _F(float(new_scale) * float(backoff)), 0      # (in double, rounded once: torch's kernel)
            else:
                tracker += 1
                if tracker == int(interval):
                    grown = _F(float(new_scale) * float(growth))
                    if np.isfinite(grown):
                        new_scale = grown
                    tracker = 0
    assert coef.dtype == norm.dtype == np.float32
    return dict(coef=coef, skip=int(skip), norm=norm, scale=new_scale, tracker=tracker)


def adamw_step_scaled(p, g, m, v, t, lr, wd, betas, eps, coef, skip):
    """ccr_adamw_step_scaled on one tensor: nothing changes on a skip, else adamw_step on g * coef (one fp32 multiply) -> (p', m', v')."""
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    if skip:
        return p.copy(), m.copy(), v.copy()
    with np.errstate(all="ignore"):
        scaled = g * _F(coef)
    return adamw_step(p, scaled, m, v, t, lr, wd, betas, eps)
