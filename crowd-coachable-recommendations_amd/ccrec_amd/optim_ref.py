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
