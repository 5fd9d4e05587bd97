"""The part probe of tests/test_gpu_loss_kernels.py can fail: on the CPU, for every probe shape, the probe's logits are exact in fp32,
fp32 arithmetic with THREE bf16 parts of the logit gradient stays under the GPU test's bound (a third of the two-part error E2) and the
same arithmetic with TWO parts -- a third part dropped, or a part read twice -- does not."""
import numpy as np
import pytest

from helpers import INBATCH_PROBE_SHAPES, POOL_PROBE_SHAPES, bf16_parts, bf16_round, loss_probe_case, loss_probe_errors

CASES = ([("inbatch", side, B, 2 * B, dim) for B, dim in INBATCH_PROBE_SHAPES for side in ("dq", "dc")]
         + [("pool", side, n_q, n_c, dim) for side, n_q, n_c, dim in POOL_PROBE_SHAPES])


def test_bf16_round_and_parts_are_the_kernels_split3():
    torch = pytest.importorskip("torch")
    x = np.random.RandomState(0).standard_normal(4096).astype(np.float32) * np.float32(1e-3)
    x[:4] = [1.00390625, 1.01171875, 0.0, -3.0e-39]      # two ties (to even: down, up), zero, a denormal
    assert np.array_equal(bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    hi, mid, lo = bf16_parts(x, 3)
    three = hi.astype(np.float64) + mid + lo
    ok = np.abs(x) > 1e-30
    assert (np.abs(three - x)[ok] <= 2.0 ** -24 * np.abs(x)[ok]).all()             # hi + mid + lo = g to 2^-24
    two = np.abs(hi.astype(np.float64) + mid - x)[ok] / np.abs(x)[ok]
    assert two.max() > 2.0 ** -18 and (two <= 2.0 ** -16).all()                   # hi + mid alone: 2^-17 or so


@pytest.mark.parametrize("kind,side,n_q,n_c,dim", CASES)
def test_three_parts_pass_the_probes_bound_and_two_parts_do_not(kind, side, n_q, n_c, dim):
    q, c, labels, w, grad_out = loss_probe_case(kind, side, n_q, n_c, dim)
    hot = c if side == "dq" else q
    assert ((hot != 0).sum(1) == 1).all() and ((hot != 0).sum(0) <= 1).all()       # one-hot rows, an injective choice of columns
    assert np.array_equal(bf16_round(q), q) and np.array_equal(bf16_round(c), c)
    ref, loss, e3, e2 = loss_probe_errors(side, q, c, labels, w, grad_out, kind)     # (asserts the exact logits and |s - lse| <= 12)
    print(f"{kind} {side} ({n_q}, {n_c}, {dim}): E3 {e3:.3e}  E2 {e2:.3e}  bound E2 / 3 {e2 / 3:.3e}")
    assert np.isfinite(loss) and (ref != 0).sum() >= n_q * min(n_c, dim) // 2
    assert e3 < e2 / 3
    assert e2 > e2 / 3 and e2 > 2.0 ** -18     # two parts: over the bound by construction, and of the size bf16 pairs give
