"""The probes of tests/test_gpu_bpr_edges.py, checked without a GPU: the integer probe gives xh = +-1 and the intended difference under an
fp32 emulation of the kernel's LayerNorm steps, zero-weight rows leave a live row's sums unchanged in the kernel's order of additions, and
why the probes are needed: the aggregate bounds of tests/test_gpu_bpr.py pass a lost batch row and a softplus without relative precision."""
import math

import numpy as np
import pytest
import torch

from helpers import (BPR_PROBE_KS, bpr_integer_probe, bpr_probe_reference, bpr_relative_error, check_grad, check_loss, frozen_problem,
                     restate_frozen)

f32 = np.float32


# ---------------------------------------------------------------------------------------------- csrc/ccr_bpr.hip in numpy fp32
def to_lanes(x):
    """A row as the kernel holds it: [NV, 64 lanes, 4], chunk lane + 64 i; chunks beyond the row are zero."""
    dim = x.size
    nv = (dim + 255) // 256
    v = np.zeros((nv * 64, 4), f32)
    v[:dim // 4] = np.asarray(x, f32).reshape(-1, 4)
    return v.reshape(nv, 64, 4), np.arange(nv * 64).reshape(nv, 64) < dim // 4


def wave_sum(v):
    v = np.asarray(v, f32).copy()
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[np.arange(64) ^ off]).astype(f32)
    assert (v == v[0]).all()
    return v[0]


def fmaf(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)      # (exact for the probe's operands)


def normalize(x, eps):
    v, inside = to_lanes(x)
    inv_dim = f32(1.0) / f32(x.size)
    s = np.zeros(64, f32)
    for i in range(v.shape[0]):
        s = (s + ((v[i, :, 0] + v[i, :, 1]) + (v[i, :, 2] + v[i, :, 3]))).astype(f32)
    mean = f32(wave_sum(s) * inv_dim)
    v = np.where(inside[..., None], (v - mean).astype(f32), f32(0))
    q = np.zeros(64, f32)
    for i in range(v.shape[0]):
        for c in range(4):
            q = fmaf(v[i, :, c], v[i, :, c], q)
    rstd = f32(1.0) / np.sqrt(f32(wave_sum(q) * inv_dim + f32(eps)))
    return (v * rstd).astype(f32), mean, rstd


def dot_diff(q, a, b):
    s = np.zeros(64, f32)
    for i in range(q.shape[0]):
        for c in range(4):
            s = fmaf(q[i, :, c], (a[i, :, c] - b[i, :, c]).astype(f32), s)
    return wave_sum(s)


@pytest.mark.parametrize("dim,gamma", [(64, 1.0), (64, 0.5), (2048, 1.0)])
def test_integer_probe_is_exact_in_the_kernels_arithmetic(dim, gamma):
    seen = set()
    for k in BPR_PROBE_KS:
        for variant in (0, 1):
            xi, xj, xn, flipped = bpr_integer_probe(dim, k, variant)
            rows = []
            for x in (xi, xj, xn):
                xh, mean, rstd = normalize(x, 0.0)
                assert mean == 0 and rstd == 1 and np.array_equal(xh.reshape(-1)[:dim].view(np.uint32), x.view(np.uint32))      # bit for bit
                rows.append(xh)
            g = f32(gamma)
            q = ((rows[0] * g + f32(0)) * g).astype(f32)
            D = float(dot_diff(q, rows[1], rows[2]))
            assert D == gamma * gamma * 4 * k == bpr_probe_reference(xi, xj, xn, gamma)[0]
            assert np.array_equal(np.nonzero(xj != xn)[0], flipped) and len(flipped) >= 2
            seen.add(D)
    step = 4 if gamma == 1.0 else 1
    assert seen == set(float(d) for d in range(-32 * step, 32 * step + 1, step))      # -128 .. 128 by 4, or every integer of -32 .. 32


def sigmoid_neg(d):
    e = np.exp(-np.abs(f32(d)), dtype=f32)
    return f32((e if d >= 0 else f32(1)) / (f32(1) + e))


def backward_row(acc_g, acc_b, xi, xj, xns, Ds, wb, gamma, beta):
    """One trip of bpr_frozen_bwd_kernel's row loop on whole rows: dg, db += R (2 xh_i gamma + beta), R gamma."""
    G, C = f32(0), np.zeros_like(xi)
    for xn, D in zip(xns, Ds):
        gn = f32(-f32(wb) * sigmoid_neg(D))
        G = f32(G + gn)
        C = (C + gn * xn).astype(f32)
    R = (G * xj - C).astype(f32)
    return (acc_g + R * (f32(2) * xi * gamma + beta)).astype(f32), (acc_b + R * gamma).astype(f32)


def test_zero_weight_rows_leave_the_live_rows_sums_unchanged():
    """Part A's argument: w = 0 gives g = -0 sigma = -0, G = +0, C = +-0 and R = +-0, and adding +-0 is exact -- before the live row, after it,
    in the other waves' shares (added through LDS) and in the other workgroups' partial rows."""
    rng = np.random.default_rng(0)
    dim, n_neg = 64, 2
    gamma = (0.05 * (1 + 0.2 * rng.standard_normal(dim))).astype(f32)
    beta = (0.02 * rng.standard_normal(dim)).astype(f32)

    def row():
        x = rng.standard_normal((2 + n_neg, dim)).astype(f32)
        xh = ((x - x.mean(1, keepdims=True)) / x.std(1, keepdims=True)).astype(f32)
        return xh[0], xh[1], xh[2:], (rng.standard_normal(n_neg) * 3).astype(f32)

    live = row()
    alone = backward_row(np.zeros(dim, f32), np.zeros(dim, f32), *live, 0.7, gamma, beta)
    assert np.abs(alone[0]).min() > 0 and np.abs(alone[1]).min() > 0
    for position in (0, 1, 4):                       # the live row on a wave's first, second and last trip of five
        acc = np.zeros(dim, f32), np.zeros(dim, f32)
        for trip in range(5):
            acc = backward_row(*acc, *(live if trip == position else row()), 0.7 if trip == position else 0.0, gamma, beta)
        dead = np.zeros(dim, f32), np.zeros(dim, f32)
        for trip in range(5):
            dead = backward_row(*dead, *row(), 0.0, gamma, beta)
        assert not dead[0].any() and not dead[1].any()
        for mine, other, lone in zip(acc, dead, alone):
            total = mine
            for _ in range(3):                       # the workgroup's other three waves, then 511 partial rows of zeros
                total = (total + other).astype(f32)
            for _ in range(511):
                total = (total + f32(-1) * other).astype(f32)      # (zeros of either sign)
            assert np.array_equal(total, lone)
    # forward: the row's share is w acc = 0, and the fp64 sum of the shares is the live row's alone
    assert f32(0) * f32(12.5) == 0 and float(np.float64(f32(0.7) * f32(1.25)) + 0.0) == float(f32(0.7) * f32(1.25))


def test_the_aggregate_bound_passes_a_lost_row_that_the_live_row_comparison_sees():
    """B = 4100 batch rows.  Where the rows pull the same way -- here they are copies of one (i, j, negatives) triple with equal weights --
    a backward that drops one of them gives (B - 1) / B of the gradient: 2.4e-4 of its size, inside check_grad's 3e-4 max |ref|.  With the
    weight on that row alone, the same backward returns zeros where the reference does not.  (On random rows the sum is incoherent and a
    lost row moves an element by 15 to 130 times the bound at this B, measured on frozen_problem(4100, 2, 64, 500): there the old bound
    would have noticed, had any test run a B past 2048.)"""
    B, lost = 4100, 2050
    table, gamma, beta, ptr_i, ptr_j, ptr_nj, _ = frozen_problem(B, 2, 64, 500)
    ptr_i, ptr_j, ptr_nj = ptr_i[7].expand(B).clone(), ptr_j[7].expand(B).clone(), ptr_nj[:, 7:8].expand(2, B).clone()
    w = torch.full((B,), 0.5)
    ref, dg, db, _ = restate_frozen(table, gamma, beta, 1e-5, ptr_i, ptr_j, ptr_nj, w)
    assert np.abs(dg).max() > 0 and np.abs(db).max() > 0
    share = float(w[lost] / w.double().sum())                  # by linearity: the lost row's part of the numerator, the denominator unchanged
    dropped_g, dropped_b = dg * (1 - share), db * (1 - share)
    check_grad(torch.from_numpy(dropped_g), dg, what="dgamma without one row")      # the old check passes
    check_grad(torch.from_numpy(dropped_b), db, what="dbeta without one row")
    one = torch.zeros(B)
    one[lost] = 0.7
    _, dg1, db1, _ = restate_frozen(table, gamma, beta, 1e-5, ptr_i, ptr_j, ptr_nj, one)
    assert np.abs(dg1).min() > 0 and np.abs(db1).min() > 0     # the live-row comparison: a backward that drops the row returns 0 in every column
    assert not np.array_equal(np.zeros_like(dg1), dg1)


def test_softplus_without_relative_precision_passes_the_loss_bound_and_fails_the_probe():
    D = 20.0
    ref = math.log1p(math.exp(-D))
    naive = float(np.log(f32(1) + np.exp(f32(-D), dtype=f32), dtype=f32))          # logf(1 + e): 1 + 2e-9 rounds to 1
    good = float(np.log1p(np.exp(f32(-D), dtype=f32), dtype=f32))
    check_loss(naive, ref)                                                           # |0 - 2.06e-9| < 2e-5: the old bound passes it
    assert bpr_relative_error(naive, ref) > 2.0 ** -20
    assert bpr_relative_error(good, ref) <= 2.0 ** -20
    assert bpr_relative_error(0.0, 2.0 ** -149) == 0.0 and bpr_relative_error(2.0 ** -149, 3 * 2.0 ** -149) == pytest.approx(1 / 3)
