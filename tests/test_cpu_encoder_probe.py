"""The selector probe of tests/test_gpu_encoder_train_edges.py held to its contract without a GPU (builder: tests/helpers.py).  The scores
keep their margin of 24, every exact gradient is a value of both 16-bit types, the unselected keys leak less than 1e-8, every column of dQ,
dK and dV is non-zero in some head, every (query tile, key tile) pair of the long sequences holds a selected key, and an fp32 + 16-bit
emulation of the kernel's arithmetic returns the exact answer -- and fails to once two streamed rows trade places."""
import numpy as np
import pytest

from helpers import (ENC_PROBE_HEADS, ENC_PROBE_LENS, ENC_PROBE_MARGIN, attention_grads_fp64, emulate_attention_bwd, encoder_probe,
                     encoder_probe_leak_bound, round16, snap_exact)

KINDS = ["bf16", "fp16"]


def _heads():
    for seq in encoder_probe():
        for h, head in enumerate(seq["heads"]):
            yield seq["length"], h, head


def test_probe_shape_and_operands():
    seqs = encoder_probe()
    assert [s["length"] for s in seqs] == ENC_PROBE_LENS == [2, 31, 33, 64, 65, 257, 512] and ENC_PROBE_HEADS == 8
    for length, h, head in _heads():
        q, k, v, d_out = head["q"], head["k"], head["v"], head["d_out"]
        for a in (q, k, v, d_out):
            assert a.shape == (length, 64) and np.array_equal(a, np.round(a)) and np.abs(a).max() <= 4
        assert not ((q != 0) & (k != 0))[:, np.roll(np.arange(64) >= 48, 8 * h)].any()       # payloads: one side is zero
        assert ((v != 0).sum(1) == 4).all()
        sizes = sorted(len(g) for g in head["groups"])
        assert sizes == [1] * (length % 2) + [2] * (length // 2)                            # pairs, one single key with an odd length
        assert sorted(m for g in head["groups"] for m in g) == list(range(length))
        if length >= 64:      # partners sit in different 32-row tiles
            assert all(g[0] // 32 != g[1] // 32 for g in head["groups"] if len(g) == 2)
        counts = np.bincount(head["select"], minlength=len(head["groups"]))
        assert length < 64 or counts.max() > 1                                              # many-to-one


def test_margin_is_at_least_24():
    for length, h, head in _heads():
        s = head["q"] @ head["k"].T * 0.125
        own = head["group_of_key"][None, :] == head["select"][:, None]
        assert (s[own] == 96.0).all(), (length, h)
        if (~own).any():
            assert (96.0 - s[~own]).min() >= ENC_PROBE_MARGIN, (length, h, (96.0 - s[~own]).min())


def test_exact_gradients_are_representable_and_the_leak_is_below_1e_8():
    worst = 0.0
    for length, h, head in _heads():
        out, lse, dq, dk, dv, p = attention_grads_fp64(head["q"], head["k"], head["v"], head["d_out"])
        sel = np.stack([np.isin(np.arange(length), head["groups"][g]) for g in head["select"]])
        want_p = sel / sel.sum(1, keepdims=True)
        assert np.abs(p - want_p).max() <= length * np.exp(-ENC_PROBE_MARGIN)
        assert np.abs(out - want_p @ head["v"]).max() <= 1e-8
        for g in (dq, dk, dv):
            exact = snap_exact(g)
            worst = max(worst, np.abs(g - exact).max())
            assert np.abs(g - exact).max() <= min(1e-8, encoder_probe_leak_bound(length)), (length, h)
            for kind in KINDS:
                assert np.array_equal(round16(exact.astype(np.float32), kind).astype(np.float64), exact), (length, h, kind)
    print(f"largest leak {worst:.2e}")


def test_every_column_is_non_zero_in_some_head():
    for seq in encoder_probe():
        if seq["length"] < 31:
            continue
        seen = np.zeros((3, 64), bool)
        share = np.zeros((3, ENC_PROBE_HEADS))
        for h, head in enumerate(seq["heads"]):
            grads = attention_grads_fp64(head["q"], head["k"], head["v"], head["d_out"])[2:5]
            for i, g in enumerate(grads):
                nz = snap_exact(g) != 0
                seen[i] |= nz.any(0)
                share[i, h] = nz.mean()
        assert seen.all(), (seq["length"], np.nonzero(~seen))
        print(f"len {seq['length']}: non-zero share per head dQ {share[0].mean():.2f} dK {share[1].mean():.2f} dV {share[2].mean():.2f}")


@pytest.mark.parametrize("length", [257, 512])
def test_every_tile_pair_holds_a_selected_key(length):
    """P >= 1/2 somewhere in every (query tile, key tile) pair of 32 x 32 rows -- the (own, streamed) pairs of the dQ pass and, transposed,
    of the dK / dV pass -- in every head.  The last query tile of length 257 has ONE row, whose pair reaches two key tiles per head: that
    tile must reach all nine over the eight heads."""
    seq = encoder_probe()[ENC_PROBE_LENS.index(length)]
    n_tiles = (length + 31) // 32
    single_row_reach = set()
    for h, head in enumerate(seq["heads"]):
        p = attention_grads_fp64(head["q"], head["k"], head["v"], head["d_out"])[5]
        hit = np.zeros((n_tiles, n_tiles), bool)
        qi, ki = np.nonzero(p >= 0.5 - 1e-8)          # (1/2 less the leak)
        hit[qi // 32, ki // 32] = True
        full = n_tiles if length % 32 == 0 else n_tiles - 1
        assert hit[:full].all(), (h, np.argwhere(~hit[:full]))
        if full < n_tiles:
            assert hit[full].sum() == 2
            single_row_reach |= set(np.nonzero(hit[full])[0].tolist())
    if length == 257:
        assert single_row_reach == set(range(n_tiles)), single_row_reach


@pytest.mark.parametrize("kind", KINDS)
def test_the_kernels_arithmetic_is_exact_on_the_probe_and_a_swapped_row_is_not(kind):
    total = differ = 0
    caught = []
    for length, h, head in _heads():
        args = (head["q"], head["k"], head["v"], head["d_out"])
        exact = [snap_exact(g) for g in attention_grads_fp64(*args)[2:5]]
        got = emulate_attention_bwd(*args, kind)
        for e, g in zip(exact, got):
            nz = e != 0
            total += int(nz.sum())
            differ += int((g[nz].astype(np.float64) != e[nz]).sum())
            assert np.abs(g[~nz]).max(initial=0.0) <= encoder_probe_leak_bound(length)
        if h < 2 and length >= 31:     # the mutant: streamed rows 5 and 6 of every tile trade places in the accumulating products
            bad = emulate_attention_bwd(*args, kind, swap_rows=(5, 6))
            moved = [np.abs(b.astype(np.float64) - e).max() for e, b in zip(exact, bad)]
            caught.append((length, h, moved))
            assert min(moved) >= 1.0 / 64, (length, h, moved)      # every one of dQ, dK, dV moves by whole units of the grid
    print(f"{kind}: {differ} of {total} non-zero elements differ from the exact value; swapped rows move dQ, dK, dV by at least "
          f"{min(min(m) for _, _, m in caught):.3f}")
    assert differ == 0
