"""The shard merges (csrc/ccr_merge.hip) on synthetic lists, against the oracle, bit for bit.

The other merge tests feed lists that a real search over iid random rows produced: a handful of (R, k) pairs and one exact tie in the
whole input.  Here the lists come from helpers.synthetic_shard_lists -- distinct interleaving ids, the last shard's beyond 32 bits,
scores from a few levels (+-inf among them), so that plateaus of equal scores straddle the cut of several lists at once -- at one
(R, k) per launch path: rank-by-counting below 600 elements, bisection from 600 on, 256 / 1024 threads at 2048 elements, the dynamic
LDS opt-in above 48 KiB, the global-memory kernels above 96 KiB or 64 lists.  The bisection and the counting kernels are right only if
(score desc, id asc) is a strict order everywhere; a `<` for a `<=` shows on exactly these inputs.

The reference is orc.merge_topk / orc.merge_short_lists, themselves held to one np.lexsort in tests/test_cpu_merge_reference.py.
No NaN scores: `precedes` is no order on them and the library promises none."""
import numpy as np
import pytest
import torch

from helpers import MERGE_CASES, canonical_order, synthetic_shard_lists
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

N_Q = 4
VARIANTS = [1, 2, 6, 0]          # levels of the generator; 0 = continuous scores


def _seed(*parts):
    s = 17
    for p in parts:
        s = (s * 1000003 + int(p)) % (2 ** 31 - 1)
    return s


def _assert_lists_equal(got_s, got_i, ref_s, ref_i):
    got_s, got_i = got_s.cpu().numpy(), got_i.cpu().numpy()
    assert got_i.shape == ref_i.shape
    assert np.array_equal(got_i, ref_i), f"ids differ in {int(np.sum(got_i != ref_i))} places, first at {np.argwhere(got_i != ref_i)[:3].tolist()}"
    assert np.array_equal(got_s.view(np.uint32), ref_s.view(np.uint32))


# ----------------------------------------------------------------------------------------- ccr_merge_topk[_strided]
@pytest.mark.parametrize("levels", VARIANTS)
@pytest.mark.parametrize("R,k", MERGE_CASES)
def test_merge_topk_equals_the_oracle(R, k, levels):
    from ccrec_amd import ops
    scores, ids = synthetic_shard_lists(R, N_Q, k, levels, _seed(R, k, levels))
    ms, mi = ops.merge_topk(torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda())
    _assert_lists_equal(ms, mi, *orc.merge_topk(scores, ids))


def test_merge_topk_orders_ids_above_2_to_32():
    """Every shard's ids on its own side of 2^32 or beyond it (offsets 0, 5e9, 2^33 + ...): the id comparison is a 64-bit one."""
    from ccrec_amd import ops
    R, k = 6, 100
    scores, ids = synthetic_shard_lists(R, N_Q, k, 2, _seed(R, k, 99))
    for r, off in enumerate([5_000_000_000, 0, 2 ** 33, 2 ** 32 - 50, 2 ** 40, 2 ** 62]):
        ids[r] += off
    ms, mi = ops.merge_topk(torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda())
    _assert_lists_equal(ms, mi, *orc.merge_topk(scores, ids))


class _Spy:
    """The loaded library with every call's arguments recorded."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


@pytest.mark.parametrize("R,k", [(8, 256), (3, 2731)])        # one LDS case, one global-memory case
def test_merge_topk_reads_rank_strided_views_in_place(R, k, monkeypatch):
    """Slices of a larger [R, n_q + 3, k] allocation: the rank stride exceeds n_q k.  The views go to the library as they are (their
    own address, their own rank stride: no hidden copy), and the rows around them -- NaN scores, id -1 -- are never read."""
    from ccrec_amd import ops
    scores, ids = synthetic_shard_lists(R, N_Q, k, 6, _seed(R, k, 7))
    big_s = torch.full((R, N_Q + 3, k), float("nan"), device="cuda")
    big_i = torch.full((R, N_Q + 3, k), -1, dtype=torch.int64, device="cuda")
    vs, vi = big_s[:, 2:2 + N_Q], big_i[:, 1:1 + N_Q]
    vs.copy_(torch.from_numpy(scores))
    vi.copy_(torch.from_numpy(ids))
    assert ops._rank_strided(vs) and ops._rank_strided(vi) and not vs.is_contiguous() and not vi.is_contiguous()
    spy = _Spy(ops.require_gpu())
    monkeypatch.setattr(ops, "require_gpu", lambda: spy)
    ms, mi = ops.merge_topk(vs, vi)
    (name, args), = spy.calls
    assert name == "ccr_merge_topk_strided"
    assert args[0].value == vs.data_ptr() and args[1].value == vi.data_ptr()
    assert args[2] == args[3] == (N_Q + 3) * k > N_Q * k
    _assert_lists_equal(ms, mi, *orc.merge_topk(scores, ids))


def test_merge_topk_lds_opt_in_follows_each_call():
    """The dynamic-LDS opt-in of the LDS merge is set per call to that call's size: a 4100-element merge (49 200 bytes) after an
    8192-element one (98 304 bytes) in the same process, and the large one again after the small one."""
    from ccrec_amd import ops
    for R, k in [(2, 4096), (4, 1025), (2, 4096), (8, 1001)]:
        scores, ids = synthetic_shard_lists(R, N_Q, k, 6, _seed(R, k, 3))
        ms, mi = ops.merge_topk(torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda())
        _assert_lists_equal(ms, mi, *orc.merge_topk(scores, ids))


def test_merge_topk_refusals():
    from ccrec_amd import ops, _lib
    s = torch.zeros(2, 1, 4097, device="cuda")
    with pytest.raises(_lib.CcrError):
        ops.merge_topk(s, torch.zeros(2, 1, 4097, dtype=torch.int64, device="cuda"))       # k > MAX_K


# ----------------------------------------------------------------------------------------- packed shard messages
OFFSET_BEYOND_32_BITS = 5_000_000_000


def _shard_ids(ids):
    """The generator's ids re-based the way shards own rows: shard 0 at row_offset 5e9 (global ids above 2^32), shard 1 with local rows in
    [2^31, 2^32) at row_offset 0 (the u32 row field's upper half), shard r >= 2 at row_offset 6e9 + r * 1 000 003.  Adding a constant
    per shard keeps every list canonical, and the shards' id ranges stay disjoint (the generator's ids are below 3 * 65 * 4096 <
    1 000 003).  Shard 1's ids are the lowest, so its entries win every plateau of equal scores and are among the kept ones.
    -> (global ids, row offsets)."""
    from helpers import MERGE_ID_SHIFT
    R = ids.shape[0]
    local = ids.copy()
    local[R - 1] -= MERGE_ID_SHIFT
    assert 0 <= local.min() and local.max() < 1_000_003
    offsets = [OFFSET_BEYOND_32_BITS if r == 0 else 0 if r == 1 else 6_000_000_000 + r * 1_000_003 for r in range(R)]
    if R > 1:
        local[1] += 2 ** 31
    return local + np.array(offsets, np.int64)[:, None, None], offsets


def _with_neg_inf_tail(scores, ids, k_valid):
    """The first k_valid entries of every list of one shard ([n_q, k]), the last min(3, k_valid) of them scoring a REAL -inf (they must
    precede the padding slots, which are -inf with ids above every real one); canonical order restored."""
    s, i = scores[:, :k_valid].copy(), ids[:, :k_valid].copy()
    s[:, k_valid - min(3, k_valid):] = -np.inf
    for q in range(s.shape[0]):
        o = canonical_order(s[q], i[q])
        s[q], i[q] = s[q][o], i[q][o]
    return s, i


def _gather(n_q, k, shards):
    """shards: per rank (scores [n_q, k_valid], global ids, row_offset, n_rows) -> the gathered ShardMessage, filled through
    ShardMessage.fill and copied side by side as an all-gather would leave them."""
    from ccrec_amd.dist import ShardMessage
    world = len(shards)
    gathered = ShardMessage(n_q, k, "cuda", world)
    for r, (s, i, off, n_rows) in enumerate(shards):
        m = ShardMessage(n_q, k, "cuda", 1)
        m.fill(torch.from_numpy(np.ascontiguousarray(s)).cuda(), torch.from_numpy(np.ascontiguousarray(i)).cuda(), off, n_rows)
        gathered.recv.view(world, -1)[r].copy_(m.send)
    return gathered


def _assert_decoded(gathered, shards):
    """decoded() gives back what went in (ids beyond 32 bits, rows in the u32 field's upper half) and pads the rest."""
    gs, gi = (t.cpu().numpy() for t in gathered.decoded())
    for r, (s, i, _, _) in enumerate(shards):
        kv = s.shape[1]
        assert np.array_equal(gi[r, :, :kv], i) and np.array_equal(gs[r, :, :kv].view(np.uint32), s.view(np.uint32))
        assert np.all(np.isneginf(gs[r, :, kv:])) and np.all(gi[r, :, kv:] >= 2 ** 62)
    return gs, gi


def _message_arrangements(R):
    """k_valid kinds per shard: "full" (k_valid = k), "part" (0 < k_valid < k, real -inf scores last), "none" (k_valid = 0).  Two shards
    cannot show all three at once, so they run two arrangements.  Shard 1 -- the one whose local rows fill the upper half of the u32 row
    field -- is full in every arrangement, so those rows are decoded on every launch path; shard 0 (row_offset 5e9) holds entries in
    all but the second two-shard arrangement.  With a full shard k real entries exist: the padding slots take part in every search for a
    cut but none reaches the result (the test below covers that)."""
    if R == 2:
        return [["part", "full"], ["none", "full"]]
    return [[("part", "full", "none")[r % 3] for r in range(R)]]


@pytest.mark.parametrize("levels", VARIANTS)
@pytest.mark.parametrize("R,k", [(3, 100), (6, 100), (8, 256), (4, 1025), (2, 4096), (3, 2731)])
def test_merge_shard_messages_equals_the_oracle(R, k, levels):
    scores, ids = synthetic_shard_lists(R, N_Q, k, levels, _seed(R, k, levels, 1))
    ids, offsets = _shard_ids(ids)
    for kinds in _message_arrangements(R):
        shards = []
        for r, kind in enumerate(kinds):
            if kind == "full":
                s, i = scores[r], ids[r]
            elif kind == "part":
                s, i = _with_neg_inf_tail(scores[r], ids[r], (k + 1) // 2)
            else:
                s, i = scores[r][:, :0], ids[r][:, :0]
            shards.append((s, i, offsets[r], 3 * k))
        assert shards[1][1].shape[1] == k and (shards[1][1] - offsets[1]).min() >= 2 ** 31       # the high rows are there
        gathered = _gather(N_Q, k, shards)
        gs, gi = _assert_decoded(gathered, shards)
        ms, mi = gathered.merge()
        ref_s, ref_i = orc.merge_topk(gs, gi)
        assert all(np.isin(ids[1, q], ref_i[q]).any() for q in range(N_Q))                        # ... and some of them are kept
        _assert_lists_equal(ms, mi, ref_s, ref_i)


@pytest.mark.parametrize("R,k", [(3, 100), (2, 4096)])
def test_merge_shard_messages_with_fewer_real_entries_than_k(R, k):
    """All shards together hold fewer than k entries: the result is every real entry in the canonical order (real -inf scores included),
    then padding slots -- -inf, distinct ids in (2^62, PAD_ID].  (The order of the padding tail is the slots', not the canonical one, and
    lists that end in several padding slots are outside what orc.merge_topk takes; the real entries go against one lexsort.)"""
    from ccrec_amd.dist import PAD_ID
    scores, ids = synthetic_shard_lists(R, N_Q, k, 6, _seed(R, k, 5))
    ids, offsets = _shard_ids(ids)
    shards = []
    empty = 0 if R == 2 else 2                     # never shard 1: its local rows, in [2^31, 2^32), are decoded here too
    for r in range(R):
        s, i = _with_neg_inf_tail(scores[r], ids[r], k // (R + 1)) if r != empty else (scores[r][:, :0], ids[r][:, :0])
        shards.append((s, i, offsets[r], 3 * k))
    assert (shards[1][1] - offsets[1]).min() >= 2 ** 31
    gathered = _gather(N_Q, k, shards)
    _assert_decoded(gathered, shards)
    ms, mi = (t.cpu().numpy() for t in gathered.merge())
    n_real = sum(s.shape[1] for s, _, _, _ in shards)
    for q in range(N_Q):
        s = np.concatenate([sh[0][q] for sh in shards])
        i = np.concatenate([sh[1][q] for sh in shards])
        o = canonical_order(s, i)
        assert np.array_equal(mi[q, :n_real], i[o]) and np.array_equal(ms[q, :n_real].view(np.uint32), s[o].view(np.uint32))
        tail = mi[q, n_real:]
        assert np.all(np.isneginf(ms[q, n_real:])) and np.all(tail > 2 ** 62) and np.all(tail <= PAD_ID) and len(set(tail.tolist())) == k - n_real


def test_merge_shard_messages_refuses_65_shards():
    from ccrec_amd import ops, _lib
    nbytes = ops.shard_message_bytes(1, 1)
    with pytest.raises(_lib.CcrError):
        ops.merge_shard_messages(torch.zeros(65 * nbytes, dtype=torch.uint8, device="cuda"), 65, 1, 1)


# ----------------------------------------------------------------------------------------- short lists
SHORT_CASES = [(1, 10, 10), (4, 50, 50), (3, 157, 300), (64, 16, 100), (8, 140, 1001), (2, 600, 1024), (8, 1024, 4096)]


def _short_arrangements(R, k_list):
    """Per arrangement and shard (kind, k_valid).  Shard 0 and, from four shards on, the last one: "cut" (sent k_list entries of a
    longer shard: n_rows > k_valid); every third shard: "small" (holds fewer rows than k_list and sent them all: k_valid < k_list); the
    others: "all" (k_list rows, all sent).  Two shards run a second arrangement whose shard 1 is small -- by a quarter, so that the real
    entries still fill k_out = 1024 of the (2, 600, 1024) case; one shard can only be cut."""
    def kind(r):
        if r == 0 or (R >= 4 and r == R - 1):
            return "cut"
        return "small" if r % 3 == 2 else "all"
    first = [(kind(r), k_list - k_list // 3 if kind(r) == "small" else k_list) for r in range(R)]
    return [first, [("cut", k_list), ("small", k_list - k_list // 4)]] if R == 2 else [first]


def _tier_scores(kl, tier):
    return (10.0 * tier + 1.0 - (np.arange(kl) + 1.0) / (kl + 1.0)).astype(np.float32)


@pytest.mark.parametrize("levels", VARIANTS)
@pytest.mark.parametrize("R,k_list,k_out", SHORT_CASES)
def test_merge_short_lists_equals_the_oracle(R, k_list, k_out, levels):
    """Queries 0 .. N_Q - 1: the generator's.  Query N_Q: shard 0 -- truncated -- holds the best k_list entries, its list is consumed and
    the query flagged.  Query N_Q + 1 (two shards or more): the best entries are those of shard 1, which sent everything it has, then
    those of the other complete shards; the truncated shards rank last with one score profile (ties across shards down to the id) and
    none of them is consumed: no flag."""
    from ccrec_amd import ops
    n_q = N_Q + (2 if R > 1 else 1)
    scores, ids = synthetic_shard_lists(R, n_q, k_list, levels, _seed(R, k_list, k_out, levels))
    ids, offsets = _shard_ids(ids)
    for r in range(R):
        scores[r, N_Q] = _tier_scores(k_list, 2 if r == 0 else 0) + (0 if r == 0 else np.float32(r) / 64)
        if R > 1:
            scores[r, N_Q + 1] = _tier_scores(k_list, 3 if r == 1 else 1 if r == 0 or (R >= 4 and r == R - 1) else 2)
    for arrangement in _short_arrangements(R, k_list):
        shards, truncated = [], []
        for r, (kind, kv) in enumerate(arrangement):
            shards.append((scores[r][:, :kv], ids[r][:, :kv], offsets[r], 10 * k_list if kind == "cut" else kv))
            truncated.append(kind == "cut")
        gathered = _gather(n_q, k_list, shards)
        gs, gi = _assert_decoded(gathered, shards)
        ref_s, ref_i, ref_flags = orc.merge_short_lists(gs, gi, truncated, k_out)
        assert ref_flags[N_Q] == 1 and (R == 1 or ref_flags[N_Q + 1] == 0)       # the two constructions do what they say
        assert not (ref_i >= 2 ** 62).any()                                      # real entries fill every list: no padding slot is kept
        ms, mi, flags, count = ops.merge_short_lists(gathered.recv, R, n_q, k_list, k_out)
        _assert_lists_equal(ms, mi, ref_s, ref_i)
        assert np.array_equal(flags.cpu().numpy(), ref_flags)
        assert int(count) == int(ref_flags.sum())


def test_merge_short_lists_refusals():
    """The library's own refusals (ops.merge_short_lists asserts the same shapes before it calls)."""
    from ccrec_amd import ops, _lib
    lib = ops.require_gpu()

    def call(R, n_q, k_list, k_out):
        buf = torch.zeros(R * ops.shard_message_bytes(n_q, k_list), dtype=torch.uint8, device="cuda")
        os_ = torch.empty(n_q, k_out, device="cuda")
        oi = torch.empty(n_q, k_out, dtype=torch.int64, device="cuda")
        flags = torch.zeros(n_q + 1, dtype=torch.int32, device="cuda")
        _lib.check(lib.ccr_merge_short_lists(ops._ptr(buf), buf.numel() // R, R, n_q, k_list, k_out, ops._ptr(os_), ops._ptr(oi),
                                             ops._ptr(flags), ops._ptr(flags[n_q:]), ops._stream(buf)), "ccr_merge_short_lists")

    with pytest.raises(_lib.CcrError):
        call(2, 1, 12, 10)            # k_list > k_out
    with pytest.raises(_lib.CcrError):
        call(2, 1, 4, 9)              # R * k_list < k_out
    with pytest.raises(_lib.CcrError):
        call(8, 1, 1025, 4096)        # R * k_list * 12 = 98 400 bytes > 96 KiB
    with pytest.raises(_lib.CcrError):
        call(65, 1, 4, 8)             # R > 64
    for bad in [(2, 12, 10), (2, 4, 9), (8, 1025, 4096)]:
        with pytest.raises(AssertionError):
            ops.merge_short_lists(torch.zeros(bad[0] * 16, dtype=torch.uint8, device="cuda"), bad[0], 1, bad[1], bad[2])
