"""The two forms of the sample-threshold kernel (threshold_kernel: 16 or 64 group phases per query, CCR_THR_PHASES pins one): a
histogram count does not depend on the order of its adds, so both forms give the same thresholds bit for bit -- the same ids and
score BITS, equal to the oracle's, and the same n_candidates / n_fallback / n_retried / skipped_tiles (n_candidates is a function of
the thresholds alone).  Every shape is a single-launch estimated-threshold plan (CCR_OPTIMISTIC=1, checked on the CPU with the
planner), with the sample pinned so that n_groups = 16 x sample tiles lands on 160 (64 phases: two or three groups each, the
remainder loop only), 1 008 / 1 024 / 1 040 (the unrolled loop of the 64-phase form exactly below, at and above its first
batch) and 2 064 (two batches and a remainder); with CCR_SKIP_SAMPLED 0 and 1 both instantiations (without / with the select's
short list) run.  Batches of at most 128 queries take the small-batch threshold kernel whatever the knob says (phases reported 0)."""
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

DENSE, FUSED = 1, 2
OFFSET = 4321
DIM = 64
PLAN = {"CCR_NARROW": 0, "CCR_OPTIMISTIC": 1, "CCR_SAMPLE_DIV": 4}
STATS = ("n_candidates", "n_fallback", "n_retried", "skipped_tiles")
# rows -> n_groups under CCR_SAMPLE_DIV=4: ceil(tiles / 4) sampled tiles of 16 groups (the last corpus tile is partial everywhere but at 65 536)
ROWS = {160: 10_206, 1008: 64_507, 1024: 65_536, 1040: 66_555, 2064: 132_090}


def _bf16(bits):
    return torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16).cuda()


_bits, _refs = {}, {}


def _rand_bits(n, seed):
    """Seeded bf16 rows, made once per shape and left unchanged."""
    if (n, seed) not in _bits:
        g = torch.Generator().manual_seed(seed)
        _bits[(n, seed)] = orc.pack_bf16((torch.randn(n, DIM, generator=g) * DIM ** -0.5).numpy())
    return _bits[(n, seed)]


def _oracle(n, nq, k):
    """The oracle's answer of a shape, computed once and shared by its two cases."""
    if (n, nq, k) not in _refs:
        _refs[(n, nq, k)] = orc.canonical_search(_rand_bits(nq, nq + 5), _rand_bits(n, n + 3), k, None)
    return _refs[(n, nq, k)]


@contextmanager
def _knobs(**kv):
    """Environment knobs are read ONCE, when an index is created."""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _index(D, **kv):
    from ccrec_amd import ops
    with _knobs(**kv):
        return ops.CorpusIndex(D, global_row_offset=OFFSET)


def _search(D, Q, k, phases, skip, groups, nq):
    index = _index(D, CCR_THR_PHASES=phases, CCR_SKIP_SAMPLED=skip, **PLAN)
    s, i = index.search(Q, k, FUSED)
    st = index.last_stats()
    print("phases", phases, "->", index.last_threshold_phases(), st)
    assert st["path"] == 1 and st["main_launches"] == 1 and st["opt_rank"] > 0, st
    assert st["sample_tiles"] * 16 == groups and (st["skipped_tiles"] > 0) == bool(skip), st
    assert index.last_threshold_phases() == (phases if nq > 128 else 0)
    return s, i, st, index


@pytest.mark.parametrize("skip", [0, 1], ids=["every tile", "skip"])
@pytest.mark.parametrize("nq,k,groups", [
    (65, 10, 160),       # the small-batch threshold kernel (at most 128 queries): the knob changes nothing
    (129, 1, 160),       # the smallest batch of threshold_kernel; 160 groups in 64 phases: two or three each
    (257, 10, 160),
    (257, 1, 1008),      # 64 phases: one group short of a full batch, remainder loop only
    (400, 100, 1024),    # exactly one batch, no remainder
    (257, 10, 1040),     # one batch and a remainder of one group in sixteen of the phases
    (65, 100, 1040),
    (400, 100, 2064),    # two batches and a remainder
    (257, 1, 2064),
])
def test_both_phase_counts_give_the_same_search(nq, k, groups, skip):
    n = ROWS[groups]
    Db, Qb = _rand_bits(n, n + 3), _rand_bits(nq, nq + 5)
    D, Q = _bf16(Db), _bf16(Qb)
    s16, i16, st16, _ = _search(D, Q, k, 16, skip, groups, nq)
    s64, i64, st64, _ = _search(D, Q, k, 64, skip, groups, nq)
    assert torch.equal(i16, i64) and torch.equal(s16.view(torch.int32), s64.view(torch.int32))
    assert [st16[f] for f in STATS] == [st64[f] for f in STATS], (st16, st64)
    ref_i, ref_s = _oracle(n, nq, k)
    assert np.array_equal(i64.cpu().numpy() - OFFSET, ref_i), f"ids differ in {np.sum(i64.cpu().numpy() - OFFSET != ref_i)} places"
    assert np.array_equal(s64.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))


def test_the_launcher_picks_the_wide_form_by_the_size_of_the_sample():
    """Unpinned: 64 phases from 2 048 sampled groups on (two full batches of 16 loads per phase and pass), 16 below."""
    for groups, want in ((1040, 16), (2064, 64)):
        n, nq, k = ROWS[groups], 257, 10
        index = _index(_bf16(_rand_bits(n, n + 3)), **PLAN)
        s, i = index.search(_bf16(_rand_bits(nq, nq + 5)), k, FUSED)
        st = index.last_stats()
        assert st["path"] == 1 and st["sample_tiles"] * 16 == groups, st
        assert index.last_threshold_phases() == want
        ref_i, ref_s = _oracle(n, nq, k)
        assert np.array_equal(i.cpu().numpy() - OFFSET, ref_i) and np.array_equal(s.cpu().numpy().view(np.uint32), ref_s.view(np.uint32))


@pytest.mark.parametrize("skip", [0, 1], ids=["every tile", "skip"])
def test_a_nan_row_poisons_every_threshold_in_both_forms(skip):
    """A NaN corpus row: the shard's norm bound is not finite, every threshold becomes NaN, nothing is recorded and the dense path
    answers every query -- the same bits from both forms and from the forced dense search."""
    n, nq, k, groups = ROWS[1040], 257, 10, 1040
    Db = _rand_bits(n, n + 3).copy()
    Db[12_345] = 0x7FC0
    D, Q = _bf16(Db), _bf16(_rand_bits(nq, nq + 5))
    out = []
    for phases in (16, 64):
        index = _index(D, CCR_THR_PHASES=phases, CCR_SKIP_SAMPLED=skip, **PLAN)
        s, i = index.search(Q, k, FUSED)
        st = index.last_stats()
        print(phases, st)
        assert st["path"] == 1 and st["sample_tiles"] * 16 == groups and index.last_threshold_phases() == phases, st
        assert st["n_fallback"] == nq and st["n_candidates"] == 0, st
        out.append((s, i, [st[f] for f in STATS]))
    sd, idn = index.search(Q, k, DENSE)
    for s, i, _ in out:
        assert torch.equal(i, idn) and torch.equal(s.view(torch.int32), sd.view(torch.int32))
    assert out[0][2] == out[1][2]


def test_sixteen_waves_agree_on_every_histogram_fifty_times():
    """The 64-phase form exchanges histogram data between 16 waves through LDS: a barrier passed with a histogram add still in flight
    would change a digit count, a threshold and with it n_candidates.  Fifty searches on one index: one value."""
    n, nq, k, groups = ROWS[2064], 400, 100, 2064
    D, Q = _bf16(_rand_bits(n, n + 3)), _bf16(_rand_bits(nq, nq + 5))
    s0, i0, st0, index = _search(D, Q, k, 64, 1, groups, nq)
    seen = set()
    for _ in range(50):
        s, i = index.search(Q, k, FUSED)
        seen.add(index.last_stats()["n_candidates"])
    assert seen == {st0["n_candidates"]}, seen
    assert torch.equal(i, i0) and torch.equal(s.view(torch.int32), s0.view(torch.int32))
