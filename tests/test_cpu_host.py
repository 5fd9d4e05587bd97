"""CPU-side checks: the C-ABI library loads and exports every symbol include/ccr_retrieval.h declares
(no compute calls without a GPU), the host mirror keeps the reference's config/error behaviour, and the
multi-process exchange path (all-gather of per-shard top-k + merge) is correct under gloo, world_size 2."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, PKG, has_gpu


def test_header_symbols_are_exported():
    from ccrec_amd import _lib
    header = open(os.path.join(ROOT, "include", "ccr_retrieval.h")).read()
    declared = set(re.findall(r"\b(ccr_[a-z0-9_]+)\s*\(", header))
    declared -= {"ccr_index", "ccr_search_stats"}
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} not exported by libccr_hip.so"
    assert lib.ccr_version() >= 100
    assert lib.ccr_last_error() is not None


def test_header_is_plain_c_and_links_against_the_library(tmp_path):
    """include/ccr_retrieval.h must be usable from C (the reference-side binding could be cgo / ctypes / a C extension): a C
    translation unit that takes the address of every declared entry point compiles with gcc -std=c99 -pedantic and links
    against the in-tree library; run without a GPU it reports the version and an error string (no compute call)."""
    import subprocess
    from ccrec_amd import _lib
    header = open(os.path.join(ROOT, "include", "ccr_retrieval.h")).read()
    names = sorted(set(re.findall(r"\b(ccr_[a-z0-9_]+)\s*\(", header)) - {"ccr_index", "ccr_search_stats"})
    src = tmp_path / "abi.c"
    src.write_text("#include <stdio.h>\n#include \"ccr_retrieval.h\"\n"
                   "typedef void (*fn)(void);\n"
                   "static fn table[] = {" + ", ".join(f"(fn){n}" for n in names) + "};\n"
                   "int main(void) {\n"
                   "    ccr_search_stats st; (void)st;\n"
                   "    printf(\"%d %d %s|\\n\", (int)(sizeof(table) / sizeof(table[0])), ccr_version(), ccr_last_error());\n"
                   "    return ccr_index_rows(NULL) == -1 ? 0 : 1;\n}\n")
    exe = tmp_path / "abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", libdir, "-lccr_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.split()[0] == str(len(names)) and int(run.stdout.split()[1]) >= 100


def test_planner_invariants_on_cpu(tmp_path):
    """The search planner is host code (ccr::make_plan, csrc/ccr_plan.hip, in the library): tests/native/planner_check.cpp walks 800+ shapes --
    every BASELINE config among them -- and checks range / phase / sample / candidate-segment / workspace-layout invariants
    (phases are whole rounds of work items, capacities hold one whole tile, segments do not overlap ...).  No GPU call."""
    import shutil
    import subprocess
    from ccrec_amd import _lib
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = tmp_path / "planner_check"
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = [hipcc, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "native", "planner_check.cpp"), "-o", str(exe), "-L", libdir, "-lccr_hip", f"-Wl,-rpath,{libdir}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.endswith(", 0 violations") and int(last.split()[0]) > 500, last
    nq_line = [ln for ln in run.stdout.splitlines() if ln.startswith("n=2681468 nq=3452 k=100:")][0]
    # NQ on the 256 x 384 tile: nine query blocks x 14 range rows = 126 items per XCD set = 3.94 rounds of its 32 workgroups, one launch
    assert "items/XCD-set 126 = 3.94 rounds" in nq_line and "phases end at 0 / 0" in nq_line, nq_line


def test_library_is_in_tree_and_has_no_torch_dependency():
    from ccrec_amd import _lib
    assert _lib.LIB_PATH.startswith(PKG)
    import subprocess
    # library NAMES only: the addresses ldd/readelf print beside them can contain any hex string (e.g. "c10")
    out = subprocess.run(["readelf", "-d", _lib.LIB_PATH], capture_output=True, text=True).stdout
    needed = re.findall(r"\(NEEDED\)\s+Shared library: \[([^\]]+)\]", out)
    assert any(n.startswith("libamdhip64") for n in needed), needed
    assert not any(("torch" in n) or ("c10" in n) for n in needed), needed


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU behaviour")
def test_product_path_fails_loudly_without_gpu():
    from ccrec_amd import _lib, ops
    from ccrec_amd.ms_marco_eval import ranking, cos_sim
    os.environ["CCREC_SIM_TYPE"] = "dot"
    with pytest.raises(_lib.CcrError, match="no CPU fallback"):
        ranking({"p": 0}, {"q": 0}, lambda rows: torch.zeros(len(rows), 8), 4)
    with pytest.raises(_lib.CcrError):
        cos_sim(torch.zeros(2, 8), torch.zeros(3, 8))
    with pytest.raises(_lib.CcrError):
        ops.require_gpu()


def test_product_package_never_imports_the_oracle():
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src and "oracle/_" not in src, f


def test_env_defaults_follow_reference_names():
    import ccrec_amd
    names = [n for n, _, _ in ccrec_amd.env_defaults]
    for n in ["CCREC_EMBEDDING_TYPE", "CCREC_MAX_LENGTH", "CCREC_SIM_TYPE", "CCREC_BBPR_INV_TEMPERATURE", "CCREC_NON_BLOCKING"]:
        assert n in names and n in os.environ
    old = os.environ["CCREC_SIM_TYPE"]
    os.environ["CCREC_SIM_TYPE"] = "euclid"
    try:
        with pytest.raises(AssertionError):
            ccrec_amd.init_env_defaults()
    finally:
        os.environ["CCREC_SIM_TYPE"] = old


def test_shard_bounds_partition():
    from ccrec_amd.dist import shard_bounds
    for n, w in [(10, 3), (2681468, 8), (7, 8), (256, 2)]:
        b = [shard_bounds(n, w, r) for r in range(w)]
        assert b[0][0] == 0 and b[-1][1] == n
        assert all(b[i][1] == b[i + 1][0] for i in range(w - 1))
        assert max(h - l for l, h in b) - min(h - l for l, h in b) <= 1


def test_shard_bounds_by_weight():
    """shard_bounds(weights=...): contiguous blocks of equal WEIGHT (token counts).  A corpus sorted by passage length -- the case where
    equal row counts leave the last rank with several times the tokens of the first -- gives every rank the same tokens within 2 %;
    the blocks partition the rows; zero weights / a single heavy row / more ranks than rows stay well-formed."""
    from ccrec_amd.dist import shard_bounds, weighted_cuts
    from ccrec_amd.encode import token_weights
    rs = np.random.RandomState(0)
    lens = np.sort(np.clip(rs.lognormal(4.6, 0.6, 200_000), 8, 512).astype(np.int64))       # sorted by length: 8 .. 512 tokens
    for world in (2, 3, 8):
        b = [shard_bounds(len(lens), world, r, lens) for r in range(world)]
        assert b[0][0] == 0 and b[-1][1] == len(lens) and all(b[i][1] == b[i + 1][0] for i in range(world - 1))
        tok = np.array([lens[lo:hi].sum() for lo, hi in b], np.float64)
        assert tok.max() / tok.min() < 1.02, tok
        rows = np.array([shard_bounds(len(lens), world, r) for r in range(world)])
        tok_rows = np.array([lens[lo:hi].sum() for lo, hi in rows], np.float64)
        if world == 8:
            assert tok_rows.max() / tok_rows.min() > 3.0          # what equal row counts would have cost
    assert weighted_cuts(np.zeros(10), 3) == [0, 4, 7, 10]                        # nothing to balance: equal rows
    assert weighted_cuts([0, 0, 100, 0, 0], 2)[1] in (2, 3) and weighted_cuts([1, 1], 4)[-1] == 2
    assert weighted_cuts([1000, 1, 1, 1], 4) == [0, 1, 2, 3, 4] and weighted_cuts([1, 1, 1, 1000], 4) == [0, 1, 2, 3, 4]   # no rank without rows
    assert weighted_cuts([5, 0, 0, 0, 0, 5], 3) in ([0, 1, 2, 6], [0, 1, 5, 6])
    cuts = weighted_cuts(rs.randint(1, 50, 7), 8)
    assert cuts[0] == 0 and cuts[-1] == 7 and all(a <= b_ for a, b_ in zip(cuts, cuts[1:]))
    # the estimate every rank computes without a tokeniser: words x 1.3 + 2, clipped to max_length
    w = token_weights(["a b c", "", "x " * 400], 256)
    assert w.tolist() == [3 * 1.3 + 2, 2.0, 256.0]

    class Pieces:      # 2 tokens per word + 2 special tokens: the fit on a sample recovers both constants
        def __call__(self, texts, truncation=True, padding=False, max_length=64):
            return {"input_ids": [[0] * min(2 * (t.count(" ") + 1) + 2, max_length) for t in texts]}
    texts = [" ".join(["w"] * n) for n in rs.randint(1, 60, 3000)]
    w = token_weights(texts, 64, tokenizer=Pieces())
    want = np.minimum(2.0 * np.array([t.count(" ") + 1 for t in texts]) + 2, 64)
    assert np.abs(w - want).max() < 1e-6


def test_short_lists_are_suspended_after_an_exchange_that_repeats_too_many_queries(monkeypatch):
    """The k / R + 6 sigma budget assumes exchangeable rows; an exchange that had to repeat more than 5 % of its queries with full lists
    (a corpus in topical order) suspends the shortcut for that (k, world): later exchanges send full lists.  Explicit short_lists=True and
    CCREC_SHORT_LISTS=1 still force it; resume_short_lists() forgets."""
    from ccrec_amd import dist as cdist
    monkeypatch.delenv("CCREC_SHORT_LISTS", raising=False)
    cdist.resume_short_lists()
    assert cdist.exchange_list_length(1001, 8) == 196 and cdist.exchange_list_length(1001, 8, blocked=True) == 1001
    cdist.note_short_list_outcome(1001, 8, 3452, 100)            # 2.9 %: fine
    assert cdist.short_lists_pay(1001, 8) and cdist.short_lists_suspended(1001, 8) is None
    cdist.note_short_list_outcome(1001, 8, 3452, 400)            # 11.6 %
    assert not cdist.short_lists_pay(1001, 8) and cdist.short_lists_suspended(1001, 8) == {"queries": 3452, "repeated": 400}
    assert cdist.exchange_list_length(1001, 8) == 1001 and cdist.exchange_list_length(1001, 8, short_lists=True) == 196
    assert cdist.short_lists_pay(1001, 4)                         # another world size is another budget
    monkeypatch.setenv("CCREC_SHORT_LISTS", "1")
    assert cdist.short_lists_pay(1001, 8)
    monkeypatch.delenv("CCREC_SHORT_LISTS")
    cdist.resume_short_lists()
    assert cdist.short_lists_pay(1001, 8)


def test_round_robin_negatives():
    from ccrec_amd.bbpr_loss import pick_round_robin_negatives
    table = {0: [5, 6, 7], 1: [9]}
    assert pick_round_robin_negatives(table, [0, 1, 0, 0, 0]) == [5, 9, 6, 7, 5]
    assert table == {0: [6, 7, 5], 1: [9]}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n, nq, k, out_dir):
    import torch.distributed as dist
    sys.path[:0] = [ROOT, PKG]
    from ccrec_amd.dist import shard_bounds, sharded_search
    from oracle import oracle as orc
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(3)
    Db = orc.pack_bf16((torch.randn(n, 64, generator=g) / 8).numpy())
    Qb = orc.pack_bf16((torch.randn(nq, 64, generator=g) / 8).numpy())
    Db[n // 2 + 1] = Db[1]          # cross-shard exact tie: the lower global id must win
    lo, hi = shard_bounds(n, world, rank)

    class Shard:  # CPU stand-in for a CorpusIndex: the oracle scores the local rows
        n_rows = hi - lo
        offset = lo

    def search_fn(q, kk):
        ids, sc = orc.canonical_search(Qb, Db[lo:hi], kk)
        return torch.from_numpy(sc), torch.from_numpy(ids + lo)

    def merge_fn(gs, gi):
        s, i = orc.merge_topk(gs.numpy(), gi.numpy())
        return torch.from_numpy(s), torch.from_numpy(i)

    if n >= k:
        # (short_lists=False: the FULL-list protocol -- at world 8 the automatic choice would be short lists, which have their own test)
        s, i = sharded_search(Shard(), None, k, merge_fn=merge_fn, search_fn=search_fn, short_lists=False)
        ref_i, ref_s = orc.canonical_search(Qb, Db, k)
        ok = np.array_equal(i.numpy(), ref_i) and np.array_equal(s.numpy(), ref_s)
    else:
        # the whole corpus holds fewer than k rows: n_total clamps k; without it the tail is (-inf, distinct pad ids) --
        # every output slot written, never uninitialised memory
        ref_i, ref_s = orc.canonical_search(Qb, Db, n)
        s, i = sharded_search(Shard(), None, k, merge_fn=merge_fn, search_fn=search_fn, n_total=n, short_lists=False)
        ok = tuple(i.shape) == (nq, n) and np.array_equal(i.numpy(), ref_i) and np.array_equal(s.numpy(), ref_s)
        s, i = sharded_search(Shard(), None, k, merge_fn=merge_fn, search_fn=search_fn, short_lists=False)
        ok = ok and tuple(i.shape) == (nq, k) and np.array_equal(i.numpy()[:, :n], ref_i) and np.array_equal(s.numpy()[:, :n], ref_s)
        tail_i, tail_s = i.numpy()[:, n:], s.numpy()[:, n:]
        ok = ok and bool(np.isneginf(tail_s).all()) and bool((tail_i > 2 ** 62).all())
        ok = ok and all(len(set(r.tolist())) == k - n for r in tail_i)
    open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write("ok" if ok else "MISMATCH")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("n,k", [(1000, 50), (9, 8), (5, 8)])   # a shard smaller than k (padding path); a CORPUS smaller than k
def test_sharded_search_gloo_world2(tmp_path, n, k):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_worker, args=(2, port, n, 6, k, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        assert open(tmp_path / f"rank{r}.txt").read() == "ok"


@pytest.mark.parametrize("n,k", [(1600, 100), (30, 8)])   # world 8: the target world size; 30 rows: shards of 3-4 rows < k
def test_sharded_search_gloo_world8(tmp_path, n, k):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_worker, args=(8, port, n, 6, k, str(tmp_path)), nprocs=8, join=True)
    for r in range(8):
        assert open(tmp_path / f"rank{r}.txt").read() == "ok"


def _short_worker(rank, world, port, n, nq, k, skew, out_dir):
    """Short-list exchange over gloo with CPU stand-ins (the oracle scores the local rows; numpy merges): every rank searches and
    sends only short_list_length(k, world) entries per query; the merge verifies the cuts and the flagged queries are repeated with
    full lists by all ranks together."""
    import torch.distributed as dist
    sys.path[:0] = [ROOT, PKG]
    from ccrec_amd import dist as cdist
    from oracle import oracle as orc
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(11)
    D = torch.randn(n, 64, generator=g) / 8
    Q = torch.linalg.qr(torch.randn(64, nq, generator=g))[0].T.contiguous()      # orthonormal query rows: a row built for one query is noise for the others
    if skew:   # queries 0 and 3 find their whole top-k inside the LAST shard: its short list is consumed to its end
        lo_last = cdist.shard_bounds(n, world, world - 1)[0]
        for j, qi in enumerate((0, 3)):
            rows = slice(lo_last + 5 + j * k, lo_last + 5 + (j + 1) * k)
            D[rows] = 3.0 * Q[qi] + 0.2 * D[rows]
    Db, Qb = orc.pack_bf16(D.numpy()), orc.pack_bf16(Q.numpy())
    Db[n // 2 + 1] = Db[1]          # cross-shard exact tie
    lo, hi = cdist.shard_bounds(n, world, rank)
    calls = []

    class Shard:
        n_rows = hi - lo
        offset = lo

    def search_fn(q, kk):
        rows = np.arange(nq) if q is None else q.numpy().astype(np.int64)     # the fallback hands over the flagged queries' rows
        calls.append((len(rows), kk))
        ids, sc = orc.canonical_search(Qb[rows], Db[lo:hi], kk)
        return torch.from_numpy(sc), torch.from_numpy(ids + lo)

    def merge_fn(gs, gi):
        s, i = orc.merge_topk(gs.numpy(), gi.numpy())
        return torch.from_numpy(s), torch.from_numpy(i)

    def short_merge_fn(gs, gi, truncated, k_out):
        s, i, flags = orc.merge_short_lists(gs.numpy(), gi.numpy(), truncated, k_out)
        return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(flags), torch.tensor([int(flags.sum())])

    k_list = cdist.short_list_length(k, world)
    ok = k_list < k
    # queries as a tensor of their own row numbers, so that the fallback's `queries[which]` names the flagged rows for search_fn
    qrows = torch.arange(nq)
    index = Shard()
    msg = cdist.ShardMessage(nq, k_list, "cpu", world)
    scores, ids = search_fn(qrows, k_list)
    msg.fill(scores, ids, lo, hi - lo)
    ex = cdist.ShardExchange(msg, index, None, merge_fn, k_out=k, queries=qrows, search_fn=search_fn, short_merge_fn=short_merge_fn).submit()
    s, i = ex.result()
    ref_i, ref_s = orc.canonical_search(Qb, Db, k)
    ok = ok and np.array_equal(i.numpy(), ref_i) and np.array_equal(s.numpy().view(np.uint32), ref_s.view(np.uint32))
    if skew:
        ok = ok and ex.fallback_queries == 2 and calls == [(nq, k_list), (2, k)]      # exactly the two skewed queries were repeated, with full lists
        # 2 of 7 queries repeated: every rank has suspended the shortcut for this (k, world); the next automatic exchange sends full lists
        ok = ok and cdist.short_lists_suspended(k, world) == {"queries": nq, "repeated": 2}
        calls.clear()
        s4, i4 = cdist.sharded_search(index, qrows, k, merge_fn=merge_fn, search_fn=search_fn, short_merge_fn=short_merge_fn)
        ok = ok and np.array_equal(i4.numpy(), ref_i) and calls == [(nq, k)]
    else:
        ok = ok and ex.fallback_queries == 0 and calls == [(nq, k_list)] and cdist.short_lists_suspended(k, world) is None
    # the same through sharded_search's own routing (short_lists=True), and switched off
    calls.clear()
    s2, i2 = cdist.sharded_search(index, qrows, k, merge_fn=merge_fn, search_fn=search_fn, short_lists=True, short_merge_fn=short_merge_fn)
    ok = ok and np.array_equal(i2.numpy(), ref_i) and calls[0] == (nq, k_list)
    calls.clear()
    s3, i3 = cdist.sharded_search(index, qrows, k, merge_fn=merge_fn, search_fn=search_fn, short_lists=False)
    ok = ok and np.array_equal(i3.numpy(), ref_i) and calls == [(nq, k)]
    open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write("ok" if ok else f"MISMATCH fallback={ex.fallback_queries} calls={calls}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,skew", [(2, False), (3, False), (2, True), (3, True)])
def test_short_list_exchange_gloo(tmp_path, world, skew):
    """Short-list exchange (ccrec_amd/dist.py): world 2 / 3 over gloo, k = 300 -> 210 / 157 entries per rank and query; iid rows need no
    repeat; with two queries whose top-k sits in one shard exactly those two are repeated with full lists -- the merged lists equal
    the single-index oracle search bit for bit either way (a cross-shard exact tie included)."""
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_short_worker, args=(world, port, 2400, 7, 300, skew, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        assert open(tmp_path / f"rank{r}.txt").read() == "ok"


@pytest.mark.parametrize("k,n,skew", [(1001, 16800, False), (1001, 16800, True), (100, 2400, False), (100, 2400, True)])
def test_short_list_exchange_gloo_world8(tmp_path, k, n, skew):
    """The same exchange at the TARGET world size, eight ranks over gloo: ranking()'s k = 1001 -> k_list = 196 entries per rank and query,
    k = 100 -> 41; eight headers parsed on every rank; with two queries whose whole top-k sits in the last shard exactly those two
    are repeated with full lists (a matched second collective on eight ranks) and the shortcut is suspended afterwards."""
    import torch.multiprocessing as mp
    from ccrec_amd.dist import short_list_length
    assert short_list_length(k, 8) == (196 if k == 1001 else 41)
    port = _free_port()
    mp.spawn(_short_worker, args=(8, port, n, 7, k, skew, str(tmp_path)), nprocs=8, join=True)
    for r in range(8):
        assert open(tmp_path / f"rank{r}.txt").read() == "ok"


def test_short_list_length_and_policy(monkeypatch):
    from ccrec_amd import dist as cdist
    monkeypatch.delenv("CCREC_SHORT_LISTS", raising=False)
    assert cdist.short_list_length(1001, 1) == 1001
    assert cdist.short_list_length(1001, 8) == 196 and cdist.short_list_length(1001, 2) == 604 and cdist.short_list_length(100, 8) == 41
    assert cdist.short_list_length(10, 8) == 10                       # never above k
    for k in (1, 10, 100, 1001, 4096):
        for world in (2, 3, 8, 64):
            assert world * cdist.short_list_length(k, world) >= k      # the R lists can always fill k ranks
    assert cdist.short_lists_pay(1001, 8) and cdist.short_lists_pay(1001, 2) and cdist.short_lists_pay(100, 8)
    assert not cdist.short_lists_pay(100, 2) and not cdist.short_lists_pay(1001, 1) and not cdist.short_lists_pay(10, 8)
    assert cdist.short_lists_pay(4096, 64) and cdist.short_lists_pay(4096, 3)
    monkeypatch.setattr(cdist.ops, "SHORT_LIST_LDS_BYTES", 32 * 1024)
    assert not cdist.short_lists_pay(4096, 3) and cdist.short_lists_pay(1001, 8)       # 3 x 1 555 x 12 B of lists would not fit the merge kernel's LDS
    monkeypatch.undo()
    monkeypatch.delenv("CCREC_SHORT_LISTS", raising=False)
    monkeypatch.setenv("CCREC_SHORT_LISTS", "0")
    assert not cdist.short_lists_pay(1001, 8)
    monkeypatch.setenv("CCREC_SHORT_LISTS", "1")
    assert cdist.short_lists_pay(100, 2) and not cdist.short_lists_pay(1001, 1)


def test_plan_batches_covers_every_text_once_under_the_budget():
    """Host logic of the length-sorted encoder."""
    from ccrec_amd.encode import plan_batches
    rs = np.random.RandomState(0)
    lengths = rs.randint(1, 200, 5000)
    batches = plan_batches(lengths, max_tokens=4096, max_batch=64, pad_multiple=8)
    seen = np.concatenate([idx for idx, _ in batches])
    assert np.array_equal(np.sort(seen), np.arange(5000))
    prev = 0
    for idx, padded in batches:
        assert 1 <= len(idx) <= 64 and padded % 8 == 0 and padded >= lengths[idx].max() > padded - 8
        assert len(idx) * padded <= 4096 or len(idx) == 1
        assert lengths[idx].min() >= prev          # ascending across batches
        prev = lengths[idx].max()
    padded_total = sum(len(i) * p for i, p in batches)
    assert padded_total < 1.1 * lengths.sum() + 8 * 5000 and padded_total < 0.6 * 5000 * 200
    assert plan_batches([], 4096) == [] and plan_batches([9000], 4096)[0][1] == 9000


def test_shard_message_layout_on_cpu():
    """The packed exchange message {32-byte header | fp32 scores | u32 local rows} (include/ccr_retrieval.h): the views alias
    one byte buffer, blocks are 16-byte aligned, the size matches ccr_shard_message_bytes, padding slots decode to
    (-inf, distinct ids above every real id)."""
    from ccrec_amd import _lib, ops
    from ccrec_amd.dist import ShardMessage, PAD_ID
    m = ShardMessage(7, 5, "cpu", 3)           # 7 * 5 * 4 = 140 bytes of scores after the 32-byte header: rows start at 176
    assert m.rows_at == 176 and m.nbytes == 176 + 140 + 4 and m.nbytes % 16 == 0 == m.rows_at % 16
    assert m.nbytes == ops.shard_message_bytes(7, 5) and ctypes.sizeof(_lib.ShardHeader) == _lib.SHARD_HEADER_BYTES == 32
    sc = torch.arange(21, dtype=torch.float32).view(7, 3)
    ids = torch.arange(21).view(7, 3) + (1 << 40) + (1 << 31)       # local rows at and above 2^31: u32, not i32
    m.fill(sc, ids, row_offset=1 << 40, n_rows=1 << 32)            # k_valid = 3 of k = 5
    h = ShardMessage.parse_headers(m.header.view(1, 8))[0]
    assert h == {"magic": _lib.SHARD_MAGIC, "n_flagged": 0, "k_valid": 3, "n_covered": 0, "row_offset": 1 << 40, "n_rows": 1 << 32}
    assert m.send[32:172].view(torch.float32).view(7, 5)[:, :3].equal(sc) and m.send[172:176].eq(0).all()
    for r in range(3):
        m.recv.view(3, -1)[r].copy_(m.send)
    gs, gi = m.decoded()
    assert gs.shape == (3, 7, 5) and gi.shape == (3, 7, 5)
    for r in range(3):
        assert gi[r, :, :3].equal(ids) and gs[r, :, :3].equal(sc) and bool(torch.isinf(gs[r, :, 3:]).all())
        assert gi[r, 0, 3] == PAD_ID - (r * 5 + 3) and gi[r, 6, 4] == PAD_ID - (r * 5 + 4)
    assert len(set(gi[:, 0, 3:].flatten().tolist())) == 6


def _flag_worker(rank, world, port, out_dir):
    """The asynchronous exchange when exactly ONE rank's lists are not final at the first all-gather: its header says so, every
    rank reads every header, every rank repeats the collective (a matched second all-gather), the merged lists are exact."""
    import torch.distributed as dist
    sys.path[:0] = [ROOT, PKG]
    from ccrec_amd.dist import shard_bounds, submit_sharded_search, ShardMessage
    from ccrec_amd import _lib
    from oracle import oracle as orc
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    n, nq, k = 900, 40, 30
    g = torch.Generator().manual_seed(5)
    Db = orc.pack_bf16((torch.randn(n, 64, generator=g) / 8).numpy())
    Qb = orc.pack_bf16((torch.randn(nq, 64, generator=g) / 8).numpy())
    lo, hi = shard_bounds(n, world, rank)
    ids, sc = orc.canonical_search(Qb, Db[lo:hi], k)
    flagged_rank = world - 1

    class FakeIndex:   # CPU stand-in for CorpusIndex.search_shard(defer=True) / finish()
        n_rows, offset, _deferred, finished = hi - lo, lo, None, 0

        def search_shard(self, q, kk, send, defer=False):
            msg = self.msg
            msg.fill(torch.from_numpy(sc), torch.from_numpy(ids + lo), lo, hi - lo)
            if rank == flagged_rank:           # 20 queries flagged, 16 covered on the stream: rows of 4 queries are not final yet
                msg.scores[:4] = 0.0
                msg.rows[:4] = 0
                msg.header[1], msg.header[3] = 20, 16
            else:
                msg.header[3] = 16
            self._deferred = (q, send)

        def finish(self):
            self.finished += 1
            self._deferred = None
            if rank == flagged_rank:
                self.msg.scores[:4] = torch.from_numpy(sc[:4])
                self.msg.rows[:4] = torch.from_numpy(ids[:4].astype(np.int32))

    def merge_fn(gs, gi):
        s, i = orc.merge_topk(gs.numpy(), gi.numpy())
        return torch.from_numpy(s), torch.from_numpy(i)

    ok = True
    for flag_it in (True, False):
        ix = FakeIndex()
        ix.msg = ShardMessage(nq, k, "cpu", world)
        if not flag_it:
            flagged_rank = -1
        ex = submit_sharded_search(ix, torch.zeros(nq, 64), k, message=ix.msg, merge_fn=merge_fn)
        s, i = ex.result()
        ref_i, ref_s = orc.canonical_search(Qb, Db, k)
        ok = ok and np.array_equal(i.numpy(), ref_i) and np.array_equal(s.numpy(), ref_s)
        ok = ok and ex.repeated == flag_it and ix.finished == 1
        ok = ok and [h["n_flagged"] for h in ex.headers] == [20 if (flag_it and r == world - 1) else 0 for r in range(world)]
    open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write("ok" if ok else "MISMATCH")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_exchange_repeats_on_every_rank_when_one_rank_flags(tmp_path, world):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_flag_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        assert open(tmp_path / f"rank{r}.txt").read() == "ok"

def _cuts_worker(rank, world, port, out_dir):
    """Every rank computes its OWN cuts from weights that differ by one part in 1e9 on rank 1 (another BLAS behind the polyfit, a
    caller's array): the local cuts disagree, agreed_cuts() hands every rank rank 0's."""
    import json
    import torch.distributed as dist
    sys.path[:0] = [ROOT, PKG]
    from ccrec_amd.dist import agreed_cuts, largest_share, weighted_cuts
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    w = np.ones(10)
    if rank == 1:
        w[0] += 1e-9                    # cum[4] now exceeds half the total: the local boundary moves from 5 to 4
    local = weighted_cuts(w, world)
    cuts = agreed_cuts(10, world, w)
    rows = agreed_cuts(11, world)       # no weights: equal row counts, still one answer for all
    json.dump({"local": local, "agreed": cuts, "rows": rows, "share": largest_share(cuts)}, open(os.path.join(out_dir, f"rank{rank}.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()


def test_shard_cuts_are_agreed_on_not_computed_per_rank(tmp_path):
    """Round-5 advisor (medium): token-balanced cuts come from a float cumsum + searchsorted over weights every rank computes for
    itself; a one-ulp difference moves a boundary on one rank only (rows dropped or encoded twice under wrong row offsets).
    agreed_cuts(): rank 0's boundaries, broadcast as int64, validated on every rank."""
    import json
    import torch.multiprocessing as mp
    mp.spawn(_cuts_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (json.load(open(tmp_path / f"rank{r}.json")) for r in range(2))
    assert r0["local"] == [0, 5, 10] and r1["local"] == [0, 4, 10]          # the hazard is real: the ranks' own cuts differ
    assert r0["agreed"] == r1["agreed"] == [0, 5, 10] and r0["rows"] == r1["rows"] == [0, 6, 11]
    assert r0["share"] == 0.5
    # unequal shards size the short lists from the largest row share (advisor, low): 8 ranks, one holding 30 % of the rows
    from ccrec_amd import dist as cdist
    assert cdist.short_list_length(1001, 8) == 196 and cdist.short_list_length(1001, 8, share=0.30) == 396
    assert cdist.short_list_length(1001, 8, share=0.01) == 196              # never below the equal-shard budget
    assert cdist.exchange_list_length(1001, 8, share=0.30) == 396 and cdist.exchange_list_length(1001, 8, share=0.9) == 1001
    assert cdist.largest_share([0, 3, 4, 10]) == 0.6


def _bench_worker(rank, world, port, data, out_dir):
    """bench.Workload -- the pipelined step loop, set_k, the exchange record -- on eight gloo ranks with the oracle-backed stand-ins
    of tests/cpu_stand_ins.py in place of the device ops (no GPU here; the product has no CPU path: this rehearses CONTROL FLOW)."""
    import json
    import torch.distributed as dist
    sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tests")]
    import cpu_stand_ins
    index_cls = cpu_stand_ins.install()
    import bench
    from ccrec_amd import dist as cdist
    from oracle import oracle as orc
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    rows, queries, dim = 8 * 1100, 24, 64
    if data == "skewed":
        # three of the 24 queries find 300 strongly aligned rows inside the LAST shard (a corpus in topical order): that shard's short
        # list is consumed to its end for them (k_list 41 / 196), 3 / 24 > 5 % of the queries -> the shortcut is suspended
        iid = bench.gen_rows

        def gen_rows(n, d, seed, device, data_="gaussian", chunk=262144, lo=0, hi=None):
            x = iid(n, d, seed, device, "gaussian")
            if seed == 1234:
                q = iid(queries, d, 4321, device, "gaussian")
                for j, qi in enumerate((0, 7, 13)):
                    blk = slice(n - 1000 + 300 * j, n - 1000 + 300 * (j + 1))
                    x[blk] = 3.0 * q[qi] + 0.2 * x[blk]
            return x[lo:n if hi is None else hi].clone()
        bench.gen_rows = gen_rows
        data = "gaussian"
        skewed = True
    else:
        skewed = False
    full = orc.pack_bf16(bench.gen_rows(rows, dim, 1234, "cpu", data).numpy())
    qb = orc.pack_bf16(bench.gen_rows(queries, dim, 4321, "cpu", data).numpy())
    rec = {}
    w = bench.Workload(rows, queries, dim, 100, data, "cpu", rank, world, "gloo")
    for k in (100, 1001):
        if k != w.k:
            w.set_k(k)
        k_list0 = w.k_list
        r = w.run(3, 1, f"k{k}")
        ref_i, ref_s = orc.canonical_search(qb, full, k)
        ex = bench.exchange_obj(w, r)
        rec[str(k)] = {"ids_equal": bool(np.array_equal(w.ids.numpy(), ref_i)),
                       "scores_equal": bool(np.array_equal(w.scores.numpy().view(np.uint32), ref_s.view(np.uint32))),
                       "k_list_first": k_list0, "k_list_last": w.k_list, "entries": ex["entries_per_query_per_rank"], "n_ranks_seen": ex["n_ranks_seen"],
                       "repeated_queries": ex["queries_repeated_with_full_lists"], "suspended_at": ex["short_lists_suspended_at_step"],
                       "message_bytes": ex["message_bytes_per_rank"], "searches": list(index_cls.calls)}
        index_cls.calls.clear()
    json.dump(rec, open(os.path.join(out_dir, f"rank{rank}.json"), "w"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("data", ["gaussian", "skewed"])
def test_bench_step_loop_rehearsal_world8_gloo(tmp_path, data):
    """`bench.py --gpus 8`'s step loop at world 8: eight gloo processes, a CPU-sized corpus (8,800 x 64, 24 queries),
    top-100 (k_list 41) and top-1001 (k_list 196).  Every rank ends with the single-index oracle lists; iid rows never repeat a
    query; a corpus in topical order (--data sorted) repeats queries with full lists and every rank suspends the shortcut at the
    same step (the k_list of the last step is then k itself; "skewed": three queries with 300 aligned rows inside the last shard)."""
    import json
    import torch.multiprocessing as mp
    mp.spawn(_bench_worker, args=(8, _free_port(), data, str(tmp_path)), nprocs=8, join=True)
    recs = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(8)]
    for k, kl in (("100", 41), ("1001", 196)):
        for r in recs:
            assert r[k]["ids_equal"] and r[k]["scores_equal"] and r[k]["n_ranks_seen"] == 8 and r[k]["k_list_first"] == kl
        assert len({(r[k]["k_list_last"], r[k]["suspended_at"], r[k]["repeated_queries"]) for r in recs}) == 1   # every rank took the same branches
        if data == "gaussian":
            assert recs[0][k]["repeated_queries"] == 0 and recs[0][k]["suspended_at"] is None and recs[0][k]["k_list_last"] == kl
            assert all(c == [24, kl] for c in recs[0][k]["searches"])
        if data == "skewed":   # the warm-up step repeats the three skewed queries with full lists; every rank then switches to full lists
            assert recs[0][k]["suspended_at"] is not None and recs[0][k]["k_list_last"] == int(k)
            assert [24, kl] in recs[0][k]["searches"] or recs[0][k]["searches"][-1] == [24, int(k)]


def test_committed_bench_line_has_the_contract_fields():
    """The NEWEST default bench line committed under profiles/ (a real MI355X run of `python bench.py` when it measured everything that
    `--full` measures now: profiles/rNN_bench<i>.json) carries every field the driver reads."""
    import glob
    import json
    import re
    runs = [(tuple(int(v) for v in re.findall(r"r(\d+)_bench(\d+)\.json$", f)[0]), f)
            for f in glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench[0-9].json"))]
    assert runs, "no committed default bench line"
    path = max(runs)[1]
    line = json.loads(open(path).read().strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["n_gpus"] == 1 and line["higher_is_better"] is True and line["vs_baseline"] is None
    assert "workload" in line["config"] and "model" not in line["config"]
    roof = line["roofline"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(roof)
    assert roof["bound"] in ("hbm", "mfma") and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    cpu = line["cpu_baseline"]
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(cpu) and cpu["kind"] in ("port", "reference")
    assert abs(line["value"] - line["config"]["queries"] / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3


def test_bench_dump_outputs_keeps_values_exact_and_samples_past_the_limit(tmp_path):
    """bench.py --dump-outputs (its file writer, no GPU): fp32 scores stay fp32 and int64 ids become exact fp64; past the byte limit every
    array keeps the SAME seeded sample of query rows (rows.npy names them, ascending), whatever the values -- two builds dump alike."""
    import bench
    rs = np.random.RandomState(5)
    scores = rs.standard_normal((1000, 100)).astype(np.float32)
    ids = rs.randint(0, 2 ** 40, (1000, 100)).astype(np.int64)
    assert bench.dump_outputs(str(tmp_path / "all"), {"scores": scores, "ids": ids}) == ["ids", "scores"]
    s, i = np.load(tmp_path / "all" / "scores.npy"), np.load(tmp_path / "all" / "ids.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64
    assert np.array_equal(s.view(np.uint32), scores.view(np.uint32)) and np.array_equal(i.astype(np.int64), ids)
    limit, picked = 300_000, []
    for tag in ("a", "b"):
        sc = np.random.RandomState(len(picked)).standard_normal((1000, 100)).astype(np.float32)
        assert bench.dump_outputs(str(tmp_path / tag), {"scores": sc, "ids": ids}, limit=limit) == ["ids", "rows", "scores"]
        files = [tmp_path / tag / f"{n}.npy" for n in ("ids", "rows", "scores")]
        assert sum(os.path.getsize(f) for f in files) <= limit
        rows = np.load(files[1])
        assert rows.dtype == np.float64 and 0 < len(rows) < 1000 and np.all(np.diff(rows) > 0)
        r = rows.astype(np.int64)
        assert np.array_equal(np.load(files[2]), sc[r]) and np.array_equal(np.load(files[0]).astype(np.int64), ids[r])
        picked.append(rows)
    assert np.array_equal(picked[0], picked[1])


def test_bench_full_is_off_by_default_and_side_run_rehearsals_imply_it():
    """bench.py's extra measurements and checks run only with --full; --rehearse-secondary, which only sizes side runs, turns it on."""
    import bench
    assert bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full is False
    assert bench.parse(["--full"]).full is True
    assert bench.parse(["--rehearse-secondary", "40"]).full is True



def test_replica_cache_replicate_returns_cached_copies_for_a_device_subset(monkeypatch):
    """src/ccrec/util/data_parallel.py:8-20: after cache_replicas(), torch's DataParallel.forward asks replicate() for the
    devices that received a chunk and must get the STORED copies (no new broadcast).  No GPU here: the broadcast, scatter,
    parallel_apply and gather are faked, torch's own forward() and our replicate() are the code under test."""
    import copy
    import torch
    from ccrec_amd import replica_cache

    broadcasts = []

    def fake_broadcast(module, device_ids, detach=False):
        broadcasts.append((list(device_ids), detach))
        out = []
        for d in device_ids:
            m = copy.deepcopy(module)
            m.tag = d
            out.append(m)
        return out

    monkeypatch.setattr(replica_cache, "_broadcast_module", fake_broadcast)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(4, 3)
            self.tag = "source"
            self.calls = 0

        def forward(self, x):
            self.calls += 1
            return self.lin(x)

    dp = replica_cache.DataParallel(Net())     # CPU host: torch leaves device_ids empty
    assert dp.cache_replicas() is dp and broadcasts == []            # nothing to copy without devices
    dp.device_ids, dp.output_device, dp.src_device_obj = [0, 1, 2], 0, torch.device("cpu")
    assert dp.cache_replicas() is dp
    assert broadcasts == [([0, 1, 2], True)]                          # one detached broadcast
    copies = dp._by_device
    assert [copies[d].tag for d in (0, 1, 2)] == [0, 1, 2]
    # a device subset, in any order, returns the stored objects themselves
    assert [m.tag for m in dp.replicate(dp.module, [0, 2])] == [0, 2]
    assert dp.replicate(dp.module, [2, 1])[0] is copies[2]
    # torch's DataParallel.forward: a batch of 5 rows split over two of the three devices -> replicate(module, [0, 1])
    dp.scatter = lambda inputs, kwargs, device_ids: (((inputs[0][:3],), (inputs[0][3:],)), ({}, {}))
    dp.parallel_apply = lambda replicas, inputs, kwargs: [m(*i, **k) for m, i, k in zip(replicas, inputs, kwargs)]
    dp.gather = lambda outputs, output_device: torch.cat(outputs, 0)
    x = torch.randn(5, 4)
    y = dp(x)
    assert torch.allclose(y, dp.module.lin(x))
    assert (copies[0].calls, copies[1].calls, copies[2].calls, dp.module.calls) == (1, 1, 0, 0)
    assert broadcasts == [([0, 1, 2], True)]                          # forward did not broadcast again
    # without the cache the class behaves like torch's (replicate goes to the broadcast)
    fresh = replica_cache.DataParallel(Net())
    fresh.device_ids = [0, 1]
    monkeypatch.setattr(torch.nn.DataParallel, "replicate", lambda self, module, device_ids: ["torch", list(device_ids)])
    assert fresh.replicate(fresh.module, [0, 1]) == ["torch", [0, 1]]


def test_unwrap_item_tower_shapes():
    """al_0_rank.py:84-90: BertBPR/BertMT-style wrappers, bare Lightning modules and plain towers."""
    from ccrec_amd.al_rank import unwrap_item_tower

    class T:
        pass

    tower = T()
    with_attr, wrapper = T(), T()
    with_attr.item_tower = tower
    wrapper.model = with_attr
    assert unwrap_item_tower(with_attr) is tower and unwrap_item_tower(wrapper) is tower and unwrap_item_tower(tower) is tower


def test_a_hung_child_fails_with_stacks_and_kernel_state(tmp_path):
    """The harness the GPU rehearsal tests run bench.py children under (helpers.run_child_with_evidence): a child that is still
    running at the limit is a FAILURE that carries every thread's Python stack (SIGUSR1 -> the faulthandler bench.install_watchdog
    registers, written to a file that survives the kill), the kernel-side state / wait channel of its threads and its stderr --
    and the whole process group is gone afterwards.  (Round 2 turned such a timeout into a skip and kept no record.)"""
    from helpers import run_child_with_evidence
    code = ("import sys, time; sys.path.insert(0, %r); import bench; bench.install_watchdog(); "
            "print('child: waiting forever', file=sys.stderr, flush=True)\n"
            "def stuck_here():\n    time.sleep(1000)\n"
            "stuck_here()") % ROOT
    env = dict(os.environ, CCR_BENCH_WATCHDOG="900")
    with pytest.raises(pytest.fail.Exception) as info:
        run_child_with_evidence([sys.executable, "-c", code], env, tmp_path, "hung", limit=20)
    msg = str(info.value)
    assert "child still running after" in msg and "stuck_here" in msg
    assert "State:" in msg and "wchan=" in msg and "child: waiting forever" in msg and "stacks.rank0.txt" in msg
    pids = [int(m) for m in re.findall(r"^pid (\d+):", msg, flags=re.M)]
    assert pids and not any(os.path.exists(f"/proc/{p}") for p in pids), pids       # the whole group was killed and reaped
    # a child that exits non-zero (the in-child watchdog's exit path) is a failure with its stderr as well
    with pytest.raises(pytest.fail.Exception, match="exit code 3"):
        run_child_with_evidence([sys.executable, "-c", "import sys; print('boom', file=sys.stderr); sys.exit(3)"], env, tmp_path, "bad", limit=20)


def test_kernel_forward_policy_and_coverage_checks_run_without_a_gpu(monkeypatch):
    """Host logic of ccrec_amd/fused_bert.py: which encoders the layer kernels cover, and when an inference forward may take them
    (explicit flag > CCREC_FUSED_ENCODER > "inside a CUDA autocast context" -- never on a machine without a GPU by default)."""
    import torch
    from transformers import BertConfig, BertModel
    from ccrec_amd import fused_bert

    def bert(hidden, heads, act="gelu"):
        return BertModel(BertConfig(vocab_size=50, hidden_size=hidden, num_hidden_layers=1, num_attention_heads=heads,
                                    intermediate_size=2 * hidden, max_position_embeddings=32, hidden_act=act))

    assert fused_bert.unsupported_reason(bert(256, 4)) is None
    assert "head width" in fused_bert.unsupported_reason(bert(256, 8))
    assert "hidden size" in fused_bert.unsupported_reason(bert(192, 3))
    assert "activation" in fused_bert.unsupported_reason(bert(256, 4, "relu"))
    assert "not a BertModel" in fused_bert.unsupported_reason(torch.nn.Linear(4, 4))
    from transformers import DistilBertConfig, DistilBertModel
    assert fused_bert.unsupported_reason(DistilBertModel(DistilBertConfig(vocab_size=50, dim=256, n_layers=1, n_heads=4, hidden_dim=512))) is None
    assert "head width" in fused_bert.unsupported_reason(DistilBertModel(DistilBertConfig(vocab_size=50, dim=256, n_layers=1, n_heads=2, hidden_dim=512)))
    monkeypatch.delenv("CCREC_FUSED_ENCODER", raising=False)
    assert fused_bert.wanted(True) is True and fused_bert.wanted(False) is False
    assert fused_bert.wanted("auto") is False                       # no GPU here: never by default
    monkeypatch.setenv("CCREC_FUSED_ENCODER", "1")
    assert fused_bert.wanted("auto") is True and fused_bert.wanted(False) is False
    monkeypatch.setenv("CCREC_FUSED_ENCODER", "0")
    assert fused_bert.wanted("auto") is False
    # the encoder object itself refuses to run without the HIP library (no CPU fallback)
    model = bert(256, 4).eval()
    enc = fused_bert.for_model(model)
    assert enc is not None and fused_bert.for_model(model) is enc and fused_bert.for_model(bert(256, 8)) is None
    from ccrec_amd import _lib
    with pytest.raises((_lib.CcrError, AssertionError)):
        enc.forward(torch.zeros(1, 4, dtype=torch.long), torch.ones(1, dtype=torch.int32))
