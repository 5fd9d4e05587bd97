"""Host side of the pool contrastive loss, without a GPU: the round-robin picking of several negatives per user, and the
cross-rank protocol of dist.gathered_pool_ce rehearsed over gloo with a torch fp64 stand-in for the device loss."""
import copy
import os
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "crowd-coachable-recommendations_amd")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---------------------------------------------------------------------------------------------- round robin
def test_round_robin_takes_m_successive_pops_per_user():
    from ccrec_amd.bbpr_loss import pick_round_robin_negatives
    lists = {0: [10], 1: [20, 21], 2: [30, 31, 32, 33, 34]}
    users = torch.tensor([0, 1, 2])
    got = pick_round_robin_negatives(lists, users, n_negatives=3)
    # block k = every user's k-th pop; a list shorter than 3 cycles
    assert got == [10, 20, 30, 10, 21, 31, 10, 20, 32]
    # ... and the lists are left as three calls of bbpr.py:188-193 leave them
    ref = {0: [10], 1: [20, 21], 2: [30, 31, 32, 33, 34]}
    seq = []
    for _ in range(3):
        for u in users.tolist():
            neg = ref[u].pop(0)
            seq.append(neg)
            ref[u].append(neg)
    assert got == seq and lists == ref == {0: [10], 1: [21, 20], 2: [33, 34, 30, 31, 32]}
    # the next call goes on from there
    assert pick_round_robin_negatives(lists, users, n_negatives=3) == [10, 21, 33, 10, 20, 34, 10, 21, 30]


def test_round_robin_default_is_one_pop_and_a_user_twice_in_a_batch_pops_twice():
    from ccrec_amd.bbpr_loss import pick_round_robin_negatives
    lists = {0: [1, 2, 3], 1: [7]}
    before = copy.deepcopy(lists)
    assert pick_round_robin_negatives(lists, [0, 1, 0]) == [1, 7, 2]
    assert lists == {0: [3, 1, 2], 1: [7]} and before != lists
    assert pick_round_robin_negatives(lists, [0, 1, 0], n_negatives=2) == [3, 7, 1, 2, 7, 3]


def test_step_takes_the_new_keywords_and_keeps_its_defaults():
    from ccrec_amd.bbpr_loss import BertMTStep, MultipleNrlStep
    step = MultipleNrlStep(None, None, None, {})
    assert step.n_negatives == 1 and step.use_weights is False
    step = BertMTStep(None, None, None, {}, alpha=0.5, n_negatives=4, use_weights=True)
    assert step.n_negatives == 4 and step.use_weights is True and step.alpha == 0.5
    with pytest.raises(ValueError):
        MultipleNrlStep(None, None, None, {}, n_negatives=0)


def test_binding_refuses_a_library_older_than_it_was_written_for(monkeypatch):
    from ccrec_amd import _lib
    assert _lib.MIN_VERSION == 101
    lib = _lib.load()
    # a binding written for a newer library than the one in the tree: load() refuses it, with both versions in the text
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "MIN_VERSION", lib.ccr_version() + 1)
    with pytest.raises(_lib.CcrError, match=f"version {lib.ccr_version()}.*needs {lib.ccr_version() + 1}"):
        _lib.load()
    monkeypatch.undo()
    assert _lib.load() is lib
    assert lib.ccr_version() >= _lib.MIN_VERSION
    for name in ("ccr_pool_ce_workspace_bytes", "ccr_pool_ce_fwd", "ccr_pool_ce_fwd_f32", "ccr_pool_ce_bwd_dev"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    # sizes: supported shapes report a workspace, shapes beyond the range report 0 and a text (no device needed)
    assert lib.ccr_pool_ce_workspace_bytes(4096, 65536, 4096) > 4096 * 65536 * 4
    assert lib.ccr_pool_ce_workspace_bytes(1, 1, 8) > 0
    assert lib.ccr_pool_ce_workspace_bytes(8, (1 << 20) + 1, 64) == 0
    assert b"beyond the supported range" in lib.ccr_last_error()
    assert lib.ccr_pool_ce_workspace_bytes(8, 8, 12) == 0 and b"dim" in lib.ccr_last_error()


# ---------------------------------------------------------------------------------------------- cross-rank rehearsal
# Run as a child process per rank (this file is its own script): `python test_cpu_pool_ce.py rank world port case out_dir`.
def fp64_pool_ce(q, pool, labels, weights, inv_temperature):
    """torch fp64 stand-in for the device loss (the local_fn contract of dist.gathered_pool_ce)."""
    with torch.enable_grad():   # (it is called inside an autograd node's forward, where recording is off)
        qd = q.detach().double().requires_grad_(True)
        pd = pool.detach().double().requires_grad_(True)
        s = qd @ pd.T * inv_temperature
        ce = torch.logsumexp(s, dim=1) - s.gather(1, labels.long()[:, None])[:, 0]
        w = weights.double() if weights is not None else torch.ones_like(ce)
        num, den = (w * ce).sum(), w.sum()

    def backward(grad_out, W):
        dq, dp = torch.autograd.grad(num, (qd, pd))
        return dq * grad_out.double() / W.double(), dp * grad_out.double() / W.double()

    return num.detach(), den.detach(), backward


def _problem(world, n_q, n_c, dim, weighted):
    """The whole problem, the same on every rank: bf16-exact fp64 operands, labels local to each rank's block, weights with zeros."""
    g = torch.Generator().manual_seed(100 + world)
    Q = (torch.randn(world * n_q, dim, generator=g) / dim ** 0.5).to(torch.bfloat16).double()
    C = (torch.randn(world * n_c, dim, generator=g) / dim ** 0.5).to(torch.bfloat16).double()
    labels = torch.randint(0, n_c, (world * n_q,), generator=g)
    W = torch.rand(world * n_q, generator=g).double() + 0.1
    W[::5] = 0.0
    return Q, C, labels, (W if weighted else None)


def _rank_main(rank, world, port, case, out_dir):
    sys.path[:0] = [ROOT, PKG]
    import torch.distributed as dist
    from ccrec_amd.dist import gathered_pool_ce
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    n_q, n_c, dim, inv_t = 5, 11, 24, 20.0
    if case == "unequal":
        q = torch.zeros(n_q, dim, dtype=torch.float64)
        c = torch.zeros(n_c + (1 if rank == world - 1 else 0), dim, dtype=torch.float64)   # the last rank holds one candidate more
        try:
            gathered_pool_ce(q, c, torch.zeros(n_q, dtype=torch.long), inv_t, local_fn=fp64_pool_ce)
            verdict = "no error"
        except ValueError as e:
            verdict = "ValueError" if "same shapes" in str(e) else f"ValueError without the reason: {e}"
        open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write(verdict)
        dist.destroy_process_group()
        return
    weighted = case == "weighted"
    Q, C, labels, W = _problem(world, n_q, n_c, dim, weighted)
    # single process: all queries over the whole pool, labels shifted to the pool
    glob = labels + torch.arange(world).repeat_interleave(n_q) * n_c
    Qa, Ca = Q.clone().requires_grad_(True), C.clone().requires_grad_(True)
    s = Qa @ Ca.T * inv_t
    ce = torch.logsumexp(s, 1) - s.gather(1, glob[:, None])[:, 0]
    w = W if weighted else torch.ones_like(ce)
    whole = (w * ce).sum() / w.sum()
    (whole * 3.0).backward()
    # this rank's share
    qs, cs = slice(rank * n_q, (rank + 1) * n_q), slice(rank * n_c, (rank + 1) * n_c)
    q, c = Q[qs].clone().requires_grad_(True), C[cs].clone().requires_grad_(True)
    loss = gathered_pool_ce(q, c, labels[qs], inv_t, weights=W[qs] if weighted else None, local_fn=fp64_pool_ce)
    (loss * 3.0).backward()
    errs = (abs(float(loss) - float(whole)), float((q.grad - Qa.grad[qs]).abs().max()), float((c.grad - Ca.grad[cs]).abs().max()))
    ok = max(errs) <= 1e-12 and loss.dtype == torch.float64 and float(Ca.grad[cs].abs().max()) > 0
    open(os.path.join(out_dir, f"rank{rank}.txt"), "w").write("ok" if ok else f"MISMATCH loss, dq, dc errors = {errs}")
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(tmp_path, world, case, limit=120, script=None):
    """One child per rank (of `script`, this file by default), each under a time limit: a rank that hangs in a collective fails the
    test instead of stalling it."""
    port = _free_port()
    env = dict(os.environ, OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, script or os.path.abspath(__file__), str(r), str(world), str(port), case, str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs, hung = [], False
    for p in procs:
        try:
            outs.append(p.communicate(timeout=limit)[0])
        except subprocess.TimeoutExpired:
            hung = True
            for x in procs:
                x.kill()
            outs.append(p.communicate()[0])
    assert not hung, f"a rank was still running after {limit} s:\n" + "\n---\n".join(o[-3000:] for o in outs)
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r}: exit code {p.returncode}\n{o[-3000:]}"
    return [open(tmp_path / f"rank{r}.txt").read() for r in range(world)]


@pytest.mark.parametrize("case", ["plain", "weighted"])
@pytest.mark.parametrize("world", [2, 3])
def test_gathered_loss_and_gradients_equal_the_single_process_ones(tmp_path, world, case):
    """Loss on every rank and every rank's q.grad / c.grad against the single-process loss over the concatenated queries and pool,
    all in fp64: 1e-12 (the decomposition itself is exact; the differences are reordered fp64 sums)."""
    assert _run_ranks(tmp_path, world, case) == ["ok"] * world


@pytest.mark.parametrize("world", [2, 3])
def test_unequal_shapes_raise_on_every_rank_without_a_hang(tmp_path, world):
    assert _run_ranks(tmp_path, world, "unequal") == ["ValueError"] * world


if __name__ == "__main__":
    _rank_main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5])
