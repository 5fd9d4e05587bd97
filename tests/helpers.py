"""Shared test helpers: comparison of rank lists (tie-aware); child processes that must not hang silently."""
import os
import signal
import subprocess
import time

import numpy as np
import pytest


def canonicalise(ids, scores):
    """Re-order each row by (score desc, id asc) -- the reference leaves tie order unspecified."""
    out_i = np.empty_like(ids)
    out_s = np.empty_like(scores)
    for q in range(ids.shape[0]):
        o = np.lexsort((ids[q], -scores[q].astype(np.float64)))
        out_i[q], out_s[q] = ids[q][o], scores[q][o]
    return out_i, out_s


def assert_rank_close(ids, scores, ref_ids, ref_scores, tol, truncated=False):
    """ids/scores: ours (canonical order). ref_*: reference order (ties arbitrary, fp32 MKL sums).

    * scores agree rank by rank within tol;
    * ids agree at every rank whose reference score is separated from both neighbours by > 2 tol;
    * as sets, ids agree except for members whose score is within 2 tol of the cut (if truncated).
    """
    assert ids.shape == ref_ids.shape, (ids.shape, ref_ids.shape)
    np.testing.assert_allclose(scores, ref_scores, atol=tol, rtol=0)
    for q in range(ids.shape[0]):
        rs = ref_scores[q].astype(np.float64)
        gap_prev = np.r_[np.inf, rs[:-1] - rs[1:]]
        gap_next = np.r_[rs[:-1] - rs[1:], np.inf if not truncated else 0.0]
        clear = (gap_prev > 2 * tol) & (gap_next > 2 * tol)
        bad = clear & (ids[q] != ref_ids[q])
        assert not bad.any(), f"query {q}: id mismatch at clear ranks {np.nonzero(bad)[0][:10]}"
        diff = set(ids[q].tolist()) ^ set(ref_ids[q].tolist())
        if diff:
            assert truncated, f"query {q}: id sets differ {sorted(diff)[:10]}"
            cut = rs[-1]
            ours = dict(zip(ids[q].tolist(), scores[q].tolist()))
            refd = dict(zip(ref_ids[q].tolist(), ref_scores[q].tolist()))
            for j in diff:
                s = ours.get(j, refd.get(j))
                assert abs(s - cut) <= 2 * tol, f"query {q}: id {j} score {s} far from cut {cut}"


# ---------------------------------------------------------------------------------------------- synthetic shard lists for the merges
MERGE_LEVELS = np.array([-np.inf, -1.0, 0.0, 0.5, 2.0, np.inf], np.float32)
MERGE_ID_SHIFT = 3_000_000_000   # added to the ids of the last shard: global ids that no 32-bit signed field holds

# (R, k) of the full-list merge, one per launch path of csrc/ccr_merge.hip (R k < 600 ranks every element, then bisection; 256
# threads below 2048 elements; R k 12 bytes > 48 KiB opts in to dynamic LDS; > 96 KiB or R > 64 merges from global memory)
MERGE_CASES = [(1, 1), (1, 37), (2, 1), (64, 3), (5, 119), (6, 100), (7, 292), (8, 256), (4, 1024), (4, 1025), (8, 1001), (2, 4096),
               (64, 128), (3, 2731), (9, 1001), (65, 8)]


def canonical_order(scores, ids):
    """The permutation that puts one list into the canonical order (score desc, id asc)."""
    return np.lexsort((ids, -scores.astype(np.float64)))


def synthetic_shard_lists(R, n_q, k, levels, seed):
    """[R, n_q, k] per-shard lists as a search would leave them, built to stress the merge's order instead of a search's scores: per
    query R k DISTINCT ids drawn from a range three times as large (the shards interleave), the last shard's shifted by MERGE_ID_SHIFT;
    scores drawn from the first `levels` values of MERGE_LEVELS -- 1: the whole input is one plateau (of real -inf scores), 2 and 6:
    plateaus straddle the cut of every list, +-inf included -- or, with levels = 0, continuous (standard normal); every list sorted
    into the canonical order.  -> (scores fp32, ids int64)."""
    rs = np.random.RandomState(seed)
    scores = np.empty((R, n_q, k), np.float32)
    ids = np.empty((R, n_q, k), np.int64)
    for q in range(n_q):
        i = rs.permutation(3 * R * k)[:R * k].astype(np.int64).reshape(R, k)
        i[R - 1] += MERGE_ID_SHIFT
        s = MERGE_LEVELS[rs.randint(0, levels, (R, k))] if levels else rs.standard_normal((R, k)).astype(np.float32)
        for r in range(R):
            o = canonical_order(s[r], i[r])
            scores[r, q], ids[r, q] = s[r][o], i[r][o]
    return scores, ids


# ---------------------------------------------------------------------------------------------- child processes
def _proc_state(pid):
    """What the kernel says a process and its threads are doing: state + wait channel of every thread (readable without root)."""
    lines = []
    try:
        for tid in sorted(os.listdir(f"/proc/{pid}/task"), key=int):
            base = f"/proc/{pid}/task/{tid}"
            try:
                comm = open(base + "/comm").read().strip()
                state = [ln for ln in open(base + "/status").read().splitlines() if ln.startswith("State:")][0]
                wchan = open(base + "/wchan").read().strip()
                lines.append(f"  tid {tid} {comm}: {state} wchan={wchan}")
            except OSError:
                pass
    except OSError:
        lines.append(f"  pid {pid}: gone")
    return lines


def _children_of(pid):
    try:
        out = subprocess.run(["ps", "-o", "pid=", "--ppid", str(pid)], capture_output=True, text=True).stdout.split()
        kids = [int(x) for x in out]
    except Exception:
        kids = []
    return kids + [g for c in kids for g in _children_of(c)]


def run_child_with_evidence(cmd, env, tmp_path, tag, limit=240):
    """Run a bench.py child in its own process group.  A child that overruns `limit` is a FAILURE with evidence: the Python
    stacks of every rank (SIGUSR1 -> faulthandler, written to files that survive the kill), the kernel-side state and wait
    channel of every thread of every process of the group, and the child's stderr so far.  The whole group is killed then
    (a killed launcher alone would leave its ranks holding the GPU)."""
    dump_dir = tmp_path / f"{tag}_stacks"
    dump_dir.mkdir(exist_ok=True)
    env = dict(env, CCR_BENCH_WATCHDOG_DIR=str(dump_dir))
    err_path, out_path = tmp_path / f"{tag}.stderr", tmp_path / f"{tag}.stdout"
    with open(err_path, "w") as ferr, open(out_path, "w") as fout:
        proc = subprocess.Popen(cmd, stdout=fout, stderr=ferr, env=env, start_new_session=True)
        t0 = time.time()
        try:
            proc.wait(timeout=limit)
        except subprocess.TimeoutExpired:
            pids = [proc.pid] + _children_of(proc.pid)
            evidence = [f"{tag}: child still running after {time.time() - t0:.0f} s: {' '.join(cmd)}"]
            for pid in pids:
                evidence.append(f"pid {pid}: {open(f'/proc/{pid}/cmdline').read().replace(chr(0), ' ')[:200] if os.path.exists(f'/proc/{pid}/cmdline') else 'gone'}")
                evidence += _proc_state(pid)
            for pid in pids:
                if not _children_of(pid):                  # the ranks (leaves): launchers have no handler and would just die
                    try:
                        os.kill(pid, signal.SIGUSR1)       # faulthandler: every thread's Python stack into the dump file
                    except OSError:
                        pass
            time.sleep(3)
            try:
                os.killpg(proc.pid, signal.SIGKILL)
            except OSError:
                pass
            try:
                proc.wait(timeout=30)
            except subprocess.TimeoutExpired:
                evidence.append("child did not die within 30 s of SIGKILL (uninterruptible)")
            for f in sorted(dump_dir.iterdir()):
                evidence.append(f"--- {f.name}\n{f.read_text()[-6000:]}")
            evidence.append(f"--- stderr\n{err_path.read_text()[-6000:]}")
            pytest.fail("\n".join(evidence))
    stderr, stdout = err_path.read_text(), out_path.read_text()
    if proc.returncode != 0:   # includes the in-child watchdog (exit code 1 after its stack dump)
        dumps = "".join(f"--- {f.name}\n{f.read_text()[-6000:]}\n" for f in sorted(dump_dir.iterdir()))
        pytest.fail(f"{tag}: exit code {proc.returncode}\n{dumps}--- stderr\n{stderr[-6000:]}")
    return stdout, stderr




# ---------------------------------------------------------------------------------------------- goldens g18 / g19 (shared with tools/make_golden.py)
class GoldenTokenizer:
    """Deterministic whitespace tokenizer with the HF call shapes the reference uses (padding=True | "max_length" | False, truncation,
    max_length, return_tensors="pt"): id = 4 + crc32(word) % (vocab - 4); [CLS] = 1, [SEP] = 2, [PAD] = 0.  (No Python hash(): the golden
    generator and the tests must tokenise alike in every process.)"""
    pad_token_id = 0

    def __init__(self, vocab=64):
        self.vocab = int(vocab)

    def __call__(self, texts, truncation=True, padding=True, max_length=32, return_tensors="pt", **kw):
        import zlib
        import torch
        ids = [[1] + [4 + zlib.crc32(w.encode()) % (self.vocab - 4) for w in t.split()][: max_length - 2] + [2] for t in texts]
        if padding is False:
            return {"input_ids": ids, "attention_mask": [[1] * len(r) for r in ids]}
        L = max_length if padding == "max_length" else max(len(r) for r in ids)
        out = torch.zeros(len(ids), L, dtype=torch.int64)
        mask = torch.zeros(len(ids), L, dtype=torch.int64)
        for r, row in enumerate(ids):
            out[r, :len(row)] = torch.tensor(row)
            mask[r, :len(row)] = 1
        return {"input_ids": out, "attention_mask": mask}


def numpy_seeded_bert(cfg, seed):
    """A transformers BertModel whose every parameter is drawn from numpy's RandomState(seed) in named_parameters() order (the same
    bits on every host and torch build -- torch's own CPU normal sampler depends on the vector width): weights N(0, 0.05) with the
    query / key projections x 6 (softmaxes that are not uniform), LayerNorm weights U(0.6, 1.4), biases N(0, 0.05); every value
    rounded to a bf16-exact fp32.  eval() mode."""
    import torch
    from transformers import BertConfig, BertModel
    model = BertModel(BertConfig(**cfg)).eval()
    rs = np.random.RandomState(seed)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            shape = tuple(prm.shape)
            if "LayerNorm.weight" in name:
                v = rs.uniform(0.6, 1.4, shape)
            else:
                v = rs.standard_normal(shape) * 0.05
                if "attention.self.query.weight" in name or "attention.self.key.weight" in name:
                    v = v * 6.0
            prm.copy_(torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16).float())
    return model


G18_CFG = dict(vocab_size=64, hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, max_position_embeddings=40)
G19_CFG = dict(vocab_size=64, hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=128, max_position_embeddings=24)


def golden_texts(n, seed, longest=20, words=150):
    rs = np.random.RandomState(seed)
    vocab = [f"w{i}" for i in range(words)]
    return [" ".join(rs.choice(vocab, rs.randint(1, longest + 1))) for _ in range(n)]


# ---------------------------------------------------------------------------------------------- the part probe of the contrastive losses
# One operand of the loss is ONE-HOT, so every element of the gradient on the other side is a single product g * amplitude: the GEMM adds
# nothing to the error and what is left is the accuracy of g itself -- fp32 lse, fp32 exp, the fp32 scale and the split into bf16 parts
# (g = hi + mid + lo).  The kernels' bound is a third of what the same fp32 arithmetic gives with TWO parts (hi + mid), computed from the
# same inputs by loss_probe_errors below; tests/test_cpu_loss_probe.py shows that three parts pass it and two cannot.
LOSS_PROBE_INV_T = 4.0
INBATCH_PROBE_SHAPES = [(40, 128), (33, 144), (64, 128), (96, 384)]         # (B, dim): row-major x 2, fragment-major with 2B = dim, and a wider one
POOL_PROBE_SHAPES = [("dq", 40, 100, 128), ("dc", 100, 40, 128)]           # (side, n_q, n_c, dim)


def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32.  Finite inputs."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_parts(g, n_parts):
    """split3 of the kernels, cut after n_parts: g = p0 + p1 + ... with every p a bf16 and every residual taken in fp32."""
    parts, r = [], np.asarray(g, np.float32)
    for _ in range(n_parts):
        p = bf16_round(r)
        parts.append(p)
        r = (r - p).astype(np.float32)
    return parts


def loss_probe(side, n_q, n_c, dim, seed):
    """-> (q [n_q, dim], c [n_c, dim]) fp32 holding bf16 values.  side "dq": the candidates are one-hot (row j = b_j e_sigma(j), sigma
    injective, b_j in {1/2, 1, 2}) and the queries dense (randn / 8), so dQ[i][sigma(j)] = G_ij b_j and every other column is 0;
    side "dc": the mirror image, dC[j][pi(i)] = G_ij a_i."""
    rs = np.random.RandomState(seed)
    n_hot, n_dense = (n_c, n_q) if side == "dq" else (n_q, n_c)
    assert n_hot <= dim, "one column per one-hot row"
    dense = bf16_round((rs.standard_normal((n_dense, dim)) * 0.125).astype(np.float32))
    hot = np.zeros((n_hot, dim), np.float32)
    hot[np.arange(n_hot), rs.permutation(dim)[:n_hot]] = np.array([0.5, 1.0, 2.0], np.float32)[rs.randint(0, 3, n_hot)]
    return (dense, hot) if side == "dq" else (hot, dense)


def loss_probe_errors(side, q, c, labels, weights, grad_out, kind):
    """The probe's fp64 gradient and what fp32 arithmetic with two and with three bf16 parts makes of it.
    kind "inbatch": the scale is inv_T / n_q * grad_out (no weights); kind "pool": w_i * (inv_T * grad_out / sum w).
    -> (ref fp64 [rows, dim], loss fp64, E3, E2): E = the largest relative error of an element whose reference is not 0."""
    inv_t = LOSS_PROBE_INV_T
    n_q = q.shape[0]
    s = q.astype(np.float64) @ c.astype(np.float64).T * inv_t
    s32 = s.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), s), "the probe's logits are exact in fp32"
    assert np.array_equal((q @ c.T) * np.float32(inv_t), s32), "... and an fp32 GEMM finds them"
    w = np.ones(n_q) if weights is None else np.asarray(weights, np.float64)
    hit = np.zeros(s.shape, bool)
    hit[np.arange(n_q), labels] = True
    # fp64
    m = s.max(1, keepdims=True)
    lse = m + np.log(np.exp(s - m).sum(1, keepdims=True))
    assert np.abs(s - lse).max() <= 12.0, "the derivation of the kernel's own error assumes |s - lse| <= 12"
    loss = float((w * (lse[:, 0] - s[hit])).sum() / w.sum())
    G = (np.exp(s - lse) - hit) * (w[:, None] * inv_t * grad_out / w.sum())
    ref = G @ c.astype(np.float64) if side == "dq" else G.T @ q.astype(np.float64)
    # fp32, as the kernels evaluate it
    f32 = np.float32
    m32 = s32.max(1, keepdims=True)
    lse32 = (m32 + np.log(np.exp(s32 - m32).sum(1, keepdims=True, dtype=f32))).astype(f32)
    e32 = (np.exp(s32 - lse32) - hit.astype(f32)).astype(f32)
    if kind == "inbatch":
        coef = np.full((n_q, 1), f32(f32(inv_t) / f32(n_q)) * f32(grad_out), f32)
    else:
        coef = (w.astype(f32) * f32(f32(f32(inv_t) * f32(grad_out)) / f32(w.sum())))[:, None].astype(f32)
    g32 = (e32 * coef).astype(f32)
    hot = c if side == "dq" else q
    errs = []
    for n_parts in (3, 2):
        acc = np.zeros(ref.shape, f32)
        for p in bf16_parts(g32, n_parts):   # one product per element: the other terms of the GEMM are exact zeros
            acc = (acc + (p @ hot if side == "dq" else p.T @ hot)).astype(f32)
        errs.append(probe_error(acc, ref))
    return ref, loss, errs[0], errs[1]


def probe_error(got, ref):
    """Largest relative error over the elements whose reference is not 0; where it is 0 the value must be exactly 0."""
    got = np.asarray(got, np.float64)
    nz = ref != 0
    assert nz.any() and np.array_equal(got[~nz], np.zeros((~nz).sum())), "an element whose reference is 0 is not exactly 0"
    return float((np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])).max())


def loss_probe_case(kind, side, n_q, n_c, dim):
    """One probe, complete: operands, labels, weights (pool only; a fifth of them 0) and grad_out.  In-batch: n_c = 2 n_q."""
    seed = 7 * n_q + n_c + dim + (side == "dc")
    q, c = loss_probe(side, n_q, n_c, dim, seed)
    rs = np.random.RandomState(seed + 1)
    if kind == "inbatch":
        assert n_c == 2 * n_q
        return q, c, np.arange(n_q), None, 1.0
    w = (rs.rand(n_q) + 0.1).astype(np.float32)
    w[::5] = 0.0
    return q, c, rs.randint(0, n_c, n_q), w, 1.0
