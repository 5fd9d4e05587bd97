"""Shared test helpers: comparison of rank lists (tie-aware); child processes that must not hang silently."""
import math
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


# ---------------------------------------------------------------------------------------------- the selector probe of the attention backward
# Inputs for which every element of dQ, dK and dV is a sum of a few exactly representable products, so that a streamed row that is dropped,
# doubled or misplaced moves an element by many spacings instead of hiding in rounding noise.  One head (width 64, scale 1/8), before its roll:
#   columns  0..47  the 8-bit CODE of a key group, as +-4, repeated 6 times: K holds the code of the key's own group, Q the code of the group
#                   the query SELECTS.  A group is a pair of keys (partners drawn from different 32-row tiles where the length allows) or,
#                   with an odd length, the one key left single.
#   columns 48..55  Q payload, integers in [-2, 2]; K is zero there
#   columns 56..63  K payload, integers in [-2, 2]; Q is zero there
# so a query scores 48 * 16 / 8 = 96 on the keys of its group, both alike, and at most 96 - 2 * 16 * 6 / 8 = 72 on any other: the softmax is
# (1/2, 1/2) on a pair or 1 on a single key up to e^-24, O = (V_a + V_b) / 2, dV = 1/2 sum d_out over the selecting queries,
# dS = +-1/4 (dp_a - dp_b), dQ = 1/32 (dp_a - dp_b) (K_a - K_b) (non-zero on the K payload only: the codes cancel) and
# dK = 1/32 sum_i +-(dp_a - dp_b)_i Q_i.  V has 4 non-zero columns per row and d_out is dense, integers in [-2, 2].
# dQ lives on the 8 K-payload columns of a head, so it takes EIGHT heads, rolled by 0, 8, .., 56 columns, for every column of dQ to be
# non-zero somewhere (four heads rolled by 16 reach 32 of the 64).  The query -> group map is many-to-one and drawn so that every
# (query tile, key tile) pair of 32 x 32 rows holds a selected key in every head; a tile with too few queries for that (the one-row tile of
# length 257) reaches every key tile over the eight heads.
ENC_PROBE_LENS = [2, 31, 33, 64, 65, 257, 512]
ENC_PROBE_HEADS = 8
ENC_PROBE_MARGIN = 24.0        # lowest (own group's score - any other score), asserted by tests/test_cpu_encoder_probe.py
ENC_PROBE_SNAP = 64.0          # every exact gradient is a multiple of 1 / 64


def round16(x, kind):
    """float32 -> the nearest value of the 16-bit type ("bf16" | "fp16", ties to even), as float32."""
    x = np.ascontiguousarray(x, np.float32)
    return bf16_round(x) if kind == "bf16" else x.astype(np.float16).astype(np.float32)


def attention_grads_fp64(q, k, v, d_out, scale=0.125):
    """Plain softmax attention of one head and its backward in numpy fp64 -> (out, lse, dq, dk, dv, p)."""
    q, k, v, d_out = (np.asarray(a, np.float64) for a in (q, k, v, d_out))
    s = q @ k.T * scale
    m = s.max(1, keepdims=True)
    e = np.exp(s - m)
    lse = m[:, 0] + np.log(e.sum(1))
    p = e / e.sum(1, keepdims=True)
    out = p @ v
    ds = p * (d_out @ v.T - (d_out * out).sum(1, keepdims=True))
    return out, lse, ds @ k * scale, ds.T @ q * scale, p.T @ d_out, p


def _probe_head_draw(length, head, rs):
    tile = np.arange(length) // 32
    n_tiles = int(tile[-1]) + 1
    perm = rs.permutation(length)
    a, b = perm[0:length - length % 2:2].copy(), perm[1:length:2].copy()
    for i in np.nonzero(tile[a] == tile[b])[0]:          # partners into different tiles where a swap of two partners does it
        for j in rs.permutation(len(a)):
            if tile[a[i]] != tile[b[j]] and tile[a[j]] != tile[b[i]]:
                b[i], b[j] = b[j], b[i]
                break
    groups = [(int(x), int(y)) for x, y in zip(a, b)] + ([(int(perm[-1]),)] if length % 2 else [])
    codes = rs.permutation(256)[:len(groups)]
    group_tiles = [set(int(tile[m]) for m in grp) for grp in groups]
    select = np.empty(length, np.int64)
    for t in range(n_tiles):                              # greedy: the tile's queries first reach every key tile, then draw freely
        mine = np.nonzero(tile == t)[0]
        missing = set(range(n_tiles))
        if 2 * len(mine) < n_tiles:                       # too few queries for every key tile: each head takes its share of them
            first = 2 * head % n_tiles
            missing = {first, first + 1} & set(range(n_tiles))
        for i in rs.permutation(mine):
            choice = int(rs.randint(len(groups)))
            if missing:
                gain = np.array([len(gt & missing) for gt in group_tiles])
                best = np.nonzero(gain == gain.max())[0]
                choice = int(best[rs.randint(len(best))])
                missing -= group_tiles[choice]
            select[i] = choice
    bits = lambda c: np.tile(((np.asarray(c)[:, None] >> np.arange(8)) & 1) * 8.0 - 4.0, (1, 6))      # [n, 48] of +-4
    group_of_key = np.empty(length, np.int64)
    for gi, grp in enumerate(groups):
        group_of_key[list(grp)] = gi
    q, k, v = np.zeros((length, 64)), np.zeros((length, 64)), np.zeros((length, 64))
    q[:, :48], k[:, :48] = bits(codes[select]), bits(codes[group_of_key])
    q[:, 48:56] = rs.randint(-2, 3, (length, 8))
    k[:, 56:64] = rs.randint(-2, 3, (length, 8))
    for r in range(length):
        v[r, rs.permutation(64)[:4]] = rs.choice([-2.0, -1.0, 1.0, 2.0], 4)
    d_out = rs.randint(-2, 3, (length, 64)).astype(np.float64)
    return dict(q=q, k=k, v=v, d_out=d_out, groups=groups, select=select, group_of_key=group_of_key)


def snap_exact(x):
    """The exact value of a probe gradient: the fp64 result snapped to a multiple of 1 / 64 (what is left is the e^-24 leak)."""
    return np.round(np.asarray(x, np.float64) * ENC_PROBE_SNAP) / ENC_PROBE_SNAP


def encoder_probe_head(length, head, seed):
    """One (sequence, head) of the probe, Q and K rolled by 8 * head columns.  Draws are repeated (seed + 1000 * attempt) until every exact
    gradient is a bf16 value -- eight significant bits; fp16 holds whatever bf16 does at these magnitudes -- so the builder never hands
    out a rounding lottery; tests/test_cpu_encoder_probe.py asserts the result again."""
    for attempt in range(200):
        h = _probe_head_draw(length, head, np.random.RandomState(seed + 1000 * attempt))
        h["q"], h["k"] = np.roll(h["q"], 8 * head, axis=1), np.roll(h["k"], 8 * head, axis=1)
        grads = attention_grads_fp64(h["q"], h["k"], h["v"], h["d_out"])[2:5]
        exact = [snap_exact(g) for g in grads]
        if all(np.array_equal(bf16_round(e.astype(np.float32)).astype(np.float64), e) for e in exact):
            h["attempt"] = attempt
            return h
    raise AssertionError(f"no representable probe for length {length}, head {head}")


_ENC_PROBE = {}


def encoder_probe():
    """The whole probe, built once per process: per sequence of ENC_PROBE_LENS qkv [len, 3, H, 64] and d_out [len, H, 64] (fp64 arrays of
    integers), plus the per-head draws (groups, select) for the checks of the builder itself."""
    if not _ENC_PROBE:
        seqs = []
        for si, length in enumerate(ENC_PROBE_LENS):
            heads = [encoder_probe_head(length, h, seed=100 * si + h) for h in range(ENC_PROBE_HEADS)]
            qkv = np.stack([np.stack([hd[name] for hd in heads], axis=1) for name in ("q", "k", "v")], axis=1)      # [len, 3, H, 64]
            d_out = np.stack([hd["d_out"] for hd in heads], axis=1)                                                  # [len, H, 64]
            seqs.append(dict(length=length, heads=heads, qkv=qkv, d_out=d_out))
        _ENC_PROBE["seqs"] = seqs
    return _ENC_PROBE["seqs"]


def encoder_probe_leak_bound(length):
    """What the unselected keys can add to any gradient element: at most `length` of them, each with P <= e^-margin, times 64 columns of
    operands no larger than 4 -- from the margin, not measured."""
    return length * np.exp(-ENC_PROBE_MARGIN) * 64 * 4


def emulate_attention_bwd(q, k, v, d_out, kind, swap_rows=None, row_factor=True):
    """The arithmetic of csrc/ccr_encoder_bwd.hip for one head on the CPU: fp32 scores, lse and P = exp2(s scale log2e - lse log2e), dS = P (dP -
    delta) in fp32, dS and P rounded to the 16-bit type (fp16: under the per-own-row power-of-two factor 2^(8 - e_run), the accumulator rescaled
    when e_run grows), fp32 accumulation over streamed tiles of 32 rows, `scale` applied once, one rounding at the end.
    swap_rows = (i, j): the accumulating products read streamed rows i and j of every tile in each other's place (a misplaced transposed read).
    -> (dq, dk, dv) float32 holding values of the type."""
    f32 = np.float32
    q, k, v, d_out = (np.asarray(a, f32) for a in (q, k, v, d_out))
    n = q.shape[0]
    scale, log2e = f32(0.125), f32(1.4426950408889634)
    scale_log2e = f32(scale * log2e)
    raw = q @ k.T
    s = raw * scale
    m = s.max(1, keepdims=True)
    lse = (m[:, 0] + np.log(np.exp(s - m).sum(1, dtype=f32))).astype(f32)
    out = round16(round16(np.exp(s - lse[:, None]), kind) @ v, kind)          # the forward's output, 16-bit
    delta = (d_out * out).sum(1, dtype=f32)
    lse2 = (lse * log2e).astype(f32)
    p = np.exp2((raw.astype(np.float64) * np.float64(scale_log2e) - lse2[:, None].astype(np.float64)).astype(f32)).astype(f32)      # one fma
    ds = (p * ((d_out @ v.T) - delta[:, None])).astype(f32)
    scaled = kind == "fp16" and row_factor

    def stream(ds_own, p_own, x1, x2):
        """own rows x streamed rows: ds_own, p_own [own, streamed]; x1, x2 [streamed, 64] -> (acc, accv)."""
        own = ds_own.shape[0]
        acc, accv = np.zeros((own, 64), f32), np.zeros((own, 64), f32)
        e_run = np.full(own, -1000)
        for t0 in range(0, ds_own.shape[1], 32):
            d_t, p_t = ds_own[:, t0:t0 + 32], p_own[:, t0:t0 + 32]
            a1, a2 = x1[t0:t0 + 32].copy(), x2[t0:t0 + 32].copy()
            if swap_rows is not None and max(swap_rows) < a1.shape[0]:
                i, j = swap_rows
                a1[[i, j]], a2[[i, j]] = a1[[j, i]], a2[[j, i]]
            if scaled:
                amax = np.abs(d_t).max(1)
                ex = np.maximum(np.floor(np.log2(np.where(amax > 0, amax, 1.0))).astype(np.int64), -100)
                grow = (amax > 0) & (ex > e_run)
                shrink = np.where(e_run == -1000, 0.0, np.exp2((e_run - ex).astype(np.float64))).astype(f32)
                acc[grow] *= shrink[grow][:, None]
                e_run = np.where(grow, ex, e_run)
                factor = np.where(e_run == -1000, 0.0, np.exp2((8 - e_run).astype(np.float64))).astype(f32)
                d_t = d_t * factor[:, None]
            acc += round16(d_t, kind) @ a1
            accv += round16(p_t, kind) @ a2
        unscale = np.full(own, scale, f32)
        if scaled:
            unscale = np.where(e_run == -1000, 0.0, scale * np.exp2((e_run - 8).astype(np.float64))).astype(f32)
        return acc * unscale[:, None], accv

    dq, _ = stream(ds, p, k, v)
    dk, dv = stream(np.ascontiguousarray(ds.T), np.ascontiguousarray(p.T), q, d_out)
    return tuple(round16(g, kind) for g in (dq, dk, dv))


# ---------------------------------------------------------------------------------------------- encoder backward: cases, inputs, references
# (shared by tests/test_gpu_encoder_train.py and tests/test_gpu_encoder_train_edges.py)
import torch  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
MANTISSA = {torch.bfloat16: 7, torch.float16: 10}      # explicit significand bits: one spacing at v is 2^(floor(log2 |v|) - bits)


def spacing(value, dtype):
    """One spacing (ulp) of the 16-bit type at |value| (a Python float; normal range)."""
    return 2.0 ** (math.floor(math.log2(abs(value))) - MANTISSA[dtype])


ATT_CASES = {
    "padded_edges": ("padded", [1, 2, 31, 32, 33, 63, 64, 65], 2),
    "packed_blocks": ("packed", [127, 128, 129, 255, 256, 257], 3),
    "padded_512_empty": ("padded", [512, 300, 1, 0], 2),           # an empty sequence appended
    "packed_12_heads": ("packed", [136, 17, 200], 12),
}


def att_inputs(kind, lens, H, dtype, seed):
    """qkv ~ 1.5 N(0, 1), d_out ~ N(0, 1), rounded to the type; padding rows (padded batches) are NaN."""
    g = torch.Generator().manual_seed(seed)
    n = len(lens)
    if kind == "padded":
        L = max(lens)
        starts, pad_len, T = [s * L for s in range(n)], L, n * L
    else:
        starts, pad_len, T = [sum(lens[:s]) for s in range(n)], 0, sum(lens)
    qkv = (1.5 * torch.randn(T, 3 * H * 64, generator=g)).to(dtype)
    d_out = torch.randn(T, H * 64, generator=g).to(dtype)
    live = torch.zeros(T, dtype=torch.bool)
    for s, ln in zip(starts, lens):
        live[s:s + ln] = True
    qkv[~live] = float("nan")
    d_out[~live] = float("nan")
    dev = "cuda"
    return dict(qkv=qkv.to(dev), d_out=d_out.to(dev), live=live.to(dev), starts=starts, lens=lens, H=H, pad_len=pad_len, max_len=max(max(lens), 1),
                seq_start=torch.tensor(starts, dtype=torch.int32, device=dev), seq_len=torch.tensor(lens, dtype=torch.int32, device=dev))


def att_reference(case, half):
    """Per (sequence, head): autograd of softmax(Q K^T / 8) V on the rounded operands.  half None: everything fp32 (the reference).
    half = a 16-bit type: the matmul operands and results are 16-bit and the softmax fp32 -- autocast's arithmetic (the yardstick).
    -> (d_qkv fp32 [T, 3 H 64] with zeros on padding rows, lse fp32 [T, H])."""
    qkv, d_out, H = case["qkv"], case["d_out"], case["H"]
    T = qkv.shape[0]
    grad = torch.zeros(T, 3 * H * 64, dtype=torch.float32, device=qkv.device)
    lse = torch.zeros(T, H, dtype=torch.float32, device=qkv.device)
    for s, ln in zip(case["starts"], case["lens"]):
        if ln == 0:
            continue
        rows = qkv[s:s + ln].view(ln, 3, H, 64).permute(1, 2, 0, 3)          # [3, H, len, 64]
        dt = torch.float32 if half is None else half
        q, k, v = (rows[i].to(dt).detach().clone().requires_grad_(True) for i in range(3))
        scores = (q @ k.transpose(1, 2)).float() * 0.125
        p = torch.softmax(scores, dim=-1)
        o = p.to(dt) @ v
        do = d_out[s:s + ln].view(ln, H, 64).permute(1, 0, 2).to(dt)
        o.backward(do)
        g3 = torch.stack([q.grad, k.grad, v.grad]).float()                    # [3, H, len, 64]
        grad[s:s + ln] = g3.permute(2, 0, 1, 3).reshape(ln, 3 * H * 64)
        lse[s:s + ln] = torch.logsumexp(scores.detach(), dim=-1).T
    return grad, lse


def run_att(case, d_out=None):
    from ccrec_amd import ops
    out, lse = ops.attention_fwd_train(case["qkv"], case["seq_start"], case["seq_len"], case["H"], case["max_len"], case["pad_len"])
    out_nan = out.clone()
    out_nan[~case["live"]] = float("nan")                 # the backward must not read the forward's padding rows either
    d_qkv = ops.attention_bwd(case["qkv"], out_nan, lse, case["d_out"] if d_out is None else d_out, case["seq_start"], case["seq_len"],
                              case["H"], case["max_len"], case["pad_len"])
    return out, lse, d_qkv


LN_EPS = 1e-12      # BERT's


def ln_inputs(rows, dim, dtype, with_res, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, dim, generator=g).to(dtype)
    res = torch.randn(rows, dim, generator=g) if with_res else None
    if rows >= 4:
        x[1] = 0.5                       # a row of equal elements: 0.5 (+ 1.25) is exact in every format
        if with_res:
            res[1] = 1.25
            res[2] += 1000.0             # a large common offset
        else:
            x[2] = (x[2].float() + 1000.0).to(dtype)
    gamma = 1.0 + 0.2 * torch.randn(dim, generator=g)
    d_y = torch.randn(rows, dim, generator=g)
    dev = "cuda"
    return x.to(dev), None if res is None else res.to(dev), gamma.to(dev), d_y.to(dev)


def ln_torch_backward(v, gamma, d_y, dt):
    """d v, d gamma, d beta of F.layer_norm(v) * gamma + beta in precision dt, from the SAME summed input v = x + residual (fp32)."""
    v = v.to(dt).detach().requires_grad_(True)
    gm = gamma.to(dt).detach().requires_grad_(True)
    bt = torch.zeros_like(gm).requires_grad_(True)
    torch.nn.functional.layer_norm(v, (v.shape[1],), gm, bt, LN_EPS).backward(d_y.to(dt))
    return v.grad, gm.grad, bt.grad


# ---------------------------------------------------------------------------------------------- the bpr objective: builders and checks
# (shared by tests/test_gpu_bpr.py and tests/test_gpu_bpr_edges.py; the integer probe also by tests/test_cpu_bpr_probe.py)
LAST_U = 1.0 - 2.0 ** -53


def make_prior(n_users, n_items, row_len, values, seed):
    """CSR with row_len(u) entries in row u (columns ascending and unique), values(rng, m) fp32."""
    rng = np.random.default_rng(seed)
    ptr, idx, t = [0], [], []
    for u in range(n_users):
        m = row_len(u)
        idx.append(np.sort(rng.choice(n_items, size=m, replace=False)).astype(np.int64))
        t.append(np.asarray(values(rng, m), dtype=np.float32))
        ptr.append(ptr[-1] + m)
    return np.asarray(ptr, dtype=np.int64), np.concatenate(idx) if idx else np.zeros(0, np.int64), np.concatenate(t) if t else np.zeros(0, np.float32)


def dense_weights(u, prior, t0, proposal):
    """w_j = proposal_j exp(t_uj - M) of one user in fp64 (the numerators of the softmax after its max-shift)."""
    trow = np.full(proposal.shape[0], np.float64(np.float32(t0)))
    if prior is not None:
        ptr, idx, t = prior
        trow[idx[ptr[u]:ptr[u + 1]]] = t[ptr[u]:ptr[u + 1]].astype(np.float64)
    return proposal.astype(np.float64) * np.exp(trow - trow.max())


def run_sampler(users, n_neg, n_items, prior, t0, uniforms=None, seed=0, proposal=None):
    from ccrec_amd import ops
    rng = np.random.default_rng(seed)
    drawn = ((rng.integers(0, 50, n_items) + 0.1) ** 0.5).astype(np.float32)   # (drawn either way: the uniforms stay the same)
    proposal = drawn if proposal is None else np.ascontiguousarray(proposal, dtype=np.float32)
    prop = torch.from_numpy(proposal).cuda()
    cdf = ops.bpr_proposal_cdf(prop)
    B = len(users)
    if uniforms is None:
        uniforms = rng.random((n_neg, B))
    uni = torch.from_numpy(np.ascontiguousarray(uniforms, dtype=np.float64)).cuda()
    dev_prior = None
    if prior is not None:
        ptr, idx, t = prior
        dev_prior = (torch.from_numpy(ptr).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(t).cuda(), int(np.diff(ptr).max()))
    usr = torch.from_numpy(np.asarray(users, dtype=np.int64)).cuda()
    got = ops.bpr_sample_negatives(usr, n_neg, prop, cdf, prior=dev_prior, t0=t0, uniforms=uni)
    again = ops.bpr_sample_negatives(usr, n_neg, prop, cdf, prior=dev_prior, t0=t0, uniforms=uni)
    assert got.shape == (n_neg, B) and got.dtype == torch.int64 and torch.equal(got, again)   # a second call: identical output
    return got.cpu().numpy(), proposal, cdf.cpu().numpy(), np.asarray(uniforms, dtype=np.float64)


def check_draws(got, users, prior, t0, proposal, cdf, uniforms):
    """Every draw equals searchsorted(cumsum(w), u Z, 'right'), or the target lies within 1e-9 Z of the boundary between the two
    answers and they are neighbours among the items of non-zero weight; at most 0.1 % of the draws may be excused that way."""
    excused = 0
    for b, u in enumerate(users):
        w = dense_weights(u, prior, t0, proposal)
        cum = np.cumsum(w) if prior is not None else cdf   # (no prior: the weights are the proposal, their running sum the cdf itself)
        Z = cum[-1]
        target = uniforms[:, b] * Z
        ref = np.searchsorted(cum, target, side="right")
        for n in np.nonzero(got[:, b] != ref)[0]:
            lo, hi = sorted((int(got[n, b]), int(ref[n])))
            assert 0 <= lo and hi < len(w), (b, n, got[n, b], ref[n])
            assert w[lo] > 0 and w[hi] > 0 and not w[lo + 1:hi].any(), f"row {b} draw {n}: {got[n, b]} and {ref[n]} are not neighbours"
            assert abs(target[n] - cum[lo]) <= 1e-9 * Z, f"row {b} draw {n}: {got[n, b]} != {ref[n]}, target {target[n]!r} boundary {cum[lo]!r}"
            excused += 1
    print(f"draws {got.size} excused {excused}")
    assert excused <= 1e-3 * got.size


def restate_frozen(table, gamma, beta, eps, ptr_i, ptr_j, ptr_nj, w):
    """bbpr.py:144-147, 180-185 with forward = LayerNorm(all_cls[ptr]) in torch fp64 on the CPU -> loss, dgamma, dbeta (grad_out = 1)."""
    T = table.detach().cpu().double()
    dim = T.shape[1]
    g = gamma.detach().cpu().double().requires_grad_(True) if gamma is not None else None
    b = beta.detach().cpu().double().requires_grad_(True) if beta is not None else None
    pi, pj, pnj, wd = ptr_i.cpu(), ptr_j.cpu(), ptr_nj.cpu(), w.detach().cpu().double()
    emb = lambda p: torch.nn.functional.layer_norm(T[p], (dim,), g, b, eps)
    pos = (emb(pi) * emb(pj)).sum(-1)
    neg = (emb(pi) * emb(pnj)).sum(-1)
    loglik = torch.nn.functional.logsigmoid(pos - neg)
    loss = (-loglik * wd).sum() / (pnj.shape[0] * wd.sum())
    if g is None:
        return float(loss), None, None, (pos - neg).detach()
    loss.backward()
    return float(loss.detach()), g.grad.numpy(), b.grad.numpy(), (pos - neg).detach()


def check_loss(got, ref):
    print(f"loss {got!r} ref {ref!r} err {abs(got - ref):.3e}")
    assert abs(got - ref) < 2e-5 * max(1.0, abs(ref))


def check_grad(got, ref, scale=1.0, what=""):
    got = got.detach().float().cpu().numpy()
    print(f"{what} max |got - ref| {np.abs(got - scale * ref).max():.3e} of max |ref| {np.abs(scale * ref).max():.3e}")
    np.testing.assert_allclose(got, scale * ref, rtol=2e-4, atol=3e-4 * np.abs(scale * ref).max())


def frozen_problem(B, n_neg, dim, n_rows, gamma_scale=0.05, seed=None):
    g = torch.Generator().manual_seed(B * 131 + dim if seed is None else seed)
    table = torch.randn(n_rows, dim, generator=g) * (0.5 + torch.rand(n_rows, 1, generator=g)) + torch.randn(n_rows, 1, generator=g) * 0.3
    if gamma_scale == 1.0:
        gamma, beta = torch.ones(dim), torch.zeros(dim)
    else:
        gamma = gamma_scale * (1.0 + 0.2 * torch.randn(dim, generator=g))
        beta = 0.02 * torch.randn(dim, generator=g)
    ptr_i = torch.randint(0, n_rows, (B,), generator=g)
    ptr_j = torch.randint(0, n_rows, (B,), generator=g)
    ptr_nj = torch.randint(0, n_rows, (n_neg, B), generator=g)
    if B > 2:
        ptr_nj[0, ::3] = ptr_j[::3]      # duplicate pointers: these differences are exactly 0
    else:                                # one row: three different pointers (with ptr_nj == ptr_j the true gradient is zero, and a
        ptr_i[0], ptr_j[0], ptr_nj[0, 0] = 0, 1, 2                           # bound relative to max |ref| says nothing about it)
    if gamma_scale == 1.0 and B > 2 and n_neg > 1:
        ptr_j[1], ptr_nj[1, 2] = ptr_i[1], ptr_i[2]      # e_i . e_i = dim: differences of about +dim and -dim
    w = torch.rand(B, generator=g) + 0.1
    w[::5] = 0.0
    if B == 1:
        w[0] = 0.7
    return table, gamma, beta, ptr_i, ptr_j, ptr_nj, w


def run_frozen(table, gamma, beta, eps, ptr_i, ptr_j, ptr_nj, w, scale=3.0):
    from ccrec_amd import ops
    gc, bc = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    loss = ops.bpr_frozen_loss(table.cuda(), gc, bc, eps, ptr_i.cuda(), ptr_j.cuda(), ptr_nj.cuda(), w.cuda())
    (loss * scale).backward()
    return loss.detach(), gc.grad, bc.grad


# The integer probe of the frozen loss: table rows of +-1 with as many +1 as -1, so that with eps = 0 the LayerNorm's mean is 0, its variance
# 1, rstd 1 and xh = x, all exact in fp32.  x_n is x_j with 2p columns flipped (p of each sign: x_n stays balanced), x_i is x_j with q of
# those columns flipped (and as many columns outside them as keep it balanced), so with beta = 0
#   D = gamma^2 sum_d x_i (x_j - x_n) = gamma^2 * 2 (2p - 2q) = gamma^2 * 4 (p - q):   every multiple of 4 at gamma = 1, every integer at 1/2,
# and the gradients live on the flipped columns alone: R = -sigmoid(-D) (x_j - x_n), dbeta = R gamma, dgamma = R 2 x_i gamma.
BPR_PROBE_KS = list(range(-32, 33))      # k = p - q


def bpr_integer_probe(dim, k, variant):
    """-> (x_i, x_j, x_n [dim] fp32 of +-1, the flipped columns).  variant 0: the fewest flips (p = |k|; k = 0: one agreeing and one
    disagreeing flip); variant 1: p drawn from [max(|k|, 1), 31] and the columns spread over the row."""
    half = dim // 2
    assert dim % 2 == 0 and abs(k) <= 32 <= half
    rng = np.random.default_rng(1000 * dim + 10 * (k + 32) + variant)
    perm = rng.permutation(dim) if variant else np.arange(dim).reshape(half, 2).T.reshape(-1)      # variant 0: x_j = +1 on the even columns
    plus, minus = perm[:half], perm[half:]
    p = max(abs(k), 1)
    if variant and abs(k) < 31:
        p = int(rng.integers(p, 32))
    q = p - k
    assert 0 <= q <= 2 * p
    q_plus, q_minus = (q + 1) // 2, q // 2
    extra = q_plus - q_minus                                  # an odd q: one more disagreement outside the flips, on a -1 column
    r = int(rng.integers(0, half - p - extra + 1)) if variant else 0
    assert p + extra + r <= half
    xj = np.empty(dim, np.float32)
    xj[plus], xj[minus] = 1.0, -1.0
    flipped = np.sort(np.concatenate([plus[:p], minus[:p]]))
    xn = xj.copy()
    xn[flipped] *= -1.0
    xi = xj.copy()
    for cols in (plus[:q_plus], minus[:q_minus], plus[p:p + r], minus[p:p + extra + r]):
        xi[cols] *= -1.0
    assert xi.sum() == 0 and xj.sum() == 0 and xn.sum() == 0 and float((xi * (xj - xn)).sum()) == 4.0 * k
    return xi, xj, xn, flipped


def bpr_probe_reference(xi, xj, xn, gamma):
    """fp64: D, softplus(-D), dgamma and dbeta of the probe (w = 1, one negative, grad_out = 1)."""
    xi, xj, xn = (np.asarray(a, np.float64) for a in (xi, xj, xn))
    D = gamma * gamma * float((xi * (xj - xn)).sum())
    loss = max(-D, 0.0) + math.log1p(math.exp(-abs(D)))
    sig = math.exp(-D) / (1.0 + math.exp(-D)) if D >= 0 else 1.0 / (1.0 + math.exp(D))      # sigmoid(-D)
    R = -sig * (xj - xn)
    return D, loss, R * 2.0 * xi * gamma, R * gamma


BPR_SUBNORMAL = 2.0 ** -149


def bpr_relative_error(got, ref):
    """max |got - ref| / |ref| over the elements whose reference is not 0, one subnormal step (2^-149) forgiven where |ref| < 2^-126;
    where the reference is 0 the value must be exactly 0."""
    got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(ref, np.float64))
    nz = ref != 0
    assert np.array_equal(got[~nz], np.zeros((~nz).sum())), "an element whose reference is 0 is not exactly 0"
    if not nz.any():
        return 0.0
    err = np.abs(got[nz] - ref[nz])
    err = np.where(np.abs(ref[nz]) < 2.0 ** -126, np.maximum(err - BPR_SUBNORMAL, 0.0), err)
    return float((err / np.abs(ref[nz])).max())


# ---------------------------------------------------------------------------------------------- BM25: reference, builders and probes
# (shared by tests/test_bm25.py, tests/test_cpu_bm25_reference.py and tests/test_gpu_bm25_edges.py)
def _random_postings(rs, n_docs, n_terms, dense_terms):
    """Term-major postings of a random count matrix: `dense_terms` terms in ~half of the documents, the others with Zipf-like
    document frequencies down to a single posting and a few empty terms."""
    indptr, rows, counts = [0], [], []
    for t in range(n_terms):
        if t < dense_terms:
            df = int(n_docs * rs.uniform(0.3, 0.98))
        elif t % 97 == 5:
            df = 0
        else:
            df = max(1, int(n_docs * 0.2 / (t - dense_terms + 1) ** 1.1))
        r = np.sort(rs.choice(n_docs, df, replace=False)) if df else np.zeros(0, np.int64)
        rows.append(r)
        counts.append(rs.randint(1, 6, df))
        indptr.append(indptr[-1] + df)
    idf = np.log(n_docs / np.maximum(np.diff(indptr), 1).astype(np.float64))
    doc_k = 1.2 * (0.25 + 0.75 * rs.uniform(0.3, 2.5, n_docs))
    return np.asarray(indptr, np.int64), np.concatenate(rows).astype(np.int32), np.concatenate(counts).astype(np.float32), doc_k, idf


BM25_SAMPLE_PIECE = 1024     # csrc/ccr_bm25.hip: documents per sampled piece, one piece out of every BM25_SAMPLE_EVERY
BM25_SAMPLE_EVERY = 64
BM25_LIST_CAP = 16384        # candidate records per row
BM25_SLICE_KINDS = ("0", "1", "step-1", "step", "step+1", "2step", "2step+1", "tile")


def bm25_reference_rows(indptr, rows, counts, doc_k, weights, queries, k1):
    """fp32 [n_q, n_docs]: acc[d] = acc[d] + ((f * w_t) * (k1 + 1)) / (f + doc_k[d]) in numpy fp64, one operation at a time, the query's
    terms in ascending id, then ONE cast to fp32.  (A term's documents are distinct, so the fancy-indexed add is one add per cell.)"""
    doc_k = np.asarray(doc_k, np.float64)
    weights = np.asarray(weights, np.float64)
    out = np.zeros((len(queries), len(doc_k)), np.float32)
    k1p1 = np.float64(k1) + 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        for qi, q in enumerate(queries):
            acc = np.zeros(len(doc_k), np.float64)
            for t in sorted(int(t) for t in q):
                d = rows[indptr[t]:indptr[t + 1]]
                f = counts[indptr[t]:indptr[t + 1]].astype(np.float64)
                numer = (f * weights[t]) * k1p1
                denom = f + doc_k[d]
                acc[d] = acc[d] + numer / denom
            out[qi] = acc.astype(np.float32)
    return out


def bm25_reference_topk(rows_fp32, k):
    """(ids int64 [n_q, k], scores fp32 [n_q, k]) in the total order (score descending, document ascending).  No NaN rows."""
    rows_fp32 = np.atleast_2d(rows_fp32)
    assert not np.isnan(rows_fp32).any(), "rows with NaN are compared between the paths, not with this order"
    ids = np.empty((rows_fp32.shape[0], k), np.int64)
    sc = np.empty((rows_fp32.shape[0], k), np.float32)
    doc = np.arange(rows_fp32.shape[1])
    for r, row in enumerate(rows_fp32):
        o = np.lexsort((doc, -row.astype(np.float64)))[:k]
        ids[r], sc[r] = o, row[o]
    return ids, sc


def _f32_order_key(x):
    """The unsigned key whose order is the order of the floats, -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN (ccr_common.h)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))


def bm25_reference_filter(row_fp32, n_docs, rank, k):
    """What the fused selection must do with one row -> (tau, n, redo): tau = the rank-th largest score of the sampled documents (pieces
    of 1 024 out of every 64 pieces; a piece that reaches beyond the corpus is filled with -inf), n = #{score >= tau and (tau > 0 or
    score > 0)}, redo = (n < k and not (tau <= 0 and no negative / NaN score)) or n > 16 384."""
    row = np.asarray(row_fp32, np.float32)
    assert row.shape == (n_docs,)
    n_all = (n_docs + BM25_SAMPLE_PIECE - 1) // BM25_SAMPLE_PIECE
    assert (n_all + BM25_SAMPLE_EVERY - 1) // BM25_SAMPLE_EVERY * BM25_SAMPLE_PIECE <= 16384, "larger corpora sample more sparsely"
    pieces = []
    for p in range(0, n_all, BM25_SAMPLE_EVERY):
        piece = np.full(BM25_SAMPLE_PIECE, -np.inf, np.float32)
        part = row[p * BM25_SAMPLE_PIECE:(p + 1) * BM25_SAMPLE_PIECE]
        piece[:len(part)] = part
        pieces.append(piece)
    sample = np.concatenate(pieces)
    assert 1 <= rank <= len(sample)
    tau = sample[np.argsort(_f32_order_key(sample), kind="stable")[len(sample) - rank]]
    with np.errstate(invalid="ignore"):
        n = int(((row >= tau) & ((tau > 0) | (row > 0))).sum())
        odd = bool(((row < 0) | np.isnan(row)).any())
        redo = (n < k and not (tau <= 0 and not odd)) or n > BM25_LIST_CAP
    return tau, n, bool(redo)


def bm25_structured_postings(n_docs, tile, step, seed, n_regular=64):
    """A term-major index written around the tile scorer's control flow (tile = documents per tile, step = postings per cursor step).
    Terms, in id order:
      0                      empty
      1 .. n_regular         "regular": the slice of term j in tile i has the length BM25_SLICE_KINDS[(j + 3 i + seed) % 8] (clipped to the
                             tile: 2 step + 1 does not fit a tile of 2 step documents, and the last tile may be short) and lies at the
                             front of the tile, at its end, or scattered, by (j + i) % 3; an empty PAIR sits after the first half of them
      E                      a posting at every multiple of 512 and at every multiple of 512 minus 1 (the run and tile boundaries)
      A                      every document
      L                      `step` consecutive postings: the LAST list of the index, ending exactly at a full step
      last                   empty
    tf is 1 .. 5, on a few postings up to 2^24 (exact in fp32); doc_k is log-uniform over [1e-3, 1e3]; idf is uniform over [0.1, 8), all
    different.  -> (indptr, rows, counts, doc_k, idf); bm25_structured_layout() names the special terms."""
    rs = np.random.RandomState(seed)
    lay = bm25_structured_layout(n_regular)
    lens = {"0": 0, "1": 1, "step-1": step - 1, "step": step, "step+1": step + 1, "2step": 2 * step, "2step+1": 2 * step + 1, "tile": tile}
    n_tiles = (n_docs + tile - 1) // tile
    lists = [np.zeros(0, np.int64) for _ in range(lay["n_terms"])]
    for j, t in enumerate(lay["regular"]):
        parts = []
        for i in range(n_tiles):
            lo, hi = i * tile, min(n_docs, (i + 1) * tile)
            n = min(lens[BM25_SLICE_KINDS[(j + 3 * i + seed) % 8]], hi - lo)
            place = (j + i) % 3
            parts.append(np.arange(lo, lo + n) if place == 0 else np.arange(hi - n, hi) if place == 1 else
                         lo + np.sort(rs.choice(hi - lo, n, replace=False)))
        lists[t] = np.concatenate(parts).astype(np.int64)
    edges = np.arange(0, n_docs + 512, 512)
    e = np.unique(np.concatenate([edges, edges - 1]))
    lists[lay["E"]] = e[(e >= 0) & (e < n_docs)]
    lists[lay["A"]] = np.arange(n_docs)
    full = [i for i in range(n_tiles) if min(n_docs, (i + 1) * tile) - i * tile >= step][-1]      # the last tile that holds a whole step
    lists[lay["L"]] = full * tile + np.arange(step)
    indptr = np.zeros(lay["n_terms"] + 1, np.int64)
    indptr[1:] = np.cumsum([len(x) for x in lists])
    rows = np.concatenate(lists).astype(np.int32)
    counts = rs.randint(1, 6, len(rows)).astype(np.float32)
    big = rs.choice(len(rows), min(40, len(rows)), replace=False)
    counts[big] = np.float32(2.0) ** rs.randint(10, 25, len(big))
    counts[big[0]] = np.float32(2.0 ** 24)
    doc_k = 10.0 ** rs.uniform(-3.0, 3.0, n_docs)
    doc_k[0], doc_k[-1] = 1e-3, 1e3
    idf = rs.uniform(0.1, 8.0, lay["n_terms"])
    return indptr, rows, counts, doc_k, idf


def bm25_structured_layout(n_regular=64):
    """Term ids of bm25_structured_postings: regular (non-empty by construction except where a slice kind says 0), the empty terms and
    the special lists."""
    half = n_regular // 2
    regular = list(range(1, 1 + half)) + list(range(3 + half, 3 + n_regular))
    E = 3 + n_regular
    return dict(regular=regular, empty=[0, 1 + half, 2 + half, E + 3], E=E, A=E + 1, L=E + 2, n_terms=E + 4)


def bm25_slice_lengths(indptr, rows, term, n_docs, tile):
    """Postings of `term` per tile."""
    d = rows[indptr[term]:indptr[term + 1]]
    return np.bincount(d // tile, minlength=(n_docs + tile - 1) // tile)


def bm25_structured_queries(indptr, rows, n_docs, tile, seed, n_regular=64):
    """The query set of the every-document tests: each single term (the empty ones and the every-document term among them), for
    n in 1, 4, 5, 8, 9 and every tile i two queries with exactly n terms active in tile i (plus two that are not), 64 regular terms, an
    empty query, a query of empty terms only."""
    lay = bm25_structured_layout(n_regular)
    rs = np.random.RandomState(seed + 77)
    queries = [np.asarray([t], np.int32) for t in range(lay["n_terms"])]
    reg = np.asarray(lay["regular"])
    per_tile = np.stack([bm25_slice_lengths(indptr, rows, t, n_docs, tile) for t in reg])      # [regular, tiles]
    for i in range(per_tile.shape[1]):
        on, off = reg[per_tile[:, i] > 0], reg[per_tile[:, i] == 0]
        for n in (1, 4, 5, 8, 9):
            for _ in range(2):
                q = np.concatenate([rs.choice(on, n, replace=False), rs.choice(off, min(2, len(off)), replace=False)])
                queries.append(np.sort(q).astype(np.int32))
    queries.append(np.sort(reg[:64]).astype(np.int32))
    queries.append(np.zeros(0, np.int32))
    queries.append(np.asarray(lay["empty"], np.int32))
    return queries


# The exact probes: k1 = 1, tf = 1 and doc_k = 1 make a posting's contribution (1 w)(1 + 1) / (1 + 1) = w, exactly.
BM25_PROBE_DOCS = 4096
BM25_PROBE_TERMS = 260
# (first term, weights in term order, document, fp32 bits the score must have)
BM25_ROUNDING_PROBES = [
    (3, [1.0 + 2.0 ** -24, 2.0 ** -53, 2.0 ** -53], 1024, 0x3F800000),        # ascending ids: each 2^-53 is dropped by a tie to even
    (63, [1.0 + 2.0 ** -24, 2.0 ** -53, 2.0 ** -53], 1535, 0x3F800000),       # .. across the cursor groups 0 | 1
    (191, [1.0 + 2.0 ** -24, 2.0 ** -53, 2.0 ** -53], 1536, 0x3F800000),      # .. across the cursor groups 2 | 3
    (7, [2.0 ** -53, 2.0 ** -53, 1.0 + 2.0 ** -24], 1025, 0x3F800001),        # the reversed ids: 2^-52 survives, fp32 rounds up
    (127, [2.0 ** -53, 2.0 ** -53, 1.0 + 2.0 ** -24], 2047, 0x3F800001),      # .. across the cursor groups 1 | 2
    (195, [2.0 ** -53, 2.0 ** -53, 1.0 + 2.0 ** -24], 1537, 0x3F800001),
    (11, [1.0, 2.0 ** -24, 2.0 ** -50], 1026, 0x3F800001),                    # one rounding: fp32 accumulation gives 0x3F800000
    (15, [1.0, 2.0 ** -24], 1027, 0x3F800000),                                # the tie itself
]
BM25_PROBE_SHARED_DOC = 1500      # holds every term


def bm25_order_probe(seed=0):
    """260 terms over 4 096 documents, tf = 1, doc_k = 1, k1 = 1.  Every term has a posting in document BM25_PROBE_SHARED_DOC and six more
    in tile [1024, 2048) and elsewhere (none in a probe document), with weights in [2^-8, 2^-4); the terms of BM25_ROUNDING_PROBES carry the
    probes' weights instead and meet in the probe's document.  A query of the first n terms puts term i at position i, so the probes sit
    across the fetch groups of four (3|4, 7|8, 11|12, 15|16) and across the cursor groups (63|64, 127|128, 191|192).
    -> (indptr, rows, counts, doc_k, weights)."""
    rs = np.random.RandomState(seed)
    n_docs, n_terms = BM25_PROBE_DOCS, BM25_PROBE_TERMS
    weights = rs.uniform(2.0 ** -8, 2.0 ** -4, n_terms)
    probe_docs = {p[2] for p in BM25_ROUNDING_PROBES}
    free = np.asarray([d for d in range(n_docs) if d not in probe_docs and d != BM25_PROBE_SHARED_DOC])
    in_tile = free[(free >= 1024) & (free < 2048)]
    lists = []
    for t in range(n_terms):
        d = np.concatenate([rs.choice(in_tile, 3, replace=False), rs.choice(free, 3, replace=False), [BM25_PROBE_SHARED_DOC]])
        lists.append(set(int(x) for x in d))
    for first, w, doc, _ in BM25_ROUNDING_PROBES:
        for j, wj in enumerate(w):
            weights[first + j] = wj
            lists[first + j].add(doc)
    lists = [np.asarray(sorted(s), np.int64) for s in lists]
    indptr = np.zeros(n_terms + 1, np.int64)
    indptr[1:] = np.cumsum([len(x) for x in lists])
    rows = np.concatenate(lists).astype(np.int32)
    return indptr, rows, np.ones(len(rows), np.float32), np.ones(n_docs, np.float64), weights


BM25_MASK_EDGE_DOCS = [0, 1, 63, 64, 511, 512, 513, 1023, 1024, 1025, 1535, 1536, 2047, 2048, 2049, 2559, 2560, 3071, 3072, 3073, 4094, 4095]
BM25_MASK_WINDOWS = [0, 24, 40]      # positions [w, w + 24) of a 64-term query: 24 different residues mod 24; lanes 0, 1 and 62, 63 are inside


def bm25_mask_probe(seed=0):
    """The presence mask: 256 terms over 4 096 documents (tf = 1, doc_k = 1, k1 = 1), term t weighs 2^-(t % 24).  Per block of 64 terms a
    document is in a non-empty subset of ONE window of 24 consecutive terms, so the query of that block scores it with the subset's
    bitmask, sum of 2^-(t % 24), exact in fp32: a dropped, doubled or misplaced posting changes named bits.  Documents: the tile and
    run edges plus 300 others.  -> (indptr, rows, counts, doc_k, weights, member [n_docs, 256] bool)."""
    rs = np.random.RandomState(seed + 5)
    n_docs, n_terms = BM25_PROBE_DOCS, 256
    docs = sorted(set(BM25_MASK_EDGE_DOCS) | set(int(d) for d in rs.choice(n_docs, 300, replace=False)))
    member = np.zeros((n_docs, n_terms), bool)
    for n, d in enumerate(docs):
        for g in range(4):
            w = BM25_MASK_WINDOWS[(n + g) % 3]
            sub = rs.rand(24) < 0.5
            sub[rs.randint(24)] = True
            if n % 7 == 0:
                sub[:] = True
            member[d, 64 * g + w:64 * g + w + 24] = sub
    weights = 2.0 ** -(np.arange(n_terms) % 24).astype(np.float64)
    lists = [np.flatnonzero(member[:, t]) for t in range(n_terms)]
    indptr = np.zeros(n_terms + 1, np.int64)
    indptr[1:] = np.cumsum([len(x) for x in lists])
    rows = np.concatenate(lists).astype(np.int32)
    return indptr, rows, np.ones(len(rows), np.float32), np.ones(n_docs, np.float64), weights, member


def bm25_mask_value(member_row, block):
    """The bitmask score of one document under the query of terms [64 block, 64 block + 64)."""
    t = np.flatnonzero(member_row[64 * block:64 * block + 64])
    return np.float32((2.0 ** -((64 * block + t) % 24).astype(np.float64)).sum())


def bm25_postings_from_lists(lists):
    """[(documents, tf)] per term -> (indptr, rows, counts)."""
    indptr = np.zeros(len(lists) + 1, np.int64)
    indptr[1:] = np.cumsum([len(d) for d, _ in lists])
    rows = np.concatenate([np.asarray(d, np.int64) for d, _ in lists]).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    counts = np.concatenate([np.asarray(f, np.float32) for _, f in lists]).astype(np.float32) if indptr[-1] else np.zeros(0, np.float32)
    return indptr, rows, counts


# ------------------------------------------------------------------------------------------------ the exact-score probe of the search
# A corpus of width 8 whose canonical score row is chosen digit by digit (tests/test_cpu_exact_probe.py checks every claim made here
# against the oracle; tests/test_gpu_exact_paths.py searches it).  Row j is sign_j 2^e_j (a_j, b_j, c_j, 0, ..), the query is
# 2^EXACT_PROBE[kind]["query"] on the first three elements: the score is sign 2^(e + q0) (a + b / 256 + c / 65536), a 24-bit number, so
# the fp64 sum and every fp32 partial sum in any order are exact, and the fp32 pattern's bytes are (sign | exponent >> 1), (exponent's
# low bit | a's low seven bits), b, c.  fp16 takes another query and a narrower exponent range: 2^-16 is no normal fp16 number.
EXACT_PROBE = {"bf16": {"query": (0, -8, -16), "e": (-12, 12)}, "fp16": {"query": (8, 0, -8), "e": (-6, 6)}}
EXACT_PROBE_FP16_WIDE_E = (-12, 6)     # 19 exponents (ten values of exponent >> 1): elements from 2^-12 to 255 x 2^6, all normal in fp16


def f32_orderable(x):
    """uint32 keys whose unsigned order is the order of the fp32 values (ccr_common.h: f32_orderable)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def exact_probe_pack(values, kind):
    """fp64 values -> uint16 bit patterns of `kind`; asserts that nothing is lost and, for fp16, that nothing is subnormal."""
    v64 = np.ascontiguousarray(values, np.float64)
    v = v64.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), v64)
    if kind == "fp16":
        h = v.astype(np.float16)
        assert np.array_equal(h.astype(np.float32), v) and np.all((v == 0) | (np.abs(v) >= 2.0 ** -14))
        return h.view(np.uint16)
    u = v.view(np.uint32)
    assert not (u & np.uint32(0xFFFF)).any()
    return (u >> np.uint32(16)).astype(np.uint16)


def exact_probe_draw(n, seed, kind, e_range=None):
    """n rows with every digit drawn uniformly: (sign, e, a, b, c), int64 arrays."""
    rs = np.random.RandomState(seed)
    lo, hi = e_range or EXACT_PROBE[kind]["e"]
    return (rs.choice([-1, 1], n).astype(np.int64), rs.randint(lo, hi + 1, n).astype(np.int64), rs.randint(128, 256, n).astype(np.int64),
            rs.randint(0, 256, n).astype(np.int64), rs.randint(0, 256, n).astype(np.int64))


def exact_probe_fixed(n, sign, e, a, b, c):
    """n rows with the same digits."""
    return tuple(np.full(n, v, np.int64) for v in (sign, e, a, b, c))


def exact_probe_cat(*parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(5))


def exact_probe_take(digits, rows):
    return tuple(d[rows] for d in digits)


def _exact_probe_check(digits, kind, e_range):
    sign, e, a, b, c = digits
    lo, hi = e_range or EXACT_PROBE[kind]["e"]
    assert np.all(np.abs(sign) == 1) and e.min() >= lo and e.max() <= hi
    assert a.min() >= 128 and a.max() <= 255 and min(b.min(), c.min()) >= 0 and max(b.max(), c.max()) <= 255


def exact_probe_rows(digits, kind, dim=8, e_range=None):
    """[n, dim] bit patterns of the probe's corpus rows."""
    _exact_probe_check(digits, kind, e_range)
    sign, e, a, b, c = digits
    rows = np.zeros((len(a), dim), np.float64)
    scale = sign * np.exp2(e.astype(np.float64))
    for col, digit in enumerate((a, b, c)):
        rows[:, col] = scale * digit
    return exact_probe_pack(rows, kind)


def exact_probe_queries(scales, kind, dim=8):
    """[len(scales), dim] bit patterns: the probe's query times each of `scales` (signed powers of two)."""
    scales = np.asarray(scales, np.float64)
    assert np.all(np.exp2(np.round(np.log2(np.abs(scales)))) == np.abs(scales))
    q = np.zeros((len(scales), dim), np.float64)
    for col, p in enumerate(EXACT_PROBE[kind]["query"]):
        q[:, col] = scales * 2.0 ** p
    return exact_probe_pack(q, kind)


def exact_probe_scores(digits, kind):
    """[n] fp32: the score row of the unscaled probe query, from the integers alone (asserted to be exact in fp32)."""
    sign, e, a, b, c = digits
    m = (a << 16) + (b << 8) + c
    assert m.min() >= 1 << 23 and m.max() < 1 << 24
    s = sign * m * np.exp2((e + EXACT_PROBE[kind]["query"][0] - 16).astype(np.float64))
    f = s.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), s)
    return f


def exact_probe_topk(digits, kind, scales, k):
    """(ids [len(scales), k] int64, scores [len(scales), k] fp32) by (score descending, row ascending), in numpy from the integers: a
    positive scale keeps the order of the unscaled row, a negative one ranks by ascending score; the scores scale exactly."""
    base = exact_probe_scores(digits, kind)
    rows = np.arange(len(base))
    order = {1: np.lexsort((rows, -base))[:k], -1: np.lexsort((rows, base))[:k]}
    ids = np.stack([order[1 if s > 0 else -1] for s in scales])
    sc = np.asarray(scales, np.float64)[:, None] * base[ids].astype(np.float64)
    out = sc.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), sc)
    return ids, out
