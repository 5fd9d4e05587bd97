"""The 16-bit weight set that optim.FusedAdamW(shadow_for=...) keeps current for FusedBertEncoder: a fine-tune step that reads it gives the
bits of the step that casts the fp32 masters in every forward; nothing ever reads a stale copy.

The towers are the 2-layer tiny BERT / DistilBERT of test_gpu_encoder_train.py (rebuilt here), on the kernels' training path
(CCREC_FUSED_ENCODER_TRAIN=1, under autocast) in bf16 and fp16.  Everything is compared bit for bit: the maintained copies hold exactly what
the cast would produce, so the forwards compute on identical operands."""
import contextlib

import pytest
import torch

from conftest import ROOT, PKG  # noqa: F401

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
STACK_LENS = [1, 70, 17, 33, 64, 65, 9, 40, 2]
LR = 1e-3


def _tiny_model(kind, dropout=0.0, seed=0):
    torch.manual_seed(seed)
    if kind == "bert":
        from transformers import BertConfig, BertModel
        m = BertModel(BertConfig(vocab_size=600, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                                 max_position_embeddings=128, hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout))
        attn = [(l.attention.self.query, l.attention.self.key) for l in m.encoder.layer]
    else:
        from transformers import DistilBertConfig, DistilBertModel
        m = DistilBertModel(DistilBertConfig(vocab_size=600, dim=256, n_layers=2, n_heads=4, hidden_dim=512, max_position_embeddings=128,
                                             dropout=dropout, attention_dropout=dropout))
        attn = [(l.attention.q_lin, l.attention.k_lin) for l in m.transformer.layer]
    with torch.no_grad():      # the default init (std 0.02) leaves every softmax uniform: widen the attention projections
        for q, k in attn:
            q.weight.mul_(20.0)
            k.weight.mul_(20.0)
    return m.cuda()


def _tower(kind, dropout=0.0):
    from ccrec_amd.item_tower import NaiveItemTower
    return NaiveItemTower(_tiny_model(kind, dropout), torch.nn.LayerNorm(256, elementwise_affine=False)).cuda().train()


def _batch():
    g = torch.Generator().manual_seed(11)
    L = max(STACK_LENS)
    ids = torch.zeros(len(STACK_LENS), L, dtype=torch.int64)
    mask = torch.zeros(len(STACK_LENS), L, dtype=torch.int64)
    for r, n in enumerate(STACK_LENS):
        ids[r, :n] = torch.randint(1, 600, (n,), generator=g)
        mask[r, :n] = 1
    return ids.cuda(), mask.cuda()


def _step_loss(tower, ids, mask, dtype):
    """One MultipleNrlStep loss: three tower forwards with gradients on (queries, positives, hard negatives) over the nine texts."""
    from ccrec_amd.bbpr_loss import MultipleNrlStep

    def forward(ptr):
        ptr = torch.as_tensor(ptr, device=ids.device)
        return tower(input_ids=ids[ptr], attention_mask=mask[ptr], input_step="inputs", output_step="mean_pooling")

    step = MultipleNrlStep(forward, torch.tensor([0, 1, 2]), torch.arange(9), {0: [6, 7], 1: [7, 8], 2: [8, 6]})
    batch = torch.tensor([[0, 3, 1.0], [1, 4, 1.0], [2, 5, 1.0]])
    with torch.autocast("cuda", dtype=dtype):
        return step(batch)


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _loss_and_grads(tower, ids, mask, dtype, seed=None):
    tower.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    loss = _step_loss(tower, ids, mask, dtype)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in tower.named_parameters() if p.grad is not None}


def _same_step(a, b, what):
    (loss_a, grads_a), (loss_b, grads_b) = a, b
    assert torch.equal(_bits(loss_a), _bits(loss_b)), (what, loss_a.item(), loss_b.item())
    assert set(grads_a) == set(grads_b) and grads_a
    for name in grads_a:
        assert torch.equal(_bits(grads_a[name]), _bits(grads_b[name])), (what, name)


@contextlib.contextmanager
def _watch_weight_source(enc):
    """Records, per training forward of `enc`, whether it read the maintained set (True) or cast the masters (False)."""
    seen, real = [], enc._train_weights
    enc._train_weights = lambda *args: (lambda kept: (seen.append(kept is not None), kept)[1])(real(*args))
    try:
        yield seen
    finally:
        del enc._train_weights


@pytest.fixture
def train_env(monkeypatch):
    monkeypatch.setenv("CCREC_SIM_TYPE", "cos")
    monkeypatch.setenv("CCREC_BBPR_INV_TEMPERATURE", "20")
    monkeypatch.setenv("CCREC_FUSED_ENCODER_TRAIN", "1")
    return monkeypatch


def _pair(kind, dtype, dropout=0.0):
    """Two identical towers: one whose optimizer maintains the weight set, one whose optimizer does not (every forward casts)."""
    from ccrec_amd import fused_bert, optim
    kept, cast = _tower(kind, dropout), _tower(kind, dropout)
    for p, q in zip(kept.parameters(), cast.parameters()):
        assert torch.equal(p, q)
    opt_kept = optim.FusedAdamW(kept.parameters(), lr=LR, weight_decay=0.01, shadow_for=kept, shadow_dtype=dtype)
    opt_cast = optim.FusedAdamW(cast.parameters(), lr=LR, weight_decay=0.01)
    enc = fused_bert.for_model(kept.cls_model)
    assert enc is not None and enc.adopted_current(dtype) and fused_bert.for_model(cast.cls_model)._adopted is None
    return kept, cast, opt_kept, opt_cast, enc


def _fresh_copy(kind, tower, dropout=0.0):
    """A tower with the same masters and no maintained set: the cast path's answer for the weights as they are now."""
    other = _tower(kind, dropout)
    other.load_state_dict(tower.state_dict())
    return other


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["bert", "distilbert"])
def test_three_steps_on_the_maintained_set_equal_three_steps_on_the_cast_path(kind, dtype, train_env):
    """Loss and every parameter gradient of every step, and the final masters, bit for bit; after each step the set is current (refresh
    finds nothing to do), holds what _build_layers would build, and an inference forward in eval() matches a fresh encoder's."""
    from ccrec_amd import fused_bert
    kept, cast, opt_kept, opt_cast, enc = _pair(kind, dtype)
    ids, mask = _batch()
    lengths = mask.sum(1).to(torch.int32)
    with _watch_weight_source(enc) as seen:
        for step in range(3):
            _same_step(_loss_and_grads(kept, ids, mask, dtype), _loss_and_grads(cast, ids, mask, dtype), f"step {step}")
            opt_kept.step()
            opt_cast.step()
            assert enc.refresh(dtype) is False and enc.adopted_current(dtype)
            fresh = enc._build_layers(dtype)
            for mine, want in zip(enc._layers[dtype], fresh):
                for name in fused_bert._LAYER_16BIT:
                    assert torch.equal(_bits(getattr(mine, name)), _bits(getattr(want, name))), (step, name)
                for name in ("g1", "b1", "g2", "b2"):
                    assert torch.equal(getattr(mine, name), getattr(want, name)), (step, name)
        assert seen == [True] * 9      # three forwards per step, all on the maintained set
    for (name, p), q in zip(kept.named_parameters(), cast.parameters()):
        assert torch.equal(_bits(p), _bits(q)), name
    kept.eval()
    out = enc.forward(ids, lengths, dtype=dtype)
    assert enc._layers[dtype] is enc._adopted[1]      # the ranking step's forward reused the set: no rebuild
    want = fused_bert.FusedBertEncoder(kept.cls_model).forward(ids, lengths, dtype=dtype)
    assert torch.equal(_bits(out), _bits(want))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("how", ["load_state_dict", "inplace_add", "sgd_step"])
def test_a_stale_set_is_never_read(how, dtype, train_env):
    """After one maintained step the parameters change behind the optimizer's back: the next training forward casts the masters (the loss
    has the cast path's bits) and rebuilds the set, the one after reads the set again, and the next step keeps it current.

    The in-place change is made under torch.no_grad(), which autograd's version counter records.  A write through p.data is one that torch
    itself hides from that counter (p.data.add_() leaves p._version where it was), so neither this set nor the 16-bit copies refresh() has
    always kept can notice it: DESIGN 4.8o says what to do after such a write."""
    kind = "bert"
    kept, cast, opt_kept, opt_cast, enc = _pair(kind, dtype)
    ids, mask = _batch()
    _loss_and_grads(kept, ids, mask, dtype)
    opt_kept.step()
    assert enc.adopted_current(dtype)
    if how == "load_state_dict":
        other = _tower(kind)
        with torch.no_grad():
            for p in other.parameters():
                p.mul_(1.01)
        kept.load_state_dict(other.state_dict())
    elif how == "inplace_add":
        with torch.no_grad():
            for p in kept.parameters():
                p.add_(0.003)
    else:
        torch.optim.SGD(kept.parameters(), lr=0.05).step()      # on the gradients of the step above
    assert not enc.adopted_current(dtype)
    want = _loss_and_grads(_fresh_copy(kind, kept), ids, mask, dtype)
    with _watch_weight_source(enc) as seen:
        got = _loss_and_grads(kept, ids, mask, dtype)
        assert seen == [False, True, True]      # the first forward of the step found it stale, cast, and rebuilt it for the others
        _same_step(got, want, how)
        assert enc.adopted_current(dtype)
        _same_step(_loss_and_grads(kept, ids, mask, dtype), want, how + ", again")
        assert seen[3:] == [True] * 3
    opt_kept.step()
    assert enc.adopted_current(dtype) and enc.refresh(dtype) is False
    _same_step(_loss_and_grads(kept, ids, mask, dtype), _loss_and_grads(_fresh_copy(kind, kept), ids, mask, dtype), how + ", after the next step")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_step_without_a_forward_after_an_outside_change_rebuilds_the_set(dtype, train_env):
    """The optimizer steps on a set that was already stale (parameters moved by hand, no forward since): parameters without a gradient would
    keep old copies, so the whole set is rebuilt from the masters."""
    kind = "distilbert"
    kept, cast, opt_kept, opt_cast, enc = _pair(kind, dtype)
    ids, mask = _batch()
    _loss_and_grads(kept, ids, mask, dtype)
    with torch.no_grad():
        for p in kept.parameters():
            p.mul_(0.99)
    opt_kept.step()
    assert enc.adopted_current(dtype)
    _same_step(_loss_and_grads(kept, ids, mask, dtype), _loss_and_grads(_fresh_copy(kind, kept), ids, mask, dtype), "stale at step()")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_other_16_bit_type_casts_and_its_copies_are_dropped_at_step(dtype, train_env):
    from ccrec_amd import fused_bert
    kind = "bert"
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    kept, cast, opt_kept, opt_cast, enc = _pair(kind, dtype)
    ids, mask = _batch()
    lengths = mask.sum(1).to(torch.int32)
    _loss_and_grads(kept, ids, mask, dtype)
    opt_kept.step()
    kept.eval()
    out = enc.forward(ids, lengths, dtype=other)      # a ranking forward in the other type builds that type's inference copies
    assert other in enc._layers and dtype in enc._layers
    assert torch.equal(_bits(out), _bits(fused_bert.FusedBertEncoder(kept.cls_model).forward(ids, lengths, dtype=other)))
    kept.train()
    with _watch_weight_source(enc) as seen:      # a training forward in the other type: the cast path, correct
        _same_step(_loss_and_grads(kept, ids, mask, other), _loss_and_grads(_fresh_copy(kind, kept), ids, mask, other), "other type")
        assert seen == [False] * 3
    assert enc.adopted_current(dtype)
    opt_kept.step()
    assert other not in enc._layers and enc.adopted_current(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["bert", "distilbert"])
def test_dropout_steps_agree_with_and_without_the_maintained_set(kind, dtype, train_env):
    """CCREC_FUSED_ENCODER_TRAIN_DROPOUT=1, dropout 0.1, the same torch.manual_seed in front of each step: the same keep bits, the same
    loss and gradients on both weight sources, over two steps."""
    train_env.setenv("CCREC_FUSED_ENCODER_TRAIN_DROPOUT", "1")
    kept, cast, opt_kept, opt_cast, enc = _pair(kind, dtype, dropout=0.1)
    ids, mask = _batch()
    with _watch_weight_source(enc) as seen:
        for step in range(2):
            a = _loss_and_grads(kept, ids, mask, dtype, seed=40 + step)
            seed_kept = enc.last_seed
            b = _loss_and_grads(cast, ids, mask, dtype, seed=40 + step)
            assert seed_kept is not None
            _same_step(a, b, f"dropout step {step}")
            opt_kept.step()
            opt_cast.step()
        assert seen == [True] * 6
    no_drop = _loss_and_grads(kept.eval(), ids, mask, dtype)[0]
    kept.train()
    assert not torch.equal(_bits(no_drop), _bits(_loss_and_grads(kept, ids, mask, dtype, seed=40)[0]))      # (dropout was live)
