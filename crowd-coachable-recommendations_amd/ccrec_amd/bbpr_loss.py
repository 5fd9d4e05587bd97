"""The 'multiple_nrl' in-batch-negative objective of src/ccrec/models/bbpr.py:187-214 with the score
GEMMs + softmax-CE in HIP (ccr_inbatch_ce_fwd/bwd).  Embeddings are the three encoder outputs
(query, positive, hard negative); the round-robin negative picking (:188-193) stays host Python."""
import os

import torch

from . import ops


def pick_round_robin_negatives(user_to_negs, users, n_negatives=1):
    """bbpr.py:188-193: pop the front negative of each user and re-append it.  n_negatives = m repeats that pass m times:
    the result is m blocks of len(users) negatives, block k holding every user's k-th pop (a list shorter than m cycles, and
    its duplicates count twice in the loss, as they would in torch)."""
    nj = []
    for _ in range(int(n_negatives)):
        for user in users:
            u = int(user)
            neg = user_to_negs[u].pop(0)
            nj.append(neg)
            user_to_negs[u].append(neg)
    return nj


def multiple_nrl_loss(qid_emb, pos_emb, neg_emb, inv_temperature=None, sim_type=None, weights=None):
    """scores = cat(Q P^T, Q N^T) * inv_temperature; CrossEntropyLoss()(scores, arange(B))  (bbpr.py:205-212).
    cos: rows are L2-normalised first by torch (autograd handles that Jacobian), then the HIP loss.
    neg_emb of B rows and no weights: the square kernels (ops.inbatch_ce), as ever.  neg_emb of m B rows (m hard negatives per
    query; every query sees all of them), or weights [B] (the loss becomes (ce * w).sum() / w.sum(), the weighting of the bpr
    objective, bbpr.py:183-185): the pool is [pos ; neg], the labels arange(B), through ops.pool_ce."""
    if sim_type is None:
        sim_type = os.environ["CCREC_SIM_TYPE"]
    if inv_temperature is None:
        inv_temperature = float(os.environ["CCREC_BBPR_INV_TEMPERATURE"])
    if sim_type == "cos":
        qid_emb = torch.nn.functional.normalize(qid_emb, p=2, dim=1)
        pos_emb = torch.nn.functional.normalize(pos_emb, p=2, dim=1)
        neg_emb = torch.nn.functional.normalize(neg_emb, p=2, dim=1)
    B = qid_emb.shape[0]
    if weights is None and neg_emb.shape[0] == B:
        return ops.inbatch_ce(qid_emb, pos_emb, neg_emb, inv_temperature)
    if pos_emb.shape[0] != B or neg_emb.shape[0] % B != 0 or neg_emb.shape[0] < B:
        raise ValueError(f"multiple_nrl_loss: {B} queries need {B} positives and a multiple of {B} negatives, "
                         f"got {pos_emb.shape[0]} and {neg_emb.shape[0]}")
    labels = torch.arange(B, dtype=torch.int32, device=qid_emb.device)
    return ops.pool_ce(qid_emb, torch.cat([pos_emb, neg_emb]), labels, inv_temperature, weights=weights)


def compute_user_to_negatives(tr_prior_score):
    """bbpr.py:216-227: {user: [hard negatives]} from the sparse prior (entries with value >= 1.0 are negatives; every
    user that appears gets a list)."""
    coo = tr_prior_score.coalesce() if not tr_prior_score.is_coalesced() else tr_prior_score
    users, negs = coo.indices().tolist()
    out = {}
    for u, j, v in zip(users, negs, coo.values().tolist()):
        out.setdefault(u, [])
        if v >= 1.0:
            out[u].append(j)
    return out


class MultipleNrlStep:
    """training_and_validation_step of _BertBPR for objective == "multiple_nrl" (bbpr.py:149-152,187-214) as a callable:
    batch [B,3] = (i, j, w) -> scalar loss with autograd through `forward`.

    forward: item pointer tensor -> embeddings [n, dim] (the item tower on self.all_inputs[ptr] in the reference);
    i_to_ptr / j_to_ptr: user / item index -> item pointer; user_to_negs: round-robin hard-negative lists (mutated)."""

    def __init__(self, forward, i_to_ptr, j_to_ptr, user_to_negs, n_negatives=1, use_weights=False):
        self.forward, self.i_to_ptr, self.j_to_ptr, self.user_to_negs = forward, i_to_ptr, j_to_ptr, user_to_negs
        self.n_negatives, self.use_weights = int(n_negatives), bool(use_weights)
        if self.n_negatives < 1:
            raise ValueError("n_negatives must be at least 1")

    def __call__(self, batch, batch_idx=0):
        i, j, w = batch.T
        i, j = i.to(int), j.to(int)
        with torch.no_grad():
            nj = pick_round_robin_negatives(self.user_to_negs, i, self.n_negatives)
        qid_emb = self.forward(self.i_to_ptr[i.ravel()]).reshape([*i.shape, -1])
        pos_emb = self.forward(self.j_to_ptr[j.ravel()]).reshape([*j.shape, -1])
        neg_emb = self.forward(self.j_to_ptr[nj])
        neg_emb = neg_emb.reshape([self.n_negatives * j.shape[0], *j.shape[1:], -1])   # m blocks of B: block k = every user's k-th negative
        return multiple_nrl_loss(qid_emb, pos_emb, neg_emb, weights=w if self.use_weights else None)

    training_and_validation_step = __call__


class BertMTStep(MultipleNrlStep):
    """training_and_validation_step of _BertMT (src/ccrec/models/bert_mt.py:105-113): the fine-tune loss of the base step
    weighted alpha / ft_cycles; the corpus-tuning (VAE) term is identically zero for contriever models there
    ((1 - alpha) / ct_cycles * 0).  batch = (ijw, inputs) as the reference's CombinedLoader hands it over."""

    def __init__(self, forward, i_to_ptr, j_to_ptr, user_to_negs, alpha=1.0, ct_cycles=1, ft_cycles=1, n_negatives=1, use_weights=False):
        super().__init__(forward, i_to_ptr, j_to_ptr, user_to_negs, n_negatives=n_negatives, use_weights=use_weights)
        self.alpha, self.ct_cycles, self.ft_cycles = float(alpha), ct_cycles, ft_cycles

    def __call__(self, batch, batch_idx=0):
        ijw = batch[0] if isinstance(batch, (tuple, list)) else batch
        ft_loss = super().__call__(ijw, batch_idx)
        return (1 - self.alpha) / self.ct_cycles * 0.0 + self.alpha / self.ft_cycles * ft_loss.mean()

    training_and_validation_step = __call__
