"""The 'multiple_nrl' in-batch-negative objective of src/ccrec/models/bbpr.py:187-214 with the score
GEMMs + softmax-CE in HIP (ccr_inbatch_ce_fwd/bwd).  Embeddings are the three encoder outputs
(query, positive, hard negative); the round-robin negative picking (:188-193) stays host Python.
The 'bpr' objective of bbpr.py:153-185 (BprStep): prior-guided negative sampling in HIP (ccr_bpr_sample) and, when the
encoder is frozen and the CLS rows are cached, the whole loss in HIP (ccr_bpr_frozen_*)."""
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
    i_to_ptr / j_to_ptr: user / item index -> item pointer; user_to_negs: round-robin hard-negative lists (mutated).

    one_pass (default False): the reference calls the tower three times (bbpr.py:195-197: queries, positives, negatives), and so does
    this step.  With one_pass=True it calls `forward` ONCE on cat(i_to_ptr[i], j_to_ptr[j], j_to_ptr[nj]) and splits the rows into the
    three blocks: one encoder forward and one backward per step instead of three.  Every operation of the tower is row-wise or
    per-sequence, so without dropout the two differ only by what the projection GEMMs do at another row count (a pure table lookup gives
    the same bits).  Under live dropout on the kernels' training path the one-pass step draws ONE seed where the three-pass step draws
    three; keep bits are a function of (seed, stream, row), so the rows of the one call still get independent masks."""

    def __init__(self, forward, i_to_ptr, j_to_ptr, user_to_negs, n_negatives=1, use_weights=False, one_pass=False):
        self.forward, self.i_to_ptr, self.j_to_ptr, self.user_to_negs = forward, i_to_ptr, j_to_ptr, user_to_negs
        self.n_negatives, self.use_weights, self.one_pass = int(n_negatives), bool(use_weights), bool(one_pass)
        if self.n_negatives < 1:
            raise ValueError("n_negatives must be at least 1")

    def _encode_one_pass(self, i, j, nj):
        ptr_i, ptr_j = torch.as_tensor(self.i_to_ptr[i.ravel()]), torch.as_tensor(self.j_to_ptr[j.ravel()])
        ptr_n = torch.as_tensor(self.j_to_ptr[nj])
        emb = self.forward(torch.cat([ptr_i.ravel(), ptr_j.ravel(), ptr_n.ravel()]))
        n_i, n_j = ptr_i.numel(), ptr_j.numel()
        return emb[:n_i], emb[n_i:n_i + n_j], emb[n_i + n_j:]

    def __call__(self, batch, batch_idx=0):
        i, j, w = batch.T
        i, j = i.to(int), j.to(int)
        with torch.no_grad():
            nj = pick_round_robin_negatives(self.user_to_negs, i, self.n_negatives)
        if self.one_pass:
            qid_emb, pos_emb, neg_emb = self._encode_one_pass(i, j, nj)
            qid_emb, pos_emb = qid_emb.reshape([*i.shape, -1]), pos_emb.reshape([*j.shape, -1])
        else:
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

    def __init__(self, forward, i_to_ptr, j_to_ptr, user_to_negs, alpha=1.0, ct_cycles=1, ft_cycles=1, n_negatives=1, use_weights=False,
                 one_pass=False):
        super().__init__(forward, i_to_ptr, j_to_ptr, user_to_negs, n_negatives=n_negatives, use_weights=use_weights, one_pass=one_pass)
        self.alpha, self.ct_cycles, self.ft_cycles = float(alpha), ct_cycles, ft_cycles

    def __call__(self, batch, batch_idx=0):
        ijw = batch[0] if isinstance(batch, (tuple, list)) else batch
        ft_loss = super().__call__(ijw, batch_idx)
        return (1 - self.alpha) / self.ct_cycles * 0.0 + self.alpha / self.ft_cycles * ft_loss.mean()

    training_and_validation_step = __call__


def item_proposal(item_freq, sample_with_posterior=0.5):
    """bbpr.py:119: (item_freq + 0.1) ** sample_with_posterior, the proposal the negatives are drawn from."""
    freq = torch.as_tensor(item_freq)
    if not freq.is_floating_point():
        freq = freq.to(torch.float64)   # (numpy's int + 0.1)
    return (freq + 0.1) ** sample_with_posterior


def prior_to_csr(tr_prior_score, training_prior_fcn=None):
    """Sparse prior [n_users, n_items] (torch COO, as compute_user_to_negatives takes it; duplicate entries are summed, as
    to_dense() would) -> (ptr [n_users + 1] int64, idx int64 ascending per row, t fp32, t0, max_row_nnz): the CSR form
    ops.bpr_sample_negatives takes, with training_prior_fcn applied ONCE, to the stored values and to a zero (t0, the value of
    every absent entry after to_dense()).  That is the reference's f(dense matrix) only for an ELEMENTWISE function."""
    coo = tr_prior_score.coalesce()   # sorted by (row, column), duplicates summed
    rows, cols = coo.indices()
    vals = coo.values()
    n_users = coo.shape[0]
    counts = torch.bincount(rows, minlength=n_users)
    ptr = torch.zeros(n_users + 1, dtype=torch.int64, device=rows.device)
    ptr[1:] = torch.cumsum(counts, 0)
    fcn = training_prior_fcn if training_prior_fcn is not None else (lambda x: x)
    t = torch.as_tensor(fcn(vals)).to(torch.float32).contiguous()
    t0 = float(fcn(torch.zeros((), dtype=vals.dtype, device=vals.device)))
    return ptr, cols.contiguous(), t, t0, (int(counts.max()) if vals.numel() else 0)


class BprStep:
    """training_and_validation_step of _BertBPR for objective == "bpr" (bbpr.py:149-185) as a callable:
    batch [B,3] = (i, j, w) -> scalar loss  (-logsigmoid(pos - neg) * w).sum() / (n_negatives * w.sum()).

    Negatives: n_negatives per row (valid_n_negatives when .training is False) from softmax(training_prior_fcn(prior[i]) +
    log item_proposal) when tr_prior_score is given and sample_with_prior, from item_proposal alone otherwise -- always through
    ops.bpr_sample_negatives, never a dense [B, n_items] matrix.  The prior is turned into device CSR once (prior_to_csr):
    training_prior_fcn must be ELEMENTWISE (it sees the stored values and one zero, not the dense matrix).  With replacement only.
    all_cls [n_rows, dim] fp32 + layer_norm (the tower's torch.nn.LayerNorm; freeze_bert > 0, bbpr.py:436-438): the loss is
    ops.bpr_frozen_loss, with gradients into the LayerNorm; at a width the kernel does not take (not a multiple of 64, above 2048)
    the same expression in torch.  Otherwise forward(item pointers) -> embeddings [n, dim] with autograd (the item tower on
    all_inputs[ptr]) and _pairwise is torch products + logsigmoid, as in the reference.
    i_to_ptr / j_to_ptr: user / item index -> item pointer.  The last draw stays in .last_negatives [n_negatives, B]."""

    def __init__(self, forward, i_to_ptr, j_to_ptr, item_freq, tr_prior_score=None, training_prior_fcn=None, n_negatives=10,
                 valid_n_negatives=None, sample_with_prior=True, sample_with_posterior=0.5, replacement=True, all_cls=None,
                 layer_norm=None, generator=None):
        if not replacement:
            raise ValueError("BprStep: replacement=False (sampling without replacement) is not supported")
        if (all_cls is None) != (layer_norm is None):
            raise ValueError("BprStep: all_cls and layer_norm go together")
        if forward is None and all_cls is None:
            raise ValueError("BprStep: needs forward, or all_cls and layer_norm")
        self.n_negatives = int(n_negatives)
        self.valid_n_negatives = self.n_negatives if valid_n_negatives is None else int(valid_n_negatives)
        if self.n_negatives < 1 or self.valid_n_negatives < 1:
            raise ValueError("n_negatives must be at least 1")
        self.forward, self.all_cls, self.layer_norm = forward, all_cls, layer_norm
        self.i_to_ptr, self.j_to_ptr = torch.as_tensor(i_to_ptr), torch.as_tensor(j_to_ptr)
        self.sample_with_prior, self.sample_with_posterior, self.replacement = bool(sample_with_prior), sample_with_posterior, True
        self.training_prior_fcn = training_prior_fcn if training_prior_fcn is not None else (lambda x: x)
        self.training, self.generator, self.last_negatives = True, generator, None
        self.item_proposal = item_proposal(item_freq, sample_with_posterior).to(torch.float32).contiguous()
        self.prior_csr = None   # (ptr, idx, t, t0, max_row_nnz)
        if tr_prior_score is not None and self.sample_with_prior:
            self.prior_csr = prior_to_csr(tr_prior_score, self.training_prior_fcn)
            assert tr_prior_score.shape[1] == self.item_proposal.numel(), "the prior's columns are the items of item_freq"
        self._dev = {}   # device -> (i_to_ptr, j_to_ptr, proposal, proposal_cdf, prior)

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def _on_device(self, dev):
        st = self._dev.get(dev)
        if st is None:
            proposal = self.item_proposal.to(dev)
            prior = None
            if self.prior_csr is not None:
                ptr, idx, t, _, max_row_nnz = self.prior_csr
                prior = (ptr.to(dev), idx.to(dev), t.to(dev), max_row_nnz)
            st = self._dev[dev] = (self.i_to_ptr.to(dev), self.j_to_ptr.to(dev), proposal, ops.bpr_proposal_cdf(proposal), prior)
        return st

    def sample_negatives(self, i, n_negatives):
        """[n_negatives, B] item indices for the users i (bbpr.py:160-179)."""
        _, _, proposal, cdf, prior = self._on_device(i.device)
        return ops.bpr_sample_negatives(i, n_negatives, proposal, cdf, prior=prior, t0=self.prior_csr[3] if prior is not None else 0.0,
                                        generator=self.generator)

    def _embed(self, ptr):
        if self.all_cls is not None:   # forward of bbpr.py:134-137 on the cached rows
            return self.layer_norm(self.all_cls[ptr])
        return self.forward(ptr)

    def _pairwise(self, i, j):   # auto-broadcast on first dimension (bbpr.py:144-147)
        i_to_ptr, j_to_ptr = self._on_device(i.device)[:2]
        x = self._embed(i_to_ptr[i.ravel()]).reshape([*i.shape, -1])
        y = self._embed(j_to_ptr[j.ravel()]).reshape([*j.shape, -1])
        return (x * y).sum(-1)

    def __call__(self, batch, batch_idx=0):
        i, j, w = batch.T
        i, j = i.to(int), j.to(int)
        n_negatives = self.n_negatives if self.training else self.valid_n_negatives
        with torch.no_grad():
            nj = self.last_negatives = self.sample_negatives(i, n_negatives)
        if self.all_cls is not None and ops.bpr_frozen_supported(self.all_cls.shape[1]):
            i_to_ptr, j_to_ptr = self._on_device(i.device)[:2]
            ln = self.layer_norm
            return ops.bpr_frozen_loss(self.all_cls, ln.weight, ln.bias, ln.eps, i_to_ptr[i], j_to_ptr[j], j_to_ptr[nj], w)
        loglik = torch.nn.functional.logsigmoid(self._pairwise(i, j) - self._pairwise(i, nj))   # n_negatives x B
        return (-loglik * w).sum() / (n_negatives * w.sum())

    training_and_validation_step = __call__
