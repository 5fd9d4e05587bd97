"""Host side of the bpr objective, without a GPU: the item proposal, BprStep's constructor, the COO -> CSR form of the prior, the
sizes ccr_bpr_frozen_workspace_bytes reports and the binding's refusal of a library that lacks an entry point."""
import numpy as np
import pytest
import torch


def test_item_proposal_values():
    from ccrec_amd import item_proposal
    freq = np.array([0, 1, 9, 100])
    got = item_proposal(freq)
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), (freq + 0.1) ** 0.5, rtol=1e-15)
    np.testing.assert_allclose(item_proposal(freq, 1.0).numpy(), freq + 0.1, rtol=1e-15)
    np.testing.assert_allclose(item_proposal(torch.tensor([3.0, 0.0]), 0.25).numpy(), np.float32([3.1, 0.1]) ** np.float32(0.25), rtol=1e-6)
    assert torch.equal(item_proposal(freq, 0), torch.ones(4, dtype=torch.float64))


def test_step_defaults_and_refusals():
    from ccrec_amd import BprStep
    fwd = lambda ptr: ptr
    step = BprStep(fwd, [0, 1], [2, 3, 4], np.array([1, 2, 3]))
    assert step.n_negatives == 10 and step.valid_n_negatives == 10 and step.sample_with_prior is True and step.sample_with_posterior == 0.5
    assert step.replacement is True and step.training is True and step.prior_csr is None and step.all_cls is None
    assert step.item_proposal.dtype == torch.float32
    np.testing.assert_allclose(step.item_proposal.numpy(), np.float32((np.array([1, 2, 3]) + 0.1) ** 0.5))
    assert float(step.training_prior_fcn(torch.tensor(1.5))) == 1.5
    assert step.eval().training is False and step.train().training is True
    step = BprStep(fwd, [0], [0], np.ones(1), n_negatives=4, valid_n_negatives=2)
    assert (step.n_negatives, step.valid_n_negatives) == (4, 2)
    with pytest.raises(ValueError, match="replacement"):
        BprStep(fwd, [0], [0], np.ones(1), replacement=False)
    with pytest.raises(ValueError):
        BprStep(fwd, [0], [0], np.ones(1), n_negatives=0)
    with pytest.raises(ValueError):
        BprStep(fwd, [0], [0], np.ones(1), all_cls=torch.zeros(1, 64))      # no layer_norm
    with pytest.raises(ValueError):
        BprStep(None, [0], [0], np.ones(1))


def test_prior_goes_to_csr_once_with_duplicates_summed_and_t0_from_the_function():
    from ccrec_amd import BprStep
    from ccrec_amd.bbpr_loss import prior_to_csr
    # 4 users x 6 items; (2, 1) appears twice (1.0 + 0.5), user 1 has no entry, entries given out of order
    idx = torch.tensor([[2, 0, 2, 3, 2, 0], [1, 5, 4, 0, 1, 2]])
    val = torch.tensor([1.0, 2.0, 3.0, 4.0, 0.5, 6.0])
    prior = torch.sparse_coo_tensor(idx, val, (4, 6))
    fcn = lambda x: 2 * x + 1
    ptr, cols, t, t0, max_row_nnz = prior_to_csr(prior, fcn)
    assert ptr.tolist() == [0, 2, 2, 4, 5] and cols.tolist() == [2, 5, 1, 4, 0] and ptr.dtype == cols.dtype == torch.int64
    assert t.dtype == torch.float32 and t.tolist() == [13.0, 5.0, 4.0, 7.0, 9.0]      # f(1.5) = 4: summed BEFORE the function
    assert t0 == 1.0 and max_row_nnz == 2
    # the CSR rows hold what f(to_dense()) holds, the rest of the dense matrix is t0
    dense = fcn(prior.to_dense())
    for u in range(4):
        row = torch.full((6,), t0)
        row[cols[ptr[u]:ptr[u + 1]]] = t[ptr[u]:ptr[u + 1]]
        assert torch.equal(row, dense[u])
    _, _, t_id, t0_id, _ = prior_to_csr(prior)
    assert t_id.tolist() == [6.0, 2.0, 1.5, 3.0, 4.0] and t0_id == 0.0
    step = BprStep(lambda p: p, [0, 1, 2, 3], list(range(6)), np.ones(6), tr_prior_score=prior, training_prior_fcn=fcn)
    assert step.prior_csr[0].tolist() == [0, 2, 2, 4, 5] and step.prior_csr[3] == 1.0 and step.prior_csr[4] == 2
    assert BprStep(lambda p: p, [0, 1, 2, 3], list(range(6)), np.ones(6), tr_prior_score=prior, sample_with_prior=False).prior_csr is None
    empty = torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.long), torch.zeros(0), (3, 6))
    ptr, cols, t, t0, max_row_nnz = prior_to_csr(empty, fcn)
    assert ptr.tolist() == [0, 0, 0, 0] and cols.numel() == t.numel() == 0 and t0 == 1.0 and max_row_nnz == 0


def test_workspace_sizes_and_range():
    from ccrec_amd import _lib
    lib = _lib.load()
    assert lib.ccr_version() >= _lib.BPR_VERSION == 102
    for name in ("ccr_bpr_sample", "ccr_bpr_frozen_workspace_bytes", "ccr_bpr_frozen_fwd", "ccr_bpr_frozen_bwd_dev"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    # the forward's [B] partial losses or the backward's partial gradient rows ([min(ceil(B / 4), 512)][2][dim] fp32), + alignment slack
    assert lib.ccr_bpr_frozen_workspace_bytes(10000, 10, 768) == 512 * 2 * 768 * 4 + 256
    assert lib.ccr_bpr_frozen_workspace_bytes(1, 1, 64) == 1 * 2 * 64 * 4 + 256
    assert lib.ccr_bpr_frozen_workspace_bytes(1 << 20, 1, 64) == (1 << 20) * 4 + 256
    assert lib.ccr_bpr_frozen_workspace_bytes(64, 10, 2048) == 16 * 2 * 2048 * 4 + 256
    for shape, word in (((8, 2, 72), b"dim"), ((8, 2, 2112), b"beyond the supported range"), ((0, 2, 64), b"B"), ((8, 0, 64), b"n_neg"),
                        (((1 << 20) + 1, 2, 64), b"beyond the supported range"), ((8, 4097, 64), b"beyond the supported range")):
        assert lib.ccr_bpr_frozen_workspace_bytes(*shape) == 0 and word in lib.ccr_last_error(), shape


def test_binding_asks_for_a_rebuild_when_the_library_lacks_an_entry_point(monkeypatch):
    from ccrec_amd import _lib
    lib = _lib.load()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "EXPORTS", _lib.EXPORTS + ["ccr_entry_point_of_a_later_version"])
    with pytest.raises(_lib.CcrError, match="lacks ccr_entry_point_of_a_later_version.*rebuild"):
        _lib.load()
    monkeypatch.undo()
    assert _lib.load() is lib
