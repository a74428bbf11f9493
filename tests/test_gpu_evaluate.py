"""Trainer.evaluate (w2l_trainer_evaluate): an eval-mode forward and the criterion's loss and Viterbi path in one call, equal to
forward(train=False) + the criterion + viterbi, and invisible to the training run around it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _make(arch, nfeat, nlabel, crit, mode, transdiag, B, T, Lt, seed=0):
    from wav2letter_amd.trainer import Trainer
    tr = Trainer(arch, nfeat, nlabel, crit, mode, transdiag)
    tr.init_params(seed)
    if crit == "asg":
        rng = np.random.default_rng(seed)
        A = (np.eye(nlabel) * transdiag + 0.1 * rng.normal(size=(nlabel, nlabel))).astype(np.float32)
        tr.host_params[tr.n_net:tr.n_net + nlabel * nlabel] = A.reshape(-1)
    tr.plan(B, T, Lt)
    tr.to_device()
    return tr


def _batch(rng, B, nfeat, T, Lt, nlabel, blank_last=True):
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32), device="cuda")
    tgt = np.full((B, Lt), -1, np.int32)
    for b in range(B):
        n = int(rng.integers(1, Lt + 1))
        tgt[b, :n] = rng.integers(0, nlabel - 1 if blank_last else nlabel, n)
    return x, torch.tensor(tgt, device="cuda")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("crit", ["ctc", "asg"])
def test_evaluate_equals_eval_forward_criterion_and_viterbi(crit):
    from wav2letter_amd import _lib, recipes
    from wav2letter_amd.criterion import CTCLoss
    rng = np.random.default_rng(1)
    nfeat, nlabel, B, T, Lt = 8, 21, 3, 64, 6
    arch = recipes.tds_ctc_small_arch(c=(4, 6), h=nfeat, kw=5, drop=0.2)
    tr = _make(arch, nfeat, nlabel, crit, 4, 2.0, B, T, Lt)
    x, tgt = _batch(rng, B, nfeat, T, Lt, nlabel)
    loss, path = tr.evaluate(x, tgt)
    loss, path = loss.clone(), path.clone()
    em = tr.forward(x, train=False).clone()
    if crit == "ctc":
        want_loss = CTCLoss(4)(em, tgt).detach()
    else:
        L = _lib.lib()
        N = nlabel
        trans = tr.params[tr.n_net:tr.n_net + N * N].contiguous()
        ws = torch.empty(L.w2l_asg_workspace_size(B, tr.Tout, N, Lt), dtype=torch.uint8, device="cuda")
        want_loss = torch.empty(B, device="cuda")
        _lib.check(L.w2l_asg_forward(B, tr.Tout, N, Lt, 4, em.data_ptr(), tgt.data_ptr(), trans.data_ptr(), want_loss.data_ptr(),
                                     ws.data_ptr(), torch.cuda.current_stream().cuda_stream), "asg forward")
    want_path = tr.viterbi(em)
    torch.cuda.synchronize()
    assert loss.shape == (B,) and path.shape == (B, tr.Tout)
    assert torch.isfinite(loss).all()
    assert torch.equal(_bits(loss), _bits(want_loss)), (loss, want_loss)
    assert torch.equal(path.cpu(), want_path.cpu())


@pytest.mark.parametrize("crit", ["ctc", "asg"])
def test_evaluate_between_steps_leaves_training_bit_identical(crit):
    """dropout on (network and TDS blocks): a run that evaluates a batch of ANOTHER shape between every step holds the same
    parameters and losses, bit for bit, as one that never evaluates"""
    from wav2letter_amd import recipes
    nfeat, nlabel, B, T, Lt = 8, 21, 3, 64, 6
    arch = recipes.tds_ctc_small_arch(c=(4, 6), h=nfeat, kw=5, drop=0.3)

    def run(evaluate):
        rng = np.random.default_rng(7)
        tr = _make(arch, nfeat, nlabel, crit, 4, 2.0, B, T, Lt)
        vx, vt = _batch(np.random.default_rng(99), 5, nfeat, 48, 9, nlabel)
        losses, evals = [], []
        for _ in range(4):
            x, tgt = _batch(rng, B, nfeat, T, Lt, nlabel)
            if evaluate:
                evals.append(tr.evaluate(vx, vt)[0].clone())
            losses.append(tr.forward_backward(x, tgt).clone())
            tr.update(lr=0.1, lrcrit=0.01, momentum=0.5, max_grad_norm=1.0)
        torch.cuda.synchronize()
        return [_bits(l) for l in losses], tr.params.cpu(), evals

    l0, p0, _ = run(False)
    l1, p1, ev = run(True)
    for a, b in zip(l0, l1):
        assert torch.equal(a, b)
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))
    assert all(torch.isfinite(e).all() for e in ev)
    assert not torch.equal(ev[0], ev[-1])   # the evaluations saw the parameters move
