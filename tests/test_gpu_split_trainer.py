"""Trainer.set_split_precision on the two miniatures of tests/test_gpu_trainer.py: one step within the fp32 bars of
the reference interpreter + CTC oracle, NOT bit-equal to the fp32 step (the split kernel ran), the mode kept across a re-plan, the
fp32 bits again after switching off, and the two refusals next to the mixed-precision mode."""
import numpy as np
import pytest
import torch

from tests.test_gpu_trainer import TOL, build, check_grads, rel
from wav2letter_amd import recipes

pytestmark = pytest.mark.gpu
CASES = {"tds": (recipes.tds_ctc_small_arch(c=(4, 6), h=8, kw=5), 8, 21, 3, 64, 6),
         "transformer": ("V -1 1 NFEAT 0\nWN 3 C NFEAT 64 3 1 -1\nGLU 2\nDO 0.0\nM 1 1 2 1\nRO 2 0 3 1\n"
                         "TR 32 64 4 5 0.0 0.0\nTR 32 64 4 5 0.0 0.0\nDO 0.0\nL 32 NLABEL\n", 16, 12, 3, 44, 4)}


@pytest.mark.parametrize("kind", list(CASES))
def test_one_step_in_split_precision(oracle, kind):
    (arch, nfeat, nlabel, B, T, L), rng = CASES[kind], np.random.default_rng(17)
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)
    xd, td = torch.tensor(x.reshape(B, nfeat, T)).cuda(), torch.tensor(tgt).cuda()
    step = lambda: (tr.forward(xd, train=False).clone(), tr.forward_backward(xd, td).clone(), tr.grads.clone())
    same = lambda p, q: all(torch.equal(a, b) for a, b in zip(p, q))
    f32 = step()
    tr.set_split_precision(True)
    with pytest.raises(ValueError):
        tr.set_mixed_precision(True)
    em, loss, grads = step()
    assert not torch.equal(em, f32[0]) and not torch.equal(grads, f32[2])       # the split kernel ran, forward and backward
    em_ref = ref.forward(x, params)
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(em.cpu().numpy(), em_ref) < TOL and rel(loss.cpu().numpy(), o.forward()) < TOL
    want = ref.backward(o.backward().astype(np.float32), len(params))
    for i, (name, _n, _off) in enumerate(tr.param_table()):
        if name == "tr.wk.b":
            want[i] = None      # exactly zero in theory, rounding noise on both sides (tests/test_gpu_trainer.py)
    check_grads(tr, want)
    tr.plan(B - 1, T - 8, L), tr.plan(B, T, L)   # a re-plan keeps the mode: the same step after another shape was planned in between
    assert same(step(), (em, loss, grads))
    tr.set_split_precision(False)
    assert same(step(), f32)                                                    # the fp32 step's bits again
    tr.set_mixed_precision(True)
    with pytest.raises(ValueError):
        tr.set_split_precision(True)
