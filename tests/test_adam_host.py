"""Adam without a GPU: the float64 restatement (tests/adam_ref.py) against torch.optim and the contract's closed form, the refusals
of w2l_adam_step_guarded, and the Python trainer's optimizer table and checkpoint header."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as R
from wav2letter_amd import _lib

N, STEPS, LR, B1, B2 = 257, 6, 0.01, 0.9, 0.999


@pytest.fixture(scope="module")
def problem():
    g = torch.Generator().manual_seed(11)
    p0 = torch.randn(N, generator=g, dtype=torch.float64)
    grads = [torch.randn(N, generator=g, dtype=torch.float64) for _ in range(STEPS)]
    assert all((gi != 0).all() for gi in grads)        # so that v > 0 and eps = 0 divides by something
    return p0, grads


def torch_run(cls, p0, grads, **kw):
    ref = p0.clone().requires_grad_(True)
    opt = cls([ref], lr=LR, betas=(B1, B2), **kw)
    out = []
    for gi in grads:
        ref.grad = gi.clone()
        opt.step()
        out.append(ref.detach().clone().numpy())
    return out


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_restatement_is_adamw_when_eps_is_zero(problem, wd):
    """with eps = 0 the placement of eps is moot and the decay step is torch.optim.AdamW's: the same arithmetic, 1e-12 relative"""
    p0, grads = problem
    want = torch_run(torch.optim.AdamW, p0, grads, eps=0.0, weight_decay=wd)
    got = R.run(p0.numpy(), [g.numpy() for g in grads], LR, B1, B2, 0.0, wd)
    for t in range(STEPS):
        err = np.abs(got[t][0] - want[t]).max() / np.abs(want[t]).max()
        assert err < 1e-12, (t, err)
        assert got[t][3] == t + 1


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_eps_sits_outside_the_bias_correction(problem, wd):
    """at eps = 1e-3 the restatement is NOT torch.optim.Adam (sqrt(v) / sqrt(1 - beta2^t) + eps): it is the contract's closed form"""
    p0, grads = problem
    gs = [g.numpy() for g in grads]
    got = R.run(p0.numpy(), gs, LR, B1, B2, 1e-3, wd)
    torch_style = torch_run(torch.optim.AdamW, p0, grads, eps=1e-3, weight_decay=wd)
    assert np.abs(got[-1][0] - torch_style[-1]).max() > 1e-6
    assert np.abs(got[-1][0] - torch_run(torch.optim.Adam, p0, grads, eps=1e-3, weight_decay=wd)[-1]).max() > 1e-6
    for t in range(1, STEPS + 1):
        want = R.closed_form(p0.numpy(), gs[:t], LR, B1, B2, 1e-3, wd)
        assert np.abs(got[t - 1][0] - want).max() < 1e-12 * np.abs(want).max(), t


def test_a_skipped_step_advances_nothing(problem):
    p0, grads = problem
    gs = [g.numpy() for g in grads]
    skipped = R.run(p0.numpy(), gs, LR, B1, B2, 1e-8, 0.1, skips=[0, 0, 1, 0, 0, 0])
    assert skipped[2][3] == 2 and all(np.array_equal(a, b) for a, b in zip(skipped[2][:3], skipped[1][:3]))
    without = R.run(p0.numpy(), gs[:2] + gs[3:], LR, B1, B2, 1e-8, 0.1)
    assert np.array_equal(skipped[-1][0], without[-1][0]) and skipped[-1][3] == 5


def test_entry_point_is_declared_and_refuses_without_touching_the_gpu():
    """every pointer below is host memory (or null): a call that got past its checks would fault"""
    names = {"w2l_adam_step_guarded", "w2l_trainer_set_adam", "w2l_trainer_adam_steps", "w2l_trainer_set_adam_steps"}
    assert names <= set(_lib.exported_symbols())
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n), n
    assert hasattr(_lib._SIGS, "w2l_adam_step_guarded")
    buf = (C.c_float * 16)()
    a = C.addressof(buf)
    nan = float("nan")

    def call(p=a, g=a, m=a, v=a, n=4, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step=1, count=None):
        return L.w2l_adam_step_guarded(p, g, m, v, n, 0.01, beta1, beta2, eps, wd, 1.0, 0.0, None, step, count, None)
    for bad in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan),
                dict(beta2=1.0), dict(beta2=-0.1), dict(beta2=nan), dict(eps=-1e-8), dict(eps=nan), dict(wd=-0.1), dict(wd=nan),
                dict(step=0)):
        assert call(**bad) == _lib.W2L_EINVAL, bad
    assert call(n=0) == _lib.W2L_OK                       # nothing to do: no launch
    assert call(n=0, step=0, count=a) == _lib.W2L_OK      # a counter stands in for the host step
    assert call(n=0, beta1=0.0, beta2=0.0, eps=0.0) == _lib.W2L_OK


ARCH = "V -1 NFEAT 1 0\nTDS 1 5 8 0.1 0\nV 0 8 1 0\nRO 1 0 3 2\nL 8 NLABEL\n"


def cpu_trainer():
    from wav2letter_amd.trainer import Trainer
    tr = Trainer(ARCH, 8, 12, "ctc", 4, device="cpu")     # layout only: no kernel runs on the host
    tr.init_params(3)
    tr.to_device()
    return tr


def test_trainer_knows_adam_without_a_gpu():
    from wav2letter_amd.trainer import Trainer, _lib_tr
    tr = Trainer(ARCH, 8, 12, "ctc", 4, device="cpu")
    tr.set_optimizer("adam", "adam")
    assert tr._optim == ("adam", "adam") and tr._adam == (0.9, 0.999, 1e-8, 0.0)
    tr.set_optimizer("adam", "sgd", beta1=0.95, beta2=0.99, eps=1e-6, weight_decay=0.01)      # kinds mix per group
    assert tr._adam == (0.95, 0.99, 1e-6, 0.01)
    for bad in (dict(beta1=1.0), dict(beta2=-0.5), dict(eps=-1.0), dict(weight_decay=-0.1), dict(beta1=float("nan"))):
        with pytest.raises(_lib.W2LInvalidArgument):
            tr.set_optimizer("adam", "adam", **bad)
    with pytest.raises(_lib.W2LInvalidArgument):
        tr.set_optimizer("adagrad", "adagrad", weight_decay=0.1)      # the other optimizers have no decay
    with pytest.raises(_lib.W2LInvalidArgument):
        tr.set_optimizer("adamax", "sgd")
    L = _lib_tr()
    assert L.w2l_trainer_set_optimizer(tr.h, 3, 3) == 0 and L.w2l_trainer_set_optimizer(tr.h, 4, 0) == _lib.W2L_EINVAL
    assert L.w2l_trainer_set_adam(None, 0.9, 0.999, 1e-8, 0.0) == _lib.W2L_EINVAL
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert L.w2l_trainer_adam_steps(tr.h, C.byref(a), C.byref(b), None) == 0 and (a.value, b.value) == (0, 0)   # no Adam update yet
    tr2 = cpu_trainer()
    tr2.set_optimizer("adam", "adam")
    assert tr2.state2 is not None and tr2.state2.shape == tr2.params.shape and not tr2.state2.any()


def test_checkpoint_header_carries_adam(tmp_path):
    from wav2letter_amd import checkpoint
    a = cpu_trainer()
    a.set_optimizer("adam", "sgd", beta1=0.95, beta2=0.99, eps=1e-6, weight_decay=0.01)
    a.mom.copy_(torch.arange(a.n_floats, dtype=torch.float32))
    a.state2.copy_(torch.arange(a.n_floats, dtype=torch.float32) * 0.5)
    a.set_adam_steps(5, 3)
    path = str(tmp_path / "adam.w2l")
    checkpoint.save(path, a, ARCH, "ctc", step=6)
    hdr, arrays = checkpoint.read(path)
    assert hdr["optim"] == ["adam", "sgd"] and [t["kind"] for t in hdr["tensors"]][-2:] == ["momentum", "state2"]
    assert hdr["adam"] == {"beta1": 0.95, "beta2": 0.99, "eps": 1e-6, "weight_decay": 0.01, "steps": [5, 3]}
    b = cpu_trainer()
    with pytest.raises(ValueError):
        checkpoint.load(path, b, ARCH)                    # still an SGD trainer: the arenas would be misread
    b.set_optimizer("adam", "sgd")
    assert checkpoint.load(path, b, ARCH) == 6
    assert b._adam == a._adam and b.adam_steps() == (5, 3)
    assert torch.equal(b.mom, a.mom) and torch.equal(b.state2, a.state2) and torch.equal(b.params, a.params)
    # a file of another optimizer has no "adam" key: the bytes those files always had
    c = cpu_trainer()
    c.set_optimizer("adagrad", "adagrad")
    other = str(tmp_path / "adagrad.w2l")
    checkpoint.save(other, c, ARCH, "ctc", step=1)
    assert "adam" not in checkpoint.read(other)[0]
