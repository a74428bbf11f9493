"""Host side of the recurrent layers: the float64 restatement (tests/rnn_ref.py) against torch.nn.RNN / GRU / LSTM with
the weights copied in the contract's order -- which pins the gate order and the place of the GRU's b_hn --, the refusals of the C ABI,
the arch-line arguments and the layout refusal.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import rnn_ref as RR
from wav2letter_amd import _lib, recipes
from wav2letter_amd.trainer import Trainer

I, H, LAYERS, B, T = 24, 33, 2, 3, 7
MODULES = {0: lambda **k: torch.nn.RNN(nonlinearity="relu", **k), 1: lambda **k: torch.nn.RNN(nonlinearity="tanh", **k),
           2: torch.nn.LSTM, 3: torch.nn.GRU}


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("dirs", [1, 2])
def test_restatement_equals_torch_nn(mode, dirs):
    torch.manual_seed(mode * 2 + dirs)
    m = MODULES[mode](input_size=I, hidden_size=H, num_layers=LAYERS, bidirectional=dirs == 2, batch_first=True).double()
    flat = torch.cat([p.detach().flatten() for p in m.parameters()]).requires_grad_()
    assert flat.numel() == RR.param_count(mode, I, H, LAYERS, dirs)
    x, dy = torch.randn(B, T, I, dtype=torch.float64, requires_grad=True), torch.randn(B, T, H * dirs, dtype=torch.float64)
    want = m(x)[0]
    (want * dy).sum().backward()
    want_dx, x.grad = x.grad.clone(), None
    got = RR.forward(x, flat, mode, H, LAYERS, dirs)
    (got * dy).sum().backward()
    torch.testing.assert_close(got, want, rtol=0, atol=1e-12)
    torch.testing.assert_close(x.grad, want_dx, rtol=0, atol=1e-12)
    torch.testing.assert_close(flat.grad, torch.cat([p.grad.flatten() for p in m.parameters()]), rtol=0, atol=1e-12)


def desc(**k):
    f = dict(mode=2, I=I, H=H, layers=2, dirs=2, B=B, T=T, ldx=I, ldy=2 * H, train=1, dropP=0.0, seed=0, rngStream=0)
    f.update(k)
    return _lib.RnnDesc(*[f[n] for n, _ in _lib.RnnDesc._fields_])


def test_abi_sizes_and_refusals():
    L, one = _lib.lib(), ctypes.c_void_p(64)   # never dereferenced: every refusal precedes the first launch
    for mode in range(4):
        for dirs in (1, 2):
            assert L.w2l_rnn_param_count(ctypes.byref(desc(mode=mode, dirs=dirs, ldy=dirs * H))) == RR.param_count(mode, I, H, 2, dirs)
    train, infer = (L.w2l_rnn_workspace_size(ctypes.byref(desc(train=t))) for t in (1, 0))
    assert 0 < infer < train and train % 256 == 0
    call = lambda d, ws=train: L.w2l_rnn_forward(ctypes.byref(d), one, one, one, one, ws, None)
    for bad in (dict(mode=4), dict(mode=-1), dict(H=0), dict(dirs=3), dict(layers=0), dict(T=0), dict(ldx=I - 1), dict(ldy=2 * H - 1), dict(dropP=1.0)):
        assert call(desc(**bad)) == _lib.W2L_EINVAL, bad
        assert L.w2l_rnn_workspace_size(ctypes.byref(desc(**bad))) == 0
    assert call(desc(), train - 1) == _lib.W2L_EINVAL                                   # workspace too small
    assert L.w2l_rnn_forward(ctypes.byref(desc()), None, one, one, one, train, None) == _lib.W2L_EINVAL
    assert L.w2l_rnn_backward(ctypes.byref(desc(train=0)), one, one, one, one, one, one, one, train, None) == _lib.W2L_EINVAL
    for big in (dict(H=4097, ldy=2 * 4097), dict(I=4097, ldx=4097), dict(B=1025), dict(layers=9), dict(B=1024, T=65536)):
        assert call(desc(**big)) == _lib.W2L_EUNSUPPORTED, big
    assert L.w2l_rnn_workspace_size(ctypes.byref(desc(I=2048, H=2048, ldx=2048, ldy=4096, layers=8, B=256, T=100))) > 0   # the least the caps must cover


def net(line):
    return f"RO 1 3 0 2\n{line}\nRO 0 2 1 3\n"


@pytest.mark.parametrize("line,name,numel", [("RNN 8 5", "RNN", RR.param_count(0, 8, 5, 1, 1)), ("GRU 8 5 2", "GRU", RR.param_count(3, 8, 5, 2, 1)),
                                              ("LSTM 8 5 2 1 0.25", "LSTM", RR.param_count(2, 8, 5, 2, 2)), ("RNN 8 5 1 0 0 TANH", "RNN(tanh)", 5 * 15)])
def test_arch_lines_and_defaults(line, name, numel):
    tr = Trainer(net(line), 8, 5 * (2 if line.startswith("LSTM") else 1), "ctc", device="cpu")
    assert [(n, k) for n, k, _ in tr.param_table()] == [("rnn.params", numel)] and name in tr.describe()


@pytest.mark.parametrize("line", ["LSTM 8 x", "GRU 8 5 1 0 1.5", "RNN 8 5 1 0 0 SIGMOID", "LSTM 8 0", "GRU 8 5 0", "LSTM 8 5 1 0 0 TANH"])
def test_malformed_line_is_refused_with_the_line(line):
    with pytest.raises(_lib.W2LInvalidArgument, match="Failed parsing - " + line):
        Trainer(net(line), 8, 5, "ctc", device="cpu")


def test_layout_refusal_and_recipe():
    with pytest.raises(_lib.W2LInvalidArgument, match=r"LSTM: input must be \(8, B, T, 1\)"):
        Trainer("LSTM 8 5\n", 8, 5, "ctc", device="cpu")                               # the input layout (T, NFEAT, 1, B) itself
    with pytest.raises(_lib.W2LInvalidArgument, match=r"GRU: input must be \(4, B, T, 1\)"):
        Trainer("RO 1 3 0 2\nGRU 4 5\n", 8, 5, "ctc", device="cpu")                      # a frame of another width
    arch = recipes.blstm_ctc_arch(8, 16, 2, 6, 0.0)
    assert arch.splitlines() == ["RO 1 3 0 2", "LSTM 8 16 2 1 0.0", "RO 0 2 1 3", "L 32 6"]
    tr = Trainer(arch, 8, 6, "ctc", device="cpu")
    assert [n for n, _, _ in tr.param_table()] == ["rnn.params", "linear.w", "linear.b"]
    tr.init_params(1)
    p = tr.export_from(0, tr.host_params)
    assert np.abs(p).max() <= 0.25 and np.abs(p).max() > 0.24 and abs(float(p.mean())) < 0.01   # uniform +-1/sqrt(16)
