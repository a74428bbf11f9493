"""The recurrent layers on the GPU against the float64 restatement (tests/rnn_ref.py): the scan kernels through the C
ABI, the long scan, determinism and independence of the batch tile, dropout between the layers, the BLSTM-CTC arch under the trainer
(checkpoint, re-plan) and fl::RNN through a compiled caller.  The bar is the project's fp32 bar, 1e-4 of the largest magnitude of each
compared tensor (float32 torch.nn against float64 stays within 1e-6 on these shapes: a miss is a bug, not rounding)."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import rnn_ref as RR
from oracle import pyoracle as O
from tests.test_gpu_residual import batch, gpu_pass, make_trainer, rel
from wav2letter_amd import checkpoint, ops, recipes
from wav2letter_amd.criterion import CriterionScaleMode, CTCLoss
from wav2letter_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
MODES = ["relu", "tanh", "lstm", "gru"]
# the kernels' edges: a workgroup takes 32 batch rows and 32 / G hidden units (32 in the backward); the reduction is staged in chunks
# of 128 columns, 32 per wave; weight rows are read 16 bytes at a time when H % 4 == 0
SHAPES = {                                   # I, H, layers, dirs, B, T
    "base": (24, 33, 2, 2, 3, 7),            # H no tile multiple and past every hidden slice, I != H, layer 2 reads 2 H, element-wise weight reads
    "B1": (24, 33, 2, 2, 1, 7),
    "T1": (24, 33, 2, 2, 3, 1),              # no recurrent product at all: dW_hh is exactly zero
    "T2": (24, 33, 2, 2, 3, 2),              # one hand-over
    "B33": (24, 33, 1, 2, 33, 3),            # a second batch tile of one row
    "H132": (20, 132, 1, 2, 3, 4),           # a second reduction chunk of 4 columns (three waves idle in it); 16-byte weight reads
}
ARCH = recipes.blstm_ctc_arch(8, 16, 2, 6, 0.0)
NET = dict(nfeat=8, nlabel=6)


def operands(mode, I, H, layers, dirs, B, T, seed=0):
    rng = np.random.default_rng(seed)
    n = RR.param_count(ops.RNN_MODES[mode], I, H, layers, dirs)
    params = rng.uniform(-1, 1, n).astype(np.float32) / np.float32(np.sqrt(H))
    return rng.normal(size=(B, T, I)).astype(np.float32), params, rng.normal(size=(B, T, H * dirs)).astype(np.float32)


def gpu(mode, x, params, dy, H, layers, dirs, **k):
    """(y, dx, dparams) through the C ABI; dy None: forward only"""
    xd, pd = torch.from_numpy(x).cuda(), torch.from_numpy(params).cuda()
    d = ops.rnn_desc(xd, mode, H, layers, dirs == 2, **k)
    y, ws = ops.rnn_forward(d, xd, pd)
    if dy is None:
        return y.cpu().numpy()
    dx, dp = ops.rnn_backward(d, xd, pd, y, torch.from_numpy(dy).cuda(), ws)
    return y.cpu().numpy(), dx.cpu().numpy(), dp.cpu().numpy()


def ref(mode, x, params, dy, H, layers, dirs, masks=None):
    xt, pt = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (x, params))
    y = RR.forward(xt, pt, ops.RNN_MODES[mode], H, layers, dirs, masks)
    (y * torch.tensor(dy.astype(np.float64))).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), pt.grad.numpy()


def compare(got, want, what):
    figures = {k: rel(g, w) for k, g, w in zip(("y", "dx", "dparams"), got, want)}
    print(what, figures)
    for k, v in figures.items():
        assert v < TOL, (what, k, v)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", MODES)
def test_scan_against_restatement(mode, shape):
    I, H, layers, dirs, B, T = SHAPES[shape]
    x, params, dy = operands(mode, *SHAPES[shape])
    compare(gpu(mode, x, params, dy, H, layers, dirs, train=True), ref(mode, x, params, dy, H, layers, dirs), (mode, shape))


@pytest.mark.parametrize("mode,layers,dirs", [("gru", 1, 1), ("lstm", 2, 2)])
def test_long_scan(mode, layers, dirs):
    """300 hand-overs between launches, and the error growth along the scan, under the same bar"""
    x, params, dy = operands(mode, 40, 64, layers, dirs, 3, 300, seed=1)
    compare(gpu(mode, x, params, dy, 64, layers, dirs, train=True), ref(mode, x, params, dy, 64, layers, dirs), (mode, "T300"))


@pytest.mark.parametrize("mode", MODES)
def test_two_runs_agree_and_a_row_does_not_depend_on_its_tile(mode):
    """B = 65: three batch tiles.  One layer with I <= 32, so that the input-side product is one K step of the GEMM whatever its M
    and the statement is about the scan"""
    I, H, dirs, B, T = 24, 33, 2, 65, 5
    x, params, dy = operands(mode, I, H, 1, dirs, B, T, seed=2)
    a, b = (gpu(mode, x, params, dy, H, 1, dirs, train=True) for _ in range(2))
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    for row in (0, 40, 64):
        alone = gpu(mode, x[row:row + 1], params, None, H, 1, dirs)
        assert np.array_equal(alone[0], gpu(mode, x, params, None, H, 1, dirs)[row]), row


@pytest.mark.parametrize("mode", ["lstm", "gru"])
def test_dropout_between_the_layers(mode):
    I, H, layers, dirs, B, T = SHAPES["base"]
    x, params, dy = operands(mode, *SHAPES["base"], seed=3)
    plain = gpu(mode, x, params, None, H, layers, dirs)
    assert np.array_equal(gpu(mode, x, params, None, H, layers, dirs, dropout=0.5, seed=11, rng_stream=4), plain)        # eval: the identity
    got = gpu(mode, x, params, dy, H, layers, dirs, dropout=0.5, train=True, seed=11, rng_stream=4)
    assert not np.array_equal(got[0], plain)
    # the mask the layer kept: the library's stateless hash over the flat [B T][H dirs] input of layer l (include/w2l_hip.h)
    masks = [None] + [torch.tensor(O.dropout(np.ones((B, T, H * dirs), np.float32), 0.5, 11 ^ (0x9E3779B9 * l & 0xFFFFFFFF), 4).astype(np.float64))
                      for l in range(1, layers)]
    assert 0.3 < float((masks[1] == 0).double().mean()) < 0.7
    compare(got, ref(mode, x, params, dy, H, layers, dirs, masks), (mode, "dropout"))


@functools.lru_cache(None)
def trained():
    """one CTC step of the BLSTM recipe at B = 2, T = 12 on the GPU and in the restatement"""
    shape = (2, 12, 3)
    tr = make_trainer(ARCH, shape=shape, **NET)
    x, tgt, _ = batch(5, shape, **NET)
    from residual_ref import ctc_loss, to_torch
    params = to_torch([tr.export_from(i, tr.host_params) for i in range(len(tr.param_table()))], RR.param_shapes(ARCH, 8, 6))
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    em = RR.Net(ARCH, 8, 6).forward(xt, params)
    loss = ctc_loss(em, tgt)
    loss.sum().backward()
    return tr, x, tgt, gpu_pass(tr, x, tgt), (loss.detach().numpy(), em.detach().numpy(), [p.grad.numpy().reshape(-1) for p in params], xt.grad.numpy())


def test_blstm_ctc_step_against_restatement():
    tr, x, tgt, (gl, gem, ggrads, gdx), (l, em, grads, dx) = trained()
    figures = {"loss": rel(gl, l), "emission": rel(gem, em), "dx": rel(gdx, dx)}
    figures.update({f"grad {tr.param_table()[i][0]}": rel(g, w) for i, (g, w) in enumerate(zip(ggrads, grads))})
    print(figures)
    assert len(ggrads) == 3 and np.isfinite(gl).all()
    for k, v in figures.items():
        assert v < TOL, (k, v)


def test_checkpoint_round_trip_and_replan(tmp_path):
    tr, x, tgt = trained()[:3]
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    tr.update(0.05, momentum=0.5)
    path = str(tmp_path / "blstm.bin")
    checkpoint.save(path, tr, ARCH, "ctc", step=1)
    fresh = Trainer(ARCH, 8, 6, "ctc", CriterionScaleMode.TARGET_SZ_SQRT)
    assert checkpoint.load(path, fresh, ARCH) == 1
    fresh.to_device()
    fresh.plan(2, 12, 3)
    assert torch.equal(fresh.params, tr.params) and torch.equal(fresh.mom, tr.mom)
    out = []
    for t in (tr, fresh):
        loss = t.forward_backward(xd, td).cpu().numpy().copy()
        t.update(0.05, momentum=0.5)
        out.append((loss, t.params.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.isfinite(out[0][1]).all()
    # a second (B, T) through the same trainer equals a trainer planned for it alone
    shape = (3, 9, 3)
    x2, tgt2, _ = batch(6, shape, **NET)
    other = make_trainer(ARCH, shape=shape, **NET)
    other.params.copy_(tr.params)
    tr.plan(*shape)
    a, b = gpu_pass(tr, x2, tgt2), gpu_pass(other, x2, tgt2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(u, v) for u, v in zip(a[2], b[2]))


def test_fl_rnn_caller_and_autograd_wrapper_give_the_abi_bits(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "rnn_caller.mk", "rnn_caller", f"OUT={tmp_path}"], check=True, capture_output=True)
    out = subprocess.run([str(tmp_path / "rnn_caller"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "rnn caller ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
    B, T, I, H = 2, 9, 8, 5
    n = RR.param_count(3, I, H, 2, 2)
    x, params, y, loss, grad = np.split(np.fromfile(tmp_path / "out.bin", np.float32), np.cumsum([B * I * T, n, B * T * 2 * H, B]))
    xd = torch.from_numpy(x.reshape(B, I, T).transpose(0, 2, 1).copy()).cuda()
    pd = torch.from_numpy(params).cuda().requires_grad_()
    yd = ops.rnn(xd, pd, "gru", H, 2, True)
    l = CTCLoss(CriterionScaleMode.TARGET_SZ_SQRT)(yd, torch.tensor([[1, 2], [3, -1]], dtype=torch.int32, device="cuda"))
    l.sum().backward()
    assert np.array_equal(yd.detach().cpu().numpy().reshape(-1), y) and np.array_equal(l.detach().cpu().numpy(), loss)
    assert np.array_equal(pd.grad.cpu().numpy(), grad) and np.abs(grad).max() > 0
