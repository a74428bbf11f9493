"""The depthwise time-convolution kernels (w2l_conv_depthwise_*, conv_depthwise.hip) and the Swish kernels on the GPU against the
float64 restatement (tests/depthwise_ref.py), each tensor within 1e-4 of the largest reference magnitude.  The kernels' time chunk
is 32 output frames (16 above kw = 32), a column tile 256 floats of the H * C frame, the unroll classes kw <= 8 / 16 / 32 / 64."""
import ctypes

import numpy as np
import pytest
import torch

import depthwise_ref as D
import residual_ref as R
from wav2letter_amd import _lib, ops

pytestmark = pytest.mark.gpu
TOL = 1e-4
CHUNK, CHUNK_WIDE = 32, 16
SAME = "same"

# (C, kw, (padl, padr), T, B, H, bias, skew): skew = floats between a 16-byte boundary and the start of x / dy.  kw on both sides of
# every unroll class (8 | 9, 16 | 17, 32 | 33, 64); T around the class's chunk (32 frames, 16 above kw = 32)
CASES = [
    (4, 1, (0, 0), 1, 1, 1, True, 0),
    (6, 2, SAME, CHUNK + 1, 3, 2, True, 0),
    (6, 3, (2, 5), 2, 1, 1, False, 0),                 # T = kw - 1; a frame of 6 floats: column-by-column staging
    (6, 8, SAME, 2 * CHUNK + 3, 3, 1, True, 0),
    (68, 9, (8, 0), CHUNK - 1, 1, 1, True, 1),         # float4 frames on a base that is not 16-byte aligned
    (68, 16, SAME, CHUNK + 1, 3, 1, False, 0),
    (260, 17, (2, 5), 2 * CHUNK + 3, 1, 2, True, 0),   # 520 columns: two full tiles and one of 8
    (260, 31, (0, 0), 2 * CHUNK + 3, 3, 1, True, 0),
    (68, 32, (31, 0), 31, 1, 1, True, 0),              # 63 staged frames: the most LDS under 64 KiB
    (68, 33, (32, 0), CHUNK_WIDE + 1, 3, 1, False, 0),
    (260, 64, SAME, 2 * CHUNK_WIDE + 3, 1, 2, True, 0),
    (68, 64, (63, 0), CHUNK_WIDE - 1, 1, 1, True, 0),
    (260, 3, (2, 5), 1, 1, 1, True, 0),
    (4, 33, (2, 5), 32, 1, 2, True, 0),
]


def rel(got, want):
    want = want.detach().numpy()
    return np.abs(got.cpu().numpy().astype(np.float64) - want).max() / max(np.abs(want).max(), 1e-30)


def skewed(a, skew):
    """the array on the GPU, `skew` floats behind a 16-byte boundary"""
    buf = torch.empty(a.size + 4, device="cuda", dtype=torch.float32)
    v = buf[skew:skew + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


@pytest.mark.parametrize("C,kw,pad,T,B,H,bias,skew", CASES)
def test_three_passes_against_restatement(C, kw, pad, T, B, H, bias, skew):
    padl, padr = (R.same_pad(T, kw, 1),) * 2 if pad == SAME else pad
    rng = np.random.default_rng(C + kw + T)
    x = rng.normal(size=(B, T, H, C)).astype(np.float32)
    w = rng.normal(size=(kw, C)).astype(np.float32)
    b = rng.normal(size=C).astype(np.float32) if bias else None
    To = T + padl + padr - kw + 1
    dy = rng.normal(size=(B, To, H, C)).astype(np.float32)
    xt, wt = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (x, w))
    bt = torch.tensor(b.astype(np.float64), requires_grad=True) if bias else None
    yr = D.depthwise(xt, wt, bt, padl, padr)
    (yr * torch.tensor(dy.astype(np.float64))).sum().backward()

    xd, dyd, wd = skewed(x, skew), skewed(dy, skew), torch.from_numpy(w).cuda()
    bd = torch.from_numpy(b).cuda() if bias else None
    y = ops.conv_depthwise_forward(xd, wd, bd, padl=padl, padr=padr)
    dx, dw, db = ops.conv_depthwise_backward(xd, wd, dyd, padl=padl, padr=padr, need_dbias=bias)
    dx2, dw2, db2 = ops.conv_depthwise_backward(xd, wd, dyd, padl=padl, padr=padr)
    figures = {"y": rel(y, yr), "dx": rel(dx, xt.grad), "dw": rel(dw, wt.grad), "dbias": rel(db2, torch.tensor(dy.astype(np.float64)).sum((0, 1, 2)))}
    print(figures)
    assert y.shape == yr.shape and all(v <= TOL for v in figures.values()), figures
    # no atomics: a second run of the filter gradient gives the same bits, with and without the bias gradient
    assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32)) and torch.equal(dx.view(torch.int32), dx2.view(torch.int32))
    assert db is None or torch.equal(db.view(torch.int32), db2.view(torch.int32))


@pytest.mark.parametrize("C,kw,pad,T,lead", [(68, 31, (15, 15), 2 * CHUNK + 3, 5), (260, 3, (2, 5), CHUNK - 1, 7), (68, 15, (7, 7), CHUNK + 1, 11),
                                           (6, 64, (63, 0), 2 * CHUNK_WIDE + 1, 29)])
def test_a_frame_does_not_depend_on_tile_placement(C, kw, pad, T, lead):
    """frames 0 .. To-1 of a padded utterance equal, bit for bit, the same frames inside a longer unpadded utterance that supplies
    the padding as real zero frames behind `lead` other frames, so that every chunk boundary falls elsewhere"""
    padl, padr = pad
    rng = np.random.default_rng(kw)
    x = rng.normal(size=(2, T, 1, C)).astype(np.float32)
    w, b = torch.from_numpy(rng.normal(size=(kw, C)).astype(np.float32)).cuda(), torch.from_numpy(rng.normal(size=C).astype(np.float32)).cuda()
    longer = np.zeros((2, lead + padl + T + padr, 1, C), np.float32)
    longer[:, :lead] = rng.normal(size=(2, lead, 1, C))
    longer[:, lead + padl:lead + padl + T] = x
    y = ops.conv_depthwise_forward(torch.from_numpy(x).cuda(), w, b, padl=padl, padr=padr)
    y2 = ops.conv_depthwise_forward(torch.from_numpy(longer).cuda(), w, b)
    assert y2.shape[1] == lead + y.shape[1] and float(y.abs().max()) > 0
    assert torch.equal(y.view(torch.int32), y2[:, lead:].contiguous().view(torch.int32))


@pytest.mark.parametrize("beta", [1.0, 0.5])
@pytest.mark.parametrize("n,offs", [(1, (0, 0, 0)), (3, (1, 1, 1)), (4, (0, 1, 2)), (1027, (3, 3, 3)), (1027, (2, 0, 2))])
def test_swish_against_restatement(n, offs, beta):
    """x over +-30 (beta x around 20 included); operands 0 to 3 floats behind a 16-byte boundary, in and out of phase"""
    rng = np.random.default_rng(n)
    x = np.concatenate([rng.uniform(-30, 30, size=n), [30.0, -30.0, 20.0 / beta, -20.0 / beta]])[-n:].astype(np.float32)
    dy = rng.normal(size=n).astype(np.float32)
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    yr = D.swish(xt, beta)
    (yr * torch.tensor(dy.astype(np.float64))).sum().backward()
    xd, dyd = skewed(x, offs[0]), skewed(dy, offs[1])
    y = torch.empty(n + 4, device="cuda")[offs[2]:offs[2] + n]
    dx = torch.empty(n + 4, device="cuda")[offs[2]:offs[2] + n]
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib().w2l_swish_forward(xd.data_ptr(), y.data_ptr(), n, beta, s), "swish forward")
    ops.swish_backward(xd, dyd, beta, out=dx)
    figures = {"y": rel(y, yr), "dx": rel(dx, xt.grad)}
    print(figures)
    assert all(v <= TOL for v in figures.values()), figures
    assert torch.equal(ops.swish_forward(xd, beta), y)
    assert torch.equal(ops.swish_backward(xd, dyd, beta, out=dyd), dx)      # dx may be dy


@pytest.mark.parametrize("cin,cout,kw,stride", [(8, 8, 3, 2), (8, 12, 3, 1), (8, 8, 65, 1)], ids=["stride-2", "cin-not-cout", "kw-65"])
def test_refusals(cin, cout, kw, stride):
    x, w = torch.zeros(1, 80, 1, cin, device="cuda"), torch.zeros(kw, cout, device="cuda")
    d = ops.conv_depthwise_desc(x, w, stride)
    assert _lib.lib().w2l_conv_depthwise_workspace_floats(ctypes.byref(d)) == 0
    with pytest.raises(_lib.W2LError, match="W2L_EUNSUPPORTED"):
        ops.conv_depthwise_forward(x, w, stride=stride)
    with pytest.raises(_lib.W2LError, match="W2L_EUNSUPPORTED"):
        ops.conv_depthwise_backward(x, w, torch.zeros(1, 80, 1, cout, device="cuda"), stride=stride)
