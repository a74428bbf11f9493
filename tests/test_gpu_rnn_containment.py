"""Containment of w2l_rnn_forward / _backward (DESIGN.md 3.19 is the contract): with a workspace of exactly w2l_rnn_workspace_size
bytes and leading dimensions wider than the frames, the calls read their operands only inside their extents, write every element of
their results and nothing else, and do not depend on what the workspace held.

As in tests/test_gpu_cpc_containment.py the case runs on identical inputs in three guarded arenas (tests/arena.py) -- quiet, quiet
again, NaN -- and is compared with the float64 restatement (tests/rnn_ref.py).  I = 24, H = 33, two bidirectional layers, B = 3, T = 7:
H off every tile, layer 2 reading 2 H columns."""
import ctypes

import numpy as np
import pytest
import torch

import rnn_ref as RR
from tests.test_gpu_containment import _stream
from tests.test_gpu_cpc_containment import run_three
from wav2letter_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_forward_and_backward_stay_inside(mode):
    I, H, layers, dirs, B, T = 24, 33, 2, 2, 3, 7
    ldx, ldy = I + 3, H * dirs + 5
    rng = np.random.default_rng(mode)
    x, dy = rng.normal(size=(B, T, I)).astype(np.float32), rng.normal(size=(B, T, H * dirs)).astype(np.float32)
    params = (rng.uniform(-1, 1, RR.param_count(mode, I, H, layers, dirs)) / np.sqrt(H)).astype(np.float32)
    d = _lib.RnnDesc(mode, I, H, layers, dirs, B, T, ldx, ldy, 1, 0.0, 0, 0)

    def fn(r):
        L, dp = r.L, ctypes.byref(d)
        nbytes = L.w2l_rnn_workspace_size(dp)
        px, pdy, pp, ws = r.inp("x", x, ld=ldx), r.inp("dy", dy, ld=ldy), r.inp("params", params), r.work("workspace", nbytes)
        py = r.out("y", (B, T, H * dirs), ld=ldy)
        r.ok(L.w2l_rnn_forward(dp, px, pp, py, ws, nbytes, _stream()), "forward")
        r.ok(L.w2l_rnn_backward(dp, px, pp, py, pdy, r.out("dx", (B, T, I), ld=ldx), r.out("dparams", params.shape), ws, nbytes, _stream()), "backward")

        def ref():
            xt, pt = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (x, params))
            y = RR.forward(xt, pt, mode, H, layers, dirs)
            (y * torch.tensor(dy.astype(np.float64))).sum().backward()
            return {"y": ("rel", y.detach().numpy()), "dx": ("rel", xt.grad.numpy()), "dparams": ("rel", pt.grad.numpy())}
        return ref
    run_three(fn)
