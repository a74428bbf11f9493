"""Containment of the depthwise convolution entry points (DESIGN.md 3.19 is the contract): the forward pass, the data gradient and
the filter gradient with its workspace of exactly w2l_conv_depthwise_workspace_floats floats read their operands only inside their
extents, write every element of their results and nothing else, and do not depend on what the workspace held.

As in tests/test_gpu_cpc_containment.py the case runs on identical inputs in three guarded arenas (tests/arena.py) -- quiet, quiet
again, NaN -- and is compared with the float64 restatement (tests/depthwise_ref.py).  C = 260 (a second column tile of four
columns), kw = 31, T = one time chunk + 1, H on and off the float4 staging path."""
import ctypes

import numpy as np
import pytest
import torch

import depthwise_ref as D
from tests.test_gpu_containment import _stream
from tests.test_gpu_cpc_containment import run_three
from wav2letter_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("C,H", [(260, 1), (65, 3)])
def test_entry_points_stay_inside(C, H):
    B, T, kw, padl, padr = 2, 33, 31, 15, 15
    rng = np.random.default_rng(C)
    x, dy = (rng.normal(size=(B, T, H, C)).astype(np.float32) for _ in range(2))
    w, b = rng.normal(size=(kw, C)).astype(np.float32), rng.normal(size=C).astype(np.float32)
    d = _lib.ConvDesc(B, T, H, C, C, kw, 1, padl, padr)

    def fn(r):
        L, dp = r.L, ctypes.byref(d)
        px, pdy, pw, pb = r.inp("x", x), r.inp("dy", dy), r.inp("w", w), r.inp("b", b)
        ws = r.work("workspace", 4 * L.w2l_conv_depthwise_workspace_floats(dp))
        r.ok(L.w2l_conv_depthwise_forward(dp, px, pw, pb, r.out("y", (B, T, H, C)), _stream()), "forward")
        r.ok(L.w2l_conv_depthwise_backward_data(dp, pdy, pw, r.out("dx", (B, T, H, C)), _stream()), "backward data")
        r.ok(L.w2l_conv_depthwise_backward_filter(dp, px, pdy, r.out("dw", (kw, C)), r.out("db", (C,)), ws, _stream()), "backward filter")
        r.ok(L.w2l_conv_depthwise_backward_filter(dp, px, pdy, r.out("dw_alone", (kw, C)), None, ws, _stream()), "backward filter, no bias")

        def ref():
            xt, wt, bt = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (x, w, b))
            y = D.depthwise(xt, wt, bt, padl, padr)
            (y * torch.tensor(dy.astype(np.float64))).sum().backward()
            return {"y": ("rel", y.detach().numpy()), "dx": ("rel", xt.grad.numpy()), "dw": ("rel", wt.grad.numpy()),
                    "dw_alone": ("rel", wt.grad.numpy()), "db": ("rel", bt.grad.numpy())}
        return ref
    run_three(fn)
