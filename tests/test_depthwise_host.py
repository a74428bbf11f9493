"""Host side of the depthwise convolutions and Swish: what the arch builder refuses, by name; the workspace arithmetic of the filter
gradient; fl::Conv2D's groups refusal through the compiled caller (tests/cpp/depthwise_caller.cpp).  No GPU."""
import ctypes
import os
import subprocess

import pytest

from wav2letter_amd import _lib, recipes, streaming
from wav2letter_amd.trainer import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFEAT, N = 8, 11
HEAD = "V -1 1 NFEAT 0\nC NFEAT 16 3 1 -1 1\n"
TAIL = "C 16 NLABEL 1 1 -1 1\nRO 2 0 3 1\n"


def module_net(kw=3):
    return "V -1 1 NFEAT 0\nC NFEAT 8 3 1 -1\n" + recipes.conformer_conv_module_arch(8, kw, 0.0) + "RO 2 0 3 1\nL 8 NLABEL\n"


@pytest.mark.parametrize("line,message", [
    ("C 16 16 3 1 -1 1 1 2", "groups = 2: besides 1, only a depthwise convolution is built"),
    ("C 16 32 3 1 -1 1 1 16", "groups = 16: besides 1, only a depthwise convolution is built"),
    ("C 16 16 3 2 -1 1 1 16", "groups = 16: besides 1, only a depthwise convolution is built"),
    ("C 16 16 3 1 -1 2 1 16", "dilation != 1 not supported"),
    ("C 16 16 65 1 -1 1 1 16", "kernel widths up to 64"),
    ("CFR 16 32 4 30 0.1 0.1", "outside the hot path"),
])
def test_arch_refusals_name_the_reason(line, message):
    with pytest.raises(_lib.W2LInvalidArgument, match=message):
        Trainer(HEAD + line + "\n" + TAIL, NFEAT, N, "ctc", device="cpu")


def test_module_builds_and_its_depthwise_line_keeps_a_following_relu():
    tr = Trainer(module_net(), NFEAT, N, "ctc", device="cpu")
    names = [(name, n) for name, n, _ in tr.param_table()]
    # front; LN; 1 x 1 to 2C; depthwise (kw, 1, 1, C); LN; 1 x 1; output Linear
    assert names == [("conv.w", 3 * 8 * 8), ("conv.b", 8), ("ln.weight+bias", 2), ("conv.w", 8 * 16), ("conv.b", 16), ("conv.w", 3 * 8), ("conv.b", 8),
                     ("ln.weight+bias", 2), ("conv.w", 8 * 8), ("conv.b", 8), ("linear.w", 8 * N), ("linear.b", N)]
    assert "Residual" in tr.describe()
    with_relu = Trainer(HEAD + "C 16 16 3 1 -1 1 1 16\nR\nSH 0.5\n" + TAIL, NFEAT, N, "ctc", device="cpu")
    assert "ReLU -> (4) Swish" in with_relu.describe()         # the R is not folded into the depthwise layer
    wn = Trainer(HEAD + "WN 3 C 16 16 5 1 -1 1 1 16\n" + TAIL, NFEAT, N, "ctc", device="cpu")
    assert [(name, n) for name, n, _ in wn.param_table()][2:5] == [("wn.v", 5 * 16), ("wn.g", 16), ("conv.b", 16)]


def test_streaming_session_refuses_the_depthwise_line():
    with pytest.raises(_lib.W2LError, match=r"arch line 'C 16 16 3 1 -1 1 1 16' \(Conv2D\) cannot be streamed: depthwise"):
        streaming.query(HEAD + "C 16 16 3 1 -1 1 1 16\n" + TAIL, NFEAT, N, 2, 8)


@pytest.mark.parametrize("B,T,H,C,kw,padl,padr", [(1, 1, 1, 4, 1, 0, 0), (3, 67, 2, 260, 31, 15, 15), (2, 40, 1, 260, 33, 16, 16), (16, 500, 1, 512, 31, 15, 15),
                                                   (16, 500, 1, 1024, 15, 7, 7), (64, 2000, 1, 768, 64, 0, 0)])
def test_workspace_arithmetic(B, T, H, C, kw, padl, padr):
    """S (kw + 1) H C floats: S segments of the B ceil(To / chunk) (utterance, chunk) items of a 256-column tile (chunk = 32 frames,
    16 above kw = 32), as many as give two workgroups per CU (512 / tiles), at most 128 and at most one per item"""
    To = T + padl + padr - kw + 1
    items, tiles = B * -(-To // (16 if kw > 32 else 32)), -(-H * C // 256)
    S = min(items, max(1, min(128, 512 // tiles)))
    d = _lib.ConvDesc(B, T, H, C, C, kw, 1, padl, padr)
    assert _lib.lib().w2l_conv_depthwise_workspace_floats(ctypes.byref(d)) == S * (kw + 1) * H * C
    for bad in (_lib.ConvDesc(B, T, H, C, C, 65, 1, 40, 40), _lib.ConvDesc(B, T, H, C, C + 1, kw, 1, padl, padr),
                _lib.ConvDesc(B, T + 64, H, C, C, kw, 2, padl, padr)):
        assert _lib.lib().w2l_conv_depthwise_workspace_floats(ctypes.byref(bad)) == 0


def test_fl_conv2d_refuses_groups_that_are_not_depthwise(tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "depthwise_caller.mk", "depthwise_caller", f"OUT={tmp_path}"],
                   check=True, capture_output=True)
    out = subprocess.run([str(tmp_path / "depthwise_caller"), "refusals"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "depthwise refusals ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
