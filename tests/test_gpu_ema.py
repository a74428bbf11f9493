"""slimIPL's two per-step primitives on the device: w2l_ema_update (the averaged teacher network, one launch over a flat
parameter arena; recipes/slimIPL/src/Train.cpp:1819-1832) and w2l_trainer_set_dropout (dynamic dropout of the `TR` layers,
:1465-1469 with the recipe plugin's 100h_supervised_slimipl.cpp:41-58)."""
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GUARD = 64
DECAYS = (0.0, 0.5, 0.999, 1.0)


def _arena(n, off, gen):
    """N(0,1) floats: 64 guards, `off` floats past a 16-byte boundary, n payload floats, 64 guards (+ slack)"""
    buf = torch.randn(GUARD + 4 + n + GUARD, device="cuda", generator=gen)
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + off
    return buf, buf[lo:lo + n]


@pytest.mark.parametrize("n", [1, 5, 255, 256, 257, 4099, 2 ** 20 + 3])
def test_ema_update_against_float64_every_alignment(n):
    """|got - r| <= 4 * 2^-24 * (|d * ema| + |(1 - d) * p|) per element: two roundings of the constants d and 1 - d to fp32, one
    per product, one for the sum, each at most 2^-24 relative to a term no larger than the two magnitudes' sum.  ema and p
    sit 0..3 floats past a 16-byte boundary, independently; the guards on both sides of both arrays stay as they were."""
    from wav2letter_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(n)
    for oe in range(4):
        for op in range(4):
            for d in DECAYS:
                ebuf, e = _arena(n, oe, gen)
                pbuf, p = _arena(n, op, gen)
                assert e.data_ptr() % 16 == 4 * oe and p.data_ptr() % 16 == 4 * op
                ebuf0, pbuf0, e0 = ebuf.clone(), pbuf.clone(), e.clone()
                ops.ema_update(e, p, d)
                t0, t1 = d * e0.double(), (1.0 - d) * p.double()
                err = (e.double() - (t0 + t1)).abs()
                bound = 4 * 2.0 ** -24 * (t0.abs() + t1.abs())
                worst = float((err - bound).max())
                assert worst <= 0.0, (n, oe, op, d, worst, float(err.max()))
                if d == 1.0:
                    assert torch.equal(e, e0), (n, oe, op)
                if d == 0.0:
                    assert torch.equal(e, p), (n, oe, op)
                lo = GUARD + oe
                assert torch.equal(ebuf[:lo], ebuf0[:lo]) and torch.equal(ebuf[lo + n:], ebuf0[lo + n:]), (n, oe, op, d)
                assert torch.equal(pbuf, pbuf0), (n, oe, op, d)


def test_ema_update_refusals_leave_the_arrays_alone():
    from wav2letter_amd import _lib, ops
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(3)
    e = torch.randn(300, device="cuda", generator=gen)
    p = torch.randn(300, device="cuda", generator=gen)
    e0, p0 = e.clone(), p.clone()
    assert L.w2l_ema_update(None, p.data_ptr(), 300, 0.5, s) == _lib.W2L_EINVAL
    assert L.w2l_ema_update(e.data_ptr(), None, 300, 0.5, s) == _lib.W2L_EINVAL
    for bad in (float("nan"), -1e-9, 1.0 + 1e-9, float("inf"), -float("inf")):
        assert L.w2l_ema_update(e.data_ptr(), p.data_ptr(), 300, bad, s) == _lib.W2L_EINVAL, bad
        with pytest.raises(ValueError):
            ops.ema_update(e, p, bad)
    assert L.w2l_ema_update(e.data_ptr(), p.data_ptr(), 0, 0.5, s) == _lib.W2L_OK   # n == 0: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(e, e0) and torch.equal(p, p0)


# ---- w2l_trainer_set_dropout

def _tr_arch(p, pld):
    return f"V -1 1 NFEAT 0\nRO 2 0 3 1\nTR 32 48 4 6 {p} {pld}\nTR 32 48 4 6 {p} {pld}\nDO 0.25\nL 32 NLABEL\n"


def _one_step(arch, override, mixed, step):
    """emissions (training mode) and every gradient of one step from the library's own initialisation"""
    from wav2letter_amd.trainer import Trainer
    nfeat, nlabel, B, T, L = 32, 9, 3, 21, 4
    rng = np.random.default_rng(11)
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    tr = Trainer(arch, nfeat, nlabel, "ctc", 4, 0.0)
    tr.init_params(5)
    tr.plan(B, T, L)
    tr.to_device()
    if mixed:
        tr.set_mixed_precision(True)
    out = []
    for ov in override:
        if ov is not None:
            tr.set_dropout(*ov)
        tr.set_step(step)
        em = tr.forward(x, train=True).clone()
        tr.set_step(step)
        loss = tr.forward_backward(x, tgt).clone()
        out.append((em.cpu().numpy(), loss.cpu().numpy(), tr.grads.cpu().numpy().copy()))
    return out


@pytest.mark.parametrize("mixed", [False, True], ids=["fp32", "bf16"])
def test_set_dropout_equals_the_arch_written_with_those_numbers(mixed):
    """two `TR` blocks with 0.3 / 0.3 in the arch: the override (0.1, 0.1) gives, bit for bit, the emissions, losses and
    gradients of the arch written with 0.1 / 0.1 at the same step and seed; (-1, -1) restores the 0.3 / 0.3 results.  The `DO`
    layer keeps its own probability throughout (only TR layers answer).  Steps are chosen so that layer drop takes a block
    out in one of the two settings at least (the numbers differ between 0.3 and 0.1, asserted)."""
    hit = False
    for step in (3, 4):
        base, over, back = _one_step(_tr_arch(0.3, 0.3), [None, (0.1, 0.1), (-1, -1)], mixed, step)
        want01, = _one_step(_tr_arch(0.1, 0.1), [None], mixed, step)
        for got, want in ((over, want01), (back, base)):
            for a, b in zip(got, want):
                assert np.array_equal(a, b)
        assert np.isfinite(base[1]).all() and np.isfinite(over[1]).all()
        hit = hit or not np.array_equal(base[0], over[0])
    assert hit
    # an arch without TR dropout takes the override too (no new plan), and a mixed override moves each number on its own
    z, zo = _one_step(_tr_arch(0.0, 0.0), [None, (0.1, 0.1)], mixed, 3)
    want01, = _one_step(_tr_arch(0.1, 0.1), [None], mixed, 3)
    assert all(np.array_equal(a, b) for a, b in zip(zo, want01)) and not np.array_equal(z[0], zo[0])
    half, = _one_step(_tr_arch(0.3, 0.3), [(0.1, -1)], mixed, 3)
    want_half, = _one_step(_tr_arch(0.1, 0.3), [None], mixed, 3)
    assert all(np.array_equal(a, b) for a, b in zip(half, want_half))


def test_set_dropout_refuses_bad_probabilities():
    from wav2letter_amd.trainer import Trainer
    tr = Trainer(_tr_arch(0.3, 0.3), 32, 9, "ctc", 4, 0.0)
    for bad in ((1.0, 0.1), (0.1, 1.5), (float("nan"), 0.1)):
        with pytest.raises(ValueError):
            tr.set_dropout(*bad)


def test_facade_select_batch_ema_update_and_dropout_switch(tmp_path):
    """G3 and the fl:: side of the two primitives, in C++ (tests/cpp/ipl_test.cpp -DIPL_TEST_FACADE against libw2l_hip.so):
    fl::ext::selectBatch with B = 4 and rows {2, 0} -- forward equals the gathered rows, backward the scattered gradient with
    exact zeros elsewhere, all rows in order is the argument itself; fl::ext::emaUpdate over two planned networks' arenas and over
    plain parameter lists; fl::Sequential::setTransformerDropout"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "ipl_facade_test")
    lib = os.path.join(root, "wav2letter_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-DIPL_TEST_FACADE", os.path.join(root, "tests", "cpp", "ipl_test.cpp"), "-o", exe,
                    f"-L{lib}", "-lw2l_hip", f"-Wl,-rpath,{lib}", "-ldl"], check=True)
    out = subprocess.run([exe, "facade"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.splitlines() == ["selectBatch ok", "emaUpdate ok", "setTransformerDropout ok"]
