"""The bf16 wide time convolution at H = 1 (w2l_conv_bf16_*, conv_bf16.hip) and the second level of the mixed-precision mode
(Trainer.set_mixed_precision(True, convs=True), --w2l_amp_convs) on the GPU: the three passes against the oracle on the SAME
bf16-rounded operands, the recipe's widest layer against the bound that holds for any summation order, a conv_glu miniature
against the bf16-operand reference network, and the drivers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import refnet
from tests.list_fixture import ENV, ROOT, _fixture, _train_cmd
from tests.test_gpu_nn import BF16_TOL, dev, from_fm, rel, to_fm, w_to_dev

pytestmark = pytest.mark.gpu

DECODE_EXE = os.path.join(ROOT, "wav2letter_amd", "bin", "Decode")
U = 2.0 ** -24   # unit roundoff of the fp32 accumulation


def _operands(rng, B, Cin, Cout, T, kw):
    x = rng.standard_normal((B, Cin, 1, T), dtype=np.float32)
    w = rng.standard_normal((Cout, Cin, kw), dtype=np.float32) / np.float32(np.sqrt(Cin * kw))
    b = rng.standard_normal(Cout, dtype=np.float32)
    return x, w, b


def _within(got, want, bar, bound, what):
    """the project's bar on |error| / max |reference|; an error above it must still lie, element by element, under the bound that
    holds for ANY summation order of exact bf16 x bf16 products in fp32.  Prints the measured figure either way."""
    e = rel(got, want)
    print(f"{what}: rel {e:.3e} (bar {bar:.0e})")
    if e < bar:
        return e
    lim = bound()
    over = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) - lim
    assert (over <= 0).all(), (what, e, float(over.max()))
    return e


CASES = [(3, 40, 46, 37, 5, 1, 0, 0),        # channels no multiples of 8, M and K tails
         (2, 33, 32, 9, 5, 1, 12, 12),       # padding larger than kw: windows wholly inside the padding
         (2, 64, 96, 13, 13, 1, 0, 0),       # T = kw: one output frame
         (2, 48, 80, 31, 3, 2, 1, 1),        # stride 2, odd T
         (1, 321, 706, 40, 19, 1, 0, 0),     # a recipe layer's odd widths
         (1, 80, 1024, 50, 3, 1, 1, 1)]      # the Transformer front end


@pytest.mark.parametrize("B,Cin,Cout,T,kw,stride,padl,padr", CASES)
def test_conv_bf16_three_passes(oracle, B, Cin, Cout, T, kw, stride, padl, padr):
    """forward (+ bias, + ReLU), backward-data (with and without the addend), filter and bias gradient against the oracle on the same
    bf16-rounded operands at the TDS family's bars (2e-5 for y and dx, 5e-5 for dw; measured on MI355X: every figure of every case between 5e-8
    and 7e-7, the bias gradient exact), BF16_TOL against the unrounded convolution, and a second call bit-identical"""
    from wav2letter_amd import ops
    rng = np.random.default_rng(1000 * Cin + T)
    x, w, b = _operands(rng, B, Cin, Cout, T, kw)
    xr, wr = refnet.bf16_round(x), refnet.bf16_round(w)
    y_ref = oracle.conv_fwd(xr, wr, b, stride, padl, padr)
    xd, wd, bd = dev(to_fm(x)), dev(w_to_dev(w)), dev(b)
    out = ops.conv_bf16(xd, wd, bd, padl, padr, stride=stride)
    assert out is not None, "the accepted set of the issue must have a kernel"
    y, imgs, d = out
    Kf = kw * Cin
    fwd_bound = lambda: Kf * U * (oracle.conv_fwd(np.abs(xr), np.abs(wr), np.abs(b), stride, padl, padr).astype(np.float64))
    _within(from_fm(y.cpu().numpy()), y_ref, 2e-5, fwd_bound, "y")
    assert rel(from_fm(y.cpu().numpy()), oracle.conv_fwd(x, w, b, stride, padl, padr)) < BF16_TOL
    yr, _, _ = ops.conv_bf16(xd, wd, bd, padl, padr, relu=True, stride=stride)
    _within(from_fm(yr.cpu().numpy()), np.maximum(y_ref, 0), 2e-5, fwd_bound, "relu(y)")
    y0, _, _ = ops.conv_bf16(xd, wd, None, padl, padr, stride=stride)
    _within(from_fm(y0.cpu().numpy()), oracle.conv_fwd(xr, wr, None, stride, padl, padr), 2e-5, fwd_bound, "y without bias")
    assert torch.equal(y, ops.conv_bf16(xd, wd, bd, padl, padr, stride=stride)[0])

    dy = rng.standard_normal(y_ref.shape, dtype=np.float32)
    add = rng.standard_normal(x.shape, dtype=np.float32)
    dyr = refnet.bf16_round(dy)
    odx, odw, odb = oracle.conv_bwd(xr, wr, dyr, stride, padl, padr)
    absb = lambda: oracle.conv_bwd(np.abs(xr), np.abs(wr), np.abs(dyr), stride, padl, padr)
    dyd, addd = dev(to_fm(dy)), dev(to_fm(add))
    dx, dw, db = ops.conv_bf16_backward(xd, dyd, imgs, d, add=addd, with_bias=True)
    To = y_ref.shape[3]
    _within(from_fm(dx.cpu().numpy()), odx + add, 2e-5, lambda: kw * Cout * U * (absb()[0].astype(np.float64) + np.abs(add)), "dx + add")
    _within(dw.cpu().numpy(), w_to_dev(odw), 5e-5, lambda: B * To * U * w_to_dev(absb()[1]).astype(np.float64), "dw")
    _within(db.cpu().numpy(), odb, 5e-5, lambda: B * To * U * absb()[2].astype(np.float64), "dbias")
    dx2, dw2, db2 = ops.conv_bf16_backward(xd, dyd, imgs, d, add=addd, with_bias=True)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    dx0, dw0 = ops.conv_bf16_backward(xd, dyd, imgs, d)
    _within(from_fm(dx0.cpu().numpy()), odx, 2e-5, lambda: kw * Cout * U * absb()[0].astype(np.float64), "dx")
    assert torch.equal(dw0, dw)
    assert rel(from_fm(dx0.cpu().numpy()), oracle.conv_bwd(x, w, dy, stride, padl, padr)[0]) < BF16_TOL
    assert rel(dw.cpu().numpy(), w_to_dev(oracle.conv_bwd(x, w, dy, stride, padl, padr)[1])) < BF16_TOL


def test_conv_bf16_recipe_width_under_the_summation_order_bound(oracle):
    """conv_glu's widest layer, 826 -> 1816 channels at kw 29 (K = 23 954), one utterance of 40 frames: bf16 x bf16 products are
    exact in fp32, so for any summation order every element's error is at most K 2^-24 (sum |x~| |w~| + |bias|), with K the
    element's reduction length (kw Cin forward, kw Cout backward-data, B To for the filter gradient) -- the bound is the same oracle
    call on absolute values.  Measured on MI355X (|error| / max |reference|): y 3.0e-07, dx 7.0e-07, dw 7.1e-08, dbias 0; the
    largest |error| / bound of any element: y 1.3e-05, dx 2.3e-05, dw 0.17 (its reduction is 12 terms long)."""
    from wav2letter_amd import ops
    B, Cin, Cout, T, kw = 1, 826, 1816, 40, 29
    rng = np.random.default_rng(826)
    x, w, b = _operands(rng, B, Cin, Cout, T, kw)
    xr, wr = refnet.bf16_round(x), refnet.bf16_round(w)
    xd, wd = dev(to_fm(x)), dev(w_to_dev(w))
    y, imgs, d = ops.conv_bf16(xd, wd, dev(b), 0, 0)
    y_ref = oracle.conv_fwd(xr, wr, b, 1, 0, 0)
    worst = 0.0

    def check(got, want, bound, what):
        nonlocal worst
        err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, ratio)
        print(f"{what}: rel {rel(got, want):.3e}, largest |error| / bound {ratio:.3e}")
        assert (err <= bound).all(), (what, ratio)

    check(from_fm(y.cpu().numpy()), y_ref, kw * Cin * U * oracle.conv_fwd(np.abs(xr), np.abs(wr), np.abs(b), 1, 0, 0).astype(np.float64), "y")
    assert torch.equal(y, ops.conv_bf16(xd, wd, dev(b), 0, 0)[0])
    To = y_ref.shape[3]
    dy = rng.standard_normal(y_ref.shape, dtype=np.float32)
    dyr = refnet.bf16_round(dy)
    odx, odw, odb = oracle.conv_bwd(xr, wr, dyr, 1, 0, 0)
    adx, adw, adb = oracle.conv_bwd(np.abs(xr), np.abs(wr), np.abs(dyr), 1, 0, 0)
    dx, dw, db = ops.conv_bf16_backward(xd, dev(to_fm(dy)), imgs, d, with_bias=True)
    check(from_fm(dx.cpu().numpy()), odx, kw * Cout * U * adx.astype(np.float64), "dx")
    check(dw.cpu().numpy(), w_to_dev(odw), B * To * U * w_to_dev(adw).astype(np.float64), "dw")
    check(db.cpu().numpy(), odb, B * To * U * adb.astype(np.float64), "dbias")
    print(f"largest |error| / bound over the four results: {worst:.3e}")


def test_conv_bf16_returns_none_without_a_kernel():
    from wav2letter_amd import ops
    x = torch.zeros(2, 20, 80, 64, device="cuda")
    assert ops.conv_bf16(x, torch.zeros(5, 64, 64, device="cuda"), None, 2, 2) is None                      # H = 80
    x1 = torch.zeros(2, 20, 1, 64, device="cuda")
    assert ops.conv_bf16(x1, torch.zeros(5, 64, 64, device="cuda"), None, 2, 2, stride=3) is None           # stride 3
    assert ops.conv_bf16(torch.zeros(2, 20, 1, 1, device="cuda"), torch.zeros(5, 1, 64, device="cuda"), None, 2, 2) is None


# ---- the trainer's second level on a conv_glu miniature ------------------------------------------------------------------------
MINI_ARCH = ("V -1 1 NFEAT 0\nWN 3 C NFEAT 64 5 1 0\nGLU 2\nDO 0\nWN 3 C 32 66 6 1 -1\nGLU 2\nDO 0\nWN 3 C 33 48 7 1 0\nGLU 2\nDO 0\n"
             "RO 2 0 3 1\nWN 0 L 24 48\nGLU 0\nWN 0 L 24 NLABEL\n")


def _library_rule(monkeypatch):
    """refnet rounds a convolution's operands where the product multiplies them in bf16: the TDS rule of oracle/refnet.py, or -- at
    the second level -- wherever the library has a wide kernel"""
    from wav2letter_amd import _lib
    tds_rule = refnet.conv_rounds_to_bf16

    def rule(cin, cout, kw, stride, H):
        if tds_rule(cin, cout, kw, stride, H):
            return True
        d = _lib.ConvDesc(1, 64 + kw, H, cin, cout, kw, stride, 0, 0)
        return _lib.lib().w2l_conv_bf16_image_elems(C.byref(d)) != 0
    monkeypatch.setattr(refnet, "conv_rounds_to_bf16", rule)


def test_trainer_level_two_on_a_conv_glu_miniature(oracle, monkeypatch):
    """40 -> 64 -> 66 -> 48 channels (GLU halves them: the convolutions read 40 / 32 / 33), kw 5 / 6 / 7, one SAME-padded layer,
    ASG: loss, emissions and every parameter gradient of level 2 against the reference network that rounds the operands of every
    Linear and every convolution the library has a wide kernel for, at the bar of the bf16-operand full-network tests (2e-3);
    level 1 is what it was (bit for bit, before and after the switch was on and off again, and the switch alone changes
    nothing while the mode is off); level 2 differs from it; evaluate() at level 2 agrees with the training forward at DO 0"""
    from tests.test_gpu_trainer import build
    rng = np.random.default_rng(77)
    nfeat, nlabel, B, T, L = 40, 9, 3, 50, 7
    tr, _, params, A = build(MINI_ARCH, nfeat, nlabel, "asg", 4, 4.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.array([[1, 2, 3, 1, -1, -1, -1], [0, 5, 5, 2, 7, 1, 0], [4, 4, -1, -1, -1, -1, -1]], np.int32)
    xd, td = torch.tensor(x.reshape(B, nfeat, T)).cuda(), torch.tensor(tgt).cuda()

    def step():
        em = tr.forward(xd, train=False).clone()
        loss = tr.forward_backward(xd, td).clone()
        return em, loss, tr.grads.clone()

    fp32 = step()
    tr.set_mixed_precision(False, convs=True)          # the second switch alone: nothing changes
    assert all(torch.equal(a, b) for a, b in zip(fp32, step()))
    tr.set_mixed_precision(True)
    level1 = step()
    tr.set_mixed_precision(True, convs=True)
    level2 = step()
    assert all(torch.equal(a, b) for a, b in zip(level2, step()))                      # deterministic
    assert not torch.equal(level1[0], level2[0]) and not torch.equal(level1[2], level2[2])   # the wide kernels really ran

    _library_rule(monkeypatch)
    ref = refnet.RefNet(MINI_ARCH, nfeat, nlabel, bf16=True)
    em_ref = ref.forward(x, params)
    assert sum(1 for rec in ref.tape if rec[0] == "C" and rec[-1] is True) == 3       # all three convolutions are rounded
    em, loss, grads = level2
    e = rel(em.cpu().numpy(), em_ref)
    print(f"emissions: rel {e:.3e}")
    assert e < 2e-3
    ol, odx, odA = oracle.asg(em_ref, A, tgt, 4)
    e = rel(loss.cpu().numpy(), ol)
    print(f"loss: rel {e:.3e}")
    assert e < 2e-3
    ref_grads = ref.backward(odx.astype(np.float32), len(params))
    g = grads.cpu().numpy()
    table = tr.param_table()
    for i, want in enumerate(ref_grads):
        e = rel(tr.export_from(i, g), np.asarray(want).reshape(-1))
        print(f"gradient {i} {table[i][0]}: rel {e:.3e}")
        assert e < 2e-3, (i, table[i][0], e)
    assert rel(g[tr.n_net:tr.n_net + nlabel * nlabel], np.asarray(odA).reshape(-1)) < 2e-3
    # evaluation (a plan of its own, made with the same switch) against the training forward: DO 0, so the same numbers
    ev_loss, _ = tr.evaluate(xd, td)
    assert rel(ev_loss.cpu().numpy(), loss.cpu().numpy()) < 1e-6
    tr.set_mixed_precision(True, convs=False)          # back to level 1: what it was
    assert all(torch.equal(a, b) for a, b in zip(level1, step()))
    ev1, _ = tr.evaluate(xd, td)
    assert rel(ev1.cpu().numpy(), level1[1].cpu().numpy()) < 1e-6


# ---- drivers ----------------------------------------------------------------------------------------------------------------
def _net(path):
    from wav2letter_amd import checkpoint
    return checkpoint.read(str(path))[1]


def test_drivers_take_the_flag(tmp_path):
    """Train --w2l_amp_convs=true on the six-WAV list fixture with the miniature arch: six updates in one run end where three updates
    + `continue` end, bit for bit (the flag travels in the checkpoint's flags), the run differs from the one without the flag, and
    Decode runs on the checkpoint with the flag"""
    d = tmp_path
    _fixture(d)
    (d / "arch" / "net.arch").write_text(MINI_ARCH.replace("DO 0\n", "DO 0.1\n"))
    amp = ["--fl_amp_use_mixed_precision=true", "--w2l_amp_convs=true"]

    def run(cmd):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=ENV)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        return out.stdout

    text = run(_train_cmd(d, d / "w") + amp)
    assert "wide time convolutions multiply bf16" in text
    run(_train_cmd(d, d / "p") + amp + ["--iter=3"])
    run([_train_cmd(d, d)[0], "continue", str(d / "p" / "exp"), "--iter=6"])
    whole, cont = _net(d / "w/exp/001_model_last.bin"), _net(d / "p/exp/002_model_last.bin")
    assert len(whole) == len(cont) and all(np.array_equal(a, b) for a, b in zip(whole, cont))
    assert "--w2l_amp_convs=true" in (d / "w/exp/001_config").read_text()
    run(_train_cmd(d, d / "l1") + amp[:1])
    level1 = _net(d / "l1/exp/001_model_last.bin")
    assert not all(np.array_equal(a, b) for a, b in zip(whole, level1))
    bad = subprocess.run(_train_cmd(d, d / "bad") + amp[1:], capture_output=True, text=True, timeout=120, env=ENV)
    assert bad.returncode != 0 and "fl_amp_use_mixed_precision" in bad.stdout + bad.stderr
    res = subprocess.run([DECODE_EXE, f"--am={d / 'w/exp/001_model_last.bin'}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}"],
                         capture_output=True, text=True, timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert len((d / "out" / "other.hyp").read_text().splitlines()) == 5
