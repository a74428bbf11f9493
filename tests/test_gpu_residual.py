"""Residual blocks (arch tokens RES / SKIP / SKIPL) on the GPU: the ResNet-CTC recipe in miniature against the float64
restatement (tests/residual_ref.py), and the properties of the container -- composition out of its layers and the join kernels, the
folded ReLU, dropout streams, the weight-gradient stream, re-planning, checkpoints, the Train / Decode tools."""
import os
import subprocess

import numpy as np
import pytest
import torch

import residual_ref as R
from tests.list_fixture import ENV, ROOT, _fixture, _train_cmd
from wav2letter_amd import _lib, checkpoint
from wav2letter_amd.criterion import CriterionScaleMode
from wav2letter_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
NFEAT, N, B, T, L = 8, 11, 3, 37, 3
TOL = 1e-4            # BASELINE's fp32 bar: of the largest reference magnitude of the tensor
KINK_MARGIN = 1e-4    # no ReLU input of the restatement within this many rms of zero (asserted)
SIZES = [37, 30, 23]  # ragged utterances inside the padded batch (frames)
TARGET_LENS = [3, 2, 1]
DECODE_EXE = os.path.join(ROOT, "wav2letter_amd", "bin", "Decode")


def mini_arch(drop="0", skip="SKIP 0 10 0.70711", after=("R", "DO {drop}", "LN 0 1 2"), c=16):
    """the recipe in miniature: strided front convolution, one block of three convolutions, max-pool, 1 x 1 output convolution"""
    post = ["R", f"DO {drop}", "LN 0 1 2"]
    conv = f"C {c} {c} 3 1 -1 1"
    lines = ["V -1 1 NFEAT 0", f"C NFEAT {c} 3 2 -1 1"] + post + ["RES 9 1 1", conv] + post + [conv] + post + [conv, skip]
    lines += [a.format(drop=drop) for a in after] + ["M 2 1 2 1", f"C {c} NLABEL 1 1 -1 1", "RO 2 0 3 1"]
    return "\n".join(lines) + "\n"


SKIPL_ARCH = ("V -1 1 NFEAT 0\nC NFEAT 16 3 1 -1 1\nRES 4 1 1\nC 16 24 3 1 -1 1\nR\nDO 0\nC 24 24 3 1 -1 1\nSKIPL 0 5 1 0.7071\nC 16 24 1 1 -1 1\n"
              "R\nM 2 1 2 1\nC 24 NLABEL 1 1 -1 1\nRO 2 0 3 1\n")
# a WeightNorm Linear projection in the (C, T, B, 1) layout between two RO lines, as the ConvLM blocks are written
WN_ARCH = ("V -1 1 NFEAT 0\nC NFEAT 16 3 1 -1 1\nRO 2 0 3 1\nRES 3 1 1\nWN 0 L 16 24\nR\nWN 0 L 24 24\nSKIPL 0 4 1 0.7071\nWN 0 L 16 24\n"
           "RO 1 3 0 2\nR\nM 2 1 2 1\nC 24 NLABEL 1 1 -1 1\nRO 2 0 3 1\n")


def shapes_of(arch):
    """ArrayFire dims of the parameters in table order: the arch lines in order (a projection's lines follow their SKIPL line)"""
    out = []
    for f in R.parse(arch, NFEAT, N):
        if f[0] == "C":
            cin, cout, kw = int(f[1]), int(f[2]), int(f[3])
            out += [(kw, 1, cin, cout), (1, 1, cout, 1)]
        elif f[0] == "WN":
            out += [(int(f[4]), int(f[3])), (int(f[4]), 1), (int(f[4]),)]
        elif f[0] == "L":
            out += [(int(f[2]), int(f[1])), (int(f[2]),)]
        elif f[0] == "LN":
            out += [(2,)]
    return out


def make_trainer(arch, seed=3, nfeat=NFEAT, nlabel=N, shape=(B, T, L)):
    tr = Trainer(arch, nfeat, nlabel, "ctc", CriterionScaleMode.TARGET_SZ_SQRT)
    tr.init_params(seed)
    rng = np.random.default_rng(seed)
    for i, (name, n, off) in enumerate(tr.param_table()):
        if name.startswith("ln."):                       # gamma, beta away from (1, 0)
            tr.import_param(i, np.array([1 + 0.2 * rng.normal(), 0.2 * rng.normal()], np.float32))
        elif name.endswith(".b"):                        # biases of a size that matters
            tr.import_param(i, (0.2 * rng.normal(size=n)).astype(np.float32))
    tr.to_device()
    tr.plan(*shape)
    return tr


def batch(seed, shape=(B, T, L), nfeat=NFEAT, nlabel=N):
    b, t, l = shape
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(b, nfeat, t)).astype(np.float32)
    sizes = ([t] + SIZES[1:] + [t] * b)[:b]
    for k, s in enumerate(sizes):
        x[k, :, min(s, t):] = 0                          # the padding behind a short utterance
    tgt = np.full((b, l), -1, np.int32)
    for k in range(b):
        n = min(TARGET_LENS[k % 3], l)
        tgt[k, :n] = rng.permutation(nlabel - 1)[:n]      # distinct labels: every target fits its frames
    return x, tgt, np.array(sizes, np.float32)


def ref_pass(arch, tr, x, tgt):
    """the restatement on the trainer's parameters: (net, params, x tensor, emission, loss) after loss.sum().backward()"""
    params = R.to_torch([tr.export_from(i, tr.host_params) for i in range(len(tr.param_table()))], shapes_of(arch))
    net = R.Net(arch, NFEAT, N)
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    em = net.forward(xt, params)
    loss = R.ctc_loss(em, tgt)
    loss.sum().backward()
    return net, params, xt, em, loss


def kink_margin(net):
    return min(float(a.detach().abs().min() / a.detach().pow(2).mean().sqrt()) for a in net.pre_relu)


def kink_free(arch, tr):
    """a batch none of whose ReLU inputs lies within KINK_MARGIN rms of zero in the restatement (tests/test_gpu_trainer.py's rule:
    the margin is asserted, then nothing is excused)"""
    best = None
    for seed in range(100, 160):
        x, tgt, sizes = batch(seed)
        ref = ref_pass(arch, tr, x, tgt)
        m = kink_margin(ref[0])
        if best is None or m > best[0]:
            best = (m, x, tgt, sizes, ref)
        if m >= KINK_MARGIN:
            break
    assert best[0] >= KINK_MARGIN, ("no kink-free batch found", best[0])
    return best[1:]


def gpu_pass(tr, x, tgt, sizes=None):
    """one forward_backward: (loss, emission, parameter gradients in reference layout, input gradient [B][NFEAT][T])"""
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()
    if sizes is not None:
        tr.set_input_sizes(torch.from_numpy(sizes).cuda())
    tr.set_input_gradient(True)
    loss = tr.forward_backward(xd, td).cpu().numpy().copy()
    torch.cuda.synchronize()
    dx = tr.input_gradient().cpu().numpy().transpose(0, 2, 1).copy()
    g = tr.grads.cpu().numpy()
    grads = [tr.export_from(i, g) for i in range(len(tr.param_table()))]
    em = tr.forward(xd, train=True).cpu().numpy().copy()
    return loss, em, grads, dx


def rel(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30)


def check_against_restatement(arch):
    tr = make_trainer(arch)
    x, tgt, sizes, (net, params, xt, em, loss) = kink_free(arch, tr)
    gl, gem, ggrads, gdx = gpu_pass(tr, x, tgt, sizes)
    figures = {"loss": rel(gl, loss.detach().numpy()), "emission": rel(gem, em.detach().numpy()), "dx": rel(gdx, xt.grad.numpy())}
    for i, (p, g) in enumerate(zip(params, ggrads)):
        figures[f"grad {i} {tr.param_table()[i][0]}"] = rel(g, p.grad.numpy().reshape(-1))
    print(figures)
    assert np.isfinite(gl).all() and (gl > 0).all()
    for k, v in figures.items():
        assert v < TOL, (k, v)


# ---- (a) parity with the restatement ----------------------------------------------------------------------------------------------
def test_mini_recipe_against_restatement():
    """(a) CTC loss, emissions, input gradient and every parameter gradient of the miniature recipe (NFEAT 8, 11 labels, B 3, T 37:
    19 frames behind the stride-2 SAME convolution, 9 behind the pool's floor; ragged utterances, zero-padded, with their sizes set --
    a convolutional network ignores them, as the reference's does -- and ragged targets), each within 1e-4 of the largest reference
    magnitude of that tensor, on a batch with an asserted ReLU margin"""
    check_against_restatement(mini_arch())


# ---- (b) composition -------------------------------------------------------------------------------------------------------------
C_B = 32   # channels of the isolated block: the second mixed-precision level takes time convolutions from 32 channels on
BODY = ["C 32 32 3 1 -1 1", "R", "DO 0", "LN 0 1 2", "C 32 32 3 1 -1 1", "R", "DO 0", "LN 0 1 2", "C 32 32 3 1 -1 1"]


def _isolated(lines, mixed):
    tr = make_trainer("\n".join(["V -1 1 NFEAT 0"] + lines + ["RO 2 0 3 1"]) + "\n", seed=5, nfeat=C_B, nlabel=C_B)
    if mixed:
        tr.set_mixed_precision(True, convs=mixed == 2)
    tr.set_input_gradient(True)
    return tr


def _run_isolated(tr, x, dy):
    y = tr.forward(torch.from_numpy(x).cuda(), train=True).clone()
    tr.backward(dy)
    torch.cuda.synchronize()
    return y, tr.grads.clone(), tr.input_gradient().clone()


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("mixed", [0, 1, 2])
def test_block_is_its_layers_and_the_join(mixed, relu):
    """(b) the block's output, parameter gradients and input gradient equal, bit for bit, its layers run as a plain network on the
    same parameters, followed by w2l_residual_join_forward / _backward and w2l_axpy called by hand -- in fp32 and at both
    mixed-precision levels, with and without the folded ReLU"""
    Lk = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    scale = 0.70711
    blk = _isolated(["RES 9 1 1"] + BODY + [f"SKIP 0 10 {scale}"] + (["R"] if relu else []), mixed)
    plain = _isolated(BODY, mixed)
    assert blk.param_table() == plain.param_table()
    rng = np.random.default_rng(17)
    x = rng.normal(size=(B, C_B, T)).astype(np.float32)
    dy = torch.from_numpy(rng.normal(size=(B, T, C_B)).astype(np.float32)).cuda()
    y, grads, dx = _run_isolated(blk, x, dy.clone())
    # by hand
    n = B * T * C_B
    xfm = torch.from_numpy(x).cuda().transpose(1, 2).contiguous()          # the input as the network holds it: frame-major
    fx = plain.forward(torch.from_numpy(x).cuda(), train=True)
    y2 = torch.empty_like(fx)
    assert Lk.w2l_residual_join_forward(y2.data_ptr(), fx.data_ptr(), xfm.data_ptr(), n, scale, relu, s) == 0
    g = torch.empty_like(fx)
    assert Lk.w2l_residual_join_backward(g.data_ptr(), dy.data_ptr(), y2.data_ptr(), n, scale, relu, s) == 0
    plain.backward(g.clone())
    dx2 = plain.input_gradient().clone()
    assert Lk.w2l_axpy(dx2.data_ptr(), g.data_ptr(), n, 1.0, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32))
    assert torch.equal(grads.view(torch.int32), plain.grads.view(torch.int32))
    assert torch.equal(dx.view(torch.int32), dx2.view(torch.int32))
    assert float(grads.abs().max()) > 0 and float(dx.abs().max()) > 0 and bool(torch.isfinite(y).all())
    if relu:
        assert float((y == 0).float().mean()) > 0.2


# ---- (c) SKIPL -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", [SKIPL_ARCH, WN_ARCH], ids=["conv-projection", "weightnorm-linear-projection"])
def test_projection_shortcut_against_restatement(arch):
    """(c) SKIPL with a 1 x 1 convolution 16 -> 24, and with a WeightNorm Linear in the (C, T, B, 1) layout between two RO lines"""
    check_against_restatement(arch)


@pytest.mark.parametrize("arch", [SKIPL_ARCH, WN_ARCH])
def test_block_without_its_projection_is_refused_for_its_shape(arch):
    lines = arch.splitlines()
    k = next(i for i, l in enumerate(lines) if l.startswith("SKIPL"))
    bad = lines[:k] + [f"SKIP 0 {lines[k].split()[2]} 0.7071"] + lines[k + 2:]
    with pytest.raises(_lib.W2LInvalidArgument, match="differ in shape or layout.*SKIP 0"):
        Trainer("\n".join(bad) + "\n", NFEAT, N, "ctc")


# ---- (d) the R fold ---------------------------------------------------------------------------------------------------------------
def test_folded_relu_equals_the_relu_layer():
    """(d) the `R` line behind the block folded into the join, against the same network with a `DO 0` in between so that it stays
    a layer: bit for bit"""
    x, tgt, _ = batch(7)
    folded = make_trainer(mini_arch())
    apart = make_trainer(mini_arch(after=("DO 0", "R", "DO {drop}", "LN 0 1 2")))
    assert "ReLU" not in folded.describe() and apart.describe().count("ReLU") == 1      # (the R lines behind convolutions fold either way)
    a, b = gpu_pass(folded, x, tgt), gpu_pass(apart, x, tgt)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(p, q) for p, q in zip(a[2], b[2]))


# ---- (e) dropout -----------------------------------------------------------------------------------------------------------------
def test_dropout_in_the_block():
    """(e) DO 0.2 in train mode: two trainers at the same seed and step agree bit for bit and another step differs; the DO layers of
    one block draw different masks; eval mode ignores them.  The mask check is a block of two DO 0.5 lines on an input of ones --
    y = drop(drop(1)) + 1 is 5 where both layers keep the element: a quarter of the elements with two masks, half with one (and the
    block's first layer rewrites its input in place: the shortcut reads its own copy)"""
    x, tgt, _ = batch(9)
    arch = mini_arch(drop="0.2")
    runs = []
    for step in (4, 4, 5):
        tr = make_trainer(arch)
        tr.set_step(step)
        runs.append(gpu_pass(tr, x, tgt))
    assert np.array_equal(runs[0][0], runs[1][0]) and all(np.array_equal(p, q) for p, q in zip(runs[0][2], runs[1][2]))
    assert not np.array_equal(runs[0][0], runs[2][0])
    ev = make_trainer(arch)
    plain = make_trainer(mini_arch())
    xd = torch.from_numpy(x).cuda()
    assert torch.equal(ev.forward(xd, train=False), plain.forward(xd, train=False))
    assert not torch.equal(ev.forward(xd, train=True), plain.forward(xd, train=True))
    # (a network needs a parameter: a 1 x 1 convolution with the identity for its weight hands the block's output on bit for bit)
    two = make_trainer("V -1 1 NFEAT 0\nRES 2 1 1\nDO 0.5\nDO 0.5\nSKIP 0 3\nC 16 16 1 1 -1 1\nRO 2 0 3 1\n", nfeat=16, nlabel=16)
    two.import_param(0, np.eye(16, dtype=np.float32))
    two.import_param(1, np.zeros(16, np.float32))
    two.to_device()
    ones = torch.ones(B, 16, T, device="cuda")
    y = two.forward(ones, train=True).cpu().numpy()
    assert set(np.unique(y)) == {1.0, 5.0}
    kept = float((y == 5).mean())                        # 1776 elements: 0.25 +- 0.01 with independent masks
    assert 0.2 < kept < 0.3, kept
    assert (two.forward(ones, train=False).cpu().numpy() == 2.0).all()


# ---- (f) weight-gradient stream ----------------------------------------------------------------------------------------------------
def test_weight_gradient_stream_on_equals_off():
    """(f) three SGD steps with the weight-gradient stream on against off: losses and parameters bit for bit (the block's g is the
    output gradient of its last convolution's filter gradient, which runs on the side stream)"""
    out = []
    for on in (True, False):
        tr = make_trainer(mini_arch(drop="0.1"))
        tr.set_weight_grad_stream(on)
        losses = []
        for k in range(3):
            x, tgt, _ = batch(20 + k)
            tr.set_step(k)
            losses.append(tr.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()).cpu().numpy().copy())
            tr.update(0.05, momentum=0.5, max_grad_norm=1.0)
        out.append((np.stack(losses), tr.params.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.isfinite(out[0][1]).all()


# ---- (g) re-planning ---------------------------------------------------------------------------------------------------------------
def test_replanned_trainer_equals_fresh_ones():
    """(g) one trainer planned through three (B, T, L) shapes against a fresh trainer per shape: bit for bit"""
    arch = mini_arch()
    shapes = [(3, 37, 3), (2, 64, 2), (1, 21, 1)]
    one = make_trainer(arch, shape=shapes[0])
    for k, shape in enumerate(shapes):
        if k:
            one.plan(*shape)
        x, tgt, _ = batch(30 + k, shape)
        a = gpu_pass(one, x, tgt)
        b = gpu_pass(make_trainer(arch, shape=shape), x, tgt)
        assert a[1].shape == b[1].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]), shape
        assert all(np.array_equal(p, q) for p, q in zip(a[2], b[2])), shape


# ---- (h) checkpoints -------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(tmp_path):
    """(h) save after two steps, load into a fresh trainer, and both take the same third step"""
    arch = mini_arch(drop="0.1")
    tr = make_trainer(arch)
    for k in range(2):
        x, tgt, _ = batch(40 + k)
        tr.set_step(k)
        tr.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda())
        tr.update(0.05, momentum=0.5)
    path = str(tmp_path / "res.bin")
    checkpoint.save(path, tr, arch, "ctc", step=2)
    fresh = Trainer(arch, NFEAT, N, "ctc", CriterionScaleMode.TARGET_SZ_SQRT)
    assert checkpoint.load(path, fresh, arch) == 2
    fresh.to_device()
    fresh.plan(B, T, L)
    assert torch.equal(fresh.params, tr.params) and torch.equal(fresh.mom, tr.mom)
    x, tgt, _ = batch(42)
    out = []
    for t in (tr, fresh):
        t.set_step(2)
        loss = t.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()).cpu().numpy().copy()
        t.update(0.05, momentum=0.5)
        out.append((loss, t.params.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    with pytest.raises(Exception):
        checkpoint.load(path, Trainer(mini_arch(), NFEAT, N, "ctc"), mini_arch())   # another arch text: refused by its hash


# ---- (i) the tools ---------------------------------------------------------------------------------------------------------------
def test_train_continue_and_decode(tmp_path):
    """(i) `Train train` on the six-WAV list fixture for six updates with a finite loss; three updates + `Train continue` end where
    the six end, bit for bit; Decode loads the checkpoint"""
    d = tmp_path
    _fixture(d)
    (d / "arch" / "net.arch").write_text(mini_arch(drop="0.1", c=32))

    def run(cmd):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=ENV)
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        return out.stdout

    text = run(_train_cmd(d, d / "w"))
    assert "Residual" in text
    losses = [float(item.split(":")[1]) for line in text.splitlines() if line.startswith("epoch:") for item in line.split(" | ")
              if item.strip().startswith("loss")]
    assert losses and np.isfinite(losses).all()
    run(_train_cmd(d, d / "p") + ["--iter=3"])
    run([_train_cmd(d, d)[0], "continue", str(d / "p" / "exp"), "--iter=6"])
    whole, cont = checkpoint.read(str(d / "w/exp/001_model_last.bin"))[1], checkpoint.read(str(d / "p/exp/002_model_last.bin"))[1]
    assert len(whole) == len(cont) and all(np.array_equal(a, b) for a, b in zip(whole, cont))
    res = subprocess.run([DECODE_EXE, f"--am={d / 'w/exp/001_model_last.bin'}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}"],
                         capture_output=True, text=True, timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert len((d / "out" / "other.hyp").read_text().splitlines()) == 5
