"""Adam with decoupled weight decay on the GPU, layer by layer: w2l_adam_step_guarded, the trainer's kind 3, checkpoints,
fl::AdamOptimizer and `Train --netoptim=adam`, each against the float64 restatement of the contract (tests/adam_ref.py).

The C ABI carries the hyperparameters as float32; the restatement is evaluated at the float32 values (adam_ref.f32), so the bars
below measure the kernel's arithmetic and not the rounding of 0.999.  Worst errors seen on an MI355X are in DESIGN.md 3.22."""
import functools
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import adam_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = R.f32
LR, B1, B2 = F(0.01), F(0.9), F(0.999)
CASES = {"eps1e-8": (F(1e-8), 0.0), "eps1e-3,wd": (F(1e-3), F(0.1))}
PAD = 8          # floats around every operand: offsets of 0-3 floats move it against 16 bytes, the rest must stay as it was
SENTINEL = 7.25


def stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def problem(n, case):
    """five steps with gradient scales 0.1 + i, and the restatement's states after each -- computed once per (n, case)"""
    eps, wd = CASES[case]
    g = torch.Generator().manual_seed(1000 + n)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (0.1 + i) for i in range(5)]
    want = R.run(p0.numpy(), [x.numpy() for x in grads], LR, B1, B2, eps, wd)
    return p0, grads, want


class Operand:
    """n floats at an offset of `off` floats inside a padded device buffer"""

    def __init__(self, values, off):
        n = values.numel()
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, device="cuda")
        self.lo, self.hi = PAD + off, PAD + off + n
        self.t = self.buf[self.lo:self.hi]
        self.t.copy_(values)
        self.ptr = self.t.data_ptr()

    def untouched_outside(self):
        return bool((self.buf[:self.lo] == SENTINEL).all() and (self.buf[self.hi:] == SENTINEL).all())


def adam_call(L, p, g, m, v, n, eps, wd, step=0, count=None, guard=None, grad_scale=1.0, lr=LR, b1=B1, b2=B2):
    return L.w2l_adam_step_guarded(p.ptr, g.ptr, m.ptr, v.ptr, n, lr, b1, b2, eps, wd, grad_scale, 0.0,
                                   guard.data_ptr() if guard is not None else None, step, count.data_ptr() if count is not None else None,
                                   stream())


def check_state(p, m, v, want, what):
    wp, wm, wv = want[:3]
    ep = np.abs(p.t.cpu().double().numpy() - wp).max()
    em = np.abs(m.t.cpu().double().numpy() - wm).max() / np.abs(wm).max()
    ev = np.abs(v.t.cpu().double().numpy() - wv).max() / np.abs(wv).max()
    print(f"adam {what}: |p - ref| {ep:.3g}  m {em:.3g}  v {ev:.3g} (relative to the largest)")
    assert ep < 1e-5, (what, ep)                  # the siblings' bar (test_optimizer_kernels_against_torch_optim)
    assert em < 1e-6 and ev < 1e-6, (what, em, ev)
    return ep, em, ev


@pytest.mark.parametrize("counter", ["host-step", "device-counter"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("n", [1, 3, 4, 7, 4099])
def test_kernel_follows_the_contract(n, case, counter):
    """1: every pair of offsets (0-3 floats) of p / g against m / v -- the float4 body with its scalar head and tail where the
    phases agree, element by element where they do not --, five steps, t from the host or from the device counter"""
    from wav2letter_amd import _lib
    L = _lib.lib()
    eps, wd = CASES[case]
    p0, grads, want = problem(n, case)
    if case == "eps1e-3,wd":     # the bar tells the contract from eps inside the bias correction
        other = R.run(p0.numpy(), [x.numpy() for x in grads], LR, B1, B2, eps, wd, torch_eps=True)
        assert np.abs(other[-1][0] - want[-1][0]).max() > 1e-4
    worst = (0.0, 0.0, 0.0)
    for p_off in range(4):
        for s_off in range(4):
            p, m, v = Operand(p0, p_off), Operand(torch.zeros(n), s_off), Operand(torch.zeros(n), s_off)
            count = torch.zeros(1, dtype=torch.int64, device="cuda") if counter == "device-counter" else None
            gs = []
            for i, gi in enumerate(grads):
                g = Operand(gi, p_off)
                gs.append(g)
                assert adam_call(L, p, g, m, v, n, eps, wd, step=0 if count is not None else i + 1, count=count) == 0
            worst = tuple(max(a, b) for a, b in zip(worst, check_state(p, m, v, want[-1], f"n={n} {case} {counter} offsets {p_off}/{s_off}")))
            assert all(o.untouched_outside() for o in [p, m, v] + gs)
            assert all(torch.equal(g.t.cpu(), gi) for g, gi in zip(gs, grads))
            assert count is None or count.item() == 5
    print(f"adam kernel worst n={n} {case} {counter}: p {worst[0]:.3g} m {worst[1]:.3g} v {worst[2]:.3g}")


def test_zero_lanes_stay_put():
    """2: 0 / (0 + eps) -- where g, m and v are zero a step leaves p bit-identical (wd = 0: the alignment gaps of a planned
    network's arena), and a zero p stays zero under weight decay"""
    from wav2letter_amd import _lib
    L = _lib.lib()
    n = 4099
    gen = torch.Generator().manual_seed(5)
    p0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    lanes = torch.rand(n, generator=gen) < 0.3
    lanes[[0, 1, 5, n - 1, n - 2]] = True           # in the head, the body and the tail
    g0[lanes] = 0.0
    for wd in (0.0, F(0.1)):
        p_start = p0.clone()
        if wd:
            p_start[lanes] = 0.0
        p, g, m, v = Operand(p_start, 1), Operand(g0, 1), Operand(torch.zeros(n), 1), Operand(torch.zeros(n), 1)
        for step in (1, 2):
            assert adam_call(L, p, g, m, v, n, F(1e-8), wd, step=step) == 0
        got = p.t.cpu()
        assert torch.equal(got[lanes].view(torch.int32), p_start[lanes].view(torch.int32))
        assert (got[~lanes] != p_start[~lanes]).all() and not m.t[lanes].any() and not v.t[lanes].any()


def test_guard_skips_the_step_and_the_count():
    """3: a NaN in the guard slot leaves p, m, v and the device count as they were; the next good step continues the bias
    correction from the last APPLIED step"""
    from wav2letter_amd import _lib
    L = _lib.lib()
    n, case = 4099, "eps1e-8"
    eps, wd = CASES[case]
    p0, grads, _ = problem(n, case)
    gs = [x.numpy() for x in grads[:3]]
    want = R.run(p0.numpy(), gs, LR, B1, B2, eps, wd, skips=[0, 1, 0])
    counted = R.run(p0.numpy(), gs, LR, B1, B2, eps, wd, skips=[0, 1, 0], count_skipped=True)
    assert np.abs(want[-1][0] - counted[-1][0]).max() > 1e-4
    p, m, v = Operand(p0, 0), Operand(torch.zeros(n), 0), Operand(torch.zeros(n), 0)
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    good = torch.tensor([4.0, 0.0], dtype=torch.float64, device="cuda")      # [norm^2, 1 / batch (0: the caller's scale stands)]
    bad = torch.tensor([float("nan"), 0.0], dtype=torch.float64, device="cuda")
    assert adam_call(L, p, Operand(grads[0], 0), m, v, n, eps, wd, count=count, guard=good) == 0
    before = [t.clone() for t in (p.buf, m.buf, v.buf, count)]
    assert adam_call(L, p, Operand(grads[1], 0), m, v, n, eps, wd, count=count, guard=bad) == 0
    assert all(torch.equal(a, b) for a, b in zip(before, (p.buf, m.buf, v.buf, count))) and count.item() == 1
    assert adam_call(L, p, Operand(grads[2], 0), m, v, n, eps, wd, count=count, guard=good) == 0
    check_state(p, m, v, want[-1], "after a skipped step")
    assert count.item() == 2 and want[-1][3] == 2
    assert np.abs(p.t.cpu().double().numpy() - counted[-1][0]).max() > 1e-4      # not the rule that counts the skipped step
    # the host step is the caller's to hold back: a guarded skip with the host step leaves the state alone as well
    before = [t.clone() for t in (p.buf, m.buf, v.buf)]
    assert adam_call(L, p, Operand(grads[1], 0), m, v, n, eps, wd, step=3, guard=bad) == 0
    assert all(torch.equal(a, b) for a, b in zip(before, (p.buf, m.buf, v.buf)))


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
NFEAT, NLABEL, B, T, LT = 8, 7, 3, 30, 4
ADAM = dict(beta1=0.95, beta2=0.99, eps=1e-8, weight_decay=0.05)      # the betas of the recipes' cfgs


def asg_trainer(linseg=0, optim=("adam", "adam"), seed=5, **adam):
    from wav2letter_amd import recipes
    from wav2letter_amd.trainer import Trainer
    tr = Trainer(recipes.conv_glu_small_arch(), NFEAT, NLABEL, "asg", 4, 1.0)
    if linseg:
        tr.set_linseg(linseg)
    tr.init_params(seed)
    tr.plan(B, T, LT)
    tr.to_device()
    tr.set_optimizer(*optim, **adam)
    return tr


def batch(seed):
    rng = np.random.default_rng(seed)
    x = torch.tensor(rng.normal(size=(B, NFEAT, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, NLABEL, size=(B, LT)).astype(np.int32)).cuda()
    return x, tgt


def slices(tr, net, crit):
    out = np.full(tr.n_floats, crit, np.float64)
    out[:tr.n_net] = net
    return out


def test_trainer_updates_follow_the_recurrence():
    """4: --netoptim=adam --critoptim=adam on an ASG network: four updates against the restatement with one global clip
    coefficient, a learning rate per group and the weight decay on the network's slice alone; a non-finite gradient leaves
    parameters, both arenas and both counts untouched; the --linseg hand-over resets the counts with the arenas"""
    x, tgt = batch(21)
    tr = asg_trainer(**ADAM)
    lr, lrcrit, clip = 0.002, 0.0005, 0.05
    ref = R.Adam(tr.params.double().cpu().numpy(), 0.0, F(ADAM["beta1"]), F(ADAM["beta2"]), F(ADAM["eps"]))
    lr_vec, wd_vec = slices(tr, F(lr), F(lrcrit)), slices(tr, F(ADAM["weight_decay"]), 0.0)
    worst = 0.0
    for it in range(4):
        tr.forward_backward(x, tgt)
        g = tr.grads.double().cpu().numpy() / B
        c = min(1.0, clip / (np.linalg.norm(g) + 1e-6))
        assert it > 0 or c < 1.0                       # the clip is live on the first update
        ref.step(g * c, lr=lr_vec, wd=wd_vec)
        tr.update(lr=lr, lrcrit=lrcrit, momentum=0.0, max_grad_norm=clip, total_batch=B)
        err = np.abs(tr.params.double().cpu().numpy() - ref.p).max()
        worst = max(worst, err / max(1.0, np.abs(ref.p).max()))
        print(f"adam trainer update {it}: |p - ref| {err:.3g} (largest |p| {np.abs(ref.p).max():.3g})")
        assert err < 2e-6 * max(1.0, np.abs(ref.p).max()), it        # the Adagrad test's bar
    em = np.abs(tr.mom.double().cpu().numpy() - ref.m).max() / np.abs(ref.m).max()
    ev = np.abs(tr.state2.double().cpu().numpy() - ref.v).max() / np.abs(ref.v).max()
    print(f"adam trainer worst: p {worst:.3g} of max(1, |p|)  m {em:.3g}  v {ev:.3g}")
    assert em < 1e-5 and ev < 1e-4                     # the Adadelta test's bars
    assert tr.adam_steps() == (4, 4)
    before = [t.clone() for t in (tr.params, tr.mom, tr.state2)]
    tr.forward_backward(x, tgt)
    tr.grads[5] = float("nan")
    tr.update(lr=lr, lrcrit=lrcrit, momentum=0.0, max_grad_norm=clip, total_batch=B)
    assert all(torch.equal(a, b) for a, b in zip(before, (tr.params, tr.mom, tr.state2)))
    assert tr.adam_steps() == (4, 4) and tr.skipped_updates() == 1

    # --linseg=2: the hand-over update starts from fresh optimizer state.  With that update skipped, what the reset left is visible
    ls = asg_trainer(linseg=2, **ADAM)
    for _ in range(2):
        ls.forward_backward(x, tgt)
        ls.update(lr=lr, lrcrit=lrcrit, max_grad_norm=clip, total_batch=B)
    assert ls.adam_steps() == (2, 2) and ls.mom.abs().max().item() > 0 and ls.state2.abs().max().item() > 0
    ls.forward_backward(x, tgt)
    ls.grads[5] = float("nan")
    ls.update(lr=lr, lrcrit=lrcrit, max_grad_norm=clip, total_batch=B)
    assert ls.adam_steps() == (0, 0) and not ls.mom.any() and not ls.state2.any()
    fresh = R.Adam(ls.params.double().cpu().numpy(), 0.0, F(ADAM["beta1"]), F(ADAM["beta2"]), F(ADAM["eps"]))
    ls.forward_backward(x, tgt)
    g = ls.grads.double().cpu().numpy() / B
    fresh.step(g * min(1.0, clip / (np.linalg.norm(g) + 1e-6)), lr=lr_vec, wd=wd_vec)
    ls.update(lr=lr, lrcrit=lrcrit, max_grad_norm=clip, total_batch=B)
    assert ls.adam_steps() == (1, 1)
    assert np.abs(ls.params.double().cpu().numpy() - fresh.p).max() < 2e-6 * max(1.0, np.abs(fresh.p).max())


def test_weight_decay_acts_on_the_network_alone_and_kinds_mix():
    """4 (the decay's reach) and the mixed kinds: the same update with and without weight decay moves the criterion's slice
    identically and the network's differently; network adam with criterion sgd steps the transitions by -lrcrit g"""
    x, tgt = batch(22)
    kw = dict(lr=0.002, lrcrit=0.0005, max_grad_norm=0.0, total_batch=B)
    a, b = asg_trainer(**ADAM), asg_trainer(**dict(ADAM, weight_decay=0.0))
    for tr in (a, b):
        tr.forward_backward(x, tgt)
        tr.update(**kw)
    n = a.n_net
    assert torch.equal(a.params[n:], b.params[n:]) and not torch.equal(a.params[:n], b.params[:n])
    assert torch.equal(a.mom, b.mom) and torch.equal(a.state2, b.state2)          # decoupled: the moments never see the decay
    m = asg_trainer(optim=("adam", "sgd"), **ADAM)
    p0 = m.params.clone()
    m.forward_backward(x, tgt)
    g = m.grads.clone()
    m.update(**kw)
    want = p0[n:].double() - 0.0005 * g[n:].double() / B
    assert (m.params[n:].double() - want).abs().max().item() < 1e-6 * max(1.0, want.abs().max().item())
    assert torch.equal(m.params[:n], a.params[:n]) and m.adam_steps() == (1, 0)


def test_kind_3_without_the_second_arena_is_refused():
    """5"""
    from wav2letter_amd._lib import W2LInvalidArgument
    x, tgt = batch(23)
    tr = asg_trainer(optim=("sgd", "sgd"))
    assert tr.L.w2l_trainer_set_optimizer(tr.h, 3, 3) == 0      # behind the wrapper's back: no second arena bound
    tr.forward_backward(x, tgt)
    with pytest.raises(W2LInvalidArgument, match="w2l_trainer_bind_state2"):
        tr.update(lr=0.002, lrcrit=0.0005, total_batch=B)


def parent_container(trainer, arch_text, criterion, step, optim):
    """the W2LAMD01 file as the code before Adam wrote it (wav2letter_amd/checkpoint.py): the same keys in the same order"""
    host = trainer.params.detach().cpu().numpy()
    tensors, blobs = [], []
    for i, (name, numel, _) in enumerate(trainer.param_table()):
        tensors.append({"name": name, "kind": "network", "numel": int(numel), "shape": [int(numel)]})
        blobs.append(np.ascontiguousarray(trainer.export_from(i, host), np.float32))
    n = trainer.nlabel
    tensors.append({"name": "criterion.transitions", "kind": "criterion", "numel": n * n, "shape": [n, n]})
    blobs.append(np.ascontiguousarray(host[trainer.n_net:trainer.n_net + n * n], np.float32))
    tensors.append({"name": "netoptim.momentum(internal arena)", "kind": "momentum", "numel": int(trainer.n_floats), "shape": [int(trainer.n_floats)]})
    blobs.append(trainer.mom.detach().cpu().numpy())
    header = json.dumps({"nfeat": trainer.nfeat, "nlabel": trainer.nlabel, "criterion": criterion, "optim": list(optim),
                         "arch_sha256": hashlib.sha256(arch_text.encode()).hexdigest(), "step": int(step), "flags": {},
                         "tensors": tensors}).encode()
    raw = b"W2LAMD01" + struct.pack("<I", len(header)) + header
    for b in blobs:
        raw += b"\0" * (-len(raw) % 16) + b.tobytes()
    return raw


def test_checkpoint_resumes_adam_bit_for_bit(tmp_path):
    """6: two updates, save, load into a fresh trainer, two more == four uninterrupted ones, in parameters, both arenas and the
    counts; an Adagrad file keeps the bytes it always had"""
    from wav2letter_amd import checkpoint, recipes
    arch = recipes.conv_glu_small_arch()
    x, tgt = batch(24)
    kw = dict(lr=0.002, lrcrit=0.0005, max_grad_norm=0.05, total_batch=B)

    def steps(tr, k):
        for _ in range(k):
            tr.forward_backward(x, tgt)
            tr.update(**kw)
    whole, first = asg_trainer(**ADAM), asg_trainer(**ADAM)
    steps(whole, 4)
    steps(first, 2)
    path = str(tmp_path / "adam.w2l")
    checkpoint.save(path, first, arch, "asg", step=2)
    hdr, arrays = checkpoint.read(path)
    assert hdr["optim"] == ["adam", "adam"] and [t["kind"] for t in hdr["tensors"]][-2:] == ["momentum", "state2"]
    assert hdr["adam"] == dict(beta1=0.95, beta2=0.99, eps=1e-8, weight_decay=0.05, steps=[2, 2])
    assert np.array_equal(arrays[-2], first.mom.cpu().numpy()) and np.array_equal(arrays[-1], first.state2.cpu().numpy())
    from wav2letter_amd.trainer import Trainer
    sgd = Trainer(arch, NFEAT, NLABEL, "asg", 4, 1.0)
    with pytest.raises(ValueError):
        checkpoint.load(path, sgd, arch)               # still an SGD trainer
    second = Trainer(arch, NFEAT, NLABEL, "asg", 4, 1.0)
    second.set_optimizer("adam", "adam")               # the hyperparameters come from the file
    assert checkpoint.load(path, second, arch) == 2    # the natural order: load() before to_device()
    second.plan(B, T, LT)
    second.to_device()
    assert second.adam_steps() == (2, 2) and second._adam == first._adam
    assert torch.equal(second.mom, first.mom) and torch.equal(second.state2, first.state2) and torch.equal(second.params, first.params)
    steps(second, 2)
    assert torch.equal(second.params, whole.params) and torch.equal(second.mom, whole.mom) and torch.equal(second.state2, whole.state2)
    assert second.adam_steps() == whole.adam_steps() == (4, 4)
    ada = asg_trainer(optim=("adagrad", "adagrad"))
    steps(ada, 1)
    other = str(tmp_path / "adagrad.w2l")
    checkpoint.save(other, ada, arch, "asg", step=1)
    assert open(other, "rb").read() == parent_container(ada, arch, "asg", 1, ("adagrad", "adagrad"))


def test_cpp_optimizer_flat_and_per_parameter(tmp_path):
    """7: fl::AdamOptimizer through tests/cpp/adam_caller.cpp: the flat path over a planned fl::Sequential and the per-parameter
    path on copies agree bit for bit (checked in the caller) and with the restatement at the kernel test's bars; three steps on
    CPCCriterion::params() change every parameter that has a gradient"""
    exe = str(tmp_path / "adam_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "adam_caller.cpp"),
                    "-o", exe, "-L" + libdir, "-lw2l_hip", "-Wl,-rpath," + libdir, "-ldl"], check=True)
    lr, b1, b2, eps, wd = F(0.003), F(0.95), F(0.99), F(1e-3), F(0.1)
    outp = tmp_path / "out.bin"
    out = subprocess.run([exe, str(outp)] + [repr(v) for v in (lr, b1, b2, eps, wd)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "adam caller ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
    raw = outp.read_bytes()
    n_params, n_steps = np.frombuffer(raw, np.int32, 2)
    sizes = np.frombuffer(raw, np.int32, n_params, 8)
    total = int(sizes.sum())
    data = np.frombuffer(raw, np.float32, -1, 8 + 4 * n_params)
    assert n_steps == 3 and data.size == total * (1 + 4 * n_steps)
    ref = R.Adam(data[:total], lr, b1, b2, eps, wd)
    for t in range(n_steps):
        g, p, m, v = data[total * (1 + 4 * t):total * (5 + 4 * t)].reshape(4, total)
        assert np.abs(g).max() > 0
        ref.step(g)
        ep = np.abs(p - ref.p).max()
        em, ev = np.abs(m - ref.m).max() / np.abs(ref.m).max(), np.abs(v - ref.v).max() / np.abs(ref.v).max()
        print(f"adam c++ step {t}: p {ep:.3g} m {em:.3g} v {ev:.3g}")
        assert ep < 1e-5 and em < 1e-6 and ev < 1e-6, (t, ep, em, ev)


def test_train_binary_runs_adam_and_continues_bit_identically(tmp_path):
    """8: `Train --netoptim=adam --critoptim=adam --adambeta1 --adambeta2 --weightdecay`: the optimizer lines, and three updates,
    stop, continue to five == five uninterrupted updates bit for bit (network, both moments, the step counts)"""
    from tests.test_gpu_fl_compat import _TINY_ARCH, _tiny_train_cmd
    from wav2letter_amd import checkpoint
    exe = os.path.join(ROOT, "wav2letter_amd", "bin", "Train")
    d = tmp_path
    os.makedirs(d / "arch")
    open(d / "arch" / "net.arch", "w").write(_TINY_ARCH)
    opt = ["--netoptim=adam", "--critoptim=adam", "--adambeta1=0.95", "--adambeta2=0.99", "--weightdecay=0.01", "--lr=0.002"]

    def run(cmd):
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
        return out.stdout
    text = run(_tiny_train_cmd(d, d / "A", 5, opt))
    assert "[Network Optimizer] Adam (beta1=0.95) (beta2=0.99) (epsilon=1e-08) (weight decay=0.01)" in text
    assert "[Criterion Optimizer] Adam (beta1=0.95) (beta2=0.99) (epsilon=1e-08)\n" in text      # the criterion's gets no decay
    run(_tiny_train_cmd(d, d / "B", 3, opt))
    text = run([exe, "continue", str(d / "B" / "exp"), "--w2l_synth_updates=5"])
    assert "Loaded model for continue training" in text and "[Network Optimizer] Adam (beta1=0.95)" in text
    ha, ta = checkpoint.read(str(d / "A" / "exp" / "001_model_last.bin"))
    hb, tb = checkpoint.read(str(d / "B" / "exp" / "002_model_last.bin"))
    h3, t3 = checkpoint.read(str(d / "B" / "exp" / "001_model_last.bin"))
    assert ha["step"] == hb["step"] == 5 and ha["optim"] == hb["optim"] == ["adam", "adam"]
    kinds = [t["kind"] for t in ha["tensors"]]
    assert kinds == [t["kind"] for t in hb["tensors"]] and kinds[-2:] == ["momentum", "state2"]
    assert ha["adam"] == hb["adam"] == dict(beta1=0.95, beta2=0.99, eps=1e-8, weight_decay=0.01, steps=[5, 5]) and h3["adam"]["steps"] == [3, 3]
    for t, a, b in zip(ha["tensors"], ta, tb):
        assert np.array_equal(a, b), t["name"]
    assert not np.array_equal(t3[0], ta[0]) and np.abs(ta[-1]).max() > 0 and np.abs(ta[-2]).max() > 0
    # the Python side resumes the C++ run's file: optimizer, hyperparameters and counts
    from wav2letter_amd.trainer import Trainer
    tr = Trainer(_TINY_ARCH, 8, 12, "ctc", 4)
    tr.set_optimizer("adam", "adam")
    assert checkpoint.load(str(d / "A" / "exp" / "001_model_last.bin"), tr, _TINY_ARCH) == 5
    assert tr._adam == (0.95, 0.99, 1e-8, 0.01) and tr.adam_steps() == (5, 5)
    bad = subprocess.run(_tiny_train_cmd(d, d / "C", 1, ["--netoptim=novograd"]), capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "unsupported optimizer 'novograd' (this build: sgd, adagrad, adadelta, adam)" in bad.stderr
