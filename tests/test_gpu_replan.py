"""One trainer through a SEQUENCE of batch shapes -- what a training run does on every batch -- against trainers planned once.

The statement: trainer A has been planned through shapes S1, S2, ... with a pass taken at each; trainer F is fresh, planned once at
Si, with the same parameters, optimizer state and step count.  On a batch of shape Si both produce THE SAME BITS: eval-mode
emissions, per-utterance loss, every network and criterion gradient, and parameters / optimizer state after an update.  The bar is
derived, not measured: same kernels, same values, same order, and the library has no atomics on these nets.  Each comparison first
runs its control -- two fresh trainers at Si agree bit for bit -- so a difference between A and F is the plan's, not the kernels'.

What a plan could leave behind lives in the layers of csrc/host/net.cpp and in csrc/host/trainer.cpp: arena offsets, bf16 image
sizes and the once-per-arena notes of their padding and ones rows, `uOnlyImages`, the recorded forward pass, LayerNorm scratch whose
size follows the group size, the criterion workspace, the level-2 convolution weight images, the guard accumulators, the input
sizes.  Every sequence below has six entries; B, T and L each grow and shrink; the first shape comes back twice (some state only
bites on the second visit).

Cases (the flips each sequence was chosen for are at its definition):
  R1  TDS-CTC small, dropout 0.3, fp32, weight-gradient stream on / off
  R2  TDS with utterance-sized LayerNorm groups across the three LayerNorm kernel families
  R3  streaming-style TDS (per-frame LayerNorm, H = 16), mixed precision level 1
  R4  conv_glu small with WN, ASG with a two-update linseg warm-up; fp32, level 1, level 2
  R5  Transformer, CTC, fp32 and bf16, ragged input sizes given again after each plan
Two forms: (a) fixed parameters, F rebuilt per shape; (b) a six-step training run that re-plans one trainer per step against a run
that saves a checkpoint after every step and continues it in a NEW trainer planned once (checkpoint.save / load continue bit for
bit: tests/test_gpu_trainer.py), under SGD with momentum, Adadelta and Adam.

Then: the skipped-update count and the last norm survive a plan; input sizes do not; Trainer.evaluate over more shapes than it
keeps planned; the fl:: surface through tests/cpp/replan_caller.cpp."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from wav2letter_amd import recipes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TR_ARCH = ("V -1 1 NFEAT 0\nWN 3 C NFEAT 64 3 1 -1\nGLU 2\nDO 0.0\nM 1 1 2 1\nRO 2 0 3 1\n"
           "TR 32 64 4 9 0.0 0.0\nTR 32 64 4 9 0.0 0.0\nL 32 NLABEL\n")     # of test_transformer_padding_mask_from_input_sizes

# per-frame LayerNorm, asymmetric padding, right-padded TDS blocks: the streaming recipe's lines at H = 16.  The second block's
# hidden width 30 (l2 % 4 != 0) is one whose lin1 cannot write u as images (FeedForward::uOnlyImages off: fp32 u + conversion);
# the others can -- whether it can is decided by the widths alone, so every plan holds blocks of both kinds
STREAM_ARCH = ("V -1 NFEAT 1 0\n"
               "PD 0 5 3\nC2 1 4 10 1 2 1 0 0\nR\nDO 0.1\nLN 1 2\nTDS 4 9 16 0.1 0 1 0\nTDS 4 9 16 0.1 30 1 0\n"
               "PD 0 7 1\nC2 4 6 10 1 2 1 0 0\nR\nDO 0.1\nLN 1 2\nTDS 6 9 16 0.1 0 0 0\n"
               "RO 2 1 0 3\nV 96 -1 1 0\nL 96 NLABEL\nV NLABEL 0 -1 1\n")


class Case:
    def __init__(self, name, arch, nfeat, nlabel, seq, crit="ctc", transdiag=0.0, linseg=0, mixed=False, convs=False, wgrad=True,
                 sizes=False):
        self.name, self.arch, self.nfeat, self.nlabel, self.seq = name, arch, nfeat, nlabel, seq
        self.crit, self.transdiag, self.linseg = crit, transdiag, linseg
        self.mixed, self.convs, self.wgrad, self.sizes = mixed, convs, wgrad, sizes
        assert len(seq) >= 6 and seq[0] == seq[3] == seq[5]
        for axis in range(3):   # every one of B, T, L both grows and shrinks
            d = [b[axis] - a[axis] for a, b in zip(seq, seq[1:])]
            assert min(d) < 0 < max(d), (name, axis)


# R1.  T' = ceil(ceil(T / 2) / 2) = 16, 11, 50, 16, 5, 16: T even and odd (41, 17), B T' = 32, 33, 50, 25 (three of them no multiple
# of 4: the vector tails of the element-wise kernels), H = 16 (the block-Toeplitz TDS convolutions)
R1_SEQ = [(2, 64, 5), (3, 41, 3), (1, 200, 7), (2, 64, 5), (5, 17, 2), (2, 64, 5)]
R1_ARCH = recipes.tds_ctc_small_arch(c=(4, 6), h=16, kw=5, drop=0.3)
# R2.  One stride-2 stage, groups of inner = T' H C = 64 T' floats: 2304 (the one-wave kernel's last size), 2368 (one block per
# group), 8256 (> 8192: partial sums, scratch grows), 2304, 8192 (the one-block kernel's last size), 2304
R2_SEQ = [(2, 72, 5), (3, 73, 3), (1, 257, 7), (2, 72, 5), (4, 256, 2), (2, 72, 5)]
R2_INNER = [2304, 2368, 8256, 2304, 8192, 2304]
R2_ARCH = recipes.tds_ctc_small_arch(c=(4,), h=16, kw=5, drop=0.0)
# R3.  T' = T / 4; M = B T' = 32 (below one 64-row image tile), 64 (a whole tile: no row padding to zero), 111 (ragged), 32, 150, 32:
# the images' padded sizes, their once-per-arena zero padding and ones rows move with M
R3_SEQ = [(2, 64, 4), (4, 64, 2), (3, 148, 6), (2, 64, 4), (1, 600, 5), (2, 64, 4)]
# R4.  Explicit padding 2 on the first layer (its padded copy and row remap), SAME on the second; widths 64 / 48 (cin 40 and 32: the
# level-2 kernels take both); the ASG workspace (B T N and B T L terms) grows and shrinks; linseg(2): the hand-over to ASG proper,
# with its optimizer-state reset, falls between the second and the third shape of the training run
R4_SEQ = [(2, 64, 5), (3, 41, 9), (1, 200, 3), (2, 64, 5), (5, 17, 2), (2, 64, 5)]
R4_ARCH = recipes.conv_glu_small_arch(widths=(64, 48), kws=(5, 4), pad0=2)
# R5.  T' = ceil(T / 2) = 8 (below the relative-position window csz = 9), 19 (twice it and more), 10, 8, 9 (the window itself), 8
R5_SEQ = [(2, 16, 2), (4, 37, 3), (1, 20, 4), (2, 16, 2), (3, 18, 1), (2, 16, 2)]

CASES = [
    Case("R1-wgrad-on", R1_ARCH, 16, 12, R1_SEQ),
    Case("R1-wgrad-off", R1_ARCH, 16, 12, R1_SEQ, wgrad=False),
    Case("R2-ln-families", R2_ARCH, 16, 12, R2_SEQ),
    Case("R3-stream-bf16", STREAM_ARCH, 16, 12, R3_SEQ, mixed=True),
    Case("R4-asg-fp32", R4_ARCH, 40, 9, R4_SEQ, crit="asg", transdiag=4.0, linseg=2),
    Case("R4-asg-level1", R4_ARCH, 40, 9, R4_SEQ, crit="asg", transdiag=4.0, linseg=2, mixed=True),
    Case("R4-asg-level2", R4_ARCH, 40, 9, R4_SEQ, crit="asg", transdiag=4.0, linseg=2, mixed=True, convs=True),
    Case("R5-tr-fp32", TR_ARCH, 16, 12, R5_SEQ, sizes=True),
    Case("R5-tr-bf16", TR_ARCH, 16, 12, R5_SEQ, sizes=True, mixed=True),
]
IDS = [c.name for c in CASES]

OPTIMS = {"sgd": dict(lr=0.05, lrcrit=0.01, momentum=0.9, max_grad_norm=1.0),
          "adadelta": dict(lr=0.4, lrcrit=0.4, max_grad_norm=1.0),
          "adam": dict(lr=1e-3, lrcrit=1e-3, max_grad_norm=1.0)}


def new_trainer(case, optim="sgd"):
    """built and configured, neither planned nor on the device"""
    from wav2letter_amd.trainer import Trainer
    tr = Trainer(case.arch, case.nfeat, case.nlabel, case.crit, 4, case.transdiag)
    if case.linseg:
        tr.set_linseg(case.linseg)
    if optim == "adam":
        tr.set_optimizer("adam", "adam", weight_decay=0.01)
    elif optim != "sgd":
        tr.set_optimizer(optim, optim)
    tr.set_mixed_precision(case.mixed, convs=case.convs)
    tr.set_weight_grad_stream(case.wgrad)
    return tr


def make(case, shape, optim="sgd"):
    tr = new_trainer(case, optim)
    tr.init_params(seed=7)
    tr.plan(*shape)
    tr.to_device()
    return tr


def batch(case, k, shape):
    """the k-th batch of a case: features, -1 padded targets of ragged lengths, ragged input sizes (the longest fills the batch)"""
    B, T, L = shape
    rng = np.random.default_rng([len(case.name), case.nfeat, k])
    x = torch.tensor(rng.normal(size=(B, case.nfeat, T)).astype(np.float32)).cuda()
    tgt = np.full((B, L), -1, np.int32)
    for b in range(B):
        n = max(1, L - b % 3)
        tgt[b, :n] = rng.integers(0, case.nlabel - 1, size=n)
    sizes = None
    if case.sizes:
        sizes = torch.tensor([T * (1.0 - 0.23 * ((2 * b) % 4)) for b in range(B)], dtype=torch.float32).cuda()
    return x, torch.tensor(tgt).cuda(), sizes


def passes(tr, x, tgt, sizes, update=None):
    """what one batch leaves behind, cloned: eval-mode emissions, losses, the whole gradient arena [, the state after an update]"""
    if sizes is not None:
        tr.set_input_sizes(sizes)
    out = {"emissions": tr.forward(x, train=False).clone()}
    out["loss"] = tr.forward_backward(x, tgt).clone()
    out["grads"] = tr.grads_full.clone()
    if update is not None:
        tr.update(**update)
        out["params"], out["momentum"] = tr.params.clone(), tr.mom.clone()
        if getattr(tr, "state2", None) is not None:
            out["state2"] = tr.state2.clone()
        out["adam_steps"] = torch.tensor(tr.adam_steps())
    return out


def differences(got, want):
    """[(name, worst absolute difference)] of the entries that are not the same bits"""
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    bad = []
    for name in want:
        a, b = got[name], want[name]
        same = a.shape == b.shape and (torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b))
        if not same:
            bad.append((name, float("nan") if a.shape != b.shape else (a.double() - b.double()).abs().max().item()))
    return bad


# ---- (a) fixed parameters: the re-planned trainer against a fresh one at every shape ---------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_replanned_trainer_equals_fresh_one_at_every_shape(case):
    a = make(case, case.seq[0])
    for k, shape in enumerate(case.seq):
        if k:
            a.plan(*shape)
        x, tgt, sizes = batch(case, k, shape)
        want = None
        for _ in range(2):          # the control: two fresh trainers agree
            f = make(case, shape)
            f.params.copy_(a.params)
            f.set_step(k)           # (the dropout masks' seed comes from the step count)
            got = passes(f, x, tgt, sizes)
            assert torch.isfinite(got["loss"]).all() and torch.isfinite(got["grads"]).all(), (case.name, k, shape)
            if want is None:
                want = got
            else:
                assert differences(got, want) == [], ("control: two fresh trainers differ", case.name, k, shape)
        a.set_step(k)
        assert differences(passes(a, x, tgt, sizes), want) == [], (case.name, k, shape)
        assert want["grads"][:a.n_net].abs().max().item() > 0


def test_r2_sequence_crosses_the_layernorm_scratch_sizes():
    """R2's premise, through the entry point itself: per group the scratch is 2 doubles up to 8192 floats and more above, and the
    sequence's group sizes are the last of the first family, the first of the second, the first of the third, and the last of the second"""
    from wav2letter_amd import _lib
    from wav2letter_amd.trainer import _lib_tr
    lib, ltr = _lib.lib(), _lib_tr()
    per_group = []
    for (B, T, L), inner in zip(R2_SEQ, R2_INNER):
        h = ltr.w2l_trainer_create(R2_ARCH.encode(), 16, 12, b"ctc", 4, 0.0)
        to = C.c_int(0)
        assert ltr.w2l_trainer_plan(h, B, T, L, None, None, C.byref(to)) == 0
        ltr.w2l_trainer_destroy(h)
        assert to.value * 16 * 4 == inner, (T, to.value, inner)
        doubles = int(lib.w2l_layernorm_scratch_doubles(B, inner))
        assert doubles % B == 0
        per_group.append(doubles // B)
    assert per_group[0] == per_group[1] == per_group[3] == per_group[4] == per_group[5] == 2 and per_group[2] > 2, per_group
    assert int(lib.w2l_layernorm_scratch_doubles(1, 8192)) == 2 and int(lib.w2l_layernorm_scratch_doubles(1, 8196)) > 2


# ---- (b) a training run that re-plans per step against one continued from checkpoints in new trainers ----------------------

def _state(tr, losses):
    out = {"params": tr.params.clone(), "momentum": tr.mom.clone(), "adam_steps": torch.tensor(tr.adam_steps()),
           "losses": torch.cat(losses)}
    if getattr(tr, "state2", None) is not None:
        out["state2"] = tr.state2.clone()
    return out


@pytest.mark.parametrize("optim", list(OPTIMS))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_replanning_run_equals_checkpointed_run(case, optim, tmp_path):
    from wav2letter_amd import checkpoint
    hyper = OPTIMS[optim]

    def step(tr, k, shape, losses):
        x, tgt, sizes = batch(case, k, shape)
        if sizes is not None:
            tr.set_input_sizes(sizes)
        losses.append(tr.forward_backward(x, tgt).clone())
        tr.update(**hyper)

    # run A: one trainer, planned again for every step
    a, la = make(case, case.seq[0], optim), []
    for k, shape in enumerate(case.seq):
        if k:
            a.plan(*shape)
        step(a, k, shape, la)
    got = _state(a, la)
    # run B: a new trainer per step, planned once, continued from the checkpoint of the step before
    b, lb = make(case, case.seq[0], optim), []
    path = str(tmp_path / "ck.w2l")
    for k, shape in enumerate(case.seq):
        if k:
            checkpoint.save(path, b, case.arch, case.crit, step=k)
            b = new_trainer(case, optim)
            assert checkpoint.load(path, b, case.arch) == k
            b.plan(*shape)
            b.to_device()
        step(b, k, shape, lb)
    want = _state(b, lb)
    assert torch.isfinite(want["losses"]).all() and torch.isfinite(want["params"]).all()
    assert a.skipped_updates() == 0
    if optim == "adam":
        steps = len(case.seq) - case.linseg       # (the linseg hand-over starts the counts again)
        assert tuple(want["adam_steps"].tolist()) == (steps, steps if case.crit == "asg" else 0)
    assert differences(got, want) == [], (case.name, optim)


# ---- what survives a plan, and what does not -------------------------------------------------------------------------------

def test_skipped_update_count_and_last_norm_survive_a_plan():
    """after test_non_finite_gradient_skips_the_update: the count of skipped updates is "so far", over the life of the trainer, and
    grad_norm() is the norm of the last update -- both across plan() (a fresh arena, filled here with a pattern: neither number is
    read from it)"""
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(9)
    nfeat, nlabel = 8, 12
    tr = Trainer(recipes.tds_ctc_small_arch(c=(4,), h=nfeat, kw=5), nfeat, nlabel, "ctc", 4)
    tr.init_params(3)
    hyper = dict(lr=0.1, momentum=0.5, max_grad_norm=1.0)

    def step(shape, poison):
        B, T, L = shape
        x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
        tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
        tr.forward_backward(x, tgt)
        if poison:
            tr.grads[tr.grads.numel() // 2] = float("nan")
        tr.update(total_batch=B, **hyper)

    def replan(shape):
        tr.plan(*shape)
        tr.arena.fill_(12345.0)

    tr.plan(2, 48, 4)
    tr.to_device()
    assert tr.skipped_updates() == 0
    step((2, 48, 4), False)
    norm = tr.grad_norm()
    assert math.isfinite(norm) and norm > 0 and tr.skipped_updates() == 0
    replan((3, 33, 2))
    assert tr.grad_norm() == norm and tr.skipped_updates() == 0     # the last update's norm, not the new arena's bytes
    step((3, 33, 2), True)
    assert tr.skipped_updates() == 1 and not math.isfinite(tr.grad_norm())
    replan((1, 80, 6))
    assert tr.skipped_updates() == 1 and not math.isfinite(tr.grad_norm())   # BEFORE any update on the new plan
    p0 = tr.params.clone()
    step((1, 80, 6), False)
    assert tr.skipped_updates() == 1 and math.isfinite(tr.grad_norm()) and not torch.equal(tr.params, p0)
    replan((2, 48, 4))
    step((2, 48, 4), True)
    assert tr.skipped_updates() == 2
    replan((3, 33, 2))
    assert tr.skipped_updates() == 2
    step((3, 33, 2), False)
    assert tr.skipped_updates() == 2 and math.isfinite(tr.grad_norm())


def test_input_sizes_do_not_survive_a_plan():
    """sizes are B floats of the planned B: after a plan to a larger B a forward without sizes runs unmasked -- the bits of a trainer
    that never had any.  The sizes given before the plan are the first two entries of a buffer with room for the largest B, so a
    library that kept the pointer would read memory this test owns (and mask with it)"""
    case = Case("sizes", TR_ARCH, 16, 12, R5_SEQ)
    (b_old, t_old, l_old), (b_new, t_new, l_new) = (2, 16, 2), (4, 37, 3)
    buf = torch.tensor([16.0, 7.0, 5.0, 3.0], dtype=torch.float32).cuda()
    a = make(case, (b_old, t_old, l_old))
    x0, _, _ = batch(case, 0, (b_old, t_old, l_old))
    a.set_input_sizes(buf[:b_old])
    masked = a.forward(x0, train=False).clone()
    a.set_input_sizes(None)
    assert not torch.equal(masked, a.forward(x0, train=False))          # the mask matters
    a.set_input_sizes(buf[:b_old])
    a.plan(b_new, t_new, l_new)
    x, tgt, _ = batch(case, 1, (b_new, t_new, l_new))
    f = make(case, (b_new, t_new, l_new))
    want = passes(f, x, tgt, None)
    assert differences(passes(a, x, tgt, None), want) == []
    f.set_input_sizes(torch.tensor([37.0, 7.0, 5.0, 3.0], dtype=torch.float32).cuda())
    assert not torch.equal(f.forward(x, train=False), want["emissions"])   # ... and would have mattered here
    # the same shape planned again (a change of the convolution level does that inside the trainer) keeps the sizes it was given
    sizes = torch.tensor([37.0, 20.0, 30.0, 11.0], dtype=torch.float32).cuda()
    a.set_input_sizes(sizes)
    masked = a.forward(x, train=False).clone()
    a.set_mixed_precision(False, convs=True)
    assert torch.equal(a.forward(x, train=False), masked)


# ---- Trainer.evaluate: more shapes than it keeps planned -------------------------------------------------------------------

EVAL_SHAPES = [(2, 64, 5), (3, 41, 3), (1, 120, 7), (5, 17, 2), (2, 65, 4), (4, 30, 1)]
EVAL_ORDER = [0, 1, 2, 3, 4, 5, 0, 2, 5, 1, 0, 3, 4, 0]      # six distinct shapes > _EVAL_PLANS; 0 and 1 come back after eviction


@pytest.mark.parametrize("toggle", [False, True], ids=["fp32", "mixed-toggled"])
def test_evaluate_across_more_shapes_than_plans_kept(toggle):
    from wav2letter_amd.trainer import Trainer
    case = Case("eval", recipes.tds_ctc_small_arch(c=(4, 6), h=16, kw=5, drop=0.3), 16, 12, R1_SEQ)
    assert len(set(EVAL_SHAPES)) > Trainer._EVAL_PLANS
    a = make(case, (2, 48, 4))
    fresh = {}

    def reference(i, mixed):
        if (i, mixed) not in fresh:
            f = new_trainer(case)
            f.init_params(seed=7)
            f.to_device()
            f.set_mixed_precision(mixed)
            x, tgt, _ = batch(case, i, EVAL_SHAPES[i])
            loss, path = f.evaluate(x, tgt)
            fresh[(i, mixed)] = (loss.clone(), path.clone())
        return fresh[(i, mixed)]

    seen_mixed = set()
    for n, i in enumerate(EVAL_ORDER):
        mixed = toggle and n % 2 == 1
        if toggle:
            a.set_mixed_precision(mixed)
        x, tgt, _ = batch(case, i, EVAL_SHAPES[i])
        loss, path = a.evaluate(x, tgt)
        want_loss, want_path = reference(i, mixed)
        assert torch.isfinite(loss).all()
        assert torch.equal(loss.view(torch.int32), want_loss.view(torch.int32)) and torch.equal(path, want_path), (n, i, mixed)
        assert len(a._eval_plans) <= Trainer._EVAL_PLANS
        seen_mixed.add((i, mixed))
    if toggle:   # shape 0 was evaluated in both modes, and the modes differ
        assert {(0, False), (0, True)} <= seen_mixed
        assert not torch.equal(fresh[(0, False)][0], fresh[(0, True)][0])


# ---- the fl:: surface ------------------------------------------------------------------------------------------------------

def test_fl_network_replans_in_train_and_eval_mode(tmp_path):
    """tests/cpp/replan_caller.cpp: one fl:: network in train mode over S1, S2, S1 with a backward pass each, and in eval mode over
    three shapes (its eval arena only grows), against a network built fresh for each shape: emissions and every gradient bit for bit"""
    exe = str(tmp_path / "replan_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "replan_caller.cpp"),
                    "-o", exe, "-L" + libdir, "-lw2l_hip", "-Wl,-rpath," + libdir, "-ldl"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
