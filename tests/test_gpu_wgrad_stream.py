"""The weight-gradient stream: the fp32 backward enqueues the weight, bias and
filter gradients on a side stream the network owns and joins it before forward_backward returns.  Every kernel and every operand
is the one of the single-stream step, so a trainer with the switch on must equal one with it off BIT FOR BIT -- loss, the whole
gradient arena and the parameters, step after step.  A buffer handed to the side stream too early, overwritten too early, or a
missing join shows as a difference (or as gradients of the step before).

The net: the first two stages of the TDS-CTC recipe (recipes.tds_ctc_arch: strided C2 1 -> 10 / TDS 10 / strided C2 10 -> 14 /
TDS 14, on 80 mel rows) and a final Linear; B = 4, T = 1024, so the first stage runs on 4 x 512 = 2048 frames and its
weight-gradient products (K = 2048) are cut by the stream-K schedule on both streams.
Not the 16 / 32-channel net of test_librivox_two_dimensional_subsampling_convolutions: its second stage (C2 with 3 x 16 = 48 unrolled
input channels, TDS with 32 channels and kw * c = 672 > 383) falls through to the skinny implicit-GEMM filter gradient, which splits
K with atomicAdd (w2l_conv_backward_filter, EPI_ATOMIC) -- there two SINGLE-stream trainers already differ in those two gradients
at step 1 (measured: 1.3e-5 of 21, 3.3e-6 of 5.4) and in everything from step 2 on, so bit-identity is no property of that net with
or without the side stream.  On the recipe's own widths every kernel reduces in a fixed order; the first test below checks that
premise instead of assuming it.
Three full steps: steps 2 and 3 follow a forward that overwrote what the side stream had read the step before."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NFEAT, NLABEL, B, T, L = 80, 30, 4, 1024, 12
STEPS = 3


def arch(p):
    return ("V -1 NFEAT 1 0\n"
            f"C2 1 10 21 1 2 1 -1 -1\nR\nDO 0.0\nLN 0 1 2\nTDS 10 21 80 {p} 2400\n"
            f"C2 10 14 21 1 2 1 -1 -1\nR\nDO 0.0\nLN 0 1 2\nTDS 14 21 80 {p} 3360\n"
            "V 0 1120 1 0\nRO 1 0 3 2\nL 1120 NLABEL\n")


def make(p, on):
    from wav2letter_amd.trainer import Trainer
    tr = Trainer(arch(p), NFEAT, NLABEL, "ctc", 4)
    tr.init_params(seed=5)
    tr.plan(B, T, L)
    tr.to_device()
    tr.set_weight_grad_stream(on)
    return tr


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(14)
    x = torch.tensor(rng.normal(size=(B, NFEAT, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, NLABEL - 1, size=(B, L)).astype(np.int32)).cuda()
    return x, tgt


def run(tr, batch, steps=STEPS, before_step=None):
    """`steps` full steps; after each one a snapshot (loss, whole gradient arena, parameters)"""
    x, tgt = batch
    out = []
    for k in range(steps):
        if before_step:
            before_step(k)
        loss = tr.forward_backward(x, tgt)
        snap = [loss.clone(), tr.grads_full.clone()]
        tr.update(lr=0.05, momentum=0.9, max_grad_norm=1.0)
        snap.append(tr.params.clone())
        out.append(snap)
    torch.cuda.synchronize()
    return out


def assert_same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("loss", "grads_full", "params"), g, w):
            assert torch.isfinite(b).all(), (k, name)
            assert torch.equal(a, b), (k, name, (a - b).abs().max().item())


@pytest.fixture(scope="module")
def single_stream(batch):
    """the switch off, dropout 0.2 (the masked-copy path): computed once, read by every test below"""
    return run(make(0.2, False), batch)


def test_single_stream_step_is_repeatable(batch, single_stream):
    """the premise of every comparison below: on this net two single-stream trainers agree bit for bit"""
    assert_same(run(make(0.2, False), batch), single_stream)


def test_bit_identical_over_steps_with_dropout(batch, single_stream):
    want = single_stream
    assert not torch.equal(want[0][1], want[1][1]) and want[0][1].abs().max().item() > 0   # the steps really differ
    assert_same(run(make(0.2, True), batch), want)


def test_bit_identical_over_steps_without_dropout(batch):
    """p = 0: no masked copy -- dW2 reads LayerNorm 2's own data gradient"""
    assert_same(run(make(0.0, True), batch), run(make(0.0, False), batch))


def test_bucket_events_cover_both_streams(batch, single_stream):
    """three gradient buckets: a consumer stream that waits for a bucket's event must see that bucket's FINAL gradients (the
    arena is zeroed before the step, so a bucket signalled before the side stream has written it reads zeros)"""
    tr = make(0.2, True)
    offs = sorted({off for _n, _num, off in tr.param_table()})
    offs = [0, offs[len(offs) // 2], offs[-2]]
    tr.set_grad_buckets(offs)
    bounds = offs + [tr.grads_full.numel()]
    consumer = torch.cuda.Stream()
    x, tgt = batch
    for k in range(3):   # the third step's buckets are read
        tr.grads_full.zero_()
        tr.forward_backward(x, tgt)
        copies = {}
        if k == 2:
            for b in reversed(range(3)):   # last layers first, as the reducers walk them
                tr.wait_bucket(b, consumer)
                with torch.cuda.stream(consumer):
                    copies[b] = tr.grads_full[bounds[b]:bounds[b + 1]].clone()
        tr.update(lr=0.05, momentum=0.9, max_grad_norm=1.0)
    torch.cuda.synchronize()
    want = single_stream[2][1]
    for b in range(3):
        assert torch.equal(copies[b], want[bounds[b]:bounds[b + 1]]), b


def launch_counts(Lib):
    out = []
    for kind in range(7):
        n, ms, wk = C.c_int(0), C.c_double(0), C.c_double(0)
        Lib.w2l_profile_report_kind(kind, C.byref(n), C.byref(ms), C.byref(wk))
        out.append(n.value)
    return out


def test_event_brackets_keep_one_stream(batch, single_stream):
    """while w2l_profile_enable(1) is in force every launch stays on the caller's stream: same results, and the per-kind launch
    counts of a bracketed step equal those with the switch off"""
    from wav2letter_amd import _lib
    Lib = _lib.lib()
    counts = {}
    for on in (False, True):
        tr = make(0.2, on)

        def bracket(k):
            if k == STEPS - 1:
                torch.cuda.synchronize()
                Lib.w2l_profile_enable(1)
        try:
            got = run(tr, batch, before_step=bracket)
            counts[on] = launch_counts(Lib)
        finally:
            Lib.w2l_profile_enable(0)
        assert_same(got, single_stream)
    assert counts[True] == counts[False] and sum(counts[False]) > 0, counts


def test_caller_on_a_non_default_stream(batch, single_stream):
    s = torch.cuda.Stream()
    tr = make(0.2, True)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = run(tr, batch)
    assert_same(got, single_stream)
