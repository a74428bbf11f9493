"""Latency of LocalNorm (wav2letter_amd.streaming.StreamingLocalNorm: one launch per step; features.local_normalize: two launches
per batch), alone and inside the chain features -> norm -> network, beside what it stands next to:

    python tools/local_norm_one.py [--steps 200] [--rounds 3] [--left 300] [--no-chain] [--no-batch]

80 filters, left context 300 (the streaming recipe's --localnrmlleftctx).  Three legs, one JSON line per shape:

  session  S x chunk in {1 x 80 ms, 16 x 160 ms, 64 x 320 ms}: every slot is fed chunk_ms / 10 frames per step, mid-utterance (the
           window is full after 300 frames of warm-up).  First the contract is CHECKED on the shape -- the session fed the chunks
           equals local_normalize(right = 0) of the whole run bit for bit --, then `rounds` rounds of `steps` steps are timed, each
           step between its own pair of events after a warm-up.
  chain    the same shapes: StreamingFeatures.step, StreamingLocalNorm.step (in place on the feature step's view) and
           the step of a bf16 StreamingSession over the streaming TDS-CTC recipe, alternating, each between its own events: the
           norm step's share of the streaming step.
  batch    B in {32, 64}, T = 1500: local_normalize at left = 300 and at left = 0 (the difference is the window pass: 301 against 1
           pair per frame), the achieved bandwidth against the 2 x 4 B F T bytes the call must move, and beside it the
           per-utterance sequence of the list-file tools (gather into a dense [F][T_b] buffer, w2l_residual_layernorm_forward with
           gamma = 1 and beta = 0, scatter into the zeroed batch: 3 B launches) on the same batch, alternating."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wav2letter_amd import _lib
from wav2letter_amd.features import Mfsc, local_normalize
from wav2letter_amd.streaming import StreamingFeatures, StreamingLocalNorm

F, FS, STRIDE_MS = 80, 16000, 10


def feats(S, T, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (5.0 + 3.0 * torch.randn(S, F, T, generator=g)).cuda()


def timed(fn, events):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    events.append((e0, e1))


def medians(rounds):
    torch.cuda.synchronize()
    per_round = [float(np.median([a.elapsed_time(b) for a, b in ev])) for ev in rounds]
    allms = [a.elapsed_time(b) for ev in rounds for a, b in ev]
    return float(np.median(allms)), per_round


def us(ms):
    return round(ms * 1e3, 2)


def check_contract(S, frames, left):
    x = feats(S, 5 * frames + 3, 3 * S + frames)
    want = local_normalize(x, None, left, 0)
    sess = StreamingLocalNorm(F, S, frames, left)
    got = torch.empty_like(x)
    for i, t0 in enumerate(range(0, x.shape[2], frames)):
        k = min(frames, x.shape[2] - t0)
        c = torch.full((S, F, frames), float("nan"), device="cuda")
        c[:, :, :k] = x[:, :, t0:t0 + k]
        sess.step(c, np.full(S, k, np.int32), np.full(S, int(i == 0), np.int32))
        got[:, :, t0:t0 + k] = c[:, :, :k]
    if not torch.equal(got.view(torch.int32), want.view(torch.int32)):
        raise SystemExit(f"S = {S}, {frames} frames per step: the session differs from the batch call")


def session_leg(S, chunk_ms, left, steps, rounds, warmup=None):
    frames = chunk_ms // STRIDE_MS
    check_contract(S, frames, left)
    sess = StreamingLocalNorm(F, S, frames, left)
    x = feats(S, frames, S + frames)
    y = torch.empty_like(x)
    n = np.full(S, frames, np.int32)
    sess.step(x, n, np.ones(S, np.int32), out=y)
    for _ in range(warmup or (left // frames + 20)):   # the window fills
        sess.step(x, n, out=y)
    r = []
    for _ in range(rounds):
        ev = []
        for _ in range(steps):
            timed(lambda: sess.step(x, n, out=y), ev)
        r.append(ev)
    m, per = medians(r)
    return {"leg": "session", "S": S, "chunk_ms": chunk_ms, "frames_per_slot": frames, "left": left, "steps": steps, "rounds": rounds,
            "norm_step_us": us(m), "norm_step_us_rounds": [us(v) for v in per], "state_KiB": round(sess.state_bytes / 1024, 1)}


def chain_leg(S, chunk_ms, left, steps, rounds, warmup=None):
    from wav2letter_amd import recipes
    from wav2letter_amd.streaming import StreamingSession
    from wav2letter_amd.trainer import Trainer
    fe = Mfsc(num_filters=F, fs=FS)
    frames = chunk_ms // STRIDE_MS
    chunk = frames * fe.S
    tr = Trainer(recipes.streaming_tds_arch(), F, 9998, "ctc")
    tr.init_params(1)
    tr.to_device()
    tr.set_mixed_precision(True)
    fs = StreamingFeatures(fe, S, chunk)
    assert fs.max_out == frames
    ln = StreamingLocalNorm(F, S, frames, left)
    net = StreamingSession(tr, S, frames, mixed_precision=True)
    g = torch.Generator(device="cpu").manual_seed(S + chunk)
    pcm = (torch.randn(S, chunk, generator=g) * 3000.0).cuda()
    n, ones = np.full(S, chunk, np.int32), np.ones(S, np.int32)
    f, nf = fs.step(pcm, n, start=ones)
    ln.step(f, nf, ones)
    net.step(f, nf, start=ones)
    for _ in range(warmup or (left // frames + 12)):
        f, nf = fs.step(pcm, n)
        ln.step(f, nf)
        net.step(f, nf)
    ra, rb, rc = [], [], []
    for _ in range(rounds):
        ea, eb, ec = [], [], []
        for _ in range(steps):
            timed(lambda: fs.step(pcm, n), ea)
            timed(lambda: ln.step(f, nf), eb)
            timed(lambda: net.step(f, nf), ec)
        ra.append(ea)
        rb.append(eb)
        rc.append(ec)
    (ma, _), (mb, _), (mc, _) = medians(ra), medians(rb), medians(rc)
    return {"leg": "chain", "S": S, "chunk_ms": chunk_ms, "left": left, "feature_step_us": us(ma), "norm_step_us": us(mb),
            "bf16_stream_step_us": us(mc), "norm_share_of_stream_step": round(mb / mc, 4)}


def per_utterance(x, frames_host, out, tmp, nrm, unit, stats, mr):
    """the list-file tools' sequence: per utterance gather -> LayerNorm with (1, 0) -> scatter into the zeroed batch"""
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    for b, tb in enumerate(frames_host):
        t = tmp[:F * tb].view(F, tb)
        t.copy_(x[b, :, :tb])
        rc = L.w2l_residual_layernorm_forward(1, F * tb, t.data_ptr(), None, t.data_ptr(), nrm.data_ptr(), unit.data_ptr(), 1e-10, 0.0, 0, 0,
                                              stats.data_ptr(), mr.data_ptr(), st)
        assert rc == 0, rc
        out[b, :, :tb].copy_(nrm[:F * tb].view(F, tb))


def batch_leg(B, T, left, steps, rounds, warmup=10):
    x = feats(B, T, B)
    frames_host = [T - (37 * b) % 400 for b in range(B)]          # ragged, as a batch of utterances is
    frames = torch.tensor(frames_host, dtype=torch.int32, device="cuda")
    out, out0, out2 = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    L = _lib.lib()
    tmp, nrm = torch.empty(F * T, device="cuda"), torch.empty(F * T, device="cuda")
    unit, mr = torch.tensor([1.0, 0.0], device="cuda"), torch.empty(2, device="cuda")
    stats = torch.empty(2 * L.w2l_layernorm_scratch_doubles(1, F * T) + 2, dtype=torch.float64, device="cuda")
    # the two normalisations agree where every window is the whole utterance
    local_normalize(x, frames, T, T, out=out)
    per_utterance(x, frames_host, out2, tmp, nrm, unit, stats, mr)
    agree = float((out - out2).abs().max())
    if not agree < 1e-4:
        raise SystemExit(f"B = {B}: whole-utterance windows differ from the per-utterance LayerNorm by {agree:.3g}")
    for _ in range(warmup):
        local_normalize(x, frames, left, 0, out=out)
        local_normalize(x, frames, 0, 0, out=out0)
        per_utterance(x, frames_host, out2, tmp, nrm, unit, stats, mr)
    ra, rb, rc = [], [], []
    for _ in range(rounds):
        ea, eb, ec = [], [], []
        for _ in range(steps):
            timed(lambda: local_normalize(x, frames, left, 0, out=out), ea)
            timed(lambda: local_normalize(x, frames, 0, 0, out=out0), eb)
            timed(lambda: per_utterance(x, frames_host, out2, tmp, nrm, unit, stats, mr), ec)
        ra.append(ea)
        rb.append(eb)
        rc.append(ec)
    (ma, pa), (mb, _), (mc, pc) = medians(ra), medians(rb), medians(rc)
    moved = 2 * 4 * F * sum(frames_host)
    return {"leg": "batch", "B": B, "T": T, "F": F, "left": left, "frames": sum(frames_host), "local_norm_us": us(ma),
            "local_norm_us_rounds": [us(v) for v in pa], "local_norm_left0_us": us(mb), "window_pass_us": us(ma - mb),
            "min_bytes": moved, "achieved_GBps": round(moved / (ma * 1e-3) / 1e9, 1),
            "per_utterance_us": us(mc), "per_utterance_us_rounds": [us(v) for v in pc], "per_utterance_over_local_norm": round(mc / ma, 2),
            "whole_window_vs_per_utterance_maxdiff": float(f"{agree:.3g}")}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--left", type=int, default=300)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--no-batch", action="store_true")
    a = ap.parse_args()
    for S, c in ((1, 80), (16, 160), (64, 320)):
        print(json.dumps(session_leg(S, c, a.left, a.steps, a.rounds)), flush=True)
    if not a.no_batch:
        for B in (32, 64):
            print(json.dumps(batch_leg(B, 1500, a.left, max(20, a.steps // 4), a.rounds)), flush=True)
    if not a.no_chain:
        for S, c in ((1, 80), (16, 160), (64, 320)):
            print(json.dumps(chain_leg(S, c, a.left, a.steps, a.rounds)), flush=True)
