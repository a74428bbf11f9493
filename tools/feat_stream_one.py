"""Per-step latency of the streaming log-mel front end (wav2letter_amd.streaming.StreamingFeatures: one launch per step) beside
features.Mfsc.__call__ (four launches, two of them stream-K GEMMs) on the same number of frame rows, in the same process:

    python tools/feat_stream_one.py [--slots 1,16,64] [--chunk-ms 80,160,320] [--steps 200] [--rounds 3] [--share]
                                    [--profile-steps N]

16 kHz audio, 80 filters, float32 samples.  Every slot is fed chunk_ms of audio per step, mid-utterance (the carry is full after
the first step, so every step yields chunk_ms / 10 frames per slot).  For each (S, chunk) the tool first CHECKS the contract on
that shape -- the session fed the chunks equals, bit for bit, the session fed the same audio in thirds, and Mfsc of the whole
signal within 1e-4 of the largest feature magnitude -- and then times: `rounds` rounds of `steps` steps, the session's step and
Mfsc's call ALTERNATING inside a round, each call between its own pair of events on the stream after a warm-up of both.  Prints
one JSON line per (S, chunk): the median (over all rounds) and the per-round medians of both, and their ratio.
--share adds, for (S = 1, 80 ms) and (S = 16, 160 ms), the step of a bf16 StreamingSession over the streaming TDS-CTC recipe on
the frames of such a step, timed the same way beside the feature step: the front end's share of the streaming step.
--profile-steps N runs N feature steps of the first (S, chunk) and nothing else, for a kernel trace taken around this script."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wav2letter_amd.features import Mfsc
from wav2letter_amd.streaming import StreamingFeatures

FS, STRIDE_MS = 16000, 10


def audio(S, n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(S, n, generator=g) * 3000.0).cuda()


def check_contract(fe, S, chunk):
    """chunk invariance (bit for bit) and agreement with Mfsc on this shape: 4 chunks per slot, against the same audio in thirds of
    a chunk"""
    x = audio(S, 4 * chunk, 7 * S + chunk)
    third = -(-chunk // 3)
    outs = []
    for c in (chunk, third):
        sess = StreamingFeatures(fe, S, chunk)
        got, pos, first = [], 0, True
        while pos < x.shape[1]:
            k = min(c, x.shape[1] - pos)
            pcm = torch.full((S, chunk), float("nan"), device="cuda")
            pcm[:, :k] = x[:, pos:pos + k]
            pos += k
            f, n = sess.step(pcm, np.full(S, k, np.int32), start=np.full(S, int(first), np.int32),
                             finish=np.full(S, int(pos == x.shape[1]), np.int32))
            first = False
            assert (n == n[0]).all()
            got.append(f[:, :, :n[0]].clone())
        outs.append(torch.cat(got, dim=2))
    if not torch.equal(outs[0], outs[1]):
        raise SystemExit(f"S = {S}, chunk = {chunk}: the features depend on the chunking")
    whole = fe(x)
    err = float((outs[0] - whole).abs().max() / whole.abs().max())
    if outs[0].shape != whole.shape or not err < 1e-4:
        raise SystemExit(f"S = {S}, chunk = {chunk}: features differ from Mfsc by {err:.3g} of the largest magnitude")
    return err


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


def feature_leg(fe, S, chunk_ms, steps, rounds, warmup=20):
    frames = chunk_ms // STRIDE_MS
    chunk = frames * fe.S
    err = check_contract(fe, S, chunk)
    sess = StreamingFeatures(fe, S, chunk)
    pcm = audio(S, chunk, S + chunk)
    n = np.full(S, chunk, np.int32)
    whole = audio(S, (frames - 1) * fe.S + fe.N, S + chunk + 1)   # `frames` frames per utterance: the same S x frames rows
    _, n_out = sess.step(pcm, n, start=np.ones(S, np.int32))
    for _ in range(warmup):
        _, n_out = sess.step(pcm, n)
        fe(whole)
    assert (n_out == frames).all() and fe.num_frames(whole.shape[1]) == frames
    ra, rb = [], []
    for _ in range(rounds):
        ea, eb = [], []
        for _ in range(steps):
            timed(lambda: sess.step(pcm, n), ea)
            timed(lambda: fe(whole), eb)
        ra.append(ea)
        rb.append(eb)
    ma, pa = medians(ra)
    mb, pb = medians(rb)
    return {"leg": "features", "S": S, "chunk_ms": chunk_ms, "frames_per_slot": frames, "rows": S * frames, "steps": steps, "rounds": rounds,
            "session_step_us": round(ma * 1e3, 2), "session_step_us_rounds": [round(v * 1e3, 2) for v in pa],
            "mfsc_call_us": round(mb * 1e3, 2), "mfsc_call_us_rounds": [round(v * 1e3, 2) for v in pb],
            "mfsc_over_session": round(mb / ma, 2), "err_to_mfsc": float(f"{err:.3g}"), "state_KiB": round(sess.state_bytes / 1024, 1)}


def share_leg(fe, S, chunk_ms, steps, rounds, warmup=12):
    from wav2letter_amd import recipes
    from wav2letter_amd.streaming import StreamingSession
    from wav2letter_amd.trainer import Trainer
    frames = chunk_ms // STRIDE_MS
    chunk = frames * fe.S
    tr = Trainer(recipes.streaming_tds_arch(), 80, 9998, "ctc")
    tr.init_params(1)
    tr.to_device()
    tr.set_mixed_precision(True)
    feats = StreamingFeatures(fe, S, chunk)
    assert feats.max_out == frames
    net = StreamingSession(tr, S, feats.max_out, mixed_precision=True)
    pcm = audio(S, chunk, S + chunk)
    n = np.full(S, chunk, np.int32)
    ones = np.ones(S, np.int32)
    f, nf = feats.step(pcm, n, start=ones)
    net.step(f, nf, start=ones)
    for _ in range(warmup):
        f, nf = feats.step(pcm, n)
        net.step(f, nf)
    ra, rb = [], []
    for _ in range(rounds):
        ea, eb = [], []
        for _ in range(steps):
            timed(lambda: feats.step(pcm, n), ea)
            timed(lambda: net.step(f, nf), eb)
        ra.append(ea)
        rb.append(eb)
    ma, _ = medians(ra)
    mb, _ = medians(rb)
    return {"leg": "share", "S": S, "chunk_ms": chunk_ms, "feature_step_us": round(ma * 1e3, 2), "bf16_stream_step_us": round(mb * 1e3, 2),
            "feature_share_of_stream_step": round(ma / mb, 4)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,16,64")
    ap.add_argument("--chunk-ms", default="80,160,320")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--share", action="store_true")
    ap.add_argument("--profile-steps", type=int, default=0)
    a = ap.parse_args()
    slots = [int(v) for v in a.slots.split(",")]
    chunks = [int(v) for v in a.chunk_ms.split(",")]
    fe = Mfsc(num_filters=80, fs=FS)
    if a.profile_steps:
        S, chunk = slots[0], chunks[0] // STRIDE_MS * fe.S
        sess = StreamingFeatures(fe, S, chunk)
        pcm, n = audio(S, chunk, 1), np.full(S, chunk, np.int32)
        sess.step(pcm, n, start=np.ones(S, np.int32))
        for _ in range(a.profile_steps):
            sess.step(pcm, n)
        torch.cuda.synchronize()
        print(json.dumps({"leg": "profile", "S": S, "chunk_ms": chunks[0], "steps": a.profile_steps}))
        sys.exit(0)
    for S in slots:
        for c in chunks:
            print(json.dumps(feature_leg(fe, S, c, a.steps, a.rounds)), flush=True)
    if a.share:
        for S, c in ((1, 80), (16, 160)):
            print(json.dumps(share_leg(fe, S, c, a.steps, a.rounds)), flush=True)
