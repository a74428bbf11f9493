"""Per-step latency and real-time factor of the chunked streaming forward on the streaming TDS-CTC recipe
(am_500ms_future_context.arch, 80 mel, 9998 classes, fp32), beside the per-frame cost of the whole-utterance forward:

    python tools/stream_one.py [--slots 1,16,64] [--chunks 8,16,32] [--steps 60] [--whole-T 1500] [--no-whole] [--greedy]
                               [--bf16] [--probe]

Every slot is fed `chunk` input frames per step (10 ms each), mid-utterance, after a warm-up that fills every carry.  Prints one
JSON line per (S, chunk): the median and the 10th / 90th percentile step latency over `steps` steps (each timed with its own
pair of events on the stream), the real-time factor S x chunk_ms / step_ms, and the input frames per second; then one line per S
with w2l_trainer_forward at B = S, T = whole-T (eval mode) -- the yardstick: streaming cannot beat it per frame.
--bf16 adds, behind every fp32 line, the same leg through a mixed-precision session (StreamingSession(mixed_precision=True) over the
trainer in mixed-precision mode) in the same process, with the time of its first step -- the parameter snapshot and the bf16 weight
images -- as first_step_ms; the whole-utterance yardstick then runs in both precisions too.
--profile-steps N runs N steps of one (S, chunk) and nothing else (with --bf16: of the bf16 session alone), for a kernel trace
taken around this script.  --probe loads libw2l_hip_probe.so, which honours W2L_SMALLM_OFF=1 (the bf16 session's products back on
w2l_gemm_bf16: the A/B of the few-rows kernel).
--greedy prints the running greedy CTC collapse of slot 0's emissions (random parameters: noise; a smoke of the plumbing)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wav2letter_amd import recipes
from wav2letter_amd.streaming import StreamingSession
from wav2letter_amd.trainer import Trainer

NFEAT, NLABEL, FRAME_MS = 80, 9998, 10.0


def make_trainer():
    tr = Trainer(recipes.streaming_tds_arch(), NFEAT, NLABEL, "ctc")
    tr.init_params(1)
    tr.to_device()
    return tr


def stream_leg(tr, S, chunk, steps, warmup=12, greedy=False, bf16=False):
    tr.set_mixed_precision(bf16)
    sess = StreamingSession(tr, S, chunk, mixed_precision=bf16)
    g = torch.Generator(device="cpu").manual_seed(S * 100 + chunk)
    x = torch.randn(S, NFEAT, chunk, generator=g).cuda()
    n = np.full(S, chunk, np.int32)
    f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    f0.record()
    sess.step(x, n, start=np.ones(S, np.int32))
    f1.record()
    for _ in range(warmup):
        sess.step(x, n)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    frames, hyp, last = 0, [], -1
    for e0, e1 in ev:
        e0.record()
        out, n_out = sess.step(x, n)
        e1.record()
        frames += int(n_out.sum())
        if greedy:
            for t in out[0, :n_out[0]].argmax(dim=1).tolist():
                if t != last and t != NLABEL - 1:
                    hyp.append(t)
                last = t
    torch.cuda.synchronize()
    ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    med = float(np.median(ms))
    r = {"leg": "stream", "precision": "bf16" if bf16 else "fp32", "first_step_ms": round(f0.elapsed_time(f1), 3), "S": S, "chunk_frames": chunk, "chunk_ms": chunk * FRAME_MS, "steps": steps, "step_ms_median": round(med, 4),
         "step_ms_p10": round(float(np.percentile(ms, 10)), 4), "step_ms_p90": round(float(np.percentile(ms, 90)), 4),
         "rtf": round(S * chunk * FRAME_MS / med, 1), "input_frames_per_s": round(S * chunk / med * 1e3),
         "us_per_input_frame": round(med * 1e3 / (S * chunk), 3), "emission_frames": frames, "max_out": sess.max_out,
         "state_MiB": round(sess.state_bytes / 2**20, 1)}
    if greedy:
        r["greedy_tokens_slot0"] = hyp[:32]
    return r


def whole_leg(tr, B, T, reps=5, bf16=False):
    tr.set_mixed_precision(bf16)
    tr.plan(B, T, 1)
    x = torch.randn(B, NFEAT, T, generator=torch.Generator(device="cpu").manual_seed(B)).cuda()
    for _ in range(2):
        tr.forward(x, train=False)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        tr.forward(x, train=False)
        e1.record()
    torch.cuda.synchronize()
    med = float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))
    return {"leg": "whole", "precision": "bf16" if bf16 else "fp32", "B": B, "T": T, "forward_ms_median": round(med, 3), "us_per_input_frame": round(med * 1e3 / (B * T), 3),
            "input_frames_per_s": round(B * T / med * 1e3)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1,16,64")
    ap.add_argument("--chunks", default="8,16,32")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--whole-T", type=int, default=1500)
    ap.add_argument("--no-whole", action="store_true")
    ap.add_argument("--greedy", action="store_true")
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--probe", action="store_true")
    a = ap.parse_args()
    if a.probe:
        from wav2letter_amd import _lib
        _lib.use_probe().__enter__()
    slots = [int(v) for v in a.slots.split(",")]
    chunks = [int(v) for v in a.chunks.split(",")]
    tr = make_trainer()
    if a.profile_steps:
        print(json.dumps(stream_leg(tr, slots[0], chunks[0], a.profile_steps, warmup=2, bf16=a.bf16)))
        sys.exit(0)
    precisions = (False, True) if a.bf16 else (False,)
    for S in slots:
        for c in chunks:
            for bf in precisions:
                print(json.dumps(stream_leg(tr, S, c, a.steps, greedy=a.greedy, bf16=bf)), flush=True)
    if not a.no_whole:
        for S in slots:
            for bf in precisions:
                print(json.dumps(whole_leg(tr, S, a.whole_T, bf16=bf)), flush=True)
