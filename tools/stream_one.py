"""Per-step latency and real-time factor of the chunked streaming forward on the streaming TDS-CTC recipe
(am_500ms_future_context.arch, 80 mel, 9998 classes, fp32), beside the per-frame cost of the whole-utterance forward:

    python tools/stream_one.py [--slots 1,16,64] [--chunks 8,16,32] [--steps 60] [--whole-T 1500] [--no-whole] [--greedy]

Every slot is fed `chunk` input frames per step (10 ms each), mid-utterance, after a warm-up that fills every carry.  Prints one
JSON line per (S, chunk): the median and the 10th / 90th percentile step latency over `steps` steps (each timed with its own
pair of events on the stream), the real-time factor S x chunk_ms / step_ms, and the input frames per second; then one line per S
with w2l_trainer_forward at B = S, T = whole-T (eval mode) -- the yardstick: streaming cannot beat it per frame.
--profile-steps N runs N steps of one (S, chunk) and nothing else, for a kernel trace taken around this script.
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


def stream_leg(tr, S, chunk, steps, warmup=12, greedy=False):
    sess = StreamingSession(tr, S, chunk)
    g = torch.Generator(device="cpu").manual_seed(S * 100 + chunk)
    x = torch.randn(S, NFEAT, chunk, generator=g).cuda()
    n = np.full(S, chunk, np.int32)
    sess.step(x, n, start=np.ones(S, np.int32))
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
    r = {"leg": "stream", "S": S, "chunk_frames": chunk, "chunk_ms": chunk * FRAME_MS, "steps": steps, "step_ms_median": round(med, 4),
         "step_ms_p10": round(float(np.percentile(ms, 10)), 4), "step_ms_p90": round(float(np.percentile(ms, 90)), 4),
         "rtf": round(S * chunk * FRAME_MS / med, 1), "input_frames_per_s": round(S * chunk / med * 1e3),
         "us_per_input_frame": round(med * 1e3 / (S * chunk), 3), "emission_frames": frames, "max_out": sess.max_out,
         "state_MiB": round(sess.state_bytes / 2**20, 1)}
    if greedy:
        r["greedy_tokens_slot0"] = hyp[:32]
    return r


def whole_leg(tr, B, T, reps=5):
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
    return {"leg": "whole", "B": B, "T": T, "forward_ms_median": round(med, 3), "us_per_input_frame": round(med * 1e3 / (B * T), 3),
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
    a = ap.parse_args()
    slots = [int(v) for v in a.slots.split(",")]
    chunks = [int(v) for v in a.chunks.split(",")]
    tr = make_trainer()
    if a.profile_steps:
        print(json.dumps(stream_leg(tr, slots[0], chunks[0], a.profile_steps, warmup=2)))
        sys.exit(0)
    whole = {}
    for S in slots:
        for c in chunks:
            print(json.dumps(stream_leg(tr, S, c, a.steps, greedy=a.greedy)), flush=True)
    if not a.no_whole:
        for S in slots:
            whole[S] = whole_leg(tr, S, a.whole_T)
            print(json.dumps(whole[S]), flush=True)
