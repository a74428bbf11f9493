"""Split-bf16 GEMM (csrc/gemm_split.hpp) against the fp32 route, one process, medians:
    python tools/gemm_split_one.py [--reps 15] [--steps 6] > profiles/gemm_split_one.log
The three products of fl::Linear (forward with bias + ReLU, dx, dW with the bias gradient) at the shapes of the headline step
(BASELINE config 2: recipes.tds_ctc_arch at B = 32, T = 1500 -- the Linear pairs of its three TDS stages and the final Linear), the
split route and the fp32 route ALTERNATING on the same operands; then one config-2 training step through Trainer with the switch
off / on / off / on.  Per shape: median ms of both routes, the ratio fp32 / split, and the fp32 route's own spread (max - min of
its samples over its median): a ratio inside 1 +- spread says nothing.  Timing is device events around `inner` back-to-back calls."""
import argparse
import os
import re
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from wav2letter_amd import CriterionScaleMode, _lib, recipes  # noqa: E402
from wav2letter_amd.trainer import Trainer  # noqa: E402


def linear_shapes(B, T):
    """(M, in, out) of every distinct fl::Linear of the arch: frames halve at each strided C2, a TDS block is in -> l2 -> in"""
    shapes, frames = [], T
    for line in recipes.tds_ctc_arch().splitlines():
        if line.startswith("C2 "):
            frames = (frames + 1) // 2
        m = re.match(r"TDS (\d+) \d+ (\d+) \S+ (\d+)", line)
        if m:
            c, h, l2 = (int(v) for v in m.groups())
            shapes += [(B * frames, c * h, l2), (B * frames, l2, c * h)]
        m = re.match(r"L (\d+) NLABEL", line)
        if m:
            shapes.append((B * frames, int(m.group(1)), 9998))
    return list(dict.fromkeys(shapes))


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(fn, reps, inner, switch):
    """fn timed with the switch off / on alternately; returns the two sample lists"""
    out = ([], [])
    try:
        for on in (0, 1):            # warm both routes: code objects, the stream scratch
            switch(on)
            timed(fn, 2)
        for _ in range(reps):
            for on in (0, 1):
                switch(on)
                out[on].append(timed(fn, inner))
    finally:
        switch(0)
    return out


def report(tag, f32, split):
    mf, ms = statistics.median(f32), statistics.median(split)
    print(f"{tag:44s} fp32 {mf:8.3f} ms  split {ms:8.3f} ms  fp32/split {mf / ms:5.2f}  fp32 spread {(max(f32) - min(f32)) / mf:5.1%}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1500)
    a = ap.parse_args()
    L, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
    print(f"device {torch.cuda.get_device_name(0)}; {a.reps} alternating samples per route", flush=True)
    for M, nin, nout in linear_shapes(a.batch, a.frames):
        x, w, dy, b = (torch.randn(*sh, device="cuda") for sh in ((M, nin), (nin, nout), (M, nout), (nout,)))
        y, dx, dw, db = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
        calls = {
            "forward": lambda: L.w2l_linear_forward(M, nin, nout, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, s),
            "dx": lambda: L.w2l_linear_backward_data(M, nin, nout, dy.data_ptr(), w.data_ptr(), dx.data_ptr(), 0, None, 1.0, s),
            "dW+db": lambda: L.w2l_linear_backward_weight_bias(M, nin, nout, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), s),
        }
        for name, fn in calls.items():
            report(f"M={M} {nin}->{nout} {name}", *alternate(fn, a.reps, 10, L.w2l_set_matmul_split))
    # one config-2 training step, the trainer's switch off / on / off / on
    nfeat, nlabel, Lmax, fl = 80, 9998, 80, recipes.TDS_CTC_FLAGS
    tr = Trainer(recipes.tds_ctc_arch(), nfeat, nlabel, "ctc", CriterionScaleMode.TARGET_SZ_SQRT, device=torch.device("cuda"))
    tr.init_params(seed=1)
    tr.plan(a.batch, a.frames, Lmax)
    tr.to_device()
    xb, tgt = bench.make_batch(a.batch, a.frames, nfeat, nlabel, Lmax, 2026, torch.device("cuda"))

    def step():
        tr.forward_backward(xb, tgt)
        tr.update(lr=fl["lr"], momentum=fl["momentum"], max_grad_norm=fl["maxgradnorm"], total_batch=a.batch)

    f32, split = alternate(step, 2, a.steps, lambda on: tr.set_split_precision(bool(on)))
    report(f"config 2 step B={a.batch} T={a.frames} (off/on/off/on)", f32, split)
    print("step samples ms: fp32 " + ", ".join(f"{t:.2f}" for t in f32) + "; split " + ", ".join(f"{t:.2f}" for t in split))


if __name__ == "__main__":
    main()
