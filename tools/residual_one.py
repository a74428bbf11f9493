"""The join of a residual block, w2l_residual_join_forward / _backward, against w2l_axpy on the same element count in the same process:
both move two reads and one write per element.  n = 4 * 1024 * 750 and 32 * 2304 * 93, the first and the last block of the ResNet-CTC
recipe at its batch of 4 / at 32 utterances of 1500 frames.  Windows of `inner` launches between two events (none inside the window),
the kernels alternating; the median window per kernel is reported.  w2l_axpy is timed as two series on operand pairs of its own
("axpy" / "axpy_again"): the distance between their medians is the spread that a difference between the join and w2l_axpy has to
exceed to mean anything -- the join may exceed axpy's median by at most twice that spread (the tool says whether it does).
The join out of place touches three arrays where the in-place w2l_axpy touches two; "join_fwd_inplace" (y == a) and
"join_bwd_relu_inplace" (g == dy) are the join on w2l_axpy's footprint.
With `recipe` as the first argument: one training step of am_resnet_ctc.arch at B = 4, T = 1500 in fp32 and one with the second
mixed-precision level (convs=True), loss and utterances/s of each -- recorded, not held to a bar.
  python tools/residual_one.py [windows] [inner]      python tools/residual_one.py recipe [steps]"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from wav2letter_amd import CriterionScaleMode, _lib, recipes
from wav2letter_amd.trainer import Trainer

L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream


def recipe(steps):
    B, T, Lt, nfeat, nlabel = 4, 1500, 40, 80, 9998
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.from_numpy(rng.integers(0, nlabel - 1, size=(B, Lt)).astype(np.int32)).cuda()
    for tag, mixed, convs in (("fp32", False, False), ("bf16 convs", True, True)):
        tr = Trainer(recipes.resnet_ctc_arch(), nfeat, nlabel, "ctc", CriterionScaleMode.TARGET_SZ_SQRT)
        tr.init_params(1)
        tr.to_device()
        if mixed:
            tr.set_mixed_precision(True, convs=convs)
        tout = tr.plan(B, T, Lt)
        losses, times = [], []
        for k in range(steps + 1):                     # the first step warms up (code objects, stream scratch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.set_step(k)
            loss = tr.forward_backward(x, tgt)
            tr.update(0.4, momentum=0.6, max_grad_norm=1.0)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            losses.append([float(v) for v in loss.cpu()])
        assert np.isfinite(losses).all(), losses
        step_s = statistics.median(times[1:])
        print("[residual recipe] " + json.dumps({
            "arch": "am_resnet_ctc.arch", "precision": tag, "B": B, "T": T, "T_out": tout, "params": int(tr.n_net), "steps_timed": steps,
            "first_loss": [round(v, 4) for v in losses[0]], "last_loss": [round(v, 4) for v in losses[-1]],
            "step_ms": round(step_s * 1e3, 2), "utterances_per_s": round(B / step_s, 2),
            "arena_GiB": round(tr.arena.numel() * 4 / 2 ** 30, 2)}), flush=True)
        del tr
        torch.cuda.empty_cache()


def join(windows, inner):
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner * 1e3   # us per launch

    for tag, n in (("first block, B = 4", 4 * 1024 * 750), ("last block, B = 32", 32 * 2304 * 93)):
        gen = torch.Generator(device="cuda").manual_seed(1)
        buf = [torch.randn(n, device="cuda", generator=gen) * 1e-3 for _ in range(9)]
        p = [b.data_ptr() for b in buf]
        fns = {"axpy": lambda: L.w2l_axpy(p[0], p[1], n, 1.0, s),
               "join_fwd": lambda: L.w2l_residual_join_forward(p[2], p[3], p[4], n, 0.70711, 0, s),
               "join_fwd_relu": lambda: L.w2l_residual_join_forward(p[2], p[3], p[4], n, 0.70711, 1, s),
               "axpy_again": lambda: L.w2l_axpy(p[5], p[6], n, 1.0, s),
               "join_bwd": lambda: L.w2l_residual_join_backward(p[7], p[8], p[2], n, 0.70711, 0, s),
               "join_bwd_relu": lambda: L.w2l_residual_join_backward(p[7], p[8], p[2], n, 0.70711, 1, s),
               # the allowed aliases y == a and g == dy: two arrays, w2l_axpy's footprint (scale 1: the values stay in range)
               "join_fwd_inplace": lambda: L.w2l_residual_join_forward(p[3], p[3], p[4], n, 1.0, 0, s),
               "join_bwd_relu_inplace": lambda: L.w2l_residual_join_backward(p[8], p[8], p[2], n, 1.0, 1, s)}
        for f in fns.values():   # warm-up: code objects, clocks
            for _ in range(5):
                assert f() == 0
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(windows):
            for k, f in fns.items():
                t[k].append(window(f))
        med = {k: statistics.median(x) for k, x in t.items()}
        gb = 12.0 * n / 1e9
        spread = abs(med["axpy"] - med["axpy_again"])
        bar = med["axpy"] + 2 * spread
        print("[residual join] " + json.dumps({
            "n": n, "where": tag, "gbytes_per_launch": round(gb, 4), "windows": windows, "launches_per_window": inner,
            **{f"{k}_us": round(x, 2) for k, x in med.items()},
            **{f"{k}_min_max_us": [round(min(t[k]), 2), round(max(t[k]), 2)] for k in t},
            **{f"{k}_TBps": round(gb / x * 1e3, 2) for k, x in med.items()},
            "axpy_spread_us": round(spread, 2), "bar_us": round(bar, 2),
            "within_bar": {k: bool(med[k] <= bar) for k in med if k.startswith("join")}}), flush=True)
        del buf


if len(sys.argv) > 1 and sys.argv[1] == "recipe":
    recipe(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
else:
    join(int(sys.argv[1]) if len(sys.argv) > 1 else 15, int(sys.argv[2]) if len(sys.argv) > 2 else 20)
