"""The fused causal self-attention kernel (ops.attn_causal) against the unfused fp32 sequence on the same operands -- two
batched products, mask and softmax, dropout, one product, all torch on the device -- forward, and forward + backward:
    python tools/attn_causal_one.py [--log profiles/attn_causal_one.log]
The routes alternate timing by timing in one process (fused, unfused, fused, ...); every figure is the median of 7 timings, each of as
many calls between two device synchronisations as last 10 ms, after a warm-up of both, with the spread (max - min) / median beside
it.  Also the Transformer criterion's forward + backward at the recipe's size.  Its per-part share comes from a kernel trace in a run
of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ac -- python tools/attn_causal_one.py --criterion-steps 10
    python tools/attn_causal_one.py --kernel-stats DIR/.../ac_kernel_stats.csv        (no GPU: groups the kernels by part)"""
import argparse
import csv
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_amd import TransformerCriterion, ops  # noqa: E402

SHAPES = [(8, 120, 4, 64), (32, 120, 4, 64), (8, 400, 4, 128)]   # B, U, Hd, d: the LibriSpeech recipe; a larger batch; long targets


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def timed(fns, reps=7, least_us=10000.0):
    """{name: (median us, spread)} of the routes `fns`, alternating: one timing of each per repetition; a timing lasts >= least_us"""
    calls = {n: max(5, int(least_us / window(f, 5)) + 1) for n, f in fns.items()}
    ts = {n: [] for n in fns}
    for _ in range(reps):
        for n, f in fns.items():
            ts[n].append(window(f, calls[n]))
    return {n: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for n, t in ts.items()}


PARTS = [("causal self-attention (attn_causal_*)", "attn_causal"), ("Linear products (gemm*)", "gemm"), ("encoder-decoder attention (s2s_attn_*)", "s2s_attn"),
         ("cross entropy (xent_*)", "xent"), ("LayerNorm (ln_*, residual_ln_*)", "ln_"), ("embedding (emb_*)", "emb_")]


def kernel_shares(path):
    """rocprofv3's kernel statistics grouped by part of the criterion"""
    rows = [{k.lower(): v for k, v in r.items()} for r in csv.DictReader(open(path))]
    total = sum(float(r["totaldurationns"]) for r in rows)
    left, out = list(rows), [f"kernel time by part, from {os.path.basename(path)}: {total / 1e6:.2f} ms in {sum(int(r['calls']) for r in rows)} launches"]
    for what, key in PARTS:
        mine = [r for r in left if key in r["name"]]
        left = [r for r in left if key not in r["name"]]
        out.append(f"  {what}: {sum(float(r['totaldurationns']) for r in mine) / total:.1%} in {sum(int(r['calls']) for r in mine)} launches")
    out.append(f"  everything else (copies, torch glue, colsum, ...): {sum(float(r['totaldurationns']) for r in left) / total:.1%} in {sum(int(r['calls']) for r in left)} launches")
    return out


def unfused(q, k, v, E, Hd, n0, scale, p):
    B, U, C = q.shape
    split = lambda z: z.reshape(B, U, Hd, C // Hd).permute(0, 2, 1, 3)
    qh, kh, vh = split(q), split(k), split(v)
    i = torch.arange(U, device=q.device)
    rel = (qh @ E.t()).gather(3, (i[None, :] - i[:, None] + n0).clamp(0, 2 * n0).expand(B, Hd, U, U))
    s = ((qh @ kh.transpose(-1, -2) + rel) * scale).masked_fill(i[None, :] > i[:, None], float("-inf"))
    P = torch.nn.functional.dropout(torch.softmax(s, dim=-1), p)
    return (P @ vh).permute(0, 2, 1, 3).reshape(B, U, C)


def criterion_step():
    """forward + backward of the criterion at the recipe's size (dropout 0.1, layer drop 0.1, one seed: the same blocks every step)"""
    B, T, U, H, N = 8, 250, 120, 256, 10000
    torch.manual_seed(0)
    crit = TransformerCriterion(N, H, N - 1, 6, "keyvalue", None, False, 99, 0.05, 0.1, 0.1, 120, 4).cuda().train()
    enc = torch.randn(B, T, 2 * H, device="cuda", requires_grad=True)
    y = np.random.default_rng(0).integers(0, N - 1, size=(B, U))

    def step():
        loss, _ = crit(enc, y, seed=3)
        loss.sum().backward()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--criterion-steps", type=int, default=0, help="only this many criterion steps, for a kernel trace")
    ap.add_argument("--kernel-stats", default=None, help="group a rocprofv3 kernel statistics file by part (no GPU)")
    args = ap.parse_args()
    if args.kernel_stats:
        print("\n".join(kernel_shares(args.kernel_stats)))
        return
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    if args.criterion_steps:
        step = criterion_step()
        for _ in range(3 + args.criterion_steps):
            step()
        torch.cuda.synchronize()
        return
    lines = [f"device: {torch.cuda.get_device_name(0)}; microseconds per call, medians of 7 alternating timings of >= 10 ms (spread)"]
    for B, U, Hd, d in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, U, 3 * Hd * d, device="cuda", generator=g, requires_grad=True)
        E = (torch.randn(2 * U - 1, d, device="cuda", generator=g) * d ** -0.5).requires_grad_()
        dctx, ln, C = torch.randn(B, U, Hd * d, device="cuda", generator=g), np.full(B, U, np.int32), Hd * d
        parts = lambda: (qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:])
        routes = {"fused": lambda: ops.attn_causal(*parts(), E, ln, Hd, U - 1, d ** -0.5, 0.1, 1, 0),
                  "unfused": lambda: unfused(*parts(), E, Hd, U - 1, d ** -0.5, 0.1)}
        err = (ops.attn_causal(*parts(), E, ln, Hd, U - 1, d ** -0.5) - unfused(*parts(), E, Hd, U - 1, d ** -0.5, 0.0)).abs().max().item()

        def both(f):
            qkv.grad = E.grad = None
            (f() * dctx).sum().backward()
        for f in routes.values():   # warm-up of every route and direction
            for _ in range(3):
                both(f)
        res = {"forward": timed({n: (lambda f=f: f().detach()) for n, f in routes.items()}),
               "forward + backward": timed({n: (lambda f=f: both(f)) for n, f in routes.items()})}
        for what in ("forward", "forward + backward"):
            (tf, sf), (tu, su) = res[what]["fused"], res[what]["unfused"]
            lines.append(f"B={B} U={U} Hd={Hd} d={d} {what}: fused {tf:.1f} ({sf:.0%}), unfused {tu:.1f} ({su:.0%}), unfused / fused {tu / tf:.2f}"
                         f"{'  ** fused slower **' if tf > tu else ''}  [max |fused - unfused| at p = 0: {err:.1e}]")
    step = criterion_step()
    for _ in range(3):
        step()
    total = timed({"step": step})["step"]
    lines.append(f"criterion B=8 T=250 U=120 H=256 N=10000 nLayer=6 forward + backward: {total[0]:.0f} us ({total[1]:.0%})")
    print("\n".join(lines))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        open(args.log, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
