"""Latency of the CPC criterion (w2l_cpc_forward / w2l_cpc_backward through wav2letter_amd.criterion._CPC) beside the same
arithmetic written as plain torch ops on the same device, in the same process:

    python tools/cpc_one.py [--steps 50] [--rounds 3] [--warmup 10] [--variants w2l,torch_gather,torch_dense]

The "small" recipe's shape: B = 3, Ce = 512, Cc = 768, D = 256, K = 100, tau = 0.1, at T = 800 with M = 400 and at T = 1600 with
M = 800.  Per shape one JSON line with the medians of forward and of forward + backward (all six gradients) for
  w2l           the criterion of this library
  torch_gather  the baseline: the reference's formulation (CPCCriterion.cpp:192-220) op by op -- gather the masked rows, two
                Linear layers, divide by the norms, index the K negatives of every anchor ([M][K][D] per utterance), multiply and
                sum, log-sum-exp --, a Python loop over the utterances as the reference's is
  torch_dense   the same values from one [M][M] score matrix per utterance (torch.matmul) and a gather of K + 1 columns: what the
                library's own shape looks like in torch ops
Every call sits between its own pair of events after a warm-up; the three variants alternate inside one loop, `rounds` rounds of
`steps` steps; the medians over all steps and per round are printed.  Before the timing the three variants are compared (loss and
gradients, 1e-4 of the largest magnitude).  --variants w2l times the library alone (a kernel trace of its launches)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wav2letter_amd import cpc
from wav2letter_amd.criterion import _CPC

B, CE, CC, D, NNEG, TAU = 3, 512, 768, 256, 100, 0.1
NAMES = ("enc", "ctx", "We", "be", "Wc", "bc")


def operands(T, M, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = {"enc": torch.randn(B, T, CE, generator=g), "ctx": torch.randn(B, T, CC, generator=g),
         "We": torch.randn(D, CE, generator=g) / CE ** 0.5, "be": 0.1 * torch.randn(D, generator=g),
         "Wc": torch.randn(D, CC, generator=g) / CC ** 0.5, "bc": 0.1 * torch.randn(D, generator=g)}
    t = {k: v.cuda().requires_grad_() for k, v in t.items()}
    r = np.random.default_rng(seed)
    index = np.stack([np.sort(r.choice(T, M, replace=False)) for _ in range(B)]).astype(np.int32)
    neg = cpc.negatives(cpc.CpcRng(seed), B, M, NNEG)
    return t, torch.tensor(index, device="cuda"), torch.tensor(neg, device="cuda"), torch.rand(B, generator=g).add(0.5).cuda()


def rows(t, index, b):
    idx = index[b].long()
    a = torch.nn.functional.linear(t["ctx"][b, idx], t["Wc"], t["bc"])
    p = torch.nn.functional.linear(t["enc"][b, idx], t["We"], t["be"])
    return a / a.norm(dim=1, keepdim=True), p / p.norm(dim=1, keepdim=True)


def torch_gather(t, index, neg):
    out = []
    for b in range(B):
        a, p = rows(t, index, b)
        pos = (p * a).sum(1, keepdim=True) / TAU
        negs = (p[neg[b].long()] * a.unsqueeze(1)).sum(2) / TAU
        s = torch.cat([pos, negs], 1)
        out.append((torch.logsumexp(s, 1) - s[:, 0]).mean())
    return torch.stack(out)


def torch_dense(t, index, neg):
    out = []
    for b in range(B):
        a, p = rows(t, index, b)
        S = (a @ p.T) / TAU
        M = S.shape[0]
        cols = torch.cat([torch.arange(M, device=S.device).unsqueeze(1), neg[b].long()], 1)
        s = S.gather(1, cols)
        out.append((torch.logsumexp(s, 1) - s[:, 0]).mean())
    return torch.stack(out)


def w2l(t, index, neg):
    return _CPC.apply(t["enc"], t["ctx"], t["We"], t["be"], t["Wc"], t["bc"], index, neg, TAU)


ALL_VARIANTS = {"w2l": w2l, "torch_gather": torch_gather, "torch_dense": torch_dense}


def forward(fn, t, index, neg, g):
    with torch.no_grad():
        return fn(t, index, neg)


def both(fn, t, index, neg, g):
    return torch.autograd.grad(fn(t, index, neg), [t[k] for k in NAMES], g)


def timed(fn, events):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    events.append((e0, e1))


def medians(rounds):
    torch.cuda.synchronize()
    per_round = [float(np.median([a.elapsed_time(b) for a, b in ev])) for ev in rounds]
    return float(np.median([a.elapsed_time(b) for ev in rounds for a, b in ev])), per_round


def us(ms):
    return round(ms * 1e3, 1)


def shape_leg(T, M, steps, rounds, warmup, names):
    VARIANTS = {k: v for k, v in ALL_VARIANTS.items() if k in names}
    t, index, neg, g = operands(T, M, T + M)
    ref_loss = forward(torch_gather, t, index, neg, g)
    ref_grads = both(torch_gather, t, index, neg, g)
    worst = 0.0
    for name, fn in VARIANTS.items():
        loss, grads = forward(fn, t, index, neg, g), both(fn, t, index, neg, g)
        for got, want in [(loss, ref_loss)] + list(zip(grads, ref_grads)):
            worst = max(worst, float((got - want).abs().max() / want.abs().max()))
    if not worst < 1e-4:
        raise SystemExit(f"T = {T}: the variants differ by {worst:.3g} of the largest magnitude")
    out = {"B": B, "T": T, "M": M, "K": int(neg.shape[2]), "Ce": CE, "Cc": CC, "D": D, "tau": TAU, "steps": steps, "rounds": rounds,
           "variants_agree_within": float(f"{worst:.3g}")}
    for leg, call in (("forward", forward), ("forward_backward", both)):
        for _ in range(warmup):
            for fn in VARIANTS.values():
                call(fn, t, index, neg, g)
        rec = {name: [] for name in VARIANTS}
        for _ in range(rounds):
            ev = {name: [] for name in VARIANTS}
            for _ in range(steps):
                for name, fn in VARIANTS.items():
                    timed(lambda: call(fn, t, index, neg, g), ev[name])
            for name in VARIANTS:
                rec[name].append(ev[name])
        for name in VARIANTS:
            m, per = medians(rec[name])
            out[f"{leg}_{name}_us"] = us(m)
            out[f"{leg}_{name}_us_rounds"] = [us(v) for v in per]
        for name in [k for k in ("torch_gather", "torch_dense") if k in VARIANTS and "w2l" in VARIANTS]:
            out[f"{leg}_{name}_over_w2l"] = round(out[f"{leg}_{name}_us"] / out[f"{leg}_w2l_us"], 2)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--variants", default="w2l,torch_gather,torch_dense")
    a = ap.parse_args()
    names = a.variants.split(",")
    if not names or any(k not in ALL_VARIANTS for k in names):
        raise SystemExit(f"--variants: a comma-separated list of {', '.join(ALL_VARIANTS)}")
    for T, M in ((800, 400), (1600, 800)):
        print(json.dumps(shape_leg(T, M, a.steps, a.rounds, a.warmup, names)), flush=True)
