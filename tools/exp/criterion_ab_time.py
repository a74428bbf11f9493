"""FCC / ASG forward + backward in milliseconds (median of five series of 200 steps) with the library of this tree, or with the one
W2L_HIP_SO names (an A/B build of the same ABI).  Run it alternately with both to compare two builds on one device:
   [W2L_HIP_SO=<other build>/libw2l_hip.so] python tools/exp/criterion_ab_time.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from wav2letter_amd import ASGLoss, FullConnectionCriterion


def timeit(f, n=200):
    for _ in range(20):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            f()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / n)
    return sorted(ts)[2]


rng = np.random.default_rng(0)
for name, cls, B, T, N, L in (("ASG", lambda n: ASGLoss(n, 4, 4.0), 64, 2000, 30, 300), ("FCC", lambda n: FullConnectionCriterion(n, 4), 64, 2000, 30, 300),
                              ("FCC", lambda n: FullConnectionCriterion(n, 4), 64, 2000, 64, 300), ("FCC", lambda n: FullConnectionCriterion(n, 4), 64, 2000, 40, 300)):
    crit = cls(N).cuda()
    x = torch.from_numpy(rng.normal(size=(B, T, N)).astype(np.float32)).cuda().requires_grad_(True)
    tgt = np.full((B, L), -1, np.int32)
    for b in range(B):
        l = int(rng.integers(100, L + 1))
        tgt[b, :l] = rng.integers(0, N - 2, size=l)
    tg = torch.from_numpy(tgt).cuda()

    def step():
        x.grad = None
        crit(x, tg).sum().backward()
    print(f"{'W2L_HIP_SO' if os.environ.get('W2L_HIP_SO') else 'tree'}: {name} B={B} T={T} N={N}: fwd+bwd {timeit(step):.4f} ms", flush=True)
