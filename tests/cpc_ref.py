"""The CPC criterion restated in torch-CPU float64 from its contract (include/w2l_hip.h), gradients from autograd, and the
textbook sampler: an independent restatement of include/fl_compat/cpc.h with Python sets, not the twin the package ships
(wav2letter_amd/cpc.py).  Shared by tests/test_cpc_host.py, tests/test_gpu_cpc.py and tests/test_gpu_cpc_containment.py."""
import math

import numpy as np
import torch

MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------- the arithmetic
def apply_mask(x, mask, emb):
    """y[b][t][:] = mask[b][t] ? emb : x[b][t][:]"""
    return torch.where(mask.bool().unsqueeze(-1), emb.expand_as(x), x)


def loss(enc, ctx, We, be, Wc, bc, mask_index, neg, tau):
    """loss [B] float64.  enc [B][T][Ce], ctx [B][T][Cc], We [D][Ce], Wc [D][Cc], mask_index [B][M], neg [B][M][K] (long)"""
    out = []
    for b in range(enc.shape[0]):
        idx = mask_index[b]
        a = ctx[b, idx] @ Wc.T + bc
        p = enc[b, idx] @ We.T + be
        a = a / a.norm(dim=1, keepdim=True)
        p = p / p.norm(dim=1, keepdim=True)
        pos = (p * a).sum(1, keepdim=True) / tau                     # [M][1]
        negs = (p[neg[b]] * a.unsqueeze(1)).sum(2) / tau             # [M][K]
        s = torch.cat([pos, negs], 1)
        out.append((torch.logsumexp(s, 1) - s[:, 0]).mean())
    return torch.stack(out)


class Case:
    """inputs of one shape, drawn once; the float64 loss and the six gradients for the seed g, computed once"""

    def __init__(self, B, T, Ce, Cc, D, M, K, tau, seed=0, neg=None):
        self.dims = (B, T, Ce, Cc, D, M, K)
        self.tau = tau
        r = np.random.default_rng(seed)
        self.enc = r.normal(size=(B, T, Ce)).astype(np.float32)
        self.ctx = r.normal(size=(B, T, Cc)).astype(np.float32)
        self.We = (r.normal(size=(D, Ce)) / math.sqrt(Ce)).astype(np.float32)
        self.be = (0.1 * r.normal(size=D)).astype(np.float32)
        self.Wc = (r.normal(size=(D, Cc)) / math.sqrt(Cc)).astype(np.float32)
        self.bc = (0.1 * r.normal(size=D)).astype(np.float32)
        self.g = r.uniform(0.5, 1.5, size=B).astype(np.float32)
        self.mask_index = np.stack([np.sort(r.choice(T, M, replace=False)) for _ in range(B)]).astype(np.int32)
        self.neg = r.integers(0, M, size=(B, M, K)).astype(np.int32) if neg is None else np.ascontiguousarray(neg, np.int32)
        assert self.neg.shape == (B, M, K)
        self.mask = np.zeros((B, T), np.uint8)
        for b in range(B):
            self.mask[b, self.mask_index[b]] = 1
        t = {k: torch.tensor(getattr(self, k), dtype=torch.float64, requires_grad=True) for k in ("enc", "ctx", "We", "be", "Wc", "bc")}
        ls = loss(t["enc"], t["ctx"], t["We"], t["be"], t["Wc"], t["bc"], torch.tensor(self.mask_index, dtype=torch.long),
                  torch.tensor(self.neg, dtype=torch.long), tau)
        (ls * torch.tensor(self.g, dtype=torch.float64)).sum().backward()
        self.loss = ls.detach().numpy()
        self.grads = {k: v.grad.numpy() for k, v in t.items()}


def loss_bruteforce(c):
    """the same loss as plain loops over (b, m, k) in numpy float64"""
    B, T, Ce, Cc, D, M, K = c.dims
    out = np.zeros(B)
    for b in range(B):
        a = np.zeros((M, D))
        p = np.zeros((M, D))
        for m in range(M):
            t = c.mask_index[b, m]
            a[m] = c.Wc.astype(np.float64) @ c.ctx[b, t].astype(np.float64) + c.bc
            p[m] = c.We.astype(np.float64) @ c.enc[b, t].astype(np.float64) + c.be
            a[m] /= math.sqrt(float((a[m] * a[m]).sum()))
            p[m] /= math.sqrt(float((p[m] * p[m]).sum()))
        for m in range(M):
            s = [float(p[m] @ a[m]) / c.tau]
            for k in range(K):
                s.append(float(p[c.neg[b, m, k]] @ a[m]) / c.tau)
            mx = max(s)
            out[b] += mx + math.log(sum(math.exp(v - mx) for v in s)) - s[0]
        out[b] /= M
    return out


# ------------------------------------------------------------------------------------------------------------------- the sampler
class _Rng:
    def __init__(self, seed):
        self.s = seed & MASK64

    def __call__(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & MASK64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        return z ^ (z >> 31)


def span(s, mask_length, n):
    """the frames start s marks: s, s+1, s-1, s+2, s-2, ... clipped to [0, n)"""
    want = [s]
    d = 1
    while len(want) < mask_length:
        want.append(s + d)
        if len(want) < mask_length:
            want.append(s - d)
        d += 1
    return {t for t in want if 0 <= t < n}


def allowed_negatives(m, M):
    """the positions a negative of masked position m may name"""
    return [j for j in range(M) if abs(j - m) > 1]


def sampler(B, T, mask_prob, mask_length, n_negative, frames=None, seed=0):
    """(mask_index: list of B ascending lists of M frames, neg [B][M][K] nested lists, starts: the drawn start frames per utterance)"""
    rng = _Rng(seed)
    count = int(math.floor(mask_prob * T))
    marked, starts = [], []
    for b in range(B):
        n = T if frames is None else frames[b]
        got, st = set(), []
        for _ in range(count):
            st.append(rng() % n)
            got |= span(st[-1], mask_length, n)
        marked.append(sorted(got))
        starts.append(st)
    M = min(len(v) for v in marked)
    if M < 4:
        raise ValueError(f"M = {M}")
    index = []
    for v in marked:
        v = list(v)
        for i in range(len(v) - 1, 0, -1):
            j = rng() % (i + 1)
            v[i], v[j] = v[j], v[i]
        index.append(sorted(v[:M]))
    K = min(n_negative, M)
    neg = []
    for b in range(B):
        rows = []
        for m in range(M):
            # the allowed positions in the reference's rotated order: from min(M, m + 2) upward, wrapping past M - 1 to 0
            ring = [j % M for j in range(min(M, m + 2), min(M, m + 2) + M) if abs(j % M - m) > 1]
            assert sorted(ring) == allowed_negatives(m, M)
            rows.append([ring[rng() % len(ring)] for _ in range(K)])
        neg.append(rows)
    return index, neg, starts
