"""float64 restatement of the seq2seq criterion's contract, as torch ops so that autograd gives the gradients; the GRU
is tests/rnn_ref.py's.  Every function takes the dtype of its operands, so the same text run in float32 on the CPU shows how much
room the 1e-4 bar leaves (the figures are in the docstrings of tests/test_gpu_s2s.py)."""
import numpy as np
import torch

import rnn_ref as RR

_M64 = (1 << 64) - 1


def teacher_forcing(y, nClass, pct, seed):
    """(y', replaced): splitmix64 from `seed`; every entry in row-major order takes a draw, is replaced when draw % 100 >= pct, and
    then takes a second draw % (nClass - 1) as its token"""
    state, y = [int(seed) & _M64], np.array(y, np.int32)
    replaced = np.zeros(y.shape, bool)

    def draw():
        state[0] = (state[0] + 0x9E3779B97F4A7C15) & _M64
        z = state[0]
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)
    for i in range(y.size if pct < 100 else 0):
        if draw() % 100 >= pct:
            y.flat[i], replaced.flat[i] = draw() % (nClass - 1), True
    return y, replaced


def attention(h, enc, kl, tl, keyvalue, std):
    """h [B][U][H], enc [B][T][C] -> (context [B][U][H], alpha [B][U][T])"""
    (B, U, H), T, dt = h.shape, enc.shape[1], h.dtype
    k, v = (enc[..., :H], enc[..., H:]) if keyvalue else (enc, enc)
    t, u = torch.arange(T, dtype=dt)[None, None, :], torch.arange(U, dtype=dt)[None, :, None]
    kl, tl = torch.as_tensor(kl, dtype=dt)[:, None, None], torch.as_tensor(tl, dtype=dt)[:, None, None]
    score = h @ k.transpose(1, 2) / H ** 0.5
    if std:
        score = score + torch.where(u < tl, -(t - u * kl / tl) ** 2 / (2 * std * std), torch.zeros((), dtype=dt))
    alpha = torch.softmax(score.masked_fill(t >= kl, -np.inf), dim=2)
    return alpha @ v, alpha


def cross_entropy(z, target, row_utt, B, eps):
    """z [M][N], target [M] (-1: the row counts nothing) -> loss [B]"""
    target, N = torch.as_tensor(target, dtype=torch.int64), z.shape[1]
    lp = torch.log_softmax(z, dim=1)
    row = (1 - eps) * -lp.gather(1, target.clamp(min=0)[:, None])[:, 0] - eps / N * lp.sum(1)
    return torch.zeros(B, dtype=z.dtype).index_add(0, torch.as_tensor(row_utt, dtype=torch.int64), torch.where(target >= 0, row, torch.zeros((), dtype=z.dtype)))


def embedding(tokens, E, start):
    """tokens (-1: the start embedding) -> [*tokens.shape][H]"""
    return torch.cat([E, start[None]])[torch.as_tensor(tokens, dtype=torch.int64)]


def criterion(p, enc, prev, y, tl, kl, keyvalue, std, eps):
    """p: embedding, rnn, linear_weight, linear_bias, start; prev [B][U]: the decoder's teacher tokens y' -> (loss [B], alpha)"""
    B, U = y.shape
    H = p["start"].shape[0]
    tokens = np.concatenate([np.full((B, 1), -1), prev[:, :U - 1]], axis=1)
    h = RR.forward(embedding(tokens, p["embedding"], p["start"]), p["rnn"], 3, H)
    ctx, alpha = attention(h, enc, kl, tl, keyvalue, std)
    z = (h + ctx).reshape(B * U, H) @ p["linear_weight"] + p["linear_bias"]
    valid = np.arange(U)[None, :] < np.asarray(tl)[:, None]
    return cross_entropy(z, np.where(valid, y, -1).reshape(-1), np.repeat(np.arange(B), U), B, eps), alpha


class Case:
    """operands (float32 numpy, in `a`) of one function above, its results and the gradients of sum(result_i * weight_i) in float64
    (or `dtype`): fn(*tensors in order of `names`) -> tuple of results"""

    def __init__(self, fn, names, arrays, weights, dtype=torch.float64):
        self.a = dict(zip(names, arrays))
        ts = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in arrays]
        outs = fn(*ts)
        sum((o * torch.tensor(np.asarray(w), dtype=dtype)).sum() for o, w in zip(outs, weights) if w is not None).backward()
        self.out = [o.detach().numpy() for o in outs]
        self.grad = {n: t.grad.numpy() for n, t in zip(names, ts)}
