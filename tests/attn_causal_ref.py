"""float64 restatement of the causal self-attention kernel's contract and of the Transformer decoder criterion, as torch
ops so that autograd gives the gradients: oracle/transformer_oracle.py's attention arithmetic plus the j <= i mask, the len rule and the
dropout multiplier; its block arithmetic around that attention; tests/s2s_ref.py's encoder-decoder attention and cross entropy."""
import numpy as np
import torch
import torch.nn.functional as F

import s2s_ref as S
from oracle import transformer_oracle as TO

_M64 = (1 << 64) - 1


def attention(q, k, v, E, n_heads, scale, length, mult=None, with_lse=False):
    """q, k, v [B][U][C]; E [2 n0 + 1][d] or None; length [B]; mult [B][heads][U][U] the dropout multiplier or None -> ctx [B][U][C]
    (and lse [B][heads][U], 0 in the padded rows)"""
    B, U, C = q.shape
    split = lambda z: z.reshape(B, U, n_heads, C // n_heads).permute(0, 2, 1, 3)
    qh, kh, vh = split(q), split(k), split(v)
    s = qh @ kh.transpose(-1, -2)
    if E is not None:
        n0 = E.shape[0] // 2
        s = s + TO.relative_position_rotate(qh @ E.t())[..., n0:n0 + U]          # rel[i][j] = q_i . E[j - i + n0], 0 outside the table
    i = torch.arange(U)
    s = (s * scale).masked_fill(i[None, :] > i[:, None], -np.inf)
    P, valid = torch.softmax(s, dim=-1), i[None, :] < torch.as_tensor(np.asarray(length))[:, None]
    ctx = ((P if mult is None else P * mult) @ vh).permute(0, 2, 1, 3).reshape(B, U, C) * valid[:, :, None]
    return (ctx, torch.logsumexp(s, dim=-1) * valid[:, None, :]) if with_lse else ctx


def layer_drop(n_layer, p, seed, draws_before=0):
    """[n_layer] bool: splitmix64 from `seed`, `draws_before` draws discarded, then one draw per block; dropped when its upper 53 bits
    as a fraction lie below p"""
    state, out = int(seed) & _M64, []
    for n in range(draws_before + n_layer):
        state = (state + 0x9E3779B97F4A7C15) & _M64
        z = ((state ^ (state >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        out.append(((z ^ (z >> 31)) >> 11) / 2.0 ** 53 < p)
    return np.array(out[draws_before:], bool)


def block(x, ps, n_heads, tl, f):
    """transformer_oracle.tr_block's arithmetic (post-LayerNorm, f the layer-drop factor) around the causal attention above"""
    C = x.shape[-1]
    pos, w1, b1, w2, b2, wq, bq, wk, bk, wv, bv, wf, bf, g1, g2 = ps
    lin = lambda z, w, b: z @ w + b
    ln = lambda z, gb: F.layer_norm(z, (C,), eps=1e-5) * gb[0] + gb[1]
    o = lin(attention(lin(x, wq, bq), lin(x, wk, bk), lin(x, wv, bv), pos.t(), n_heads, (C // n_heads) ** -0.5, tl), wf, bf)
    h = ln(f * o + x, g1)
    return ln(f * lin(torch.relu(lin(h, w1, b1)), w2, b2) + h, g2)


def criterion(p, blocks, enc, prev, y, tl, kl, keyvalue, std, eps, n_heads, dropped):
    """p: embedding, linear_weight, linear_bias, start; blocks: nLayer lists of 15 in tr_param_shapes order -> (loss [B], alpha)"""
    B, U = y.shape
    tokens = np.concatenate([np.full((B, 1), -1), prev[:, :U - 1]], axis=1)
    x = S.embedding(tokens, p["embedding"], p["start"])
    for ps, gone in zip(blocks, dropped):
        x = block(x, ps, n_heads, tl, 0.0 if gone else 1.0)
    ctx, alpha = S.attention(x, enc, kl, tl, keyvalue, std)
    z = ctx.reshape(B * U, -1) @ p["linear_weight"] + p["linear_bias"]
    valid = np.arange(U)[None, :] < np.asarray(tl)[:, None]
    return S.cross_entropy(z, np.where(valid, y, -1).reshape(-1), np.repeat(np.arange(B), U), B, eps), alpha
