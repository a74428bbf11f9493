"""The fused causal self-attention kernel (w2l_attn_causal_*) and the Transformer decoder criterion built on it against
the float64 restatement tests/attn_causal_ref.py.  The bar is the project's fp32 bar: every tensor within 1e-4 of its largest reference
magnitude.  Every call runs twice and must give the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import attn_causal_ref as R
from wav2letter_amd import TransformerCriterion, _lib, ops

pytestmark = pytest.mark.gpu
TOL = 1e-4


def close(got, want, what, scale=None):
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max() / max(1e-30, np.abs(want).max() if scale is None else scale)
    print(f"{what}: {err:.2e}")
    assert err < TOL, (what, err)


def dev(a, grad=False):
    return torch.tensor(a, device="cuda", requires_grad=grad)


def reference(fn, arrays, weights):
    """results and gradients (zeros for an operand nothing reaches) of sum(result_i * weight_i) in float64"""
    ts = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in arrays]
    outs = fn(*ts)
    sum((o * torch.tensor(w, dtype=torch.float64)).sum() for o, w in zip(outs, weights)).backward()
    return [o.detach().numpy() for o in outs], [np.zeros(a.shape) if t.grad is None else t.grad.numpy() for a, t in zip(arrays, ts)]


def operands(B, Hd, d, U, n0, seed=0):
    """ragged lengths: one utterance of all U positions, one of a single position"""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    ln = np.array([U // 2 + 1, U, 1][-B:] if B > 1 else [U], np.int32)
    return f(B, U, 3 * Hd * d), (None if n0 is None else f(2 * n0 + 1, d) * d ** -0.5), f(B, U, Hd * d), ln


def run(qkv, E, dctx, ln, Hd, n0, p, packed):
    """-> ctx, dq | dk | dv [B][U][3 C], dE (or None): the operands as thirds of one buffer (packed) or as three arrays"""
    Cc, scale = qkv.shape[2] // 3, (qkv.shape[2] // 3 // Hd) ** -0.5
    Et = None if E is None else dev(E, True)
    if packed:
        leaf = dev(qkv, True)
        q, k, v = leaf[..., :Cc], leaf[..., Cc:2 * Cc], leaf[..., 2 * Cc:]
    else:
        q, k, v = (dev(np.ascontiguousarray(qkv[..., n * Cc:(n + 1) * Cc]), True) for n in range(3))
    ctx = ops.attn_causal(q, k, v, Et, ln, Hd, n0 or 0, scale, p, 11, 3)
    (ctx * dev(dctx)).sum().backward()
    return ctx.detach(), (leaf.grad if packed else torch.cat([q.grad, k.grad, v.grad], dim=2)), None if E is None else Et.grad


# (B, Hd, d, U, n0 (None: no table), p, packed): one tile and a single position; the tile edge; two tiles with a table shorter than U;
# three tiles; every width class; four tiles of the recipe's heads.  n0 below U - 1 leaves distances outside the table.
CASES = [(2, 2, 32, 1, 3, 0.0, False), (2, 2, 32, 31, None, 0.2, False), (3, 4, 64, 33, 20, 0.2, True), (2, 1, 128, 65, 64, 0.0, False),
         (1, 2, 256, 97, 119, 0.2, True), (2, 4, 64, 121, None, 0.0, True)]


@pytest.mark.parametrize("B,Hd,d,U,n0,p,packed", CASES)
def test_kernel(B, Hd, d, U, n0, p, packed):
    qkv, E, dctx, ln = operands(B, Hd, d, U, n0)
    Cc = Hd * d
    mult = ops.dropout_copy(torch.ones(B, Hd, U, U, device="cuda"), p, 11, 3).double().cpu() if p else None
    fn = lambda qkv, *E: (R.attention(qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:], E[0] if E else None, Hd, d ** -0.5, ln, mult),)
    (want,), grads = reference(fn, [qkv] + ([] if E is None else [E]), (dctx,))
    a, b = (run(qkv, E, dctx, ln, Hd, n0, p, packed) for _ in range(2))
    assert all(x is None and y is None or torch.equal(x, y) for x, y in zip(a, b))
    ctx, dqkv, dE = a
    close(ctx, want, "ctx")
    for n, what in enumerate(("dq", "dk", "dv")):
        close(dqkv[..., n * Cc:(n + 1) * Cc], grads[0][..., n * Cc:(n + 1) * Cc], what)
    if E is not None:
        close(dE, grads[1], "dE")
    for u in range(B):   # padded positions: +0.0f, bit for bit
        assert (ctx[u, ln[u]:].view(torch.int32) == 0).all() and (dqkv[u, ln[u]:].contiguous().view(torch.int32) == 0).all()


def test_causal_and_batch_independent():
    """row i does not read k, v behind i; utterance 0 of B = 3 is the B = 1 call: bit for bit, dropout on"""
    B, Hd, d, U, n0 = 3, 4, 64, 33, 20
    qkv, E, dctx, ln = operands(B, Hd, d, U, n0)
    ln[0] = U
    ctx, dqkv, dE = run(qkv, E, dctx, ln, Hd, n0, 0.2, True)
    i, other = 17, qkv.copy()
    other[:, i + 1:, Hd * d:] = np.random.default_rng(1).normal(size=other[:, i + 1:, Hd * d:].shape)
    assert torch.equal(run(other, E, dctx, ln, Hd, n0, 0.2, True)[0][:, :i + 1], ctx[:, :i + 1])
    one = run(qkv[:1], E, dctx[:1], ln[:1], Hd, n0, 0.2, True)
    assert torch.equal(one[0][0], ctx[0]) and torch.equal(one[1][0], dqkv[0])


def test_stays_inside():
    """the three entry points in guarded arenas (tests/arena.py) with workspaces of exactly the declared bytes: quiet,
    quiet again, NaN-filled; the operands are the thirds of one buffer whose rows lie 4 floats further apart than 3 C"""
    from tests.test_gpu_containment import _stream
    from tests.test_gpu_cpc_containment import run_three
    B, Hd, d, U, n0, p = 2, 2, 32, 37, 9, 0.2
    qkv, E, dctx, ln = operands(B, Hd, d, U, n0, seed=3)
    Cc, ld = Hd * d, 3 * Hd * d + 4
    mult = ops.dropout_copy(torch.ones(B, Hd, U, U, device="cuda"), p, 11, 3).double().cpu()
    fn = lambda qkv, E: R.attention(qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:], E, Hd, d ** -0.5, ln, mult, with_lse=True)
    (want, lse), (dqkv, dE) = reference(fn, [qkv, E], (dctx,))
    desc = _lib.AttnCausalDesc(B, Hd, U, d, ld, Cc, n0, d ** -0.5, p, 11, 3)

    def case(r):
        L, dp = r.L, ctypes.byref(desc)
        n0b, n1b = L.w2l_attn_causal_workspace_size(dp, 0), L.w2l_attn_causal_workspace_size(dp, 1)
        pq, pe, pc, pl = r.inp("qkv", qkv, ld=ld), r.inp("E", E), r.out("ctx", (B, U, Cc)), r.out("lse", (B, Hd, U))
        r.ok(L.w2l_attn_causal_forward(dp, pq, pq + 4 * Cc, pq + 8 * Cc, pe, ln.ctypes.data, pc, pl, r.work("ws0", n0b), n0b, _stream()), "forward")
        pg = r.out("dqkv", (B, U, 3 * Cc), ld=ld)
        r.ok(L.w2l_attn_causal_backward(dp, pq, pq + 4 * Cc, pq + 8 * Cc, pe, ln.ctypes.data, pl, r.inp("dctx", dctx), pg, pg + 4 * Cc,
                                        pg + 8 * Cc, r.out("dE", E.shape), r.work("ws1", n1b), n1b, _stream()), "backward")
        return lambda: {"ctx": ("rel", want), "lse": ("rel", lse), "dqkv": ("rel", dqkv), "dE": ("rel", dE)}
    run_three(case)


@pytest.mark.parametrize("attention,window", [("keyvalue", ("softPretrain", 4.0)), ("content", None)])
def test_criterion(attention, window):
    """loss, alpha and every gradient, each tensor to the bar on its own; teacher forcing 50 % and a layer drop that takes one of the
    two blocks, both from seed 5.  One tensor has no magnitude of its own: a dropped block is LN2(LN1(x)), which does not depend on
    LN1's (gamma, beta) but through eps, so that gradient is a difference of O(1) sums that cancels to 2e-7 in float64 (measured in
    fp32: -2.26e-07, -8.9e-08 for -2.38e-07, -2.2e-16), the size of one fp32 rounding of its terms.  It alone is held to 1e-4 of the
    largest magnitude of the same block's norm2 gradient, the O(1) sums it is a difference of."""
    N, H, Hd, nL, B, T, U, seed, csz = 11, 64, 2, 2, 3, 20, 7, 5, 9
    torch.manual_seed(1)
    crit = TransformerCriterion(N, H, N - 1, nL, attention, window, True, 50, 0.05, 0.0, 0.5, csz, Hd).cuda().train()
    with torch.no_grad():
        for blk in crit.blocks:
            blk[9].copy_(torch.tensor([1.3, -0.2])), blk[10].copy_(torch.tensor([0.8, 0.1]))
    rng = np.random.default_rng(2)
    enc = rng.normal(size=(B, T, 2 * H if attention == "keyvalue" else H)).astype(np.float32)
    y, tl, sizes = rng.integers(0, N - 1, size=(B, U)), np.array([7, 1, 4], np.int32), np.array([1.0, 0.3, 0.6])
    g, dalpha = rng.normal(size=B).astype(np.float32), rng.normal(size=(B, U, T)).astype(np.float32)
    names = ["embedding", "linear_weight", "linear_bias", "start"]
    arrays = [enc] + [getattr(crit, n).detach().cpu().numpy() for n in names] + [p.detach().cpu().numpy() for blk in crit.blocks for p in blk]
    prev, replaced = R.S.teacher_forcing(np.where(np.arange(U)[None] < tl[:, None], y, N - 1), N, 50, seed)
    dropped = R.layer_drop(nL, 0.5, seed, B * U + int(replaced.sum()))
    assert dropped.sum() == 1
    kl = np.ceil(sizes / sizes.max() * T).astype(np.int32)
    def ref_block(pos, w1, b1, w2, b2, wqkv, bqkv, wf, bf, g1, g2):   # the stored layouts -> tr_param_shapes order
        return [pos.t(), w1, b1, w2, b2] + [t for n in range(3) for t in (wqkv[:, n * H:(n + 1) * H], bqkv[n * H:(n + 1) * H])] + [wf, bf, g1, g2]
    fn = lambda enc, *p: R.criterion(dict(zip(names, p[:4])), [ref_block(*p[4 + 11 * n:15 + 11 * n]) for n in range(nL)], enc, prev, y, tl, kl,
                                     attention == "keyvalue", window and window[1], 0.05, Hd, dropped)
    (loss_w, alpha_w), grads = reference(fn, arrays, (g, dalpha))
    runs = []
    for _ in range(2):
        crit.zero_grad()
        et = dev(enc, True)
        loss, alpha = crit(et, y, sizes, tl, seed=seed)
        ((loss * dev(g)).sum() + (alpha * dev(dalpha)).sum()).backward()
        params = [getattr(crit, n) for n in names] + [p for blk in crit.blocks for p in blk]
        runs.append([loss.detach(), alpha.detach(), et.grad] + [torch.zeros_like(p) if p.grad is None else p.grad.clone() for p in params])
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and np.array_equal(crit.dropped, dropped) and np.array_equal(crit.replaced, replaced)
    close(runs[0][0], loss_w, "loss"), close(runs[0][1], alpha_w, "alpha")
    got = runs[0][2:]
    for n in range(len(grads)):
        gone = (n - 5) // 11 if n >= 5 and (n - 5) % 11 == 9 and dropped[(n - 5) // 11] else None   # norm1 of a dropped block: the docstring
        close(got[n], grads[n], f"gradient {n}", None if gone is None else np.abs(grads[n + 1]).max())
