"""The seq2seq criterion's kernels against what a user could write before them, alternating in one process:
  attention      ops.s2s_attention forward and forward + backward against torch.bmm + mask + softmax + bmm (autograd for the backward);
  cross entropy  ops.s2s_xent_forward / _backward against log_softmax + gather + sums (autograd), and against w2l_axpy over the same
                 bytes (one read and one write of z) as a bandwidth floor;
  embedding      ops.embedding_forward / _backward against index_select / index_add_;
  criterion      Seq2SeqCriterion forward + backward, and the share of it spent in the GRU (ops.rnn forward + backward alone).
Shapes: the seq2seq_tds recipe (B = 16, U = 120, T = 188, H = 512, N = 9998), the sota/2019 pair (B = 8, H = 256), and T = 440.
Each figure is the median of `windows` timings between two events; `*_again` is a second series of the composition, whose distance
from the first is the spread to hold every ratio against.
  python tools/s2s_one.py [windows]"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from wav2letter_amd import Seq2SeqCriterion, _lib, ops

L = _lib.lib()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3   # us


def medians(fns, windows):
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            t[k].append(timed(f))
    return {k + "_us": round(statistics.median(v), 1) for k, v in t.items()}


def one(B, U, T, H, N, windows):
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    rng = np.random.default_rng(1)
    kl, tl = rng.integers(T // 2, T + 1, B).astype(np.int32), rng.integers(U // 2, U + 1, B).astype(np.int32)
    kl[0], tl[0] = T, U
    h, enc, dctx = rnd(B, U, H).requires_grad_(), rnd(B, T, 2 * H).requires_grad_(), rnd(B, U, H)
    mask = (torch.arange(T, device="cuda")[None, None, :] >= torch.tensor(kl, device="cuda")[:, None, None])

    def attn(bwd):
        ctx, _ = ops.s2s_attention(h, enc, kl, tl, True, None)
        if bwd:
            torch.autograd.grad((ctx * dctx).sum(), (h, enc))

    def attn_comp(bwd):
        s = torch.bmm(h, enc[..., :H].transpose(1, 2)) / H ** 0.5
        ctx = torch.bmm(torch.softmax(s.masked_fill(mask, float("-inf")), 2), enc[..., H:])
        if bwd:
            torch.autograd.grad((ctx * dctx).sum(), (h, enc))

    M = B * U
    z, g = (rnd(M, N) * 3).requires_grad_(), rnd(B)
    y = rng.integers(0, N, (B, U)).astype(np.int32)
    target = np.where(np.arange(U)[None, :] < tl[:, None], y, -1).reshape(-1).astype(np.int32)
    tdev, keep = torch.tensor(target, device="cuda").long().clamp(min=0), torch.tensor(target >= 0, device="cuda")
    zd, dz = z.detach(), torch.empty(M, N, device="cuda")

    def xent(bwd):
        loss, lse = ops.s2s_xent_forward(zd, target, 0.05, None, B)
        if bwd:
            ops.s2s_xent_backward(zd, lse, target, 0.05, g, None, out=dz)

    def xent_comp(bwd):
        lp = torch.log_softmax(z, 1)
        loss = ((0.95 * -lp.gather(1, tdev[:, None])[:, 0] - 0.05 / N * lp.sum(1)) * keep).view(B, U).sum(1)
        if bwd:
            torch.autograd.grad((loss * g).sum(), z)

    s = torch.cuda.current_stream().cuda_stream
    tokens = np.concatenate([np.full((B, 1), -1), y[:, :U - 1]], 1).reshape(-1).astype(np.int32)
    E, st, dx = rnd(N, H), rnd(H), rnd(M, H)
    idx = torch.tensor(np.where(tokens < 0, N, tokens), device="cuda").long()
    Es = torch.cat([E, st[None]])

    def emb_comp_bwd():
        torch.zeros(N + 1, H, device="cuda").index_add_(0, idx, dx)

    crit = Seq2SeqCriterion(N, H, N - 1, "keyvalue", ("softPretrain", 4.0), True, 100, 0.05).cuda()
    yt = np.where(np.arange(U)[None, :] < tl[:, None], np.minimum(y, N - 2), -1)
    yt[np.arange(B), tl - 1] = N - 1
    encd, x = enc.detach().requires_grad_(), rnd(B, U, H)

    def criterion():
        loss, _ = crit(encd, yt, inputSizes=kl)
        torch.autograd.grad(loss.sum(), [encd] + list(crit.parameters()))

    def gru():
        d = ops.rnn_desc(x, "gru", H, train=True)
        yy, ws = ops.rnn_forward(d, x, crit.rnn.detach())
        ops.rnn_backward(d, x, crit.rnn.detach(), yy, dctx, ws)

    fns = {"attn_fwd": lambda: attn(False), "attn_comp_fwd": lambda: attn_comp(False), "attn_comp_fwd_again": lambda: attn_comp(False),
           "attn_fwd_bwd": lambda: attn(True), "attn_comp_fwd_bwd": lambda: attn_comp(True), "attn_comp_fwd_bwd_again": lambda: attn_comp(True),
           "xent_fwd": lambda: xent(False), "xent_fwd_bwd": lambda: xent(True), "xent_comp_fwd": lambda: xent_comp(False),
           "xent_comp_fwd_bwd": lambda: xent_comp(True), "xent_comp_fwd_bwd_again": lambda: xent_comp(True),
           "axpy_same_bytes": lambda: L.w2l_axpy(dz.data_ptr(), zd.data_ptr(), M * N, 1.0, s),
           "emb_fwd": lambda: ops.embedding_forward(tokens, E, st), "emb_comp_fwd": lambda: Es.index_select(0, idx),
           "emb_bwd": lambda: ops.embedding_backward(tokens, dx, N), "emb_comp_bwd": emb_comp_bwd, "emb_comp_bwd_again": emb_comp_bwd,
           "criterion_fwd_bwd": criterion, "gru_fwd_bwd": gru}
    m = medians(fns, windows)
    out = {"B": B, "U": U, "T": T, "H": H, "N": N, "windows": windows, **m}
    out["gru_share"] = round(m["gru_fwd_bwd_us"] / m["criterion_fwd_bwd_us"], 2)
    for k, c in (("attn_fwd", "attn_comp_fwd"), ("attn_fwd_bwd", "attn_comp_fwd_bwd"), ("xent_fwd_bwd", "xent_comp_fwd_bwd"), ("emb_bwd", "emb_comp_bwd")):
        out[f"comp_over_{k}"] = round(m[c + "_us"] / m[k + "_us"], 2)
    print("[s2s] " + json.dumps(out), flush=True)


if __name__ == "__main__":
    windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    one(16, 120, 188, 512, 9998, windows)
    one(8, 120, 188, 256, 9998, windows)
    one(16, 120, 440, 512, 9998, windows)
