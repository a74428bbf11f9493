"""The recurrent layer (w2l_rnn_forward / _backward) against what a user could write before it, in the same process:
  layer        the whole layer through the C ABI: forward (inference descriptor) and forward + backward (training descriptor);
  step         the T step launches alone -- the layer minus its whole-sequence products, timed as the same calls at T and the
               products issued on their own (ops.gemm on the same operands) -- in us per step, beside `empty`, the cost of an empty
               launch (a one-element w2l_fill) in the same process;
  composition  per step w2l_linear_forward at M = B for h W_hh^T, then the gate arithmetic as torch element-wise ops, over the same
               pre-activations; forward + backward adds torch autograd over that graph.
Shapes: a bidirectional one-layer LSTM at B = 32, T in {188, 500}, I = H in {512, 1024}, and the seq2seq decoder's GRU at B = 16,
T = 120, I = H = 512.  The BLSTM shapes are ASSUMPTIONS: the reference tree holds no recurrent arch file.  Each figure is the median of
`windows` timings between two events; `spread` is the distance between the medians of two series of the composition, and the bar is
its median plus twice that.
  python tools/rnn_one.py [windows]"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wav2letter_amd import _lib, ops

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
    return {k: statistics.median(v) for k, v in t.items()}


def composition(mode, x, w, H, dirs, train):
    """per direction: one input-side product, then per step linear_forward at M = B and torch gate arithmetic"""
    B, T, I = x.shape
    G = 4 if mode == "lstm" else 3
    outs, at = [], 0
    for d in range(dirs):
        wih, whh = w[at:at + G * H * I].view(G * H, I), w[at + G * H * I:at + G * H * (I + H)].view(G * H, H)
        bih, bhh = w[at + G * H * (I + H):at + G * H * (I + H + 1)], w[at + G * H * (I + H + 1):at + G * H * (I + H + 2)]
        at += G * H * (I + H + 2)
        pre = (x.reshape(B * T, I) @ wih.T + bih).view(B, T, G * H)
        whhT = whh.T.contiguous()
        h, c, hs = x.new_zeros(B, H), x.new_zeros(B, H), [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            hh = (h @ whhT + bhh) if train else ops.linear_forward(h, whhT, bhh)   # autograd needs a torch op; same product
            if mode == "lstm":
                i, f, g, o = (pre[:, t] + hh).split(H, dim=1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
                h = torch.sigmoid(o) * torch.tanh(c)
            else:
                r, z = torch.sigmoid(pre[:, t, :H] + hh[:, :H]), torch.sigmoid(pre[:, t, H:2 * H] + hh[:, H:2 * H])
                n = torch.tanh(pre[:, t, 2 * H:] + r * hh[:, 2 * H:])
                h = (1 - z) * n + z * h
            hs[t] = h
        outs.append(torch.stack(hs, dim=1))
    return torch.cat(outs, dim=2)


def one(mode, B, T, H, dirs, windows):
    I, G = H, 4 if mode == "lstm" else 3
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, T, I, device="cuda", generator=gen)
    dy = torch.randn(B, T, H * dirs, device="cuda", generator=gen)
    w = (torch.rand(ops.rnn_param_count(mode, I, H, 1, dirs == 2), device="cuda", generator=gen) * 2 - 1) / H ** 0.5
    infer, train = (ops.rnn_desc(x, mode, H, 1, dirs == 2, train=t) for t in (False, True))
    one_el = torch.zeros(1, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    wih, dg = w[:G * H * I].view(G * H, I), torch.randn(B * T, G * H, device="cuda", generator=gen)
    x2 = x.view(B * T, I)

    def fwd_bwd():
        y, ws = ops.rnn_forward(train, x, w)
        ops.rnn_backward(train, x, w, y, dy, ws)

    def products_fwd():
        for _ in range(dirs):
            ops.gemm(x2, wih, True, True)

    def products_bwd():   # dW_ih, dW_hh (same shape at I == H), dX per direction; the two column sums
        for _ in range(dirs):
            ops.gemm(dg, x2, False, False)
            ops.gemm(dg, x2, False, False)
            ops.gemm(dg, wih, True, False)
            ops.colsum(dg)
            ops.colsum(dg)

    def empty():
        for _ in range(T):
            L.w2l_fill(one_el.data_ptr(), 1, 0.0, s)

    wr = w.clone().requires_grad_()

    def comp_fwd_bwd():
        wr.grad = None
        (composition(mode, x, wr, H, dirs, True) * dy).sum().backward()

    fns = {"layer_fwd": lambda: ops.rnn_forward(infer, x, w), "layer_fwd_bwd": fwd_bwd, "products_fwd": products_fwd,
           "products_bwd": products_bwd, "empty_T_launches": empty,
           "comp_fwd": lambda: composition(mode, x, w, H, dirs, False), "comp_fwd_again": lambda: composition(mode, x, w, H, dirs, False),
           "comp_fwd_bwd": comp_fwd_bwd, "comp_fwd_bwd_again": comp_fwd_bwd}
    m = medians(fns, windows)
    out = {"mode": mode, "B": B, "T": T, "I": I, "H": H, "dirs": dirs, "windows": windows, **{k + "_us": round(v, 1) for k, v in m.items()}}
    out["step_fwd_us"] = round((m["layer_fwd"] - m["products_fwd"]) / T, 2)
    out["step_bwd_us"] = round((m["layer_fwd_bwd"] - m["layer_fwd"] - m["products_bwd"]) / T, 2)
    out["empty_launch_us"] = round(m["empty_T_launches"] / T, 2)
    for k in ("fwd", "fwd_bwd"):
        spread = abs(m["comp_" + k] - m["comp_" + k + "_again"])
        out[f"bar_{k}_us"] = round(m["comp_" + k] + 2 * spread, 1)
        out[f"comp_over_layer_{k}"] = round(m["comp_" + k] / m["layer_" + k], 1)
        out[f"meets_bar_{k}"] = bool(m["layer_" + k] <= m["comp_" + k] + 2 * spread)
    print("[rnn] " + json.dumps(out), flush=True)


if __name__ == "__main__":
    windows = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    for T in (188, 500):
        for H in (512, 1024):
            one("lstm", 32, T, H, 2, windows)
    one("gru", 16, 120, 512, 1, windows)
