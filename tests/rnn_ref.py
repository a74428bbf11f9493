"""float64 restatement of the recurrent layer's contract, as torch ops so that autograd gives the backward.
Modes: 0 ReLU, 1 tanh, 2 LSTM (gates i, f, g, o), 3 GRU (gates r, z, n; b_hn inside the product with r).  Flat parameter: layer by
layer, forward direction then reverse, each W_ih [G H][I_l], W_hh [G H][H], b_ih, b_hh.  Initial h and c are zero, every frame is
scanned, the reverse direction starts at frame T - 1; `masks[l]` (scaled keep masks, [B][T][H dirs]) multiplies the input of layer l."""
import torch

import residual_ref as R

GATES = {0: 1, 1: 1, 2: 4, 3: 3}
TOKENS = {"RNN": 0, "LSTM": 2, "GRU": 3}


def param_count(mode, I, H, layers, dirs):
    return sum(dirs * GATES[mode] * H * ((I if l == 0 else H * dirs) + H + 2) for l in range(layers))


def unpack(params, mode, I, H, layers, dirs):
    """[(W_ih, W_hh, b_ih, b_hh)] per (layer, direction), views of the flat parameter"""
    out, at, GH = [], 0, GATES[mode] * H
    for l in range(layers):
        Il = I if l == 0 else H * dirs
        for _ in range(dirs):
            sizes = [(GH, Il), (GH, H), (GH,), (GH,)]
            cut = []
            for s in sizes:
                n = s[0] * (s[1] if len(s) > 1 else 1)
                cut.append(params[at:at + n].reshape(s))
                at += n
            out.append(tuple(cut))
    assert at == params.numel()
    return out


def cell(mode, H, pre, h, c, whh, bhh):
    hh = h @ whh.T + bhh
    if mode == 0:
        return torch.relu(pre + hh), c
    if mode == 1:
        return torch.tanh(pre + hh), c
    if mode == 2:
        i, f, g, o = (pre + hh).split(H, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        return torch.sigmoid(o) * torch.tanh(c), c
    r, z = torch.sigmoid(pre[:, :H] + hh[:, :H]), torch.sigmoid(pre[:, H:2 * H] + hh[:, H:2 * H])
    n = torch.tanh(pre[:, 2 * H:] + r * hh[:, 2 * H:])
    return (1 - z) * n + z * h, c


def forward(x, params, mode, H, layers=1, dirs=1, masks=None):
    """x [B][T][I] -> y [B][T][H dirs]"""
    B, T, I = x.shape
    a = x
    for l in range(layers):
        if l > 0 and masks is not None:
            a = a * masks[l]
        outs = []
        for d in range(dirs):
            wih, whh, bih, bhh = unpack(params, mode, I, H, layers, dirs)[l * dirs + d]
            pre = a @ wih.T + bih
            h, c, hs = x.new_zeros(B, H), x.new_zeros(B, H), [None] * T
            for t in (range(T - 1, -1, -1) if d else range(T)):
                h, c = cell(mode, H, pre[:, t], h, c, whh, bhh)
                hs[t] = h
            outs.append(torch.stack(hs, dim=1))
        a = torch.cat(outs, dim=2)
    return a


def param_shapes(arch, nfeat, nlabel):
    """ArrayFire dims of the parameters in table order (recurrent lines: one flat parameter)"""
    out = []
    for f in R.parse(arch, nfeat, nlabel):
        if f[0] in TOKENS:
            out += [(param_count(TOKENS[f[0]], int(f[1]), int(f[2]), int(f[3]), 2 if int(f[4]) else 1),)]
        elif f[0] == "L":
            out += [(int(f[2]), int(f[1])), (int(f[2]),)]
    return out


class Net(R.Net):
    def _layer(self, f, a, it):
        if f[0] in TOKENS:                                     # (I, B, T, 1) == torch [1][T][B][I]
            y = forward(a[0].transpose(0, 1), next(it), TOKENS[f[0]], int(f[2]), int(f[3]), 2 if int(f[4]) else 1)
            return y.transpose(0, 1)[None]
        return super()._layer(f, a, it)
