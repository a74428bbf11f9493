"""float64 restatement, on torch CPU with autograd, of what tests/test_gpu_depthwise*.py run: the depthwise time convolution as
conv1d(groups = C), Swish as x * sigmoid(beta * x), and the Conformer convolution module as a composition -- residual_ref.Net
(V, RO, C, L, DO, RES / SKIP) extended by the tokens the module adds: the ninth field of a `C` line (groups), `WN 3 C`, `LN 1 2`,
`GLU 2` and `SH [beta]`.  Activations are held as there: ArrayFire (d0, d1, d2, d3) as torch (d3, d2, d1, d0)."""
import torch
import torch.nn.functional as F

import residual_ref as R


def swish(x, beta):
    return x * torch.sigmoid(beta * x)


def depthwise(x, w, bias, padl, padr):
    """x [B][T][H][C], w [kw][C], bias [C] or None -> y [B][To][H][C]; zero padding, cross-correlation"""
    B, T, H, C = x.shape
    a = F.pad(x.permute(0, 2, 3, 1).reshape(B * H, C, T), (padl, padr))
    y = F.conv1d(a, w.t().reshape(C, 1, -1), bias, groups=C)
    return y.reshape(B, H, C, -1).permute(0, 3, 1, 2)


def param_shapes(arch, nfeat, nlabel):
    """ArrayFire dims of the parameters in table order"""
    out = []
    for f in R.parse(arch, nfeat, nlabel):
        wn = f[:3] == ["WN", "3", "C"]
        f = f[2:] if wn else f
        if f[0] == "C":
            cin, cout, kw, groups = int(f[1]), int(f[2]), int(f[3]), int(f[8]) if len(f) > 8 else 1
            out += [(kw, 1, cin // groups, cout)] + ([(1, 1, 1, cout)] if wn else []) + [(1, 1, cout, 1)]
        elif f[0] == "L":
            out += [(int(f[2]), int(f[1])), (int(f[2]),)]
        elif f[0] == "LN":
            out += [(2,)]
    return out


class Net(R.Net):
    def _layer(self, f, a, it):
        wn = f[:3] == ["WN", "3", "C"]
        f = f[2:] if wn else f
        if f[0] == "C":
            cin, cout, kw, stride, pad = (int(v) for v in f[1:6])
            w = next(it)                                       # (kw, 1, cin / groups, cout) ArrayFire == torch [cout][cin / groups][1][kw]
            if wn:                                             # WN 3: one norm per output channel
                w = w * (next(it).reshape(-1, 1, 1, 1) / w.flatten(1).norm(dim=1).reshape(-1, 1, 1, 1))
            p = R.same_pad(a.shape[3], kw, stride) if pad == -1 else pad
            return F.conv2d(F.pad(a, (p, p)), w, next(it).reshape(-1), stride=(1, stride), groups=int(f[8]) if len(f) > 8 else 1)
        if f[0] == "LN" and f[1:] == ["1", "2"]:               # over (H, C) of every frame
            gb = next(it)
            mu, var = a.mean((1, 2), keepdim=True), a.var((1, 2), unbiased=False, keepdim=True)
            return (a - mu) / torch.sqrt(var + 1e-5) * gb[0] + gb[1]
        if f[0] == "GLU":
            assert f[1] == "2", f
            half = a.shape[1] // 2
            return a[:, :half] * torch.sigmoid(a[:, half:])
        if f[0] == "SH":
            return swish(a, float(f[1]) if len(f) > 1 else 1.0)
        return super()._layer(f, a, it)
