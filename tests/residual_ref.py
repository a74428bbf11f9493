"""float64 restatement, on torch CPU, of the networks the residual-block tests run (tests/test_gpu_residual*.py).

An interpreter of the arch tokens those networks use -- V, RO, C (time convolution, SAME padding by the project's rule), L and
WN 0 L, R, DO (identity: p = 0 or eval), LN 0 1 2, M w 1 s 1, GLU is not needed -- and of RES / SKIP / SKIPL as DESIGN 3.29 states
them: y = scale * (f(x) + p(x)), f the block's layers in order, p the identity or the projection layers, the shortcut from the
block's input to its output.  Written from the arch grammar and the reference's layer semantics, not from the project's code:
activations are ArrayFire arrays (d0, d1, d2, d3) held as torch tensors of shape (d3, d2, d1, d0) -- column-major ArrayFire memory
is row-major torch memory with the dimensions reversed -- so V is a reshape and RO a permute.

Parameters come in the order and the reference layout of Trainer.param_table() / export_from(): convolution (kw, 1, cin, cout),
Linear (out, in), WeightNorm v then g, bias, LayerNorm (gamma, beta).  The CTC loss is torch's, summed per utterance and scaled by
1 / sqrt(target length) (--onorm=target --sqnorm).  join_forward / join_backward restate the two join kernels in numpy fp32, bit
for bit."""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32


def join_forward(a, b, scale, relu):
    """w2l_residual_join_forward: one fp32 add, one fp32 multiply, then the positive part"""
    y = F32(scale) * (a.astype(F32) + b.astype(F32))
    return np.where(y > 0, y, F32(0)).astype(F32) if relu else y.astype(F32)


def join_backward(dy, y, scale, relu):
    """w2l_residual_join_backward: g = scale * dy, 0 where y <= 0 with relu"""
    g = (F32(scale) * dy.astype(F32)).astype(F32)
    return np.where(y <= 0, F32(0), g).astype(F32) if relu else g


def same_pad(T, kw, stride):
    """SAME padding of a strided convolution over T frames: the total is kw - stride when stride divides T, else kw - T % stride
    (never negative), and each side gets the rounded-up half"""
    total = max(kw - stride if T % stride == 0 else kw - T % stride, 0)
    return (total + 1) // 2


def parse(arch_text, nfeat, nlabel):
    out = []
    for raw in arch_text.splitlines():
        line = raw.strip()
        if line and not line.startswith("#"):
            out.append(line.replace("NFEAT", str(nfeat)).replace("NLABEL", str(nlabel)).split())
    return out


class Net:
    """forward(x [B][NFEAT][T], params) -> emissions [B][T'][N]; `pre_relu` collects every ReLU input of the last forward"""

    def __init__(self, arch_text, nfeat, nlabel):
        self.lines = parse(arch_text, nfeat, nlabel)
        self.pre_relu = []

    def _layer(self, f, a, it):
        tok = f[0]
        if tok == "V":
            want = [int(v) for v in f[1:5]]
            have = list(a.shape[::-1])
            want = [have[i] if w == 0 else w for i, w in enumerate(want)]
            return a.reshape(want[::-1])
        if tok == "RO":
            perm = [int(v) for v in f[1:5]]
            return a.permute([3 - perm[3 - j] for j in range(4)]).contiguous()
        if tok == "WN":
            assert f[1] == "0" and f[2] == "L", f
            v, g, b = next(it), next(it), next(it)           # (out, in) ArrayFire == torch [in][out]; g (out, 1)
            w = v * (g.reshape(1, -1) / v.norm(dim=0, keepdim=True))
            return a @ w + b
        if tok == "L":
            w, b = next(it), next(it)
            return a @ w + b
        if tok == "C":
            cin, cout, kw, stride, pad = (int(v) for v in f[1:6])
            w, b = next(it), next(it)                        # (kw, 1, cin, cout) ArrayFire == torch [cout][cin][1][kw]
            assert a.shape[1] == cin and a.shape[2] == 1, (f, a.shape)
            p = same_pad(a.shape[3], kw, stride) if pad == -1 else pad
            return F.conv2d(F.pad(a, (p, p)), w, b.reshape(-1), stride=(1, stride))
        if tok == "R":
            self.pre_relu.append(a)
            return torch.relu(a)
        if tok == "DO":
            return a
        if tok == "LN":
            assert f[1:] == ["0", "1", "2"], f
            gb = next(it)
            return F.layer_norm(a, a.shape[1:], eps=1e-5) * gb[0] + gb[1]
        if tok == "M":
            w, wy, s, sy = (int(v) for v in f[1:5])
            assert wy == 1 and sy == 1, f
            return F.max_pool2d(a, (1, w), (1, s))
        raise AssertionError(f)

    def _run(self, lines, a, it):
        i = 0
        while i < len(lines):
            f = lines[i]
            if f[0] != "RES":
                a = self._layer(f, a, it)
                i += 1
                continue
            n_layers, n_skips, blocks = int(f[1]), int(f[2]), int(f[3])
            body, proj, skip, taken, j = [], [], None, 0, i + 1
            while taken < n_layers + n_skips:
                g = lines[j]
                j += 1
                taken += 1
                if g[0] in ("SKIP", "SKIPL"):
                    assert skip is None and g[1] == "0" and int(g[2]) == n_layers + 1, g
                    skip = g
                    if g[0] == "SKIPL":
                        proj = lines[j:j + int(g[3])]
                        j += int(g[3])
                else:
                    body.append(g)
            scale_at = 4 if skip[0] == "SKIPL" else 3
            scale = float(F32(skip[scale_at])) if len(skip) > scale_at else 1.0
            for _ in range(blocks):
                # parameters in arch-line order, the projection's at the place of its SKIPL line: the body is cut there
                cut = sum(1 for g in lines[i + 1:lines.index(skip, i)] if g[0] not in ("SKIP", "SKIPL"))
                fx = self._run(body[:cut], a, it)
                held = [next(it) for _ in range(self._count(proj))]
                fx = self._run(body[cut:], fx, it)
                px = self._run(proj, a, iter(held))
                a = scale * (fx + px)
            i = j
        return a

    @staticmethod
    def _count(lines):
        n = 0
        for g in lines:
            n += {"C": 2, "L": 2, "LN": 1, "WN": 3}.get(g[0], 0)
        return n

    def forward(self, x, params):
        self.pre_relu = []
        a = x[:, None, :, :]                                  # (T, NFEAT, 1, B)
        it = iter(params)
        a = self._run(self.lines, a, it)
        assert next(it, None) is None, "parameters left over"
        assert a.shape[0] == 1, a.shape                        # (N, T', B, 1)
        return a[0]                                            # [B][T'][N]


def to_torch(ref_params, table_shapes):
    """the reference-layout arrays of Trainer.export_from(), as float64 leaf tensors in the restatement's shapes"""
    out = []
    for p, shape in zip(ref_params, table_shapes):
        out.append(torch.tensor(np.asarray(p, np.float64).reshape(shape[::-1]), requires_grad=True))
    return out


def ctc_loss(emission, targets):
    """per-utterance CTC loss over all T' frames, blank = the last label, scaled by 1 / sqrt(target length); targets [B][L], -1 padded"""
    B, T, N = emission.shape
    lens = [int((t >= 0).sum()) for t in targets]
    lp = F.log_softmax(emission, dim=2).permute(1, 0, 2)
    flat = torch.tensor(np.concatenate([t[:n] for t, n in zip(targets, lens)]).astype(np.int64))
    loss = F.ctc_loss(lp, flat, torch.full((B,), T, dtype=torch.long), torch.tensor(lens), blank=N - 1, reduction="none", zero_infinity=False)
    return loss / torch.sqrt(torch.tensor(lens, dtype=torch.float64))
