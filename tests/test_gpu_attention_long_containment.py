"""Containment (tests/test_gpu_containment.py) of the long-sequence fused attention kernels: forward and backward on the guarded
arena of tests/arena.py -- operands read only inside, results written in full, nothing outside the declared workspace touched,
results independent of the bytes around the operands."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_gpu_containment as TC
from wav2letter_amd import _lib

pytestmark = pytest.mark.gpu
GRADS = "float64 restatement from the kernel's own dS: tests/test_gpu_attention_long.py::test_fused_attention_backward_long"


def _case(B, H, T, d, csz, p, ragged):
    name = f"attn_fused_long/B={B},H={H},T={T},d={d},csz={csz},p={p}" + (",keyLen" if ragged else "")

    @TC.case(name, capacity=64 << 20)
    def _(r):
        from oracle import pyoracle
        from oracle import transformer_oracle as TO
        g = torch.Generator().manual_seed(T * 7 + d + csz)
        Cc = H * d
        q, k, v, dctx = (torch.randn(B, T, Cc, generator=g) for _ in range(4))
        E = torch.randn(max(1, 2 * csz - 1), d, generator=g) * 0.5
        n0 = csz - 1
        rlo = max(0, n0 - (T - 1)) if csz else 0
        W = (min(2 * csz - 1, n0 + T) - rlo) if csz else 0
        scale = float(1.0 / np.sqrt(d))
        kl = np.array([T, 40][:B], np.int32)
        D = _lib.AttnFusedDesc(B=B, H=H, T=T, d=d, ld=Cc, ldc=Cc, W=W, n0=n0, rlo=rlo, scale=scale, dropP=p, dropSeed=4321, dropStream=5)
        pq, pk, pv = r.inp("q", q.numpy()), r.inp("k", k.numpy()), r.inp("v", v.numpy())
        pE = r.inp("posTable", E.numpy()) if csz else None
        pP = r.out("P", (B, H, T, T))
        pPd = r.out("Pd", (B, H, T, T)) if p > 0 else None
        r.ok(r.L.w2l_attn_fused_forward(C.byref(D), pq, pk, pv, pE, r.inp("keyLen", kl) if ragged else None, pP, pPd, r.out("ctx", (B, T, Cc)),
                                        TC._stream()), "forward")
        nws = r.L.w2l_attn_fused_backward_workspace(C.byref(D), 1 if csz else 0)
        assert nws > 0
        r.ok(r.L.w2l_attn_fused_backward(C.byref(D), pq, pk, pv, pE, pP, r.inp("dctx", dctx.numpy()), r.out("dq", (B, T, Cc)),
                                         r.out("dk", (B, T, Cc)), r.out("dv", (B, T, Cc)), r.out("dPosTable", (2 * csz - 1, d)) if csz else None,
                                         r.work("ws", nws), nws, TC._stream()), "backward")
        got = {key: r.view(key) for key in (("P", "Pd") if p > 0 else ("P",))}

        def ref():
            rd = lambda x: x.bfloat16().double()
            heads = lambda x: x.reshape(B, T, H, d).permute(0, 2, 1, 3)
            qh, kh, vh = heads(rd(q)), heads(rd(k)), heads(rd(v))
            S = qh @ kh.transpose(-1, -2)
            if csz:
                S = S + TO.relative_position_rotate(qh @ rd(E).t())[..., E.shape[0] // 2:E.shape[0] // 2 + T]
            S = S * scale
            if ragged:
                S = S.masked_fill(torch.arange(T)[None, None, None, :] >= torch.from_numpy(kl).long()[:, None, None, None], float("-inf"))
            Pk = got["P"].cpu()
            Pdk = got["Pd"].cpu() if p > 0 else Pk
            bar = ("rel", 2e-5)
            out = {"P": (bar, torch.softmax(S, dim=-1).numpy()), "ctx": (bar, (rd(Pdk) @ vh).permute(0, 2, 1, 3).reshape(B, T, Cc).numpy())}
            if p > 0:
                out["Pd"] = ("exact", pyoracle.dropout(Pk.numpy().reshape(-1), p, 4321, 5).reshape(B, H, T, T))
            out.update({key: ("none", GRADS) for key in ("dq", "dk", "dv", "dPosTable")})
            return out
        return ref
    return name


NAMES = [_case(1, 2, 193, 32, 460, 0.0, False), _case(1, 1, 512, 192, 460, 0.0, False), _case(2, 1, 257, 32, 40, 0.2, True)]


@pytest.mark.parametrize("name", NAMES)
def test_containment_long(name):
    TC.run_case(name)
