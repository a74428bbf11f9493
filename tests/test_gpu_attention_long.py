"""The long-sequence family of the fused attention kernels (attention_fused_long.hip: 192 < T <= 512, keys streamed through LDS)
and head width 192 in both families, through the unchanged C ABI.  Shapes: the first length past the short family, tile and
chunk edges, the recipe's table, the largest length, every head width, dropout, ragged batches, no table, a table shorter than
the sequence."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_gpu_attention as TA
from tests import test_gpu_trainer as TT

pytestmark = pytest.mark.gpu
rel, _stream = TA.rel, TA._stream


@pytest.mark.parametrize("B,H,T,d,csz,p,ragged", [
    (1, 2, 193, 32, 460, 0.0, False), (2, 1, 193, 192, 460, 0.2, True), (1, 1, 193, 256, 40, 0.0, False),
    (2, 2, 225, 32, 0, 0.1, True), (1, 2, 257, 32, 460, 0.0, False), (1, 1, 300, 32, 40, 0.2, False),
    (2, 1, 321, 32, 460, 0.0, True), (1, 2, 460, 32, 460, 0.2, False), (1, 1, 511, 32, 460, 0.0, False),
    (1, 1, 512, 192, 460, 0.2, False), (2, 1, 512, 256, 460, 0.0, True), (1, 2, 512, 32, 0, 0.0, False),
    (2, 2, 33, 192, 7, 0.1, True), (1, 2, 188, 192, 460, 0.2, False)])
def test_fused_attention_forward_long(B, H, T, d, csz, p, ragged):
    """tests/test_gpu_attention.py's forward check at its own bars: P 2e-5 against float64 on the bf16-rounded operands, ctx from the
    kernel's own P, P 2e-6 against the unfused sequence, Pd bit-equal to w2l_dropout_copy"""
    TA.test_fused_attention_forward(B, H, T, d, csz, p, ragged)


def _tp(T):
    nt = (T + 31) // 32
    return 32 * (2 if nt <= 2 else 4 if nt <= 4 else 6) if nt <= 6 else 64 * ((T + 63) // 64)


@pytest.mark.parametrize("B,H,T,d,csz,p,ragged", [
    (1, 2, 193, 32, 460, 0.2, False), (2, 1, 193, 192, 40, 0.0, True), (1, 1, 257, 256, 460, 0.1, False),
    (1, 2, 460, 32, 460, 0.0, False), (2, 1, 512, 192, 0, 0.2, True), (1, 1, 512, 256, 460, 0.0, False),
    (2, 1, 100, 192, 460, 0.1, True)])
def test_fused_attention_backward_long(B, H, T, d, csz, p, ragged):
    """test_fused_attention_backward's method for any tile rounding: the dS^T image at the head of the workspace against float64 on
    the same rounded operands at bf16 resolution (2^-8 of the largest entry), the Pd^T image bit for bit, dq / dk / dv / dPosTable
    from the kernel's own dS at 2e-5 of the largest magnitude (only fp32 accumulation differs), dPosTable zero outside the reached
    rows, a workspace one byte short refused, the bf16 image sinks bit-equal to rounding the fp32 results.  The ragged batch's second
    utterance has 40 valid keys: it ends inside the first key chunk."""
    from wav2letter_amd import _lib
    L = _lib.lib()
    g = torch.Generator().manual_seed(T * 11 + d + csz)
    Cc = H * d
    q, k, v, dctx = (torch.randn(B, T, Cc, generator=g).cuda() for _ in range(4))
    E = (torch.randn(max(1, 2 * csz - 1), d, generator=g) * 0.5).cuda()
    n0 = csz - 1
    rlo = max(0, n0 - (T - 1)) if csz else 0
    W = (min(2 * csz - 1, n0 + T) - rlo) if csz else 0
    scale = 1.0 / np.sqrt(d)
    keyLen = torch.tensor([T, 40][:B], dtype=torch.int32).cuda() if ragged else None
    P, Pd, ctx, dq, dk, dv = (torch.full(s, float("nan"), device="cuda") for s in [(B, H, T, T)] * 2 + [(B, T, Cc)] * 4)
    dE = torch.full((max(1, 2 * csz - 1), d), float("nan"), device="cuda")
    D = _lib.AttnFusedDesc(B=B, H=H, T=T, d=d, ld=Cc, ldc=Cc, W=W, n0=n0, rlo=rlo, scale=scale, dropP=p, dropSeed=977, dropStream=3)
    ptr = lambda t: t.data_ptr() if t is not None else None
    Ep, dEp = (ptr(E), ptr(dE)) if csz else (None, None)
    assert L.w2l_attn_fused_forward(C.byref(D), ptr(q), ptr(k), ptr(v), Ep, ptr(keyLen), ptr(P), ptr(Pd) if p > 0 else None, ptr(ctx),
                                    _stream()) == 0
    if ragged:
        assert float(P[1, :, :, 40:].abs().max()) == 0.0 and rel(P.sum(-1).cpu().numpy(), np.ones((B, H, T))) < 1e-5
    if p == 0:
        Pd = P
    nws = L.w2l_attn_fused_backward_workspace(C.byref(D), 1 if csz else 0)
    assert nws > 0
    ws = torch.full((nws,), 0xff, dtype=torch.uint8, device="cuda")     # (0xffff: a bf16 NaN in every unwritten slot)
    bwd = lambda n: L.w2l_attn_fused_backward(C.byref(D), ptr(q), ptr(k), ptr(v), Ep, ptr(P), ptr(dctx), ptr(dq), ptr(dk), ptr(dv), dEp,
                                              ptr(ws), n, _stream())
    assert bwd(nws) == 0
    assert bwd(nws - 1) != 0
    # the bf16 image sinks: bit for bit the rounding of the fp32 results, nothing outside the matrix touched
    M = B * T
    ldR, ldT = (Cc + 63) // 64 * 64 + 64, (M + 63) // 64 * 64
    sinks = []
    for _ in range(4):
        rows = torch.full((M, ldR), 7.0, dtype=torch.bfloat16, device="cuda")
        trans = torch.full((Cc, ldT), 7.0, dtype=torch.bfloat16, device="cuda")
        sinks.append((rows, trans, _lib.Bf16ImageSink(rowMajor=rows.data_ptr(), ldRows=ldR, transposed=trans.data_ptr(), ldTrans=ldT)))
    dE_i, P_i, Pd_i = torch.full_like(dE, float("nan")), torch.empty_like(P), torch.empty_like(P)
    assert L.w2l_attn_fused_backward_images(C.byref(D), ptr(q), ptr(k), ptr(v), Ep, ptr(P), ptr(dctx), None, None, None, C.byref(sinks[0][2]),
                                            C.byref(sinks[1][2]), C.byref(sinks[2][2]), ptr(dE_i) if csz else None, ptr(ws), nws,
                                            _stream()) == 0
    assert L.w2l_attn_fused_forward_images(C.byref(D), ptr(q), ptr(k), ptr(v), Ep, ptr(keyLen), ptr(P_i), ptr(Pd_i) if p > 0 else None, None,
                                           C.byref(sinks[3][2]), _stream()) == 0
    assert torch.equal(P_i, P)
    for (rows, trans, _), ref32 in zip(sinks, (dq, dk, dv, ctx)):
        want = ref32.reshape(M, Cc).bfloat16()
        assert torch.equal(rows[:, :Cc], want) and torch.equal(trans[:, :M], want.t())
        assert bool((rows[:, Cc:] == 7.0).all()) and bool((trans[:, M:] == 7.0).all())
    # float64 on the bf16-rounded operands
    r = lambda x: x.bfloat16().double()
    heads = lambda x: x.reshape(B, T, H, d).permute(0, 2, 1, 3)
    unheads = lambda x: x.permute(0, 2, 1, 3).reshape(B, T, Cc)
    qh, kh, vh, dch = heads(r(q)), heads(r(k)), heads(r(v)), heads(r(dctx))
    dP = dch @ vh.transpose(-1, -2)
    if p > 0:
        dP = dP * (Pd != 0).double() / (1.0 - p)
    P64 = P.double()
    dS64 = scale * P64 * (dP - (P64 * dP).sum(-1, keepdim=True))
    TP = _tp(T)
    img = ws[:2 * B * H * TP * TP * 2].view(torch.bfloat16).view(2, B, H, TP, TP)
    dSk = img[0, :, :, :T, :T].transpose(-1, -2).double()          # the kernel's dS, [query][key]
    assert rel(dSk.cpu().numpy(), dS64.cpu().numpy()) < 4.2e-3
    assert torch.equal(img[1, :, :, :T, :T].transpose(-1, -2), Pd.bfloat16())
    if TP > T:
        assert float(img[:, :, :, T:, :T].float().abs().max()) == 0.0   # padded key rows
    dq_ref, dk_ref, dv_ref = dSk @ kh, dSk.transpose(-1, -2) @ qh, r(Pd).transpose(-1, -2) @ dch
    if csz:
        dE_ref, Er = torch.zeros_like(dE, dtype=torch.float64), r(E)
        for delta in range(max(-(T - 1), -n0), min(T, csz)):
            diag = dSk.diagonal(offset=delta, dim1=-2, dim2=-1)    # [B][H][n]: entries (i, i + delta)
            lo, n = max(0, -delta), diag.shape[-1]
            dq_ref[:, :, lo:lo + n] += diag[..., None] * Er[delta + n0]
            dE_ref[delta + n0] += (diag[..., None] * qh[:, :, lo:lo + n]).sum((0, 1, 2))
        assert torch.equal(dE_i, dE) and rel(dE.cpu().numpy(), dE_ref.cpu().numpy()) < 2e-5
        assert rlo == 0 or float(dE[:rlo].abs().max()) == 0.0       # rows no frame pair reaches
    for got, want in ((dq, dq_ref), (dk, dk_ref), (dv, dv_ref)):
        assert rel(got.cpu().numpy(), unheads(want).cpu().numpy()) < 2e-5


@pytest.mark.parametrize("T,d", [(513, 32), (200, 64), (100, 64)])
def test_fused_attention_refusals(T, d):
    """T > 512 and other head widths: W2L_EUNSUPPORTED from both calls, workspace size 0"""
    from wav2letter_amd import _lib
    L = _lib.lib()
    x = torch.zeros(1, T, d, device="cuda")
    P = torch.zeros(1, 1, T, T, device="cuda")
    D = _lib.AttnFusedDesc(B=1, H=1, T=T, d=d, ld=d, ldc=d, W=0, n0=0, rlo=0, scale=1.0, dropP=0.0, dropSeed=1, dropStream=1)
    unsupported = [c for c, n in _lib._ERR.items() if "UNSUPPORTED" in str(n)]
    assert L.w2l_attn_fused_forward(C.byref(D), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, P.data_ptr(), None, x.data_ptr(),
                                    _stream()) in unsupported
    assert L.w2l_attn_fused_backward_workspace(C.byref(D), 0) == 0 and L.w2l_attn_fused_backward_workspace(C.byref(D), 1) == 0
    ws = torch.zeros(256, dtype=torch.uint8, device="cuda")
    dx = [torch.zeros_like(x) for _ in range(3)]
    assert L.w2l_attn_fused_backward(C.byref(D), x.data_ptr(), x.data_ptr(), x.data_ptr(), None, P.data_ptr(), x.data_ptr(), dx[0].data_ptr(),
                                     dx[1].data_ptr(), dx[2].data_ptr(), None, ws.data_ptr(), 256, _stream()) in unsupported


def test_transformer_blocks_bf16_long_sequence(oracle):
    """two mixed-precision TR blocks (dim 64, 2 heads: head width 32; csz 300) on a ragged batch of 250 frames -- in the trainer the
    long family's fused backward after the unfused forward (host/net.cpp fusedForwardPays) -- at the bars of
    test_transformer_block_bf16_geometries"""
    TT.test_transformer_block_bf16_geometries(oracle, "TR 64 128 2 300 0.0 0.0\nTR 64 128 2 300", 2, 250, [25000.0, 17000.0])
