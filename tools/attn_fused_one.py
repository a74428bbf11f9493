"""w2l_attn_fused_forward at one geometry, timed with events next to the unfused launch sequence on the same operands (three
alternating windows each); W2L_AF_ABL / W2L_AF_BPW (probe build) select ablations
usage: attn_fused_one.py B H T d csz p"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wav2letter_amd import _lib
if os.environ.get("W2L_AF_ABL") is not None or os.environ.get("W2L_AF_BPW") is not None: _lib.use_probe().__enter__()
B, H, T, d, csz = [int(v) for v in sys.argv[1:6]]
p = float(sys.argv[6]) if len(sys.argv) > 6 else 0.2
L = _lib.lib(); Cc = H * d
q, k, v = [torch.randn(B, T, Cc, device="cuda") for _ in range(3)]
E = torch.randn(2 * csz - 1, d, device="cuda") * 0.5
n0 = csz - 1; rlo = max(0, n0 - (T - 1)); W = min(2 * csz - 1, n0 + T) - rlo
P = torch.empty(B, H, T, T, device="cuda"); Pd = torch.empty_like(P); ctx = torch.empty(B, T, Cc, device="cuda")
D = _lib.AttnFusedDesc(B=B, H=H, T=T, d=d, ld=Cc, ldc=Cc, W=W, n0=n0, rlo=rlo, scale=d ** -0.5, dropP=p, dropSeed=1, dropStream=2)
s = torch.cuda.current_stream().cuda_stream
def run():
    st = L.w2l_attn_fused_forward(C.byref(D), q.data_ptr(), k.data_ptr(), v.data_ptr(), E.data_ptr(), None, P.data_ptr(),
                                  Pd.data_ptr() if p > 0 else None, ctx.data_ptr(), s)
    assert st == 0, st
# the unfused sequence on the same operands (host/net.cpp: scores, position product, masked softmax, dropout copy, P V)
TC, TT = T * Cc, T * T; ldr = (W + 3) // 4 * 4
S2 = torch.empty(B, H, T, T, device="cuda"); Pd2 = torch.empty_like(S2); R = torch.empty(B * T * H, ldr, device="cuda"); ctx2 = torch.empty_like(ctx)
G = _lib.BgemmDesc
def unfused():
    g = G(M=T, N=T, K=d, G1=B, G2=H, sam=Cc, sak=1, a1=TC, a2=d, sbk=1, sbn=Cc, b1=TC, b2=d, ldc=T, c1=H * TT, c2=TT)
    L.w2l_bgemm_bf16(C.byref(g), q.data_ptr(), k.data_ptr(), S2.data_ptr(), s)
    g = G(M=B * T * H, N=W, K=d, G1=1, G2=1, sam=d, sak=1, sbk=1, sbn=d, ldc=ldr)
    L.w2l_bgemm_bf16(C.byref(g), q.data_ptr(), E[rlo:].data_ptr(), R.data_ptr(), s)
    L.w2l_attn_softmax_forward(S2.data_ptr(), R.data_ptr(), None, B, H, T, ldr, rlo, W, n0, d ** -0.5, s)
    if p > 0: L.w2l_dropout_copy(Pd2.data_ptr(), S2.data_ptr(), B * H * TT, p, 1, 2, s)
    g = G(M=T, N=d, K=T, G1=B, G2=H, sam=T, sak=1, a1=H * TT, a2=TT, sbk=Cc, sbn=1, b1=TC, b2=d, ldc=Cc, c1=TC, c2=d)
    L.w2l_bgemm_bf16(C.byref(g), (Pd2 if p > 0 else S2).data_ptr(), v.data_ptr(), ctx2.data_ptr(), s)
def timeit(f, n=200):
    for _ in range(5): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
rounds = [(timeit(run), timeit(unfused)) for _ in range(3)]   # alternating windows of 200 calls
print("attn_fused B=%d H=%d T=%d d=%d csz=%d p=%.1f abl=%s bpw=%s: fused %s us, unfused sequence %s us" % (
    B, H, T, d, csz, p, os.environ.get("W2L_AF_ABL", "-"), os.environ.get("W2L_AF_BPW", "-"),
    " / ".join("%.1f" % a for a, _ in rounds), " / ".join("%.1f" % b for _, b in rounds)))
