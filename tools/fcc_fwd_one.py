"""w2l_fcc_forward alone at the config-4 criterion shape, timed with events.   usage: fcc_fwd_one.py [B T N]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wav2letter_amd import _lib
B, T, N = (int(v) for v in sys.argv[1:4]) if len(sys.argv) > 3 else (64, 2000, 30)
L = _lib.lib(); s = torch.cuda.current_stream().cuda_stream
x = torch.randn(B, T, N, device="cuda"); trans = (torch.eye(N) * 4 + 0.1 * torch.randn(N, N)).cuda()
ts = torch.full((B,), 100, dtype=torch.int32, device="cuda"); loss = torch.empty(B, device="cuda")
ws = torch.empty(L.w2l_fcc_workspace_size(B, T, N), dtype=torch.uint8, device="cuda")
def f(): assert L.w2l_fcc_forward(B, T, N, 4, x.data_ptr(), ts.data_ptr(), trans.data_ptr(), loss.data_ptr(), ws.data_ptr(), s) == 0
for _ in range(3): f()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20): f()
e1.record(); torch.cuda.synchronize()
print("fcc_forward B=%d T=%d N=%d: %.1f us (%.0f cycles per frame at 2.4 GHz)" % (B, T, N, e0.elapsed_time(e1) / 20 * 1e3, e0.elapsed_time(e1) / 20 * 1e3 * 2400 / T))
