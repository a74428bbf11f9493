"""The depthwise time convolution (w2l_conv_depthwise_*) and Swish against two yardsticks in the same process:
  * w2l_axpy over the same number of bytes -- the traffic floor.  A depthwise pass moves 8 bytes per element (forward: x in, y out;
    data gradient: dy in, dx out; filter gradient: x and dy in), Swish forward 8 and Swish backward 12; w2l_axpy moves 12 per element,
    so each is set against axpy on bytes / 12 elements.  axpy is timed as two series on operand pairs of its own: the distance
    between their medians is the spread, and "over_2x" says whether a pass costs more than twice axpy's median plus twice that spread;
  * what a user had before: w2l_conv_forward / _backward_data / _backward_filter on the dense [kw][C][C] filter with the depthwise
    taps on its diagonal (fewer, shorter windows: a launch takes milliseconds).
Shapes: B = 16, T = 500, C in {512, 768, 1024}, kw in {15, 31}, SAME padding.  These are ASSUMPTIONS -- the reference tree holds no
Conformer arch file, and nobody has measured a workload of this kind here.  Windows of `inner` launches
between two events (none inside the window), the kernels alternating; the median window per kernel is reported.
  python tools/depthwise_one.py [windows] [inner]"""
import ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wav2letter_amd import _lib

L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream
B, T = 16, 500


def window(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        assert fn() == 0
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3   # us per launch


def medians(fns, windows, inner):
    for f in fns.values():   # warm-up: code objects, scratch, clocks
        for _ in range(3):
            assert f() == 0
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            t[k].append(window(f, inner))
    return {k: statistics.median(v) for k, v in t.items()}


def one(C, kw, windows, inner):
    n = B * T * C
    pad = kw // 2
    gen = torch.Generator(device="cuda").manual_seed(1)
    x, dy, y, dx, a0, a1, a2, a3 = (torch.randn(n, device="cuda", generator=gen) * 1e-2 for _ in range(8))
    w = torch.randn(kw, C, device="cuda", generator=gen)
    bias, dw, db = torch.randn(C, device="cuda", generator=gen), torch.empty(kw, C, device="cuda"), torch.empty(C, device="cuda")
    d = _lib.ConvDesc(B, T, 1, C, C, kw, 1, pad, pad)
    dp = ctypes.byref(d)
    ws = torch.empty(L.w2l_conv_depthwise_workspace_floats(dp), device="cuda")
    n8, p = 8 * n // 12, lambda t: t.data_ptr()
    fns = {"axpy_8B": lambda: L.w2l_axpy(p(a0), p(a1), n8, 1e-3, s),
           "dw_fwd": lambda: L.w2l_conv_depthwise_forward(dp, p(x), p(w), p(bias), p(y), s),
           "dw_bwd_data": lambda: L.w2l_conv_depthwise_backward_data(dp, p(dy), p(w), p(dx), s),
           "dw_bwd_filter": lambda: L.w2l_conv_depthwise_backward_filter(dp, p(x), p(dy), p(dw), p(db), p(ws), s),
           "swish_fwd": lambda: L.w2l_swish_forward(p(x), p(y), n, 1.0, s),
           "axpy_8B_again": lambda: L.w2l_axpy(p(a2), p(a3), n8, 1e-3, s),
           "axpy_12B": lambda: L.w2l_axpy(p(a0), p(a1), n, 1e-3, s),
           "swish_bwd": lambda: L.w2l_swish_backward(p(x), p(dy), p(dx), n, 1.0, s),
           "axpy_12B_again": lambda: L.w2l_axpy(p(a2), p(a3), n, 1e-3, s)}
    med = medians(fns, windows, inner)
    # the dense convolution with the taps on the diagonal
    wd = torch.zeros(kw, C, C, device="cuda")
    wd[:, torch.arange(C), torch.arange(C)] = w
    dwd = torch.empty_like(wd)
    dense = medians({"dense_fwd": lambda: L.w2l_conv_forward(dp, p(x), p(wd), p(bias), p(y), 0, s),
                     "dense_bwd_data": lambda: L.w2l_conv_backward_data(dp, p(dy), p(wd), p(dx), 0, s),
                     "dense_bwd_filter": lambda: L.w2l_conv_backward_filter(dp, p(x), p(dy), p(dwd), p(db), s)}, 3, 2)
    out = {"B": B, "T": T, "C": C, "kw": kw, "elements": n, "windows": windows, "launches_per_window": inner,
           **{f"{k}_us": round(v, 2) for k, v in {**med, **dense}.items()}}
    for floor, names in (("axpy_8B", ("dw_fwd", "dw_bwd_data", "dw_bwd_filter", "swish_fwd")), ("axpy_12B", ("swish_bwd",))):
        spread = abs(med[floor] - med[floor + "_again"])
        out[floor + "_spread_us"] = round(spread, 2)
        for k in names:
            out[k + "_over_axpy"] = round(med[k] / med[floor], 2)
            out[k + "_over_2x"] = bool(med[k] > 2 * med[floor] + 2 * spread)
    for k in ("fwd", "bwd_data", "bwd_filter"):
        out[f"dense_over_dw_{k}"] = round(dense["dense_" + k] / med["dw_" + k], 1)
    print("[depthwise] " + json.dumps(out), flush=True)


if __name__ == "__main__":
    windows, inner = (int(sys.argv[1]) if len(sys.argv) > 1 else 15), (int(sys.argv[2]) if len(sys.argv) > 2 else 20)
    for C in (512, 768, 1024):
        for kw in (15, 31):
            one(C, kw, windows, inner)
