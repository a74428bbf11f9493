"""w2l_ema_update (slimIPL's averaged teacher, one launch over the parameter arena) against w2l_axpy on the same n in the same
process: both read two arrays and write one, 12 bytes per element.  n = the network parameter floats of BASELINE configs 2
(TDS-CTC) and 5 (Transformer-CTC), from w2l_trainer_net_param_floats.  Windows of `inner` launches between two events (none
inside the window), the two kernels alternating; the median window per kernel is reported, and the EMA at the float offsets
(1, 3) from a 16-byte boundary next to the aligned one.   python tools/ema_one.py [windows] [inner]"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wav2letter_amd import CriterionScaleMode, _lib, recipes
from wav2letter_amd.trainer import Trainer

windows = int(sys.argv[1]) if len(sys.argv) > 1 else 15
inner = int(sys.argv[2]) if len(sys.argv) > 2 else 10
L = _lib.lib()
s = torch.cuda.current_stream().cuda_stream


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner * 1e3   # us per launch


for tag, arch, nfeat, nlabel in (("config 2 (TDS-CTC)", recipes.tds_ctc_arch(), 80, 9998),
                                 ("config 5 (Transformer-CTC)", recipes.transformer_ctc_arch(), 80, 9998)):
    tr = Trainer(arch, nfeat, nlabel, "ctc", CriterionScaleMode.TARGET_SZ_SQRT)
    n = int(tr.n_net)
    del tr
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.randn(n + 8, device="cuda", generator=g)
    b = torch.randn(n + 8, device="cuda", generator=g)
    P = lambda t, off: t.data_ptr() + 4 * off
    fns = {
        "axpy": lambda: L.w2l_axpy(P(a, 0), P(b, 0), n, 1e-3, s),
        "ema": lambda: L.w2l_ema_update(P(a, 0), P(b, 0), n, 0.999, s),
        "ema+1+3": lambda: L.w2l_ema_update(P(a, 1), P(b, 3), n, 0.999, s),
    }
    for f in fns.values():   # warm-up: code objects, clocks
        for _ in range(5):
            assert f() == 0
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            t[k].append(window(f))
    med = {k: statistics.median(v) for k, v in t.items()}
    gb = 12.0 * n / 1e9
    print("[ema] " + json.dumps({
        "n": n, "where": tag, "gbytes_per_launch": round(gb, 3), "windows": windows, "launches_per_window": inner,
        **{f"{k}_us": round(v, 1) for k, v in med.items()},
        **{f"{k}_min_max_us": [round(min(t[k]), 1), round(max(t[k]), 1)] for k in t},
        **{f"{k}_TBps": round(gb / v * 1e3, 2) for k, v in med.items()},
        "ema_over_axpy": round(med["ema"] / med["axpy"], 3), "ema_misaligned_over_axpy": round(med["ema+1+3"] / med["axpy"], 3)}), flush=True)
