"""w2l_adam_step_guarded against w2l_adadelta_step_guarded on the same parameter and gradient arena in the same process: both read
p, g and two state arrays and write p and the two state arrays back, 28 bytes per parameter.  n = the network parameter floats of
BASELINE configs 2 (TDS-CTC) and 5 (Transformer-CTC), from w2l_trainer_net_param_floats.  Windows of `inner` launches between two
events (none inside the window), the kernels alternating; the median window per kernel is reported.  Each optimizer is timed as
two series on two state-array pairs of its own ("adadelta" / "adadelta_again", "adam" / "adam_again"): the distance between the
two medians of ONE kernel -- repetition and the placement of its arrays -- is the spread a difference between Adam and Adadelta
has to exceed to mean anything.  Adam also runs with the device counter (its one-thread launch behind every step included) and
with weight decay.   python tools/adam_one.py [windows] [inner]"""
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
    gen = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randn(n, device="cuda", generator=gen)
    g = torch.randn(n, device="cuda", generator=gen) * 1e-2
    # each series its own two state arrays: [adadelta, adam, adadelta_again, adam_again]
    state = [(torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")) for _ in range(4)]
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    step = [0]

    def adam(pair=1, wd=0.0, counter=False):
        step[0] += 1
        m, v = state[pair]
        return L.w2l_adam_step_guarded(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-4, 0.9, 0.999, 1e-8, wd, 1.0, 0.0, None,
                                       0 if counter else step[0], count.data_ptr() if counter else None, s)

    def adadelta(pair=0):
        ag, ad = state[pair]
        return L.w2l_adadelta_step_guarded(p.data_ptr(), g.data_ptr(), ag.data_ptr(), ad.data_ptr(), n, 1e-2, 0.9, 1e-8, 1.0, 0.0, None, s)
    fns = {"adadelta": adadelta, "adam": adam, "adadelta_again": lambda: adadelta(2), "adam_again": lambda: adam(3),
           "adam_counter": lambda: adam(counter=True), "adam_wd": lambda: adam(wd=0.01)}
    for f in fns.values():   # warm-up: code objects, clocks
        for _ in range(5):
            assert f() == 0
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            t[k].append(window(f))
    assert torch.isfinite(p).all()
    med = {k: statistics.median(x) for k, x in t.items()}
    gb = 28.0 * n / 1e9
    print("[adam] " + json.dumps({
        "n": n, "where": tag, "gbytes_per_launch": round(gb, 3), "windows": windows, "launches_per_window": inner,
        **{f"{k}_us": round(x, 1) for k, x in med.items()},
        **{f"{k}_min_max_us": [round(min(t[k]), 1), round(max(t[k]), 1)] for k in t},
        **{f"{k}_TBps": round(gb / x * 1e3, 2) for k, x in med.items()},
        "adam_over_adadelta": round(med["adam"] / med["adadelta"], 3),
        "adadelta_spread_us": round(abs(med["adadelta"] - med["adadelta_again"]), 1),
        "adam_spread_us": round(abs(med["adam"] - med["adam_again"]), 1),
        "adam_minus_adadelta_us": round(med["adam"] - med["adadelta"], 1),
        "adam_again_minus_adadelta_again_us": round(med["adam_again"] - med["adadelta_again"], 1)}), flush=True)
    del p, g, state
