"""The many-token beam searches (w2l_*_beam_search*_mt, K up to 256) against their xl twins on the same emissions in the same
process, timed with hip events after warm-up:
    python tools/beam_mt_one.py [reps]                      the xl twin at K = 64 against the many-token entry point at K = 64 / 100 /
                                                            150 / 256, at W = 500 (the sota/2019 configs' pair is 500 / 100) and 2500
    python tools/beam_mt_one.py [reps] parent <libw2l_hip.so of the parent commit>
                                                            the existing xl entry points (K = 64, W = 500 and 2500) of that library and
                                                            of this one in alternating runs, twice each
B = 32, N = 9998, T = 188, the five searches -- ctc (LM-free), ctc_lm, ctc_lex, asg (with a token LM), asg_lex --, max search on the
raw emissions, no threshold, nbest = 1; the models are tools/asg_beam_one.py's.  A run is one warm-up call and `reps` timed calls
between two events; the runs of a (search, W) are interleaved and repeated three times.  Prints one JSON line per (search, W): the
median microseconds per frame of every entry, the spread of the runs ((max - min) / median) and the ratios to the xl twin; in parent
mode one line per (search, W) with the four runs, the ratio of the means and the spread of the parent's two runs, which is the bar."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from asg_beam_one import setup
from wav2letter_amd import _lib

B, T, N, HOT = 32, 188, 9998, 2048
WIDTHS = (500, 2500)
KS = (64, 100, 150, 256)
ROUNDS = 3
SEARCHES = ("ctc", "ctc_lm", "ctc_lex", "asg", "asg_lex")
STEM = {"ctc": "w2l_ctc_beam_search", "ctc_lm": "w2l_ctc_beam_search_lm", "ctc_lex": "w2l_ctc_beam_search_lex",
        "asg": "w2l_asg_beam_search", "asg_lex": "w2l_asg_beam_search_lex"}


def parent_lib(path):
    """the xl entry points of another build of the library, with this build's signatures (the parent commit has them all)"""
    P = C.CDLL(path)
    for stem in STEM.values():
        f = getattr(P, stem + "_xl")
        f.restype, f.argtypes = getattr(_lib._SIGS, stem + "_xl")
    return P


def main(reps, parent):
    L = _lib.lib()
    s = setup(N, HOT, 4)
    tok_lm_asg, tok_lm_ctc, lex_asg, lex_ctc, word_lm = (s[k] for k in ("tok_lm_asg", "tok_lm_ctc", "lex_asg", "lex_ctc", "word_lm"))
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(B, T, N, generator=g)
    x[:, :, :HOT] += 2.0
    x = x.cuda()
    A = torch.zeros(N, N)
    A[:HOT, :HOT] = torch.randn(HOT, HOT, generator=g)
    A += 2.0 * torch.eye(N)
    A = A.cuda()
    kmax = 64 if parent else max(KS)
    ws = torch.empty(max(L.w2l_asg_beam_lex_mt_workspace_size(B, T, N, max(WIDTHS), kmax), L.w2l_ctc_beam_lex_mt_workspace_size(B, T, N, max(WIDTHS), kmax)),
                     dtype=torch.uint8, device="cuda")
    labels = torch.empty(B, 1, T, dtype=torch.int32, device="cuda")
    lengths = torch.empty(B, 1, dtype=torch.int32, device="cuda")
    scores = torch.empty(B, 1, device="cuda")
    lms = torch.empty(B, 1, device="cuda")
    words = torch.empty(B, 1, T, dtype=torch.int32, device="cuda")
    counts = torch.empty(B, 1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    inf = float("inf")
    out4 = (labels.data_ptr(), lengths.data_ptr(), scores.data_ptr(), lms.data_ptr())
    ta, tc, wl = tok_lm_asg.device_blob("cuda"), tok_lm_ctc.device_blob("cuda"), word_lm.device_blob("cuda")
    la, lc = lex_asg.device_blob("cuda"), lex_ctc.device_blob("cuda")

    def call(lib, search, W, K, mt):
        """the xl twin of `lib`, or (mt) the many-token entry point: the same list, then no silence token and no score"""
        f0 = getattr(lib, STEM[search] + ("_mt" if mt else "_xl"))
        f = (lambda *a: f0(*a, -1, 0.0)) if mt else f0
        if search == "ctc":
            return lambda: f(B, T, N, x.data_ptr(), None, W, K, inf, 0, 0, 1, T, *out4[:3], ws.data_ptr(), st)
        if search == "ctc_lm":
            return lambda: f(B, T, N, x.data_ptr(), None, W, K, inf, 0, 0, 1, T, tc.data_ptr(), int(tok_lm_ctc.has_eos), 0.5, None, 0.0,
                             *out4, ws.data_ptr(), st)
        if search == "ctc_lex":
            return lambda: f(B, T, N, x.data_ptr(), None, W, K, inf, 0, 0, 1, T, wl.data_ptr(), int(word_lm.has_eos), 0.5, lc.data_ptr(),
                             0.5, 0.0, *out4, T, words.data_ptr(), counts.data_ptr(), ws.data_ptr(), st)
        if search == "asg":
            return lambda: f(B, T, N, x.data_ptr(), None, A.data_ptr(), W, K, inf, 0, 0, 1, T, ta.data_ptr(), int(tok_lm_asg.has_eos), 0.5,
                             None, 0.0, *out4, ws.data_ptr(), st)
        return lambda: f(B, T, N, x.data_ptr(), None, A.data_ptr(), W, K, inf, 0, 0, 1, T, wl.data_ptr(), int(word_lm.has_eos), 0.5,
                         la.data_ptr(), 0.5, 0.0, *out4, T, words.data_ptr(), counts.data_ptr(), ws.data_ptr(), st)

    def timed(fn, n):
        _lib.check(fn(), "beam")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    P = parent_lib(parent) if parent else None
    for search in SEARCHES:
        for W in WIDTHS:
            if P is not None:
                fp, fn = call(P, search, W, 64, False), call(L, search, W, 64, False)
                runs = {"parent": [], "new": []}
                for _ in range(2):
                    runs["parent"].append(timed(fp, reps))
                    runs["new"].append(timed(fn, reps))
                mp, mn = statistics.mean(runs["parent"]), statistics.mean(runs["new"])
                print(json.dumps({"search": search, "W": W, "K": 64, "entry": "xl", "parent_us": [round(v, 1) for v in runs["parent"]],
                                  "new_us": [round(v, 1) for v in runs["new"]], "new/parent": round(mn / mp, 4),
                                  "parent_spread": round((max(runs["parent"]) - min(runs["parent"])) / mp, 4)}), flush=True)
                continue
            fns = {"xl64": call(L, search, W, 64, False)}
            fns.update({f"mt{K}": call(L, search, W, K, True) for K in KS})
            t = {k: [] for k in fns}
            for _ in range(ROUNDS):
                for k, fn in fns.items():
                    t[k].append(timed(fn, reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            out = {"search": search, "B": B, "T": T, "N": N, "W": W}
            out["us_per_frame"] = {k: round(v / T, 1) for k, v in med.items()}
            out["spread"] = round(max((max(v) - min(v)) / med[k] for k, v in t.items()), 3)
            out["mt64/xl64"] = round(med["mt64"] / med["xl64"], 3)
            out["mt100/mt64"] = round(med["mt100"] / med["mt64"], 3)
            out["mt256/mt64"] = round(med["mt256"] / med["mt64"], 3)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    parent = sys.argv[3] if len(sys.argv) > 3 and sys.argv[2] == "parent" else None
    main(reps, parent)
