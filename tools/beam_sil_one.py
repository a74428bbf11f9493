"""The beam searches with a silence score (w2l_*_beam_search*_sil, silScore = -1 on token 0) against their siblings on the same
emissions in the same process, timed with hip events after warm-up:
    python tools/beam_sil_one.py [reps] [pieces|letters] [K ...]
  pieces   B = 32, N = 9998, T = 188, K = 64 and 8 (or the K given): the five searches -- ctc (LM-free), ctc_lm, ctc_lex, asg (with a
           token LM), asg_lex
  letters  B = 64, N = 30, T = 1000, K = 30 and 8: the ASG pair
Each search runs in the three kernel families -- narrow W = 64, wide W = 1024, xl W = 2500 -- as the sibling's entry point and as
the *_sil one.  Max search on the raw emissions, no threshold, nbest = 1; the models are tools/asg_beam_one.py's.  A run is one
warm-up call and `reps` timed calls between two events; the runs of a (search, family) are interleaved and repeated three times.
Prints one JSON line per (shape, K, search): the median microseconds per frame of the sibling and of the *_sil call in each family,
the spread of the runs ((max - min) / median) and the sil / sibling ratio.  Everything is expected within noise except the narrow
LM-free CTC search, which with a silence score leaves the one-wavefront lazy scan for the workgroup token scan."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from asg_beam_one import setup
from wav2letter_amd import _lib

FAMILIES = (("narrow", 0, "", 64), ("wide", 1, "_wide", 1024), ("xl", 2, "_xl", 2500))
ROUNDS = 3
SIL, SIL_SCORE = 0, -1.0


def bench(B, T, N, K, hot, reps, searches, tok_lm_asg, tok_lm_ctc, lex_asg, lex_ctc, word_lm):
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(B, T, N, generator=g)
    x[:, :, :hot] += 2.0
    x = x.cuda()
    A = torch.zeros(N, N)
    A[:hot, :hot] = torch.randn(hot, hot, generator=g)
    A += 2.0 * torch.eye(N)
    A = A.cuda()
    ws = torch.empty(max(L.w2l_asg_beam_lex_sil_workspace_size(2, B, T, N, 2500, K), L.w2l_ctc_beam_lex_sil_workspace_size(2, B, T, N, 2500, K),
                         L.w2l_asg_beam_lex_sil_workspace_size(1, B, T, N, 1024, K), L.w2l_ctc_beam_lm_sil_workspace_size(0, B, T, N, 64, K)),
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

    def call(search, family, sfx, W, sil):
        """the sibling's entry point of the family, or (sil) the *_sil one with the family in front and the score behind"""
        def pick(stem):
            if not sil:
                return getattr(L, stem + sfx)
            f = getattr(L, stem + "_sil")
            return lambda *a: f(family, *a, SIL, SIL_SCORE)
        if search == "ctc":
            f = pick("w2l_ctc_beam_search")
            return lambda: f(B, T, N, x.data_ptr(), None, W, K, inf, 0, 0, 1, T, *out4[:3], ws.data_ptr(), st)
        if search == "ctc_lm":
            f = pick("w2l_ctc_beam_search_lm")
            return lambda: f(B, T, N, x.data_ptr(), None, W, K, inf, 0, 0, 1, T, tc.data_ptr(), int(tok_lm_ctc.has_eos), 0.5, None, 0.0,
                             *out4, ws.data_ptr(), st)
        if search == "ctc_lex":
            f = pick("w2l_ctc_beam_search_lex")
            return lambda: f(B, T, N, x.data_ptr(), None, W, K, inf, 0, 0, 1, T, wl.data_ptr(), int(word_lm.has_eos), 0.5, lc.data_ptr(),
                             0.5, 0.0, *out4, T, words.data_ptr(), counts.data_ptr(), ws.data_ptr(), st)
        if search == "asg":
            f = pick("w2l_asg_beam_search")
            return lambda: f(B, T, N, x.data_ptr(), None, A.data_ptr(), W, K, inf, 0, 0, 1, T, ta.data_ptr(), int(tok_lm_asg.has_eos), 0.5,
                             None, 0.0, *out4, ws.data_ptr(), st)
        f = pick("w2l_asg_beam_search_lex")
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

    for search in searches:
        out = {"search": search, "B": B, "T": T, "N": N, "K": K}
        for name, family, sfx, W in FAMILIES:
            fns = {"sibling": call(search, family, sfx, W, False), "sil": call(search, family, sfx, W, True)}
            t = {k: [] for k in fns}
            for _ in range(ROUNDS):
                for k, fn in fns.items():
                    t[k].append(timed(fn, reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            out[f"{name}{W}"] = {"sibling_us_per_frame": round(med["sibling"] / T, 2), "sil_us_per_frame": round(med["sil"] / T, 2),
                                 "spread": round(max((max(v) - min(v)) / med[k] for k, v in t.items()), 3),
                                 "sil/sibling": round(med["sil"] / med["sibling"], 3)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    which = sys.argv[2] if len(sys.argv) > 2 else "pieces"
    ks = [int(v) for v in sys.argv[3:]]
    if which == "pieces":
        s = setup(9998, 2048, 4)
        # one emission tensor for both criteria: the CTC searches take its last column as their blank (setup's CTC models are over
        # the 9997 classes before it)
        for K in ks or (64, 8):
            bench(32, 188, 9998, K, 2048, reps, ("ctc", "ctc_lm", "ctc_lex", "asg", "asg_lex"), **s)
    if which == "letters":
        s = setup(30, 28, 3)
        for K in ks or (30, 8):
            bench(64, 1000, 30, K, 28, reps, ("asg", "asg_lex"), **s)
