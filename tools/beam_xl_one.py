"""The xl beam searches (w2l_*_beam_search*_xl) against their wide twins on the same emissions in the same process, timed with hip
events after warm-up:
    python tools/beam_xl_one.py [reps] [pieces|letters] [K ...]
  pieces   B = 32, N = 9998, T = 188, K = 64 and 8 (or the K given): the five searches -- ctc (LM-free), ctc_lm, ctc_lex, asg (with a
           token LM), asg_lex; the ASG transition matrix (400 MB) is gathered from global memory by both families
  letters  B = 64, N = 30, T = 1000, K = 30 and 8: the ASG pair; the wide kernel stages the 30 x 30 matrix in LDS, the xl kernel
           gathers it from global memory
Each search runs on the wide kernel at W = 1024 -- the yardstick -- and on the xl kernel at W = 1024, 1500, 2500, 5000 and 8192.  Max
search on the raw emissions, no threshold, nbest = 1; the models are tools/asg_beam_one.py's (a random 3-gram token model, a
synthetic lexicon of 20000 words of 1 to 4 of the favoured tokens and a random 3-gram word model).  A run is one warm-up call and
`reps` timed calls between two events; the runs of a shape are interleaved and repeated three times.  Prints one JSON line per
(shape, K, search): the median microseconds per call and per frame of every width with the spread of the runs ((max - min) /
median), the xl / wide ratio at W = 1024 and the ratio of the per-frame time at W = 8192 to the xl one at W = 1024 (8 would be a
cost linear in W)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from asg_beam_one import setup
from wav2letter_amd import _lib

WIDTHS = (1024, 1500, 2500, 5000, 8192)
ROUNDS = 3


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
    Wmax = WIDTHS[-1]
    ws = torch.empty(max(L.w2l_asg_beam_lex_xl_workspace_size(B, T, N, Wmax, K), L.w2l_ctc_beam_lex_xl_workspace_size(B, T, N, Wmax, K),
                         L.w2l_asg_beam_lex_wide_workspace_size(B, T, N, 1024, K)), dtype=torch.uint8, device="cuda")
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

    def call(search, sfx, W):
        if search == "ctc":
            return lambda: getattr(L, "w2l_ctc_beam_search" + sfx)(B, T, N, x.data_ptr(), None, W, K, inf, 0, 0, 1, T, *out4[:3],
                                                                   ws.data_ptr(), st)
        if search == "ctc_lm":
            return lambda: getattr(L, "w2l_ctc_beam_search_lm" + sfx)(B, T, N, x.data_ptr(), None, W, K, inf, 0, 0, 1, T, tc.data_ptr(),
                                                                      int(tok_lm_ctc.has_eos), 0.5, None, 0.0, *out4, ws.data_ptr(), st)
        if search == "ctc_lex":
            return lambda: getattr(L, "w2l_ctc_beam_search_lex" + sfx)(B, T, N, x.data_ptr(), None, W, K, inf, 0, 0, 1, T, wl.data_ptr(),
                                                                       int(word_lm.has_eos), 0.5, lc.data_ptr(), 0.5, 0.0, *out4, T,
                                                                       words.data_ptr(), counts.data_ptr(), ws.data_ptr(), st)
        if search == "asg":
            return lambda: getattr(L, "w2l_asg_beam_search" + sfx)(B, T, N, x.data_ptr(), None, A.data_ptr(), W, K, inf, 0, 0, 1, T,
                                                                   ta.data_ptr(), int(tok_lm_asg.has_eos), 0.5, None, 0.0, *out4,
                                                                   ws.data_ptr(), st)
        return lambda: getattr(L, "w2l_asg_beam_search_lex" + sfx)(B, T, N, x.data_ptr(), None, A.data_ptr(), W, K, inf, 0, 0, 1, T,
                                                                   wl.data_ptr(), int(word_lm.has_eos), 0.5, la.data_ptr(), 0.5, 0.0,
                                                                   *out4, T, words.data_ptr(), counts.data_ptr(), ws.data_ptr(), st)

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
        fns = {"wide1024": call(search, "_wide", 1024)}
        fns.update({f"xl{W}": call(search, "_xl", W) for W in WIDTHS})
        # the same hypothesis from both families at the width both take, before anything is timed
        _lib.check(fns["wide1024"](), "beam")
        torch.cuda.synchronize()
        ref = (labels.clone(), lengths.clone(), scores.clone())
        _lib.check(fns["xl1024"](), "beam")
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ref, (labels, lengths, scores)))
        t = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                t[k].append(timed(fn, reps))
        out = {"search": search, "B": B, "T": T, "N": N, "K": K, "xl1024_equals_wide1024": same}
        for k in fns:
            med = statistics.median(t[k])
            out[k] = {"us": round(med, 1), "us_runs": [round(v, 1) for v in t[k]], "spread": round((max(t[k]) - min(t[k])) / med, 3),
                      "us_per_frame": round(med / T, 2)}
        out["xl1024/wide1024"] = round(out["xl1024"]["us"] / out["wide1024"]["us"], 2)
        out["xl8192/xl1024"] = round(out["xl8192"]["us"] / out["xl1024"]["us"], 2)
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
