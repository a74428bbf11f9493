"""The lexicon searches with a token LM (w2l_*_beam_search_lextok) against their two siblings -- the token-LM search and the
word-LM lexicon search -- on the same emissions in the same process, timed with hip events after warm-up:
    python tools/beam_lextok_one.py [reps] [pieces|letters|ab] [K ...]
  pieces   B = 32, N = 9998, T = 188, K = 64 and 8 (or the K given): CTC and ASG
  letters  B = 64, N = 30, T = 1000, K = 30 and 8: ASG
  ab       the UNCHANGED lexicon searches alone (w2l_ctc_beam_search_lex / w2l_asg_beam_search_lex, narrow and wide, pieces at K = 8
           and letters at K = 30), from the library W2L_AB_LIB names (default: the package's): run it alternately with the parent
           commit's library and this one's; the symbols are resolved one by one, so a library without the new entry points loads
Each search runs narrow at W = 64 and wide at W = 1000.  Max search on the raw emissions, no threshold, nbest = 1; the models are
tools/asg_beam_one.py's (the token LM under the lexicon is the token-LM search's model, the lexicon the word search's).  A run is
one warm-up call and `reps` timed calls between two events; the runs of a (lattice, family) are interleaved and repeated three
times.  Prints one JSON line per (shape, K, lattice): the median microseconds per frame of the three searches in each family and
the spread of the runs ((max - min) / median).  The new search does one LM lookup per (entry, token) pair and none in selection; the
word search up to six per pair and more in selection; the token-LM search one per pair and no lexicon lookups."""
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

FAMILIES = (("narrow", 0, "", 64), ("wide", 1, "_wide", 1000))
ROUNDS = 3


def library(names):
    """the package's library; with W2L_AB_LIB that file, of which only `names` are resolved (an older build has no newer ones); the
    models and lexicons are still built by the package's"""
    path = os.environ.get("W2L_AB_LIB")
    if not path:
        return _lib.lib()
    L = C.CDLL(path)
    for name in names:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = getattr(_lib._SIGS, name)
    return L


def bench(B, T, N, K, hot, reps, lattices, searches, tok_lm_asg, tok_lm_ctc, lex_asg, lex_ctc, word_lm):
    stems = ["w2l_ctc_beam_search_lex", "w2l_asg_beam_search_lex", "w2l_ctc_beam_lex_workspace_size", "w2l_asg_beam_lex_workspace_size"]
    names = [s + sfx if "workspace" not in s else s.replace("_workspace_size", sfx + "_workspace_size") for s in stems for _, _, sfx, _ in FAMILIES]
    L = library(names)
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(B, T, N, generator=g)
    x[:, :, :hot] += 2.0
    x = x.cuda()
    A = torch.zeros(N, N)
    A[:hot, :hot] = torch.randn(hot, hot, generator=g)
    A += 2.0 * torch.eye(N)
    A = A.cuda()
    ws = torch.empty(max(L.w2l_asg_beam_lex_wide_workspace_size(B, T, N, 1000, K), L.w2l_ctc_beam_lex_wide_workspace_size(B, T, N, 1000, K),
                         L.w2l_asg_beam_lex_workspace_size(B, T, N, 64, K)), dtype=torch.uint8, device="cuda")
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
    lex_out = (*out4, T, words.data_ptr(), counts.data_ptr(), ws.data_ptr(), st)

    def call(lattice, search, family, sfx, W):
        asg = lattice == "asg"
        head = (B, T, N, x.data_ptr(), None) + ((A.data_ptr(),) if asg else ()) + (W, K, inf, 0, 0, 1, T)
        tok, tlm = (ta, tok_lm_asg) if asg else (tc, tok_lm_ctc)
        lex = la if asg else lc
        if search == "token_lm":
            f = getattr(L, ("w2l_asg_beam_search" if asg else "w2l_ctc_beam_search_lm") + sfx)
            return lambda: f(*head, tok.data_ptr(), int(tlm.has_eos), 0.5, None, 0.0, *out4, ws.data_ptr(), st)
        if search == "word_lex":
            f = getattr(L, ("w2l_asg_beam_search_lex" if asg else "w2l_ctc_beam_search_lex") + sfx)
            return lambda: f(*head, wl.data_ptr(), int(word_lm.has_eos), 0.5, lex.data_ptr(), 0.5, 0.0, *lex_out)
        f = L.w2l_asg_beam_search_lextok if asg else L.w2l_ctc_beam_search_lextok
        return lambda: f(family, *head, tok.data_ptr(), int(tlm.has_eos), 0.5, lex.data_ptr(), 0.5, 0.0, *lex_out, -1, 0.0)

    def timed(fn, n):
        _lib.check(fn(), "beam")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    for lattice in lattices:
        out = {"lattice": lattice, "B": B, "T": T, "N": N, "K": K}
        for name, family, sfx, W in FAMILIES:
            fns = {s: call(lattice, s, family, sfx, W) for s in searches}
            t = {k: [] for k in fns}
            for _ in range(ROUNDS):
                for k, fn in fns.items():
                    t[k].append(timed(fn, reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            out[f"{name}{W}"] = dict({f"{k}_us_per_frame": round(med[k] / T, 2) for k in fns},
                                     spread=round(max((max(v) - min(v)) / med[k] for k, v in t.items()), 3))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    which = sys.argv[2] if len(sys.argv) > 2 else "pieces"
    ks = [int(v) for v in sys.argv[3:]]
    three = ("token_lm", "word_lex", "lextok")
    if which in ("pieces", "ab"):
        s = setup(9998, 2048, 4)
        # one emission tensor for both criteria: the CTC searches take its last column as their blank (setup's CTC models are over
        # the 9997 classes before it)
        for K in ks or ((8,) if which == "ab" else (64, 8)):
            bench(32, 188, 9998, K, 2048, reps, ("ctc", "asg"), ("word_lex",) if which == "ab" else three, **s)
    if which in ("letters", "ab"):
        s = setup(30, 28, 3)
        for K in ks or ((30,) if which == "ab" else (30, 8)):
            bench(64, 1000, 30, K, 28, reps, ("asg",), ("word_lex",) if which == "ab" else three, **s)
