"""Entry points that existed before the many-token beam session, timed from TWO builds of the library in one process, in
alternating runs, twice each (the method of tools/beam_mt_one.py's parent mode):
    python tools/beam_stream_mt_ab.py <libw2l_hip.so of the parent commit> [reps]
  w2l_ctc_beam_search_lex_mt   B = 32, W = 500, K = 100
  w2l_ctc_beam_search_lex_xl   B = 32, W = 500, K = 64
  the wide session's step      w2l_beam_session_create_wide / bind / step, lexicon variant, S = 16, W = 500, K = 64, one frame a step
N = 9998, T = 188, max search on the raw emissions, no threshold; the models are tools/asg_beam_one.py's.  One JSON line per entry:
the four runs in microseconds (per call; the session: per step), the ratio of the means and the spread of the parent's two runs,
which is the bar the new library's mean has to fall inside."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from asg_beam_one import setup
from wav2letter_amd import _lib

B, S, T, N, HOT = 32, 16, 188, 9998, 2048
NAMES = ("w2l_ctc_beam_search_lex_mt", "w2l_ctc_beam_search_lex_xl", "w2l_beam_session_create_wide", "w2l_beam_session_wide_state_bytes",
         "w2l_beam_session_bind", "w2l_beam_session_step", "w2l_beam_session_destroy")


def other_lib(path):
    P = C.CDLL(path)
    for name in NAMES:
        f = getattr(P, name)
        f.restype, f.argtypes = getattr(_lib._SIGS, name)
    return P


def main(parent, reps):
    libs = {"parent": other_lib(parent), "new": _lib.lib()}
    s = setup(N, HOT, 4)
    lex, word_lm = s["lex_ctc"], s["word_lm"]
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(B, T, N, generator=g)
    x[:, :, :HOT] += 2.0
    x = x.cuda()
    L = libs["new"]
    ws = torch.empty(L.w2l_ctc_beam_lex_mt_workspace_size(B, T, N, 500, 100), dtype=torch.uint8, device="cuda")
    labels = torch.empty(B, 1, T, dtype=torch.int32, device="cuda")
    lengths = torch.empty(B, 1, dtype=torch.int32, device="cuda")
    scores, lms = torch.empty(B, 1, device="cuda"), torch.empty(B, 1, device="cuda")
    words = torch.empty(B, 1, T, dtype=torch.int32, device="cuda")
    counts = torch.empty(B, 1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    wl, lc = word_lm.device_blob("cuda"), lex.device_blob("cuda")
    inf = float("inf")

    def whole(lib, name, K, tail):
        f = getattr(lib, name)
        return lambda: f(B, T, N, x.data_ptr(), None, 500, K, inf, 0, 0, 1, T, wl.data_ptr(), int(word_lm.has_eos), 0.5, lc.data_ptr(), 0.5, 0.0,
                         labels.data_ptr(), lengths.data_ptr(), scores.data_ptr(), lms.data_ptr(), T, words.data_ptr(), counts.data_ptr(),
                         ws.data_ptr(), st, *tail)

    def session(lib):
        d = _lib.BeamSessionDesc(slots=S, maxChunk=1, maxFrames=T, N=N, beam=500, beamToken=64, threshold=inf, logAdd=0, normalize=0, variant=2,
                                 lm=wl.data_ptr(), lmHasEos=int(word_lm.has_eos), lmWeight=0.5, classScore=None, eosScore=0.0,
                                 lexicon=lc.data_ptr(), wordScore=0.5)
        h = C.c_void_p(0)
        _lib.check(lib.w2l_beam_session_create_wide(C.byref(d), C.byref(h)), "create")
        state = torch.empty(lib.w2l_beam_session_wide_state_bytes(C.byref(d)), dtype=torch.uint8, device="cuda")
        _lib.check(lib.w2l_beam_session_bind(h, state.data_ptr(), state.numel()), "bind")
        frames = [x[:S, t:t + 1].contiguous() for t in range(T)]
        one, first = np.ones(S, np.int32), np.zeros(S, np.int32)

        def utterance():   # T steps; the figure below is per step
            rc = 0
            for t, em in enumerate(frames):
                first[:] = t == 0
                rc |= lib.w2l_beam_session_step(h, em.data_ptr(), one.ctypes.data, first.ctypes.data, st)
            return rc
        utterance.keep = (state, frames, h)
        return utterance

    def timed(fn, n):
        _lib.check(fn(), "beam")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    entries = [("w2l_ctc_beam_search_lex_mt W=500 K=100", {k: whole(v, "w2l_ctc_beam_search_lex_mt", 100, (-1, 0.0)) for k, v in libs.items()}, 1),
               ("w2l_ctc_beam_search_lex_xl W=500 K=64", {k: whole(v, "w2l_ctc_beam_search_lex_xl", 64, ()) for k, v in libs.items()}, 1),
               ("wide session step, lexicon, S=16 W=500 K=64", {k: session(v) for k, v in libs.items()}, T)]
    for what, fns, per in entries:
        runs = {"parent": [], "new": []}
        for _ in range(2):
            for k in ("parent", "new"):
                runs[k].append(timed(fns[k], reps) / per)
        mp, mn = statistics.mean(runs["parent"]), statistics.mean(runs["new"])
        print(json.dumps({"entry": what, "parent_us": [round(v, 1) for v in runs["parent"]], "new_us": [round(v, 1) for v in runs["new"]],
                          "new/parent": round(mn / mp, 4), "parent_spread": round((max(runs["parent"]) - min(runs["parent"])) / mp, 4)}),
              flush=True)
    for _, fns, _ in entries[2:]:
        for k, fn in fns.items():
            libs[k].w2l_beam_session_destroy(fn.keep[2])


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 2)
