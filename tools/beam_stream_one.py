"""The incremental CTC beam search (w2l_beam_session_*) against the whole-utterance search of the same variant, in one process,
timed with hip events after warm-up at the TDS-CTC recipe's emission shape:   python tools/beam_stream_one.py [variant] [reps] [--wide]
  N = 9998, T = 188 emission frames per utterance, the max search on the raw emissions, no threshold, nbest = 1
  variant: lm (default; the 3-gram token LM of tools/ctc_beam_lm_one.py, lmWeight 0.5), lex (the lexicon and word LM of
  tools/ctc_beam_lex_one.py) or plain
  S = 1 / 16 / 64 slots, chunks of 1 / 2 / 4 emission frames per step, (W, K) = (64, 64) and (8, 8)
Per shape one JSON line: the median step latency (a step = every slot advanced by one chunk, timed step by step), microseconds per
frame summed over the utterance (all steps between two events), beside it the whole-utterance search at B = S, T = 188 -- the
yardstick -- per frame, their ratio, the constant a step adds ((session - whole) / steps), and what the session replaces: searching
again from frame 0 after every chunk, the sum of the whole search over the prefixes (timed at 8 prefix lengths, summed by the
trapezoid rule).  The session's final hypotheses are checked bit for bit against the whole search before anything is timed.
  --wide: the wide session (w2l_beam_session_create_wide) against the wide whole search (the w2l_*_wide entry points) at B = S in
  the same run: W = 128, 500 and 1024 with K = 64, S = 1 / 16 / 64, chunks of 1 and 4; then, at W = K = 64 where both families
  exist, the narrow session and the wide session side by side ("family"), each against its own whole search.
  --commit-every=K: w2l_beam_session_commit at one-frame steps, W = K = 64 narrow, W = 500 and 1024 wide, S = 1 / 16 /
  64.  First the exactness contract: a session that commits after every K-th step against one that never does, fed the same frames
  -- committed ++ tail == the uncommitted rows, scores the same bits, after every commit and at the end.  Then one JSON line per
  shape: the median one-frame step of the committing session, the median commit (the C call, host clock: it waits for the stream),
  per slot and as a multiple of the step, the nodes a commit leaves and the labels committed, and the utterance with commits
  against the utterance without in the same run (host clock, both synchronised at the end).
  --mt: the many-token session (w2l_beam_session_create_mt) against the many-token whole search (the w2l_*_mt entry
  points) at B = S in the same run: (W, K) = (500, 100) -- the streaming recipes' pair --, (500, 64) and (2500, 100), S = 1 / 16 /
  64, chunks of 1 and 4; then, at W = 500, K = 64 where both families exist, the wide session and the many-token session side by
  side ("family"), each against its own whole search, nothing routed.  With --commit-every=K: the commit leg at W = 500, K = 100 on
  the many-token session alone."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from ctc_beam_lm_one import HOT
from ctc_beam_lm_one import model as token_model
from wav2letter_amd import criterion
from wav2letter_amd.streaming import ManyTokenStreamingDecoder, StreamingDecoder, WideStreamingDecoder

T, N = 188, 9998


def tables(variant):
    if variant == "plain":
        return {}
    if variant == "lm":
        return dict(lm=token_model(N - 1, np.random.default_rng(3))[0], lm_weight=0.5)
    from ctc_beam_lex_one import smear_of, spellings, word_model
    from wav2letter_amd import Lexicon
    from ctc_beam_lex_one import WORDS
    rng = np.random.default_rng(3)
    rows, _ = spellings(N - 1, rng)
    lm, _ = word_model(WORDS, rng)
    return dict(lm=lm, lm_weight=0.5, word_score=-0.5, lexicon=Lexicon.from_spellings(rows, N - 1, WORDS, smear_of(lm), None))


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def family(wide, mt):
    """(name, session class, ctc_beam_search's wide=) of a kernel family"""
    if mt:
        return "mt", ManyTokenStreamingDecoder, "mt"
    return ("wide", WideStreamingDecoder, True) if wide else ("narrow", StreamingDecoder, False)


def bench(S, chunk, W, reps, opts, wide=False, K=None, mt=False):
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(S, T, N, generator=g)
    x[:, :, :HOT] += 2.0
    x = x.cuda()
    K = K or min(W, 64)
    fam, cls, whole_family = family(wide, mt)
    o = dict(beam=W, beam_token=K, threshold=float("inf"), log_add=False, normalize=False, **opts)
    dec = cls(S, chunk, T, N, **o)
    steps = [(x[:, t:t + chunk].contiguous() if t + chunk <= T else
              torch.cat([x[:, t:], torch.zeros(S, chunk - (T - t), N, device="cuda")], 1), min(chunk, T - t)) for t in range(0, T, chunk)]
    one = np.ones(S, np.int32)

    def utterance():
        for i, (em, c) in enumerate(steps):
            dec.step(em, one * c, one * (i == 0))

    def whole(F=T):
        return criterion.ctc_beam_search(x[:, :F].contiguous() if F < T else x, nbest=1, max_len=T, wide=whole_family, **o)

    utterance()
    got, want = dec.result(nbest=1, max_len=T), whole()
    torch.cuda.synchronize()
    assert all((a.cpu().numpy().view(np.int32) == b.cpu().numpy().view(np.int32)).all() for a, b in zip(got, want)), \
        "the session's hypotheses are not the whole search's"
    for _ in range(2):
        utterance()
    t_utt = min(events(utterance, reps) for _ in range(2))
    lat = []
    for _ in range(max(reps // 2, 1)):   # step by step: the latency a caller sees between a chunk's emissions and the beam
        for i, (em, c) in enumerate(steps):
            lat.append(events(lambda: dec.step(em, one * c, one * (i == 0)), 1))
    res = min(events(lambda: dec.result(nbest=1, max_len=T), reps) for _ in range(2))
    t_whole = min(events(whole, reps) for _ in range(2))
    marks = sorted({max(1, round(T * k / 8)) for k in range(1, 9)})
    tp = [min(events(lambda: whole(F), max(reps // 2, 1)) for _ in range(2)) for F in marks]
    # the sum over the prefixes a chunked caller would search again, by the trapezoid rule over the timed lengths
    ends = list(range(chunk, T, chunk)) + [T]
    research = float(np.interp(ends, marks, tp).sum())
    return {"family": fam, "S": S, "chunk": chunk, "W": W, "K": K, "steps": len(steps), "step_us_median": round(statistics.median(lat), 1),
            "session_us_per_utterance": round(t_utt, 1), "session_us_per_frame": round(t_utt / T, 2), "result_us": round(res, 1),
            "whole_us": round(t_whole, 1), "whole_us_per_frame": round(t_whole / T, 2), "ratio": round(t_utt / t_whole, 2),
            "per_step_constant_us": round((t_utt - t_whole) / len(steps), 1), "research_from_zero_us": round(research, 1),
            "research_over_session": round(research / t_utt, 1)}


def bench_commit(S, W, every, reps, opts, wide, K=None, mt=False):
    from wav2letter_amd import _lib
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(S, T, N, generator=g)
    x[:, :, :HOT] += 2.0
    x = x.cuda()
    K = K or min(W, 64)
    fam, cls, _ = family(wide, mt)
    o = dict(beam=W, beam_token=K, threshold=float("inf"), log_add=False, normalize=False, **opts)
    a, b = cls(S, 1, T, N, **o), cls(S, 1, T, N, **o)
    steps = [x[:, t:t + 1].contiguous() for t in range(T)]
    one = np.ones(S, np.int32)

    def rows(dec, full):
        return [t.cpu().numpy() for t in dec.result(nbest=1, max_len=T, full=full)]

    def check(what):
        ra, rb = rows(a, False), rows(b, True)
        assert (rb[0][:, :, :T] == ra[0]).all() and (rb[0][:, :, T:] == -1).all() and (rb[1] == ra[1]).all(), what
        assert all((p.view(np.int32) == q.view(np.int32)).all() for p, q in zip(ra[2:4], rb[2:4])), what

    # the exactness contract first
    for i, em in enumerate(steps):
        a.step(em, one, one * (i == 0))
        b.step(em, one, one * (i == 0))
        if i % every == every - 1:
            b.commit()
            check(("commit after step", i))
    check("end")
    done = [len(b.committed(s)[0]) for s in range(S)]

    # then the clock: the C call, with buffers made once
    scratch = torch.empty(L.w2l_beam_session_commit_bytes(b.h), dtype=torch.uint8, device="cuda")
    labels = torch.empty(S, T, dtype=torch.int32, device="cuda")
    words = torch.empty(S, T, dtype=torch.int32, device="cuda")
    nl, nw, live = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    commits, lives = [], []

    def commit(dec, timed):
        if timed:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = L.w2l_beam_session_commit(dec.h, None, scratch.data_ptr(), scratch.numel(), T, labels.data_ptr(), T, words.data_ptr(),
                                       nl.ctypes.data, nw.ctypes.data, live.ctypes.data, stream)
        assert st == 0, L.w2l_host_last_error().decode()
        if timed:
            commits.append((time.perf_counter() - t0) * 1e6)
            lives.append(float(live.mean()))

    def utterance(dec, k, timed=False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, em in enumerate(steps):
            dec.step(em, one, one * (i == 0))
            if k and i % k == k - 1:
                commit(dec, timed)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for k in (0, every):
        utterance(b, k)
    t_plain = min(utterance(b, 0) for _ in range(reps))
    t_commit = min(utterance(b, every) for _ in range(reps))
    utterance(b, every, timed=True)
    lat = []
    for i, em in enumerate(steps):   # one-frame steps of a session that commits, timed one by one
        lat.append(events(lambda: b.step(em, one, one * (i == 0)), 1))
        if i % every == every - 1:
            commit(b, False)
    step, com = statistics.median(lat), statistics.median(commits)
    return {"family": fam, "S": S, "W": W, "K": K, "commit_every": every, "scratch_bytes": scratch.numel(),
            "step_us_median": round(step, 1), "commit_us_median": round(com, 1), "commit_us_max": round(max(commits), 1),
            "commit_us_per_slot": round(com / S, 1), "commit_over_step": round(com / step, 2),
            "live_nodes_mean": round(statistics.mean(lives), 1), "labels_committed_mean": round(statistics.mean(done), 1),
            "utterance_us": round(t_plain, 1), "utterance_with_commits_us": round(t_commit, 1),
            "added_percent": round(100 * (t_commit - t_plain) / t_plain, 1)}


if __name__ == "__main__":
    every = [int(a.split("=", 1)[1]) for a in sys.argv[1:] if a.startswith("--commit-every=")]
    mt = "--mt" in sys.argv[1:]
    if mt:
        args = [a for a in sys.argv[1:] if not a.startswith("--")]
        variant = args[0] if len(args) > 0 else "lm"
        reps = int(args[1]) if len(args) > 1 else 3
        opts = tables(variant)
        print(json.dumps({"variant": variant, "T": T, "N": N, "reps": reps, "mt": True, "commit_every": every[0] if every else None}), flush=True)
        if every:
            for S in (1, 16, 64):
                print(json.dumps(bench_commit(S, 500, every[0], reps, opts, False, K=100, mt=True)), flush=True)
            sys.exit(0)
        for W, K in ((500, 100), (500, 64), (2500, 100)):
            for S in (1, 16, 64):
                for chunk in (1, 4):
                    print(json.dumps(bench(S, chunk, W, reps, opts, K=K, mt=True)), flush=True)
        for S in (1, 16, 64):
            for chunk in (1, 4):
                print(json.dumps(bench(S, chunk, 500, reps, opts, wide=True)), flush=True)   # the mt lines at (500, 64) are above
        sys.exit(0)
    if every:
        args = [a for a in sys.argv[1:] if not a.startswith("--")]
        variant = args[0] if len(args) > 0 else "lm"
        reps = int(args[1]) if len(args) > 1 else 3
        opts = tables(variant)
        print(json.dumps({"variant": variant, "T": T, "N": N, "reps": reps, "commit_every": every[0]}), flush=True)
        for W, fam in ((64, False), (500, True), (1024, True)):
            for S in (1, 16, 64):
                print(json.dumps(bench_commit(S, W, every[0], reps, opts, fam)), flush=True)
        sys.exit(0)
    args = [a for a in sys.argv[1:] if a != "--wide"]
    wide = "--wide" in sys.argv[1:]
    variant = args[0] if len(args) > 0 else "lm"
    reps = int(args[1]) if len(args) > 1 else 6
    opts = tables(variant)
    print(json.dumps({"variant": variant, "T": T, "N": N, "reps": reps, "wide": wide}), flush=True)
    if wide:
        for W in (128, 500, 1024):
            for S in (1, 16, 64):
                for chunk in (1, 4):
                    print(json.dumps(bench(S, chunk, W, reps, opts, wide=True)), flush=True)
        for S in (1, 16, 64):
            for chunk in (1, 4):
                for fam in (False, True):
                    print(json.dumps(bench(S, chunk, 64, reps, opts, wide=fam)), flush=True)
        sys.exit(0)
    for W in (64, 8):
        for S in (1, 16, 64):
            for chunk in (1, 2, 4):
                print(json.dumps(bench(S, chunk, W, reps, opts)), flush=True)
