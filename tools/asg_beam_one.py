"""Each ASG beam search against its CTC sibling on the same emissions in the same process, timed with hip events after warm-up:
    python tools/asg_beam_one.py [reps] [letters|pieces]
  letters   B = 64, N = 30 (the sibling: N = 31, a blank column appended), T = 1000 and 2000, W = K = 30 and 8: the config-4
            criterion shape; the 30 x 30 transition matrix is staged in LDS
  pieces    B = 32, N = 9998 (the sibling: the same 9998 columns, the last one its blank), T = 188, W = K = 64 and 8: the matrix
            (400 MB) is gathered from global memory
Pairs: `asg_plain` (lm = NULL) with `ctc_plain` (w2l_ctc_beam_search: the one-wavefront lazy scan, which ASG cannot use) and with
`ctc_lm`; `asg_lm` with `ctc_lm`; `asg_lex` with `ctc_lex`.  Max search on the raw emissions, no threshold, nbest = 1, random
transitions N(0, 1) + 2 on the diagonal, a random 3-gram token model, a synthetic lexicon of 20000 words of 1 to 4 of the favoured
tokens (spellings without a doubled token, so that both searches can reach every word) and a random 3-gram word model.
The runs are interleaved and repeated twice (a drift of the box shows as a spread between the two runs of one).  The LDS-vs-global
A/B of the transition matrix runs at N = 90, the largest matrix that is staged (32400 bytes), through libw2l_hip_probe.so with and
without W2L_ASG_BEAM_TRANS=global.  Prints microseconds per call, one JSON line per shape, with the ASG / CTC ratios."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wav2letter_amd import Lexicon, NGramLM, _lib

WORDS = 20000


def _vals(rng, n, lo, hi):
    return rng.uniform(lo, hi, n).astype(np.float32)


def ngram_model(V, hot, rng, pairs=20000, triples=20000, listed=None):
    listed = V if listed is None else min(listed, V)
    uni = np.concatenate([np.arange(listed, dtype=np.int32), np.array([V, V + 1], np.int32)]).reshape(-1, 1)
    two = np.unique(rng.integers(0, hot, size=(pairs, 2)).astype(np.int32), axis=0)
    ctx = two[rng.integers(0, len(two), size=triples)]
    three = np.unique(np.concatenate([ctx, rng.integers(0, hot, size=(triples, 1)).astype(np.int32)], axis=1), axis=0)
    return NGramLM.from_ngrams([(uni, _vals(rng, len(uni), -9, -5), _vals(rng, len(uni), -1, 0)),
                                (two, _vals(rng, len(two), -4, -1), _vals(rng, len(two), -1, 0)),
                                (three, _vals(rng, len(three), -3, -0.5), None)], V, -12.0)


def spellings(hot, rng, words=WORDS):
    """rows (word, tokens): distinct spellings of 1..4 favoured tokens, no token twice in a row"""
    rows, seen = [], set()
    while len(rows) < words:
        sp = tuple(int(t) for t in rng.integers(0, hot, int(rng.integers(1, 5))))
        if any(a == b for a, b in zip(sp, sp[1:])) or sp in seen:
            continue
        seen.add(sp)
        rows.append((len(rows), list(sp)))
    return rows


def bench(B, T, N, W, K, hot, reps, tok_lm_asg, tok_lm_ctc, lex_asg, lex_ctc, word_lm, only=None):
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(B, T, N, generator=g)
    x[:, :, :hot] += 2.0
    if N <= 100:   # the sibling's blank column; at N = 9998 the sibling reads the same tensor, its last column as blank
        xc = torch.cat([x, torch.randn(B, T, 1, generator=g) + 2.0], dim=2).cuda()
    x = x.cuda()
    if N > 100:
        xc = x
    Nc = xc.shape[2]
    A = torch.randn(N, N, generator=g) if N <= 100 else torch.zeros(N, N)
    if N > 100:
        A[:hot, :hot] = torch.randn(hot, hot, generator=g)
    A += 2.0 * torch.eye(N)
    A = A.cuda()
    sizes = [L.w2l_asg_beam_workspace_size(B, T, N, W, K), L.w2l_asg_beam_lex_workspace_size(B, T, N, W, K),
             L.w2l_ctc_beam_lex_workspace_size(B, T, Nc, W, K)]
    ws = torch.empty(max(sizes), dtype=torch.uint8, device="cuda")
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
    fns = {
        "asg_plain": lambda: L.w2l_asg_beam_search(B, T, N, x.data_ptr(), None, A.data_ptr(), W, K, inf, 0, 0, 1, T, None, 0, 0.0, None,
                                                   0.0, *out4, ws.data_ptr(), st),
        "ctc_plain": lambda: L.w2l_ctc_beam_search(B, T, Nc, xc.data_ptr(), None, W, K, inf, 0, 0, 1, T, *out4[:3], ws.data_ptr(), st),
        "asg_lm": lambda: L.w2l_asg_beam_search(B, T, N, x.data_ptr(), None, A.data_ptr(), W, K, inf, 0, 0, 1, T, ta.data_ptr(),
                                                int(tok_lm_asg.has_eos), 0.5, None, 0.0, *out4, ws.data_ptr(), st),
        "ctc_lm": lambda: L.w2l_ctc_beam_search_lm(B, T, Nc, xc.data_ptr(), None, W, K, inf, 0, 0, 1, T, tc.data_ptr(),
                                                   int(tok_lm_ctc.has_eos), 0.5, None, 0.0, *out4, ws.data_ptr(), st),
        "asg_lex": lambda: L.w2l_asg_beam_search_lex(B, T, N, x.data_ptr(), None, A.data_ptr(), W, K, inf, 0, 0, 1, T, wl.data_ptr(),
                                                     int(word_lm.has_eos), 0.5, la.data_ptr(), 0.5, 0.0, *out4, T, words.data_ptr(),
                                                     counts.data_ptr(), ws.data_ptr(), st),
        "ctc_lex": lambda: L.w2l_ctc_beam_search_lex(B, T, Nc, xc.data_ptr(), None, W, K, inf, 0, 0, 1, T, wl.data_ptr(),
                                                     int(word_lm.has_eos), 0.5, lc.data_ptr(), 0.5, 0.0, *out4, T, words.data_ptr(),
                                                     counts.data_ptr(), ws.data_ptr(), st),
    }
    if only:
        fns = {k: fns[k] for k in only}

    def timed(fn, n):
        for _ in range(2):
            _lib.check(fn(), "beam")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    t = {k: [] for k in fns}
    for _ in range(2):
        for k, fn in fns.items():
            t[k].append(timed(fn, reps))
    out = {"B": B, "T": T, "N": N, "W": W, "K": K}
    for k in fns:
        out[k] = {"us": round(min(t[k]), 1), "us_runs": [round(v, 1) for v in t[k]], "us_per_frame": round(min(t[k]) / T, 2)}
    for a, c in (("asg_plain", "ctc_plain"), ("asg_plain", "ctc_lm"), ("asg_lm", "ctc_lm"), ("asg_lex", "ctc_lex")):
        if a in out and c in out:
            out[f"{a}/{c}"] = round(out[a]["us"] / out[c]["us"], 2)
    return out


def setup(N, hot, seed):
    rng = np.random.default_rng(seed)
    rows = spellings(hot, rng)
    word_lm = ngram_model(WORDS, 4096, rng, listed=20000)
    smear = np.array([word_lm.score(word_lm.start, w)[0] for w in range(WORDS)], np.float32)
    ctc_tokens = N if N <= 100 else N - 1           # the sibling's token classes: all of ours, or ours without its blank column
    return dict(tok_lm_asg=ngram_model(N, hot, rng), tok_lm_ctc=ngram_model(ctc_tokens, hot, rng),
                lex_asg=Lexicon.from_spellings(rows, N, WORDS, smear), lex_ctc=Lexicon.from_spellings(rows, ctc_tokens, WORDS, smear),
                word_lm=word_lm)


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    which = sys.argv[2] if len(sys.argv) > 2 else "all"
    if which in ("all", "letters"):
        s = setup(30, 28, 3)
        for T in (1000, 2000):
            for W in (30, 8):
                print(json.dumps(bench(64, T, 30, W, W, 28, reps, **s)), flush=True)
    if which in ("all", "pieces"):
        s = setup(9998, 2048, 4)
        for W in (64, 8):
            print(json.dumps(bench(32, 188, 9998, W, W, 2048, reps, **s)), flush=True)
    if which in ("all", "ab"):
        s = setup(90, 28, 5)
        with _lib.use_probe():
            for home in ("lds", "global"):
                os.environ["W2L_ASG_BEAM_TRANS"] = home
                for W in (64, 8):
                    r = bench(64, 1000, 90, W, W, 28, reps, only=("asg_plain", "asg_lm", "asg_lex"), **s)
                    r["transitions"] = home
                    print(json.dumps(r), flush=True)
        os.environ.pop("W2L_ASG_BEAM_TRANS", None)
