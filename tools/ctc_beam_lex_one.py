"""w2l_ctc_beam_search_lex against w2l_ctc_beam_search_lm on the same emissions in the same process, timed with hip events after
warm-up at the criterion shapes of the TDS-CTC recipe:   python tools/ctc_beam_lex_one.py [reps] [T] [W]
  B = 32, T = 188 and 1500, N = 9998, (W, K) = (64, 64) and (8, 8), max search on the raw emissions, no threshold, nbest = 1
The lexicon is synthetic: about 2 * 10^5 words over the 9997 pieces, spellings of 1 to 4 pieces drawn from the 2048 pieces the
emissions favour (+2 on those classes), about 1 % of the words sharing the spelling of an earlier word (homophones).  The word LM
is a random 3-gram model of about 10^5 n-grams: the unigrams of the first 20000 words, BOS and EOS (the other words score as
<unk>), and 40000 bigrams and 40000 trigrams over the first 4096 words.  lmWeight = 0.5, wordScore = 0.5, max smearing.  The
token-LM search runs with the 3-gram TOKEN model of tools/ctc_beam_lm_one.py: the yardstick this kernel is reported against.
A/B for where the added time goes, the same call with
  `lex_no_smear`   the lexicon built with wordSmear = NULL (the same trie, smear 0 everywhere: the search keeps other hypotheses,
                   the work per candidate is the same);
  `lex_unigram`    a unigram-only word LM (every word candidate one probe chain from state 0, no back-off walk).
Prints microseconds per call, one JSON line per shape, with the ratio to the token-LM search and the differences per frame."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ctc_beam_lm_one import HOT
from ctc_beam_lm_one import model as token_model
from wav2letter_amd import Lexicon, NGramLM, _lib

WORDS, HOT_WORDS = 200000, 4096


def spellings(V, rng, words=WORDS, homophones=0.01):
    """rows (word, pieces): distinct spellings of 1..4 favoured pieces; a homophone copies the spelling of an earlier word"""
    lens = rng.integers(1, 5, words)
    toks = rng.integers(0, HOT, size=(words, 4))
    rows, seen, shared = [], set(), 0
    for w in range(words):
        if w and rng.random() < homophones:
            rows.append((w, rows[int(rng.integers(w))][1]))
            shared += 1
            continue
        sp = tuple(int(t) for t in toks[w, :lens[w]])
        while sp in seen:
            sp = sp + (int(rng.integers(HOT)),)
        seen.add(sp)
        rows.append((w, list(sp)))
    return rows, shared


def word_model(V, rng, listed=20000, pairs=40000, triples=40000, order=3):
    uni = np.concatenate([np.arange(listed, dtype=np.int32), np.array([V, V + 1], np.int32)]).reshape(-1, 1)

    def vals(n, lo, hi):
        return rng.uniform(lo, hi, n).astype(np.float32)
    if order == 1:
        return NGramLM.from_ngrams([(uni, vals(len(uni), -12, -5), None)], V, -14.0), len(uni)
    two = np.unique(rng.integers(0, HOT_WORDS, size=(pairs, 2)).astype(np.int32), axis=0)
    ctx = two[rng.integers(0, len(two), size=triples)]
    three = np.unique(np.concatenate([ctx, rng.integers(0, HOT_WORDS, size=(triples, 1)).astype(np.int32)], axis=1), axis=0)
    lm = NGramLM.from_ngrams([(uni, vals(len(uni), -12, -5), vals(len(uni), -1, 0)), (two, vals(len(two), -4, -1), vals(len(two), -1, 0)),
                              (three, vals(len(three), -3, -0.5), None)], V, -14.0)
    return lm, len(uni) + len(two) + len(three)


def smear_of(lm):
    return np.array([lm.score(lm.start, w)[0] for w in range(lm.num_tokens)], np.float32)


def bench(T, W, K, reps, tok_lm, variants, B=32, N=9998):
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(B, T, N, generator=g)
    x[:, :, :HOT] += 2.0
    x = x.cuda()
    wsl = torch.empty(L.w2l_ctc_beam_lm_workspace_size(B, T, N, W, K), dtype=torch.uint8, device="cuda")
    wsx = torch.empty(L.w2l_ctc_beam_lex_workspace_size(B, T, N, W, K), dtype=torch.uint8, device="cuda")
    labels = torch.empty(B, 1, T, dtype=torch.int32, device="cuda")
    lengths = torch.empty(B, 1, dtype=torch.int32, device="cuda")
    scores = torch.empty(B, 1, device="cuda")
    lms = torch.empty(B, 1, device="cuda")
    words = torch.empty(B, 1, T, dtype=torch.int32, device="cuda")
    counts = torch.empty(B, 1, dtype=torch.int32, device="cuda")
    tok_blob = tok_lm.device_blob("cuda")
    st = torch.cuda.current_stream().cuda_stream

    def token_lm():
        _lib.check(L.w2l_ctc_beam_search_lm(B, T, N, x.data_ptr(), None, W, K, float("inf"), 0, 0, 1, T, tok_blob.data_ptr(),
                                            int(tok_lm.has_eos), 0.5, None, 0.0, labels.data_ptr(), lengths.data_ptr(),
                                            scores.data_ptr(), lms.data_ptr(), wsl.data_ptr(), st), "beam lm")

    def lex_call(lex, lm):
        lb, mb = lex.device_blob("cuda"), lm.device_blob("cuda")

        def fn():
            _lib.check(L.w2l_ctc_beam_search_lex(B, T, N, x.data_ptr(), None, W, K, float("inf"), 0, 0, 1, T, mb.data_ptr(),
                                                 int(lm.has_eos), 0.5, lb.data_ptr(), 0.5, 0.0, labels.data_ptr(), lengths.data_ptr(),
                                                 scores.data_ptr(), lms.data_ptr(), T, words.data_ptr(), counts.data_ptr(),
                                                 wsx.data_ptr(), st), "beam lex")
        return fn

    def timed(fn, n):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    fns = {"beam_lm_max": token_lm}
    fns.update({k: lex_call(lex, lm) for k, (lex, lm) in variants.items()})
    t = {k: [] for k in fns}
    for _ in range(2):   # alternate, twice each: a drift of the box shows as a spread between the two runs of one
        for k, fn in fns.items():
            t[k].append(timed(fn, reps))
    fns["lex"]()
    torch.cuda.synchronize()
    out = {"B": B, "T": T, "N": N, "W": W, "K": K, "utterances_with_a_hypothesis": int((counts.cpu() >= 0).sum()),
           "mean_words": float(counts.cpu().clamp(min=0).float().mean())}
    for k in fns:
        out[k] = {"us": round(min(t[k]), 1), "us_runs": [round(v, 1) for v in t[k]]}
    out["ratio_to_token_lm"] = round(out["lex"]["us"] / out["beam_lm_max"]["us"], 2)
    out["extra_us_per_frame"] = round((out["lex"]["us"] - out["beam_lm_max"]["us"]) / T, 2)
    out["smearing_us_per_frame"] = round((out["lex"]["us"] - out["lex_no_smear"]["us"]) / T, 2)
    out["longer_lookups_us_per_frame"] = round((out["lex"]["us"] - out["lex_unigram"]["us"]) / T, 2)
    return out


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    V = 9997
    tok_lm, _ = token_model(V, np.random.default_rng(3))
    rows, shared = spellings(V, np.random.default_rng(5))
    lm, count = word_model(WORDS, np.random.default_rng(6))
    lm1, _ = word_model(WORDS, np.random.default_rng(7), order=1)
    lex = Lexicon.from_spellings(rows, V, WORDS, smear_of(lm))
    variants = {"lex": (lex, lm), "lex_no_smear": (Lexicon.from_spellings(rows, V, WORDS), lm),
                "lex_unigram": (Lexicon.from_spellings(rows, V, WORDS, smear_of(lm1)), lm1)}
    print(json.dumps({"words": WORDS, "homophones": shared, "lexicon_nodes": lex.num_nodes, "lexicon_dropped": lex.dropped,
                      "lexicon_blob_bytes": int(lex.blob.nbytes), "lm_order": lm.order, "ngrams": count, "states": lm.num_states,
                      "lm_blob_bytes": int(lm.blob.nbytes)}), flush=True)
    for T in ([int(sys.argv[2])] if len(sys.argv) > 2 else (188, 1500)):
        for W in ([int(sys.argv[3])] if len(sys.argv) > 3 else (64, 8)):
            print(json.dumps(bench(T, W, W, reps, tok_lm, variants)), flush=True)
