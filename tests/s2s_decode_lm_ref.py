"""float64 restatement of the LM-fused seq2seq decoder's contract: tests/s2s_decode_ref.py's search with the LM terms,
the LM being the textbook back-off scorer of tests/ctc_beam_lm_ref.py on word tuples (the LM state of a hypothesis is its tokens)."""
import functools

import numpy as np
import torch

import s2s_decode_ref as D
from tests.ctc_beam_lm_ref import random_lm


def search(p, enc, kl, keyvalue, eos, lm, lm_weight, beam, beam_token, max_len, nbest, threshold=None, eos_score=0.0, attention_threshold=None):
    """-> (per utterance the best nbest (tokens, score, lm score), the smallest score margin of any decision, the smallest attention
    margin, how many candidates the beam threshold dropped).  A hypothesis is (score, tokens, h, peak, lm score)."""
    N, H = p["linear_bias"].shape[0], p["start"].shape[0]
    bt, out, margin, amargin, dropped = min(beam_token, N), [], [np.inf], np.inf, 0
    ended = lambda x: bool(x[1]) and x[1][-1] == eos
    # the unweighted LM term of token n behind `tokens`: eos is the LM's EOS word, and nothing in a model without one
    q = lambda tokens, n: 0.0 if n == eos and not lm.has_eos else np.float64(lm.score(lm.history(tokens), lm.eos if n == eos else n, np.float64))

    def cut(s, n):   # the first n of a descending list are kept
        if n < len(s):
            margin[0] = min(margin[0], s[n - 1] - s[n])

    for b in range(enc.shape[0]):
        level, pool = [(0.0, (), torch.zeros(H, dtype=enc.dtype), -1, 0.0)], []
        last = level
        for u in range(max_len):
            pool += [x for x in level if ended(x)]
            live = [x for x in level if not ended(x)]
            if len(pool) >= beam:
                pool.sort(key=lambda x: -x[0])
                cut([x[0] for x in pool], beam)
                del pool[beam:]
            if not live:
                break
            h, o, alpha, z = D.step(p, enc, kl, keyvalue, [b] * len(live), [x[1][-1] if x[1] else -1 for x in live], torch.stack([x[2] for x in live]))
            lp, cands = torch.log_softmax(z, 1).numpy(), []
            for j, x in enumerate(live):
                a = alpha[j, :kl[b]].numpy()
                peak = int(a.argmax())
                if attention_threshold is not None:
                    if kl[b] > 1:
                        amargin = min(amargin, a[peak] - np.delete(a, peak).max())
                    if x[3] >= 0 and abs(peak - x[3]) > attention_threshold:
                        continue
                order = np.argsort(-lp[j], kind="stable")
                cut(list(lp[j][order]), bt)                                  # the tokens are chosen by the acoustic score alone
                for n, g in [(int(n), q(x[1], int(n))) for n in order[:bt]]:
                    cands.append((x[0] + lp[j][n] + (eos_score if n == eos else 0.0) + lm_weight * g, j, n, h[j], peak, x[4] + g))
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            if threshold is not None and cands:
                margin[0] = min(margin[0], min(abs(c[0] - (cands[0][0] - threshold)) for c in cands))
                dropped += sum(c[0] < cands[0][0] - threshold for c in cands)
                cands = [c for c in cands if c[0] >= cands[0][0] - threshold]
            cut([c[0] for c in cands], beam)
            level = [(c[0], live[c[1]][1] + (c[2],), c[3], c[4], c[5]) for c in cands[:beam]]
            level = [x for x in level if not ended(x)] + [x for x in level if ended(x)]
            last = level or last
        final = sorted(pool or last, key=lambda x: -x[0])
        s = [x[0] for x in final]
        cut(s, nbest)
        margin[0] = min([margin[0]] + [s[i] - s[i + 1] for i in range(min(nbest, len(s)) - 1)])
        out.append([(list(x[1]), x[0], x[4]) for x in final[:nbest]])
    return out, margin[0], amargin, dropped


# shape (B, T, H, N, keyvalue), (operand seed, scale of the output weight), LM (order, n-grams per order, eos, classes without a unigram,
# seed), LM weight, options.  B = 2 has key lengths (T, 1)
CASES = {
    "unigram_greedy": ((2, 19, 32, 11, False), (1, 10.0), (1, 0, True, (), 5), 0.8, dict(beam=1, beam_token=3, max_len=6, nbest=1)),
    "trigram_backoff": ((2, 19, 32, 37, True), (82, 10.0), (3, 150, True, tuple(range(3, 37, 3)), 6), 1.2, dict(beam=3, beam_token=4, max_len=8, nbest=3, eos_score=1.0)),
    "no_eos_threshold": ((2, 7, 32, 9, False), (3, 10.0), (3, 40, False, (4,), 7), 1.0, dict(beam=4, beam_token=9, max_len=12, nbest=3, threshold=2.0)),
    "wide": ((1, 19, 32, 70, False), (51, 30.0), (3, 400, True, (7,), 8), 0.7, dict(beam=128, beam_token=64, max_len=5, nbest=3, eos_score=90.0)),
    "attention_threshold": ((2, 40, 32, 37, True), (39, 10.0), (2, 120, True, (), 9), 1.0, dict(beam=4, beam_token=37, max_len=10, nbest=3, attention_threshold=3)),
}


@functools.lru_cache(maxsize=None)
def run_case(name):
    """computed once and shared: nobody changes it.  -> (parameters, enc, keyLen, keyvalue, the TextbookLM, LM weight, options, the
    reference's result, that result as the four arrays of the C ABI)"""
    shape, (seed, w_scale), (order, per, eos, drop, lm_seed), weight, opt = CASES[name]
    p, enc, kl = D.operands(*shape, seed, w_scale, D.K_SCALE)
    lm = random_lm(np.random.default_rng(lm_seed), shape[3], order, per, eos=eos, drop_unigrams=drop)
    ref = search(*D.f64(p, enc), kl, shape[4], D.EOS, lm, weight, **opt)
    arrays = [np.full((shape[0], opt["nbest"], opt["max_len"]), -1), *(np.full((shape[0], opt["nbest"]), v) for v in (0, -np.inf, -np.inf))]
    for b, utt in enumerate(ref[0]):
        for i, (t, s, g) in enumerate(utt):
            arrays[0][b, i, :len(t)], arrays[1][b, i], arrays[2][b, i], arrays[3][b, i] = t, len(t), s, g
    return p, enc, kl, shape[4], lm, weight, opt, ref, arrays
