"""float64 restatement of the seq2seq decoder's contract: one decoder step and the token beam search of the
reference's LexiconFreeSeq2SeqDecoder with a zero LM.  The GRU cell is tests/rnn_ref.py's and the attention tests/s2s_ref.py's.  The
search also reports its smallest decision margins, so that a test can tell where exact agreement is a fair demand."""
import functools

import numpy as np
import torch

import rnn_ref as RR
import s2s_ref as R

NAMES = ("embedding", "start", "rnn", "linear_weight", "linear_bias")


def step(p, enc, kl, keyvalue, utt, tok, h_prev, temperature=1.0):
    """rows of any utterances: utt [R] the utterance of a row, tok [R] (-1: the start embedding; its h_prev must be zero), h_prev [R][H]
    -> h [R][H], o [R][H], alpha [R][T], z [R][N]"""
    H, utt = p["start"].shape[0], np.asarray(utt)
    wih, whh, bih, bhh = RR.unpack(p["rnn"], 3, H, H, 1, 1)[0]
    h, _ = RR.cell(3, H, R.embedding(tok, p["embedding"], p["start"]) @ wih.T + bih, h_prev, None, whh, bhh)
    ctx, alpha = R.attention(h[:, None], enc[utt], np.asarray(kl)[utt], np.ones(len(utt)), keyvalue, None)
    o = h + ctx[:, 0]
    return h, o, alpha[:, 0], (o @ p["linear_weight"] + p["linear_bias"]) / temperature


def search(p, enc, kl, keyvalue, eos, beam, beam_token, max_len, nbest, threshold=None, eos_score=0.0, attention_threshold=None, temperature=1.0):
    """-> (per utterance the best nbest (tokens, score), the smallest score margin of any decision -- a token, a candidate or a finished
    hypothesis kept against one dropped, a threshold test, the order of the results --, the smallest gap between the two largest
    attention weights where a peak is compared)"""
    N, H = p["linear_bias"].shape[0], p["start"].shape[0]
    bt, out, margin, amargin = min(beam_token, N), [], [np.inf], np.inf
    ended = lambda x: bool(x[1]) and x[1][-1] == eos

    def cut(s, n):   # the first n of a descending list are kept
        if n < len(s):
            margin[0] = min(margin[0], s[n - 1] - s[n])

    for b in range(enc.shape[0]):
        level, pool = [(0.0, (), torch.zeros(H, dtype=enc.dtype), -1)], []   # (score, tokens, h, peak), live hypotheses in front
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
            h, o, alpha, z = step(p, enc, kl, keyvalue, [b] * len(live), [x[1][-1] if x[1] else -1 for x in live], torch.stack([x[2] for x in live]), temperature)
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
                cut(list(lp[j][order]), bt)
                cands += [(x[0] + lp[j][n] + (eos_score if n == eos else 0.0), j, int(n), h[j], peak) for n in order[:bt]]
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            if threshold is not None and cands:
                margin[0] = min(margin[0], min(abs(c[0] - (cands[0][0] - threshold)) for c in cands))
                cands = [c for c in cands if c[0] >= cands[0][0] - threshold]
            cut([c[0] for c in cands], beam)
            level = [(c[0], live[c[1]][1] + (c[2],), c[3], c[4]) for c in cands[:beam]]
            level = [x for x in level if not ended(x)] + [x for x in level if ended(x)]
            last = level or last
        final = sorted(pool or last, key=lambda x: -x[0])
        s = [x[0] for x in final]
        cut(s, nbest)
        margin[0] = min([margin[0]] + [s[i] - s[i + 1] for i in range(min(nbest, len(s)) - 1)])
        out.append([(list(x[1]), x[0]) for x in final[:nbest]])
    return out, margin[0], amargin


def operands(B, T, H, N, keyvalue, seed, w_scale=1.0, k_scale=1.0):
    """(parameters in the order of NAMES, enc, keyLen): float32 numpy; the output weight times w_scale spreads the logits, the keys
    times k_scale sharpen the attention; ragged key lengths, one of them 1"""
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32) * H ** -0.5
    p = [u(N, H), rng.uniform(-0.1, 0.1, H).astype(np.float32), u(3 * H * (2 * H + 2)), u(H, N) * np.float32(w_scale), u(N)]
    enc = rng.normal(size=(B, T, 2 * H if keyvalue else H)).astype(np.float32)
    enc[..., :H] *= np.float32(k_scale)
    return p, enc, np.array([T, 1, T // 2 + 1][:B], np.int32)


def f64(p, enc):
    return {n: torch.tensor(x, dtype=torch.float64) for n, x in zip(NAMES, p)}, torch.tensor(enc, dtype=torch.float64)


# the searches both test files run: shape (B, T, H, N, keyvalue), seed, the search's options
CASES = {
    "greedy": ((3, 19, 32, 11, False), 1, dict(beam=1, beam_token=3, max_len=6, nbest=1)),
    "threshold": ((2, 19, 32, 37, True), 16, dict(beam=4, beam_token=3, max_len=20, nbest=3, threshold=2.0)),
    "two_row_tiles": ((2, 19, 32, 130, False), 1, dict(beam=33, beam_token=3, max_len=6, nbest=3)),
    "attention_threshold": ((3, 41, 32, 37, True), 30, dict(beam=4, beam_token=37, max_len=20, nbest=3, attention_threshold=3)),
    "eos_early": ((2, 19, 32, 11, False), 1, dict(beam=4, beam_token=11, max_len=20, nbest=3, eos_score=3.0)),
    "eos_early_wide": ((2, 19, 32, 11, False), 32, dict(beam=33, beam_token=11, max_len=6, nbest=3, eos_score=3.0)),
    "max_len_empty_pool": ((3, 19, 32, 11, True), 4, dict(beam=4, beam_token=3, max_len=6, nbest=3, eos_score=-100.0)),
}
W_SCALE, K_SCALE, EOS = 10.0, 6.0, 0


@functools.lru_cache(maxsize=None)
def run_case(name):
    """computed once and shared: nobody changes it.  -> (parameters, enc, keyLen, keyvalue, options, the reference's result)"""
    shape, seed, opt = CASES[name]
    p, enc, kl = operands(*shape, seed, W_SCALE, K_SCALE)
    return p, enc, kl, shape[4], opt, search(*f64(p, enc), kl, shape[4], EOS, **opt)
