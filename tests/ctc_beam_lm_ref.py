"""numpy restatement of w2l_ngram_lm_* and w2l_ctc_beam_search_lm's contracts (include/w2l_hip.h), shared by
test_ctc_beam_lm_host.py and test_gpu_ctc_beam_lm.py.

TextbookLM is the textbook back-off scorer on word tuples and dictionaries: p(w | h) = p[h + (w,)] if listed, else bo[h] (1 when h
is not listed) * p(w | h without its first word), <unk> for a word no context lists.  It knows nothing of states, suffix links or
hash tables: the library's table is held to it, and the search restatement below scores its prefixes with it.

beam_search_lm_one is ctc_beam_ref.beam_search_one with the LM terms of the contract.  Prefixes are tuples, the LM state of a
prefix is the prefix itself."""
import numpy as np

from tests.ctc_beam_ref import Diag, _oplus, frame_scores

F32 = np.float32


class TextbookLM:
    """ngrams: {word tuple: (logp, backoff)}, natural logs (kept as float32: that is what the table stores); words 0 .. V-1 the
    tokens, V = BOS, V + 1 = EOS"""

    def __init__(self, ngrams, num_tokens, unk_logp):
        self.p = {g: F32(v[0]) for g, v in ngrams.items()}
        self.order = max(len(g) for g in ngrams)
        self.bo = {g: F32(v[1]) for g, v in ngrams.items() if len(g) < self.order}
        self.V = num_tokens
        self.bos, self.eos = num_tokens, num_tokens + 1
        self.unk = F32(unk_logp)
        self.has_bos = (self.bos,) in self.p
        self.has_eos = (self.eos,) in self.p
        self.max_chain = 0      # the longest run of listed back-offs one query walked
        self.unk_hits = 0       # queries that ended at <unk>
        self._memo = {}

    def history(self, prefix):
        return ((self.bos,) if self.has_bos else ()) + tuple(prefix)

    def score(self, hist, w, dtype=F32):
        """log p(w | hist), the adds in `dtype` in the contract's order: ((bo1 + bo2) + ...) + p"""
        ctx = tuple(hist[max(0, len(hist) - (self.order - 1)):]) if self.order > 1 else ()
        memo = self._memo.get((ctx, w, dtype))
        if memo is not None:
            return memo
        start = ctx
        acc = dtype(0)
        chain = 0
        while True:
            if ctx + (w,) in self.p:
                out = dtype(acc + dtype(self.p[ctx + (w,)]))
                break
            if not ctx:
                out = dtype(acc + dtype(self.unk))
                self.unk_hits += 1
                break
            if ctx in self.bo:
                acc = dtype(acc + dtype(self.bo[ctx]))
                chain += 1
            ctx = ctx[1:]
        self.max_chain = max(self.max_chain, chain)
        self._memo[(start, w, dtype)] = out
        return out

    def sentence(self, labels, dtype=F32):
        """the unweighted LM score of a hypothesis as lmScores defines it: q in label order, then the EOS term"""
        hist = self.history(())
        acc = dtype(0)
        for c in labels:
            acc = dtype(acc + self.score(hist, int(c), dtype))
            hist = hist + (int(c),)
        if self.has_eos:
            acc = dtype(acc + self.score(hist, self.eos, dtype))
        return acc

    def arrays(self):
        """from_ngrams' argument: per order (words, logp, backoff)"""
        out = []
        for k in range(1, self.order + 1):
            gs = sorted(g for g in self.p if len(g) == k)
            out.append((np.array(gs, np.int32).reshape(len(gs), k), np.array([self.p[g] for g in gs], F32),
                        np.array([self.bo.get(g, 0) for g in gs], F32)))
        return out


class LmDiag(Diag):
    """Diag, and what shows that a case exercises the LM paths: lanes whose extension totals were not non-increasing in k (the
    LM-free kernel's selection would be wrong there), extensions merged into a stay, hypotheses whose rank the end term changed"""

    def __init__(self):
        super().__init__()
        self.nonmonotone = 0
        self.merges = 0
        self.eos_moves = 0


def beam_search_lm_one(x, F, W, K, lm, lm_weight, class_score=None, eos_score=0.0, threshold=np.inf, log_add=False,
                       normalize=False, dtype=F32, M=None, lm_dtype=F32):
    """x [T][N] float32 -> ([(labels tuple, score, lm score)] in rank order, LmDiag).  lm_dtype: the precision of q and g
    (float32: the contract's; float64: for the comparison with the enumeration)"""
    lp_all = frame_scores(np.asarray(x)[:F], normalize, dtype)
    N = lp_all.shape[1]
    blank = N - 1
    K = min(K, N - 1)
    ninf = dtype(-np.inf)
    thr = dtype(threshold)
    lmw = lm_dtype(lm_weight)
    d = LmDiag()

    def g_of(prefix, c):
        g = lm_dtype(lmw * lm.score(lm.history(prefix), c, lm_dtype))
        if class_score is not None:
            g = lm_dtype(g + lm_dtype(class_score[c]))
        return g

    beam = [((), dtype(0), ninf, np.inf)]
    for t in range(F):
        lp = lp_all[t]
        nb = lp[:blank]
        order = np.lexsort((np.arange(blank), -nb))
        toks = [int(c) for c in order[:K]]
        if K < blank:
            d.token_gap = min(d.token_gap, float(nb[order[K - 1]] - nb[order[K]]))
        index = {p: j for j, (p, _, _, _) in enumerate(beam)}
        tots = [_oplus(pb, pnb, log_add) for _, pb, pnb, _ in beam]
        stay = [[lp[blank] + tots[r], (lp[p[-1]] + pnb) if p else ninf] for r, (p, pb, pnb, _) in enumerate(beam)]
        exts = []
        for r, (p, pb, pnb, _) in enumerate(beam):
            e = p[-1] if p else -1
            lane = []
            for k, c in enumerate(toks):
                val = dtype(dtype(lp[c] + (pb if c == e else tots[r])) + dtype(g_of(p, c)))
                if c != e:
                    lane.append(val)
                j = index.get(p + (c,))
                if j is not None:
                    stay[j][1] = _oplus(stay[j][1], val, log_add)
                    d.merges += 1
                else:
                    exts.append((val, r, 1, k, p + (c,), ninf, val))
            if any(b > a for a, b in zip(lane, lane[1:])):
                d.nonmonotone += 1
        cands = [(_oplus(s[0], s[1], log_add), r, 0, 0, beam[r][0], s[0], s[1]) for r, s in enumerate(stay)] + exts
        cands = [c for c in cands if c[0] != -np.inf]
        if not cands:
            beam = []
            break
        best = max(c[0] for c in cands)
        line = dtype(best - thr)
        d.S = max(d.S, max(abs(float(c[0])) for c in cands))
        if np.isfinite(threshold):
            d.threshold_gap = min(d.threshold_gap, min(abs(float(c[0] - line)) for c in cands))
        cands = [c for c in cands if not c[0] < line]
        cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
        first_dropped = float(cands[W][0]) if len(cands) > W else -np.inf
        if len(cands) > W:
            d.beam_gap = min(d.beam_gap, float(cands[W - 1][0]) - first_dropped)
        floor = max(first_dropped, float(line))
        beam = [(c[4], c[5], c[6], min(beam[c[1]][3], float(c[0]) - floor)) for c in cands[:W]]
    out = []
    for r, (p, pb, pnb, mg) in enumerate(beam):
        s = _oplus(pb, pnb, log_add)
        if lm.has_eos:
            ge = lm_dtype(lm_dtype(lmw * lm.score(lm.history(p), lm.eos, lm_dtype)) + lm_dtype(eos_score))
            s = dtype(s + dtype(ge))
        else:
            assert eos_score == 0
        out.append((p, s, mg, r))
    ranked = sorted(out, key=lambda o: (-o[1], o[3]))
    d.eos_moves = sum(1 for i, o in enumerate(ranked) if o[3] != i)
    d.S = max([d.S] + [abs(float(o[1])) for o in ranked if np.isfinite(o[1])])
    m_out = len(ranked) if M is None else min(M, len(ranked))
    d.final_gaps = [float(ranked[m][1] - ranked[m + 1][1]) for m in range(min(m_out, len(ranked) - 1))]
    d.margins = [o[2] for o in ranked[:m_out]]
    return [(o[0], o[1], lm.sentence(o[0], F32)) for o in ranked[:m_out]], d


def beam_search_lm(x, frames, W, K, lm, lm_weight, class_score, eos_score, threshold, log_add, normalize, M, Lmax, dtype,
                   lm_dtype=F32):
    """the C ABI's outputs: labels [B][M][Lmax], lengths [B][M], scores [B][M] (dtype), lm_scores [B][M] float32, the LmDiags"""
    x = np.asarray(x, F32)
    B, T, _ = x.shape
    labels = np.full((B, M, Lmax), -1, np.int32)
    lengths = np.full((B, M), -1, np.int32)
    scores = np.full((B, M), -np.inf, dtype)
    lm_scores = np.full((B, M), -np.inf, F32)
    diags = []
    for b in range(B):
        F = T if frames is None else int(frames[b])
        hyps, dg = beam_search_lm_one(x[b], F, W, K, lm, lm_weight, class_score, eos_score, threshold, log_add, normalize, dtype,
                                      M, lm_dtype)
        diags.append(dg)
        for m, (p, s, ls) in enumerate(hyps):
            lengths[b, m] = len(p)
            labels[b, m, :min(len(p), Lmax)] = p[:Lmax]
            scores[b, m] = s
            lm_scores[b, m] = ls
    return labels, lengths, scores, lm_scores, diags


def delta_lm(T, S):
    """ctc_beam_ref.delta with one more dependent rounding per frame, the add of g (g itself is fp32 on both sides)"""
    return 2.0 * T * (5.0 * 2.0 ** -24 * max(1.0, S) + 4e-6)


def random_lm(rng, V, order, n_per_order, bos=True, eos=True, drop_unigrams=(), eighths=False, unk=-6.0, hot=None):
    """a random back-off model as TextbookLM: every listed n-gram's context is listed; some contexts are listed with a back-off
    and no extension; the classes in drop_unigrams have no unigram (they score as <unk>).  eighths: every value a multiple of
    1/8 (sums of them are exact in fp32).  hot: the n-grams of order 2 and above use the classes below `hot` only"""
    def val(lo, hi):
        return F32(rng.integers(int(lo * 8), int(hi * 8) + 1) / 8) if eighths else F32(rng.uniform(lo, hi))
    words = [w for w in range(V) if w not in set(drop_unigrams)]
    ng = {}
    for w in words:
        ng[(w,)] = (val(-5, -0.5), val(-2, 0))
    if bos:
        ng[(V,)] = (F32(-99.0), val(-2, 0))
    if eos:
        ng[(V + 1,)] = (val(-5, -0.5), F32(0))
    if hot is not None:
        words = [w for w in words if w < hot]
    prev = [g for g in ng if g != (V + 1,) and (g[0] == V or g[0] in set(words))]   # contexts: nothing follows EOS
    for k in range(2, order + 1):
        cur = []
        if prev:
            for _ in range(n_per_order):
                ctx = prev[int(rng.integers(len(prev)))]
                last = words + ([V + 1] if eos else [])
                g = ctx + (int(last[int(rng.integers(len(last)))]),)
                if g not in ng:
                    ng[g] = (val(-4, -0.25), val(-2, 0))
                    if g[-1] != V + 1 and V not in g[1:]:
                        cur.append(g)
        prev = cur
    return TextbookLM(ng, V, unk)
