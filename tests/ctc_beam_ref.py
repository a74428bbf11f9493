"""numpy restatement of w2l_ctc_beam_search's contract (include/w2l_hip.h), shared by test_ctc_beam_host.py and
test_gpu_ctc_beam.py.

Prefixes are tuples of labels, so "spells the same prefix" is tuple equality.  dtype = float32 reproduces the kernel bit for bit
when logAdd = 0 (every value is one fp32 add of two stored values, or a compare); dtype = float64 is the reference for logAdd = 1.
Besides the hypotheses the search returns what the tests need to know how far every decision it took was from going the other
way (see Diag)."""
import numpy as np


class Diag:
    """S: largest finite |score| seen.  token_gap: K-th against (K+1)-th frame token.  beam_gap: W-th kept against the first
    dropped candidate.  threshold_gap: distance of any candidate from the threshold line.  final_gaps: totals of ranks m, m+1 for
    m < M (the (M+1)-th entry included when it exists).  margins[m]: over the ancestors of final hypothesis m, the smallest
    distance by which one of them survived a selection (against the first dropped candidate and the threshold line)."""

    def __init__(self):
        self.S = 0.0
        self.token_gap = np.inf
        self.beam_gap = np.inf
        self.threshold_gap = np.inf
        self.final_gaps = []
        self.margins = []

    def decision_gap(self):
        return min(self.token_gap, self.beam_gap, self.threshold_gap)


def _oplus(a, b, log_add):
    m = a if a >= b else b
    if not log_add or m == -np.inf:
        return m
    lo = b if a >= b else a
    return m + np.log1p(np.exp(lo - m))


def frame_scores(x, normalize, dtype):
    x = np.asarray(x, np.float32)
    if not normalize:
        return x.astype(dtype)
    xd = x.astype(dtype)
    m = xd.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(xd - m).sum(axis=1, keepdims=True, dtype=dtype))
    return (xd - lse).astype(dtype)


def beam_search_one(x, F, W, K, threshold=np.inf, log_add=False, normalize=False, dtype=np.float32, M=None):
    """x [T][N] float32 -> ([(labels tuple, score)] in rank order (at most M of them; all when M is None), Diag)"""
    lp_all = frame_scores(np.asarray(x)[:F], normalize, dtype)
    N = lp_all.shape[1]
    blank = N - 1
    K = min(K, N - 1)
    ninf = dtype(-np.inf)
    thr = dtype(threshold)
    d = Diag()
    beam = [((), dtype(0), ninf, np.inf)]                       # prefix, pb, pnb, lineage margin
    for t in range(F):
        lp = lp_all[t]
        nb = lp[:blank]
        order = np.lexsort((np.arange(blank), -nb))              # lp descending, class ascending
        toks = [int(c) for c in order[:K]]
        if K < blank:
            d.token_gap = min(d.token_gap, float(nb[order[K - 1]] - nb[order[K]]))
        index = {p: j for j, (p, _, _, _) in enumerate(beam)}
        tots = [_oplus(pb, pnb, log_add) for _, pb, pnb, _ in beam]
        stay = [[lp[blank] + tots[r], (lp[p[-1]] + pnb) if p else ninf] for r, (p, pb, pnb, _) in enumerate(beam)]
        exts = []
        for r, (p, pb, pnb, _) in enumerate(beam):
            e = p[-1] if p else -1
            for k, c in enumerate(toks):
                val = lp[c] + (pb if c == e else tots[r])
                j = index.get(p + (c,))
                if j is not None:
                    stay[j][1] = _oplus(stay[j][1], val, log_add)
                else:
                    exts.append((val, r, 1, k, p + (c,), ninf, val))
        cands = [(_oplus(s[0], s[1], log_add), r, 0, 0, beam[r][0], s[0], s[1]) for r, s in enumerate(stay)] + exts
        cands = [c for c in cands if c[0] != -np.inf]
        if not cands:
            beam = []
            break
        best = max(c[0] for c in cands)
        line = dtype(best - thr)
        fin = [abs(float(c[0])) for c in cands]
        d.S = max(d.S, max(fin))
        if np.isfinite(threshold):
            d.threshold_gap = min(d.threshold_gap, min(abs(float(c[0] - line)) for c in cands))
        cands = [c for c in cands if not c[0] < line]
        cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
        first_dropped = float(cands[W][0]) if len(cands) > W else -np.inf
        if len(cands) > W:
            d.beam_gap = min(d.beam_gap, float(cands[W - 1][0]) - first_dropped)
        floor = max(first_dropped, float(line))
        beam = [(c[4], c[5], c[6], min(beam[c[1]][3], float(c[0]) - floor)) for c in cands[:W]]
    out = [(p, _oplus(pb, pnb, log_add), mg) for p, pb, pnb, mg in beam]
    m_out = len(out) if M is None else min(M, len(out))
    d.final_gaps = [float(out[m][1] - out[m + 1][1]) for m in range(min(m_out, len(out) - 1))]
    d.margins = [mg for _, _, mg in out[:m_out]]
    return [(p, s) for p, s, _ in out[:m_out]], d


def beam_search(x, frames, W, K, threshold, log_add, normalize, M, Lmax, dtype):
    """the C ABI's outputs: labels [B][M][Lmax], lengths [B][M], scores [B][M] (dtype), and the per-utterance Diags"""
    x = np.asarray(x, np.float32)
    B, T, _ = x.shape
    labels = np.full((B, M, Lmax), -1, np.int32)
    lengths = np.full((B, M), -1, np.int32)
    scores = np.full((B, M), -np.inf, dtype)
    diags = []
    for b in range(B):
        F = T if frames is None else int(frames[b])
        hyps, dg = beam_search_one(x[b], F, W, K, threshold, log_add, normalize, dtype, M)
        diags.append(dg)
        for m, (p, s) in enumerate(hyps):
            lengths[b, m] = len(p)
            labels[b, m, :min(len(p), Lmax)] = p[:Lmax]
            scores[b, m] = s
    return labels, lengths, scores, diags


def delta(T, S):
    """the fp32 kernel against the float64 restatement, logAdd = 1: four dependent fp32 roundings per frame on magnitudes <= S,
    two transcendental evaluations of absolute error <= 2e-6, linear accumulation, both sides"""
    return 2.0 * T * (4.0 * 2.0 ** -24 * max(1.0, S) + 4e-6)


def enumerate_labellings(x, log_add, normalize):
    """every one of the N^T paths of x [T][N] (float64): {labelling: sum (logAdd) or max of its paths' scores}"""
    import itertools
    lp = frame_scores(x, normalize, np.float64)
    T, N = lp.shape
    blank = N - 1
    acc = {}
    for path in itertools.product(range(N), repeat=T):
        s = float(sum(lp[t, c] for t, c in enumerate(path)))
        lab, prev = [], None
        for c in path:
            if c != prev and c != blank:
                lab.append(c)
            prev = c
        lab = tuple(lab)
        if log_add:
            acc.setdefault(lab, []).append(s)
        else:
            acc[lab] = max(acc.get(lab, -np.inf), s)
    if log_add:
        for lab, v in acc.items():
            v = np.array(v)
            m = v.max()
            acc[lab] = float(m + np.log(np.exp(v - m).sum()))
    return acc
