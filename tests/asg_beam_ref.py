"""numpy restatement of w2l_asg_beam_search's and w2l_asg_beam_search_lex's contracts (include/w2l_hip.h), shared by
test_asg_beam_host.py and test_gpu_asg_beam.py.

Prefixes are tuples of labels; a lexicon hypothesis is the tuple of its extensions (token, word or None); the lexicon is the
textbook dict trie of ctc_beam_lex_ref, the LM the textbook back-off scorer of ctc_beam_lm_ref (over all N classes: there is no
blank).  dtype = float32 reproduces the kernels bit for bit when logAdd = 0; dtype = float64 is the reference for logAdd = 1.
An entry has ONE value p: stay is (p + A[e][e]) + lp[e], an extension by c != e is (p + A[c][e]) + lp[c] (lp[c] alone from the
empty prefix), then the siblings' LM or smear / word terms; c == e makes no candidate."""
import itertools

import numpy as np

from tests.ctc_beam_ref import Diag, _oplus, frame_scores

F32 = np.float32


class AsgDiag(Diag):
    """Diag's margins, and: cuts, the candidates W cut (those the threshold left standing beyond the W-th); skipped, the (entry,
    frame token) pairs with c == e; merges; unreachable, the lexicon's words whose spelling has one token twice in a row;
    track_lost, the frames after which the tracked prefix (see `track`) was not in the beam; end_dropped and eos_moves as in the
    siblings' diags"""

    def __init__(self):
        super().__init__()
        self.cuts = self.skipped = self.merges = self.unreachable = self.track_lost = self.end_dropped = self.eos_moves = 0


def _select(cands, beam, W, thr, threshold, dtype, d, nkey):
    """the siblings' prune and order over candidates (total, r, ext, k[, slot], ...): the kept ones with their lineage margin"""
    cands = [c for c in cands if c[0] != -np.inf]
    if not cands:
        return None
    best = max(c[0] for c in cands)
    line = dtype(best - thr)
    d.S = max(d.S, max(abs(float(c[0])) for c in cands))
    if np.isfinite(threshold):
        d.threshold_gap = min(d.threshold_gap, min(abs(float(c[0] - line)) for c in cands))
    cands = [c for c in cands if not c[0] < line]
    cands.sort(key=lambda c: (-c[0],) + tuple(c[1:nkey]))
    first_dropped = float(cands[W][0]) if len(cands) > W else -np.inf
    if len(cands) > W:
        d.beam_gap = min(d.beam_gap, float(cands[W - 1][0]) - first_dropped)
        d.cuts += len(cands) - W
    floor = max(first_dropped, float(line))
    return [(c, min(beam[c[1]][2], float(c[0]) - floor)) for c in cands[:W]]


def _frame_tokens(lp, K, d):
    N = lp.shape[0]
    order = np.lexsort((np.arange(N), -lp))                      # lp descending, class ascending; every class is a token
    if K < N:
        d.token_gap = min(d.token_gap, float(lp[order[K - 1]] - lp[order[K]]))
    return [int(c) for c in order[:K]]


def asg_beam_one(x, A, F, W, K, lm=None, lm_weight=0.0, class_score=None, eos_score=0.0, threshold=np.inf, log_add=False,
                 normalize=False, dtype=F32, M=None, lm_dtype=F32, track=None):
    """x [T][N], A [N][N] (to x from) float32 -> ([(labels tuple, score, lm score)] in rank order, AsgDiag).  lm: a TextbookLM
    over N tokens or None.  track: per frame the prefix that must be in the beam after it (d.track_lost counts the misses)"""
    lp_all = frame_scores(np.asarray(x)[:F], normalize, dtype)
    N = lp_all.shape[1]
    A = np.asarray(np.asarray(A, F32), dtype)                   # no copy at float32: N = 9998 is 400 MB
    K = min(K, N)
    ninf, thr, lmw = dtype(-np.inf), dtype(threshold), lm_dtype(lm_weight)
    d = AsgDiag()

    def g_of(prefix, c):
        g = lm_dtype(lmw * lm.score(lm.history(prefix), c, lm_dtype))
        if class_score is not None:
            g = lm_dtype(g + lm_dtype(class_score[c]))
        return g

    beam = [((), dtype(0), np.inf)]                              # prefix, p, lineage margin
    for t in range(F):
        lp = lp_all[t]
        toks = _frame_tokens(lp, K, d)
        index = {en[0]: j for j, en in enumerate(beam)}
        stay = [dtype(dtype(p + A[pre[-1], pre[-1]]) + lp[pre[-1]]) if pre else ninf for pre, p, _ in beam]
        exts = []
        for r, (pre, p, _) in enumerate(beam):
            e = pre[-1] if pre else -1
            for k, c in enumerate(toks):
                if c == e:
                    d.skipped += 1
                    continue
                val = lp[c] if not pre else dtype(dtype(p + A[c, e]) + lp[c])
                if lm is not None:
                    val = dtype(val + dtype(g_of(pre, c)))
                j = index.get(pre + (c,))
                if j is not None:
                    stay[j] = _oplus(stay[j], val, log_add)
                    d.merges += 1
                else:
                    exts.append((val, r, 1, k, pre + (c,)))
        kept = _select([(s, r, 0, 0, beam[r][0]) for r, s in enumerate(stay)] + exts, beam, W, thr, threshold, dtype, d, 4)
        if kept is None:
            beam = []
            break
        beam = [(c[4], c[0], mg) for c, mg in kept]
        if track is not None and track[t] not in {en[0] for en in beam}:
            d.track_lost += 1
    out = []
    for r, (pre, p, mg) in enumerate(beam):
        s = p
        if lm is not None and lm.has_eos:
            ge = lm_dtype(lm_dtype(lmw * lm.score(lm.history(pre), lm.eos, lm_dtype)) + lm_dtype(eos_score))
            s = dtype(s + dtype(ge))
        else:
            assert eos_score == 0
        out.append((pre, s, mg, r))
    ranked = sorted(out, key=lambda o: (-o[1], o[3]))
    d.eos_moves = sum(1 for i, o in enumerate(ranked) if o[3] != i)
    d.S = max([d.S] + [abs(float(o[1])) for o in ranked if np.isfinite(o[1])])
    m_out = len(ranked) if M is None else min(M, len(ranked))
    d.final_gaps = [float(ranked[m][1] - ranked[m + 1][1]) for m in range(min(m_out, len(ranked) - 1))]
    d.margins = [o[2] for o in ranked[:m_out]]
    return [(o[0], o[1], F32(0) if lm is None else lm.sentence(o[0], F32)) for o in ranked[:m_out]], d


def asg_beam_lex_one(x, A, F, W, K, trie, lm, lm_weight, word_score=0.0, eos_score=0.0, threshold=np.inf, log_add=False,
                     normalize=False, dtype=F32, M=None, lm_dtype=F32):
    """-> ([(labels tuple, words tuple, score, lm score, hypothesis)] in rank order, AsgDiag); trie: a TextbookTrie over N tokens,
    lm: a TextbookLM over its words"""
    lp_all = frame_scores(np.asarray(x)[:F], normalize, dtype)
    N = lp_all.shape[1]
    A = np.asarray(np.asarray(A, F32), dtype)                   # no copy at float32: N = 9998 is 400 MB
    K = min(K, N)
    ninf, thr = dtype(-np.inf), dtype(threshold)
    lmw, wsc = lm_dtype(lm_weight), lm_dtype(word_score)
    d = AsgDiag()
    d.unreachable = len({w for w, sp in trie.rows} - {w for w, sp in trie.rows if all(a != b for a, b in zip(sp, sp[1:]))})
    root = trie.root
    beam = [((), dtype(0), np.inf, root, ())]                    # hypothesis, p, lineage margin, lexicon node, words
    for t in range(F):
        lp = lp_all[t]
        toks = _frame_tokens(lp, K, d)
        index = {en[0]: j for j, en in enumerate(beam)}
        stay = [dtype(dtype(en[1] + A[en[0][-1][0], en[0][-1][0]]) + lp[en[0][-1][0]]) if en[0] else ninf for en in beam]
        exts = []
        for r, (hyp, p, _, u, words) in enumerate(beam):
            e = hyp[-1][0] if hyp else -1
            for k, c in enumerate(toks):
                if c == e:
                    d.skipped += 1
                    continue
                a0 = lp[c] if not hyp else dtype(dtype(p + A[c, e]) + lp[c])
                made = []                                        # (slot, value, hypothesis, node, words)
                if c == trie.sil and u is root:
                    made.append((0, a0, hyp + ((c, None),), root, words))
                else:
                    v = u.children.get(c)
                    if v is None:
                        continue
                    su = lm_dtype(0) if u is root else lm_dtype(u.smear)
                    smv = lm_dtype(v.smear)
                    a = dtype(a0 + dtype(lm_dtype(lmw * lm_dtype(smv - su))))
                    if v.children:
                        made.append((0, a, hyp + ((c, None),), v, words))
                    for i, w in enumerate(v.words):
                        q = lm.score(lm.history(words), w, lm_dtype)
                        val = dtype(a + dtype(lm_dtype(lm_dtype(lmw * lm_dtype(q - smv)) + wsc)))
                        made.append((1 + i, val, hyp + ((c, w),), root, words + (w,)))
                for slot, val, nh, nu, nwords in made:
                    j = index.get(nh)
                    if j is not None:
                        stay[j] = _oplus(stay[j], val, log_add)
                        d.merges += 1
                    else:
                        exts.append((val, r, 1, k, slot, nh, nu, nwords))
        cands = [(s, r, 0, 0, 0, beam[r][0], beam[r][3], beam[r][4]) for r, s in enumerate(stay)] + exts
        kept = _select(cands, beam, W, thr, threshold, dtype, d, 5)
        if kept is None:
            beam = []
            break
        beam = [(c[5], c[0], mg, c[6], c[7]) for c, mg in kept]
    out = []
    d.end_dropped = sum(1 for en in beam if en[3] is not root)
    for r, (hyp, p, mg, u, words) in enumerate(beam):
        if u is not root:
            continue
        s = p
        if lm.has_eos:
            ge = lm_dtype(lm_dtype(lmw * lm.score(lm.history(words), lm.eos, lm_dtype)) + lm_dtype(eos_score))
            s = dtype(s + dtype(ge))
        else:
            assert eos_score == 0
        out.append((hyp, s, mg, r, words))
    ranked = sorted(out, key=lambda o: (-o[1], o[3]))
    d.eos_moves = sum(1 for i, o in enumerate(ranked) if o[3] != out[i][3])
    d.S = max([d.S] + [abs(float(o[1])) for o in ranked if np.isfinite(o[1])])
    m_out = len(ranked) if M is None else min(M, len(ranked))
    d.final_gaps = [float(ranked[m][1] - ranked[m + 1][1]) for m in range(min(m_out, len(ranked) - 1))]
    d.margins = [o[2] for o in ranked[:m_out]]
    return [(tuple(c for c, _ in o[0]), o[4], o[1], lm.sentence(o[4], F32), o[0]) for o in ranked[:m_out]], d


def asg_beam(x, A, frames, W, K, M, Lmax, dtype=F32, trie=None, max_words=None, **kw):
    """the C ABI's outputs as a dict: labels [B][M][Lmax], lengths, scores (dtype), lm_scores float32; with a trie also words
    [B][M][max_words] and word_counts; diags"""
    x = np.asarray(x, F32)
    B, T, _ = x.shape
    o = dict(labels=np.full((B, M, Lmax), -1, np.int32), lengths=np.full((B, M), -1, np.int32),
             scores=np.full((B, M), -np.inf, dtype), lm_scores=np.full((B, M), -np.inf, F32), diags=[])
    if trie is not None:
        max_words = Lmax if max_words is None else max_words
        o["words"] = np.full((B, M, max_words), -1, np.int32)
        o["word_counts"] = np.full((B, M), -1, np.int32)
    for b in range(B):
        F = T if frames is None else int(frames[b])
        if trie is None:
            hyps, dg = asg_beam_one(x[b], A, F, W, K, dtype=dtype, M=M, **kw)
            hyps = [(p, (), s, ls) for p, s, ls in hyps]
        else:
            hyps, dg = asg_beam_lex_one(x[b], A, F, W, K, trie, dtype=dtype, M=M, **kw)
        o["diags"].append(dg)
        for m, h in enumerate(hyps):
            p, ws, s, ls = h[:4]
            o["lengths"][b, m] = len(p)
            o["labels"][b, m, :min(len(p), Lmax)] = p[:Lmax]
            o["scores"][b, m] = s
            o["lm_scores"][b, m] = ls
            if trie is not None:
                o["word_counts"][b, m] = len(ws)
                o["words"][b, m, :min(len(ws), max_words)] = ws[:max_words]
    return o


def delta_asg(T, S, extra=0):
    """the fp32 kernel against the float64 restatement, logAdd = 1, derived as ctc_beam_ref.delta is: per frame the dependent fp32
    roundings on magnitudes <= S are the transition add, the emission add and the two of (+) (4, as CTC's 4: the blank's add is
    gone, the transition's is new), plus `extra` for the siblings' terms (1: the add of g; 4: the lexicon's smear add, word add,
    the sum inside the word term and the subtraction inside it); two transcendental evaluations of absolute error <= 2e-6; linear
    accumulation; both sides"""
    return 2.0 * T * ((4.0 + extra) * 2.0 ** -24 * max(1.0, S) + 4e-6)


def viterbi(x, A):
    """the fp32 max recursion in w2l_viterbi_compute's order, (p + A[c][e]) + x[t][c], lowest index on ties: (path [T], score)"""
    x, A = np.asarray(x, F32), np.asarray(A, F32)
    T, N = x.shape
    p = x[0].copy()
    back = np.zeros((T, N), np.int64)
    for t in range(1, T):
        cand = (p[None, :] + A) + x[t][:, None]                  # [to][from], two fp32 adds
        back[t] = cand.argmax(axis=1)
        p = cand.max(axis=1)
    path = [int(p.argmax())]
    for t in range(T - 1, 0, -1):
        path.append(int(back[t, path[-1]]))
    return path[::-1], F32(p.max())


def collapse(path):
    return tuple(c for i, c in enumerate(path) if i == 0 or c != path[i - 1])


def enumerate_labellings(x, A, log_add, normalize):
    """every one of the N^T paths of x [T][N] in float64, score x[0][p0] + sum over t >= 1 of (A[pt][pt-1] + x[t][pt]), collapsed
    over runs: {labelling: sum (logAdd) or max of its paths' scores}"""
    lp = frame_scores(x, normalize, np.float64)
    A = np.asarray(A, np.float64)
    T, N = lp.shape
    acc = {}
    for path in itertools.product(range(N), repeat=T):
        s = float(lp[0, path[0]] + sum(A[path[t], path[t - 1]] + lp[t, path[t]] for t in range(1, T)))
        acc.setdefault(collapse(path), []).append(s)
    out = {}
    for lab, v in acc.items():
        v = np.array(v)
        out[lab] = float(v.max() + np.log(np.exp(v - v.max()).sum())) if log_add else float(v.max())
    return out


def enumerate_lm(x, A, lm, lm_weight, class_score, eos_score, log_add, normalize):
    """enumerate_labellings with the textbook LM's score of every labelling added, float64"""
    out = {}
    for lab, s in enumerate_labellings(x, A, log_add, normalize).items():
        hist = lm.history(())
        for c in lab:
            s += lm_weight * float(lm.score(hist, c, np.float64)) + (0.0 if class_score is None else float(class_score[c]))
            hist = hist + (c,)
        if lm.has_eos:
            s += lm_weight * float(lm.score(hist, lm.eos, np.float64)) + eos_score
        out[lab] = s
    return out


def enumerate_hypotheses(x, A, trie, lm, lm_weight, word_score, eos_score, log_add, normalize):
    """every labelling expanded into every (segmentation, homophone choice) the lexicon allows: {hypothesis: score}, float64"""
    out = {}
    for lab, s in enumerate_labellings(x, A, log_add, normalize).items():
        for hyp in trie.derivations(lab):
            words = tuple(w for _, w in hyp if w is not None)
            hist = lm.history(())
            q = 0.0
            for w in words:
                q += float(lm.score(hist, w, np.float64))
                hist = hist + (w,)
            total = s + lm_weight * q + word_score * len(words)
            if lm.has_eos:
                total += lm_weight * float(lm.score(hist, lm.eos, np.float64)) + eos_score
            out[hyp] = total
    return out
