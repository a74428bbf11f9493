"""numpy restatement of w2l_ctc_beam_search_lextok and w2l_asg_beam_search_lextok (include/w2l_hip.h): the beam searches under a
lexicon scored by a TOKEN-level LM, shared by test_beam_lextok_host.py, test_gpu_beam_lextok.py and
test_gpu_beam_lextok_containment.py.

lextok_beam_one is ctc_beam_lex_ref.beam_search_lex_one with the contract's changes written out: the lexicon (a TextbookTrie, whose
smear values are never read here) says which extensions exist and where words end; the LM (ctc_beam_lm_ref.TextbookLM over the
TOKENS, the textbook back-off scorer) scores every token that moves along a trie edge -- a = a0 + (lmWeight * q), the state
advances -- and a completed word adds wordScore alone.  The silence loop at the root has no LM term and leaves the state.  `A` (a
transition matrix) chooses the ASG lattice over the CTC one.  The silence score follows beam_sil_ref's rule.  A hypothesis is the
tuple of its extensions (token, word or None); its LM history is the tuple of the tokens that were LM-scored, which is a function
of it.  dtype = float32 reproduces the kernels bit for bit when logAdd = 0; dtype = float64 is the reference for logAdd = 1.
The LexDiag records the margin of every decision and counts merges, lexicon-blocked extensions and end drops."""
import numpy as np

from tests.ctc_beam_lex_ref import LexDiag
from tests.ctc_beam_ref import _oplus, frame_scores

F32 = np.float32


def lm_history(hyp, sil):
    """the tokens of a hypothesis that the LM scored: all but the silence loops at the root (slot 0 on sil at the root).  A sil
    extension is a loop exactly when the extension before it ended a word, or was such a loop, or there is none"""
    out, at_root = [], True
    for c, w in hyp:
        if not (c == sil and at_root):
            out.append(c)
            at_root = w is not None
    return tuple(out)


def lextok_beam_one(x, F, W, K, trie, lm, lm_weight, word_score=0.0, eos_score=0.0, A=None, sil=-1, sil_score=0.0,
                    threshold=np.inf, log_add=False, normalize=False, dtype=F32, M=None, lm_dtype=F32):
    """x [T][N] float32 -> ([(labels, words, score, lm score, hypothesis)] in rank order, LexDiag).  sil: the class of the silence
    SCORE (-1: none); the silence token of the lexicon is trie.sil"""
    lp_all = frame_scores(np.asarray(x)[:F], normalize, dtype)
    N = lp_all.shape[1]
    asg = A is not None
    ntok = N if asg else N - 1
    blank = -1 if asg else N - 1
    if asg:
        A = np.asarray(np.asarray(A, F32), dtype)
    K = min(K, ntok)
    ninf, thr = dtype(-np.inf), dtype(threshold)
    lmw, wsc = lm_dtype(lm_weight), lm_dtype(word_score)
    d = LexDiag()
    root = trie.root
    # entry: hypothesis, pb, pnb, lineage margin, lexicon node, words, LM history (the scored tokens), unweighted LM sum
    beam = [((), dtype(0), ninf, np.inf, root, (), (), F32(0))]
    for t in range(F):
        ac = lp_all[t]
        order = np.lexsort((np.arange(ntok), -ac[:ntok]))        # the ACOUSTIC lp descending, class ascending
        toks = [int(c) for c in order[:K]]
        if K < ntok:
            d.token_gap = min(d.token_gap, float(ac[order[K - 1]] - ac[order[K]]))
        lp = ac.copy()                                            # ... and only now the silence score
        if sil >= 0 and sil_score != 0:
            lp[sil] = dtype(lp[sil] + dtype(sil_score))
        index = {en[0]: j for j, en in enumerate(beam)}
        tots = [_oplus(en[1], en[2], log_add) for en in beam]
        stay = []
        for r, en in enumerate(beam):
            e = en[0][-1][0] if en[0] else -1
            if asg:
                stay.append([ninf, dtype(dtype(en[2] + A[e, e]) + lp[e]) if en[0] else ninf])
            else:
                stay.append([lp[blank] + tots[r], (lp[e] + en[2]) if en[0] else ninf])
        exts, blocked = [], []
        for r, (hyp, pb, pnb, _, u, words, hist, acc) in enumerate(beam):
            e = hyp[-1][0] if hyp else -1
            for k, c in enumerate(toks):
                if asg:
                    if c == e:
                        continue
                    a0 = lp[c] if not hyp else dtype(dtype(tots[r] + A[c, e]) + lp[c])
                else:
                    a0 = dtype(lp[c] + (pb if c == e else tots[r]))
                made = []                                        # (slot, value, hypothesis, node, words, history, lm sum)
                if c == trie.sil and u is root:
                    made.append((0, a0, hyp + ((c, None),), root, words, hist, acc))
                else:
                    v = u.children.get(c)
                    if v is None:
                        d.blocked += 1
                        blocked.append(a0)
                        continue
                    q = lm.score(lm.history(hist), c, lm_dtype)           # ONE lookup per (entry, token) pair
                    a = dtype(a0 + dtype(lm_dtype(lmw * q)))
                    nacc = F32(acc + F32(lm.score(lm.history(hist), c, F32)))
                    if v.children:
                        made.append((0, a, hyp + ((c, None),), v, words, hist + (c,), nacc))
                    for i, w in enumerate(v.words):
                        made.append((1 + i, dtype(a + dtype(wsc)), hyp + ((c, w),), root, words + (w,), hist + (c,), nacc))
                    d.homophones += len(v.words) if len(v.words) >= 2 else 0
                for slot, val, nh, nu, nwords, nhist, nacc in made:
                    j = index.get(nh)
                    if j is not None:
                        stay[j][1] = _oplus(stay[j][1], val, log_add)
                        d.merges += 1
                    else:
                        exts.append((val, r, 1, k, slot, nh, ninf, val, nu, nwords, nhist, nacc))
        cands = [(_oplus(s[0], s[1], log_add), r, 0, 0, 0, beam[r][0], s[0], s[1]) + beam[r][4:] for r, s in enumerate(stay)]
        cands = [c for c in cands + exts if c[0] != -np.inf]
        if not cands:
            beam = []
            break
        best = max(c[0] for c in cands)
        line = dtype(best - thr)
        d.S = max(d.S, max(abs(float(c[0])) for c in cands))
        if np.isfinite(threshold):
            d.threshold_gap = min(d.threshold_gap, min(abs(float(c[0] - line)) for c in cands))
        cands = [c for c in cands if not c[0] < line]
        cands.sort(key=lambda c: (-c[0], c[1], c[2], c[3], c[4]))
        first_dropped = float(cands[W][0]) if len(cands) > W else -np.inf
        if len(cands) > W:
            d.beam_gap = min(d.beam_gap, float(cands[W - 1][0]) - first_dropped)
        floor = max(first_dropped, float(line))
        kept = cands[:W]
        last_kept = float(kept[-1][0]) if len(cands) >= W else -np.inf
        d.removed += sum(1 for v in blocked if v >= last_kept and not v < line and v != -np.inf)
        d.slot_ties += sum(1 for i in range(min(W, len(cands) - 1)) if cands[i][:4] == cands[i + 1][:4] and cands[i][2] == 1)
        d.sil_loops += sum(1 for c in kept if c[2] == 1 and c[5][-1] == (trie.sil, None) and c[8] is root)
        beam = [(c[5], c[6], c[7], min(beam[c[1]][3], float(c[0]) - floor)) + c[8:] for c in kept]
    out = []
    d.end_dropped = sum(1 for en in beam if en[4] is not root)
    d.end_changed_best = bool(beam) and beam[0][4] is not root
    for r, (hyp, pb, pnb, mg, u, words, hist, acc) in enumerate(beam):
        if u is not root:
            continue                                             # only finished words count at the end
        s = _oplus(pb, pnb, log_add)
        if lm.has_eos:
            ge = lm_dtype(lm_dtype(lmw * lm.score(lm.history(hist), lm.eos, lm_dtype)) + lm_dtype(eos_score))
            s = dtype(s + dtype(ge))
            acc = F32(acc + F32(lm.score(lm.history(hist), lm.eos, F32)))
        else:
            assert eos_score == 0
        out.append((hyp, s, mg, r, words, acc))
    ranked = sorted(out, key=lambda o: (-o[1], o[3]))
    d.eos_moves = sum(1 for i, o in enumerate(ranked) if o[3] != out[i][3])
    d.S = max([d.S] + [abs(float(o[1])) for o in ranked if np.isfinite(o[1])])
    m_out = len(ranked) if M is None else min(M, len(ranked))
    d.final_gaps = [float(ranked[m][1] - ranked[m + 1][1]) for m in range(min(m_out, len(ranked) - 1))]
    d.margins = [o[2] for o in ranked[:m_out]]
    return [(tuple(c for c, _ in o[0]), o[4], o[1], o[5], o[0]) for o in ranked[:m_out]], d


def lextok_beam(x, frames, W, K, M, Lmax, trie, lm, lm_weight, word_score=0.0, eos_score=0.0, dtype=F32, max_words=None, **kw):
    """the C ABI's outputs as a dict: labels [B][M][Lmax], lengths, scores (dtype), lm_scores float32, words [B][M][max_words],
    word_counts; diags"""
    x = np.asarray(x, F32)
    B, T, _ = x.shape
    max_words = Lmax if max_words is None else max_words
    o = dict(labels=np.full((B, M, Lmax), -1, np.int32), lengths=np.full((B, M), -1, np.int32),
             scores=np.full((B, M), -np.inf, dtype), lm_scores=np.full((B, M), -np.inf, F32),
             words=np.full((B, M, max_words), -1, np.int32), word_counts=np.full((B, M), -1, np.int32), diags=[])
    for b in range(B):
        F = T if frames is None else int(frames[b])
        hyps, dg = lextok_beam_one(x[b], F, W, K, trie, lm, lm_weight, word_score, eos_score, dtype=dtype, M=M, **kw)
        o["diags"].append(dg)
        for m, (p, ws, s, ls, _) in enumerate(hyps):
            o["lengths"][b, m] = len(p)
            o["labels"][b, m, :min(len(p), Lmax)] = p[:Lmax]
            o["scores"][b, m] = s
            o["lm_scores"][b, m] = ls
            o["word_counts"][b, m] = len(ws)
            o["words"][b, m, :min(len(ws), max_words)] = ws[:max_words]
    return o


def enumerate_lextok(x, trie, lm, lm_weight, word_score, eos_score, log_add, normalize, A=None):
    """every one of the N^T paths, collapsed, every collapsed labelling expanded into every (segmentation, homophone choice) the
    lexicon allows: {hypothesis: score} in float64, the tokens scored by the textbook LM.  A: the ASG lattice (asg_beam_ref's
    enumeration of labellings)"""
    if A is None:
        from tests.ctc_beam_ref import enumerate_labellings
        labellings = enumerate_labellings(x, log_add, normalize)
    else:
        from tests.asg_beam_ref import enumerate_labellings
        labellings = enumerate_labellings(x, A, log_add, normalize)
    out = {}
    for lab, s in labellings.items():
        for hyp in trie.derivations(lab):
            toks = lm_history(hyp, trie.sil)
            hist = lm.history(())
            q = 0.0
            for c in toks:
                q += float(lm.score(hist, c, np.float64))
                hist = hist + (c,)
            total = s + lm_weight * q + word_score * sum(1 for _, w in hyp if w is not None)
            if lm.has_eos:
                total += lm_weight * float(lm.score(hist, lm.eos, np.float64)) + eos_score
            out[hyp] = total
    return out
