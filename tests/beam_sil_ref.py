"""numpy restatement of the silence score of the five beam searches (w2l_*_beam_search*_sil; include/w2l_hip.h), shared by
test_beam_sil_host.py, test_gpu_beam_sil.py and test_gpu_beam_sil_containment.py.

The rule: the frame tokens of a frame, their order and the tie key's k are those of the acoustic lp alone; AFTER they have been
chosen, lp[sil] is replaced by lp[sil] + silScore (one add in the search's dtype), and every later use of lp[sil] -- the stay of an
entry that ends in sil, every extension by sil (in the lexicon searches the root's sil slot and any trie edge on that token), the
merged term, thresholds, totals, keys -- reads that value.

sil_beam_one restates all five searches with that rule, written out in full: `A` (a transition matrix) chooses the ASG lattice
over the CTC one, `trie` the lexicon search, else `lm` the token-LM search, else the LM-free one.  Everything but the rule is the
contract restated in ctc_beam_ref, ctc_beam_lm_ref, ctc_beam_lex_ref and asg_beam_ref, whose helpers, LM and trie classes it uses;
with sil_score = 0 it returns what those return (test_beam_sil_host.py holds it to them).  dtype = float32 reproduces the kernels
bit for bit when logAdd = 0; dtype = float64 is the reference for logAdd = 1."""
import numpy as np

from tests.ctc_beam_ref import Diag, _oplus, frame_scores

F32 = np.float32


def bias_column(x, sil, sil_score):
    """the emissions with sil_score added to column sil on the host in fp32: I2's other side"""
    x = np.array(x, F32, copy=True)
    x[..., sil] = x[..., sil] + F32(sil_score)
    return x


def sil_beam_one(x, F, W, K, sil=-1, sil_score=0.0, A=None, lm=None, trie=None, lm_weight=0.0, class_score=None, word_score=0.0,
                 eos_score=0.0, threshold=np.inf, log_add=False, normalize=False, dtype=F32, M=None, lm_dtype=F32):
    """x [T][N] float32 -> ([(labels, words, score, lm score, hypothesis)] in rank order, Diag).  A hypothesis is the tuple of its
    extensions (token, word or None); without a lexicon every word is None.  sil = -1: no silence score"""
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
    d = Diag()
    root = trie.root if trie is not None else None
    if trie is None and lm is None:
        assert lm_weight == 0 and class_score is None and eos_score == 0

    def g_of(prefix, c):
        g = lm_dtype(lmw * lm.score(lm.history(prefix), c, lm_dtype))
        if class_score is not None:
            g = lm_dtype(g + lm_dtype(class_score[c]))
        return g

    # entry: hypothesis, pb, pnb, lineage margin, lexicon node, words.  ASG: one value p = pnb, pb = -inf (the empty prefix: pb = 0)
    beam = [((), dtype(0), ninf, np.inf, root, ())]
    for t in range(F):
        ac = lp_all[t]
        order = np.lexsort((np.arange(ntok), -ac[:ntok]))        # the ACOUSTIC lp descending, class ascending
        toks = [int(c) for c in order[:K]]
        if K < ntok:
            d.token_gap = min(d.token_gap, float(ac[order[K - 1]] - ac[order[K]]))
        lp = ac.copy()                                            # ... and only now the silence score
        if sil >= 0:
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
        exts = []
        for r, (hyp, pb, pnb, _, u, words) in enumerate(beam):
            e = hyp[-1][0] if hyp else -1
            for k, c in enumerate(toks):
                if asg:
                    if c == e:
                        continue
                    a0 = lp[c] if not hyp else dtype(dtype(tots[r] + A[c, e]) + lp[c])
                else:
                    a0 = dtype(lp[c] + (pb if c == e else tots[r]))
                made = []                                        # (slot, value, hypothesis, node, words)
                if trie is not None:
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
                elif lm is not None:
                    made.append((0, dtype(a0 + dtype(g_of(tuple(cc for cc, _ in hyp), c))), hyp + ((c, None),), None, ()))
                else:
                    made.append((0, a0, hyp + ((c, None),), None, ()))
                for slot, val, nh, nu, nwords in made:
                    j = index.get(nh)
                    if j is not None:
                        stay[j][1] = _oplus(stay[j][1], val, log_add)
                    else:
                        exts.append((val, r, 1, k, slot, nh, ninf, val, nu, nwords))
        cands = [(_oplus(s[0], s[1], log_add), r, 0, 0, 0, beam[r][0], s[0], s[1], beam[r][4], beam[r][5]) for r, s in enumerate(stay)]
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
        beam = [(c[5], c[6], c[7], min(beam[c[1]][3], float(c[0]) - floor), c[8], c[9]) for c in cands[:W]]
    out = []
    for r, (hyp, pb, pnb, mg, u, words) in enumerate(beam):
        if u is not root:
            continue                                             # only finished words count at the end
        s = _oplus(pb, pnb, log_add)
        if lm is not None and lm.has_eos:
            hist = words if trie is not None else tuple(c for c, _ in hyp)
            ge = lm_dtype(lm_dtype(lmw * lm.score(lm.history(hist), lm.eos, lm_dtype)) + lm_dtype(eos_score))
            s = dtype(s + dtype(ge))
        else:
            assert eos_score == 0
        out.append((hyp, s, mg, r, words))
    ranked = sorted(out, key=lambda o: (-o[1], o[3]))
    d.S = max([d.S] + [abs(float(o[1])) for o in ranked if np.isfinite(o[1])])
    m_out = len(ranked) if M is None else min(M, len(ranked))
    d.final_gaps = [float(ranked[m][1] - ranked[m + 1][1]) for m in range(min(m_out, len(ranked) - 1))]
    d.margins = [o[2] for o in ranked[:m_out]]
    res = []
    for hyp, s, _, _, words in ranked[:m_out]:
        labels = tuple(c for c, _ in hyp)
        lms = F32(0) if lm is None else lm.sentence(words if trie is not None else labels, F32)
        res.append((labels, words, s, lms, hyp))
    return res, d


def sil_beam(x, frames, W, K, M, Lmax, sil=-1, sil_score=0.0, dtype=F32, max_words=None, **kw):
    """the C ABI's outputs as a dict: labels [B][M][Lmax], lengths, scores (dtype), lm_scores float32 (the LM-free CTC search has no
    such output: ignore it there), with a trie also words [B][M][max_words] and word_counts; diags"""
    x = np.asarray(x, F32)
    B, T, _ = x.shape
    trie = kw.get("trie")
    o = dict(labels=np.full((B, M, Lmax), -1, np.int32), lengths=np.full((B, M), -1, np.int32),
             scores=np.full((B, M), -np.inf, dtype), lm_scores=np.full((B, M), -np.inf, F32), diags=[])
    if trie is not None:
        max_words = Lmax if max_words is None else max_words
        o["words"] = np.full((B, M, max_words), -1, np.int32)
        o["word_counts"] = np.full((B, M), -1, np.int32)
    for b in range(B):
        F = T if frames is None else int(frames[b])
        hyps, dg = sil_beam_one(x[b], F, W, K, sil, sil_score, dtype=dtype, M=M, **kw)
        o["diags"].append(dg)
        for m, (p, ws, s, ls, _) in enumerate(hyps):
            o["lengths"][b, m] = len(p)
            o["labels"][b, m, :min(len(p), Lmax)] = p[:Lmax]
            o["scores"][b, m] = s
            o["lm_scores"][b, m] = ls
            if trie is not None:
                o["word_counts"][b, m] = len(ws)
                o["words"][b, m, :min(len(ws), max_words)] = ws[:max_words]
    return o


def selection_case(rng, B, T, N, sil, ntok):
    """emissions (multiples of 1/8, so every fp32 sum is exact) in which the silence class is acoustically LAST among the tokens in
    the even frames and FIRST in the odd ones, by a margin of 1: with K below the token count, biasing by +8 before selection
    would bring sil into the even frames' tokens, biasing by -8 before selection would push it out of the odd frames'"""
    x = (rng.integers(-24, 1, size=(B, T, N)) / 8).astype(F32)
    x[:, 0::2, sil] = x[:, 0::2, :ntok].min(axis=-1) - 1
    x[:, 1::2, sil] = x[:, 1::2, :ntok].max(axis=-1) + 1
    return x
