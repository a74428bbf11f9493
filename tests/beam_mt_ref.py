"""The numpy restatements of the five beam searches with the counts the many-token tests need (w2l_*_beam_search*_mt, K up to 256;
include/w2l_hip.h), shared by test_beam_mt_host.py and test_gpu_beam_mt.py.

The restatements of tests/ (ctc_beam_ref, ctc_beam_lm_ref, ctc_beam_lex_ref, asg_beam_ref, beam_sil_ref) carry no cap on K and are
not touched.  What they do not return is WHERE in the token order a frame's decisions fell: the many-token scan keeps a gone mask
of ceil(K / 64) words per (slot, entry) and a tie key with 8 bits of k, so a test of it has to know, from the CPU alone, that
extensions merged in every mask word and that selections were decided by k on both sides of a 64-boundary.  mt_beam_one is
beam_sil_ref.sil_beam_one, statement for statement, with those counts added (MtDiag); test_beam_mt_host.py holds its outputs to
sil_beam_one's on every kind, so the counts describe the search the other restatements describe.

The counts, per utterance:
  merges[slot > 0][k >> 6]   extensions (r, k, slot) that spelled a prefix the beam holds and joined its stay, by mask word, the
                             lexicon's word slots (slot >= 1) apart from slot 0
  tie_high                   pairs of extensions with k >= 64 and EQUAL totals that follow one another (among those with k >= 64) in
                             a frame's final order, the first of the pair selected (rank < W): the tie key alone -- r, then k in
                             its upper bits -- put the selected one first
  tie_cross                  neighbours in that order with equal totals, the first selected, both extensions of one entry r, whose
                             k lie in different mask words (k >> 6 differs): decided by k across a 64-boundary
  tokens[t]                  the frame tokens in the contract's order (classes)"""
import numpy as np

from tests.ctc_beam_ref import Diag, _oplus, frame_scores

F32 = np.float32


class MtDiag(Diag):
    def __init__(self):
        super().__init__()
        self.merges = [[0, 0, 0, 0], [0, 0, 0, 0]]
        self.tie_high = 0
        self.tie_cross = 0
        self.tokens = []
        self.end_dropped = 0


def mt_beam_one(x, F, W, K, sil=-1, sil_score=0.0, A=None, lm=None, trie=None, lm_weight=0.0, class_score=None, word_score=0.0,
                eos_score=0.0, threshold=np.inf, log_add=False, normalize=False, dtype=F32, M=None, lm_dtype=F32):
    """sil_beam_one's arguments and first return value; the second is an MtDiag"""
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
    d = MtDiag()
    root = trie.root if trie is not None else None

    def g_of(prefix, c):
        g = lm_dtype(lmw * lm.score(lm.history(prefix), c, lm_dtype))
        if class_score is not None:
            g = lm_dtype(g + lm_dtype(class_score[c]))
        return g

    beam = [((), dtype(0), ninf, np.inf, root, ())]
    for t in range(F):
        ac = lp_all[t]
        order = np.lexsort((np.arange(ntok), -ac[:ntok]))        # the ACOUSTIC lp descending, class ascending
        toks = [int(c) for c in order[:K]]
        d.tokens.append(toks)
        if K < ntok:
            d.token_gap = min(d.token_gap, float(ac[order[K - 1]] - ac[order[K]]))
        lp = ac.copy()
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
                        d.merges[1 if slot > 0 else 0][k >> 6] += 1
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
        i = 0
        while i < min(W, len(cands)):                             # the groups of equal totals that begin among the selected
            j = i
            high = -1                                            # the last extension of the group with k >= 64
            while j < len(cands) and cands[j][0] == cands[i][0]:
                a = cands[j]
                if a[2] == 1 and a[3] >= 64:
                    if 0 <= high < W:
                        d.tie_high += 1
                    high = j
                if j > i and j - 1 < W and a[2] == 1 and cands[j - 1][2] == 1 and a[1] == cands[j - 1][1] and (a[3] >> 6) != (cands[j - 1][3] >> 6):
                    d.tie_cross += 1
                j += 1
            i = j
        first_dropped = float(cands[W][0]) if len(cands) > W else -np.inf
        if len(cands) > W:
            d.beam_gap = min(d.beam_gap, float(cands[W - 1][0]) - first_dropped)
        floor = max(first_dropped, float(line))
        beam = [(c[5], c[6], c[7], min(beam[c[1]][3], float(c[0]) - floor), c[8], c[9]) for c in cands[:W]]
    out = []
    for r, (hyp, pb, pnb, mg, u, words) in enumerate(beam):
        if u is not root:
            d.end_dropped += 1
            continue                                             # only finished words count at the end
        s = _oplus(pb, pnb, log_add)
        if lm is not None and lm.has_eos:
            hist = words if trie is not None else tuple(c for c, _ in hyp)
            ge = lm_dtype(lm_dtype(lmw * lm.score(lm.history(hist), lm.eos, lm_dtype)) + lm_dtype(eos_score))
            s = dtype(s + dtype(ge))
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


def mt_beam(x, frames, W, K, M, Lmax, sil=-1, sil_score=0.0, dtype=F32, max_words=None, **kw):
    """beam_sil_ref.sil_beam's dict (labels, lengths, scores, lm_scores, with a trie words and word_counts; diags: MtDiags)"""
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
        hyps, dg = mt_beam_one(x[b], F, W, K, sil, sil_score, dtype=dtype, M=M, **kw)
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


def case_ref(c, W, K, M, Lmax, dtype=F32, threshold=np.inf, log_add=False, normalize=False, max_words=None, sil=-1, sil_score=0.0):
    """mt_beam for a tests.test_gpu_beam_wide.Case-like object (kind, x, frames, A, tb, trie, cls, lmw, wsc, eos), with the keys the
    kind's entry point does not return removed"""
    kw = dict(threshold=threshold, log_add=log_add, normalize=normalize)
    if c.A is not None:
        kw["A"] = c.A
    if c.tb is not None:
        kw.update(lm=c.tb, lm_weight=c.lmw, eos_score=c.eos)
    if c.trie is not None:
        kw.update(trie=c.trie, word_score=c.wsc)
    elif c.cls is not None:
        kw.update(class_score=c.cls)
    o = mt_beam(c.x, c.frames, W, K, M, Lmax, sil, sil_score, dtype, max_words, **kw)
    if c.tb is None:
        del o["lm_scores"]
    return o


# ---- the cases whose restatement is too slow to run with the suite: inputs from a seed, outputs as digests ---------------------
# tests/golden/beam_mt_golden.json holds, per case, the SHA-256 of every output array of the float32 restatement (M = W rows, so a
# digest speaks for every row the search returns), the digest of the inputs the seed gave (a numpy whose streams differ fails
# there, not in a kernel's name) and the counts above.  tests/golden/make_beam_mt_golden.py writes it: minutes on the CPU.

KINDS = ("ctc", "ctc_lm", "ctc_lex", "asg", "asg_lm", "asg_lex")
KEYS = ("labels", "lengths", "scores", "lm_scores", "words", "word_counts")
M2_K = (65, 100, 128, 129, 192, 193, 256)          # every mask-word boundary from both sides, and the recipes' 100
M2_W = (200, 1500)
M2_SHAPE = (300, 10, 3, (10, 4, 7))                 # N, T, B, frames: K binds (256 < N - 1)
M3_SHAPE = (300, 3, 1, 256, 8192)                   # N, T, B, K, W
GOLDEN = "beam_mt_golden.json"


def digest(a):
    import hashlib
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.view(np.uint8).tobytes()).hexdigest()


def digests(o):
    return {k: digest(o[k]) for k in KEYS if k in o}


def input_digest(c):
    parts = [c.x] + ([c.A] if c.A is not None else []) + ([c.cls] if c.cls is not None else [])
    return digest(np.concatenate([np.asarray(p, F32).ravel() for p in parts]))


def m2_case(kind):
    """dense ties on N = 300 classes: tests.test_gpu_beam_wide._dense_case (LM and transition values of 1/8: every fp32 sum exact)
    with its emissions, multiples of 1/4 in [-3, 0], coarsened to the two values 0 and -1/2 (the classes a lexicon has no letters
    for: -1 to -2): more than a hundred classes share a frame's best score, so the tokens around rank 64 tie with one another and
    with the best, and entries tie in their totals -- selections are decided by r and k on both sides of the first mask-word
    boundary even at K = 65.  260 letters under the lexicon, so that tokens of every mask word have trie edges"""
    from tests.test_gpu_beam_wide import _dense_case
    N, T, B, frames = M2_SHAPE
    c = _dense_case(kind, 500 + KINDS.index(kind), B, T, N, list(frames), hot=260, nwords=3000, max_len=2)
    c.x = (np.ceil(c.x / 1.5) / 2).astype(F32)
    return c


def m2_facts(diags):
    return dict(tie_high=sum(d.tie_high for d in diags), tie_cross=sum(d.tie_cross for d in diags),
                merges=[[sum(d.merges[s][w] for d in diags) for w in range(4)] for s in range(2)])


def m3_case(kind):
    """three frames whose rankings are permutations of one another, with distinct scores on a grid of 1/4: class i < 256 has rank
    i at frame 0 and (i + 64) mod 256 at frame 1; at frame 2 the classes 192..255, the best of frame 1, have the ranks 64, 67, ..,
    253 and the others fill the rest in class order.  With W = 8192 every one-token prefix of frame 0 is in the beam at frame 1,
    where (CTC) the root's extension by it merges into its stay, in mask word (rank at frame 1) >> 6: the classes 0..191 merge in
    the three upper words.  ASG has no root after frame 0: there the two-token prefixes that end in a class of 192..255 are in the
    beam at frame 2 with their parents, and the parents' extensions by those classes merge in the words their ranks 64..253 lie in.
    Under a lexicon every token is a one-token word (its word slot merges the same way), the first 50 have a homophone, and every
    token begins two-token words"""
    from tests import ctc_beam_lex_ref as XR
    from tests import ctc_beam_lm_ref as LR
    from tests.test_gpu_beam_wide import Case, _quarters, _smear
    N, T, B, K, W = M3_SHAPE
    rng = np.random.default_rng(800 + KINDS.index(kind))
    asg = kind.startswith("asg")
    tokens = N if asg else N - 1
    x = np.zeros((B, T, N), F32)
    for t in range(T):
        rank = np.arange(tokens)
        if t == 1:
            rank[:256] = (np.arange(256) + 64) % 256
        if t == 2:
            best = 64 + 3 * np.arange(64)
            rank[192:256] = best
            rank[:192] = np.setdiff1d(np.arange(256), best)
        x[:, t, :tokens] = (-rank / 4).astype(F32)
    if not asg:
        x[:, :, N - 1] = -1.0
    A = (rng.integers(-8, 9, size=(N, N)) / 8).astype(F32) if asg else None
    if kind.endswith("lex"):
        rows = [(c, [c]) for c in range(tokens)] + [(tokens + c, [c, (7 * c + 3) % tokens]) for c in range(tokens)]
        rows += [(2 * tokens + c, [c]) for c in range(50)]
        nwords = 2 * tokens + 50
        tb = LR.random_lm(rng, nwords, 3, 2 * nwords, True, True, (), eighths=True)
        trie = XR.TextbookTrie(rows, tokens, nwords, _smear(tb, nwords), None)
        return Case(kind, x, None, A, tb, trie, None, 0.5, -0.25, -0.25)
    if kind.endswith("lm"):
        tb = LR.random_lm(rng, tokens, 3, 40 * tokens, True, True, (), eighths=True)
        return Case(kind, x, None, A, tb, None, _quarters(rng, (tokens,), -1, 0), 0.5, 0.0, -0.25)
    return Case(kind, x, None, A)


def golden():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)) as f:
        return json.load(f)
