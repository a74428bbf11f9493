"""numpy restatement of w2l_lexicon_* and w2l_ctc_beam_search_lex's contracts (include/w2l_hip.h), shared by
test_ctc_beam_lex_host.py and test_gpu_ctc_beam_lex.py.

TextbookTrie is the textbook dict-of-dicts trie over spelling rows: a node is a dictionary of children, the words whose spelling
ends there in row order, and the max of the word smear values over the words KEPT (the first six of a node) at or below.  It knows
nothing of node numbers, hash tables or blobs: the library's table is held to it node for node.

beam_search_lex_one is ctc_beam_lm_ref.beam_search_lm_one with the lexicon terms of the contract.  A hypothesis is the tuple of its
extensions (token, word or None); its lexicon node, word list and LM history are functions of it."""
import numpy as np

from tests.ctc_beam_ref import Diag, _oplus, frame_scores

F32 = np.float32
MAX_WORDS = 6


class TrieNode:
    def __init__(self):
        self.children = {}       # token -> TrieNode, in the order the rows first reach them
        self.all_words = []      # every word whose spelling ends here, row order
        self.smear = F32(0)

    @property
    def words(self):
        return self.all_words[:MAX_WORDS]


class TextbookTrie:
    """rows: [(word id, [token ids])]; word_smear: {word: value} / array or None (all 0); sil: the silence token or None"""

    def __init__(self, rows, num_tokens, num_words, word_smear=None, sil=None):
        self.rows = [(int(w), [int(t) for t in sp]) for w, sp in rows]
        self.num_tokens, self.num_words, self.sil = num_tokens, num_words, sil
        self.word_smear = None if word_smear is None else np.asarray(word_smear, F32)
        self.root = TrieNode()
        self.dropped = 0
        for w, sp in self.rows:
            u = self.root
            for t in sp:
                u = u.children.setdefault(t, TrieNode())
            u.all_words.append(w)
            self.dropped += len(u.all_words) > MAX_WORDS
        self._smear(self.root)

    def _smear(self, u):
        vals = [F32(0) if self.word_smear is None else self.word_smear[w] for w in u.words]
        vals += [self._smear(c) for c in u.children.values()]
        u.smear = F32(max(vals)) if vals else F32(0)
        return u.smear

    def nodes(self):
        """every node with the token path that reaches it, the root first"""
        out, todo = [], [((), self.root)]
        while todo:
            path, u = todo.pop()
            out.append((path, u))
            todo += [(path + (t,), c) for t, c in u.children.items()]
        return out

    def derivations(self, labels):
        """every hypothesis (tuple of (token, word or None)) that spells `labels` and ends at the root"""
        out = []

        def walk(i, u, hyp):
            if i == len(labels):
                if u is self.root:
                    out.append(hyp)
                return
            c = labels[i]
            if c == self.sil and u is self.root:
                walk(i + 1, u, hyp + ((c, None),))
                return
            v = u.children.get(c)
            if v is None:
                return
            if v.children:
                walk(i + 1, v, hyp + ((c, None),))
            for w in v.words:
                walk(i + 1, self.root, hyp + ((c, w),))
        walk(0, self.root, ())
        return out


class LexDiag(Diag):
    """Diag, and what shows that a case exercises the lexicon paths.  blocked: (entry, frame token) pairs without a lexicon edge.
    removed: those among them whose acoustic total lp + base alone reached the frame's last kept total and the threshold line, so a
    search without the lexicon constraint -- whose LM term is a bonus or penalty on top -- had the candidate in reach of its beam.
    merges: candidates merged into a stay.  homophones: word candidates made at a node with two words or more.  sil_loops: silence
    extensions at the root that entered a beam.  slot_ties: adjacent candidates in selection order, the first of them kept, that
    differ in nothing but the slot.  end_dropped: entries inside a word at the end.  end_changed_best: the entry of rank 0 was one
    of them.  eos_moves as in LmDiag."""

    def __init__(self):
        super().__init__()
        self.blocked = self.removed = self.merges = self.homophones = self.sil_loops = self.slot_ties = 0
        self.end_dropped = self.eos_moves = 0
        self.end_changed_best = False


def beam_search_lex_one(x, F, W, K, trie, lm, lm_weight, word_score=0.0, eos_score=0.0, threshold=np.inf, log_add=False,
                        normalize=False, dtype=F32, M=None, lm_dtype=F32):
    """x [T][N] float32 -> ([(labels tuple, words tuple, score, lm score)] in rank order, LexDiag).  lm_dtype: the precision of
    the smear, q and word-score terms (float32: the contract's; float64: for the comparison with the enumeration)"""
    lp_all = frame_scores(np.asarray(x)[:F], normalize, dtype)
    N = lp_all.shape[1]
    blank = N - 1
    K = min(K, N - 1)
    ninf = dtype(-np.inf)
    thr = dtype(threshold)
    lmw, wsc = lm_dtype(lm_weight), lm_dtype(word_score)
    d = LexDiag()
    root = trie.root
    # entry: hypothesis, pb, pnb, lineage margin, lexicon node, words
    beam = [((), dtype(0), ninf, np.inf, root, ())]
    for t in range(F):
        lp = lp_all[t]
        nb = lp[:blank]
        order = np.lexsort((np.arange(blank), -nb))
        toks = [int(c) for c in order[:K]]
        if K < blank:
            d.token_gap = min(d.token_gap, float(nb[order[K - 1]] - nb[order[K]]))
        index = {en[0]: j for j, en in enumerate(beam)}
        tots = [_oplus(en[1], en[2], log_add) for en in beam]
        stay = [[lp[blank] + tots[r], (lp[en[0][-1][0]] + en[2]) if en[0] else ninf] for r, en in enumerate(beam)]
        exts, blocked = [], []
        for r, (hyp, pb, pnb, _, u, words) in enumerate(beam):
            e = hyp[-1][0] if hyp else -1
            for k, c in enumerate(toks):
                acoustic = dtype(lp[c] + (pb if c == e else tots[r]))
                made = []                                        # (slot, value, hypothesis, node, words)
                if c == trie.sil and u is root:
                    made.append((0, acoustic, hyp + ((c, None),), root, words))
                else:
                    v = u.children.get(c)
                    if v is None:
                        d.blocked += 1
                        blocked.append(acoustic)
                        continue
                    su = lm_dtype(0) if u is root else lm_dtype(u.smear)
                    smv = lm_dtype(v.smear)
                    a = dtype(acoustic + dtype(lm_dtype(lmw * lm_dtype(smv - su))))
                    if v.children:
                        made.append((0, a, hyp + ((c, None),), v, words))
                    for i, w in enumerate(v.words):
                        q = lm.score(lm.history(words), w, lm_dtype)
                        val = dtype(a + dtype(lm_dtype(lm_dtype(lmw * lm_dtype(q - smv)) + wsc)))
                        made.append((1 + i, val, hyp + ((c, w),), root, words + (w,)))
                    d.homophones += len(v.words) if len(v.words) >= 2 else 0
                for slot, val, nh, nu, nwords in made:
                    j = index.get(nh)
                    if j is not None:
                        stay[j][1] = _oplus(stay[j][1], val, log_add)
                        d.merges += 1
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
        kept = cands[:W]
        last_kept = float(kept[-1][0]) if len(cands) >= W else -np.inf
        d.removed += sum(1 for ac in blocked if ac >= last_kept and not ac < line and ac != -np.inf)
        d.slot_ties += sum(1 for i in range(min(W, len(cands) - 1)) if cands[i][:4] == cands[i + 1][:4] and cands[i][2] == 1)
        d.sil_loops += sum(1 for c in kept if c[2] == 1 and c[5][-1] == (trie.sil, None) and c[8] is root)
        beam = [(c[5], c[6], c[7], min(beam[c[1]][3], float(c[0]) - floor), c[8], c[9]) for c in kept]
    out = []
    d.end_dropped = sum(1 for en in beam if en[4] is not root)
    d.end_changed_best = bool(beam) and beam[0][4] is not root
    for r, (hyp, pb, pnb, mg, u, words) in enumerate(beam):
        if u is not root:
            continue
        s = _oplus(pb, pnb, log_add)
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


def beam_search_lex(x, frames, W, K, trie, lm, lm_weight, word_score, eos_score, threshold, log_add, normalize, M, Lmax, max_words,
                    dtype, lm_dtype=F32):
    """the C ABI's outputs: labels [B][M][Lmax], lengths [B][M], scores [B][M] (dtype), lm_scores [B][M] float32, words
    [B][M][max_words], word_counts [B][M], the LexDiags"""
    x = np.asarray(x, F32)
    B, T, _ = x.shape
    labels = np.full((B, M, Lmax), -1, np.int32)
    lengths = np.full((B, M), -1, np.int32)
    scores = np.full((B, M), -np.inf, dtype)
    lm_scores = np.full((B, M), -np.inf, F32)
    words = np.full((B, M, max_words), -1, np.int32)
    counts = np.full((B, M), -1, np.int32)
    diags = []
    for b in range(B):
        F = T if frames is None else int(frames[b])
        hyps, dg = beam_search_lex_one(x[b], F, W, K, trie, lm, lm_weight, word_score, eos_score, threshold, log_add, normalize,
                                       dtype, M, lm_dtype)
        diags.append(dg)
        for m, (p, ws, s, ls, _) in enumerate(hyps):
            lengths[b, m] = len(p)
            labels[b, m, :min(len(p), Lmax)] = p[:Lmax]
            counts[b, m] = len(ws)
            words[b, m, :min(len(ws), max_words)] = ws[:max_words]
            scores[b, m] = s
            lm_scores[b, m] = ls
    return labels, lengths, scores, lm_scores, words, counts, diags


def delta_lex(T, S):
    """ctc_beam_lm_ref.delta_lm with the three further dependent fp32 roundings an extension of this contract has on the way from
    lp + base to pnb' (the add of the smear term, the add of the word term, and the sum inside the word term); the smear and word
    terms themselves are fp32 on both sides"""
    return 2.0 * T * (8.0 * 2.0 ** -24 * max(1.0, S) + 4e-6)


def enumerate_hypotheses(x, trie, lm, lm_weight, word_score, eos_score, log_add, normalize):
    """every one of the N^T paths, collapsed, every collapsed labelling expanded into every (segmentation, homophone choice) the
    lexicon allows: {hypothesis: score} in float64, scored by the textbook LM"""
    from tests.ctc_beam_ref import enumerate_labellings
    out = {}
    for lab, s in enumerate_labellings(x, log_add, normalize).items():
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


def random_lexicon(rng, num_tokens, num_words, max_len=4, homophones=0.0, sil=None, hot=None, crowd=0, min_len=1):
    """rows [(word, spelling)]: distinct random spellings of min_len .. max_len tokens (of the first `hot` tokens, never beginning with
    `sil`), a fraction `homophones` of the words sharing the spelling of an earlier word, and `crowd` words (the last ones) all on
    the spelling of word 0: more than six of them show the cap"""
    toks = num_tokens if hot is None else min(hot, num_tokens)
    rows, seen = [], set()
    for w in range(num_words - crowd):
        if rows and rng.random() < homophones:
            rows.append((w, list(rows[int(rng.integers(len(rows)))][1])))
            continue
        for _ in range(1000):
            sp = tuple(int(t) for t in rng.integers(0, toks, int(rng.integers(min_len, max_len + 1))))
            if sp[0] != sil and sp not in seen:
                break
        seen.add(sp)
        rows.append((w, list(sp)))
    rows += [(w, list(rows[0][1])) for w in range(num_words - crowd, num_words)]
    return rows
