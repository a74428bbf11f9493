"""The token LM under a lexicon (w2l_ctc_beam_search_lextok, w2l_asg_beam_search_lextok) on the GPU, narrow and wide, against
tests/beam_lextok_ref.py and against the siblings.
K1 dyadic values, logAdd = 0: every output bit-equal to the float32 restatement, both lattices, every W and K of the lists below;
K2 dense ties (emissions of four dyadic values), slot order among homophones included; K3 identity with the token-LM search on a
lexicon of one-token words; K4 identity with the word search at lmWeight = 0; K5 logAdd = 1 on normalised rows against the float64
restatement where its decisions have a margin; K6 narrow == wide at every W <= 64; K7 the silence score; K8 ASG with zero
transitions == CTC with a -inf blank column.  (K9, the three surfaces: tests/test_gpu_beam_lextok_surfaces.py.)
Shapes: B = 3 with ragged frames, T = 24, CTC N = 9 (8 tokens and blank) / ASG N = 8, sil = token 2, a lexicon of 30 words with a
homophone pair, a word that is a prefix of another, a spelling that ends on sil and one-token words; a 3-gram token LM with missing
n-grams (back-off walks) and token 1 without a unigram (scored as <unk>)."""
import functools

import numpy as np
import pytest
import torch

from tests import beam_lextok_ref as TR
from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR
from tests.test_gpu_beam_wide import F32, INF, KEYS, Case, _lex_table, _lm_table, _same_bits
from tests.test_gpu_ctc_beam import _close

pytestmark = pytest.mark.gpu
SIL, UNK = 2, 1
B, T, FRAMES = 3, 24, [24, 1, 17]
NWORDS = 30
WIDTHS = [(0, 1), (0, 2), (0, 7), (0, 64), (1, 65), (1, 200), (1, 1024)]     # (family, W)
ENTRY = {False: "w2l_ctc_beam", True: "w2l_asg_beam"}


def classes(asg):
    return 8 if asg else 9


def lexicon_rows(rng, ntok, nwords=NWORDS):
    """random words of 1 to 3 tokens, then a homophone of word 0, a word that continues word 1's spelling, a spelling that ends on
    sil, and a one-token word"""
    rows = XR.random_lexicon(rng, ntok, nwords - 4, 3, 0.0, SIL)
    have = {tuple(sp) for _, sp in rows}
    cont = next(t for t in range(ntok) if t != rows[1][1][-1] and tuple(rows[1][1] + [t]) not in have)
    have.add(tuple(rows[1][1] + [cont]))
    ends = next(sp for sp in ([t, SIL] for t in range(ntok) if t != SIL) if tuple(sp) not in have)
    have.add(tuple(ends))
    one = next(([t] for t in range(ntok) if t != SIL and (t,) not in have), None) or next(sp for _, sp in rows if len(sp) == 1)
    rows += [(nwords - 4, list(rows[0][1])), (nwords - 3, rows[1][1] + [cont]), (nwords - 2, ends), (nwords - 1, list(one))]
    sps = [tuple(sp) for _, sp in rows]
    assert len(set(sps)) < len(sps) and any(a != b and a == b[:len(a)] for a in sps for b in sps)
    assert any(sp[-1] == SIL for sp in sps) and all(sp[0] != SIL for sp in sps) and any(len(sp) == 1 for sp in sps)
    return rows


class TokCase:
    """the inputs of one search: x [B][T][N], frames, A (ASG), the textbook token LM and trie with their tables, the options"""

    def __init__(self, asg, x, frames, A, tb, trie, lmw=0.5, wsc=-0.25, eos=-0.25, sil=-1, score=0.0):
        self.asg, self.x, self.frames, self.A, self.tb, self.trie = asg, x, frames, A, tb, trie
        self.lmw, self.wsc, self.eos, self.sil, self.score = lmw, wsc, eos, sil, score

    def but(self, **kw):
        c = TokCase(self.asg, self.x, self.frames, self.A, self.tb, self.trie, self.lmw, self.wsc, self.eos, self.sil, self.score)
        for k in ("_lm", "_lex"):
            if hasattr(self, k):
                setattr(c, k, getattr(self, k))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def tables(self):
        if not hasattr(self, "_lm"):
            self._lm = _lm_table(self.tb)
        if not hasattr(self, "_lex"):
            self._lex = _lex_table(self.trie)

    def gpu(self, W, K, M, Lmax, wide, threshold=INF, log_add=False, normalize=False, max_words=None):
        """the Python front end with lm_token=True -> {key: numpy array}"""
        from wav2letter_amd import criterion
        self.tables()
        xd = torch.tensor(self.x, device="cuda")
        fd = torch.tensor(self.frames, dtype=torch.int32, device="cuda") if self.frames is not None else None
        kw = dict(beam=W, beam_token=K, threshold=threshold, log_add=log_add, normalize=normalize, nbest=M, max_len=Lmax, wide=wide,
                  lm=self._lm, lm_weight=self.lmw, eos_score=self.eos, lexicon=self._lex, word_score=self.wsc, max_words=max_words,
                  lm_token=True, sil_token=self.sil, sil_score=self.score)
        if self.asg:
            out = criterion.asg_beam_search(xd, torch.tensor(self.A, device="cuda"), fd, **kw)
        else:
            out = criterion.ctc_beam_search(xd, fd, **kw)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in zip(KEYS, out)}

    def abi(self, family, W, K, M, Lmax, threshold=INF, log_add=False, normalize=False, max_words=None):
        """the C ABI's entry point itself, on poisoned outputs -> {key: numpy array}"""
        from wav2letter_amd import _lib as L
        lib = L.lib()
        self.tables()
        Bc, Tc, N = self.x.shape
        dev = torch.device("cuda")
        xd = torch.tensor(self.x, device=dev)
        fd = torch.tensor(self.frames, dtype=torch.int32, device=dev) if self.frames is not None else None
        Ad = torch.tensor(self.A, device=dev) if self.asg else None
        mw = Lmax if max_words is None else max_words
        o = dict(labels=torch.full((Bc, M, Lmax), -7, dtype=torch.int32, device=dev), lengths=torch.full((Bc, M), -7, dtype=torch.int32, device=dev),
                 scores=torch.full((Bc, M), 7.0, device=dev), lm_scores=torch.full((Bc, M), 7.0, device=dev),
                 words=torch.full((Bc, M, mw), -7, dtype=torch.int32, device=dev), word_counts=torch.full((Bc, M), -7, dtype=torch.int32, device=dev))
        nws = getattr(lib, ENTRY[self.asg] + "_lextok_workspace_size")(family, Bc, Tc, N, W, K)
        assert nws > 0
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        p = lambda t: t.data_ptr() if t is not None else None
        f = getattr(lib, ENTRY[self.asg] + "_search_lextok")
        head = (family, Bc, Tc, N, p(xd), p(fd)) + ((p(Ad),) if self.asg else ()) + (W, K, threshold, int(log_add), int(normalize), M, Lmax)
        rc = f(*head, p(self._lm.device_blob(dev)), int(self.tb.has_eos), self.lmw, p(self._lex.device_blob(dev)), self.wsc, self.eos,
               p(o["labels"]), p(o["lengths"]), p(o["scores"]), p(o["lm_scores"]), mw, p(o["words"]), p(o["word_counts"]), p(ws),
               torch.cuda.current_stream().cuda_stream, self.sil, float(self.score))
        L.check(rc, "beam_search_lextok")
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in o.items()}

    def ref(self, W, K, M, Lmax, dtype, threshold=INF, log_add=False, normalize=False, max_words=None):
        return TR.lextok_beam(self.x, self.frames, W, K, M, Lmax, self.trie, self.tb, self.lmw, self.wsc, self.eos, dtype, max_words,
                              A=self.A, sil=self.sil, sil_score=self.score, threshold=threshold, log_add=log_add, normalize=normalize)


def make_case(asg, seed, values="eighths", frames=FRAMES, t=T, nwords=NWORDS, rows=None, eos=True):
    """eighths: emissions, transitions and LM values multiples of 1/8, lmWeight 1/2, word and EOS scores multiples of 1/4: every fp32
    sum is exact.  four: emissions drawn from four dyadic values: dense ties.  normal: normal values"""
    rng = np.random.default_rng(seed)
    N = classes(asg)
    ntok = N if asg else N - 1
    shape = (len(frames) if frames is not None else B, t, N)
    if values == "eighths":
        x = (rng.integers(-24, 1, size=shape) / 8).astype(F32)
    elif values == "four":
        x = np.array([-2.0, -1.0, -0.5, 0.0], F32)[rng.integers(0, 4, size=shape)]
    else:
        x = rng.normal(0, 2, size=shape).astype(F32)
    A = None
    if asg:
        A = (rng.integers(-8, 9, size=(N, N)) / 8).astype(F32) if values != "normal" else rng.normal(0, 1, size=(N, N)).astype(F32)
    rows = lexicon_rows(rng, ntok, nwords) if rows is None else rows
    tb = LR.random_lm(rng, ntok, 3, 30, eos=eos, drop_unigrams=(UNK,), eighths=values != "normal")
    assert tb.order == 3
    nw = 1 + max(w for w, _ in rows)
    trie = XR.TextbookTrie(rows, ntok, nw, None, SIL)
    return TokCase(asg, x, frames, A, tb, trie)


def _family(family):
    return bool(family)


# ---- K1, K2: bit for bit against the float32 restatement -----------------------------------------------------------------------

# K2's seeds: those at which every (W, K) of the test has ties between the slots of a pair (found on the CPU, asserted there)
K1_SEEDS = {("eighths", False): 700, ("eighths", True): 701, ("four", False): 802, ("four", True): 803}


@functools.lru_cache(maxsize=None)
def k1_case(asg, values):
    return make_case(asg, K1_SEEDS[values, asg], values)


@functools.lru_cache(maxsize=None)
def k1_reference(asg, values, W, K):
    c = k1_case(asg, values)
    want = c.ref(W, K, min(W, 16), T, F32, INF, False, False, 6)
    return c, want


def _k_exact(asg, values, family, W, K):
    c, want = k1_reference(asg, values, W, K)
    dg = want["diags"]
    print("K1/K2", "asg" if asg else "ctc", values, (family, W, K), "live rows", int((want["lengths"] >= 0).sum()),
          {k: sum(getattr(d, k) for d in dg) for k in ("merges", "blocked", "homophones", "sil_loops", "slot_ties", "end_dropped")},
          "binds", any(d.beam_gap < INF for d in dg), "unk hits", c.tb.unk_hits, "back-off chain", c.tb.max_chain)
    assert (want["lengths"] >= 0).any() or W == 1
    got = c.gpu(W, K, min(W, 16), T, _family(family), INF, False, False, 6)
    _same_bits(got, {k: v for k, v in want.items() if k != "diags"})
    if K == 3:
        _same_bits(c.abi(family, W, K, min(W, 16), T, INF, False, False, 6), got)
    return dg


@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("family,W", WIDTHS)
@pytest.mark.parametrize("asg", [False, True])
def test_k1_dyadic_values_bit_equal_to_the_restatement(asg, family, W, K):
    dg = _k_exact(asg, "eighths", family, W, K)
    if K > 1 and W in (7, 65):                                   # the beam binds in both families
        assert any(d.beam_gap < INF for d in dg)
    if K == 64 and W >= 7:
        assert sum(d.merges for d in dg) > 0 and sum(d.blocked for d in dg) > 0 and sum(d.end_dropped for d in dg) > 0


@pytest.mark.parametrize("K", [3, 64])
@pytest.mark.parametrize("family,W", [(0, 7), (0, 64), (1, 200)])
@pytest.mark.parametrize("asg", [False, True])
def test_k2_dense_ties_bit_equal_slot_order_included(asg, family, W, K):
    dg = _k_exact(asg, "four", family, W, K)
    assert sum(d.slot_ties for d in dg) > 0 and sum(d.homophones for d in dg) > 0


# ---- K3: identity with the token-LM search --------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("family,W", [(0, 16), (1, 100)])
@pytest.mark.parametrize("asg", [False, True])
def test_k3_one_token_words_are_the_token_lm_search(asg, family, W, log_add):
    """every token a one-token word, no silence token, wordScore = 0, classScore = NULL"""
    ntok = classes(asg) - (0 if asg else 1)
    c = make_case(asg, 720 + asg, rows=[(t, [t]) for t in range(ntok)])
    c.trie = XR.TextbookTrie(c.trie.rows, ntok, ntok, None, None)
    c = c.but(wsc=0.0)
    norm = log_add and not asg
    got = c.gpu(W, 5, 8, T, _family(family), 4.0, log_add, norm, T)
    sib = Case("asg_lm" if asg else "ctc_lm", c.x, c.frames, c.A, c.tb, None, None, c.lmw, 0.0, c.eos)
    sib._lm = c._lm
    want = sib.gpu(W, 5, 8, T, _family(family), 4.0, log_add, norm)
    assert (want["lengths"] > 2).any()
    for k in ("labels", "lengths", "scores", "lm_scores"):
        assert (got[k].view(np.int32) == want[k].view(np.int32)).all(), k
    assert (got["words"] == got["labels"]).all() and (got["word_counts"] == got["lengths"]).all()


# ---- K4: identity with the word search at lmWeight = 0 --------------------------------------------------------------------------

@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("family,W", [(0, 12), (1, 100)])
@pytest.mark.parametrize("asg", [False, True])
def test_k4_weight_zero_is_the_word_search_on_an_unsmeared_lexicon(asg, family, W, log_add):
    c = make_case(asg, 730 + asg, eos=False).but(lmw=0.0, eos=0.0)
    assert not c.tb.has_eos
    norm = log_add and not asg
    got = c.gpu(W, 5, 8, T, _family(family), 4.0, log_add, norm, 6)
    word_lm = LR.random_lm(np.random.default_rng(1), NWORDS, 2, 30, eos=False)
    sib = Case("asg_lex" if asg else "ctc_lex", c.x, c.frames, c.A, word_lm, c.trie, None, 0.0, c.wsc, 0.0)
    sib._lex = c._lex
    want = sib.gpu(W, 5, 8, T, _family(family), 4.0, log_add, norm, 6)
    assert (want["word_counts"] > 1).any()
    for k in ("labels", "lengths", "scores", "words", "word_counts"):
        assert (got[k].view(np.int32) == want[k].view(np.int32)).all(), k


# ---- K5: logAdd = 1 on normalised rows against the float64 restatement ----------------------------------------------------------

# Beams of 4 and 7 as in X4: with random emissions a beam of 64 or more has its W-th and (W+1)-th candidate closer than the bar in
# some frame of nearly every utterance.  The log-sum at wider beams: K3, K4 and K6.
K5_T, K5_B = 12, 5
K5_SEEDS = {False: 2, True: 2}                                  # found on the CPU: test_k5_the_margin_filter_drops_at_most_a_fifth
K5_WIDTHS = [(0, 4), (0, 7), (1, 7)]


def k5_rows(ntok):
    """the recipe's kind of lexicon: every spelling ends on `|` (the silence token) and has it nowhere else, no homophones -- one
    token string has one segmentation, so no two hypotheses tie by construction"""
    rng = np.random.default_rng(5)
    letters = [t for t in range(ntok) if t != SIL]
    seen, rows = set(), []
    while len(rows) < 20:
        sp = tuple(int(letters[i]) for i in rng.integers(0, len(letters), int(rng.integers(1, 4))))
        if sp not in seen:
            seen.add(sp)
            rows.append((len(rows), list(sp) + [SIL]))
    return rows


@functools.lru_cache(maxsize=None)
def k5_reference(asg, W):
    """the float64 restatement and, per utterance, whether its decisions all have margins above X4's bar: every decision gap and every
    final gap >= 10 delta_lex(T, S)"""
    ntok = classes(asg) - (0 if asg else 1)
    c = make_case(asg, 740 + K5_SEEDS[asg], "normal", frames=None, t=K5_T, rows=k5_rows(ntok))
    c.x = np.random.default_rng(750 + K5_SEEDS[asg]).normal(0, 2, size=(K5_B, K5_T, classes(asg))).astype(F32)
    c = c.but(lmw=0.8, wsc=0.3, eos=-0.3)
    want = c.ref(W, 4, 2, K5_T, np.float64, INF, True, True, K5_T)
    ok = []
    for dg in want["diags"]:
        dl = XR.delta_lex(K5_T, dg.S)
        ok.append(dg.decision_gap() >= 10 * dl and min(dg.final_gaps + [np.inf]) >= 10 * dl)
    return c, want, ok


def test_k5_the_margin_filter_drops_at_most_a_fifth():
    total = kept = 0
    for asg in (False, True):
        for _, W in K5_WIDTHS:
            ok = k5_reference(asg, W)[2]
            total, kept = total + len(ok), kept + sum(ok)
    print("K5 compared utterances", kept, "of", total)
    assert 5 * (total - kept) <= total


@pytest.mark.parametrize("family,W", K5_WIDTHS)
@pytest.mark.parametrize("asg", [False, True])
def test_k5_log_sum_search_against_the_float64_restatement(asg, family, W):
    c, want, ok = k5_reference(asg, W)
    got = c.gpu(W, 4, 2, K5_T, _family(family), INF, True, True, K5_T)
    assert any(ok) and all(d.beam_gap < INF for d in want["diags"])   # the beam binds
    for b in range(K5_B):
        if not ok[b]:
            continue
        for k in ("labels", "lengths", "words", "word_counts"):
            assert (got[k][b] == want[k][b]).all(), (asg, W, b, k)
        g, w = got["scores"][b], want["scores"][b]
        fin = np.isfinite(w)
        assert (np.isfinite(g) == fin).all() and _close(g[fin], w[fin]).all(), (asg, W, b)
        assert (got["lm_scores"][b].view(np.int32) == want["lm_scores"][b].view(np.int32)).all()
        print("K5", "asg" if asg else "ctc", W, b, "max |score diff|", float(np.abs(g[fin] - w[fin]).max(initial=0.0)))


# ---- K6: narrow == wide ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("W", [1, 2, 7, 64])
@pytest.mark.parametrize("asg", [False, True])
def test_k6_the_two_families_agree_bit_for_bit(asg, W, log_add):
    c = k1_case(asg, "eighths").but(sil=SIL, score=-0.75)
    norm = log_add and not asg
    for K, thr in ((3, INF), (64, 5.0)):
        narrow = c.gpu(W, K, W, 5, False, thr, log_add, norm, 2)
        wide = c.gpu(W, K, W, 5, True, thr, log_add, norm, 2)
        assert (narrow["lengths"] >= 0).any() or W == 1
        _same_bits(wide, narrow)


# ---- K7: the silence score ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("family,W", [(0, 8), (1, 96)])
@pytest.mark.parametrize("asg", [False, True])
def test_k7_silence_score(asg, family, W, log_add):
    """normal values: the frame tokens' order, the tie key's k, is the acoustic one with a score and the biased one on biased
    emissions, so two candidates of one entry that tie exactly at the beam's cut (dyadic values have such ties: the restatement
    itself then differs between the two) would be kept in another order; both sides do the same fp32 operations on the same values"""
    from tests.beam_sil_ref import bias_column
    c = k7_case(asg)
    plain = c.gpu(W, 64, 8, T, _family(family), INF, log_add, False, 6)
    for score in (-1.5, 0.75):
        got = c.but(sil=SIL, score=score).gpu(W, 64, 8, T, _family(family), INF, log_add, False, 6)
        want = c.but(x=bias_column(c.x, SIL, score)).gpu(W, 64, 8, T, _family(family), INF, log_add, False, 6)
        assert (want["lengths"] >= 0).any()
        _same_bits(got, want)
        assert any((plain[k].view(np.int32) != got[k].view(np.int32)).any() for k in ("labels", "scores"))   # the score acts
    for sil, score in ((SIL, 0.0), (-1, 3.0), (SIL, -0.0)):      # no score: the bytes of silToken = -1
        _same_bits(c.but(sil=sil, score=score).abi(family, W, 4, 8, T, 6.0, log_add, False, 6), plain_abi(c, family, W, log_add))


@functools.lru_cache(maxsize=None)
def k7_case(asg):
    return make_case(asg, 760 + asg, "normal")


def plain_abi(c, family, W, log_add):
    return c.but(sil=-1, score=0.0).abi(family, W, 4, 8, T, 6.0, log_add, False, 6)


def test_k7_score_with_selection_bit_equal_to_the_restatement():
    """K = 3: the frame tokens are those of the acoustic lp alone"""
    for asg in (False, True):
        c = k1_case(asg, "eighths").but(sil=SIL, score=2.0)
        want = c.ref(8, 3, 8, T, F32, INF, False, False, 6)
        _same_bits(c.gpu(8, 3, 8, T, False, INF, False, False, 6), {k: v for k, v in want.items() if k != "diags"})


# ---- K8: ASG with zero transitions == CTC with a -inf blank column ---------------------------------------------------------------

@pytest.mark.parametrize("family,W", [(0, 8), (1, 96)])
def test_k8_asg_with_zero_transitions_is_ctc_with_an_impossible_blank(family, W):
    a = k1_case(True, "eighths")
    a = a.but(A=np.zeros_like(a.A))
    x = np.concatenate([a.x, np.full(a.x.shape[:2] + (1,), -np.inf, F32)], axis=2)
    c = TokCase(False, x, a.frames, None, a.tb, a.trie, a.lmw, a.wsc, a.eos)
    got = a.gpu(W, 5, 8, T, _family(family), INF, False, False, 6)
    want = c.gpu(W, 5, 8, T, _family(family), INF, False, False, 6)
    assert (want["lengths"] >= 0).any()
    _same_bits(got, want)
