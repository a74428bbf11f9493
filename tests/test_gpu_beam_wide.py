"""The wide beam searches (w2l_*_beam_search*_wide, W up to 1024) on the GPU.
W1 identity with the narrow kernels at the widths both accept, byte for byte, both (+) modes; W2 logAdd = 0 bit for bit against
the float32 restatements (tests/*_beam_ref.py, generic in W) above the narrow limit, on inputs whose sums are exact and whose
ties are dense, with the proof on the CPU that the beam holds more than 64 entries, binds and merges; W3 logAdd = 1 against the
float64 restatements where the decisions have a margin; W4 the output rules at M = W = 1024; W5 the complete labelling list of an
enumeration; W6 the surfaces: Python, the compiled C++ caller, Decode --beamsize.
A search is named by its kind: ctc, ctc_lm, ctc_lex, asg (no LM), asg_lm, asg_lex -- the five entry points, w2l_asg_beam_search
with and without its optional LM."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import asg_beam_ref as AR
from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR
from tests import ctc_beam_ref as R

pytestmark = pytest.mark.gpu
INF = float("inf")
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("ctc", "ctc_lm", "ctc_lex", "asg", "asg_lm", "asg_lex")
KEYS = ("labels", "lengths", "scores", "lm_scores", "words", "word_counts")


def _lm_table(tb):
    from wav2letter_amd import NGramLM
    return NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk))


def _lex_table(trie):
    from wav2letter_amd import Lexicon
    return Lexicon.from_spellings(trie.rows, trie.num_tokens, trie.num_words, trie.word_smear, trie.sil)


def _smear(tb, nwords):
    return np.array([tb.score(tb.history(()), w, F32) for w in range(nwords)], F32)


class Case:
    """the inputs of one search of one kind: x [B][T][N], frames, A, the textbook LM and trie with their tables, the options"""

    def __init__(self, kind, x, frames=None, A=None, tb=None, trie=None, cls=None, lmw=0.0, wsc=0.0, eos=0.0):
        self.kind, self.x, self.frames, self.A, self.tb, self.trie, self.cls = kind, x, frames, A, tb, trie, cls
        self.lmw, self.wsc, self.eos = lmw, wsc, eos
        self.asg = kind.startswith("asg")

    def gpu(self, W, K, M, Lmax, wide, threshold=INF, log_add=False, normalize=False, max_words=None):
        """the Python front end (criterion.ctc_beam_search / asg_beam_search) -> {key: numpy array}"""
        from wav2letter_amd import criterion
        xd = torch.tensor(self.x, device="cuda")
        fd = torch.tensor(self.frames, dtype=torch.int32, device="cuda") if self.frames is not None else None
        kw = dict(beam=W, beam_token=K, threshold=threshold, log_add=log_add, normalize=normalize, nbest=M, max_len=Lmax, wide=wide)
        if self.tb is not None:
            if not hasattr(self, "_lm"):
                self._lm = _lm_table(self.tb)
            kw.update(lm=self._lm, lm_weight=self.lmw, eos_score=self.eos)
            if self.cls is not None:
                kw.update(class_score=torch.tensor(self.cls, device="cuda"))
        if self.trie is not None:
            if not hasattr(self, "_lex"):
                self._lex = _lex_table(self.trie)
            kw.update(lexicon=self._lex, word_score=self.wsc, max_words=max_words)
        if self.asg:
            out = criterion.asg_beam_search(xd, torch.tensor(self.A, device="cuda"), fd, **kw)
        else:
            out = criterion.ctc_beam_search(xd, fd, **kw)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in zip(KEYS, out)}

    def ref(self, W, K, M, Lmax, dtype, threshold=INF, log_add=False, normalize=False, max_words=None):
        """the restatement -> {key: numpy array, "diags": [...]}"""
        x, fr, tb, trie = self.x, self.frames, self.tb, self.trie
        if self.asg:
            kw = dict(threshold=threshold, log_add=log_add, normalize=normalize)
            if tb is not None:
                kw.update(lm=tb, lm_weight=self.lmw, eos_score=self.eos)
            if trie is not None:
                kw.update(word_score=self.wsc)
            elif self.cls is not None:
                kw.update(class_score=self.cls)
            o = AR.asg_beam(x, self.A, fr, W, K, M, Lmax, dtype, trie=trie, max_words=max_words, **kw)
            if tb is None:
                del o["lm_scores"]
            return o
        if trie is not None:
            mw = Lmax if max_words is None else max_words
            out = XR.beam_search_lex(x, fr, W, K, trie, tb, self.lmw, self.wsc, self.eos, threshold, log_add, normalize, M, Lmax, mw, dtype)
            return dict(zip(KEYS + ("diags",), out))
        if tb is not None:
            out = LR.beam_search_lm(x, fr, W, K, tb, self.lmw, self.cls, self.eos, threshold, log_add, normalize, M, Lmax, dtype)
            return dict(zip(KEYS[:4] + ("diags",), out))
        out = R.beam_search(x, fr, W, K, threshold, log_add, normalize, M, Lmax, dtype)
        return dict(zip(KEYS[:3] + ("diags",), out))

    def merges(self, W, K, threshold, diags):
        """merged extensions per utterance in the logAdd = 0 search whose Diags are `diags` (the LM-free CTC restatement does not
        count them: the token-LM restatement does, and with weight 0 on a model of zeros it is the same search)"""
        if self.kind != "ctc":
            return [d.merges for d in diags]
        V = self.x.shape[2] - 1
        zero = LR.TextbookLM({(w,): (0.0, 0.0) for w in range(V + 2)}, V, 0.0)
        out = LR.beam_search_lm(self.x, self.frames, W, K, zero, 0.0, None, 0.0, threshold, False, False, 1, 1, F32)
        return [d.merges for d in out[4]]


def _same_bits(got, want):
    for k in KEYS:
        if k in want:
            assert k in got and got[k].dtype == want[k].dtype, k
            assert (got[k].view(np.int32) == want[k].view(np.int32)).all(), k
    assert sum(k in got for k in KEYS) == sum(k in want for k in KEYS)


def _quarters(rng, shape, lo, hi):
    return (rng.integers(lo * 4, hi * 4 + 1, size=shape) / 4).astype(F32)


def _dense_case(kind, seed, B, T, N, frames, hot=10, nwords=300, max_len=3):
    """dense ties: emissions multiples of 1/4, transitions, LM values and smear values multiples of 1/8, lmWeight = 1/2, wordScore and
    eosScore multiples of 1/4: every sum is exact in fp32.  With a lexicon the first `hot` classes (its letters) and the blank lead
    the rows.  The lexicon has homophones, words that are prefixes of others and silence at the root (asserted)"""
    rng = np.random.default_rng(seed)
    asg = kind.startswith("asg")
    tokens = N if asg else N - 1
    x = _quarters(rng, (B, T, N), -3, 0)
    A = (rng.integers(-8, 9, size=(N, N)) / 8).astype(F32) if asg else None
    if kind.endswith("lex"):
        hot = min(hot, tokens)
        x = _quarters(rng, (B, T, N), -6, -3)
        x[:, :, :hot] = _quarters(rng, (B, T, hot), -3, 0)
        if not asg:
            x[:, :, N - 1] = _quarters(rng, (B, T), -3, 0)
        sil = hot - 1
        rows = XR.random_lexicon(rng, tokens, nwords, max_len, 0.1, sil, hot)
        tb = LR.random_lm(rng, nwords, 3, 2 * nwords, True, True, (), eighths=True)
        trie = XR.TextbookTrie(rows, tokens, nwords, _smear(tb, nwords), sil)
        nodes = [u for _, u in trie.nodes()]
        assert any(len(u.words) >= 2 for u in nodes) and any(u.words and u.children for u in nodes) and trie.sil is not None
        return Case(kind, x, frames, A, tb, trie, None, 0.5, -0.25, -0.25)
    if kind.endswith("lm"):
        tb = LR.random_lm(rng, tokens, 3, 40 * tokens, True, True, (), eighths=True)      # 3-grams with back-off, EOS
        assert tb.order == 3 and tb.has_eos
        cls = _quarters(rng, (tokens,), -1, 0)
        return Case(kind, x, frames, A, tb, None, cls, 0.5, 0.0, -0.25)
    return Case(kind, x, frames, A)


# ---- W1: identity with the narrow kernels ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _w1_case(kind):
    return _dense_case(kind, 11 + KINDS.index(kind), 3, 24, 30, [24, 1, 17])


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("K", [8, 29])
@pytest.mark.parametrize("W", [1, 8, 63, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_w1_twin_equals_sibling_byte_for_byte(kind, W, K, log_add):
    """every output tensor, both (+) modes (with logAdd = 1 a stay receives at most one merged term: no sum depends on an order),
    with a threshold that cuts at the wider beams and with label and word rows shorter than the hypotheses"""
    c = _w1_case(kind)
    M, Lmax, thr = W, 5, (INF if W < 63 else 4.0)
    narrow = c.gpu(W, K, M, Lmax, False, thr, log_add, log_add and not c.asg, 2)
    wide = c.gpu(W, K, M, Lmax, True, thr, log_add, log_add and not c.asg, 2)
    assert (narrow["lengths"] >= 0).any() and narrow["lengths"].max() > Lmax
    _same_bits(wide, narrow)


# ---- W2: bit for bit against the float32 restatement, logAdd = 0 -------------------------------------------------------------

W2_SHAPES = {  # name: (W, K, N, T, B, frames, threshold)
    "w65": (65, 8, 30, 24, 3, [24, 1, 17], INF),
    "w100": (100, 8, 30, 24, 3, [24, 1, 17], INF),
    "w256": (256, 16, 30, 24, 3, [24, 1, 17], INF),
    "w256_threshold": (256, 16, 30, 24, 3, [24, 1, 17], None),      # W2_THRESHOLD[kind]
    "w1024_k64": (1024, 64, 70, 8, 2, None, INF),
    "w100_n100": (100, 8, 100, 24, 3, [24, 1, 17], INF),      # the ASG kinds only: transitions gathered from global memory
}


# small enough to cut, large enough to leave more than 64 entries: the LM and lexicon terms spread the totals
W2_THRESHOLD = {"ctc": 1.0, "ctc_lm": 2.5, "ctc_lex": 2.5, "asg": 1.0, "asg_lm": 2.5, "asg_lex": 2.5}


def _w2_kinds(name):
    return [k for k in KINDS if name != "w100_n100" or k.startswith("asg")]


@functools.lru_cache(maxsize=None)
def _w2_reference(name, kind):
    """inputs, the float32 restatement's outputs (M = W rows) and the facts that make the case worth running, asserted here on the
    CPU: the beam holds more than 64 entries, the beam binds, every utterance of three frames and more merges, and in the
    threshold case the line removes candidates (the same search without it ends otherwise)"""
    W, K, N, T, B, frames, thr = W2_SHAPES[name]
    thr = W2_THRESHOLD[kind] if thr is None else thr
    big = name == "w1024_k64"
    seed = 100 + 7 * list(W2_SHAPES).index(name.replace("_threshold", "")) + KINDS.index(kind)
    c = _dense_case(kind, seed, B, T, N, frames, hot=64 if big else 10, nwords=2000 if big else 300, max_len=2 if big else 3)
    want = c.ref(W, K, W, T, F32, thr, False, False, T)
    diags = want["diags"]
    held = int((want["lengths"] >= 0).sum(axis=1).max()) + (max(d.end_dropped for d in diags) if kind.endswith("lex") else 0)
    binds = any(d.cuts > 0 for d in diags) if c.asg else any(d.beam_gap < INF for d in diags)
    merges = c.merges(W, K, thr, diags)
    long_utts = [b for b in range(B) if (T if frames is None else frames[b]) >= 3]
    facts = dict(held=held, binds=binds, merges=merges)
    assert held > 64 and binds and all(merges[b] > 0 for b in long_utts), (name, kind, facts)
    if thr != INF:
        free = _w2_reference("w256", kind)[1]                             # the same inputs without the line
        assert any((free[k].view(np.int32) != want[k].view(np.int32)).any() for k in ("labels", "scores")), (name, kind)
    return c, want, facts


@pytest.mark.parametrize("name,kind", [(n, k) for n in W2_SHAPES for k in _w2_kinds(n)])
def test_w2_bitwise_against_the_float32_restatement(name, kind):
    W, K, N, T, B, frames, thr = W2_SHAPES[name]
    c, want, facts = _w2_reference(name, kind)
    thr = W2_THRESHOLD[kind] if thr is None else thr
    print("W2", name, kind, facts, "live rows", int((want["lengths"] >= 0).sum()))
    got = c.gpu(W, K, W, T, True, thr, False, False, T)
    assert want["scores"].dtype == F32
    _same_bits(got, {k: v for k, v in want.items() if k != "diags"})


# ---- W3: logAdd = 1 against the float64 restatement --------------------------------------------------------------------------

W3_EXTRA = {"ctc": 0, "ctc_lm": 1, "ctc_lex": 4, "asg": 0, "asg_lm": 1, "asg_lex": 4}     # the siblings' own roundings per frame
W3_SHAPES = [(100, 8, 30, 16, 4), (1024, 8, 30, 12, 4)]                                      # (W, K, N, T, B)
W3_M = 4


def _delta(kind, T, S):
    if kind.startswith("asg"):
        return AR.delta_asg(T, S, W3_EXTRA[kind])
    return {"ctc": R.delta, "ctc_lm": LR.delta_lm, "ctc_lex": XR.delta_lex}[kind](T, S)


@functools.lru_cache(maxsize=None)
def _w3_reference(i, kind):
    W, K, N, T, B = W3_SHAPES[i]
    rng = np.random.default_rng(900 + 10 * i + KINDS.index(kind))
    asg = kind.startswith("asg")
    tokens = N if asg else N - 1
    x = rng.normal(0, 3, size=(B, T, N)).astype(F32)
    x[:, :, :8] += 6
    if not asg:
        x[:, :, N - 1] += 6
    A = rng.normal(0, 1, size=(N, N)).astype(F32) if asg else None
    c = Case(kind, x, None, A)
    if kind.endswith("lm"):
        c = Case(kind, x, None, A, LR.random_lm(rng, tokens, 3, 300), None, rng.normal(0, 0.3, tokens).astype(F32), 0.8, 0.0, -0.3)
    if kind.endswith("lex"):
        nwords = 60
        tb = LR.random_lm(rng, nwords, 3, 200)
        trie = XR.TextbookTrie(XR.random_lexicon(rng, tokens, nwords, 3, 0.1, 7, 8), tokens, nwords, _smear(tb, nwords), 7)
        c = Case(kind, x, None, A, tb, trie, None, 0.8, 0.3, -0.3)
    want = c.ref(W, K, W3_M, T, np.float64, INF, True, not asg, T)
    lead = []      # per utterance: the leading ranks whose every decision has a margin above twice the bound, and the bound
    for dg in want["diags"]:
        dl = _delta(kind, T, dg.S)
        n = 0
        if dg.token_gap > 2 * dl:
            while n < len(dg.margins) and dg.margins[n] > 2 * dl and (n >= len(dg.final_gaps) or dg.final_gaps[n] > 2 * dl):
                n += 1
        lead.append((n, dl))
    return c, want, lead


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(W3_SHAPES)))
def test_w3_log_sum_search_against_the_float64_restatement(i, kind):
    """the method of the siblings' log-sum tests: the scores within delta(T, S), the hypotheses compared where the restatement's own
    margins (lineage, frame tokens, next rank) exceed twice that bound; at most one utterance in four may have no such rank"""
    W, K, N, T, B = W3_SHAPES[i]
    c, want, lead = _w3_reference(i, kind)
    left_out = sum(1 for n, _ in lead if n == 0)
    print("W3", W3_SHAPES[i], kind, "compared ranks per utterance", [n for n, _ in lead], "delta", max(dl for _, dl in lead))
    assert 4 * left_out <= B and (want["lengths"] >= 0).any()
    got = c.gpu(W, K, W3_M, T, True, INF, True, not c.asg, T)
    for b, (n, dl) in enumerate(lead):
        for k in ("labels", "lengths", "words", "word_counts"):
            if k in want:
                assert (got[k][b, :n] == want[k][b, :n]).all(), (b, k)
        assert (np.abs(got["scores"][b, :n].astype(np.float64) - want["scores"][b, :n]) <= dl).all(), b
        if "lm_scores" in want:
            assert (got["lm_scores"][b, :n].view(np.int32) == want["lm_scores"][b, :n].view(np.int32)).all()


# ---- W4: outputs -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_w4_m_equals_w_1024_with_short_label_rows(kind):
    """M = W = 1024, Lmax = 3 (and two word rows): truncated rows, true lengths"""
    c, want, _ = _w2_reference("w1024_k64", kind)
    W, K, N, T, B, frames, thr = W2_SHAPES["w1024_k64"]
    got = c.gpu(W, K, W, 3, True, thr, False, False, 2)
    assert want["lengths"].max() > 3
    for k in ("lengths", "scores", "lm_scores", "word_counts"):
        if k in want:
            assert (got[k].view(np.int32) == want[k].view(np.int32)).all(), k
    assert (got["labels"] == want["labels"][:, :, :3]).all()
    if "words" in want:
        assert want["word_counts"].max() > 2 and (got["words"] == want["words"][:, :, :2]).all()


@pytest.mark.parametrize("kind", ["ctc", "ctc_lm", "asg", "asg_lm"])
def test_w4_fewer_prefixes_than_w(kind):
    """N = 3, T = 4: a handful of prefixes; the rows beyond the survivors are -1 / -inf"""
    c = _dense_case(kind, 5, 2, 4, 3, None)
    want = c.ref(1024, 64, 1024, 4, F32)
    got = c.gpu(1024, 64, 1024, 4, True)
    live = (want["lengths"] >= 0).sum(axis=1)
    assert (live > 4).all() and (live < 64).all()
    _same_bits(got, {k: v for k, v in want.items() if k != "diags"})
    assert (got["lengths"][:, 64:] == -1).all() and np.isneginf(got["scores"][:, 64:]).all() and (got["labels"][:, 64:] == -1).all()


@pytest.mark.parametrize("kind", ["ctc_lex", "asg_lex"])
def test_w4_lexicon_without_an_entry_at_the_root(kind):
    """every word has two tokens and the utterance one frame: every entry ends inside a word, all rows are empty (CTC: the empty
    prefix, which stands at the root, stays on the blank, so the blank is far below the threshold line here; ASG has no blank)"""
    asg = kind.startswith("asg")
    rng = np.random.default_rng(3)
    N, tokens = 12, 12 if asg else 11
    x = _quarters(rng, (2, 1, N), -3, 0)
    thr = INF if asg else 8.0
    if not asg:
        x[:, :, N - 1] = -40.0
    rows = [(w, [w % tokens, (w + 1) % tokens]) for w in range(tokens)]
    tb = LR.random_lm(rng, tokens, 2, 30, True, True, (), eighths=True)
    trie = XR.TextbookTrie(rows, tokens, tokens, _smear(tb, tokens), None)
    c = Case(kind, x, None, (rng.integers(-8, 9, size=(N, N)) / 8).astype(F32) if asg else None, tb, trie, None, 0.5, 0.25, 0.0)
    want = c.ref(200, 64, 200, 4, F32, thr, max_words=4)
    assert sum(d.end_dropped for d in want["diags"]) > 0 and (want["lengths"] == -1).all()
    got = c.gpu(200, 64, 200, 4, True, thr, max_words=4)
    _same_bits(got, {k: v for k, v in want.items() if k != "diags"})
    assert (got["lengths"] == -1).all() and (got["word_counts"] == -1).all() and (got["labels"] == -1).all()
    assert (got["words"] == -1).all() and np.isneginf(got["scores"]).all() and np.isneginf(got["lm_scores"]).all()


# ---- W5: exhaustive ----------------------------------------------------------------------------------------------------------

def _w5_inputs(N, T, seed):
    """random multiples of 1/64 in (-4096, 0]: every path sum is exact in fp32; that no two labellings tie is asserted"""
    rng = np.random.default_rng(seed)
    return (-rng.integers(0, 1 << 18, size=(1, T, N)) / 64).astype(F32)


@pytest.mark.parametrize("kind,N,T,count", [("ctc", 5, 5, 625), ("asg", 5, 4, 425)])
def test_w5_the_complete_labelling_list_of_the_enumeration(kind, N, T, count):
    """W = 1024 holds every labelling of these shapes (625 and 425 of them: the narrow kernels' 64 cannot): with logAdd = 0 the
    output is the enumeration's list, every labelling with the maximum over its paths, in the enumeration's order.  (N = 5, T = 6
    has 2065 CTC labellings and 6825 ASG ones, more than any W here: that shape runs below against the restatement.)"""
    x = _w5_inputs(N, T, 50)
    A = np.zeros((N, N), F32)
    c = Case(kind, x, None, A if kind == "asg" else None)
    want = AR.enumerate_labellings(x[0], A, False, False) if kind == "asg" else R.enumerate_labellings(x[0], False, False)
    order = sorted(want, key=lambda h: -want[h])
    assert len(order) == count and len({want[h] for h in order}) == count
    got = c.gpu(1024, 64, 1024, T, True)
    ln = got["lengths"][0]
    assert (ln[:count] >= 0).all() and (ln[count:] == -1).all()
    assert [tuple(got["labels"][0, m, :ln[m]]) for m in range(count)] == order
    assert (got["scores"][0, :count].astype(np.float64) == np.array([want[h] for h in order])).all()


@pytest.mark.parametrize("kind", ["ctc", "asg"])
def test_w5_n5_t6_w1024_against_the_restatement(kind):
    x = _w5_inputs(5, 6, 77)
    c = Case(kind, x, None, np.zeros((5, 5), F32) if kind == "asg" else None)
    want = c.ref(1024, 64, 1024, 6, F32)
    assert (want["lengths"] >= 0).all()                                  # 2065 / 6825 labellings: the beam is full
    _same_bits(c.gpu(1024, 64, 1024, 6, True), {k: v for k, v in want.items() if k != "diags"})


# ---- W6: surfaces ------------------------------------------------------------------------------------------------------------

def test_w6_python_methods_take_wide():
    from wav2letter_amd import ASGLoss, CTCLoss, _lib, criterion
    c = _w1_case("ctc_lm")
    xd, fd = torch.tensor(c.x, device="cuda"), torch.tensor(c.frames, dtype=torch.int32, device="cuda")
    want = c.gpu(200, 8, 3, 24, True)
    got = CTCLoss().beamSearch(xd, fd, beam=200, beam_token=8, nbest=3, lm=c._lm, lm_weight=c.lmw, eos_score=c.eos,
                               class_score=torch.tensor(c.cls, device="cuda"), wide=True)
    assert all((g.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all() for g, k in zip(got, KEYS))
    a = _w1_case("asg")
    crit = ASGLoss(30).cuda()
    with torch.no_grad():
        crit.transitions.copy_(torch.tensor(a.A))
    xa, fa = torch.tensor(a.x, device="cuda"), torch.tensor(a.frames, dtype=torch.int32, device="cuda")
    want = a.gpu(200, 8, 3, 24, True)
    got = crit.beamSearch(xa, fa, beam=200, beam_token=8, nbest=3, wide=True)
    assert len(got) == 3 and all((g.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all() for g, k in zip(got, KEYS))
    # wide=False is the narrow path with its refusal; the wide one refuses beyond 1024
    for wide, beam in ((False, 65), (True, 1025)):
        with pytest.raises(_lib.W2LError):
            criterion.ctc_beam_search(xd, beam=beam, wide=wide)
        with pytest.raises(_lib.W2LError):
            criterion.asg_beam_search(xa, torch.tensor(a.A, device="cuda"), beam=beam, wide=wide)
    assert criterion.ctc_beam_search(xd, beam=65, wide=True)[1].min() >= 0


def test_w6_cpp_options_wide_equal_the_c_abi(tmp_path):
    """tests/cpp/decode_wide_caller.cpp (plain g++ against libw2l_hip.so): BeamSearchOptions::wide for CTC + lexicon and ASG + token
    LM, from the same lexicon and ARPA files; its output equals the Python front end's, which calls the C ABI"""
    from tests.test_ctc_beam_lm_host import _arpa_text
    from wav2letter_amd import Lexicon, NGramLM
    exe, libdir = str(tmp_path / "decode_wide_caller"), os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "decode_wide_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    rng = np.random.default_rng(21)
    B, T, W, K, M, Lmax, maxw = 3, 20, 200, 8, 5, 20, 6
    letters = [chr(ord("a") + i) for i in range(10)]
    spell = sorted({"".join(letters[int(t)] for t in rng.integers(0, 9, int(rng.integers(1, 4)))) for _ in range(120)})
    (tmp_path / "tokens.txt").write_text("\n".join(letters) + "\n")
    (tmp_path / "lexicon.txt").write_text("".join(f"{w} {' '.join(w)}\n" for w in spell) + f"{spell[0]}x {' '.join(spell[0])}\n")
    for mode, N in (("ctc_lex", 11), ("asg_lm", 10)):
        x = rng.normal(0, 2, size=(B, T, N)).astype(F32)
        frames = np.array([T, 7, 13], np.int32)
        A = rng.normal(0, 1, size=(N, N)).astype(F32)
        if mode == "ctc_lex":
            lex = Lexicon.from_file(tmp_path / "lexicon.txt", letters, sil=letters[-1], smearing="none")
            tb = LR.random_lm(rng, lex.num_words, 2, 150)
            (tmp_path / "lm.arpa").write_text(_arpa_text(tb, lex.words, unk10=-3.0)[0])
            lm = NGramLM.from_arpa(tmp_path / "lm.arpa", lex.words)
            lex = Lexicon.from_file(tmp_path / "lexicon.txt", letters, lm=lm, sil=letters[-1])
        else:
            tb = LR.random_lm(rng, N, 3, 200)
            (tmp_path / "lm.arpa").write_text(_arpa_text(tb, letters, unk10=-3.0)[0])
            lm, lex = NGramLM.from_arpa(tmp_path / "lm.arpa", letters), None
        c = Case(mode, x, frames, A if mode == "asg_lm" else None)
        c.tb, c._lm, c.lmw, c.eos = tb, lm, 0.75, -0.25
        if lex is not None:
            c.trie, c._lex, c.wsc = True, lex, 0.5
        want = c.gpu(W, K, M, Lmax, True, 6.0, True, mode == "ctc_lex", maxw)
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([N, T, B, W, K, M, Lmax, maxw], np.int32).tobytes() + frames.tobytes() + x.tobytes() + A.tobytes())
        run = subprocess.run([exe, mode, inp, outp, str(tmp_path / "tokens.txt"), str(tmp_path / "lexicon.txt"), str(tmp_path / "lm.arpa")],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "decode wide caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
        raw = np.fromfile(outp, np.int32)
        pos = 0
        for k, shape in (("labels", (B, M, Lmax)), ("lengths", (B, M)), ("scores", (B, M)), ("lm_scores", (B, M)),
                         ("words", (B, M, maxw)), ("word_counts", (B, M))):
            if k in want:
                n = int(np.prod(shape))
                assert (raw[pos:pos + n].reshape(shape) == want[k].view(np.int32)).all(), (mode, k)
                pos += n
        assert pos == len(raw) and (want["lengths"] >= 0).any()


# ---- Decode --beamsize ---------------------------------------------------------------------------------------------------------

from tests.list_fixture import ENV  # noqa: E402
from tests.test_gpu_asg_beam import trained_asg  # noqa: E402,F401  (the module-scoped ASG checkpoint)
from tests.test_gpu_ctc_beam import DECODE_EXE, _sclite_lines, trained  # noqa: E402,F401  (the module-scoped CTC checkpoint)


def _decode(d, model, *flags):
    res = subprocess.run([DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}"] + list(flags),
                         capture_output=True, text=True, timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return res.stderr, (d / "out" / "other.hyp").read_text()


def _decode_checks(d, model):
    """--beamsize above 64 runs the wide kernels; with --logadd=false and no LM the 1-best of every width is the transcript of the
    greedy / Viterbi path, which is also what a beam of one entry keeps; beyond 1024 the width is limited, and said so"""
    err1, greedy = _decode(d, model, "--beamsize=1")
    err0, default = _decode(d, model)                                   # no --beamsize: the default, limited to 64, narrow
    assert "limited to 64 (the kernel's beam width)" in err0 and "(wide)" not in err0 and "(wide)" not in err1
    assert default == greedy and len(_sclite_lines(d / "out" / "other.hyp")) == 5
    for w in (16, 64):
        err, hyp = _decode(d, model, f"--beamsize={w}")
        assert "(wide)" not in err and "limited to" not in err.split("--beamsizetoken")[0] and hyp == greedy
    err, hyp = _decode(d, model, "--beamsize=200")
    assert f"beam 200 (wide)" in err and "limited to 1024" not in err and hyp == greedy
    dump = ["--isbeamdump=true", "--nbest=3", "--beamthreshold=100"]
    err, at1024 = _decode(d, model, "--beamsize=1024", *dump)
    assert "beam 1024 (wide)" in err and "limited to 1024" not in err
    err, at5000 = _decode(d, model, "--beamsize=5000", *dump)
    assert "--beamsize=5000 limited to 1024 (the kernel's beam width)" in err and "beam 1024 (wide)" in err
    assert at5000 == at1024 and len(at1024.splitlines()) == 15
    rows = [line.split(" | ") for line in at1024.splitlines()]
    assert [r[5].split() for r in rows[::3]] == [w for w, _ in [(ln[:-1].rsplit(" (", 1)[0].split(), 0) for ln in greedy.splitlines()]]
    # the narrow dump at 16 entries against the wide one: the same first rows wherever 16 entries were enough for the three best
    err, at16 = _decode(d, model, "--beamsize=16", *dump)
    assert "(wide)" not in err and [ln.split(" | ")[5] for ln in at16.splitlines()[::3]] == [r[5] for r in rows[::3]]


def test_w6_decode_beamsize_ctc(trained):
    _decode_checks(*trained)


def test_w6_decode_beamsize_asg_and_lexicon(trained_asg, tmp_path):
    from tests.test_gpu_ctc_beam_lex import _lexicon_files
    d, model = trained_asg
    _decode_checks(d, model)
    lex_path, arpa, words = _lexicon_files(tmp_path)
    lex = ["--beamthreshold=100", "--uselexicon=true", "--decodertype=wrd", f"--lexicon={lex_path}", f"--lm={arpa}", "--lmweight=0.5",
           "--wordscore=6", "--smearing=max"]
    err, hyp = _decode(d, model, "--beamsize=200", *lex)
    assert "beam 200 (wide)" in err and "--lexicon: 26 words" in err
    got = _sclite_lines(d / "out" / "other.hyp")
    assert [s for _, s in got] == [f"u{k}" for k in range(5)] and all(set(w) <= set(words) for w, _ in got) and any(w for w, _ in got)
    err, at5000 = _decode(d, model, "--beamsize=5000", *lex)
    assert "limited to 1024" in err and at5000 == _decode(d, model, "--beamsize=1024", *lex)[1]
