"""The wide beam searches (w2l_*_beam_search*_wide, W up to 1024) without a GPU: the five twins exist, size their workspaces and
refuse bad arguments in their siblings' order before anything touches the device; the siblings still refuse W = 65; and the numpy
restatements of the four contracts (tests/*_beam_ref.py, generic in W), which are the oracle of tests/test_gpu_beam_wide.py, are
sound above 64 entries on N = 5, T = 6.  That shape has 2065 CTC labellings and 6825 ASG ones (counted and asserted below), more than
W = 300 holds: at W = 300 each restatement returns 300 distinct hypotheses, every one of them a hypothesis of the enumeration of
all N^T paths with a score that does not exceed the enumeration's (a beam scores a subset of a labelling's paths) and the best of
them with exactly the enumeration's best score; at a width that holds them all (W = 65536) it returns every one with the
enumeration's score, in the enumeration's order."""
import numpy as np
import pytest

from tests import asg_beam_ref as AR
from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR
from tests import ctc_beam_ref as R

INF = float("inf")
F32 = np.float32
NAN = float("nan")

# name: (sibling, workspace size of the twin, of the sibling, has trans, has LM arguments, has lexicon arguments)
TWINS = {
    "w2l_ctc_beam_search_wide": ("w2l_ctc_beam_search", "w2l_ctc_beam_wide_workspace_size", "w2l_ctc_beam_workspace_size", 0, 0, 0),
    "w2l_ctc_beam_search_lm_wide": ("w2l_ctc_beam_search_lm", "w2l_ctc_beam_lm_wide_workspace_size", "w2l_ctc_beam_lm_workspace_size",
                                    0, 1, 0),
    "w2l_ctc_beam_search_lex_wide": ("w2l_ctc_beam_search_lex", "w2l_ctc_beam_lex_wide_workspace_size",
                                     "w2l_ctc_beam_lex_workspace_size", 0, 1, 1),
    "w2l_asg_beam_search_wide": ("w2l_asg_beam_search", "w2l_asg_beam_wide_workspace_size", "w2l_asg_beam_workspace_size", 1, 1, 0),
    "w2l_asg_beam_search_lex_wide": ("w2l_asg_beam_search_lex", "w2l_asg_beam_lex_wide_workspace_size",
                                     "w2l_asg_beam_lex_workspace_size", 1, 1, 1),
}


def _L():
    from wav2letter_amd import _lib
    return _lib


def _caller(name):
    """call(**overrides) of entry point `name` (a twin or a sibling: one argument list) on host pointers that are never read"""
    L = _L()
    fn = getattr(L.lib(), name)
    _, _, _, trans, has_lm, has_lex = TWINS[name if name in TWINS else name + "_wide"]
    buf = np.zeros(64, np.uint8).ctypes.data

    def call(B=2, T=10, N=30, x=buf, tr=buf, W=8, K=8, thr=INF, M=2, Lmax=10, lm=buf, has_eos=1, lmw=1.0, cs=None, lex=buf, wsc=0.0,
             eos=0.0, labels=buf, lengths=buf, scores=buf, lms=buf, maxw=4, words=buf, counts=buf, ws=buf):
        args = [B, T, N, x, None] + ([tr] if trans else []) + [W, K, thr, 0, 0, M, Lmax]
        if has_lex:
            args += [lm, has_eos, lmw, lex, wsc, eos, labels, lengths, scores, lms, maxw, words, counts]
        elif has_lm:
            args += [lm, has_eos, lmw, cs, eos, labels, lengths, scores, lms]
        else:
            args += [labels, lengths, scores]
        return fn(*args, ws, None)
    return call


@pytest.mark.parametrize("name", list(TWINS))
def test_twin_exists_sizes_its_workspace_and_refuses_as_its_sibling(name):
    L = _L()
    sibling, size_name, sib_size_name, trans, has_lm, has_lex = TWINS[name]
    assert {name, size_name} <= set(L.exported_symbols())
    size, sib_size = getattr(L.lib(), size_name), getattr(L.lib(), sib_size_name)
    # W = 65 and W = 1024 are accepted, the size is monotone in W (and in B, T, K); beyond the limits: 0
    s = [size(2, 10, 100, W, 8) for W in (1, 64, 65, 100, 1024)]
    assert s[0] > 0 and all(a < b for a, b in zip(s, s[1:])), s
    assert size(2, 10, 100, 1025, 8) == 0 and size(2, 10, 100, 8, 65) == 0 and size(2, 10, 100, 1024, 64) > 0
    assert size(0, 10, 30, 8, 8) == 0 and size(2, 0, 30, 8, 8) == 0 and size(2, 10, 1, 8, 8) == 0 and size(2, 10, 30, 0, 8) == 0
    assert size(2, 10, 30, 100, 8) < size(4, 10, 30, 100, 8) and size(2, 10, 30, 100, 8) < size(2, 20, 30, 100, 8)
    assert size(2, 10, 100, 100, 8) < size(2, 10, 100, 100, 64)
    tokens = 30 if trans else 29
    assert size(2, 10, 30, 100, tokens) == size(2, 10, 30, 100, 64) == size(2, 10, 30, 100, 250000)     # K is clipped
    assert sib_size(2, 10, 100, 65, 8) == 0 and sib_size(2, 10, 100, 64, 8) > 0                          # the sibling's limit stays

    call, sib = _caller(name), _caller(sibling)
    bad = [dict(B=0), dict(T=0), dict(N=1), dict(B=-1), dict(x=None), dict(labels=None), dict(lengths=None), dict(scores=None),
           dict(ws=None), dict(W=0), dict(K=0), dict(M=0), dict(M=9), dict(Lmax=0), dict(thr=-0.5), dict(thr=NAN), dict(thr=-INF),
           dict(W=100, M=101), dict(W=1024, M=1025)]
    if trans:
        bad += [dict(tr=None)]
    if has_lm:
        bad += [dict(lms=None), dict(lmw=INF), dict(lmw=NAN), dict(eos=NAN), dict(eos=-INF), dict(has_eos=0, eos=0.5)]
        bad += [dict(lm=None, has_eos=1)] if trans and not has_lex else [dict(lm=None)]
    if has_lex:
        bad += [dict(lex=None), dict(words=None), dict(counts=None), dict(maxw=0), dict(wsc=NAN), dict(wsc=INF)]
    for kw in bad:
        assert call(**kw) == L.W2L_EINVAL, kw
    for kw in (dict(W=1025, M=2), dict(W=5000, M=2), dict(N=100, K=65), dict(N=100, K=250000), dict(N=100, W=1024, K=65)):
        assert call(**kw) == L.W2L_EUNSUPPORTED, kw
    # every W2L_EINVAL comes before W2L_EUNSUPPORTED
    for kw in (dict(W=1025, x=None), dict(W=1025, thr=-1.0), dict(W=1025, M=1026), dict(N=100, K=65, ws=None), dict(W=1025, Lmax=0)):
        assert call(**kw) == L.W2L_EINVAL, kw
    if has_lm:
        assert call(W=1025, lms=None) == L.W2L_EINVAL and call(W=1025, lmw=NAN) == L.W2L_EINVAL
    if has_lex:
        assert call(W=1025, lex=None) == L.W2L_EINVAL and call(N=100, K=65, maxw=0) == L.W2L_EINVAL
    # the sibling still refuses what the twin takes, and M up to W is the twin's alone
    assert sib(W=65, M=2) == L.W2L_EUNSUPPORTED and sib(W=1024, M=2) == L.W2L_EUNSUPPORTED
    assert sib(W=65, x=None) == L.W2L_EINVAL


# ---- the oracle above 64 entries ----------------------------------------------------------------------------------------------

N5, T6 = 5, 6
WIDTHS = [300, 1 << 16]


def _lexicon(tokens):
    """homophones on one spelling, a word that is a prefix of another, a two- and a three-token word, silence = token 3"""
    rows = [(0, [0]), (1, [0]), (2, [0, 1]), (3, [1]), (4, [2, 1]), (5, [2]), (6, [1, 2, 0])]
    return rows, 3, 7


def _check(W, hyps, want, key, score):
    """W holds the enumeration: every hypothesis of it, its score, its order.  W binds: W distinct hypotheses of the enumeration in
    descending order, none above its enumerated score, the first one the enumeration's best.  Either way more than 64 of them"""
    got = {key(h): score(h) for h in hyps}
    assert len(hyps) == len(got) > 64 and set(got) <= set(want)
    assert len(hyps) == len(want) if W >= len(want) else len(hyps) <= W       # with a lexicon entries inside a word leave at the end
    assert all(score(a) >= score(b) for a, b in zip(hyps, hyps[1:]))
    if W >= len(want):
        assert max(abs(got[h] - want[h]) for h in want) <= 1e-9
        assert all(want[key(a)] >= want[key(b)] - 1e-9 for a, b in zip(hyps, hyps[1:]))   # its order, up to exact ties (homophones)
    else:
        assert all(got[h] <= want[h] + 1e-9 for h in got)
        best = max(want, key=lambda h: want[h])
        assert key(hyps[0]) == best and abs(got[best] - want[best]) <= 1e-9
    return len(want)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("log_add", [False, True])
def test_restatements_above_64_entries_against_the_enumeration(log_add, W):
    rng = np.random.default_rng(56)
    x = rng.normal(0, 2, size=(T6, N5)).astype(F32)
    A = rng.normal(0, 1.5, size=(N5, N5)).astype(F32)
    counts = {}
    # CTC, LM-free
    hyps, dg = R.beam_search_one(x, T6, W, N5 - 1, INF, log_add, log_add, np.float64)
    counts["ctc"] = _check(W, hyps, R.enumerate_labellings(x, log_add, log_add), lambda h: h[0], lambda h: h[1])
    assert (dg.beam_gap == INF) == (W == 1 << 16)
    # CTC, token LM
    tb = LR.random_lm(rng, N5 - 1, 3, 12)
    cs = rng.normal(0, 0.5, N5 - 1).astype(F32)
    hyps, dg = LR.beam_search_lm_one(x, T6, W, N5 - 1, tb, 0.7, cs, -0.4, INF, log_add, log_add, np.float64, None, np.float64)
    want = {lab: s + 0.7 * float(tb.sentence(lab, np.float64)) + float(sum(np.float64(cs[c]) for c in lab)) - 0.4
            for lab, s in R.enumerate_labellings(x, log_add, log_add).items()}
    counts["ctc_lm"] = _check(W, hyps, want, lambda h: h[0], lambda h: h[1])
    assert (dg.beam_gap == INF) == (W == 1 << 16) and dg.merges > 0
    # CTC, lexicon
    rows, sil, nwords = _lexicon(N5 - 1)
    tw = LR.random_lm(rng, nwords, 3, 14)
    smear = np.array([tw.score(tw.history(()), w, F32) for w in range(nwords)], F32)
    trie = XR.TextbookTrie(rows, N5 - 1, nwords, smear, sil)
    hyps, dg = XR.beam_search_lex_one(x, T6, W, N5 - 1, trie, tw, 0.7, -0.3, -0.4, INF, log_add, log_add, np.float64, None,
                                      lm_dtype=np.float64)
    counts["ctc_lex"] = _check(W, hyps, XR.enumerate_hypotheses(x, trie, tw, 0.7, -0.3, -0.4, log_add, log_add), lambda h: h[4],
                               lambda h: h[2])
    assert (dg.beam_gap == INF) == (W == 1 << 16) and dg.merges > 0 and dg.homophones > 0 and dg.sil_loops > 0
    # ASG, LM-free and with a token LM
    hyps, dg = AR.asg_beam_one(x, A, T6, W, N5, None, 0.0, None, 0.0, INF, log_add, log_add, np.float64)
    counts["asg"] = _check(W, hyps, AR.enumerate_labellings(x, A, log_add, log_add), lambda h: h[0], lambda h: h[1])
    assert (dg.cuts == 0) == (W == 1 << 16) and dg.merges > 0
    ta = LR.random_lm(rng, N5, 3, 12)
    ca = rng.normal(0, 0.5, N5).astype(F32)
    hyps, dg = AR.asg_beam_one(x, A, T6, W, N5, ta, 0.7, ca, -0.4, INF, log_add, log_add, np.float64, lm_dtype=np.float64)
    counts["asg_lm"] = _check(W, hyps, AR.enumerate_lm(x, A, ta, 0.7, ca.astype(np.float64), -0.4, log_add, log_add), lambda h: h[0],
                              lambda h: h[1])
    assert (dg.cuts == 0) == (W == 1 << 16)
    # ASG, lexicon (over 5 tokens; token 4 spells nothing)
    trie5 = XR.TextbookTrie(rows, N5, nwords, smear, sil)
    hyps, dg = AR.asg_beam_lex_one(x, A, T6, W, N5, trie5, tw, 0.7, -0.3, -0.4, INF, log_add, log_add, np.float64, None,
                                   lm_dtype=np.float64)
    counts["asg_lex"] = _check(W, hyps, AR.enumerate_hypotheses(x, A, trie5, tw, 0.7, -0.3, -0.4, log_add, log_add), lambda h: h[4],
                               lambda h: h[2])
    assert (dg.cuts == 0) == (W == 1 << 16) and dg.merges > 0
    print("hypotheses at N = 5, T = 6:", counts)
    assert counts["ctc"] == counts["ctc_lm"] == 2065 and counts["asg"] == counts["asg_lm"] == 6825
    assert counts["ctc_lex"] > 64 and counts["asg_lex"] > 64
