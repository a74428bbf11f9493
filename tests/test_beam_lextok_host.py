"""The token LM under a lexicon (w2l_ctc_beam_search_lextok, w2l_asg_beam_search_lextok) without a GPU: the restatement
tests/beam_lextok_ref.py against an enumeration of every path and every segmentation, in both lattices and both logAdd modes; at
lmWeight = 0 against ctc_beam_lex_ref on an unsmeared lexicon; with a lexicon of one-token words against the token-LM
restatement; and the C ABI's refusals and workspace sizes through ctypes, none of which touches a device."""
import numpy as np
import pytest

from tests import asg_beam_ref as AR
from tests import beam_lextok_ref as TR
from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR

F32 = np.float32
INF = float("inf")
SIL = 2
# a word that is a prefix of another (0 of 1, 2), a homophone pair (1, 2), a spelling that ends in the silence token (3), a
# one-token word (0); tokens 0 .. 3, sil = 2
ROWS = [(0, [0]), (1, [0, 1]), (2, [0, 1]), (3, [1, 2]), (4, [3, 0]), (5, [1, 3, 0])]


def _tiny(ntok):
    trie = XR.TextbookTrie(ROWS, ntok, 6, None, SIL)
    sps = [tuple(sp) for _, sp in ROWS]
    assert any(a != b and a == b[:len(a)] for a in sps for b in sps) and len(set(sps)) == len(sps) - 1
    assert any(sp[-1] == SIL and len(sp) > 1 for sp in sps) and any(len(sp) == 1 for sp in sps)
    return trie


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("lattice,T", [("ctc", 5), ("asg", 5)])
def test_restatement_scores_every_hypothesis_as_the_enumeration_does(lattice, T, log_add):
    N = 5                                                        # CTC: 4 tokens and blank; ASG: 5 tokens, the last in no spelling
    asg = lattice == "asg"
    ntok = N if asg else N - 1
    trie = _tiny(ntok)
    rng = np.random.default_rng(50 + T + asg)
    tb = LR.random_lm(rng, ntok, 3, 14, drop_unigrams=(3,))      # back-off walks; token 3 scores as <unk>
    lmw, word_score, eos_score = 0.7, -0.3, -0.4
    worst, seen = 0.0, XR.LexDiag()
    for seed in range(3):
        r = np.random.default_rng(seed)
        x = r.normal(0, 2, size=(T, N)).astype(F32)
        A = r.normal(0, 1, size=(N, N)).astype(F32) if asg else None
        norm = log_add and not asg
        hyps, dg = TR.lextok_beam_one(x, T, 4096, ntok, trie, tb, lmw, word_score, eos_score, A=A, log_add=log_add, normalize=norm,
                                      dtype=np.float64, lm_dtype=np.float64)
        assert dg.beam_gap == np.inf                             # the beam never cuts
        want = TR.enumerate_lextok(x, trie, tb, lmw, word_score, eos_score, log_add, norm, A)
        got = {h[4]: h[2] for h in hyps}
        assert set(got) == set(want) and len(hyps) == len(want) > 10
        worst = max(worst, max(abs(got[h] - want[h]) for h in want))
        # rank order; two segmentations of one spelling into as many words tie exactly under a token LM, so ties are allowed
        assert all(want[a[4]] >= want[b[4]] - 1e-9 for a, b in zip(hyps, hyps[1:]))
        assert any(sum(1 for g in got if tuple(c for c, _ in g) == tuple(c for c, _ in h)) > 1 for h in got)   # one spelling, two hypotheses
        for h in hyps:                                           # the LM sum is the sentence score of the scored tokens
            assert h[3].view(np.int32) == tb.sentence(TR.lm_history(h[4], SIL), F32).view(np.int32)
        for k in ("merges", "blocked", "homophones", "sil_loops", "end_dropped"):
            setattr(seen, k, getattr(seen, k) + getattr(dg, k))
    print("enumeration", lattice, T, "logAdd", log_add, "hypotheses", len(want), "worst |score - enumeration|", worst,
          {k: getattr(seen, k) for k in ("merges", "blocked", "homophones", "sil_loops", "end_dropped")}, "unk hits", tb.unk_hits,
          "longest back-off chain", tb.max_chain)
    assert worst <= 1e-9
    assert seen.merges > 0 and seen.blocked > 0 and seen.homophones > 0 and seen.sil_loops > 0 and seen.end_dropped > 0
    assert tb.unk_hits > 0 and tb.max_chain > 0


def _case(seed, asg, B=3, T=14, N=9, nwords=20):
    rng = np.random.default_rng(seed)
    ntok = N if asg else N - 1
    x = (rng.integers(-24, 1, size=(B, T, N)) / 8).astype(F32)
    A = (rng.integers(-8, 9, size=(N, N)) / 8).astype(F32) if asg else None
    rows = XR.random_lexicon(rng, ntok, nwords, 3, 0.15, SIL, 6)
    tb = LR.random_lm(rng, ntok, 3, 40, eighths=True, drop_unigrams=(1,))
    return x, A, rows, tb, ntok


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("asg", [False, True])
def test_weight_zero_is_the_word_search_restatement_on_an_unsmeared_lexicon(asg, log_add):
    """lmWeight = 0, no EOS: labels, words and scores are ctc_beam_lex_ref's (asg_beam_ref's) with a word LM of weight 0"""
    x, A, rows, tb, ntok = _case(7 + asg, asg)
    trie = XR.TextbookTrie(rows, ntok, 20, None, SIL)
    tok_lm = LR.TextbookLM({g: (v, tb.bo.get(g, 0)) for g, v in tb.p.items() if g != (tb.eos,) and tb.eos not in g}, ntok, -6.0)
    word_lm = LR.random_lm(np.random.default_rng(1), 20, 2, 30, eos=False)
    assert not tok_lm.has_eos and not word_lm.has_eos
    frames, W, K, M = [14, 5, 9], 12, 5, 8
    dt = np.float64 if log_add else F32
    got = TR.lextok_beam(x, frames, W, K, M, 14, trie, tok_lm, 0.0, -0.5, 0.0, dt, 6, A=A, threshold=3.0, log_add=log_add)
    if asg:
        want = AR.asg_beam(x, A, frames, W, K, M, 14, dt, trie=trie, max_words=6, lm=word_lm, lm_weight=0.0, word_score=-0.5,
                           threshold=3.0, log_add=log_add)
    else:
        want = dict(zip(("labels", "lengths", "scores", "lm_scores", "words", "word_counts"),
                        XR.beam_search_lex(x, frames, W, K, trie, word_lm, 0.0, -0.5, 0.0, 3.0, log_add, False, M, 14, 6, dt)))
    assert (got["lengths"] >= 0).any() and (got["word_counts"] > 1).any()
    for k in ("labels", "lengths", "words", "word_counts"):
        assert (got[k] == want[k]).all(), k
    assert (got["scores"].view(np.int64 if log_add else np.int32) == want["scores"].view(np.int64 if log_add else np.int32)).all()
    assert any(d.beam_gap < INF for d in got["diags"])           # the beam binds


def test_one_token_words_are_the_token_lm_restatement():
    """every token a one-token word, no silence token, wordScore = 0: the token-LM search with classScore = NULL"""
    rng = np.random.default_rng(4)
    B, T, N, W, K, M = 3, 14, 12, 16, 5, 8
    x = (rng.integers(-24, 1, size=(B, T, N)) / 8).astype(F32)
    tb = LR.random_lm(rng, N - 1, 3, 40, eighths=True, drop_unigrams=(2,))
    trie = XR.TextbookTrie([(c, [c]) for c in range(N - 1)], N - 1, N - 1)
    got = TR.lextok_beam(x, [14, 5, 9], W, K, M, T, trie, tb, 0.5, 0.0, -0.5, F32, T, threshold=2.5)
    rlab, rln, rsc, rlms, _ = LR.beam_search_lm(x, [14, 5, 9], W, K, tb, 0.5, None, -0.5, 2.5, False, False, M, T, F32)
    assert (got["labels"] == rlab).all() and (got["lengths"] == rln).all() and (rln > 2).any()
    assert (got["scores"].view(np.int32) == rsc.view(np.int32)).all() and (got["lm_scores"].view(np.int32) == rlms.view(np.int32)).all()
    assert (got["words"] == got["labels"]).all() and (got["word_counts"] == got["lengths"]).all()


def test_smear_values_are_never_read():
    x, A, rows, tb, ntok = _case(11, False)
    plain = XR.TextbookTrie(rows, ntok, 20, None, SIL)
    smeared = XR.TextbookTrie(rows, ntok, 20, np.random.default_rng(0).uniform(-5, 0, 20).astype(F32), SIL)
    a = TR.lextok_beam(x, None, 8, 5, 8, 14, plain, tb, 0.5, -0.25, -0.25)
    b = TR.lextok_beam(x, None, 8, 5, 8, 14, smeared, tb, 0.5, -0.25, -0.25)
    assert all((a[k].view(np.int32) == b[k].view(np.int32)).all() for k in ("labels", "scores", "lm_scores", "words"))


# ---- the C ABI: refusals before the device, workspace sizes ---------------------------------------------------------------------

def _abi():
    from wav2letter_amd import _lib as L
    lib = L.lib()
    buf = np.zeros(64, np.uint8).ctypes.data                     # never read: every call below is refused first

    def ctc(fam=0, B=2, T=10, N=30, W=8, K=8, M=2, sil=2, score=-1.0, ws=buf, thr=INF, lm=buf, lex=buf, x=buf, out=buf, wsc=0.0,
            mw=4, eos=1, eosc=0.0, lmw=1.0):
        return lib.w2l_ctc_beam_search_lextok(fam, B, T, N, x, None, W, K, thr, 0, 0, M, 10, lm, eos, lmw, lex, wsc, eosc, out, buf,
                                              buf, buf, mw, buf, buf, ws, None, sil, score)

    def asg(fam=0, B=2, T=10, N=30, W=8, K=8, M=2, sil=2, score=-1.0, ws=buf, thr=INF, lm=buf, lex=buf, x=buf, out=buf, wsc=0.0,
            mw=4, eos=1, eosc=0.0, lmw=1.0, trans=buf):
        return lib.w2l_asg_beam_search_lextok(fam, B, T, N, x, None, trans, W, K, thr, 0, 0, M, 10, lm, eos, lmw, lex, wsc, eosc, out,
                                              buf, buf, buf, mw, buf, buf, ws, None, sil, score)

    return L, lib, dict(ctc=ctc, asg=asg), dict(ctc=lib.w2l_ctc_beam_lextok_workspace_size, asg=lib.w2l_asg_beam_lextok_workspace_size)


def test_lextok_refusals_return_before_the_device():
    L, lib, calls, _ = _abi()
    nan = float("nan")
    for name, f in calls.items():
        tokens = 30 if name == "asg" else 29
        for kw in (dict(fam=-1), dict(fam=3), dict(score=nan), dict(score=INF), dict(score=-INF), dict(sil=-2), dict(sil=tokens),
                   dict(sil=tokens, score=0.0), dict(wsc=nan), dict(wsc=INF), dict(lmw=nan), dict(eosc=-INF), dict(eos=0, eosc=1.0),
                   dict(lm=None), dict(lex=None), dict(x=None), dict(out=None), dict(ws=None), dict(ws=None, score=0.0),
                   dict(ws=None, sil=-1), dict(mw=0), dict(thr=nan), dict(thr=-1.0), dict(M=9), dict(M=0), dict(W=0), dict(K=0),
                   dict(N=1), dict(B=0), dict(T=0), dict(W=0, fam=1), dict(W=0, fam=2), dict(lm=None, fam=2), dict(fam=2, sil=-2),
                   dict(fam=-1, sil=-1, score=0.0)):
            assert f(**kw) == L.W2L_EINVAL, (name, kw)
        if name == "asg":
            assert f(trans=None) == L.W2L_EINVAL and f(trans=None, fam=1) == L.W2L_EINVAL
        assert f(sil=tokens - 1, ws=None) == L.W2L_EINVAL        # the last token is in range: the refusal is the workspace's
        # the xl family and the families' limits, after every W2L_EINVAL
        for kw in (dict(fam=2), dict(fam=2, score=0.0), dict(fam=2, sil=-1), dict(fam=2, W=2000), dict(fam=0, W=65), dict(fam=1, W=1025),
                   dict(fam=0, K=65, N=100), dict(fam=1, K=65, N=100), dict(fam=1, W=1025, sil=-1), dict(fam=1, T=1 << 20, W=1024)):
            assert f(**kw) == L.W2L_EUNSUPPORTED, (name, kw)
            assert f(**dict(kw, sil=-2)) == L.W2L_EINVAL and f(**dict(kw, wsc=nan)) == L.W2L_EINVAL, (name, kw)


def test_lextok_workspace_sizes():
    L, lib, _, sizes = _abi()
    sib = dict(ctc=("w2l_ctc_beam_lex", "w2l_ctc_beam_lex_wide"), asg=("w2l_asg_beam_lex", "w2l_asg_beam_lex_wide"))
    for name, size in sizes.items():
        for fam, W in ((0, 64), (1, 1024)):
            want = getattr(lib, sib[name][fam] + "_workspace_size")(3, 16, 7, W, 64)
            assert size(fam, 3, 16, 7, W, 64) == want > 0, (name, fam)
            assert size(fam, 3, 16, 7, W + 1, 64) == 0 and size(fam, 3, 16, 100, W, 65) == 0, (name, fam)
            assert size(fam, 0, 16, 7, 8, 8) == 0 and size(fam, 3, 0, 7, 8, 8) == 0 and size(fam, 3, 16, 1, 8, 8) == 0
            assert size(fam, 3, 16, 7, 0, 8) == 0 and size(fam, 3, 16, 7, 8, 0) == 0
        assert size(2, 3, 16, 7, 8, 8) == 0 and size(-1, 3, 16, 7, 8, 8) == 0 and size(3, 3, 16, 7, 8, 8) == 0


def test_python_front_end_refusals():
    import torch
    from wav2letter_amd import Lexicon, NGramLM, criterion
    tb = LR.random_lm(np.random.default_rng(0), 6, 2, 10)
    lm6 = NGramLM.from_ngrams(tb.arrays(), 6, -6.0)
    tb5 = LR.random_lm(np.random.default_rng(0), 5, 2, 10)
    lm5 = NGramLM.from_ngrams(tb5.arrays(), 5, -6.0)
    lex = Lexicon.from_spellings([(0, [0]), (1, [1, 3])], 6, 2, None, 2)
    x, A = torch.zeros(1, 4, 7), torch.zeros(6, 6)
    with pytest.raises(ValueError, match="lm_token=True needs lexicon"):
        criterion.ctc_beam_search(x, lm=lm6, lm_weight=1.0, lm_token=True)
    with pytest.raises(ValueError, match="lm_token=True needs lexicon"):
        criterion.asg_beam_search(x[:, :, :6], A, lm=lm6, lm_weight=1.0, lm_token=True)
    with pytest.raises(ValueError, match="the LM has 5 tokens, the lexicon 6"):
        criterion.ctc_beam_search(x, lm=lm5, lexicon=lex, lm_token=True)
    with pytest.raises(ValueError, match="the LM has 5 tokens, the lexicon 6"):
        criterion.asg_beam_search(x[:, :, :6], A, lm=lm5, lexicon=lex, lm_token=True)
