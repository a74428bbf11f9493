"""The restatement of the silence score (tests/beam_sil_ref.py) against the four existing restatements, against the enumeration of
every path on biased frame scores, on a case that tells "bias after selection" from "bias before selection", and the refusals of
the five w2l_*_beam_search*_sil entry points.  No GPU."""
import numpy as np
import pytest

from tests import asg_beam_ref as AR
from tests import beam_sil_ref as SR
from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR
from tests import ctc_beam_ref as CR
from tests.test_asg_beam_host import _asg_tiny
from tests.test_ctc_beam_lex_host import _tiny

INF = float("inf")
F32 = np.float32
SELECTION_SEED = 9
SEARCHES = ("ctc", "ctc_lm", "ctc_lex", "asg", "asg_lm", "asg_lex")   # asg and asg_lm are one entry point, two code paths


def _models(search, rng, N, eighths):
    """the keyword arguments of sil_beam_one for `search` over N classes, sil = token 2: random transitions, a random token LM
    with class scores, or a random lexicon with sil and a word LM smeared down it"""
    asg = search.startswith("asg")
    ntok = N if asg else N - 1
    kw = {}
    if asg:
        kw["A"] = (rng.integers(-12, 13, (N, N)) / 8).astype(F32) if eighths else rng.normal(0, 1.5, (N, N)).astype(F32)
    if search.endswith("_lm"):
        kw["lm"] = LR.random_lm(rng, ntok, 3, 30, eighths=eighths)
        kw["lm_weight"], kw["eos_score"] = 0.5, -0.25
        kw["class_score"] = (rng.integers(-8, 9, ntok) / 8).astype(F32)
    if search.endswith("_lex"):
        nwords = 12
        rows = XR.random_lexicon(rng, ntok, nwords, 3, 0.2, 2)
        tb = LR.random_lm(rng, nwords, 2, 30, eighths=eighths)
        smear = np.array([tb.score(tb.history(()), w, F32) for w in range(nwords)], F32)
        kw["trie"] = XR.TextbookTrie(rows, ntok, nwords, smear, 2)
        kw["lm"], kw["lm_weight"], kw["word_score"], kw["eos_score"] = tb, 0.5, -0.25, -0.5
    return kw


def _old(search, x, F, W, K, kw, threshold, log_add, normalize, dtype):
    """the existing restatement of `search`, as sil_beam_one's rows (labels, words, score, lm score, hypothesis)"""
    if search == "ctc":
        hyps, _ = CR.beam_search_one(x, F, W, K, threshold, log_add, normalize, dtype)
        return [(p, (), s, F32(0), tuple((c, None) for c in p)) for p, s in hyps]
    if search == "ctc_lm":
        hyps, _ = LR.beam_search_lm_one(x, F, W, K, kw["lm"], kw["lm_weight"], kw["class_score"], kw["eos_score"], threshold,
                                        log_add, normalize, dtype)
        return [(p, (), s, ls, tuple((c, None) for c in p)) for p, s, ls in hyps]
    if search == "ctc_lex":
        hyps, _ = XR.beam_search_lex_one(x, F, W, K, kw["trie"], kw["lm"], kw["lm_weight"], kw["word_score"], kw["eos_score"],
                                         threshold, log_add, normalize, dtype)
        return hyps
    if search == "asg_lex":
        hyps, _ = AR.asg_beam_lex_one(x, kw["A"], F, W, K, kw["trie"], kw["lm"], kw["lm_weight"], kw["word_score"], kw["eos_score"],
                                      threshold, log_add, normalize, dtype)
        return hyps
    hyps, _ = AR.asg_beam_one(x, kw["A"], F, W, K, kw.get("lm"), kw.get("lm_weight", 0.0), kw.get("class_score"),
                              kw.get("eos_score", 0.0), threshold, log_add, normalize, dtype)
    return [(p, (), s, ls, tuple((c, None) for c in p)) for p, s, ls in hyps]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[0] == w[0] and tuple(g[1]) == tuple(w[1]) and g[4] == w[4]
        assert type(g[2]) is type(w[2]) and g[2] == w[2] and F32(g[3]) == F32(w[3])


# ---- 1. silScore = 0 is the existing restatements -------------------------------------------------------------------------------

@pytest.mark.parametrize("W,K,thr,log_add", [(64, 64, INF, False), (6, 3, INF, True), (16, 4, 2.5, False), (1, 1, INF, True)])
@pytest.mark.parametrize("search", SEARCHES)
def test_zero_score_is_the_existing_restatement(search, W, K, thr, log_add):
    N, T = 7, 14
    rng = np.random.default_rng(W * 100 + K)
    kw = _models(search, rng, N, eighths=not log_add)
    dtype = np.float64 if log_add else F32
    for seed in range(3):
        x = np.random.default_rng(seed).normal(0, 2, size=(T, N)).astype(F32)
        want = _old(search, x, T - seed, W, K, kw, thr, log_add, log_add, dtype)
        for sil, score in ((2, 0.0), (-1, 3.0)):
            got, _ = SR.sil_beam_one(x, T - seed, W, K, sil, score, threshold=thr, log_add=log_add, normalize=log_add, dtype=dtype,
                                     **kw)
            _same(got, want)
    assert len(want) > 0 or search.endswith("_lex")


# ---- 2. I2: at K = all and normalize = 0 the new rule is the old search on emissions biased on the host in fp32 ---------------

@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("score", [-1.5, 0.75])
@pytest.mark.parametrize("search", SEARCHES)
def test_i2_equals_the_existing_restatement_on_biased_emissions(search, score, log_add):
    N, T, W = 7, 14, 8
    rng = np.random.default_rng(7)
    kw = _models(search, rng, N, eighths=False)
    hits = 0
    for seed in range(3):
        x = np.random.default_rng(seed).normal(0, 2, size=(T, N)).astype(F32)
        got, _ = SR.sil_beam_one(x, T, W, 64, 2, score, log_add=log_add, dtype=F32, **kw)
        _same(got, _old(search, SR.bias_column(x, 2, score), T, W, 64, kw, INF, log_add, False, F32))
        plain = _old(search, x, T, W, 64, kw, INF, log_add, False, F32)
        hits += [g[4] for g in got] != [p[4] for p in plain]
    assert hits > 0                                              # the score changed what the search finds


# ---- 3. at K = all the restatement equals the enumeration of every path on biased frame scores ---------------------------------

def _grid(rng, T, N):
    """emissions on a grid of 2^-10: x + silScore is exact in fp32, so the biased scores reach the enumeration unrounded"""
    return (np.round(rng.normal(0, 2, size=(T, N)) * 1024) / 1024).astype(F32)


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("score", [-1.5, 0.75])
@pytest.mark.parametrize("search", SEARCHES)
def test_restatement_equals_the_enumeration_on_biased_frame_scores(search, score, log_add):
    asg = search.startswith("asg")
    lmw, word_score, eos_score = 0.7, -0.3, -0.4
    kw, A = {}, None
    if search.endswith("_lex"):
        if asg:
            N, rows, sil, nwords = _asg_tiny(4)
        else:
            N = 4
            rows, sil, nwords = _tiny(N)
        T = 3
        ntok = N if asg else N - 1
        tb = LR.random_lm(np.random.default_rng(N * 10 + T), nwords, 3, 12)
        smear = np.array([tb.score(tb.history(()), w, F32) for w in range(nwords)], F32)
        trie = XR.TextbookTrie(rows, ntok, nwords, smear, sil)
        kw = dict(trie=trie, lm=tb, lm_weight=lmw, word_score=word_score, eos_score=eos_score)
    else:
        N, T, sil = 3, 4, 1
        ntok = N if asg else N - 1
        if search.endswith("_lm"):
            tb = LR.random_lm(np.random.default_rng(N * 10 + T), ntok, 3, 12)
            cls = np.random.default_rng(5).normal(0, 0.5, ntok)
            kw = dict(lm=tb, lm_weight=lmw, class_score=cls, eos_score=eos_score)
    worst, sil_seen = 0.0, 0
    for seed in range(3):
        rng = np.random.default_rng(seed + 3)
        x = _grid(rng, T, N)
        if asg:
            A = rng.normal(0, 1.5, size=(N, N)).astype(F32)
            kw["A"] = A
        hyps, dg = SR.sil_beam_one(x, T, 64, 64, sil, score, log_add=log_add, dtype=np.float64, lm_dtype=np.float64, **kw)
        assert dg.beam_gap == np.inf                             # W = 64 never binds here
        xb = SR.bias_column(x, sil, score)
        assert (xb.astype(np.float64)[:, sil] == x.astype(np.float64)[:, sil] + score).all()
        if search == "ctc":
            want = {tuple((c, None) for c in lab): s for lab, s in CR.enumerate_labellings(xb, log_add, False).items()}
        elif search == "ctc_lm":
            want = {tuple((c, None) for c in lab): s + lmw * float(tb.sentence(lab, np.float64)) + float(sum(cls[c] for c in lab)) + eos_score
                    for lab, s in CR.enumerate_labellings(xb, log_add, False).items()}
        elif search == "ctc_lex":
            want = XR.enumerate_hypotheses(xb, trie, tb, lmw, word_score, eos_score, log_add, False)
        elif search == "asg":
            want = {tuple((c, None) for c in lab): s for lab, s in AR.enumerate_labellings(xb, A, log_add, False).items()}
        elif search == "asg_lm":
            want = {tuple((c, None) for c in lab): s for lab, s in AR.enumerate_lm(xb, A, tb, lmw, cls, eos_score, log_add, False).items()}
        else:
            want = AR.enumerate_hypotheses(xb, A, trie, tb, lmw, word_score, eos_score, log_add, False)
        got = {h[4]: h[2] for h in hyps}
        assert set(got) == set(want) and len(hyps) == len(want)
        worst = max(worst, max(abs(got[h] - want[h]) for h in want))
        assert [h[4] for h in hyps] == sorted(want, key=lambda h: -want[h])
        sil_seen += sum(1 for h in got if any(c == sil for c, _ in h))
    print("enumeration", search, score, "logAdd", log_add, "hypotheses", len(want), "worst", worst, "with sil", sil_seen)
    assert worst <= 1e-9 and sil_seen > 0


# ---- 4. the rule is "after selection": a case in which biasing before selection changes the frame tokens -------------------

@pytest.mark.parametrize("score", [8.0, -8.0])
@pytest.mark.parametrize("search", SEARCHES)
def test_selection_case_tells_the_two_rules_apart(search, score):
    N, T, W, K, sil = (6 if search.startswith("asg") else 7), 16, 8, 3, 2
    ntok = N if search.startswith("asg") else N - 1
    # seed 9: every search differs in at least one utterance in both directions.  With -8 the old rule drops sil from the odd
    # frames' tokens and the new one keeps it 7 or more below the others, which shows only where such a candidate still enters the
    # beam of 8: not at every seed in every search.
    rng = np.random.default_rng(SELECTION_SEED)
    kw = _models(search, rng, N, eighths=True)
    x = SR.selection_case(rng, 3, T, N, sil, ntok)
    order = np.argsort(-x[..., :ntok], axis=-1, kind="stable")
    rank = (order == sil).argmax(axis=-1)
    assert (rank[:, 0::2] == ntok - 1).all() and (rank[:, 1::2] == 0).all()
    brank = (np.argsort(-SR.bias_column(x, sil, score)[..., :ntok], axis=-1, kind="stable") == sil).argmax(axis=-1)
    assert ((brank < K) != (rank < K)).any()                     # biasing first would change the frame tokens
    differ = 0
    for b in range(3):
        new, _ = SR.sil_beam_one(x[b], T, W, K, sil, score, dtype=F32, **kw)
        pre = _old(search, SR.bias_column(x[b], sil, score), T, W, K, kw, INF, False, False, F32)
        differ += [(h[4], h[2]) for h in new] != [(h[4], h[2]) for h in pre]
    assert differ > 0


# ---- 5. the C ABI: refusals before the device, workspace sizes ----------------------------------------------------------------

def _abi():
    from wav2letter_amd import _lib as L
    lib = L.lib()
    buf = np.zeros(64, np.uint8).ctypes.data                     # never read: every call below is refused first

    def ctc(fam=0, B=2, T=10, N=30, W=8, K=8, M=2, sil=2, score=-1.0, ws=buf, thr=INF):
        return lib.w2l_ctc_beam_search_sil(fam, B, T, N, buf, None, W, K, thr, 0, 0, M, 10, buf, buf, buf, ws, None, sil, score)

    def ctc_lm(fam=0, B=2, T=10, N=30, W=8, K=8, M=2, sil=2, score=-1.0, ws=buf, thr=INF, lm=buf):
        return lib.w2l_ctc_beam_search_lm_sil(fam, B, T, N, buf, None, W, K, thr, 0, 0, M, 10, lm, 1, 1.0, None, 0.0, buf, buf, buf,
                                              buf, ws, None, sil, score)

    def ctc_lex(fam=0, B=2, T=10, N=30, W=8, K=8, M=2, sil=2, score=-1.0, ws=buf, thr=INF, lm=buf):
        return lib.w2l_ctc_beam_search_lex_sil(fam, B, T, N, buf, None, W, K, thr, 0, 0, M, 10, lm, 1, 1.0, buf, 0.0, 0.0, buf, buf,
                                               buf, buf, 4, buf, buf, ws, None, sil, score)

    def asg(fam=0, B=2, T=10, N=30, W=8, K=8, M=2, sil=2, score=-1.0, ws=buf, thr=INF, lm=buf):
        return lib.w2l_asg_beam_search_sil(fam, B, T, N, buf, None, buf, W, K, thr, 0, 0, M, 10, lm, 1, 1.0, None, 0.0, buf, buf, buf,
                                           buf, ws, None, sil, score)

    def asg_lex(fam=0, B=2, T=10, N=30, W=8, K=8, M=2, sil=2, score=-1.0, ws=buf, thr=INF, lm=buf):
        return lib.w2l_asg_beam_search_lex_sil(fam, B, T, N, buf, None, buf, W, K, thr, 0, 0, M, 10, lm, 1, 1.0, buf, 0.0, 0.0, buf,
                                               buf, buf, buf, 4, buf, buf, ws, None, sil, score)

    sizes = dict(ctc=lib.w2l_ctc_beam_sil_workspace_size, ctc_lm=lib.w2l_ctc_beam_lm_sil_workspace_size,
                 ctc_lex=lib.w2l_ctc_beam_lex_sil_workspace_size, asg=lib.w2l_asg_beam_sil_workspace_size,
                 asg_lex=lib.w2l_asg_beam_lex_sil_workspace_size)
    return L, lib, dict(ctc=ctc, ctc_lm=ctc_lm, ctc_lex=ctc_lex, asg=asg, asg_lex=asg_lex), sizes


def test_sil_refusals_return_before_the_device():
    L, lib, calls, sizes = _abi()
    nan = float("nan")
    for name, f in calls.items():
        tokens = 30 if name.startswith("asg") else 29
        for kw in (dict(fam=-1), dict(fam=3), dict(score=nan), dict(score=INF), dict(score=-INF), dict(sil=-2), dict(sil=tokens),
                   dict(sil=tokens, score=0.0), dict(fam=3, sil=-1), dict(fam=3, score=0.0),
                   # the siblings' own W2L_EINVALs, with and without a score (without: through the sibling itself)
                   dict(ws=None), dict(ws=None, score=0.0), dict(ws=None, sil=-1), dict(thr=nan), dict(thr=-1.0), dict(M=9), dict(M=0),
                   dict(W=0), dict(K=0), dict(N=1), dict(B=0), dict(T=0), dict(W=0, fam=1), dict(W=0, fam=2)):
            assert f(**kw) == L.W2L_EINVAL, (name, kw)
        if name != "ctc":
            if name != "asg":
                assert f(lm=None) == L.W2L_EINVAL, name
            assert f(lm=None, fam=2) == L.W2L_EINVAL, name      # asg: lmHasEos without an LM
        assert f(sil=tokens - 1, ws=None) == L.W2L_EINVAL        # the last token is in range: the refusal is the workspace's
        # the families' limits, after every W2L_EINVAL: a bad silence argument wins over them
        for kw in (dict(fam=0, W=65), dict(fam=1, W=1025), dict(fam=2, W=8193), dict(fam=0, K=65, N=100), dict(fam=1, K=65, N=100),
                   dict(fam=2, K=65, N=100), dict(fam=0, W=65, score=0.0), dict(fam=1, W=1025, sil=-1), dict(fam=2, W=8193, score=0.0)):
            assert f(**kw) == L.W2L_EUNSUPPORTED, (name, kw)
            assert f(**dict(kw, sil=-2)) == L.W2L_EINVAL and f(**dict(kw, score=nan)) == L.W2L_EINVAL, (name, kw)
        assert f(fam=2, T=1 << 17, W=8192) == L.W2L_EUNSUPPORTED  # T * W > 2^29: node ids are ints


def test_sil_workspace_sizes():
    L, lib, _, sizes = _abi()
    sib = dict(ctc=("w2l_ctc_beam_lm", "w2l_ctc_beam_wide", "w2l_ctc_beam_xl"),       # narrow: the LM variant's (the token scan)
               ctc_lm=("w2l_ctc_beam_lm", "w2l_ctc_beam_lm_wide", "w2l_ctc_beam_lm_xl"),
               ctc_lex=("w2l_ctc_beam_lex", "w2l_ctc_beam_lex_wide", "w2l_ctc_beam_lex_xl"),
               asg=("w2l_asg_beam", "w2l_asg_beam_wide", "w2l_asg_beam_xl"),
               asg_lex=("w2l_asg_beam_lex", "w2l_asg_beam_lex_wide", "w2l_asg_beam_lex_xl"))
    for name, size in sizes.items():
        for fam, W in ((0, 64), (1, 1024), (2, 8192)):
            want = getattr(lib, sib[name][fam] + "_workspace_size")(3, 16, 7, W, 64)
            assert size(fam, 3, 16, 7, W, 64) == want > 0, (name, fam)
            assert size(fam, 3, 16, 7, W + 1, 64) == 0 and size(fam, 3, 16, 100, W, 65) == 0, (name, fam)
            assert size(fam, 0, 16, 7, 8, 8) == 0 and size(fam, 3, 0, 7, 8, 8) == 0 and size(fam, 3, 16, 1, 8, 8) == 0
            assert size(fam, 3, 16, 7, 0, 8) == 0 and size(fam, 3, 16, 7, 8, 0) == 0
        assert size(-1, 3, 16, 7, 8, 8) == 0 and size(3, 3, 16, 7, 8, 8) == 0
    assert sizes["ctc"](0, 3, 16, 7, 8, 8) > lib.w2l_ctc_beam_workspace_size(3, 16, 7, 8, 8)


def test_python_front_end_refuses_a_score_without_a_token():
    import torch
    from wav2letter_amd import _lib, criterion
    x = torch.zeros(1, 4, 7)
    with pytest.raises(_lib.W2LInvalidArgument, match="sil_score needs a silence token"):
        criterion.ctc_beam_search(x, sil_score=-1.0)
    with pytest.raises(_lib.W2LInvalidArgument, match="sil_score needs a silence token"):
        criterion.asg_beam_search(x, torch.zeros(7, 7), sil_score=0.5)
