"""The restatements of the ASG beam searches (tests/asg_beam_ref.py) against the enumeration of every path, against the CTC
restatements under zero transitions, the refusals of w2l_asg_beam_search / w2l_asg_beam_search_lex, and Lexicon.from_file's
replabel packing against its C++ twin.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import asg_beam_ref as AR
from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR
from tests import ctc_beam_ref as CR
from tests.test_ctc_beam_lex_host import _tiny

INF = float("inf")
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pkg():
    from wav2letter_amd import Lexicon, NGramLM, _lib
    return Lexicon, NGramLM, _lib


def _case(N, T, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 2, size=(T, N)).astype(F32), rng.normal(0, 1.5, size=(N, N)).astype(F32)


# ---- 1. the restatements against the enumeration of every path: only where W never cuts (45 labellings at N = 3, T = 4) ----------

SHAPES = [(3, 4), (3, 2), (2, 8), (2, 1)]


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("N,T", SHAPES)
def test_restatement_ranks_every_labelling_as_the_enumeration_does(N, T, log_add):
    worst = 0.0
    for seed in range(4):
        x, A = _case(N, T, seed * 7 + N)
        hyps, dg = AR.asg_beam_one(x, A, T, 64, N, None, 0.0, None, 0.0, INF, log_add, log_add, np.float64)
        want = AR.enumerate_labellings(x, A, log_add, log_add)
        assert dg.cuts == 0 and dg.beam_gap == np.inf
        got = {h[0]: h[1] for h in hyps}
        assert set(got) == set(want) and len(hyps) == len(want)
        assert all(a != b for lab in got for a, b in zip(lab, lab[1:]))           # no token after itself
        worst = max(worst, max(abs(got[h] - want[h]) for h in want))
        assert [h[0] for h in hyps] == sorted(want, key=lambda h: -want[h])
        assert (T == 1 or dg.skipped > 0) and (T <= 2 or dg.merges > 0)                # a merge needs a third frame
    print("enumeration", (N, T), "logAdd", log_add, "labellings", len(want), "worst |score - enumeration|", worst)
    assert worst <= 1e-9


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("N,T", [(3, 4), (2, 8)])
def test_restatement_with_an_lm_ranks_as_the_enumeration_with_the_textbook_lm(N, T, log_add):
    rng = np.random.default_rng(N + T)
    tb = LR.random_lm(rng, N, 3, 12)
    cs = rng.normal(0, 0.5, N).astype(F32)
    worst = 0.0
    for seed in range(3):
        x, A = _case(N, T, seed + 40)
        hyps, dg = AR.asg_beam_one(x, A, T, 64, N, tb, 0.7, cs, -0.4, INF, log_add, log_add, np.float64, lm_dtype=np.float64)
        want = AR.enumerate_lm(x, A, tb, 0.7, cs.astype(np.float64), -0.4, log_add, log_add)
        assert dg.cuts == 0
        got = {h[0]: h[1] for h in hyps}
        assert set(got) == set(want)
        worst = max(worst, max(abs(got[h] - want[h]) for h in want))
        assert [h[0] for h in hyps] == sorted(want, key=lambda h: -want[h])
    print("enumeration with LM", (N, T), "logAdd", log_add, "worst", worst)
    assert worst <= 1e-9


def _asg_tiny(name):
    """tokens, rows, sil, words.  The first two are test_ctc_beam_lex_host's lexicons over their N - 1 tokens (their doubled
    spellings are unreachable here); `asg` has a homophone pair, a word that is a prefix of another, silence inside a spelling, a
    word that starts with the token another ends on, and one unreachable word"""
    if name == "asg":
        rows = [(0, [0]), (1, [0]), (2, [0, 1]), (3, [1, 0]), (4, [1, 2, 0]), (5, [1, 1])]
        return 3, rows, 2, 6
    rows, sil, nwords = _tiny(name)
    return name - 1, rows, sil, nwords


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("name,T", [(3, 5), (4, 3), ("asg", 3)])
def test_lexicon_restatement_scores_every_hypothesis_as_the_enumeration_does(name, T, log_add):
    N, rows, sil, nwords = _asg_tiny(name)
    rng = np.random.default_rng(T * 10 + N)
    tb = LR.random_lm(rng, nwords, 3, 12)
    lmw, word_score, eos_score = 0.7, -0.3, -0.4
    smear = np.array([tb.score(tb.history(()), w, F32) for w in range(nwords)], F32)
    trie = XR.TextbookTrie(rows, N, nwords, smear, sil)
    worst, merges, dropped = 0.0, 0, 0
    for seed in range(3):
        x, A = _case(N, T, seed + 3)
        hyps, dg = AR.asg_beam_lex_one(x, A, T, 64, N, trie, tb, lmw, word_score, eos_score, INF, log_add, log_add, np.float64,
                                       None, lm_dtype=np.float64)
        assert dg.cuts == 0
        assert dg.unreachable == len({w for w, sp in rows if any(a == b for a, b in zip(sp, sp[1:]))}) > 0
        want = AR.enumerate_hypotheses(x, A, trie, tb, lmw, word_score, eos_score, log_add, log_add)
        got = {h[4]: h[2] for h in hyps}
        assert set(got) == set(want) and len(hyps) == len(want)
        assert not any(w in h[1] for h in hyps for w, sp in rows if any(a == b for a, b in zip(sp, sp[1:])))
        worst = max(worst, max(abs(got[h] - want[h]) for h in want))
        assert [h[4] for h in hyps] == sorted(want, key=lambda h: -want[h])
        merges += dg.merges
        dropped += dg.end_dropped
    print("lexicon enumeration", (name, T), "logAdd", log_add, "hypotheses", len(want), "worst", worst, "merges", merges)
    assert worst <= 1e-9 and merges > 0 and (name == 3 or dropped > 0)


# ---- 2. identity (i): zero transitions reduce to CTC with a -inf blank column, byte for byte, both (+) modes ------------------

def _with_blank(x):
    return np.concatenate([x, np.full(x.shape[:-1] + (1,), -np.inf, F32)], axis=-1)


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("W,K,thr", [(64, 64, INF), (6, 3, INF), (16, 5, 2.5), (1, 1, INF)])
def test_zero_transitions_are_the_ctc_restatements(W, K, thr, log_add):
    rng = np.random.default_rng(W + K)
    B, T, N, M = 5, 12, 9, min(W, 8)
    frames = [12, 5, 9, 1, 12]
    x = (rng.integers(-24, 1, size=(B, T, N)) / 8).astype(F32) if not log_add else rng.normal(0, 2, size=(B, T, N)).astype(F32)
    A = np.zeros((N, N), F32)
    xb = _with_blank(x)
    a = AR.asg_beam(x, A, frames, W, K, M, T, threshold=thr, log_add=log_add)
    lab, ln, sc, _ = CR.beam_search(xb, frames, W, K, thr, log_add, False, M, T, F32)
    assert np.array_equal(a["labels"], lab) and np.array_equal(a["lengths"], ln) and np.array_equal(a["scores"], sc)
    assert (a["lm_scores"][ln >= 0] == 0).all() and np.isneginf(a["lm_scores"][ln < 0]).all()
    tb = LR.random_lm(rng, N, 3, 40, eighths=not log_add)
    cs = (rng.integers(-8, 8, N) / 8).astype(F32)
    a = AR.asg_beam(x, A, frames, W, K, M, T, lm=tb, lm_weight=0.5, class_score=cs, eos_score=-0.5, threshold=thr, log_add=log_add)
    lab, ln, sc, lms, _ = LR.beam_search_lm(xb, frames, W, K, tb, 0.5, cs, -0.5, thr, log_add, False, M, T, F32)
    assert np.array_equal(a["labels"], lab) and np.array_equal(a["lengths"], ln) and np.array_equal(a["scores"], sc)
    assert np.array_equal(a["lm_scores"], lms)
    nwords = 30
    rows = XR.random_lexicon(rng, N, nwords, 3, 0.2, N - 1, hot=5)
    wtb = LR.random_lm(rng, nwords, 2, 30, eighths=not log_add)
    smear = np.array([wtb.score(wtb.history(()), w, F32) for w in range(nwords)], F32)
    trie = XR.TextbookTrie(rows, N, nwords, smear, N - 1)
    a = AR.asg_beam(x, A, frames, W, K, M, T, trie=trie, lm=wtb, lm_weight=0.5, word_score=0.25, eos_score=-0.5, threshold=thr,
                    log_add=log_add)
    lab, ln, sc, lms, wd, wc, _ = XR.beam_search_lex(xb, frames, W, K, trie, wtb, 0.5, 0.25, -0.5, thr, log_add, False, M, T, T, F32)
    for k, v in (("labels", lab), ("lengths", ln), ("scores", sc), ("lm_scores", lms), ("words", wd), ("word_counts", wc)):
        assert np.array_equal(a[k], v), k


def test_restatement_max_mode_is_viterbi_where_the_beam_never_binds():
    for seed in range(6):
        x, A = _case(3, 4, seed + 90)
        path, score = AR.viterbi(x, A)
        hyps, dg = AR.asg_beam_one(x, A, 4, 64, 3)
        assert dg.cuts == 0 and hyps[0][0] == AR.collapse(path) and hyps[0][1].view(np.int32) == score.view(np.int32)


# ---- 3. refusals of the C ABI, before anything touches the device -----------------------------------------------------------

def test_search_refusals_return_before_the_device():
    _, _, L = _pkg()
    lib = L.lib()
    buf = np.zeros(64, np.uint8).ctypes.data                                    # never read: every call below is refused first
    nan = float("nan")

    def plain(B=2, T=10, N=30, x=buf, tr=buf, W=8, K=8, thr=INF, M=2, Lmax=10, lm=buf, has_eos=1, lmw=1.0, cs=None, eos=0.0,
              labels=buf, lengths=buf, scores=buf, lms=buf, ws=buf):
        return lib.w2l_asg_beam_search(B, T, N, x, None, tr, W, K, thr, 0, 0, M, Lmax, lm, has_eos, lmw, cs, eos, labels, lengths,
                                       scores, lms, ws, None)

    def lex(B=2, T=10, N=30, x=buf, tr=buf, W=8, K=8, thr=INF, M=2, Lmax=10, lm=buf, has_eos=1, lmw=1.0, lx=buf, wsc=0.0, eos=0.0,
            labels=buf, lengths=buf, scores=buf, lms=buf, maxw=4, words=buf, counts=buf, ws=buf):
        return lib.w2l_asg_beam_search_lex(B, T, N, x, None, tr, W, K, thr, 0, 0, M, Lmax, lm, has_eos, lmw, lx, wsc, eos, labels,
                                           lengths, scores, lms, maxw, words, counts, ws, None)

    shared = (dict(tr=None), dict(lms=None), dict(x=None), dict(labels=None), dict(lengths=None), dict(scores=None), dict(ws=None),
              dict(lmw=INF), dict(lmw=nan), dict(eos=nan), dict(eos=-INF), dict(has_eos=0, eos=0.5), dict(thr=nan), dict(thr=-1.0),
              dict(M=9), dict(M=0), dict(W=0), dict(K=0), dict(Lmax=0), dict(N=1), dict(B=0), dict(T=0))
    for kw in shared + (dict(lm=None, has_eos=1), dict(lm=None, has_eos=0, eos=0.5), dict(lm=None, has_eos=1, eos=0.5),
                        dict(lm=None, has_eos=0, cs=buf)):
        assert plain(**kw) == L.W2L_EINVAL, kw
    for kw in shared + (dict(lx=None), dict(words=None), dict(counts=None), dict(maxw=0), dict(wsc=nan), dict(wsc=INF), dict(lm=None)):
        assert lex(**kw) == L.W2L_EINVAL, kw
    for f in (plain, lex):
        for kw in (dict(W=65, M=2), dict(K=65, N=100)):
            assert f(**kw) == L.W2L_EUNSUPPORTED, kw
    for size in (lib.w2l_asg_beam_workspace_size, lib.w2l_asg_beam_lex_workspace_size):
        assert size(2, 10, 30, 65, 8) == 0 and size(2, 10, 100, 8, 65) == 0 and size(0, 10, 30, 8, 8) == 0
        assert size(8, 100, 30, 8, 65) == size(8, 100, 30, 8, 30) > size(8, 100, 30, 8, 29)     # K clipped to N, not N - 1
    assert lib.w2l_asg_beam_workspace_size(2, 10, 31, 8, 8) == lib.w2l_ctc_beam_lm_workspace_size(2, 10, 31, 8, 8)


def test_python_front_end_refuses_bad_options_before_the_device():
    import torch
    from wav2letter_amd import criterion
    Lexicon, NGramLM, L = _pkg()
    x, A = torch.zeros(1, 4, 6), torch.zeros(6, 6)
    rng = np.random.default_rng(0)

    def lm(nw, eos=True):
        tb = LR.random_lm(rng, nw, 2, 5, eos=eos)
        return NGramLM.from_ngrams(tb.arrays(), nw, float(tb.unk))

    lex = Lexicon.from_spellings([(0, [0, 1]), (1, [2]), (2, [4])], 6, 3)
    with pytest.raises(ValueError, match=r"transitions must be float32 \[6\]\[6\]"):
        criterion.asg_beam_search(x, torch.zeros(5, 5))
    with pytest.raises(ValueError, match="the LM has 5 tokens, the emissions 6"):
        criterion.asg_beam_search(x, A, lm=lm(5))
    with pytest.raises(ValueError, match="the lexicon has 5 tokens, the emissions 6"):
        criterion.asg_beam_search(x, A, lexicon=Lexicon.from_spellings([(0, [0])], 5, 3), lm=lm(3))
    with pytest.raises(ValueError, match="lexicon needs lm"):
        criterion.asg_beam_search(x, A, lexicon=lex)
    with pytest.raises(ValueError, match="need lm"):
        criterion.asg_beam_search(x, A, lm_weight=0.5)
    with pytest.raises(ValueError, match="eos_score needs a model with EOS"):
        criterion.asg_beam_search(x, A, lm=lm(6, eos=False), eos_score=1.0)
    with pytest.raises(L.W2LError, match="GPU only"):                 # a well-formed call on CPU tensors: no CPU fallback
        criterion.asg_beam_search(x, A, lm=lm(6), lm_weight=0.5)


# ---- 4. Lexicon.from_file(replabel=) against its C++ twin ----------------------------------------------------------------------

@pytest.mark.parametrize("replabel", [1, 2])
def test_from_file_packs_replabels_as_the_cpp_header_does(tmp_path, replabel):
    """include/fl_compat/lexicon.h (Lexicon::fromFile(..., replabel)) through tests/cpp/lexicon_replabel_test.cpp compiled here
    with g++, and the Python front end, on the same file: the same table node for node, and the spellings are the packed ones"""
    from wav2letter_amd import text
    Lexicon, _, _ = _pkg()
    exe, libdir = str(tmp_path / "lexicon_replabel_test"), os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "lexicon_replabel_test.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    tokens = ["|", "a", "e", "h", "l", "o"] + [text.replabel_token(r) for r in range(1, replabel + 1)]
    lines = ["aaa a a a |", "hello h e l l o |", "aa a a |", "aaaa a a a a |", "ole o l e |", "hell h e l l |", "all a l l |", "a a |"]
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n")
    (tmp_path / "lex.txt").write_text("\n".join(lines) + "\n")
    d = text.Dictionary(tokens)
    lex = Lexicon.from_file(tmp_path / "lex.txt", d, smearing="none", sil="|", replabel=replabel)
    plain = Lexicon.from_file(tmp_path / "lex.txt", tokens, smearing="none", sil="|")
    assert np.array_equal(plain.blob, Lexicon.from_file(tmp_path / "lex.txt", tokens, smearing="none", sil="|", replabel=0).blob)
    assert not np.array_equal(lex.blob, plain.blob) and lex.num_tokens == len(tokens)

    def walk(lx, spelling):
        node = 0
        for t in spelling:
            node = lx.child(node, d.get_index(t))
            if node < 0:
                return None
        return [lx.words[w] for w in lx.node(node)[1]]

    r1 = text.replabel_token(1)
    assert walk(lex, ["h", "e", "l", r1, "o", "|"]) == ["hello"] and walk(lex, ["h", "e", "l", "l"]) is None
    aaa = ["a", "<2>", "|"] if replabel == 2 else ["a", r1, "a", "|"]
    assert walk(lex, aaa) == ["aaa"]
    aaaa = ["a", "<2>", "a", "|"] if replabel == 2 else ["a", r1, "a", r1, "|"]
    assert walk(lex, aaaa) == ["aaaa"]
    for w, sp in ((w, sp) for line in lines for w, *sp in [line.split()]):                 # every spelling is pack_replabels'
        packed = text.pack_replabels([d.get_index(t) for t in sp], d, replabel)
        assert all(a != b for a, b in zip(packed, packed[1:])) and w in walk(lex, [d.get_entry(t) for t in packed])
    run = subprocess.run([exe, str(tmp_path / "tokens.txt"), str(tmp_path / "lex.txt"), "|", str(replabel)], capture_output=True, timeout=60)
    assert run.returncode == 0, run.stderr
    out = run.stdout.decode("utf-8").splitlines()
    assert out[0].split() == ["info"] + [str(int(v)) for v in (lex.num_tokens, lex.num_words, lex.num_nodes, lex.sil, lex.smeared, lex.dropped)]
    assert out[1:1 + lex.num_words] == [f"word {i} {w}" for i, w in enumerate(lex.words)]
    for v, line in enumerate(out[1 + lex.num_words:]):
        _, words, has_children = lex.node(v)
        kids = " ".join(f"{t}:{lex.child(v, t)}" for t in range(lex.num_tokens) if lex.child(v, t) >= 0)
        head, tail = line.split(" |")
        f = head.split()
        assert f[:2] == ["node", str(v)] and f[2] == str(int(has_children)) and " ".join(f[3:]) == kids
        assert tail.split() == [str(w) for w in words]
    assert len(out) == 1 + lex.num_words + lex.num_nodes
    with pytest.raises(ValueError, match=f"replabel={replabel + 1} needs the token `<{replabel + 1}>`"):
        Lexicon.from_file(tmp_path / "lex.txt", d, smearing="none", sil="|", replabel=replabel + 1)
    run = subprocess.run([exe, str(tmp_path / "tokens.txt"), str(tmp_path / "lex.txt"), "|", str(replabel + 1)], capture_output=True,
                         text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("refused ") and f"needs the token `<{replabel + 1}>`" in run.stdout
