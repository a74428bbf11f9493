"""The lexicon table (w2l_lexicon_*) against a textbook dict-of-dicts trie, the restatement of the lexicon-constrained beam search
(tests/ctc_beam_lex_ref.py) against the enumeration of every path and every (segmentation, homophone choice), and
w2l_ctc_beam_search_lex's refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR

INF = float("inf")
F32 = np.float32


def _pkg():
    from wav2letter_amd import Lexicon, NGramLM, _lib
    return Lexicon, NGramLM, _lib


def _table(trie):
    return _pkg()[0].from_spellings(trie.rows, trie.num_tokens, trie.num_words, trie.word_smear, trie.sil)


# ---- 1. the table against the textbook trie -------------------------------------------------------------------------------

TRIES = {  # name: (tokens, words, longest spelling, homophone fraction, sil, smeared, words crowded on one spelling)
    "letters": (29, 400, 6, 0.05, 28, True, 0),
    "pieces_no_smear": (500, 300, 3, 0.0, None, False, 0),
    "two_tokens_dense": (2, 40, 5, 0.3, 1, True, 0),
    "crowded_node": (10, 60, 3, 0.1, None, True, 9),
    "one_word": (3, 1, 1, 0.0, None, True, 0),
}


@pytest.mark.parametrize("name", list(TRIES))
def test_table_equals_the_textbook_trie_node_for_node(name):
    V, nwords, max_len, homo, sil, smeared, crowd = TRIES[name]
    rng = np.random.default_rng(len(name) * 13 + V)
    rows = XR.random_lexicon(rng, V, nwords, max_len, homo, sil, crowd=crowd)
    smear = rng.normal(-5, 2, nwords).astype(F32) if smeared else None
    trie = XR.TextbookTrie(rows, V, nwords, smear, sil)
    lex = _table(trie)
    nodes = trie.nodes()
    assert (lex.num_tokens, lex.num_words, lex.num_nodes, lex.sil, lex.smeared) == (V, nwords, len(nodes), -1 if sil is None else sil, smeared)
    assert lex.dropped == trie.dropped and (crowd < 6 or trie.dropped == crowd + 1 - 6)
    seen = set()
    for path, u in nodes:
        node = 0
        for t in path:
            node = lex.child(node, t)
            assert node > 0
        seen.add(node)
        sm, words, has_children = lex.node(node)
        assert words == u.words and has_children == bool(u.children)
        assert sm.view(np.int32) == u.smear.view(np.int32), (name, path)
        for t in range(V):                                       # and no edge the textbook trie lacks
            assert (lex.child(node, t) >= 0) == (t in u.children)
    assert seen == set(range(len(nodes)))                        # every node of the table is one of the textbook's
    if homo or crowd:
        assert any(len(u.words) >= 2 for _, u in nodes)
    print("trie", name, "nodes", len(nodes), "dropped", trie.dropped, "largest node", max(len(u.all_words) for _, u in nodes))


def test_smear_is_the_max_over_the_kept_words_only():
    """seven words on one spelling: the seventh is dropped and its (largest) smear value must not reach the node or its ancestors"""
    rows = [(w, [0, 1]) for w in range(7)] + [(7, [0])]
    smear = np.array([-3, -2, -4, -5, -6, -7, -0.5, -9], F32)
    lex = _pkg()[0].from_spellings(rows, 2, 8, smear)
    assert lex.dropped == 1
    n0 = lex.child(0, 0)
    n01 = lex.child(n0, 1)
    assert lex.node(n01) == (F32(-2), [0, 1, 2, 3, 4, 5], False)
    assert lex.node(n0) == (F32(-2), [7], True)
    assert lex.node(0)[0] == F32(-2)


def test_build_refusals_and_the_two_call_protocol():
    Lexicon, _, L = _pkg()

    def refused(rows, match, V=3, nw=3, smear=None, sil=None):
        with pytest.raises(ValueError, match=match):
            Lexicon.from_spellings(rows, V, nw, smear, sil)

    good = [(0, [0, 1]), (1, [1]), (2, [0, 1])]
    assert Lexicon.from_spellings(good, 3, 3).num_nodes == 4
    refused([(0, [])], "empty spelling")
    refused([(0, [0, 3])], "token 3 is outside 0 .. numTokens-1 .blank cannot be spelled.")
    refused([(0, [-1])], "token -1 is outside")
    refused([(3, [0])], "word id 3 is outside 0 .. numWords-1")
    refused([(-1, [0])], "word id -1 is outside")
    refused(good + [(0, [0, 1])], "row 3: duplicate .word, spelling. row, word 0")
    refused([(0, [2, 1])], "begins with the silence token", sil=2)
    assert Lexicon.from_spellings([(0, [1, 2])], 3, 3, None, 2).num_nodes == 3       # silence inside a spelling is a token like any
    refused(good, "smear value of word 1 is not finite", smear=np.array([0, np.inf, 0], F32))
    refused(good, "smear value of word 2 is not finite", smear=np.array([0, 0, np.nan], F32))
    refused(good, "silToken", sil=3)
    # the C ABI's two calls: the size, too little room, then exactly the size
    lib = L.lib()
    sw, off, toks = np.array([0, 1], np.int32), np.array([0, 2, 3], np.uintp), np.array([0, 1, 1], np.int32)
    size, dropped = C.c_size_t(0), C.c_size_t(99)

    def build(blob, n):
        return lib.w2l_lexicon_build(3, 2, 2, sw.ctypes.data, off.ctypes.data, toks.ctypes.data, None, -1, blob, C.addressof(n), C.addressof(dropped))
    assert build(None, size) == L.W2L_OK and size.value > 64 and dropped.value == 0
    need = size.value
    from wav2letter_amd.lm import _aligned
    room = _aligned(need)
    small = C.c_size_t(need - 16)
    assert build(room.ctypes.data, small) == L.W2L_EINVAL and f"needs {need} bytes".encode() in lib.w2l_host_last_error()
    assert not room.any()                                                           # a refused call writes nothing
    big = C.c_size_t(need)
    assert build(room.ctypes.data, big) == L.W2L_OK and big.value == need
    assert np.array_equal(room, Lexicon.from_spellings([(0, [0, 1]), (1, [1])], 3, 2).blob)
    assert lib.w2l_lexicon_build(3, 2, 2, sw.ctypes.data, off.ctypes.data, toks.ctypes.data, None, -1, None, None, None) == L.W2L_EINVAL
    with pytest.raises(ValueError, match="not a table"):
        Lexicon(np.zeros(256, np.uint8))
    lex = Lexicon(room)
    for node, tok in ((-1, 0), (lex.num_nodes, 0), (0, -1), (0, 3)):
        with pytest.raises(ValueError, match="out of range"):
            lex.child(node, tok)
    with pytest.raises(ValueError, match="out of range"):
        lex.node(lex.num_nodes)


def test_from_file_word_order_smear_and_refusals(tmp_path):
    Lexicon, NGramLM, _ = _pkg()
    tokens = ["|", "a", "b", "c"]
    (tmp_path / "lex.txt").write_text("cab c a b |\nab a b |\nb b |\nabc a b |\ncab c a |\n\xe9b a |\nZ a b |\n")
    lex = Lexicon.from_file(tmp_path / "lex.txt", tokens, smearing="none", sil="|")
    assert lex.words == ["Z", "ab", "abc", "b", "cab", "\xe9b"]                      # bytewise: upper case first, UTF-8 last
    assert (lex.num_tokens, lex.num_words, lex.sil, lex.smeared) == (4, 6, 0, False)
    node = 0
    for t in (1, 2, 0):
        node = lex.child(node, t)
    assert lex.node(node)[1] == [1, 2, 0]                                           # homophones in FILE order: ab, abc, Z
    tb = LR.random_lm(np.random.default_rng(1), 6, 2, 10)
    lm = NGramLM.from_ngrams(tb.arrays(), 6, float(tb.unk))
    sm = Lexicon.from_file(tmp_path / "lex.txt", tokens, lm=lm, sil="|")
    want = max(lm.score(lm.start, w)[0] for w in (1, 2, 0))
    assert sm.smeared and sm.node(node)[0] == want
    assert sm.node(0)[0] == max(lm.score(lm.start, w)[0] for w in range(6))
    (tmp_path / "bad.txt").write_text("ab a b\nax a x\n")
    with pytest.raises(ValueError, match="`ax` has the token `x`"):
        Lexicon.from_file(tmp_path / "bad.txt", tokens)
    with pytest.raises(ValueError, match="smearing 'logadd' is not built"):
        Lexicon.from_file(tmp_path / "lex.txt", tokens, smearing="logadd")
    with pytest.raises(ValueError, match="the LM has 6 words, the lexicon 2"):
        (tmp_path / "two.txt").write_text("ab a b\nb b\n")
        Lexicon.from_file(tmp_path / "two.txt", tokens, lm=lm)


# ---- 2. the search restatement against the enumeration of every path -------------------------------------------------------

def _tiny(N):
    """a lexicon with a homophone pair, a word that is a prefix of another, a spelling with a doubled token, a two-token word and
    the silence token (the last token class), over N-1 tokens"""
    sil = N - 2
    if N == 3:      # tokens: 0, sil = 1
        rows = [(0, [0, 0]), (1, [0, 0]), (2, [0])]       # 57 hypotheses fit 5 frames: W = 64 does not bind
    else:           # tokens: 0, 1, sil = 2
        rows = [(0, [0]), (1, [0]), (2, [0, 1]), (3, [1, 1]), (4, [1, 2, 0])]
    return rows, sil, 1 + max(w for w, _ in rows)


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("N,T", [(3, 5), (4, 3)])
def test_restatement_scores_every_hypothesis_as_the_enumeration_does(N, T, log_add):
    rows, sil, nwords = _tiny(N)
    rng = np.random.default_rng(N * 10 + T)
    tb = LR.random_lm(rng, nwords, 3, 12)
    lmw, word_score, eos_score = 0.7, -0.3, -0.4
    smear = np.array([tb.score(tb.history(()), w, F32) for w in range(nwords)], F32)
    trie = XR.TextbookTrie(rows, N - 1, nwords, smear, sil)
    shapes = {len(sp) for _, sp in rows}
    assert 2 in shapes and any(sp[0] == sp[1] for _, sp in rows if len(sp) > 1)                 # two tokens; a doubled token
    assert any(len(u.words) == 2 for _, u in trie.nodes()) and any(u.words and u.children for _, u in trie.nodes())
    worst, seen = 0.0, XR.LexDiag()
    for seed in range(3):
        x = np.random.default_rng(seed).normal(0, 2, size=(T, N)).astype(F32)
        hyps, dg = XR.beam_search_lex_one(x, T, 64, N - 1, trie, tb, lmw, word_score, eos_score, INF, log_add, log_add, np.float64,
                                          None, lm_dtype=np.float64)
        assert dg.beam_gap == np.inf                                                              # W = 64 never binds here
        want = XR.enumerate_hypotheses(x, trie, tb, lmw, word_score, eos_score, log_add, log_add)
        got = {h[4]: h[2] for h in hyps}
        assert set(got) == set(want) and len(hyps) == len(want)
        worst = max(worst, max(abs(got[h] - want[h]) for h in want))
        assert [h[4] for h in hyps] == sorted(want, key=lambda h: -want[h])
        assert any(sum(1 for g in got if tuple(c for c, _ in g) == tuple(c for c, _ in h)) > 1 for h in got)   # one spelling, two hypotheses
        for k in ("merges", "blocked", "homophones", "sil_loops", "end_dropped"):
            setattr(seen, k, getattr(seen, k) + getattr(dg, k))
    print("enumeration", (N, T), "logAdd", log_add, "hypotheses", len(want), "worst |score - enumeration|", worst,
          {k: getattr(seen, k) for k in ("merges", "blocked", "homophones", "sil_loops", "end_dropped")})
    assert worst <= 1e-9
    assert seen.merges > 0 and seen.blocked > 0 and seen.homophones > 0 and seen.sil_loops > 0 and seen.end_dropped > 0


def test_identity_lexicon_is_the_lm_search_restatement():
    """every token a one-token word with its own id, no silence, no smearing: the token-LM search with classScore = wordScore"""
    rng = np.random.default_rng(4)
    B, T, N, W, K, M = 3, 14, 12, 16, 5, 8
    x = (rng.integers(-24, 1, size=(B, T, N)) / 8).astype(F32)
    tb = LR.random_lm(rng, N - 1, 3, 40, eighths=True)
    trie = XR.TextbookTrie([(c, [c]) for c in range(N - 1)], N - 1, N - 1)
    lab, ln, sc, lms, wd, wc, _ = XR.beam_search_lex(x, [14, 5, 9], W, K, trie, tb, 0.5, 0.25, -0.5, 2.5, False, False, M, T, T, F32)
    rlab, rln, rsc, rlms, _ = LR.beam_search_lm(x, [14, 5, 9], W, K, tb, 0.5, np.full(N - 1, 0.25, F32), -0.5, 2.5, False, False, M, T, F32)
    assert np.array_equal(lab, rlab) and np.array_equal(ln, rln) and np.array_equal(sc, rsc) and np.array_equal(lms, rlms)
    assert np.array_equal(wd, lab) and np.array_equal(wc, ln)


# ---- 3. refusals of the C ABI, before anything touches the device -----------------------------------------------------------

def test_search_refusals_return_before_the_device():
    _, _, L = _pkg()
    lib = L.lib()
    buf = np.zeros(64, np.uint8).ctypes.data                                    # never read: every call below is refused first
    nan = float("nan")

    def call(B=2, T=10, N=30, x=buf, W=8, K=8, thr=INF, M=2, Lmax=10, lm=buf, has_eos=1, lmw=1.0, lex=buf, wsc=0.0, eos=0.0,
             labels=buf, lengths=buf, scores=buf, lms=buf, maxw=4, words=buf, counts=buf, ws=buf):
        return lib.w2l_ctc_beam_search_lex(B, T, N, x, None, W, K, thr, 0, 0, M, Lmax, lm, has_eos, lmw, lex, wsc, eos, labels, lengths,
                                           scores, lms, maxw, words, counts, ws, None)

    for kw in (dict(lex=None), dict(words=None), dict(counts=None), dict(maxw=0), dict(maxw=-1), dict(wsc=nan), dict(wsc=INF),
               dict(wsc=-INF), dict(lm=None), dict(lms=None), dict(x=None), dict(labels=None), dict(lengths=None), dict(scores=None),
               dict(ws=None), dict(lmw=INF), dict(lmw=nan), dict(eos=nan), dict(eos=-INF), dict(has_eos=0, eos=0.5), dict(thr=nan),
               dict(thr=-1.0), dict(M=9), dict(M=0), dict(W=0), dict(K=0), dict(Lmax=0), dict(N=1), dict(B=0), dict(T=0)):
        assert call(**kw) == L.W2L_EINVAL, kw
    for kw in (dict(W=65, M=2), dict(K=65, N=100)):
        assert call(**kw) == L.W2L_EUNSUPPORTED, kw
    size = lib.w2l_ctc_beam_lex_workspace_size
    assert size(2, 10, 30, 65, 8) == 0 and size(2, 10, 100, 8, 65) == 0 and size(0, 10, 30, 8, 8) == 0
    assert size(2, 10, 30, 8, 65) == size(2, 10, 30, 8, 29)                      # K clipped
    assert size(32, 188, 9998, 64, 64) >= lib.w2l_ctc_beam_lm_workspace_size(32, 188, 9998, 64, 64) + 32 * 64 * 4


def test_python_front_end_refuses_bad_lexicon_options_before_the_device():
    """the option checks come before the device checks: CPU tensors reach them"""
    import torch
    from wav2letter_amd import criterion
    Lexicon, NGramLM, L = _pkg()
    x = torch.zeros(1, 4, 6)
    rng = np.random.default_rng(0)
    lex = Lexicon.from_spellings([(0, [0, 1]), (1, [2]), (2, [4])], 5, 3)

    def lm(nw, eos=True):
        tb = LR.random_lm(rng, nw, 2, 5, eos=eos)
        return NGramLM.from_ngrams(tb.arrays(), nw, float(tb.unk))

    with pytest.raises(ValueError, match="lexicon needs lm"):
        criterion.ctc_beam_search(x, lexicon=lex)
    with pytest.raises(ValueError, match="class_score must be None with a lexicon"):
        criterion.ctc_beam_search(x, lexicon=lex, lm=lm(3), class_score=torch.zeros(5))
    with pytest.raises(ValueError, match="the LM has 5 words, the lexicon 3"):
        criterion.ctc_beam_search(x, lexicon=lex, lm=lm(5))
    with pytest.raises(ValueError, match="the lexicon has 4 tokens, the emissions 5"):
        criterion.ctc_beam_search(x, lexicon=Lexicon.from_spellings([(0, [0])], 4, 3), lm=lm(3))
    with pytest.raises(ValueError, match="eos_score needs a model with EOS"):
        criterion.ctc_beam_search(x, lexicon=lex, lm=lm(3, eos=False), eos_score=1.0)
    with pytest.raises(ValueError, match="max_words must be at least 1"):
        criterion.ctc_beam_search(x, lexicon=lex, lm=lm(3), max_words=0)
    for kw in (dict(word_score=0.5), dict(max_words=3)):
        with pytest.raises(ValueError, match="need lexicon"):
            criterion.ctc_beam_search(x, **kw)
    with pytest.raises(L.W2LError, match="GPU only"):                 # a well-formed call on CPU tensors: no CPU fallback
        criterion.ctc_beam_search(x, lexicon=lex, lm=lm(3), lm_weight=0.5, word_score=1.0)


def test_cpp_lexicon_header_equals_the_python_front_end_on_the_same_file(tmp_path):
    """include/fl_compat/lexicon.h (Lexicon::fromFile, child, node, the library's messages as exceptions) through
    tests/cpp/lexicon_text_test.cpp compiled here with g++: word order, node numbers, children, words in row order and smear bits
    equal wav2letter_amd.lexicon's on the same lexicon file and word ARPA"""
    import os
    import subprocess
    from tests.test_ctc_beam_lm_host import _arpa_text
    Lexicon, NGramLM, _ = _pkg()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = str(tmp_path / "lexicon_text_test"), os.path.join(root, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "lexicon_text_test.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    tokens = ["|", "a", "b", "c", "_d"]
    rng = np.random.default_rng(9)
    names = ["Zed", "ab", "abc", "b", "cab", "\xe9b", "a", "B", "_d", "ba"] + [f"w{i}" for i in range(8)]
    lines = []
    for w in names:
        for _ in range(int(rng.integers(1, 3))):
            lines.append(w + " " + " ".join(tokens[int(t)] for t in rng.integers(1, 5, int(rng.integers(1, 4)))) + " |")
    lines += [f"w{i} a b |" for i in range(8)]                                       # eight words on one spelling: two are dropped
    lines = list(dict.fromkeys(lines))
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n")
    (tmp_path / "lex.txt").write_text("\n".join(lines) + "\n", encoding="utf-8")
    plain = Lexicon.from_file(tmp_path / "lex.txt", tokens, smearing="none", sil="|")
    tb = LR.random_lm(np.random.default_rng(2), plain.num_words, 2, 30)
    (tmp_path / "lm.arpa").write_text(_arpa_text(tb, plain.words, unk10=-3.0)[0], encoding="utf-8")
    lm = NGramLM.from_arpa(tmp_path / "lm.arpa", plain.words)
    for lex, extra in ((plain, []), (Lexicon.from_file(tmp_path / "lex.txt", tokens, lm=lm, sil="|"), [str(tmp_path / "lm.arpa")])):
        run = subprocess.run([exe, str(tmp_path / "tokens.txt"), str(tmp_path / "lex.txt"), "|"] + extra, capture_output=True, timeout=60)
        assert run.returncode == 0, run.stderr
        out = run.stdout.decode("utf-8").splitlines()
        assert out[0].split() == ["info"] + [str(int(v)) for v in (lex.num_tokens, lex.num_words, lex.num_nodes, lex.sil, lex.smeared, lex.dropped)]
        assert lex.dropped >= 2
        assert out[1:1 + lex.num_words] == [f"word {i} {w}" for i, w in enumerate(lex.words)]
        for v, line in enumerate(out[1 + lex.num_words:]):
            sm, words, has_children = lex.node(v)
            kids = " ".join(f"{t}:{lex.child(v, t)}" for t in range(lex.num_tokens) if lex.child(v, t) >= 0)
            head, tail = line.split(" |")
            f = head.split()
            assert f[:2] == ["node", str(v)] and F32(float.fromhex(f[2])).view(np.int32) == sm.view(np.int32) and f[3] == str(int(has_children))
            assert " ".join(f[4:]) == kids and tail.split() == [str(w) for w in words]
        assert len(out) == 1 + lex.num_words + lex.num_nodes
    (tmp_path / "bad.txt").write_text("ab a b\nax a x\n")
    run = subprocess.run([exe, str(tmp_path / "tokens.txt"), str(tmp_path / "bad.txt"), "-"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("refused ") and "`ax` has the token `x`" in run.stdout
