"""The xl beam searches (w2l_*_beam_search*_xl, W up to 8192) on the GPU, with the machinery of tests/test_gpu_beam_wide.py.
X1 identity with the wide kernels at widths both accept, byte for byte, both (+) modes; X2 logAdd = 0 bit for bit against the
float32 restatements (tests/*_beam_ref.py, generic in W) above the wide limit -- 1025, 2500 (the reference's default), 2500 with
a threshold line, 8192 with K = 32 -- on inputs whose sums are exact and whose ties are dense, with the proof on the CPU that the
beam holds more than 1024 entries, binds and merges; X3 logAdd = 1 against the float64 restatements where the decisions have a
margin; X4 the output rules at M = W = 8192; X5 the complete labelling list of an enumeration the wide family cannot hold; X6 the
surfaces: Python, the compiled C++ caller, Decode --w2l_beam_xl."""
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
from tests.test_gpu_beam_wide import (F32, INF, KEYS, KINDS, ROOT, W3_M, Case, _delta, _dense_case, _quarters, _same_bits, _smear,
                                      _w1_case, _w5_inputs)

pytestmark = pytest.mark.gpu
XL = "xl"


def _rows(want):
    return {k: v for k, v in want.items() if k != "diags"}


# ---- X1: identity with the wide kernels --------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("K", [8, 29])
@pytest.mark.parametrize("W", [1, 64, 65, 1000, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_x1_xl_equals_the_wide_twin_byte_for_byte(kind, W, K, log_add):
    """every output tensor, both (+) modes, with a threshold that cuts from W = 64 up and label and word rows shorter than the
    hypotheses; 1000 and 1024 entries are the strided ownership at n < 1024 and n = 1024"""
    c = _w1_case(kind)
    M, Lmax, thr = W, 5, (INF if W < 64 else 4.0)
    wide = c.gpu(W, K, M, Lmax, True, thr, log_add, log_add and not c.asg, 2)
    xl = c.gpu(W, K, M, Lmax, XL, thr, log_add, log_add and not c.asg, 2)
    assert (wide["lengths"] >= 0).any() and wide["lengths"].max() > Lmax
    _same_bits(xl, wide)


# ---- X2: bit for bit against the float32 restatement, logAdd = 0 -------------------------------------------------------------

X2_SHAPES = {  # name: (W, K, N, T, B, frames, hot, nwords, max_len); T of w8192_k32: _x2_shape
    "w1025": (1025, 16, 30, 6, 2, [6, 4], 16, 600, 2),
    "w2500": (2500, 16, 30, 6, 2, [6, 4], 16, 600, 2),
    "w2500_threshold": (2500, 16, 30, 6, 2, [6, 4], 16, 600, 2),
    "w8192_k32": (8192, 32, 40, None, 1, None, 32, 1500, 2),
}
X2_THRESHOLD = {"ctc": 2.0, "ctc_lm": 4.0, "ctc_lex": 3.0, "asg": 2.0, "asg_lm": 4.0, "asg_lex": 3.0}


def _x2_shape(name, kind):
    W, K, N, T, B, frames, hot, nwords, max_len = X2_SHAPES[name]
    if T is None:      # the restatement of a lexicon search at W = 8192 costs 38 s on the CPU at T = 5
        T = 3 if kind.endswith("lex") else 5
    return W, K, N, T, B, frames, hot, nwords, max_len, (X2_THRESHOLD[kind] if name.endswith("_threshold") else INF)


def _legal_lexicon(c):
    """_dense_case's lexicon as the library takes it.  The X2 shapes ask random_lexicon for more distinct spellings than their
    letters have (600 words on 16 letters of which one is the silence and at most two a word: 255 spellings; 1500 words on 32: 1023),
    so once they are used up it hands out whatever it drew last, and one draw in `hot` begins with the silence token -- a row the
    textbook trie takes and w2l_lexicon_build refuses by contract.  Those rows are dropped (their words stay in the LM, without a
    spelling); every other row, the LM, the smear values and the emissions are the seed's"""
    if c.trie is None:
        return c
    rows = [(w, sp) for w, sp in c.trie.rows if sp[0] != c.trie.sil]
    assert 0 < len(c.trie.rows) - len(rows) < len(rows) // 10
    trie = XR.TextbookTrie(rows, c.trie.num_tokens, c.trie.num_words, c.trie.word_smear, c.trie.sil)
    nodes = [u for _, u in trie.nodes()]
    assert any(len(u.words) >= 2 for u in nodes) and any(u.words and u.children for u in nodes)
    return Case(c.kind, c.x, c.frames, c.A, c.tb, trie, None, c.lmw, c.wsc, c.eos)


@functools.lru_cache(maxsize=None)
def _x2_reference(name, kind):
    """inputs, the float32 restatement's outputs (M = W rows) and the facts that make the case worth running, asserted here on the
    CPU: the beam holds more than 1024 entries, the beam binds (without a threshold line), every utterance of three frames and more
    merges, and in the threshold case the line changes labels or scores against the same search without it"""
    W, K, N, T, B, frames, hot, nwords, max_len, thr = _x2_shape(name, kind)
    c = _legal_lexicon(_dense_case(kind, 300 + KINDS.index(kind), B, T, N, frames, hot, nwords, max_len))
    want = c.ref(W, K, W, T, F32, thr, False, False, T)
    diags = want["diags"]
    held = int((want["lengths"] >= 0).sum(axis=1).max()) + (max(d.end_dropped for d in diags) if kind.endswith("lex") else 0)
    binds = any(d.cuts > 0 for d in diags) if c.asg else any(d.beam_gap < INF for d in diags)
    merges = c.merges(W, K, thr, diags)
    long_utts = [b for b in range(B) if (T if frames is None else frames[b]) >= 3]
    facts = dict(held=held, binds=binds, merges=merges)
    assert held > 1024 and all(merges[b] > 0 for b in long_utts), (name, kind, facts)
    # what prunes: without a line the width (the beam binds); with the line the line itself -- for ctc_lm and asg_lm it leaves
    # 1927 and 1971 entries, fewer than W, so there the width cannot bind and the line's effect is what is asserted
    assert binds or thr != INF, (name, kind, facts)
    if thr != INF:
        free = _x2_reference("w2500", kind)[1]                             # the same inputs without the line
        assert any((free[k].view(np.int32) != want[k].view(np.int32)).any() for k in ("labels", "scores")), (name, kind)
    return c, want, facts


@pytest.mark.parametrize("name,kind", [(n, k) for n in X2_SHAPES for k in KINDS])
def test_x2_bitwise_against_the_float32_restatement(name, kind):
    W, K, N, T, B, frames, hot, nwords, max_len, thr = _x2_shape(name, kind)
    c, want, facts = _x2_reference(name, kind)
    print("X2", name, kind, facts, "live rows", int((want["lengths"] >= 0).sum()))
    got = c.gpu(W, K, W, T, XL, thr, False, False, T)
    assert want["scores"].dtype == F32
    _same_bits(got, _rows(want))
    # a second run: the same bytes (ranks are a function of the keys, never of the order in which atomics arrived)
    _same_bits(c.gpu(W, K, W, T, XL, thr, False, False, T), got)


# ---- X3: logAdd = 1 against the float64 restatement --------------------------------------------------------------------------

X3_SHAPE = (2500, 8, 30, 12, 4)                                                               # (W, K, N, T, B)


@functools.lru_cache(maxsize=None)
def _x3_reference(kind):
    """tests/test_gpu_beam_wide.py's _w3_reference at W = 2500 with seeds of its own (seed 903 would leave two of four `asg`
    utterances without a compared rank; with these the restatement leaves none out)"""
    W, K, N, T, B = X3_SHAPE
    rng = np.random.default_rng(940 + KINDS.index(kind))
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
def test_x3_log_sum_search_against_the_float64_restatement(kind):
    """the method of test_w3_*: the scores within delta(T, S), the hypotheses compared where the restatement's own margins exceed
    twice that bound; at most one utterance in four may have no such rank"""
    W, K, N, T, B = X3_SHAPE
    c, want, lead = _x3_reference(kind)
    left_out = sum(1 for n, _ in lead if n == 0)
    print("X3", X3_SHAPE, kind, "compared ranks per utterance", [n for n, _ in lead], "delta", max(dl for _, dl in lead))
    assert 4 * left_out <= B and (want["lengths"] >= 0).any()
    got = c.gpu(W, K, W3_M, T, XL, INF, True, not c.asg, T)
    for b, (n, dl) in enumerate(lead):
        for k in ("labels", "lengths", "words", "word_counts"):
            if k in want:
                assert (got[k][b, :n] == want[k][b, :n]).all(), (b, k)
        assert (np.abs(got["scores"][b, :n].astype(np.float64) - want["scores"][b, :n]) <= dl).all(), b
        if "lm_scores" in want:
            assert (got["lm_scores"][b, :n].view(np.int32) == want["lm_scores"][b, :n].view(np.int32)).all()


# ---- X4: outputs -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_x4_m_equals_w_8192_with_short_label_rows(kind):
    """M = W = 8192, Lmax = 3 and two word rows: truncated rows, true lengths.  The four kinds without a lexicon run five frames and
    have hypotheses longer than three labels; the two with one run three frames, and it is their word rows that are cut"""
    W, K, N, T, B, frames, hot, nwords, max_len, thr = _x2_shape("w8192_k32", kind)
    c, want, _ = _x2_reference("w8192_k32", kind)
    got = c.gpu(W, K, W, 3, XL, thr, False, False, 2)
    assert want["word_counts"].max() > 2 if "words" in want else want["lengths"].max() > 3
    for k in ("lengths", "scores", "lm_scores", "word_counts"):
        if k in want:
            assert (got[k].view(np.int32) == want[k].view(np.int32)).all(), k
    assert (got["labels"] == want["labels"][:, :, :3]).all()
    if "words" in want:
        assert (got["words"] == want["words"][:, :, :2]).all()


@pytest.mark.parametrize("kind", ["ctc", "ctc_lm", "asg", "asg_lm"])
def test_x4_fewer_prefixes_than_w(kind):
    """N = 3, T = 4: a handful of prefixes; the rows beyond the survivors are -1 / -inf"""
    c = _dense_case(kind, 5, 2, 4, 3, None)
    want = c.ref(8192, 64, 8192, 4, F32)
    got = c.gpu(8192, 64, 8192, 4, XL)
    live = (want["lengths"] >= 0).sum(axis=1)
    assert (live > 4).all() and (live < 64).all()
    _same_bits(got, _rows(want))
    assert (got["lengths"][:, 64:] == -1).all() and np.isneginf(got["scores"][:, 64:]).all() and (got["labels"][:, 64:] == -1).all()


@pytest.mark.parametrize("kind", ["ctc_lex", "asg_lex"])
def test_x4_lexicon_without_an_entry_at_the_root(kind):
    """test_w4_lexicon_without_an_entry_at_the_root at W = 2000: every word has two tokens and the utterance one frame, every
    entry ends inside a word, all rows are empty"""
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
    want = c.ref(2000, 64, 2000, 4, F32, thr, max_words=4)
    assert sum(d.end_dropped for d in want["diags"]) > 0 and (want["lengths"] == -1).all()
    got = c.gpu(2000, 64, 2000, 4, XL, thr, max_words=4)
    _same_bits(got, _rows(want))
    assert (got["lengths"] == -1).all() and (got["word_counts"] == -1).all() and (got["labels"] == -1).all()
    assert (got["words"] == -1).all() and np.isneginf(got["scores"]).all() and np.isneginf(got["lm_scores"]).all()


# ---- X5: exhaustive ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,count", [("ctc", 2065), ("asg", 6825)])
def test_x5_the_complete_labelling_list_of_n5_t6(kind, count):
    """N = 5, T = 6 has 2065 CTC labellings and 6825 ASG ones, more than the wide family holds and fewer than 8192: with logAdd = 0
    and zero transitions the output at W = 8192 is the enumeration's complete list, every labelling with the maximum over its
    paths, in the enumeration's order.  These inputs (_w5_inputs(5, 6, 77), the wide file's) do have labellings that tie -- 2064
    and 6811 distinct scores, found when this test first ran -- so "the enumeration's order" is the order of the scores, which
    must be the enumeration's list value for value, with every labelling at a position that holds its own score; inside a group of
    equal scores the order is the search's tie key, and that is held to the float32 restatement bit for bit"""
    N, T = 5, 6
    x = _w5_inputs(N, T, 77)
    A = np.zeros((N, N), F32)
    c = Case(kind, x, None, A if kind == "asg" else None)
    want = AR.enumerate_labellings(x[0], A, False, False) if kind == "asg" else R.enumerate_labellings(x[0], False, False)
    order = sorted(want, key=lambda h: -want[h])
    ties = count - len({want[h] for h in order})
    print("X5", kind, "labellings", len(order), "of which", ties, "share a score with another")
    assert len(order) == count and 10 * ties < count
    got = c.gpu(8192, 64, 8192, T, XL)
    ln = got["lengths"][0]
    assert (ln[:count] >= 0).all() and (ln[count:] == -1).all()
    hyps = [tuple(got["labels"][0, m, :ln[m]]) for m in range(count)]
    scores = got["scores"][0, :count].astype(np.float64)
    assert (scores == np.array([want[h] for h in order])).all()                    # the enumeration's list of scores, in its order
    assert len(set(hyps)) == count and set(hyps) == set(order)                     # every labelling, once
    assert all(want[h] == s for h, s in zip(hyps, scores))                         # each where its own score stands
    assert np.isneginf(got["scores"][0, count:]).all()
    _same_bits(got, _rows(c.ref(8192, 64, 8192, T, F32)))                          # the order inside the ties: the contract's tie key


# ---- X6: surfaces ------------------------------------------------------------------------------------------------------------

def test_x6_python_methods_take_xl():
    from wav2letter_amd import ASGLoss, CTCLoss, _lib, criterion
    c = _w1_case("ctc_lm")
    xd, fd = torch.tensor(c.x, device="cuda"), torch.tensor(c.frames, dtype=torch.int32, device="cuda")
    want = c.gpu(2500, 8, 3, 24, XL)
    got = CTCLoss().beamSearch(xd, fd, beam=2500, beam_token=8, nbest=3, lm=c._lm, lm_weight=c.lmw, eos_score=c.eos,
                               class_score=torch.tensor(c.cls, device="cuda"), wide=XL)
    assert all((g.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all() for g, k in zip(got, KEYS))
    a = _w1_case("asg")
    crit = ASGLoss(30).cuda()
    with torch.no_grad():
        crit.transitions.copy_(torch.tensor(a.A))
    xa, fa = torch.tensor(a.x, device="cuda"), torch.tensor(a.frames, dtype=torch.int32, device="cuda")
    want = a.gpu(2500, 8, 3, 24, XL)
    got = crit.beamSearch(xa, fa, beam=2500, beam_token=8, nbest=3, wide=XL)
    assert len(got) == 3 and all((g.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all() for g, k in zip(got, KEYS))
    # the xl path refuses beyond 8192; the other two keep their limits
    for wide, beam in ((False, 65), (True, 1025), (XL, 8193)):
        with pytest.raises(_lib.W2LError):
            criterion.ctc_beam_search(xd, beam=beam, wide=wide)
        with pytest.raises(_lib.W2LError):
            criterion.asg_beam_search(xa, torch.tensor(a.A, device="cuda"), beam=beam, wide=wide)
    assert criterion.ctc_beam_search(xd, beam=1025, wide=XL)[1].min() >= 0


def test_x6_cpp_options_xl_equal_the_c_abi(tmp_path):
    """tests/cpp/decode_xl_caller.cpp (plain g++ against libw2l_hip.so): BeamSearchOptions::xl at W = 2500 for CTC + lexicon and
    ASG + token LM, from the same lexicon and ARPA files; its output equals the Python front end's, which calls the C ABI"""
    from tests.test_ctc_beam_lm_host import _arpa_text
    from wav2letter_amd import Lexicon, NGramLM
    exe, libdir = str(tmp_path / "decode_xl_caller"), os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "decode_xl_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    rng = np.random.default_rng(22)
    B, T, W, K, M, Lmax, maxw = 3, 20, 2500, 8, 5, 20, 6
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
        want = c.gpu(W, K, M, Lmax, XL, 6.0, True, mode == "ctc_lex", maxw)
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([N, T, B, W, K, M, Lmax, maxw], np.int32).tobytes() + frames.tobytes() + x.tobytes() + A.tobytes())
        run = subprocess.run([exe, mode, inp, outp, str(tmp_path / "tokens.txt"), str(tmp_path / "lexicon.txt"), str(tmp_path / "lm.arpa")],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "decode xl caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
        raw = np.fromfile(outp, np.int32)
        pos = 0
        for k, shape in (("labels", (B, M, Lmax)), ("lengths", (B, M)), ("scores", (B, M)), ("lm_scores", (B, M)),
                         ("words", (B, M, maxw)), ("word_counts", (B, M))):
            if k in want:
                n = int(np.prod(shape))
                assert (raw[pos:pos + n].reshape(shape) == want[k].view(np.int32)).all(), (mode, k)
                pos += n
        assert pos == len(raw) and (want["lengths"] >= 0).any()


# ---- Decode --w2l_beam_xl ------------------------------------------------------------------------------------------------------

from tests.list_fixture import ENV  # noqa: E402
from tests.test_gpu_asg_beam import trained_asg  # noqa: E402,F401  (the module-scoped ASG checkpoint)
from tests.test_gpu_ctc_beam import DECODE_EXE, _sclite_lines, trained  # noqa: E402,F401  (the module-scoped CTC checkpoint)


def _decode(d, model, *flags):
    res = subprocess.run([DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}"] + list(flags),
                         capture_output=True, text=True, timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return res.stderr, (d / "out" / "other.hyp").read_text()


def _beam_part(err):
    """stderr without the --beamsizetoken line, which says "limited to 64 tokens per frame" whatever the beam is"""
    return "\n".join(line for line in err.splitlines() if "--beamsizetoken" not in line)


def test_x6_decode_w2l_beam_xl_ctc(trained):
    """without the flag nothing changes; with it a --beamsize above 1024 runs the xl kernels, beyond 8192 it is limited and said so;
    with --logadd=false and no LM the 1-best of every width is the greedy transcript, which a beam of one entry keeps"""
    d, model = trained
    err1, greedy = _decode(d, model, "--beamsize=1")
    assert "(xl)" not in err1 and "(wide)" not in err1 and len(_sclite_lines(d / "out" / "other.hyp")) == 5
    err, hyp = _decode(d, model, "--beamsize=5000")
    assert "--beamsize=5000 limited to 1024 (the kernel's beam width)" in err and "beam 1024 (wide)" in err and "(xl)" not in err
    assert hyp == greedy
    err, hyp = _decode(d, model, "--beamsize=5000", "--w2l_beam_xl=true")
    assert "beam 5000 (xl)" in err and "limited to" not in _beam_part(err) and "(wide)" not in err and hyp == greedy
    err, hyp = _decode(d, model, "--beamsize=9000", "--w2l_beam_xl=true")
    assert "--beamsize=9000 limited to 8192 (the kernel's beam width)" in err and "beam 8192 (xl)" in err and hyp == greedy
    # values up to 1024 and an absent --beamsize route as without the flag
    err, hyp = _decode(d, model, "--beamsize=200", "--w2l_beam_xl=true")
    assert "beam 200 (wide)" in err and "(xl)" not in err and hyp == greedy
    err, hyp = _decode(d, model, "--w2l_beam_xl=true")
    assert "limited to 64 (the kernel's beam width)" in err and "(xl)" not in err and "(wide)" not in err and hyp == greedy


def test_x6_decode_w2l_beam_xl_asg(trained_asg):
    d, model = trained_asg
    _, viterbi = _decode(d, model, "--beamsize=1")
    err, hyp = _decode(d, model, "--beamsize=2500", "--w2l_beam_xl=true")
    assert "beam 2500 (xl)" in err and "limited to" not in _beam_part(err) and hyp == viterbi
