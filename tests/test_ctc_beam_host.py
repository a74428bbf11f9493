"""CTC prefix beam search without a GPU: the numpy restatement of w2l_ctc_beam_search's contract (tests/ctc_beam_ref.py) against
the enumeration of all N^T paths, the argument refusals of the C ABI (they return before anything touches the device), and the host
logic that turns a decoded label row into letters and words (wav2letter_amd/text.py, include/fl_compat/text.h)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import ctc_beam_ref as R
from wav2letter_amd import _lib, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


@pytest.mark.parametrize("N,T", [(3, 5), (4, 3)])
@pytest.mark.parametrize("normalize", [True, False])
def test_restatement_equals_enumeration(N, T, normalize):
    """W = 64, K = N-1, no threshold: the beam never binds.  logAdd = 1: every labelling's score is the log-sum over its paths and
    the ranking is the exact one wherever consecutive exact scores differ by more than 1e-9; logAdd = 0: the max over its paths"""
    for seed in range(3):
        x = np.random.default_rng(seed).normal(0, 2, size=(T, N)).astype(np.float32)
        for log_add in (True, False):
            exact = R.enumerate_labellings(x, log_add, normalize)
            hyps, diag = R.beam_search_one(x, T, 64, N - 1, INF, log_add, normalize, np.float64)
            assert len(hyps) == len(exact) <= 64 and len({p for p, _ in hyps}) == len(hyps)
            assert max(abs(s - exact[p]) for p, s in hyps) <= (1e-13 if log_add else 0.0) * max(1.0, diag.S)
            assert all(a[1] >= b[1] for a, b in zip(hyps, hyps[1:]))
            order = sorted(exact.items(), key=lambda kv: -kv[1])
            for m, (p, _) in enumerate(hyps):
                near = [q for q, s in order if abs(s - order[m][1]) <= 1e-9]
                assert p == order[m][0] or p in near
            assert diag.beam_gap == INF and diag.token_gap == INF and diag.threshold_gap == INF   # nothing was ever cut


def test_restatement_rules_on_a_worked_example():
    """two frames, N = 3 (labels 0, 1, blank 2), exact arithmetic: merge, tie order, threshold, K, W, frames, Lmax"""
    x = np.array([[0.0, -1.0, -1.0], [-1.0, 0.0, -1.0]], np.float32)
    hyps, _ = R.beam_search_one(x, 2, 64, 2, INF, False, False, np.float32)
    # after frame 0 the ranks are (0) = 0, () = -1 (stay before extension), (1) = -1.  Frame 1, tokens in the order 1, 0:
    #   rank 0 (0):  stay -1 | ext 1 -> (0,1) = 0 | ext 0: its own label adds pb = -inf: dropped
    #   rank 1 ():   stay -2 | ext 1 spells rank 2: merged into stay (1) | ext 0 spells rank 0: merged into stay (0)
    #   rank 2 (1):  stay -1 | ext 1: dropped | ext 0 -> (1,0) = -2
    # order: total, then rank, then stay before extension
    assert hyps == [((0, 1), 0.0), ((0,), -1.0), ((1,), -1.0), ((), -2.0), ((1, 0), -2.0)]
    # threshold 0: only the best survives each frame; threshold 1 keeps the candidates ON the line
    assert [p for p, _ in R.beam_search_one(x, 2, 64, 2, 0.0, False, False, np.float32)[0]] == [(0, 1)]
    on_line, _ = R.beam_search_one(x, 2, 64, 2, 1.0, False, False, np.float32)
    assert {s for _, s in on_line} == {0.0, -1.0}
    # K = 1: only the best token of a frame extends; W = 1: greedy
    assert {p for p, _ in R.beam_search_one(x, 2, 64, 1, INF, False, False, np.float32)[0]} == {(0, 1), (0,), (1,), ()}
    assert R.beam_search_one(x, 2, 1, 2, INF, False, False, np.float32)[0] == [((0, 1), 0.0)]
    # the merge: with logAdd the repeated label gathers both of its alignments' mass
    xs = np.log(np.array([[0.5, 0.25, 0.25], [0.5, 0.25, 0.25]], np.float32))
    h = dict(R.beam_search_one(xs, 2, 64, 2, INF, True, False, np.float64)[0])
    assert abs(np.exp(h[(0,)]) - (0.5 * 0.5 + 0.5 * 0.25 + 0.25 * 0.5)) < 1e-7     # 00, 0_, _0
    assert abs(np.exp(h[()]) - 0.0625) < 1e-8 and abs(sum(np.exp(v) for v in h.values()) - 1.0) < 1e-6
    # the C ABI's layout: frames, Lmax shorter than a hypothesis, ranks that do not exist
    lab, ln, sc, _ = R.beam_search(np.stack([x, x]), [2, 1], 64, 2, INF, False, False, 8, 1, np.float32)
    assert ln[0, 0] == 2 and lab[0, 0].tolist() == [0] and sc[0, 0] == 0.0
    assert ln[1, :4].tolist() == [1, 0, 1, -1] and lab[1, :3, 0].tolist() == [0, -1, 1] and sc[1, 3] == -INF


def test_c_abi_exists_and_refuses_bad_arguments():
    """w2l_ctc_beam_search / w2l_ctc_beam_workspace_size: declared, exported, host arithmetic and argument checks before any GPU
    work (every pointer below is host memory: a call that got past its checks would fault)"""
    assert {"w2l_ctc_beam_search", "w2l_ctc_beam_workspace_size"} <= set(_lib.exported_symbols())
    lib = _lib.lib()
    size = lib.w2l_ctc_beam_workspace_size
    assert size(0, 10, 10, 4, 4) == 0 and size(2, 0, 10, 4, 4) == 0 and size(2, 10, 1, 4, 4) == 0 and size(2, 10, 10, 0, 4) == 0
    assert size(2, 10, 10, 65, 4) == 0 and size(2, 10, 100, 4, 65) == 0
    assert 0 < size(2, 10, 30, 4, 4) < size(2, 20, 30, 4, 4) < size(2, 2000, 30, 4, 4)
    assert size(2, 10, 30, 4, 4) < size(4, 10, 30, 4, 4)
    assert size(2, 100, 30, 4, 4) < size(2, 100, 30, 64, 4) and size(2, 100, 100, 4, 4) < size(2, 100, 100, 4, 64)
    assert size(2, 100, 30, 4, 29) == size(2, 100, 30, 4, 64) == size(2, 100, 30, 4, 250000)      # K is clipped to N-1
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf)

    def call(B=2, T=4, N=5, x=p, frames=None, W=4, K=3, thr=1.0, log_add=0, norm=0, M=2, Lmax=4, lab=p, ln=p, sc=p, ws=p):
        return lib.w2l_ctc_beam_search(B, T, N, x, frames, W, K, thr, log_add, norm, M, Lmax, lab, ln, sc, ws, None)

    for bad in (dict(B=0), dict(T=0), dict(N=1), dict(B=-1), dict(x=None), dict(lab=None), dict(ln=None), dict(sc=None), dict(ws=None),
                dict(W=0), dict(K=0), dict(M=0), dict(M=5), dict(Lmax=0), dict(thr=-0.5), dict(thr=float("nan")), dict(thr=-INF)):
        assert call(**bad) == _lib.W2L_EINVAL, bad
    for big in (dict(W=65, M=2), dict(N=100, K=65), dict(N=100, K=250000)):
        assert call(**big) == _lib.W2L_EUNSUPPORTED, big
    assert call(W=65, x=None) == _lib.W2L_EINVAL                # null pointers are refused first, as the neighbouring CTC calls
    assert call(W=65, thr=-1.0) == _lib.W2L_EINVAL


# ---- from a decoded label row to letters and words ------------------------------------------------------------------------

LETTERS = ["|", "'"] + [chr(c) for c in range(ord("a"), ord("z") + 1)]


def test_decoded_labels_keep_doubled_letters():
    d = text.create_token_dict(LETTERS, "ctc")
    i = d.get_index
    row = [i(c) for c in "hello|bee|"] + [-1, -1]
    assert text.tkn_labels_to_ltr(row, d, "ctc", wordsep="|") == list("hello|bee")
    assert text.tkn_labels_to_wrd(row, d, "ctc", wordsep="|") == ["hello", "bee"]
    # the per-frame helper would collapse the doubled letters
    assert text.tkn2wrd(text.tkn_prediction_to_ltr(row, d, "ctc", wordsep="|"), "|") == ["helo", "be"]
    lead = [i(c) for c in "|a||aa"]
    assert text.tkn_labels_to_wrd(lead, d, "ctc", wordsep="|") == ["a", "aa"]
    assert text.tkn_labels_to_ltr(lead, d, "ctc", surround="|", wordsep="|") == ["a", "|", "|", "a", "a"]
    assert text.tkn_labels_to_ltr([], d, "ctc", wordsep="|") == [] and text.tkn_labels_to_wrd([-1, -1], d, "ctc", wordsep="|") == []
    assert text.tkn_labels_to_wrd(np.array(row, np.int32), d, "ctc", wordsep="|") == ["hello", "bee"]


def test_decoded_word_pieces():
    d = text.create_token_dict(["_the", "_c", "at", "_cat", "s", "_", "t", "h", "e", "c", "a"], "ctc")
    i = d.get_index
    row = [i("_the"), i("_cat"), i("s"), i("_"), i("e"), i("a"), i("t"), i("t"), -1]
    assert text.tkn_labels_to_ltr(row, d, "ctc", use_wordpiece=True, wordsep="_") == list("the_cats_eatt")
    assert text.tkn_labels_to_wrd(row, d, "ctc", use_wordpiece=True, wordsep="_") == ["the", "cats", "eatt"]


def test_cpp_header_twins_compile_and_agree(tmp_path):
    """include/fl_compat/text.h: tknLabels2Ltr / tknLabels2Wrd through tests/cpp/decode_text_test.cpp -- plain g++, no device
    code; the worked examples of this file asserted in C++"""
    exe = str(tmp_path / "decode_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "decode_text_test.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True)
    assert "decode text ok" in out.stdout
