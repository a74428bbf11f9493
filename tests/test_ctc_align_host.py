"""CTC forced alignment without a GPU: the numpy restatement of w2l_ctc_align's contract (tests/ctc_align_ref.py) against the
enumeration of all lattice paths, the argument refusals of the C ABI, and the host logic that turns a path into token spans, word
spans and the segment lines the Align tool writes (wav2letter_amd/text.py, include/fl_compat/text.h)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import ctc_align_ref as R
from wav2letter_amd import _lib, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def enumerate_best(x, y, F):
    """every path through the CTC lattice of y over F frames: (best score in float64, the paths reaching it) or (None, [])"""
    N = x.shape[1]
    blank, S = N - 1, 2 * len(y) + 1
    ext = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    best, arg = None, []

    def walk(t, s, score, states):
        nonlocal best, arg
        score += float(x[t, ext[s]])
        states = states + [s]
        if t == F - 1:
            if s >= S - 2:
                if best is None or score > best:
                    best, arg = score, [states]
                elif score == best:
                    arg.append(states)
            return
        for d in (0, 1, 2):
            n = s + d
            if n >= S or (d == 2 and not (n % 2 == 1 and ext[n] != ext[n - 2])):
                continue
            walk(t + 1, n, score, states)

    walk(0, 0, 0.0, [])
    if S > 1:
        walk(0, 1, 0.0, [])
    return best, [[ext[s] for s in st] for st in arg]


def test_restatement_equals_path_enumeration():
    """T <= 8, N <= 5, L <= 4, small-integer emissions (exact in fp32, exact ties everywhere): the restatement's best score equals
    the enumeration's, its path is one of the best paths and collapses to the target; infeasible -> -1 / -inf"""
    rng = np.random.default_rng(2019)
    feasible = infeasible = 0
    for _ in range(600):
        T, N, Lb = int(rng.integers(1, 9)), int(rng.integers(2, 6)), int(rng.integers(0, 5))
        x = rng.integers(-3, 4, size=(T, N)).astype(np.float32)
        y = rng.integers(0, N - 1, size=Lb)
        F = int(rng.integers(1, T + 1))
        path, end = R.align_one(x, y, F)
        best, paths = enumerate_best(x, y, F)
        Rr = int((y[1:] == y[:-1]).sum())
        if Lb + Rr > F:
            infeasible += 1
            assert best is None and (path == -1).all() and end == -np.inf
            continue
        feasible += 1
        assert best is not None and float(end) == best
        assert list(path[:F]) in paths and (path[F:] == N - 1).all()
        assert R.collapse(path[:F], N - 1) == [int(v) for v in y]
        assert sum(float(x[t, path[t]]) for t in range(F)) == best
    assert feasible > 312 and infeasible > 30


def test_restatement_frames_is_truncation_plus_blank_fill():
    rng = np.random.default_rng(7)
    B, T, N, L = 6, 12, 5, 4
    x = rng.integers(-2, 3, size=(B, T, N)).astype(np.float32)
    tgt = rng.integers(0, N - 1, size=(B, L)).astype(np.int32)
    tgt[1, 2:] = -1
    tgt[4, 0:] = -1                                            # empty target: all blank
    frames = np.array([12, 5, 9, 3, 7, 8], np.int32)           # row 3: 4 labels (+ repeats) in 3 frames: infeasible
    path, score = R.ctc_align_ref(x, tgt, frames)
    ts = R.ctc_target_size(tgt, T)
    for b in range(B):
        F = int(frames[b])
        p, _ = R.align_one(x[b, :F], tgt[b][:ts[b]], F)
        if (p == -1).all():
            assert (path[b] == -1).all() and score[b] == -np.inf
            continue
        assert (path[b, :F] == p).all() and (path[b, F:] == N - 1).all()
        assert score[b] == R.path_logprob(x[b], path[b], F)
    assert (path[3] == -1).all() and (path[4] == N - 1).all()


def test_c_abi_exists_and_refuses_bad_arguments():
    """w2l_ctc_align / w2l_ctc_align_workspace_size: declared, exported, host arithmetic and argument checks before any GPU work"""
    assert {"w2l_ctc_align", "w2l_ctc_align_workspace_size"} <= set(_lib.exported_symbols())
    lib = _lib.lib()
    size = lib.w2l_ctc_align_workspace_size
    assert size(0, 10, 10, 4) == 0 and size(2, 0, 10, 4) == 0
    assert 0 < size(2, 10, 30, 4) < size(2, 20, 30, 4) < size(2, 2000, 30, 4)
    assert size(2, 10, 30, 4) < size(4, 10, 30, 4)
    assert size(1, 100, 30, 1023) > size(1, 100, 30, 64)          # 32 positions per lane: 64-bit back-pointer words
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf)

    def call(B=2, T=4, N=5, L=3, x=p, y=p, ts=p, frames=None, path=p, score=None, ws=p):
        return lib.w2l_ctc_align(B, T, N, L, x, y, ts, frames, path, score, ws, None)

    for bad in (dict(B=0), dict(T=0), dict(N=1), dict(L=0), dict(B=-1), dict(x=None), dict(y=None), dict(ts=None),
                dict(path=None), dict(ws=None)):
        assert call(**bad) == _lib.W2L_EINVAL, bad
    assert call(L=1024) == _lib.W2L_EUNSUPPORTED
    assert call(L=1024, x=None) == _lib.W2L_EINVAL             # null pointers are refused first, as the neighbouring CTC calls


# ---- from a path to token spans, word spans and segment lines --------------------------------------------------------------

LETTERS = ["|", "'"] + [chr(c) for c in range(ord("a"), ord("z") + 1)]


def parse_segments(line):
    """the consumers' view of an Align line (the reference's filter_segmentations.py:31-39): sample id, tab, segments joined by
    the two characters backslash-n; of each segment the fields 3, 4 and 5 = begin, length, word; entry 0 is skipped"""
    assert line.endswith("\n") and "\n" not in line[:-1]
    sample, segs = line[:-1].split("\t")
    out = []
    for seg in segs.split("\\n"):
        fields = seg.split(" ")
        assert len(fields) == 5
        out.append((float(fields[2]), float(fields[3]), fields[4]))
    return sample, out[1:], out[0]


def test_ctc_letters_with_word_separator():
    d = text.create_token_dict(LETTERS, "ctc")
    lex = text.load_lexicon(["hi\th i |", "aa\ta a |"])
    words = ["hi", "aa"]
    tgt = text.target_indices(words, lex, d, "ctc", wordsep="|")
    assert [d.get_entry(i) for i in tgt] == list("hi|aa|")
    widx = text.target_word_index(words, lex, d, "ctc", wordsep="|")
    assert widx == [0, 0, -1, 1, 1, -1] and len(widx) == len(tgt)
    i, b = d.get_index, d.get_index(text.BLANK)
    #       0  1       2       3       4       5  6       7  8       9  10      11
    path = [b, i("h"), i("h"), i("i"), i("|"), b, i("a"), b, i("a"), b, i("|"), b]
    spans = text.alignment_token_spans(path, tgt, blank=b)
    assert spans == [(1, 2), (3, 3), (4, 4), (6, 6), (8, 8), (10, 10)]
    segs = text.word_segments(spans, widx, words, frames=12, seconds_per_frame=0.08)
    assert [(round(s, 6), round(n, 6), w) for s, n, w in segs] == [
        (0.0, 0.08, "$"), (0.08, 0.24, "hi"), (0.32, 0.16, "$"), (0.48, 0.24, "aa"), (0.72, 0.24, "$")]
    line = text.format_alignment_line("utt-1", segs)
    assert line == ("utt-1\tID A 0.00 0.08 $\\nID A 0.08 0.24 hi\\nID A 0.32 0.16 $\\nID A 0.48 0.24 aa\\nID A 0.72 0.24 $\n")
    sample, rest, first = parse_segments(line)
    assert sample == "utt-1" and first[2] == "$" and [w for _, _, w in rest if w != "$"] == words
    # a path that does not spell the target is refused
    with pytest.raises(ValueError):
        text.alignment_token_spans(path[:6] + [b] * 6, tgt, blank=b)
    with pytest.raises(ValueError):
        text.alignment_token_spans([-1] * 12, tgt, blank=b)     # an infeasible row of w2l_ctc_align


def test_speech_from_frame_zero_and_no_trailing_silence():
    """the list always starts with a `$` segment (length 0 when speech starts in frame 0: the consumers skip entry 0); other
    zero-length silences are left out"""
    d = text.create_token_dict(LETTERS, "ctc")
    lex = text.load_lexicon(["a\ta |", "b\tb |"])
    words = ["a", "b"]
    tgt = text.target_indices(words, lex, d, "ctc", wordsep="|")          # a | b |
    widx = text.target_word_index(words, lex, d, "ctc", wordsep="|")
    assert widx == [0, -1, 1, -1]
    i = d.get_index
    path = [i("a"), i("|"), i("b"), i("b"), i("|")]
    spans = text.alignment_token_spans(path, tgt, blank=d.get_index(text.BLANK))
    segs = text.word_segments(spans, widx, words, frames=5, seconds_per_frame=0.5)
    assert segs == [(0.0, 0.0, "$"), (0.0, 0.5, "a"), (0.5, 0.5, "$"), (1.0, 1.0, "b"), (2.0, 0.5, "$")]
    # words that touch: no zero-length silence between them; frames beyond the path's speech are trailing silence
    tgt2 = [i("a"), i("b")]
    spans2 = text.alignment_token_spans([i("a"), i("b"), d.get_index(text.BLANK)], tgt2, blank=d.get_index(text.BLANK))
    segs2 = text.word_segments(spans2, [0, 1], words, frames=3, seconds_per_frame=1.0)
    assert segs2 == [(0.0, 0.0, "$"), (0.0, 1.0, "a"), (1.0, 1.0, "b"), (2.0, 1.0, "$")]
    _, rest, first = parse_segments(text.format_alignment_line("s", segs2))
    assert first == (0.0, 0.0, "$") and rest == [(0.0, 1.0, "a"), (1.0, 1.0, "b"), (2.0, 1.0, "$")]


def test_asg_with_replabels_and_surround():
    d = text.create_token_dict(LETTERS, "asg", replabel=2)
    lex = text.load_lexicon(["hello\th e l l o |", "aaa\ta a a |"])
    words = ["hello", "aaa"]
    tgt = text.target_indices(words, lex, d, "asg", replabel=2, wordsep="|", surround="|")
    names = [d.get_entry(i) for i in tgt]
    # (the last word's separator and the surround token are one run: the second becomes a replabel, which belongs to no word)
    assert names == ["|", "h", "e", "l", "<1>", "o", "|", "a", "<2>", "|", "<1>"]
    widx = text.target_word_index(words, lex, d, "asg", replabel=2, wordsep="|", surround="|")
    assert widx == [-1, 0, 0, 0, 0, 0, -1, 1, 1, -1, -1] and len(widx) == len(tgt)
    # an ASG path has no blank: every frame belongs to a token (w2l_fac_viterbi's output)
    reps = [2, 1, 1, 2, 1, 1, 3, 1, 2, 1, 1]
    path = [t for t, n in zip(tgt, reps) for _ in range(n)]
    spans = text.alignment_token_spans(path, tgt)
    assert spans[0] == (0, 1) and spans[-1] == (15, 15) and all(a <= b2 for a, b2 in spans)
    assert all(spans[k + 1][0] == spans[k][1] + 1 for k in range(len(spans) - 1))
    segs = text.word_segments(spans, widx, words, frames=16, seconds_per_frame=0.1)
    assert [(round(s, 6), round(n, 6), w) for s, n, w in segs] == [
        (0.0, 0.2, "$"), (0.2, 0.6, "hello"), (0.8, 0.3, "$"), (1.1, 0.3, "aaa"), (1.4, 0.2, "$")]
    with pytest.raises(ValueError):
        text.alignment_token_spans(path[1:] + path[:1], tgt)
    # a run longer than replabel + 1 restarts (a a a a -> a <2> a): the word index follows the packing
    lex4 = text.load_lexicon(["aaaa\ta a a a |", "a\ta |"])
    for ws, names4, widx4 in ((["aaaa"], ["a", "<2>", "a", "|"], [0, 0, 0, -1]),
                              (["a", "aaaa", "a"], ["a", "|", "a", "<2>", "a", "|", "a", "|"], [0, -1, 1, 1, 1, -1, 2, -1])):
        t4 = text.target_indices(ws, lex4, d, "asg", replabel=2, wordsep="|")
        assert [d.get_entry(i) for i in t4] == names4
        assert text.target_word_index(ws, lex4, d, "asg", replabel=2, wordsep="|") == widx4


def test_word_pieces():
    pieces = ["_the", "_c", "at", "_cat", "s", "_", "t", "h", "e", "c", "a"]
    d = text.create_token_dict(pieces, "ctc")
    lex = text.load_lexicon(["the _the", "cats _cat s", "cat _c at"])
    words = ["the", "cats", "eat"]                                         # "eat": out of the lexicon, spelled _ e a t
    kw = dict(wordsep="_", use_wordpiece=True)
    tgt = text.target_indices(words, lex, d, "ctc", fallback_sep_left=True, fallback_sep_right=False, wordsep="_")
    assert [d.get_entry(i) for i in tgt] == ["_the", "_cat", "s", "_", "e", "a", "t"]
    widx = text.target_word_index(words, lex, d, "ctc", fallback_sep_left=True, fallback_sep_right=False, **kw)
    assert widx == [0, 1, 1, 2, 2, 2, 2] and len(widx) == len(tgt)
    b, i = d.get_index(text.BLANK), d.get_index
    path = [b, b, i("_the"), b, i("_cat"), i("_cat"), i("s"), b, i("_"), i("e"), i("a"), i("t"), i("t"), b]
    spans = text.alignment_token_spans(path, tgt, blank=b)
    segs = text.word_segments(spans, widx, words, frames=14, seconds_per_frame=0.04)
    assert [(round(s, 6), round(n, 6), w) for s, n, w in segs] == [
        (0.0, 0.08, "$"), (0.08, 0.04, "the"), (0.12, 0.04, "$"), (0.16, 0.12, "cats"), (0.28, 0.04, "$"), (0.32, 0.2, "eat"),
        (0.52, 0.04, "$")]
    _, rest, _ = parse_segments(text.format_alignment_line("wp", segs))
    assert [w for _, _, w in rest if w != "$"] == words
    # segments are ordered, do not overlap and cover [0, frames * seconds_per_frame]
    t = 0.0
    for s, n, _ in segs:
        assert abs(s - t) < 1e-9 and n >= 0
        t = s + n
    assert abs(t - 14 * 0.04) < 1e-9


def test_cpp_header_twins_compile_and_agree(tmp_path):
    """include/fl_compat/text.h: alignmentTokenSpans / targetWordIndex / wordSegments / formatAlignmentLine through
    tests/cpp/align_text_test.cpp -- plain g++, no device code; the worked examples of this file asserted in C++"""
    exe = str(tmp_path / "align_text_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "align_text_test.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True)
    assert "align text ok" in out.stdout
