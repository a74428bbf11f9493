"""w2l_asg_beam_search and w2l_asg_beam_search_lex on the GPU against the numpy restatement of their contract
(tests/asg_beam_ref.py).  G1 the exact recurrences at the enumeration shapes (small-integer emissions and transitions: every fp32 sum
is exact); G2 selection, merge, tie and end rules BITWISE against the fp32 restatement, with dense ties, for the plain, LM and lexicon
searches over both scan widths and both homes of the transition matrix (LDS: N * N * 4 <= 32 KiB, i.e. N <= 90; global beyond);
G3 zero transitions reduce to the three CTC siblings byte for byte; G4 the max search is w2l_viterbi_compute; G5 the log-sum search
against the float64 restatement; G6 the three surfaces; G7 `Decode --criterion=asg` end to end."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import asg_beam_ref as AR
from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR
from tests.test_gpu_ctc_beam import _close, _search as _ctc_search
from tests.test_gpu_ctc_beam_lex import _lex_table, _search_lex as _ctc_search_lex, _smear
from tests.test_gpu_ctc_beam_lm import _search_lm as _ctc_search_lm
from tests.test_gpu_ctc_beam_lm import _table as _lm_table

pytestmark = pytest.mark.gpu
INF = float("inf")
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("labels", "lengths", "scores", "lm_scores", "words", "word_counts")


def _lib():
    from wav2letter_amd import _lib
    return _lib


def _search(x, A, frames, W, K, M, Lmax, threshold=INF, log_add=False, normalize=False, lm=None, lm_weight=0.0, class_score=None,
            eos_score=0.0, lex=None, word_score=0.0, max_words=None):
    """the C ABI on numpy inputs -> the dict of asg_beam_ref.asg_beam (lm: an NGramLM, lex: a Lexicon)"""
    L = _lib()
    lib = L.lib()
    B, T, N = x.shape
    st = torch.cuda.current_stream().cuda_stream
    xd, ad = torch.tensor(x, device="cuda"), torch.tensor(np.asarray(A, F32), device="cuda")
    fd = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
    fp = fd.data_ptr() if fd is not None else None
    cd = torch.tensor(np.asarray(class_score, F32), device="cuda") if class_score is not None else None
    blob = lm.device_blob("cuda") if lm is not None else None
    size = lib.w2l_asg_beam_lex_workspace_size if lex is not None else lib.w2l_asg_beam_workspace_size
    ws = torch.empty(max(size(B, T, N, W, K), 256), dtype=torch.uint8, device="cuda")
    o = dict(labels=torch.full((B, M, Lmax), -7, dtype=torch.int32, device="cuda"),
             lengths=torch.full((B, M), -7, dtype=torch.int32, device="cuda"), scores=torch.full((B, M), 7.0, device="cuda"),
             lm_scores=torch.full((B, M), 7.0, device="cuda"))
    if lex is not None:
        max_words = Lmax if max_words is None else max_words
        o["words"] = torch.full((B, M, max_words), -7, dtype=torch.int32, device="cuda")
        o["word_counts"] = torch.full((B, M), -7, dtype=torch.int32, device="cuda")
        L.check(lib.w2l_asg_beam_search_lex(B, T, N, xd.data_ptr(), fp, ad.data_ptr(), W, K, threshold, int(log_add), int(normalize), M,
                                            Lmax, blob.data_ptr(), int(lm.has_eos), float(lm_weight), lex.device_blob("cuda").data_ptr(),
                                            float(word_score), float(eos_score), o["labels"].data_ptr(), o["lengths"].data_ptr(),
                                            o["scores"].data_ptr(), o["lm_scores"].data_ptr(), max_words, o["words"].data_ptr(),
                                            o["word_counts"].data_ptr(), ws.data_ptr(), st), "asg_beam_search_lex")
    else:
        L.check(lib.w2l_asg_beam_search(B, T, N, xd.data_ptr(), fp, ad.data_ptr(), W, K, threshold, int(log_add), int(normalize), M,
                                        Lmax, blob.data_ptr() if blob is not None else None, int(lm.has_eos) if lm is not None else 0,
                                        float(lm_weight), cd.data_ptr() if cd is not None else None, float(eos_score),
                                        o["labels"].data_ptr(), o["lengths"].data_ptr(), o["scores"].data_ptr(),
                                        o["lm_scores"].data_ptr(), ws.data_ptr(), st), "asg_beam_search")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def _same_bits(got, want):
    for k in KEYS:
        if k in want:
            assert got[k].dtype == want[k].dtype and (got[k].view(np.int32) == want[k].view(np.int32)).all(), k


def _eighths(rng, shape, lo, hi):
    return (rng.integers(lo * 8, hi * 8 + 1, size=shape) / 8).astype(F32)


# ---- G1: the exact recurrences ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,T", [(3, 4), (2, 8)])
def test_g1_exact_recurrences_at_the_enumeration_shapes(N, T):
    """small-integer emissions and transitions, W = 64, K = N: the beam never binds (45 and 16 labellings), every sum is exact in
    fp32 and in float64, so every labelling's score EQUALS the enumeration's over all N^T paths, in max mode; with an LM in eighths
    and lmWeight 0.5 too.  Integers tie: ranks are compared as a score-sorted set"""
    B = 4
    rng = np.random.default_rng(N * 100 + T)
    x = rng.integers(-6, 7, size=(B, T, N)).astype(F32)
    A = rng.integers(-3, 4, size=(N, N)).astype(F32)
    tb = LR.random_lm(rng, N, 3, 12, eighths=True)
    lm = _lm_table(tb)
    for use_lm in (False, True):
        got = _search(x, A, None, 64, N, 64, T, lm=lm if use_lm else None, lm_weight=0.5 if use_lm else 0.0,
                      eos_score=-0.25 if use_lm else 0.0)
        for b in range(B):
            want = (AR.enumerate_lm(x[b], A, tb, 0.5, None, -0.25, False, False) if use_lm
                    else AR.enumerate_labellings(x[b], A, False, False))
            n = len(want)
            assert (got["lengths"][b, :n] >= 0).all() and (got["lengths"][b, n:] == -1).all()
            mine = {tuple(got["labels"][b, m, :got["lengths"][b, m]]): float(got["scores"][b, m]) for m in range(n)}
            assert mine == want
            assert (np.diff(got["scores"][b, :n]) <= 0).all()
        print("G1", (N, T), "lm" if use_lm else "plain", "labellings", n)


# ---- G2: bitwise against the fp32 restatement --------------------------------------------------------------------------------

# name: (B, T, N, frames, W, K, threshold, M, Lmax, hot classes or None)
G2_SHAPES = {
    "n5_w8_k5_256_threads_lds": (3, 20, 5, [20, 1, 13], 8, 5, INF, 8, 20, None),
    "n30_w64_k30_1024_threads": (2, 14, 30, None, 64, 30, INF, 64, 14, None),
    "n30_threshold_short_rows": (3, 24, 30, [24, 9, 17], 16, 8, 2.5, 16, 4, None),
    "n70_k64_the_cap_below_n": (2, 12, 70, None, 16, 64, 3.0, 16, 12, None),
    "n100_global_transitions": (2, 14, 100, [14, 6], 16, 12, INF, 16, 14, 10),
    "n9998_t20": (2, 20, 9998, None, 64, 64, INF, 8, 20, 40),
    "t1": (3, 1, 30, None, 8, 8, INF, 8, 1, None),
}


@functools.lru_cache(maxsize=None)
def _zero_trans(N):
    return np.zeros((N, N), F32)                                     # shared and never written: N = 9997 is 400 MB


@functools.lru_cache(maxsize=None)
def _g2_trans(name):
    """a case's transitions, shared by its three variants: eighths in [-1, 1]; at N = 9998 only between the hot classes (the rest 0)"""
    N, hot = G2_SHAPES[name][2], G2_SHAPES[name][9]
    rng = np.random.default_rng(len(name))
    if N <= 100:
        return _eighths(rng, (N, N), -1, 1)
    A = np.zeros((N, N), F32)
    A[:hot, :hot] = _eighths(rng, (hot, hot), -1, 1)
    return A


@functools.lru_cache(maxsize=None)
def _g2_reference(name, variant):
    """inputs and the float32 restatement's outputs; emissions, transitions, LM values, smear values and scores in eighths from a
    few values, lmWeight a power of two: every sum is exact, ties are dense"""
    B, T, N, frames, W, K, thr, M, Lmax, hot = G2_SHAPES[name]
    rng = np.random.default_rng(len(name) * 100 + T + len(variant))
    x = _eighths(rng, (B, T, N), -3, 0)
    if hot is not None:                                              # the frame tokens are among the first `hot` classes
        x[:, :, hot:] -= 3
    A = _g2_trans(name)
    kw = dict(threshold=thr, log_add=False, normalize=False)
    tb = trie = None
    if variant == "lm":
        tb = LR.random_lm(rng, N, 3, 300, eighths=True, hot=min(N, hot or 30))
        kw.update(lm=tb, lm_weight=0.5, class_score=_eighths(rng, N, -1, 1), eos_score=-0.25)
    if variant == "lex":
        nwords = 200 if N > 5 else 40
        sil = (hot or min(N, 30)) - 1
        rows = XR.random_lexicon(rng, N, nwords, 3, 0.1, sil, hot or min(N, 30))
        tb = LR.random_lm(rng, nwords, 3, 300, eighths=True)
        trie = XR.TextbookTrie(rows, N, nwords, _smear(tb, nwords), sil)
        kw.update(lm=tb, lm_weight=0.5, word_score=0.25, eos_score=-0.25)
    want = AR.asg_beam(x, A, frames, W, K, M, Lmax, F32, trie=trie, **kw)
    d = want["diags"]
    facts = {k: sum(getattr(g, k) for g in d) for k in ("cuts", "skipped", "merges", "eos_moves", "end_dropped")}
    assert (want["lengths"] >= 0).any() and (T == 1 or facts["skipped"] > 0), (name, variant, facts)
    assert facts["merges"] > 0 or W < 2 or T < 3, (name, variant, facts)
    assert facts["cuts"] > 0 or name in ("t1",), (name, variant, facts)
    return x, A, tb, trie, kw, want, facts


@pytest.mark.parametrize("variant", ["plain", "lm", "lex"])
@pytest.mark.parametrize("name", list(G2_SHAPES))
def test_g2_bitwise_against_the_float32_restatement(name, variant):
    B, T, N, frames, W, K, thr, M, Lmax, hot = G2_SHAPES[name]
    x, A, tb, trie, kw, want, facts = _g2_reference(name, variant)
    print("G2", name, variant, facts, "hypotheses", int((want["lengths"] >= 0).sum()), "longest", int(want["lengths"].max()))
    assert (N * N * 4 <= 32 * 1024) == (N <= 90)                     # which side of the LDS budget the case is on
    if name == "n30_threshold_short_rows":
        assert want["lengths"].max() > Lmax
    gkw = dict(kw)
    if tb is not None:
        gkw["lm"] = _lm_table(tb)
    got = _search(x, A, frames, W, K, M, Lmax, lex=_lex_table(trie) if trie is not None else None, **gkw)
    _same_bits(got, want)
    if variant == "plain":
        assert (got["lm_scores"][got["lengths"] >= 0] == 0).all()


# ---- G3: zero transitions are the CTC siblings ---------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,N,W,K,thr,log_add", [(3, 24, 30, 16, 8, 6.0, False), (3, 24, 30, 64, 30, INF, True),
                                                    (2, 20, 9997, 64, 64, INF, False), (2, 16, 9997, 16, 8, INF, True)])
def test_g3_zero_transitions_are_the_ctc_siblings(B, T, N, W, K, thr, log_add):
    """trans = 0, normalize = 0: labels, lengths and scores are byte-identical to the CTC sibling's on the same emissions with a
    column of -inf appended as blank (x + 0 and (+) with -inf are exact); the lexicon-free ASG call with lm = NULL is held to
    w2l_ctc_beam_search, whose scan is the one-wavefront lazy one"""
    rng = np.random.default_rng(N + T + W)
    x = rng.normal(0, 2, size=(B, T, N)).astype(F32) if log_add else _eighths(rng, (B, T, N), -3, 0)
    x[:, :, :12] += 10 if log_add else 3                             # the frame tokens are among the lexicon's twelve letters
    xb = np.concatenate([x, np.full((B, T, 1), -np.inf, F32)], axis=2)
    A = _zero_trans(N)
    frames = [T, T // 3, 1][:B]
    M = min(W, 8)
    got = _search(x, A, frames, W, K, M, T, thr, log_add)
    lab, ln, sc = _ctc_search(xb, frames, W, K, thr, log_add, False, M, T)
    _same_bits(got, dict(labels=lab, lengths=ln, scores=sc))
    assert (ln >= 0).any() and ln.max() > 1
    tb = LR.random_lm(rng, N, 3, 500, hot=min(N, 300))
    lm, cs = _lm_table(tb), rng.normal(0, 0.5, N).astype(F32)
    got = _search(x, A, frames, W, K, M, T, thr, log_add, lm=lm, lm_weight=0.75, class_score=cs, eos_score=-0.25)
    lab, ln, sc, lms = _ctc_search_lm(xb, frames, W, K, thr, log_add, False, M, T, lm, 0.75, cs, -0.25)
    _same_bits(got, dict(labels=lab, lengths=ln, scores=sc, lm_scores=lms))
    nwords = 150
    wtb = LR.random_lm(rng, nwords, 3, 300)
    trie = XR.TextbookTrie(XR.random_lexicon(rng, N, nwords, 3, 0.1, 11, 12), N, nwords, _smear(wtb, nwords), 11)
    lex, wlm = _lex_table(trie), _lm_table(wtb)
    got = _search(x, A, frames, W, K, M, T, thr, log_add, lm=wlm, lm_weight=0.75, lex=lex, word_score=0.5, eos_score=-0.25)
    ref = _ctc_search_lex(xb, frames, W, K, thr, log_add, False, M, T, T, lex, wlm, 0.75, 0.5, -0.25)
    _same_bits(got, dict(zip(KEYS, ref)))
    assert (ref[5] > 0).any()


# ---- G4: the max search is Viterbi ---------------------------------------------------------------------------------------------

def _path_score(x, A, path):
    """the path's score accumulated in the recursion's order: (p + A[c][e]) + x[t][c], fp32"""
    s = F32(x[0, path[0]])
    for t in range(1, len(path)):
        s = F32(F32(s + A[path[t], path[t - 1]]) + x[t, path[t]])
    return s


def _viterbi_gpu(x, A):
    from wav2letter_amd import ASGLoss
    crit = ASGLoss(x.shape[2]).cuda()
    with torch.no_grad():
        crit.transitions.copy_(torch.tensor(A))
    return crit.viterbiPath(torch.tensor(x, device="cuda")).cpu().numpy()


def test_g4_max_search_is_viterbi_where_the_beam_cannot_bind():
    """max mode, no LM, normalize = 0, N = 3, T = 4, W = 64 (45 labellings: the beam can never bind): the 1-best labels are the
    collapsed w2l_viterbi_compute path and the score is that path's, accumulated in the recursion's order, bit for bit"""
    B, T, N = 16, 4, 3
    rng = np.random.default_rng(44)
    x, A = rng.normal(0, 2, size=(B, T, N)).astype(F32), rng.normal(0, 1.5, size=(N, N)).astype(F32)
    paths = _viterbi_gpu(x, A)
    got = _search(x, A, None, 64, N, 1, T)
    for b in range(B):
        lab = AR.collapse([int(c) for c in paths[b]])
        assert tuple(got["labels"][b, 0, :got["lengths"][b, 0]]) == lab
        assert got["scores"][b, 0].view(np.int32) == _path_score(x[b], A, paths[b]).view(np.int32)


def test_g4_max_search_is_viterbi_on_peaked_emissions():
    """N = 30, T = 40, W = 64, K = 30, peaked emissions.  The precondition, asserted on the restatement: after every frame the
    collapsed prefix of the Viterbi path is in the beam (zero cuts on the winner's lineage)"""
    B, T, N = 3, 40, 30
    rng = np.random.default_rng(45)
    x = rng.normal(0, 1, size=(B, T, N)).astype(F32)
    for b in range(B):
        peak = np.repeat(rng.integers(0, N, T // 4 + 1), 4)[:T]
        x[b, np.arange(T), peak] += 6
    A = (rng.normal(0, 0.5, size=(N, N)) + 1.5 * np.eye(N)).astype(F32)
    paths = _viterbi_gpu(x, A)
    got = _search(x, A, None, 64, 30, 1, T)
    for b in range(B):
        path = [int(c) for c in paths[b]]
        ref_path, ref_score = AR.viterbi(x[b], A)
        assert path == ref_path
        track = [AR.collapse(path[:t + 1]) for t in range(T)]
        hyps, dg = AR.asg_beam_one(x[b], A, T, 64, 30, track=track)
        assert dg.track_lost == 0 and dg.cuts > 0                    # the beam binds, but never on the winner's lineage
        assert hyps[0][0] == track[-1] and len(track[-1]) > 3
        assert tuple(got["labels"][b, 0, :got["lengths"][b, 0]]) == track[-1]
        assert got["scores"][b, 0].view(np.int32) == _path_score(x[b], A, path).view(np.int32) == ref_score.view(np.int32)


# ---- G5: the log-sum search against the float64 restatement -----------------------------------------------------------------

G5_SKIPPED_SHARE = 0.25     # at most this share of the live rows may go uncompared (measured on the restatement alone: see the test)
G5_CASES = [  # (variant, B, T, N, W, K, M, extra roundings per frame)
    ("plain", 6, 16, 30, 8, 5, 4, 0), ("lm", 6, 16, 30, 8, 5, 4, 1), ("lex", 6, 16, 30, 8, 5, 4, 4), ("plain", 4, 12, 100, 64, 20, 4, 0),
]


@functools.lru_cache(maxsize=None)
def _g5_reference(i):
    variant, B, T, N, W, K, M, extra = G5_CASES[i]
    rng = np.random.default_rng(500 + i)
    x = rng.normal(0, 3, size=(B, T, N)).astype(F32)
    x[:, :, :8] += 6
    A = rng.normal(0, 1, size=(N, N)).astype(F32)
    kw = dict(log_add=True, normalize=False)
    tb = trie = None
    if variant == "lm":
        tb = LR.random_lm(rng, N, 3, 300)
        kw.update(lm=tb, lm_weight=0.8, eos_score=-0.3)
    if variant == "lex":
        nwords = 60
        tb = LR.random_lm(rng, nwords, 3, 200)
        trie = XR.TextbookTrie(XR.random_lexicon(rng, N, nwords, 3, 0.1, 7, 8), N, nwords, _smear(tb, nwords), 7)
        kw.update(lm=tb, lm_weight=0.8, word_score=0.3, eos_score=-0.3)
    want = AR.asg_beam(x, A, None, W, K, M, T, np.float64, trie=trie, **kw)
    # the leading ranks of every utterance that the bound lets us compare: every decision on the lineage of each of them, the frame
    # token choices of the utterance and the gap to the next rank exceed TWICE the bound
    lead = []
    for b, dg in enumerate(want["diags"]):
        dl = AR.delta_asg(T, dg.S, extra)
        n = 0
        if dg.token_gap > 2 * dl:
            while n < len(dg.margins) and dg.margins[n] > 2 * dl and (n >= len(dg.final_gaps) or dg.final_gaps[n] > 2 * dl):
                n += 1
        lead.append((n, dl))
    return x, A, tb, trie, kw, want, lead


@pytest.mark.parametrize("i", range(len(G5_CASES)))
def test_g5_log_sum_search_against_the_float64_restatement(i):
    """logAdd = 1.  The bound is asg_beam_ref.delta_asg: ctc_beam_ref.delta's derivation with the per-frame transition add counted
    (and the siblings' LM or lexicon adds).  Only the leading ranks whose every decision has a margin above twice the bound are
    compared; the rest is skipped, and at most G5_SKIPPED_SHARE of the live rows may be (on the restatement alone these inputs skip
    0 to 17 percent)"""
    variant, B, T, N, W, K, M, extra = G5_CASES[i]
    x, A, tb, trie, kw, want, lead = _g5_reference(i)
    live = int((want["lengths"] >= 0).sum())
    compared = sum(n for n, _ in lead)
    print("G5", G5_CASES[i], "live rows", live, "compared", compared, "skipped share", 1 - compared / live,
          "delta", max(dl for _, dl in lead), "cuts", sum(d.cuts for d in want["diags"]))
    assert live > 0 and 1 - compared / live <= G5_SKIPPED_SHARE
    assert sum(d.cuts for d in want["diags"]) > 0                    # the beam binds
    gkw = dict(kw)
    if tb is not None:
        gkw["lm"] = _lm_table(tb)
    got = _search(x, A, None, W, K, M, T, lex=_lex_table(trie) if trie is not None else None, **gkw)
    for b, (n, dl) in enumerate(lead):
        for k in ("labels", "lengths") + (("words", "word_counts") if trie is not None else ()):
            assert (got[k][b, :n] == want[k][b, :n]).all(), (b, k)
        assert (np.abs(got["scores"][b, :n].astype(np.float64) - want["scores"][b, :n]) <= dl).all(), b
        assert _close(got["scores"][b, :n], want["scores"][b, :n]).all()
        if variant != "plain":
            assert (got["lm_scores"][b, :n].view(np.int32) == want["lm_scores"][b, :n].view(np.int32)).all()


# ---- G6: the three surfaces ------------------------------------------------------------------------------------------------------

def test_g6_three_surfaces_agree(tmp_path):
    """C ABI == Python (criterion.asg_beam_search, ASGLoss.beamSearch) == compiled C++ ASGLoss::beamSearch (tests/cpp/
    decode_asg_caller.cpp, plain g++ against libw2l_hip.so), without LM, with a token LM and with a lexicon read from the same file
    with replabel = 1 and a word LM read from the same ARPA file"""
    from tests.test_ctc_beam_lm_host import _arpa_text
    from wav2letter_amd import ASGLoss, Lexicon, NGramLM, criterion, text
    exe, libdir = str(tmp_path / "decode_asg_caller"), os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "decode_asg_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    rng = np.random.default_rng(8)
    N, nwords, hot = 30, 120, 8
    tokens = [f"t{c}" for c in range(N - 1)] + [text.replabel_token(1)]
    rows = XR.random_lexicon(rng, N - 1, nwords, 3, 0.1, hot - 1, hot)
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n")
    (tmp_path / "lex.txt").write_text("".join(f"word{w:03d} " + " ".join(tokens[t] for t in sp) + "\n" for w, sp in rows))
    assert any(a == b for _, sp in rows for a, b in zip(sp, sp[1:]))              # doubled tokens: packed to t<c> <1>
    dic = text.Dictionary(tokens)
    plain = Lexicon.from_file(tmp_path / "lex.txt", dic, smearing="none", sil=tokens[hot - 1], replabel=1)
    (tmp_path / "words.arpa").write_text(_arpa_text(LR.random_lm(rng, nwords, 3, 200), plain.words, unk10=-3.0)[0])
    (tmp_path / "tokens.arpa").write_text(_arpa_text(LR.random_lm(rng, N, 3, 200), tokens, unk10=-3.0)[0])
    wlm = NGramLM.from_arpa(tmp_path / "words.arpa", plain.words)
    tlm = NGramLM.from_arpa(tmp_path / "tokens.arpa", tokens)
    lex = Lexicon.from_file(tmp_path / "lex.txt", dic, lm=wlm, sil=tokens[hot - 1], replabel=1)
    A = rng.normal(0, 1, size=(N, N)).astype(F32)
    crit = ASGLoss(N).cuda()
    with torch.no_grad():
        crit.transitions.copy_(torch.tensor(A))
    for mode, (B, T, W, K, M, Lmax, maxw, log_add, thr) in [("plain", (3, 25, 8, 5, 3, 25, 25, 0, INF)), ("lm", (4, 31, 8, 5, 3, 31, 31, 1, INF)),
                                                            ("lex", (2, 20, 64, 64, 16, 6, 2, 0, 8.0))]:
        x = rng.normal(0, 2, size=(B, T, N)).astype(F32)
        x[:, :, :hot] += 4
        x[:, :, N - 1] += 4
        frames = rng.integers(1, T + 1, B).astype(np.int32)
        frames[1] = 1
        lmw, wsc, eos_score = 0.75, 0.5, -0.25
        kw, okw, args = {}, {}, []
        if mode == "lm":
            kw = okw = dict(lm=tlm, lm_weight=lmw, eos_score=eos_score)
            args = [str(tmp_path / "tokens.txt"), str(tmp_path / "tokens.arpa")]
        if mode == "lex":
            kw = dict(lm=wlm, lm_weight=lmw, lex=lex, word_score=wsc, eos_score=eos_score, max_words=maxw)
            okw = dict(lm=wlm, lm_weight=lmw, lexicon=lex, word_score=wsc, eos_score=eos_score, max_words=maxw)
            args = [str(tmp_path / "tokens.txt"), str(tmp_path / "words.arpa"), str(tmp_path / "lex.txt"), tokens[hot - 1], "1"]
        want_f = _search(x, A, frames, W, K, M, Lmax, thr, bool(log_add), **kw)
        want = _search(x, A, None, W, K, M, Lmax, thr, bool(log_add), **kw)
        keys = KEYS[:3] + (KEYS[3:4] if mode != "plain" else ()) + (KEYS[4:] if mode == "lex" else ())
        assert (want["lengths"] >= 0).any() and (mode != "lex" or (want["word_counts"] > 0).any())
        xd, fd = torch.tensor(x, device="cuda"), torch.tensor(frames, device="cuda")
        opts = dict(beam=W, beam_token=K, threshold=thr, log_add=bool(log_add), nbest=M, max_len=Lmax, **okw)
        for got, ref in ((crit.beamSearch(xd, fd, **opts), want_f), (crit.beamSearch(xd, **opts), want),
                         (criterion.asg_beam_search(xd, crit.transitions, fd, **opts), want_f)):
            assert len(got) == len(keys)
            assert all((g.cpu().numpy().view(np.int32) == ref[k].view(np.int32)).all() for g, k in zip(got, keys))
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([N, T, B, W, K, M, Lmax, maxw, log_add, 0], np.int32).tobytes()
                    + np.array([thr, lmw, wsc, eos_score], F32).tobytes() + x.tobytes() + frames.tobytes() + A.tobytes())
        run = subprocess.run([exe, inp, outp] + args, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "decode asg caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
        out = np.fromfile(outp, np.int32)
        at = 0
        for ref in (want_f, want):
            for k in keys:
                n = ref[k].size
                assert (out[at:at + n] == ref[k].view(np.int32).ravel()).all(), (mode, k)
                at += n
        assert at == len(out)


# ---- G7: Decode --criterion=asg end to end, on the six-WAV fixture of tests/list_fixture.py ---------------------------------

from tests.list_fixture import ENV, LETTERS, TRAIN_EXE, UTTS, _fixture  # noqa: E402
from tests.test_gpu_ctc_beam import DECODE_EXE, _sclite_lines, trained  # noqa: E402,F401  (the CTC checkpoint, for the refusal)


@pytest.fixture(scope="module")
def trained_asg(tmp_path_factory):
    d = tmp_path_factory.mktemp("decode_asg")
    _fixture(d)
    cmd = [TRAIN_EXE, "train", f"--archdir={d / 'arch'}", "--arch=net.arch", "--criterion=asg", "--replabel=1", "--transdiag=0.5",
           "--filterbanks=40", f"--tokensdir={d}", "--tokens=tokens.txt", f"--lexicon={d / 'lexicon.txt'}", f"--datadir={d}",
           "--train=train.lst", "--batchsize=3", "--iter=6", "--reportiters=3", "--lr=0.05", "--lrcrit=0.002", "--momentum=0.8",
           "--maxgradnorm=1.0", "--onorm=target", "--sqnorm=true", f"--rundir={d / 'run'}", "--runname=exp"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return d, d / "run" / "exp" / "001_model_last.bin"


def test_g7_decode_tool_asg_end_to_end(trained_asg, tmp_path):
    """Decode of an ASG checkpoint trained with --replabel=1: with --logadd=false the hypotheses are the Viterbi transcripts of the
    same model (checkpoint.load, the eval forward on the features Decode dumped, w2l_viterbi_compute under the checkpoint's
    transitions, tkn_prediction_to_ltr with the replabel); the beam dump is well formed; with a token LM the dump carries lmScore;
    with the lexicon (spellings packed with the replabel) the hypotheses are lexicon words only"""
    from tests.test_ctc_beam_lm_host import _arpa_text
    from tests.test_gpu_ctc_beam_lex import _lexicon_files
    from wav2letter_amd import ASGLoss, checkpoint, text
    from wav2letter_amd.trainer import Trainer
    d, model = trained_asg
    common = [DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}"]
    res = subprocess.run(common + ["--show=true", f"--w2l_dump_features={d / 'dfeat'}"], capture_output=True, text=True, timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "AutoSegmentationCriterion, 29 classes" in res.stderr
    hyp, ref = _sclite_lines(d / "out" / "other.hyp"), _sclite_lines(d / "out" / "other.ref")
    assert [s for _, s in hyp] == [s for _, s in ref] == [f"u{k}" for k in range(5)]
    assert [w for w, _ in ref] == [tr.split() for _, tr in UTTS[:5]]
    assert "-- WER: " in res.stdout

    dic = text.create_token_dict(LETTERS, "asg", 1)
    N = dic.index_size()
    assert N == 29
    arch = (d / "arch" / "net.arch").read_text()
    viterbi = []
    for k in range(3):                                                  # batches of 2, 2, 1 in list order
        utts = UTTS[2 * k:2 * k + 2][:5 - 2 * k]
        raw = (d / f"dfeat.{k + 1}").read_bytes()
        B, nfeat, T = (int(v) for v in np.frombuffer(raw[:12], np.int32))
        x = torch.tensor(np.frombuffer(raw[12:], np.float32).reshape(B, nfeat, T).copy()).cuda()
        tr_ = Trainer(arch, nfeat, N, "asg", 4, 0.5)                     # --onorm=target --sqnorm=true --transdiag=0.5
        checkpoint.load(str(model), tr_, arch)
        tr_.plan(B, T, 8)
        tr_.to_device()
        em = tr_.forward(x, train=False).clone()
        Tout = em.shape[1]
        frames = [min(max(-(-min(1 + (n - 400) // 160, T) * Tout // T), 1), Tout) for n, _ in utts]
        crit = ASGLoss(N).cuda()
        with torch.no_grad():
            crit.transitions.copy_(tr_.params[tr_.n_net:tr_.n_net + N * N].view(N, N))
        assert not torch.equal(crit.transitions.detach(), 0.5 * torch.eye(N, device="cuda"))       # trained transitions
        for b in range(B):                                              # Viterbi over the utterance's own frames
            path = crit.viterbiPath(em[b:b + 1, :frames[b]].contiguous()).cpu().numpy()[0]
            viterbi.append(text.tkn2wrd(text.tkn_prediction_to_ltr(path, dic, "asg", replabel=1, wordsep="|"), "|"))
    assert [w for w, _ in hyp] == viterbi

    # the beam dump, both (+) modes: three well-formed lines per sample, scores non-increasing
    for extra in ([], ["--logadd=true"]):
        res = subprocess.run(common + ["--isbeamdump=true", "--nbest=3", "--beamsize=16", "--beamthreshold=100"] + extra,
                             capture_output=True, text=True, timeout=600, env=ENV)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        rows = [line.split(" | ") for line in (d / "out" / "other.hyp").read_text().splitlines()]
        assert len(rows) == 15 and all(len(r) == 6 for r in rows)
        for k in range(5):
            mine = rows[3 * k:3 * k + 3]
            assert [r[0] for r in mine] == [f"u{k}"] * 3
            scores = [float(r[1]) for r in mine]
            assert scores == sorted(scores, reverse=True) and all(np.isfinite(scores))
            assert all(r[1] == r[2] and float(r[3]) == 0.0 and float(r[4]) >= 0.0 for r in mine)
            if not extra:
                assert mine[0][5].split() == viterbi[k]

    # a token LM over the 29 classes, the replabel among them
    tokens = [dic.get_entry(c) for c in range(N)]
    (tmp_path / "tokens.arpa").write_text(_arpa_text(LR.random_lm(np.random.default_rng(3), N, 3, 80), tokens, unk10=-3.0)[0])
    res = subprocess.run(common + [f"--lm={tmp_path / 'tokens.arpa'}", "--lmweight=0.5", "--isbeamdump=true", "--nbest=2", "--beamsize=16",
                                   "--beamthreshold=100"], capture_output=True, text=True, timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = [line.split(" | ") for line in (d / "out" / "other.hyp").read_text().splitlines()]
    assert len(rows) == 10 and all(len(r) == 6 and float(r[3]) < 0 for r in rows)
    assert all(abs(float(r[1]) - (float(r[2]) + 0.5 * float(r[3]))) <= 1e-4 * max(1.0, abs(float(r[1]))) for r in rows)

    # the lexicon: spellings packed with the replabel, silence between the words
    lex_path, arpa, words = _lexicon_files(tmp_path)
    res = subprocess.run(common + ["--beamsize=16", "--beamthreshold=100", "--uselexicon=true", "--decodertype=wrd", f"--lexicon={lex_path}",
                                   f"--lm={arpa}", "--lmweight=0.5", "--wordscore=6", "--smearing=max"],
                         capture_output=True, text=True, timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "--lexicon: 26 words" in res.stderr and "silence token |" in res.stderr
    hyp = _sclite_lines(d / "out" / "other.hyp")
    assert [s for _, s in hyp] == [f"u{k}" for k in range(5)] and all(set(w) <= set(words) for w, _ in hyp)
    assert any(w for w, _ in hyp)


def test_g7_a_ctc_checkpoint_is_not_decoded_as_asg(trained):
    d, model = trained
    res = subprocess.run([DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--criterion=asg"], capture_output=True, text=True,
                         timeout=120, env=ENV)
    assert res.returncode != 0 and "--criterion=asg" in res.stderr and "--criterion=ctc" in res.stderr, (res.returncode, res.stderr)


def test_g7_an_asg_checkpoint_is_not_decoded_as_ctc(trained_asg):
    d, model = trained_asg
    res = subprocess.run([DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--criterion=ctc"], capture_output=True, text=True,
                         timeout=120, env=ENV)
    assert res.returncode != 0 and "--criterion" in res.stderr, (res.returncode, res.stderr)
