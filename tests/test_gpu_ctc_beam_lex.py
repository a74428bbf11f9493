"""w2l_ctc_beam_search_lex on the GPU against the numpy restatement of its contract (tests/ctc_beam_lex_ref.py).
X1 the exact recurrences at the enumeration shapes; X2 selection, merge, homophone, silence, tie and end rules BITWISE (logAdd = 0;
emissions, LM values, smear values and wordScore multiples of 1/8, lmWeight a power of two: every sum is exact in fp32 and ties are
dense); X3 identity with w2l_ctc_beam_search_lm on a lexicon of one-token words; X4 the log-sum search with the beam binding, on
inputs whose every decision has a margin; then the surfaces (C ABI == Python == compiled C++) and `Decode --uselexicon=true
--decodertype=wrd` end to end with its refusals."""
import functools

import numpy as np
import pytest
import torch

from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR
from tests.test_gpu_ctc_beam import _close, _ints
from tests.test_gpu_ctc_beam_lm import _search_lm
from tests.test_gpu_ctc_beam_lm import _table as _lm_table

pytestmark = pytest.mark.gpu
INF = float("inf")
F32 = np.float32


def _lib():
    from wav2letter_amd import _lib
    return _lib


def _lex_table(trie):
    from wav2letter_amd import Lexicon
    return Lexicon.from_spellings(trie.rows, trie.num_tokens, trie.num_words, trie.word_smear, trie.sil)


def _smear(tb, nwords):
    """max smearing: wordSmear[w] = q(start, w)"""
    return np.array([tb.score(tb.history(()), w, F32) for w in range(nwords)], F32)


def _search_lex(x, frames, W, K, threshold, log_add, normalize, M, Lmax, max_words, lex, lm, lmw, word_score, eos_score):
    """the C ABI on numpy inputs -> labels, lengths, scores, lmScores, words, wordCounts"""
    L = _lib()
    lib = L.lib()
    B, T, N = x.shape
    st = torch.cuda.current_stream().cuda_stream
    xd = torch.tensor(x, device="cuda")
    fd = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
    blob, lblob = lm.device_blob("cuda"), lex.device_blob("cuda")
    ws = torch.empty(max(lib.w2l_ctc_beam_lex_workspace_size(B, T, N, W, K), 256), dtype=torch.uint8, device="cuda")
    labels = torch.full((B, M, Lmax), -7, dtype=torch.int32, device="cuda")
    lengths = torch.full((B, M), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((B, M), 7.0, device="cuda")
    lms = torch.full((B, M), 7.0, device="cuda")
    words = torch.full((B, M, max_words), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((B, M), -7, dtype=torch.int32, device="cuda")
    L.check(lib.w2l_ctc_beam_search_lex(B, T, N, xd.data_ptr(), fd.data_ptr() if fd is not None else None, W, K, threshold,
                                        int(log_add), int(normalize), M, Lmax, blob.data_ptr(), int(lm.has_eos), float(lmw),
                                        lblob.data_ptr(), float(word_score), float(eos_score), labels.data_ptr(), lengths.data_ptr(),
                                        scores.data_ptr(), lms.data_ptr(), max_words, words.data_ptr(), counts.data_ptr(),
                                        ws.data_ptr(), st), "ctc_beam_search_lex")
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (labels, lengths, scores, lms, words, counts))


# ---- X1: the exact recurrences ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,T", [(3, 5), (4, 3)])
def test_x1_exact_recurrences_at_the_enumeration_shapes(N, T):
    """W = 64, K = N-1, no threshold: the beam never binds (asserted) and every hypothesis the lexicon allows is there.  The float64
    restatement takes the smear, q and word terms in fp32 as the contract has them, so both sides share them; the ranks compared
    are those whose gaps are >= 10 delta: all of them (asserted)"""
    from tests.test_ctc_beam_lex_host import _tiny
    rows, sil, nwords = _tiny(N)
    B = 3
    rng = np.random.default_rng(100 + N)
    tb = LR.random_lm(rng, nwords, 3, 40)     # dense in bigrams: `A B` and `B A` on one spelling are no mathematical tie
    trie = XR.TextbookTrie(rows, N - 1, nwords, _smear(tb, nwords), sil)
    lmw, word_score, eos_score = 0.7, -0.3, -0.4
    x = np.stack([np.random.default_rng(seed).normal(0, 2, size=(T, N)) for seed in X1_SEEDS[N]]).astype(F32)
    M = min(len(XR.beam_search_lex_one(x[b], T, 64, N - 1, trie, tb, lmw, word_score, eos_score, INF, True, True, np.float64)[0])
            for b in range(B))
    lab, ln, sc, lms, wd, wc, diags = XR.beam_search_lex(x, None, 64, N - 1, trie, tb, lmw, word_score, eos_score, INF, True, True, M,
                                                         T, T, np.float64)
    glab, gln, gsc, glms, gwd, gwc = _search_lex(x, None, 64, N - 1, INF, True, True, M, T, T, _lex_table(trie), _lm_table(tb), lmw,
                                                 word_score, eos_score)
    print("X1", N, T, "hypotheses at the root", M, "max |score diff|", np.abs(gsc - sc).max())
    assert M >= 20 and (gln >= 0).all() and _close(gsc, sc).all()
    for b in range(B):
        assert diags[b].beam_gap == np.inf
        dl = XR.delta_lex(T, diags[b].S)
        lead = 0
        while lead < M - 1 and diags[b].final_gaps[lead] >= 10 * dl:
            lead += 1
        print("X1 seed", b, "delta", dl, "leading ranks with a margin", lead, "smallest gap", min(diags[b].final_gaps))
        assert lead == M - 1
        assert (gln[b] == ln[b]).all() and (glab[b] == lab[b]).all() and (gwc[b] == wc[b]).all() and (gwd[b] == wd[b]).all()
        assert (glms[b].view(np.int32) == lms[b].view(np.int32)).all()      # lmScores is fp32 on both sides: exact
        assert len({(tuple(glab[b, m, :gln[b, m]]), tuple(gwd[b, m, :gwc[b, m]])) for m in range(M)}) == M


X1_SEEDS = {3: (1, 2, 3), 4: (0, 2, 3)}     # seeds at which every final gap is >= 10 delta (asserted)


# ---- X2: selection, merge, homophone, silence, tie and end rules, bit for bit ------------------------------------------------

def _hot(rng, B, T, N, hot):
    """multiples of 1/8: the first `hot` classes and the blank in [-3, 0], the rest in [-6, -3.125]: the frame tokens are hot ones"""
    x = (rng.integers(-48, -24, size=(B, T, N)) / 8).astype(F32)
    x[:, :, :hot] = rng.integers(-24, 1, size=(B, T, hot)) / 8
    x[:, :, N - 1] = rng.integers(-24, 1, size=(B, T)) / 8
    return x


# name: (B, T, N, frames, W, K, threshold, M, Lmax, maxWords, hot classes or None,
#        (words, longest spelling, shortest, homophone fraction, silence token, words crowded on word 0's spelling),
#        (LM order, n-grams per order, eos), lmWeight, wordScore, eosScore, seed)
X2_CASES = {
    "full_width_frames": (3, 24, 9998, [24, 1, 17], 64, 64, INF, 64, 24, 24, 80, (3000, 3, 1, 0.02, None, 0), (3, 4000, True), 0.5, -0.25, -0.25, 0),
    "w32_k5_threshold_m1": (2, 20, 30, None, 32, 5, 2.5, 1, 20, 20, None, (300, 3, 1, 0.1, 28, 0), (3, 300, True), 0.5, 0.25, 0.0, 2),
    "w1_k1": (2, 16, 30, None, 1, 1, INF, 1, 16, 16, None, (300, 2, 1, 0.1, 28, 0), (3, 300, True), 1.0, 0.0, 0.0, 1),
    "n30_silence_short_rows": (3, 30, 30, [30, 9, 22], 16, 8, 4.0, 16, 3, 2, None, (200, 3, 1, 0.1, 28, 0), (3, 300, True), 0.5, 0.5, 0.5, 1),
    "n30_seven_homophones": (2, 16, 30, None, 16, 8, INF, 16, 16, 16, 6, (40, 2, 1, 0.0, None, 6), (2, 100, True), 0.5, 0.0, 0.0, 2),
    "n30_nothing_at_the_root": (2, 12, 30, [2, 12], 4, 3, 2.5, 4, 12, 12, None, (200, 3, 2, 0.0, None, 0), (3, 300, True), 0.5, 0.25, 0.0, 0),
    "n30_negative_weight": (2, 20, 30, None, 16, 8, INF, 16, 20, 20, None, (60, 3, 1, 0.15, 28, 0), (3, 300, True), -0.25, -0.5, 0.25, 0),
    "n30_no_eos": (2, 20, 30, [20, 13], 16, 8, 4.0, 16, 20, 20, None, (300, 3, 1, 0.1, 28, 0), (3, 300, False), 0.5, -0.125, 0.0, 5),
}


@functools.lru_cache(maxsize=None)
def _x2_reference(name):
    return _x2_build(name, X2_CASES[name][-1])


def _x2_build(name, seed):
    """inputs, the float32 restatement's outputs, and the proof on the CPU that the case is not vacuous.  Every case must show that
    the lexicon removed a candidate a search without it had in reach of its beam (LexDiag.removed).  The other facts are asserted
    wherever the case's shape allows them at all -- a DELIBERATE limit: a merge needs two beam entries (impossible at W = 1), a
    homophone candidate and a tie decided by the slot need a node with two words (the lexicon of n30_nothing_at_the_root, spellings of two
    tokens and more over 29 letters, has no homophones; the case is kept for the path it alone reaches), a silence loop needs a silence token,
    and an end-drop can change the best only where word-internal entries can lead (not at w1_k1 on one-token words: its beam is one
    entry, printed)."""
    (B, T, N, frames, W, K, thr, M, Lmax, maxw, hot, (nwords, max_len, min_len, homo, sil, crowd), (order, per, eos), lmw, wsc,
     eos_score, _) = X2_CASES[name]
    rng = np.random.default_rng(len(name) * 1000 + T + seed)
    x = _ints(rng, B, T, N) if hot is None else _hot(rng, B, T, N, hot)
    rows = XR.random_lexicon(rng, N - 1, nwords, max_len, homo, sil, hot, crowd, min_len)
    if name == "n30_nothing_at_the_root":     # utterance 0: token 5 at frame 0, blank after it, and no word is spelled `5`
        rows = [r for r in rows if r[1][0] != 5] + [(nwords, [5, 6])]
        nwords += 1
        x[0] = -3.0
        x[0, 0, 5] = 4.0
        x[0, 1:, N - 1] = 0.0
    tb = LR.random_lm(rng, nwords, order, per, True, eos, (), eighths=True)
    trie = XR.TextbookTrie(rows, N - 1, nwords, _smear(tb, nwords), sil)
    out = XR.beam_search_lex(x, frames, W, K, trie, tb, lmw, wsc, eos_score, thr, False, False, M, Lmax, maxw, F32)
    diags = out[6]
    facts = {k: sum(getattr(d, k) for d in diags) for k in ("blocked", "removed", "merges", "homophones", "sil_loops", "slot_ties",
                                                             "end_dropped", "eos_moves")}
    facts["end_changed_best"] = sum(d.end_changed_best for d in diags)
    assert facts["removed"] > 0 and (out[1] >= 0).any(), (name, facts)
    assert facts["merges"] > 0 or W < 2, (name, facts)
    assert facts["homophones"] > 0 or not (homo or crowd), (name, facts)
    assert facts["slot_ties"] > 0 or not (homo or crowd), (name, facts)
    assert facts["sil_loops"] > 0 or sil is None, (name, facts)
    assert facts["end_changed_best"] > 0 or name == "w1_k1", (name, facts)
    if crowd:
        assert trie.dropped == crowd + 1 - XR.MAX_WORDS and any(len(u.words) == XR.MAX_WORDS for _, u in trie.nodes())
    return x, trie, tb, out, facts


@pytest.mark.parametrize("name", list(X2_CASES))
def test_x2_bitwise_against_the_float32_restatement(name):
    B, T, N, frames, W, K, thr, M, Lmax, maxw, _, _, _, lmw, wsc, eos_score, _ = X2_CASES[name]
    x, trie, tb, (lab, ln, sc, lms, wd, wc, diags), facts = _x2_reference(name)
    print("X2", name, facts, "hypotheses", int((ln >= 0).sum()), "longest", int(ln.max()), "most words", int(wc.max()))
    if name == "n30_silence_short_rows":
        assert ln.max() > Lmax and wc.max() > maxw                   # hypotheses longer than the label and the word rows
        assert any(trie.sil in lab[b, m, :Lmax] for b in range(B) for m in range(M))
    if name == "n30_nothing_at_the_root":
        assert (ln[0] == -1).all() and (wc[0] == -1).all() and np.isinf(sc[0]).all() and (ln[1] >= 0).any()
    if name == "n30_seven_homophones":
        crowd = [w for w, _ in trie.rows[-6:]]                       # with word 0 seven words on one spelling: the last is dropped
        assert not (wd == crowd[-1]).any() and np.isin(wd, crowd[:-1]).any()
    glab, gln, gsc, glms, gwd, gwc = _search_lex(x, frames, W, K, thr, False, False, M, Lmax, maxw, _lex_table(trie), _lm_table(tb),
                                                 lmw, wsc, eos_score)
    assert sc.dtype == F32 and lms.dtype == F32
    assert (gln == ln).all() and (gwc == wc).all()
    assert (glab == lab).all() and (gwd == wd).all()
    assert (gsc.view(np.int32) == sc.view(np.int32)).all()
    assert (glms.view(np.int32) == lms.view(np.int32)).all()


# ---- X3: a lexicon of one-token words is w2l_ctc_beam_search_lm ----------------------------------------------------------------

@pytest.mark.parametrize("B,T,N,W,K,thr,log_add", [(2, 24, 9998, 64, 64, INF, False), (3, 30, 30, 8, 5, 6.0, True),
                                                    (2, 20, 9998, 16, 8, INF, True), (2, 24, 9998, 64, 64, INF, True)])
def test_x3_one_token_words_are_the_token_lm_search(B, T, N, W, K, thr, log_add):
    """every token a one-token word whose id is its class, no silence token, wordSmear = NULL, the same LM: the token-LM search with
    classScore filled with wordScore.  The smear terms are lmWeight * 0: scores are equal as values"""
    from wav2letter_amd import Lexicon
    rng = np.random.default_rng(N + T)
    x = rng.normal(0, 2, size=(B, T, N)).astype(F32) if log_add else _ints(rng, B, T, N)
    frames = [T, T // 3, 1][:B]
    tb = LR.random_lm(rng, N - 1, 3, 500, hot=min(N - 1, 300))
    lm = _lm_table(tb)
    lex = Lexicon.from_spellings([(c, [c]) for c in range(N - 1)], N - 1, N - 1)
    M, wsc = min(W, 8), 0.375
    lab, ln, sc, lms = _search_lm(x, frames, W, K, thr, log_add, log_add, M, T, lm, 0.75, np.full(N - 1, wsc, F32), -0.25)
    glab, gln, gsc, glms, gwd, gwc = _search_lex(x, frames, W, K, thr, log_add, log_add, M, T, T, lex, lm, 0.75, wsc, -0.25)
    assert (gln == ln).all() and (glab == lab).all() and (gwd == lab).all() and (gwc == ln).all()
    assert (gsc == sc).all()
    assert (glms.view(np.int32) == lms.view(np.int32)).all()
    assert (ln >= 0).any() and ln.max() > 1


# ---- X4: the log-sum search with the beam binding ------------------------------------------------------------------------------

X4_CASES = [  # (T, N, W, K, scale, hot, seeds): seeds whose every decision gap and final gap is >= 10 delta (asserted, never skipped)
    (12, 32, 4, 3, 2.0, 8, (0, 2)),
    (16, 9998, 4, 3, 3.0, 8, (2, 3)),
    (12, 6, 3, 2, 2.0, 5, (0, 2)),
]


def _x4_inputs(T, N, W, K, scale, hot, seeds):
    rng = np.random.default_rng(T * N)
    nwords = 60
    rows = XR.random_lexicon(rng, N - 1, nwords, 3, 0.1, hot - 1 if N > 6 else None, hot)
    tb = LR.random_lm(rng, nwords, 3, 200)
    trie = XR.TextbookTrie(rows, N - 1, nwords, _smear(tb, nwords), hot - 1 if N > 6 else None)
    x = np.stack([np.random.default_rng(s).normal(0, scale, size=(T, N)) for s in seeds]).astype(F32)
    x[:, :, :hot] += 3 * scale                                       # the frame tokens are among the lexicon's letters
    x[:, :, N - 1] += 3 * scale
    return x, trie, tb, XR.beam_search_lex(x, None, W, K, trie, tb, 0.8, 0.3, -0.3, INF, True, True, W, T, T, np.float64)


@pytest.mark.parametrize("T,N,W,K,scale,hot,seeds", X4_CASES)
def test_x4_log_sum_search_small_beams(T, N, W, K, scale, hot, seeds):
    x, trie, tb, (lab, ln, sc, lms, wd, wc, diags) = _x4_inputs(T, N, W, K, scale, hot, seeds)
    for dg in diags:
        dl = XR.delta_lex(T, dg.S)
        print("X4", (T, N, W, K), "S", dg.S, "delta", dl, "decision gap", dg.decision_gap(), "final gap", min(dg.final_gaps + [np.inf]),
              "blocked", dg.blocked, "merges", dg.merges, "dropped at the end", dg.end_dropped)
        assert dg.decision_gap() >= 10 * dl and min(dg.final_gaps + [np.inf]) >= 10 * dl
        assert dg.beam_gap < np.inf and dg.blocked > 0                # the beam binds and the lexicon constrains
    assert (wc > 0).any()
    glab, gln, gsc, glms, gwd, gwc = _search_lex(x, None, W, K, INF, True, True, W, T, T, _lex_table(trie), _lm_table(tb), 0.8, 0.3, -0.3)
    print("X4 max |score diff|", np.abs(gsc[ln >= 0] - sc[ln >= 0]).max())
    assert (gln == ln).all() and (glab == lab).all() and (gwc == wc).all() and (gwd == wd).all()
    assert _close(gsc[ln >= 0], sc[ln >= 0]).all() and np.isinf(gsc[ln < 0]).all()
    assert (glms.view(np.int32) == lms.view(np.int32)).all()


# ---- surfaces ---------------------------------------------------------------------------------------------------------------

def test_python_front_end_equals_the_c_abi():
    from wav2letter_amd import CTCLoss, criterion
    B, T, N, nwords = 3, 30, 40, 200
    rng = np.random.default_rng(5)
    x = rng.normal(0, 2, size=(B, T, N)).astype(F32)
    x[:, :, :10] += 4
    frames = np.array([30, 11, 1], np.int32)
    tb = LR.random_lm(rng, nwords, 3, 300)
    lm = _lm_table(tb)
    trie = XR.TextbookTrie(XR.random_lexicon(rng, N - 1, nwords, 3, 0.1, 9, 10), N - 1, nwords, _smear(tb, nwords), 9)
    lex = _lex_table(trie)
    xd, fd = torch.tensor(x, device="cuda"), torch.tensor(frames, device="cuda")
    for log_add, norm, thr, M, maxw in ((True, True, INF, 4, 5), (False, False, 6.0, 1, None)):
        want = _search_lex(x, frames, 8, 5, thr, log_add, norm, M, T, maxw or T, lex, lm, 0.6, 0.4, -0.2)
        assert (want[5] > 0).any()
        for got in (criterion.ctc_beam_search(xd, fd, beam=8, beam_token=5, threshold=thr, log_add=log_add, nbest=M, lm=lm,
                                              lm_weight=0.6, lexicon=lex, word_score=0.4, eos_score=-0.2, max_words=maxw),
                    CTCLoss().beamSearch(xd, fd, beam=8, beam_token=5, threshold=thr, log_add=log_add, normalize=norm, nbest=M,
                                         lm=lm, lm_weight=0.6, lexicon=lex, word_score=0.4, eos_score=-0.2, max_words=maxw)):
            assert len(got) == 6 and got[4].dtype == torch.int32 and got[5].dtype == torch.int32
            assert all((g.cpu().numpy().view(np.int32) == w.view(np.int32)).all() for g, w in zip(got, want))
        from wav2letter_amd import text
        ids = want[4][0, 0, :max(want[5][0, 0], 0)]
        assert text.word_ids_to_words(ids, lex.words) == [lex.words[i] for i in ids]


def test_three_surfaces_agree(tmp_path):
    """C ABI == Python CTCLoss.beamSearch(lexicon=) == compiled C++ CTCLoss::beamSearch with BeamSearchOptions::lexicon
    (tests/cpp/decode_lex_caller.cpp, plain g++ against libw2l_hip.so), all three on a lexicon read from the same file and a word
    LM read from the same ARPA file"""
    import os
    import subprocess
    from tests.test_ctc_beam_lm_host import _arpa_text
    from wav2letter_amd import CTCLoss, Lexicon, NGramLM
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = str(tmp_path / "decode_lex_caller"), os.path.join(root, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "decode_lex_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    rng = np.random.default_rng(8)
    N, nwords, hot = 30, 120, 8
    tokens = [f"t{c}" for c in range(N - 1)]
    rows = XR.random_lexicon(rng, N - 1, nwords, 3, 0.1, hot - 1, hot)
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n")
    (tmp_path / "lex.txt").write_text("".join(f"word{w:03d} " + " ".join(tokens[t] for t in sp) + "\n" for w, sp in rows))
    plain = Lexicon.from_file(tmp_path / "lex.txt", tokens, smearing="none", sil=tokens[hot - 1])
    assert plain.words == [f"word{w:03d}" for w in range(nwords)]
    (tmp_path / "lm.arpa").write_text(_arpa_text(LR.random_lm(rng, nwords, 3, 200), plain.words, unk10=-3.0)[0])
    lm = NGramLM.from_arpa(tmp_path / "lm.arpa", plain.words)
    lex = Lexicon.from_file(tmp_path / "lex.txt", tokens, lm=lm, sil=tokens[hot - 1])
    for B, T, W, K, M, Lmax, maxw, log_add, norm, thr in [(4, 31, 8, 5, 3, 31, 31, 1, 1, INF), (2, 20, 64, 64, 16, 6, 2, 0, 0, 4.0)]:
        x = rng.normal(0, 2, size=(B, T, N)).astype(F32) if log_add else _ints(rng, B, T, N)
        x[:, :, :hot] += 4
        x[:, :, N - 1] += 4
        frames = rng.integers(1, T + 1, B).astype(np.int32)
        frames[1] = 1
        lmw, wsc, eos_score = 0.75, 0.5, -0.25
        want_f = _search_lex(x, frames, W, K, thr, log_add, norm, M, Lmax, maxw, lex, lm, lmw, wsc, eos_score)
        want = _search_lex(x, None, W, K, thr, log_add, norm, M, Lmax, maxw, lex, lm, lmw, wsc, eos_score)
        assert (want[5] > 0).any()
        xd = torch.tensor(x, device="cuda")
        opts = dict(beam=W, beam_token=K, threshold=thr, log_add=bool(log_add), normalize=bool(norm), nbest=M, max_len=Lmax, lm=lm,
                    lm_weight=lmw, lexicon=lex, word_score=wsc, eos_score=eos_score, max_words=maxw)
        for got, ref in ((CTCLoss().beamSearch(xd, torch.tensor(frames, device="cuda"), **opts), want_f),
                         (CTCLoss().beamSearch(xd, **opts), want)):
            assert all((g.cpu().numpy().view(np.int32) == r.view(np.int32)).all() for g, r in zip(got, ref))
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([N, T, B, W, K, M, Lmax, maxw, log_add, norm], np.int32).tobytes()
                    + np.array([thr, lmw, wsc, eos_score], F32).tobytes() + x.tobytes() + frames.tobytes())
        run = subprocess.run([exe, inp, outp, str(tmp_path / "tokens.txt"), str(tmp_path / "lex.txt"), str(tmp_path / "lm.arpa"),
                              tokens[hot - 1]], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "decode lex caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
        got = np.fromfile(outp, np.int32)
        sizes = [B * M * Lmax, B * M, B * M, B * M, B * M * maxw, B * M]
        at = 0
        for ref in (want_f, want):
            for r, n in zip(ref, sizes):
                assert (got[at:at + n] == r.view(np.int32).ravel()).all()
                at += n
        assert at == len(got)


# ---- Decode --uselexicon=true --decodertype=wrd end to end, on the six-WAV fixture of tests/list_fixture.py ----------------

import subprocess  # noqa: E402

from tests.list_fixture import ENV, LETTERS, UTTS  # noqa: E402
from tests.test_gpu_ctc_beam import DECODE_EXE, trained  # noqa: E402,F401  (the module-scoped trained checkpoint)

LEX_WORDS = [("hello", "hello"), ("aaa", "aaa"), ("bee", "bee"), ("zoo", "zoo"), ("add", "add"), ("be", "bee"), ("Bee", "bee"), ("a", "a"),
             ("ad", "ad"), ("he", "he"), ("lo", "lo"), ("o", "o"), ("z", "z"), ("e", "e"), ("l", "l"), ("d", "d"), ("b", "b"), ("oo", "oo")]
LEX_BARE = ["a", "b", "d", "e", "h", "l", "o", "z"]      # and these letters as words spelled WITHOUT the separator: `A a`, `B b`, ...


def _lexicon_files(tmp_path):
    from tests.test_ctc_beam_lm_host import _arpa_text
    (tmp_path / "lex.txt").write_text("".join(f"{w}\t{' '.join(sp)} |\n" for w, sp in LEX_WORDS) + "".join(f"{c.upper()} {c}\n" for c in LEX_BARE))
    words = sorted([w for w, _ in LEX_WORDS] + [c.upper() for c in LEX_BARE], key=lambda w: w.encode())
    tb = LR.random_lm(np.random.default_rng(2), len(words), 3, 80)
    (tmp_path / "words.arpa").write_text(_arpa_text(tb, words, unk10=-3.0)[0])
    return tmp_path / "lex.txt", tmp_path / "words.arpa", words


def test_decode_tool_with_lexicon_end_to_end(trained, tmp_path):
    """.hyp words come from the lexicon only; the beam dump carries lmScore and score = amScore + lmweight * lmScore + wordscore *
    words + eosscore; every row equals the Python front end (Lexicon.from_file, NGramLM.from_arpa over its words,
    CTCLoss.beamSearch(lexicon=)) on the emissions of the same model over the features Decode dumped"""
    from wav2letter_amd import CTCLoss, Lexicon, NGramLM, checkpoint, text
    from wav2letter_amd.trainer import Trainer
    d, model = trained
    lex_path, arpa, words = _lexicon_files(tmp_path)
    lmw, wsc, eos = 0.5, 6.0, -0.5                                      # a word score that makes the short-trained model's letters words
    base = [DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}", "--beamsize=16",
            "--beamthreshold=100", "--uselexicon=true", "--decodertype=wrd", f"--lexicon={lex_path}", f"--lm={arpa}", f"--lmweight={lmw}",
            f"--wordscore={wsc}", f"--eosscore={eos}", "--smearing=max"]
    res = subprocess.run(base + ["--isbeamdump=true", "--nbest=3", f"--w2l_dump_features={d / 'xfeat'}"], capture_output=True, text=True,
                         timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "--lexicon: 26 words" in res.stderr and "silence token |" in res.stderr
    rows = [line.split(" | ") for line in (d / "out" / "other.hyp").read_text().splitlines()]
    assert rows and all(len(r) == 6 for r in rows)
    for r in rows:
        score, am, lms = float(r[1]), float(r[2]), float(r[3])
        hyp = r[5].split()
        assert set(hyp) <= set(words)
        assert lms < 0 and abs(score - (am + lmw * lms + wsc * len(hyp) + eos)) <= 1e-4 * max(1.0, abs(score))
    assert any(r[5].split() for r in rows)

    lm = NGramLM.from_arpa(arpa, words)
    lex = Lexicon.from_file(lex_path, LETTERS, lm=lm, sil="|")
    assert lex.words == words
    dic = text.create_token_dict(LETTERS, "ctc")
    arch = (d / "arch" / "net.arch").read_text()
    N = dic.index_size()
    want = []
    for k in range(3):                                                  # batches of 2, 2, 1 in list order
        utts = UTTS[2 * k:2 * k + 2][:5 - 2 * k]
        raw = (d / f"xfeat.{k + 1}").read_bytes()
        B, nfeat, T = (int(v) for v in np.frombuffer(raw[:12], np.int32))
        x = torch.tensor(np.frombuffer(raw[12:], np.float32).reshape(B, nfeat, T).copy()).cuda()
        tr_ = Trainer(arch, nfeat, N, "ctc", 4, 0.0)
        checkpoint.load(str(model), tr_, arch)
        tr_.plan(B, T, 8)
        tr_.to_device()
        em = tr_.forward(x, train=False).clone()
        Tout = em.shape[1]
        frames = [min(max(-(-min(1 + (n - 400) // 160, T) * Tout // T), 1), Tout) for n, _ in utts]
        out = CTCLoss().beamSearch(em, torch.tensor(frames, dtype=torch.int32, device="cuda"), beam=16, beam_token=64, threshold=100.0,
                                   log_add=False, normalize=False, nbest=3, lm=lm, lm_weight=lmw, lexicon=lex, word_score=wsc, eos_score=eos)
        _, _, sc, lms, wd, wc = (t.cpu().numpy() for t in out)
        for b in range(B):
            for m in range(3):
                if wc[b, m] >= 0:
                    want.append((f"u{2 * k + b}", f"{float(sc[b, m]):.6f}", f"{float(lms[b, m]):.6f}",
                                 " ".join(text.word_ids_to_words(wd[b, m], lex.words))))
    assert [(r[0], r[1], r[3], r[5]) for r in rows] == want

    res = subprocess.run(base, capture_output=True, text=True, timeout=600, env=ENV)     # the sclite files: one line per sample
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    hyp = [line for line in (d / "out" / "other.hyp").read_text().splitlines()]
    assert len(hyp) == 5 and all(line.endswith(f"(u{k})") for k, line in enumerate(hyp))
    first = {}
    for r in rows:
        first.setdefault(r[0], r[5])
    assert [line.rsplit(" (", 1)[0] for line in hyp] == [first.get(f"u{k}", "") for k in range(5)]
    assert "-- WER: " in res.stdout


@pytest.mark.parametrize("flags,name", [
    (["--uselexicon=true", "--lexicon="], "--uselexicon"),
    (["--uselexicon=true", "--lexicon=LEX", "--decodertype=wrd"], "--uselexicon"),
    (["--decodertype=wrd", "--lexicon=LEX", "--lm=ARPA"], "--decodertype"),
    (["--uselexicon=true", "--lexicon=LEX", "--lm=ARPA", "--decodertype=tkn"], "--decodertype=tkn"),
    (["--uselexicon=true", "--lexicon=LEX", "--lm=ARPA", "--decodertype=wrd", "--smearing=logadd"], "--smearing=logadd"),
    (["--uselexicon=true", "--lexicon=LEX", "--lm=ARPA", "--decodertype=wrd", "--unkscore=-5"], "--unkscore"),
    (["--uselexicon=true", "--lexicon=LEX", "--lm=ARPA", "--decodertype=wrd", "--silscore=0.5"], "--silscore"),
    (["--uselexicon=true", "--lexicon=BAD", "--lm=ARPA", "--decodertype=wrd"], "`box`"),
])
def test_decode_tool_lexicon_refusals(trained, tmp_path, flags, name):
    d, model = trained
    lex_path, arpa, _ = _lexicon_files(tmp_path)
    (tmp_path / "bad.txt").write_text("bee b e e |\nbox b o 7 |\n")
    flags = [f.replace("LEX", str(lex_path)).replace("ARPA", str(arpa)).replace("BAD", str(tmp_path / "bad.txt")) for f in flags]
    res = subprocess.run([DECODE_EXE, f"--am={model}", "--test=sub/other.lst"] + flags, capture_output=True, text=True, timeout=120, env=ENV)
    assert res.returncode != 0 and name in res.stderr, (res.returncode, res.stderr)
