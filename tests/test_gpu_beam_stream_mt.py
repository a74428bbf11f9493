"""GPU tests of the many-token incremental CTC beam search (wav2letter_amd/streaming.py ManyTokenStreamingDecoder,
w2l_beam_session_create_mt, csrc/criterion_beam_stream.hpp over csrc/criterion_beam_xl.hpp).  The oracle is always the
whole-utterance MANY-TOKEN entry point of the same variant on the same device -- criterion.ctc_beam_search(..., wide="mt") at B = 1
over the frames fed so far, with the same silence pair; every comparison is bit for bit (floats through .view(np.int32)).  That
the inputs hand over a full beam, merges in every mask word, a beam the threshold line cut and completed words is proved on the CPU
in test_beam_stream_mt_host.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import beam_stream_cases as BC
from tests import beam_stream_mt_cases as MC
from tests.test_gpu_beam_stream import host, same, tables
from wav2letter_amd import Lexicon, NGramLM, _lib, criterion
from wav2letter_amd.streaming import ManyTokenStreamingDecoder, StreamingDecoder, WideStreamingDecoder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, INF = np.float32, float("inf")
VARIANTS = ("plain", "lm", "lex")
N_OUT = {"plain": 3, "lm": 4, "lex": 6}


def options(variant, shape, log_add, normalize, **sil):
    _, _, _, N, W, K, thr, _ = MC.SHAPES[shape]
    return dict(beam=W, beam_token=K, threshold=thr, log_add=bool(log_add), normalize=bool(normalize), **tables(variant, N), **sil)


def extra(variant, Lmax):
    return dict(max_words=Lmax) if variant == "lex" else {}


def whole_search(x, variant, opts, M, Lmax):
    """the oracle on frames x [F][N]: the many-token whole search at B = 1, frames = None -> numpy rows [M]..."""
    xd = torch.tensor(np.ascontiguousarray(x)[None], device="cuda")
    return tuple(a[0] for a in host(criterion.ctc_beam_search(xd, nbest=M, max_len=Lmax, wide="mt", **extra(variant, Lmax), **opts)))


def empty_prefix(variant, opts, M, Lmax):
    """the contract's value for a started slot without frames: the empty prefix (with the EOS term) in row 0, empty rows below"""
    lab, ln, sc = np.full((M, Lmax), -1, np.int32), np.full(M, -1, np.int32), np.full(M, -np.inf, F32)
    lms, wd, wc = np.full(M, -np.inf, F32), np.full((M, Lmax), -1, np.int32), np.full(M, -1, np.int32)
    ln[0], sc[0], lms[0], wc[0] = 0, 0.0, 0.0, 0
    if variant != "plain":
        lm = opts["lm"]
        q = F32(lm.score(lm.start, lm.eos)[0])
        sc[0] = F32(sc[0] + F32(F32(F32(opts["lm_weight"]) * q) + F32(opts["eos_score"])))
        lms[0] = F32(lms[0] + q)
    return (lab, ln, sc, lms, wd, wc)[:N_OUT[variant]]


_WHOLE = {}


def whole(variant, shape, log_add, normalize, slot, F, M, Lmax, sil=()):
    """computed once per (case, slot, F) and shared"""
    key = (variant, shape, log_add, normalize, slot, F, M, Lmax, sil)
    if key not in _WHOLE:
        opts = options(variant, shape, log_add, normalize, **dict(sil))
        _WHOLE[key] = (empty_prefix(variant, opts, M, Lmax) if F == 0
                       else whole_search(MC.utterances(shape)[slot][:F], variant, opts, M, Lmax))
    return _WHOLE[key]


def empty_rows(got, s):
    return (got[1][s] == -1).all() and np.isneginf(got[2][s]).all() and (got[0][s] == -1).all() and all(
        (g[s] == -1).all() if g.dtype == np.int32 else np.isneginf(g[s]).all() for g in got[3:])


def run(cls, xs, variant, opts, chunkings, M, Lmax, ask=False, nan_fill=False, max_frames=None, max_chunk=None):
    """test_gpu_beam_stream_wide.run: a session of class cls over the utterances xs, slot s starting at BC.FIRST_STEP[s]"""
    T, N = xs[0].shape
    max_chunk = max_chunk or T
    dec = cls(len(xs), max_chunk, max_frames or T, N, **opts)
    ex = extra(variant, Lmax)
    asked, fed, started = [], [0] * len(xs), [False] * len(xs)
    for em, n, st in BC.schedule(xs, chunkings, max_chunk, nan_fill):
        dec.step(torch.tensor(em, device="cuda"), n, st)
        for s in range(len(xs)):
            started[s] = started[s] or bool(st[s])
            fed[s] = (0 if st[s] else fed[s]) + int(n[s])
            assert dec.frames(s) == fed[s]
        if ask:
            first, second = host(dec.result(nbest=M, max_len=Lmax, **ex)), host(dec.result(nbest=M, max_len=Lmax, **ex))
            same(first, second, "asking twice")
            asked.append((first, list(fed), list(started)))
    return host(dec.result(nbest=M, max_len=Lmax, **ex)), asked


# ---- M1: bit for bit under any chunking --------------------------------------------------------------------------------------
M1 = ([(v, s, la, nm) for s in MC.MANY for v in VARIANTS for la, nm in ((0, 0), (1, 1))]
      + [(v, "peaked_n70_w65_k65", la, nm) for v in VARIANTS for la, nm in ((0, 1), (1, 0))])


@pytest.mark.parametrize("variant,shape,log_add,normalize", M1)
def test_m1_bitwise_under_any_chunking(variant, shape, log_add, normalize):
    _, _, T, N, W, K, _, _ = MC.SHAPES[shape]
    assert K > 64                                                            # no other creator accepts the shape
    M, Lmax = W, T
    xs = MC.utterances(shape)
    opts = options(variant, shape, log_add, normalize)
    for name in BC.CHUNKINGS:
        chunkings = [BC.chunking(name, x.shape[0], seed=s) for s, x in enumerate(xs)]
        if name == "random":
            assert any(0 in c[:-1] for c in chunkings)                      # an empty chunk in mid-utterance
        got, _ = run(ManyTokenStreamingDecoder, xs, variant, opts, chunkings, M, Lmax)
        for s, x in enumerate(xs):
            same(tuple(g[s] for g in got), whole(variant, shape, log_add, normalize, s, x.shape[0], M, Lmax), (variant, shape, name, s))
            assert np.isfinite(got[2][s, 0]) or variant == "lex"             # a hypothesis exists (the lexicon may leave none)
    print("M1", variant, shape, "logAdd", log_add, "normalize", normalize, "hypotheses of slot 0", int((got[1][0] >= 0).sum()),
          "longest", int(got[1].max()))
    if variant == "plain":
        assert (got[1][0] >= 0).sum() == W                                    # the beam is full at the end (test_beam_stream_mt_host.py)


# ---- M2: partial results -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_m2_partial_results_equal_the_whole_search_on_the_prefix(variant):
    shape, log_add = "peaked_n130_w200_k129", 1
    M, Lmax = 200, 12
    xs = MC.utterances(shape)
    opts = options(variant, shape, log_add, log_add)
    chunkings = [BC.fixed(x.shape[0], 3) for x in xs]
    final, asked = run(ManyTokenStreamingDecoder, xs, variant, opts, chunkings, M, Lmax, ask=True)
    assert len(asked) >= 6
    seen_closed = seen_open = 0
    for got, fed, started in asked:
        for s in range(len(xs)):
            if not started[s]:      # never started: empty rows
                assert empty_rows(got, s)
                seen_closed += 1
                continue
            same(tuple(g[s] for g in got), whole(variant, shape, log_add, log_add, s, fed[s], M, Lmax), ("partial", s, fed[s]))
            seen_open += 1
    assert seen_closed and seen_open
    silent, _ = run(ManyTokenStreamingDecoder, xs, variant, opts, chunkings, M, Lmax)
    same(final, silent, "a run that never asked")


def test_m2_a_started_slot_without_frames_returns_the_empty_prefix():
    for variant in VARIANTS:
        shape = "peaked_n130_w200_k129"
        dec = ManyTokenStreamingDecoder(2, 4, 8, 130, **options(variant, shape, 0, 0))
        dec.step(torch.zeros(2, 4, 130, device="cuda"), [0, 0], [1, 0])
        got = host(dec.result(nbest=3, max_len=5, **extra(variant, 5)))
        same(tuple(g[0] for g in got), whole(variant, shape, 0, 0, 0, 0, 3, 5), variant)
        assert empty_rows(got, 1)
        assert got[1][0, 0] == 0 and np.isfinite(got[2][0, 0])


# ---- M3: slots ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_m3_slots_are_independent_restartable_and_read_no_row_beyond_their_count(variant):
    shape = "peaked_n130_w200_k129"
    M, Lmax = 200, 12
    xs = MC.utterances(shape)
    x = xs[0]
    T, N = x.shape
    opts = options(variant, shape, 0, 0)
    ex = extra(variant, Lmax)
    want = whole(variant, shape, 0, 0, 0, T, M, Lmax)

    # the same utterance in two slots under different chunkings, rows beyond the counts NaN; max_frames is exactly T
    dec = ManyTokenStreamingDecoder(2, 9, T, N, **opts)
    plans = [BC.fixed(T, 7), [0, 0] + BC.chunking("random", T, seed=5)]
    pos = [0, 0]
    for i in range(max(len(p) for p in plans)):
        em = np.full((2, 9, N), np.nan, F32)
        n, st = np.zeros(2, np.int32), np.zeros(2, np.int32)
        for s in range(2):
            if i < len(plans[s]):
                c = plans[s][i]
                em[s, :c] = x[pos[s]:pos[s] + c]
                pos[s] += c
                n[s], st[s] = c, i == 0
        dec.step(torch.tensor(em, device="cuda"), n, st)
    got = host(dec.result(nbest=M, max_len=Lmax, **ex))
    for s in range(2):
        same(tuple(g[s] for g in got), want, ("slot", s))
    assert np.isfinite(got[2][got[1] >= 0]).all()
    if variant != "lex":
        assert (got[1][0] >= 0).sum() == 200                                  # the beam the restart below leaves behind is full
    # an utterance of exactly max_frames was accepted; one frame more is refused and changes nothing
    assert dec.frames(0) == T
    em = np.full((2, 9, N), np.nan, F32)
    em[0, :1] = x[:1]
    with pytest.raises(ValueError, match=f"slot 0.*maxFrames = {T}"):
        dec.step(torch.tensor(em, device="cuda"), [1, 0], None)
    same(host(dec.result(nbest=M, max_len=Lmax, **ex)), got, "after the refusal")
    with pytest.raises(ValueError):
        dec.result(nbest=M + 1, max_len=Lmax, **ex)

    # slot 0, whose stored beam has 200 entries, restarted on a 1-frame utterance: nothing beyond the new n is read
    y = xs[2]
    assert y.shape[0] == 1
    em[0, :1] = y
    dec.step(torch.tensor(em, device="cuda"), [1, 0], [1, 0])
    again = host(dec.result(nbest=M, max_len=Lmax, **ex))
    same(tuple(g[0] for g in again), whole(variant, shape, 0, 0, 2, 1, M, Lmax), "restarted slot")
    same(tuple(g[1] for g in again), want, "the other slot kept its result")
    dec.reset(1)
    closed = host(dec.result(nbest=M, max_len=Lmax, **ex))
    assert empty_rows(closed, 1) and dec.frames(1) == 0
    same(tuple(g[0] for g in closed), tuple(g[0] for g in again), "a reset touches its slot alone")


@pytest.mark.parametrize("log_add", [0, 1])
def test_m3_a_beam_that_dies_stays_dead_and_its_slot_can_be_restarted(log_add):
    """test_gpu_beam_stream_wide's V5 on the many-token session: a lexicon whose every word has two tokens, a blank far below the
    threshold line, frame 4 -inf in every class: n = 0 from there on, and the half of the beam stops flipping.  Slot 0 runs in chunks
    of 3, slot 1 the same utterance in chunks of 1; after every step both equal the whole many-token search on their frames.  Then
    slot 1 starts anew and lives."""
    from tests import ctc_beam_lex_ref as XR
    from tests import ctc_beam_lm_ref as LR
    rng = np.random.default_rng(3)
    N, tokens, T, W = 12, 11, 9, 100
    x = (rng.integers(-12, 1, size=(T, N)) / 4).astype(F32)
    x[:, N - 1] = -40.0
    x[4, :] = -np.inf
    rows = [(w, [w % tokens, (w + 1) % tokens]) for w in range(tokens)]
    tb = LR.random_lm(rng, tokens, 2, 30, True, True, (), eighths=True)
    trie = XR.TextbookTrie(rows, tokens, tokens, BC.smear(tb, tokens), None)
    opts = dict(beam=W, beam_token=100, threshold=8.0, log_add=bool(log_add), normalize=False,
                lm=NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk)), lm_weight=0.5, eos_score=0.0, word_score=0.25,
                lexicon=Lexicon.from_spellings(trie.rows, trie.num_tokens, trie.num_words, trie.word_smear, trie.sil))
    M, Lmax = W, T
    dec = ManyTokenStreamingDecoder(2, 3, T, N, **opts)
    plans = [BC.fixed(T, 3), BC.fixed(T, 1)]
    pos, alive = [0, 0], [[], []]
    for i in range(T):
        em = np.zeros((2, 3, N), F32)
        n = np.zeros(2, np.int32)
        for s in range(2):
            if i < len(plans[s]):
                c = plans[s][i]
                em[s, :c] = x[pos[s]:pos[s] + c]
                pos[s] += c
                n[s] = c
        dec.step(torch.tensor(em, device="cuda"), n, [i == 0, i == 0])
        got = host(dec.result(nbest=M, max_len=Lmax, max_words=Lmax))
        for s in range(2):
            same(tuple(g[s] for g in got), whole_search(x[:pos[s]], "lex", opts, M, Lmax), ("slot", s, "frames", pos[s]))
            alive[s].append((pos[s], not empty_rows(got, s)))
    by_frames = dict(alive[1])
    assert by_frames[2] or by_frames[3] or by_frames[4]       # words were completed before the beam died
    assert not any(by_frames[f] for f in range(5, T + 1))     # dead from frame 4 on
    assert dict(alive[0])[3] and not dict(alive[0])[6] and not dict(alive[0])[9]
    em = np.zeros((2, 3, N), F32)
    em[1, :3] = x[:3]
    dec.step(torch.tensor(em, device="cuda"), [0, 3], [0, 1])
    got = host(dec.result(nbest=M, max_len=Lmax, max_words=Lmax))
    same(tuple(g[1] for g in got), whole_search(x[:3], "lex", opts, M, Lmax), "restarted after death")
    assert not empty_rows(got, 1) and empty_rows(got, 0)


# ---- M4: the silence score -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "lex"])
def test_m4_a_silence_score(variant):
    shape = "peaked_n130_w200_k129"
    _, _, T, N, W, _, _, _ = MC.SHAPES[shape]
    M, Lmax = W, T
    xs = MC.utterances(shape)
    chunkings = [BC.fixed(x.shape[0], 5) for x in xs]
    tok = int(np.argmax(xs[0][0, :N - 1]))                                   # LM-free: a class that is hot in frame 0
    if variant == "lex":
        assert tables("lex", N)["lexicon"].sil == N - 2                      # sil_token=None: the lexicon's silence token
    results = {}
    for score in (-1.0, 0.5, 0.0):
        for log_add in (0, 1):
            sil = (("sil_score", score),) if variant == "lex" else (("sil_token", tok), ("sil_score", score))   # lex: the lexicon's token
            opts = options(variant, shape, log_add, log_add, **dict(sil))
            got, _ = run(ManyTokenStreamingDecoder, xs, variant, opts, chunkings, M, Lmax)
            for s, x in enumerate(xs):
                same(tuple(g[s] for g in got), whole(variant, shape, log_add, log_add, s, x.shape[0], M, Lmax, sil), (variant, score, s))
            results[score, log_add] = got
    for log_add in (0, 1):
        bare, _ = run(ManyTokenStreamingDecoder, xs, variant, options(variant, shape, log_add, log_add), chunkings, M, Lmax)
        same(results[0.0, log_add], bare, "a silence score of 0 is no silence score")
        for score in (-1.0, 0.5) if variant == "plain" else ():                # and a real one changes the search
            assert any((a.view(np.int32) != b.view(np.int32)).any() for a, b in zip(results[score, log_add], bare))


# ---- M5: the families agree where both exist -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_m5_many_token_and_wide_sessions_return_the_same_bytes(variant):
    shape = "peaked_n30_w256_k16"
    _, _, T, N, W, _, _, _ = MC.SHAPES[shape]
    xs = MC.utterances(shape)
    chunkings = [BC.fixed(x.shape[0], 7) for x in xs]
    for log_add in (0, 1):
        opts = options(variant, shape, log_add, log_add)
        wide, asked_w = run(WideStreamingDecoder, xs, variant, opts, chunkings, W, T, ask=True)
        mt, asked_m = run(ManyTokenStreamingDecoder, xs, variant, opts, chunkings, W, T, ask=True)
        same(mt, wide, (variant, log_add))
        assert len(asked_w) == len(asked_m)
        for (gw, _, _), (gm, _, _) in zip(asked_w, asked_m):
            same(gm, gw, "partial")
        assert np.isfinite(mt[2][0, 0]) or variant == "lex"


# ---- M6: commit ------------------------------------------------------------------------------------------------------------------
def _m6(variant, every, beam=None):
    """sessions a (never commits) and b (commits after every `every`-th frame) over the first two utterances of the shape, one
    frame a step: after every step committed ++ tail == a's rows, scores the same bits, and everything committed earlier is a prefix
    of every live row of a.  Returns the labels slot 0 committed, per logAdd mode."""
    shape = "peaked_n130_w200_k129"
    _, _, T, N, W, _, _, _ = MC.SHAPES[shape]
    W = beam or W
    M, Lmax = W, T
    xs = MC.utterances(shape)[:2]
    ex = extra(variant, Lmax)
    totals = []
    for log_add in (0, 1):
        opts = dict(options(variant, shape, log_add, log_add), beam=W)
        a, b = (ManyTokenStreamingDecoder(2, 1, T, N, **opts) for _ in range(2))
        committed_then = []
        for t in range(T):
            em = np.zeros((2, 1, N), F32)
            n = np.zeros(2, np.int32)
            for s, x in enumerate(xs):
                if t < x.shape[0]:
                    em[s, 0], n[s] = x[t], 1
            for d in (a, b):
                d.step(torch.tensor(em, device="cuda"), n, [t == 0, t == 0])
            ra = host(a.result(nbest=M, max_len=Lmax, **ex))
            if (t + 1) % every == 0:
                b.commit()
                committed_then.append([b.committed(s)[0].copy() for s in range(2)])
                for s in range(2):      # maximality: max(0, LCP - 1) of ALL live rows of a (nbest = beam); the lexicon: at most that
                    rows = [ra[0][s, m, :ra[1][s, m]] for m in np.nonzero(ra[1][s] >= 0)[0]]
                    if rows:
                        lcp = 0
                        while all(len(r) > lcp and r[lcp] == rows[0][lcp] for r in rows):
                            lcp += 1
                        done = len(b.committed(s)[0])
                        assert done <= max(0, lcp - 1) and (done == max(0, lcp - 1) or variant == "lex"), (variant, t, s, done, lcp)
            rb = host(b.result(nbest=M, max_len=Lmax, full=True, **ex))
            for s in range(2):
                live = ra[1][s] >= 0
                assert (rb[1][s] == ra[1][s]).all(), (variant, every, t, s)
                n_sc = 1 if variant == "plain" else 2                          # scores, and lm_scores with an LM
                same(tuple(r[s] for r in rb[2:2 + n_sc]), tuple(r[s] for r in ra[2:2 + n_sc]), ("scores", t, s))
                for m in np.nonzero(live)[0]:
                    ln = ra[1][s, m]
                    assert (rb[0][s, m, :ln] == ra[0][s, m, :ln]).all(), ("labels", t, s, m)
                    if variant == "lex":
                        wc = ra[5][s, m]
                        assert rb[5][s, m] == wc and (rb[4][s, m, :wc] == ra[4][s, m, :wc]).all(), ("words", t, s, m)
                for then in committed_then:                                    # stability: a prefix of every later row
                    c = then[s]
                    assert all((ra[0][s, m, :len(c)] == c).all() for m in np.nonzero(live)[0])
        total = len(b.committed(0)[0])
        print("M6", variant, "beam", W, "every", every, "logAdd", log_add, "committed", total, "of", int(ra[1][0, 0]), "live", b.live)
        assert b.frames(0) == T and (b.live > 0).all()
        totals.append(total)
    return totals


@pytest.mark.parametrize("every", [2, 5])
@pytest.mark.parametrize("variant", VARIANTS)
def test_m6_committed_and_tail_equal_a_session_that_never_commits(variant, every):
    """at W = 200 over 129 tokens the beam keeps both readings of the first frames to the end: the cut is the root or its child,
    nothing is handed out, and every commit still rebuilds the table and rewrites the current half's node and parent ids, after
    which the search must go on bit for bit"""
    _m6(variant, every)


@pytest.mark.parametrize("variant", VARIANTS)
def test_m6_a_narrow_beam_over_many_tokens_commits_labels(variant):
    """the same frames at W = 4, still 129 tokens a frame (no other session takes them).  What a commit must hand out is stated
    by _m6 from the uncommitted session's rows (maximality: max(0, LCP - 1)); that this is more than nothing is a fact of the
    inputs, and it holds LM-free, where the four entries agree on their first labels.  Under the token LM (lmWeight 0.5 on a
    model in eighths, class scores) the best rows after 12 frames are two or three labels long and share at most one: nothing to
    hand out, and the test says so instead of asking for labels.  Hidden unfinished entries may hold a lexicon's cut back."""
    totals = _m6(variant, 2, beam=4)
    if variant == "plain":
        assert min(totals) > 0


def test_m6_the_budget_rule_and_its_refusal():
    shape = "peaked_n130_w200_k129"
    _, _, T, N, W, _, _, _ = MC.SHAPES[shape]
    x = MC.utterances(shape)[0]
    Fmax = 5
    dec = ManyTokenStreamingDecoder(1, 1, Fmax, N, **options("plain", shape, 0, 0))
    feed = lambda t, start=False: dec.step(torch.tensor(x[t][None, None], device="cuda"), [1], [start])  # noqa: E731
    feed(0, True)
    feed(1)
    dec.commit()
    live = int(dec.live[0])
    held = (live + W - 1) // W
    room = Fmax - held
    assert live > 0 and 1 <= room < Fmax
    for i in range(room):
        feed(2 + i)
    before = host(dec.result(nbest=W, max_len=T))
    with pytest.raises(_lib.W2LInvalidArgument, match=f"slot 0 would pass its budget of maxFrames = {Fmax}.*{live} nodes"):
        feed(2 + room)
    assert dec.frames(0) == 2 + room
    same(host(dec.result(nbest=W, max_len=T)), before, "after the refusal")
    dec.commit()                                                               # commit again: room again
    feed(2 + room)
    full = host(dec.result(nbest=W, max_len=T, full=True))
    want = whole("plain", shape, 0, 0, 0, 3 + room, W, T)
    assert (full[1][0] == want[1]).all() and (full[2][0].view(np.int32) == want[2].view(np.int32)).all()
    for m in range(W):
        assert (full[0][0, m, :want[1][m]] == want[0][m, :want[1][m]]).all()


def test_m6_commit_is_refused_above_beam_1024_and_changes_nothing():
    shape = "peaked_n110_w1500_k100"
    _, _, T, N, W, _, _, _ = MC.SHAPES[shape]
    x = MC.utterances(shape)[0]
    dec = ManyTokenStreamingDecoder(1, T, T, N, **options("plain", shape, 0, 0))
    dec.step(torch.tensor(x[None], device="cuda"), [T], [1])
    before = host(dec.result(nbest=W, max_len=T))
    same(tuple(g[0] for g in before), whole("plain", shape, 0, 0, 0, T, W, T), "before")
    with pytest.raises(_lib.W2LUnsupported, match="1024"):
        dec.commit()
    assert _lib.lib().w2l_beam_session_commit_bytes(dec.h) == 0
    same(host(dec.result(nbest=W, max_len=T)), before, "after the refused commit")
    assert dec.frames(0) == T and len(dec.committed(0)[0]) == 0


# ---- M7: surfaces ------------------------------------------------------------------------------------------------------------
def _c_abi(steps, S, Cm, Fmax, N, W, K, thr, log_add, norm, M, Lmax, lm, lmw, eos_score, sil_token, sil_score):
    """every step through the C ABI (w2l_beam_session_create_mt, then the shared entry points); the outputs after each, lmScores
    included in every variant"""
    L = _lib.lib()
    blob = lm.device_blob("cuda") if lm is not None else None
    d = _lib.BeamSessionDesc(slots=S, maxChunk=Cm, maxFrames=Fmax, N=N, beam=W, beamToken=K, threshold=thr, logAdd=log_add, normalize=norm,
                             variant=1 if lm is not None else 0, lm=blob.data_ptr() if lm is not None else None,
                             lmHasEos=int(lm.has_eos) if lm is not None else 0, lmWeight=lmw if lm is not None else 0.0,
                             eosScore=eos_score if lm is not None else 0.0)
    h = C.c_void_p(0)
    assert L.w2l_beam_session_create_mt(C.byref(d), sil_token, sil_score, C.byref(h)) == 0
    outs = []
    try:
        need = L.w2l_beam_session_mt_state_bytes(C.byref(d))
        state = torch.empty(need, dtype=torch.uint8, device="cuda")
        assert L.w2l_beam_session_bind(h, state.data_ptr(), need - 1) == 1
        assert L.w2l_beam_session_bind(h, state.data_ptr(), state.numel()) == 0
        st_ = torch.cuda.current_stream().cuda_stream
        for em, n, st in steps:
            ed = torch.tensor(em, device="cuda")
            assert L.w2l_beam_session_step(h, ed.data_ptr(), n.ctypes.data, st.ctypes.data, st_) == 0
            lab = torch.full((S, M, Lmax), -7, dtype=torch.int32, device="cuda")
            ln = torch.full((S, M), -7, dtype=torch.int32, device="cuda")
            sc, lms = torch.full((S, M), 7.0, device="cuda"), torch.full((S, M), 7.0, device="cuda")
            assert L.w2l_beam_session_result(h, M, Lmax, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), lms.data_ptr(), 0, None, None, st_) == 0
            assert L.w2l_beam_session_result(h, 0, Lmax, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), lms.data_ptr(), 0, None, None, st_) == 1
            assert L.w2l_beam_session_result(h, W + 1, Lmax, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), lms.data_ptr(), 0, None, None, st_) == 1
            assert L.w2l_beam_session_result(h, M, Lmax, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), None, 0, None, None, st_) == 1
            outs.append(host((lab, ln, sc, lms)))
    finally:
        L.w2l_beam_session_destroy(h)
    return outs


def test_m7_three_surfaces_agree(tmp_path):
    """C ABI == Python ManyTokenStreamingDecoder == compiled C++ fl::pkg::speech::ManyTokenStreamingDecoder (tests/cpp/
    beam_stream_mt_caller.cpp, built by its .mk against libw2l_hip.so) at W = 150, K = 100 with a silence score, LM-free and with a
    token LM read from one ARPA file; the C++ refusals are checked inside the caller"""
    from tests.test_ctc_beam_lm_host import _arpa_text
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "beam_stream_mt_caller.mk", "beam_stream_mt_caller", f"OUT={tmp_path}"],
                   check=True, capture_output=True)
    exe = str(tmp_path / "beam_stream_mt_caller")
    shape = "peaked_n130_w200_k129"
    xs = MC.utterances(shape)
    S, (T, N) = len(xs), xs[0].shape
    W, K, thr, M, Lmax, Cm = 150, 100, 6.0, 120, 8, 5
    sil_token, sil_score = 7, -0.5
    steps = BC.schedule(xs, [BC.fixed(x.shape[0], 5) for x in xs], Cm)
    tokens = [f"t{c}" for c in range(N - 1)]
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n")
    (tmp_path / "lm.arpa").write_text(_arpa_text(BC.token_lm(N), tokens, unk10=-3.0)[0])
    arpa_lm = NGramLM.from_arpa(tmp_path / "lm.arpa", tokens)
    for lm, log_add in ((None, 0), (arpa_lm, 0), (arpa_lm, 1)):
        lmw, eos_score = 0.75, -0.25
        want = _c_abi(steps, S, Cm, T, N, W, K, thr, log_add, log_add, M, Lmax, lm, lmw, eos_score, sil_token, sil_score)
        assert (want[-1][1][0] >= 0).sum() > 64
        if lm is None:      # the LM-free variant's lmScores: 0 for live rows, -inf for empty ones
            for lab, ln, sc, lms in want:
                assert ((lms == 0) == (ln >= 0)).all() and (np.isneginf(lms) == (ln < 0)).all()
        kw = dict(lm=lm, lm_weight=lmw, eos_score=eos_score) if lm is not None else {}
        opts = dict(beam=W, beam_token=K, threshold=thr, log_add=bool(log_add), sil_token=sil_token, sil_score=sil_score, **kw)
        n_out = 4 if lm is not None else 3
        for s, x in enumerate(xs):      # the last step's rows are the whole many-token search's
            same(tuple(a[s] for a in want[-1][:n_out]), whole_search(x, "lm" if lm is not None else "plain", opts, M, Lmax), ("oracle", s))
        dec = ManyTokenStreamingDecoder(S, Cm, T, N, **opts)
        for (em, n, st), ref in zip(steps, want):
            dec.step(torch.tensor(em, device="cuda"), n, st)
            same(host(dec.result(nbest=M, max_len=Lmax)), ref[:n_out], "python")
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([S, Cm, T, N, W, K, M, Lmax, log_add, log_add, len(steps), sil_token], np.int32).tobytes()
                    + np.array([thr, lmw, eos_score, sil_score], F32).tobytes())
            for em, n, st in steps:
                f.write(n.tobytes() + st.tobytes() + em.tobytes())
        args = [exe, inp, outp] + ([str(tmp_path / "tokens.txt"), str(tmp_path / "lm.arpa")] if lm is not None else [])
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "beam stream mt caller ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
        raw = np.fromfile(outp, np.int32)
        at = 0
        for ref in want:
            for a in ref[:n_out]:
                assert (raw[at:at + a.size] == a.view(np.int32).ravel()).all()
                at += a.size
        assert at == len(raw)
    with pytest.raises(_lib.W2LUnsupported):
        StreamingDecoder(S, Cm, T, N, beam=64, beam_token=65)
    with pytest.raises(_lib.W2LUnsupported):
        WideStreamingDecoder(S, Cm, T, N, beam=100, beam_token=65)


# ---- M8: end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "lm"])
def test_m8_streaming_session_feeds_the_many_token_decoder(variant):
    """StreamingSession on the tiny arch feeds a ManyTokenStreamingDecoder step by step (S = 2, chunks of 16 and 8 input frames,
    max_chunk = max_out), its (out, n_out) as they are: the final hypotheses equal the whole many-token search over the emissions
    the session itself produced"""
    import stream_ref as SR
    from tests.test_gpu_stream import fixed, make_trainer
    from wav2letter_amd.streaming import StreamingSession
    S, cmax, T = 2, 16, 64
    tr = make_trainer(SR.TINY_ARCH, SR.NFEAT, SR.NLABEL, 5)
    sess = StreamingSession(tr, S, cmax)
    N = SR.NLABEL
    opts = dict(beam=150, beam_token=100, threshold=INF, log_add=True, normalize=True, sil_token=0, sil_score=-0.25)
    if variant == "lm":
        tb = BC.LR.random_lm(np.random.default_rng(6), N - 1, 3, 30, True, True, (), eighths=True)
        opts.update(lm=NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk)), lm_weight=0.5, eos_score=-0.25)
    dec = ManyTokenStreamingDecoder(S, sess.max_out, T, N, **opts)
    rng = np.random.default_rng(12)
    xs = [rng.normal(size=(SR.NFEAT, 64)).astype(F32), rng.normal(size=(SR.NFEAT, 40)).astype(F32)]
    plans = [fixed(64, 16), [0] + fixed(40, 8)]
    pos, kept = [0, 0], [[], []]
    for i in range(max(len(p) for p in plans)):
        x = np.zeros((S, SR.NFEAT, cmax), F32)
        n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for s in range(S):
            if i < len(plans[s]):
                c = plans[s][i]
                x[s, :, :c] = xs[s][:, pos[s]:pos[s] + c]
                pos[s] += c
                n[s], st[s], fi[s] = c, i == 0, i == len(plans[s]) - 1
        out, n_out = sess.step(torch.tensor(x, device="cuda"), n, st, fi)
        dec.step(out, n_out, st)                                   # the session's output, as it is
        for s in range(S):
            kept[s].append(out[s, :n_out[s]].clone())
    got = host(dec.result(nbest=150, max_len=T))
    for s in range(S):
        em = torch.cat(kept[s])
        assert em.shape[0] == dec.frames(s) > 4
        want = host(criterion.ctc_beam_search(em[None], nbest=150, max_len=T, wide="mt", **opts))
        same(tuple(g[s] for g in got), tuple(w[0] for w in want), ("end to end", s))
        assert got[1][s, 0] >= 0
    assert (got[1][0] >= 0).sum() > 64
