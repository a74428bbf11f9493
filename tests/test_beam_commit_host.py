"""Host tests of w2l_beam_session_commit (csrc/criterion_beam_commit.hpp): the scratch arithmetic, every refusal with its message
(all before any device call: the library loads without a GPU), the unchanged maxFrames rule of a slot that never committed, and
the proof on the CPU -- by the numpy restatement of the commit rule in tests/beam_commit_ref.py -- that the inputs of
test_gpu_beam_commit.py let the commits keep up: (a) the committed total reaches 3/4 of the final best row, (b) the table a
commit leaves never costs a slot the frames of its next two steps.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import beam_commit_ref as CR
from tests import beam_stream_cases as BC
from wav2letter_amd import _lib

OK, EINVAL = _lib.W2L_OK, _lib.W2L_EINVAL
FAKE = 0x10000     # a non-null, 256-byte aligned pointer: no test here reaches the device


def desc(**kw):
    d = dict(slots=3, maxChunk=3, maxFrames=8, N=12, beam=4, beamToken=4, threshold=float("inf"), logAdd=0, normalize=0, variant=0)
    d.update(kw)
    return _lib.BeamSessionDesc(**d)


def create(wide=False, **kw):
    h = C.c_void_p(0)
    fn = _lib.lib().w2l_beam_session_create_wide if wide else _lib.lib().w2l_beam_session_create
    assert fn(C.byref(desc(**kw)), C.byref(h)) == OK
    return h


def err():
    return _lib.lib().w2l_host_last_error().decode()


def _documented_bytes(S, Fmax, W, wide):
    def au(n):
        return (n + 255) // 256 * 256
    cap = 64
    while cap < 2 * Fmax * W:
        cap *= 2
    return au(4 * S * 4) + au(cap * 8) + au(Fmax * (W if wide else 64) * 4)


def test_the_new_entry_points_are_declared_and_exported():
    names = {"w2l_beam_session_commit_bytes", "w2l_beam_session_commit", "w2l_beam_session_committed"}
    assert names <= set(_lib.exported_symbols())
    for n in names:
        assert hasattr(_lib.lib(), n)


def test_commit_bytes_is_the_documented_arithmetic_and_leaves_the_state_sizes_alone():
    L = _lib.lib()
    assert L.w2l_beam_session_commit_bytes(None) == 0
    for S, Fmax, W, wide in [(3, 8, 4, False), (1, 1, 1, False), (64, 4096, 64, False), (3, 8, 65, True), (2, 48, 128, True),
                             (1, 4096, 1024, True), (16, 100, 64, True)]:
        h = create(wide, slots=S, maxFrames=Fmax, beam=W)
        try:
            assert L.w2l_beam_session_commit_bytes(h) == _documented_bytes(S, Fmax, W, wide), (S, Fmax, W, wide)
        finally:
            L.w2l_beam_session_destroy(h)
    # the figure the header quotes: beam 1024, maxFrames 4096 is a 64 MiB table and a 16 MiB stack
    assert _documented_bytes(1, 4096, 1024, True) == 256 + (64 << 20) + (16 << 20)
    # W = 4, maxFrames = 8: the smallest table, 64 edges
    assert _documented_bytes(3, 8, 4, False) == 256 + 64 * 8 + 8 * 64 * 4
    # the state buffers are what they were (test_beam_stream_host.py / test_beam_stream_wide_host.py pin their arithmetic)
    assert L.w2l_beam_session_state_bytes(C.byref(desc())) > 0 and L.w2l_beam_session_wide_state_bytes(C.byref(desc(beam=65))) > 0


@pytest.mark.parametrize("wide", [False, True])
def test_every_refusal_comes_before_any_device_call(wide):
    L = _lib.lib()
    n = np.zeros(3, np.int32)
    for variant in (dict(), dict(variant=2, lm=0x1000, lmHasEos=1, lmWeight=0.5, lexicon=0x1000, wordScore=0.25)):
        lex = bool(variant)
        h = create(wide, **variant)
        need = L.w2l_beam_session_commit_bytes(h)
        words = FAKE if lex else None

        def commit(scratch=FAKE, nbytes=need, max_len=8, labels=FAKE, max_words=8, words=words, nl=n.ctypes.data, session=h):
            return L.w2l_beam_session_commit(session, None, scratch, nbytes, max_len, labels, max_words, words, nl, None, None, None)

        try:
            assert commit(session=None) == EINVAL and "null session" in err()
            assert commit(scratch=None) == EINVAL and "scratch" in err() and "aligned" in err()
            assert commit(scratch=FAKE + 16) == EINVAL and "aligned" in err()
            assert commit(nbytes=need - 1) == EINVAL and "smaller than w2l_beam_session_commit_bytes" in err() and str(need) in err()
            assert commit(max_len=0) == EINVAL and "maxLen < 1" in err()
            assert commit(labels=None) == EINVAL and "null labels" in err()
            assert commit(nl=None) == EINVAL and "null h_nLabels" in err()
            if lex:
                assert commit(words=None) == EINVAL and "lexicon variant writes words" in err()
                assert commit(max_words=0) == EINVAL and "maxWords >= 1" in err()
            else:
                assert commit(words=None, max_words=0) == EINVAL and "bind" in err()     # words are the lexicon variant's alone
            # every argument in order: the call comes before bind
            assert commit() == EINVAL and "no state bound" in err() and "w2l_beam_session_bind" in err()
            a, b = C.c_int(-1), C.c_int(-1)
            assert L.w2l_beam_session_committed(h, 0, C.byref(a), C.byref(b)) == OK and (a.value, b.value) == (0, 0)
            assert L.w2l_beam_session_committed(h, 2, None, None) == OK
            assert L.w2l_beam_session_committed(h, 3, C.byref(a), C.byref(b)) == EINVAL and "no such slot" in err()
            assert L.w2l_beam_session_committed(h, -1, C.byref(a), C.byref(b)) == EINVAL
            assert L.w2l_beam_session_committed(None, 0, C.byref(a), C.byref(b)) == EINVAL
        finally:
            L.w2l_beam_session_destroy(h)


@pytest.mark.parametrize("wide", [False, True])
def test_a_slot_that_never_committed_keeps_the_max_frames_rule_and_its_message(wide):
    L = _lib.lib()
    h = create(wide)
    try:
        def counts(n, start=None):
            n = np.asarray(n, np.int32)
            s = np.asarray(start, np.int32) if start is not None else None
            return L.w2l_beam_session_counts(h, n.ctypes.data, s.ctypes.data if s is not None else None)

        assert counts([3, 3, 0], [1, 1, 0]) == OK and counts([3, 2, 0]) == OK and counts([2, 3, 0]) == OK
        assert counts([1, 0, 0]) == EINVAL
        assert err() == "beam session step: slot 0 would pass maxFrames = 8 (8 fed, 1 given)"
        assert counts([0, 1, 0]) == EINVAL and err() == "beam session step: slot 1 would pass maxFrames = 8 (8 fed, 1 given)"
        f = C.c_int(0)
        assert L.w2l_beam_session_frames(h, 0, C.byref(f)) == OK and f.value == 8
        assert counts([3, 0, 0], [1, 0, 0]) == OK           # a start takes the count, and the budget, back to 0
        assert L.w2l_beam_session_reset(h, 1) == OK and counts([0, 1, 0]) == EINVAL and "started" in err()
    finally:
        L.w2l_beam_session_destroy(h)


# ---- the rule, restated ------------------------------------------------------------------------------------------------------
def test_the_restated_rule_on_hand_made_beams():
    assert CR.lcp([]) == 0 and CR.commit_len([]) == 0 and CR.commit_len([()]) == 0
    assert CR.commit_len([(1,)]) == 0 and CR.commit_len([(1, 2, 3)]) == 2            # one entry: all but its last label
    assert CR.commit_len([(1, 2), (1, 2, 3)]) == 1                                     # "a" and "ab": C is an entry itself
    assert CR.commit_len([(1, 2, 3), (1, 2, 4), (1, 2)]) == 1 and CR.commit_len([(1, 2, 3), (2,)]) == 0
    assert CR.split((1, 2, 3), 2) == ((1, 2), (3,))
    assert CR.live_nodes([(1, 2), (1, 2, 3)], 1) == 2 and CR.live_nodes([(1, 2, 3), (1, 2, 4)], 1) == 3
    assert CR.live_nodes([()], 0) == 0 and CR.live_nodes([(5,), (6,)], 0) == 2
    assert CR.budget(0, 4, 8) == 8 and CR.budget(1, 4, 8) == 7 and CR.budget(9, 4, 8) == 5 and CR.budget(32, 4, 8) == 0


def _search(variant, N):
    if variant == "plain":
        return {}
    cls = (np.random.default_rng(N).integers(-8, 9, N - 1) / 8).astype(np.float32)      # test_gpu_beam_commit.tables' class scores
    return dict(lm=BC.token_lm(N), lm_weight=0.5, class_score=cls, eos_score=-0.25)


def _feeds(N):
    """per life of a slot in the GPU tests' schedule: (utterance, [(frames, commit after the step)])"""
    lives, open_ = [], {}
    for em, n, st, reset, commit, fed in CR.schedule(N):
        for s in reset:
            lives.append(open_.pop(s))
        for s in range(3):
            if st[s]:
                if s in open_:
                    lives.append(open_.pop(s))
                open_[s] = (fed[s][0], [])
            if s in open_:
                open_[s][1].append((int(n[s]), commit))
    return lives + list(open_.values())


def test_the_schedule_is_what_the_gpu_tests_say_it_is():
    for N in (6, 12):
        steps = CR.schedule(N)
        chunks = {int(c) for _, n, _, _, _, _ in steps for c in n}
        assert chunks == {0, 1, 2, 3}
        assert all(not st[2] and n[2] == 0 for _, n, st, _, _, _ in steps)                   # slot 2 never starts
        assert steps[CR.LATE][2][0] == 1 and not any(s[2][0] for s in steps[:CR.LATE])        # slot 0 starts late
        assert steps[CR.RESET_AT][3] == [1] and steps[CR.AGAIN][2][1] == 1                    # slot 1 is reset mid-way, starts anew
        assert steps[-1][5][0] == (0, CR.T) and steps[-1][5][1] == (2, CR.T)                  # both utterances are fed whole
        assert CR.T == 5 * CR.MAX_FRAMES_B
        lives = _feeds(N)
        assert len(lives) == 3 and sorted(sum(n for n, _ in f) for _, f in lives)[-2:] == [CR.T, CR.T]
        for x in CR.utterances(N):
            assert x.shape == (CR.T, N) and (x * 8 == np.round(x * 8)).all() and np.abs(x).max() < 2 ** 16


@pytest.mark.parametrize("N", [6, 12])
def test_the_lexicon_variants_utterances_have_one_reading(N):
    """the classes on top of the lexicon variant's emissions, collapsed as CTC collapses them, spell words of the lexicon in exactly
    one way at the last word boundary inside the 40 frames -- no pair of hypotheses differs by LM terms alone, which no ramp scales"""
    trie, _ = BC.lexicon_and_word_lm(N)
    for x in CR.utterances(N, lex=True):
        assert x.shape == (CR.T, N) and (x * 8 == np.round(x * 8)).all() and np.abs(x).max() < 2 ** 16
        top = [int(c) for c in x.argmax(1)]
        labels = [c for i, c in enumerate(top) if c != N - 1 and (i == 0 or c != top[i - 1])]
        readings = [len(trie.derivations(tuple(labels[:k]))) for k in range(len(labels), 0, -1)]
        assert 1 in readings and max(readings[:readings.index(1) + 1]) <= 1, readings
        assert readings.index(1) <= 3                         # the 40 frames end inside a word of at most 3 tokens
    assert CR.schedule(N, lex=True)[-1][5][0] == (0, CR.T)


@pytest.mark.parametrize("N", [6, 12])
@pytest.mark.parametrize("variant", ["plain", "lm"])
def test_condition_a_the_commits_reach_three_quarters_of_the_best_row(variant, N):
    """the budget test's shape (W = K = 4, maxFrames = 8), both of its variants, over the full 40 frames"""
    W = K = 4
    search = _search(variant, N)
    for u, feed in _feeds(N):
        F = sum(n for n, _ in feed)
        if F < CR.T:
            continue
        x = CR.utterances(N)[u]
        out = CR.simulate(x, feed + [(0, True)], W, K, CR.MAX_FRAMES_B, **search)
        best = CR.live_prefixes(x, F, W, K, **search)[0]
        print(variant, N, "utterance", u, "best row", len(best), "committed", out[-1]["done"])
        assert not any(o["refused"] for o in out)
        assert 4 * out[-1]["done"] >= 3 * len(best) and out[-1]["done"] > CR.MAX_FRAMES_B


@pytest.mark.parametrize("N", [6, 12])
@pytest.mark.parametrize("variant", ["plain", "lm"])
@pytest.mark.parametrize("W,K", [(4, 4), (64, 5), (65, 5), (128, 5)])
def test_condition_b_every_commit_leaves_room_for_the_steps_before_the_next(variant, N, W, K):
    """maxFrames = 8 against 40 frames: after every scheduled commit the budget covers the next two steps (3 frames at most, one
    chunk of MAX_CHUNK), so no step of the long run is refused for its budget; without commits the same feed is refused"""
    search = _search(variant, N)
    K = min(K, N - 1)
    for u, feed in _feeds(N):
        x = CR.utterances(N)[u]
        out = CR.simulate(x, feed, W, K, CR.MAX_FRAMES_B, **search)
        assert not any(o["refused"] for o in out), (u, [o for o in out if o["refused"]][:1])
        for o in out:
            if o["live"] is not None:
                assert CR.budget(o["live"], W, CR.MAX_FRAMES_B) >= CR.MAX_CHUNK
        if sum(n for n, _ in feed) > CR.MAX_FRAMES_B:
            never = CR.simulate(x, [(n, False) for n, _ in feed], W, K, CR.MAX_FRAMES_B, **search)
            assert any(o["refused"] for o in never)
