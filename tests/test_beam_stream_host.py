"""Host tests of the incremental CTC beam search (w2l_beam_session_*, csrc/criterion_beam_stream.hpp): the refusals (all before
any device call: the library loads without a GPU), the state buffer's arithmetic, the frame bookkeeping, and the proof on the CPU
that the inputs of test_gpu_beam_stream.py put the hand-over between two steps to work.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import beam_stream_cases as BC
from tests import ctc_beam_ref as R
from wav2letter_amd import _lib, streaming

OK, EINVAL, EUNSUPPORTED = _lib.W2L_OK, _lib.W2L_EINVAL, _lib.W2L_EUNSUPPORTED
FAKE = 0x1000     # a non-null table pointer: creation looks at presence only, and no test here reaches the device


def desc(**kw):
    d = dict(slots=3, maxChunk=8, maxFrames=48, N=30, beam=16, beamToken=8, threshold=float("inf"), logAdd=0, normalize=0, variant=0)
    d.update(kw)
    return _lib.BeamSessionDesc(**d)


def create(**kw):
    h = C.c_void_p(0)
    st = _lib.lib().w2l_beam_session_create(C.byref(desc(**kw)), C.byref(h))
    return st, h


def err():
    return _lib.lib().w2l_host_last_error().decode()


LM = dict(variant=1, lm=FAKE, lmHasEos=1, lmWeight=0.5)
LEX = dict(variant=2, lm=FAKE, lmHasEos=1, lmWeight=0.5, lexicon=FAKE, wordScore=0.25)


@pytest.mark.parametrize("kw,want", [
    (dict(slots=0), EINVAL), (dict(maxChunk=0), EINVAL), (dict(maxFrames=0), EINVAL), (dict(N=1), EINVAL), (dict(beam=0), EINVAL),
    (dict(beamToken=0), EINVAL), (dict(threshold=-1.0), EINVAL), (dict(threshold=float("nan")), EINVAL),
    (dict(variant=1), EINVAL),                                              # the token-LM variant without a table
    (dict(LM, lmWeight=float("inf")), EINVAL), (dict(LM, lmHasEos=0, eosScore=1.0), EINVAL), (dict(LM, lexicon=FAKE), EINVAL),
    (dict(variant=2, lm=FAKE), EINVAL),                                     # the lexicon variant without a lexicon
    (dict(LEX, classScore=FAKE), EINVAL), (dict(LEX, wordScore=float("nan")), EINVAL),
    (dict(lm=FAKE), EINVAL), (dict(lmWeight=0.5), EINVAL),                  # the LM-free variant takes none of them
    (dict(variant=3), EUNSUPPORTED), (dict(variant=-1), EUNSUPPORTED),
    (dict(beam=65), EUNSUPPORTED), (dict(N=9998, beamToken=65), EUNSUPPORTED), (dict(LEX, beam=128), EUNSUPPORTED),
    (dict(maxFrames=1 << 26, beam=16), EUNSUPPORTED),
    (dict(), OK), (dict(beamToken=65), OK),                                 # K is clipped to N - 1 = 29 first
    (LM, OK), (LEX, OK),
])
def test_creation_follows_the_whole_searches_argument_rules(kw, want):
    L = _lib.lib()
    st, h = create(**kw)
    assert st == want, (kw, err())
    assert (L.w2l_beam_session_state_bytes(C.byref(desc(**kw))) > 0) == (want == OK)
    if want == OK:
        L.w2l_beam_session_destroy(h)
    else:
        assert not h.value and err()
    assert L.w2l_beam_session_create(None, C.byref(h)) == EINVAL


def _documented_bytes(S, C_, Fmax, N, W, Kt):
    def au(n):
        return (n + 255) // 256 * 256
    K = min(Kt, N - 1)
    cap = 64
    while cap < 2 * Fmax * W:
        cap *= 2
    rows = S * C_
    return au(3 * S * 4) + 2 * au(rows * 4) + 2 * au(rows * K * 4) + au(S * cap * 8) + au(S * 4) + 11 * au(S * 64 * 4)


def test_state_bytes_is_the_documented_arithmetic():
    L = _lib.lib()
    size = lambda **kw: L.w2l_beam_session_state_bytes(C.byref(desc(**kw)))  # noqa: E731
    for S, C_, Fmax, N, W, K in [(3, 8, 48, 30, 16, 8), (1, 1, 1, 2, 1, 1), (64, 4, 4096, 9998, 64, 64), (5, 7, 100, 30, 64, 64)]:
        assert size(slots=S, maxChunk=C_, maxFrames=Fmax, N=N, beam=W, beamToken=K) == _documented_bytes(S, C_, Fmax, N, W, K)
    base = size()
    assert size(maxFrames=4800) > base and size(beam=64) > base and size(slots=30) > base and size(maxChunk=80) > base
    # the figures DESIGN quotes: W = 64, maxFrames = 4096 is a 4 MiB table per slot (2^19 edges of 8 bytes); the beam arrays stay
    # under 3 KiB per slot
    per_slot = size(slots=2, maxFrames=4096, beam=64) - size(slots=1, maxFrames=4096, beam=64)
    assert 4 << 20 <= per_slot < (4 << 20) + (64 << 10)
    assert 11 * 64 * 4 < 3 * 1024
    assert size(**LM) == base == size(**LEX)


def test_frames_and_reset_bookkeeping_and_refused_steps_leave_the_counts():
    L = _lib.lib()
    st, h = create()
    assert st == OK
    S = 3

    def counts(n, start=None):
        n = np.asarray(n, np.int32)
        s = np.asarray(start, np.int32) if start is not None else None
        return L.w2l_beam_session_counts(h, n.ctypes.data, s.ctypes.data if s is not None else None)

    def frames():
        out = []
        for s in range(S):
            f = C.c_int(-1)
            assert L.w2l_beam_session_frames(h, s, C.byref(f)) == OK
            out.append(f.value)
        return out

    try:
        assert frames() == [0, 0, 0]
        assert counts([0, 0, 0]) == OK                                                # idle slots may idle
        assert counts([1, 0, 0]) == EINVAL and "slot 0" in err() and "started" in err()   # frames before a start
        assert counts([8, 0, 3], [1, 0, 1]) == OK and frames() == [8, 0, 3]
        assert counts([8, 0, 0]) == OK and counts([0, 5, 8], [0, 1, 0]) == OK and frames() == [16, 5, 11]
        before = frames()
        assert counts([9, 0, 0]) == EINVAL and "0..8" in err()                            # above maxChunk
        assert counts([-1, 0, 0]) == EINVAL
        assert counts([8, 8, 8, ][:3], [0, 0, 0]) == OK and frames() == [24, 13, 19]
        assert counts([8, 8, 8]) == OK and counts([8, 8, 8]) == OK and frames() == [40, 29, 35]
        before = frames()
        assert counts([8, 8, 8]) == OK and frames() == [48, 37, 43]                        # slot 0 sits exactly at maxFrames
        before = frames()
        assert counts([1, 1, 1]) == EINVAL and "slot 0" in err() and "maxFrames = 48" in err()
        assert frames() == before                                                         # a refused step moves no count, of any slot
        assert counts([0, 1, 6], [0, 0, 0]) == EINVAL and "slot 2" in err() and frames() == before
        assert counts([1, 1, 1], [1, 0, 0]) == OK and frames() == [1, 38, 44]             # a start takes the count back to 0 first
        assert L.w2l_beam_session_reset(h, 1) == OK and frames() == [1, 0, 44]
        assert counts([0, 1, 0]) == EINVAL and "slot 1" in err()                           # a reset slot is closed
        assert L.w2l_beam_session_reset(h, 3) == EINVAL and L.w2l_beam_session_reset(h, -1) == EINVAL
        f = C.c_int(0)
        assert L.w2l_beam_session_frames(h, 3, C.byref(f)) == EINVAL and L.w2l_beam_session_frames(h, 0, None) == EINVAL
        assert counts([0, 0, 0]) == OK and L.w2l_beam_session_counts(h, None, None) == EINVAL
    finally:
        L.w2l_beam_session_destroy(h)


def test_step_result_and_bind_refusals_come_before_any_device_call():
    L = _lib.lib()
    st, h = create()
    assert st == OK
    n = np.zeros(3, np.int32)
    try:
        assert L.w2l_beam_session_step(h, FAKE, n.ctypes.data, None, None) == EINVAL and "bind" in err()
        assert L.w2l_beam_session_result(h, 1, 8, FAKE, FAKE, FAKE, FAKE, 0, None, None, None) == EINVAL and "bind" in err()
        need = L.w2l_beam_session_state_bytes(C.byref(desc()))
        assert L.w2l_beam_session_bind(h, 0x10000, need - 1) == EINVAL and "smaller" in err()
        assert L.w2l_beam_session_bind(h, None, need) == EINVAL
        assert L.w2l_beam_session_bind(h, 0x10010, need) == EINVAL and "aligned" in err()
        assert L.w2l_beam_session_step(None, FAKE, n.ctypes.data, None, None) == EINVAL
        assert L.w2l_beam_session_bind(None, 0x10000, need) == EINVAL
    finally:
        L.w2l_beam_session_destroy(h)


def test_python_front_end_refuses_on_the_host():
    with pytest.raises(_lib.W2LUnsupported, match="wide"):
        streaming.StreamingDecoder(2, 4, 48, 30, wide=True)
    with pytest.raises(_lib.W2LUnsupported):
        streaming.StreamingDecoder(2, 4, 48, 30, beam=65)
    with pytest.raises(ValueError, match="need lm"):
        streaming.StreamingDecoder(2, 4, 48, 30, lm_weight=0.5)
    with pytest.raises(ValueError):
        streaming.StreamingDecoder(2, 0, 48, 30)
    d = streaming.StreamingDecoder(2, 4, 48, 30, beam=16, beam_token=8)
    assert d.state_bytes == _documented_bytes(2, 4, 48, 30, 16, 8) and d.frames(1) == 0
    d.reset(0)
    with pytest.raises(ValueError):
        d.frames(2)


# ---------------------------------------------------------------------------------------------- the inputs are not vacuous
def _beam(x, f, W, K, thr):
    """the beam after f frames: prefixes in rank order with their totals (the float32 restatement of the LM-free search)"""
    hyps, _ = R.beam_search_one(x, f, W, K, thr, False, False, np.float32, None)
    return hyps


@pytest.mark.parametrize("shape", BC.NONVACUOUS)
def test_the_hand_over_has_work_to_do_at_the_chunk_boundaries(shape):
    """Over the boundaries f >= 2 between two steps of the 40-frame utterance (chunks of 1 put one at every frame) all four must
    happen: the beam is full; two entries carry equal totals (rank order must survive the hand-over); the frame after the boundary
    merges an extension into an entry of the beam (needs the parent links); the frame after the boundary keeps an extension that
    repeats the entry's last label (needs pb apart from pnb)."""
    _, _, T, N, W, K, thr, _ = BC.SHAPES[shape]
    x = BC.utterances(shape)[0]
    assert x.shape == (T, N) and (x * 8 == np.round(x * 8)).all()
    K = min(K, N - 1)
    full, ties, merges, repeats = [], [], [], []
    for f in range(2, T):
        beam = _beam(x, f, W, K, thr)
        prefixes = {p for p, _ in beam}
        if len(beam) == W:
            full.append(f)
        tots = [s for _, s in beam]
        if len(set(tots)) < len(tots):
            ties.append(f)
        lp = x[f]
        toks = [int(c) for c in np.lexsort((np.arange(N - 1), -lp[:N - 1]))[:K]]
        if any(p + (c,) in prefixes for p in prefixes for c in toks):
            merges.append(f)
        nxt = {p for p, _ in _beam(x, f + 1, W, K, thr)}
        if any(p and p + (p[-1],) in nxt and p + (p[-1],) not in prefixes for p in prefixes):
            repeats.append(f)
    print(shape, "full", full[:3], "...", "ties", ties, "merges", merges, "repeats kept", repeats)
    assert full and ties and merges and repeats
    for c in (3, 7):
        at = set(range(c, T, c))
        print(shape, "chunks of", c, "full", len(at & set(full)), "ties", len(at & set(ties)), "merges", sorted(at & set(merges)),
              "repeats kept", sorted(at & set(repeats)))


def test_the_tables_have_what_the_l2_and_x2_cases_have():
    for N in (5, 30):
        trie, tb = BC.lexicon_and_word_lm(N)
        spellings = [tuple(sp) for _, sp in trie.rows]
        assert len(set(spellings)) < len(spellings)                                                    # homophones
        assert any(a != b and b[:len(a)] == a for a in set(spellings) for b in set(spellings))         # a word that begins another
        assert trie.sil == N - 2 and all(sp[0] != trie.sil for sp in spellings)
        for t in (tb, BC.token_lm(N)):
            arr = t.arrays()
            assert t.V in (N - 1, trie.num_words) and arr is not None
