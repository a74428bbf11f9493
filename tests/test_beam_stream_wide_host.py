"""Host tests of the wide incremental CTC beam search (w2l_beam_session_create_wide, csrc/criterion_beam_stream.hpp): the refusals
(all before any device call: the library loads without a GPU), the state buffer's arithmetic, the frame bookkeeping through the
shared entry points, and the proof on the CPU that the inputs of test_gpu_beam_stream_wide.py hand over more than 64 entries with
ties, merges and kept repeats at the chunk boundaries.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import beam_stream_wide_cases as WC
from tests import ctc_beam_ref as R
from wav2letter_amd import _lib, streaming

OK, EINVAL, EUNSUPPORTED = _lib.W2L_OK, _lib.W2L_EINVAL, _lib.W2L_EUNSUPPORTED
FAKE = 0x1000     # a non-null table pointer: creation looks at presence only, and no test here reaches the device


def desc(**kw):
    d = dict(slots=3, maxChunk=8, maxFrames=48, N=30, beam=100, beamToken=8, threshold=float("inf"), logAdd=0, normalize=0, variant=0)
    d.update(kw)
    return _lib.BeamSessionDesc(**d)


def create(**kw):
    h = C.c_void_p(0)
    st = _lib.lib().w2l_beam_session_create_wide(C.byref(desc(**kw)), C.byref(h))
    return st, h


def err():
    return _lib.lib().w2l_host_last_error().decode()


LM = dict(variant=1, lm=FAKE, lmHasEos=1, lmWeight=0.5)
LEX = dict(variant=2, lm=FAKE, lmHasEos=1, lmWeight=0.5, lexicon=FAKE, wordScore=0.25)


@pytest.mark.parametrize("kw,want", [
    (dict(beam=65), OK), (dict(beam=500), OK), (dict(beam=1024), OK), (dict(beam=1), OK), (dict(beam=64), OK),
    (dict(beam=1025), EUNSUPPORTED), (dict(N=9998, beamToken=65), EUNSUPPORTED), (dict(LEX, beam=2048), EUNSUPPORTED),
    (dict(beamToken=65), OK),                                               # K is clipped to N - 1 = 29 first
    (dict(N=9998, beamToken=64, beam=1024), OK),
    (dict(maxFrames=1 << 20, beam=512), OK), (dict(maxFrames=(1 << 20) + 1, beam=512), EUNSUPPORTED),   # maxFrames * beam against 2^29
    (dict(maxFrames=1 << 26, beam=16), EUNSUPPORTED),
    # every W2L_EINVAL rule of the narrow check
    (dict(slots=0), EINVAL), (dict(slots=65536), EINVAL), (dict(maxChunk=0), EINVAL), (dict(maxFrames=0), EINVAL), (dict(N=1), EINVAL),
    (dict(beam=0), EINVAL), (dict(beamToken=0), EINVAL), (dict(threshold=-1.0), EINVAL), (dict(threshold=float("nan")), EINVAL),
    (dict(variant=1), EINVAL),
    (dict(LM, lmWeight=float("inf")), EINVAL), (dict(LM, lmHasEos=0, eosScore=1.0), EINVAL), (dict(LM, lexicon=FAKE), EINVAL),
    (dict(LM, wordScore=0.5), EINVAL), (dict(LM, eosScore=float("nan")), EINVAL),
    (dict(variant=2, lm=FAKE), EINVAL),
    (dict(LEX, classScore=FAKE), EINVAL), (dict(LEX, wordScore=float("nan")), EINVAL),
    (dict(lm=FAKE), EINVAL), (dict(lmWeight=0.5), EINVAL), (dict(lexicon=FAKE), EINVAL), (dict(classScore=FAKE), EINVAL),
    (dict(lmHasEos=1), EINVAL), (dict(eosScore=0.5), EINVAL), (dict(wordScore=0.5), EINVAL),
    (dict(beam=0, variant=3), EINVAL),                                      # W2L_EINVAL comes before W2L_EUNSUPPORTED
    (dict(variant=3), EUNSUPPORTED), (dict(variant=-1), EUNSUPPORTED),
    (dict(), OK), (LM, OK), (LEX, OK), (dict(LEX, beam=1024), OK),
])
def test_creation_rules_of_the_wide_session(kw, want):
    L = _lib.lib()
    st, h = create(**kw)
    assert st == want, (kw, err())
    assert (L.w2l_beam_session_wide_state_bytes(C.byref(desc(**kw))) > 0) == (want == OK)
    if want == OK:
        L.w2l_beam_session_destroy(h)
    else:
        assert not h.value and err()
    assert L.w2l_beam_session_create_wide(None, C.byref(h)) == EINVAL
    assert L.w2l_beam_session_create_wide(C.byref(desc(**kw)), None) == EINVAL
    assert L.w2l_beam_session_wide_state_bytes(None) == 0


def test_the_narrow_session_still_refuses_a_beam_above_64():
    L = _lib.lib()
    h = C.c_void_p(0)
    assert L.w2l_beam_session_create(C.byref(desc(beam=65)), C.byref(h)) == EUNSUPPORTED and not h.value
    assert "64" in err()
    assert L.w2l_beam_session_state_bytes(C.byref(desc(beam=65))) == 0
    assert L.w2l_beam_session_create(C.byref(desc(beam=64)), C.byref(h)) == OK
    L.w2l_beam_session_destroy(h)


def _documented_bytes(S, C_, Fmax, N, W, Kt, lex):
    """the layout include/w2l_hip.h states for w2l_beam_session_wide_state_bytes, every part 256-byte aligned"""
    def au(n):
        return (n + 255) // 256 * 256
    K = min(Kt, N - 1)
    cap = 64
    while cap < 2 * Fmax * W:
        cap *= 2
    rows = S * C_
    cand = W * K * (7 if lex else 1) + W
    return (au(3 * S * 4) + 2 * au(rows * 4) + 2 * au(rows * K * 4) + au(S * cap * 8) + au(S * cand * 8) + au(S * 4)
            + (10 if lex else 8) * au(S * W * 4))


def test_wide_state_bytes_is_the_documented_arithmetic():
    L = _lib.lib()
    size = lambda **kw: L.w2l_beam_session_wide_state_bytes(C.byref(desc(**kw)))  # noqa: E731
    for S, C_, Fmax, N, W, K in [(3, 8, 48, 30, 100, 8), (1, 1, 1, 2, 1, 1), (2, 4, 4096, 9998, 1024, 64), (5, 7, 100, 30, 65, 64),
                                 (64, 4, 188, 9998, 500, 64), (3, 8, 48, 30, 16, 8)]:
        kw = dict(slots=S, maxChunk=C_, maxFrames=Fmax, N=N, beam=W, beamToken=K)
        assert size(**kw) == _documented_bytes(S, C_, Fmax, N, W, K, False)
        assert size(**dict(LM, **kw)) == _documented_bytes(S, C_, Fmax, N, W, K, False)
        assert size(**dict(LEX, **kw)) == _documented_bytes(S, C_, Fmax, N, W, K, True) > size(**kw)     # 7 slots per token, 2 more arrays
    base = size()
    assert size(maxFrames=4800) > base and size(beam=200) > base and size(slots=30) > base and size(maxChunk=80) > base
    assert size(beam=1025) == 0 and size(N=9998, beamToken=65) == 0 and size(slots=0) == 0
    # the figures the documentation quotes: W = 1024, maxFrames = 4096 is a 64 MiB table per slot (2^23 edges of 8 bytes), the
    # candidate list with a lexicon at K = 64 is 3.6 MiB
    big = dict(maxFrames=4096, beam=1024, N=9998, beamToken=64)
    per_slot = size(slots=2, **big) - size(slots=1, **big)
    assert 64 << 20 <= per_slot < (64 << 20) + (1 << 20)
    cand = (1024 * 64 * 7 + 1024) * 8
    assert 3.5 * 2 ** 20 < cand < 3.6 * 2 ** 20
    per_slot_lex = size(slots=2, **dict(LEX, **big)) - size(slots=1, **dict(LEX, **big))
    assert per_slot_lex - per_slot == (1024 * 64 * 6) * 8 + 2 * 1024 * 4


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
        assert counts([0, 0, 0]) == OK
        assert counts([1, 0, 0]) == EINVAL and "slot 0" in err() and "started" in err()   # frames for a never-started slot
        assert counts([8, 0, 3], [1, 0, 1]) == OK and frames() == [8, 0, 3]
        assert counts([8, 0, 0]) == OK and counts([0, 5, 8], [0, 1, 0]) == OK and frames() == [16, 5, 11]
        before = frames()
        assert counts([9, 0, 0]) == EINVAL and "0..8" in err() and frames() == before     # above maxChunk
        assert counts([-1, 0, 0]) == EINVAL and frames() == before
        for _ in range(4):
            assert counts([8, 8, 8]) == OK
        assert frames() == [48, 37, 43]                                                    # slot 0 sits exactly at maxFrames
        before = frames()
        assert counts([1, 1, 1]) == EINVAL and "slot 0" in err() and "maxFrames = 48" in err()
        assert frames() == before                                                          # a refused step moves no count, of any slot
        assert counts([0, 1, 6], [0, 0, 0]) == EINVAL and "slot 2" in err() and frames() == before
        assert counts([1, 1, 1], [1, 0, 0]) == OK and frames() == [1, 38, 44]
        assert L.w2l_beam_session_reset(h, 1) == OK and frames() == [1, 0, 44]
        assert counts([0, 1, 0]) == EINVAL and "slot 1" in err()                            # a reset slot is closed
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
        need = L.w2l_beam_session_wide_state_bytes(C.byref(desc()))
        assert need > L.w2l_beam_session_state_bytes(C.byref(desc(beam=64)))
        assert L.w2l_beam_session_bind(h, 0x10000, need - 1) == EINVAL and "smaller" in err() and "wide_state_bytes" in err()
        assert L.w2l_beam_session_bind(h, None, need) == EINVAL
        assert L.w2l_beam_session_bind(h, 0x10010, need) == EINVAL and "aligned" in err()
        # still unbound: the refused binds bound nothing, and nbest is not looked at before the state is
        for nbest in (0, 101, 1):
            assert L.w2l_beam_session_result(h, nbest, 8, FAKE, FAKE, FAKE, FAKE, 0, None, None, None) == EINVAL
        assert L.w2l_beam_session_step(h, FAKE, n.ctypes.data, None, None) == EINVAL and "bind" in err()
    finally:
        L.w2l_beam_session_destroy(h)


def test_python_front_end_refuses_on_the_host():
    with pytest.raises(_lib.W2LUnsupported, match="wide"):
        streaming.StreamingDecoder(2, 4, 48, 30, wide=True)
    with pytest.raises(_lib.W2LUnsupported):
        streaming.StreamingDecoder(2, 4, 48, 30, beam=65)
    with pytest.raises(_lib.W2LUnsupported):
        streaming.WideStreamingDecoder(2, 4, 48, 30, beam=1025)
    with pytest.raises(_lib.W2LUnsupported):
        streaming.WideStreamingDecoder(2, 4, 48, 9998, beam=100, beam_token=65)
    with pytest.raises(_lib.W2LUnsupported):
        streaming.WideStreamingDecoder(2, 4, 1 << 22, 30, beam=512)
    with pytest.raises(TypeError):
        streaming.WideStreamingDecoder(2, 4, 48, 30, wide=True)          # StreamingDecoder's arguments minus `wide`
    with pytest.raises(ValueError, match="need lm"):
        streaming.WideStreamingDecoder(2, 4, 48, 30, lm_weight=0.5)
    with pytest.raises(ValueError, match="needs lexicon"):
        streaming.WideStreamingDecoder(2, 4, 48, 30, word_score=0.5)
    with pytest.raises(ValueError):
        streaming.WideStreamingDecoder(2, 0, 48, 30)
    d = streaming.WideStreamingDecoder(2, 4, 48, 30, beam=500, beam_token=8)
    assert isinstance(d, streaming.StreamingDecoder)
    assert d.state_bytes == _documented_bytes(2, 4, 48, 30, 500, 8, False) and d.frames(1) == 0
    assert streaming.WideStreamingDecoder(2, 4, 48, 30).beam == 1024
    d.reset(0)
    with pytest.raises(ValueError):
        d.frames(2)


# ---------------------------------------------------------------------------------------------- the inputs are not vacuous
@functools.lru_cache(maxsize=None)
def _beam(shape, f):
    """the beam after f frames: prefixes in rank order with their totals (the float32 restatement of the LM-free search)"""
    _, _, _, N, W, K, thr, _ = WC.SHAPES[shape]
    hyps, _ = R.beam_search_one(WC.utterances(shape)[0], f, W, min(K, N - 1), thr, False, False, np.float32, None)
    return hyps


@pytest.mark.parametrize("shape", sorted(WC.SHAPES))
def test_the_wide_hand_over_has_work_to_do_at_the_chunk_boundaries(shape):
    """test_beam_stream_host's method on the wide shapes.  Over the boundaries f >= 2 each of the four happens at least 3 times:
    the beam is full; two entries carry equal totals; the frame after the boundary merges an extension into an entry of the beam;
    it keeps an extension that repeats the entry's last label.  And the beam that is handed over holds MORE THAN 64 entries -- the
    state beyond the narrow session's -- at some boundary of the chunkings by 3 and by 7 too."""
    _, _, T, N, W, K, thr, _ = WC.SHAPES[shape]
    xs = WC.utterances(shape)
    x = xs[0]
    assert x.shape == (T, N) and (x * 8 == np.round(x * 8)).all() and [len(u) for u in xs] == [T, min(17, T), 1]
    assert tuple(len(_beam(shape, f)) for f in range(1, 1 + len(WC.BEAM_SIZES[shape]))) == WC.BEAM_SIZES[shape]
    K = min(K, N - 1)
    size, full, ties, merges, repeats = {}, [], [], [], []
    for f in range(2, T):
        beam = _beam(shape, f)
        size[f] = len(beam)
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
        nxt = {p for p, _ in _beam(shape, f + 1)}
        if any(p and p + (p[-1],) in nxt and p + (p[-1],) not in prefixes for p in prefixes):
            repeats.append(f)
    print(shape, "sizes", [size[f] for f in sorted(size)][:6], "full", len(full), "ties", len(ties), "merges", len(merges),
          "repeats kept", len(repeats))
    assert W > 64 and max(size.values()) > 64
    assert min(len(full), len(ties), len(merges), len(repeats)) >= 3
    for c in (3, 7):
        at = set(range(c, T, c))
        print(shape, "chunks of", c, "sizes", [size[f] for f in sorted(at)])
        assert any(size[f] > 64 for f in at)
