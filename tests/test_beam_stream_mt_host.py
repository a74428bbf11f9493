"""Host tests of the many-token incremental CTC beam search (w2l_beam_session_create_mt, csrc/criterion_beam_stream.hpp over
csrc/criterion_beam_xl.hpp): the refusals through the C ABI (all before any device call: the library loads without a GPU), the
state buffer's arithmetic, the frame bookkeeping of ManyTokenStreamingDecoder.counts, and the proof on the CPU, with
beam_mt_ref.mt_beam_one's counts, that the inputs of test_gpu_beam_stream_mt.py give the hand-over work to do.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import beam_mt_ref as MR
from tests import beam_stream_cases as BC
from tests import beam_stream_mt_cases as MC
from wav2letter_amd import _lib, streaming

OK, EINVAL, EUNSUPPORTED = _lib.W2L_OK, _lib.W2L_EINVAL, _lib.W2L_EUNSUPPORTED
FAKE = 0x1000     # a non-null table pointer: creation looks at presence only, and no test here reaches the device
LM = dict(variant=1, lm=FAKE, lmHasEos=1, lmWeight=0.5)
LEX = dict(variant=2, lm=FAKE, lmHasEos=1, lmWeight=0.5, lexicon=FAKE, wordScore=0.25)


def desc(**kw):
    d = dict(slots=3, maxChunk=8, maxFrames=48, N=300, beam=500, beamToken=100, threshold=float("inf"), logAdd=0, normalize=0, variant=0)
    d.update(kw)
    return _lib.BeamSessionDesc(**d)


def create(sil=(-1, 0.0), fn="w2l_beam_session_create_mt", **kw):
    h = C.c_void_p(0)
    f = getattr(_lib.lib(), fn)
    st = f(C.byref(desc(**kw)), int(sil[0]), float(sil[1]), C.byref(h)) if fn.endswith("_mt") else f(C.byref(desc(**kw)), C.byref(h))
    return st, h


def err():
    return _lib.lib().w2l_host_last_error().decode()


# ---------------------------------------------------------------------------------------------------------- limits and refusals
@pytest.mark.parametrize("kw,sil,want", [
    (dict(), (-1, 0.0), OK), (LM, (-1, 0.0), OK), (LEX, (5, -1.0), OK), (dict(), (298, 0.5), OK), (dict(), (0, 0.0), OK),
    (dict(beam=8192, beamToken=256), (-1, 0.0), OK), (dict(beam=1, beamToken=1), (-1, 0.0), OK),
    (dict(beamToken=257), (-1, 0.0), EUNSUPPORTED),                          # K 257 after clipping (N - 1 = 299)
    (dict(N=257, beamToken=1000), (-1, 0.0), OK),                            # clipped to N - 1 = 256 first
    (dict(N=258, beamToken=1000), (-1, 0.0), EUNSUPPORTED),
    (dict(beam=8193), (-1, 0.0), EUNSUPPORTED), (dict(LEX, beam=8193), (-1, 0.0), EUNSUPPORTED),
    (dict(maxFrames=1 << 20, beam=512), (-1, 0.0), OK), (dict(maxFrames=(1 << 20) + 1, beam=512), (-1, 0.0), EUNSUPPORTED),
    (dict(), (-1, float("inf")), EINVAL), (dict(), (3, float("nan")), EINVAL), (dict(), (3, float("-inf")), EINVAL),
    (dict(), (299, 0.5), EINVAL),                                            # silToken = N - 1: the blank is no token
    (dict(), (-2, 0.5), EINVAL), (dict(), (300, 0.0), EINVAL),
    (dict(beam=8193), (299, 0.5), EINVAL),                                   # the silence pair comes before everything else
    (dict(variant=3), (0, float("inf")), EINVAL),
    # the wide session's refusals, in its order
    (dict(slots=0), (-1, 0.0), EINVAL), (dict(maxChunk=0), (-1, 0.0), EINVAL), (dict(beam=0), (-1, 0.0), EINVAL),
    (dict(threshold=float("nan")), (-1, 0.0), EINVAL), (dict(variant=1), (-1, 0.0), EINVAL), (dict(lm=FAKE), (-1, 0.0), EINVAL),
    (dict(LM, lexicon=FAKE), (-1, 0.0), EINVAL), (dict(LEX, classScore=FAKE), (-1, 0.0), EINVAL),
    (dict(beam=0, variant=3), (-1, 0.0), EINVAL), (dict(variant=3), (-1, 0.0), EUNSUPPORTED),
    (dict(beam=0, beamToken=257), (-1, 0.0), EINVAL),                        # W2L_EINVAL comes before W2L_EUNSUPPORTED
])
def test_creation_rules_of_the_many_token_session(kw, sil, want):
    L = _lib.lib()
    st, h = create(sil, **kw)
    assert st == want, (kw, sil, err())
    if want == OK:
        assert L.w2l_beam_session_mt_state_bytes(C.byref(desc(**kw))) > 0
        L.w2l_beam_session_destroy(h)
    else:
        assert not h.value and err()
    if want == EUNSUPPORTED:
        assert L.w2l_beam_session_mt_state_bytes(C.byref(desc(**kw))) == 0
    assert L.w2l_beam_session_create_mt(None, -1, 0.0, C.byref(h)) == EINVAL
    assert L.w2l_beam_session_create_mt(C.byref(desc(**kw)), -1, 0.0, None) == EINVAL
    assert L.w2l_beam_session_mt_state_bytes(None) == 0


def test_the_documented_codes_and_messages():
    st, _ = create(beamToken=257)
    assert st == EUNSUPPORTED and "256" in err() and "many-token" in err()
    st, _ = create(beam=8193)
    assert st == EUNSUPPORTED and "8192" in err()
    st, _ = create((-1, float("inf")))
    assert st == EINVAL and "silScore" in err()
    st, _ = create((299, 0.5))
    assert st == EINVAL and "silToken" in err()


def test_the_narrow_and_wide_creators_still_refuse_65_tokens_with_their_old_messages():
    L = _lib.lib()
    kw = dict(N=9998, beam=64, beamToken=65)
    st, h = create(fn="w2l_beam_session_create", **kw)
    assert st == EUNSUPPORTED and not h.value
    assert err() == ("beam session: beam and beamToken above 64 (the wide searches) are not incremental here; "
                     "w2l_beam_session_create_wide takes a beam up to 1024")
    st, h = create(fn="w2l_beam_session_create_wide", **kw)
    assert st == EUNSUPPORTED and not h.value
    assert err() == "wide beam session: beam above 1024 or beamToken (clipped to N - 1) above 64"
    assert L.w2l_beam_session_state_bytes(C.byref(desc(**kw))) == 0 and L.w2l_beam_session_wide_state_bytes(C.byref(desc(**kw))) == 0
    st, h = create(**kw)
    assert st == OK
    L.w2l_beam_session_destroy(h)


def test_commit_bytes_is_0_above_beam_1024_and_commit_is_refused_before_anything_else():
    L = _lib.lib()
    st, h = create(beam=1025)
    assert st == OK
    try:
        assert L.w2l_beam_session_commit_bytes(h) == 0
        n = np.zeros(3, np.int32)
        # not bound, no scratch, no labels: the limit is what the call names
        assert L.w2l_beam_session_commit(h, None, None, 0, 8, None, 0, None, n.ctypes.data, None, None, None) == EUNSUPPORTED
        assert "1024" in err() and "1025" in err()
    finally:
        L.w2l_beam_session_destroy(h)
    st, h = create(beam=1024)
    assert st == OK
    try:
        assert L.w2l_beam_session_commit_bytes(h) == _commit_bytes(3, 48, 1024)
        assert L.w2l_beam_session_commit(h, None, None, 0, 8, None, 0, None, n.ctypes.data, None, None, None) == EINVAL
    finally:
        L.w2l_beam_session_destroy(h)


def au(n):
    return (n + 255) // 256 * 256


def _cap(Fmax, W):
    cap = 64
    while cap < 2 * Fmax * W:
        cap *= 2
    return cap


def _commit_bytes(S, Fmax, W):
    return au(4 * S * 4) + au(_cap(Fmax, W) * 8) + au(Fmax * W * 4)


def _documented_bytes(S, C_, Fmax, N, W, Kt, lex):
    """the layout include/w2l_hip.h states for w2l_beam_session_mt_state_bytes, every part 256-byte aligned"""
    K = min(Kt, N - 1)
    rows, slots, kF = S * C_, 7 if lex else 1, 9 if lex else 8
    return (au(3 * S * 4)                                                    # the control ints
            + 2 * au(rows * 4) + 2 * au(rows * K * 4)                        # the chunk's row pass
            + au(S * _cap(Fmax, W) * 8)                                      # S prefix tables
            + au(S * (W * K * slots + W) * 8)                                # S candidate lists
            + au(S * slots * W * ((K + 63) // 64) * 8)                       # S gone-mask areas
            + au(S * 2 * W * 4)                                              # S stay areas
            + au(S * 2 * 4)                                                  # S x (cur, n)
            + au(S * 2 * kF * W * 4)                                         # the beam halves
            + (5 if lex else 4) * au(S * W * 4) + au(S * 4))                 # what the finish reads


def test_mt_state_bytes_is_the_documented_arithmetic():
    L = _lib.lib()
    size = lambda **kw: L.w2l_beam_session_mt_state_bytes(C.byref(desc(**kw)))  # noqa: E731
    for S, C_, Fmax, N, W, K in [(3, 8, 48, 300, 500, 100), (1, 1, 1, 2, 1, 1), (2, 4, 1024, 9998, 500, 100), (5, 7, 100, 130, 200, 129),
                                 (64, 4, 188, 9998, 2500, 100), (3, 8, 48, 30, 16, 8), (2, 3, 16, 300, 8192, 256), (2, 3, 16, 70, 65, 65)]:
        kw = dict(slots=S, maxChunk=C_, maxFrames=Fmax, N=N, beam=W, beamToken=K)
        assert size(**kw) == _documented_bytes(S, C_, Fmax, N, W, K, False)
        assert size(**dict(LM, **kw)) == _documented_bytes(S, C_, Fmax, N, W, K, False)
        assert size(**dict(LEX, **kw)) == _documented_bytes(S, C_, Fmax, N, W, K, True) > size(**kw)
    # the figures the header quotes: beam 500, K = 100, maxFrames 1024 with a lexicon
    assert _cap(1024, 500) * 8 == 8 << 20
    assert 2.6 * 2 ** 20 < (500 * 100 * 7 + 500) * 8 < 2.7 * 2 ** 20
    assert 54 * 1024 < 7 * 500 * 2 * 8 < 55 * 1024


# ------------------------------------------------------------------------------------------------------------- the Python class
def test_counts_is_the_step_rule_on_the_host():
    S, Cm, Fmax = 3, 8, 48
    d = streaming.ManyTokenStreamingDecoder(S, Cm, Fmax, 300)                 # LM-free: no table, no device
    assert (d.beam, d.sil_token, d.sil_score) == (500, -1, 0.0)
    assert d.state_bytes == _documented_bytes(S, Cm, Fmax, 300, 500, 100, False)
    frames = lambda: [d.frames(s) for s in range(S)]  # noqa: E731
    assert frames() == [0, 0, 0]
    d.counts([0, 0, 0])
    with pytest.raises(ValueError, match="slot 0.*started"):
        d.counts([1, 0, 0])
    d.counts([8, 0, 3], [1, 0, 1])
    assert frames() == [8, 0, 3]
    d.counts([8, 0, 0])
    d.counts([0, 5, 8], [0, 1, 0])
    assert frames() == [16, 5, 11]
    with pytest.raises(ValueError, match="0..8"):
        d.counts([9, 0, 0])
    assert frames() == [16, 5, 11]
    for _ in range(4):
        d.counts([8, 8, 8])
    assert frames() == [48, 37, 43]
    with pytest.raises(ValueError, match="slot 0.*maxFrames = 48"):
        d.counts([1, 1, 1])
    assert frames() == [48, 37, 43]                                          # a refused step moves no count, of any slot
    d.counts([1, 1, 1], [1, 0, 0])
    assert frames() == [1, 38, 44]
    d.reset(1)
    assert frames() == [1, 0, 44]
    with pytest.raises(ValueError):
        d.counts([1, 1])


def test_python_front_end_refuses_on_the_host():
    M = streaming.ManyTokenStreamingDecoder
    assert issubclass(M, streaming.StreamingDecoder)
    with pytest.raises(_lib.W2LUnsupported, match="8192"):
        M(2, 4, 48, 300, beam=8193)
    with pytest.raises(_lib.W2LUnsupported, match="256"):
        M(2, 4, 48, 300, beam_token=257)
    with pytest.raises(_lib.W2LUnsupported):
        M(2, 4, 1 << 22, 300, beam=512)
    with pytest.raises(ValueError, match="silence token"):
        M(2, 4, 48, 300, sil_score=0.5)
    with pytest.raises(ValueError, match="silToken"):
        M(2, 4, 48, 300, sil_token=299, sil_score=0.5)
    with pytest.raises(ValueError, match="silScore"):
        M(2, 4, 48, 300, sil_token=3, sil_score=float("inf"))
    with pytest.raises(TypeError):
        M(2, 4, 48, 300, wide=True)
    d = M(2, 4, 48, 300, beam=8192, beam_token=256, sil_token=7, sil_score=-1.0)
    assert (d.sil_token, d.sil_score) == (7, -1.0)
    # the two older classes keep their limits
    with pytest.raises(_lib.W2LUnsupported):
        streaming.StreamingDecoder(2, 4, 48, 300, beam=64, beam_token=65)
    with pytest.raises(_lib.W2LUnsupported):
        streaming.WideStreamingDecoder(2, 4, 48, 300, beam=100, beam_token=65)
    with pytest.raises(TypeError):
        streaming.WideStreamingDecoder(2, 4, 48, 300, sil_score=0.5)


# ---------------------------------------------------------------------------------------------- the inputs are not vacuous
@functools.lru_cache(maxsize=None)
def _plain(shape, slot, f):
    """(beam size, MtDiag) of the LM-free search after f frames (float32): without an end rule every entry is a row"""
    _, _, _, N, W, K, thr, _ = MC.SHAPES[shape]
    rows, d = MR.mt_beam_one(MC.utterances(shape)[slot], f, W, K, threshold=thr)
    return len(rows), d


@pytest.mark.parametrize("shape", sorted(MC.SHAPES))
def test_the_many_token_hand_over_has_work_to_do(shape):
    _, _, T, N, W, K, thr, _ = MC.SHAPES[shape]
    xs = MC.utterances(shape)
    assert xs[0].shape == (T, N) and [len(u) for u in xs] == [T, min(17, T), 1]
    assert all((x * 8 == np.round(x * 8)).all() for x in xs)
    K = min(K, N - 1)
    # the beam binds at least two frames before the end: a full beam crosses a chunk boundary under every chunking but "all"
    n_early, _ = _plain(shape, 0, T - 2)
    n_end, d_end = _plain(shape, 0, T)
    assert n_early == W and n_end == W
    # merges in every mask word, in frames after the second (cumulative counts: those up to frame f are the search of f frames')
    words = (K + 63) // 64
    _, d2 = _plain(shape, 0, 2)
    later = [d_end.merges[0][w] - d2.merges[0][w] for w in range(4)]
    print(shape, "merges by mask word", d_end.merges[0], "of them after frame 2", later)
    assert all(m > 0 for m in later[:words]) and not any(later[words:])
    if shape in MC.MANY:
        assert words >= 2
    # the lexicon variant completes words (slots above 0), in every mask word it has merges in, and hides unfinished entries
    trie, tb = BC.lexicon_and_word_lm(N)
    rows, dl = MR.mt_beam_one(xs[0], T, W, K, sil=trie.sil, lm=tb, trie=trie, lm_weight=0.5, word_score=-0.25, eos_score=-0.25, threshold=thr)
    print(shape, "lexicon: rows", len(rows), "with words", sum(1 for r in rows if r[1]), "word-slot merges", dl.merges[1], "hidden",
          dl.end_dropped)
    assert sum(1 for r in rows if r[1]) >= 3 and dl.merges[1][0] > 0 and dl.end_dropped > 0
    if shape in MC.MANY:
        assert dl.merges[1][1] > 0


def test_the_threshold_line_cuts_and_hands_over_a_beam_it_cut():
    """At W = 300 and K = 256 a frame has more than W candidates inside a line of 4 from its second frame on (the beam fills),
    so the line is what decides in an utterance's FIRST frame: there fewer than W of the 257 candidates survive although more than
    that many exist.  It does so in the first frame of each of the three utterances of the schedule -- three frames, in three slots
    -- and every one of those beams is handed over at a chunk boundary (every chunking but "all" ends a chunk after frame 1)."""
    shape = "peaked_n260_w300_k256_thr4"
    _, _, T, N, W, K, thr, _ = MC.SHAPES[shape]
    cut = []
    for slot in range(3):
        n1, _ = _plain(shape, slot, 1)
        print(shape, "slot", slot, "beam after frame 1:", n1, "of", K + 1, "candidates")
        if n1 < min(W, K + 1):
            cut.append(slot)
    assert len(cut) >= 2
    # and without the line the first frame keeps all 257
    assert len(MR.mt_beam_one(MC.utterances(shape)[0], 1, W, K)[0]) == K + 1
