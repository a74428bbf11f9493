"""Host tests of the chunked streaming forward: the numpy protocol model against the numpy whole-utterance forward (index
arithmetic, independent of the device), the library's count bookkeeping against the model's, and the refusals.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import stream_ref as R
from wav2letter_amd import _lib, streaming

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _model_and_whole(seed, T):
    rng = np.random.default_rng(seed)
    layers = R.tiny_layers(rng)
    x = rng.normal(size=(T, R.NFEAT))
    return R.StreamModel(layers, R.NFEAT), x, R.whole_forward(layers, x)


# ---------------------------------------------------------------------------------------------- numpy model == whole forward
@pytest.mark.parametrize("T", range(1, 10))
def test_model_equals_whole_forward_for_every_composition(T):
    """all 2^(T-1) splits of T <= 9 frames, float64, 1e-12"""
    model, x, want = _model_and_whole(T, T)
    n = 0
    for chunks in R.compositions(T):
        got, counts, _ = R.stream_utterance(model, x, chunks)
        assert got.shape == want.shape, (chunks, got.shape, want.shape)
        assert sum(counts) == want.shape[0]
        if want.size:
            assert np.abs(got - want).max() < 1e-12, chunks
        n += 1
    assert n == 1 << (T - 1)


@pytest.mark.parametrize("T", [10, 17, 23, 40, 64])
def test_model_equals_whole_forward_for_random_chunkings_with_zero_chunks(T):
    model, x, want = _model_and_whole(100 + T, T)
    rng = np.random.default_rng(T)
    zero_seen = False
    for _ in range(12):
        chunks = R.random_chunking(rng, T, 17)
        zero_seen = zero_seen or 0 in chunks
        got, counts, _ = R.stream_utterance(model, x, chunks)
        assert got.shape == want.shape, chunks
        assert np.abs(got - want).max() < 1e-12, chunks
    assert zero_seen


def test_whole_forward_frame_count_is_the_plans():
    """Tout of the tiny arch by the conv arithmetic: two strides of 2 under the asymmetric PDs"""
    for T in (1, 5, 23, 40, 64):
        model, x, want = _model_and_whole(7, T)
        t1 = (T + 2 + 1 - 3) // 2 + 1
        t2 = (t1 + 3 + 0 - 4) // 2 + 1
        assert want.shape == (max(t2, 0), R.NLABEL)


# ---------------------------------------------------------------------------------------------- library counts == model counts
def _session(slots, max_chunk, arch=R.TINY_ARCH, nfeat=R.NFEAT, nlabel=R.NLABEL):
    return streaming.StreamingSession.from_arch(arch, nfeat, nlabel, None, slots, max_chunk)


def test_library_counts_equal_the_models():
    """nOut per step and the carry count of every time-extent layer, on random chunkings with zero-length chunks, two slots at
    different phases, and a slot that is started, finished and started again"""
    S, cmax = 2, 17
    sess = _session(S, cmax)
    assert sess.num_time_layers == 5
    rng = np.random.default_rng(3)
    models = [R.StreamModel(R.tiny_layers(rng), R.NFEAT) for _ in range(S)]
    max_seen = 0
    for rnd in range(3):   # each slot: three utterances one after the other
        plans = []
        for s in range(S):
            T = int(rng.integers(1, 65))
            plans.append((rng.normal(size=(T, R.NFEAT)), R.random_chunking(rng, T, cmax)))
        pos = [0] * S
        for i in range(max(len(p[1]) for p in plans) + 1):
            n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
            want = np.zeros(S, np.int32)
            for s, (x, chunks) in enumerate(plans):
                k = i - s   # slot 1 lags one step behind slot 0: idle first, different phase afterwards
                if 0 <= k < len(chunks):
                    n[s], st[s], fi[s] = chunks[k], k == 0, k == len(chunks) - 1
                    y = models[s].step(x[pos[s]:pos[s] + chunks[k]], start=bool(st[s]), finish=bool(fi[s]))
                    pos[s] += chunks[k]
                    want[s] = y.shape[0]
            got = sess.counts(n, st, fi)
            assert (got == want).all(), (rnd, i, n, st, fi, got, want)
            max_seen = max(max_seen, int(got.max()))
            for s, (x, chunks) in enumerate(plans):
                k = i - s
                active, carry = sess.slot_state(s)
                if 0 <= k < len(chunks) - 1:
                    assert active and list(carry) == models[s].carry_frames(), (rnd, i, s)
                elif k >= len(chunks) - 1:
                    assert not active and not carry.any()
    assert 0 < max_seen <= sess.max_out


def test_max_out_bounds_every_step_and_is_reached():
    """maxOut from the host query for (arch, Cmax): no step returns more, and full chunks in steady state reach it"""
    for cmax in (1, 3, 8, 17):
        mo, sb = streaming.query(R.TINY_ARCH, R.NFEAT, R.NLABEL, 3, cmax)
        sess = _session(3, cmax)
        assert mo == sess.max_out and sb == sess.state_bytes and sb > 0
        top = 0
        out = sess.counts([cmax] * 3, [1] * 3, None)
        for _ in range(8):
            out = sess.counts([cmax] * 3)
            top = max(top, int(out.max()))
        out = sess.counts([cmax] * 3, None, [1] * 3)
        top = max(top, int(out.max()))
        assert top <= mo
        assert top >= mo - 1   # the window is sized for the worst phase (longest carry + full chunk + right padding)


def test_total_count_equals_whole_plan_for_short_utterances():
    """shorter than the receptive field: everything comes out at finish, and the total is the whole plan's"""
    sess = _session(1, 8)
    for T in (1, 2, 3, 4):
        model, x, want = _model_and_whole(T, T)
        first = sess.counts([T], [1], None)
        last = sess.counts([0], None, [1])
        assert first[0] + last[0] == want.shape[0]
        assert first[0] == 0


# ---------------------------------------------------------------------------------------------- refusals
_HEAD = "V -1 NFEAT 1 0\nC2 1 4 3 1 1 1 1 0\n"
_HEAD1 = "V -1 1 NFEAT 0\nC2 4 16 3 1 1 1 1 0\n"   # H = 1: the frame is one factor
_TAIL = "RO 2 1 0 3\nV 16 -1 1 0\nL 16 NLABEL\n"


@pytest.mark.parametrize("line,head,tail", [
    ("TR 16 32 2 8 0.1", _HEAD1 + "RO 2 0 3 1\n", "L 16 NLABEL\n"),
    ("LN 0 1 2", _HEAD, _TAIL),
    ("TDS 4 3 4 0.1 0 1 1", _HEAD, _TAIL),
    ("TDS 4 3 4 0.1", _HEAD, _TAIL),                    # lnIncludeTime defaults to 1 (config 2's form)
    ("M 2 1 2 1", _HEAD, _TAIL),
    ("C2 4 4 3 1 2 1 -1 0", _HEAD, _TAIL),              # SAME padding at stride 2: the pad depends on T
    ("GLU 0", _HEAD1 + "RO 2 0 1 3\n", "L 8 NLABEL\n"),
])
def test_non_streamable_lines_are_refused_with_the_line_named(line, head, tail):
    arch = head + line + "\n" + tail
    L = _lib.lib()
    n = C.c_int(0)
    assert L.w2l_arch_check(arch.encode(), 4, 5, C.byref(n)) == 0   # the arch itself is one the trainer builds
    h = C.c_void_p(0)
    st = L.w2l_stream_create(arch.encode(), 4, 5, 2, 8, C.byref(h))
    assert st == _lib.W2L_EUNSUPPORTED and not h.value
    assert line in L.w2l_host_last_error().decode()
    with pytest.raises(_lib.W2LUnsupported, match=line.split()[0]):
        _session(2, 8, arch)


def test_streamable_recipe_and_config2_refusal():
    """the streaming recipe (config 3) is accepted as it stands; config 2's TDS arch (lnIncludeTime = 1) is refused"""
    rec = json.load(open(os.path.join(GOLD, "reference_recipes.json")))["arch"]
    arch = rec["streaming_convnets/librispeech/am_500ms_future_context.arch"]
    mo, sb = streaming.query(arch, 80, 9998, 4, 16)
    # the window arithmetic restated on the arch lines: carry capacity max(kw - 1, padL), window = capacity + the producer's most
    # frames + padR, most frames out = (window - kw) / stride + 1
    nmax, pd = 16, (0, 0)
    for ln in arch.splitlines():
        a = ln.split()
        if a[0] == "PD":
            pd = (int(a[2]), int(a[3]))
        elif a[0] in ("C2", "TDS"):
            kw, stride = (int(a[3]), int(a[5])) if a[0] == "C2" else (int(a[2]), 1)
            padl, padr = pd if a[0] == "C2" else (kw - 1 - int(a[6]), int(a[6]))
            nmax = (max(kw - 1, padl) + nmax + padr - kw) // stride + 1
            pd = (0, 0)
    assert mo == nmax and 2 <= mo <= 16 and sb > 0
    for k in ("sota/2019/am_arch/am_tds_ctc.arch", "sota/2019/am_arch/am_tds_ctc_librivox.arch"):
        with pytest.raises(_lib.W2LUnsupported) as e:   # its first offending line: the SAME-padded strided C2, or the TDS
            streaming.query(rec[k], 80, 9998, 2, 16)
        named = str(e.value).split("'")[1]
        assert named in rec[k].splitlines() and named.split()[0] in ("C2", "TDS"), named


def test_mixed_precision_trainer_is_refused():
    L = _lib.lib()
    from wav2letter_amd import trainer as T
    Lt = T._lib_tr()
    tr = Lt.w2l_trainer_create(R.TINY_ARCH.encode(), R.NFEAT, R.NLABEL, b"ctc", 0, 0.0)
    assert tr
    try:
        h = C.c_void_p(0)
        assert L.w2l_stream_create_for_trainer(tr, 2, 8, C.byref(h)) == 0 and h.value
        assert L.w2l_stream_max_out(h) == streaming.query(R.TINY_ARCH, R.NFEAT, R.NLABEL, 2, 8)[0]
        L.w2l_stream_destroy(h)
        Lt.w2l_trainer_set_mixed_precision(tr, 1)
        h = C.c_void_p(0)
        assert L.w2l_stream_create_for_trainer(tr, 2, 8, C.byref(h)) == _lib.W2L_EUNSUPPORTED and not h.value
        assert "mixed-precision" in L.w2l_host_last_error().decode()
    finally:
        Lt.w2l_trainer_destroy(tr)


def test_argument_checks_come_before_any_state_change():
    sess = _session(2, 8)
    with pytest.raises(_lib.W2LInvalidArgument, match="outside 0..8"):
        sess.counts([9, 0], [1, 0], None)
    assert not sess.slot_state(0)[0]                     # the refused call started nothing
    with pytest.raises(_lib.W2LInvalidArgument, match="finishes before it was started"):
        sess.counts([0, 0], None, [0, 1])
    with pytest.raises(_lib.W2LInvalidArgument, match="is fed before it was started"):
        sess.counts([0, 3], None, None)
    sess.counts([8, 0], [1, 0], None)
    with pytest.raises(_lib.W2LInvalidArgument):
        sess.counts([1, -1], None, None)
    active, carry = sess.slot_state(0)
    assert active and carry.any()
    sess.reset(0)
    assert not sess.slot_state(0)[0]
    with pytest.raises(_lib.W2LInvalidArgument):
        sess.counts([1, 0], None, None)                  # a reset slot has to be started again
    L = _lib.lib()
    n = (C.c_int * 2)(1, 1)
    out = (C.c_int * 2)()
    assert L.w2l_stream_step(sess.h, None, n, None, None, None, out, None) == _lib.W2L_EINVAL       # null input
    assert L.w2l_stream_step(sess.h, 256, n, None, None, None, None, None) == _lib.W2L_EINVAL       # null nOut
    assert L.w2l_stream_step(sess.h, 256, n, n, None, None, out, None) == _lib.W2L_EINVAL           # nothing bound
    assert L.w2l_stream_bind(sess.h, None, None, 0) == _lib.W2L_EINVAL
    assert L.w2l_stream_create(None, 4, 5, 2, 8, None) == _lib.W2L_EINVAL
