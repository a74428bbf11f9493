"""Host-side checks of the streaming log-mel front end (no GPU): the numpy model in the reference's buffer / consume form
(tests/feat_stream_ref.py) against oracle.mfsc of the whole signal over every chunking of short signals, the library's count
arithmetic (w2l_feat_session_counts, host only) against the model's, max_out against its formula, the refusals, the ABI."""
import ctypes as C

import numpy as np
import pytest

import feat_stream_ref as R
from wav2letter_amd import _lib
from wav2letter_amd.features import Mfsc
from wav2letter_amd.streaming import StreamingFeatures, feat_desc

TOY = dict(fs=1000, frame_ms=10, stride_ms=3, num_filters=5)   # N = 10, St = 3, nfft = 16


def toy_mfsc():
    return Mfsc(device="cpu", **TOY)


def test_toy_geometry():
    fe = toy_mfsc()
    assert (fe.N, fe.S, fe.nfft, fe.nb) == (10, 3, 16, 9) == R.geometry(1000, 10, 3)[:4]
    d = feat_desc(fe)
    assert (d.frameSize, d.frameStride, d.nbins, d.ldSpec, d.numFilters, d.usePower) == (10, 3, 9, 32, 5, 0)


def test_model_equals_oracle_under_every_chunking(oracle):
    rng = np.random.default_rng(1)
    fe = toy_mfsc()
    for T in range(1, 15):
        x = rng.normal(size=T) * 3000.0
        want = oracle.mfsc(x, **TOY)
        assert want.shape == (fe.num_frames(T), TOY["num_filters"])
        if T >= 10:
            assert np.abs(want).max() > 1.0   # above the mel floor: the comparison sees the arithmetic
        for chunks in R.compositions(T):
            got, counts, carries = R.stream_utterance(R.FeatModel(**TOY), x, chunks)
            assert got.shape == want.shape, (T, chunks)
            assert np.abs(got - want).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(want).max(initial=0.0)), (T, chunks)
            assert sum(counts) == fe.num_frames(T) and carries[-1] == 0


def _lib_stream(sess, slot, chunks, S):
    """drives one slot of a session through `chunks` by counts alone: (frames per step, carried samples after each step)"""
    counts, carries = [], []
    for i, c in enumerate(chunks):
        n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        n[slot], st[slot], fi[slot] = c, i == 0, i == len(chunks) - 1
        n_out = sess.counts(n, st, fi)
        assert all(n_out[s] == 0 for s in range(S) if s != slot)
        counts.append(int(n_out[slot]))
        carries.append(sess.slot_state(slot)[1])
    return counts, carries


def test_library_counts_equal_the_model_under_every_chunking():
    fe = toy_mfsc()
    sess = StreamingFeatures(fe, 2, 14)
    assert sess.max_out == R.max_out(14, 10, 3) == 5
    for T in range(1, 15):
        x = np.zeros(T)
        for chunks in R.compositions(T):
            _, counts, carries = R.stream_utterance(R.FeatModel(values=False, **TOY), x, chunks)
            got_counts, got_carries = _lib_stream(sess, T % 2, chunks, 2)
            assert got_counts == counts and got_carries == carries, (T, chunks)
            assert sess.slot_state(T % 2) == (False, 0)


def test_library_counts_random_sequences_slots_at_different_phases_and_reuse():
    rng = np.random.default_rng(2)
    fe = toy_mfsc()
    S, cmax = 3, 7
    sess = StreamingFeatures(fe, S, cmax)
    models = [R.FeatModel(values=False, **TOY) for _ in range(S)]
    left = [0] * S
    for step in range(600):
        n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for s in range(S):
            if not models[s].active or (step % 97 == 13 and s == 1):
                if models[s].active:       # reset mid-utterance, then reuse
                    sess.reset(s)
                    models[s].reset()
                    assert sess.slot_state(s) == (False, 0)
                if rng.random() < 0.5:     # idle this step
                    continue
                st[s] = 1
                left[s] = int(rng.integers(0, 40))
            n[s] = 0 if rng.random() < 0.3 else min(left[s], int(rng.integers(1, cmax + 1)))
            left[s] -= n[s]
            fi[s] = left[s] == 0 and rng.random() < 0.7
        want = [models[s].step(np.zeros(n[s]), bool(st[s]), bool(fi[s])).shape[0] for s in range(S)]
        got = sess.counts(n, st, fi)
        assert list(got) == want, step
        for s in range(S):
            assert sess.slot_state(s) == (models[s].active, models[s].carry()), (step, s)
            assert got[s] <= sess.max_out


@pytest.mark.parametrize("max_samples", [1, 159, 160, 161, 400, 5120])
def test_max_out_formula_16k(max_samples):
    fe = Mfsc(device="cpu")
    sess = StreamingFeatures(fe, 1, max_samples)
    assert sess.max_out == (400 - 1 + max_samples - 400) // 160 + 1 == R.max_out(max_samples, 400, 160)
    # the formula is tight: a full carry plus a full chunk yields exactly max_out frames
    mo, sb = C.c_int(0), C.c_size_t(0)
    assert _lib.lib().w2l_feat_session_query(C.byref(feat_desc(fe)), 1, max_samples, C.byref(mo), C.byref(sb)) == _lib.W2L_OK
    assert mo.value == sess.max_out and sb.value == sess.state_bytes and sb.value % 256 == 0
    assert sb.value >= 4 * 80 * sess.max_out + 2 * 4 * 399
    sess.counts([min(399, max_samples)], [1])
    while sess.slot_state(0)[1] < 399:
        assert sess.counts([min(399 - sess.slot_state(0)[1], max_samples)])[0] == 0
    assert sess.counts([max_samples])[0] == sess.max_out


def _desc(**over):
    d = dict(frameSize=400, frameStride=160, nbins=257, ldSpec=288, numFilters=80, usePower=0, melFloor=1.0)
    d.update(over)
    return _lib.FeatDesc(**d)


def _create(d, slots=1, max_samples=160):
    h = C.c_void_p(0)
    st = _lib.lib().w2l_feat_session_create(C.byref(d), slots, max_samples, C.byref(h))
    if h.value:
        _lib.lib().w2l_feat_session_destroy(h)
    return st, _lib.lib().w2l_host_last_error().decode()


@pytest.mark.parametrize("over,field", [
    (dict(frameSize=513, nbins=257), "frameSize"),
    (dict(nbins=258, ldSpec=288), "nbins"),
    (dict(numFilters=129), "numFilters"),
])
def test_geometries_beyond_the_kernel_are_unsupported_and_name_the_field(over, field):
    st, msg = _create(_desc(**over))
    assert st == _lib.W2L_EUNSUPPORTED and field in msg, (st, msg)


def test_the_bounds_themselves_are_accepted():
    assert _create(_desc(frameSize=512, frameStride=512, nbins=257, ldSpec=257, numFilters=128))[0] == _lib.W2L_OK
    assert _create(_desc(frameSize=1, frameStride=1, nbins=1, ldSpec=1, numFilters=1))[0] == _lib.W2L_OK


@pytest.mark.parametrize("over", [
    dict(frameSize=0), dict(frameSize=-4), dict(frameStride=0), dict(frameStride=401), dict(nbins=0), dict(ldSpec=256),
    dict(numFilters=0), dict(melFloor=0.0), dict(melFloor=-1.0), dict(melFloor=float("nan")),
])
def test_nonsense_geometries_are_invalid(over):
    assert _create(_desc(**over))[0] == _lib.W2L_EINVAL


def test_nonsense_session_sizes_are_invalid():
    assert _create(_desc(), slots=0)[0] == _lib.W2L_EINVAL
    assert _create(_desc(), max_samples=0)[0] == _lib.W2L_EINVAL
    assert _lib.lib().w2l_feat_session_create(None, 1, 160, C.byref(C.c_void_p(0))) == _lib.W2L_EINVAL
    assert _lib.lib().w2l_feat_session_create(C.byref(_desc()), 1, 160, None) == _lib.W2L_EINVAL


def test_refused_steps_leave_the_counts_alone():
    fe = toy_mfsc()
    sess = StreamingFeatures(fe, 2, 7)
    sess.counts([7, 0], [1, 0])
    before = [sess.slot_state(s) for s in range(2)]
    assert before == [(True, 7), (False, 0)]
    with pytest.raises(_lib.W2LInvalidArgument, match="is fed before it was started"):
        sess.counts([3, 2])
    with pytest.raises(_lib.W2LInvalidArgument, match="finishes before it was started"):
        sess.counts([3, 0], None, [0, 1])
    with pytest.raises(_lib.W2LInvalidArgument, match="outside 0..7"):
        sess.counts([8, 0])
    with pytest.raises(_lib.W2LInvalidArgument, match="outside 0..7"):
        sess.counts([3, -1], [0, 1])
    L = _lib.lib()
    assert L.w2l_feat_session_counts(sess.h, None, None, None, None) == _lib.W2L_EINVAL
    assert L.w2l_feat_session_counts(None, None, None, None, None) == _lib.W2L_EINVAL
    n = np.array([1, 0], np.int32)
    out, ptr = np.zeros(2, np.int32), C.c_void_p(0)
    # a step before bind, and null pointers: refused on the host, nothing moves
    assert L.w2l_feat_session_step(sess.h, 256, 0, n.ctypes.data, None, None, C.byref(ptr), out.ctypes.data, None) == _lib.W2L_EINVAL
    assert "bind" in L.w2l_host_last_error().decode()
    assert L.w2l_feat_session_step(sess.h, None, 0, n.ctypes.data, None, None, C.byref(ptr), out.ctypes.data, None) == _lib.W2L_EINVAL
    assert L.w2l_feat_session_step(sess.h, 256, 0, n.ctypes.data, None, None, C.byref(ptr), None, None) == _lib.W2L_EINVAL
    assert L.w2l_feat_session_step(sess.h, 256, 7, n.ctypes.data, None, None, C.byref(ptr), out.ctypes.data, None) == _lib.W2L_EINVAL
    assert L.w2l_feat_session_bind(sess.h, None, None, None, 0) == _lib.W2L_EINVAL
    assert L.w2l_feat_session_slot_state(sess.h, 2, None, None) == _lib.W2L_EINVAL
    assert L.w2l_feat_session_reset(sess.h, -1) == _lib.W2L_EINVAL
    assert [sess.slot_state(s) for s in range(2)] == before
    assert list(sess.counts([3, 0])) == [1, 0] and sess.slot_state(0) == (True, 7)   # 10 buffered: one frame, 3 consumed


def test_abi_names_are_declared_and_exported():
    names = {"w2l_feat_session_" + n for n in ("query", "create", "destroy", "max_out", "state_bytes", "bind", "counts", "step",
                                               "slot_state", "reset")} | {"w2l_feat_stream_frames", "w2l_feat_stream_tile_rows"}
    assert names <= set(_lib.exported_symbols())
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n), n
    assert L.w2l_feat_stream_tile_rows() == 16
    assert C.sizeof(_lib.FeatDesc) == 28
