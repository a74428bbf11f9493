"""Host-side tests of LocalNorm (include/w2l_hip.h w2l_local_norm / w2l_norm_session_*; no GPU): the reference's streaming recurrence
against the contract on the GPU tests' inputs, every refusal with its message (refusals come before anything touches the device, so
the device pointers here are made-up addresses), the size queries as arithmetic, the ABI, and the reference's flag files."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import local_norm_ref as R
from wav2letter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, WS = 1 << 20, 1 << 24, 1 << 28   # far apart, 256-byte aligned: never dereferenced


def err():
    return _lib.lib().w2l_host_last_error().decode()


# ---------------------------------------------------------------------------------------------- (b) against (a)
def test_reference_recurrence_against_the_contract():
    """reference() -- fp32 stored sums, a consumed list -- and contract() -- fp64 sums over lo..hi -- describe the same windows:
    they differ by the roundings of the fp32 sums alone.  The worst difference is the figure the GPU test's bar is four times of."""
    worst, where = 0.0, None
    for F, L, T, seed in R.cases():
        x = R.features(F, T, seed)
        a, _, _ = R.contract(x, L, 0)
        b = R.reference(x, L)
        d = float(np.abs(a.astype(np.float64) - b).max())
        if d > worst:
            worst, where = d, (F, L, T)
    print(f"reference vs contract: worst {worst:.4g} at (F, L, T) = {where}")
    assert worst <= R.REF_VS_CONTRACT_WORST, (worst, where)
    # what the bar is there to tell apart: a window one frame too long at the small contexts
    for L in (1, 2):
        x = R.features(80, 2 * L + 5, 7)
        off = np.abs(R.contract(x, L, 0)[0] - R.contract(x, L + 1, 0)[0]).max()
        assert off > 1000 * 4 * R.REF_VS_CONTRACT_WORST, off


def test_contract_window_edges():
    """right context, clipping at both ends, the eps rule"""
    x = R.features(3, 9, 1)
    y, mean, sd = R.contract(x, 2, 1)
    for t in range(9):
        w = x[:, max(0, t - 2):min(8, t + 1) + 1].astype(np.float64)
        assert abs(mean[t] - w.mean()) < 1e-12 and abs(sd[t] - w.std()) < 1e-12
    assert np.all(R.contract(np.full((3, 4), 2.5, np.float32), 1)[0] == 0.0)


# ---------------------------------------------------------------------------------------------- the batch call's refusals
def _batch(B=2, F=80, T=100, ldx=None, x=X, frames=None, left=3, right=0, ldy=None, y=Y, ws=WS):
    st = _lib.lib().w2l_local_norm(B, F, T, T if ldx is None else ldx, x, frames, left, right, T if ldy is None else ldy, y, ws, None)
    return st, err()


@pytest.mark.parametrize("over,word", [
    (dict(B=0), "positive"), (dict(F=0), "positive"), (dict(T=0), "positive"), (dict(B=-1), "positive"),
    (dict(left=-1), "negative"), (dict(right=-1), "negative"),
    (dict(ldx=99), "at least T"), (dict(ldy=99), "at least T"),
    (dict(x=None), "null"), (dict(y=None), "null"), (dict(ws=None), "null"),
    (dict(ws=WS + 8), "aligned"),
    (dict(y=X + 4), "overlap"),                     # shifted by one float
    (dict(y=X, ldy=101), "overlap"),                # the same start, another leading dimension
    (dict(y=X + 4 * (2 * 80 * 100 - 1)), "overlap"),   # the last float of x
])
def test_batch_refusals_are_invalid_arguments_with_a_message(over, word):
    st, msg = _batch(**over)
    assert st == _lib.W2L_EINVAL and word in msg and msg.startswith("local norm:"), (st, msg)


@pytest.mark.parametrize("over,word", [
    (dict(left=65536), "65537"), (dict(left=65000, right=536), "65537"), (dict(F=4097), "4097"),
])
def test_batch_sizes_beyond_the_kernel_are_unsupported(over, word):
    st, msg = _batch(**over)
    assert st == _lib.W2L_EUNSUPPORTED and word in msg, (st, msg)


def test_workspace_size_is_arithmetic():
    L = _lib.lib()
    for B, T in ((1, 1), (3, 605), (64, 1500)):
        assert L.w2l_local_norm_workspace_size(B, T) == 16 * B * T
    assert L.w2l_local_norm_workspace_size(0, 5) == 0 and L.w2l_local_norm_workspace_size(5, 0) == 0
    assert L.w2l_local_norm_workspace_size(65536, 65536) == 16 << 32


# ---------------------------------------------------------------------------------------------- the session
def _create(nfeat=80, slots=2, max_chunk=8, left=300, right=0):
    h = C.c_void_p(0)
    st = _lib.lib().w2l_norm_session_create(nfeat, slots, max_chunk, left, right, C.byref(h))
    return st, err(), h


def _query(nfeat, slots, max_chunk, left, right=0):
    sb = C.c_size_t(0)
    st = _lib.lib().w2l_norm_session_query(nfeat, slots, max_chunk, left, right, C.byref(sb))
    return st, sb.value


def test_a_right_context_is_refused_as_in_the_reference():
    st, msg, h = _create(right=1)
    assert st == _lib.W2L_EINVAL and not h.value and "LocalNorm.cpp:33" in msg and "right context 1" in msg, (st, msg)
    assert _query(80, 1, 8, 300, 2)[0] == _lib.W2L_EINVAL


@pytest.mark.parametrize("over", [dict(nfeat=0), dict(slots=0), dict(slots=65536), dict(max_chunk=0), dict(left=-1)])
def test_nonsense_session_sizes_are_invalid(over):
    st, msg, h = _create(**over)
    assert st == _lib.W2L_EINVAL and not h.value and msg.startswith("norm session:"), (st, msg)


@pytest.mark.parametrize("over,word", [(dict(left=65536), "65537"), (dict(nfeat=4097), "nfeat 4097"), (dict(max_chunk=65537), "maxChunk 65537")])
def test_session_sizes_beyond_the_kernel_are_unsupported(over, word):
    st, msg, h = _create(**over)
    assert st == _lib.W2L_EUNSUPPORTED and not h.value and word in msg, (st, msg)


@pytest.mark.parametrize("nfeat,slots,max_chunk,left", [(80, 1, 8, 300), (80, 16, 16, 300), (3, 3, 4, 0), (80, 64, 32, 65535), (1, 65535, 1, 0)])
def test_state_bytes_are_arithmetic(nfeat, slots, max_chunk, left):
    al = lambda v: (v + 255) // 256 * 256
    want = al(16 * slots) + al(16 * slots * (left + max_chunk))
    st, sb = _query(nfeat, slots, max_chunk, left)
    assert st == _lib.W2L_OK and sb == want
    st, _, h = _create(nfeat, slots, max_chunk, left)
    assert st == _lib.W2L_OK and _lib.lib().w2l_norm_session_state_bytes(h) == want
    _lib.lib().w2l_norm_session_destroy(h)
    assert _lib.lib().w2l_norm_session_state_bytes(None) == 0


def test_refused_steps_and_binds():
    L = _lib.lib()
    st, _, h = _create(nfeat=3, slots=2, max_chunk=4, left=2)
    assert st == _lib.W2L_OK
    try:
        n = lambda *v: np.array(v, np.int32)
        step = lambda x, ld, cnt, start, y, ldy: L.w2l_norm_session_step(h, x, ld, cnt.ctypes.data if cnt is not None else None,
                                                                         start.ctypes.data if start is not None else None, y, ldy, None)
        assert step(None, 4, n(1, 0), n(1, 0), Y, 4) == _lib.W2L_EINVAL and "null" in err()
        assert step(X, 4, n(1, 0), n(1, 0), None, 4) == _lib.W2L_EINVAL and "null" in err()
        assert step(X, 4, None, None, Y, 4) == _lib.W2L_EINVAL and "null" in err()
        assert step(X, 4, n(5, 0), n(1, 0), Y, 4) == _lib.W2L_EINVAL and "slot 0 was given 5 frames, outside 0..4" in err()
        assert step(X, 4, n(0, -1), n(1, 1), Y, 4) == _lib.W2L_EINVAL and "slot 1 was given -1 frames, outside 0..4" in err()
        assert step(X, 3, n(4, 0), n(1, 0), Y, 4) == _lib.W2L_EINVAL and "more than a row" in err()
        assert step(X, 4, n(4, 0), n(1, 0), Y, 3) == _lib.W2L_EINVAL and "more than a row" in err()
        assert step(X, 4, n(1, 2), n(1, 0), Y, 4) == _lib.W2L_EINVAL and "slot 1 is fed before it was started" in err()
        assert step(X, 4, n(1, 2), None, Y, 4) == _lib.W2L_EINVAL and "slot 0 is fed before it was started" in err()
        assert step(X, 4, n(1, 1), n(1, 1), X + 4, 4) == _lib.W2L_EINVAL and "overlap" in err()
        assert step(X, 4, n(1, 1), n(1, 1), X, 5) == _lib.W2L_EINVAL and "overlap" in err()
        # all in order, but nothing is bound -- in place included
        assert step(X, 4, n(1, 1), n(1, 1), Y, 4) == _lib.W2L_EINVAL and "bind" in err()
        assert step(X, 4, n(1, 1), n(1, 1), X, 4) == _lib.W2L_EINVAL and "bind" in err()
        act, fr = C.c_int(-1), C.c_longlong(-1)
        for s in range(2):   # no refused step opened a slot
            assert L.w2l_norm_session_slot_state(h, s, C.byref(act), C.byref(fr)) == _lib.W2L_OK and (act.value, fr.value) == (0, 0)
        sb = L.w2l_norm_session_state_bytes(h)
        assert L.w2l_norm_session_bind(h, None, sb) == _lib.W2L_EINVAL and "aligned" in err()
        assert L.w2l_norm_session_bind(h, X + 128, sb) == _lib.W2L_EINVAL and "aligned" in err()
        assert L.w2l_norm_session_bind(h, X, sb - 1) == _lib.W2L_EINVAL and "smaller" in err()
        assert L.w2l_norm_session_bind(None, X, sb) == _lib.W2L_EINVAL
        assert L.w2l_norm_session_slot_state(h, 2, None, None) == _lib.W2L_EINVAL
        assert L.w2l_norm_session_reset(h, -1) == _lib.W2L_EINVAL and L.w2l_norm_session_reset(h, 1) == _lib.W2L_OK
        assert L.w2l_norm_session_step(None, X, 4, None, None, Y, 4, None) == _lib.W2L_EINVAL
        assert L.w2l_norm_session_create(3, 1, 1, 0, 0, None) == _lib.W2L_EINVAL
    finally:
        L.w2l_norm_session_destroy(h)


def test_python_front_ends_refuse_on_the_host():
    import torch
    from wav2letter_amd.features import local_normalize
    from wav2letter_amd.loader import PrefetchLoader
    from wav2letter_amd.streaming import StreamingLocalNorm
    with pytest.raises(_lib.W2LInvalidArgument, match="LocalNorm.cpp:33"):
        StreamingLocalNorm(80, 1, 8, 300, right=2)
    with pytest.raises(_lib.W2LUnsupported, match="65537"):
        StreamingLocalNorm(80, 1, 8, 65536)
    sess = StreamingLocalNorm(80, 2, 8, 300)
    assert sess.state_bytes == 256 + 9984     # the table, then 16 x 2 x (300 + 8) = 9856 bytes of pairs to the next 256
    assert sess.slot_state(1) == (False, 0)
    with pytest.raises(_lib.W2LInvalidArgument, match="CUDA tensor"):
        sess.step(torch.zeros(2, 80, 8), [1, 1], [1, 1])
    with pytest.raises(_lib.W2LInvalidArgument, match="on the device"):
        local_normalize(torch.zeros(2, 80, 8), left=3)
    with pytest.raises(ValueError, match="negative"):
        PrefetchLoader.__new__(PrefetchLoader).__init__([], [], None, local_norm=(-1, 0))


def test_abi_names_are_declared_and_exported():
    names = {"w2l_norm_session_" + n for n in ("query", "create", "destroy", "state_bytes", "bind", "step", "slot_state", "reset")}
    names |= {"w2l_local_norm", "w2l_local_norm_workspace_size"}
    assert names <= set(_lib.exported_symbols())
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n) and hasattr(_lib._SIGS, n), n


def test_flags_check_still_accepts_every_reference_cfg():
    """the two context flags are ordinary --k=v lines of the streaming recipe's cfg; every flag file of the reference still loads"""
    import json
    from wav2letter_amd.trainer import flags_check
    with open(os.path.join(ROOT, "tests", "golden", "reference_recipes.json")) as f:
        cfgs = json.load(f)["cfg"]
    assert len(cfgs) >= 100
    for name, text in cfgs.items():
        assert flags_check(text) > 0, name
    streaming = [t for k, t in cfgs.items() if "500ms_future_context" in k]
    assert streaming and all("--localnrmlleftctx=300" in t for t in streaming)
    assert flags_check("--localnrmlleftctx=300\n--localnrmlrightctx=0\n") == 2
