"""Host tests of w2l_gemm_bf16_smallm (csrc/gemm_smallm.hip) and of the precision-carrying session calls (w2l_stream_*_ex,
csrc/host/stream.cpp): refusals that come back before anything touches the device, the pure-host queries, the exported symbols,
and the count bookkeeping, which does not depend on the precision.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import stream_ref as R
from wav2letter_amd import _lib, streaming

OK, EINVAL, EUNSUPPORTED = _lib.W2L_OK, _lib.W2L_EINVAL, _lib.W2L_EUNSUPPORTED
FP32, BF16 = 0, 1
NEW_SYMBOLS = ["w2l_gemm_bf16_smallm", "w2l_gemm_bf16_smallm_max_m", "w2l_gemm_bf16_smallm_workspace_bytes", "w2l_stream_create_ex",
               "w2l_stream_create_for_trainer_ex", "w2l_stream_query_ex", "w2l_stream_refresh_weights"]


class Sink(C.Structure):
    _fields_ = [("rowMajor", C.c_void_p), ("ldRows", C.c_size_t), ("transposed", C.c_void_p), ("ldTrans", C.c_size_t)]


def call(M=4, N=40, K=200, A=4096, lda=256, B=8192, ldb=256, Cp=16384, ldc=40, bias=None, relu=0, addend=None, image=None, ws=1 << 20,
         ws_bytes=1 << 30):
    """the pointers are made-up addresses (16-byte aligned): a call that is refused never dereferences them"""
    return _lib.lib().w2l_gemm_bf16_smallm(M, N, K, A, lda, B, ldb, Cp, ldc, bias, relu, addend, C.byref(image) if image else None, ws,
                                           ws_bytes, None)


def test_new_symbols_are_exported_and_declared():
    L = _lib.lib()
    declared = set(_lib.exported_symbols())
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in declared, name
    assert streaming.FP32 == FP32 and streaming.BF16 == BF16


def test_cap_query():
    assert _lib.lib().w2l_gemm_bf16_smallm_max_m() >= 1024


@pytest.mark.parametrize("kw", [dict(A=None), dict(B=None), dict(Cp=None), dict(M=0), dict(M=-3), dict(N=0), dict(K=0), dict(K=-1),
                                dict(lda=192), dict(ldb=199), dict(lda=8), dict(ldc=39)])
def test_bad_arguments_are_einval(kw):
    assert call(**kw) == EINVAL


def test_m_above_the_cap_is_unsupported():
    cap = _lib.lib().w2l_gemm_bf16_smallm_max_m()
    assert call(M=cap + 1) == EUNSUPPORTED
    assert call(M=1 << 20) == EUNSUPPORTED
    assert call(M=cap + 1, A=None) == EINVAL   # a bad argument stays a bad argument


def test_image_sink_rules():
    assert call(image=Sink(4096, 64, 8192, 64)) == EINVAL            # a transposed image is refused
    assert call(Cp=None, image=Sink(None, 64, None, 0)) == EINVAL    # neither C nor a row image
    assert call(image=Sink(4096, 32, None, 0)) == EINVAL             # row image narrower than N


def test_workspace_query_is_pure_host_and_monotone():
    L = _lib.lib()
    q = L.w2l_gemm_bf16_smallm_workspace_bytes
    assert q(0, 40, 200) == 0 and q(4, 0, 200) == 0 and q(4, 40, 0) == 0
    for K in (8, 200, 2160, 6480):
        for M in (1, 33, 144, 1024):
            prev = 0
            for N in range(1, 1400):
                b = q(M, N, K)
                assert b >= prev, (M, N, K, b, prev)
                prev = b
            assert q(M + 1, 1200, K) >= q(M, 1200, K)
    assert q(144, 1200, 6480) == q(144, 1200, 6480)


# ---------------------------------------------------------------------------------------------- the _ex session calls
def _create(precision, slots=2, chunk=8):
    h = C.c_void_p(0)
    st = _lib.lib().w2l_stream_create_ex(R.TINY_ARCH.encode(), R.NFEAT, R.NLABEL, slots, chunk, precision, C.byref(h))
    return st, h


def test_ex_fp32_equals_the_old_calls():
    L = _lib.lib()
    for S, c in ((1, 4), (2, 8), (3, 17)):
        mo, sb = C.c_int(0), C.c_size_t(0)
        assert L.w2l_stream_query(R.TINY_ARCH.encode(), R.NFEAT, R.NLABEL, S, c, C.byref(mo), C.byref(sb)) == OK
        mo2, sb2 = C.c_int(0), C.c_size_t(0)
        assert L.w2l_stream_query_ex(R.TINY_ARCH.encode(), R.NFEAT, R.NLABEL, S, c, FP32, C.byref(mo2), C.byref(sb2)) == OK
        assert (mo.value, sb.value) == (mo2.value, sb2.value)
        st, h = _create(FP32, S, c)
        assert st == OK and h.value
        assert L.w2l_stream_max_out(h) == mo.value and L.w2l_stream_state_bytes(h) == sb.value
        L.w2l_stream_destroy(h)
        mo3, sb3 = streaming.query(R.TINY_ARCH, R.NFEAT, R.NLABEL, S, c, mixed_precision=True)
        assert mo3 == mo.value and sb3 > sb.value   # the parameter snapshot rides in a bf16 session's state
    st, h = _create(7)
    assert st == EINVAL and not h.value


def test_ex_over_a_trainer():
    L = _lib.lib()
    from wav2letter_amd import trainer as T
    Lt = T._lib_tr()
    tr = Lt.w2l_trainer_create(R.TINY_ARCH.encode(), R.NFEAT, R.NLABEL, b"ctc", 0, 0.0)
    assert tr
    try:
        h = C.c_void_p(0)
        assert L.w2l_stream_create_for_trainer_ex(tr, 2, 8, FP32, C.byref(h)) == OK and h.value
        L.w2l_stream_destroy(h)
        h = C.c_void_p(0)
        assert L.w2l_stream_create_for_trainer_ex(tr, 2, 8, BF16, C.byref(h)) == EINVAL and not h.value   # an fp32 trainer
        assert "mixed-precision" in L.w2l_host_last_error().decode()
        Lt.w2l_trainer_set_mixed_precision(tr, 1)
        assert L.w2l_stream_create_for_trainer_ex(tr, 2, 8, FP32, C.byref(h)) == EUNSUPPORTED and not h.value
        assert L.w2l_stream_create_for_trainer(tr, 2, 8, C.byref(h)) == EUNSUPPORTED and not h.value     # the old call, as ever
        assert L.w2l_stream_create_for_trainer_ex(tr, 2, 8, BF16, C.byref(h)) == OK and h.value
        assert L.w2l_stream_refresh_weights(h) == OK
        L.w2l_stream_destroy(h)
        assert Lt.w2l_trainer_set_mixed_precision_convs(tr, 1) == OK
        h = C.c_void_p(0)
        assert L.w2l_stream_create_for_trainer_ex(tr, 2, 8, BF16, C.byref(h)) == EUNSUPPORTED and not h.value
        assert "set_mixed_precision_convs" in L.w2l_host_last_error().decode()
    finally:
        Lt.w2l_trainer_destroy(tr)


def test_refresh_weights_on_unbound_and_fp32_sessions():
    L = _lib.lib()
    for precision in (FP32, BF16):
        st, h = _create(precision)
        assert st == OK
        assert L.w2l_stream_refresh_weights(h) == OK
        L.w2l_stream_destroy(h)
    assert L.w2l_stream_refresh_weights(None) == EINVAL
    sess = streaming.StreamingSession.from_arch(R.TINY_ARCH, R.NFEAT, R.NLABEL, None, 2, 8, mixed_precision=True)
    assert sess.mixed_precision
    sess.refresh_weights()


def test_counts_do_not_depend_on_the_precision():
    S, cmax = 3, 17
    a = streaming.StreamingSession.from_arch(R.TINY_ARCH, R.NFEAT, R.NLABEL, None, S, cmax)
    b = streaming.StreamingSession.from_arch(R.TINY_ARCH, R.NFEAT, R.NLABEL, None, S, cmax, mixed_precision=True)
    assert (a.max_out, a.num_time_layers, a.param_floats) == (b.max_out, b.num_time_layers, b.param_floats)
    rng = np.random.default_rng(5)
    for _ in range(4):
        plans = [R.random_chunking(rng, int(rng.integers(1, 65)), cmax) for _ in range(S)]
        for i in range(max(len(p) for p in plans)):
            n = np.array([p[i] if i < len(p) else 0 for p in plans], np.int32)
            st = np.array([i == 0 for p in plans], np.int32)
            fi = np.array([i == len(p) - 1 for p in plans], np.int32)
            assert (a.counts(n, st, fi) == b.counts(n, st, fi)).all()
            for s in range(S):
                sa, sb = a.slot_state(s), b.slot_state(s)
                assert sa[0] == sb[0] and (sa[1] == sb[1]).all()
