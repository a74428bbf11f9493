"""Host tests of the split-bf16 GEMM surface (csrc/gemm_split.hpp): exported symbols, the refusals that come back before anything
touches the device, the switch's return value, and the mutual exclusion with the mixed-precision mode.  No GPU."""
import pytest
import torch

import stream_ref as R
from wav2letter_amd import _lib, ops
from wav2letter_amd import trainer as T

OK, EINVAL, EUNSUPPORTED = _lib.W2L_OK, _lib.W2L_EINVAL, _lib.W2L_EUNSUPPORTED


@pytest.mark.parametrize("kw,want", [(dict(A=None), EINVAL), (dict(B=None), EINVAL), (dict(Cp=None), EINVAL), (dict(M=0), EINVAL),
                                     (dict(N=-1), EINVAL), (dict(K=0), EINVAL), (dict(K=31), EUNSUPPORTED), (dict(K=1), EUNSUPPORTED)])
def test_refusals_precede_the_device(kw, want):
    """made-up addresses: a refused call never dereferences them"""
    a = {**dict(M=64, N=64, K=64, A=4096, B=8192, Cp=16384), **kw}
    L = _lib.lib()
    assert len(L.w2l_gemm_f32_split.argtypes) == 15       # the header's fifteen arguments
    assert L.w2l_gemm_f32_split(a["M"], a["N"], a["K"], a["A"], a["K"], 1, a["B"], a["N"], 0, a["Cp"], a["N"], None, 0, None, None) == want


def test_switches_and_the_exclusion_with_mixed_precision():
    L, Lt = _lib.lib(), T._lib_tr()
    for name in ("w2l_gemm_f32_split", "w2l_set_matmul_split", "w2l_trainer_set_split_precision"):
        assert hasattr(L, name) and name in _lib.exported_symbols(), name
    assert L.w2l_set_matmul_split(1) == 0 and L.w2l_set_matmul_split(7) == 1 and L.w2l_set_matmul_split(0) == 1   # the previous value
    with pytest.raises(ValueError):
        ops.gemm_split(torch.zeros(64, 64), torch.zeros(64, 64))          # CPU tensors
    tr = Lt.w2l_trainer_create(R.TINY_ARCH.encode(), R.NFEAT, R.NLABEL, b"ctc", 0, 0.0)
    assert tr
    try:
        assert Lt.w2l_trainer_set_split_precision(None, 1) == EINVAL and Lt.w2l_trainer_set_split_precision(tr, 1) == OK
        assert Lt.w2l_trainer_set_mixed_precision(tr, 1) == EINVAL and "exclude" in Lt.w2l_host_last_error().decode()
        assert Lt.w2l_trainer_set_mixed_precision(tr, 0) == OK            # switching the other one OFF is always fine
        assert Lt.w2l_trainer_set_split_precision(tr, 0) == OK and Lt.w2l_trainer_set_mixed_precision(tr, 1) == OK
        assert Lt.w2l_trainer_set_split_precision(tr, 1) == EINVAL and Lt.w2l_trainer_set_split_precision(tr, 0) == OK
    finally:
        Lt.w2l_trainer_destroy(tr)
    assert T.flags_check("--w2l_split_gemm=true\n") == 1
    with pytest.raises(ValueError):
        T.flags_check("--w2l_split_gemm=true\n--fl_amp_use_mixed_precision=true\n")
