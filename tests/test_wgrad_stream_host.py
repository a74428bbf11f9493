"""CPU side of the weight-gradient stream switch (w2l_trainer_set_weight_grad_stream): declared, exported, host-only."""
from wav2letter_amd import _lib
from wav2letter_amd import trainer as T

NAME = "w2l_trainer_set_weight_grad_stream"
ARCH = "V -1 NFEAT 1 0\nTDS 1 5 8 0.1 0\nV 0 8 1 0\nRO 1 0 3 2\nL 8 NLABEL\n"


def test_symbol_is_declared_and_exported():
    assert NAME in _lib.exported_symbols()
    assert hasattr(_lib.lib(), NAME)
    assert callable(getattr(T.Trainer, "set_weight_grad_stream"))


def test_null_handle_is_rejected_without_touching_the_gpu():
    Lt = T._lib_tr()
    assert Lt.w2l_trainer_set_weight_grad_stream(None, 1) == _lib.W2L_EINVAL
    assert Lt.w2l_trainer_set_weight_grad_stream(None, 0) == _lib.W2L_EINVAL


def test_setter_is_host_only():
    """on an unplanned, unbound trainer, on a machine that may have no GPU at all: the stream itself is created by a backward"""
    Lt = T._lib_tr()
    h = Lt.w2l_trainer_create(ARCH.encode(), 8, 5, b"ctc", 0, 0.0)
    assert h, Lt.w2l_host_last_error().decode()
    try:
        assert Lt.w2l_trainer_set_weight_grad_stream(h, 0) == _lib.W2L_OK
        assert Lt.w2l_trainer_set_weight_grad_stream(h, 1) == _lib.W2L_OK
    finally:
        Lt.w2l_trainer_destroy(h)
