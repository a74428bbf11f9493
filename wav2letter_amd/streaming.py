"""Chunked streaming forward (wav2letter_amd/csrc/host/stream.cpp, csrc/stream.hip).

A StreamingSession runs a trained network on audio as it arrives: `slots` concurrent streams, at most `max_chunk` input
frames per slot and step.  For any utterance and any split of it into chunks the concatenated emissions equal
Trainer.forward(train=False) of that utterance alone (fp32 parity), and the frame count equals its Tout.  Feature extraction
and normalisation stay with the caller.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib


def _check(st, what):
    if st == _lib.W2L_OK:
        return
    msg = f"{what}: {_lib.lib().w2l_host_last_error().decode()}"
    if st == _lib.W2L_EINVAL:
        raise _lib.W2LInvalidArgument(msg)
    if st == _lib.W2L_EUNSUPPORTED:
        raise _lib.W2LUnsupported(msg)
    raise _lib.W2LError(msg)


def query(arch_text, nfeat, nlabel, slots, max_chunk):
    """(max_out, state_bytes) of a session over this arch: host arithmetic, no device"""
    mo, sb = C.c_int(0), C.c_size_t(0)
    _check(_lib.lib().w2l_stream_query(arch_text.encode(), nfeat, nlabel, slots, max_chunk, C.byref(mo), C.byref(sb)), "stream query")
    return mo.value, sb.value


def _flags(v, S, what):
    if v is None:
        return np.zeros(S, np.int32)
    a = np.ascontiguousarray(np.asarray(v).astype(np.int32))
    if a.shape != (S,):
        raise _lib.W2LInvalidArgument(f"{what}: one value per slot ({S}), got shape {a.shape}")
    return a


class StreamingSession:
    """StreamingSession(trainer, slots, max_chunk): the trainer's arch, its parameter arena (trainer.params: to_device() first;
    read at every step, so further training shows).  StreamingSession.from_arch(...) takes an arch text and a parameter tensor in
    the trainer's arena layout instead.  Creation is host arithmetic (a non-streamable arch line raises W2LUnsupported naming the
    line); the device state is allocated at the first step."""

    def __init__(self, trainer, slots, max_chunk, device=None):
        L = _lib.lib()
        h = C.c_void_p(0)
        _check(L.w2l_stream_create_for_trainer(trainer.h, int(slots), int(max_chunk), C.byref(h)), "streaming session")
        self._init(L, h, trainer.nfeat, trainer.nlabel, slots, max_chunk, device or trainer.device)
        self._trainer = trainer   # kept alive: the C session reads it

    @classmethod
    def from_arch(cls, arch_text, nfeat, nlabel, params, slots, max_chunk, device="cuda"):
        L = _lib.lib()
        h = C.c_void_p(0)
        _check(L.w2l_stream_create(arch_text.encode(), int(nfeat), int(nlabel), int(slots), int(max_chunk), C.byref(h)), "streaming session")
        self = cls.__new__(cls)
        self._init(L, h, nfeat, nlabel, slots, max_chunk, device)
        self._trainer = None
        if params is not None:
            if not (torch.is_tensor(params) and params.dtype == torch.float32 and params.is_contiguous()
                    and params.numel() >= self.param_floats):
                raise _lib.W2LInvalidArgument(f"params: contiguous float32 tensor of {self.param_floats} floats (the trainer's arena)")
        self._params = params
        return self

    def _init(self, L, h, nfeat, nlabel, slots, max_chunk, device):
        self.L, self.h = L, h
        self.nfeat, self.nlabel, self.slots, self.max_chunk = int(nfeat), int(nlabel), int(slots), int(max_chunk)
        self.device = device
        self.max_out = L.w2l_stream_max_out(h)
        self.state_bytes = L.w2l_stream_state_bytes(h)
        self.param_floats = L.w2l_stream_param_floats(h)
        self.num_time_layers = L.w2l_stream_num_time_layers(h)
        self._params = None
        self._state = None
        self._none = None

    def __del__(self):
        try:
            if self.h:
                self.L.w2l_stream_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _bind(self):
        params = self._params
        if params is None and self._trainer is not None:
            params = self._trainer.params
        if params is None:
            raise _lib.W2LInvalidArgument("streaming session: no parameters on the device (trainer.to_device() first)")
        self._bound_params = params
        self._state = torch.empty(max(self.state_bytes, 256), dtype=torch.uint8, device=params.device)
        _check(self.L.w2l_stream_bind(self.h, params.data_ptr(), self._state.data_ptr(), self._state.numel()), "stream bind")

    def counts(self, counts, start=None, finish=None):
        """the integer bookkeeping of a step alone (host arithmetic; advances the session's counts as a step would): n_out [S]"""
        S = self.slots
        n, st, fi = _flags(counts, S, "counts"), _flags(start, S, "start"), _flags(finish, S, "finish")
        n_out = np.zeros(S, np.int32)
        _check(self.L.w2l_stream_counts(self.h, n.ctypes.data, st.ctypes.data, fi.ctypes.data, n_out.ctypes.data), "stream counts")
        return n_out

    def slot_state(self, slot):
        """(active, carry frames of each time-extent layer) of a slot: host state"""
        act = C.c_int(0)
        carry = np.zeros(max(self.num_time_layers, 1), np.int32)
        _check(self.L.w2l_stream_slot_state(self.h, int(slot), C.byref(act), carry.ctypes.data, self.num_time_layers), "stream slot state")
        return bool(act.value), carry[:self.num_time_layers].copy()

    def step(self, x, counts, start=None, finish=None):
        """x: [S][NFEAT][max_chunk] float32 on the device, the first counts[s] columns of slot s are used; counts / start /
        finish: one int per slot on the host.  Returns (out, n_out): out [S][max_out][NLABEL] is a view of the session's state,
        valid until the next step, whose rows [0, n_out[s]) of slot s are that slot's new emission frames; n_out is a numpy
        int32 array computed on the host -- the step does not synchronise."""
        S = self.slots
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
                and tuple(x.shape) == (S, self.nfeat, self.max_chunk)):
            raise _lib.W2LInvalidArgument(
                f"input must be a contiguous float32 CUDA tensor [S={S}][NFEAT={self.nfeat}][max_chunk={self.max_chunk}], got "
                f"{tuple(x.shape) if torch.is_tensor(x) else type(x)}")
        n, st, fi = _flags(counts, S, "counts"), _flags(start, S, "start"), _flags(finish, S, "finish")
        if self._state is None:
            self._bind()
        n_out = np.zeros(S, np.int32)
        ptr = C.c_void_p(0)
        _check(self.L.w2l_stream_step(self.h, x.data_ptr(), n.ctypes.data, st.ctypes.data, fi.ctypes.data, C.byref(ptr),
                                      n_out.ctypes.data, torch.cuda.current_stream().cuda_stream), "stream step")
        numel = S * self.max_out * self.nlabel
        if not ptr.value:   # no slot had work
            if self._none is None:
                self._none = torch.zeros(S, self.max_out, self.nlabel, dtype=torch.float32, device=x.device)
            return self._none, n_out
        off = ptr.value - self._state.data_ptr()
        return self._state[off:off + 4 * numel].view(torch.float32).view(S, self.max_out, self.nlabel), n_out

    def reset(self, slot):
        """closes a slot and discards its state"""
        _check(self.L.w2l_stream_reset(self.h, int(slot)), "stream reset")
