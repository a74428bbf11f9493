"""Chunked streaming forward (wav2letter_amd/csrc/host/stream.cpp, csrc/stream.hip).

A StreamingSession runs a trained network on audio as it arrives: `slots` concurrent streams, at most `max_chunk` input
frames per slot and step.  For any utterance and any split of it into chunks the concatenated emissions equal
Trainer.forward(train=False) of that utterance alone (fp32 parity), and the frame count equals its Tout.  StreamingFeatures
(below) is the feature extraction, StreamingLocalNorm the windowed normalisation between the two (csrc/local_norm.hip,
csrc/host/norm_stream.cpp): features.local_normalize(left, right = 0) frame by frame, bit for bit under any chunking.

mixed_precision=True makes it a bf16 session over a mixed-precision trainer (Trainer.set_mixed_precision): bf16 operands for the
fl::Linear products and the TDS convolutions, everything else fp32, equal to the trainer's own mixed-precision eval forward within
the mixed-precision bar (2e-3).  Such a session holds a SNAPSHOT of the model: it copies the parameters and writes the bf16 weight
images at its first step, and shows later changes of the parameters only after refresh_weights() -- unlike an fp32 session over a
trainer, which reads the trainer's live arena at every step.

A StreamingDecoder (csrc/criterion_beam_stream.hpp) is the CTC beam search continued chunk by chunk over such emissions: it
takes StreamingSession.step's output directly, and its result after any number of frames is, bit for bit, ctc_beam_search of
those frames alone.

StreamingFeatures (csrc/host/feat_stream.cpp, csrc/feat_stream.hip) is the front of that chain: PCM chunks in, features.Mfsc's
log-mel frames out, one launch per step, the same frames bit for bit however the audio was chunked.  Its step() output is what
StreamingSession.step takes when max_chunk == StreamingFeatures.max_out.
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


FP32, BF16 = 0, 1   # W2L_STREAM_FP32 / W2L_STREAM_BF16


def query(arch_text, nfeat, nlabel, slots, max_chunk, mixed_precision=False):
    """(max_out, state_bytes) of a session over this arch: host arithmetic, no device"""
    mo, sb = C.c_int(0), C.c_size_t(0)
    _check(_lib.lib().w2l_stream_query_ex(arch_text.encode(), nfeat, nlabel, slots, max_chunk, BF16 if mixed_precision else FP32,
                                          C.byref(mo), C.byref(sb)), "stream query")
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
    line); the device state is allocated at the first step.  mixed_precision=True: a bf16 session (the trainer's mixed-precision
    mode must be on); it reads the parameters at its first step and again only after refresh_weights()."""

    def __init__(self, trainer, slots, max_chunk, device=None, mixed_precision=False):
        L = _lib.lib()
        h = C.c_void_p(0)
        _check(L.w2l_stream_create_for_trainer_ex(trainer.h, int(slots), int(max_chunk), BF16 if mixed_precision else FP32, C.byref(h)),
               "streaming session")
        self._init(L, h, trainer.nfeat, trainer.nlabel, slots, max_chunk, device or trainer.device)
        self.mixed_precision = bool(mixed_precision)
        self._trainer = trainer   # kept alive: the C session reads it

    @classmethod
    def from_arch(cls, arch_text, nfeat, nlabel, params, slots, max_chunk, device="cuda", mixed_precision=False):
        L = _lib.lib()
        h = C.c_void_p(0)
        _check(L.w2l_stream_create_ex(arch_text.encode(), int(nfeat), int(nlabel), int(slots), int(max_chunk),
                                      BF16 if mixed_precision else FP32, C.byref(h)), "streaming session")
        self = cls.__new__(cls)
        self._init(L, h, nfeat, nlabel, slots, max_chunk, device)
        self.mixed_precision = bool(mixed_precision)
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

    def refresh_weights(self):
        """a bf16 session: the next step copies the parameters and writes the bf16 weight images again (host only; a no-op for fp32)"""
        _check(self.L.w2l_stream_refresh_weights(self.h), "stream refresh weights")


PCM_F32, PCM_S16 = 0, 1   # W2L_PCM_F32 / W2L_PCM_S16


def feat_desc(mfsc):
    """the w2l_feat_desc of a features.Mfsc"""
    return _lib.FeatDesc(frameSize=mfsc.N, frameStride=mfsc.S, nbins=mfsc.nb, ldSpec=mfsc.ld, numFilters=mfsc.F,
                         usePower=int(mfsc.use_power), melFloor=mfsc.floor)


class StreamingFeatures:
    """StreamingFeatures(mfsc, slots, max_samples): features.Mfsc on audio as it arrives (the contract is in include/w2l_hip.h,
    w2l_feat_session_*).  `slots` concurrent streams, at most max_samples new samples per slot and step; the session uses the
    Mfsc's own tables (mfsc.G, mfsc.H) and geometry.  A slot buffers what does not fill a frame yet (fewer than mfsc.N samples);
    finish drops that rest, as Mfsc drops the same tail of a whole utterance.  No normalisation.  Creation is host arithmetic
    (geometries beyond the kernel's bounds raise W2LUnsupported naming the field); the device state is allocated at the first
    step."""

    def __init__(self, mfsc, slots, max_samples):
        self.L = _lib.lib()
        self.mfsc = mfsc   # kept alive: the session reads its tables
        self.slots, self.max_samples, self.nfeat = int(slots), int(max_samples), int(mfsc.F)
        self._desc = feat_desc(mfsc)
        self.h = C.c_void_p(0)
        _check(self.L.w2l_feat_session_create(C.byref(self._desc), self.slots, self.max_samples, C.byref(self.h)), "streaming features")
        self.max_out = self.L.w2l_feat_session_max_out(self.h)
        self.state_bytes = self.L.w2l_feat_session_state_bytes(self.h)
        self._state = None
        self.feats = None   # the view step() returned last

    def __del__(self):
        try:
            if self.h:
                self.L.w2l_feat_session_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _bind(self):
        G, H = self.mfsc.G, self.mfsc.H
        if not (G.is_cuda and H.is_cuda and G.is_contiguous() and H.is_contiguous()):
            raise _lib.W2LInvalidArgument("streaming features: the Mfsc's tables must be contiguous and on the device")
        self._state = torch.empty(max(self.state_bytes, 256), dtype=torch.uint8, device=G.device)
        _check(self.L.w2l_feat_session_bind(self.h, G.data_ptr(), H.data_ptr(), self._state.data_ptr(), self._state.numel()),
               "streaming features bind")

    def counts(self, counts, start=None, finish=None):
        """the integer bookkeeping of a step alone (host arithmetic; advances the session's counts as a step would): n_out [S]"""
        S = self.slots
        n, st, fi = _flags(counts, S, "counts"), _flags(start, S, "start"), _flags(finish, S, "finish")
        n_out = np.zeros(S, np.int32)
        _check(self.L.w2l_feat_session_counts(self.h, n.ctypes.data, st.ctypes.data, fi.ctypes.data, n_out.ctypes.data),
               "streaming features counts")
        return n_out

    def slot_state(self, slot):
        """(active, carried samples) of a slot: host state"""
        act, carry = C.c_int(0), C.c_int(0)
        _check(self.L.w2l_feat_session_slot_state(self.h, int(slot), C.byref(act), C.byref(carry)), "streaming features slot state")
        return bool(act.value), carry.value

    def step(self, pcm, counts, start=None, finish=None):
        """pcm: [S][max_samples] float32 or int16 (scaled by 1 / 32768) on the device, the first counts[s] samples of slot s are
        used; counts / start / finish: one int per slot on the host.  Returns (feats, n_out): feats [S][NFEAT][max_out] is a view
        of the session's state, valid until the next step, whose columns [0, n_out[s]) of slot s are that slot's new frames (the
        columns beyond keep what they held); n_out is a numpy int32 array computed on the host -- the step does not synchronise."""
        S = self.slots
        if not (torch.is_tensor(pcm) and pcm.is_cuda and pcm.dtype in (torch.float32, torch.int16) and pcm.is_contiguous()
                and tuple(pcm.shape) == (S, self.max_samples)):
            raise _lib.W2LInvalidArgument(
                f"pcm must be a contiguous float32 or int16 CUDA tensor [S={S}][max_samples={self.max_samples}], got "
                f"{(tuple(pcm.shape), pcm.dtype) if torch.is_tensor(pcm) else type(pcm)}")
        n, st, fi = _flags(counts, S, "counts"), _flags(start, S, "start"), _flags(finish, S, "finish")
        if self._state is None:
            self._bind()
        n_out = np.zeros(S, np.int32)
        ptr = C.c_void_p(0)
        _check(self.L.w2l_feat_session_step(self.h, pcm.data_ptr(), PCM_S16 if pcm.dtype == torch.int16 else PCM_F32, n.ctypes.data,
                                            st.ctypes.data, fi.ctypes.data, C.byref(ptr), n_out.ctypes.data,
                                            torch.cuda.current_stream().cuda_stream), "streaming features step")
        off = ptr.value - self._state.data_ptr()
        numel = S * self.nfeat * self.max_out
        self.feats = self._state[off:off + 4 * numel].view(torch.float32).view(S, self.nfeat, self.max_out)
        return self.feats, n_out

    def reset(self, slot):
        """closes a slot and discards its carry"""
        _check(self.L.w2l_feat_session_reset(self.h, int(slot)), "streaming features reset")


class StreamingLocalNorm:
    """StreamingLocalNorm(nfeat, slots, max_chunk, left): features.local_normalize(..., left=left, right=0) on frames as they
    arrive, the reference's streaming LocalNorm between the features and the network (the contract is in include/w2l_hip.h,
    w2l_norm_session_*).  `slots` concurrent streams, at most max_chunk new frames per slot and step; however an utterance's frames
    are split into chunks, the concatenated output is local_normalize of the whole utterance, bit for bit.  Creation is host
    arithmetic; the device state (16 bytes per slot and frame of left + max_chunk) is allocated at the first step."""

    def __init__(self, nfeat, slots, max_chunk, left, right=0):
        self.L = _lib.lib()
        self.nfeat, self.slots, self.max_chunk, self.left = int(nfeat), int(slots), int(max_chunk), int(left)
        self.h = C.c_void_p(0)
        _check(self.L.w2l_norm_session_create(self.nfeat, self.slots, self.max_chunk, self.left, int(right), C.byref(self.h)),
               "streaming local norm")
        self.state_bytes = self.L.w2l_norm_session_state_bytes(self.h)
        self._state = None

    def __del__(self):
        try:
            if self.h:
                self.L.w2l_norm_session_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def slot_state(self, slot):
        """(active, frames since the start) of a slot: host state"""
        act, frames = C.c_int(0), C.c_longlong(0)
        _check(self.L.w2l_norm_session_slot_state(self.h, int(slot), C.byref(act), C.byref(frames)), "streaming local norm slot state")
        return bool(act.value), frames.value

    def step(self, x, counts, start=None, out=None):
        """x: [S][NFEAT][ld] float32 on the device with a unit time stride and rows of one slot F * ld apart (StreamingFeatures.step's
        view is one), the first counts[s] columns of slot s are its new frames; counts / start: one int per slot on the host.
        out=None normalises in place and returns x; otherwise out is a tensor of x's kind (its ld may differ) and is returned.
        Columns at or beyond counts[s] are not written.  One launch, no synchronisation."""
        S, F = self.slots, self.nfeat
        y = x if out is None else out
        for name, t in (("x", x), ("out", y)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and tuple(t.shape[:2]) == (S, F)
                    and t.is_contiguous()):
                raise _lib.W2LInvalidArgument(
                    f"{name} must be a contiguous float32 CUDA tensor [S={S}][NFEAT={F}][ld], got "
                    f"{(tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t)}")
        n, st = _flags(counts, S, "counts"), _flags(start, S, "start")
        if self._state is None:
            self._state = torch.empty(max(self.state_bytes, 256), dtype=torch.uint8, device=x.device)
            _check(self.L.w2l_norm_session_bind(self.h, self._state.data_ptr(), self._state.numel()), "streaming local norm bind")
        _check(self.L.w2l_norm_session_step(self.h, x.data_ptr(), x.shape[2], n.ctypes.data, st.ctypes.data, y.data_ptr(), y.shape[2],
                                            torch.cuda.current_stream().cuda_stream), "streaming local norm step")
        return y

    def reset(self, slot):
        """closes a slot"""
        _check(self.L.w2l_norm_session_reset(self.h, int(slot)), "streaming local norm reset")


BEAM_PLAIN, BEAM_LM, BEAM_LEX = 0, 1, 2


class StreamingDecoder:
    """StreamingDecoder(slots, max_chunk, max_frames, nlabel, **options): an incremental criterion.ctc_beam_search (the contract is
    in include/w2l_hip.h, w2l_beam_session_*).  `slots` utterances in progress, at most max_chunk emission frames per slot and
    step, at most max_frames per utterance.  options: ctc_beam_search's beam, beam_token, threshold, log_add, normalize, lm,
    lm_weight, class_score, eos_score, lexicon, word_score; the variant is chosen as ctc_beam_search chooses its entry point (no
    lm: LM-free; lm: token LM; lm and lexicon: lexicon with a word LM).  beam and beam_token go up to 64; wide=True is refused:
    WideStreamingDecoder is the incremental form of the wide searches.  With max_chunk = StreamingSession.max_out, step() takes StreamingSession.step's (out, n_out) as they are.
    Creation is host arithmetic; the device state is allocated at the first step."""

    _create_fn, _bytes_fn = "w2l_beam_session_create", "w2l_beam_session_state_bytes"

    def __init__(self, slots, max_chunk, max_frames, nlabel, beam=64, beam_token=64, threshold=float("inf"), log_add=False,
                 normalize=None, lm=None, lm_weight=0.0, class_score=None, eos_score=0.0, lexicon=None, word_score=0.0, wide=False,
                 device="cuda"):
        if wide:
            raise _lib.W2LUnsupported("StreamingDecoder runs the narrow searches (beam up to 64); the wide searches are incremental "
                                      "as WideStreamingDecoder")
        N = int(nlabel)
        if lexicon is not None:
            if lm is None:
                raise _lib.W2LInvalidArgument("StreamingDecoder: lexicon needs lm, a model over the lexicon's words")
            if class_score is not None:
                raise _lib.W2LInvalidArgument("StreamingDecoder: class_score must be None with a lexicon")
            if lm.num_tokens != lexicon.num_words:
                raise _lib.W2LInvalidArgument(f"StreamingDecoder: the LM has {lm.num_tokens} words, the lexicon {lexicon.num_words}")
            if lexicon.num_tokens != N - 1:
                raise _lib.W2LInvalidArgument(f"StreamingDecoder: the lexicon has {lexicon.num_tokens} tokens, the emissions {N - 1}")
            variant = BEAM_LEX
        elif word_score != 0.0:
            raise _lib.W2LInvalidArgument("StreamingDecoder: word_score needs lexicon")
        elif lm is None:
            if lm_weight != 0.0 or class_score is not None or eos_score != 0.0:
                raise _lib.W2LInvalidArgument("StreamingDecoder: lm_weight, class_score and eos_score need lm")
            variant = BEAM_PLAIN
        else:
            if lm.num_tokens != N - 1:
                raise _lib.W2LInvalidArgument(f"StreamingDecoder: the LM has {lm.num_tokens} tokens, the emissions {N - 1}")
            if class_score is not None and not (torch.is_tensor(class_score) and class_score.dtype == torch.float32
                                                and class_score.numel() == N - 1):
                raise _lib.W2LInvalidArgument("StreamingDecoder: class_score must be float32 with one entry per token class")
            variant = BEAM_LM
        if normalize is None:
            normalize = bool(log_add)
        self.L = _lib.lib()
        self.slots, self.max_chunk, self.max_frames, self.nlabel = int(slots), int(max_chunk), int(max_frames), N
        self.beam, self.variant, self.device = int(beam), variant, device
        # the descriptor is checked here, on the host, with placeholders for the device tables (the check looks at presence only);
        # the session itself is created with the tables at the first step
        self._lm, self._lexicon, self._class_score = lm, lexicon, class_score
        self._opts = dict(beam=int(beam), beamToken=int(beam_token), threshold=float(threshold), logAdd=int(bool(log_add)),
                          normalize=int(bool(normalize)), lmHasEos=int(lm.has_eos) if lm is not None else 0, lmWeight=float(lm_weight),
                          eosScore=float(eos_score), wordScore=float(word_score))
        self.h = None
        self._state = None
        self._keep = ()
        self.state_bytes = 0
        self._done = None      # per slot: (labels, words) committed since its start; None before the first commit
        self._scratch = None   # commit's device scratch, allocated at the first commit
        self.live = None
        self._create(placeholders=True)

    def _desc(self, lm_ptr, lex_ptr, cs_ptr):
        return _lib.BeamSessionDesc(slots=self.slots, maxChunk=self.max_chunk, maxFrames=self.max_frames, N=self.nlabel, variant=self.variant,
                                    lm=lm_ptr, lexicon=lex_ptr, classScore=cs_ptr, **self._opts)

    def _create(self, placeholders):
        if placeholders:   # host only: any non-null value stands for a table that is given
            ptrs = (1 if self._lm is not None else None, 1 if self._lexicon is not None else None,
                    1 if self._class_score is not None else None)
        else:
            dev = self.device
            blob = self._lm.device_blob(dev) if self._lm is not None else None
            lex = self._lexicon.device_blob(dev) if self._lexicon is not None else None
            cs = self._class_score.contiguous() if self._class_score is not None else None
            if cs is not None and not cs.is_cuda:
                raise _lib.W2LInvalidArgument("StreamingDecoder: class_score must be on the device")
            self._keep = (blob, lex, cs)
            ptrs = tuple(t.data_ptr() if t is not None else None for t in self._keep)
        d = self._desc(*ptrs)
        h = C.c_void_p(0)
        _check(self._make(d, h), "streaming decoder")
        self.state_bytes = getattr(self.L, self._bytes_fn)(C.byref(d))
        if placeholders:
            self.L.w2l_beam_session_destroy(h)
        else:
            self.h = h

    def _make(self, d, h):
        return getattr(self.L, self._create_fn)(C.byref(d), C.byref(h))

    def __del__(self):
        try:
            if self.h:
                self.L.w2l_beam_session_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _bind(self, device):
        self.device = device
        if self.h is None:
            self._create(placeholders=False)
        self._state = torch.empty(max(self.state_bytes, 256), dtype=torch.uint8, device=device)
        _check(self.L.w2l_beam_session_bind(self.h, self._state.data_ptr(), self._state.numel()), "streaming decoder bind")

    def step(self, emissions, counts, start=None):
        """emissions: [S][max_chunk][NLABEL] float32 on the device, rows [0, counts[s]) of slot s are its new frames; counts /
        start: one int per slot on the host.  start[s]: the slot begins a new utterance before these frames.  Does not
        synchronise."""
        S = self.slots
        if not (torch.is_tensor(emissions) and emissions.is_cuda and emissions.dtype == torch.float32 and emissions.is_contiguous()
                and tuple(emissions.shape) == (S, self.max_chunk, self.nlabel)):
            raise _lib.W2LInvalidArgument(
                f"emissions must be a contiguous float32 CUDA tensor [S={S}][max_chunk={self.max_chunk}][NLABEL={self.nlabel}], got "
                f"{tuple(emissions.shape) if torch.is_tensor(emissions) else type(emissions)}")
        n, st = _flags(counts, S, "counts"), _flags(start, S, "start")
        if self._state is None:
            self._bind(emissions.device)
        _check(self.L.w2l_beam_session_step(self.h, emissions.data_ptr(), n.ctypes.data, st.ctypes.data,
                                            torch.cuda.current_stream().cuda_stream), "streaming decoder step")
        for s in np.nonzero(st)[0]:   # a slot that starts has committed nothing
            self._forget(int(s))

    def counts(self, counts, start=None):
        """the bookkeeping of a step alone (w2l_beam_session_counts): counts / start are checked as step() checks them and the
        slots' frame counts move as a step would move them; host arithmetic, nothing is enqueued (with an LM or a lexicon the
        session is made here, with its device tables).  For a caller that keeps the counts of frames fed elsewhere in step."""
        n, st = _flags(counts, self.slots, "counts"), _flags(start, self.slots, "start")
        if self.h is None:
            self._create(placeholders=False)
        _check(self.L.w2l_beam_session_counts(self.h, n.ctypes.data, st.ctypes.data), "streaming decoder counts")
        for s in np.nonzero(st)[0]:
            self._forget(int(s))

    def _forget(self, slot):
        if self._done is not None:
            self._done[slot] = (np.zeros(0, np.int32), np.zeros(0, np.int32))

    def committed(self, slot):
        """(labels, words) a slot has committed since its start, int32 numpy arrays (words is empty without a lexicon)"""
        if not 0 <= int(slot) < self.slots:
            raise _lib.W2LInvalidArgument(f"StreamingDecoder: no slot {slot}")
        if self._done is None:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        return self._done[int(slot)]

    def commit(self, slots=None):
        """Commits what can no longer change (w2l_beam_session_commit: the labels above the deepest common ancestor of all beam
        entries but its own) and compacts the slots' prefix tables, which gives back most of the max_frames budget.  slots: None =
        every started slot, else an iterable of slot numbers.  Returns a list with one (labels, words) pair of int32 numpy arrays
        per slot: what THIS call committed (empty for a slot that was not asked or had nothing).  The decoder keeps the total per
        slot (committed()); result() then returns tails, result(full=True) the whole rows.  Synchronises: the one call that does.
        self.live[s] is the node count of slot s's table after its last commit."""
        if self._state is None:
            self._bind(self.device)
        S, lex = self.slots, self.variant == BEAM_LEX
        if self._done is None:
            self._done = [(np.zeros(0, np.int32), np.zeros(0, np.int32)) for _ in range(S)]
            self.live = np.zeros(S, np.int32)
        flags = None
        if slots is not None:
            flags = np.zeros(S, np.int32)
            for s in slots:
                if not 0 <= int(s) < S:
                    raise _lib.W2LInvalidArgument(f"StreamingDecoder: no slot {s}")
                flags[int(s)] = 1
        if self._scratch is None:
            nbytes = self.L.w2l_beam_session_commit_bytes(self.h)
            self._scratch = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self._state.device)
        # no commit is longer than the labels a slot still holds: its frames less what it has committed
        max_len = max([1] + [self.frames(s) - len(self._done[s][0]) for s in range(S)])
        dev = self._state.device
        labels = torch.empty(S, max_len, dtype=torch.int32, device=dev)
        words = torch.empty(S, max_len, dtype=torch.int32, device=dev) if lex else None
        nl, nw, live = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        _check(self.L.w2l_beam_session_commit(self.h, flags.ctypes.data if flags is not None else None, self._scratch.data_ptr(),
                                              self._scratch.numel(), max_len, labels.data_ptr(), max_len,
                                              words.data_ptr() if lex else None, nl.ctypes.data, nw.ctypes.data, live.ctypes.data,
                                              torch.cuda.current_stream().cuda_stream), "streaming decoder commit")
        hl = labels.cpu().numpy() if nl.any() else None
        hw = words.cpu().numpy() if lex and nw.any() else None
        out = []
        for s in range(S):
            a = hl[s, :nl[s]].copy() if nl[s] else np.zeros(0, np.int32)
            b = hw[s, :nw[s]].copy() if lex and nw[s] else np.zeros(0, np.int32)
            out.append((a, b))
            if nl[s] or nw[s]:
                self._done[s] = (np.concatenate([self._done[s][0], a]), np.concatenate([self._done[s][1], b]))
        self.live = live
        return out

    def _full(self, slot_rows, lengths, done, width):
        """committed ++ tail for every live row of one field ([S][nbest][.]); empty rows (length -1) stay empty"""
        S, M, L = slot_rows.shape
        full = torch.full((S, M, width + L), -1, dtype=torch.int32, device=slot_rows.device)
        total = lengths.clone()
        for s in range(S):
            c = len(done[s])
            live = lengths[s] >= 0
            full[s, :, c:c + L] = slot_rows[s]
            if c:
                full[s, :, :c] = torch.from_numpy(done[s]).to(slot_rows.device)
                total[s] = torch.where(live, lengths[s] + c, lengths[s])
            full[s, ~live] = -1
        return full, total

    def result(self, nbest=1, max_len=None, max_words=None, full=False):
        """the tuple ctc_beam_search returns for this variant, one row block per slot ([S][nbest]...), for the frames fed so far;
        changes nothing.  max_len defaults to max_frames, max_words to max_len.  After commit() the rows are the TAILS behind the
        committed labels (and words); full=True returns the whole rows instead -- committed ++ tail, lengths and word counts with
        the committed totals added, labels / words as wide as the longest committed part plus max_len / max_words."""
        if full:
            r = self.result(nbest, max_len, max_words)
            if self._done is None or not any(len(d[0]) for d in self._done):
                return r
            r = list(r)
            r[0], r[1] = self._full(r[0], r[1], [d[0] for d in self._done], max(len(d[0]) for d in self._done))
            if self.variant == BEAM_LEX:
                r[4], r[5] = self._full(r[4], r[5], [d[1] for d in self._done], max(len(d[1]) for d in self._done))
            return tuple(r)
        if self._state is None:
            self._bind(self.device)
        S, nbest = self.slots, int(nbest)
        max_len = self.max_frames if max_len is None else int(max_len)
        if max_words is not None and self.variant != BEAM_LEX:
            raise _lib.W2LInvalidArgument("StreamingDecoder: max_words needs lexicon")
        max_words = max(max_len, 1) if max_words is None else int(max_words)
        dev, shape = self._state.device, (S, max(nbest, 1))
        labels = torch.empty(*shape, max(max_len, 1), dtype=torch.int32, device=dev)
        lengths = torch.empty(*shape, dtype=torch.int32, device=dev)
        scores = torch.empty(*shape, dtype=torch.float32, device=dev)
        lm_scores = torch.empty(*shape, dtype=torch.float32, device=dev)
        words = word_counts = None
        if self.variant == BEAM_LEX:
            words = torch.empty(*shape, max(max_words, 1), dtype=torch.int32, device=dev)
            word_counts = torch.empty(*shape, dtype=torch.int32, device=dev)
        _check(self.L.w2l_beam_session_result(self.h, nbest, max_len, labels.data_ptr(), lengths.data_ptr(), scores.data_ptr(),
                                              lm_scores.data_ptr(), max_words, words.data_ptr() if words is not None else None,
                                              word_counts.data_ptr() if word_counts is not None else None,
                                              torch.cuda.current_stream().cuda_stream), "streaming decoder result")
        if self.variant == BEAM_LEX:
            return labels, lengths, scores, lm_scores, words, word_counts
        if self.variant == BEAM_LM:
            return labels, lengths, scores, lm_scores
        return labels, lengths, scores

    def frames(self, slot):
        """emission frames fed to a slot since its start"""
        if not 0 <= int(slot) < self.slots:
            raise _lib.W2LInvalidArgument(f"StreamingDecoder: no slot {slot}")
        if self.h is None:
            return 0
        f = C.c_int(0)
        _check(self.L.w2l_beam_session_frames(self.h, int(slot), C.byref(f)), "streaming decoder frames")
        return f.value

    def reset(self, slot):
        """closes a slot"""
        if not 0 <= int(slot) < self.slots:
            raise _lib.W2LInvalidArgument(f"StreamingDecoder: no slot {slot}")
        if self.h is None:
            return
        _check(self.L.w2l_beam_session_reset(self.h, int(slot)), "streaming decoder reset")
        self._forget(int(slot))


class WideStreamingDecoder(StreamingDecoder):
    """WideStreamingDecoder(slots, max_chunk, max_frames, nlabel, **options): StreamingDecoder on the wide kernels, an incremental
    criterion.ctc_beam_search(..., wide=True) (the contract is in include/w2l_hip.h, w2l_beam_session_create_wide).  The arguments
    are StreamingDecoder's without `wide`; beam goes up to 1024, beam_token (after clipping to NLABEL - 1) up to 64.  The methods
    are StreamingDecoder's.  A slot's state grows with beam * max_frames (16 bytes per prefix-table edge, two edges per entry and
    frame): 64 MiB at beam 1024 and max_frames 4096."""

    _create_fn, _bytes_fn = "w2l_beam_session_create_wide", "w2l_beam_session_wide_state_bytes"

    def __init__(self, slots, max_chunk, max_frames, nlabel, beam=1024, beam_token=64, threshold=float("inf"), log_add=False,
                 normalize=None, lm=None, lm_weight=0.0, class_score=None, eos_score=0.0, lexicon=None, word_score=0.0, device="cuda"):
        super().__init__(slots, max_chunk, max_frames, nlabel, beam=beam, beam_token=beam_token, threshold=threshold, log_add=log_add,
                         normalize=normalize, lm=lm, lm_weight=lm_weight, class_score=class_score, eos_score=eos_score, lexicon=lexicon,
                         word_score=word_score, device=device)


class ManyTokenStreamingDecoder(StreamingDecoder):
    """ManyTokenStreamingDecoder(slots, max_chunk, max_frames, nlabel, **options): StreamingDecoder on the many-token kernels, an
    incremental criterion.ctc_beam_search(..., wide="mt") (the contract is in include/w2l_hip.h, w2l_beam_session_create_mt).  The
    arguments are StreamingDecoder's without `wide`, plus the silence score of ctc_beam_search: sil_token (None with a lexicon: the
    lexicon's silence token) and sil_score (0: the search without it, the same bytes; non-zero without any silence token is
    refused).  beam goes up to 8192, beam_token (after clipping to NLABEL - 1) up to 256: the streaming recipes' 500 / 100.  The
    methods are StreamingDecoder's; commit() needs beam <= 1024 (beyond, W2LUnsupported and nothing changed)."""

    _create_fn, _bytes_fn = "w2l_beam_session_create_mt", "w2l_beam_session_mt_state_bytes"

    def __init__(self, slots, max_chunk, max_frames, nlabel, beam=500, beam_token=100, threshold=float("inf"), log_add=False,
                 normalize=None, lm=None, lm_weight=0.0, class_score=None, eos_score=0.0, lexicon=None, word_score=0.0, sil_token=None,
                 sil_score=0.0, device="cuda"):
        from .criterion import _sil_args
        sil = _sil_args("ManyTokenStreamingDecoder", sil_token, sil_score, lexicon)
        self.sil_token, self.sil_score = sil if sil is not None else (-1, 0.0)
        super().__init__(slots, max_chunk, max_frames, nlabel, beam=beam, beam_token=beam_token, threshold=threshold, log_add=log_add,
                         normalize=normalize, lm=lm, lm_weight=lm_weight, class_score=class_score, eos_score=eos_score, lexicon=lexicon,
                         word_score=word_score, device=device)

    def _make(self, d, h):
        return self.L.w2l_beam_session_create_mt(C.byref(d), int(self.sil_token), float(self.sil_score), C.byref(h))
