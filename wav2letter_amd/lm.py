"""NGramLM: the back-off n-gram language model table of the LM-fused CTC beam search (w2l_ngram_lm_*; the contract -- words,
states, edges, the score rule q, the blob -- is in include/w2l_hip.h).  The table is built and scored on the host by libw2l_hip.so;
device_blob() copies its bytes, unchanged, to the GPU for criterion.ctc_beam_search(..., lm=...)."""
import ctypes as C

import numpy as np

from . import _lib


def _fail(status, what):
    msg = _lib.lib().w2l_host_last_error().decode()
    if status == _lib.W2L_EINVAL:
        raise _lib.W2LInvalidArgument(f"{what}: {msg}")
    raise _lib.W2LError(f"{what}: {_lib._ERR.get(status, status)}: {msg}")


def _aligned(nbytes):
    raw = np.zeros(nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + nbytes]


class NGramLM:
    """words 0 .. num_tokens-1 are the token classes, `bos` = num_tokens, `eos` = num_tokens + 1"""

    def __init__(self, blob, message=""):
        L = _lib.lib()
        self.blob = blob
        self.message = message
        v = [C.c_int() for _ in range(5)]
        st = L.w2l_ngram_lm_info(blob.ctypes.data, *[C.addressof(x) for x in v])
        if st:
            _fail(st, "NGramLM")
        self.order, self.num_tokens, self.num_states = v[0].value, v[1].value, v[2].value
        self.has_bos, self.has_eos = bool(v[3].value), bool(v[4].value)
        self.bos, self.eos = self.num_tokens, self.num_tokens + 1
        s = C.c_int()
        st = L.w2l_ngram_lm_start(blob.ctypes.data, C.addressof(s))
        if st:
            _fail(st, "NGramLM")
        self.start = s.value
        self._device = {}

    @classmethod
    def _two_calls(cls, call, what):
        size = C.c_size_t(0)
        st = call(None, C.addressof(size))
        if st:
            _fail(st, what)
        blob = _aligned(size.value)
        st = call(blob.ctypes.data, C.addressof(size))
        if st:
            _fail(st, what)
        return blob

    @classmethod
    def from_ngrams(cls, ngrams, num_tokens, unk_logp=0.0):
        """ngrams[k-1] = (words [count][k] int, logp [count], backoff [count] or None), natural logs"""
        L = _lib.lib()
        order = len(ngrams)
        counts = (C.c_size_t * max(order, 1))(*[len(g[1]) for g in ngrams])
        words = np.concatenate([np.asarray(g[0], np.int32).reshape(-1) for g in ngrams] + [np.zeros(0, np.int32)])
        logp = np.concatenate([np.asarray(g[1], np.float32).reshape(-1) for g in ngrams] + [np.zeros(0, np.float32)])
        bo = np.concatenate([(np.zeros(len(g[1]), np.float32) if g[2] is None else np.asarray(g[2], np.float32).reshape(-1))
                             for g in ngrams] + [np.zeros(0, np.float32)])
        for k, g in enumerate(ngrams):
            if np.asarray(g[0]).size != (k + 1) * len(g[1]) or (g[2] is not None and len(g[2]) != len(g[1])):
                raise _lib.W2LInvalidArgument(f"NGramLM.from_ngrams: order {k + 1}: words, logp and backoff disagree in size")
        blob = cls._two_calls(lambda b, n: L.w2l_ngram_lm_build(order, C.addressof(counts), words.ctypes.data, logp.ctypes.data,
                                                                bo.ctypes.data, int(num_tokens), float(unk_logp), b, n),
                              "NGramLM.from_ngrams")
        return cls(blob)

    @classmethod
    def from_arpa(cls, path, tokens):
        """ARPA text; tokens[i] spells class i.  .skipped counts the n-grams left out for a word outside the dictionary"""
        L = _lib.lib()
        toks = (C.c_char_p * max(len(tokens), 1))(*[t.encode() for t in tokens])
        skipped = C.c_int(0)
        blob = cls._two_calls(lambda b, n: L.w2l_ngram_lm_from_arpa(str(path).encode(), len(tokens), C.addressof(toks), b, n,
                                                                    C.addressof(skipped)), "NGramLM.from_arpa")
        lm = cls(blob, L.w2l_host_last_error().decode())
        lm.skipped = skipped.value
        return lm

    def score(self, state, word):
        """q(state, word) -> (log p as float32, next state)"""
        p, nxt = C.c_float(), C.c_int()
        st = _lib.lib().w2l_ngram_lm_score(self.blob.ctypes.data, int(state), int(word), C.addressof(p), C.addressof(nxt))
        if st:
            _fail(st, "NGramLM.score")
        return np.float32(p.value), nxt.value

    def device_blob(self, device):
        """the table on `device` (copied once per device)"""
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._device:
            self._device[device] = torch.from_numpy(np.array(self.blob)).to(device)
        return self._device[device]
