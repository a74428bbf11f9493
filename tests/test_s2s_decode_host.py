"""Host side of the seq2seq decoder: every refusal of the C ABI against its code (all precede the first launch, so the
device pointers are never dereferenced), the refusals of the Python class by name, and the decision margins of the float64 reference on
the case table of tests/test_gpu_s2s_decode.py: exact tokens are demanded there, so here every case's smallest margin must be ten
times the fp32 bar's absolute size.  A seed that falls short is replaced; the margin is never loosened.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import s2s_decode_ref as D
from wav2letter_amd import Seq2SeqCriterion, _lib

EINVAL, EUNSUP = _lib.W2L_EINVAL, _lib.W2L_EUNSUPPORTED
ONE = ctypes.c_void_p(64)


def call(step=False, null=None, kl=(7, 1), parent=(0, -1, 2, 1, 0, 0), token=(-1, 3, 8, 0, 1, 2), ws=None, **k):
    f = dict(B=2, T=7, H=32, N=9, ldenc=64, eos=0, beam=3, beamToken=4, maxLen=5, nbest=2, threshold=1.0, eosScore=0.0, temperature=1.0,
             attentionThreshold=-1, lmWeight=0.0)
    f.update(k)
    d, L = _lib.S2sDecodeDesc(*[f[n] for n, _ in _lib.S2sDecodeDesc._fields_]), _lib.lib()
    ws = max(L.w2l_s2s_decode_workspace_size(ctypes.byref(d)), 1) if ws is None else ws
    kl, parent, token = (np.array(v, np.int32) for v in (kl, parent, token))
    klp = kl.ctypes.data if kl.size else None   # kl=(): a null keyLen
    p = [None if i == null else ONE for i in range(16)]
    if step:
        return L.w2l_s2s_decode_step(ctypes.byref(d), *p[:7], klp, parent.ctypes.data, token.ctypes.data, *p[7:15], ws, None)
    return L.w2l_s2s_decode(ctypes.byref(d), *p[:7], klp, *p[7:11], ws, None)


REFUSALS = [*[(dict(**{n: 0}), EINVAL) for n in ("B", "T", "H", "beam", "beamToken", "maxLen", "nbest")], (dict(N=1), EINVAL), (dict(ldenc=31), EINVAL),
            (dict(eos=9), EINVAL), (dict(eos=-1), EINVAL), (dict(nbest=4), EINVAL), (dict(temperature=0.0), EINVAL), (dict(threshold=-1.0), EINVAL),
            (dict(threshold=float("nan")), EINVAL), (dict(kl=(8, 1)), EINVAL), (dict(kl=(7, 0)), EINVAL), (dict(kl=()), EINVAL),
            (dict(step=True, kl=()), EINVAL), (dict(ws=8), EINVAL),
            *[(dict(null=i), EINVAL) for i in range(11)], *[(dict(step=True, null=i), EINVAL) for i in range(15) if i != 7],
            (dict(step=True, parent=(0, -1, 3, 1, 0, 0)), EINVAL), (dict(step=True, token=(-1, 9, 8, 0, 1, 2)), EINVAL),
            (dict(step=True, token=(-2, 3, 8, 0, 1, 2)), EINVAL), (dict(step=True, null=7), EINVAL),   # a live row with a token and no hPrev
            (dict(lmWeight=0.5), EUNSUP), (dict(beam=129), EUNSUP), (dict(beamToken=65), EUNSUP), (dict(maxLen=513), EUNSUP), (dict(H=48, ldenc=48), EUNSUP),
            (dict(H=1056, ldenc=1056), EUNSUP), (dict(T=1025), EUNSUP), (dict(N=65537), EUNSUP), (dict(B=1025, kl=(1,) * 1025), EUNSUP)]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals(i):
    bad, code = REFUSALS[i]
    assert call(**bad) == code, bad


def test_workspace_covers_the_recipe():
    L = _lib.lib()
    d = _lib.S2sDecodeDesc(16, 440, 512, 9998, 1024, 9997, 80, 10, 120, 1, 7.0, 0.0, 1.0, 30, 0.0)
    big = _lib.S2sDecodeDesc(1024, 1024, 1024, 65536, 2048, 0, 128, 64, 512, 128, float("inf"), 0.0, 1.0, -1, 0.0)
    assert 0 < L.w2l_s2s_decode_workspace_size(ctypes.byref(d)) < 1 << 28 and L.w2l_s2s_decode_workspace_size(ctypes.byref(big)) > 0


@pytest.mark.parametrize("option,name", [(dict(lm_weight=0.5), "LM fusion"), (dict(lmweight=1.0), "LM fusion"), (dict(hardselection=1.0), "hardselection"),
                                         (dict(softselection=0.5), "softselection")])
def test_python_refusals(option, name):
    crit = Seq2SeqCriterion(23, 32, 22)
    with pytest.raises(_lib.W2LInvalidArgument, match=name):
        crit.beamSearch(torch.zeros(1, 5, 32), **option)


@pytest.mark.parametrize("name", D.CASES)
def test_reference_is_decisive(name):
    *_, (hyps, margin, amargin) = D.run_case(name)
    scale = max(abs(s) for utt in hyps for _, s in utt)
    print(f"{name}: score margin {margin:.3g} against 10 x 1e-4 x {scale:.3g}; attention margin {amargin:.3g}; lengths {[[len(t) for t, _ in u] for u in hyps]}")
    assert margin >= 10 * 1e-4 * scale and amargin >= 10 * 1e-4
