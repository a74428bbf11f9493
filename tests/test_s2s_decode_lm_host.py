"""Host side of the LM-fused seq2seq decoder, no GPU: the refusals w2l_s2s_decode_lm adds to its sibling's against their
codes (all precede the first launch: the device pointers are never dereferenced), the Python refusals by name, and the float64
reference on the cases of tests/test_gpu_s2s_decode_lm.py: tokens are compared exactly there, so every case's smallest decision margin
must be ten times the fp32 bar's absolute size (a seed that falls short is replaced, the margin never loosened), and the cases must be
what their names say."""
import ctypes

import numpy as np
import pytest
import torch

import s2s_decode_lm_ref as DL
import s2s_decode_ref as D
from wav2letter_amd import NGramLM, Seq2SeqCriterion, _lib

EINVAL, EUNSUP = _lib.W2L_EINVAL, _lib.W2L_EUNSUPPORTED


@pytest.mark.parametrize("bad,code", [(dict(null=10), EINVAL), (dict(null=12), EINVAL), (dict(lmWeight=float("inf")), EINVAL),
                                      (dict(lmWeight=float("nan")), EINVAL), (dict(eosScore=float("-inf")), EINVAL), (dict(has_eos=2), EINVAL),
                                      (dict(has_eos=-1), EINVAL), (dict(null=0), EINVAL), (dict(nbest=4), EINVAL), (dict(beam=129), EUNSUP),
                                      (dict(N=65537), EUNSUP)], ids=str)
def test_refusals(bad, code):
    f = dict(B=2, T=7, H=32, N=9, ldenc=64, eos=0, beam=3, beamToken=4, maxLen=5, nbest=2, threshold=1.0, eosScore=0.0, temperature=1.0,
             attentionThreshold=-1, lmWeight=0.5)
    f.update({k: v for k, v in bad.items() if k in f})
    d, L = _lib.S2sDecodeDesc(*[f[n] for n, _ in _lib.S2sDecodeDesc._fields_]), _lib.lib()
    free = _lib.S2sDecodeDesc(*[0.0 if n == "lmWeight" else f[n] for n, _ in _lib.S2sDecodeDesc._fields_])
    if code == EINVAL and "null" in bad:   # a valid descriptor: the LM columns stand behind the sibling's workspace, which refuses the weight
        assert L.w2l_s2s_decode_lm_workspace_size(ctypes.byref(d)) > L.w2l_s2s_decode_workspace_size(ctypes.byref(free)) > 0
        assert L.w2l_s2s_decode_workspace_size(ctypes.byref(d)) == 0
    p = [None if i == bad.get("null") else ctypes.c_void_p(64) for i in range(13)]   # 7 operands, 4 results, workspace, lm
    kl = np.array((7, 1), np.int32)
    ws = max(L.w2l_s2s_decode_lm_workspace_size(ctypes.byref(d)), 1)
    assert L.w2l_s2s_decode_lm(ctypes.byref(d), *p[:7], kl.ctypes.data, *p[7:12], ws, None, p[12], bad.get("has_eos", 1)) == code


def test_python_refusals():
    crit, enc = Seq2SeqCriterion(23, 32, 22), torch.zeros(1, 5, 32)
    lm = NGramLM.from_ngrams([(np.arange(9).reshape(9, 1), np.full(9, -1.0), None)], 9)
    for option, words in [(dict(lm=lm, lm_weight=1.0), "the LM has 9 tokens"), (dict(lm=lm, hardselection=1.0), "hardselection")]:
        with pytest.raises(_lib.W2LInvalidArgument, match=words):
            crit.beamSearch(enc, **option)


@pytest.mark.parametrize("name", DL.CASES)
def test_reference_is_decisive(name):
    p, enc, kl, keyvalue, lm, weight, opt, (hyps, margin, amargin, dropped), _ = DL.run_case(name)
    scale = max(abs(s) for utt in hyps for _, s, _ in utt)
    print(f"{name}: score margin {margin:.3g} against 10 x 1e-4 x {scale:.3g}; attention margin {amargin:.3g}; dropped {dropped}; "
          f"back-off chain {lm.max_chain}, <unk> {lm.unk_hits}; lengths {[[len(t) for t, _, _ in u] for u in hyps]}")
    assert margin >= 10 * 1e-4 * scale and amargin >= 10 * 1e-4
    if name == "trigram_backoff":   # real back-off chains, <unk> fallbacks, and an LM that changes the 1-best
        free = D.search(*D.f64(p, enc), kl, keyvalue, D.EOS, **opt)[0]
        assert lm.max_chain >= 2 and lm.unk_hits > 0 and any(f[0][0] != h[0][0] for f, h in zip(free, hyps))
    assert name != "no_eos_threshold" or (dropped > 0 and not lm.has_eos)
