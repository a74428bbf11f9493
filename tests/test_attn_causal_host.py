"""Host side of the causal self-attention kernel and the Transformer decoder criterion: every refusal of the C ABI
against its expected code (all of them precede the first launch, so the device pointers are never dereferenced), the workspace sizes,
the refusals of the Python class by name, and the draw order against the restatement.  No GPU."""
import ctypes

import numpy as np
import pytest

import attn_causal_ref as R
from wav2letter_amd import TransformerCriterion, _lib, seq2seq, transformer_criterion

EINVAL, EUNSUP = _lib.W2L_EINVAL, _lib.W2L_EUNSUPPORTED
ONE = ctypes.c_void_p(64)


def call(null=None, ln=(5, 1), ws=None, backward=False, ptr=ONE, **k):
    f = dict(B=2, Hd=2, U=5, d=32, ld=192, ldc=64, n0=4, scale=0.1, dropP=0.1, dropSeed=1, dropStream=2)
    f.update(k)
    d, L = _lib.AttnCausalDesc(*[f[n] for n, _ in _lib.AttnCausalDesc._fields_]), _lib.lib()
    ln = np.array(ln, np.int32)
    ws = max(L.w2l_attn_causal_workspace_size(ctypes.byref(d), int(backward)), 1) if ws is None else ws
    p = [None if i == null else ptr for i in range(12)]
    if backward:   # q k v E | lse dctx dq dk dv dE | workspace
        return L.w2l_attn_causal_backward(ctypes.byref(d), *p[:4], ln.ctypes.data, *p[4:11], ws, None)
    return L.w2l_attn_causal_forward(ctypes.byref(d), *p[:4], ln.ctypes.data, p[4], p[5], p[6], ws, None)


REFUSALS = [*[(dict(**{n: 0}), EINVAL) for n in ("B", "Hd", "U", "d")], (dict(n0=-1), EINVAL), (dict(ld=63), EINVAL), (dict(ldc=63), EINVAL),
            (dict(dropP=1.0), EINVAL), (dict(dropP=-0.1), EINVAL), (dict(scale=float("nan")), EINVAL), (dict(ln=(6, 1)), EINVAL),
            (dict(ln=(5, 0)), EINVAL), (dict(ws=8), EINVAL), (dict(ws=8, backward=True), EINVAL),
            *[(dict(null=i), EINVAL) for i in (0, 1, 2, 4, 5, 6)], *[(dict(null=i, backward=True), EINVAL) for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10)],
            (dict(d=48, ld=288, ldc=96), EUNSUP), (dict(d=288, ld=1728, ldc=576), EUNSUP), (dict(Hd=5, d=256, ld=3840, ldc=1280), EUNSUP),
            (dict(U=513), EUNSUP), (dict(B=1025, ln=(1,) * 1025), EUNSUP), (dict(ld=194), EUNSUP), (dict(ldc=66), EUNSUP),
            (dict(ptr=ctypes.c_void_p(68)), EUNSUP), (dict(ptr=ctypes.c_void_p(68), backward=True), EUNSUP)]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals(i):
    bad, code = REFUSALS[i]
    assert call(**bad) == code, bad


def test_sizes():
    """pure host functions: lengths only forward; D [B Hd][U] and the table partials [B Hd][U][d] besides in backward; 0 when refused"""
    L, d = _lib.lib(), _lib.AttnCausalDesc(8, 4, 120, 64, 768, 256, 119, 0.125, 0.1, 0, 0)
    fwd, bwd = (L.w2l_attn_causal_workspace_size(ctypes.byref(d), b) for b in (0, 1))
    assert 0 < fwd < 1024 and bwd >= 8 * 4 * 120 * (64 + 1) * 4
    big = _lib.AttnCausalDesc(1024, 4, 512, 256, 3072, 1024, 511, 0.1, 0.0, 0, 0)       # the least the caps must cover
    assert L.w2l_attn_causal_workspace_size(ctypes.byref(big), 1) > 2 ** 31
    bad = _lib.AttnCausalDesc(8, 4, 120, 48, 768, 256, 119, 0.125, 0.1, 0, 0)
    assert L.w2l_attn_causal_workspace_size(ctypes.byref(bad), 1) == 0 and L.w2l_attn_causal_workspace_size(None, 0) == 0


@pytest.mark.parametrize("kwargs,name", [(dict(attention="location"), "attention 'location'"), (dict(attention="neural"), "attention 'neural'"),
                                         (dict(window=("median", 3)), "window"), (dict(window=("soft", 4.0)), "window"),
                                         (dict(nHeads=3), "no multiple of nHeads"), (dict(nHeads=8), "head width 8"),
                                         (dict(nHeads=1, hiddenDim=320), "head width 320")])
def test_python_refusals(kwargs, name):
    args = dict(nClass=23, hiddenDim=64, eos=22, nLayer=1, nHeads=2)
    args.update(kwargs)
    with pytest.raises(_lib.W2LInvalidArgument, match=name):
        TransformerCriterion(**args)


def test_python_refuses_long_targets_and_decoding():
    import torch
    crit = TransformerCriterion(23, 64, 22, 1, nHeads=2, maxDecoderOutputLen=4)
    with pytest.raises(_lib.W2LInvalidArgument, match="maxDecoderOutputLen"):
        crit(torch.zeros(1, 3, 64), np.zeros((1, 5), np.int32))
    for fn in (crit.beamSearch, crit.viterbiPath):
        with pytest.raises(_lib.W2LError, match="not built"):
            fn(None)


@pytest.mark.parametrize("pct,p,seed", [(50, 0.5, 77), (100, 0.3, 1), (0, 0.9, 2 ** 63 + 5)])
def test_draw_order(pct, p, seed):
    """teacher forcing first (one draw per entry, a second per replacement), then one draw per block from the same stream"""
    y = np.random.default_rng(pct).integers(0, 23, size=(4, 9))
    replaced = seq2seq.teacher_forcing(y, 23, pct, seed)[1]
    before = y.size + int(replaced.sum()) if pct < 100 else 0
    got, want = transformer_criterion.layer_drop(6, p, seed, before), R.layer_drop(6, p, seed, before)
    assert np.array_equal(got, want) and np.array_equal(replaced, R.S.teacher_forcing(y, 23, pct, seed)[1])
