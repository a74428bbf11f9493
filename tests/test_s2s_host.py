"""Host side of the seq2seq criterion: every refusal of the three kernel groups' C ABI against its expected code (all
of them precede the first launch, so the device pointers are never dereferenced), the refusals of the Python class by name, the
teacher-forcing draw stream against the restatement, and the room the 1e-4 bar leaves over plain float32.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import s2s_ref as R
from wav2letter_amd import Seq2SeqCriterion, _lib, seq2seq

EINVAL, EUNSUP = _lib.W2L_EINVAL, _lib.W2L_EUNSUPPORTED
ONE = ctypes.c_void_p(64)
ints = lambda *v: np.array(v, np.int32)


def attn(null=None, kl=(7, 1), tl=(3, 5), ws=None, backward=False, **k):
    f = dict(B=2, U=5, T=7, H=32, ldenc=64, windowStd=4.0, addQuery=1)
    f.update(k)
    d, L = _lib.S2sAttnDesc(*[f[n] for n, _ in _lib.S2sAttnDesc._fields_]), _lib.lib()
    kl, tl = ints(*kl), ints(*tl)
    ws = max(L.w2l_s2s_attn_workspace_size(ctypes.byref(d), int(backward)), 1) if ws is None else ws
    p = [None if i == null else ONE for i in range(12)]
    if backward:
        return L.w2l_s2s_attn_backward(ctypes.byref(d), p[0], p[1], p[2], kl.ctypes.data, tl.ctypes.data, *p[3:10], ws, None)
    return L.w2l_s2s_attn_forward(ctypes.byref(d), p[0], p[1], p[2], kl.ctypes.data, tl.ctypes.data, p[3], p[4], p[5], ws, None)


def xent(M=4, N=9, B=2, target=(0, 8, -1, 3), utt=(0, 0, 1, 1), eps=0.1, null=None, ws=None, backward=False):
    L, t, u = _lib.lib(), ints(*target), None if utt is None else ints(*utt)
    ws = max(L.w2l_s2s_xent_workspace_size(M, B), 1) if ws is None else ws
    p = [None if i == null else ONE for i in range(5)]
    up = None if u is None else u.ctypes.data
    if backward:
        return L.w2l_s2s_xent_backward(M, N, B, p[0], p[1], t.ctypes.data, up, eps, p[2], p[3], p[4], ws, None)
    return L.w2l_s2s_xent_forward(M, N, B, p[0], t.ctypes.data, up, eps, p[1], p[2], p[3], ws, None)


def emb(M=3, N=5, H=8, tokens=(-1, 4, 0), null=None, ws=None, backward=False):
    L, t = _lib.lib(), ints(*tokens)
    ws = max(L.w2l_embedding_workspace_size(M, N), 1) if ws is None else ws
    p = [None if i == null else ONE for i in range(4)]
    fn = L.w2l_embedding_backward if backward else L.w2l_embedding_forward
    return fn(M, N, H, t.ctypes.data, p[0], p[1], p[2], p[3], ws, None)


REFUSALS = [(attn, dict(B=0), EINVAL), (attn, dict(U=0), EINVAL), (attn, dict(T=0), EINVAL), (attn, dict(H=0), EINVAL), (attn, dict(ldenc=31), EINVAL),
            (attn, dict(kl=(8, 1)), EINVAL), (attn, dict(kl=(7, 0)), EINVAL), (attn, dict(tl=(0, 5)), EINVAL), (attn, dict(tl=(3, 6)), EINVAL),
            (attn, dict(ws=8), EINVAL), (attn, dict(ws=8, backward=True), EINVAL), (attn, dict(windowStd=float("nan")), EINVAL),
            *[(attn, dict(null=i), EINVAL) for i in range(6)], *[(attn, dict(null=i, backward=True), EINVAL) for i in (0, 1, 2, 3, 4, 6, 7, 8, 9)],
            (attn, dict(H=48, ldenc=48), EUNSUP), (attn, dict(H=1056, ldenc=1056), EUNSUP), (attn, dict(T=1025), EUNSUP), (attn, dict(U=513), EUNSUP),
            (attn, dict(B=1025, kl=(1,) * 1025, tl=(1,) * 1025), EUNSUP),
            (xent, dict(M=0), EINVAL), (xent, dict(N=0), EINVAL), (xent, dict(B=0), EINVAL), (xent, dict(target=(0, 9, -1, 3)), EINVAL),
            (xent, dict(target=(0, -2, -1, 3)), EINVAL), (xent, dict(utt=(0, 1, 0, 1)), EINVAL), (xent, dict(utt=(0, 0, 1, 2)), EINVAL),
            (xent, dict(utt=None, B=3), EINVAL), (xent, dict(eps=1.0), EINVAL), (xent, dict(eps=-0.1), EINVAL), (xent, dict(ws=8), EINVAL),
            *[(xent, dict(null=i), EINVAL) for i in range(4)], *[(xent, dict(null=i, backward=True), EINVAL) for i in range(5)],
            (xent, dict(N=65537), EUNSUP), (xent, dict(B=1025), EUNSUP),
            (emb, dict(M=0), EINVAL), (emb, dict(N=0), EINVAL), (emb, dict(H=0), EINVAL), (emb, dict(tokens=(-1, 5, 0)), EINVAL),
            (emb, dict(tokens=(-2, 4, 0)), EINVAL), (emb, dict(ws=8), EINVAL), *[(emb, dict(null=i, backward=b), EINVAL) for i in range(4) for b in (False, True)],
            (emb, dict(N=65537), EUNSUP), (emb, dict(H=4097), EUNSUP)]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals(i):
    fn, bad, code = REFUSALS[i]
    assert fn(**bad) == code, bad


def test_sizes():
    L, d = _lib.lib(), _lib.S2sAttnDesc(16, 120, 188, 512, 1024, 4.0, 1)
    fwd, bwd = (L.w2l_s2s_attn_workspace_size(ctypes.byref(d), b) for b in (0, 1))
    assert 0 < fwd < bwd and bwd >= 16 * 120 * 188 * 4
    big = _lib.S2sAttnDesc(1024, 512, 1024, 1024, 2048, 0.0, 0)                      # the least the caps must cover
    assert L.w2l_s2s_attn_workspace_size(ctypes.byref(big), 0) > 0 and L.w2l_s2s_xent_workspace_size(0, 16) == 0 and L.w2l_embedding_workspace_size(1920, 0) == 0


@pytest.mark.parametrize("kwargs,name", [(dict(inputFeeding=True), "input feeding"), (dict(samplingStrategy="model"), "sampling strategy 'model'"),
                                         (dict(samplingStrategy="gumbel"), "sampling strategy 'gumbel'"), (dict(nAttnRound=2), "more than one attention round"),
                                         (dict(nRnnLayer=3), "more than one attention round or RNN layer"), (dict(attention="location"), "attention 'location'"),
                                         (dict(attention="neural"), "attention 'neural'"), (dict(window=("median", 3)), "window"),
                                         (dict(window=("soft", 4.0)), "window"), (dict(window=("step", 1)), "window")])
def test_python_refusals(kwargs, name):
    with pytest.raises(_lib.W2LInvalidArgument, match=name):
        Seq2SeqCriterion(23, 32, 22, **kwargs)


@pytest.mark.parametrize("pct,seed", [(50, 77), (0, 1), (75, 2 ** 63 + 5), (100, 3)])
def test_draw_stream(pct, seed):
    y = np.random.default_rng(pct).integers(0, 23, size=(4, 9))
    got, want = seq2seq.teacher_forcing(y, 23, pct, seed), R.teacher_forcing(y, 23, pct, seed)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].max() <= 22
    assert want[1].all() if pct == 0 else (not want[1].any() if pct == 100 else want[1].any())
    assert (got[0][want[1]] <= 21).all()                                             # a replacement is uniform in 0..N-2


def test_float32_leaves_room():
    """the restatement in float32 against itself in float64 on the GPU tests' criterion case: the error a correct fp32 implementation
    makes, to be held against the 1e-4 bar"""
    B, U, T, H, N = 3, 6, 19, 32, 23
    rng = np.random.default_rng(5)
    names = ("embedding", "rnn", "linear_weight", "linear_bias", "start")
    p = [rng.uniform(-1, 1, s).astype(np.float32) * H ** -0.5 for s in ((N, H), (3 * H * (2 * H + 2),), (H, N), (N,), (H,))]
    enc, y = rng.normal(size=(B, T, 2 * H)).astype(np.float32), rng.integers(0, N, size=(B, U))
    tl, kl, g = np.array([6, 1, 4]), np.array([19, 6, 12]), rng.normal(size=B).astype(np.float32)
    fn = lambda enc, *p: R.criterion(dict(zip(names, p)), enc, y, y, tl, kl, True, 4.0, 0.05)[:1]
    c64, c32 = (R.Case(fn, ("enc",) + names, [enc] + p, (g,), dtype=dt) for dt in (torch.float64, torch.float32))
    worst = max(np.abs(c32.grad[n] - c64.grad[n]).max() / np.abs(c64.grad[n]).max() for n in c64.grad)
    worst = max(worst, np.abs(c32.out[0] - c64.out[0]).max() / np.abs(c64.out[0]).max())
    print(f"float32 against float64: {worst:.2e}")
    assert worst < 1e-5
