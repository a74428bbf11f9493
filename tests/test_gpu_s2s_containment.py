"""Containment of the seq2seq criterion's device calls (DESIGN.md 3.19 is the contract): with workspaces of exactly the declared
bytes and an encoder output whose frames lie further apart than its columns, the calls read their operands only inside their extents,
write every element of their results and nothing else, and do not depend on what the workspaces held.

As in tests/test_gpu_cpc_containment.py every case runs on identical inputs in three guarded arenas (tests/arena.py) -- quiet, quiet
again, NaN -- and is compared with the float64 restatement (tests/s2s_ref.py).  Lengths, targets and tokens are host arrays."""
import ctypes

import numpy as np
import pytest

import s2s_ref as R
from tests.test_gpu_containment import _stream
from tests.test_gpu_cpc_containment import run_three
from tests.test_gpu_s2s import attn_operands
from wav2letter_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("keyvalue", [False, True])
def test_attention_stays_inside(keyvalue):
    """B = 3, U = 37, T = 41, H = 96, frames 3 floats further apart than their columns: the keys and values are read unaligned"""
    B, U, T, H = 3, 37, 41, 96
    h, enc, dout, dalpha, kl, tl = attn_operands(B, U, T, H, keyvalue, seed=3)
    Cc = enc.shape[2]
    d = _lib.S2sAttnDesc(B, U, T, H, Cc + 3, 4.0, 0)
    c = R.Case(lambda h, enc: R.attention(h, enc, kl, tl, keyvalue, 4.0), ("h", "enc"), (h, enc), (dout, dalpha))

    def fn(r):
        L, dp, off = r.L, ctypes.byref(d), 4 * H * int(keyvalue)
        n0, n1 = L.w2l_s2s_attn_workspace_size(dp, 0), L.w2l_s2s_attn_workspace_size(dp, 1)
        ph, pe = r.inp("h", h), r.inp("enc", enc, ld=Cc + 3)
        pa = r.out("alpha", (B, U, T))
        r.ok(L.w2l_s2s_attn_forward(dp, ph, pe, pe + off, kl.ctypes.data, tl.ctypes.data, r.out("ctx", (B, U, H)), pa, r.work("ws0", n0), n0, _stream()), "forward")
        pd = r.out("denc", (B, T, Cc), ld=Cc + 3)
        r.ok(L.w2l_s2s_attn_backward(dp, ph, pe, pe + off, kl.ctypes.data, tl.ctypes.data, pa, r.inp("dout", dout), r.inp("dalpha", dalpha),
                                     r.out("dh", (B, U, H)), pd, pd + off, r.work("ws1", n1), n1, _stream()), "backward")
        return lambda: {"ctx": ("rel", c.out[0]), "alpha": ("rel", c.out[1]), "dh": ("rel", c.grad["h"]), "denc": ("rel", c.grad["enc"])}
    run_three(fn)


def test_cross_entropy_and_embedding_stay_inside():
    M, N, B, H, eps = 7, 1030, 3, 40, 0.05
    rng = np.random.default_rng(2)
    z, g = rng.normal(size=(M, N)).astype(np.float32), rng.normal(size=B).astype(np.float32)
    target, utt = np.array([3, N - 1, -1, 0, -1, 17, 5], np.int32), np.array([0, 0, 0, 1, 1, 2, 2], np.int32)
    tokens = np.array([-1, 2, 0, 6, 2, -1, 1], np.int32)
    E, s, dx = (rng.normal(size=sh).astype(np.float32) for sh in ((7, H), (H,), (M, H)))
    cz = R.Case(lambda z: (R.cross_entropy(z, target, utt, B, eps),), ("z",), (z,), (g,))
    ce = R.Case(lambda E, s: (R.embedding(tokens, E, s),), ("E", "s"), (E, s), (dx,))

    def fn(r):
        L = r.L
        nz, ne = L.w2l_s2s_xent_workspace_size(M, B), L.w2l_embedding_workspace_size(M, 7)
        pz, plse, wz = r.inp("z", z), r.out("lse", (M,)), r.work("wsz", nz)
        r.ok(L.w2l_s2s_xent_forward(M, N, B, pz, target.ctypes.data, utt.ctypes.data, eps, plse, r.out("loss", (B,)), wz, nz, _stream()), "xent forward")
        r.ok(L.w2l_s2s_xent_backward(M, N, B, pz, plse, target.ctypes.data, utt.ctypes.data, eps, r.inp("g", g), r.out("dz", (M, N)), wz, nz, _stream()), "xent backward")
        we = r.work("wse", ne)
        r.ok(L.w2l_embedding_forward(M, 7, H, tokens.ctypes.data, r.inp("E", E), r.inp("s", s), r.out("x", (M, H)), we, ne, _stream()), "embedding forward")
        r.ok(L.w2l_embedding_backward(M, 7, H, tokens.ctypes.data, r.inp("dx", dx), r.out("dE", (7, H)), r.out("ds", (H,)), we, ne, _stream()), "embedding backward")
        lse = np.log(np.exp(z.astype(np.float64)).sum(1))
        return lambda: {"lse": ("rel", lse), "loss": ("rel", cz.out[0]), "dz": ("rel", cz.grad["z"]), "x": ("exact", ce.out[0]), "dE": ("rel", ce.grad["E"]),
                        "ds": ("rel", ce.grad["s"])}
    run_three(fn)
