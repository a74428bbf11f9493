"""Containment of the four device calls of the CPC criterion (DESIGN.md 3.19 is the contract): operands are read only inside their
extents, results and the DECLARED bytes of the workspaces are written only inside theirs, every element of a result is written.

As in tests/test_gpu_containment.py every case runs on identical inputs in three guarded arenas (tests/arena.py) of identical
layout -- quiet, quiet again, NaN -- and asserts (a) status 0 and every guard byte unchanged, (b) results bit-identical between the
quiet and the NaN arena, (c) no element of a result still holds the prefill pattern after the NaN run, (d) agreement with the float64
restatement (tests/cpc_ref.py) at the fp32 bar.  The workspaces are exactly w2l_cpc_workspace_size / w2l_cpc_mask_workspace_size
bytes and start as NaN in the third run: a call that reads a workspace byte it has not written turns its result NaN."""
import numpy as np
import pytest
import torch

import cpc_ref as R
from tests.arena import NAN_PATTERN, QUIET_PATTERN, Arena
from tests.test_gpu_containment import U8, Run, _stream, bits, meets
from wav2letter_amd import _lib

pytestmark = pytest.mark.gpu


def run_three(fn):
    runs = []
    for pattern in (QUIET_PATTERN, QUIET_PATTERN, NAN_PATTERN):
        r = Run(Arena("cuda", pattern, 48 << 20), _lib.lib())
        ref = fn(r)
        torch.cuda.synchronize()
        r.ar.check()                                                                  # (a)
        runs.append((r, ref))
    (q, ref), (q2, _), (n, _) = runs
    want = ref()
    assert set(want) == set(q.results)
    for key in q.results:
        a, b, c = q.results[key], q2.results[key], n.results[key]
        assert torch.equal(bits(a), bits(b)), f"'{key}' differs between two quiet runs: the contract says bit-identical"
        assert torch.equal(bits(a), bits(c)), (                                       # (b)
            f"result '{key}' depends on bytes outside the operands: {int((bits(a) != bits(c)).sum())} of {a.numel()} elements differ "
            f"between the quiet and the NaN arena, {int(torch.isnan(c).sum())} are NaN")
    for key in n.fresh:                                                               # (c)
        assert n.ar.unwritten(key) == 0, f"{n.ar.unwritten(key)} valid elements of result '{key}' were never written"
    for key, (bar, ref64) in want.items():                                            # (d)
        meets(bar, q.results[key].cpu().numpy(), ref64, key)


@pytest.mark.parametrize("dims,tau", [((3, 37, 20, 12, 8, 11, 5), 0.1), ((2, 64, 33, 17, 7, 16, 16), 0.05), ((1, 9, 5, 3, 2, 9, 9), 0.2),
                                       ((2, 300, 36, 64, 32, 130, 100), 0.1)])
def test_forward_and_backward_stay_inside(dims, tau):
    """odd sizes; K = M; M = T with one utterance; a shape whose products take the LDS-DMA GEMM (K % 32 == 0) and more than one tile"""
    B, T, Ce, Cc, D, M, K = dims
    c = R.Case(*dims, tau, seed=sum(dims))

    def fn(r):
        L = r.L
        p = {k: r.inp(k, getattr(c, k)) for k in ("enc", "ctx", "mask_index", "neg", "We", "be", "Wc", "bc", "g")}
        ws = r.work("workspace", L.w2l_cpc_workspace_size(*dims))
        r.ok(L.w2l_cpc_forward(B, T, Ce, Cc, D, M, K, tau, p["enc"], p["ctx"], p["mask_index"], p["neg"], p["We"], p["be"], p["Wc"], p["bc"],
                               r.out("loss", (B,)), ws, _stream()), "forward")
        r.ok(L.w2l_cpc_backward(B, T, Ce, Cc, D, M, K, tau, p["mask_index"], p["neg"], p["We"], p["Wc"], p["g"], r.out("denc", (B, T, Ce)),
                                r.out("dctx", (B, T, Cc)), r.out("dWe", (D, Ce)), r.out("dbe", (D,)), r.out("dWc", (D, Cc)), r.out("dbc", (D,)),
                                ws, _stream()), "backward")
        return lambda: {"loss": ("rel", c.loss), "denc": ("rel", c.grads["enc"]), "dctx": ("rel", c.grads["ctx"]), "dWe": ("rel", c.grads["We"]),
                        "dbe": ("rel", c.grads["be"]), "dWc": ("rel", c.grads["Wc"]), "dbc": ("rel", c.grads["bc"])}
    run_three(fn)


@pytest.mark.parametrize("B,T,C,p", [(3, 37, 20, 0.4), (1, 70, 257, 0.4), (2, 64, 5, 1.0), (1, 1, 1, 1.0)])
def test_masking_stays_inside(B, T, C, p):
    """frame counts on both sides of a 64-frame chunk, more channels than a workgroup has threads, everything masked, one element"""
    rng = np.random.default_rng(B + T + C)
    x = rng.normal(size=(B, T, C)).astype(np.float32)
    emb = rng.uniform(-1, 1, size=C).astype(np.float32)
    gy = rng.normal(size=(B, T, C)).astype(np.float32)
    mask = (rng.uniform(size=(B, T)) < p).astype(np.uint8)
    sel = mask[:, :, None] != 0

    def fn(r):
        L = r.L
        pm = r.inp("mask", mask, dtype=U8)
        r.ok(L.w2l_cpc_apply_mask(B, T, C, r.inp("x", x), pm, r.inp("emb", emb), r.out("y", (B, T, C)), _stream()), "apply_mask")
        ws = r.work("workspace", L.w2l_cpc_mask_workspace_size(B, T, C))
        r.ok(L.w2l_cpc_apply_mask_backward(B, T, C, r.inp("gy", gy), pm, r.out("dx", (B, T, C)), r.out("demb", (C,)), ws, _stream()), "backward")
        return lambda: {"y": ("exact", np.where(sel, emb[None, None, :], x)), "dx": ("exact", np.where(sel, np.float32(0), gy)),
                        "demb": (("rel", 1e-4), (gy.astype(np.float64) * sel).sum((0, 1)))}
    run_three(fn)
