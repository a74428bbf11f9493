"""The LM-fused seq2seq decoder against the float64 restatement tests/s2s_decode_lm_ref.py.  The bar is the project's
fp32 bar, 1e-4 of the tensor's largest reference magnitude; tokens and lengths are compared exactly, which
tests/test_s2s_decode_lm_host.py makes a fair demand.  One run in the guarded arenas of tests/arena.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import s2s_decode_lm_ref as DL
import s2s_decode_ref as D
from tests.test_gpu_containment import _stream, _table
from tests.test_gpu_cpc_containment import run_three
from tests.test_gpu_s2s_decode import close, dev, operand_pointers
from wav2letter_amd import NGramLM, _lib, ops

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def table(name):
    tb = DL.run_case(name)[4]
    return NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk))


@pytest.mark.parametrize("name", DL.CASES)
def test_search(name):
    p, enc, kl, keyvalue, _, weight, opt, _, want = DL.run_case(name)
    dp, denc = dev(p, enc)
    run = lambda e, k, w: ops.s2s_decode(dp, e, k, keyvalue, eos=D.EOS, lm=table(name), lm_weight=w, **opt)
    runs = [run(denc, kl, weight) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))                       # two calls: the same bits
    tokens, lengths, scores, lm_scores = (x.cpu().numpy() for x in runs[0])
    assert np.array_equal(tokens, want[0]) and np.array_equal(lengths, want[1]), (tokens, want[0])
    there = np.isfinite(want[2])
    assert np.array_equal(np.isneginf(scores), ~there) and np.array_equal(np.isneginf(lm_scores), ~there)
    close(scores[there], want[2][there], "scores"), close(lm_scores[there], want[3][there], "lm scores")
    alone = run(denc[:1], kl[:1], weight)                                      # utterance 0 alone: the bits it has in the batch
    assert all(torch.equal(x[0], y[0]) for x, y in zip(alone, runs[0]))
    free = ops.s2s_decode(dp, denc, kl, keyvalue, eos=D.EOS, **opt)            # a zero weight: the LM-free entry point's bits
    assert all(torch.equal(x, y) for x, y in zip(run(denc, kl, 0.0)[:3], free))


def test_search_stays_inside(name="trigram_backoff"):
    """every table, state and list of the search lives in a workspace of exactly the declared bytes, which starts as NaN in the third
    run; the blob and the operands are only read (frames ldenc = C + 3 apart); every element of the four results is written"""
    p, enc, kl, keyvalue, _, weight, opt, _, want = DL.run_case(name)
    (B, T, Cc), (N, H), U, nbest = enc.shape, p[0].shape, opt["max_len"], opt["nbest"]
    d = _lib.S2sDecodeDesc(B, T, H, N, Cc + 3, D.EOS, opt["beam"], opt["beam_token"], U, nbest, float("inf"), opt["eos_score"], 1.0, -1, weight)
    assert np.abs(want[2]).max() >= 1 and np.abs(want[3]).max() >= 1   # so the "loss" bar is 1e-4 of the largest magnitude here

    def fn(r):
        L, dp = r.L, ctypes.byref(d)
        nb = L.w2l_s2s_decode_lm_workspace_size(dp)
        ptrs = operand_pointers(r, p, enc, kl, keyvalue)
        ptrs += [r.out("tokens", (B, nbest, U), torch.int32), r.out("lengths", (B, nbest), torch.int32), r.out("scores", (B, nbest)),
                 r.out("lmScores", (B, nbest))]
        r.ok(L.w2l_s2s_decode_lm(dp, *ptrs, r.work("workspace", nb), nb, _stream(), _table(r, "lm", table(name)), int(table(name).has_eos)), "decode")
        return lambda: dict(zip(("tokens", "lengths", "scores", "lmScores"), zip(("exact", "exact", "loss", "loss"), want)))
    run_three(fn)
