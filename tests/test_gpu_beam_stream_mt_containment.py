"""Containment of the many-token beam session (w2l_beam_session_create_mt) on the guarded arena of tests/arena.py, by the method of
tests/test_gpu_containment.py (its run_case: guards intact, results independent of the bytes around the operands, every valid
element written, bit-exact against the CPU restatement): step, result and commit stay inside the state of exactly
w2l_beam_session_mt_state_bytes, the scratch of exactly w2l_beam_session_commit_bytes, the emissions and the outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import beam_mt_ref as MR
from tests import beam_stream_mt_cases as MC
from tests import test_gpu_containment as TC
from wav2letter_amd import _lib

pytestmark = pytest.mark.gpu
I32 = torch.int32
NAMES = []


def _session_case(shape, plans, M, Lmax, commit, sil=(-1, 0.0)):
    """plans[s]: the chunk lengths of slot s, step by step (0: idle; the slot starts with its first non-empty chunk)"""
    _, _, T, N, W, K, thr, _ = MC.SHAPES[shape]
    S, Cm, steps = len(plans), max(max(p) for p in plans), len(plans[0])
    fed = [sum(p) for p in plans]
    name = f"beam_session_mt/{shape},S={S},maxChunk={Cm},frames={fed},commit={int(commit)},sil={sil[0]}"
    NAMES.append(name)

    def fn(r):
        lib = r.L
        all_xs = MC.utterances(shape)
        xs = [all_xs[0] if s == 0 else MC.utterances(shape)[0][::-1].copy() if s == 1 else all_xs[1] for s in range(S)]
        xs = [x[:fed[s]] for s, x in enumerate(xs)]
        assert all(len(x) == fed[s] for s, x in enumerate(xs))
        Fmax = max(fed)
        d = _lib.BeamSessionDesc(slots=S, maxChunk=Cm, maxFrames=Fmax, N=N, beam=W, beamToken=K, threshold=thr, logAdd=0, normalize=0,
                                 variant=0, lm=None, lmHasEos=0, lmWeight=0.0, classScore=None, eosScore=0.0, lexicon=None, wordScore=0.0)
        h = C.c_void_p(0)
        r.ok(lib.w2l_beam_session_create_mt(C.byref(d), sil[0], sil[1], C.byref(h)), "create")
        n_lab = np.zeros(S, np.int32)
        try:
            nbytes = lib.w2l_beam_session_mt_state_bytes(C.byref(d))
            r.ok(lib.w2l_beam_session_bind(h, r.work("state", nbytes), nbytes), "bind")
            pos = [0] * S
            for i in range(steps):
                em = np.full((S, Cm, N), np.nan, np.float32)              # rows at or beyond n[s] are nobody's to read
                n, st = np.zeros(S, np.int32), np.zeros(S, np.int32)
                for s_ in range(S):
                    c = plans[s_][i]
                    em[s_, :c] = xs[s_][pos[s_]:pos[s_] + c]
                    n[s_], st[s_] = c, c > 0 and pos[s_] == 0
                    pos[s_] += c
                r.ok(lib.w2l_beam_session_step(h, r.inp(f"emissions{i}", em), n.ctypes.data, st.ctypes.data, TC._stream()), f"step {i}")
            ncb = lib.w2l_beam_session_commit_bytes(h)
            if commit:
                live = np.zeros(S, np.int32)
                clab = r.ar.place((S, Fmax), I32, kind="work", name="commit_labels")[1]   # rows of slots that commit nothing are not written
                r.ok(lib.w2l_beam_session_commit(h, None, r.work("commit_scratch", ncb), ncb, Fmax, clab, 0, None, n_lab.ctypes.data, None,
                                                 live.ctypes.data, TC._stream()), "commit")
            else:       # above beam 1024: no scratch, refused before anything is enqueued
                assert ncb == 0
                assert lib.w2l_beam_session_commit(h, None, None, 0, Fmax, None, 0, None, n_lab.ctypes.data, None, None,
                                                   TC._stream()) == _lib.W2L_EUNSUPPORTED
            r.ok(lib.w2l_beam_session_result(h, M, Lmax, r.out("labels", (S, M, Lmax), I32), r.out("lengths", (S, M), I32), r.out("scores", (S, M)),
                                             r.out("lm_scores", (S, M)), 0, None, None, TC._stream()), "result")
            torch.cuda.synchronize()
            if commit:
                committed = [r.view("commit_labels")[s_, :n_lab[s_]].clone() for s_ in range(S)]
                r.results["committed"] = torch.cat(committed + [torch.tensor(n_lab, device="cuda")])
        finally:
            lib.w2l_beam_session_destroy(h)

        def ref():   # the never-committing search of the whole utterance (tests/beam_mt_ref.py, bit-exact): committed labels + tail rows
            lab, ln, sc, com = np.full((S, M, Lmax), -1, np.int32), np.full((S, M), -1, np.int32), np.full((S, M), -np.inf, np.float32), []
            for s_ in range(S):
                F = xs[s_].shape[0]
                o = MR.mt_beam(xs[s_][None], None, W, K, M, F, sil[0], sil[1], threshold=thr)
                wl, wn, ws_ = o["labels"], o["lengths"], o["scores"]
                nc = int(n_lab[s_])
                com.append(wl[0, 0, :nc])
                sc[s_] = ws_[0]
                for m in range(M):
                    if wn[0, m] >= 0:
                        assert (wl[0, m, :nc] == wl[0, 0, :nc]).all()         # stability: a prefix of every row
                        ln[s_, m] = wn[0, m] - nc
                        rest = wl[0, m, nc:wn[0, m]][:Lmax]
                        lab[s_, m, :len(rest)] = rest
            out = {"labels": ("exact", lab), "lengths": ("exact", ln), "scores": ("exact", sc),
                   "lm_scores": ("exact", np.where(ln >= 0, np.float32(0), np.float32(-np.inf)))}      # W2L_BEAM_PLAIN: 0 live, -inf empty
            if commit:
                out["committed"] = ("exact", np.concatenate(com + [n_lab]))
            return out
        return ref

    TC.CASES[name] = (fn, {}, 64 << 20)


_session_case("peaked_n130_w200_k129", [[5, 3, 4], [0, 4, 3]], 4, 5, True)                          # three mask words, slot 1 idle first
_session_case("peaked_n110_w1500_k100", [[3, 5]], 4, 5, False)                                        # a beam above the wide family's
_session_case("peaked_n70_w65_k65", [[4, 0, 5, 3], [0, 1, 7, 0], [7, 2, 0, 3]], 3, 4, True, (68, -0.5))   # S = 3, ragged counts, a silence score


@pytest.mark.parametrize("name", NAMES)
def test_containment_of_the_many_token_session(name):
    TC.run_case(name)
