"""Containment of the many-token beam searches (w2l_*_beam_search*_mt; DESIGN.md "Containment"), in the manner of
tests/test_gpu_beam_xl_containment.py and on its harness: the six kinds at B = 2, T = 4, N = 300, W = 130, at K = 65 -- one bit in
the second mask word -- and K = 256 -- four full words --, with every operand, result and the workspace of EXACTLY the declared
bytes in a guarded arena.  Guards intact in the quiet, quiet-again and NaN arenas, identical bytes in all three, every element of
every result written, bit-equal to the float32 restatement."""
import numpy as np
import pytest

from tests.test_gpu_containment import I32, _stream, _table, case, run_case

pytestmark = pytest.mark.gpu

MT_CASES = []


def _beam_mt_case(kind, K):
    B, T, N, W, M, Lmax, MW = 2, 4, 300, 130, 2, 3, 3
    name = f"beam/{kind}_mt/B={B},T={T},N={N},W={W},K={K},nbest={M},maxLen={Lmax}"
    MT_CASES.append(name)

    @case(name)
    def _(r):
        from tests.test_gpu_beam_wide import _dense_case, _lex_table, _lm_table
        lib = r.L
        frames = np.array([T, T - 1], np.int32)
        c = _dense_case(kind, 11, B, T, N, frames, hot=260, nwords=600, max_len=2)
        asg, lm, lex = kind.startswith("asg"), c.tb is not None, c.trie is not None
        fn = lambda stem: getattr(lib, stem + "_mt")
        size = {"ctc": "w2l_ctc_beam", "ctc_lm": "w2l_ctc_beam_lm", "ctc_lex": "w2l_ctc_beam_lex", "asg": "w2l_asg_beam", "asg_lm": "w2l_asg_beam",
                "asg_lex": "w2l_asg_beam_lex"}[kind]
        nws = getattr(lib, size + "_mt_workspace_size")(B, T, N, W, K)
        assert nws > 0
        px, pf = r.inp("x", c.x), r.inp("frames", frames)
        pA = r.inp("trans", c.A) if asg else None
        plm = _table(r, "lm", _lm_table(c.tb)) if lm else None
        plex = _table(r, "lexicon", _lex_table(c.trie)) if lex else None
        pcls = r.inp("classScore", c.cls) if c.cls is not None else None
        eos = int(c.tb.has_eos) if lm else 0
        labels, lengths, scores = r.out("labels", (B, M, Lmax), I32), r.out("lengths", (B, M), I32), r.out("scores", (B, M))
        lms = r.out("lm_scores", (B, M)) if (lm or asg) else None
        words, counts = (r.out("words", (B, M, MW), I32), r.out("word_counts", (B, M), I32)) if lex else (None, None)
        ws = r.work("ws", nws)
        head = (B, T, N, px, pf) + ((pA,) if asg else ()) + (W, K, float("inf"), 0, 0, M, Lmax)
        sil = (-1, 0.0)
        if lex:
            st = fn("w2l_asg_beam_search_lex" if asg else "w2l_ctc_beam_search_lex")(*head, plm, eos, c.lmw, plex, c.wsc, c.eos, labels, lengths, scores, lms,
                                                                                   MW, words, counts, ws, _stream(), *sil)
        elif lm or asg:
            st = fn("w2l_asg_beam_search" if asg else "w2l_ctc_beam_search_lm")(*head, plm, eos, c.lmw if lm else 0.0, pcls, c.eos if lm else 0.0,
                                                                              labels, lengths, scores, lms, ws, _stream(), *sil)
        else:
            st = fn("w2l_ctc_beam_search")(*head, labels, lengths, scores, ws, _stream(), *sil)
        r.ok(st, kind)

        def ref():   # bit-exact with logAdd = 0 (the float32 restatements of tests/*_beam_ref.py)
            o = c.ref(W, K, M, Lmax, np.float32, float("inf"), False, False, MW)
            out = {key: ("exact", o[key]) for key in ("labels", "lengths", "scores", "lm_scores", "words", "word_counts") if key in o}
            if "lm_scores" not in out:      # the header: without an LM the rows are 0 for live hypotheses and -inf for empty ones
                out["lm_scores"] = ("exact", np.where(o["lengths"] >= 0, np.float32(0), np.float32(-np.inf)))
            return out
        return ref


for _kind in ("ctc", "ctc_lm", "ctc_lex", "asg", "asg_lm", "asg_lex"):
    for _K in (65, 256):
        _beam_mt_case(_kind, _K)


@pytest.mark.parametrize("name", MT_CASES)
def test_mt_containment(name):
    run_case(name)
