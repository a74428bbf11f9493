"""Containment of the beam searches with a silence score (w2l_*_beam_search*_sil; DESIGN.md "Containment"), in the manner of
tests/test_gpu_beam_xl_containment.py and on the harness of tests/test_gpu_containment.py: the five entry points (w2l_asg_beam_search_sil
with and without its LM) in each kernel family, on the shapes of tests/test_gpu_beam_sil.py S1 -- B = 3 with ragged frames, T = 16,
N = 7 / 6, K = 64 clipped to all tokens, W = 8 narrow, 96 wide, 1030 xl -- with every operand, result and the workspace of EXACTLY
*_sil_workspace_size bytes in a guarded arena.  Guards intact in the quiet, quiet-again and NaN arenas, identical bytes in all three,
every element of every result written, bit-equal to the float32 restatement of tests/beam_sil_ref.py."""
import numpy as np
import pytest

from tests.test_gpu_containment import I32, _stream, _table, case, run_case

pytestmark = pytest.mark.gpu

SIL_CASES = []


def _beam_sil_case(kind, family, W):
    from tests.test_gpu_beam_sil import B, FRAMES, SIL, SIZES, T, classes
    N, K, M, Lmax, MW, score = classes(kind), 64, 4, 6, 3, -1.5
    name = f"beam/{kind}_sil/family={family},B={B},T={T},N={N},W={W},K={K},nbest={M},maxLen={Lmax}"
    SIL_CASES.append(name)

    @case(name)
    def _(r):
        from tests.test_gpu_beam_sil import s1_case
        from tests.test_gpu_beam_wide import _lex_table, _lm_table
        lib = r.L
        c = s1_case(kind).scored(score)
        frames = np.array(FRAMES, np.int32)
        asg, lm, lex = c.asg, c.tb is not None, c.trie is not None
        nws = getattr(lib, SIZES[kind] + "_sil_workspace_size")(family, B, T, N, W, K)
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
        head = (family, B, T, N, px, pf) + ((pA,) if asg else ()) + (W, K, float("inf"), 0, 0, M, Lmax)
        tail = (ws, _stream(), SIL, score)
        if lex:
            f = lib.w2l_asg_beam_search_lex_sil if asg else lib.w2l_ctc_beam_search_lex_sil
            st = f(*head, plm, eos, c.lmw, plex, c.wsc, c.eos, labels, lengths, scores, lms, MW, words, counts, *tail)
        elif lm or asg:
            f = lib.w2l_asg_beam_search_sil if asg else lib.w2l_ctc_beam_search_lm_sil
            st = f(*head, plm, eos, c.lmw if lm else 0.0, pcls, c.eos if lm else 0.0, labels, lengths, scores, lms, *tail)
        else:
            st = lib.w2l_ctc_beam_search_sil(*head, labels, lengths, scores, *tail)
        r.ok(st, kind)

        def ref():   # bit-exact with logAdd = 0 (the float32 restatement)
            o = c.ref(W, K, M, Lmax, np.float32, float("inf"), False, False, MW)
            out = {key: ("exact", o[key]) for key in ("labels", "lengths", "scores", "lm_scores", "words", "word_counts") if key in o}
            if "lm_scores" not in out:      # the header: without an LM the rows are 0 for live hypotheses and -inf for empty ones
                out["lm_scores"] = ("exact", np.where(o["lengths"] >= 0, np.float32(0), np.float32(-np.inf)))
            return out
        return ref


for _kind in ("ctc", "ctc_lm", "ctc_lex", "asg", "asg_lm", "asg_lex"):
    for _family, _W in ((0, 8), (1, 96), (2, 1030)):
        _beam_sil_case(_kind, _family, _W)


@pytest.mark.parametrize("name", SIL_CASES)
def test_sil_containment(name):
    run_case(name)
