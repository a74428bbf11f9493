"""Containment of the lexicon searches with a token LM (w2l_*_beam_search_lextok; DESIGN.md "Containment"), in the manner of
tests/test_gpu_beam_sil_containment.py and on the harness of tests/test_gpu_containment.py: both lattices in both kernel families, on
the shapes of tests/test_gpu_beam_lextok.py K1 -- B = 3 with ragged frames, T = 24, N = 9 / 8, K = 64 clipped to all tokens, W = 8
narrow and 96 wide, with a silence score -- with every operand, result and the workspace of EXACTLY *_lextok_workspace_size bytes in
a guarded arena.  Guards intact in the quiet, quiet-again and NaN arenas, identical bytes in all three, every element of every
result written, bit-equal to the float32 restatement of tests/beam_lextok_ref.py."""
import numpy as np
import pytest

from tests.test_gpu_containment import I32, _stream, _table, case, run_case

pytestmark = pytest.mark.gpu

LEXTOK_CASES = []


def _beam_lextok_case(asg, family, W):
    from tests.test_gpu_beam_lextok import B, ENTRY, FRAMES, SIL, T, classes
    N, K, M, Lmax, MW, score = classes(asg), 64, 4, 6, 3, -1.5
    name = f"beam/{'asg' if asg else 'ctc'}_lextok/family={family},B={B},T={T},N={N},W={W},K={K},nbest={M},maxLen={Lmax}"
    LEXTOK_CASES.append(name)

    @case(name)
    def _(r):
        from tests.test_gpu_beam_lextok import k1_case
        from tests.test_gpu_beam_wide import _lex_table, _lm_table
        lib = r.L
        c = k1_case(asg, "eighths").but(sil=SIL, score=score)
        frames = np.array(FRAMES, np.int32)
        nws = getattr(lib, ENTRY[asg] + "_lextok_workspace_size")(family, B, T, N, W, K)
        assert nws > 0
        px, pf = r.inp("x", c.x), r.inp("frames", frames)
        pA = r.inp("trans", c.A) if asg else None
        plm, plex = _table(r, "lm", _lm_table(c.tb)), _table(r, "lexicon", _lex_table(c.trie))
        labels, lengths, scores = r.out("labels", (B, M, Lmax), I32), r.out("lengths", (B, M), I32), r.out("scores", (B, M))
        lms = r.out("lm_scores", (B, M))
        words, counts = r.out("words", (B, M, MW), I32), r.out("word_counts", (B, M), I32)
        ws = r.work("ws", nws)
        head = (family, B, T, N, px, pf) + ((pA,) if asg else ()) + (W, K, float("inf"), 0, 0, M, Lmax)
        f = getattr(lib, ENTRY[asg] + "_search_lextok")
        st = f(*head, plm, int(c.tb.has_eos), c.lmw, plex, c.wsc, c.eos, labels, lengths, scores, lms, MW, words, counts, ws, _stream(),
               SIL, score)
        r.ok(st, name)

        def ref():   # bit-exact with logAdd = 0 (the float32 restatement)
            o = c.ref(W, K, M, Lmax, np.float32, float("inf"), False, False, MW)
            return {key: ("exact", o[key]) for key in ("labels", "lengths", "scores", "lm_scores", "words", "word_counts")}
        return ref


for _asg in (False, True):
    for _family, _W in ((0, 8), (1, 96)):
        _beam_lextok_case(_asg, _family, _W)


@pytest.mark.parametrize("name", LEXTOK_CASES)
def test_lextok_containment(name):
    run_case(name)
