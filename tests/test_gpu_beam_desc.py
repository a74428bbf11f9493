"""w2l_beam_search on the device: for every route -- (ctc | asg) x (plain, LM, lexicon, token LM under a lexicon) x (narrow, wide,
xl, many-token) -- the descriptor call writes, byte for byte, what the named entry point it stands for writes: labels, lengths,
scores and, where the search has them, lmScores, words and wordCounts; in both logAdd modes, with a silence score and without
(without, also what the plain sibling writes).  criterion.ctc_beam_search / asg_beam_search, which go through the descriptor
call, return the same bytes as the direct named calls.  Shapes: B = 2, T = 12, frames [12, 7], N = 6 (5 tokens for CTC), beam 4,
beamToken 3, nbest 2; one many-token case at N = 70, beamToken 66 (K > 64), T = 6."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR
from tests.test_beam_desc_host import LEX, LEXTOK, LM, MT, NARROW, PLAIN, WIDE, XL, _desc, _named
from tests.test_gpu_beam_wide import F32, INF, _lex_table, _lm_table, _smear

pytestmark = pytest.mark.gpu
SIL, NWORDS = 2, 8
FRAMES = [12, 7]
WIDE_ARG = {NARROW: False, WIDE: True, XL: "xl", MT: "mt"}
SEARCHES = [(asg, kind) for asg in (0, 1) for kind in (PLAIN, LM, LEX, LEXTOK)]
OUT = ("labels", "lengths", "scores", "lmScores", "words", "wordCounts")


class Inputs:
    """one search's inputs on the device and its tables; kind PLAIN with asg: the ASG token search without an LM"""

    def __init__(self, asg, kind, N=6, T=12, frames=FRAMES, seed=0):
        rng = np.random.default_rng(9100 + 10 * asg + kind + seed)
        self.asg, self.kind, self.N, self.T, self.B = asg, kind, N, T, len(frames)
        ntok = N if asg else N - 1
        dev = torch.device("cuda")
        self.x = torch.tensor((rng.integers(-24, 1, size=(self.B, T, N)) / 8).astype(F32), device=dev)
        self.frames = torch.tensor(frames, dtype=torch.int32, device=dev)
        self.A = torch.tensor((rng.integers(-8, 9, size=(N, N)) / 8).astype(F32), device=dev) if asg else None
        self.lm = self.lex = self.cls = None
        if kind == LM:
            self.lm = _lm_table(LR.random_lm(rng, ntok, 2, 12, eighths=True))
            self.cls = torch.tensor((rng.integers(-4, 1, ntok) / 4).astype(F32), device=dev)
        elif kind >= LEX:
            rows = XR.random_lexicon(rng, ntok, NWORDS, 3, 0.0, SIL)
            tb = LR.random_lm(rng, ntok if kind == LEXTOK else NWORDS, 2, 12, eighths=True)
            self.lm = _lm_table(tb)
            self.lex = _lex_table(XR.TextbookTrie(rows, ntok, NWORDS, None if kind == LEXTOK else _smear(tb, NWORDS), SIL))
        self.lm_blob = self.lm.device_blob(dev) if self.lm is not None else None
        self.lex_blob = self.lex.device_blob(dev) if self.lex is not None else None

    def outputs(self, M, Lmax, max_words):
        dev, B = self.x.device, self.B
        o = dict(labels=torch.full((B, M, Lmax), -7, dtype=torch.int32, device=dev),
                 lengths=torch.full((B, M), -7, dtype=torch.int32, device=dev), scores=torch.full((B, M), 7.0, device=dev))
        if self.kind != PLAIN or self.asg:
            o["lmScores"] = torch.full((B, M), 7.0, device=dev)
        if self.kind >= LEX:
            o["words"] = torch.full((B, M, max_words), -7, dtype=torch.int32, device=dev)
            o["wordCounts"] = torch.full((B, M), -7, dtype=torch.int32, device=dev)
        return o

    def args(self, o, ws, W, K, M, Lmax, max_words, log_add, sil):
        """the argument dict of tests/test_beam_desc_host.py, on device pointers"""
        p = lambda t: t.data_ptr() if t is not None else None
        a = dict(B=self.B, T=self.T, N=self.N, input=p(self.x), frames=p(self.frames), trans=p(self.A), beam=W, beamToken=K, threshold=INF,
                 logAdd=int(log_add), normalize=int(log_add and not self.asg), nbest=M, maxLen=Lmax, lm=p(self.lm_blob),
                 lmHasEos=int(self.lm.has_eos) if self.lm is not None else 0, lmWeight=0.5 if self.lm is not None else 0.0,
                 classScore=p(self.cls), eosScore=-0.25 if self.lm is not None and self.lm.has_eos else 0.0, lexicon=p(self.lex_blob),
                 wordScore=-0.25 if self.lex is not None else 0.0, labels=p(o["labels"]), lengths=p(o["lengths"]), scores=p(o["scores"]),
                 lmScores=p(o.get("lmScores")), maxWords=max_words if self.lex is not None else 0, words=p(o.get("words")),
                 wordCounts=p(o.get("wordCounts")), workspace=p(ws), silToken=sil[0], silScore=sil[1])
        return a

    def run(self, how, family, W, K, M, Lmax, log_add, sil, max_words=5):
        """how: a route of the named entry points ("named", "sil", "mt", "lextok") or "desc" -> {output: numpy array}.  Both run on
        the null stream, as tests/test_beam_desc_host.py's callers pass it: torch's current stream here"""
        from wav2letter_amd import _lib as L
        lib = L.lib()
        o = self.outputs(M, Lmax, max_words)
        a = self.args(o, None, W, K, M, Lmax, max_words, log_add, sil)
        nkind = LM if self.asg and self.kind == PLAIN else self.kind   # the named ASG token search takes lm == NULL
        if how == "desc":
            d = _desc(family, self.kind, a)
            nws = lib.w2l_beam_search_workspace_size(C.byref(d))
            assert nws > 0
            ws = torch.empty(nws, dtype=torch.uint8, device=self.x.device)
            L.check(lib.w2l_beam_search(C.byref(d), ws.data_ptr(), None), "w2l_beam_search")
        else:
            search, size = _named(self.asg, nkind, how, family)
            nws = size(a)
            assert nws > 0
            ws = torch.empty(nws, dtype=torch.uint8, device=self.x.device)
            a["workspace"] = ws.data_ptr()
            L.check(search(a), how)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in o.items()}

    def front_end(self, family, W, K, M, Lmax, log_add, sil, max_words=5):
        from wav2letter_amd import criterion
        kw = dict(beam=W, beam_token=K, threshold=INF, log_add=bool(log_add), normalize=bool(log_add and not self.asg), nbest=M,
                  max_len=Lmax, wide=WIDE_ARG[family], sil_token=sil[0], sil_score=sil[1])
        if self.lm is not None:
            kw.update(lm=self.lm, lm_weight=0.5, eos_score=-0.25 if self.lm.has_eos else 0.0)
        if self.cls is not None:
            kw.update(class_score=self.cls)
        if self.lex is not None:
            kw.update(lexicon=self.lex, word_score=-0.25, max_words=max_words, lm_token=self.kind == LEXTOK)
        if self.asg:
            out = criterion.asg_beam_search(self.x, self.A, self.frames, **kw)
        else:
            out = criterion.ctc_beam_search(self.x, self.frames, **kw)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in zip(OUT, out)}


def _same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])


@functools.lru_cache(maxsize=None)
def inputs(asg, kind):
    return Inputs(asg, kind)


def _route(kind, family):
    return "lextok" if kind == LEXTOK else "mt" if family == MT else "sil"


@pytest.mark.parametrize("asg,kind", SEARCHES, ids=[f"{'asg' if a else 'ctc'}-{('plain', 'lm', 'lex', 'lextok')[k]}" for a, k in SEARCHES])
def test_descriptor_call_writes_the_named_entry_points_bytes(asg, kind):
    c = inputs(asg, kind)
    W, K, M, Lmax = 4, 3, 2, 12
    seen = 0
    for family in ((NARROW, WIDE) if kind == LEXTOK else (NARROW, WIDE, XL, MT)):
        for log_add in (0, 1):
            for sil in ((SIL, -0.5), (-1, 0.0), (SIL, 0.0)):
                what = (asg, kind, family, log_add, sil)
                want = c.run(_route(kind, family), family, W, K, M, Lmax, log_add, sil)
                _same(c.run("desc", family, W, K, M, Lmax, log_add, sil), want, what)
                if sil[1] == 0.0 and kind != LEXTOK and family != MT:   # without a score: the plain sibling
                    _same(c.run("named", family, W, K, M, Lmax, log_add, sil), want, what)
                if sil[0] == SIL:
                    front = c.front_end(family, W, K, M, Lmax, log_add, sil)
                    _same(front, {k: v for k, v in want.items() if k in front}, what)
                    assert set(want) - set(front) <= ({"lmScores"} if asg and kind == PLAIN else set())
                seen += int((want["lengths"] >= 0).sum())
    assert seen > 0   # live hypotheses were compared, not empty rows alone


def test_descriptor_call_many_tokens_above_64():
    """N = 70, beamToken 66: K = 66 (ASG) and 66 (CTC, 69 tokens) frame tokens, more than one mask word"""
    W, K, M, Lmax = 4, 66, 2, 6
    for asg in (0, 1):
        for kind in (PLAIN, LM):
            c = Inputs(asg, kind, N=70, T=6, frames=[6, 4], seed=50)
            for log_add in (0, 1):
                for sil in ((SIL, -0.5), (-1, 0.0)):
                    want = c.run("mt", MT, W, K, M, Lmax, log_add, sil)
                    _same(c.run("desc", MT, W, K, M, Lmax, log_add, sil), want, (asg, kind, log_add, sil))
                    assert (want["lengths"] >= 0).any()
            front = c.front_end(MT, W, K, M, Lmax, 0, (SIL, -0.5))
            want = c.run("mt", MT, W, K, M, Lmax, 0, (SIL, -0.5))
            _same(front, {k: v for k, v in want.items() if k in front}, (asg, kind, "front end"))
