"""The silence score of the five beam searches (w2l_*_beam_search*_sil) on the GPU, in the three kernel families, on the machinery
of tests/test_gpu_beam_wide.py and against tests/beam_sil_ref.py.
S1 = I2 on the device: at K = all and normalize = 0 every output equals, bit for bit, the sibling's on emissions whose sil column
was biased on the host in fp32; S2 the selection case at K = 3 against the float32 restatement, bit for bit; S3 = I3 the families
agree; S4 normalize = 1 and logAdd = 1 against the float64 restatement; S5 = I1 no score is the sibling's bytes; S6 the narrow
LM-free CTC call, which leaves the lazy scan; S7 the three surfaces; S8 Decode --w2l_silscore.
Shapes: B = 3 with ragged frames, T = 16, CTC N = 7 (6 tokens and blank), ASG N = 6 with random transitions, sil = token 2; a lexicon
of 12 words with sil, a homophone pair, a word that is a prefix of another and a spelling that ends on sil; 2-gram LMs."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import beam_sil_ref as SR
from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR
from tests.test_beam_sil_host import SELECTION_SEED
from tests.test_gpu_beam_wide import F32, INF, KEYS, KINDS, ROOT, Case, _delta, _lex_table, _lm_table, _same_bits, _smear

pytestmark = pytest.mark.gpu
SIL = 2
B, T, FRAMES = 3, 16, [16, 1, 11]
FAMILIES = {0: False, 1: True, 2: "xl"}                    # family -> the front end's `wide`
WIDTHS = [(0, 8), (1, 8), (1, 96), (2, 8), (2, 96), (2, 1030)]
SIZES = {"ctc": "w2l_ctc_beam", "ctc_lm": "w2l_ctc_beam_lm", "ctc_lex": "w2l_ctc_beam_lex", "asg": "w2l_asg_beam", "asg_lm": "w2l_asg_beam",
         "asg_lex": "w2l_asg_beam_lex"}


def classes(kind):
    return 6 if kind.startswith("asg") else 7


def lexicon_rows(rng, ntok):
    """9 random words, then a homophone of word 0, a word that continues word 1's spelling, and a spelling that ends on sil"""
    rows = XR.random_lexicon(rng, ntok, 9, 3, 0.0, SIL)
    cont = next(t for t in range(ntok) if t != rows[1][1][-1] and tuple(rows[1][1] + [t]) not in {tuple(sp) for _, sp in rows})
    have = {tuple(sp) for _, sp in rows}
    ends = next(sp for sp in ([t, SIL] for t in range(ntok) if t != SIL) if tuple(sp) not in have and sp != rows[1][1] + [cont])
    rows += [(9, list(rows[0][1])), (10, rows[1][1] + [cont]), (11, ends)]
    sps = [tuple(sp) for _, sp in rows]
    assert len(set(sps)) == len(sps) - 1                                       # one homophone pair
    assert any(a != b and a == b[:len(a)] for a in sps for b in sps)           # a word that is a prefix of another
    assert any(sp[-1] == SIL for sp in sps) and all(sp[0] != SIL for sp in sps)
    return rows


class SilCase(Case):
    """tests/test_gpu_beam_wide.py's Case with the silence token and score; score None: the sibling's call"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.score = None

    def scored(self, score, sil=SIL):
        c = SilCase(self.kind, self.x, self.frames, self.A, self.tb, self.trie, self.cls, self.lmw, self.wsc, self.eos)
        c.score, c.sil = score, sil
        for k in ("_lm", "_lex"):
            if hasattr(self, k):
                setattr(c, k, getattr(self, k))
        return c

    def on(self, x):
        c = self.scored(self.score, getattr(self, "sil", SIL))
        c.x = x
        return c

    def tables(self):
        if self.tb is not None and not hasattr(self, "_lm"):
            self._lm = _lm_table(self.tb)
        if self.trie is not None and not hasattr(self, "_lex"):
            self._lex = _lex_table(self.trie)

    def gpu(self, W, K, M, Lmax, wide, threshold=INF, log_add=False, normalize=False, max_words=None):
        from wav2letter_amd import criterion
        if self.score is None:
            return super().gpu(W, K, M, Lmax, wide, threshold, log_add, normalize, max_words)
        self.tables()
        xd = torch.tensor(self.x, device="cuda")
        fd = torch.tensor(self.frames, dtype=torch.int32, device="cuda") if self.frames is not None else None
        kw = dict(beam=W, beam_token=K, threshold=threshold, log_add=log_add, normalize=normalize, nbest=M, max_len=Lmax, wide=wide,
                  sil_token=self.sil, sil_score=self.score)
        if self.tb is not None:
            kw.update(lm=self._lm, lm_weight=self.lmw, eos_score=self.eos)
            if self.cls is not None:
                kw.update(class_score=torch.tensor(self.cls, device="cuda"))
        if self.trie is not None:
            kw.update(lexicon=self._lex, word_score=self.wsc, max_words=max_words)
        if self.asg:
            out = criterion.asg_beam_search(xd, torch.tensor(self.A, device="cuda"), fd, **kw)
        else:
            out = criterion.ctc_beam_search(xd, fd, **kw)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in zip(KEYS, out)}

    def abi(self, family, W, K, M, Lmax, threshold=INF, log_add=False, normalize=False, max_words=None):
        """the C ABI's *_sil entry point itself -> {key: numpy array}"""
        from wav2letter_amd import _lib as L
        lib = L.lib()
        self.tables()
        Bc, Tc, N = self.x.shape
        dev = torch.device("cuda")
        st = torch.cuda.current_stream().cuda_stream
        xd = torch.tensor(self.x, device=dev)
        fd = torch.tensor(self.frames, dtype=torch.int32, device=dev) if self.frames is not None else None
        Ad = torch.tensor(self.A, device=dev) if self.asg else None
        mw = Lmax if max_words is None else max_words
        o = dict(labels=torch.full((Bc, M, Lmax), -7, dtype=torch.int32, device=dev), lengths=torch.full((Bc, M), -7, dtype=torch.int32, device=dev),
                 scores=torch.full((Bc, M), 7.0, device=dev))
        lm = self._lm.device_blob(dev) if self.tb is not None else None
        if self.tb is not None or self.asg:
            o["lm_scores"] = torch.full((Bc, M), 7.0, device=dev)
        if self.trie is not None:
            lex = self._lex.device_blob(dev)
            o["words"] = torch.full((Bc, M, mw), -7, dtype=torch.int32, device=dev)
            o["word_counts"] = torch.full((Bc, M), -7, dtype=torch.int32, device=dev)
        nws = getattr(lib, SIZES[self.kind] + "_sil_workspace_size")(family, Bc, Tc, N, W, K)
        assert nws > 0
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        p = lambda t: t.data_ptr() if t is not None else None
        head = (family, Bc, Tc, N, p(xd), p(fd)) + ((p(Ad),) if self.asg else ()) + (W, K, threshold, int(log_add), int(normalize), M, Lmax)
        tail = (p(ws), st, self.sil, float(self.score))
        eos = int(self.tb.has_eos) if self.tb is not None else 0
        cls = torch.tensor(self.cls, device=dev) if self.cls is not None else None
        if self.trie is not None:
            f = lib.w2l_asg_beam_search_lex_sil if self.asg else lib.w2l_ctc_beam_search_lex_sil
            rc = f(*head, p(lm), eos, self.lmw, p(lex), self.wsc, self.eos, p(o["labels"]), p(o["lengths"]), p(o["scores"]),
                   p(o["lm_scores"]), mw, p(o["words"]), p(o["word_counts"]), *tail)
        elif self.tb is not None or self.asg:
            f = lib.w2l_asg_beam_search_sil if self.asg else lib.w2l_ctc_beam_search_lm_sil
            rc = f(*head, p(lm), eos, self.lmw, p(cls), self.eos, p(o["labels"]), p(o["lengths"]), p(o["scores"]), p(o["lm_scores"]), *tail)
        else:
            rc = lib.w2l_ctc_beam_search_sil(*head, p(o["labels"]), p(o["lengths"]), p(o["scores"]), *tail)
        L.check(rc, "beam_search_sil")
        torch.cuda.synchronize()
        if self.asg and self.tb is None:
            del o["lm_scores"]
        return {k: t.cpu().numpy() for k, t in o.items()}

    def ref(self, W, K, M, Lmax, dtype, threshold=INF, log_add=False, normalize=False, max_words=None):
        if self.score is None:
            return super().ref(W, K, M, Lmax, dtype, threshold, log_add, normalize, max_words)
        kw = dict(threshold=threshold, log_add=log_add, normalize=normalize)
        if self.asg:
            kw["A"] = self.A
        if self.tb is not None:
            kw.update(lm=self.tb, lm_weight=self.lmw, eos_score=self.eos)
        if self.trie is not None:
            kw.update(trie=self.trie, word_score=self.wsc)
        elif self.cls is not None:
            kw.update(class_score=self.cls)
        o = SR.sil_beam(self.x, self.frames, W, K, M, Lmax, self.sil, self.score, dtype, max_words, **kw)
        if self.tb is None:
            del o["lm_scores"]
        return o


def make_case(kind, seed, x=None, eighths=True, frames=FRAMES, t=T):
    """the shapes of the module docstring.  eighths: emissions, transitions, LM and smear values multiples of 1/8, lmWeight 1/2,
    word and EOS scores multiples of 1/4, so every fp32 sum is exact and ties are dense; else normal values"""
    rng = np.random.default_rng(seed)
    N = classes(kind)
    asg = kind.startswith("asg")
    ntok = N if asg else N - 1
    if x is None:
        x = (rng.integers(-24, 1, size=(len(frames), t, N)) / 8).astype(F32) if eighths else rng.normal(0, 2, size=(len(frames), t, N)).astype(F32)
    A = None
    if asg:
        A = (rng.integers(-8, 9, size=(N, N)) / 8).astype(F32) if eighths else rng.normal(0, 1, size=(N, N)).astype(F32)
    if kind.endswith("lex"):
        rows = lexicon_rows(rng, ntok)
        tb = LR.random_lm(rng, 12, 2, 40, eighths=eighths)
        trie = XR.TextbookTrie(rows, ntok, 12, _smear(tb, 12), SIL)
        return SilCase(kind, x, frames, A, tb, trie, None, 0.5, -0.25, -0.25)
    if kind.endswith("lm"):
        tb = LR.random_lm(rng, ntok, 2, 20, eighths=eighths)
        cls = (rng.integers(-4, 1, ntok) / 4).astype(F32)
        return SilCase(kind, x, frames, A, tb, None, cls, 0.5, 0.0, -0.25)
    return SilCase(kind, x, frames, A)


@functools.lru_cache(maxsize=None)
def s1_case(kind):
    return make_case(kind, 500 + KINDS.index(kind))


# ---- S1 = I2 on the device -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("family,W", WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_s1_equals_the_sibling_on_biased_emissions_bit_for_bit(kind, family, W, log_add):
    c = s1_case(kind)
    M, Lmax = min(W, 16), 6
    for score in (-1.5, 0.75):
        got = c.scored(score).gpu(W, 64, M, Lmax, FAMILIES[family], INF, log_add, False, 3)
        want = c.on(SR.bias_column(c.x, SIL, score)).gpu(W, 64, M, Lmax, FAMILIES[family], INF, log_add, False, 3)
        plain = c.gpu(W, 64, M, Lmax, FAMILIES[family], INF, log_add, False, 3)
        assert (want["lengths"] >= 0).any()
        _same_bits(got, want)
        assert any((plain[k].view(np.int32) != got[k].view(np.int32)).any() for k in ("labels", "scores"))   # the score acts


def test_s1_asg_max_search_is_viterbi_on_the_biased_emissions():
    """the ASG max search without LM at a beam that never cuts: w2l_viterbi_compute's path and score on the biased emissions"""
    from tests import asg_beam_ref as AR
    c = s1_case("asg")
    for score in (-1.5, 0.75):
        got = c.scored(score).gpu(1030, 64, 1, T, "xl")
        xb = SR.bias_column(c.x, SIL, score)
        for b, F in enumerate(FRAMES):
            path, s = AR.viterbi(xb[b, :F], c.A)
            want = AR.collapse(path)
            assert got["lengths"][b, 0] == len(want) and tuple(got["labels"][b, 0, :len(want)]) == want
            assert got["scores"][b, 0].view(np.int32) == np.float32(s).view(np.int32)


# ---- S2: the selection case, K = 3 -----------------------------------------------------------------------------------------------

# emission seeds at which the restatement's eight output rows differ from bias-before-selection in both directions (found on the
# CPU, asserted by test_s2_the_case_tells_the_two_rules_apart; with -8 the penalised sil candidate must still enter the beam to show)
S2_SEEDS = {"ctc": 10, "ctc_lm": SELECTION_SEED, "ctc_lex": SELECTION_SEED, "asg": SELECTION_SEED, "asg_lm": 10, "asg_lex": 12}


@functools.lru_cache(maxsize=None)
def s2_case(kind):
    N = classes(kind)
    rng = np.random.default_rng(S2_SEEDS[kind])
    x = SR.selection_case(rng, B, T, N, SIL, N if kind.startswith("asg") else N - 1)
    return make_case(kind, 520 + KINDS.index(kind), x=x)


@pytest.mark.parametrize("score", [8.0, -8.0])
@pytest.mark.parametrize("kind", KINDS)
def test_s2_selection_case_bitwise_against_the_float32_restatement(kind, score):
    c = s2_case(kind).scored(score)
    W, K, M, Lmax = 8, 3, 8, T
    want = c.ref(W, K, M, Lmax, F32, INF, False, False, 4)
    pre = c.scored(None).on(SR.bias_column(c.x, SIL, score)).ref(W, K, M, Lmax, F32, INF, False, False, 4)
    differs = any((pre[k].view(np.int32) != want[k].view(np.int32)).any() for k in ("labels", "scores"))
    got = c.gpu(W, K, M, Lmax, False, INF, False, False, 4)
    print("S2", kind, score, "differs from bias-before-selection:", differs, "live rows", int((want["lengths"] >= 0).sum()))
    assert want["scores"].dtype == F32 and (want["lengths"] >= 0).any()
    _same_bits(got, {k: v for k, v in want.items() if k != "diags"})
    _same_bits(c.abi(0, W, K, M, Lmax, INF, False, False, 4), got)


def test_s2_the_case_tells_the_two_rules_apart():
    for kind in KINDS:
        for score in (8.0, -8.0):
            c = s2_case(kind).scored(score)
            want = c.ref(8, 3, 8, T, F32, INF, False, False, 4)
            pre = c.scored(None).on(SR.bias_column(c.x, SIL, score)).ref(8, 3, 8, T, F32, INF, False, False, 4)
            assert any((pre[k].view(np.int32) != want[k].view(np.int32)).any() for k in ("labels", "scores")), (kind, score)


# ---- S3 = I3: the families agree -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("K", [3, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_s3_the_three_families_agree_bit_for_bit(kind, K, log_add):
    c = s1_case(kind).scored(-1.5)
    norm = log_add and not c.asg
    narrow = c.gpu(8, K, 8, 5, False, 6.0, log_add, norm, 2)
    wide8 = c.gpu(8, K, 8, 5, True, 6.0, log_add, norm, 2)
    xl8 = c.gpu(8, K, 8, 5, "xl", 6.0, log_add, norm, 2)
    assert (narrow["lengths"] >= 0).any()
    _same_bits(wide8, narrow)
    _same_bits(xl8, wide8)
    _same_bits(c.gpu(96, K, 96, 5, "xl", 6.0, log_add, norm, 2), c.gpu(96, K, 96, 5, True, 6.0, log_add, norm, 2))
    n64, w64 = c.gpu(64, K, 64, 5, False, 6.0, log_add, norm, 2), c.gpu(64, K, 64, 5, True, 6.0, log_add, norm, 2)
    _same_bits(w64, n64)


# ---- S4: normalize = 1, logAdd = 1 against the float64 restatement ----------------------------------------------------------------

# seeds at which the restatement's own Diags qualify every utterance (ctc_lm: all but one of nine), found on the CPU
S4_SEEDS = {"ctc": 0, "ctc_lm": 2, "ctc_lex": 0, "asg": 1, "asg_lm": 0, "asg_lex": 0}
S4_WIDTHS = [(0, 8), (1, 96), (2, 1030)]
S4_K, S4_M = 4, 2


@functools.lru_cache(maxsize=None)
def s4_reference(kind, W):
    """the float64 restatement and, per utterance, whether its decisions have ten times the bound delta of room (the kind's own
    delta of tests/test_gpu_beam_wide.py), by the rules of tests/test_gpu_ctc_beam.py: the frame tokens and the final gaps always;
    then either T3's -- every decision of every frame, the dropped tail included -- or, where the tail is dense (a beam of 96 or
    1030 over 6 tokens), T4's -- the ancestors of the compared hypotheses survived every selection with that room, and a beam one
    narrower or one wider returns the same rows.  The other utterances are not compared"""
    c = make_case(kind, 540 + S4_SEEDS[kind], eighths=False).scored(-1.5)
    want = c.ref(W, S4_K, S4_M, T, np.float64, INF, True, True, T)
    near, ok = None, []
    for b, dg in enumerate(want["diags"]):
        dl = _delta(kind, T, dg.S)
        t3 = dg.decision_gap() >= 10 * dl
        t4 = not t3 and min(dg.margins, default=INF) >= 10 * dl
        if t4:
            near = near or [c.ref(w, S4_K, S4_M, T, np.float64, INF, True, True, T) for w in (W - 1, W + 1)]
            t4 = all((o[k][b] == want[k][b]).all() for o in near for k in ("labels", "scores"))
        ok.append(dg.token_gap >= 10 * dl and min(dg.final_gaps, default=INF) >= 10 * dl and (t3 or t4))
    return c, want, ok


def test_s4_the_rule_discards_at_most_a_quarter():
    total = kept = 0
    for kind in KINDS:
        for _, W in S4_WIDTHS:
            ok = s4_reference(kind, W)[2]
            total, kept = total + len(ok), kept + sum(ok)
    print("S4 compared utterances", kept, "of", total)
    assert 4 * (total - kept) <= total


@pytest.mark.parametrize("family,W", S4_WIDTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_s4_log_sum_search_against_the_float64_restatement(kind, family, W):
    c, want, ok = s4_reference(kind, W)
    got = c.gpu(W, S4_K, S4_M, T, FAMILIES[family], INF, True, True, T)
    for b in range(B):
        if not ok[b]:
            continue
        for k in ("labels", "lengths", "words", "word_counts"):
            if k in want:
                assert (got[k][b] == want[k][b]).all(), (kind, W, b, k)
        g, w = got["scores"][b].astype(np.float64), want["scores"][b]
        fin = np.isfinite(w)
        assert (np.isfinite(g) == fin).all() and (np.abs(g[fin] - w[fin]) <= 1e-4 * np.maximum(1.0, np.abs(w[fin]))).all(), (kind, W, b)
        print("S4", kind, W, b, "max |score diff|", float(np.abs(g[fin] - w[fin]).max(initial=0.0)))


# ---- S5 = I1: no score is the sibling's bytes ------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,W", [(0, 8), (1, 96), (2, 1030)])
@pytest.mark.parametrize("kind", KINDS)
def test_s5_no_score_is_the_sibling_byte_for_byte(kind, family, W):
    c = s1_case(kind)
    for log_add in (False, True):
        want = c.gpu(W, 4, 8, 6, FAMILIES[family], 6.0, log_add, log_add and not c.asg, 3)
        for sil, score in ((SIL, 0.0), (-1, 3.0), (SIL, -0.0)):
            _same_bits(c.scored(score, sil).gpu(W, 4, 8, 6, FAMILIES[family], 6.0, log_add, log_add and not c.asg, 3), want)
            _same_bits(c.scored(score, sil).abi(family, W, 4, 8, 6, 6.0, log_add, log_add and not c.asg, 3), want)


# ---- S6: the narrow LM-free CTC call leaves the lazy scan ------------------------------------------------------------------------

@pytest.mark.parametrize("score", [-1.5, 0.75, 8.0])
def test_s6_narrow_lm_free_ctc_on_the_token_scan(score):
    W, K, T6 = 64, 6, 40
    frames = [40, 1, 27]
    c = make_case("ctc", 560, frames=frames, t=T6).scored(score)
    want = c.ref(W, K, W, T6, F32, INF, False, False)
    assert any(d.beam_gap < INF for d in want["diags"])                        # the beam binds
    got = c.gpu(W, K, W, T6, False)
    _same_bits(got, {k: v for k, v in want.items() if k != "diags"})
    _same_bits(c.gpu(W, K, W, T6, True), got)
    # with a threshold line and the log-sum on normalised rows: the wide family's bytes
    for log_add in (False, True):
        _same_bits(c.gpu(W, K, 4, 9, False, 5.0, log_add, log_add), c.gpu(W, K, 4, 9, True, 5.0, log_add, log_add))


# ---- S7: the three surfaces ------------------------------------------------------------------------------------------------------

def test_s7_three_surfaces_agree(tmp_path):
    """C ABI == Python (criterion.*_beam_search, CTCLoss / ASGLoss.beamSearch) == compiled C++ beamSearch with
    BeamSearchOptions::silToken / silScore (tests/cpp/decode_sil_caller.cpp, built by tests/cpp/decode_sil_caller.mk), the LM and the lexicon read from the same files"""
    from tests.test_ctc_beam_lm_host import _arpa_text
    from wav2letter_amd import ASGLoss, CTCLoss, Lexicon, NGramLM, text
    subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "decode_sil_caller.mk", "decode_sil_caller", f"OUT={tmp_path}"],
                   check=True, capture_output=True)
    exe = str(tmp_path / "decode_sil_caller")
    score = -1.5
    for i, kind in enumerate(("ctc", "ctc_lm", "ctc_lex", "asg", "asg_lm", "asg_lex")):
        family = i % 3
        W = (8, 96, 1030)[family]
        base = make_case(kind, 580 + i)
        N = classes(kind)
        ntok = N if base.asg else N - 1
        tokens = [f"t{c}" for c in range(ntok)]
        d = tmp_path / kind
        d.mkdir()
        (d / "tokens.txt").write_text("\n".join(tokens) + "\n")
        args = []
        c = base.scored(score)
        if base.trie is not None:
            (d / "lex.txt").write_text("".join(f"word{w:02d} " + " ".join(tokens[t] for t in sp) + "\n" for w, sp in base.trie.rows))
            dic = text.Dictionary(tokens)
            plain = Lexicon.from_file(d / "lex.txt", dic, smearing="none", sil=tokens[SIL])
            (d / "lm.arpa").write_text(_arpa_text(base.tb, plain.words, unk10=-3.0)[0])
            c._lm = NGramLM.from_arpa(d / "lm.arpa", plain.words)
            c._lex = Lexicon.from_file(d / "lex.txt", dic, lm=c._lm, sil=tokens[SIL])
            assert c._lex.sil == SIL
            args = [str(d / "tokens.txt"), str(d / "lm.arpa"), str(d / "lex.txt"), tokens[SIL], "0"]
        elif base.tb is not None:
            (d / "lm.arpa").write_text(_arpa_text(base.tb, tokens, unk10=-3.0)[0])
            c._lm = NGramLM.from_arpa(d / "lm.arpa", tokens)
            c.cls = None
            args = [str(d / "tokens.txt"), str(d / "lm.arpa")]
        M, Lmax, maxw, thr = 4, 6, 3, 8.0
        want = c.abi(family, W, 4, M, Lmax, thr, False, False, maxw)
        assert (want["lengths"] >= 0).any()
        _same_bits(c.gpu(W, 4, M, Lmax, FAMILIES[family], thr, False, False, maxw), want)
        if base.trie is not None:                                               # sil_token=None: the lexicon's
            _same_bits(c.scored(score, None).gpu(W, 4, M, Lmax, FAMILIES[family], thr, False, False, maxw), want)
        xd, fd = torch.tensor(c.x, device="cuda"), torch.tensor(np.array(FRAMES, np.int32), device="cuda")
        opts = dict(beam=W, beam_token=4, threshold=thr, nbest=M, max_len=Lmax, wide=FAMILIES[family], sil_token=SIL, sil_score=score)
        if base.tb is not None:
            opts.update(lm=c._lm, lm_weight=c.lmw, eos_score=c.eos)
        if base.trie is not None:
            opts.update(lexicon=c._lex, word_score=c.wsc, max_words=maxw)
        if base.asg:
            crit = ASGLoss(N).cuda()
            with torch.no_grad():
                crit.transitions.copy_(torch.tensor(c.A))
        else:
            crit = CTCLoss()
        got = crit.beamSearch(xd, fd, normalize=False, **opts)
        keys = [k for k in KEYS if k in want]
        assert len(got) == len(keys) and all((g.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all() for g, k in zip(got, keys))
        inp, outp = str(d / "in.bin"), str(d / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([N, T, B, W, 4, M, Lmax, maxw, 0, 0, int(base.asg), family, -1 if base.trie is not None else SIL], np.int32).tobytes()
                    + np.array([thr, c.lmw, c.wsc, c.eos, score], F32).tobytes() + c.x.tobytes() + np.array(FRAMES, np.int32).tobytes()
                    + (c.A.tobytes() if base.asg else b""))
        run = subprocess.run([exe, inp, outp] + args, capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "decode sil caller ok" in run.stdout, (kind, run.returncode, run.stdout, run.stderr)
        out = np.fromfile(outp, np.int32)
        at = 0
        for k in keys:
            n = want[k].size
            assert (out[at:at + n] == want[k].view(np.int32).ravel()).all(), (kind, k)
            at += n
        assert at == len(out)


# ---- S8: Decode --w2l_silscore end to end, on the ASG fixture of tests/test_gpu_asg_beam.py -----------------------------------------

from tests.list_fixture import ENV, LETTERS, TRAIN_EXE, UTTS, _fixture  # noqa: E402
from tests.test_gpu_ctc_beam import DECODE_EXE  # noqa: E402


@pytest.fixture(scope="module")
def trained_asg(tmp_path_factory):
    d = tmp_path_factory.mktemp("decode_sil")
    _fixture(d)
    cmd = [TRAIN_EXE, "train", f"--archdir={d / 'arch'}", "--arch=net.arch", "--criterion=asg", "--replabel=1", "--transdiag=0.5",
           "--filterbanks=40", f"--tokensdir={d}", "--tokens=tokens.txt", f"--lexicon={d / 'lexicon.txt'}", f"--datadir={d}",
           "--train=train.lst", "--batchsize=3", "--iter=6", "--reportiters=3", "--lr=0.05", "--lrcrit=0.002", "--momentum=0.8",
           "--maxgradnorm=1.0", "--onorm=target", "--sqnorm=true", f"--rundir={d / 'run'}", "--runname=exp"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return d, d / "run" / "exp" / "001_model_last.bin"


def test_s8_decode_tool_silence_score(trained_asg):
    from wav2letter_amd import ASGLoss, checkpoint, criterion, text
    from wav2letter_amd.trainer import Trainer
    d, model = trained_asg
    common = [DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}", "--isbeamdump=true", "--nbest=3",
              "--beamsize=16", "--beamthreshold=100"]

    def dump(extra, ok=True):
        res = subprocess.run(common + extra, capture_output=True, text=True, timeout=600, env=ENV)
        assert (res.returncode == 0) == ok, res.stdout[-2000:] + res.stderr[-2000:]
        return res, (d / "out" / "other.hyp").read_text() if ok else None

    res, plain = dump([f"--w2l_dump_features={d / 'dfeat'}"])
    res, weight = dump(["--w2l_silscore=true", "--silweight=-1"])
    assert "--silscore=-1 on the silence token `|` (class 0)" in res.stderr
    _, named = dump(["--w2l_silscore=true", "--silscore=-1"])
    _, both = dump(["--w2l_silscore=true", "--silscore=-1", "--silweight=-1"])
    assert weight == named == both and weight != plain
    res, _ = dump(["--w2l_silscore=true", "--silscore=-1", "--silweight=-2"], ok=False)
    assert "--silscore" in res.stderr and "--silweight" in res.stderr
    res, off = dump(["--silweight=-1"])
    assert off == plain and "--silweight=-1 has no effect without --w2l_silscore=true" in res.stderr
    res, _ = dump(["--silscore=-1"], ok=False)
    assert "--silscore" in res.stderr and "--w2l_silscore=true" in res.stderr
    res, zero = dump(["--w2l_silscore=true", "--silscore=0"])
    assert zero == plain

    # the Python front end on the same emissions: checkpoint.load, the eval forward on the features Decode dumped
    dic = text.create_token_dict(LETTERS, "asg", 1)
    N = dic.index_size()
    sil = dic.get_index("|")
    assert sil == 0
    arch = (d / "arch" / "net.arch").read_text()
    want = []
    for k in range(3):                                                  # batches of 2, 2, 1 in list order
        utts = UTTS[2 * k:2 * k + 2][:5 - 2 * k]
        raw = (d / f"dfeat.{k + 1}").read_bytes()
        Bk, nfeat, Tk = (int(v) for v in np.frombuffer(raw[:12], np.int32))
        x = torch.tensor(np.frombuffer(raw[12:], np.float32).reshape(Bk, nfeat, Tk).copy()).cuda()
        tr_ = Trainer(arch, nfeat, N, "asg", 4, 0.5)                     # --onorm=target --sqnorm=true --transdiag=0.5
        checkpoint.load(str(model), tr_, arch)
        tr_.plan(Bk, Tk, 8)
        tr_.to_device()
        em = tr_.forward(x, train=False).clone()
        Tout = em.shape[1]
        frames = [min(max(-(-min(1 + (n - 400) // 160, Tk) * Tout // Tk), 1), Tout) for n, _ in utts]
        A = tr_.params[tr_.n_net:tr_.n_net + N * N].view(N, N).clone()
        lab, ln, sc = criterion.asg_beam_search(em, A, torch.tensor(frames, dtype=torch.int32, device="cuda"), beam=16, beam_token=64,
                                                threshold=100.0, nbest=3, sil_token=sil, sil_score=-1.0)
        lab, ln, sc = lab.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()
        for b in range(Bk):
            for m in range(3):
                if ln[b, m] < 0:
                    break
                words = text.tkn_labels_to_wrd([int(c) for c in lab[b, m, :ln[b, m]]], dic, "asg", replabel=1, wordsep="|")
                want.append((f"u{2 * k + b}", f"{float(sc[b, m]):.6f}", " ".join(words)))
    rows = [line.split(" | ") for line in weight.splitlines()]
    assert [(r[0], r[1], r[5].strip() if len(r) > 5 else "") for r in rows] == want
