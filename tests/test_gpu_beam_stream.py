"""GPU tests of the incremental CTC beam search (wav2letter_amd/streaming.py StreamingDecoder, w2l_beam_session_*,
csrc/criterion_beam_stream.hpp).  The oracle is always the whole-utterance entry point of the same variant on the same device, at
B = 1 over the frames fed so far; every comparison is bit for bit (floats through .view(np.int32)).  The inputs' hand-over facts
(full beam, ties, merges, kept repeats at the boundaries) are proved on the CPU in test_beam_stream_host.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import beam_stream_cases as BC
from wav2letter_amd import Lexicon, NGramLM, _lib, criterion
from wav2letter_amd.streaming import StreamingDecoder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, INF = np.float32, float("inf")
VARIANTS = ("plain", "lm", "lex")


@functools.lru_cache(maxsize=None)
def tables(variant, N):
    """the options a variant adds to ctc_beam_search / StreamingDecoder: values in multiples of 1/8, lmWeight a power of two"""
    if variant == "plain":
        return {}
    if variant == "lm":
        tb = BC.token_lm(N)
        cls = torch.tensor((np.random.default_rng(N).integers(-8, 9, N - 1) / 8).astype(F32), device="cuda")
        return dict(lm=NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk)), lm_weight=0.5, class_score=cls, eos_score=-0.25)
    trie, tb = BC.lexicon_and_word_lm(N)
    return dict(lm=NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk)), lm_weight=0.5, eos_score=-0.25, word_score=-0.25,
                lexicon=Lexicon.from_spellings(trie.rows, trie.num_tokens, trie.num_words, trie.word_smear, trie.sil))


def options(variant, shape, log_add, normalize):
    _, _, _, N, W, K, thr, _ = BC.SHAPES[shape]
    return dict(beam=W, beam_token=K, threshold=thr, log_add=bool(log_add), normalize=bool(normalize), **tables(variant, N))


def host(out):
    return tuple(t.cpu().numpy().copy() for t in out)


def same(got, want, what=""):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape)
        assert (g.view(np.int32) == w.view(np.int32)).all(), (what, i)


@functools.lru_cache(maxsize=None)
def whole(variant, shape, log_add, normalize, slot, F, M, Lmax):
    """the oracle: the whole search of slot's first F frames at B = 1, frames = None -> numpy rows [M]...; F = 0: the contract's
    value for a started slot without frames, the empty prefix (with the EOS term) in row 0"""
    opts = options(variant, shape, log_add, normalize)
    extra = dict(max_words=Lmax) if variant == "lex" else {}
    if F == 0:
        n = {"plain": 3, "lm": 4, "lex": 6}[variant]
        lab, ln, sc = np.full((M, Lmax), -1, np.int32), np.full(M, -1, np.int32), np.full(M, -np.inf, F32)
        ln[0], sc[0] = 0, 0.0
        lms, wd, wc = np.full(M, -np.inf, F32), np.full((M, Lmax), -1, np.int32), np.full(M, -1, np.int32)
        lms[0], wc[0] = 0.0, 0
        if variant != "plain":
            lm = opts["lm"]
            q = F32(lm.score(lm.start, lm.eos)[0])
            sc[0] = F32(sc[0] + F32(F32(F32(opts["lm_weight"]) * q) + F32(opts["eos_score"])))
            lms[0] = F32(lms[0] + q)
        return (lab, ln, sc, lms, wd, wc)[:n]
    x = torch.tensor(BC.utterances(shape)[slot][:F][None], device="cuda")
    return tuple(a[0] for a in host(criterion.ctc_beam_search(x, nbest=M, max_len=Lmax, **extra, **opts)))


def run(variant, shape, log_add, normalize, chunkings, M, Lmax, ask=False, nan_fill=False, max_frames=None, max_chunk=None):
    """a session over the three utterances of the shape; returns the final result (numpy, [S][M]...) and, with ask, the result after
    every step together with the frames each slot had then"""
    xs = BC.utterances(shape)
    T, N = xs[0].shape
    max_chunk = max_chunk or T      # "everything at once" is one chunk of T frames
    dec = StreamingDecoder(len(xs), max_chunk, max_frames or T, N, **options(variant, shape, log_add, normalize))
    extra = dict(max_words=Lmax) if variant == "lex" else {}
    asked, fed, started = [], [0] * len(xs), [False] * len(xs)
    for em, n, st in BC.schedule(xs, chunkings, max_chunk, nan_fill):
        dec.step(torch.tensor(em, device="cuda"), n, st)
        for s in range(len(xs)):
            started[s] = started[s] or bool(st[s])
            fed[s] = (0 if st[s] else fed[s]) + int(n[s])
            assert dec.frames(s) == fed[s]
        if ask:
            first, second = host(dec.result(nbest=M, max_len=Lmax, **extra)), host(dec.result(nbest=M, max_len=Lmax, **extra))
            same(first, second, "asking twice")
            asked.append((first, list(fed), list(started)))
    return host(dec.result(nbest=M, max_len=Lmax, **extra)), asked


def check_final(got, variant, shape, log_add, normalize, M, Lmax, what):
    for s, x in enumerate(BC.utterances(shape)):
        want = whole(variant, shape, log_add, normalize, s, x.shape[0], M, Lmax)
        same(tuple(g[s] for g in got), want, (what, "slot", s))
        assert np.isfinite(got[2][s, 0]) or variant == "lex"     # a hypothesis exists (the lexicon may leave none)


# ---- S1: bit for bit under any chunking ------------------------------------------------------------------------------------
S1 = ([(v, "ints_n5_w16_k4", la, nm) for v in VARIANTS for la, nm in ((0, 0), (1, 1), (0, 1), (1, 0))]
      + [(v, "peaked_n30_w16_k8_thr3", la, nm) for v in VARIANTS for la, nm in ((0, 0), (1, 1), (0, 1), (1, 0))]
      + [(v, "peaked_n30_w64_k64", la, nm) for v in VARIANTS for la, nm in ((0, 0), (1, 1))]
      + [(v, "peaked_n30_w1_k1", 0, 0) for v in VARIANTS]
      + [(v, "peaked_n9998_w32_k5", la, la) for v in VARIANTS for la in (0, 1)]
      + [(v, "ints_n12300_rows_from_memory", 0, 0) for v in VARIANTS])


@pytest.mark.parametrize("variant,shape,log_add,normalize", S1)
def test_s1_bitwise_under_any_chunking(variant, shape, log_add, normalize):
    _, _, T, N, W, _, _, _ = BC.SHAPES[shape]
    M, Lmax = W, T
    for name in BC.CHUNKINGS:
        chunkings = [BC.chunking(name, x.shape[0], seed=s) for s, x in enumerate(BC.utterances(shape))]
        got, _ = run(variant, shape, log_add, normalize, chunkings, M, Lmax)
        check_final(got, variant, shape, log_add, normalize, M, Lmax, (variant, shape, name))
    print("S1", variant, shape, "logAdd", log_add, "normalize", normalize, "hypotheses", int((got[1] >= 0).sum()), "longest",
          int(got[1].max()))


# ---- S2: partial results ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("log_add", [0, 1])
def test_s2_partial_results_equal_the_whole_search_on_the_prefix(variant, log_add):
    shape = "peaked_n30_w16_k8_thr3"
    M, Lmax = 16, 40
    xs = BC.utterances(shape)
    chunkings = [BC.fixed(x.shape[0], 3) for x in xs]
    final, asked = run(variant, shape, log_add, log_add, chunkings, M, Lmax, ask=True)
    assert len(asked) >= 14
    for got, fed, started in asked:
        for s in range(len(xs)):
            if not started[s]:      # never started: empty rows
                assert (got[1][s] == -1).all() and (got[2][s] == -np.inf).all() and (got[0][s] == -1).all()
                continue
            same(tuple(g[s] for g in got), whole(variant, shape, log_add, log_add, s, fed[s], M, Lmax), ("partial", s, fed[s]))
    silent, _ = run(variant, shape, log_add, log_add, chunkings, M, Lmax)
    same(final, silent, "a run that never asked")


def test_s2_a_started_slot_without_frames_returns_the_empty_prefix():
    for variant in VARIANTS:
        shape = "peaked_n30_w16_k8_thr3"
        dec = StreamingDecoder(2, 4, 8, 30, **options(variant, shape, 0, 0))
        dec.step(torch.zeros(2, 4, 30, device="cuda"), [0, 0], [1, 0])
        got = host(dec.result(nbest=3, max_len=5, **(dict(max_words=5) if variant == "lex" else {})))
        same(tuple(g[0] for g in got), whole(variant, shape, 0, 0, 0, 0, 3, 5), variant)
        assert (got[1][1] == -1).all() and (got[2][1] == -np.inf).all() and (got[0][1] == -1).all()
        assert got[1][0, 0] == 0 and np.isfinite(got[2][0, 0])


# ---- S3: slots ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_s3_slots_are_independent_restartable_and_read_no_row_beyond_their_count(variant):
    shape, M, Lmax = "peaked_n30_w16_k8_thr3", 16, 40
    x = BC.utterances(shape)[0]
    T, N = x.shape
    opts = options(variant, shape, 0, 0)
    extra = dict(max_words=Lmax) if variant == "lex" else {}
    want = whole(variant, shape, 0, 0, 0, T, M, Lmax)

    # the same utterance in two slots under different chunkings, rows beyond the counts NaN
    dec = StreamingDecoder(2, 9, T, N, **opts)
    plans = [BC.fixed(T, 7), [0, 0] + BC.chunking("random", T, seed=5)]
    pos = [0, 0]
    for i in range(max(len(p) for p in plans)):
        em = np.full((2, 9, N), np.nan, F32)
        n, st = np.zeros(2, np.int32), np.zeros(2, np.int32)
        for s in range(2):
            if i < len(plans[s]):
                c = plans[s][i]
                em[s, :c] = x[pos[s]:pos[s] + c]
                pos[s] += c
                n[s], st[s] = c, i == 0
        dec.step(torch.tensor(em, device="cuda"), n, st)
    got = host(dec.result(nbest=M, max_len=Lmax, **extra))
    for s in range(2):
        same(tuple(g[s] for g in got), want, ("slot", s))
    assert np.isfinite(got[2][got[1] >= 0]).all()

    # slot 0 restarted on another utterance after this one equals a fresh session: the table was cleared
    y = BC.utterances(shape)[1]
    em = np.zeros((2, 9, N), F32)
    for i, c in enumerate(BC.fixed(y.shape[0], 9)):
        em[0, :c] = y[9 * i:9 * i + c]
        dec.step(torch.tensor(em, device="cuda"), [c, 0], [i == 0, 0])
    again = host(dec.result(nbest=M, max_len=Lmax, **extra))
    same(tuple(g[0] for g in again), whole(variant, shape, 0, 0, 1, y.shape[0], M, Lmax), "restarted slot")
    same(tuple(g[1] for g in again), want, "the other slot kept its result")
    dec.reset(1)
    closed = host(dec.result(nbest=M, max_len=Lmax, **extra))
    assert (closed[1][1] == -1).all() and (closed[2][1] == -np.inf).all() and dec.frames(1) == 0
    same(tuple(g[0] for g in closed), tuple(g[0] for g in again), "a reset touches its slot alone")


# ---- S4: the limit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_s4_an_utterance_of_exactly_max_frames(variant):
    """48 frames at W = 64 fill the table's node budget: bit-equal to the whole search; the 49th frame is refused and changes nothing"""
    N, W, T = 30, 64, 48
    x = BC.peaked(np.random.default_rng(48), T, N)
    opts = dict(beam=W, beam_token=64, threshold=INF, log_add=False, normalize=False, **tables(variant, N))
    extra = dict(max_words=T) if variant == "lex" else {}
    want = tuple(a[0] for a in host(criterion.ctc_beam_search(torch.tensor(x[None], device="cuda"), nbest=W, max_len=T, **extra, **opts)))
    dec = StreamingDecoder(1, 5, T, N, **opts)
    em = np.zeros((1, 5, N), F32)
    for i, c in enumerate(BC.fixed(T, 5)):
        em[0, :c] = x[5 * i:5 * i + c]
        dec.step(torch.tensor(em, device="cuda"), [c], [i == 0])
    got = host(dec.result(nbest=W, max_len=T, **extra))
    same(tuple(g[0] for g in got), want)
    assert dec.frames(0) == T
    with pytest.raises(ValueError, match="slot 0.*maxFrames = 48"):
        dec.step(torch.tensor(em, device="cuda"), [1], None)
    assert dec.frames(0) == T
    same(host(dec.result(nbest=W, max_len=T, **extra)), got, "after the refusal")


# ---- S5: surfaces ------------------------------------------------------------------------------------------------------------
def _c_abi(steps, S, Cm, Fmax, N, W, K, thr, log_add, norm, M, Lmax, lm, lmw, eos_score):
    """every step through the C ABI; the outputs after each, lmScores included in every variant"""
    L = _lib.lib()
    blob = lm.device_blob("cuda") if lm is not None else None
    d = _lib.BeamSessionDesc(slots=S, maxChunk=Cm, maxFrames=Fmax, N=N, beam=W, beamToken=K, threshold=thr, logAdd=log_add, normalize=norm,
                             variant=1 if lm is not None else 0, lm=blob.data_ptr() if lm is not None else None,
                             lmHasEos=int(lm.has_eos) if lm is not None else 0, lmWeight=lmw if lm is not None else 0.0,
                             eosScore=eos_score if lm is not None else 0.0)
    h = C.c_void_p(0)
    assert L.w2l_beam_session_create(C.byref(d), C.byref(h)) == 0
    outs = []
    try:
        state = torch.empty(L.w2l_beam_session_state_bytes(C.byref(d)), dtype=torch.uint8, device="cuda")
        assert L.w2l_beam_session_bind(h, state.data_ptr(), state.numel()) == 0
        st_ = torch.cuda.current_stream().cuda_stream
        for em, n, st in steps:
            ed = torch.tensor(em, device="cuda")
            assert L.w2l_beam_session_step(h, ed.data_ptr(), n.ctypes.data, st.ctypes.data, st_) == 0
            lab = torch.full((S, M, Lmax), -7, dtype=torch.int32, device="cuda")
            ln = torch.full((S, M), -7, dtype=torch.int32, device="cuda")
            sc, lms = torch.full((S, M), 7.0, device="cuda"), torch.full((S, M), 7.0, device="cuda")
            assert L.w2l_beam_session_result(h, M, Lmax, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), lms.data_ptr(), 0, None, None, st_) == 0
            assert L.w2l_beam_session_result(h, 0, Lmax, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), lms.data_ptr(), 0, None, None, st_) == 1
            assert L.w2l_beam_session_result(h, W + 1, Lmax, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), lms.data_ptr(), 0, None, None, st_) == 1
            assert L.w2l_beam_session_result(h, M, Lmax, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), None, 0, None, None, st_) == 1
            outs.append(host((lab, ln, sc, lms)))
    finally:
        L.w2l_beam_session_destroy(h)
    return outs


def test_s5_three_surfaces_agree(tmp_path):
    """C ABI == Python StreamingDecoder == compiled C++ fl::pkg::speech::StreamingDecoder (tests/cpp/beam_stream_caller.cpp, plain
    g++ against libw2l_hip.so), LM-free and with a token LM read from one ARPA file; wide=True is refused on both front ends (the
    C++ refusals are checked inside the caller)"""
    from tests.test_ctc_beam_lm_host import _arpa_text
    exe = str(tmp_path / "beam_stream_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "beam_stream_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    shape = "peaked_n30_w16_k8_thr3"
    xs = BC.utterances(shape)
    S, (T, N) = len(xs), xs[0].shape
    W, K, thr, M, Lmax, Cm = 16, 8, 3.0, 4, 12, 7
    steps = BC.schedule(xs, [BC.fixed(x.shape[0], 7) for x in xs], Cm)
    tokens = [f"t{c}" for c in range(N - 1)]
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n")
    (tmp_path / "lm.arpa").write_text(_arpa_text(BC.token_lm(N), tokens, unk10=-3.0)[0])
    arpa_lm = NGramLM.from_arpa(tmp_path / "lm.arpa", tokens)
    for lm, log_add in ((None, 0), (arpa_lm, 0), (arpa_lm, 1)):
        lmw, eos_score = 0.75, -0.25
        want = _c_abi(steps, S, Cm, T, N, W, K, thr, log_add, log_add, M, Lmax, lm, lmw, eos_score)
        if lm is None:      # the LM-free variant's lmScores: 0 for live rows, -inf for empty ones
            for lab, ln, sc, lms in want:
                assert ((lms == 0) == (ln >= 0)).all() and (np.isneginf(lms) == (ln < 0)).all()
        kw = dict(lm=lm, lm_weight=lmw, eos_score=eos_score) if lm is not None else {}
        dec = StreamingDecoder(S, Cm, T, N, beam=W, beam_token=K, threshold=thr, log_add=bool(log_add), **kw)
        n_out = 4 if lm is not None else 3
        for (em, n, st), ref in zip(steps, want):
            dec.step(torch.tensor(em, device="cuda"), n, st)
            same(host(dec.result(nbest=M, max_len=Lmax)), ref[:n_out], "python")
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([S, Cm, T, N, W, K, M, Lmax, log_add, log_add, len(steps)], np.int32).tobytes()
                    + np.array([thr, lmw, eos_score], F32).tobytes())
            for em, n, st in steps:
                f.write(n.tobytes() + st.tobytes() + em.tobytes())
        args = [exe, inp, outp] + ([str(tmp_path / "tokens.txt"), str(tmp_path / "lm.arpa")] if lm is not None else [])
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "beam stream caller ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
        raw = np.fromfile(outp, np.int32)
        at = 0
        for ref in want:
            for a in ref[:n_out]:
                assert (raw[at:at + a.size] == a.view(np.int32).ravel()).all()
                at += a.size
        assert at == len(raw)
    with pytest.raises(_lib.W2LUnsupported, match="wide"):
        StreamingDecoder(S, Cm, T, N, wide=True)


# ---- S6: end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "lm"])
def test_s6_streaming_session_feeds_the_decoder(variant):
    """StreamingSession on the tiny arch feeds a StreamingDecoder step by step (S = 2, chunks of 16 and 8 input frames): the final
    hypotheses equal the whole search over the emissions the session itself produced, bit for bit"""
    import stream_ref as SR
    from tests.test_gpu_stream import fixed, make_trainer
    from wav2letter_amd.streaming import StreamingSession
    S, cmax, T = 2, 16, 64
    tr = make_trainer(SR.TINY_ARCH, SR.NFEAT, SR.NLABEL, 5)
    sess = StreamingSession(tr, S, cmax)
    N = SR.NLABEL
    opts = dict(beam=16, beam_token=8, threshold=INF, log_add=True, normalize=True)
    if variant == "lm":
        tb = BC.LR.random_lm(np.random.default_rng(6), N - 1, 3, 30, True, True, (), eighths=True)
        opts.update(lm=NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk)), lm_weight=0.5, eos_score=-0.25)
    dec = StreamingDecoder(S, sess.max_out, T, N, **opts)
    rng = np.random.default_rng(12)
    xs = [rng.normal(size=(SR.NFEAT, 64)).astype(F32), rng.normal(size=(SR.NFEAT, 40)).astype(F32)]
    plans = [fixed(64, 16), [0] + fixed(40, 8)]
    pos, kept = [0, 0], [[], []]
    for i in range(max(len(p) for p in plans)):
        x = np.zeros((S, SR.NFEAT, cmax), F32)
        n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for s in range(S):
            if i < len(plans[s]):
                c = plans[s][i]
                x[s, :, :c] = xs[s][:, pos[s]:pos[s] + c]
                pos[s] += c
                n[s], st[s], fi[s] = c, i == 0, i == len(plans[s]) - 1
        out, n_out = sess.step(torch.tensor(x, device="cuda"), n, st, fi)
        dec.step(out, n_out, st)                                   # the session's output, as it is
        for s in range(S):
            kept[s].append(out[s, :n_out[s]].clone())
    got = host(dec.result(nbest=8, max_len=T))
    for s in range(S):
        em = torch.cat(kept[s])
        assert em.shape[0] == dec.frames(s) > 4
        want = host(criterion.ctc_beam_search(em[None], nbest=8, max_len=T, **opts))
        same(tuple(g[s] for g in got), tuple(w[0] for w in want), ("end to end", s))
        assert got[1][s, 0] >= 0
