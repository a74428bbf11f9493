"""GPU tests of the wide incremental CTC beam search (wav2letter_amd/streaming.py WideStreamingDecoder,
w2l_beam_session_create_wide, csrc/criterion_beam_stream.hpp over csrc/criterion_beam_wide.hpp).  The oracle is always the
whole-utterance WIDE entry point of the same variant on the same device -- criterion.ctc_beam_search(..., wide=True) at B = 1 over
the frames fed so far; every comparison is bit for bit (floats through .view(np.int32)).  That the inputs hand over more than 64
entries, with ties, merges and kept repeats at the boundaries, is proved on the CPU in test_beam_stream_wide_host.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import beam_stream_cases as BC
from tests import beam_stream_wide_cases as WC
from tests import test_gpu_beam_stream as GS
from tests.test_gpu_beam_stream import host, same, tables
from wav2letter_amd import Lexicon, NGramLM, _lib, criterion
from wav2letter_amd.streaming import StreamingDecoder, WideStreamingDecoder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, INF = np.float32, float("inf")
VARIANTS = ("plain", "lm", "lex")


def options(variant, shape, log_add, normalize):
    _, _, _, N, W, K, thr, _ = WC.SHAPES[shape]
    return dict(beam=W, beam_token=K, threshold=thr, log_add=bool(log_add), normalize=bool(normalize), **tables(variant, N))


def extra(variant, Lmax):
    return dict(max_words=Lmax) if variant == "lex" else {}


def whole_search(x, variant, opts, M, Lmax):
    """the oracle on frames x [F][N]: the wide whole search at B = 1, frames = None -> numpy rows [M]..."""
    xd = torch.tensor(np.ascontiguousarray(x)[None], device="cuda")
    return tuple(a[0] for a in host(criterion.ctc_beam_search(xd, nbest=M, max_len=Lmax, wide=True, **extra(variant, Lmax), **opts)))


@functools.lru_cache(maxsize=None)
def whole(variant, shape, log_add, normalize, slot, F, M, Lmax):
    """computed once per (case, slot, F) and shared; F = 0: the contract's value for a started slot without frames (the narrow
    tests' statement of it: it depends on the LM's tables and scores alone, and those are the same per N)"""
    if F == 0:
        assert WC.SHAPES[shape][3] == 30
        return GS.whole(variant, "peaked_n30_w16_k8_thr3", log_add, normalize, 0, 0, M, Lmax)
    return whole_search(WC.utterances(shape)[slot][:F], variant, options(variant, shape, log_add, normalize), M, Lmax)


def empty_rows(got, s):
    return (got[1][s] == -1).all() and np.isneginf(got[2][s]).all() and (got[0][s] == -1).all() and all(
        (g[s] == -1).all() if g.dtype == np.int32 else np.isneginf(g[s]).all() for g in got[3:])


def run(cls, xs, variant, opts, chunkings, M, Lmax, ask=False, nan_fill=False, max_frames=None, max_chunk=None):
    """a session of class cls over the utterances xs, slot s starting at BC.FIRST_STEP[s]; returns the final result (numpy,
    [S][M]...) and, with ask, the result after every step together with the frames each slot had then"""
    T, N = xs[0].shape
    max_chunk = max_chunk or T
    dec = cls(len(xs), max_chunk, max_frames or T, N, **opts)
    ex = extra(variant, Lmax)
    asked, fed, started = [], [0] * len(xs), [False] * len(xs)
    for em, n, st in BC.schedule(xs, chunkings, max_chunk, nan_fill):
        dec.step(torch.tensor(em, device="cuda"), n, st)
        for s in range(len(xs)):
            started[s] = started[s] or bool(st[s])
            fed[s] = (0 if st[s] else fed[s]) + int(n[s])
            assert dec.frames(s) == fed[s]
        if ask:
            first, second = host(dec.result(nbest=M, max_len=Lmax, **ex)), host(dec.result(nbest=M, max_len=Lmax, **ex))
            same(first, second, "asking twice")
            asked.append((first, list(fed), list(started)))
    return host(dec.result(nbest=M, max_len=Lmax, **ex)), asked


# ---- V1: bit for bit under any chunking --------------------------------------------------------------------------------------
V1 = ([(v, s, la, nm) for s in WC.SHAPES for v in VARIANTS for la, nm in ((0, 0), (1, 1))]
      + [(v, "ints_n5_w100_k4", la, nm) for v in VARIANTS for la, nm in ((0, 1), (1, 0))])


@pytest.mark.parametrize("variant,shape,log_add,normalize", V1)
def test_v1_bitwise_under_any_chunking(variant, shape, log_add, normalize):
    _, _, T, N, W, _, _, _ = WC.SHAPES[shape]
    M, Lmax = W, T
    xs = WC.utterances(shape)
    opts = options(variant, shape, log_add, normalize)
    for name in BC.CHUNKINGS:
        chunkings = [BC.chunking(name, x.shape[0], seed=s) for s, x in enumerate(xs)]
        if name == "random":
            assert any(0 in c[:-1] for c in chunkings)                      # an empty chunk in mid-utterance
        got, _ = run(WideStreamingDecoder, xs, variant, opts, chunkings, M, Lmax)
        for s, x in enumerate(xs):
            same(tuple(g[s] for g in got), whole(variant, shape, log_add, normalize, s, x.shape[0], M, Lmax), (variant, shape, name, s))
            assert np.isfinite(got[2][s, 0]) or variant == "lex"             # a hypothesis exists (the lexicon may leave none)
    print("V1", variant, shape, "logAdd", log_add, "normalize", normalize, "hypotheses of slot 0", int((got[1][0] >= 0).sum()),
          "longest", int(got[1].max()))
    if variant != "lex":
        assert (got[1][0] >= 0).sum() > 64                                    # more rows than a narrow session has entries


# ---- V2: partial results -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_v2_partial_results_equal_the_whole_wide_search_on_the_prefix(variant):
    shape, log_add = "peaked_n30_w256_k16_thr4", 1
    M, Lmax = 256, 24
    xs = WC.utterances(shape)
    opts = options(variant, shape, log_add, log_add)
    chunkings = [BC.fixed(x.shape[0], 3) for x in xs]
    final, asked = run(WideStreamingDecoder, xs, variant, opts, chunkings, M, Lmax, ask=True)
    assert len(asked) >= 8
    seen_closed = seen_open = 0
    for got, fed, started in asked:
        for s in range(len(xs)):
            if not started[s]:      # never started: empty rows
                assert empty_rows(got, s)
                seen_closed += 1
                continue
            same(tuple(g[s] for g in got), whole(variant, shape, log_add, log_add, s, fed[s], M, Lmax), ("partial", s, fed[s]))
            seen_open += 1
    assert seen_closed and seen_open
    silent, _ = run(WideStreamingDecoder, xs, variant, opts, chunkings, M, Lmax)
    same(final, silent, "a run that never asked")


def test_v2_a_started_slot_without_frames_returns_the_empty_prefix():
    for variant in VARIANTS:
        shape = "peaked_n30_w256_k16_thr4"
        dec = WideStreamingDecoder(2, 4, 8, 30, **options(variant, shape, 0, 0))
        dec.step(torch.zeros(2, 4, 30, device="cuda"), [0, 0], [1, 0])
        got = host(dec.result(nbest=3, max_len=5, **extra(variant, 5)))
        same(tuple(g[0] for g in got), whole(variant, shape, 0, 0, 0, 0, 3, 5), variant)
        assert empty_rows(got, 1)
        assert got[1][0, 0] == 0 and np.isfinite(got[2][0, 0])


# ---- V3: slots ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_v3_slots_are_independent_restartable_and_read_no_row_beyond_their_count(variant):
    shape = "peaked_n30_w256_k16_thr4"
    M, Lmax = 256, 24
    xs = WC.utterances(shape)
    x = xs[0]
    T, N = x.shape
    opts = options(variant, shape, 0, 0)
    ex = extra(variant, Lmax)
    want = whole(variant, shape, 0, 0, 0, T, M, Lmax)

    # the same utterance in two slots under different chunkings, rows beyond the counts NaN
    dec = WideStreamingDecoder(2, 9, T, N, **opts)
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
    got = host(dec.result(nbest=M, max_len=Lmax, **ex))
    for s in range(2):
        same(tuple(g[s] for g in got), want, ("slot", s))
    assert np.isfinite(got[2][got[1] >= 0]).all()
    if variant != "lex":
        assert (got[1][0] >= 0).sum() == 256                                  # the beam the restart below leaves behind is full

    # slot 0, whose stored beam has 256 entries, restarted on a 1-frame utterance: nothing beyond the new n is read
    y = xs[2]
    assert y.shape[0] == 1
    em = np.full((2, 9, N), np.nan, F32)
    em[0, :1] = y
    dec.step(torch.tensor(em, device="cuda"), [1, 0], [1, 0])
    again = host(dec.result(nbest=M, max_len=Lmax, **ex))
    same(tuple(g[0] for g in again), whole(variant, shape, 0, 0, 2, 1, M, Lmax), "restarted slot")
    same(tuple(g[1] for g in again), want, "the other slot kept its result")
    if variant != "lex":
        assert 0 < (again[1][0] >= 0).sum() < 64
    dec.reset(1)
    closed = host(dec.result(nbest=M, max_len=Lmax, **ex))
    assert empty_rows(closed, 1) and dec.frames(1) == 0
    same(tuple(g[0] for g in closed), tuple(g[0] for g in again), "a reset touches its slot alone")


# ---- V4: the limit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_v4_an_utterance_of_exactly_max_frames(variant):
    """24 frames at W = 100 with max_frames = 24: bit-equal to the whole search; the 25th frame is refused and changes nothing"""
    shape = "ints_n5_w100_k4"
    x = WC.utterances(shape)[0]
    T, N = x.shape
    W = 100
    opts = options(variant, shape, 0, 0)
    ex = extra(variant, T)
    dec = WideStreamingDecoder(1, 5, T, N, **opts)
    em = np.zeros((1, 5, N), F32)
    for i, c in enumerate(BC.fixed(T, 5)):
        em[0, :c] = x[5 * i:5 * i + c]
        dec.step(torch.tensor(em, device="cuda"), [c], [i == 0])
    got = host(dec.result(nbest=W, max_len=T, **ex))
    same(tuple(g[0] for g in got), whole(variant, shape, 0, 0, 0, T, W, T))
    assert dec.frames(0) == T
    with pytest.raises(ValueError, match="slot 0.*maxFrames = 24"):
        dec.step(torch.tensor(em, device="cuda"), [1], None)
    assert dec.frames(0) == T
    same(host(dec.result(nbest=W, max_len=T, **ex)), got, "after the refusal")
    with pytest.raises(ValueError):
        dec.result(nbest=W + 1, max_len=T, **ex)
    with pytest.raises(ValueError):
        dec.result(nbest=0, max_len=T, **ex)


# ---- V5: a beam that dies ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_add", [0, 1])
def test_v5_a_beam_that_dies_stays_dead(log_add):
    """test_w4_lexicon_without_an_entry_at_the_root's lexicon (every word has two tokens) and blank (far below the threshold line):
    after one frame every entry ends inside a word and all rows are empty although the beam lives.  Frame 4 is -inf in every class:
    no candidate is left, n = 0, and the later frames leave the beam dead.  Slot 0 runs in chunks of 3, slot 1 the same utterance
    in chunks of 1; after every step both equal the whole wide search on their frames."""
    from tests import ctc_beam_lex_ref as XR
    from tests import ctc_beam_lm_ref as LR
    rng = np.random.default_rng(3)
    N, tokens, T, W = 12, 11, 9, 100
    x = (rng.integers(-12, 1, size=(T, N)) / 4).astype(F32)
    x[:, N - 1] = -40.0
    x[4, :] = -np.inf
    rows = [(w, [w % tokens, (w + 1) % tokens]) for w in range(tokens)]
    tb = LR.random_lm(rng, tokens, 2, 30, True, True, (), eighths=True)
    trie = XR.TextbookTrie(rows, tokens, tokens, BC.smear(tb, tokens), None)
    opts = dict(beam=W, beam_token=64, threshold=8.0, log_add=bool(log_add), normalize=False,
                lm=NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk)), lm_weight=0.5, eos_score=0.0, word_score=0.25,
                lexicon=Lexicon.from_spellings(trie.rows, trie.num_tokens, trie.num_words, trie.word_smear, trie.sil))
    M, Lmax = W, T
    dec = WideStreamingDecoder(2, 3, T, N, **opts)
    plans = [BC.fixed(T, 3), BC.fixed(T, 1)]
    pos, alive_then_dead = [0, 0], [[], []]
    for i in range(T):
        em = np.zeros((2, 3, N), F32)
        n = np.zeros(2, np.int32)
        for s in range(2):
            if i < len(plans[s]):
                c = plans[s][i]
                em[s, :c] = x[pos[s]:pos[s] + c]
                pos[s] += c
                n[s] = c
        dec.step(torch.tensor(em, device="cuda"), n, [i == 0, i == 0])
        got = host(dec.result(nbest=M, max_len=Lmax, max_words=Lmax))
        for s in range(2):
            want = whole_search(x[:pos[s]], "lex", opts, M, Lmax)
            same(tuple(g[s] for g in got), want, ("slot", s, "frames", pos[s]))
            alive_then_dead[s].append((pos[s], not empty_rows(got, s)))
    by_frames = dict(alive_then_dead[1])
    assert not by_frames[1]                                   # no entry at the root after one frame
    assert by_frames[2] or by_frames[3] or by_frames[4]       # words were completed before the beam died
    assert not any(by_frames[f] for f in range(5, T + 1))     # dead from frame 4 on
    assert dict(alive_then_dead[0])[3] and not dict(alive_then_dead[0])[6] and not dict(alive_then_dead[0])[9]


# ---- V6: the two families agree where both exist -------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", ["peaked_n30_w16_k8_thr3", "peaked_n30_w64_k64"])
def test_v6_wide_and_narrow_sessions_return_the_same_bytes(variant, shape):
    _, _, T, N, W, _, _, _ = BC.SHAPES[shape]
    xs = BC.utterances(shape)
    chunkings = [BC.fixed(x.shape[0], 3) for x in xs]
    for log_add in (0, 1):
        opts = GS.options(variant, shape, log_add, log_add)
        narrow, asked_n = run(StreamingDecoder, xs, variant, opts, chunkings, W, T, ask=True)
        wide, asked_w = run(WideStreamingDecoder, xs, variant, opts, chunkings, W, T, ask=True)
        same(wide, narrow, (variant, shape, log_add))
        assert len(asked_n) == len(asked_w)
        for (gn, _, _), (gw, _, _) in zip(asked_n, asked_w):
            same(gw, gn, "partial")
        assert np.isfinite(wide[2][0, 0]) or variant == "lex"


# ---- V7: surfaces ------------------------------------------------------------------------------------------------------------
def _c_abi(steps, S, Cm, Fmax, N, W, K, thr, log_add, norm, M, Lmax, lm, lmw, eos_score):
    """every step through the C ABI (w2l_beam_session_create_wide, then the shared entry points); the outputs after each, lmScores
    included in every variant"""
    L = _lib.lib()
    blob = lm.device_blob("cuda") if lm is not None else None
    d = _lib.BeamSessionDesc(slots=S, maxChunk=Cm, maxFrames=Fmax, N=N, beam=W, beamToken=K, threshold=thr, logAdd=log_add, normalize=norm,
                             variant=1 if lm is not None else 0, lm=blob.data_ptr() if lm is not None else None,
                             lmHasEos=int(lm.has_eos) if lm is not None else 0, lmWeight=lmw if lm is not None else 0.0,
                             eosScore=eos_score if lm is not None else 0.0)
    h = C.c_void_p(0)
    assert L.w2l_beam_session_create_wide(C.byref(d), C.byref(h)) == 0
    outs = []
    try:
        need = L.w2l_beam_session_wide_state_bytes(C.byref(d))
        state = torch.empty(need, dtype=torch.uint8, device="cuda")
        assert L.w2l_beam_session_bind(h, state.data_ptr(), need - 1) == 1
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


def test_v7_three_surfaces_agree(tmp_path):
    """C ABI == Python WideStreamingDecoder == compiled C++ fl::pkg::speech::WideStreamingDecoder (tests/cpp/
    beam_stream_wide_caller.cpp, plain g++ against libw2l_hip.so) at W = 100, LM-free and with a token LM read from one ARPA file;
    the C++ refusals (beamSize 1025: std::runtime_error) are checked inside the caller"""
    from tests.test_ctc_beam_lm_host import _arpa_text
    exe = str(tmp_path / "beam_stream_wide_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "beam_stream_wide_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    shape = "peaked_n30_w256_k16_thr4"
    xs = WC.utterances(shape)
    S, (T, N) = len(xs), xs[0].shape
    W, K, thr, M, Lmax, Cm = 100, 8, 4.0, 70, 12, 7
    steps = BC.schedule(xs, [BC.fixed(x.shape[0], 7) for x in xs], Cm)
    tokens = [f"t{c}" for c in range(N - 1)]
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n")
    (tmp_path / "lm.arpa").write_text(_arpa_text(BC.token_lm(N), tokens, unk10=-3.0)[0])
    arpa_lm = NGramLM.from_arpa(tmp_path / "lm.arpa", tokens)
    for lm, log_add in ((None, 0), (arpa_lm, 0), (arpa_lm, 1)):
        lmw, eos_score = 0.75, -0.25
        want = _c_abi(steps, S, Cm, T, N, W, K, thr, log_add, log_add, M, Lmax, lm, lmw, eos_score)
        assert (want[-1][1][0] >= 0).sum() > 64                       # rows beyond a narrow session's beam
        if lm is None:      # the LM-free variant's lmScores: 0 for live rows, -inf for empty ones
            for lab, ln, sc, lms in want:
                assert ((lms == 0) == (ln >= 0)).all() and (np.isneginf(lms) == (ln < 0)).all()
        kw = dict(lm=lm, lm_weight=lmw, eos_score=eos_score) if lm is not None else {}
        opts = dict(beam=W, beam_token=K, threshold=thr, log_add=bool(log_add), **kw)
        n_out = 4 if lm is not None else 3
        # the last step's rows are the whole wide search's
        for s, x in enumerate(xs):
            same(tuple(a[s] for a in want[-1][:n_out]), whole_search(x, "lm" if lm is not None else "plain", opts, M, Lmax), ("oracle", s))
        dec = WideStreamingDecoder(S, Cm, T, N, **opts)
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
        assert r.returncode == 0 and "beam stream wide caller ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
        raw = np.fromfile(outp, np.int32)
        at = 0
        for ref in want:
            for a in ref[:n_out]:
                assert (raw[at:at + a.size] == a.view(np.int32).ravel()).all()
                at += a.size
        assert at == len(raw)
    with pytest.raises(_lib.W2LUnsupported, match="wide"):
        StreamingDecoder(S, Cm, T, N, wide=True)
    with pytest.raises(_lib.W2LUnsupported):
        WideStreamingDecoder(S, Cm, T, N, beam=1025)


# ---- V8: end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "lm"])
def test_v8_streaming_session_feeds_the_wide_decoder(variant):
    """StreamingSession on the tiny arch feeds a WideStreamingDecoder at W = 100 step by step (S = 2, chunks of 16 and 8 input
    frames, max_chunk = max_out): the final hypotheses equal the whole wide search over the emissions the session itself produced"""
    import stream_ref as SR
    from tests.test_gpu_stream import fixed, make_trainer
    from wav2letter_amd.streaming import StreamingSession
    S, cmax, T = 2, 16, 64
    tr = make_trainer(SR.TINY_ARCH, SR.NFEAT, SR.NLABEL, 5)
    sess = StreamingSession(tr, S, cmax)
    N = SR.NLABEL
    opts = dict(beam=100, beam_token=8, threshold=INF, log_add=True, normalize=True)
    if variant == "lm":
        tb = BC.LR.random_lm(np.random.default_rng(6), N - 1, 3, 30, True, True, (), eighths=True)
        opts.update(lm=NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk)), lm_weight=0.5, eos_score=-0.25)
    dec = WideStreamingDecoder(S, sess.max_out, T, N, **opts)
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
    got = host(dec.result(nbest=100, max_len=T))
    for s in range(S):
        em = torch.cat(kept[s])
        assert em.shape[0] == dec.frames(s) > 4
        want = host(criterion.ctc_beam_search(em[None], nbest=100, max_len=T, wide=True, **opts))
        same(tuple(g[s] for g in got), tuple(w[0] for w in want), ("end to end", s))
        assert got[1][s, 0] >= 0
    assert (got[1][0] >= 0).sum() > 64
