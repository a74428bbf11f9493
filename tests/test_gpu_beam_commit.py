"""GPU tests of w2l_beam_session_commit (csrc/criterion_beam_commit.hpp; StreamingDecoder.commit / WideStreamingDecoder.commit).
The reference is always a second session with the same descriptor, fed the same frames, that never commits (session A, maxFrames
= 64); every comparison is bit for bit (floats through .view(np.int32)).  That the inputs let the commits keep up with a table of
maxFrames = 8 over 40 frames is proved on the CPU in test_beam_commit_host.py."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import beam_commit_ref as CR
from tests import beam_stream_cases as BC
from wav2letter_amd import Lexicon, NGramLM, _lib
from wav2letter_amd.streaming import StreamingDecoder, WideStreamingDecoder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, INF = np.float32, float("inf")
VARIANTS = ("plain", "lm", "lex")
WIDTHS = ((4, 4), (64, 5), (65, 5), (128, 5))      # (W, K): narrow sessions up to 64, wide ones above
T = CR.T


@functools.lru_cache(maxsize=None)
def tables(variant, N):
    """the small LM and lexicon fixtures of the stream tests (test_gpu_beam_stream.tables): values in multiples of 1/8"""
    if variant == "plain":
        return {}
    if variant == "lm":
        tb = BC.token_lm(N)
        cls = torch.tensor((np.random.default_rng(N).integers(-8, 9, N - 1) / 8).astype(F32), device="cuda")
        return dict(lm=NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk)), lm_weight=0.5, class_score=cls, eos_score=-0.25)
    trie, tb = BC.lexicon_and_word_lm(N)
    return dict(lm=NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk)), lm_weight=0.5, eos_score=-0.25, word_score=-0.25,
                lexicon=Lexicon.from_spellings(trie.rows, trie.num_tokens, trie.num_words, trie.word_smear, trie.sil))


def decoder(variant, N, W, K, max_frames, log_add=0, slots=3, max_chunk=CR.MAX_CHUNK, threshold=INF):
    cls = WideStreamingDecoder if W > 64 else StreamingDecoder
    return cls(slots, max_chunk, max_frames, N, beam=W, beam_token=K, threshold=threshold, log_add=bool(log_add),
               normalize=bool(log_add), **tables(variant, N))


def host(out):
    return tuple(t.cpu().numpy().copy() for t in out)


def ask(dec, variant, M, Lmax=T, **kw):
    return host(dec.result(nbest=M, max_len=Lmax, **(dict(max_words=Lmax) if variant == "lex" else {}), **kw))


def same_bytes(got, want, what=""):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape)
        assert (g.view(np.int32) == w.view(np.int32)).all(), (what, i)


def check_exact(ra, rb, dec_b, variant, what):
    """the contract's exactness: committed ++ B's row m == A's row m, counts add up, scores are the same bits, empty rows stay empty"""
    S, M, Lmax = ra[0].shape
    assert (ra[2].view(np.int32) == rb[2].view(np.int32)).all(), (what, "scores")
    if variant != "plain":
        assert (ra[3].view(np.int32) == rb[3].view(np.int32)).all(), (what, "lmScores")
    fields = [(0, 1, 0)] + ([(4, 5, 1)] if variant == "lex" else [])
    for rows, counts, which in fields:
        for s in range(S):
            done = dec_b.committed(s)[which]
            for m in range(M):
                na, nb = int(ra[counts][s, m]), int(rb[counts][s, m])
                if na < 0:
                    assert nb == -1 and (rb[rows][s, m] == -1).all() and (ra[rows][s, m] == -1).all(), (what, s, m, "empty row")
                    continue
                assert na == len(done) + nb, (what, s, m, "count", na, len(done), nb)
                full = np.concatenate([done, rb[rows][s, m, :nb]])
                assert (ra[rows][s, m, :na] == full).all(), (what, s, m, ra[rows][s, m, :na], full)
                assert (rb[rows][s, m, nb:] == -1).all()


def live_rows(r, s):
    return [tuple(r[0][s, m, :r[1][s, m]]) for m in range(r[0].shape[1]) if r[1][s, m] >= 0]


# ---- 1: exactness, stability, maximality -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6, 12])
@pytest.mark.parametrize("W,K", WIDTHS)
@pytest.mark.parametrize("log_add", [0, 1])
@pytest.mark.parametrize("variant", VARIANTS)
def test_1_a_committing_session_returns_what_an_uncommitted_one_returns(variant, log_add, W, K, N):
    """three slots at different phases (one started late, one reset mid-way and started anew, one never started), chunks of 0 to 3
    frames, T = 40; B has maxFrames = 8 and commits after every 2nd step, A has maxFrames = 64 and never commits.  After every
    step and every commit: exactness; the committed labels are a prefix of every row of A (stability); LM-free and token LM: the
    total committed is max(0, LCP - 1) over all live rows of A at nbest = beam (maximality), the lexicon variant: at most that."""
    K = min(K, N - 1)
    a, b = decoder(variant, N, W, K, CR.MAX_FRAMES_A, log_add), decoder(variant, N, W, K, CR.MAX_FRAMES_B, log_add)
    assert b.max_frames * 5 == T
    committed_any = 0
    for i, (em, n, st, reset, commit, fed) in enumerate(CR.schedule(N, variant == "lex")):
        for s in reset:
            a.reset(s)
            b.reset(s)
        x = torch.tensor(em, device="cuda")
        a.step(x, n, st)
        b.step(x, n, st)
        ra = ask(a, variant, W)
        check_exact(ra, ask(b, variant, W), b, variant, ("step", i))
        if not commit:
            continue
        before = [len(b.committed(s)[0]) for s in range(3)]
        out = b.commit()
        for s in range(3):
            labels, words = b.committed(s)
            assert len(labels) == before[s] + len(out[s][0]) and b.frames(s) == a.frames(s)
            rows = live_rows(ra, s)
            for row in rows:                                                     # stability, against A
                assert row[:len(labels)] == tuple(labels), (i, s, row, labels)
            want = CR.commit_len(rows)
            if fed[s][0] is None:
                assert len(labels) == 0 and b.live[s] == 0 and len(out[s][0]) == 0
            elif variant == "lex":      # the hidden unfinished entries hold the cut back; with no finished row at all nothing bounds it
                assert len(labels) <= want or not rows, (i, s)
            else:
                assert len(labels) == want, (i, s, len(labels), want)           # maximality
                assert b.live[s] == CR.live_nodes(rows, want)
            assert CR.budget(int(b.live[s]), W, CR.MAX_FRAMES_B) >= CR.MAX_CHUNK
            committed_any += len(out[s][0])
        check_exact(ra, ask(b, variant, W), b, variant, ("commit", i))
    assert b.frames(0) == T and b.frames(1) == T and b.frames(2) == 0
    assert committed_any > CR.MAX_FRAMES_B
    # the Python surface's whole rows
    rf = ask(b, variant, W, full=True)
    ra = ask(a, variant, W)
    for k in range(len(ra)):
        if ra[k].ndim == 3:
            assert (rf[k][:, :, :T] == ra[k]).all() and (rf[k][:, :, T:] == -1).all()
        else:
            same_bytes((rf[k],), (ra[k],), "full")


# ---- 2: an entry that is the ancestor of another --------------------------------------------------------------------------
def _hand(N, rows):
    """emission rows from {class: value}; everything else -20"""
    x = np.full((len(rows), N), -20.0, F32)
    for t, r in enumerate(rows):
        for c, v in r.items():
            x[t, c] = v
    return x


def _feed(decs, x, start):
    em = np.zeros((1, CR.MAX_CHUNK, x.shape[1]), F32)
    em[0, :len(x)] = x
    for d in decs:
        d.step(torch.tensor(em, device="cuda"), [len(x)], [int(start)])


@pytest.mark.parametrize("W,K", [(4, 4), (65, 5)])
def test_2_the_cut_is_itself_a_beam_entry(W, K):
    """two frames leave "a" and "ab" alive (threshold 5 drops the rest): C is "a", an entry and the other's ancestor; its parent is
    the root, so nothing is committed but the table is rebuilt.  With a frame of "x" in front the same two frames commit "x"."""
    N, blank = 6, 5
    two = _hand(N, [{0: 0.0}, {1: 0.0, blank: -1.0, 0: -2.0}])
    more = _hand(N, [{2: 0.0, blank: -0.5}, {blank: 0.0, 3: -1.0}, {3: 0.0, 2: -1.0}])
    for front, want_done in ((None, []), (_hand(N, [{4: 0.0}]), [4])):
        a, b = (decoder("plain", N, W, K, 16, slots=1, threshold=5.0) for _ in range(2))
        if front is not None:
            _feed((a, b), front, True)
        _feed((a, b), two, front is None)
        ra = ask(a, "plain", W, 8)
        assert live_rows(ra, 0) == [tuple(want_done) + (0, 1), tuple(want_done) + (0,)]
        out = b.commit()
        assert list(out[0][0]) == want_done and list(b.committed(0)[0]) == want_done and b.live[0] == 2
        check_exact(ra, ask(b, "plain", W, 8), b, "plain", "after the commit")
        for t in range(len(more)):
            _feed((a, b), more[t:t + 1], False)
            check_exact(ask(a, "plain", W, 8), ask(b, "plain", W, 8), b, "plain", ("frame", t))
        b.commit()
        rows = live_rows(ask(a, "plain", W, 8), 0)
        assert len(b.committed(0)[0]) == CR.commit_len(rows) >= len(want_done)
        check_exact(ask(a, "plain", W, 8), ask(b, "plain", W, 8), b, "plain", "end")


# ---- 3: nothing to commit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("W,K", [(4, 4), (65, 5)])
def test_3_nothing_to_commit_changes_nothing(variant, W, K):
    """slot 0 right after its start (C is the root), slot 1 with a dead beam (a row of -inf after a live one), slot 2 never started:
    all counts are 0 and the results are the same bytes before and after"""
    N = 6
    dec = decoder(variant, N, W, K, 8, threshold=3.0)
    em = np.zeros((3, CR.MAX_CHUNK, N), F32)
    em[1, 0] = CR.utterances(N)[0][T - 1]
    em[1, 1] = -np.inf
    dec.step(torch.tensor(em, device="cuda"), [0, 2, 0], [1, 1, 0])
    before = ask(dec, variant, W, 8)
    assert before[1][0, 0] == 0 and (before[1][1] == -1).all() and (before[1][2] == -1).all()
    out = dec.commit()
    assert all(len(o[0]) == 0 and len(o[1]) == 0 for o in out) and list(dec.live) == [0, 0, 0]
    same_bytes(ask(dec, variant, W, 8), before, "after the commit")
    out = dec.commit([2])
    assert all(len(o[0]) == 0 for o in out)
    same_bytes(ask(dec, variant, W, 8), before, "after the commit of the slot that never started")
    assert [dec.frames(s) for s in range(3)] == [0, 2, 0]


# ---- 4, 5: twice in a row; a row that is too short ---------------------------------------------------------------------------
def _c_commit(dec, max_len, flags=None):
    """w2l_beam_session_commit through the C ABI with a maxLen of the caller's choice"""
    L, S = _lib.lib(), dec.slots
    scratch = torch.empty(L.w2l_beam_session_commit_bytes(dec.h), dtype=torch.uint8, device="cuda")
    labels = torch.full((S, max_len), -7, dtype=torch.int32, device="cuda")
    nl, nw, live = np.full(S, -7, np.int32), np.full(S, -7, np.int32), np.full(S, -7, np.int32)
    fl = np.asarray(flags, np.int32) if flags is not None else None
    st = L.w2l_beam_session_commit(dec.h, fl.ctypes.data if fl is not None else None, scratch.data_ptr(), scratch.numel(), max_len,
                                   labels.data_ptr(), 0, None, nl.ctypes.data, nw.ctypes.data, live.ctypes.data,
                                   torch.cuda.current_stream().cuda_stream)
    return st, labels.cpu().numpy(), nl, nw, live


def _totals(dec, slot):
    a, b = C.c_int(-1), C.c_int(-1)
    assert _lib.lib().w2l_beam_session_committed(dec.h, slot, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


@pytest.mark.parametrize("variant", ["plain", "lm"])
@pytest.mark.parametrize("W,K", [(4, 4), (65, 5)])
def test_4_5_twice_in_a_row_and_a_row_too_short(variant, W, K):
    N = 12
    xs = CR.utterances(N)
    dec = decoder(variant, N, W, K, 32, slots=2, max_chunk=8)
    for c in range(3):
        em = np.stack([xs[0][8 * c:8 * c + 8], xs[1][8 * c:8 * c + 8]])
        dec.step(torch.tensor(em, device="cuda"), [8, 8], [c == 0, c == 0])
    before = ask(dec, variant, W)
    need = [CR.commit_len(live_rows(before, s)) for s in range(2)]
    assert min(need) >= 2
    # 5: maxLen = 1 holds neither slot's labels: both are refused and wholly unchanged
    st, _, nl, nw, live = _c_commit(dec, 1)
    msg = _lib.lib().w2l_host_last_error().decode()
    assert st == _lib.W2L_EINVAL and "slot 0" in msg and f"{need[0]} labels" in msg and "maxLen = 1" in msg and "unchanged" in msg
    assert list(nl) == need and list(live) == [0, 0] and _totals(dec, 0) == (0, 0) and _totals(dec, 1) == (0, 0)
    same_bytes(ask(dec, variant, W), before, "after the refusal")
    # ... slot 1 alone, with exactly the room it needs: slot 0 is not flagged and stays as it was
    st, lab, nl, nw, live = _c_commit(dec, need[1], [0, 1])
    rows1 = live_rows(before, 1)
    assert st == 0 and list(nl) == [0, need[1]] and list(lab[1]) == list(rows1[0][:need[1]])
    assert list(live) == [0, CR.live_nodes(rows1, need[1])]
    assert _totals(dec, 1) == (need[1], 0) and _totals(dec, 0) == (0, 0)
    mid = ask(dec, variant, W)
    same_bytes(tuple(r[0] for r in mid), tuple(r[0] for r in before), "slot 0 is as it was")
    assert (mid[1][1][mid[1][1] >= 0] == before[1][1][before[1][1] >= 0] - need[1]).all()
    same_bytes((mid[2],), (before[2],), "scores")
    # ... both flagged, room for one label less than slot 0 needs: slot 0 is refused, slot 1 (nothing left to commit) is not
    st, _, nl, nw, live1 = _c_commit(dec, need[0] - 1)
    assert st == _lib.W2L_EINVAL and "slot 0" in _lib.lib().w2l_host_last_error().decode()
    assert list(nl) == [need[0], 0] and list(live1) == list(live) and _totals(dec, 0) == (0, 0)
    same_bytes(ask(dec, variant, W), mid, "after the second refusal")
    # 4: twice in a row
    st, lab, nl, nw, live1 = _c_commit(dec, T)
    assert st == 0 and list(nl) == [need[0], 0] and list(lab[0, :need[0]]) == list(live_rows(before, 0)[0][:need[0]])
    assert (lab[0, need[0]:] == -1).all() and live1[1] == live[1]
    once = ask(dec, variant, W)
    st, lab, nl, nw, live2 = _c_commit(dec, T)
    assert st == 0 and list(nl) == [0, 0] and list(nw) == [0, 0] and list(live2) == list(live1)
    same_bytes(ask(dec, variant, W), once, "a second commit")
    assert _totals(dec, 0) == (need[0], 0) and _totals(dec, 1) == (need[1], 0)


# ---- 6: the budget -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [6, 12])
@pytest.mark.parametrize("variant", ["plain", "lm"])
def test_6_commits_give_the_budget_back(variant, N):
    """W = K = 4, maxFrames = 8, one slot, 40 frames in the schedule's chunks.  Without commits the step past maxFrames is refused with
    today's message; with a commit after every 2nd step the same feed is accepted whole, and the committed total reaches 3/4 of the
    final best row (test_beam_commit_host.py's condition (a))."""
    W = K = 4
    x = CR.utterances(N)[0]
    chunks, F, i = [], 0, 0
    while F < T:
        chunks.append(min(CR.PATTERN[i % len(CR.PATTERN)], T - F))
        F += chunks[-1]
        i += 1
    never, dec = (decoder(variant, N, W, K, CR.MAX_FRAMES_B, slots=1) for _ in range(2))
    pos, refused_at = 0, None
    for i, c in enumerate(chunks):
        try:
            _feed((never,), x[pos:pos + c], i == 0)
        except _lib.W2LInvalidArgument as e:
            refused_at = pos
            assert f"slot 0 would pass maxFrames = 8 ({pos} fed, {c} given)" in str(e)
            break
        pos += c
    assert refused_at is not None and refused_at + 3 > CR.MAX_FRAMES_B >= refused_at and never.frames(0) == refused_at
    pos = 0
    for i, c in enumerate(chunks):
        _feed((dec,), x[pos:pos + c], i == 0)
        pos += c
        if i % 2 == 1:
            dec.commit()
    dec.commit()
    best = ask(dec, variant, 1, full=True)
    assert dec.frames(0) == T and 4 * len(dec.committed(0)[0]) >= 3 * int(best[1][0, 0]) and len(dec.committed(0)[0]) > CR.MAX_FRAMES_B
    assert _totals(dec, 0) == (len(dec.committed(0)[0]), 0)


@pytest.mark.parametrize("W,K", [(4, 4), (65, 5)])
def test_6_a_commit_that_leaves_no_room_makes_the_next_step_refuse(W, K):
    """maxFrames = 2 and two frames that leave "ab", "ac", "db", "dc": six nodes stay; at W = 4 they count as 2 frames, so the slot has
    no room until it commits again or starts anew; at W = 65 the beam keeps the runners-up too and the room follows from `live`"""
    N = 6
    dec = decoder("plain", N, W, K, 2, slots=2)
    x = _hand(N, [{0: 0.0, 3: 0.0}, {1: 0.0, 2: 0.0}])
    em = np.zeros((2, CR.MAX_CHUNK, N), F32)
    em[1, :2] = x
    dec.step(torch.tensor(em, device="cuda"), [0, 2], [0, 1])
    before = ask(dec, "plain", 4, 4)
    assert live_rows(before, 1)[:4] == [(0, 1), (0, 2), (3, 1), (3, 2)]
    rows = live_rows(ask(dec, "plain", W, 4), 1)
    out = dec.commit()
    live = CR.live_nodes(rows, 0)
    assert len(out[1][0]) == 0 and dec.live[1] == live and (live == 6 or W > 4)
    room = CR.budget(live, W, 2)
    assert room == 0 if W == 4 else room in (0, 1)
    one = torch.tensor(em[:, 1:2].repeat(CR.MAX_CHUNK, axis=1), device="cuda")
    dec.step(one, [0, 0], None)                                  # no frames: always fine
    for _ in range(room):
        dec.step(one, [0, 1], None)
    with pytest.raises(_lib.W2LInvalidArgument, match=f"slot 1 would pass its budget of maxFrames = 2.*{live} nodes"):
        dec.step(one, [0, 1], None)
    assert dec.frames(1) == 2 + room
    if room == 0:
        same_bytes(ask(dec, "plain", 4, 4), before, "after the refusal")
    dec.step(one, [0, 1], [0, 1])                                # a start gives the whole budget back
    assert dec.frames(1) == 1 and len(dec.committed(1)[0]) == 0


# ---- 7: surfaces -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,K", [(4, 4), (65, 5)])
def test_7_the_cpp_caller_prints_what_python_returns(tmp_path, W, K):
    """fl::pkg::speech::StreamingDecoder / WideStreamingDecoder ::commit and ::committed (tests/cpp/beam_commit_caller.cpp, plain g++
    against libw2l_hip.so) against the Python front end, token LM read from one ARPA file; Python's result(full=True) against A"""
    from tests.test_ctc_beam_lm_host import _arpa_text
    N = 12
    exe = str(tmp_path / "beam_commit_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "beam_commit_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    tokens = [f"t{c}" for c in range(N - 1)]
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n")
    (tmp_path / "lm.arpa").write_text(_arpa_text(BC.token_lm(N), tokens, unk10=-3.0)[0])
    lm = NGramLM.from_arpa(tmp_path / "lm.arpa", tokens)
    steps = [(em, n, st, commit) for em, n, st, _, commit, _ in CR.schedule(N)]      # the caller has no reset: slot 1 stays open
    lmw, eos = 0.75, -0.25
    kw = dict(beam=W, beam_token=K, lm=lm, lm_weight=lmw, eos_score=eos)
    cls = WideStreamingDecoder if W > 64 else StreamingDecoder
    a, b = cls(3, CR.MAX_CHUNK, CR.MAX_FRAMES_A, N, **kw), cls(3, CR.MAX_CHUNK, CR.MAX_FRAMES_B, N, **kw)
    lines, live = [], ["-"] * 3
    for i, (em, n, st, commit) in enumerate(steps):
        x = torch.tensor(em, device="cuda")
        a.step(x, n, st)
        b.step(x, n, st)
        live = ["-" if st[s] else live[s] for s in range(3)]
        if commit:
            b.commit()
            live = [str(int(v)) for v in b.live]
        rb, ra, rf = ask(b, "lm", 1), ask(a, "lm", 1), ask(b, "lm", 1, full=True)
        for k in range(4):
            if ra[k].ndim == 3:
                assert (rf[k][:, :, :T] == ra[k]).all() and (rf[k][:, :, T:] == -1).all()
            else:
                same_bytes((rf[k],), (ra[k],), ("full", i))
        for s in range(3):
            done, tail = b.committed(s)[0], rb[0][s, 0, :max(rb[1][s, 0], 0)]
            lines.append(f"{i} {s} {live[s]} :" + "".join(f" {v}" for v in done) + " |" + "".join(f" {v}" for v in tail))
    inp = str(tmp_path / "in.bin")
    with open(inp, "wb") as f:
        f.write(np.array([3, CR.MAX_CHUNK, CR.MAX_FRAMES_B, N, W, K, T, 0, 0, len(steps), CR.COMMIT_EVERY], np.int32).tobytes()
                + np.array([INF, lmw, eos], F32).tobytes())
        for em, n, st, _ in steps:
            f.write(n.tobytes() + st.tobytes() + em.tobytes())
    r = subprocess.run([exe, inp, str(tmp_path / "tokens.txt"), str(tmp_path / "lm.arpa")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "beam commit caller ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr)
    got = r.stdout.splitlines()
    assert got[-1] == "beam commit caller ok" and got[:-1] == lines
    assert any(ln.split(":")[1].split("|")[0].strip() for ln in lines)               # something was committed
