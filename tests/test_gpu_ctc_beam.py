"""w2l_ctc_beam_search on the GPU against the numpy restatement of its contract (tests/ctc_beam_ref.py).
T1 the exact recurrences at the enumeration shapes; T2 selection, merge and tie rules BITWISE (logAdd = 0 on emissions whose sums
are exact in fp32); T3 the log-sum search with the beam binding, on inputs whose every decision has a margin; T4 the log-sum
search at full width, qualified on the CPU; T5 identity with w2l_ctc_viterbi; then the surfaces and the Decode tool."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import ctc_beam_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _lib():
    from wav2letter_amd import _lib
    return _lib


def _search(x, frames, W, K, threshold, log_add, normalize, M, Lmax):
    """the C ABI on numpy inputs -> labels [B][M][Lmax], lengths [B][M], scores [B][M]"""
    L = _lib()
    lib = L.lib()
    B, T, N = x.shape
    st = torch.cuda.current_stream().cuda_stream
    xd = torch.tensor(x, device="cuda")
    fd = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
    ws = torch.empty(max(lib.w2l_ctc_beam_workspace_size(B, T, N, W, K), 256), dtype=torch.uint8, device="cuda")
    labels = torch.full((B, M, Lmax), -7, dtype=torch.int32, device="cuda")
    lengths = torch.full((B, M), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((B, M), 7.0, device="cuda")
    L.check(lib.w2l_ctc_beam_search(B, T, N, xd.data_ptr(), fd.data_ptr() if fd is not None else None, W, K, threshold,
                                    int(log_add), int(normalize), M, Lmax, labels.data_ptr(), lengths.data_ptr(),
                                    scores.data_ptr(), ws.data_ptr(), st), "ctc_beam_search")
    torch.cuda.synchronize()
    return labels.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy()


def _close(got, want):
    """the project's fp32 parity bar (BASELINE north_star): 1e-4 relative to max(1, |score|)"""
    return np.abs(got.astype(np.float64) - want) <= 1e-4 * np.maximum(1.0, np.abs(want))


# ---- T1: the exact recurrences -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,T", [(3, 5), (4, 3)])
def test_t1_exact_recurrences_at_the_enumeration_shapes(N, T):
    """W = 64, K = N-1, no threshold: the beam never binds, every labelling's score is the sum over its paths.  The ranks compared
    are the leading ones whose gaps are >= 10 delta: at these seeds all of them (asserted), so every rank is compared by position"""
    B, M = 3, 25
    x = np.stack([np.random.default_rng(seed).normal(0, 2, size=(T, N)) for seed in range(B)]).astype(np.float32)
    lab, ln, sc, diags = R.beam_search(x, None, 64, N - 1, INF, True, True, M, T, np.float64)
    glab, gln, gsc = _search(x, None, 64, N - 1, INF, True, True, M, T)
    print("T1", N, T, "max |score diff|", np.abs(gsc - sc).max())
    assert (gln >= 0).all() and _close(gsc, sc).all()                 # all 25 labellings are there, whatever their order
    for b in range(B):
        dl = R.delta(T, diags[b].S)
        lead = 0
        while lead < M - 1 and diags[b].final_gaps[lead] >= 10 * dl:
            lead += 1
        print("T1 seed", b, "delta", dl, "leading ranks with a margin", lead)
        assert lead == M - 1
        assert (gln[b, :lead] == ln[b, :lead]).all() and (glab[b, :lead] == lab[b, :lead]).all()
        want = {tuple(lab[b, m, :ln[b, m]]) for m in range(M)}
        assert {tuple(glab[b, m, :gln[b, m]]) for m in range(M)} == want and len(want) == M


# ---- T2: selection, merge and tie rules, bit for bit -----------------------------------------------------------------------

def _ints(rng, B, T, N):
    return (rng.integers(-24, 1, size=(B, T, N)) / 8).astype(np.float32)


def _few_owners(rng, B, T, N):
    """distinct multiples of 1/8 whose largest 1280 values sit at classes c with c % 1024 < 128: in the row kernel 32 threads own
    all of them, the per-thread maxima bound nothing and the candidates overflow the LDS list (the extraction rounds run)"""
    x = np.empty((B, T, N), np.float32)
    c = np.arange(N)
    top = np.nonzero(c % 1024 < 128)[0]
    rest = np.nonzero(c % 1024 >= 128)[0]
    for b in range(B):
        for t in range(T):
            x[b, t, rng.permutation(top)] = -np.arange(len(top)) / 8
            x[b, t, rng.permutation(rest)] = -(len(top) + np.arange(len(rest))) / 8
    return x


def _integer_steps(rng, B, T, N):
    """every row a permutation of 0, -1, ..., -(N-1): with threshold 1.0 a candidate sits exactly ON the line (kept) or one step
    below it (dropped)"""
    return np.stack([[-rng.permutation(N).astype(np.float32) for _ in range(T)] for _ in range(B)])


T2_CASES = {  # name: (make, B, T, N, frames, W, K, threshold, M, Lmax)
    "full_width_frames": (_ints, 4, 40, 9998, [40, 1, 17, 33], 64, 64, INF, 64, 40),
    "w32_k5_threshold_m1": (_ints, 2, 40, 9998, None, 32, 5, 2.5, 1, 40),
    "w1_k1": (_ints, 2, 24, 9998, None, 1, 1, INF, 1, 24),
    "n30_k_clipped_short_lmax": (_ints, 3, 40, 30, [40, 9, 26], 16, 64, 3.0, 16, 3),
    "n30_threshold_binds": (_integer_steps, 2, 12, 30, None, 64, 64, 1.0, 64, 12),
    "n2": (_ints, 2, 12, 2, [12, 5], 8, 1, INF, 8, 12),
    "n2_k_clipped": (_ints, 1, 9, 2, None, 64, 64, 1.0, 3, 9),
    "rows_extraction_rounds": (_few_owners, 1, 5, 9998, None, 8, 64, INF, 8, 5),
    "rows_from_memory": (_ints, 2, 5, 12300, [5, 3], 8, 64, INF, 8, 5),
    "rows_from_memory_few_owners": (_few_owners, 1, 3, 12300, None, 4, 7, 4.0, 4, 3),
}


@functools.lru_cache(maxsize=None)
def _t2_reference(name):
    make, B, T, N, frames, W, K, thr, M, Lmax = T2_CASES[name]
    x = make(np.random.default_rng(len(name) * 1000 + T), B, T, N)
    return x, R.beam_search(x, frames, W, K, thr, False, False, M, Lmax, np.float32)


@pytest.mark.parametrize("name", list(T2_CASES))
def test_t2_bitwise_against_the_float32_restatement(name):
    _, B, T, N, frames, W, K, thr, M, Lmax = T2_CASES[name]
    x, (lab, ln, sc, _) = _t2_reference(name)
    glab, gln, gsc = _search(x, frames, W, K, thr, False, False, M, Lmax)
    assert sc.dtype == np.float32
    print("T2", name, "hypotheses", int((ln >= 0).sum()), "longest", int(ln.max()), "ties in the output",
          int(sum(len(s[s > -np.inf]) - len(np.unique(s[s > -np.inf])) for s in sc)))
    assert (gln == ln).all()
    assert (glab == lab).all()
    assert (gsc.view(np.int32) == sc.view(np.int32)).all()
    if name == "n30_k_clipped_short_lmax":
        assert ln.max() > Lmax                                       # a hypothesis longer than the label rows
    if name == "n30_threshold_binds":
        assert (ln == -1).any() and (ln[:, 0] >= 0).all()            # the threshold left fewer than M entries


# ---- T3: the log-sum search with the beam binding ---------------------------------------------------------------------------

T3_CASES = [  # (T, N, W, K, scale, seeds): seeds whose every decision gap is >= 10 delta (asserted, never skipped)
    (12, 32, 4, 3, 2.0, (1, 4)),
    (16, 9998, 4, 3, 3.0, (1, 2)),
    (12, 6, 3, 2, 2.0, (0, 1)),
]


@pytest.mark.parametrize("T,N,W,K,scale,seeds", T3_CASES)
def test_t3_log_sum_search_small_beams(T, N, W, K, scale, seeds):
    x = np.stack([np.random.default_rng(s).normal(0, scale, size=(T, N)) for s in seeds]).astype(np.float32)
    lab, ln, sc, diags = R.beam_search(x, None, W, K, INF, True, True, W, T, np.float64)
    for dg in diags:
        dl = R.delta(T, dg.S)
        print("T3", (T, N, W, K), "S", dg.S, "delta", dl, "decision gap", dg.decision_gap(), "final gap", min(dg.final_gaps))
        assert dg.decision_gap() >= 10 * dl and min(dg.final_gaps) >= 10 * dl
    glab, gln, gsc = _search(x, None, W, K, INF, True, True, W, T)
    print("T3 max |score diff|", np.abs(gsc - sc).max())
    assert (gln == ln).all() and (glab == lab).all()
    assert _close(gsc, sc).all()


# ---- T4: the log-sum search at full width -----------------------------------------------------------------------------------

def test_t4_log_sum_search_full_width():
    from wav2letter_amd import criterion
    T, N, W, K, M = 33, 9998, 64, 64, 2
    seeds = (0, 1, 3)
    x = np.stack([np.random.default_rng(s).normal(0, 3, size=(T, N)) for s in seeds]).astype(np.float32)
    lab, ln, sc, diags = R.beam_search(x, None, W, K, INF, True, True, M, T, np.float64)
    for b, dg in enumerate(diags):                                   # tail decisions are dense here: qualified on the CPU
        dl = R.delta(T, dg.S)
        for w in (W - 1, W + 1):
            hyps, _ = R.beam_search_one(x[b], T, w, K, INF, True, True, np.float64, M)
            assert [p for p, _ in hyps] == [tuple(lab[b, m, :ln[b, m]]) for m in range(M)]
            assert [s for _, s in hyps] == [sc[b, m] for m in range(M)]
        print("T4 seed", seeds[b], "delta", dl, "final gaps", dg.final_gaps, "ancestor margins", dg.margins)
        assert min(dg.final_gaps) >= 10 * dl and min(dg.margins) >= 10 * dl
    glab, gln, gsc = _search(x, None, W, K, INF, True, True, M, T)
    print("T4 max |score diff|", np.abs(gsc - sc).max())
    assert (gln == ln).all() and (glab == lab).all() and _close(gsc, sc).all()
    # a beam's mass is a lower bound of the labelling's probability: score <= -loss of the hypothesis as a target
    B = len(seeds)
    tgt = np.full((B * M, int(gln.max())), -1, np.int32)
    for b in range(B):
        for m in range(M):
            tgt[b * M + m, :gln[b, m]] = glab[b, m, :gln[b, m]]
    xd = torch.tensor(np.repeat(x, M, axis=0), device="cuda")
    loss, _ = criterion.ctc_score(xd, torch.tensor(tgt, device="cuda"))
    loss = loss.cpu().numpy().reshape(B, M)
    print("T4 score", gsc.tolist(), "-loss", (-loss).tolist())
    assert (gsc <= -loss + 1e-4 * np.abs(loss)).all()
    for b in range(B):                                               # distinct and sorted
        assert len({tuple(glab[b, m, :gln[b, m]]) for m in range(M)}) == M and (np.diff(gsc[b]) <= 0).all()


# ---- T5: identity with what exists ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 8])
@pytest.mark.parametrize("B,T,N", [(3, 50, 30), (2, 40, 9998)])
def test_t5_max_search_rank0_is_the_collapsed_greedy_path(W, B, T, N):
    from wav2letter_amd import CTCLoss
    x = np.random.default_rng(N + T).normal(0, 2, size=(B, T, N)).astype(np.float32)
    top2 = np.sort(x, axis=2)[:, :, -2:]
    assert (top2[:, :, 1] - top2[:, :, 0]).min() >= 1e-3
    frames = np.array([T, T // 3, 1, T - 1][:B], np.int32)
    path = CTCLoss().viterbiPath(torch.tensor(x, device="cuda")).cpu().numpy()
    glab, gln, _ = _search(x, frames, W, 3, INF, False, True, 1, T)
    for b in range(B):
        want, prev = [], None
        for p in path[b, :frames[b]]:
            if p != prev and p != N - 1:
                want.append(int(p))
            prev = p
        assert gln[b, 0] == len(want) and list(glab[b, 0, :len(want)]) == want and (glab[b, 0, len(want):] == -1).all()


# ---- surfaces ---------------------------------------------------------------------------------------------------------------

def test_python_front_end_equals_the_c_abi():
    from wav2letter_amd import CTCLoss, criterion
    B, T, N = 3, 30, 40
    x = np.random.default_rng(5).normal(0, 2, size=(B, T, N)).astype(np.float32)
    frames = np.array([30, 11, 1], np.int32)
    xd, fd = torch.tensor(x, device="cuda"), torch.tensor(frames, device="cuda")
    for log_add, norm, thr, M in ((True, True, INF, 4), (False, False, 6.0, 1)):
        lab, ln, sc = _search(x, frames, 8, 5, thr, log_add, norm, M, T)
        for got in (criterion.ctc_beam_search(xd, fd, beam=8, beam_token=5, threshold=thr, log_add=log_add, nbest=M),
                    CTCLoss().beamSearch(xd, fd, beam=8, beam_token=5, threshold=thr, log_add=log_add, normalize=norm, nbest=M)):
            assert got[0].dtype == torch.int32 and (got[0].cpu().numpy() == lab).all() and (got[1].cpu().numpy() == ln).all()
            assert (got[2].cpu().numpy().view(np.int32) == sc.view(np.int32)).all()
    lab, ln, _ = _search(x, None, 8, 5, INF, False, False, 2, 4)      # no frames, short label rows
    got = criterion.ctc_beam_search(xd, beam=8, beam_token=5, nbest=2, max_len=4)
    assert (got[0].cpu().numpy() == lab).all() and (got[1].cpu().numpy() == ln).all()
    with pytest.raises(ValueError):
        criterion.ctc_beam_search(xd, fd[:2])
    with pytest.raises(_lib().W2LError):
        criterion.ctc_beam_search(xd, beam=65)


def test_three_surfaces_agree(tmp_path):
    """C ABI == Python CTCLoss.beamSearch == compiled C++ fl::pkg::speech::CTCLoss::beamSearch (tests/cpp/decode_caller.cpp, plain
    g++ against libw2l_hip.so with the flags of tests/cpp/Makefile)"""
    from wav2letter_amd import CTCLoss
    exe = str(tmp_path / "decode_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "decode_caller.cpp"),
                    "-o", exe, "-L" + libdir, "-lw2l_hip", "-Wl,-rpath," + libdir, "-ldl"], check=True)
    rng = np.random.default_rng(8)
    for B, T, N, W, K, M, Lmax, log_add, norm, thr in [(4, 31, 30, 8, 5, 3, 31, 1, 1, INF), (2, 20, 9998, 16, 64, 16, 6, 0, 0, 2.0)]:
        x = rng.normal(0, 2, size=(B, T, N)).astype(np.float32) if log_add else _ints(rng, B, T, N)
        frames = rng.integers(1, T + 1, B).astype(np.int32)
        frames[1] = 1
        want_f = _search(x, frames, W, K, thr, log_add, norm, M, Lmax)
        want = _search(x, None, W, K, thr, log_add, norm, M, Lmax)
        xd = torch.tensor(x, device="cuda")
        opts = dict(beam=W, beam_token=K, threshold=thr, log_add=bool(log_add), normalize=bool(norm), nbest=M, max_len=Lmax)
        for got, ref in ((CTCLoss().beamSearch(xd, torch.tensor(frames, device="cuda"), **opts), want_f),
                         (CTCLoss().beamSearch(xd, **opts), want)):
            assert all((g.cpu().numpy().view(np.int32) == r.view(np.int32)).all() for g, r in zip(got, ref))
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([N, T, B, W, K, M, Lmax, log_add, norm], np.int32).tobytes() + np.array([thr], np.float32).tobytes()
                    + x.tobytes() + frames.tobytes())
        run = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "decode caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
        got = np.fromfile(outp, np.int32)
        sizes = [B * M * Lmax, B * M, B * M]
        at = 0
        for ref in (want_f, want):
            for r, n in zip(ref, sizes):
                assert (got[at:at + n] == r.view(np.int32).ravel()).all()
                at += n
        assert at == len(got)


# ---- the Decode tool end to end, on the six-WAV fixture of tests/list_fixture.py ------------------------------------------

from tests.list_fixture import ENV, LETTERS, UTTS, _fixture, _train_cmd  # noqa: E402

DECODE_EXE = os.path.join(ROOT, "wav2letter_amd", "bin", "Decode")


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    d = tmp_path_factory.mktemp("decode")
    _fixture(d)
    out = subprocess.run(_train_cmd(d, d / "run"), capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return d, d / "run" / "exp" / "001_model_last.bin"


def _sclite_lines(path):
    """`words (sampleId)` per line -> [(words, id)]"""
    out = []
    for line in path.read_text().splitlines():
        assert line.endswith(")") and " (" in line, line
        words, sid = line[:-1].rsplit(" (", 1)
        out.append((words.split(), sid))
    return out


def test_decode_tool_end_to_end(trained):
    """Decode over a five-sample list in batches of 2 (a short last batch): .hyp / .ref / .log formats, and with --logadd=false the
    hypotheses are the greedy transcripts of the same model (checkpoint.load, the eval forward on the features Decode dumped,
    CTCLoss.viterbiPath over the utterance's frames, tkn_prediction_to_ltr)"""
    from wav2letter_amd import CTCLoss, checkpoint, text
    from wav2letter_amd.trainer import Trainer
    d, model = trained
    res = subprocess.run([DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}", "--show=true",
                          "--showletters=true", f"--w2l_dump_features={d / 'dfeat'}"], capture_output=True, text=True, timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    hyp, ref = _sclite_lines(d / "out" / "other.hyp"), _sclite_lines(d / "out" / "other.ref")
    assert [s for _, s in hyp] == [s for _, s in ref] == [f"u{k}" for k in range(5)]
    assert [w for w, _ in ref] == [tr.split() for _, tr in UTTS[:5]]
    log = (d / "out" / "other.log").read_text()
    assert log in res.stdout and log.count("|T|: ") == log.count("|P|: ") == log.count("|t|: ") == log.count("|p|: ") == 5
    assert log.count("[sample: u") == 5 and "slice WER: " in log
    last = log.splitlines()[-1]
    assert log.splitlines()[-2] == "------" and last.startswith("[Decode sub/other.lst (5 samples) in ") and "-- WER: " in last and "%, TER: " in last

    dic = text.create_token_dict(LETTERS, "ctc")
    arch = (d / "arch" / "net.arch").read_text()
    N = dic.index_size()
    greedy = []
    for k in range(3):                                                  # batches of 2, 2, 1 in list order
        utts = UTTS[2 * k:2 * k + 2][:5 - 2 * k]
        raw = (d / f"dfeat.{k + 1}").read_bytes()
        B, nfeat, T = (int(v) for v in np.frombuffer(raw[:12], np.int32))
        assert B == len(utts)
        x = torch.tensor(np.frombuffer(raw[12:], np.float32).reshape(B, nfeat, T).copy()).cuda()
        tr_ = Trainer(arch, nfeat, N, "ctc", 4, 0.0)                    # --onorm=target --sqnorm=true
        checkpoint.load(str(model), tr_, arch)
        tr_.plan(B, T, 8)
        tr_.to_device()
        em = tr_.forward(x, train=False).clone()
        Tout = em.shape[1]
        frames = [min(max(-(-min(1 + (n - 400) // 160, T) * Tout // T), 1), Tout) for n, _ in utts]
        path = CTCLoss().viterbiPath(em).cpu().numpy()
        for b in range(B):
            greedy.append(text.tkn2wrd(text.tkn_prediction_to_ltr(path[b, :frames[b]], dic, "ctc", wordsep="|"), "|"))
    assert [w for w, _ in hyp] == greedy
    wer = text.EditDistanceMeter()
    for g, (_, tr) in zip(greedy, UTTS):
        wer.add(g, tr.split())
    assert abs(float(last.split("-- WER: ")[1].split("%")[0]) - wer.value()) < 1e-3

    # the beam dump: three well-formed lines per sample, scores non-increasing; the labelling-probability search
    for extra in ([], ["--logadd=true"]):
        res = subprocess.run([DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}",
                              "--isbeamdump=true", "--nbest=3", "--beamsize=16", "--beamthreshold=100"] + extra,
                             capture_output=True, text=True, timeout=600, env=ENV)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        rows = [line.split(" | ") for line in (d / "out" / "other.hyp").read_text().splitlines()]
        assert len(rows) == 15 and all(len(r) == 6 for r in rows)
        for k in range(5):
            mine = rows[3 * k:3 * k + 3]
            assert [r[0] for r in mine] == [f"u{k}"] * 3
            scores = [float(r[1]) for r in mine]
            assert scores == sorted(scores, reverse=True) and all(np.isfinite(scores))
            assert all(r[1] == r[2] and float(r[3]) == 0.0 and float(r[4]) >= 0.0 for r in mine)
            if not extra:
                assert mine[0][5].split() == greedy[k]


@pytest.mark.parametrize("flag,name", [("--lm=lm.bin", "--lm"), ("--uselexicon=true", "--uselexicon"), ("--decodertype=wrd", "--decodertype"),
                                       ("--silscore=0.5", "--silscore"), ("--wordscore=-1", "--wordscore"), ("--criterion=asg", "--criterion")])
def test_decode_tool_refuses_what_it_does_not_decode(trained, flag, name):
    d, model = trained
    res = subprocess.run([DECODE_EXE, f"--am={model}", "--test=sub/other.lst", flag], capture_output=True, text=True, timeout=120, env=ENV)
    assert res.returncode != 0 and name in res.stderr, (res.returncode, res.stderr)
