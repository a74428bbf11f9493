"""w2l_ctc_align on the GPU: the path BITWISE equal to the numpy restatement of the contract (tests/ctc_align_ref.py: fp32 compares
and single fp32 adds on the raw emissions, stay beats advance beats skip on ties), the score against a float64 log-softmax summed
over the reference path, the relation to w2l_ctc_forward / w2l_ctc_viterbi, and the three surfaces (C ABI, Python, compiled C++)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import ctc_align_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from wav2letter_amd import _lib
    return _lib


def _align(x, tgt, frames=None, with_score=True):
    """the C ABI on numpy inputs -> (path [B][T], score [B] or None, targetSize [B])"""
    L = _lib()
    lib = L.lib()
    B, T, N = x.shape
    Lt = tgt.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    xd, yd = torch.tensor(x, device="cuda"), torch.tensor(tgt, device="cuda")
    ts = torch.empty(B, dtype=torch.int32, device="cuda")
    L.check(lib.w2l_batch_ctc_target_size(B, Lt, T, yd.data_ptr(), ts.data_ptr(), st), "target size")
    fd = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
    ws = torch.empty(max(lib.w2l_ctc_align_workspace_size(B, T, N, Lt), 256), dtype=torch.uint8, device="cuda")
    path = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B,), 7.0, device="cuda") if with_score else None
    L.check(lib.w2l_ctc_align(B, T, N, Lt, xd.data_ptr(), yd.data_ptr(), ts.data_ptr(), fd.data_ptr() if fd is not None else None,
                              path.data_ptr(), score.data_ptr() if with_score else None, ws.data_ptr(), st), "ctc_align")
    torch.cuda.synchronize()
    return path.cpu().numpy(), score.cpu().numpy() if with_score else None, ts.cpu().numpy()


def _emissions(rng, kind, B, T, N):
    if kind == "int":        # small integers: every sum exact in fp32, exact ties everywhere
        return rng.integers(-2, 3, size=(B, T, N)).astype(np.float32)
    x = rng.normal(size=(B, T, N)).astype(np.float32)
    if kind == "x50":        # confident (and confidently wrong) frames
        x *= np.float32(50)
    return x


def _targets(rng, B, L, N, runs):
    """[B][L] -1 padded; row 0 uses all L positions; `runs`: stretches of one repeated label"""
    tgt = np.full((B, L), -1, np.int32)
    for b in range(B):
        n = L if b == 0 else int(rng.integers(0, L + 1))
        lab = rng.integers(0, N - 1, n)
        if runs and n:
            lab = np.repeat(rng.integers(0, N - 1, n), rng.integers(1, 4, n))[:n]
        elif n > 3:
            lab[1] = lab[0]
        tgt[b, :n] = lab
    return tgt


def _check_case(x, tgt, frames):
    """path bitwise, score within the fp32 bar, score == NULL gives the same path.  Returns (path, score, reference score)"""
    B, T, N = x.shape
    ref_path, ref_score = R.ctc_align_ref(x, tgt, frames)
    path, score, ts = _align(x, tgt, frames)
    assert (ts == R.ctc_target_size(tgt, T)).all()
    bad = np.argwhere(path != ref_path)
    assert len(bad) == 0, (x.shape, tgt.shape, bad[:8], path[bad[0][0]][:40], ref_path[bad[0][0]][:40])
    path2, _, _ = _align(x, tgt, frames, with_score=False)
    assert (path2 == ref_path).all()
    feas = ref_path[:, 0] >= 0
    assert (score[~feas] == -np.inf).all() and np.isfinite(score[feas]).all()
    d = np.abs(score[feas].astype(np.float64) - ref_score[feas])
    print("ctc_align", x.shape, tgt.shape[1], "feasible", int(feas.sum()), "of", B, "max |score - ref| / max(1, |ref|) =",
          float((d / np.maximum(1, np.abs(ref_score[feas]))).max()) if feas.any() else 0.0)
    assert (d <= 1e-4 * np.maximum(1, np.abs(ref_score[feas]))).all(), (d, ref_score[feas])
    return path, score, ref_score


# every ctc_positions_per_lane class: 2 L + 1 <= 128, 192, 256, 320, 384, 512, 1024, 2048
LANE_CLASSES = [1, 63, 64, 95, 128, 160, 192, 255, 256, 512, 1023]


@pytest.mark.parametrize("L", LANE_CLASSES)
@pytest.mark.parametrize("kind", ["normal", "int"])
def test_path_bitwise_every_positions_per_lane_class(L, kind):
    rng = np.random.default_rng(100 + L)
    B, N = 3, 30
    T = 1500 if L >= 512 else 2 * L + 37
    x = _emissions(rng, kind, B, T, N)
    tgt = _targets(rng, B, L, N, runs=(L % 2 == 1))
    frames = rng.integers(1, T + 1, B).astype(np.int32)
    frames[0] = T
    _check_case(x, tgt, frames)
    _check_case(x, tgt, None)


SHAPES = [  # (B, T, N, L): register-resident rows and the big-row regime (N = 13000), T from 1, the recipe's criterion shapes
    (1, 1, 5, 1), (3, 1, 30, 2), (3, 2, 5, 2), (1, 2, 9998, 1), (3, 37, 5, 9), (32, 37, 30, 20), (3, 37, 9998, 12), (3, 37, 13000, 12),
    (1, 188, 5, 64), (3, 188, 30, 95), (32, 188, 9998, 80), (3, 188, 13000, 64), (1, 1500, 5, 255), (32, 1500, 30, 256),
    (3, 1500, 9998, 80), (1, 1500, 13000, 160),
]


@pytest.mark.parametrize("B,T,N,L", SHAPES)
def test_path_bitwise_shapes(B, T, N, L):
    rng = np.random.default_rng(B * 7 + T * 3 + N + L)
    for kind, runs, use_frames in (("normal", False, False), ("x50", True, True), ("int", True, True), ("int", False, False)):
        x = _emissions(rng, kind, B, T, N)
        tgt = _targets(rng, B, L, N, runs)
        frames = rng.integers(1, T + 1, B).astype(np.int32) if use_frames else None
        _check_case(x, tgt, frames)
        if N > 5000:
            break             # (the wide rows: one flavour with all frames, the flavours below on the narrow shapes)
    if N > 5000:
        x = _emissions(rng, "x50", B, T, N)
        _check_case(x, _targets(rng, B, L, N, True), rng.integers(1, T + 1, B).astype(np.int32))


@pytest.mark.parametrize("kind", ["normal", "int"])
def test_exactly_one_feasible_path_and_infeasible_rows_mixed_in(kind):
    """frames = L_b + R exactly: one lattice path; one frame fewer: no path (-1 row, -inf score) beside feasible rows"""
    rng = np.random.default_rng(5)
    B, T, N, L = 8, 90, 30, 40
    x = _emissions(rng, kind, B, T, N)
    tgt = _targets(rng, B, L, N, runs=True)
    tgt[3, 0] = -1                                            # an empty target: all blank
    tgt[3, 1:] = -1
    ts = R.ctc_target_size(tgt, T)
    need = np.array([ts[b] + int((tgt[b, 1:ts[b]] == tgt[b, :max(ts[b] - 1, 0)]).sum()) for b in range(B)])
    frames = np.maximum(need, 1).astype(np.int32)
    path, score, _ = _check_case(x, tgt, frames)
    assert (path[:, 0] >= 0).all()
    for b in range(B):
        assert R.collapse(path[b, :frames[b]], N - 1) == [int(v) for v in tgt[b, :ts[b]]]
    assert (path[3] == N - 1).all()
    short = frames.copy()
    short[::2] = np.maximum(short[::2] - 1, 1)                 # rows 0, 2, 4, 6: one frame too few
    path, score, _ = _check_case(x, tgt, short)
    for b in range(0, B, 2):
        if need[b] > short[b]:
            assert (path[b] == -1).all() and score[b] == -np.inf
    assert (path[1::2, 0] >= 0).all()


def test_score_is_below_the_ctc_likelihood_and_greedy_path_is_recovered():
    """a path is no likelier than the sum over paths: score <= -loss of w2l_ctc_forward (scale mode NONE) on every feasible row.
    Both are fp32 results held to the project's 1e-4 * max(1, |value|) bar against the exact numbers, so the comparison is made
    with that slack (a target with ONE feasible path has score = -loss exactly, up to rounding).  With continuous random emissions
    (no ties) and the greedy path's collapse as the target, the aligned path IS the greedy path."""
    L = _lib()
    lib = L.lib()
    rng = np.random.default_rng(11)
    st = torch.cuda.current_stream().cuda_stream
    for B, T, N, Lt in [(8, 60, 30, 64), (32, 188, 9998, 80), (3, 40, 13000, 12)]:
        x = _emissions(rng, "normal", B, T, N)
        tgt = _targets(rng, B, Lt, N, runs=False)
        path, score, ts = _align(x, tgt)
        xd, yd, tsd = torch.tensor(x, device="cuda"), torch.tensor(tgt, device="cuda"), torch.tensor(ts, device="cuda")
        ws = torch.empty(lib.w2l_ctc_workspace_size(B, T, N, Lt), dtype=torch.uint8, device="cuda")
        loss = torch.empty(B, device="cuda")
        L.check(lib.w2l_ctc_forward(B, T, N, Lt, 0, xd.data_ptr(), yd.data_ptr(), tsd.data_ptr(), loss.data_ptr(), ws.data_ptr(), st), "fwd")
        nll = loss.cpu().numpy().astype(np.float64)
        print("score", score[:4], "-loss", -nll[:4])
        assert (path[:, 0] >= 0).all()
        assert (score <= -nll + 1e-4 * np.maximum(1, np.abs(nll))).all(), (score, -nll)
        # greedy path -> its collapse as the target -> the alignment is the greedy path
        greedy = torch.empty(B, T, dtype=torch.int32, device="cuda")
        L.check(lib.w2l_ctc_viterbi(B, T, N, xd.data_ptr(), greedy.data_ptr(), st), "viterbi")
        greedy = greedy.cpu().numpy()
        rows = [R.collapse(g, N - 1) for g in greedy]
        gt = np.full((B, max(len(r) for r in rows) + 1), -1, np.int32)
        for b, r in enumerate(rows):
            gt[b, :len(r)] = r
        apath, ascore, _ = _align(x, gt)
        assert (apath == greedy).all()
        assert (ascore < 0).all()                                            # a log-probability


def test_python_front_end_equals_the_c_abi():
    from wav2letter_amd import CTCLoss, criterion
    rng = np.random.default_rng(3)
    B, T, N, Lt = 4, 50, 30, 12
    x = _emissions(rng, "normal", B, T, N)
    tgt = _targets(rng, B, Lt, N, runs=True)
    frames = np.array([50, 31, 44, 2], np.int32)
    path, score, _ = _align(x, tgt, frames)
    xd, yd, fd = torch.tensor(x, device="cuda"), torch.tensor(tgt, device="cuda"), torch.tensor(frames, device="cuda")
    p, s = criterion.ctc_align(xd, yd, fd)
    assert p.dtype == torch.int32 and (p.cpu().numpy() == path).all()
    assert (s.cpu().numpy().view(np.int32) == score.view(np.int32)).all()
    p2, s2 = criterion.ctc_align(xd, yd, fd, with_score=False)
    assert s2 is None and (p2.cpu().numpy() == path).all()
    assert (CTCLoss().viterbiPathWithTarget(xd, yd, fd).cpu().numpy() == path).all()
    full, _, _ = _align(x, tgt)
    assert (CTCLoss().viterbiPathWithTarget(xd, yd).cpu().numpy() == full).all()
    with pytest.raises(ValueError):
        criterion.ctc_align(xd, yd, fd[:2])


def test_three_surfaces_agree(tmp_path):
    """C ABI == Python CTCLoss.viterbiPathWithTarget == compiled C++ fl::pkg::speech::CTCLoss::viterbiPathWithTarget
    (tests/cpp/align_caller.cpp, plain g++ against libw2l_hip.so with the flags of tests/cpp/Makefile)"""
    from wav2letter_amd import CTCLoss
    exe = str(tmp_path / "align_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "align_caller.cpp"),
                    "-o", exe, "-L" + libdir, "-lw2l_hip", "-Wl,-rpath," + libdir, "-ldl"], check=True)
    rng = np.random.default_rng(8)
    for B, T, N, Lt, kind in [(5, 61, 30, 17, "normal"), (3, 40, 9998, 12, "int")]:
        x = _emissions(rng, kind, B, T, N)
        tgt = _targets(rng, B, Lt, N, runs=True)
        frames = rng.integers(1, T + 1, B).astype(np.int32)
        frames[1] = 1                                          # too short for its target unless that is empty or one label
        want_f, _, _ = _align(x, tgt, frames, with_score=False)
        want, _, _ = _align(x, tgt, None, with_score=False)
        xd, yd = torch.tensor(x, device="cuda"), torch.tensor(tgt, device="cuda")
        crit = CTCLoss()
        assert (crit.viterbiPathWithTarget(xd, yd, torch.tensor(frames, device="cuda")).cpu().numpy() == want_f).all()
        assert (crit.viterbiPathWithTarget(xd, yd).cpu().numpy() == want).all()
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([N, T, B, Lt], np.int32).tobytes() + x.tobytes() + tgt.tobytes() + frames.tobytes())
        run = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "align caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
        got = np.fromfile(outp, np.int32).reshape(3, B, T)
        assert (got[0] == want_f).all() and (got[1] == want_f).all() and (got[2] == want).all()


# ---- the Align tool end to end, on the six-WAV fixture recipe of tests/test_gpu_train_valid.py (its helper, copied) ----------

TRAIN_EXE = os.path.join(ROOT, "wav2letter_amd", "bin", "Train")
ALIGN_EXE = os.path.join(ROOT, "wav2letter_amd", "bin", "Align")
ENV = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
UTTS = [(9600, "hello bee"), (6400, "aaa"), (8000, "zoo hello"), (4800, "bee"), (7300, "add zoo"), (5100, "hello")]
LETTERS = ["|", "'"] + [chr(c) for c in range(ord("a"), ord("z") + 1)]


def _wav(path, x):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.asarray(x, "<i2").tobytes())


def _fixture(d):
    """letter tokens + lexicon, six WAV utterances; train.lst and sub/other.lst (5 of them: a short last batch)"""
    from wav2letter_amd import recipes
    os.makedirs(d / "arch")
    os.makedirs(d / "audio")
    os.makedirs(d / "sub")
    (d / "arch" / "net.arch").write_text(recipes.conv_glu_small_arch(widths=(32, 48), kws=(5, 5), drop=0.2))
    (d / "tokens.txt").write_text("\n".join(LETTERS) + "\n")
    (d / "lexicon.txt").write_text("".join(f"{w}\t{' '.join(w)} |\n" for w in ["hello", "aaa", "bee", "zoo", "add"]))
    rng = np.random.default_rng(0)
    lines = []
    for k, (n, tr) in enumerate(UTTS):
        t = np.arange(n) / 16000.0
        sig = np.round((0.3 * np.sin(2 * np.pi * (200 + 150 * k) * t) + 0.05 * rng.normal(size=n)) * 30000).astype(np.int16)
        _wav(d / "audio" / f"u{k}.wav", sig)
        lines.append(f"u{k} audio/u{k}.wav {n / 16.0:.1f} {tr}")
    (d / "train.lst").write_text("\n".join(lines) + "\n")
    (d / "sub" / "other.lst").write_text("\n".join(lines[:5]) + "\n")


def _train_cmd(d, run, crit):
    return [TRAIN_EXE, "train", f"--archdir={d / 'arch'}", "--arch=net.arch", f"--criterion={crit}", "--filterbanks=40",
            f"--tokensdir={d}", "--tokens=tokens.txt", f"--lexicon={d / 'lexicon.txt'}", f"--datadir={d}", "--train=train.lst",
            "--batchsize=3", "--iter=6", "--reportiters=3", "--lr=0.05", "--lrcrit=0.002", "--momentum=0.8", "--maxgradnorm=1.0",
            "--onorm=target", "--sqnorm=true", f"--rundir={run}", "--runname=exp"] + (["--replabel=2"] if crit == "asg" else [])


def _parse_line(line):
    """the consumers' view (the reference's filter_segmentations.py:31-39): fields 3-5 of every segment"""
    assert line.endswith("\n") and "\n" not in line[:-1]
    sample, segs = line[:-1].split("\t")
    out = []
    for seg in segs.split("\\n"):
        f = seg.split(" ")
        assert len(f) == 5
        out.append((float(f[2]), float(f[3]), f[4]))
    return sample, out


@pytest.mark.parametrize("crit", ["ctc", "asg"])
def test_align_tool_end_to_end(tmp_path, crit):
    """train a few updates, run Align over a five-sample list in batches of 2 (a short last batch), and reproduce every line from
    the Python front end: checkpoint.load, the eval forward on the features Align dumped, ctc_align (CTC) or
    ForceAlignmentCriterion.viterbiPath per utterance prefix (ASG), and the span functions of text.py"""
    from wav2letter_amd import ForceAlignmentCriterion, checkpoint, criterion, text
    from wav2letter_amd.trainer import Trainer
    d = tmp_path
    _fixture(d)
    out = subprocess.run(_train_cmd(d, d / "run", crit), capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    model = d / "run" / "exp" / "001_model_last.bin"
    res = subprocess.run([ALIGN_EXE, str(d / "align.txt"), f"--am={model}", "--test=sub/other.lst", "--batchsize=2",
                          f"--w2l_dump_features={d / 'afeat'}"], capture_output=True, text=True, timeout=600, env=ENV)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = (d / "align.txt").read_text().splitlines(keepends=True)
    assert len(lines) == 5, res.stderr

    replabel = 2 if crit == "asg" else 0
    dic = text.create_token_dict(LETTERS, crit, replabel=replabel)
    lex = text.load_lexicon((d / "lexicon.txt").read_text().splitlines())
    arch = (d / "arch" / "net.arch").read_text()
    header, arrays = checkpoint.read(str(model))
    trans = [a for t, a in zip(header["tensors"], arrays) if t["kind"] == "criterion"]
    N = dic.index_size()
    want = []
    for k in range(3):                                                  # batches of 2, 2, 1 in list order
        utts = UTTS[2 * k:2 * k + 2][:5 - 2 * k]
        raw = (d / f"afeat.{k + 1}").read_bytes()
        B, nfeat, T = (int(v) for v in np.frombuffer(raw[:12], np.int32))
        assert B == len(utts)
        x = torch.tensor(np.frombuffer(raw[12:], np.float32).reshape(B, nfeat, T).copy()).cuda()
        rows = [text.target_indices(tr.split(), lex, dic, crit, replabel=replabel, wordsep="|") for _, tr in utts]
        tgt = torch.tensor(text.pad_targets(rows)).cuda()
        tr_ = Trainer(arch, nfeat, N, crit, 4, 0.0)                     # --onorm=target --sqnorm=true
        checkpoint.load(str(model), tr_, arch)
        tr_.plan(B, T, tgt.shape[1])
        tr_.to_device()
        em = tr_.forward(x, train=False).clone()
        Tout = em.shape[1]
        frames = [min(max(-(-min(1 + (n - 400) // 160, T) * Tout // T), 1), Tout) for n, _ in utts]
        spf = 10 / 1000.0 * T / Tout
        if crit == "ctc":
            path, score = criterion.ctc_align(em, tgt, torch.tensor(frames, dtype=torch.int32).cuda())
            assert np.isfinite(score.cpu().numpy()).all()
            path = path.cpu().numpy()
        else:
            fac = ForceAlignmentCriterion(N, transitions=torch.tensor(trans[0].reshape(N, N)).cuda())
            path = np.full((B, Tout), -1, np.int32)
            for b in range(B):
                path[b, :frames[b]] = fac.viterbiPath(em[b:b + 1, :frames[b]].contiguous(), tgt[b:b + 1].contiguous()).cpu().numpy()[0]
        for b, (n, tr) in enumerate(utts):
            words = tr.split()
            spans = text.alignment_token_spans(path[b, :frames[b]], rows[b], blank=N - 1 if crit == "ctc" else None)
            widx = text.target_word_index(words, lex, dic, crit, replabel=replabel, wordsep="|")
            want.append((text.format_alignment_line(f"u{2 * k + b}", text.word_segments(spans, widx, words, frames[b], spf)),
                         frames[b] * spf, words))
    for line, (ref, total, words) in zip(lines, want):
        assert line == ref, (line, ref)
        sample, segs = _parse_line(line)
        assert segs[0][2] == "$" and segs[0][0] == 0.0
        assert [w for _, _, w in segs if w != "$"] == words               # the words in order are the transcript
        t = 0.0
        for begin, length, _ in segs:                                     # ordered, no overlap, no gap (2 decimals printed)
            assert abs(begin - t) <= 0.011 and length >= 0
            t = begin + length
        assert abs(t - total) <= 0.011, (t, total)
