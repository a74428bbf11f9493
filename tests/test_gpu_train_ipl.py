"""`Train train --unsup_train=...`: slimIPL in the C++ binary (recipes/slimIPL/src/Train.cpp:73-102, :1141-1168, :1214-1333,
:1362-1415, :1478-1660, :1786-1841) -- the averaged teacher network, training on the model's own transcripts through the four
cache types, labelling that leaves training alone, `continue`, two ranks, the refusals."""
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import ipl_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "wav2letter_amd", "bin", "Train")
ENV = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
UTTS = [(9600, "hello bee"), (6400, "aaa"), (8000, "zoo hello"), (4800, "bee"), (7300, "add zoo"), (5100, "hello")]
TR_ARCH = ("V -1 1 NFEAT 0\nWN 3 C NFEAT 64 3 1 -1\nGLU 2\nDO 0.1\nM 1 1 2 1\nRO 2 0 3 1\n"
           "TR 32 64 4 40 0.1 0.1\nTR 32 64 4 40 0.1 0.1\nDO 0.1\nL 32 NLABEL\n")


def _wav(path, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.asarray(x, "<i2").tobytes())


def _fixture(d):
    """letter tokens + lexicon, six WAV utterances: train.lst (all six), unsup.lst (the six with a garbage transcript column),
    unsup3.lst (three of them: one batch); net.arch (conv_glu with dropout), plain.arch (without), tr.arch (two TR blocks)"""
    from wav2letter_amd import recipes
    os.makedirs(d / "arch")
    os.makedirs(d / "audio")
    (d / "arch" / "net.arch").write_text(recipes.conv_glu_small_arch(widths=(32, 48), kws=(5, 5), drop=0.2))
    (d / "arch" / "plain.arch").write_text(recipes.conv_glu_small_arch(widths=(32, 48), kws=(5, 5), drop=0.0))
    (d / "arch" / "tr.arch").write_text(TR_ARCH)
    letters = ["|", "'"] + [chr(c) for c in range(ord("a"), ord("z") + 1)]
    (d / "tokens.txt").write_text("\n".join(letters) + "\n")
    (d / "lexicon.txt").write_text("".join(f"{w}\t{' '.join(w)} |\n" for w in ["hello", "aaa", "bee", "zoo", "add"]))
    rng = np.random.default_rng(0)
    lines, garbage = [], []
    for k, (n, tr) in enumerate(UTTS):
        t = np.arange(n) / 16000.0
        sig = np.round((0.3 * np.sin(2 * np.pi * (200 + 150 * k) * t) + 0.05 * rng.normal(size=n)) * 30000).astype(np.int16)
        _wav(d / "audio" / f"u{k}.wav", sig)
        lines.append(f"u{k} audio/u{k}.wav {n / 16.0:.1f} {tr}")
        garbage.append(f"p{k} audio/u{k}.wav {n / 16.0:.1f} qqq zz{'z' * k} xkcd")
    (d / "train.lst").write_text("\n".join(lines) + "\n")
    (d / "unsup.lst").write_text("\n".join(garbage) + "\n")
    (d / "unsup3.lst").write_text("\n".join(garbage[1:4]) + "\n")


def _cmd(d, run, extra=(), arch="net.arch", mode="train", where=None):
    base = [EXE, mode] + ([str(where)] if where is not None else [])
    if mode == "train":
        base += [f"--archdir={d / 'arch'}", f"--arch={arch}", "--criterion=asg", "--replabel=2", "--filterbanks=40",
                 f"--tokensdir={d}", "--tokens=tokens.txt", f"--lexicon={d / 'lexicon.txt'}", f"--datadir={d}", "--train=train.lst",
                 f"--unsup_datadir={d}", "--batchsize=3", "--iter=12", "--reportiters=1", "--lr=0.05", "--lrcrit=0.002", "--momentum=0.8",
                 "--maxgradnorm=1.0", "--onorm=target", "--sqnorm=true", "--saug_start_update=2", "--saug_fmaskf=6", "--saug_tmaskt=4",
                 f"--rundir={run}", "--runname=exp"]
    return base + list(extra)


def _run(cmd, ok=True):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=ENV)
    if ok:
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out


def _rows(text):
    r = []
    for line in text.splitlines():
        if line.startswith("epoch:"):
            r.append({k.strip(): v.strip() for k, v in (item.split(":", 1) for item in line.split(" | "))})
    return r


def _net(path):
    """the network tensors of a W2LAMD01 file, in file order"""
    from wav2letter_amd import checkpoint
    h, t = checkpoint.read(str(path))
    return [a for meta, a in zip(h["tensors"], t) if meta["kind"] == "network"]


def _all(path):
    from wav2letter_amd import checkpoint
    return checkpoint.read(str(path))[1]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _cache(path):
    return dict(line.split("|", 1) for line in path.read_text().splitlines())


def _steps(text):
    """the Sup / Unsup / skip lines of a log as ipl_ref.expected_log words them"""
    out = []
    for line in text.splitlines():
        m = re.match(r"Unsup batch \d+ \| (\d+) \| [\d ]+?(?: update cache (\d))?$", line)
        if line.startswith("Sup batch "):
            out.append("sup")
        elif m:
            out.append(f"unsup {m.group(1)}" + (f" {m.group(2)}" if m.group(2) is not None else ""))
        elif line.startswith("Skip usage of unsup batch as fixed cache is not ready"):
            out.append("notready")
        elif line.startswith("Skip update step as unsup data has no label"):
            out.append("skip")
    return out


PLAIN = ["--saug_start_update=-1", "--momentum=0", "--warmup=1"]
CTC = ["--criterion=ctc"]   # runs that train on pseudo-labels: an empty label (an untrained model says little) is an all-blank CTC target


def test_ema_file_is_the_average_and_decay_zero_a_copy(tmp_path):
    """G4: one update with --slimIPL_ema_decay=0.9 leaves 0.9 p0 + 0.1 p1 in 001_model_last_ema.bin (p1: 001_model_last.bin, p0:
    the same command with --lr=0 --lrcrit=0), within w2l_ema_update's bound 4 * 2^-24 * (|0.9 p0| + |0.1 p1|) per element; with
    decay 0 the two files hold the same network bit for bit"""
    d = tmp_path
    _fixture(d)
    _run(_cmd(d, d / "a", ["--iter=1", "--slimIPL_ema=true", "--slimIPL_ema_decay=0.9"]))
    _run(_cmd(d, d / "z", ["--iter=1", "--slimIPL_ema=true", "--slimIPL_ema_decay=0.9", "--lr=0", "--lrcrit=0"]))
    _run(_cmd(d, d / "c", ["--iter=1", "--slimIPL_ema=true", "--slimIPL_ema_decay=0"]))
    p1, ema, p0 = _net(d / "a/exp/001_model_last.bin"), _net(d / "a/exp/001_model_last_ema.bin"), _net(d / "z/exp/001_model_last.bin")
    assert len(p1) == len(ema) == len(p0) > 0
    for e, z in zip(_net(d / "z/exp/001_model_last_ema.bin"), p0):       # nothing moved: the average of p0 with itself, rounded
        assert (np.abs(e.astype(np.float64) - z) <= 4 * 2.0 ** -24 * np.abs(z.astype(np.float64))).all()
    moved = 0
    for a, e, z in zip(p1, ema, p0):
        t0, t1 = 0.9 * z.astype(np.float64), (1.0 - 0.9) * a.astype(np.float64)
        err = np.abs(e.astype(np.float64) - (t0 + t1))
        bound = 4 * 2.0 ** -24 * (np.abs(t0) + np.abs(t1))
        print("G4 worst err / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
        moved += int(not np.array_equal(a, z))
    assert moved > 0
    assert _same(_net(d / "c/exp/001_model_last_ema.bin"), _net(d / "c/exp/001_model_last.bin"))
    assert _same(_net(d / "c/exp/001_model_last.bin"), p1)               # the student is the student of run a


def test_cache_and_naive_modes_are_supervised_training_on_the_models_own_output(tmp_path):
    """G5: no dropout, no SpecAugment, momentum 0, constant learning rate, pseudo-labels alone (sup:unsup 0:1) on an unsupervised
    list of one batch with a garbage transcript column.  cache: update 1 is skipped and leaves the initial model's labels in the
    cache, update 2 trains on them -- the parameters equal, bit for bit, ONE supervised update on the same audio with those texts
    as transcripts; the cache then holds what the UPDATED model says (a fresh labelling of it through `fork`).  naive with one
    update: the same labels (its "PL for index" lines) and the same parameters."""
    d = tmp_path
    _fixture(d)
    ipl = ["--unsup_train=unsup3.lst", "--slimIPL_sup_updates=0", "--slimIPL_unsup_updates=1", "--w2l_ipl_print_every=1"] + PLAIN + CTC
    one = _run(_cmd(d, d / "c1", ipl + ["--slimIPL_type=cache", "--iter=1"], arch="plain.arch"))
    two = _run(_cmd(d, d / "c2", ipl + ["--slimIPL_type=cache", "--iter=2"], arch="plain.arch"))
    assert _steps(one.stdout) == ["unsup 0", "skip"] and _steps(two.stdout) == ["unsup 0", "skip", "unsup 0"]
    first = _cache(d / "c1/exp/001_model_last_cache0")
    ids = ["p1", "p2", "p3"]
    assert sorted(first) == ids
    audio = {l.split()[0]: l.split()[1:3] for l in (d / "unsup3.lst").read_text().splitlines()}
    (d / "pl.lst").write_text("".join(f"{i} {audio[i][0]} {audio[i][1]} {first[i]}\n" for i in ids))
    sup = _run(_cmd(d, d / "s", ["--train=pl.lst", "--iter=1"] + PLAIN + CTC, arch="plain.arch"))
    want = _all(d / "s/exp/001_model_last.bin")
    assert _same(_all(d / "c2/exp/001_model_last.bin"), want)
    assert not _same(want, _all(d / "c1/exp/001_model_last.bin"))        # (the update did move the model)
    assert _rows(two.stdout)[-1]["loss Unsup"] == _rows(sup.stdout)[-1]["loss"]
    # the cache after update 2: the updated model's labels
    pl = lambda text: [l.split(": ", 1)[1] if ": " in l else "" for l in text.splitlines() if l.startswith("PL for index")]
    fresh = _run(_cmd(d, d / "f", ["--slimIPL_type=naive", "--iter=1", "--lr=0", "--lrcrit=0", f"--rundir={d / 'f'}"], mode="fork",
                      where=d / "c2/exp/001_model_last.bin"))
    second = _cache(d / "c2/exp/001_model_last_cache0")
    assert [second[i] for i in ids] == pl(fresh.stdout)[:3]
    # naive, one update: labels of the initial model, then the same supervised update
    nv = _run(_cmd(d, d / "n", ipl + ["--slimIPL_type=naive", "--iter=1"], arch="plain.arch"))
    assert pl(nv.stdout) == [first[i] for i in ids] and _steps(nv.stdout) == ["unsup 0"]
    assert _same(_all(d / "n/exp/001_model_last.bin"), want)
    assert not (d / "n/exp/001_model_last_cache0").exists()


def test_labelling_leaves_training_untouched(tmp_path):
    """G6: dropout and SpecAugment on.  An unsupervised list that is never used (sup:unsup 1:0) gives the run without the list,
    bit for bit; with sup:unsup 1:1 in pre-cache mode the supervised updates log the losses of the plain run up to the first
    unsupervised step (the teacher's forwards move no dropout seed and no SpecAugment counter)"""
    d = tmp_path
    _fixture(d)
    plain = _run(_cmd(d, d / "plain", ["--iter=6"]))
    idle = _run(_cmd(d, d / "idle", ["--iter=6", "--unsup_train=unsup.lst", "--slimIPL_sup_updates=1", "--slimIPL_unsup_updates=0",
                                     "--slimIPL_type=pre-cache"]))
    assert "Unsup is in use 1" in idle.stdout and _steps(idle.stdout) == ["sup"] * 6
    assert [r["loss"] for r in _rows(idle.stdout)] == [r["loss"] for r in _rows(plain.stdout)]
    assert _same(_all(d / "idle/exp/001_model_last.bin"), _all(d / "plain/exp/001_model_last.bin"))
    seed = next(s for s in range(50) if ipl_ref.expected_log("pre-cache", 1, 1, 2, 2, 1.0, s, 3, 2)[0][:3] == ["sup", "unsup 0", "skip"])
    base = _run(_cmd(d, d / "b", ["--iter=6", f"--seed={seed}"] + CTC))
    mix = _run(_cmd(d, d / "m", CTC + ["--iter=6", f"--seed={seed}", "--unsup_train=unsup.lst", "--slimIPL_sup_updates=1", "--slimIPL_unsup_updates=1",
                                 "--slimIPL_type=pre-cache"]))
    steps = _steps(mix.stdout)
    assert steps == ipl_ref.expected_log("pre-cache", 1, 1, 2, 2, 1.0, seed, 6, 2)[0]
    n_sup = steps.index("unsup 0")
    assert n_sup >= 1 and "PL Quality for Batch" in mix.stdout
    # (a supervised update AFTER an unsupervised step draws the dropout seed of its own update number on another batch: only the
    # updates before the first unsupervised step are comparable)
    assert [r["loss"] for r in _rows(mix.stdout)[:n_sup]] == [r["loss"] for r in _rows(base.stdout)[:n_sup]]


def test_decay_zero_teacher_is_the_student_under_mixed_precision(tmp_path):
    """G7: bf16 products, two TR blocks, naive labelling.  --slimIPL_ema_decay=0 makes the averaged network a copy of the student
    after every update, so four updates end in the model of --slimIPL_ema=false, bit for bit -- a teacher that kept bf16 weight
    images or weight-norm products of its old parameters would label differently"""
    d = tmp_path
    _fixture(d)
    common = ["--arch=tr.arch", "--criterion=ctc", "--iter=4", "--fl_amp_use_mixed_precision=true", "--unsup_train=unsup.lst",
              "--slimIPL_type=naive", "--slimIPL_sup_updates=1", "--slimIPL_unsup_updates=3", "--lr=0.1", "--w2l_ipl_print_every=1"]
    off = _run(_cmd(d, d / "off", common + ["--slimIPL_ema=false"]))
    on = _run(_cmd(d, d / "on", common + ["--slimIPL_ema=true", "--slimIPL_ema_decay=0"]))
    assert _steps(on.stdout) == _steps(off.stdout) and _steps(on.stdout).count("sup") < 4
    assert [l for l in on.stdout.splitlines() if l.startswith("PL ")] == [l for l in off.stdout.splitlines() if l.startswith("PL ")]
    assert _same(_all(d / "on/exp/001_model_last.bin"), _all(d / "off/exp/001_model_last.bin"))
    assert _same(_net(d / "on/exp/001_model_last_ema.bin"), _net(d / "on/exp/001_model_last.bin"))
    assert not (d / "off/exp/001_model_last_ema.bin").exists()


def test_fixed_pre_cache_end_to_end(tmp_path):
    """G8: a cache of two batch indices, relabelled with probability 0.5, 12 updates: the Sup / Unsup / skip lines are the ones
    tests/ipl_ref.py predicts for the seed, the losses are finite, the fixed cache file holds two indices and the text cache a
    line for every sample of every labelled batch"""
    d = tmp_path
    _fixture(d)
    out = _run(_cmd(d, d / "r", CTC + ["--unsup_train=unsup.lst", "--slimIPL_type=fixed-pre-cache", "--slimIPL_fixed_cache_updates=2",
                                 "--slimIPL_fixed_cache_update_prob=0.5", "--seed=3"]))
    want, labelled, fixed = ipl_ref.expected_log("fixed-pre-cache", 1, 3, 2, 2, 0.5, 3, 12, 2)
    assert _steps(out.stdout) == want
    assert "notready" in want and any(w.endswith(" 0") for w in want if w.startswith("unsup")) and "sup" in want
    rows = _rows(out.stdout)
    assert len(rows) == 12
    assert all(np.isfinite(float(r["loss"])) and np.isfinite(float(r["loss Unsup"])) for r in rows)
    assert any(float(r["loss Unsup"]) > 0 for r in rows)
    assert [int(v) for v in (d / "r/exp/001_model_last_fixed_cache0").read_text().split()] == fixed and len(fixed) == 2
    ids = [f"p{k}" for b in labelled for k in range(3 * b, 3 * b + 3)]
    assert sorted(_cache(d / "r/exp/001_model_last_cache0")) == sorted(ids)


def test_continue_goes_on_where_the_run_stopped(tmp_path):
    """G9: cache mode with the averaged teacher: 3 updates + `continue` to 6 end where 6 updates in one run end -- student,
    teacher and the text cache, bit for bit (one unsupervised batch, so the continued run relabels everything the cache file
    held: the reference reloads a cache file read-only and writes only what the new run touched)"""
    d = tmp_path
    _fixture(d)
    ipl = ["--unsup_train=unsup3.lst", "--slimIPL_type=cache", "--slimIPL_sup_updates=1", "--slimIPL_unsup_updates=1", "--slimIPL_ema=true",
           "--slimIPL_ema_decay=0.9"] + CTC
    whole = _run(_cmd(d, d / "w", ipl + ["--iter=6"]))
    _run(_cmd(d, d / "p", ipl + ["--iter=3"]))
    cont = _run([EXE, "continue", str(d / "p/exp"), "--iter=6"])
    assert "Reading PL cache is done; total size 3" in cont.stdout
    assert _steps(whole.stdout)[-len(_steps(cont.stdout)):] == _steps(cont.stdout) and "sup" in _steps(cont.stdout)
    assert any(s.startswith("unsup") for s in _steps(cont.stdout))
    assert _same(_all(d / "p/exp/002_model_last.bin"), _all(d / "w/exp/001_model_last.bin"))
    assert _same(_net(d / "p/exp/002_model_last_ema.bin"), _net(d / "w/exp/001_model_last_ema.bin"))
    assert not _same(_net(d / "w/exp/001_model_last_ema.bin"), _net(d / "w/exp/001_model_last.bin"))
    assert (d / "p/exp/002_model_last_cache0").read_bytes() == (d / "w/exp/001_model_last_cache0").read_bytes()
    assert len(_cache(d / "w/exp/001_model_last_cache0")) == 3


def test_two_ranks_skip_together_and_stay_identical(tmp_path):
    """G10: two processes on one GPU through the host-memory test collective, cache mode, pseudo-labels alone: update 1 is skipped
    on both ranks, the replicas are bit-identical after four updates, "PL Quality" is printed by rank 0 alone and its last value is
    the WER of both ranks' cached labels against the transcript column"""
    from wav2letter_amd import text
    d = tmp_path
    _fixture(d)
    shm = f"/dev/shm/w2l_test_ipl_{os.getpid()}"
    extra = CTC + ["--iter=4", "--unsup_train=unsup.lst", "--slimIPL_type=cache", "--slimIPL_sup_updates=0", "--slimIPL_unsup_updates=1",
             "--w2l_save_all_ranks=true", "--enable_distributed=true", "--world_size=2", f"--rndv_filepath=shm:{shm}"]
    procs = [subprocess.Popen(_cmd(d, d / "R", extra + [f"--world_rank={r}"]), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=ENV)
             for r in (0, 1)]
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, o, e))
    for rc, o, e in outs:
        assert rc == 0, (o[-2000:], e[-2000:])
    for _, o, _ in outs:
        assert _steps(o) == ["unsup 0", "skip", "unsup 0", "unsup 0", "unsup 0"]
    assert _same(_all(d / "R/exp/001_model_last.bin"), _all(d / "R/exp/001_model_last.bin.rank1"))
    q0 = [float(l.rsplit(":", 1)[1]) for l in outs[0][1].splitlines() if l.startswith("PL Quality for Batch")]
    assert len(q0) == 5 and "PL Quality" not in outs[1][1]            # update 1 labels before and after the skipped update
    c0, c1 = _cache(d / "R/exp/001_model_last_cache0"), _cache(d / "R/exp/001_model_last_cache1")
    assert sorted(c0) == ["p0", "p1", "p2"] and sorted(c1) == ["p3", "p4", "p5"]
    ref = {l.split()[0]: l.split()[3:] for l in (d / "unsup.lst").read_text().splitlines()}
    wer = text.EditDistanceMeter()
    for i, t in {**c0, **c1}.items():
        wer.add(t.split(), ref[i])
    assert abs(q0[-1] - wer.value()) <= 1e-4 * max(1.0, wer.value()), (q0, wer.value())


@pytest.mark.parametrize("flags,name", [
    (["--slimIPL_use_soft=true", "--unsup_train=unsup.lst"], "--slimIPL_use_soft"),
    (["--unsup_train=unsup.lst", "--train=[DATA_DST]/train.lst", "--w2l_nlabel=30"], "--unsup_train"),
    (["--unsup_train=unsup.lst", "--slimIPL_type=semi-cache"], "--slimIPL_type"),
    (["--slimIPL_ema=true", "--slimIPL_ema_decay=1.5"], "--slimIPL_ema_decay"),
    (["--slimIPL_ema=true", "--slimIPL_ema_decay=-0.1"], "--slimIPL_ema_decay"),
])
def test_refusals_name_the_flag_before_any_training(tmp_path, flags, name):
    """G11"""
    d = tmp_path
    _fixture(d)
    out = _run(_cmd(d, d / "x", flags + ["--iter=2"]), ok=False)
    assert out.returncode != 0 and name in out.stderr, (out.returncode, out.stderr[-500:])
    assert "epoch:" not in out.stdout and not (d / "x/exp/001_model_last.bin").exists()
