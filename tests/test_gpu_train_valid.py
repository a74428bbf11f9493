"""`Train train --valid=...`: the reference Trainer's validation (test(), recipes/slimIPL/src/Train.cpp:874-980) in the C++ binary --
`<tag>-loss | <tag>-TER | <tag>-WER` on every log line (MyLogger.cpp:60-70), NNN_model_<tag>.bin on a new best WER (:783-800),
and a training run that is bit for bit the one without --valid."""
import os
import subprocess
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "wav2letter_amd", "bin", "Train")
ENV = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
UTTS = [(9600, "hello bee"), (6400, "aaa"), (8000, "zoo hello"), (4800, "bee"), (7300, "add zoo"), (5100, "hello")]


def _wav(path, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.asarray(x, "<i2").tobytes())


def _fixture(d):
    """letter tokens + lexicon, six WAV utterances; train.lst, dev.lst (3 of them) and sub/other.lst (5: a short last batch)"""
    from wav2letter_amd import recipes
    os.makedirs(d / "arch")
    os.makedirs(d / "audio")
    os.makedirs(d / "sub")
    (d / "arch" / "net.arch").write_text(recipes.conv_glu_small_arch(widths=(32, 48), kws=(5, 5), drop=0.2))
    letters = ["|", "'"] + [chr(c) for c in range(ord("a"), ord("z") + 1)]
    (d / "tokens.txt").write_text("\n".join(letters) + "\n")
    (d / "lexicon.txt").write_text("".join(f"{w}\t{' '.join(w)} |\n" for w in ["hello", "aaa", "bee", "zoo", "add"]))
    rng = np.random.default_rng(0)
    lines = []
    for k, (n, tr) in enumerate(UTTS):
        t = np.arange(n) / 16000.0
        sig = np.round((0.3 * np.sin(2 * np.pi * (200 + 150 * k) * t) + 0.05 * rng.normal(size=n)) * 30000).astype(np.int16)
        _wav(d / "audio" / f"u{k}.wav", sig)
        lines.append(f"u{k} audio/u{k}.wav {n / 16.0:.1f} {tr}")
    (d / "train.lst").write_text("\n".join(lines) + "\n")
    (d / "dev.lst").write_text("\n".join(lines[1::2]) + "\n")
    (d / "sub" / "other.lst").write_text("\n".join(lines[:5]) + "\n")


def _cmd(d, run, extra=()):
    return [EXE, "train", f"--archdir={d / 'arch'}", "--arch=net.arch", "--criterion=asg", "--replabel=2", "--filterbanks=40",
            f"--tokensdir={d}", "--tokens=tokens.txt", f"--lexicon={d / 'lexicon.txt'}", f"--datadir={d}", "--train=train.lst",
            "--batchsize=3", "--iter=12", "--reportiters=4", "--lr=0.05", "--lrcrit=0.002", "--momentum=0.8", "--maxgradnorm=1.0",
            "--onorm=target", "--sqnorm=true", "--saug_start_update=2", "--saug_fmaskf=6", "--saug_tmaskt=4", f"--rundir={run}",
            "--runname=exp"] + list(extra)


def _rows(text):
    r = []
    for line in text.splitlines():
        if line.startswith("epoch:"):
            r.append({k.strip(): v.strip() for k, v in (item.split(":", 1) for item in line.split(" | "))})
    return r


def _run(cmd):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out


VALID = "--valid=dev:dev.lst,sub/other:sub/other.lst"


def test_valid_columns_best_models_and_untouched_training(tmp_path):
    from wav2letter_amd import checkpoint
    d = tmp_path
    _fixture(d)
    plain = _run(_cmd(d, d / "plain"))
    out = _run(_cmd(d, d / "valid", [VALID, "--validbatchsize=2"]))
    assert "[Valid] dev: 3 samples, 3 on this rank, 2 batches of 2" in out.stdout
    assert "[Valid] sub/other: 5 samples, 5 on this rank, 3 batches of 2" in out.stdout
    rows, rows0 = _rows(out.stdout), _rows(plain.stdout)
    assert [int(r["nupdates"]) for r in rows] == [4, 8, 12]
    for r in rows:
        keys = list(r)
        i = keys.index("train-WER")
        assert keys[i + 1:i + 7] == ["dev-loss", "dev-TER", "dev-WER", "sub/other-loss", "sub/other-TER", "sub/other-WER"]
        for tag in ("dev", "sub/other"):
            assert np.isfinite(float(r[f"{tag}-loss"]))
            assert 0.0 <= float(r[f"{tag}-TER"]) <= 1000.0 and 0.0 <= float(r[f"{tag}-WER"]) <= 1000.0
    # the training run is the one without --valid: dropout, SpecAugment and the data order untouched
    assert [r["loss"] for r in rows] == [r["loss"] for r in rows0]
    assert [r["train-TER"] for r in rows] == [r["train-TER"] for r in rows0]
    _, t_plain = checkpoint.read(str(d / "plain" / "exp" / "001_model_last.bin"))
    _, t_valid = checkpoint.read(str(d / "valid" / "exp" / "001_model_last.bin"))
    assert len(t_plain) == len(t_valid) and all(np.array_equal(a, b) for a, b in zip(t_plain, t_valid))
    # the best model of each set ('/' -> '#'), in the W2LAMD01 container
    for name in ("001_model_dev.bin", "001_model_sub#other.bin"):
        p = d / "valid" / "exp" / name
        assert p.exists(), sorted(os.listdir(d / "valid" / "exp"))
        h, t = checkpoint.read(str(p))
        assert len(t) == len(t_valid)
    # the log file carries the same columns
    log = (d / "valid" / "exp" / "001_log").read_text()
    assert "dev-WER" in log and "sub/other-loss" in log


def test_valid_tag_defaults_to_the_path_and_synthetic_runs_ignore_valid(tmp_path):
    d = tmp_path
    _fixture(d)
    out = _run(_cmd(d, d / "r", ["--valid=dev.lst", "--iter=4"]))
    r = _rows(out.stdout)[-1]
    assert "dev.lst-loss" in r and "dev.lst-WER" in r
    assert (d / "r" / "exp" / "001_model_dev.lst.bin").exists()
    syn = _run(_cmd(d, d / "s", ["--train=[DATA_DST]/train.lst", "--w2l_nlabel=30", "--iter=2", "--reportiters=1", "--w2l_synth_frames=64",
                                 "--w2l_synth_target_len=8", "--valid=dev:dev.lst"]))
    assert "[Valid] --valid is ignored" in syn.stdout
    assert all("dev-loss" not in r for r in _rows(syn.stdout))


def test_missing_valid_list_fails_cleanly(tmp_path):
    d = tmp_path
    _fixture(d)
    out = subprocess.run(_cmd(d, d / "m", ["--valid=dev:nope.lst"]), capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 1
    assert "cannot read the list file" in out.stderr and "nope.lst" in out.stderr and "--valid" in out.stderr


def test_valid_numbers_equal_python_evaluate_of_the_saved_model(tmp_path):
    """a valid set equal to the train list: the binary's dev-loss / dev-TER / dev-WER of its last log line (scored with the model
    it then saves as 001_model_last.bin) equal Trainer.evaluate of that checkpoint loaded through the Python front end, on the
    features the binary computed for that list (--w2l_dump_features: update 1 trains on the whole list, in list order) and the
    targets of the Python text pipeline, turned into TER / WER by text.eval_output"""
    import torch
    from wav2letter_amd import checkpoint, text
    from wav2letter_amd.trainer import Trainer
    d = tmp_path
    _fixture(d)
    out = _run(_cmd(d, d / "r", ["--valid=dev:train.lst", "--batchsize=6", "--validbatchsize=6", "--iter=4", "--reportiters=4",
                                 f"--w2l_dump_features={d / 'feat'}"]))
    row = _rows(out.stdout)[-1]
    raw = (d / "feat.1").read_bytes()
    B, nfeat, T = np.frombuffer(raw[:12], np.int32)
    x = torch.tensor(np.frombuffer(raw[12:], np.float32).reshape(B, nfeat, T).copy()).cuda()
    letters = ["|", "'"] + [chr(c) for c in range(ord("a"), ord("z") + 1)]
    dic = text.create_token_dict(letters, "asg", replabel=2)
    lex = text.load_lexicon((d / "lexicon.txt").read_text().splitlines())
    tgt = text.pad_targets([text.target_indices(tr.split(), lex, dic, "asg", replabel=2, wordsep="|") for _, tr in UTTS])
    arch = (d / "arch" / "net.arch").read_text()
    tr = Trainer(arch, int(nfeat), dic.index_size(), "asg", 4, 0.0)   # --onorm=target --sqnorm=true: TARGET_SZ_SQRT
    checkpoint.load(str(d / "r" / "exp" / "001_model_last.bin"), tr, arch)
    tr.plan(int(B), int(T), tgt.shape[1])
    tr.to_device()
    loss, path = tr.evaluate(x, torch.tensor(tgt).cuda())
    loss = loss.cpu().numpy().astype(np.float64)
    mean = 0.0
    for v in loss:
        mean += v
    mean /= len(loss)
    assert abs(float(row["dev-loss"]) - mean) <= 1e-4 * max(1.0, abs(mean)), (row["dev-loss"], loss)
    ter, wer = text.eval_output(path.cpu().numpy(), tgt, dic, "asg", replabel=2, wordsep="|")
    assert row["dev-TER"] == f"{ter.value():5.2f}".strip() and row["dev-WER"] == f"{wer.value():5.2f}".strip(), (row, ter.value(), wer.value())


def test_two_ranks_log_the_valid_numbers_of_one_process(tmp_path):
    """two processes on one GPU through the host-memory test collective: each scores its round-robin share and the sums are
    all-reduced, so rank 0 logs what a one-process run logs.  lr = 0 keeps the two runs' models identical, and one-utterance valid
    batches make every utterance's loss independent of which rank scores it: the valid columns must agree exactly"""
    d = tmp_path
    _fixture(d)
    same = [VALID, "--validbatchsize=1", "--iter=2", "--reportiters=2", "--lr=0", "--lrcrit=0", "--momentum=0"]
    one = _run(_cmd(d, d / "one", same + ["--batchsize=6"]))
    shm = f"/dev/shm/w2l_test_valid_{os.getpid()}"
    procs = [subprocess.Popen(_cmd(d, d / f"R{r}", same + ["--enable_distributed=true", f"--world_rank={r}", "--world_size=2",
                                                           f"--rndv_filepath=shm:{shm}"]),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=ENV) for r in (0, 1)]
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
        assert rc == 0, (o[-1500:], e[-1500:])
    r2, r1 = _rows(outs[0][1]), _rows(one.stdout)
    assert r2 and [list(r) for r in r2][0][:-1] == [list(r) for r in r1][0][:-1]   # (timestamp last)
    assert "[Valid] dev: 3 samples, 2 on this rank" in outs[0][1] and "[Valid] dev: 3 samples, 1 on this rank" in outs[1][1]
    assert "[Valid] sub/other: 5 samples, 3 on this rank" in outs[0][1] and "[Valid] sub/other: 5 samples, 2 on this rank" in outs[1][1]
    for tag in ("dev", "sub/other"):
        for k in ("loss", "TER", "WER"):
            assert r2[-1][f"{tag}-{k}"] == r1[-1][f"{tag}-{k}"], (tag, k, r2[-1], r1[-1])
        assert np.isfinite(float(r2[-1][f"{tag}-loss"]))
