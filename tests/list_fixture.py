"""The six-WAV list fixture of the tool tests (the recipe of tests/test_gpu_ctc_align.py): letter tokens, a lexicon, six short WAV
utterances, train.lst and sub/other.lst, and the Train command that makes a CTC checkpoint from them."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_EXE = os.path.join(ROOT, "wav2letter_amd", "bin", "Train")
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
    os.makedirs(d / "out")
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


def _train_cmd(d, run):
    return [TRAIN_EXE, "train", f"--archdir={d / 'arch'}", "--arch=net.arch", "--criterion=ctc", "--filterbanks=40",
            f"--tokensdir={d}", "--tokens=tokens.txt", f"--lexicon={d / 'lexicon.txt'}", f"--datadir={d}", "--train=train.lst",
            "--batchsize=3", "--iter=6", "--reportiters=3", "--lr=0.05", "--lrcrit=0.002", "--momentum=0.8", "--maxgradnorm=1.0",
            "--onorm=target", "--sqnorm=true", f"--rundir={run}", "--runname=exp"]
