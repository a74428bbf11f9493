"""Audio in, labels out, as the audio arrives: the shape of the reference's AudioToWords
(recipes/streaming_convnets/inference/inference/examples/AudioToWords.cpp) over this project's three streaming sessions:

    python tools/audio_to_words.py [--wav FILE | --seconds 3 --seed 1] [--chunk-ms 160] [--commit-every 4]
                                   [--arch FILE] [--nlabel 29] [--checkpoint FILE] [--tokens FILE] [--beam 16]
                                   [--local-norm-left N] [--beam-token K] [--sil-token C] [--sil-score X]

    samples -> StreamingFeatures (log-mel, one launch per step) [-> StreamingLocalNorm (windowed normalisation, one launch per
    step, in place)] -> StreamingSession (chunked forward) -> StreamingDecoder (incremental CTC beam search), commit() every few
    steps.

The audio is a 16-bit mono WAV file, or a seeded synthetic signal (a few drifting tones in noise).  It is cut into chunks of
--chunk-ms and fed as int16, one chunk per step; every --commit-every steps the decoder commits what can no longer change, and
the tool prints those labels as they become final, then the tail at the end.  Without --checkpoint the network has its seeded
initial parameters and the labels are noise: a run of the plumbing.  --arch defaults to the streaming TDS-CTC recipe's;
--tokens names the labels (one per line), else their numbers are printed.  Without --local-norm-left the features are not
normalised (a model trained through the Python trainer and PrefetchLoader(local_norm=None) sees them that way);
--local-norm-left=N normalises every frame over itself and the N frames before it, the features a model trained with
--localnrmlleftctx=N (and no right context) through `Train` or PrefetchLoader(local_norm=(N, 0)) sees.
--beam-token (default: the beam, at most the token classes), --sil-token and --sil-score are the decoder's --beamsizetoken and
--silscore.  With none of the three and --beam up to 64 the decoder is StreamingDecoder, as before; a beam up to 1024 with at most
64 tokens is WideStreamingDecoder; more than 64 tokens per frame, a beam above 1024 or a silence score pick
ManyTokenStreamingDecoder (the streaming recipe's 500 / 100 is --beam=500 --beam-token=100), which commits at a beam up to 1024:
above that the tool prints the whole hypothesis at the end."""
import argparse
import os
import sys
import wave

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wav2letter_amd import checkpoint, recipes
from wav2letter_amd.features import Mfsc
from wav2letter_amd.streaming import (ManyTokenStreamingDecoder, StreamingDecoder, StreamingFeatures, StreamingLocalNorm, StreamingSession,
                                     WideStreamingDecoder)
from wav2letter_amd.trainer import Trainer


def read_wav(path):
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2 or w.getnchannels() != 1:
            raise SystemExit(f"{path}: 16-bit mono WAV expected")
        return np.frombuffer(w.readframes(w.getnframes()), np.int16).copy(), w.getframerate()


def synthetic(seconds, fs, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * fs)) / fs
    x = 0.02 * rng.normal(size=t.size)
    for _ in range(4):
        f0, f1 = rng.uniform(150, 3000, size=2)
        x += 0.15 * np.sin(2 * np.pi * (f0 + (f1 - f0) * t / max(seconds, 1e-3) / 2) * t)
    return np.clip(np.round(x * 32767 / 2), -32768, 32767).astype(np.int16)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--wav")
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fs", type=int, default=16000, help="rate of the synthetic signal")
    ap.add_argument("--chunk-ms", type=int, default=160)
    ap.add_argument("--commit-every", type=int, default=4)
    ap.add_argument("--arch")
    ap.add_argument("--nlabel", type=int, default=29)
    ap.add_argument("--filters", type=int, default=80)
    ap.add_argument("--mel-floor", type=float, default=1.0)
    ap.add_argument("--checkpoint")
    ap.add_argument("--tokens")
    ap.add_argument("--beam", type=int, default=16)
    ap.add_argument("--local-norm-left", type=int, default=None, help="normalise over this many frames of left context")
    ap.add_argument("--beam-token", type=int, default=None, help="tokens kept per frame (default: the beam)")
    ap.add_argument("--sil-token", type=int, default=None, help="the silence class of --sil-score")
    ap.add_argument("--sil-score", type=float, default=0.0, help="added to the silence class's frame score")
    a = ap.parse_args()

    x, fs = read_wav(a.wav) if a.wav else (synthetic(a.seconds, a.fs, a.seed), a.fs)
    arch = open(a.arch).read() if a.arch else recipes.streaming_tds_arch()
    names = [l.strip() for l in open(a.tokens)] if a.tokens else None
    show = (lambda ids: " ".join(names[i] if names and i < len(names) else str(i) for i in ids))

    tr = Trainer(arch, a.filters, a.nlabel, "ctc")
    tr.init_params(a.seed)
    if a.checkpoint:
        checkpoint.load(a.checkpoint, tr, arch)
    tr.to_device()

    fe = Mfsc(num_filters=a.filters, fs=fs, mel_floor=a.mel_floor)
    chunk = max(1, fs * a.chunk_ms // 1000)
    feats = StreamingFeatures(fe, 1, chunk)
    norm = StreamingLocalNorm(a.filters, 1, feats.max_out, a.local_norm_left) if a.local_norm_left is not None else None
    net = StreamingSession(tr, 1, feats.max_out)
    max_frames = fe.num_frames(len(x)) + 64   # emission frames never outnumber feature frames (plus the flush)
    tokens = min(a.beam if a.beam_token is None else a.beam_token, a.nlabel - 1)
    if tokens > 64 or a.beam > 1024 or a.sil_score != 0.0:
        dec = ManyTokenStreamingDecoder(1, net.max_out, max_frames, a.nlabel, beam=a.beam, beam_token=tokens, sil_token=a.sil_token,
                                        sil_score=a.sil_score)
    elif a.beam > 64:
        dec = WideStreamingDecoder(1, net.max_out, max_frames, a.nlabel, beam=a.beam, beam_token=tokens)
    else:
        dec = StreamingDecoder(1, net.max_out, max_frames, a.nlabel, beam=a.beam, beam_token=tokens)
    commits = a.beam <= 1024 or not isinstance(dec, ManyTokenStreamingDecoder)

    pcm = torch.zeros(1, chunk, dtype=torch.int16, device="cuda")
    steps = max(1, -(-len(x) // chunk))
    frames = emitted = 0
    for i in range(steps):
        part = x[i * chunk:(i + 1) * chunk]
        pcm[0, :len(part)] = torch.from_numpy(part).cuda()
        st, fi = [int(i == 0)], [int(i == steps - 1)]
        f, nf = feats.step(pcm, [len(part)], st, fi)
        if norm is not None:
            norm.step(f, nf, st)   # in place, on the feature step's view
        out, n_out = net.step(f, nf, st, fi)
        dec.step(out, n_out, st)
        frames += int(nf[0])
        emitted += int(n_out[0])
        if commits and ((i + 1) % a.commit_every == 0 or i == steps - 1):
            labels, _ = dec.commit()[0]
            if len(labels):
                print(f"[{(i + 1) * chunk / fs:7.2f} s] {show(labels)}", flush=True)
    labels, lengths, scores = dec.result()
    tail = labels[0, 0, :max(int(lengths[0, 0]), 0)].cpu().numpy()
    print(f"[   tail  ] {show(tail)}")
    done = dec.committed(0)[0]
    stages = "features -> local norm (left %d) -> network -> decoder" % a.local_norm_left if norm is not None else "features -> network -> decoder"
    print(f"{stages}: {len(x)} samples at {fs} Hz in {steps} steps of {a.chunk_ms} ms: {frames} feature frames, {emitted} emission frames, "
          f"{len(done)} labels committed + {len(tail)} in the tail, score {float(scores[0, 0]):.3f}")
