"""Numpy model of the streaming log-mel front end (wav2letter_amd/csrc/host/feat_stream.cpp), in the reference's buffer /
consume form (LogMelFeature.cpp): start empties the buffer, run appends the chunk, produces numFrames(buffered) frames with
oracle.mfsc's per-frame fp64 arithmetic, consumes numFrames x stride samples and keeps the rest; finish drops the rest.  It pins
the index arithmetic independently of the device code, which runs one launch per step over a host-computed count table.
"""
import numpy as np

from oracle import pyoracle


def geometry(fs=16000, frame_ms=25, stride_ms=10):
    """(N, St, nfft, nbins, ldSpec) as features.Mfsc and oracle.mfsc derive them"""
    N, St = int(round(1e-3 * frame_ms * fs)), int(round(1e-3 * stride_ms * fs))
    nfft = 1 << (N - 1).bit_length()
    nb = nfft // 2 + 1
    return N, St, nfft, nb, (nb + 31) // 32 * 32


def num_frames(n, N, St):
    return 0 if n < N else 1 + (n - N) // St


def max_out(max_samples, N, St):
    """frames one step can return: N - 1 carried samples and max_samples new ones"""
    return (N - 1 + max_samples - N) // St + 1


class FeatModel:
    """one stream: step(chunk, start, finish) -> the frames [n][F] that became final.  kw: oracle.mfsc's keyword arguments;
    values=False: the frames are zeros (the count arithmetic alone)"""

    def __init__(self, values=True, **kw):
        self.kw, self.values = kw, values
        self.N, self.St = geometry(kw.get("fs", 16000), kw.get("frame_ms", 25), kw.get("stride_ms", 10))[:2]
        self.F = kw.get("num_filters", 80)
        self.buf = None

    @property
    def active(self):
        return self.buf is not None

    def carry(self):
        return 0 if self.buf is None else len(self.buf)

    def reset(self):
        self.buf = None

    def step(self, x, start=False, finish=False):
        if start:
            self.buf = np.zeros(0, np.float64)
        if self.buf is None:
            assert len(x) == 0 and not finish, "fed or finished before start"
            return np.zeros((0, self.F))
        self.buf = np.concatenate([self.buf, np.asarray(x, np.float64)])
        if self.values:
            y = pyoracle.mfsc(self.buf, **self.kw)   # numFrames(buffered) frames
            assert y.shape[0] == num_frames(len(self.buf), self.N, self.St)
        else:
            y = np.zeros((num_frames(len(self.buf), self.N, self.St), self.F))
        self.buf = self.buf[y.shape[0] * self.St:]
        assert len(self.buf) < self.N
        if finish:
            self.buf = None
        return y


def stream_utterance(model, x, chunks):
    """feeds x [T] in `chunks`; returns (concatenated frames [n][F], frames per step, carried samples after each step)"""
    outs, counts, carries = [], [], []
    pos = 0
    for i, c in enumerate(chunks):
        y = model.step(x[pos:pos + c], start=i == 0, finish=i == len(chunks) - 1)
        pos += c
        outs.append(y)
        counts.append(y.shape[0])
        carries.append(model.carry())
    assert pos == len(x)
    return np.concatenate(outs), counts, carries


def compositions(T):
    """all 2^(T-1) ways to write T as an ordered sum of positive chunks"""
    for mask in range(1 << (T - 1)):
        out, run = [], 1
        for i in range(T - 1):
            if mask >> i & 1:
                out.append(run)
                run = 1
            else:
                run += 1
        out.append(run)
        yield out


def random_chunking(rng, T, max_chunk, p_zero=0.25):
    """chunks of 0..max_chunk samples that sum to T (zero-length chunks included)"""
    out, left = [], T
    while left > 0:
        c = 0 if rng.random() < p_zero else int(rng.integers(1, max_chunk + 1))
        c = min(c, left)
        out.append(c)
        left -= c
    if rng.random() < 0.5:
        out.append(0)   # the utterance ends on an empty chunk
    return out


def fixed(T, c):
    return [c] * (T // c) + ([T % c] if T % c else [])
