"""Numpy model of the chunked streaming protocol (wav2letter_amd/csrc/host/stream.cpp), over a numpy whole-utterance forward
of the same tiny network.  Written in the start / run / finish form -- every layer with a time extent owns a carry, `finish`
cascades layer by layer, a TDS block holds its input frames back until the convolution's output for the same time index
exists -- so it pins the index arithmetic independently of the device code, which runs one pass per step over count tables.

Activations are frame-major [T][F]; a convolution frame is [H][C], C fastest.  Everything runs in the dtype of the input.
"""
import numpy as np

EPS = 1e-5


# ---------------------------------------------------------------------------------------------- layers
class Conv:
    """valid convolution over time on frames [H][cin] -> [H][cout], zero padding padl / padr around the utterance"""

    def __init__(self, w, b, H, stride, padl, padr, relu=False):
        self.w, self.b, self.H, self.stride, self.padl, self.padr, self.relu = w, b, H, stride, padl, padr, relu
        self.kw, self.cin, self.cout = w.shape
        self.carry = None

    def valid(self, x):   # x [n][H*cin] -> [(n - kw) / stride + 1][H*cout]
        n = x.shape[0]
        no = (n - self.kw) // self.stride + 1 if n >= self.kw else 0
        y = np.zeros((no, self.H, self.cout), x.dtype)
        xs = x.reshape(n, self.H, self.cin)
        for i in range(no):
            seg = xs[i * self.stride:i * self.stride + self.kw]            # [kw][H][cin]
            y[i] = np.einsum("khc,kco->ho", seg, self.w) + self.b
        if self.relu:
            y = np.maximum(y, 0)
        return y.reshape(no, self.H * self.cout)

    def whole(self, x):
        F = x.shape[1]
        return self.valid(np.concatenate([np.zeros((self.padl, F), x.dtype), x, np.zeros((self.padr, F), x.dtype)]))

    # streaming
    def start(self, F, dtype):
        self.carry = np.zeros((self.padl, F), dtype)

    def run(self, x):
        buf = np.concatenate([self.carry, x])
        y = self.valid(buf)
        self.carry = buf[y.shape[0] * self.stride:]
        return y

    def finish(self):
        return self.run(np.zeros((self.padr, self.carry.shape[1]), self.carry.dtype))

    def carry_frames(self):
        return [self.carry.shape[0]]


def layernorm(x, g, b):
    m = x.mean(axis=1, keepdims=True)
    v = ((x - m) ** 2).mean(axis=1, keepdims=True)
    return (x - m) / np.sqrt(v + EPS) * g + b


class Local:
    """a frame-local layer: fn maps frames [n][F] -> [n][F']"""

    def __init__(self, fn):
        self.fn = fn

    def whole(self, x):
        return self.fn(x)

    def start(self, F, dtype):
        pass

    def run(self, x):
        return self.fn(x)

    def finish(self):
        return None

    def carry_frames(self):
        return []


class TDS:
    """y1 = LN(relu(conv(x)) + x); out = LN(lin2(relu(lin1(y1))) + y1); conv pads kw - 1 - rpad left, rpad right"""

    def __init__(self, conv, ln1, w1, b1, w2, b2, ln2):
        self.conv, self.ln1, self.w1, self.b1, self.w2, self.b2, self.ln2 = conv, ln1, w1, b1, w2, b2, ln2
        self.held = None

    def tail(self, a, x):
        y1 = layernorm(a + x, *self.ln1)
        u = np.maximum(y1 @ self.w1 + self.b1, 0)
        return layernorm(u @ self.w2 + self.b2 + y1, *self.ln2)

    def whole(self, x):
        return self.tail(self.conv.whole(x), x)

    def start(self, F, dtype):
        self.conv.start(F, dtype)
        self.held = np.zeros((0, F), dtype)

    def _join(self, a):
        n = a.shape[0]
        x, self.held = self.held[:n], self.held[n:]
        return self.tail(a, x)

    def run(self, x):
        self.held = np.concatenate([self.held, x])   # the residual branch waits for the convolution
        return self._join(self.conv.run(x))

    def finish(self):
        return self._join(self.conv.finish())

    def carry_frames(self):
        return self.conv.carry_frames()


def whole_forward(layers, x):
    for l in layers:
        x = l.whole(x)
    return x


class StreamModel:
    """one stream through `layers`: start(), run(chunk) -> new emission frames, finish() -> the flushed ones"""

    def __init__(self, layers, nfeat, dtype=np.float64):
        self.layers, self.nfeat, self.dtype = layers, nfeat, dtype

    def start(self):
        # frame widths along the chain: run an empty chunk through the whole-utterance maps
        x = np.zeros((0, self.nfeat), self.dtype)
        for l in self.layers:
            l.start(x.shape[1], self.dtype)
            x = x if isinstance(l, TDS) else (l.valid(x) if isinstance(l, Conv) else l.fn(x))

    def run(self, x):
        for l in self.layers:
            x = l.run(x)
        return x

    def finish(self):
        x = None
        for l in self.layers:   # the flush cascades: a layer first takes what its producer flushed, then its own right padding
            y = l.run(x) if x is not None else None
            f = l.finish()
            parts = [p for p in (y, f) if p is not None]
            x = np.concatenate(parts) if parts else None
        return x

    def step(self, x, start=False, finish=False):
        """the session's step for one slot: frames that became final"""
        if start:
            self.start()
        y = self.run(x)
        if finish:
            f = self.finish()
            if f is not None:
                y = np.concatenate([y, f])
        return y

    def carry_frames(self):
        return [c for l in self.layers for c in l.carry_frames()]


# ---------------------------------------------------------------------------------------------- the tiny network
NFEAT, NLABEL = 4, 5
# every streamable token, two strides of 2, asymmetric PD, a TDS with rPad = 1 and one with rPad = 0
TINY_ARCH = """V -1 NFEAT 1 0
SAUG 4 2 1 5 1.0 1
PD 0 2 1
C2 1 2 3 1 2 1 0 0
R
DO 0.1
LN 1 2
TDS 2 3 4 0.1 0 1 0
PD 0 3 0
C2 2 3 4 1 2 1 0 0
R
LN 1 2
TDS 3 3 4 0.1 16 0 0
WN 3 C2 3 3 3 1 1 1 1 0
RO 2 1 0 3
V 12 -1 1 0
WN 0 L 12 8
R
L 8 NLABEL
V NLABEL 0 -1 1
"""


def tiny_layers(rng, dtype=np.float64):
    """the numpy twin of TINY_ARCH's time structure (random weights of its own: the device tests compare against the
    trainer's whole forward, the host tests compare this model against whole_forward and its counts against the library's)"""
    def r(*shape):
        return rng.normal(size=shape).astype(dtype) * 0.5

    def tds(c, kw, h, l2, rpad):
        l = c * h
        return TDS(Conv(r(kw, c, c), r(c), h, 1, kw - 1 - rpad, rpad, relu=True), (1.2, -0.1), r(l, l2), r(l2), r(l2, l), r(l), (0.9, 0.2))

    return [
        Conv(r(3, 1, 2), r(2), 4, 2, 2, 1, relu=True),
        Local(lambda x: layernorm(x, 1.1, 0.05)),
        tds(2, 3, 4, 8, 1),
        Conv(r(4, 2, 3), r(3), 4, 2, 3, 0, relu=True),
        Local(lambda x: layernorm(x, 0.8, -0.05)),
        tds(3, 3, 4, 16, 0),
        Conv(r(3, 3, 3), r(3), 4, 1, 1, 1),
        Local(lambda x, w=r(12, 8), b=r(8): np.maximum(x @ w + b, 0)),
        Local(lambda x, w=r(8, NLABEL), b=r(NLABEL): x @ w + b),
    ]


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
    """chunks of 0..max_chunk frames that sum to T (zero-length chunks included)"""
    out, left = [], T
    while left > 0:
        c = 0 if rng.random() < p_zero else int(rng.integers(1, max_chunk + 1))
        c = min(c, left)
        out.append(c)
        left -= c
    if rng.random() < 0.5:
        out.append(0)   # the utterance ends on an empty chunk
    return out


def stream_utterance(model, x, chunks):
    """feeds x [T][F] in `chunks`; returns (concatenated emissions, frames per step, carry counts after each step)"""
    outs, counts, carries = [], [], []
    pos = 0
    for i, c in enumerate(chunks):
        y = model.step(x[pos:pos + c], start=i == 0, finish=i == len(chunks) - 1)
        pos += c
        outs.append(y)
        counts.append(y.shape[0])
        carries.append(model.carry_frames())
    assert pos == x.shape[0]
    return np.concatenate(outs), counts, carries
