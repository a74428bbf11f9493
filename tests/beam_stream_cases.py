"""Inputs shared by test_beam_stream_host.py and test_gpu_beam_stream.py (the incremental CTC beam search, w2l_beam_session_*):
the two emission generators, the LM / lexicon tables (built the way the L2 / X2 cases of test_gpu_ctc_beam_lm.py and
test_gpu_ctc_beam_lex.py build theirs), the chunkings and the step schedule of the three slots."""
import functools

import numpy as np

from tests import ctc_beam_lex_ref as XR
from tests import ctc_beam_lm_ref as LR

F32 = np.float32
INF = float("inf")
LENGTHS = (40, 17, 1)       # the three slots' utterances (clipped to a case's T)
FIRST_STEP = (0, 2, 5)      # the step at which each slot starts


def ints(rng, T, N):
    """test_gpu_ctc_beam._ints for one utterance: multiples of 1/8 in [-3, 0]"""
    return (rng.integers(-24, 1, size=(T, N)) / 8).astype(F32)


def peaked(rng, T, N, hot=None):
    """multiples of 1/8: a background in [-5, -2]; runs of 1-3 frames in which one random class (of the first `hot`) is 0, the
    blank is -[0, 5]/8 and one more class is -[1, 7]/8 -- the repeats, near-ties and merges a real acoustic model makes"""
    x = (rng.integers(-40, -15, size=(T, N)) / 8).astype(F32)
    top = N - 1 if hot is None else hot
    t = 0
    while t < T:
        run = int(rng.integers(1, 4))
        c, c2 = int(rng.integers(0, top)), int(rng.integers(0, top))
        for u in range(t, min(t + run, T)):
            x[u, c2] = -rng.integers(1, 8) / 8
            x[u, c] = 0.0
            x[u, N - 1] = -rng.integers(0, 6) / 8
        t += run
    return x


# name: (generator, hot, T, N, W, K, threshold, seed)
SHAPES = {
    "ints_n5_w16_k4": (ints, None, 40, 5, 16, 4, INF, 0),
    "peaked_n30_w16_k8_thr3": (peaked, None, 40, 30, 16, 8, 3.0, 0),
    "peaked_n30_w64_k64": (peaked, None, 40, 30, 64, 64, INF, 1),
    "peaked_n30_w1_k1": (peaked, None, 40, 30, 1, 1, INF, 2),
    "peaked_n9998_w32_k5": (peaked, 80, 24, 9998, 32, 5, INF, 3),
    "ints_n12300_rows_from_memory": (ints, None, 5, 12300, 8, 64, INF, 4),
}
NONVACUOUS = ("ints_n5_w16_k4", "peaked_n30_w16_k8_thr3")    # the shapes whose hand-over facts the host test proves


@functools.lru_cache(maxsize=None)
def utterances(shape):
    gen, hot, T, N, _, _, _, seed = SHAPES[shape]
    rng = np.random.default_rng(seed)
    first = gen(rng, T, N) if hot is None else gen(rng, T, N, hot)
    rest = [gen(rng, min(n, T), N) if hot is None else gen(rng, min(n, T), N, hot) for n in LENGTHS[1:]]
    return [first] + rest


def smear(tb, nwords):
    """max smearing: wordSmear[w] = q(start, w)"""
    return np.array([tb.score(tb.history(()), w, F32) for w in range(nwords)], F32)


@functools.lru_cache(maxsize=None)
def token_lm(N):
    """a token LM in multiples of 1/8 with BOS and EOS, order 3"""
    rng = np.random.default_rng(1000 + N)
    if N > 1000:
        return LR.random_lm(rng, N - 1, 3, 4000, True, True, (), eighths=True, hot=80)
    return LR.random_lm(rng, N - 1, 3, 300 if N > 10 else 12, True, True, (), eighths=True)


@functools.lru_cache(maxsize=None)
def lexicon_and_word_lm(N):
    """(TextbookTrie, word LM): homophones, a silence token, words that are prefixes of others, values in multiples of 1/8"""
    rng = np.random.default_rng(2000 + N)
    if N > 1000:
        nwords, rows = 3000, None
        rows = XR.random_lexicon(rng, N - 1, nwords, 3, 0.02, None, 80, 0, 1)
        sil = None
    elif N > 10:
        nwords, sil = 300, N - 2
        rows = XR.random_lexicon(rng, N - 1, nwords, 3, 0.1, sil, None, 0, 1)
    else:
        nwords, sil = 14, N - 2
        rows = XR.random_lexicon(rng, N - 1, nwords, 3, 0.2, sil, None, 0, 1)
    tb = LR.random_lm(rng, nwords, 3, 4000 if N > 1000 else 300 if N > 10 else 20, True, True, (), eighths=True)
    return XR.TextbookTrie(rows, N - 1, nwords, smear(tb, nwords), sil), tb


def fixed(T, c):
    return [c] * (T // c) + ([T % c] if T % c else [])


def random_with_zeros(rng, T, max_chunk):
    out, left = [], T
    while left > 0:
        c = 0 if rng.random() < 0.3 else min(int(rng.integers(1, max_chunk + 1)), left)
        out.append(c)
        left -= c
    return out + [0]


CHUNKINGS = ("1", "3", "7", "all", "random")


def chunking(name, T, seed=0):
    if name == "all":
        return [T]
    if name == "random":
        return random_with_zeros(np.random.default_rng(seed + T), T, 9)
    return fixed(T, int(name))


def schedule(xs, chunkings, max_chunk, nan_fill=False):
    """the steps of a session whose slot s gets utterance xs[s] in chunkings[s], starting at FIRST_STEP[s]: a list of
    (emissions [S][max_chunk][N], n [S], start [S]).  Rows nobody may read are 0, or NaN with nan_fill."""
    S, N = len(xs), xs[0].shape[1]
    steps, pos = [], [0] * S
    total = max(FIRST_STEP[s] + len(chunkings[s]) for s in range(S))
    for i in range(total):
        em = np.full((S, max_chunk, N), np.nan if nan_fill else 0.0, F32)
        n, st = np.zeros(S, np.int32), np.zeros(S, np.int32)
        for s in range(S):
            k = i - FIRST_STEP[s]
            if 0 <= k < len(chunkings[s]):
                c = chunkings[s][k]
                em[s, :c] = xs[s][pos[s]:pos[s] + c]
                pos[s] += c
                n[s], st[s] = c, k == 0
        steps.append((em, n, st))
    assert all(pos[s] == xs[s].shape[0] for s in range(S))
    return steps
