"""numpy restatements for the LocalNorm tests (tests/test_local_norm_host.py, tests/test_gpu_local_norm.py).

contract()   the contract of include/w2l_hip.h (w2l_local_norm), step for step in float64 / float32.
reference()  the reference's streaming recurrence (recipes/streaming_convnets/inference/inference/module/nn/LocalNorm.cpp), written
             from its description: per frame the sum and the sum of squares (the squares are fp32 products) accumulated in double
             and stored as fp32; the stored values form a list that loses its oldest entry once it is longer than L; the list's
             totals are accumulated in double and stored as fp32; mean and deviation are fp32, a deviation at or below 1e-5 becomes
             1, the output is (x - mean) / deviation in fp32.

Inputs are [F][n] float32 (time fastest, as on the device)."""
import numpy as np

EPS = np.float64(np.float32(1e-5))

# worst |reference() - contract()| over every utterance of the GPU tests' grid (cases() below), measured on the CPU by
# test_local_norm_host.py::test_reference_recurrence_against_the_contract, which asserts it.  It only separates fp32-sum from
# fp64-sum roundings; the GPU's session is given four times this against reference().
REF_VS_CONTRACT_WORST = 6.7e-6   # measured 6.676e-6 at F = 3, L = 2, T = 4 (outputs are of order 1); a window one frame off: 0.16

FS = (3, 80)
LS = (0, 1, 2, 7, 300)
RS = (0, 1, 5)


def lengths(L):
    """the T of the grid for a left context L: 1, 2, L, L + 1, L + 2, 2 L + 5 (those that are at least 1)"""
    return sorted({t for t in (1, 2, L, L + 1, L + 2, 2 * L + 5) if t >= 1})


def features(F, T, seed):
    """log-mel-like features: N(5, 3)"""
    return np.random.default_rng([seed, F, T]).normal(5.0, 3.0, size=(F, T)).astype(np.float32)


def _seq_sum(a):
    """the sum of the rows of a [k][n] float64 array, row 0 first, one rounding per addition (np.sum adds pairwise)"""
    acc = np.zeros(a.shape[1], np.float64)
    for row in a:
        acc = acc + row
    return acc


def contract(x, left, right=0):
    """-> (y [F][n] float32, mean [n] float64, sd [n] float64: the moments each frame was normalised with)"""
    x = np.asarray(x, np.float32)
    F, n = x.shape
    x64 = x.astype(np.float64)
    s, q = _seq_sum(x64), _seq_sum(x64 * x64)                                  # 1. frame sums, f ascending
    t = np.arange(n)
    lo, hi = np.maximum(0, t - left), np.minimum(n - 1, t + right)
    S, Q = np.zeros(n, np.float64), np.zeros(n, np.float64)
    for k in range(int((hi - lo).max()) + 1 if n else 0):                      # 2. window sums, u ascending, summed directly
        u = lo + k
        m = u <= hi
        S[m] = S[m] + s[u[m]]
        Q[m] = Q[m] + q[u[m]]
    cnt = ((hi - lo + 1) * F).astype(np.float64)                               # 3. moments
    mean = S / cnt
    var = np.maximum(Q / cnt - mean * mean, 0.0)
    sd = np.sqrt(var)
    sd = np.where(sd <= EPS, 1.0, sd)
    m32, r32 = mean.astype(np.float32), (1.0 / sd).astype(np.float32)          # 4. output: one fp32 subtract, one fp32 multiply
    y = ((x - m32[None, :]).astype(np.float32) * r32[None, :]).astype(np.float32)
    return y, mean, sd


def bound(x, mean, sd):
    """the elementwise bound of the contract's output: 2^-22 (|x| + |mean|) / sd -- four fp32 roundings (mean, 1 / sd, the
    subtract, the multiply), the first of which is made before the subtract and so counts with the whole of |mean|"""
    return 2.0 ** -22 * (np.abs(np.asarray(x, np.float64)) + np.abs(mean)[None, :]) / sd[None, :]


def reference(x, left):
    """the reference's streaming module, frame by frame -> y [F][n] float32"""
    x = np.asarray(x, np.float32)
    F, n = x.shape
    f32 = np.float32
    y = np.empty_like(x)
    sums, sqs = [], []
    sq = (x * x).astype(np.float32)            # float times float is a float product
    for t in range(n):
        # (a one-dimensional cumsum adds in order, one rounding per element: the last entry is the sequential sum)
        sums.append(f32(np.cumsum(x[:, t].astype(np.float64))[-1]))
        sqs.append(f32(np.cumsum(sq[:, t].astype(np.float64))[-1]))
        tot = f32(np.cumsum(np.asarray(sums, np.float64))[-1])
        tot2 = f32(np.cumsum(np.asarray(sqs, np.float64))[-1])
        cnt = f32(len(sums) * F)               # an int product converted for the float division
        mean = f32(tot / cnt)
        with np.errstate(invalid="ignore"):
            sd = f32(np.sqrt(f32(f32(tot2 / cnt) - f32(mean * mean))))
        if sd <= f32(1e-5):
            sd = f32(1.0)
        y[:, t] = ((x[:, t] - mean).astype(np.float32) / sd).astype(np.float32)
        if len(sums) > left:
            sums.pop(0)
            sqs.pop(0)
    return y


def cases():
    """(F, L, T, seed) of every utterance of the grid"""
    out = []
    for F in FS:
        for L in LS:
            for T in lengths(L):
                out.append((F, L, T, 7))
    return out
