"""numpy restatement of w2l_ctc_align's contract (include/w2l_hip.h), shared by test_ctc_align_host.py and test_gpu_ctc_align.py.

The recursion runs on the RAW fp32 emissions: per frame and lattice position two compares and ONE fp32 add, candidates in the order
stay, advance, skip, a later one winning only when strictly greater.  Every operation below is an fp32 compare or a single fp32
add, so the GPU kernel must reproduce the path bit for bit, ties included."""
import numpy as np


def ctc_target_size(target, T):
    """w2l_batch_ctc_target_size: labels up to the first negative one, cut so that labels + adjacent repeats fit T frames"""
    out = []
    for y in np.asarray(target):
        neg = np.nonzero(y < 0)[0]
        n = int(neg[0]) if len(neg) else len(y)
        R = int((y[1:n] == y[:max(n - 1, 0)]).sum())
        out.append(max(min(n + R, T) - R, 0))
    return np.array(out, np.int32)


def align_one(x, y, F):
    """x [T][N] float32, y the L_b labels, F frames of the utterance -> (path [T] int32, end score float32 or -inf).
    Infeasible (L_b + R > F): path -1 everywhere."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.int64)
    T, N = x.shape
    blank, Lb = N - 1, len(y)
    S = 2 * Lb + 1
    R = int((y[1:] == y[:-1]).sum())
    if Lb + R > F:
        return np.full(T, -1, np.int32), -np.inf
    ext = np.full(S, blank, np.int64)
    ext[1::2] = y
    skip = np.zeros(S, bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    ninf = np.float32(-np.inf)
    a = np.full(S, ninf, np.float32)
    a[0] = x[0, blank]
    if S > 1:
        a[1] = x[0, ext[1]]
    bp = np.zeros((F, S), np.int8)
    for t in range(1, F):
        best = a.copy()                                   # stay
        adv = np.concatenate(([ninf], a[:-1]))
        m = adv > best
        best[m], bp[t][m] = adv[m], 1
        sk = np.concatenate(([ninf, ninf], a[:-2]))[:S]
        m = skip & (sk > best)
        best[m], bp[t][m] = sk[m], 2
        a = best + x[t, ext]                              # float32 + float32: one fp32 add
        assert a.dtype == np.float32
    s = S - 1
    if S >= 2 and a[S - 2] > a[S - 1]:
        s = S - 2
    end = a[s]
    path = np.full(T, blank, np.int32)
    for t in range(F - 1, -1, -1):
        path[t] = ext[s]
        s -= int(bp[t][s])
    return path, end


def path_logprob(x, path, F):
    """float64 log_softmax of x summed over the first F frames of path"""
    x64 = np.asarray(x[:F], np.float64)
    m = x64.max(axis=1)
    lse = m + np.log(np.exp(x64 - m[:, None]).sum(axis=1))
    return float((x64[np.arange(F), path[:F]] - lse).sum())


def ctc_align_ref(x, target, frames=None):
    """x [B][T][N] float32, target [B][L] (negative = padding), frames [B] or None -> (path [B][T] int32, score [B] float64)"""
    x = np.asarray(x, np.float32)
    B, T, _ = x.shape
    ts = ctc_target_size(target, T)
    paths = np.empty((B, T), np.int32)
    score = np.empty(B, np.float64)
    for b in range(B):
        F = T if frames is None else int(frames[b])
        paths[b], _ = align_one(x[b], np.asarray(target)[b][:ts[b]], F)
        score[b] = -np.inf if paths[b][0] < 0 else path_logprob(x[b], paths[b], F)
    return paths, score


def collapse(path, blank):
    """CTC collapse: merge repeats, drop blanks"""
    out, prev = [], None
    for p in path:
        if p != prev and p != blank:
            out.append(int(p))
        prev = p
    return out
