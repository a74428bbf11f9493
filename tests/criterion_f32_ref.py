"""A yardstick for what one number format can hold: the sequence criteria as per-frame-renormalised log-domain forward-backward
recursions in plain numpy, every intermediate (the running log Z included) kept in the `dtype` given.  float64 restates the C oracle
(oracle/criterion_oracle.c) and is pinned to it at 1e-10 by tests/test_criterion_f32_ref_host.py; float32 is
the same code and shows how far a careful fp32 evaluation sits from the fp64 answer, which is what the device kernels' bars are set against.

Renormalised: after every frame the log-alphas are shifted so that their logsumexp is 0 and the shift goes into a running sum (log Z).
The alphas that the backward pass exponentiates therefore stay O(1) in magnitude however long the utterance, and the rounding of a
frame does not grow with the size of the accumulated score.  Gradients are posteriors: softmaxes of shift-invariant sums, so the
shifts never enter them.

Layout as in the oracle: emissions [B][T][N], transitions [N][N] indexed [to][from], targets [B][L] int32 padded with negatives,
CTC blank = N - 1.  Every function returns float64 arrays holding the values computed in `dtype`."""
import numpy as np


def scale_factor(mode, T, L):
    """CriterionUtils scale modes (oracle: scale_of): none, 1/T, 1/sqrt(T), 1/L, 1/sqrt(L)"""
    if mode == 1:
        return 1.0 / T if T > 0 else 1.0
    if mode == 2:
        return np.sqrt(1.0 / T) if T > 0 else 1.0
    if mode == 3:
        return 1.0 / L if L > 0 else 1.0
    if mode == 4:
        return np.sqrt(1.0 / L) if L > 0 else 1.0
    return 1.0


def target_size(row, max_size):
    n = 0
    while n < len(row) and row[n] >= 0:
        n += 1
    return min(n, max_size)


def ctc_target_size(row, T):
    n = target_size(row, len(row))
    R = int(sum(row[i] == row[i - 1] for i in range(1, n)))
    return max(min(n + R, T) - R, 0)


def _lse(v):
    m = v.max()
    if not np.isfinite(m):
        return m
    return m + np.log(np.exp(v - m).sum(dtype=v.dtype))


def _weights(grad, B):
    return np.ones(B) if grad is None else np.asarray(grad, np.float64)


def fcc(x, trans, target_size, scale_mode=0, grad=None, dtype=np.float64):
    """FullConnectionCriterion: log of the summed score of every label path.  -> loss [B], dx [B][T][N], dA [N][N]"""
    dt = np.dtype(dtype).type
    x = np.asarray(x, np.float32).astype(dt)
    A = np.asarray(trans, np.float32).astype(dt)
    B, T, N = x.shape
    w = _weights(grad, B)
    loss = np.zeros(B)
    dx = np.zeros((B, T, N), dt)
    dA = np.zeros((N, N), dt)
    for b in range(B):
        s = scale_factor(scale_mode, T, int(target_size[b]))
        g = dt(s * w[b])
        la = np.empty((T, N), dt)          # normalised log alpha: logsumexp of every row is 0
        c = _lse(x[b, 0])
        la[0] = x[b, 0] - c
        logz = dt(c)
        for t in range(1, T):
            M = la[t - 1][None, :] + A     # [to][from]
            m = M.max(axis=1)
            new = x[b, t] + m + np.log(np.exp(M - m[:, None]).sum(axis=1, dtype=dt))
            c = _lse(new)
            la[t] = new - c
            logz = dt(logz + c)
        logz = dt(logz + _lse(la[T - 1]))
        loss[b] = float(dt(dt(s) * logz))
        lb = np.zeros(N, dt)               # normalised log beta: the paths after frame t, the emission of frame t not included
        part = np.zeros((N, N), dt)         # dA in partial sums of 64 frames: an entry that grows to hundreds is not rounded at every frame
        for t in range(T - 1, -1, -1):
            q = la[t] + lb
            e = np.exp(q - q.max())
            dx[b, t] = g * (e / e.sum(dtype=dt))
            if t == 0 or t % 64 == 0:
                dA += part
                part[:] = 0
            if t == 0:
                break
            v = x[b, t] + lb                # what entering label `to` at frame t is worth from there on
            M = la[t - 1][None, :] + A + v[:, None]
            E = np.exp(M - M.max())
            part += g * (E / E.sum(dtype=dt))   # posterior of the pair (to, from) at frame t
            Mb = A + v[:, None]
            m = Mb.max(axis=0)
            lb = m + np.log(np.exp(Mb - m[None, :]).sum(axis=0, dtype=dt))
            lb = lb - _lse(lb)
    return loss, dx.astype(np.float64), dA.astype(np.float64)


def fac(x, trans, target, scale_mode=0, grad=None, dtype=np.float64):
    """ForceAlignmentCriterion: log of the summed score of the paths that spell the target, every position at least one frame,
    a repeated label being a position like any other (transition y[i] -> y[i]).  -> loss [B], dx [B][T][N], dA [N][N]"""
    dt = np.dtype(dtype).type
    x = np.asarray(x, np.float32).astype(dt)
    A = np.asarray(trans, np.float32).astype(dt)
    target = np.asarray(target, np.int32)
    B, T, N = x.shape
    w = _weights(grad, B)
    ninf = dt(-np.inf)
    loss = np.zeros(B)
    dx = np.zeros((B, T, N), dt)
    dA = np.zeros((N, N), dt)
    for b in range(B):
        S = target_size(target[b], T)
        if S <= 0:
            continue
        y = target[b, :S].astype(np.int64)
        s = scale_factor(scale_mode, T, S)
        g = dt(s * w[b])
        stay = A[y, y]
        move = np.full(S, ninf)
        move[1:] = A[y[1:], y[:-1]]
        pos = np.arange(S)
        la = np.full((T, S), ninf)
        la[0, 0] = 0
        logz = dt(x[b, 0, y[0]])

        def arcs(prev):
            s1 = prev + stay
            s2 = np.full(S, ninf)
            s2[1:] = prev[:-1] + move[1:]
            return s1, s2
        for t in range(1, T):
            s1, s2 = arcs(la[t - 1])
            new = np.logaddexp(s1, s2) + x[b, t, y]
            new[pos < S - (T - t)] = ninf      # too late to reach the last position by the last frame
            c = _lse(new)
            la[t] = new - c
            logz = dt(logz + c)
        loss[b] = float(dt(dt(s) * dt(logz + la[T - 1, S - 1])))
        lb = np.full(S, ninf)               # normalised log beta, the emission of frame t not included
        lb[S - 1] = 0
        part = np.zeros((N, N), dt)         # dA in partial sums of 64 frames, as in fcc()
        for t in range(T - 1, -1, -1):
            q = la[t] + lb
            q = np.where(np.isfinite(q), q, ninf)
            e = np.exp(q - q.max())
            np.add.at(dx[b, t], y, g * (e / e.sum(dtype=dt)))
            if t % 64 == 0:
                dA += part
                part[:] = 0
            if t == 0:
                break
            v = x[b, t, y] + lb
            a1 = la[t - 1] + stay + v          # arc i -> i into frame t
            a2 = np.full(S, ninf)
            a2[1:] = la[t - 1][:-1] + move[1:] + v[1:]   # arc i-1 -> i
            a1 = np.where(np.isfinite(a1), a1, ninf)
            a2 = np.where(np.isfinite(a2), a2, ninf)
            m = max(a1.max(), a2.max())
            e1, e2 = np.exp(a1 - m), np.exp(a2 - m)
            z = dt(e1.sum(dtype=dt) + e2.sum(dtype=dt))
            np.add.at(part, (y, y), g * (e1 / z))
            np.add.at(part, (y[1:], y[:-1]), g * (e2[1:] / z))
            nb = stay + v
            nb[:-1] = np.logaddexp(nb[:-1], move[1:] + v[1:])
            c = _lse(np.where(np.isfinite(la[t - 1]), nb, ninf))
            lb = nb - c
    return loss, dx.astype(np.float64), dA.astype(np.float64)


def asg(x, trans, target, scale_mode=0, grad=None, dtype=np.float64):
    """ASG = FCC - FAC on the same transitions, composed from the two"""
    x = np.asarray(x, np.float32)
    ts = [target_size(r, x.shape[1]) for r in np.asarray(target)]
    l1, dx1, dA1 = fcc(x, trans, ts, scale_mode, grad, dtype)
    l2, dx2, dA2 = fac(x, trans, target, scale_mode, grad, dtype)
    dt = np.dtype(dtype).type
    sub = lambda p, q: (p.astype(dt) - q.astype(dt)).astype(np.float64)
    return sub(l1, l2), sub(dx1, dx2), sub(dA1, dA2)


def ctc(x, target, target_size=None, scale_mode=0, grad=None, dtype=np.float64):
    """CTC on the log-softmax of every row, blank = N - 1.  -> loss [B] (+inf where no path exists), dx [B][T][N].
    The occupancy of a frame is the softmax over lattice states of alpha + beta - emission: every path passes through exactly one
    state per frame, so the states' posteriors sum to one and log Z never has to be subtracted from a sum of two running scores."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, np.float32).astype(dt)
    target = np.asarray(target, np.int32)
    B, T, N = x.shape
    w = _weights(grad, B)
    ninf = dt(-np.inf)
    blank = N - 1
    loss = np.zeros(B)
    dx = np.zeros((B, T, N), dt)
    for b in range(B):
        Lb = ctc_target_size(target[b], T) if target_size is None else int(target_size[b])
        S = 2 * Lb + 1
        s = scale_factor(scale_mode, T, Lb)
        g = dt(s * w[b])
        m = x[b].max(axis=1, keepdims=True)
        lp = x[b] - (m + np.log(np.exp(x[b] - m).sum(axis=1, keepdims=True, dtype=dt)))
        ext = np.full(S, blank, np.int64)
        ext[1::2] = target[b, :Lb]
        skip = np.zeros(S, bool)
        skip[2:] = (np.arange(2, S) & 1).astype(bool) & (ext[2:] != ext[:-2])
        em = lp[:, ext]                       # [T][S]

        def step(prev, skip_in):
            v = prev.copy()
            v[1:] = np.logaddexp(v[1:], prev[:-1])
            far = np.full(S, ninf)
            far[2:] = prev[:-2]
            return np.where(skip_in, np.logaddexp(v, far), v)
        la = np.full((T, S), ninf)
        la[0, :2] = em[0, :2]
        c = _lse(la[0])
        la[0] -= c
        logz = dt(c)
        feasible = True
        for t in range(1, T):
            new = step(la[t - 1], skip) + em[t]
            c = _lse(new)
            if not np.isfinite(c):
                feasible = False
                break
            la[t] = new - c
            logz = dt(logz + c)
        if feasible:
            tail = _lse(la[T - 1, max(S - 2, 0):])
            feasible = bool(np.isfinite(tail))
        sm = np.exp(lp)
        if not feasible:
            loss[b] = np.inf
            dx[b] = g * sm                     # no path: occupancy 0, as the oracle
            continue
        loss[b] = float(dt(-dt(s) * dt(logz + tail)))
        skip_b = np.zeros(S, bool)             # the lattice read from its end (state S-1-k): s may be left for s+2
        skip_b[:-2] = (np.arange(S - 2) & 1).astype(bool) & (ext[:-2] != ext[2:])
        skip_b = skip_b[::-1]
        lb = np.full(S, ninf)
        lb[max(S - 2, 0):] = em[T - 1, max(S - 2, 0):]
        for t in range(T - 1, -1, -1):
            if t < T - 1:
                lb = (step(lb[::-1], skip_b) + em[t, ::-1])[::-1]
            lb = lb - _lse(np.where(np.isfinite(la[t]), lb, ninf))
            q = la[t] + lb - em[t]
            q = np.where(np.isfinite(q), q, ninf)
            e = np.exp(q - q.max())
            occ = np.zeros(N, dt)
            np.add.at(occ, ext, e / e.sum(dtype=dt))
            dx[b, t] = g * (sm[t] - occ)
    return loss, dx.astype(np.float64)
