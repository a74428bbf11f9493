"""Which frames the CPC criterion masks and which negatives every masked frame is scored against: the Python twin of
include/fl_compat/cpc.h (the same splitmix64 stream consumed in the same order, so both give the same draws for a seed;
tests/test_cpc_host.py compares them bit for bit).  The rules and the reference's lines are in that header.  Host logic only."""
import math

import numpy as np

_M64 = (1 << 64) - 1


class CpcRng:
    def __init__(self, seed):
        self.state = int(seed) & _M64

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & _M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)


def mark_span(row, s, mask_length, n):
    """start s marks s, s+1, s-1, s+2, s-2, ... (mask_length frames) clipped to [0, n)"""
    for i in range(mask_length):
        d = (i + 1) // 2
        t = s + d if i & 1 else s - d
        if 0 <= t < n:
            row[t] = 1


def negatives(rng, B, M, n_negative):
    """neg [B][M][K] int32, K = min(n_negative, M): positions of the masked list that are neither m nor a list neighbour"""
    if M < 4:
        raise ValueError(f"CPC: negative sampling needs M >= 4 masked frames per utterance, got M = {M}")
    if n_negative < 1:
        raise ValueError("CPC: nNegative must be positive")
    K = min(n_negative, M)
    neg = np.empty((B, M, K), np.int32)
    for b in range(B):
        for m in range(M):
            lo, hi = min(M, m + 2), max(M, M - 1 + m)
            for k in range(K):
                neg[b, m, k] = (lo + rng.next() % (hi - lo)) % M
    return neg


def sample(B, T, mask_prob, mask_length, n_negative, frames=None, seed=0):
    """(mask [B][T] uint8, mask_index [B][M] int32 ascending per row, neg [B][M][K] int32)"""
    if B < 1 or T < 1:
        raise ValueError("CPC: B and T must be positive")
    if not mask_prob >= 0.0 or mask_length < 1:
        raise ValueError("CPC: maskProb must not be negative and maskLength must be positive")
    rng = CpcRng(seed)
    num_mask = math.floor(float(mask_prob) * float(T))
    marked = np.zeros((B, T), np.uint8)
    for b in range(B):
        n = T if frames is None else int(frames[b])
        if n < 1 or n > T:
            raise ValueError(f"CPC: frames[{b}] = {n} is outside 1 .. T")
        for _ in range(num_mask):
            mark_span(marked[b], rng.next() % n, mask_length, n)
    lists = [[int(t) for t in np.flatnonzero(marked[b])] for b in range(B)]
    M = min(len(v) for v in lists)
    if M < 4:
        raise ValueError(f"CPC: negative sampling needs M >= 4 masked frames per utterance, got M = {M}")
    mask = np.zeros((B, T), np.uint8)
    index = np.empty((B, M), np.int32)
    for b, v in enumerate(lists):
        for i in range(len(v) - 1, 0, -1):
            j = rng.next() % (i + 1)
            v[i], v[j] = v[j], v[i]
        index[b] = sorted(v[:M])
        mask[b, index[b]] = 1
    return mask, index, negatives(rng, B, M, n_negative)
