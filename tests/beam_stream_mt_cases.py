"""Inputs shared by test_beam_stream_mt_host.py, test_gpu_beam_stream_mt.py and test_gpu_beam_stream_mt_containment.py (the
many-token incremental CTC beam search, w2l_beam_session_create_mt): shapes in the form of beam_stream_cases.SHAPES, built with its
generators, at token counts above the other sessions' 64 and at a beam above the wide family's 1024.  The host test proves on the
CPU, with beam_mt_ref.mt_beam_one's counts, what each shape gives the hand-over to do."""
import functools

import numpy as np

from tests import beam_stream_cases as BC

INF = BC.INF

# name: (generator, hot, T, N, W, K, threshold, seed)
SHAPES = {
    "peaked_n130_w200_k129": (BC.peaked, None, 12, 130, 200, 129, INF, 20),          # three mask words (the third: k = 128 alone)
    "peaked_n70_w65_k65": (BC.peaked, None, 12, 70, 65, 65, INF, 26),                # the first K the other sessions refuse
    "peaked_n260_w300_k256_thr4": (BC.peaked, None, 8, 260, 300, 256, 4.0, 22),      # four mask words, the threshold line cuts
    "peaked_n110_w1500_k100": (BC.peaked, None, 8, 110, 1500, 100, INF, 23),         # a beam above the wide family's
    "peaked_n30_w256_k16": (BC.peaked, None, 24, 30, 256, 16, INF, 24),              # the wide session's domain
}
MANY = tuple(s for s in SHAPES if SHAPES[s][5] > 64)      # the shapes no other creator accepts


@functools.lru_cache(maxsize=None)
def utterances(shape):
    """slot 0: gen(default_rng(seed), T, N); slots 1 and 2: the next draws of 17 and 1 frames (clipped to T), as
    beam_stream_cases.utterances"""
    gen, hot, T, N, _, _, _, seed = SHAPES[shape]
    assert hot is None
    rng = np.random.default_rng(seed)
    return [gen(rng, T, N)] + [gen(rng, min(n, T), N) for n in BC.LENGTHS[1:]]
