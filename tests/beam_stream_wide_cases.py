"""Inputs shared by test_beam_stream_wide_host.py and test_gpu_beam_stream_wide.py (the wide incremental CTC beam search,
w2l_beam_session_create_wide): shapes in the form of beam_stream_cases.SHAPES, built with its generators, at beams above the
narrow session's 64.  The host test proves on the CPU what each shape gives the hand-over to do."""
import functools

import numpy as np

from tests import beam_stream_cases as BC

INF = BC.INF

# name: (generator, hot, T, N, W, K, threshold, seed); the beam sizes after frames 1, 2, 3, 4 (LM-free, fp32) are beside each
SHAPES = {
    "ints_n5_w100_k4": (BC.ints, None, 24, 5, 100, 4, INF, 10),                   # 5, 17, 57, 100 ...
    "peaked_n30_w65_k8": (BC.peaked, None, 24, 30, 65, 8, INF, 11),               # 9, 65 ...
    "peaked_n30_w256_k16_thr4": (BC.peaked, None, 24, 30, 256, 16, 4.0, 12),      # 17, 75, 251, 256 ...: the line cuts at 2 and 3
    "peaked_n30_w1024_k29": (BC.peaked, None, 12, 30, 1024, 29, INF, 13),         # 30, 842, 1024 ...
}
BEAM_SIZES = {"ints_n5_w100_k4": (5, 17, 57, 100), "peaked_n30_w65_k8": (9, 65), "peaked_n30_w256_k16_thr4": (17, 75, 251, 256),
              "peaked_n30_w1024_k29": (30, 842, 1024)}


@functools.lru_cache(maxsize=None)
def utterances(shape):
    """slot 0: gen(default_rng(seed), T, N); slots 1 and 2: the next draws of 17 and 1 frames, as beam_stream_cases.utterances"""
    gen, hot, T, N, _, _, _, seed = SHAPES[shape]
    assert hot is None
    rng = np.random.default_rng(seed)
    return [gen(rng, T, N)] + [gen(rng, min(n, T), N) for n in BC.LENGTHS[1:]]
