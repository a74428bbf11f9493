"""Containment of w2l_gemm_f32_split on the guarded arena of tests/arena.py, by the rules (a) - (d) of tests/test_gpu_containment.py:
ragged M / N / K in the four layouts, the scalar load path (odd leading dimensions), the K split (whose slabs live in the
library's stream scratch, not in the arena) and every optional epilogue operand.  (d) is the split kernel's own bound."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_containment import CASES, _keep_factors, _stream, case, run_case
from wav2letter_amd import _lib

pytestmark = pytest.mark.gpu


def _split_case(M, N, K, akc, bkc, pad, epilogue):
    def fn(r):
        rng = np.random.default_rng(M * 1009 + N * 31 + K)
        A, B = rng.normal(size=(M, K)).astype(np.float32), rng.normal(size=(K, N)).astype(np.float32)
        bias, mask, add = (rng.normal(size=s).astype(np.float32) for s in ((N,), (M, N), (M, N)))
        As, Bs = (A if akc else A.T), (B.T if bkc else B)
        lda, ldb, ldc = As.shape[1] + pad, Bs.shape[1] + pad, N + pad
        pa, pb = r.inp("A", As, ld=lda), r.inp("B", Bs, ld=ldb)
        e = _lib.GemmEpilogue()
        if epilogue:
            e.mask, e.maskScale, e.addend = r.inp("mask", mask, ld=ldc), 0.5, r.inp("addend", add, ld=ldc)
            e.dropP, e.dropSeed, e.dropStream = 0.3, 12345, 7
        pbias = r.inp("bias", bias) if epilogue else None
        r.ok(r.L.w2l_gemm_f32_split(M, N, K, pa, lda, int(akc), pb, ldb, int(bkc), r.out("C", (M, N), ld=ldc), ldc, pbias, int(epilogue),
                                    C.byref(e), _stream()))

        def ref():
            c = A.astype(np.float64) @ B.astype(np.float64)
            bound = (2.0 ** -16 + K * 2.0 ** -23) * (np.abs(A).astype(np.float64) @ np.abs(B))
            if epilogue:
                from oracle import pyoracle
                keep = _keep_factors(pyoracle, M * ldc, 0.3, 12345, 7).reshape(M, ldc)[:, :N] * np.where(mask > 0, 0.5, 0.0)
                c = np.maximum(c + bias, 0) * keep + add
                bound = bound * keep + 4 * 2.0 ** -24 * (np.abs(c) + np.abs(add))
            return {"C": (("bound", bound), c)}
        return ref
    return fn


for _M, _N, _K, _pad in ((129, 127, 33, 0), (1, 257, 95, 4), (131, 5, 160, 1), (130, 129, 2100, 0)):
    for _akc, _bkc in ((1, 0), (1, 1), (0, 0), (0, 1)):
        for _epi in ((False,) if _K > 2048 else (False, True)):      # (the K split runs without an epilogue)
            case(f"gemm_split/{_M}x{_N}x{_K}/a{'k' if _akc else 'm'}b{'k' if _bkc else 'n'}/ld+{_pad}/{'epilogue' if _epi else 'plain'}")(
                _split_case(_M, _N, _K, _akc, _bkc, _pad, _epi))


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("gemm_split/")])
def test_split_containment(name):
    run_case(name)
