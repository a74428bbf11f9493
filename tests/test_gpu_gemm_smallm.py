"""GPU tests of w2l_gemm_bf16_smallm (csrc/gemm_smallm.hip): C[M][N] = A[M][K] . B[N][K]^T on bf16 operand images, fp32 accumulation.

Operands are random normals rounded to bf16 on the host, in images laid out as w2l_bf16_convert lays them out (leading dimension
K rounded up to 64, zero-filled).  The reference is the float64 product of the same rounded operands, so the only error left is
the fp32 accumulation: |got - ref| <= (K + 2) 2^-24 (sum_k |a||b| + |bias| + |addend|) for ANY summation order (K - 1 additions,
the bias and the addend, each with relative error 2^-24; the bound of tests/test_gpu_conv_bf16.py carried over).

The cases cover M in {1, 31, 32, 33, 144, cap}, N in {1, 5, 40, 1200} and K in {8, 200, 2160, 6480}: one to four row tiles per
wave, one to eight waves, a last slab of 1, 5, 8 and 16 weight rows.  The kernel does not split K (an element is one MFMA chain,
the chain of w2l_gemm_bf16), so there is no split threshold to straddle; G6 pins that the two kernels agree bit for bit where
w2l_gemm_bf16 does not split K either."""
import ctypes as C

import numpy as np
import pytest
import torch

from wav2letter_amd import _lib

pytestmark = pytest.mark.gpu

CAP = 1024
CASES = [(1, 1, 8), (31, 5, 200), (32, 40, 2160), (33, 1200, 200), (144, 1200, 2160), (CAP, 40, 6480), (144, 5, 6480)]
BASE = (144, 1200, 2160)   # the row-independence, determinism, image and cross-kernel checks


class Sink(C.Structure):
    _fields_ = [("rowMajor", C.c_void_p), ("ldRows", C.c_size_t), ("transposed", C.c_void_p), ("ldTrans", C.c_size_t)]


def pad64(n):
    return (n + 63) // 64 * 64


def to_bf16(x):
    """float32 -> bf16 bits, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def image(h, ld):
    """bf16 bits [rows][cols] -> zero-padded image [rows][ld] on the device (as int16: the bits are what matters)"""
    out = np.zeros((h.shape[0], ld), np.uint16)
    out[:, :h.shape[1]] = h
    return torch.from_numpy(out.view(np.int16)).cuda()


_cache = {}


def operands(M, N, K):
    """rounded operands, their images, bias / addend and the float64 reference pieces: computed once per shape, never changed"""
    key = (M, N, K)
    if key not in _cache:
        rng = np.random.default_rng(M * 7919 + N * 104729 + K)
        ah, bh = to_bf16(rng.normal(size=(M, K)).astype(np.float32)), to_bf16(rng.normal(size=(N, K)).astype(np.float32))
        a, b = from_bf16(ah).astype(np.float64), from_bf16(bh).astype(np.float64)
        bias, add = rng.normal(size=N).astype(np.float32), rng.normal(size=(M, N)).astype(np.float32)
        _cache[key] = dict(ah=ah, bh=bh, A=image(ah, pad64(K)), B=image(bh, pad64(K)), bias=bias, add=add, prod=a @ b.T,
                           mag=np.abs(a) @ np.abs(b).T, bias_d=torch.from_numpy(bias).cuda(), add_d=torch.from_numpy(add).cuda())
    return _cache[key]


def workspace(M, N, K):
    n = _lib.lib().w2l_gemm_bf16_smallm_workspace_bytes(M, N, K)
    return torch.empty(max(n, 256), dtype=torch.uint8, device="cuda"), n


def smallm(M, N, K, A, B, bias=None, relu=0, add=None, want_c=True, img=None, ld_img=0):
    """one call; returns C [M][N] (or None).  A, B: device images with leading dimension pad64(K)"""
    ws, nws = workspace(M, N, K)
    c = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda") if want_c else None
    sink = Sink(img.data_ptr(), ld_img, None, 0) if img is not None else None
    st = _lib.lib().w2l_gemm_bf16_smallm(M, N, K, A.data_ptr(), pad64(K), B.data_ptr(), pad64(K), c.data_ptr() if want_c else None, N,
                                         bias.data_ptr() if bias is not None else None, relu, add.data_ptr() if add is not None else None,
                                         C.byref(sink) if sink else None, ws.data_ptr(), nws, torch.cuda.current_stream().cuda_stream)
    assert st == 0, (st, _lib.lib().w2l_last_hip_error())
    torch.cuda.synchronize()
    return c


def test_cap_is_the_one_the_cases_use():
    assert _lib.lib().w2l_gemm_bf16_smallm_max_m() == CAP


@pytest.mark.parametrize("M,N,K", CASES)
def test_g1_accuracy(M, N, K):
    o = operands(M, N, K)
    eps = (K + 2) * 2.0 ** -24
    worst = 0.0
    for bias, relu, add in ((False, 0, False), (True, 0, False), (True, 1, False), (False, 0, True), (True, 1, True)):
        got = smallm(M, N, K, o["A"], o["B"], o["bias_d"] if bias else None, relu, o["add_d"] if add else None).cpu().numpy().astype(np.float64)
        ref = o["prod"] + (o["bias"] if bias else 0.0)
        if relu:
            ref = np.maximum(ref, 0.0)
        if add:
            ref = ref + o["add"]
        bound = eps * (o["mag"] + (np.abs(o["bias"]) if bias else 0.0) + (np.abs(o["add"]) if add else 0.0))
        assert np.isfinite(got).all()
        ratio = float((np.abs(got - ref) / bound).max())
        print(f"M={M} N={N} K={K} bias={bias} relu={relu} addend={add}: max err / bound = {ratio:.4f}")
        worst = max(worst, ratio)
        assert ratio <= 1.0, (M, N, K, bias, relu, add, ratio)
    print(f"M={M} N={N} K={K}: largest error-to-bound ratio {worst:.4f}")


@pytest.mark.parametrize("poison", [False, True])
def test_g2_rows_are_bitwise_independent(poison):
    """row r of the result is a function of row r of A and of B alone: the M = 144 result against M = 1 calls on rows 0, 77, 143 and
    an M = 33 call on rows 100 .. 132 -- and again with every OTHER row of A set to NaN"""
    M, N, K = BASE
    o = operands(M, N, K)
    ld = pad64(K)
    keep = [0, 77, 143] + list(range(100, 133))
    A = o["A"]
    if poison:
        a = o["A"].cpu().numpy().view(np.uint16).copy()
        mask = np.ones(M, bool)
        mask[keep] = False
        a[mask, :K] = 0x7FC0   # bf16 NaN
        A = torch.from_numpy(a.view(np.int16)).cuda()
    full = smallm(M, N, K, A, o["B"], o["bias_d"], 0, o["add_d"]).cpu().numpy()
    clean = smallm(M, N, K, o["A"], o["B"], o["bias_d"], 0, o["add_d"]).cpu().numpy()
    assert np.isfinite(full[keep]).all()
    assert np.array_equal(full[keep], clean[keep])
    if poison:
        assert np.isnan(full[1]).any()   # the poison did reach the kernel
    for r in (0, 77, 143):
        one = smallm(1, N, K, A[r:r + 1].contiguous(), o["B"], o["bias_d"], 0, o["add_d"][r:r + 1].contiguous()).cpu().numpy()
        assert np.array_equal(one[0], full[r]), r
    some = smallm(33, N, K, A[100:133].contiguous(), o["B"], o["bias_d"], 0, o["add_d"][100:133].contiguous()).cpu().numpy()
    assert np.array_equal(some, full[100:133])
    assert A.shape[1] == ld


def test_g3_two_calls_are_bit_identical():
    for M, N, K in (BASE, (CAP, 40, 6480)):
        o = operands(M, N, K)
        a = smallm(M, N, K, o["A"], o["B"], o["bias_d"], 0, o["add_d"])
        b = smallm(M, N, K, o["A"], o["B"], o["bias_d"], 0, o["add_d"])
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,N,K", [BASE, (33, 40, 200), (31, 5, 200)])
def test_g4_image_epilogue(M, N, K):
    """the row image beside C equals w2l_bf16_convert of C bit for bit, only elements of the matrix are written (the padding keeps
    its sentinel), and the image of a call without C equals it"""
    o = operands(M, N, K)
    ld = pad64(N)
    sentinel = 0x1234
    img = torch.full((M, ld), sentinel, dtype=torch.int16, device="cuda")
    c = smallm(M, N, K, o["A"], o["B"], o["bias_d"], 1, None, True, img, ld)
    want = torch.zeros((M, ld), dtype=torch.int16, device="cuda")
    st = _lib.lib().w2l_bf16_convert(c.data_ptr(), M, N, N, want.data_ptr(), ld, None, 0, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(img[:, :N], want[:, :N])
    assert (img[:, N:] == sentinel).all()
    assert (c > 0).any() and (c == 0).any()   # the ReLU is in what the image holds
    alone = torch.full((M, ld), sentinel, dtype=torch.int16, device="cuda")
    assert smallm(M, N, K, o["A"], o["B"], o["bias_d"], 1, None, False, alone, ld) is None
    assert torch.equal(alone, img)


@pytest.mark.parametrize("M,N,K", [BASE, (CAP, 40, 6480), (33, 1200, 200)])
def test_g5_against_gemm_bf16(M, N, K):
    """both kernels are inside G1's bound on the same operands, so they are within twice that bound of each other"""
    o = operands(M, N, K)
    got = smallm(M, N, K, o["A"], o["B"], o["bias_d"]).cpu().numpy().astype(np.float64)
    c = torch.empty((M, N), dtype=torch.float32, device="cuda")
    st = _lib.lib().w2l_gemm_bf16(M, N, K, o["A"].data_ptr(), pad64(K), o["B"].data_ptr(), pad64(K), c.data_ptr(), N, o["bias_d"].data_ptr(), 0,
                                  None, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    other = c.cpu().numpy().astype(np.float64)
    bound = (K + 2) * 2.0 ** -24 * (o["mag"] + np.abs(o["bias"]))
    ref = o["prod"] + o["bias"]
    r1, r2 = float((np.abs(got - ref) / bound).max()), float((np.abs(other - ref) / bound).max())
    r12 = float((np.abs(got - other) / (2 * bound)).max())
    print(f"M={M} N={N} K={K}: smallm err / bound {r1:.4f}, gemm_bf16 err / bound {r2:.4f}, difference / (2 bound) {r12:.4f}")
    assert r1 <= 1.0 and r2 <= 1.0 and r12 <= 1.0


@pytest.mark.parametrize("M,N,K", [BASE, (33, 1200, 200), (32, 40, 2160), (31, 5, 200)])
def test_g6_the_bits_of_gemm_bf16(M, N, K):
    """below K = 4096 w2l_gemm_bf16 adds an element up in one MFMA chain over ascending k, and so does this kernel: the same bits,
    with bias, ReLU and addend.  A mixed-precision session rests on this: with any other summation order its bf16 roundings part
    from the trainer's and the difference grows from block to block (tests/test_gpu_stream_bf16.py, the whole recipe arch)"""
    o = operands(M, N, K)

    class Epi(C.Structure):
        _fields_ = [("mask", C.c_void_p), ("maskScale", C.c_float), ("addend", C.c_void_p), ("accumulate", C.c_int), ("dropP", C.c_double),
                    ("dropSeed", C.c_uint32), ("dropStream", C.c_uint32)]

    for relu, add in ((0, False), (1, False), (0, True)):
        got = smallm(M, N, K, o["A"], o["B"], o["bias_d"], relu, o["add_d"] if add else None)
        c = torch.empty((M, N), dtype=torch.float32, device="cuda")
        e = Epi(None, 1.0, o["add_d"].data_ptr() if add else None, 0, 0.0, 0, 0)
        st = _lib.lib().w2l_gemm_bf16(M, N, K, o["A"].data_ptr(), pad64(K), o["B"].data_ptr(), pad64(K), c.data_ptr(), N, o["bias_d"].data_ptr(),
                                      relu, C.byref(e) if add else None, torch.cuda.current_stream().cuda_stream)
        assert st == 0
        torch.cuda.synchronize()
        assert torch.equal(got, c), (M, N, K, relu, add, float((got - c).abs().max()))
