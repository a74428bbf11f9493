"""The split-bf16 GEMM (csrc/gemm_split.hpp) on the GPU.  Every element is held to the derived bound
|C - ref| <= (2^-16 + K 2^-23) (|A| |B|)[m][n] (x - hi - lo <= 2^-18 |x| per operand, three dropped or rounded terms per product, fp32
accumulation); ref and |A| |B| are float64 products of the fp32 inputs on the CPU.  A bf16 product misses it by two orders of
magnitude.  An epilogue adds at most four fp32 roundings of the values it handles: 4 * 2^-24 of their magnitude on top."""
import pytest
import torch

from wav2letter_amd import _lib, ops

pytestmark = pytest.mark.gpu
LAYOUTS = [(1, 0), (1, 1), (0, 0), (0, 1)]


def place(x, kcontig, pad=0, off=0):   # x [i][k] as the layout asks ([i][k] or [k][i]), rows pad floats apart, off floats in
    src = x if kcontig else x.t()
    r, c = src.shape
    return torch.zeros(off + r * (c + pad), device="cuda").as_strided((r, c), (c + pad, 1), off).copy_(src)


def worst(got, A, B):   # largest error / bound over the elements; A [M][K], B [K][N] fp32 on the CPU
    ref, mag = A.double() @ B.double(), A.abs().double() @ B.abs().double()
    return ((got.double().cpu() - ref).abs() / ((2.0 ** -16 + A.shape[1] * 2.0 ** -23) * mag)).max().item()


def rand(M, N, K):
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    return torch.randn(M, K, generator=g), torch.randn(K, N, generator=g), g


@pytest.mark.parametrize("K", [32, 33, 95, 160])
@pytest.mark.parametrize("akc,bkc", LAYOUTS)
def test_layouts_edges_scalar_path_mixed_magnitudes_k_split(akc, bkc, K):
    for M in (1, 127, 129, 257):
        for N in (1, 127, 129, 257):
            A, B, _ = rand(M, N, K)
            assert worst(ops.gemm_split(place(A, akc), place(B.t(), bkc), akc, bkc), A, B) <= 1.0, (M, N)
    # odd leading dimensions, pointers one float off 16-byte alignment: the scalar load path.  Rows of A scaled by 2^+-20 and
    # columns of B by 2^-+20 inside one tile: the bound is per element, a scaling shared by a tile or a row would break it
    A, B, g = rand(129, 127, K)
    A = A * torch.exp2(20.0 * (2 * torch.randint(0, 2, (129, 1), generator=g) - 1))
    B = B * torch.exp2(-20.0 * (2 * torch.randint(0, 2, (1, 127), generator=g) - 1))
    a, b = place(A, akc, pad=1 - K % 2 if akc else 0, off=1), place(B.t(), bkc, pad=1 - K % 2 if bkc else 0, off=1)
    assert a.stride(0) % 2 == 1 and b.stride(0) % 2 == 1 and a.data_ptr() % 8 == 4
    out = torch.zeros(1 + 129 * 131, device="cuda").as_strided((129, 127), (131, 1), 1)
    assert worst(ops.gemm_split(a, b, akc, bkc, out=out), A, B) <= 1.0
    # few tiles, long reduction, no epilogue: partial slabs added in slice order; the same bits twice, there and in one launch
    for M, N, Kl in ((128, 128, 4096), (129, 130, 2500), (129, 130, 96)) if K == 160 else ():
        A, B, _ = rand(M, N, Kl)
        a, b = place(A, akc), place(B.t(), bkc)
        c1, c2 = ops.gemm_split(a, b, akc, bkc), ops.gemm_split(a, b, akc, bkc)
        assert torch.equal(c1, c2) and worst(c1, A, B) <= 1.0, (M, N, Kl)


@pytest.mark.parametrize("which", ["bias", "relu", "mask", "addend", "accumulate", "dropout", "all"])
def test_epilogue(which):
    M, N, K, p, seed, sid = 129, 130, 96, 0.25, 77, 5
    A, B, g = rand(M, N, K)
    bias, mask, add = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    on = lambda name: which in (name, "all")
    x, w, y = place(A, 1), place(B.t(), 0), torch.empty(M, N, device="cuda")
    # the library's own dropout mask: what the fp32 route keeps under the same seed, element by element
    _lib.check(_lib.lib().w2l_linear_forward_dropout(M, K, N, x.data_ptr(), w.data_ptr(), None, y.data_ptr(), 0, p, seed, sid,
                                                     torch.cuda.current_stream().cuda_stream), "fp32 dropout")
    keep, joined = (y != 0).cpu(), on("addend") or on("accumulate")
    got = ops.gemm_split(x, w, 1, 0, bias=bias.cuda() if on("bias") else None, relu=on("relu"), mask=mask.cuda() if on("mask") else None,
                         mask_scale=1.5, addend=add.cuda() if on("addend") else None, out=add.cuda() if which == "accumulate" else None,
                         accumulate=on("accumulate"), drop_p=p if on("dropout") else 0.0, drop_seed=seed, drop_stream=sid).cpu()
    ref = A.double() @ B.double() + (bias.double() if on("bias") else 0)
    ref = ref.clamp_min(0) if on("relu") else ref
    scale = (keep / (1 - p) if on("dropout") else 1.0) * ((mask > 0) * 1.5 if on("mask") else 1.0) * torch.ones(M, N, dtype=torch.float64)
    if which == "dropout":
        assert torch.equal(got != 0, keep)          # the kept / dropped pattern is the fp32 route's
    ref = ref * scale + (add.double() if joined else 0)
    bound = (2.0 ** -16 + K * 2.0 ** -23) * (A.abs().double() @ B.abs().double()) * scale + 4 * 2.0 ** -24 * (ref.abs() + add.abs() * joined)
    assert ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item() <= 1.0


def test_switch_routes_the_linear_products():
    L, s, g, (M, nin, nout) = _lib.lib(), torch.cuda.current_stream().cuda_stream, torch.Generator().manual_seed(3), (130, 96, 160)
    x, w, dy, b = (torch.randn(*sh, generator=g).cuda() for sh in ((M, nin), (nin, nout), (M, nout), (nout,)))

    def three():
        y, dx, dw, db = torch.empty(M, nout).cuda(), torch.empty(M, nin).cuda(), torch.empty(nin, nout).cuda(), torch.empty(nout).cuda()
        _lib.check(L.w2l_linear_forward(M, nin, nout, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), 1, s), "forward")
        _lib.check(L.w2l_linear_backward_data(M, nin, nout, dy.data_ptr(), w.data_ptr(), dx.data_ptr(), 0, None, 1.0, s), "dx")
        _lib.check(L.w2l_linear_backward_weight_bias(M, nin, nout, x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), s), "dw")
        return y, dx, dw, db

    same = lambda p, q: all(torch.equal(a, c) for a, c in zip(p, q))
    direct = (ops.gemm_split(x, w, 1, 0, bias=b, relu=True), ops.gemm_split(dy, w, 1, 1), ops.gemm_split(x, dy, 0, 0))
    f32 = three()
    assert L.w2l_set_matmul_split(1) == 0
    try:
        split = three()
        assert same(split[:3], direct) and not same(split[:3], f32[:3])
        assert (split[3].double() - dy.double().sum(0)).abs().max().item() < 1e-4 * dy.abs().sum(0).max().item()
        assert L.w2l_set_matmul_precision(1) == 0          # the mixed-precision mode takes precedence
        both = three()
        L.w2l_set_matmul_split(0)
        assert same(both, three()) and not same(both[:3], split[:3])
    finally:
        L.w2l_set_matmul_precision(0), L.w2l_set_matmul_split(0)
    assert same(three(), f32)
    with pytest.raises(_lib.W2LError, match="UNSUPPORTED"):
        ops.gemm_split(x[:, :31], dy[:, :31], 1, 1)        # K = 31
