"""w2l_residual_join_forward / w2l_residual_join_backward, the join of a residual block, bit for bit against numpy
fp32 (tests/residual_ref.py): y = np.float32(s) * (a + b) -- one add, one multiply -- then the positive part; g = np.float32(s) * dy,
then 0 where y <= 0.  Every element count on both sides of the float4 body and of one workgroup's trip, every phase of each of the
three pointers against 16 bytes on its own (the vector body needs all three to agree; the element-wise path takes the rest), the
three aliases the contract allows, exact zeros and sign changes in the inputs, and the refusals."""
import numpy as np
import pytest
import torch

import residual_ref as R
from wav2letter_amd import _lib

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = [1, 3, 4, 63, 64, 65, 1027, (1 << 20) + 5]
SCALES = [1.0, 0.70711, -0.5, 0.0]
SENTINEL = F32(-7.25)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _values(rng, n):
    """normal values with exact zeros, exact cancellations (a == -b) and both signs of zero among them"""
    a = rng.normal(size=n).astype(F32)
    b = rng.normal(size=n).astype(F32)
    k = rng.integers(0, 6, size=n)
    a[k == 0] = 0
    b[k == 1] = 0
    b[k == 2] = -a[k == 2]
    a[k == 3] = -0.0
    return a, b


def _padded(x, off):
    buf = np.full(x.size + 3, SENTINEL, F32)
    buf[off:off + x.size] = x
    return torch.from_numpy(buf).cuda()


def _inside(t, off, n):
    return t[off:off + n].cpu().numpy()


def _outside_untouched(t, off, n):
    h = t.cpu().numpy()
    rest = np.concatenate([h[:off], h[off + n:]])
    return (rest.view(np.int32) == SENTINEL.view(np.int32)).all()


def _same_bits(got, want):
    return np.array_equal(got.view(np.int32), want.view(np.int32))


@pytest.fixture(scope="module")
def cases():
    """one draw per size, shared and never modified"""
    rng = np.random.default_rng(29)
    out = {}
    for n in SIZES:
        a, b = _values(rng, n)
        dy, _ = _values(rng, n)
        out[n] = (a, b, dy)
    return out


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("n", SIZES)
def test_join_bit_equal_at_every_phase(cases, n):
    """forward and backward at every combination of the three pointers' phases (0 to 3 floats each, independently), all four scales,
    ReLU off and on; the floats in front of and behind each result keep their bits.  Compared on the device, one read-back per phase
    combination"""
    L = _lib.lib()
    a, b, dy = cases[n]
    combos = [(s, relu) for s in SCALES for relu in (0, 1)]
    want_y = {c: R.join_forward(a, b, *c) for c in combos}
    want_g = {c: R.join_backward(dy, want_y[c], *c) for c in combos}
    dev_y = {c: _bits(torch.from_numpy(want_y[c]).cuda()) for c in combos}
    dev_g = {c: _bits(torch.from_numpy(want_g[c]).cuda()) for c in combos}
    sent = int(SENTINEL.view(np.int32))
    srcs = {off: (_padded(a, off), _padded(b, off), _padded(dy, off)) for off in range(4)}
    y, g = torch.empty(n + 3, device="cuda"), torch.empty(n + 3, device="cuda")

    def held(t, off, want):
        tb = _bits(t)
        return (tb[off:off + n] == want).all() & (tb[:off] == sent).all() & (tb[off + n:] == sent).all()

    for py in range(4):
        for pa in range(4):
            for pb in range(4):
                da, db, ddy = srcs[pa][0], srcs[pb][1], srcs[pa][2]
                flags = []
                for c in combos:
                    s, relu = c
                    y.fill_(float(SENTINEL))
                    g.fill_(float(SENTINEL))
                    assert L.w2l_residual_join_forward(y.data_ptr() + 4 * py, da.data_ptr() + 4 * pa, db.data_ptr() + 4 * pb, n, s, relu, _stream()) == 0
                    # backward: g at phase pb, dy at pa, y at py
                    assert L.w2l_residual_join_backward(g.data_ptr() + 4 * pb, ddy.data_ptr() + 4 * pa, y.data_ptr() + 4 * py, n, s, relu, _stream()) == 0
                    flags += [held(y, py, dev_y[c]), held(g, pb, dev_g[c])]
                flags = torch.stack(flags).cpu().numpy().reshape(len(combos), 2)
                assert flags.all(), (n, py, pa, pb, [(c, tuple(f)) for c, f in zip(combos, flags) if not f.all()])
    for off in range(4):   # the operands were only read
        for src, x in zip(srcs[off], (a, b, dy)):
            assert _same_bits(_inside(src, off, n), x) and _outside_untouched(src, off, n)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("n", [5, 1027])
def test_allowed_aliases(cases, n, relu):
    """y == a, y == b and g == dy, at an aligned and at an odd phase"""
    L = _lib.lib()
    a, b, dy = cases[1027]
    a, b, dy = a[:n], b[:n], dy[:n]
    s = 0.70711
    want = R.join_forward(a, b, s, relu)
    for off in (0, 1):
        for alias in ("a", "b"):
            da, db = _padded(a, off), _padded(b, off)
            y = da if alias == "a" else db
            assert L.w2l_residual_join_forward(y.data_ptr() + 4 * off, da.data_ptr() + 4 * off, db.data_ptr() + 4 * off, n, s, relu, _stream()) == 0
            assert _same_bits(_inside(y, off, n), want), (alias, off)
            assert _outside_untouched(y, off, n)
            other = db if alias == "a" else da
            assert _same_bits(_inside(other, off, n), b if alias == "a" else a)
        g, y = _padded(dy, off), _padded(want, off)
        assert L.w2l_residual_join_backward(g.data_ptr() + 4 * off, g.data_ptr() + 4 * off, y.data_ptr() + 4 * off, n, s, relu, _stream()) == 0
        assert _same_bits(_inside(g, off, n), R.join_backward(dy, want, s, relu)), off
        assert _outside_untouched(g, off, n)


def test_zero_elements_and_refusals():
    """n == 0 launches nothing (null pointers included) and leaves sentinels alone; a null pointer with n > 0 and a non-finite scale
    are W2L_EINVAL before any launch"""
    L = _lib.lib()
    t = [torch.full((8,), float(SENTINEL), device="cuda") for _ in range(3)]
    p = [x.data_ptr() for x in t]
    assert L.w2l_residual_join_forward(p[0], p[1], p[2], 0, 1.0, 1, _stream()) == 0
    assert L.w2l_residual_join_backward(p[0], p[1], p[2], 0, 1.0, 1, _stream()) == 0
    assert L.w2l_residual_join_forward(None, None, None, 0, 1.0, 0, _stream()) == 0
    assert L.w2l_residual_join_backward(None, None, None, 0, 1.0, 0, _stream()) == 0
    E = _lib.W2L_EINVAL
    for k in range(3):
        q = list(p)
        q[k] = None
        assert L.w2l_residual_join_forward(q[0], q[1], q[2], 8, 1.0, 0, _stream()) == E
        assert L.w2l_residual_join_backward(q[0], q[1], q[2], 8, 1.0, 1, _stream()) == E
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.w2l_residual_join_forward(p[0], p[1], p[2], 8, bad, 0, _stream()) == E
        assert L.w2l_residual_join_backward(p[0], p[1], p[2], 8, bad, 0, _stream()) == E
    torch.cuda.synchronize()
    for x in t:
        assert (x.cpu().numpy().view(np.int32) == SENTINEL.view(np.int32)).all()
