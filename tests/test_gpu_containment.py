"""Containment of the C ABI (DESIGN.md "Containment"): a call reads only inside its operands, writes only its results, its in-place
operands and the declared bytes of its workspaces, and writes every element of a result it does not accumulate into.

Every operand, result and workspace of a case lives in a guarded arena (tests/arena.py).  A case is one ABI call or the short
sequence a result needs; it runs on identical inputs in three arenas of identical layout -- quiet, quiet again, NaN -- and asserts
  (a) status 0 every time and every guard byte (before, between the rows of, behind each buffer) unchanged in every arena;
  (b) results and in-place operands bit-identical between the quiet and the NaN run (the two quiet runs establish that the entry
      point is reproducible at all; one that is not is compared at the bar of (d) instead and printed as NOT REPRODUCIBLE);
  (c) no valid element of a non-accumulated result still holds the prefill pattern after the NaN run;
  (d) the quiet result agrees with the float64 restatement of the operation at the bar the family's own test uses: 1e-4 of the
      largest magnitude for fp32 (tests/test_gpu_nn.py, test_gpu_criterion.py, test_gpu_attention.py), the (K + 2) 2^-24 bound
      on bf16 operands (tests/test_gpu_gemm_smallm.py), bit-exact for copies, masks, paths and integer results.
Shapes are the smallest at which the address arithmetic can go wrong: odd sizes, sizes that are no multiple of a tile or a vector,
one element, leading dimensions above the natural one.  Every call is a legal one: nothing here is meant to fault."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.arena import NAN_PATTERN, QUIET_PATTERN, Arena
from wav2letter_amd import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-4
F32, I32, I16, U8, F64 = torch.float32, torch.int32, torch.int16, torch.uint8, torch.float64


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def switches(env):
    """the product library, or -- for the kernel-variant switches -- the probe library with `env` set (tests/test_gpu_nn.py `probe`)"""
    if not env:
        yield _lib.lib()
        return
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with _lib.use_probe() as L:
            yield L
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Run:
    """one run of a case in one arena: places buffers, collects the results to compare"""

    def __init__(self, arena, L):
        self.ar, self.L, self.results, self.fresh, self.empty_work = arena, L, {}, [], []

    def inp(self, name, data, ld=None, dtype=None):
        data = np.asarray(data)
        dtype = dtype or {np.dtype(np.float32): F32, np.dtype(np.int32): I32, np.dtype(np.int16): I16, np.dtype(np.float64): F64}[data.dtype]
        return self.ar.place(data.shape, dtype, ld=ld, kind="in", name=name, data=data)[1]

    def inout(self, name, data, ld=None):
        data = np.asarray(data)
        dtype = {np.dtype(np.float32): F32, np.dtype(np.int32): I32, np.dtype(np.int16): I16, np.dtype(np.float64): F64}[data.dtype]
        view, ptr = self.ar.place(data.shape, dtype, ld=ld, kind="inout", name=name, data=data)
        self.results[name] = view
        return ptr

    def out(self, name, shape, dtype=F32, ld=None):
        """a result the call overwrites: every valid element must be written (c).  A buffer a call writes only in part by contract is
        placed as a workspace instead and what was written is added to `results` by the case"""
        view, ptr = self.ar.place(shape, dtype, ld=ld, kind="out", name=name)
        self.results[name] = view
        self.fresh.append(name)
        return ptr

    def work(self, name, nbytes):
        """a workspace of EXACTLY the declared bytes (one untouchable byte when the size function says 0)"""
        nbytes = int(nbytes)
        if nbytes == 0:
            self.empty_work.append(name)
        return self.ar.place((max(nbytes, 1),), U8, kind="work", name=name)[1]

    def view(self, name):
        return self.ar.buffer(name).view

    def ok(self, status, what=""):
        assert status == 0, (what, _lib._ERR.get(status, status), self.L.w2l_last_hip_error())


def bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def meets(bar, got, want, what):
    """(d): `got` (numpy) against the float64 restatement `want` at the family's bar"""
    got64, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got64.shape == want.shape, (what, got64.shape, want.shape)
    if bar == "exact":
        assert np.array_equal(got64, want), (what, float(np.abs(got64 - want).max()))
    elif bar == "rel":        # tests/test_gpu_nn.py rel(): 1e-4 of the largest reference magnitude
        err = np.abs(got64 - want).max() / max(1e-30, np.abs(want).max())
        assert err < TOL, (what, err)
    elif bar == "loss":       # tests/test_gpu_criterion.py relerr(): losses, 1e-4 of max(1, largest magnitude)
        with np.errstate(invalid="ignore"):
            err = np.nan_to_num(np.abs(got64 - want), nan=0.0, posinf=np.inf).max() / max(1.0, np.abs(want[np.isfinite(want)]).max(initial=0.0))
        assert np.array_equal(np.isinf(got64), np.isinf(want)) and err < TOL, (what, err)
    elif bar == "each":       # tests/test_gpu_ctc_align.py: every element within 1e-4 of max(1, its own magnitude); -inf where the reference is
        fin = np.isfinite(want)
        assert np.array_equal(got64[~fin], want[~fin]), what
        assert (np.abs(got64[fin] - want[fin]) <= TOL * np.maximum(1, np.abs(want[fin]))).all(), (what, got64, want)
    elif bar == "param":      # tests/test_gpu_nn.py: the two LayerNorm parameter gradients, 1e-3 of max(1, magnitude)
        assert (np.abs(got64 - want) < 10 * TOL * np.maximum(1, np.abs(want))).all(), (what, got64, want)
    elif isinstance(bar, tuple) and bar[0] == "rel":
        err = np.abs(got64 - want).max() / max(1e-30, np.abs(want).max())
        assert err < bar[1], (what, err)
    elif isinstance(bar, tuple) and bar[0] == "bound":     # elementwise bound (bf16 operands, fp32 accumulation)
        assert np.isfinite(got64).all(), what
        over = np.abs(got64 - want) - bar[1]      # (an element no product reaches has error 0 under a bound of 0)
        assert (over <= 0).all(), (what, float(over.max()))
    else:
        raise AssertionError(bar)


CASES = {}


def case(name, env=None, capacity=32 << 20):
    def reg(fn):
        assert name not in CASES, name
        CASES[name] = (fn, env or {}, capacity)
        return fn
    return reg


def run_case(name):
    fn, env, capacity = CASES[name]
    runs = []
    with switches(env) as L:
        for pattern in (QUIET_PATTERN, QUIET_PATTERN, NAN_PATTERN):
            r = Run(Arena("cuda", pattern, capacity), L)
            ref = fn(r)
            torch.cuda.synchronize()
            r.ar.check()                                                      # (a)
            runs.append((r, ref))
    (q, ref), (q2, _), (n, _) = runs
    assert q.results, name
    want = {key: v for key, v in ref().items() if key in q.results}      # (a reference table may cover variants this case did not run)
    missing = set(q.results) - set(want)
    assert not missing, f"{name}: results without a reference or a stated reason for having none: {sorted(missing)}"
    for key in q.results:
        a, b, c = q.results[key], q2.results[key], n.results[key]
        if torch.equal(bits(a), bits(b)):
            assert torch.equal(bits(a), bits(c)), (                          # (b)
                f"{name}: result '{key}' depends on bytes outside the operands: {int((bits(a) != bits(c)).sum())} of {a.numel()} "
                f"elements differ between the quiet and the NaN arena, {int(torch.isnan(c).sum()) if c.is_floating_point() else 0} are NaN")
        else:
            print(f"NOT REPRODUCIBLE: {name}: '{key}' differs between two quiet runs; compared at the bar of (d)")
            assert want[key][0] != "none", (name, key)
            meets(want[key][0], c.cpu().numpy(), want[key][1], f"{name}/{key} (NaN arena)")
    for key in n.fresh:                                                       # (c)
        left = n.ar.unwritten(key)
        assert left == 0, f"{name}: {left} valid elements of result '{key}' were never written"
    for key in n.empty_work:
        assert n.ar.unwritten(key) == 1, f"{name}: workspace '{key}' has a declared size of 0 bytes and was written"
    for key, (bar, ref64) in want.items():                                    # (d)
        if bar == "none":      # ref64 is the reason why the result has no restatement: (a) - (c) only
            assert isinstance(ref64, str) and ref64, (name, key)
            continue
        meets(bar, q.results[key].cpu().numpy(), ref64, f"{name}/{key}")


# ---- the harness on the device -------------------------------------------------------------------------------------------------
def test_arena_finds_scribbles_on_the_device():
    """tests/test_arena_host.py's scribbles with plain torch indexing into a device arena: no kernel of the project involved"""
    from tests.arena import GuardError
    for pattern in (NAN_PATTERN, QUIET_PATTERN):
        ar = Arena("cuda", pattern, capacity=4 << 20)
        ar.place((3,), I32, kind="in", name="sizes")
        v, ptr = ar.place((5, 7), F32, ld=11, kind="out", name="c")
        ar.place((1001,), U8, kind="work", name="ws")
        assert ptr % 256 == 0 and v.is_cuda
        ar.check()
        if pattern:
            assert ar.unwritten("c") == 35 and torch.isnan(v).all()
        v.copy_(torch.arange(35, dtype=F32).reshape(5, 7))
        ar.check()
        if pattern:
            assert ar.unwritten("c") == 0
        for name, offset, where in (("c", -1, "before"), ("c", 7 * 4, "between rows"), ("c", 3 * 44 + 43, "between rows"),
                                    ("c", 51 * 4, "behind"), ("ws", 1001, "behind"), ("sizes", -4, "before"), ("sizes", 12, "behind")):
            b = ar.buffer(name)
            at = b.start + offset
            ar.mem[at] = ar.mem[at] ^ 0x40
            assert ar.damage(name)[:3] == (where, offset, offset), (name, offset)
            with pytest.raises(GuardError) as e:
                ar.check()
            assert f"'{name}'" in str(e.value) and where in str(e.value) and f"offset {offset}," in str(e.value)
            ar.mem[at] = ar.mem[at] ^ 0x40
            ar.check()


# ---- fp32 GEMM: every dispatch line of gemm.hip, four operand layouts, natural and padded leading dimensions --------------------
GEMM_LINES = [  # tag, (M, N, K), switches, leading-dimension paddings
    ("line5", (1, 1, 1), {}, (0, 4, 1)), ("line5", (5, 7, 3), {}, (0, 4, 1)), ("line5", (129, 127, 33), {}, (0, 4, 1)),
    ("line5forced", (132, 124, 96), {"W2L_GEMM_GLDS": "0"}, (0, 4, 1)),
    ("line4", (132, 124, 96), {}, (0, 4, 1)), ("line4", (4, 4, 32), {}, (0, 4, 1)),
    ("line3t160=2", (132, 164, 96), {"W2L_GEMM_T160": "2"}, (0, 4)), ("line3t160=3", (132, 164, 96), {"W2L_GEMM_T160": "3"}, (0, 4)),
    ("line2", (132, 124, 300), {}, (0, 4)),
    ("streamk", (256, 384, 2000), {}, (0, 4)), ("streamk-fixup", (256, 384, 2000), {"W2L_GEMM_INFIX": "0", "W2L_GEMM_T160": "0"}, (0, 4)),
]


EPILOGUES = {"plain": (False, 0), "bias": (True, 0), "bias_relu": (True, 1)}


def _gemm_case(M, N, K, akc, bkc, pad, epilogue):
    def fn(r):
        rng = np.random.default_rng(M * 1009 + N * 31 + K)
        A = rng.normal(size=(M, K)).astype(np.float32)
        B = (rng.normal(size=(K, N)) / np.sqrt(K)).astype(np.float32)
        bias = rng.normal(size=N).astype(np.float32)
        As, Bs = (A if akc else A.T), (B.T if bkc else B)
        lda, ldb, ldc = As.shape[1] + pad, Bs.shape[1] + pad, N + pad
        with_bias, relu = EPILOGUES[epilogue]
        pa, pb = r.inp("A", As, ld=lda), r.inp("B", Bs, ld=ldb)
        pbias = r.inp("bias", bias) if with_bias else None
        r.ok(r.L.w2l_gemm_f32(M, N, K, pa, lda, int(akc), pb, ldb, int(bkc), r.out("C", (M, N), ld=ldc), ldc, pbias, relu, 1, _stream()))

        def ref():
            c = A.astype(np.float64) @ B.astype(np.float64) + (bias if with_bias else 0.0)
            return {"C": ("rel", np.maximum(c, 0) if relu else c)}
        return ref
    return fn


for _tag, (_M, _N, _K), _env, _pads in GEMM_LINES:
    for _akc, _bkc in ((1, 0), (1, 1), (0, 0), (0, 1)):
        for _pad in _pads:
            for _epi in EPILOGUES:
                case(f"gemm_f32/{_tag}/{_M}x{_N}x{_K}/a{'k' if _akc else 'm'}b{'k' if _bkc else 'n'}/ld+{_pad}/{_epi}", env=_env)(
                    _gemm_case(_M, _N, _K, _akc, _bkc, _pad, _epi))


# ---- fl::Linear epilogues -------------------------------------------------------------------------------------------------------
def _keep_factors(oracle, n, p, seed, sid):
    """the dropout of the library as factors 0 or 1 / (1 - p) over a flat index range (oracle/pyoracle.py dropout: bit-exact mask)"""
    return oracle.dropout(np.ones(n, np.float32), p, seed, sid).astype(np.float64)


def _linear_cases(M, nin, nout):
    rng = np.random.default_rng(M + nin + nout)
    x = rng.normal(size=(M, nin)).astype(np.float32)
    w = (rng.normal(size=(nin, nout)) / np.sqrt(nin)).astype(np.float32)
    b = rng.normal(size=nout).astype(np.float32)
    dy = rng.normal(size=(M, nout)).astype(np.float32)
    add_y = rng.normal(size=(M, nout)).astype(np.float32)
    add_x = rng.normal(size=(M, nin)).astype(np.float32)
    msk = rng.normal(size=(M, nin)).astype(np.float32)
    x64, w64, dy64 = x.astype(np.float64), w.astype(np.float64), dy.astype(np.float64)
    p, seed, sid = 0.3, 12345, 7
    tag = f"linear/{M}x{nin}x{nout}/"

    @case(tag + "forward")
    def _(r):
        px, pw, pb = r.inp("x", x), r.inp("w", w), r.inp("b", b)
        r.ok(r.L.w2l_linear_forward(M, nin, nout, px, pw, pb, r.out("y", (M, nout)), 0, _stream()))
        r.ok(r.L.w2l_linear_forward(M, nin, nout, px, pw, pb, r.out("y_relu", (M, nout)), 1, _stream()))
        r.ok(r.L.w2l_linear_forward(M, nin, nout, px, pw, None, r.out("y_nobias", (M, nout)), 0, _stream()))
        return lambda: {"y": ("rel", x64 @ w64 + b), "y_relu": ("rel", np.maximum(x64 @ w64 + b, 0)), "y_nobias": ("rel", x64 @ w64)}

    def keep():
        from oracle import pyoracle
        return _keep_factors(pyoracle, M * nout, p, seed, sid).reshape(M, nout)

    @case(tag + "forward_dropout")
    def _(r):
        px, pw, pb = r.inp("x", x), r.inp("w", w), r.inp("b", b)
        r.ok(r.L.w2l_linear_forward_dropout(M, nin, nout, px, pw, pb, r.out("y", (M, nout)), 1, p, seed, sid, _stream()))
        return lambda: {"y": ("rel", np.maximum(x64 @ w64 + b, 0) * keep())}

    @case(tag + "forward_dropout_add")
    def _(r):
        px, pw, pb, padd = r.inp("x", x), r.inp("w", w), r.inp("b", b), r.inp("add", add_y)
        r.ok(r.L.w2l_linear_forward_dropout_add(M, nin, nout, px, pw, pb, padd, r.out("y_add", (M, nout)), 0, p, seed, sid, _stream()))
        r.ok(r.L.w2l_linear_forward_dropout_add(M, nin, nout, px, pw, pb, padd, r.out("y_add_p0", (M, nout)), 0, 0.0, seed, sid, _stream()))
        return lambda: {"y_add": ("rel", (x64 @ w64 + b) * keep() + add_y), "y_add_p0": ("rel", x64 @ w64 + b + add_y)}

    dx = dy64 @ w64.T

    @case(tag + "backward_data")
    def _(r):
        pdy, pw, pm = r.inp("dy", dy), r.inp("w", w), r.inp("mask", msk)
        r.ok(r.L.w2l_linear_backward_data(M, nin, nout, pdy, pw, r.out("dx", (M, nin)), 0, None, 1.0, _stream()))
        r.ok(r.L.w2l_linear_backward_data(M, nin, nout, pdy, pw, r.inout("dx_acc", add_x), 1, None, 1.0, _stream()))
        r.ok(r.L.w2l_linear_backward_data(M, nin, nout, pdy, pw, r.out("dx_mask", (M, nin)), 0, pm, 1.25, _stream()))
        return lambda: {"dx": ("rel", dx), "dx_acc": ("rel", dx + add_x), "dx_mask": ("rel", np.where(msk > 0, dx * 1.25, 0.0))}

    @case(tag + "backward_data_add")
    def _(r):
        r.ok(r.L.w2l_linear_backward_data_add(M, nin, nout, r.inp("dy", dy), r.inp("w", w), r.inp("add", add_x), r.out("dx_add", (M, nin)), _stream()))
        return lambda: {"dx_add": ("rel", dx + add_x)}

    @case(tag + "backward_weight")
    def _(r):
        r.ok(r.L.w2l_linear_backward_weight(M, nin, nout, r.inp("x", x), r.inp("dy", dy), r.out("dw", (nin, nout)), _stream()))
        return lambda: {"dw": ("rel", x64.T @ dy64)}

    @case(tag + "backward_weight_bias")
    def _(r):
        r.ok(r.L.w2l_linear_backward_weight_bias(M, nin, nout, r.inp("x", x), r.inp("dy", dy), r.out("dw", (nin, nout)), r.out("db", (nout,)), _stream()))
        return lambda: {"dw": ("rel", x64.T @ dy64), "db": (("rel", 1e-5), dy64.sum(0))}


_linear_cases(132, 96, 252)
_linear_cases(37, 20, 13)
_linear_cases(132, 96, 320)      # dw [96][320] is eligible for the 160-wide kernel: the column sums ride on it


def _colsum_case(M, N):
    @case(f"colsum/{M}x{N}")
    def _(r):
        x = np.random.default_rng(M + N).normal(size=(M, N)).astype(np.float32)
        r.ok(r.L.w2l_colsum(r.inp("x", x), r.out("out", (N,)), M, N, _stream()))
        return lambda: {"out": ("rel", x.astype(np.float64).sum(0))}


for _M, _N in ((1, 5), (63, 1), (513, 37)):
    _colsum_case(_M, _N)


# ---- elementwise and the rest: element counts that are not vector multiples ------------------------------------------------------
def _elementwise_cases(n):
    rng = np.random.default_rng(n)
    x = rng.normal(size=n).astype(np.float32)
    y = rng.normal(size=n).astype(np.float32)
    z = np.abs(rng.normal(size=n)).astype(np.float32)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    tag = f"elementwise/n={n}/"

    @case(tag + "dropout_copy")
    def _(r):
        from oracle import pyoracle
        px = r.inp("x", x)
        r.ok(r.L.w2l_dropout_copy(r.out("y", (n,)), px, n, 0.25, 77, 5, _stream()))
        r.ok(r.L.w2l_dropout_copy(r.out("y_p0", (n,)), px, n, 0.0, 77, 5, _stream()))
        return lambda: {"y": ("exact", pyoracle.dropout(x, 0.25, 77, 5)), "y_p0": ("exact", x)}

    @case(tag + "dropout_inplace")
    def _(r):
        from oracle import pyoracle
        r.ok(r.L.w2l_dropout_inplace(r.inout("x", x), n, 0.25, 77, 5, _stream()))
        return lambda: {"x": ("exact", pyoracle.dropout(x, 0.25, 77, 5))}

    @case(tag + "mask_backward")
    def _(r):
        r.ok(r.L.w2l_mask_backward(r.inp("dy", y), r.inp("src", x), r.out("dx", (n,)), n, 1.25, _stream()))
        return lambda: {"dx": ("rel", np.where(x > 0, y64 * 1.25, 0.0))}

    @case(tag + "axpy")
    def _(r):
        r.ok(r.L.w2l_axpy(r.inout("y", y), r.inp("x", x), n, 0.5, _stream()))
        return lambda: {"y": ("rel", y64 + 0.5 * x64)}

    @case(tag + "ema_update")
    def _(r):
        r.ok(r.L.w2l_ema_update(r.inout("ema", y), r.inp("p", x), n, 0.75, _stream()))
        return lambda: {"ema": ("rel", 0.75 * y64 + 0.25 * x64)}

    @case(tag + "fill")
    def _(r):
        r.ok(r.L.w2l_fill(r.out("filled", (n,)), n, 3.5, _stream()))
        return lambda: {"filled": ("exact", np.full(n, 3.5))}

    s2 = float((x64 ** 2).sum())

    @case(tag + "sumsq")
    def _(r):
        pg = r.inp("g", x)
        r.ok(r.L.w2l_sumsq(pg, n, r.out("ss", (1,), F64), 1, _stream()))
        r.ok(r.L.w2l_sumsq(pg, n, r.inout("ss_acc", np.array([2.0])), 0, _stream()))
        return lambda: {"ss": (("rel", 1e-5), [s2]), "ss_acc": (("rel", 1e-5), [s2 + 2.0])}

    bar5 = ("rel", 1e-5)       # tests/test_gpu_nn.py test_glu_transpose_sgd

    @case(tag + "sgd_step")
    def _(r):
        pg = r.inp("g", x)
        r.ok(r.L.w2l_sgd_step(r.inout("p", y), pg, r.inout("v", z), n, 0.3, 0.5, 0.25, 1.0, r.inp("sumsq", np.array([s2])), _stream()))
        r.ok(r.L.w2l_sgd_step(r.inout("p_noclip", y), pg, r.inout("v_noclip", z), n, 0.3, 0.5, 0.25, 0.0, None, _stream()))

        def ref():
            gs = x64 * 0.25
            coef = min(1.0, 1.0 / (np.linalg.norm(gs) + 1e-6))
            v1, v2 = 0.5 * z + gs * coef, 0.5 * z + gs
            return {"v": (bar5, v1), "p": (bar5, y64 - 0.3 * v1), "v_noclip": (bar5, v2), "p_noclip": (bar5, y64 - 0.3 * v2)}
        return ref

    @case(tag + "sgd_step_guarded")
    def _(r):
        guard = np.array([s2, 0.5])
        r.ok(r.L.w2l_sgd_step_guarded(r.inout("p", y), r.inp("g", x), r.inout("v", z), n, 0.3, 0.5, 0.25, 0.0, r.inp("guard", guard), _stream()))
        v3 = 0.5 * z + x64 * 0.5
        return lambda: {"v": (bar5, v3), "p": (bar5, y64 - 0.3 * v3)}

    g = x64 * 0.25

    @case(tag + "adagrad_step_guarded")
    def _(r):
        r.ok(r.L.w2l_adagrad_step_guarded(r.inout("p", y), r.inp("g", x), r.inout("var", z), n, 0.3, 1e-8, 0.25, 0.0, None, _stream()))
        var = z + g * g
        return lambda: {"var": ("rel", var), "p": ("rel", y64 - 0.3 * g / (np.sqrt(var) + 1e-8))}

    @case(tag + "adadelta_step_guarded")
    def _(r):
        r.ok(r.L.w2l_adadelta_step_guarded(r.inout("p", y), r.inp("g", x), r.inout("acc_grad", z), r.inout("acc_delta", np.flip(z).copy()), n,
                                           0.3, 0.9, 1e-8, 0.25, 0.0, None, _stream()))

        def ref():
            ag = 0.9 * z + 0.1 * g * g
            ad0 = np.flip(z).astype(np.float64)
            delta = np.sqrt(ad0 + 1e-8) / np.sqrt(ag + 1e-8) * g
            return {"acc_grad": ("rel", ag), "p": ("rel", y64 - 0.3 * delta), "acc_delta": ("rel", 0.9 * ad0 + 0.1 * delta * delta)}
        return ref


for _n in (1, 3, 1023, 4097):
    _elementwise_cases(_n)


@case("glu/M=3,half=5")
def _(r):
    from oracle import pyoracle
    rng = np.random.default_rng(8)
    M, half = 3, 5
    x = rng.normal(size=(M, 2 * half)).astype(np.float32)
    dy = rng.normal(size=(M, half)).astype(np.float32)
    px = r.inp("x", x)
    r.ok(r.L.w2l_glu_forward(px, r.out("y", (M, half)), M, half, _stream()))
    r.ok(r.L.w2l_glu_backward(px, r.inp("dy", dy), r.out("dx", (M, 2 * half)), M, half, _stream()))
    return lambda: {"y": ("rel", pyoracle.glu_fwd(x, M, half, 1).reshape(M, half)), "dx": ("rel", pyoracle.glu_bwd(x, dy, M, half, 1).reshape(M, 2 * half))}


def _transpose_case(G, R, Cc):
    @case(f"transpose/{G}x{R}x{Cc}")
    def _(r):
        t = np.random.default_rng(R).normal(size=(G, R, Cc)).astype(np.float32)
        r.ok(r.L.w2l_transpose(r.inp("in", t), r.out("out", (G, Cc, R)), G, R, Cc, _stream()))
        return lambda: {"out": ("exact", t.transpose(0, 2, 1))}


_transpose_case(2, 5, 7)
_transpose_case(1, 33, 65)


def _hexpand_case(rows, H, Cc, kh, padh):
    @case(f"hexpand/rows={rows},H={H},C={Cc},kh={kh},padh={padh}")
    def _(r):
        rng = np.random.default_rng(rows + H)
        x = rng.normal(size=(rows, H, Cc)).astype(np.float32)
        dxe = rng.normal(size=(rows, H, kh * Cc)).astype(np.float32)
        r.ok(r.L.w2l_hexpand_forward(r.inp("x", x), r.out("xe", (rows, H, kh * Cc)), rows, H, Cc, kh, padh, _stream()))
        r.ok(r.L.w2l_hexpand_backward(r.inp("dxe", dxe), r.out("dx", (rows, H, Cc)), rows, H, Cc, kh, padh, _stream()))

        def ref():
            xe, dx = np.zeros((rows, H, kh, Cc)), np.zeros((rows, H, Cc))
            d4 = dxe.astype(np.float64).reshape(rows, H, kh, Cc)
            for h in range(H):
                for dh in range(kh):
                    hs = h + dh - padh
                    if 0 <= hs < H:
                        xe[:, h, dh] = x[:, hs]
                        dx[:, hs] += d4[:, h, dh]
            return {"xe": ("exact", xe.reshape(rows, H, kh * Cc)), "dx": ("rel", dx)}
        return ref


_hexpand_case(3, 5, 3, 3, 1)
_hexpand_case(1, 7, 1, 5, 2)


def _weightnorm_case(K, N):
    @case(f"weightnorm/{K}x{N}")
    def _(r):
        from oracle import pyoracle
        rng = np.random.default_rng(K + N)
        v = rng.normal(size=(K, N)).astype(np.float32)
        g = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
        dw = rng.normal(size=(K, N)).astype(np.float32)
        pv, pg = r.inp("v", v), r.inp("g", g)
        pnorm = r.out("norm", (N,))
        r.ok(r.L.w2l_weightnorm_forward(pv, pg, r.out("w", (K, N)), pnorm, K, N, _stream()))
        r.ok(r.L.w2l_weightnorm_backward(pv, pg, pnorm, r.inp("dw", dw), r.out("dv", (K, N)), r.out("dg", (N,)), r.work("dot", 4 * N),
                                         K, N, _stream()))

        def ref():
            odv, odg = pyoracle.weightnorm_bwd(v, g, dw, K, N, 1)
            return {"w": ("rel", np.asarray(pyoracle.weightnorm_fwd(v, g, K, N, 1)).reshape(K, N)),
                    "norm": (("rel", 1e-5), np.sqrt((v.astype(np.float64) ** 2).sum(0))), "dv": ("rel", np.asarray(odv).reshape(K, N)),
                    "dg": ("rel", np.asarray(odg).reshape(N))}
        return ref


_weightnorm_case(15, 4)
_weightnorm_case(333, 77)


@case("specaugment/3x57x40")
def _(r):
    from oracle import pyoracle
    B, T, F = 3, 57, 40
    args = (15, 1, 50, 0.2, 2)
    x = np.random.default_rng(3).normal(size=(B, T, F)).astype(np.float32)
    r.ok(r.L.w2l_specaugment_inplace(r.inout("x", x), B, T, F, *args, 99, _stream()))
    return lambda: {"x": ("exact", pyoracle.specaugment(x, *args, 99)[0])}


@case("mfsc/spectrum_and_log_transpose")
def _(r):
    rng = np.random.default_rng(4)
    M, nbins, ldo = 7, 33, 40
    reim = rng.normal(size=(M, 2 * nbins)).astype(np.float32)
    for power in (0, 1):   # the header: zero-padded to ldOut columns -- the padding is part of the result
        r.ok(r.L.w2l_mfsc_spectrum(r.inp(f"reim{power}", reim), r.out(f"spec{power}", (M, ldo)), M, nbins, ldo, power, _stream()))
    B, Tp, T, F = 2, 9, 7, 5
    mel = (np.abs(rng.normal(size=(B, Tp, F))) * 3).astype(np.float32)
    r.ok(r.L.w2l_mfsc_log_transpose(r.inp("mel", mel), r.out("feat", (B, F, T)), B, Tp, T, F, 1.0, _stream()))

    def ref():
        re, im = reim[:, :nbins].astype(np.float64), reim[:, nbins:].astype(np.float64)
        out = {}
        for power in (0, 1):
            s = np.zeros((M, ldo))
            s[:, :nbins] = re * re + im * im if power else np.sqrt(re * re + im * im)
            out[f"spec{power}"] = ("rel", s)
        out["feat"] = ("rel", np.log(np.maximum(mel[:, :T].astype(np.float64), 1.0)).transpose(0, 2, 1))
        return out
    return ref


def _mean_rstd(r32, eps):
    """[2 groups]: mean and 1 / sqrt(biased variance + eps) of every group, interleaved as the kernels store them"""
    r64 = r32.astype(np.float64)
    return np.stack([r64.mean(1), 1.0 / np.sqrt(r64.var(1) + eps)], axis=1).reshape(-1)


# ---- LayerNorm: the wave, one-block, two-level and scalar kernels ------------------------------------------------------------------
def _layernorm_case(groups, inner, p, with_x, alias, with_mask):
    name = f"layernorm/groups={groups},inner={inner},p={p}" + ("" if with_x else ",no-x") + (",r==a" if alias else "") + (",mask" if with_mask else "")

    @case(name, capacity=(192 << 20) if inner > 4096 else (64 << 20))
    def _(r):
        from oracle import pyoracle
        L = r.L
        rng = np.random.default_rng(groups * 100003 + inner)
        a = np.maximum(rng.normal(size=(groups, inner)), 0).astype(np.float32)
        x = rng.normal(size=(groups, inner)).astype(np.float32)
        dy = rng.normal(size=(groups, inner)).astype(np.float32)
        gb = np.array([1.3, -0.2], np.float32)
        nd = int(L.w2l_layernorm_scratch_doubles(groups, inner))
        pa = r.inout("a", a)
        pr = pa if alias else r.out("r", (groups, inner))
        py, pgb, pmr = r.out("y", (groups, inner)), r.inp("gammaBeta", gb), r.out("meanRstd", (2 * groups,))
        r.ok(L.w2l_residual_layernorm_forward(groups, inner, pa, r.inp("x", x) if with_x else None, pr, py, pgb, 1e-5, p, 77, 5,
                                              r.work("stats", 8 * nd), pmr, _stream()), "forward")
        if inner % 4 == 0:
            pmask = r.inp("maskSrc", a) if with_mask else None      # a copy of the un-dropped branch output: any mask source will do
            r.ok(L.w2l_layernorm_backward(groups, inner, pr, r.inp("dy", dy), pgb, pmr, r.out("dr", (groups, inner)), r.out("dGammaBeta", (2,)),
                                          pmask, r.out("dmask", (groups, inner)) if with_mask else None, 1.25, r.work("sums", 8 * nd),
                                          _stream()), "backward")

        def ref():
            a_drop = pyoracle.dropout(a.reshape(-1), p, 77, 5).reshape(a.shape) if p > 0 else a
            r_ref = a_drop.astype(np.float64) + (x if with_x else 0.0)
            r32 = r_ref.astype(np.float32)
            y_ref = np.asarray(pyoracle.layernorm_fwd(r32, groups, 1.3, -0.2, 1e-5)).reshape(groups, inner)
            out = {"y": ("rel", y_ref), ("a" if alias else "r"): (("rel", 1e-6), r_ref), "meanRstd": ("rel", _mean_rstd(r32, 1e-5))}
            if not alias:
                out["a"] = ("exact", a_drop)
            if inner % 4 == 0:
                odr, odg, odb = pyoracle.layernorm_bwd(r32, dy, groups, 1.3, 1e-5)
                odr = np.asarray(odr).reshape(groups, inner)
                out["dr"] = ("rel", odr)
                out["dGammaBeta"] = ("param", [float(odg), float(odb)])
                if with_mask:
                    out["dmask"] = ("rel", odr * (a > 0) * 1.25)
            return out
        return ref


for _inner in (8, 2304, 2308, 8192, 8196):
    for _groups in (1, 3, 5):
        _layernorm_case(_groups, _inner, 0.0, True, False, False)
        _layernorm_case(_groups, _inner, 0.25, True, False, True)
    _layernorm_case(3, _inner, 0.25, False, False, False)
    _layernorm_case(3, _inner, 0.25, True, True, True)
for _groups in (1, 3, 5):
    _layernorm_case(_groups, 10, 0.25, True, False, False)      # scalar kernel: forward only, r must not alias a


# ---- fp32 convolutions -------------------------------------------------------------------------------------------------------------
def _conv_ref64(x, w, b, dy, stride, padl, padr):
    """float64 cross-correlation over time and its gradients; x [B][T][H][Cin], w [kw][Cin][Cout], dy [B][To][H][Cout]"""
    import torch.nn.functional as Fn
    xr = torch.from_numpy(x).double().permute(0, 3, 2, 1).requires_grad_(True)          # [B][Cin][H][T]
    wr = torch.from_numpy(w).double().permute(2, 1, 0)[:, :, None, :].contiguous().requires_grad_(True)   # [Cout][Cin][1][kw]
    br = torch.from_numpy(b).double().requires_grad_(True)
    yr = Fn.conv2d(Fn.pad(xr, (padl, padr)), wr, br, stride=(1, stride))
    yr.backward(torch.from_numpy(dy).double().permute(0, 3, 2, 1))
    return (yr.permute(0, 3, 2, 1).detach().numpy(), xr.grad.permute(0, 3, 2, 1).numpy(), wr.grad[:, :, 0, :].permute(2, 1, 0).numpy(),
            br.grad.numpy())


def _conv_case(B, Cin, Cout, H, T, kw, stride, padl, padr, why):
    @case(f"conv_f32/{why}/B={B},Cin={Cin},Cout={Cout},H={H},T={T},kw={kw},s={stride},pad={padl}+{padr}")
    def _(r):
        L = r.L
        rng = np.random.default_rng(Cin * 100 + Cout + T)
        To = (T + padl + padr - kw) // stride + 1
        assert To == L.w2l_conv_out_len(T, kw, stride, padl, padr) and To >= 1
        x = rng.normal(size=(B, T, H, Cin)).astype(np.float32)
        w = (rng.normal(size=(kw, Cin, Cout)) / np.sqrt(Cin * kw)).astype(np.float32)
        b = rng.normal(size=Cout).astype(np.float32)
        dy = rng.normal(size=(B, To, H, Cout)).astype(np.float32)
        base = rng.normal(size=x.shape).astype(np.float32)
        d = _lib.ConvDesc(B, T, H, Cin, Cout, kw, stride, padl, padr)
        px, pw, pb, pdy, padd = r.inp("x", x), r.inp("w", w), r.inp("bias", b), r.inp("dy", dy), r.inp("add", base)
        r.ok(L.w2l_conv_forward(C.byref(d), px, pw, pb, r.out("y", dy.shape), 0, _stream()), "forward")
        r.ok(L.w2l_conv_forward(C.byref(d), px, pw, pb, r.out("y_relu", dy.shape), 1, _stream()), "forward relu")
        r.ok(L.w2l_conv_backward_data(C.byref(d), pdy, pw, r.out("dx", x.shape), 0, _stream()), "backward data")
        r.ok(L.w2l_conv_backward_data(C.byref(d), pdy, pw, r.inout("dx_acc", base), 1, _stream()), "backward data accumulate")
        r.ok(L.w2l_conv_backward_data_add(C.byref(d), pdy, pw, padd, r.out("dx_add", x.shape), _stream()), "backward data add")
        r.ok(L.w2l_conv_backward_filter(C.byref(d), px, pdy, r.out("dw", w.shape), r.out("dbias", (Cout,)), _stream()), "backward filter")

        def ref():
            y, dx, dw, db = _conv_ref64(x, w, b, dy, stride, padl, padr)
            return {"y": ("rel", y), "y_relu": ("rel", np.maximum(y, 0)), "dx": ("rel", dx), "dx_acc": ("rel", dx + base),
                    "dx_add": ("rel", dx + base), "dw": ("rel", dw), "dbias": ("rel", db)}
        return ref


_conv_case(2, 1, 10, 8, 50, 21, 2, 10, 10, "stride2-first-layer")
_conv_case(2, 10, 14, 6, 41, 21, 2, 10, 10, "stride2-odd-T")
_conv_case(2, 40, 400, 1, 90, 13, 1, 170, 170, "pad>kw")
_conv_case(2, 5, 7, 3, 6, 9, 1, 8, 0, "T<kw")
_conv_case(1, 33, 70, 1, 45, 4, 1, 2, 2, "odd-channels")
for _Cc, _T, _B, _H in ((10, 1, 1, 80), (14, 1, 1, 80), (18, 2, 2, 80), (10, 50, 2, 80), (14, 24, 2, 80), (18, 12, 2, 80), (10, 77, 2, 12)):
    _conv_case(_B, _Cc, _Cc, _H, _T, 21, 1, 10, 10, "tds")


# ---- criteria with caller workspaces ---------------------------------------------------------------------------------------------------
def _targets(rng, B, L, hi, T):
    tgt = np.full((B, L), -1, np.int32)
    for b in range(B):
        n = int(rng.integers(1, min(L, T) + 1))
        tgt[b, :n] = rng.integers(0, hi, size=n)
    return tgt


def _ctc_case(B, T, N, L, long_row=False):
    @case(f"ctc/B={B},T={T},N={N},L={L}", capacity=160 << 20)
    def _(r):
        from oracle import pyoracle
        from tests.ctc_align_ref import ctc_align_ref
        lib = r.L
        rng = np.random.default_rng(N + L)
        x = (rng.normal(size=(B, T, N)) * 2).astype(np.float32)
        tgt = _targets(rng, B, L, N - 1, T)
        if long_row:
            tgt[0, :] = np.arange(L) % (N - 1)          # L labels, no adjacent repeats: the widest lattice
        elif B > 2:
            tgt[0, :] = -1                              # empty transcription
        if L >= 4:
            tgt[1, :4] = [1, 1, 0, 0]                   # repeats
        w = rng.normal(size=B).astype(np.float32)
        ts = pyoracle.batch_ctc_target_size(tgt, T)
        frames = np.array([T - (b % 2) for b in range(B)], np.int32)
        px, pt, pts, pw = r.inp("x", x), r.inp("target", tgt), r.inp("targetSize", ts), r.inp("grad", w)
        r.ok(lib.w2l_batch_ctc_target_size(B, L, T, pt, r.out("targetSize_dev", (B,), I32), _stream()), "target size")
        ws = r.work("ws", lib.w2l_ctc_workspace_size(B, T, N, L))
        r.ok(lib.w2l_ctc_forward(B, T, N, L, 4, px, pt, pts, r.out("loss", (B,)), ws, _stream()), "forward")
        r.ok(lib.w2l_ctc_backward(B, T, N, L, px, pt, pts, pw, r.out("dx", (B, T, N)), ws, _stream()), "backward")
        r.ok(lib.w2l_ctc_viterbi(B, T, N, px, r.out("greedy", (B, T), I32), _stream()), "viterbi")
        r.ok(lib.w2l_ctc_score(B, T, N, L, 4, px, pt, pts, r.out("score_loss", (B,)), r.out("score_path", (B, T), I32),
                               r.work("score_ws", lib.w2l_ctc_score_workspace_size(B, T, N, L)), _stream()), "score")
        r.ok(lib.w2l_ctc_align(B, T, N, L, px, pt, pts, r.inp("frames", frames), r.out("align_path", (B, T), I32), r.out("align_score", (B,)),
                               r.work("align_ws", lib.w2l_ctc_align_workspace_size(B, T, N, L)), _stream()), "align")

        def ref():
            o = pyoracle.CTC(x, tgt, scale_mode=4)
            loss = o.forward()
            dx = o.backward(w.astype(np.float64))
            paths, score = ctc_align_ref(x, tgt, frames)
            greedy = pyoracle.ctc_viterbi(x)
            return {"targetSize_dev": ("exact", ts), "loss": ("loss", loss), "dx": ("rel", dx), "greedy": ("exact", greedy),
                    "score_loss": ("loss", loss), "score_path": ("exact", greedy), "align_path": ("exact", paths),
                    "align_score": ("each", score)}
        return ref


_ctc_case(3, 8, 3, 4)
_ctc_case(2, 50, 1000, 40)
_ctc_case(2, 300, 12, 260, long_row=True)      # L past 255: the linear-domain lattice changes there


def _fcc_case(B, T, N):
    @case(f"fcc/B={B},T={T},N={N}")
    def _(r):
        from oracle import pyoracle
        lib = r.L
        rng = np.random.default_rng(B * 1000 + T * 10 + N)
        x = (rng.normal(size=(B, T, N)) * 1.5).astype(np.float32)
        A = rng.normal(size=(N, N)).astype(np.float32)
        ts = np.array([1 + b for b in range(B)], np.int32)
        w = rng.normal(size=B).astype(np.float32)
        px, pA = r.inp("x", x), r.inp("trans", A)
        ws = r.work("ws", lib.w2l_fcc_workspace_size(B, T, N))
        r.ok(lib.w2l_fcc_forward(B, T, N, 4, px, r.inp("targetSize", ts), pA, r.out("loss", (B,)), ws, _stream()), "forward")
        r.ok(lib.w2l_fcc_backward(B, T, N, pA, r.inp("grad", w), r.out("dx", (B, T, N)), r.out("dtrans", (N, N)), ws, _stream()), "backward")
        r.ok(lib.w2l_fcc_range_flags(B, T, N, ws, r.out("flags", (B,), I32), _stream()), "flags")
        r.ok(lib.w2l_viterbi_compute(B, T, N, px, pA, r.out("path", (B, T), I32), r.work("vit_ws", lib.w2l_viterbi_workspace_size(B, T, N)),
                                     _stream()), "viterbi")

        def ref():
            o = pyoracle.FCC(x, A, ts, 4)
            loss = o.forward()
            dx, dA = o.backward(w.astype(np.float64))
            return {"loss": ("loss", loss), "dx": ("rel", dx), "dtrans": ("rel", dA), "path": ("exact", pyoracle.viterbi(x, A)),
                    "flags": ("none", "which utterances took the log-domain path is the scans' internal range decision, a diagnostic without a restatement")}
        return ref


for _N in (5, 33, 70):
    _fcc_case(2, 9, _N)
_fcc_case(3, 1, 2)


def _fac_asg_case(B, T, N, L):
    @case(f"fac_asg/B={B},T={T},N={N},L={L}")
    def _(r):
        from oracle import pyoracle
        lib = r.L
        rng = np.random.default_rng(L * 7 + T)
        x = (rng.normal(size=(B, T, N)) * 1.5).astype(np.float32)
        A = rng.normal(size=(N, N)).astype(np.float32)
        tgt = _targets(rng, B, L, N, T)
        tgt[0, :min(L, T)] = rng.integers(0, N, size=min(L, T))
        w = rng.normal(size=B).astype(np.float32)
        ts = pyoracle.batch_target_size(tgt, T)
        px, pA, pt, pts, pw = r.inp("x", x), r.inp("trans", A), r.inp("target", tgt), r.inp("targetSize", ts), r.inp("grad", w)
        r.ok(lib.w2l_batch_target_size(B, L, T, pt, r.out("targetSize_dev", (B,), I32), _stream()), "target size")
        ws = r.work("fac_ws", lib.w2l_fac_workspace_size(B, T, N, L))
        r.ok(lib.w2l_fac_forward(B, T, N, L, 4, px, pt, pts, pA, r.out("fac_loss", (B,)), ws, _stream()), "fac forward")
        r.ok(lib.w2l_fac_backward(B, T, N, L, pt, pts, pw, r.out("fac_dx", (B, T, N)), r.out("fac_dtrans", (N, N)), ws, _stream()), "fac backward")
        r.ok(lib.w2l_fac_range_flags(B, T, N, L, ws, r.out("fac_flags", (B,), I32), _stream()), "fac flags")
        r.ok(lib.w2l_fac_viterbi(B, T, N, L, px, pt, pts, pA, r.out("fac_path", (B, T), I32),
                                 r.work("facv_ws", lib.w2l_fac_workspace_size(B, T, N, L)), _stream()), "fac viterbi")
        assert lib.w2l_asg_workspace_size(B, T, N, L) > 0
        aws = r.work("asg_ws", lib.w2l_asg_workspace_size(B, T, N, L))
        r.ok(lib.w2l_asg_forward(B, T, N, L, 4, px, pt, pA, r.out("asg_loss", (B,)), aws, _stream()), "asg forward")
        r.ok(lib.w2l_asg_backward(B, T, N, L, pt, pA, pw, r.out("asg_dx", (B, T, N)), r.out("asg_dtrans", (N, N)), aws, _stream()), "asg backward")

        def ref():
            o = pyoracle.FAC(x, A, tgt, scale_mode=4)
            loss = o.forward()
            dx, dA = o.backward(w.astype(np.float64))
            al, adx, adA = pyoracle.asg(x, A, tgt, 4, w.astype(np.float64))
            return {"targetSize_dev": ("exact", ts), "fac_loss": ("loss", loss), "fac_dx": ("rel", dx), "fac_dtrans": ("rel", dA),
                    "fac_path": ("exact", o.viterbi()), "fac_flags": ("none", "which utterances took the log-domain path is the scans' internal range decision, a diagnostic without a restatement"),
                    "asg_loss": ("loss", al), "asg_dx": ("rel", adx), "asg_dtrans": ("rel", adA)}
        return ref


_fac_asg_case(3, 6, 4, 3)
_fac_asg_case(2, 40, 30, 40)
_fac_asg_case(2, 17, 33, 9)


@case("linseg/B=3,T=50,N=6,L=9")
def _(r):
    from oracle import pyoracle
    lib = r.L
    B, T, N, L = 3, 50, 6, 9
    rng = np.random.default_rng(59)
    x = (rng.normal(size=(B, T, N)) * 1.5).astype(np.float32)
    A = rng.normal(size=(N, N)).astype(np.float32)
    tgt = _targets(rng, B, L, N, T)
    w = rng.normal(size=B).astype(np.float32)
    lin = pyoracle.linear_target(tgt, T)
    r.ok(lib.w2l_linear_target(B, L, T, r.inp("target", tgt), r.out("lin_dev", (B, T), I32), _stream()), "linear target")
    plin = r.inp("lin", lin)
    r.ok(lib.w2l_fac_fullpath_forward(B, T, N, 4, r.inp("x", x), plin, r.inp("trans", A), r.out("loss", (B,)), _stream()), "forward")
    r.ok(lib.w2l_fac_fullpath_backward(B, T, N, 4, plin, r.inp("grad", w), r.out("dx", (B, T, N)), r.out("dtrans", (N, N)), _stream()), "backward")

    def ref():
        o = pyoracle.FAC(x, A, lin, scale_mode=4)
        loss = o.forward()
        dx, dA = o.backward(w.astype(np.float64))
        return {"lin_dev": ("exact", lin), "loss": ("loss", loss), "dx": ("rel", dx), "dtrans": ("rel", dA)}
    return ref


# ---- attention: the unfused softmax, the batched products, the pool, the key lengths ------------------------------------------------
def _softmax_case(B, H, T, d, csz, ld_pad, ragged):
    @case(f"attn_softmax/B={B},H={H},T={T},d={d},csz={csz},ldr+{ld_pad}" + (",keyLen" if ragged else ""))
    def _(r):
        lib = r.L
        rng = np.random.default_rng(T * 10 + csz)
        n0 = csz - 1
        rlo = max(0, n0 - (T - 1))
        W = min(2 * csz - 1, n0 + T) - rlo
        ldr = (W + 3) // 4 * 4 + ld_pad
        scale = float(1.0 / np.sqrt(d))
        S = rng.normal(size=(B, H, T, T)).astype(np.float32)
        Rm = rng.normal(size=(B * T * H, W)).astype(np.float32)
        dP = rng.normal(size=(B, H, T, T)).astype(np.float32)
        kl = np.array([max(1, T - 2 * b - 1) for b in range(B)], np.int32)
        pP = r.inout("P", S)
        r.ok(lib.w2l_attn_softmax_forward(pP, r.inp("R", Rm, ld=ldr), r.inp("keyLen", kl) if ragged else None, B, H, T, ldr, rlo, W, n0, scale,
                                          _stream()), "forward")
        r.ok(lib.w2l_attn_softmax_backward(pP, r.inout("dS", dP), r.out("dR", (B * T * H, ldr)), B, H, T, ldr, rlo, W, n0, scale,
                                           _stream()), "backward")
        r.ok(lib.w2l_attn_softmax_forward(r.inout("P_plain", S), None, None, B, H, T, 0, 0, 0, 0, scale, _stream()), "plain")

        def ref():
            R4 = Rm.astype(np.float64).reshape(B, T, H, W)
            skew = np.zeros((B, H, T, T))
            idx = np.zeros((T, T), np.int64) - 1
            for i in range(T):
                for j in range(T):
                    wcol = j - i + n0 - rlo
                    if 0 <= wcol < W:
                        skew[:, :, i, j] = R4[:, i, :, wcol]
                        idx[i, j] = wcol
            z = scale * (S.astype(np.float64) + skew)
            if ragged:
                for b in range(B):
                    z[b, :, :, kl[b]:] = -np.inf
            z -= z.max(-1, keepdims=True)
            P = np.exp(z)
            P /= P.sum(-1, keepdims=True)
            PdP = P * dP
            dS = scale * (PdP - P * PdP.sum(-1, keepdims=True))
            dR = np.zeros((B, T, H, ldr))      # the header: every column up to ldr is written, zeros beyond W
            for i in range(T):
                for j in range(T):
                    if idx[i, j] >= 0:
                        dR[:, i, :, idx[i, j]] = dS[:, :, i, j]
            z0 = scale * S.astype(np.float64)
            P0 = np.exp(z0 - z0.max(-1, keepdims=True))
            return {"P": ("rel", P), "dS": ("rel", dS), "dR": ("rel", dR.reshape(B * T * H, ldr)), "P_plain": ("rel", P0 / P0.sum(-1, keepdims=True))}
        return ref


for _shape in ((2, 2, 5, 4, 3), (1, 2, 33, 8, 40)):
    for _pad in (0, 4):
        for _ragged in (False, True):
            _softmax_case(*_shape, _pad, _ragged)


def _bgemm_case(B, H, T, d, bf16):
    @case(f"bgemm_{'bf16' if bf16 else 'f32'}/B={B},H={H},T={T},d={d},ldc+4")
    def _(r):
        lib = r.L
        fn = lib.w2l_bgemm_bf16 if bf16 else lib.w2l_bgemm_f32
        g = torch.Generator().manual_seed(B * 1000 + T)
        Cc, ldS, ldX = H * d, T + 4, H * d + 4
        q, k = torch.randn(B, T, Cc, generator=g), torch.randn(B, T, Cc, generator=g)
        P, dv0 = torch.randn(B, H, T, T, generator=g), torch.randn(B, T, Cc, generator=g)
        pq, pk = r.inp("q", q.numpy(), ld=ldX), r.inp("k", k.numpy(), ld=ldX)
        pPm = r.inp("P", P.numpy(), ld=ldS)
        TX, TS = T * ldX, T * ldS
        D = _lib.BgemmDesc(M=T, N=T, K=d, G1=B, G2=H, sam=ldX, sak=1, a1=TX, a2=d, sbk=1, sbn=ldX, b1=TX, b2=d, ldc=ldS, c1=H * TS, c2=TS)
        r.ok(fn(C.byref(D), pq, pk, r.out("S", (B, H, T, T), ld=ldS), _stream()), "q k^T")
        D = _lib.BgemmDesc(M=T, N=d, K=T, G1=B, G2=H, sam=ldS, sak=1, a1=H * TS, a2=TS, sbk=ldX, sbn=1, b1=TX, b2=d, ldc=ldX, c1=TX, c2=d)
        r.ok(fn(C.byref(D), pPm, pk, r.out("ctx", (B, T, Cc), ld=ldX), _stream()), "P v")
        D = _lib.BgemmDesc(M=T, N=d, K=T, G1=B, G2=H, sam=1, sak=ldS, a1=H * TS, a2=TS, sbk=ldX, sbn=1, b1=TX, b2=d, ldc=ldX, c1=TX, c2=d,
                           accumulate=1)
        r.ok(fn(C.byref(D), pPm, pq, r.inout("dv", dv0.numpy(), ld=ldX), _stream()), "P^T q accumulate")

        def ref():
            rd = (lambda t: t.bfloat16().double()) if bf16 else (lambda t: t.double())
            qh = rd(q).reshape(B, T, H, d).permute(0, 2, 1, 3)
            kh = rd(k).reshape(B, T, H, d).permute(0, 2, 1, 3)
            bar = ("rel", 2e-5) if bf16 else "rel"       # tests/test_gpu_attention.py
            return {"S": (bar, (qh @ kh.transpose(-1, -2)).numpy()), "ctx": (bar, (rd(P) @ kh).permute(0, 2, 1, 3).reshape(B, T, Cc).numpy()),
                    "dv": (bar, (dv0.double() + (rd(P).transpose(-1, -2) @ qh).permute(0, 2, 1, 3).reshape(B, T, Cc)).numpy())}
        return ref


for _bf in (False, True):
    _bgemm_case(2, 1, 5, 4, _bf)
    _bgemm_case(2, 3, 47, 8, _bf)



# ---- fused attention ---------------------------------------------------------------------------------------------------------------
def _fused_attention_case(B, H, T, d, csz, p, ragged):
    @case(f"attn_fused/B={B},H={H},T={T},d={d},csz={csz},p={p}" + (",keyLen" if ragged else ""))
    def _(r):
        from oracle import transformer_oracle as TO
        lib = r.L
        g = torch.Generator().manual_seed(T * 7 + d + csz)
        Cc = H * d
        q, k, v, dctx = (torch.randn(B, T, Cc, generator=g) for _ in range(4))
        E = torch.randn(max(1, 2 * csz - 1), d, generator=g) * 0.5
        n0 = csz - 1
        rlo = max(0, n0 - (T - 1)) if csz else 0
        W = (min(2 * csz - 1, n0 + T) - rlo) if csz else 0
        scale = float(1.0 / np.sqrt(d))
        kl = np.array([T] + [max(1, (T * (3 + b)) // (5 + b)) for b in range(1, B)], np.int32)
        if ragged and B == 1:
            kl[0] = max(1, (3 * T) // 5)
        D = _lib.AttnFusedDesc(B=B, H=H, T=T, d=d, ld=Cc, ldc=Cc, W=W, n0=n0, rlo=rlo, scale=scale, dropP=p, dropSeed=4321, dropStream=5)
        pq, pk, pv = r.inp("q", q.numpy()), r.inp("k", k.numpy()), r.inp("v", v.numpy())
        pE = r.inp("posTable", E.numpy()) if csz else None
        pP = r.out("P", (B, H, T, T))
        pPd = r.out("Pd", (B, H, T, T)) if p > 0 else None
        r.ok(lib.w2l_attn_fused_forward(C.byref(D), pq, pk, pv, pE, r.inp("keyLen", kl) if ragged else None, pP, pPd, r.out("ctx", (B, T, Cc)),
                                        _stream()), "forward")
        nws = lib.w2l_attn_fused_backward_workspace(C.byref(D), 1 if csz else 0)
        assert nws > 0
        ws = r.work("ws", nws)
        r.ok(lib.w2l_attn_fused_backward(C.byref(D), pq, pk, pv, pE, pP, r.inp("dctx", dctx.numpy()), r.out("dq", (B, T, Cc)), r.out("dk", (B, T, Cc)),
                                         r.out("dv", (B, T, Cc)), r.out("dPosTable", (2 * csz - 1, d)) if csz else None, ws, nws, _stream()), "backward")
        got = {key: r.view(key) for key in (("P", "Pd", "ws") if p > 0 else ("P", "ws"))}

        def ref():   # tests/test_gpu_attention.py: float64 on the bf16-rounded operands, 2e-5; ctx and the gradients from the kernel's own P / dS
            rd = lambda x: x.bfloat16().double()
            heads = lambda x: x.reshape(B, T, H, d).permute(0, 2, 1, 3)
            unheads = lambda x: x.permute(0, 2, 1, 3).reshape(B, T, Cc)
            qh, kh, vh, dch = heads(rd(q)), heads(rd(k)), heads(rd(v)), heads(rd(dctx))
            S = qh @ kh.transpose(-1, -2)
            if csz:
                S = S + TO.relative_position_rotate(qh @ rd(E).t())[..., E.shape[0] // 2:E.shape[0] // 2 + T]
            S = S * scale
            if ragged:
                S = S.masked_fill(torch.arange(T)[None, None, None, :] >= torch.from_numpy(kl).long()[:, None, None, None], float("-inf"))
            Pk = got["P"].cpu()
            Pdk = got["Pd"].cpu() if p > 0 else Pk
            bar = ("rel", 2e-5)
            out = {"P": (bar, torch.softmax(S, dim=-1).numpy()), "ctx": (bar, unheads(rd(Pdk) @ vh).numpy())}
            if p > 0:   # tests/test_gpu_attention.py: the keep pattern and scaling of w2l_dropout_copy over the kernel's own P, bit for bit
                from oracle import pyoracle
                out["Pd"] = ("exact", pyoracle.dropout(Pk.numpy().reshape(-1), p, 4321, 5).reshape(B, H, T, T))
            nt = (T + 31) // 32
            TP = 32 * (2 if nt <= 2 else 4 if nt <= 4 else 6)
            img = got["ws"].cpu()[:2 * B * H * TP * TP * 2].view(torch.bfloat16).view(2, B, H, TP, TP)
            dSk = img[0, :, :, :T, :T].transpose(-1, -2).double()
            dP = dch @ vh.transpose(-1, -2)
            if p > 0:
                dP = dP * (Pdk != 0).double() / (1.0 - p)
            P64 = Pk.double()
            dS64 = scale * P64 * (dP - (P64 * dP).sum(-1, keepdim=True))
            meets(("rel", 4.2e-3), dSk.numpy(), dS64.numpy(), "dS image at the head of the workspace")
            dq_ref, dk_ref, dv_ref = dSk @ kh, dSk.transpose(-1, -2) @ qh, rd(Pdk).transpose(-1, -2) @ dch
            if csz:
                dE_ref, Er = torch.zeros(2 * csz - 1, d, dtype=torch.float64), rd(E)
                for delta in range(-(T - 1), T):
                    w = delta + n0
                    if 0 <= w < 2 * csz - 1:
                        diag = dSk.diagonal(offset=delta, dim1=-2, dim2=-1)
                        lo, n = max(0, -delta), diag.shape[-1]
                        dq_ref[:, :, lo:lo + n] += diag[..., None] * Er[w]
                        dE_ref[w] += (diag[..., None] * qh[:, :, lo:lo + n]).sum((0, 1, 2))
                out["dPosTable"] = (bar, dE_ref.numpy())
            out.update({"dq": (bar, unheads(dq_ref).numpy()), "dk": (bar, unheads(dk_ref).numpy()), "dv": (bar, unheads(dv_ref).numpy())})
            return out
        return ref


_fused_attention_case(3, 1, 1, 32, 2, 0.0, False)
_fused_attention_case(2, 2, 33, 32, 0, 0.0, True)
_fused_attention_case(2, 2, 33, 32, 7, 0.2, False)
_fused_attention_case(1, 2, 190, 32, 40, 0.2, True)
_fused_attention_case(2, 1, 190, 32, 0, 0.0, False)


def _pool_case(B, T, F, w, stride):
    @case(f"pool_time/B={B},T={T},F={F},w={w},stride={stride}")
    def _(r):
        rng = np.random.default_rng(T + F)
        To = (T - w) // stride + 1
        x = rng.normal(size=(B, T, F)).astype(np.float32)
        dy = rng.normal(size=(B, To, F)).astype(np.float32)
        px = r.inp("x", x)
        r.ok(r.L.w2l_pool_time_forward(px, r.out("y", (B, To, F)), B, T, F, w, stride, _stream()), "forward")
        r.ok(r.L.w2l_pool_time_backward(px, r.inp("dy", dy), r.out("dx", (B, T, F)), B, T, F, w, stride, _stream()), "backward")

        def ref():
            y, dx = np.zeros((B, To, F)), np.zeros((B, T, F))
            for t in range(To):
                win = x[:, t * stride:t * stride + w]
                y[:, t] = win.max(1)
                first = win.argmax(1)              # the first maximum of the window
                for b in range(B):
                    dx[b, t * stride + first[b], np.arange(F)] += dy[b, t]
            return {"y": ("exact", y), "dx": ("rel", dx)}
        return ref


_pool_case(2, 9, 5, 2, 2)
_pool_case(1, 33, 70, 3, 2)


@case("attn_key_lengths")
def _(r):
    from oracle import transformer_oracle as TO
    B, Tin, Tk = 4, 37, 13
    sizes = np.array([37.0, 20.0, 1.0, 29.5], np.float32)
    full = np.array([50.0], np.float32)
    ps = r.inp("sizes", sizes)
    r.ok(r.L.w2l_attn_key_lengths(ps, B, Tin, Tk, r.out("keyLen", (B,), I32), _stream()), "key lengths")
    r.ok(r.L.w2l_attn_key_lengths_full(ps, r.inp("full", full), B, Tin, Tk, r.out("keyLen_full", (B,), I32), _stream()), "key lengths full")

    def ref():   # oracle/transformer_oracle.py key_lengths, with *fullSize in the place of the largest size
        nb = np.ceil(sizes * np.float32(Tin) / full[0])
        xs_ = (np.arange(Tk, dtype=np.float32) * (np.float32(Tin) / np.float32(Tk))).astype(np.float32)
        lo = np.floor(xs_)
        src = np.minimum(lo + ((xs_ - lo) >= 0.5), Tin - 1)
        return {"keyLen": ("exact", np.asarray(TO.key_lengths(sizes, Tin, Tk))),
                "keyLen_full": ("exact", (src[None, :] < nb[:, None]).sum(axis=1).astype(np.int32))}
    return ref


# ---- bf16 operand path ----------------------------------------------------------------------------------------------------------------
def pad64(n):
    return (n + 63) // 64 * 64


def bf16_bits(x):
    """fp32 -> bf16 bits as int16 (round to nearest even: torch's conversion, the reference of tests/test_gpu_nn.py)"""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).bfloat16().view(torch.int16).numpy()


def bf16_val(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).bfloat16().double().numpy()


def image_of(x, ld):
    out = np.zeros((x.shape[0], ld), np.int16)
    out[:, :x.shape[1]] = bf16_bits(x)
    return out


def _convert_case(rows, cols, ldx_pad):
    @case(f"bf16_convert/{rows}x{cols}/ldx+{ldx_pad}")
    def _(r):
        from oracle import pyoracle
        lib = r.L
        g = torch.Generator().manual_seed(rows * 31 + cols)
        x = (torch.randn(rows, cols, generator=g) * 10.0 ** torch.randint(-3, 4, (rows, cols), generator=g)).numpy()
        ldx, ldR, ldT = cols + ldx_pad, pad64(cols), pad64(rows)
        px = r.inp("x", x, ld=ldx)
        r.ok(lib.w2l_bf16_convert(px, rows, cols, ldx, r.out("rows", (rows, ldR), I16), ldR, r.out("trans", (cols, ldT), I16), ldT, _stream()), "both")
        r.ok(lib.w2l_bf16_convert(px, rows, cols, ldx, r.out("rows_alone", (rows, ldR), I16), ldR, None, 0, _stream()), "rows")
        r.ok(lib.w2l_bf16_convert(px, rows, cols, ldx, None, 0, r.out("trans_alone", (cols, ldT), I16), ldT, _stream()), "trans")
        r.ok(lib.w2l_bf16_convert_dropout(px, rows, cols, ldx, r.out("rows_drop", (rows, ldR), I16), ldR, r.out("trans_drop", (cols, ldT), I16), ldT,
                                          0.25, 77, 5, _stream()), "dropout")
        arr = (_lib.Bf16ConvertDesc * 2)()
        arr[0] = _lib.Bf16ConvertDesc(x=px, rows=rows, cols=cols, ldx=ldx, rowMajor=r.out("multi_rows", (rows, ldR), I16), ldRows=ldR,
                                      transposed=r.out("multi_trans", (cols, ldT), I16), ldTrans=ldT)
        arr[1] = _lib.Bf16ConvertDesc(x=px, rows=rows, cols=cols, ldx=ldx, rowMajor=r.out("multi_rows2", (rows, ldR), I16), ldRows=ldR,
                                      transposed=None, ldTrans=0)
        r.ok(lib.w2l_bf16_convert_multi(2, arr, _stream()), "multi")

        def ref():
            rm, tr = image_of(x, ldR), image_of(x.T, ldT)
            dense = np.zeros((rows, ldx), np.float32)      # the mask of w2l_dropout_copy over the dense [rows][ldx] matrix
            dense[:, :cols] = x
            xd = pyoracle.dropout(dense.reshape(-1), 0.25, 77, 5).reshape(rows, ldx)[:, :cols]
            return {"rows": ("exact", rm), "trans": ("exact", tr), "rows_alone": ("exact", rm), "trans_alone": ("exact", tr),
                    "multi_rows": ("exact", rm), "multi_trans": ("exact", tr), "multi_rows2": ("exact", rm),
                    "rows_drop": ("exact", image_of(xd, ldR)), "trans_drop": ("exact", image_of(xd.T, ldT))}
        return ref


for _rows, _cols in ((1, 1), (5, 3), (70, 130)):
    _convert_case(_rows, _cols, 0)
    _convert_case(_rows, _cols, 5)


def _gemm_bf16_operands(M, N, K):
    rng = np.random.default_rng(M * 7919 + N * 104729 + K)
    A, B = rng.normal(size=(M, K)).astype(np.float32), (rng.normal(size=(N, K)) / np.sqrt(K)).astype(np.float32)
    bias, add = rng.normal(size=N).astype(np.float32), rng.normal(size=(M, N)).astype(np.float32)
    a, b = bf16_val(A), bf16_val(B)
    return A, B, bias, add, a @ b.T, np.abs(a) @ np.abs(b).T


def _bound(K, mag, *others):
    """tests/test_gpu_gemm_smallm.py: |got - ref| <= (K + 2) 2^-24 (sum |a||b| + |bias| + |addend|) for any summation order"""
    return ("bound", (K + 2) * 2.0 ** -24 * (mag + sum(np.abs(o) for o in others)))


def _gemm_bf16_case(M, N, K):
    @case(f"gemm_bf16/{M}x{N}x{K}")
    def _(r):
        lib = r.L
        A, B, bias, add, prod, mag = _gemm_bf16_operands(M, N, K)
        ld = pad64(K)
        pA, pB, pbias, padd = r.inp("A", image_of(A, ld)), r.inp("B", image_of(B, ld)), r.inp("bias", bias), r.inp("addend", add)
        ldc = N + 4
        r.ok(lib.w2l_gemm_bf16(M, N, K, pA, ld, pB, ld, r.out("C", (M, N), ld=ldc), ldc, None, 0, None, _stream()), "plain, ldc above natural")
        r.ok(lib.w2l_gemm_bf16(M, N, K, pA, ld, pB, ld, r.out("C_bias_relu", (M, N)), N, pbias, 1, None, _stream()), "bias relu")
        e = _lib.GemmEpilogue(None, 1.0, padd, 0, 0.0, 0, 0)
        r.ok(lib.w2l_gemm_bf16(M, N, K, pA, ld, pB, ld, r.out("C_add", (M, N)), N, pbias, 0, C.byref(e), _stream()), "addend")
        e2 = _lib.GemmEpilogue(None, 1.0, None, 1, 0.0, 0, 0)
        r.ok(lib.w2l_gemm_bf16(M, N, K, pA, ld, pB, ld, r.inout("C_acc", add), N, None, 0, C.byref(e2), _stream()), "accumulate")
        # k-major operands read in place: A stored [K][lda >= M], B stored [K][ldb >= N], leading dimensions multiples of 8
        M8, N8 = (M + 7) // 8 * 8, (N + 7) // 8 * 8
        pAt, pBt = r.inp("A_kmajor", image_of(A.T, M8)), r.inp("B_kmajor", image_of(B.T, N8))
        for ta, tb in ((1, 1), (1, 0), (0, 1)):
            r.ok(lib.w2l_gemm_bf16_ex(M, N, K, pAt if ta else pA, M8 if ta else ld, ta, pBt if tb else pB, N8 if tb else ld, tb,
                                      r.out(f"C_ex{ta}{tb}", (M, N)), N, pbias, 1, None, _stream()), f"ex {ta}{tb}")
        # two products of one shape in one launch
        pA2, pB2 = r.inp("A2", image_of(A[::-1].copy(), ld)), r.inp("B2", image_of(B[::-1].copy(), ld))     # the second group: both reversed
        arr = lambda *ps: (C.c_void_p * len(ps))(*ps)
        r.ok(lib.w2l_gemm_bf16_grouped(2, M, N, K, arr(pA, pA2), ld, arr(pB, pB2), ld, arr(r.out("C_g0", (M, N)), r.out("C_g1", (M, N))), N,
                                       arr(pbias, None), _stream()), "grouped")
        nws = lib.w2l_gemm_bf16_smallm_workspace_bytes(M, N, K)
        sink = _lib.Bf16ImageSink(r.inout("smallm_image", np.zeros((M, pad64(N)), np.int16)), pad64(N), None, 0)
        r.ok(lib.w2l_gemm_bf16_smallm(M, N, K, pA, ld, pB, ld, r.out("C_smallm", (M, N)), N, pbias, 1, padd, C.byref(sink),
                                      r.work("smallm_ws", nws), nws, _stream()), "smallm")
        got = {"C_smallm": r.view("C_smallm")}

        def ref():
            pb = prod + bias
            return {"C": (_bound(K, mag), prod), "C_bias_relu": (_bound(K, mag, bias), np.maximum(pb, 0)),
                    "C_add": (_bound(K, mag, bias, add), pb + add), "C_acc": (_bound(K, mag, add), prod + add),
                    "C_ex11": (_bound(K, mag, bias), np.maximum(pb, 0)), "C_ex10": (_bound(K, mag, bias), np.maximum(pb, 0)),
                    "C_ex01": (_bound(K, mag, bias), np.maximum(pb, 0)), "C_g0": (_bound(K, mag, bias), pb),
                    "C_g1": (_bound(K, mag[::-1, ::-1]), prod[::-1, ::-1]),
                    "C_smallm": (_bound(K, mag, bias, add), np.maximum(pb, 0) + add),
                    "smallm_image": ("exact", image_of(got["C_smallm"].cpu().numpy(), pad64(N)))}
        return ref


for _shape in ((130, 250, 70), (4, 4, 8), (31, 5, 200)):
    _gemm_bf16_case(*_shape)


def _gemm_bf16_images_case(M, N, K):
    @case(f"gemm_bf16_images/{M}x{N}x{K}")
    def _(r):
        lib = r.L
        A, B, bias, add, prod, mag = _gemm_bf16_operands(M, N, K)
        ld, ldR, ldT = pad64(K), pad64(N), pad64(M)
        pA, pB, pbias = r.inp("A", image_of(A, ld)), r.inp("B", image_of(B, ld)), r.inp("bias", bias)
        # only elements of the matrix are written: the zero padding is the caller's, so the images start zero-filled
        sink = _lib.Bf16ImageSink(r.inout("rows", np.zeros((M, ldR), np.int16)), ldR, r.inout("trans", np.zeros((N, ldT), np.int16)), ldT)
        r.ok(lib.w2l_gemm_bf16_images(M, N, K, pA, ld, pB, ld, r.out("C", (M, N)), N, pbias, 1, None, C.byref(sink), None, 0, 1.0, _stream()), "images")
        sink2 = _lib.Bf16ImageSink(r.inout("rows_alone", np.zeros((M, ldR), np.int16)), ldR, None, 0)
        r.ok(lib.w2l_gemm_bf16_images(M, N, K, pA, ld, pB, ld, None, N, pbias, 1, None, C.byref(sink2), None, 0, 1.0, _stream()), "images without C")
        got = {"C": r.view("C")}

        def ref():
            c = got["C"].cpu().numpy()
            return {"C": (_bound(K, mag, bias), np.maximum(prod + bias, 0)),
                    "rows": ("exact", image_of(c, ldR)), "trans": ("exact", image_of(c.T, ldT)), "rows_alone": ("exact", image_of(c, ldR))}
        return ref


_gemm_bf16_images_case(130, 252, 70)
_gemm_bf16_images_case(4, 4, 8)


# ---- bf16 convolutions ---------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24


def _conv_bf16_case(family, B, Cin, Cout, H, T, kw, stride, padl, padr):
    @case(f"{family}/B={B},Cin={Cin},Cout={Cout},H={H},T={T},kw={kw},s={stride},pad={padl}+{padr}")
    def _(r):
        lib = r.L
        tds = family == "tds_conv_bf16"
        rng = np.random.default_rng(1000 * Cin + T)
        To = (T + padl + padr - kw) // stride + 1
        x = rng.normal(size=(B, T, H, Cin)).astype(np.float32)
        w = (rng.normal(size=(kw, Cin, Cout)) / np.sqrt(Cin * kw)).astype(np.float32)
        b = rng.normal(size=Cout).astype(np.float32)
        dy = rng.normal(size=(B, To, H, Cout)).astype(np.float32)
        add = rng.normal(size=x.shape).astype(np.float32)
        d = _lib.ConvDesc(B, T, H, Cin, Cout, kw, stride, padl, padr)
        n_img = (lib.w2l_tds_conv_bf16_image_elems if tds else lib.w2l_conv_bf16_image_elems)(C.byref(d))
        assert n_img > 0, "the geometry must have a bf16 kernel"
        px, pw, pb, pdy, padd = r.inp("x", x), r.inp("w", w), r.inp("bias", b), r.inp("dy", dy), r.inp("add", add)
        # the weight images hold exactly *_image_elems elements (a kernel may leave padding elements of an image unwritten and unread:
        # they are buffers of the declared size here, what depends on them shows in y and dx)
        imgF, imgB = r.work("imgForward", 2 * n_img), r.work("imgBackward", 2 * n_img)
        outs = lambda: (r.out("y", dy.shape), r.out("y_relu", dy.shape), r.out("dx", x.shape), r.out("dx_add", x.shape), r.out("dw", w.shape),
                        r.out("dbias", (Cout,)))
        if tds:
            r.ok(lib.w2l_tds_conv_bf16_prepare(C.byref(d), pw, imgF, imgB, _stream()), "prepare")
            y, yr, dx, dxa, dw, db = outs()
            r.ok(lib.w2l_tds_conv_bf16_forward(C.byref(d), px, imgF, pb, y, 0, _stream()), "forward")
            r.ok(lib.w2l_tds_conv_bf16_forward(C.byref(d), px, imgF, pb, yr, 1, _stream()), "forward relu")
            r.ok(lib.w2l_tds_conv_bf16_backward_data(C.byref(d), pdy, imgB, None, dx, _stream()), "backward data")
            r.ok(lib.w2l_tds_conv_bf16_backward_data(C.byref(d), pdy, imgB, padd, dxa, _stream()), "backward data add")
            r.ok(lib.w2l_tds_conv_bf16_backward_filter_bias(C.byref(d), px, pdy, dw, db, _stream()), "backward filter bias")
            r.ok(lib.w2l_tds_conv_bf16_backward_filter(C.byref(d), px, pdy, r.out("dw_alone", w.shape), _stream()), "backward filter")
        else:
            n_scr = lib.w2l_conv_bf16_scratch_elems(C.byref(d))
            assert n_scr > 0
            scr = r.work("scratch", 2 * n_scr)
            r.ok(lib.w2l_conv_bf16_prepare(C.byref(d), pw, imgF, imgB, _stream()), "prepare")
            y, yr, dx, dxa, dw, db = outs()
            r.ok(lib.w2l_conv_bf16_forward(C.byref(d), px, imgF, pb, y, 0, scr, _stream()), "forward")
            r.ok(lib.w2l_conv_bf16_forward(C.byref(d), px, imgF, pb, yr, 1, scr, _stream()), "forward relu")
            r.ok(lib.w2l_conv_bf16_backward_data(C.byref(d), pdy, imgB, None, dx, scr, _stream()), "backward data")
            r.ok(lib.w2l_conv_bf16_backward_data(C.byref(d), pdy, imgB, padd, dxa, scr, _stream()), "backward data add")
            r.ok(lib.w2l_conv_bf16_backward_filter_bias(C.byref(d), px, pdy, dw, db, scr, _stream()), "backward filter bias")

        def ref():   # the oracle on the SAME bf16-rounded operands; the bound that holds for any summation order (tests/test_gpu_conv_bf16.py)
            f32 = lambda a: a.astype(np.float32)
            xr, wr, dyr = f32(bf16_val(x)), f32(bf16_val(w)), f32(bf16_val(dy))
            y64, dx64, dw64, db64 = _conv_ref64(xr, wr, b, dyr, stride, padl, padr)
            ay, adx, adw, adb = _conv_ref64(np.abs(xr), np.abs(wr), np.abs(b), np.abs(dyr), stride, padl, padr)
            rows = B * To * H
            by, bdx, bdw = ("bound", kw * Cin * U * ay), ("bound", kw * Cout * U * adx), ("bound", rows * U * adw)
            out = {"y": (by, y64), "y_relu": (by, np.maximum(y64, 0)), "dx": (bdx, dx64), "dx_add": (("bound", kw * Cout * U * (adx + np.abs(add))), dx64 + add),
                   "dw": (bdw, dw64), "dbias": (("bound", rows * U * adb), db64)}
            if tds:
                out["dw_alone"] = (bdw, dw64)
            return out
        return ref


_conv_bf16_case("conv_bf16", 2, 33, 32, 1, 9, 5, 1, 12, 12)
_conv_bf16_case("conv_bf16", 2, 48, 80, 1, 31, 3, 2, 1, 1)
_conv_bf16_case("conv_bf16", 3, 40, 46, 1, 37, 5, 1, 0, 0)
_conv_bf16_case("tds_conv_bf16", 1, 27, 27, 16, 5, 11, 1, 10, 0)
_conv_bf16_case("tds_conv_bf16", 2, 14, 14, 32, 64, 21, 1, 10, 10)


# ---- LayerNorm with the bf16 images of its result -------------------------------------------------------------------------------------------
def _layernorm_images_case(groups, inner, p):
    @case(f"layernorm_images/groups={groups},inner={inner},p={p}", capacity=64 << 20)
    def _(r):
        from oracle import pyoracle
        lib = r.L
        rng = np.random.default_rng(groups * 100003 + inner)
        a = np.maximum(rng.normal(size=(groups, inner)), 0).astype(np.float32)
        x = rng.normal(size=(groups, inner)).astype(np.float32)
        dy = rng.normal(size=(groups, inner)).astype(np.float32)
        gb = np.array([1.3, -0.2], np.float32)
        ldR, ldT = pad64(inner), pad64(groups)
        zr, zt = np.zeros((groups, ldR), np.int16), np.zeros((inner, ldT), np.int16)
        nd = int(lib.w2l_layernorm_scratch_doubles(groups, inner))
        pr, pgb, pmr = r.out("r", (groups, inner)), r.inp("gammaBeta", gb), r.out("meanRstd", (2 * groups,))
        ysink = _lib.Bf16ImageSink(r.inout("y_rows", zr), ldR, r.inout("y_trans", zt), ldT)
        r.ok(lib.w2l_residual_layernorm_forward_images(groups, inner, r.inout("a", a), r.inp("x", x), pr, r.out("y", (groups, inner)), pgb, 1e-5, p, 77, 5,
                                                       pmr, C.byref(ysink), _stream()), "forward")
        dsink = _lib.Bf16ImageSink(r.inout("dr_rows", zr), ldR, r.inout("dr_trans", zt), ldT)
        r.ok(lib.w2l_layernorm_backward_images(groups, inner, pr, r.inp("dy", dy), pgb, pmr, r.out("dr", (groups, inner)), r.out("dGammaBeta", (2,)),
                                               None, None, 1.0, r.work("sums", 8 * nd), C.byref(dsink), 0.0, 0, 0, _stream()), "backward")
        got = {key: r.view(key) for key in ("y", "dr")}

        def ref():
            a_drop = pyoracle.dropout(a.reshape(-1), p, 77, 5).reshape(a.shape) if p > 0 else a
            r32 = (a_drop.astype(np.float64) + x).astype(np.float32)
            odr, odg, odb = pyoracle.layernorm_bwd(r32, dy, groups, 1.3, 1e-5)
            yk, drk = got["y"].cpu().numpy(), got["dr"].cpu().numpy()
            return {"y": ("rel", np.asarray(pyoracle.layernorm_fwd(r32, groups, 1.3, -0.2, 1e-5)).reshape(groups, inner)),
                    "dr": ("rel", np.asarray(odr).reshape(groups, inner)), "a": ("exact", a_drop), "dGammaBeta": ("param", [float(odg), float(odb)]),
                    "r": (("rel", 1e-6), a_drop.astype(np.float64) + x), "meanRstd": ("rel", _mean_rstd(r32, 1e-5)),
                    "y_rows": ("exact", image_of(yk, ldR)), "y_trans": ("exact", image_of(yk.T, ldT)),
                    "dr_rows": ("exact", image_of(drk, ldR)), "dr_trans": ("exact", image_of(drk.T, ldT))}
        return ref


for _groups, _inner in ((1, 8), (5, 8), (3, 2304), (17, 1440)):
    _layernorm_images_case(_groups, _inner, 0.25)



# ---- beam searches: B = 2, T = 12, N = 6, W = K = 4 (the wide twins at W = 65), two best, label rows cut at maxLen < T ---------------
def _table(r, name, table):
    """an LM / lexicon blob as an int32 input: like every integer input its guards are zero, a stray read is no wild index"""
    raw = np.frombuffer(np.array(table.blob).tobytes(), np.uint8)
    padded = np.zeros((raw.size + 3) // 4 * 4, np.uint8)
    padded[:raw.size] = raw
    return r.inp(name, padded.view(np.int32))


def _beam_case(kind, W, wide):
    B, T, N, K, M, Lmax, MW = 2, 12, 6, 4, 2, 5, 3

    @case(f"beam/{kind}{'_wide' if wide else ''}/B={B},T={T},N={N},W={W},K={K},nbest={M},maxLen={Lmax}")
    def _(r):
        from tests.test_gpu_beam_wide import _dense_case, _lex_table, _lm_table
        lib = r.L
        frames = np.array([T, T - 3], np.int32)
        c = _dense_case(kind, 11, B, T, N, frames, hot=5, nwords=20, max_len=3)
        asg, lm, lex = kind.startswith("asg"), c.tb is not None, c.trie is not None
        fn = lambda stem: getattr(lib, stem + ("_wide" if wide else ""))
        size = {"ctc": "w2l_ctc_beam", "ctc_lm": "w2l_ctc_beam_lm", "ctc_lex": "w2l_ctc_beam_lex", "asg": "w2l_asg_beam", "asg_lm": "w2l_asg_beam",
                "asg_lex": "w2l_asg_beam_lex"}[kind]
        nws = getattr(lib, size + ("_wide" if wide else "") + "_workspace_size")(B, T, N, W, K)
        assert nws > 0
        px, pf = r.inp("x", c.x), r.inp("frames", frames)
        pA = r.inp("trans", c.A) if asg else None
        plm = _table(r, "lm", _lm_table(c.tb)) if lm else None
        plex = _table(r, "lexicon", _lex_table(c.trie)) if lex else None
        pcls = r.inp("classScore", c.cls) if c.cls is not None else None
        eos = int(c.tb.has_eos) if lm else 0
        labels, lengths, scores = r.out("labels", (B, M, Lmax), I32), r.out("lengths", (B, M), I32), r.out("scores", (B, M))
        lms = r.out("lm_scores", (B, M)) if (lm or asg) else None
        words, counts = (r.out("words", (B, M, MW), I32), r.out("word_counts", (B, M), I32)) if lex else (None, None)
        ws = r.work("ws", nws)
        head = (B, T, N, px, pf) + ((pA,) if asg else ()) + (W, K, float("inf"), 0, 0, M, Lmax)
        if lex:
            st = fn("w2l_asg_beam_search_lex" if asg else "w2l_ctc_beam_search_lex")(*head, plm, eos, c.lmw, plex, c.wsc, c.eos, labels, lengths, scores, lms,
                                                                                   MW, words, counts, ws, _stream())
        elif lm or asg:
            st = fn("w2l_asg_beam_search" if asg else "w2l_ctc_beam_search_lm")(*head, plm, eos, c.lmw if lm else 0.0, pcls, c.eos if lm else 0.0,
                                                                              labels, lengths, scores, lms, ws, _stream())
        else:
            st = fn("w2l_ctc_beam_search")(*head, labels, lengths, scores, ws, _stream())
        r.ok(st, kind)

        def ref():   # bit-exact with logAdd = 0 (the float32 restatements of tests/*_beam_ref.py)
            o = c.ref(W, K, M, Lmax, np.float32, float("inf"), False, False, MW)
            out = {key: ("exact", o[key]) for key in ("labels", "lengths", "scores", "lm_scores", "words", "word_counts") if key in o}
            if "lm_scores" not in out:      # the header: without an LM the rows are 0 for live hypotheses and -inf for empty ones
                out["lm_scores"] = ("exact", np.where(o["lengths"] >= 0, np.float32(0), np.float32(-np.inf)))
            return out
        return ref


for _kind in ("ctc", "ctc_lm", "ctc_lex", "asg", "asg_lm", "asg_lex"):
    _beam_case(_kind, 4, False)
    _beam_case(_kind, 65, True)



# ---- sessions with caller-owned state ---------------------------------------------------------------------------------------------------
@case("feat_session/toy,S=2,maxSamples=20")
def _(r):
    """w2l_feat_session_*: the state buffer has exactly w2l_feat_session_state_bytes bytes and needs no initialisation (it starts as
    the guard pattern); three steps with different chunk lengths, slot 1 idle in the first.  The features live inside the state."""
    from oracle import pyoracle
    from wav2letter_amd.features import Mfsc
    from wav2letter_amd.streaming import feat_desc
    lib = r.L
    kw = dict(num_filters=5, fs=1000, frame_ms=10, stride_ms=3)       # tests/test_gpu_feat_stream.py "toy": N = 10, St = 3, 9 bins
    fe = Mfsc(**kw)
    S, cmax, F = 2, 20, 5
    rng = np.random.default_rng(31)
    xs = [(rng.normal(size=40) * 3000.0).astype(np.float32), (rng.normal(size=31) * 3000.0).astype(np.float32)]
    plans = [[20, 7, 13], [None, 11, 20]]                              # None: the slot is idle in that step
    h = C.c_void_p(0)
    d = feat_desc(fe)
    r.ok(lib.w2l_feat_session_create(C.byref(d), S, cmax, C.byref(h)), "create")
    try:
        mo = lib.w2l_feat_session_max_out(h)
        nbytes = lib.w2l_feat_session_state_bytes(h)
        state = r.work("state", nbytes)
        r.ok(lib.w2l_feat_session_bind(h, r.inp("G", fe.G.cpu().numpy()), r.inp("H", fe.H.cpu().numpy()), state, nbytes), "bind")
        pos, frames = [0, 0], [[], []]
        for i in range(3):
            pcm = np.full((S, cmax), np.nan, np.float32)               # samples at or beyond n[s] are nobody's to read
            n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
            for s_ in range(S):
                c = plans[s_][i]
                if c is not None:
                    pcm[s_, :c] = xs[s_][pos[s_]:pos[s_] + c]
                    pos[s_] += c
                    n[s_], st[s_], fi[s_] = c, pos[s_] == c, pos[s_] == len(xs[s_])
            n_out, ptr = np.zeros(S, np.int32), C.c_void_p(0)
            r.ok(lib.w2l_feat_session_step(h, r.inp(f"pcm{i}", pcm), 0, n.ctypes.data, st.ctypes.data, fi.ctypes.data, C.byref(ptr),
                                           n_out.ctypes.data, _stream()), f"step {i}")
            torch.cuda.synchronize()
            off = ptr.value - state
            assert 0 <= off and off + 4 * S * F * mo <= nbytes
            out = r.view("state")[off:off + 4 * S * F * mo].view(F32).view(S, F, mo)
            for s_ in range(S):
                frames[s_].append(out[s_, :, :n_out[s_]].clone())
        for s_ in range(S):
            r.results[f"features{s_}"] = torch.cat(frames[s_], dim=1)
    finally:
        lib.w2l_feat_session_destroy(h)
    return lambda: {f"features{s_}": ("rel", pyoracle.mfsc(xs[s_], **kw).T) for s_ in range(S)}



def _beam_session_case(W, wide):
    S, Cm, T0, T1, N, K, M, Lmax = 2, 5, 12, 7, 6, 4, 2, 5

    @case(f"beam_session/{'wide' if wide else 'narrow'}/S={S},maxChunk={Cm},maxFrames={T0},N={N},W={W},K={K}")
    def _(r):
        """w2l_beam_session_*: state of exactly the declared bytes (it starts as the guard pattern), three steps with different chunk
        lengths and slot 1 idle in the first, one commit with a scratch of exactly w2l_beam_session_commit_bytes, then the result"""
        from tests import beam_stream_cases as BC
        from tests import ctc_beam_ref as R
        lib = r.L
        rng = np.random.default_rng(5)
        xs = [BC.peaked(rng, T0, N), BC.peaked(rng, T1, N)]
        plans = [[5, 3, 4], [0, 4, 3]]
        d = _lib.BeamSessionDesc(slots=S, maxChunk=Cm, maxFrames=T0, N=N, beam=W, beamToken=K, threshold=float("inf"), logAdd=0, normalize=0,
                                 variant=0, lm=None, lmHasEos=0, lmWeight=0.0, classScore=None, eosScore=0.0, lexicon=None, wordScore=0.0)
        h = C.c_void_p(0)
        r.ok((lib.w2l_beam_session_create_wide if wide else lib.w2l_beam_session_create)(C.byref(d), C.byref(h)), "create")
        try:
            nbytes = (lib.w2l_beam_session_wide_state_bytes if wide else lib.w2l_beam_session_state_bytes)(C.byref(d))
            r.ok(lib.w2l_beam_session_bind(h, r.work("state", nbytes), nbytes), "bind")
            pos = [0, 0]
            for i in range(3):
                em = np.full((S, Cm, N), np.nan, np.float32)              # rows at or beyond n[s] are nobody's to read
                n, st = np.zeros(S, np.int32), np.zeros(S, np.int32)
                for s_ in range(S):
                    c = plans[s_][i]
                    em[s_, :c] = xs[s_][pos[s_]:pos[s_] + c]
                    n[s_], st[s_] = c, c > 0 and pos[s_] == 0
                    pos[s_] += c
                r.ok(lib.w2l_beam_session_step(h, r.inp(f"emissions{i}", em), n.ctypes.data, st.ctypes.data, _stream()), f"step {i}")
            ncb = lib.w2l_beam_session_commit_bytes(h)
            n_lab, live = np.zeros(S, np.int32), np.zeros(S, np.int32)
            clab = r.ar.place((S, T0), I32, kind="work", name="commit_labels")[1]     # rows of slots that commit nothing are not written
            r.ok(lib.w2l_beam_session_commit(h, None, r.work("commit_scratch", ncb), ncb, T0, clab, 0, None, n_lab.ctypes.data, None,
                                             live.ctypes.data, _stream()), "commit")
            r.ok(lib.w2l_beam_session_result(h, M, Lmax, r.out("labels", (S, M, Lmax), I32), r.out("lengths", (S, M), I32), r.out("scores", (S, M)),
                                             r.out("lm_scores", (S, M)), 0, None, None, _stream()), "result")
            torch.cuda.synchronize()
            committed = [r.view("commit_labels")[s_, :n_lab[s_]].clone() for s_ in range(S)]
            r.results["committed"] = torch.cat(committed + [torch.tensor(n_lab, device="cuda")])
        finally:
            lib.w2l_beam_session_destroy(h)

        def ref():   # the never-committing search of the whole utterance (tests/ctc_beam_ref.py, bit-exact): committed labels + tail rows
            lab, ln, sc, com = np.full((S, M, Lmax), -1, np.int32), np.full((S, M), -1, np.int32), np.zeros((S, M), np.float32), []
            for s_ in range(S):
                wl, wn, ws_, _ = R.beam_search(xs[s_][None], None, W, K, float("inf"), False, False, M, xs[s_].shape[0], np.float32)
                nc = int(n_lab[s_])
                com.append(wl[0, 0, :nc])
                sc[s_] = ws_[0]
                for m in range(M):
                    if wn[0, m] >= 0:
                        assert (wl[0, m, :nc] == wl[0, 0, :nc]).all()         # stability: a prefix of every row
                        ln[s_, m] = wn[0, m] - nc
                        rest = wl[0, m, nc:wn[0, m]][:Lmax]
                        lab[s_, m, :len(rest)] = rest
            return {"labels": ("exact", lab), "lengths": ("exact", ln), "scores": ("exact", sc),
                    "lm_scores": ("exact", np.where(ln >= 0, np.float32(0), np.float32(-np.inf))),      # W2L_BEAM_PLAIN: 0 live, -inf empty
                    "committed": ("exact", np.concatenate(com + [n_lab]))}
        return ref


_beam_session_case(4, False)
_beam_session_case(65, True)



_tiny = {}


def _tiny_trainer(mixed):
    """the tiny streaming arch of tests/stream_ref.py with perturbed parameters, as an fp32 trainer (tests/test_gpu_stream.py) and as
    a mixed-precision one (tests/test_gpu_stream_bf16.py): built once each"""
    if mixed not in _tiny:
        from tests import stream_ref as SR
        from tests.test_gpu_stream_bf16 import make_trainer
        _tiny[mixed] = make_trainer(SR.TINY_ARCH, SR.NFEAT, SR.NLABEL, 5, mixed=bool(mixed))
    return _tiny[mixed]


def _stream_session_case(precision):
    S, cmax = 2, 8

    @case(f"stream_session/{'bf16' if precision else 'fp32'}/tiny,S={S},maxChunk={cmax}")
    def _(r):
        """w2l_stream_*: parameters and a state buffer of exactly w2l_stream_state_bytes in the arena (the state starts as the guard
        pattern), three steps with different chunk lengths, slot 1 idle in the first; the emissions live inside the state.  fp32: the
        trainer's own eval forward of the whole utterance at 1e-4 (tests/test_gpu_stream.py); bf16: the eval forward of the
        mixed-precision trainer at the mixed-precision bar, 2e-3 of the largest magnitude (tests/test_gpu_stream_bf16.py)."""
        from tests import stream_ref as SR
        from tests.test_gpu_stream import whole
        lib = r.L
        tr = _tiny_trainer(precision)
        nf, nl = SR.NFEAT, SR.NLABEL
        rng = np.random.default_rng(2)
        xs = [rng.normal(size=(nf, 19)).astype(np.float32), rng.normal(size=(nf, 11)).astype(np.float32)]
        plans = [[8, 3, 8], [None, 5, 6]]
        h = C.c_void_p(0)
        r.ok(lib.w2l_stream_create_ex(SR.TINY_ARCH.encode(), nf, nl, S, cmax, precision, C.byref(h)), "create")
        try:
            mo, npar, nbytes = lib.w2l_stream_max_out(h), lib.w2l_stream_param_floats(h), lib.w2l_stream_state_bytes(h)
            state = r.work("state", nbytes)
            r.ok(lib.w2l_stream_bind(h, r.inp("params", tr.params[:npar].cpu().numpy()), state, nbytes), "bind")
            pos, frames = [0, 0], [[], []]
            for i in range(3):
                x = np.full((S, nf, cmax), np.nan, np.float32)          # columns at or beyond n[s] are nobody's to read
                n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
                for s_ in range(S):
                    c = plans[s_][i]
                    if c is not None:
                        x[s_, :, :c] = xs[s_][:, pos[s_]:pos[s_] + c]
                        pos[s_] += c
                        n[s_], st[s_], fi[s_] = c, pos[s_] == c, pos[s_] == xs[s_].shape[1]
                n_out, ptr = np.zeros(S, np.int32), C.c_void_p(0)
                r.ok(lib.w2l_stream_step(h, r.inp(f"x{i}", x), n.ctypes.data, st.ctypes.data, fi.ctypes.data, C.byref(ptr), n_out.ctypes.data,
                                         _stream()), f"step {i}")
                torch.cuda.synchronize()
                off = ptr.value - state
                assert 0 <= off and off + 4 * S * mo * nl <= nbytes
                out = r.view("state")[off:off + 4 * S * mo * nl].view(F32).view(S, mo, nl)
                for s_ in range(S):
                    frames[s_].append(out[s_, :n_out[s_]].clone())
            for s_ in range(S):
                r.results[f"emissions{s_}"] = torch.cat(frames[s_])
        finally:
            lib.w2l_stream_destroy(h)
        bar = ("rel", 2e-3) if precision else "rel"
        return lambda: {f"emissions{s_}": (bar, whole(tr, xs[s_])) for s_ in range(S)}


_stream_session_case(0)
_stream_session_case(1)


@pytest.mark.parametrize("name", list(CASES))
def test_containment(name):
    run_case(name)
