"""LayerNorm held to a bar PER GROUP, on tensors whose groups differ wildly in |mean| / sigma and in scale (tests/layernorm_cases.py:
N(0, 1) next to mean +-1000, sigma 0.01 about 10, constant groups, one outlier in front): every kernel family and chunk-count edge of
w2l_residual_layernorm_forward / w2l_layernorm_backward and of the _images entry points, against the fp64 oracle.

Whole-tensor bars (rel() of tests/test_gpu_nn.py) divide by the tensor's largest magnitude and pass a group whose own values are small
at any error; N(0, 1) inputs never make var = E[r^2] - mu^2 cancel.  Here
  * y is within 1e-4 of the group's largest |y_ref - beta|, the saved rstd within 1e-4, the saved mean within half an fp32 ulp + 1e-4 sigma;
  * a constant group gives y == beta bit for bit and an rstd within 1e-6 of 1 / sqrt(eps);
  * dr and dmask are within 1e-4 of the group's largest |dr_ref|, for a dy whose scale cycles 1e-3, 1, 1e3 over the groups and for
    one of mean 100, sigma 1; dgamma within 1e-4 of sum |dy xhat_ref|, dbeta of sum |dy| (the sums' own condition scales);
  * two calls are bit-identical; the _images entry points agree with the plain ones at 2e-6 per group and their bf16 images are the
    rounding of their own fp32 result, bit for bit.
The inputs leave half the bar (floor <= 5e-5: what rounding the mean to fp32 costs) and are shown on the CPU to fail the arithmetic the
kernels had before they took their sums about a pilot (tests/test_layernorm_stats_model.py).  Every test prints its worst per-group
figures with the CPU model's beside them (-s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import layernorm_cases as LC
from oracle import layernorm_stats_model as M

pytestmark = pytest.mark.gpu
BAR = 1e-4
MASK_SCALE = 1.25


def dev(a):
    return torch.tensor(np.asarray(a)).cuda()      # (a copy: the shared inputs are read-only)


def host(t):
    return t.detach().cpu().numpy()


_built = {}


def inputs(case, oracle):
    """the case's inputs and everything derived from them on the CPU: built once, shared, never written"""
    if case.id not in _built:
        d = LC.build(case, oracle.dropout)
        d["a_after"] = d["a"] if case.p == 0 else oracle.dropout(d["a"].reshape(-1), case.p, LC.DROP_SEED, LC.DROP_STREAM).reshape(d["a"].shape)
        d["ref"] = references(d["r"], d, case, oracle)
        y, _, rstd = M.layernorm_model(d["r"], LC.GAMMA, LC.BETA, LC.EPS, case.family, "shipped")
        ey, er = LC.group_errors(y, rstd, d["r"], d["ref"]["y"])
        d["model"] = (np.where(d["const"], 0.0, ey).max(), er.max())     # the CPU model's worst group, printed beside the device's
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _built[case.id] = d
    return _built[case.id]


def references(r, d, case, oracle):
    G = case.groups
    y64, mu, rstd = LC.reference(r)
    ref = dict(y=oracle.layernorm_fwd(r, G, LC.GAMMA, LC.BETA, LC.EPS).reshape(r.shape), mu=mu, rstd=rstd,
               sigma=np.sqrt(((r.astype(np.float64) - mu[:, None]) ** 2).mean(1)))
    xhat = (r.astype(np.float64) - mu[:, None]) * rstd[:, None]
    for name in ("dy1", "dy2"):
        dy = d[name]
        dr, dg, db = oracle.layernorm_bwd(r, dy, G, LC.GAMMA, LC.EPS)
        ref[name] = dict(dr=dr.reshape(r.shape), dg=dg, db=db, dg_scale=np.abs(dy.astype(np.float64) * xhat).sum(),
                         db_scale=np.abs(dy.astype(np.float64)).sum())
    return ref


class Sink:
    """the two bf16 images with sentinel padding, as tests/test_gpu_nn.py::test_layernorm_writes_the_bf16_images_of_its_result"""

    def __init__(self, groups, inner):
        from wav2letter_amd import _lib
        self.groups, self.inner = groups, inner
        ldR, ldT = (inner + 63) // 64 * 64 + 64, (groups + 63) // 64 * 64
        self.rows = torch.full((groups, ldR), 7.0, dtype=torch.bfloat16, device="cuda")
        self.trans = torch.full((inner, ldT), 7.0, dtype=torch.bfloat16, device="cuda")
        self.c = _lib.Bf16ImageSink(rowMajor=self.rows.data_ptr(), ldRows=ldR, transposed=self.trans.data_ptr(), ldTrans=ldT)

    def check(self, want32):
        groups, inner = self.groups, self.inner
        want = want32.bfloat16()
        assert torch.equal(self.rows[:, :inner], want) and torch.equal(self.trans[:, :groups], want.t())
        assert bool((self.rows[:, inner:] == 7.0).all())
        g16 = (groups + 15) // 16 * 16
        assert bool((self.trans[:, groups:g16] == 0.0).all()) and bool((self.trans[:, g16:] == 7.0).all())


def forward(case, d, images=False):
    """one forward call in the case's call pattern -> (a after the call, r, y, meanRstd), device tensors.  plain: x = NULL and r
    stored over a (the scalar kernel refuses the alias: r apart); residual / dropout: r apart"""
    from wav2letter_amd import _lib, ops
    L = _lib.lib()
    G, n = case.groups, case.inner
    s = torch.cuda.current_stream().cuda_stream
    a = dev(d["a"])
    x = None if d["x"] is None else dev(d["x"])
    r = a if case.pattern == "plain" and case.family != "scalar" else torch.empty_like(a)
    y = torch.empty_like(a)
    mr = torch.empty(2 * G, device="cuda")
    gb = dev(np.array([LC.GAMMA, LC.BETA], np.float32))
    px = None if x is None else x.data_ptr()
    if images:
        sink = Sink(G, n)
        assert L.w2l_residual_layernorm_forward_images(G, n, a.data_ptr(), px, r.data_ptr(), y.data_ptr(), gb.data_ptr(), LC.EPS, case.p,
                                                       LC.DROP_SEED, LC.DROP_STREAM, mr.data_ptr(), C.byref(sink.c), s) == 0
        sink.check(y)
    else:
        stats = torch.empty(int(L.w2l_layernorm_scratch_doubles(G, n)), device="cuda", dtype=torch.float64)
        ops.check(L.w2l_residual_layernorm_forward(G, n, a.data_ptr(), px, r.data_ptr(), y.data_ptr(), gb.data_ptr(), LC.EPS, case.p,
                                                   LC.DROP_SEED, LC.DROP_STREAM, stats.data_ptr(), mr.data_ptr(), s), "res_ln_fwd")
    return a, r, y, mr


def backward(case, r, dy, mr, mask_src, images=False):
    """-> (dr, dmask, dGammaBeta)"""
    from wav2letter_amd import _lib, ops
    L = _lib.lib()
    G, n = case.groups, case.inner
    s = torch.cuda.current_stream().cuda_stream
    gb = dev(np.array([LC.GAMMA, LC.BETA], np.float32))
    dr = torch.empty_like(r); dm = torch.empty_like(r); dgb = torch.empty(2, device="cuda")
    if images:
        sums = torch.empty(2 * G + 64, dtype=torch.float64, device="cuda")
        sink = Sink(G, n)
        assert L.w2l_layernorm_backward_images(G, n, r.data_ptr(), dy.data_ptr(), gb.data_ptr(), mr.data_ptr(), dr.data_ptr(), dgb.data_ptr(),
                                               mask_src.data_ptr(), dm.data_ptr(), MASK_SCALE, sums.data_ptr(), C.byref(sink.c), 0.0, 0, 0, s) == 0
        sink.check(dr)
    else:
        sums = torch.empty(int(L.w2l_layernorm_scratch_doubles(G, n)), device="cuda", dtype=torch.float64)
        ops.check(L.w2l_layernorm_backward(G, n, r.data_ptr(), dy.data_ptr(), gb.data_ptr(), mr.data_ptr(), dr.data_ptr(), dgb.data_ptr(),
                                           mask_src.data_ptr(), dm.data_ptr(), MASK_SCALE, sums.data_ptr(), s), "ln_bwd")
    return dr, dm, dgb


def per_group(got, want, scale):
    """max |got - want| of every group over `scale` [G]"""
    return np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max(1) / scale


def check_case(case, oracle, images=False):
    d = inputs(case, oracle)
    G, n = case.groups, case.inner
    a, r, y, mr = forward(case, d, images)
    # the dropout pattern and the pre-norm sum: as test_residual_dropout_layernorm checks them, per group
    if case.pattern != "plain":
        assert (host(a) == d["a_after"]).all()
    rh = host(r)
    assert (per_group(rh, d["r"], np.maximum(np.abs(d["r"]).max(1), 1e-30)) < 1e-6).all()
    ref = d["ref"] if np.array_equal(rh, d["r"]) else references(rh, d, case, oracle)   # the reference takes the r the kernel returned
    yh, mrh = host(y), host(mr).reshape(G, 2)
    muf, rstd = mrh[:, 0], mrh[:, 1]
    ey, er = LC.group_errors(yh, rstd, rh, ref["y"])
    emu = np.abs(muf.astype(np.float64) - ref["mu"])
    worst = dict(y=0.0, rstd=er.max())
    for g, kind in enumerate(d["kinds"]):
        where = (case.id, g, kind)
        assert er[g] < BAR, (where, er[g])
        assert emu[g] <= 0.5 * np.spacing(np.float32(abs(ref["mu"][g]))) + BAR * ref["sigma"][g], (where, emu[g])
        if d["const"][g]:
            assert (yh[g] == np.float32(LC.BETA)).all(), where
            assert abs(float(rstd[g]) * np.sqrt(np.float64(np.float32(LC.EPS))) - 1.0) < 1e-6, (where, rstd[g])
        else:
            worst["y"] = max(worst["y"], ey[g])
            assert ey[g] < BAR, (where, ey[g], "floor", d["floor"][g])
    a2, r2, y2, mr2 = forward(case, d, images)
    assert torch.equal(y, y2) and torch.equal(mr, mr2) and torch.equal(r, r2)
    line = f"{case.id + (' [images]' if images else ''):44s} y {worst['y']:.2e} (model {d['model'][0]:.2e})  rstd {worst['rstd']:.2e} (model {d['model'][1]:.2e})"
    out = dict(r=r, y=y, mr=mr, a=a)
    if case.family != "scalar":            # (the scalar kernel is forward only)
        keep = (d["a_after"] if case.pattern != "plain" else rh) > 0
        for name in ("dy1", "dy2"):
            dy = dev(d[name])
            dr, dm, dgb = backward(case, r, dy, mr, a, images)
            b = ref[name]
            scale = np.abs(b["dr"]).max(1)
            edr = per_group(host(dr), b["dr"], scale)
            edm = per_group(host(dm), b["dr"] * keep * MASK_SCALE, scale)
            edg = abs(float(dgb[0]) - b["dg"]) / b["dg_scale"]
            edb = abs(float(dgb[1]) - b["db"]) / b["db_scale"]
            line += f"  {name}: dr {edr.max():.2e} dmask {edm.max():.2e} dgamma {edg:.2e} dbeta {edb:.2e}"
            for g, kind in enumerate(d["kinds"]):
                assert edr[g] < BAR and edm[g] < BAR, (case.id, name, g, kind, edr[g], edm[g])
            assert edg < BAR and edb < BAR, (case.id, name, edg, edb)
            dr2, dm2, dgb2 = backward(case, r, dy, mr, a, images)
            assert torch.equal(dr, dr2) and torch.equal(dm, dm2) and torch.equal(dgb, dgb2)
            out[name] = (dr, dm, dgb)
    print("\n" + line)
    return out


PLAIN_API = [c for c in LC.CASES if c.family != "images" and c.wave]
NOWAVE = [c for c in LC.CASES if not c.wave]
IMAGES = [c for c in LC.CASES if c.family == "images"]


@pytest.mark.parametrize("case", PLAIN_API, ids=lambda c: c.id)
def test_layernorm_per_group(oracle, case):
    """scalar, one wave per group, one block per group, two-level: forward, backward, determinism"""
    check_case(case, oracle)


@pytest.mark.parametrize("case", NOWAVE, ids=lambda c: c.id)
def test_layernorm_per_group_block_kernel_on_wave_sized_groups(oracle, case, monkeypatch):
    """the one-block-per-group kernels at a group the product gives to the wave kernels: probe library, W2L_LN_WAVE=0"""
    from wav2letter_amd import _lib
    monkeypatch.setenv("W2L_LN_WAVE", "0")
    with _lib.use_probe():
        check_case(case, oracle)


@pytest.mark.parametrize("case", IMAGES, ids=lambda c: c.id)
def test_layernorm_images_per_group(oracle, case):
    """the _images entry points: the same bars, their images bit for bit the rounding of their own result, and the plain entry
    points' values at 2e-6 per group"""
    img = check_case(case, oracle, images=True)
    pln = check_case(case, oracle)
    G = case.groups
    assert torch.equal(img["r"], pln["r"]) and torch.equal(img["a"], pln["a"])
    yp = host(pln["y"])
    assert (per_group(host(img["y"]), yp, np.abs(yp).max(1)) < 2e-6).all()
    mi, mp = host(img["mr"]).reshape(G, 2).astype(np.float64), host(pln["mr"]).reshape(G, 2).astype(np.float64)
    assert (np.abs(mi[:, 1] - mp[:, 1]) <= 2e-6 * mp[:, 1]).all()
    assert (np.abs(mi[:, 0] - mp[:, 0]) <= 2e-6 * (np.abs(mp[:, 0]) + 1.0 / mp[:, 1])).all()
    for name in ("dy1", "dy2"):
        (dri, dmi, dgi), (drp, dmp, dgp) = img[name], pln[name]
        scale = np.abs(host(drp)).max(1)
        assert (per_group(host(dri), host(drp), scale) < 2e-6).all() and (per_group(host(dmi), host(dmp), scale) < 2e-6).all()
        assert np.abs(host(dgi).astype(np.float64) - host(dgp)).max() <= 1e-5 * np.abs(host(dgp)).max()


@pytest.mark.parametrize("inner", [260, 2308, 8196])
def test_layernorm_on_both_sides_of_the_conditioning_threshold(oracle, inner):
    """the register-resident kernels take their sums a second time where |mean| > 8 sigma (common.hpp::ln_ill_conditioned): groups
    just below and just above, in one tensor, per group at the same bar (8196: the two-level kernel, which chooses between two pairs of sums at the same bound)"""
    from wav2letter_amd import ops
    means = np.array([7.0, -7.5, 7.9, 7.99, 8.01, -8.1, 8.5, 9.0, 64.0])
    rng = np.random.default_rng(inner)
    z = rng.normal(size=(len(means), inner))
    z = (z - z.mean(1, keepdims=True)) / z.std(1, keepdims=True)          # mean / sigma of every group as listed, up to fp32 rounding
    r = (means[:, None] + z).astype(np.float32)
    G = len(means)
    y, _, mr = ops.residual_layernorm_forward(dev(r), None, dev(np.array([LC.GAMMA, LC.BETA], np.float32)), G, LC.EPS)
    ey, er = LC.group_errors(host(y), host(mr).reshape(G, 2)[:, 1], r, oracle.layernorm_fwd(r, G, LC.GAMMA, LC.BETA, LC.EPS))
    print(f"\nconditioning threshold, inner {inner}: y {ey.max():.2e} rstd {er.max():.2e}")
    assert (LC.floor_of(r) <= LC.FLOOR_MAX).all()
    assert ey.max() < BAR and er.max() < BAR, (ey, er)


def test_weightnorm_columns_of_mixed_scale(oracle):
    """test_weightnorm_columns judges w, dv and dg over the whole matrix; here the columns of v span 1e-3 ... 1e3 and every COLUMN is
    held to 1e-4 of its own largest reference magnitude, dg[n] to 1e-4 of sum_k |v dw| / norm (its condition scale)"""
    from wav2letter_amd import ops
    K, N = 333, 77
    rng = np.random.default_rng(K + N)
    v = (rng.normal(size=(K, N)) * 10.0 ** (-3 + 6 * np.arange(N) / 76.0)).astype(np.float32)
    g = rng.uniform(0.5, 2.0, size=N).astype(np.float32)
    dw = rng.normal(size=(K, N)).astype(np.float32)
    w, norm = ops.weightnorm_forward(dev(v), dev(g))
    norm_ref = np.sqrt((v.astype(np.float64) ** 2).sum(0))
    w_ref = oracle.weightnorm_fwd(v, g, K, N, 1).reshape(K, N)
    ew = np.abs(host(w).astype(np.float64) - w_ref).max(0) / np.abs(w_ref).max(0)
    en = np.abs(host(norm) - norm_ref) / norm_ref
    dv, dg = ops.weightnorm_backward(dev(v), dev(g), norm, dev(dw))
    odv, odg = oracle.weightnorm_bwd(v, g, dw, K, N, 1)
    odv = odv.reshape(K, N)
    edv = np.abs(host(dv).astype(np.float64) - odv).max(0) / np.abs(odv).max(0)
    edg = np.abs(host(dg).astype(np.float64) - odg) / (np.abs(v.astype(np.float64) * dw).sum(0) / norm_ref)
    print(f"\nweightnorm 333 x 77, columns 1e-3 ... 1e3: w {ew.max():.2e} norm {en.max():.2e} dv {edv.max():.2e} dg {edg.max():.2e}")
    assert ew.max() < BAR and en.max() < 1e-5, (ew.max(), en.max())
    assert edv.max() < BAR and edg.max() < BAR, (edv.max(), int(edv.argmax()), edg.max(), int(edg.argmax()))
    dv2, dg2 = ops.weightnorm_backward(dev(v), dev(g), norm, dev(dw))
    assert torch.equal(dv, dv2) and torch.equal(dg, dg2)
