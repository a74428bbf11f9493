"""Parity of the HIP sequence criteria (through the C ABI) against the CPU oracle.

Bar (BASELINE.json north_star): Viterbi paths bit-exact; loss / gradients within
1e-4 of the oracle relative to the largest reference magnitude, fp32.
"""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-4


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def relerr(got, want):
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64)
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def gradrel(got, want):
    want = np.asarray(want, np.float64)
    got = np.asarray(got, np.float64)
    return np.abs(got - want).max() / max(1e-30, np.abs(want).max())


def make_targets(rng, B, L, N, T, min_len=1, no_adjacent_repeat=False, hi=None):
    hi = N if hi is None else hi
    tgt = np.full((B, L), -1, np.int32)
    for b in range(B):
        l = int(rng.integers(min_len, min(L, T) + 1))
        y = rng.integers(0, hi, size=l)
        if no_adjacent_repeat:
            for i in range(1, l):
                while y[i] == y[i - 1]:
                    y[i] = rng.integers(0, hi)
        tgt[b, :l] = y
    return tgt


def test_wave_ops_selftest():
    from wav2letter_amd import _lib
    rng = np.random.default_rng(0)
    v = rng.normal(size=64).astype(np.float32)
    i = dev(v)
    o = torch.zeros(384, device="cuda")
    _lib.check(_lib.lib().w2l_selftest_wave_ops(i.data_ptr(), o.data_ptr(), None))
    torch.cuda.synchronize()
    o = o.cpu().numpy()
    assert (o[:64] == v.max()).all()
    assert np.allclose(o[64:128], v.astype(np.float64).sum(), rtol=1e-5, atol=1e-5)
    assert o[128] == -1 and (o[129:192] == v[:-1]).all()
    assert o[255] == -2 and (o[192:255] == v[1:]).all()
    assert o[256] == -3 and np.allclose(o[257:320], 3 * v[:-1], rtol=1e-6)
    assert (o[320:384] == v[17]).all()


@pytest.mark.parametrize("B,T,N", [(3, 1, 2), (2, 2, 5), (3, 9, 30), (2, 50, 33), (2, 17, 64), (4, 301, 30),
                                   (2, 50, 32), (2, 257, 32)])   # N = 32: the only size on fcc_*_small<32> / fcc_*_log<32> / fcc_dtrans_small<32>
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_fcc_matches_oracle(oracle, B, T, N, mode):
    from wav2letter_amd import FullConnectionCriterion
    rng = np.random.default_rng(B * 1000 + T * 10 + N)
    x = (rng.normal(size=(B, T, N)) * 1.5).astype(np.float32)
    A = rng.normal(size=(N, N)).astype(np.float32)
    tgt = make_targets(rng, B, 7, N, T)
    w = rng.normal(size=B).astype(np.float32)
    crit = FullConnectionCriterion(N, mode).cuda()
    crit.transitions.data = dev(A)
    xt = dev(x).requires_grad_(True)
    loss = crit(xt, dev(tgt))
    (loss * dev(w)).sum().backward()
    ts = oracle.batch_target_size(tgt, T)
    o = oracle.FCC(x, A, ts, mode)
    ol = o.forward()
    odx, odA = o.backward(w.astype(np.float64))
    assert relerr(loss.detach().cpu().numpy(), ol) < TOL
    assert gradrel(xt.grad.cpu().numpy(), odx) < TOL
    assert gradrel(crit.transitions.grad.cpu().numpy(), odA) < TOL


@pytest.mark.parametrize("B,T,N,L", [(3, 6, 4, 3), (2, 40, 30, 40), (3, 90, 30, 70), (2, 300, 28, 200),
                                      (2, 400, 30, 300), (2, 120, 100, 64), (2, 50, 1500, 20),
                                      # N = 33: outside the linear-domain path -- fac_fwd_blk / fac_bwd_blk in their 2 x 1, 4 x 1, 8 x 1 and 4 x 2 shapes
                                      (2, 140, 33, 100), (2, 270, 33, 200), (2, 340, 33, 300)])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_fac_matches_oracle(oracle, B, T, N, L, mode):
    from wav2letter_amd import ForceAlignmentCriterion
    rng = np.random.default_rng(L * 7 + T)
    x = (rng.normal(size=(B, T, N)) * 1.5).astype(np.float32)
    A = rng.normal(size=(N, N)).astype(np.float32)
    tgt = make_targets(rng, B, L, N, T)
    tgt[0, :min(L, T)] = rng.integers(0, N, size=min(L, T))  # one utterance with L == min(L,T)
    w = rng.normal(size=B).astype(np.float32)
    crit = ForceAlignmentCriterion(N, mode).cuda()
    crit.transitions.data = dev(A)
    xt = dev(x).requires_grad_(True)
    loss = crit(xt, dev(tgt))
    (loss * dev(w)).sum().backward()
    o = oracle.FAC(x, A, tgt, scale_mode=mode)
    ol = o.forward()
    odx, odA = o.backward(w.astype(np.float64))
    assert relerr(loss.detach().cpu().numpy(), ol) < TOL
    assert gradrel(xt.grad.cpu().numpy(), odx) < TOL
    assert gradrel(crit.transitions.grad.cpu().numpy(), odA) < TOL
    # forced alignment path: bit-exact
    p = crit.viterbiPath(dev(x), dev(tgt)).cpu().numpy()
    assert (p == o.viterbi()).all()


def test_asg_loss_librispeech_shape_slice(oracle):
    """conv_glu LibriSpeech ASG geometry (N=30, --transdiag=4, target/sqrt scaling), B reduced"""
    from wav2letter_amd import ASGLoss, CriterionScaleMode
    rng = np.random.default_rng(42)
    B, T, N, L = 4, 500, 30, 120
    x = rng.normal(size=(B, T, N)).astype(np.float32)
    tgt = make_targets(rng, B, L, 28, T, min_len=20, no_adjacent_repeat=True)
    crit = ASGLoss(N, CriterionScaleMode.TARGET_SZ_SQRT, 4.0).cuda()
    A = (np.eye(N) * 4 + rng.normal(size=(N, N)) * 0.1).astype(np.float32)
    crit.transitions.data = dev(A)
    xt = dev(x).requires_grad_(True)
    loss = crit(xt, dev(tgt))
    loss.sum().backward()
    ol, odx, odA = oracle.asg(x, A, tgt, 4)
    assert relerr(loss.detach().cpu().numpy(), ol) < TOL
    assert gradrel(xt.grad.cpu().numpy(), odx) < TOL
    assert gradrel(crit.transitions.grad.cpu().numpy(), odA) < TOL


def test_asg_full_size_identities():
    """BASELINE config 4 criterion shape (B=64,T=2000,N=30): size-independent properties
    (SURVEY App. B.6 iv, v): per-frame gradient mass and transition-gradient mass."""
    from wav2letter_amd import ForceAlignmentCriterion, FullConnectionCriterion
    rng = np.random.default_rng(4)
    B, T, N, L = 64, 2000, 30, 300
    x = dev(rng.normal(size=(B, T, N)).astype(np.float32))
    tgt = dev(make_targets(rng, B, L, 28, T, min_len=60))
    A = dev((np.eye(N) * 4 + rng.normal(size=(N, N)) * 0.1).astype(np.float32))
    for cls in (FullConnectionCriterion, ForceAlignmentCriterion):
        crit = cls(N, 0).cuda()
        crit.transitions.data = A.clone()
        xt = x.clone().requires_grad_(True)
        loss = crit(xt, tgt)
        assert torch.isfinite(loss).all()
        loss.sum().backward()
        mass = xt.grad.double().sum(-1)
        assert (mass - 1).abs().max().item() < 1e-4
        assert abs(crit.transitions.grad.double().sum().item() - B * (T - 1)) < 1e-4 * B * (T - 1)


@pytest.mark.parametrize("B,T,N", [(3, 1, 2), (2, 7, 5), (5, 60, 30), (2, 33, 64), (3, 700, 30),
                                   (3, 129, 32)])   # N = 32: viterbi_small<32>
def test_viterbi_bit_exact(oracle, B, T, N):
    from wav2letter_amd import ASGLoss
    rng = np.random.default_rng(T + N)
    x = rng.normal(size=(B, T, N)).astype(np.float32)
    A = rng.normal(size=(N, N)).astype(np.float32)
    crit = ASGLoss(N).cuda()
    crit.transitions.data = dev(A)
    got = crit.viterbiPath(dev(x)).cpu().numpy()
    assert (got == oracle.viterbi(x, A)).all()
    # heavy ties: quantised scores, first max must win exactly like the CPU scan
    xq = np.round(x * 2) / 2
    Aq = np.round(A * 2) / 2
    crit.transitions.data = dev(Aq.astype(np.float32))
    got = crit.viterbiPath(dev(xq.astype(np.float32))).cpu().numpy()
    assert (got == oracle.viterbi(xq, Aq)).all()


def test_viterbi_full_size_bit_exact(oracle):
    from wav2letter_amd import ASGLoss
    rng = np.random.default_rng(9)
    B, T, N = 64, 2000, 30
    x = rng.normal(size=(B, T, N)).astype(np.float32)
    A = (np.eye(N) * 4 + rng.normal(size=(N, N)) * 0.1).astype(np.float32)
    crit = ASGLoss(N).cuda()
    crit.transitions.data = dev(A)
    got = crit.viterbiPath(dev(x)).cpu().numpy()
    assert (got == oracle.viterbi(x, A)).all()


@pytest.mark.parametrize("B,T,N,L", [(3, 8, 3, 4), (4, 30, 29, 10), (2, 50, 1000, 40), (3, 64, 9998, 80),
                                      (2, 300, 50, 140), (2, 20, 12290, 5)])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_ctc_matches_oracle(oracle, B, T, N, L, mode):
    from wav2letter_amd import CTCLoss
    rng = np.random.default_rng(N + L)
    x = (rng.normal(size=(B, T, N)) * 2).astype(np.float32)
    tgt = make_targets(rng, B, L, N, T, hi=N - 1)
    tgt[0, :] = -1                      # empty transcription
    if L >= 4:
        tgt[1, :4] = [1, 1, 0, 0]       # repeats
    w = rng.normal(size=B).astype(np.float32)
    crit = CTCLoss(mode)
    xt = dev(x).requires_grad_(True)
    loss = crit(xt, dev(tgt))
    (loss * dev(w)).sum().backward()
    o = oracle.CTC(x, tgt, scale_mode=mode)
    ol = o.forward()
    odx = o.backward(w.astype(np.float64))
    assert relerr(loss.detach().cpu().numpy(), ol) < TOL
    assert gradrel(xt.grad.cpu().numpy(), odx) < TOL
    assert (crit.viterbiPath(dev(x)).cpu().numpy() == oracle.ctc_viterbi(x)).all()


@pytest.mark.parametrize("B,T,N,L", [(2, 700, 40, 300), (3, 640, 29, 256), (2, 1300, 30, 600), (2, 1100, 12, 1023)])
def test_ctc_long_transcriptions(oracle, B, T, N, L):
    """letter-level CTC recipes have transcriptions longer than 255 labels (round 2 refused 2L+1 > 512): 16 / 32 label
    positions per lane, up to L = 1023; every utterance of the batch uses (nearly) the whole target width, one has
    repeats that need the blank between them"""
    from wav2letter_amd import CTCLoss
    rng = np.random.default_rng(L)
    x = (rng.normal(size=(B, T, N)) * 2).astype(np.float32)
    tgt = make_targets(rng, B, L, N, T, min_len=L - 3, hi=N - 1)
    tgt[0, :L] = rng.integers(0, N - 1, size=L)
    tgt[0, 10:14] = [1, 1, 1, 0]
    w = rng.normal(size=B).astype(np.float32)
    crit = CTCLoss(4)
    xt = dev(x).requires_grad_(True)
    loss = crit(xt, dev(tgt))
    (loss * dev(w)).sum().backward()
    o = oracle.CTC(x, tgt, scale_mode=4)
    ol = o.forward()
    assert np.isfinite(ol).all()
    assert relerr(loss.detach().cpu().numpy(), ol) < TOL
    assert gradrel(xt.grad.cpu().numpy(), o.backward(w.astype(np.float64))) < TOL


def test_ctc_refuses_more_than_1023_labels():
    from wav2letter_amd import CTCLoss
    from wav2letter_amd._lib import W2LError
    x = torch.zeros(1, 1100, 5, device="cuda")
    with pytest.raises(W2LError, match="UNSUPPORTED"):
        CTCLoss()(x, torch.zeros(1, 1024, dtype=torch.int32, device="cuda"))


def test_ctc_target_longer_than_input_is_truncated(oracle):
    from wav2letter_amd import CTCLoss
    rng = np.random.default_rng(1)
    B, T, N, L = 2, 5, 6, 9
    x = rng.normal(size=(B, T, N)).astype(np.float32)
    tgt = np.array([[1, 1, 1, 1, 2, 3, 4, 0, 1], [0, 1, 2, 3, 4, 0, 1, 2, 3]], np.int32)
    loss = CTCLoss()(dev(x), dev(tgt)).cpu().numpy()
    ol = oracle.CTC(x, tgt).forward()
    assert np.isfinite(ol).all() == np.isfinite(loss).all()
    fin = np.isfinite(ol)
    assert relerr(loss[fin], ol[fin]) < TOL


def test_ctc_infeasible_forced_target_size_has_infinite_loss(oracle):
    """a caller-supplied target size the frames cannot hold (a repeat needs a blank: 3 labels with one repeat in 3 frames): the
    likelihood is exactly 0 -- loss +inf, gradient = grad * softmax, as the log-domain oracle; the utterance beside it is untouched.
    (Before round 4 a position nothing feeds inherited 2^-2^28 from a disallowed skip and the loss came out as 1.9e8:
    oracle/ctc_linear_domain.py, tests/test_ctc_linear_domain.py.)"""
    import ctypes as C
    from wav2letter_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(3)
    B, T, N, Lt = 2, 3, 7, 3
    x = rng.normal(size=(B, T, N)).astype(np.float32)
    tgt = np.array([[1, 1, 2], [1, 2, 3]], np.int32)
    ts = np.array([3, 3], np.int32)
    w = np.array([0.5, -1.25], np.float32)
    xd, td, sd, wd = dev(x), dev(tgt), dev(ts), dev(w)
    ws = torch.zeros(L.w2l_ctc_workspace_size(B, T, N, Lt), dtype=torch.uint8, device="cuda")
    loss = torch.zeros(B, device="cuda")
    dx = torch.full((B, T, N), float("nan"), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert L.w2l_ctc_forward(B, T, N, Lt, 0, xd.data_ptr(), td.data_ptr(), sd.data_ptr(), loss.data_ptr(), ws.data_ptr(), st) == 0
    assert L.w2l_ctc_backward(B, T, N, Lt, xd.data_ptr(), td.data_ptr(), sd.data_ptr(), wd.data_ptr(), dx.data_ptr(), ws.data_ptr(), st) == 0
    o = oracle.CTC(x, tgt, target_size=ts)
    ol = o.forward()
    odx = o.backward(w.astype(np.float64))
    got = loss.cpu().numpy()
    assert ol[0] == np.inf and got[0] == np.inf
    assert abs(got[1] - ol[1]) < TOL * abs(ol[1])
    assert gradrel(dx.cpu().numpy(), odx) < TOL


def test_ctc_tds_shape_full_size(oracle):
    """BASELINE config 2 criterion shape: B=32, T'=188, N=9998 word pieces + blank."""
    from wav2letter_amd import CTCLoss, CriterionScaleMode
    rng = np.random.default_rng(2)
    B, T, N, L = 32, 188, 9998, 80
    x = rng.normal(size=(B, T, N)).astype(np.float32)
    tgt = make_targets(rng, B, L, N, T, min_len=20, hi=N - 1)
    crit = CTCLoss(CriterionScaleMode.TARGET_SZ_SQRT)
    xt = dev(x).requires_grad_(True)
    loss = crit(xt, dev(tgt))
    loss.sum().backward()
    o = oracle.CTC(x, tgt, scale_mode=4)
    assert relerr(loss.detach().cpu().numpy(), o.forward()) < TOL
    assert gradrel(xt.grad.cpu().numpy(), o.backward()) < TOL
    # softmax - occupancy sums to 0 over classes for every frame
    assert xt.grad.double().sum(-1).abs().max().item() < 1e-5


def test_ctc_gradient_repeats_bit_for_bit():
    """the positions that share a gradient column (the blank at every even one, a label the target repeats) are added in a
    fixed order: the same inputs give the same gradient bits on every call, so a training run repeats exactly"""
    from wav2letter_amd import CTCLoss, CriterionScaleMode
    rng = np.random.default_rng(5)
    B, T, N, L = 32, 188, 9998, 80
    x = dev(rng.normal(size=(B, T, N)).astype(np.float32))
    tgt = dev(make_targets(rng, B, L, N, T, min_len=60, hi=40))    # 40 classes for 60 - 80 labels: every target repeats labels
    crit = CTCLoss(CriterionScaleMode.TARGET_SZ_SQRT)
    grads = []
    for _ in range(3):
        xt = x.clone().requires_grad_(True)
        crit(xt, tgt).sum().backward()
        grads.append(xt.grad)
    assert torch.isfinite(grads[0]).all()
    assert all(torch.equal(grads[0], g) for g in grads[1:])


def test_error_behaviour_mirrors_flashlight():
    from wav2letter_amd import ASGLoss, CTCLoss
    from wav2letter_amd._lib import W2LInvalidArgument
    x = torch.zeros(2, 5, 7, device="cuda")
    with pytest.raises(W2LInvalidArgument):
        CTCLoss()(x.double(), torch.zeros(2, 3, dtype=torch.int32, device="cuda"))
    with pytest.raises(W2LInvalidArgument):
        CTCLoss()(x, torch.zeros(2, 3, dtype=torch.int64, device="cuda"))
    with pytest.raises(W2LInvalidArgument):
        ASGLoss(6).cuda()(x, torch.zeros(2, 3, dtype=torch.int32, device="cuda"))


def test_criterion_timings_report():
    """not a pass/fail test: prints kernel timings at the BASELINE criterion shapes"""
    from wav2letter_amd import ASGLoss, CTCLoss, CriterionScaleMode
    rng = np.random.default_rng(0)

    def timeit(f, n=5):
        f(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    B, T, N, L = 64, 2000, 30, 300
    x = dev(rng.normal(size=(B, T, N)).astype(np.float32)).requires_grad_(True)
    tgt = dev(make_targets(rng, B, L, 28, T, min_len=60, no_adjacent_repeat=True))
    asg = ASGLoss(N, CriterionScaleMode.TARGET_SZ_SQRT, 4.0).cuda()
    f_ms = timeit(lambda: asg(x, tgt))
    fb_ms = timeit(lambda: asg(x, tgt).sum().backward())
    v_ms = timeit(lambda: asg.viterbiPath(x.detach()))
    print(f"\n[timing] ASG B={B} T={T} N={N}: fwd {f_ms:.3f} ms, fwd+bwd {fb_ms:.3f} ms, viterbi {v_ms:.3f} ms")
    B, T, N, L = 32, 188, 9998, 80
    x = dev(rng.normal(size=(B, T, N)).astype(np.float32)).requires_grad_(True)
    tgt = dev(make_targets(rng, B, L, N, T, min_len=20, hi=N - 1))
    ctc = CTCLoss(CriterionScaleMode.TARGET_SZ_SQRT)
    f_ms = timeit(lambda: ctc(x, tgt))
    fb_ms = timeit(lambda: ctc(x, tgt).sum().backward())
    gb = 12 * B * T * N / 1e9
    print(f"[timing] CTC B={B} T={T} N={N}: fwd {f_ms:.3f} ms, fwd+bwd {fb_ms:.3f} ms "
          f"({gb / (fb_ms * 1e-3):.0f} GB/s algorithmic incl. host overhead)")


# ----------------------------------------------------------------------------------------------
# large label sets (N > 64): criterion_fcc_big.hip -- packed-transition streaming MFMA recursion
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,N", [(3, 1, 70), (2, 7, 100), (5, 12, 257), (33, 5, 130), (70, 4, 96), (2, 30, 1000)])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_fcc_large_n_matches_oracle(oracle, B, T, N, mode):
    from wav2letter_amd import FullConnectionCriterion
    rng = np.random.default_rng(B * 1000 + T * 10 + N)
    x = (rng.normal(size=(B, T, N)) * 1.5).astype(np.float32)
    A = (rng.normal(size=(N, N)) + 4 * np.eye(N)).astype(np.float32)
    tgt = make_targets(rng, B, 7, N, T)
    w = rng.normal(size=B).astype(np.float32)
    crit = FullConnectionCriterion(N, mode).cuda()
    crit.transitions.data = dev(A)
    xt = dev(x).requires_grad_(True)
    loss = crit(xt, dev(tgt))
    (loss * dev(w)).sum().backward()
    ts = oracle.batch_target_size(tgt, T)
    o = oracle.FCC(x, A, ts, mode)
    ol = o.forward()
    odx, odA = o.backward(w.astype(np.float64))
    assert relerr(loss.detach().cpu().numpy(), ol) < TOL
    assert gradrel(xt.grad.cpu().numpy(), odx) < TOL
    assert gradrel(crit.transitions.grad.cpu().numpy(), odA) < TOL


def test_fcc_north_star_size_identities():
    """N = 9998 word pieces (the BASELINE stress width; T reduced so the test runs in seconds).
    Size-independent known answers: (i) A = 0  =>  FCC = sum_t LSE_n x[t][n];
    (iv) sum_n dFCC/dx[t][n] = 1 for every t; (v) sum_ij dFCC/dA[i][j] = T - 1."""
    from wav2letter_amd import FullConnectionCriterion
    B, T, N = 4, 6, 9998
    g = torch.Generator(device="cpu").manual_seed(9)
    x = torch.randn(B, T, N, generator=g) * 2
    tgt = torch.zeros(B, 3, dtype=torch.int32)
    crit = FullConnectionCriterion(N, 0).cuda()
    crit.transitions.data = torch.zeros(N, N, device="cuda")
    xt = x.cuda().requires_grad_(True)
    loss = crit(xt, tgt.cuda())
    loss.sum().backward()
    want = torch.logsumexp(x.double(), dim=2).sum(dim=1).numpy()
    assert relerr(loss.detach().cpu().numpy(), want) < 1e-5
    colsum = xt.grad.double().sum(dim=2).cpu().numpy()
    assert np.abs(colsum - 1.0).max() < 1e-4
    # with A = 0 the posterior factorises: dx[t] = softmax(x[t])
    assert gradrel(xt.grad.cpu().numpy(), torch.softmax(x.double(), dim=2).numpy()) < TOL
    assert abs(crit.transitions.grad.double().sum().item() - B * (T - 1)) < 1e-3 * B * (T - 1)
    # non-trivial transitions at full width: still a probability distribution per frame
    crit.transitions.data = (torch.randn(N, N, generator=g) * 0.1 + 4 * torch.eye(N)).cuda()
    crit.transitions.grad = None
    xt.grad = None
    loss = crit(xt, tgt.cuda())
    loss.sum().backward()
    assert np.isfinite(loss.detach().cpu().numpy()).all()
    assert np.abs(xt.grad.double().sum(dim=2).cpu().numpy() - 1.0).max() < 1e-4
    assert abs(crit.transitions.grad.double().sum().item() - B * (T - 1)) < 1e-3 * B * (T - 1)
    assert (xt.grad >= 0).all()


@pytest.mark.parametrize("B,T,N", [(1, 9, 100), (3, 40, 300), (9, 11, 129), (33, 6, 200), (2, 8, 3000)])
def test_viterbi_large_n_bit_exact(oracle, B, T, N):
    from wav2letter_amd import ASGLoss
    rng = np.random.default_rng(B + T + N)
    x = rng.normal(size=(B, T, N)).astype(np.float32)
    A = rng.normal(size=(N, N)).astype(np.float32)
    crit = ASGLoss(N, 0, 0.0).cuda()
    crit.transitions.data = dev(A)
    got = crit.viterbiPath(dev(x)).cpu().numpy()
    assert (got == oracle.viterbi(x, A)).all()
    # heavy ties: small-integer scores -> the first-max rule decides everywhere
    xq = rng.integers(-2, 3, size=(B, T, N)).astype(np.float32)
    Aq = rng.integers(-1, 2, size=(N, N)).astype(np.float32)
    crit.transitions.data = dev(Aq)
    got = crit.viterbiPath(dev(xq)).cpu().numpy()
    assert (got == oracle.viterbi(xq, Aq)).all()


@pytest.mark.parametrize("B,T,N,L,mode", [(3, 50, 6, 9, 0), (4, 333, 30, 120, 4), (2, 64, 100, 64, 3), (5, 17, 5, 40, 2)])
def test_linseg_criterion(oracle, B, T, N, L, mode):
    """LinSegCriterion (ASG on the linearly stretched target; first --linseg updates): stretched target bit-exact
    against the getLinearTarget restatement, loss / gradients within 1e-4 of the oracle's ASG on it; rows that cannot
    be stretched (empty or longer than T) contribute FCC only; run-to-run identical for letter-sized N"""
    from wav2letter_amd import LinSegCriterion, linear_target
    rng = np.random.default_rng(B * 1000 + T)
    x = rng.normal(size=(B, T, N)).astype(np.float32)
    tgt = make_targets(rng, B, L, N, 10 ** 9, min_len=1)
    tgt[0, :] = -1                                   # empty target
    if L > T:
        tgt[1, :] = rng.integers(0, N, size=L)       # longer than T
    lin = linear_target(dev(tgt), T).cpu().numpy()
    assert (lin == oracle.linear_target(tgt, T)).all()
    A = (np.eye(N) * 2 + rng.normal(size=(N, N)) * 0.3).astype(np.float32)
    crit = LinSegCriterion(N, mode).cuda()
    crit.transitions.data = dev(A)
    xt = dev(x).requires_grad_(True)
    g = rng.uniform(0.5, 1.5, size=B).astype(np.float32)
    loss = crit(xt, dev(tgt))
    (loss * dev(g)).sum().backward()
    ol, odx, odA = oracle.linseg(x, A, tgt, mode, grad=g.astype(np.float64))
    assert relerr(loss.detach().cpu().numpy(), ol) < TOL
    assert gradrel(xt.grad.cpu().numpy(), odx) < TOL
    assert gradrel(crit.transitions.grad.cpu().numpy(), odA) < TOL
    if N <= 64:
        xt2 = dev(x).requires_grad_(True)
        crit.transitions.grad = None
        (crit(xt2, dev(tgt)) * dev(g)).sum().backward()
        assert torch.equal(xt2.grad, xt.grad)


def test_linseg_shares_asg_transitions():
    """linseg->setParams(criterion->param(0), 0): one transition parameter, gradients of both criteria land on it"""
    from wav2letter_amd import ASGLoss, LinSegCriterion
    asg = ASGLoss(8, 0, 1.5).cuda()
    lin = LinSegCriterion(8, 0).cuda()
    lin.setParams(asg.transitions, 0)
    assert lin.transitions is asg.transitions
    x = torch.randn(2, 20, 8, device="cuda", requires_grad=True)
    tgt = torch.tensor([[1, 2, 3, -1], [4, 4, 5, 6]], dtype=torch.int32, device="cuda")
    lin(x, tgt).sum().backward()
    assert asg.transitions.grad is not None and torch.isfinite(asg.transitions.grad).all()
    with pytest.raises(Exception):
        lin.setParams(asg.transitions, 1)


def test_fcc_large_n_folded_step_variant_is_bit_identical():
    """W2L_FCC_FOLD=1 (probe library): the forward step epilogue folded into the transition stream -- last arriver of each
    row group, device-scope stores / loads for the cross-XCD hand-over -- gives the product's two-launch result bit for bit
    (and run to run); the product ignores the switch.  Measured slower, kept for the record"""
    import os
    from wav2letter_amd import _lib
    from wav2letter_amd.criterion import CriterionScaleMode, FullConnectionCriterion
    B, T, N = 5, 40, 1500
    g = torch.Generator(device="cpu").manual_seed(9)
    x = torch.randn(B, T, N, generator=g).cuda()
    tgt = torch.zeros(B, 4, dtype=torch.int32).cuda()
    A = (torch.randn(N, N, generator=g) * 0.3).cuda()

    def run():
        crit = FullConnectionCriterion(N, CriterionScaleMode.TARGET_SZ_SQRT).cuda()
        crit.transitions.data = A
        xx = x.clone().requires_grad_(True)
        loss = crit(xx, tgt)
        loss.sum().backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), xx.grad.clone(), crit.transitions.grad.clone()
    want = run()
    os.environ["W2L_FCC_FOLD"] = "1"
    try:
        assert all(torch.equal(a, b) for a, b in zip(run(), want))      # the product never reads the environment
        with _lib.use_probe():
            got = run()
            again = run()
    finally:
        os.environ.pop("W2L_FCC_FOLD")
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert all(torch.equal(a, b) for a, b in zip(got, again))
