"""w2l_ctc_score: CTC loss and greedy path in one read of the emissions, bitwise equal to w2l_ctc_forward and w2l_ctc_viterbi
(include/w2l_hip.h).  The workspace query and the refusals are host code and run without a GPU."""
import numpy as np
import pytest
import torch

MODES = range(5)   # NONE, INPUT_SZ, INPUT_SZ_SQRT, TARGET_SZ, TARGET_SZ_SQRT


def _lib():
    from wav2letter_amd import _lib
    return _lib


def test_score_workspace_is_host_arithmetic_and_smaller_than_training():
    lib = _lib().lib()
    for B, T, N, L in [(32, 188, 9998, 80), (32, 1500, 9998, 80), (1, 1, 2, 1), (3, 37, 30, 1023), (2, 100, 12289, 500)]:
        s, f = lib.w2l_ctc_score_workspace_size(B, T, N, L), lib.w2l_ctc_workspace_size(B, T, N, L)
        assert 0 < s < f, (B, T, N, L, s, f)
        assert s >= B * T * 4 + B * T * (2 * L + 1) * 8   # lse and the label probabilities
    assert lib.w2l_ctc_score_workspace_size(0, 10, 10, 4) == 0


def test_score_refuses_bad_arguments_before_any_launch():
    L = _lib()
    lib = L.lib()
    fake = 0x1000   # never dereferenced: every refusal returns before a launch
    args = dict(B=2, T=10, N=30, L=4, mode=0, x=fake, y=fake, ts=fake, loss=fake, path=fake, ws=fake)

    def call(**kw):
        a = dict(args, **kw)
        return lib.w2l_ctc_score(a["B"], a["T"], a["N"], a["L"], a["mode"], a["x"], a["y"], a["ts"], a["loss"], a["path"], a["ws"], None)

    assert call(L=1024) == L.W2L_EUNSUPPORTED
    assert lib.w2l_ctc_forward(2, 10, 30, 1024, 0, fake, fake, fake, fake, fake, None) == L.W2L_EUNSUPPORTED
    for k in ("x", "y", "ts", "loss", "path", "ws"):
        assert call(**{k: None}) == L.W2L_EINVAL, k
    for kw in (dict(B=0), dict(T=0), dict(N=1), dict(L=0)):
        assert call(**kw) == L.W2L_EINVAL, kw


def _targets(rng, B, Lmax, N, T, full=False):
    tgt = np.full((B, Lmax), -1, np.int32)
    for b in range(B):
        n = Lmax if full or b == 0 else int(rng.integers(1, Lmax + 1))
        lab = rng.integers(0, max(N - 1, 1), n)
        if n > 3:
            lab[1] = lab[0]   # a repeated label: the lattice's no-skip case
        tgt[b, :n] = lab
    return tgt


def _both(x, tgt, ts, mode):
    """(forward loss, viterbi path, score loss, score path) on the same inputs"""
    lib = _lib().lib()
    check = _lib().check
    B, T, N = x.shape
    Lt = tgt.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(max(lib.w2l_ctc_workspace_size(B, T, N, Lt), 256), dtype=torch.uint8, device="cuda")
    wss = torch.empty(max(lib.w2l_ctc_score_workspace_size(B, T, N, Lt), 256), dtype=torch.uint8, device="cuda")
    lf = torch.full((B,), 7.0, device="cuda")
    pf = torch.full((B, T), -5, dtype=torch.int32, device="cuda")
    ls = torch.full((B,), -7.0, device="cuda")
    ps = torch.full((B, T), -9, dtype=torch.int32, device="cuda")
    check(lib.w2l_ctc_forward(B, T, N, Lt, mode, x.data_ptr(), tgt.data_ptr(), ts.data_ptr(), lf.data_ptr(), ws.data_ptr(), st), "fwd")
    check(lib.w2l_ctc_viterbi(B, T, N, x.data_ptr(), pf.data_ptr(), st), "viterbi")
    check(lib.w2l_ctc_score(B, T, N, Lt, mode, x.data_ptr(), tgt.data_ptr(), ts.data_ptr(), ls.data_ptr(), ps.data_ptr(),
                            wss.data_ptr(), st), "score")
    torch.cuda.synchronize()
    return lf.cpu(), pf.cpu(), ls.cpu(), ps.cpu()


def _assert_bitwise(lf, pf, ls, ps):
    assert torch.equal(lf.view(torch.int32), ls.view(torch.int32)), (lf, ls)
    assert torch.equal(pf, ps), (pf != ps).nonzero()[:8]


SHAPES = [  # (B, T, N): the register-resident rows (N <= 12288) and the big-row path (12289); odd N = rows of every alignment
    (1, 1, 2), (3, 37, 2), (3, 37, 30), (1, 188, 30), (3, 1500, 30), (3, 188, 257), (32, 37, 257),
    (32, 188, 9998), (2, 1500, 9998), (1, 1, 12289), (3, 37, 12289), (2, 188, 12289),
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,N", SHAPES)
def test_score_equals_forward_and_viterbi_bitwise(B, T, N):
    from wav2letter_amd import criterion as Cr
    rng = np.random.default_rng(B * 100003 + T * 101 + N)
    Lmax = max(1, min(80, T // 2))
    x = torch.tensor(rng.normal(size=(B, T, N)).astype(np.float32) * 3, device="cuda")
    tgt = torch.tensor(_targets(rng, B, Lmax, N, T), device="cuda")
    ts = Cr.batch_target_size(tgt, T, ctc=True)
    for mode in MODES:
        _assert_bitwise(*_both(x, tgt, ts, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("Lmax", [6, 80, 120, 150, 180, 250, 500, 1023])
def test_score_every_lattice_width(Lmax):
    """positions per lane P = 2, 3, 4, 5, 6, 8, 16, 32 (ctc_positions_per_lane); L = 1023 is the largest accepted"""
    from wav2letter_amd import criterion as Cr
    rng = np.random.default_rng(Lmax)
    B, N = 3, 30
    T = 2 * Lmax + 40
    x = torch.tensor(rng.normal(size=(B, T, N)).astype(np.float32), device="cuda")
    tgt = torch.tensor(_targets(rng, B, Lmax, N, T, full=Lmax == 1023), device="cuda")
    ts = Cr.batch_target_size(tgt, T, ctc=True)
    for mode in MODES:
        _assert_bitwise(*_both(x, tgt, ts, mode))


@pytest.mark.gpu
def test_score_infeasible_target_is_inf_like_forward():
    """target sizes handed in directly (batch_target_size would shorten them): a repeat-heavy target longer than the
    frames allow has likelihood 0 -- loss +inf in both passes"""
    rng = np.random.default_rng(5)
    B, T, N, Lt = 3, 6, 30, 5
    x = torch.tensor(rng.normal(size=(B, T, N)).astype(np.float32), device="cuda")
    tgt = torch.tensor([[1, 1, 1, 1, 1], [2, 3, 4, -1, -1], [7, 7, 7, 7, -1]], dtype=torch.int32, device="cuda")
    ts = torch.tensor([5, 3, 4], dtype=torch.int32, device="cuda")
    for mode in MODES:
        lf, pf, ls, ps = _both(x, tgt, ts, mode)
        _assert_bitwise(lf, pf, ls, ps)
        assert np.isinf(ls[0].item()) and ls[0].item() > 0 and np.isinf(ls[2].item()) and np.isfinite(ls[1].item())


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2, 30, 257, 9998, 12289])
def test_score_path_first_max_wins_on_exact_ties(N):
    """rows of a few distinct values (many exact ties, the max at several places: head / body / tail of rows of every
    alignment), constant rows, and rows whose max sits in the last element only"""
    from wav2letter_amd import criterion as Cr
    rng = np.random.default_rng(N)
    B, T = 3, 37
    x = rng.integers(-3, 2, size=(B, T, N)).astype(np.float32)
    x[0, 0, :] = 0.5                         # constant row: index 0
    x[0, 1, :] = -1.0
    x[0, 1, N - 1] = 4.0                     # the max in the last element alone
    x[1, 2, :] = -2.0
    x[1, 2, [N // 2, N - 1]] = 3.0           # a tie in the body and the tail
    x[2, 3, :] = 1.0
    x[2, 3, 0] = -0.0                        # -0.0 / +0.0 compare equal: the first max wins
    x[2, 3, 1:] = 0.0
    xd = torch.tensor(x, device="cuda")
    tgt = torch.tensor(_targets(rng, B, 10, N, T), device="cuda")
    ts = Cr.batch_target_size(tgt, T, ctc=True)
    lf, pf, ls, ps = _both(xd, tgt, ts, 0)
    _assert_bitwise(lf, pf, ls, ps)
    assert ps[0, 0] == 0 and ps[0, 1] == N - 1 and ps[1, 2] == min(N // 2, N - 1) and ps[2, 3] == 0


@pytest.mark.gpu
def test_ctc_score_python_front_end():
    """criterion.ctc_score / CTCLoss.score == CTCLoss.forward and CTCLoss.viterbiPath"""
    from wav2letter_amd import CTCLoss, CriterionScaleMode
    rng = np.random.default_rng(3)
    B, T, N = 4, 60, 257
    x = torch.tensor(rng.normal(size=(B, T, N)).astype(np.float32), device="cuda")
    tgt = torch.tensor(_targets(rng, B, 12, N, T), device="cuda")
    crit = CTCLoss(CriterionScaleMode.TARGET_SZ_SQRT)
    loss, path = crit.score(x, tgt)
    assert loss.shape == (B,) and path.shape == (B, T) and path.dtype == torch.int32
    assert torch.equal(loss.view(torch.int32), crit(x, tgt).detach().view(torch.int32))
    assert torch.equal(path, crit.viterbiPath(x))
