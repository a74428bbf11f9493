"""Host-side tests of the CPC criterion (no GPU): the sampler of include/fl_compat/cpc.h against its Python twin
(wav2letter_amd/cpc.py) bit for bit and against the textbook restatement (tests/cpc_ref.py), the properties of the mask and of the
negatives, every refusal of the C ABI (refusals come before anything touches the device, so the device pointers here are made-up
addresses), the workspace query as arithmetic, and the float64 restatement against a brute-force loop."""
import os
import subprocess

import numpy as np
import pytest

import cpc_ref as R
from wav2letter_amd import _lib, cpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = [1 << 20, 1 << 24, 1 << 28, 1 << 30, 1 << 32, 1 << 33, 1 << 34, 1 << 35, 1 << 36, 1 << 37, 1 << 38, 1 << 39]   # never dereferenced


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpc") / "cpc_sampler_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "cpc_sampler_test.cpp"), "-o", out],
                   check=True)
    return out


def run_cpp(exe, B, T, prob, length, n_neg, seed, frames=None):
    args = [exe, "sample", str(B), str(T), repr(prob), str(length), str(n_neg), str(seed)] + [str(f) for f in (frames or [])]
    lines = subprocess.run(args, capture_output=True, text=True, check=True).stdout.splitlines()
    if lines[0].startswith("refused"):
        return lines[0]
    M, K = (int(v) for v in lines[0].split())
    index = np.array([[int(v) for v in lines[1 + 2 * b].split()] for b in range(B)], np.int32)
    mask = np.array([[int(ch) for ch in lines[2 + 2 * b]] for b in range(B)], np.uint8)
    neg = np.array([[int(v) for v in ln.split()] for ln in lines[1 + 2 * B:]], np.int32).reshape(B, M, K)
    return mask, index, neg


SAMPLES = [  # B, T, maskProb, maskLength, nNegative, seed, frames
    (3, 50, 0.3, 5, 7, 12345, None),
    (3, 50, 0.3, 5, 7, 12345, [50, 31, 20]),
    (2, 37, 0.2, 4, 100, 1, None),                      # nNegative clipped to M
    (4, 200, 0.065, 10, 10, 2 ** 63 + 11, None),        # the recipe's maskProb / maskLength; a seed above 2^63
    (1, 23, 0.9, 1, 3, 0, None),                        # single frames, one utterance
    (2, 64, 0.5, 6, 5, 77, [9, 64]),                    # one utterance much shorter than the other
]


@pytest.mark.parametrize("case", SAMPLES)
def test_python_sampler_equals_the_header_and_the_textbook(exe, case):
    """S1: the same mask, index and negatives from the C++ header, the Python twin and the textbook sampler, bit for bit"""
    B, T, prob, length, n_neg, seed, frames = case
    got = run_cpp(exe, B, T, prob, length, n_neg, seed, frames)
    mask, index, neg = cpc.sample(B, T, prob, length, n_neg, frames, seed)
    assert mask.dtype == np.uint8 and index.dtype == np.int32 and neg.dtype == np.int32
    for a, b in zip(got, (mask, index, neg)):
        assert a.shape == b.shape and (a == b).all()
    t_index, t_neg, _ = R.sampler(B, T, prob, length, n_neg, frames, seed)
    assert (np.array(t_index) == index).all() and (np.array(t_neg) == neg).all()


@pytest.mark.parametrize("case", SAMPLES)
def test_mask_rows_ascend_share_m_and_stay_inside_the_frames(case):
    """S2: every row of maskIndex strictly ascending with the same M; the byte mask marks exactly those frames; every kept frame
    belongs to the span of a drawn start; with frames nothing is marked at or beyond frames[b]"""
    B, T, prob, length, n_neg, seed, frames = case
    mask, index, neg = cpc.sample(B, T, prob, length, n_neg, frames, seed)
    M = index.shape[1]
    assert M >= 4 and neg.shape == (B, M, min(n_neg, M))
    _, _, starts = R.sampler(B, T, prob, length, n_neg, frames, seed)
    smallest = T
    for b in range(B):
        n = T if frames is None else frames[b]
        assert (np.diff(index[b]) > 0).all() and index[b].min() >= 0 and index[b].max() < n
        assert (np.flatnonzero(mask[b]) == index[b]).all()
        marked = set().union(*(R.span(s, length, n) for s in starts[b]))
        assert set(index[b].tolist()) <= marked
        smallest = min(smallest, len(marked))
    assert M == smallest   # the smallest marked count of the batch


def test_spans_alternate_around_the_start_and_are_clipped():
    """S3: s, s+1, s-1, s+2, s-2 ...; frames outside [0, n) are dropped, nothing wraps around"""
    def marks(s, length, n):
        row = np.zeros(n, np.uint8)
        cpc.mark_span(row, s, length, n)
        return np.flatnonzero(row).tolist()
    assert marks(10, 1, 20) == [10]
    assert marks(10, 2, 20) == [10, 11]
    assert marks(10, 3, 20) == [9, 10, 11]
    assert marks(10, 4, 20) == [9, 10, 11, 12]
    assert marks(10, 5, 20) == [8, 9, 10, 11, 12]
    assert marks(0, 5, 20) == [0, 1, 2]          # -1 and -2 dropped
    assert marks(19, 4, 20) == [18, 19]          # 20 and 21 dropped, nothing lands on frame 0
    assert marks(1, 6, 3) == [0, 1, 2]
    for s, length, n in ((0, 5, 20), (19, 4, 20), (7, 10, 9)):
        assert set(marks(s, length, n)) == R.span(s, length, n)


@pytest.mark.parametrize("M", [4, 5, 9])
def test_negatives_avoid_the_window_and_reach_every_other_position(exe, M):
    """S4: no negative names m or a list neighbour; every allowed position is drawn at some point; the header agrees"""
    B, n_neg, seed = 2, 300, 5
    neg = cpc.negatives(cpc.CpcRng(seed), B, M, n_neg)
    K = min(n_neg, M)
    assert neg.shape == (B, M, K)
    lines = subprocess.run([exe, "negatives", str(B), str(M), str(n_neg), str(seed)], capture_output=True, text=True, check=True).stdout.split()
    assert (np.array([int(v) for v in lines], np.int32).reshape(B, M, K) == neg).all()
    seen = [set() for _ in range(M)]
    rng = cpc.CpcRng(seed)
    for _ in range(40):   # K is at most M: draw often enough that every allowed position turns up
        for b, rows in enumerate(cpc.negatives(rng, B, M, n_neg)):
            for m, row in enumerate(rows):
                seen[m] |= set(int(v) for v in row)
    for m in range(M):
        assert sorted(seen[m]) == R.allowed_negatives(m, M), (m, seen[m])
    assert R.allowed_negatives(0, M) == list(range(2, M)) and R.allowed_negatives(M - 1, M) == list(range(M - 2))


def test_fewer_than_four_masked_frames_are_refused_by_name(exe):
    """S5: M = 4 works, M = 3 is refused and the message names M"""
    assert cpc.negatives(cpc.CpcRng(1), 1, 4, 2).shape == (1, 4, 2)
    with pytest.raises(ValueError, match="M >= 4.*M = 3"):
        cpc.negatives(cpc.CpcRng(1), 1, 3, 2)
    with pytest.raises(ValueError, match="M >= 4"):
        cpc.sample(1, 20, 0.05, 3, 5, None, 3)      # one start, at most three frames
    got = run_cpp(exe, 1, 20, 0.05, 3, 5, 3)
    assert isinstance(got, str) and "M >= 4" in got
    with pytest.raises(ValueError, match=r"frames\[1\]"):
        cpc.sample(2, 20, 0.5, 3, 5, [20, 21], 3)
    assert "frames[1]" in run_cpp(exe, 2, 20, 0.5, 3, 5, 3, [20, 21])


# ---------------------------------------------------------------------------------------------- the C ABI without a device
def err():
    return _lib.lib().w2l_host_last_error().decode()


def _fwd(B=3, T=37, Ce=20, Cc=12, D=8, M=11, K=5, tau=0.1, ptr=None):
    p = list(P[:10]) if ptr is None else ptr
    return _lib.lib().w2l_cpc_forward(B, T, Ce, Cc, D, M, K, tau, *p, None), err()


def _bwd(B=3, T=37, Ce=20, Cc=12, D=8, M=11, K=5, tau=0.1, ptr=None):
    p = list(P[:12]) if ptr is None else ptr
    return _lib.lib().w2l_cpc_backward(B, T, Ce, Cc, D, M, K, tau, *p, None), err()


@pytest.mark.parametrize("call", [_fwd, _bwd])
@pytest.mark.parametrize("over,word", [
    (dict(M=0), "M = 0"), (dict(M=38), "M = 38"), (dict(K=0), "K = 0"), (dict(K=12), "K = 12"), (dict(D=0), "D must"),
    (dict(tau=0.0), "temperature"), (dict(tau=-0.1), "temperature"), (dict(tau=float("inf")), "temperature"),
    (dict(tau=float("nan")), "temperature"), (dict(B=0), "positive"), (dict(T=0), "positive"), (dict(Ce=0), "positive"),
    (dict(Cc=-3), "positive"),
])
def test_bad_shapes_are_invalid_arguments_with_a_message(call, over, word):
    st, msg = call(**over)
    assert st == _lib.W2L_EINVAL and word in msg and msg.startswith("cpc"), (st, msg)


def test_every_null_pointer_is_refused():
    for call, n in ((_fwd, 10), (_bwd, 12)):
        for i in range(n):
            p = list(P[:n])
            p[i] = None
            st, msg = call(ptr=p)
            assert st == _lib.W2L_EINVAL and "null" in msg, (call.__name__, i, st, msg)
    L = _lib.lib()
    for i in range(4):
        p = list(P[:4])
        p[i] = None
        assert L.w2l_cpc_apply_mask(2, 5, 3, *p, None) == _lib.W2L_EINVAL and "null" in err()
    for i in range(5):
        p = list(P[:5])
        p[i] = None
        assert L.w2l_cpc_apply_mask_backward(2, 5, 3, *p, None) == _lib.W2L_EINVAL and "null" in err()
    assert L.w2l_cpc_apply_mask(0, 5, 3, *P[:4], None) == _lib.W2L_EINVAL and "positive" in err()
    assert L.w2l_cpc_apply_mask_backward(2, 5, 0, *P[:5], None) == _lib.W2L_EINVAL and "positive" in err()
    p = list(P[:10])
    p[9] += 8
    st, msg = _fwd(ptr=p)
    assert st == _lib.W2L_EINVAL and "aligned" in msg


def test_workspace_query_is_host_arithmetic():
    L = _lib.lib()
    f = L.w2l_cpc_workspace_size

    def region(n):
        return (n + 63) // 64 * 64

    def want(B, T, Ce, Cc, D, M, K):
        R_ = B * M
        floats = (2 * region(R_ * Ce) + 2 * region(R_ * Cc) + 4 * region(R_ * D) + region(2 * R_) + 2 * region(R_ * M) + region(R_))
        return 4 * floats
    for dims in ((3, 37, 20, 12, 8, 11, 5), (2, 64, 33, 17, 7, 16, 16), (3, 800, 512, 768, 256, 400, 100), (3, 1600, 512, 768, 256, 800, 100)):
        assert f(*dims) == want(*dims), dims
    for bad in ((0, 37, 20, 12, 8, 11, 5), (3, 37, 20, 12, 0, 11, 5), (3, 37, 20, 12, 8, 0, 1), (3, 37, 20, 12, 8, 38, 5),
                (3, 37, 20, 12, 8, 11, 0), (3, 37, 20, 12, 8, 11, 12), (1, 20000, 4, 4, 4, 15999, 4)):
        assert f(*bad) == 0, bad
    st, msg = _fwd(T=20000, M=15999, K=4)
    assert st == _lib.W2L_EUNSUPPORTED and "16000" in msg
    assert L.w2l_cpc_mask_workspace_size(3, 37, 20) == 4 * 2 * 20 and L.w2l_cpc_mask_workspace_size(2, 64, 5) == 4 * 2 * 5
    assert L.w2l_cpc_mask_workspace_size(0, 64, 5) == 0 and L.w2l_cpc_mask_workspace_size(2, 64, 0) == 0


# ---------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("dims,tau", [((3, 37, 20, 12, 8, 11, 5), 0.1), ((2, 64, 33, 17, 7, 16, 16), 0.05)])
def test_restatement_against_a_brute_force_loop(dims, tau):
    """R1: the vectorised float64 restatement equals plain loops over (b, m, k); the loss of a chance-level model is near log(K + 1)"""
    c = R.Case(*dims, tau, seed=3)
    brute = R.loss_bruteforce(c)
    assert np.abs(c.loss - brute).max() < 1e-12 * max(1.0, np.abs(brute).max())
    # unmasked frames take no gradient; masked ones do
    for k in ("enc", "ctx"):
        g = c.grads[k]
        assert (g[c.mask == 0] == 0).all() and (np.abs(g[c.mask == 1]).max(axis=-1) > 0).all()
    assert np.isfinite(c.loss).all() and (c.loss > 0).all()
