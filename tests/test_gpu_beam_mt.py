"""The many-token beam searches (w2l_*_beam_search*_mt, W up to 8192, K up to 256) on the GPU, with the machinery of
tests/test_gpu_beam_wide.py and the restatement with counts of tests/beam_mt_ref.py.
M1 identity with the xl kernels at K <= 64, byte for byte, both (+) modes, with and without a silence score; M2 logAdd = 0 bit for
bit against the float32 restatement at every K around a mask-word boundary, on inputs whose sums are exact and whose ties are
dense, with the proof from the CPU that selections were decided by the tie key among tokens of rank 64 and above and across a
64-boundary; M3 merges in the three upper mask words at W = 8192, K = 256, in the lexicon's word slots too; M4 logAdd = 1 against
the float64 restatement where the decisions have a margin; M5 the row pass alone; M6 clipping; M7 the surfaces: Python, the
compiled C++ caller, Decode --w2l_beam_tokens.
The restatements of M2 and M3 take up to a minute each on the CPU: their outputs are digests in tests/golden/beam_mt_golden.json
(tests/golden/make_beam_mt_golden.py writes it; M = W rows, so a digest speaks for every row), the inputs come from the seeds."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import beam_mt_ref as MR
from tests.test_gpu_beam_wide import F32, INF, KEYS, KINDS, ROOT, W3_M, Case, _delta, _dense_case, _same_bits, _w1_case

pytestmark = pytest.mark.gpu
MT, XL = "mt", "xl"
SIZE = {"ctc": "w2l_ctc_beam", "ctc_lm": "w2l_ctc_beam_lm", "ctc_lex": "w2l_ctc_beam_lex", "asg": "w2l_asg_beam", "asg_lm": "w2l_asg_beam",
        "asg_lex": "w2l_asg_beam_lex"}
WS_MAX = 256 << 20


def _ws_bytes(c, W, K):
    """the declared workspace of the many-token search of this case's kind"""
    from wav2letter_amd import _lib
    B, T, N = c.x.shape
    return getattr(_lib.lib(), SIZE[c.kind] + "_mt_workspace_size")(B, T, N, W, K)


def _gpu(c, W, K, M, Lmax, wide, threshold=INF, log_add=False, normalize=False, max_words=None, sil=None):
    """Case.gpu with a silence score: sil = (token, score) or None"""
    if sil is None:
        return c.gpu(W, K, M, Lmax, wide, threshold, log_add, normalize, max_words)
    from tests.test_gpu_beam_wide import _lex_table, _lm_table
    from wav2letter_amd import criterion
    if c.tb is not None and not hasattr(c, "_lm"):
        c._lm = _lm_table(c.tb)
    if c.trie is not None and not hasattr(c, "_lex"):
        c._lex = _lex_table(c.trie)
    xd = torch.tensor(c.x, device="cuda")
    fd = torch.tensor(c.frames, dtype=torch.int32, device="cuda") if c.frames is not None else None
    kw = dict(beam=W, beam_token=K, threshold=threshold, log_add=log_add, normalize=normalize, nbest=M, max_len=Lmax, wide=wide,
              sil_token=sil[0], sil_score=sil[1])
    if c.tb is not None:
        kw.update(lm=c._lm, lm_weight=c.lmw, eos_score=c.eos)
        if c.cls is not None:
            kw.update(class_score=torch.tensor(c.cls, device="cuda"))
    if c.trie is not None:
        kw.update(lexicon=c._lex, word_score=c.wsc, max_words=max_words)
    out = criterion.asg_beam_search(xd, torch.tensor(c.A, device="cuda"), fd, **kw) if c.asg else criterion.ctc_beam_search(xd, fd, **kw)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in zip(KEYS, out)}


def _rows(want):
    return {k: v for k, v in want.items() if k != "diags"}


# ---- M1: identity with the xl kernels below the old limit ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _m1_case(kind):
    return _dense_case(kind, 700 + KINDS.index(kind), 3, 12, 70, [12, 1, 7], hot=64, nwords=600, max_len=2)


@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("K", [1, 29, 64])
@pytest.mark.parametrize("W", [1, 64, 65, 1025])
@pytest.mark.parametrize("kind", KINDS)
def test_m1_mt_equals_the_xl_twin_byte_for_byte(kind, W, K, log_add):
    """every output tensor, both (+) modes, N = 70, T = 12, B = 3 with ragged frames, a threshold that cuts from W = 64 up and label
    and word rows shorter than the hypotheses; with a silence score the other side is the *_sil entry point at family 2"""
    c = _m1_case(kind)
    M, Lmax, thr = W, 5, (INF if W < 64 else 4.0)
    norm = log_add and not c.asg
    xl = c.gpu(W, K, M, Lmax, XL, thr, log_add, norm, 2)
    mt = c.gpu(W, K, M, Lmax, MT, thr, log_add, norm, 2)
    assert (xl["lengths"] >= 0).any() or kind.endswith("lex")
    _same_bits(mt, xl)
    sil = (c.trie.sil if c.trie is not None else 3, -0.75)
    xl_sil = _gpu(c, W, K, M, Lmax, XL, thr, log_add, norm, 2, sil)
    _same_bits(_gpu(c, W, K, M, Lmax, MT, thr, log_add, norm, 2, sil), xl_sil)
    if W >= 64 and K == 64 and c.trie is None:
        assert any((xl_sil[k].view(np.int32) != xl[k].view(np.int32)).any() for k in ("labels", "scores")), "the silence score is inert"


# ---- M2: bit for bit against the float32 restatement, logAdd = 0 -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _m2_case(kind):
    c = MR.m2_case(kind)
    return c, MR.input_digest(c)


@pytest.mark.parametrize("K", MR.M2_K)
@pytest.mark.parametrize("W", MR.M2_W)
@pytest.mark.parametrize("kind", KINDS)
def test_m2_bitwise_against_the_float32_restatement(kind, W, K):
    """N = 300 (K binds, 256 < N - 1), T = 10, B = 3; the restatement's digests and counts are the golden file's.  Asserted from
    the restatement before the device is asked: a selected candidate was put first by the tie key alone between two extensions
    whose k are both >= 64, and one between two extensions of one entry whose k lie in different mask words (beam_mt_ref's tie_high and
    tie_cross)"""
    N, T, B, _ = MR.M2_SHAPE
    c, xsha = _m2_case(kind)
    g = MR.golden()[f"m2/{kind}/W{W}/K{K}"]
    assert g["x"] == xsha, "the seed gives other inputs than the golden file's"
    words = (K + 63) // 64
    assert g["tie_high"] > 0 and g["tie_cross"] > 0 and g["live"] > 0, g
    assert not any(g["merges"][0][words:]) and not any(g["merges"][1][words:]), g         # no token beyond K (M3 is about the merges)
    assert 0 < _ws_bytes(c, W, K) <= WS_MAX
    got = c.gpu(W, K, W, T, MT, INF, False, False, T)
    sha = MR.digests(got)
    print("M2", kind, W, K, {k: g[k] for k in ("tie_high", "tie_cross", "merges", "live")}, "live rows", int((got["lengths"] >= 0).sum()))
    assert int((got["lengths"] >= 0).sum()) == g["live"]
    assert sha == g["sha"], [k for k in sha if sha[k] != g["sha"].get(k)]


# ---- M3: merges in the upper mask words ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_m3_merges_in_the_upper_mask_words_at_w8192_k256(kind):
    """T = 3, N = 300, K = 256, W = 8192, no threshold line, the frames' rankings permuted (beam_mt_ref.m3_case): the restatement
    counts merged extensions in each of the three upper mask words, with a lexicon in a word slot (slot >= 1) too; bit-equal"""
    N, T, B, K, W = MR.M3_SHAPE
    c = MR.m3_case(kind)
    g = MR.golden()[f"m3/{kind}/W{W}/K{K}"]
    assert g["x"] == MR.input_digest(c), "the seed gives other inputs than the golden file's"
    assert all(g["merges"][0][w] > 0 for w in (1, 2, 3)), g
    if kind.endswith("lex"):
        assert all(g["merges"][1][w] > 0 for w in (1, 2, 3)), g
    assert 0 < _ws_bytes(c, W, K) <= WS_MAX
    got = c.gpu(W, K, W, T, MT, INF, False, False, T)
    print("M3", kind, {k: g[k] for k in ("merges", "live")})
    assert int((got["lengths"] >= 0).sum()) == g["live"]
    sha = MR.digests(got)
    assert sha == g["sha"], [k for k in sha if sha[k] != g["sha"].get(k)]


# ---- M4: logAdd = 1 against the float64 restatement ----------------------------------------------------------------------------

M4_SHAPE = (150, 300, 6, 4)                                                                    # (W, N, T, B)


@functools.lru_cache(maxsize=None)
def _m4_reference(kind, K):
    """the method of test_gpu_beam_xl.py's X3 at K = 100 and 256.  The rows are a permuted grid of step 0.05 with a jitter of a
    tenth of it, eight classes (and the blank) lifted by 6: the K-th and the (K + 1)-th token are 0.04 apart wherever K falls, a
    hundred times the bound, so whether a rank is compared depends on the beam's margins alone"""
    from tests import ctc_beam_lex_ref as XR
    from tests import ctc_beam_lm_ref as LR
    from tests.test_gpu_beam_wide import _smear
    W, N, T, B = M4_SHAPE
    rng = np.random.default_rng(960 + 10 * KINDS.index(kind) + (K == 256))
    asg = kind.startswith("asg")
    tokens = N if asg else N - 1
    x = np.stack([[rng.permutation(N) * -0.05 + rng.uniform(-0.005, 0.005, N) for _ in range(T)] for _ in range(B)]).astype(F32)
    x[:, :, :8] += 6
    if not asg:
        x[:, :, N - 1] += 6
    A = rng.normal(0, 1, size=(N, N)).astype(F32) if asg else None
    c = Case(kind, x, None, A)
    if kind.endswith("lm"):
        c = Case(kind, x, None, A, LR.random_lm(rng, tokens, 3, 300), None, rng.normal(0, 0.3, tokens).astype(F32), 0.8, 0.0, -0.3)
    if kind.endswith("lex"):
        nwords = 600
        tb = LR.random_lm(rng, nwords, 3, 600)
        trie = XR.TextbookTrie(XR.random_lexicon(rng, tokens, nwords, 2, 0.1, 7, 260), tokens, nwords, _smear(tb, nwords), 7)
        c = Case(kind, x, None, A, tb, trie, None, 0.8, 0.3, -0.3)
    want = MR.case_ref(c, W, K, W3_M, T, np.float64, INF, True, not asg, T)
    lead = []      # per utterance: the leading ranks whose every decision has a margin above twice the bound, and the bound
    for dg in want["diags"]:
        dl = _delta(kind, T, dg.S)
        n = 0
        if dg.token_gap > 2 * dl:
            while n < len(dg.margins) and dg.margins[n] > 2 * dl and (n >= len(dg.final_gaps) or dg.final_gaps[n] > 2 * dl):
                n += 1
        lead.append((n, dl))
    return c, want, lead


@pytest.mark.parametrize("K", [100, 256])
@pytest.mark.parametrize("kind", KINDS)
def test_m4_log_sum_search_against_the_float64_restatement(kind, K):
    """the scores within ctc_beam_ref.delta / asg_beam_ref.delta_asg and their siblings (no new number), the hypotheses compared where
    the restatement's own margins exceed twice that bound; at most one utterance in four may have no such rank"""
    W, N, T, B = M4_SHAPE
    c, want, lead = _m4_reference(kind, K)
    left_out = sum(1 for n, _ in lead if n == 0)
    print("M4", M4_SHAPE, kind, K, "compared ranks per utterance", [n for n, _ in lead], "delta", max(dl for _, dl in lead))
    assert 4 * left_out <= B and (want["lengths"] >= 0).any()
    got = c.gpu(W, K, W3_M, T, MT, INF, True, not c.asg, T)
    for b, (n, dl) in enumerate(lead):
        for k in ("labels", "lengths", "words", "word_counts"):
            if k in want:
                assert (got[k][b, :n] == want[k][b, :n]).all(), (b, k)
        assert (np.abs(got["scores"][b, :n].astype(np.float64) - want["scores"][b, :n]) <= dl).all(), b
        if "lm_scores" in want:
            assert (got["lm_scores"][b, :n].view(np.int32) == want["lm_scores"][b, :n].view(np.int32)).all()


# ---- M5: the row pass alone ----------------------------------------------------------------------------------------------------

def _m5_rows(name):
    """(N, K, x [2][1][N]): one frame, two utterances"""
    rng = np.random.default_rng(50)
    if name == "n257_k256":                      # K = N - 1: every token of a CTC row
        N, K = 257, 256
        x = (rng.integers(-40, 1, size=(2, 1, N)) / 4).astype(F32)
    elif name == "n9998_k100":                   # the word-piece model's row, in registers
        N, K = 9998, 100
        x = (rng.integers(-400, 1, size=(2, 1, N)) / 4).astype(F32)
    elif name == "n12289_k100":                  # just past the register-resident limit: the row is re-read from memory
        N, K = 12289, 100
        x = (rng.integers(-400, 1, size=(2, 1, N)) / 4).astype(F32)
    elif name == "flat_k256":                    # more than 1024 elements equal to the maximum: K rounds of block-wide extraction
        N, K = 2000, 256
        x = np.zeros((2, 1, N), F32)
        x[1, 0, 1500:] = -1.0
    elif name == "flat_big_k256":                # the same beyond the register-resident limit
        N, K = 12400, 256
        x = np.zeros((2, 1, N), F32)
    else:                                        # fewer than K finite values
        assert name == "few_finite_k100"
        N, K = 300, 100
        x = np.full((2, 1, N), -np.inf, F32)
        x[0, 0, rng.permutation(N - 1)[:40]] = (rng.integers(-40, 1, size=40) / 4).astype(F32)
        x[1, 0, 5] = -2.0
    return N, K, x


M5_ROWS = ["n257_k256", "n9998_k100", "n12289_k100", "flat_k256", "flat_big_k256", "few_finite_k100"]


@pytest.mark.parametrize("name,kind", [(n, "ctc") for n in M5_ROWS] + [(n, "asg") for n in ("n257_k256", "flat_k256", "few_finite_k100")])
def test_m5_the_row_pass_alone(name, kind):
    """T = 1, W = M = K + 1: the output rows list the frame tokens in the contract's order -- lp descending, class ascending -- with
    the empty prefix (CTC: the blank's stay) where its score puts it; bit-equal to the restatement, whose tokens are numpy's
    lexsort.  ASG (no blank, K may reach N) runs the rows whose N * N transitions stay small"""
    N, K, x = _m5_rows(name)
    asg = kind == "asg"
    x = x.copy()
    if not asg:
        x[:, :, N - 1] = -1000.0                 # the empty prefix comes last
    c = Case(kind, x, None, np.zeros((N, N), F32) if asg else None)
    with np.errstate(invalid="ignore"):
        want = MR.case_ref(c, K + 1, K, K + 1, 1)
    toks = [d.tokens[0] for d in want["diags"]]
    if name.startswith("flat"):
        assert toks[0] == list(range(K))         # classes ascending
    finite = [int(np.isfinite(x[b, 0, :N if asg else N - 1]).sum()) for b in range(2)]
    for b in range(2):
        n = min(K, finite[b])
        assert [int(v) for v in want["labels"][b, :n, 0]] == toks[b][:n] and (want["lengths"][b, :n] == 1).all()
    got = c.gpu(K + 1, K, K + 1, 1, MT)
    _same_bits(got, _rows(want))


# ---- M6: clipping ----------------------------------------------------------------------------------------------------------------

def test_m6_ctc_n200_beam_token_256_runs_199_tokens():
    from wav2letter_amd import _lib
    c = _dense_case("ctc_lm", 77, 2, 4, 200, None)
    size = _lib.lib().w2l_ctc_beam_lm_mt_workspace_size
    assert size(2, 4, 200, 300, 256) == size(2, 4, 200, 300, 199) > size(2, 4, 200, 300, 198)
    want = MR.case_ref(c, 300, 256, 300, 4)
    assert all(len(d.tokens[0]) == 199 for d in want["diags"])
    got = c.gpu(300, 256, 300, 4, MT)
    _same_bits(got, _rows(want))
    _same_bits(c.gpu(300, 199, 300, 4, MT), got)


@pytest.mark.parametrize("kind", ["asg", "asg_lm", "asg_lex"])
def test_m6_asg_n30_beam_token_1500_equals_the_xl_twin(kind):
    c = _w1_case(kind)
    for log_add in (False, True):
        _same_bits(c.gpu(1025, 1500, 8, 24, MT, 4.0, log_add, False, 4), c.gpu(1025, 1500, 8, 24, XL, 4.0, log_add, False, 4))


# ---- M7: surfaces ----------------------------------------------------------------------------------------------------------------

def test_m7_python_methods_take_mt():
    from wav2letter_amd import ASGLoss, CTCLoss, _lib, criterion
    c, _ = _m2_case("ctc_lm")
    xd, fd = torch.tensor(c.x, device="cuda"), torch.tensor(c.frames, dtype=torch.int32, device="cuda")
    want = c.gpu(300, 100, 3, 10, MT)
    got = CTCLoss().beamSearch(xd, fd, beam=300, beam_token=100, nbest=3, lm=c._lm, lm_weight=c.lmw, eos_score=c.eos,
                               class_score=torch.tensor(c.cls, device="cuda"), wide=MT)
    assert all((g.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all() for g, k in zip(got, KEYS))
    a, _ = _m2_case("asg")
    crit = ASGLoss(300).cuda()
    with torch.no_grad():
        crit.transitions.copy_(torch.tensor(a.A))
    xa, fa = torch.tensor(a.x, device="cuda"), torch.tensor(a.frames, dtype=torch.int32, device="cuda")
    want = _gpu(a, 300, 150, 3, 10, MT, sil=(7, -0.5))
    got = crit.beamSearch(xa, fa, beam=300, beam_token=150, nbest=3, wide=MT, sil_token=7, sil_score=-0.5)
    assert len(got) == 3 and all((g.cpu().numpy().view(np.int32) == want[k].view(np.int32)).all() for g, k in zip(got, KEYS))
    # beyond 8192 entries and 256 tokens the many-token path refuses; the other families keep 64 tokens
    for wide, beam, tok in ((MT, 8193, 100), (MT, 300, 257), (XL, 300, 65), (True, 300, 65), (False, 64, 65)):
        with pytest.raises(_lib.W2LError):
            criterion.ctc_beam_search(xd, beam=beam, beam_token=tok, wide=wide)
        with pytest.raises(_lib.W2LError):
            criterion.asg_beam_search(xa, torch.tensor(a.A, device="cuda"), beam=beam, beam_token=tok, wide=wide)
    assert criterion.ctc_beam_search(xd, beam=65, beam_token=256, wide=MT)[1].min() >= 0


def test_m7_cpp_options_many_tokens_equal_the_c_abi(tmp_path):
    """tests/cpp/decode_mt_caller.cpp (plain g++ against libw2l_hip.so): BeamSearchOptions::manyTokens at K = 100 for CTC with a
    silence score and at K = 150 for ASG; its output equals the Python front end's, which calls the C ABI"""
    exe, libdir = str(tmp_path / "decode_mt_caller"), os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "decode_mt_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    W, M, Lmax = 300, 5, 10
    for mode, K, sil in (("ctc", 100, (7, -0.5)), ("asg", 150, None)):
        c, _ = _m2_case(mode)
        B, T, N = c.x.shape
        frames = np.array(c.frames, np.int32)
        want = _gpu(c, W, K, M, Lmax, MT, 6.0, sil=sil)
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([N, T, B, W, K, M, Lmax, sil[0] if sil else -1], np.int32).tobytes()
                    + np.array([sil[1] if sil else 0.0], F32).tobytes() + frames.tobytes() + c.x.tobytes()
                    + (c.A if c.A is not None else np.zeros(0, F32)).tobytes())
        run = subprocess.run([exe, mode, inp, outp], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "decode mt caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
        raw = np.fromfile(outp, np.int32)
        pos = 0
        for k, shape in (("labels", (B, M, Lmax)), ("lengths", (B, M)), ("scores", (B, M))):
            n = int(np.prod(shape))
            assert (raw[pos:pos + n].reshape(shape) == want[k].view(np.int32)).all(), (mode, k)
            pos += n
        assert pos == len(raw) and (want["lengths"] >= 0).any()


# ---- Decode --w2l_beam_tokens ------------------------------------------------------------------------------------------------------

from tests.list_fixture import ENV, LETTERS, TRAIN_EXE, UTTS, _fixture, _train_cmd  # noqa: E402
from tests.test_gpu_ctc_beam import DECODE_EXE, _sclite_lines  # noqa: E402

TOKENS = LETTERS + [f"x{i:03d}" for i in range(272)]            # 300 tokens: --beamsizetoken=100 and 150 are not clipped


@pytest.fixture(scope="module")
def trained_100(tmp_path_factory):
    """the tiny CTC checkpoint of the xl tests on a token dictionary of 300 entries (the letters, then 272 that no transcript uses)"""
    d = tmp_path_factory.mktemp("decode_mt")
    _fixture(d)
    (d / "tokens.txt").write_text("\n".join(TOKENS) + "\n")
    out = subprocess.run(_train_cmd(d, d / "run"), capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return d, d / "run" / "exp" / "001_model_last.bin"


@pytest.fixture(scope="module")
def trained_asg_100(tmp_path_factory):
    d = tmp_path_factory.mktemp("decode_mt_asg")
    _fixture(d)
    (d / "tokens.txt").write_text("\n".join(TOKENS) + "\n")
    cmd = [TRAIN_EXE, "train", f"--archdir={d / 'arch'}", "--arch=net.arch", "--criterion=asg", "--replabel=1", "--transdiag=0.5",
           "--filterbanks=40", f"--tokensdir={d}", "--tokens=tokens.txt", f"--lexicon={d / 'lexicon.txt'}", f"--datadir={d}",
           "--train=train.lst", "--batchsize=3", "--iter=6", "--reportiters=3", "--lr=0.05", "--lrcrit=0.002", "--momentum=0.8",
           "--maxgradnorm=1.0", "--onorm=target", "--sqnorm=true", f"--rundir={d / 'run'}", "--runname=exp"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=ENV)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return d, d / "run" / "exp" / "001_model_last.bin"


def _decode(d, model, *flags, ok=True):
    res = subprocess.run([DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}"] + list(flags),
                         capture_output=True, text=True, timeout=600, env=ENV)
    assert (res.returncode == 0) == ok, res.stdout[-2000:] + res.stderr[-2000:]
    return res.stderr, (d / "out" / "other.hyp").read_text() if ok else ""


def test_m7_decode_w2l_beam_tokens_ctc(trained_100):
    """with the flag a --beamsizetoken of 100 runs the many-token kernels at 100 tokens and any given --beamsize; the .hyp is the
    Python call's at K = 100 on the same emissions (the features Decode dumped, the eval forward); 300 is limited to 256 and 9000
    entries to 8192, each said on stderr; without the flag the line and the limit to 64 stay"""
    from wav2letter_amd import checkpoint, criterion, text
    from wav2letter_amd.trainer import Trainer
    d, model = trained_100
    err64, hyp64 = _decode(d, model, "--beamsize=200", "--beamsizetoken=100")
    assert "--beamsizetoken limited to 64 tokens per frame" in err64 and "(many-token)" not in err64 and "beam 200 (wide)" in err64
    err, hyp = _decode(d, model, "--beamsize=200", "--beamsizetoken=100", "--w2l_beam_tokens=true", f"--w2l_dump_features={d / 'dfeat'}")
    assert "beam 200 (many-token), tokens per frame 100" in err and "limited to" not in err and len(_sclite_lines(d / "out" / "other.hyp")) == 5
    dic = text.create_token_dict(TOKENS, "ctc")
    arch = (d / "arch" / "net.arch").read_text()
    N = dic.index_size()
    assert N == 301
    mine = []
    for k in range(3):                                                  # batches of 2, 2, 1 in list order
        utts = UTTS[2 * k:2 * k + 2][:5 - 2 * k]
        raw = (d / f"dfeat.{k + 1}").read_bytes()
        B, nfeat, T = (int(v) for v in np.frombuffer(raw[:12], np.int32))
        x = torch.tensor(np.frombuffer(raw[12:], np.float32).reshape(B, nfeat, T).copy()).cuda()
        tr_ = Trainer(arch, nfeat, N, "ctc", 4, 0.0)
        checkpoint.load(str(model), tr_, arch)
        tr_.plan(B, T, 8)
        tr_.to_device()
        em = tr_.forward(x, train=False).clone()
        Tout = em.shape[1]
        frames = torch.tensor([min(max(-(-min(1 + (n - 400) // 160, T) * Tout // T), 1), Tout) for n, _ in utts], dtype=torch.int32).cuda()
        labels, lengths, _ = criterion.ctc_beam_search(em, frames, beam=200, beam_token=100, threshold=25.0, wide=MT)
        for b in range(B):
            letters = "".join(TOKENS[int(t)] for t in labels[b, 0, :int(lengths[b, 0])].cpu())
            mine.append([w for w in letters.split("|") if w])
    assert [w for w, _ in _sclite_lines(d / "out" / "other.hyp")] == mine
    # the other widths: narrow, and beyond the limits
    err, h = _decode(d, model, "--beamsize=8", "--beamsizetoken=100", "--w2l_beam_tokens=true")
    assert "beam 8 (many-token), tokens per frame 100" in err and h == hyp
    err, h = _decode(d, model, "--beamsize=9000", "--beamsizetoken=300", "--w2l_beam_tokens=true")
    assert "--beamsize=9000 limited to 8192 (the kernel's beam width)" in err and "--beamsizetoken limited to 256 tokens per frame" in err
    assert "beam 8192 (many-token), tokens per frame 256" in err and h == hyp       # the max search's 1-best: the greedy transcript
    # at or under 64 tokens, or without a --beamsizetoken, routing is as without the flag
    err, h = _decode(d, model, "--beamsize=200", "--beamsizetoken=64", "--w2l_beam_tokens=true")
    assert "beam 200 (wide), tokens per frame 64" in err and "(many-token)" not in err and h == hyp64
    err, h = _decode(d, model, "--beamsize=200", "--w2l_beam_tokens=true")
    assert "--beamsizetoken limited to 64 tokens per frame" in err and "(many-token)" not in err and h == hyp64
    err, _ = _decode(d, model, "--beamsizetoken=100", "--w2l_beam_tokens=true", "--w2l_lex_tkn=true", ok=False)
    assert "--w2l_beam_tokens=true with --w2l_lex_tkn=true" in err


def test_m7_decode_w2l_beam_tokens_asg(trained_asg_100):
    """the ASG checkpoint (301 classes with the replabel): with --logadd=false and no LM the 1-best of every search is the Viterbi
    transcript, which a beam of one entry keeps"""
    d, model = trained_asg_100
    _, viterbi = _decode(d, model, "--beamsize=1")
    err, hyp = _decode(d, model, "--beamsize=2500", "--beamsizetoken=150", "--w2l_beam_tokens=true")
    assert "beam 2500 (many-token), tokens per frame 150" in err and "limited to" not in err and hyp == viterbi
