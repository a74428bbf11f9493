"""w2l_ctc_beam_search_lm on the GPU against the numpy restatement of its contract (tests/ctc_beam_lm_ref.py).
L1 the exact recurrences at the enumeration shapes; L2 selection, merge, tie and end rules BITWISE (logAdd = 0; emissions, LM values
and class scores multiples of 1/8, lmWeight a power of two: every sum is exact in fp32 and ties are dense); L3 identity with
w2l_ctc_beam_search at lmWeight = 0; L4 the log-sum search with the beam binding, on inputs whose every decision has a margin;
then the surfaces (C ABI == Python == compiled C++) and `Decode --lm` end to end."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import ctc_beam_lm_ref as LR
from tests import ctc_beam_ref as R
from tests.test_gpu_ctc_beam import _close, _ints, _search

pytestmark = pytest.mark.gpu
INF = float("inf")
F32 = np.float32


def _lib():
    from wav2letter_amd import _lib
    return _lib


def _table(tb):
    from wav2letter_amd import NGramLM
    return NGramLM.from_ngrams(tb.arrays(), tb.V, float(tb.unk))


def _search_lm(x, frames, W, K, threshold, log_add, normalize, M, Lmax, lm, lmw, cls, eos_score):
    """the C ABI on numpy inputs -> labels [B][M][Lmax], lengths [B][M], scores [B][M], lmScores [B][M]"""
    L = _lib()
    lib = L.lib()
    B, T, N = x.shape
    st = torch.cuda.current_stream().cuda_stream
    xd = torch.tensor(x, device="cuda")
    fd = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
    cd = torch.tensor(np.asarray(cls, F32), device="cuda") if cls is not None else None
    blob = lm.device_blob("cuda")
    ws = torch.empty(max(lib.w2l_ctc_beam_lm_workspace_size(B, T, N, W, K), 256), dtype=torch.uint8, device="cuda")
    labels = torch.full((B, M, Lmax), -7, dtype=torch.int32, device="cuda")
    lengths = torch.full((B, M), -7, dtype=torch.int32, device="cuda")
    scores = torch.full((B, M), 7.0, device="cuda")
    lms = torch.full((B, M), 7.0, device="cuda")
    L.check(lib.w2l_ctc_beam_search_lm(B, T, N, xd.data_ptr(), fd.data_ptr() if fd is not None else None, W, K, threshold,
                                       int(log_add), int(normalize), M, Lmax, blob.data_ptr(), int(lm.has_eos), float(lmw),
                                       cd.data_ptr() if cd is not None else None, float(eos_score), labels.data_ptr(),
                                       lengths.data_ptr(), scores.data_ptr(), lms.data_ptr(), ws.data_ptr(), st), "ctc_beam_search_lm")
    torch.cuda.synchronize()
    return labels.cpu().numpy(), lengths.cpu().numpy(), scores.cpu().numpy(), lms.cpu().numpy()


# ---- L1: the exact recurrences ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,T", [(3, 5), (4, 3)])
def test_l1_exact_recurrences_at_the_enumeration_shapes(N, T):
    """W = 64, K = N-1, no threshold: the beam never binds and every labelling is there.  The float64 restatement takes g in fp32
    as the contract has it, so both sides share it; the ranks compared are those whose gaps are >= 10 delta: all of them
    (asserted)"""
    B, M = 3, 25
    rng = np.random.default_rng(100 + N)
    tb = LR.random_lm(rng, N - 1, 3, 12)
    cls = rng.normal(0, 0.5, N - 1).astype(F32)
    lmw, eos_score = 0.7, -0.4
    x = np.stack([np.random.default_rng(seed).normal(0, 2, size=(T, N)) for seed in (0, 1, 3)]).astype(F32)
    lab, ln, sc, lms, diags = LR.beam_search_lm(x, None, 64, N - 1, tb, lmw, cls, eos_score, INF, True, True, M, T, np.float64)
    glab, gln, gsc, glms = _search_lm(x, None, 64, N - 1, INF, True, True, M, T, _table(tb), lmw, cls, eos_score)
    print("L1", N, T, "max |score diff|", np.abs(gsc - sc).max())
    assert (gln >= 0).all() and _close(gsc, sc).all()
    for b in range(B):
        dl = LR.delta_lm(T, diags[b].S)
        lead = 0
        while lead < M - 1 and diags[b].final_gaps[lead] >= 10 * dl:
            lead += 1
        print("L1 seed", b, "delta", dl, "leading ranks with a margin", lead, "smallest gap", min(diags[b].final_gaps))
        assert lead == M - 1
        assert (gln[b] == ln[b]).all() and (glab[b] == lab[b]).all()
        assert (glms[b].view(np.int32) == lms[b].view(np.int32)).all()      # lmScores is fp32 on both sides: exact
        assert len({tuple(glab[b, m, :gln[b, m]]) for m in range(M)}) == M


# ---- L2: selection, merge, tie and end rules, bit for bit --------------------------------------------------------------------

# name: (B, T, N, frames, W, K, threshold, M, Lmax, (order, n-grams per order, bos, eos, classes without unigram, hot), lmWeight,
#        class scores, eosScore, seed)
L2_CASES = {
    "full_width_frames": (3, 40, 9998, [40, 1, 17], 64, 64, INF, 64, 40, (3, 4000, True, True, (), 300), 0.5, True, -0.25, 0),
    "w32_k5_threshold_m1": (2, 24, 9998, None, 32, 5, 2.5, 1, 24, (3, 4000, True, True, (), 300), 0.5, False, 0.0, 0),
    "w1_k1": (2, 16, 9998, None, 1, 1, INF, 1, 16, (3, 4000, True, True, (), 300), 1.0, False, 0.0, 0),
    "n30_k_clipped_short_lmax_order5": (3, 40, 30, [40, 9, 26], 16, 64, 3.0, 16, 3, (5, 300, True, True, (), None), 0.5, True, 0.5, 0),
    "n2_order2": (2, 12, 2, [12, 5], 8, 1, INF, 8, 12, (2, 4, True, True, (), None), 2.0, False, 0.0, 0),
    "n30_order1": (2, 20, 30, None, 8, 8, INF, 8, 20, (1, 0, True, True, (), None), 1.0, False, 0.0, 0),
    "n30_order2_wide": (2, 20, 30, None, 64, 64, INF, 64, 20, (2, 200, True, True, (), None), 0.5, True, 0.0, 0),
    "n30_no_eos_no_bos": (2, 20, 30, [20, 13], 16, 8, 4.0, 16, 20, (3, 300, False, False, (), None), 0.5, False, 0.0, 0),
    "n30_classes_fall_to_unk": (2, 20, 30, None, 16, 8, INF, 16, 20, (3, 300, True, True, (0, 3, 7), None), 0.5, False, 0.0, 0),
    "n30_eos_changes_the_best": (4, 10, 30, None, 16, 8, INF, 4, 10, (3, 300, True, True, (), None), 2.0, False, -1.0, 0),
    "n30_negative_weight": (2, 20, 30, None, 16, 8, INF, 16, 20, (3, 300, True, True, (), None), -0.5, True, 0.25, 0),
    "rows_from_memory": (2, 5, 12300, [5, 3], 8, 64, INF, 8, 5, (3, 4000, True, True, (), 300), 0.5, False, 0.0, 0),
}


@functools.lru_cache(maxsize=None)
def _l2_reference(name):
    """inputs, the float32 restatement's outputs, and the proof on the CPU that the case is not vacuous.  Every case must show that
    the LM changed a selection.  The other three facts are asserted wherever the case's shape allows them at all -- a DELIBERATE
    limit: a merge needs two beam entries (impossible at W = 1), out-of-order regular extensions need three tokens (impossible at
    K <= 2), a back-off chain of two needs a model of order three (impossible at order 1 and 2).  The degenerate cases (w1_k1,
    n2_order2, n30_order1, n30_order2_wide) are kept for the paths they alone reach; their families' siblings (w32_k5..., the other
    n30 cases) show all four."""
    B, T, N, frames, W, K, thr, M, Lmax, (order, per, bos, eos, drop, hot), lmw, with_cls, eos_score, seed = L2_CASES[name]
    rng = np.random.default_rng(len(name) * 1000 + T + seed)
    x = _ints(rng, B, T, N)
    tb = LR.random_lm(rng, N - 1, order, per, bos, eos, drop, eighths=True, hot=hot)
    cls = (rng.integers(-8, 9, N - 1) / 8).astype(F32) if with_cls else None
    out = LR.beam_search_lm(x, frames, W, K, tb, lmw, cls, eos_score, thr, False, False, M, Lmax, F32)
    free = R.beam_search(x, frames, W, K, thr, False, False, M, Lmax, F32)
    diags = out[4]
    Kc = min(K, N - 1)
    facts = dict(changed=not (np.array_equal(out[0], free[0]) and np.array_equal(out[1], free[1])),
                 nonmonotone=sum(d.nonmonotone for d in diags), merges=sum(d.merges for d in diags), chain=tb.max_chain,
                 unk=tb.unk_hits, eos_moves=sum(d.eos_moves for d in diags))
    assert facts["changed"], name
    assert facts["nonmonotone"] > 0 or Kc < 3, name
    assert facts["merges"] > 0 or W < 2, name
    assert facts["chain"] >= 2 or order < 3, name
    if drop:
        assert facts["unk"] > 0, name
    return x, tb, cls, out, facts


@pytest.mark.parametrize("name", list(L2_CASES))
def test_l2_bitwise_against_the_float32_restatement(name):
    B, T, N, frames, W, K, thr, M, Lmax, _, lmw, _, eos_score, _ = L2_CASES[name]
    x, tb, cls, (lab, ln, sc, lms, diags), facts = _l2_reference(name)
    print("L2", name, facts, "hypotheses", int((ln >= 0).sum()), "longest", int(ln.max()), "ties in the output",
          int(sum(len(s[s > -np.inf]) - len(np.unique(s[s > -np.inf])) for s in sc)))
    if name == "n30_k_clipped_short_lmax_order5":
        assert ln.max() > Lmax                                       # a hypothesis longer than the label rows
    if name == "n30_eos_changes_the_best":                           # without the end term another hypothesis leads
        lab0, ln0, _, _, _ = LR.beam_search_lm(x, frames, W, K, _without_eos(tb), lmw, cls, 0.0, thr, False, False, M, Lmax, F32)
        assert any(tuple(lab0[b, 0, :ln0[b, 0]]) != tuple(lab[b, 0, :ln[b, 0]]) for b in range(B)) and facts["eos_moves"] > 0
    glab, gln, gsc, glms = _search_lm(x, frames, W, K, thr, False, False, M, Lmax, _table(tb), lmw, cls, eos_score)
    assert sc.dtype == F32 and lms.dtype == F32
    assert (gln == ln).all()
    assert (glab == lab).all()
    assert (gsc.view(np.int32) == sc.view(np.int32)).all()
    assert (glms.view(np.int32) == lms.view(np.int32)).all()


def _without_eos(tb):
    """the same model with every n-gram that ends in EOS taken out"""
    ng = {g: (tb.p[g], tb.bo.get(g, 0)) for g in tb.p if g[-1] != tb.eos}
    return LR.TextbookLM(ng, tb.V, tb.unk)


# ---- L3: lmWeight = 0 is w2l_ctc_beam_search -------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,N,W,K,thr,log_add", [(2, 24, 9998, 64, 64, INF, False), (3, 30, 30, 8, 5, 6.0, True),
                                                    (2, 20, 9998, 16, 8, INF, True), (2, 24, 9998, 64, 64, INF, True)])
def test_l3_zero_weight_is_the_lm_free_search(B, T, N, W, K, thr, log_add):
    rng = np.random.default_rng(N + T)
    x = rng.normal(0, 2, size=(B, T, N)).astype(F32) if log_add else _ints(rng, B, T, N)
    frames = [T, T // 3, 1][:B]
    tb = LR.random_lm(rng, N - 1, 3, 500, hot=min(N - 1, 300))
    M = min(W, 8)
    lab, ln, sc = _search(x, frames, W, K, thr, log_add, log_add, M, T)
    glab, gln, gsc, glms = _search_lm(x, frames, W, K, thr, log_add, log_add, M, T, _table(tb), 0.0, None, 0.0)
    assert (gln == ln).all() and (glab == lab).all()
    assert (gsc == sc).all()                                         # equal as values: 0 * q is -0
    assert (np.isfinite(glms) == (ln >= 0)).all()


# ---- L4: the log-sum search with the beam binding ------------------------------------------------------------------------------

L4_CASES = [  # (T, N, W, K, scale, seeds): seeds whose every decision gap is >= 10 delta (asserted, never skipped)
    (12, 32, 4, 3, 2.0, (0, 1)),
    (16, 9998, 4, 3, 3.0, (1, 3)),
    (12, 6, 3, 2, 2.0, (0, 1)),
]


def _l4_inputs(T, N, W, K, scale, seeds):
    rng = np.random.default_rng(T * N)
    tb = LR.random_lm(rng, N - 1, 3, 400, hot=min(N - 1, 300))
    cls = rng.normal(0, 0.3, N - 1).astype(F32)
    x = np.stack([np.random.default_rng(s).normal(0, scale, size=(T, N)) for s in seeds]).astype(F32)
    return x, tb, cls, LR.beam_search_lm(x, None, W, K, tb, 0.8, cls, -0.3, INF, True, True, W, T, np.float64)


@pytest.mark.parametrize("T,N,W,K,scale,seeds", L4_CASES)
def test_l4_log_sum_search_small_beams(T, N, W, K, scale, seeds):
    x, tb, cls, (lab, ln, sc, lms, diags) = _l4_inputs(T, N, W, K, scale, seeds)
    for dg in diags:
        dl = LR.delta_lm(T, dg.S)
        print("L4", (T, N, W, K), "S", dg.S, "delta", dl, "decision gap", dg.decision_gap(), "final gap", min(dg.final_gaps))
        assert dg.decision_gap() >= 10 * dl and min(dg.final_gaps) >= 10 * dl
    glab, gln, gsc, glms = _search_lm(x, None, W, K, INF, True, True, W, T, _table(tb), 0.8, cls, -0.3)
    print("L4 max |score diff|", np.abs(gsc - sc).max())
    assert (gln == ln).all() and (glab == lab).all()
    assert _close(gsc, sc).all()
    assert (glms.view(np.int32) == lms.view(np.int32)).all()


# ---- surfaces ---------------------------------------------------------------------------------------------------------------

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arpa_files(tmp_path, tb, tokens):
    from tests.test_ctc_beam_lm_host import _arpa_text
    (tmp_path / "tokens.txt").write_text("\n".join(tokens) + "\n")
    (tmp_path / "lm.arpa").write_text(_arpa_text(tb, tokens, unk10=-3.0)[0])
    return tmp_path / "tokens.txt", tmp_path / "lm.arpa"


def test_python_front_end_equals_the_c_abi():
    from wav2letter_amd import CTCLoss, criterion
    B, T, N = 3, 30, 40
    rng = np.random.default_rng(5)
    x = rng.normal(0, 2, size=(B, T, N)).astype(F32)
    frames = np.array([30, 11, 1], np.int32)
    tb = LR.random_lm(rng, N - 1, 3, 300)
    lm = _table(tb)
    cls = rng.normal(0, 0.3, N - 1).astype(F32)
    xd, fd, cd = torch.tensor(x, device="cuda"), torch.tensor(frames, device="cuda"), torch.tensor(cls, device="cuda")
    for log_add, norm, thr, M, c, cdev in ((True, True, INF, 4, cls, cd), (False, False, 6.0, 1, None, None)):
        want = _search_lm(x, frames, 8, 5, thr, log_add, norm, M, T, lm, 0.6, c, -0.2)
        for got in (criterion.ctc_beam_search(xd, fd, beam=8, beam_token=5, threshold=thr, log_add=log_add, nbest=M, lm=lm,
                                              lm_weight=0.6, class_score=cdev, eos_score=-0.2),
                    CTCLoss().beamSearch(xd, fd, beam=8, beam_token=5, threshold=thr, log_add=log_add, normalize=norm, nbest=M,
                                         lm=lm, lm_weight=0.6, class_score=cdev, eos_score=-0.2)):
            assert len(got) == 4 and got[0].dtype == torch.int32 and got[3].dtype == torch.float32
            assert all((g.cpu().numpy().view(np.int32) == w.view(np.int32)).all() for g, w in zip(got, want))
    free = criterion.ctc_beam_search(xd, fd, beam=8, beam_token=5, nbest=2)          # without lm: the old call, three tensors
    lab, ln, sc = _search(x, frames, 8, 5, INF, False, False, 2, T)
    assert len(free) == 3 and (free[0].cpu().numpy() == lab).all() and (free[2].cpu().numpy().view(np.int32) == sc.view(np.int32)).all()
    with pytest.raises(ValueError, match="need lm"):
        criterion.ctc_beam_search(xd, fd, lm_weight=0.5)
    with pytest.raises(ValueError, match="tokens"):
        criterion.ctc_beam_search(xd, fd, lm=_table(LR.random_lm(rng, N, 2, 10)))
    with pytest.raises(ValueError):
        criterion.ctc_beam_search(xd, fd, lm=_table(LR.random_lm(rng, N - 1, 2, 10, eos=False)), eos_score=1.0)


def test_three_surfaces_agree(tmp_path):
    """C ABI == Python CTCLoss.beamSearch(lm=) == compiled C++ CTCLoss::beamSearch with BeamSearchOptions::lm
    (tests/cpp/decode_lm_caller.cpp, plain g++ against libw2l_hip.so), all three on a model read from the same ARPA file"""
    from wav2letter_amd import CTCLoss, NGramLM
    exe = str(tmp_path / "decode_lm_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "decode_lm_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    rng = np.random.default_rng(8)
    for B, T, N, W, K, M, Lmax, log_add, norm, thr, with_cls in [(4, 31, 30, 8, 5, 3, 31, 1, 1, INF, True),
                                                                 (2, 20, 30, 64, 64, 16, 6, 0, 0, 2.0, False)]:
        tokens = [f"t{c}" for c in range(N - 1)]
        tok_path, arpa = _arpa_files(tmp_path, LR.random_lm(rng, N - 1, 3, 200), tokens)
        lm = NGramLM.from_arpa(arpa, tokens)
        x = rng.normal(0, 2, size=(B, T, N)).astype(F32) if log_add else _ints(rng, B, T, N)
        frames = rng.integers(1, T + 1, B).astype(np.int32)
        frames[1] = 1
        cls = rng.normal(0, 0.3, N - 1).astype(F32) if with_cls else None
        lmw, eos_score = 0.75, -0.25
        want_f = _search_lm(x, frames, W, K, thr, log_add, norm, M, Lmax, lm, lmw, cls, eos_score)
        want = _search_lm(x, None, W, K, thr, log_add, norm, M, Lmax, lm, lmw, cls, eos_score)
        xd = torch.tensor(x, device="cuda")
        opts = dict(beam=W, beam_token=K, threshold=thr, log_add=bool(log_add), normalize=bool(norm), nbest=M, max_len=Lmax, lm=lm,
                    lm_weight=lmw, class_score=torch.tensor(cls, device="cuda") if with_cls else None, eos_score=eos_score)
        for got, ref in ((CTCLoss().beamSearch(xd, torch.tensor(frames, device="cuda"), **opts), want_f),
                         (CTCLoss().beamSearch(xd, **opts), want)):
            assert all((g.cpu().numpy().view(np.int32) == r.view(np.int32)).all() for g, r in zip(got, ref))
        inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(inp, "wb") as f:
            f.write(np.array([N, T, B, W, K, M, Lmax, log_add, norm, int(with_cls)], np.int32).tobytes()
                    + np.array([thr, lmw, eos_score], F32).tobytes() + x.tobytes() + frames.tobytes()
                    + (cls if with_cls else np.zeros(N - 1, F32)).tobytes())
        run = subprocess.run([exe, inp, outp, str(tok_path), str(arpa)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "decode lm caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
        got = np.fromfile(outp, np.int32)
        sizes = [B * M * Lmax, B * M, B * M, B * M]
        at = 0
        for ref in (want_f, want):
            for r, n in zip(ref, sizes):
                assert (got[at:at + n] == r.view(np.int32).ravel()).all()
                at += n
        assert at == len(got)


# ---- Decode --lm end to end, on the six-WAV fixture of tests/list_fixture.py ------------------------------------------------

from tests.list_fixture import ENV, LETTERS  # noqa: E402
from tests.test_gpu_ctc_beam import DECODE_EXE, trained  # noqa: E402,F401  (the module-scoped trained checkpoint)


def _dump_rows(d):
    rows = [line.split(" | ") for line in (d / "out" / "other.hyp").read_text().splitlines()]
    assert len(rows) == 15 and all(len(r) == 6 for r in rows)
    return rows


def test_decode_tool_with_lm_end_to_end(trained, tmp_path):
    d, model = trained
    tb = LR.random_lm(np.random.default_rng(2), len(LETTERS), 3, 250)
    _, arpa = _arpa_files(tmp_path, tb, LETTERS)
    base = [DECODE_EXE, f"--am={model}", "--test=sub/other.lst", "--batchsize=2", f"--sclite={d / 'out'}", "--isbeamdump=true", "--nbest=3",
            "--beamsize=16", "--beamthreshold=100"]

    def run(*extra):
        res = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600, env=ENV)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
        return _dump_rows(d), (d / "out" / "other.hyp").read_bytes()

    free, free_bytes = run()
    assert all(r[1] == r[2] and r[3] == "0.000000" for r in free)                   # without --lm: the format as it was
    zero, _ = run(f"--lm={arpa}", "--lmtype=kenlm")                                 # --lmweight defaults to 0: the same search
    assert [(r[0], r[1], r[5]) for r in zero] == [(r[0], r[1], r[5]) for r in free]
    assert all(float(r[3]) < 0 and r[2] == r[1] for r in zero)                      # and the lmScore column is filled
    lmw, eos = 0.7, -0.5
    rows, _ = run(f"--lm={arpa}", f"--lmweight={lmw}", f"--eosscore={eos}")
    changed = 0
    for k in range(5):
        mine = rows[3 * k:3 * k + 3]
        assert [r[0] for r in mine] == [f"u{k}"] * 3
        scores = [float(r[1]) for r in mine]
        assert scores == sorted(scores, reverse=True) and all(np.isfinite(scores))
        for r in mine:
            score, am, lms = float(r[1]), float(r[2]), float(r[3])
            assert lms < 0 and abs(score - (am + lmw * lms + eos)) <= 1e-4 * max(1.0, abs(score))
        changed += [r[5] for r in mine] != [r[5] for r in free[3 * k:3 * k + 3]]
    assert changed > 0                                                              # LM-weighted hypotheses
    ws = 0.25
    rows, _ = run(f"--lm={arpa}", f"--lmweight={lmw}", f"--eosscore={eos}", f"--wordscore={ws}")
    for r in rows:                                                                  # the word score: once per separator label
        n_sep = (float(r[1]) - (float(r[2]) + lmw * float(r[3]) + eos)) / ws
        assert abs(n_sep - round(n_sep)) <= 1e-3 and round(n_sep) >= max(len(r[5].split()) - 1, 0)
    again, again_bytes = run()
    assert again_bytes == free_bytes


@pytest.mark.parametrize("flags,name", [(["--lm=missing.arpa"], "--lm"), (["--lm=x.arpa", "--lmtype=convlm"], "convlm"),
                                        (["--lmweight=1", "--wordscore=0.5"], "--wordscore")])
def test_decode_tool_lm_refusals(trained, flags, name):
    d, model = trained
    res = subprocess.run([DECODE_EXE, f"--am={model}", "--test=sub/other.lst"] + flags, capture_output=True, text=True, timeout=120, env=ENV)
    assert res.returncode != 0 and name in res.stderr, (res.returncode, res.stderr)
