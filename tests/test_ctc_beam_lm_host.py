"""The n-gram LM table (w2l_ngram_lm_*) against a textbook back-off scorer, the ARPA reader, the restatement of the LM-fused beam
search (tests/ctc_beam_lm_ref.py) against the enumeration of every path, and w2l_ctc_beam_search_lm's refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import ctc_beam_lm_ref as LR
from tests import ctc_beam_ref as R

INF = float("inf")
F32 = np.float32
LN10 = 2.302585092994045684


def _pkg():
    from wav2letter_amd import NGramLM, _lib
    return NGramLM, _lib


def _table(tb):
    return _pkg()[0].from_ngrams(tb.arrays(), tb.V, float(tb.unk))


# ---- 1. the table against the textbook -----------------------------------------------------------------------------------

MODELS = {  # name: (V, order, n-grams drawn per order, bos, eos, classes without unigram)
    "order1": (7, 1, 0, True, True, ()),
    "order1_bare": (5, 1, 0, False, False, (2,)),
    "order2": (6, 2, 20, True, True, (4,)),
    "order2_no_bos": (6, 2, 20, False, True, ()),
    "order3": (5, 3, 30, True, True, (0,)),
    "order3_no_eos": (5, 3, 30, True, False, ()),
    "order5": (4, 5, 40, True, True, (3,)),
    "order5_bare": (4, 5, 40, False, False, ()),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_table_equals_the_textbook_scorer(name):
    V, order, per, bos, eos, drop = MODELS[name]
    rng = np.random.default_rng(len(name) * 7 + order)
    tb = LR.random_lm(rng, V, order, per, bos, eos, drop)
    lm = _table(tb)
    assert (lm.order, lm.num_tokens, lm.has_bos, lm.has_eos) == (order, V, bos, eos)
    assert lm.num_states == 1 + sum(1 for g in tb.p if len(g) < order)
    childless = [g for g in tb.bo if not any(h[:-1] == g for h in tb.p if len(h) == len(g) + 1)]
    if order >= 3:
        assert any(len(g) >= 2 for g in childless)                    # contexts listed with a back-off and no extension
    worst = 0.0
    for walk in range(30):
        state, hist = lm.start, tb.history(())
        for step in range(12):
            w = int(rng.integers(V)) if (not eos or rng.random() > 0.1) else tb.eos
            got, state = lm.score(state, w)
            want = tb.score(hist, w, F32)
            assert got.view(np.int32) == want.view(np.int32), (name, hist, w, got, want)
            w64 = tb.score(hist, w, np.float64)
            worst = max(worst, abs(float(got) - w64) / abs(w64))
            hist = hist + (w,)
    print("table", name, "states", lm.num_states, "longest back-off chain", tb.max_chain, "worst relative error against float64", worst)
    assert worst <= 1e-5                                              # fp32 storage and at most order + 1 adds
    assert tb.max_chain >= min(order - 1, 2)
    if drop:
        got, nxt = lm.score(lm.start, drop[0])                        # a class without unigram: back-offs, then <unk>, state 0
        assert nxt == 0 and got.view(np.int32) == tb.score(tb.history(()), drop[0], F32).view(np.int32)


def test_start_state_and_bounds():
    NGramLM, L = _pkg()
    tb = LR.random_lm(np.random.default_rng(0), 4, 3, 10)
    lm = _table(tb)
    assert lm.start != 0 and (lm.bos, lm.eos) == (4, 5)
    assert _table(LR.random_lm(np.random.default_rng(0), 4, 3, 10, bos=False)).start == 0
    for state, word in ((-1, 0), (lm.num_states, 0), (0, -1), (0, 6)):
        with pytest.raises(ValueError, match="out of range"):
            lm.score(state, word)
    with pytest.raises(ValueError, match="not a table"):
        NGramLM(np.zeros(256, np.uint8))


# ---- 2. ARPA ----------------------------------------------------------------------------------------------------------------

def _arpa_text(tb, tokens, unk10=None, extra=None, counts=None, end=True):
    """tb's n-grams in arrays() order with log10 values of four decimals; extra: {order: [lines]} appended to that section"""
    spell = {i: t for i, t in enumerate(tokens)}
    spell[tb.bos], spell[tb.eos] = "<s>", "</s>"
    sections, listed = [], {}
    for k in range(1, tb.order + 1):
        lines = []
        for g in sorted(g for g in tb.p if len(g) == k):
            p10 = round(float(tb.p[g]) / LN10, 4)
            b10 = round(float(tb.bo.get(g, 0)) / LN10, 4)
            listed[g] = (F32(p10 * LN10), F32(b10 * LN10))
            lines.append(f"{p10:.4f}\t{' '.join(spell[w] for w in g)}" + (f"\t{b10:.4f}" if k < tb.order else ""))
        if k == 1 and unk10 is not None:
            lines.insert(1, f"{unk10:.4f}\t<unk>")
        lines += (extra or {}).get(k, [])
        sections.append(lines)
    out = ["a comment before the data", "\\data\\"]
    out += [f"ngram {k + 1}={(counts or {}).get(k + 1, len(s))}" for k, s in enumerate(sections)]
    for k, s in enumerate(sections):
        out += ["", f"\\{k + 1}-grams:"] + s
    out += ["", "\\end\\"] if end else []
    return "\n".join(out) + "\n", listed


TOKENS = ["|", "a", "b", "_c", "d"]


def _arpa_model():
    return LR.random_lm(np.random.default_rng(11), len(TOKENS), 3, 25)


def test_arpa_round_trips_to_the_table_of_its_converted_values(tmp_path):
    NGramLM, _ = _pkg()
    tb = _arpa_model()
    extra = {1: ["-2.5000\tzzz\t-0.1000"], 2: ["-1.0000\ta zzz\t-0.2000", "-1.5000\tyyy b"], 3: ["-0.7000\ta b <unk>"]}
    text, listed = _arpa_text(tb, TOKENS, unk10=-3.25, extra=extra)
    path = tmp_path / "lm.arpa"
    path.write_text(text)
    lm = NGramLM.from_arpa(path, TOKENS)
    assert lm.skipped == 4 and "skipped 4 n-grams" in lm.message
    want = _table(LR.TextbookLM(listed, len(TOKENS), F32(-3.25 * LN10)))
    assert (lm.order, lm.start, lm.has_bos, lm.has_eos) == (3, want.start, True, True)
    assert np.array_equal(lm.blob, want.blob)
    conv = LR.TextbookLM(listed, len(TOKENS), F32(-3.25 * LN10))
    rng = np.random.default_rng(3)
    state, hist = lm.start, conv.history(())
    for _ in range(40):
        w = int(rng.integers(len(TOKENS)))
        got, state = lm.score(state, w)
        assert got.view(np.int32) == conv.score(hist, w, F32).view(np.int32)
        hist += (w,)


def test_arpa_class_without_unigram_scores_as_unk(tmp_path):
    NGramLM, _ = _pkg()
    tb = LR.random_lm(np.random.default_rng(5), len(TOKENS), 2, 10, drop_unigrams=(3,))
    path = tmp_path / "lm.arpa"
    path.write_text(_arpa_text(tb, TOKENS, unk10=-4.0)[0])
    lm = NGramLM.from_arpa(path, TOKENS)
    got, nxt = lm.score(0, 3)
    assert nxt == 0 and got == F32(-4.0 * LN10) and lm.skipped == 0
    path.write_text(_arpa_text(tb, TOKENS)[0])
    with pytest.raises(ValueError, match="token `_c` has no unigram and the file has no <unk>"):
        NGramLM.from_arpa(path, TOKENS)


def test_arpa_refusals(tmp_path):
    NGramLM, _ = _pkg()
    tb = _arpa_model()
    path = tmp_path / "lm.arpa"

    def refused(text, match, binary=False):
        path.write_bytes(text if binary else text.encode())
        with pytest.raises(ValueError, match=match):
            NGramLM.from_arpa(path, TOKENS)

    good, _ = _arpa_text(tb, TOKENS, unk10=-3.0)
    refused(_arpa_text(tb, TOKENS, unk10=-3.0, counts={2: 999})[0], "declares 999 2-grams, the section holds")
    refused(_arpa_text(tb, TOKENS, unk10=-3.0, end=False)[0], r"ends before \\end\\")
    refused(good[:good.rfind("\n", 0, len(good) // 2) + 1], r"ends before \\end\\")     # truncated between two lines of a section
    refused(good[:good.index("\t", len(good) // 2) + 1], "-gram line has 1 fields")      # and in the middle of a line
    refused(b"mmap lm http://kheafield.com/code format version 5\n\x00\x01", "KenLM binary file; supply the ARPA text", binary=True)
    refused(b"\x1f\x8b\x08\x00rest", "gzip is not read", binary=True)
    refused("no data here\n", r"no \\data\\ section")
    refused(good.replace("\\2-grams:", "\\3-grams:", 1), "out of order")
    refused(_arpa_text(tb, TOKENS, unk10=-3.0, extra={1: ["nan\tzzz"]})[0], "not a finite number")
    refused(_arpa_text(tb, TOKENS, unk10=-3.0, extra={1: ["-1.0"]})[0], "1-gram line has 1 fields")
    refused(_arpa_text(tb, TOKENS, unk10=-3.0, extra={1: ["-1.0000\ta\t-0.5000"]})[0], "duplicate 1-gram")
    pair = next((a, b) for a in range(5) for b in range(5) if (a, b) not in tb.p)
    orphan = f"-1.0000\t{TOKENS[pair[0]]} {TOKENS[pair[1]]} a"
    refused(_arpa_text(tb, TOKENS, unk10=-3.0, extra={3: [orphan]})[0], "is not itself an n-gram")
    with pytest.raises(ValueError, match="cannot read"):
        NGramLM.from_arpa(tmp_path / "missing.arpa", TOKENS)
    path.write_text(good)
    assert NGramLM.from_arpa(path, TOKENS).skipped == 0                         # and the unharmed file loads


def test_build_refusals():
    NGramLM, L = _pkg()
    uni = ([[0], [1], [2]], [-1.0, -2.0, -3.0], [-0.5, -0.5, -0.5])

    def refused(ngrams, match, V=3, unk=-5.0, exc=ValueError):
        with pytest.raises(exc, match=match):
            NGramLM.from_ngrams(ngrams, V, unk)

    refused([uni, ([[0, 1], [3, 1]], [-1.0, -1.0], None)], "context of the 2-gram .3 1. is not itself an n-gram", V=4)
    refused([uni, ([[0, 1], [0, 1]], [-1.0, -1.0], None)], "duplicate 2-gram")
    refused([([[0], [5]], [-1.0, -1.0], None)], "word id out of range")         # V = 3: BOS 3, EOS 4
    refused([([[0], [-1]], [-1.0, -1.0], None)], "word id out of range")
    refused([([[0], [1]], [-1.0, -np.inf], None)], "non-finite value")
    refused([([[0], [1]], [-1.0, -1.0], [0.0, np.nan]), ([[0, 1]], [-1.0], None)], "non-finite value")
    refused([uni], "<unk> log-probability is not finite", unk=np.nan)
    chain = [([[0] * k], [-1.0], [-0.5]) for k in range(1, 10)]
    with pytest.raises(L.W2LError, match="order 9 is above the format's 8") as err:
        NGramLM.from_ngrams(chain, 3, -5.0)
    assert not isinstance(err.value, ValueError)                                # W2L_EUNSUPPORTED, not W2L_EINVAL
    assert NGramLM.from_ngrams(chain[:6], 3, -5.0).order == 6
    size = C.c_size_t(16)                                                       # the second call with too little room
    counts = (C.c_size_t * 1)(3)
    w, p = np.array([0, 1, 2], np.int32), np.array([-1, -2, -3], F32)
    room = np.zeros(64, np.uint8)
    assert L.lib().w2l_ngram_lm_build(1, C.addressof(counts), w.ctypes.data, p.ctypes.data, None, 3, -5.0, room.ctypes.data,
                                      C.addressof(size)) == L.W2L_EINVAL
    assert b"bytes" in L.lib().w2l_host_last_error()


# ---- 3. the search restatement against the enumeration of every path -------------------------------------------------------

@pytest.mark.parametrize("log_add", [False, True])
@pytest.mark.parametrize("N,T", [(3, 5), (4, 3)])
def test_restatement_ranks_every_labelling_as_the_enumeration_does(N, T, log_add):
    rng = np.random.default_rng(N * 10 + T)
    tb = LR.random_lm(rng, N - 1, 3, 12)
    cls = rng.normal(0, 0.5, N - 1)
    lmw, eos_score = 0.7, -0.4
    worst, nonmono = 0.0, 0
    for seed in range(3):
        x = np.random.default_rng(seed).normal(0, 2, size=(T, N)).astype(F32)
        hyps, dg = LR.beam_search_lm_one(x, T, 64, N - 1, tb, lmw, cls, eos_score, INF, log_add, log_add, np.float64, None,
                                         lm_dtype=np.float64)
        enum = R.enumerate_labellings(x, log_add, log_add)
        want = {lab: s + lmw * float(tb.sentence(lab, np.float64)) + float(sum(cls[c] for c in lab)) + eos_score
                for lab, s in enum.items()}
        assert {p for p, _, _ in hyps} == set(want) and len(hyps) == len(want) == 25
        worst = max(worst, max(abs(s - want[p]) for p, s, _ in hyps))
        assert [p for p, _, _ in hyps] == sorted(want, key=lambda lab: -want[lab])
        nonmono += dg.nonmonotone
        assert dg.merges > 0
    print("enumeration", (N, T), "logAdd", log_add, "worst |score - enumeration|", worst, "non-monotone lanes", nonmono)
    assert worst <= 1e-9
    # lanes whose REGULAR extensions (the own-label one apart, as the LM-free kernel already treats it) are out of order: there the
    # LM-free kernel's lazy selection would not hold.  A deliberate limit of this assertion: at N = 3 there are two tokens, only the
    # empty prefix has two regular extensions and the count may be 0 (it is printed); the N = 4 shape must show such lanes.
    assert nonmono > 0 or N == 3


# ---- 4. lmWeight = 0 is the LM-free search ----------------------------------------------------------------------------------

@pytest.mark.parametrize("W,K,thr", [(64, 64, INF), (6, 3, INF), (16, 5, 2.5), (1, 1, INF)])
def test_zero_weight_is_the_lm_free_restatement(W, K, thr):
    rng = np.random.default_rng(W + K)
    B, T, N, M = 3, 14, 12, min(W, 8)
    x = (rng.integers(-24, 1, size=(B, T, N)) / 8).astype(F32)
    frames = [14, 5, 9]
    for eos in (False, True):
        tb = LR.random_lm(rng, N - 1, 3, 40, eos=eos)
        lab, ln, sc, lms, _ = LR.beam_search_lm(x, frames, W, K, tb, 0.0, None, 0.0, thr, False, False, M, T, F32)
        rlab, rln, rsc, _ = R.beam_search(x, frames, W, K, thr, False, False, M, T, F32)
        assert np.array_equal(lab, rlab) and np.array_equal(ln, rln) and np.array_equal(sc, rsc)
        assert (np.isfinite(lms) == (ln >= 0)).all()


# ---- 5. refusals of the C ABI, before anything touches the device -----------------------------------------------------------

def test_search_refusals_return_before_the_device():
    _, L = _pkg()
    lib = L.lib()
    buf = np.zeros(64, np.uint8).ctypes.data                                    # never read: every call below is refused first
    nan = float("nan")

    def call(B=2, T=10, N=30, x=buf, W=8, K=8, thr=INF, M=2, Lmax=10, lm=buf, has_eos=1, lmw=1.0, cls=None, eos=0.0, labels=buf,
             lengths=buf, scores=buf, lms=buf, ws=buf):
        return lib.w2l_ctc_beam_search_lm(B, T, N, x, None, W, K, thr, 0, 0, M, Lmax, lm, has_eos, lmw, cls, eos, labels, lengths,
                                          scores, lms, ws, None)

    for kw in (dict(lm=None), dict(lms=None), dict(x=None), dict(labels=None), dict(lengths=None), dict(scores=None), dict(ws=None),
               dict(lmw=INF), dict(lmw=nan), dict(eos=nan), dict(eos=-INF), dict(has_eos=0, eos=0.5), dict(thr=nan), dict(thr=-1.0),
               dict(M=9), dict(M=0), dict(W=0), dict(K=0), dict(Lmax=0), dict(N=1), dict(B=0), dict(T=0)):
        assert call(**kw) == L.W2L_EINVAL, kw
    for kw in (dict(W=65, M=2), dict(K=65, N=100)):
        assert call(**kw) == L.W2L_EUNSUPPORTED, kw
    assert lib.w2l_ctc_beam_lm_workspace_size(2, 10, 30, 65, 8) == 0 and lib.w2l_ctc_beam_lm_workspace_size(2, 10, 100, 8, 65) == 0
    assert lib.w2l_ctc_beam_lm_workspace_size(0, 10, 30, 8, 8) == 0
    assert lib.w2l_ctc_beam_lm_workspace_size(2, 10, 30, 8, 65) == lib.w2l_ctc_beam_lm_workspace_size(2, 10, 30, 8, 29)   # K clipped
    assert lib.w2l_ctc_beam_lm_workspace_size(32, 188, 9998, 64, 64) >= lib.w2l_ctc_beam_workspace_size(32, 188, 9998, 64, 64) + 2 * 32 * 64 * 4


def test_python_front_end_refuses_bad_lm_options_before_the_device():
    """the LM option checks come before the device checks: CPU tensors reach them"""
    import torch
    from wav2letter_amd import criterion
    NGramLM, L = _pkg()
    x = torch.zeros(1, 4, 6)
    rng = np.random.default_rng(0)
    for kw in (dict(lm_weight=0.5), dict(eos_score=-1.0), dict(class_score=torch.zeros(5))):
        with pytest.raises(ValueError, match="need lm"):
            criterion.ctc_beam_search(x, **kw)
    with pytest.raises(ValueError, match="the LM has 6 tokens, the emissions 5"):
        criterion.ctc_beam_search(x, lm=_table(LR.random_lm(rng, 6, 2, 5)))
    with pytest.raises(ValueError, match="eos_score needs a model with EOS"):
        criterion.ctc_beam_search(x, lm=_table(LR.random_lm(rng, 5, 2, 5, eos=False)), eos_score=1.0)
    for bad in (torch.zeros(4), torch.zeros(5, dtype=torch.float64)):
        with pytest.raises(ValueError, match="class_score must be float32"):
            criterion.ctc_beam_search(x, lm=_table(LR.random_lm(rng, 5, 2, 5)), class_score=bad)
    with pytest.raises(L.W2LError, match="GPU only"):                 # a well-formed LM call on CPU tensors: no CPU fallback
        criterion.ctc_beam_search(x, lm=_table(LR.random_lm(rng, 5, 2, 5)), lm_weight=0.5)


def test_cpp_lm_header_and_text_glue_through_a_compiled_caller(tmp_path):
    """include/fl_compat/lm.h (NGramLM::fromArpa, score, sentence, the library's messages as exceptions) and tknLabels2Wrd on a
    label row, through tests/cpp/lm_text_test.cpp compiled here with g++: every printed value equals the Python front end's"""
    import os
    import subprocess
    from wav2letter_amd import text
    NGramLM, _ = _pkg()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = str(tmp_path / "lm_text_test"), os.path.join(root, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "lm_text_test.cpp"),
                    "-o", exe, "-L" + libdir, "-lw2l_hip", "-Wl,-rpath," + libdir, "-ldl"], check=True)
    tb = _arpa_model()
    (tmp_path / "tokens.txt").write_text("\n".join(TOKENS) + "\n")
    (tmp_path / "lm.arpa").write_text(_arpa_text(tb, TOKENS, unk10=-3.0, extra={2: ["-1.0000\ta zzz"]})[0])
    lm = NGramLM.from_arpa(tmp_path / "lm.arpa", TOKENS)
    walk = [1, 2, 0, 3, 4, 0, 1, 1, lm.eos]
    run = subprocess.run([exe, str(tmp_path / "tokens.txt"), str(tmp_path / "lm.arpa"), "|"] + [str(w) for w in walk], capture_output=True,
                         text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert lines[0].split() == ["info"] + [str(int(v)) for v in (lm.order, lm.num_tokens, lm.num_states, lm.start, lm.has_bos, lm.has_eos, 1)]
    state, acc = lm.start, F32(0)
    for w, line in zip(walk, lines[1:]):
        p, state = lm.score(state, w)
        tag, hexp, nxt = line.split()
        assert tag == "q" and F32(float.fromhex(hexp)).view(np.int32) == p.view(np.int32) and int(nxt) == state
    row = walk[:-1]
    state = lm.start
    for w in row + [lm.eos]:
        p, state = lm.score(state, w)
        acc = F32(acc + p)
    assert lines[len(walk) + 1].split()[0] == "sentence" and F32(float.fromhex(lines[len(walk) + 1].split()[1])).view(np.int32) == acc.view(np.int32)
    dic = text.Dictionary(TOKENS)
    assert lines[len(walk) + 2] == "words " + " ".join(text.tkn_labels_to_wrd(row, dic, "ctc", wordsep="|"))
    assert lines[len(walk) + 3] == "refused ngram lm: state out of range"
    (tmp_path / "bad.arpa").write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\x00")
    run = subprocess.run([exe, str(tmp_path / "tokens.txt"), str(tmp_path / "bad.arpa"), "|"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.startswith("refused arpa ") and "KenLM binary file; supply the ARPA text" in run.stdout
