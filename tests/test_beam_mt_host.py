"""The many-token beam searches (w2l_*_beam_search*_mt, W up to 8192, K up to 256) without a GPU: the ten symbols exist with the
declared signatures, size their workspaces and refuse bad arguments in the xl twins' order -- every W2L_EINVAL, those of the
silence arguments included, before W2L_EUNSUPPORTED -- before anything touches the device; the xl twins still refuse K = 65; the
Python front end knows wide="mt"; the fl:: options carry `manyTokens` (a compiled C++ program); and the restatement with counts
of tests/beam_mt_ref.py, the oracle of tests/test_gpu_beam_mt.py, returns what the restatements it was written from return."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

INF = float("inf")
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (xl twin, workspace size of the mt twin, of the xl twin, has trans, has LM arguments, has lexicon arguments)
TWINS = {
    "w2l_ctc_beam_search_mt": ("w2l_ctc_beam_search_xl", "w2l_ctc_beam_mt_workspace_size", "w2l_ctc_beam_xl_workspace_size", 0, 0, 0),
    "w2l_ctc_beam_search_lm_mt": ("w2l_ctc_beam_search_lm_xl", "w2l_ctc_beam_lm_mt_workspace_size", "w2l_ctc_beam_lm_xl_workspace_size",
                                  0, 1, 0),
    "w2l_ctc_beam_search_lex_mt": ("w2l_ctc_beam_search_lex_xl", "w2l_ctc_beam_lex_mt_workspace_size",
                                   "w2l_ctc_beam_lex_xl_workspace_size", 0, 1, 1),
    "w2l_asg_beam_search_mt": ("w2l_asg_beam_search_xl", "w2l_asg_beam_mt_workspace_size", "w2l_asg_beam_xl_workspace_size", 1, 1, 0),
    "w2l_asg_beam_search_lex_mt": ("w2l_asg_beam_search_lex_xl", "w2l_asg_beam_lex_mt_workspace_size",
                                   "w2l_asg_beam_lex_xl_workspace_size", 1, 1, 1),
}


def _L():
    from wav2letter_amd import _lib
    return _lib


def _caller(name):
    """call(**overrides) of a many-token entry point or of its xl twin (the same list without the two silence arguments) on host
    pointers that are never read"""
    L = _L()
    fn = getattr(L.lib(), name)
    mt = name in TWINS
    _, _, _, trans, has_lm, has_lex = TWINS[name if mt else name[:-len("_xl")] + "_mt"]
    buf = np.zeros(64, np.uint8).ctypes.data

    def call(B=2, T=10, N=30, x=buf, tr=buf, W=8, K=8, thr=INF, M=2, Lmax=10, lm=buf, has_eos=1, lmw=1.0, cs=None, lex=buf, wsc=0.0,
             eos=0.0, labels=buf, lengths=buf, scores=buf, lms=buf, maxw=4, words=buf, counts=buf, ws=buf, sil=-1, sil_score=0.0):
        args = [B, T, N, x, None] + ([tr] if trans else []) + [W, K, thr, 0, 0, M, Lmax]
        if has_lex:
            args += [lm, has_eos, lmw, lex, wsc, eos, labels, lengths, scores, lms, maxw, words, counts]
        elif has_lm:
            args += [lm, has_eos, lmw, cs, eos, labels, lengths, scores, lms]
        else:
            args += [labels, lengths, scores]
        return fn(*args, ws, None, *([sil, sil_score] if mt else []))
    return call


def test_the_ten_symbols_are_declared_with_the_xl_twins_lists_and_the_silence_pair():
    L = _L()
    lib = L.lib()
    for name, (xl, size, xl_size, *_r) in TWINS.items():
        assert {name, size} <= set(L.exported_symbols())
        f, g = getattr(lib, name), getattr(lib, xl)
        assert f.restype is C.c_int and list(f.argtypes) == list(g.argtypes) + [C.c_int, C.c_float], name
        s = getattr(lib, size)
        assert s.restype is C.c_size_t and list(s.argtypes) == [C.c_int] * 5 == list(getattr(lib, xl_size).argtypes), size
    header = open(os.path.join(ROOT, "include", "w2l_hip.h")).read()
    for name, (_, size, *_r) in TWINS.items():
        assert f"int {name}(int B, int T, int N" in header and f"size_t {size}(int B, int T, int N, int beam, int beamToken);" in header


@pytest.mark.parametrize("name", list(TWINS))
def test_mt_twin_sizes_its_workspace_and_refuses_in_order(name):
    L = _L()
    xl_name, size_name, xl_size_name, trans, has_lm, has_lex = TWINS[name]
    size, xl_size = getattr(L.lib(), size_name), getattr(L.lib(), xl_size_name)
    slots = 7 if has_lex else 1
    # K after clipping up to 256: non-zero and monotone over the mask-word boundaries; beyond the limits: 0
    s = [size(2, 10, 400, 300, K) for K in (1, 64, 65, 128, 129, 256)]
    assert s[0] > 0 and all(a < b for a, b in zip(s, s[1:])), s
    assert size(2, 10, 400, 300, 257) == 0 and size(2, 10, 400, 8193, 8) == 0 and size(2, 10, 400, 8192, 256) > 0
    assert size(1, 1 << 17, 30, 8192, 8) == 0 and size(1, 1 << 16, 30, 8192, 8) > 0                 # T * W above 2^29
    assert size(0, 10, 30, 8, 8) == 0 and size(2, 0, 30, 8, 8) == 0 and size(2, 10, 1, 8, 8) == 0 and size(2, 10, 30, 0, 8) == 0
    assert size(2, 10, 30, 8, 0) == 0
    tokens = 200 if trans else 199
    assert size(2, 10, 200, 300, tokens) == size(2, 10, 200, 300, 256) == size(2, 10, 200, 300, 250000)     # K is clipped
    assert size(2, 10, 258, 300, 250000) == 0 and size(2, 10, 257 if not trans else 256, 300, 250000) > 0  # ... and then held to 256
    # at K <= 64 the xl twin's size (one mask word); above it the xl twin has none
    for W, K in ((1, 1), (300, 29), (1025, 64), (8192, 64)):
        assert size(2, 10, 400, W, K) >= xl_size(2, 10, 400, W, K) > 0, (W, K)
    assert xl_size(2, 10, 400, 300, 65) == 0
    # the candidate list is the worst case, W * K (* 7 with a lexicon) + W keys of 8 bytes per utterance, counted in size_t; the
    # masks are ceil(K / 64) words per (slot, entry)
    assert size(1, 3, 400, 8192, 256) >= 8 * (8192 * 256 * slots + 8192) + 8 * slots * 8192 * 4
    assert size(64, 3, 400, 8192, 256) >= 64 * 8 * (8192 * 256 * slots + 8192) > (1 << 32 if has_lex else 1 << 30)
    assert size(1, 3, 400, 1000, 129) - size(1, 3, 400, 1000, 128) >= 8 * slots * 1000 + 8 * 1000 * slots

    call, xl = _caller(name), _caller(xl_name)
    bad = [dict(B=0), dict(T=0), dict(N=1), dict(B=-1), dict(x=None), dict(labels=None), dict(lengths=None), dict(scores=None),
           dict(ws=None), dict(W=0), dict(K=0), dict(M=0), dict(M=9), dict(Lmax=0), dict(thr=-0.5), dict(thr=NAN), dict(thr=-INF),
           dict(W=2500, M=2501), dict(W=8192, M=8193),
           dict(sil_score=NAN), dict(sil_score=INF), dict(sil_score=-INF), dict(sil=-2), dict(sil=30 if trans else 29), dict(sil=1000)]
    if trans:
        bad += [dict(tr=None)]
    if has_lm:
        bad += [dict(lms=None), dict(lmw=INF), dict(lmw=NAN), dict(eos=NAN), dict(eos=-INF), dict(has_eos=0, eos=0.5)]
        bad += [dict(lm=None, has_eos=1)] if trans and not has_lex else [dict(lm=None)]
    if has_lex:
        bad += [dict(lex=None), dict(words=None), dict(counts=None), dict(maxw=0), dict(wsc=NAN), dict(wsc=INF)]
    for kw in bad:
        assert call(**kw) == L.W2L_EINVAL, kw
    for kw in (dict(W=8193, M=2), dict(W=100000, M=2), dict(N=400, K=257), dict(N=400, K=250000), dict(N=400, W=8192, K=257),
               dict(N=258, K=250000), dict(N=400, K=257, sil=5, sil_score=1.0)):
        assert call(**kw) == L.W2L_EUNSUPPORTED, kw
    assert call(T=1 << 17, W=8192) == L.W2L_EUNSUPPORTED                                     # T * W above 2^29: node ids are ints
    # every W2L_EINVAL comes before W2L_EUNSUPPORTED, the silence arguments' too
    for kw in (dict(W=8193, x=None), dict(W=8193, thr=-1.0), dict(W=8193, M=8194), dict(N=400, K=257, ws=None), dict(W=8193, Lmax=0),
               dict(W=8193, B=0), dict(N=400, K=257, labels=None), dict(W=8193, M=0), dict(W=8193, thr=NAN),
               dict(W=8193, sil_score=NAN), dict(N=400, K=257, sil=399 if not trans else 400), dict(W=8193, sil=-2),
               dict(T=1 << 17, W=8192, sil_score=INF)):
        assert call(**kw) == L.W2L_EINVAL, kw
    if trans:
        assert call(W=8193, tr=None) == L.W2L_EINVAL
    if has_lm:
        assert call(W=8193, lms=None) == L.W2L_EINVAL and call(W=8193, lmw=NAN) == L.W2L_EINVAL
        assert call(N=400, K=257, has_eos=0, eos=0.5) == L.W2L_EINVAL
    if has_lex:
        assert call(W=8193, lex=None) == L.W2L_EINVAL and call(N=400, K=257, maxw=0) == L.W2L_EINVAL
        assert call(W=8193, wsc=NAN) == L.W2L_EINVAL
    # the xl twin still refuses what the many-token twin takes, after its own W2L_EINVALs
    assert xl(N=400, K=65) == L.W2L_EUNSUPPORTED and xl(N=400, K=256) == L.W2L_EUNSUPPORTED and xl(N=66, K=250000) == L.W2L_EUNSUPPORTED
    assert xl(N=400, K=65, x=None) == L.W2L_EINVAL


def test_python_front_end_routes_mt():
    """criterion._beam_family: "mt" names the many-token family, whose descriptor call is the many-token twin (its size, the silence
    pair in the descriptor); an unknown string is refused with the accepted values named; lm_token=True has no many-token family"""
    L = _L()
    from wav2letter_amd import criterion
    lib = L.lib()
    assert criterion._beam_family("mt") == L.BEAM_MT == 3 and criterion._beam_family("xl") == L.BEAM_XL == 2
    for kind, stem in ((L.SEARCH_PLAIN, "w2l_ctc_beam"), (L.SEARCH_LM, "w2l_ctc_beam_lm"), (L.SEARCH_LEX, "w2l_ctc_beam_lex")):
        d = L.BeamSearchDesc(family=criterion._beam_family("mt"), kind=kind, B=2, T=10, N=400, beam=300, beamToken=200, silToken=3,
                             silScore=0.5)
        assert lib.w2l_beam_search_workspace_size(C.byref(d)) == getattr(lib, stem + "_mt_workspace_size")(2, 10, 400, 300, 200) > 0
    with pytest.raises(L.W2LInvalidArgument) as e:
        criterion._beam_family("many")
    assert all(v in str(e.value) for v in ("True", '"xl"', '"mt"'))
    with pytest.raises(L.W2LInvalidArgument):
        criterion._beam_family("mt", lm_token=True)
    # the silence pair rides in the descriptor: null pointers are refused by the library, then the limits, the silence token first
    buf = np.zeros(64, np.uint8).ctypes.data

    def call(x, K, sil=-1, sil_score=0.0):
        d = L.BeamSearchDesc(family=L.BEAM_MT, kind=L.SEARCH_PLAIN, B=2, T=10, N=400, input=x, beam=8, beamToken=K, threshold=INF,
                             nbest=2, maxLen=10, labels=buf, lengths=buf, scores=buf, silToken=sil, silScore=sil_score)
        return lib.w2l_beam_search(C.byref(d), buf, None)
    assert call(None, 257) == L.W2L_EINVAL
    assert call(buf, 257) == L.W2L_EUNSUPPORTED
    assert call(buf, 8, 399, 0.5) == L.W2L_EINVAL                                            # the blank is no silence token


def test_python_argument_checks_with_mt():
    """ctc_beam_search / asg_beam_search(wide="mt") refuse lm_token=True and an unknown `wide` before they touch a device"""
    torch = pytest.importorskip("torch")
    L = _L()
    from wav2letter_amd import criterion
    x = torch.zeros(1, 4, 6)
    with pytest.raises(L.W2LInvalidArgument):
        criterion.ctc_beam_search(x, wide="m")
    with pytest.raises(L.W2LInvalidArgument):
        criterion.asg_beam_search(x, torch.zeros(6, 6), wide="MT")
    for fn, args in ((criterion.ctc_beam_search, (x,)), (criterion.asg_beam_search, (x, torch.zeros(6, 6)))):
        with pytest.raises(L.W2LInvalidArgument) as e:
            fn(*args, wide="mt", lm_token=True)
        assert "many-token" in str(e.value)
        with pytest.raises(L.W2LError) as e:                     # "mt" itself passes: the tensor on the CPU is what is refused
            fn(*args, wide="mt", beam=8192, beam_token=256)
        assert "GPU only" in str(e.value)


def test_cpp_options_carry_many_tokens(tmp_path):
    """tests/cpp/beam_mt_options_test.cpp, plain g++ against libw2l_hip.so: BeamSearchOptions{}.manyTokens == false; with wide, xl
    or lmToken it throws std::invalid_argument; the streaming decoder refuses it"""
    exe, libdir = str(tmp_path / "beam_mt_options_test"), os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "beam_mt_options_test.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "beam mt options ok" in run.stdout, (run.returncode, run.stdout, run.stderr)


@pytest.mark.parametrize("kind", ["ctc", "ctc_lm", "ctc_lex", "asg", "asg_lm", "asg_lex"])
def test_the_restatement_with_counts_is_the_restatements(kind):
    """tests/beam_mt_ref.py against the restatements it must not differ from (tests/*_beam_ref.py through the wide tests' Case),
    both (+) modes, with a threshold line, at a K above 64 -- and its counts are counts of that search: the merges are the other
    restatements' where they count them"""
    from tests import beam_mt_ref as MR
    from tests.test_gpu_beam_wide import F32, KEYS, _dense_case
    c = _dense_case(kind, 41, 2, 5, 90, [5, 3], hot=80, nwords=400, max_len=2)
    for dtype, log_add, thr in ((F32, False, INF), (F32, False, 2.5), (np.float64, True, INF)):
        norm = log_add and not c.asg
        want = c.ref(60, 70, 60, 5, dtype, thr, log_add, norm, 4)
        got = MR.case_ref(c, 60, 70, 60, 5, dtype, thr, log_add, norm, 4)
        for k in KEYS:
            assert (k in got) == (k in want), k
            if k in want:
                assert got[k].dtype == want[k].dtype and (got[k] == want[k]).all(), (k, log_add, thr)
        assert (want["lengths"] >= 0).any()
        if kind != "ctc" and not log_add:
            assert [sum(map(sum, d.merges)) for d in got["diags"]] == c.merges(60, 70, thr, want["diags"])
        assert all(len(d.tokens[0]) == 70 for d in got["diags"])
