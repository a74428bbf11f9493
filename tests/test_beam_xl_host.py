"""The xl beam searches (w2l_*_beam_search*_xl, W up to 8192) without a GPU: the five twins exist, size their workspaces and refuse
bad arguments in their siblings' order -- every W2L_EINVAL before W2L_EUNSUPPORTED -- before anything touches the device; the wide
entry points still refuse W = 1025; the Python front end knows wide="xl" and nothing else but False / True; and the fl:: options
carry `xl` (false by default, refused together with `wide`), checked by a compiled C++ program.  The oracle of
tests/test_gpu_beam_xl.py is the set of numpy restatements tests/test_beam_wide_host.py holds against an enumeration."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

INF = float("inf")
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (wide twin, workspace size of the xl twin, of the wide twin, has trans, has LM arguments, has lexicon arguments)
TWINS = {
    "w2l_ctc_beam_search_xl": ("w2l_ctc_beam_search_wide", "w2l_ctc_beam_xl_workspace_size", "w2l_ctc_beam_wide_workspace_size", 0, 0, 0),
    "w2l_ctc_beam_search_lm_xl": ("w2l_ctc_beam_search_lm_wide", "w2l_ctc_beam_lm_xl_workspace_size",
                                  "w2l_ctc_beam_lm_wide_workspace_size", 0, 1, 0),
    "w2l_ctc_beam_search_lex_xl": ("w2l_ctc_beam_search_lex_wide", "w2l_ctc_beam_lex_xl_workspace_size",
                                   "w2l_ctc_beam_lex_wide_workspace_size", 0, 1, 1),
    "w2l_asg_beam_search_xl": ("w2l_asg_beam_search_wide", "w2l_asg_beam_xl_workspace_size", "w2l_asg_beam_wide_workspace_size", 1, 1, 0),
    "w2l_asg_beam_search_lex_xl": ("w2l_asg_beam_search_lex_wide", "w2l_asg_beam_lex_xl_workspace_size",
                                   "w2l_asg_beam_lex_wide_workspace_size", 1, 1, 1),
}


def _L():
    from wav2letter_amd import _lib
    return _lib


def _caller(name):
    """call(**overrides) of entry point `name` (an xl twin or a wide one: one argument list) on host pointers that are never read"""
    L = _L()
    fn = getattr(L.lib(), name)
    _, _, _, trans, has_lm, has_lex = TWINS[name if name in TWINS else name[:-len("_wide")] + "_xl"]
    buf = np.zeros(64, np.uint8).ctypes.data

    def call(B=2, T=10, N=30, x=buf, tr=buf, W=8, K=8, thr=INF, M=2, Lmax=10, lm=buf, has_eos=1, lmw=1.0, cs=None, lex=buf, wsc=0.0,
             eos=0.0, labels=buf, lengths=buf, scores=buf, lms=buf, maxw=4, words=buf, counts=buf, ws=buf):
        args = [B, T, N, x, None] + ([tr] if trans else []) + [W, K, thr, 0, 0, M, Lmax]
        if has_lex:
            args += [lm, has_eos, lmw, lex, wsc, eos, labels, lengths, scores, lms, maxw, words, counts]
        elif has_lm:
            args += [lm, has_eos, lmw, cs, eos, labels, lengths, scores, lms]
        else:
            args += [labels, lengths, scores]
        return fn(*args, ws, None)
    return call


@pytest.mark.parametrize("name", list(TWINS))
def test_xl_twin_exists_sizes_its_workspace_and_refuses_in_order(name):
    L = _L()
    wide_name, size_name, wide_size_name, trans, has_lm, has_lex = TWINS[name]
    assert {name, size_name} <= set(L.exported_symbols())
    size, wide_size = getattr(L.lib(), size_name), getattr(L.lib(), wide_size_name)
    # every W in 1..8192 is accepted, the size is monotone in W (and in B, T, K); beyond the limits: 0
    s = [size(2, 10, 100, W, 8) for W in (1, 64, 1024, 1025, 2500, 5000, 8192)]
    assert s[0] > 0 and all(a < b for a, b in zip(s, s[1:])), s
    assert size(2, 10, 100, 8193, 8) == 0 and size(2, 10, 100, 8, 65) == 0 and size(2, 10, 100, 8192, 64) > 0
    assert size(0, 10, 30, 8, 8) == 0 and size(2, 0, 30, 8, 8) == 0 and size(2, 10, 1, 8, 8) == 0 and size(2, 10, 30, 0, 8) == 0
    assert size(2, 10, 30, 2500, 8) < size(4, 10, 30, 2500, 8) and size(2, 10, 30, 2500, 8) < size(2, 20, 30, 2500, 8)
    assert size(2, 10, 100, 2500, 8) < size(2, 10, 100, 2500, 64)
    tokens = 30 if trans else 29
    assert size(2, 10, 30, 2500, tokens) == size(2, 10, 30, 2500, 64) == size(2, 10, 30, 2500, 250000)     # K is clipped
    # the beam, the gone masks and the stays are in the workspace: more than the wide twin's at a width both take
    assert size(2, 10, 100, 1024, 8) > wide_size(2, 10, 100, 1024, 8) > 0
    assert wide_size(2, 10, 100, 1025, 8) == 0                                                             # the wide limit stays
    # the candidate list is the worst case, W * K (* 7 with a lexicon) + W keys of 8 bytes per utterance
    assert size(1, 4, 100, 8192, 64) >= 8 * (8192 * 64 * (7 if has_lex else 1) + 8192)

    call, wide = _caller(name), _caller(wide_name)
    bad = [dict(B=0), dict(T=0), dict(N=1), dict(B=-1), dict(x=None), dict(labels=None), dict(lengths=None), dict(scores=None),
           dict(ws=None), dict(W=0), dict(K=0), dict(M=0), dict(M=9), dict(Lmax=0), dict(thr=-0.5), dict(thr=NAN), dict(thr=-INF),
           dict(W=2500, M=2501), dict(W=8192, M=8193)]
    if trans:
        bad += [dict(tr=None)]
    if has_lm:
        bad += [dict(lms=None), dict(lmw=INF), dict(lmw=NAN), dict(eos=NAN), dict(eos=-INF), dict(has_eos=0, eos=0.5)]
        bad += [dict(lm=None, has_eos=1)] if trans and not has_lex else [dict(lm=None)]
    if has_lex:
        bad += [dict(lex=None), dict(words=None), dict(counts=None), dict(maxw=0), dict(wsc=NAN), dict(wsc=INF)]
    for kw in bad:
        assert call(**kw) == L.W2L_EINVAL, kw
    for kw in (dict(W=8193, M=2), dict(W=100000, M=2), dict(N=100, K=65), dict(N=100, K=250000), dict(N=100, W=8192, K=65)):
        assert call(**kw) == L.W2L_EUNSUPPORTED, kw
    assert call(T=1 << 17, W=8192) == L.W2L_EUNSUPPORTED                                     # T * W above 2^29: node ids are ints
    # every W2L_EINVAL comes before W2L_EUNSUPPORTED
    for kw in (dict(W=8193, x=None), dict(W=8193, thr=-1.0), dict(W=8193, M=8194), dict(N=100, K=65, ws=None), dict(W=8193, Lmax=0),
               dict(W=8193, B=0), dict(N=100, K=65, labels=None), dict(W=8193, M=0), dict(W=8193, thr=NAN)):
        assert call(**kw) == L.W2L_EINVAL, kw
    if trans:
        assert call(W=8193, tr=None) == L.W2L_EINVAL
    if has_lm:
        assert call(W=8193, lms=None) == L.W2L_EINVAL and call(W=8193, lmw=NAN) == L.W2L_EINVAL
        assert call(N=100, K=65, has_eos=0, eos=0.5) == L.W2L_EINVAL
    if has_lex:
        assert call(W=8193, lex=None) == L.W2L_EINVAL and call(N=100, K=65, maxw=0) == L.W2L_EINVAL
        assert call(W=8193, wsc=NAN) == L.W2L_EINVAL
    # the wide twin still refuses what the xl twin takes
    assert wide(W=1025, M=2) == L.W2L_EUNSUPPORTED and wide(W=8192, M=2) == L.W2L_EUNSUPPORTED
    assert wide(W=1025, x=None) == L.W2L_EINVAL and wide(W=1024, M=1025) == L.W2L_EINVAL


def test_python_front_end_routes_wide_xl():
    """criterion._beam_family: False the narrow family, True the wide one, "xl" the xl one, any other string refused; the
    descriptor call with that family is the named twin: its size, and its refusal of a beam above the family's limit"""
    L = _L()
    from wav2letter_amd import criterion
    lib = L.lib()
    assert [criterion._beam_family(w) for w in (False, True, "xl")] == [L.BEAM_NARROW, L.BEAM_WIDE, L.BEAM_XL] == [0, 1, 2]
    with pytest.raises(L.W2LInvalidArgument):
        criterion._beam_family("xxl")
    buf = np.zeros(64, np.uint8).ctypes.data
    for wide, suffix, limit in ((False, "", 64), (True, "_wide", 1024), ("xl", "_xl", 8192)):
        for kind, stem in ((L.SEARCH_LM, "w2l_ctc_beam_lm"), (L.SEARCH_LEX, "w2l_ctc_beam_lex")):
            d = L.BeamSearchDesc(family=criterion._beam_family(wide), kind=kind, B=2, T=10, N=30, beam=limit, beamToken=8, silToken=-1)
            assert lib.w2l_beam_search_workspace_size(C.byref(d)) == getattr(lib, stem + suffix + "_workspace_size")(2, 10, 30, limit, 8) > 0
            d.beam = limit + 1
            assert lib.w2l_beam_search_workspace_size(C.byref(d)) == 0
        d = L.BeamSearchDesc(family=criterion._beam_family(wide), kind=L.SEARCH_PLAIN, B=2, T=10, N=30, input=buf, beam=limit + 1,
                             beamToken=8, threshold=INF, nbest=2, maxLen=10, labels=buf, lengths=buf, scores=buf, silToken=-1)
        assert lib.w2l_beam_search(C.byref(d), buf, None) == L.W2L_EUNSUPPORTED
        d.input = None
        assert lib.w2l_beam_search(C.byref(d), buf, None) == L.W2L_EINVAL


def test_cpp_options_carry_xl(tmp_path):
    """tests/cpp/beam_xl_options_test.cpp, plain g++ against libw2l_hip.so: BeamSearchOptions{}.xl == false, xl && wide throws
    std::invalid_argument"""
    exe, libdir = str(tmp_path / "beam_xl_options_test"), os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "beam_xl_options_test.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "beam xl options ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
