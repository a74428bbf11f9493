"""w2l_beam_search / w2l_beam_search_workspace_size without a GPU: the descriptor call is defined by the named entry point that
(trans ? asg : ctc, kind, family) names, so on a grid of calls with exactly one spoiled argument (and with two, one W2L_EINVAL and
one W2L_EUNSUPPORTED) it returns that entry point's code and that entry point's workspace size; and its own refusals -- a null
descriptor, an enumerator out of range, the token LM under a lexicon beyond the wide family, a field the chosen search does not
take.  Refusals and sizes are host arithmetic: nothing here touches a device, every pointer is a host buffer that is never read."""
import ctypes as C

import numpy as np
import pytest

INF = float("inf")
NAN = float("nan")
PLAIN, LM, LEX, LEXTOK = range(4)
NARROW, WIDE, XL, MT = range(4)
MAX_BEAM = {NARROW: 64, WIDE: 1024, XL: 8192, MT: 8192}
MAX_TOKENS = {NARROW: 64, WIDE: 64, XL: 64, MT: 256}
SUFFIX = {NARROW: "", WIDE: "_wide", XL: "_xl"}
STEM = {(0, PLAIN): "w2l_ctc_beam", (0, LM): "w2l_ctc_beam_lm", (0, LEX): "w2l_ctc_beam_lex", (1, LM): "w2l_asg_beam",
        (1, LEX): "w2l_asg_beam_lex"}
BUF = np.zeros(64, np.uint8).ctypes.data


def _L():
    from wav2letter_amd import _lib
    return _lib


def _routes():
    """(id, asg, kind, route, family, without an LM): the 27 named searches, the *_sil and *_lextok ones once per family they take,
    and the ASG token searches once more with lm == NULL, the form W2L_SEARCH_PLAIN names"""
    out = []
    for (asg, kind) in STEM:
        for no_lm in ((False, True) if (asg, kind) == (1, LM) else (False,)):
            tag = "_nolm" if no_lm else ""
            out += [(f"{STEM[asg, kind]}{SUFFIX[f]}{tag}", asg, kind, "named", f, no_lm) for f in (NARROW, WIDE, XL)]
            out += [(f"{STEM[asg, kind]}_sil{f}{tag}", asg, kind, "sil", f, no_lm) for f in (NARROW, WIDE, XL)]
            out.append((f"{STEM[asg, kind]}_mt{tag}", asg, kind, "mt", MT, no_lm))
    for asg in (0, 1):
        out += [(f"{STEM[asg, LEX]}tok{f}", asg, LEXTOK, "lextok", f, False) for f in (NARROW, WIDE, XL)]
    return out


ROUTES = _routes()


def _base(asg, kind, no_lm):
    a = dict(B=2, T=10, N=6, input=BUF, frames=None, trans=BUF if asg else None, beam=4, beamToken=3, threshold=INF, logAdd=0,
             normalize=0, nbest=2, maxLen=8, lm=None, lmHasEos=0, lmWeight=0.0, classScore=None, eosScore=0.0, lexicon=None,
             wordScore=0.0, labels=BUF, lengths=BUF, scores=BUF, lmScores=None, maxWords=0, words=None, wordCounts=None,
             workspace=BUF, silToken=-1, silScore=0.0)
    if kind != PLAIN or asg:
        a.update(lmScores=BUF)
    if kind != PLAIN and not no_lm:
        a.update(lm=BUF, lmHasEos=1, lmWeight=1.0)
    if kind >= LEX:
        a.update(lexicon=BUF, maxWords=4, words=BUF, wordCounts=BUF)
    return a


def _named(asg, kind, route, family):
    """(search, size) of the named entry point as functions of the argument dict"""
    lib = _L().lib()
    stem = STEM[asg, LEX if kind == LEXTOK else kind]
    mid = {"named": SUFFIX.get(family), "sil": "_sil", "mt": "_mt", "lextok": "tok"}[route]
    fn = getattr(lib, stem.replace("_beam", "_beam_search", 1) + mid)
    size = getattr(lib, stem + mid + "_workspace_size")
    fam = [family] if route in ("sil", "lextok") else []

    def search(a):
        args = fam + [a["B"], a["T"], a["N"], a["input"], a["frames"]] + ([a["trans"]] if asg else [])
        args += [a[k] for k in ("beam", "beamToken", "threshold", "logAdd", "normalize", "nbest", "maxLen")]
        if kind >= LEX:
            args += [a[k] for k in ("lm", "lmHasEos", "lmWeight", "lexicon", "wordScore", "eosScore")]
        elif kind == LM:
            args += [a[k] for k in ("lm", "lmHasEos", "lmWeight", "classScore", "eosScore")]
        args += [a["labels"], a["lengths"], a["scores"]] + ([a["lmScores"]] if kind != PLAIN else [])
        if kind >= LEX:
            args += [a["maxWords"], a["words"], a["wordCounts"]]
        args += [a["workspace"], None] + ([a["silToken"], a["silScore"]] if route != "named" else [])
        return fn(*args)
    return search, lambda a: size(*fam, a["B"], a["T"], a["N"], a["beam"], a["beamToken"])


def _desc(family, kind, a):
    fields = {k: v for k, v in a.items() if k != "workspace"}
    return _L().BeamSearchDesc(family=family, kind=kind, **fields)


def _cases(asg, kind, route, family, no_lm):
    """the spoiled calls of a route: [(overrides, the code both calls must return)]"""
    L = _L()
    E, U = L.W2L_EINVAL, L.W2L_EUNSUPPORTED
    tokens = 400 if asg else 399
    big = dict(beam=MAX_BEAM[family] + 1)
    cases = [(dict(B=0), E), (dict(T=0), E), (dict(nbest=0), E), (dict(maxLen=0), E), (dict(N=1), E), (dict(beam=0), E),
             (dict(nbest=5), E), (dict(threshold=NAN), E), (dict(threshold=-1.0), E),
             (dict(input=None), E), (dict(labels=None), E), (dict(lengths=None), E), (dict(scores=None), E), (dict(workspace=None), E),
             (big, U), (dict(N=400, beamToken=MAX_TOKENS[family] + 1), U), (dict(N=400, beamToken=tokens + 7), U),
             (dict(T=(1 << 29) // MAX_BEAM[family] + 1, beam=MAX_BEAM[family]), U),
             (dict(input=None, **big), E), (dict(threshold=NAN, N=400, beamToken=300), E), (dict(nbest=0, **big), E)]
    # trans is the one required pointer a descriptor cannot spoil: NULL there names the CTC search
    if kind != PLAIN or asg:
        cases += [(dict(lmScores=None), E), (dict(lmWeight=INF), E), (dict(eosScore=INF), E), (dict(lmHasEos=0, eosScore=0.5), E),
                  (dict(lmWeight=NAN, **big), E)]
        if not no_lm:
            cases += [(dict(lm=None), E)]   # the ASG token search may do without an LM, but not with lmHasEos set
        else:
            cases += [(dict(lmHasEos=1), E), (dict(classScore=BUF), E)]
    if kind >= LEX:
        cases += [(dict(maxWords=0), E), (dict(lexicon=None), E), (dict(words=None), E), (dict(wordCounts=None), E),
                  (dict(wordScore=INF), E), (dict(wordScore=NAN, **big), E)]
    if route != "named":
        cases += [(dict(silScore=INF), E), (dict(silScore=NAN), E), (dict(silToken=-2), E), (dict(silToken=6 if asg else 5), E),
                  (dict(silToken=1000, silScore=0.5), E), (dict(silScore=INF, **big), E), (dict(silToken=2, silScore=0.5, **big), U)]
    if route == "lextok" and family == XL:   # no xl family: every W2L_EINVAL first, then W2L_EUNSUPPORTED for whatever is left
        cases = [(kw, code if code == E else U) for kw, code in cases] + [(dict(), U), (dict(silToken=2, silScore=0.5), U)]
    return cases


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_descriptor_call_is_the_named_entry_point(route):
    _, asg, kind, how, family, no_lm = route
    L = _L()
    lib = L.lib()
    search, size = _named(asg, kind, how, family)
    dkind = PLAIN if no_lm else kind
    # the size function the contract names: the *_sil one for families 0..2 (the *_mt and *_lextok ones are their own)
    sil_size = getattr(lib, STEM[asg, LEX if kind == LEXTOK else kind] + "_sil_workspace_size")
    narrow_plain_ctc = how == "named" and family == NARROW and kind == PLAIN and not asg
    for kw, expected in _cases(asg, kind, how, family, no_lm):
        a = dict(_base(asg, kind, no_lm), **kw)
        d = _desc(family, dkind, a)
        want = search(a)
        assert want == expected, (kw, want)                                    # a refusal: nothing reached the device
        assert lib.w2l_beam_search(C.byref(d), a["workspace"], None) == want, kw
        got = lib.w2l_beam_search_workspace_size(C.byref(d))
        if narrow_plain_ctc:
            # w2l_ctc_beam_search is the *_sil route without a score; that route's size is the LM-free scan's with a silence
            # score, which holds two arrays more than w2l_ctc_beam_workspace_size: the descriptor's size serves both
            assert got == sil_size(family, a["B"], a["T"], a["N"], a["beam"], a["beamToken"]) >= size(a), kw
            assert (got == 0) == (size(a) == 0), kw
        else:
            assert got == size(a), kw


def test_descriptor_sizes_are_positive_on_the_valid_base():
    """the grid above compares sizes that are often 0 (a refused call has none): on the valid base they are not"""
    lib = _L().lib()
    for _, asg, kind, how, family, no_lm in ROUTES:
        if (how == "lextok" and family == XL) or (how, family, kind, asg) == ("named", NARROW, PLAIN, 0):
            continue
        a = _base(asg, kind, no_lm)
        got = lib.w2l_beam_search_workspace_size(C.byref(_desc(family, PLAIN if no_lm else kind, a)))
        assert got == _named(asg, kind, how, family)[1](a) > 0, (how, family, kind, asg)
    a = _base(0, PLAIN, False)
    got = lib.w2l_beam_search_workspace_size(C.byref(_desc(NARROW, PLAIN, a)))
    assert got == lib.w2l_ctc_beam_sil_workspace_size(0, 2, 10, 6, 4, 3) > lib.w2l_ctc_beam_workspace_size(2, 10, 6, 4, 3) > 0


def test_the_descriptor_calls_own_refusals():
    L = _L()
    lib = L.lib()
    E, U = L.W2L_EINVAL, L.W2L_EUNSUPPORTED

    def both(family, kind, a):
        d = _desc(family, kind, a)
        return lib.w2l_beam_search(C.byref(d), a["workspace"], None), lib.w2l_beam_search_workspace_size(C.byref(d))
    assert lib.w2l_beam_search(None, BUF, None) == E and lib.w2l_beam_search_workspace_size(None) == 0
    # an enumerator out of range, also together with an argument that is W2L_EUNSUPPORTED
    for asg, kind in STEM:
        a = _base(asg, kind, False)
        for family, k in ((4, kind), (-1, kind), (NARROW, 4), (NARROW, -1), (1000, kind)):
            assert both(family, k, a) == (E, 0)
            assert both(family, k, dict(a, beam=100000)) == (E, 0)
    # the token LM under a lexicon has the narrow and wide families only: every W2L_EINVAL, then W2L_EUNSUPPORTED; no size
    for asg in (0, 1):
        a = _base(asg, LEXTOK, False)
        for family in (XL, MT):
            assert both(family, LEXTOK, a) == (U, 0)
            assert both(family, LEXTOK, dict(a, silToken=2, silScore=0.5)) == (U, 0)
            for kw in (dict(lexicon=None), dict(input=None), dict(silScore=INF), dict(nbest=0), dict(lmWeight=NAN), dict(B=0)):
                assert both(family, LEXTOK, dict(a, **kw))[0] == E, kw
        for family in (NARROW, WIDE):
            assert both(family, LEXTOK, dict(a, beam=100000)) == (U, 0)
            assert both(family, LEXTOK, dict(a, workspace=None))[1] > 0
    # a field the chosen search does not take: W2L_EINVAL before anything else, W2L_EUNSUPPORTED arguments included; the size,
    # like the named size functions, looks at the shape alone
    stray = {PLAIN: [dict(lm=BUF), dict(lmHasEos=1), dict(lmWeight=0.5), dict(classScore=BUF), dict(eosScore=0.5), dict(lexicon=BUF),
                     dict(wordScore=0.5), dict(maxWords=4), dict(words=BUF), dict(wordCounts=BUF)],
             LM: [dict(lexicon=BUF), dict(wordScore=0.5), dict(maxWords=4), dict(words=BUF), dict(wordCounts=BUF)],
             LEX: [dict(classScore=BUF)], LEXTOK: [dict(classScore=BUF)]}
    for asg in (0, 1):
        for kind, spoils in stray.items():
            a = _base(asg, kind, kind == PLAIN)
            for family in (NARROW, WIDE, XL, MT):
                if kind == LEXTOK and family > WIDE:
                    continue
                size = both(family, kind, a)[1]
                assert size > 0
                for kw in spoils:
                    assert both(family, kind, dict(a, **kw)) == (E, size), (asg, kind, family, kw)
                    assert both(family, kind, dict(a, beam=100000, **kw)) == (E, 0), (asg, kind, family, kw)
    assert both(NARROW, PLAIN, dict(_base(0, PLAIN, False), lmScores=BUF))[0] == E         # the plain CTC search has no LM sums


def test_the_header_declares_the_descriptor_call():
    import os
    L = _L()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "w2l_hip.h")).read()
    assert "size_t w2l_beam_search_workspace_size(const w2l_beam_search_desc* desc);" in header
    assert "int w2l_beam_search(const w2l_beam_search_desc* desc, void* workspace, w2l_stream_t stream);" in header
    assert {"w2l_beam_search", "w2l_beam_search_workspace_size"} <= set(L.exported_symbols())
    assert (L.BEAM_NARROW, L.BEAM_WIDE, L.BEAM_XL, L.BEAM_MT) == (0, 1, 2, 3)
    assert (L.SEARCH_PLAIN, L.SEARCH_LM, L.SEARCH_LEX, L.SEARCH_LEXTOK) == (0, 1, 2, 3)
    # the structure's layout as a C compiler lays out the header's: 5 ints, 3 pointers, ... on an LP64 target
    assert C.sizeof(L.BeamSearchDesc) == 192 and L.BeamSearchDesc.input.offset == 24 and L.BeamSearchDesc.silScore.offset == 188
