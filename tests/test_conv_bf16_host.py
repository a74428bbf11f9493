"""The bf16 wide time convolution (w2l_conv_bf16_*, conv_bf16.hip) without a GPU: the six entry points and the trainer switch are
declared and exported; the two size queries are host arithmetic, nonzero for every `C` line with H = 1 and at least 32 input
channels of the reference arch files (tests/golden/reference_recipes.json), for channel counts that are no multiple of 8 and for
padding far beyond the kernel width, and zero for what the family leaves to w2l_conv_*; null pointers and bad descriptors are
W2L_EINVAL and unsupported geometry W2L_EUNSUPPORTED before anything touches a device; --w2l_amp_convs without the mixed-precision
flag is refused by the flag check the drivers run."""
import ctypes as C
import json
import os

import numpy as np
import pytest

_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_recipes.json")
SYMBOLS = ["w2l_conv_bf16_image_elems", "w2l_conv_bf16_scratch_elems", "w2l_conv_bf16_prepare", "w2l_conv_bf16_forward",
           "w2l_conv_bf16_backward_data", "w2l_conv_bf16_backward_filter_bias"]


def _L():
    from wav2letter_amd import _lib
    return _lib


def _desc(B, T, H, Cin, Cout, kw, stride, padl, padr):
    return _L().ConvDesc(B, T, H, Cin, Cout, kw, stride, padl, padr)


def _sizes(*a):
    d = _desc(*a)
    lib = _L().lib()
    return lib.w2l_conv_bf16_image_elems(C.byref(d)), lib.w2l_conv_bf16_scratch_elems(C.byref(d))


def census(nfeat=40, nlabel=30):
    """(arch, Cin, Cout, kw, stride, pad) of every `C cin cout kw s pad [dilation]` line (bare or under WN) of the reference arch
    files: their inputs are `V -1 1 NFEAT 0`, so H = 1 and the channels are the features"""
    out = []
    for name, text in json.load(open(_FIXTURE))["arch"].items():
        for line in text.splitlines():
            t = line.split()
            if t[:1] == ["WN"]:
                t = t[2:]
            if t[:1] != ["C"]:
                continue
            num = lambda s: nfeat if s == "NFEAT" else nlabel if s == "NLABEL" else int(s)
            out.append((name,) + tuple(num(v) for v in t[1:6]))
    return out


def test_symbols_are_declared_and_exported():
    L = _L()
    names = set(L.exported_symbols())
    assert set(SYMBOLS) | {"w2l_trainer_set_mixed_precision_convs"} <= names
    for n in SYMBOLS:
        assert hasattr(L.lib(), n)
    from wav2letter_amd import ops, trainer
    assert callable(ops.conv_bf16) and callable(ops.conv_bf16_backward)
    assert hasattr(trainer._lib_tr(), "w2l_trainer_set_mixed_precision_convs")


def test_size_queries_cover_the_reference_recipes():
    lib = _L().lib()
    lines = census()
    assert len(lines) >= 60 and sum(c[1] >= 32 for c in lines) >= 60
    assert (826, 1816, 29) in {c[1:4] for c in lines} and (80, 1024, 3) in {c[1:4] for c in census(nfeat=80)}
    for nfeat in (40, 80):
        for name, cin, cout, kw, stride, pad in census(nfeat=nfeat):
            if cin < 32:
                continue
            for B, T in ((1, 64), (4, 333), (64, 2000)):
                p = lib.w2l_conv_same_pad(T, kw, stride) if pad == -1 else pad
                img, scr = _sizes(B, T, 1, cin, cout, kw, stride, p, p)
                cpi, cpo = (cin + 7) // 8 * 8, (cout + 7) // 8 * 8
                assert img >= max(cout * kw * cpi, cin * kw * cpo) and img % 8 == 0, (name, cin, cout, kw, stride, pad, B, T)
                # room for the x image and the dy image (kw - 1 frames in front) side by side
                assert scr >= B * (T + 2 * p) * (cpi + cpo) + (kw - 1) * cpo, (name, cin, cout, kw, stride, pad, B, T)
    # the whole conv_glu LibriSpeech recipe at its training shape (config 4: B = 64, T = 2000) has a kernel
    glu = [c for c in census() if c[0] == "conv_glu/librispeech/network.arch"]
    assert len(glu) == 17 and all(_sizes(64, 2000, 1, c[1], c[2], c[3], c[4], max(c[5], 0), max(c[5], 0))[0] for c in glu)


@pytest.mark.parametrize("cin,cout", [(242, 532), (321, 706), (353, 776), (565, 1242), (621, 1366), (683, 1502), (751, 1652), (33, 32), (40, 46)])
def test_odd_channel_counts_large_padding_and_strides(cin, cout):
    for stride in (1, 2):
        for kw, padl, padr, T in ((13, 170, 170, 50), (5, 12, 12, 9), (32, 0, 0, 32), (3, 1, 1, 31), (1, 0, 0, 1), (29, 0, 3, 40)):
            img, scr = _sizes(2, T, 1, cin, cout, kw, stride, padl, padr)
            assert img > 0 and scr > 0, (cin, cout, stride, kw, padl, padr, T)
    assert _sizes(2, 50, 1, cin, cout, 13, 1, 0, 0)[1] < _sizes(4, 50, 1, cin, cout, 13, 1, 0, 0)[1] < _sizes(4, 99, 1, cin, cout, 13, 1, 0, 0)[1]


def test_what_the_family_leaves_to_the_fp32_kernels():
    assert _sizes(2, 100, 80, 64, 64, 5, 1, 2, 2) == (0, 0)        # H = 80
    assert _sizes(2, 100, 1, 64, 64, 5, 3, 2, 2) == (0, 0)         # stride 3
    assert _sizes(2, 100, 1, 1, 64, 5, 1, 2, 2) == (0, 0)          # Cin = 1
    assert _sizes(2, 100, 1, 31, 64, 5, 1, 2, 2) == (0, 0)         # Cin < 32
    assert _sizes(2, 100, 1, 64, 64, 65, 1, 0, 0) == (0, 0)        # kw beyond 64
    assert _sizes(2, 10, 1, 64, 64, 13, 1, 0, 0) == (0, 0)         # no output frame
    assert _sizes(0, 10, 1, 64, 64, 3, 1, 0, 0) == (0, 0) and _sizes(2, 10, 1, 64, 64, 3, 1, -1, 0) == (0, 0)
    assert _L().lib().w2l_conv_bf16_image_elems(None) == 0 and _L().lib().w2l_conv_bf16_scratch_elems(None) == 0
    # the TDS family's geometries stay there
    d = _desc(2, 100, 80, 15, 15, 9, 1, 7, 1)
    assert _L().lib().w2l_tds_conv_bf16_image_elems(C.byref(d)) > 0 and _sizes(2, 100, 80, 15, 15, 9, 1, 7, 1) == (0, 0)


def test_null_pointers_bad_shapes_and_unsupported_geometry_without_a_gpu():
    """every call below carries something that must be refused, so none may reach a launch: the pointers are host memory"""
    L = _L()
    lib = L.lib()
    buf = np.zeros(256, np.uint8)
    p = (buf.ctypes.data + 15) // 16 * 16
    ok = _desc(2, 40, 1, 64, 96, 5, 1, 2, 2)
    ref = lambda d: C.byref(d) if d is not None else None
    prepare = lambda d, w=p, f=p, b=p: lib.w2l_conv_bf16_prepare(ref(d), w, f, b, None)
    forward = lambda d, x=p, f=p, y=p, scr=p: lib.w2l_conv_bf16_forward(ref(d), x, f, None, y, 0, scr, None)
    bwd_data = lambda d, dy=p, b=p, dx=p, scr=p: lib.w2l_conv_bf16_backward_data(ref(d), dy, b, None, dx, scr, None)
    bwd_filter = lambda d, x=p, dy=p, dw=p, scr=p: lib.w2l_conv_bf16_backward_filter_bias(ref(d), x, dy, dw, None, scr, None)
    four = lambda d: [prepare(d), forward(d), bwd_data(d), bwd_filter(d)]

    assert four(None) == [L.W2L_EINVAL] * 4
    for bad in (_desc(0, 40, 1, 64, 96, 5, 1, 2, 2), _desc(2, 0, 1, 64, 96, 5, 1, 2, 2), _desc(2, 40, 0, 64, 96, 5, 1, 2, 2),
                _desc(2, 40, 1, 0, 96, 5, 1, 2, 2), _desc(2, 40, 1, 64, 0, 5, 1, 2, 2), _desc(2, 40, 1, 64, 96, 0, 1, 2, 2),
                _desc(2, 40, 1, 64, 96, 5, 0, 2, 2), _desc(2, 40, 1, 64, 96, 5, 1, -1, 2), _desc(2, 40, 1, 64, 96, 5, 1, 2, -1),
                _desc(2, 3, 1, 64, 96, 5, 1, 0, 0)):
        assert four(bad) == [L.W2L_EINVAL] * 4
    for unsup in (_desc(2, 40, 80, 64, 96, 5, 1, 2, 2), _desc(2, 40, 1, 64, 96, 5, 3, 2, 2), _desc(2, 40, 1, 1, 96, 5, 1, 2, 2)):
        assert four(unsup) == [L.W2L_EUNSUPPORTED] * 4
    # null pointers are W2L_EINVAL, on a geometry with a kernel and -- before W2L_EUNSUPPORTED -- on one without
    for d in (ok, _desc(2, 40, 1, 64, 96, 5, 3, 2, 2)):
        E = L.W2L_EINVAL
        assert prepare(d, w=None) == E and prepare(d, f=None, b=None) == E
        assert forward(d, x=None) == E and forward(d, f=None) == E and forward(d, y=None) == E and forward(d, scr=None) == E
        assert bwd_data(d, dy=None) == E and bwd_data(d, b=None) == E and bwd_data(d, dx=None) == E and bwd_data(d, scr=None) == E
        assert bwd_filter(d, x=None) == E and bwd_filter(d, dy=None) == E and bwd_filter(d, dw=None) == E and bwd_filter(d, scr=None) == E
    # images and scratch are 16-byte aligned
    E = L.W2L_EINVAL
    assert prepare(ok, f=p + 2) == E and prepare(ok, b=p + 8) == E
    assert forward(ok, f=p + 2) == E and forward(ok, scr=p + 2) == E
    assert bwd_data(ok, b=p + 8) == E and bwd_data(ok, scr=p + 4) == E and bwd_filter(ok, scr=p + 2) == E


def test_amp_convs_flag_needs_the_mixed_precision_flag():
    from wav2letter_amd import trainer
    L = _L()
    assert trainer.flags_check("--fl_amp_use_mixed_precision=true\n--w2l_amp_convs=true\n") == 2
    assert trainer.flags_check("--w2l_amp_convs=false\n") == 1
    assert trainer.flags_check("--fl_amp_use_mixed_precision=true\n") == 1
    for text in ("--w2l_amp_convs=true\n", "--w2l_amp_convs=true\n--fl_amp_use_mixed_precision=false\n", "--w2l_amp_convs\n--lr=1\n"):
        with pytest.raises(L.W2LInvalidArgument, match="fl_amp_use_mixed_precision"):
            trainer.flags_check(text)


def test_driver_refuses_the_flag_alone_before_it_looks_for_anything_else(tmp_path):
    """Train reads its flags, checks their dependencies and stops: no arch file, no token dictionary, no device is needed to get
    there"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wav2letter_amd", "bin", "Train")
    r = subprocess.run([exe, "train", "--w2l_amp_convs=true", "--w2l_nlabel=30", f"--rundir={tmp_path}"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "fl_amp_use_mixed_precision" in (r.stdout + r.stderr)
