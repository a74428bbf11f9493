"""GPU tests of the mixed-precision streaming session (StreamingSession(mixed_precision=True), w2l_stream_*_ex): for any split of an
utterance into chunks the concatenated emissions equal Trainer.forward(train=False) of a MIXED-PRECISION trainer on that utterance
alone -- frame counts exactly, values within the project's mixed-precision bar, 2e-3 of the largest reference magnitude (the bar of
tests/test_gpu_trainer.py for config 3).  The session's products add in the order of the trainer's (w2l_gemm_bf16_smallm has the bits
of w2l_gemm_bf16), so every error measured here (printed) was 0 on one MI355X.  The bar cannot be met any other way on the whole
recipe arch: with a kernel that split K -- 5000 times inside the fp32 error bound -- a bf16 rounding flipped here and there, each
flip moved more roundings in the next block, and after 18 blocks the session was 1.2e-2 off."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import stream_ref as R
from test_gpu_stream import check, fixed, run_jobs
from wav2letter_amd import _lib
from wav2letter_amd.streaming import StreamingSession
from wav2letter_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 2e-3        # the mixed-precision bar
TOL_FP32 = 1e-4   # the fp32 bar: a bf16 session has to be FARTHER than this from the fp32 session (B4)
TDS_STAGE = "V -1 15 80 0\nRO 0 2 1 3\nTDS 15 9 80 0.1 0 1 0\nRO 2 1 0 3\nV 1200 -1 1 0\n"
C2_STAGE = "V -1 NFEAT 1 0\nPD 0 5 3\nC2 1 15 10 1 2 1 0 0\nR\nRO 2 1 0 3\nV 1200 -1 1 0\n"


def make_trainer(arch, nfeat, nlabel, seed, perturb=0.1, mixed=True):
    tr = Trainer(arch, nfeat, nlabel, "ctc")
    tr.init_params(seed)
    if perturb:   # LayerNorm gains / offsets and biases away from their initial 1 / 0
        tr.host_params += (np.random.default_rng(seed).normal(size=tr.host_params.shape) * perturb).astype(np.float32)
    tr.to_device()
    tr.set_mixed_precision(mixed)
    return tr


def whole(tr, x):
    """Trainer.forward(train=False) of one utterance x [NFEAT][T] alone, in the trainer's precision: [Tout][N] on the host"""
    tr.plan(1, x.shape[1], 1)
    return tr.forward(torch.tensor(x[None], device="cuda"), train=False)[0].cpu().numpy().copy()


def bf16_session(tr, slots, chunk):
    return StreamingSession(tr, slots, chunk, mixed_precision=True)


# ---------------------------------------------------------------------------------------------- the tiny arch
@pytest.fixture(scope="module")
def tiny():
    tr = make_trainer(R.TINY_ARCH, R.NFEAT, R.NLABEL, 5)
    rng = np.random.default_rng(11)
    utts = {T: rng.normal(size=(R.NFEAT, T)).astype(np.float32) for T in (1, 2, 3, 23, 40, 64)}
    refs = {T: whole(tr, x) for T, x in utts.items()}
    return tr, utts, refs


@pytest.mark.parametrize("chunking", ["1", "3", "8", "17", "all", "random"])
def test_b1_chunking_invariance(tiny, chunking):
    tr, utts, refs = tiny
    Ts = (23, 40, 64)
    rng = np.random.default_rng(17)
    if chunking == "all":
        cmax, chunks = 64, {T: [T] for T in Ts}
    elif chunking == "random":
        cmax, chunks = 17, {T: R.random_chunking(rng, T, 17, p_zero=0.3) for T in Ts}
        assert any(0 in c for c in chunks.values())
    else:
        cmax = int(chunking)
        chunks = {T: fixed(T, cmax) for T in Ts}
    sess = bf16_session(tr, 3, cmax)
    res = run_jobs(sess, [(s, 0, utts[T], chunks[T]) for s, T in enumerate(Ts)])
    for T, (got, _) in zip(Ts, res):
        check(got, refs[T], f"bf16, chunks of {chunking}, T = {T}", TOL)


def test_b2_slots_at_different_phases(tiny):
    tr, utts, refs = tiny
    sess = bf16_session(tr, 3, 8)
    c0 = [5, 5, 5, 5, 0, 0, 0, 0, 5, 5, 5, 5, 8, 8, 8]
    jobs = [(0, 0, utts[64], c0), (1, 3, utts[40], fixed(40, 7)), (2, 0, utts[23], [8, 8, 4, 3])]
    res = run_jobs(sess, jobs)
    for (slot, _, x, _), (got, _) in zip(jobs, res):
        check(got, refs[x.shape[1]], f"bf16, slot {slot}", TOL)
    assert res[0][1][4:8] == [0, 0, 0, 0]


def test_b2_slot_reuse(tiny):
    tr, utts, refs = tiny
    sess = bf16_session(tr, 2, 8)
    a, b = utts[40], utts[23]
    res = run_jobs(sess, [(0, 0, a, fixed(40, 8)), (0, 5, b, fixed(23, 3)), (1, 1, utts[64], fixed(64, 5))])
    check(res[0][0], refs[40], "bf16, A", TOL)
    check(res[1][0], refs[23], "bf16, B after A", TOL)
    check(res[2][0], refs[64], "bf16, neighbour", TOL)
    # A abandoned: feed 16 of its frames without finish, then start B on the slot
    sess.step(torch.tensor(np.ascontiguousarray(np.stack([a[:, :8], a[:, 8:16]])), device="cuda"), [8, 0], [1, 0], None)
    sess.step(torch.tensor(np.ascontiguousarray(np.stack([a[:, 8:16], a[:, 8:16]])), device="cuda"), [8, 0], None, None)
    res = run_jobs(sess, [(0, 0, b, fixed(23, 8))])
    check(res[0][0], refs[23], "bf16, B after an abandoned A", TOL)


@pytest.mark.parametrize("T", [1, 2, 3])
def test_b2_shorter_than_the_receptive_field(tiny, T):
    tr, utts, refs = tiny
    sess = bf16_session(tr, 1, 4)
    (got, per_step), = run_jobs(sess, [(0, 0, utts[T], [T, 0])])
    assert per_step == [0, refs[T].shape[0]] and refs[T].shape[0] >= 1
    check(got, refs[T], f"bf16, T = {T}", TOL)


# ---------------------------------------------------------------------------------------------- the recipe's geometry
@pytest.mark.parametrize("name,arch,nfeat,nlabel", [("TDS 15 9 80", TDS_STAGE, 1200, 1200), ("C2 1 15 10 stride 2", C2_STAGE, 80, 1200)])
def test_b3_recipe_first_stage_layers(name, arch, nfeat, nlabel):
    tr = make_trainer(arch, nfeat, nlabel, 3)
    x = np.random.default_rng(4).normal(size=(nfeat, 48)).astype(np.float32)
    ref = whole(tr, x)
    (got, _), = run_jobs(bf16_session(tr, 1, 8), [(0, 0, x, fixed(48, 8))])
    check(got, ref, "bf16, " + name, TOL)


def test_b3_whole_recipe_arch():
    """streaming_convnets/librispeech/am_500ms_future_context.arch as it stands, random parameters, S = 2, T = 200, one slot in
    chunks of 16 and one in chunks of 8 (NLABEL = 29 keeps the output Linear small; every other shape is the recipe's)"""
    arch = json.load(open(os.path.join(GOLD, "reference_recipes.json")))["arch"]["streaming_convnets/librispeech/am_500ms_future_context.arch"]
    tr = make_trainer(arch, 80, 29, 9, perturb=0.02)
    rng = np.random.default_rng(10)
    xs = [rng.normal(size=(80, 200)).astype(np.float32) for _ in range(2)]
    refs = [whole(tr, x) for x in xs]
    res = run_jobs(bf16_session(tr, 2, 16), [(0, 0, xs[0], fixed(200, 16)), (1, 0, xs[1], fixed(200, 8))])
    for s in range(2):
        check(res[s][0], refs[s], f"bf16, recipe arch, slot {s}", TOL)


@pytest.fixture(scope="module")
def stage():
    """the recipe-stage TDS block, its parameters, one utterance and the mixed-precision whole forward"""
    tr = make_trainer(TDS_STAGE, 1200, 1200, 3)
    x = np.random.default_rng(4).normal(size=(1200, 48)).astype(np.float32)
    return tr, x, whole(tr, x)


def test_b4_bf16_is_really_in_use(stage):
    """the bf16 session is inside the mixed-precision bar of the mixed-precision forward and OUTSIDE the fp32 bar of the fp32 session
    on the same parameters: a session that quietly ran in fp32 would sit on the fp32 one"""
    tr, x, ref = stage
    (bf, _), = run_jobs(bf16_session(tr, 1, 8), [(0, 0, x, fixed(48, 8))])
    check(bf, ref, "bf16 session against the mixed-precision forward", TOL)
    tr.set_mixed_precision(False)
    try:
        (fp, _), = run_jobs(StreamingSession(tr, 1, 8), [(0, 0, x, fixed(48, 8))])
    finally:
        tr.set_mixed_precision(True)
    diff = np.abs(bf - fp).max() / np.abs(fp).max()
    print(f"bf16 session against the fp32 session: max diff / max |fp32| = {diff:.3g} (fp32 bar {TOL_FP32})")
    assert diff > TOL_FP32, f"ran in fp32: the bf16 session is within {diff:.3g} of the fp32 session"


def test_b5_weight_snapshot(stage):
    """a bf16 session keeps the model it saw at its first step until refresh_weights()"""
    tr, x, ref_old = stage
    old = tr.params.clone()
    sess = bf16_session(tr, 1, 8)
    (got0, _), = run_jobs(sess, [(0, 0, x, fixed(48, 8))])
    check(got0, ref_old, "snapshot: the old model", TOL)
    try:
        rng = np.random.default_rng(77)
        other = tr.host_params + (rng.normal(size=tr.host_params.shape) * 0.05).astype(np.float32)
        tr.params.copy_(torch.from_numpy(other.astype(np.float32)).cuda())
        ref_new = whole(tr, x)
        assert np.abs(ref_new - ref_old).max() > 10 * TOL * np.abs(ref_old).max()   # another model
        (got1, _), = run_jobs(sess, [(0, 0, x, fixed(48, 8))])
        assert np.array_equal(got1, got0)   # no step after the first read a parameter or converted a weight
        sess.refresh_weights()
        (got2, _), = run_jobs(sess, [(0, 0, x, fixed(48, 8))])
        check(got2, ref_new, "snapshot: the new model after refresh_weights", TOL)
    finally:
        tr.params.copy_(old)


def _drive(sess, x, chunk, other):
    """utterance x through slot 0 in chunks of `chunk`; other(i) -> (frames [NFEAT][chunk] or None, start) for slot 1.  Returns slot 0's
    emissions (no finiteness assertion on slot 1: it may be fed NaN on purpose)"""
    S, T = sess.slots, x.shape[1]
    got = []
    steps = (T + chunk - 1) // chunk
    for i in range(steps):
        xs = np.zeros((S, sess.nfeat, chunk), np.float32)
        c = min(chunk, T - i * chunk)
        xs[0, :, :c] = x[:, i * chunk:i * chunk + c]
        n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        n[0], st[0], fi[0] = c, i == 0, i == steps - 1
        frames, start = other(i)
        if frames is not None:
            xs[1], n[1], st[1] = frames, chunk, start
        out, n_out = sess.step(torch.tensor(xs, device="cuda"), n, st, fi)
        got.append(out[0, :n_out[0]].clone())
    return torch.cat(got).cpu().numpy()


def test_b6_slot_isolation(stage):
    """slot 0's emissions are bit-identical whether slot 1 is idle, runs another utterance, or is fed NaN frames"""
    tr, x, ref = stage
    y = np.random.default_rng(6).normal(size=(1200, 8)).astype(np.float32)
    nan = np.full((1200, 8), np.nan, np.float32)
    idle = _drive(bf16_session(tr, 2, 8), x, 8, lambda i: (None, 0))
    busy = _drive(bf16_session(tr, 2, 8), x, 8, lambda i: (y, i == 0))
    poisoned = _drive(bf16_session(tr, 2, 8), x, 8, lambda i: (nan, i == 0))
    check(idle, ref, "slot 0 beside an idle slot", TOL)
    assert np.isfinite(poisoned).all()
    assert np.array_equal(idle, busy)
    assert np.array_equal(idle, poisoned)


# ---------------------------------------------------------------------------------------------- the three surfaces
def test_b7_three_surfaces_agree(tmp_path):
    """C ABI through ctypes == Python StreamingSession(mixed_precision=True) == compiled C++ fl::pkg::speech::StreamingSession with
    mixedPrecision = true (tests/cpp/stream_bf16_caller.cpp, plain g++ against libw2l_hip.so with the flags of tests/cpp/Makefile)"""
    exe = str(tmp_path / "stream_bf16_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "stream_bf16_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip", "-Wl,-rpath," + libdir,
                    "-ldl"], check=True)
    S, cmax, nf, nl = 2, 8, R.NFEAT, R.NLABEL
    tr = make_trainer(R.TINY_ARCH, nf, nl, 1, perturb=0)   # seed 1: the parameters buildSequentialModule gives the C++ network
    rng = np.random.default_rng(2)
    xs = [rng.normal(size=(nf, 40)).astype(np.float32), rng.normal(size=(nf, 23)).astype(np.float32)]
    plans = [fixed(40, 8), [0] + fixed(23, 5)]
    steps = []
    pos = [0, 0]
    for i in range(max(len(p) for p in plans)):
        x = np.zeros((S, nf, cmax), np.float32)
        n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for s in range(S):
            if i < len(plans[s]):
                c = plans[s][i]
                x[s, :, :c] = xs[s][:, pos[s]:pos[s] + c]
                pos[s] += c
                n[s], st[s], fi[s] = c, i == 0, i == len(plans[s]) - 1
        steps.append((x, n, st, fi))

    # Python
    sess = bf16_session(tr, S, cmax)
    py = []
    for x, n, st, fi in steps:
        out, n_out = sess.step(torch.tensor(x, device="cuda"), n, st, fi)
        py.append((n_out.copy(), out.cpu().numpy().copy()))
    mo = sess.max_out
    cat = [np.concatenate([o[s, :k[s]] for k, o in py]) for s in range(S)]
    for s in range(S):
        check(cat[s], whole(tr, xs[s]), f"bf16, python surface, slot {s}", TOL)

    # C ABI
    L = _lib.lib()
    h = C.c_void_p(0)
    assert L.w2l_stream_create_ex(R.TINY_ARCH.encode(), nf, nl, S, cmax, 1, C.byref(h)) == 0
    try:
        assert L.w2l_stream_max_out(h) == mo and L.w2l_stream_param_floats(h) == tr.n_net
        assert L.w2l_stream_state_bytes(h) == sess.state_bytes
        state = torch.empty(L.w2l_stream_state_bytes(h), dtype=torch.uint8, device="cuda")
        assert L.w2l_stream_bind(h, tr.params.data_ptr(), state.data_ptr(), state.numel()) == 0
        for (x, n, st, fi), (want_n, want) in zip(steps, py):
            xd = torch.tensor(x, device="cuda")
            n_out = np.zeros(S, np.int32)
            ptr = C.c_void_p(0)
            assert L.w2l_stream_step(h, xd.data_ptr(), n.ctypes.data, st.ctypes.data, fi.ctypes.data, C.byref(ptr), n_out.ctypes.data,
                                     torch.cuda.current_stream().cuda_stream) == 0
            assert (n_out == want_n).all()
            off = ptr.value - state.data_ptr()
            got = state[off:off + 4 * S * mo * nl].view(torch.float32).view(S, mo, nl).cpu().numpy()
            for s in range(S):
                assert np.array_equal(got[s, :n_out[s]], want[s, :n_out[s]])   # the same launches on the same shapes
    finally:
        L.w2l_stream_destroy(h)

    # compiled C++
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    arch = R.TINY_ARCH.encode()
    with open(inp, "wb") as f:
        f.write(np.array([nf, nl, S, cmax, len(steps), len(arch)], np.int32).tobytes() + arch + b"\0" * (-len(arch) % 4))
        for x, n, st, fi in steps:
            f.write(n.tobytes() + st.tobytes() + fi.tobytes() + x.tobytes())
    run = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "stream bf16 caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
    raw = np.fromfile(outp, np.int32)
    assert raw[0] == mo
    at = 1
    for want_n, want in py:
        n_out = raw[at:at + S]
        at += S
        got = raw[at:at + S * mo * nl].view(np.float32).reshape(S, mo, nl)
        at += S * mo * nl
        assert (n_out == want_n).all()
        for s in range(S):
            assert np.array_equal(got[s, :n_out[s]], want[s, :n_out[s]])
    assert at == len(raw)


# ---------------------------------------------------------------------------------------------- the rules, on the device
def test_b8_precision_rules_on_the_device(tiny):
    tr, utts, _ = tiny
    with pytest.raises(_lib.W2LUnsupported, match="mixed-precision"):   # the old constructor, as ever
        StreamingSession(tr, 2, 8)
    x = torch.zeros(2, R.NFEAT, 8, device="cuda")
    sess = bf16_session(tr, 2, 8)
    sess.step(x, [8, 0], [1, 0])
    tr.set_mixed_precision(False)
    try:
        with pytest.raises(_lib.W2LInvalidArgument, match="mixed-precision"):   # the trainer left the mode under a live bf16 session
            sess.step(x, [8, 0])
        with pytest.raises(_lib.W2LInvalidArgument, match="mixed-precision"):
            bf16_session(tr, 2, 8)
        fp = StreamingSession(tr, 2, 8)
        fp.step(x, [8, 0], [1, 0])
        tr.set_mixed_precision(True)
        with pytest.raises(_lib.W2LUnsupported, match="mixed-precision"):       # and an fp32 session refuses a mixed trainer at a step
            fp.step(x, [8, 0])
    finally:
        tr.set_mixed_precision(True)
    out, n_out = sess.step(x, [8, 0])   # the bf16 session goes on where it was
    assert torch.isfinite(out).all()
