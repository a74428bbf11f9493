"""GPU tests of the chunked streaming forward (wav2letter_amd/streaming.py, csrc/host/stream.cpp, csrc/stream.hip): for any
split of an utterance into chunks the concatenated emissions equal Trainer.forward(train=False) of that utterance alone --
frame counts exactly, values within the project's fp32 parity bar, 1e-4 of the largest reference magnitude."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import stream_ref as R
from wav2letter_amd import _lib
from wav2letter_amd.streaming import StreamingSession
from wav2letter_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TOL = 1e-4


def make_trainer(arch, nfeat, nlabel, seed, perturb=0.1):
    tr = Trainer(arch, nfeat, nlabel, "ctc")
    tr.init_params(seed)
    if perturb:   # LayerNorm gains / offsets and biases away from their initial 1 / 0
        tr.host_params += (np.random.default_rng(seed).normal(size=tr.host_params.shape) * perturb).astype(np.float32)
    tr.to_device()
    return tr


def whole(tr, x):
    """Trainer.forward(train=False) of one utterance x [NFEAT][T] alone: [Tout][N] on the host"""
    tr.plan(1, x.shape[1], 1)
    return tr.forward(torch.tensor(x[None], device="cuda"), train=False)[0].cpu().numpy().copy()


def run_jobs(sess, jobs):
    """jobs: (slot, first_step, x [NFEAT][T], chunks).  Drives the session step by step -- a job's first chunk carries `start`, its
    last `finish`; columns of x nobody may read are NaN -- and returns per job (emissions [n][N], frames per step)."""
    S, cmax = sess.slots, sess.max_chunk
    steps = max(first + len(chunks) for _, first, _, chunks in jobs)
    got = [[] for _ in jobs]
    per_step = [[] for _ in jobs]
    pos = [0] * len(jobs)
    for i in range(steps):
        xs = np.full((S, sess.nfeat, cmax), np.nan, np.float32)
        n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        live = {}
        for j, (slot, first, x, chunks) in enumerate(jobs):
            k = i - first
            if 0 <= k < len(chunks):
                assert slot not in live, "two jobs on one slot in one step"
                live[slot] = j
                c = chunks[k]
                xs[slot, :, :c] = x[:, pos[j]:pos[j] + c]
                pos[j] += c
                n[slot], st[slot], fi[slot] = c, k == 0, k == len(chunks) - 1
        out, n_out = sess.step(torch.tensor(xs, device="cuda"), n, st, fi)
        assert out.shape == (S, sess.max_out, sess.nlabel) and n_out.max() <= sess.max_out
        assert torch.isfinite(out).all()   # rows nobody reads are computed from zero-filled windows, never from stale memory
        for slot in range(S):
            if slot in live:
                got[live[slot]].append(out[slot, :n_out[slot]].clone())
                per_step[live[slot]].append(int(n_out[slot]))
            else:
                assert n_out[slot] == 0
    for j, (_, _, x, _) in enumerate(jobs):
        assert pos[j] == x.shape[1]
    return [(torch.cat(g).cpu().numpy(), p) for g, p in zip(got, per_step)]


def check(got, ref, what, tol=TOL):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)   # the frame count is exact
    if ref.shape[0] > 1:   # the reference is no constant: a frame in the wrong place would show
        assert np.abs(np.diff(ref, axis=0)).max() > 1e-2 * np.abs(ref).max(), what
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{what}: {ref.shape[0]} frames, max err / max |ref| = {err:.3g}")
    assert err < tol, (what, err)


def fixed(T, c):
    return [c] * (T // c) + ([T % c] if T % c else [])


# ---------------------------------------------------------------------------------------------- the tiny arch
@pytest.fixture(scope="module")
def tiny():
    tr = make_trainer(R.TINY_ARCH, R.NFEAT, R.NLABEL, 5)
    rng = np.random.default_rng(11)
    utts = {T: rng.normal(size=(R.NFEAT, T)).astype(np.float32) for T in (1, 2, 3, 23, 40, 64)}
    refs = {T: whole(tr, x) for T, x in utts.items()}
    return tr, utts, refs


@pytest.mark.parametrize("chunking", ["1", "3", "8", "17", "all", "random"])
def test_s1_chunking_invariance(tiny, chunking):
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
    sess = StreamingSession(tr, 3, cmax)
    res = run_jobs(sess, [(s, 0, utts[T], chunks[T]) for s, T in enumerate(Ts)])
    for T, (got, _) in zip(Ts, res):
        check(got, refs[T], f"chunks of {chunking}, T = {T}")


def test_s2_slots_at_different_phases(tiny):
    """in step 3 slot 0 is mid-utterance, slot 1 starts and slot 2 finishes; slot 1 is idle before its start and after its
    finish, and slot 0 sits through four steps without a frame in the middle of its utterance"""
    tr, utts, refs = tiny
    sess = StreamingSession(tr, 3, 8)
    c0 = [5, 5, 5, 5, 0, 0, 0, 0, 5, 5, 5, 5, 8, 8, 8]
    assert sum(c0) == 64
    jobs = [(0, 0, utts[64], c0), (1, 3, utts[40], fixed(40, 7)), (2, 0, utts[23], [8, 8, 4, 3])]
    res = run_jobs(sess, jobs)
    for (slot, _, x, _), (got, _) in zip(jobs, res):
        check(got, refs[x.shape[1]], f"slot {slot}")
    assert res[0][1][4:8] == [0, 0, 0, 0]


def test_s3_slot_reuse(tiny):
    """utterance A then B through the same slot equals B alone -- after A finished, and after A was abandoned half way (B's
    start discards the state); the neighbour slot runs on undisturbed"""
    tr, utts, refs = tiny
    sess = StreamingSession(tr, 2, 8)
    a, b = utts[40], utts[23]
    res = run_jobs(sess, [(0, 0, a, fixed(40, 8)), (0, 5, b, fixed(23, 3)), (1, 1, utts[64], fixed(64, 5))])
    check(res[0][0], refs[40], "A")
    check(res[1][0], refs[23], "B after A")
    check(res[2][0], refs[64], "neighbour")
    # A abandoned: feed 20 of its frames without finish, then start B on the slot
    out, n_out = sess.step(torch.tensor(np.ascontiguousarray(np.stack([a[:, :8], a[:, 8:16]])), device="cuda"), [8, 0], [1, 0], None)
    out, n_out = sess.step(torch.tensor(np.ascontiguousarray(np.stack([a[:, 8:16], a[:, 8:16]])), device="cuda"), [8, 0], None, None)
    res = run_jobs(sess, [(0, 0, b, fixed(23, 8))])
    check(res[0][0], refs[23], "B after an abandoned A")
    sess.reset(0)
    with pytest.raises(_lib.W2LInvalidArgument, match="before it was started"):
        sess.step(torch.zeros(2, R.NFEAT, 8, device="cuda"), [1, 0])


@pytest.mark.parametrize("T", [1, 2, 3])
def test_s4_shorter_than_the_receptive_field(tiny, T):
    tr, utts, refs = tiny
    sess = StreamingSession(tr, 1, 4)
    (got, per_step), = run_jobs(sess, [(0, 0, utts[T], [T, 0])])
    assert per_step == [0, refs[T].shape[0]] and refs[T].shape[0] >= 1
    check(got, refs[T], f"T = {T}")


# ---------------------------------------------------------------------------------------------- the reference's golden vectors
_GOLD_HEAD = "V -1 2 5 0\nRO 0 2 1 3\n"           # (T, 10, 1, B) -> (T, H = 5, C = 2, B), frame [H][C]
_GOLD_TAIL = "RO 2 1 0 3\nV 10 -1 1 0\n"


def _golden_session(g, line, params, chunk):
    """a one-layer session over the fixture's layer: no trainer (the whole-utterance plan refuses LayerNorm frames of 10 floats);
    the parameter arena is the trainer's layout -- parameters in order, each slot rounded up to 4 floats"""
    T, H, Cc, kw = g["T"], g["groups"], g["channels"] // g["groups"], g["kernelSize"]
    assert (H, Cc, kw, g["leftPadding"], g["rightPadding"], g["stride"]) == (5, 2, 3, 1, 1, 1)
    arena = []
    for val in params:
        val = np.asarray(val, np.float32).ravel()
        arena.append(np.concatenate([val, np.zeros(-val.size % 4, np.float32)]))
    arena = torch.tensor(np.concatenate(arena), device="cuda")
    sess = StreamingSession.from_arch(_GOLD_HEAD + line + "\n" + _GOLD_TAIL, 10, 10, arena, 1, chunk)
    assert sess.param_floats == arena.numel()
    x = np.array(g["input" if "input" in g else "in"], np.float32).reshape(T, H * Cc).T.copy()   # frame-major [T][H][C] -> [NFEAT][T]
    (got, _), = run_jobs(sess, [(0, 0, x, fixed(T, chunk))])
    assert got.shape == (T, 10)
    return got


@pytest.mark.parametrize("chunk", [1, 3, 10])
def test_s5_golden_conv1d_in_chunks(chunk):
    """Conv1dTest.cpp:30-104 through a one-layer session, at the fixture's own tolerance"""
    g = json.load(open(os.path.join(GOLD, "conv1d_golden.json")))
    w = np.array(g["weights"], np.float32).reshape(2, 3, 2).transpose(1, 2, 0)   # [co][k][ci] -> [k][ci][co]
    got = _golden_session(g, "C2 2 2 3 1 1 1 1 0", [w, g["bias"]], chunk)
    err = np.abs(got.reshape(-1) - np.array(g["target"])).max()
    print("conv1d golden, chunks of", chunk, "max abs err", err)
    assert err < g["tol"], err


@pytest.mark.parametrize("chunk", [1, 3, 10])
def test_s5_golden_tdsblock_in_chunks(chunk):
    """TDSBlockTest.cpp:27-188 through a one-layer session, at the fixture's own tolerance"""
    g = json.load(open(os.path.join(GOLD, "tdsblock_golden.json")))
    wc = np.array(g["conv_weights"], np.float32).reshape(2, 3, 2).transpose(1, 2, 0)
    # conv w, b; LN1 gamma, beta; lin1 w [in][out], b; lin2 w, b; LN2 gamma, beta
    params = [wc, g["conv_bias"], [g["ln1_weights"][0], g["ln1_bias"][0]], g["lin1_weights"], g["lin1_bias"], g["lin2_weights"],
              g["lin2_bias"], [g["ln2_weights"][0], g["ln2_bias"][0]]]
    got = _golden_session(g, "TDS 2 3 5 0 0 1 0", params, chunk)
    err = np.abs(got.reshape(-1) - np.array(g["expectedOutput"])).max()
    print("tdsblock golden, chunks of", chunk, "max abs err", err)
    assert err < g["tol"], err


# ---------------------------------------------------------------------------------------------- the recipe's geometry
@pytest.mark.parametrize("name,arch,nfeat,nlabel", [
    ("TDS 15 9 80", "V -1 15 80 0\nRO 0 2 1 3\nTDS 15 9 80 0.1 0 1 0\nRO 2 1 0 3\nV 1200 -1 1 0\n", 1200, 1200),
    ("C2 1 15 10 stride 2", "V -1 NFEAT 1 0\nPD 0 5 3\nC2 1 15 10 1 2 1 0 0\nR\nRO 2 1 0 3\nV 1200 -1 1 0\n", 80, 1200),
])
def test_s6_recipe_first_stage_layers(name, arch, nfeat, nlabel):
    tr = make_trainer(arch, nfeat, nlabel, 3)
    x = np.random.default_rng(4).normal(size=(nfeat, 48)).astype(np.float32)
    ref = whole(tr, x)
    (got, _), = run_jobs(StreamingSession(tr, 1, 8), [(0, 0, x, fixed(48, 8))])
    check(got, ref, name)


def test_s6_whole_recipe_arch():
    """streaming_convnets/librispeech/am_500ms_future_context.arch as it stands, random parameters, S = 2, T = 200, one slot in
    chunks of 16 and one in chunks of 8 (NLABEL = 29 keeps the output Linear small; every other shape is the recipe's)"""
    arch = json.load(open(os.path.join(GOLD, "reference_recipes.json")))["arch"]["streaming_convnets/librispeech/am_500ms_future_context.arch"]
    tr = make_trainer(arch, 80, 29, 9, perturb=0.02)
    rng = np.random.default_rng(10)
    xs = [rng.normal(size=(80, 200)).astype(np.float32) for _ in range(2)]
    refs = [whole(tr, x) for x in xs]
    res = run_jobs(StreamingSession(tr, 2, 16), [(0, 0, xs[0], fixed(200, 16)), (1, 0, xs[1], fixed(200, 8))])
    for s in range(2):
        check(res[s][0], refs[s], f"recipe arch, slot {s}")


# ---------------------------------------------------------------------------------------------- the three surfaces
def test_s7_three_surfaces_agree(tmp_path):
    """C ABI through ctypes == Python StreamingSession == compiled C++ fl::pkg::speech::StreamingSession
    (tests/cpp/stream_caller.cpp, plain g++ against libw2l_hip.so with the flags of tests/cpp/Makefile)"""
    exe = str(tmp_path / "stream_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "stream_caller.cpp"),
                    "-o", exe, "-L" + libdir, "-lw2l_hip", "-Wl,-rpath," + libdir, "-ldl"], check=True)
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
    sess = StreamingSession(tr, S, cmax)
    py = []
    for x, n, st, fi in steps:
        out, n_out = sess.step(torch.tensor(x, device="cuda"), n, st, fi)
        py.append((n_out.copy(), out.cpu().numpy().copy()))
    mo = sess.max_out
    cat = [np.concatenate([o[s, :k[s]] for k, o in py]) for s in range(S)]
    for s in range(S):
        check(cat[s], whole(tr, xs[s]), f"python surface, slot {s}")

    # C ABI
    L = _lib.lib()
    h = C.c_void_p(0)
    assert L.w2l_stream_create(R.TINY_ARCH.encode(), nf, nl, S, cmax, C.byref(h)) == 0
    try:
        assert L.w2l_stream_max_out(h) == mo and L.w2l_stream_param_floats(h) == tr.n_net
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
    assert run.returncode == 0 and "stream caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
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
