"""GPU tests of LocalNorm (include/w2l_hip.h w2l_local_norm / w2l_norm_session_*, csrc/local_norm.hip, csrc/host/norm_stream.cpp):
the batch call against the contract's numpy restatement under the contract's own bound, the eps rule, the session against the
batch call BIT FOR BIT under any chunking, the session against the reference's streaming recurrence, containment on the guarded
arena, the three surfaces, the streaming chain and `Train` on list files."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import local_norm_ref as R
from tests.list_fixture import ENV, _fixture, _train_cmd
from tests.arena import NAN_PATTERN, QUIET_PATTERN, Arena
from wav2letter_amd import _lib
from wav2letter_amd.features import Mfsc, local_normalize
from wav2letter_amd.streaming import StreamingFeatures, StreamingLocalNorm, StreamingSession
from wav2letter_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.25


def _s():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.contiguous().view(torch.int32)


def batch_call(x, frames, left, right, pad_x=3, pad_y=5, inplace=False):
    """w2l_local_norm through ctypes on [B][F][T] numpy input with ldx = T + pad_x, ldy = T + pad_y; everything the call may not
    write holds SENTINEL.  -> y [B][F][ldy] on the device"""
    B, F, T = x.shape
    L = _lib.lib()
    xd = torch.full((B, F, T + pad_x), SENTINEL, device="cuda")
    xd[:, :, :T] = torch.from_numpy(x).cuda()
    yd = xd if inplace else torch.full((B, F, T + pad_y), SENTINEL, device="cuda")
    fr = torch.tensor(frames, dtype=torch.int32, device="cuda") if frames is not None else None
    ws = torch.empty(L.w2l_local_norm_workspace_size(B, T), dtype=torch.uint8, device="cuda")
    st = L.w2l_local_norm(B, F, T, xd.shape[2], xd.data_ptr(), fr.data_ptr() if fr is not None else None, left, right, yd.shape[2],
                          yd.data_ptr(), ws.data_ptr(), _s())
    assert st == 0, (st, L.w2l_host_last_error())
    return yd


def check_against_contract(y, x, n, left, right, what):
    """columns [0, n) of y [F][>= T] (numpy) against contract(x[:, :n]) under the contract's bound"""
    ref, mean, sd = R.contract(x[:, :n], left, right)
    err = np.abs(y[:, :n].astype(np.float64) - ref)
    over = err - R.bound(x[:, :n], mean, sd)
    assert np.isfinite(y[:, :n]).all() and (over <= 0).all(), (what, float(over.max()), float(err.max()))
    return float(err.max())


# ---------------------------------------------------------------------------------------------- 1: batch against the contract
@pytest.mark.parametrize("L", R.LS)
@pytest.mark.parametrize("F", R.FS)
def test_1_batch_against_the_contract(F, L):
    """every element within 2^-22 (|x| + |mean|) / sd of the restatement; B = 3 with frames = {T, T - 1, 0}; columns at or beyond
    frames[b] untouched; in place equal to out of place byte for byte"""
    worst = 0.0
    for T in R.lengths(L):
        x = np.stack([R.features(F, T, 7 + b) for b in range(3)])
        frames = [T, T - 1, 0]
        for right in R.RS:
            y = batch_call(x, frames, L, right)
            yi = batch_call(x, frames, L, right, inplace=True)
            yh, yih = y.cpu().numpy(), yi.cpu().numpy()
            for b, n in enumerate(frames):
                assert (yh[b, :, n:] == SENTINEL).all(), (T, right, b)          # beyond frames[b] and in the row gaps: not written
                assert np.array_equal(yih[b, :, n:T], x[b, :, n:]) and (yih[b, :, T:] == SENTINEL).all()
                assert np.array_equal(yh[b, :, :n].view(np.int32), yih[b, :, :n].view(np.int32))
                if n:
                    worst = max(worst, check_against_contract(yh[b], x[b], n, L, right, (F, L, T, right, b)))
    print(f"batch F={F} L={L}: worst |got - contract| = {worst:.3g}")


def test_1_frames_null_means_T_and_counts_are_clamped():
    x = np.stack([R.features(3, 9, b) for b in range(3)])
    full = batch_call(x, None, 2, 1)
    clamped = batch_call(x, [100, -5, 9], 2, 1)
    assert torch.equal(bits(full[0]), bits(clamped[0])) and torch.equal(bits(full[2]), bits(clamped[2]))
    assert (clamped[1] == SENTINEL).all()
    for b in range(3):
        check_against_contract(full[b].cpu().numpy(), x[b], 9, 2, 1, b)


def test_1_more_than_one_workgroup_per_row():
    """T = 605 spans three tiles of 256 frames; a window that straddles a tile border is like any other"""
    x = R.features(80, 605, 3)[None]
    y = batch_call(x, None, 300, 5)[0].cpu().numpy()
    check_against_contract(y, x[0], 605, 300, 5, "T=605")


# ---------------------------------------------------------------------------------------------- 2: the eps rule
def _alternating(F, T, a):
    sign = np.where((np.arange(F)[:, None] + np.arange(T)[None, :]) % 2 == 0, 1.0, -1.0)
    return (sign * a).astype(np.float32)


@pytest.mark.parametrize("F", R.FS)
def test_2_eps_rule(F):
    T, L = 12, 3
    const = np.full((1, F, T), 3.7, np.float32)
    assert (batch_call(const, None, L, 0)[0, :, :T] == 0).all()                     # deviation 0 -> 1: exact zeros
    small = _alternating(F, T, 2.0 ** -18)[None]                                    # deviation below 1e-5: x - m, not divided
    y = batch_call(small, None, L, 0)[0].cpu().numpy()
    ref, mean, sd = R.contract(small[0], L, 0)
    assert (sd == 1.0).all()
    assert np.array_equal(y[:, :T], (small[0] - mean.astype(np.float32)[None, :]).astype(np.float32))
    check_against_contract(y, small[0], T, L, 0, "2^-18")
    big = _alternating(F, T, 2.0 ** -16)[None]                                      # deviation above 1e-5: divided
    y = batch_call(big, None, L, 0)[0].cpu().numpy()
    ref, mean, sd = R.contract(big[0], L, 0)
    assert (sd < 2.0 ** -15).all() and np.abs(y[:, :T]).max() > 0.9
    check_against_contract(y, big[0], T, L, 0, "2^-16")
    # an offset of 1000 with unit noise: the cancellation the double sums are for
    off = (1000.0 + np.random.default_rng(5).normal(size=(1, F, 40))).astype(np.float32)
    y = batch_call(off, None, 7, 1)[0].cpu().numpy()
    check_against_contract(y, off[0], 40, 7, 1, "offset 1000")
    assert 0.5 < y[:, :40].std() < 1.5


# ---------------------------------------------------------------------------------------------- 3: session against batch
def run_session(sess, jobs, ld, inplace):
    """jobs: (slot, first_step, x [F][n], chunks, reset_after_step or None).  A job's first chunk carries `start`.  Columns nobody
    may read are NaN, columns nobody may write hold SENTINEL and are checked.  -> per job y [F][n] on the device"""
    S, F = sess.slots, sess.nfeat
    steps = max(first + len(chunks) for _, first, _, chunks, _ in jobs)
    got = [[] for _ in jobs]
    pos = [0] * len(jobs)
    dirty = []
    xd = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for _, _, x, _, _ in jobs]
    for i in range(steps):
        xs = torch.full((S, F, ld), float("nan"), device="cuda")
        n, st = np.zeros(S, np.int32), np.zeros(S, np.int32)
        live = {}
        for j, (slot, first, x, chunks, _) in enumerate(jobs):
            k = i - first
            if 0 <= k < len(chunks):
                assert slot not in live
                live[slot] = j
                c = chunks[k]
                xs[slot, :, :c] = xd[j][:, pos[j]:pos[j] + c]
                pos[j] += c
                n[slot], st[slot] = c, k == 0
        if inplace:
            keep = xs.clone()
            out = sess.step(xs, n, st)
            assert out is xs
        else:
            out = torch.full((S, F, ld + 2), SENTINEL, device="cuda")
            assert sess.step(xs, n, st, out=out) is out
        for slot in range(S):     # (flags stay on the device until the end: no synchronisation per step)
            c = int(n[slot])
            if inplace:
                dirty.append((bits(out[slot, :, c:]) != bits(keep[slot, :, c:])).any())
            else:
                dirty.append((out[slot, :, c:] != SENTINEL).any())
            if slot in live:
                got[live[slot]].append(out[slot, :, :c].clone())
        for j, (slot, first, _, chunks, reset_after) in enumerate(jobs):
            if reset_after is not None and i == first + reset_after:
                sess.reset(slot)
    assert not bool(torch.stack(dirty).any()), "a step wrote at or beyond a slot's new frames"
    return [torch.cat(g, dim=1) for g in got]


def schedules(T, L, seed):
    rng = np.random.default_rng([seed, T, L])
    small, left = [], T
    while left > 0:
        c = int(min(left, rng.integers(0, 4)))
        small.append(c)
        left -= c
    out = {"0-3": small + [0], "whole": [T]}
    for name, c in (("L-1", L - 1), ("L+1", L + 1)):
        if c >= 1:
            out[name] = [min(c, T - t) for t in range(0, T, c)]
    return out


def batch_reference(x, left):
    return batch_call(x[None], None, left, 0, pad_x=0, pad_y=0)[0]


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("L", R.LS)
def test_3_session_equals_batch_bit_for_bit_three_slots(L, inplace):
    """slot 0: an utterance from step 0 whose slot is reset mid-way (the rest of it is never fed) and restarted with another
    utterance; slot 1: started late; slot 2: never started.  Every chunk schedule; each utterance equals w2l_local_norm(right = 0)
    of it alone, and what was fed before the reset equals the same prefix of the batch result."""
    F = 80
    T = 2 * L + 5
    xa, xb, xc = (R.features(F, T, 20 + k) for k in range(3))
    ya, yb, yc = (batch_reference(x, L) for x in (xa, xb, xc))
    for name, chunks in schedules(T, L, 1).items():
        half = max(1, len(chunks) // 2)
        fed = sum(chunks[:half])
        sess = StreamingLocalNorm(F, 3, max(chunks + [1]), L)
        jobs = [(0, 0, xa[:, :fed], chunks[:half], half - 1),
                (0, half + 1, xc, chunks, None),
                (1, 2, xb, chunks, None)]
        ga, gc, gb = run_session(sess, jobs, max(chunks + [1]) + 1, inplace)
        assert torch.equal(bits(ga), bits(ya[:, :fed])), (name, "before the reset")
        assert torch.equal(bits(gc), bits(yc)), (name, "restarted slot")
        assert torch.equal(bits(gb), bits(yb)), (name, "late slot")
        assert sess.slot_state(2) == (False, 0) and sess.slot_state(1) == (True, T)
        x = torch.zeros(3, F, 4, device="cuda")
        with pytest.raises(_lib.W2LInvalidArgument, match="slot 2 is fed before it was started"):
            sess.step(x, [0, 0, 1])
        sess.reset(1)
        with pytest.raises(_lib.W2LInvalidArgument, match="slot 1 is fed before it was started"):
            sess.step(x, [0, 1, 0])


@pytest.mark.parametrize("F", R.FS)
def test_3_session_equals_batch_bit_for_bit_one_slot(F):
    """S = 1, every length of the grid, every schedule, both placements"""
    for L in R.LS:
        for T in R.lengths(L):
            x = R.features(F, T, 40)
            want = batch_reference(x, L)
            for name, chunks in schedules(T, L, 2).items():
                for inplace in (False, True):
                    sess = StreamingLocalNorm(F, 1, max(chunks + [1]), L)
                    got, = run_session(sess, [(0, 0, x, chunks, None)], max(chunks + [1]), inplace)
                    assert torch.equal(bits(got), bits(want)), (F, L, T, name, inplace)


# ---------------------------------------------------------------------------------------------- 4: session against the reference
def test_4_session_against_the_reference_recurrence():
    """the bar is four times the worst |reference - contract| measured on the CPU over this very grid
    (local_norm_ref.REF_VS_CONTRACT_WORST, asserted by test_local_norm_host.py): it only separates fp32-sum from fp64-sum
    roundings.  What it pins is the window membership: a window one frame too long or short is off by 0.16 at L = 1, 2."""
    bar = 4 * R.REF_VS_CONTRACT_WORST
    worst = 0.0
    for F, L, T, seed in R.cases():
        x = R.features(F, T, seed)
        sess = StreamingLocalNorm(F, 1, 4, L)
        chunks = [min(3, T - t) for t in range(0, T, 3)]
        got, = run_session(sess, [(0, 0, x, chunks, None)], 4, True)
        d = float(np.abs(got.cpu().numpy().astype(np.float64) - R.reference(x, L)).max())
        worst = max(worst, d)
        assert d <= bar, (F, L, T, d, bar)
    print(f"session vs reference recurrence: worst {worst:.3g}, bar {bar:.3g}")


# ---------------------------------------------------------------------------------------------- 5: containment
def _contained(fn):
    """fn(arena) -> dict of result tensors; run in two quiet arenas and one NaN arena: guards intact, results identical bit for bit"""
    runs = []
    for pattern in (QUIET_PATTERN, QUIET_PATTERN, NAN_PATTERN):
        ar = Arena("cuda", pattern, 8 << 20)
        res = fn(ar)
        torch.cuda.synchronize()
        ar.check()
        runs.append((ar, res))
    (_, a), (_, b), (n, c) = runs
    for key in a:
        assert torch.equal(bits(a[key]), bits(b[key])) and torch.equal(bits(a[key]), bits(c[key])), key
        assert torch.isfinite(c[key]).all(), key
    return n, c


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
def test_5_batch_call_stays_inside_its_buffers(inplace):
    """operands with padded leading dimensions, a workspace of exactly the declared bytes; full rows so that every element of y
    is written (checked in the NaN arena) -- and a second case with ragged frame counts"""
    B, F, T, left, right = 3, 80, 300, 7, 5
    x = np.stack([R.features(F, T, 60 + b) for b in range(B)])
    L = _lib.lib()

    def full(ar, frames=None):
        kind = "inout" if inplace else "in"
        xv, xp = ar.place((B, F, T), torch.float32, ld=T + 4, kind=kind, name="x", data=x)
        yv, yp = (xv, xp) if inplace else ar.place((B, F, T), torch.float32, ld=T + 9, kind="out", name="y")
        _, wp = ar.place((L.w2l_local_norm_workspace_size(B, T),), torch.uint8, kind="work", name="ws")
        fp = ar.place((B,), torch.int32, kind="in", name="frames", data=np.array(frames, np.int32))[1] if frames else None
        assert L.w2l_local_norm(B, F, T, T + 4, xp, fp, left, right, T + 4 if inplace else T + 9, yp, wp, _s()) == 0
        return {"y": yv}

    n, res = _contained(full)
    if not inplace:
        assert n.unwritten("y") == 0
    for b in range(B):
        check_against_contract(res["y"][b].cpu().numpy(), x[b], T, left, right, b)
    frames = [T, 257, 1]
    _, res = _contained(lambda ar: {k: v[:, :, :1] for k, v in full(ar, frames).items()})   # (frame 0: every row has one)
    for b in range(B):
        ref, mean, sd = R.contract(x[b, :, :frames[b]], left, right)
        err = np.abs(res["y"][b].cpu().numpy().astype(np.float64) - ref[:, :1])
        assert (err <= R.bound(x[b, :, :1], mean[:1], sd[:1])).all(), (b, float(err.max()))


def test_5_session_stays_inside_its_state_and_rows():
    """the state buffer has exactly w2l_norm_session_state_bytes bytes and starts as the guard pattern (no initialisation needed)"""
    S, F, cmax, left = 3, 80, 6, 7
    xs = [R.features(F, 20, 70 + s) for s in range(S)]
    L = _lib.lib()

    def run(ar):
        h = C.c_void_p(0)
        assert L.w2l_norm_session_create(F, S, cmax, left, 0, C.byref(h)) == 0
        try:
            nbytes = L.w2l_norm_session_state_bytes(h)
            _, sp = ar.place((nbytes,), torch.uint8, kind="work", name="state")
            assert L.w2l_norm_session_bind(h, sp, nbytes) == 0
            outs = []
            for i, t0 in enumerate(range(0, 20, 5)):
                chunk = np.stack([x[:, t0:t0 + 5] for x in xs])
                n = np.array([5, 5 if i else 0, 5], np.int32)          # slot 1 starts one step late
                st = np.array([i == 0, i == 1, i == 0], np.int32)
                if i:
                    chunk[1] = xs[1][:, t0 - 5:t0]
                xv, xp = ar.place((S, F, 5), torch.float32, ld=cmax + 1, kind="inout", name=f"x{i}", data=chunk)
                assert L.w2l_norm_session_step(h, xp, cmax + 1, n.ctypes.data, st.ctypes.data, xp, cmax + 1, _s()) == 0
                outs.append(xv)
            torch.cuda.synchronize()
            return {"slot0": torch.cat([o[0] for o in outs], dim=1), "slot1": torch.cat([o[1] for o in outs[1:]], dim=1)}
        finally:
            L.w2l_norm_session_destroy(h)

    _, res = _contained(run)
    assert torch.equal(bits(res["slot0"]), bits(batch_reference(xs[0], left)))
    assert torch.equal(bits(res["slot1"]), bits(batch_reference(xs[1][:, :15], left)))


# ---------------------------------------------------------------------------------------------- 6: the surfaces
def test_6_three_surfaces_agree(tmp_path):
    """C ABI through ctypes == features.local_normalize / StreamingLocalNorm == compiled C++ fl::pkg::speech::localNormalize /
    StreamingLocalNorm (tests/cpp/local_norm_caller.cpp, plain g++ against libw2l_hip.so), byte for byte"""
    exe = str(tmp_path / "local_norm_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "local_norm_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    B, F, T, left, chunk = 3, 80, 37, 7, 5
    x = np.stack([R.features(F, T, 80 + b) for b in range(B)])
    frames = np.array([T, T - 1, 3], np.int32)
    outs = {}
    for right in (0, 2):
        inp, outp = str(tmp_path / f"in{right}.bin"), str(tmp_path / f"out{right}.bin")
        with open(inp, "wb") as f:
            f.write(np.array([B, F, T, left, right, chunk], np.int32).tobytes() + frames.tobytes() + x.tobytes())
        run = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "local norm caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
        outs[right] = np.fromfile(outp, np.float32).reshape(2, B, F, T)
    xd = torch.from_numpy(x).cuda()
    for right in (0, 2):
        abi = batch_call(x, list(frames), left, right, pad_x=0, pad_y=0)
        for b in range(B):
            abi[b, :, frames[b]:] = 0                                   # the other two surfaces hand out zeros there
        py = local_normalize(xd, frames, left, right)
        assert torch.equal(bits(abi), bits(py)), right
        assert np.array_equal(outs[right][0].view(np.int32), py.cpu().numpy().view(np.int32)), right
    sess = StreamingLocalNorm(F, B, chunk, left)
    stream = torch.zeros(B, F, T, device="cuda")
    for t0 in range(0, T, chunk):
        n = np.clip(frames - t0, 0, chunk).astype(np.int32)
        c = torch.zeros(B, F, chunk, device="cuda")
        c[:, :, :min(chunk, T - t0)] = xd[:, :, t0:t0 + chunk]
        sess.step(c, n, [int(t0 == 0)] * B)
        for b in range(B):
            stream[b, :, t0:t0 + n[b]] = c[b, :, :n[b]]
    assert np.array_equal(outs[0][1].view(np.int32), stream.cpu().numpy().view(np.int32))
    assert torch.equal(bits(stream), bits(local_normalize(xd, frames, left, 0)))
    # out= in place, and the refusals of the Python front end reach the caller as exceptions
    y = xd.clone()
    assert local_normalize(y, frames, left, 0, out=y) is y
    for b in range(B):
        assert torch.equal(bits(y[b, :, :frames[b]]), bits(stream[b, :, :frames[b]])) and torch.equal(y[b, :, frames[b]:], xd[b, :, frames[b]:])
    with pytest.raises(_lib.W2LInvalidArgument, match="negative"):
        local_normalize(xd, frames, -1, 0)
    with pytest.raises(_lib.W2LUnsupported, match="65537"):
        local_normalize(xd, frames, 65536, 0)


def test_6_prefetch_loader_local_norm(tmp_path):
    """PrefetchLoader(local_norm=(left, right)) hands out local_normalize of its own unnormalised features over every utterance's
    OWN frames, zero beyond them; local_norm=None keeps the unnormalised output"""
    import wave
    from wav2letter_amd.loader import PrefetchLoader
    rng = np.random.default_rng(11)
    paths, lens = [], [4000, 2500, 3300]
    for k, n in enumerate(lens):
        paths.append(str(tmp_path / f"u{k}.wav"))
        with wave.open(paths[-1], "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes(np.round(rng.normal(size=n) * 3000).astype("<i2").tobytes())
    fe = Mfsc(num_filters=40)
    (raw, sizes, _), = [(f.clone(), s.clone(), i) for f, s, i in PrefetchLoader(paths, [[0, 1, 2]], fe, workers=2, depth=2)]
    (got, _, _), = [(f.clone(), s, i) for f, s, i in PrefetchLoader(paths, [[0, 1, 2]], fe, workers=2, depth=2, local_norm=(5, 1))]
    frames = [fe.num_frames(n) for n in lens]
    assert sizes.cpu().tolist() == lens and got.shape == raw.shape == (3, 40, max(frames))
    want = local_normalize(raw, frames, 5, 1)
    assert torch.equal(bits(got), bits(want))
    for b, n in enumerate(frames):
        assert (got[b, :, n:] == 0).all()
        check_against_contract(got[b].cpu().numpy(), raw[b].cpu().numpy(), n, 5, 1, b)


CHAIN_ARCH = ("V -1 NFEAT 1 0\nPD 0 5 3\nC2 1 15 10 1 2 1 0 0\nR\nLN 1 2\nTDS 15 9 80 0.1 0 1 0\nRO 2 1 0 3\nV 1200 -1 1 0\n"
              "L 1200 NLABEL\n")


def test_6_features_norm_network_chain():
    """StreamingFeatures -> StreamingLocalNorm (in place, on the feature step's view) -> StreamingSession on 0.5 s of seeded audio
    in 80 ms chunks against the whole-utterance eval forward of local_normalize(Mfsc(x)), within the streaming forward's 1e-4 bar"""
    fe = Mfsc(num_filters=80)
    nlabel, left = 29, 20
    tr = Trainer(CHAIN_ARCH, 80, nlabel, "ctc")
    tr.init_params(3)
    tr.to_device()
    x = (np.random.default_rng(21).normal(size=8000) * 3000.0).astype(np.float32)
    feats = local_normalize(fe(torch.from_numpy(x).cuda()[None]), None, left, 0)
    T = feats.shape[2]
    assert T == fe.num_frames(len(x)) == 48
    tr.plan(1, T, 1)
    ref = tr.forward(feats.contiguous(), train=False)[0].cpu().numpy().copy()
    fs = StreamingFeatures(fe, 1, 1280)
    ln = StreamingLocalNorm(80, 1, fs.max_out, left)
    ss = StreamingSession(tr, 1, fs.max_out)
    em, normed = [], []
    chunks = [min(1280, len(x) - p) for p in range(0, len(x), 1280)]
    pos = 0
    for i, c in enumerate(chunks):
        pcm = torch.full((1, 1280), float("nan"), device="cuda")
        pcm[0, :c] = torch.from_numpy(x[pos:pos + c]).cuda()
        pos += c
        st, fi = [int(i == 0)], [int(i == len(chunks) - 1)]
        f, nf = fs.step(pcm, [c], st, fi)
        assert ln.step(f, nf, st) is f                     # in place on the feature session's output view
        normed.append(f[0, :, :nf[0]].clone())
        out, n_out = ss.step(f, nf, st, fi)
        em.append(out[0, :n_out[0]].clone())
    normed = torch.cat(normed, dim=1)
    assert normed.shape == feats[0].shape
    # the streamed features are Mfsc's up to summation order (1e-4 of the largest magnitude); the normalisation adds nothing to that
    assert (normed - feats[0]).abs().max() < 1e-3
    em = torch.cat(em).cpu().numpy()
    assert em.shape == ref.shape
    err = np.abs(em - ref).max() / np.abs(ref).max()
    print(f"chain: {ref.shape[0]} emission frames, max err / max |ref| = {err:.3g}")
    assert err < 1e-4, err


# ---------------------------------------------------------------------------------------------- 7: Train on list files
def _rows(text):
    r = []
    for line in text.splitlines():
        if line.startswith("epoch:"):
            r.append({k.strip(): v.strip() for k, v in (item.split(":", 1) for item in line.split(" | "))})
    return r


def _one_update(d, model, run, extra):
    """`Train fork <model>`: one update at --lr=0 --lrcrit=0 on the checkpoint's network, the checkpoint's flags plus `extra`"""
    cmd = [_train_cmd(d, run)[0], "fork", str(model), f"--rundir={run}", "--iter=1", "--reportiters=1", "--lr=0", "--lrcrit=0"] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=ENV)


def test_7_train_reads_the_context_flags(tmp_path):
    """the six-WAV fixture.  A freshly initialised network of this arch emits the same scores whatever it is fed (its reported loss
    is the same to every printed digit under any normalisation), so the update that is compared runs on a network that has trained
    for the fixture's six updates first: `Train fork` of that checkpoint, one update at --lr=0 --lrcrit=0."""
    d = tmp_path
    _fixture(d)
    first = subprocess.run(_train_cmd(d, d / "first"), capture_output=True, text=True, timeout=600, env=ENV)
    assert first.returncode == 0, first.stdout[-2000:] + first.stderr[-2000:]
    model = d / "first" / "exp" / "001_model_last.bin"
    plain = _one_update(d, model, d / "plain", [])
    whole = _one_update(d, model, d / "whole", ["--localnrmlleftctx=100000", "--localnrmlrightctx=100000"])
    local = _one_update(d, model, d / "local", ["--localnrmlleftctx=5"])
    for out in (plain, whole, local):
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    l0, l1, l2 = (float(_rows(o.stdout)[-1]["loss"]) for o in (plain, whole, local))
    print(f"Train loss: whole utterance {l0!r}, both contexts 100000 {l1!r}, left context 5 {l2!r}")
    # every window the whole utterance: the flag-free normalisation up to how mean and variance are rounded (fp32 parity bar)
    assert np.isfinite(l0) and abs(l1 - l0) <= 1e-4 * abs(l0), (l0, l1)
    assert np.isfinite(l2) and l2 != l0, (l0, l2)
    bad = _one_update(d, model, d / "bad", ["--localnrmlleftctx=-1"])
    assert bad.returncode != 0 and "localnrmlleftctx" in bad.stdout + bad.stderr, bad.stdout[-500:] + bad.stderr[-500:]
