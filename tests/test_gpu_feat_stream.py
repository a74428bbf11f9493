"""GPU tests of the streaming log-mel front end (wav2letter_amd/streaming.py StreamingFeatures, csrc/host/feat_stream.cpp,
csrc/feat_stream.hip): the features of an utterance do not depend on how its audio was chunked -- bit for bit --, they are
oracle.mfsc's and Mfsc's within the bar test_mfsc_features_on_device sets (1e-4 of the largest feature magnitude), frame counts
exactly; int16 input, the edges, the hand-over to StreamingSession / StreamingDecoder and the three surfaces."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import feat_stream_ref as R
from wav2letter_amd import _lib
from wav2letter_amd.features import Mfsc
from wav2letter_amd.streaming import StreamingDecoder, StreamingFeatures, StreamingSession, feat_desc
from wav2letter_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
TILE = 16   # frames per workgroup (w2l_feat_stream_tile_rows)

GEOMS = {
    "16k_f80": dict(num_filters=80),
    "16k_f40_power": dict(num_filters=40, use_power=True),
    "8k": dict(num_filters=80, fs=8000),                               # N = 200, St = 80, 129 bins
    "toy": dict(num_filters=5, fs=1000, frame_ms=10, stride_ms=3),     # N = 10, St = 3, 9 bins
}


def noise(seed, n):
    return (np.random.default_rng(seed).normal(size=n) * 3000.0).astype(np.float32)


def run_jobs(sess, jobs, dtype=np.float32, poison=True):
    """jobs: (slot, first_step, x [T], chunks).  Drives the session step by step -- a job's first chunk carries `start`, its last
    `finish`; with `poison`, samples nobody may read (columns at or beyond n[s], whole rows of idle slots) are NaN (int16: -32768).
    Checks at every step that what was written is finite and that columns at or beyond n_out[s] keep what they held.  Returns per
    job (features [F][n] on the device, frames per step)."""
    S, cmax = sess.slots, sess.max_samples
    steps = max(first + len(chunks) for _, first, _, chunks in jobs)
    got = [[] for _ in jobs]
    per_step = [[] for _ in jobs]
    pos = [0] * len(jobs)
    bad = (np.nan if dtype == np.float32 else -32768) if poison else 0
    prev = sess.feats.clone() if sess.feats is not None else None
    for i in range(steps):
        xs = np.full((S, cmax), bad, dtype)
        n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        live = {}
        for j, (slot, first, x, chunks) in enumerate(jobs):
            k = i - first
            if 0 <= k < len(chunks):
                assert slot not in live, "two jobs on one slot in one step"
                live[slot] = j
                c = chunks[k]
                xs[slot, :c] = x[pos[j]:pos[j] + c]
                pos[j] += c
                n[slot], st[slot], fi[slot] = c, k == 0, k == len(chunks) - 1
        out, n_out = sess.step(torch.tensor(xs, device="cuda"), n, st, fi)
        assert out.shape == (S, sess.nfeat, sess.max_out) and n_out.max() <= sess.max_out
        if prev is None:
            prev = torch.zeros_like(out)   # the output area is zeroed at bind
        for slot in range(S):
            k = int(n_out[slot])
            assert torch.equal(out[slot, :, k:], prev[slot, :, k:]), f"step {i}: slot {slot} wrote at or beyond its {k} frames"
            assert torch.isfinite(out[slot, :, :k]).all()
            if slot in live:
                got[live[slot]].append(out[slot, :, :k].clone())
                per_step[live[slot]].append(k)
            else:
                assert k == 0
        prev = out.clone()
    for j, (_, _, x, _) in enumerate(jobs):
        assert pos[j] == len(x)
    return [(torch.cat(g, dim=1), p) for g, p in zip(got, per_step)]


class Geometry:
    """one geometry's Mfsc, session (three slots, steps of up to TILE + 4 strides), utterances of about 0.3 s and their features
    from the session fed max_samples at a time: computed once, shared, never changed"""

    def __init__(self, name):
        self.kw = GEOMS[name]
        self.fe = Mfsc(**self.kw)
        N, St = self.fe.N, self.fe.S
        self.max_samples = (TILE + 4) * St
        self.sess = StreamingFeatures(self.fe, 3, self.max_samples)
        fs = self.kw.get("fs", 16000)
        self.utts = [noise(100 + i, n) for i, n in enumerate((int(0.3 * fs) + 17, int(0.25 * fs) + 3, int(0.2 * fs)))]
        self.short = noise(7, N + 2 * St + 1)
        self.ref = self.features(self.utts)
        self.ref_short = self.features([self.short])[0]

    def features(self, utts):
        jobs = [(s, 0, x, R.fixed(len(x), self.max_samples)) for s, x in enumerate(utts)]
        return [g for g, _ in run_jobs(self.sess, jobs)]


_geoms = {}


def geom(name):
    if name not in _geoms:
        _geoms[name] = Geometry(name)
    return _geoms[name]


# ---------------------------------------------------------------------------------------------- F1: chunk invariance, bit for bit
CHUNKINGS = ["1", "St-1", "St", "St+1", "N-1", "N", "N+1", "max", "random", "frames15", "frames16", "frames17"]


@pytest.mark.parametrize("chunking", CHUNKINGS)
@pytest.mark.parametrize("name", list(GEOMS))
def test_f1_chunk_invariance_bit_for_bit(name, chunking):
    g = geom(name)
    N, St, cmax = g.fe.N, g.fe.S, g.max_samples
    rng = np.random.default_rng(len(name) * 131 + CHUNKINGS.index(chunking))
    if chunking == "1":   # one sample per step: the short signal on slot 1, the other slots idle throughout
        (got, per_step), = run_jobs(g.sess, [(1, 0, g.short, [1] * len(g.short))])
        assert sum(per_step) == g.fe.num_frames(len(g.short)) == 3
        assert torch.equal(got, g.ref_short)
        return
    if chunking == "random":
        plans = [R.random_chunking(rng, len(x), cmax, p_zero=0.3) for x in g.utts]
        assert any(0 in p for p in plans)
    elif chunking.startswith("frames"):   # a first step of exactly TILE - 1 / TILE / TILE + 1 frames, the rest in random chunks
        k = int(chunking[6:])
        first = N + (k - 1) * St
        assert first <= cmax and k in (TILE - 1, TILE, TILE + 1)
        plans = [[first] + R.random_chunking(rng, len(x) - first, cmax, p_zero=0.1) for x in g.utts]
    else:
        c = {"St-1": St - 1, "St": St, "St+1": St + 1, "N-1": N - 1, "N": N, "N+1": N + 1, "max": cmax}[chunking]
        plans = [R.fixed(len(x), c) for x in g.utts]
    # three slots at different phases: slot 1 starts two steps late, slot 2 one step late and sits through four steps without a
    # sample in the middle of its utterance
    idle = min(2, len(plans[2]))
    plans[2] = plans[2][:idle] + [0, 0, 0, 0] + plans[2][idle:]
    res = run_jobs(g.sess, [(0, 0, g.utts[0], plans[0]), (1, 2, g.utts[1], plans[1]), (2, 1, g.utts[2], plans[2])])
    for s, (got, per_step) in enumerate(res):
        assert sum(per_step) == g.fe.num_frames(len(g.utts[s])) == g.ref[s].shape[1]
        if chunking.startswith("frames"):
            assert per_step[0] == int(chunking[6:])
        assert torch.equal(got, g.ref[s]), (name, chunking, s)
    assert res[2][1][idle:idle + 4] == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- F2: against the oracle and Mfsc
@pytest.mark.parametrize("name", list(GEOMS))
def test_f2_features_equal_the_oracle_and_mfsc(oracle, name):
    g = geom(name)
    kw = dict(g.kw)
    F = kw.pop("num_filters")
    for s, x in enumerate(g.utts + [g.short]):
        got = (g.ref[s] if s < 3 else g.ref_short).cpu().numpy()
        want = oracle.mfsc(x, F, **kw).T
        assert got.shape == want.shape == (F, g.fe.num_frames(len(x)))   # the frame count is exact
        assert np.abs(want).max() > 5.0 and np.abs(np.diff(want, axis=1)).max() > 1e-2 * np.abs(want).max()
        err = np.abs(got - want).max() / np.abs(want).max()
        whole = g.fe(torch.tensor(x[None], device="cuda"))[0].cpu().numpy()
        assert whole.shape == want.shape
        err_mfsc = np.abs(got - whole).max() / np.abs(want).max()
        print(f"{name} utterance {s}: {want.shape[1]} frames, max err / max |want| = {err:.3g} to the oracle, {err_mfsc:.3g} to Mfsc "
              f"(Mfsc to the oracle {np.abs(whole - want).max() / np.abs(want).max():.3g})")
        assert err < TOL, (name, s, err)
        assert err_mfsc < TOL, (name, s, err_mfsc)


# ---------------------------------------------------------------------------------------------- F3: int16
def test_f3_int16_equals_float_scaled_by_32768():
    """int16 samples scaled by exactly 1 / 32768 on the way into the window; the mel floor is lowered so that audio of that scale
    is above it (at the default floor of 1 every feature would be log(1))"""
    fe = Mfsc(num_filters=80, mel_floor=1e-6)
    x16 = [np.clip(np.round(noise(200 + i, n)), -32768, 32767).astype(np.int16) for i, n in enumerate((4817, 3200))]
    xf = [(torch.tensor(x).float() / 32768).numpy() for x in x16]
    sess = StreamingFeatures(fe, 2, 1000)
    plans = [R.fixed(4817, 1000), R.fixed(3200, 333)]
    a = run_jobs(sess, [(s, 0, x16[s], plans[s]) for s in range(2)], dtype=np.int16)
    b = run_jobs(sess, [(s, 0, xf[s], plans[s]) for s in range(2)])
    for s in range(2):
        assert a[s][1] == b[s][1] and a[s][0].shape[1] == fe.num_frames(len(x16[s]))
        assert a[s][0].std() > 0.1   # no constant
        assert torch.equal(a[s][0], b[s][0])


# ---------------------------------------------------------------------------------------------- F4: edges
def test_f4_shorter_than_one_frame():
    g = geom("16k_f80")
    sess = StreamingFeatures(g.fe, 2, 400)
    (got, per_step), = run_jobs(sess, [(1, 0, noise(1, 399), [399])])
    assert per_step == [0] and got.shape == (80, 0)
    assert sess.slot_state(1) == (False, 0)
    (got, per_step), = run_jobs(sess, [(1, 0, noise(1, 399), [200, 199, 0])])
    assert per_step == [0, 0, 0] and sess.slot_state(1) == (False, 0)


@pytest.mark.parametrize("extra", [0, 1])
def test_f4_finish_on_and_just_past_a_frame_boundary(oracle, extra):
    g = geom("16k_f80")
    T = 400 + 3 * 160 + extra
    x = noise(3 + extra, T)
    sess = StreamingFeatures(g.fe, 1, 500)
    (got, per_step), = run_jobs(sess, [(0, 0, x, R.fixed(T, 500))])
    (one, _), = run_jobs(StreamingFeatures(g.fe, 1, T), [(0, 0, x, [T])])
    assert sum(per_step) == 4 == one.shape[1] and torch.equal(got, one)
    want = oracle.mfsc(x, 80).T
    assert np.abs(got.cpu().numpy() - want).max() < TOL * np.abs(want).max()
    assert sess.slot_state(0) == (False, 0)


def test_f4_restart_after_finish_and_after_reset_leaks_no_carry():
    g = geom("8k")
    a, b = noise(11, 2000), noise(12, 1500)
    (fresh, _), = run_jobs(StreamingFeatures(g.fe, 2, 300), [(0, 0, b, R.fixed(1500, 300))])
    sess = StreamingFeatures(g.fe, 2, 300)
    res = run_jobs(sess, [(0, 0, a, R.fixed(2000, 300)), (0, 7, b, R.fixed(1500, 300)), (1, 1, a, R.fixed(2000, 170))])
    assert torch.equal(res[1][0], fresh)   # B after A finished (A left 2000 - 23 * 80 = 160 samples behind)
    assert torch.equal(res[0][0], res[2][0])
    # A abandoned mid-utterance with a carry, the slot reset, B started on it
    sess.step(torch.tensor(np.stack([a[:300], a[:300]]), device="cuda"), [300, 0], [1, 0])
    sess.step(torch.tensor(np.stack([a[300:600], a[:300]]), device="cuda"), [250, 0])
    assert sess.slot_state(0) == (True, 550 - 5 * 80)
    sess.reset(0)
    assert sess.slot_state(0) == (False, 0)
    with pytest.raises(_lib.W2LInvalidArgument, match="before it was started"):
        sess.step(torch.zeros(2, 300, device="cuda"), [1, 0])
    (again, _), = run_jobs(sess, [(0, 0, b, R.fixed(1500, 300))])
    assert torch.equal(again, fresh)
    # and without the reset: B's start alone discards A's carry
    sess.step(torch.tensor(np.stack([a[:300], a[:300]]), device="cuda"), [290, 0], [1, 0])
    (again, _), = run_jobs(sess, [(0, 0, b, R.fixed(1500, 300))])
    assert torch.equal(again, fresh)


def test_f4_poisoned_samples_change_nothing():
    """NaN in every pcm column at or beyond n[s] and in the whole row of an idle slot (run_jobs' default) against a clean run"""
    g = geom("16k_f40_power")
    plans = [R.fixed(len(x), 700) for x in g.utts]
    jobs = [(0, 0, g.utts[0], plans[0]), (1, 3, g.utts[1], plans[1]), (2, 1, g.utts[2], plans[2][:1] + [0, 0] + plans[2][1:])]
    clean = run_jobs(g.sess, jobs, poison=False)
    dirty = run_jobs(g.sess, jobs, poison=True)
    for s in range(3):
        assert clean[s][1] == dirty[s][1]
        assert torch.equal(clean[s][0], dirty[s][0]) and torch.equal(clean[s][0], g.ref[s])


# ---------------------------------------------------------------------------------------------- F5: hand-over
HANDOVER_ARCH = ("V -1 NFEAT 1 0\nPD 0 5 3\nC2 1 15 10 1 2 1 0 0\nR\nLN 1 2\nTDS 15 9 80 0.1 0 1 0\nRO 2 1 0 3\nV 1200 -1 1 0\n"
                 "L 1200 NLABEL\n")


def test_f5_features_feed_the_streaming_session_and_decoder():
    """audio -> StreamingFeatures -> StreamingSession (max_chunk == max_out) -> StreamingDecoder under two chunkings of the audio:
    emissions against Trainer.forward(train=False) on the one-chunk features within the session's 1e-4 bar, frame counts exact,
    labels identical"""
    g = geom("16k_f80")
    nlabel = 29
    tr = Trainer(HANDOVER_ARCH, 80, nlabel, "ctc")
    tr.init_params(3)
    tr.to_device()
    x = noise(21, 8000 + 77)
    (feats, _), = run_jobs(StreamingFeatures(g.fe, 1, len(x)), [(0, 0, x, [len(x)])])
    T = feats.shape[1]
    assert T == g.fe.num_frames(len(x)) == 48
    tr.plan(1, T, 1)
    ref = tr.forward(feats[None].contiguous(), train=False)[0].cpu().numpy().copy()
    runs = []
    for chunks in (R.fixed(len(x), 1600), R.random_chunking(np.random.default_rng(5), len(x), 1100, p_zero=0.2)):
        fs = StreamingFeatures(g.fe, 1, 1600)
        ss = StreamingSession(tr, 1, fs.max_out)
        dec = StreamingDecoder(1, ss.max_out, 64, nlabel, beam=16, beam_token=16)
        em, pos = [], 0
        for i, c in enumerate(chunks):
            pcm = torch.full((1, 1600), float("nan"), device="cuda")
            pcm[0, :c] = torch.tensor(x[pos:pos + c], device="cuda")
            pos += c
            st, fi = [int(i == 0)], [int(i == len(chunks) - 1)]
            f, nf = fs.step(pcm, [c], st, fi)
            out, n_out = ss.step(f, nf, st, fi)          # the feature step's output as it is
            dec.step(out, n_out, st)
            em.append(out[0, :n_out[0]].clone())
        em = torch.cat(em).cpu().numpy()
        labels, lengths, _ = dec.result()
        runs.append((em, labels[0, 0, :int(lengths[0, 0])].cpu().numpy().copy()))
    for em, _ in runs:
        assert em.shape == ref.shape   # the frame count is exact
        err = np.abs(em - ref).max() / np.abs(ref).max()
        print(f"hand-over: {ref.shape[0]} emission frames, max err / max |ref| = {err:.3g}")
        assert err < TOL, err
    print("hand-over: emissions of the two chunkings bit-equal:", np.array_equal(runs[0][0], runs[1][0]))
    assert np.array_equal(runs[0][1], runs[1][1])
    assert len(runs[0][1]) > 0


# ---------------------------------------------------------------------------------------------- F6: the three surfaces
def test_f6_three_surfaces_agree(tmp_path):
    """C ABI through ctypes == Python StreamingFeatures == compiled C++ fl::pkg::speech::StreamingFeatures
    (tests/cpp/feat_stream_caller.cpp, plain g++ against libw2l_hip.so), bit for bit on one chunked utterance per slot.  The
    tables are fl::lib::audio::Mfsc's: the caller writes them out and the other two surfaces bind the same numbers (the Python
    Mfsc computes its own, equal to rounding)."""
    exe = str(tmp_path / "feat_stream_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "feat_stream_caller.cpp"), "-o", exe, "-L" + libdir, "-lw2l_hip",
                    "-Wl,-rpath," + libdir, "-ldl"], check=True)
    S, cmax, F = 2, 1000, 40
    xs = [noise(31, 4817), noise(32, 3200)]
    plans = [R.fixed(4817, 1000), [0] + R.fixed(3200, 333)]
    steps, pos = [], [0, 0]
    for i in range(max(len(p) for p in plans)):
        x = np.zeros((S, cmax), np.float32)
        n, st, fi = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(S, np.int32)
        for s in range(S):
            if i < len(plans[s]):
                c = plans[s][i]
                x[s, :c] = xs[s][pos[s]:pos[s] + c]
                pos[s] += c
                n[s], st[s], fi[s] = c, i == 0, i == len(plans[s]) - 1
        steps.append((x, n, st, fi))

    # compiled C++
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(np.array([16000, 25, 10, F, 0, S, cmax, len(steps)], np.int32).tobytes())
        for x, n, st, fi in steps:
            f.write(n.tobytes() + st.tobytes() + fi.tobytes() + x.tobytes())
    run = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "feat stream caller ok" in run.stdout, (run.returncode, run.stdout, run.stderr)
    raw = np.fromfile(outp, np.int32)
    fe = Mfsc(num_filters=F)
    mo, N, St, nb, ld = raw[:5]
    assert (N, St, nb, ld) == (fe.N, fe.S, fe.nb, fe.ld) and mo == (cmax - 1) // St + 1
    at = 5
    G = raw[at:at + N * 2 * nb].view(np.float32).reshape(N, 2 * nb)
    at += G.size
    H = raw[at:at + ld * F].view(np.float32).reshape(ld, F)
    at += H.size
    assert np.abs(G - fe.G.cpu().numpy()).max() < 1e-6 * np.abs(G).max() and np.abs(H - fe.H.cpu().numpy()).max() < 1e-6
    cpp = []
    for _ in steps:
        n_out = raw[at:at + S].copy()
        at += S
        cpp.append((n_out, raw[at:at + S * F * mo].view(np.float32).reshape(S, F, mo).copy()))
        at += S * F * mo
    assert at == len(raw)
    fe.G, fe.H = torch.tensor(G, device="cuda"), torch.tensor(H, device="cuda")

    # Python
    sess = StreamingFeatures(fe, S, cmax)
    assert sess.max_out == mo
    for (x, n, st, fi), (want_n, want) in zip(steps, cpp):
        out, n_out = sess.step(torch.tensor(x, device="cuda"), n, st, fi)
        assert (n_out == want_n).all()
        for s in range(S):
            assert np.array_equal(out[s, :, :n_out[s]].cpu().numpy(), want[s, :, :n_out[s]])
    assert sum(k[0] for k, _ in cpp) == fe.num_frames(4817) and sum(k[1] for k, _ in cpp) == fe.num_frames(3200)

    # C ABI
    L = _lib.lib()
    h = C.c_void_p(0)
    d = feat_desc(fe)
    assert L.w2l_feat_session_create(C.byref(d), S, cmax, C.byref(h)) == 0
    try:
        assert L.w2l_feat_session_max_out(h) == mo
        state = torch.empty(L.w2l_feat_session_state_bytes(h), dtype=torch.uint8, device="cuda")
        assert L.w2l_feat_session_bind(h, fe.G.data_ptr(), fe.H.data_ptr(), state.data_ptr(), state.numel()) == 0
        for (x, n, st, fi), (want_n, want) in zip(steps, cpp):
            xd = torch.tensor(x, device="cuda")
            n_out = np.zeros(S, np.int32)
            ptr = C.c_void_p(0)
            assert L.w2l_feat_session_step(h, xd.data_ptr(), 0, n.ctypes.data, st.ctypes.data, fi.ctypes.data, C.byref(ptr),
                                           n_out.ctypes.data, torch.cuda.current_stream().cuda_stream) == 0
            assert (n_out == want_n).all()
            off = ptr.value - state.data_ptr()
            got = state[off:off + 4 * S * F * mo].view(torch.float32).view(S, F, mo).cpu().numpy()
            for s in range(S):
                assert np.array_equal(got[s, :, :n_out[s]], want[s, :, :n_out[s]])
    finally:
        L.w2l_feat_session_destroy(h)
