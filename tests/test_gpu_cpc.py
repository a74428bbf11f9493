"""The CPC criterion on the device (w2l_cpc_*, csrc/criterion_cpc.hip; the contract is in include/w2l_hip.h) against the float64
restatement of tests/cpc_ref.py.

The bar is the project's fp32 bar: 1e-4 of the largest reference magnitude of each tensor.  Plain torch fp32 against float64 on the
CPU lands at 2e-8 to 5e-7 on the small shapes and at 2.5e-6 on the recipe's, so the bar has room and is not a measurement of the
kernel."""
import os
import subprocess

import numpy as np
import pytest
import torch

import cpc_ref as R
from wav2letter_amd import CPCCriterion, _lib, cpc
from wav2letter_amd.criterion import _CPC, _CPCMask

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
GRADS = ("enc", "ctx", "We", "be", "Wc", "bc")

SHAPES = {  # (B, T, Ce, Cc, D, M, K), tau
    "odd": ((3, 37, 20, 12, 8, 11, 5), 0.1),            # nothing a multiple of 4 or 64, K < M
    "clipped": ((2, 64, 33, 17, 7, 16, 16), 0.05),      # nNegative = 100 clipped to K = M
}
_cases = {}


def case(name):
    """the inputs and the float64 reference of a shape, computed once and shared"""
    if name not in _cases:
        dims, tau = SHAPES[name]
        _cases[name] = R.Case(*dims, tau, seed=len(name))
    return _cases[name]


def within(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{what}: {err:.3g} of the largest reference magnitude")
    assert err < TOL, (what, err)


def run(c):
    """loss and the six gradients of a case through the autograd function (w2l_cpc_forward / w2l_cpc_backward)"""
    t = {k: torch.tensor(getattr(c, k), device="cuda", requires_grad=True) for k in GRADS}
    loss = _CPC.apply(t["enc"], t["ctx"], t["We"], t["be"], t["Wc"], t["bc"], torch.tensor(c.mask_index, device="cuda"),
                      torch.tensor(c.neg, device="cuda"), c.tau)
    loss.backward(torch.tensor(c.g, device="cuda"))
    return loss.detach().cpu().numpy(), {k: v.grad.cpu().numpy() for k, v in t.items()}


def check(c, what):
    loss, grads = run(c)
    within(loss, c.loss, f"{what} loss")
    for k in GRADS:
        within(grads[k], c.grads[k], f"{what} d{k}")
    for k in ("enc", "ctx"):      # written by the call as exactly 0.0f, not assumed: the results start as torch.empty
        rows = grads[k][c.mask == 0]
        assert rows.size and (rows == 0).all() and not np.signbit(rows).any(), (what, k)
    return loss, grads


@pytest.mark.parametrize("name", list(SHAPES))
def test_c1_loss(name):
    c = case(name)
    t = {k: torch.tensor(getattr(c, k), device="cuda") for k in GRADS}
    loss = _CPC.apply(t["enc"], t["ctx"], t["We"], t["be"], t["Wc"], t["bc"], torch.tensor(c.mask_index, device="cuda"),
                      torch.tensor(c.neg, device="cuda"), c.tau)
    within(loss.cpu().numpy(), c.loss, f"C1 {name} loss")


@pytest.mark.parametrize("name", list(SHAPES))
def test_c2_gradients(name):
    check(case(name), f"C2 {name}")


def _repeat_cases():
    B, T, Ce, Cc, D, M, K = dims = (2, 23, 9, 7, 5, 8, 6)
    m = np.arange(M)
    same = np.broadcast_to(((m + 3) % M)[None, :, None], (B, M, K))          # every negative of an anchor is the same index
    # negatives equal to m itself, every other one (with ALL of them equal to m every logit of a row is the same number, the loss
    # is log(K + 1) whatever the inputs and every gradient is zero in exact arithmetic: nothing for a relative bar to hold on to)
    own = np.where(np.arange(K)[None, None, :] % 2 == 0, m[None, :, None], ((m + 2)[None, :, None] + np.arange(K)[None, None, :]) % M)
    own = np.broadcast_to(own, (B, M, K))
    shared = np.zeros((B, M, K), np.int32)                                   # every anchor names position 0, K times
    mixed = np.stack([np.stack([np.array([0, 0, mm, 3, 3, 0])[:K] for mm in range(M)]) for _ in range(B)])
    return dims, {"same": same, "own": own, "shared": shared, "mixed": mixed}


@pytest.mark.parametrize("kind", ["same", "own", "shared", "mixed"])
def test_c3_repeated_negatives(kind):
    """C3: values within the bar, and two runs bit-identical in the loss and in all six gradients"""
    dims, negs = _repeat_cases()
    c = R.Case(*dims, 0.1, seed=11, neg=negs[kind])
    loss, grads = check(c, f"C3 {kind}")
    loss2, grads2 = run(c)
    assert loss.tobytes() == loss2.tobytes()
    for k in GRADS:
        assert grads[k].tobytes() == grads2[k].tobytes(), k


def test_c3_second_backward_on_the_same_workspace_gives_the_same_bits():
    """the backward call leaves what the forward pass stored untouched"""
    c = case("odd")
    L = _lib.lib()
    B, T, Ce, Cc, D, M, K = c.dims
    d = {k: torch.tensor(getattr(c, k), device="cuda") for k in GRADS + ("g", "mask_index", "neg")}
    ws = torch.empty(L.w2l_cpc_workspace_size(*c.dims), dtype=torch.uint8, device="cuda")
    loss = torch.empty(B, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(L.w2l_cpc_forward(B, T, Ce, Cc, D, M, K, c.tau, d["enc"].data_ptr(), d["ctx"].data_ptr(), d["mask_index"].data_ptr(),
                                 d["neg"].data_ptr(), d["We"].data_ptr(), d["be"].data_ptr(), d["Wc"].data_ptr(), d["bc"].data_ptr(),
                                 loss.data_ptr(), ws.data_ptr(), s), "forward")
    outs = []
    for _ in range(2):
        o = [torch.empty_like(d[k]) for k in ("enc", "ctx", "We", "be", "Wc", "bc")]
        _lib.check(L.w2l_cpc_backward(B, T, Ce, Cc, D, M, K, c.tau, d["mask_index"].data_ptr(), d["neg"].data_ptr(), d["We"].data_ptr(),
                                      d["Wc"].data_ptr(), d["g"].data_ptr(), *[v.data_ptr() for v in o], ws.data_ptr(), s), "backward")
        outs.append([v.cpu().numpy().tobytes() for v in o])
    assert outs[0] == outs[1]
    within(loss.cpu().numpy(), c.loss, "loss")


@pytest.mark.parametrize("B,T,C,everything", [(3, 37, 20, False), (1, 70, 257, False), (2, 64, 5, True), (1, 129, 300, True)])
def test_c4_masking(B, T, C, everything):
    """C4: apply_mask and its backward are bitwise the select; demb within the bar.  One utterance; M = T (everything masked);
    more channels than a workgroup has threads; frame counts on both sides of the 64-frame chunks of the embedding's gradient"""
    r = np.random.default_rng(B * T + C)
    x = r.normal(size=(B, T, C)).astype(np.float32)
    emb = r.uniform(-1, 1, size=C).astype(np.float32)
    gy = r.normal(size=(B, T, C)).astype(np.float32)
    mask = np.ones((B, T), np.uint8) if everything else (r.uniform(size=(B, T)) < 0.4).astype(np.uint8)
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    et = torch.tensor(emb, device="cuda", requires_grad=True)
    y = _CPCMask.apply(xt, et, torch.tensor(mask, device="cuda"))
    y.backward(torch.tensor(gy, device="cuda"))
    want = np.where(mask[:, :, None] != 0, emb[None, None, :], x)
    assert y.detach().cpu().numpy().tobytes() == want.astype(np.float32).tobytes()
    dx = np.where(mask[:, :, None] != 0, np.float32(0), gy)
    assert xt.grad.cpu().numpy().tobytes() == dx.astype(np.float32).tobytes()
    demb = (gy.astype(np.float64) * (mask[:, :, None] != 0)).sum((0, 1))
    within(et.grad.cpu().numpy(), demb, "C4 demb")
    x64, e64 = torch.tensor(x, dtype=torch.float64, requires_grad=True), torch.tensor(emb, dtype=torch.float64, requires_grad=True)
    R.apply_mask(x64, torch.tensor(mask), e64).backward(torch.tensor(gy, dtype=torch.float64))
    assert np.abs(e64.grad.numpy() - demb).max() < 1e-12 and (x64.grad.numpy() == dx).all()


def test_c5_recipe_shape():
    """C5: the "small" recipe's shape, loss and gradients within the bar; the products split their reduction at this size and two
    runs are still bit-identical"""
    c = R.Case(3, 800, 512, 768, 256, 400, 100, 0.1, seed=5)
    loss, grads = check(c, "C5")
    loss2, grads2 = run(c)
    assert loss.tobytes() == loss2.tobytes() and all(grads[k].tobytes() == grads2[k].tobytes() for k in GRADS)


def test_c6_python_surface_end_to_end():
    """C6: get_mask, a stand-in context map, forward and backward of CPCCriterion equal the restatement on the same draws"""
    B, T, Ce, Cc, D = 3, 37, 20, 12, 8
    torch.manual_seed(3)
    crit = CPCCriterion(Ce, Cc, D, 1, 2, 3, 5, 4, 0.1).cuda()
    names = [n for n, _ in crit.named_parameters()]
    assert names == ["mask_embedding", "encoder_weight", "encoder_bias", "context_weight", "context_bias"]
    assert [tuple(p.shape) for p in crit.parameters()] == [(Ce,), (D, Ce), (D,), (D, Cc), (D,)]
    assert float(crit.mask_embedding.detach().abs().max()) < 1.0 and crit.prettyString() == "CPCCriterion"
    assert (crit.nOffset, crit.nUnits, crit.nPieces, crit.nBuffer) == (1, 2, 3, 4)
    r = np.random.default_rng(9)
    enc = r.normal(size=(B, T, Ce)).astype(np.float32)
    wmap = (r.normal(size=(Ce, Cc)) / np.sqrt(Ce)).astype(np.float32)
    g = r.uniform(0.5, 1.5, size=B).astype(np.float32)
    frames = [37, 30, 25]
    et = torch.tensor(enc, device="cuda", requires_grad=True)
    wt = torch.tensor(wmap, device="cuda", requires_grad=True)
    masked = crit.get_mask(et, 0.3, 4, frames=frames, seed=17)
    loss = crit(et, masked @ wt)
    loss.backward(torch.tensor(g, device="cuda"))
    mask, index, neg = cpc.sample(B, T, 0.3, 4, 5, frames, 17)
    assert (crit.mask.cpu().numpy() == mask).all() and (crit.mask_index.cpu().numpy() == index).all() and (crit.negatives.cpu().numpy() == neg).all()
    assert crit.num_mask() == index.size and all(index[b].max() < frames[b] for b in range(B))
    p64 = [p.detach().cpu().double().requires_grad_() for p in crit.parameters()]
    e64, w64 = torch.tensor(enc, dtype=torch.float64, requires_grad=True), torch.tensor(wmap, dtype=torch.float64, requires_grad=True)
    m64 = R.apply_mask(e64, torch.tensor(mask), p64[0])
    want = R.loss(e64, m64 @ w64, p64[1], p64[2], p64[3], p64[4], torch.tensor(index, dtype=torch.long), torch.tensor(neg, dtype=torch.long), 0.1)
    (want * torch.tensor(g, dtype=torch.float64)).sum().backward()
    within(loss.detach().cpu().numpy(), want.detach().numpy(), "C6 loss")
    within(et.grad.cpu().numpy(), e64.grad.numpy(), "C6 denc")
    within(wt.grad.cpu().numpy(), w64.grad.numpy(), "C6 dmap")
    for (n, p), q in zip(crit.named_parameters(), p64):
        within(p.grad.cpu().numpy(), q.grad.numpy(), f"C6 d{n}")
    with pytest.raises(_lib.W2LError):
        crit.viterbiPath(et.detach())
    with pytest.raises(_lib.W2LInvalidArgument, match="M >= 4"):
        crit.get_mask(et, 1.0 / T, 3, seed=1)
    with pytest.raises(_lib.W2LInvalidArgument, match="get_mask first"):
        CPCCriterion(Ce, Cc, D, 1, 2, 3, 5, 4, 0.1).cuda()(et, masked @ wt)


@pytest.mark.parametrize("frames", [None, [37, 30, 25]])
def test_c6_cpp_surface(tmp_path, frames):
    """C6: fl::pkg::speech::CPCCriterion through tests/cpp/cpc_caller.cpp (plain g++ against libw2l_hip.so): the header's draws
    equal the Python twin's, the numbers equal the restatement within the bar and the Python surface bit for bit; prettyString,
    viterbiPath throwing, the refusals and a Serializer round trip of the five parameters are checked inside the caller"""
    exe = str(tmp_path / "cpc_caller")
    libdir = os.path.join(ROOT, "wav2letter_amd")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "cpc_caller.cpp"),
                    "-o", exe, "-L" + libdir, "-lw2l_hip", "-Wl,-rpath," + libdir, "-ldl"], check=True)
    B, T, Ce, Cc, D, n_neg, length, seed = 3, 37, 20, 12, 8, 5, 4, 2 ** 40 + 17
    tau, prob = np.float32(0.1), np.float32(0.3)
    r = np.random.default_rng(21)
    f = {k: v.astype(np.float32) for k, v in dict(
        enc=r.normal(size=(B, T, Ce)), ctx=r.normal(size=(B, T, Cc)), g=r.uniform(0.5, 1.5, size=B), gy=r.normal(size=(B, T, Ce)),
        emb=r.uniform(-1, 1, size=Ce), We=r.normal(size=(D, Ce)) / np.sqrt(Ce), be=0.1 * r.normal(size=D),
        Wc=r.normal(size=(D, Cc)) / np.sqrt(Cc), bc=0.1 * r.normal(size=D)).items()}
    fr = frames or []
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    head = np.array([B, T, Ce, Cc, D, n_neg, length, seed & 0xFFFFFFFF, seed >> 32, len(fr)], np.uint32).tobytes()
    inp.write_bytes(head + tau.tobytes() + prob.tobytes() + np.array(fr, np.int32).tobytes() + b"".join(v.tobytes() for v in f.values()))
    out = subprocess.run([exe, str(inp), str(outp), str(tmp_path / "model.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "cpc caller ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
    raw = outp.read_bytes()
    M, K, num_mask = np.frombuffer(raw, np.int32, 3)
    mask, index, neg = cpc.sample(B, T, float(prob), length, n_neg, frames, seed)
    assert (M, K, num_mask) == (index.shape[1], neg.shape[2], index.size)
    at = 12
    got_index = np.frombuffer(raw, np.int32, B * M, at).reshape(B, M)
    at += 4 * B * M
    got_neg = np.frombuffer(raw, np.int32, B * M * K, at).reshape(B, M, K)
    at += 4 * B * M * K
    assert (got_index == index).all() and (got_neg == neg).all()
    got = {}
    for k, shape in (("masked", (B, T, Ce)), ("loss", (B,)), ("enc", (B, T, Ce)), ("ctx", (B, T, Cc)), ("We", (D, Ce)), ("be", (D,)),
                     ("Wc", (D, Cc)), ("bc", (D,)), ("dx", (B, T, Ce)), ("demb", (Ce,))):
        n = int(np.prod(shape))
        got[k] = np.frombuffer(raw, np.float32, n, at).reshape(shape)
        at += 4 * n
    assert at == len(raw)
    sel = mask[:, :, None] != 0
    assert got["masked"].tobytes() == np.where(sel, f["emb"][None, None, :], f["enc"]).astype(np.float32).tobytes()
    assert got["dx"].tobytes() == np.where(sel, np.float32(0), f["gy"]).astype(np.float32).tobytes()
    within(got["demb"], (f["gy"].astype(np.float64) * sel).sum((0, 1)), "C6 C++ demb")
    t = {k: torch.tensor(f[k], dtype=torch.float64, requires_grad=True) for k in GRADS}
    want = R.loss(t["enc"], t["ctx"], t["We"], t["be"], t["Wc"], t["bc"], torch.tensor(index, dtype=torch.long), torch.tensor(neg, dtype=torch.long), float(tau))
    (want * torch.tensor(f["g"], dtype=torch.float64)).sum().backward()
    within(got["loss"], want.detach().numpy(), "C6 C++ loss")
    for k in GRADS:
        within(got[k], t[k].grad.numpy(), f"C6 C++ d{k}")
    # the Python surface on the same operands: the same kernels, the same bits
    d = {k: torch.tensor(f[k], device="cuda", requires_grad=True) for k in GRADS}
    loss = _CPC.apply(d["enc"], d["ctx"], d["We"], d["be"], d["Wc"], d["bc"], torch.tensor(index, device="cuda"), torch.tensor(neg, device="cuda"),
                      float(tau))
    loss.backward(torch.tensor(f["g"], device="cuda"))
    assert loss.detach().cpu().numpy().tobytes() == got["loss"].tobytes()
    for k in GRADS:
        assert d[k].grad.cpu().numpy().tobytes() == got[k].tobytes(), k
