"""End-to-end parity of the C++ host graph (arch file -> layers -> forward / criterion /
backward / SGD) against the oracle-side reference-layout interpreter (tests/refnet.py)."""
import numpy as np
import pytest
import torch

from oracle import refnet

pytestmark = pytest.mark.gpu
TOL = 1e-4


def rel(got, want):
    want = np.asarray(want, np.float64).reshape(-1)
    got = np.asarray(got, np.float64).reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.abs(got - want).max() / max(1e-30, np.abs(want).max())


def build(arch, nfeat, nlabel, crit, mode, transdiag, rng, B, T, L, linseg=0):
    from wav2letter_amd.trainer import Trainer
    tr = Trainer(arch, nfeat, nlabel, crit, mode, transdiag)
    if linseg:
        tr.set_linseg(linseg)
    ref = refnet.RefNet(arch, nfeat, nlabel)
    params = ref.random_params(rng)
    table = tr.param_table()
    assert len(table) == len(params), (len(table), len(params))
    for i, p in enumerate(params):
        assert table[i][1] == p.size, (i, table[i], p.shape)
        tr.import_param(i, p)
    if crit == "asg":
        A = (np.eye(nlabel) * transdiag + 0.1 * rng.normal(size=(nlabel, nlabel))).astype(np.float32)
        tr.host_params[tr.n_net:tr.n_net + nlabel * nlabel] = A.reshape(-1)
    else:
        A = None
    tr.plan(B, T, L)
    tr.to_device()
    return tr, ref, params, A


def check_grads(tr, ref_grads):
    g = tr.grads.cpu().numpy()
    table = tr.param_table()
    worst = 0.0
    for i, want in enumerate(ref_grads):
        if want is None:   # checked by the caller on its own scale
            continue
        got = tr.export_from(i, g)
        e = rel(got, want)
        worst = max(worst, e)
        assert e < 2 * TOL, (i, table[i][0], e)
    return worst


def check_grads_relu_robust(tr, ref_grads, strict_tol=2 * TOL):
    """Gradient parity for a DEEP ReLU network.  relu'(0) is a discontinuity: among the ~3 million ReLU inputs of the full
    TDS-CTC recipe a handful lie within fp32 rounding of zero, and whichever side of zero a kernel's summation order lands
    on decides whether that position passes its gradient.  One flipped position moves a weight gradient by ~1/sqrt(N)
    of its size (a gradient is a sum of N random-sign terms): 0.3 - 4 % -- seen with BOTH conv kernel generations,
    depending on the data (profiles/r02_run4_config2_relu_kink_diag.log, r02_run5_relu_kink_bisect.log).  So: every
    parameter must agree in direction and size (cosine > 0.99, relative L2 error < 10 %: a layout / plumbing error
    gives ~0 cosine), and the strict 2e-4 bar is applied to the shallower networks below, where no input is near a kink."""
    g = tr.grads.cpu().numpy()
    table = tr.param_table()
    n_strict = 0
    for i, want in enumerate(ref_grads):
        got = np.asarray(tr.export_from(i, g), np.float64).reshape(-1)
        w = np.asarray(want, np.float64).reshape(-1)
        l2 = np.linalg.norm(got - w) / max(1e-30, np.linalg.norm(w))
        cos = float(got @ w) / max(1e-30, np.linalg.norm(got) * np.linalg.norm(w))
        assert l2 < 0.1 and cos > 0.99, (i, table[i][0], l2, cos)
        n_strict += rel(got, w) < strict_tol
    return n_strict, len(ref_grads)


def test_tds_ctc_small_end_to_end(oracle):
    from wav2letter_amd import recipes
    rng = np.random.default_rng(0)
    nfeat, nlabel, B, T, L = 8, 21, 3, 64, 6
    arch = recipes.tds_ctc_small_arch(c=(4, 6), h=nfeat, kw=5)
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.full((B, L), -1, np.int32)
    for b in range(B):
        l = int(rng.integers(1, L + 1))
        tgt[b, :l] = rng.integers(0, nlabel - 1, l)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    assert em.shape == em_ref.shape
    assert rel(em, em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < TOL
    d_em = o.backward().astype(np.float32)
    ref_grads = ref.backward(d_em, len(params))
    check_grads(tr, ref_grads)
    # one SGD step with clipping == reference formula on the flat arena
    p0 = tr.params.cpu().numpy().copy()
    g0 = tr.grads.cpu().numpy().copy()
    tr.update(lr=0.3, momentum=0.5, max_grad_norm=1.0, total_batch=B)
    gs = g0.astype(np.float64) / B
    coef = min(1.0, 1.0 / (np.linalg.norm(gs) + 1e-6))
    want = p0 - 0.3 * (gs * coef)
    assert rel(tr.params.cpu().numpy(), want) < 1e-5


@pytest.mark.parametrize("seed", [1, 2])
def test_tds_ctc_random_small_networks(oracle, seed):
    """the reduced TDS-CTC topology over random channel counts (incl. the recipe's 10 / 14 / 18, whose convolutions run on the
    block-Toeplitz kernels when the mel rows are a multiple of 16), mel-row counts, kernel widths, batch and frame counts: emissions
    and loss at 1e-4, every parameter gradient by direction and size (a ReLU input may sit on the kink: check_grads_relu_robust)"""
    from wav2letter_amd import recipes
    rng = np.random.default_rng(4000 + seed)
    for c in range(5):
        chans = [(4, 6), (10, 14), (14, 18), (3, 5), (10, 10)][int(rng.integers(0, 5))]
        nfeat = int(rng.choice([8, 16, 32, 48]))
        kw = int(rng.choice([5, 9, 21]))
        B, T, L = int(rng.integers(1, 4)), int(rng.choice([24, 40, 64, 97])), 4
        nlabel = int(rng.choice([9, 21, 40]))
        arch = recipes.tds_ctc_small_arch(c=chans, h=nfeat, kw=kw)
        what = f"case {c}: channels {chans} nfeat {nfeat} kw {kw} B {B} T {T} nlabel {nlabel}"
        tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
        x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
        tgt = np.full((B, L), -1, np.int32)
        for b in range(B):
            l = int(rng.integers(1, L + 1))
            tgt[b, :l] = rng.integers(0, nlabel - 1, l)
        xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
        em_ref = ref.forward(x, params)
        assert rel(tr.forward(xd, train=False).cpu().numpy(), em_ref) < TOL, what
        loss = tr.forward_backward(xd, torch.tensor(tgt).cuda()).cpu().numpy()
        o = oracle.CTC(em_ref, tgt, scale_mode=4)
        assert rel(loss, o.forward()) < TOL, what
        try:
            check_grads_relu_robust(tr, ref.backward(o.backward().astype(np.float32), len(params)))
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from e


def test_conv_glu_asg_small_end_to_end(oracle):
    """BASELINE config 1 geometry in miniature: WN-Conv+GLU stack, ASG criterion, 2 utterances"""
    from wav2letter_amd import recipes
    rng = np.random.default_rng(1)
    nfeat, nlabel, B, T, L = 6, 9, 2, 40, 7
    arch = recipes.conv_glu_small_arch(widths=(16, 24), kws=(5, 4), pad0=2)
    tr, ref, params, A = build(arch, nfeat, nlabel, "asg", 4, 4.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.array([[1, 2, 3, 1, -1, -1, -1], [0, 5, 5, 2, 7, 1, 0]], np.int32)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    assert em.shape == em_ref.shape, (em.shape, em_ref.shape)
    assert rel(em, em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    ol, odx, odA = oracle.asg(em_ref, A, tgt, 4)
    assert rel(loss, ol) < TOL
    ref_grads = ref.backward(odx.astype(np.float32), len(params))
    check_grads(tr, ref_grads)
    gA = tr.grads.cpu().numpy()[tr.n_net:tr.n_net + nlabel * nlabel]
    assert rel(gA, odA) < TOL
    # Viterbi through the trainer: bit-exact
    path = tr.viterbi(tr.forward(xd, train=False)).cpu().numpy()
    assert (path == oracle.viterbi(em, A)).all()


def test_conv_glu_asg_wide_layers_end_to_end(oracle):
    """the same miniature with layers wide enough for the overlapping-row LDS-DMA convolution path (kw*C_in >= 64,
    C_out >= 32; first layer explicitly padded, second SAME-padded with an even kernel): emissions, loss, every
    parameter gradient (weight-norm v, g, bias) and the transition gradient against the reference network + oracle"""
    from wav2letter_amd import recipes
    rng = np.random.default_rng(5)
    nfeat, nlabel, B, T, L = 16, 9, 3, 50, 7
    arch = recipes.conv_glu_small_arch(widths=(64, 96), kws=(5, 4), pad0=2)
    tr, ref, params, A = build(arch, nfeat, nlabel, "asg", 4, 4.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.array([[1, 2, 3, 1, -1, -1, -1], [0, 5, 5, 2, 7, 1, 0], [4, 4, -1, -1, -1, -1, -1]], np.int32)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    assert em.shape == em_ref.shape, (em.shape, em_ref.shape)
    assert rel(em, em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    ol, odx, odA = oracle.asg(em_ref, A, tgt, 4)
    assert rel(loss, ol) < TOL
    check_grads(tr, ref.backward(odx.astype(np.float32), len(params)))
    gA = tr.grads.cpu().numpy()[tr.n_net:tr.n_net + nlabel * nlabel]
    assert rel(gA, odA) < TOL


def test_tds_ctc_config2_full_network_end_to_end(oracle):
    """BASELINE config 2 -- the full sota/2019 TDS-CTC recipe network (21 TDS blocks, 203.4 M parameters, 80 mel
    rows, 9998 word pieces) -- at a reduced batch and number of frames, with SpecAugment and dropout switched off so
    that both sides see the same activations: emissions, CTC loss and every parameter gradient against the numpy
    reference network + the CTC oracle.  Runs every fc GEMM kernel variant of the step (128x128 and 160-wide tiles,
    the N = 9998 final layer on dword-aligned rows) and the TDS / strided convolutions at the recipe's channel counts."""
    import re
    from wav2letter_amd import recipes
    rng = np.random.default_rng(21)
    nfeat, nlabel, B, T, L = 80, 9998, 2, 96, 5
    arch = re.sub(r"(TDS \d+ \d+ \d+) [0-9.]+", r"\1 0.0", recipes.tds_ctc_arch())
    arch = "\n".join(l for l in arch.splitlines() if not l.startswith("SAUG")) + "\n"
    arch = re.sub(r"^DO [0-9.]+$", "DO 0.0", arch, flags=re.M)
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.full((B, L), -1, np.int32)
    tgt[0, :5] = [17, 4021, 9996, 3, 3]
    tgt[1, :2] = [9000, 12]
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    assert em.shape == em_ref.shape == (B, 12, nlabel)
    assert rel(em, em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < TOL
    n_strict, n = check_grads_relu_robust(tr, ref.backward(o.backward().astype(np.float32), len(params)))
    # the final Linear never sees a ReLU kink between itself and the loss: always at the strict bar
    assert n_strict >= 2


@pytest.mark.parametrize("seed", [23, 21])
def test_tds_ctc_config2_teacher_forced_blocks_fp32(oracle, seed):
    """BASELINE config 2 at FULL DEPTH, block by block, at the strict fp32 bar (round-4 verdict item 6): the 21 TDS blocks of the
    sota/2019 recipe network (C = 10 / 14 / 18, 80 mel rows, kw = 21, fc widths 2400 / 3360 / 4320) each run alone on the
    oracle's activation and upstream gradient -- teacher_forced_tds_blocks_fp32.  The statistical full-depth bars of
    test_tds_ctc_config2_full_network_end_to_end (cosine / relative L2) stay as the end-to-end plumbing check; THIS is the
    per-tensor 1e-4 statement for the headline config: block outputs and the eight parameter gradients of EVERY block -- each
    block's input is first moved off the ReLU kinks with an asserted margin (kink_free_block_input; round-5 verdict, weak 4:
    no `kinked <= 4`, no chosen seed)."""
    import re
    from wav2letter_amd import recipes
    rng = np.random.default_rng(seed)
    nfeat, nlabel, B, T, L = 80, 9998, 2, 200, 5
    arch = re.sub(r"(TDS \d+ \d+ \d+) [0-9.]+", r"\1 0.0", recipes.tds_ctc_arch())
    arch = "\n".join(l for l in arch.splitlines() if not l.startswith("SAUG")) + "\n"
    arch = re.sub(r"^DO [0-9.]+$", "DO 0.0", arch, flags=re.M)
    ref = refnet.RefNet(arch, nfeat, nlabel)
    params = ref.random_params(rng)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.full((B, L), -1, np.int32)
    tgt[0, :5] = [17, 4021, 9996, 3, 3]
    tgt[1, :2] = [9000, 12]
    em_ref = ref.forward(x, params)
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    o.forward()
    ref.upstream = []
    ref_grads = ref.backward(o.backward().astype(np.float32), len(params))
    n, tries, worst = teacher_forced_tds_blocks_fp32(ref, arch, params, ref_grads, seed)
    print("config 2 fp32, seed %d: %d teacher-forced TDS blocks, ALL strict (worst error %.2e); at most %d input perturbations to clear the ReLU kinks" % (seed, n, worst, tries))
    assert n == 21


def relu_kink_margin(ref):
    """smallest |input| / rms over every ReLU of the network the reference interpreter has just run (arch `R` lines and the two
    ReLUs inside every TDS block)"""
    m = np.inf
    for rec in ref.tape:
        zs = [rec[1]] if rec[0] == "R" else [rec[2]["a"], rec[2]["u"]] if rec[0] == "TDS" else []
        for z in zs:
            m = min(m, float(np.abs(z).min() / np.sqrt(np.mean(np.square(z, dtype=np.float64)))))
    return m


@pytest.mark.parametrize("seed", [21, 22, 23, 24, 25, 26])
@pytest.mark.parametrize("stages", [[(10, 1, 2400)], [(10, 1, 0), (14, 1, 0), (18, 1, 0)], [(18, 3, 4320)]])
def test_tds_ctc_recipe_channel_counts_strict_gradients(oracle, stages, seed):
    """the recipe's TDS geometry (80 mel rows, kw = 21, C = 10 / 14 / 18, the 3x fc width, strided C2 layers between the
    stages): every parameter gradient at the strict 2e-4 bar, for EVERY seed (round-5 verdict, weak 4: the round-5 test was
    re-seeded 21 -> 22 when a new summation order put one ReLU input of seed 21 across zero).  relu'(0) is a discontinuity, so the
    test first makes its input kink-free: the features are perturbed (relative 1e-3 noise) until no ReLU input anywhere in the
    oracle's network lies within KINK_MARGIN x rms of zero -- the margin is asserted -- and then nothing is excused."""
    rng = np.random.default_rng(seed)
    nfeat, nlabel, B, T, L = 80, 40, 2, 96, 5
    if sum(nb for _, nb, _ in stages) >= 3 and stages[0][2]:
        B, T = 1, 64   # three wide blocks: 1.8 M ReLU inputs at B = 2, T = 96 -- ~6 of them inside the margin per draw, hundreds of draws
    lines = ["V -1 NFEAT 1 0"]
    cin = 1
    for c, nb, l2 in stages:
        lines += [f"C2 {cin} {c} 21 1 2 1 -1 -1", "R", "DO 0.0", "LN 0 1 2"] + [f"TDS {c} 21 80 0.0 {l2}"] * nb
        cin = c
    lines += [f"V 0 {cin * 80} 1 0", "RO 1 0 3 2", f"L {cin * 80} NLABEL"]
    arch = "\n".join(lines) + "\n"
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    x0 = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)
    best = None
    for k in range(400):
        x = x0 if k == 0 else (x0 * (1.0 + 1e-3 * rng.standard_normal(x0.shape))).astype(np.float32)
        em_ref = ref.forward(x, params)
        m = relu_kink_margin(ref)
        if best is None or m > best[0]:
            best = (m, x)
        if m >= KINK_MARGIN:
            break
    assert best[0] >= KINK_MARGIN, ("no kink-free input found", best[0])
    x = best[1]
    em_ref = ref.forward(x, params)   # (the tape of the input that is used)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    assert rel(tr.forward(xd, train=False).cpu().numpy(), em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < TOL
    check_grads(tr, ref.backward(o.backward().astype(np.float32), len(params)))


def test_librivox_two_dimensional_subsampling_convolutions(oracle):
    """am_tds_ctc_librivox.arch's geometry: `C2 cin cout 21 3 2 1 -1 -1` (21 frames x 3 mel rows, SAME on both axes)
    between TDS stages of 16 / 32 channels on 80 mel rows -- emissions, CTC loss and every parameter gradient (the
    [cout][cin][kh][kw] kernels included) against the reference network + criterion oracle"""
    rng = np.random.default_rng(33)
    nfeat, nlabel, B, T, L = 80, 30, 2, 64, 5
    arch = ("V -1 NFEAT 1 0\nC2 1 16 21 3 2 1 -1 -1\nR\nDO 0.0\nLN 0 1 2\nTDS 16 21 80 0.0 2400\nC2 16 32 21 3 2 1 -1 -1\nR\nDO 0.0\n"
            "LN 0 1 2\nTDS 32 21 80 0.0 0\nV 0 2560 1 0\nRO 1 0 3 2\nL 2560 NLABEL\n")
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em_ref = ref.forward(x, params)
    assert rel(tr.forward(xd, train=False).cpu().numpy(), em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < TOL
    check_grads(tr, ref.backward(o.backward().astype(np.float32), len(params)))


@pytest.mark.parametrize("T,csz", [(21, 12), (44, 5)])
def test_transformer_ctc_small_end_to_end(oracle, T, csz):
    """the shape of am_transformer_ctc.arch at reduced widths -- WN-conv + GLU + max-pool front end, Reorder, two TR blocks
    (position table longer / shorter than the utterance), Linear -- emissions, CTC loss and every parameter gradient
    (position tables included) against the reference-layout interpreter + criterion oracle"""
    rng = np.random.default_rng(T)
    nfeat, nlabel, B, L = 16, 12, 3, 4
    arch = ("V -1 1 NFEAT 0\nWN 3 C NFEAT 64 3 1 -1\nGLU 2\nDO 0.0\nM 1 1 2 1\nRO 2 0 3 1\n"
            f"TR 32 64 4 {csz} 0.0 0.0\nTR 32 64 4 {csz} 0.0 0.0\nDO 0.0\nL 32 NLABEL\n")
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em_ref = ref.forward(x, params)
    em = tr.forward(xd, train=False).cpu().numpy()
    assert em.shape == em_ref.shape
    assert rel(em, em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < TOL
    want = ref.backward(o.backward().astype(np.float32), len(params))
    # the key bias shifts every score of a query by the same q_i . b_k, which softmax ignores: its gradient is exactly
    # zero and both sides only hold rounding noise there -- compare it on the scale of the query bias gradient instead
    g = tr.grads.cpu().numpy()
    table = tr.param_table()
    for i, (name, _n, _off) in enumerate(table):
        if name == "tr.wk.b":
            qb = np.abs(want[i - 2]).max()
            assert table[i - 2][0] == "tr.wq.b" and np.abs(want[i]).max() < 1e-9 * qb
            assert np.abs(tr.export_from(i, g)).max() < 1e-5 * qb, (i, name)
            want[i] = None
    check_grads(tr, want)


@pytest.mark.parametrize("mid", ["DO 0.4", "R", "DO 0.4\nR"])
def test_mixed_precision_images_are_not_reused_across_in_place_layers(oracle, mid):
    """`TR ... / DO p / L` (recipes/sota/2019/am_arch/am_transformer_ctc.arch, the order of the repo's own recipes.py) in the
    mixed-precision mode: a Transformer block writes the bf16 images of its output for the next fl::Linear; a Dropout (in
    training) or ReLU between the two rewrites that activation IN PLACE, so the images are stale and the Linear has to
    convert again (round-4 advisor finding: it did not -- the final dropout was silently skipped in the forward and in the
    weight gradient).  Training-mode emissions and every gradient of the bf16 step against the SAME step in fp32 (the dropout
    mask is a stateless hash of (element, seed, layer): identical on both sides) at the bf16 bars; with the stale images the
    emissions differ by the whole dropout mask (tens of percent)"""
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(7)
    nfeat, nlabel, B, T, L = 64, 24, 3, 40, 5
    arch = f"V -1 1 NFEAT 0\nRO 2 0 3 1\nTR 64 128 4 30 0.0 0.0\n{mid}\nL 64 NLABEL\n"
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    outs = {}
    for mp in (False, True):
        tr = Trainer(arch, nfeat, nlabel, "ctc", 4)
        tr.init_params(seed=11)
        tr.plan(B, T, L)
        tr.to_device()
        tr.set_mixed_precision(mp)
        tr.set_step(3)
        em = tr.forward(x, train=True).clone()
        tr.set_step(3)
        loss = tr.forward_backward(x, tgt).clone()
        outs[mp] = (em, loss, tr.grads.clone(), tr)
    em32, l32, g32, _ = outs[False]
    em16, l16, g16, tr16 = outs[True]
    assert not torch.equal(em16, em32)          # the bf16 path really ran
    assert (em16 - em32).abs().max().item() < 2e-2 * em32.abs().max().item()
    assert (l16 - l32).abs().max().item() < 2e-2 * l32.abs().max().item()
    for name, n, off in tr16.param_table():
        a, b = g16[off:off + n].double(), g32[off:off + n].double()
        if n < 64 or b.norm().item() < 1e-12 or name == "tr.wk.b":
            continue
        l2 = ((a - b).norm() / b.norm()).item()
        assert l2 < 0.1, (name, l2)


def test_transformer_block_at_config5_width(oracle):
    """one TR block at the recipe's own width -- `TR 1024 4096 4 460`: 4 heads of 256, 919-row position table, 188 frames
    (T = 1500 after the three max-pools), i.e. the GEMM / batched-GEMM / softmax launch shapes of BASELINE config 5 at a
    2-utterance batch -- emissions, CTC loss and every parameter gradient against the float64 restatement"""
    rng = np.random.default_rng(12)
    nfeat, nlabel, B, T, L = 1024, 40, 2, 188, 20
    arch = "V -1 1 NFEAT 0\nRO 2 0 3 1\nTR 1024 4096 4 460 0.0 0.0\nL 1024 NLABEL\n"
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em_ref = ref.forward(x, params)
    assert rel(tr.forward(xd, train=False).cpu().numpy(), em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < TOL
    want = ref.backward(o.backward().astype(np.float32), len(params))
    g = tr.grads.cpu().numpy()
    for i, (name, _n, _off) in enumerate(tr.param_table()):
        if name == "tr.wk.b":   # exactly zero (see test_transformer_ctc_small_end_to_end)
            assert np.abs(tr.export_from(i, g)).max() < 1e-5 * np.abs(want[i - 2]).max()
            want[i] = None
    check_grads(tr, want)


def test_transformer_block_at_config5_width_bf16(oracle):
    """the same block in the mixed-precision mode (BASELINE config 5's dtype): every product -- the six fl::Linear GEMMs and
    the attention products Q K^T, Q E^T, P V and their gradients -- on bf16-rounded operands with fp32 accumulation, softmax /
    LayerNorm / CTC in fp32.  Against the UNROUNDED float64 restatement at the stated bf16 tolerance: emissions and CTC loss
    1e-2 of the largest magnitude; parameter gradients by direction and size (a bf16 operand carries 2^-9 relative rounding,
    a gradient is a sum of many such terms: cosine > 0.995, relative L2 < 8 %)"""
    rng = np.random.default_rng(12)
    nfeat, nlabel, B, T, L = 1024, 40, 2, 188, 20
    arch = "V -1 1 NFEAT 0\nRO 2 0 3 1\nTR 1024 4096 4 460 0.0 0.0\nL 1024 NLABEL\n"
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    tr.set_mixed_precision(True)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em_ref = ref.forward(x, params)
    em = tr.forward(xd, train=False).cpu().numpy()
    assert rel(em, em_ref) < 1e-2
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < 1e-2
    want = ref.backward(o.backward().astype(np.float32), len(params))
    g = tr.grads.cpu().numpy()
    for i, (name, _n, _off) in enumerate(tr.param_table()):
        if name == "tr.wk.b":   # exactly zero in exact arithmetic
            continue
        got = tr.export_from(i, g).astype(np.float64).reshape(-1)
        w = np.asarray(want[i], np.float64).reshape(-1)
        cos = float(got @ w / (np.linalg.norm(got) * np.linalg.norm(w) + 1e-300))
        l2 = float(np.linalg.norm(got - w) / (np.linalg.norm(w) + 1e-300))
        assert cos > 0.995 and l2 < 0.08, (name, cos, l2)


def _one_block_trainer(arch, nfeat, nlabel, B, T, block_params):
    from wav2letter_amd.trainer import Trainer
    tr = Trainer(arch, nfeat, nlabel, "ctc", 4, 0.0)
    table = tr.param_table()
    assert len(table) == len(block_params), (len(table), len(block_params))
    for i, p in enumerate(block_params):
        assert table[i][1] == np.asarray(p).size, (i, table[i], np.asarray(p).shape)
        tr.import_param(i, p)
    tr.plan(B, T, 1)
    tr.to_device()
    tr.set_mixed_precision(True)
    return tr, table


def teacher_forced_tds_blocks(ref, arch, params, ref_grads):
    """Every TDS block of the network ALONE, in the mixed-precision mode, at the geometry and with the parameters it has in the
    network: fed the oracle's own input activation of that block and the oracle's own gradient at its output (recorded by
    RefNet.backward in ref.upstream), through a one-block `V / TDS / RO / V / V` network and w2l_trainer_backward -- output and
    every parameter gradient of the block against the bf16-operand oracle's at 2e-3 of the largest magnitude (LayerNorm pairs
    2e-2): with the inputs forced nothing compounds, what is left is fp32 accumulation order and the odd one-sided rounding."""
    lines = [l.split() for l in arch.splitlines() if l.startswith("TDS")]
    blocks = [(rec, da) for rec, da in reversed(ref.upstream) if rec[0] == "TDS"]     # network order
    assert len(blocks) == len(lines) > 0
    worst = 0.0
    for (rec, da), tok in zip(blocks, lines):
        _, p, saved, pl, pr, mode, pi = rec
        xin = np.ascontiguousarray(saved["x"], dtype=np.float32)                        # [B][c][h][T]
        B, c, h, T = xin.shape
        assert (c, h) == (int(tok[1]), int(tok[3]))
        l = c * h
        out = refnet.tds_fwd(xin, p, pl, pr, mode, bf16=True)
        # the features are read as (T, c, h, B) and reordered to the block's (T, h, c, B): feature index c + C h, channels contiguous,
        # the layout the recipe's C2 line leaves
        one = ("V -1 %d %d 0\nRO 0 2 1 3\n%s\nRO 2 1 0 3\nV %d -1 1 0\nV %d 0 -1 1\n" % (c, h, " ".join(tok[:4] + ["0.0"] + tok[5:]), l, l))
        tr, table = _one_block_trainer(one, l, l, B, T, params[pi - 8:pi])
        to_em = lambda a: np.ascontiguousarray(a.transpose(0, 3, 2, 1)).reshape(B, T, l)   # [B][c][h][T] -> [B][T][h * C + c]
        feed = np.ascontiguousarray(xin.transpose(0, 2, 1, 3)).reshape(B, l, T)            # [B][h * C + c][T]
        em = tr.forward(torch.tensor(feed).cuda(), train=True).cpu().numpy()
        e = rel(em, to_em(out))
        assert e < 2e-3, (pi, tok, "output", e)
        tr.backward(torch.tensor(to_em(np.asarray(da, np.float32))).cuda())
        g = tr.grads.cpu().numpy()
        for i in range(8):
            want = ref_grads[pi - 8 + i]
            err = rel(tr.export_from(i, g), want)
            assert err < (2e-3 if np.asarray(want).size > 2 else 2e-2), (pi, tok, table[i][0], err)
            if np.asarray(want).size > 2:
                worst = max(worst, err, e)
        del tr
    return len(blocks), worst


KINK_MARGIN = 4e-6   # of the rms of a ReLU layer's inputs: twice what an fp32 sum of ~1000 terms can differ by between two summation orders


def kink_free_block_input(xin, p, pl, pr, mode, rng, tries=200):
    """A TDS block has two ReLUs (0.2 - 3.8 M inputs each at the recipe's sizes).  relu'(0) is a discontinuity: an input within fp32
    rounding of zero passes its gradient or not depending on the summation order of whoever computes it, and ONE flipped input
    moves a weight gradient by ~1 / sqrt(N) of its size.  Instead of counting such blocks (round 5: `kinked <= 4`) or choosing a
    seed, the block's input is perturbed (relative noise of 1e-3, a few tries) until NO ReLU input of the oracle's block lies
    within KINK_MARGIN x rms of zero; the margin is asserted, and then every tensor of every block is held to the strict bar.
    Returns (input, oracle output, oracle tape, tries used, smallest |input| / rms over both ReLUs)."""
    best = None
    for k in range(tries):
        x = xin if k == 0 else (xin * (1.0 + 1e-3 * rng.standard_normal(xin.shape))).astype(np.float32)
        out, saved = refnet.tds_fwd(x, p, pl, pr, mode, keep=True)
        m = min(float(np.abs(saved[name]).min() / np.sqrt(np.mean(np.square(saved[name], dtype=np.float64)))) for name in ("a", "u"))
        if best is None or m > best[4]:
            best = (x, out, saved, k + 1, m)
        if m >= KINK_MARGIN:
            break
    return best


def teacher_forced_tds_blocks_fp32(ref, arch, params, ref_grads, seed=0):
    """Every TDS block of the network ALONE in fp32, at the geometry and with the parameters it has in the network, fed the
    oracle's input activation (made kink-free: kink_free_block_input) and the oracle's own gradient at its output: output and every
    parameter gradient at the STRICT bar (1e-4 of the largest reference magnitude; the two-element LayerNorm (gain, offset)
    pairs, sums of every activation with heavy cancellation, 1e-3).  With the inputs forced nothing compounds from block to
    block, and with every ReLU input at least KINK_MARGIN x rms away from zero (asserted) no summation order can flip one:
    EVERY block is strict on EVERY tensor.  Returns (blocks, most perturbation tries a block needed, worst strict error)."""
    lines = [l.split() for l in arch.splitlines() if l.startswith("TDS")]
    blocks = [(rec, da) for rec, da in reversed(ref.upstream) if rec[0] == "TDS"]     # network order
    assert len(blocks) == len(lines) > 0
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(1000 + seed)
    worst, most_tries = 0.0, 0
    for (rec, da), tok in zip(blocks, lines):
        _, p, saved0, pl, pr, mode, pi = rec
        xin0 = np.ascontiguousarray(saved0["x"], dtype=np.float32)                      # [B][c][h][T]
        B, c, h, T = xin0.shape
        assert (c, h) == (int(tok[1]), int(tok[3]))
        l = c * h
        xin, out, saved, tries, margin = kink_free_block_input(xin0, p, pl, pr, mode, rng)
        assert margin >= KINK_MARGIN, (pi, tok, "no kink-free input found", margin)
        most_tries = max(most_tries, tries)
        da = np.ascontiguousarray(da, dtype=np.float32)
        _, gg = refnet.tds_bwd(da, p, saved, pl, pr, mode)
        want_grads = [gg["wc"], gg["bc"], np.array([gg["g1"], gg["b1n"]], np.float32), gg["w1"], gg["b1"], gg["w2"], gg["b2"],
                      np.array([gg["g2"], gg["b2n"]], np.float32)]
        one = ("V -1 %d %d 0\nRO 0 2 1 3\n%s\nRO 2 1 0 3\nV %d -1 1 0\nV %d 0 -1 1\n" % (c, h, " ".join(tok[:4] + ["0.0"] + tok[5:]), l, l))
        tr = Trainer(one, l, l, "ctc", 4, 0.0)
        table = tr.param_table()
        assert len(table) == 8
        for i, q in enumerate(params[pi - 8:pi]):
            tr.import_param(i, q)
        tr.plan(B, T, 1)
        tr.to_device()
        to_em = lambda a: np.ascontiguousarray(a.transpose(0, 3, 2, 1)).reshape(B, T, l)   # [B][c][h][T] -> [B][T][h * C + c]
        feed = np.ascontiguousarray(xin.transpose(0, 2, 1, 3)).reshape(B, l, T)            # [B][h * C + c][T]
        em = tr.forward(torch.tensor(feed).cuda(), train=True).cpu().numpy()
        e = rel(em, to_em(out))
        assert e < TOL, (pi, tok, "output", e)
        worst = max(worst, e)
        tr.backward(torch.tensor(to_em(da)).cuda())
        g = tr.grads.cpu().numpy()
        for i in range(8):
            want = np.asarray(want_grads[i], np.float64).reshape(-1)
            got = np.asarray(tr.export_from(i, g), np.float64).reshape(-1)
            err = rel(got, want)
            assert err < (TOL if want.size > 2 else 1e-3), (pi, tok, table[i][0], err, "kink margin %.1e after %d tries" % (margin, tries))
            if want.size > 2:
                worst = max(worst, err)
        del tr
    return len(blocks), most_tries, worst


def teacher_forced_tr_blocks(ref, arch, params, ref_grads):
    """the same for every Transformer block of config 5 against the float64 (unrounded) oracle block: output at 1e-2 of the
    largest magnitude, parameter gradients by direction and size at the one-block bars (cosine > 0.995, relative L2 < 8 %;
    tests/test_gpu_trainer.py::test_transformer_block_at_config5_width_bf16), the attention's q / k path on the scale of the
    block's wv.w gradient (5e-3; see the full-network test), LayerNorm pairs 0.2"""
    tok = [l.split() for l in arch.splitlines() if l.startswith("TR")]
    blocks = [(rec, da) for rec, da in reversed(ref.upstream) if rec[0] == "TR"]
    assert len(blocks) == len(tok) > 0
    qk_path = {"tr.posemb", "tr.wq.w", "tr.wq.b", "tr.wk.w", "tr.wk.b"}
    worst = {}
    for (rec, da), t in zip(blocks, tok):
        _, xt, pt, yt, pi = rec
        xin = xt.detach().numpy().astype(np.float32)                                    # [B][T][C]
        B, T, Cc = xin.shape
        n = len(pt)
        one = "V -1 1 NFEAT 0\nRO 2 0 3 1\n%s\n" % " ".join(t[:5] + ["0.0", "0.0"])
        tr, table = _one_block_trainer(one, Cc, Cc, B, T, params[pi - n:pi])
        em = tr.forward(torch.tensor(np.ascontiguousarray(xin.transpose(0, 2, 1))).cuda(), train=True).cpu().numpy()
        e = rel(em, yt.detach().numpy())
        assert e < 1e-2, (pi, "output", e)
        tr.backward(torch.tensor(np.ascontiguousarray(np.asarray(da, np.float32).reshape(B, T, Cc))).cuda())
        g = tr.grads.cpu().numpy()
        names = [table[i][0] for i in range(n)]
        scale = np.abs(np.asarray(ref_grads[pi - n + names.index("tr.wv.w")])).max()
        for i, name in enumerate(names):
            got = np.asarray(tr.export_from(i, g), np.float64).reshape(-1)
            w = np.asarray(ref_grads[pi - n + i], np.float64).reshape(-1)
            if name in qk_path:
                err = np.abs(got - w).max() / scale
                assert err < 5e-3, (pi, name, "block scale", err)
            elif w.size <= 2:
                err = np.abs(got - w).max() / max(1e-30, np.abs(w).max())
                assert err < 0.2, (pi, name, err)     # (gain, offset): two sums over every activation with heavy cancellation; measured 0.065
            else:
                l2 = np.linalg.norm(got - w) / max(1e-30, np.linalg.norm(w))
                cos = float(got @ w) / max(1e-30, np.linalg.norm(got) * np.linalg.norm(w))
                assert l2 < 0.08 and cos > 0.995, (pi, name, l2, cos)
                err = l2
            worst[name] = max(worst.get(name, 0.0), float(err))
        del tr
    return len(blocks), worst


def _transformer_ctc_arch_no_dropout():
    import re
    from wav2letter_amd import recipes
    arch = re.sub(r"^DO [0-9.]+$", "DO 0.0", recipes.transformer_ctc_arch(), flags=re.M)
    return re.sub(r"^(TR \d+ \d+ \d+ \d+) [0-9.]+ [0-9.]+$", r"\1 0.0 0.0", arch, flags=re.M)


def _config5_case(rng):
    nfeat, nlabel, B, T, L = 80, 9998, 2, 296, 6
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.full((B, L), -1, np.int32)
    tgt[0, :6] = [17, 4021, 9996, 3, 3, 77]
    tgt[1, :2] = [9000, 12]
    return nfeat, nlabel, B, T, L, x, tgt


def test_transformer_ctc_config5_full_network_end_to_end(oracle):
    """BASELINE config 5 in fp32 -- the full sota/2019 Transformer-CTC recipe network (am_transformer_ctc.arch: three WN-conv +
    GLU + max-pool stages, 24 `TR 1024 4096 4 460` blocks, Linear to 9998 word pieces; 323 M parameters with the position
    tables) -- at a reduced batch and number of frames (T = 296 -> 37 frames in the blocks), dropout and layer drop off:
    emissions, CTC loss and every parameter gradient against the reference-layout interpreter (oracle/refnet.py with the
    float64 Transformer block of oracle/transformer_oracle.py) + the CTC oracle.  24 ReLU MLPs deep: the gradient bar is the
    deep-network one (direction and size of every tensor; the strict bar where no kink lies between tensor and loss), as
    for configs 2 and 3."""
    rng = np.random.default_rng(51)
    nfeat, nlabel, B, T, L, x, tgt = _config5_case(rng)
    arch = _transformer_ctc_arch_no_dropout()
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    assert em.shape == em_ref.shape == (B, 37, nlabel)
    assert rel(em, em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < TOL
    want = ref.backward(o.backward().astype(np.float32), len(params))
    g = tr.grads.cpu().numpy()
    table = tr.param_table()
    # The attention's q / k path at initialisation: the frames a block sees are nearly alike, so dP = dctx . v is almost constant
    # along the keys and the softmax backward removes that common mode -- the oracle's q / k / position-table gradients are 1e-5
    # of the block's other gradients (wq.b 2e-5, wk.w 3e-5 against wv.w 6.5), wk.b exactly zero (float64 leaves 1e-17).  In fp32
    # the cancellation leaves rounding of the size of the operands, not of the result: those five tensors are held at the 1e-4
    # bar on the scale of the BLOCK's gradients (its wv.w), every other tensor on its own scale.
    qk_path = {"tr.posemb", "tr.wq.w", "tr.wq.b", "tr.wk.w", "tr.wk.b"}
    n_strict = n_own_scale = 0
    fails = []
    for i, (name, _n, _off) in enumerate(table):
        got = np.asarray(tr.export_from(i, g), np.float64).reshape(-1)
        w = np.asarray(want[i], np.float64).reshape(-1)
        l2 = np.linalg.norm(got - w) / max(1e-30, np.linalg.norm(w))
        cos = float(got @ w) / max(1e-30, np.linalg.norm(got) * np.linalg.norm(w))
        if name in qk_path:
            j = i
            while table[j][0] != "tr.wv.w":
                j += 1
            assert j - i <= 9
            err = np.abs(got - w).max() / np.abs(np.asarray(want[j])).max()
            if not err < TOL:
                fails.append((i, name, "block scale", err, l2, cos))
            n_own_scale += name != "tr.wk.b" and l2 < 0.1 and cos > 0.99
            continue
        if not (l2 < 0.1 and cos > 0.99):
            fails.append((i, name, l2, cos))
        n_strict += rel(got, w) < 2 * TOL
    assert not fails, (len(fails), fails[:12])
    n_rest = len(table) - 5 * 24
    assert n_strict >= n_rest // 2, (n_strict, n_rest)   # most tensors sit at the strict bar; the rest carry a flipped kink
    print("config 5 fp32: %d of %d tensors at the strict bar; q / k path: %d of 96 within 10 %% on their own scale" % (n_strict, n_rest, n_own_scale))


def test_transformer_ctc_config5_full_network_bf16(oracle):
    """the same network in the mixed-precision mode (BASELINE config 5's dtype) against the UNROUNDED float64 restatement at the
    stated bf16 bars: emissions / loss 2e-2 of the largest magnitude (24 blocks of bf16 products), parameter gradients by
    direction and size (cosine > 0.97, relative L2 < 25 %; a deep bf16 network agrees with any second implementation only
    statistically -- tests/test_gpu_trainer.py::test_streaming_tds_config3_bf16_against_bf16_operand_oracle); the exactness of
    the bf16 products is held per operator and by the one-block test above"""
    rng = np.random.default_rng(51)
    nfeat, nlabel, B, T, L, x, tgt = _config5_case(rng)
    arch = _transformer_ctc_arch_no_dropout()
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    tr.set_mixed_precision(True)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    assert rel(em, em_ref) < 2e-2
    assert rel(em, em_ref) > 1e-6          # the bf16 path really ran
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < 2e-2
    ref.upstream = []
    want = ref.backward(o.backward().astype(np.float32), len(params))
    g = tr.grads.cpu().numpy()
    # the attention's q / k path (see the fp32 test above: its gradients are 1e-5 .. 1e-6 of the block's at initialisation, the rest
    # cancels): with bf16 operands the cancellation leaves bf16 rounding of the COMMON-MODE operands -- up to 750 x the tensor's own
    # size in the last block, identically with the fused attention backward and with the unfused launch sequence
    # (profiles/r04_run19_c5_qk_noise.log) -- so those tensors are held on the scale of the block's gradients (its wv.w) at 5e-3
    # (measured 4e-4), every other tensor on its own scale
    qk_path = {"tr.posemb", "tr.wq.w", "tr.wq.b", "tr.wk.w", "tr.wk.b"}
    table = tr.param_table()
    fails = []
    worst = {}
    for i, (name, _n, _off) in enumerate(table):
        got = np.asarray(tr.export_from(i, g), np.float64).reshape(-1)
        w = np.asarray(want[i], np.float64).reshape(-1)
        assert np.isfinite(got).all()
        if w.size <= 2:
            continue   # LayerNorm (gain, offset): two sums over every activation with heavy cancellation
        if name in qk_path:
            j = i
            while table[j][0] != "tr.wv.w":
                j += 1
            err = np.abs(got - w).max() / np.abs(np.asarray(want[j])).max()
            if not err < 5e-3:
                fails.append((i, name, "block scale", err))
            if err > worst.get(name, (0, 0))[0]:
                worst[name] = (err, 0.0)
            continue
        l2 = np.linalg.norm(got - w) / max(1e-30, np.linalg.norm(w))
        cos = float(got @ w) / max(1e-30, np.linalg.norm(got) * np.linalg.norm(w))
        lim = (0.25, 0.97) if w.size > 1000 else (0.35, 0.95)   # measured: 0.13 / 0.9915 (profiles/r04_run19_c5_qk_noise.log)
        if not (l2 < lim[0] and cos > lim[1]):
            fails.append((i, name, l2, cos))
        if l2 > worst.get(name, (0, 0))[0]:
            worst[name] = (l2, cos)
    print("config 5 bf16, worst relative L2 / cosine per tensor kind (q / k path: error on the block's scale):",
          {k: (float("%.3g" % v[0]), round(v[1], 4)) for k, v in worst.items()})
    assert not fails, (len(fails), fails[:12])
    # teacher-forced: every block alone on the oracle's activation and upstream gradient (round-3 verdict item 9)
    del tr
    nblk, worst_tf = teacher_forced_tr_blocks(ref, arch, params, want)
    assert nblk == 24
    print("config 5 bf16, teacher-forced blocks: worst per tensor kind", {k: float("%.3g" % v) for k, v in worst_tf.items()})


def test_transformer_padding_mask_from_input_sizes(oracle):
    """a ragged batch: the trainer is given the utterances' input sizes and every Transformer block masks the padded keys
    (forwardSequentialModuleWithPadMask, cpc/SequentialBuilder.cpp:58-81; TransformerCPC.cpp:138-144) -- emissions, CTC loss
    and every parameter gradient against the oracle with the same mask; without sizes the mask is off again"""
    rng = np.random.default_rng(3)
    nfeat, nlabel, B, T, L = 16, 12, 4, 37, 3
    arch = ("V -1 1 NFEAT 0\nWN 3 C NFEAT 64 3 1 -1\nGLU 2\nDO 0.0\nM 1 1 2 1\nRO 2 0 3 1\n"
            "TR 32 64 4 9 0.0 0.0\nTR 32 64 4 9 0.0 0.0\nL 32 NLABEL\n")
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    sizes = np.array([5920.0, 3100.0, 5000.0, 1700.0], np.float32)       # samples; the longest fills the batch
    em_full = ref.forward(x, params)
    tr.set_input_sizes(torch.tensor(sizes).cuda())
    ref.input_sizes = sizes
    em_ref = ref.forward(x, params)
    assert rel(em_ref, em_full) > 1e-2                                     # the mask matters on this batch
    assert rel(tr.forward(xd, train=False).cpu().numpy(), em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < TOL
    want = ref.backward(o.backward().astype(np.float32), len(params))
    g = tr.grads.cpu().numpy()
    for i, (name, _n, _off) in enumerate(tr.param_table()):
        if name == "tr.wk.b":
            assert np.abs(tr.export_from(i, g)).max() < 1e-5 * np.abs(want[i - 2]).max()
            want[i] = None
    check_grads(tr, want)
    tr.set_input_sizes(None)
    assert rel(tr.forward(xd, train=False).cpu().numpy(), em_full) < TOL


def test_transformer_training_mode_attention_dropout_and_layer_drop(oracle):
    """training mode of a TR block: (a) dropout 0.3 on the attention probabilities -- the mask is the library's stateless
    integer hash (oracle/nn_oracle.c holds the same function), so the oracle applies the IDENTICAL mask and loss and
    gradients are held to the usual tolerance; (b) layer drop with probability 1: both sublayers vanish, h = LN1(x),
    out = LN2(h), their parameters receive exactly zero gradient (TransformerCPC.cpp:170-181)"""
    nfeat, nlabel, B, T, L, H = 32, 9, 2, 19, 3, 4
    for p, pld in ((0.3, 0.0), (0.0, 1.0)):
        rng = np.random.default_rng(5)
        arch = f"V -1 1 NFEAT 0\nRO 2 0 3 1\nTR 32 48 {H} 6 {p} {pld}\nL 32 NLABEL\n"
        tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
        x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
        tgt = rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)
        xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
        td = torch.tensor(tgt).cuda()
        step = 7
        tr.set_step(step)
        loss = tr.forward_backward(xd, td).cpu().numpy()
        if p > 0:
            seed = (0x9E3779B9 * (step + 1)) & 0xFFFFFFFF          # host/trainer.cpp: the step's dropout seed
            stream = 1 + 4 * 2                                     # layer 2 of the Sequential (V, RO, TR, L)
            mask = oracle.dropout(np.ones(B * H * T * T, np.float32), p, seed, stream).reshape(B, H, T, T)
            assert 0.2 < (mask == 0).mean() < 0.4
            ref.tr_opts = [{"attn_mask": mask}]
        else:
            ref.tr_opts = [{"f": 0.0}]
        em_ref = ref.forward(x, params)
        o = oracle.CTC(em_ref, tgt, scale_mode=4)
        assert rel(loss, o.forward()) < TOL, (p, pld)
        want = ref.backward(o.backward().astype(np.float32), len(params))
        g = tr.grads.cpu().numpy()
        table = tr.param_table()
        for i, (name, _n, _off) in enumerate(table):
            zero = name == "tr.wk.b" or (pld > 0 and name.startswith("tr.") and "norm" not in name)
            if zero:
                assert np.abs(want[i]).max() < 1e-9 and np.abs(tr.export_from(i, g)).max() < (1e-6 if pld == 0 else 1e-30), (i, name)
                want[i] = None
            if pld > 0 and name == "tr.norm1.weight+bias":
                # LN2(gamma1 * xhat + beta1) does not depend on gamma1 / beta1 (up to eps): a near-zero gradient on both
                # sides, compared on the scale of norm2's
                n2 = np.abs(want[i + 1]).max()
                assert np.abs(want[i]).max() < 1e-3 * n2 and np.abs(tr.export_from(i, g) - want[i]).max() < 1e-4 * n2, (i, name)
                want[i] = None
        check_grads(tr, want)
        # evaluation mode ignores both
        ref.tr_opts = None
        em_eval = refnet.RefNet(arch.replace(f"{p} {pld}", "0.0 0.0"), nfeat, nlabel).forward(x, params)
        assert rel(tr.forward(xd, train=False).cpu().numpy(), em_eval) < TOL


def test_conv_glu_librispeech_config4_full_network_end_to_end(oracle):
    """BASELINE config 4 -- the full conv_glu LibriSpeech recipe network (17 WN-conv + GLU layers, 208.9 M parameters,
    first layer padded by 170 frames, kernels 13..29), ASG criterion -- at a reduced batch and number of frames, dropout
    off: emissions, ASG loss, weight-norm v / g / bias gradients of every layer and the transition gradient against the
    numpy reference network + criterion oracle.  Every convolution runs as an overlapping-row LDS-DMA GEMM here."""
    import re
    from wav2letter_amd import recipes
    rng = np.random.default_rng(44)
    nfeat, nlabel, B, T, L = 40, 30, 2, 24, 6
    arch = re.sub(r"^DO [0-9.]+$", "DO 0.0", recipes.conv_glu_librispeech_arch(), flags=re.M)
    tr, ref, params, A = build(arch, nfeat, nlabel, "asg", 4, 4.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.full((B, L), -1, np.int32)
    tgt[0, :6] = [3, 7, 1, 28, 4, 9]
    tgt[1, :3] = [11, 0, 27]
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    assert em.shape == em_ref.shape == (B, T, nlabel)
    assert rel(em, em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    ol, odx, odA = oracle.asg(em_ref, A, tgt, 4)
    assert rel(loss, ol) < TOL
    check_grads(tr, ref.backward(odx.astype(np.float32), len(params)))
    gA = tr.grads.cpu().numpy()[tr.n_net:tr.n_net + nlabel * nlabel]
    assert rel(gA, odA) < TOL


def test_conv_glu_wsj_config1_end_to_end(oracle):
    """BASELINE config 1 -- the conv_glu WSJ recipe (15 WN-conv + GLU layers, SAME padding, even kernels, 17.1 M
    parameters), ASG criterion, 2-utterance batch -- at a reduced number of frames: emissions, ASG loss, every
    parameter gradient and the transition gradient against the reference network (numpy) + the criterion oracle.
    Evaluation mode of dropout (p = 0.25 in the recipe) so that both sides see the same activations."""
    from wav2letter_amd import recipes
    rng = np.random.default_rng(7)
    nfeat, nlabel, B, T, L = 40, 30, 2, 72, 9
    arch = recipes.conv_glu_wsj_arch().replace("DO 0.25", "DO 0.0")
    tr, ref, params, A = build(arch, nfeat, nlabel, "asg", 4, 4.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.full((B, L), -1, np.int32)
    tgt[0, :9] = [3, 7, 1, 28, 4, 9, 9 + 1, 2, 5]
    tgt[1, :5] = [11, 0, 27, 6, 13]
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    assert em.shape == em_ref.shape, (em.shape, em_ref.shape)
    assert rel(em, em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    ol, odx, odA = oracle.asg(em_ref, A, tgt, 4)
    assert rel(loss, ol) < TOL
    check_grads(tr, ref.backward(odx.astype(np.float32), len(params)))
    gA = tr.grads.cpu().numpy()[tr.n_net:tr.n_net + nlabel * nlabel]
    assert rel(gA, odA) < TOL


def test_linseg_warmup_then_asg(oracle):
    """--linseg=1 (every ASG recipe): update 0 runs LinSegCriterion on the ASG transitions, update 1 onwards ASG;
    both through the C++ trainer, against the oracle on the reference network's emissions"""
    from wav2letter_amd import recipes
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(11)
    nfeat, nlabel, B, T, L = 6, 9, 2, 40, 7
    arch = recipes.conv_glu_small_arch(widths=(16, 24), kws=(5, 4), pad0=2)
    tr, ref, params, A = build(arch, nfeat, nlabel, "asg", 4, 4.0, rng, B, T, L, linseg=1)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.array([[1, 2, 3, 1, -1, -1, -1], [0, 5, 5, 2, 7, 1, 0]], np.int32)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em_ref = ref.forward(x, params)
    loss = tr.forward_backward(xd, td).cpu().numpy()
    ol, odx, odA = oracle.linseg(em_ref, A, tgt, 4)
    assert rel(loss, ol) < TOL
    check_grads(tr, ref.backward(odx.astype(np.float32), len(params)))
    gA = tr.grads.cpu().numpy()[tr.n_net:tr.n_net + nlabel * nlabel]
    assert rel(gA, odA) < TOL
    tr.set_step(1)                       # past the warm-up: the ASG criterion proper
    loss = tr.forward_backward(xd, td).cpu().numpy()
    ol, odx, odA = oracle.asg(em_ref, A, tgt, 4)
    assert rel(loss, ol) < TOL
    gA = tr.grads.cpu().numpy()[tr.n_net:tr.n_net + nlabel * nlabel]
    assert rel(gA, odA) < TOL
    with pytest.raises(Exception):       # "linseg may only be used with ASG criterion" (Train.cpp:593)
        Trainer(recipes.tds_ctc_small_arch(c=(4,), h=8, kw=5), 8, 12, "ctc", 4).set_linseg(1)


def test_non_finite_gradient_skips_the_update():
    """a NaN anywhere in the (reduced) gradient arena: parameters and momentum stay untouched, the reported norm is
    non-finite; the next clean step updates again (reference: NaN guards of Train.cpp:1651-1660, :1686-1698)"""
    import math
    from wav2letter_amd import recipes
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(9)
    nfeat, nlabel, B, T, L = 8, 12, 2, 48, 4
    tr = Trainer(recipes.tds_ctc_small_arch(c=(4,), h=nfeat, kw=5), nfeat, nlabel, "ctc", 4)
    tr.init_params(3)
    tr.plan(B, T, L)
    tr.to_device()
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    tr.forward_backward(x, tgt)
    tr.update(lr=0.1, momentum=0.5, max_grad_norm=1.0, total_batch=B)
    assert math.isfinite(tr.grad_norm()) and tr.grad_norm() > 0
    p0, m0 = tr.params.clone(), tr.mom.clone()
    tr.forward_backward(x, tgt)
    tr.grads[tr.grads.numel() // 2] = float("nan")
    tr.update(lr=0.1, momentum=0.5, max_grad_norm=1.0, total_batch=B)
    assert not math.isfinite(tr.grad_norm())
    assert torch.equal(tr.params, p0) and torch.equal(tr.mom, m0)
    tr.forward_backward(x, tgt)
    tr.update(lr=0.1, momentum=0.5, max_grad_norm=1.0, total_batch=B)
    assert math.isfinite(tr.grad_norm()) and not torch.equal(tr.params, p0)


@pytest.mark.parametrize("crit,clamp_crit", [("ctc", True), ("asg", False)])
def test_non_finite_guard_without_clipping(crit, clamp_crit):
    """--maxgradnorm=0 (the reference default) and clampCrit = 0: the guard must still hold -- a NaN in the network OR in
    the criterion gradients leaves parameters and momentum of BOTH untouched, the skipped-update counter ticks, the
    next clean update goes through (round-1 advisor finding, trainer.cpp:205)"""
    import math
    from wav2letter_amd import recipes
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(10)
    nfeat, nlabel, B, T, L = 8, 12, 2, 48, 4
    tr = Trainer(recipes.tds_ctc_small_arch(c=(4,), h=nfeat, kw=5), nfeat, nlabel, crit, 4, 1.0)
    tr.init_params(3)
    tr.plan(B, T, L)
    tr.to_device()
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    kw = dict(lr=0.1, lrcrit=0.01, momentum=0.5, max_grad_norm=0.0, total_batch=B, clamp_crit=clamp_crit)
    tr.forward_backward(x, tgt)
    tr.update(**kw)
    assert math.isfinite(tr.grad_norm()) and tr.grad_norm() > 0 and tr.skipped_updates() == 0
    bad = [tr.n_net // 2] + ([tr.n_net + 5] if crit == "asg" else [])
    for k, where in enumerate(bad):
        p0, m0 = tr.params.clone(), tr.mom.clone()
        tr.forward_backward(x, tgt)
        tr.grads[where] = float("inf") if k else float("nan")
        tr.update(**kw)
        assert not math.isfinite(tr.grad_norm())
        assert torch.equal(tr.params, p0) and torch.equal(tr.mom, m0)
        assert tr.skipped_updates() == k + 1
    tr.forward_backward(x, tgt)
    tr.update(**kw)
    assert math.isfinite(tr.grad_norm()) and not torch.equal(tr.params, p0)
    assert tr.skipped_updates() == len(bad)


def test_unclipped_update_is_plain_sgd_and_batch_size_rides_the_arena():
    """max_grad_norm = 0: p -= lr * (mom*v + g / total_batch) exactly; total_batch = "reduced" takes 1 / (the batch
    size in the gradient arena's tail) -- written by forward_backward, summed by the gradient all-reduce"""
    from wav2letter_amd import recipes
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(11)
    nfeat, nlabel, B, T, L = 8, 12, 3, 40, 4
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    outs = []
    for tb in (B, "reduced"):
        tr = Trainer(recipes.tds_ctc_small_arch(c=(4,), h=nfeat, kw=5), nfeat, nlabel, "ctc", 4)
        tr.init_params(3)
        tr.plan(B, T, L)
        tr.to_device()
        p0 = tr.params.clone()
        tr.forward_backward(x, tgt)
        assert tr.grads_full[tr.n_floats].item() == B and (tr.grads_full[tr.n_floats + 1:] == 0).all()
        g = tr.grads.clone()
        tr.update(lr=0.1, momentum=0.0, max_grad_norm=0.0, total_batch=tb)
        want = p0.double() - 0.1 * g.double() / B
        assert (tr.params.double() - want).abs().max().item() < 1e-6 * max(1.0, want.abs().max().item())
        outs.append(tr.params.clone())
    assert torch.equal(outs[0], outs[1])
    # a world of 2 identical ranks: gradients and the batch slot both double, the update is unchanged
    tr.params.copy_(p0)
    tr.forward_backward(x, tgt)
    tr.grads_full.mul_(2.0)
    tr.update(lr=0.1, momentum=0.0, max_grad_norm=0.0, total_batch="reduced")
    assert (tr.params - outs[0]).abs().max().item() < 1e-6


def test_adagrad_updates_follow_the_recurrence():
    """--netoptim=adagrad --critoptim=adagrad (the Transformer-CTC recipe): three updates of an ASG network against the fp64
    recurrence  g' = clip(g / B),  var += g'^2,  p -= lr g' / (sqrt(var) + 1e-8)  on network and transition parameters (each
    with its own learning rate, one global clip coefficient); a non-finite gradient leaves parameters AND sums untouched"""
    from wav2letter_amd import recipes
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(21)
    nfeat, nlabel, B, T, L = 8, 7, 3, 30, 4
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel, size=(B, L)).astype(np.int32)).cuda()
    tr = Trainer(recipes.conv_glu_small_arch(), nfeat, nlabel, "asg", 4, 1.0)
    tr.init_params(5)
    tr.plan(B, T, L)
    tr.to_device()
    tr.set_optimizer("adagrad", "adagrad")
    n_net = tr.n_net
    p = tr.params.double().clone()
    var = torch.zeros_like(p)
    lr, lrcrit, clip = 0.02, 0.005, 0.05
    for it in range(3):
        tr.forward_backward(x, tgt)
        g = tr.grads.double().clone() / B
        c = min(1.0, clip / (g.norm().item() + 1e-6))
        assert it > 0 or c < 1.0                       # the clip is live on the first update
        g = g * c
        var += g * g
        step = g / (var.sqrt() + 1e-8)
        p[:n_net] -= lr * step[:n_net]
        p[n_net:] -= lrcrit * step[n_net:]
        tr.update(lr=lr, lrcrit=lrcrit, momentum=0.0, max_grad_norm=clip, total_batch=B)
        assert (tr.params.double() - p).abs().max().item() < 2e-6 * max(1.0, p.abs().max().item()), it
    assert (tr.mom.double() - var).abs().max().item() < 1e-6 * var.abs().max().item()
    before, vbefore = tr.params.clone(), tr.mom.clone()
    tr.forward_backward(x, tgt)
    tr.grads[5] = float("nan")
    tr.update(lr=lr, lrcrit=lrcrit, momentum=0.0, max_grad_norm=clip, total_batch=B)
    assert torch.equal(tr.params, before) and torch.equal(tr.mom, vbefore) and tr.skipped_updates() == 1


def test_adadelta_updates_follow_the_recurrence():
    """--netoptim=adadelta --critoptim=adadelta --lr=0.4 (the LibriSpeech Transformer-CTC recipe): four updates against the fp64
    recurrence of fl::AdadeltaOptimizer (rho 0.9, eps 1e-8) on both parameter groups; without the second state arena the
    update is refused"""
    from wav2letter_amd import recipes
    from wav2letter_amd._lib import W2LInvalidArgument
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(22)
    nfeat, nlabel, B, T, L = 8, 7, 3, 30, 4
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel, size=(B, L)).astype(np.int32)).cuda()
    tr = Trainer(recipes.conv_glu_small_arch(), nfeat, nlabel, "asg", 4, 1.0)
    tr.init_params(5)
    tr.plan(B, T, L)
    tr.to_device()
    tr.set_optimizer("adadelta", "adadelta")
    n_net = tr.n_net
    p = tr.params.double().clone()
    ag, ad = torch.zeros_like(p), torch.zeros_like(p)
    lr, lrcrit, clip, rho, eps = 0.4, 0.1, 0.05, 0.9, 1e-8
    for it in range(4):
        tr.forward_backward(x, tgt)
        g = tr.grads.double().clone() / B
        g = g * min(1.0, clip / (g.norm().item() + 1e-6))
        ag = rho * ag + (1 - rho) * g * g
        delta = (ad + eps).sqrt() / (ag + eps).sqrt() * g
        p[:n_net] -= lr * delta[:n_net]
        p[n_net:] -= lrcrit * delta[n_net:]
        ad = rho * ad + (1 - rho) * delta * delta
        tr.update(lr=lr, lrcrit=lrcrit, momentum=0.0, max_grad_norm=clip, total_batch=B)
        assert (tr.params.double() - p).abs().max().item() < 5e-6 * max(1.0, p.abs().max().item()), it
    assert (tr.mom.double() - ag).abs().max().item() < 1e-5 * ag.abs().max().item()
    assert (tr.state2.double() - ad).abs().max().item() < 1e-4 * ad.abs().max().item()
    tr2 = Trainer(recipes.conv_glu_small_arch(), nfeat, nlabel, "asg", 4, 1.0)
    tr2.init_params(5)
    tr2.plan(B, T, L)
    tr2.to_device()
    tr2.L.w2l_trainer_set_optimizer(tr2.h, 2, 2)      # behind the wrapper's back: no second arena bound
    tr2.forward_backward(x, tgt)
    with pytest.raises(W2LInvalidArgument):
        tr2.update(lr=lr, lrcrit=lrcrit, total_batch=B)


@pytest.mark.parametrize("kind", ["adagrad", "adadelta"])
def test_optimizer_kernels_against_torch_optim(kind):
    """w2l_adagrad_step_guarded / w2l_adadelta_step_guarded (no clip, no guard) against torch.optim's Adagrad (eps 1e-8) and
    Adadelta (rho 0.9, eps 1e-8) -- a second implementation of the recurrences fl::AdagradOptimizer / fl::AdadeltaOptimizer
    restate -- over five steps on an odd-length vector (float4 body + scalar tail)"""
    from wav2letter_amd import _lib
    L = _lib.lib()
    n = 4099
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (0.1 + i) for i in range(5)]
    ref = p0.double().clone().requires_grad_(True)
    opt = (torch.optim.Adagrad([ref], lr=0.02, eps=1e-8) if kind == "adagrad"
           else torch.optim.Adadelta([ref], lr=0.4, rho=0.9, eps=1e-8))
    p = p0.cuda().clone()
    s1, s2 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for gi in grads:
        ref.grad = gi.double().clone()
        opt.step()
        gd = gi.cuda()
        if kind == "adagrad":
            assert L.w2l_adagrad_step_guarded(p.data_ptr(), gd.data_ptr(), s1.data_ptr(), n, 0.02, 1e-8, 1.0, 0.0, None, st) == 0
        else:
            assert L.w2l_adadelta_step_guarded(p.data_ptr(), gd.data_ptr(), s1.data_ptr(), s2.data_ptr(), n, 0.4, 0.9, 1e-8, 1.0, 0.0, None, st) == 0
        assert (p.cpu().double() - ref.detach()).abs().max().item() < 1e-5


def test_batch_larger_than_64_and_unbound_calls():
    """B > 64 (round-1 limit of the loss slots) and the ABI's bound-state checks"""
    from wav2letter_amd import _lib, recipes
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(12)
    nfeat, nlabel, B, T, L = 8, 12, 70, 32, 4
    arch = recipes.tds_ctc_small_arch(c=(4,), h=nfeat, kw=5)
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    tr = Trainer(arch, nfeat, nlabel, "ctc", 4)
    tr.init_params(3)
    tr.plan(B, T, L)
    tr.to_device()
    loss = tr.forward_backward(x, tgt)
    assert loss.shape == (B,) and torch.isfinite(loss).all()
    # the same utterances in two half batches give the same losses and the same summed gradient
    g = tr.grads.clone()
    h = Trainer(arch, nfeat, nlabel, "ctc", 4)
    h.init_params(3)
    h.plan(B // 2, T, L)
    h.to_device()
    l0 = h.forward_backward(x[:B // 2].contiguous(), tgt[:B // 2].contiguous()).clone()
    g0 = h.grads.clone()
    l1 = h.forward_backward(x[B // 2:].contiguous(), tgt[B // 2:].contiguous()).clone()
    assert (torch.cat([l0, l1]) - loss).abs().max().item() < 1e-4 * loss.abs().max().item()
    assert (g0 + h.grads - g).abs().max().item() < 1e-4 * g.abs().max().item()
    with pytest.raises(_lib.W2LInvalidArgument):
        tr.forward_backward(x[:, :, :T - 1], tgt)            # wrong shape
    with pytest.raises(_lib.W2LInvalidArgument):
        tr.forward_backward(x, tgt.long())                   # wrong dtype
    u = Trainer(arch, nfeat, nlabel, "ctc", 4)               # never planned / bound
    assert u.L.w2l_trainer_update(u.h, 0.1, 0.0, 0.0, 0.0, 1.0, 1, None) == _lib.W2L_EINVAL
    assert u.L.w2l_trainer_forward_backward(u.h, x.data_ptr(), tgt.data_ptr(), None, None) == _lib.W2L_EINVAL


def test_training_reduces_loss():
    """a few SGD steps on a fixed batch must drive the CTC loss down (plumbing sanity)"""
    from wav2letter_amd import recipes
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(2)
    nfeat, nlabel, B, T, L = 8, 12, 4, 48, 5
    tr = Trainer(recipes.tds_ctc_small_arch(c=(4,), h=nfeat, kw=5, drop=0.1), nfeat, nlabel, "ctc", 4)
    tr.init_params(3)
    tr.plan(B, T, L)
    tr.to_device()
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    losses = []
    for _ in range(30):
        losses.append(tr.forward_backward(x, tgt).sum().item())
        tr.update(lr=0.05, momentum=0.5, max_grad_norm=1.0)
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.7 * losses[0], losses


def test_gradient_bucket_events_and_single_rank_rccl():
    """the data-parallel overlap path on one GPU: bucket events recorded during backward gate a side stream,
    a 1-rank RCCL ("nccl") process group runs the bucketed all-reduce, gradients and the update are
    unchanged against the plain step"""
    import os
    import socket
    import torch.distributed as dist
    from wav2letter_amd import recipes
    from wav2letter_amd.parallel import OverlappedReducer
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(5)
    nfeat, nlabel, B, T, L = 8, 12, 4, 48, 5
    arch = recipes.tds_ctc_small_arch(c=(4, 6), h=nfeat, kw=5)

    def make():
        tr = Trainer(arch, nfeat, nlabel, "ctc", 4)
        tr.init_params(3)
        tr.plan(B, T, L)
        tr.to_device()
        return tr
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    ref = make()
    ref.forward_backward(x, tgt)
    g_ref = ref.grads.clone()
    ref.update(lr=0.1, momentum=0.5, max_grad_norm=1.0)

    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        tr = make()
        red = OverlappedReducer(tr, n_buckets=3)
        assert red.offsets[0] == 0 and red.offsets[-1] == tr.n_floats + 4 and len(red.offsets) >= 3
        for _ in range(2):  # events are re-recorded every step
            tr.set_step(0)
            tr.grads.zero_()
            tr.forward_backward(x, tgt)
            red.reduce()
            torch.cuda.synchronize()
            assert torch.equal(tr.grads, g_ref)
        tr.update(lr=0.1, momentum=0.5, max_grad_norm=1.0)
        assert torch.equal(tr.params, ref.params)
        with pytest.raises(Exception):
            tr.wait_bucket(99, red.comm)
        # bf16 buckets (mixed-precision mode): one rank's "sum" is its own gradients rounded to bf16; the batch-size tail
        # goes through its own fp32 collective and stays exact
        tb = make()
        rb = OverlappedReducer(tb, n_buckets=3, bf16=True)
        tb.forward_backward(x, tgt)
        rb.reduce()
        torch.cuda.synchronize()
        assert torch.equal(tb.grads, g_ref.bfloat16().float())
        assert tb.grads_full[tb.n_floats].item() == float(B)
        assert sum(rb.bucket_bytes()) == 2 * tb.n_floats + 16
        tr.set_grad_buckets([])  # hooks off again
        tr.forward_backward(x, tgt)
    finally:
        dist.destroy_process_group()


def test_checkpoint_resume_reproduces_the_next_step(tmp_path):
    """save (params + momentum + step) after two SGD steps, load into a fresh trainer: the third step is bit-identical"""
    from wav2letter_amd import checkpoint, recipes
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(8)
    nfeat, nlabel, B, T, L = 8, 12, 3, 40, 5
    arch = recipes.tds_ctc_small_arch(c=(4,), h=nfeat, kw=5, drop=0.1)

    def make(seed):
        tr = Trainer(arch, nfeat, nlabel, "ctc", 4)
        tr.init_params(seed)
        tr.plan(B, T, L)
        tr.to_device()
        return tr
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    a = make(1)
    for _ in range(2):
        a.forward_backward(x, tgt)
        a.update(lr=0.05, momentum=0.9, max_grad_norm=1.0)
    path = str(tmp_path / "ck.w2l")
    checkpoint.save(path, a, arch, "ctc", step=2)
    b = make(77)
    assert checkpoint.load(path, b, arch) == 2
    # the natural resume order -- load() BEFORE to_device() -- must restore the momentum too
    c = Trainer(arch, nfeat, nlabel, "ctc", 4)
    assert checkpoint.load(path, c, arch) == 2
    c.plan(B, T, L)
    c.to_device()
    assert torch.equal(c.mom, a.mom) and torch.equal(c.params, a.params)
    la = a.forward_backward(x, tgt).clone()
    a.update(lr=0.05, momentum=0.9, max_grad_norm=1.0)
    lb = b.forward_backward(x, tgt).clone()
    b.update(lr=0.05, momentum=0.9, max_grad_norm=1.0)
    assert torch.equal(la, lb)                  # same dropout masks: the step counter was restored
    assert torch.equal(a.params, b.params)      # same momentum


def test_checkpoint_resume_with_adadelta_state(tmp_path):
    """the Transformer-CTC recipe's optimizer has TWO state arenas (accGrad, accDelta): both travel in the checkpoint, a resume
    (load before to_device) reproduces the next update bit for bit, and loading into a trainer set up for another optimizer
    is refused (the arena would be misread as SGD velocity)"""
    from wav2letter_amd import checkpoint
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(9)
    nfeat, nlabel, B, T, L = 16, 10, 2, 24, 3
    arch = "V -1 1 NFEAT 0\nRO 2 0 3 1\nTR 16 32 2 7 0.1 0.0\nL 16 NLABEL\n"
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    a = Trainer(arch, nfeat, nlabel, "ctc", 4)
    a.init_params(1)
    a.plan(B, T, L)
    a.to_device()
    a.set_optimizer("adadelta", "adadelta")
    for _ in range(2):
        a.forward_backward(x, tgt)
        a.update(lr=0.4, max_grad_norm=1.0)
    path = str(tmp_path / "ck.w2l")
    checkpoint.save(path, a, arch, "ctc", step=2)
    hdr, _ = checkpoint.read(path)
    assert hdr["optim"] == ["adadelta", "adadelta"] and [t["kind"] for t in hdr["tensors"]][-2:] == ["momentum", "state2"]
    b = Trainer(arch, nfeat, nlabel, "ctc", 4)
    with pytest.raises(ValueError):
        checkpoint.load(path, b, arch)                 # still an SGD trainer
    b.set_optimizer("adadelta", "adadelta")
    assert checkpoint.load(path, b, arch) == 2
    b.plan(B, T, L)
    b.to_device()
    assert torch.equal(b.mom, a.mom) and torch.equal(b.state2, a.state2) and torch.equal(b.params, a.params)
    la = a.forward_backward(x, tgt).clone(); a.update(lr=0.4, max_grad_norm=1.0)
    lb = b.forward_backward(x, tgt).clone(); b.update(lr=0.4, max_grad_norm=1.0)
    assert torch.equal(la, lb) and torch.equal(a.params, b.params) and torch.equal(a.state2, b.state2)


def test_bench_refuses_more_ranks_than_gpus():
    """on a 1-GPU box `python bench.py --gpus 2` must fail loudly, not silently run one rank (round-1 verdict, missing 1)"""
    import os
    import subprocess
    import sys
    if torch.cuda.device_count() >= 2:
        pytest.skip("more than one GPU visible")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode != 0
    assert "needs 2 visible GPUs" in out.stderr
    assert not any(l.startswith("{") for l in out.stdout.splitlines())


def test_bench_plain_run_is_the_headline_only():
    """`python bench.py` without --full times the headline step and prints its line, and runs none of the legs that take
    runs of their own (those come with --full)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "1", "--warmup", "1", "--batch", "2",
                          "--frames", "800"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert (r["metric"], r["unit"], r["higher_is_better"], r["dtype"]) == ("utterances/sec", "utterances/sec", True, "f32")
    assert (r["steps"], r["warmup"], r["config"]["global_batch"]) == (1, 1, 2)
    assert r["value"] > 0 and r["ms_per_step"] > 0
    assert abs(r["value"] - 2 * 1e3 / r["ms_per_step"]) < 1e-2 * r["value"]
    legs = {"input_pipeline", "train_binary_config2", "asg_loss_ms_per_step", "ctc_loss_ms_per_step", "asg_stress",
            "conv_glu_asg_step", "streaming_tds_bf16_step", "transformer_ctc_step", "cpu_baseline"}
    assert not legs & set(r), sorted(legs & set(r))
    assert "] leg " not in out.stderr


def test_mixed_precision_streaming_tds_step(oracle):
    """BASELINE config 3 (streaming_convnets am_500ms_future_context.arch: asymmetric padding, per-frame LayerNorm, TDS
    blocks with 15 / 19 / 23 / 27 channels, 115.1 M parameters), reduced batch / frames, dropout and SpecAugment off:
    the bf16-multiply step against the SAME step in fp32 -- a sanity bound on what operand rounding does END TO END (the
    parity statement is the comparison with the oracle on bf16-rounded operands below, and 1e-2 per operation in
    test_gpu_nn.py): emissions and loss within 2e-2 of the largest magnitude after the 4 + 18 convolutions and 37 fl::Linear
    of the recipe all round their operands (1.04e-2 measured since the sub-sampling convolutions -- and with them the input
    features -- are rounded too, as fl's O1 mode casts every conv2d input; 0.7e-2 before), every parameter gradient in
    direction and size; the criterion input and the master weights stay fp32; training with it reduces the loss"""
    import re
    from wav2letter_amd import recipes
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(33)
    nfeat, nlabel, B, T, L = 80, 9998, 2, 160, 6
    arch = re.sub(r"(TDS \d+ \d+ \d+) [0-9.]+", r"\1 0.0", recipes.streaming_tds_arch())
    arch = "\n".join(l for l in arch.splitlines() if not l.startswith("SAUG")) + "\n"
    arch = re.sub(r"^DO [0-9.]+$", "DO 0.0", arch, flags=re.M)
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)).cuda()
    outs = {}
    for mp in (False, True):
        tr = Trainer(arch, nfeat, nlabel, "ctc", 4)
        tr.init_params(seed=5)
        To = tr.plan(B, T, L)
        tr.to_device()
        tr.set_mixed_precision(mp)
        em = tr.forward(x, train=False).clone()
        loss = tr.forward_backward(x, tgt).clone()
        outs[mp] = (em, loss, tr.grads.clone(), tr)
    assert To >= L
    em32, l32, g32, _ = outs[False]
    em16, l16, g16, tr16 = outs[True]
    assert em16.dtype == torch.float32 and tr16.params.dtype == torch.float32
    assert not torch.equal(em16, em32)          # the bf16 kernel really ran
    assert (em16 - em32).abs().max().item() < 2e-2 * em32.abs().max().item()
    assert (l16 - l32).abs().max().item() < 2e-2 * l32.abs().max().item()
    for name, n, off in tr16.param_table():
        a, b = g16[off:off + n].double(), g32[off:off + n].double()
        assert torch.isfinite(a).all()
        if n <= 2:
            continue   # LayerNorm (gain, offset): two sums over every activation with heavy cancellation -- no direction to check
        l2 = ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
        cos = (a @ b / (a.norm() * b.norm()).clamp_min(1e-30)).item()
        # bias vectors are column sums with cancellation (and bf16 noise flips ReLU masks upstream): looser than the weights;
        # since round 3 the TDS convolutions round their operands too (see the bars of the oracle comparison below)
        lim = (0.2, 0.98) if n > 1000 else (0.35, 0.95)
        assert l2 < lim[0] and cos > lim[1], (name, off, l2, cos)
    losses = []
    for _ in range(12):
        losses.append(tr16.forward_backward(x, tgt).sum().item())
        tr16.update(lr=0.05, momentum=0.0, max_grad_norm=0.5)
    assert np.isfinite(losses).all() and losses[-1] < 0.8 * losses[0], losses


def _streaming_arch_no_dropout():
    import re
    from wav2letter_amd import recipes
    arch = re.sub(r"(TDS \d+ \d+ \d+) [0-9.]+", r"\1 0.0", recipes.streaming_tds_arch())
    arch = "\n".join(l for l in arch.splitlines() if not l.startswith("SAUG")) + "\n"
    return re.sub(r"^DO [0-9.]+$", "DO 0.0", arch, flags=re.M)


def test_streaming_tds_config3_full_network_end_to_end(oracle):
    """BASELINE config 3 in fp32 -- the full streaming_convnets recipe network (am_500ms_future_context.arch: `PD`
    asymmetric padding, unpadded strided C2, per-frame LayerNorm, 16 TDS blocks with 15 / 19 / 23 / 27 channels and a
    right padding, 115.1 M parameters, 9998 word pieces) -- at a reduced batch and number of frames, dropout and
    SpecAugment off: emissions, CTC loss and every parameter gradient against the numpy reference network
    (oracle/refnet.py, itself held to torch autograd on this arch by tests/test_oracle_nn.py) + the CTC oracle."""
    rng = np.random.default_rng(31)
    nfeat, nlabel, B, T, L = 80, 9998, 2, 160, 6
    arch = _streaming_arch_no_dropout()
    tr, ref, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.full((B, L), -1, np.int32)
    tgt[0, :6] = [17, 4021, 9996, 3, 3, 77]
    tgt[1, :2] = [9000, 12]
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    assert em.shape == em_ref.shape == (B, 20, nlabel)
    assert rel(em, em_ref) < TOL
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < TOL
    n_strict, n = check_grads_relu_robust(tr, ref.backward(o.backward().astype(np.float32), len(params)))
    assert n_strict >= 2      # the final Linear has no ReLU kink between itself and the loss


def test_streaming_tds_config3_bf16_against_bf16_operand_oracle(oracle):
    """BASELINE config 3 in its mixed-precision mode against the ORACLE (not against the fp32 HIP step): the reference
    network with every fl::Linear multiplying bf16-ROUNDED operands (refnet.RefNet(bf16=True): x, w, dy rounded to nearest
    even, fp32 accumulation, fp32 bias / LayerNorm / convolutions / criterion -- cpc/Train.cpp:1184 keeps the criterion
    input f32).  Emissions and loss within the stated bf16 tolerance 1e-2 of the largest reference magnitude; parameter
    gradients in direction and size.  A rounding boundary crossed on one side only (an activation that rounds up here and
    down there because the fp32 values differ in the last bit) moves a product by 2^-8 relative: hence 1e-2, not 1e-4."""
    rng = np.random.default_rng(32)
    nfeat, nlabel, B, T, L = 80, 9998, 2, 160, 6
    arch = _streaming_arch_no_dropout()
    tr, _, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    tr.set_mixed_precision(True)
    ref = refnet.RefNet(arch, nfeat, nlabel, bf16=True)
    ref32 = refnet.RefNet(arch, nfeat, nlabel)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = np.full((B, L), -1, np.int32)
    tgt[0, :4] = [5, 5, 9000, 1]
    tgt[1, :6] = [1, 2, 3, 4, 5, 6]
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    em_32 = ref32.forward(x, params)
    BF16_TOL = 1e-2
    assert rel(em, em_ref) < BF16_TOL
    # the bf16 path really ran, and it is closer to the bf16-operand oracle than the fp32 oracle is
    assert rel(em, em_32) > 1e-5 and rel(em, em_ref) <= rel(em_32, em_ref) * 1.5 + 1e-4
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < BF16_TOL
    ref.upstream = []
    ref_grads = ref.backward(o.backward().astype(np.float32), len(params))
    g = tr.grads.cpu().numpy()
    table = tr.param_table()
    for i, want in enumerate(ref_grads):
        got = np.asarray(tr.export_from(i, g), np.float64).reshape(-1)
        w = np.asarray(want, np.float64).reshape(-1)
        assert np.isfinite(got).all()
        if w.size <= 2:
            continue   # LayerNorm (gain, offset): two sums over every activation with heavy cancellation
        l2 = np.linalg.norm(got - w) / max(1e-30, np.linalg.norm(w))
        cos = float(got @ w) / max(1e-30, np.linalg.norm(got) * np.linalg.norm(w))
        # Two bf16 implementations of a DEEP network agree statistically, not element by element: an activation that falls on
        # the other side of a bf16 rounding boundary (the two sides' fp32 sums differ in the last bit) moves by 2^-8 relative,
        # which moves later roundings and ReLU masks, 32 bf16 products deep -- measured on this arch (run j3): relative L2
        # 15 %, cosine 0.988 on the first TDS convolution's weights.  Hence direction-and-size bars here; the EXACTNESS of
        # the bf16 path (same rounded operands -> same result to fp32 accumulation error) is held by the one-block test below
        # and by tests/test_gpu_nn.py::test_gemm_bf16_operand_storage.
        lim = (0.2, 0.98) if w.size > 1000 else (0.35, 0.95)
        assert l2 < lim[0] and cos > lim[1], (i, table[i][0], l2, cos)
    # ... and at FULL depth with the compounding taken out: every one of the 14 TDS blocks alone, at its own geometry and
    # parameters, on the oracle's activation and upstream gradient, at the strict 2e-3 bar (round-3 verdict item 9)
    del tr
    nblk, worst = teacher_forced_tds_blocks(ref, arch, params, ref_grads)
    assert nblk == 14
    print("config 3 bf16, 14 teacher-forced TDS blocks: worst relative error of an output / parameter gradient %.2e" % worst)


def test_streaming_tds_one_block_bf16_matches_bf16_operand_oracle_closely(oracle):
    """ONE TDS block of the streaming recipe's first stage (c = 15, kw = 9, 80 mel rows, per-frame LayerNorm, right padding 1)
    between a sub-sampling convolution and the output Linear, mixed precision against the bf16-operand oracle: with no depth
    for rounding-boundary flips to compound, emissions, loss and EVERY parameter gradient agree to 2e-3 of the largest
    magnitude (the residue: a handful of activations rounded to the neighbouring bf16 value on one side only)"""
    rng = np.random.default_rng(35)
    nfeat, nlabel, B, T, L = 80, 50, 3, 96, 5
    arch = ("V -1 NFEAT 1 0\nPD 0 5 3\nC2 1 15 10 1 2 1 0 0\nR\nDO 0.0\nLN 1 2\nTDS 15 9 80 0.0 0 1 0\n"
            "RO 2 1 0 3\nV 1200 -1 1 0\nL 1200 NLABEL\nV NLABEL 0 -1 1\n")
    tr, _, params, _ = build(arch, nfeat, nlabel, "ctc", 4, 0.0, rng, B, T, L)
    tr.set_mixed_precision(True)
    ref = refnet.RefNet(arch, nfeat, nlabel, bf16=True)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    em = tr.forward(xd, train=False).cpu().numpy()
    em_ref = ref.forward(x, params)
    assert rel(em, em_ref) < 2e-3
    loss = tr.forward_backward(xd, td).cpu().numpy()
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    assert rel(loss, o.forward()) < 2e-3
    ref_grads = ref.backward(o.backward().astype(np.float32), len(params))
    g = tr.grads.cpu().numpy()
    table = tr.param_table()
    for i, want in enumerate(ref_grads):
        got = tr.export_from(i, g)
        assert rel(got, want) < (2e-3 if np.asarray(want).size > 2 else 2e-2), (i, table[i][0], rel(got, want))


def test_linseg_phase_has_its_own_momentum():
    """the reference trains the --linseg warm-up with separate optimizers (linNetoptim / linCritoptim, Train.cpp:589-617):
    the first ASG update starts from ZERO momentum, not from the warm-up's"""
    from wav2letter_amd import recipes
    from wav2letter_amd.trainer import Trainer
    rng = np.random.default_rng(3)
    nfeat, nlabel, B, T, L = 40, 12, 2, 40, 5
    arch = recipes.conv_glu_small_arch()
    x = torch.tensor(rng.normal(size=(B, nfeat, T)).astype(np.float32)).cuda()
    tgt = torch.tensor(rng.integers(0, nlabel - 2, size=(B, L)).astype(np.int32)).cuda()
    tr = Trainer(arch, nfeat, nlabel, "asg", 4, 1.0)
    tr.set_linseg(2)
    tr.init_params(3)
    tr.plan(B, T, L)
    tr.to_device()
    kw = dict(lr=0.05, lrcrit=0.001, momentum=0.9, max_grad_norm=1.0, total_batch=B)
    for _ in range(2):                      # two warm-up updates build up momentum
        tr.forward_backward(x, tgt)
        tr.update(**kw)
    assert tr.mom.abs().max().item() > 0
    tr.forward_backward(x, tgt)             # update 2: the ASG criterion proper
    g = tr.grads.clone()
    p0 = tr.params.clone()
    tr.update(**kw)
    # with zero starting momentum the step is exactly -lr * clip(g / B)
    n = tr.n_net
    gs = g[:n].double() / B
    norm = (g.double() / B).norm().item()
    gs = gs * min(1.0, 1.0 / (norm + 1e-6))
    want = p0[:n].double() - 0.05 * gs
    assert (tr.params[:n].double() - want).abs().max().item() < 1e-6 * max(1.0, want.abs().max().item())
    assert (tr.mom[:n].double() - gs).abs().max().item() < 1e-6 * max(1.0, gs.abs().max().item())


# ---- the mixed-precision TDS block across geometries ------------------------------------------------------------------------
# One block alone (the `V / TDS / RO / V / V` network of teacher_forced_tds_blocks), random input and output gradient, each case
# at a geometry meant to reach one branch of the choice TDSLayer and its FeedForward pair make between the bf16 operators
# (host/net.cpp; launch128h's refusal conditions in gemm_bf16g.hpp).  Line: TDS c kw h dropout l2 rPad lnIncludeTime.
TDS_BF16_CASES = [
    # config 2's block (sota TDS-CTC), reduced B / T: time-wise LayerNorm, so y1's rows are not the LayerNorm's groups -- no LN
    # images, y1 joins the weights' w2l_bf16_convert_multi and gets its ones row from ensureOnes; c = 10, kw = 21 at 80 rows:
    # bf16 convolution kernels
    pytest.param("TDS 10 21 80 0.0 0 -1 1", 2, 24, id="sota-c2-timewise-ln"),
    # wide hidden layer with l2 % 32 != 0 (l2 % 4 == 0): lin1's image-writing epilogue at an N that is not a tile multiple
    # (M = 128 rows: at 32 a single one-sided bf16 rounding of du moves lin1's weight gradient by 2.4e-3 of its largest value)
    pytest.param("TDS 14 21 80 0.0 1000", 2, 64, id="wide-l2-1000"),
    # per-frame LayerNorm with 2400-float rows (> 2304): the LayerNorm-images kernels refuse -> plain LayerNorm + conversion;
    # right padding 1; c = 30 at kw = 11 still has bf16 convolution kernels
    pytest.param("TDS 30 11 80 0.0 0 1 0", 2, 16, id="frame-ln-row-2400"),
    # h = 10 (not a multiple of 16): convImgElems == 0, the convolution stays fp32 (the oracle must not round it either)
    pytest.param("TDS 8 9 10 0.0 0 -1 1", 2, 20, id="conv-fp32-h10"),
    # c = 40 > 32 at h = 16: convImgElems == 0 as well
    pytest.param("TDS 40 5 16 0.0 0", 2, 16, id="conv-fp32-c40"),
    # l = 15 (l % 4 != 0), l2 = 16: lin1 writes u as images only (FeedForward::uOnlyImages); y1's images, the backward-data
    # product of lin1 and the fp32 du all have rows of 15; h = 3 keeps the convolution fp32
    pytest.param("TDS 5 3 3 0.0 16", 2, 16, id="l15-l2-16"),
    # l2 = 30 (l2 % 4 != 0): lin1's image epilogue refuses -> fp32 u + conversion; lin2's backward-data with the fp32 mask
    pytest.param("TDS 8 9 16 0.0 30", 2, 16, id="l2-30-fp32-u"),
    # B = 3, T = 37: M = 111 rows, partial GEMM / convolution tiles everywhere
    pytest.param("TDS 8 9 16 0.0 0", 3, 37, id="ragged-M-111"),
    # dropout 0.2 in config 2's block: lin1's dropout epilogue into the images; time-wise LayerNorm -> dv's images by
    # convertDropout (maskInConvert: the bias gradient rides on the weight-gradient product)
    pytest.param("TDS 10 21 80 0.2 0 -1 1", 2, 24, id="sota-c2-dropout"),
    # dropout 0.2 in config 3's per-frame block: dropout inside the LayerNorm-images kernels (forward and backward)
    pytest.param("TDS 15 9 80 0.2 0 1 0", 2, 16, id="c3-frame-dropout"),
]


def _tds_block_run(one, l, B, T, params, feed, dout, mp, step):
    tr, table = _one_block_trainer(one, l, l, B, T, params)
    tr.set_mixed_precision(mp)
    tr.set_step(step)
    em = tr.forward(torch.tensor(feed).cuda(), train=True).cpu().numpy().copy()
    tr.backward(torch.tensor(dout).cuda())
    g = tr.grads.cpu().numpy()
    grads = [tr.export_from(i, g).copy() for i in range(8)]
    del tr
    return em, grads, table


@pytest.mark.parametrize("line, B, T", TDS_BF16_CASES)
def test_tds_block_bf16_geometries_against_bf16_operand_oracle(oracle, line, B, T):
    """one mixed-precision TDS block, training mode, against refnet.tds_fwd / tds_bwd(bf16=True) with the library's own dropout
    masks (seed of the step, host/trainer.cpp; streams rngStream, + 1, + 2 of the block's layer, Sequential::finalize): output
    and EVERY parameter gradient at 2e-3 of the largest magnitude (LayerNorm (gain, bias) pairs 2e-2), as the config 3
    one-block test.  The bf16 path must have run (the output differs from the fp32 run of the same block), and without dropout
    the bar must tell the rounded oracle from the unrounded one (error against the first at most half that against the second)"""
    from oracle import pyoracle
    t = line.split()
    c, kw, h = int(t[1]), int(t[2]), int(t[3])
    pdrop = float(t[4])
    l = c * h
    l2 = int(t[5]) if len(t) > 5 and int(t[5]) else l
    rpad = int(t[6]) if len(t) > 6 else -1
    mode = "frame" if len(t) > 7 and int(t[7]) == 0 else "all"
    pl, pr = (pyoracle.same_pad(T, kw, 1),) * 2 if rpad < 0 else (kw - 1 - rpad, rpad)
    rng = np.random.default_rng(sum(line.encode()) + B * 100 + T)
    p = refnet.TDSParams(c, kw, h, l2, rng=rng)
    params = [p.wc, p.bc, np.array([p.g1, p.b1n], np.float32), p.w1, p.b1, p.w2, p.b2, np.array([p.g2, p.b2n], np.float32)]
    x = rng.normal(size=(B, c, h, T)).astype(np.float32)
    dout = rng.normal(size=(B, c, h, T)).astype(np.float32)
    step = 3
    masks = None
    if pdrop > 0:
        seed = (0x9E3779B9 * (step + 1)) & 0xFFFFFFFF    # host/trainer.cpp makeCtx: the step's dropout seed
        stream = 1 + 4 * 2                                # layer 2 of the Sequential (V, RO, TDS, ...): rngStream
        n = B * c * h * T
        draw = lambda k, size: pyoracle.dropout(np.ones(size, np.float32), pdrop, seed, stream + k)
        masks = (refnet.from_frames(draw(0, n).reshape(B * T, l), B, c, h, T), draw(1, B * T * l2).reshape(B * T, l2),
                 refnet.from_frames(draw(2, n).reshape(B * T, l), B, c, h, T))
    want = {}
    for bf in (True, False):
        out, saved = refnet.tds_fwd(x, p, pl, pr, mode, keep=True, bf16=bf, masks=masks)
        dx, g = refnet.tds_bwd(dout, p, saved, pl, pr, mode, bf16=bf)
        want[bf] = (out, [g["wc"], g["bc"], np.array([g["g1"], g["b1n"]]), g["w1"], g["b1"], g["w2"], g["b2"], np.array([g["g2"], g["b2n"]])])
    one = "V -1 %d %d 0\nRO 0 2 1 3\n%s\nRO 2 1 0 3\nV %d -1 1 0\nV %d 0 -1 1\n" % (c, h, line, l, l)
    to_em = lambda a: np.ascontiguousarray(a.transpose(0, 3, 2, 1)).reshape(B, T, l)   # [B][c][h][T] -> [B][T][h * C + c]
    feed = np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B, l, T)              # [B][h * C + c][T]
    em16, g16, table = _tds_block_run(one, l, B, T, params, feed, to_em(dout), True, step)
    em32, g32, _ = _tds_block_run(one, l, B, T, params, feed, to_em(dout), False, step)
    err = {bf: [rel(em16, to_em(want[bf][0]))] + [rel(g16[i], want[bf][1][i]) for i in range(8)] for bf in (True, False)}
    big = [True] + [np.asarray(w).size > 2 for w in want[True][1]]
    worst = {bf: max(e for e, b in zip(err[bf], big) if b) for bf in (True, False)}
    d32 = rel(em16, em32)
    print("\n%s B=%d T=%d: worst error vs bf16-operand oracle %.2e, vs unrounded oracle %.2e; output vs fp32 run %.2e"
          % (line, B, T, worst[True], worst[False], d32))
    for i, (e, b) in enumerate(zip(err[True], big)):
        assert e < (2e-3 if b else 2e-2), (line, "output" if i == 0 else table[i - 1][0], e)
    assert d32 > 1e-4, d32                           # the bf16 kernels ran
    assert max(rel(a, b) for a, b in zip(g16, g32)) > 1e-4
    if pdrop == 0:
        assert worst[True] <= 0.5 * worst[False], (worst[True], worst[False])


# ---- the mixed-precision Transformer block across geometries ----------------------------------------------------------------
TR_BF16_CASES = [
    # mlp = 70 (% 4 != 0): lin1's image epilogue refuses -> fp32 u + conversion (FeedForward::uOnlyImages false)
    pytest.param("TR 64 70 4 8", 2, 40, None, id="mlp70"),
    # mlp = 100 (% 4 == 0, % 32 != 0): the image epilogue at a non-tile-multiple N
    pytest.param("TR 64 100 4 8", 2, 40, None, id="mlp100"),
    # csz = 0: no position table
    pytest.param("TR 64 128 4 0", 2, 40, None, id="csz0"),
    # head size 32, T <= 192: the fused attention kernels
    pytest.param("TR 128 256 4 10", 2, 150, None, id="head32-fused-T150"),
    # head size 32, T > 192: the unfused bf16 attention at a head size that otherwise fuses
    pytest.param("TR 128 256 4 10", 2, 200, None, id="head32-unfused-T200"),
    # B = 3 with input sizes: the padded keys are masked (key lengths 48, 40, 29 frames)
    pytest.param("TR 64 128 4 8", 3, 48, [4800.0, 4000.0, 2900.0], id="padded-B3"),
]


@pytest.mark.parametrize("line, B, T, sizes", TR_BF16_CASES)
def test_transformer_block_bf16_geometries(oracle, line, B, T, sizes):
    """one mixed-precision TR block between a View and the output Linear, against the float64 restatement at the bars of
    test_transformer_block_at_config5_width_bf16 (emissions and loss 1e-2 of the largest magnitude; every parameter gradient
    cosine > 0.995, relative L2 < 8 %), and against the fp32 step of the same network: emissions and loss within 2e-2 of the
    largest magnitude, gradients at the same direction-and-size bars (as test_mixed_precision_streaming_tds_step: a gradient's
    largest element moves by up to ~10 % between the two modes at these sizes)"""
    from wav2letter_amd.trainer import Trainer
    C = int(line.split()[1])
    nfeat, nlabel, L = C, 12, 4
    arch = "V -1 1 NFEAT 0\nRO 2 0 3 1\n%s 0.0 0.0\nL %d NLABEL\n" % (line, C)
    rng = np.random.default_rng(B * 1000 + T + C)
    ref = refnet.RefNet(arch, nfeat, nlabel)
    params = ref.random_params(rng)
    x = rng.normal(size=(B, 1, nfeat, T)).astype(np.float32)
    tgt = rng.integers(0, nlabel - 1, size=(B, L)).astype(np.int32)
    xd = torch.tensor(x.reshape(B, nfeat, T)).cuda()
    td = torch.tensor(tgt).cuda()
    if sizes is not None:
        ref.input_sizes = np.array(sizes, np.float32)
        assert rel(ref.forward(x, params), refnet.RefNet(arch, nfeat, nlabel).forward(x, params)) > 1e-2   # the mask matters
    em_ref = ref.forward(x, params)
    o = oracle.CTC(em_ref, tgt, scale_mode=4)
    loss_ref = o.forward()
    want = ref.backward(o.backward().astype(np.float32), len(params))
    runs = {}
    for mp in (False, True):
        tr = Trainer(arch, nfeat, nlabel, "ctc", 4, 0.0)
        for i, p in enumerate(params):
            tr.import_param(i, p)
        tr.plan(B, T, L)
        tr.to_device()
        tr.set_mixed_precision(mp)
        if sizes is not None:
            szd = torch.tensor(np.array(sizes, np.float32)).cuda()
            tr.set_input_sizes(szd)
        em = tr.forward(xd, train=False).cpu().numpy().copy()
        loss = tr.forward_backward(xd, td).cpu().numpy().copy()
        g = tr.grads.cpu().numpy()
        runs[mp] = (em, loss, [tr.export_from(i, g).copy() for i in range(len(params))], tr.param_table())
        del tr
    em, loss, g16, table = runs[True]
    em32, loss32, g32, _ = runs[False]
    worst_cos, worst_l2 = 1.0, 0.0
    print("\n%s B=%d T=%d: emissions vs float64 %.2e, vs fp32 step %.2e" % (line, B, T, rel(em, em_ref), rel(em, em32)))
    assert rel(em, em_ref) < 1e-2 and rel(loss, loss_ref) < 1e-2, (rel(em, em_ref), rel(loss, loss_ref))
    assert rel(em, em32) < 2e-2 and rel(loss, loss32) < 2e-2, (rel(em, em32), rel(loss, loss32))
    assert not np.array_equal(em, em32)           # the bf16 kernels ran
    bad = []
    for i, (name, _n, _off) in enumerate(table):
        if name == "tr.wk.b":   # exactly zero in exact arithmetic
            continue
        got = g16[i].astype(np.float64).reshape(-1)
        w = np.asarray(want[i], np.float64).reshape(-1)
        cos = float(got @ w / (np.linalg.norm(got) * np.linalg.norm(w) + 1e-300))
        l2 = float(np.linalg.norm(got - w) / (np.linalg.norm(w) + 1e-300))
        b = g32[i].astype(np.float64).reshape(-1)
        cos32 = float(got @ b / (np.linalg.norm(got) * np.linalg.norm(b) + 1e-300))
        l2_32 = float(np.linalg.norm(got - b) / (np.linalg.norm(b) + 1e-300))
        worst_cos, worst_l2 = min(worst_cos, cos, cos32), max(worst_l2, l2, l2_32)
        bad += [(name, cos, l2, cos32, l2_32)] if not (min(cos, cos32) > 0.995 and max(l2, l2_32) < 0.08) else []
    print("  gradients vs float64 and fp32 step: worst cosine %.5f, relative L2 %.2e" % (worst_cos, worst_l2))
    assert not bad, bad
