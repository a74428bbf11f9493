"""BASELINE config C4 on one GPU: conv_glu LibriSpeech (17 WN-conv + GLU layers, 208.9 M parameters) with the ASG
criterion, N = 30 tokens, T = 2000 frames of 40 filterbanks, batch 64: full training steps (forward, ASG forward /
backward, backward, clip + SGD) in three modes of ONE process -- fp32, mixed precision (level 1: the fl::Linear products), mixed
precision + the bf16 wide convolutions (level 2, w2l_conv_bf16_*) -- visited in turn `rounds` times (same-run A/B: a mode's figure is
the median over all its timed steps, each visit starts with an untimed step), then the 17 convolutions one by one: the three
passes on the fp32 kernels (w2l_conv_*) and on the bf16 kernels (image conversions included; the share of the GEMM launches
from the library's event brackets), medians of `reps` calls.
  python tools/c4_step.py [steps per visit] [batch] [rounds] [reps]"""
import ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from wav2letter_amd import CriterionScaleMode, _lib, recipes
from wav2letter_amd.trainer import Trainer

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
T, nfeat, nlabel, Lmax = 2000, 40, 30, 300
fl = recipes.CONV_GLU_FLAGS
arch = recipes.conv_glu_librispeech_arch()
L = _lib.lib()
g = torch.Generator().manual_seed(4)
x = torch.randn(B, nfeat, T, generator=g).cuda()
tgt = torch.full((B, Lmax), -1, dtype=torch.int32)
for b in range(B):
    l = int(torch.randint(60, Lmax + 1, (1,), generator=g))
    y = torch.randint(0, 28, (l,), generator=g, dtype=torch.int32)
    for i in range(1, l):
        if y[i] == y[i - 1]:
            y[i] = (y[i] + 1) % 28
    tgt[b, :l] = y
tgt = tgt.cuda()

tr = Trainer(arch, nfeat, nlabel, "asg", CriterionScaleMode.TARGET_SZ_SQRT, transdiag=fl["transdiag"])
tr.init_params(seed=1)
Tout = tr.plan(B, T, Lmax)
tr.to_device()
MODES = [("fp32", False, False), ("mixed", True, False), ("mixed+convs", True, True)]


def step():
    loss = tr.forward_backward(x, tgt)
    tr.update(lr=fl["lr"], lrcrit=fl["lrcrit"], momentum=fl["momentum"], max_grad_norm=fl["maxgradnorm"], total_batch=B)
    return loss


times = {m[0]: [] for m in MODES}
losses = {}
for r in range(rounds):
    for name, mixed, convs in MODES:
        tr.set_mixed_precision(mixed, convs=convs)
        step()
        torch.cuda.synchronize()
        for _ in range(steps):
            t0 = time.perf_counter()
            loss = step()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
        losses[name] = float(loss.float().mean().item())
for name, _, _ in MODES:
    dt = statistics.median(times[name])
    print("[c4] " + json.dumps({"config": f"C4 conv_glu LibriSpeech ASG: B={B}, T={T}, 40 fbank, N=30, Tout={Tout}", "mode": name,
                                "ms_per_step_median": round(dt * 1e3, 1), "ms_per_step_all": [round(t * 1e3, 1) for t in times[name]],
                                "utterances_per_sec": round(B / dt, 2), "loss_mean": losses[name]}), flush=True)
f32, l2 = statistics.median(times["fp32"]), statistics.median(times["mixed+convs"])
print(f"[c4] level 2 against fp32, same run: {f32 / l2:.2f}x ({f32 * 1e3:.1f} -> {l2 * 1e3:.1f} ms)", flush=True)
del tr
torch.cuda.empty_cache()

# ---- the 17 convolutions one by one ----------------------------------------------------------------------------------------
s = torch.cuda.current_stream().cuda_stream


def timed(fn):
    fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def gemm_ms(fn):
    """ms of the bf16 GEMM launches inside fn (the library's event brackets)"""
    L.w2l_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    n_, ms_, w_ = C.c_int(0), C.c_double(0), C.c_double(0)
    L.w2l_profile_report_kind(6, C.byref(n_), C.byref(ms_), C.byref(w_))
    L.w2l_profile_enable(0)
    return ms_.value


def ok(st):
    assert st == 0, st


print("[c4-layer] cin cout kw pad T | fp32 fwd bwd-data bwd-filter ms | bf16 fwd bwd-data bwd-filter ms (of which GEMM) | prepare ms | "
      "TFLOP/s fp32 -> bf16 (three passes)", flush=True)
Tl = T
tot = {"f32": 0.0, "bf16": 0.0, "gemm": 0.0, "prep": 0.0}
for line in arch.splitlines():
    t = line.split()
    if t[:3] != ["WN", "3", "C"]:
        continue
    cin = nfeat if t[3] == "NFEAT" else int(t[3])
    cout, kw, stride, pad = int(t[4]), int(t[5]), int(t[6]), int(t[7])
    if pad == -1:
        pad = L.w2l_conv_same_pad(Tl, kw, stride)
    d = _lib.ConvDesc(B, Tl, 1, cin, cout, kw, stride, pad, pad)
    To = L.w2l_conv_out_len(Tl, kw, stride, pad, pad)
    xs = torch.randn(B, Tl, 1, cin, device="cuda")
    w = torch.randn(kw, cin, cout, device="cuda") / (cin * kw) ** 0.5
    bias = torch.randn(cout, device="cuda")
    dy = torch.randn(B, To, 1, cout, device="cuda")
    ys, dx, dw, db = torch.empty_like(dy), torch.empty_like(xs), torch.empty_like(w), torch.empty_like(bias)
    P = lambda a: a.data_ptr()
    f = [timed(lambda: ok(L.w2l_conv_forward(C.byref(d), P(xs), P(w), P(bias), P(ys), 0, s))),
         timed(lambda: ok(L.w2l_conv_backward_data(C.byref(d), P(dy), P(w), P(dx), 0, s))),
         timed(lambda: ok(L.w2l_conv_backward_filter(C.byref(d), P(xs), P(dy), P(dw), P(db), s)))]
    n = L.w2l_conv_bf16_image_elems(C.byref(d))
    row = f"[c4-layer] {cin:4d} {cout:4d} {kw:2d} {pad:3d} {Tl:4d} | {f[0]:7.2f} {f[1]:7.2f} {f[2]:7.2f} |"
    if n:
        imgs = torch.empty(2, n, dtype=torch.bfloat16, device="cuda")
        scr = torch.empty(L.w2l_conv_bf16_scratch_elems(C.byref(d)), dtype=torch.bfloat16, device="cuda")
        prep = lambda: ok(L.w2l_conv_bf16_prepare(C.byref(d), P(w), P(imgs[0]), P(imgs[1]), s))
        calls = [lambda: ok(L.w2l_conv_bf16_forward(C.byref(d), P(xs), P(imgs[0]), P(bias), P(ys), 0, P(scr), s)),
                 lambda: ok(L.w2l_conv_bf16_backward_data(C.byref(d), P(dy), P(imgs[1]), None, P(dx), P(scr), s)),
                 lambda: ok(L.w2l_conv_bf16_backward_filter_bias(C.byref(d), P(xs), P(dy), P(dw), P(db), P(scr), s))]
        tp = timed(prep)
        h = [timed(c) for c in calls]
        gm = [gemm_ms(c) for c in calls]
        flops = 2.0 * B * To * cin * cout * kw * 3
        row += (f" {h[0]:7.2f} {h[1]:7.2f} {h[2]:7.2f} ({gm[0]:.2f} {gm[1]:.2f} {gm[2]:.2f}) | {tp:6.2f} | "
                f"{flops / sum(f) / 1e9:6.1f} -> {flops / (sum(h) + tp) / 1e9:6.1f}")
        tot["f32"] += sum(f); tot["bf16"] += sum(h); tot["gemm"] += sum(gm); tot["prep"] += tp
    else:
        row += " no bf16 kernel: fp32"
        tot["f32"] += sum(f); tot["bf16"] += sum(f)
    print(row, flush=True)
    del xs, w, dy, ys, dx, dw
    torch.cuda.empty_cache()
    Tl = To
conv = tot["bf16"] - tot["gemm"]
print(f"[c4-layer] sum of the 17 layers: fp32 {tot['f32']:.1f} ms; bf16 {tot['bf16'] + tot['prep']:.1f} ms = GEMM launches {tot['gemm']:.1f} + "
      f"activation / gradient images and column sums {conv:.1f} + weight images {tot['prep']:.1f} "
      f"(images: {(conv + tot['prep']) / (tot['bf16'] + tot['prep']):.1%} of the bf16 convolution time)", flush=True)
