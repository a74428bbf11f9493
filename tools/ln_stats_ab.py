"""LayerNorm entry points of TWO builds of the library timed against each other in one process, alternately, on the shapes the
benchmark launches: what a change of the statistic costs (profiles/layernorm_stats_ab.log).

    python tools/ln_stats_ab.py --old /path/to/parent/libw2l_hip.so [--new wav2letter_amd/libw2l_hip.so]

Shapes: the LayerNorms of the headline network (config 2), derived here from recipes.tds_ctc_arch() -- one group per utterance, the
group the frames x 80 mel rows x channels behind every stride-2 convolution -- and the per-frame LayerNorms 11968 x 1200 and
11968 x 2160 of the streaming recipe (config 3).  Per shape and call: four series old / new / old / new, each the median of `--windows`
windows of `--launches` launches between two device events.  The margin of a comparison is the spread the two series of the SAME
library show; a new median outside it is marked `<-- outside`."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from wav2letter_amd import _lib, recipes  # noqa: E402


def headline_shapes(B=32, T=1500, H=80):
    """(groups, inner) of the LayerNorms in recipes.tds_ctc_arch() at the benchmark's batch: LN 0 1 2 -> one group per utterance"""
    shapes, t, c = [], T, 1
    for line in recipes.tds_ctc_arch().splitlines():
        f = line.split()
        if f and f[0] == "C2":
            c, stride = int(f[2]), int(f[5])
            t = (t + stride - 1) // stride
            shapes.append((B, t * H * c))
    assert len(shapes) == 3, shapes
    return shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", required=True)
    ap.add_argument("--new", default=_lib.SO_PATH)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    a = ap.parse_args()
    libs = {"old": _lib._load(a.old), "new": _lib._load(a.new)}
    s = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()  # noqa: E731

    def series(fn, reset):
        ts = []
        for _ in range(a.windows):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                assert fn() == 0
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / a.launches * 1e3)
        return statistics.median(ts)

    print(f"# old = {os.path.basename(os.path.dirname(a.old))}/{os.path.basename(a.old)}, new = this tree; us per launch, "
          f"median of {a.windows} windows x {a.launches} launches; series order old new old new", flush=True)
    for G, inner in headline_shapes() + [(11968, 1200), (11968, 2160)]:
        g = torch.Generator(device="cuda").manual_seed(1)
        a0 = torch.randn(G * inner, device="cuda", generator=g).relu_()
        x = torch.randn(G * inner, device="cuda", generator=g)
        dy = torch.randn(G * inner, device="cuda", generator=g)
        gb = torch.tensor([1.3, 0.2], device="cuda")
        av = a0.clone(); r = torch.empty_like(av); y = torch.empty_like(av); mr = torch.empty(2 * G, device="cuda")
        dr = torch.empty_like(av); dm = torch.empty_like(av); dgb = torch.empty(2, device="cuda")
        nd = max(int(L.w2l_layernorm_scratch_doubles(G, inner)) for L in libs.values())
        st = torch.empty(nd, device="cuda", dtype=torch.float64)
        images = inner % 4 == 0 and inner <= 2304
        if images:
            ldR, ldT = (inner + 63) // 64 * 64, (G + 63) // 64 * 64
            rows = torch.empty((G, ldR), dtype=torch.bfloat16, device="cuda")
            trans = torch.empty((inner, ldT), dtype=torch.bfloat16, device="cuda")
            k = _lib.Bf16ImageSink(rowMajor=rows.data_ptr(), ldRows=ldR, transposed=trans.data_ptr(), ldTrans=ldT)
        reset = lambda: av.copy_(a0)  # noqa: E731  (the dropout of `a` is in place)

        def calls(L):
            c = {"forward (dropout + residual)": lambda: L.w2l_residual_layernorm_forward(G, inner, P(av), P(x), P(r), P(y), P(gb), 1e-5, 0.1, 7, 3, P(st), P(mr), s),
                 "forward (plain, in place)": lambda: L.w2l_residual_layernorm_forward(G, inner, P(r), None, P(r), P(y), P(gb), 1e-5, 0.0, 0, 0, P(st), P(mr), s),
                 "backward (+ mask)": lambda: L.w2l_layernorm_backward(G, inner, P(r), P(dy), P(gb), P(mr), P(dr), P(dgb), P(av), P(dm), 1.1, P(st), s)}
            if images:
                c["forward_images (dropout + residual)"] = lambda: L.w2l_residual_layernorm_forward_images(
                    G, inner, P(av), P(x), P(r), P(y), P(gb), 1e-5, 0.1, 7, 3, P(mr), C.byref(k), s)
                c["backward_images (+ mask)"] = lambda: L.w2l_layernorm_backward_images(
                    G, inner, P(r), P(dy), P(gb), P(mr), P(dr), P(dgb), P(av), P(dm), 1.1, P(st), C.byref(k), 0.0, 0, 0, s)
            return c

        table = {n: calls(L) for n, L in libs.items()}
        for name in table["new"]:
            for n in ("old", "new"):          # warm both: code objects, caches
                reset(); table[n]["forward (dropout + residual)"](); table[n][name]()
            torch.cuda.synchronize()
            t = [series(table[n][name], reset) for n in ("old", "new", "old", "new")]
            old, new = (t[0] + t[2]) / 2, (t[1] + t[3]) / 2
            margin = max(abs(t[0] - t[2]), abs(t[1] - t[3]))
            flag = "  <-- outside" if abs(new - old) > margin else ""
            print(f"{G} x {inner}  {name:38s} old {t[0]:8.1f} {t[2]:8.1f}  new {t[1]:8.1f} {t[3]:8.1f}  new - old {new - old:+7.1f} us "
                  f"({(new / old - 1) * 100:+.2f} %), same-library spread {margin:.1f} us{flag}", flush=True)


if __name__ == "__main__":
    main()
