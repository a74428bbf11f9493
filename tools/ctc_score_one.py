"""w2l_ctc_score against w2l_ctc_forward + w2l_ctc_viterbi, timed with hip events after warm-up, at the validation shapes of the
TDS-CTC recipe:   python tools/ctc_score_one.py [reps]
  B = 32, T = 188,  N = 9998, L <= 80   (config 2: 240 MB of emissions)
  B = 32, T = 1500, N = 9998, L <= 80
Prints per call: microseconds, the emission bytes the pass must read (4 B T N per read: 1 read for score, 2 for forward +
viterbi) over that time, and that rate as a fraction of the 8.0 TB/s HBM peak (MI355X spec).  At T = 188 the emissions fit
the 256 MiB Infinity Cache, so the second read of forward + viterbi may be served from there."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from wav2letter_amd import _lib, criterion as Cr

HBM_PEAK = 8.0e12


def bench(T, reps, B=32, N=9998, Lt=80):
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(B, T, N, generator=g).cuda()
    tgt = torch.full((B, Lt), -1, dtype=torch.int32)
    for b in range(B):
        n = int(torch.randint(20, Lt + 1, (1,), generator=g))
        tgt[b, :n] = torch.randint(0, N - 1, (n,), generator=g, dtype=torch.int32)
    tgt = tgt.cuda()
    ts = Cr.batch_target_size(tgt, T, ctc=True)
    ws = torch.empty(L.w2l_ctc_workspace_size(B, T, N, Lt), dtype=torch.uint8, device="cuda")
    wss = torch.empty(L.w2l_ctc_score_workspace_size(B, T, N, Lt), dtype=torch.uint8, device="cuda")
    loss, loss2 = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    path = torch.empty(B, T, dtype=torch.int32, device="cuda")
    path2 = torch.empty_like(path)
    st = torch.cuda.current_stream().cuda_stream

    def two_pass():
        _lib.check(L.w2l_ctc_forward(B, T, N, Lt, 4, x.data_ptr(), tgt.data_ptr(), ts.data_ptr(), loss.data_ptr(), ws.data_ptr(), st), "fwd")
        _lib.check(L.w2l_ctc_viterbi(B, T, N, x.data_ptr(), path.data_ptr(), st), "viterbi")

    def score():
        _lib.check(L.w2l_ctc_score(B, T, N, Lt, 4, x.data_ptr(), tgt.data_ptr(), ts.data_ptr(), loss2.data_ptr(), path2.data_ptr(),
                                   wss.data_ptr(), st), "score")

    def timed(fn):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    out = {"B": B, "T": T, "N": N, "L": Lt}
    # alternate the two, twice each: a drift of the box shows as a spread between the two runs of one
    t = {"fwd+viterbi": [], "score": []}
    for _ in range(2):
        t["fwd+viterbi"].append(timed(two_pass))
        t["score"].append(timed(score))
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(path, path2), "results differ"
    one_read = 4.0 * B * T * N
    for name, reads in (("fwd+viterbi", 2), ("score", 1)):
        us = min(t[name])
        out[name] = {"us": round(us, 1), "us_runs": [round(v, 1) for v in t[name]], "emission_reads": reads,
                     "read_TBps": round(reads * one_read / (us * 1e-6) / 1e12, 2),
                     "hbm_fraction": round(reads * one_read / (us * 1e-6) / HBM_PEAK, 3)}
    out["speedup"] = round(out["fwd+viterbi"]["us"] / out["score"]["us"], 2)
    return out


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    for T in (188, 1500):
        print(json.dumps(bench(T, reps)))
