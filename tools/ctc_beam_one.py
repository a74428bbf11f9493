"""w2l_ctc_beam_search, and w2l_ctc_score at the same shape in the same process, timed with hip events after warm-up at the
criterion shapes of the TDS-CTC recipe:   python tools/ctc_beam_one.py [reps] [T] [W]
  B = 32, T = 188 and 1500, N = 9998, (W, K) = (64, 64) and (8, 8), no threshold, nbest = 1
w2l_ctc_score is the yardstick: its row pass reads the same rows once.  Both searches are timed: logadd (sum over alignments, on
log-softmax rows) and max (on the raw emissions: no normaliser in the row pass, no exp / log in the scan).  Prints microseconds per
call, one JSON line per shape; a kernel trace (rocprofv3 --kernel-trace --stats, a run of its own) splits a call into
ctc_beam_rows / ctc_beam_scan / ctc_beam_finish and the clearing of the prefix table."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from wav2letter_amd import _lib, criterion as Cr


def bench(T, W, K, reps, B=32, N=9998, Lt=80):
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(B, T, N, generator=g).cuda()
    tgt = torch.full((B, Lt), -1, dtype=torch.int32)
    for b in range(B):
        n = int(torch.randint(20, Lt + 1, (1,), generator=g))
        tgt[b, :n] = torch.randint(0, N - 1, (n,), generator=g, dtype=torch.int32)
    tgt = tgt.cuda()
    ts = Cr.batch_target_size(tgt, T, ctc=True)
    wsb = torch.empty(L.w2l_ctc_beam_workspace_size(B, T, N, W, K), dtype=torch.uint8, device="cuda")
    wss = torch.empty(L.w2l_ctc_score_workspace_size(B, T, N, Lt), dtype=torch.uint8, device="cuda")
    loss = torch.empty(B, device="cuda")
    greedy = torch.empty(B, T, dtype=torch.int32, device="cuda")
    labels = torch.empty(B, 1, T, dtype=torch.int32, device="cuda")
    lengths = torch.empty(B, 1, dtype=torch.int32, device="cuda")
    scores = torch.empty(B, 1, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def beam(log_add):
        _lib.check(L.w2l_ctc_beam_search(B, T, N, x.data_ptr(), None, W, K, float("inf"), log_add, log_add, 1, T, labels.data_ptr(),
                                         lengths.data_ptr(), scores.data_ptr(), wsb.data_ptr(), st), "beam")

    def ctc_score():
        _lib.check(L.w2l_ctc_score(B, T, N, Lt, 0, x.data_ptr(), tgt.data_ptr(), ts.data_ptr(), loss.data_ptr(), greedy.data_ptr(),
                                   wss.data_ptr(), st), "score")

    def timed(fn, n):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    fns = {"ctc_score": (ctc_score, 5 * reps), "beam_logadd": (lambda: beam(1), reps), "beam_max": (lambda: beam(0), reps)}
    t = {k: [] for k in fns}
    for _ in range(2):   # alternate, twice each: a drift of the box shows as a spread between the two runs of one
        for k, (fn, n) in fns.items():
            t[k].append(timed(fn, n))
    # the max search's 1-best is the collapsed greedy path
    beam(0)
    torch.cuda.synchronize()
    gp, lab, ln = greedy.cpu(), labels.cpu(), lengths.cpu()
    for b in range(B):
        want = [int(c) for c in torch.unique_consecutive(gp[b]) if int(c) != N - 1]
        assert int(ln[b, 0]) == len(want) and lab[b, 0, :len(want)].tolist() == want, "1-best of the max search is not the greedy path"
    out = {"B": B, "T": T, "N": N, "W": W, "K": K}
    for k in fns:
        out[k] = {"us": round(min(t[k]), 1), "us_runs": [round(v, 1) for v in t[k]]}
    return out


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    for T in ([int(sys.argv[2])] if len(sys.argv) > 2 else (188, 1500)):   # one T and W: the shape of a kernel trace
        for W in ([int(sys.argv[3])] if len(sys.argv) > 3 else (64, 8)):
            print(json.dumps(bench(T, W, W, reps)), flush=True)
