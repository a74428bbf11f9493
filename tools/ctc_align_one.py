"""w2l_ctc_align with and without the score, and w2l_ctc_score at the same shape in the same process, timed with hip events after
warm-up at the criterion shapes of the TDS-CTC recipe:   python tools/ctc_align_one.py [reps] [T]
  B = 32, T = 188,  N = 9998, L <= 80   (config 2)
  B = 32, T = 1500, N = 9998, L <= 80
w2l_ctc_score is the yardstick: it reads the same rows and scans a lattice of the same length.  With the score the alignment adds the
back-pointer walk to a row pass and a scan; without it the row pass disappears (only the L_b + 1 label emissions of a frame are
read).  Prints microseconds per call, one JSON line per shape; a kernel trace (rocprofv3 --kernel-trace --stats, a run of its own)
splits a call into ctc_rows_lse_only / ctc_align_scan / ctc_align_walk / ctc_align_finish."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from wav2letter_amd import _lib, criterion as Cr


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
    wsa = torch.empty(L.w2l_ctc_align_workspace_size(B, T, N, Lt), dtype=torch.uint8, device="cuda")
    wss = torch.empty(L.w2l_ctc_score_workspace_size(B, T, N, Lt), dtype=torch.uint8, device="cuda")
    loss, score = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    greedy = torch.empty(B, T, dtype=torch.int32, device="cuda")
    path, path2 = torch.empty_like(greedy), torch.empty_like(greedy)
    st = torch.cuda.current_stream().cuda_stream

    def align_score():
        _lib.check(L.w2l_ctc_align(B, T, N, Lt, x.data_ptr(), tgt.data_ptr(), ts.data_ptr(), None, path.data_ptr(), score.data_ptr(),
                                   wsa.data_ptr(), st), "align")

    def align_path():
        _lib.check(L.w2l_ctc_align(B, T, N, Lt, x.data_ptr(), tgt.data_ptr(), ts.data_ptr(), None, path2.data_ptr(), None,
                                   wsa.data_ptr(), st), "align")

    def ctc_score():
        _lib.check(L.w2l_ctc_score(B, T, N, Lt, 0, x.data_ptr(), tgt.data_ptr(), ts.data_ptr(), loss.data_ptr(), greedy.data_ptr(),
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

    fns = {"ctc_score": ctc_score, "align+score": align_score, "align": align_path}
    t = {k: [] for k in fns}
    for _ in range(2):   # alternate, twice each: a drift of the box shows as a spread between the two runs of one
        for k, fn in fns.items():
            t[k].append(timed(fn))
    assert torch.equal(path, path2), "the path depends on whether the score is asked for"
    assert bool((score <= -loss + 1e-4 * loss.abs().clamp(min=1)).all()), "a path likelier than the sum over paths"
    out = {"B": B, "T": T, "N": N, "L": Lt}
    for k in fns:
        out[k] = {"us": round(min(t[k]), 1), "us_runs": [round(v, 1) for v in t[k]]}
    return out


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    for T in ([int(sys.argv[2])] if len(sys.argv) > 2 else (188, 1500)):   # one T: the shape of a kernel trace
        print(json.dumps(bench(T, reps)))
