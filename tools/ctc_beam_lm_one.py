"""w2l_ctc_beam_search_lm against w2l_ctc_beam_search on the same inputs in the same process, timed with hip events after warm-up
at the criterion shapes of the TDS-CTC recipe:   python tools/ctc_beam_lm_one.py [reps] [T] [W]
  B = 32, T = 188 and 1500, N = 9998, (W, K) = (64, 64) and (8, 8), max search on the raw emissions, no threshold, nbest = 1
The LM is a random 3-gram model of about 10^5 n-grams over the 9997 tokens: every unigram, BOS and EOS, 45000 bigrams and 45000
trigrams over the 2048 classes the emissions favour (+2 on those classes, so that frame tokens meet listed contexts as well as
unlisted ones and queries end at every depth of the back-off walk).  lmWeight = 0.5.
A/B for where the time goes: the same call with a unigram-only model of the same tokens (`beam_lm_unigram_max`: one table, every
query one probe chain from state 0 and no back-off walk -- the least a lookup can cost) keeps the selection as it is; what the
3-gram model adds to it is the cost of the longer lookup chains, what it adds to the LM-free search is candidates plus selection.
Prints microseconds per call, one JSON line per shape, with the ratio and the difference per frame; a kernel trace (rocprofv3
--kernel-trace --stats, a run of its own with one T and W) splits a call into ctc_beam_rows / ctc_beam_lm_scan /
ctc_beam_lm_finish and the clearing of the prefix table."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from wav2letter_amd import NGramLM, _lib

HOT = 2048


def model(V, rng, pairs=45000, triples=45000):
    uni = np.arange(V + 2, dtype=np.int32).reshape(-1, 1)
    two = np.unique(rng.integers(0, HOT, size=(pairs, 2)).astype(np.int32), axis=0)
    ctx = two[rng.integers(0, len(two), size=triples)]
    three = np.unique(np.concatenate([ctx, rng.integers(0, HOT, size=(triples, 1)).astype(np.int32)], axis=1), axis=0)

    def vals(n, lo, hi):
        return rng.uniform(lo, hi, n).astype(np.float32)
    return NGramLM.from_ngrams([(uni, vals(len(uni), -9, -5), vals(len(uni), -1, 0)), (two, vals(len(two), -4, -1), vals(len(two), -1, 0)),
                                (three, vals(len(three), -3, -0.5), None)], V, -12.0), len(uni) + len(two) + len(three)


def unigram_model(V, rng):
    uni = np.arange(V + 2, dtype=np.int32).reshape(-1, 1)
    return NGramLM.from_ngrams([(uni, rng.uniform(-9, -5, len(uni)).astype(np.float32), None)], V, -12.0)


def bench(T, W, K, reps, lm, lm1, B=32, N=9998):
    L = _lib.lib()
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(B, T, N, generator=g)
    x[:, :, :HOT] += 2.0
    x = x.cuda()
    wsb = torch.empty(L.w2l_ctc_beam_workspace_size(B, T, N, W, K), dtype=torch.uint8, device="cuda")
    wsl = torch.empty(L.w2l_ctc_beam_lm_workspace_size(B, T, N, W, K), dtype=torch.uint8, device="cuda")
    labels = torch.empty(B, 1, T, dtype=torch.int32, device="cuda")
    lengths = torch.empty(B, 1, dtype=torch.int32, device="cuda")
    scores = torch.empty(B, 1, device="cuda")
    lms = torch.empty(B, 1, device="cuda")
    blob, blob1 = lm.device_blob("cuda"), lm1.device_blob("cuda")
    st = torch.cuda.current_stream().cuda_stream

    def free():
        _lib.check(L.w2l_ctc_beam_search(B, T, N, x.data_ptr(), None, W, K, float("inf"), 0, 0, 1, T, labels.data_ptr(),
                                         lengths.data_ptr(), scores.data_ptr(), wsb.data_ptr(), st), "beam")

    def fused(weight=0.5):
        _lib.check(L.w2l_ctc_beam_search_lm(B, T, N, x.data_ptr(), None, W, K, float("inf"), 0, 0, 1, T, blob.data_ptr(),
                                            int(lm.has_eos), weight, None, 0.0, labels.data_ptr(), lengths.data_ptr(),
                                            scores.data_ptr(), lms.data_ptr(), wsl.data_ptr(), st), "beam lm")

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

    def fused1():
        _lib.check(L.w2l_ctc_beam_search_lm(B, T, N, x.data_ptr(), None, W, K, float("inf"), 0, 0, 1, T, blob1.data_ptr(),
                                            int(lm1.has_eos), 0.5, None, 0.0, labels.data_ptr(), lengths.data_ptr(),
                                            scores.data_ptr(), lms.data_ptr(), wsl.data_ptr(), st), "beam lm unigram")

    fns = {"beam_max": free, "beam_lm_max": fused, "beam_lm_unigram_max": fused1}
    t = {k: [] for k in fns}
    for _ in range(2):   # alternate, twice each: a drift of the box shows as a spread between the two runs of one
        for k, fn in fns.items():
            t[k].append(timed(fn, reps))
    # lmWeight = 0 is the LM-free search
    free()
    torch.cuda.synchronize()
    want = (labels.cpu().clone(), lengths.cpu().clone(), scores.cpu().clone())
    fused(0.0)
    torch.cuda.synchronize()
    assert (labels.cpu() == want[0]).all() and (lengths.cpu() == want[1]).all() and (scores.cpu() == want[2]).all(), \
        "the fused search at lmWeight = 0 is not the LM-free search"
    out = {"B": B, "T": T, "N": N, "W": W, "K": K}
    for k in fns:
        out[k] = {"us": round(min(t[k]), 1), "us_runs": [round(v, 1) for v in t[k]]}
    out["ratio"] = round(out["beam_lm_max"]["us"] / out["beam_max"]["us"], 2)
    out["extra_us_per_frame"] = round((out["beam_lm_max"]["us"] - out["beam_max"]["us"]) / T, 2)
    out["longer_lookups_us_per_frame"] = round((out["beam_lm_max"]["us"] - out["beam_lm_unigram_max"]["us"]) / T, 2)
    return out


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    lm, count = model(9997, np.random.default_rng(3))
    lm1 = unigram_model(9997, np.random.default_rng(4))
    print(json.dumps({"lm_order": lm.order, "ngrams": count, "states": lm.num_states, "blob_bytes": int(lm.blob.nbytes)}), flush=True)
    for T in ([int(sys.argv[2])] if len(sys.argv) > 2 else (188, 1500)):   # one T and W: the shape of a kernel trace
        for W in ([int(sys.argv[3])] if len(sys.argv) > 3 else (64, 8)):
            print(json.dumps(bench(T, W, W, reps, lm, lm1)), flush=True)
