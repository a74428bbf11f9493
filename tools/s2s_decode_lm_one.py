"""The LM-fused seq2seq decoder against the LM-free one, the whole search, alternating in one process:
  free         ops.s2s_decode without an LM (w2l_s2s_decode);
  lm           ops.s2s_decode with a synthetic 3-gram LM of about 10^5 n-grams over the 9998 classes (w2l_s2s_decode_lm), lm_weight 1.158:
               every class has a unigram, the 2- and 3-grams are drawn at random, so most lookups walk the full back-off chain;
  lm_zero      the same with lm_weight 0: the LM-free search's decisions with the LM kernels' work, and a check that its tokens, lengths
               and scores are the LM-free bits;
  free_again   a second series of `free`, whose distance from the first is the spread to hold every difference against;
  parent       with --parent LIB: w2l_s2s_decode of another build of libw2l_hip.so (the parent commit's) on the same operands, against
               `free`; its results are compared bit for bit.
Shapes: the cells of tools/s2s_decode_one.py (H = 512, N = 9998, beam 80, 10 tokens per hypothesis, 120 steps, no eos score so that
the search runs its length), T in 188 and 440, B in 1 and 16.  Each figure is the median of `windows` timings between two events.
  python tools/s2s_decode_lm_one.py [--parent LIB] [windows [B T]]"""
import ctypes as C
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from tools.s2s_decode_one import medians
from wav2letter_amd import NGramLM, Seq2SeqCriterion, ops


def synthetic_lm(N, n2, n3, seed):
    """every class, BOS (N) and EOS (N + 1) as unigrams; n2 distinct 2-grams (BOS or a class, then a class); n3 distinct 3-grams, each
    a listed 2-gram and one more class"""
    rng = np.random.default_rng(seed)
    val = lambda n, lo, hi: rng.uniform(lo, hi, n).astype(np.float32)
    two = np.unique(np.stack([rng.integers(0, N + 1, 2 * n2), rng.integers(0, N, 2 * n2)], 1), axis=0)
    two = two[rng.permutation(len(two))[:n2]]
    three = np.unique(np.concatenate([two[rng.integers(0, len(two), 2 * n3)], rng.integers(0, N, (2 * n3, 1))], 1), axis=0)
    three = three[rng.permutation(len(three))[:n3]]
    return NGramLM.from_ngrams([(np.arange(N + 2).reshape(-1, 1), val(N + 2, -10, -3), val(N + 2, -1, 0)),
                                (two, val(len(two), -6, -1), val(len(two), -1, 0)), (three, val(len(three), -4, -0.5), None)], N, -12.0)


def parent_call(path, params, enc, kl, opt):
    """w2l_s2s_decode of the library at `path` on the same operands -> (the call, its three result tensors)"""
    L = C.CDLL(path)
    L.w2l_s2s_decode_workspace_size.restype, L.w2l_s2s_decode_workspace_size.argtypes = C.c_size_t, [C.c_void_p]
    L.w2l_s2s_decode.restype, L.w2l_s2s_decode.argtypes = C.c_int, [C.c_void_p] * 13 + [C.c_size_t, C.c_void_p]
    d, klh, keep, ptrs = ops._s2s_decode_operands("parent", params, enc, kl, True, opt["beam"], opt["beam_token"], opt["max_len"], 1, opt["eos"],
                                                  opt["threshold"], 0.0, None, 1.0)
    nbytes = L.w2l_s2s_decode_workspace_size(C.byref(d))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = [torch.empty(d.B, 1, d.maxLen, dtype=torch.int32, device="cuda"), torch.empty(d.B, 1, dtype=torch.int32, device="cuda"),
           torch.empty(d.B, 1, device="cuda")]

    def call(hold=(klh, keep)):
        st = L.w2l_s2s_decode(C.byref(d), *ptrs, *[t.data_ptr() for t in out], ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
    return call, out


def one(B, T, H, N, beam, bt, max_len, threshold, windows, lm, parent):
    torch.manual_seed(1)
    eos = N - 1
    crit = Seq2SeqCriterion(N, H, eos, "keyvalue").cuda().eval()
    params = [p.detach() for p in (crit.embedding, crit.start, crit.rnn, crit.linear_weight, crit.linear_bias)]
    enc = torch.randn(B, T, 2 * H, device="cuda")
    kl = np.random.default_rng(1).integers(T // 2, T + 1, B).astype(np.int32)
    kl[0] = T
    opt = dict(eos=eos, beam=beam, beam_token=bt, threshold=threshold, max_len=max_len)
    dec = lambda **k: ops.s2s_decode(params, enc, kl, True, nbest=1, **opt, **k)
    fns = {"free": dec, "lm": lambda: dec(lm=lm, lm_weight=1.158), "lm_zero": lambda: dec(lm=lm, lm_weight=0.0), "free_again": dec}
    if parent:
        fns["parent"], parent_out = parent_call(parent, params, enc, kl, opt)
    m = medians(fns, windows)
    free, zero, fused = dec(), dec(lm=lm, lm_weight=0.0), dec(lm=lm, lm_weight=1.158)
    out = {"B": B, "T": T, "H": H, "N": N, "beam": beam, "beam_token": bt, "max_len": max_len, "windows": windows, **m,
           "lm_over_free": round(m["lm_us"] / m["free_us"], 3), "lm_zero_over_free": round(m["lm_zero_us"] / m["free_us"], 3),
           "free_again_over_free": round(m["free_again_us"] / m["free_us"], 3),
           "lm_extra_per_step_us": round((m["lm_us"] - m["free_us"]) / max_len, 2),
           "lm_zero_is_free_bitwise": all(torch.equal(a, b) for a, b in zip(zero[:3], free)),
           "fused_1best_differs": not torch.equal(fused[0], free[0]), "decoded_len_max": int(fused[1].max())}
    if parent:
        torch.cuda.synchronize()
        out["parent_over_free"] = round(m["parent_us"] / m["free_us"], 3)
        out["parent_is_free_bitwise"] = all(torch.equal(a, b) for a, b in zip(parent_out, free))
    print("[s2s_decode_lm] " + json.dumps(out), flush=True)


if __name__ == "__main__":
    argv = sys.argv[1:]
    parent = argv.pop(argv.index("--parent") + 1) if "--parent" in argv else None
    argv = [a for a in argv if a != "--parent"]
    windows = int(argv[0]) if argv else 7
    cells = [tuple(int(x) for x in argv[1:3])] if len(argv) > 2 else [(B, T) for B in (1, 16) for T in (188, 440)]
    lm = synthetic_lm(9998, 45000, 45000, 1)
    print(f"[s2s_decode_lm] LM: order {lm.order}, {lm.num_states} states, blob {lm.blob.nbytes} bytes, eos {lm.has_eos}", flush=True)
    for B, T in cells:
        one(B, T, 512, 9998, 80, 10, 120, 7.0, windows, lm, parent)
