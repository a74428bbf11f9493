"""The seq2seq decoder against what a user could write before it, alternating in one process:
  decode       ops.s2s_decode, the whole search, against a torch composition of the same search that stays on the device: index_select
               of the parents' states, the GRU cell as two matmuls, bmm + mask + softmax + bmm attention, matmul, log_softmax, topk per
               row, topk per utterance with the beam threshold, gather of the survivors.  The composition keeps no completed pool and
               no trace table (it does less than the decoder), and never reads anything back;
  step         ops.s2s_decode_step: the cell, attention, vocabulary and merge launches of one step at full beam.
Shapes: the seq2seq_tds recipe's decoder (H = 512, N = 9998, beam 80, 10 tokens per hypothesis, 120 steps, no eos score so that the
search runs its length), T in 188 and 440, B in 1 and 16.  Each figure is the median of `windows` timings between two events;
`*_again` is a second series of the composition, whose distance from the first is the spread to hold every ratio against.
  python tools/s2s_decode_one.py [windows [B T]]
The time of each kernel of a step comes from a kernel trace of one cell in a run of its own (three searches and two step entries):
  tools/prof.sh s2s_decode_1_188 tools/s2s_decode_one.py 1 1 188"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from wav2letter_amd import Seq2SeqCriterion, ops


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3   # us


def medians(fns, windows):
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():
            t[k].append(timed(f))
    return {k + "_us": round(statistics.median(v), 1) for k, v in t.items()}


def one(B, T, H, N, beam, bt, max_len, threshold, windows):
    torch.manual_seed(1)
    eos = N - 1
    crit = Seq2SeqCriterion(N, H, eos, "keyvalue").cuda().eval()
    params = [p.detach() for p in (crit.embedding, crit.start, crit.rnn, crit.linear_weight, crit.linear_bias)]
    E, start, rnn, W, bias = params
    enc = torch.randn(B, T, 2 * H, device="cuda")
    kl = np.random.default_rng(1).integers(T // 2, T + 1, B).astype(np.int32)
    kl[0] = T
    wih, whh, bih, bhh = rnn[:3 * H * H].view(3 * H, H), rnn[3 * H * H:6 * H * H].view(3 * H, H), rnn[6 * H * H:6 * H * H + 3 * H], rnn[6 * H * H + 3 * H:]
    Es = torch.cat([E, start[None]])
    keys, vals = enc[..., :H].transpose(1, 2).contiguous(), enc[..., H:].contiguous()
    mask = (torch.arange(T, device="cuda")[None, None, :] >= torch.tensor(kl, device="cuda")[:, None, None])
    base = (torch.arange(B, device="cuda") * beam)[:, None]

    def comp():
        R = B * beam
        h = torch.zeros(R, H, device="cuda")
        tok = torch.full((R,), N, device="cuda", dtype=torch.long)
        par = base.expand(B, beam).reshape(-1)
        score = torch.full((B, beam), float("-inf"), device="cuda")
        score[:, 0] = 0
        for _ in range(max_len):
            hp, x = h.index_select(0, par), Es.index_select(0, tok)
            gi, gh = x @ wih.T + bih, hp @ whh.T + bhh
            r, z = torch.sigmoid(gi[:, :H] + gh[:, :H]), torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
            h = (1 - z) * torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:]) + z * hp
            q = h.view(B, beam, H)
            o = q + torch.bmm(torch.softmax((torch.bmm(q, keys) / H ** 0.5).masked_fill(mask, float("-inf")), 2), vals)
            v, t = torch.log_softmax(o.view(R, H) @ W + bias, 1).topk(bt, 1)
            cand = (score.view(R, 1) + v).view(B, beam * bt)
            score, at = cand.topk(beam, 1)
            score = score.masked_fill(score < score[:, :1] - threshold, float("-inf"))
            par, tok = (base + at // bt).reshape(-1), t.view(B, beam * bt).gather(1, at).reshape(-1)
        return score

    dec = lambda: ops.s2s_decode(params, enc, kl, True, eos=eos, beam=beam, beam_token=bt, threshold=threshold, max_len=max_len, nbest=1)
    parent = np.tile(np.arange(beam)[::-1], (B, 1))
    token, hprev = np.random.default_rng(2).integers(0, N, (B, beam)), torch.randn(B, beam, H, device="cuda") * 0.3
    step = lambda: ops.s2s_decode_step(params, enc, parent, token, hprev, kl, True, beam=beam, beam_token=bt)
    m = medians({"decode": dec, "comp": comp, "comp_again": comp, "step_entry": step}, windows)
    lengths = dec()[1]
    out = {"B": B, "T": T, "H": H, "N": N, "beam": beam, "beam_token": bt, "max_len": max_len, "windows": windows, **m,
           "decoded_len_max": int(lengths.max()), "decode_per_step_us": round(m["decode_us"] / max_len, 1),
           "comp_over_decode": round(m["comp_us"] / m["decode_us"], 2)}
    print("[s2s_decode] " + json.dumps(out), flush=True)


if __name__ == "__main__":
    windows = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    cells = [tuple(int(x) for x in sys.argv[2:4])] if len(sys.argv) > 3 else [(B, T) for B in (1, 16) for T in (188, 440)]
    for B, T in cells:
        one(B, T, 512, 9998, 80, 10, 120, 7.0, windows)
