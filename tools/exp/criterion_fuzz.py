"""Randomised range check of the sequence criteria against the fp64 oracle: FCC / FAC / ASG (loss, dx, dA) and CTC over label-set sizes on
both sides of every kernel switch (N <= 31 / 64 / large), lattice widths, emission and transition magnitudes far outside the recipes'.

Two tiers, decided per case from the scales it drew: tier A (emissions x <= 5 and transitions x <= 2: what a recipe produces) is held to
the project's contract of 1e-4, everything else (the wide tier) to 1e-3.  Every quantity is measured per utterance on that utterance's
own scale (judge()): the loss against max(1, |loss_b|); dx of utterance b against the largest entry of the oracle's dx_b, never less
than 1e-3 w_b s_b -- a posterior of 1e-3 under the utterance's weight w_b and the factor s_b of its scale mode --; dA against the
largest entry of the oracle's dA, never less than 1e-3 max_b(w_b s_b) / N -- one frame's posterior of 1e-3 spread over the N labels it
can come from.  ASG is a difference of two O(1) quantities: its gradients are measured on the larger of the FCC and FAC parts' scales.
Where the oracle's quantity is identically zero (dA at T = 1, a CTC utterance of weight 0) the device's must be exactly zero.
Prints one line per case; `BAD` where the device result is non-finite while the oracle is finite or an error passes the case's bar,
followed by the quantity, the utterance and the tier.
   python tools/exp/criterion_fuzz.py [cases] [seed]

   python tools/exp/criterion_fuzz.py tests            every run of tests/test_gpu_criterion_fuzz.py, one line per case

Worst device error over those runs (MI355X, profiles/criterion_fuzz_tiers.log; loss / dx / dA, `-`: no such quantity):
   tier A (bar 1e-4):  FCC 1.1e-7 / 5.8e-6 / 3.1e-6   FAC 1.7e-6 / 5.5e-6 / 6.6e-6   ASG 1.5e-7 (lossp) / 5.8e-6 / 6.6e-6   CTC 1.7e-7 / 3.7e-6 / -
   wide   (bar 1e-3):  FCC 8.8e-8 / 1.3e-4 / 6.2e-5   FAC 1.5e-6 / 5.3e-6 / 2.8e-6   ASG 2.1e-7 (lossp) / 1.3e-4 / 1.8e-5   CTC 1.3e-6 / 2.4e-5 / -
   ASG loss on the scale of the difference (bar 1e-3 in either tier): 1.1e-5.
Before the backward scans of FCC refreshed their normaliser once per chunk (fcc_bwd_small, fcc_mitm_bwd) tier A read FCC dx 2.7e-4 and
dA 1.6e-4 at 32 <= N <= 64, T = 2000, and dx 1.1e-4 at N = 30, T = 2000."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from oracle import pyoracle as O

TIER_BAR = {"A": 1e-4, "wide": 1e-3}
ALL_N = (3, 5, 16, 29, 30, 31, 32, 33, 40, 64, 65, 100, 1000)
# recipe magnitudes only (every case tier A); shared by the device test and the host test of the fp32 yardstick
RECIPE = dict(x_scales=(0.1, 1.0, 5.0), a_scales=(0.0, 0.3, 2.0), n_choices=ALL_N, big_n_t_cap=50)
RECIPE_SEEDS, RECIPE_CASES = (41, 42), 24
# The class that the fp32 yardstick (tests/criterion_f32_ref.py, tests/test_criterion_f32_ref_host.py) cannot hold to a quarter of the
# contract: the input gradient dx of the lattice criteria (FAC, CTC, and ASG which contains FAC) from 1000 frames on.  A lattice
# position on the posterior path lies hundreds of nats under the frame's best prefix, and an fp32 log-alpha of -500 is known to 3e-5
# only: the yardstick reads 2.5e-4 (FAC, ASG dx) and 1.2e-4 (CTC dx) there, against 1.4e-5 at most below 1000 frames.  Their dA stays
# under the cap at every length and stays in tier A.  The randomised cases hold dx of this class to the wide bar; the deterministic
# cases of the test module (Case.hold_A: loud and quiet emissions at T = 2000) still hold it to 1e-4, which the device meets because
# its lattice scans carry fp64 mantissas (measured 5.5e-6).
LONG_LATTICE_T = 1000


def tier_of(x_scale, a_scale):
    return "A" if x_scale <= 5.0 and a_scale <= 2.0 else "wide"


def scale_factor(mode, T, L):
    """the factor the scale mode applies to an utterance of T frames and L labels (CriterionUtils; oracle: scale_of)"""
    return {0: 1.0, 1: 1.0 / max(T, 1), 2: np.sqrt(1.0 / max(T, 1)), 3: 1.0 / max(L, 1), 4: np.sqrt(1.0 / max(L, 1))}[mode]


class Case:
    def __init__(self, c, x, A, tgt, w, mode, xs, as_, diag, hold_A=False):
        self.hold_A = hold_A   # a tier-A case that keeps every quantity in tier A (the deterministic cases: see quantity_tier)
        self.c, self.x, self.A, self.tgt, self.w, self.mode, self.xs, self.as_, self.diag = c, x, A, tgt, w, mode, xs, as_, diag
        self.B, self.T, self.N = x.shape
        self.tier = tier_of(xs, as_)
        self.bar = TIER_BAR[self.tier]
        self.ts = O.batch_target_size(tgt, self.T)
        # CTC: N includes the blank (last index); targets without the blank
        self.ctc_tgt = np.where(tgt >= 0, np.minimum(tgt, self.N - 2), -1).astype(np.int32)

    def head(self):
        return (f"case {self.c:3d} B={self.B} T={self.T:4d} N={self.N:3d} L<={self.tgt.shape[1]:3d} x*{self.xs:<4} A*{self.as_:<4} "
                f"diag {self.diag} mode {self.mode} tier {self.tier}:")


def draw_cases(cases, seed, x_scales=(0.1, 1.0, 5.0, 20.0, 50.0), a_scales=(0.0, 0.3, 2.0, 8.0, 20.0, 40.0), n_choices=ALL_N,
               big_n_t_cap=300):
    """the fuzz's generator; N >= 500 caps T at big_n_t_cap (the fp64 oracle is N^2 T per utterance on the host)"""
    rng = np.random.default_rng(seed)
    for c in range(cases):
        N = int(rng.choice(n_choices))
        T = int(rng.choice([1, 2, 17, 50, 300, 1000, 2000]))
        if N >= 500:
            T = min(T, big_n_t_cap)
        B = int(rng.integers(1, 4))
        Lmax = int(rng.choice([1, 2, 7, 64, 65, 128, 200, 300]))
        xs = float(rng.choice(x_scales))
        as_ = float(rng.choice(a_scales))
        diag = float(rng.choice([0.0, 4.0]))
        mode = int(rng.choice([0, 1, 2, 3, 4]))
        x = (rng.normal(size=(B, T, N)) * xs).astype(np.float32)
        A = (rng.normal(size=(N, N)) * as_ + np.eye(N) * diag).astype(np.float32)
        tgt = np.full((B, Lmax), -1, np.int32)
        for b in range(B):
            l = int(rng.integers(1, min(Lmax, T) + 1))
            y = rng.integers(0, N, size=l)
            tgt[b, :l] = y
        w = rng.uniform(0.5, 1.5, size=B)
        yield Case(c, x, A, tgt, w, mode, xs, as_, diag)


def fixed_case(N, T, B, Lmax, xs, as_, diag, mode, seed):
    """one deterministic case: every utterance's target as long as Lmax and T allow down to half of that"""
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(B, T, N)) * xs).astype(np.float32)
    A = (rng.normal(size=(N, N)) * as_ + np.eye(N) * diag).astype(np.float32)
    tgt = np.full((B, Lmax), -1, np.int32)
    top = min(Lmax, T)
    for b in range(B):
        l = top if b == 0 else int(rng.integers(max(1, top // 2), top + 1))
        tgt[b, :l] = rng.integers(0, N, size=l)
    w = rng.uniform(0.5, 1.5, size=B)
    return Case(0, x, A, tgt, w, mode, xs, as_, diag, hold_A=True)


def oracle_case(case):
    """-> {criterion: dict(loss [B], dx [B][T][N], dA, w [B], s [B], dx_parts, dA_parts)} from the fp64 oracle, each computed once.
    ASG = FCC - FAC on the same transitions (oracle/pyoracle.py::asg); its *_parts are the two gradients it is the difference of.
    CTC: an utterance the oracle finds infeasible gets weight 0."""
    k, out = case, {}
    s = np.array([scale_factor(k.mode, k.T, int(l)) for l in k.ts])
    fcc = O.FCC(k.x, k.A, k.ts, k.mode)
    fac = O.FAC(k.x, k.A, k.tgt, scale_mode=k.mode)
    for name, o in (("FCC", fcc), ("FAC", fac)):
        loss = o.forward()
        dx, dA = o.backward(k.w)
        out[name] = dict(name=name, loss=loss, dx=dx, dA=dA, w=k.w, s=s)
    a, c = out["FCC"], out["FAC"]
    out["ASG"] = dict(loss_parts=(a["loss"], c["loss"]), loss=a["loss"] - c["loss"], dx=a["dx"] - c["dx"], dA=a["dA"] - c["dA"], w=k.w, s=s, name="ASG",
                      dx_parts=(a["dx"], c["dx"]), dA_parts=(a["dA"], c["dA"]))
    if k.N >= 2 and k.T >= 1:
        o = O.CTC(k.x, k.ctc_tgt, scale_mode=k.mode)
        loss = o.forward()
        wz = np.where(np.isfinite(loss), k.w, 0.0)
        out["CTC"] = dict(name="CTC", loss=loss, dx=o.backward(wz), dA=None, w=wz,
                          s=np.array([scale_factor(k.mode, k.T, int(l)) for l in o.ts]))
    return out


def _err(got, want, floor, parts=None):
    """largest |got - want| over the largest |entry| of want (of either part, for a difference), never less than floor; a want that is
    identically zero asks for a got that is exactly zero"""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    if not np.isfinite(got).all():
        return np.inf
    if not want.any() and (parts is None or not any(p.any() for p in parts)):
        return 0.0 if not got.any() else np.inf
    scale = max([floor, np.abs(want).max()] + [np.abs(p).max() for p in (parts or ())])
    return float(np.abs(got - want).max() / scale)


def quantity_tier(case, name, quantity):
    """the tier one quantity of one criterion is held to.  A wide case is wide throughout.  In a tier-A case dx of the lattice
    criteria (FAC, CTC, and ASG which contains FAC) leaves tier A from LONG_LATTICE_T frames on: see LONG_LATTICE_T."""
    if case.tier == "A" and name in ("FAC", "ASG", "CTC") and quantity == "dx" and case.T >= LONG_LATTICE_T and not case.hold_A:
        return "wide"
    return case.tier


def judge(case, ref, loss, dx, dA=None):
    """-> {quantity: (error, utterance, tier, bar)}: the worst utterance of each quantity of one criterion against ref =
    oracle_case(case)[name]; utterance -1: the batch as a whole (dA).  Utterances whose oracle loss is not finite are left out of the
    loss (CTC: infeasible; the caller compares the pattern) but not of dx.
    ASG's loss is a difference as well and is measured twice: `loss` against max(1, |loss_b|) at 1e-3 in either tier -- an fp32 FCC
    loss of 8000 is only known to 5e-4, whatever it is subtracted from -- and `lossp` against the larger of the two parts' losses
    at the bar of the tier."""
    B, N, name = case.B, case.N, ref["name"]
    fin = np.isfinite(ref["loss"])
    loss = np.asarray(loss, np.float64)
    d = np.array([(abs(loss[b] - ref["loss"][b]) if np.isfinite(loss[b]) else np.inf) if fin[b] else 0.0 for b in range(B)])
    el = d / np.maximum(1.0, np.abs(np.where(fin, ref["loss"], 0.0)))
    out = {"loss": (float(el.max()), int(el.argmax()))}
    if "loss_parts" in ref:
        ep = d / np.maximum(1.0, np.maximum(*[np.abs(p) for p in ref["loss_parts"]]))
        out["lossp"] = (float(ep.max()), int(ep.argmax()))
    parts = ref.get("dx_parts")
    ex = np.array([_err(dx[b], ref["dx"][b], 1e-3 * ref["w"][b] * ref["s"][b], None if parts is None else [p[b] for p in parts])
                   for b in range(B)])
    out["dx"] = (float(ex.max()), int(ex.argmax()))
    if ref["dA"] is not None:
        out["dA"] = (_err(dA, ref["dA"], 1e-3 * float((ref["w"] * ref["s"]).max()) / N, ref.get("dA_parts")), -1)
    full = {}
    for q, (e, b) in out.items():
        tier = quantity_tier(case, name, q)
        full[q] = (e, b, tier, TIER_BAR["wide"] if (name, q) == ("ASG", "loss") else TIER_BAR[tier])
    return full


def verdict(case, name, errs, worst=None, extra_bad=""):
    """the piece of the case's line for one criterion; fills worst[(tier, criterion, quantity)]"""
    if worst is not None:
        for q, (e, _, tier, _) in errs.items():
            worst[(tier, name, q)] = max(worst.get((tier, name, q), 0.0), e)
    over = [f"{q}[{'batch' if b < 0 else b}]={e:.1e}>{bar:g} tier {tier}" for q, (e, b, tier, bar) in errs.items() if not e < bar]
    over += [extra_bad.strip()] if extra_bad else []
    text = f" {name} " + "/".join(f"{e:.1e}" for e, *_ in errs.values())
    if over:
        text += f" BAD({', '.join(over)})"
    return text


def run_case(case, worst=None):
    """one case on the device against the oracle -> its line (holds `BAD` where something is off)"""
    import torch
    from wav2letter_amd import ASGLoss, CTCLoss, ForceAlignmentCriterion, FullConnectionCriterion
    k = case
    x, A, tgt, w, N, mode = k.x, k.A, k.tgt, k.w, k.N, k.mode
    ref = oracle_case(k)
    line = k.head()
    for name, cls in (("FCC", FullConnectionCriterion), ("FAC", ForceAlignmentCriterion),
                      ("ASG", lambda n_, m_: ASGLoss(n_, m_, 0.0))):   # ASGLoss: w2l_asg_forward / w2l_asg_backward (N <= 31: the fused sequence)
        crit = cls(N, mode).cuda()
        crit.transitions.data = torch.from_numpy(A).cuda()
        xt = torch.from_numpy(x).cuda().requires_grad_(True)
        loss = crit(xt, torch.from_numpy(tgt).cuda())
        (loss * torch.from_numpy(w.astype(np.float32)).cuda()).sum().backward()
        r = ref[name]
        if not np.isfinite(r["loss"]).all():
            line += f" {name} oracle-nonfinite"
            continue
        errs = judge(k, r, loss.detach().cpu().numpy(), xt.grad.cpu().numpy(), crit.transitions.grad.cpu().numpy())
        line += verdict(k, name, errs, worst)
    # Viterbi paths: bit-exact (the free path of ASGLoss::viterbiPath and the forced alignment)
    asg = ASGLoss(N, mode, 0.0).cuda()
    asg.transitions.data = torch.from_numpy(A).cuda()
    vp = asg.viterbiPath(torch.from_numpy(x).cuda()).cpu().numpy()
    okv = bool((vp == O.viterbi(x, A)).all())
    fac = ForceAlignmentCriterion(N, mode).cuda()
    fac.transitions.data = torch.from_numpy(A).cuda()
    fp = fac.viterbiPath(torch.from_numpy(x).cuda(), torch.from_numpy(tgt).cuda()).cpu().numpy()
    okf_ = bool((fp == O.FAC(x, A, tgt, scale_mode=mode).viterbi()).all())
    if not (okv and okf_):
        line += f" VITERBI free {okv} forced {okf_} BAD"
    if "CTC" in ref:
        r = ref["CTC"]
        okf = np.isfinite(r["loss"])
        if okf.any():
            crit = CTCLoss(mode)
            xt = torch.from_numpy(x).cuda().requires_grad_(True)
            loss = crit(xt, torch.from_numpy(k.ctc_tgt).cuda())
            fin = torch.isfinite(loss)
            (torch.where(fin, loss, torch.zeros_like(loss)) * torch.from_numpy(r["w"].astype(np.float32)).cuda()).sum().backward()
            got = loss.detach().cpu().numpy().astype(np.float64)
            same_inf = bool((np.isfinite(got) == okf).all())
            errs = judge(k, r, got, xt.grad.cpu().numpy())
            line += verdict(k, "CTC", errs, worst, "" if same_inf else " inf-mismatch")
        else:
            line += " CTC all-infeasible"
    return line


def run(cases, seed, x_scales=(0.1, 1.0, 5.0, 20.0, 50.0), a_scales=(0.0, 0.3, 2.0, 8.0, 20.0, 40.0), verbose=True,
        n_choices=ALL_N, big_n_t_cap=300, worst=None):
    """-> the lines of the cases whose device result is non-finite where the oracle's is finite, or off by more than the bar of the
    case's tier; worst, if given, is filled with the largest error per (tier, criterion, quantity)"""
    bad_lines = []
    for case in draw_cases(cases, seed, x_scales, a_scales, n_choices, big_n_t_cap):
        line = run_case(case, worst)
        if verbose:
            print(line, flush=True)
        if 'BAD' in line:
            bad_lines.append(line)
    return bad_lines


def worst_lines(worst):
    return [f"worst tier {t:4s} {n} {q:4s} {e:.1e}" for (t, n, q), e in sorted(worst.items())]


# the runs of tests/test_gpu_criterion_fuzz.py: (cases, seed, arguments of run())
TEST_RUNS = [(40, 11, dict(x_scales=(0.1, 1.0, 5.0, 20.0), a_scales=(0.0, 0.3, 2.0, 8.0))),
             (40, 12, dict(x_scales=(0.1, 1.0, 5.0, 20.0), a_scales=(0.0, 0.3, 2.0, 8.0))),
             (RECIPE_CASES, RECIPE_SEEDS[0], RECIPE), (RECIPE_CASES, RECIPE_SEEDS[1], RECIPE),
             (30, 9, dict(x_scales=(5.0, 20.0, 50.0), a_scales=(8.0, 20.0, 40.0))),
             (30, 21, dict(x_scales=(5.0, 20.0, 50.0), a_scales=(8.0, 20.0, 40.0))),
             (30, 7, dict(x_scales=(1.0, 20.0, 50.0), a_scales=(20.0, 40.0)))]
# N, T, emission scale of the deterministic cases: B = 2, L <= 300, A * 2, diagonal 4, every mode.  x * 5: one per scan family at its
# longest T; x * 0.1: quiet emissions under loud transitions, where a scan's rounding repeats frame after frame (what showed the FCC
# normaliser's drift), on the two families that run 2000 frames
FIXED_RUNS = [(30, 2000, 5.0), (64, 2000, 5.0), (100, 300, 5.0), (30, 2000, 0.1), (64, 2000, 0.1)]


def fixed_cases(N, T, xs=5.0):
    return [fixed_case(N, T, 2, 300, xs, 2.0, 4.0, mode, seed=1000 + N) for mode in range(5)]


if __name__ == "__main__":
    if sys.argv[1:2] == ["tests"]:   # the verbose log of every run of the test module (profiles/criterion_fuzz_tiers.log)
        worst, nbad = {}, 0
        for n, seed, kw in TEST_RUNS:
            print(f"== run({n}, {seed}, {kw})")
            nbad += len(run(n, seed, worst=worst, **kw))
        for N, T, xs in FIXED_RUNS:
            print(f"== fixed_cases({N}, {T}, {xs})")
            for case in fixed_cases(N, T, xs):
                line = run_case(case, worst)
                nbad += "BAD" in line
                print(line, flush=True)
        print("\n".join(worst_lines(worst)))
        print(f"{nbad} BAD lines")
        sys.exit(1 if nbad else 0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
    worst = {}
    lines = run(n, int(sys.argv[2]) if len(sys.argv) > 2 else 5, worst=worst)
    print("\n".join(worst_lines(worst)))
    print(f"{len(lines)} BAD of {n} cases")
