"""The fp32 yardstick of the sequence criteria (tests/criterion_f32_ref.py) without a GPU: its float64 instantiation IS the C oracle
(1e-10), so it is no third opinion; its float32 instantiation, on the very cases the device's tier-A fuzz draws
(tools/exp/criterion_fuzz.py::RECIPE), stays within a quarter of the device's bar of 1e-4.  That cap is a condition on the inputs and
on the yardstick -- it shows that fp32 itself can hold the contract at recipe magnitudes -- and no tolerance for a kernel.

Two classes of tier-A quantities exceed the cap on a correct fp32 evaluation and are taken out of tier A, not given a wider cap:
 * the input gradient dx of the lattice criteria (FAC, CTC, ASG) from 1000 frames on -- criterion_fuzz.LONG_LATTICE_T: 2.5e-4
   (FAC / ASG dx), 1.2e-4 (CTC dx); an fp32 log-alpha hundreds of nats under the frame's best is only known to 3e-5.  Their dA
   stays in tier A at every length (worst 2.2e-5, FAC / ASG at T = 2000);
 * the ASG loss on the scale of the difference FCC - FAC: 3.6e-4 (two losses of 8000 that differ by a few nats; fp32 knows each to
   5e-4).  It keeps the 1e-3 it had, and tier A holds the ASG loss on the scale of its parts instead (`lossp`: 2.5e-6)."""
import numpy as np
import pytest

import criterion_f32_ref as R
from oracle import pyoracle as O
from tools.exp import criterion_fuzz as F

YARDSTICK_CAP = 2.5e-5


def close(got, want, tol=1e-10):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert (np.isfinite(got) == np.isfinite(want)).all(), (got, want)
    fin = np.isfinite(want)
    if fin.any():
        assert np.abs(got[fin] - want[fin]).max() <= tol * max(np.abs(want[fin]).max(), 1e-300), np.abs(got[fin] - want[fin]).max()
    assert (got[~fin] == want[~fin]).all()


def small_problem(seed, B, T, N, L, x_scale=1.0, a_scale=0.5):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(B, T, N)) * x_scale).astype(np.float32)
    A = (rng.normal(size=(N, N)) * a_scale + np.eye(N)).astype(np.float32)
    tgt = np.full((B, L), -1, np.int32)
    for b in range(B):
        l = int(rng.integers(1, L + 1))
        tgt[b, :l] = rng.integers(0, min(N - 1, 3), size=l)     # few distinct labels: repeats in most targets
    w = rng.uniform(0.5, 1.5, size=B)
    return x, A, tgt, w


SHAPES = [(3, 9, 5, 4), (2, 1, 4, 1), (2, 2, 3, 3), (3, 23, 7, 30), (2, 40, 33, 12)]   # L > T: targets clamped (ASG) / truncated (CTC)


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_float64_instantiation_equals_the_oracle(shape, mode):
    """FCC, FAC, ASG and CTC: loss, dx and dA at 1e-10 of the largest entry, every scale mode, weights in 0.5 .. 1.5"""
    B, T, N, L = shape
    x, A, tgt, w = small_problem(100 + T, B, T, N, L, x_scale=2.0)
    ts = O.batch_target_size(tgt, T)
    o = O.FCC(x, A, ts, mode)
    want = (o.forward(),) + o.backward(w)
    for g, v in zip(R.fcc(x, A, ts, mode, w), want):
        close(g, v)
    o = O.FAC(x, A, tgt, scale_mode=mode)
    want = (o.forward(),) + o.backward(w)
    for g, v in zip(R.fac(x, A, tgt, mode, w), want):
        close(g, v)
    # ASG against the oracle's composition: on the scale of the parts (the difference of two sums that agree to 1e-10 of themselves)
    part = O.FCC(x, A, ts, mode)
    part = (part.forward(),) + part.backward(w)
    for g, v, p in zip(R.asg(x, A, tgt, mode, w), O.asg(x, A, tgt, mode, w), part):
        assert np.abs(g - v).max() <= 1e-10 * np.abs(p).max()
    o = O.CTC(x, tgt, scale_mode=mode)
    loss, dx = R.ctc(x, tgt, None, mode, w)
    close(loss, o.forward())
    close(dx, o.backward(w))
    assert (np.array([R.ctc_target_size(r, T) for r in tgt]) == o.ts).all()


def test_ctc_without_a_path_is_plus_infinity_and_its_gradient_the_softmax():
    """three equal labels need five frames; handed their full length with T = 3 (and next to a feasible utterance) the loss is +inf
    and the gradient the weighted softmax, as the oracle has it"""
    x, _, _, w = small_problem(5, 2, 3, 4, 3)
    tgt = np.array([[1, 1, 1], [0, 1, -1]], np.int32)
    ts = np.array([3, 2], np.int32)
    o = O.CTC(x, tgt, target_size=ts, scale_mode=4)
    want = o.forward()
    assert np.isposinf(want[0]) and np.isfinite(want[1])
    for dtype in (np.float64, np.float32):
        loss, dx = R.ctc(x, tgt, ts, 4, w, dtype=dtype)
        tol = 1e-10 if dtype is np.float64 else 1e-6
        close(loss, want, tol)
        close(dx, o.backward(w), tol)


def yardstick_errors(case, dtype=np.float32):
    """{(criterion, quantity): error}: the yardstick in dtype against the fp64 oracle, judged as the device is (criterion_fuzz.judge)"""
    ref = F.oracle_case(case)
    k = case
    got = {"FCC": R.fcc(k.x, k.A, k.ts, k.mode, k.w, dtype), "FAC": R.fac(k.x, k.A, k.tgt, k.mode, k.w, dtype),
           "ASG": R.asg(k.x, k.A, k.tgt, k.mode, k.w, dtype)}
    if "CTC" in ref:
        got["CTC"] = R.ctc(k.x, k.ctc_tgt, None, k.mode, ref["CTC"]["w"], dtype)
        assert (np.isfinite(got["CTC"][0]) == np.isfinite(ref["CTC"]["loss"])).all()
    out = {}
    for name, g in got.items():
        assert np.isfinite(ref[name]["loss"]).all() or name == "CTC"
        for q, v in F.judge(k, ref[name], *g).items():
            out[(name, q)] = v
    return out


@pytest.mark.parametrize("seed", F.RECIPE_SEEDS)
def test_float32_instantiation_holds_a_quarter_of_the_contract_at_recipe_magnitudes(seed):
    """the cases of test_gpu_criterion_fuzz.py::test_criteria_at_recipe_magnitudes_hold_the_contract, same seeds, same generator, T
    capped at 50 for N = 1000: every quantity of every criterion, per utterance with the fuzz's scaling, within 2.5e-5 of the fp64
    oracle.  Measured worst over both seeds (float32 yardstick against the oracle), loss / dx / dA: FCC 1.9e-6 / 2.0e-6 / 6.9e-7,
    FAC 9.5e-6 / 8.8e-6 / 2.2e-5, ASG 2.5e-6 (lossp) / 8.8e-6 / 2.2e-5, CTC 9.9e-7 / 1.4e-5.  The quantities taken out of tier A
    (module docstring) are printed next to them and held to the bar they keep, 1e-3."""
    worst = {}
    over = []
    for case in F.draw_cases(F.RECIPE_CASES, seed, **F.RECIPE):
        assert case.tier == "A"
        for (n, q), (e, b, tier, bar) in yardstick_errors(case).items():
            held = bar == F.TIER_BAR["A"]
            worst[(held, n, q)] = max(worst.get((held, n, q), 0.0), e)
            if not e <= (YARDSTICK_CAP if held else bar):
                over.append(f"{case.head()} {n} {q}[{b}] {e:.1e}")
    print("\n".join(f"yardstick fp32 seed {seed} {'tier A   ' if held else 'taken out'} {n} {q:5s} {e:.1e}"
                    for (held, n, q), e in sorted(worst.items())))
    assert not over, "\n".join(over)


def test_float32_instantiation_on_the_wide_tier_is_recorded():
    """emissions x 20 / 50 and transitions x 8 / 20 / 40, two orders of magnitude beyond a recipe: the yardstick's worst error is
    printed, and held to the wide tier's own bar of 1e-3.  Measured, loss / dx / dA: FCC 9.5e-7 / 4.3e-6 / 1.7e-6, FAC 8.7e-7 /
    8.8e-5 / 1.9e-5, ASG 1.8e-6 / 8.8e-5 / 1.9e-5, CTC 1.8e-6 / 5.2e-5 (16 cases, T capped at 50 for N = 1000).  A renormalised fp32
    recursion does not walk to "a few 1e-4 over 1000 frames" on FCC: it stays under 5e-6 at transitions x 40."""
    worst = {}
    for case in F.draw_cases(16, 9, x_scales=(20.0, 50.0), a_scales=(8.0, 20.0, 40.0), big_n_t_cap=50):
        assert case.tier == "wide"
        for key, (e, b, tier, bar) in yardstick_errors(case).items():
            assert tier == "wide"
            worst[key] = max(worst.get(key, 0.0), e)
    print("\n".join(f"yardstick fp32 wide tier {n} {q:5s} {e:.1e}" for (n, q), e in sorted(worst.items())))
    assert max(worst.values()) < F.TIER_BAR["wide"], worst
