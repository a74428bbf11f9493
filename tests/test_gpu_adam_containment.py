"""Containment of w2l_adam_step_guarded: g is read only inside its n floats; p, m, v and the step counter are the only bytes written.

As in tests/test_gpu_cpc_containment.py a case runs on identical inputs in three guarded arenas (tests/arena.py) -- quiet, quiet
again, NaN -- and must leave every guard byte as it was, give bit-identical p, m, v and counter in all three, and agree with the
float64 restatement (tests/adam_ref.py) at the kernel test's bars.  Each operand sits `off` floats into a buffer three floats
longer than itself, so the entry point meets every phase against 16 bytes -- the float4 body with its scalar head and tail where
p / g and m / v share a phase, the element-wise path where they do not -- and the floats of that buffer before and behind the
operand must keep their bits too."""
import numpy as np
import pytest

import adam_ref as R
from tests.test_gpu_containment import _stream
from tests.test_gpu_cpc_containment import run_three

pytestmark = pytest.mark.gpu
F = R.f32
LR, B1, B2, EPS, WD = F(0.01), F(0.9), F(0.999), F(1e-3), F(0.1)
SENTINEL = np.float32(7.25)


@pytest.mark.parametrize("counter", [False, True])
@pytest.mark.parametrize("s_off", range(4))
@pytest.mark.parametrize("p_off", range(4))
@pytest.mark.parametrize("n", [4099, 5])
def test_adam_step_stays_inside(n, p_off, s_off, counter):
    rng = np.random.default_rng(n + 4 * p_off + s_off)
    vals = {"p": rng.normal(size=n), "g": rng.normal(size=n), "m": 0.1 * rng.normal(size=n), "v": 0.01 * rng.uniform(size=n)}
    vals = {k: x.astype(np.float32) for k, x in vals.items()}
    offs = {"p": p_off, "g": p_off, "m": s_off, "v": s_off}

    def padded(key):
        buf = np.full(n + 3, SENTINEL, np.float32)
        buf[offs[key]:offs[key] + n] = vals[key]
        return buf

    def fn(r):
        ptr = {"g": r.inp("g", padded("g")) + 4 * offs["g"]}
        for key in ("p", "m", "v"):
            ptr[key] = r.inout(key, padded(key)) + 4 * offs[key]
        count = r.inout("count", np.array([2, 0], np.int32)) if counter else None      # the 8-byte counter: two applied steps so far
        r.ok(r.L.w2l_adam_step_guarded(ptr["p"], ptr["g"], ptr["m"], ptr["v"], n, LR, B1, B2, EPS, WD, 1.0, 0.0, None, 0 if counter else 3,
                                       count, _stream()), "adam")

        def ref():
            a = R.Adam(vals["p"], LR, B1, B2, EPS, WD)
            a.m, a.v, a.t = vals["m"].astype(np.float64), vals["v"].astype(np.float64), 2
            a.step(vals["g"])
            want = {}
            for key, x, bar in (("p", a.p, 1e-5), ("m", a.m, 1e-6 * np.abs(a.m).max()), ("v", a.v, 1e-6 * np.abs(a.v).max())):
                inside = np.zeros(n + 3, bool)
                inside[offs[key]:offs[key] + n] = True
                got = r.view(key).cpu().numpy()
                assert (got[~inside].view(np.int32) == SENTINEL.view(np.int32)).all(), f"{key}: a float outside the operand changed"
                full = padded(key).astype(np.float64)
                full[inside] = x
                want[key] = (("bound", bar), full)       # the kernel test's bars, element by element
            if counter:
                want["count"] = ("exact", np.array([3, 0]))
            return want
        return ref
    run_three(fn)
