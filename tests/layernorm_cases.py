"""The inputs of the per-group LayerNorm tests (tests/test_layernorm_stats_model.py on the CPU, tests/test_gpu_layernorm_groups.py on
the device): ONE tensor per case whose groups cycle through kinds with very different |mean| / sigma and scales, so that an error bar
over the whole tensor and one per group are different things.  Everything comes from fixed seeds; nothing here touches a GPU."""
import numpy as np

from oracle import layernorm_stats_model as M

GAMMA, BETA, EPS = 1.3, -0.2, 1e-5
DROP_P, DROP_SEED, DROP_STREAM = 0.25, 77, 5
FLOOR_MAX = 5e-5     # half the 1e-4 bar: what rounding the saved mean to fp32 may cost on these inputs

# kind -> (mean, sigma) of a drawn group, or the value of a constant one
DRAWN = {"n01": (0.0, 1.0), "mean+100": (100.0, 1.0), "mean-100": (-100.0, 1.0), "mean+1000": (1000.0, 1.0),
         "mean-1000": (-1000.0, 1.0), "mean10_sigma.01": (10.0, 0.01), "sigma1e-3": (0.0, 1e-3), "sigma1e3": (0.0, 1e3),
         "first1000_rest100": (100.0, 1.0)}
CONSTANT = {"const0": 0.0, "const3": 3.0, "const100.1": 100.1, "const-23.0259": -23.0259}
KINDS = ("n01", "mean+100", "const100.1", "mean-1000", "mean10_sigma.01", "const0", "first1000_rest100", "mean-100", "const-23.0259",
         "sigma1e-3", "mean+1000", "const3", "sigma1e3")
OFFSET_KINDS = ("mean+100", "mean-100", "mean+1000", "mean-1000", "mean10_sigma.01", "first1000_rest100")
assert set(KINDS) == set(DRAWN) | set(CONSTANT)


class Case:
    def __init__(self, family, groups, inner, pattern, start, wave=True):
        self.family, self.groups, self.inner, self.pattern, self.start, self.wave = family, groups, inner, pattern, start, wave
        assert M.family_of(inner, wave=wave, images=family == "images") == family
        self.id = f"{family}-{groups}x{inner}-{pattern}" + ("" if wave else "-nowave")
        self.kinds = [KINDS[(start + g) % len(KINDS)] for g in range(groups)]
        self.p = DROP_P if pattern == "dropout" else 0.0

    def __repr__(self):
        return self.id


def _cases():
    shapes = [("scalar", 3, 10, True), ("wave", 5, 8, True), ("wave", 6, 260, True), ("wave", 5, 2304, True),
              ("block", 3, 2308, True), ("block", 3, 8192, True), ("block", 5, 64, False),
              ("two_level", 2, 8196, True), ("two_level", 2, 160004, True),
              ("images", 17, 8, True), ("images", 5, 260, True), ("images", 3, 2304, True)]
    dropout_shape = {"scalar": 10, "wave": 260, "block": 2308, "two_level": 8196, "images": 260}   # one residual + dropout case per family
    out, start = [], 0
    for family, groups, inner, wave in shapes:
        patterns = ["plain", "residual"] + (["dropout"] if wave and dropout_shape[family] == inner else [])
        for pattern in patterns:
            out.append(Case(family, groups, inner, pattern, start, wave))
            start += groups        # the next case goes on where this one stopped: every kind meets every family
    return out


CASES = _cases()


def floor_of(r):
    """per group: what rounding the group's mean to fp32 costs, relative to the group's largest |r - mean| (inf on constant groups)"""
    r64 = np.asarray(r, np.float64)
    mu = r64.mean(1)
    dev = np.abs(r64 - mu[:, None]).max(1)
    with np.errstate(divide="ignore"):
        return 0.5 * np.spacing(np.abs(mu).astype(np.float32)).astype(np.float64) / dev


def _draw(kind, n, rng):
    mean, sigma = DRAWN[kind]
    t = (mean + sigma * rng.normal(size=n)).astype(np.float32)
    if kind == "first1000_rest100":
        t[0] = 1000.0
    return t


def build(case, dropout=None):
    """-> dict(a, x, r, kinds, const, floor, dy1, dy2).  a [G][n] fp32 (>= 0) and x (None in the plain pattern) are what the kernel is
    given; r is the fp32 pre-norm sum it must return (a in the plain pattern, dropout(a) + x otherwise; `dropout` =
    oracle.dropout is needed by the dropout pattern only); const marks the groups of r that are constant, floor is floor_of(r)."""
    G, n = case.groups, case.inner
    target = np.empty((G, n), np.float32)
    a = np.empty((G, n), np.float32)
    for g, kind in enumerate(case.kinds):
        if kind in CONSTANT:
            target[g] = np.float32(CONSTANT[kind])
            a[g] = 0.0 if case.p > 0 else 0.5      # (a dropped constant would not leave a constant group)
            continue
        for attempt in range(64):                   # a fixed sequence of seeds; the first draw whose floor leaves a margin
            rng = np.random.default_rng([2024, CASES.index(case), g, attempt])
            target[g] = _draw(kind, n, rng)
            if floor_of(target[g:g + 1])[0] <= 0.8 * FLOOR_MAX:
                break
        a[g] = np.maximum(rng.normal(size=n), 0.0) * DRAWN[kind][1]
    if case.pattern == "plain":
        a, x, r = target, None, target
    else:
        x = target - a
        a_drop = dropout(a.reshape(-1), case.p, DROP_SEED, DROP_STREAM).reshape(a.shape) if case.p > 0 else a
        r = a_drop + x
        assert x.dtype == np.float32 and r.dtype == np.float32
    rng = np.random.default_rng([2025, CASES.index(case)])
    scale = np.array([1e-3, 1.0, 1e3])[np.arange(G) % 3][:, None]
    dy1 = (rng.normal(size=(G, n)) * scale).astype(np.float32)
    dy2 = (100.0 + rng.normal(size=(G, n))).astype(np.float32)
    const = (r == r[:, :1]).all(1)
    return dict(a=a, x=x, r=r, kinds=list(case.kinds), const=const, floor=floor_of(r), dy1=dy1, dy2=dy2)


def reference(r, gamma=GAMMA, beta=BETA, eps=EPS):
    """two passes in fp64 on the fp32 r: (y, mean, rstd), all fp64 -- the arithmetic of w2l_oracle_layernorm_fwd, kept in fp64"""
    r64 = np.asarray(r, np.float64)
    mu = r64.mean(1)
    var = ((r64 - mu[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    y = np.float64(np.float32(gamma)) * ((r64 - mu[:, None]) * rstd[:, None]) + np.float64(np.float32(beta))
    return y, mu, rstd


def group_errors(y, rstd, r, y_ref, beta=BETA):
    """per group: (error of y over the group's largest |y_ref - beta|, relative error of rstd); y_ref [G][n] is the oracle's
    (oracle.layernorm_fwd), the rstd that of reference(r)"""
    rstd_ref = reference(r)[2]
    y_ref = np.asarray(y_ref, np.float64).reshape(np.shape(r))
    scale = np.abs(y_ref - np.float64(np.float32(beta))).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ey = np.abs(np.asarray(y, np.float64) - y_ref).max(1) / scale
    return ey, np.abs(np.asarray(rstd, np.float64) - rstd_ref) / rstd_ref
