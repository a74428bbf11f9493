"""TEST INFRASTRUCTURE (oracle side).  The ARITHMETIC of the LayerNorm forward statistic (wav2letter_amd/csrc/elementwise.hip:
residual_dropout_stats_k + ln_apply_k, residual_ln_small_k, residual_ln_wave_k, residual_ln_scalar_k; csrc/layernorm_images.hip's
forward branch) restated in numpy, so that its numerics are pinned on the CPU against the two-pass fp64 oracle
(oracle/nn_oracle.c: w2l_oracle_layernorm_fwd) -- in the manner of oracle/ctc_linear_domain.py.

What is fp32 and what is fp64 in the kernels, and this file repeats:
  * the pre-norm sum r is fp32 (it is this model's INPUT: dropout and the residual add happen before the statistic);
  * the vector kernels reduce every float4 of the group to two fp32 partials, (d0 + d1) + (d2 + d3) and
    (d0*d0 + d1*d1) + (d2*d2 + d3*d3), and add the partials in fp64 (the order of the fp64 additions differs between the kernels and
    is below everything judged here: the model adds them with numpy's pairwise sum);
  * mu and var are fp64; muf = (float)mu and rstd = (float)(1 / sqrt(var + eps)) are what is saved for the backward pass;
  * y = (r - muf) * (gamma * rstd) + beta in fp32.

`parent`: d = r.  The fp32 partial of four elements of a group with mean 100 is ~400 with an ulp of 3e-5, mu*mu then carries
2 * mu * dmu and is subtracted from E[r^2]: the error of var is of order 1e-3 * |mean| and does not shrink by accumulating in fp64.
`shipped`: the kernels that hold the group in registers (wave, block, images) compute the parent's statistic and, where it cancels
(mu^2 > 64 var: |mean| above 8 sigma), take the sums AGAIN with d = r - K about the pilot K = (float)mu: mu = K + s/n,
var = ss/n - (s/n)^2, partials of the size of the group's spread, not of its mean.  A group that is not ill-conditioned keeps the
parent's bits (there the parent loses at most 6e-8 * 65 of var).  The two-level kernel (groups of more than 8192 floats, several
workgroups per group, not held in registers) cannot go back: it takes both kinds of sums in its one pass and the apply kernel uses
the shifted ones where the plain ones cancel.  A K shared between workgroups would mean reading an element another workgroup may be
overwriting in place (dropout, r stored over a), so every workgroup takes the FIRST element it meets as its pilot and turns its
sums into the raw moments
sum r = n_b K_b + s_b, sum r^2 = ss_b + 2 K_b s_b + n_b K_b^2 in fp64 before they are merged: fp64 raw moments lose
1e-16 * mean^2 / var, which is 1e-8 at mean 100, sigma 0.01.  The scalar kernel (group sizes that are no multiple of 4) converts
every element to fp64 before both sums."""
import numpy as np

FAMILIES = ("scalar", "wave", "block", "two_level", "images")
_EW_THREADS = 256      # kEwThreads
_LN_MAX_PARTS = 64     # kLnMaxParts
_LN_SMALL = 8192       # kLnSmall
_LN_WAVE_FLOATS = 2304  # 64 lanes * 4 floats * kLnWaveV


def family_of(inner, wave=True, images=False):
    """which kernel w2l_residual_layernorm_forward launches for a group of `inner` floats"""
    if images:
        assert inner % 4 == 0 and inner <= _LN_WAVE_FLOATS
        return "images"
    if inner % 4:
        return "scalar"
    if inner <= _LN_WAVE_FLOATS and wave:
        return "wave"
    return "block" if inner <= _LN_SMALL else "two_level"


def ln_parts(inner):
    """workgroups (partials) per group of the two-level kernel: elementwise.hip::ln_parts"""
    return int(min(max(((inner >> 2) + _EW_THREADS * 4 - 1) // (_EW_THREADS * 4), 1), _LN_MAX_PARTS))


def _partials4(d):
    """[G][n] fp32 -> the fp32 partials of every float4: ([G][n/4] sums, [G][n/4] sums of squares)"""
    q = d.reshape(d.shape[0], -1, 4)
    q0, q1, q2, q3 = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    p1 = (q0 + q1) + (q2 + q3)
    p2 = (q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3)
    assert p1.dtype == np.float32 and p2.dtype == np.float32
    return p1, p2


def stats_parent(r, family):
    """(mu, var) in fp64 as the kernels BEFORE the pilot computed them"""
    r = np.ascontiguousarray(r, np.float32)
    n = r.shape[1]
    if family == "scalar":            # s += (double)rv; ss += (double)(rv * rv)
        s = r.astype(np.float64).sum(1)
        ss = (r * r).astype(np.float64).sum(1)
    else:
        p1, p2 = _partials4(r)
        s = p1.astype(np.float64).sum(1)
        ss = p2.astype(np.float64).sum(1)
    mu = s / n
    return mu, ss / n - mu * mu


LN_ILL_COND = 64.0     # common.hpp::kLnIllCond


def ill_conditioned(mu, var):
    """common.hpp::ln_ill_conditioned: |mean| above 8 sigma (a constant group of a value other than 0 counts)"""
    return mu * mu > LN_ILL_COND * var


def stats_shipped(r, family):
    """(mu, var) in fp64 as the kernels compute them now"""
    r = np.ascontiguousarray(r, np.float32)
    G, n = r.shape
    if family == "scalar":            # every element converted before both sums
        r64 = r.astype(np.float64)
        mu = r64.sum(1) / n
        return mu, (r64 * r64).sum(1) / n - mu * mu
    if family != "two_level":         # wave, block, images: the parent's sums, taken again about K = (float)mu where they cancel
        mu, var = stats_parent(r, family)
        ill = ill_conditioned(mu, var)
        K = np.where(ill, mu, 0.0).astype(np.float32)[:, None]
        p1, p2 = _partials4(r - K)
        m = p1.astype(np.float64).sum(1) / n
        return (np.where(ill, K[:, 0].astype(np.float64) + m, mu),
                np.where(ill, p2.astype(np.float64).sum(1) / n - m * m, var))
    mu0, var0 = stats_parent(r, family)          # two_level: both kinds of sums in one pass, the pilots' where the plain ones cancel
    ill = ill_conditioned(mu0, var0)
    parts = ln_parts(n)
    n4 = n >> 2
    blk = (np.arange(n4) // _EW_THREADS) % parts                       # grid-stride loop: float4 i belongs to this workgroup
    K = r[:, 4 * _EW_THREADS * np.arange(parts)]                        # [G][parts]: the first element each workgroup meets
    p1, p2 = _partials4(r - np.repeat(K[:, blk], 4, axis=1))
    S = np.zeros(G)
    SS = np.zeros(G)
    for b in range(parts):
        sel = blk == b
        nb = 4.0 * sel.sum()
        Kb = K[:, b].astype(np.float64)
        sb = p1[:, sel].astype(np.float64).sum(1)
        ssb = p2[:, sel].astype(np.float64).sum(1)
        S += nb * Kb + sb
        SS += ssb + 2.0 * Kb * sb + nb * Kb * Kb
    mu = S / n
    return np.where(ill, mu, mu0), np.where(ill, SS / n - mu * mu, var0)


def layernorm_model(r, gamma, beta, eps, family, arithmetic="shipped"):
    """r [groups][inner] fp32 -> (y fp32 [groups][inner], muf fp32 [groups], rstd fp32 [groups]) as the kernel of `family` leaves them"""
    assert family in FAMILIES and arithmetic in ("shipped", "parent")
    r = np.ascontiguousarray(r, np.float32)
    mu, var = (stats_shipped if arithmetic == "shipped" else stats_parent)(r, family)
    var = np.maximum(var, 0.0)
    rstd = (1.0 / np.sqrt(var + np.float64(np.float32(eps)))).astype(np.float32)
    muf = mu.astype(np.float32)
    gam = np.float32(gamma) * rstd
    y = (r - muf[:, None]) * gam[:, None] + np.float32(beta)
    assert y.dtype == np.float32
    return y, muf, rstd
