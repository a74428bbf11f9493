"""float64 restatement of the Adam contract of w2l_adam_step_guarded / fl::AdamOptimizer (include/w2l_hip.h), for the tests.

With t = the number of APPLIED steps including this one (a skipped step advances nothing):
    clr = lr sqrt(1 - beta2^t) / (1 - beta1^t)
    p   = p - (wd lr) p                      first, with lr and not clr; decoupled: the moments never see it
    m   = beta1 m + (1 - beta1) g
    v   = beta2 v + (1 - beta2) g g
    p   = p - clr m / (sqrt(v) + eps)        eps OUTSIDE the bias correction (torch.optim.Adam: sqrt(v) / sqrt(1 - beta2^t) + eps)
g is the gradient as the rule sees it (scaled and clipped by the caller).  The C ABI carries lr, beta1, beta2, eps and wd as
float32: f32() gives the value a Python float has there, so that a test states the rule at the numbers the kernel was given."""
import numpy as np


def f32(x):
    return float(np.float32(x))


class Adam:
    def __init__(self, p, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, torch_eps=False):
        """torch_eps: eps where torch.optim.Adam puts it, inside the bias correction -- NOT the contract; for the tests that show
        their bar tells the two apart"""
        self.torch_eps = torch_eps
        self.p = np.array(p, np.float64)
        self.m = np.zeros_like(self.p)
        self.v = np.zeros_like(self.p)
        self.t = 0
        self.lr, self.beta1, self.beta2, self.eps, self.wd = lr, beta1, beta2, eps, wd

    def step(self, g, skip=False, lr=None, wd=None, count_skipped=False):
        """one update with gradient g; skip: the update the guard refuses -- p, m, v and t stay.  lr / wd: per-call values
        (an array to give the network and the criterion slices of one arena their own).  count_skipped: the WRONG rule a test
        must be able to tell from the right one -- a skipped update that still advances the bias correction"""
        if skip:
            self.t += 1 if count_skipped else 0
            return self
        lr = self.lr if lr is None else lr
        wd = self.wd if wd is None else wd
        g = np.asarray(g, np.float64)
        self.t += 1
        clr = lr * np.sqrt(1.0 - self.beta2 ** self.t) / (1.0 - self.beta1 ** self.t)
        self.p = self.p - (wd * lr) * self.p
        self.m = self.beta1 * self.m + (1.0 - self.beta1) * g
        self.v = self.beta2 * self.v + (1.0 - self.beta2) * g * g
        eps = self.eps * np.sqrt(1.0 - self.beta2 ** self.t) if self.torch_eps else self.eps
        self.p = self.p - clr * self.m / (np.sqrt(self.v) + eps)
        return self


def run(p0, grads, lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, skips=None, count_skipped=False, torch_eps=False):
    """the states after each step: a list of (p, m, v, t) copies"""
    a = Adam(p0, lr, beta1, beta2, eps, wd, torch_eps)
    out = []
    for i, g in enumerate(grads):
        a.step(g, skip=bool(skips and skips[i]), count_skipped=count_skipped)
        out.append((a.p.copy(), a.m.copy(), a.v.copy(), a.t))
    return out


def closed_form(p0, grads, lr, beta1, beta2, eps, wd):
    """the contract unrolled, no recurrence: m_t = (1 - beta1) sum_k beta1^(t-k) g_k, v_t likewise on g_k^2, and every step's
    decay factor (1 - wd lr) applied to what came before it"""
    p = np.array(p0, np.float64)
    gs = [np.asarray(g, np.float64) for g in grads]
    for t in range(1, len(gs) + 1):
        m = (1.0 - beta1) * sum(beta1 ** (t - k) * gs[k - 1] for k in range(1, t + 1))
        v = (1.0 - beta2) * sum(beta2 ** (t - k) * gs[k - 1] ** 2 for k in range(1, t + 1))
        clr = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        p = p * (1.0 - wd * lr) - clr * m / (np.sqrt(v) + eps)
    return p
