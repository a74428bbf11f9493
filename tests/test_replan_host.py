"""w2l_trainer_plan drops the binding of the plan before (include/w2l_hip.h): the activation arena and the criterion workspace were
sized for the old shape, so between a plan and the next w2l_trainer_bind every call that would run a pass is refused ON THE HOST --
W2L_EINVAL, "trainer not planned / bound" -- before anything is enqueued.  No device is needed: the refusals come first, and the
calls that show a binding is accepted again are ones the trainer refuses one check LATER (a null input, no forward pass to
differentiate, an optimizer without its state arena), so nothing here ever reaches a launch.  The pointers handed to bind are host
buffers that no call dereferences.

The library before this contract kept `arena` / `critWs` of the old plan across w2l_trainer_plan: requireBound passed, and a forward
ran the new plan in the old, possibly smaller, arena."""
import ctypes as C

import numpy as np
import pytest

from wav2letter_amd import _lib, recipes

NFEAT, NLABEL = 8, 12
UNBOUND = "not planned / bound"


@pytest.fixture()
def tr():
    from wav2letter_amd.trainer import _lib_tr
    L = _lib_tr()
    arch = recipes.tds_ctc_small_arch(c=(4,), h=NFEAT, kw=5)
    h = L.w2l_trainer_create(arch.encode(), NFEAT, NLABEL, b"ctc", 4, 0.0)
    assert h
    yield L, h
    L.w2l_trainer_destroy(h)


class Buffers:
    """host memory standing in for the caller's device buffers (never read or written: every call below stops at a host check)"""

    def __init__(self, L, h):
        self.keep = [np.zeros(max(int(L.w2l_trainer_grad_floats(h)), 64), np.float32) for _ in range(6)]
        self.params, self.grads, self.arena, self.ws, self.x, self.tgt = (a.ctypes.data for a in self.keep)


def plan(L, h, B, T, Lt):
    af, cw, to = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    assert L.w2l_trainer_plan(h, B, T, Lt, C.byref(af), C.byref(cw), C.byref(to)) == 0
    assert af.value > 0 and to.value > 0
    return af.value


def passes(L, h, m):
    """the five calls that run a pass, with non-null operands: (name, status) each"""
    lp, pp, ep = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)
    return [("forward", L.w2l_trainer_forward(h, m.x, 0, C.byref(ep), None)),
            ("forward_backward", L.w2l_trainer_forward_backward(h, m.x, m.tgt, C.byref(lp), None)),
            ("backward", L.w2l_trainer_backward(h, m.x, None)),
            ("update", L.w2l_trainer_update(h, 0.1, 0.0, 0.0, 1.0, 1.0, 1, None)),
            ("evaluate", L.w2l_trainer_evaluate(h, m.x, m.tgt, C.byref(lp), C.byref(pp), None))]


def refused_as_unbound(L, h, m):
    for name, st in passes(L, h, m):
        msg = L.w2l_host_last_error().decode()
        assert st == _lib.W2L_EINVAL and UNBOUND in msg, (name, st, msg)


def accepted_as_bound(L, h, m):
    """past the bound-state check, each call stops at its NEXT host check (same status, another message)"""
    lp, pp = C.c_void_p(0), C.c_void_p(0)
    assert L.w2l_trainer_set_optimizer(h, 1, 1) == 0          # Adagrad keeps its sums in the momentum arena; none is bound
    # (statuses and messages are read call by call: w2l_host_last_error holds the last one only)
    checks = [
        (lambda: L.w2l_trainer_forward(h, None, 0, None, None), "forward: null input"),
        (lambda: L.w2l_trainer_forward_backward(h, None, m.tgt, None, None), "forward_backward: null input"),
        (lambda: L.w2l_trainer_backward(h, m.x, None), "no forward pass to differentiate"),
        (lambda: L.w2l_trainer_update(h, 0.1, 0.0, 0.0, 1.0, 1.0, 1, None), "momentum arena"),
        (lambda: L.w2l_trainer_evaluate(h, m.x, None, C.byref(lp), C.byref(pp), None), "evaluate: null input")]
    for call, want in checks:
        st = call()
        msg = L.w2l_host_last_error().decode()
        assert st == _lib.W2L_EINVAL and want in msg and UNBOUND not in msg, (want, st, msg)
    assert L.w2l_trainer_set_optimizer(h, 0, 0) == 0


def test_never_planned_is_refused(tr):
    L, h = tr
    refused_as_unbound(L, h, Buffers(L, h))


def test_planned_but_not_bound_is_refused(tr):
    L, h = tr
    plan(L, h, 2, 48, 4)
    refused_as_unbound(L, h, Buffers(L, h))


def test_a_second_plan_drops_the_binding_until_the_next_bind(tr):
    L, h = tr
    m = Buffers(L, h)
    small = plan(L, h, 1, 17, 2)
    assert L.w2l_trainer_bind(h, m.params, m.grads, None, m.arena, m.ws) == 0
    accepted_as_bound(L, h, m)
    assert plan(L, h, 3, 200, 5) > small          # the old arena could not hold this plan
    refused_as_unbound(L, h, m)
    refused_as_unbound(L, h, m)                   # a refusal changes nothing
    assert L.w2l_trainer_bind(h, m.params, m.grads, None, m.arena, m.ws) == 0
    accepted_as_bound(L, h, m)
    plan(L, h, 1, 17, 2)                          # back to the first shape: same sizes, still a new plan
    refused_as_unbound(L, h, m)
    assert L.w2l_trainer_bind(h, m.params, m.grads, None, m.arena, m.ws) == 0
    accepted_as_bound(L, h, m)


def test_backward_without_a_forward_pass_is_refused(tr):
    """plan -> bind -> backward: bound, but nothing to differentiate -- after the first plan and after a second one alike"""
    L, h = tr
    m = Buffers(L, h)
    for shape in [(2, 48, 4), (3, 33, 2)]:
        plan(L, h, *shape)
        assert L.w2l_trainer_bind(h, m.params, m.grads, None, m.arena, m.ws) == 0
        assert L.w2l_trainer_backward(h, m.x, None) == _lib.W2L_EINVAL
        assert "no forward pass to differentiate" in L.w2l_host_last_error().decode()


def test_a_plan_refused_for_its_arguments_changes_nothing(tr):
    L, h = tr
    m = Buffers(L, h)
    plan(L, h, 2, 48, 4)
    assert L.w2l_trainer_bind(h, m.params, m.grads, None, m.arena, m.ws) == 0
    assert L.w2l_trainer_plan(h, 0, 48, 4, None, None, None) == _lib.W2L_EINVAL     # no shape: the plan and its binding stay in force
    accepted_as_bound(L, h, m)


def test_counters_read_zero_before_any_update(tr):
    """the skipped-update count and the last norm live in memory the trainer allocates at its first update: before it both read 0
    on the host, planned or not"""
    L, h = tr
    n, g = C.c_uint64(7), C.c_double(7.0)
    assert L.w2l_trainer_skipped_updates(h, C.byref(n), None) == 0 and n.value == 0
    assert L.w2l_trainer_grad_norm(h, C.byref(g), None) == 0 and g.value == 0.0
    plan(L, h, 2, 48, 4)
    n, g = C.c_uint64(7), C.c_double(7.0)
    assert L.w2l_trainer_skipped_updates(h, C.byref(n), None) == 0 and n.value == 0
    assert L.w2l_trainer_grad_norm(h, C.byref(g), None) == 0 and g.value == 0.0
