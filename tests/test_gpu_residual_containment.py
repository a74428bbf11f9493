"""Containment of the residual block (DESIGN.md 3.19 is the contract, 3.29 the block): the two join kernels read their operands only
inside n floats and write only the n floats of their result, and one forward and backward pass of a block stays inside the
activation arena the plan asked for, the parameter arena and the gradient arena.

As in tests/test_gpu_cpc_containment.py a case runs on identical inputs in three guarded arenas (tests/arena.py) -- quiet, quiet
again, NaN -- and must leave every guard byte as it was, give bit-identical results in all three, write every element of a result,
and agree with the restatement (tests/residual_ref.py).  The kernels' operands sit 0 to 3 floats into buffers three floats longer
than themselves -- the float4 body with its scalar head and tail where the phases agree, the element-wise path where they do not --
and the floats before and behind an operand must keep their bits.  The activation arena of the block pass is a workspace of exactly
the planned size and starts as NaN in the third run: a layer that reads an arena float nobody wrote turns the results NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import residual_ref as R
from tests.test_gpu_containment import _stream
from tests.test_gpu_cpc_containment import run_three
from wav2letter_amd.criterion import CriterionScaleMode
from wav2letter_amd.trainer import Trainer

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(7.25)
SCALE = 0.70711


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("offs", [(0, 0, 0), (1, 1, 1), (3, 3, 3), (0, 1, 2), (2, 2, 0), (1, 0, 0)])
@pytest.mark.parametrize("n", [4099, 5])
def test_join_kernels_stay_inside(n, offs, relu):
    rng = np.random.default_rng(n + sum(offs))
    a, b, dy = (rng.normal(size=n).astype(np.float32) for _ in range(3))
    b[::7] = -a[::7]
    oy, oa, ob = offs

    def padded(x, off):
        buf = np.full(n + 3, SENTINEL, np.float32)
        buf[off:off + n] = x
        return buf

    def fn(r):
        pa, pb, pdy = r.inp("a", padded(a, oa)) + 4 * oa, r.inp("b", padded(b, ob)) + 4 * ob, r.inp("dy", padded(dy, oa)) + 4 * oa
        py = r.inout("y", padded(np.zeros(n, np.float32), oy)) + 4 * oy
        pg = r.inout("g", padded(np.zeros(n, np.float32), ob)) + 4 * ob
        r.ok(r.L.w2l_residual_join_forward(py, pa, pb, n, SCALE, relu, _stream()), "join forward")
        r.ok(r.L.w2l_residual_join_backward(pg, pdy, py, n, SCALE, relu, _stream()), "join backward")

        def ref():
            y = R.join_forward(a, b, SCALE, relu)
            return {"y": ("exact", padded(y, oy)), "g": ("exact", padded(R.join_backward(dy, y, SCALE, relu), ob))}
        return ref
    run_three(fn)


BLOCK = "V -1 1 NFEAT 0\nRES 3 1 1\nC 16 16 3 1 -1 1\nR\nC 16 16 3 1 -1 1\nSKIP 0 4 0.70711\nR\nRO 2 0 3 1\n"
PROJ = "V -1 1 NFEAT 0\nRES 3 1 1\nC 16 24 3 1 -1 1\nR\nC 24 24 3 1 -1 1\nSKIPL 0 4 1 0.7071\nC 16 24 1 1 -1 1\nR\nRO 2 0 3 1\n"


@pytest.mark.parametrize("arch,cout", [(BLOCK, 16), (PROJ, 24)], ids=["identity", "projection"])
def test_block_pass_stays_inside(arch, cout):
    """forward (training mode) and backward of one block, B = 3, T = 37, with the input gradient: emissions, parameter gradients and
    input gradient against the restatement at the fp32 bar"""
    B, T, cin = 3, 37, 16
    rng = np.random.default_rng(cout)
    x = rng.normal(size=(B, cin, T)).astype(np.float32)
    dy = rng.normal(size=(B, T, cout)).astype(np.float32)
    host = Trainer(arch, cin, cout, "ctc", CriterionScaleMode.NONE, device="cpu")
    host.init_params(11)
    table = host.param_table()
    # reference shapes from the arch lines: conv.w (kw, 1, cin, cout), conv.b (1, 1, cout, 1)
    convs = [f for f in R.parse(arch, cin, cout) if f[0] == "C"]
    shapes = sum(([(int(f[3]), 1, int(f[1]), int(f[2])), (1, 1, int(f[2]), 1)] for f in convs), [])
    ref_params = [host.export_from(i, host.host_params) for i in range(len(table))]

    def fn(r):
        tr = Trainer(arch, cin, cout, "ctc", CriterionScaleMode.NONE, device="cpu")
        Lt = tr.L
        af, cw, to = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        assert Lt.w2l_trainer_plan(tr.h, B, T, 2, C.byref(af), C.byref(cw), C.byref(to)) == 0 and to.value == T
        assert Lt.w2l_trainer_set_input_gradient(tr.h, 1) == 0
        p = r.inp("params", host.host_params)
        n_grad = int(Lt.w2l_trainer_grad_floats(tr.h))
        g = r.work("grads", 4 * n_grad)
        mom = r.inp("momentum", np.zeros_like(host.host_params))
        arena = r.work("arena", 4 * af.value)
        ws = r.work("criterion workspace", cw.value)
        r.ok(Lt.w2l_trainer_bind(tr.h, p, g, mom, arena, ws), "bind")
        em = C.c_void_p(0)
        r.ok(Lt.w2l_trainer_forward(tr.h, r.inp("x", x), 1, C.byref(em), _stream()), "forward")
        r.ok(Lt.w2l_trainer_backward(tr.h, r.inp("dy", dy), _stream()), "backward")
        dx = C.c_void_p(0)
        r.ok(Lt.w2l_trainer_input_gradient(tr.h, C.byref(dx)), "input gradient")
        assert arena <= em.value and em.value + 4 * dy.size <= arena + 4 * af.value
        assert arena <= dx.value and dx.value + 4 * x.size <= arena + 4 * af.value
        torch.cuda.synchronize()
        av = r.view("arena").view(torch.float32)
        gv = r.view("grads").view(torch.float32)
        r.results["y"] = av[(em.value - arena) // 4:][:dy.size].clone().view(B, T, cout)
        r.results["dx"] = av[(dx.value - arena) // 4:][:x.size].clone().view(B, T, cin)
        for i, (name, n, off) in enumerate(table):
            r.results[f"grad {i}"] = gv[off:off + n].clone()
        r.keep = tr                                   # (alive until the run has been compared)

        def ref():
            params = R.to_torch(ref_params, shapes)
            xt = torch.tensor(x.astype(np.float64), requires_grad=True)
            y = R.Net(arch, cin, cout).forward(xt, params)
            (y * torch.tensor(dy.astype(np.float64))).sum().backward()
            want = {"y": ("rel", y.detach().numpy()), "dx": ("rel", xt.grad.numpy().transpose(0, 2, 1))}
            probe = Trainer(arch, cin, cout, "ctc", CriterionScaleMode.NONE, device="cpu")
            for i, q in enumerate(params):          # the gradient arena holds the internal layout: the reference gradient, imported
                probe.import_param(i, q.grad.numpy().reshape(-1).astype(np.float32))
                name, n, off = table[i]
                want[f"grad {i}"] = ("rel", probe.host_params[off:off + n].astype(np.float64))
            return want
        return ref
    run_three(fn)
