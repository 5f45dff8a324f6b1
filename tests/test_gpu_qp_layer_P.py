"""GPU (-m gpu): the QP layer differentiable in P (osqp-solver_amd/qp_layer.py, README "Adjoint derivative").

qp_layer(..., Px=Px) feeds triu(P) through update_P_A_bounds_device and asks the adjoint for dP.  The problems, fixtures,
settings and the bound are those of test_gpu_adjoint.py: Px.grad within adjoint_refs.GPU_BOUND of the float64 reference in
the scale of its terms, and bitwise what a direct adjoint_device call returns for the same solve."""
import numpy as np
import pytest

import adjoint_refs as AR
import osqp_solver_amd as M

pytestmark = pytest.mark.gpu
SETTINGS = dict(polish=1, eps_abs=1e-7, eps_rel=1e-7)
KEYS = ("dq", "dP", "dA", "dl", "du")
B = AR.GPU_B


@pytest.fixture(scope="module")
def refs():
    """the problems, their fixtures (asserted), the seed of the loss and the reference gradients: computed once"""
    pr = AR.gpu_problem()
    fxs = [AR.fixture(pr, b, key="gpu") for b in range(B)]
    for fx in fxs:
        AR.assert_preconditions(fx)
    gx, _ = AR.gradient_seeds(B, pr["n"], pr["m"])
    ref = [AR.adjoint_ref(fx["P"], fx["A"], fx["act"], fx["x"], fx["y"], gx[b]) for b, fx in enumerate(fxs)]
    gx.setflags(write=False)
    return dict(pr=pr, fx=fxs, gx=gx, ref=ref)


def make(pr):
    return M.BatchSolver(pr["P"], pr["Px"], pr["q"], pr["A"], pr["Ax"], pr["l"], pr["u"], **SETTINGS)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def leaves(pr, grad=True):
    import torch
    t = lambda a: torch.tensor(a, device="cuda", requires_grad=grad)
    return dict(q=t(pr["q"]), Ax=t(pr["Ax"]), l=t(pr["l"]), u=t(pr["u"]), Px=t(pr["Px"]))


@pytest.mark.parametrize("ruiz", ["host", "device"])          # 6 QPs equilibrate on host threads unless told otherwise
def test_Px_grad_is_the_adjoint_dP_within_the_bound_and_bitwise_the_direct_call(refs, ruiz, monkeypatch):
    import torch
    from osqp_solver_amd.qp_layer import qp_layer
    monkeypatch.delenv("MI_OSQP_HOST_RUIZ", raising=False)
    if ruiz == "device":
        monkeypatch.setenv("MI_OSQP_DEVICE_RUIZ", "1")
    pr = refs["pr"]
    s = make(pr)
    v = leaves(pr)
    x = qp_layer(s, v["q"], v["Ax"], v["l"], v["u"], Px=v["Px"])
    info = s.info()
    assert [i.status_val for i in info] == [1] * B and [i.status_polish for i in info] == [1] * B
    act = s.polish_active()
    for b in range(B):
        np.testing.assert_array_equal(act[b], refs["fx"][b]["act"], err_msg=f"QP {b}")
    assert same_bits(x.detach().cpu().numpy(), s.primal())
    w = torch.tensor(refs["gx"], device="cuda")
    asked = []
    inner = s.adjoint_device
    monkeypatch.setattr(s, "adjoint_device", lambda *a, **kw: (asked.append(kw), inner(*a, **kw))[1])
    (x * w).sum().backward()
    monkeypatch.setattr(s, "adjoint_device", inner)
    assert len(asked) == 1 and all(asked[0][k] is not None for k in KEYS)
    got = dict(dq=v["q"].grad, dP=v["Px"].grad, dA=v["Ax"].grad, dl=v["l"].grad, du=v["u"].grad)
    got = {k: g.cpu().numpy() for k, g in got.items()}
    assert got["dP"].shape == pr["Px"].shape
    direct = {k: torch.empty_like(v[n]) for k, n in zip(KEYS, ("q", "Px", "Ax", "l", "u"))}
    s.adjoint_device(w, None, **direct)                          # the same handle state the backward saw
    torch.cuda.synchronize()
    for k in KEYS:
        assert same_bits(got[k], direct[k].cpu().numpy()), k
    worst, where = 0.0, None
    for b in range(B):
        fx = refs["fx"][b]
        e, k = AR.worst_ratio({k: got[k][b] for k in KEYS}, refs["ref"][b], fx["x"], fx["y"])
        if e >= worst:
            worst, where = e, (b, k)
        eP, _ = AR.worst_ratio({"dP": got["dP"][b]}, refs["ref"][b], fx["x"], fx["y"], keys=("dP",))
        assert eP <= AR.GPU_BOUND, (b, eP)
    print(f"layer with Px ({ruiz} equilibration): worst ratio {worst:.3e} at {where}")
    assert worst <= AR.GPU_BOUND, (worst, where)
    s.close()


def test_only_the_gradients_autograd_needs_are_asked_for(refs, monkeypatch):
    import torch
    from osqp_solver_amd.qp_layer import qp_layer
    pr = refs["pr"]
    s = make(pr)
    v = leaves(pr, grad=False)
    v["Px"].requires_grad_(True)
    x = qp_layer(s, v["q"], v["Ax"], v["l"], v["u"], Px=v["Px"])
    asked = []
    inner = s.adjoint_device
    monkeypatch.setattr(s, "adjoint_device", lambda *a, **kw: (asked.append(kw), inner(*a, **kw))[1])
    x.sum().backward()
    monkeypatch.setattr(s, "adjoint_device", inner)
    assert len(asked) == 1 and asked[0]["dP"] is not None
    assert all(asked[0][k] is None for k in ("dq", "dA", "dl", "du"))
    assert v["Px"].grad is not None and v["q"].grad is None
    assert bool(torch.all(torch.isfinite(v["Px"].grad)))
    s.close()


def test_without_Px_the_layer_is_the_one_without_the_argument_bitwise(refs, monkeypatch):
    import torch
    from osqp_solver_amd.qp_layer import qp_layer
    pr = refs["pr"]
    w = torch.tensor(refs["gx"], device="cuda")
    out = []
    for explicit_none in (False, True):
        s = make(pr)
        calls = []
        for name in ("update_q_device", "update_A_bounds_device", "update_P_A_bounds_device", "update_P_device", "solve_device", "adjoint_device"):
            inner = getattr(s, name)
            monkeypatch.setattr(s, name, (lambda nm, fn: lambda *a, **kw: (calls.append((nm, sorted(kw))), fn(*a, **kw))[1])(name, inner))
        v = leaves(pr)
        x = qp_layer(s, v["q"], v["Ax"], v["l"], v["u"], Px=None) if explicit_none else qp_layer(s, v["q"], v["Ax"], v["l"], v["u"])
        (x * w).sum().backward()
        out.append((calls, x.detach().cpu().numpy(), [v[k].grad.cpu().numpy() for k in ("q", "Ax", "l", "u")]))
        s.close()
    (c0, x0, g0), (c1, x1, g1) = out
    assert c0 == c1
    assert [c[0] for c in c0] == ["update_q_device", "update_A_bounds_device", "solve_device", "adjoint_device"]
    assert "dP" not in c0[3][1]
    assert same_bits(x0, x1)
    for a, b in zip(g0, g1):
        assert same_bits(a, b)


def test_a_second_forward_before_the_backward_still_raises(refs):
    from osqp_solver_amd.qp_layer import qp_layer
    pr = refs["pr"]
    s = make(pr)
    v = leaves(pr)
    x1 = qp_layer(s, v["q"], v["Ax"], v["l"], v["u"], Px=v["Px"])
    qp_layer(s, v["q"], v["Ax"], v["l"], v["u"], Px=v["Px"])
    with pytest.raises(RuntimeError, match="another forward"):
        x1.sum().backward()
    s.close()
