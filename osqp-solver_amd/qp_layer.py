"""A batch of QPs as a differentiable torch layer: x*(q, A, l, u) with P fixed (there is no device-side P update).

    x = qp_layer(solver, q, Ax, l, u)        # CUDA float64: q [B, n], Ax [B, nnzA] (CSC order of A), l, u [B, m]
    loss(x).backward()                       # q.grad, Ax.grad, l.grad, u.grad

Forward is update_q_device, update_A_bounds_device, solve_device on the given BatchSolver; backward is one
BatchSolver.adjoint_device call that asks only for the gradients autograd needs.  No solver logic lives here: the
derivative is that of the active-set solution map (mi_osqp.h "adjoint derivative"), so set up the solver with polish = 1 or
tight tolerances.  A QP whose solve did not end kOptimal gets NaN gradients.

The solver holds ONE solve: backward differentiates the state its forward left, so it must run before the next forward on
the same solver (that is checked: RuntimeError) and before any other update, warm start or solve of it (that is not).
"""
import torch


class QPFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, Ax, l, u, solver):
        for t in (q, Ax, l, u):
            if not (t.is_cuda and t.dtype == torch.float64):
                raise TypeError("qp_layer: q, Ax, l and u must be CUDA float64 tensors")
        q, Ax, l, u = (t.detach().contiguous() for t in (q, Ax, l, u))
        stream = torch.cuda.current_stream().cuda_stream
        solver.update_q_device(q, stream=stream)
        solver.update_A_bounds_device(Ax, l, u, stream=stream)
        x = torch.empty((solver.B, solver.n), dtype=torch.float64, device=q.device)
        solver.solve_device(x_out=x, stream=stream)
        solver._qp_layer_forwards = getattr(solver, "_qp_layer_forwards", 0) + 1
        ctx.solver, ctx.forward_no = solver, solver._qp_layer_forwards
        ctx.shapes = (q.shape, Ax.shape, l.shape, u.shape)
        return x

    @staticmethod
    def backward(ctx, gx):
        want = ctx.needs_input_grad[:4]
        if not any(want):
            return None, None, None, None, None
        if ctx.solver._qp_layer_forwards != ctx.forward_no:
            raise RuntimeError("qp_layer: another forward ran on this solver since; its state is no longer this solve's")
        gx = gx.contiguous()
        out = [torch.empty(s, dtype=torch.float64, device=gx.device) if w else None for s, w in zip(ctx.shapes, want)]
        dq, dA, dl, du = out
        ctx.solver.adjoint_device(gx, None, dq=dq, dA=dA, dl=dl, du=du, stream=torch.cuda.current_stream().cuda_stream)
        return dq, dA, dl, du, None


def qp_layer(solver, q, Ax, l, u):
    """Solutions x [B, n] of the solver's QPs with the objective vectors q, the values Ax of A and the bounds l, u."""
    return QPFunction.apply(q, Ax, l, u, solver)
