"""A batch of QPs as a differentiable torch layer: x*(q, A, l, u), or x*(q, A, l, u, P) when the values of P are given.

    x = qp_layer(solver, q, Ax, l, u)        # CUDA float64: q [B, n], Ax [B, nnzA] (CSC order of A), l, u [B, m]
    loss(x).backward()                       # q.grad, Ax.grad, l.grad, u.grad

    x = qp_layer(solver, q, Ax, l, u, Px=Px) # Px [B, nnzPu]: triu(P) in the order of solver.P_upper_pattern()
    loss(x).backward()                       # ... and Px.grad, on the same pattern: a gradient step on Px can be fed back

Without Px the forward is update_q_device, update_A_bounds_device, solve_device on the given BatchSolver and P stays what the
solver holds.  With Px it is update_q_device, ONE update_P_A_bounds_device (one equilibration and one refactorisation for P, A
and the bounds), solve_device; nothing crosses PCIe either way.  Backward is one BatchSolver.adjoint_device call that asks
only for the gradients autograd needs (dP among them when Px requires one).  No solver logic lives here: the derivative is
that of the active-set solution map (mi_osqp.h "adjoint derivative"), so set up the solver with polish = 1 or tight
tolerances.  A QP whose solve did not end kOptimal gets NaN gradients.  Px.grad is the derivative with respect to the stored
value of triu(P), which stands for (i, j) and (j, i); a P that is not positive semidefinite ends its QP as kNonConvex.

The solver holds ONE solve: backward differentiates the state its forward left, so it must run before the next forward on
the same solver (that is checked: RuntimeError) and before any other update, warm start or solve of it (that is not).
"""
import torch


class QPFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, Ax, l, u, solver, Px=None):
        given = (q, Ax, l, u) if Px is None else (q, Ax, l, u, Px)
        for t in given:
            if not (t.is_cuda and t.dtype == torch.float64):
                raise TypeError("qp_layer: q, Ax, l, u and Px must be CUDA float64 tensors")
        q, Ax, l, u = (t.detach().contiguous() for t in (q, Ax, l, u))
        stream = torch.cuda.current_stream().cuda_stream
        solver.update_q_device(q, stream=stream)
        if Px is None:
            solver.update_A_bounds_device(Ax, l, u, stream=stream)
        else:
            Px = Px.detach().contiguous()
            solver.update_P_A_bounds_device(Px, Ax, l, u, stream=stream)
        x = torch.empty((solver.B, solver.n), dtype=torch.float64, device=q.device)
        solver.solve_device(x_out=x, stream=stream)
        solver._qp_layer_forwards = getattr(solver, "_qp_layer_forwards", 0) + 1
        ctx.solver, ctx.forward_no = solver, solver._qp_layer_forwards
        ctx.shapes = (q.shape, Ax.shape, l.shape, u.shape, None if Px is None else Px.shape)
        return x

    @staticmethod
    def backward(ctx, gx):
        want = ctx.needs_input_grad[:4] + (ctx.needs_input_grad[5],)
        if not any(want):
            return None, None, None, None, None, None
        if ctx.solver._qp_layer_forwards != ctx.forward_no:
            raise RuntimeError("qp_layer: another forward ran on this solver since; its state is no longer this solve's")
        gx = gx.contiguous()
        out = [torch.empty(s, dtype=torch.float64, device=gx.device) if w else None for s, w in zip(ctx.shapes, want)]
        dq, dA, dl, du, dP = out
        extra = {} if ctx.shapes[4] is None else dict(dP=dP)       # (without Px: the call of a layer that has no P input)
        ctx.solver.adjoint_device(gx, None, dq=dq, dA=dA, dl=dl, du=du, stream=torch.cuda.current_stream().cuda_stream, **extra)
        return dq, dA, dl, du, None, dP


def qp_layer(solver, q, Ax, l, u, Px=None):
    """Solutions x [B, n] of the solver's QPs with the objective vectors q, the values Ax of A and the bounds l, u - and, when
    Px is given, the values Px [B, nnzPu] of triu(P) (order of solver.P_upper_pattern())."""
    return QPFunction.apply(q, Ax, l, u, solver, Px)
