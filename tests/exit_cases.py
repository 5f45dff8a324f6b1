"""Problem families that end a solve with each exit code (a helper module of the tests, not a conftest).

Plain numpy / scipy: nothing here solves anything and nothing touches the oracle or the GPU (the one import from the
package is its data-generation module, problems.py, where the dual infeasible construction lives for the stress script).  A family takes a
batch dict of problems.random_box_qp / problems.grid_qp and one kind per QP and returns a NEW batch dict with the SAME
shared pattern: only values and bounds change (a batch has one pattern; zeros that a construction writes into P stay
explicit entries of Px).  Both generators put the identity on top of A (row k < n is the box of variable k), which the
constructions below rely on and `assert_identity_block` verifies.

Kinds
  feas  the QP as generated: P strictly diagonally dominant (random_box_qp) or Laplacian + I (grid_qp), every row boxed
        around 0, so x = 0 is feasible and the minimiser is unique.
  pinf  primal infeasible by an interval argument (make_pinf / grid_pinf).
  dinf  dual infeasible (unbounded below) along the ray d = -e_0 (make_dinf).

The inaccurate codes come from the same families at loose iteration limits: `ALL_CODES` names, per slot of one batch,
the base QP, the kind and the size of the dual-infeasible push for which ONE handle (one max_iter, one set of
tolerances) ends with all seven statuses 1, 2, 3, 4, -2, -3, -4.  tests/test_exit_case_references.py pins every one of
them on the CPU oracle, checks each construction without the oracle and checks that no status moves when max_iter moves
by +-1 and the tolerances by +-1 %."""
import numpy as np

from osqp_solver_amd import problems as PR

INF = 1e30
KINDS = ("feas", "pinf", "dinf")


def assert_identity_block(pr):
    """Rows 0..n-1 of A are the identity (one entry per row, on the diagonal, value 1 for every QP)."""
    n = pr["n"]
    A = pr["A"].tocoo()
    top = A.row < n
    assert np.count_nonzero(top) == n and np.array_equal(np.sort(A.row[top]), np.arange(n))
    assert np.array_equal(A.row[top], A.col[top])
    csc_top = pr["A"].indices < n                      # CSC order = order of the value arrays
    assert np.all(pr["Ax"][:, csc_top] == 1.0)


def take(pr, idx):
    """The batch made of QPs `idx` of pr (an index may repeat), same pattern."""
    idx = np.asarray(idx, np.int64)
    out = dict(pr)
    for k in ("Px", "Ax", "q", "l", "u"):
        out[k] = None if pr[k] is None else pr[k][idx].copy()
    return out


def _copy(pr):
    return take(pr, np.arange(pr["Ax"].shape[0]))


def _a_row(pr, b, row):
    """(columns, values) of one row of A of QP b."""
    A = pr["A"]
    cols = np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    sel = A.indices == row
    return cols[sel], pr["Ax"][b, sel]


def make_pinf(pr, b, row=None):
    """QP b becomes primal infeasible, in place.  Row `row` of A (default: row n, the first one below the identity) gets
    bounds no point of the box reaches: every x the identity rows admit has |x_k| <= max(|l_k|, |u_k|), so
    |a'x| <= cap = sum_k |a_k| max(|l_k|, |u_k|), and the row now asks for a'x in [cap + 1, cap + 2].  The feasible set is
    empty whatever P and q are."""
    n = pr["n"]
    row = n if row is None else row
    cols, vals = _a_row(pr, b, row)
    cap = float(np.sum(np.abs(vals) * np.maximum(np.abs(pr["l"][b, cols]), np.abs(pr["u"][b, cols]))))
    pr["l"][b, row], pr["u"][b, row] = cap + 1.0, cap + 2.0


def grid_pinf(pr, b=0):
    """grid_qp, in place: x0 in [1, 2], x1 in [-2, -1], but row n of A, the first difference x1 - x0, in [0.5, 1].  Over the
    two boxes x1 - x0 ranges over [-4, -2], which misses [0.5, 1] (the same interval argument as make_pinf, with the
    boxes moved instead of the row)."""
    n = pr["n"]
    cols, vals = _a_row(pr, b, n)
    assert sorted(cols.tolist()) == [0, 1] and vals[np.argsort(cols)].tolist() == [-1.0, 1.0]
    pr["l"][b, 0], pr["u"][b, 0] = 1.0, 2.0
    pr["l"][b, 1], pr["u"][b, 1] = -2.0, -1.0
    pr["l"][b, n], pr["u"][b, n] = 0.5, 1.0


def make_dinf(pr, b, push=1.0):
    """QP b becomes dual infeasible (unbounded below), in place, along d = -e_0:
      * every stored entry of row 0 and of column 0 of P is set to 0.0 and STAYS an entry of Px, so P d = 0.  What is left
        of P is a principal submatrix of a positive definite matrix bordered by zeros: still positive semidefinite.
      * q[0] = push > 0, so q'd = -push < 0;
      * every row of A that holds column 0 becomes free (l = -1e30, u = 1e30: a change of bounds only), so A d is zero in
        every row that still has a finite bound: d is in the recession cone of the feasible set.
    The other rows still admit x = 0, so the QP is feasible and x = t d is feasible with cost -push t -> -inf.  This holds
    for random_box_qp and for grid_qp alike (grid_qp: P = Laplacian + I loses the curvature of x0 only; the rows freed are
    the box of x0 and the two differences that hold it).  A small `push` makes the certificate slow to show: that is how
    kDualInfeasibleInaccurate is reached."""
    PR.make_dual_infeasible(pr, b, push)        # (shared with scripts/stress_settings.py, which must not depend on tests/)


def apply_kinds(pr, kinds, push=1.0, grid=False):
    """New batch dict: QP b of pr turned into kinds[b] (len(kinds) == B).  push: scalar or one value per QP (read for the
    dinf QPs only).  grid=True uses grid_pinf for `pinf`."""
    B = pr["Ax"].shape[0]
    assert len(kinds) == B and all(k in KINDS for k in kinds)
    out = _copy(pr)
    push = np.broadcast_to(np.asarray(push, float), (B,))
    for b, k in enumerate(kinds):
        if k == "pinf":
            (grid_pinf if grid else make_pinf)(out, b)
        elif k == "dinf":
            make_dinf(out, b, float(push[b]))
    return out


def rotations(base, B):
    """The len(base) cyclic shifts of `base`, each repeated to B kinds: every kind sits at every class position of a tile
    of len(base) QPs once."""
    return [[base[(i + s) % len(base)] for i in range(B)] for s in range(len(base))]


def perturbations(settings):
    """The settings around `settings` under which a chosen case must keep its oracle status: max_iter -1 / 0 / +1 times
    (all four tolerances x 0.99 / 1 / 1.01 together), and each tolerance alone x 0.99 / 1.01.  `settings` names all four
    tolerances and max_iter explicitly."""
    tol = ("eps_abs", "eps_rel", "eps_prim_inf", "eps_dual_inf")
    out = []
    for dm in (-1, 0, 1):
        for f in (0.99, 1.0, 1.01):
            if dm == 0 and f == 1.0:
                continue
            out.append(dict(settings, max_iter=settings["max_iter"] + dm, **{k: settings[k] * f for k in tol}))
    for k in tol:
        for f in (0.99, 1.01):
            out.append(dict(settings, **{k: settings[k] * f}))
    return out


# ---- one batch, all seven statuses ----------------------------------------------------------------------------------------
# Base problem of every small-QP case: problems.random_box_qp(BASE_B, **BASE_SHAPE).  A slot is (kind, base QP, push,
# expected oracle status).  Chosen on the CPU oracle: eps_abs = eps_rel = 1e-5 leaves some feasible QPs short of
# convergence at max_iter = 147 (2 or -2), eps_dual_inf = 1e-8 with a weak push leaves the ray short of its exact test (4),
# and the primal infeasible QPs need 150 to 875 iterations for their exact certificate (3 or -2 before that).  147 is not a
# multiple of check_termination = 25: the last regular check is at 125, the closing one at 147.  Every slot keeps its
# status under `perturbations` (test_exit_case_references.py verifies that, and the statuses themselves).
BASE_B = 12
BASE_SHAPE = dict(n=96, mg=64, nnz_per_row=6)
ALL_CODES_TOL = dict(eps_abs=1e-5, eps_rel=1e-5, eps_prim_inf=1e-4, eps_dual_inf=1e-8, max_iter=147)
_S10 = [("feas", 0, 1.0, 1), ("pinf", 0, 1.0, -2), ("dinf", 0, 1.0, -4), ("pinf", 3, 1.0, 3), ("feas", 5, 1.0, 2),
        ("dinf", 2, 0.003, 4), ("pinf", 1, 1.0, -3), ("feas", 1, 1.0, 1), ("dinf", 0, 0.001, 4), ("pinf", 5, 1.0, 3),
        ("pinf", 2, 1.0, -2), ("dinf", 1, 1.0, -4), ("pinf", 6, 1.0, -3)]
ALL_CODES = {
    # name: (settings on top of ALL_CODES_TOL, slots)
    "s10": (dict(scaling=10), _S10),
    "s10_st": (dict(scaling=10, scaled_termination=1), [s if s[:2] != ("pinf", 5) else ("pinf", 4, 1.0, 3) for s in _S10]),
    "ct0": (dict(scaling=10, check_termination=0), _S10),          # only the closing check runs
    "s0": (dict(scaling=0),
           [("feas", 1, 1.0, 1), ("pinf", 0, 1.0, -2), ("dinf", 0, 1.0, -4), ("pinf", 8, 1.0, 3), ("feas", 0, 1.0, 2),
            ("dinf", 0, 0.003, 4), ("pinf", 1, 1.0, -3), ("feas", 6, 1.0, 1), ("dinf", 2, 0.003, 4), ("feas", 2, 1.0, 2),
            ("pinf", 2, 1.0, -2), ("dinf", 1, 1.0, -4), ("pinf", 6, 1.0, -3)]),
}
STATUSES = (1, 2, 3, 4, -2, -3, -4)


def all_codes_batch(base, name, slots=None):
    """(batch dict, settings, expected statuses) of ALL_CODES[name], built from base = random_box_qp(BASE_B, **BASE_SHAPE).
    slots: positions of the spec to keep (default all, B = 13: a ragged last tile for tiles of 2 and of 4)."""
    extra, spec = ALL_CODES[name]
    if slots is not None:
        spec = [spec[i] for i in slots]
    pr = apply_kinds(take(base, [s[1] for s in spec]), [s[0] for s in spec], push=[s[2] for s in spec])
    return pr, dict(ALL_CODES_TOL, **extra), [s[3] for s in spec]


# ---- exact codes at ordinary settings: kinds rotated through the tile positions ------------------------------------------
ROTATED = ("feas", "pinf", "dinf", "feas")
EXACT_B = 11                                   # ragged last tile for tiles of 2 and of 4
EXACT_SETTINGS = {
    "default": {}, "s0": dict(scaling=0), "st": dict(scaled_termination=1), "s0_st": dict(scaling=0, scaled_termination=1),
    "inf_tol": dict(eps_prim_inf=1e-6, eps_dual_inf=1e-7),      # non-default certificates: later exits, counts follow the oracle
}
KIND_STATUS = {"feas": 1, "pinf": -3, "dinf": -4}
WHOLE_TILE_INFEASIBLE = ["pinf", "dinf", "dinf", "pinf", "feas", "feas", "pinf", "feas", "dinf", "feas", "feas"]


def exact_batches(base):
    """[(name, batch, kinds)]: the four cyclic shifts of ROTATED over EXACT_B QPs of base, and one batch whose first tile
    (of 1, 2 or 4 QPs) is infeasible throughout."""
    sub = take(base, np.arange(EXACT_B))
    out = [(f"rot{s}", apply_kinds(sub, k), k) for s, k in enumerate(rotations(ROTATED, EXACT_B))]
    out.append(("tile_inf", apply_kinds(sub, WHOLE_TILE_INFEASIBLE), WHOLE_TILE_INFEASIBLE))
    return out


# ---- the grid pattern (dataflow form of a single QP) ---------------------------------------------------------------------
# (kind, push, settings, expected oracle status) on problems.grid_qp(40); the inaccurate ray: a closing check before the
# first regular one (max_iter < 25) with the certificate tolerance tightened or the push weakened.
_GT = dict(eps_abs=1e-5, eps_rel=1e-5, eps_prim_inf=1e-4)
GRID_CASES = {
    "pinf": ("pinf", 1.0, {}, -3),
    "dinf": ("dinf", 1.0, {}, -4),
    "dinf_s0": ("dinf", 1.0, dict(scaling=0), -4),
    "dinf_inacc": ("dinf", 1.0, dict(_GT, eps_dual_inf=1e-6, max_iter=20), 4),
    "dinf_inacc_weak": ("dinf", 0.1, dict(_GT, eps_dual_inf=1e-4, max_iter=5), 4),
    "maxiter": ("feas", 1.0, dict(_GT, eps_dual_inf=1e-4, max_iter=60), -2),
}


def grid_case(grid, name):
    kind, push, settings, status = GRID_CASES[name]
    return apply_kinds(grid, [kind], push=push, grid=True), dict(settings), status
