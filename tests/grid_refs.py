"""Distance grids (mi_gomp_grid, DistanceGrid) beside tests/tilt_refs.py, tests/pair_refs.py, tests/cuboid_refs.py,
tests/capsule_refs.py, tests/gomp_refs.py and tests/dh_refs.py: a helper module of the tests, not a conftest.

A grid is a box of n[0] x n[1] x n[2] nodes (each n[k] >= 2) of spacing cell > 0, axis-aligned in the world, node (0,0,0) at
`origin`, each node holding a finite fp64 distance (positive: free space, negative: inside material), the x index fastest:
V[(iz n[1] + iy) n[0] + ix].  inv_cell = 1 / cell is one fp64 number, taken once and handed on as data.  For a ball with centre
p = fk(q_w), radius r and 3 x D position Jacobian J (include/mi_osqp.h has the same definition, restated here from it alone),
in this order of operations:

    f_k = (p_k - origin_k) * inv_cell
    inside  <=>  for every k:  f_k >= 0  and  f_k <= n_k - 1            (a NaN is outside)
    outside:  g = 0 (written), l = -1e30, u = +1e30, no say in the verdict
    inside:   i_k = min(n_k - 2, floor(f_k)),  t_k = f_k - i_k
      v_abc = V at node (i_0 + a, i_1 + b, i_2 + c)
      e_bc  = v_1bc - v_0bc,          x_bc = v_0bc + t_0 e_bc
      ey_c  = x_1c - x_0c,            y_c  = x_0c + t_1 ey_c
      ex_c  = e_0c + t_1 (e_1c - e_0c)
      phi   = y_0 + t_2 (y_1 - y_0)
      G_x   = (ex_0 + t_2 (ex_1 - ex_0)) inv_cell,  G_y = (ey_0 + t_2 (ey_1 - ey_0)) inv_cell,  G_z = (y_1 - y_0) inv_cell
      reach = offset + r,  s = phi - reach
      g_j   = G_x J[x][j] + G_y J[y][j] + G_z J[z][j]                  written whether the row is active or not
      s < margin:  l = (reach - phi) + sum_j g_j q_w[j],  u = +1e30      otherwise  l = -1e30, u = +1e30
      accepted only if s >= -ERROR

in mpmath at 50 digits and in np.float64 (gomp_refs.MPA / F64).  All other rows and their part of the verdict are tilt_refs'
(with pair_refs, cuboid_refs, capsule_refs, gomp_refs and dh_refs behind it); this module computes the grid rows and merges
them in the library's row order: per ball and waypoint the three work-space rows of a gripper ball, the lines, the capsules,
the cuboids, then the grids in the order given; the pair rows and the tilt rows follow the last block.

A row is `near` when it hangs on a threshold: |s - margin| or |s + ERROR| below NEAR, an f_k within NEAR of an integer without
being one, an f_k within NEAR of 0 or n_k - 1 without being one.  A verdict is excluded when it hangs on a near comparison.
The term scale of a bound is reach + |phi| + sum_j |g_j q_j|.

The trilinear interpolant of the distance to an axis-aligned box, sampled on a grid whose nodes fall on the box's faces, is
exact at a point p when all eight corners of p's cell lie in the region of ONE face (the face region: outside the box beyond
that face, within the face's extent in the other two coordinates) - there the distance is linear in one coordinate and the
interpolant reproduces it; beside an edge or a corner (some corner of the cell beyond two faces at once) and inside the box
across its medial planes it is not.  face_region_exact() states this for scene GX.

The scenes of tests/test_gpu_grids.py are defined here so that tests/test_grid_refs.py can check their populations on the CPU
first; the ctypes declarations of mi_gomp_scene_create_grids / mi_gomp_scene_update_grid take the library as an argument."""
import ctypes as C
import functools
import json
import os

import numpy as np

import capsule_refs as K
import cuboid_refs as X
import dh_refs as DH
import gomp_refs as G
import pair_refs as P
import tilt_refs as T

NEAR = K.NEAR
CLASSES = ("active", "none", "outside")
E20 = K.E20


def grid(origin, cell, n, values, offset=0.0, margin=0.0):
    n = [int(v) for v in n]
    values = [float(v) for v in np.asarray(values, np.float64).reshape(-1)]
    assert len(values) == n[0] * n[1] * n[2]
    return dict(origin=[float(v) for v in origin], cell=float(cell), n=n, offset=float(offset), margin=float(margin), values=values)


def node(gr, ix, iy, iz):
    return gr["values"][(iz * gr["n"][1] + iy) * gr["n"][0] + ix]


def inv_cell(gr):
    """1 / cell as the host takes it: once, in fp64."""
    return float(np.float64(1.0) / np.float64(gr["cell"]))


# ------------------------------------------------------------------ DistanceGrid::fromObstacles, restated (np.float64)

def _capsule_distance(cap, Pt):
    a, b = np.array(cap["a"], np.float64), np.array(cap["b"], np.float64)
    e = b - a
    ee = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
    if ee == 0.0:
        c = a
    else:
        t = min(1.0, max(0.0, ((Pt[0] - a[0]) * e[0] + (Pt[1] - a[1]) * e[1] + (Pt[2] - a[2]) * e[2]) / ee))
        c = a + t * e
    v = Pt - c
    return float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))


def from_obstacles(origin, cell, n, capsules, cuboids, offset=0.0, margin=0.0):
    """Every node at origin + (ix, iy, iz) cell gets the minimum over the primitives of their exact signed distance, the radius
    taken off: capsule distance - radius, cuboid signed distance (cuboid_refs.probe) - radius, in np.float64."""
    vals = []
    o, c = [np.float64(v) for v in origin], np.float64(cell)
    for iz in range(n[2]):
        for iy in range(n[1]):
            for ix in range(n[0]):
                Pt = np.array([o[0] + ix * c, o[1] + iy * c, o[2] + iz * c], np.float64)
                d = np.float64(G.INF)
                for cap in capsules:
                    d = min(d, np.float64(_capsule_distance(cap, Pt)) - np.float64(cap["radius"]))
                for cub in cuboids:
                    d = min(d, X.probe(cub, [np.float64(v) for v in Pt], G.F64)[0] - np.float64(cub["radius"]))
                vals.append(float(d))
    return grid(origin, cell, n, vals, offset, margin)


# ------------------------------------------------------------------ one grid row

def sample(gr, p, K_=G.MPA):
    """(inside, phi, G[3], f[3]) of a grid at p, in K_'s numbers; phi and G are None outside."""
    num = K_.num
    inv = num(inv_cell(gr))
    f = [(p[k] - num(gr["origin"][k])) * inv for k in range(3)]
    n = gr["n"]
    inside = all(f[k] >= 0 and f[k] <= n[k] - 1 for k in range(3))
    if not inside:
        return False, None, None, f
    i = [min(n[k] - 2, int(np.floor(float(f[k]))) if K_ is G.F64 else int(G.MP.floor(f[k]))) for k in range(3)]
    t = [f[k] - i[k] for k in range(3)]
    v = [[[num(node(gr, i[0] + a, i[1] + b, i[2] + c)) for c in (0, 1)] for b in (0, 1)] for a in (0, 1)]       # v[a][b][c]
    e = [[v[1][b][c] - v[0][b][c] for c in (0, 1)] for b in (0, 1)]                                            # e[b][c]
    x = [[v[0][b][c] + t[0] * e[b][c] for c in (0, 1)] for b in (0, 1)]
    ey = [x[1][c] - x[0][c] for c in (0, 1)]
    y = [x[0][c] + t[1] * ey[c] for c in (0, 1)]
    ex = [e[0][c] + t[1] * (e[1][c] - e[0][c]) for c in (0, 1)]
    phi = y[0] + t[2] * (y[1] - y[0])
    Gr = [(ex[0] + t[2] * (ex[1] - ex[0])) * inv, (ey[0] + t[2] * (ey[1] - ey[0])) * inv, (y[1] - y[0]) * inv]
    return True, phi, Gr, f


def grid_row(gr, p, J, q, r, K_=G.MPA):
    """The row of one (ball, waypoint, grid): a dict with vals[D], l, u, l_scale, cls, near, inside, phi, s (floats) and s_hi."""
    num = K_.num
    D = len(q)
    inside, phi, Gr, f = sample(gr, p, K_)
    near = False
    for k in range(3):
        fk = f[k]
        if not (abs(float(fk)) < 1e15):                     # NaN, inf, 1e300: outside, nowhere near a threshold
            continue
        rk = round(float(fk))
        near = near or (fk != rk and abs(fk - rk) < num(NEAR))
        for edge in (0, gr["n"][k] - 1):
            near = near or (fk != edge and abs(fk - edge) < num(NEAR))
    if not inside:
        return dict(vals=[0.0] * D, l=-G.INF, u=G.INF, l_scale=0.0, cls="outside", near=bool(near), inside=False, phi=np.nan, s=np.nan, s_hi=None)
    reach = num(gr["offset"]) + r
    s = phi - reach
    g = [Gr[0] * J[0][j] + Gr[1] * J[1][j] + Gr[2] * J[2][j] for j in range(D)]
    gq = sum((g[j] * q[j] for j in range(D)), num(0))
    margin = num(gr["margin"])
    active = s < margin
    near = near or abs(s - margin) < num(NEAR) or abs(s + num(G.ERROR)) < num(NEAR)
    low = (reach - phi) + gq if active else -num(G.INF)
    scale = reach + abs(phi) + sum((abs(g[j] * q[j]) for j in range(D)), num(0)) if active else num(0)
    return dict(vals=[float(x) for x in g], l=float(low), u=G.INF, l_scale=float(scale), cls="active" if active else "none", near=bool(near),
                inside=True, phi=float(phi), s=float(s), s_hi=s)


# ------------------------------------------------------------------ rows and verdict of a scene

_CACHE = {}


def _evaluate(D, W, chain, balls, lines, capsules, cuboids, pairs, tilts, grids, con_lo, con_hi, traj, K_, margin, bad=()):
    traj = np.ascontiguousarray(traj, np.float64)
    key = (D, W, json.dumps([chain, [{k: v for k, v in b.items() if k != "chain"} for b in balls], lines, capsules, cuboids, pairs, tilts, grids,
                             None if con_lo is None else list(con_lo), None if con_hi is None else list(con_hi)]), traj.tobytes(), K_.name, margin)
    if key in _CACHE:
        return _CACHE[key]
    base = T.with_obstacles(D, W, chain, balls, lines, capsules, cuboids, pairs, tilts, con_lo, con_hi, traj, margin, K_)
    num, err = K_.num, K_.num(G.ERROR)
    keys = ("l", "u", "l_scale", "u_scale", "cls", "ball", "w", "pair", "near", "tilt", "c")
    rows = {k: [] for k in keys + ("vals", "grid", "inside", "phi")}
    comparisons = []
    ok_grid, uncertain, definite = True, False, False
    cache = {}
    src = 0

    def copy(count):
        nonlocal src
        for _ in range(count):
            for k in keys:
                rows[k].append(base[k][src])
            rows["vals"].append(base["vals"][src])
            rows["grid"].append(-1); rows["inside"].append(False); rows["phi"].append(np.nan)
            src += 1

    for bi, ball in enumerate(balls):
        r = num(ball["radius"])
        for w in range(W):
            copy((3 if ball["gripper"] else 0) + len(lines) + len(capsules) + len(cuboids))
            if not grids:
                continue
            qf = traj[w * D:(w + 1) * D]
            p, J = G.fk_jac(ball, qf, w, K_, cache)
            q = [num(x) for x in qf]
            for gi, gr in enumerate(grids):
                e = grid_row(gr, p, J, q, r, K_)
                rows["vals"].append(e["vals"]); rows["l"].append(e["l"]); rows["u"].append(e["u"])
                rows["l_scale"].append(e["l_scale"]); rows["u_scale"].append(0.0)
                rows["cls"].append(e["cls"]); rows["ball"].append(bi); rows["w"].append(w); rows["pair"].append(-1)
                rows["near"].append(e["near"]); rows["tilt"].append(-1); rows["c"].append(np.nan)
                rows["grid"].append(gi); rows["inside"].append(e["inside"]); rows["phi"].append(e["phi"])
                if not e["inside"]:
                    continue                                   # no say in the verdict
                slack = e["s_hi"] + err                        # s >= -ERROR
                near = bool(abs(slack) < num(NEAR))
                comparisons.append(dict(kind="grid", ball=bi, w=w, idx=gi, slack=float(slack), near=near))
                if slack < 0:
                    ok_grid = False
                if near:
                    uncertain = True
                elif slack < 0:
                    definite = True
    block_rows = len(rows["l"])
    assert src == base["block_rows"]
    copy(len(base["l"]) - src)
    out = {k: (v if k == "cls" else np.array(v)) for k, v in rows.items() if k != "vals"}
    out["vals"] = np.array(rows["vals"], np.float64).reshape(len(rows["l"]), D)
    out["near"] = np.array(rows["near"], bool)
    definite = definite or (not base["ok"] and not base["verdict_excluded"])
    uncertain = uncertain or base["verdict_excluded"]
    causes = set(base["causes"]) | ({"grid"} if not ok_grid else set())
    out.update(margins=base["margins"] + comparisons, ok=bool(base["ok"] and ok_grid), causes=causes,
               verdict_excluded=bool(uncertain and not definite), block_rows=block_rows,
               tilt_rows0=block_rows + (base["tilt_rows0"] - base["block_rows"]))
    _CACHE[key] = out
    return out


def with_obstacles(D, W, chain, balls, lines, capsules, cuboids, pairs, tilts, grids, con_lo, con_hi, traj, margin=G.MARGIN, K_=G.MPA):
    """tilt_refs.with_obstacles with the grid rows behind the cuboid rows of every (ball, waypoint) block.  The arrays over the
    rows are those of tilt_refs (for a grid row: cls "active" / "none" / "outside", pair -1, tilt -1), with "grid" (the grid's
    index, -1 for the other rows), "inside" and "phi" (nan for the other rows and outside) besides; ok / causes (with "grid") /
    verdict_excluded / margins cover the whole acceptance test; block_rows = the rows before the first pair row, tilt_rows0 =
    the rows before the first tilt row."""
    return _evaluate(D, W, chain, balls, lines, capsules, cuboids, pairs, tilts, grids, con_lo, con_hi, traj, K_, margin)


# ------------------------------------------------------------------ the scenes of the GPU tests

IDENTITY = K.IDENTITY
# scenes GT / GP, exact: the TABLE model with the identity table (p = q, J = I, D = 3); every number dyadic, so every product of
# the formulas is exact in fp64 and contraction into FMAs cannot matter.  Grid A: n = (3, 4, 5), three different extents,
# cell 1/4; values multiples of 1/8 without a symmetry; the edge (0,0,0) - (1,0,0) runs from 0 to 1/4 (phi = f_x / 4 on it: the
# flips); the cell (1,2,3) holds eight equal values (G = 0).  Grid B (GT only): 2 x 2 x 2, phi = f_x / 4 everywhere, offset 1/16,
# margin 0.  GP is GT with A's margin 0 and without B.
GT_N, GT_CELL, GT_O = (3, 4, 5), 1 / 4, (0.5, -0.25, 1.0)
GT_R, GT_MA = 1 / 16, 1 / 8                                  # the ball's radius, A's margin in GT
GT_OB, GT_OFFB = (8.5, -0.25, 1.0), 1 / 16
GT_FLAT = 2.0
GT_ACCEPT = G.grid(GT_R - G.ERROR)                           # phi at which the ball has s = -ERROR from A, on the 2^-30 grid
GT_W = 8


def _gt_values():
    v = np.empty(GT_N[::-1])                                  # [iz][iy][ix]
    for iz in range(GT_N[2]):
        for iy in range(GT_N[1]):
            for ix in range(GT_N[0]):
                v[iz, iy, ix] = (8 + 3 * ix - 2 * iy + iz + ix * iy - (iy * iz) // 2 + (ix * iz * iz) % 5) / 8
    v[3:5, 2:4, 1:3] = GT_FLAT                                # the cell (1, 2, 3): eight equal values
    v[0, 0, 0], v[0, 0, 1] = 0.0, 0.25                        # the edge of the flips
    return v


def gt_grids(name):
    a = grid(GT_O, GT_CELL, GT_N, _gt_values(), 0.0, GT_MA if name == "GT" else 0.0)
    if name == "GP":
        return [a]
    vb = np.zeros((2, 2, 2))
    vb[:, :, 1] = 0.25
    return [a, grid(GT_OB, GT_CELL, (2, 2, 2), vb, GT_OFFB, 0.0)]


def _gt_point(f, origin=GT_O):
    return [origin[k] + f[k] * GT_CELL for k in range(3)]


def _gt_tour(*special):
    p = np.tile(_gt_point((10.0, 10.0, 10.0)), (GT_W, 1))     # outside both grids
    for w, f in special:
        p[w] = _gt_point(f) if len(f) == 3 else _gt_point(f[:3], GT_OB)
    return p


def _gt_trajectories(name):
    ma = GT_MA if name == "GT" else 0.0
    act = 4 * (GT_R + ma)                                    # f_x on the edge at which s = margin (phi = f_x / 4)
    acc = 4 * GT_ACCEPT
    e = 4 * E20
    actb = 4 * (GT_OFFB + GT_R)
    out = [
        _gt_tour((1, (1, 1, 1)), (2, (1, 1.5, 2.25)), (3, (2, 1, 1)), (4, (1, 3, 1)), (5, (1, 1, 4)), (6, (2, 3, 4))),   # 0: a node; a point on a cell face; the last node of each axis and of all
        _gt_tour((1, (2 + 4 * E20, 1, 1)), (2, (1, 3 + 4 * E20, 1)), (3, (1, 1, 4 + 4 * E20)), (4, (-4 * E20, 0, 0)),
                 (5, (1, -4 * E20, 1)), (6, (1, 1, -4 * E20))),                                                          # 1: 2^-20 outside on each side of each axis: zero rows, no verdict (node (0,0,0) would reject)
        _gt_tour((2, (0.25, 1.5, 2.75)), (4, (1.25, 2.5, 0.75)), (6, (1.75, 0.5, 3.25))),                                # 2: mid-cell, t = (1/4, 1/2, 3/4)
        _gt_tour((1, (1.5, 2.5, 3.5)), (3, (1, 2, 3)), (5, (2, 3, 4)), (6, (1.25, 2.75, 3.5))),                          # 3: the flat cell: G = 0
        _gt_tour((1, (act - e, 0, 0)), (2, (act + e, 0, 0))),                                                            # 4: s = margin -+ 2^-20: active | not; accepted
        _gt_tour((2, (acc + e, 0, 0))),                                                                                  # 5: s = -ERROR + 2^-20: accepted
        _gt_tour((2, (acc - e, 0, 0))),                                                                                  # 6: s = -ERROR - 2^-20: rejected, by that row alone
        _gt_tour((1, (actb - e, 0.5, 0.5, "B")), (2, (actb + e, 0.25, 1, "B")), (5, (1, 1, 1, "B"))),                    # 7: grid B (offset 1/16, margin 0): active | not; its last node
    ]
    return np.array([G._with_velocities(p) for p in out])


# scene G8: 8 joints, 2 waypoints, one ball, one grid of 2 x 2 x 2 (one cell around the whole sweep) and nothing else
G8_GRID = grid((-1.0, -1.0, -0.5), 2.0, (2, 2, 2), [0.31, 0.12, 0.27, -0.05, 0.44, 0.2, 0.38, 0.09], 0.01, 0.1)

# scene G7: the 7-joint chain of dh_refs, 40 waypoints, its 7 balls = 280 items; a line, a capsule, a cuboid, two pairs and a
# tilt beside two grids: 9 x 8 x 7 nodes from from_obstacles over a box and a capsule, and 3 x 3 x 3 that most balls are outside of
G7_BOX = X.cuboid((0.65, -0.05, 0.5), (0.1, 0.12, 0.08), 0.0, 0.0)
G7_CAP = K.capsule((0.5, 0.25, 0.4), (0.6, 0.3, 0.9), 0.03, 0.0)
G7_BALL = K.capsule((0.4, 0.2, 0.3), (0.4, 0.2, 0.3), 0.05, 0.0)


@functools.lru_cache(maxsize=None)
def g7_grids():
    return [from_obstacles((0.11, -0.34, 0.36), 0.1, (9, 8, 7), [G7_CAP], [G7_BOX], 0.01, 0.05),
            from_obstacles((0.06, -0.09, 0.51), 0.1, (3, 3, 3), [G7_BALL], [], 0.0, 0.3)]


# scene GM, the row order: tilt_refs' TM without its pairs and tilts (a gripper ball's work-space rows, two lines, a capsule, a
# cuboid) and a grid around the origin
def gm_grid():
    n = (4, 3, 5)
    v = [0.3 * ix - 0.2 * iy + 0.15 * iz + 0.05 * ix * iz - 0.4 for iz in range(n[2]) for iy in range(n[1]) for ix in range(n[0])]
    return grid((-1.1, -1.05, -1.2), 0.55, n, v, 0.02, 0.3)


# scene GX: cuboid_refs' XT with its cuboid 0 (a cube of half 1/4 around XT_O, rounded by 1/8, margin 1/8) re-sampled as a grid
# of 7 x 7 x 7 nodes, cell 1/4, whose nodes fall on the cube's faces (nodes 2 and 4 of every axis)
GX_N, GX_CELL = (7, 7, 7), 1 / 4
GX_O = tuple(c - 3 * GX_CELL for c in X.XT_O)


@functools.lru_cache(maxsize=None)
def gx_grid():
    cube = X.cuboid(X.XT_O, (X.XT_H,) * 3, X.XT_RA, 0.0)
    return from_obstacles(GX_O, GX_CELL, GX_N, [], [cube], 0.0, X.XT_MA)


def face_region_exact(p):
    """True when the trilinear interpolant of scene GX's grid is the cube's distance at p: p lies in the grid's box and every
    corner of its cell is in the region of one face - beyond the cube in exactly one coordinate (|d_k| >= h for one k, at every
    corner) and within the face's extent (|d_j| <= h) in the two others."""
    d = [p[k] - X.XT_O[k] for k in range(3)]
    f = [(p[k] - GX_O[k]) / GX_CELL for k in range(3)]
    if not all(0 <= f[k] <= GX_N[k] - 1 for k in range(3)):
        return False
    beyond = 0
    for k in range(3):
        i = min(GX_N[k] - 2, int(np.floor(f[k])))
        lo, hi = GX_O[k] + i * GX_CELL - X.XT_O[k], GX_O[k] + (i + 1) * GX_CELL - X.XT_O[k]      # the cell's extent about the centre
        if lo >= X.XT_H or hi <= -X.XT_H:
            beyond += 1
        elif not (lo >= -X.XT_H and hi <= X.XT_H):
            return False
    return beyond == 1 and any(abs(v) >= X.XT_H for v in d)


SCENES = ("GT", "GP", "G8", "G7", "GM")
EXACT = ("GT", "GP")


@functools.lru_cache(maxsize=None)
def scene(name):
    """name: one of SCENES or "GX".  A dict as tilt_refs.scene gives, with "grids" besides."""
    none = dict(lines=[], capsules=[], cuboids=[], pairs=[], tilts=[], con_lo=None, con_hi=None, margin=G.MARGIN)
    if name in ("GT", "GP"):
        return dict(none, name=name, D=3, W=GT_W, chain=None, balls=[G._ball(G.TABLE, 0, GT_R, IDENTITY)], grids=gt_grids(name), trajs=_gt_trajectories(name))
    if name == "G8":
        return dict(none, name=name, D=8, W=2, chain=DH.C8, balls=[DH.chain_ball(DH.C8, 8, (0, 0, 0.02), 0, 0.04)], grids=[G8_GRID],
                    trajs=DH._c8_trajectories())
    if name == "G7":
        t7 = T.scene("T7")
        return dict(t7, name=name, cuboids=X.X7_CUBOIDS[:1], pairs=t7["pairs"][:2], tilts=t7["tilts"][:1], grids=g7_grids())
    if name == "GM":
        tm = T.scene("TM")
        return dict(tm, name=name, balls=tm["balls"][:2], chain=None, pairs=[], tilts=[], grids=[gm_grid()])
    if name == "GX":
        xt = X.scene("XT")
        return dict(none, name=name, D=3, W=xt["W"], chain=None, balls=xt["balls"], grids=[gx_grid()], trajs=xt["trajs"])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene_reference(name, K_=G.MPA):
    """with_obstacles of the scene's eight trajectories."""
    s = scene(name)
    return [with_obstacles(s["D"], s["W"], s["chain"], s["balls"], s["lines"], s["capsules"], s["cuboids"], s["pairs"], s["tilts"], s["grids"],
                           s["con_lo"], s["con_hi"], t, s["margin"], K_) for t in s["trajs"]]


@functools.lru_cache(maxsize=None)
def fp64_error(name):
    """dh_refs.fp64_error for the scenes of this module: the np.float64 evaluation of the formulas against the mpmath one."""
    ev = eb = 0.0
    for hi, lo in zip(scene_reference(name), scene_reference(name, G.F64)):
        v, b = DH.row_distance(hi, lo)
        ev, eb = max(ev, v), max(eb, b)
    return ev, eb


def gpu_tolerance(name):
    """The project's rule (cuboid_refs.gpu_tolerance): 32 x fp64_error, never looser than 1e-13.  (0, 0) for the exact scenes."""
    ev, eb = fp64_error(name)
    return min(32 * ev, 1e-13), min(32 * eb, 1e-13)


@functools.lru_cache(maxsize=None)
def scene_batch(name, over_allocate=False):
    """pair_refs.scene_problem for the scene's eight trajectories: a grid takes a row per (ball, waypoint) as a cuboid does."""
    s = scene(name)
    D, W = s["D"], s["W"]
    ends = s["trajs"][:, (W - 3) * D:(W - 2) * D] if W >= 4 else None
    return P.scene_problem(D, W, s["balls"], len(s["lines"]) + len(s["capsules"]) + len(s["cuboids"]) + len(s["grids"]),
                           len(s["pairs"]) + len(s["tilts"]), 8, over_allocate, starts=s["trajs"][:, :D], ends=ends)


def populations(name):
    """Counts a test can assert on and print: grid rows per class and grid, rejecting grid rows, verdicts, causes, exclusions."""
    s, ref = scene(name), scene_reference(name)
    ng = len(s["grids"])
    cells = {c: np.zeros(ng, int) for c in CLASSES}
    rejecting = np.zeros(ng, int)
    near = rows = 0
    causes, only_grid = {}, 0
    for e in ref:
        for k in range(len(e["l"])):
            near += bool(e["near"][k])
            if e["grid"][k] < 0:
                continue
            cells[e["cls"][k]][int(e["grid"][k])] += 1
            rows += 1
        for m in e["margins"]:
            if m["kind"] == "grid":
                rejecting[m["idx"]] += bool(m["slack"] < 0)
        for c in e["causes"]:
            causes[c] = causes.get(c, 0) + 1
        only_grid += e["causes"] == {"grid"}
    return dict(cells=cells, rejecting=rejecting, near=near, grid_rows=rows, accepted=sum(e["ok"] for e in ref), rejected=sum(not e["ok"] for e in ref),
                causes=causes, rejected_by_a_grid_alone=only_grid, verdicts_excluded=sum(e["verdict_excluded"] for e in ref),
                near_comparisons=sum(m["near"] for e in ref for m in e["margins"]))


# ------------------------------------------------------------------ the known answers in tests/golden/grid_kats.json

KAT_SCENES = ("GT", "GP", "GM")


def kats_now():
    """What tests/golden/grid_kats.json holds, computed now: per scene the grids (as the C++ test builds them) and per trajectory
    the trajectory, the rows (vals, l, u as JSON numbers: the shortest decimal that reads back as the same double) and the verdict
    of the mpmath reference; for GT besides the samples (inside, phi, G) of grid 0 at every waypoint, and the nodes of G7's
    first grid as from_obstacles gives them."""
    out = {}
    for name in KAT_SCENES:
        s = scene(name)
        out[name] = dict(grids=s["grids"], cases=[dict(traj=[float(x) for x in t], vals=[[float(x) for x in row] for row in e["vals"]],
                                                       l=[float(x) for x in e["l"]], u=[float(x) for x in e["u"]], ok=bool(e["ok"]))
                                                  for t, e in zip(s["trajs"], scene_reference(name))])
    s = scene("GT")
    samples = []
    for t in s["trajs"]:
        for w in range(s["W"]):
            p = [G.MP.mpf(float(x)) for x in t[w * 3:(w + 1) * 3]]
            inside, phi, Gr, _ = sample(s["grids"][0], p)
            samples.append(dict(p=[float(x) for x in p], inside=bool(inside), phi=float(phi) if inside else 0.0,
                                grad=[float(x) for x in Gr] if inside else [0.0, 0.0, 0.0]))
    out["GT"]["samples"] = samples
    g7 = g7_grids()[0]
    out["from_obstacles"] = dict(origin=g7["origin"], cell=g7["cell"], n=g7["n"], box=G7_BOX, capsule=G7_CAP, values=g7["values"])
    return out


def kats_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_kats.json")


def load_kats():
    with open(kats_path()) as f:
        return json.load(f)


# ------------------------------------------------------------------ ctypes: mi_gomp_scene_create_grids (tests only)

class Grid(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("cell", C.c_double), ("n", C.c_int32 * 3), ("reserved", C.c_int32), ("offset", C.c_double),
                ("margin", C.c_double), ("values", C.POINTER(C.c_double))]


def c_grids(grids, null_values=()):
    """(array, keep): the structs and the arrays their `values` point to (keep them alive for the call)."""
    arr = (Grid * max(len(grids), 1))()
    keep = []
    for k, gr in enumerate(grids):
        for i in range(3):
            arr[k].origin[i], arr[k].n[i] = gr["origin"][i], gr["n"][i]
        arr[k].cell, arr[k].offset, arr[k].margin = gr["cell"], gr["offset"], gr["margin"]
        if k not in null_values:
            v = np.ascontiguousarray(gr["values"], np.float64)
            keep.append(v)
            arr[k].values = v.ctypes.data_as(C.POINTER(C.c_double))
    return arr, keep


def declare(L):
    T.declare(L)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    L.mi_gomp_scene_create_grids.argtypes = [C.POINTER(vp), vp, C.c_int64, C.c_int64, C.POINTER(DH.Chain), C.c_int64, C.POINTER(G.Ball), C.c_int64,
                                             C.POINTER(G.Line), C.c_int64, C.POINTER(K.Capsule), C.c_int64, C.POINTER(X.Cuboid), C.c_int64, C.POINTER(P.Pair),
                                             C.c_int64, C.POINTER(T.Tilt), C.c_int64, C.POINTER(Grid), dp, dp]
    L.mi_gomp_scene_create_grids.restype = C.c_int
    L.mi_gomp_scene_update_grid.argtypes = [vp, C.c_int64, dp]
    L.mi_gomp_scene_update_grid.restype = C.c_int
    return L


def create_grids(L, handle, D, W, ch, balls, lines, capsules, cuboids, pairs, tilts, grids, con_lo=None, con_hi=None, n_grids=None, null_grids=False,
                 null_values=()):
    """(rc, scene pointer) of mi_gomp_scene_create_grids; ch: a Chain, a chain dict or None.  n_grids / null_grids / null_values
    override what is passed for the grid count, the array and single grids' values (the refusals).  The pointer starts as a value
    that is not NULL, so a refusal shows that it was cleared."""
    ptr = C.c_void_p(1)
    lo = None if con_lo is None else np.ascontiguousarray(con_lo, np.float64)
    hi = None if con_hi is None else np.ascontiguousarray(con_hi, np.float64)
    cc = DH.c_chain(ch) if isinstance(ch, dict) else ch
    arr, keep = c_grids(grids, null_values)
    rc = L.mi_gomp_scene_create_grids(C.byref(ptr), handle, D, W, None if cc is None else C.byref(cc), len(balls), G.c_balls(balls), len(lines),
                                      G.c_lines(lines), len(capsules), K.c_capsules(capsules), len(cuboids), X.c_cuboids(cuboids),
                                      len(pairs), P.c_pairs(pairs), len(tilts), T.c_tilts(tilts), len(grids) if n_grids is None else n_grids,
                                      None if null_grids else arr, G._dp(lo), G._dp(hi))
    del keep
    return rc, ptr


class GridScene(G.GompScene):
    """gomp_refs.GompScene made by mi_gomp_scene_create_grids."""

    def __init__(self, L, solver, D, W, ch, balls, lines, capsules, cuboids, pairs, tilts, grids, con_lo, con_hi):
        self.L, self.solver = declare(L), solver
        self.rc, self.ptr = create_grids(L, solver._h, D, W, ch, balls, lines, capsules, cuboids, pairs, tilts, grids, con_lo, con_hi)

    def update_grid(self, k, values):
        v = np.ascontiguousarray(values, np.float64)
        return self.L.mi_gomp_scene_update_grid(self.ptr, k, G._dp(v))
