"""Grasp goals through the C++ layer of include/mi_osqp/gomp.hpp (tests/cpp/gomp_goal.cpp).

CPU : the program is built with -fsanitize=address,undefined and run as a program.  ConstraintBuilder<3> with goals on scenes
      GF, GX and GM of tests/goal_refs.py against the known answers of tests/golden/goal_kats.json (values and bounds within
      1e-12 of their term scale, +-1e30 exact, the verdicts of the goals and of the whole scene equal; GX, exact by construction,
      bit for bit); the allocation (4 |goals| rows more, in the columns of the goal's waypoint, the empty rows behind them); a
      builder with an empty goal list against the eight-argument one, bit for bit; setGoalTarget on a copied template; goalOK at
      the 1 mm and the 1 mrad.  The reach problem (7 joints, 20 waypoints: the gripper ball into a box of 30 x 30 x 5 mm with
      the tool axis within 10 degrees of straight down) through the three planners on oracle backends: the same exit codes,
      solves and trajectories, bit for bit; the accepted end point inside tol + 1 mm and max_angle + 1 mrad; the fixed-end plan
      bit for bit what the parent commit planned.
      The first QP of the goal run against the first QP of the fixed-end run, both linearised at goalWarmStart, whose third-last
      waypoint is the seed and satisfies the goal: the goal QP's feasible set holds the fixed-end QP's, so its oracle objective
      must not exceed the other's by more than 10 x the change of the fixed-end objective between the oracle tolerances 1e-5 and
      1e-7.  Measured: fixed end 0.011586083718 (1e-5) and 0.011586083583 (1e-7), so the margin is 1.3e-09; goal 0.002772278827.
GPU : (built without the sanitizers) the continuous driver with the SQP step on the device (mi_gomp_scene_create_goals, the
      targets set per arrival with mi_gomp_scene_set_goal_values) against the host-assembling one on the reach problem: same exit
      codes and counters, trajectories within 1e-6 - max |dx| is printed -, then the same planner to a fixed end; the example."""
import os
import re
import subprocess

import numpy as np
import pytest

import goal_refs as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out, sanitize):
    import osqp_solver_amd as M
    from oracle import oracle as O
    M.lib(); O.lib()
    libdir, ordir = os.path.join(ROOT, "osqp-solver_amd"), os.path.join(ROOT, "oracle", "_build")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2"] + san + ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gomp_goal.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-L" + ordir, "-loracle_osqp", "-fopenmp", "-pthread",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + ordir], check=True)
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("gomp_goal") / "gomp_goal_san", True)


def _env():
    # the libraries the program links were not built with the sanitizers: what they keep until exit is not this program's leak
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def _clean(r, word):
    return r.returncode == 0 and word in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def _scene_file(s, path):
    hx = lambda vals: " ".join(float(v).hex() for v in vals)
    inf = 1e30
    ch = s["chain"]
    text = [str(len(ch["a"]))] + [hx([ch["a"][i], ch["d"][i], ch["alpha"][i], ch["theta0"][i]]) for i in range(len(ch["a"]))]
    text += [str(len(s["balls"]))] + [f"{b['model']} {int(b['gripper'])} {hx([b['radius']])} {hx((list(b['param']) + [0.0] * 9)[:9])}" for b in s["balls"]]
    text += [str(len(s["lines"]))] + [f"{hx(ln['dir'])} {hx(ln['point'])} {int(bool(ln.get('below')))}" for ln in s["lines"]]
    text += [str(len(s["capsules"]))] + [f"{hx(c['a'])} {hx(c['b'])} {hx([c['radius'], c['margin']])}" for c in s["capsules"]]
    text += [str(len(s["cuboids"]))] + [f"{hx(c['centre'])} {hx(c['axes'])} {hx(c['half'])} {hx([c['radius'], c['margin']])}" for c in s["cuboids"]]
    text += [str(len(s["pairs"]))] + [f"{p['a']} {p['b']} {hx([p['margin']])}" for p in s["pairs"]]
    text += [str(len(s["tilts"]))] + [f"{t['frame']} {hx(t['axis'])} {hx(t['ref'])} {hx([t['max_angle'], t['margin']])}" for t in s["tilts"]]
    text += [str(len(s["grids"]))] + [f"{hx(g['origin'])} {hx([g['cell']])} {g['n'][0]} {g['n'][1]} {g['n'][2]} {hx([g['offset'], g['margin']])} {hx(g['values'])}"
                                      for g in s["grids"]]
    text += [str(len(s["goals"]))] + [f"{g['ball']} {g['waypoint']} {g['frame']} {hx(g['axis'])}" for g in s["goals"]]
    text += [hx(s["con_lo"] if s["con_lo"] is not None else [-inf] * 3), hx(s["con_hi"] if s["con_hi"] is not None else [inf] * 3)]
    text += [str(s["W"]), str(len(s["trajs"]))]
    for per, t in zip(s["values"], s["trajs"]):
        text += [" ".join(hx(v["point"] + v["tol"] + v["ref"] + [v["max_angle"]]) for v in per), hx(t)]
    path.write_text("\n".join(text) + "\n")


@pytest.mark.parametrize("name", Q.KAT_SCENES)
def test_constraint_builder_and_verdicts_against_the_known_answers(exe, name, tmp_path):
    s, kats = Q.scene(name), Q.load_kats()[name]
    ref = Q.scene_reference(name)
    D = s["D"]
    assert D == 3 and kats["goals"] == s["goals"]
    path = tmp_path / "scene.txt"
    _scene_file(s, path)
    r = subprocess.run([exe, "rows", str(path)], capture_output=True, text=True, timeout=300, env=_env())
    assert _clean(r, "ROWS OK"), r.stdout[-2000:] + r.stderr[-4000:]
    rows, verdicts, before = {}, {}, {}
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "R":
            rows.setdefault(int(t[1]), []).append([float.fromhex(v) for v in t[3:]])
        elif t[0] == "V":
            verdicts[int(t[1])] = (bool(int(t[2])), bool(int(t[3])))
        elif t[0] == "N":
            before[int(t[1])] = int(t[2])
    worst_v = worst_b = 0.0
    for b, kat in enumerate(kats["cases"]):
        got = np.array(rows[b])
        vals, l, u = np.array(kat["vals"]), np.array(kat["l"]), np.array(kat["u"])
        assert got.shape == (4 * len(s["goals"]), D + 2) and before[b] == kat["rows_before"]
        assert verdicts[b] == (kat["ok_goal"], kat["ok"]), b
        worst_v = max(worst_v, float(np.max(np.abs(got[:, :D] - vals))))
        assert np.max(np.abs(got[:, :D] - vals)) <= 1e-12
        g0 = ref[b]["goal_rows0"]
        for side, dev, want in (("l", got[:, D], l), ("u", got[:, D + 1], u)):
            sc = ref[b][side + "_scale"][g0:]
            inf = sc == 0
            assert np.array_equal(dev[inf].view(np.int64), want[inf].view(np.int64)), (b, side)      # +-1e30 exactly
            assert np.all(np.abs(want[inf]) == 1e30)
            fin = ~inf
            eb = float(np.max(np.abs(dev[fin] - want[fin]) / sc[fin], initial=0.0))
            worst_b = max(worst_b, eb)
            assert eb <= 1e-12, (b, side, eb)
        if name in Q.EXACT:                                                   # exact by construction
            assert np.array_equal(got[:, :D], vals) and np.array_equal(got[:, D], l) and np.array_equal(got[:, D + 1], u)
    print(f"\nscene {name}: ConstraintBuilder against the known answers: values {worst_v:.3e}, bounds {worst_b:.3e} of their term scale")


def test_goal_ok_dh_goal_and_the_warm_start(exe):
    r = subprocess.run([exe, "checks"], capture_output=True, text=True, timeout=60, env=_env())
    assert _clean(r, "CHECKS OK"), r.stdout + r.stderr[-4000:]


def test_the_reach_problem_through_the_three_planners_on_oracle_backends(exe, tmp_path):
    """See the module's docstring for the first-QP comparison and its measured margin."""
    plain = tmp_path / "plain.txt"
    plain.write_text(" ".join(Q.load_kats()["plain_plan"]["x"]) + "\n")
    r = subprocess.run([exe, "plan", str(plain)], capture_output=True, text=True, timeout=600, env=_env())
    assert _clean(r, "PLAN OK"), r.stdout + r.stderr[-4000:]
    print("\n" + r.stdout)
    assert "fixed-end plan against the kept one: 140 numbers, bit for bit" in r.stdout
    assert r.stdout.count("trajectories bit for bit the sequential planner's") == 2
    m = re.search(r"first QP: fixed end ([0-9.]+) \(eps 1e-5\), ([0-9.]+) \(eps 1e-7\), goal ([0-9.]+) \(eps 1e-7\); margin ([0-9.e+-]+)", r.stdout)
    f5, f7, g7, margin = (float(v) for v in m.groups())
    assert abs(margin - 10 * abs(f5 - f7)) <= 1e-10 and g7 <= f7 + 10 * abs(f5 - f7)


@pytest.mark.gpu
def test_continuous_planner_with_a_goal_device_against_host_assembly(tmp_path):
    exe = _build(tmp_path / "gomp_goal", False)
    r = subprocess.run([exe, "cont"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CONT OK" in r.stdout and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    print("\n" + r.stdout)


@pytest.mark.gpu
def test_grasp_gomp_example_plans_both_ways(tmp_path):
    import osqp_solver_amd as M
    M.lib()
    libdir = os.path.join(ROOT, "osqp-solver_amd")
    out = tmp_path / "grasp_gomp_example"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "grasp_gomp_example.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-pthread", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(out), "20"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    print("\n" + r.stdout)
    assert "planned to the fixed joint goal" in r.stdout and "planned to the grasp goal" in r.stdout
    fixed = float(re.search(r"cost to the fixed joint goal ([0-9.e+-]+)", r.stdout).group(1))
    grasp = float(re.search(r"cost to the grasp goal ([0-9.e+-]+)", r.stdout).group(1))
    assert re.search(r"turn about the tool axis chosen by the planner ([0-9.e+-]+) rad", r.stdout) and fixed > 0 and grasp > 0
