"""Tilt limits through the C++ layer of include/mi_osqp/gomp.hpp (tests/cpp/gomp_tilt.cpp).

CPU : ConstraintBuilder<2> and <3> with tilts and GOMPSolver::isSolutionOK on scenes TF, TE, TEA and TM of tests/tilt_refs.py
      against the known answers of tests/golden/tilt_kats.json (values and bounds within 1e-12 of their term scale, +-1e30 exact,
      verdicts equal; scenes TE and TEA, exact by construction, bit for bit); the allocation (W |tilts| rows more, the empty rows
      behind the tilt rows); a builder with an empty tilt list against the six-argument one, bit for bit; dh::axis against
      central differences, tiltsOK and tiltsOKAlong at the 1 mrad; the upright problem through the sequential GOMPSolver on the
      oracle backend: the tool tips 39 degrees over without the limit and stays within 15 degrees with it.
GPU : the continuous driver with the SQP step on the device (mi_gomp_scene_create_tilts) against the host-assembling one on the
      upright problem (2 trajectories of 20 waypoints): same exit codes and counters, largest tilt within the limit plus 1 mrad
      with the limit and beyond it without; the example plans every trajectory and prints both tilts."""
import os
import re
import subprocess

import numpy as np
import pytest

import tilt_refs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import osqp_solver_amd as M
    from oracle import oracle as O
    M.lib(); O.lib()
    out = tmp_path_factory.mktemp("gomp_tilt") / "gomp_tilt"
    libdir, ordir = os.path.join(ROOT, "osqp-solver_amd"), os.path.join(ROOT, "oracle", "_build")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gomp_tilt.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-L" + ordir, "-loracle_osqp", "-fopenmp", "-pthread",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + ordir], check=True)
    return str(out)


def _scene_file(s, path):
    hx = lambda vals: " ".join(float(v).hex() for v in vals)
    inf = 1e30
    ch = s["chain"]
    text = [str(s["D"]), str(len(ch["a"]))] + [hx([ch["a"][i], ch["d"][i], ch["alpha"][i], ch["theta0"][i]]) for i in range(len(ch["a"]))]
    text += [str(len(s["balls"]))] + [f"{b['model']} {int(b['gripper'])} {hx([b['radius']])} {hx((list(b['param']) + [0.0] * 9)[:9])}" for b in s["balls"]]
    text += [str(len(s["lines"]))] + [f"{hx(ln['dir'])} {hx(ln['point'])} {int(bool(ln.get('below')))}" for ln in s["lines"]]
    text += [str(len(s["capsules"]))] + [f"{hx(c['a'])} {hx(c['b'])} {hx([c['radius'], c['margin']])}" for c in s["capsules"]]
    text += [str(len(s["cuboids"]))] + [f"{hx(c['centre'])} {hx(c['axes'])} {hx(c['half'])} {hx([c['radius'], c['margin']])}" for c in s["cuboids"]]
    text += [str(len(s["pairs"]))] + [f"{p['a']} {p['b']} {hx([p['margin']])}" for p in s["pairs"]]
    text += [str(len(s["tilts"]))] + [f"{t['frame']} {hx(t['axis'])} {hx(t['ref'])} {hx([t['max_angle'], t['margin']])}" for t in s["tilts"]]
    text += [hx(s["con_lo"] if s["con_lo"] is not None else [-inf] * 3), hx(s["con_hi"] if s["con_hi"] is not None else [inf] * 3)]
    text += [str(s["W"]), str(len(s["trajs"]))] + [hx(t) for t in s["trajs"]]
    path.write_text("\n".join(text) + "\n")


@pytest.mark.parametrize("name", T.KAT_SCENES)
def test_constraint_builder_and_verdict_against_the_known_answers(exe, name, tmp_path):
    s, kats, ref = T.scene(name), T.load_kats()[name], T.scene_reference(name)
    D = s["D"]
    path = tmp_path / "scene.txt"
    _scene_file(s, path)
    r = subprocess.run([exe, "rows", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ROWS OK" in r.stdout, r.stdout[-2000:] + r.stderr
    rows, verdicts = {}, {}
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "R":
            rows.setdefault(int(t[1]), []).append([float.fromhex(v) for v in t[3:]])
        elif t[0] == "V":
            verdicts[int(t[1])] = bool(int(t[2]))
    worst_v = worst_b = 0.0
    for b, kat in enumerate(kats):
        got = np.array(rows[b])
        vals, l, u = np.array(kat["vals"]), np.array(kat["l"]), np.array(kat["u"])
        assert got.shape == (len(l), D + 2)
        assert verdicts[b] == kat["ok"], b
        worst_v = max(worst_v, float(np.max(np.abs(got[:, :D] - vals))))
        assert np.max(np.abs(got[:, :D] - vals)) <= 1e-12
        for side, dev, want in (("l", got[:, D], l), ("u", got[:, D + 1], u)):
            sc = ref[b][side + "_scale"]
            inf = sc == 0
            assert np.array_equal(dev[inf].view(np.int64), want[inf].view(np.int64)), (b, side)      # +-1e30 exactly
            assert np.all(np.abs(want[inf]) == 1e30)
            fin = ~inf
            eb = float(np.max(np.abs(dev[fin] - want[fin]) / sc[fin], initial=0.0))
            worst_b = max(worst_b, eb)
            assert eb <= 1e-12, (b, side, eb)
        if name in T.EXACT:                                                   # exact by construction
            assert np.array_equal(got[:, :D], vals) and np.array_equal(got[:, D], l) and np.array_equal(got[:, D + 1], u)
    print(f"\nscene {name}: ConstraintBuilder against the known answers: values {worst_v:.3e}, bounds {worst_b:.3e} of their term scale")


def test_axis_kinematics_and_tilts_ok(exe):
    r = subprocess.run([exe, "checks"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "CHECKS OK" in r.stdout, r.stdout + r.stderr


def test_the_upright_problem_on_the_oracle_backend(exe):
    """The planning problem of `gomp_tilt cont` through the sequential driver on the oracle: the host path alone."""
    r = subprocess.run([exe, "tilt_oracle"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "TILT ORACLE OK" in r.stdout, r.stdout + r.stderr
    print("\n" + r.stdout)
    tip = {(m[0], m[1]): float(m[2]) for m in re.findall(r"upright traj (\d) (with|without) tilt limit: kOptimal .* largest tilt ([0-9.]+) deg \(", r.stdout)}
    assert len(tip) == 4
    allowed = np.degrees(np.radians(15) + 1e-3)
    for b in "01":
        assert tip[(b, "without")] > 30.0 and tip[(b, "with")] <= allowed


@pytest.mark.gpu
def test_continuous_planner_with_tilts_device_against_host_assembly(exe):
    r = subprocess.run([exe, "cont"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CONT OK" in r.stdout and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    print("\n" + r.stdout)


@pytest.mark.gpu
def test_tilt_gomp_example_plans_every_trajectory(tmp_path):
    import osqp_solver_amd as M
    M.lib()
    libdir = os.path.join(ROOT, "osqp-solver_amd")
    out = tmp_path / "tilt_gomp_example"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "tilt_gomp_example.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-pthread", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(out), "2", "20", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    print("\n" + r.stdout)
    assert "2 of 2 trajectories planned without the limit" in r.stdout and "2 of 2 trajectories planned with the limit" in r.stdout
    without = float(re.search(r"largest tilt without the limit ([0-9.]+) deg", r.stdout).group(1))
    with_ = float(re.search(r"largest tilt with the limit ([0-9.]+) deg", r.stdout).group(1))
    assert without > 30.0 and with_ <= np.degrees(np.radians(15) + 1e-3)
