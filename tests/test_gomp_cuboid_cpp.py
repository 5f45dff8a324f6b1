"""Cuboid obstacles through the C++ layer of include/mi_osqp/gomp.hpp (tests/cpp/gomp_cuboid.cpp).

CPU : ConstraintBuilder<3> with cuboids and GOMPSolver::isSolutionOK on scenes XT, XP and XM of tests/cuboid_refs.py against
      the known answers of tests/golden/cuboid_kats.json (values and bounds within 1e-12 of their term scale, +-1e30 exact,
      verdicts equal; scenes XT and XP, exact by construction, bit for bit); a builder with an empty cuboid list against the
      four-argument one, bit for bit; the host twin on the corner cases of the formulas and a point robot past a box corner
      through the sequential GOMPSolver on the oracle backend; the planning problems of the GPU test through the same.
GPU : the continuous driver with the SQP step on the device (mi_gomp_scene_create_cuboids) against the host-assembling one on
      a 3-joint scene (4 trajectories of 20 waypoints) and the 7-joint bin scene (2 trajectories of 20 waypoints): same exit
      codes and counters, trajectories within 1e-6; the example plans its bin scene."""
import os
import subprocess

import numpy as np
import pytest

import cuboid_refs as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import osqp_solver_amd as M
    from oracle import oracle as O
    M.lib(); O.lib()
    out = tmp_path_factory.mktemp("gomp_cuboid") / "gomp_cuboid"
    libdir, ordir = os.path.join(ROOT, "osqp-solver_amd"), os.path.join(ROOT, "oracle", "_build")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gomp_cuboid.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-L" + ordir, "-loracle_osqp", "-fopenmp", "-pthread",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + ordir], check=True)
    return str(out)


def _scene_file(s, path):
    hx = lambda vals: " ".join(float(v).hex() for v in vals)
    inf = 1e30
    text = [str(len(s["balls"]))] + [f"{int(b['gripper'])} {hx([b['radius']])} {hx(b['param'][:9])}" for b in s["balls"]]
    text += [str(len(s["lines"]))] + [f"{hx(ln['dir'])} {hx(ln['point'])} {int(bool(ln.get('below')))}" for ln in s["lines"]]
    text += [str(len(s["capsules"]))] + [f"{hx(c['a'])} {hx(c['b'])} {hx([c['radius'], c['margin']])}" for c in s["capsules"]]
    text += [str(len(s["cuboids"]))] + [f"{hx(c['centre'])} {hx(c['axes'])} {hx(c['half'])} {hx([c['radius'], c['margin']])}" for c in s["cuboids"]]
    text += [hx(s["con_lo"] if s["con_lo"] is not None else [-inf] * 3), hx(s["con_hi"] if s["con_hi"] is not None else [inf] * 3)]
    text += [str(s["W"]), str(len(s["trajs"]))] + [hx(t) for t in s["trajs"]]
    path.write_text("\n".join(text) + "\n")


@pytest.mark.parametrize("name", X.KAT_SCENES)
def test_constraint_builder_and_verdict_against_the_known_answers(exe, name, tmp_path):
    s, kats, ref = X.scene(name), X.load_kats()[name], X.scene_reference(name)
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
        assert got.shape == (len(l), 5)
        assert verdicts[b] == kat["ok"], b
        worst_v = max(worst_v, float(np.max(np.abs(got[:, :3] - vals))))
        assert np.max(np.abs(got[:, :3] - vals)) <= 1e-12
        for side, dev, want in (("l", got[:, 3], l), ("u", got[:, 4], u)):
            sc = ref[b][side + "_scale"]
            inf = sc == 0
            assert np.array_equal(dev[inf].view(np.int64), want[inf].view(np.int64)), (b, side)      # +-1e30 exactly
            assert np.all(np.abs(want[inf]) == 1e30)
            fin = ~inf
            eb = float(np.max(np.abs(dev[fin] - want[fin]) / sc[fin], initial=0.0))
            worst_b = max(worst_b, eb)
            assert eb <= 1e-12, (b, side, eb)
        if name in X.EXACT:                                                   # exact by construction
            assert np.array_equal(got[:, :3], vals) and np.array_equal(got[:, 3], l) and np.array_equal(got[:, 4], u)
    print(f"\nscene {name}: ConstraintBuilder against the known answers: values {worst_v:.3e}, bounds {worst_b:.3e} of their term scale")


def test_host_twin_and_point_robot_past_a_box_corner_on_the_oracle_backend(exe):
    r = subprocess.run([exe, "oracle"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ORACLE OK" in r.stdout and "kOptimal" in r.stdout, r.stdout + r.stderr
    print("\n" + r.stdout)


def test_the_planning_problems_of_the_gpu_test_on_the_oracle_backend(exe):
    """The planning problems of `gomp_cuboid cont` through the sequential driver on the oracle: the host path alone."""
    r = subprocess.run([exe, "bin_oracle"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BIN ORACLE OK" in r.stdout, r.stdout + r.stderr
    print("\n" + r.stdout)


@pytest.mark.gpu
def test_continuous_planner_with_cuboids_device_against_host_assembly(exe):
    r = subprocess.run([exe, "cont"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CONT OK" in r.stdout and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    print("\n" + r.stdout)


@pytest.mark.gpu
def test_cuboid_gomp_example_plans_every_trajectory(tmp_path):
    import osqp_solver_amd as M
    M.lib()
    libdir = os.path.join(ROOT, "osqp-solver_amd")
    out = tmp_path / "cuboid_gomp_example"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "cuboid_gomp_example.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-pthread", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(out), "2", "20", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "2 of 2 trajectories planned" in r.stdout and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    assert "SQP step on the device" in r.stdout and "re-linearisations" in r.stdout and "minimum clearance" in r.stdout
