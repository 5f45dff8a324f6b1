"""Self-collision pairs through the C++ layer of include/mi_osqp/gomp.hpp (tests/cpp/gomp_pairs.cpp).

CPU : ConstraintBuilder<3> with pairs and GOMPSolver::isSolutionOK on scenes PT and PM of tests/pair_refs.py against the known
      answers of tests/golden/pair_kats.json (values and bounds within 1e-12 of their term scale, +-1e30 exact, verdicts equal;
      scene PT, exact by construction, bit for bit); the allocation (W |pairs| rows more, the empty rows behind the pair rows); a
      builder with an empty pair list against the five-argument one, bit for bit; dhSelfPairs on the seven balls of the 7-joint
      chain; the folding problem through the sequential GOMPSolver on the oracle backend: it penetrates without pairs and is
      clear with them.
GPU : the continuous driver with the SQP step on the device (mi_gomp_scene_create_pairs) against the host-assembling one on the
      folding problem (2 trajectories of 20 waypoints): same exit codes and counters, trajectories within 1e-6; the example
      plans every trajectory and prints both clearances."""
import os
import re
import subprocess

import numpy as np
import pytest

import pair_refs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    import osqp_solver_amd as M
    from oracle import oracle as O
    M.lib(); O.lib()
    out = tmp_path_factory.mktemp("gomp_pairs") / "gomp_pairs"
    libdir, ordir = os.path.join(ROOT, "osqp-solver_amd"), os.path.join(ROOT, "oracle", "_build")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gomp_pairs.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-L" + ordir, "-loracle_osqp", "-fopenmp", "-pthread",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + ordir], check=True)
    return str(out)


def _scene_file(s, path):
    hx = lambda vals: " ".join(float(v).hex() for v in vals)
    inf = 1e30
    text = [str(len(s["balls"]))] + [f"{b['model']} {int(b['gripper'])} {hx([b['radius']])} {hx(b['param'][:9])}" for b in s["balls"]]
    text += [str(len(s["lines"]))] + [f"{hx(ln['dir'])} {hx(ln['point'])} {int(bool(ln.get('below')))}" for ln in s["lines"]]
    text += [str(len(s["capsules"]))] + [f"{hx(c['a'])} {hx(c['b'])} {hx([c['radius'], c['margin']])}" for c in s["capsules"]]
    text += [str(len(s["cuboids"]))] + [f"{hx(c['centre'])} {hx(c['axes'])} {hx(c['half'])} {hx([c['radius'], c['margin']])}" for c in s["cuboids"]]
    text += [str(len(s["pairs"]))] + [f"{p['a']} {p['b']} {hx([p['margin']])}" for p in s["pairs"]]
    text += [hx(s["con_lo"] if s["con_lo"] is not None else [-inf] * 3), hx(s["con_hi"] if s["con_hi"] is not None else [inf] * 3)]
    text += [str(s["W"]), str(len(s["trajs"]))] + [hx(t) for t in s["trajs"]]
    path.write_text("\n".join(text) + "\n")


@pytest.mark.parametrize("name", P.KAT_SCENES)
def test_constraint_builder_and_verdict_against_the_known_answers(exe, name, tmp_path):
    s, kats, ref = P.scene(name), P.load_kats()[name], P.scene_reference(name)
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
        if name in P.EXACT:                                                   # exact by construction
            assert np.array_equal(got[:, :3], vals) and np.array_equal(got[:, 3], l) and np.array_equal(got[:, 4], u)
    print(f"\nscene {name}: ConstraintBuilder against the known answers: values {worst_v:.3e}, bounds {worst_b:.3e} of their term scale")


def test_dh_self_pairs_of_the_seven_chain_balls(exe):
    r = subprocess.run([exe, "selfpairs"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "SELFPAIRS OK" in r.stdout, r.stdout + r.stderr


def test_the_folding_problem_on_the_oracle_backend(exe):
    """The planning problem of `gomp_pairs cont` through the sequential driver on the oracle: the host path alone."""
    r = subprocess.run([exe, "fold_oracle"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "FOLD ORACLE OK" in r.stdout, r.stdout + r.stderr
    print("\n" + r.stdout)
    clear = {(m[0], m[1]): float(m[2]) for m in re.findall(r"fold traj (\d) (with|without) pairs: kOptimal .* minimum pair clearance (-?[0-9.]+) ", r.stdout)}
    assert len(clear) == 4
    for b in "01":
        assert clear[(b, "without")] < -0.01 and clear[(b, "with")] >= -1e-3


@pytest.mark.gpu
def test_continuous_planner_with_pairs_device_against_host_assembly(exe):
    r = subprocess.run([exe, "cont"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CONT OK" in r.stdout and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    print("\n" + r.stdout)


@pytest.mark.gpu
def test_selfcollision_gomp_example_plans_every_trajectory(tmp_path):
    import osqp_solver_amd as M
    M.lib()
    libdir = os.path.join(ROOT, "osqp-solver_amd")
    out = tmp_path / "selfcollision_gomp_example"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "selfcollision_gomp_example.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-pthread", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(out), "2", "20", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    print("\n" + r.stdout)
    assert "2 of 2 trajectories planned without pairs" in r.stdout and "2 of 2 trajectories planned with pairs" in r.stdout
    without = float(re.search(r"minimum pair clearance without pairs (-?[0-9.]+)", r.stdout).group(1))
    with_ = float(re.search(r"minimum pair clearance with pairs (-?[0-9.]+)", r.stdout).group(1))
    assert without < -0.01 and with_ >= -1e-3
