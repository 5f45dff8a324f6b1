"""Distance grids through the C++ layer of include/mi_osqp/gomp.hpp (tests/cpp/gomp_grid.cpp).

CPU : the program is built with -fsanitize=address,undefined and run as a program.  DistanceGrid::sample on scene GT of
      tests/grid_refs.py against the known answers of tests/golden/grid_kats.json, bit for bit; DistanceGrid::fromObstacles
      against the reference's restatement (within 4 ulp of the largest value; the count of nodes that differ at all is printed);
      ConstraintBuilder<3> with grids and GOMPSolver::isSolutionOK on scenes GT, GP and GM against the known answers (values and
      bounds within 1e-12 of their term scale, +-1e30 exact, verdicts equal; GT and GP bit for bit); the allocation; a builder
      with an empty grid list against the seven-argument one, bit for bit; the host twin on the corner cases; a point robot past
      the corner of a box that exists only as a grid, through the sequential GOMPSolver on the oracle backend.
GPU : (built without the sanitizers) the continuous driver with the SQP step on the device (mi_gomp_scene_create_grids) against
      the host-assembling one and the batch driver on that problem (4 trajectories of 20 waypoints): same exit codes and counters,
      trajectories within 1e-6 - max |dx| is printed -, then updateGrid with an empty world; the example plans both ways."""
import os
import re
import subprocess

import numpy as np
import pytest

import grid_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out, sanitize):
    import osqp_solver_amd as M
    from oracle import oracle as O
    M.lib(); O.lib()
    libdir, ordir = os.path.join(ROOT, "osqp-solver_amd"), os.path.join(ROOT, "oracle", "_build")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2"] + san + ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gomp_grid.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-L" + ordir, "-loracle_osqp", "-fopenmp", "-pthread",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath," + ordir], check=True)
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("gomp_grid") / "gomp_grid_san", True)


def _env():
    # the libraries the program links were not built with the sanitizers: what they keep until exit is not this program's leak
    return dict(os.environ, ASAN_OPTIONS="detect_leaks=0")


def _scene_file(s, path, samples=(), from_obstacles=None):
    hx = lambda vals: " ".join(float(v).hex() for v in vals)
    inf = 1e30
    text = [str(len(s["balls"]))] + [f"{int(b['gripper'])} {hx([b['radius']])} {hx(b['param'][:9])}" for b in s["balls"]]
    text += [str(len(s["lines"]))] + [f"{hx(ln['dir'])} {hx(ln['point'])} {int(bool(ln.get('below')))}" for ln in s["lines"]]
    text += [str(len(s["capsules"]))] + [f"{hx(c['a'])} {hx(c['b'])} {hx([c['radius'], c['margin']])}" for c in s["capsules"]]
    text += [str(len(s["cuboids"]))] + [f"{hx(c['centre'])} {hx(c['axes'])} {hx(c['half'])} {hx([c['radius'], c['margin']])}" for c in s["cuboids"]]
    text += [str(len(s["grids"]))] + [f"{hx(g['origin'])} {hx([g['cell']])} {g['n'][0]} {g['n'][1]} {g['n'][2]} {hx([g['offset'], g['margin']])} {hx(g['values'])}"
                                      for g in s["grids"]]
    text += [hx(s["con_lo"] if s["con_lo"] is not None else [-inf] * 3), hx(s["con_hi"] if s["con_hi"] is not None else [inf] * 3)]
    text += [str(s["W"]), str(len(s["trajs"]))] + [hx(t) for t in s["trajs"]]
    text += [str(len(samples))] + [hx(p) for p in samples]
    if from_obstacles is None:
        text += ["0"]
    else:
        f = from_obstacles
        text += ["1", f"{hx(f['origin'])} {hx([f['cell']])} {f['n'][0]} {f['n'][1]} {f['n'][2]} {hx(f['box']['centre'])} {hx(f['box']['half'])} "
                      f"{hx(f['capsule']['a'])} {hx(f['capsule']['b'])} {hx([f['capsule']['radius']])}"]
    path.write_text("\n".join(text) + "\n")


@pytest.mark.parametrize("name", R.KAT_SCENES)
def test_constraint_builder_verdict_samples_and_from_obstacles_against_the_known_answers(exe, name, tmp_path):
    s, kats, ref = R.scene(name), R.load_kats(), R.scene_reference(name)
    D = s["D"]
    path = tmp_path / "scene.txt"
    samples = kats["GT"]["samples"] if name == "GT" else []
    _scene_file(s, path, [k["p"] for k in samples], kats["from_obstacles"] if name == "GT" else None)
    r = subprocess.run([exe, "rows", str(path)], capture_output=True, text=True, timeout=300, env=_env())
    assert r.returncode == 0 and "ROWS OK" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    rows, verdicts, got_samples, nodes = {}, {}, {}, {}
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "R":
            rows.setdefault(int(t[1]), []).append([float.fromhex(v) for v in t[3:]])
        elif t[0] == "V":
            verdicts[int(t[1])] = bool(int(t[2]))
        elif t[0] == "S":
            got_samples[int(t[1])] = (bool(int(t[2])), [float.fromhex(v) for v in t[3:]])
        elif t[0] == "F":
            nodes[int(t[1])] = float.fromhex(t[2])
    worst_v = worst_b = 0.0
    for b, kat in enumerate(kats[name]["cases"]):
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
        if name in R.EXACT:                                                   # exact by construction
            assert np.array_equal(got[:, :D], vals) and np.array_equal(got[:, D], l) and np.array_equal(got[:, D + 1], u)
    print(f"\nscene {name}: ConstraintBuilder against the known answers: values {worst_v:.3e}, bounds {worst_b:.3e} of their term scale")
    if name != "GT":
        return
    assert len(got_samples) == len(samples) == 64 and sum(k["inside"] for k in samples) >= 15
    for i, k in enumerate(samples):                                           # DistanceGrid::sample, bit for bit
        inside, (phi, gx, gy, gz) = got_samples[i]
        assert inside == k["inside"], i
        assert np.array_equal(np.array([phi, gx, gy, gz]).view(np.int64), np.array([k["phi"]] + k["grad"]).view(np.int64)), (i, k)
    want = np.array(kats["from_obstacles"]["values"])
    got = np.array([nodes[k] for k in range(len(want))])
    print(f"fromObstacles: {len(want)} nodes, {int(np.sum(got != want))} differ from the restatement, by at most {np.max(np.abs(got - want)):.3e}")
    assert np.max(np.abs(got - want)) <= 4 * np.spacing(np.max(np.abs(want)))


def test_host_twin_and_a_point_robot_past_a_gridded_box_corner(exe):
    r = subprocess.run([exe, "oracle"], capture_output=True, text=True, timeout=600, env=_env())
    assert r.returncode == 0 and "ORACLE OK" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr[-4000:]
    print("\n" + r.stdout)


@pytest.mark.gpu
def test_continuous_and_batch_planner_with_a_grid_device_against_host_assembly(tmp_path):
    exe = _build(tmp_path / "gomp_grid", False)
    r = subprocess.run([exe, "cont"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CONT OK" in r.stdout and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    print("\n" + r.stdout)


@pytest.mark.gpu
def test_grid_gomp_example_plans_both_ways(tmp_path):
    import osqp_solver_amd as M
    M.lib()
    libdir = os.path.join(ROOT, "osqp-solver_amd")
    out = tmp_path / "grid_gomp_example"
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "grid_gomp_example.cpp"),
                    "-o", str(out), "-L" + libdir, "-lmi_osqp", "-pthread", "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(out), "2", "20", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Memory access fault" not in r.stdout + r.stderr, r.stdout + r.stderr
    print("\n" + r.stdout)
    assert "2 of 2 trajectories planned with the cuboids" in r.stdout and "2 of 2 trajectories planned with the grid alone" in r.stdout
    diff = float(re.search(r"largest difference between the two plans ([0-9.e+-]+) rad", r.stdout).group(1))
    assert diff < 1.0
