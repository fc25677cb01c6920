"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy files -- the same files for the
same arguments, at most 64 MB, and (on the device) the very values of the steps it timed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_write_outputs_samples_the_same_rows_within_the_budget(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    a = rng.standard_normal((1000, 3)).astype(np.float32)
    b = rng.standard_normal(1000)                       # float64 stays float64
    c = np.float32([0.5])
    budget = 8000
    for d in ("x", "y"):
        bench.write_outputs(str(tmp_path / d), {"a": a, "b": b, "dt": c}, budget=budget)
    x, y = _load_dir(str(tmp_path / "x")), _load_dir(str(tmp_path / "y"))
    assert sorted(x) == ["a", "b", "dt"]
    for k in x:
        assert np.array_equal(x[k], y[k])               # same arguments, same files
    assert x["a"].dtype == np.float32 and x["b"].dtype == np.float64 and x["dt"].dtype == np.float32
    assert sum(v.nbytes for v in x.values()) <= budget + c.nbytes
    assert 0 < x["b"].shape[0] < 1000 and x["a"].shape == (x["b"].shape[0], 3)
    rows = np.array([np.flatnonzero(b == v)[0] for v in x["b"]])   # where the kept values sit in b
    assert np.all(np.diff(rows) > 0)                                 # in order, and a keeps the same rows
    assert np.array_equal(x["a"], a[rows]) and np.array_equal(x["dt"], c)
    bench.write_outputs(str(tmp_path / "z"), {"a": a, "dt": c}, budget=1 << 20)
    z = _load_dir(str(tmp_path / "z"))
    assert np.array_equal(z["a"], a) and np.array_equal(z["dt"], c)   # within the budget: everything, unsampled


def _bench(args, out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "rae2822_37k", "--repeats", "2",
                        "--no-cpu-baseline", "--dump-outputs", out_dir] + args, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), _load_dir(out_dir)


def _partition(boundaries, families):
    """The one partition bench.py builds for rae2822_37k on one GPU, with its synthetic fields."""
    import bench
    import ibamd
    msh = bench.build_mesh("rae2822_37k")
    npb = msh.block_size ** msh.ndims
    mps = -(-len(msh) // npb) * npb
    dom = ibamd.Domain(msh, max_partition_size=mps, boundaries=boundaries, only=[1], hypercube_families=families)
    part = dom.partitions[1]
    u_h, C_h = bench.synthetic_fields(part.centers)
    return dom, ibamd.to_backend(part, ibamd.hip), ibamd.hip(u_h), ibamd.hip(C_h)


@pytest.mark.gpu
def test_sweep_dump_is_the_residual(tmp_path):
    import ibamd
    out, got = _bench(["--steps", "5", "--warmup", "2"], str(tmp_path / "d"))
    assert out["steps"] == 5 and sorted(got) == ["residual"]
    _, dpart, u, C = _partition(False, ())
    exp = ibamd.to_host(ibamd.residual_advection(dpart, u, C))
    assert got["residual"].dtype == np.float32 and np.array_equal(got["residual"], exp)


@pytest.mark.gpu
def test_march_dump_is_the_steps_it_timed(tmp_path):
    """7 steps a block, graphs of 4: one replay and three eager steps must chain into 7 consecutive steps of the march,
    equal to the same 7 steps launched one by one."""
    import torch
    import ibamd
    from conftest import RAE_FAMILIES
    out, got = _bench(["--step", "march", "--steps", "7", "--warmup", "3", "--graph-batch", "4"], str(tmp_path / "d"))
    assert out["steps"] == 7 and sorted(got) == ["dt", "u"]
    dom, dpart, u, C = _partition(True, RAE_FAMILIES)
    bcs = ibamd.BCSet(dom, [(name, "copy" if name == "farfield" else 0.0) for name in dom.boundaries], ipart=1)
    dt = ibamd.timestep_advection(dpart, C, scale=0.75)
    a, b = u.clone(), torch.empty_like(u)
    for _ in range(7):
        ibamd.step_advection(dpart, a, C, dt, bcs, out=b, next_dt=dt, scale=0.75)
        a, b = b, a
    assert np.array_equal(got["dt"], ibamd.to_host(dt))
    assert np.array_equal(got["u"], ibamd.to_host(a))
    assert not np.array_equal(got["u"], ibamd.to_host(u))
