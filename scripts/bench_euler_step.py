"""Time one explicit Euler step on the GPU, fused (``timestep_euler`` + ``step_euler``) against the composition it replaces
(wave-speed broadcasts + ``timestep_advection`` + the sweep + ``primitive2state``, the update per column and
``state2primitive``), with the sweep alone as the floor: one JSON line per mesh, and two files under profiles/.

Meshes (``bench.build_mesh``, one partition each): ``rae2822_0.87M`` -- every block eligible for the 2-D single-kernel sweep,
so ``step_euler`` is ONE launch -- and ``sphere3d_4.6M`` -- 3-D: the sweep into ``work`` and ``update_euler``, two launches.
State: ``conftest.euler_field``-like Mach 0.3 with 5 % noise, seeded.  Variants, per step:
  (a) ``fused``:    ``timestep_euler`` (2 launches) + ``step_euler`` (1 or 2 launches);
  (b) ``composed``: ``speed_of_sound`` + one ``abs(u_d) + a`` broadcast per dimension + ``timestep_advection`` (2 launches)
                    + ``residual_euler_hll`` + ``primitive2state`` + ``ibh_update_dev`` per column + ``state2primitive``;
  (c) ``sweep``:    ``residual_euler_hll`` alone (the floor: no step can take less);
  (d) ``step``:     ``step_euler`` alone, the time step given.
(a) and (b) give the same bits (checked here before anything is timed).

How a figure is taken: after ``--warmup`` eager calls a variant is captured into a HIP graph of ``--batch`` calls on a side
stream; a timed block is that graph replayed back to back between two device events, as often as a first short block says
is needed to fill ``--block-seconds``.  The variants alternate: ``--rounds`` rounds, one block of each in every round; the
figure is the median over the rounds with the spread (min, max).  Needs a GPU; there is no CPU path.

Written: ``bench_euler_step.json`` (everything) and ``timings.md`` (the table of it) in ``--out-dir``.

    python scripts/bench_euler_step.py [--meshes rae2822_0.87M,sphere3d_4.6M] [--scheme hll] [--rounds 5] [--batch 10]
                                       [--block-seconds 0.3] [--out-dir profiles/euler_step]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import ibamd  # noqa: E402
from ibamd import _lib, cfd  # noqa: E402
from ibamd import backend as B  # noqa: E402
from ibamd.hiparray import HipArray as H  # noqa: E402

SCALE = 0.75
LABELS = {"fused": "(a) fused: `timestep_euler` + `step_euler`", "composed": "(b) composed: broadcasts + `timestep_advection` "
          "+ sweep + 3 update passes", "sweep": "(c) the sweep alone", "step": "(d) `step_euler` alone"}


def variants(dpart, P, fluid, scheme):
    n, nv = P.shape
    nd = nv - 2
    sweep_fn = ibamd.residual_euler_hll if scheme == "hll" else ibamd.residual_euler_sensor
    out, work, R = B.colmajor_empty(n, nv), B.colmajor_empty(n, nv), B.colmajor_empty(n, nv)
    Cd, Q2 = B.colmajor_empty(n, nd), B.colmajor_empty(n, nv)
    dt = ibamd.timestep_euler(dpart, P, fluid, SCALE)
    dt_c = dt.clone()

    def fused():
        ibamd.timestep_euler(dpart, P, fluid, SCALE, out=dt)
        return ibamd.step_euler(dpart, P, dt, out, fluid, scheme, work=work)

    def composed():
        a = cfd.speed_of_sound(fluid, P[:, 1])
        for d in range(nd):
            Cd[:, d] = (abs(H(P[:, 2 + d])) + H(a)).t
        ibamd.timestep_advection(dpart, Cd, scale=SCALE, out=dt_c)
        sweep_fn(dpart, P, out=R, fluid=fluid)
        Q = cfd.primitive2state(fluid, P)
        B._stream()
        for v in range(nv):
            _lib.call("ibh_update_dev", n, B._ptr(dt_c), B._ptr(Q[:, v]), B._ptr(R[:, v]), B._ptr(Q2[:, v]))
        return cfd.state2primitive(fluid, Q2)

    def sweep():
        return sweep_fn(dpart, P, out=R, fluid=fluid)

    def step():
        return ibamd.step_euler(dpart, P, dt, out, fluid, scheme, work=work)

    return {"fused": fused, "composed": composed, "sweep": sweep, "step": step}


class Launcher:
    """``calls`` calls of one variant captured in a HIP graph; ``block_us(runs)`` replays it ``runs`` times."""

    def __init__(self, f, calls, warmup, stream):
        import torch
        self.stream, self.calls = stream, calls
        with torch.cuda.stream(stream):
            for _ in range(warmup):
                f()
        stream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=stream):
            for _ in range(calls):
                self.keep = f()
        torch.cuda.synchronize()
        self.block_us(1)

    def block_us(self, runs):
        import torch
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            t0.record()
            for _ in range(runs):
                self.graph.replay()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / (runs * self.calls)


def time_mesh(name, part, scheme, rounds, batch, warmup, block_seconds):
    import torch
    dpart = ibamd.to_backend(part, ibamd.hip)
    nc, nd = dpart.nc, dpart.nd
    fluid = cfd.Fluid()
    rng = np.random.default_rng(12345)
    Ph = np.empty((nc, nd + 2), np.float32)
    Ph[:, 0] = 1e5 * (1 + 0.05 * rng.uniform(-1, 1, nc))
    Ph[:, 1] = 288.15 * (1 + 0.05 * rng.uniform(-1, 1, nc))
    for d in range(nd):
        Ph[:, 2 + d] = 100.0 * (1 + 0.1 * rng.uniform(-1, 1, nc))
    P = ibamd.hip(Ph)
    i = dpart.info
    one = nd == 2 and i["fusable_blocks"] == i["full_blocks"] > 0 and i["irregular_cells"] == 0
    fns = variants(dpart, P, fluid, scheme)
    a, b = fns["fused"](), fns["composed"]()
    assert torch.equal(a, b), f"{name}: the composed step differs from the fused one"
    side = torch.cuda.Stream()
    launchers, runs = {}, {}
    for key, f in fns.items():
        L = launchers[key] = Launcher(f, batch, warmup, side)
        L.block_us(3)
        first = L.block_us(5) * L.calls * 1e-6
        runs[key] = max(3, int(block_seconds / max(first, 1e-7)) + 1)
    times = {key: [] for key in launchers}
    for _ in range(rounds):
        for key, L in launchers.items():
            times[key].append(L.block_us(runs[key]))
    us = {}
    for key, v in times.items():
        us[key] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                   "calls_per_block": runs[key] * launchers[key].calls}
    f_, c_, s_, t_ = (us[k] for k in ("fused", "composed", "sweep", "step"))
    return {"mesh": name, "cells": int(nc), "nd": nd, "scheme": scheme, "rounds": rounds,
            "step_launches": 1 if one else 2, "device": torch.cuda.get_device_name(0), "same_bits": True, "us_per_step": us,
            "composed_over_fused": round(c_["median_us"] / f_["median_us"], 2),
            "fused_faster_outside_the_spread": bool(f_["max_us"] < c_["min_us"]),
            "step_over_sweep": round(t_["median_us"] / s_["median_us"], 2)}


def timings_md(results):
    s = ["# One explicit Euler step, fused against composed: timings", "",
         "Written by `scripts/bench_euler_step.py` from the run recorded in `bench_euler_step.json`; not edited by hand.",
         "Time per step: median (min - max) over the alternating rounds, every variant replayed from a HIP graph.", ""]
    for r in results:
        s += [f"## `{r['mesh']}`: {r['cells']} cells, {r['nd']}-D, scheme {r['scheme']}, `step_euler` in {r['step_launches']} "
              f"launch(es), {r['rounds']} rounds, {r['device']}", "", "| variant | us per step | calls per block |", "|---|---|---|"]
        for key, v in r["us_per_step"].items():
            s.append(f"| {LABELS[key]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) | {v['calls_per_block']} |")
        s += ["", f"* composed / fused: {r['composed_over_fused']}",
              f"* fused faster outside the spread (max fused < min composed): {r['fused_faster_outside_the_spread']}",
              f"* `step_euler` alone / the sweep alone: {r['step_over_sweep']}", ""]
    return "\n".join(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="rae2822_0.87M,sphere3d_4.6M")
    ap.add_argument("--scheme", default="hll", choices=["hll", "sensor"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10, help="steps captured per HIP graph")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-seconds", type=float, default=0.3, help="GPU time a timed block is sized to")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "euler_step"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_euler_step.py needs a GPU: nothing is measured without one")
    os.makedirs(a.out_dir, exist_ok=True)
    results = []
    for name in a.meshes.split(","):
        t0 = time.time()
        dom = ibamd.Domain(bench.build_mesh(name), max_partition_size=10 ** 9, boundaries=False)
        part = next(iter(dom.partitions.values()))
        print(f"# {name}: {len(dom)} cells, built in {time.time() - t0:.0f} s", flush=True)
        r = time_mesh(name, part, a.scheme, a.rounds, a.batch, a.warmup, a.block_seconds)
        print(json.dumps(r), flush=True)
        results.append(r)
        with open(os.path.join(a.out_dir, "bench_euler_step.json"), "w") as f:
            json.dump({"meshes": results}, f, indent=1)
        with open(os.path.join(a.out_dir, "timings.md"), "w") as f:
            f.write(timings_md(results))
        del dom, part
    return 0


if __name__ == "__main__":
    sys.exit(main())
