"""Time the boundary conditions of BASELINE.json configs[4] on the GPU, fused against composed: one JSON line per level, and
two files under profiles/.

Per level of ``multigrid`` over ``bench.build_mesh`` (``sphere3d_8M``: the fine level and two coarse ones, each with its own
``Boundary`` structs), ``closures.config5_boundary_conditions(dom, Q, far)`` on a seeded state ``Q = [p T u v w R]`` as
  (a) ``fused=True``: two ``impose_flow_bc`` calls, one launch per boundary partition (two where a ghost cell is a donor),
  (b) ``fused=False``: two ``impose_bc`` calls with the wall closure at operator granularity.

How a figure is taken (as scripts/bench_euler_sensor.py does): after ``--warmup`` eager calls a variant is captured into a
HIP graph of ``--batch`` calls on a side stream; a timed block is that graph replayed back to back between two device
events, as often as a first short block says is needed to fill ``--block-seconds``.  (b) is NOT captured: ``impose_bc``
hands a constant boundary value to ``ibh_bc_blend`` as a host pointer, which a captured copy would read again at every
replay, after the array is gone; it runs eagerly, one call per run, and so does (a) a second time, so that the two are
compared like for like (eager figures are bounded below by the host's launch rate -- which is what the composed closure
is bound by in a solver loop too).  ``launch`` says how each figure was launched.  The variants alternate: ``--rounds``
rounds, one block of each in every round; the figure is the median over the rounds with the spread (min, max).
``launches`` is the number of device kernels of ONE eager call, counted from a profiler trace of that call.  Both variants
leave the same ghost cells within 1e-5 (checked here before anything is timed).  Needs a GPU; there is no CPU path.

Written: ``bench_wall_bc.json`` (everything) and ``timings.md`` (the table of it) in ``--out-dir``.

    python scripts/bench_wall_bc.py [--mesh sphere3d_8M] [--levels 2] [--rounds 5] [--batch 10] [--block-seconds 0.5]
                                    [--out-dir profiles/wall_bc]
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
from ibamd.closures import config5_boundary_conditions  # noqa: E402

FAR = [1.0e5, 288.15, 100.0, 0.0, 0.0]
LABELS = {"fused": "(a) fused: `impose_flow_bc`", "fused_eager": "(a) fused, eager calls",
          "composed": "(b) composed: `impose_bc` + closure, eager calls"}
NOT_CAPTURED = "impose_bc passes constant boundary values to ibh_bc_blend by host pointer: a replay would read it again"


class Launcher:
    """``calls`` calls of one variant per ``run()``: a captured graph of them, or one eager call."""

    def __init__(self, f, calls, warmup, Q, stream, capture):
        import torch
        self.f, self.stream, self.graph, self.calls, self.why = f, stream, None, 1, None if capture else NOT_CAPTURED
        with torch.cuda.stream(stream):
            for _ in range(warmup):
                f()
        stream.synchronize()
        assert bool(torch.isfinite(Q).all().item()), "non-finite state"
        if capture:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                for _ in range(calls):
                    f()
            self.graph, self.calls = g, calls
            torch.cuda.synchronize()
        self.block_us(1)

    @property
    def launch(self):
        return f"hip-graph x{self.calls}" if self.graph is not None else "eager"

    def block_us(self, runs):
        """us per call of ``runs`` runs back to back between two events on the launch stream."""
        import torch
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            t0.record()
            for _ in range(runs):
                if self.graph is not None:
                    self.graph.replay()
                else:
                    self.f()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / (runs * self.calls)


def seeded_state(n, seed=12345):
    rng = np.random.default_rng(seed)
    Q = np.empty((n, 6), np.float32)
    Q[:, 0] = 1e5 * (1 + 0.05 * rng.uniform(-1, 1, n))
    Q[:, 1] = 288.15 * (1 + 0.05 * rng.uniform(-1, 1, n))
    Q[:, 2] = 100.0 * (1 + 0.1 * rng.uniform(-1, 1, n))
    Q[:, 3:5] = 20.0 * rng.uniform(-1, 1, (n, 2))
    Q[:, 5] = 4.5e-5 * (1 + 0.5 * rng.uniform(0, 1, n))
    return Q


def count_kernels(f):
    """Device kernels of one call of ``f``, from a profiler trace; or the reason they could not be counted."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            f()
            torch.cuda.synchronize()
        dev = getattr(torch.autograd.DeviceType, "CUDA")
        n = sum(1 for e in prof.events() if e.device_type == dev and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        copies = sum(1 for e in prof.events() if e.device_type == dev and ("memcpy" in e.name.lower()
                                                                           or "memset" in e.name.lower()))
        return {"kernels": n, "copies": copies} if n else {"not_counted": "the trace holds no device kernel"}
    except Exception as e:  # recorded beside the figures
        return {"not_counted": f"{type(e).__name__}: {e}"[:200]}


def time_level(l, dom, rounds, batch, warmup, block_seconds):
    import torch
    n = len(dom)
    ghosts = {k: int(sum(b.ghost_indices.size for b in v.values())) for k, v in dom.boundaries.items()}
    direct = {}
    for name, parts in dom.boundaries.items():
        for b in parts.values():
            ibamd.to_backend(b, ibamd.hip)
    Q0 = ibamd.hip(seeded_state(n))
    Qs = {k: Q0.clone() for k in LABELS}
    fns = {k: (lambda k=k: config5_boundary_conditions(dom, Qs[k], FAR, fused=k.startswith("fused"))) for k in LABELS}
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    for name, parts in dom.boundaries.items():
        direct[name] = [bool(getattr(ibamd.to_backend(b), "flow_direct", None)) for b in parts.values()]
    a, b = Qs["fused"], Qs["composed"]
    differ = float(((a - b).abs().amax(dim=0) / b.abs().amax(dim=0)).max().item())
    assert differ <= 1e-5, f"level {l}: fused and composed differ by {differ}"
    launches = {k: count_kernels(f) for k, f in fns.items()}
    side = torch.cuda.Stream()
    launchers, runs = {}, {}
    for k, f in fns.items():
        L = launchers[k] = Launcher(f, batch, warmup, Qs[k], side, capture=(k == "fused"))
        L.block_us(3)
        first = L.block_us(5) * L.calls * 1e-6
        runs[k] = max(5, int(block_seconds / max(first, 1e-7)) + 1)
    times = {k: [] for k in launchers}
    for _ in range(rounds):
        for k, L in launchers.items():
            times[k].append(L.block_us(runs[k]))
    us = {}
    for k, v in times.items():
        L = launchers[k]
        us[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                 "launch": L.launch, "calls_per_block": runs[k] * L.calls, "launches": launches[k]}
        if k == "composed":
            us[k]["not_captured_because"] = L.why
    f_, c_ = us["fused_eager"], us["composed"]
    return {"level": l, "cells": int(n), "ghost_cells": ghosts, "direct_write": direct, "rounds": rounds,
            "device": torch.cuda.get_device_name(0), "fused_vs_composed_rel_inf": differ, "us_per_call": us,
            "composed_over_fused_eager": round(c_["median_us"] / f_["median_us"], 2),
            "composed_over_fused_graph": round(c_["median_us"] / us["fused"]["median_us"], 2),
            "fused_not_slower_outside_the_spread": bool(f_["max_us"] <= c_["min_us"])}


def timings_md(mesh, results):
    s = ["# `config5_boundary_conditions`, fused against composed: timings", "",
         "Written by `scripts/bench_wall_bc.py` from the run recorded in `bench_wall_bc.json`; not edited by hand.",
         "Time per call (far field + wall of one level): median (min - max) over the alternating rounds; `launch` is how the",
         "calls of a timed block were launched; `launches` are the device kernels of one eager call.  The composed closure is not",
         f"captured: {NOT_CAPTURED}.", ""]
    for r in results:
        s += [f"## `{mesh}` level {r['level']}: {r['cells']} cells, ghost cells {r['ghost_cells']}, {r['rounds']} rounds, "
              f"{r['device']}", "", "| variant | us per call | launch | calls per block | launches per call |", "|---|---|---|---|---|"]
        for k, v in r["us_per_call"].items():
            ln = v["launches"]
            s.append(f"| {LABELS[k]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) | {v['launch']} | "
                     f"{v['calls_per_block']} | {ln.get('kernels', ln.get('not_counted'))} |")
        s += ["", f"* composed / fused, both eager: {r['composed_over_fused_eager']}; composed eager / fused in a graph: "
                  f"{r['composed_over_fused_graph']}",
              f"* fused not slower, outside the spread (max fused eager <= min composed): "
              f"{r['fused_not_slower_outside_the_spread']}",
              f"* written in the interpolating launch (per boundary partition): {r['direct_write']}", ""]
    return "\n".join(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="sphere3d_8M")
    ap.add_argument("--levels", type=int, default=2, help="coarse levels of multigrid() below the mesh")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10, help="calls captured per HIP graph")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-seconds", type=float, default=0.5, help="GPU time a timed block is sized to")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "wall_bc"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_wall_bc.py needs a GPU: nothing is measured without one")
    os.makedirs(a.out_dir, exist_ok=True)
    t0 = time.time()
    msh = bench.build_mesh(a.mesh)
    fam = [("farfield", [(d, s_) for d in (1, 2, 3) for s_ in (False, True)])]
    dom = ibamd.Domain(msh, max_partition_size=10 ** 9, hypercube_families=fam)
    levels = [dom] + list(ibamd.multigrid(dom, max_levels=a.levels)[0])
    print(f"# {a.mesh}: {[len(d) for d in levels]} cells per level, built in {time.time() - t0:.0f} s", flush=True)
    results = []
    for l, d in enumerate(levels):
        r = time_level(l, d, a.rounds, a.batch, a.warmup, a.block_seconds)
        print(json.dumps(r), flush=True)
        results.append(r)
        with open(os.path.join(a.out_dir, "bench_wall_bc.json"), "w") as f:
            json.dump({"mesh": a.mesh, "levels": results}, f, indent=1)
        with open(os.path.join(a.out_dir, "timings.md"), "w") as f:
            f.write(timings_md(a.mesh, results))


if __name__ == "__main__":
    main()
