"""Time ``residual_euler_sensor`` on the GPU against its neighbours: one JSON line per mesh, and two files under profiles/.

Per mesh (``bench.build_mesh``: ``rae2822_0.87M``, ``sphere3d_4.6M``; one partition, the synthetic Euler state of bench.py's
kind), time per sweep of
  (a) ``residual_euler_sensor``, default form (one kernel where the partition qualifies),
  (b) ``residual_euler_hll``, default form, same partition and state,
  (c) the same closure at operator granularity on the device: ``JST_sensor``, ``cell_gradient``, ``MUSCL``, ``at_owners`` /
      ``at_neighbors``, ``cfd.inviscid_fluxes`` with sensors, ``green_gauss``,
  (d) the literal form (``IBH_FORCE_GENERAL``).

How a figure is taken.  A 2-D sweep is about 6 us of GPU work and a call from Python costs several times that, so a loop of
eager calls between two events would time the interpreter.  Every variant is therefore captured, after ``--warmup`` eager
calls (they also allocate the gradient workspace, which cannot be allocated during capture), into a HIP graph of ``--batch``
sweeps ((c): one closure call) on a side stream, as bench.py does with its step loop; a timed block is that graph replayed
back to back between two device events on that stream, as often as a first short block says is needed to fill
``--block-seconds``.  The variants alternate: ``--rounds`` rounds, one block of every variant in each; the figure is the
median over the rounds and the spread (min, max) is kept.  Beside each figure ``launch`` says how its sweeps were launched:
``hip-graph xN``, or ``eager`` with the reason where a variant could not be captured (then the figure is bounded below by
the host's launch rate, and says so).  A variant that raises is recorded with its error, never replaced by another.
(a) and (b) move the same 32 / 40 B per cell (2-D / 3-D: the primitives in, the residual out).  Needs a GPU; there is no CPU
path.

Written: ``bench_euler_sensor.json`` (everything) and ``timings.md`` (the table of it) in ``--out-dir``.

    python scripts/bench_euler_sensor.py [--meshes rae2822_0.87M,sphere3d_4.6M] [--rounds 5] [--batch 20]
                                         [--block-seconds 1.0] [--out-dir profiles/euler_sensor]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ibamd  # noqa: E402
from graph_timing import noisy_euler_state, single_partition  # noqa: E402
from ibamd import cfd  # noqa: E402

IBH_FORCE_GENERAL = 1
LABELS = {"a_sensor_default": "(a) `residual_euler_sensor`, default", "b_hll_default": "(b) `residual_euler_hll`, default",
          "c_operator_granularity": "(c) the closure at operator granularity", "d_sensor_literal": "(d) literal form"}


def variants(dpart, P, R, fluid):
    nd = P.shape[1] - 2

    def ops():
        R.zero_()
        D = ibamd.JST_sensor(dpart, P[:, 0])
        for dim in range(1, nd + 1):
            gP = ibamd.cell_gradient(dpart, P, dim)
            PL, PR = ibamd.MUSCL(dpart, P, gP, dim, D=D, high_order=True)
            F = cfd.inviscid_fluxes(fluid, PL, PR, ibamd.at_owners(dpart, D, dim), ibamd.at_neighbors(dpart, D, dim), dim)
            R.sub_(ibamd.green_gauss(dpart, F, dim))

    return {"a_sensor_default": lambda: ibamd.residual_euler_sensor(dpart, P, out=R),
            "b_hll_default": lambda: ibamd.residual_euler_hll(dpart, P, out=R),
            "c_operator_granularity": ops,
            "d_sensor_literal": lambda: ibamd.residual_euler_sensor(dpart, P, out=R, flags=IBH_FORCE_GENERAL)}


class Launcher:
    """``sweeps`` sweeps of one variant per ``run()``: a captured graph of them, or (capture refused) one eager call."""

    def __init__(self, f, sweeps, warmup, R, stream):
        import torch
        self.f, self.stream, self.graph, self.sweeps, self.why = f, stream, None, sweeps, None
        with torch.cuda.stream(stream):
            for _ in range(warmup):
                f()
        stream.synchronize()
        assert bool(torch.isfinite(R).all().item()), "non-finite residual"
        g = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(g, stream=stream):
                for _ in range(sweeps):
                    f()
            self.graph = g
        except Exception as e:  # recorded beside the figure; the eager call below must still work
            self.why, self.sweeps = f"{type(e).__name__}: {e}"[:300], 1
        torch.cuda.synchronize()
        self.block_us(1)

    @property
    def launch(self):
        return f"hip-graph x{self.sweeps}" if self.graph is not None else "eager"

    def run(self):  # (on the current stream: block_us sets it)
        if self.graph is not None:
            self.graph.replay()
        else:
            self.f()

    def block_us(self, runs):
        """us per sweep of ``runs`` runs back to back between two events on the launch stream."""
        import torch
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            t0.record()
            for _ in range(runs):
                self.run()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / (runs * self.sweeps)


def time_mesh(name, rounds, batch, warmup, block_seconds):
    import torch
    dom, part = single_partition(name)
    dpart = ibamd.to_backend(part, ibamd.hip)
    P = noisy_euler_state(dpart.nc, dpart.nd)
    R = ibamd.hip(np.zeros(tuple(P.shape), np.float32))
    fns = variants(dpart, P, R, cfd.Fluid())
    nc, nd = P.shape[0], P.shape[1] - 2
    side = torch.cuda.Stream()
    launchers, runs, errors = {}, {}, {}
    for k, f in fns.items():
        try:
            L = launchers[k] = Launcher(f, 1 if k == "c_operator_granularity" else batch, warmup, R, side)
            L.block_us(3)                                              # clocks up
            first = L.block_us(10) * L.sweeps * 1e-6                   # seconds per run, from a short block
            runs[k] = max(10, int(block_seconds / max(first, 1e-7)) + 1)
        except ibamd._lib.IbhError as e:  # the library refused the call: recorded, not replaced (anything else ends the run)
            errors[k] = f"{type(e).__name__}: {e}"[:300]
            launchers.pop(k, None)
    times = {k: [] for k in launchers}
    for _ in range(rounds):
        for k, L in launchers.items():
            times[k].append(L.block_us(runs[k]))
    us = {}
    for k, v in times.items():
        L = launchers[k]
        med = statistics.median(v)
        us[k] = {"median_us": round(med, 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3), "launch": L.launch,
                 "sweeps_per_block": runs[k] * L.sweeps, "block_seconds": round(med * runs[k] * L.sweeps * 1e-6, 3)}
        if L.why:
            us[k]["not_captured_because"] = L.why
            us[k]["note"] = "eager calls: bounded below by the host's launch rate, not the kernels' time"
    out = {"mesh": name, "cells": int(nc), "nd": int(nd), "bytes_per_cell": 8 * (nd + 2), "rounds": rounds,
           "device": torch.cuda.get_device_name(0),
           "partition_info": {k: int(v) for k, v in dpart.info.items() if isinstance(v, (int, np.integer, bool))},
           "us_per_sweep": us, "errors": errors}
    m = {k: v["median_us"] for k, v in us.items()}
    if "a_sensor_default" in m:
        a = m["a_sensor_default"]
        out["TB_s_a"] = round(nc * 8 * (nd + 2) / a / 1e6, 3)
        for k, label in (("b_hll_default", "a_over_b"), ("c_operator_granularity", "c_over_a"), ("d_sensor_literal", "d_over_a")):
            if k in m:
                out[label] = round(a / m[k], 3) if label == "a_over_b" else round(m[k] / a, 2)
    return out


def timings_md(results):
    """The table of the JSON: one section per mesh."""
    s = ["# `residual_euler_sensor`: timings", "",
         "Written by `scripts/bench_euler_sensor.py` from the run recorded in `bench_euler_sensor.json`; not edited by hand.",
         "Time per sweep: median (min - max) over the alternating rounds; `launch` is how the sweeps of a timed block were",
         "launched.", ""]
    for r in results:
        s += [f"## `{r['mesh']}`: {r['cells']} cells, {r['nd']}-D, {r['bytes_per_cell']} B per cell, {r['rounds']} rounds, "
              f"{r['device']}", "", "| variant | us per sweep | launch | sweeps per block | block, s |", "|---|---|---|---|---|"]
        for k, v in r["us_per_sweep"].items():
            s.append(f"| {LABELS[k]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) | {v['launch']} | "
                     f"{v['sweeps_per_block']} | {v['block_seconds']} |")
        for k, e in r["errors"].items():
            s.append(f"| {LABELS[k]} | failed: {e} | | | |")
        s.append("")
        for key, text in (("TB_s_a", "(a) in TB/s of primitives in + residual out"), ("a_over_b", "(a) / (b)"),
                          ("c_over_a", "(c) / (a)"), ("d_over_a", "(d) / (a)")):
            if key in r:
                s.append(f"* {text}: {r[key]}")
        s.append("")
    return "\n".join(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="rae2822_0.87M,sphere3d_4.6M")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20, help="sweeps captured per HIP graph (bench.py's --graph-batch)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--block-seconds", type=float, default=1.0, help="GPU time a timed block is sized to")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "euler_sensor"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_euler_sensor.py needs a GPU: nothing is measured without one")
    os.makedirs(a.out_dir, exist_ok=True)
    results = []
    for name in a.meshes.split(","):
        r = time_mesh(name, a.rounds, a.batch, a.warmup, a.block_seconds)
        print(json.dumps(r), flush=True)
        results.append(r)
        with open(os.path.join(a.out_dir, "bench_euler_sensor.json"), "w") as f:
            json.dump(results, f, indent=1)
        with open(os.path.join(a.out_dir, "timings.md"), "w") as f:
            f.write(timings_md(results))


if __name__ == "__main__":
    main()
