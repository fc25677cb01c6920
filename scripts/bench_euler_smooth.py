"""Time the implicit residual smoothing of an Euler stage on the GPU (``smooth_residual``, ``update_euler_smoothed``) and
record what it buys a pseudo-time march: one JSON line per mesh, and files under profiles/.

Meshes (``bench.build_mesh``, one partition each): ``rae2822_0.87M`` and ``sphere3d_4.6M``.  State: Mach 0.3 with 5 % noise,
seeded; the stage sweeps ``P`` = one ``step_euler`` from the base state ``P0``; per-cell time step (smoothing serves the
pseudo-time march), ``eps = 0.5``, ``alpha = 1/4``.  Variants, alternating in one process:
  (a) ``stage``:      ``stage_euler`` -- the unsmoothed stage, one launch where the 2-D single-kernel sweep applies;
  (b) ``smoothed1``:  the sweep into ``work`` + ``update_euler_smoothed`` (``n_iter = 1``: 2 launches);
  (c) ``smoothed2``:  the sweep + ``smooth_residual(1)`` + ``update_euler_smoothed`` (``n_iter = 2``: 3 launches);
  (d) ``sweep``:      the sweep into ``work`` alone;
  (e) ``jacobi``:     one ``smooth_residual`` launch on the ``nd + 2`` columns alone;
  (f) ``fused``:      ``update_euler_smoothed`` alone;
  (g) ``update``:     ``update_euler_stage`` alone -- the yardstick: the same three passes over ``nd + 2`` columns as (e),
                      streamed, without the gather through the side table.
(c) is checked bit for bit against ``smooth_residual(2)`` + ``update_euler_stage`` before anything is timed.  A Jacobi launch
moves ``4 nv 3 + 4 2 nd`` B per cell algorithmically (R, the gathered iterate -- every row is some cell's own -- and S; the
side table); the achieved rate is given against the 8 TB/s HBM peak of an MI355X.

How a figure is taken: as in scripts/bench_euler_step.py -- a variant is captured into a HIP graph of ``--batch`` calls on a
side stream, a timed block replays it between two device events, the variants alternate over ``--rounds`` rounds; the figure
is the median with the spread (min, max).  Needs a GPU; there is no CPU path.

``--march``: on the small RAE mesh (``rae2822_37k``, free stream Mach 0.73 at 2.3 degrees, far field and slip wall by
``impose_flow_bc``) a ``local_dt``, ``rk_stages(4)`` march is run until ``||P_{n+1} - P_n||_2`` has dropped by 10^3 from its
first value, for every base scale in ``--scale`` without smoothing at 1 and 1.5 times it and with ``smoothing=(0.5, 2)`` at 1,
1.5, 2 and 3 times it; the steps needed (or the drop reached at ``--max-steps``), whether the run stayed finite and where it
did not are recorded, nothing is asserted.

``--profile-pass``: a few calls of the two new kernels and nothing else, for ``rocprofv3 --kernel-trace --stats -- python
scripts/bench_euler_smooth.py --profile-pass`` in a run of its own.

Written: ``bench_euler_smooth.json`` (everything) and ``timings.md`` (the table of it) in ``--out-dir``.

    python scripts/bench_euler_smooth.py [--meshes rae2822_0.87M,sphere3d_4.6M] [--rounds 5] [--batch 10] [--march]
                                         [--out-dir profiles/euler_smooth]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench  # noqa: E402
import ibamd  # noqa: E402
from graph_timing import noisy_euler_state, single_partition, time_variants  # noqa: E402
from ibamd import cfd  # noqa: E402
from ibamd import backend as B  # noqa: E402
from ibamd.solver import EulerMarch, rk_stages  # noqa: E402

SCALE, EPS, ALPHA = 0.75, 0.5, 0.25
HBM_PEAK = 8.0e12
LABELS = {"stage": "(a) `stage_euler`", "smoothed1": "(b) smoothed stage, n_iter = 1 (sweep + fused update)",
          "smoothed2": "(c) smoothed stage, n_iter = 2 (sweep + Jacobi + fused update)", "sweep": "(d) the sweep into `work`",
          "jacobi": "(e) one `smooth_residual` launch", "fused": "(f) `update_euler_smoothed` alone",
          "update": "(g) `update_euler_stage` alone (streamed yardstick)"}


def variants(dpart, P0, fluid):
    n, nv = P0.shape
    out, work, s1 = (B.colmajor_empty(n, nv) for _ in range(3))
    dt = ibamd.timestep_euler(dpart, P0, fluid, SCALE)
    cells = ibamd.timestep_euler(dpart, P0, fluid, SCALE, out=False, cells=B.colmajor_empty(n))
    P = B.colmajor_empty(n, nv)
    ibamd.step_euler(dpart, P0, dt, P, fluid, "hll", work=work)

    def sweep():
        return ibamd.residual_euler_hll(dpart, P, out=work, fluid=fluid)

    def smoothed1():
        sweep()
        return ibamd.update_euler_smoothed(dpart, P0, None, work, work, EPS, cells, (ALPHA,), fluid, out=out)

    def smoothed2():
        sweep()
        ibamd.smooth_residual(dpart, work, EPS, 1, out=s1)
        return ibamd.update_euler_smoothed(dpart, P0, None, work, s1, EPS, cells, (ALPHA,), fluid, out=out)

    fns = {"stage": lambda: ibamd.stage_euler(dpart, P, P0, cells, ALPHA, out, fluid, "hll", work=work),
           "smoothed1": smoothed1, "smoothed2": smoothed2, "sweep": sweep,
           "jacobi": lambda: ibamd.smooth_residual(dpart, work, EPS, 1, out=s1),
           "fused": lambda: ibamd.update_euler_smoothed(dpart, P0, None, work, s1, EPS, cells, (ALPHA,), fluid, out=out),
           "update": lambda: ibamd.update_euler_stage(P0, work, cells, ALPHA, fluid, out=out)}
    sweep()
    ref = ibamd.update_euler_stage(P0, ibamd.smooth_residual(dpart, work, EPS, 2), cells, ALPHA, fluid)
    return fns, ref


def time_mesh(name, part, rounds, batch, warmup, block_seconds):
    import torch
    dpart = ibamd.to_backend(part, ibamd.hip)
    nc, nd = dpart.nc, dpart.nd
    nv = nd + 2
    fluid = cfd.Fluid()
    fns, ref = variants(dpart, noisy_euler_state(nc, nd), fluid)
    assert torch.equal(fns["smoothed2"](), ref), f"{name}: the fused last iteration differs from smooth_residual + the update"
    st = time_variants(fns, rounds, batch, warmup, block_seconds, torch.cuda.Stream())
    jb, ub = 4 * nv * 3 + 4 * 2 * nd, 4 * nv * 3 + 4
    rate = lambda b, k: b * nc / (st[k]["median_us"] * 1e-6)  # noqa: E731
    return {"mesh": name, "cells": int(nc), "nd": nd, "rounds": rounds, "eps": EPS, "alpha": ALPHA, "dt": "per cell",
            "device": torch.cuda.get_device_name(0), "same_bits": True, "direct_sides": int(dpart.info["direct_sides"]),
            "direct_side_fraction": round(dpart.info["direct_sides"] / (2.0 * nd * nc), 4), "us": st,
            "jacobi_bytes_per_cell": jb, "jacobi_tbytes_per_s": round(rate(jb, "jacobi") / 1e12, 3),
            "jacobi_fraction_of_hbm_peak": round(rate(jb, "jacobi") / HBM_PEAK, 3),
            "update_bytes_per_cell": ub, "update_tbytes_per_s": round(rate(ub, "update") / 1e12, 3),
            "jacobi_over_update": round(st["jacobi"]["median_us"] / st["update"]["median_us"], 3),
            "fused_minus_update_us": round(st["fused"]["median_us"] - st["update"]["median_us"], 2),
            "smoothed1_over_stage": round(st["smoothed1"]["median_us"] / st["stage"]["median_us"], 3),
            "smoothed2_over_stage": round(st["smoothed2"]["median_us"] / st["stage"]["median_us"], 3)}


def march_record(scales, max_steps, mach=0.73):
    """Steps a local_dt, rk_stages(4) march on rae2822_37k needs to drop ||P_{n+1} - P_n|| by 10^3: for every base scale the
    unsmoothed march at 1 and 1.5 times it and the smoothed one at 1, 1.5, 2 and 3 times it (each combination once)."""
    import torch
    fam = [("farfield", [(1, False), (1, True), (2, False), (2, True)])]
    dom = ibamd.Domain(bench.build_mesh("rae2822_37k"), hypercube_families=fam, max_partition_size=10 ** 9)
    (part,) = dom.partitions.values()
    dpart = ibamd.to_backend(part, ibamd.hip)
    fluid = cfd.Fluid()
    a, aoa = float(np.sqrt(1.4 * 283.0 * 288.15)), np.deg2rad(2.3)
    u_inf = [mach * a * float(np.cos(aoa)), mach * a * float(np.sin(aoa))]
    far = cfd.FlowBC(fluid, [1e5, 288.15] + u_inf)
    wall = cfd.FlowBC(fluid, [1e5, 288.15, 0.0], normal_flow=True)

    def bcs(P):
        ibamd.impose_flow_bc(dom, "farfield", far, P)
        ibamd.impose_flow_bc(dom, "wall", wall, P)

    nc = dpart.nc
    start = ibamd.hip(np.tile(np.array([1e5, 288.15] + u_inf, np.float32), (nc, 1)))
    bcs(start)
    runs, todo = [], []
    for base in scales:
        for label, smoothing, factor in (("unsmoothed", None, 1.0), ("unsmoothed", None, 1.5), ("smoothed", (0.5, 2), 1.0),
                                         ("smoothed", (0.5, 2), 1.5), ("smoothed", (0.5, 2), 2.0), ("smoothed", (0.5, 2), 3.0)):
            if (label, smoothing, round(base * factor, 4)) not in todo:
                todo.append((label, smoothing, round(base * factor, 4)))
    for label, smoothing, scale in todo:
        m = EulerMarch(dpart, fluid, scale=scale, bcs=bcs, local_dt=True, stages=rk_stages(4), smoothing=smoothing)
        P, first, last, steps, finite, where = start, None, None, None, True, None
        t0 = time.time()
        for k in range(1, max_steps + 1):
            Pn = m.step(P)
            if k % 10 == 1 or k == max_steps:       # (a host read-back every tenth step: this loop measures, it does not march)
                last = float(torch.linalg.vector_norm((Pn - P).double()))
                if first is None:
                    first = last
                if not np.isfinite(last):
                    bad = torch.nonzero(~torch.isfinite(Pn).all(dim=1))[:1, 0]
                    finite, where = False, [round(float(x), 4) for x in dpart.centers[bad].flatten().tolist()]
                    break
                if last <= 1e-3 * first:
                    steps = k
                    break
            P = Pn
        runs.append({"march": label, "smoothing": list(smoothing) if smoothing else None, "scale": scale, "finite": finite,
                     "first_non_finite_cell_at": where, "steps_to_1e-3": steps, "steps_run": k, "first_norm": first, "last_norm": last,
                     "drop_reached": (last / first) if finite and first else None, "seconds": round(time.time() - t0, 1)})
        print("# march", json.dumps(runs[-1]), flush=True)
    return {"mesh": "rae2822_37k", "cells": int(nc), "stages": "rk_stages(4)", "local_dt": True, "mach": mach, "aoa_deg": 2.3,
            "base_scales": list(scales), "max_steps": max_steps, "norm_checked_every": 10, "runs": runs}


def timings_md(results, march):
    s = ["# Implicit residual smoothing of an Euler stage: timings", "",
         "Written by `scripts/bench_euler_smooth.py` from the run recorded in `bench_euler_smooth.json`; not edited by hand.",
         "Median (min - max) in us over the alternating rounds, every variant replayed from a HIP graph; eps = 0.5, alpha = 1/4,",
         "per-cell time step.", ""]
    for r in results:
        s += [f"## `{r['mesh']}`: {r['cells']} cells, {r['nd']}-D, {r['rounds']} rounds, {r['device']}", "",
              "| variant | us |", "|---|---|"]
        s += [f"| {LABELS[k]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) |" for k, v in r["us"].items()]
        s += ["", f"* a Jacobi launch: {r['jacobi_bytes_per_cell']} B per cell algorithmic, {r['jacobi_tbytes_per_s']} TB/s achieved, "
                  f"{r['jacobi_fraction_of_hbm_peak']} of the 8 TB/s HBM peak; {r['jacobi_over_update']} times the streamed "
                  f"`update_euler_stage` ({r['update_bytes_per_cell']} B per cell, {r['update_tbytes_per_s']} TB/s)",
              f"* the fused last iteration costs {r['fused_minus_update_us']:+} us over `update_euler_stage`",
              f"* a smoothed stage / `stage_euler`: {r['smoothed1_over_stage']} (n_iter = 1), {r['smoothed2_over_stage']} "
              f"(n_iter = 2); sides read directly from the side table: {r['direct_side_fraction']}", ""]
    if march:
        s += [f"## March to a steady state: `{march['mesh']}`, {march['cells']} cells, local dt, {march['stages']}, Mach "
              f"{march['mach']} at {march['aoa_deg']} degrees", "",
              f"Steps until `||P_(n+1) - P_n||_2` has dropped by 10^3 from its first value (checked every "
              f"{march['norm_checked_every']} steps, at most {march['max_steps']} steps).", "",
              "| march | scale | finite | steps to 10^-3 | last norm / first norm | steps run |", "|---|---|---|---|---|---|"]
        for r in march["runs"]:
            drop = f"{r['drop_reached']:.2e}" if r["drop_reached"] is not None else "-"
            s.append(f"| {r['march']} {r['smoothing'] or ''} | {r['scale']} | {r['finite']} | {r['steps_to_1e-3'] or '-'} | {drop} | "
                     f"{r['steps_run']} |")
        s.append("")
    return "\n".join(s)


def profile_pass(meshes):
    """The two new kernels, a few launches each, and the sweep that feeds them once."""
    import torch
    for name in meshes:
        dom, part = single_partition(name)
        dpart = ibamd.to_backend(part, ibamd.hip)
        fns, _ = variants(dpart, noisy_euler_state(dpart.nc, dpart.nd), cfd.Fluid())
        for _ in range(20):
            fns["jacobi"]()
            fns["fused"]()
        torch.cuda.synchronize()
        print(f"# {name}: 20 launches of each kernel", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="rae2822_0.87M,sphere3d_4.6M")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10, help="calls captured per HIP graph")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-seconds", type=float, default=0.3, help="GPU time a timed block is sized to")
    ap.add_argument("--march", action="store_true", help="record the steps to convergence of the small RAE march as well")
    ap.add_argument("--scale", default="0.75,0.25", help="base scales of the march record: EulerMarch's default, and the "
                                                          "largest at which the unsmoothed march was seen to stay finite")
    ap.add_argument("--mach", type=float, default=0.73, help="free-stream Mach number of the march")
    ap.add_argument("--max-steps", type=int, default=3000)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "euler_smooth"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_euler_smooth.py needs a GPU: nothing is measured without one")
    meshes = [m for m in a.meshes.split(",") if m]
    if a.profile_pass:
        return profile_pass(meshes)
    os.makedirs(a.out_dir, exist_ok=True)
    results, march = [], None

    def write():
        with open(os.path.join(a.out_dir, "bench_euler_smooth.json"), "w") as f:
            json.dump({"meshes": results, "march": march}, f, indent=1)
        with open(os.path.join(a.out_dir, "timings.md"), "w") as f:
            f.write(timings_md(results, march))

    for name in meshes:
        t0 = time.time()
        dom, part = single_partition(name)
        print(f"# {name}: {len(dom)} cells, built in {time.time() - t0:.0f} s", flush=True)
        r = time_mesh(name, part, a.rounds, a.batch, a.warmup, a.block_seconds)
        print(json.dumps(r), flush=True)
        results.append(r)
        write()
        del dom, part
    if a.march:
        march = march_record([float(x) for x in a.scale.split(",")], a.max_steps, a.mach)
        print(json.dumps(march), flush=True)
        write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
