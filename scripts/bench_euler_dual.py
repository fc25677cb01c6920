"""Time one pseudo-time stage of a dual time step on the GPU (``stage_euler_dual``) in the forms it can take: one JSON line
per mesh, and two files under profiles/.

Meshes (``bench.build_mesh``, one partition each): ``rae2822_0.87M`` -- every block eligible for the 2-D single-kernel sweep,
so ``stage_euler_dual`` is ONE launch -- and ``sphere3d_4.6M`` -- 3-D: the sweep into ``work`` and ``update_euler_dual``, two
launches whatever is asked.  State: Mach 0.3 with 5 % noise, seeded; the stage sweeps ``P`` = one ``step_euler`` from the
base state ``P0``; the source is ``dual_source(P0, P)`` with the BDF2 coefficients of a physical step of 8 x the explicit
time step.  Variants, per stage (``alpha`` = 1/3):
  (a) ``dual``:        ``stage_euler_dual`` with the global ``dt``;
  (b) ``dual_cells``:  ``stage_euler_dual`` with a per-cell ``dt``;
  (c) ``stage``:       ``stage_euler`` with the global ``dt`` (the floor: the same stage without the row of ``S``, 4 B x
                       (nd + 2) per cell, and without the divide);
  (d) ``stage_cells``: ``stage_euler`` with a per-cell ``dt``;
  (e) ``two``:         the two-launch form by hand: ``residual_euler_*`` into ``work``, then ``update_euler_dual``;
  (f) ``composed``:    the composition that defines the bits: the sweep, ``primitive2state``, per column ``R .+ S``,
                       ``ibh_update_dev`` and ``./``, ``state2primitive`` (``h = dt .* alpha`` and ``h .* g .+ 1``, one element
                       each and constant here, are taken once before the timing).
(a), (e) and (f) give the same bits (checked here before anything is timed).

How a figure is taken: as in scripts/bench_euler_step.py -- a variant is captured into a HIP graph of ``--batch`` calls on a
side stream, a timed block replays it between two device events, the variants alternate over ``--rounds`` rounds in one
process; the figure is the median with the spread (min, max).  Needs a GPU; there is no CPU path.

Written: ``bench_euler_dual.json`` (everything) and ``timings.md`` (the table of it) in ``--out-dir``.

    python scripts/bench_euler_dual.py [--meshes rae2822_0.87M,sphere3d_4.6M] [--scheme hll] [--rounds 5] [--batch 10]
                                       [--block-seconds 0.3] [--out-dir profiles/euler_dual]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import ibamd  # noqa: E402
from graph_timing import noisy_euler_state, one_launch, run_meshes, time_variants  # noqa: E402
from ibamd import _lib, cfd  # noqa: E402
from ibamd import backend as B  # noqa: E402
from ibamd.hiparray import HipArray as H  # noqa: E402
from ibamd.solver import bdf_coefficients  # noqa: E402

SCALE = 0.75
ALPHA = float(np.float32(1.0) / np.float32(3.0))
LABELS = {"dual": "(a) `stage_euler_dual`, global dt", "dual_cells": "(b) `stage_euler_dual`, per-cell dt",
          "stage": "(c) `stage_euler`, global dt", "stage_cells": "(d) `stage_euler`, per-cell dt",
          "two": "(e) two launches: sweep into `work` + `update_euler_dual`",
          "composed": "(f) composed: sweep + the defining launches"}


def variants(dpart, P0, fluid, scheme):
    """{key: callable} per stage."""
    n, nv = P0.shape
    sweep_fn = ibamd.residual_euler_hll if scheme == "hll" else ibamd.residual_euler_sensor
    out, work = B.colmajor_empty(n, nv), B.colmajor_empty(n, nv)
    dt = ibamd.timestep_euler(dpart, P0, fluid, SCALE)
    cells = ibamd.timestep_euler(dpart, P0, fluid, SCALE, out=False, cells=B.colmajor_empty(n))
    P = B.colmajor_empty(n, nv)
    ibamd.step_euler(dpart, P0, dt, P, fluid, scheme, work=work)
    cn, cm, g = bdf_coefficients(2, 8.0 * float(dt.item()))
    S = ibamd.dual_source(P0, P, cn, cm, fluid)
    h = (H(dt) * ALPHA).t
    den = float((H(h) * g + 1.0).t.item())
    Q2, num = B.colmajor_empty(n, nv), B.colmajor_empty(n)

    def two():
        sweep_fn(dpart, P, out=work, fluid=fluid)
        return ibamd.update_euler_dual(P0, work, S, dt, ALPHA, g, fluid, out=out)

    def composed():
        sweep_fn(dpart, P, out=work, fluid=fluid)
        Q0 = cfd.primitive2state(fluid, P0)
        for v in range(nv):
            RS = (H(work[:, v]) + H(S[:, v])).t
            B._stream()
            _lib.call("ibh_update_dev", n, B._ptr(h), B._ptr(Q0[:, v]), B._ptr(RS), B._ptr(num))
            Q2[:, v] = (H(num) / den).t
        return cfd.state2primitive(fluid, Q2)

    return {"dual": lambda: ibamd.stage_euler_dual(dpart, P, P0, S, dt, ALPHA, g, out, fluid, scheme, work=work),
            "dual_cells": lambda: ibamd.stage_euler_dual(dpart, P, P0, S, cells, ALPHA, g, out, fluid, scheme, work=work),
            "stage": lambda: ibamd.stage_euler(dpart, P, P0, dt, ALPHA, out, fluid, scheme, work=work),
            "stage_cells": lambda: ibamd.stage_euler(dpart, P, P0, cells, ALPHA, out, fluid, scheme, work=work),
            "two": two, "composed": composed}


def time_mesh(name, part, scheme, rounds, batch, warmup, block_seconds):
    import torch
    dpart = ibamd.to_backend(part, ibamd.hip)
    nc, nd = dpart.nc, dpart.nd
    fluid = cfd.Fluid()
    P0 = noisy_euler_state(nc, nd)
    one = one_launch(dpart)
    fns = variants(dpart, P0, fluid, scheme)
    a = fns["dual"]().clone()
    assert torch.equal(a, fns["two"]()) and torch.equal(a, fns["composed"]()), f"{name}: the forms of a dual stage differ"
    st = time_variants(fns, rounds, batch, warmup, block_seconds, torch.cuda.Stream())
    r = {"mesh": name, "cells": int(nc), "nd": nd, "scheme": scheme, "rounds": rounds, "alpha": ALPHA,
         "stage_launches": 1 if one else 2, "device": torch.cuda.get_device_name(0), "same_bits": True, "us_per_stage": st,
         "two_over_dual": round(st["two"]["median_us"] / st["dual"]["median_us"], 3),
         "composed_over_dual": round(st["composed"]["median_us"] / st["dual"]["median_us"], 3),
         # what the dual stage reads beyond the stage: the row of S, 4 B x (nd + 2) per cell
         "extra_bytes_per_cell": 4 * (nd + 2), "extra_mbytes": round(4 * (nd + 2) * nc / 1e6, 2),
         "dual_minus_stage_us": round(st["dual"]["median_us"] - st["stage"]["median_us"], 2),
         "dual_cells_minus_stage_cells_us": round(st["dual_cells"]["median_us"] - st["stage_cells"]["median_us"], 2)}
    if one:
        r["one_launch_below_two_outside_the_spread"] = bool(st["dual"]["max_us"] < st["two"]["min_us"])
    return r


def timings_md(results):
    s = ["# One pseudo-time stage of a dual time step: timings", "",
         "Written by `scripts/bench_euler_dual.py` from the run recorded in `bench_euler_dual.json`; not edited by hand.",
         "Median (min - max) over the alternating rounds of one process, every variant replayed from a HIP graph; alpha = 1/3,",
         "the BDF2 source and g of a physical step of 8 x the explicit time step, the time step given.", ""]
    for r in results:
        s += [f"## `{r['mesh']}`: {r['cells']} cells, {r['nd']}-D, scheme {r['scheme']}, `stage_euler_dual` in "
              f"{r['stage_launches']} launch(es), {r['rounds']} rounds, {r['device']}", "",
              "| variant | us per stage |", "|---|---|"]
        for key, v in r["us_per_stage"].items():
            s.append(f"| {LABELS[key]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) |")
        s += ["", f"* two launches / `stage_euler_dual`: {r['two_over_dual']}; composed / `stage_euler_dual`: "
              f"{r['composed_over_dual']}",
              f"* the row of `S` ({r['extra_bytes_per_cell']} B per cell, {r['extra_mbytes']} MB) and the divide over "
              f"`stage_euler` in the same run: +{r['dual_minus_stage_us']} us global dt, "
              f"+{r['dual_cells_minus_stage_cells_us']} us per-cell dt"]
        if "one_launch_below_two_outside_the_spread" in r:
            s.append(f"* one launch below two launches outside the spread (max one < min two): "
                     f"{r['one_launch_below_two_outside_the_spread']}")
        s.append("")
    return "\n".join(s)


def main():
    return run_meshes(sys.argv[1:], os.path.join(ROOT, "profiles", "euler_dual"), "bench_euler_dual.json", time_mesh,
                      timings_md)


if __name__ == "__main__":
    sys.exit(main())
