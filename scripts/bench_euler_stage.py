"""Time one Runge-Kutta stage of an Euler step on the GPU (``stage_euler``) and a whole 4-stage step, in the forms the stage
can take: one JSON line per mesh, and two files under profiles/.

Meshes (``bench.build_mesh``, one partition each): ``rae2822_0.87M`` -- every block eligible for the 2-D single-kernel sweep,
so ``stage_euler`` is ONE launch -- and ``sphere3d_4.6M`` -- 3-D: the sweep into ``work`` and ``update_euler_stage``, two
launches whatever is asked.  State: Mach 0.3 with 5 % noise, seeded; the stage sweeps ``P`` = one ``step_euler`` from the
base state ``P0``, so the two arrays differ.  Variants, per stage (``alpha`` = 1/3) and per 4-stage step (``rk_stages(4)``,
the arrays rotated as ``solver.EulerMarch`` rotates them, the time step given):
  (a) ``stage``:       ``stage_euler`` with the global ``dt``;
  (b) ``stage_cells``: ``stage_euler`` with a per-cell ``dt``;
  (c) ``step``:        ``step_euler`` alone (forward Euler: the floor of a stage; per stage only);
  (d) ``two``:         the two-launch form by hand: ``residual_euler_*`` into ``work``, then ``update_euler_stage``;
  (e) ``composed``:    the composition that defines the bits: the sweep, ``dt .* alpha`` by the broadcast layer,
                       ``update_euler``.
(a), (d) and (e) give the same bits (checked here before anything is timed).

How a figure is taken: as in scripts/bench_euler_step.py -- a variant is captured into a HIP graph of ``--batch`` calls on a
side stream, a timed block replays it between two device events, the variants alternate over ``--rounds`` rounds; the figure
is the median with the spread (min, max).  Needs a GPU; there is no CPU path.

Written: ``bench_euler_stage.json`` (everything) and ``timings.md`` (the table of it) in ``--out-dir``.

    python scripts/bench_euler_stage.py [--meshes rae2822_0.87M,sphere3d_4.6M] [--scheme hll] [--rounds 5] [--batch 10]
                                        [--block-seconds 0.3] [--out-dir profiles/euler_stage]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import ibamd  # noqa: E402
from graph_timing import noisy_euler_state, one_launch, run_meshes, time_variants  # noqa: E402
from ibamd import cfd  # noqa: E402
from ibamd import backend as B  # noqa: E402
from ibamd.hiparray import HipArray as H  # noqa: E402
from ibamd.solver import rk_stages  # noqa: E402

SCALE = 0.75
ALPHA = float(np.float32(1.0) / np.float32(3.0))
LABELS = {"stage": "(a) `stage_euler`, global dt", "stage_cells": "(b) `stage_euler`, per-cell dt",
          "step": "(c) `step_euler` (forward Euler)", "two": "(d) two launches: sweep into `work` + `update_euler_stage`",
          "composed": "(e) composed: sweep + `dt .* alpha` + `update_euler`"}


def variants(dpart, P0, fluid, scheme):
    """{key: callable} per stage and per 4-stage step."""
    n, nv = P0.shape
    sweep_fn = ibamd.residual_euler_hll if scheme == "hll" else ibamd.residual_euler_sensor
    out, work = B.colmajor_empty(n, nv), B.colmajor_empty(n, nv)
    bufs = (B.colmajor_empty(n, nv), B.colmajor_empty(n, nv))
    dt = ibamd.timestep_euler(dpart, P0, fluid, SCALE)
    cells = ibamd.timestep_euler(dpart, P0, fluid, SCALE, out=False, cells=B.colmajor_empty(n))
    P = B.colmajor_empty(n, nv)
    ibamd.step_euler(dpart, P0, dt, P, fluid, scheme, work=work)

    def one(src, a, o, h=dt):
        return ibamd.stage_euler(dpart, src, P0, h, a, o, fluid, scheme, work=work)

    def two(src, a, o):
        sweep_fn(dpart, src, out=work, fluid=fluid)
        return ibamd.update_euler_stage(P0, work, dt, a, fluid, out=o)

    def composed(src, a, o):
        sweep_fn(dpart, src, out=work, fluid=fluid)
        return ibamd.update_euler(P0, work, (H(dt) * a).t, fluid, out=o)

    def four(stage):
        def f():
            src = P0
            for k, a in enumerate(rk_stages(4)):
                src = stage(src, a, bufs[k % 2])
            return src
        return f

    per_stage = {"stage": lambda: one(P, ALPHA, out), "stage_cells": lambda: one(P, ALPHA, out, cells),
                 "step": lambda: ibamd.step_euler(dpart, P, dt, out, fluid, scheme, work=work),
                 "two": lambda: two(P, ALPHA, out), "composed": lambda: composed(P, ALPHA, out)}
    per_step = {"stage": four(one), "stage_cells": four(lambda s, a, o: one(s, a, o, cells)), "two": four(two),
                "composed": four(composed)}
    return per_stage, per_step


def time_mesh(name, part, scheme, rounds, batch, warmup, block_seconds):
    import torch
    dpart = ibamd.to_backend(part, ibamd.hip)
    nc, nd = dpart.nc, dpart.nd
    fluid = cfd.Fluid()
    P0 = noisy_euler_state(nc, nd)
    one = one_launch(dpart)
    per_stage, per_step = variants(dpart, P0, fluid, scheme)
    for fns in (per_stage, per_step):
        a = fns["stage"]().clone()
        assert torch.equal(a, fns["two"]()) and torch.equal(a, fns["composed"]()), f"{name}: the forms of a stage differ"
    side = torch.cuda.Stream()
    st = time_variants(per_stage, rounds, batch, warmup, block_seconds, side)
    sp = time_variants(per_step, rounds, max(1, batch // 4), warmup, block_seconds, side)
    r = {"mesh": name, "cells": int(nc), "nd": nd, "scheme": scheme, "rounds": rounds, "alpha": ALPHA,
         "stage_launches": 1 if one else 2, "device": torch.cuda.get_device_name(0), "same_bits": True,
         "us_per_stage": st, "us_per_4_stage_step": sp,
         "two_over_stage": round(st["two"]["median_us"] / st["stage"]["median_us"], 3),
         "stage_over_step": round(st["stage"]["median_us"] / st["step"]["median_us"], 3),
         "stage_cells_over_step": round(st["stage_cells"]["median_us"] / st["step"]["median_us"], 3),
         "stage_minus_step_us": round(st["stage"]["median_us"] - st["step"]["median_us"], 2),
         "stage_cells_minus_step_us": round(st["stage_cells"]["median_us"] - st["step"]["median_us"], 2),
         # what the stage reads beyond the step: the row of P0 (4 B x (nd + 2)), and 4 B of dt per cell with a local dt
         "extra_bytes_per_cell": {"stage": 4 * (nd + 2), "stage_cells": 4 * (nd + 2) + 4},
         "extra_mbytes": {"stage": round(4 * (nd + 2) * nc / 1e6, 2), "stage_cells": round((4 * (nd + 2) + 4) * nc / 1e6, 2)}}
    if one:
        r["one_launch_below_two_outside_the_spread"] = bool(st["stage"]["max_us"] < st["two"]["min_us"])
        r["one_launch_step_below_two_outside_the_spread"] = bool(sp["stage"]["max_us"] < sp["two"]["min_us"])
    return r


def timings_md(results):
    s = ["# One Runge-Kutta stage of an Euler step, and a 4-stage step: timings", "",
         "Written by `scripts/bench_euler_stage.py` from the run recorded in `bench_euler_stage.json`; not edited by hand.",
         "Median (min - max) over the alternating rounds, every variant replayed from a HIP graph; alpha = 1/3 per stage,",
         "`rk_stages(4)` per step, the time step given.", ""]
    for r in results:
        s += [f"## `{r['mesh']}`: {r['cells']} cells, {r['nd']}-D, scheme {r['scheme']}, `stage_euler` in "
              f"{r['stage_launches']} launch(es), {r['rounds']} rounds, {r['device']}", "",
              "| variant | us per stage | us per 4-stage step |", "|---|---|---|"]
        for key, v in r["us_per_stage"].items():
            w = r["us_per_4_stage_step"].get(key)
            step = f"{w['median_us']} ({w['min_us']} - {w['max_us']})" if w else "-"
            s.append(f"| {LABELS[key]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) | {step} |")
        s += ["", f"* two launches / `stage_euler`, per stage: {r['two_over_stage']}",
              f"* `stage_euler` / `step_euler`: {r['stage_over_step']} global dt (+{r['stage_minus_step_us']} us for "
              f"{r['extra_mbytes']['stage']} MB more read: {r['extra_bytes_per_cell']['stage']} B per cell), "
              f"{r['stage_cells_over_step']} per-cell dt (+{r['stage_cells_minus_step_us']} us for "
              f"{r['extra_mbytes']['stage_cells']} MB: {r['extra_bytes_per_cell']['stage_cells']} B per cell)"]
        if "one_launch_below_two_outside_the_spread" in r:
            s.append(f"* one launch below two launches outside the spread (max one < min two): per stage "
                     f"{r['one_launch_below_two_outside_the_spread']}, per 4-stage step "
                     f"{r['one_launch_step_below_two_outside_the_spread']}")
        s.append("")
    return "\n".join(s)


def main():
    return run_meshes(sys.argv[1:], os.path.join(ROOT, "profiles", "euler_stage"), "bench_euler_stage.json", time_mesh,
                      timings_md, batch_help="stages captured per HIP graph (a quarter as many 4-stage steps)")


if __name__ == "__main__":
    sys.exit(main())
