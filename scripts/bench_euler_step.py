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
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ibamd  # noqa: E402
from graph_timing import noisy_euler_state, one_launch, run_meshes, time_variants  # noqa: E402
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


def time_mesh(name, part, scheme, rounds, batch, warmup, block_seconds):
    import torch
    dpart = ibamd.to_backend(part, ibamd.hip)
    nc, nd = dpart.nc, dpart.nd
    fluid = cfd.Fluid()
    P = noisy_euler_state(nc, nd)
    one = one_launch(dpart)
    fns = variants(dpart, P, fluid, scheme)
    a, b = fns["fused"](), fns["composed"]()
    assert torch.equal(a, b), f"{name}: the composed step differs from the fused one"
    us = time_variants(fns, rounds, batch, warmup, block_seconds, torch.cuda.Stream())
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
    return run_meshes(sys.argv[1:], os.path.join(ROOT, "profiles", "euler_step"), "bench_euler_step.json", time_mesh,
                      timings_md, batch_help="steps captured per HIP graph")


if __name__ == "__main__":
    sys.exit(main())
