"""Time one Shu-Osher stage of a strong-stability-preserving Runge-Kutta step on the GPU (``stage_euler_ssp``) and a whole
SSPRK3 step, in the forms the stage can take: one JSON line per mesh, and two files under profiles/.

Meshes (``bench.build_mesh``, one partition each): ``rae2822_0.87M`` -- every block eligible for the 2-D single-kernel sweep,
so ``stage_euler_ssp`` is ONE launch -- and ``sphere3d_4.6M`` -- 3-D: the sweep into ``work`` and ``update_euler_ssp``, two
launches whatever is asked.  State: Mach 0.3 with 5 % noise, seeded; the stage sweeps ``P`` = one ``step_euler`` from the
base state ``P0``, so the two arrays differ.  Variants, per stage (``(a, b, c) = (3/4, 1/4, 1/4)``) and per three-stage step
(the arrays rotated as ``solver.EulerMarch`` rotates them, the time step given):
  (a) ``ssp``:         ``stage_euler_ssp`` with the global ``dt``; per step ``ssp_stages(3)`` as ``EulerMarch`` runs it (the
                       first stage, ``(0, 1, 1)``, is ``stage_euler``);
  (b) ``ssp_cells``:   the same with a per-cell ``dt``;
  (c) ``two``:         the two-launch form by hand: ``residual_euler_*`` into ``work``, then ``update_euler_ssp``
                       (``update_euler_stage`` for the first stage of a step);
  (d) ``composed``:    the composition that defines the bits: the sweep, two ``primitive2state``, ``dt .* c`` and per column
                       ``Q0 .* a .+ Q .* b`` by the broadcast layer, ``ibh_update_dev`` per column, ``state2primitive``;
  (e) ``stage``:       ``stage_euler`` of the low-storage family in the same run, for comparison (``alpha`` = 1/4; per step
                       ``rk_stages(3)``).
(a), (c) and (d) give the same bits (checked here before anything is timed).

How a figure is taken: as in scripts/bench_euler_step.py -- a variant is captured into a HIP graph of ``--batch`` calls on a
side stream, a timed block replays it between two device events, the variants alternate over ``--rounds`` rounds; the figure
is the median with the spread (min, max).  Needs a GPU; there is no CPU path.

The dispatch rule this table serves: the one-launch instantiations stay in ``ibh_stage_euler_ssp``'s dispatch only if their
range (min - max) lies below the two-launch form's without overlap, per stage and per step, in one run on one box.

Written: ``bench_euler_ssp.json`` (everything) and ``timings.md`` (the table of it) in ``--out-dir``.

    python scripts/bench_euler_ssp.py [--meshes rae2822_0.87M,sphere3d_4.6M] [--scheme hll] [--rounds 5] [--batch 10]
                                      [--block-seconds 0.3] [--out-dir profiles/euler_ssp]
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
from ibamd import _lib  # noqa: E402
from ibamd.solver import rk_stages, ssp_stages  # noqa: E402

SCALE = 0.75
ABC = (0.75, 0.25, 0.25)
LABELS = {"ssp": "(a) `stage_euler_ssp`, global dt", "ssp_cells": "(b) `stage_euler_ssp`, per-cell dt",
          "two": "(c) two launches: sweep into `work` + `update_euler_ssp`",
          "composed": "(d) composed: sweep + 2 `primitive2state` + broadcasts + `ibh_update_dev` + `state2primitive`",
          "stage": "(e) `stage_euler` (low-storage stage; per step `rk_stages(3)`)"}


def variants(dpart, P0, fluid, scheme):
    """{key: callable} per stage and per three-stage step."""
    n, nv = P0.shape
    sweep_fn = ibamd.residual_euler_hll if scheme == "hll" else ibamd.residual_euler_sensor
    out, work = B.colmajor_empty(n, nv), B.colmajor_empty(n, nv)
    bufs = (B.colmajor_empty(n, nv), B.colmajor_empty(n, nv))
    dt = ibamd.timestep_euler(dpart, P0, fluid, SCALE)
    cells = ibamd.timestep_euler(dpart, P0, fluid, SCALE, out=False, cells=B.colmajor_empty(n))
    P = B.colmajor_empty(n, nv)
    ibamd.step_euler(dpart, P0, dt, P, fluid, scheme, work=work)
    f32 = lambda x: float(np.float32(x))  # noqa: E731

    def plain(abc):
        return abc[0] == 0.0 and abc[1] == 1.0

    def one(src, abc, o, h=dt):
        if plain(abc):          # as EulerMarch runs it: no blend, the low-storage stage on the previous stage itself
            return ibamd.stage_euler(dpart, src, src, h, abc[2], o, fluid, scheme, work=work)
        return ibamd.stage_euler_ssp(dpart, src, P0, h, *abc, o, fluid, scheme, work=work)

    def two(src, abc, o):
        sweep_fn(dpart, src, out=work, fluid=fluid)
        if plain(abc):
            return ibamd.update_euler_stage(src, work, dt, abc[2], fluid, out=o)
        return ibamd.update_euler_ssp(P0, src, work, dt, *abc, fluid, out=o)

    def composed(src, abc, o):
        sweep_fn(dpart, src, out=work, fluid=fluid)
        if plain(abc):
            return ibamd.update_euler(src, work, (H(dt) * f32(abc[2])).t, fluid, out=o)
        a, b, c = (f32(x) for x in abc)
        Q0, Q = cfd.primitive2state(fluid, P0), cfd.primitive2state(fluid, src)
        dts = (H(dt) * c).t
        Q2 = B.colmajor_empty(n, nv)
        for v in range(nv):
            T = (H(Q0[:, v]) * a + H(Q[:, v]) * b).t
            B._stream()
            _lib.call("ibh_update_dev", n, B._ptr(dts), B._ptr(T), B._ptr(work[:, v]), B._ptr(Q2[:, v]))
        o.copy_(cfd.state2primitive(fluid, Q2))       # (one more copy than the six kinds of launch: into the caller's array)
        return o

    def low_storage(src, alpha, o):
        return ibamd.stage_euler(dpart, src, P0, dt, alpha, o, fluid, scheme, work=work)

    def three(stage, coeffs):
        def f():
            src = P0
            for k, c in enumerate(coeffs):
                src = stage(src, c, bufs[k % 2])
            return src
        return f

    per_stage = {"ssp": lambda: one(P, ABC, out), "ssp_cells": lambda: one(P, ABC, out, cells),
                 "two": lambda: two(P, ABC, out), "composed": lambda: composed(P, ABC, out),
                 "stage": lambda: low_storage(P, ABC[2], out)}
    per_step = {"ssp": three(one, ssp_stages(3)), "ssp_cells": three(lambda s, c, o: one(s, c, o, cells), ssp_stages(3)),
                "two": three(two, ssp_stages(3)), "composed": three(composed, ssp_stages(3)),
                "stage": three(low_storage, rk_stages(3))}
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
        a = fns["ssp"]().clone()
        assert torch.equal(a, fns["two"]()) and torch.equal(a, fns["composed"]()), f"{name}: the forms of a stage differ"
    side = torch.cuda.Stream()
    st = time_variants(per_stage, rounds, batch, warmup, block_seconds, side)
    sp = time_variants(per_step, rounds, max(1, batch // 3), warmup, block_seconds, side)
    r = {"mesh": name, "cells": int(nc), "nd": nd, "scheme": scheme, "rounds": rounds, "abc": list(ABC),
         "stage_launches": 1 if one else 2, "device": torch.cuda.get_device_name(0), "same_bits": True,
         "us_per_stage": st, "us_per_3_stage_step": sp,
         "two_over_ssp": round(st["two"]["median_us"] / st["ssp"]["median_us"], 3),
         "composed_over_ssp": round(st["composed"]["median_us"] / st["ssp"]["median_us"], 3),
         "ssp_over_stage": round(st["ssp"]["median_us"] / st["stage"]["median_us"], 3),
         "ssp_minus_stage_us": round(st["ssp"]["median_us"] - st["stage"]["median_us"], 2),
         "ssp_step_over_rk_step": round(sp["ssp"]["median_us"] / sp["stage"]["median_us"], 3),
         # what the Shu-Osher stage reads beyond the low-storage stage: in one launch nothing -- the second row is the swept
         # state the cell already holds -- and in two launches the row of P (4 B x (nd + 2)) in the update
         "extra_bytes_per_cell": {"one_launch": 0, "two_launches": 4 * (nd + 2)},
         "extra_mbytes": {"one_launch": 0.0, "two_launches": round(4 * (nd + 2) * nc / 1e6, 2)}}
    if one:
        r["one_launch_below_two_outside_the_spread"] = {
            "per_stage": bool(st["ssp"]["max_us"] < st["two"]["min_us"]),
            "per_stage_cells": bool(st["ssp_cells"]["max_us"] < st["two"]["min_us"]),
            "per_step": bool(sp["ssp"]["max_us"] < sp["two"]["min_us"]),
            "per_step_cells": bool(sp["ssp_cells"]["max_us"] < sp["two"]["min_us"])}
    return r


def timings_md(results):
    s = ["# One Shu-Osher stage of an Euler step, and an SSPRK3 step: timings", "",
         "Written by `scripts/bench_euler_ssp.py` from the run recorded in `bench_euler_ssp.json`; not edited by hand.",
         "Median (min - max) over the alternating rounds, every variant replayed from a HIP graph; (a, b, c) = (3/4, 1/4, 1/4)",
         "per stage, `ssp_stages(3)` per step (row (e): `rk_stages(3)`), the time step given.", ""]
    for r in results:
        s += [f"## `{r['mesh']}`: {r['cells']} cells, {r['nd']}-D, scheme {r['scheme']}, `stage_euler_ssp` in "
              f"{r['stage_launches']} launch(es), {r['rounds']} rounds, {r['device']}", "",
              "| variant | us per stage | us per 3-stage step |", "|---|---|---|"]
        for key, v in r["us_per_stage"].items():
            w = r["us_per_3_stage_step"].get(key)
            step = f"{w['median_us']} ({w['min_us']} - {w['max_us']})" if w else "-"
            s.append(f"| {LABELS[key]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) | {step} |")
        e = r["extra_bytes_per_cell"]
        s += ["", f"* two launches / `stage_euler_ssp`, per stage: {r['two_over_ssp']}; composed / `stage_euler_ssp`: "
                  f"{r['composed_over_ssp']}",
              f"* `stage_euler_ssp` / `stage_euler`, per stage: {r['ssp_over_stage']} ({r['ssp_minus_stage_us']:+} us); "
              f"SSPRK3 step / `rk_stages(3)` step: {r['ssp_step_over_rk_step']}",
              f"* the second base row: {e['one_launch']} B per cell more read than `stage_euler` in one launch (the swept state is "
              f"in the cell's registers; both read {e['two_launches']} B per cell more than `step_euler`, the row of `P0`), {e['two_launches']} B per cell ({r['extra_mbytes']['two_launches']} MB) in the update "
              f"of the two-launch form"]
        if "one_launch_below_two_outside_the_spread" in r:
            o = r["one_launch_below_two_outside_the_spread"]
            keep = all(o.values())
            s.append(f"* one launch below two launches outside the spread (max one < min two): per stage {o['per_stage']} "
                     f"(per-cell dt {o['per_stage_cells']}), per step {o['per_step']} (per-cell dt {o['per_step_cells']}) -- the "
                     f"rule {'keeps the one-launch instantiations in' if keep else 'sends these forms to two launches in'} the "
                     f"dispatch")
        s.append("")
    return "\n".join(s)


def main():
    return run_meshes(sys.argv[1:], os.path.join(ROOT, "profiles", "euler_ssp"), "bench_euler_ssp.json", time_mesh,
                      timings_md, batch_help="stages captured per HIP graph (a third as many 3-stage steps)")


if __name__ == "__main__":
    sys.exit(main())
