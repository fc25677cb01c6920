"""Time the LES closure of a velocity field on the GPU, fused (``les_closure_of``: one launch, ``ibh_les_of``) against composed
(``cell_gradient`` + ``WALE_nuSGS`` + ``Ducros_sensor``): one JSON line per level, and two files under profiles/.

Per level of ``multigrid`` over ``bench.build_mesh`` (``sphere3d_4.6M``: the fine level is one partition of complete 8^3
blocks -- the wave-per-block kernel --, its first coarse level has no block structure -- the thread-per-cell kernel), on a
seeded velocity field, the closure that wants ``nusgs`` (WALE), ``ducros`` and the gradients for its viscous terms as
  (a) ``fused``: ``les_closure_of(part, vel, Delta, model="wale", ducros=True, gradients=True)``, 1 launch;
  (b) ``composed_tuple``: the tuple ``cell_gradient(part, vel)`` and the two pointwise kernels on views of it, 1 + 2 launches;
  (c) ``composed_components``: ``cell_gradient`` per velocity component (what an LES script written against the reference
      does) and the two pointwise kernels, 3 + 2 launches -- the gradient arrays are the ones the viscous terms take.
(b) and (c) are code the fused entry does not touch.  All three give the same bits (checked here before anything is timed).
Three more legs time the other fused closures over ``cell_gradient`` alone, as the calls a V-cycle makes:
  (d) ``shear``: ``shear_rate_of_velocity(part, vel)``;  (e) ``shear_gradients``: the same with ``gradients=True``;
  (f) ``wray_agarwal``: ``Wray_Agarwal_of(part, R, S)`` on two seeded positive scalars.

How a figure is taken: after ``--warmup`` eager calls a variant is captured into a HIP graph of ``--batch`` calls on a side
stream; a timed block is that graph replayed back to back between two device events, as often as a first short block says
is needed to fill ``--block-seconds``.  The variants alternate: ``--rounds`` rounds, one block of each in every round; the
figure is the median over the rounds with the spread (min, max).  ``bytes_per_cell`` are counted from the code (what each
launch must read and write once), not measured.  Needs a GPU; there is no CPU path.

Written: ``bench_les_closure.json`` (everything) and ``timings.md`` (the table of it) in ``--out-dir``.

    python scripts/bench_les_closure.py [--mesh sphere3d_4.6M] [--levels 1] [--rounds 7] [--batch 10] [--block-seconds 0.5]
                                        [--out-dir profiles/les_closure]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import ibamd  # noqa: E402
from graph_timing import time_variants  # noqa: E402
from ibamd import turbulence as T  # noqa: E402

LABELS = {"fused": "(a) fused: `les_closure_of`", "composed_tuple": "(b) composed: tuple `cell_gradient` + 2 pointwise",
          "composed_components": "(c) composed: `cell_gradient` per component + 2 pointwise",
          "shear": "(d) `shear_rate_of_velocity`", "shear_gradients": "(e) `shear_rate_of_velocity(gradients=True)`",
          "wray_agarwal": "(f) `Wray_Agarwal_of`"}
# per cell, counted from the code (field values only; side tables, spacings and block descriptors are left out on both sides):
# fused = 12 in (velocity) + 4 (Delta) + 4 + 4 (nusgs, ducros) + 36 (gradients); the least any form moves is the same 60
# (24 without the gradients).  The composition writes the nine gradients -- on a block partition cell_gradient's sensor
# column beside every field's three -- and reads all nine back once per closure (WALE: 36 + 4 in, 4 out; Ducros: 36 in, 4 out).


def bytes_per_cell(blocks):
    grad = 3 * (4 + (16 if blocks else 12))
    return {"fused": 12 + 4 + 8 + 36, "algorithmic_without_gradients": 12 + 4 + 8, "algorithmic_with_gradients": 12 + 4 + 8 + 36,
            "composed_tuple": grad + (36 + 4 + 4) + (36 + 4), "composed_components": grad + (36 + 4 + 4) + (36 + 4),
            "shear": 12 + 4, "shear_gradients": 12 + 4 + 36, "wray_agarwal": 8 + 12}


def variants(dpart, vel, Delta, R, S):
    nd = 3

    def fused():
        r = T.les_closure_of(dpart, vel, Delta, model="wale", ducros=True, gradients=True)
        return r["nusgs"], r["ducros"], r["gradients"]

    def composed_tuple():
        gV = ibamd.cell_gradient(dpart, vel)
        g = [[gV[j][:, i] for j in range(nd)] for i in range(nd)]
        return T.WALE_nuSGS(Delta, g), T.Ducros_sensor(g), gV

    def composed_components():
        g = [list(ibamd.cell_gradient(dpart, vel[:, i])) for i in range(nd)]
        return T.WALE_nuSGS(Delta, g), T.Ducros_sensor(g), g

    return {"fused": fused, "composed_tuple": composed_tuple, "composed_components": composed_components,
            "shear": lambda: T.shear_rate_of_velocity(dpart, vel),
            "shear_gradients": lambda: T.shear_rate_of_velocity(dpart, vel, gradients=True),
            "wray_agarwal": lambda: T.Wray_Agarwal_of(dpart, R, S)}


def time_level(l, part, rounds, batch, warmup, block_seconds):
    import torch
    dpart = ibamd.to_backend(part, ibamd.hip)
    nc = dpart.nc
    path = "blocks (k_les_of3)" if T.all_blocks(dpart) else "face lists (k_les_of_cells)"
    BYTES = bytes_per_cell(T.all_blocks(dpart))
    assert T.fused_closures_apply(dpart), "the fused closure does not apply on this partition"
    rng = np.random.default_rng(12345)
    X = np.asarray(part.centers, np.float64)
    vel = ibamd.hip(np.stack([100 * (1 + 0.1 * np.sin(X[:, 1])), 10 * np.cos(X[:, 0] + X[:, 2]), 5 * np.sin(X[:, 0] * X[:, 1])],
                             axis=1).astype(np.float32) + rng.uniform(-1, 1, (nc, 3)).astype(np.float32))
    Delta = ibamd.hip(np.cbrt(np.prod(np.asarray(part.spacing, np.float64), axis=1)).astype(np.float32))
    R = ibamd.hip((1e-4 * (1.5 + np.sin(X[:, 0]) * np.cos(X[:, 2])) * (1 + 0.05 * rng.uniform(-1, 1, nc))).astype(np.float32))
    S = ibamd.hip((20 * (1.5 + np.cos(X[:, 1] + X[:, 2])) * (1 + 0.05 * rng.uniform(-1, 1, nc))).astype(np.float32))
    fns = variants(dpart, vel, Delta, R, S)
    ref = fns["fused"]()
    for k in ("composed_tuple", "composed_components"):
        nus, duc, g = fns[k]()
        assert torch.equal(nus, ref[0]) and torch.equal(duc, ref[1]), f"level {l}: {k} differs from fused"
        for j in range(3):
            for i in range(3):
                gji = g[j][:, i] if k == "composed_tuple" else g[i][j]
                assert torch.equal(gji, ref[2][j][:, i]), f"level {l}: {k} gradient ({i}, {j}) differs from fused"
    us = time_variants(fns, rounds, batch, warmup, block_seconds, torch.cuda.Stream())
    for k, v in us.items():
        v.update(bytes_per_cell=BYTES[k], counted_GB_per_s=round(BYTES[k] * nc / v["median_us"] * 1e-3, 1))
    f_ = us["fused"]
    return {"level": l, "cells": int(nc), "path": path, "rounds": rounds, "device": torch.cuda.get_device_name(0),
            "same_bits": True, "us_per_call": us, "bytes_per_cell": BYTES,
            "composed_tuple_over_fused": round(us["composed_tuple"]["median_us"] / f_["median_us"], 2),
            "composed_components_over_fused": round(us["composed_components"]["median_us"] / f_["median_us"], 2),
            "fused_faster_outside_the_spread": bool(f_["max_us"] < min(us["composed_tuple"]["min_us"],
                                                                       us["composed_components"]["min_us"]))}


def timings_md(mesh, results):
    s = ["# `les_closure_of`, fused against composed: timings", "",
         "Written by `scripts/bench_les_closure.py` from the run recorded in `bench_les_closure.json`; not edited by hand.",
         "Requested: `nusgs` (WALE), `ducros`, `gradients`.  Time per call: median (min - max) over the alternating rounds, every",
         "variant replayed from a HIP graph.  Bytes per cell are counted from the code, not measured.", ""]
    for r in results:
        s += [f"## `{mesh}` level {r['level']}: {r['cells']} cells, {r['path']}, {r['rounds']} rounds, {r['device']}", "",
              "| variant | us per call | calls per block | counted B per cell | counted GB/s |", "|---|---|---|---|---|"]
        for k, v in r["us_per_call"].items():
            s.append(f"| {LABELS[k]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) | {v['calls_per_block']} | "
                     f"{v['bytes_per_cell']} | {v['counted_GB_per_s']} |")
        s += ["", f"* composed (tuple) / fused: {r['composed_tuple_over_fused']}; composed (per component) / fused: "
                  f"{r['composed_components_over_fused']}",
              f"* fused faster than both, outside the spread (max fused < min composed): {r['fused_faster_outside_the_spread']}",
              ""]
    return "\n".join(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="sphere3d_4.6M")
    ap.add_argument("--levels", type=int, default=1, help="coarse levels of multigrid() below the mesh")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=10, help="calls captured per HIP graph")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-seconds", type=float, default=0.5, help="GPU time a timed block is sized to")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "les_closure"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_les_closure.py needs a GPU: nothing is measured without one")
    os.makedirs(a.out_dir, exist_ok=True)
    t0 = time.time()
    dom = ibamd.Domain(bench.build_mesh(a.mesh), max_partition_size=10 ** 9, boundaries=False)
    levels = [dom] + (list(ibamd.multigrid(dom, max_levels=a.levels)[0]) if a.levels else [])
    print(f"# {a.mesh}: {[len(d) for d in levels]} cells per level, built in {time.time() - t0:.0f} s", flush=True)
    results = []
    for l, d in enumerate(levels):
        part = next(iter(d.partitions.values()))   # (one partition per level: max_partition_size above)
        r = time_level(l, part, a.rounds, a.batch, a.warmup, a.block_seconds)
        print(json.dumps(r), flush=True)
        results.append(r)
        with open(os.path.join(a.out_dir, "bench_les_closure.json"), "w") as f:
            json.dump({"mesh": a.mesh, "levels": results}, f, indent=1)
        with open(os.path.join(a.out_dir, "timings.md"), "w") as f:
            f.write(timings_md(a.mesh, results))


if __name__ == "__main__":
    main()
