"""Time the right-hand sides of the standard k-epsilon model on the GPU, fused (``k_epsilon_rhs``: one launch,
``ibh_k_epsilon_rhs``) against the four-launch composition it replaces (``shear_rate_of_velocity``, ``standard_k_epsilon``,
two ``scalar_transport``): one JSON line per level, and two files under profiles/.

Per level of ``multigrid`` over ``bench.build_mesh`` (``sphere3d_4.6M``: the fine level is one partition of complete 8^3
blocks -- the wave-per-block kernel ``k_k_epsilon_rhs3`` --, its first coarse level has no block structure -- the
thread-per-cell kernel ``k_k_epsilon_rhs_cells``), on seeded fields (k in [0.5, 2], eps in [1, 4]):
  (a) ``fused``: ``k_epsilon_rhs(part, vel, k, eps, nu)``, 1 launch, writes rk, reps, nut;
  (b) ``composed``: the four calls, which write S, then nuk, nueps, Sk, Seps, nut, then rk, then reps.
Both give the same bits (checked here before anything is timed).  The composition's kernels are the ones the project had
before the fused entry (the block transport kernel now calls the shared device body).

How a figure is taken: after ``--warmup`` eager calls a variant is captured into a HIP graph of ``--batch`` calls on a side
stream; a timed block is that graph replayed back to back between two device events, as often as a first short block says
is needed to fill ``--block-seconds``.  The variants alternate: ``--rounds`` rounds, one block of each in every round; the
figure is the median over the rounds with the spread (min, max).  ``bytes_per_cell`` are counted from the code (what each
launch must read and write once; side tables, spacings and block descriptors left out on both sides), not measured.  Needs a
GPU; there is no CPU path.

Written: ``bench_k_epsilon.json`` (everything) and ``timings.md`` (the table of it) in ``--out-dir``.

    python scripts/bench_k_epsilon.py [--mesh sphere3d_4.6M] [--levels 1] [--rounds 5] [--batch 10] [--block-seconds 0.3]
                                      [--out-dir profiles/k_epsilon]
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

NU = 1.5e-5
LABELS = {"fused": "(a) fused: `k_epsilon_rhs`, 1 launch", "composed": "(b) composed: 4 launches"}
# per cell: fused = 12 (velocity) + 4 + 4 (k, eps) in, 4 + 4 + 4 (rk, reps, nut) out; composed = shear_rate_of_velocity 12 in
# + 4 out, standard_k_epsilon 12 in + 20 out, scalar_transport 24 in + 4 out, twice
BYTES = {"fused": 20 + 12, "composed": (12 + 4) + (12 + 20) + 2 * (24 + 4)}


def variants(dpart, vel, k, eps):
    def fused():
        r = T.k_epsilon_rhs(dpart, vel, k, eps, NU)
        return r["rk"], r["reps"], r["nut"]

    def composed():
        S = T.shear_rate_of_velocity(dpart, vel)
        ke = T.standard_k_epsilon(k, eps, S)
        return (T.scalar_transport(dpart, k, ke["nuk"], vel, NU, ke["Sk"]),
                T.scalar_transport(dpart, eps, ke["nueps"], vel, NU, ke["Seps"]), ke["nut"])

    return {"fused": fused, "composed": composed}


def time_level(l, part, rounds, batch, warmup, block_seconds):
    import torch
    dpart = ibamd.to_backend(part, ibamd.hip)
    nc = dpart.nc
    path = "blocks (k_k_epsilon_rhs3)" if T.all_blocks(dpart) else "face lists (k_k_epsilon_rhs_cells)"
    assert T.fused_closures_apply(dpart), "the fused closure does not apply on this partition"
    rng = np.random.default_rng(12345)
    X = np.asarray(part.centers, np.float64)
    vel = ibamd.hip(np.stack([100 * (1 + 0.1 * np.sin(X[:, 1])), 10 * np.cos(X[:, 0] + X[:, 2]), 5 * np.sin(X[:, 0] * X[:, 1])],
                             axis=1).astype(np.float32) + rng.uniform(-1, 1, (nc, 3)).astype(np.float32))
    k = ibamd.hip(((1.25 + 0.65 * np.sin(1.3 * X[:, 0]) * np.cos(0.9 * X[:, 2])) * (1 + 0.05 * rng.uniform(-1, 1, nc))).astype(np.float32))
    eps = ibamd.hip(((2.5 + 1.3 * np.cos(1.1 * X[:, 1]) * np.sin(0.7 * X[:, 0])) * (1 + 0.05 * rng.uniform(-1, 1, nc))).astype(np.float32))
    fns = variants(dpart, vel, k, eps)
    ref, comp = fns["fused"](), fns["composed"]()
    for a, b, name in zip(ref, comp, ("rk", "reps", "nut")):
        assert torch.equal(a, b), f"level {l}: {name} of the composition differs from fused"
    us = time_variants(fns, rounds, batch, warmup, block_seconds, torch.cuda.Stream())
    for key, v in us.items():
        v.update(bytes_per_cell=BYTES[key], counted_GB_per_s=round(BYTES[key] * nc / v["median_us"] * 1e-3, 1))
    f_, c_ = us["fused"], us["composed"]
    return {"level": l, "cells": int(nc), "path": path, "rounds": rounds, "device": torch.cuda.get_device_name(0),
            "same_bits": True, "us_per_call": us, "bytes_per_cell": BYTES,
            "composed_over_fused": round(c_["median_us"] / f_["median_us"], 2),
            "fused_faster_outside_the_spread": bool(f_["max_us"] < c_["min_us"])}


def timings_md(mesh, results):
    s = ["# `k_epsilon_rhs`, fused against composed: timings", "",
         "Written by `scripts/bench_k_epsilon.py` from the run recorded in `bench_k_epsilon.json`; not edited by hand.",
         "Outputs: `rk`, `reps`, `nut`.  Time per call: median (min - max) over the alternating rounds, every variant replayed",
         "from a HIP graph.  Bytes per cell are counted from the code, not measured.", ""]
    for r in results:
        s += [f"## `{mesh}` level {r['level']}: {r['cells']} cells, {r['path']}, {r['rounds']} rounds, {r['device']}", "",
              "| variant | us per call | calls per block | counted B per cell | counted GB/s |", "|---|---|---|---|---|"]
        for key, v in r["us_per_call"].items():
            s.append(f"| {LABELS[key]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) | {v['calls_per_block']} | "
                     f"{v['bytes_per_cell']} | {v['counted_GB_per_s']} |")
        s += ["", f"* composed / fused: {r['composed_over_fused']}",
              f"* fused faster outside the spread (max fused < min composed): {r['fused_faster_outside_the_spread']}", ""]
    return "\n".join(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default="sphere3d_4.6M")
    ap.add_argument("--levels", type=int, default=1, help="coarse levels of multigrid() below the mesh")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10, help="calls captured per HIP graph")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-seconds", type=float, default=0.3, help="GPU time a timed block is sized to")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "k_epsilon"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_k_epsilon.py needs a GPU: nothing is measured without one")
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
        with open(os.path.join(a.out_dir, "bench_k_epsilon.json"), "w") as f:
            json.dump({"mesh": a.mesh, "levels": results}, f, indent=1)
        with open(os.path.join(a.out_dir, "timings.md"), "w") as f:
            f.write(timings_md(a.mesh, results))


if __name__ == "__main__":
    main()
