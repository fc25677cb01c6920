"""Time the multigrid transfers of the Euler march on the GPU (``restrict_euler``, ``prolong_euler``) against the compositions
of launches they replace, and write down the residual history of ``MultigridMarch`` against the single-grid march: one JSON
line per measurement, and three files under profiles/.

Transfers (``--meshes``, ``bench.build_mesh``, one partition each, the operators of ``multigrid(dom, max_levels=1)``; state: Mach
0.3 with 5 % noise, seeded; ``R`` one sweep of it, ``S`` a BDF2 source), per call:
  (a) ``restrict``:          ``restrict_euler`` -- one launch;
  (b) ``restrict_composed``: ``primitive2state``, the broadcast ``R .+ S``, the coarsener applied twice, ``state2primitive``;
  (c) ``prolong``:           ``prolong_euler`` -- two launches, ``P_out`` another array than ``P_f``;
  (d) ``prolong_composed``:  ``primitive2state`` three times, ``prolongator.diff_add``, ``state2primitive``.
(a) and (b), (c) and (d) give the same bits (checked here before anything is timed).  The parent of the change that added the
fused entries has none of them: the compositions of its own launches are the baseline.  How a figure is taken:
scripts/graph_timing.py -- HIP graphs of ``--batch`` calls replayed between device events, the variants alternating over
``--rounds`` rounds in one process; median (min - max).

History (``--history-mesh``, with its far-field and wall boundaries, Mach 0.5 at zero incidence from the free stream): the
single-grid ``EulerMarch(local_dt=True, stages=4)`` and V-cycles of ``MultigridMarch(stages=4)`` on 2 and 3 levels, each for
``--history-sweeps`` fine-level sweeps; ``||R_rho||_2`` over all rows of the fine array every few steps, against work units
(sweeps weighted by the level's cell count, in fine-level sweeps) and against wall time (eager calls, the device synchronised
at every sample).  Written down, not asserted.  Needs a GPU; there is no CPU path.

    python scripts/bench_euler_mg.py [--meshes rae2822_0.87M,sphere3d_4.6M] [--history-mesh rae2822_0.87M | none]
                                     [--history-sweeps 280] [--scale 0.3] [--rounds 5] [--out-dir profiles/euler_mg]
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
from graph_timing import noisy_euler_state, time_variants  # noqa: E402
from ibamd import cfd  # noqa: E402
from ibamd import backend as B  # noqa: E402
from ibamd.hiparray import HipArray as H  # noqa: E402
from ibamd.solver import EulerMarch, MultigridMarch  # noqa: E402

LABELS = {"restrict": "(a) `restrict_euler`", "restrict_composed": "(b) restriction composed",
          "prolong": "(c) `prolong_euler`", "prolong_composed": "(d) prolongation composed"}
FAMILIES = [("farfield", [(1, False), (1, True), (2, False), (2, True)])]


def part_of(dom):
    return next(iter(dom.partitions.values()))


def time_transfers(name, rounds, batch, warmup, block_seconds):
    import torch
    t0 = time.time()
    dom = ibamd.Domain(bench.build_mesh(name), max_partition_size=10 ** 9, boundaries=False)
    (cdom,), (pro,), (coa,) = ibamd.multigrid(dom, max_levels=1)
    print(f"# {name}: {len(dom)} -> {len(cdom)} cells, built in {time.time() - t0:.0f} s", flush=True)
    fluid = cfd.Fluid()
    dpart = ibamd.to_backend(part_of(dom), ibamd.hip)
    nf, nk, nd = len(dom), len(cdom), dpart.nd
    nv = nd + 2
    dcoa, dpro = ibamd.to_backend(coa), ibamd.to_backend(pro)
    P, P2 = noisy_euler_state(nf, nd), noisy_euler_state(nf, nd, seed=7)
    R = ibamd.residual_euler_hll(dpart, P, fluid=fluid)
    S = ibamd.dual_source(P, P2, 2.0e3, -5.0e2, fluid)
    Pn, Po = noisy_euler_state(nk, nd, seed=3), noisy_euler_state(nk, nd, seed=4)
    oP, oD, out = B.colmajor_empty(nk, nv), B.colmajor_empty(nk, nv), B.colmajor_empty(nf, nv)
    pack = torch.empty(8 * nk, dtype=torch.float32, device="cuda")

    def restrict_composed():
        Pc = cfd.state2primitive(fluid, dcoa(cfd.primitive2state(fluid, P)))
        return Pc, dcoa((H(R) + H(S)).t)

    def prolong_composed():
        Q = cfd.primitive2state(fluid, P)
        dpro.diff_add(Q, cfd.primitive2state(fluid, Pn), cfd.primitive2state(fluid, Po))
        return cfd.state2primitive(fluid, Q)

    fns = {"restrict": lambda: ibamd.restrict_euler(dcoa, P, R, S, fluid, out=oP, out_D=oD),
           "restrict_composed": restrict_composed,
           "prolong": lambda: ibamd.prolong_euler(dpro, P, Pn, Po, fluid, out=out, pack=pack),
           "prolong_composed": prolong_composed}
    a, b = fns["restrict"](), fns["restrict_composed"]()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"{name}: the restriction differs from its composition"
    assert torch.equal(fns["prolong"](), fns["prolong_composed"]()), f"{name}: the prolongation differs from its composition"
    st = time_variants(fns, rounds, batch, warmup, block_seconds, torch.cuda.Stream())
    r = {"mesh": name, "fine_cells": int(nf), "coarse_cells": int(nk), "nd": nd, "rounds": rounds, "same_bits": True,
         "device": torch.cuda.get_device_name(0), "us_per_call": st}
    for k in ("restrict", "prolong"):
        r[f"{k}_composed_over_fused"] = round(st[k + "_composed"]["median_us"] / st[k]["median_us"], 3)
        r[f"{k}_fused_below_composed_outside_the_spread"] = bool(st[k]["max_us"] < st[k + "_composed"]["min_us"])
    return r


def history(name, sweeps, scale, stages=4, mach=0.5, sample=4):
    """{march: [[work units, seconds, ||R_rho||_2], ...]} of the single grid and of V-cycles on 2 and 3 levels."""
    import torch
    t0 = time.time()
    dom = ibamd.Domain(bench.build_mesh(name), hypercube_families=FAMILIES, max_partition_size=10 ** 9)
    coarse, pros, coas = ibamd.multigrid(dom, max_levels=2)
    doms = [dom] + list(coarse)
    print(f"# {name}: levels of {[len(d) for d in doms]} cells, built in {time.time() - t0:.0f} s", flush=True)
    fluid = cfd.Fluid()
    far = [1e5, 288.15, mach * float(np.sqrt(fluid.gamma * fluid.R * 288.15)), 0.0]
    free, wall = cfd.FlowBC(fluid, far), cfd.FlowBC(fluid, [far[0], far[1], 0.0], normal_flow=True)

    def bcs_of(d):
        def bcs(P):
            ibamd.impose_flow_bc(d, "farfield", free, P)
            ibamd.impose_flow_bc(d, "wall", wall, P)
        return bcs
    bcs = [bcs_of(d) for d in doms]
    dparts = [ibamd.to_backend(part_of(d), ibamd.hip) for d in doms]
    nf = len(dom)
    start = ibamd.hip(np.tile(np.float32(far), (nf, 1)))
    bcs[0](start)

    def norm(P):
        Rr = ibamd.residual_euler_hll(dparts[0], P, fluid=fluid)
        return float(torch.linalg.vector_norm(Rr[:, 0].double()).item())

    def run(step, units_per_call, calls):
        P, rows, spent = start, [[0.0, 0.0, norm(start)]], 0.0
        step(P)                                    # (workspaces and boundaries on their first use, outside the clock)
        for k in range(calls):
            torch.cuda.synchronize()
            t = time.perf_counter()
            P = step(P)
            torch.cuda.synchronize()
            spent += time.perf_counter() - t
            if (k + 1) % sample == 0 or k == calls - 1:
                rows.append([round((k + 1) * units_per_call, 3), round(spent, 5), norm(P)])
        return rows
    out = {}
    e = EulerMarch(dparts[0], fluid, scale=scale, bcs=bcs[0], local_dt=True, stages=stages)
    out["single_grid"] = run(e.step, float(stages), sweeps // stages)
    for nlev in (2, 3):
        m = MultigridMarch(dparts[:nlev], coas[:nlev - 1], pros[:nlev - 1], fluid=fluid, scale=scale, bcs=bcs[:nlev], stages=stages)
        # sweeps of one cycle, weighted by the cell count: (pre + post) stages + 1 on a level with a coarser one, its coarse
        # sweep before the forcing, n_coarsest stages on the last
        units = sum(((2 * stages + 1) if l < nlev - 1 else 2 * stages) * len(doms[l]) + (len(doms[l]) if l else 0)
                    for l in range(nlev)) / nf
        out[f"v_cycle_{nlev}_levels"] = run(m.cycle, units, sweeps // (2 * stages + 1))
    return {"mesh": name, "cells": [len(d) for d in doms], "mach": mach, "scale": scale, "stages": stages,
            "fine_sweeps": sweeps, "device": torch.cuda.get_device_name(0), "columns": ["work_units", "seconds", "norm_R_rho"],
            "history": out}


def timings_md(results, hist):
    s = ["# Multigrid for the Euler march: the fused transfers against their compositions, and residual histories", "",
         "Written by `scripts/bench_euler_mg.py` from the run recorded in `bench_euler_mg.json`; not edited by hand.",
         "Transfers: median (min - max) over the alternating rounds of one process, every variant replayed from a HIP graph.", ""]
    for r in results:
        s += [f"## `{r['mesh']}`: {r['fine_cells']} -> {r['coarse_cells']} cells, {r['nd']}-D, {r['rounds']} rounds, {r['device']}",
              "", "| variant | us per call |", "|---|---|"]
        for key, v in r["us_per_call"].items():
            s.append(f"| {LABELS[key]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) |")
        s += ["", f"* restriction: composed / fused {r['restrict_composed_over_fused']}, fused below composed outside the spread: "
              f"{r['restrict_fused_below_composed_outside_the_spread']}",
              f"* prolongation: composed / fused {r['prolong_composed_over_fused']}, fused below composed outside the spread: "
              f"{r['prolong_fused_below_composed_outside_the_spread']}", ""]
    if hist:
        s += [f"## Residual history on `{hist['mesh']}` (levels of {hist['cells']} cells), Mach {hist['mach']}, scale "
              f"{hist['scale']}, {hist['stages']} stages, {hist['fine_sweeps']} fine-level sweeps each", "",
              "`||R_rho||_2` over all rows of the fine array (ghost cells included) against work units (fine-level sweep",
              "equivalents) and wall time of eager calls.", ""]
        for key, rows in hist["history"].items():
            s += [f"### {key}", "", "| work units | seconds | norm |", "|---|---|---|"]
            s += [f"| {w} | {t} | {n:.5g} |" for w, t, n in rows]
            s.append("")
    return "\n".join(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="rae2822_0.87M,sphere3d_4.6M")
    ap.add_argument("--history-mesh", default="rae2822_0.87M")
    ap.add_argument("--history-sweeps", type=int, default=288)
    ap.add_argument("--scale", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10, help="calls captured per HIP graph")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-seconds", type=float, default=0.3, help="GPU time a timed block is sized to")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "euler_mg"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_euler_mg.py needs a GPU: nothing is measured without one")
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, "bench_euler_mg.json")
    doc = {"meshes": [], "history": None}
    if os.path.exists(path):                       # (a run of one part keeps the other parts of an earlier run)
        with open(path) as f:
            doc.update(json.load(f))

    def write():
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)
        with open(os.path.join(a.out_dir, "timings.md"), "w") as f:
            f.write(timings_md(doc["meshes"], doc["history"]))
    for name in [m for m in a.meshes.split(",") if m and m != "none"]:
        r = time_transfers(name, a.rounds, a.batch, a.warmup, a.block_seconds)
        print(json.dumps(r), flush=True)
        doc["meshes"] = [x for x in doc["meshes"] if x["mesh"] != name] + [r]
        write()
    if a.history_mesh != "none":
        doc["history"] = history(a.history_mesh, a.history_sweeps, a.scale)
        print(json.dumps(doc["history"]), flush=True)
        write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
