"""Time the cell-role entries of the Euler march on the GPU (``restrict_euler(roles=...)``, ``forcing_roles``, ``sumsq_roles``,
the blank of ``EulerMarch(roles=...)``) against what they replace, and write down the residual history of ``MultigridMarch``
with and without roles against the single-grid march: one JSON line per measurement, and two files under profiles/.

Per mesh (``--meshes``, ``bench.build_mesh``, one partition, the operators of ``multigrid(dom, max_levels=1)``; state: Mach 0.3
with 5 % noise, seeded; ``R`` one sweep of it, ``S`` a BDF2 source), per call:
  (a) ``restrict``:                ``restrict_euler`` without roles, the entry the parent has -- one launch;
  (b) ``restrict_roles``:          ``restrict_euler(roles=...)`` -- one launch, one byte more per fine row;
  (c) ``restrict_roles_composed``: the select as one broadcast, ``ifelse(roles == 0, R .+ S, 0)``, then (a) on it with ``S = None``;
  (d) ``forcing_roles``:           ``forcing_roles`` on the coarse level -- one launch, in place;
  (e) ``forcing_composed``:        the broadcast ``D .-= R`` in place, then the select as a second broadcast;
  (f) ``sumsq_roles``:             ``sumsq_roles`` of the ``nd + 2`` columns -- one launch and the final stage;
  (g) ``sumsq_per_column``:        ``ibh_sumsq`` once per column (all rows: the parent has no masked sum);
  (h) ``stage``:                   ``stage_euler`` alone;
  (i) ``stage_blank``:             ``stage_euler`` and the blank of the solid rows (``Roles.blank``: one ``ibh_scatter_rows``).
(b) and (c), (d) and (e) give the same bits (checked here before anything is timed).  Roles: ``cell_roles`` of the domain where
it has boundaries (the 2-D meshes, built with their far field); on the sphere meshes, whose ghost cells take minutes to
project on the host, roles by the distance of a centre from the origin -- solid inside 0.9 radii, ghost up to 1.1 -- which
cost the kernels what real ones do.  How a figure is taken: scripts/graph_timing.py -- HIP graphs of ``--batch`` calls replayed
between device events, the variants alternating over ``--rounds`` rounds in one process; median (min - max).

History (``--history-mesh``, far field and slip wall on every level, Mach 0.5 at zero incidence from the free stream, ``stages=4``,
``scale`` 0.3 -- the settings of DESIGN.md's multigrid paragraph): the single grid and V-cycles on 3 levels, each without and with
roles, for ``--history-sweeps`` fine-level sweeps; ``||R_rho||_2`` over ALL rows and over the FLUID rows every few steps.
Written down, not asserted.  Needs a GPU; there is no CPU path.

    python scripts/bench_euler_roles.py [--meshes rae2822_0.87M,sphere3d_4.6M] [--history-mesh rae2822_0.87M | none]
                                        [--history-sweeps 288] [--scale 0.3] [--rounds 5] [--out-dir profiles/euler_roles]
"""
import argparse
import ctypes as C
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
from ibamd import cfd, hiparray, solver  # noqa: E402
from ibamd import backend as B  # noqa: E402
from ibamd.hiparray import HipArray as H  # noqa: E402
from ibamd.solver import EulerMarch, MultigridMarch  # noqa: E402

LABELS = {"restrict": "(a) `restrict_euler`", "restrict_roles": "(b) `restrict_euler(roles=...)`",
          "restrict_roles_composed": "(c) select broadcast + `restrict_euler`", "forcing_roles": "(d) `forcing_roles`",
          "forcing_composed": "(e) `D .-= R`, then the select", "sumsq_roles": "(f) `sumsq_roles`",
          "sumsq_per_column": "(g) `ibh_sumsq` per column", "stage": "(h) `stage_euler`",
          "stage_blank": "(i) `stage_euler` + blank"}
PAIRS = (("restrict_roles", "restrict_roles_composed"), ("forcing_roles", "forcing_composed"), ("sumsq_roles", "sumsq_per_column"))
FAMILIES = [("farfield", [(1, False), (1, True), (2, False), (2, True)])]


def part_of(dom):
    return next(iter(dom.partitions.values()))


def roles_of(dom, real):
    """``cell_roles`` of the domain (``real``), or roles by the distance from the origin: the sphere meshes."""
    if real:
        return ibamd.cell_roles(dom)
    r = np.linalg.norm(dom.global_centers(), axis=1)
    return np.where(r < 0.9, 2, np.where(r < 1.1, 1, 0)).astype(np.uint8)


def time_mesh(name, rounds, batch, warmup, block_seconds):
    import torch
    t0 = time.time()
    two_d = not name.startswith("sphere3d")
    dom = ibamd.Domain(bench.build_mesh(name), max_partition_size=10 ** 9, boundaries=two_d,
                       hypercube_families=FAMILIES if two_d else ())
    (cdom,), (pro,), (coa,) = ibamd.multigrid(dom, max_levels=1)
    hr, hrc = roles_of(dom, two_d), roles_of(cdom, two_d)
    print(f"# {name}: {len(dom)} -> {len(cdom)} cells, roles (fluid, ghost, solid) {np.bincount(hr, minlength=3).tolist()} -> "
          f"{np.bincount(hrc, minlength=3).tolist()}, built in {time.time() - t0:.0f} s", flush=True)
    fluid = cfd.Fluid()
    dpart = ibamd.to_backend(part_of(dom), ibamd.hip)
    nf, nk, nd = len(dom), len(cdom), dpart.nd
    nv = nd + 2
    dcoa = ibamd.to_backend(coa)
    P, P2 = noisy_euler_state(nf, nd), noisy_euler_state(nf, nd, seed=7)
    far = [1e5, 288.15] + [100.0] * nd
    roles, roles_c = ibamd.Roles(part_of(dom), hr, far), ibamd.Roles(part_of(cdom), hrc, far)
    R = ibamd.residual_euler_hll(dpart, P, fluid=fluid)
    S = ibamd.dual_source(P, P2, 2.0e3, -5.0e2, fluid)
    # the roles as Float32 arrays of the fields' shapes: the operand of the composed select (outside the clock)
    rf = ibamd.hip(np.repeat(hr.astype(np.float32)[:, None], nv, axis=1))
    rc = ibamd.hip(np.repeat(hrc.astype(np.float32)[:, None], nv, axis=1))
    oP, oD, oP2, oD2 = (B.colmajor_empty(nk, nv) for _ in range(4))
    Rc = ibamd.hip(np.random.default_rng(5).normal(size=(nk, nv)).astype(np.float32))
    D0 = ibamd.hip(np.random.default_rng(6).normal(size=(nk, nv)).astype(np.float32))
    D1, D2 = D0.clone(), D0.clone()
    sums = torch.zeros(nv, dtype=torch.float64, device="cuda")
    cols = torch.zeros(nv, dtype=torch.float64, device="cuda")
    dt = ibamd.timestep_euler(dpart, P, fluid, 0.3)
    out, work = B.colmajor_empty(nf, nv), B.colmajor_empty(nf, nv)

    def select(X, r):
        return hiparray.ifelse(hiparray.eq(H(r), 0.0), X, 0.0).t

    def restrict_roles_composed():
        return ibamd.restrict_euler(dcoa, P, select(H(R) + H(S), rf), None, fluid, out=oP2, out_D=oD2)

    def forcing_composed():
        solver._sub_into(D2, Rc)
        return select(H(D2), rc)

    def sumsq_per_column():
        B._stream()
        for v in range(nv):
            B.call("ibh_sumsq", nf, C.c_void_p(R.data_ptr() + 4 * v * R.stride(1)), C.c_void_p(cols.data_ptr() + 8 * v))
        return cols

    def stage():
        return ibamd.stage_euler(dpart, P, P, dt, 0.5, out, fluid, "hll", work=work)

    fns = {"restrict": lambda: ibamd.restrict_euler(dcoa, P, R, S, fluid, out=oP, out_D=oD),
           "restrict_roles": lambda: ibamd.restrict_euler(dcoa, P, R, S, fluid, out=oP, out_D=oD, roles=roles),
           "restrict_roles_composed": restrict_roles_composed,
           "forcing_roles": lambda: ibamd.forcing_roles(D1, Rc, roles_c),
           "forcing_composed": forcing_composed,
           "sumsq_roles": lambda: ibamd.sumsq_roles(R, roles, out=sums),
           "sumsq_per_column": sumsq_per_column,
           "stage": stage,
           "stage_blank": lambda: roles.blank(stage())}
    a, b = fns["restrict_roles"](), fns["restrict_roles_composed"]()
    assert torch.equal(oP, oP2) and torch.equal(oD, oD2), f"{name}: the roles restriction differs from its composition"
    assert torch.equal(fns["forcing_roles"](), fns["forcing_composed"]()), f"{name}: the forcing differs from its composition"
    D1.copy_(D0)
    D2.copy_(D0)
    st = time_variants(fns, rounds, batch, warmup, block_seconds, torch.cuda.Stream())
    r = {"mesh": name, "fine_cells": int(nf), "coarse_cells": int(nk), "nd": nd, "rounds": rounds, "same_bits": True,
         "roles_fine": np.bincount(hr, minlength=3).tolist(), "roles_coarse": np.bincount(hrc, minlength=3).tolist(),
         "device": torch.cuda.get_device_name(0), "us_per_call": st}
    for k, c in PAIRS:
        r[f"{k}_composed_over_fused"] = round(st[c]["median_us"] / st[k]["median_us"], 3)
        r[f"{k}_below_composed_outside_the_spread"] = bool(st[k]["max_us"] < st[c]["min_us"])
    r["restrict_roles_over_restrict"] = round(st["restrict_roles"]["median_us"] / st["restrict"]["median_us"], 3)
    r["restrict_roles_extra_us"] = round(st["restrict_roles"]["median_us"] - st["restrict"]["median_us"], 2)
    r["restrict_roles_extra_bytes"] = int(nf)                    # one byte per fine row
    r["blank_us_per_stage"] = round(st["stage_blank"]["median_us"] - st["stage"]["median_us"], 2)
    return r


def history(name, sweeps, scale, stages=4, mach=0.5, sample=4):
    """{march: [[work units, ||R_rho||_2 over all rows, over the fluid rows], ...]}."""
    import torch
    t0 = time.time()
    dom = ibamd.Domain(bench.build_mesh(name), hypercube_families=FAMILIES, max_partition_size=10 ** 9)
    coarse, pros, coas = ibamd.multigrid(dom, max_levels=2)
    doms = [dom] + list(coarse)
    host_roles = [ibamd.cell_roles(d) for d in doms]
    counts = [np.bincount(r, minlength=3).tolist() for r in host_roles]
    print(f"# {name}: levels of {[len(d) for d in doms]} cells, roles {counts}, built in {time.time() - t0:.0f} s", flush=True)
    fluid = cfd.Fluid()
    far = [1e5, 288.15, mach * float(np.sqrt(fluid.gamma * fluid.R * 288.15)), 0.0]
    free, wall = cfd.FlowBC(fluid, far), cfd.FlowBC(fluid, [far[0], far[1], 0.0], normal_flow=True)

    def bcs_of(d):
        def bcs(P):
            ibamd.impose_flow_bc(d, "farfield", free, P)
            ibamd.impose_flow_bc(d, "wall", wall, P)
        return bcs
    bcs = [bcs_of(d) for d in doms]
    parts = [part_of(d) for d in doms]
    dparts = [ibamd.to_backend(p, ibamd.hip) for p in parts]
    roles = [ibamd.Roles(p, r, far) for p, r in zip(parts, host_roles)]
    nf = len(dom)
    start = ibamd.hip(np.tile(np.float32(far), (nf, 1)))
    bcs[0](start)
    everything = torch.zeros(nf, dtype=torch.uint8, device="cuda")

    def norms(P):
        Rr = ibamd.residual_euler_hll(dparts[0], P, fluid=fluid)
        return [float(ibamd.sumsq_roles(Rr, r)[0].item()) ** 0.5 for r in (everything, roles[0])]

    def run(step, units_per_call, calls):
        P, rows = start, [[0.0] + norms(start)]
        for k in range(calls):
            P = step(P)
            if (k + 1) % sample == 0 or k == calls - 1:
                rows.append([round((k + 1) * units_per_call, 3)] + norms(P))
        return rows
    out = {}
    kw = dict(scale=scale, local_dt=True, stages=stages)
    out["single_grid"] = run(EulerMarch(dparts[0], fluid, bcs=bcs[0], **kw).step, float(stages), sweeps // stages)
    print("# single grid done", flush=True)
    out["single_grid_roles"] = run(EulerMarch(dparts[0], fluid, bcs=bcs[0], roles=roles[0], **kw).step, float(stages),
                                   sweeps // stages)
    units = sum(((2 * stages + 1) if l < 2 else 2 * stages) * len(doms[l]) + (len(doms[l]) if l else 0) for l in range(3)) / nf
    for key, rl in (("v_cycle_3_levels", None), ("v_cycle_3_levels_roles", roles)):
        m = MultigridMarch(dparts, coas, pros, fluid=fluid, scale=scale, bcs=bcs, stages=stages, roles=rl)
        out[key] = run(m.cycle, units, sweeps // (2 * stages + 1))
        print(f"# {key} done", flush=True)
    return {"mesh": name, "cells": [len(d) for d in doms], "roles": counts, "mach": mach, "scale": scale, "stages": stages,
            "fine_sweeps": sweeps, "device": torch.cuda.get_device_name(0),
            "columns": ["work_units", "norm_R_rho_all_rows", "norm_R_rho_fluid_rows"], "history": out}


def timings_md(results, hist):
    s = ["# Cell roles in the Euler march: the role entries against what they replace, and residual histories", "",
         "Written by `scripts/bench_euler_roles.py` from the run recorded in `bench_euler_roles.json`; not edited by hand.",
         "Median (min - max) over the alternating rounds of one process, every variant replayed from a HIP graph.", ""]
    for r in results:
        s += [f"## `{r['mesh']}`: {r['fine_cells']} -> {r['coarse_cells']} cells, {r['nd']}-D, {r['rounds']} rounds, {r['device']}",
              "", f"Roles (fluid, ghost, solid): fine {r['roles_fine']}, coarse {r['roles_coarse']}.", "",
              "| variant | us per call |", "|---|---|"]
        for key, v in r["us_per_call"].items():
            s.append(f"| {LABELS[key]} | {v['median_us']} ({v['min_us']} - {v['max_us']}) |")
        s.append("")
        for k, c in PAIRS:
            s.append(f"* `{k}`: composed / fused {r[f'{k}_composed_over_fused']}, fused below composed outside the spread: "
                     f"{r[f'{k}_below_composed_outside_the_spread']}")
        s += [f"* the roles restriction over the unmasked entry: x {r['restrict_roles_over_restrict']}, "
              f"{r['restrict_roles_extra_us']} us for {r['restrict_roles_extra_bytes']} bytes of roles",
              f"* the blank: {r['blank_us_per_stage']} us per stage over `stage_euler` alone", ""]
    if hist:
        s += [f"## Residual history on `{hist['mesh']}` (levels of {hist['cells']} cells, roles {hist['roles']}), Mach "
              f"{hist['mach']}, scale {hist['scale']}, {hist['stages']} stages, {hist['fine_sweeps']} fine-level sweeps each", "",
              "`||R_rho||_2` of the fine array over all rows (ghost and solid cells included) and over the fluid rows, against",
              "work units (fine-level sweep equivalents).", ""]
        for key, rows in hist["history"].items():
            s += [f"### {key}", "", "| work units | all rows | fluid rows |", "|---|---|---|"]
            s += [f"| {w} | {a:.5g} | {f:.5g} |" for w, a, f in rows]
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
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "euler_roles"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_euler_roles.py needs a GPU: nothing is measured without one")
    os.makedirs(a.out_dir, exist_ok=True)
    path = os.path.join(a.out_dir, "bench_euler_roles.json")
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
        r = time_mesh(name, a.rounds, a.batch, a.warmup, a.block_seconds)
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
