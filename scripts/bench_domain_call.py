"""Time ``(dom::Domain)(f, args...)`` on the GPU: the device-resident call (``ibh_domain_gather`` / ``ibh_domain_scatter``
around the per-partition closures) against the host path (converters: gather on the host, upload, closure, download,
write-back).  One JSON line per case.

Cases: the RAE2822 mesh of 867 904 cells with ``max_partition_size`` 100 000 (the reference default, 9 partitions),
16 384, and one partition (the floor: gather and scatter of one partition plus one closure).  Closures: the advection
closure of test/advection.jl:67-83 at operator granularity (``u``, ``ud``, ``C``) and the fused ``residual_advection``.
Per-call median from device events around each call, after ``--warmup`` calls; the host path is timed the same way over
fewer calls (``--host-reps``).  ``gather_scatter_bytes``: what the two kernels move by the tables (per row and field:
a 4-B index plus 8 * nv B, read and written), against 8 TB/s for the kernel times of a separate
``rocprofv3 --kernel-trace --stats`` run (pass ``--reps`` small then).

    python scripts/bench_domain_call.py [--reps 50] [--warmup 5] [--host-reps 5] [--out profiles/domain_call/x.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import ibamd  # noqa: E402
from ibamd.domain import domain_plan_tables  # noqa: E402

PEAK = 8.0e12


def adv_closure(part, u, ud, Cl):
    import torch
    D = ibamd.JST_sensor(part, u)
    for dim in range(1, part.ndims + 1):
        Cf = ibamd.at_faces(part, Cl[:, dim - 1].contiguous(), dim)
        gu = ibamd.cell_gradient(part, u, dim)
        uL, uR = ibamd.MUSCL(part, u, gu, dim, D=D, high_order=True)
        ud -= ibamd.green_gauss(part, (uL + uR) * Cf / 2 + torch.abs(Cf) * (uL - uR) / 2, dim)


def fused_closure(part, u, ud, Cl):
    ibamd.residual_advection(part, u, Cl, out=ud)


CLOSURES = {"operators": adv_closure, "fused": fused_closure}


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def table_bytes(dom, nvs):
    T = domain_plan_tables(dom)
    rows, imgs = int(T["rows"].size), int(T["image"].size)
    per_field = [(rows * (4 + 8 * nv), imgs * (8 + 8 * nv)) for nv in nvs]   # gather: index + read + write; scatter: pair
    return sum(g for g, _ in per_field), sum(s for _, s in per_field)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--sizes", default="100000,16384,1000000000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    out = open(a.out, "a") if a.out else None
    msh = bench.build_mesh("rae2822_0.87M")
    for mps in [int(s) for s in a.sizes.split(",")]:
        dom = ibamd.Domain(msh, max_partition_size=mps, boundaries=False)
        n = len(dom)
        u_h, C_h = bench.synthetic_fields(dom.global_centers())
        u, C = ibamd.hip(u_h), ibamd.hip(C_h)
        ud = ibamd.colmajor_empty(n)
        gb, sb = table_bytes(dom, [1, 1, 2])
        for name, f in CLOSURES.items():
            dev = timed(lambda: dom(f, u, ud, C), a.reps, a.warmup)
            uh, udh = u_h.copy(), np.zeros(n, np.float32)
            host = timed(lambda: dom(f, uh, udh, C_h, conv_to_backend=ibamd.hip, conv_from_backend=ibamd.to_host),
                         a.host_reps, 1)
            rec = {"case": "domain_call", "cells": n, "max_partition_size": mps, "partitions": len(dom.partitions),
                   "closure": name, "us_device_call": round(dev, 1), "us_host_call": round(host, 1),
                   "speedup": round(host / dev, 2), "gather_bytes": gb, "scatter_bytes": sb,
                   "gather_scatter_us_at_8TBs": round((gb + sb) / PEAK * 1e6, 2), "reps": a.reps}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
        del dom
        torch.cuda.synchronize()
    if out:
        out.close()


if __name__ == "__main__":
    main()
