"""Time ``TimeAverage.push`` (``ibh_time_average_push``) on the GPU: one JSON line per case.

Cases: 0.87 M x 1 and 7.9 M x 5 cells x variables; dt a host scalar or elementwise; eta in Float32 or Float64; stores
plain, non-temporal, or "auto", non-temporal past the Infinity Cache only (the default; ``ibh_set_tuning(
"time_average_nt", 0 / 1 / -1)``).  Time per push from device events around ``--reps`` back-to-back pushes (after
``--warmup``); bytes = 20 per element (read mu, sigma, Q; write mu, sigma), 24 with an elementwise dt; HBM fraction
against 8 TB/s.  Under ``rocprofv3 --kernel-trace --stats`` the same run gives the kernel time (pass ``--reps`` small to
keep the trace short).

    python scripts/bench_time_average.py [--reps 200] [--warmup 20] [--cases all|small|big]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ibamd  # noqa: E402
from ibamd import _lib, cfd  # noqa: E402

PEAK = 8.0e12
SIZES = {"small": (870_000, 1), "big": (7_900_000, 5)}


def run_case(n, nv, dt_form, prec, nt, reps, warmup):
    import torch
    _lib.call("ibh_set_tuning", b"time_average_nt", {"plain": 0, "nt": 1, "auto": -1}[nt])
    g = torch.Generator(device="cuda").manual_seed(1)
    shape = (n,) if nv == 1 else (nv, n)
    Q = torch.randn(shape, device="cuda", generator=g)
    Q = Q if nv == 1 else Q.T
    tau = np.float32(0.5) if prec == "Float32" else 0.5
    dt = np.float32(1e-3) if dt_form == "host" else torch.full_like(Q, 1e-3)
    avg = cfd.TimeAverage(tau)
    avg.push(Q)
    for _ in range(warmup):
        avg.push(Q, dt)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        avg.push(Q, dt)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) * 1e3 / reps
    nbytes = n * nv * (24 if dt_form == "element" else 20)
    return {"case": "time_average_push", "n": n, "nv": nv, "dt": dt_form, "precision": prec, "stores": nt,
            "us_per_push": round(us, 3), "bytes": nbytes, "TB_s": round(nbytes / us / 1e6, 3),
            "hbm_fraction_8TBs": round(nbytes / (us * 1e-6) / PEAK, 3), "reps": reps,
            "finite": bool(torch.isfinite(avg.sigma).all().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cases", default="all", choices=["all", "small", "big"])
    a = ap.parse_args()
    sizes = list(SIZES.values()) if a.cases == "all" else [SIZES[a.cases]]
    for n, nv in sizes:
        for dt_form in ("host", "element"):
            for prec in ("Float32", "Float64"):
                for nt in ("plain", "nt", "auto"):
                    print(json.dumps(run_case(n, nv, dt_form, prec, nt, a.reps, a.warmup)), flush=True)
    _lib.call("ibh_set_tuning", b"time_average_nt", -1)


if __name__ == "__main__":
    main()
