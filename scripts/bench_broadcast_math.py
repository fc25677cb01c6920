"""Generic broadcast forms of the reference's formulas on the widened device broadcast (ibh_ew_eval's extended
interpreter) against the dedicated kernels, at one size.  Run on the GPU box:
    python scripts/bench_broadcast_math.py [cells]
One JSON line per case: time per call (CUDA events over 50 calls after 5 warm-up calls), the bytes the call must move
(inputs + output, 4 B per element) and the fraction of an 8 TB/s HBM floor for those bytes."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ibamd  # noqa: E402
from ibamd import cfd  # noqa: E402
from ibamd import hiparray as H  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 7917568
f32 = np.float32
A = H.HipArray
rng = np.random.default_rng(0)
fl = cfd.Fluid()
g, R, mu, Tr, S = (f32(v) for v in (fl.gamma, fl.R, fl.mu_ref, fl.Tref, fl.S))
T = A(rng.uniform(5, 2000, n).astype(f32))
Tt = T.t
un, M, p = (A(rng.uniform(lo, hi, n).astype(f32)) for lo, hi in ((-1, 1), (0.2, 2.0), (0.5e5, 2e5)))
yp = A(rng.uniform(0.5, 1e4, n).astype(f32))
Rey = A(rng.uniform(1.0, 1e8, n).astype(f32))
p_inf, T_inf, kap, C, om = f32(1e5), f32(288.0), f32(0.41), f32(4.9), f32(0.5)
out = A(np.zeros(n, f32))


def dynamic_viscosity_fused():
    # the same tree evaluated straight into `out` (no copy): clamp twice, as `@.` inlines the let-bound T
    Tc = H.clamp(T, 10.0, float("inf"))
    e = mu * (Tc / Tr) ** (f32(2.0) / 3) * (Tr + S) / (Tc + S)
    e._evaluate_into(out.t)


def dynamic_viscosity_dedicated():
    cfd.dynamic_viscosity(fl, Tt)


def flowbc_pb():
    e = (un >= 0.0) * ((M > 1.0) * p_inf + (M <= 1.0) * p) + (un < 0.0) * ((M > 1.0) * p + (M <= 1.0) * p_inf)
    e._evaluate_into(out.t)


def flowbc_Tb():
    e = (un > 0.0) * T_inf + (un <= 0.0) * T
    e._evaluate_into(out.t)


def wall_function_step():
    # one step of wall_function(Rey)'s fixed point: von_Karman (turbulence.jl:16) and the relaxation
    up = (H.log(yp.maximum_with(1.0)) / kap + C).minimum_with(yp)
    e = om * (Rey / up) + (f32(1) - om) * yp
    e._evaluate_into(out.t)


cases = [("dynamic_viscosity_generic_fused", dynamic_viscosity_fused, 2),
         ("dynamic_viscosity_dedicated", dynamic_viscosity_dedicated, 2),
         ("flowbc_pb", flowbc_pb, 4), ("flowbc_Tb", flowbc_Tb, 3), ("von_Karman_step", wall_function_step, 3)]
for name, f, words in cases:
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        f()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 50
    floor_us = n * 4 * words / 8e12 * 1e6
    print(json.dumps({"case": name, "cells": n, "us": round(us, 1), "bytes_per_cell": 4 * words,
                      "hbm_floor_us": round(floor_us, 1), "fraction_of_floor": round(floor_us / us, 3),
                      "floor_8B_us": round(n * 8 / 8e12 * 1e6, 1)}), flush=True)
