#!/usr/bin/env python3
"""Handle ownership against the parent commit: nothing in it is on a hot path, so no number may move.

    scripts/bench_handle_ownership.py --parent-lib <libibhip.so built at the parent commit> [--out profiles/handle_ownership/timings.md]

Both libraries run under this tree's Python layer (the parent's through ``IBHIP_LIB``), alternating parent / head:

* ``bench.py`` headline and ``--residual euler`` on the 3-D workload, three runs each; the ranges must overlap;
* ``ibh_partition_create`` on the headline mesh and ``BCSet(...)`` on its three boundaries, five runs each: one worker process
  per library builds the domain once and is then asked for a run at a time (a run: the median of 3 creates / 200 sets); the
  head's median must lie inside the parent's range or below it.

A run that fails ends the script.  Writes the table and exits 1 if a criterion is missed.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCHES = [("headline", []), ("euler 3-D", ["--workload", "sphere3d_4.6M", "--residual", "euler"])]
BENCH_ARGS = ["--gpus", "1", "--steps", "200", "--warmup", "20", "--no-cpu-baseline"]


def env_of(lib):
    e = dict(os.environ)
    e.pop("IBHIP_LIB", None)
    if lib:
        e["IBHIP_LIB"] = lib
    return e


def worker():
    """Builds the march domain of the headline workload, then answers every line on stdin with one JSON line of timings."""
    sys.path.insert(0, ROOT)
    import torch

    import bench
    import ibamd
    from ibamd import backend as B
    msh = bench.build_mesh("rae2822_0.87M")
    fam = [("farfield", [(1, False), (1, True), (2, False), (2, True)])]
    dom = ibamd.Domain(msh, max_partition_size=10 ** 9, boundaries=True, hypercube_families=fam)
    part = dom.partitions[1]
    specs = [(name, "copy" if name == "farfield" else 0.0) for name in dom.boundaries]
    took = {}
    inner = B.call

    def timed(name, *a):
        t0 = time.perf_counter()
        rc = inner(name, *a)
        took.setdefault(name, []).append(time.perf_counter() - t0)
        return rc
    B.call = timed
    B.BCSet(dom, specs)                      # the device boundaries are cached on the host ones from here on
    B.DevicePartition(part)
    torch.cuda.synchronize()
    print(json.dumps({"ready": True, "cells": int(part.spacing.shape[0]), "boundaries": len(specs)}), flush=True)
    for _ in sys.stdin:
        took.clear()
        for _ in range(3):
            B.DevicePartition(part)
        sets = []
        for _ in range(200):
            t0 = time.perf_counter()
            B.BCSet(dom, specs)
            sets.append(time.perf_counter() - t0)
        print(json.dumps({"partition_create_ms": statistics.median(took["ibh_partition_create"]) * 1e3,
                          "bcset_us": statistics.median(sets) * 1e6}), flush=True)


def run_bench(lib, extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + BENCH_ARGS + extra, env=env_of(lib), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.exit(f"bench.py {' '.join(extra)} failed with {r.returncode}:\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]


def answer(who, proc):
    """the worker's next JSON line"""
    while True:
        line = proc.stdout.readline()
        if not line:
            sys.exit(f"the {who} worker ended with {proc.wait()}")
        if line.startswith("{"):
            return json.loads(line)


def row(name, parent, head, fmt, ok):
    f = lambda v: ", ".join(fmt % x for x in v) + " (" + fmt % min(v) + " - " + fmt % max(v) + ")"
    return f"| {name} | {f(parent)} | {f(head)} | {fmt % statistics.median(head)} | {'yes' if ok else 'NO'} |"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "handle_ownership", "timings.md"))
    ap.add_argument("--title", default="Handle ownership", help="what the table's heading names: the change that is measured")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker()
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("--parent-lib: the library of the parent commit")
    libs = [("parent", os.path.abspath(args.parent_lib)), ("head", None)]
    good = True
    lines = [f"# {args.title}: timings against the parent commit", "",
             "Parent and head libraries run on the same MI355X in one session, alternating parent / head (the parent's library",
             "through `IBHIP_LIB`; the scripts and the Python layer are the head's).  Written by",
             "`scripts/bench_handle_ownership.py`.", "",
             "## `bench.py " + " ".join(BENCH_ARGS) + "`", "",
             "`ms_per_step` of three runs in run order and their range.", "",
             "| run | parent | head | head median | ranges overlap |", "|---|---|---|---|---|"]
    for name, extra in BENCHES:
        got = {"parent": [], "head": []}
        for _ in range(3):
            for who, lib in libs:
                got[who].append(run_bench(lib, extra))
                print(name, who, got[who][-1], flush=True)
        ok = max(got["parent"]) >= min(got["head"]) and max(got["head"]) >= min(got["parent"])
        good &= ok
        lines.append(row(name + (" `" + " ".join(extra) + "`" if extra else ""), got["parent"], got["head"], "%.5f", ok))
    procs = {}
    for who, lib in libs:
        procs[who] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], env=env_of(lib), cwd=ROOT,
                                      stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    ready = {}
    for who in procs:
        ready[who] = answer(who, procs[who])
        print(who, ready[who], flush=True)
    got = {who: {"partition_create_ms": [], "bcset_us": []} for who in procs}
    for _ in range(5):
        for who, _lib in libs:
            procs[who].stdin.write("go\n")
            procs[who].stdin.flush()
            run = answer(who, procs[who])
            for k, v in run.items():
                got[who][k].append(v)
            print(who, run, flush=True)
    for p in procs.values():
        p.stdin.close()
        if p.wait(timeout=60) != 0:
            sys.exit("a worker ended with an error")
    lines += ["", f"## Creation on the headline mesh ({ready['head']['cells']} cells, {ready['head']['boundaries']} boundaries)", "",
              "Five runs per library in run order and their range; a run is the median of 3 `ibh_partition_create` calls (ms, the C",
              "call alone) and of 200 `BCSet(...)` constructions (us, device boundaries already made).", "",
              "| what | parent | head | head median | inside the parent's range or below |", "|---|---|---|---|---|"]
    for key, name, fmt in (("partition_create_ms", "`ibh_partition_create` (ms)", "%.2f"), ("bcset_us", "`BCSet(...)` (us)", "%.1f")):
        ok = statistics.median(got["head"][key]) <= max(got["parent"][key])
        good &= ok
        lines.append(row(name, got["parent"][key], got["head"][key], fmt, ok))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
