"""What the ``bench_*.py`` timing scripts share: how a figure is taken, the seeded state and the command line of the Euler
scripts.  ``bench.py`` at the repository's root does not use it.

How a figure is taken: after ``warmup`` eager calls a variant is captured into a HIP graph of ``batch`` calls on a side stream
(``Launcher``); a timed block is that graph replayed back to back between two device events, as often as a first short block
says is needed to fill ``block_seconds``.  The variants alternate: ``rounds`` rounds, one block of each in every round; the
figure is the median over the rounds with the spread (min, max) (``time_variants``).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
import ibamd  # noqa: E402


class Launcher:
    """``calls`` calls of one variant captured in a HIP graph; ``block_us(runs)`` replays it ``runs`` times."""

    def __init__(self, f, calls, warmup, stream):
        import torch
        self.stream, self.calls = stream, calls
        with torch.cuda.stream(stream):
            for _ in range(warmup):
                f()
        stream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=stream):
            for _ in range(calls):
                self.keep = f()
        torch.cuda.synchronize()
        self.block_us(1)

    def block_us(self, runs):
        import torch
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            t0.record()
            for _ in range(runs):
                self.graph.replay()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / (runs * self.calls)


def time_variants(fns, rounds, batch, warmup, block_seconds, side):
    """{key: {median_us, min_us, max_us, calls_per_block}} of the variants ``fns`` on the side stream ``side``."""
    launchers, runs = {}, {}
    for key, f in fns.items():
        L = launchers[key] = Launcher(f, batch, warmup, side)
        L.block_us(3)
        first = L.block_us(5) * L.calls * 1e-6
        runs[key] = max(3, int(block_seconds / max(first, 1e-7)) + 1)
    times = {key: [] for key in launchers}
    for _ in range(rounds):
        for key, L in launchers.items():
            times[key].append(L.block_us(runs[key]))
    return {key: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                  "calls_per_block": runs[key] * launchers[key].calls} for key, v in times.items()}


def noisy_euler_state(nc, nd, seed=12345):
    """P = [p T u v (w)] on the device: Mach 0.3, 5 % noise on p and T, 10 % on the velocities, seeded."""
    rng = np.random.default_rng(seed)
    Ph = np.empty((nc, nd + 2), np.float32)
    Ph[:, 0] = 1e5 * (1 + 0.05 * rng.uniform(-1, 1, nc))
    Ph[:, 1] = 288.15 * (1 + 0.05 * rng.uniform(-1, 1, nc))
    for d in range(nd):
        Ph[:, 2 + d] = 100.0 * (1 + 0.1 * rng.uniform(-1, 1, nc))
    return ibamd.hip(Ph)


def single_partition(name):
    """(domain, its one partition) of ``bench.build_mesh(name)``, without boundaries."""
    dom = ibamd.Domain(bench.build_mesh(name), max_partition_size=10 ** 9, boundaries=False)
    return dom, next(iter(dom.partitions.values()))


def one_launch(dpart):
    """Whether the 2-D single-kernel sweep takes the whole partition: a step or stage on it is one launch."""
    i = dpart.info
    return dpart.nd == 2 and i["fusable_blocks"] == i["full_blocks"] > 0 and i["irregular_cells"] == 0


def run_meshes(argv, default_out_dir, json_name, time_mesh, timings_md, batch_help="stages captured per HIP graph"):
    """The ``main()`` of an Euler timing script: per mesh of ``--meshes`` one call
    ``time_mesh(name, part, scheme, rounds, batch, warmup, block_seconds)``, its result printed as one JSON line, and
    ``json_name`` (``{"meshes": results}``) and ``timings.md`` (``timings_md(results)``) rewritten in ``--out-dir``."""
    script = os.path.splitext(json_name)[0] + ".py"
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="rae2822_0.87M,sphere3d_4.6M")
    ap.add_argument("--scheme", default="hll", choices=["hll", "sensor"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10, help=batch_help)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-seconds", type=float, default=0.3, help="GPU time a timed block is sized to")
    ap.add_argument("--out-dir", default=default_out_dir)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{script} needs a GPU: nothing is measured without one")
    os.makedirs(a.out_dir, exist_ok=True)
    results = []
    for name in a.meshes.split(","):
        t0 = time.time()
        dom, part = single_partition(name)
        print(f"# {name}: {len(dom)} cells, built in {time.time() - t0:.0f} s", flush=True)
        r = time_mesh(name, part, a.scheme, a.rounds, a.batch, a.warmup, a.block_seconds)
        print(json.dumps(r), flush=True)
        results.append(r)
        with open(os.path.join(a.out_dir, json_name), "w") as f:
            json.dump({"meshes": results}, f, indent=1)
        with open(os.path.join(a.out_dir, "timings.md"), "w") as f:
            f.write(timings_md(results))
        del dom, part
    return 0
