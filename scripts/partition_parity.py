#!/usr/bin/env python3
"""What ``ibh_partition_create`` reports and allocates, this build against another build of libibhip.so.

    scripts/partition_parity.py --parent-lib <libibhip.so of the parent commit> [--out profiles/partition_build/info_parity.md]

Builds the partitions once -- the two test fixtures (advection in 3, RAE2822 in 3), the headline bench mesh and the
sphere3d_4.6M workload, whole and split in two -- then forks one process per library (the GPU is first touched in the
children).  Each creates every partition and records the ``IBH_INFO_COUNT`` values of ``ibh_partition_info`` and what the
create added to ``ibh_owned_device_memory`` (bytes, buffers).  Writes the table; exits 1 unless every row is identical.
"""
import argparse
import multiprocessing as mp
import os
import queue
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def partitions(small):
    import bench
    import ibamd
    from conftest import ADV_FAMILIES, RAE_FAMILIES, advection_mesh, rae_mesh
    out = {}
    for name, dom in (("advection", ibamd.Domain(advection_mesh(), hypercube_families=ADV_FAMILIES, max_partition_size=4096)),
                      ("rae2822", ibamd.Domain(rae_mesh(), hypercube_families=RAE_FAMILIES, max_partition_size=16384))):
        for k, p in dom.partitions.items():
            out[f"{name} fixture, partition {k}"] = p
    if small:
        return out
    for wl, worlds in (("rae2822_0.87M", (1,)), ("sphere3d_4.6M", (1, 2))):
        msh = bench.build_mesh(wl)
        npb = msh.block_size ** msh.ndims
        for world in worlds:   # bench.py's block-aligned split over `world` ranks
            mps = -(-(-(-len(msh) // world)) // npb) * npb
            dom = ibamd.Domain(msh, max_partition_size=mps, boundaries=False)
            for k, p in dom.partitions.items():
                out[f"{wl}, partition {k} of {world}"] = p
    return out


def child(lib, parts, q):
    import ctypes as C
    import gc
    from ibamd import _lib
    assert _lib._lib is None
    if lib:
        _lib.LIB_PATH = os.environ["IBHIP_LIB"] = lib
    from ibamd import backend as B
    rows = {}
    for name, part in parts.items():
        gc.collect()
        base = B.owned_device_memory()
        dp = B.DevicePartition(part)
        now = B.owned_device_memory()
        info = (C.c_int64 * _lib.INFO_COUNT)()
        _lib.call("ibh_partition_info", dp.handle, info, _lib.INFO_COUNT)
        rows[name] = (list(info), now[0] - base[0], now[1] - base[1], int(dp.nd), int(dp.nc))
        del dp
    q.put(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partition_build", "info_parity.md"))
    ap.add_argument("--small", action="store_true", help="the two fixtures only")
    args = ap.parse_args()
    from ibamd import _lib
    parts = partitions(args.small)
    ctx, got = mp.get_context("fork"), {}
    for who, lib in (("parent", os.path.abspath(args.parent_lib)), ("head", None)):
        q = ctx.Queue()
        p = ctx.Process(target=child, args=(lib, parts, q))
        p.start()
        while who not in got:   # a child that dies is reported at once, not after the queue's timeout
            try:
                got[who] = q.get(timeout=1)
            except queue.Empty:
                if not p.is_alive():
                    sys.exit(f"the {who} process ended with {p.exitcode} before it reported")
        p.join(60)
        if p.exitcode != 0:
            sys.exit(f"the {who} process ended with {p.exitcode}")
    lines = ["# Partition create: info and device memory against the parent commit", "",
             "`ibh_partition_info` (all `IBH_INFO_COUNT` slots) and what one `ibh_partition_create` adds to `ibh_owned_device_memory`, the parent's",
             "library against this one, one process each on the same partitions.  Written by `scripts/partition_parity.py`.", "",
             "| partition | nd | cells | info (the named slots; the rest are zero) | bytes | buffers | identical |", "|---|---|---|---|---|---|---|"]
    good = True
    for name in parts:
        a, b = got["parent"][name], got["head"][name]
        same = a == b and not any(b[0][len(_lib.INFO_SLOTS):])
        good &= same
        lines.append(f"| {name} | {b[3]} | {b[4]} | {' '.join(map(str, b[0][:len(_lib.INFO_SLOTS)]))} | {b[1]} | {b[2]} | "
                     + ("yes" if same else f"NO: parent {a}") + " |")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
