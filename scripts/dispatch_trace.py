"""What the fused-sweep dispatch of csrc/ibh_fused.hip (kernels and launchers: csrc/ibh_fused2d.hip, ibh_fused3d.hip,
ibh_fused_general.hip, the block closures of ibh_turb.hip) launches and computes, for comparing two builds of libibhip.so.

    IBHIP_LIB=<build> python scripts/dispatch_trace.py --out run.json
        runs every sweep entry point on five kinds of partition (2-D single, 2-D with skirt fragments, 3-D all-block, 3-D
        with skirt fragments, no block structure) over the cross product of flag combinations and tuning values, and records
        per case the return code, the message (without its file:line) and a hash of the bits of every output array.
        Cases the library rejects are recorded, not skipped.
    python scripts/dispatch_trace.py --reduce <rocprofv3 output dir> launches.txt.gz
        reduces the kernel trace of such a run (rocprofv3 --kernel-trace --output-format csv -d <dir> -- python ...) to the
        ordered list of (kernel, grid, workgroup) of the library's own kernels.
    python scripts/dispatch_trace.py --compare A.json B.json A.txt.gz B.txt.gz
        exits 0 when the two runs agree in every return code, message, hash and launch.

Two builds that differ only in host code must agree exactly: same kernels, same launch shapes, same bits.
"""
import argparse
import csv
import glob
import gzip
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VARIANTS = (0, 4, 512)
TUNING = dict(quad_parts=(3, 1, 2), rows=(0, 1), rows_singles=(-1, 0, 1, 2), pairs=(1, 0), arith_ids=(1, 0))
DEFAULTS = dict(quad_variant=0, quad_parts=3, rows=0, rows_singles=-1, pairs=1, arith_ids=1)


def partitions():
    import copy
    import numpy as np
    import bench
    import ibamd
    from conftest import ADV_FAMILIES, RAE_FAMILIES, advection_mesh, rae_mesh
    from ibamd.mesher import Ball, Mesh
    f32 = np.float32
    out = {}
    dom = ibamd.Domain(advection_mesh(2e-2), hypercube_families=ADV_FAMILIES, max_partition_size=10 ** 9, boundaries=False)
    (out["2d_single"],) = dom.partitions.values()
    dom = ibamd.Domain(rae_mesh(2e-2, 1e-2), hypercube_families=RAE_FAMILIES, max_partition_size=6144, boundaries=False)
    out["2d_skirt"] = dom.partitions[sorted(dom.partitions)[1]]
    msh = Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8, refinement_regions=[(Ball(np.array([-2.0, -2.0, -2.0]), 0.1), f32(0.1))])
    (out["3d_blocks"],) = ibamd.Domain(msh, max_partition_size=10 ** 9, boundaries=False).partitions.values()
    msh = Mesh(f32([-4, -4, -4]), f32([8, 8, 8]), ("sphere", bench.icosphere(subdiv=2), f32(0.2)), block_size=8)
    msh.distance_fields = {}
    mps = -(-(-(-len(msh) // 4)) // 512) * 512
    out["3d_skirt"] = ibamd.Domain(msh, max_partition_size=mps, boundaries=False, only=[1]).partitions[1]
    plain = copy.copy(out["2d_skirt"])
    plain.block_size = 0   # the library is given no block size: face-list kernels everywhere
    out["no_blocks"] = plain
    return out


def run(path):
    import ctypes as C
    import numpy as np
    import torch
    import ibamd
    from conftest import euler_field, seeded_field
    from ibamd import _lib
    backend = sys.modules[ibamd.residual_advection.__module__]
    lib = _lib.load()
    F = {k: getattr(ibamd, "IBH_" + k) for k in ("NO_FUSE", "NO_QUAD", "IMAGE_ONLY", "PHASE_INTERIOR", "PHASE_BOUNDARY",
                                                 "PASS_A_ONLY", "PASS_B_ONLY", "EXACT", "FORCE_GENERAL", "FORCE_MIXED",
                                                 "SWEEP_ONLY")}
    PH1, PH2 = F["PHASE_INTERIOR"], F["PHASE_BOUNDARY"]
    base = [0, F["NO_FUSE"], F["NO_QUAD"], F["IMAGE_ONLY"], F["PASS_A_ONLY"], F["PASS_B_ONLY"], F["EXACT"], F["FORCE_GENERAL"],
            F["FORCE_MIXED"], F["SWEEP_ONLY"] | F["FORCE_MIXED"], F["IMAGE_ONLY"] | F["NO_QUAD"]]
    flag_sets = base + [f | ph for ph in (PH1, PH2) for f in (0, F["NO_FUSE"], F["NO_QUAD"], F["IMAGE_ONLY"], F["EXACT"],
                                                               F["FORCE_GENERAL"], F["FORCE_MIXED"])] + [PH1 | PH2]
    records = []
    hashes = torch.zeros(1 << 20, dtype=torch.int64, device="cuda")   # one per output array, read back once at the end
    nh = [0]

    def tune(**kv):
        for k, v in kv.items():
            assert lib.ibh_set_tuning(k.encode(), int(v)) == 0

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    def record(case, name, outs, *args):
        rc = getattr(lib, name)(*args)
        msg = "" if rc == 0 else re.sub(r" \([^()]*:\d+\)$", "", lib.ibh_last_error().decode())
        for o in outs:
            x = o.view(torch.int32).reshape(-1)
            torch.sum(x * wts[: x.numel()], dim=(0,), dtype=torch.int64, out=hashes[nh[0]])
            nh[0] += 1
        records.append([case, name, rc, msg, len(outs)])

    tunings = [dict(zip(TUNING, v)) for v in itertools.product(*TUNING.values())]
    fluid = _lib.ibh_fluid(R=283.0, gamma=1.4)
    nmax = 0
    parts = partitions()
    for part in parts.values():
        nmax = max(nmax, part.spacing.shape[0])
    g = torch.Generator().manual_seed(7)
    wts = (torch.randint(1, 2 ** 31 - 1, (nmax * 16,), generator=g, dtype=torch.int32) | 1).cuda()
    nan = float("nan")
    for pname, part in parts.items():
        dp = backend.DevicePartition(part)
        h, nd, nc = dp.handle, dp.nd, dp.nc
        x = part.centers
        u = ibamd.hip(seeded_field(x))
        Cf = torch.ones((nd, nc), dtype=torch.float32, device="cuda")
        Cf[1] = -0.5
        Cf[0] += 0.3 * u
        Pt = torch.from_numpy(np.ascontiguousarray(euler_field(x, seed=3).T)).cuda()   # (nd + 2, nc): rows = fields
        ud = torch.full((nc,), nan, device="cuda")
        R = torch.full((nd + 2, nc), nan, device="cuda")
        uo = torch.full((nc,), nan, device="cuda")
        dt = torch.full((1,), 1e-3, device="cuda")
        vel = torch.stack([u, 0.5 * u + 1, -u]).contiguous()
        gnd = torch.full((nd * 3 + 3, nc), nan, device="cuda")
        gfl = torch.full((3 * (nd + 1), nc), nan, device="cuda")
        S = torch.full((nc,), nan, device="cuda")
        Gv = torch.full((9, nc), nan, device="cuda")
        nut, nuR, So = (torch.full((nc,), nan, device="cuda") for _ in range(3))
        Rpos = u.abs() + 0.1
        backend._stream()
        for qv in VARIANTS:
            for tn in tunings:
                tune(quad_variant=qv, **tn)
                tag = f"{pname} qv={qv} " + " ".join(f"{k}={v}" for k, v in tn.items())
                for fl in flag_sets:
                    record(f"{tag} flags={fl}", "ibh_residual_advection", [ud], h, ptr(u), ptr(Cf), nc, ptr(ud), fl)
                    record(f"{tag} flags={fl}", "ibh_residual_euler_hll", [R], h, ptr(Pt), nc, ptr(R), nc, C.byref(fluid), fl)
                ud.fill_(nan)
                R.fill_(nan)
                record(tag, "ibh_step_advection", [uo], h, ptr(u), ptr(uo), ptr(Cf), nc, ptr(dt), None)
                if tn["quad_parts"] == 3 and tn["rows"] == 0 and tn["rows_singles"] == -1:
                    # (these read no tuning key beyond the ones varied here: pass A, the closures)
                    record(tag, "ibh_cell_gradient_nd", [gnd], h, ptr(vel), 3, nc, ptr(gnd), nc, ptr(gnd[nd * 3:]), nc)
                    record(tag, "ibh_cell_gradient_nd", [gnd], h, ptr(u), 1, nc, ptr(gnd), nc, ptr(gnd[nd:]), nc)
                    record(tag, "ibh_cell_gradient_fields", [gfl], h, ptr(vel), 3, nc, ptr(gfl))
                    record(tag, "ibh_shear_rate_of_velocity", [S], h, ptr(vel), nc, ptr(S))
                    record(tag, "ibh_shear_rate_of_velocity_grad", [S, Gv], h, ptr(vel), nc, ptr(S), ptr(Gv), nc)
                    record(tag, "ibh_wray_agarwal_of", [nut, nuR, So], h, ptr(Rpos), ptr(S), C.c_float(0.6), C.c_float(0.2),
                           C.c_float(0.41), ptr(nut), ptr(nuR), ptr(So))
        tune(**DEFAULTS)
        torch.cuda.synchronize()
        print(f"{pname}: nd {nd}, {nc} cells, info {dp.info}, {len(records)} calls so far", flush=True)
    hv = hashes[: nh[0]].cpu().tolist()
    i = 0
    for r in records:
        n = r.pop()
        r.append(hv[i:i + n])
        i += n
    with open(path, "w") as f:
        json.dump(records, f)
    print(f"{len(records)} calls, {sum(1 for r in records if r[2])} rejected -> {path}")


def reduce_trace(d, path):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = []
    with open(files[0], newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if re.search(r"\bk_[a-z0-9_]+", name) and "at::" not in name:
                # (the unnamed namespace first: its "(anonymous namespace)::" would otherwise count as the parameter list)
                name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "")
                rows.append((int(r["Start_Timestamp"]), name, r["Grid_Size_X"], r["Workgroup_Size_X"]))
    rows.sort()
    with gzip.open(path, "wt") as f:
        for _, name, grid, wg in rows:
            f.write(f"{name}|{grid}|{wg}\n")
    print(f"{len(rows)} launches -> {path}")


def compare(ja, jb, la, lb):
    a, b = json.load(open(ja)), json.load(open(jb))
    bad = [(x, y) for x, y in zip(a, b) if x != y]
    print(f"calls: {len(a)} / {len(b)}, rejected {sum(1 for r in a if r[2])} / {sum(1 for r in b if r[2])}, "
          f"differing in code, message or output bits: {len(bad)}")
    for x, y in bad[:10]:
        print("  ", x, "|", y)
    ka, kb = gzip.open(la, "rt").read().splitlines(), gzip.open(lb, "rt").read().splitlines()
    first = next((i for i, (x, y) in enumerate(zip(ka, kb)) if x != y), None)
    print(f"launches: {len(ka)} / {len(kb)}, first difference: {first}")
    if first is not None:
        print("  ", ka[first], "|", kb[first])
    ok = len(a) == len(b) and not bad and ka == kb
    print("IDENTICAL" if ok else "DIFFERENT")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reduce", nargs=2)
    ap.add_argument("--compare", nargs=4)
    a = ap.parse_args()
    if a.reduce:
        reduce_trace(*a.reduce)
    elif a.compare:
        sys.exit(compare(*a.compare))
    else:
        run(a.out)
