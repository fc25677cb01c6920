"""Dump every output of the fused gradient closures on the four small partitions of tests/closure_cases.py, or compare two
dumps: the check that a build computes what another build computed, bit for bit.

    python scripts/dump_closures.py dump OUT.npz          (needs a GPU; run it in the tree of each build)
    python scripts/dump_closures.py compare A.npz B.npz   (prints "N arrays, D differ"; exit status 1 when D > 0)

Per mesh (``octree``, ``single``: wave per 8^3 block; ``bs4 2d``, ``bs4 3d``: thread per cell over the side table), on the
seeded fields of tests/kepsilon_model.py, once as they are and once with a NaN velocity entry: ``shear_rate_of_velocity`` with
the gradients, ``les_closure_of`` with every output (Smagorinsky, and WALE in 3-D), ``Wray_Agarwal_of``, ``k_epsilon_rhs``
with ``S`` and the gradients, and ``scalar_transport``.  Then the users of the 3-D gradient sweep below the closures
(``dump_sweeps``), on ``octree``, ``single`` and the second of two partitions of the octree (``skirt``: GENERAL sides and
skirt fragments), with and without a NaN entry: the tuple ``cell_gradient`` of one field and of a 5-column array,
``JST_sensor``, ``residual_advection`` and ``residual_euler_hll`` with ``IBH_NO_FUSE`` (the two-kernel form) and with
``quad_variant`` 512 (the thread-per-cell single kernels).  Two arrays are the same when their NaN patterns are equal and
every other element has the same bits.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def dump(path):
    import ibamd
    import kepsilon_model as km
    import les_model as lm
    from ibamd import turbulence as T
    meshes = {"octree": lm.octree_mesh(), "single": lm.single_block_mesh(), "bs4 2d": lm.bs4_mesh(2), "bs4 3d": lm.bs4_mesh(3)}
    out = {}
    for name, msh in meshes.items():
        part = lm.one_partition(msh)
        dpart = ibamd.to_backend(part, ibamd.hip)
        assert T.fused_closures_apply(dpart), name
        nd, nc = part.ndims, dpart.nc
        Delta = ibamd.hip(lm.filter_width(part))
        for tag in ("", " nan"):
            v = km.wavy_velocity(part, 21)
            if tag:
                v[nc // 2, 0] = np.nan
            kh, eh = km.k_eps_fields(part, 22)
            vel, k, eps = ibamd.hip(v), ibamd.hip(kh), ibamd.hip(eh)
            res = {}
            S, G = T.shear_rate_of_velocity(dpart, vel, gradients=True)
            res["shear"] = dict(S=S, S_alone=T.shear_rate_of_velocity(dpart, vel), gradients=G)
            for model in ("smagorinsky", "wale")[:nd - 1]:
                res[model] = T.les_closure_of(dpart, vel, Delta, model=model, ducros=True, shock=True, shear=True, gradients=True)
            res["wray_agarwal"] = T.Wray_Agarwal_of(dpart, k, eps)
            res["k_epsilon"] = T.k_epsilon_rhs(dpart, vel, k, eps, float(km.NU), shear=True, gradients=True)
            res["transport"] = dict(out=T.scalar_transport(dpart, k, eps, vel, float(km.NU), S))
            for call, d in res.items():
                for key, a in d.items():
                    for j, b in enumerate(a if isinstance(a, tuple) else (a,)):
                        out[f"{name}{tag} | {call} | {key}{j if isinstance(a, tuple) else ''}"] = ibamd.to_host(b)
    dump_sweeps(out, {"octree": meshes["octree"], "single": meshes["single"]})
    np.savez(path, **out)
    print(f"{len(out)} arrays written to {path}")


def dump_sweeps(out, meshes):
    import closure_cases
    import ibamd
    import les_model as lm
    from ibamd import _lib
    f32 = np.float32
    parts = {name: lm.one_partition(msh) for name, msh in meshes.items()}
    parts["skirt"] = closure_cases.skirt_case(closure_cases.Case).part
    for name, part in parts.items():
        dpart = ibamd.to_backend(part, ibamd.hip)
        x, nc = part.centers, part.centers.shape[0]
        rng = np.random.default_rng(31)
        r = lambda: rng.uniform(-1, 1, nc)
        for tag in ("", " nan"):
            u = (np.sin(2 * x[:, 0]) * np.cos(3 * x[:, 1]) + 0.3 * x[:, 2] + 0.1 * r()).astype(f32)
            C = np.stack([np.ones(nc), 0.5 + 0.1 * r(), -0.25 * np.ones(nc)], axis=1).astype(f32)
            P = np.stack([1e5 * (1 + 0.05 * r()), 288.15 * (1 + 0.05 * r()), 100.0 * (1 + 0.1 * r()), 60.0 * (1 + 0.1 * r()),
                          -40.0 * (1 + 0.1 * r())], axis=1).astype(f32)
            if tag:
                u[nc // 2] = np.nan
                P[nc // 3, 0] = np.nan
            du, dC, dP = ibamd.hip(u), ibamd.hip(C), ibamd.hip(P)
            res = {"gradient of one field": ibamd.cell_gradient(dpart, du), "gradient of five columns": ibamd.cell_gradient(dpart, dP),
                   "JST_sensor": ibamd.JST_sensor(dpart, du),
                   "advection two-kernel": ibamd.residual_advection(dpart, du, dC, flags=ibamd.IBH_NO_FUSE),
                   "euler two-kernel": ibamd.residual_euler_hll(dpart, dP, flags=ibamd.IBH_NO_FUSE)}
            _lib.call("ibh_set_tuning", b"quad_variant", 512)
            try:
                res["advection 512"] = ibamd.residual_advection(dpart, du, dC)
                res["euler 512"] = ibamd.residual_euler_hll(dpart, dP)
            finally:
                _lib.call("ibh_set_tuning", b"quad_variant", 0)
            for call, a in res.items():
                for j, b in enumerate(a if isinstance(a, tuple) else (a,)):
                    out[f"{name}{tag} | {call} | {j}"] = ibamd.to_host(b)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        nx, ny = np.isnan(x), np.isnan(y)
        if x.shape != y.shape or not np.array_equal(nx, ny) or not np.array_equal(x[~nx].view(np.uint32), y[~ny].view(np.uint32)):
            bad.append(k)
    for k in bad:
        print("DIFFERENT ", k)
    n_nan = sum(int(np.isnan(a[k]).any()) for k in a.files)
    print(f"{len(a.files)} arrays ({n_nan} with NaN), {len(bad)} differ")
    return 1 if bad or not a.files else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
