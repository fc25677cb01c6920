"""Every production form of the fused residual sweeps, per cell, against one float64 evaluation of the oracle.

The checker is tests/percell.py (bounds, scales and the per-class report); tests/test_percell.py calibrates it and shows
that it sees errors the norm-wise checks cannot.  Each test builds one float64 reference per mesh and field and runs
every form of ``ibh_residual_advection`` / ``ibh_residual_euler_hll`` (csrc/ibh_fused*.hip) that computes the residual on
that kind of partition against it, with the same bound.  ``dpart.info`` pins the coverage: a mesh change that empties a
block or side class fails here instead of silently dropping it.

Not run here, on purpose:
- ``quad_variant`` 4: the measurement variant (wave time stamps).
"""
import numpy as np
import pytest
import torch

import ibamd
import percell as pc
from conftest import ADV_FAMILIES, RAE_FAMILIES, euler_field, oracle_view, seeded_field
from ibamd import _lib

pytestmark = pytest.mark.gpu
f32 = np.float32
NO_QUAD, NO_FUSE, EXACT, GENERAL = ibamd.IBH_NO_QUAD, ibamd.IBH_NO_FUSE, ibamd.IBH_EXACT, ibamd.IBH_FORCE_GENERAL
MIXED, IMAGE, PH1, PH2 = ibamd.IBH_FORCE_MIXED, ibamd.IBH_IMAGE_ONLY, ibamd.IBH_PHASE_INTERIOR, ibamd.IBH_PHASE_BOUNDARY
# library defaults of the tuning keys (restored after every form)
DEFAULTS = {"quad_variant": 0, "pairs": 1, "arith_ids": 1, "quad_singles_first": 0, "rows_singles": -1, "rows": 0}
MEASURED = {}   # form -> worst per-cell error (printed at the end of the module, with -s)


def _tuned(tuning, fn):
    try:
        for k, v in tuning.items():
            _lib.call("ibh_set_tuning", k.encode(), int(v))
        return fn()
    finally:
        for k in tuning:
            _lib.call("ibh_set_tuning", k.encode(), DEFAULTS[k])


def _adv(dpart, u, C, flags=0, phases=False):
    """The scalar sweep into a NaN-filled output (whole sweep, or the two overlap phases one after the other)."""
    out = torch.full((u.shape[0],), float("nan"), dtype=torch.float32, device="cuda")
    du, dC = ibamd.hip(u), ibamd.hip(C)
    if phases:
        ibamd.residual_advection(dpart, du, dC, out=out, flags=flags | PH1)
        ibamd.residual_advection(dpart, du, dC, out=out, flags=flags | PH2)
    else:
        ibamd.residual_advection(dpart, du, dC, out=out, flags=flags)
    return ibamd.to_host(out)


def _euler(dpart, P, flags=0, phases=False):
    out = torch.full((P.shape[1], P.shape[0]), float("nan"), dtype=torch.float32, device="cuda").T
    dP = ibamd.hip(P)
    if phases:
        ibamd.residual_euler_hll(dpart, dP, out=out, flags=flags | PH1)
        ibamd.residual_euler_hll(dpart, dP, out=out, flags=flags | PH2)
    else:
        ibamd.residual_euler_hll(dpart, dP, out=out, flags=flags)
    return ibamd.to_host(out)


def _record(form, err):
    MEASURED[form] = max(MEASURED.get(form, 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    if MEASURED:
        print("\nper-cell maxima against float64:")
        for k in sorted(MEASURED):
            print(f"  {k}: {MEASURED[k]:.3e}")


class Case:
    """One partition with its device handle, cell classes, fields and float64 references."""

    def __init__(self, part, kinds=("smooth", "step"), nd=2):
        self.part = part
        self.dpart = ibamd.to_backend(part, ibamd.hip)
        self.info = self.dpart.info
        self.classes = pc.cell_classes(part)
        self.img = np.asarray(part.image_in_domain)
        op = oracle_view(part)
        x = part.centers
        n = x.shape[0]
        if nd == 2:
            self.C = np.stack([f32(1) + seeded_field(x, seed=5) * f32(0.3), f32(-0.5) + seeded_field(x, seed=3) * f32(0.1)],
                              axis=1)
            self.u = {kind: seeded_field(x, kind=kind) for kind in kinds}
        else:
            rng = np.random.default_rng(11)
            self.C = np.stack([np.ones(n, f32), f32(0.5) + f32(0.1) * rng.uniform(-1, 1, n).astype(f32),
                               np.full(n, -0.25, f32)], axis=1)
            self.u = {"smooth": (np.sin(2 * x[:, 0]) * np.cos(3 * x[:, 1]) + 0.3 * x[:, 2]
                                 + 0.1 * rng.uniform(-1, 1, n)).astype(f32)}
        self.r64 = {k: pc.ref64_advection(op, u, self.C) for k, u in self.u.items()}
        self.s = {k: pc.scalar_scale(part, u, self.r64[k]) for k, u in self.u.items()}
        self.P = euler_field(x, seed=3)
        self.R64 = pc.ref64_euler(op, self.P)
        self.S = pc.euler_scale(part, self.P, self.R64)

    def check_adv(self, form, got, kind, cells=None, bound=pc.BOUND):
        e = pc.check(got, self.r64[kind], self.s[kind], bound, self.part, cells=cells, classes=self.classes,
                     what=f"{form} [{kind}]")
        _record(form, e)

    def check_euler(self, form, got, cells=None, bound=pc.BOUND_EULER):
        e = pc.check(got, self.R64, self.S, bound, self.part, cells=cells, classes=self.classes, what=form)
        _record(form, e)


# ---------------------------------------------------------------------------------------------------------------------
# 2-D meshes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_part(adv_mesh, rae_mesh_small):
    """One-partition domains (every block eligible: quad sweep, pairs, rows): the advection case and RAE2822."""
    out = {}
    for name, msh, fam in (("adv", adv_mesh, ADV_FAMILIES), ("rae", rae_mesh_small, RAE_FAMILIES)):
        dom = ibamd.Domain(msh, hypercube_families=fam, max_partition_size=10 ** 9, boundaries=False)
        (part,) = dom.partitions.values()
        out[name] = Case(part)
    return out


@pytest.fixture(scope="module")
def partitions(rae_mesh_small):
    """RAE2822 partitions with skirt fragments: the three of the test domain and two cut at 6144 cells whose image holds a
    block that takes its deeper cells from the table (BlockDesc2::dt)."""
    out = {}
    dom = ibamd.Domain(rae_mesh_small, hypercube_families=RAE_FAMILIES, max_partition_size=16384, boundaries=False)
    for k, part in dom.partitions.items():
        out[f"rae16k_{k}"] = Case(part, kinds=("step",))
    dom = ibamd.Domain(rae_mesh_small, hypercube_families=RAE_FAMILIES, max_partition_size=6144, boundaries=False,
                       only=[2, 5])
    for k in (2, 5):
        out[f"rae6k_{k}"] = Case(dom.partitions[k], kinds=("step",))
    return out


def test_2d_coverage(one_part, partitions):
    for name, c in one_part.items():
        i = c.info
        assert c.dpart.info["fusable_blocks"] == i["full_blocks"] > 0 and i["irregular_cells"] == 0, name
        for key in ("quads", "quad_singles", "quad_pairs", "sides_coarse", "sides_fine", "sides_mirror"):
            assert i[key] > 0, (name, key)
        assert i["row_sweep"], name
    for name, c in partitions.items():
        i = c.info
        assert i["irregular_cells"] > 0 and i["image_blocks_all_eligible"], name
        assert i["image_quads"] > 0 and i["image_quad_singles"] > 0, name
    for key in ("sides_coarse", "sides_fine", "sides_mirror"):
        assert all(c.info[key] > 0 for n, c in partitions.items() if n.startswith("rae16k")), key
    assert sum(c.classes.get("deeper_table", np.zeros(1, bool)).any() for c in partitions.values()) >= 1
    assert all(c.classes.get("deeper_table", np.zeros(1, bool))[c.img].any()
               for n, c in partitions.items() if n.startswith("rae6k"))


QUAD_TUNINGS = [dict(pairs=p, arith_ids=a, quad_singles_first=s, rows_singles=r)
                for p in (0, 1) for a in (0, 1) for s in (0, 1) for r in (0, 1, 2)]


@pytest.mark.parametrize("case", ["adv", "rae"])
def test_2d_scalar_one_partition(one_part, case):
    c = one_part[case]
    for kind, u in c.u.items():
        for t in QUAD_TUNINGS:
            got = _tuned(t, lambda: _adv(c.dpart, u, c.C))
            c.check_adv("2d scalar quad " + ",".join(f"{k}={v}" for k, v in t.items()), got, kind)
        c.check_adv("2d scalar quad phases", _adv(c.dpart, u, c.C, phases=True), kind)
        c.check_adv("2d scalar NO_QUAD (k_sweep_adv)", _adv(c.dpart, u, c.C, NO_QUAD), kind)
        c.check_adv("2d scalar NO_QUAD phases", _adv(c.dpart, u, c.C, NO_QUAD, phases=True), kind)
        c.check_adv("2d scalar rows", _tuned({"rows": 1}, lambda: _adv(c.dpart, u, c.C)), kind)
        c.check_adv("2d scalar rows phases", _tuned({"rows": 1}, lambda: _adv(c.dpart, u, c.C, phases=True)), kind)
        c.check_adv("2d scalar NO_FUSE", _adv(c.dpart, u, c.C, NO_FUSE), kind)
        c.check_adv("2d scalar NO_FUSE phases", _adv(c.dpart, u, c.C, NO_FUSE, phases=True), kind)
        c.check_adv("2d scalar EXACT", _adv(c.dpart, u, c.C, EXACT), kind)
        c.check_adv("2d scalar FORCE_GENERAL", _adv(c.dpart, u, c.C, GENERAL), kind)


def test_2d_scalar_partitions(partitions):
    for name, c in partitions.items():
        u = c.u["step"]
        c.check_adv("2d scalar partition default", _adv(c.dpart, u, c.C), "step")
        c.check_adv("2d scalar partition default phases", _adv(c.dpart, u, c.C, phases=True), "step")
        c.check_adv("2d scalar partition FORCE_MIXED", _adv(c.dpart, u, c.C, MIXED), "step")
        c.check_adv("2d scalar partition FORCE_MIXED phases", _adv(c.dpart, u, c.C, MIXED, phases=True), "step")
        c.check_adv("2d scalar partition NO_FUSE", _adv(c.dpart, u, c.C, NO_FUSE), "step")
        c.check_adv("2d scalar partition EXACT", _adv(c.dpart, u, c.C, EXACT), "step")
        c.check_adv("2d scalar partition FORCE_GENERAL", _adv(c.dpart, u, c.C, GENERAL), "step")
        for t in ({}, {"quad_singles_first": 1}, {"arith_ids": 0}):
            got = _tuned(t, lambda: _adv(c.dpart, u, c.C, IMAGE))
            assert np.isnan(got).sum() == got.shape[0] - c.img.size, name       # nothing written outside the image
            c.check_adv("2d scalar IMAGE_ONLY quads " + ",".join(f"{k}={v}" for k, v in t.items()), got, "step",
                        cells=c.img)
        c.check_adv("2d scalar IMAGE_ONLY phases", _adv(c.dpart, u, c.C, IMAGE, phases=True), "step", cells=c.img)
        c.check_adv("2d scalar IMAGE_ONLY NO_QUAD", _adv(c.dpart, u, c.C, IMAGE | NO_QUAD), "step", cells=c.img)
        c.check_adv("2d scalar IMAGE_ONLY NO_QUAD phases", _adv(c.dpart, u, c.C, IMAGE | NO_QUAD, phases=True), "step",
                    cells=c.img)


@pytest.mark.parametrize("case", ["adv", "rae"])
def test_2d_step_advection(one_part, case):
    """out = u + dt R(u) in one launch (the quad sweep stores the update), against u + dt R64: the per-cell bound on
    dt x scale, plus the one rounding of the stored sum."""
    c = one_part[case]
    for kind, u in c.u.items():
        dt = ibamd.timestep_advection(c.dpart, ibamd.hip(c.C), scale=0.75)
        for t in ({}, {"pairs": 0}, {"arith_ids": 0}):
            out = torch.full((u.shape[0],), float("nan"), dtype=torch.float32, device="cuda")
            _tuned(t, lambda: ibamd.step_advection(c.dpart, ibamd.hip(u), ibamd.hip(c.C), dt, out=out))
            got = ibamd.to_host(out).astype(np.float64)
            h = float(ibamd.to_host(dt)[0])
            exp = u.astype(np.float64) + h * c.r64[kind]
            ulp = np.spacing(np.abs(exp).astype(f32)).astype(np.float64)
            d = got - exp
            got_eff = exp + np.sign(d) * np.maximum(np.abs(d) - ulp, 0.0)
            e = pc.check(got_eff, exp, h * c.s[kind], pc.BOUND, c.part, classes=c.classes,
                         what=f"step_advection {t} [{kind}]")
            _record("2d step_advection " + ",".join(f"{k}={v}" for k, v in t.items()), e)


@pytest.mark.parametrize("case", ["adv", "rae"])
def test_2d_euler_one_partition(one_part, case):
    c = one_part[case]
    for t in ({}, {"quad_singles_first": 1}):
        c.check_euler("2d euler quad " + ",".join(f"{k}={v}" for k, v in t.items()),
                      _tuned(t, lambda: _euler(c.dpart, c.P)))
    c.check_euler("2d euler quad phases", _euler(c.dpart, c.P, phases=True))
    c.check_euler("2d euler NO_QUAD (k_sweep_euler)", _euler(c.dpart, c.P, NO_QUAD))
    c.check_euler("2d euler NO_QUAD phases", _euler(c.dpart, c.P, NO_QUAD, phases=True))
    c.check_euler("2d euler NO_FUSE", _euler(c.dpart, c.P, NO_FUSE))
    c.check_euler("2d euler EXACT", _euler(c.dpart, c.P, EXACT))
    c.check_euler("2d euler FORCE_GENERAL", _euler(c.dpart, c.P, GENERAL))


def test_2d_euler_partitions(partitions):
    for name, c in partitions.items():
        c.check_euler("2d euler partition default", _euler(c.dpart, c.P))
        c.check_euler("2d euler partition FORCE_GENERAL", _euler(c.dpart, c.P, GENERAL))
        got = _euler(c.dpart, c.P, IMAGE)
        assert np.isnan(got[:, 0]).sum() == got.shape[0] - c.img.size, name
        c.check_euler("2d euler IMAGE_ONLY quads", got, cells=c.img)
        c.check_euler("2d euler IMAGE_ONLY phases", _euler(c.dpart, c.P, IMAGE, phases=True), cells=c.img)
        c.check_euler("2d euler IMAGE_ONLY NO_QUAD", _euler(c.dpart, c.P, IMAGE | NO_QUAD), cells=c.img)


# ---------------------------------------------------------------------------------------------------------------------
# 3-D meshes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def octrees():
    """One-partition octrees of 8^3 blocks with level jumps (SAME / MIRROR / COARSE / FINE sides, rim cells) and the
    partitions with skirt fragments of a sphere mesh (image-only column sweeps)."""
    import bench
    from ibamd.mesher import Ball, Mesh
    out = {}
    for name, ball in (("corner", (Ball(np.array([-2.0, -2.0, -2.0]), 0.1), f32(0.1))),
                       ("ball", (Ball(np.array([1.2, 1.2, 1.2]), 0.1), f32(0.1)))):
        msh = Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8, refinement_regions=[ball])
        dom = ibamd.Domain(msh, max_partition_size=10 ** 9, boundaries=False)
        (part,) = dom.partitions.values()
        out[name] = Case(part, nd=3)
    msh = Mesh(f32([-4, -4, -4]), f32([8, 8, 8]), ("sphere", bench.icosphere(subdiv=2), f32(0.2)), block_size=8)
    msh.distance_fields = {}
    n = len(msh)
    mps = -(-(-(-n // 4)) // 512) * 512
    dom = ibamd.Domain(msh, max_partition_size=mps, boundaries=False, only=[1, 3])
    for k in (1, 3):
        out[f"sphere_{k}"] = Case(dom.partitions[k], nd=3)
    return out


def test_3d_coverage(octrees):
    for name, c in octrees.items():
        i = c.info
        for key in ("sides_same", "sides_mirror", "sides_coarse", "sides_fine"):
            assert i[key] > 0, (name, key)
        if name.startswith("sphere"):
            assert i["image_blocks_all_eligible"] and i["image_blocks"] * 512 == c.img.size < c.part.spacing.shape[0]
        else:
            assert i["fusable_blocks"] == i["full_blocks"] > 0 and i["irregular_cells"] == 0 and i["rim4_rows"] > 0


def test_3d_scalar(octrees):
    for name, c in octrees.items():
        u = c.u["smooth"]
        if name.startswith("sphere"):
            got = _adv(c.dpart, u, c.C, IMAGE)
            assert np.isnan(got).sum() == got.shape[0] - c.img.size, name
            c.check_adv("3d scalar IMAGE_ONLY (cols)", got, "smooth", cells=c.img)
            c.check_adv("3d scalar partition default", _adv(c.dpart, u, c.C), "smooth")
            c.check_adv("3d scalar partition NO_FUSE", _adv(c.dpart, u, c.C, NO_FUSE), "smooth")
            continue
        c.check_adv("3d scalar cols (default)", _adv(c.dpart, u, c.C), "smooth")
        # 512: thread per cell
        for v in (512,):
            c.check_adv(f"3d scalar quad_variant {v}", _tuned({"quad_variant": v}, lambda: _adv(c.dpart, u, c.C)), "smooth")
        c.check_adv("3d scalar NO_FUSE", _adv(c.dpart, u, c.C, NO_FUSE), "smooth")
        c.check_adv("3d scalar NO_FUSE phases", _adv(c.dpart, u, c.C, NO_FUSE, phases=True), "smooth")
        c.check_adv("3d scalar FORCE_GENERAL", _adv(c.dpart, u, c.C, GENERAL), "smooth")


def test_3d_euler(octrees):
    for name, c in octrees.items():
        if name.startswith("sphere"):
            got = _euler(c.dpart, c.P, IMAGE)
            assert np.isnan(got[:, 0]).sum() == got.shape[0] - c.img.size, name
            c.check_euler("3d euler IMAGE_ONLY (cols)", got, cells=c.img)
            c.check_euler("3d euler partition default", _euler(c.dpart, c.P))
            continue
        c.check_euler("3d euler cols (default)", _euler(c.dpart, c.P))
        c.check_euler("3d euler quad_variant 512", _tuned({"quad_variant": 512}, lambda: _euler(c.dpart, c.P)))
        c.check_euler("3d euler NO_FUSE", _euler(c.dpart, c.P, NO_FUSE))
        c.check_euler("3d euler FORCE_GENERAL", _euler(c.dpart, c.P, GENERAL))


# the kernel forms that lost their A/B and were removed (gather subsets and the seven 4-byte gathers of the quad sweep, the
# persistent Euler sweep, the strip form and the 4- and 5-wave column forms of the 3-D scalar sweep), and one value never defined
RETIRED_QUAD_VARIANTS = (5, 69, 85, 100, 126, 514, 515, 518, 519, 520, 7)


def test_retired_quad_variants_are_rejected(octrees, one_part):
    """``ibh_set_tuning("quad_variant", v)`` takes 0, 4 and 512 only: a value of a removed form is an error that leaves
    the setting as it was -- it must not quietly run (and let a probe script time) the default form."""
    lib = _lib.load()
    c3, c2 = octrees["corner"], one_part["adv"]
    try:
        for v in RETIRED_QUAD_VARIANTS:
            rc = lib.ibh_set_tuning(b"quad_variant", v)   # (the raw entry: _lib.call raises on a non-zero code)
            msg = lib.ibh_last_error().decode()
            assert rc != 0, v
            assert "quad_variant" in msg, (v, msg)
        # the setting is still 0: the default forms, with the bound they pass in test_3d_scalar / test_2d_scalar_one_partition
        c3.check_adv("3d scalar cols (default) after rejected quad_variant", _adv(c3.dpart, c3.u["smooth"], c3.C), "smooth")
        c2.check_adv("2d scalar quad (default) after rejected quad_variant", _adv(c2.dpart, c2.u["smooth"], c2.C), "smooth")
        for v in (0, 4, 512):
            assert lib.ibh_set_tuning(b"quad_variant", v) == 0, v
    finally:
        _lib.call("ibh_set_tuning", b"quad_variant", 0)
