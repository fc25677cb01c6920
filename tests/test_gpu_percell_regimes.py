"""The fused residual sweeps per cell across flow regimes, one production form per distinct implementation.

tests/test_gpu_percell.py runs every form on one flow state: Mach 0.3 with every velocity component positive, C_x > 0 > C_y.
Neither clamp of the HLL wave speeds binds there, no velocity changes sign, T stays off max(T, 10) and the upwind switch
|Cf| never changes sign inside a partition -- while the tuned forms do not evaluate the literal HLL combine but
rs = rcp(SL - SR), wL = SL rs, wR = SR rs, c = SL wR (ibh_sweep2d.h, ibh_block2d.h, ibh_block3d.h) and a regrouping by
state (ibh_quad2d_euler.h, ibh_strip3d_euler.h).  Here the fields of tests/regimes.py reach those branches, on the scales
``percell.euler_scale_waves`` / ``percell.scalar_scale_c`` and the bounds ``BOUND_EULER_REGIMES`` / ``BOUND_SCALAR_REGIMES``
calibrated on the CPU in tests/test_percell_regimes.py (under the present scales correct Float32 arithmetic fails at rest and
for |C| ~ 50, and anything passes for |C| ~ 1e-3).

Meshes, small because the float64 references dominate the time: the advection mesh in one partition (quads, pairs, singles,
rows, all three side classes), partition 2 of the 6144-cell RAE2822 cut (skirts, face-list cells, deeper-cell table,
image-only sweeps), the corner octree and sphere partition 1 (image-only columns).  One reference per (mesh, regime), built on
first use and kept for the module.  A form that gives NaN or Inf where the reference is finite fails ``percell.check``'s NaN
pattern or bound like any other error.
"""
import numpy as np
import pytest
import torch

import ibamd
import percell as pc
import percell_steps as ps
import regimes as rg
from conftest import ADV_FAMILIES, RAE_FAMILIES, oracle_view
from test_gpu_percell import EXACT, GENERAL, IMAGE, MIXED, NO_FUSE, NO_QUAD, _adv, _euler, _tuned

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MESHES = ("adv", "rae6k_2", "corner", "sphere_1")
MEASURED = {}   # (family, regime) -> worst per-cell error (printed at the end of the module, with -s)


def _record(form, regime, err):
    MEASURED[form, regime] = max(MEASURED.get((form, regime), 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    if MEASURED:
        print("\nper-cell maxima against float64 across regimes (form, regime):")
        for k in sorted(MEASURED):
            print(f"  {k[0]} | {k[1]}: {MEASURED[k]:.3e}")


class RegimeCase:
    """One partition with its device handle and cell classes; fields, float64 references and scales per regime."""

    def __init__(self, name, part):
        self.name, self.part = name, part
        self.nd = part.ndims
        self.dpart = ibamd.to_backend(part, ibamd.hip)
        self.info = self.dpart.info
        self.classes = pc.cell_classes(part)
        self.img = np.asarray(part.image_in_domain)
        self.op = oracle_view(part)
        self.partial = self.img.size < part.spacing.shape[0]     # a partition with skirts: image-only forms apply
        self._e, self._s, self._c = {}, {}, {}

    def euler(self, reg):
        if reg not in self._e:
            P = rg.euler_regime(self.part, reg)
            R64 = pc.ref64_euler(self.op, P)
            self._e[reg] = (P, R64, pc.euler_scale_waves(self.part, P, R64))
        return self._e[reg]

    def C(self, creg):
        if creg not in self._c:
            self._c[creg] = rg.c_regime(self.part, creg)
        return self._c[creg]

    def scalar(self, creg, kind):
        if (creg, kind) not in self._s:
            u, C = rg.u_kind(self.part, kind), self.C(creg)
            r64 = pc.ref64_advection(self.op, u, C)
            self._s[creg, kind] = (u, r64, pc.scalar_scale_c(self.part, u, C, r64))
        return self._s[creg, kind]


@pytest.fixture(scope="module")
def meshes(adv_mesh, rae_mesh_small):
    import bench
    from ibamd.mesher import Ball, Mesh
    out = {}
    dom = ibamd.Domain(adv_mesh, hypercube_families=ADV_FAMILIES, max_partition_size=10 ** 9, boundaries=False)
    (part,) = dom.partitions.values()
    out["adv"] = RegimeCase("adv", part)
    dom = ibamd.Domain(rae_mesh_small, hypercube_families=RAE_FAMILIES, max_partition_size=6144, boundaries=False, only=[2])
    out["rae6k_2"] = RegimeCase("rae6k_2", dom.partitions[2])
    msh = Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8,
               refinement_regions=[(Ball(np.array([-2.0, -2.0, -2.0]), 0.1), f32(0.1))])
    dom = ibamd.Domain(msh, max_partition_size=10 ** 9, boundaries=False)
    (part,) = dom.partitions.values()
    out["corner"] = RegimeCase("corner", part)
    msh = Mesh(f32([-4, -4, -4]), f32([8, 8, 8]), ("sphere", bench.icosphere(subdiv=2), f32(0.2)), block_size=8)
    msh.distance_fields = {}
    mps = -(-(-(-len(msh) // 4)) // 512) * 512
    dom = ibamd.Domain(msh, max_partition_size=mps, boundaries=False, only=[1])
    out["sphere_1"] = RegimeCase("sphere_1", dom.partitions[1])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# coverage: the meshes hold the block and side classes, the fields reach their branches
# ---------------------------------------------------------------------------------------------------------------------
def test_mesh_coverage(meshes):
    i = meshes["adv"].info
    assert i["fusable_blocks"] == i["full_blocks"] > 0 and i["irregular_cells"] == 0 and i["row_sweep"]
    for key in ("quads", "quad_singles", "quad_pairs", "sides_coarse", "sides_fine", "sides_mirror"):
        assert i[key] > 0, key
    c = meshes["rae6k_2"]
    i = c.info
    assert c.partial and i["irregular_cells"] > 0 and i["image_blocks_all_eligible"]
    assert i["image_quads"] > 0 and i["image_quad_singles"] > 0
    assert c.classes["deeper_table"][c.img].any() and "face_list" in c.classes and "skirt" in c.classes
    i = meshes["corner"].info
    assert i["fusable_blocks"] == i["full_blocks"] > 0 and i["irregular_cells"] == 0 and i["rim4_rows"] > 0
    c = meshes["sphere_1"]
    i = c.info
    assert c.partial and i["image_blocks_all_eligible"] and i["image_blocks"] * 512 == c.img.size
    for name in ("corner", "sphere_1"):
        for key in ("sides_same", "sides_mirror", "sides_coarse", "sides_fine"):
            assert meshes[name].info[key] > 0, (name, key)


@pytest.mark.parametrize("mesh", MESHES)
def test_regimes_reach_their_branches(meshes, mesh):
    """From the float64 reference's own intermediate values: supersonic+ has SR = 0 on every face (supersonic- SL = 0),
    transonic and crossing bind both clamps on at least 1 % of the faces each, cold clamps T on at least 25 % of the cells,
    floor has Df = 1e-7 on every uniform face (the majority; the rest is the mesh's, see ``regimes.assert_euler_coverage``),
    no regime has a face near SL = SR = 0, and the crossing C changes sign inside blocks."""
    c = meshes[mesh]
    for reg in rg.EULER_REGIMES:
        rg.assert_euler_coverage(c.op, c.euler(reg)[0], reg, what=mesh)
    both, _ = rg.cf_signs_in_blocks(c.op, c.C("crossing"))
    assert both >= 1, mesh
    assert not c.C("zero").any() and np.abs(c.C("big")).max() > 40 and np.abs(c.C("tiny")).max() < 2e-3


# ---------------------------------------------------------------------------------------------------------------------
# Euler
# ---------------------------------------------------------------------------------------------------------------------
def _euler_forms(c):
    """(family, form name, callable) of the Euler forms that run on the case: one per distinct HLL implementation."""
    d = c.dpart
    if c.nd == 2 and not c.partial:
        return [("2d quad", "2d euler quad", lambda P: _euler(d, P)),
                ("2d quad", "2d euler quad quad_singles_first=1",
                 lambda P: _tuned({"quad_singles_first": 1}, lambda: _euler(d, P))),
                ("2d quad", "2d euler quad phases", lambda P: _euler(d, P, phases=True)),
                ("2d per-block", "2d euler NO_QUAD", lambda P: _euler(d, P, NO_QUAD)),
                ("2d two-kernel", "2d euler NO_FUSE", lambda P: _euler(d, P, NO_FUSE)),
                ("2d literal", "2d euler EXACT", lambda P: _euler(d, P, EXACT)),
                ("2d literal", "2d euler FORCE_GENERAL", lambda P: _euler(d, P, GENERAL))]
    if c.nd == 2:
        return [("2d partition", "2d euler partition default", lambda P: _euler(d, P)),
                ("2d literal", "2d euler partition FORCE_GENERAL", lambda P: _euler(d, P, GENERAL)),
                ("2d image-only", "2d euler IMAGE_ONLY quads", lambda P: _euler(d, P, IMAGE)),
                ("2d image-only", "2d euler IMAGE_ONLY NO_QUAD", lambda P: _euler(d, P, IMAGE | NO_QUAD))]
    if not c.partial:
        return [("3d columns", "3d euler cols (default)", lambda P: _euler(d, P)),
                ("3d thread per cell", "3d euler quad_variant 512",
                 lambda P: _tuned({"quad_variant": 512}, lambda: _euler(d, P))),
                ("3d two-kernel", "3d euler NO_FUSE", lambda P: _euler(d, P, NO_FUSE)),
                ("3d literal", "3d euler FORCE_GENERAL", lambda P: _euler(d, P, GENERAL))]
    return [("3d partition", "3d euler partition default", lambda P: _euler(d, P)),
            ("3d image-only", "3d euler IMAGE_ONLY (cols)", lambda P: _euler(d, P, IMAGE))]


@pytest.mark.parametrize("regime", rg.EULER_REGIMES)
@pytest.mark.parametrize("mesh", MESHES)
def test_euler(meshes, mesh, regime):
    c = meshes[mesh]
    P, R64, S = c.euler(regime)
    assert np.isfinite(R64).all()
    for family, form, run in _euler_forms(c):
        got = run(P)
        cells = None
        if "IMAGE_ONLY" in form:
            assert np.isnan(got[:, 0]).sum() == got.shape[0] - c.img.size, form      # nothing written outside the image
            cells = c.img
        e = pc.check(got, R64, S, pc.BOUND_EULER_REGIMES, c.part, cells=cells, classes=c.classes,
                     what=f"{form} [{mesh}, regime {regime}]")
        _record("euler " + family, regime, e)


# ---------------------------------------------------------------------------------------------------------------------
# scalar
# ---------------------------------------------------------------------------------------------------------------------
def _scalar_forms(c):
    d = c.dpart
    if c.nd == 2 and not c.partial:
        return [("2d quad", "2d scalar quad", lambda u, C: _adv(d, u, C)),
                ("2d quad", "2d scalar quad pairs=0", lambda u, C: _tuned({"pairs": 0}, lambda: _adv(d, u, C))),
                ("2d quad", "2d scalar quad arith_ids=0", lambda u, C: _tuned({"arith_ids": 0}, lambda: _adv(d, u, C))),
                ("2d rows", "2d scalar rows", lambda u, C: _tuned({"rows": 1}, lambda: _adv(d, u, C))),
                ("2d per-block", "2d scalar NO_QUAD", lambda u, C: _adv(d, u, C, NO_QUAD)),
                ("2d two-kernel", "2d scalar NO_FUSE", lambda u, C: _adv(d, u, C, NO_FUSE)),
                ("2d literal", "2d scalar EXACT", lambda u, C: _adv(d, u, C, EXACT))]
    if c.nd == 2:
        return [("2d partition", "2d scalar partition default", lambda u, C: _adv(d, u, C)),
                ("2d mixed", "2d scalar partition FORCE_MIXED", lambda u, C: _adv(d, u, C, MIXED)),
                ("2d two-kernel", "2d scalar partition NO_FUSE", lambda u, C: _adv(d, u, C, NO_FUSE)),
                ("2d literal", "2d scalar partition EXACT", lambda u, C: _adv(d, u, C, EXACT)),
                ("2d image-only", "2d scalar IMAGE_ONLY quads", lambda u, C: _adv(d, u, C, IMAGE)),
                ("2d image-only", "2d scalar IMAGE_ONLY NO_QUAD", lambda u, C: _adv(d, u, C, IMAGE | NO_QUAD))]
    if not c.partial:
        return [("3d columns", "3d scalar cols (default)", lambda u, C: _adv(d, u, C)),
                ("3d thread per cell", "3d scalar quad_variant 512",
                 lambda u, C: _tuned({"quad_variant": 512}, lambda: _adv(d, u, C))),
                ("3d two-kernel", "3d scalar NO_FUSE", lambda u, C: _adv(d, u, C, NO_FUSE)),
                ("3d literal", "3d scalar FORCE_GENERAL", lambda u, C: _adv(d, u, C, GENERAL))]
    return [("3d partition", "3d scalar partition default", lambda u, C: _adv(d, u, C)),
            ("3d two-kernel", "3d scalar partition NO_FUSE", lambda u, C: _adv(d, u, C, NO_FUSE)),
            ("3d image-only", "3d scalar IMAGE_ONLY (cols)", lambda u, C: _adv(d, u, C, IMAGE))]


@pytest.mark.parametrize("creg", rg.C_REGIMES)
@pytest.mark.parametrize("mesh", MESHES)
def test_scalar(meshes, mesh, creg):
    """Every (C, u) pair in every form; C = 0 gives exactly zero (an equality, not a bound)."""
    c = meshes[mesh]
    C = c.C(creg)
    n = c.part.spacing.shape[0]
    for kind in rg.U_KINDS:
        u, r64, s = c.scalar(creg, kind)
        for family, form, run in _scalar_forms(c):
            got = run(u, C)
            cells = None
            if "IMAGE_ONLY" in form:
                assert np.isnan(got).sum() == n - c.img.size, form
                cells = c.img
            what = f"{form} [{mesh}, C {creg}, u {kind}]"
            if creg == "zero":
                sel = np.arange(n) if cells is None else cells
                assert not r64.any()
                assert np.array_equal(got[sel], np.zeros(sel.size, f32)), what
                continue
            e = pc.check(got, r64, s, pc.BOUND_SCALAR_REGIMES, c.part, cells=cells, classes=c.classes, what=what)
            _record("scalar " + family, f"C {creg}", e)


@pytest.mark.parametrize("creg", rg.C_REGIMES)
@pytest.mark.parametrize("mesh", MESHES)
def test_timestep(meshes, mesh, creg):
    """``timestep_advection(scale=0.75)`` against the float64 maximum: 4 ulp; C = 0 gives the reference's 0.375 / 0 = Inf."""
    c = meshes[mesh]
    C = c.C(creg)
    got = float(ibamd.to_host(ibamd.timestep_advection(c.dpart, ibamd.hip(C), scale=0.75))[0])
    ref = float(ps.dt_ref(ps.dt_percell(c.op, C), 0.75))
    if creg == "zero":
        assert ref == np.inf and got == np.inf, (got, ref)
        return
    _record("timestep_advection", f"C {creg}", ps.check_dt(got, ref, what=f"dt [{mesh}, C {creg}]"))


@pytest.mark.parametrize("creg", ["crossing", "big"])
def test_step_advection(meshes, creg):
    """out = u + dt R(u) in one launch against u + dt R64: the regime bound on dt x scale, plus the one rounding of the
    stored sum (as tests/test_gpu_percell.py::test_2d_step_advection)."""
    c = meshes["adv"]
    C = c.C(creg)
    dt = ibamd.timestep_advection(c.dpart, ibamd.hip(C), scale=0.75)
    h = float(ibamd.to_host(dt)[0])
    for kind in rg.U_KINDS:
        u, r64, s = c.scalar(creg, kind)
        for t in ({}, {"pairs": 0}, {"arith_ids": 0}):
            out = torch.full((u.shape[0],), float("nan"), dtype=torch.float32, device="cuda")
            _tuned(t, lambda: ibamd.step_advection(c.dpart, ibamd.hip(u), ibamd.hip(C), dt, out=out))
            got = ibamd.to_host(out).astype(f64)
            exp = u.astype(f64) + h * r64
            ulp = np.spacing(np.abs(exp).astype(f32)).astype(f64)
            d = got - exp
            got_eff = exp + np.sign(d) * np.maximum(np.abs(d) - ulp, 0.0)
            e = pc.check(got_eff, exp, h * s, pc.BOUND_SCALAR_REGIMES, c.part, classes=c.classes,
                         what=f"step_advection {t} [adv, C {creg}, u {kind}]")
            _record("scalar 2d step_advection", f"C {creg}", e)
