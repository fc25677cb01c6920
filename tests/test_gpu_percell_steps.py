"""The kernels a solver step runs around the sweep, per element, against float64 (tests/percell_steps.py).

Accumulator application in all its forms, the time step cell by cell, the two-stage reductions with their element-wise
halves, and the point-implicit block kernels.  tests/test_percell_steps.py calibrates the bounds and shows that each check
sees the error it is there for.  Every coverage claim (entry paths, tiled and untiled partitions, side classes, the
arg-max of every probe) is asserted from the data.

The boundary conditions run as ``ibh_bc_apply`` (both closures), ``BCSet.apply`` and inside ``step_advection(...,
next_dt=...)`` (the BC + time-step launches), on real boundaries and on synthetic sets that each force one branch of the
level construction of ``ibh_bcset_create`` (level and direct-level counts asserted from ``ibh_bcset_info``).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ibamd
import percell as pc
import percell_steps as ps
from conftest import ADV_FAMILIES, RAE_FAMILIES, oracle_view
from ibamd import _lib
from ibamd import backend as B
from ibamd import hiparray as H
from ibamd.accumulator import Accumulator

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MEASURED = {}


def _record(name, e):
    MEASURED[name] = max(MEASURED.get(name, 0.0), float(e))


@pytest.fixture(scope="module", autouse=True)
def _print_measured():
    yield
    if MEASURED:
        print("\nper-element maxima against float64:")
        for k in sorted(MEASURED, key=str):
            print(f"  {k}: {MEASURED[k]:.3e}")


def call(name, *a):
    B._stream()
    _lib.call(name, *a)


def dvec(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


KEEP = []


def keep(a, dtype=torch.float32):
    """``dvec`` whose tensor lives until the end of the test: a temporary would be freed as soon as its pointer is taken,
    and the next upload would get the same block."""
    KEEP.append(dvec(a, dtype))
    return KEEP[-1]


@pytest.fixture(autouse=True)
def _release():
    yield
    KEEP.clear()


def to_field(v, ld):
    """(n, nv) host array -> (nv, ld) device buffer, column v at [v, :n], NaN in the padding: a column-major view of a
    wider array."""
    v = np.asarray(v, f32)
    v = v[:, None] if v.ndim == 1 else v
    buf = torch.full((v.shape[1], ld), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :v.shape[0]] = torch.from_numpy(np.ascontiguousarray(v.T)).cuda()
    return buf


def from_field(buf, n):
    """(n, nv) host array of the buffer's rows; asserts that the padding is still NaN (nothing written past a column)."""
    h = buf.cpu().numpy()
    assert np.isnan(h[:, n:]).all(), "a kernel wrote into the padding between columns"
    return np.ascontiguousarray(h[:, :n].T)


# ---------------------------------------------------------------------------------------------------------------------
# 1. Accumulator family
# ---------------------------------------------------------------------------------------------------------------------
def _dacc(off, idx, w, n_in):
    return B.DeviceAccumulator(Accumulator(csr=(off, idx, w), n_input=n_in))


def _apply(dacc, v, ldv, ldo):
    nv = 1 if v.ndim == 1 else v.shape[1]
    vb = to_field(v, ldv)
    ob = torch.full((nv, ldo), float("nan"), dtype=torch.float32, device="cuda")
    call("ibh_accumulate", dacc.handle, B._ptr(vb), nv, ldv, B._ptr(ob), ldo)
    return from_field(ob, dacc.n_output)


@pytest.mark.parametrize("n_out", [1, 255, 257, 4001])
def test_accumulate_synthetic(n_out):
    """k_accumulate (1 field), k_accumulate_rows<4> (2, 3, 4; 9 and 11 with a ragged last blockIdx.y) and <8> (5, 7, 8):
    rows of every length on the dwordx4 entry path and on the scalar path, weighted and unweighted, padded columns."""
    n_in = 300
    for weighted in (True, False):
        off, idx, w = ps.synthetic_csr(n_out, n_in, seed=n_out, weighted=weighted)
        if n_out > 1:
            ps.assert_paths_covered(off)
        dacc = _dacc(off, idx, w, n_in)
        for nv in (1, 2, 3, 4, 5, 7, 8, 9, 11):
            v = ps.seeded((n_in, nv), 10 + nv)
            got = _apply(dacc, v, n_in + 5, n_out + 3)
            ref, sc = ps.acc_ref(off, idx, w, v)
            _record("accumulate synthetic", ps.check(got, ref, sc, ps.BOUND_ACC, f"n_out={n_out} w={weighted} nv={nv}"))
        v = ps.seeded(n_in, 9)
        ref, sc = ps.acc_ref(off, idx, w, v)
        got = ibamd.to_host(dacc(ibamd.hip(v)))                     # the 1-D form of the public call
        _record("accumulate synthetic", ps.check(got, ref, sc, ps.BOUND_ACC, f"n_out={n_out} w={weighted} 1-D"))


@pytest.mark.parametrize("n_out,n_in,nvs", [(257, 64, (2, 3, 4, 5, 6, 7, 8)), (4001, 1000, (2, 3, 4, 5, 6, 7, 8)),
                                            (257, 300, (1, 3, 8, 11)), (4001, 4001, (1, 3, 8, 11))])
def test_diff_add(n_out, n_in, nvs):
    """out .+= acc(a .- b): the packed form (k_pack_diff8 + k_accumulate_packed_add<2..8>, n_out >= 4 n_in) and the
    unpacked one (k_accumulate_rows<8, ADD>), both against float64."""
    packed = n_out >= 4 * n_in
    off, idx, w = ps.synthetic_csr(n_out, n_in, seed=n_out + n_in)
    ps.assert_paths_covered(off)
    dacc = _dacc(off, idx, w, n_in)
    for nv in nvs:
        a, b, o0 = ps.seeded((n_in, nv), nv), ps.seeded((n_in, nv), nv + 20), ps.seeded((n_out, nv), nv + 40)
        ld, ldo = n_in + 3, n_out + 1
        ab, bb, ob = to_field(a, ld), to_field(b, ld), to_field(o0, ldo)
        call("ibh_accumulate_diff_add", dacc.handle, B._ptr(ab), B._ptr(bb), nv, ld, B._ptr(ob), ldo)
        ref, sc = ps.acc_ref(off, idx, w, a, v2=b, out0=o0)
        e = ps.check(from_field(ob, n_out), ref, sc, ps.BOUND_ACC, f"diff_add n_out={n_out} n_in={n_in} nv={nv}")
        _record("diff_add packed" if packed and 2 <= nv <= 8 else "diff_add rows", e)


@pytest.mark.parametrize("n_out,n_in", [(255, 300), (1020, 255)], ids=["rows", "packed"])
def test_row_walk_bits_against_the_model(n_out, n_in):
    """The order of the row walk (ibh_stencil_dev.h), which the float64 bound above cannot see: ``ibh_accumulate`` and
    ``ibh_accumulate_diff_add`` bit for bit against ``euler_mg_model.apply`` -- numpy Float32, product per entry, the first
    assigned, entry order; multiplications and additions only, so IEEE arithmetic without contraction leaves no room
    (tests/test_percell_steps.py::test_row_walk_model_is_sound).  (255, 300): ``diff_add`` through ``k_accumulate_rows<8,
    true>``; (1020, 255): ``n_out >= 4 n_in``, through ``k_pack_diff8`` + ``k_accumulate_packed_add<6>``."""
    import euler_mg_model as mg
    from euler_forms import same_bits
    host = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=f32))      # (same_bits takes tensors)
    for weighted in (True, False):
        off, idx, w = ps.synthetic_csr(n_out, n_in, seed=n_out, weighted=weighted)
        ps.assert_paths_covered(off)
        acc = Accumulator(csr=(off, idx, w), n_input=n_in)
        dacc = B.DeviceAccumulator(acc)
        for nv in (1, 3, 6):
            v = ps.seeded((n_in, nv), 10 + nv)
            model = mg.apply(acc, v)
            assert np.isfinite(model).all()
            same_bits(host(_apply(dacc, v, n_in + 5, n_out + 3)), host(model), f"accumulate n_out={n_out} w={weighted} nv={nv}")
        nv = 6                                             # (without weights both shapes take k_accumulate_rows<8, true>)
        a, b, o0 = ps.seeded((n_in, nv), nv), ps.seeded((n_in, nv), nv + 20), ps.seeded((n_out, nv), nv + 40)
        ld, ldo = n_in + 3, n_out + 1
        ab, bb, ob = to_field(a, ld), to_field(b, ld), to_field(o0, ldo)
        call("ibh_accumulate_diff_add", dacc.handle, B._ptr(ab), B._ptr(bb), nv, ld, B._ptr(ob), ldo)
        same_bits(host(from_field(ob, n_out)), host(o0 + mg.apply(acc, a - b)), f"diff_add n_out={n_out} n_in={n_in} w={weighted}")


def _octree_domain():
    from ibamd.mesher import Ball, Mesh
    msh = Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8,
               refinement_regions=[(Ball(np.array([-2.0, -2.0, -2.0]), 0.1), f32(0.1))])
    return ibamd.Domain(msh, max_partition_size=10 ** 9, boundaries=False)


@pytest.fixture(scope="module")
def adv_one(adv_mesh_coarse):
    return ibamd.Domain(adv_mesh_coarse, hypercube_families=ADV_FAMILIES, max_partition_size=10 ** 9)


@pytest.fixture(scope="module")
def octree_dom():
    return _octree_domain()


def test_transfer_operators(adv_one, octree_dom):
    """The coarsener and the prolongator of ``multigrid`` on the 2-D advection mesh and on a 3-D octree with level jumps,
    applied to a non-constant field with 1, 3 and 6 components, and ``diff_add`` of the prolongator (the step of FAS)."""
    for name, dom in (("adv", adv_one), ("octree", octree_dom)):
        (fine,) = dom.partitions.values()
        assert pc.levels(fine).max() >= 1, name                             # level jumps in the fine mesh
        _, pros, coas = ibamd.multigrid(dom, max_levels=1)
        for kind, acc in (("coarsener", coas[0]), ("prolongator", pros[0])):
            dacc = ibamd.to_backend(acc, ibamd.hip)
            assert acc.lengths.max() > 1, (name, kind)                     # a stencil, not a copy
            for nv in (1, 3, 6):
                v = ps.seeded((acc.n_input, nv), nv) + f32(0.5)
                got = ibamd.to_host(dacc(ibamd.hip(v if nv > 1 else v[:, 0])))
                ref, sc = ps.acc_ref(acc.off, acc.idx, acc.w, v if nv > 1 else v[:, 0])
                _record(f"{kind}", ps.check(got, ref, sc, ps.BOUND_ACC, f"{name} {kind} nv={nv}"))
                if nv > 1:
                    b, o0 = ps.seeded((acc.n_input, nv), nv + 7), ps.seeded((acc.n_output, nv), nv + 9)
                    out = ibamd.hip(o0)
                    dacc.diff_add(out, ibamd.hip(v), ibamd.hip(b))
                    ref, sc = ps.acc_ref(acc.off, acc.idx, acc.w, v, v2=b, out0=o0)
                    _record(f"{kind} diff_add", ps.check(ibamd.to_host(out), ref, sc, ps.BOUND_ACC,
                                                         f"{name} {kind} diff_add nv={nv}"))


def test_bc_interp_remap(adv_mesh, rae_mesh_small):
    """``ibh_bc_interp``: the only caller that passes ``remap`` (the stencil's donors go through ``image_domain``)."""
    seen = 0
    for name, msh, fam in (("adv", adv_mesh, ADV_FAMILIES), ("rae", rae_mesh_small, RAE_FAMILIES)):
        dom = ibamd.Domain(msh, hypercube_families=fam, max_partition_size=10 ** 9)
        nc = len(dom)
        for bname, parts in dom.boundaries.items():
            for ipart, b in parts.items():
                acc = b.image_interpolator
                if acc.n_output == 0:
                    continue
                db = ibamd.to_backend(b, ibamd.hip)
                for nv in (1, 3, 6):
                    a = ps.seeded((nc, nv), nv + 1) + f32(0.3)
                    ab = to_field(a, nc + 2)
                    ia = torch.full((nv, db.ng + 1), float("nan"), dtype=torch.float32, device="cuda")
                    call("ibh_bc_interp", db.handle, B._ptr(ab), nv, nc + 2, B._ptr(ia), db.ng + 1)
                    ref, sc = ps.acc_ref(acc.off, acc.idx, acc.w, a, remap=b.image_domain)
                    _record("bc_interp (remap)", ps.check(from_field(ia, db.ng), ref, sc, ps.BOUND_ACC,
                                                          f"{name} {bname} nv={nv}"))
                seen += 1
                assert not np.array_equal(b.image_domain, np.arange(b.image_domain.size)), "remap is the identity"
    assert seen >= 4


# ---------------------------------------------------------------------------------------------------------------------
# 2. Boundary conditions
# ---------------------------------------------------------------------------------------------------------------------
class SynthBoundary:
    """``ibh_bc_create`` straight from the arrays of a ``percell_steps.synthetic_boundary``: the donors go through a
    shuffled ``image_domain``."""

    def __init__(self, b, n, seed=0):
        perm = np.random.default_rng(seed).permutation(n).astype(np.int32)
        inv = np.empty(n, np.int32)
        inv[perm] = np.arange(n, dtype=np.int32)
        self.ng = int(b["ghost"].size)
        ghost = np.ascontiguousarray(np.concatenate([b["ghost"], [0]]), np.int32)          # (never empty arrays)
        gd = np.ascontiguousarray(np.concatenate([b["ghost_distances"], [1]]), f32)
        idist = np.ascontiguousarray(np.concatenate([b["image_distances"], [1]]), f32)
        off = np.ascontiguousarray(b["off"], np.int32)
        idx = np.ascontiguousarray(np.concatenate([inv[b["idx"]], [0]]), np.int32)
        w = np.ascontiguousarray(np.concatenate([b["w"], [0]]), f32)
        h = C.c_void_p()
        B._dev()
        _lib.call("ibh_bc_create", C.byref(h), self.ng, B._hptr(ghost), B._hptr(gd), B._hptr(idist), n, B._hptr(perm),
                  B._hptr(off), B._hptr(idx), B._hptr(w), 0)
        self.handle = h

    def __del__(self):
        if getattr(self, "handle", None):
            _lib.load().ibh_bc_destroy(self.handle)
            self.handle = None


class SynthSet:
    def __init__(self, bs, n):
        self.bcs = [SynthBoundary(b, n, seed=k) for k, b in enumerate(bs)]
        arr = (C.c_void_p * len(bs))(*[b.handle for b in self.bcs])
        m = np.asarray([b["mode"] for b in bs], np.int32)
        v = np.asarray([b["value"] for b in bs], f32)
        h = C.c_void_p()
        _lib.call("ibh_bcset_create", C.byref(h), len(bs), arr, B._hptr(m), B._hptr(v))
        self.handle = h
        ng, nl = C.c_int32(0), C.c_int32(0)
        _lib.call("ibh_bcset_info", h, C.byref(ng), C.byref(nl))
        self.n_ghost, self.n_levels, self.n_direct_levels = int(ng.value), int(nl.value) & 0xffff, int(nl.value) >> 16

    def apply(self, u):
        call("ibh_bcset_apply", self.handle, B._ptr(u))

    def __del__(self):
        if getattr(self, "handle", None):
            _lib.load().ibh_bcset_destroy(self.handle)
            self.handle = None


@pytest.fixture(scope="module")
def march_case(adv_one):
    """The one-partition advection case for ``step_advection``: partition, C, dt and a step field."""
    (part,) = adv_one.partitions.values()
    dpart = ibamd.to_backend(part, ibamd.hip)
    x = part.centers
    Ch = np.stack([1.0 + 0.3 * np.sin(3 * x[:, 1]), 0.8 + 0.2 * np.cos(2 * x[:, 0])], axis=1).astype(f32)
    u0 = ps.seeded(x.shape[0], 21) + np.sin(4 * x[:, 0]).astype(f32)
    return dict(dom=adv_one, part=part, dpart=dpart, n=x.shape[0], Ch=Ch, u0=u0, op=oracle_view(part))


def _step_with_set(mc, bcs, bs, what):
    """``step_advection(..., next_dt=...)`` with the set riding beside the time step: the field against ``bc_ref`` applied
    to the same step without boundary conditions, the next time step against the float64 reference."""
    dpart, n = mc["dpart"], mc["n"]
    Cd, u = ibamd.hip(mc["Ch"]), ibamd.hip(mc["u0"])
    dt = ibamd.timestep_advection(dpart, Cd, scale=0.75)
    plain = ibamd.to_host(ibamd.step_advection(dpart, u, Cd, dt))
    nxt = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    ibamd.step_advection(dpart, u, Cd, dt, bcs=bcs, out=out, next_dt=nxt, scale=0.6)
    ref, sc = ps.bc_ref(plain, bs)
    _record("bc sets in step_advection", ps.check(ibamd.to_host(out), ref, sc, ps.BOUND_BC, f"{what} in step_advection"))
    _record("dt beside the bc set", ps.check_dt(nxt.item(), ps.dt_ref(ps.dt_percell(mc["op"], mc["Ch"]), f64(f32(0.6))),
                                                f"{what}: next_dt"))


@pytest.mark.parametrize("name", ["dependent", "hazard", "direct", "hazard_later", "shared_ghost", "chain8", "empty_middle"])
def test_bcset_synthetic(march_case, name):
    """Each set forces one branch of ``ibh_bcset_create``; the level and direct-level counts say that it ran."""
    n = march_case["n"]
    bs, nlev, ndir = ps.synthetic_sets(n)[name]
    S = SynthSet(bs, n)
    assert (S.n_levels, S.n_direct_levels) == (nlev, ndir), (name, S.n_levels, S.n_direct_levels)
    assert S.n_ghost == sum(b["ghost"].size for b in bs)
    a = ps.seeded(n, 31)
    ref, sc = ps.bc_ref(a, bs)
    u = dvec(a)
    S.apply(u)
    _record("bc sets", ps.check(u.cpu().numpy(), ref, sc, ps.BOUND_BC, f"set {name}"))
    if name == "dependent":                       # the one-level answer is a different one
        merged, _ = ps.bc_ref(a, bs[:1])
        merged[bs[1]["ghost"]] = ps.bc_ref(a, bs[1:])[0][bs[1]["ghost"]]
        with pytest.raises(AssertionError):
            ps.check(merged, ref, sc, ps.BOUND_BC)
    if name == "shared_ghost":                    # cell 39: the later boundary wins
        first, _ = ps.bc_ref(a, bs[:1])
        assert abs(first[39] - ref[39]) > 1e-3 and abs(u.cpu().numpy()[39] - ref[39]) <= ps.BOUND_BC * sc[39]
    _step_with_set(march_case, S, bs, f"set {name}")


def _real_cases(adv_one):
    from ibamd.mesher import Ball, Mesh
    msh = Mesh(f32([-2, -2, -2]), f32([4, 4, 4]), block_size=8,
               refinement_regions=[(Ball(np.array([-2.0, -2.0, -2.0]), 0.1), f32(0.1))])
    fam = [("upper", [(1, True)]), ("lower", [(1, False)]), ("outlet", [(2, False), (2, True), (3, False), (3, True)])]
    oct3 = ibamd.Domain(msh, hypercube_families=fam, max_partition_size=10 ** 9)
    return (("adv", adv_one), ("octree", oct3))


def test_bc_real_boundaries(adv_one, march_case):
    """``ibh_bc_apply`` in both modes (1 and 3 fields) and ``BCSet.apply`` with the three-boundary set of
    test/advection.jl, on the 2-D advection mesh and a 3-D octree; the 2-D set inside ``step_advection`` as well."""
    specs = [("upper", 1.0), ("lower", 0.0), ("outlet", "copy")]
    for name, dom in _real_cases(adv_one):
        n = len(dom)
        assert all(dom.boundaries[nm][1].ghost_indices.size > 0 for nm, _ in specs), name
        a = ps.seeded((n, 3), 41) + f32(0.3)
        for bname in dom.boundaries:
            b = dom.boundaries[bname][1]
            db = ibamd.to_backend(b, ibamd.hip)
            for mode in (0, 1):
                for nv in (1, 3):
                    consts = f32([0.7, -1.2, 0.1])[:nv]
                    buf = to_field(a[:, :nv], n + 2)
                    call("ibh_bc_apply", db.handle, B._ptr(buf), nv, n + 2, mode, B._hptr(consts))
                    got = from_field(buf, n)
                    for v in range(nv):
                        ref, sc = ps.bc_ref(a[:, v], [ps.boundary_dict(b, mode, consts[v])])
                        _record("bc_apply", ps.check(got[:, v], ref, sc, ps.BOUND_BC, f"{name} {bname} mode {mode} field {v}"))
        bs = [ps.boundary_dict(dom.boundaries[nm][1], int(sp == "copy"), 0.0 if sp == "copy" else sp) for nm, sp in specs]
        bcs = ibamd.BCSet(dom, specs)
        assert bcs.n_levels >= 1 and bcs.n_ghost == sum(b["ghost"].size for b in bs)
        u = dvec(a[:, 0])
        bcs.apply(u)
        ref, sc = ps.bc_ref(a[:, 0], bs)
        _record("BCSet.apply", ps.check(u.cpu().numpy(), ref, sc, ps.BOUND_BC, f"{name} BCSet"))
        if name == "adv":
            _step_with_set(march_case, bcs, bs, "advection BCSet")


# ---------------------------------------------------------------------------------------------------------------------
# 3. Time step, cell by cell
# ---------------------------------------------------------------------------------------------------------------------
class DtCase:
    def __init__(self, part):
        self.part = part
        self.op = oracle_view(part)
        self.dpart = ibamd.to_backend(part, ibamd.hip)
        self.nc, self.nd = part.spacing.shape[0], part.ndims
        self.tiled = self.dpart.info["tiled"]
        self.M = [ps.dt_matrix(part, d) for d in range(self.nd)]

    def dt(self, C_, scale=1.0):
        out = ibamd.timestep_advection(self.dpart, ibamd.hip(C_), scale=scale)
        return float(out.cpu()[0])

    def probe_cells(self):
        if self.nc <= 4096:
            return np.arange(self.nc), None
        classes = {k: m for k, m in pc.cell_classes(self.part, block_classes=False).items() if k.startswith("side_")}
        cells = [np.nonzero(m)[0][:256] for m in classes.values()]
        bs = 8 ** self.nd
        if self.tiled:
            bases = [0, self.nc - bs]
        else:
            from ibamd import hostview
            bases = [int(b) for b in hostview.analyze2(self.part)["blocks"]["base"][[0, -1]]]
        pos = np.arange(bs)
        edge = np.zeros(bs, bool)
        for d in range(self.nd):
            x = (pos >> (3 * d)) & 7
            edge |= (x == 0) | (x == 7)
        for b in bases:
            cells.append(b + pos[edge])
        return np.unique(np.concatenate(cells)), classes

    def probe(self, cells, d, wide=None):
        """Device dt of every probe (one upload-free element write, two launches; one read-back for all)."""
        Cd = torch.zeros((self.nd, self.nc), dtype=torch.float32, device="cuda")
        out = torch.full((cells.size,), float("nan"), dtype=torch.float32, device="cuda")
        E = ps.dt_probe_inputs(self.part, cells, d, wide) if wide is not None and wide.any() else None
        B._stream()
        for i, c in enumerate(cells.tolist()):
            if E is not None and wide[i]:
                Cd[d].copy_(torch.from_numpy(E[:, i].astype(f32)))
            else:
                Cd[d, c] = 1.0
            _lib.call("ibh_timestep_advection", self.dpart.handle, B._ptr(Cd), self.nc, C.c_float(1.0),
                      C.c_void_p(out.data_ptr() + 4 * i))
            if E is not None and wide[i]:
                Cd[d].zero_()
            else:
                Cd[d, c] = 0.0
        return out.cpu().numpy().astype(f64)


@pytest.fixture(scope="module")
def dt_cases(adv_one, octree_dom, rae_mesh_small):
    out = {}
    (p,) = adv_one.partitions.values()
    out["adv"] = DtCase(p)
    (p,) = octree_dom.partitions.values()
    out["octree"] = DtCase(p)
    dom = ibamd.Domain(rae_mesh_small, hypercube_families=RAE_FAMILIES, max_partition_size=10 ** 9, boundaries=False)
    (p,) = dom.partitions.values()
    out["rae"] = DtCase(p)
    dom = ibamd.Domain(rae_mesh_small, hypercube_families=RAE_FAMILIES, max_partition_size=16384, boundaries=False,
                       only=[2])
    out["rae_skirt"] = DtCase(dom.partitions[2])
    return out


def test_dt_coverage(dt_cases):
    assert {c.tiled for c in dt_cases.values()} == {True, False}, {k: c.tiled for k, c in dt_cases.items()}
    assert {c.nd for c in dt_cases.values()} == {2, 3}
    assert dt_cases["octree"].dpart.info["sides_mirror"] > 0               # a mesh with mirror sides
    for k in ("sides_coarse", "sides_fine"):
        assert dt_cases["octree"].dpart.info[k] > 0 and dt_cases["rae"].dpart.info[k] > 0
    sk = pc.cell_classes(dt_cases["rae_skirt"].part, block_classes=False)
    assert sk["skirt"].sum() > 0 and sk["image"].sum() > 0                 # skirt fragments beside the image
    assert "skirt" not in pc.cell_classes(dt_cases["rae"].part, block_classes=False)


@pytest.mark.parametrize("name", ["adv", "octree", "rae", "rae_skirt"])
def test_dt_probes(dt_cases, name):
    """C_d = 1 at one cell and 0 elsewhere puts the reference's maximum at that cell (asserted from the float64 per-cell
    array; a probe for which it does not hold is widened to 0.25 at the face neighbours, and then it must): dt is that
    cell's value alone, at relative 4 ulp."""
    c = dt_cases[name]
    cells, classes = c.probe_cells()
    if classes is not None:
        for k, m in classes.items():
            assert np.isin(np.nonzero(m)[0][:256], cells).all(), k          # every side class is probed
    worst, nfail = 0.0, 0
    for d in range(c.nd):
        wide = np.zeros(cells.size, bool)
        refs = np.empty(cells.size)
        for lo in range(0, cells.size, 128):
            sl = slice(lo, lo + 128)
            per = ps.dt_probe_refs(c.M[d], c.part, cells[sl], d)
            bad = per[cells[sl], np.arange(per.shape[1])] < per.max(axis=0)
            if bad.any():
                nfail += int(bad.sum())
                wide[sl] = bad
                per = ps.dt_probe_refs(c.M[d], c.part, cells[sl], d, wide[sl])
                assert np.all(per[cells[sl], np.arange(per.shape[1])] == per.max(axis=0)), (name, d, cells[sl][bad])
            refs[sl] = [ps.dt_ref(per[:, i]) for i in range(per.shape[1])]
        got = c.probe(cells, d, wide)
        assert not np.isnan(got).any()
        err = np.abs(got - refs) / np.abs(refs)
        i = int(np.argmax(err))
        assert err[i] <= ps.BOUND_DT, (f"{name} dim {d}: dt of the probe at cell {cells[i]} is {got[i]!r}, reference "
                                       f"{refs[i]!r} ({err[i] / ps.ULP:.1f} ulp); {int((err > ps.BOUND_DT).sum())} probes fail")
        worst = max(worst, err[i])
    assert nfail == 0, f"{name}: the plain probe's maximum left its cell {nfail} times"
    _record(f"dt probes {name} ({cells.size} cells x {c.nd})", worst)


def _smooth_C(c):
    x = c.part.centers
    C0 = np.stack([f32(1) + f32(0.5) * np.sin(3 * x[:, d] + d).astype(f32) + f32(0.2) * np.cos(5 * x[:, (d + 1) % c.nd])
                   for d in range(c.nd)], axis=1).astype(f32)
    assert (C0 > 0).all()
    return C0


DT_KEEPS_FMAXF = ("dt_partial_wg keeps fmaxf: with ibh_max (and the maximum seeded below every value) the march of bench.py "
                  "measured 30.6 - 31.4 k against 33.0 - 33.2 k Mcells*steps/s (three alternating runs per build, -6.5 %, "
                  "spread within a build 1 - 2 %); DESIGN.md section 5")


@pytest.mark.parametrize("name", ["adv", "octree", "rae", "rae_skirt"])
def test_dt_inputs(dt_cases, name):
    """A smooth non-uniform positive C, with scale = 1 and scale != 1."""
    c = dt_cases[name]
    C0 = _smooth_C(c)
    for what, scale in (("positive", 1.0), ("scaled", 0.35)):
        ref = ps.dt_ref(ps.dt_percell(c.op, C0), f64(f32(scale)))
        got = c.dt(C0, scale)
        _record(f"dt {what}", ps.check_dt(got, ref, f"{name} {what}"))


@pytest.mark.parametrize("name", ["adv", "octree", "rae_skirt"])
def test_dt_all_negative(dt_cases, name):
    """Julia's maximum has no floor at zero: an all-negative C gives a negative dt (a maximum that starts at 0 gives
    0.5 / 0 = Inf)."""
    c = dt_cases[name]
    C0 = -_smooth_C(c)
    ref = ps.dt_ref(ps.dt_percell(c.op, C0))
    assert math.isfinite(ref) and ref < 0
    _record("dt negative", ps.check_dt(c.dt(C0), ref, f"{name} negative"))


@pytest.mark.xfail(strict=True, reason=DT_KEEPS_FMAXF)
@pytest.mark.parametrize("name", ["adv", "octree"])
def test_dt_nan(dt_cases, name):
    """Julia's maximum propagates NaN: one NaN in C gives dt = NaN.  fmaxf drops it and dt is finite."""
    c = dt_cases[name]
    Cn = _smooth_C(c)
    Cn[c.nc // 3, c.nd - 1] = np.nan
    assert math.isnan(ps.dt_ref(ps.dt_percell(c.op, Cn)))
    ps.check_dt(c.dt(Cn), np.nan, f"{name}: one NaN in C")


# ---------------------------------------------------------------------------------------------------------------------
# 4. Reductions and updates
# ---------------------------------------------------------------------------------------------------------------------
def _dbl():
    return torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("n", ps.REDUCTION_SIZES)
def test_sums(n):
    """ibh_sumsq, ibh_dot, ibh_axpy_clamped_sumsq and the norm halves of ibh_fas_update against math.fsum, each twice in a
    row into the same output (a stale partial or a missing reset would show in the second)."""
    xs = [ps.seeded(n, 1), ps.seeded(n, 2, -0.5, 0.25)]
    ys = [ps.seeded(n, 3), ps.seeded(n, 4)]
    out = _dbl()
    for x in xs:
        call("ibh_sumsq", n, B._ptr(keep(x)), B._ptr(out))
        _record("sums", ps.check_sum(out.item(), x, what=f"sumsq n={n}"))
    for x, y in zip(xs, ys):
        call("ibh_dot", n, B._ptr(keep(x)), B._ptr(keep(y)), B._ptr(out))
        _record("sums", ps.check_sum(out.item(), x, y, what=f"dot n={n}"))
    for x, y in zip(xs, ys):
        q = dvec(y)
        call("ibh_axpy_clamped_sumsq", n, C.c_float(0.3), B._ptr(keep(x)), B._ptr(q), B._ptr(out))
        _record("sums", ps.check_sum(out.item(), x, what=f"axpy_clamped_sumsq n={n}"))
        ref, sc, _ = ps.fas_ref(0.3, x, None, y)
        _record("updates", ps.check(q.cpu().numpy(), ref, sc, ps.BOUND_EW, f"axpy_clamped_sumsq q n={n}"))
    for src in (False, True):
        for upd in (False, True):
            for x, y in zip(xs, ys):
                s = ps.seeded(n, 5) if src else None
                q = dvec(y) if upd else None
                call("ibh_fas_update", n, C.c_float(0.3), B._ptr(keep(x)), B._ptr(keep(s) if src else None),
                     B._ptr(q), B._ptr(out))
                ref, sc, rr = ps.fas_ref(0.3, x, s, y if upd else None)
                _record("sums", ps.check_sum(out.item(), rr, what=f"fas_update src={src} upd={upd} n={n}"))
                if upd:
                    _record("updates", ps.check(q.cpu().numpy(), ref, sc, ps.BOUND_EW, f"fas q src={src} n={n}"))


@pytest.mark.parametrize("n", [1, 65, 257, 1000, 256 * 2048 + 3])
@pytest.mark.parametrize("omega", [-0.5, 0.0, 0.3, 1.0, 1.7, float("nan")])
def test_clamped_updates(n, omega):
    """q += clamp(omega, 0, 1) (r [+ src]) in its four entries; Julia's clamp keeps a NaN omega."""
    r, s, q0 = ps.seeded(n, 1), ps.seeded(n, 2), ps.seeded(n, 3)
    out = _dbl()
    for name, src, fn in (
            ("ibh_axpy_clamped", None, lambda q: call("ibh_axpy_clamped", n, C.c_float(omega), B._ptr(keep(r)), B._ptr(q))),
            ("ibh_axpy_clamped_sumsq", None, lambda q: call("ibh_axpy_clamped_sumsq", n, C.c_float(omega), B._ptr(keep(r)),
                                                            B._ptr(q), B._ptr(out))),
            ("ibh_fas_update <0,1,0>", None, lambda q: call("ibh_fas_update", n, C.c_float(omega), B._ptr(keep(r)),
                                                            C.c_void_p(None), B._ptr(q), C.c_void_p(None))),
            ("ibh_fas_update <1,1,0>", s, lambda q: call("ibh_fas_update", n, C.c_float(omega), B._ptr(keep(r)),
                                                         B._ptr(keep(s)), B._ptr(q), C.c_void_p(None)))):
        q = dvec(q0)
        fn(q)
        ref, sc, _ = ps.fas_ref(omega, r, src, q0)
        _record("updates", ps.check(q.cpu().numpy(), ref, sc, ps.BOUND_EW, f"{name} omega={omega} n={n}"))


@pytest.mark.parametrize("n", [1, 65, 257, 1000, 256 * 2048 + 3])
def test_elementwise_updates(n):
    x, y, r = ps.seeded(n, 1), ps.seeded(n, 2), ps.seeded(n, 3)
    x64, y64, r64 = ps.to64(x, y, r)
    a = f32(-0.37)
    dy = dvec(y)
    call("ibh_axpy", n, C.c_float(a), B._ptr(keep(x)), B._ptr(dy))
    ref = f64(a) * x64 + y64
    _record("updates", ps.check(dy.cpu().numpy(), ref, np.abs(ref) + abs(f64(a)) * np.abs(x64) + np.abs(y64), ps.BOUND_EW,
                                f"axpy n={n}"))
    dt = f32(0.0123)
    o = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    call("ibh_update_dev", n, B._ptr(keep(np.array([dt]))), B._ptr(keep(x)), B._ptr(keep(r)), B._ptr(o))
    ref = x64 + f64(dt) * r64
    _record("updates", ps.check(o.cpu().numpy(), ref, np.abs(ref) + np.abs(x64) + f64(dt) * np.abs(r64), ps.BOUND_EW,
                                f"update_dev n={n}"))
    dots = np.array([0.731, 2.25])
    eps = f32(ps.EPS32)
    dx, dr = dvec(x), dvec(r)
    s, As = ps.seeded(n, 4), ps.seeded(n, 5)
    call("ibh_pi_update", n, B._ptr(keep(dots, torch.float64)), C.c_float(eps), B._ptr(keep(s)), B._ptr(keep(As)),
         B._ptr(dx), B._ptr(dr))
    alpha = dots[0] / (dots[1] + f64(eps))
    for got, base, inc, sign, what in ((dx, x64, s, 1.0, "x"), (dr, r64, As, -1.0, "r")):
        ref = base + sign * alpha * inc.astype(f64)
        _record("updates", ps.check(got.cpu().numpy(), ref, np.abs(ref) + np.abs(base) + abs(alpha) * np.abs(inc.astype(f64)),
                                    ps.BOUND_EW, f"pi_update {what} n={n}"))
    mx = f32(0.83)
    o = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    call("ibh_pi_normalize", n, B._ptr(keep(r)), B._ptr(keep(np.array([mx]))), C.c_float(eps), B._ptr(o))
    ref = r64 / (f64(eps) + f64(mx))
    _record("updates", ps.check(o.cpu().numpy(), ref, 2 * np.abs(ref), ps.BOUND_EW, f"pi_normalize n={n}"))


def _maxabs(a):
    out = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    call("ibh_maxabs", a.size, B._ptr(keep(a)), B._ptr(out))
    return out.cpu().numpy()[0]


@pytest.mark.parametrize("n", ps.REDUCTION_SIZES)
def test_maxabs(n):
    """maximum(abs, a): exact, with the largest element first, last, at 63 / 64 and in the last partial workgroup; twice
    into the same output; -0.0, Inf and NaN (Julia's maximum propagates it)."""
    base = ps.seeded(n, 6)
    places = sorted({0, n - 1, min(63, n - 1), min(64, n - 1), max(0, n - 1 - (n - 1) % 256)})
    out = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    for p in places:
        for big in (f32(-3.25), f32(1.5)):                      # the second call into the same output has the smaller maximum
            a = base.copy()
            a[p] = big
            call("ibh_maxabs", n, B._ptr(keep(a)), B._ptr(out))
            assert out.cpu().numpy()[0] == abs(big), (n, p, big)
    z = np.full(n, -0.0, f32)
    got = _maxabs(z)
    assert got == 0.0 and not np.signbit(got)
    a = base.copy()
    a[n // 2] = -np.inf
    assert _maxabs(a) == np.inf
    a[n - 1] = np.nan
    assert np.isnan(_maxabs(a)), "maxabs dropped a NaN"
    a = base.copy()
    a[0] = np.nan
    assert np.isnan(_maxabs(a)), "maxabs dropped a NaN"


@pytest.mark.parametrize("n", ps.EW_REDUCE_TOTALS)
def test_ew_reduce(n):
    """sum / maximum / minimum of a flat array (``ibh_ew_reduce``), each twice into the same output.  The extremes are
    exact, with the extreme element at the places of ``test_maxabs``; the Float32 sum is within ``check_sum32``'s bound of
    ``math.fsum`` (depth from the grid formula; the Float32 model of the same order measures 0.06 of the bound)."""
    out = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")
    for x in (ps.seeded(n, 1), ps.seeded(n, 2, 0.0, 1.0)):
        call("ibh_ew_reduce", H.SUM, n, B._ptr(keep(x)), B._ptr(out))
        _record("ew_reduce sum / bound", ps.check_sum32(out.item(), x, f"ew_reduce sum n={n}"))
    d = keep(ps.seeded(n, 6))
    for op, sign in ((H.MAX, 1.0), (H.MIN, -1.0)):
        for p in ps.extreme_places(n):
            old = d[p].item()
            for big in (3.25, 1.5):                                 # the second call into the same output is less extreme
                d[p] = sign * big                                   # (both exact in Float32)
                call("ibh_ew_reduce", op, n, B._ptr(d), B._ptr(out))
                assert out.item() == sign * big, (op, n, p, big)
            d[p] = old


@pytest.mark.parametrize("n", [256 * 1024 + 1, 256 * 2048 + 3])
def test_dot_reproducible(n):
    """Two calls of ``ibh_dot`` on the same input give the same bits: workgroup sums in an array and one workgroup that adds
    them in a fixed order (no arrival order)."""
    x, y = keep(ps.seeded(n, 1)), keep(ps.seeded(n, 3))
    o1, o2 = _dbl(), _dbl()
    call("ibh_dot", n, B._ptr(x), B._ptr(y), B._ptr(o1))
    call("ibh_dot", n, B._ptr(x), B._ptr(y), B._ptr(o2))
    a, b = o1.cpu().numpy().view(np.uint64)[0], o2.cpu().numpy().view(np.uint64)[0]
    assert a == b, (n, hex(a), hex(b))


# ---------------------------------------------------------------------------------------------------------------------
# 5. Point-implicit blocks
# ---------------------------------------------------------------------------------------------------------------------
def _blocks_to_dev(A):
    """(n, M, M) [p, k, i] -> device (M, M, n) [i, k, p]: D[p + n (k + M i)]."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(A, f32).transpose(2, 1, 0))).cuda()


def _blocks_to_host(D):
    return np.ascontiguousarray(D.cpu().numpy().transpose(2, 1, 0))


@pytest.mark.parametrize("M", [2, 3, 4, 5, 6, 7, 8])
def test_pinv_blocks(M):
    for n in (1, 63, 65, 1000):
        A, kind = ps.pinv_blocks(M, n)
        D = _blocks_to_dev(A)
        call("ibh_pi_invert_blocks", n, M, B._ptr(D))
        got = _blocks_to_host(D)
        P, bins, _ = ps.pinv_ref(A)
        for k, e in ps.pinv_binned(ps.pinv_error(got, P), bins).items():
            _record(f"pinv bin {k}", e)
        ps.check_pinv(got, A, f"pinv M={M} n={n}")


@pytest.mark.parametrize("M", [1, 2, 3, 4, 5, 6, 7, 8])
def test_apply_blocks(M):
    for n in (1, 65, 257, 1000):
        if M == 1:
            D, v = ps.seeded(n, 1), ps.seeded(n, 2)
            dD, dv = dvec(D), dvec(v)
        else:
            D, v = ps.seeded((n, M, M), M), ps.seeded((n, M), M + 10)
            dD, dv = _blocks_to_dev(D), dvec(v.T)
        o = torch.full(dv.shape, float("nan"), dtype=torch.float32, device="cuda")
        call("ibh_pi_apply_blocks", n, M, B._ptr(dD), B._ptr(dv), B._ptr(o))
        ref, sc = ps.apply_ref(D, v)
        got = o.cpu().numpy() if M == 1 else o.cpu().numpy().T
        _record("apply_blocks", ps.check(got, ref, sc, ps.BOUND_APPLY, f"apply M={M} n={n}"))


@pytest.mark.parametrize("n", [65, 1000])
def test_pi_elementwise(n):
    h = f32(1e-2)
    h64 = f64(h)
    x, v = ps.seeded(n, 1), ps.seeded(n, 2)
    x64, v64 = ps.to64(x, v)
    o = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    call("ibh_pi_perturb", n, B._ptr(keep(x)), B._ptr(keep(v)), C.c_float(h), B._ptr(o))
    ref = x64 + v64 * h64
    _record("pi elementwise", ps.check(o.cpu().numpy(), ref, np.abs(ref) + np.abs(x64) + np.abs(v64) * h64, ps.BOUND_EW,
                                       "perturb"))
    o.fill_(float("nan"))
    call("ibh_pi_fd", n, B._ptr(keep(x)), B._ptr(keep(v)), C.c_float(h), B._ptr(o))
    ref = (x64 - v64) / h64
    _record("pi elementwise", ps.check(o.cpu().numpy(), ref, np.abs(ref) + (np.abs(x64) + np.abs(v64)) / h64, ps.BOUND_EW,
                                       "fd"))
    d = f32(7.0)
    ds = dvec(x)
    call("ibh_pi_div_scalar", n, C.c_float(d), B._ptr(ds))
    ref = x64 / f64(d)
    _record("pi elementwise", ps.check(ds.cpu().numpy(), ref, 2 * np.abs(ref), ps.BOUND_EW, "div_scalar"))
    Dg = ps.seeded(n, 3, 0.5, 2.0)
    dD = dvec(Dg)
    call("ibh_pi_invert_blocks", n, 1, B._ptr(dD))
    ref = 1.0 / (ps.EPS32 + Dg.astype(f64))
    _record("pi elementwise", ps.check(dD.cpu().numpy(), ref, 2 * np.abs(ref), ps.BOUND_EW, "invert_diag"))
    for nv in (1, 3, 5):                      # i % n crosses columns away from a workgroup boundary
        fxb, fx, s0 = ps.seeded((nv, n), nv), ps.seeded((nv, n), nv + 1), ps.seeded((nv, n), nv + 2)
        z = ps.splitmix_signs(n, 99)
        dsum = dvec(s0)
        call("ibh_pi_hutch_accum", n, nv, B._ptr(keep(fxb)), B._ptr(keep(fx)), B._ptr(keep(z)), C.c_float(h), B._ptr(dsum))
        a, b, s64 = ps.to64(fxb, fx, s0)
        ref = s64 + z.astype(f64)[None, :] * ((a - b) / h64)
        _record("pi elementwise", ps.check(dsum.cpu().numpy(), ref, np.abs(ref) + np.abs(s64) + (np.abs(a) + np.abs(b)) / h64,
                                           ps.BOUND_EW, f"hutch_accum nv={nv}"))


@pytest.mark.parametrize("n,seed", [(1, 0), (65, 1), (1000, 12345), (256 * 4096 + 7, 2 ** 63 + 11)])
def test_rademacher(n, seed):
    z = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    call("ibh_pi_rademacher", n, C.c_uint64(seed), B._ptr(z))
    got = z.cpu().numpy()
    assert np.isin(got, (-1.0, 1.0)).all()
    assert np.array_equal(got, ps.splitmix_signs(n, seed))
