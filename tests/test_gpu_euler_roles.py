"""Cell roles in the Euler march on the device -- ``restrict_euler(roles=...)``, ``forcing_roles``, ``sumsq_roles``,
``EulerMarch(roles=...)``, ``MultigridMarch(roles=...)`` -- bit for bit against the compositions that define them (the library's
own unmasked launches around a select), the sums against float64, and the cycle with roles written out, captured in a graph
and converging on the airfoil.  The definition: tests/euler_roles_model.py; hierarchies and helpers: tests/test_gpu_euler_mg.py.

Roles in the transfer tests are seeded random ones, about a third of each kind, and every masked row of ``R`` and ``S`` holds
NaN: a kernel that multiplied by a mask instead of selecting would show it."""
import numpy as np
import pytest
import torch

import euler_forms as ef
import euler_mg_model as mg
import ibamd
import percell_steps as ps
from conftest import RAE_FAMILIES
from euler_forms import FLUID, NAN, padded, same_bits
from ibamd import _lib
from ibamd import backend as B
from ibamd.hiparray import HipArray as H
from ibamd.solver import DualTimeMarch, EulerMarch, MultigridMarch, rk_stages
from test_gpu_euler_mg import TRANSFERS, Hierarchy, adv, compact, corner, flow_bcs, hier, ragged, rows  # noqa: F401

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def random_roles(n, seed=11):
    r = np.random.default_rng(seed).integers(0, 3, n).astype(np.uint8)
    return r, torch.from_numpy(r).cuda()


def poisoned(X, rd):
    """``X`` with NaN in every row that is not fluid."""
    out = B.colmajor_empty(*X.shape)
    out.copy_(X)
    out[rd != 0] = NAN
    return out


def masked(X, rd):
    """``X`` in fluid rows, +0 elsewhere: the select, as a compact column-major array."""
    out = B.colmajor_empty(*X.shape)
    out.copy_(torch.where((rd == 0)[:, None], X, torch.zeros((), dtype=torch.float32, device=X.device)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1: the restriction with roles
# ---------------------------------------------------------------------------------------------------------------------
def check_restrict_roles(acc, P, R, S, what, pads=True):
    nf, n_out, nv = acc.n_input, acc.n_output, P.shape[1]
    roles, rd = random_roles(nf)
    assert all((roles == k).sum() > nf // 5 for k in (0, 1, 2))
    Rn, Sn = poisoned(R, rd), poisoned(S, rd)
    plain_P, _ = ibamd.restrict_euler(acc, P, R, S, FLUID)
    for with_S in (True, False):
        tag = f"{what} S={'given' if with_S else 'NULL'}"
        t = masked((H(R) + H(S)).t if with_S else R, rd)
        ref_P, ref_D = ibamd.restrict_euler(acc, P, t, None, FLUID)
        oP, oD = B.colmajor_empty(n_out, nv), B.colmajor_empty(n_out, nv)
        oP.fill_(NAN)
        oD.fill_(NAN)
        got = ibamd.restrict_euler(acc, P, Rn, Sn if with_S else None, FLUID, out=oP, out_D=oD, roles=rd)
        assert got[0] is oP and got[1] is oD
        same_bits(oD, ref_D, tag + " D_c")
        same_bits(oP, ref_P, tag + " P_c")
        same_bits(oP, plain_P, tag + " P_c is the unmasked entry's")
        assert not torch.isnan(oD).any(), tag + ": a masked NaN reached D_c"
        if pads:     # padded leading dimensions, every array its own, and nothing written past the rows
            pp = [padded(nf, nv, pad) for pad in (13, 5, 7)]
            for p, src in zip(pp, (P, Rn, Sn)):
                p.copy_(src)
            baseP = torch.full((nv, n_out + 29), NAN, dtype=torch.float32, device="cuda")
            baseD = torch.full((nv, n_out + 3), NAN, dtype=torch.float32, device="cuda")
            ibamd.restrict_euler(acc, pp[0], pp[1], pp[2] if with_S else None, FLUID, out=baseP.T[:n_out], out_D=baseD.T[:n_out],
                                 roles=rd)
            same_bits(compact(baseP.T[:n_out]), ref_P, tag + " P_c padded")
            same_bits(compact(baseD.T[:n_out]), ref_D, tag + " D_c padded")
            assert torch.isnan(baseP[:, n_out:]).all() and torch.isnan(baseD[:, n_out:]).all()
        # every row fluid: ibh_restrict_euler outright
        fluid = torch.zeros(nf, dtype=torch.uint8, device="cuda")
        Sx = S if with_S else None
        all_P, all_D = ibamd.restrict_euler(acc, P, R, Sx, FLUID, roles=fluid)
        un_P, un_D = ibamd.restrict_euler(acc, P, R, Sx, FLUID)
        same_bits(all_P, un_P, tag + " all fluid P_c")
        same_bits(all_D, un_D, tag + " all fluid D_c")
    return ref_D


@pytest.mark.parametrize("mesh,l", TRANSFERS, ids=[f"{m}{l}" for m, l in TRANSFERS])
def test_restrict_roles_bit_for_bit(hier, mesh, l):
    h = hier[mesh]
    P = h.state(l, "transonic")
    R = ef.residual(h.dparts[l], P, "hll", 0)
    S = ibamd.dual_source(P, h.state(l, "transonic", seed=9), 1.7e3, -4.0e2, FLUID)
    D = check_restrict_roles(h.coarseners[l], P, R, S, f"{mesh} level {l}")
    assert np.isfinite(ibamd.to_host(D)).all() and ibamd.to_host(D).any()


@pytest.mark.parametrize("nd,n_out,n_in", [(2, 1000, 333), (3, 777, 2100), (3, 4096 * 256 + 77, 2048 * 256 + 55)],
                         ids=["2d", "3d", "3d_grid_stride"])
def test_restrict_roles_on_ragged_rows(nd, n_out, n_in):
    """The synthetic operators of tests/test_gpu_euler_mg.py: rows of 0 .. 12 entries on and off 16-byte boundaries, and the
    one with rows of 0 .. 5 entries and more output rows than one pass of the grid."""
    acc = ragged(n_out, n_in)
    P, R = rows(n_in, nd, 5)
    _, S = rows(n_in, nd, 6)
    check_restrict_roles(acc, P, R, S, f"ragged {nd}-D", pads=n_out < 10 ** 5)


# ---------------------------------------------------------------------------------------------------------------------
# 2: the forcing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nv", [(1, 4), (255, 4), (257, 5), (976, 4), (4096 * 256 + 77, 5), (1000, 1), (1000, 8)])
def test_forcing_roles_bit_for_bit(n, nv):
    """``D .- R`` (the broadcast) followed by the select, in place; padded leading dimensions; more rows than one pass."""
    rng = np.random.default_rng(n + nv)
    D0, R = (ibamd.hip(rng.normal(size=(n, nv)).astype(f32) * f32(1e3)) for _ in range(2))
    roles, rd = random_roles(n, seed=n)
    ref = masked((H(D0) - H(R)).t, rd)
    Rn = poisoned(R, rd)
    D = poisoned(D0, rd)
    assert ibamd.forcing_roles(D, Rn, rd) is D
    same_bits(D, ref, f"forcing n={n} nv={nv}")
    assert not torch.isnan(D).any() and not torch.signbit(D[rd != 0]).any()
    base = torch.full((nv, n + 13), NAN, dtype=torch.float32, device="cuda")
    Dp, Rp = base.T[:n], padded(n, nv, 5)
    Dp.copy_(D0)
    Rp.copy_(Rn)
    ibamd.forcing_roles(Dp, Rp, rd)
    same_bits(compact(Dp), ref, f"forcing padded n={n} nv={nv}")
    assert torch.isnan(base[:, n:]).all()
    fluid = torch.zeros(n, dtype=torch.uint8, device="cuda")
    Df = D0.clone()
    ibamd.forcing_roles(Df, R, fluid)
    same_bits(Df, (H(D0) - H(R)).t, "forcing, all fluid")


# ---------------------------------------------------------------------------------------------------------------------
# 3: the sums
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [1, 4, 5])
@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 1000, 256 * 256 + 3, 256 * 256 * 3 + 77])
def test_sumsq_roles_against_float64(n, nv):
    """Per column against ``math.fsum`` at the bound of ``ibh_sumsq``'s test (``percell_steps.BOUND_SUM``), with NaN in the
    masked rows: one wave, one workgroup and its neighbours, several workgroups, more rows than one pass of the 256
    workgroups of a column; compact and padded; all-solid roles give zeros; ``out`` is assigned."""
    rng = np.random.default_rng(n * 8 + nv)
    x = (rng.normal(size=(n, nv)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))).astype(f32)
    roles, rd = random_roles(n, seed=n + 1)
    xd = poisoned(ibamd.hip(x) if nv > 1 else ibamd.hip(x).reshape(n, 1), rd)
    xp = padded(n, nv, 11)
    xp.copy_(xd)
    for what, arr in (("compact", xd), ("padded", xp)) + ((("vector", xd[:, 0].contiguous()),) if nv == 1 else ()):
        out = torch.full((nv,), NAN, dtype=torch.float64, device="cuda")
        assert ibamd.sumsq_roles(arr, rd, out=out) is out
        got = out.cpu().numpy()
        for v in range(nv):
            ps.check_sum(got[v], x[roles == 0, v], what=f"sumsq_roles {what} n={n} nv={nv} column {v}")
    solid = torch.full((n,), 2, dtype=torch.uint8, device="cuda")
    z = ibamd.sumsq_roles(xd, solid)
    assert z.dtype == torch.float64 and z.shape == (nv,) and not z.cpu().numpy().any()
    # every row fluid, no NaN: ibh_sumsq of each column, which shares the scheme but not the grid
    clean = ibamd.hip(x) if nv > 1 else ibamd.hip(x).reshape(n, 1)
    got = ibamd.sumsq_roles(clean, torch.zeros(n, dtype=torch.uint8, device="cuda")).cpu().numpy()
    for v in range(nv):
        ps.check_sum(got[v], x[:, v], what=f"sumsq_roles all fluid n={n} column {v}")


def test_python_argument_checks():
    P, R = rows(100, 2, 5)
    _, rd = random_roles(100)
    with pytest.raises(ValueError, match="roles has 99 entries"):
        ibamd.sumsq_roles(R, rd[:99])
    with pytest.raises(TypeError, match="uint8"):
        ibamd.sumsq_roles(R, rd.to(torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        ibamd.sumsq_roles(R, rd, out=torch.zeros(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="more than 8 columns"):
        ibamd.forcing_roles(B.colmajor_empty(100, 9), B.colmajor_empty(100, 9), rd)
    with pytest.raises(ValueError, match="R must be"):
        ibamd.forcing_roles(B.colmajor_empty(100, 4), B.colmajor_empty(100, 5), rd)
    with pytest.raises(_lib.IbhError, match="ibh_forcing_roles: .*may not alias"):
        ibamd.forcing_roles(R, R, rd)
    z = ibamd.sumsq_roles(B.colmajor_empty(0, 4), torch.zeros(0, dtype=torch.uint8, device="cuda"))
    assert z.shape == (4,) and not z.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------------------------------
# 4: the marches on the airfoil
# ---------------------------------------------------------------------------------------------------------------------
class Airfoil(Hierarchy):
    """``rae_mesh_small`` as one partition with two coarser levels, the far field and the slip wall on every level, the roles
    of every level (``cell_roles`` of its own domain) and the free stream as the state of the solid rows."""

    def __init__(self, mesh):
        from test_euler_mg_model import conv_far
        doms, coa, pro = mg.hierarchy(mesh, 2, hypercube_families=RAE_FAMILIES)
        self.far = [float(x) for x in conv_far()]
        super().__init__(doms, coa, pro, [flow_bcs(d, self.far, "farfield", ("wall",)) for d in doms])
        self.host_roles = [ibamd.cell_roles(d) for d in doms]
        self.roles = [ibamd.Roles(p, r[p.domain], self.far) for p, r in zip(self.parts, self.host_roles)]
        self.start = ibamd.hip(np.tile(f32(self.far), (len(doms[0]), 1)))
        self.bcs[0](self.start)


@pytest.fixture(scope="module")
def rae(rae_mesh_small):
    return Airfoil(rae_mesh_small)


def test_roles_on_the_device(rae):
    for r, host, counts in zip(rae.roles, rae.host_roles, [(33374, 1976, 1770), (8034, 958, 288), (1859, 457, 4)]):
        assert r.counts == counts and r.n_solid == counts[2] and r.roles.dtype == torch.uint8
        assert np.array_equal(r.roles.cpu().numpy(), host) and np.array_equal(r.solid.cpu().numpy(), np.nonzero(host == 2)[0])
        assert r.solid.dtype == torch.int32 and r.solid_rows.shape == (counts[2], 4)
        assert np.array_equal(ibamd.to_host(r.solid_rows), np.tile(f32(rae.far), (counts[2], 1)))
    P = rae.state(0)
    keep = P.clone()
    assert rae.roles[0].blank(P) is P
    solid = rae.host_roles[0] == 2
    got, ref = ibamd.to_host(P), ibamd.to_host(keep)
    assert (got[solid] == f32(rae.far)).all() and np.array_equal(got[~solid], ref[~solid])


@pytest.mark.parametrize("stages", [1, 3])
def test_euler_march_blanks_the_solid_rows(rae, stages, monkeypatch):
    """One step from a disturbed state.  With one stage the blank is the step's last call: the solid rows equal
    ``solid_state`` exactly and every other row the march without roles, bit for bit.  With three stages the later sweeps read
    the blanked rows, and rows near the body may differ from the plain march: there the solid rows and the calls are
    asserted, and the number of rows that differ is printed."""
    dpart, bcs, roles = rae.dparts[0], rae.bcs[0], rae.roles[0]
    P0 = rae.state(0, "transonic")
    bcs(P0)
    kw = dict(fluid=FLUID, scale=0.3, bcs=bcs, local_dt=True, stages=stages)
    plain, mine = EulerMarch(dpart, **kw), EulerMarch(dpart, roles=roles, **kw)
    names = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    got = mine.step(P0)
    with_roles, names[:] = [n for n in names if n != "ibh_set_stream"], []
    ref = plain.step(P0)
    without = [n for n in names if n != "ibh_set_stream"]
    monkeypatch.undo()
    assert with_roles.count("ibh_scatter_rows") == stages and "ibh_scatter_rows" not in without
    assert [n for n in with_roles if n != "ibh_scatter_rows"] == without      # one launch more per stage, nothing else
    g, r = ibamd.to_host(got), ibamd.to_host(ref)
    solid = rae.host_roles[0] == 2
    assert (g[solid] == f32(rae.far)).all() and np.isfinite(g).all()
    if stages == 1:
        assert np.array_equal(g[~solid].view(np.uint32), r[~solid].view(np.uint32))
    else:
        fluid = rae.host_roles[0] == 0
        print(f"stages={stages}: {np.count_nonzero((g != r).any(axis=1) & ~solid)} non-solid rows differ from the plain march, "
              f"{np.count_nonzero((g != r).any(axis=1) & fluid)} of them fluid")
    # the norms: fluid rows only, per column, without a read-back
    n = mine.residual_norms(got)
    assert n is mine._norms and n.dtype == torch.float64 and n.shape == (4,)
    R = ibamd.to_host(ef.residual(dpart, got, "hll", 0))
    for v in range(4):
        ps.check_sum(n[v].item(), R[rae.host_roles[0] == 0, v], what=f"residual_norms column {v}")
    with pytest.raises(ValueError, match="has no roles"):
        plain.residual_norms(got)
    with pytest.raises(ValueError, match="partition of 9280 cells"):
        EulerMarch(dpart, roles=rae.roles[1], **kw)
    with pytest.raises(ValueError, match="partition of 9280 cells"):
        MultigridMarch(rae.dparts, rae.coarseners, rae.prolongators, roles=[rae.roles[1], rae.roles[1], rae.roles[2]])


def test_dual_time_march_inherits_the_blank(rae):
    dpart, bcs, roles = rae.dparts[0], rae.bcs[0], rae.roles[0]
    P0 = rae.state(0, "transonic")
    bcs(P0)
    dt = float(ibamd.timestep_euler(dpart, P0, FLUID, 0.3).item())
    m = DualTimeMarch(dpart, 8 * dt, 2, fluid=FLUID, scale=0.3, bcs=bcs, stages=3, roles=roles)
    got = ibamd.to_host(m.step(P0))
    assert (got[rae.host_roles[0] == 2] == f32(rae.far)).all() and np.isfinite(got).all()
    assert m.residual_norms(m.step(P0)).shape == (4,)


# ---------------------------------------------------------------------------------------------------------------------
# 5: the cycle with roles, written out and in a graph
# ---------------------------------------------------------------------------------------------------------------------
def written_out_cycle(h, P, S, stages, scale, pre, post, n_coarsest, l=0, history=None):
    """The V-cycle with roles of the class docstring from level ``l`` in the library's unmasked calls, the select and the
    blank written with torch, every array a new one."""
    part, bcs, roles = h.dparts[l], h.bcs[l], h.roles[l]
    n, nv = part.nc, part.nd + 2
    state = torch.tensor(h.far, dtype=torch.float32, device="cuda")

    def blank(X):
        X[roles.roles == 2] = state
        return X

    def smooth(P, count):
        for _ in range(count):
            dt = ibamd.timestep_euler(part, P, FLUID, scale, out=False, cells=B.colmajor_empty(n))
            P0 = src = P
            for alpha in stages:
                out, work = B.colmajor_empty(n, nv), B.colmajor_empty(n, nv)
                if S is not None:
                    ibamd.stage_euler_dual(part, src, P0, S, dt, alpha, 0.0, out, FLUID, "hll", work=work)
                else:
                    ibamd.stage_euler(part, src, P0, dt, alpha, out, FLUID, "hll", work=work)
                bcs(out)
                src = blank(out)
            P = src
        return P

    if l == len(h.dparts) - 1:
        return smooth(P, n_coarsest)
    P = smooth(P, pre)
    R = ef.residual(part, P, "hll", 0)
    if l == 0 and history is not None:
        history.append((ibamd.to_host(R)[h.host_roles[0] == 0].astype(f64) ** 2).sum(axis=0))
    t = masked(R if S is None else (H(R) + H(S)).t, roles.roles)
    Pc0, D = ibamd.restrict_euler(h.coarseners[l], P, t, None, FLUID)
    h.bcs[l + 1](Pc0)
    c = h.roles[l + 1]
    Pc0[c.roles == 2] = state
    Sc = masked((H(D) - H(ef.residual(h.dparts[l + 1], Pc0, "hll", 0))).t, c.roles)
    Pc = written_out_cycle(h, Pc0, Sc, stages, scale, pre, post, n_coarsest, l + 1)
    Pn = ibamd.prolong_euler(h.prolongators[l], P, Pc, Pc0, FLUID)
    bcs(Pn)
    return smooth(blank(Pn), post)


def make_march(h, roles=True, history=0, **kw):
    kw = {**dict(fluid=FLUID, scale=0.3, stages=3, pre=1, post=1, n_coarsest=2), **kw}
    return MultigridMarch(h.dparts, h.coarseners, h.prolongators, bcs=h.bcs, history=history,
                          roles=h.roles if roles else None, **kw)


def test_cycle_is_the_cycle_written_out(rae, monkeypatch):
    """Two cycles from a disturbed state against the written-out cycle, bit for bit; the history against float64; the calls
    a cycle makes beyond the plain cycle's."""
    P0 = rae.state(0, "transonic")
    rae.bcs[0](P0)
    start = P0.clone()
    hist, ref = [], P0
    for _ in range(2):
        ref = written_out_cycle(rae, ref, None, rk_stages(3), 0.3, 1, 1, 2, history=hist)
    m = make_march(rae, history=3)
    names = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    got = m.cycle(m.cycle(P0))
    monkeypatch.undo()
    same_bits(got, ref, "two cycles with roles")
    same_bits(P0, start, "the initial array is left alone")
    assert np.isfinite(ibamd.to_host(got)).all() and not torch.equal(got, P0)
    assert (ibamd.to_host(got)[rae.host_roles[0] == 2] == f32(rae.far)).all()
    rh = m.residual_history()
    assert rh.shape == (3, 4) and np.isnan(rh[2]).all()
    assert np.allclose(rh[:2], np.array(hist), rtol=1e-12, atol=0.0), (rh, hist)      # (two summation orders in float64)
    per_cycle = {k: names.count(k) // 2 for k in set(names)}
    assert per_cycle["ibh_restrict_euler_roles"] == 2 and per_cycle["ibh_forcing_roles"] == 2 and per_cycle["ibh_sumsq_roles"] == 1
    assert "ibh_restrict_euler" not in per_cycle and "ibh_sumsq" not in per_cycle
    # blanks: one per stage of every step (levels 0 and 1: pre + post, level 2: n_coarsest), P0 of two levels, two prolonged
    assert per_cycle["ibh_scatter_rows"] == 3 * (2 + 2 + 2) + 2 + 2
    plain = make_march(rae, roles=False, history=3)
    plain.cycle(P0)
    assert plain.residual_history().shape == (3,)


def test_cycle_with_roles_in_a_graph(rae):
    """Two cycles captured after one eager cycle and replayed from the restored arrays: the bits of three eager cycles, history
    rows 1 and 2 written by the replay alone, row 3 untouched; no allocation in a cycle."""
    P0 = rae.start
    e = make_march(rae, history=4)
    ref = e.cycle(P0)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ref = e.cycle(e.cycle(ref))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before, "a cycle allocated after construction"
    m = make_march(rae, history=4)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        Pw = m.cycle(P0)
        first = Pw.clone()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            Pg = m.cycle(m.cycle(Pw))
        stream.synchronize()
        assert np.isnan(m.residual_history()[1:]).all(), "the capture ran a cycle"
        Pg.fill_(NAN)
        Pw.copy_(first)
        graph.replay()
    stream.synchronize()
    B._stream()
    same_bits(Pg, ref, "graph replay with roles")
    rh, eh = m.residual_history(), e.residual_history()
    assert rh.shape == (4, 4) and np.isfinite(rh[:3]).all() and np.isnan(rh[3]).all() and np.array_equal(rh[:3], eh[:3])


# ---------------------------------------------------------------------------------------------------------------------
# 6: convergence
# ---------------------------------------------------------------------------------------------------------------------
def test_convergence(rae):
    """tests/test_euler_roles_model.py::test_convergence_in_the_model on the device: 40 V-cycles with roles on 3 levels
    against the device's own single grid -- ``EulerMarch`` without roles, and with them -- over the 93 whole steps within the
    cycles' 280 fine sweeps, ``rk_stages(3)``, per-cell time steps, ``scale`` 0.3, from the free stream.  All end finite and the
    cycles' ``||R_rho||_2`` over the fluid rows is at most 0.9 times either single grid's.  The Float32 numpy model gives 4.763e4
    for the cycles and 5.942e4 / 5.944e4 for the two single grids; the device's figures are printed beside them
    (tests/test_gpu_euler_mg.py::test_convergence asserts no agreement with its model either: the two sweeps round
    differently and the march stalls rather than converges, so there is no rounding argument for a bound)."""
    from test_euler_roles_model import CONV, conv_single_grid_steps
    m = make_march(rae, history=CONV["cycles"], scale=CONV["scale"], stages=CONV["stages"], pre=CONV["pre"], post=CONV["post"],
                   n_coarsest=CONV["n_coarsest"])
    kw = dict(fluid=FLUID, scale=CONV["scale"], stages=CONV["stages"], bcs=rae.bcs[0], local_dt=True)
    single, blanked = EulerMarch(rae.dparts[0], **kw), EulerMarch(rae.dparts[0], roles=rae.roles[0], **kw)
    P = Ps = Pb = rae.start
    for _ in range(CONV["cycles"]):
        P = m.cycle(P)
    for _ in range(conv_single_grid_steps()):
        Ps, Pb = single.step(Ps), blanked.step(Pb)

    def norm(X):
        return float(blanked.residual_norms(X)[0].item()) ** 0.5
    n0, n_mg, n_sg, n_sb = norm(rae.start), norm(P), norm(Ps), norm(Pb)
    hist = np.sqrt(m.residual_history()[:, 0])
    print(f"{CONV['cycles']} cycles with roles: fluid-row ||R_rho|| {n0:.4g} -> {n_mg:.4g} (model 4.763e4; history peak "
          f"{hist.max():.4g}, last {hist[-1]:.4g}); single grid after {conv_single_grid_steps()} steps {n_sg:.4g} (model "
          f"5.942e4), with roles {n_sb:.4g} (model 5.944e4); ratios {n_mg / n_sg:.3f}, {n_mg / n_sb:.3f}")
    for X in (P, Ps, Pb):
        assert np.isfinite(ibamd.to_host(X)).all()
    assert np.isfinite(hist).all()
    assert n_mg <= CONV["ratio"] * n_sg and n_mg <= CONV["ratio"] * n_sb
