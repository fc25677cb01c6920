"""Multigrid for the Euler march on the device -- ``restrict_euler``, ``prolong_euler``, ``MultigridMarch`` -- bit for bit
against the compositions of the library's own launches that define them, and the cycle's fixed point, graph capture and
convergence.  The numpy model and the mesh hierarchies: tests/euler_mg_model.py; states: tests/regimes.py; helpers:
tests/euler_forms.py.

The compositions: the restriction is ``primitive2state``, the broadcast ``R .+ S``, the coarsener applied to both
(``ibh_accumulate``) and ``state2primitive``; the prolongation is ``primitive2state`` three times, ``prolongator.diff_add``
(``ibh_accumulate_diff_add``) and ``state2primitive``.

Meshes: ``adv_mesh_coarse`` as one partition (3904 cells, refinement, immersed walls) with the two coarser levels of
``multigrid`` (8 -> 4 -> 2 cells per block side: 976 and 244 cells), and the 3-D ``corner`` mesh with one coarser level.  Every
row of their operators starts on a 16-byte boundary, so synthetic operators -- rows of 0 .. 12 entries on and off the
boundary (``percell_steps.synthetic_csr``), and one with more rows than one pass of either grid covers -- stand beside them.
The restricted defect ``D_c`` is also held bit for bit against ``euler_mg_model.apply``, numpy's statement of the row walk.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import euler_forms as ef
import euler_mg_model as mg
import ibamd
import percell_steps as ps
import regimes as rg
from conftest import ADV_FAMILIES, RAE_FAMILIES
from euler_forms import FLUID, NAN, SCALE, padded, same_bits
from ibamd import _lib, cfd
from ibamd import backend as B
from ibamd.accumulator import Accumulator
from ibamd.hiparray import HipArray as H
from ibamd.solver import EulerMarch, MultigridMarch, bdf_coefficients, rk_stages

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


def flow_bcs(dom, far, far_name, wall_names):
    """The far-field and slip-wall closures of ``euler_forms.march_dom`` on the boundaries of ``dom``."""
    free = cfd.FlowBC(FLUID, far)
    wall = cfd.FlowBC(FLUID, [far[0], far[1], 0.0], normal_flow=True)

    def bcs(P):
        ibamd.impose_flow_bc(dom, far_name, free, P)
        for name in wall_names:
            ibamd.impose_flow_bc(dom, name, wall, P)
    return bcs


class Hierarchy:
    """The levels of one mesh on the device: host and device partitions, device operators, one ``bcs`` per level."""

    def __init__(self, doms, coarseners, prolongators, bcs=None):
        self.doms = doms
        self.parts = [mg.part_of(d) for d in doms]
        self.dparts = [ibamd.to_backend(p, ibamd.hip) for p in self.parts]
        self.coarseners, self.prolongators = coarseners, prolongators
        self.bcs = bcs if bcs is not None else [None] * len(doms)
        self.nd = self.parts[0].ndims

    def state(self, l, regime="transonic", seed=7):
        return ibamd.hip(rg.euler_regime(self.parts[l], regime, seed))


@pytest.fixture(scope="module")
def adv(adv_mesh_coarse):
    doms, coa, pro = mg.hierarchy(adv_mesh_coarse, 2, hypercube_families=ADV_FAMILIES)
    far = [1e5, 288.15, 340.0, -340.0]
    return Hierarchy(doms, coa, pro, [flow_bcs(d, far, "outlet", ("lower", "upper")) for d in doms])


@pytest.fixture(scope="module")
def corner():
    return Hierarchy(*mg.hierarchy(mg.corner_mesh(), 1))


@pytest.fixture(scope="module")
def hier(adv, corner):
    return {"adv": adv, "corner": corner}


TRANSFERS = [("adv", 0), ("adv", 1), ("corner", 0)]        # (mesh, the finer of the two levels)


def ragged(n_out, n_in, seed=3):
    """A synthetic operator with random donors and positive weights (the restricted density stays positive).  Its rows are
    those of ``percell_steps.synthetic_csr``: every length of ``ROW_LENGTHS`` -- empty rows, tails after one and after two
    groups of four -- starting at every residue of the 16-byte boundary (asserted).  The grid-stride shape, too long for that
    row-by-row construction, keeps ``r % 6`` entries in row ``r``."""
    rng = np.random.default_rng(seed)
    if n_out < 10 ** 5:
        off, idx, _ = ps.synthetic_csr(n_out, n_in, seed=seed)
        ps.assert_paths_covered(off)
    else:
        off = np.concatenate([[0], np.cumsum(np.arange(n_out) % 6)])
        idx = rng.integers(0, n_in, int(off[-1]))
    w = rng.uniform(0.05, 0.5, int(off[-1])).astype(f32)
    return Accumulator(csr=(off, idx, w), n_input=n_in)


def rows(n, nd, seed):
    """Primitive rows, every eighth one below the temperature clamp (``euler_step_model.synthetic_rows``), and residuals."""
    import euler_step_model as em
    P, R, _ = em.synthetic_rows(n, nd, seed=seed)
    return ibamd.hip(P), ibamd.hip(R)


# ---------------------------------------------------------------------------------------------------------------------
# the compositions
# ---------------------------------------------------------------------------------------------------------------------
def composed_restrict(acc, P, R, S):
    dacc = ibamd.to_backend(acc)
    Pc = cfd.state2primitive(FLUID, dacc(cfd.primitive2state(FLUID, P)))
    return Pc, dacc(R if S is None else (H(R) + H(S)).t)


def composed_prolong(acc, P, Pn, Po):
    Q = cfd.primitive2state(FLUID, P)
    ibamd.to_backend(acc).diff_add(Q, cfd.primitive2state(FLUID, Pn), cfd.primitive2state(FLUID, Po))
    return cfd.state2primitive(FLUID, Q)


def compact(t):
    out = B.colmajor_empty(*t.shape)
    out.copy_(t)
    return out


def check_restrict(acc, P, R, S, what):
    n_out, nv = acc.n_output, P.shape[1]
    for with_S in (True, False):
        Sx = S if with_S else None
        ref_P, ref_D = composed_restrict(acc, P, R, Sx)
        tag = f"{what} S={'given' if with_S else 'NULL'}"
        oP, oD = B.colmajor_empty(n_out, nv), B.colmajor_empty(n_out, nv)
        oP.fill_(NAN)
        oD.fill_(NAN)
        got = ibamd.restrict_euler(acc, P, R, Sx, FLUID, out=oP, out_D=oD)
        assert got[0] is oP and got[1] is oD
        same_bits(oP, ref_P, tag + " P_c")
        same_bits(oD, ref_D, tag + " D_c")
        # D_c against a witness that shares no code with the device's row walk (multiplications and additions only: the
        # model's bits; P_c passes through divisions and stays proved against the composition)
        Rh = ibamd.to_host(R)
        model_D = mg.apply(acc, Rh + ibamd.to_host(S) if with_S else Rh)
        same_bits(oD, torch.from_numpy(model_D), tag + " D_c against the numpy model")
        aP, aD = ibamd.restrict_euler(acc, P, R, Sx, FLUID)
        same_bits(aP, ref_P, tag + " P_c allocated")
        same_bits(aD, ref_D, tag + " D_c allocated")
        # padded leading dimensions, every array its own, and nothing written past the rows
        pads = [padded(P.shape[0], nv, pad) for pad in (13, 5, 7)]
        for p, src in zip(pads, (P, R, S)):
            p.copy_(src)
        baseP = torch.full((nv, n_out + 29), NAN, dtype=torch.float32, device="cuda")
        baseD = torch.full((nv, n_out + 3), NAN, dtype=torch.float32, device="cuda")
        ibamd.restrict_euler(acc, pads[0], pads[1], pads[2] if with_S else None, FLUID, out=baseP.T[:n_out],
                             out_D=baseD.T[:n_out])
        same_bits(compact(baseP.T[:n_out]), ref_P, tag + " P_c padded")
        same_bits(compact(baseD.T[:n_out]), ref_D, tag + " D_c padded")
        assert torch.isnan(baseP[:, n_out:]).all() and torch.isnan(baseD[:, n_out:]).all()
    return ref_P


def check_prolong(acc, P, Pn, Po, what):
    n_out, nv = acc.n_output, P.shape[1]
    ref = composed_prolong(acc, P, Pn, Po)
    out = B.colmajor_empty(n_out, nv)
    out.fill_(NAN)
    assert ibamd.prolong_euler(acc, P, Pn, Po, FLUID, out=out) is out
    same_bits(out, ref, what)
    same_bits(ibamd.prolong_euler(acc, P, Pn, Po, FLUID), ref, what + " allocated")
    inplace = P.clone()
    assert ibamd.prolong_euler(acc, inplace, Pn, Po, FLUID, out=inplace) is inplace
    same_bits(inplace, ref, what + " P_out is P_f")
    # padded: the coarse states share a leading dimension, the fine ones have their own; a pack of the caller's
    Pp, Pnp, Pop = padded(n_out, nv, 13), padded(acc.n_input, nv, 5), padded(acc.n_input, nv, 5)
    for p, src in ((Pp, P), (Pnp, Pn), (Pop, Po)):
        p.copy_(src)
    base = torch.full((nv, n_out + 29), NAN, dtype=torch.float32, device="cuda")
    pack = torch.full((8 * acc.n_input + 8,), NAN, dtype=torch.float32, device="cuda")
    ibamd.prolong_euler(acc, Pp, Pnp, Pop, FLUID, out=base.T[:n_out], pack=pack)
    same_bits(compact(base.T[:n_out]), ref, what + " padded")
    assert torch.isnan(base[:, n_out:]).all() and torch.isnan(pack[8 * acc.n_input:]).all()
    ibamd.prolong_euler(acc, Pp, Pnp, Pop, FLUID, out=Pp)
    same_bits(compact(Pp), ref, what + " padded, P_out is P_f")
    assert np.isfinite(ibamd.to_host(ref)).any()


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the transfers against their compositions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,l", TRANSFERS, ids=[f"{m}{l}" for m, l in TRANSFERS])
def test_restrict_bit_for_bit(hier, mesh, l):
    h = hier[mesh]
    for regime in ("transonic", "cold"):          # cold: every row below the max(T, 10) clamp or near it
        P = h.state(l, regime)
        R = ef.residual(h.dparts[l], P, "hll", 0)
        S = ibamd.dual_source(P, h.state(l, regime, seed=9), 1.7e3, -4.0e2, FLUID)
        Pc = check_restrict(h.coarseners[l], P, R, S, f"{mesh} level {l} {regime}")
        assert np.isfinite(ibamd.to_host(Pc)).all()


@pytest.mark.parametrize("mesh,l", TRANSFERS, ids=[f"{m}{l}" for m, l in TRANSFERS])
def test_prolong_bit_for_bit(hier, mesh, l):
    h = hier[mesh]
    for regime in ("transonic", "cold"):
        P, Pn, Po = h.state(l, regime), h.state(l + 1, regime), h.state(l + 1, regime, seed=9)
        check_prolong(h.prolongators[l], P, Pn, Po, f"{mesh} level {l} {regime}")


@pytest.mark.parametrize("nd,n_out,n_in", [(2, 1000, 333), (3, 777, 2100), (3, 4096 * 256 + 77, 2048 * 256 + 55)],
                         ids=["2d", "3d", "3d_grid_stride"])
def test_transfers_on_ragged_rows(nd, n_out, n_in):
    """Rows of 0 .. 12 entries (0 .. 5 in the last case) that start on and off 16-byte boundaries; the last case has more
    output rows than one pass of the row kernels' grids (4096 x 256) and more input rows than one pass of the pack kernel's
    (2048 x 256)."""
    acc = ragged(n_out, n_in)
    P, R = rows(n_in, nd, 5)
    _, S = rows(n_in, nd, 6)
    if n_out < 10 ** 5:
        check_restrict(acc, P, R, S, f"ragged {nd}-D restrict")
    else:
        ref_P, ref_D = composed_restrict(acc, P, R, S)
        got_P, got_D = ibamd.restrict_euler(acc, P, R, S, FLUID)
        same_bits(got_P, ref_P, "large ragged P_c")
        same_bits(got_D, ref_D, "large ragged D_c")
    Pf, _ = rows(n_out, nd, 7)
    Pn, _ = rows(n_in, nd, 8)
    if n_out < 10 ** 5:
        check_prolong(acc, Pf, Pn, P, f"ragged {nd}-D prolong")
    else:
        same_bits(ibamd.prolong_euler(acc, Pf, Pn, P, FLUID), composed_prolong(acc, Pf, Pn, P), "large ragged prolong")


# ---------------------------------------------------------------------------------------------------------------------
# 3: argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_checks(adv):
    """Every misuse raises before any launch: the sentinel-filled outputs are as they were."""
    coa, pro = ibamd.to_backend(adv.coarseners[0]), ibamd.to_backend(adv.prolongators[0])
    nf, nk, nv = coa.n_input, coa.n_output, 4
    P, R, S = adv.state(0), B.colmajor_empty(nf, nv), B.colmajor_empty(nf, nv)
    R.fill_(1.0)
    S.fill_(2.0)
    Pn, Po = adv.state(1), adv.state(1, seed=9)
    oP, oD, out = B.colmajor_empty(nk, nv), B.colmajor_empty(nk, nv), B.colmajor_empty(nf, nv)
    pack = torch.empty(8 * nk + 8, dtype=torch.float32, device="cuda")
    outputs = (oP, oD, out, pack)
    for t in outputs:
        t.fill_(-7.0)
    keep = P.clone()
    f, p = FLUID._c(), B._ptr

    def restrict(**o):
        d = dict(acc=coa.handle, f=C.byref(f), nd=2, P=p(P), ldp=nf, R=p(R), ldr=nf, S=p(S), lds=nf, Pc=p(oP), ldpc=nk, D=p(oD),
                 ldd=nk)
        d.update(o)
        _lib.call("ibh_restrict_euler", *d.values())

    def prolong(**o):
        d = dict(acc=pro.handle, f=C.byref(f), nd=2, Pn=p(Pn), Po=p(Po), ldc=nk, pack=p(pack), P=p(P), ldp=nf, out=p(out), ldo=nf)
        d.update(o)
        _lib.call("ibh_prolong_euler", *d.values())

    null = None
    B._stream()
    for o, what in ([(dict([(k, null)]), "null") for k in ("acc", "f", "P", "R", "Pc", "D")]
                    + [(dict(nd=1), "nd must be 2 or 3"), (dict(nd=4), "nd must be 2 or 3")]
                    + [(dict([(k, nf - 1)]), "leading dimension") for k in ("ldp", "ldr", "lds")]
                    + [(dict([(k, nk - 1)]), "leading dimension") for k in ("ldpc", "ldd")]
                    + [(dict(D=p(oP)), "D_c may not alias P_c"), (dict(D=p(oP[1:])), "D_c may not alias P_c")]
                    + [(dict([(k, p(t))]), "may not alias P_f, R_f or S_f") for k in ("Pc", "D") for t in (P, R, S)]):
        with pytest.raises(_lib.IbhError, match="ibh_restrict_euler: .*" + what):
            restrict(**o)
    for o, what in ([(dict([(k, null)]), "null") for k in ("acc", "f", "Pn", "Po", "P", "out")]
                    + [(dict(nd=1), "nd must be 2 or 3"), (dict(nd=5), "nd must be 2 or 3")]
                    + [(dict(pack=null), "pack is missing"), (dict(pack=p(pack[1:])), "32-byte aligned"),
                       (dict(pack=p(pack[4:])), "32-byte aligned")]
                    + [(dict(ldc=nk - 1), "leading dimension"), (dict(ldp=nf - 1), "leading dimension"),
                       (dict(ldo=nf - 1), "leading dimension")]
                    # (an output placed on a smaller or shifted array runs past its end, into whatever the allocator put
                    # there: which of the aliasing rules speaks first is not the test's to say)
                    + [(dict(out=p(Pn)), "may not (alias|overlap)"), (dict(out=p(Po)), "may not (alias|overlap)"),
                       (dict(pack=p(Pn)), "pack may not alias"), (dict(pack=p(P)), "pack may not alias"),
                       (dict(out=p(P[8:]), ldo=nf), "may not (alias|overlap)"),
                       (dict(out=p(P), ldo=nf + 8), "may not (alias|overlap)")]):
        with pytest.raises(_lib.IbhError, match="ibh_prolong_euler: .*" + what):
            prolong(**o)
    torch.cuda.synchronize()
    for t in outputs:
        assert bool((t == -7.0).all()), "an output was written by a refused call"
    same_bits(P, keep, "P_f")
    # the Python layer's own checks
    with pytest.raises(ValueError, match="one leading dimension"):
        ibamd.prolong_euler(pro, P, Pn, padded(nk, nv, 5), FLUID)
    with pytest.raises(ValueError, match="pack must be"):
        ibamd.prolong_euler(pro, P, Pn, Po, FLUID, pack=pack[:8])
    with pytest.raises(ValueError, match="rows"):
        ibamd.restrict_euler(coa, Pn, R, None, FLUID)
    with pytest.raises(TypeError, match="Accumulator"):
        ibamd.restrict_euler(adv.dparts[0], P, R, None, FLUID)
    # zero rows: no error, nothing launched
    empty = Accumulator(csr=(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, f32)), n_input=nf)
    zP, zD = ibamd.restrict_euler(empty, P, R, None, FLUID)
    assert zP.shape == (0, nv) and zD.shape == (0, nv)


# ---------------------------------------------------------------------------------------------------------------------
# 4: one level is the march
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", [1, 3])
def test_one_level_is_the_euler_march(adv, stages, monkeypatch):
    dpart, bcs = adv.dparts[0], adv.bcs[0]
    P0 = adv.state(0)
    m = MultigridMarch([dpart], fluid=FLUID, scale=SCALE, bcs=[bcs], stages=stages, n_coarsest=2)
    e = EulerMarch(dpart, FLUID, scale=SCALE, bcs=bcs, local_dt=True, stages=stages)
    bcs(P0.clone())                               # (the boundaries go to the device with their first use)
    names = []
    real = B.call
    monkeypatch.setattr(B, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    got = m.cycle(m.cycle(P0))
    mine, names[:] = [n for n in names if n != "ibh_set_stream"], []
    ref = P0
    for _ in range(4):
        ref = e.step(ref)
    theirs = [n for n in names if n != "ibh_set_stream"]
    same_bits(got, ref, f"one level, stages={stages}")
    assert mine == theirs and "ibh_timestep_euler" in mine
    assert ("ibh_step_euler" if stages == 1 else "ibh_stage_euler") in mine
    assert not any(n in mine for n in ("ibh_stage_euler_dual", "ibh_restrict_euler", "ibh_prolong_euler", "ibh_sumsq"))


# ---------------------------------------------------------------------------------------------------------------------
# 5: the cycle written out
# ---------------------------------------------------------------------------------------------------------------------
def written_out_cycle(h, P, S, g, scheme, stages, pre, post, n_coarsest, l=0, history=None):
    """The V-cycle of the class docstring from level ``l`` in the library's own calls, every array a new one."""
    part, bcs = h.dparts[l], h.bcs[l]
    n, nv = part.nc, part.nd + 2

    def smooth(P, count):
        for _ in range(count):
            dt = ibamd.timestep_euler(part, P, FLUID, SCALE, out=False, cells=B.colmajor_empty(n))
            P0 = src = P
            for alpha in stages:
                out, work = B.colmajor_empty(n, nv), B.colmajor_empty(n, nv)
                if S is not None:
                    ibamd.stage_euler_dual(part, src, P0, S, dt, alpha, g, out, FLUID, scheme, work=work)
                elif stages == (1.0,):
                    ibamd.step_euler(part, src, dt, out, FLUID, scheme, work=work)
                else:
                    ibamd.stage_euler(part, src, P0, dt, alpha, out, FLUID, scheme, work=work)
                if bcs is not None:
                    bcs(out)
                src = out
            P = src
        return P

    if l == len(h.dparts) - 1:
        return smooth(P, n_coarsest)
    P = smooth(P, pre)
    R = ef.residual(part, P, scheme, 0)
    if l == 0 and history is not None:
        history.append(float((ibamd.to_host(R)[:, 0].astype(f64) ** 2).sum()))
    Pc0, D = ibamd.restrict_euler(h.coarseners[l], P, R, S, FLUID)
    if h.bcs[l + 1] is not None:
        h.bcs[l + 1](Pc0)
    Sc = (H(D) - H(ef.residual(h.dparts[l + 1], Pc0, scheme, 0))).t
    Pc = written_out_cycle(h, Pc0, Sc, g, scheme, stages, pre, post, n_coarsest, l + 1)
    Pn = ibamd.prolong_euler(h.prolongators[l], P, Pc, Pc0, FLUID)
    if bcs is not None:
        bcs(Pn)
    return smooth(Pn, post)


def make_march(h, scheme="hll", stages=1, pre=1, post=1, n_coarsest=2, bcs=True, history=0):
    return MultigridMarch(h.dparts, h.coarseners, h.prolongators, fluid=FLUID, scheme=scheme, scale=SCALE,
                          bcs=h.bcs if bcs else None, stages=stages, pre=pre, post=post, n_coarsest=n_coarsest, history=history)


@pytest.mark.parametrize("stages", [1, 3], ids=["euler", "rk3"])
@pytest.mark.parametrize("scheme", ["hll", "sensor"])
@pytest.mark.parametrize("mesh", ["adv", "corner"])
def test_cycle_is_the_cycle_written_out(hier, mesh, scheme, stages):
    h = hier[mesh]
    P0 = h.state(0)
    start = P0.clone()
    dt1 = ibamd.timestep_euler(h.dparts[0], P0, FLUID, SCALE)
    cn, cm, g = bdf_coefficients(2, 8 * float(dt1.item()))
    S = ibamd.dual_source(P0, h.state(0, seed=9), cn, cm, FLUID)
    S_start = S.clone()
    for pre, post in ((1, 1), (2, 0)):
        for Sx, gx in ((None, 0.0), (S, g)):
            what = f"{mesh} {scheme} stages={stages} pre={pre} post={post} {'steady' if Sx is None else 'BDF2'}"
            m = make_march(h, scheme, stages, pre, post, history=3)
            hist = []
            ref = P0
            for _ in range(2):
                ref = written_out_cycle(h, ref, Sx, gx, scheme, rk_stages(stages), pre, post, 2, history=hist)
            got = m.cycle(m.cycle(P0, Sx, gx), Sx, gx)
            same_bits(got, ref, what)
            assert np.isfinite(ibamd.to_host(got)).all(), what
            assert not torch.equal(got, P0)
            same_bits(P0, start, what + ": the initial array is left alone")
            same_bits(S, S_start, what + ": the source is left alone")
            rh = m.residual_history()
            assert rh.shape == (3,) and np.isnan(rh[2])
            assert np.allclose(rh[:2], hist, rtol=1e-12, atol=0.0), (what, rh, hist)      # (two summation orders in float64)
    with pytest.raises(ValueError, match="g > 0 needs"):
        m.cycle(P0, None, g)


def test_march_checks(adv, corner):
    """The constructor's own checks on real levels (the refusals that need no device: tests/test_euler_mg_model.py)."""
    with pytest.raises(ValueError, match="coarseners"):
        MultigridMarch(adv.dparts, adv.coarseners[:1], adv.prolongators)
    with pytest.raises(ValueError, match="returns \\(coarse_doms, prolongators, coarseners\\)"):
        MultigridMarch(adv.dparts, adv.prolongators, adv.coarseners)             # the two lists swapped
    with pytest.raises(ValueError, match="cells"):
        MultigridMarch([adv.dparts[0], adv.dparts[2]], adv.coarseners[:1], adv.prolongators[:1])
    with pytest.raises(ValueError, match="one callable per level"):
        MultigridMarch(adv.dparts, adv.coarseners, adv.prolongators, bcs=adv.bcs[:2])
    m = MultigridMarch(adv.parts, adv.coarseners, adv.prolongators)              # host partitions are taken to the device
    assert [lv.part for lv in m.levels] == adv.dparts and m.residual_history().shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# 6: the fixed point
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages,pre,post", [(1, 1, 1), (3, 1, 1), (1, 2, 0)], ids=["euler", "rk3", "pre2"])
def test_fixed_point(adv, stages, pre, post):
    """With ``S = -R(P)`` the fine residual ``R + S`` of the first stage, the restricted defect and so the coarse correction
    are zero up to what rounding makes of them: one cycle moves ``P`` by no more than ``n e_v`` per column, ``e_v`` the most
    one primitive -> conserved -> primitive round trip moves a value of that column on these arrays and ``n`` the number of
    such round trips in the cycle (``euler_mg_model.round_trips``: a count).  The state is the transonic one, whose
    velocities are of the size of the sound speed: ``e_v`` of a velocity column is relative to the velocities, and the
    yardstick holds where a rounding of ``p`` moves ``u`` by no more than a rounding of ``u`` itself (tests/
    test_euler_mg_model.py runs the same case in the model).  The same cycle with ``S = 0`` moves ``P`` by more than the bound,
    so the bound tells the two apart."""
    P = adv.state(0)
    R = ibamd.residual_euler_hll(adv.dparts[0], P, fluid=FLUID)
    S = (H(R) * -1.0).t
    assert torch.equal(S, -R)
    back = cfd.state2primitive(FLUID, cfd.primitive2state(FLUID, P))
    e = np.abs(ibamd.to_host(back).astype(f64) - ibamd.to_host(P)).max(axis=0)
    n = mg.round_trips(3, stages, pre, post, 2)
    assert (e > 0).all()
    moved = {}
    for name, Sx in (("S = -R", S), ("S = 0", torch.zeros_like(S))):
        m = make_march(adv, "hll", stages, pre, post, bcs=False)
        got = m.cycle(P, Sx, 0.0)
        moved[name] = np.abs(ibamd.to_host(got).astype(f64) - ibamd.to_host(P)).max(axis=0)
        print(f"stages={stages} pre={pre} post={post} {name}: moved {moved[name]} = {moved[name] / (n * e)} x n e_v, n = {n}, e_v = {e}")
    assert (moved["S = -R"] <= n * e).all()
    assert (moved["S = 0"] > n * e).all()


# ---------------------------------------------------------------------------------------------------------------------
# 7: graph capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["adv", "corner"])
def test_cycle_in_a_graph(hier, mesh):
    """Two cycles captured after one eager cycle and replayed from the restored arrays: the bits of three eager cycles, history
    entries 1 and 2 written by the replay alone, entry 3 untouched; no allocation in a cycle."""
    h = hier[mesh]
    P0 = h.state(0)
    e = make_march(h, stages=3, history=4)
    ref = e.cycle(P0)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ref = e.cycle(e.cycle(ref))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before, "a cycle allocated after construction"
    m = make_march(h, stages=3, history=4)
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
    same_bits(Pg, ref, f"{mesh}: graph replay")
    rh, eh = m.residual_history(), e.residual_history()
    assert np.isfinite(rh[:3]).all() and np.isnan(rh[3]) and np.array_equal(rh[:3], eh[:3])


# ---------------------------------------------------------------------------------------------------------------------
# 8: convergence
# ---------------------------------------------------------------------------------------------------------------------
def test_convergence(rae_mesh_small):
    """``rae_mesh_small`` as one partition at Mach 0.5 and zero incidence, from the free stream, far field and slip wall on
    every level: 3 V-cycles on 3 levels against 7 single-grid ``EulerMarch`` steps -- both ``rk_stages(3)``, per-cell time
    steps, ``scale`` 0.3: 21 fine-level sweeps each, the cycle's sweep before the restriction counted.  Both end finite and
    the cycles end with the smaller ``||R_rho||_2`` over all rows.  The case, its length and what happens beyond it:
    tests/test_euler_mg_model.py::test_convergence_in_the_model (Float32 model: 1.44e5 against 1.77e5)."""
    from test_euler_mg_model import CONV, conv_far
    doms, coa, pro = mg.hierarchy(rae_mesh_small, 2, hypercube_families=RAE_FAMILIES)
    far = [float(x) for x in conv_far()]
    h = Hierarchy(doms, coa, pro, [flow_bcs(d, far, "farfield", ("wall",)) for d in doms])
    start = ibamd.hip(np.tile(f32(far), (len(doms[0]), 1)))
    h.bcs[0](start)
    kw = dict(fluid=FLUID, scale=CONV["scale"], stages=CONV["stages"])
    m = MultigridMarch(h.dparts, coa, pro, bcs=h.bcs, pre=CONV["pre"], post=CONV["post"], n_coarsest=CONV["n_coarsest"],
                       history=CONV["cycles"], **kw)
    e = EulerMarch(h.dparts[0], bcs=h.bcs[0], local_dt=True, **kw)
    P = Ps = start
    for _ in range(CONV["cycles"]):
        P = m.cycle(P)
    fine_sweeps = CONV["cycles"] * ((CONV["pre"] + CONV["post"]) * CONV["stages"] + 1)
    for _ in range(fine_sweeps // CONV["stages"]):
        Ps = e.step(Ps)

    def norm(X):
        R = ibamd.to_host(ibamd.residual_euler_hll(h.dparts[0], X, fluid=FLUID))
        return float(np.sqrt((R[:, 0].astype(f64) ** 2).sum()))
    n0, n_mg, n_sg = norm(start), norm(P), norm(Ps)
    print(f"{fine_sweeps} fine sweeps: ||R_rho|| {n0:.4g} -> multigrid {n_mg:.4g}, single grid {n_sg:.4g}; history "
          f"{np.sqrt(m.residual_history())}")
    assert np.isfinite(ibamd.to_host(P)).all() and np.isfinite(ibamd.to_host(Ps)).all()
    assert n_mg < n_sg
