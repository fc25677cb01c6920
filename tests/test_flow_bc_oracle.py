"""The reference side of the bound the fused FlowBC boundary condition is held to on the GPU (test_gpu_flow_bc.py): the
oracle's composed closure -- tests/test_config5.py:87-98: rho, nu, un, ut, ``wall_function(y, ut, nu)``, the slip-wall
``FlowBC`` with ``du!dn``, and the far-field ``FlowBC`` -- evaluated in Float32 against the same lines in Float64, on the
seeded image-point family of flow_bc_model.py.  Rounding of the reference alone must stay inside the project's standing
1e-5, or the GPU comparison against the Float32 oracle would measure the oracle.

Measured (200 000 points, 3-D, rel_inf Float32 against Float64): P columns <= 2.0e-7, nut 2.3e-7, du_dn 3.3e-7, k 4.9e-7,
omega 4.7e-7, epsilon 8.2e-7; in 2-D omega is the largest at 1.2e-6."""
import numpy as np
import pytest

from conftest import rel_inf
import flow_bc_model as fm

f32 = np.float32
N = 200_000


def _evaluate(nd, dtype):
    from oracle import cfd as ocfd
    far = fm.FAR3[:nd + 2]
    P, nrm, y = (a.astype(dtype) for a in fm.image_point_family(N, nd, seed=11))
    ofluid = ocfd.Fluid()
    o_wall = ocfd.FlowBC(ofluid, f32([far[0], far[1], 0.0]), normal_flow=True)
    o_free = ocfd.FlowBC(ofluid, f32(far))
    ba, wf = fm.oracle_wall_closure(ofluid, o_wall, P, nrm, y)
    out = {f"wall P[:, {v}]": ba[:, v] for v in range(nd + 2)}
    out.update({k: wf[k] for k in ("nut", "du_dn", "k", "omega", "epsilon")})
    bf = o_free(P, nrm)
    out.update({f"far P[:, {v}]": bf[:, v] for v in range(nd + 2)})
    return out


@pytest.mark.parametrize("nd", [2, 3])
def test_float32_closure_stays_inside_the_gpu_bound(nd):
    lo, hi = _evaluate(nd, f32), _evaluate(nd, np.float64)
    assert all(v.dtype == f32 for v in lo.values()) and all(v.dtype == np.float64 for v in hi.values())
    errs = {k: float(rel_inf(lo[k], hi[k])) for k in lo}
    print(f"FlowBC closure, {nd}-D, Float32 against Float64 on {N} points:", errs)
    assert all(np.isfinite(v).all() for v in hi.values())
    assert max(errs.values()) <= fm.TOL, errs
