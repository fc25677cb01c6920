"""The per-element checker of the step kernels (tests/percell_steps.py), on the CPU.

Calibration: the Float32 numpy oracle stays at or below half of each family's bound against the float64 reference (the
rule of tests/test_percell_closures.py); the pseudo-inverse bounds are 4 x the Float32 LAPACK error measured here.
Sensitivity: each check fails on a planted error of the kind it is there to find.
"""
import math

import numpy as np
import pytest

import percell_steps as ps
from oracle import point_implicit as opi

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------------
# calibration
# ---------------------------------------------------------------------------------------------------------------------
def test_synthetic_accumulator_covers_both_entry_paths():
    for n_out in (255, 257, 4001):
        off, _, _ = ps.synthetic_csr(n_out, 300, seed=n_out)
        ps.assert_paths_covered(off)
    off, idx, w = ps.synthetic_csr(1, 300)
    assert off.tolist() == [0, 8] and idx.size == 8


def test_calibration_accumulator():
    worst = {}
    for n_out, n_in in ((257, 64), (4001, 1000), (255, 255)):
        for weighted in (True, False):
            off, idx, w = ps.synthetic_csr(n_out, n_in, seed=n_out, weighted=weighted)
            for nv in (1, 3, 8):
                v, v2, o0 = ps.seeded((n_in, nv), 1), ps.seeded((n_in, nv), 2), ps.seeded((n_out, nv), 3)
                for name, kw in (("apply", {}), ("diff_add", dict(v2=v2, out0=o0))):
                    ref, sc = ps.acc_ref(off, idx, w, v, **kw)
                    e = ps.check(ps.acc_oracle32(off, idx, w, v, **kw), ref, sc, ps.BOUND_ACC / 2, f"{name} nv={nv}")
                    worst[name] = max(worst.get(name, 0.0), e)
    print("Float32 oracle against float64, accumulator:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_row_walk_model_is_sound():
    """``euler_mg_model.apply`` -- numpy Float32, product per entry, the first one assigned, the others added in entry order:
    the witness tests/test_gpu_percell_steps.py and tests/test_gpu_euler_mg.py hold the device's row walk against bit for bit,
    and which shares no code with it -- on the synthetic rows, weighted and unweighted: within ``BOUND_ACC`` of the float64
    reference and the bits of the Float32 oracle, with and without ``diff`` and ``add``."""
    import euler_mg_model as mg
    from ibamd.accumulator import Accumulator
    worst = 0.0
    for n_out, n_in in ((255, 300), (1020, 255), (257, 64)):
        for weighted in (True, False):
            off, idx, w = ps.synthetic_csr(n_out, n_in, seed=n_out, weighted=weighted)
            ps.assert_paths_covered(off)
            acc = Accumulator(csr=(off, idx, w), n_input=n_in)
            for nv in (1, 3, 6):
                v, v2, o0 = ps.seeded((n_in, nv), 1), ps.seeded((n_in, nv), 2), ps.seeded((n_out, nv), 3)
                for name, got, kw in (("apply", mg.apply(acc, v), {}),
                                      ("diff_add", o0 + mg.apply(acc, v - v2), dict(v2=v2, out0=o0))):
                    what = f"{name} n_out={n_out} w={weighted} nv={nv}"
                    assert got.dtype == f32 and np.isfinite(got).all(), what
                    ref, sc = ps.acc_ref(off, idx, w, v, **kw)
                    worst = max(worst, ps.check(got, ref, sc, ps.BOUND_ACC, what))
                    oracle = np.asarray(ps.acc_oracle32(off, idx, w, v, **kw), f32)
                    assert np.array_equal(got.view(np.uint32), oracle.view(np.uint32)), what
    print(f"Float32 model of the row walk against float64: {worst:.2e}")


def _oracle_set(a, bs):
    dom = ps.oracle_boundaries(bs)
    return ps.oracle_impose(a, dom, [(f"b{k}", b["mode"], b["value"]) for k, b in enumerate(bs)])


def test_calibration_bc():
    """``oracle.domain.impose_bc`` (Float32, sequential calls) against ``bc_ref`` in float64: on every synthetic set and
    on the three boundaries of the advection case, (name, value) as in test/advection.jl."""
    from conftest import ADV_FAMILIES, advection_mesh, oracle_boundaries_view
    import ibamd
    worst = {}
    n = 3904
    a = ps.seeded(n, 4)
    for name, (bs, nlev, ndir) in ps.synthetic_sets(n).items():
        ref, sc = ps.bc_ref(a, bs)
        worst["synthetic"] = max(worst.get("synthetic", 0.0), ps.check(_oracle_set(a, bs), ref, sc, ps.BOUND_BC / 2, name))
    dom = ibamd.Domain(advection_mesh(2e-2), hypercube_families=ADV_FAMILIES, max_partition_size=10 ** 9)
    view = oracle_boundaries_view(dom)
    specs = [("upper", 0, 1.0), ("lower", 0, 0.0), ("outlet", 1, 0.0)]
    a = ps.seeded(len(dom), 5) + f32(0.3)
    bs = [ps.boundary_dict(dom.boundaries[nm][1], mode, val) for nm, mode, val in specs]
    assert all(b["ghost"].size for b in bs)
    ref, sc = ps.bc_ref(a, bs)
    worst["advection"] = ps.check(ps.oracle_impose(a, view, specs), ref, sc, ps.BOUND_BC / 2, "advection boundaries")
    print("Float32 oracle impose_bc against float64:", {k: f"{v:.2e}" for k, v in worst.items()})


def test_calibration_apply():
    worst = 0.0
    for M in range(2, 9):
        D, v = ps.seeded((1000, M, M), M), ps.seeded((1000, M), M + 10)
        ref, sc = ps.apply_ref(D, v)
        worst = max(worst, ps.check(opi.apply_prec(D, v), ref, sc, ps.BOUND_APPLY / 2, f"apply M={M}"))
    print(f"Float32 oracle against float64, block apply: {worst:.2e}")


def test_calibration_pinv():
    """The Float32 LAPACK pinv against the float64 reference per bin: the table PINV_LAPACK holds its maxima (the
    device bound is 4 x)."""
    worst, numpy_worst = {}, {}
    for M in range(2, 9):
        for n in (65, 1000):
            A, kind = ps.pinv_blocks(M, n)
            P, bins, s = ps.pinv_ref(A)
            assert set(kind) >= {"svd", "equal_columns", "zero", "diagonal", "small", "large"}
            assert np.all(bins[kind == "equal_columns"] == "deficient") and np.all(bins[kind == "zero"] == "zero")
            full = ~np.isin(bins, ["deficient", "zero"])
            assert np.all(s[full, -1] >= 0.8e-3 * s[full, 0])
            got = ps.pinv_lapack32(A)
            assert got.dtype == f32
            for k, e in ps.pinv_binned(ps.pinv_error(got, P), bins).items():
                worst[k] = max(worst.get(k, 0.0), e)
            # the oracle's own pinv is numpy's, which computes in double and rounds the result: it sits inside the bounds
            for k, e in ps.pinv_binned(ps.pinv_error(opi.inverse_blocks(A), P), bins).items():
                numpy_worst[k] = max(numpy_worst.get(k, 0.0), e)
                assert e <= (ps.PINV_BOUND[k] if k != "zero" else 0.0)
            mp = ps.moore_penrose(A, got)
            for k in ps.PINV_BOUND:
                if np.any(bins == k):
                    assert mp[bins == k].max() <= ps.PINV_BOUND[k], (M, k, mp[bins == k].max())
    print("Float32 LAPACK pinv against float64 per bin:", {k: f"{v:.2e}" for k, v in worst.items()})
    print("numpy pinv of the oracle (double inside):   ", {k: f"{v:.2e}" for k, v in numpy_worst.items()})
    assert set(worst) == set(ps.PINV_LAPACK) | {"zero"}
    assert worst["zero"] == 0.0
    for k, v in ps.PINV_LAPACK.items():
        assert v / 3 <= worst[k] <= v, (k, worst[k], v)      # the table is the measurement, not a loose cover


def test_rademacher_statement():
    z = ps.splitmix_signs(1000, 12345)
    assert set(np.unique(z)) == {-1.0, 1.0} and abs(z.mean()) < 0.1
    # splitmix64's first output for state 0 (x = 0 + golden gamma) is 0xE220A8397B1DCDAF: top bit set
    assert ps.splitmix_signs(1, 0)[0] == 1.0


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity
# ---------------------------------------------------------------------------------------------------------------------
def _acc_case():
    off, idx, w = ps.synthetic_csr(257, 64, seed=257)
    v = ps.seeded((64, 3), 1)
    ref, sc = ps.acc_ref(off, idx, w, v)
    return off, idx, w, v, ref, sc


def test_sensitivity_wrong_donor_in_a_row_of_eight():
    off, idx, w, v, ref, sc = _acc_case()
    r = int(np.nonzero(np.diff(off) == 8)[0][0])
    bad = idx.copy()
    bad[off[r] + 5] = (bad[off[r] + 5] + 1) % 64
    got = ps.acc_oracle32(off, bad, w, v)
    with pytest.raises(AssertionError, match="bound"):
        ps.check(got, ref, sc, ps.BOUND_ACC, "wrong donor")


def test_sensitivity_fourth_entry_of_an_aligned_row_dropped():
    off, idx, w, v, ref, sc = _acc_case()
    ls = np.diff(off)
    r = int(np.nonzero((ls >= 4) & (off[:-1] % 4 == 0))[0][0])
    w2 = w.copy()
    w2[off[r] + 3] = 0
    with pytest.raises(AssertionError, match="bound"):
        ps.check(ps.acc_oracle32(off, idx, w2, v), ref, sc, ps.BOUND_ACC, "dropped entry")
    ps.check(ps.acc_oracle32(off, idx, w, v), ref, sc, ps.BOUND_ACC, "intact")


def test_sensitivity_two_bc_levels_merged():
    """The planted error comes from the oracle, not from ``bc_ref``: boundary 2 interpolated from the field as it was
    BEFORE boundary 1 wrote its ghosts (two levels run as one)."""
    n = 3904
    a = ps.seeded(n, 4)
    bs, nlev, _ = ps.synthetic_sets(n)["dependent"]
    assert nlev == 2
    ref, sc = ps.bc_ref(a, bs)
    ps.check(_oracle_set(a, bs), ref, sc, ps.BOUND_BC, "sequential")
    merged = _oracle_set(a, bs[:1])
    merged[bs[1]["ghost"]] = _oracle_set(a, bs[1:])[bs[1]["ghost"]]
    with pytest.raises(AssertionError, match="bound"):
        ps.check(merged, ref, sc, ps.BOUND_BC, "merged levels")


def test_sensitivity_reduction_skips_its_last_element():
    x = ps.seeded(257, 7)
    ps.check_sum(float(np.sum(x.astype(f64) ** 2)), x, what="intact")
    with pytest.raises(AssertionError, match="fsum"):
        ps.check_sum(float(np.sum(x[:-1].astype(f64) ** 2)), x, what="skipped")


def test_calibration_ew_sum():
    """The Float32 model of the two-stage sum (the order of ibh_reduce_dev.h) stays at or below half of ``check_sum32``'s
    bound at every total of the device test; the depth is the one read from the code."""
    assert [ps.ew_sum_depth(n) for n in (1, 256, 257, 2048, 2049, 16384, 16385, 256 * 8 * 1024 + 1)] == [11, 11, 12, 18, 26, 29, 29, 33]
    assert ps.ew_reduce_stages(16385) == [(16385, 9), (9, 1)] and ps.ew_reduce_stages(256 * 8 * 1024 + 1)[0][1] == 1024
    worst = 0.0
    for n in ps.EW_REDUCE_TOTALS:
        for seed, lo in ((1, -1.0), (2, 0.0)):                      # mixed signs, and all positive (the sum grows)
            x = ps.seeded(n, seed, lo, 1.0)
            worst = max(worst, ps.check_sum32(ps.ew_sum_model32(x), x, f"model n={n}"))
    print(f"Float32 model of the two-stage sum against fsum: {worst:.2f} of the bound")
    assert worst <= 0.5


def test_sensitivity_ew_sum_drops_one_element():
    for n in (257, 2049, 16385):
        x = ps.seeded(n, 3)
        x[-1] = f32(0.75)
        ps.check_sum32(ps.ew_sum_model32(x), x, "intact")
        with pytest.raises(AssertionError, match="fsum"):
            ps.check_sum32(ps.ew_sum_model32(x[:-1]), x, "dropped")


def test_sensitivity_time_step_wrong_in_one_coarse_side_cell():
    """A probe of a cell with a face to a coarser cell whose value is evaluated as if the neighbour had its own spacing."""
    from conftest import ADV_FAMILIES, advection_mesh, oracle_view
    import ibamd
    import percell as pc
    dom = ibamd.Domain(advection_mesh(2e-2), hypercube_families=ADV_FAMILIES, max_partition_size=10 ** 9, boundaries=False)
    (part,) = dom.partitions.values()
    op = oracle_view(part)
    assert pc.cell_classes(part, block_classes=False)["side_coarse"].any()
    o, nb = (np.asarray(a, np.int64) for a in part.face_owners_neighbors[1])
    sp = part.spacing[:, 0]
    cells = np.unique(o[sp[nb] > sp[o]])[:4]           # cells whose face along x is shared with a coarser cell
    assert cells.size == 4
    M = ps.dt_matrix(part, 0)
    C0 = ps.seeded((part.spacing.shape[0], 2), 8).astype(f64)          # the sparse statement is the oracle's operators
    C0[:, 1] = -2
    assert np.abs(np.maximum(M @ C0[:, 0], ps.dt_matrix(part, 1) @ C0[:, 1]) - ps.dt_percell(op, C0)).max() <= 1e-12
    per = ps.dt_probe_refs(M, part, cells, 0)
    assert np.array_equal(per.argmax(axis=0), cells)
    ref = ps.dt_ref(per[:, 0])
    h = f64(part.spacing[cells[0], 0])
    same = 0.5 / ((0.5 + 0.5) / h)           # both faces with a neighbour of the cell's own spacing
    ps.check_dt(f32(ref), ref, "rounded reference")
    with pytest.raises(AssertionError, match="ulp"):
        ps.check_dt(f32(same), ref, "coarse side read as a side of the cell's own spacing")
    with pytest.raises(AssertionError, match="reference"):
        ps.check_dt(f32(ref), np.nan, "lost NaN")


def test_sensitivity_pinv_keeps_a_singular_value_it_should_cut():
    A, kind = ps.pinv_blocks(4, 65)
    A64 = A.astype(f64)
    got = np.stack([np.linalg.pinv(A64[p], rcond=1e-30) for p in range(A.shape[0])])
    with pytest.raises(AssertionError, match="deficient"):
        ps.check_pinv(got, A, "kept")
    ps.check_pinv(ps.pinv_ref(A)[0], A, "reference")


def test_nan_pattern_comes_first():
    ref = np.array([1.0, np.nan, 2.0])
    with pytest.raises(AssertionError, match="NaN pattern"):
        ps.check(np.array([1.0, 0.0, 2.0]), ref, np.ones(3), 1.0, "lost NaN")
    assert ps.check(np.array([1.0, np.nan, 2.0]), ref, np.ones(3), 0.0) == 0.0
    assert math.isnan(ps.dt_ref(np.array([1.0, np.nan]))) and ps.dt_ref(np.array([-2.0, -4.0])) == -0.25
    assert math.isnan(ps.clamp_julia(np.nan, 0, 1)) and ps.clamp_julia(1.7, 0, 1) == 1 and ps.clamp_julia(-0.5, 0, 1) == 0
