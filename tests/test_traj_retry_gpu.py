"""The overflow retry of the three trajectory batch calls (batch.totp3d_batch, polytraj3d_batch,
splinetraj3d_batch) where the other suites do not reach it: in the cells form, with per-path boundary
conditions, and for the time-optimal sample profiles; and the empty batch.  A call whose first point_cap
is too small for some paths must return what an uncapped call returns, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VMAX, AMAX, DT, DEGREE = (2.0, 2.0, 1.5), (1.5, 1.5, 1.0), 0.05, 3
DIMS, PATH_CAP = (8, 8, 8), 8
# 3, 4, 5 and 6 cells, strictly monotone in x (no repeated waypoint: the spline accepts them)
PATHS = [np.array(p, np.float64) for p in (
    [(0, 0, 0), (1, 1, 0), (2, 1, 1)],
    [(0, 1, 1), (1, 2, 1), (2, 2, 2), (3, 3, 2)],
    [(1, 0, 2), (2, 1, 2), (3, 1, 3), (4, 2, 3), (5, 2, 4)],
    [(0, 3, 0), (1, 3, 1), (2, 4, 1), (3, 4, 2), (4, 5, 2), (5, 5, 3)])]
NQ = len(PATHS)
# initial / final velocity, initial / final acceleration: non-zero, different for every path
BC = ((np.arange(NQ * 12).reshape(NQ, 4, 3) % 7) - 3) * 0.05


def _cells():
    import torch

    X, Y, Z = DIMS
    ids = np.zeros((NQ, PATH_CAP), np.int32)
    for q, p in enumerate(PATHS):
        v = p.astype(np.int64)
        ids[q, : len(p)] = v[:, 0] * Y * Z + v[:, 1] * Z + v[:, 2]
    lens = np.array([len(p) for p in PATHS], np.int32)
    return torch.as_tensor(ids, device="cuda"), torch.as_tensor(lens, device="cuda"), DIMS


def _same(a, b):
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan], b[~nan])


def _cap(full):
    """A first cap between the batch's counts (their median): the longer paths overflow it, the shorter do not."""
    npt = full["n_points"].cpu().numpy()
    cap = int(np.median(npt))
    over = npt > cap
    assert over.any() and not over.all(), npt
    return npt, cap, over


def _retry_equals_uncapped(full, capped, npt, cap, over):
    assert capped["status"].cpu().numpy().tolist() == [0] * NQ == full["status"].cpu().numpy().tolist()
    assert np.array_equal(capped["n_points"].cpu().numpy(), npt)
    assert np.array_equal(capped["total_time"].cpu().numpy(), full["total_time"].cpu().numpy())
    assert capped["points"].shape[1] == int(npt[over].max())
    fp, cp = full["points"].cpu().numpy(), capped["points"].cpu().numpy()
    for q in range(NQ):
        assert _same(cp[q, : npt[q]], fp[q, : npt[q]]), q
        if not over[q]:
            assert np.isnan(cp[q, cap:]).all(), q


def test_polytraj_cells_retry_with_boundary_conditions():
    from python_motion_planning_amd import _lib, batch

    prm = _lib.PolyTrajParams.make(VMAX, AMAX, DT)
    full = batch.polytraj3d_batch(PATHS, prm, bc=BC)
    npt, cap, over = _cap(full)
    capped = batch.polytraj3d_batch(None, prm, bc=BC, cells=_cells(), point_cap=cap)
    _retry_equals_uncapped(full, capped, npt, cap, over)
    # the boundary conditions reached the retried paths: without them their rows differ
    plain = batch.polytraj3d_batch(PATHS, prm)
    q = int(np.nonzero(over)[0][0])
    assert not _same(plain["points"][q, : npt[q]].cpu().numpy(), full["points"][q, : npt[q]].cpu().numpy())


def test_splinetraj_cells_retry():
    from python_motion_planning_amd import _lib, batch

    prm = _lib.SplineTrajParams.make(VMAX, AMAX, DT, DEGREE)
    full = batch.splinetraj3d_batch(PATHS, prm)
    npt, cap, over = _cap(full)
    capped = batch.splinetraj3d_batch(None, prm, cells=_cells(), point_cap=cap)
    _retry_equals_uncapped(full, capped, npt, cap, over)


def test_totp_retry_merges_the_sample_profiles():
    from python_motion_planning_amd import _lib, batch

    prm = _lib.TotpParams.make(VMAX, AMAX, DT, 0.05)
    full = batch.totp3d_batch(PATHS, prm)
    npt, cap, over = _cap(full)
    capped = batch.totp3d_batch(PATHS, prm, point_cap=cap)
    _retry_equals_uncapped(full, capped, npt, cap, over)
    ns = full["n_samples"].cpu().numpy()
    assert np.array_equal(capped["n_samples"].cpu().numpy(), ns)
    for q in np.nonzero(over)[0]:
        for k in ("s_values", "s_dot", "s_ddot", "time"):
            assert np.array_equal(capped[k][q, : ns[q]].cpu().numpy(), full[k][q, : ns[q]].cpu().numpy()), (q, k)


def test_empty_batch():
    import torch

    from python_motion_planning_amd import _lib, batch

    i32 = dict(dtype=torch.int32, device="cuda")
    none = (torch.zeros((0, PATH_CAP), **i32), torch.zeros(0, **i32), DIMS)
    common = {"points", "n_points", "total_time", "status"}
    totp = batch.totp3d_batch([], _lib.TotpParams.make(VMAX, AMAX, DT, 0.05))
    assert set(totp) == common | {"s_values", "s_dot", "s_ddot", "time", "n_samples"}
    pprm, sprm = _lib.PolyTrajParams.make(VMAX, AMAX, DT), _lib.SplineTrajParams.make(VMAX, AMAX, DT, DEGREE)
    poly, poly_c = batch.polytraj3d_batch([], pprm), batch.polytraj3d_batch(None, pprm, cells=none)
    assert set(poly) == common | {"segment_times", "seg_off"} and set(poly_c) == common | {"segment_times"}
    assert poly["seg_off"].tolist() == [0] and poly_c["segment_times"].shape == (0, PATH_CAP)
    spl, spl_c = batch.splinetraj3d_batch([], sprm), batch.splinetraj3d_batch(None, sprm, cells=none)
    assert set(spl) == common and set(spl_c) == common
    for r, row in ((totp, 12), (poly, 15), (poly_c, 15), (spl, 12), (spl_c, 12)):
        assert r["points"].shape[0] == 0 and r["points"].shape[2] == row and r["points"].dtype == torch.float64
        assert r["n_points"].shape == (0,) and r["status"].shape == (0,) and r["total_time"].shape == (0,)
        assert r["n_points"].dtype == torch.int32 and r["status"].dtype == torch.int32
