"""gad_ball_query_grid (include/gaddpg.h section A): the radius search through a uniform grid in global memory against the CPU
oracle and against gad_ball_query on the same input -- indices and counts bit for bit.  Direct calls of the entry point, each on
a workspace filled with 0xFF bytes; the shapes are the smallest at which each mechanism can go wrong: just past the LDS kernels'
4096 points, past 65 535 points, clouds with different boxes in one batch, nsample that is no multiple of 64, centroids outside
the box, distances exactly on the radius, more candidates than the kernel holds, flat clouds and non-finite coordinates."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_WS = {}


def _workspace(nbytes):
    """ONE buffer for the whole module (grown when a shape asks for more): successive calls, of different shapes, reuse it"""
    if _WS.get("t") is None or _WS["t"].numel() < nbytes:
        _WS["t"] = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    return _WS["t"]


def _grid(new_xyz, xyz, radius, nsample):
    """a direct call of gad_ball_query_grid -> (idx, cnt) as numpy arrays"""
    from ga_ddpg_amd import hip
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    nbytes = hip.lib().gad_ball_query_grid_workspace_bytes(B, N, M, nsample)
    assert nbytes > 0
    ws = _workspace(nbytes)
    ws.fill_(0xFF)
    x, c = torch.from_numpy(xyz).cuda(), torch.from_numpy(new_xyz).cuda()
    idx = torch.full((B, M, nsample), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((B, M), -7, dtype=torch.int32, device="cuda")
    hip.call("gad_ball_query_grid", c, x, B, N, M, float(radius), nsample, idx, cnt, ws)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), cnt.cpu().numpy()


def _scan(new_xyz, xyz, radius, nsample):
    from ga_ddpg_amd import hip
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    x, c = torch.from_numpy(xyz).cuda(), torch.from_numpy(new_xyz).cuda()
    idx = torch.full((B, M, nsample), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((B, M), -7, dtype=torch.int32, device="cuda")
    hip.call("gad_ball_query", c, x, B, N, M, float(radius), nsample, idx, cnt)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), cnt.cpu().numpy()


def _check(new_xyz, xyz, radius, nsample):
    """grid == oracle == scan, exactly -> the oracle's (idx, cnt)"""
    from oracle import cref
    new_xyz, xyz = np.ascontiguousarray(new_xyz, dtype=np.float32), np.ascontiguousarray(xyz, dtype=np.float32)
    want_idx, want_cnt = cref.ball_query(new_xyz, xyz, radius, nsample, return_count=True)
    got_idx, got_cnt = _grid(new_xyz, xyz, radius, nsample)
    np.testing.assert_array_equal(got_cnt, want_cnt)
    np.testing.assert_array_equal(got_idx, want_idx)
    scan_idx, scan_cnt = _scan(new_xyz, xyz, radius, nsample)
    np.testing.assert_array_equal(got_cnt, scan_cnt)
    np.testing.assert_array_equal(got_idx, scan_idx)
    return want_idx, want_cnt


def _hits(new_xyz, xyz, radius):
    """unclipped hit counts (B,M) with the pinned float32 evaluation order"""
    c, p = new_xyz.astype(np.float32)[:, :, None, :], xyz.astype(np.float32)[:, None, :, :]
    with np.errstate(invalid="ignore", over="ignore"):
        d = c - p
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        return (d2 < np.float32(radius) * np.float32(radius)).sum(axis=2)


RADIUS = 0.02
_SCENES = {}


def _scene(N, M):
    """three box-surface clouds with different boxes -- as sampled, shifted far from the origin, ten times larger -- and M
    centroids each: cloud points, then m = 0 far outside the box (no hit), m = 1 / 2 outside the box by half a radius, next to
    the border point of largest x / smallest z"""
    if (N, M) not in _SCENES:
        from ga_ddpg_amd.synth_data import box_surface_cloud
        rng = np.random.default_rng(N)
        xyz = np.stack([box_surface_cloud(rng, N, (0.3, 0.2, 0.1)) + 0.25 for _ in range(3)])
        xyz[1] += (100.0, -50.0, 30.0)
        xyz[2] *= 10.0
        xyz = xyz.astype(np.float32)
        ctr = np.stack([xyz[b, rng.choice(N, size=M, replace=False)] for b in range(3)])
        for b in range(3):
            ctr[b, 0] = xyz[b].max(axis=0) + 1000.0
            ctr[b, 1] = xyz[b, xyz[b, :, 0].argmax()] + np.float32([0.5 * RADIUS, 0, 0])
            ctr[b, 2] = xyz[b, xyz[b, :, 2].argmin()] - np.float32([0, 0, 0.5 * RADIUS])
        ctr = ctr.astype(np.float32)
        for b in range(3):
            assert ctr[b, 1, 0] > xyz[b, :, 0].max() and ctr[b, 2, 2] < xyz[b, :, 2].min()
        _SCENES[(N, M)] = (xyz, ctr, _hits(ctr, xyz, RADIUS))
    return _SCENES[(N, M)]


@pytest.mark.parametrize("nsample", [1, 16, 64, 200])
def test_matches_oracle_and_scan(nsample):
    """N = 70000 (past the 65 535 a 16-bit slot map could hold) and then N = 4097 on the SAME workspace buffer; nsample = 200 is
    neither a multiple of 64 nor within the LDS kernels' 128 / 256.  The dense clouds give more hits than nsample (the smallest
    indices have to be selected), the ten times larger one fewer; m = 0 has none, m = 1 / 2 lie outside the box"""
    over = False
    for N, M in [(70000, 64), (4097, 33)]:
        xyz, ctr, hits = _scene(N, M)
        assert (hits[:, 0] == 0).all() and (hits[:, 1:3] >= 1).all()
        assert ((hits > 0) & (hits < nsample)).any() or nsample == 1
        over = over or bool((hits > nsample).any())
        idx, cnt = _check(ctr, xyz, RADIUS, nsample)
        np.testing.assert_array_equal(cnt, np.minimum(hits, nsample))
        assert (idx[:, 0] == 0).all() and (cnt[:, 0] == 0).all()
    assert over                                                   # (about 400 points per ball of the dense clouds at N = 70000)


def test_distances_exactly_on_the_radius_are_excluded():
    """lattice coordinates (multiples of 0.125), radius 0.25: pairs two lattice steps apart along an axis have d2 == r2 exactly
    and fail the strict <"""
    rng = np.random.default_rng(7)
    xyz = (rng.integers(0, 16, size=(2, 4500, 3)) * 0.125).astype(np.float32)
    ctr = xyz[:, :48].copy()
    d = ctr[:, :, None, :] - xyz[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert (d2 == np.float32(0.0625)).sum() > 100                 # pairs exactly on the sphere exist
    hits = _hits(ctr, xyz, 0.25)
    assert (hits > 32).any() and (hits < 32).any()
    idx, cnt = _check(ctr, xyz, 0.25, 32)
    np.testing.assert_array_equal(cnt, np.minimum(hits, 32))
    for b in range(2):
        for m in range(48):
            assert (d2[b, m, idx[b, m, :cnt[b, m]]] < np.float32(0.0625)).all()


@pytest.mark.parametrize("nsample", [16, 200])
def test_more_candidates_than_the_kernel_holds(nsample):
    """5000 points inside a 0.01 cube, radius 0.5: one cell, every point a hit of every centroid -- the answer is the first
    nsample indices"""
    rng = np.random.default_rng(5000)
    xyz = (rng.random((2, 5000, 3)) * 0.01 + 0.3).astype(np.float32)
    ctr = np.concatenate([xyz[:, :19], xyz[:, :1] + np.float32(0.2)], axis=1)
    idx, cnt = _check(ctr, xyz, 0.5, nsample)
    assert (cnt == nsample).all()
    assert (idx == np.arange(nsample, dtype=np.int32)).all()


@pytest.mark.parametrize("kind", ["flat", "one_point"])
def test_degenerate_boxes(kind):
    rng = np.random.default_rng(11)
    xyz = (rng.random((2, 5000, 3)) * 0.5 + 0.1).astype(np.float32)
    if kind == "flat":
        xyz[:, :, 2] = 0.375
        radius = 0.03
    else:
        xyz[:] = np.float32([0.3, -0.2, 0.7])
        radius = 0.05
    ctr = xyz[:, :30].copy()
    ctr[:, 1] += np.float32([0, 0, 0.5 * radius])                   # off the plane / off the point, inside the radius
    ctr[:, 2] += np.float32([0, 0, 2.0 * radius])                   # outside it
    idx, cnt = _check(ctr, xyz, radius, 24)
    assert (cnt[:, 2] == 0).all() and (cnt[:, 1] > 0).all()


def test_non_finite_points_and_centroids():
    """a NaN point, a +inf point and a NaN centroid: none is ever a hit, the box and every other answer are unaffected"""
    rng = np.random.default_rng(13)
    xyz = (rng.random((2, 5000, 3)) * 0.4 + 0.1).astype(np.float32)
    ctr = xyz[:, 100:140].copy()
    clean_idx, clean_cnt = _check(ctr, xyz, 0.04, 32)
    near = clean_idx[0, 5, :2].copy()                              # two neighbours of centroid 5 of cloud 0 ...
    assert clean_cnt[0, 5] >= 2
    xyz[0, near[0], 0] = np.nan                                    # ... turn non-finite
    xyz[0, near[1]] = np.inf
    ctr[1, 7, 1] = np.nan
    idx, cnt = _check(ctr, xyz, 0.04, 32)
    assert not np.isin(idx[0, 5, :cnt[0, 5]], near).any()
    assert cnt[1, 7] == 0 and (idx[1, 7] == 0).all()
    np.testing.assert_array_equal(cnt[1, :7], clean_cnt[1, :7])


def test_nothing_to_search():
    """B * M == 0: GAD_OK without a launch, a NULL workspace is legal and idx stays as it was"""
    from ga_ddpg_amd import hip
    L = hip.lib()
    x = torch.rand(2, 5000, 3, device="cuda")
    c = torch.rand(2, 4, 3, device="cuda")
    idx = torch.full((2, 4, 8), -7, dtype=torch.int32, device="cuda")
    null = C.c_void_p(None)
    args = lambda B, M: (C.c_void_p(c.data_ptr()), C.c_void_p(x.data_ptr()), B, 5000, M, 0.1, 8, C.c_void_p(idx.data_ptr()), null,
                         null, hip.stream())
    assert L.gad_ball_query_grid(*args(2, 0)) == 0
    assert L.gad_ball_query_grid(*args(0, 4)) == 0
    torch.cuda.synchronize()
    assert (idx == -7).all()


def test_degenerate_radius_runs_the_scan():
    """radius 0, negative, NaN and beyond 1e18 have no grid: the entry point runs the scan kernel, right for every radius"""
    rng = np.random.default_rng(17)
    xyz = (rng.random((1, 4200, 3)) * 0.4).astype(np.float32)
    ctr = xyz[:, :8].copy()
    for radius in (0.0, -1.0, float("nan"), 2.0e18):
        idx, cnt = _check(ctr, xyz, radius, 8)
        assert (cnt == (8 if radius * radius > 0.5 else 0)).all()  # (r2 = radius * radius, as the scan forms it: 1 for -1)


def test_facade_routing(monkeypatch):
    """pointnet2_utils.ball_query.  With library option bq_grid = 2 (every cloud beyond the LDS kernels' 4096 points) N = 5000
    reaches gad_ball_query_grid and N = 4096 does not; with bq_grid = 0 the N = 5000 call runs the scan, with equal output.  By
    default (the measured rule) N = 5000 keeps gad_ball_query as well and N = 262144 is the first cloud sent to the grid"""
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    from oracle import cref
    names, real = [], hip.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(hip, "call", spy)

    def run(N, want_name, want_idx=None):
        xyz = (np.random.default_rng(N).random((2, N, 3)) * 0.4 + 0.2).astype(np.float32)
        ctr = np.ascontiguousarray(xyz[:, :40])
        del names[:]
        got = pu.ball_query(0.05, 16, torch.from_numpy(xyz).cuda(), torch.from_numpy(ctr).cuda())
        assert got.dtype == torch.int32 and tuple(got.shape) == (2, 40, 16)
        assert names == [want_name], (N, names)
        got = got.cpu().numpy()
        np.testing.assert_array_equal(got, cref.ball_query(ctr, xyz, 0.05, 16) if want_idx is None else want_idx)
        return got

    try:
        hip.set_option("bq_grid", 2)
        grid_idx = run(5000, "gad_ball_query_grid")
        run(4096, "gad_ball_query")
        hip.set_option("bq_grid", 0)
        run(5000, "gad_ball_query", grid_idx)
        run(262144, "gad_ball_query")
    finally:
        hip.set_option("bq_grid", 1)
    run(5000, "gad_ball_query", grid_idx)
    run(262143, "gad_ball_query")
    run(262144, "gad_ball_query_grid")
