"""gad_fps_tiled (include/gaddpg.h section A): furthest point sampling of clouds that do not fit one workgroup, and of
npoint > N, against the CPU oracle -- indices bit for bit -- directly, through pointnet2_utils.furthest_point_sample's routing,
through core.utils.regularize_pc_point_count and through the generic PointnetSAModule path.  The shapes are the smallest at which
each mechanism can go wrong: slices cut at places that are no multiple of 64 or of the tie block, ties and skipped runs across
slice boundaries, more picks than points, and the two kinds of shape the LDS kernel refuses."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _tiled(xyz, M, groups, with_new_xyz=True):
    """a direct call of the entry point -> (idx, new_xyz | None) as numpy arrays"""
    from ga_ddpg_amd import hip
    B, N, _ = xyz.shape
    x = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).cuda()
    nbytes = hip.lib().gad_fps_tiled_workspace_bytes(B, N, M, groups)
    assert nbytes >= B * N * 4
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    idx = torch.full((B, M), -7, dtype=torch.int32, device="cuda")
    new_xyz = torch.full((B, M, 3), float("nan"), device="cuda") if with_new_xyz else None
    hip.call("gad_fps_tiled", x, B, N, M, groups, idx, new_xyz, ws)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), (new_xyz.cpu().numpy() if with_new_xyz else None)


def _check_direct(xyz, M, groups):
    from oracle import cref
    want = cref.fps(xyz, M)
    got, new_xyz = _tiled(xyz, M, groups)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(new_xyz, np.take_along_axis(xyz, want[:, :, None].astype(np.int64), axis=1))
    return got


def _lattice(N):
    """the cloud of tests/test_gpu_ops.py::test_fps_exact_ties_on_a_lattice: almost every round has exact ties"""
    rng = np.random.default_rng(N)
    xyz = (rng.integers(0, 6, size=(3, N, 3)).astype(np.float32) * 0.125 + 0.25)
    xyz[1, N // 2:] = xyz[1, : N - N // 2]                      # every point twice
    xyz[2, ::7] = 0.0                                           # a seventh of the cloud inside the skip ball
    return xyz


@pytest.mark.parametrize("groups", [1, 3, 7])
def test_slices_cut_at_awkward_places(groups):
    """N = 1000 in 1, 3 (334 points) or 7 (143 points) slices: no slice is a multiple of 64, the tie block is 512"""
    xyz = np.random.default_rng(1000).random((2, 1000, 3)).astype(np.float32)
    _check_direct(xyz, 64, groups)


@pytest.mark.parametrize("N,groups", [(1024, 4), (300, 5)])
def test_exact_ties_across_slice_boundaries(N, groups):
    """the winner of a tie is decided by the bit-reversed index inside the tie block (512 / 256), which the cross-workgroup
    maximum has to respect exactly as the one inside a workgroup"""
    _check_direct(_lattice(N), 48, groups)


def test_skip_rule_across_a_slice_boundary():
    """slices of 67 points: point 0 and the run 60..75 (over the boundary at 67) lie inside the skip ball and are never picked
    although they are the farthest from the rest, a tight cluster; the point whose |p|^2 is the float nearest 0.001 (above the
    double 1e-3) is kept -- it is farther from point 0 (d^2 = 3.2e-3) than the cluster is wide (d^2 < 2.7e-3), so it is the third
    pick -- and the float below it is skipped"""
    from tests.test_oracle_ops import edge_points
    edge, below = edge_points()
    rng = np.random.default_rng(200)
    xyz = (rng.random((2, 200, 3)) * 0.03 + 0.5).astype(np.float32)
    xyz[:, 0] = (-0.018, -0.018, 0.0)
    xyz[:, 60:76] = (rng.random((2, 16, 3)) * 0.015).astype(np.float32)          # |p|^2 < 3 * 0.015^2 = 6.75e-4
    xyz[:, 130] = 0.0
    xyz[:, 130, :2] = edge
    xyz[:, 140] = 0.0
    xyz[:, 140, :2] = below
    got = _check_direct(xyz, 16, 3)
    assert not np.isin(got[:, 1:], [0, 140] + list(range(60, 76))).any()
    assert (got[:, 2] == 130).all()


def test_every_point_skipped_gives_index_zero():
    xyz = (np.random.default_rng(3).random((2, 200, 3)) * 0.015).astype(np.float32)
    got = _check_direct(xyz, 16, 3)
    assert (got == 0).all()


@pytest.mark.parametrize("N,M", [(64, 100), (5, 12)])
def test_more_picks_than_points(N, M):
    """npoint > N, as upstream accepts it: once every distance is 0 the tie rule picks the index.  Through the facade (which
    raised before gad_fps_tiled existed) and directly with two slices"""
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    from oracle import cref
    xyz = (np.random.default_rng(N).random((2, N, 3)) * 0.5 + 0.2).astype(np.float32)
    want = cref.fps(xyz, M)
    got = pu.furthest_point_sample(torch.from_numpy(xyz).cuda(), M)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, M)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    _check_direct(xyz, M, 2)


def _box_clouds(B, N, seed):
    from ga_ddpg_amd.synth_data import box_surface_cloud
    rng = np.random.default_rng(seed)
    return np.stack([box_surface_cloud(rng, N, (0.3, 0.2, 0.1)) + 0.25 for _ in range(B)]).astype(np.float32)


@pytest.mark.parametrize("B,N,M", [(1, 20000, 128), (2, 12000, 5000)])
def test_routed_large_cloud(B, N, M):
    """shapes the LDS kernel refuses (N > 16384; 3N + M > 40 896) go to gad_fps_tiled through the facade; the second runs 5000
    rounds, the last of them on a nearly exhausted cloud"""
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    from oracle import cref
    assert not pu.fps_fits_one_workgroup(N, M)
    xyz = _box_clouds(B, N, N)
    got = pu.furthest_point_sample(torch.from_numpy(xyz).cuda(), M).cpu().numpy()
    np.testing.assert_array_equal(got, cref.fps(xyz, M))


@pytest.mark.parametrize("N,M", [(1024, 32), (4096, 512)])
def test_routing_leaves_old_shapes_alone(N, M, monkeypatch):
    """shapes that worked before keep their entry point (gad_furthest_point_sampling does not register with gad_last_kernel, so
    the facade's calls are recorded instead)"""
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    from oracle import cref
    names, real = [], hip.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(hip, "call", spy)
    xyz = (np.random.default_rng(N).random((2, N, 3)) * 0.4 + 0.2).astype(np.float32)
    got = pu.furthest_point_sample(torch.from_numpy(xyz).cuda(), M).cpu().numpy()
    assert names == ["gad_furthest_point_sampling"]
    np.testing.assert_array_equal(got, cref.fps(xyz, M))


def test_regularize_pc_point_count_with_furthest_points():
    from ga_ddpg_amd.core.utils import regularize_pc_point_count
    from oracle import cref
    rng = np.random.default_rng(3000)
    pc = np.concatenate([rng.random((3000, 3)) * 0.5 + 0.2, rng.integers(0, 3, size=(3000, 1))], axis=1)
    assert pc.dtype == np.float64
    out = regularize_pc_point_count(pc, 1024, use_farthest_point=True)
    pc32 = pc.astype(np.float32)
    want = pc32[cref.fps(pc32[None, :, :3], 1024)[0]]
    assert out.shape == (1024, 4) and out.dtype == np.float32
    np.testing.assert_array_equal(out, want)


def test_generic_module_path_takes_npoint_beyond_n():
    """PointnetSAModule(bn=False) takes upstream's composition over this package's operators: with npoint = 40 > N = 32 it returns
    the centroids of the CPU restatement of upstream's module"""
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    from oracle.detfill import fill_module_
    from oracle.pointnet2_ops import pointnet2_modules as om
    g = torch.Generator().manual_seed(32)
    xyz = torch.rand(2, 32, 3, generator=g) * 0.5 + 0.2
    feats = torch.randn(2, 4, 32, generator=g)
    kw = dict(mlp=[4, 8], npoint=40, radius=0.3, nsample=8, bn=False)
    mine, ref = pm.PointnetSAModule(**kw), om.PointnetSAModule(**kw)
    fill_module_(mine, "sa", 3)
    fill_module_(ref, "sa", 3)
    xr, outr = ref(xyz, feats)
    xm, outm = mine.cuda()(xyz.cuda(), feats.cuda())
    assert tuple(xm.shape) == (2, 40, 3)
    np.testing.assert_array_equal(xm.cpu().numpy(), xr.numpy())
    np.testing.assert_allclose(outm.detach().cpu().numpy(), outr.detach().numpy(), rtol=1e-4, atol=1e-5)
