"""The fused set-abstraction path (PointnetSAModule[MSG] with bn=True, use_xyz=True and features) on clouds the one-workgroup
kernels refuse: N > 16384, npoint > N, 3N + npoint beyond the LDS -- the plan then calls gad_fps_tiled and, where
pointnet2_utils.ball_query_uses_grid holds, gad_ball_query_grid (by default from 262 144 points; these tests set library option
bq_grid = 2, every cloud beyond 4096 points, where they mean the grid) -- against the CPU oracle's module, with the tolerances of
tests/test_gpu_facade.py::test_sa_module_gradients_match_oracle; shapes that fitted keep their calls."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_close

pytestmark = pytest.mark.gpu
SEED = 1234
_GEOMETRY = ("gad_furthest_point_sampling", "gad_fps_tiled", "gad_ball_query", "gad_ball_query_grid", "gad_rows_from_ball_query")


def _box_clouds(B, N, seed):
    from ga_ddpg_amd.synth_data import box_surface_cloud
    rng = np.random.default_rng(seed)
    return torch.tensor(np.stack([box_surface_cloud(rng, N, (0.3, 0.2, 0.1)) + 0.25 for _ in range(B)]), dtype=torch.float32)


def _pair(kw, cls="PointnetSAModule", tag="sa"):
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    from oracle.detfill import fill_module_
    from oracle.pointnet2_ops import pointnet2_modules as opm
    ref = fill_module_(getattr(opm, cls)(**kw), tag, SEED).train()
    mine = fill_module_(getattr(pm, cls)(**kw), tag, SEED).cuda().train()
    return mine, ref


def _spy_plan_calls(monkeypatch):
    """names of the entry points the plans of the fused path record"""
    from ga_ddpg_amd import engine
    names, real = [], engine.Plan.call

    def spy(self, name, *a, **k):
        names.append(name)
        return real(self, name, *a, **k)

    monkeypatch.setattr(engine.Plan, "call", spy)
    return names


def _grid_beyond_4096():
    """library option bq_grid = 2 for the length of a with-block"""
    import contextlib
    from ga_ddpg_amd import hip

    @contextlib.contextmanager
    def cm():
        hip.set_option("bq_grid", 2)
        try:
            yield
        finally:
            hip.set_option("bq_grid", 1)
    return cm()


_BIG = {}


def _big():
    """the N = 20000 module after ONE training forward + probe-loss backward on both sides (shared by the tests below)"""
    if not _BIG:
        B, N, C = 2, 20000, 4
        kw = dict(mlp=[C, 16, 32, 32], npoint=128, radius=0.05, nsample=16)
        mine, ref = _pair(kw)
        rng = np.random.default_rng(20000)
        xyz = _box_clouds(B, N, 20000)
        feats = torch.tensor(rng.normal(size=(B, C, N)), dtype=torch.float32)
        probe = torch.tensor(rng.normal(size=(B, 32, 128)), dtype=torch.float32)
        f_ref, f_gpu = feats.clone().requires_grad_(True), feats.cuda().requires_grad_(True)
        x_ref, o_ref = ref(xyz, f_ref)
        (o_ref * probe).sum().backward()
        with _grid_beyond_4096():                                 # (the run's plans are recorded inside the first call)
            x_gpu, o_gpu = mine(xyz.cuda(), f_gpu)                 # (RuntimeError before the fused path routed)
        (o_gpu * probe.cuda()).sum().backward()
        torch.cuda.synchronize()
        _BIG.update(mine=mine, ref=ref, xyz=xyz, feats=feats, f_ref=f_ref, f_gpu=f_gpu, x_ref=x_ref, o_ref=o_ref, x_gpu=x_gpu,
                    o_gpu=o_gpu)
    return _BIG


def test_forward_and_backward_beyond_the_lds_kernels(monkeypatch):
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    assert not pu.fps_fits_one_workgroup(20000, 128) and not pu.ball_query_uses_grid(20000)
    names = _spy_plan_calls(monkeypatch)
    _BIG.clear()
    s = _big()
    assert [n for n in names if n in _GEOMETRY] == ["gad_fps_tiled", "gad_ball_query_grid", "gad_rows_from_ball_query"] * 2
    np.testing.assert_array_equal(s["x_gpu"].cpu().numpy(), s["x_ref"].numpy())
    assert_close(s["o_gpu"].detach().cpu().numpy(), s["o_ref"].detach().numpy(), 1e-4, 2e-5, "SA output")

    def close(a, b, what):
        assert_close(a.cpu().numpy(), b.numpy(), 0.0, 3e-4 * float(b.abs().max()) + 1e-7, what)
    close(s["f_gpu"].grad, s["f_ref"].grad, "d features")
    for (n, a), (_, b) in zip(s["mine"].named_parameters(), s["ref"].named_parameters()):
        close(a.grad, b.grad, "d " + n)


def test_eval_mode_after_a_training_forward(monkeypatch):
    """running statistics after the one training forward, then the eval-mode forward that uses them -- a new run, recorded under
    the default option: tiled sampling and, at 20000 points, the scan"""
    s = _big()
    names = _spy_plan_calls(monkeypatch)
    mine, ref = s["mine"], s["ref"]
    for (n, a), (_, b) in zip(mine.state_dict().items(), ref.state_dict().items()):
        if "running" in n:
            assert_close(a.cpu().numpy(), b.numpy(), 1e-4, 1e-6, n)
        elif "num_batches" in n:
            assert int(a) == int(b), n
    mine.eval(), ref.eval()
    try:
        with torch.no_grad():
            x_ref, e_ref = ref(s["xyz"], s["feats"])
            x_gpu, e_gpu = mine(s["xyz"].cuda(), s["feats"].cuda())
    finally:
        mine.train(), ref.train()
    assert [n for n in names if n in _GEOMETRY] == ["gad_fps_tiled", "gad_ball_query", "gad_rows_from_ball_query"] * 2
    np.testing.assert_array_equal(x_gpu.cpu().numpy(), x_ref.numpy())
    assert_close(e_gpu.cpu().numpy(), e_ref.numpy(), 1e-4, 2e-5, "eval-mode SA output")


def test_more_centroids_than_points():
    """npoint = 40 > N = 32 with bn=True: the fused path (it raised before), centroids exact"""
    B, N, C = 2, 32, 4
    mine, ref = _pair(dict(mlp=[C, 16, 32, 32], npoint=40, radius=0.3, nsample=8))
    g = torch.Generator().manual_seed(32)
    xyz = torch.rand(B, N, 3, generator=g) * 0.5 + 0.2
    feats = torch.randn(B, C, N, generator=g)
    x_ref, o_ref = ref(xyz, feats)
    x_gpu, o_gpu = mine(xyz.cuda(), feats.cuda())
    assert tuple(x_gpu.shape) == (B, 40, 3) and tuple(o_gpu.shape) == (B, 32, 40)
    np.testing.assert_array_equal(x_gpu.cpu().numpy(), x_ref.numpy())
    assert_close(o_gpu.detach().cpu().numpy(), o_ref.detach().numpy(), 1e-4, 2e-5, "SA output")


def test_shape_refused_for_its_lds_sum_only():
    """N = 12000 <= 16384 but 3N + npoint = 41000 words do not fit the LDS: tiled sampling (5000 rounds) and the grid search"""
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    B, N, C = 1, 12000, 4
    assert not pu.fps_fits_one_workgroup(N, 5000)
    mine, ref = _pair(dict(mlp=[C, 16, 32, 32], npoint=5000, radius=0.01, nsample=8))
    xyz = _box_clouds(B, N, 12000)
    feats = torch.tensor(np.random.default_rng(12000).normal(size=(B, C, N)), dtype=torch.float32)
    with torch.no_grad(), _grid_beyond_4096():
        x_ref, o_ref = ref(xyz, feats)
        x_gpu, o_gpu = mine(xyz.cuda(), feats.cuda())
    np.testing.assert_array_equal(x_gpu.cpu().numpy(), x_ref.numpy())
    assert_close(o_gpu.cpu().numpy(), o_ref.numpy(), 1e-4, 2e-5, "SA output")


def test_two_scales_share_their_centroids():
    """PointnetSAModuleMSG at N = 20000: each scale's fused pass samples again and reports the same new_xyz; the channels are
    concatenated in scale order"""
    from ga_ddpg_amd.sa_function import sa_module_forward
    B, N, C = 2, 20000, 4
    kw = dict(npoint=64, radii=[0.03, 0.06], nsamples=[8, 16], mlps=[[C, 16, 16, 32], [C, 16, 32, 64]])
    mine, ref = _pair(kw, "PointnetSAModuleMSG", "msg")
    xyz = _box_clouds(B, N, 20001)
    feats = torch.tensor(np.random.default_rng(20001).normal(size=(B, C, N)), dtype=torch.float32)
    with torch.no_grad(), _grid_beyond_4096():
        x_ref, o_ref = ref(xyz, feats)
        x_gpu, o_gpu = mine(xyz.cuda(), feats.cuda())
        per_scale = [sa_module_forward(sc, xyz.cuda(), feats.cuda()) for sc in mine._scales]
    assert tuple(o_gpu.shape) == (B, 96, 64)
    for x_sc, _ in per_scale:
        np.testing.assert_array_equal(x_sc.cpu().numpy(), x_ref.numpy())
    np.testing.assert_array_equal(x_gpu.cpu().numpy(), x_ref.numpy())
    assert_close(o_gpu.cpu().numpy(), o_ref.numpy(), 1e-4, 2e-5, "MSG output")


def test_old_shapes_keep_their_calls(monkeypatch):
    """N = 1024, npoint = 128: the recorded plans name the entry points they named before the routing, and the output is the
    oracle's within the existing tolerance"""
    names = _spy_plan_calls(monkeypatch)
    B, N, C = 2, 1024, 4
    mine, ref = _pair(dict(mlp=[C, 16, 32, 32], npoint=128, radius=0.05, nsample=16))
    xyz = _box_clouds(B, N, 1024)
    feats = torch.tensor(np.random.default_rng(1024).normal(size=(B, C, N)), dtype=torch.float32)
    x_ref, o_ref = ref(xyz, feats)
    x_gpu, o_gpu = mine(xyz.cuda(), feats.cuda())
    assert [n for n in names if n in _GEOMETRY] == ["gad_furthest_point_sampling", "gad_ball_query", "gad_rows_from_ball_query"] * 2
    np.testing.assert_array_equal(x_gpu.cpu().numpy(), x_ref.numpy())
    assert_close(o_gpu.detach().cpu().numpy(), o_ref.detach().numpy(), 1e-4, 2e-5, "SA output")
