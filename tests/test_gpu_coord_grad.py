"""Coordinate gradients of the fused set-abstraction path (module switch `coordinate_grad`, entry point gad_sa_coord_grad).

1. the entry point alone against float64 numpy on hand-built row lists, every element inside the worst-case float32 sum bound of
   tests/gemm_cases.py: |got - ref| <= (T + 6) * 2^-24 * sum|terms|, T = the f32 products summed into the element, terms =
   |P g W| + |w S z W| + |w Q W| of every row that reaches the element, + |g_new_xyz| of every group centred on it, + the
   pre-fill (the call ADDS into dxyz, so what it finds there is one more summand of the same float32 sum).  The 6 covers the four
   roundings inside dZ, the product and the centroid subtraction.
2. - 5. modules against the CPU oracle (oracle.pointnet2_ops: plain indexing, so torch autograd differentiates xyz), gate
   3e-4 * max|ref| + 1e-7 per tensor -- test_gpu_facade.test_sa_module_gradients_match_oracle's yardstick for the same free-running
   comparison (room for a ReLU / arg-max decision that rounds the other way).
6. - 7. the switch off is today's behaviour; refusals.

Largest err / bound seen on an MI355X in test 1: 0.058 (8 channels; 0.002 at 128)."""
import contextlib

import numpy as np
import pytest
import torch

from tests.helpers import assert_close

pytestmark = pytest.mark.gpu
SEED = 1234
U = 2.0 ** -24
GUARD = 64            # floats of guard in front of and behind every output


def _round8(k):
    return (k + 7) // 8 * 8


class _Case(object):
    """rows built by hand: cap static rows of which `live` are live; groups are runs of rows; the collisions of the docstring"""

    def __init__(self, n_out, col0, cap=300, live=261, n_pts=100, sizes=(1, 50, 3, 64, 17, 30, 2, 40, 20, 10, 5, 19), seed=0):
        rng = np.random.default_rng(1000 * n_out + col0 + seed)
        self.n_out, self.col0, self.Kp, self.cap, self.live, self.n_pts = n_out, col0, _round8(col0 + 3), cap, live, n_pts
        assert sum(sizes) == live <= cap
        G = self.G = len(sizes)
        used = n_pts * 4 // 5                                         # points [used, n_pts) are in no row and no centroid
        pt, grp = [], []
        for g, s in enumerate(sizes):
            p = rng.choice(np.arange(8, used), size=s, replace=False)
            if s >= 2:
                p[0] = 7                                              # point 7: hit by every group of two rows or more
            pt += list(p)
            grp += [g] * s
        ctr = rng.integers(8, used, size=G)
        pt[0] = 3
        ctr[0] = 3                                                    # group 0: one row, and that point is its own centroid
        ctr[2] = ctr[1]                                               # two groups share a centroid point
        ctr[3] = 7                                                    # the busy point is a centroid as well
        # dead rows: a point nothing else touches and a valid group -- were they read, their NaNs would land where the test looks
        self.row_pt = np.array(pt + [n_pts - 1] * (cap - live), dtype=np.int32)
        self.row_grp = np.array(grp + [G - 1] * (cap - live), dtype=np.int32)
        self.ctr = ctr.astype(np.int32)
        self.W = rng.normal(size=(n_out, self.Kp)).astype(np.float32)       # neighbouring columns non-zero: they must not leak in
        self.P = rng.uniform(0.5, 2.0, n_out).astype(np.float32) * rng.choice([-1.0, 1.0], n_out).astype(np.float32)
        self.Q = rng.normal(size=n_out).astype(np.float32) * 0.3
        self.S = rng.normal(size=n_out).astype(np.float32) * 0.2
        self.w = rng.choice([1.0, 1.0, 3.0, 7.0], size=cap).astype(np.float32)
        self.Gm = rng.normal(size=(cap, n_out)).astype(np.float32)
        self.z = rng.normal(size=(cap, n_out)).astype(np.float32)
        self.Gm[live:] = np.nan
        self.z[live:] = np.nan
        self.g_new = rng.normal(size=(G, 3)).astype(np.float32)
        self.prefill = (0.25 + 0.01 * np.arange(n_pts * 3)).reshape(n_pts, 3).astype(np.float32)

    def reference(self, live=None, grouped=True, g_new=True, drop_centroids=False, col0=None):
        """(ref, bound) in float64 from the float32 operands; the keyword variants are the negative controls"""
        live = self.live if live is None else live
        col0 = self.col0 if col0 is None else col0
        f = np.float64
        Gm, z, w = self.Gm[:live].astype(f), self.z[:live].astype(f), self.w[:live].astype(f)[:, None]
        P, Q, S = self.P.astype(f), self.Q.astype(f), self.S.astype(f)
        W3 = self.W[:, col0:col0 + 3].astype(f)
        t = (P * Gm - w * (S * z + Q)) @ W3
        mag = (np.abs(P * Gm) + np.abs(w * S * z) + np.abs(w * Q)) @ np.abs(W3)
        ref, tot, cnt = self.prefill.astype(f), np.abs(self.prefill).astype(f), np.zeros((self.n_pts, 3))
        np.add.at(ref, self.row_pt[:live], t)
        np.add.at(tot, self.row_pt[:live], mag)
        np.add.at(cnt, self.row_pt[:live], float(self.n_out))
        if grouped and not drop_centroids:
            dctr, mctr, nctr = np.zeros((self.G, 3)), np.zeros((self.G, 3)), np.zeros((self.G, 3))
            np.add.at(dctr, self.row_grp[:live], t)
            np.add.at(mctr, self.row_grp[:live], mag)
            np.add.at(nctr, self.row_grp[:live], float(self.n_out))
            up = self.g_new.astype(f) if g_new else np.zeros((self.G, 3))
            np.add.at(ref, self.ctr, up - dctr)
            np.add.at(tot, self.ctr, np.abs(up) + mctr)
            np.add.at(cnt, self.ctr, nctr)
        return ref, (cnt + 6.0) * U * tot

    def touched(self, live=None, grouped=True):
        live = self.live if live is None else live
        m = np.zeros(self.n_pts, dtype=bool)
        m[self.row_pt[:live]] = True
        if grouped:
            m[self.ctr] = True
        return m

    def run(self, live=None, grouped=True, g_new=True):
        """-> dxyz (n_pts, 3) as the entry point leaves it; guards, and dctr against its own reference, are checked here"""
        from ga_ddpg_amd import hip
        live = self.live if live is None else live
        dev = "cuda"

        def guarded(a):
            buf = torch.full((a.size + 2 * GUARD,), -777.25, dtype=torch.float32, device=dev)
            buf[GUARD:GUARD + a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
            return buf
        t = {k: torch.from_numpy(getattr(self, k)).to(dev) for k in ("W", "P", "Q", "S", "w", "Gm", "z", "row_pt", "row_grp", "ctr", "g_new")}
        n_dev = torch.tensor([live], dtype=torch.int32, device=dev)
        dxyz = guarded(self.prefill)
        dctr = guarded(np.zeros((self.G, 3), dtype=np.float32))      # the contract: the caller clears dctr
        d = hip.DzSrc()
        d.z, d.z_pitch, d.G, d.g_pitch, d.c = t["z"].data_ptr(), self.n_out, t["Gm"].data_ptr(), self.n_out, self.n_out
        d.coefP, d.coefQ, d.coefS, d.row_w = t["P"].data_ptr(), t["Q"].data_ptr(), t["S"].data_ptr(), t["w"].data_ptr()
        d.gmode, d.relu, d.premasked = 0, 1, 1
        mid = lambda b: hip.Ptr(b.data_ptr() + 4 * GUARD)
        hip.call("gad_sa_coord_grad", d, t["W"], self.Kp, self.n_out, self.col0, n_dev, self.cap, t["row_pt"],
                 t["row_grp"] if grouped else None, t["ctr"] if grouped else None, t["g_new"] if (grouped and g_new) else None,
                 self.G, self.n_pts, mid(dxyz), mid(dctr) if grouped else None)
        torch.cuda.synchronize()
        for name, b in (("dxyz", dxyz), ("dctr", dctr)):
            b = b.cpu().numpy()
            assert (b[:GUARD] == -777.25).all() and (b[-GUARD:] == -777.25).all(), name + ": guard bytes written"
        got_ctr = dctr.cpu().numpy()[GUARD:-GUARD].reshape(self.G, 3)
        if grouped and live:
            f = np.float64
            tt = (self.P.astype(f) * self.Gm[:live] - self.w[:live, None].astype(f) * (self.S.astype(f) * self.z[:live] + self.Q)) \
                @ self.W[:, self.col0:self.col0 + 3].astype(f)
            want = np.zeros((self.G, 3))
            np.add.at(want, self.row_grp[:live], tt)
            assert np.isfinite(got_ctr).all() and np.abs(got_ctr - want).max() <= 1e-3 * max(1.0, np.abs(want).max()), "dctr: the group sums"
        else:
            assert (got_ctr == 0).all()
        return dxyz.cpu().numpy()[GUARD:-GUARD].reshape(self.n_pts, 3)


def _ratio(got, ref, bound):
    assert np.isfinite(got).all(), "NaN / inf: a dead row was read"
    return float((np.abs(got.astype(np.float64) - ref) / bound).max())


WORST = [0.0]

# (n_out, col0) of the issue: float4 rows with 2, 8, 16 and 32 lanes per row; then this kernel's other paths: the scalar form
# (n_out % 4 != 0), a sub-group that walks its row in two steps (24 channels: 6 float4s over 4 lanes), 64 lanes per row
LAYERS = [(n, c) for n in (8, 32, 64, 128) for c in (4, 12)] + [(6, 4), (24, 12), (256, 4)]


@pytest.mark.parametrize("n_out,col0", LAYERS)
def test_entry_point_against_float64(n_out, col0):
    c = _Case(n_out, col0)
    # ---- grouped form: rows + centroids + the incoming gradient of new_xyz ----
    got = c.run()
    ref, bound = c.reference()
    r = _ratio(got, ref, bound)
    WORST[0] = max(WORST[0], r)
    print("n_out %d col0 %d: grouped max err / bound %.3f" % (n_out, col0, r))
    assert r <= 1.0
    idle = ~c.touched()
    assert idle.sum() >= 10 and (got[idle].view(np.uint32) == c.prefill[idle].view(np.uint32)).all(), "untouched elements changed"
    # negative controls: each of these references must be REJECTED by the same gate
    for what, kw in (("centroid term dropped", dict(drop_centroids=True)), ("last live row dropped", dict(live=c.live - 1)),
                     ("column col0 - 1 read", dict(col0=c.col0 - 1))):
        bad, _ = c.reference(**kw)
        assert _ratio(got, bad, bound) > 1.0, what + ": the gate does not see it"
    # ---- without g_new_xyz ----
    got = c.run(g_new=False)
    ref, bound = c.reference(g_new=False)
    r = _ratio(got, ref, bound)
    WORST[0] = max(WORST[0], r)
    assert r <= 1.0
    # ---- GroupAll form: no centroid terms ----
    got = c.run(grouped=False)
    ref, bound = c.reference(grouped=False)
    r = _ratio(got, ref, bound)
    WORST[0] = max(WORST[0], r)
    print("n_out %d col0 %d: group-all max err / bound %.3f (worst so far %.3f)" % (n_out, col0, r, WORST[0]))
    assert r <= 1.0
    idle = ~c.touched(grouped=False)
    assert (got[idle].view(np.uint32) == c.prefill[idle].view(np.uint32)).all()
    # ---- a live count of 0 changes nothing (no incoming gradient: the centroids then receive 0 - 0) ----
    for grouped in (True, False):
        got = c.run(live=0, grouped=grouped, g_new=False)
        assert (got.view(np.uint32) == c.prefill.view(np.uint32)).all(), "live count 0 changed dxyz"


def test_entry_point_grid_stride_and_static_count():
    """more slabs of rows than the launch has workgroups (256 channels: 4 rows per workgroup, 2048 workgroups at the most)"""
    rng = np.random.default_rng(9)
    sizes, left = [], 9000
    while left:
        s = int(min(left, rng.integers(1, 65)))
        sizes.append(s)
        left -= s
    c = _Case(256, 4, cap=9100, live=9000, n_pts=400, sizes=tuple(sizes), seed=1)
    got = c.run()
    ref, bound = c.reference()
    r = _ratio(got, ref, bound)
    print("grid-stride case: max err / bound %.3f" % r)
    assert r <= 1.0
    bad, _ = c.reference(live=c.live - 1)
    assert _ratio(got, bad, bound) > 1.0


# ----------------------------------------------------------------------------------------------------------------------------------
# modules against the CPU oracle
# ----------------------------------------------------------------------------------------------------------------------------------
def _pair(kw, cls="PointnetSAModule", tag="sa", seed=SEED, **mine_kw):
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    from oracle.detfill import fill_module_
    from oracle.pointnet2_ops import pointnet2_modules as opm
    ref = fill_module_(getattr(opm, cls)(**kw), tag, seed).train()
    mine = fill_module_(getattr(pm, cls)(coordinate_grad=True, **kw, **mine_kw), tag, seed).cuda().train()
    return mine, ref


def _close(a, b, what):
    assert_close(a.detach().cpu().numpy(), b.detach().numpy(), 0.0, 3e-4 * float(b.abs().max()) + 1e-7, what)


def _check_module(mine, ref, xyz, feats, probe, probe2, frozen_twin=None):
    x_ref, f_ref = xyz.clone().requires_grad_(True), feats.clone().requires_grad_(True)
    x_gpu, f_gpu = xyz.cuda().requires_grad_(True), feats.cuda().requires_grad_(True)
    nr, o_ref = ref(x_ref, f_ref)
    ng, o_gpu = mine(x_gpu, f_gpu)
    loss_r, loss_g = (o_ref * probe).sum(), (o_gpu * probe.cuda()).sum()
    if nr is not None:
        assert ng.requires_grad
        np.testing.assert_array_equal(ng.detach().cpu().numpy(), nr.detach().numpy())
        loss_r, loss_g = loss_r + (nr * probe2).sum(), loss_g + (ng * probe2.cuda()).sum()
    loss_r.backward()
    loss_g.backward()
    assert_close(o_gpu.detach().cpu().numpy(), o_ref.detach().numpy(), 1e-4, 2e-5, "SA output")
    assert float(x_ref.grad.abs().max()) > 0
    _close(x_gpu.grad, x_ref.grad, "d xyz")
    _close(f_gpu.grad, f_ref.grad, "d features")
    for (n, a), (_, b) in zip(mine.named_parameters(), ref.named_parameters()):
        _close(a.grad, b.grad, "d " + n)
    if frozen_twin is not None:                # features and parameters frozen: the call differentiates for xyz alone
        for p in frozen_twin.parameters():
            p.requires_grad_(False)
        x2 = xyz.cuda().requires_grad_(True)
        n2, o2 = frozen_twin(x2, feats.cuda())
        assert o2.requires_grad
        l2 = (o2 * probe.cuda()).sum()
        if n2 is not None:
            l2 = l2 + (n2 * probe2.cuda()).sum()
        l2.backward()
        _close(x2.grad, x_ref.grad, "d xyz (features and parameters frozen)")
    return x_gpu.grad.cpu().numpy(), x_ref.grad.numpy()


@pytest.mark.parametrize("group_all,C", [(False, 8), (False, 10), (True, 5)])
def test_one_module_matches_oracle(group_all, C):
    from oracle.pointnet2_ops import pointnet2_utils as opu
    rng = np.random.default_rng(3)
    B, N = 4, 512
    kw = dict(mlp=[C, 32, 64, 64]) if group_all else dict(npoint=32, radius=0.08, nsample=32, mlp=[C, 32, 64, 64])
    mine, ref = _pair(kw)
    twin, _ = _pair(kw)
    xyz = torch.tensor(rng.random((B, N, 3)) * 0.3 + 0.2, dtype=torch.float32)
    feats = torch.tensor(rng.normal(size=(B, C, N)), dtype=torch.float32)
    probe = torch.tensor(rng.normal(size=(B, 64, 1 if group_all else 32)), dtype=torch.float32)
    probe2 = torch.tensor(rng.normal(size=(B, 32, 3)), dtype=torch.float32)
    got, want = _check_module(mine, ref, xyz, feats, probe, probe2, frozen_twin=twin)
    if not group_all:
        # a point that no neighbourhood contains and that is no centroid receives exactly 0
        fps = opu.furthest_point_sample(xyz, 32)
        new_xyz = torch.gather(xyz, 1, fps.long().unsqueeze(-1).expand(B, 32, 3))
        idx = opu.ball_query(0.08, 32, xyz, new_xyz)
        hit = np.zeros((B, N), dtype=bool)
        for b in range(B):
            hit[b, idx[b].numpy().ravel()] = True
            hit[b, fps[b].numpy()] = True
        assert 0.03 < (~hit).mean() < 0.3, (~hit).mean()
        assert (got[~hit] == 0).all() and (want[~hit] == 0).all()
        assert (np.abs(got[hit]).max(axis=-1) > 0).mean() > 0.9


def _stack(flags):
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    from oracle.detfill import fill_module_
    from oracle.pointnet2_ops import pointnet2_modules as opm
    kws = [dict(npoint=32, radius=0.1, nsample=16, mlp=[4, 16, 16, 32]), dict(npoint=8, radius=0.2, nsample=8, mlp=[32, 32, 32, 64]),
           dict(mlp=[64, 64, 64, 64])]
    ref = [fill_module_(opm.PointnetSAModule(**kw), "sa%d" % i, SEED + i).train() for i, kw in enumerate(kws)]
    mine = [fill_module_(pm.PointnetSAModule(coordinate_grad=f, **kw), "sa%d" % i, SEED + i).cuda().train()
            for i, (kw, f) in enumerate(zip(kws, flags))]
    return mine, ref


def _run_stack(mods, xyz, feats, probe):
    x = xyz.requires_grad_(True)
    cur, f = x, feats
    for m in mods:
        cur, f = m(cur, f)
    (f * probe).sum().backward()
    return x.grad


def test_stack_of_three_modules():
    """N 256 -> 32 -> 8 -> group-all (the reference's encoder shape in small); only the input xyz asks for a gradient: what the
    second and third module contribute reaches it through new_xyz"""
    rng = np.random.default_rng(5)
    B, N = 3, 256
    xyz = torch.tensor(rng.random((B, N, 3)) * 0.3 + 0.2, dtype=torch.float32)
    feats = torch.tensor(rng.normal(size=(B, 4, N)), dtype=torch.float32)
    probe = torch.tensor(rng.normal(size=(B, 64, 1)), dtype=torch.float32)
    mine, ref = _stack([True, True, True])
    for m in mine + ref:
        for p in m.parameters():
            p.requires_grad_(False)
    want = _run_stack(ref, xyz.clone(), feats, probe)
    got = _run_stack(mine, xyz.cuda(), feats.cuda(), probe.cuda())
    _close(got, want, "d xyz through the stack")
    # the middle module's switch off: its share (and the third module's, which reaches xyz through it) is gone
    cut, _ = _stack([True, False, True])
    for m in cut:
        for p in m.parameters():
            p.requires_grad_(False)
    less = _run_stack(cut, xyz.cuda(), feats.cuda(), probe.cuda())
    scale = float(want.abs().max())
    assert float((less.cpu() - want).abs().max()) > 1e-2 * scale, "the path through new_xyz is not live"


def test_multi_scale_module():
    kw = dict(npoint=16, radii=[0.15, 0.3], nsamples=[16, 32], mlps=[[4, 16, 16, 32], [4, 16, 32, 64]])
    mine, ref = _pair(kw, cls="PointnetSAModuleMSG", tag="msg", seed=7)
    rng = np.random.default_rng(2)
    xyz = torch.tensor(rng.random((3, 256, 3)), dtype=torch.float32)
    feats = torch.tensor(rng.normal(size=(3, 4, 256)), dtype=torch.float32)
    probe = torch.tensor(rng.normal(size=(3, 96, 16)), dtype=torch.float32)
    probe2 = torch.tensor(rng.normal(size=(3, 16, 3)), dtype=torch.float32)
    _check_module(mine, ref, xyz, feats, probe, probe2)


@contextlib.contextmanager
def _option(name, value):
    from ga_ddpg_amd import hip
    was = hip.get_option(name)
    hip.set_option(name, value)
    try:
        yield
    finally:
        hip.set_option(name, was)


@pytest.mark.parametrize("N", [4500, 17000])
def test_cloud_beyond_the_lds_kernels(monkeypatch, N):
    """bq_grid = 2 sends both clouds to the grid ball query; 4500 points still fit gad_furthest_point_sampling's LDS (its limit
    is 16384 points), 17000 take the tiled sampling.  Every route produces the same fps / row lists, so nothing else routes"""
    from ga_ddpg_amd import engine
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    names, real = [], engine.Plan.call

    def spy(self, name, *a, **k):
        names.append(name)
        return real(self, name, *a, **k)
    monkeypatch.setattr(engine.Plan, "call", spy)
    B, C = 2, 4
    mine, ref = _pair(dict(mlp=[C, 16, 32, 32], npoint=64, radius=0.05, nsample=16))
    rng = np.random.default_rng(N)
    xyz = torch.tensor(rng.random((B, N, 3)) * 0.3 + 0.2, dtype=torch.float32)
    feats = torch.tensor(rng.normal(size=(B, C, N)), dtype=torch.float32)
    probe = torch.tensor(rng.normal(size=(B, 32, 64)), dtype=torch.float32)
    probe2 = torch.tensor(rng.normal(size=(B, 64, 3)), dtype=torch.float32)
    with _option("bq_grid", 2):
        assert pu.fps_fits_one_workgroup(N, 64) == (N == 4500) and pu.ball_query_uses_grid(N)
        _check_module(mine, ref, xyz, feats, probe, probe2)
    assert ("gad_fps_tiled" in names) == (N == 17000) and ("gad_furthest_point_sampling" in names) == (N == 4500)
    assert "gad_ball_query_grid" in names and names.count("gad_sa_coord_grad") == 1


def test_more_centroids_than_points():
    """npoint 32 > N 20 (radius 0.2, nsample 8): several groups are centred on one point, whose gradient collects all of them.
    Layer widths [4, 16, 16, 32], not the [4, 8, 8, 8] the case was first written with: the fused backward has never taken fewer
    than 32 pooled channels, switch or no switch (gad_pool_bwd_stats: C a multiple of 32; tests/test_gpu_layer_kernels.py pins
    C = 16 as GAD_ERR_SHAPE), so that shape has no backward to compare -- the end of this test pins that it is refused by name."""
    B, N, C = 2, 20, 4
    mine, ref = _pair(dict(mlp=[C, 16, 16, 32], npoint=32, radius=0.2, nsample=8))
    g = torch.Generator().manual_seed(20)
    xyz = torch.rand(B, N, 3, generator=g) * 0.5 + 0.2
    feats = torch.randn(B, C, N, generator=g)
    probe = torch.randn(B, 32, 32, generator=g)
    probe2 = torch.randn(B, 32, 3, generator=g)
    _check_module(mine, ref, xyz, feats, probe, probe2)
    narrow, _ = _pair(dict(mlp=[C, 8, 8, 8], npoint=32, radius=0.2, nsample=8))
    new_xyz, out = narrow(xyz.cuda().requires_grad_(True), feats.cuda())
    assert new_xyz.requires_grad and tuple(out.shape) == (B, 8, 32)
    with pytest.raises(RuntimeError, match="pool_bwd_stats: C=8"):
        out.sum().backward()


def test_switch_off_is_todays_behaviour(monkeypatch):
    from ga_ddpg_amd import engine
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    names, real = [], engine.Plan.call

    def spy(self, name, *a, **k):
        names.append(name)
        return real(self, name, *a, **k)
    monkeypatch.setattr(engine.Plan, "call", spy)
    mine = pm.PointnetSAModule(npoint=8, radius=0.1, nsample=8, mlp=[4, 16, 16, 32]).cuda().train()
    assert mine.coordinate_grad is False
    xyz = torch.rand(2, 64, 3, device="cuda").requires_grad_(True)
    feats = torch.rand(2, 4, 64, device="cuda", requires_grad=True)
    new_xyz, out = mine(xyz, feats)
    assert not new_xyz.requires_grad and out.requires_grad
    out.sum().backward()
    assert xyz.grad is None and feats.grad is not None
    assert "gad_gemm_dx" in names and "gad_sa_coord_grad" not in names


def test_refusals():
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.pointnet2_ops import pointnet2_modules as pm
    mine = pm.PointnetSAModule(npoint=8, radius=0.1, nsample=8, mlp=[4, 16, 16, 32], coordinate_grad=True).cuda()
    xyz = torch.rand(2, 64, 3, device="cuda").requires_grad_(True)
    feats = torch.rand(2, 4, 64, device="cuda")
    for p in mine.parameters():
        p.requires_grad_(False)
    mine.eval()
    with pytest.raises(RuntimeError, match="eval-mode"):
        mine(xyz, feats)
    mine.train()
    with _option("deterministic", 1):
        with pytest.raises(RuntimeError, match="deterministic"):
            mine(xyz, feats)
        with torch.no_grad():
            mine(xyz, feats)                   # nothing to differentiate: the switch changes nothing
    assert hip.get_option("deterministic") == 0
    with torch.no_grad():
        new_xyz, out = mine(xyz, feats)
    assert not new_xyz.requires_grad and not out.requires_grad
    mine.eval()
    with torch.no_grad():
        mine(xyz, feats)
    mine.train()
    new_xyz, out = mine(xyz, feats)            # and with gradients it is live again
    assert new_xyz.requires_grad and out.requires_grad
    (out.sum() + new_xyz.sum()).backward()
    assert xyz.grad is not None and bool(torch.isfinite(xyz.grad).all())
