"""Depth frame -> point state on the GPU (include/gaddpg.h section A.2, core/point_state.py) against the numpy restatements of
tests/point_state_reference.py: the three kernels bit for bit against their documented float32 order; the back-projection against
the float64 reference chain under the project's 3x float64-gate rule; PointStateBuilder against the restated
_get_observation / process_pointcloud with identically seeded np.random; the FPS route against the CPU oracle; and
Agent.select_action on the builder's device-resident state.  Shapes are the smallest at which each mechanism can go wrong."""
import numpy as np
import pytest
import torch

from tests import point_state_reference as R

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _backproject(depth, mask, A, div=None):
    """a direct call over pre-filled outputs -> (xyz, count, pix) as numpy arrays"""
    from ga_ddpg_amd.core.point_state import backproject_depth
    B, H, W = depth.shape
    d = torch.from_numpy(depth.view(np.int16) if depth.dtype == np.uint16 else depth).cuda()
    m = None if mask is None else torch.from_numpy(mask).cuda()
    xyz = torch.full((B, H * W, 3), SENTINEL, dtype=torch.float32, device="cuda")
    pix = torch.full((B, H * W), -7, dtype=torch.int32, device="cuda")
    xyz, count, pix = backproject_depth(d, m, torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).cuda(), div, xyz=xyz, pix=pix)
    torch.cuda.synchronize()
    return xyz.cpu().numpy(), count.cpu().numpy(), pix.cpu().numpy()


def _check_backproject(depth, mask, A, div=None):
    xyz, count, pix = _backproject(depth, mask, A, div)
    for b in range(depth.shape[0]):
        want, wpix = R.documented_backproject(depth[b], None if mask is None else mask[b], A[b], div)
        n = wpix.size
        assert count[b] == n, (b, count[b], n)
        np.testing.assert_array_equal(pix[b, :n], wpix)
        np.testing.assert_array_equal(_bits(xyz[b, :n]), _bits(want))
        assert (xyz[b, n:] == SENTINEL).all() and (pix[b, n:] == -7).all()          # rows past the count are untouched
    return count


def _affines(rng, B, H, W):
    from ga_ddpg_amd.core.point_state import compose_camera_affine
    return np.stack([compose_camera_affine(R.intrinsics(H, W), R.random_pose(rng, 0.05), True, R.random_pose(rng, 0.4)) for _ in range(B)])


SHAPES = [(7, 9), (31, 33), (32, 32), (45, 23), (67, 96), (112, 112)]


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_backproject_bit_for_bit(H, W, u16):
    """7x9: under one wavefront; 31x33 / 32x32: one tile, short and exact; 45x23: a tile plus an 11-pixel tail, rows ending
    mid-vector, images 2 and 3 starting off 16-byte alignment; 67x96: several tiles; 112x112: the simulator's own.  B = 3 with
    different counts per image."""
    rng = np.random.default_rng(H * 1000 + W)
    frames = [R.random_frame(rng, H, W, zero_frac=z, mask_frac=m) for z, m in [(0.2, 0.3), (0.7, 0.1), (0.02, 0.6)]]
    depth = np.stack([f[0] for f in frames])
    mask = np.stack([f[1] for f in frames])
    div = None
    if u16:
        depth = np.where(depth == 0, 0, rng.integers(1, 65536, size=depth.shape)).astype(np.uint16)
        div = 5000.0
    count = _check_backproject(depth, mask, _affines(rng, 3, H, W), div)
    assert len(set(count.tolist())) == 3


@pytest.mark.parametrize("H,W", [(45, 23), (67, 96)])
def test_backproject_keep_patterns(H, W):
    """all kept; none kept; only the last pixel; first tile empty; alternate pixels -- once decided by the depth with a null
    mask, once by the mask"""
    rng = np.random.default_rng(H)
    HW = H * W
    p = np.arange(HW)
    keeps = np.stack([np.ones(HW, bool), np.zeros(HW, bool), p == HW - 1, p >= 1024, p % 2 == 1]).reshape(5, H, W)
    full = rng.uniform(0.3, 1.2, size=(5, H, W)).astype(np.float32)
    A = _affines(rng, 5, H, W)
    count = _check_backproject(np.where(keeps, full, np.float32(0)), None, A)
    np.testing.assert_array_equal(count, [HW, 0, 1, HW - 1024, HW // 2])
    count = _check_backproject(full, np.where(keeps, 0, 200).astype(np.uint8), A)
    np.testing.assert_array_equal(count, [HW, 0, 1, HW - 1024, HW // 2])


def test_backproject_keeps_a_nan_depth():
    """depth != 0 holds for a NaN (reference core/utils.py:460): the pixel is kept and its point is NaN; an infinity likewise"""
    rng = np.random.default_rng(3)
    depth, mask = R.random_frame(rng, 45, 23)
    depth, mask = depth[None].copy(), mask[None].copy()
    depth[0, 3, 7], depth[0, 44, 22], mask[0, 3, 7], mask[0, 44, 22] = np.nan, np.inf, 0, 0
    A = _affines(rng, 1, 45, 23)
    xyz, count, pix = _backproject(depth, mask, A)
    _check_backproject(depth, mask, A)
    j = int(np.flatnonzero(pix[0, :count[0]] == 3 * 23 + 7)[0])
    assert np.isnan(xyz[0, j]).all() and pix[0, count[0] - 1] == 45 * 23 - 1


@pytest.mark.parametrize("H,W", [(45, 23), (112, 112)])
def test_backproject_against_the_float64_chain(H, W):
    """Max-abs error over the kept points of K^-1, y flip, cam_offset, y flip, pose against the float64 reference chain, within
    3x the error of the same chain evaluated step by step in float32 numpy (the project's float64-gate rule).  The documented
    order stayed within 1.55x of that yardstick over 20 random 45x23 cases on the CPU (tests/test_point_state_host.py); the
    device evaluates the same order bit for bit, so the ratios printed here are those of the restatement."""
    from ga_ddpg_amd.core.point_state import compose_camera_affine
    rng = np.random.default_rng(H + 77)
    for case in range(3):
        K, cam, pose = R.intrinsics(H, W), R.random_pose(rng, 0.05), R.random_pose(rng, 0.4)
        depth, mask = R.random_frame(rng, H, W)
        ref64, pix = R.backproject_chain(depth, K, mask, cam, True, pose, np.float64)
        ref32, _ = R.backproject_chain(depth, K, mask, cam, True, pose, np.float32)
        xyz, count, gpix = _backproject(depth[None], mask[None], compose_camera_affine(K, cam, True, pose)[None])
        n = pix.size
        assert count[0] == n
        np.testing.assert_array_equal(gpix[0, :n], pix)
        yard = np.abs(ref32.astype(np.float64) - ref64).max()
        err = np.abs(xyz[0, :n].T.astype(np.float64) - ref64).max()
        print("%dx%d case %d: device error %.3e, float32 chain error %.3e, ratio %.3f" % (H, W, case, err, yard, err / yard))
        assert err <= 3.0 * yard


# ---------------------------------------------------------------------------------------------------------------------
# gad_cloud_gather_affine / gad_point_state_pack
# ---------------------------------------------------------------------------------------------------------------------
def _strided_cloud(rng, B, N, pad=5):
    """(B, N, 3) view into a larger buffer: clouds `pad` points apart from each other's ends"""
    big = rng.normal(size=(B, N + 2 * pad, 3)).astype(np.float32)
    t = torch.from_numpy(big).cuda()
    return big[:, pad:pad + N], t[:, pad:pad + N]


@pytest.mark.parametrize("n", [0, 1, 63, 65, 1024])
def test_gather_affine_and_pack_bit_for_bit(n):
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.core.point_state import cloud_gather_affine, point_state_pack
    rng = np.random.default_rng(n + 1)
    B, N = 2, 700
    src, src_t = _strided_cloud(rng, B, N)
    assert not src_t.is_contiguous()
    A = np.stack([R.random_pose(rng)[:3, :4].reshape(12) for _ in range(B)]).astype(np.float32)
    A_t = torch.from_numpy(A).cuda()
    sel = rng.integers(0, N, size=(B, n)).astype(np.int32)
    if n > 4:
        sel[:, 1] = sel[:, 0]                                   # repeats
        sel[:, -1] = sel[:, 0]
    sel_t = torch.from_numpy(sel).cuda()
    lead = rng.normal(size=(6, 3)).astype(np.float32)
    lead_t = torch.from_numpy(lead).cuda()
    same, same_t = _strided_cloud(rng, B, n)                    # the cloud of the identity selection has n points itself

    for s_np, s_t, a_np, a_t, c_np, c_t in [(sel, sel_t, A, A_t, src, src_t), (sel, sel_t, None, None, src, src_t),
                                            (None, None, A, A_t, same, same_t), (None, None, None, None, same, same_t)]:
        # into a strided view of a sentinel buffer: nothing around the clouds is written
        out_big = torch.full((B, n + 6, 3), SENTINEL, dtype=torch.float32, device="cuda")
        got = cloud_gather_affine(c_t, s_t, a_t, out=out_big[:, 2:2 + n])
        want = R.documented_gather(c_np, s_np, a_np)
        ob = out_big.cpu().numpy()
        np.testing.assert_array_equal(_bits(ob[:, 2:2 + n]), _bits(want))
        assert (ob[:, :2] == SENTINEL).all() and (ob[:, 2 + n:] == SENTINEL).all()
        np.testing.assert_array_equal(_bits(cloud_gather_affine(c_t, s_t, a_t).cpu().numpy()), _bits(want))
        assert got.shape == (B, n, 3)
        for l_np, l_t, flag in [(lead, lead_t, 1.0), (None, None, 1.0), (lead, lead_t, -1.0)]:
            state = point_state_pack(c_t, s_t, a_t, l_t, flag)
            n_lead = 0 if l_np is None else 6
            assert state.shape == (B, 4, n_lead + n)
            np.testing.assert_array_equal(_bits(state.cpu().numpy()), _bits(R.documented_pack(c_np, s_np, a_np, l_np, flag)))
            if n > 0:                                           # the inverse of gad_prep_points
                xyz = torch.empty(B, n, 3, device="cuda")
                feat = torch.empty(B * n, 4, device="cuda")
                hip.call("gad_prep_points", state, B, 4, n_lead + n, n_lead, xyz, feat)
                np.testing.assert_array_equal(_bits(xyz.cpu().numpy()), _bits(want))
                np.testing.assert_array_equal(_bits(feat.cpu().numpy()[:, :3]), _bits(want.reshape(B * n, 3)))
                assert (feat.cpu().numpy()[:, 3] == 0).all()


def test_operator_checks_raise_runtime_error():
    from ga_ddpg_amd.core.point_state import backproject_depth, cloud_gather_affine, point_state_pack
    cloud = torch.zeros(1, 8, 3, device="cuda")
    with pytest.raises(RuntimeError, match="CPU tensor"):
        cloud_gather_affine(torch.zeros(1, 8, 3))
    with pytest.raises(RuntimeError, match="float tensor"):
        cloud_gather_affine(cloud.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        cloud_gather_affine(torch.zeros(1, 3, 8, device="cuda").transpose(1, 2))
    with pytest.raises(RuntimeError, match="int32"):
        point_state_pack(cloud, torch.zeros(1, 4, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="depth_div"):
        backproject_depth(torch.zeros(1, 4, 4, dtype=torch.int16, device="cuda"), None, torch.zeros(1, 12, device="cuda"))
    with pytest.raises(RuntimeError, match="contiguous"):
        backproject_depth(torch.zeros(1, 4, 8, device="cuda")[:, :, ::2], None, torch.zeros(1, 12, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# PointStateBuilder against the restated scene
# ---------------------------------------------------------------------------------------------------------------------
H, W = 45, 23
_SEQ = {}


def _sequence():
    """4 frames with moving poses (computed once, shared, never modified)"""
    if not _SEQ:
        rng = np.random.default_rng(45023)
        _SEQ["K"] = R.intrinsics(H, W)
        _SEQ["cam"] = R.random_pose(rng, 0.05)
        base = R.random_pose(rng, 0.4)
        poses, frames = [], []
        for i in range(4):
            step = R.random_pose(rng, 0.02)
            step[:3, :3] = 0.9 * np.eye(3) + 0.1 * step[:3, :3]
            u, _, vt = np.linalg.svd(step[:3, :3])
            step[:3, :3] = u.dot(vt)                            # a small rotation
            base = base.dot(step)
            poses.append(base.copy())
            frames.append(R.random_frame(rng, H, W))
        _SEQ["poses"], _SEQ["frames"] = poses, frames
    return _SEQ


def _run_reference(dtype, seed, frames, acc, **kw):
    s = _sequence()
    scene = R.ReferenceScene(dtype=dtype, **kw)
    np.random.seed(seed)
    return [scene.get_observation(d, m, s["K"], s["cam"], s["poses"][i], i, acc) for i, (d, m) in enumerate(frames)]


CASES = {
    # ~580 kept pixels per frame: the accumulated cloud passes 512 with the second frame (random cut)
    "accumulate_cut": dict(uniform_num_pts=512, accumulate=True, acc=True, masked_first=False),
    # 4096 is more than four frames accumulate: the padding draw
    "accumulate_pad": dict(uniform_num_pts=4096, accumulate=True, acc=True, masked_first=False),
    "no_accumulate": dict(uniform_num_pts=512, accumulate=False, acc=True, masked_first=False),
    "acc_pt_off": dict(uniform_num_pts=700, accumulate=True, acc=False, masked_first=False),
    # an all-masked first frame: the lead columns only
    "masked_first": dict(uniform_num_pts=512, accumulate=True, acc=True, masked_first=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_builder_against_the_restated_scene(case):
    """Provenance (frame, pixel) of every state column identical to the reference's under the same np.random seed; the flag
    row exact; coordinates within 3x the error the float32 step-by-step scene makes against the float64 one (worst frame
    ratios are printed).  A capacity of 64 points makes the buffer double several times."""
    from ga_ddpg_amd.core.point_state import PointStateBuilder
    c = dict(CASES[case])
    acc, masked_first = c.pop("acc"), c.pop("masked_first")
    s = _sequence()
    frames = list(s["frames"])
    if masked_first:
        frames[0] = (frames[0][0], np.full((H, W), 9, dtype=np.uint8))
    ref64 = _run_reference(np.float64, 77, frames, acc, **c)
    ref32 = _run_reference(np.float32, 77, frames, acc, **c)
    b = PointStateBuilder(capacity=64, track_provenance=True, **c)
    np.random.seed(77)
    for i, (d, m) in enumerate(frames):
        state = b.observe(d, m, s["K"], s["poses"][i], i, cam_offset=s["cam"], acc=acc)
        want, prov = ref64[i]
        assert state.is_cuda and state.dtype == torch.float32 and tuple(state.shape) == want.shape, (i, state.shape, want.shape)
        got = state.cpu().numpy()
        np.testing.assert_array_equal(b.last_provenance.cpu().numpy(), prov.T)
        np.testing.assert_array_equal(got[3], want[3])
        yard = np.abs(ref32[i][0].astype(np.float64) - want).max()
        err = np.abs(got.astype(np.float64) - want).max()
        print("%s frame %d: %d columns, device error %.3e, float32 scene error %.3e, ratio %.3f"
              % (case, i, got.shape[1], err, yard, err / yard if yard else 0.0))
        assert err <= 3.0 * yard
        if masked_first and i == 0:
            assert got.shape == (4, 6)
    if c["accumulate"] and acc:
        assert b._buf.shape[0] > 64 and b.num_acc_points == sum(
            int(0.95 ** i * R.keep_mask(*frames[i])[1].sum()) for i in range(4))


def test_builder_with_an_own_generator_and_uint16_depth():
    """rng= replaces the global generator (the global stream is not touched); a uint16 frame is divided by depth_div"""
    from ga_ddpg_amd.core.point_state import PointStateBuilder, compose_camera_affine
    s = _sequence()
    depth = (np.random.default_rng(1).integers(0, 4, size=(H, W)) * 1700).astype(np.uint16)
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    b = PointStateBuilder(uniform_num_pts=256, accumulate=False, rng=np.random.RandomState(8), track_provenance=True)
    state = b.observe(depth, None, s["K"], s["poses"][0], 0, cam_offset=s["cam"]).cpu().numpy()
    assert np.array_equal(before, np.random.get_state()[1])
    pts, pix = R.documented_backproject(depth, None, compose_camera_affine(s["K"], s["cam"], True), 5000.0)
    keep = np.random.RandomState(8).choice(pix.size, size=256, replace=False)
    np.testing.assert_array_equal(_bits(state[:3, 6:]), _bits(pts[keep].T))
    np.testing.assert_array_equal(b.last_provenance.cpu().numpy()[:, 1], pix[keep])


def test_fps_route_and_regularize_acc():
    """use_farthest_point: the picked indices equal the CPU oracle's on the builder's own read-back end-effector-frame cloud, the
    packed columns equal that cloud gathered by them; regularize_acc trims the accumulated cloud the same way"""
    from oracle import cref
    from ga_ddpg_amd.core.point_state import PointStateBuilder, inverse_pose_affine
    s = _sequence()
    b = PointStateBuilder(uniform_num_pts=256, capacity=64)
    np.random.seed(11)
    for i, (d, m) in enumerate(s["frames"][:3]):
        state = b.observe(d, m, s["K"], s["poses"][i], i, cam_offset=s["cam"], use_farthest_point=True).cpu().numpy()
        acc = b.curr_acc_points.cpu().numpy()
        ef = b.last_ef_cloud.cpu().numpy()
        np.testing.assert_array_equal(_bits(ef), _bits(R.documented_affine(inverse_pose_affine(s["poses"][i]), acc)))
        want = cref.fps(ef[None], 256)[0]
        np.testing.assert_array_equal(b.last_fps_idx.cpu().numpy(), want)
        assert state.shape == (4, 6 + 256)
        np.testing.assert_array_equal(_bits(state[:3, 6:]), _bits(ef[want].T))
        np.testing.assert_array_equal(state[3], [1.0] * 6 + [0.0] * 256)
        np.testing.assert_array_equal(_bits(state[:3, :6]), _bits(R.HAND_FINGER_POINT))
    acc = b.curr_acc_points.cpu().numpy()
    assert acc.shape[0] > 300
    b.regularize_acc(300, use_farthest_point=True)
    np.testing.assert_array_equal(_bits(b.curr_acc_points.cpu().numpy()), _bits(acc[cref.fps(acc[None], 300)[0]]))
    np.random.seed(12)
    b.regularize_acc(200)
    b.regularize_acc(260)
    np.random.seed(12)
    cut = acc[cref.fps(acc[None], 300)[0]][np.random.choice(300, size=200, replace=False)]
    np.testing.assert_array_equal(_bits(b.curr_acc_points.cpu().numpy()),
                                  _bits(np.concatenate((cut, cut[np.random.choice(200, size=60)]))))


def test_reference_signature_helpers():
    """core.utils.se3_transform_pc / backproject_camera_target[_realworld]: numpy in, float32 numpy out, the documented order"""
    from ga_ddpg_amd.core import utils
    from ga_ddpg_amd.core.point_state import compose_camera_affine, pose_affine
    rng = np.random.default_rng(21)
    K, pose = R.intrinsics(H, W), R.random_pose(rng)
    depth, mask = R.random_frame(rng, H, W)
    for fn, flip in [(utils.backproject_camera_target, True), (utils.backproject_camera_target_realworld, False)]:
        got = fn(depth, K, mask.astype(np.float64))
        want, _ = R.documented_backproject(depth, mask, compose_camera_affine(K, None, flip))
        assert got.dtype == np.float32 and got.shape == (3, want.shape[0])
        np.testing.assert_array_equal(_bits(got), _bits(want.T))
        ref64, _ = R.backproject_chain(depth, K, mask, None, flip)
        assert np.abs(got - ref64).max() < 1e-6
    cloud = rng.normal(size=(4, 50))
    got = utils.se3_transform_pc(pose, cloud)
    assert got.dtype == np.float32 and got.shape == (4, 50)
    np.testing.assert_array_equal(_bits(got[:3]), _bits(R.documented_affine(pose_affine(pose), cloud[:3].T.astype(np.float32)).T))
    np.testing.assert_array_equal(got[3], cloud[3].astype(np.float32))


def test_select_action_takes_the_device_state():
    """the builder's CUDA state goes to feature_forward as it is: same four values as with its .cpu().numpy()"""
    from ga_ddpg_amd.api import make_agent
    from ga_ddpg_amd.core.point_state import PointStateBuilder
    from oracle.detfill import fill_module_
    agent, _ = make_agent("ddpg_td3_aux.yaml")
    for name in ("policy", "state_feature_extractor"):
        fill_module_(getattr(agent, name), name, 1234)
    s = _sequence()
    b = PointStateBuilder()
    np.random.seed(2)
    for i, (d, m) in enumerate(s["frames"][:2]):
        state = b.observe(d, m, s["K"], s["poses"][i], i, cam_offset=s["cam"])
    assert state.is_cuda and tuple(state.shape) == (4, 6 + 1024)
    eps = np.random.default_rng(9).normal(size=6).astype(np.float32)
    dev = agent.select_action([[state, None]], remain_timestep=11, eps=eps)
    host = agent.select_action([[state.cpu().numpy(), None]], remain_timestep=11, eps=eps)
    assert isinstance(dev[1], float) and dev[0].shape == (6,) and dev[2].shape == (6,) and dev[3].shape == (7,)
    for a, h in zip(dev, host):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(h))
