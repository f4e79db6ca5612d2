"""Host side of the observation operators (include/gaddpg.h section A.2) and of core.point_state: the argument checks run
before any launch and the affine composition is host float64, so none of this needs a GPU."""
import ctypes as C

import numpy as np

from tests import point_state_reference as R

NEW = ("gad_backproject_depth_workspace_bytes", "gad_backproject_depth", "gad_cloud_gather_affine", "gad_point_state_pack")


def _lib():
    import os
    from ga_ddpg_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return hip.lib()


def test_symbols_are_exported_and_replayable():
    from ga_ddpg_amd import hip
    L = _lib()
    for name in NEW:
        assert hasattr(L, name) and name in hip.EXPORTS, name
    plan = {L.gad_plan_entry_name(i).decode() for i in range(L.gad_plan_entry_count())}
    assert set(NEW[1:]) <= plan                       # every entry point that ends in `void* stream`
    assert NEW[0] not in plan
    assert L.gad_abi_version() == 12                  # additive: no bump


def test_workspace_bytes_and_its_refusals():
    L = _lib()
    ws = L.gad_backproject_depth_workspace_bytes
    assert ws(1, 112, 112) >= 4 * 13 and ws(3, 45, 23) >= 3 * 2 * 4 and ws(1, 4096, 4096) >= 4 * 16384
    assert ws(2, 480, 640) >= 2 * 300 * 4 and ws(0, 4, 4) == 0
    for H, W in [(0, 8), (8, 0), (-1, 8), (8, -3), (4097, 8), (8, 4097)]:
        assert ws(1, H, W) < 0 and b"outside 1..4096" in L.gad_last_error(), (H, W)
    assert ws(-1, 8, 8) < 0 and b"B=-1" in L.gad_last_error()
    assert ws(128, 4096, 4096) < 0 and b"beyond 2^31" in L.gad_last_error()          # B * H * W = 2^31
    assert ws(127, 4096, 4096) > 0
    assert ws((1 << 23), 1, 1) < 0 and b"overflows" in L.gad_last_error()             # a grid of 2^23 workgroups


def test_bad_arguments_are_status_codes_with_a_message():
    L = _lib()
    null, p = C.c_void_p(None), C.c_void_p(0x1000)
    bp = L.gad_backproject_depth
    assert bp(null, 0, 1.0, null, p, 1, 8, 8, p, p, null, p, null) < 0 and b"null pointer" in L.gad_last_error()
    assert bp(p, 0, 1.0, null, null, 1, 8, 8, p, p, null, p, null) < 0 and b"null pointer" in L.gad_last_error()
    assert bp(p, 0, 1.0, null, p, 1, 8, 8, p, p, null, null, null) < 0 and b"workspace" in L.gad_last_error()
    assert bp(p, 0, 1.0, null, p, 1, 8, 8, p, p, null, C.c_void_p(0x1004), null) < 0 and b"aligned" in L.gad_last_error()
    assert bp(C.c_void_p(0x1002), 0, 1.0, null, p, 1, 8, 8, p, p, null, p, null) < 0 and b"element size" in L.gad_last_error()
    assert bp(p, 1, 0.0, null, p, 1, 8, 8, p, p, null, p, null) < 0 and b"divisor" in L.gad_last_error()
    assert bp(p, 1, float("nan"), null, p, 1, 8, 8, p, p, null, p, null) < 0 and b"divisor" in L.gad_last_error()
    assert bp(p, 2, 1.0, null, p, 1, 8, 8, p, p, null, p, null) < 0 and b"depth_u16=2" in L.gad_last_error()
    assert bp(p, 0, 1.0, null, p, 1, 8, 5000, p, p, null, p, null) < 0 and b"outside 1..4096" in L.gad_last_error()
    assert bp(null, 0, 1.0, null, null, 0, 8, 8, null, null, null, null, null) == 0          # B == 0: GAD_OK without a launch

    ga = L.gad_cloud_gather_affine
    assert ga(null, 0, null, null, 1, 4, p, 0, null) < 0 and b"null pointer (src)" in L.gad_last_error()
    assert ga(p, 0, null, null, 1, 4, null, 0, null) < 0 and b"null pointer (dst)" in L.gad_last_error()
    assert ga(p, 0, null, null, 1, -4, p, 0, null) < 0 and b"n=-4" in L.gad_last_error()
    assert ga(p, -1, null, null, 1, 4, p, 0, null) < 0 and b"src_stride=-1" in L.gad_last_error()
    assert ga(p, 0, null, null, 1, 4, p, -2, null) < 0 and b"dst_stride=-2" in L.gad_last_error()
    assert ga(p, 0, null, null, 1 << 16, 1 << 15, p, 0, null) < 0 and b"beyond 2^31" in L.gad_last_error()
    assert ga(null, 0, null, null, 3, 0, null, 0, null) == 0 and ga(null, 0, null, null, 0, 7, null, 0, null) == 0

    pk = L.gad_point_state_pack
    assert pk(null, 0, null, null, p, 6, 1.0, 1, 4, p, null) < 0 and b"null pointer (src)" in L.gad_last_error()
    assert pk(p, 0, null, null, null, 6, 1.0, 1, 4, p, null) < 0 and b"null pointer (lead)" in L.gad_last_error()
    assert pk(p, 0, null, null, p, 6, 1.0, 1, 4, null, null) < 0 and b"null pointer (state)" in L.gad_last_error()
    assert pk(p, 0, null, null, p, -1, 1.0, 1, 4, p, null) < 0 and b"n_lead=-1" in L.gad_last_error()
    assert pk(p, 0, null, null, p, 1 << 15, 1.0, 1 << 16, 4, p, null) < 0 and b"beyond 2^31" in L.gad_last_error()
    assert pk(null, 0, null, null, null, 0, 1.0, 4, 0, null, null) == 0                       # nothing to write


def _random_setup(rng):
    K = R.intrinsics(45, 23) + np.array([[rng.uniform(-3, 3), 0, rng.uniform(-2, 2)], [0, rng.uniform(-3, 3), rng.uniform(-2, 2)],
                                         [0, 0, 0]])
    return K, R.random_pose(rng, 0.05), R.random_pose(rng, 0.4)


def test_compose_camera_affine_is_the_step_by_step_chain():
    from ga_ddpg_amd.core.point_state import compose_camera_affine
    rng = np.random.default_rng(5)
    for _ in range(10):
        K, cam, pose = _random_setup(rng)
        for cam_offset, flip_y, p in [(None, True, None), (None, False, None), (cam, True, None), (cam, False, None),
                                      (cam, True, pose), (None, True, pose), (cam, False, pose)]:
            want = R.compose_chain64(K, cam_offset, flip_y, p)
            got = compose_camera_affine(K, cam_offset, flip_y, p, dtype=np.float64)
            assert got.shape == (12,) and np.abs(got - want).max() <= 1e-12
            got32 = compose_camera_affine(K, cam_offset, flip_y, p)
            assert got32.dtype == np.float32 and np.array_equal(got32, got.astype(np.float32))
    # and the composed affine IS the chain: d * (M p~) + t in float64 against the float64 chain on an image
    K, cam, pose = _random_setup(rng)
    depth, mask = R.random_frame(rng, 45, 23)
    want, pix = R.backproject_chain(depth, K, mask, cam, True, pose)
    A = compose_camera_affine(K, cam, True, pose, dtype=np.float64).reshape(3, 4)
    pt = np.stack((pix % 23, pix // 23, np.ones_like(pix))).astype(np.float64)
    got = depth.flatten()[pix].astype(np.float64) * A[:, :3].dot(pt) + A[:, [3]]
    assert np.abs(got - want).max() <= 1e-12


def test_documented_order_against_the_float64_chain():
    """The float32 arithmetic the kernel documents -- r = (M0 x + M1 y) + M2, P = d r + t with the composed, once-rounded
    affine -- against the float64 reference chain (pose included), measured in units of the error the SAME chain makes when
    evaluated step by step in float32 numpy.  The project's float64-gate rule allows 3x.  Measured here over 20 random 45 x 23
    cases: worst ratio 1.55, median 0.80 (the composed form is usually the more accurate of the two)."""
    from ga_ddpg_amd.core.point_state import compose_camera_affine
    rng = np.random.default_rng(20261019)
    ratios = []
    for _ in range(20):
        K, cam, pose = _random_setup(rng)
        depth, mask = R.random_frame(rng, 45, 23)
        ref64, pix = R.backproject_chain(depth, K, mask, cam, True, pose, np.float64)
        ref32, _ = R.backproject_chain(depth, K, mask, cam, True, pose, np.float32)
        got, gpix = R.documented_backproject(depth, mask, compose_camera_affine(K, cam, True, pose))
        assert np.array_equal(gpix, pix) and ref32.dtype == np.float32 and got.dtype == np.float32
        yard = np.abs(ref32.astype(np.float64) - ref64).max()
        err = np.abs(got.T.astype(np.float64) - ref64).max()
        assert yard > 0
        ratios.append(err / yard)
    print("documented order / float32 step-by-step chain, max-abs error ratio: worst %.3f median %.3f" % (max(ratios), np.median(ratios)))
    assert max(ratios) <= 3.0


def test_reference_scene_restatement_draws_like_the_builder_would():
    """the restated scene's draws (range form) and the builder's (integer form) come from the same stream: same indices"""
    np.random.seed(3)
    a = np.random.choice(range(50), size=7, replace=False), np.random.choice(range(50), size=9), np.random.choice(range(0), size=0, replace=False)
    np.random.seed(3)
    b = np.random.choice(50, size=7, replace=False), np.random.choice(50, size=9), np.random.choice(0, size=0, replace=False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
