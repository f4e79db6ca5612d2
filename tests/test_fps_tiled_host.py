"""Host side of gad_fps_tiled and core.utils.regularize_pc_point_count: the argument checks run before any launch and the
random branches never touch the device, so none of this needs a GPU."""
import ctypes as C

import numpy as np


def _lib():
    import os
    from ga_ddpg_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return hip.lib()


def test_bad_arguments_are_status_codes_with_a_message():
    L = _lib()
    null, p = C.c_void_p(None), C.c_void_p(0x1000)
    assert L.gad_fps_tiled(null, 1, 64, 8, 0, p, null, p, null) < 0 and b"null pointer" in L.gad_last_error()
    assert L.gad_fps_tiled(p, 1, 64, 8, 0, null, null, p, null) < 0 and b"null pointer" in L.gad_last_error()
    assert L.gad_fps_tiled(p, 1, 64, 8, 0, p, null, null, null) < 0 and b"workspace" in L.gad_last_error()
    assert L.gad_fps_tiled(p, 1, 64, 8, 0, p, null, C.c_void_p(0x1004), null) < 0 and b"aligned" in L.gad_last_error()
    assert L.gad_fps_tiled(p, 1, (1 << 22) + 1, 8, 0, p, null, p, null) < 0 and b"N=4194305" in L.gad_last_error()
    assert L.gad_fps_tiled(p, 1, 64, 8, 65, p, null, p, null) < 0 and b"groups=65" in L.gad_last_error()
    assert L.gad_fps_tiled(p, 1, 64, 8, -1, p, null, p, null) < 0 and b"groups=-1" in L.gad_last_error()
    assert L.gad_fps_tiled(p, -1, 64, 8, 0, p, null, p, null) < 0 and b"B=-1" in L.gad_last_error()
    assert L.gad_fps_tiled(p, 1, 0, 8, 0, p, null, p, null) < 0 and b"N=0" in L.gad_last_error()
    assert L.gad_fps_tiled(p, 1, 64, -2, 0, p, null, p, null) < 0 and b"M=-2" in L.gad_last_error()
    assert L.gad_fps_tiled(p, 4096, 1 << 22, 8, 1 << 22, p, null, p, null) < 0 and b"overflows" in L.gad_last_error()
    # nothing to sample: GAD_OK without a launch (so without a GPU), a workspace is not needed
    assert L.gad_fps_tiled(p, 0, 64, 8, 0, p, null, null, null) == 0
    assert L.gad_fps_tiled(p, 2, 64, 0, 0, p, null, null, null) == 0


def test_workspace_bytes():
    L = _lib()
    ws = L.gad_fps_tiled_workspace_bytes
    for B, N, M in [(1, 1, 1), (2, 1000, 64), (1, 20000, 128), (2, 12000, 5000), (3, 5, 12), (1, 1 << 22, 4096)]:
        base = ws(B, N, M, 0)
        assert base > 0 and base >= B * N * 4 + B * M * 8
        assert ws(B, N, 4 * M + 64, 0) > base                  # grows with M ...
        assert ws(B, min(4 * N + 64, 1 << 22), M, 0) > base or N == 1 << 22        # ... and with N
        assert ws(B, N, M, 1) >= B * N * 4 and ws(B, N, M, N) >= B * N * 4
    # the size needs more than 32 bits before the shape does
    assert ws(64, 1 << 22, 1 << 20, 0) >= 64 * (1 << 22) * 4 + 64 * (1 << 20) * 8
    assert ws(1, (1 << 22) + 1, 8, 0) < 0 and b"N=4194305" in L.gad_last_error()
    assert ws(1, 64, 8, 65) < 0 and b"groups=65" in L.gad_last_error()


def test_facade_routing_predicate_is_the_entry_points_own():
    """pointnet2_utils routes by restating gad_furthest_point_sampling's acceptance rule: probe the rule itself (its checks run
    before any launch; a shape it accepts is not called here, that would launch)"""
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    L = _lib()
    p, null = C.c_void_p(0x1000), C.c_void_p(None)
    for N, M in [(64, 65), (5, 12), (16385, 16), (16384, 16384), (20000, 128), (12000, 5000), (13000, 1897), (10225, 10225)]:
        assert not pu.fps_fits_one_workgroup(N, M)
        assert L.gad_furthest_point_sampling(p, 1, N, M, p, p, null) < 0, (N, M)
    for N, M in [(1024, 32), (4096, 512), (64, 64), (13000, 16), (8000, 3000), (13000, 1896), (10224, 10224)]:
        assert pu.fps_fits_one_workgroup(N, M)


def _cloud(n, c=4, seed=0):
    return np.random.default_rng(seed).random((n, c))


def test_regularize_pc_point_count_random_branches():
    from ga_ddpg_amd.core.utils import regularize_pc_point_count
    pc = _cloud(50)
    np.random.seed(11)
    got = regularize_pc_point_count(pc, 20)
    np.random.seed(11)
    np.testing.assert_array_equal(got, pc[np.random.choice(range(50), size=20, replace=False), :])
    assert got.shape == (20, 4) and got.dtype == pc.dtype

    np.random.seed(12)
    got = regularize_pc_point_count(pc, 128)
    np.random.seed(12)
    extra = np.random.choice(range(50), size=78)
    np.testing.assert_array_equal(got, np.concatenate((pc, pc[extra, :]), axis=0))
    assert got.shape == (128, 4)

    # padding ignores use_farthest_point (no device work), as the reference does
    np.random.seed(13)
    got = regularize_pc_point_count(pc, 60, use_farthest_point=True)
    np.random.seed(13)
    np.testing.assert_array_equal(got[50:], pc[np.random.choice(range(50), size=10), :])

    assert regularize_pc_point_count(pc, 50) is pc
    assert regularize_pc_point_count(pc, 50, use_farthest_point=True) is pc
