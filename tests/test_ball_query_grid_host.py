"""Host side of gad_ball_query_grid (include/gaddpg.h section A): exports, the plan table, the argument checks -- they run before
any launch -- the workspace size and the routing predicate of the facade.  None of this needs a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from ga_ddpg_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return hip.lib()


def test_symbols_are_exported_declared_and_replayable():
    from ga_ddpg_amd import hip
    L = _lib()
    src = open(os.path.join(ROOT, "include", "gaddpg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gad_ball_query_grid_workspace_bytes", "gad_ball_query_grid"):
        assert name in hip.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, src), name
    assert "gad_ball_query_grid" in [L.gad_plan_entry_name(i).decode() for i in range(L.gad_plan_entry_count())]
    assert L.gad_abi_version() == 12
    # the library option exists next to bq_cells (the value is restored: 1 is the default)
    assert L.gad_set_option(b"bq_grid", 0) == 0 and L.gad_set_option(b"bq_grid", 1) == 0 and L.gad_set_option(b"bq_cells", 1) == 0


def test_bad_arguments_are_status_codes_with_a_message():
    L = _lib()
    f, err = L.gad_ball_query_grid, L.gad_last_error
    null, p = C.c_void_p(None), C.c_void_p(0x1000)
    assert f(null, p, 1, 5000, 8, 0.1, 4, p, p, p, null) < 0 and b"null pointer" in err()
    assert f(p, null, 1, 5000, 8, 0.1, 4, p, p, p, null) < 0 and b"null pointer" in err()
    assert f(p, p, 1, 5000, 8, 0.1, 4, null, p, p, null) < 0 and b"null pointer" in err()
    assert f(p, p, 1, 5000, 8, 0.1, 4, p, null, null, null) < 0 and b"workspace" in err()
    assert f(p, p, 1, 5000, 8, 0.1, 4, p, null, C.c_void_p(0x1004), null) < 0 and b"aligned" in err()
    assert f(p, p, -1, 5000, 8, 0.1, 4, p, null, p, null) < 0 and b"B=-1" in err()
    assert f(p, p, 1, 0, 8, 0.1, 4, p, null, p, null) < 0 and b"N=0" in err()
    assert f(p, p, 1, -3, 8, 0.1, 4, p, null, p, null) < 0 and b"N=-3" in err()
    assert f(p, p, 1, 5000, -2, 0.1, 4, p, null, p, null) < 0 and b"M=-2" in err()
    assert f(p, p, 1, 5000, 8, 0.1, 0, p, null, p, null) < 0 and b"nsample=0" in err()
    assert f(p, p, 1, 5000, 8, 0.1, -1, p, null, p, null) < 0 and b"nsample=-1" in err()
    # products beyond 32-bit indexing: 3 * N, B * N, the grid of B * M centroids
    assert f(p, p, 1, 800000000, 8, 0.1, 4, p, null, p, null) < 0 and b"overflows" in err()
    assert f(p, p, 1024, 1 << 21, 8, 0.1, 4, p, null, p, null) < 0 and b"overflows" in err()
    assert f(p, p, 1 << 10, 5000, 1 << 16, 0.1, 4, p, null, p, null) < 0 and b"overflows" in err()
    # nothing to search: GAD_OK without a launch (so without a GPU), the workspace may be NULL
    assert f(p, p, 0, 5000, 8, 0.1, 4, p, null, null, null) == 0
    assert f(p, p, 2, 5000, 0, 0.1, 4, p, null, null, null) == 0


def test_workspace_bytes():
    L = _lib()
    ws = L.gad_ball_query_grid_workspace_bytes
    sizes = [1, 64, 4097, 5000, 20000, 70000, 262144, 1 << 20, 1 << 22]
    for B in (1, 3):
        prev = 0
        for N in sizes:
            per_m = [ws(B, N, M, 16) for M in (0, 1, 33, 4096, 16384)]
            assert per_m[0] > 0 and per_m == sorted(per_m)           # positive, non-decreasing in M ...
            assert per_m[0] >= prev                                     # ... and in N
            assert per_m[0] >= B * N * 24                               # cell, rank and the sorted (x, y, z, index) of every point
            prev = per_m[-1]
    assert ws(3, 70000, 64, 200) >= ws(1, 70000, 64, 200)
    # the size needs more than 32 bits before the shape does
    assert ws(256, 1 << 22, 64, 16) > 1 << 32
    assert ws(1, 0, 8, 4) < 0 and b"N=0" in L.gad_last_error()
    assert ws(-1, 64, 8, 4) < 0 and b"B=-1" in L.gad_last_error()
    assert ws(1, 64, 8, 0) < 0 and b"nsample=0" in L.gad_last_error()
    assert ws(1, 800000000, 8, 4) < 0 and b"overflows" in L.gad_last_error()
    assert ws(1 << 10, 5000, 1 << 16, 4) < 0 and b"overflows" in L.gad_last_error()


def test_routing_predicate_at_the_boundaries(monkeypatch):
    """clouds of up to 4096 points keep gad_ball_query's LDS kernels whatever the option says; library option bq_grid = 2 makes 4097
    the first cloud sent to the grid, the default 1 the measured 262 144 (profiles/ball_query_grid.txt), 0 none.  The fused
    set-abstraction path routes by the same function."""
    from ga_ddpg_amd import hip, sa_function
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    _lib()
    assert sa_function.pu is pu
    assert (pu.BQ_LDS_MAX_N, pu.BQ_GRID_MIN_N) == (4096, 262144)
    monkeypatch.setitem(hip._options, "bq_grid", 2)
    for N in (1, 512, 1024, 1025, 4095, 4096):
        assert not pu.ball_query_uses_grid(N), N
    for N in (4097, 5000, 16384, 70000, 262144, 1 << 22):
        assert pu.ball_query_uses_grid(N), N
    monkeypatch.setitem(hip._options, "bq_grid", 1)
    for N in (1, 4096, 4097, 5000, 70000, 262143):
        assert not pu.ball_query_uses_grid(N), N
    for N in (262144, 262145, 1 << 20, 1 << 22):
        assert pu.ball_query_uses_grid(N), N
    monkeypatch.setitem(hip._options, "bq_grid", 0)
    for N in (4096, 4097, 262144, 1 << 22):
        assert not pu.ball_query_uses_grid(N), N


def test_facade_entry_points_by_shape(monkeypatch):
    """the entry point pointnet2_utils.ball_query names for a shape (the call itself is replaced: no launch): today's for N <= 4096
    under every option, and below the measured threshold by default"""
    import torch
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    _lib()
    calls = []
    monkeypatch.setattr(hip, "call", lambda name, *a: calls.append((name, len(a))))
    monkeypatch.setattr(hip, "require_cuda", lambda *t: None)
    monkeypatch.setattr(hip, "workspace", lambda name, device, *shape: ("workspace", name) + shape)
    scan, grid = "gad_ball_query", "gad_ball_query_grid"
    for mode, cases in [(2, [(64, scan), (1024, scan), (4096, scan), (4097, grid), (5000, grid)]),
                        (1, [(64, scan), (4096, scan), (4097, scan), (5000, scan), (262143, scan), (262144, grid)]),
                        (0, [(4096, scan), (5000, scan), (262144, scan)])]:
        monkeypatch.setitem(hip._options, "bq_grid", mode)
        for N, want in cases:
            del calls[:]
            idx = pu.ball_query(0.1, 8, torch.zeros(1, N, 3), torch.zeros(1, 4, 3))
            assert tuple(idx.shape) == (1, 4, 8) and idx.dtype == torch.int32
            assert calls == [(want, 10 if want == grid else 9)], (mode, N, calls)
