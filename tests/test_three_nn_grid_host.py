"""Host side of gad_three_nn_grid (include/gaddpg.h section A): exports, the plan table, the option, the argument checks -- they
run before any launch -- the workspace size and the routing predicate of the facade.  None of this needs a GPU."""
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


def test_symbols_are_exported_typed_declared_and_replayable():
    from ga_ddpg_amd import hip
    L = _lib()
    src = open(os.path.join(ROOT, "include", "gaddpg.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gad_three_nn_grid_workspace_bytes", "gad_three_nn_grid"):
        assert name in hip.EXPORTS and hasattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in hip._SIGNATURES and getattr(L, name).argtypes == hip._SIGNATURES[name]
    assert len(hip._SIGNATURES["gad_three_nn_grid_workspace_bytes"]) == 3
    assert len(hip._SIGNATURES["gad_three_nn_grid"]) == 10            # ..., stats, workspace, stream
    assert L.gad_three_nn_grid_workspace_bytes.restype is C.c_longlong and L.gad_three_nn_grid.restype is C.c_int
    assert "gad_three_nn_grid" in [L.gad_plan_entry_name(i).decode() for i in range(L.gad_plan_entry_count())]
    assert L.gad_abi_version() == 12                                   # additive: no bump


def test_option_tnn_grid_takes_0_1_2():
    from ga_ddpg_amd import hip
    L = _lib()
    assert hip.OPTION_DEFAULTS["tnn_grid"] == 1
    try:
        for v in (0, 2, 1):
            assert L.gad_set_option(b"tnn_grid", v) == 0
        assert L.gad_set_option(b"tnn_gird", 1) < 0                    # an unknown name is still refused
    finally:
        assert L.gad_set_option(b"tnn_grid", 1) == 0


def test_bad_arguments_are_status_codes_with_a_message():
    L = _lib()
    f, err = L.gad_three_nn_grid, L.gad_last_error
    null, p = C.c_void_p(None), C.c_void_p(0x1000)
    # (unknown, known, B, n, m, dist2, idx, stats, workspace, stream); every call below returns before a launch
    assert f(null, p, 1, 8, 5000, p, p, null, p, null) < 0 and b"null pointer" in err()
    assert f(p, null, 1, 8, 5000, p, p, null, p, null) < 0 and b"null pointer" in err()
    assert f(p, p, 1, 8, 5000, null, p, null, p, null) < 0 and b"null pointer" in err()
    assert f(p, p, 1, 8, 5000, p, null, null, p, null) < 0 and b"null pointer" in err()
    assert f(p, p, 1, 8, 5000, p, p, null, null, null) < 0 and b"workspace" in err()
    assert f(p, p, 1, 8, 5000, p, p, null, C.c_void_p(0x1004), null) < 0 and b"aligned" in err()
    assert f(p, p, -1, 8, 5000, p, p, null, p, null) < 0 and b"B=-1" in err()
    assert f(p, p, 1, -8, 5000, p, p, null, p, null) < 0 and b"n=-8" in err()
    assert f(p, p, 1, 8, -3, p, p, null, p, null) < 0 and b"m=-3" in err()
    assert f(p, p, 1, 8, 0, p, p, null, p, null) < 0 and b"no known point" in err()
    # products beyond 32-bit indexing: 3 * m, B * m, B * n; more clouds than a launch grid has rows
    assert f(p, p, 1, 8, 800000000, p, p, null, p, null) < 0 and b"overflows" in err()
    assert f(p, p, 1024, 8, 1 << 21, p, p, null, p, null) < 0 and b"overflows" in err()
    assert f(p, p, 1024, 1 << 21, 64, p, p, null, p, null) < 0 and b"overflows" in err()
    assert f(p, p, 65536, 8, 64, p, p, null, p, null) < 0 and b"65535" in err()
    # no query: GAD_OK without a launch (so without a GPU), the workspace may be NULL -- and m may be 0
    assert f(p, p, 0, 8, 5000, p, p, null, null, null) == 0
    assert f(p, p, 2, 0, 5000, p, p, null, null, null) == 0
    assert f(p, p, 2, 0, 0, p, p, p, null, null) == 0


def test_workspace_bytes():
    L = _lib()
    ws = L.gad_three_nn_grid_workspace_bytes
    sizes = [1, 2, 3, 64, 1025, 4097, 5000, 20000, 70000, 262144, 1 << 20, 1 << 22]
    for B in (1, 3):
        prev = 0
        for m in sizes:
            per_n = [ws(B, n, m) for n in (0, 1, 257, 3000, 1 << 20)]
            assert per_n[0] > 0 and len(set(per_n)) == 1              # positive; n enters through the checks alone
            assert per_n[0] >= prev                                     # monotone in m
            parts, slices, cells = min(64, -(-m // 4096)), min(64, -(-m // 2048)), max(64, min(65536, m // 4))
            # the arrays the header names: box partials, grid header, cell + rank, slice counts, cell starts, sorted points
            assert per_n[0] >= B * (parts * 24 + 64 + m * 8 + slices * cells * 4 + (cells + 1) * 4 + m * 16)
            assert per_n[0] >= B * m * 24
            # one grid, one layout: the ball query's workspace over the same cloud, whatever its centroids and nsample
            bq = L.gad_ball_query_grid_workspace_bytes
            assert all(bq(B, m, M, ns) == per_n[0] for M, ns in ((0, 1), (1, 16), (4096, 64), (16384, 200)))
            prev = per_n[0]
    assert ws(3, 64, 70000) >= ws(1, 64, 70000)
    assert ws(256, 64, 1 << 22) > 1 << 32                               # the size needs more than 32 bits before the shape does
    assert ws(1, 8, 0) < 0 and b"no known point" in L.gad_last_error()
    assert ws(-1, 8, 64) < 0 and b"B=-1" in L.gad_last_error()
    assert ws(1, -8, 64) < 0 and b"n=-8" in L.gad_last_error()
    assert ws(1, 8, -64) < 0 and b"m=-64" in L.gad_last_error()
    assert ws(1, 8, 800000000) < 0 and b"overflows" in L.gad_last_error()
    assert ws(1024, 8, 1 << 21) < 0 and b"overflows" in L.gad_last_error()
    assert ws(1024, 1 << 21, 64) < 0 and b"overflows" in L.gad_last_error()
    assert ws(65536, 8, 64) < 0 and b"65535" in L.gad_last_error()
    assert ws(2, 0, 0) > 0                                              # nothing to search is no error


def test_routing_predicate_under_the_three_option_values(monkeypatch):
    """one LDS tile of gad_three_nn (m <= 1024) keeps the exhaustive kernel whatever the option says; tnn_grid = 2 makes m = 1025
    the first cloud sent to the grid, the default 1 the measured 8192 (profiles/three_nn_grid.txt), 0 routes nothing.  n does
    not enter the rule."""
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    _lib()
    assert (pu.TNN_LDS_TILE, pu.TNN_GRID_MIN_M) == (1024, 8192)
    assert "m >= 8192" in open(os.path.join(ROOT, "profiles", "three_nn_grid.txt")).read()     # the table the constant cites
    monkeypatch.setitem(hip._options, "tnn_grid", 2)
    for n in (1, 300, 1 << 20):
        for m in (1, 3, 512, 1023, 1024):
            assert not pu.three_nn_uses_grid(n, m), (n, m)
        for m in (1025, 4097, 20000, 262144, 1 << 22):
            assert pu.three_nn_uses_grid(n, m), (n, m)
    monkeypatch.setitem(hip._options, "tnn_grid", 1)
    for n in (1, 300, 1 << 20):
        for m in (1, 1024, 1025, 4097, 8191):
            assert not pu.three_nn_uses_grid(n, m), (n, m)
        for m in (8192, 8193, 262144, 1 << 22):
            assert pu.three_nn_uses_grid(n, m), (n, m)
    monkeypatch.setitem(hip._options, "tnn_grid", 0)
    for m in (1024, 1025, 8192, 262144, 1 << 22):
        assert not pu.three_nn_uses_grid(300, m), m


def test_facade_entry_points_by_shape(monkeypatch):
    """the entry point pointnet2_utils.three_nn names for a shape (the call itself is replaced: no launch): shapes the predicate
    rejects make exactly the call they made before the grid existed"""
    import torch
    from ga_ddpg_amd import hip
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    _lib()
    calls = []
    monkeypatch.setattr(hip, "call", lambda name, *a: calls.append((name,) + tuple(a)))
    monkeypatch.setattr(hip, "require_cuda", lambda *t: None)
    monkeypatch.setattr(hip, "workspace", lambda name, device, *shape: ("workspace", name) + shape)
    monkeypatch.setattr(torch, "sqrt", lambda t: t)                    # (the outputs are uninitialised host memory here)
    old, grid = "gad_three_nn", "gad_three_nn_grid"
    for mode, cases in [(2, [(1, old), (1024, old), (1025, grid), (5000, grid)]),
                        (1, [(1024, old), (1025, old), (5000, old), (8191, old), (8192, grid), (300000, grid)]),
                        (0, [(1024, old), (1025, old), (8192, old), (300000, old)])]:
        monkeypatch.setitem(hip._options, "tnn_grid", mode)
        for m, want in cases:
            del calls[:]
            unknown, known = torch.zeros(2, 7, 3), torch.zeros(2, m, 3)
            dist, idx = pu.three_nn(unknown, known)
            assert tuple(dist.shape) == (2, 7, 3) and tuple(idx.shape) == (2, 7, 3) and idx.dtype == torch.int32
            assert len(calls) == 1 and calls[0][0] == want, (mode, m, calls[0][0])
            a = calls[0][1:]
            assert a[2:5] == (2, 7, m) and a[5] is dist and a[6] is idx
            if want == grid:                                            # ..., stats = NULL, a workspace sized for this call
                assert len(a) == 9 and a[7] is None and a[8] == ("workspace", grid, 2, 7, m)
            else:
                assert len(a) == 7
