"""gad_three_nn_grid (include/gaddpg.h section A): three_nn through a uniform grid over the known points, against
tests/fp_reference.three_nn_ref (pinned on the CPU by tests/test_fp_reference.py) and against gad_three_nn on the same inputs --
indices equal, the float32 bits of the squared distances equal.  Direct calls of the entry point; every buffer lives between
guard bytes, outputs start as NaN / -1, and ONE workspace, filled with 0xFF bytes before every call, serves all shapes from the
largest to the smallest.  `stats` keeps the gates honest: a kernel that always took its exhaustive fallback would pass every
parity gate, so where the queries come from the cloud's own distribution at most 5 % of them may be redone exhaustively.

The clouds are the ones at which a ring search can go wrong: mass ties at equal d across different cells (a lattice with queries
on its nodes: the tie rule and the strictness of the stop test), duplicated and coincident points, boxes of zero extent, voids
(two clusters 100 edge lengths apart, a diagonal line), queries far outside the box, non-finite coordinates, fewer than three
finite points, and a distance that differs in its last bit under FMA contraction."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fp_reference as F
from tests.test_gpu_fp_ops import _contraction_sensitive_case, _fused_sqdist
from tests.test_gpu_optim_kernels import Buf, _nan32, _same

pytestmark = pytest.mark.gpu

f32 = np.float32
M_ALL = (20000, 4097, 1025, 65, 63, 4, 3, 2, 1)                 # largest first: the workspace is sized once, then reused
KINDS_ANY_M = ("cube", "surface", "lattice", "clusters", "outside")
KINDS_TO_4097 = ("duplicates", "equal", "flat", "collinear", "nonfinite")
_WS = {}


def _hip():
    from ga_ddpg_amd import hip
    return hip


def _shapes(kind, m):
    """(B, n) per cloud size: every n of (1, 65, 257, 3000) and both B at every size the CPU reference affords"""
    if m == 20000:
        return ((1, 257), (3, 65))
    if m == 4097:
        return ((3, 65), (1, 3000)) if kind in ("cube", "surface") else ((1, 1), (3, 257))
    if m == 1025:
        return ((1, 65), (3, 257), (1, 3000))
    return ((1, 1), (3, 65), (1, 257), (3, 3000))


def _boxes(a, lattice=False):
    """a different box per batch entry: as sampled; shifted far from the origin; larger (lattice: by node-preserving amounts)"""
    a = a.astype(np.float64)
    if a.shape[0] > 1:
        a[1] += (4.0, -2.0, 1.0) if lattice else (100.0, -50.0, 30.0)
    if a.shape[0] > 2:
        a[2] *= 2.0 if lattice else 10.0
    return a.astype(f32)


def _clouds(kind, B, n, m, seed):
    """-> unknown (B,n,3), known (B,m,3) float32"""
    from ga_ddpg_amd.synth_data import box_surface_cloud
    rng = np.random.default_rng(seed)
    cube = lambda k: rng.random((B, k, 3)) * 0.4 + 0.1
    if kind == "cube":
        unknown, known = cube(n), cube(m)
    elif kind == "surface":
        edges = (0.3, 0.2, 0.1)
        known = np.stack([box_surface_cloud(rng, m, edges) for _ in range(B)]) + 0.25
        unknown = np.stack([box_surface_cloud(rng, n, edges) for _ in range(B)]) + 0.25
    elif kind == "lattice":
        L = int(min(28, max(2, round(m ** (1.0 / 3.0)))))           # about one point per node: ties at every distance
        known = rng.integers(0, L, size=(B, m, 3)) * 0.125
        unknown = rng.integers(-3, L + 3, size=(B, n, 3)) * 0.125   # on nodes, some up to three steps outside the box
        both = _boxes(np.concatenate([unknown, known], 1), True)
        return np.ascontiguousarray(both[:, :n]), np.ascontiguousarray(both[:, n:])
    elif kind == "duplicates":
        unknown, known = cube(n), cube(m)
        known[:, m // 2:] = known[:, :m - m // 2]
    elif kind == "equal":
        known = np.broadcast_to(cube(1), (B, m, 3)).copy()
        unknown = known[:, :1] + (rng.random((B, n, 3)) - 0.5) * 0.2
        unknown[:, ::3] = known[:, :1]                              # every third query ON the point
    elif kind == "flat":
        unknown, known = cube(n), cube(m)
        known[:, :, 2] = 0.375
        unknown[:, ::2, 2] = 0.375                                  # on the plane and off it
    elif kind == "collinear":
        t = rng.random((B, m, 1))
        d = np.array([[1.0, 0.0, 0.0], [0.3, 0.2, 0.1], [0.0, 0.25, -0.25]])[:B].reshape(B, 1, 3)   # an axis, a diagonal, a face diagonal
        known = 0.1 + t * d
        unknown = 0.1 + rng.random((B, n, 1)) * d + (rng.random((B, n, 3)) - 0.5) * (0.02 * (np.arange(n) % 2))[None, :, None]
    elif kind == "clusters":
        e = 0.01                                                    # two clusters of edge e, 100 e apart along the diagonal
        where = rng.integers(0, 2, size=(B, m, 1))
        known = 0.2 + rng.random((B, m, 3)) * e + where * (100 * e)
        s = np.arange(n) % 3                                        # queries in the first cluster, the second, the void between
        void = rng.random((B, n, 1)) * (100 * e) + (rng.random((B, n, 3)) - 0.5) * e
        unknown = 0.2 + np.where((s == 2)[None, :, None], void, rng.random((B, n, 3)) * e + (s == 1)[None, :, None] * (100 * e))
    elif kind == "outside":
        known = cube(m)
        unknown = 0.1 + (rng.random((B, n, 3)) * 5.0 - 2.0) * 0.4   # up to two box widths beyond every face
    elif kind == "nonfinite":
        unknown, known = cube(n), cube(m)
        bad = np.array([np.nan, np.inf, -np.inf])
        for b in range(B):
            for j, k in enumerate(rng.choice(m, size=min(m, 7), replace=False)):
                known[b, k, j % 3] = bad[j % 3]
            for j, i in enumerate(rng.choice(n, size=min(n // 2, 5), replace=False)):
                unknown[b, i, (j + 1) % 3] = bad[j % 3]
        known[B - 1, 2:] = np.nan                                   # the last cloud: fewer than three finite points
        if m >= 4:
            known[B - 1, 3, 0] = 0.3                                # (one coordinate finite is not a finite point)
    else:
        raise AssertionError(kind)
    return _boxes(unknown), _boxes(known)


def _reference(unknown, known):
    """three_nn_ref over blocks of at most 256 queries (it materialises (B, n, m, 3))"""
    d, i = [], []
    with np.errstate(all="ignore"):
        for s in range(0, unknown.shape[1], 256):
            dd, ii = F.three_nn_ref(unknown[:, s:s + 256], known)
            d.append(dd)
            i.append(ii)
    return np.concatenate(d, 1), np.concatenate(i, 1)


def _workspace(B, n, m):
    """the module's one workspace (sized by the first, largest, request; asserted large enough afterwards), 0xFF-filled"""
    hip = _hip()
    need = hip.lib().gad_three_nn_grid_workspace_bytes(B, n, m)
    assert need > 0
    if "t" not in _WS:
        _WS["t"] = torch.empty(max(need, hip.lib().gad_three_nn_grid_workspace_bytes(3, 1, M_ALL[0])), dtype=torch.uint8, device="cuda")
    assert _WS["t"].numel() >= need
    _WS["t"].fill_(0xFF)
    return _WS["t"]


def _grid(bu, bk, B, n, m, with_stats=True):
    """a direct call on fresh outputs -> (dist2, idx, stats | None)"""
    hip = _hip()
    bd, bi = Buf(_nan32((B, n, 3))), Buf(np.full((B, n, 3), -1, np.int32))
    bs = Buf(np.full((B, 2), -1, np.int32)) if with_stats else None
    hip.call("gad_three_nn_grid", bu.ptr, bk.ptr, B, n, m, bd.ptr, bi.ptr, bs.ptr if bs else None, _workspace(B, n, m))
    return bd.get("dist2"), bi.get("idx"), bs.get("stats") if bs else None


def _exhaustive(bu, bk, B, n, m):
    bd, bi = Buf(_nan32((B, n, 3))), Buf(np.full((B, n, 3), -1, np.int32))
    _hip().call("gad_three_nn", bu.ptr, bk.ptr, B, n, m, bd.ptr, bi.ptr)
    return bd.get("dist2"), bi.get("idx")


def _check(kind, B, n, m, unknown, known):
    want_d, want_i = _reference(unknown, known)
    bu, bk = Buf(unknown), Buf(known)
    what = "three_nn_grid %s B %d n %d m %d" % (kind, B, n, m)
    got_d, got_i, stats = _grid(bu, bk, B, n, m)
    _same(what + " idx", got_i, want_i)
    _same(what + " dist2", got_d, want_d)
    ex_d, ex_i = _exhaustive(bu, bk, B, n, m)
    _same(what + " idx vs gad_three_nn", got_i, ex_i)
    _same(what + " dist2 vs gad_three_nn", got_d, ex_d)
    assert (stats >= 0).all() and (stats.sum(axis=1) == n).all(), (what, stats)
    no_d, no_i, _ = _grid(bu, bk, B, n, m, with_stats=False)            # stats = NULL: the same outputs
    _same(what + " idx without stats", no_i, got_i)
    _same(what + " dist2 without stats", no_d, got_d)
    _same(what + " unknown", bu.get("unknown"), unknown)
    _same(what + " known", bk.get("known"), known)
    print("GATE %s: redone exhaustively %s of %d" % (what, stats[:, 1].tolist(), n))
    return want_d, want_i, stats


CASES = [(kind, m) for m in M_ALL for kind in KINDS_ANY_M + (KINDS_TO_4097 if m <= 4097 else ())]


@pytest.mark.parametrize("kind,m", CASES)
def test_bit_exact_against_reference_and_exhaustive_kernel(kind, m):
    for B, n in _shapes(kind, m):
        unknown, known = _clouds(kind, B, n, m, 100 * m + 10 * n + B)
        want_d, want_i, stats = _check(kind, B, n, m, unknown, known)
        if m < 3:
            assert (want_i[:, :, m:] == 0).all() and np.isposinf(want_d[:, :, m:]).all()
        if kind == "nonfinite":
            assert np.isposinf(want_d[B - 1]).sum() >= n * (3 - min(m, 2))          # at most two finite points in the last cloud
            bad = ~np.isfinite(unknown).all(axis=2)
            assert n == 1 or bad.any()
            assert np.isposinf(want_d[bad]).all() and (want_i[bad] == 0).all()
        if kind == "lattice" and m >= 63 and n >= 65:                   # ties at equal d exist in the answers, across nodes
            assert (want_d[:, :, 0] == want_d[:, :, 1]).any() or (want_d[:, :, 1] == want_d[:, :, 2]).any()
        if kind in ("cube", "surface") and m >= 4097:
            # the queries come from the cloud's own distribution: the grid has to answer them (5 %: the CPU model of the
            # first-ring stop test with a 1 % margin fails 0 of 3000 such queries at m = 4097 / 5000 / 20000)
            assert (stats[:, 1] * 20 <= n).all(), (kind, B, n, m, stats)


def test_contraction_sensitive_distance_in_a_large_cloud():
    """the FMA-contraction trap of test_gpu_fp_ops, padded to m = 4097: the nearest neighbour differs between the pinned
    evaluation of d and the one with dy*dy + dx*dx fused -- the grid's candidates get the pinned one"""
    B, n, m = 3, 65, 4097
    unknown, known = _clouds("cube", B, n, m, 77)
    for b in range(B):
        unknown[b, 0], known[b] = _contraction_sensitive_case(7 * 4097 + b, m)
    want_d, want_i, _ = _check("contraction", B, n, m, unknown, known)
    for b in range(B):                                                   # the case does tell the two evaluations apart, on the CPU
        fi = np.argsort(_fused_sqdist(unknown[b, 0], known[b]), kind="stable")[:3]
        assert fi[0] != want_i[b, 0, 0] and {int(fi[0]), int(want_i[b, 0, 0])} == {0, m - 1}


def test_option_0_runs_the_exhaustive_kernel_through_the_same_entry_point():
    hip = _hip()
    B, n, m = 3, 257, 4097
    unknown, known = _clouds("surface", B, n, m, 5)
    bu, bk = Buf(unknown), Buf(known)
    on_d, on_i, on_stats = _grid(bu, bk, B, n, m)
    try:
        hip.set_option("tnn_grid", 0)
        off_d, off_i, off_stats = _grid(bu, bk, B, n, m)
    finally:
        hip.set_option("tnn_grid", 1)
    _same("tnn_grid 0 idx", off_i, on_i)
    _same("tnn_grid 0 dist2", off_d, on_d)
    assert (off_stats == np.array([0, n], np.int32)).all() and (on_stats[:, 0] > 0).all()


def test_replayed_from_a_plan():
    """the entry point as an item of a gad_plan, one gad_plan_run: bit-equal to the direct call"""
    from ga_ddpg_amd import engine
    hip = _hip()
    L = hip.lib()
    B, n, m = 3, 257, 4097
    unknown, known = _clouds("cube", B, n, m, 6)
    bu, bk = Buf(unknown), Buf(known)
    want_d, want_i, want_stats = _grid(bu, bk, B, n, m)
    bd, bi, bs = Buf(_nan32((B, n, 3))), Buf(np.full((B, n, 3), -1, np.int32)), Buf(np.full((B, 2), -1, np.int32))
    h = C.c_void_p()
    try:
        hip.check(L.gad_plan_create(C.byref(h)), "gad_plan_create")
        words, kinds = engine._pack_words(hip._args(bu.ptr, bk.ptr, B, n, m, bd.ptr, bi.ptr, bs.ptr, _workspace(B, n, m)))
        k = len(words)
        rc = L.gad_plan_add_call(h, b"gad_three_nn_grid", (C.c_uint64 * k)(*words), (C.c_uint8 * k)(*kinds), k, 0)
        assert rc >= 0, L.gad_last_error()
        table = (C.c_void_p * 1)(torch.cuda.current_stream().cuda_stream)
        hip.check(L.gad_plan_run(h, table, 1, 0, -1), "gad_plan_run")
        torch.cuda.synchronize()
    finally:
        L.gad_plan_destroy(h)
    _same("plan replay idx", bi.get("idx"), want_i)
    _same("plan replay dist2", bd.get("dist2"), want_d)
    _same("plan replay stats", bs.get("stats"), want_stats)


def test_nothing_to_search():
    """B * n == 0: GAD_OK without a launch, a NULL workspace is legal and the outputs stay as they were"""
    hip = _hip()
    L = hip.lib()
    known = torch.rand(2, 5000, 3, device="cuda")
    unknown = torch.rand(2, 4, 3, device="cuda")
    d = torch.full((2, 4, 3), -7.0, device="cuda")
    i = torch.full((2, 4, 3), -7, dtype=torch.int32, device="cuda")
    s = torch.full((2, 2), -7, dtype=torch.int32, device="cuda")
    null, p = C.c_void_p(None), lambda t: C.c_void_p(t.data_ptr())
    assert L.gad_three_nn_grid(p(unknown), p(known), 0, 4, 5000, p(d), p(i), p(s), null, hip.stream()) == 0
    assert L.gad_three_nn_grid(p(unknown), p(known), 2, 0, 5000, p(d), p(i), p(s), null, hip.stream()) == 0
    assert L.gad_three_nn_grid(p(unknown), p(known), 2, 0, 0, p(d), p(i), null, null, hip.stream()) == 0
    torch.cuda.synchronize()
    assert (d == -7).all() and (i == -7).all() and (s == -7).all()


def test_facade_routing(monkeypatch):
    """pointnet2_utils.three_nn: with library option tnn_grid = 2, m = 1025 reaches gad_three_nn_grid and m = 1024 (one LDS tile)
    does not; with 0 every shape runs gad_three_nn; the default follows three_nn_uses_grid.  Same outputs on every route."""
    hip = _hip()
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    names, real = [], hip.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(hip, "call", spy)

    def run(m, want_name):
        unknown, known = _clouds("cube", 2, 300, m, m)
        want_d, want_i = _reference(unknown, known)
        del names[:]
        dist, idx = pu.three_nn(torch.from_numpy(unknown).cuda(), torch.from_numpy(known).cuda())
        assert names == [want_name], (m, names)
        assert idx.dtype == torch.int32 and dist.dtype == torch.float32
        _same("three_nn idx m %d" % m, idx.cpu().numpy(), want_i)
        _same("three_nn dist m %d" % m, dist.cpu().numpy(), np.sqrt(want_d))

    try:
        hip.set_option("tnn_grid", 2)
        run(1025, "gad_three_nn_grid")
        run(1024, "gad_three_nn")
        hip.set_option("tnn_grid", 0)
        run(1025, "gad_three_nn")
        run(1024, "gad_three_nn")
    finally:
        hip.set_option("tnn_grid", 1)
    for m in (1024, 1025, 8191, 8192):                                 # the default follows three_nn_uses_grid
        assert pu.three_nn_uses_grid(300, m) == (m >= pu.TNN_GRID_MIN_M)
        run(m, "gad_three_nn_grid" if pu.three_nn_uses_grid(300, m) else "gad_three_nn")


def test_fp_module_is_the_same_on_both_routes():
    """PointnetFPModule (mlp [24, 16], n = 3000, m = 1500, C = 8 + 16): the forward output and every gradient with three_nn on the
    grid (tnn_grid = 2) are bit-equal to the same module with tnn_grid = 0 -- same indices, then the same kernels.  Both runs are
    made reproducible first, or two runs of ONE route would differ as well: torch's switch for reproducible results (its
    convolution's weight gradient is not bit-reproducible without it: 351 of 384 elements of mlp.0.weight.grad differed in the
    last bits between the routes while the forward and the feature gradients were equal), which also puts library option
    "deterministic" in force (the default gradient of three_interpolate adds with float atomics in no fixed order)."""
    hip = _hip()
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    from ga_ddpg_amd.pointnet2_ops.pointnet2_modules import PointnetFPModule
    B, n, m, C1, C2 = 2, 3000, 1500, 8, 16
    torch.manual_seed(3000)
    mod = PointnetFPModule(mlp=[C1 + C2, 16], bn=True).cuda().train()
    unknown, known = (torch.rand(B, n, 3) * 0.4 + 0.1).cuda(), (torch.rand(B, m, 3) * 0.4 + 0.1).cuda()
    uf, kf, G = torch.randn(B, C1, n).cuda(), torch.randn(B, C2, m).cuda(), torch.randn(B, 16, n).cuda()
    names, real = [], hip.call
    was = hip.get_option_default("deterministic")
    torch_was = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
                 torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)

    def run(mode):
        hip.set_option("tnn_grid", mode)
        a, b = uf.clone().requires_grad_(True), kf.clone().requires_grad_(True)
        mod.zero_grad(set_to_none=True)
        del names[:]
        hip.call = lambda name, *args: (names.append(name), real(name, *args))[1]
        try:
            y = mod(unknown, known, a, b)
            (y * G).sum().backward()
        finally:
            hip.call = real
        assert ("gad_three_nn_grid" in names) == (mode == 2) and ("gad_three_nn" in names) == (mode == 0)
        out = {"forward": y.detach(), "unknow_feats.grad": a.grad, "known_feats.grad": b.grad}
        out.update({"mlp.%s.grad" % k: p.grad.clone() for k, p in mod.mlp.named_parameters()})
        return {k: v.cpu().numpy() for k, v in out.items()}

    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        hip.set_option("deterministic", 1)
        assert pu.TNN_LDS_TILE < m and hip.deterministic() == 1
        grid, exhaustive = run(2), run(0)
    finally:
        hip.call = real
        torch.use_deterministic_algorithms(torch_was[0], warn_only=torch_was[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = torch_was[2], torch_was[3]
        hip.set_option("tnn_grid", 1)
        hip.set_option("deterministic", was)
    assert set(grid) == set(exhaustive) and len(grid) >= 6
    for k in sorted(grid):
        _same("PointnetFPModule " + k, grid[k], exhaustive[k])
