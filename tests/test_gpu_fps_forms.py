"""Every form of furthest point sampling in ga-ddpg_amd/csrc/fps.hip -- each fps_kernel<points per lane, wavefronts>
instantiation gad_furthest_point_sampling can launch, library option "fps_cfg" = 1 .. 4 included, and gad_fps_tiled where stated --
called directly and held to the C oracle (oracle/cref.fps): indices bit for bit, new_xyz bit for bit against the gathered rows.
idx starts as -7 and new_xyz as NaN, so "equal" includes that everything was written.

The launches record no kernel name (gad_furthest_point_sampling does not register with gad_last_kernel), so a case cannot assert
its route: the (cfg, N) -> form table below is DERIVED FROM THE DISPATCH in gad_furthest_point_sampling (N <= 64, <= 1024, <= 4096,
beyond; fps_cfg picks among the forms of the two middle ranges) and must follow it when that changes.  With lane t of a form owning
k = s * T + t (T = 64 * wavefronts) and tie_bs = pow2 <= min(N, 512), R = tie_bs / T selects the walk through a lane's points.

a. every form at the smallest shapes that reach each of its paths, four clouds a case (skip block + duplicate run, lattice, doubled
   lattice with the start point skipped, coordinates of 1e6), with and without new_xyz, M = N on the default route;
b. directed ties: one far point stored twice in ONE lane, where the oracle picks the higher index (fps_reference.TIES);
c. contraction traps: clouds on which a distance or a skip norm with any product fused into a sum picks differently
   (tests/test_fps_reference.py shows on the CPU that each of them does separate the evaluations);
d. NaN / infinite / huge coordinates: upstream's picks (a NaN distance never updates temp and never wins);
e. the entry point's shape edges: the LDS budget filled to the byte, the refusals, empty calls, M = 1.
The last test checks that "fps_cfg" is back at its default."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import fps_reference as R

pytestmark = pytest.mark.gpu

SENT = -7


def _hip():
    from ga_ddpg_amd import hip
    return hip


@contextlib.contextmanager
def _cfg(cfg):
    hip = _hip()
    try:
        hip.set_option("fps_cfg", cfg)
        yield
    finally:
        hip.set_option("fps_cfg", hip.get_option_default("fps_cfg"))


def _outputs(B, M, with_new_xyz):
    idx = torch.full((B, M), SENT, dtype=torch.int32, device="cuda")
    new_xyz = torch.full((B, M, 3), float("nan"), device="cuda") if with_new_xyz else None
    return idx, new_xyz


def _lds(xyz, M, with_new_xyz=True):
    """a direct call of the one-workgroup entry point -> (idx, new_xyz | None) as numpy arrays"""
    B, N, _ = xyz.shape
    x = torch.from_numpy(np.array(xyz, dtype=np.float32)).cuda()
    idx, new_xyz = _outputs(B, M, with_new_xyz)
    _hip().call("gad_furthest_point_sampling", x, B, N, M, idx, new_xyz)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), (new_xyz.cpu().numpy() if with_new_xyz else None)


def _tiled(xyz, M, with_new_xyz=True, groups=3):
    hip = _hip()
    B, N, _ = xyz.shape
    x = torch.from_numpy(np.array(xyz, dtype=np.float32)).cuda()
    ws = hip.workspace("gad_fps_tiled", "cuda", B, N, M, groups)
    idx, new_xyz = _outputs(B, M, with_new_xyz)
    hip.call("gad_fps_tiled", x, B, N, M, groups, idx, new_xyz, ws)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), (new_xyz.cpu().numpy() if with_new_xyz else None)


def _check(run, xyz, want, names=None, **kw):
    """run(xyz, M, **kw) against the oracle's picks `want` (B, M): idx, and new_xyz where the call produces it"""
    got, new_xyz = run(xyz, want.shape[1], **kw)
    assert got.dtype == np.int32 and got.shape == want.shape
    for b in range(want.shape[0]):
        np.testing.assert_array_equal(got[b], want[b], err_msg="cloud %s" % (names[b] if names else b))
    if new_xyz is not None:
        np.testing.assert_array_equal(new_xyz, np.take_along_axis(xyz, want[:, :, None].astype(np.int64), axis=1))
    return got


@functools.lru_cache(maxsize=None)
def _case(names, N, M):
    """(clouds (B, N, 3), the oracle's picks (B, M)) of the named fps_reference.cloud kinds, computed once and read-only"""
    from oracle import cref
    xyz = np.stack([R.cloud(kind, N) for kind in names])
    want = cref.fps(xyz, M)
    xyz.flags.writeable = False
    want.flags.writeable = False
    return xyz, want


# ----------------------------------------------------------------------------- a. every instantiation
FOUR = ("random", "lattice", "lattice2", "far6")
# (cfg, N, form): the dispatch of gad_furthest_point_sampling, restated (module docstring)
FORMS = ([(cfg, N, "<1,1>") for cfg in range(5) for N in (1, 2, 3, 33, 64)]                # scalar path, tie_bits 0 / 1 / 5 / 6
         + [(0, N, "<4,4>") for N in (65, 255, 256, 257)]                                  # R 0 (tie_bs < T), empty lanes, k clamped to N - 1
         + [(0, N, "<4,4>") for N in (511, 512, 513, 1023, 1024)]                          # R 1 -> 2
         + [(0, N, "<16,4>") for N in (1025, 4095, 4096)]                                  # R = 2, all 16 s in use only near 4096
         + [(0, 4097, "<16,16>")]                                                          # T = 1024 > tie_bs
         + [(1, N, "<8,8>") for N in (1025, 4096)]                                         # T = 512 = tie_bs
         + [(2, N, "<4,16>") for N in (1025, 4096)]                                        # T = 1024
         + [(3, N, "<16,1>") for N in (100, 200, 300, 1000, 1024)]                         # R = 1, 2, 4, 8, 8
         + [(3, N, "<64,1>") for N in (1025, 4096)]                                        # R = 8 with 17 and 64 s
         + [(4, N, "<8,2>") for N in (100, 200, 300, 1024)]                                # R 0, 1, 2, 4
         + [(4, N, "<32,2>") for N in (1025, 4096)])                                       # R = 4


def _expected_form(cfg, N):
    if N <= 64:
        return "<1,1>"
    if N <= 1024:
        return {3: "<16,1>", 4: "<8,2>"}.get(cfg, "<4,4>")
    if N <= 4096:
        return {1: "<8,8>", 2: "<4,16>", 3: "<64,1>", 4: "<32,2>"}.get(cfg, "<16,4>")
    return "<16,16>"


def test_the_table_names_every_form():
    assert all(_expected_form(cfg, N) == form for cfg, N, form in FORMS)
    assert {form for _, _, form in FORMS} == {"<1,1>", "<4,4>", "<16,4>", "<16,16>", "<16,1>", "<8,2>", "<64,1>", "<32,2>", "<8,8>",
                                              "<4,16>"}


@pytest.mark.parametrize("cfg,N,form", FORMS, ids=["cfg%d-N%d-%s" % c for c in FORMS])
def test_every_form_matches_the_oracle(cfg, N, form):
    Ms = [min(N, 64)] + ([N] if cfg == 0 and 64 < N <= 1025 else [])
    with _cfg(cfg):
        for M in Ms:
            xyz, want = _case(FOUR, N, M)
            _check(_lds, xyz, want, FOUR)
            if M == Ms[0]:
                _check(_lds, xyz, want, FOUR, with_new_xyz=False)


# ----------------------------------------------------------------------------- b. directed in-lane ties
@pytest.mark.parametrize("cfg,form,T,N,k1,k2,winner", R.TIES, ids=["cfg%d-%s-N%d-%d-%d" % (c[0], c[1], c[3], c[4], c[5]) for c in R.TIES])
def test_directed_tie(cfg, form, T, N, k1, k2, winner):
    from oracle import cref
    assert _expected_form(cfg, N) == form
    xyz = R.tie_cloud(N, k1, k2)[None]
    want = cref.fps(xyz, 4)
    assert want[0, 1] == (k1, k2)[winner - 1]                          # not vacuous: the designated index IS the oracle's pick
    with _cfg(cfg):
        _check(_lds, xyz, want)


# ----------------------------------------------------------------------------- c. contraction traps
# (route, cfg, N, placement of the two candidates, T the placement assumes)
TRAP_ROUTES = [("<1,1>", 0, 64, "wave", 64),
               ("<4,4>", 0, 1024, "lane", 256), ("<4,4>", 0, 1024, "wave", 256), ("<4,4>", 0, 1024, "block", 256),
               ("<16,4>", 0, 4096, "lane", 256), ("<16,4>", 0, 4096, "wave", 256), ("<16,4>", 0, 4096, "block", 256),
               ("<16,1>", 3, 1024, "lane", 64), ("<32,2>", 4, 4096, "lane", 128), ("<32,2>", 4, 4096, "block", 128),
               ("tiled", 0, 1000, "lane", 400), ("tiled", 0, 1000, "wave", 256)]     # "lane" at T = 400: two of the three slices


@functools.lru_cache(maxsize=None)
def _trap_case(N, lanes, T):
    from oracle import cref
    clouds = [R.distance_trap(v, N, lanes, T) for v in R.FUSED]
    skips = [t for v in R.FUSED for t in R.skip_trap(v, N)]
    xyz = np.stack(clouds + [t.xyz for t in skips])
    return xyz, cref.fps(xyz, 6), skips


@pytest.mark.parametrize("route,cfg,N,lanes,T", TRAP_ROUTES, ids=["%s-N%d-%s" % (c[0], c[2], c[3]) for c in TRAP_ROUTES])
def test_distance_and_skip_norm_are_not_fma_contracted(route, cfg, N, lanes, T):
    """five distance traps (one per fused form of (dx*dx + dy*dy) + dz*dz) and ten skip traps (per fused form of |p|^2, a point the
    pinned norm keeps and one it skips) in one batch: a kernel that fused any product into a sum picks differently on its cloud"""
    assert route == "tiled" or _expected_form(cfg, N) == route
    xyz, want, skips = _trap_case(N, lanes, T)
    names = ["distance %s" % v for v in R.FUSED] + ["skip %s kept=%s" % (v, k) for v in R.FUSED for k in (True, False)]
    for i, t in enumerate(skips):                                       # not vacuous: the oracle's picks show which side it is on
        assert (want[len(R.FUSED) + i, 1] == t.index) == t.kept and (t.index in want[len(R.FUSED) + i]) == t.kept
    with _cfg(cfg):
        _check(_tiled if route == "tiled" else _lds, xyz, want, names)


# ----------------------------------------------------------------------------- d. non-finite and far coordinates
NONFINITE_ROUTES = [("<1,1>", 0, 64), ("<4,4>", 0, 1024), ("<16,4>", 0, 4096), ("<16,16>", 0, 4097), ("<16,1>", 3, 1024),
                    ("<8,2>", 4, 1024), ("tiled", 0, 1000)]


@pytest.mark.parametrize("kind", R.NONFINITE)
@pytest.mark.parametrize("route,cfg,N", NONFINITE_ROUTES, ids=["%s-N%d" % (c[0], c[2]) for c in NONFINITE_ROUTES])
def test_non_finite_and_far_coordinates(route, cfg, N, kind):
    """upstream's picks: `d < temp ? d : temp` keeps temp for a NaN or infinite d, and a NaN never wins '>' -- the v_min_f32 /
    v_max3_f32 of the packed path, its `tm == bd` walk, `dmax >= 0` and the tiled kernel's workspace form all have to agree"""
    assert route == "tiled" or _expected_form(cfg, N) == route
    xyz, want = _case((kind,), N, 48)
    with _cfg(cfg):
        _check(_tiled if route == "tiled" else _lds, xyz, want, (kind,))


# ----------------------------------------------------------------------------- e. shape edges of the entry point
def _fits(N, M):
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    return pu.fps_fits_one_workgroup(N, M)


def _lds_floats(N, M):
    return ((N * 3 + 3) & ~3) + 64 + M                                # coordinates, exchange slots, picks (include/gaddpg.h)


def test_lds_budget_filled_exactly_with_few_picks():
    """the largest N that fits with M = 4 -- 13630: 40 892 + 64 + 4 floats = 160 KiB to the byte -- runs and matches"""
    N = max(n for n in range(13000, 14000) if _fits(n, 4))
    assert N == 13630 and _lds_floats(N, 4) * 4 == 160 * 1024 and not _fits(N, 5) and not _fits(N + 1, 4)
    xyz, want = _case(("random", "lattice2"), N, 4)
    _check(_lds, xyz, want)


def test_lds_budget_filled_exactly_with_all_picks():
    """N = M = 10224: 30 672 + 64 + 10 224 floats = 160 KiB; the last rounds run on an exhausted cloud"""
    N = max(n for n in range(10000, 10500) if _fits(n, n))
    assert N == 10224 and _lds_floats(N, N) * 4 == 160 * 1024
    xyz, want = _case(("random",), N, N)
    _check(_lds, xyz, want)


@pytest.mark.parametrize("N,M,why", [(13630, 5, "bytes of LDS"), (64, 65, "picks from"), (16385, 4, "unsupported shape")])
def test_refused_shapes_raise_write_nothing_and_route_to_the_tiled_kernel(N, M, why, monkeypatch):
    hip = _hip()
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    assert not _fits(N, M)
    xyz, want = _case(("random", "lattice"), N, M)
    x = torch.from_numpy(xyz.copy()).cuda()
    idx, new_xyz = _outputs(2, M, True)
    with pytest.raises(RuntimeError, match=why):
        hip.call("gad_furthest_point_sampling", x, 2, N, M, idx, new_xyz)
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == SENT).all() and np.isnan(new_xyz.cpu().numpy()).all()
    names, real = [], hip.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(hip, "call", spy)
    got = pu.furthest_point_sample(x, M).cpu().numpy()
    assert names == ["gad_fps_tiled"]
    np.testing.assert_array_equal(got, want)


def test_empty_calls_touch_nothing():
    hip = _hip()
    x = torch.from_numpy(R.cloud("random", 100)[None].copy()).cuda()
    idx, new_xyz = _outputs(1, 8, True)
    hip.call("gad_furthest_point_sampling", x, 0, 100, 8, idx, new_xyz)                # B = 0
    hip.call("gad_furthest_point_sampling", x, 1, 100, 0, idx, new_xyz)                # M = 0
    torch.cuda.synchronize()
    assert (idx.cpu().numpy() == SENT).all() and np.isnan(new_xyz.cpu().numpy()).all()


@pytest.mark.parametrize("N", (64, 300, 4097))
def test_one_pick_is_point_zero_even_inside_the_skip_ball(N):
    xyz = np.stack([R.cloud("random", N), R.cloud("lattice2", N)])
    xyz[0, 0] = (0.01, 0.0, -0.01)                                      # |p|^2 = 2e-4: skipped as a candidate, still the start
    assert (R.sqnorm()(xyz[:, 0]) < R.SKIP).all()
    got, new_xyz = _lds(xyz, 1)
    assert (got == 0).all()
    np.testing.assert_array_equal(new_xyz, xyz[:, :1])


# ----------------------------------------------------------------------------- last: the switch is back
def test_fps_cfg_is_back_at_its_default():
    import os
    hip = _hip()
    assert hip.get_option("fps_cfg") == hip.get_option_default("fps_cfg")
    if "GAD_OPT_fps_cfg" not in os.environ:
        assert hip.get_option_default("fps_cfg") == 0                   # the library's own default (csrc/common.hpp: GeometryOptions::fps_cfg)
