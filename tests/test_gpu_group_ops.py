"""The grouping and row-building kernels of ga-ddpg_amd/csrc/ball_query.hip and group.hip -- gad_query_and_group / gad_ball_query on every route,
gad_group_points / gad_gather_points and their gradients, gad_prep_points, gad_rows_from_ball_query, gad_rows_group_all -- called
directly and compared with the plain numpy references of tests/group_reference.py (pinned on the CPU by tests/test_group_reference.py).

Yardsticks.  Indices, counts, offsets, copies and the recentred coordinates (one rounded float32 subtraction): bit for bit.  The
atomic gradient: exact where a destination takes 0, 1 or 2 entries (one rounding; float addition commutes), and within
(n + 2) * 2^-24 * sum |terms| of the float64 sum where it takes n >= 3 -- the bound of tests/gemm_cases.py for a float32 sum of n
terms in any order.  The deterministic gradient: bit for bit against a float32 accumulation in ascending entry order.

Every device buffer lives between two 64-byte guard zones filled with 0xA5 that must come back untouched; outputs start as NaN
(float32) or a negative sentinel (int32), and "bit for bit" includes that none of either is left in the live region.  All inputs
come from seeded generators.

Routes.  The geometry launches record no kernel name, so each query case states the dispatch predicates of ball_query.hip that place
it (_route below restates bq_route) and the tile scan below nsample = 129 is forced with option bq_cells = 0."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import group_reference as R

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64                      # bytes
FILL = 0xA5
SENT = -7654321                 # what an int32 output holds before the call
GPG_NT = 8192                   # group.hip: destinations per LDS tile of the deterministic gradient kernel


def _hip():
    from ga_ddpg_amd import hip
    return hip


# ----------------------------------------------------------------------------- plumbing
class Buf(object):
    """a device buffer holding `a` between two guard zones; the payload starts 64 bytes into a 256-byte aligned allocation"""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.dtype, self.shape, self.nbytes = a.dtype, a.shape, a.nbytes
        raw = np.full(GUARD + a.nbytes + GUARD, FILL, np.uint8)
        raw[GUARD:GUARD + a.nbytes] = a.view(np.uint8).ravel()
        self.t = torch.from_numpy(raw).cuda()
        assert self.t.data_ptr() % 256 == 0
        self.ptr = _hip().Ptr(self.t.data_ptr() + GUARD)

    def get(self, what="buffer"):
        torch.cuda.synchronize()
        raw = self.t.cpu().numpy()
        assert (raw[:GUARD] == FILL).all() and (raw[GUARD + self.nbytes:] == FILL).all(), "%s: guard bytes written" % what
        return raw[GUARD:GUARD + self.nbytes].copy().view(self.dtype).reshape(self.shape)


def _out_f(*shape):
    return Buf(np.full(shape, np.nan, f32))


def _out_i(*shape):
    return Buf(np.full(shape, SENT, np.int32))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _untouched(a):
    """mask of the elements that still hold what the buffer was filled with before the call"""
    a = np.asarray(a)
    return _bits(a) == _bits(np.full(1, np.nan, f32))[0] if a.dtype == f32 else a == SENT


def _diff(what, got, want):
    """bit-for-bit gate of one output: [] or [(message, mask of the offending elements)]"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = []
    left = _untouched(got)
    if left.any():
        bad.append(("%s: %d of %d elements were never written" % (what, int(left.sum()), left.size), left))
    ne = _bits(got) != _bits(want)
    if ne.any():
        i = np.unravel_index(int(np.flatnonzero(ne.ravel())[0]), ne.shape) if ne.ndim else ()
        bad.append(("%s: %d of %d elements differ bitwise; first at %s: got %r want %r" % (
            what, int(ne.sum()), ne.size, i, got[i], want[i]), ne))
    return bad


def _report(bad):
    return "\n".join(m for m, _ in bad)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


def _restore(name):
    hip = _hip()
    hip.set_option(name, hip.get_option_default(name))


# ----------------------------------------------------------------------------- a. fused query-and-group, every route
def _route(N, S, C, bq_cells):
    """where gad_query_and_group / gad_ball_query send a shape (ball_query.hip's bq_route: cells, then tiled, else the scan; the
    radii used here are positive and small) and which grouped write-out the cells kernel then takes (SP == 64 && C <= BQC_CPIPE)"""
    in_lds = 1024 < N <= 4096
    if bq_cells and in_lds and S <= 128:
        if S <= 64:
            return "cells64.pipe" if C <= 4 else "cells64.plain"
        return "cells128"
    if in_lds and S <= 256:
        return "tiled"
    return "scan"


# (route, N, S, C, M, bq_cells): a covering subset -- every value of every column of the issue's table appears in its row
QG_CASES = [
    ("scan", 1024, 1, 0, 1, 1), ("scan", 1024, 64, 1, 5, 1), ("scan", 1024, 65, 5, 5, 1),      # N at the LDS routes' low edge
    ("scan", 4097, 16, 3, 7, 1),                                                               # N beyond BQ_MAXN
    ("scan", 1100, 257, 2, 5, 1),                                                              # S beyond the tiled limit
    ("cells64.pipe", 1025, 1, 0, 1, 1), ("cells64.pipe", 2501, 17, 1, 3, 1), ("cells64.pipe", 4096, 64, 4, 67, 1),
    ("cells64.pipe", 4096, 64, 1, 257, 1), ("cells64.pipe", 2501, 17, 4, 515, 1), ("cells64.pipe", 1025, 64, 2, 67, 1),
    ("cells64.pipe", 2501, 1, 3, 257, 1),
    ("cells64.plain", 1025, 17, 5, 3, 1), ("cells64.plain", 4096, 64, 9, 257, 1),
    ("cells128", 2501, 65, 0, 67, 1), ("cells128", 2501, 128, 4, 257, 1), ("cells128", 2501, 65, 5, 257, 1),
    # the tile scan where it is the default: 128 < S <= 256.  Dynamic LDS 3 * 4 N + 256 S bytes: 45 324 at (1025, 129) -- under 64 KiB
    # --, 100 352 at (4096, 200), 114 688 at (4096, 256)
    ("tiled", 1025, 129, 0, 1, 1), ("tiled", 4096, 200, 4, 63, 1), ("tiled", 4096, 256, 5, 65, 1),
    ("tiled", 2501, 17, 1, 63, 0), ("tiled", 2501, 64, 5, 64, 0), ("tiled", 2501, 128, 1, 65, 0), ("tiled", 2501, 64, 5, 130, 0),
]


@functools.lru_cache(maxsize=None)
def _qg_case(N, S, C, M):
    """inputs and reference of one query case, computed once.  B = 2 clouds uniform in the unit cube, centroids = picked points,
    radius such that a ball in the interior holds about S / 3 points; centroid (0, 0) is moved far outside (empty ball: pad
    index 0, grouped coordinates = point 0 - centre); centroid (1, M - 1) sits in a crowd of S + 3 points closer than r"""
    rng = np.random.default_rng(1000003 * N + 1009 * S + 31 * C + M)
    B = 2
    r = float(f32((S / (4.0 * math.pi * N)) ** (1.0 / 3.0)))
    xyz = rng.random((B, N, 3)).astype(f32)
    crowd = rng.choice(N, size=S + 3, replace=False)
    centre = f32(0.3) + rng.random(3).astype(f32) * f32(0.4)
    xyz[1, crowd] = centre + (rng.random((S + 3, 3)).astype(f32) - f32(0.5)) * f32(r / 2)    # pairwise closer than 0.87 r
    pick = np.stack([rng.choice(N, size=M, replace=False) for _ in range(B)])
    new_xyz = np.take_along_axis(xyz, pick[..., None], 1).copy()
    new_xyz[0, 0] += f32(10.0)
    new_xyz[1, M - 1] = xyz[1, crowd[0]]
    feats = rng.normal(size=(B, C, N)).astype(f32) if C else None
    idx, cnt = R.ball_query(new_xyz, xyz, r, S)
    idx2, out = R.query_and_group(new_xyz, xyz, feats, r, S)
    assert (idx == idx2).all()
    # the edges are there, and the test is not vacuous: balls neither all empty nor all full
    assert cnt[0, 0] == 0 and (idx[0, 0] == 0).all()
    assert (R.sqdist32(new_xyz[1, M - 1:], xyz[1])[0] < f32(r) * f32(r)).sum() > S and cnt[1, M - 1] == S
    assert 0 < cnt.mean() < S, cnt.mean()
    _frozen(xyz, new_xyz, feats, idx, cnt, out)
    return {"B": B, "r": r, "xyz": xyz, "new_xyz": new_xyz, "feats": feats, "idx": idx, "cnt": cnt, "out": out}


def _run_qg(N, S, C, M, bq_cells):
    """gad_query_and_group (idx, out) and gad_ball_query (idx, cnt: the same predicates, out == nullptr) on one case"""
    hip = _hip()
    case = _qg_case(N, S, C, M)
    B, r = case["B"], case["r"]
    bx, bn = Buf(case["xyz"]), Buf(case["new_xyz"])
    bf = Buf(case["feats"]) if C else None
    idx, out = _out_i(B, M, S), _out_f(B, 3 + C, M, S)
    idx2, cnt = _out_i(B, M, S), _out_i(B, M)
    try:
        hip.set_option("bq_cells", bq_cells)
        hip.call("gad_query_and_group", bn.ptr, bx.ptr, bf.ptr if C else None, B, C, N, M, r, S, idx.ptr, out.ptr)
        hip.call("gad_ball_query", bn.ptr, bx.ptr, B, N, M, r, S, idx2.ptr, cnt.ptr)
    finally:
        _restore("bq_cells")
    got = {"idx": idx.get("idx"), "out": out.get("out"), "bq_idx": idx2.get("ball_query idx"), "cnt": cnt.get("cnt")}
    for name, b in (("xyz", bx), ("new_xyz", bn)) + ((("feats", bf),) if C else ()):
        assert not _diff("input " + name, b.get(name), case[name])
    return got


def _gate_qg(got, idx, cnt, out):
    bad = _diff("idx", got["idx"], idx) + _diff("ball_query idx", got["bq_idx"], idx) + _diff("cnt", got["cnt"], cnt)
    for p in range(out.shape[1]):
        bad += _diff("out[plane %d]" % p, got["out"][:, p], out[:, p])
    return bad


@pytest.mark.parametrize("route,N,S,C,M,bq_cells", QG_CASES)
def test_query_and_group_bit_exact_on_every_route(route, N, S, C, M, bq_cells):
    assert _route(N, S, C, bq_cells) == route and _hip().get_option("bq_cells") == 1
    case = _qg_case(N, S, C, M)
    got = _run_qg(N, S, C, M, bq_cells)
    bad = _gate_qg(got, case["idx"], case["cnt"], case["out"])
    assert not bad, _report(bad)


def test_query_gate_rejects_the_neighbouring_centroid():
    """negative control (no kernel is altered): a reference that recentres the last centroid of the partial last quad (M = 515:
    centroids 512, 513, 514) on centroid M - 2 fails, on the coordinate planes of that centroid only"""
    N, S, C, M = 2501, 17, 4, 515
    assert _route(N, S, C, 1) == "cells64.pipe" and M % 4 == 3
    case = _qg_case(N, S, C, M)
    got = _run_qg(N, S, C, M, 1)
    assert not _gate_qg(got, case["idx"], case["cnt"], case["out"])
    out = case["out"].copy()
    for b in range(case["B"]):
        out[b, :3, M - 1] = (case["xyz"][b][case["idx"][b, M - 1]] - case["new_xyz"][b, M - 2]).T
    bad = _gate_qg(got, case["idx"], case["cnt"], out)
    assert bad, "the gate accepted a reference recentred on the neighbouring centroid"
    assert {m.split(":")[0] for m, _ in bad} == {"out[plane 0]", "out[plane 1]", "out[plane 2]"}
    for _, mask in bad:
        assert mask[:, M - 1].all() and not mask[:, :M - 1].any()


def test_query_gate_rejects_a_repeated_feature_plane():
    """negative control: a reference whose feature plane 4 -- the first one past the pipelined write-out's BQC_CPIPE = 4 channels --
    is a copy of plane 3 fails, on that plane only"""
    N, S, C, M = 1025, 17, 5, 3
    assert _route(N, S, C, 1) == "cells64.plain"
    case = _qg_case(N, S, C, M)
    got = _run_qg(N, S, C, M, 1)
    assert not _gate_qg(got, case["idx"], case["cnt"], case["out"])
    out = case["out"].copy()
    out[:, 3 + 4] = out[:, 3 + 3]
    bad = _gate_qg(got, case["idx"], case["cnt"], out)
    assert [m.split(":")[0] for m, _ in bad] == ["out[plane 7]"], _report(bad)


# ----------------------------------------------------------------------------- b. group and gather, forward
# (B, C, N, M, S): M * S % 4 == 0 takes the 16-byte kernel, anything else the scalar one; C = 1; N = 1 (every index 0); M * S = 4 (one
# thread covers a whole (b, c) row: a 4-group straying across a row boundary shows); gather (S = 1) with M % 4 in {3, 0, 1, 1, 1}
GROUP_SHAPES = [(3, 7, 257, 19, 12), (2, 1, 1, 4, 1), (2, 3, 64, 1, 4), (2, 5, 33, 5, 3), (1, 2, 1000, 257, 1)]


def _points(rng, B, C, N):
    pts = rng.normal(size=(B, C, N)).astype(f32)
    special = np.array([-0.0, 1e-40, np.inf, -3.4028235e38], f32)                 # copies keep sign of zero, denormals, inf
    k = min(N, 4)
    pts[0, 0, :k] = special[:k]
    return pts


def _indices(rng, B, N, *shape):
    idx = rng.integers(0, N, size=(B,) + shape).astype(np.int32)
    flat = idx.reshape(B, -1)
    flat[:, 0], flat[:, -1] = N - 1, 0                                            # both ends of the point axis
    return idx


@pytest.mark.parametrize("B,C,N,M,S", GROUP_SHAPES)
def test_group_and_gather_forward_bit_exact(B, C, N, M, S):
    hip = _hip()
    rng = np.random.default_rng(7 * N + M)
    pts = _points(rng, B, C, N)
    idx, gi = _indices(rng, B, N, M, S), _indices(rng, B, N, M)
    bp, bi, bg = Buf(pts), Buf(idx), Buf(gi)
    out, gat = _out_f(B, C, M, S), _out_f(B, C, M)
    hip.call("gad_group_points", bp.ptr, bi.ptr, B, C, N, M, S, out.ptr)
    hip.call("gad_gather_points", bp.ptr, bg.ptr, B, C, N, M, gat.ptr)
    bad = _diff("group_points", out.get("out"), R.group_points(pts, idx))
    bad += _diff("gather_points", gat.get("out"), R.gather_points(pts, gi))
    bad += _diff("points", bp.get("points"), pts) + _diff("idx", bi.get("idx"), idx) + _diff("gather idx", bg.get("idx"), gi)
    assert not bad, _report(bad)


# ----------------------------------------------------------------------------- c. group and gather, atomic gradient
def _skewed(rng, B, N, MS):
    """at most three destinations per sample take MS / 4 entries each, capped at 512; the rest spread over the other points"""
    idx = np.empty((B, MS), np.int32)
    for b in range(B):
        hot = rng.choice(N, size=min(3, N), replace=False)
        cold = np.setdiff1d(np.arange(N), hot)
        a = np.repeat(hot, min(512, max(1, MS // 4)))[:MS]
        rest = rng.choice(cold if cold.size else hot, size=MS - a.size, replace=True)
        idx[b] = rng.permutation(np.concatenate([a, rest]))
    return idx


def _index_set(kind, rng, B, N, MS):
    """(B, MS) int32 in [0, N)"""
    if kind == "perm":                                    # distinct where MS <= N: every destination takes one entry at most
        return np.stack([rng.permutation(max(N, MS))[:MS] % N for _ in range(B)]).astype(np.int32)
    if kind == "rand":
        return rng.integers(0, N, size=(B, MS)).astype(np.int32)
    if kind == "tiny":                                    # every index in {0, 1, 2}: MS / 3 entries per destination
        return rng.integers(0, min(N, 3), size=(B, MS)).astype(np.int32)
    assert kind == "skew"
    return _skewed(rng, B, N, MS)


def _run_grad(entry, go, idx, N):
    """gad_group_points_grad on go (B,C,M,S), idx (B,M,S), or gad_gather_points_grad on go (B,C,M), idx (B,M)"""
    hip = _hip()
    B, C, M = go.shape[:3]
    bg, bi, gp = Buf(go), Buf(idx), _out_f(B, C, N)
    if entry == "gad_group_points_grad":
        hip.call(entry, bg.ptr, bi.ptr, B, C, N, M, go.shape[3], gp.ptr)
    else:
        hip.call(entry, bg.ptr, bi.ptr, B, C, N, M, gp.ptr)
    got = gp.get("grad_points")
    assert not _diff("grad_out", bg.get("grad_out"), go) and not _diff("idx", bi.get("idx"), idx)
    return got


def _gate_atomic(got, ref, n, mag):
    """got (B,C,N) float32 against the float64 sum `ref`, per destination by its number of entries n (B,N): n = 0: zero; n = 1: the
    term; n = 2: float32(a + b) -- one rounding either way round, and a + b is exact in float64 --, all bit for bit; n >= 3:
    |got - ref| <= (n + 2) * 2^-24 * sum |terms|, which holds for a float32 sum of n terms in any order.  [] or [(message, mask)]"""
    assert got.dtype == f32 and got.shape == ref.shape
    nn = np.broadcast_to(n[:, None, :], ref.shape)
    bad = []
    nan = np.isnan(got)
    if nan.any():
        bad.append(("%d elements are NaN" % int(nan.sum()), nan))
    zero = (nn == 0) & (got != 0)
    if zero.any():
        bad.append(("%d destinations without an entry are not 0" % int(zero.sum()), zero))
    few = ((nn == 1) | (nn == 2)) & (_bits(got) != _bits(ref.astype(f32)))
    if few.any():
        bad.append(("%d destinations with one or two entries differ bitwise" % int(few.sum()), few))
    err, bound = np.abs(got.astype(np.float64) - ref), (nn + 2) * 2.0 ** -24 * mag
    many = (nn >= 3) & ~(err <= bound)
    if many.any():
        i = np.unravel_index(int(np.argmax(np.where(many, err / np.maximum(bound, 1e-300), 0))), many.shape)
        bad.append(("%d destinations with n >= 3 entries beyond the bound; worst at %s: n %d err %.3e bound %.3e" % (
            int(many.sum()), i, nn[i], err[i], bound[i]), many))
    return bad


@pytest.mark.parametrize("kind", ("perm", "half", "skew"))
@pytest.mark.parametrize("B,C,N,M,S", GROUP_SHAPES + [(2, 64, 512, 64, 32)])
def test_group_and_gather_grad_atomic_within_derived_bound(B, C, N, M, S, kind):
    """default mode: a clearing pass, then one float32 atomic add per entry.  perm: N = M * S, a permutation -- every destination one
    entry; half: random over N = M * S / 2 points -- a mix of 0, 1, 2 and more; skew: the shape's own N, a few destinations with up
    to 512 entries and no more, so that a dropped term (about sum |terms| / n) stays two orders of magnitude above the bound"""
    assert _hip().get_option("deterministic") == 0
    rng = np.random.default_rng(11 * N + 3 * M + len(kind))
    seen, peak = set(), {}
    for entry, E, shape in (("gad_group_points_grad", M * S, (M, S)), ("gad_gather_points_grad", M, (M,))):
        n_pts = {"perm": E, "half": max(1, E // 2), "skew": N}[kind]
        idx = _index_set("rand" if kind == "half" else kind, rng, B, n_pts, E).reshape((B,) + shape)
        go = rng.normal(size=(B, C) + shape).astype(f32)
        ref, n, mag = R.group_points_grad(go, idx, n_pts)
        assert n.max() <= 512 and (kind != "perm" or (n == 1).all())
        seen |= set(np.minimum(n, 3).ravel().tolist())
        peak[entry] = int(n.max())
        bad = _gate_atomic(_run_grad(entry, go, idx, n_pts), ref, n, mag)
        assert not bad, entry + ":\n" + _report(bad)
    if kind == "half" and M * S >= 200:
        assert seen == {0, 1, 2, 3}
    if kind == "skew" and M * S >= 2048:
        assert peak["gad_group_points_grad"] == 512


def _hot_case():
    rng = np.random.default_rng(99)
    B, C, N, M, S = 2, 64, 512, 64, 32
    idx = _index_set("skew", rng, B, N, M * S).reshape(B, M, S)
    go = rng.normal(size=(B, C, M, S)).astype(f32)
    return go, idx, N


def test_atomic_gate_rejects_a_dropped_entry():
    """negative control: the float64 reference with one of the 512 entries of one destination left out fails, at that destination
    only (a channel whose dropped term happens to be tiny may pass: most do not)"""
    go, idx, N = _hot_case()
    ref, n, mag = R.group_points_grad(go, idx, N)
    got = _run_grad("gad_group_points_grad", go, idx, N)
    assert not _gate_atomic(got, ref, n, mag)
    h = int(np.argmax(n[0]))
    assert n[0, h] == 512
    q = int(np.flatnonzero(idx[0].reshape(-1) == h)[0])
    altered = ref.copy()
    altered[0, :, h] -= go[0].reshape(go.shape[1], -1)[:, q].astype(np.float64)
    bad = _gate_atomic(got, altered, n, mag)
    assert len(bad) == 1 and "beyond the bound" in bad[0][0], _report(bad)
    mask = bad[0][1]
    assert mask[0, :, h].sum() > mask.shape[1] // 2 and mask.sum() == mask[0, :, h].sum()


# ----------------------------------------------------------------------------- d. group and gather, deterministic gradient
# (B, C, N, M, S): B * C <= 6; N around the 256 destinations one pass of a thread covers and around the LDS tile of 8192, up to a
# third tile; M * S in {5, 256, 257, 700}: under, at and over one staged chunk of 256 entries, and a ragged third chunk
DET_SHAPES = [(2, 3, 1, 5, 1), (1, 6, 255, 16, 16), (3, 2, 256, 257, 1), (2, 2, 257, 35, 20), (1, 3, GPG_NT, 35, 20),
              (2, 1, GPG_NT + 1, 257, 1), (1, 2, 2 * GPG_NT + 3, 16, 16), (2, 2, 2 * GPG_NT + 3, 35, 20)]


def _det_case(B, C, N, M, S, kind):
    rng = np.random.default_rng(13 * N + M * S + len(kind) + ord(kind[0]))
    MS = M * S
    idx = _index_set(kind, rng, B, N, MS)
    edges = [v for v in (GPG_NT - 1, GPG_NT, 2 * GPG_NT - 1, 2 * GPG_NT) if v < N]
    if edges:                                             # both sides of every tile boundary, three entries each
        slots = rng.choice(MS, size=3 * len(edges), replace=False)
        idx[:, slots] = np.repeat(edges, 3)
    go = (rng.normal(size=(B, C, M, S)) * 10.0 ** rng.integers(-3, 4, size=(B, C, M, S))).astype(f32)
    return go, idx.reshape(B, M, S)


def _run_det(entry, go, idx, N):
    hip = _hip()
    try:
        hip.set_option("deterministic", 1)
        return _run_grad(entry, go, idx, N)
    finally:
        _restore("deterministic")


@pytest.mark.parametrize("kind", ("perm", "rand", "skew", "tiny"))
@pytest.mark.parametrize("B,C,N,M,S", DET_SHAPES + [(1, 2, 257, 96, 64)])
def test_group_grad_deterministic_is_the_ordered_sum(B, C, N, M, S, kind):
    """option "deterministic": every destination is written by one thread that adds its entries in ascending q = m * S + s, from +0,
    in float32 -- bit-equal to np.add.at on a float32 array; the NaN the buffer starts with must be gone everywhere (this mode has
    no clearing pass).  The terms span six decades, so another order gives other bits.  (1, 2, 257, 96, 64) with `tiny`: two
    thousand entries per destination."""
    go, idx = _det_case(B, C, N, M, S, kind)
    got = _run_det("gad_group_points_grad", go, idx, N)
    assert _hip().get_option("deterministic") == 0
    bad = _diff("grad_points", got, R.group_points_grad_ordered(go, idx, N))
    if S == 1:                                            # the gather entry point is the same launch with S = 1
        got_g = _run_det("gad_gather_points_grad", go[..., 0], idx[..., 0], N)
        bad += _diff("gather grad_points", got_g, R.group_points_grad_ordered(go, idx, N))
    assert not bad, _report(bad)


def test_deterministic_gate_rejects_the_descending_order():
    """negative control: the same accumulation taken in descending q fails, and only where a destination takes three entries or more
    (two float32 terms add to the same bits either way round)"""
    B, C, N, M, S = 2, 2, 257, 35, 20
    go, idx = _det_case(B, C, N, M, S, "tiny")
    got = _run_det("gad_group_points_grad", go, idx, N)
    assert not _diff("grad_points", got, R.group_points_grad_ordered(go, idx, N))
    descending = R.group_points_grad_ordered(go[:, :, ::-1, ::-1], idx[:, ::-1, ::-1], N)
    bad = _diff("grad_points", got, descending)
    assert len(bad) == 1 and "differ bitwise" in bad[0][0], _report(bad)
    n = R.group_points_grad(go, idx, N)[1]
    assert (np.broadcast_to(n[:, None, :], got.shape)[bad[0][1]] >= 3).all()


# ----------------------------------------------------------------------------- e. gad_prep_points
@pytest.mark.parametrize("B,C4,NP,skip", [(1, 3, 1, 0), (2, 4, 300, 0), (3, 4, 300, 44), (2, 5, 257, 1), (1, 4, 1024, 1023)])
def test_prep_points_bit_exact(B, C4, NP, skip):
    """point_state (B,C4,NP) channel-major -> xyz (B,N,3) and feat (B*N,4) = [x, y, z, flag], N = NP - skip: copies.  C4 = 3: flag 0;
    C4 = 5: channel 4 is ignored; the skipped leading columns (values 1e6 + ...) and channel 4 (-1e6 - ...) never reach an output"""
    hip = _hip()
    rng = np.random.default_rng(NP + skip)
    ps = rng.normal(size=(B, C4, NP)).astype(f32)
    if C4 > 3:
        ps[:, 3] = rng.integers(0, 2, size=(B, NP))
    ps[0, 0, skip:skip + 3] = np.array([-0.0, 1e-40, -1e-45], f32)[:NP - skip]           # copies keep the sign of zero and denormals
    ps[:, :, :skip] = f32(1e6) + np.arange(B * C4 * skip, dtype=f32).reshape(B, C4, skip)
    if C4 > 4:
        ps[:, 4:] = f32(-1e6) - np.arange(B * (C4 - 4) * NP, dtype=f32).reshape(B, C4 - 4, NP)
    N = NP - skip
    bp, xyz, feat = Buf(ps), _out_f(B, N, 3), _out_f(B * N, 4)
    hip.call("gad_prep_points", bp.ptr, B, C4, NP, skip, xyz.ptr, feat.ptr)
    want_xyz, want_feat = R.prep_points(ps, skip)
    got_xyz, got_feat = xyz.get("xyz"), feat.get("feat")
    bad = _diff("xyz", got_xyz, want_xyz) + _diff("feat", got_feat, want_feat) + _diff("point_state", bp.get("point_state"), ps)
    assert not bad, _report(bad)
    assert not (np.abs(got_xyz) >= 1e6).any() and not (np.abs(got_feat) >= 1e6).any()
    if C4 == 3:
        assert (_bits(got_feat[:, 3]) == 0).all()


# ----------------------------------------------------------------------------- f. row builders
# (G, M, S): B = G / M samples where M divides G; (5, 2, .) does not (b = g / M all the same).  Nsrc = 2 M + 5 != M
ROWS_CASES = [(1, 1, 1), (1, 1, 130), (3, 1, 64), (3, 3, 130), (5, 5, 64), (5, 1, 1), (5, 2, 130), (4099, 1, 64), (4099, 4099, 130),
              (4099, 4099, 1)]


def _rows_case(G, M, S):
    """synthetic idx / cnt, so the edges are exact: counts drawn from {0, 1, 63, 64, 65, S} (those <= S), several empty balls, the
    last ball full"""
    rng = np.random.default_rng(17 * G + 5 * M + S)
    Nsrc = 2 * M + 5
    allowed = sorted({v for v in (0, 1, 63, 64, 65, S) if v <= S})
    cnt = rng.choice(allowed, size=G).astype(np.int32)
    cnt[-1] = S if G > 1 or S > 1 else 0
    if G >= 3:                                            # small G: the edges by hand -- empty, the longest short ball, ..., full
        cnt[0], cnt[1] = 0, max(v for v in allowed if v < S)
    if G >= 5:
        cnt[2], cnt[G - 2] = min(1, S), 0
    idx = rng.integers(0, Nsrc, size=(G, S)).astype(np.int32)
    return idx, cnt, Nsrc


def _run_rows(idx, cnt, M, Nsrc, S):
    hip = _hip()
    G, cap = cnt.size, cnt.size * S
    bi, bc = Buf(idx), Buf(cnt)
    o = {"off": _out_i(G + 1), "row_pt": _out_i(cap), "row_grp": _out_i(cap), "row_w": _out_f(cap), "n": _out_i(1)}
    hip.call("gad_rows_from_ball_query", bi.ptr, bc.ptr, G, M, Nsrc, S, o["off"].ptr, o["row_pt"].ptr, o["row_grp"].ptr,
             o["row_w"].ptr, o["n"].ptr)
    got = {k: b.get(k) for k, b in o.items()}
    assert not _diff("idx", bi.get("idx"), idx) and not _diff("cnt", bc.get("cnt"), cnt)
    return got


def _gate_rows(got, want):
    """off, n_rows and the first n_rows entries of row_pt / row_grp / row_w bit for bit; everything past n_rows untouched"""
    off, pt, grp, w, n = want
    bad = _diff("off", got["off"], off) + _diff("n_rows", got["n"], np.array([n], np.int32))
    for name, ref in (("row_pt", pt), ("row_grp", grp), ("row_w", w)):
        bad += _diff(name, got[name][:n], ref)
        past = ~_untouched(got[name][n:])
        if past.any():
            bad.append(("%s: %d entries past n_rows were written" % (name, int(past.sum())), past))
    return bad


@pytest.mark.parametrize("G,M,S", ROWS_CASES)
def test_rows_from_ball_query_bit_exact(G, M, S):
    idx, cnt, Nsrc = _rows_case(G, M, S)
    assert G < 3 or (cnt[0] == 0 and cnt[-1] == S and (G < 5 or (cnt == 0).sum() >= 2))
    got = _run_rows(idx, cnt, M, Nsrc, S)
    bad = _gate_rows(got, R.rows_from_ball_query(idx, cnt, M, Nsrc, S))
    assert not bad, _report(bad)


def test_rows_gate_rejects_a_first_row_of_weight_one():
    """negative control: a reference in which the first row of a short ball (1 < cnt < S) weighs 1 instead of S - cnt + 1 fails, on
    row_w only"""
    G, M, S = 5, 5, 64
    idx, cnt, Nsrc = _rows_case(G, M, S)
    cnt[1] = 63
    got = _run_rows(idx, cnt, M, Nsrc, S)
    off, pt, grp, w, n = R.rows_from_ball_query(idx, cnt, M, Nsrc, S)
    assert not _gate_rows(got, (off, pt, grp, w, n))
    altered = w.copy()
    assert altered[off[1]] == 2
    altered[off[1]] = 1
    bad = _gate_rows(got, (off, pt, grp, altered, n))
    assert [m.split(":")[0] for m, _ in bad] == ["row_w"] and bad[0][1].sum() == 1 and bad[0][1][off[1]], _report(bad)


@pytest.mark.parametrize("G,P", [(1, 1), (3, 85), (1, 255), (1, 256), (2, 128), (300, 1), (7, 4096)])
def test_rows_group_all_bit_exact(G, P):
    """G * P on both sides of a 256-thread workgroup boundary; P = 1: `off` has one more entry than there are rows"""
    hip = _hip()
    o = {"off": _out_i(G + 1), "row_pt": _out_i(G * P), "row_grp": _out_i(G * P), "row_w": _out_f(G * P), "n": _out_i(1)}
    hip.call("gad_rows_group_all", G, P, o["off"].ptr, o["row_pt"].ptr, o["row_grp"].ptr, o["row_w"].ptr, o["n"].ptr)
    bad = _gate_rows({k: b.get(k) for k, b in o.items()}, R.rows_group_all(G, P))
    assert not bad, _report(bad)
