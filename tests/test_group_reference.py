"""CPU pins of tests/group_reference.py (the yardsticks of tests/test_gpu_group_ops.py): the ball query, the group / gather operators
and their gradients against the C oracle (oracle/pn2_ref.c), the ordered float32 accumulation against an explicit loop, the row
builders against cases written out by hand.  No GPU: nothing is launched."""
import numpy as np
import pytest

from tests import group_reference as G

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _cloud_with_edges(rng, B, N, M, r, S):
    """uniform clouds whose centroids are picked points, plus: (0, 0) an empty ball, (B-1, M-1) a ball with more than S points,
    (0, 1) a centroid with a point exactly on r^2"""
    xyz = rng.random((B, N, 3)).astype(f32)
    pick = np.stack([rng.choice(N, size=M, replace=False) for _ in range(B)])
    new_xyz = np.take_along_axis(xyz, pick[..., None], 1).copy()
    new_xyz[0, 0] += f32(10.0)
    crowd = rng.choice(N, size=S + 3, replace=False)
    centre = f32(0.5) + (rng.random(3).astype(f32) - f32(0.5)) * f32(0.2)
    xyz[B - 1, crowd] = centre + (rng.random((S + 3, 3)).astype(f32) - f32(0.5)) * f32(r / 2)
    new_xyz[B - 1, M - 1] = xyz[B - 1, crowd[0]]
    new_xyz[0, 1] = (0.5, 0.5, 0.5)
    xyz[0, 3] = (f32(0.5) + f32(r), 0.5, 0.5)
    return xyz, new_xyz


@pytest.mark.parametrize("B,N,M,r,S", [(2, 300, 9, 0.25, 16), (3, 1025, 5, 0.125, 64), (1, 64, 3, 0.5, 1), (2, 97, 4, 0.25, 7)])
def test_ball_query_matches_the_c_oracle(B, N, M, r, S):
    from oracle import cref
    rng = np.random.default_rng(N + S)
    xyz, new_xyz = _cloud_with_edges(rng, B, N, M, r, S)
    idx, cnt = G.ball_query(new_xyz, xyz, r, S)
    want, wcnt = cref.ball_query(new_xyz, xyz, r, S, return_count=True)
    assert idx.dtype == np.int32 and cnt.dtype == np.int32
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(cnt, wcnt)
    assert cnt[0, 0] == 0 and (idx[0, 0] == 0).all()                             # the empty ball
    d2 = G.sqdist32(new_xyz[B - 1, M - 1:], xyz[B - 1])[0]
    assert (d2 < f32(r) * f32(r)).sum() > S and cnt[B - 1, M - 1] == S           # the overflowing ball keeps the first S
    np.testing.assert_array_equal(idx[B - 1, M - 1], np.flatnonzero(d2 < f32(r) * f32(r))[:S])
    # the point exactly on r^2 is not a hit (strict <); one float closer it is
    assert G.sqdist32(new_xyz[0, 1:2], xyz[0, 3:4])[0, 0] == f32(r) * f32(r)
    assert 3 not in idx[0, 1]
    xyz2 = xyz.copy()
    xyz2[0, 3, 0] = np.nextafter(xyz[0, 3, 0], f32(0))
    idx2, _ = G.ball_query(new_xyz, xyz2, r, S)
    hits = np.flatnonzero(G.sqdist32(new_xyz[0, 1:2], xyz2[0])[0] < f32(r) * f32(r))
    assert 3 in hits and (3 in idx2[0, 1]) == (3 in hits[:S])
    np.testing.assert_array_equal(idx2, cref.ball_query(new_xyz, xyz2, r, S))


def test_sqdist_is_the_pinned_expression():
    """((dx*dx) + (dy*dy)) + (dz*dz) with every operation rounded: equal to the scalar float32 evaluation, and on some of these
    points different from the float64 value rounded once"""
    rng = np.random.default_rng(1)
    c, p = rng.random((4, 3)).astype(f32), rng.random((200, 3)).astype(f32)
    got = G.sqdist32(c, p)
    differs = 0
    for i in range(4):
        for k in range(200):
            dx, dy, dz = (f32(c[i, a] - p[k, a]) for a in range(3))
            want = f32(f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz))
            assert got[i, k] == want
            differs += f32(((c[i].astype(np.float64) - p[k].astype(np.float64)) ** 2).sum()) != want
    assert differs > 0


def test_query_and_group_planes():
    rng = np.random.default_rng(2)
    B, N, M, r, S, C = 2, 200, 6, 0.25, 8, 3
    xyz, new_xyz = _cloud_with_edges(rng, B, N, M, r, S)
    feats = rng.normal(size=(B, C, N)).astype(f32)
    idx, out = G.query_and_group(new_xyz, xyz, feats, r, S)
    assert out.shape == (B, 3 + C, M, S) and out.dtype == f32
    np.testing.assert_array_equal(idx, G.ball_query(new_xyz, xyz, r, S)[0])
    for b in range(B):
        for m in range(M):
            for s in range(S):
                k = idx[b, m, s]
                for a in range(3):
                    assert out[b, a, m, s] == f32(xyz[b, k, a] - new_xyz[b, m, a])
                assert (out[b, 3:, m, s] == feats[b, :, k]).all()
    # the empty ball: point 0 minus the centre
    np.testing.assert_array_equal(out[0, :3, 0, :], np.repeat((xyz[0, 0] - new_xyz[0, 0])[:, None], S, 1))
    i0, o0 = G.query_and_group(new_xyz, xyz, None, r, S)
    assert o0.shape == (B, 3, M, S) and _bits(o0).tobytes() == _bits(out[:, :3]).tobytes()


@pytest.mark.parametrize("B,C,N,M,S", [(3, 7, 257, 19, 12), (2, 1, 1, 4, 1), (2, 3, 64, 1, 4), (2, 5, 33, 5, 3)])
def test_group_and_gather_match_the_c_oracle(B, C, N, M, S):
    from oracle import cref
    rng = np.random.default_rng(N + M)
    pts = rng.normal(size=(B, C, N)).astype(f32)
    idx = rng.integers(0, N, size=(B, M, S)).astype(np.int32)
    out = G.group_points(pts, idx)
    assert out.dtype == f32 and _bits(out).tobytes() == _bits(cref.group_points(pts, idx)).tobytes()
    gi = rng.integers(0, N, size=(B, M)).astype(np.int32)
    g = G.gather_points(pts, gi)
    assert g.shape == (B, C, M) and _bits(g).tobytes() == _bits(cref.gather_points(pts, gi)).tobytes()
    # gradients: the ordered float32 accumulation IS the oracle's loop; the float64 sum lies within the summation bound of it
    go = rng.normal(size=out.shape).astype(f32)
    ordered = G.group_points_grad_ordered(go, idx, N)
    assert _bits(ordered).tobytes() == _bits(cref.group_points_grad(go, idx, N)).tobytes()
    ref, n, mag = G.group_points_grad(go, idx, N)
    assert ref.dtype == np.float64 and n.sum() == B * M * S and (n.sum(1) == M * S).all()
    assert (np.abs(ordered - ref) <= (n[:, None, :] + 2) * 2.0 ** -24 * mag).all()
    assert ((n[:, None, :] > 0) | (ref == 0)).all() and (mag >= np.abs(ref)).all()
    gg = rng.normal(size=g.shape).astype(f32)
    assert _bits(G.group_points_grad_ordered(gg, gi, N)).tobytes() == _bits(cref.gather_points_grad(gg, gi, N)).tobytes()
    ref_g, n_g, _ = G.group_points_grad(gg, gi, N)
    one = np.broadcast_to(n_g[:, None, :] == 1, ref_g.shape)
    assert _bits(ref_g[one].astype(f32)).tobytes() == _bits(cref.gather_points_grad(gg, gi, N)[one]).tobytes()


def test_ordered_grad_is_the_explicit_loop_and_add_at_is_sequential():
    """group_points_grad_ordered against a Python loop over q ascending, on entries whose order matters (a large term between
    small ones); np.add.at on a float32 array gives the same bits, i.e. it applies its entries one at a time, in order, in
    float32 -- which is what lets the GPU tests use it"""
    rng = np.random.default_rng(5)
    B, C, N, M, S = 2, 3, 4, 6, 7
    go = (rng.normal(size=(B, C, M, S)) * 10.0 ** rng.integers(-4, 5, size=(B, C, M, S))).astype(f32)
    idx = rng.integers(0, N, size=(B, M, S)).astype(np.int32)
    want = np.zeros((B, C, N), f32)
    for b in range(B):
        for c in range(C):
            for q in range(M * S):
                k = idx[b].reshape(-1)[q]
                want[b, c, k] = f32(want[b, c, k] + go[b, c].reshape(-1)[q])
    got = G.group_points_grad_ordered(go, idx, N)
    assert got.dtype == f32 and _bits(got).tobytes() == _bits(want).tobytes()
    acc = np.zeros(N, f32)
    np.add.at(acc, idx[0].reshape(-1), go[0, 0].reshape(-1))
    assert _bits(acc).tobytes() == _bits(want[0, 0]).tobytes()
    # the order matters on this input: descending q gives other bits, and so does the float64 sum rounded once
    rev = G.group_points_grad_ordered(go[:, :, ::-1, ::-1], idx[:, ::-1, ::-1], N)
    assert _bits(rev).tobytes() != _bits(want).tobytes()
    assert _bits(G.group_points_grad(go, idx, N)[0].astype(f32)).tobytes() != _bits(want).tobytes()


def test_prep_points_by_hand():
    ps = np.arange(2 * 5 * 4, dtype=f32).reshape(2, 5, 4)                        # (B, C4, NP): value = 20 b + 4 c + j
    xyz, feat = G.prep_points(ps, 1)
    assert xyz.shape == (2, 3, 3) and feat.shape == (6, 4) and xyz.dtype == feat.dtype == f32
    np.testing.assert_array_equal(xyz[0], [[1, 5, 9], [2, 6, 10], [3, 7, 11]])
    np.testing.assert_array_equal(feat[3:], [[21, 25, 29, 33], [22, 26, 30, 34], [23, 27, 31, 35]])
    assert not np.isin(feat, ps[:, :, 0]).any() and not np.isin(feat, ps[:, 4]).any()   # skipped column, fifth channel
    xyz3, feat3 = G.prep_points(ps[:, :3], 0)
    np.testing.assert_array_equal(feat3[:4], [[0, 4, 8, 0], [1, 5, 9, 0], [2, 6, 10, 0], [3, 7, 11, 0]])
    np.testing.assert_array_equal(xyz3.reshape(-1, 3), feat3[:, :3])


def test_rows_from_ball_query_by_hand():
    S, M, Nsrc = 4, 2, 10
    idx = np.array([[3, 5, 3, 3], [0, 0, 0, 0], [7, 8, 9, 6], [2, 2, 2, 2], [4, 1, 4, 4]], np.int32)
    cnt = np.array([2, 0, 4, 1, 2], np.int32)                                    # G = 5: groups 0, 1 sample 0; 2, 3 sample 1; 4 sample 2
    off, pt, grp, w, n = G.rows_from_ball_query(idx, cnt, M, Nsrc, S)
    assert n == 10 and off.dtype == pt.dtype == grp.dtype == np.int32 and w.dtype == f32
    np.testing.assert_array_equal(off, [0, 2, 3, 7, 8, 10])
    np.testing.assert_array_equal(pt, [3, 5, 0, 17, 18, 19, 16, 12, 24, 21])
    np.testing.assert_array_equal(grp, [0, 0, 1, 2, 2, 2, 2, 3, 4, 4])
    np.testing.assert_array_equal(w, [3, 1, 4, 1, 1, 1, 1, 4, 3, 1])
    for g in range(5):
        assert w[off[g]:off[g + 1]].sum() == S                                   # the weights reproduce the padded neighbourhood
    off1, pt1, grp1, w1, n1 = G.rows_from_ball_query(np.array([[6]], np.int32), np.array([0], np.int32), 1, 9, 1)
    assert n1 == 1 and list(off1) == [0, 1] and list(pt1) == [6] and list(grp1) == [0] and list(w1) == [1]


def test_rows_group_all_by_hand():
    off, pt, grp, w, n = G.rows_group_all(2, 3)
    assert n == 6 and list(off) == [0, 3, 6] and list(pt) == [0, 1, 2, 3, 4, 5] and list(grp) == [0, 0, 0, 1, 1, 1]
    assert w.dtype == f32 and (w == 1).all() and off.dtype == pt.dtype == grp.dtype == np.int32
    off, pt, grp, w, n = G.rows_group_all(3, 1)
    assert n == 3 and list(off) == [0, 1, 2, 3] and list(pt) == [0, 1, 2] and list(grp) == [0, 1, 2]
