"""Plain numpy references (no torch, no HIP) for the grouping and row-building kernels of ga-ddpg_amd/csrc/ball_query.hip and group.hip:
gad_ball_query, gad_query_and_group, gad_group_points / gad_gather_points and their gradients (include/gaddpg.h section A),
gad_prep_points, gad_rows_from_ball_query and gad_rows_group_all (section B), written from the semantics the header states.
numpy float32 arrays round every operation individually, which is the kernels' contract (no FMA contraction).
tests/test_group_reference.py pins these functions on the CPU; tests/test_gpu_group_ops.py holds the kernels to them."""
import numpy as np

f32 = np.float32


def sqdist32(centres, points):
    """(M,3), (N,3) float32 -> (M,N) float32: d2 = ((dx*dx) + (dy*dy)) + (dz*dz), each operation rounded"""
    centres, points = np.asarray(centres, f32), np.asarray(points, f32)
    d = centres[:, None, :] - points[None, :, :]
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def ball_query(new_xyz, xyz, radius, nsample):
    """new_xyz (B,M,3), xyz (B,N,3) -> (idx (B,M,nsample) int32, cnt (B,M) int32): the first nsample points, by ascending
    index, with d2 < float32(radius) * float32(radius) (strict); the remaining slots repeat the first hit; an empty ball is
    all zeros with cnt 0.  cnt = min(hits, nsample)."""
    new_xyz, xyz = np.asarray(new_xyz, f32), np.asarray(xyz, f32)
    B, M, _ = new_xyz.shape
    r2 = f32(radius) * f32(radius)
    idx = np.zeros((B, M, nsample), np.int32)
    cnt = np.zeros((B, M), np.int32)
    for b in range(B):
        hit = sqdist32(new_xyz[b], xyz[b]) < r2
        rank = np.cumsum(hit, axis=1) - 1                              # slot of a hit among its centroid's hits
        mm, kk = np.nonzero(hit)                                       # row-major: ascending k inside a centroid
        slot = rank[mm, kk]
        keep = slot < nsample
        total = hit.sum(axis=1)
        cnt[b] = np.minimum(total, nsample)
        first = np.where(total > 0, np.argmax(hit, axis=1), 0)
        idx[b] = first[:, None]
        idx[b][mm[keep], slot[keep]] = kk[keep]
    return idx, cnt


def query_and_group(new_xyz, xyz, features, radius, nsample):
    """-> (idx (B,M,S) int32, out (B,3+C,M,S) float32): planes 0..2 = float32(xyz[idx] - centre), one rounded subtraction;
    planes 3.. = features[:, :, idx], copied.  features (B,C,N) or None (C = 0)."""
    new_xyz, xyz = np.asarray(new_xyz, f32), np.asarray(xyz, f32)
    idx, _ = ball_query(new_xyz, xyz, radius, nsample)
    B, M, S = idx.shape
    C = 0 if features is None else features.shape[1]
    out = np.empty((B, 3 + C, M, S), f32)
    for b in range(B):
        rel = xyz[b][idx[b]] - new_xyz[b][:, None, :]                  # (M,S,3)
        out[b, :3] = rel.transpose(2, 0, 1)
    if C:
        out[:, 3:] = group_points(features, idx)
    return idx, out


def group_points(points, idx):
    """points (B,C,N), idx (B,M,S) -> (B,C,M,S): out[b,c,m,s] = points[b,c,idx[b,m,s]], dtype kept"""
    points = np.asarray(points)
    B, C, N = points.shape
    out = np.empty((B, C) + idx.shape[1:], points.dtype)
    for b in range(B):
        out[b] = points[b][:, idx[b]]
    return out


def gather_points(points, idx):
    """points (B,C,N), idx (B,M) -> (B,C,M)"""
    return group_points(points, np.asarray(idx)[:, :, None])[..., 0]


def group_points_grad(go, idx, N):
    """go (B,C,M,S) [or (B,C,M) with idx (B,M): the gather gradient] -> (grad (B,C,N) float64: the sum of the entries that land
    on each destination -- float32 terms, so every partial sum of a few thousand of them is exact to ~2^-53 relative --,
    n (B,N) int64: how many entries land there, mag (B,C,N) float64: the sum of their absolute values)"""
    go = np.asarray(go, np.float64)
    B, C = go.shape[:2]
    flat = np.asarray(idx).reshape(B, -1)
    terms = go.reshape(B, C, -1)
    grad, mag = np.zeros((B, C, N)), np.zeros((B, C, N))
    n = np.zeros((B, N), np.int64)
    for b in range(B):
        np.add.at(n[b], flat[b], 1)
        for c in range(C):
            np.add.at(grad[b, c], flat[b], terms[b, c])
            np.add.at(mag[b, c], flat[b], np.abs(terms[b, c]))
    return grad, n, mag


def group_points_grad_ordered(go, idx, N):
    """-> (B,C,N) float32: one float32 accumulator per destination, starting at +0, to which the entries q = m * S + s that
    land on it are added one at a time in ascending q, each add rounded (np.add.at applies its entries one by one, in order:
    tests/test_group_reference.py checks that against an explicit loop)"""
    go = np.asarray(go, f32)
    B, C = go.shape[:2]
    flat = np.asarray(idx).reshape(B, -1)
    terms = go.reshape(B, C, -1)
    gp = np.zeros((B, C, N), f32)
    for b in range(B):
        for c in range(C):
            np.add.at(gp[b, c], flat[b], terms[b, c])
    return gp


def prep_points(point_state, skip):
    """point_state (B,C4,NP) channel-major (rows x, y, z, flag, ...) -> (xyz (B,N,3), feat (B*N,4) = [x, y, z, flag]) for
    the N = NP - skip points behind the first `skip` columns; C4 == 3: flag 0; channels past the fourth are ignored"""
    ps = np.asarray(point_state, f32)
    B, C4, NP = ps.shape
    N = NP - skip
    live = ps[:, :, skip:]
    xyz = np.ascontiguousarray(live[:, :3].transpose(0, 2, 1))
    feat = np.zeros((B, N, 4), f32)
    feat[:, :, :3] = xyz
    if C4 > 3:
        feat[:, :, 3] = live[:, 3]
    return xyz, feat.reshape(B * N, 4)


def rows_from_ball_query(idx, cnt, M, Nsrc, nsample):
    """idx (G,nsample) [any shape of that size], cnt (G) -> (off (G+1) int32, row_pt, row_grp int32, row_w float32, n_rows):
    group g = b * M + m keeps its max(cnt, 1) leading slots as rows, in slot order; row_pt = b * Nsrc + idx, row_grp = g,
    row_w = 1 except the first row of a group, which also stands for the nsample - max(cnt, 1) padded copies.  A group with
    cnt 0 is one row (idx slot 0) of weight nsample."""
    cnt = np.asarray(cnt).reshape(-1)
    G = cnt.size
    idx = np.asarray(idx).reshape(G, nsample)
    n = np.maximum(cnt, 1).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n)])
    n_rows = int(off[-1])
    row_grp = np.repeat(np.arange(G), n)
    slot = np.arange(n_rows) - off[row_grp]
    row_pt = (row_grp // M) * Nsrc + idx[row_grp, slot]
    row_w = np.where(slot == 0, (nsample - n + 1)[row_grp], 1).astype(f32)
    return off.astype(np.int32), row_pt.astype(np.int32), row_grp.astype(np.int32), row_w, n_rows


def rows_group_all(G, P):
    """GroupAll: -> (off (G+1), row_pt (G*P), row_grp (G*P) int32, row_w (G*P) float32, n_rows): every point a row of weight 1,
    P consecutive points per group"""
    q = np.arange(G * P)
    return ((np.arange(G + 1) * P).astype(np.int32), q.astype(np.int32), (q // max(P, 1)).astype(np.int32),
            np.ones(G * P, f32), G * P)
