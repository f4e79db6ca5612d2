"""Plain numpy / CPU torch references for the feature-propagation operators of include/gaddpg.h section A (gad_three_nn,
gad_three_interpolate, gad_three_interpolate_grad) and for pointnet2_modules.PointnetFPModule, written from the semantics the
header states.  numpy float32 arrays round every operation individually, which is the kernels' contract (no FMA contraction).
tests/test_fp_reference.py pins these functions on the CPU; tests/test_gpu_fp_ops.py holds the kernels to them."""
import numpy as np
import torch

f32 = np.float32


def sqdist32(unknown, known):
    """(B,n,3), (B,m,3) float32 -> (B,n,m) float32: d = ((ux-x)*(ux-x) + (uy-y)*(uy-y)) + (uz-z)*(uz-z), each operation rounded"""
    unknown, known = np.asarray(unknown, f32), np.asarray(known, f32)
    d = unknown[:, :, None, :] - known[:, None, :, :]
    sq = d * d
    return (sq[..., 0] + sq[..., 1]) + sq[..., 2]


def three_nn_ref(unknown, known):
    """-> (dist2 (B,n,3) float32, idx (B,n,3) int32): the three known points smallest under (d, index), ascending; a d that is
    NaN or +inf is never selected; unfilled slots (m < 3) hold idx 0 and dist2 +inf"""
    d = sqdist32(unknown, known)
    B, n, m = d.shape
    key = np.where(d < f32(np.inf), d, f32(np.inf))                 # NaN and +inf fail every strict `<` against a slot
    order = np.argsort(key, axis=2, kind="stable")[:, :, :3]         # stable: equal d keep ascending index
    dist2 = np.full((B, n, 3), np.inf, f32)
    idx = np.zeros((B, n, 3), np.int32)
    k = order.shape[2]
    got = np.take_along_axis(key, order, axis=2)
    taken = got < f32(np.inf)
    dist2[:, :, :k] = np.where(taken, got, f32(np.inf))
    idx[:, :, :k] = np.where(taken, order, 0)
    return dist2, idx


def three_interpolate_ref(points, idx, weight):
    """points (B,C,m), idx (B,n,3), weight (B,n,3) -> (B,C,n) float32: (w0*f[i0] + w1*f[i1]) + w2*f[i2], each operation rounded"""
    points, weight = np.asarray(points, f32), np.asarray(weight, f32)
    B, C, m = points.shape
    out = np.empty((B, C, idx.shape[1]), f32)
    for b in range(B):
        a = [weight[b, :, k][None, :] * points[b][:, idx[b, :, k]] for k in range(3)]
        out[b] = (a[0] + a[1]) + a[2]
    return out


def three_interpolate_grad_ref(grad_out, idx, weight, m, dtype=f32):
    """grad_out (B,C,n) -> grad_points (B,C,m): sequential accumulation from 0 of grad_out[b,c,i] * weight[b,i,k] in ascending
    i*3+k order (np.add.at applies its entries one by one, in order).  dtype float32: each product rounded, then each add --
    the deterministic kernel's contract; float64: the products of float32 values are exact."""
    grad_out, weight = np.asarray(grad_out, dtype), np.asarray(weight, dtype)
    B, C, n = grad_out.shape
    gp = np.zeros((B, C, m), dtype)
    for b in range(B):
        terms = (grad_out[b][:, :, None] * weight[b][None, :, :]).reshape(C, n * 3)
        flat = idx[b].reshape(-1)
        for c in range(C):
            np.add.at(gp[b, c], flat, terms[c])
    return gp


def three_interpolate_grad_bound(grad_out, idx, weight, m):
    """per destination: (cnt (B,m) entries landing on it, sum over them of |grad_out * weight| (B,C,m) in float64)"""
    g, w = np.asarray(grad_out, np.float64), np.asarray(weight, np.float64)
    B, C, n = g.shape
    cnt = np.zeros((B, m), np.int64)
    mag = np.zeros((B, C, m))
    for b in range(B):
        flat = idx[b].reshape(-1)
        np.add.at(cnt[b], flat, 1)
        terms = np.abs(g[b][:, :, None] * w[b][None, :, :]).reshape(C, n * 3)
        for c in range(C):
            np.add.at(mag[b, c], flat, terms[c])
    return cnt, mag


def fp_module_ref(mlp, unknown, known, unknow_feats, known_feats, idx, dtype=torch.float64):
    """PointnetFPModule.forward on the CPU in `dtype` with the neighbour indices given (B,n,3): distances to the three indexed
    known points, weights 1/(dist + 1e-8) normalised over the three, interpolation, concatenation with the skip features
    (interpolated first), then `mlp` (a CPU torch module already in `dtype`).  known None: known_feats is expanded to n points.
    Inputs are torch CPU tensors (they may require grad); the result is differentiable."""
    unknown = unknown.to(dtype)
    if known is not None:
        known, feats = known.to(dtype), known_feats.to(dtype)
        B, n, _ = unknown.shape
        ix = idx.long()
        nb = torch.gather(known.unsqueeze(1).expand(B, n, known.shape[1], 3), 2, ix.unsqueeze(-1).expand(B, n, 3, 3))   # (B,n,3,3)
        dist = (unknown.unsqueeze(2) - nb).pow(2).sum(-1).sqrt()
        w = 1.0 / (dist + 1e-8)
        w = w / w.sum(dim=2, keepdim=True)
        C = feats.shape[1]
        f = torch.gather(feats.unsqueeze(2).expand(B, C, n, feats.shape[2]), 3, ix.unsqueeze(1).expand(B, C, n, 3))     # (B,C,n,3)
        x = (f * w.unsqueeze(1)).sum(-1)
    else:
        x = known_feats.to(dtype).expand(known_feats.shape[0], known_feats.shape[1], unknown.shape[1])
    if unknow_feats is not None:
        x = torch.cat([x, unknow_feats.to(dtype)], dim=1)
    return mlp(x.unsqueeze(-1)).squeeze(-1)
