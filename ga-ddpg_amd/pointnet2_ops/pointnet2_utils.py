"""pointnet2_ops.pointnet2_utils surface over libgaddpg (include/gaddpg.h section A).

Each function mirrors upstream's autograd.Function of the same name: same argument order, shapes,
dtypes (indices are int32), contiguity / device checks raising RuntimeError, gradients only where
upstream defines them (features of grouping_operation / gather_operation / three_interpolate).

furthest_point_sample takes every shape upstream's does (N up to 4 194 304, npoint > N included): shapes that fit one workgroup's
LDS run gad_furthest_point_sampling, every other shape gad_fps_tiled -- same indices.  The fused set-abstraction path
(sa_function / engine.Geometry, i.e. PointnetSAModule[MSG] with bn=True, use_xyz=True and features) does NOT route: it calls the
LDS kernel and keeps its refusals (N > 16384, npoint > N, 3N + npoint beyond 160 KiB of LDS)."""
import torch
import torch.nn as nn

from .. import hip


def _check(*tensors):
    hip.require_cuda(*tensors)


def fps_fits_one_workgroup(N, M):
    """the shapes gad_furthest_point_sampling accepts (include/gaddpg.h: cloud + exchange slots + picks in 160 KiB of LDS)"""
    return N <= 16384 and M <= N and (((N * 3 + 3) & ~3) + 64 + M) * 4 <= 160 * 1024


def furthest_point_sample(xyz, npoint):
    """xyz (B,N,3) float32 CUDA contiguous -> (B,npoint) int32."""
    _check(xyz)
    if xyz.dtype != torch.float32:
        raise RuntimeError("xyz must be a float tensor")
    B, N, _ = xyz.shape
    M = int(npoint)
    idx = torch.empty(B, M, dtype=torch.int32, device=xyz.device)
    if fps_fits_one_workgroup(N, M):
        hip.call("gad_furthest_point_sampling", xyz, B, N, M, idx, None)
        return idx
    nbytes = hip.lib().gad_fps_tiled_workspace_bytes(B, N, M, 0)
    if nbytes < 0:
        hip.check(int(nbytes), "gad_fps_tiled_workspace_bytes")
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device)
    hip.call("gad_fps_tiled", xyz, B, N, M, 0, idx, None, workspace)
    return idx


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx):
        _check(features, idx)
        B, C, N = features.shape
        M = idx.shape[1]
        out = torch.empty(B, C, M, dtype=torch.float32, device=features.device)
        hip.call("gad_gather_points", features, idx, B, C, N, M, out)
        ctx.save_for_backward(idx)
        ctx.N = N
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        B, C, M = grad_out.shape
        g = torch.empty(B, C, ctx.N, dtype=torch.float32, device=grad_out.device)
        hip.call("gad_gather_points_grad", grad_out, idx, B, C, ctx.N, M, g)
        return g, None


def gather_operation(features, idx):
    return _Gather.apply(features, idx)


def ball_query(radius, nsample, xyz, new_xyz):
    """-> (B,M,nsample) int32."""
    _check(xyz, new_xyz)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    idx = torch.empty(B, M, nsample, dtype=torch.int32, device=xyz.device)
    hip.call("gad_ball_query", new_xyz, xyz, B, N, M, float(radius), int(nsample), idx, None)
    return idx


class _Group(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx):
        _check(features, idx)
        B, C, N = features.shape
        _, M, S = idx.shape
        out = torch.empty(B, C, M, S, dtype=torch.float32, device=features.device)
        hip.call("gad_group_points", features, idx, B, C, N, M, S, out)
        ctx.save_for_backward(idx)
        ctx.N = N
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        B, C, M, S = grad_out.shape
        g = torch.empty(B, C, ctx.N, dtype=torch.float32, device=grad_out.device)
        hip.call("gad_group_points_grad", grad_out, idx, B, C, ctx.N, M, S, g)
        return g, None


def grouping_operation(features, idx):
    return _Group.apply(features, idx)


def three_nn(unknown, known):
    """unknown (B,n,3), known (B,m,3) float32 CUDA contiguous -> (dist (B,n,3) float32, idx (B,n,3) int32): the three nearest
    known points of every query point, nearest first, ties to the lower index; dist is the Euclidean distance (the square root of
    what gad_three_nn returns).  Neither output is differentiable."""
    _check(unknown, known)
    if unknown.dtype != torch.float32 or known.dtype != torch.float32:
        raise RuntimeError("unknown and known must be float tensors")
    B, n, _ = unknown.shape
    m = known.shape[1]
    dist2 = torch.empty(B, n, 3, dtype=torch.float32, device=unknown.device)
    idx = torch.empty(B, n, 3, dtype=torch.int32, device=unknown.device)
    hip.call("gad_three_nn", unknown.detach(), known.detach(), B, n, m, dist2, idx)
    return torch.sqrt(dist2), idx


class _ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        _check(features, idx, weight)
        if features.dtype != torch.float32 or weight.dtype != torch.float32:
            raise RuntimeError("features and weight must be float tensors")
        if idx.dtype != torch.int32:
            raise RuntimeError("idx must be an int tensor")
        B, C, m = features.shape
        n = idx.shape[1]
        out = torch.empty(B, C, n, dtype=torch.float32, device=features.device)
        hip.call("gad_three_interpolate", features, idx, weight, B, C, m, n, out)
        ctx.save_for_backward(idx, weight)
        ctx.m = m
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        B, C, n = grad_out.shape
        g = torch.empty(B, C, ctx.m, dtype=torch.float32, device=grad_out.device)
        hip.call("gad_three_interpolate_grad", grad_out, idx, weight, B, C, n, ctx.m, g)
        return g, None, None


def three_interpolate(features, idx, weight):
    """features (B,C,m), idx (B,n,3) int32, weight (B,n,3) -> (B,C,n): the weighted sum of three feature columns per point.
    The gradient flows to `features` only."""
    return _ThreeInterpolate.apply(features, idx, weight)


def query_and_group(radius, nsample, xyz, new_xyz, features):
    """fused QueryAndGroup(use_xyz=True) forward (no autograd): -> (idx, (B,3+C,M,S))."""
    _check(xyz, new_xyz, features)
    B, N, _ = xyz.shape
    M = new_xyz.shape[1]
    C = features.shape[1]
    idx = torch.empty(B, M, nsample, dtype=torch.int32, device=xyz.device)
    out = torch.empty(B, 3 + C, M, nsample, dtype=torch.float32, device=xyz.device)
    hip.call("gad_query_and_group", new_xyz, xyz, features, B, C, N, M, float(radius), int(nsample), idx, out)
    return idx, out


class QueryAndGroup(nn.Module):
    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None):
        idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
        grouped_xyz = grouping_operation(xyz.transpose(1, 2).contiguous(), idx)
        grouped_xyz = grouped_xyz - new_xyz.transpose(1, 2).unsqueeze(-1)
        if features is None:
            return grouped_xyz
        grouped = grouping_operation(features, idx)
        return torch.cat([grouped_xyz, grouped], dim=1) if self.use_xyz else grouped


class GroupAll(nn.Module):
    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            return grouped_xyz
        grouped = features.unsqueeze(2)
        return torch.cat([grouped_xyz, grouped], dim=1) if self.use_xyz else grouped
