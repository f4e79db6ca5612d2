"""pointnet2_ops.pointnet2_utils surface over libgaddpg (include/gaddpg.h section A).

Each function mirrors upstream's autograd.Function of the same name: same argument order, shapes,
dtypes (indices are int32), contiguity / device checks raising RuntimeError, gradients only where
upstream defines them (features of grouping_operation / gather_operation / three_interpolate).

furthest_point_sample takes every shape upstream's does (N up to 4 194 304, npoint > N included): shapes that fit one workgroup's
LDS run gad_furthest_point_sampling, every other shape gad_fps_tiled -- same indices.  ball_query sends clouds of 262 144 points
and more (ball_query_uses_grid: the sizes at which it was measured faster, profiles/ball_query_grid.txt) to gad_ball_query_grid, a
uniform grid in global memory, and every other shape to gad_ball_query -- same indices; library option "bq_grid" = 0 keeps the scan
for all of them, 2 sends every cloud beyond 4096 points to the grid.  The fused set-abstraction modules (sa_function, i.e.
PointnetSAModule[MSG] with bn=True, use_xyz=True and features) route by the same two predicates.  three_nn -- and with it
PointnetFPModule -- sends clouds of 8192 known points and more (three_nn_uses_grid: the sizes at which the grid was measured
faster, profiles/three_nn_grid.txt) to gad_three_nn_grid, which searches the same grid ring by ring instead of evaluating all n * m
distances, and every other shape to gad_three_nn -- same distances and indices; library option "tnn_grid" = 0 keeps gad_three_nn
for all of them, 2 sends every shape with more than 1024 known points to the grid.  What is left of the LDS
kernels' refusals (N > 16384, npoint > N, 3N + npoint beyond 160 KiB of LDS) is engine.Geometry: the update step and
feature_forward call gad_furthest_point_sampling directly."""
import torch
import torch.nn as nn

from .. import hip


def _check(*tensors):
    hip.require_cuda(*tensors)


def fps_fits_one_workgroup(N, M):
    """the shapes gad_furthest_point_sampling accepts (include/gaddpg.h: cloud + exchange slots + picks in 160 KiB of LDS)"""
    return N <= 16384 and M <= N and (((N * 3 + 3) & ~3) + 64 + M) * 4 <= 160 * 1024


BQ_LDS_MAX_N = 4096       # gad_ball_query keeps clouds up to here in one workgroup's LDS: never sent to the grid
# smallest cloud sent to gad_ball_query_grid by default.  profiles/ball_query_grid.txt (MI355X, B = 1, box-surface clouds): with
# balls of about 16 points -- fewer than nsample, the first-stage regime, where the scan walks the whole cloud -- the grid takes
# 0.11-0.37 of the scan's time at N = 4097 / 8192 (it loses: building it costs 140-200 us), 0.85-0.92 at N = 65536 with up to 4096
# centroids, and wins 1.7-4.3 x at N = 262144 and 3.2-6.2 x at N = 1048576 for every centroid count measured (spread of a row < 3 %).
# With balls of about 300 points the scan stops after nsample hits and stays faster at nearly every size: set "bq_grid" = 0 there.
BQ_GRID_MIN_N = 262144


def ball_query_uses_grid(N):
    """the shapes ball_query and the fused set-abstraction path send to gad_ball_query_grid.  Library option "bq_grid": 1 (default)
    = clouds of BQ_GRID_MIN_N points and more, 0 = none, 2 = every cloud beyond the BQ_LDS_MAX_N points of the LDS kernels"""
    mode = hip.get_option("bq_grid")
    if mode == 0 or N <= BQ_LDS_MAX_N:
        return False
    return mode >= 2 or N >= BQ_GRID_MIN_N


TNN_LDS_TILE = 1024       # known points per LDS tile of gad_three_nn: a cloud of one tile is never sent to the grid
# smallest known cloud sent to gad_three_nn_grid by default.  profiles/three_nn_grid.txt (MI355X; B = 1 and 8; n = m / 4, m, 4 m;
# box-surface and uniform-cube clouds with queries of the same distribution, and cube clouds with 70 % of the queries outside the
# box; us per call): building the grid costs about 190 us, gad_three_nn about 90 ns per known point -- at m = 2048 the two tie
# (0.72-1.06), at m = 4096 the grid wins 17 of 18 rows (1.1-1.9 x) and loses one (0.92: B 8, n 16384, queries outside the box), from
# m = 8192 it wins every measured row by far more than the spread of a row (< 3 %): 1.3-3.4 x at 8192, 2.2-6.5 x at 16384,
# 1.9-22 x at 65536, 3.4-38 x at 262144 (n = m = 262144: 19.5 ms -> 0.8 ms).
TNN_GRID_MIN_M = 8192


def three_nn_uses_grid(n, m):
    """the shapes three_nn (hence PointnetFPModule) sends to gad_three_nn_grid.  Library option "tnn_grid": 1 (default) = clouds of
    TNN_GRID_MIN_M known points and more, whatever n; 0 = none; 2 = every shape with more known points than the TNN_LDS_TILE of
    gad_three_nn's kernel"""
    mode = hip.get_option("tnn_grid")
    if mode == 0 or m <= TNN_LDS_TILE:
        return False
    return mode >= 2 or m >= TNN_GRID_MIN_M


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
    hip.call("gad_fps_tiled", xyz, B, N, M, 0, idx, None, hip.workspace("gad_fps_tiled", xyz.device, B, N, M, 0))
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
    if ball_query_uses_grid(N):
        hip.call("gad_ball_query_grid", new_xyz, xyz, B, N, M, float(radius), int(nsample), idx, None,
                 hip.workspace("gad_ball_query_grid", xyz.device, B, N, M, int(nsample)))
        return idx
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
    what gad_three_nn returns).  Shapes for which three_nn_uses_grid holds go to gad_three_nn_grid (a uniform grid over the known
    points, a workspace per call), every other shape to gad_three_nn: same outputs bit for bit.  Neither output is differentiable."""
    _check(unknown, known)
    if unknown.dtype != torch.float32 or known.dtype != torch.float32:
        raise RuntimeError("unknown and known must be float tensors")
    B, n, _ = unknown.shape
    m = known.shape[1]
    dist2 = torch.empty(B, n, 3, dtype=torch.float32, device=unknown.device)
    idx = torch.empty(B, n, 3, dtype=torch.int32, device=unknown.device)
    if three_nn_uses_grid(n, m):
        hip.call("gad_three_nn_grid", unknown.detach(), known.detach(), B, n, m, dist2, idx, None,
                 hip.workspace("gad_three_nn_grid", unknown.device, B, n, m))
        return torch.sqrt(dist2), idx
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
