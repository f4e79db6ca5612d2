"""pointnet2_ops.pointnet2_modules surface: PointnetSAModule / PointnetSAModuleMSG / PointnetFPModule with upstream's
module tree (`groupers`, `mlps`; shared MLP = Sequential of [Conv2d 1x1 no-bias, BatchNorm2d, ReLU]
triples) so reference checkpoints' keys `mlps.0.{0,1,3,4,6,7}.*` load unchanged.

forward(xyz (B,N,3), features (B,C,N)) -> (new_xyz (B,npoint,3) | None, (B,C',npoint)) runs the fused
set-abstraction path of libgaddpg (FPS, ball query, de-duplicated rows, FP32-MFMA shared MLP with
train-mode BatchNorm statistics, segment max-pool); see ga_ddpg_amd.sa_function for the autograd
wrapper.  Modules hold ordinary nn.Parameters; the fused update step (core.agent) re-homes them into
flat buffers.

PointnetFPModule (feature propagation, `mlp` = one shared MLP, keys `mlp.{0,1,3,4,...}.*`): three_nn and three_interpolate of
libgaddpg, the shared MLP as torch modules; three_nn takes the grid search of gad_three_nn_grid for the cloud sizes of
pointnet2_utils.three_nn_uses_grid and the exhaustive gad_three_nn otherwise -- same neighbours, so the same output."""
import torch.nn as nn

from . import pointnet2_utils


def build_shared_mlp(mlp_spec, bn=True):
    layers = []
    for cin, cout in zip(mlp_spec[:-1], mlp_spec[1:]):
        layers.append(nn.Conv2d(cin, cout, kernel_size=1, bias=not bn))
        if bn:
            layers.append(nn.BatchNorm2d(cout))
        layers.append(nn.ReLU(True))
    return nn.Sequential(*layers)


class _Scale(nn.Module):
    """one (radius, nsample, shared MLP) scale of a multi-scale module, shaped like a single-scale module for the fused path; it
    shares the parent's grouper and MLP objects (the same nn.Parameters) and is NOT registered in the parent's module tree, so
    the parent's state_dict keeps upstream's keys"""

    def __init__(self, parent, i):
        super().__init__()
        self.npoint, self.radius, self.nsample = parent.npoint, parent.radii[i], parent.nsamples[i]
        self.groupers = nn.ModuleList([parent.groupers[i]])
        self.mlps = nn.ModuleList([parent.mlps[i]])


class PointnetSAModuleMSG(nn.Module):
    """bn=True, use_xyz=True with point features (every module GA-DDPG builds, reference core/networks.py:66-81): the fused
    de-duplicated-row path of libgaddpg.  The other forms upstream's constructor accepts -- bn=False (biased convolutions, no
    BatchNorm), use_xyz=False (the recentred coordinates are not concatenated), features=None -- take upstream's own composition
    (_PointnetSAModuleBase.forward) over this package's operators: furthest_point_sample -> gather_operation -> QueryAndGroup /
    GroupAll (libgaddpg section A kernels, differentiable through their _grad counterparts) -> the shared MLP as torch modules ->
    max-pool over the neighbourhood.  Same results as upstream's module; the padded (B, C, npoint, nsample) tensor is materialised,
    as it is there (no shipped GA-DDPG configuration builds these forms).

    npoint and cloud size: both paths take what upstream takes, npoint > N and clouds beyond one workgroup's LDS included, by the
    routing predicates of pointnet2_utils (fps_fits_one_workgroup, ball_query_uses_grid): shapes the LDS kernels hold keep
    gad_furthest_point_sampling and gad_ball_query, every other shape runs gad_fps_tiled and, from 262 144 points (or beyond 4096
    with library option "bq_grid" = 2), gad_ball_query_grid -- same centroids and neighbourhoods.  With several scales the fused path runs once per scale and each
    pass repeats the furthest point sampling (npoint + 1 launches per scale for a cloud gad_fps_tiled takes); sharing it between
    the scales is left undone.  The only refusal left on the fused path is a shape whose rows overflow the layer kernels' 32-bit
    indexing (RuntimeError with the sizes).  engine.Geometry -- the update step and feature_forward, not these modules -- keeps
    the LDS sampler and its refusals (include/gaddpg.h: N <= 16384, npoint <= N, (3N + npoint + 64) * 4 bytes within 160 KiB).

    coordinate_grad (keyword-only, default False; a plain attribute that may be set after construction, not part of state_dict):
    upstream's module is differentiable in xyz -- grouped_xyz - new_xyz enters the first convolution, new_xyz is a gather of xyz --
    and so is _generic_forward.  The fused path treats xyz as geometry unless this switch is on: off, xyz.grad stays None and
    new_xyz does not require a gradient, whatever xyz.requires_grad says (GA-DDPG slices xyz out of a tensor that requires one for
    other reasons).  On, and only where xyz.requires_grad with gradients enabled, new_xyz is differentiable and xyz.grad receives
    what upstream's would (gad_sa_coord_grad; ga_ddpg_amd.sa_function); such a call is refused (RuntimeError at the forward) in
    eval mode and while hip.deterministic() is in force.  The sampling and the ball query stay non-differentiable, as upstream."""

    def __init__(self, npoint, radii, nsamples, mlps, bn=True, use_xyz=True, *, coordinate_grad=False):
        super().__init__()
        self.bn, self.use_xyz = bool(bn), bool(use_xyz)
        self.coordinate_grad = bool(coordinate_grad)
        self.npoint = npoint
        self.radii, self.nsamples = list(radii), list(nsamples)
        self.radius, self.nsample = radii[0], nsamples[0]
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            spec = list(spec)
            self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz)
                                 if npoint is not None else pointnet2_utils.GroupAll(use_xyz))
            if use_xyz:
                spec[0] += 3
            self.mlps.append(build_shared_mlp(spec, bn))
        if len(self.radii) > 1:           # (plain attribute: kept out of _modules / state_dict)
            object.__setattr__(self, "_scales", [_Scale(self, i) for i in range(len(self.radii))])

    def _generic_forward(self, xyz, features):
        """upstream _PointnetSAModuleBase.forward over this package's operators (see the class docstring)"""
        import torch
        import torch.nn.functional as F
        new_xyz = None
        if self.npoint is not None:
            idx = pointnet2_utils.furthest_point_sample(xyz, self.npoint)
            new_xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
        outs = []
        for grouper, mlp in zip(self.groupers, self.mlps):
            x = mlp(grouper(xyz, new_xyz, features))
            outs.append(F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1))
        return new_xyz, torch.cat(outs, dim=1)

    def forward(self, xyz, features):
        from ..sa_function import sa_module_forward
        if not (self.bn and self.use_xyz) or features is None:
            return self._generic_forward(xyz, features)
        if len(self.radii) == 1:
            return sa_module_forward(self, xyz, features)
        # multi-scale grouping (upstream PointnetSAModuleMSG.forward): every scale groups around the SAME centroids -- furthest
        # point sampling is deterministic, so each scale's fused pass re-derives them -- and the pooled features are
        # concatenated along the channels in scale order
        import torch
        new_xyz, outs = None, []
        for sc in self._scales:
            sc.train(self.training)
            sc.coordinate_grad = self.coordinate_grad
            new_xyz, f = sa_module_forward(sc, xyz, features)
            outs.append(f)
        return new_xyz, torch.cat(outs, dim=1)


class PointnetSAModule(PointnetSAModuleMSG):
    def __init__(self, mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True, *, coordinate_grad=False):
        super().__init__(npoint=npoint, radii=[radius], nsamples=[nsample], mlps=[mlp], bn=bn, use_xyz=use_xyz,
                         coordinate_grad=coordinate_grad)


class PointnetFPModule(nn.Module):
    """feature propagation: the features of `known` (B,m,3) are carried to `unknown` (B,n,3) by inverse-distance weights over the
    three nearest known points (pointnet2_utils.three_nn / three_interpolate: libgaddpg section A kernels, differentiable in the
    features), concatenated with the skip features and passed through the shared MLP as torch modules -- the route
    _generic_forward takes for the non-fused set-abstraction forms.  The cost in m: three_nn searches a uniform grid over `known`
    (gad_three_nn_grid) where pointnet2_utils.three_nn_uses_grid(n, m) holds and walks all m known points per query otherwise;
    the indices, the distances and hence the output and every gradient are the same bit for bit on either route"""

    def __init__(self, mlp, bn=True):
        super().__init__()
        self.mlp = build_shared_mlp(list(mlp), bn)

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown (B,n,3), known (B,m,3) | None, unknow_feats (B,C1,n) | None, known_feats (B,C2,m) -> (B,mlp[-1],n)"""
        import torch
        if known is not None:
            dist, idx = pointnet2_utils.three_nn(unknown, known)
            w = 1.0 / (dist + 1e-8)
            w = w / w.sum(dim=2, keepdim=True)
            x = pointnet2_utils.three_interpolate(known_feats, idx, w)
        else:
            x = known_feats.expand(*known_feats.shape[:2], unknown.shape[1])
        if unknow_feats is not None:
            x = torch.cat([x, unknow_feats], dim=1)
        return self.mlp(x.unsqueeze(-1)).squeeze(-1)
