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
pointnet2_utils.three_nn_uses_grid and the exhaustive gad_three_nn otherwise -- same neighbours, so the same output.  With the
module's `fused` switch (opt-in) the interpolation, the concatenation and the shared MLP run on the layer-GEMM family instead
(gaddpg.h section C.2: gad_fp_rows, gad_rows_act_out and their gradients around gad_gemm_fwd / _dx / _dw; ga_ddpg_amd.fp_function
holds the autograd wrapper)."""
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
    the indices, the distances and hence the output and every gradient are the same bit for bit on either route.

    fused (keyword-only, default False; a plain attribute that may be set after construction, not part of state_dict -- the
    precedent is PointnetSAModuleMSG.coordinate_grad): off, forward is the composition above, unchanged.  On, a call runs on the
    layer-GEMM family (ga_ddpg_amd.fp_function): the interpolation is written straight into the columns of one row matrix beside
    the skip features (gad_fp_rows; nothing is materialised channel-major between the module's input and its output), every
    layer is a gad_gemm_fwd launch with the encoder's arithmetic (FP32-MFMA or split-bf16 products, f64 BatchNorm statistics in
    the epilogue), the backward drives gad_gemm_dx / gad_gemm_dw, and under hip.deterministic() every tensor is bit-reproducible
    with the library option alone.  three_nn and the three weight lines stay as they are.  The fused path takes a call where
    bn=True, known is given, the inputs are CUDA float32, B * n >= 2, every layer width is a multiple of 4 up to 1024 (mlp[0]
    itself may be any size up to 1024) and the row tensors stay within 32-bit element indexing; every other call -- known=None,
    bn=False, a backward through eval-mode BatchNorm, CPU tensors -- takes the composition exactly as with the switch off.
    `last_route` says which one the last forward took ("fused" | "composed").  state_dict keys and values, load_state_dict,
    .train() / .eval() / .to() and ordinary torch optimizers work as before (after the first fused call the parameters and the
    running statistics are views of flat buffers, as for the set-abstraction modules); running statistics and
    num_batches_tracked advance as torch's do.
    Measured (tools/bench_fp_module.py, profiles/fp_fused.txt; forward + backward, train mode, B = 16, the four decoder levels of
    a PointNet++ SSG segmentation network on 4096-point clouds, us per call composed / fused):
    768-256-256 at n 64: 729 / 499 (1.46 x); 384-256-256 at n 256: 737 / 502 (1.47 x); 320-256-128 at n 1024: 766 / 512
    (1.50 x); 134-128-128-128 at n 4096: 1072 / 735 (1.46 x).  The fused path is ahead at every level; no level was found
    where the composition wins.  The three coarse levels follow the host's launch rate on either path (the same time
    whatever n), only the finest is long enough for device time to show"""

    def __init__(self, mlp, bn=True, *, fused=False):
        super().__init__()
        self.mlp = build_shared_mlp(list(mlp), bn)
        self.bn = bool(bn)
        self.fused = bool(fused)
        self.last_route = None            # "fused" | "composed": the route the last forward took

    def _fused_call(self, unknown, known, unknow_feats, known_feats):
        """does this call take the fused path (see the class docstring)"""
        import torch
        from .. import fp_function
        if not (self.fused and self.bn and known is not None and known_feats is not None):
            return False
        ts = [unknown, known, known_feats] + ([] if unknow_feats is None else [unknow_feats])
        if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in ts):
            return False
        if unknown.dim() != 3 or known.dim() != 3 or known_feats.dim() != 3 or (unknow_feats is not None and unknow_feats.dim() != 3):
            return False
        B, n, m = unknown.shape[0], unknown.shape[1], known.shape[1]
        c1 = 0 if unknow_feats is None else unknow_feats.shape[1]
        if known_feats.shape[0] != B or known_feats.shape[2] != m or (c1 and (unknow_feats.shape[0] != B or unknow_feats.shape[2] != n)):
            return False
        if not fp_function.fits(self, B, n, m, c1, known_feats.shape[1]):
            return False
        if not self.training and torch.is_grad_enabled():       # a backward through eval-mode BatchNorm: the composition has one
            feats = [known_feats] + ([] if unknow_feats is None else [unknow_feats])
            if any(t.requires_grad for t in feats) or any(p.requires_grad for p in self.parameters()):
                return False
        return True

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown (B,n,3), known (B,m,3) | None, unknow_feats (B,C1,n) | None, known_feats (B,C2,m) -> (B,mlp[-1],n)"""
        import torch
        if self._fused_call(unknown, known, unknow_feats, known_feats):
            from ..fp_function import fp_module_forward
            dist, idx = pointnet2_utils.three_nn(unknown, known)
            w = 1.0 / (dist + 1e-8)
            w = w / w.sum(dim=2, keepdim=True)
            self.last_route = "fused"
            return fp_module_forward(self, idx, w, unknow_feats, known_feats)
        self.last_route = "composed"
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
