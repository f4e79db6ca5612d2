"""Stand-alone evaluation of one `PointnetSAModule` through the fused libgaddpg path
(pointnet2_ops.pointnet2_modules.PointnetSAModule.forward): FPS -> ball query -> de-duplicated rows
-> gather + 3 x (1x1 conv, BatchNorm, ReLU) as FP32-MFMA GEMMs -> segment max-pool.
Every layer launch is spelled by the emitters of engine.py over this run's stage view (engine.stage_view): the same descriptions
the update step's encoder uses; this file decides which launches a module makes and owns their buffers.
Cloud size: shapes the one-workgroup kernels hold keep their calls (gad_furthest_point_sampling, gad_ball_query); every other
shape takes gad_fps_tiled (npoint + 1 launches) and, where pointnet2_utils.ball_query_uses_grid holds, gad_ball_query_grid -- the
routing predicates of pointnet2_utils, evaluated when the _StageRun is built; its workspaces belong to it.

Differentiable: the forward is wrapped in a torch.autograd.Function whose backward drives the same
dX / dW kernels as the fused update step (BatchNorm-backward with weighted statistics, max-pool routing
through the saved arg-max, scatter-add into the point features), so a network written against upstream's
`pointnet2_ops` -- the reference's own core/networks.py:66-81,217-220 -- trains through this package
with ordinary torch optimizers.  Gradients: wrt `features` and every parameter of the module.  `xyz` is
geometry by default (FPS / ball-query indices are not differentiable upstream either; GA-DDPG never asks for
the coordinates' gradient: xyz is detached and new_xyz is not differentiable).  The module attribute
`coordinate_grad` (pointnet2_modules: keyword-only, default False) switches upstream's coordinate path on: with
it set and xyz.requires_grad, the recentred xyz channels of the first convolution are differentiated by
gad_sa_coord_grad (one call behind the first layer's dX, same dZ descriptor) -- + to every row's point, - to its
group's centroid point, plus whatever arrives through new_xyz, which is then differentiable as well (the GroupAll
form has no centroid terms).  Refused at forward time with the switch live: eval mode (as for every backward
here) and the library's deterministic mode (the scatter is float atomics; there is no ordered form).
Upstream semantics mirrored: _PointnetSAModuleBase.forward: returns
(new_xyz (B,npoint,3) | None, new_features (B, mlp[-1], npoint | 1)).
"""
import ctypes as C

import torch

from . import engine, hip
from .engine import FlatNet, MatSpec, Plan, _ptr
from .pointnet2_ops import pointnet2_utils as pu


class _StageNet(object):
    """packed parameters of one SA module: what the emitters of engine.py read of an engine.EncoderNet (flat, running statistics,
    bn_off), over the module's three layers"""

    def __init__(self, mod, device):
        seq = mod.mlps[0]
        c_feat = seq[0].weight.shape[1] - 3
        if c_feat < 1:
            raise NotImplementedError("PointnetSAModule without input features is not used by GA-DDPG")
        self.c_feat = c_feat                                  # channels of the `features` argument
        self.c_pad = (c_feat + 3) // 4 * 4                    # point-major feature rows are padded to 16 bytes
        self.mats = [MatSpec(seq[0].weight, None, seq[1], gather_feat_c=self.c_pad), MatSpec(seq[3].weight, None, seq[4]),
                     MatSpec(seq[6].weight, None, seq[7])]
        for i, m in enumerate(self.mats):
            m.bn_index = i
        self.flat = FlatNet(list(mod.named_parameters()), self.mats, device)
        self.flat.enable_split(engine.split_mirror_layers(self.mats))          # (library option "mfma_split")
        (self.running_mean, self.running_var, self.batches_tracked, self.bn_off,
         self.bn_total) = engine.adopt_running_stats(self.mats, device)
        self.free = {}                                        # (B, N) -> activation sets returned by finished backwards


class _StageRun(object):
    """static buffers + launch plans of one forward (and its backward) at a fixed (B, N)"""

    def __init__(self, net, mod, B, N, device, with_backward=False):
        f32 = dict(dtype=torch.float32, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.B, self.N = B, N
        self.group_all = mod.npoint is None
        M = 1 if self.group_all else mod.npoint
        S = N if self.group_all else mod.nsample
        self.M, self.S, self.radius = M, S, None if self.group_all else float(mod.radius)
        G = B * M
        cap = G * S
        # the row lists and layer kernels hold point and row numbers, and element offsets built from them, in int32: point rows of
        # c_pad floats, activation rows of up to max(n_out) floats
        widest = max(m.n_out for m in net.mats)
        if B * N * max(net.c_pad, 3) >= 2 ** 31 or cap * widest >= 2 ** 31:
            raise RuntimeError("PointnetSAModule: B=%d N=%d npoint=%d nsample=%d needs %d point rows of %d floats and %d activation "
                               "rows of %d floats; the fused path indexes the elements of both in 32 bits"
                               % (B, N, M, S, B * N, net.c_pad, cap, widest))
        self.xyz = torch.empty(B, N, 3, **f32)
        self.feat = torch.zeros(B * N, net.c_pad, **f32)      # padding columns stay zero
        self.new_xyz = torch.empty(B, M, 3, **f32)
        self.fps = torch.empty(B, M, **i32)
        self.idx = torch.empty(B, M, S, **i32) if not self.group_all else None
        self.cnt = torch.empty(B, M, **i32) if not self.group_all else None
        self.rows = r = engine.stage_rows(G, cap, device)
        if self.group_all:
            hip.call("gad_rows_group_all", B, N, r["off"], r["pt"], r["grp"], r["w"], r["n"])
        self.Z = [torch.empty(cap, m.n_out, **f32) for m in net.mats]
        c_out = net.mats[2].n_out
        self.F = torch.empty(G, c_out, **f32)
        self.argmax = torch.empty(G, c_out, dtype=torch.int32, device=device)
        tot = net.bn_total
        self.tot = tot
        self.stats = torch.zeros(hip.STAT_REPLICAS * 2 * tot, dtype=torch.float64, device=device)
        self.scale = torch.empty(tot, **f32)
        self.shift = torch.empty(tot, **f32)
        self.mean = torch.empty(tot, **f32)
        self.istd = torch.empty(tot, **f32)
        self.count = float(G * S)
        # max-pool folded into the third GEMM's epilogue (packed arg-max keys, finished by gad_pool_finalize) where the entry point
        # takes it: rows a multiple of 4, channels a multiple of 64; else the separate segment max-pool operator
        self.fused_pool = cap % 4 == 0 and c_out % 64 == 0
        self.key = torch.zeros(G, c_out, dtype=torch.int64, device=device) if self.fused_pool else None
        # raw value of every arg-max row (the backward's BatchNorm sums read it instead of gathering z[argmax])
        self.zmax = torch.empty(G, c_out, **f32) if (self.fused_pool and with_backward) else None
        self.workspaces = {}                                  # entry point -> device workspace (shapes beyond the LDS kernels)
        self.G = self.dF = self.bwd = None
        if with_backward:
            self.bstats = torch.zeros(hip.STAT_REPLICAS * 2 * tot, dtype=torch.float64, device=device)
            self.coef = torch.empty(3 * tot, **f32)
            self.G = [torch.empty(cap * net.mats[l].n_out, **f32) for l in (1, 0)]
            self.dF = torch.zeros(G, c_out, **f32)
            self.dfeat = torch.zeros(B * N, net.c_pad, **f32)
            self.grad = torch.zeros(net.flat.n, **f32)        # this call's parameter gradients (master layout)
        # what engine's emitters read of this run: one stage whose first layer gathers [features, xyz - centroid]
        self.view = engine.stage_view(self, net.mats, net.bn_off, rows=r, Z=self.Z, F=self.F, argmax=self.argmax, key=self.key,
                                      zmax=self.zmax, count=self.count, G=self.G, dF=self.dF, src_xyz=self.xyz,
                                      ctr_xyz=None if self.group_all else self.new_xyz, feat=self.feat, feat_c=net.c_pad,
                                      action=None, act_c=0, grp_per_sample=M)
        self.plans = {t: self._plan(net, t) for t in (True, False)}
        if with_backward:
            self.bwd = self._plan_backward(net)
        self.bwd_xyz = None                                   # the backward plan with the coordinate gradient (coord_backward)

    def _workspace(self, name, *shape):
        ws = self.workspaces.get(name)
        if ws is None:
            ws = self.workspaces[name] = hip.workspace(name, self.xyz.device, *shape)
        return ws

    def _plan(self, net, train):
        plan = Plan()
        B, N, M, S, r, v = self.B, self.N, self.M, self.S, self.rows, self.view
        if not self.group_all:
            # shapes beyond the LDS kernels take the entry points of the facade (pointnet2_utils: same predicates, same indices);
            # their workspaces belong to this run -- its forward is one stream, so one per entry point serves both plans
            if pu.fps_fits_one_workgroup(N, M):
                plan.call("gad_furthest_point_sampling", self.xyz, B, N, M, self.fps, self.new_xyz)
            else:
                plan.call("gad_fps_tiled", self.xyz, B, N, M, 0, self.fps, self.new_xyz, self._workspace("gad_fps_tiled", B, N, M, 0))
            if pu.ball_query_uses_grid(N):
                plan.call("gad_ball_query_grid", self.new_xyz, self.xyz, B, N, M, self.radius, S, self.idx, self.cnt,
                          self._workspace("gad_ball_query_grid", B, N, M, S))
            else:
                plan.call("gad_ball_query", self.new_xyz, self.xyz, B, N, M, self.radius, S, self.idx, self.cnt)
            plan.call("gad_rows_from_ball_query", self.idx, self.cnt, B * M, M, N, S, r["off"], r["pt"], r["grp"],
                      r["w"], r["n"])
        plan.zero(self.stats)
        for l in range(3):
            pooled = l == 2 and self.fused_pool
            plan.call_struct("gad_gemm_fwd", engine.fwd_gemm_args(net, v, l, self.Z[l], stats=train, pooled=pooled))
            if not train:
                engine.emit_bn_eval_affine(plan, net, v, l)
            if pooled:
                engine.emit_pool_finalize(plan, net, v, train)
            elif train:
                engine.emit_bn_finalize(plan, net, v, l)
        if not self.fused_pool:
            m = net.mats[2]
            o = net.bn_off[2]
            # (gad_segment_pool: torch's "first maximal activation" arg-max; the fused form takes the largest raw value, which is the
            # same row unless two different raw values round to one activation)
            plan.call("gad_segment_pool", self.Z[2], m.n_out, m.n_out, _ptr(self.scale, o), _ptr(self.shift, o),
                      r["off"], r["G"], self.F, self.argmax)
        return plan

    def coord_backward(self, net):
        """the backward plan of a call whose xyz asks for its gradient (module switch `coordinate_grad`): built on first use, with the
        buffers only that plan needs -- dxyz (B*N, 3), the per-group sums dctr (G, 3), the incoming gradient of new_xyz and the
        centroids' global point numbers b * N + fps (refreshed by the backward: the forward plan leaves fps)"""
        if self.bwd_xyz is None:
            dev, G = self.xyz.device, self.rows["G"]
            f32 = dict(dtype=torch.float32, device=dev)
            self.dxyz = torch.zeros(self.B * self.N, 3, **f32)
            if not self.group_all:
                self.dctr = torch.zeros(G, 3, **f32)
                self.g_new = torch.zeros(G, 3, **f32)
                self.ctr = torch.zeros(self.B, self.M, dtype=torch.int32, device=dev)
                self.pt0 = (torch.arange(self.B, dtype=torch.int32, device=dev) * self.N).view(self.B, 1)
            self.bwd_xyz = self._plan_backward(net, coord=True)
        return self.bwd_xyz

    def _plan_backward(self, net, coord=False):
        """consumes self.dF (G, c_out) = dLoss/d(pooled output); leaves dLoss/dfeatures in self.dfeat (point-major,
        padded) and this call's parameter gradients in self.grad.  Train-mode BatchNorm only (batch statistics).
        coord: also consumes self.g_new = dLoss/d(new_xyz) and leaves dLoss/dxyz in self.dxyz (see coord_backward)."""
        plan = Plan()
        r, v, fl = self.rows, self.view, net.flat
        plan.zero_multi([fl.gacc, self.bstats, self.dfeat] + ([self.dxyz, None if self.group_all else self.dctr] if coord else []))
        m1, m2, m3 = net.mats
        ws = engine.dw_workspace(fl.device, lane=0)

        def dz(l, **src):
            """layer l's dZ descriptor behind its coefficient launch (which also adds its dgamma / dbeta to the arena)"""
            engine.emit_bn_bwd_coef(plan, net, v, l, self.count)
            return engine.bn_dz(net, v, l, **src)

        def dw_args(l, d):
            return engine.dw_args(fl, [net.mats[l]], engine.layer_input(net, v, l), d, ws)

        def dx_args(l, d, k_valid, **epi):
            return engine.dx_args(fl, d, net.mats[l], k_valid, r["cap"], _ptr(r["n"]), **epi)

        def bwd(l, d, k_valid):
            """dW and dX of layer l in one call (gad_gemm_bwd): SA1-like shapes (64 input channels, >= 32768 rows) stream dZ once
            for both products, every other shape runs the same two launches as gad_gemm_dw + gad_gemm_dx; the gradient travels
            ReLU-masked to layer l - 1 (store_masked / premasked)"""
            pm = net.mats[l - 1]
            aw = dw_args(l, d)
            a = dx_args(l, d, k_valid, epilogue=0, gout=_ptr(self.G[2 - l]), gout_pitch=pm.n_out, **engine.prev_block(v, l - 1))
            plan.keep.extend([a, aw])
            plan.call("gad_gemm_bwd", a, aw)

        engine.emit_pool_bwd_stats(plan, v)
        bwd(2, dz(2, pooled=True), m2.n_out)
        bwd(1, dz(1, G=self.G[0]), m1.n_out)
        d = dz(0, G=self.G[1])          # the dW precedes the dX below: both read the one coefficient launch
        plan.call_struct("gad_gemm_dw", dw_args(0, d))
        plan.call_struct("gad_gemm_dx", dx_args(0, d, net.c_pad, epilogue=1, dfeat=_ptr(self.dfeat), feat_c=net.c_pad,
                                                row_pt=_ptr(r["pt"]), row_grp=_ptr(r["grp"]), act_c=0, grp_per_sample=self.M))
        if coord:
            # the three packed columns [c_pad, c_pad + 3) the scatter epilogue above skips: same dZ, same weights
            ga = self.group_all
            plan.call("gad_sa_coord_grad", d, fl.p_w(m1), m1.Kp, m1.n_out, net.c_pad,
                      _ptr(r["n"]), r["cap"], _ptr(r["pt"]), None if ga else _ptr(r["grp"]), None if ga else self.ctr,
                      None if ga else self.g_new, r["G"], self.B * self.N, self.dxyz, None if ga else self.dctr)
        plan.call("gad_grad_from_arena", fl.gacc, fl.m2p, fl.n, self.grad, 0)
        return plan


def _stage_net(mod, dev):
    rt = mod.__dict__.get("_gad_rt")
    if rt is None:
        rt = {"net": _StageNet(mod, dev)}
        object.__setattr__(mod, "_gad_rt", rt)
    return rt


def _transpose(src, dst, B, R, C_, src_pitch, src_batch, dst_pitch, dst_batch):
    """dst[b][j][i] = src[b][i][j] (gad_transpose_batched): the (B, C, N) <-> point-major hand-over at the module boundary"""
    src = src if (src.is_contiguous() and src.dtype == torch.float32) else src.contiguous().float()
    hip.call("gad_transpose_batched", src, dst, B, R, C_, src_pitch, C.c_longlong(src_batch), dst_pitch, C.c_longlong(dst_batch))


def _run_forward(mod, net, run, xyz, features):
    B, N = run.B, run.N
    net.flat.sync_packed()            # the parameters may have been stepped by an ordinary torch optimizer
    run.xyz.copy_(xyz)
    _transpose(features, run.feat, B, net.c_feat, N, N, net.c_feat * N, net.c_pad, N * net.c_pad)     # (B,C,N) -> point-major rows
    run.plans[bool(mod.training)].run()
    if mod.training:
        net.batches_tracked += 1
    c_out = net.mats[2].n_out
    out = torch.empty(B, c_out, run.M, dtype=torch.float32, device=xyz.device)
    _transpose(run.F, out, B, run.M, c_out, c_out, run.M * c_out, run.M, c_out * run.M)
    return (None if run.group_all else run.new_xyz.clone()), out


class _SAFunction(torch.autograd.Function):
    """forward / backward of one set-abstraction module over its own activation set (held by the graph node until the
    backward has run, then recycled): several forwards of the same module may be in flight, as in the reference's
    update step (value encoder on the current and on the next state)."""

    @staticmethod
    def forward(ctx, mod, xyz, features, *params):
        rt = _stage_net(mod, xyz.device)
        net = rt["net"]
        B, N, _ = xyz.shape
        pool = net.free.setdefault((B, N), [])
        run = pool.pop() if pool else _StageRun(net, mod, B, N, xyz.device, with_backward=True)
        new_xyz, out = _run_forward(mod, net, run, xyz, features)
        ctx.run, ctx.net, ctx.key = run, net, (B, N)
        ctx.feat_grad = features.requires_grad
        ctx.coord = ctx.needs_input_grad[1]                    # (sa_module_forward detaches xyz unless the module's switch is on)
        if not ctx.coord:
            ctx.mark_non_differentiable(*([new_xyz] if new_xyz is not None else []))
        return (new_xyz if new_xyz is not None else xyz.new_zeros(0)), out

    @staticmethod
    def backward(ctx, g_xyz, g_out):
        run, net = ctx.run, ctx.net
        B, N = ctx.key
        c_out = net.mats[2].n_out
        _transpose(g_out, run.dF, B, c_out, run.M, run.M, c_out * run.M, c_out, run.M * c_out)
        g_pts = None
        if ctx.coord:
            plan = run.coord_backward(net)
            if not run.group_all:
                run.g_new.copy_(g_xyz.reshape(run.rows["G"], 3))       # (autograd hands zeros when new_xyz went unused)
                torch.add(run.fps, run.pt0, out=run.ctr)
            plan.run()
            g_pts = run.dxyz.view(B, N, 3).clone()
        else:
            run.bwd.run()
        g_feat = None
        if ctx.feat_grad:
            g_feat = torch.empty(B, net.c_feat, N, dtype=torch.float32, device=g_out.device)
            _transpose(run.dfeat, g_feat, B, N, net.c_feat, net.c_pad, N * net.c_pad, N, net.c_feat * N)
        grads = []
        # ONE copy of the call's parameter gradients; VIEWS of it go out.  Autograd may adopt such a view as p.grad (set_to_none /
        # first accumulation): the parameters' .grad tensors of one call then share one storage (disjoint slices: in-place optimizers
        # are unaffected; the flat buffer lives as long as any of them).  One clone per parameter would cost nine launches per call.
        gcopy = run.grad.clone()
        for p, o in zip(net.flat.params, net.flat.offsets[:-1]):
            o = int(o)
            grads.append(gcopy[o:o + p.numel()].view(p.shape) if p.requires_grad else None)
        net.free[ctx.key].append(run)                          # recycled: everything handed out above is a copy
        ctx.run = None
        return (None, g_pts, g_feat) + tuple(grads)


def sa_module_forward(mod, xyz, features):
    hip.require_cuda(xyz, features)
    if features is None:
        raise NotImplementedError("PointnetSAModule without input features is not used by GA-DDPG")
    # xyz may arrive with requires_grad=True for bookkeeping reasons only (the reference slices it out of the tensor that
    # carries the broadcast action channels, core/networks.py:239): it is treated as geometry, its gradient is None -- unless
    # the module's `coordinate_grad` switch asks for upstream's coordinate path
    coord = bool(getattr(mod, "coordinate_grad", False)) and torch.is_grad_enabled() and xyz.requires_grad
    if not coord:
        xyz = xyz.detach()
    B, N, _ = xyz.shape
    dev = xyz.device
    rt = _stage_net(mod, dev)
    net = rt["net"]
    if features.shape[1] != net.c_feat:
        raise RuntimeError("features have %d channels, module expects %d" % (features.shape[1], net.c_feat))
    params = net.flat.params
    needs_grad = torch.is_grad_enabled() and (coord or features.requires_grad or any(p.requires_grad for p in params))
    if needs_grad:
        if not mod.training:
            raise RuntimeError("PointnetSAModule: backward through eval-mode BatchNorm (running statistics) is not "
                               "implemented; call .train() or wrap the call in torch.no_grad()")
        if coord and hip.deterministic():
            raise RuntimeError("PointnetSAModule: coordinate_grad is on and xyz requires a gradient, but the deterministic mode is "
                               "in force (option \"deterministic\" / torch.use_deterministic_algorithms): the coordinate scatter "
                               "adds with float atomics and has no ordered form; switch one of the two off")
        new_xyz, out = _SAFunction.apply(mod, xyz, features, *params)
        return (None if new_xyz.numel() == 0 else new_xyz), out
    key = (B, N)
    if key not in rt:
        rt[key] = _StageRun(net, mod, B, N, dev)
    return _run_forward(mod, net, rt[key], xyz, features)
