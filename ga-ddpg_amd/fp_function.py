"""Stand-alone evaluation of one `PointnetFPModule` on the layer-GEMM family of libgaddpg (the module's `fused` switch,
pointnet2_ops.pointnet2_modules.PointnetFPModule.forward): the interpolated known features and the skip features become the
columns of ONE dense row matrix (gad_fp_rows, gad_transpose_batched with a destination pitch), the shared MLP runs over it as
gad_gemm_fwd launches with train-mode BatchNorm statistics between them -- a stage view with rows=None, the form of the encoder's
FC pair, at any depth -- and the last layer's activation goes out channel-major (gad_rows_act_out).  Every layer launch is spelled
by the emitters of engine.py; this file decides which launches a module makes and owns their buffers, as sa_function.py does for
set abstraction.

Row matrix: (B * n, c_pad) float32, c_pad = C2 + C1 rounded up to 4; columns [0, C2) the interpolation, [C2, C2 + C1) the skip
features, the rest zero (cleared once: nothing writes them).  The column order is torch.cat's, so the first convolution's weight
packs without a permutation; gad_transpose_batched reads and writes single floats, so C2 needs no padding of its own.  The first
layer reads the rows with no affine map and no ReLU (engine.layer_input's FC-1 form).

Routes (read off the predicates of csrc/gemm_*.hip, not probed).  The first layer has an identity input: the wide and streaming
kernels ask for scale / shift / relu, so it takes the skinny kernels up to 1024 rows and the 64 x 64 tile kernels beyond.  Later
layers also reach the wide kernels from 2048 rows (forward: outputs a multiple of 128, inputs a multiple of 32 up to 512) and the
streaming kernels from 32 768 rows with 64 input channels and 64 / 128 outputs; row_w and n_rows_dev are NULL throughout.  Every
layer width must be a multiple of 4 (check_input: an ACT input's channel count and pitch); a module with another width keeps the
composition.

Differentiable: a torch.autograd.Function whose backward drives gad_rows_act_bwd_stats, then per layer from the top
gad_bn_bwd_coef + gad_gemm_bwd (= gad_gemm_dw, gad_gemm_dx with the previous layer's mask and sums, fused where gemm_bwd.hip
fuses them), the first layer's dX storing the row gradient; its columns go back through one transpose (skip features) and
gad_fp_rows_grad + one transpose (known features).  Under hip.deterministic() the known-feature gradient takes the ordered route:
the row gradient's first C2 columns are transposed to (B, C2, n) and gad_three_interpolate_grad's ordered form scatters them, so
the whole module is bit-reproducible with the library option alone.  Gradients: wrt unknow_feats, known_feats and every parameter;
the coordinates, the neighbour indices and the weights are not differentiable (they are not in the composition either).
"""
import ctypes as C

import torch
import torch.nn as nn

from . import engine, hip
from .engine import FlatNet, MatSpec, Plan, _ptr

MAX_WIDTH = 1024              # most input / output channels of a layer (csrc/gemm_common.hpp VMAX)


def layer_modules(mod):
    """the (Conv2d, BatchNorm2d) pairs of mod.mlp in order"""
    seq = list(mod.mlp)
    convs = [m for m in seq if isinstance(m, nn.Conv2d)]
    bns = [m for m in seq if isinstance(m, nn.BatchNorm2d)]
    return list(zip(convs, bns)) if len(convs) == len(bns) else []


def fits(mod, B, n, m, c1, c2):
    """does the fused path hold this call: at least one layer, two or more rows (train-mode BatchNorm), the channel counts the
    module was built for, every width a multiple of 4 up to MAX_WIDTH, row tensors within 32-bit element indexing"""
    layers = layer_modules(mod)
    if not layers or B * n < 2 or m < 1 or c2 < 1 or layers[0][0].weight.shape[1] != c1 + c2:
        return False
    widths = [conv.weight.shape[0] for conv, _ in layers]
    c_pad = (c1 + c2 + 3) // 4 * 4
    if c_pad > MAX_WIDTH or any(w % 4 != 0 or w > MAX_WIDTH for w in widths):
        return False
    return B * n * max([c_pad] + widths) < 2 ** 31 and B * m * c2 < 2 ** 31 and B <= 65535


class _FPNet(object):
    """packed parameters of one FP module: what the emitters of engine.py read of an engine.EncoderNet (flat, running statistics,
    bn_off), over the module's layers"""

    def __init__(self, mod, device):
        self.mats = [MatSpec(conv.weight, None, bn) for conv, bn in layer_modules(mod)]
        for i, m in enumerate(self.mats):
            m.bn_index = i
        self.c_in = self.mats[0].k_in
        self.c_pad = (self.c_in + 3) // 4 * 4                 # the row matrix is read in 16-byte pieces
        self.flat = FlatNet(list(mod.named_parameters()), self.mats, device)
        # engine.split_mirror_layers' rule for layers behind a BatchNorm + ReLU (all columns, Ks = Kp); the first layer's identity
        # input never reaches a kernel that reads a mirror
        self.flat.enable_split([(m, m.Kp) for m in self.mats[1:]][:hip.MAX_SPLIT_LAYERS])
        (self.running_mean, self.running_var, self.batches_tracked, self.bn_off,
         self.bn_total) = engine.adopt_running_stats(self.mats, device)
        self.free = {}                                        # (B, n, m, C2) -> runs returned by finished backwards


def _ll(v):
    return C.c_longlong(int(v))


class _FPRun(object):
    """static buffers + launch plans of one forward (and its backward) at a fixed (B, n, m, C2); the feature tensors that come in
    and go out are not copied: their addresses are patched into the plans at every run"""

    def __init__(self, net, B, n, m, c2, device, with_backward=False):
        f32 = dict(dtype=torch.float32, device=device)
        self.B, self.n, self.m, self.c2, self.c1 = B, n, m, c2, net.c_in - c2
        R = B * n
        self.idx = torch.zeros(B, n, 3, dtype=torch.int32, device=device)
        self.w = torch.zeros(B, n, 3, **f32)
        self.kpm = torch.empty(B * m, c2, **f32)              # known features, point-major
        self.rows = torch.zeros(R, net.c_pad, **f32)          # padding columns stay zero
        self.Z = [torch.empty(R, mt.n_out, **f32) for mt in net.mats]
        tot = net.bn_total
        self.tot = tot
        self.stats = torch.zeros(hip.STAT_REPLICAS * 2 * tot, dtype=torch.float64, device=device)
        self.scale = torch.empty(tot, **f32)
        self.shift = torch.empty(tot, **f32)
        self.mean = torch.empty(tot, **f32)
        self.istd = torch.empty(tot, **f32)
        self.count = float(R)
        self.G = None
        if with_backward:
            self.bstats = torch.zeros(hip.STAT_REPLICAS * 2 * tot, dtype=torch.float64, device=device)
            self.coef = torch.empty(3 * tot, **f32)
            self.G = [torch.empty(R, mt.n_out, **f32) for mt in net.mats]        # every layer's (masked) dY
            self.drows = torch.empty(R, net.c_pad, **f32)
            self.dkpm = torch.zeros(B * m, c2, **f32)
            self.dT = None                                    # (B, C2, n): the ordered route's transposed row gradient
            self.grad = torch.zeros(net.flat.n, **f32)        # this call's parameter gradients (master layout)
        # what engine's emitters read of this run: one stage of dense rows whose first layer reads the row matrix as it is
        self.view = engine.stage_view(self, net.mats, net.bn_off, rows=None, B=R, Z=self.Z, count=self.count, G=self.G,
                                      feat=self.rows, feat_c=net.c_pad)
        self.plans = {t: self._plan(net, t) for t in (True, False)}
        self.bwd = {}                                         # deterministic (0 / 1) -> backward plan, built on first use

    def _plan(self, net, train):
        plan = Plan()
        B, n, m, c1, c2, v = self.B, self.n, self.m, self.c1, self.c2, self.view
        it = {}
        it["kf"] = plan.call("gad_transpose_batched", self.kpm, self.kpm, B, c2, m, m, _ll(c2 * m), c2, _ll(m * c2))     # (src patched)
        plan.call("gad_fp_rows", self.kpm, c2, self.idx, self.w, B, n, m, c2, self.rows, net.c_pad, 0)
        if c1:
            it["uf"] = plan.call("gad_transpose_batched", self.rows, _ptr(self.rows, c2), B, c1, n, n, _ll(c1 * n), net.c_pad,
                                 _ll(n * net.c_pad))
        plan.zero(self.stats)
        for l in range(len(net.mats)):
            plan.call_struct("gad_gemm_fwd", engine.fwd_gemm_args(net, v, l, self.Z[l], stats=train))
            if train:
                engine.emit_bn_finalize(plan, net, v, l)
            else:
                engine.emit_bn_eval_affine(plan, net, v, l)
        l, mt = len(net.mats) - 1, net.mats[-1]
        it["out"] = plan.call("gad_rows_act_out", self.Z[l], mt.n_out, engine._vec(v, "scale", l), engine._vec(v, "shift", l), B, n,
                              mt.n_out, self.Z[l])
        plan.items = it
        return plan

    def backward_plan(self, net, det):
        if det not in self.bwd:
            self.bwd[det] = self._plan_backward(net, det)
        return self.bwd[det]

    def _plan_backward(self, net, det):
        """consumes dLoss/d(output) (B, C, n) at the patched address; leaves dLoss/d(unknow_feats) and dLoss/d(known_feats) at the
        patched addresses and this call's parameter gradients in self.grad.  Train-mode BatchNorm only (batch statistics)."""
        plan = Plan()
        B, n, m, c1, c2, v, fl = self.B, self.n, self.m, self.c1, self.c2, self.view, net.flat
        R, L = B * n, len(net.mats)
        it = {}
        plan.zero_multi([fl.gacc, self.bstats] + ([] if det else [self.dkpm]))
        ws = engine.dw_workspace(fl.device, lane=0)
        top = net.mats[-1]
        it["dout"] = plan.call("gad_rows_act_bwd_stats", self.G[L - 1], self.Z[L - 1], top.n_out, engine._vec(v, "scale", L - 1),
                               engine._vec(v, "shift", L - 1), engine._vec(v, "mean", L - 1), engine._vec(v, "istd", L - 1), B, n,
                               top.n_out, self.G[L - 1], top.n_out, *engine._sums(v, "bstats", L - 1), 2 * v.tot)

        def dz(l):
            """layer l's dZ descriptor behind its coefficient launch (which also adds its dgamma / dbeta to the arena)"""
            engine.emit_bn_bwd_coef(plan, net, v, l, self.count)
            return engine.bn_dz(net, v, l, G=self.G[l])

        def dw_args(l, d):
            return engine.dw_args(fl, [net.mats[l]], engine.layer_input(net, v, l), d, ws)

        for l in range(L - 1, 0, -1):
            # dW and dX of layer l in one call: the gradient travels ReLU-masked to layer l - 1, whose dbeta / dgamma the dX sums
            pm, d = net.mats[l - 1], dz(l)
            aw = dw_args(l, d)
            a = engine.dx_args(fl, d, net.mats[l], pm.n_out, R, None, epilogue=0, gout=_ptr(self.G[l - 1]), gout_pitch=pm.n_out,
                               **engine.prev_block(v, l - 1))
            plan.keep.extend([a, aw])
            plan.call("gad_gemm_bwd", a, aw)
        d = dz(0)                       # the dW precedes the dX below: both read the one coefficient launch
        plan.call_struct("gad_gemm_dw", dw_args(0, d))
        plan.call_struct("gad_gemm_dx", engine.dx_args(fl, d, net.mats[0], net.c_pad, R, None, epilogue=0, gout=_ptr(self.drows),
                                                       gout_pitch=net.c_pad))
        if c1:
            it["g_uf"] = plan.call("gad_transpose_batched", _ptr(self.drows, c2), self.drows, B, n, c1, net.c_pad, _ll(n * net.c_pad), n,
                                   _ll(c1 * n))
        if det:
            # the ordered route: gad_three_interpolate_grad has an ordered form, gad_fp_rows_grad (float atomics) has none
            if self.dT is None:
                self.dT = torch.empty(B, c2, n, dtype=torch.float32, device=self.drows.device)
            plan.call("gad_transpose_batched", self.drows, self.dT, B, n, c2, net.c_pad, _ll(n * net.c_pad), n, _ll(c2 * n))
            it["g_kf"] = plan.call("gad_three_interpolate_grad", self.dT, self.idx, self.w, B, c2, n, m, self.dT)
            it["g_kf_arg"] = 7
        else:
            plan.call("gad_fp_rows_grad", self.drows, net.c_pad, 0, self.idx, self.w, B, n, m, c2, self.dkpm, c2)
            it["g_kf"] = plan.call("gad_transpose_batched", self.dkpm, self.dkpm, B, m, c2, c2, _ll(m * c2), m, _ll(c2 * m))
            it["g_kf_arg"] = 1
        plan.call("gad_grad_from_arena", fl.gacc, fl.m2p, fl.n, self.grad, 0)
        plan.items = it
        return plan


def _fp_net(mod, dev):
    rt = mod.__dict__.get("_gad_rt")
    if rt is None:
        rt = {"net": _FPNet(mod, dev)}
        object.__setattr__(mod, "_gad_rt", rt)
    return rt


def _f32c(t):
    return t if (t.is_contiguous() and t.dtype == torch.float32) else t.contiguous().float()


def _run_forward(mod, net, run, idx, w, unknow_feats, known_feats):
    net.flat.sync_packed()            # the parameters may have been stepped by an ordinary torch optimizer
    run.idx.copy_(idx)
    run.w.copy_(w)
    plan = run.plans[bool(mod.training)]
    kf = _f32c(known_feats)
    Plan.patch(plan.items["kf"], 0, kf)
    if run.c1:
        uf = _f32c(unknow_feats)
        Plan.patch(plan.items["uf"], 0, uf)
    out = torch.empty(run.B, net.mats[-1].n_out, run.n, dtype=torch.float32, device=kf.device)
    Plan.patch(plan.items["out"], 7, out)
    plan.run()
    if mod.training:
        net.batches_tracked += 1
    return out


class _FPFunction(torch.autograd.Function):
    """forward / backward of one feature-propagation module over its own activation set (held by the graph node until the backward
    has run, then recycled): several forwards of the same module may be in flight"""

    @staticmethod
    def forward(ctx, mod, idx, w, unknow_feats, known_feats, *params):
        rt = _fp_net(mod, known_feats.device)
        net = rt["net"]
        B, c2, m = known_feats.shape
        key = (B, idx.shape[1], m, c2)
        pool = net.free.setdefault(key, [])
        run = pool.pop() if pool else _FPRun(net, *key, known_feats.device, with_backward=True)
        out = _run_forward(mod, net, run, idx, w, unknow_feats, known_feats)
        ctx.run, ctx.net, ctx.key = run, net, key
        return out

    @staticmethod
    def backward(ctx, g_out):
        run, net = ctx.run, ctx.net
        B, n, m, c2 = ctx.key
        dev = g_out.device
        plan = run.backward_plan(net, int(bool(hip.deterministic())))
        g = _f32c(g_out)
        Plan.patch(plan.items["dout"], 0, g)
        g_uf = None
        if run.c1:
            g_uf = torch.empty(B, run.c1, n, dtype=torch.float32, device=dev)
            Plan.patch(plan.items["g_uf"], 1, g_uf)
        g_kf = torch.empty(B, c2, m, dtype=torch.float32, device=dev)
        Plan.patch(plan.items["g_kf"], plan.items["g_kf_arg"], g_kf)
        plan.run()
        # ONE copy of the call's parameter gradients; VIEWS of it go out (see sa_function._SAFunction.backward)
        gcopy = run.grad.clone()
        grads = []
        for p, o in zip(net.flat.params, net.flat.offsets[:-1]):
            o = int(o)
            grads.append(gcopy[o:o + p.numel()].view(p.shape) if p.requires_grad else None)
        net.free[ctx.key].append(run)                          # recycled: everything handed out above is the caller's
        ctx.run = None
        return (None, None, None, g_uf if ctx.needs_input_grad[3] else None, g_kf if ctx.needs_input_grad[4] else None) + tuple(grads)


def fp_module_forward(mod, idx, w, unknow_feats, known_feats):
    """the shared MLP of `mod` over [three_interpolate(known_feats, idx, w), unknow_feats] -> (B, mlp[-1], n); the caller
    (PointnetFPModule.forward) has checked fits() and that a call that needs gradients is in train mode"""
    dev = known_feats.device
    rt = _fp_net(mod, dev)
    net = rt["net"]
    params = net.flat.params
    feats = [t for t in (unknow_feats, known_feats) if t is not None]
    if torch.is_grad_enabled() and (any(t.requires_grad for t in feats) or any(p.requires_grad for p in params)):
        return _FPFunction.apply(mod, idx, w, unknow_feats, known_feats, *params)
    B, c2, m = known_feats.shape
    key = (B, idx.shape[1], m, c2)
    if key not in rt:
        rt[key] = _FPRun(net, *key, dev)
    return _run_forward(mod, net, rt[key], idx, w, unknow_feats, known_feats)
