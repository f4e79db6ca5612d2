"""The feature-propagation entry points of include/gaddpg.h section C.2 -- gad_fp_rows, gad_fp_rows_grad, gad_rows_act_out,
gad_rows_act_bwd_stats -- against the references of tests/fp_fused_reference.py (pinned on the CPU by
tests/test_fp_fused_reference.py), and PointnetFPModule(fused=True) against tests/fp_reference.fp_module_ref.

Yardsticks.  gad_fp_rows, gad_rows_act_out and the masked gradient G: bit-exact.  gad_fp_rows_grad: |hip - f64| <= (cnt + 1) *
2**-24 * sum |terms| per destination and exactly 0 where nothing lands (tests/test_gpu_fp_ops.py's, for the operator it restates).
The dbeta / dgamma sums: tests/test_gpu_layer_kernels._scaled_gate, error <= max(3 x the float32 reference's, its floor) relative
to max sum |terms|.  The module: err <= max(3 x err(float32 CPU reference), 2e-6) per tensor relative to max |float64 reference|,
the float64 reference evaluated on the GPU path's own neighbour indices (test_fp_module_against_float64's own).

Every buffer an entry point sees lives between guard bytes that must come back untouched; outputs start as NaN, so a column or an
element that must not be written comes back NaN; inputs must come back bit-identical.

Module routes (read off the predicates of csrc/gemm_fwd.hip; the last forward launch's family is asserted through
gad_last_kernel): skinny -- B * n <= 1024 rows (the B = 4 cases); tile -- 1200 rows, 16 outputs; wide -- B = 2, n = 1100 (2200
rows >= 2048), mlp [13, 64, 128]: 64 input channels (a multiple of 32), 128 outputs; streaming -- B = 2, n = 16 384 (32 768
rows), mlp [13, 64, 64]."""
import copy

import numpy as np
import pytest
import torch

from tests import fp_fused_reference as FF
from tests import fp_reference as F
from tests.test_gpu_layer_kernels import _padded, _scaled_gate
from tests.test_gpu_optim_kernels import Buf, _nan32, _same

pytestmark = pytest.mark.gpu

f32 = np.float32
OK, ERR_UNSUPPORTED = 0, -4
BIG = f32(1e30)


def _hip():
    from ga_ddpg_amd import hip
    return hip


def _rc(name, *a):
    hip = _hip()
    return getattr(hip.lib(), name)(*(hip._args(*a) + [hip.stream()]))


# ----------------------------------------------------------------------------- 1. gad_fp_rows
def _interp_inputs(B, C2, n, m, seed):
    rng = np.random.default_rng(seed)
    kf = rng.normal(size=(B, C2, m)).astype(f32)
    idx = rng.integers(0, m, size=(B, n, 3)).astype(np.int32)
    w = (rng.random((B, n, 3)) * 0.9 + 0.05).astype(f32)
    w /= w.sum(-1, keepdims=True, dtype=f32)
    idx[:, ::5] = idx[:, ::5, :1]                    # rows whose three indices coincide
    idx[:, 1::4, 2] = idx[:, 1::4, 0]                # ... and rows where two do
    w[:, ::7, 1] = 0                                 # rows with a zero weight
    return kf, idx, w


def _point_major(a):
    """(B, C, k) -> (B * k, C)"""
    return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(-1, a.shape[1])


# (known pitch - C2, row pitch - C2, column offset): 16-byte accesses where C2 is a multiple of 4 / 4-byte ones throughout
LAYOUTS = {"aligned": (4, 12, 4), "unaligned": (3, 9, 3)}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("C2", (1, 4, 5, 64, 67))
def test_fp_rows_bit_exact(C2, layout):
    hip = _hip()
    dk, dr, off = LAYOUTS[layout]
    for B in (1, 3):
        for n in (1, 63, 64, 65, 257):
            for m in (1, 3, 4, 257):
                kf, idx, w = _interp_inputs(B, C2, n, m, 1000 * C2 + 10 * n + m + B)
                kpm = _padded(_point_major(kf), C2 + dk, BIG)
                want = _nan32((B * n, C2 + dr))
                want[:, off:off + C2] = FF.fp_rows(kf, idx, w)
                bk, bi, bw, bo = Buf(kpm), Buf(idx), Buf(w), Buf(_nan32((B * n, C2 + dr)))
                hip.call("gad_fp_rows", bk.ptr, C2 + dk, bi.ptr, bw.ptr, B, n, m, C2, bo.ptr, C2 + dr, off)
                what = "fp_rows %s C2 %d B %d n %d m %d" % (layout, C2, B, n, m)
                _same(what + " (the other columns stay NaN)", bo.get("rows"), want)
                for b, a in ((bk, kpm), (bi, idx), (bw, w)):
                    _same(what + " input", b.get("input"), a)


# ----------------------------------------------------------------------------- 2. gad_fp_rows_grad
GRAD_CASES = [(3, 300, 130), (3, 300, 1), (1, 65, 4), (2, 257, 257)]


def _grad_inputs(B, C2, n, m, seed):
    rng = np.random.default_rng(seed)
    drows = rng.normal(size=(B * n, C2)).astype(f32)
    idx = rng.integers(0, max(m - 5, 1), size=(B, n, 3)).astype(np.int32)        # m > 5: the last five destinations get no entry
    idx[:, ::3, 1] = idx[:, ::3, 0]
    w = (rng.random((B, n, 3)) * 0.9 + 0.05).astype(f32)
    return drows, idx, w


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("C2", (1, 5, 64))
def test_fp_rows_grad_default_mode(C2, layout):
    hip = _hip()
    assert hip.get_option("deterministic") == 0
    dk, dr, off = LAYOUTS[layout]
    for B, n, m in GRAD_CASES:
        drows, idx, w = _grad_inputs(B, C2, n, m, 17 * C2 + m + n)
        din = _nan32((B * n, C2 + dr))                                             # a column outside the window would poison a sum
        din[:, off:off + C2] = drows
        gk0 = _nan32((B * m, C2 + dk))
        gk0[:, :C2] = 0                                                             # the caller cleared what is added to
        bd, bi, bw, bo = Buf(din), Buf(idx), Buf(w), Buf(gk0)
        hip.call("gad_fp_rows_grad", bd.ptr, C2 + dr, off, bi.ptr, bw.ptr, B, n, m, C2, bo.ptr, C2 + dk)
        out = bo.get("gknown_pm")
        what = "fp_rows_grad %s C2 %d B %d n %d m %d" % (layout, C2, B, n, m)
        _same(what + ": padding columns", out[:, C2:], gk0[:, C2:])
        got = np.ascontiguousarray(out[:, :C2])
        g64 = FF.fp_rows_grad(drows, idx, w, m, np.float64)
        cnt, mag = FF.fp_rows_grad_bound(drows, idx, w, m)
        bound = (cnt + 1) * 2.0 ** -24 * mag
        err = np.abs(got.astype(np.float64) - g64)
        print("GATE %s: max err / bound %.4f" % (what, float((err / np.where(bound > 0, bound, 1)).max())))
        assert not np.isnan(got).any() and (err <= bound).all(), what
        empty = np.broadcast_to(cnt == 0, got.shape)
        assert (m <= 5 or empty.any()) and (got[empty].view(np.uint32) == 0).all(), what + ": no entry must leave exactly +0"
        for b, a in ((bd, din), (bi, idx), (bw, w)):
            _same(what + " input", b.get("input"), a)


def test_fp_rows_grad_is_refused_in_deterministic_mode():
    hip = _hip()
    B, C2, n, m = 2, 5, 40, 9
    drows, idx, w = _grad_inputs(B, C2, n, m, 3)
    bd, bi, bw, bo = Buf(drows), Buf(idx), Buf(w), Buf(_nan32((B * m, C2)))
    hip.set_option("deterministic", 1)
    try:
        rc = _rc("gad_fp_rows_grad", bd.ptr, C2, 0, bi.ptr, bw.ptr, B, n, m, C2, bo.ptr, C2)
        msg = hip.lib().gad_last_error()
    finally:
        hip.set_option("deterministic", hip.get_option_default("deterministic"))
    assert rc == ERR_UNSUPPORTED and b"no ordered form" in msg
    _same("fp_rows_grad refused: the output is untouched", bo.get("gknown_pm"), _nan32((B * m, C2)))


# ----------------------------------------------------------------------------- 3. gad_rows_act_out
def _act_vectors(rng, C):
    scale = rng.normal(size=C).astype(f32)
    shift = (rng.normal(size=C) * 0.5).astype(f32)
    if C >= 16:                                      # scale == 0 with a live and with a dead activation
        scale[3], shift[3], scale[10], shift[10] = 0.0, 0.4, 0.0, -0.4
    mean = (rng.normal(size=C) * 0.3).astype(f32)
    istd = rng.uniform(0.5, 3.0, C).astype(f32)
    return scale, shift, mean, istd


@pytest.mark.parametrize("n", (1, 63, 65, 300))
@pytest.mark.parametrize("C", (1, 16, 33, 128))
def test_rows_act_out_bit_exact(C, n):
    hip = _hip()
    for B in (1, 3):
        rng = np.random.default_rng(3000 + 10 * C + n + B)
        z = (rng.normal(size=(B * n, C)) * 10.0 ** rng.uniform(-2, 2, (B * n, C))).astype(f32)
        scale, shift, _, _ = _act_vectors(rng, C)
        zin = _padded(z, C + 3, BIG)
        bz, bs, bt, bo = Buf(zin), Buf(scale), Buf(shift), Buf(_nan32((B, C, n)))
        hip.call("gad_rows_act_out", bz.ptr, C + 3, bs.ptr, bt.ptr, B, n, C, bo.ptr)
        what = "rows_act_out C %d n %d B %d" % (C, n, B)
        _same(what, bo.get("out"), FF.rows_act_out(z, scale, shift, B))
        for b, a in ((bz, zin), (bs, scale), (bt, shift)):
            _same(what + " input", b.get("input"), a)


# ----------------------------------------------------------------------------- 4. gad_rows_act_bwd_stats
ROWS = {1: (1, 1), 5: (1, 5), 257: (1, 257), 16500: (4, 4125)}        # rows -> (B, n); 16 500: more tiles than workgroups


def _bwd_data(C, rows):
    B, n = ROWS[rows]
    rng = np.random.default_rng(6000 + C + rows)
    z = rng.normal(size=(B * n, C)).astype(f32)
    dout = rng.normal(size=(B, C, n)).astype(f32)
    vec = _act_vectors(rng, C)
    r64 = FF.rows_act_bwd_stats(dout, z, *vec, np.float64)
    r32 = FF.rows_act_bwd_stats(dout, z, *vec, np.float32)
    return B, n, z, dout, vec, r64, r32


def _run_act_bwd(C, rows, data, what):
    hip = _hip()
    B, n, z, dout, vec, r64, r32 = data
    rng = np.random.default_rng(6100 + C + rows)
    pitch, gpitch, stride = C + 4, C + 3, C + 5
    pre_b, pre_g = rng.normal(size=4 * stride) + 3.0, rng.normal(size=4 * stride) - 3.0
    zin = _padded(z, pitch, BIG)
    bz, bd, bG, bdb, bdg = Buf(zin), Buf(dout), Buf(_nan32((B * n, gpitch))), Buf(pre_b), Buf(pre_g)
    bv = [Buf(a) for a in vec]
    hip.call("gad_rows_act_bwd_stats", bd.ptr, bz.ptr, pitch, bv[0].ptr, bv[1].ptr, bv[2].ptr, bv[3].ptr, B, n, C, bG.ptr, gpitch,
             bdb.ptr, bdg.ptr, stride)
    _same(what + ": G (the padding stays NaN)", bG.get("G"), _padded(r64["masked"], gpitch, f32(np.nan)))
    res = {}
    for name, b, pre, key in (("dbeta", bdb, pre_b, "abs_beta"), ("dgamma", bdg, pre_g, "abs_gamma")):
        acc = b.get(name)
        win = np.zeros(4 * stride, bool)
        for r in range(4):
            win[r * stride:r * stride + C] = True
        _same(what + ": %s outside the replica windows" % name, acc[~win], pre[~win])
        got = (acc - pre).reshape(4, stride)[:, :C].sum(0)
        _scaled_gate(what + ": " + name, got, r64[name], r32[name], r64[key].max())
        res[name] = acc
    for b, a in zip(bv + [bz, bd], list(vec) + [zin, dout]):
        _same(what + ": input", b.get(), a)
    if C >= 16:
        assert r64["live"][:, 3].all() and not r64["live"][:, 10].any()
    return res


@pytest.mark.parametrize("rows", sorted(ROWS))
@pytest.mark.parametrize("C", (1, 16, 33, 128, 768))
def test_rows_act_bwd_stats(C, rows):
    assert _hip().get_option("deterministic") == 0
    _run_act_bwd(C, rows, _bwd_data(C, rows), "rows_act_bwd_stats C %d rows %d" % (C, rows))


@pytest.mark.parametrize("C,rows", ((1, 257), (16, 16500), (33, 257), (128, 257), (768, 5), (768, 257)))
def test_rows_act_bwd_stats_deterministic_mode(C, rows):
    """the slot-plane form: the same gate, bit-identical on two calls, added to the pre-filled accumulators like the plain form"""
    hip = _hip()
    data = _bwd_data(C, rows)
    hip.set_option("deterministic", 1)
    try:
        a = _run_act_bwd(C, rows, data, "rows_act_bwd_stats deterministic C %d rows %d" % (C, rows))
        b = _run_act_bwd(C, rows, data, "rows_act_bwd_stats deterministic C %d rows %d (again)" % (C, rows))
    finally:
        hip.set_option("deterministic", hip.get_option_default("deterministic"))
    _same("deterministic dbeta: two calls", a["dbeta"], b["dbeta"])
    _same("deterministic dgamma: two calls", a["dgamma"], b["dgamma"])


# ----------------------------------------------------------------------------- 5. the module
def _rel_err(a, ref):
    ref = ref.double()
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


def _FP():
    from ga_ddpg_amd.pointnet2_ops.pointnet2_modules import PointnetFPModule
    return PointnetFPModule


def _spread_bn(mod):
    with torch.no_grad():                                                          # BatchNorm affine away from its (1, 0) start
        for x in mod.mlp:
            if isinstance(x, torch.nn.BatchNorm2d):
                x.weight.uniform_(0.5, 1.5)
                x.bias.uniform_(-0.3, 0.3)
                x.running_mean.uniform_(-0.2, 0.2)
                x.running_var.uniform_(0.5, 1.5)


def _inputs(branch, B, n, m, C1, C2, c_out, seed):
    g = torch.Generator().manual_seed(seed)
    unknown, known = torch.rand(B, n, 3, generator=g) * 0.4 + 0.1, torch.rand(B, m, 3, generator=g) * 0.4 + 0.1
    uf = None if branch == "no_unknow_feats" else torch.randn(B, C1, n, generator=g)
    kf = torch.randn(B, C2, m, generator=g)
    G = torch.randn(B, c_out, n, generator=g)
    return unknown, known, uf, kf, G


def _reference(cpu, unknown, known, uf, kf, G, idx, train=True, grads=True):
    """{dtype: {tensor name: value}} of fp_module_ref in float64 and float32 on the given indices: forward, feature and parameter
    gradients, and the running statistics after the call"""
    res = {}
    for dtype in (torch.float64, torch.float32):
        mlp = copy.deepcopy(cpu.mlp).to(dtype).train(train)
        r_uf = None if uf is None else uf.detach().clone().to(dtype).requires_grad_(grads)
        r_kf = kf.detach().clone().to(dtype).requires_grad_(grads)
        with torch.set_grad_enabled(grads):
            ry = F.fp_module_ref(mlp, unknown, known, r_uf, r_kf, idx, dtype)
        t = {"forward": ry.detach()}
        if grads:
            (ry * G.to(dtype)).sum().backward()
            t["known_feats.grad"] = r_kf.grad
            if r_uf is not None:
                t["unknow_feats.grad"] = r_uf.grad
            t.update({"mlp.%s.grad" % k: p.grad for k, p in mlp.named_parameters()})
        t.update({"mlp." + k: v for k, v in mlp.state_dict().items() if "running" in k})
        res[dtype] = t
    return res


def _fused_run(gpu, unknown, known, uf, kf, G, grads=True):
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils as pu
    d_uf = None if uf is None else uf.detach().cuda().requires_grad_(grads)
    d_kf = kf.detach().cuda().requires_grad_(grads)
    d_unknown, d_known = unknown.cuda(), known.cuda()
    gpu.zero_grad(set_to_none=True)
    with torch.set_grad_enabled(grads):
        y = gpu(d_unknown, d_known, d_uf, d_kf)
    kernel = _hip().lib().gad_last_kernel().decode()
    mine = {"forward": y.detach()}
    if grads:
        (y * G.cuda()).sum().backward()
        mine["known_feats.grad"] = d_kf.grad
        if d_uf is not None:
            mine["unknow_feats.grad"] = d_uf.grad
        mine.update({"mlp.%s.grad" % k: p.grad.clone() for k, p in gpu.mlp.named_parameters()})
    mine.update({"mlp." + k: v.clone() for k, v in gpu.mlp.state_dict().items() if "running" in k})
    idx = pu.three_nn(d_unknown, d_known)[1].cpu()                                 # the GPU path's own neighbours
    return mine, idx, kernel


def _gate(what, mine, res):
    assert set(mine) == set(res[torch.float64]), (sorted(mine), sorted(res[torch.float64]))
    bad = []
    for k in sorted(mine):
        ref = res[torch.float64][k]
        eh, e32 = _rel_err(mine[k], ref), _rel_err(res[torch.float32][k], ref)
        print("GATE fp_fused %s %-32s hip %.2e  f32 %.2e" % (what, k, eh, e32))
        if not eh <= max(3 * e32, 2e-6):
            bad.append((k, eh, e32))
    assert not bad, (what, bad)


def _check_module(what, branch, spec, B, n, m, C1, C2, route=None):
    hip = _hip()
    torch.manual_seed(100 + n + len(spec))
    cpu = _FP()(mlp=spec, bn=True)
    _spread_bn(cpu)
    unknown, known, uf, kf, G = _inputs(branch, B, n, m, C1, C2, spec[-1], 7 * n + m)
    res = None
    try:
        for split in (1, 0):
            hip.set_option("mfma_split", split)
            gpu = _FP()(mlp=spec, bn=True, fused=True).cuda()
            gpu.load_state_dict(cpu.state_dict(), strict=True)
            gpu.train()
            mine, idx, kernel = _fused_run(gpu, unknown, known, uf, kf, G)
            assert gpu.last_route == "fused" and mine["forward"].shape == (B, spec[-1], n)
            if route is not None:
                assert kernel.startswith(route) and (route != "gemm_fwd" or kernel == "gemm_fwd"), (kernel, route)
                if route in ("gemm_fwd(wide", "gemm_fwd(stream"):
                    assert kernel.endswith("split)") == bool(split), kernel
            if res is None:
                res = _reference(cpu, unknown, known, uf, kf, G, idx)
            assert len(mine) >= 2 + 5 * (len(spec) - 1)
            assert all(int(x.num_batches_tracked) == 1 for x in gpu.mlp if isinstance(x, torch.nn.BatchNorm2d))
            _gate("%s split %d" % (what, split), mine, res)
    finally:
        hip.set_option("mfma_split", hip.get_option_default("mfma_split"))


DEPTHS = {1: [16], 2: [32, 16], 3: [32, 32, 16]}


@pytest.mark.parametrize("n,m", ((64, 16), (130, 33)))
@pytest.mark.parametrize("depth", (1, 2, 3))
@pytest.mark.parametrize("branch", ("full", "no_unknow_feats"))
def test_fused_module_against_float64(branch, depth, n, m):
    """B = 4, C1 = 8, C2 = 5: 256 / 520 rows, the skinny kernels in every layer"""
    B, C1, C2 = 4, 8, 5
    spec = [C2 if branch == "no_unknow_feats" else C1 + C2] + DEPTHS[depth]
    _check_module("%s depth %d n %d m %d" % (branch, depth, n, m), branch, spec, B, n, m, C1, C2, route="gemm_fwd(skinny)")


@pytest.mark.parametrize("route,B,n,m,tail", (("gemm_fwd", 4, 300, 40, [32, 16]), ("gemm_fwd(wide", 2, 1100, 64, [64, 128]),
                                              ("gemm_fwd(stream", 2, 16384, 64, [64, 64])))
def test_fused_module_on_every_gemm_route(route, B, n, m, tail):
    """one case per route beyond the skinny one (the module docstring above names the predicates' terms)"""
    C1, C2 = 8, 5
    _check_module("route %s" % route, "full", [C1 + C2] + tail, B, n, m, C1, C2, route=route)


def test_fused_eval_forward_under_no_grad():
    B, n, m, C1, C2, spec = 4, 130, 33, 8, 5, [13, 32, 16]
    torch.manual_seed(5)
    cpu = _FP()(mlp=spec, bn=True)
    _spread_bn(cpu)
    unknown, known, uf, kf, G = _inputs("full", B, n, m, C1, C2, spec[-1], 11)
    gpu = _FP()(mlp=spec, bn=True, fused=True).cuda()
    gpu.load_state_dict(cpu.state_dict(), strict=True)
    gpu.eval()
    mine, idx, _ = _fused_run(gpu, unknown, known, uf, kf, G, grads=False)
    assert gpu.last_route == "fused"
    assert all(int(x.num_batches_tracked) == 0 for x in gpu.mlp if isinstance(x, torch.nn.BatchNorm2d))
    _gate("eval no_grad", mine, _reference(cpu, unknown, known, uf, kf, G, idx, train=False, grads=False))


@pytest.mark.parametrize("case", ("known_none", "bn_false", "eval_with_grad"))
def test_other_calls_take_the_composition(case):
    """bit-equal to a fused=False twin; both runs are made reproducible first (torch's convolution weight gradient and the default
    gradient of three_interpolate are not, see tests/test_gpu_three_nn_grid.py::test_fp_module_is_the_same_on_both_routes)"""
    hip = _hip()
    B, n, m, C1, C2, spec = 2, 70, 20, 8, 5, [13, 16, 8]
    torch.manual_seed(9)
    twins = [_FP()(mlp=spec, bn=case != "bn_false", fused=f).cuda() for f in (False, True)]
    twins[1].load_state_dict(twins[0].state_dict())
    unknown, known, uf, kf, G = _inputs("full", B, n, m, C1, C2, spec[-1], 13)
    if case == "known_none":
        known, kf = None, kf[:, :, :1].contiguous()
    torch_was = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
                 torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    outs = []
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
        for mod in twins:
            mod.train(case != "eval_with_grad")
            a, b = uf.cuda().requires_grad_(True), kf.cuda().requires_grad_(True)
            y = mod(unknown.cuda(), None if known is None else known.cuda(), a, b)
            (y * G.cuda()).sum().backward()
            assert mod.last_route == "composed"
            out = {"forward": y.detach(), "unknow_feats.grad": a.grad, "known_feats.grad": b.grad}
            out.update({k + ".grad": p.grad for k, p in mod.named_parameters()})
            out.update(mod.state_dict())
            outs.append({k: v.cpu().numpy() for k, v in out.items()})
    finally:
        torch.use_deterministic_algorithms(torch_was[0], warn_only=torch_was[1])
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = torch_was[2], torch_was[3]
        hip.sync_deterministic()
    assert set(outs[0]) == set(outs[1]) and "_gad_rt" not in twins[1].__dict__
    for k in sorted(outs[0]):
        _same("composed %s %s" % (case, k), outs[1][k], outs[0][k])


def test_optimizer_step_and_load_state_dict_reach_the_fused_path():
    B, n, m, C1, C2, spec = 4, 64, 16, 8, 5, [13, 32, 16]
    torch.manual_seed(21)
    cpu = _FP()(mlp=spec, bn=True)
    _spread_bn(cpu)
    unknown, known, uf, kf, G = _inputs("full", B, n, m, C1, C2, spec[-1], 17)
    gpu = _FP()(mlp=spec, bn=True, fused=True).cuda()
    gpu.load_state_dict(cpu.state_dict(), strict=True)
    gpu.train()
    keys = list(gpu.state_dict())
    opt = torch.optim.SGD(gpu.parameters(), lr=0.05)
    _fused_run(gpu, unknown, known, uf, kf, G)
    opt.step()                                                                      # the parameters are views of the flat buffer now
    assert list(gpu.state_dict()) == keys and gpu.last_route == "fused"
    cpu.load_state_dict({k: v.cpu() for k, v in gpu.state_dict().items()})          # the stepped weights, the advanced statistics
    assert all(int(x.num_batches_tracked) == 1 for x in cpu.mlp if isinstance(x, torch.nn.BatchNorm2d))
    mine, idx, _ = _fused_run(gpu, unknown, known, uf, kf, G)
    _gate("after an SGD step", mine, _reference(cpu, unknown, known, uf, kf, G, idx))
    assert all(int(x.num_batches_tracked) == 2 for x in gpu.mlp if isinstance(x, torch.nn.BatchNorm2d))
    # load_state_dict after fused calls: other weights, other statistics
    torch.manual_seed(22)
    other = _FP()(mlp=spec, bn=True)
    _spread_bn(other)
    gpu.load_state_dict(other.state_dict(), strict=True)
    gpu.to("cuda").train()
    mine, idx, _ = _fused_run(gpu, unknown, known, uf, kf, G)
    assert gpu.last_route == "fused"
    _gate("after load_state_dict", mine, _reference(other, unknown, known, uf, kf, G, idx))
    gpu.eval()
    mine, idx, _ = _fused_run(gpu, unknown, known, uf, kf, G, grads=False)
    other.load_state_dict({k: v.cpu() for k, v in gpu.state_dict().items()})
    _gate("eval after load_state_dict", mine, _reference(other, unknown, known, uf, kf, G, idx, train=False, grads=False))


def test_fused_module_is_bit_reproducible_with_the_library_option_alone():
    """hip.set_option("deterministic", 1), torch's switch untouched: two forward + backward runs of the fused module agree in every
    tensor bit for bit (the known-feature gradient takes gad_three_interpolate_grad's ordered form)"""
    hip = _hip()
    B, n, m, C1, C2, spec = 3, 300, 40, 8, 5, [13, 32, 16]
    torch.manual_seed(31)
    unknown, known, uf, kf, G = _inputs("full", B, n, m, C1, C2, spec[-1], 19)
    assert not torch.are_deterministic_algorithms_enabled()
    gpu = _FP()(mlp=spec, bn=True, fused=True).cuda().train()
    state = copy.deepcopy(gpu.state_dict())
    names, real = [], hip.call
    runs = []
    hip.set_option("deterministic", 1)
    try:
        for _ in range(2):
            gpu.load_state_dict(state)
            hip.call = lambda name, *args: (names.append(name), real(name, *args))[1]
            try:
                mine, _, _ = _fused_run(gpu, unknown, known, uf, kf, G)
            finally:
                hip.call = real
            assert gpu.last_route == "fused"
            runs.append({k: v.cpu().numpy() for k, v in mine.items()})
    finally:
        hip.call = real
        hip.set_option("deterministic", hip.get_option_default("deterministic"))
    assert "gad_three_nn" in names or "gad_three_nn_grid" in names                 # three_nn stays outside the plans
    assert "gad_three_interpolate" not in names
    assert set(runs[0]) == set(runs[1]) and len(runs[0]) >= 12
    for k in sorted(runs[0]):
        _same("deterministic fused module " + k, runs[1][k], runs[0][k])
