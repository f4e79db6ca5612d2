"""The feature-propagation operators of include/gaddpg.h section A -- gad_three_nn, gad_three_interpolate,
gad_three_interpolate_grad (default and deterministic) -- their pointnet2_utils wrappers and PointnetFPModule, on small
adversarial shapes against the plain references of tests/fp_reference.py (pinned on the CPU by tests/test_fp_reference.py).

Yardsticks.  three_nn (indices and the float32 bits of the squared distances), three_interpolate and the deterministic gradient:
bit-exact.  The default (atomic) gradient: |hip - f64| <= (cnt + 1) * 2**-24 * sum |terms| per destination -- one rounding per
product and at most cnt per sum -- and exactly 0 where no entry lands.  PointnetFPModule: err(hip) <= max(3 x err(float32 CPU
reference), 2e-6) per tensor, errors relative to max |float64 reference|, the float64 reference evaluated on the GPU path's own
neighbour indices.

Every buffer the entry points see lives between 64 guard bytes on both sides that must come back untouched; pure outputs start
as NaN (indices as -1); inputs must come back bit-identical.  All inputs come from seeded generators, of ordinary magnitude."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import fp_reference as F
from tests.test_gpu_optim_kernels import Buf, _nan32, _same

pytestmark = pytest.mark.gpu

f32 = np.float32
TNN_TILE = 1024                 # known points per LDS tile of three_nn_kernel
GPG_NT = 8192                   # destinations per LDS tile of the ordered scatter kernel
NN_B, NN_N = (1, 3), (1, 63, 64, 65, 257)
NN_M = (1, 2, 3, 4, 255, 256, 257, TNN_TILE + 1)
CLOUDS = ("random", "lattice", "duplicates", "coincident", "contraction")


def _hip():
    from ga_ddpg_amd import hip
    return hip


def _pu():
    from ga_ddpg_amd.pointnet2_ops import pointnet2_utils
    return pointnet2_utils


# ----------------------------------------------------------------------------- 1. gad_three_nn
def _fused_sqdist(u, known):
    """the distance as a compiler that contracts dy*dy + dx*dx into one FMA would form it (what the kernel must NOT compute)"""
    d = (u[None] - known).astype(f32)
    xx, zz = (d[:, 0] * d[:, 0]).astype(f32), (d[:, 2] * d[:, 2]).astype(f32)
    return ((d[:, 1].astype(np.float64) ** 2 + xx.astype(np.float64)).astype(f32) + zz).astype(f32)


@functools.lru_cache(maxsize=None)
def _contraction_sensitive_case(seed, m):
    """a query point c and m known points: p, whose squared distance differs in the last bit between the pinned evaluation and
    the one with dy*dy + dx*dx fused (found as tests/test_gpu_ops.py::_contraction_sensitive_case finds it for the ball query),
    q on the x axis through c at exactly the FUSED distance of p (dy = dz = 0: both evaluations agree on q), everything else far
    away.  p and q are ordered so that the tie the fused evaluation sees goes to the point the pinned evaluation ranks second:
    the nearest neighbour differs between the two.  m == 1: p alone -- the distance bits differ."""
    rng = np.random.default_rng(seed)
    while True:
        c = rng.random(3).astype(f32)
        pts = (c + (rng.random((4096, 3)).astype(f32) - f32(0.5)) * f32(0.2)).astype(f32)
        pinned, fused = F.sqdist32(c[None, None], pts[None])[0, 0], _fused_sqdist(c, pts)
        for i in np.nonzero(pinned != fused)[0]:
            t = fused[i]
            r = f32(np.sqrt(np.float64(t)))
            for dx in (r, np.nextafter(r, f32(0)), np.nextafter(r, f32(4))):
                for qx in (f32(c[0] - dx), f32(c[0] + dx)):
                    if f32(f32(c[0] - qx) * f32(c[0] - qx)) != t:
                        continue
                    known = (c + f32(1.0) + rng.random((m, 3)).astype(f32)).astype(f32)          # d >= 3: far away
                    p, q = pts[i], np.array([qx, c[1], c[2]], f32)
                    if m == 1:
                        known[0] = p
                    elif pinned[i] < fused[i]:      # pinned: p first.  fused: a tie, which the lower index (q) wins
                        known[0], known[m - 1] = q, p
                    else:                           # pinned: q first.  fused: a tie, which the lower index (p) wins
                        known[0], known[m - 1] = p, q
                    return c, known


def _nn_clouds(kind, B, n, m, seed):
    rng = np.random.default_rng(seed)
    unknown = (rng.random((B, n, 3)) * 0.1 + 0.2).astype(f32)
    known = (rng.random((B, m, 3)) * 0.1 + 0.2).astype(f32)
    if kind == "lattice":
        unknown = rng.integers(0, 6, size=(B, n, 3)).astype(f32) * f32(0.125) + f32(0.25)
        known = rng.integers(0, 6, size=(B, m, 3)).astype(f32) * f32(0.125) + f32(0.25)
    elif kind == "duplicates":
        known[:, m // 2:] = known[:, :m - m // 2]
    elif kind == "coincident":
        unknown = known[:, np.arange(n) % m].copy()
    elif kind == "contraction":
        for b in range(B):
            unknown[b, 0], known[b] = _contraction_sensitive_case(seed * 7 + b, m)
    return unknown, known


@pytest.mark.parametrize("m", NN_M)
@pytest.mark.parametrize("kind", CLOUDS)
def test_three_nn_bit_exact(kind, m):
    hip = _hip()
    for B in NN_B:
        for n in NN_N:
            unknown, known = _nn_clouds(kind, B, n, m, 1000 * m + 10 * n + B)
            want_d, want_i = F.three_nn_ref(unknown, known)
            if kind == "contraction":                # the case does tell the two evaluations apart, on the CPU
                for b in range(B):
                    fd = _fused_sqdist(unknown[b, 0], known[b])
                    fi = np.argsort(fd, kind="stable")[:3]
                    assert fd[fi[0]].tobytes() != want_d[b, 0, 0].tobytes() or fi[0] != want_i[b, 0, 0]
                    if m >= 2:
                        assert fi[0] != want_i[b, 0, 0] and {int(fi[0]), int(want_i[b, 0, 0])} == {0, m - 1}
            bu, bk = Buf(unknown), Buf(known)
            bd, bi = Buf(_nan32((B, n, 3))), Buf(np.full((B, n, 3), -1, np.int32))
            hip.call("gad_three_nn", bu.ptr, bk.ptr, B, n, m, bd.ptr, bi.ptr)
            got_d, got_i = bd.get("dist2"), bi.get("idx")
            what = "three_nn %s B %d n %d m %d" % (kind, B, n, m)
            _same(what + " idx", got_i, want_i)
            _same(what + " dist2", got_d, want_d)
            if m < 3:
                assert (got_i[:, :, m:] == 0).all() and np.isposinf(got_d[:, :, m:]).all()
            _same(what + " unknown", bu.get("unknown"), unknown)
            _same(what + " known", bk.get("known"), known)


# ----------------------------------------------------------------------------- 2. gad_three_interpolate
def _interp_inputs(B, C, n, m, seed):
    rng = np.random.default_rng(seed)
    pts = rng.normal(size=(B, C, m)).astype(f32)
    idx = rng.integers(0, m, size=(B, n, 3)).astype(np.int32)
    w = (rng.random((B, n, 3)) * 0.9 + 0.05).astype(f32)
    w /= w.sum(-1, keepdims=True, dtype=f32)
    idx[:, ::5] = idx[:, ::5, :1]                    # rows whose three indices coincide
    w[:, ::7, 1] = 0                                 # rows with a zero weight
    return pts, idx, w


@pytest.mark.parametrize("C_", (1, 3, 64, 65))
def test_three_interpolate_bit_exact(C_):
    hip = _hip()
    B = 3
    for n in (1, 65, 300):
        for m in (1, 3, 130):
            pts, idx, w = _interp_inputs(B, C_, n, m, 31 * C_ + 7 * n + m)
            bp, bi, bw, bo = Buf(pts), Buf(idx), Buf(w), Buf(_nan32((B, C_, n)))
            hip.call("gad_three_interpolate", bp.ptr, bi.ptr, bw.ptr, B, C_, m, n, bo.ptr)
            what = "three_interpolate C %d n %d m %d" % (C_, n, m)
            _same(what, bo.get("out"), F.three_interpolate_ref(pts, idx, w))
            for b, a in ((bp, pts), (bi, idx), (bw, w)):
                _same(what + " input", b.get("input"), a)


# ----------------------------------------------------------------------------- 3. / 4. gad_three_interpolate_grad
def _grad_inputs(B, C, n, m, seed):
    rng = np.random.default_rng(seed)
    go = rng.normal(size=(B, C, n)).astype(f32)
    idx = rng.integers(0, max(m - 5, 1), size=(B, n, 3)).astype(np.int32)        # m > 5: the last five destinations get no entry
    w = (rng.random((B, n, 3)) * 0.9 + 0.05).astype(f32)
    return go, idx, w


TIG_NT = 8192                   # floats of grad_points a workgroup of the default-mode gradient kernel keeps in LDS
GRAD_SHAPES = [(3, C_, 300, m) for C_ in (1, 65) for m in (1, 130)]
# the default mode's routes: rows of up to TIG_NT destinations accumulate in LDS, 8 / 3 / 1 channels per workgroup with a ragged last
# chunk; longer rows take global atomics behind a clearing pass
GRAD_ROUTES = [(2, 5, 40, 2049), (2, 3, 40, TIG_NT), (2, 3, 40, TIG_NT + 1)]


@pytest.mark.parametrize("B,C_,n,m", GRAD_SHAPES + GRAD_ROUTES)
def test_three_interpolate_grad_default_mode(B, C_, n, m):
    hip = _hip()
    assert hip.get_option("deterministic") == 0
    go, idx, w = _grad_inputs(B, C_, n, m, 17 * C_ + m)
    if m > 130:
        idx[:, ::2, 1] = idx[:, ::2, 0]                                            # collisions in the long rows as well
        idx[:, :, 2] = m - 6 - (idx[:, :, 2] % 3)                                  # ... and entries at their far end
    bg, bi, bw, bo = Buf(go), Buf(idx), Buf(w), Buf(_nan32((B, C_, m)))
    hip.call("gad_three_interpolate_grad", bg.ptr, bi.ptr, bw.ptr, B, C_, n, m, bo.ptr)
    got = bo.get("grad_points")
    g64 = F.three_interpolate_grad_ref(go, idx, w, m, np.float64)
    cnt, mag = F.three_interpolate_grad_bound(go, idx, w, m)
    bound = (cnt[:, None, :] + 1) * 2.0 ** -24 * mag
    err = np.abs(got.astype(np.float64) - g64)
    print("GATE three_interpolate_grad C %d m %d: max err / bound %.4f" % (C_, m, float((err / np.where(bound > 0, bound, 1)).max())))
    assert (err <= bound).all()
    empty = np.broadcast_to(cnt[:, None, :] == 0, got.shape)
    assert (m == 1 or empty.any()) and (got[empty].view(np.uint32) == 0).all()   # no entry: exactly +0
    if m == 1:
        assert (cnt == 3 * n).all()                                                # all 900 entries of a row collide
    for b, a in ((bg, go), (bi, idx), (bw, w)):
        _same("three_interpolate_grad input", b.get("input"), a)


@pytest.mark.parametrize("B,C_,n,m", GRAD_SHAPES + [(2, 2, 5, GPG_NT + 1), (1, 3, 700, 2 * GPG_NT + 3)])
def test_three_interpolate_grad_deterministic_mode(B, C_, n, m):
    hip = _hip()
    go, idx, w = _grad_inputs(B, C_, n, m, 19 * C_ + m)
    if m > GPG_NT:
        idx[:, :, 2] = m - 1 - (idx[:, :, 2] % 7)                                  # entries in the last LDS tile as well
    want = F.three_interpolate_grad_ref(go, idx, w, m)
    bg, bi, bw = Buf(go), Buf(idx), Buf(w)
    outs = [Buf(_nan32((B, C_, m))) for _ in range(4)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    was = hip.get_option_default("deterministic")
    try:
        hip.set_option("deterministic", 1)
        for o in outs[:2]:                                                         # two calls on one stream
            hip.call("gad_three_interpolate_grad", bg.ptr, bi.ptr, bw.ptr, B, C_, n, m, o.ptr)
        torch.cuda.synchronize()
        for o, s in zip(outs[2:], streams):                                        # two streams at once
            with torch.cuda.stream(s):
                hip.call("gad_three_interpolate_grad", bg.ptr, bi.ptr, bw.ptr, B, C_, n, m, o.ptr)
        torch.cuda.synchronize()
    finally:
        hip.set_option("deterministic", was)
    for k, o in enumerate(outs):
        _same("deterministic three_interpolate_grad C %d m %d, call %d" % (C_, m, k), o.get("grad_points"), want)
    for b, a in ((bg, go), (bi, idx), (bw, w)):
        _same("three_interpolate_grad input", b.get("input"), a)


# ----------------------------------------------------------------------------- 5. the autograd functions
def test_three_interpolate_autograd_and_three_nn_outputs():
    hip, pu = _hip(), _pu()
    B, C_, n, m = 2, 6, 70, 20
    pts, idx, w = _interp_inputs(B, C_, n, m, 3)
    g = np.random.default_rng(4).normal(size=(B, C_, n)).astype(f32)
    feats = torch.from_numpy(pts).cuda().requires_grad_(True)
    ti, tw, tg = torch.from_numpy(idx).cuda(), torch.from_numpy(w).cuda().requires_grad_(True), torch.from_numpy(g).cuda()
    was = hip.get_option_default("deterministic")
    try:
        hip.set_option("deterministic", 1)                                         # (the atomic form is not bit-reproducible)
        out = pu.three_interpolate(feats, ti, tw)
        out.backward(tg.transpose(1, 2).contiguous().transpose(1, 2))              # a non-contiguous grad_out
        direct = torch.full((B, C_, m), float("nan"), device="cuda")
        hip.call("gad_three_interpolate_grad", tg, ti, tw.detach(), B, C_, n, m, direct)
    finally:
        hip.set_option("deterministic", was)
    _same("three_interpolate forward", out.detach().cpu().numpy(), F.three_interpolate_ref(pts, idx, w))
    _same("features.grad", feats.grad.cpu().numpy(), direct.cpu().numpy())
    _same("features.grad vs reference", feats.grad.cpu().numpy(), F.three_interpolate_grad_ref(g, idx, w, m))
    assert tw.grad is None and out.requires_grad
    # default mode: the same gradient to summation order
    feats.grad = None
    pu.three_interpolate(feats, ti, tw).backward(tg)
    cnt, mag = F.three_interpolate_grad_bound(g, idx, w, m)
    err = np.abs(feats.grad.double().cpu().numpy() - F.three_interpolate_grad_ref(g, idx, w, m, np.float64))
    assert (err <= (cnt[:, None, :] + 1) * 2.0 ** -24 * mag).all()
    # three_nn: nothing differentiable comes out, whatever goes in
    unknown, known = _nn_clouds("random", B, n, m, 5)
    tu, tk = torch.from_numpy(unknown).cuda().requires_grad_(True), torch.from_numpy(known).cuda().requires_grad_(True)
    dist, nidx = pu.three_nn(tu, tk)
    assert not dist.requires_grad and not nidx.requires_grad and nidx.dtype == torch.int32 and dist.dtype == torch.float32
    want_d, want_i = F.three_nn_ref(unknown, known)
    _same("three_nn idx", nidx.cpu().numpy(), want_i)
    _same("three_nn dist", dist.cpu().numpy(), np.sqrt(want_d))
    # the checks of the other functions of the file: CUDA, contiguous, float32
    with pytest.raises(RuntimeError):
        pu.three_nn(tu.detach().cpu(), tk.detach())
    with pytest.raises(RuntimeError):
        pu.three_nn(tu.detach().double(), tk.detach().double())
    with pytest.raises(RuntimeError):
        pu.three_interpolate(feats.detach().transpose(1, 2), ti, tw.detach())
    with pytest.raises(RuntimeError):
        pu.three_interpolate(feats.detach(), ti.long(), tw.detach())


# ----------------------------------------------------------------------------- 6. PointnetFPModule
def _rel_err(a, ref):
    ref = ref.double()
    return float((a.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("n,m", ((64, 16), (130, 33)))
@pytest.mark.parametrize("branch", ("full", "no_unknow_feats", "no_known"))
def test_fp_module_against_float64(branch, n, m):
    import copy
    from ga_ddpg_amd.pointnet2_ops.pointnet2_modules import PointnetFPModule
    pu = _pu()
    B, C1, C2 = 4, 8, 5
    spec = [C2 if branch == "no_unknow_feats" else C1 + C2, 32, 16]
    torch.manual_seed(100 + n)
    cpu = PointnetFPModule(mlp=spec, bn=True)
    with torch.no_grad():                                                          # BatchNorm affine away from its (1, 0) start
        for mod in cpu.mlp:
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
    unknown, known = torch.rand(B, n, 3) * 0.4 + 0.1, torch.rand(B, m, 3) * 0.4 + 0.1
    uf = None if branch == "no_unknow_feats" else torch.randn(B, C1, n)
    kf = torch.randn(B, C2, 1 if branch == "no_known" else m)
    G = torch.randn(B, spec[-1], n)
    if branch == "no_known":
        known = None

    gpu = PointnetFPModule(mlp=spec, bn=True).cuda()
    gpu.load_state_dict(cpu.state_dict(), strict=True)                             # a CPU checkpoint of the same constructor
    gpu.train()
    d_uf = None if uf is None else uf.cuda().requires_grad_(True)
    d_kf = kf.cuda().requires_grad_(True)
    d_unknown, d_known = unknown.cuda(), None if known is None else known.cuda()
    y = gpu(d_unknown, d_known, d_uf, d_kf)
    assert y.shape == (B, spec[-1], n)
    (y * G.cuda()).sum().backward()
    idx = None if known is None else pu.three_nn(d_unknown, d_known)[1].cpu()     # the GPU path's own neighbours

    res = {}
    for dtype in (torch.float64, torch.float32):
        mlp = copy.deepcopy(cpu.mlp).to(dtype).train()
        r_uf = None if uf is None else uf.to(dtype).requires_grad_(True)
        r_kf = kf.to(dtype).requires_grad_(True)
        ry = F.fp_module_ref(mlp, unknown, known, r_uf, r_kf, idx, dtype)
        (ry * G.to(dtype)).sum().backward()
        t = {"forward": ry.detach(), "known_feats.grad": r_kf.grad}
        if r_uf is not None:
            t["unknow_feats.grad"] = r_uf.grad
        t.update({"mlp.%s.grad" % k: p.grad for k, p in mlp.named_parameters()})
        res[dtype] = t
    mine = {"forward": y.detach(), "known_feats.grad": d_kf.grad}
    if d_uf is not None:
        mine["unknow_feats.grad"] = d_uf.grad
    mine.update({"mlp.%s.grad" % k: p.grad for k, p in gpu.mlp.named_parameters()})
    assert set(mine) == set(res[torch.float64]) and len(mine) >= 8
    bad = []
    for k in sorted(mine):
        ref = res[torch.float64][k]
        eh, e32 = _rel_err(mine[k], ref), _rel_err(res[torch.float32][k], ref)
        print("GATE fp_module %s n %d m %d %-24s hip %.2e  f32 %.2e" % (branch, n, m, k, eh, e32))
        if not eh <= max(3 * e32, 2e-6):
            bad.append((k, eh, e32))
    assert not bad, bad


# ----------------------------------------------------------------------------- 7. plan replay
@pytest.mark.parametrize("det", (0, 1))
def test_fp_entry_points_replay_from_a_plan(det):
    """the three entry points as items of one gad_plan (three_nn feeding the indices of the other two), one gad_plan_run:
    bit-equal to the direct calls.  Default mode: indices are left as three_nn gives them for the forward, while the gradient
    takes collision-free indices (atomic adds onto one destination are not ordered); deterministic mode: colliding ones."""
    from ga_ddpg_amd import engine
    hip = _hip()
    L = hip.lib()
    B, C_, n, m = 2, 5, 70, 260
    unknown, known = _nn_clouds("random", B, n, m, 9)
    pts, gidx, w = _interp_inputs(B, C_, n, m, 10)
    if not det:
        gidx = np.stack([np.random.default_rng(b).permutation(m)[:n * 3].reshape(n, 3) for b in range(B)]).astype(np.int32)
    go = np.random.default_rng(11).normal(size=(B, C_, n)).astype(f32)
    bu, bk, bp, bw, bg, bgi = Buf(unknown), Buf(known), Buf(pts), Buf(w), Buf(go), Buf(gidx)

    def outputs():
        return (Buf(_nan32((B, n, 3))), Buf(np.full((B, n, 3), -1, np.int32)), Buf(_nan32((B, C_, n))), Buf(_nan32((B, C_, m))))

    def calls(d2, ix, out, gp):
        return (("gad_three_nn", (bu.ptr, bk.ptr, B, n, m, d2.ptr, ix.ptr)),
                ("gad_three_interpolate", (bp.ptr, ix.ptr, bw.ptr, B, C_, m, n, out.ptr)),
                ("gad_three_interpolate_grad", (bg.ptr, bgi.ptr, bw.ptr, B, C_, n, m, gp.ptr)))

    direct, replayed = outputs(), outputs()
    was = hip.get_option_default("deterministic")
    h = C.c_void_p()
    try:
        hip.set_option("deterministic", det)
        for name, a in calls(*direct):
            hip.call(name, *a)
        hip.check(L.gad_plan_create(C.byref(h)), "gad_plan_create")
        for name, a in calls(*replayed):
            words, kinds = engine._pack_words(hip._args(*a))
            k = len(words)
            rc = L.gad_plan_add_call(h, name.encode(), (C.c_uint64 * k)(*words), (C.c_uint8 * k)(*kinds), k, 0)
            assert rc >= 0, L.gad_last_error()
        assert L.gad_plan_size(h) == 3
        table = (C.c_void_p * 1)(torch.cuda.current_stream().cuda_stream)
        hip.check(L.gad_plan_run(h, table, 1, 0, -1), "gad_plan_run")
        torch.cuda.synchronize()
    finally:
        hip.set_option("deterministic", was)
        L.gad_plan_destroy(h)
    want_d, want_i = F.three_nn_ref(unknown, known)
    _same("plan three_nn idx vs reference", replayed[1].get("idx"), want_i)
    for what, a, b in zip(("dist2", "idx", "out", "grad_points"), direct, replayed):
        _same("plan replay " + what, b.get(what), a.get(what))
