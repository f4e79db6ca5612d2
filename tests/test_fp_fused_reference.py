"""Pins tests/fp_fused_reference.py on the CPU: the four references chained the way ga_ddpg_amd.fp_function chains the kernels --
rows = [fp_rows | skip features], z = rows W^T, train-mode BatchNorm (layer_reference.bn_finalize), rows_act_out, then back:
rows_act_bwd_stats, dZ = P dY - (Q + S z) (layer_reference.bn_bwd_coef), drows = dZ W, fp_rows_grad -- against torch float64
autograd of cat -> conv -> BatchNorm(train) -> ReLU on a tiny case.  The references round to float32 where the kernels do, so the
agreement asked for is 1e-5 of the largest reference value, per tensor."""
import numpy as np
import torch

from tests import fp_fused_reference as FF
from tests import fp_reference as F
from tests import layer_reference as L

f32 = np.float32
EPS = 1e-5


def _case(seed=0, B=2, n=7, m=5, C1=3, C2=4, Cout=6):
    rng = np.random.default_rng(seed)
    kf = rng.normal(size=(B, C2, m)).astype(f32)
    uf = rng.normal(size=(B, C1, n)).astype(f32)
    idx = rng.integers(0, m, size=(B, n, 3)).astype(np.int32)
    idx[:, ::3] = idx[:, ::3, :1]                                   # rows whose three indices coincide
    w = (rng.random((B, n, 3)) * 0.9 + 0.05).astype(f32)
    w /= w.sum(-1, keepdims=True, dtype=f32)
    W = (rng.normal(size=(Cout, C1 + C2)) * 0.5).astype(f32)
    gamma, beta = rng.uniform(0.5, 1.5, Cout).astype(f32), rng.uniform(-0.3, 0.3, Cout).astype(f32)
    dout = rng.normal(size=(B, Cout, n)).astype(f32)
    return kf, uf, idx, w, W, gamma, beta, dout


def _rel(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def test_fp_rows_is_three_interpolate_transposed():
    kf, uf, idx, w, *_ = _case(1)
    rows = FF.fp_rows(kf, idx, w)
    B, n = idx.shape[:2]
    want = F.three_interpolate_ref(kf, idx, w)
    assert rows.dtype == f32 and rows.shape == (B * n, kf.shape[1])
    for b in range(B):
        for i in range(n):
            assert (rows[b * n + i].view(np.uint32) == want[b, :, i].view(np.uint32)).all()


def test_chain_against_torch_float64_autograd():
    kf, uf, idx, w, W, gamma, beta, dout = _case(2)
    B, C2, m = kf.shape
    n, C1, Cout = uf.shape[2], uf.shape[1], W.shape[0]
    R = B * n
    # ---- torch float64: three_interpolate as gathers, cat, 1x1 convolution, BatchNorm (train), ReLU
    t_kf = torch.from_numpy(kf).double().requires_grad_(True)
    t_uf = torch.from_numpy(uf).double().requires_grad_(True)
    t_W = torch.from_numpy(W).double().requires_grad_(True)
    t_g = torch.from_numpy(gamma).double().requires_grad_(True)
    t_b = torch.from_numpy(beta).double().requires_grad_(True)
    ix = torch.from_numpy(idx).long()
    f = torch.gather(t_kf.unsqueeze(2).expand(B, C2, n, m), 3, ix.unsqueeze(1).expand(B, C2, n, 3))
    x = torch.cat([(f * torch.from_numpy(w).double().unsqueeze(1)).sum(-1), t_uf], dim=1)
    z = torch.nn.functional.conv2d(x.unsqueeze(-1), t_W.view(Cout, C1 + C2, 1, 1))
    y = torch.relu(torch.nn.functional.batch_norm(z, None, None, t_g, t_b, True, 0.1, EPS)).squeeze(-1)
    (y * torch.from_numpy(dout).double()).sum().backward()

    # ---- the references, chained as the kernels are
    rows = np.concatenate([FF.fp_rows(kf, idx, w), np.ascontiguousarray(uf.transpose(0, 2, 1)).reshape(R, C1)], axis=1)
    zr = (rows.astype(np.float64) @ W.astype(np.float64).T).astype(f32)
    stride = Cout + 1
    s1, s2 = np.zeros(4 * stride), np.zeros(4 * stride)
    s1[:Cout], s2[:Cout] = zr.astype(np.float64).sum(0), (zr.astype(np.float64) ** 2).sum(0)
    bn = L.bn_finalize(s1, s2, stride, R, gamma, beta, EPS, 0.1)
    scale, shift, mean, istd = (bn[k].astype(f32) for k in ("scale", "shift", "mean", "istd"))
    out = FF.rows_act_out(zr, scale, shift, B)
    assert out.shape == (B, Cout, n) and _rel(out, y.detach().numpy()) <= 1e-5
    st = FF.rows_act_bwd_stats(dout, zr, scale, shift, mean, istd, np.float64)
    assert st["live"].any() and not st["live"].all()
    assert _rel(st["dbeta"], t_b.grad.numpy()) <= 1e-5 and _rel(st["dgamma"], t_g.grad.numpy()) <= 1e-5
    db, dg = np.zeros(4 * stride), np.zeros(4 * stride)
    db[:Cout], dg[:Cout] = st["dbeta"], st["dgamma"]
    co = L.bn_bwd_coef(db, dg, stride, scale, mean, istd, R)
    dz = co["P"].astype(np.float64)[None] * st["masked"] - (co["Q"][None] + co["S"][None] * zr.astype(np.float64))
    assert _rel(dz.T @ rows.astype(np.float64), t_W.grad.numpy()) <= 1e-5
    drows = (dz @ W.astype(np.float64)).astype(f32)
    g_uf = drows[:, C2:].reshape(B, n, C1).transpose(0, 2, 1)
    assert _rel(g_uf, t_uf.grad.numpy()) <= 1e-5
    gk = FF.fp_rows_grad(np.ascontiguousarray(drows[:, :C2]), idx, w, m).reshape(B, m, C2).transpose(0, 2, 1)
    assert _rel(gk, t_kf.grad.numpy()) <= 1e-5
    cnt, mag = FF.fp_rows_grad_bound(np.ascontiguousarray(drows[:, :C2]), idx, w, m)
    assert cnt.shape == (B * m, 1) and cnt.sum() == 3 * R and mag.shape == (B * m, C2) and (mag >= np.abs(gk.transpose(0, 2, 1).reshape(B * m, C2)) - 1e-12).all()


def test_rows_act_bwd_stats_is_pool_bwd_stats_with_one_row_groups():
    rng = np.random.default_rng(3)
    B, C, n = 2, 5, 9
    z = rng.normal(size=(B * n, C)).astype(f32)
    dout = rng.normal(size=(B, C, n)).astype(f32)
    scale, shift = rng.normal(size=C).astype(f32), (rng.normal(size=C) * 0.5).astype(f32)
    scale[1], shift[1], scale[3], shift[3] = 0.0, 0.4, 0.0, -0.4      # scale == 0: every row live / every row dead
    mean, istd = (rng.normal(size=C) * 0.3).astype(f32), rng.uniform(0.5, 3, C).astype(f32)
    r = FF.rows_act_bwd_stats(dout, z, scale, shift, mean, istd, np.float64)
    live = L.fmaf32(z, scale[None], shift[None]) > 0
    assert live[:, 1].all() and not live[:, 3].any()
    G = np.where(live, dout.transpose(0, 2, 1).reshape(B * n, C), 0).astype(f32)
    assert (r["masked"].view(np.uint32) == G.view(np.uint32)).all()
    assert np.allclose(r["dbeta"], G.astype(np.float64).sum(0), rtol=0, atol=1e-12)
    xhat = (z.astype(np.float64) - mean) * istd
    assert np.allclose(r["dgamma"], (G * xhat).sum(0), rtol=0, atol=1e-12)
    want = L.affine_act(z, scale, shift, 1)
    got = FF.rows_act_out(z, scale, shift, B)
    for b in range(B):
        assert (got[b].T.view(np.uint32) == want[b * n:(b + 1) * n].view(np.uint32)).all()
