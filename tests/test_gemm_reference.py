"""tests/gemm_reference.py is the operation: every reference function, run in float64 on the CPU, against torch autograd on a small
composition of plain torch modules -- a gathered first layer (Linear without bias on [feat[pt] | xyz[pt] - ctr[grp] | action[smp]]),
train-mode BatchNorm over weighted rows, ReLU, then three Linear layers with bias and one extra input column that each read a
third of the channels.  No kernel, no GPU: the float64 gates of tests/test_gpu_gemm_f64.py stand on this."""
import pytest
import torch

from tests import gemm_reference as gr

RTOL = 1e-12


def _close(got, want, what):
    scale = float(want.abs().max()) + 1e-300
    err = float((got - want).abs().max())
    assert err <= RTOL * scale, "%s: max error %.3e of scale %.3e" % (what, err, scale)


def _setup():
    g = torch.Generator().manual_seed(7)
    f64 = dict(dtype=torch.float64)
    rows, npts, ngrp, gps, feat_c, act_c, C, H, Kp0 = 37, 11, 6, 2, 4, 6, 12, 5, 16
    c = C // 3
    Kp1 = 8
    t = dict(rows=rows, npts=npts, ngrp=ngrp, gps=gps, feat_c=feat_c, act_c=act_c, C=C, H=H, Kp0=Kp0, Kp1=Kp1, c=c)
    t["feat"] = torch.randn(npts, feat_c, generator=g, **f64).requires_grad_()
    t["src"] = torch.randn(npts, 3, generator=g, **f64)
    t["ctr"] = torch.randn(ngrp, 3, generator=g, **f64)
    t["action"] = torch.randn(ngrp // gps, act_c, generator=g, **f64).requires_grad_()
    t["row_pt"] = torch.randint(0, npts, (rows,), generator=g, dtype=torch.int32)
    t["row_grp"] = torch.sort(torch.randint(0, ngrp, (rows,), generator=g, dtype=torch.int32)).values
    t["row_w"] = torch.randint(1, 4, (rows,), generator=g).double()
    W0 = torch.randn(C, Kp0, generator=g, **f64)
    W0[:, feat_c + 3 + act_c:] = 0
    t["W0"] = W0.requires_grad_()
    t["gamma"] = (torch.rand(C, generator=g, **f64) + 0.5).requires_grad_()
    t["beta"] = (torch.randn(C, generator=g, **f64) * 0.3).requires_grad_()
    t["extra"] = torch.randn(rows, generator=g, **f64)
    # packed second layer: three groups (H, Kp1) = [c channels | extra | bias | 0 0]
    W1 = torch.randn(3, H, Kp1, generator=g, **f64)
    W1[:, :, c + 2:] = 0
    t["W1"] = W1.requires_grad_()
    t["G1"] = torch.randn(rows, 3 * H, generator=g, **f64)
    t["eps"] = 1e-5
    return t


def _autograd(t):
    """the composition in plain torch; the weighted batch statistics are those of the rows repeated row_w times"""
    pt, grp = t["row_pt"].long(), t["row_grp"].long()
    X0 = torch.cat([t["feat"][pt], t["src"][pt] - t["ctr"][grp], t["action"][grp // t["gps"]]], 1)
    z0 = torch.nn.functional.linear(X0, t["W0"][:, :X0.shape[1]])
    z0.retain_grad()
    w = t["row_w"][:, None]
    n = t["row_w"].sum()
    mean = (w * z0).sum(0) / n
    var = (w * z0 * z0).sum(0) / n - mean * mean
    istd = 1.0 / torch.sqrt(var + t["eps"])
    y0 = (z0 - mean) * istd * t["gamma"] + t["beta"]
    y0.retain_grad()
    x1 = torch.relu(y0)
    c = t["c"]
    outs = []
    for g in range(3):
        lin_in = torch.cat([x1[:, g * c:(g + 1) * c], t["extra"][:, None]], 1)
        outs.append(torch.nn.functional.linear(lin_in, t["W1"][g][:, :c + 1], t["W1"][g][:, c + 1]))
    z1 = torch.cat(outs, 1)
    (z1 * t["G1"]).sum().backward()
    return dict(z0=z0, z1=z1, mean=mean.detach(), istd=istd.detach(), n=n, y0=y0)


def test_reference_chain_matches_autograd():
    t = _setup()
    ag = _autograd(t)
    rows, C, H, c, Kp0, Kp1 = t["rows"], t["C"], t["H"], t["c"], t["Kp0"], t["Kp1"]
    d = lambda k: t[k].detach()
    # --- forward, gathered first layer
    A0 = gr.gather_operand(d("feat"), t["src"], t["ctr"], d("action"), t["row_pt"], t["row_grp"], t["gps"], Kp0)
    f0 = gr.forward([A0], d("W0"), Kp0, [0], [0], [C], C, k_used=t["feat_c"] + 3 + t["act_c"], row_w=t["row_w"])
    _close(f0["z"], ag["z0"].detach(), "gathered layer z")
    n = float(ag["n"])
    mean = f0["stat_sum"] / n
    var = f0["stat_sq"] / n - mean * mean
    istd = 1.0 / torch.sqrt(var + t["eps"])
    _close(mean, ag["mean"], "mean from stat_sum")
    _close(istd, ag["istd"], "istd from stat_sq")
    scale, shift = d("gamma") * istd, d("beta") - mean * d("gamma") * istd
    # --- forward, three groups with extra + bias column
    offs = [0, c, 2 * c]
    w_off = [g * H * Kp1 for g in range(3)]
    A1 = [gr.act_operand(f0["z"], o, c, Kp1, scale, shift, 1, t["extra"], c + 1) for o in offs]
    assert all(float(a[:, c + 2:].abs().max()) == 0.0 for a in A1)
    f1 = gr.forward(A1, d("W1"), Kp1, w_off, [0, H, 2 * H], [H] * 3, 3 * H, k_used=c + 2)
    _close(f1["z"], ag["z1"].detach(), "grouped layer z")
    # --- backward of the grouped layer: dW, dX with the previous layer's statistics
    dZ1 = gr.dz_operand(t["G1"])
    w1 = gr.dw(dZ1, A1, Kp1, c + 2, [0, H, 2 * H], w_off, [H] * 3, 3 * H * Kp1)
    _close(w1["dW"], t["W1"].grad.reshape(-1), "grouped layer dW")
    assert bool((w1["dW#mask"].view(3, H, Kp1)[:, :, c + 2:] == False).all()) and bool(w1["dW#mask"].view(3, H, Kp1)[:, :, :c + 2].all())
    prev = dict(zprev=f0["z"], scale=scale, shift=shift, mean=mean, istd=istd)
    x1 = gr.dx(dZ1, d("W1"), Kp1, c, [0, H, 2 * H], w_off, [H] * 3, offs, C, prev=prev, store_masked=1)
    _close(x1["gout"], ag["y0"].grad, "masked gradient of the BatchNorm output")
    _close(x1["dbeta"], t["beta"].grad, "dbeta")
    _close(x1["dgamma"], t["gamma"].grad, "dgamma")
    plain = gr.dx(dZ1, d("W1"), Kp1, c, [0, H, 2 * H], w_off, [H] * 3, offs, C, prev=prev, store_masked=0)
    dead = ag["y0"].detach() <= 0
    assert bool(dead.any()) and float(plain["gout"][dead].abs().min()) > 0 and float(x1["gout"][dead].abs().max()) == 0.0
    # --- BatchNorm backward folded into the first layer's dZ
    P = scale
    Q = scale * (x1["dbeta"] - mean * istd * x1["dgamma"]) / n
    S = scale * istd * x1["dgamma"] / n
    dZ0 = gr.dz_operand(x1["gout"], z=f0["z"], relu=1, premasked=1, P=P, Q=Q, S=S, row_w=t["row_w"])
    _close(dZ0, ag["z0"].grad, "dZ = P*g - w*(Q + S*z)")
    # (not premasked: the same from the unmasked gradient and this layer's own affine)
    dZ0b = gr.dz_operand(plain["gout"], z=f0["z"], scale=scale, shift=shift, relu=1, premasked=0, P=P, Q=Q, S=S, row_w=t["row_w"])
    _close(dZ0b, ag["z0"].grad, "dZ with the ReLU mask applied here")
    k0 = t["feat_c"] + 3 + t["act_c"]
    w0 = gr.dw(dZ0, [A0], Kp0, k0, [0], [0], [C], C * Kp0)
    _close(w0["dW"].view(C, Kp0), t["W0"].grad, "gathered layer dW")
    x0 = gr.dx(dZ0, d("W0"), Kp0, k0, [0], [0], [C], [0], k0)
    sc = gr.scatter(x0["gx"], x0["gout#abs"], t["row_pt"], t["row_grp"], t["gps"], t["feat_c"], t["act_c"], t["npts"],
                    t["ngrp"] // t["gps"])
    _close(sc["dfeat"], t["feat"].grad, "dfeat")
    _close(sc["daction"], t["action"].grad, "daction")


def test_pooled_routing_matches_max_pool_autograd():
    g = torch.Generator().manual_seed(3)
    rows, C, gsz = 24, 8, 4
    z = torch.randn(rows, C, generator=g, dtype=torch.float64).requires_grad_()
    s = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    t = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    dout = torch.randn(rows // gsz, C, generator=g, dtype=torch.float64)
    y = torch.relu(z * s + t).view(rows // gsz, gsz, C)
    pooled, arg = y.max(1)
    (pooled * dout).sum().backward()
    row_grp = torch.arange(rows, dtype=torch.int32) // gsz
    argmax = (arg + torch.arange(rows // gsz)[:, None] * gsz).to(torch.int32)
    dY = gr.route_pooled(argmax, dout, row_grp, rows)
    dZ = gr.dz_operand(dY, z=z.detach(), scale=s, shift=t, relu=1, premasked=0, P=s, Q=torch.zeros(C, dtype=torch.float64),
                       S=torch.zeros(C, dtype=torch.float64))
    _close(dZ, z.grad, "pooled arg-max routing")


def test_float32_operands_round_once():
    """float32 inputs: the activated operand is the correctly rounded fused multiply-add, not the twice-rounded product + sum"""
    z = torch.tensor([[1.0 + 2.0 ** -12, 3.0, -2.0, 0.5]], dtype=torch.float32)      # column 0: the product is a rounding tie, t breaks it
    s = torch.tensor([1.0 + 2.0 ** -12, 1.0, 1.0, 1.0], dtype=torch.float32)
    t = torch.tensor([2.0 ** -30, 0.0, 1.0, 0.0], dtype=torch.float32)
    A = gr.act_operand(z, 0, 4, 8, s, t, 1, torch.tensor([7.0]), 5)
    exact = (z.double() * s.double() + t.double()).clamp_min(0)
    assert torch.equal(A[:, :4], exact.float()) and A.dtype == torch.float32
    assert not torch.equal(A[:, :4], (z * s + t).clamp_min(0))          # (the two-rounding evaluation differs in column 0)
    assert A[0, 4] == 7.0 and A[0, 5] == 1.0 and float(A[0, 6:].abs().max()) == 0.0
    assert float(gr.abs_bound(A, torch.ones(2, 8))[0, 0]) == float(A.double().abs().sum())


@pytest.mark.parametrize("ctr", [True, False])
def test_gather_operand_layout(ctr):
    g = torch.Generator().manual_seed(1)
    feat, src, c3 = torch.randn(5, 4, generator=g), torch.randn(5, 3, generator=g), torch.randn(4, 3, generator=g)
    act = torch.randn(2, 6, generator=g)
    pt, grp = torch.tensor([4, 0, 2], dtype=torch.int32), torch.tensor([0, 1, 3], dtype=torch.int32)
    A = gr.gather_operand(feat, src, c3 if ctr else None, act, pt, grp, 2, 16)
    assert torch.equal(A[:, :4], feat[pt.long()])
    assert torch.equal(A[:, 4:7], src[pt.long()] - c3[grp.long()] if ctr else src[pt.long()])
    assert torch.equal(A[:, 7:13], act[torch.tensor([0, 0, 1])]) and float(A[:, 13:].abs().max()) == 0.0


def test_recomputed_operand_matches_autograd():
    """mode 2: the gathered first layer, its affine + ReLU and the second layer as one chain of plain torch modules; the float32
    slack of the recomputed operand covers a float32 evaluation of it"""
    t = _setup()
    d = lambda k: t[k].detach()
    g = torch.Generator().manual_seed(11)
    C, Kp0, k0 = t["C"], t["Kp0"], t["feat_c"] + 3 + t["act_c"]
    scale = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    W = torch.randn(7, C, generator=g, dtype=torch.float64)
    pt, grp = t["row_pt"].long(), t["row_grp"].long()
    X0 = torch.cat([d("feat")[pt], t["src"][pt] - t["ctr"][grp], d("action")[grp // t["gps"]]], 1)
    lin0, lin1 = torch.nn.Linear(k0, C, bias=False, dtype=torch.float64), torch.nn.Linear(C, 7, bias=False, dtype=torch.float64)
    with torch.no_grad():
        lin0.weight.copy_(d("W0")[:, :k0])
        lin1.weight.copy_(W)
        want_A = torch.relu(lin0(X0) * scale + shift)
        want_z = lin1(want_A)
    G = gr.gather_operand(d("feat"), t["src"], t["ctr"], d("action"), t["row_pt"], t["row_grp"], t["gps"], Kp0)
    ro = gr.recomputed_operand(G, d("W0"), k0, scale, shift, 1)
    _close(ro["A"], want_A, "recomputed operand")
    _close(ro["z1"], lin0(X0).detach(), "recomputed first layer")
    f = gr.forward([ro["A"]], W, C, [0], [0], [7], 7, row_w=t["row_w"])
    _close(f["z"], want_z, "second layer on the recomputed operand")
    # float32 inputs: A stays the float64 chain; a float32 evaluation of the same chain lies inside A#slack
    f32 = lambda x: x.float()
    G32 = gr.gather_operand(f32(d("feat")), f32(t["src"]), f32(t["ctr"]), f32(d("action")), t["row_pt"], t["row_grp"], t["gps"], Kp0)
    r32 = gr.recomputed_operand(G32, f32(d("W0")), k0, f32(scale), f32(shift), 1)
    assert r32["A"].dtype == torch.float64
    a32 = torch.relu((G32[:, :k0] @ f32(d("W0"))[:, :k0].t()) * f32(scale) + f32(shift))
    err = (a32.double() - r32["A"]).abs()
    assert bool((err <= r32["A#slack"]).all()) and float(err.max()) > 0.0


def test_backward_pair_of_one_layer_matches_autograd():
    """the fused backward (gad_gemm_bwd) is dx() and dw() on ONE layer: dW's input rows are the activation the dX side's previous-layer
    block describes, act_operand(zprev, prev scale, prev shift).  x = relu(gamma * (zprev - mean) * istd + beta), z = x W^T."""
    g = torch.Generator().manual_seed(5)
    f64 = dict(dtype=torch.float64, generator=g)
    rows, K, N = 29, 8, 12
    zprev = torch.randn(rows, K, **f64)
    mean, istd = torch.randn(K, **f64) * 0.1, torch.rand(K, **f64) + 0.5
    gamma, beta = (torch.rand(K, **f64) + 0.5).requires_grad_(), (torch.randn(K, **f64) * 0.3).requires_grad_()
    W = torch.randn(N, K, **f64).requires_grad_()
    dZ = torch.randn(rows, N, **f64)
    y = (zprev - mean) * istd * gamma + beta
    y.retain_grad()
    (torch.nn.functional.linear(torch.relu(y), W) * dZ).sum().backward()
    scale, shift = (gamma * istd).detach(), (beta - mean * gamma * istd).detach()
    A = gr.act_operand(zprev, 0, K, K, scale, shift, 1)
    prev = dict(zprev=zprev, scale=scale, shift=shift, mean=mean, istd=istd)
    x = gr.dx(dZ, W.detach(), K, K, [0], [0], [N], [0], K, prev=prev, store_masked=1)
    w = gr.dw(dZ, [A], K, K, [0], [0], [N], N * K)
    _close(x["gout"], y.grad, "fused backward: masked input gradient")
    _close(x["dbeta"], beta.grad, "fused backward: dbeta")
    _close(x["dgamma"], gamma.grad, "fused backward: dgamma")
    _close(w["dW"].view(N, K), W.grad, "fused backward: dW")
