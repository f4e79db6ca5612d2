"""tests/optim_reference.py is the right reference: in float64 it reproduces torch.optim.Adam + clip_grad_norm_ and the
reference project's target-update formulas; and the error bounds tests/test_gpu_optim_kernels.py derives from it hold."""
import math

import numpy as np
import torch

from tests import optim_reference as R

HPS = ({"lr": 3e-4, "betas": R.BETAS, "eps": 1e-5, "weight_decay": 1e-5},
       {"lr": 1e-3, "betas": R.BETAS, "eps": 1e-8, "weight_decay": 0.0})


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


def test_adam_and_clip_equal_torch_float64():
    rng = np.random.default_rng(0)
    n = 1237
    for hp in HPS:
        for clip_max in (None, 0.5):
            p0 = rng.normal(size=n) * 0.1
            ref_p = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
            opt = torch.optim.Adam([ref_p], lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"],
                                   foreach=False)
            p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
            for t in range(1, 8):
                g = rng.normal(size=n) * (10.0 if t % 2 == 0 else 0.003)          # clipped / not clipped in turn
                ref_p.grad = torch.tensor(g, dtype=torch.float64)
                if clip_max is not None:
                    torch.nn.utils.clip_grad_norm_([ref_p], clip_max)
                opt.step()
                p, g1, m, v = R.adam_step(p, g, m, v, hp, t, np.float64, sumsq=float((g * g).sum()), clip_max=clip_max)
                st = opt.state[ref_p]
                assert _rel(p, ref_p.detach().numpy()) <= 1e-12, (hp, clip_max, t)
                assert _rel(m, st["exp_avg"].numpy()) <= 1e-12, (hp, clip_max, t)
                assert _rel(v, st["exp_avg_sq"].numpy()) <= 1e-12, (hp, clip_max, t)
                assert _rel(g1, ref_p.grad.numpy()) <= 1e-12, (hp, clip_max, t)     # .grad scaled in place
                assert int(st["step"]) == t


def test_inactive_elements_are_parameters_without_grad():
    """active == 0 stands for a parameter whose .grad is None: torch skips it entirely"""
    rng = np.random.default_rng(1)
    a, b = torch.nn.Parameter(torch.tensor(rng.normal(size=5))), torch.nn.Parameter(torch.tensor(rng.normal(size=7)))
    opt = torch.optim.Adam([a, b], lr=1e-3, weight_decay=1e-2, foreach=False)
    a.grad = torch.tensor(rng.normal(size=5))
    p0 = np.concatenate([a.detach().numpy(), b.detach().numpy()])
    g = np.concatenate([a.grad.numpy(), rng.normal(size=7)])
    opt.step()
    act = np.r_[np.ones(5, np.uint8), np.zeros(7, np.uint8)]
    hp = {"lr": 1e-3, "betas": R.BETAS, "eps": 1e-8, "weight_decay": 1e-2}
    p, g1, m, v = R.adam_step(p0, g, np.zeros(12), np.zeros(12), hp, 1, np.float64, active=act)
    assert _rel(p[:5], a.detach().numpy()) <= 1e-12
    assert (p[5:] == b.detach().numpy()).all() and (m[5:] == 0).all() and (v[5:] == 0).all() and (g1 == g).all()


def test_target_update_equals_reference_formulas():
    """soft_update / half_soft_update / half_hard_update (core/utils.py) on a module named linear1 .. linear6"""
    torch.manual_seed(0)

    def net():
        m = torch.nn.Module()
        for k in range(1, 7):
            setattr(m, "linear%d" % k, torch.nn.Linear(3 + k, 2 + k).double())
        m.other = torch.nn.Linear(2, 2).double()
        return m
    src, tgt = net(), net()
    tau = 0.05
    flat = lambda m: np.concatenate([p.detach().numpy().ravel() for _, p in m.named_parameters()])
    sel = R.sel_from_names([(n, p.numel()) for n, p in tgt.named_parameters()])
    assert set(sel.tolist()) == {0, 1, 2}
    s0, t0 = flat(src), flat(tgt)
    pairs = lambda: zip(tgt.named_parameters(), src.named_parameters())
    for hard in (0, 1):
        want = R.target_update(t0, s0, sel, tau, hard, np.float64)
        for (tn, tp), (_, sp) in pairs():                                  # half_soft_update
            if tn[:7] in ["linear1", "linear2", "linear3"]:
                tp.data.copy_(tp.data * (1.0 - tau) + sp.data * tau)
        if hard:
            for (tn, tp), (_, sp) in pairs():                              # half_hard_update
                if tn[:7] in ["linear4", "linear5", "linear6"]:
                    tp.data.copy_(sp.data)
        assert (flat(tgt) == want).all()
        untouched = (sel == 0) | ((sel == 2) & (hard == 0))
        assert (want[untouched] == t0[untouched]).all()
        t0 = flat(tgt)
    # soft_update: every parameter
    want = R.target_update(t0, s0, None, tau, 0, np.float64)
    for (tn, tp), (_, sp) in pairs():
        tp.data.copy_(tp.data * (1.0 - tau) + sp.data * tau)
    assert (flat(tgt) == want).all()


def test_absmax_is_the_reference_statistic():
    """module_max_param / module_max_gradient: max |.|, 0 for a parameter without a gradient, NaN if any element is NaN"""
    x = np.array([0.5, -3.0, 2.0, -0.0], np.float32)
    assert R.absmax(x) == np.float32(3.0) and R.absmax(x, include=[1, 0, 1, 1]) == np.float32(2.0)
    assert R.absmax(x[:0]) == 0 and R.absmax(x, include=[0, 0, 0, 0]) == 0
    y = x.copy(); y[2] = np.nan
    assert np.isnan(R.absmax(y)) and np.isnan(float(torch.abs(torch.tensor(y)).max())) and np.isnan(np.amax([1.0, np.nan]))


def test_float32_conversion_is_round_to_nearest_even():
    """the bit-exact expectations of gad_grad_from_arena rest on numpy's float64 -> float32 being RNE, overflowing to inf
    and rounding into the subnormals"""
    u = 2.0 ** -23                                         # ulp of float32 in [1, 2)
    cases = [(1.0 + u / 2, 1.0), (1.0 + 3 * u / 2, 1.0 + 2 * u), (1.0 + u / 2 + 2.0 ** -52, 1.0 + u),
             (-(1.0 + u / 2), -1.0), (2.0 - u / 2, 2.0), (float(np.finfo(np.float32).max) * (1 + 2.0 ** -25), float(np.finfo(np.float32).max)),
             (float(np.finfo(np.float32).max) + 2.0 ** 103, np.inf), (2.0 ** -150, 0.0), (2.0 ** -149 * 1.5, 2.0 ** -148),
             (2.0 ** -149 * 2.5, 2.0 ** -148), (-0.0, -0.0)]
    for x, want in cases:
        got = R.f32(x)
        assert got == np.float32(want) and np.signbit(got) == np.signbit(want), (x, got, want)
        assert float(torch.tensor(x, dtype=torch.float64).float()) == float(got)
    g = R.grad_from_arena(np.array([1.0 + u / 2, 7.0]), np.array([1, -1, 0]), np.array([1, 2, 3], np.float32), True)
    assert g.tolist() == [8.0, 2.0, 4.0]


def test_sumsq_bound_holds_for_float64_sums_in_any_order():
    rng = np.random.default_rng(2)
    for n in (1, 5, 4099):
        g = (rng.normal(size=n) * 10.0 ** rng.uniform(-15, 15, n)).astype(np.float32)
        exact = R.sumsq_exact(g)
        sq = g.astype(np.float64) ** 2
        for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
            s = 0.0
            for x in sq[order]:
                s += x
            assert abs(s - exact) <= R.sumsq_bound(n, exact)
        assert abs(float(np.sum(sq)) - exact) <= R.sumsq_bound(n, exact)            # pairwise tree


def test_clip_branch_is_stable_a_stated_distance_from_the_tie():
    """the GPU cases put the norm (1 +- 1e-3) x max either side of the tie norm == max; float32 and float64 then take the same
    branch (the float32 norm is within 2**-23 relative of the float64 one, the added 1e-6 is 2e-6 relative at max = 0.5)"""
    for rel, clipped in ((-1e-3, False), (1e-3, True), (-0.5, False), (3.0, True)):
        norm = 0.5 * (1.0 + rel)
        c64, c32 = R.clip_coef(norm * norm, 0.5, np.float64), R.clip_coef(norm * norm, 0.5, np.float32)
        assert (c64 < 1.0) == clipped and (c32 < 1.0) == clipped
    assert R.clip_coef(0.0, 0.5, np.float32) == 1.0 and R.clip_coef(0.0, 0.5, np.float64) == 1.0
    assert R.clip_coef(4.0, None, np.float32) is None


def test_one_minus_beta_formed_in_float32_is_measurably_wrong():
    """why the hyper block carries 1 - beta: float32(1) - float32(0.999) is 1.29e-5 off float32(0.001)"""
    b2 = np.float32(0.999)
    assert abs(float(np.float32(1) - b2) / 0.001 - 1) > 1.2e-5
    assert abs(float(np.float32(1.0 - 0.999)) / 0.001 - 1) < 6e-8
    h = R.hyper_block({"lr": 1e-3, "betas": R.BETAS, "eps": 1e-8, "weight_decay": 0.0}, 3)
    assert h.dtype == np.float32 and h[8] == np.float32(1.0 - 0.9) and h[9] == np.float32(1.0 - 0.999)
    assert h[5] == np.float32(1 - 0.9 ** 3) and h[6] == np.float32(math.sqrt(1 - 0.999 ** 3))


def test_bn_running_update_equals_batchnorm1d_float64():
    rng = np.random.default_rng(3)
    C, eps, mom = 5, 1e-5, 0.1
    for n in (2, 48):
        bn = torch.nn.BatchNorm1d(C, eps=eps, momentum=mom).double()
        bn.running_mean.copy_(torch.tensor(rng.normal(size=C))); bn.running_var.copy_(torch.tensor(rng.uniform(0.5, 2, C)))
        rm0, rv0 = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
        x = torch.tensor(rng.normal(size=(n, C)) * 3)
        bn.train()(x)
        mean, var = x.mean(0).numpy(), x.var(0, unbiased=False).numpy()
        rm, rv = R.bn_running_update(mean, 1 / np.sqrt(var + eps), np.full(C, n), eps, mom, rm0, rv0, np.float64)
        assert _rel(rm, bn.running_mean.numpy()) <= 1e-12 and _rel(rv, bn.running_var.numpy()) <= 1e-10
        sc, sh = R.bn_eval_affine(bn.weight.detach().numpy(), bn.bias.detach().numpy(), rm, rv, eps, np.float64)
        y = bn.eval()(x).detach().numpy()
        assert _rel(x.numpy() * sc + sh, y) <= 1e-12
    rm, rv = R.bn_running_update([1.0], [1 / math.sqrt(4.0 + eps)], [1], eps, mom, [0.0], [1.0], np.float64)
    assert abs(rv[0] - (0.9 + 0.1 * 4.0)) < 1e-12                      # count 1: the biased variance


def test_group_mask_and_injection_shapes():
    rng = np.random.default_rng(4)
    m = R.group_mask(rng, 64)
    assert (m[0:4] == 0).all() and m[4:8].tolist() == [1, 0, 1, 0]
    m2p, pn = R.injection(rng, 1000)
    live = m2p[m2p >= 0]
    assert len(set(live.tolist())) == len(live) and live.max() < pn and 10 < (m2p < 0).sum() < 120 and pn >= 1500
