"""tests/layer_reference.py is the right reference: its fused multiply-add equals libm's fmaf (halfway cases included), its
max-pool and arg-max equal torch.nn.functional.max_pool2d, its BatchNorm equals torch.native_batch_norm in float64, and its
backward formulas equal torch autograd through BatchNorm -> ReLU -> max-pool."""
import ctypes
import ctypes.util

import numpy as np
import torch

from tests import layer_reference as L


def _libm_fmaf():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return lambda z, s, t: np.array([m.fmaf(float(a), float(b), float(c)) for a, b, c in zip(z, s, t)], np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_fmaf32_equals_libm_fmaf():
    fmaf = _libm_fmaf()
    f = np.float32
    u = 2.0 ** -23
    # hand-built: the exact result lies just beside a float32 halfway point, closer than float64 resolves -- (double)z * s + t
    # lands ON the halfway point and the second rounding (ties to even) goes the wrong way
    hand = [(2.0 ** -24 * (1 + u), 1 - u, 1 + u),          # 1 + 2**-23 + 2**-24 - 2**-70: down to 1 + 2**-23 (naive: 1 + 2**-22)
            (2.0 ** -24 * (1 + u), -(1 - u), -(1 + u)),
            (2.0 ** -24 * (1 + u), -(1 - u), 1 + 2 * u),     # 1 + 2**-22 - 2**-24 + 2**-70: up to 1 + 2**-22 (naive: ties to even too)
            (2.0 ** -24 * (1 + u), 1 - u, 1.0),              # 1 + 2**-24 - 2**-70: down to 1
            (2.0 ** -24 * (1 + u), 1 + u, 1.0),              # 1 + 2**-24 + 2**-46 + ...: up
            (2.0 ** -24 * (1 + u), -(1 - u), 1 + u),         # 1 + 2**-23 - 2**-24 + 2**-70: up to 1 + 2**-23 (naive: down to 1)
            (1 + u, 1 + u, -(1 + 2 * u)),                    # exact cancellation down to 2**-46
            (3.0, 1.0 / 3.0, -1.0), (0.0, 5.0, 0.0), (1e-30, 1e-30, 1.0), (1e20, 1e20, -1e38), (1.5, 0.0, -2.5)]
    z, s, t = (np.array([h[k] for h in hand], np.float64).astype(f) for k in range(3))
    for k in (0, 2, 3, 5):
        assert float(z[k]) == hand[k][0] and float(s[k]) == hand[k][1] and float(t[k]) == hand[k][2]      # all representable
    with np.errstate(over="ignore"):
        naive = (z.astype(np.float64) * s.astype(np.float64) + t.astype(np.float64)).astype(f)
        want = fmaf(z, s, t)
        assert (_bits(naive) != _bits(want)).sum() >= 3, "the hand-built cases do not separate fmaf from the double-rounded form"
        for sc in (1.0, 2.0 ** 40, 2.0 ** -60):                                        # + scaled: the same mantissas elsewhere
            zz, tt = (z * f(sc)).astype(f), (t * f(sc)).astype(f)
            assert (_bits(L.fmaf32(zz, s, tt)) == _bits(fmaf(zz, s, tt))).all()
    rng = np.random.default_rng(0)
    n = 200000
    z = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f)
    s = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f)
    t = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f)
    t[::7] = (-z[::7] * s[::7]).astype(f)                                              # heavy cancellation
    z[::11] = np.round(z[::11] * 8) / 8
    s[::13] = 0.0
    # random halfway neighbours: t = a float32, z * s a tiny fraction of its last place either side of half a unit
    base = (1 + rng.integers(0, 1 << 23, n // 4) * u).astype(f)
    z[:n // 4] = (2.0 ** -24 * (1 + rng.integers(0, 4, n // 4) * u)).astype(f)
    s[:n // 4] = (1 + rng.integers(-3, 4, n // 4) * u * 0.5).astype(f)
    t[:n // 4] = base * rng.choice(np.array([1, -1], f), n // 4)
    got, want = L.fmaf32(z, s, t), fmaf(z, s, t)
    assert (_bits(got) == _bits(want)).all(), int((_bits(got) != _bits(want)).sum())
    naive = (z.astype(np.float64) * s.astype(np.float64) + t.astype(np.float64)).astype(f)
    print("double-rounded form differs from fmaf on %d of %d" % ((_bits(naive) != _bits(want)).sum(), n))


def _padded(z, off, fill):
    """(rows, C) + CSR -> (1, C, G, nsample) with `fill` in the unused slots (torch's layout for max_pool2d)"""
    sizes = np.diff(off)
    G, ns, C = len(sizes), int(sizes.max()), z.shape[1]
    x = np.full((1, C, G, ns), fill, np.float64)
    for g in range(G):
        x[0, :, g, :sizes[g]] = z[off[g]:off[g + 1]].T
    return x, ns


def test_segment_pool_equals_torch_max_pool2d_first_of_ties():
    rng = np.random.default_rng(1)
    for C, with_affine in ((8, True), (5, False), (16, True)):
        off = L.groups(rng, [1, 2, 3, 7, 8, 9, 31, 1, 4, 16, 5])
        rows = int(off[-1])
        z = (np.round(rng.uniform(-2, 2, (rows, C)) * 8) / 8 + 0.0).astype(np.float32)          # exact ties in most groups
        z[off[3]:off[4]] = -np.abs(z[off[3]:off[4]]) - 0.125                                   # a group with nothing above 0
        sc = rng.choice(np.array([0.5, -0.25, 0.0, 2.0, -1.0], np.float32), C) if with_affine else None
        sh = rng.choice(np.array([0.25, -0.5, 0.125], np.float32), C) if with_affine else None
        out, arg = L.segment_pool(z, off, sc, sh)
        y = L.affine_act(z, sc, sh, 1).astype(np.float64)
        x, ns = _padded(y, off, -1.0)                                                         # (the activations are >= 0)
        ref, idx = torch.nn.functional.max_pool2d(torch.from_numpy(x), kernel_size=[1, ns], return_indices=True)
        ref, idx = ref[0, :, :, 0].numpy().T, idx[0, :, :, 0].numpy().T                        # (G, C); idx = g * ns + slot
        slot = idx - np.arange(len(off) - 1)[:, None] * ns
        assert (out.astype(np.float64) == ref).all()
        assert (arg == off[:-1, None] + slot).all()
        ties = sum(int(((y[off[g]:off[g + 1]] == ref[g]).sum(axis=0) > 1).sum()) for g in range(len(off) - 1))
        assert ties > 10
        assert (arg[3] == off[3]).all() or with_affine                                       # all <= 0: the group's first row
    # the tie rule itself
    y = np.array([[0.0], [1.0], [1.0], [0.5]], np.float32)
    out, arg = L.segment_pool(y, np.array([0, 4]))
    assert out[0, 0] == 1.0 and arg[0, 0] == 1
    # groups without rows: 0 and the group's offset; the others as if the empty ones were not there
    out, arg = L.segment_pool(y, np.array([0, 0, 1, 1, 1, 4, 4]))
    assert (out[:, 0] == [0, 0, 0, 0, 1, 0]).all() and (arg[:, 0] == [0, 0, 1, 1, 1, 4]).all()
    assert (L.pool_keys(y, np.array([0, 0, 4, 4]), np.ones(1, np.float32))[:, 0] == [0, (0xbf800000 << 32) | (0xffffffff - 1), 0]).all()


def test_pool_keys_and_finalize_against_plain_argmax():
    rng = np.random.default_rng(2)
    C = 12
    off = L.groups(rng, [1, 2, 3, 7, 8, 9, 31, 1, 4, 16])
    rows = int(off[-1])
    z = (np.round(rng.uniform(-2, 2, (rows, C)) * 8) / 8 + 0.0).astype(np.float32)
    gamma = rng.choice(np.array([1.0, -1.0, 0.0, 0.5, -2.0], np.float32), C)
    gamma[:3] = (1.0, -1.0, 0.0)
    keys = L.pool_keys(z, off, gamma)
    sgn = np.where(gamma < 0, -1.0, 1.0)
    for g in range(len(off) - 1):
        v = z[off[g]:off[g + 1]].astype(np.float64) * sgn
        r = off[g] + np.argmax(v, axis=0)                                                    # numpy: the first maximum
        assert ((0xffffffff - (keys[g] & np.uint64(0xffffffff)).astype(np.int64)) == r).all()
        assert (L.pool_unord((keys[g] >> np.uint64(32)).astype(np.uint32)).astype(np.float64) == v.max(axis=0)).all()
    # order-preserving bits: unsigned order == float order, and the inverse
    f = np.sort(np.concatenate([rng.normal(size=500) * 10.0 ** rng.uniform(-30, 30, 500), [0.0, -0.0, np.inf, -np.inf]]).astype(np.float32))
    o = L.pool_ord(f)
    assert (np.diff(o.astype(np.int64)) >= 0).all() and (L.pool_unord(o).view(np.uint32) == f.view(np.uint32)).all()
    # finish: scale = gamma * a power of two (the sign of gamma), shifts of both signs
    scale = (gamma * rng.choice(np.array([0.5, 1.0, 4.0], np.float32), C)).astype(np.float32)
    shift = rng.choice(np.array([0.25, -0.5], np.float32), C)
    out, arg, zmax = L.pool_finalize(keys, off, scale, shift, gamma)
    out2, arg2 = L.segment_pool(z, off, scale, shift)
    assert (out.view(np.uint32) == out2.view(np.uint32)).all()                              # a rounded fma is monotone
    assert (arg == arg2).all()                                                               # (distinct raw values: distinct activations)
    dead = (scale == 0) | (out <= 0)
    assert (arg[dead] == np.broadcast_to(off[:-1, None], arg.shape)[dead]).all() and dead.any() and (~dead).any()
    assert (zmax[:, gamma == 0] == np.maximum.reduceat(z, off[:-1], axis=0)[:, gamma == 0]).all()
    o0, a0, z0 = L.pool_finalize(np.zeros((2, C), np.uint64), np.array([3, 5, 9]), scale, shift, gamma)      # key 0: no row
    assert (o0 == 0).all() and (z0 == 0).all() and (a0 == np.array([[3], [5]])).all()


def _rows_and_sums(rng, rows, C, count):
    """float32 rows with integer weights that sum to `count`, and the float64 sums over the weighted rows"""
    w = np.ones(rows, np.int64)
    w[0] += count - rows
    z = (rng.normal(size=(rows, C)) * rng.uniform(0.1, 3.0, C) + rng.normal(size=C) * 2).astype(np.float32)
    z64 = z.astype(np.float64)
    return z, w, (w[:, None] * z64).sum(axis=0), (w[:, None] * z64 * z64).sum(axis=0)


def test_bn_finalize_equals_torch_native_batch_norm():
    rng = np.random.default_rng(3)
    eps, mom = 1e-5, 0.1
    for C, rows, count, stride in ((7, 40, 40, 7), (5, 30, 75, 10), (3, 2, 2, 3), (4, 1, 1, 9)):
        z, w, s1, s2 = _rows_and_sums(rng, rows, C, count)
        gamma, beta = rng.normal(size=C).astype(np.float32), rng.normal(size=C).astype(np.float32)
        gamma[0] = 0.0
        rm0, rv0 = rng.normal(size=C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
        ref = L.bn_finalize(L.replicate(s1, stride, C, rng, 7.0), L.replicate(s2, stride, C, rng, 7.0), stride, count, gamma,
                            beta, eps, mom, rm0, rv0)
        x = torch.from_numpy(np.repeat(z.astype(np.float64), w, axis=0))
        e64, m64 = float(np.float32(eps)), float(np.float32(mom))
        if count > 1:
            rm, rv = torch.from_numpy(rm0.astype(np.float64)), torch.from_numpy(rv0.astype(np.float64))
            y, save_mean, save_istd = torch.native_batch_norm(x, torch.from_numpy(gamma.astype(np.float64)),
                                                              torch.from_numpy(beta.astype(np.float64)), rm, rv, True, m64, e64)
            close = lambda a, b, what: np.testing.assert_allclose(a, np.asarray(b), rtol=1e-9, atol=1e-12, err_msg=what)
            close(ref["mean"], save_mean, "mean")
            close(ref["istd"], save_istd, "istd")
            close(ref["running_mean"], rm, "running_mean")
            close(ref["running_var"], rv, "running_var")
            close(z.astype(np.float64) * ref["scale"] + ref["shift"], y.numpy()[np.cumsum(w) - 1], "scale / shift")
        else:                                                    # one row: torch refuses to train; biased variance = 0, no correction
            # (the replicas are rounded shares: their exact sums give a variance of a few 1e-16, not 0)
            assert (ref["var"] < 1e-13).all() and np.allclose(ref["istd"], 1 / np.sqrt(e64)) and (ref["unbiased"] == ref["var"]).all()
            np.testing.assert_allclose(ref["running_var"], (1 - m64) * rv0.astype(np.float64), rtol=1e-15)
            np.testing.assert_allclose(ref["mean"], z[0].astype(np.float64), rtol=1e-12)
        assert ref["scale"][0] == 0 and ref["shift"][0] == beta[0]
    # a constant channel: the exact variance is 0; sums that make it slightly negative are clamped
    s1, s2 = np.array([3 * 1.1, 3 * 1.1]), np.array([3 * 1.1 * 1.1 * (1 - 1e-15), 3 * 1.1 * 1.1])
    one = np.ones(2, np.float32)
    ref = L.bn_finalize(np.r_[s1, np.zeros(6)], np.r_[s2, np.zeros(6)], 2, 3, one, one, eps, mom)
    assert ref["clamped"][0] and ref["var"][0] == 0 and ref["istd"][0] == 1 / np.sqrt(float(np.float32(eps)))
    assert (L.bn_f64_term(np.r_[s1, np.zeros(6)], np.r_[s2, np.zeros(6)], 2, 3, 2) > abs(s2[0] / 3 - (s1[0] / 3) ** 2) / 4).all()


def test_backward_formulas_equal_torch_autograd():
    """BatchNorm (train) -> ReLU -> max-pool over groups in float64 torch; the pooled-gradient statistics and the coefficients
    P, Q, S of dZ = P * dY - w * (Q + S * z) reproduce autograd's dgamma, dbeta and dZ"""
    rng = np.random.default_rng(4)
    C, eps, mom = 6, 1e-5, 0.1
    off = L.groups(rng, [1, 2, 3, 7, 8, 9, 5, 4])
    rows, G = int(off[-1]), len(off) - 1
    z = rng.normal(size=(rows, C)).astype(np.float32)
    gamma, beta = rng.normal(size=C).astype(np.float32), (rng.normal(size=C) * 0.3).astype(np.float32)
    dout = rng.normal(size=(G, C)).astype(np.float32)
    zt = torch.tensor(z.astype(np.float64), requires_grad=True)
    gt, bt = torch.tensor(gamma.astype(np.float64), requires_grad=True), torch.tensor(beta.astype(np.float64), requires_grad=True)
    y = torch.relu(torch.nn.functional.batch_norm(zt, None, None, gt, bt, True, mom, float(np.float32(eps))))
    pooled = torch.stack([y[off[g]:off[g + 1]].max(dim=0).values for g in range(G)])
    (pooled * torch.from_numpy(dout.astype(np.float64))).sum().backward()
    # the kernels' route: float32 saved statistics (here: float64 values that happen to be float32 would be a different problem,
    # so the comparison is made at float32 accuracy of the saved vectors)
    z64 = z.astype(np.float64)
    fin = L.bn_finalize(np.r_[z64.sum(0), np.zeros(3 * C)], np.r_[(z64 * z64).sum(0), np.zeros(3 * C)], C, rows, gamma, beta, eps, mom)
    sc, sh, mu, is_ = (fin[k].astype(np.float32) for k in ("scale", "shift", "mean", "istd"))
    out, arg = L.segment_pool(z, off, sc, sh)
    np.testing.assert_allclose(out, pooled.detach().numpy(), rtol=1e-5, atol=1e-6)
    zp = z[arg, np.arange(C)[None, :]]
    st = L.pool_bwd_stats(dout, zp, sc, sh, mu, is_, np.float64)
    np.testing.assert_allclose(st["dbeta"], bt.grad.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(st["dgamma"], gt.grad.numpy(), rtol=1e-5, atol=1e-5)
    st32 = L.pool_bwd_stats(dout, zp, sc, sh, mu, is_, np.float32)
    assert st32["dbeta"].dtype == np.float32 and np.allclose(st32["dgamma"], st["dgamma"], rtol=1e-4, atol=1e-5)
    assert (st["masked"] == np.where(st["live"], dout, 0)).all() and st["live"].any() and not st["live"].all()
    co = L.bn_bwd_coef(np.r_[st["dbeta"], np.zeros(3 * C)], np.r_[st["dgamma"], np.zeros(3 * C)], C, sc, mu, is_, rows,
                       gacc_gamma=np.full(C, 2.0), gacc_beta=np.full(C, -1.0))
    dY = np.zeros((rows, C))
    np.add.at(dY, (arg, np.broadcast_to(np.arange(C)[None, :], arg.shape)), st["masked"].astype(np.float64))
    dZ = co["P"].astype(np.float64) * dY - (co["Q"] + co["S"] * z64)
    np.testing.assert_allclose(dZ, zt.grad.numpy(), rtol=1e-4, atol=2e-6)
    assert (co["gacc_gamma"] == 2.0 + st["dgamma"]).all() and (co["gacc_beta"] == -1.0 + st["dbeta"]).all()
    assert (co["P"].view(np.uint32) == sc.view(np.uint32)).all()
