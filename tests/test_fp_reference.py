"""CPU pins of tests/fp_reference.py (the yardsticks of tests/test_gpu_fp_ops.py), of PointnetFPModule's module tree and of the
host-side argument checks of gad_three_nn / gad_three_interpolate / gad_three_interpolate_grad.  No GPU: nothing is launched."""
import numpy as np
import pytest
import torch

from tests import fp_reference as F

f32 = np.float32


def _insertion_loop(u, known):
    """upstream's three_nn_kernel for one query point, literally: three slots, sequential strict-< insertion, float32 distance"""
    best = [f32(np.inf)] * 3                      # (the kernel's 1e40 double is +inf once stored as a float)
    besti = [0, 0, 0]
    for k in range(known.shape[0]):
        x, y, z = known[k]
        d = f32(f32(f32(u[0] - x) * f32(u[0] - x)) + f32(f32(u[1] - y) * f32(u[1] - y)))
        d = f32(d + f32(f32(u[2] - z) * f32(u[2] - z)))
        if d < best[0]:
            best[2], besti[2] = best[1], besti[1]
            best[1], besti[1] = best[0], besti[0]
            best[0], besti[0] = d, k
        elif d < best[1]:
            best[2], besti[2] = best[1], besti[1]
            best[1], besti[1] = d, k
        elif d < best[2]:
            best[2], besti[2] = d, k
    return best, besti


def _lattice(rng, shape):
    return (rng.integers(0, 4, size=shape).astype(f32) * f32(0.25) + f32(0.5))


@pytest.mark.parametrize("m", (1, 2, 3, 4, 9, 40))
def test_three_nn_ref_is_the_sequential_insertion(m):
    rng = np.random.default_rng(100 + m)
    B, n = 2, 23
    known = _lattice(rng, (B, m, 3))
    unknown = _lattice(rng, (B, n, 3))
    if m >= 4:
        known[1, m // 2:] = known[1, :m - m // 2]                   # every known point twice: exact ties everywhere
    unknown[0, :min(n, m)] = known[0, :min(n, m)]                   # d = 0
    if m >= 9:
        known[0, 0, 0] = np.nan                                     # a NaN distance is never selected
    with np.errstate(invalid="ignore"):
        d2, idx = F.three_nn_ref(unknown, known)
        assert d2.dtype == f32 and idx.dtype == np.int32 and d2.shape == idx.shape == (B, n, 3)
        for b in range(B):
            for i in range(n):
                best, besti = _insertion_loop(unknown[b, i], known[b])
                assert list(idx[b, i]) == besti, (b, i)
                assert np.array(best, f32).tobytes() == d2[b, i].tobytes(), (b, i)
    if m < 3:
        assert (idx[:, :, m:] == 0).all() and np.isposinf(d2[:, :, m:]).all()
    ties = (d2[:, :, 0] == d2[:, :, 1]).sum() if m >= 2 else 1
    assert ties > 0                                                  # the clouds do produce exact ties


def test_three_interpolate_ref_against_float64_einsum():
    rng = np.random.default_rng(5)
    B, C, m, n = 2, 7, 11, 29
    pts = rng.normal(size=(B, C, m)).astype(f32)
    idx = rng.integers(0, m, size=(B, n, 3)).astype(np.int32)
    idx[0, 3] = 4                                                    # the three indices coincide
    w = rng.random((B, n, 3)).astype(f32)
    w[1, 5, 1] = 0
    got = F.three_interpolate_ref(pts, idx, w)
    onehot = np.zeros((B, n, 3, m))
    np.put_along_axis(onehot, idx[..., None].astype(np.int64), 1.0, axis=3)
    want = np.einsum("bnk,bnkm,bcm->bcn", w.astype(np.float64), onehot, pts.astype(np.float64))
    mag = np.einsum("bnk,bnkm,bcm->bcn", np.abs(w).astype(np.float64), onehot, np.abs(pts).astype(np.float64))
    assert got.dtype == f32
    u = 2.0 ** -24
    assert (np.abs(got - want) <= 3 * u / (1 - 3 * u) * mag).all()  # three products, two sums: at most 3 roundings deep


def test_three_interpolate_grad_ref_against_autograd_and_a_plain_loop():
    rng = np.random.default_rng(6)
    B, C, m, n = 2, 3, 5, 17
    go = rng.normal(size=(B, C, n)).astype(f32)
    idx = rng.integers(0, m, size=(B, n, 3)).astype(np.int32)
    idx[1] = 2                                                       # every entry of a sample on one destination
    w = rng.random((B, n, 3)).astype(f32)
    # float64 form == autograd of the float64 composition
    pts = torch.zeros(B, C, m, dtype=torch.float64, requires_grad=True)
    ix = torch.from_numpy(idx).long()
    f = torch.gather(pts.unsqueeze(2).expand(B, C, n, m), 3, ix.unsqueeze(1).expand(B, C, n, 3))
    out = (f * torch.from_numpy(w).double().unsqueeze(1)).sum(-1)
    out.backward(torch.from_numpy(go).double())
    g64 = F.three_interpolate_grad_ref(go, idx, w, m, np.float64)
    assert np.abs(g64 - pts.grad.numpy()).max() <= 1e-12
    # float32 form == a literal sequential loop in i*3+k order
    g32 = F.three_interpolate_grad_ref(go, idx, w, m)
    want = np.zeros((B, C, m), f32)
    for b in range(B):
        for c in range(C):
            for i in range(n):
                for k in range(3):
                    want[b, c, idx[b, i, k]] = f32(want[b, c, idx[b, i, k]] + f32(go[b, c, i] * w[b, i, k]))
    assert g32.dtype == f32 and g32.tobytes() == want.tobytes()
    cnt, mag = F.three_interpolate_grad_bound(go, idx, w, m)
    assert cnt.sum() == B * n * 3 and cnt[1, 2] == n * 3
    assert (np.abs(g32 - g64) <= (cnt[:, None, :] + 1) * 2.0 ** -24 * mag).all()


def test_fp_module_ref_runs_every_branch_and_differentiates():
    from ga_ddpg_amd.pointnet2_ops.pointnet2_modules import build_shared_mlp
    torch.manual_seed(0)
    B, n, m, C1, C2 = 2, 9, 4, 3, 2
    mlp = build_shared_mlp([C1 + C2, 8, 4], True).double()
    unknown, known = torch.rand(B, n, 3), torch.rand(B, m, 3)
    _, idx = F.three_nn_ref(unknown.numpy(), known.numpy())
    kf = torch.randn(B, C2, m, dtype=torch.float64, requires_grad=True)
    uf = torch.randn(B, C1, n, dtype=torch.float64)
    y = F.fp_module_ref(mlp, unknown, known, uf, kf, torch.from_numpy(idx))
    assert y.shape == (B, 4, n) and y.dtype == torch.float64
    y.sum().backward()
    assert kf.grad is not None and float(kf.grad.abs().sum()) > 0
    assert F.fp_module_ref(mlp, unknown, None, uf, kf[:, :, :1], None).shape == (B, 4, n)
    assert F.fp_module_ref(build_shared_mlp([C2, 4], True).double(), unknown, known, None, kf, torch.from_numpy(idx)).shape == (B, 4, n)


@pytest.mark.parametrize("bn", (True, False))
def test_fp_module_state_dict_keys(bn):
    from ga_ddpg_amd.pointnet2_ops.pointnet2_modules import PointnetFPModule
    keys = list(PointnetFPModule(mlp=[13, 32, 16], bn=bn).state_dict().keys())
    if bn:
        per_bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
        want = (["mlp.0.weight"] + ["mlp.1." + k for k in per_bn] + ["mlp.3.weight"] + ["mlp.4." + k for k in per_bn])
    else:
        want = ["mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias"]
    assert keys == want


def test_fp_entry_points_refuse_bad_arguments_without_a_launch():
    """null pointer, negative size, m = 0 with n > 0: status codes from the host-side checks (nothing is launched, so this runs
    without a GPU), the message through gad_last_error; empty problems are GAD_OK"""
    import ctypes as C
    from ga_ddpg_amd import hip
    L = hip.lib()
    OK, ERR_NULL, ERR_SHAPE = 0, -1, -2
    null, p = C.c_void_p(None), C.c_void_p(0x1000)
    assert L.gad_three_nn(null, p, 1, 4, 4, p, p, null) == ERR_NULL and b"three_nn: null" in L.gad_last_error()
    assert L.gad_three_nn(p, p, 1, 4, 4, p, null, null) == ERR_NULL
    assert L.gad_three_nn(p, p, 1, -4, 4, p, p, null) == ERR_SHAPE and b"negative" in L.gad_last_error()
    assert L.gad_three_nn(p, p, -1, 4, 4, p, p, null) == ERR_SHAPE
    assert L.gad_three_nn(p, p, 1, 4, -1, p, p, null) == ERR_SHAPE
    assert L.gad_three_nn(p, p, 1, 4, 0, p, p, null) == ERR_SHAPE and b"no known point" in L.gad_last_error()
    assert L.gad_three_nn(p, p, 1, 0, 0, p, p, null) == OK and L.gad_three_nn(p, p, 0, 4, 4, p, p, null) == OK
    for name in ("gad_three_interpolate", "gad_three_interpolate_grad"):
        f = getattr(L, name)
        # (points | grad_out, idx, weight, B, C, m | n, n | m, out, stream)
        assert f(p, null, p, 1, 2, 4, 4, p, null) == ERR_NULL and b"null" in L.gad_last_error()
        assert f(p, p, p, 1, 2, 4, 4, null, null) == ERR_NULL
        assert f(p, p, p, 1, -2, 4, 4, p, null) == ERR_SHAPE and b"negative" in L.gad_last_error()
        assert f(p, p, p, 1, 2, -4, 4, p, null) == ERR_SHAPE
        assert f(p, p, p, 1, 2, 4, -4, p, null) == ERR_SHAPE
        assert f(p, p, p, 1, 0, 4, 4, p, null) == OK              # C == 0
    assert L.gad_three_interpolate(p, p, p, 1, 2, 0, 4, p, null) == ERR_SHAPE and b"no known point" in L.gad_last_error()
    assert L.gad_three_interpolate(p, p, p, 1, 2, 4, 0, p, null) == OK          # n == 0
    assert L.gad_three_interpolate_grad(p, p, p, 1, 2, 4, 0, p, null) == ERR_SHAPE and b"no known point" in L.gad_last_error()
    with pytest.raises(TypeError):
        L.gad_three_nn(p, p, 1, 4, 4, p, p)                        # the binding carries the signature: a short call is refused
