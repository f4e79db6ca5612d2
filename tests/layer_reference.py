"""Plain references for the per-layer kernels of ga-ddpg_amd/csrc/layers.hip and their shared arithmetic in csrc/common.hpp:
train-mode BatchNorm finalisation and backward coefficients, the segment max-pool with its arg-max tie rule, the finish of the
max-pool folded into the GEMM epilogue, the pooled-gradient statistics.  numpy only (importable without a GPU), written from
torch.nn.BatchNorm1d / 2d (train mode), torch.nn.functional.max_pool2d(kernel=[1, nsample], return_indices=True) and
include/gaddpg.h; tests/test_layer_reference.py pins them to torch and to libm.

Activations are exact: a kernel forms relu(fmaf(z, scale, shift)) with ONE rounding, and fmaf32 below is that correctly rounded
fused multiply-add, so pooled maxima and arg-max rows can be compared bit for bit.  The BatchNorm references work on the GIVEN
replicated float64 sums in exact rational arithmetic (fractions.Fraction): whatever error the sums carry is the producer's, what is
checked is what the finalisation does with them."""
import math
from fractions import Fraction

import numpy as np

STAT_REPLICAS = 4          # GAD_STAT_REPLICAS (include/gaddpg.h)


# ----------------------------------------------------------------------------- the fused multiply-add
def fmaf32(z, s, t):
    """float32(z * s + t) with ONE rounding (round to nearest even), elementwise over float32 arrays.
    The product of two float32 values is exact in float64 (48 significant bits).  p + t is not: TwoSum gives the float64 sum
    and its exact error, and the sum is moved to the neighbour with an odd last bit whenever the error is non-zero (round to
    odd): float64 carries 29 bits more than float32, so rounding that value to float32 equals rounding the exact sum --
    (double)z * s + t -> float32 alone rounds twice and misses halfway cases."""
    z, s, t = np.broadcast_arrays(np.asarray(z, np.float32), np.asarray(s, np.float32), np.asarray(t, np.float32))
    p = z.astype(np.float64) * s.astype(np.float64)
    b = t.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sm = p + b
        bb = sm - p
        err = (p - (sm - bb)) + (b - bb)
        odd = (np.ascontiguousarray(sm).view(np.int64) & 1).astype(bool)
        fix = (err != 0) & ~odd & np.isfinite(sm)
        toward = np.where(err > 0, np.inf, -np.inf)
        sm = np.where(fix, np.nextafter(sm, toward), sm)
        return sm.astype(np.float32)


def affine_act(z, scale, shift, relu):
    """gad_affine_act: act(fmaf32(z, scale, shift)); scale None: no affine map"""
    y = np.asarray(z, np.float32) if scale is None else fmaf32(z, np.asarray(scale, np.float32)[None, :],
                                                              np.asarray(shift, np.float32)[None, :])
    return np.maximum(y, np.float32(0)) if relu else y.copy()


# ----------------------------------------------------------------------------- segment max-pool
def _segments(a, off, op, empty):
    """op.reduceat over the groups' rows; a group without rows gives `empty` (reduceat itself would return a[off[g]])"""
    off = np.asarray(off, np.int64)
    some = np.diff(off) > 0
    out = np.empty((len(off) - 1,) + a.shape[1:], a.dtype)
    out[...] = empty
    if some.any():
        out[some] = op.reduceat(a, off[:-1][some], axis=0)       # (dropping empty groups leaves the other boundaries where they are)
    return out


def segment_pool(z, off, scale=None, shift=None):
    """out[g, c] = max over the rows off[g] .. off[g + 1] - 1 of relu(fmaf32(z[r, c], scale[c], shift[c])) (scale None: relu(z));
    argmax[g, c] = the FIRST row of the group that attains it (torch's max_pool2d keeps the first of tied maxima).  A group
    without rows gives 0 and off[g] (include/gaddpg.h).
    z: (rows, C) float32.  -> (out float32 (G, C), argmax int32 (G, C), global row indices)"""
    z, off = np.asarray(z, np.float32), np.asarray(off, np.int64)
    assert (np.diff(off) >= 0).all() and off[0] == 0 and off[-1] == z.shape[0]
    y = affine_act(z, scale, shift, 1)
    best = _segments(y, off, np.maximum, np.float32(0))
    grp = np.repeat(np.arange(len(off) - 1), np.diff(off))
    idx = np.where(y == best[grp], np.arange(z.shape[0], dtype=np.int64)[:, None], np.int64(1) << 40)
    first = _segments(idx, off, np.minimum, 0)
    first = np.where((np.diff(off) > 0)[:, None], first, off[:-1, None])
    return best.astype(np.float32), first.astype(np.int32)


# ----------------------------------------------------------------------------- max-pool folded into the GEMM epilogue
def pool_ord(v):
    """order-preserving bits of a float32 (csrc/gemm_common.hpp pool_ord): unsigned compare == float compare"""
    u = np.ascontiguousarray(np.asarray(v, np.float32)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def pool_unord(u):
    u = np.asarray(u, np.uint32)
    return np.ascontiguousarray(np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u).astype(np.uint32)).view(np.float32)


def pool_sign(gamma):
    return np.where(np.asarray(gamma, np.float32) < 0, np.float32(-1), np.float32(1)).astype(np.float32)


def pool_keys(z, off, gamma):
    """the packed keys the GEMM epilogue leaves (csrc/gemm_common.hpp pool_ord / pool_put): per (group, channel) the maximum over the
    group's rows of  pool_ord(sgn(gamma) * z) << 32 | (0xffffffff - row),  sgn = -1 for gamma < 0, else +1 -- the largest
    sgn * z, among equal values the smallest row.  -> uint64 (G, C)"""
    z, off = np.asarray(z, np.float32), np.asarray(off, np.int64)
    v = (z * pool_sign(gamma)[None, :]).astype(np.float32)
    row = (np.uint64(0xffffffff) - np.arange(z.shape[0], dtype=np.uint64))[:, None]
    k = (pool_ord(v).astype(np.uint64) << np.uint64(32)) | row
    return _segments(k, off, np.maximum, np.uint64(0))          # (a group without rows keeps key 0, "no row yet")


def pool_finalize(keys, off, scale, shift, gamma):
    """gad_pool_finalize as include/gaddpg.h states it: zmax = the winning raw value (key 0: no row, 0), out = relu(fmaf32(zmax,
    scale, shift)), argmax = the key's row where out > 0 and scale != 0, else the group's first row off[g].
    -> (out float32, argmax int32, zmax float32), each (G, C)"""
    keys, off = np.asarray(keys, np.uint64), np.asarray(off, np.int64)
    scale, shift = np.asarray(scale, np.float32), np.asarray(shift, np.float32)
    some = keys != 0
    hi = (keys >> np.uint64(32)).astype(np.uint32)
    zmax = np.where(some, pool_sign(gamma)[None, :] * pool_unord(hi), np.float32(0)).astype(np.float32)
    out = np.where(some, affine_act(zmax, scale, shift, 1), np.float32(0)).astype(np.float32)
    row = (np.uint64(0xffffffff) - (keys & np.uint64(0xffffffff))).astype(np.int64)
    first = np.broadcast_to(off[:-1, None], keys.shape)
    arg = np.where(some & (out > 0) & (scale != 0)[None, :], row, first)
    return out, arg.astype(np.int32), zmax


# ----------------------------------------------------------------------------- BatchNorm: finalisation
def _replica_sum(a, stride, C):
    """exact sum of the replicas of every channel -> list of Fractions"""
    a = np.asarray(a, np.float64)
    return [sum((Fraction(float(a[r * stride + c])) for r in range(STAT_REPLICAS)), Fraction(0)) for c in range(C)]


def bn_finalize(stat_sum, stat_sq, stride, count, gamma, beta, eps, momentum, rmean=None, rvar=None):
    """Train-mode BatchNorm from the given replicated float64 sums (replica r of channel c at [r * stride + c]) over `count`
    rows, in exact rational arithmetic up to the square root: mean = s1 / n, var = max(s2 / n - mean**2, 0) (biased),
    istd = 1 / sqrt(var + eps), scale = gamma * istd, shift = beta - mean * scale; running statistics moved by one momentum step
    towards mean and the UNBIASED variance var * n / (n - 1) (n == 1: the biased one).  eps and momentum enter as the float32
    values the kernels receive.  -> dict of float64 arrays (the exact values rounded once; istd and what follows from it
    within 2**-51)"""
    gamma, beta = np.asarray(gamma, np.float32), np.asarray(beta, np.float32)
    C = gamma.shape[0]
    n = Fraction(float(count))
    e, m = Fraction(float(np.float32(eps))), float(np.float32(momentum))
    s1, s2 = _replica_sum(stat_sum, stride, C), _replica_sum(stat_sq, stride, C)
    out = {k: np.zeros(C) for k in ("mean", "var", "istd", "scale", "shift", "unbiased")}
    out["clamped"] = np.zeros(C, bool)
    for c in range(C):
        mean = s1[c] / n
        var = s2[c] / n - mean * mean
        out["clamped"][c] = var < 0
        var = max(var, Fraction(0))
        istd = 1.0 / math.sqrt(float(var + e))
        out["mean"][c], out["var"][c], out["istd"][c] = float(mean), float(var), istd
        out["scale"][c] = float(gamma[c]) * istd
        out["shift"][c] = float(beta[c]) - float(mean) * out["scale"][c]
        out["unbiased"][c] = float(var * n / (n - 1)) if n > 1 else float(var)
    if rmean is not None:
        out["running_mean"] = (1.0 - m) * np.asarray(rmean, np.float32).astype(np.float64) + m * out["mean"]
        out["running_mean_abs"] = np.abs((1.0 - m) * np.asarray(rmean, np.float32).astype(np.float64)) + np.abs(m * out["mean"])
    if rvar is not None:
        out["running_var"] = (1.0 - m) * np.asarray(rvar, np.float32).astype(np.float64) + m * out["unbiased"]
        out["running_var_abs"] = np.abs((1.0 - m) * np.asarray(rvar, np.float32).astype(np.float64)) + np.abs(m * out["unbiased"])
    return out


def bn_f64_term(stat_sum, stat_sq, stride, count, C):
    """What a float64 evaluation of var = s2 / n - (s1 / n)**2 from the replicated sums can be off by, per channel (absolute):
    the three adds over the replicas commit at most 2**-53 of a partial sum each (<= A = sum of |replica|), the two divisions,
    the square and the subtraction one rounding each:
        2**-53 * (4 * A2 / n + 6 * |mean| * A1 / n + 3 * mean**2 + |var|)."""
    a1 = np.abs(np.asarray(stat_sum, np.float64)).reshape(-1)
    a2 = np.abs(np.asarray(stat_sq, np.float64)).reshape(-1)
    A1 = sum(a1[r * stride:r * stride + C] for r in range(STAT_REPLICAS)) / count
    A2 = sum(a2[r * stride:r * stride + C] for r in range(STAT_REPLICAS)) / count
    s1 = sum(np.asarray(stat_sum, np.float64).reshape(-1)[r * stride:r * stride + C] for r in range(STAT_REPLICAS)) / count
    s2 = sum(np.asarray(stat_sq, np.float64).reshape(-1)[r * stride:r * stride + C] for r in range(STAT_REPLICAS)) / count
    return 2.0 ** -53 * (4 * A2 + 6 * np.abs(s1) * A1 + 3 * s1 * s1 + np.abs(s2 - s1 * s1))


# ----------------------------------------------------------------------------- BatchNorm: backward coefficients
def bn_bwd_coef(dbeta, dgamma, stride, scale, mean, istd, count, gacc_gamma=None, gacc_beta=None):
    """dZ = P * dY - w * (Q + S * z):  P = scale,  Q = scale * (dbeta - mean * istd * dgamma) / n,  S = scale * istd * dgamma / n,
    with dbeta / dgamma the exact sums of the given replicas (rational arithmetic).  The arena adds are float64 operations and
    are reproduced as such: gacc += ((r0 + r1) + r2) + r3.
    -> dict: P float32 (bit-exact), Q / S float64, Q_f64 (the magnitude the float64 evaluation's rounding is relative to),
    gacc_gamma / gacc_beta float64 (bit-exact) where given"""
    scale, mean, istd = (np.asarray(x, np.float32) for x in (scale, mean, istd))
    C = scale.shape[0]
    n = Fraction(float(count))
    db, dg = _replica_sum(dbeta, stride, C), _replica_sum(dgamma, stride, C)
    out = {"P": scale.copy(), "Q": np.zeros(C), "S": np.zeros(C), "Q_f64": np.zeros(C)}
    for c in range(C):
        sc, mu, is_ = Fraction(float(scale[c])), Fraction(float(mean[c])), Fraction(float(istd[c]))
        out["Q"][c] = float(sc * (db[c] - mu * is_ * dg[c]) / n)
        out["S"][c] = float(sc * is_ * dg[c] / n)
        out["Q_f64"][c] = float(abs(sc) * (abs(db[c]) + abs(mu * is_ * dg[c])) / n)
    for key, acc, rep in (("gacc_gamma", gacc_gamma, dgamma), ("gacc_beta", gacc_beta, dbeta)):
        if acc is not None:
            rep = np.asarray(rep, np.float64).reshape(-1)
            r = [rep[k * stride:k * stride + C] for k in range(STAT_REPLICAS)]
            out[key] = np.asarray(acc, np.float64) + ((((0.0 + r[0]) + r[1]) + r[2]) + r[3])
    return out


# ----------------------------------------------------------------------------- pooled-gradient statistics
def pool_bwd_stats(dout, zp, scale, shift, mean, istd, dtype):
    """gad_pool_bwd_stats over the (G, C) pooled gradient `dout` and the raw value `zp` of every routed row:
    live = fmaf32(zp, scale, shift) > 0 (the forward activation, exact),  dbeta[c] = sum_g dout * live,
    dgamma[c] = sum_g dout * live * xhat,  xhat = (zp - mean) * istd.
    dtype float64: the reference (float64 products, float64 sums).  float32: the yardstick -- every product rounded to float32,
    np.sum in float32 along the contiguous axis (pairwise).
    -> dict: dbeta, dgamma (C), abs_beta, abs_gamma (C; sums of |terms| in float64), masked (G, C) float32 = dout where live
    else 0, live (G, C) bool"""
    dt = np.dtype(dtype).type
    dout, zp = np.asarray(dout, np.float32), np.asarray(zp, np.float32)
    scale, shift, mean, istd = (np.asarray(x, np.float32) for x in (scale, shift, mean, istd))
    live = fmaf32(zp, scale[None, :], shift[None, :]) > 0
    d = np.where(live, dout, np.float32(0)).astype(dtype)
    xhat = ((zp.astype(dtype) - mean.astype(dtype)[None, :]) * istd.astype(dtype)[None, :]).astype(dtype)
    tb, tg = d, (d * xhat).astype(dtype)
    col = lambda a: np.sum(np.ascontiguousarray(a.T), axis=1, dtype=dtype)
    return {"dbeta": col(tb), "dgamma": col(tg), "abs_beta": np.abs(tb.astype(np.float64)).sum(axis=0),
            "abs_gamma": np.abs(tg.astype(np.float64)).sum(axis=0), "masked": np.where(live, dout, np.float32(0)).astype(np.float32),
            "live": live, "dt": dt}


# ----------------------------------------------------------------------------- inputs
def replicate(total, stride, C, rng, pad=0.0):
    """float64 totals (C) -> (STAT_REPLICAS * stride) replicated accumulators holding uneven shares of them, one negative:
    shares (u0, u1, -u2, 1 - u0 - u1 + u2) with u0, u1 in [0.2, 0.45], u2 in [0.01, 0.1], so that the partial sums of
    ((r0 + r1) + r2) + r3 stay below 0.9, 0.9 and 1 times the total.  The shares are rounded: the exact sum of the replicas
    (which is what the references take) differs from `total` in the last bits, as a real accumulation would.  The columns
    between C and stride hold `pad`."""
    total = np.asarray(total, np.float64)
    u0, u1, u2 = rng.uniform(0.2, 0.45, C), rng.uniform(0.2, 0.45, C), rng.uniform(0.01, 0.1, C)
    out = np.full(STAT_REPLICAS * stride, pad, np.float64)
    for r, sh in enumerate((u0, u1, -u2, 1.0 - u0 - u1 + u2)):
        out[r * stride:r * stride + C] = sh * total
    return out


def groups(rng, sizes):
    """CSR offsets of groups with the given sizes, shuffled -> int32 (G + 1)"""
    sizes = np.asarray(sizes, np.int64).copy()
    rng.shuffle(sizes)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
