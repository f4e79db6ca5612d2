"""The per-layer kernels of ga-ddpg_amd/csrc/layers.hip and their shared arithmetic in csrc/common.hpp -- gad_bn_finalize,
gad_bn_bwd_coef, gad_segment_pool, gad_pool_finalize, gad_pool_bwd_stats (plain and deterministic), gad_affine_act -- called
directly on small adversarial shapes and compared with the plain references of tests/layer_reference.py.

Yardsticks.  Activations, pooled maxima, arg-max rows, zmax, masks, P and the arena adds: bit-exact (a kernel's fmaf rounds once,
and so does layer_reference.fmaf32).  BatchNorm finalisation and backward coefficients: bounds derived per channel against the
exact rational reference (_check_bn, test_bn_bwd_coef).  Pooled-gradient sums and the chain against torch autograd: the
head-loss criterion, err <= max(3 x the float32 reference's own error, 1e-6).

Every buffer lives inside a byte arena filled with 0xA5 with 64 guard bytes on both sides that must come back untouched; pure
outputs start as NaN; inputs must come back bit-identical.  All inputs come from seeded generators; nothing is skipped or
filtered at run time.

What these tests found when they were written (all fixed in csrc/layers.hip; the cases stay in test_argument_checks_*):
gad_pool_bwd_stats with C = 0 evaluated 256 % C on the host (a division by zero before any check); gad_bn_bwd_coef divided by an
unchecked count (gad_bn_finalize refused count < 1, the backward did not); gad_segment_pool accepted z_pitch < C and gad_affine_act
either pitch < C, reading or writing overlapping rows; gad_bn_eval_affine and gad_bn_bwd_coef launched an empty grid for C = 0 (a
launch error) where gad_bn_running_update returned GAD_OK and gad_bn_finalize GAD_ERR_SHAPE -- now C = 0 is GAD_OK without a
launch and C < 0 GAD_ERR_SHAPE in every entry point of the file.  gad_pool_bwd_stats with zmax alone takes x_hat of a scale == 0
channel from the key's row, not from the routed first row: a host-side check cannot see scale, so the header now documents the
deviation and test_pool_bwd_stats pins it.  Groups without rows (0, grp_off[g]) are now stated in the header and pinned.  The
arithmetic itself held: every bit-exact comparison and every derived bound passed on the first run.

Largest error seen on the MI355X, as a fraction of the bound: istd 0.80 (of 1.25 * 2**-24; 0.50 of the specified 2**-23), scale 0.60,
mean 1.00 (one rounding: 0.9996), shift 0.70, running_mean 0.58, running_var 0.56, Q 0.98, S 0.99 (one rounding each);
pooled-gradient sums relative to the channel-wise max of sum |terms|: dbeta 5.8e-8, dgamma 8.6e-8, deterministic 5.1e-8 / 5.3e-8
(gate 1e-6); the chain against float64 autograd, relative to max |float64|: Y 7.0e-8, dZ 6.3e-8, dgamma 7.9e-8, dbeta 9e-18.

Mutations tried in scratch builds of the library, with the tests that failed on each: the shuffle fold's tie comparison
reversed (segment_pool_bit_exact 20, beyond_the_grid_cap 2); `>=` in the per-lane update, i.e. the last of a lane's ties
(segment_pool_bit_exact 32); the 4-deep loop's tail dropped (segment_pool 34); no grid-stride step in the pool, the pool finish or
the backward statistics (the cases above the 2048 / 1024 / 512 workgroup caps); three replicas summed in the finalisation (52: bn_finalize,
pool_finalize, the chain) or in the backward coefficients (19); the running statistics published by every workgroup
(pool_finalize G = 16400, both widths); the `scale != 0` term dropped (pool_finalize 48); the sign of gamma ignored (52); keys not
reset (52); the gather route dropped (pool_bwd_stats 26 + deterministic 6); the deterministic reduce overwriting the accumulators
(6); the biased variance in the running statistics (44); the arena add overwritten (19); the mean formed in float32 (21); a
double-rounded multiply-add in gad_affine_act (8: the halfway channels).  Three mutations survived the first version of this file
and each got a case: the variance clamp removed (within the bounds' precondition a negative variance is smaller than eps --
test_bn_finalize_clamps_a_negative_variance); the arg-max initialised to row 0 instead of the group's first row (only a group
without rows shows it -- test_pool_groups_without_rows); istd evaluated as 1.f / sqrtf(float) (inside the specified 2**-23;
outside the 1.25 * 2**-24 that the derivation gives, which is what _check_bn asserts now).  No mutation survives the file as it
stands.  Not tried: out-of-bounds mutations (dropping the g < G guards), which would write outside the buffers."""
import numpy as np
import pytest
import torch

from tests import layer_reference as L
from tests import optim_reference as R
from tests.test_gpu_optim_kernels import Buf, _nan32, _same

pytestmark = pytest.mark.gpu

OK, ERR_NULL, ERR_SHAPE = 0, -1, -2
EPS, MOM = 1e-5, 0.1
BIG = np.float32(1e30)              # what padding columns hold: a misread column would win any maximum
POOL_C = (8, 16, 32, 64, 128, 256, 512, 1024)


def _hip():
    from ga_ddpg_amd import hip
    return hip


def _rc(name, *a):
    """the status an entry point returns (hip.call raises on anything but 0)"""
    hip = _hip()
    return getattr(hip.lib(), name)(*(hip._args(*a) + [hip.stream()]))


def _P(b):
    return None if b is None else b.ptr


def _log(what, err, bound):
    """largest error of a gated quantity as a fraction of its bound (collected from the test output for the docstring above)"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    print("GATE %s: max err / bound %.4f (max err %.3e)" % (what, ratio, float(err.max()) if err.size else 0.0))
    return ratio


def _padded(a, pitch, fill=BIG):
    """(rows, C) -> (rows, pitch) with `fill` in the padding columns"""
    out = np.full((a.shape[0], pitch), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def _quantised(rng, shape):
    """multiples of 1/8 in [-2, 2], no -0.0: exact ties in most groups"""
    return (np.round(rng.uniform(-2, 2, shape) * 8) / 8 + 0.0).astype(np.float32)


# ----------------------------------------------------------------------------- 1. gad_affine_act
@pytest.mark.parametrize("rows,C", ((1, 1), (3, 5), (257, 13), (64, 512)))
@pytest.mark.parametrize("pad_in,pad_out", ((0, 0), (3, 0), (0, 3), (3, 3)))
def test_affine_act_bit_exact(rows, C, pad_in, pad_out):
    hip = _hip()
    rng = np.random.default_rng(1000 + rows + C)
    z = (rng.normal(size=(rows, C)) * 10.0 ** rng.uniform(-2, 2, (rows, C))).astype(np.float32)
    z[::3, ::2] = _quantised(rng, z[::3, ::2].shape)
    scale = rng.normal(size=C).astype(np.float32)
    special = np.array([0.0, -1.5, 2.0, 0.5, -0.25, 1.0], np.float32)
    for k in range(min(C, len(special))):
        scale[(k * 5) % C if C > 5 else k] = special[k]
    if C == 1:
        scale[0] = -1.5
    shift = (rng.normal(size=C) * 0.5).astype(np.float32)
    if C >= 13:                 # halfway cases: z * s + t lies 2**-70 beside the middle of two float32 values -- (double)z * s + t
        u = 2.0 ** -23          # rounded to float32 rounds twice and goes the other way (tests/test_layer_reference.py)
        scale[7], shift[7], scale[8], shift[8] = 1 - u, 1 + u, -(1 - u), 1 + u
        z[::2, 7:9] = 2.0 ** -24 * (1 + u)
    zin = _padded(z, C + pad_in)
    bz, bs, bt = Buf(zin), Buf(scale), Buf(shift)
    for relu in (0, 1):
        for affine in (True, False):
            want = _padded(L.affine_act(z, scale if affine else None, shift if affine else None, relu), C + pad_out, np.float32(np.nan))
            bo = Buf(_nan32((rows, C + pad_out)))
            hip.call("gad_affine_act", bz.ptr, C + pad_in, rows, C, bs.ptr if affine else None, bt.ptr if affine else None, relu,
                     bo.ptr, C + pad_out)
            _same("affine_act relu %d affine %d (the padding stays NaN)" % (relu, affine), bo.get("out"), want)
    if C >= 13:                                                     # the case can tell a fused multiply-add from the double-rounded form
        naive = (z.astype(np.float64) * scale + shift).astype(np.float32)
        assert (naive.view(np.uint32) != L.affine_act(z, scale, shift, 0).view(np.uint32)).sum() >= rows // 2
    for b, a in ((bz, zin), (bs, scale), (bt, shift)):
        _same("affine_act input", b.get("input"), a)


# ----------------------------------------------------------------------------- 2. gad_segment_pool
def _pool_sizes(C, G=40):
    rpw = 64 // min(C // 4, 64)
    base = [s for s in (1, rpw - 1, rpw, rpw + 1, 4 * rpw - 1, 4 * rpw, 4 * rpw + 1, 8 * rpw + 3) if s >= 1]
    return (base * (G // len(base) + 1))[:G]


def _pool_vectors(rng, C, kind):
    """scale / shift mixing positive, negative and exactly 0 scales with shifts of both signs"""
    if kind == "ties":
        scale = rng.choice(np.array([0.5, -0.25, 2.0, -1.0, 1.0], np.float32), C)
        shift = rng.choice(np.array([0.25, -0.5, 0.125, -0.125], np.float32), C)
    else:
        scale = rng.normal(size=C).astype(np.float32)
        shift = (rng.normal(size=C) * 0.5).astype(np.float32)
    scale[1], scale[5] = 0.0, 0.0
    shift[1], shift[5] = abs(shift[1]) + np.float32(0.25), -abs(shift[5]) - np.float32(0.25)
    scale[0], scale[2] = abs(scale[0]), -abs(scale[2])
    return scale.astype(np.float32), shift.astype(np.float32)


def _run_segment_pool(z, off, C, pitch, scale, shift, what):
    hip = _hip()
    G = len(off) - 1
    zin = _padded(z, pitch)
    want_out, want_arg = L.segment_pool(z, off, scale, shift)
    bz, bo = Buf(zin), Buf(off)
    bs, bt = (None, None) if scale is None else (Buf(scale), Buf(shift))
    out, arg = Buf(_nan32((G, C))), Buf(np.full((G, C), -7, np.int32))
    hip.call("gad_segment_pool", bz.ptr, pitch, C, _P(bs), _P(bt), bo.ptr, G, out.ptr, arg.ptr)
    _same(what + ": out", out.get("out"), want_out)
    _same(what + ": argmax", arg.get("argmax"), want_arg)
    out2 = Buf(_nan32((G, C)))
    hip.call("gad_segment_pool", bz.ptr, pitch, C, _P(bs), _P(bt), bo.ptr, G, out2.ptr, None)
    _same(what + ": out (argmax NULL)", out2.get("out"), want_out)
    _same(what + ": z", bz.get("z"), zin)
    _same(what + ": off", bo.get("off"), off)
    if bs is not None:
        _same(what + ": scale", bs.get(), scale)
        _same(what + ": shift", bt.get(), shift)
    return want_out, want_arg


@pytest.mark.parametrize("C", POOL_C)
@pytest.mark.parametrize("pad", (0, 8))
@pytest.mark.parametrize("kind", ("ties", "normal"))
def test_segment_pool_bit_exact(C, pad, kind):
    rng = np.random.default_rng(2000 + C + pad)
    off = L.groups(rng, _pool_sizes(C))
    rows, G = int(off[-1]), len(off) - 1
    grp = np.repeat(np.arange(G), np.diff(off))
    dead = (np.arange(G) % 5 == 2)                                   # whole groups with nothing above 0
    for affine in (True, False):
        scale, shift = _pool_vectors(rng, C, kind) if affine else (None, None)
        z = _quantised(rng, (rows, C)) if kind == "ties" else rng.normal(size=(rows, C)).astype(np.float32)
        if kind == "ties":
            sgn = np.sign(scale) if affine else np.ones(C, np.float32)
            mag = (2 + np.abs(_quantised(rng, (rows, C)))).astype(np.float32)
            z = np.where(dead[grp][:, None] & (sgn != 0)[None, :], -sgn[None, :] * mag, z).astype(np.float32)
        out, arg = _run_segment_pool(z, off, C, C + pad, scale, shift, "segment_pool C %d %s affine %d" % (C, kind, affine))
        if kind == "ties":
            first = np.broadcast_to(off[:-1, None], arg.shape)
            live_c = np.ones(C, bool) if not affine else ~((scale == 0) & (shift > 0))
            assert (out[dead][:, live_c] == 0).all() and (arg[dead] == first[dead]).all()         # all <= 0: the group's first row
            y = L.affine_act(z, scale, shift, 1)
            tied = sum(int(((y[off[g]:off[g + 1]] == out[g]).sum(axis=0) > 1).sum()) for g in range(G))
            assert tied > G * C // 8, tied                           # the tie rule is exercised, not assumed
            assert (arg != first).any()


@pytest.mark.parametrize("C", (8, 64))
def test_segment_pool_beyond_the_grid_cap(C):
    """G = 8200 groups of 1 - 3 rows: more than the 2048 workgroups x 4 wavefronts of one pass, the grid-stride loop runs"""
    rng = np.random.default_rng(2100 + C)
    off = L.groups(rng, rng.integers(1, 4, 8200))
    z = _quantised(rng, (int(off[-1]), C))
    scale, shift = _pool_vectors(rng, C, "ties")
    _run_segment_pool(z, off, C, C + 8, scale, shift, "segment_pool C %d G 8200" % C)


@pytest.mark.parametrize("C", (8, 64, 512))
def test_pool_groups_without_rows(C):
    """a group without rows (first, in the middle, several in a row, last): 0 and the group's offset from gad_segment_pool, and the
    same from gad_pool_finalize, whose key is still 0 = "no row yet" """
    hip = _hip()
    rng = np.random.default_rng(2200 + C)
    off = np.concatenate([[0], np.cumsum([0, 3, 0, 0, 5, 1, 0, 130, 0])]).astype(np.int32)
    z = _quantised(rng, (int(off[-1]), C))
    scale, shift = _pool_vectors(rng, C, "ties")
    out, arg = _run_segment_pool(z, off, C, C, scale, shift, "segment_pool C %d with empty groups" % C)
    empty = np.diff(off) == 0
    assert (out[empty] == 0).all() and (arg[empty] == off[:-1, None][empty]).all() and (arg[~empty] != 0).any()
    G = len(off) - 1
    keys = L.pool_keys(z, off, scale)
    assert (keys[empty] == 0).all() and (keys[~empty] != 0).all()
    bk, bo, bs, bt = Buf(keys), Buf(off), Buf(scale), Buf(shift)
    o, a, zm = Buf(_nan32((G, C))), Buf(np.full((G, C), -7, np.int32)), Buf(_nan32((G, C)))
    hip.call("gad_pool_finalize", bk.ptr, C, G, bo.ptr, None, None, C, hip.Dbl(1), bs.ptr, None, float(EPS), float(MOM), None, None, bs.ptr,
             bt.ptr, None, None, o.ptr, a.ptr, zm.ptr)
    w_out, w_arg, w_zm = L.pool_finalize(keys, off, scale, shift, scale)
    _same("pool_finalize with empty groups: out", o.get(), w_out)
    _same("pool_finalize with empty groups: argmax", a.get(), w_arg)
    _same("pool_finalize with empty groups: zmax", zm.get(), w_zm)
    _same("pool_finalize against the separate pool", w_out, out)
    assert (w_zm[empty] == 0).all() and (w_arg[empty] == off[:-1, None][empty]).all()


# ----------------------------------------------------------------------------- BatchNorm finalisation: the shared check
def _check_bn(what, ref, term, got, beta, rm_given):
    """Bounds of the train-mode finalisation against the exact reference `ref` (layer_reference.bn_finalize), per channel.
    The kernel evaluates mean = s1 / n and var = s2 / n - mean**2 in float64 from the replica sums; `term`
    (layer_reference.bn_f64_term) bounds what that evaluation can be off by.  PRECONDITION, asserted on the inputs:
    term / (var + eps) <= 2**-26.  Then
      istd   = float32(1 / sqrt(var + eps)): the float64 value is within 2**-27 + 2 * 2**-53 of the exact one, one float32 rounding
               adds 2**-24: relative error <= 2**-24 + 2**-27 + ... -- asserted as 1.25 * 2**-24, which implies the 2**-23 the gate
               was specified with and, unlike it, tells the float64 evaluation from a float32 one (1 / sqrtf: up to 2.5 * 2**-24);
      scale  = float32(gamma * istd): one more rounding: <= 2 * 2**-24 + 2**-27 <= 3 * 2**-24 relative;
      mean   = float32(mean): one rounding of a float64 quotient: <= 2**-24 relative;
      shift  = fma(-float32(mean), scale, beta): the product carries the errors of mean (2**-24) and scale (<= 2.125 * 2**-24), the
               result is rounded once, relative to |shift| <= |beta| + |mean * scale|: absolute error <= 2**-24 * (|beta| + 4.125 *
               |mean * scale|) if every rounding falls the same way; the gate is 2**-22 * (|beta| + |mean * scale|);
      running = (1 - m) * old + m * new in float32: 1 - m, the two products, float32(new) and the sum round once each, and the
               variance carries term * n / (n - 1) (asserted <= 2**-24 of the magnitude): <= 2**-22 * (|(1 - m) * old| + |m * new|)."""
    var_eps = ref["var"] + float(np.float32(EPS))
    assert (term / var_eps <= 2.0 ** -26).all(), "%s: inputs outside the bound's precondition (%.3e)" % (what, (term / var_eps).max())
    for k in ("scale", "shift", "mean", "istd"):
        if got.get(k) is not None:
            assert not np.isnan(got[k]).any(), "%s: NaN left in %s" % (what, k)
    err = lambda k: np.abs(got[k].astype(np.float64) - ref[k])
    checks = [("scale", 3 * 2.0 ** -24 * np.abs(ref["scale"])),
              ("shift", 2.0 ** -22 * (np.abs(beta.astype(np.float64)) + np.abs(ref["mean"] * ref["scale"])))]
    if got.get("istd") is not None:
        assert (err("istd") <= 2.0 ** -23 * ref["istd"]).all(), what
        checks += [("istd", 1.25 * 2.0 ** -24 * ref["istd"]), ("mean", 2.0 ** -24 * np.abs(ref["mean"]))]
    if rm_given:
        n = got["count"]
        carry = float(np.float32(MOM)) * term * (n / (n - 1) if n > 1 else 1.0)
        assert (carry <= 2.0 ** -24 * ref["running_var_abs"]).all(), what
        checks += [("running_mean", 2.0 ** -22 * ref["running_mean_abs"]), ("running_var", 2.0 ** -22 * ref["running_var_abs"])]
    for k, bound in checks:
        e = err(k)
        _log("bn " + k, e, bound)
        bad = e > bound
        assert not bad.any(), "%s: %s beyond its bound in %d channels; worst err / bound %.3f at channel %d" % (
            what, k, int(bad.sum()), float((e / np.maximum(bound, 1e-300)).max()), int(np.argmax(e / np.maximum(bound, 1e-300))))


# ----------------------------------------------------------------------------- 3. gad_pool_finalize
POOL_FIN = [(C, G) for C in (4, 32, 64, 68, 128, 512) for G in (1, 15, 16, 17)] + [(4, 16400), (64, 16400)]


@pytest.mark.parametrize("C,G", POOL_FIN)
@pytest.mark.parametrize("train", (0, 1))
def test_pool_finalize(C, G, train):
    """keys as the GEMM epilogue leaves them (layer_reference.pool_keys) -> out / argmax / zmax bit-exact, keys reset; 16400 groups
    are above the 1024-workgroup cap (grid-stride loop), and every one of those workgroups finalises the BatchNorm slice while
    only the first may publish it: the running statistics must have moved by exactly one momentum step"""
    hip = _hip()
    rng = np.random.default_rng(3000 + C + G)
    off = L.groups(rng, rng.integers(1, 6, G))
    rows = int(off[-1])
    z = _quantised(rng, (rows, C))
    gamma = (rng.choice(np.array([1.0, -1.0, 0.5, -2.0, 0.0], np.float32), C) if not train else
             np.where(rng.random(C) < 0.15, 0.0, rng.normal(size=C))).astype(np.float32)
    beta = (rng.normal(size=C) * 0.5).astype(np.float32)
    gamma[:4] = (1.0, -1.0, 0.0, 0.0) if not train else (0.8, -1.3, 0.0, 0.0)
    beta[2], beta[3] = 0.25, -0.5                                    # gamma == 0 with shift > 0 and shift < 0
    keys = L.pool_keys(z, off, gamma)
    stride = C + 5 if G % 2 else C
    if train:
        z64 = z.astype(np.float64)
        ssum, ssq = L.replicate(z64.sum(0), stride, C, rng, 3.0), L.replicate((z64 * z64).sum(0), stride, C, rng, 3.0)
        m0, v0 = z64.mean(0), z64.var(0)
        rm0, rv0 = (m0 + 5.0).astype(np.float32), (3.0 * v0 + 1.0).astype(np.float32)   # a second step: 0.45 / 0.18 * var + 0.09 further
        ref = L.bn_finalize(ssum, ssq, stride, rows, gamma, beta, EPS, MOM, rm0, rv0)
        term = L.bn_f64_term(ssum, ssq, stride, rows, C)
        bsum, bsq, brm, brv = Buf(ssum), Buf(ssq), Buf(rm0), Buf(rv0)
        bsc, bsh, bmu, bis = (Buf(_nan32(C)) for _ in range(4))
    else:
        scale = (gamma * rng.choice(np.array([0.5, 1.0, 4.0], np.float32), C)).astype(np.float32)      # +- powers of two and 0
        shift = beta.copy()
        bsum = bsq = brm = brv = bmu = bis = None
        bsc, bsh = Buf(scale), Buf(shift)
    bg, bb, boff = Buf(gamma), Buf(beta), Buf(off)
    for variant in ("all", "null") if G <= 17 else ("all",):
        bk = Buf(keys)
        out = Buf(_nan32((G, C)))
        arg, zm = (Buf(np.full((G, C), -7, np.int32)), Buf(_nan32((G, C)))) if variant == "all" else (None, None)
        if train and variant == "null":
            brm, brv = Buf(rm0), Buf(rv0)
        hip.call("gad_pool_finalize", bk.ptr, C, G, boff.ptr, _P(bsum), _P(bsq), stride, hip.Dbl(rows), bg.ptr, bb.ptr, float(EPS),
                 float(MOM), _P(brm), _P(brv), bsc.ptr, bsh.ptr, _P(bmu), _P(bis), out.ptr, _P(arg), _P(zm))
        what = "pool_finalize C %d G %d train %d %s" % (C, G, train, variant)
        if train:
            got = {"scale": bsc.get("scale"), "shift": bsh.get("shift"), "mean": bmu.get("mean"), "istd": bis.get("istd"),
                   "running_mean": brm.get("running_mean"), "running_var": brv.get("running_var"), "count": rows}
            _check_bn(what, ref, term, got, beta, True)
            scale, shift = got["scale"], got["shift"]
            assert (np.sign(scale) == np.sign(gamma)).all()
            # one momentum step, not two: a second one would move the running statistics by another m * (1 - m) * (new - old)
            twice = np.abs(float(np.float32(MOM)) * (1 - float(np.float32(MOM))) * (ref["mean"] - rm0.astype(np.float64)))
            assert (twice > 1e4 * 2.0 ** -22 * ref["running_mean_abs"]).all()
            _same(what + ": stat_sum", bsum.get(), ssum)
            _same(what + ": stat_sq", bsq.get(), ssq)
        else:
            _same(what + ": scale (an input in eval mode)", bsc.get(), scale)
            _same(what + ": shift (an input in eval mode)", bsh.get(), shift)
        w_out, w_arg, w_zm = L.pool_finalize(keys, off, scale, shift, gamma)
        _same(what + ": out", out.get("out"), w_out)
        if variant == "all":
            _same(what + ": argmax", arg.get("argmax"), w_arg)
            _same(what + ": zmax", zm.get("zmax"), w_zm)
        _same(what + ": keys are reset", bk.get("keys"), np.zeros((G, C), np.uint64))
        p_out, p_arg = L.segment_pool(z, off, scale, shift)
        _same(what + ": out against the separate pool (a rounded fma is monotone)", w_out, p_out)
        if not train:
            _same(what + ": argmax against the separate pool", w_arg, p_arg)      # distinct raw values never share an activation
            dead = (w_out <= 0) | (scale == 0)[None, :]
            assert (w_arg[dead] == np.broadcast_to(off[:-1, None], w_arg.shape)[dead]).all() and dead.any()
            assert G < 15 or ((~dead).any() and (w_arg != np.broadcast_to(off[:-1, None], w_arg.shape)).any())
    for b, a in ((bg, gamma), (bb, beta), (boff, off)):
        _same("pool_finalize input", b.get(), a)


# ----------------------------------------------------------------------------- 4. gad_bn_finalize
BANDS = ((1e-8, 1e-6), (1e-6, 1e-4), (1e-2, 1.0), (1e2, 1e4), (1e-8, 1e4))     # variance bands of test_bn_running_update_and_eval_affine
KINDS = (0.0, 1.0, 1e2, 1e3, None)                                            # |mean| / std of a channel; None: a constant channel


def _bn_sums(rng, C, count, band, k0):
    """float64 sums over `count` rows built from float32 rows (at most 48 distinct ones, integer multiplicities), channel c of
    kind KINDS[(c + k0) % 5]"""
    rows = int(min(count, 48))
    w = np.ones(rows, np.int64)
    w[:] += (count - rows) // rows
    w[0] += count - int(w.sum())
    std = np.sqrt(np.exp(rng.uniform(np.log(band[0]), np.log(band[1]), C)))
    kind = (np.arange(C) + k0) % len(KINDS)
    ratio = np.array([0.0 if k is None else k for k in KINDS])[kind]
    const = kind == len(KINDS) - 1
    centre = ratio * std
    if count <= 2:              # one or two rows: the variance is (near) 0 whatever the band, and the float64 evaluation's
        centre, std = np.minimum(centre, 3.0), np.minimum(std, 1.0)   # cancellation term has only eps to stand against: |z| < 8
    z = (centre * rng.choice([-1.0, 1.0], C) + std * rng.normal(size=(rows, C))).astype(np.float32)
    z[:, const] = (1.0 + rng.random(int(const.sum()))).astype(np.float32)[None, :]
    zero = (ratio == 0) & ~const
    z[:, zero] -= z[:, zero].mean(0).astype(np.float32)[None, :] * (rows > 2)
    z64 = z.astype(np.float64)
    s1, s2 = (w[:, None] * z64).sum(0), (w[:, None] * z64 * z64).sum(0)
    s2[const] = (w.sum() * z64[0, const] ** 2) * (1 - 2.0 ** -48)            # the exact variance is slightly negative: clamped
    return s1, s2, const


@pytest.mark.parametrize("C", (1, 255, 257))
@pytest.mark.parametrize("count", (1, 2, 48, 213034))
@pytest.mark.parametrize("pad", (0, 5))
def test_bn_finalize_within_derived_bounds(C, count, pad):
    """bounds and their derivation: _check_bn"""
    hip = _hip()
    stride = C + pad
    clamped = 0
    for k0, band in enumerate(BANDS):
        rng = np.random.default_rng(4000 + C + count + pad + 17 * k0)
        s1, s2, const = _bn_sums(rng, C, count, band, k0)           # (C = 1: the one channel's kind changes with the band)
        ssum, ssq = L.replicate(s1, stride, C, rng, -2.5), L.replicate(s2, stride, C, rng, -2.5)
        assert (ssum.reshape(4, stride)[:, :C] < 0).any() or (s1 == 0).all()
        gamma = np.where(rng.random(C) < 0.1, 0.0, rng.normal(size=C)).astype(np.float32)
        beta = (rng.normal(size=C) * 0.5).astype(np.float32)
        rm0 = (rng.normal(size=C) * 2).astype(np.float32)
        rv0 = (np.exp(rng.uniform(np.log(band[0]), np.log(band[1]), C)) * 3 + 1e-3).astype(np.float32)
        ref = L.bn_finalize(ssum, ssq, stride, count, gamma, beta, EPS, MOM, rm0, rv0)
        term = L.bn_f64_term(ssum, ssq, stride, count, C)
        if const.any():
            assert ref["clamped"][const].all() and (ref["istd"][const] == 1 / np.sqrt(float(np.float32(EPS)))).all()
        clamped += int(ref["clamped"].sum())
        bsum, bsq, bg, bb = Buf(ssum), Buf(ssq), Buf(gamma), Buf(beta)
        brm, brv = Buf(rm0), Buf(rv0)
        o = [Buf(_nan32(C)) for _ in range(4)]
        hip.call("gad_bn_finalize", bsum.ptr, bsq.ptr, stride, bg.ptr, bb.ptr, C, hip.Dbl(count), float(EPS), float(MOM), brm.ptr,
                 brv.ptr, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr)
        got = {"scale": o[0].get("scale"), "shift": o[1].get("shift"), "mean": o[2].get("mean"), "istd": o[3].get("istd"),
               "running_mean": brm.get("running_mean"), "running_var": brv.get("running_var"), "count": count}
        what = "bn_finalize C %d count %d stride %d band %s" % (C, count, stride, band)
        _check_bn(what, ref, term, got, beta, True)
        # running statistics, mean and istd NULL: the same scale / shift, bit for bit
        o2 = [Buf(_nan32(C)) for _ in range(2)]
        hip.call("gad_bn_finalize", bsum.ptr, bsq.ptr, stride, bg.ptr, bb.ptr, C, hip.Dbl(count), float(EPS), float(MOM), None,
                 None, o2[0].ptr, o2[1].ptr, None, None)
        _same(what + ": scale without the nullable outputs", o2[0].get(), got["scale"])
        _same(what + ": shift without the nullable outputs", o2[1].get(), got["shift"])
        _same(what + ": running_mean (not passed)", brm.get(), got["running_mean"])
        for b, a in ((bsum, ssum), (bsq, ssq), (bg, gamma), (bb, beta)):
            _same(what + ": input", b.get(), a)
    assert clamped > 0


def test_bn_finalize_clamps_a_negative_variance():
    """Sums whose variance is negative beyond eps -- s2 / n - mean**2 = -2**-30 * mean**2 = -9.3e-4 for a channel at 1000, as a
    damaged accumulation could leave them -- must give istd = 1 / sqrt(eps), not the square root of a negative number.  The
    float64 evaluation is off by at most bn_f64_term = 2e-9, far less than the 9.3e-4 the variance lies below 0: the kernel sees
    a negative variance like the exact reference and clamps it to exactly 0, so the bounds of _check_bn hold without its
    precondition (which only serves variances that are not clamped)."""
    hip = _hip()
    rng = np.random.default_rng(4500)
    C, count, stride = 6, 48, 11
    v = np.array([1000.0, -1000.0, 512.0, 999.5, 1.0, -3.0])
    s1, s2 = count * v, count * v * v * (1 - 2.0 ** -30)
    s2[4:] = count * v[4:] ** 2 + np.array([0.5, 2.0]) * count          # two ordinary channels beside them
    ssum, ssq = L.replicate(s1, stride, C, rng, 1.0), L.replicate(s2, stride, C, rng, 1.0)
    gamma, beta = rng.normal(size=C).astype(np.float32), rng.normal(size=C).astype(np.float32)
    rm0, rv0 = rng.normal(size=C).astype(np.float32), rng.uniform(0.5, 2, C).astype(np.float32)
    ref = L.bn_finalize(ssum, ssq, stride, count, gamma, beta, EPS, MOM, rm0, rv0)
    term = L.bn_f64_term(ssum, ssq, stride, count, C)
    assert ref["clamped"][:4].all() and not ref["clamped"][4:].any()
    exact_var = np.r_[-2.0 ** -30 * v[:4] ** 2, ref["var"][4:]]
    assert (exact_var[:4] < -10 * float(np.float32(EPS))).all() and (term[:4] < 1e-4 * np.abs(exact_var[:4])).all()
    bsum, bsq, bg, bb, brm, brv = (Buf(a) for a in (ssum, ssq, gamma, beta, rm0, rv0))
    o = [Buf(_nan32(C)) for _ in range(4)]
    hip.call("gad_bn_finalize", bsum.ptr, bsq.ptr, stride, bg.ptr, bb.ptr, C, hip.Dbl(count), float(EPS), float(MOM), brm.ptr, brv.ptr,
             o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr)
    got = {"scale": o[0].get("scale"), "shift": o[1].get("shift"), "mean": o[2].get("mean"), "istd": o[3].get("istd"),
           "running_mean": brm.get("running_mean"), "running_var": brv.get("running_var"), "count": count}
    _same("clamped istd", got["istd"][:4], np.full(4, 1 / np.sqrt(float(np.float32(EPS))), np.float32))
    _check_bn("bn_finalize clamp", ref, np.where(ref["clamped"], 0.0, term), got, beta, True)


# ----------------------------------------------------------------------------- 5. gad_bn_bwd_coef
@pytest.mark.parametrize("C", (1, 255, 257))
@pytest.mark.parametrize("count", (1, 48, 213034))
@pytest.mark.parametrize("pad", (0, 5))
def test_bn_bwd_coef(C, count, pad):
    """P = scale bit for bit.  Q = float32(sc * (db - mu * is * dg) / n) and S = float32(sc * is * dg / n) are float64 evaluations
    rounded once: 2**-24 relative, plus what the float64 evaluation commits -- the replica sum ((r0 + r1) + r2) + r3 (partial sums
    below 0.9, 0.9, 1 x the total for layer_reference.replicate's shares: 2.8 * 2**-53), two products, the difference, the
    product with sc and the quotient (5 * 2**-53), all relative to |sc| * (|db| + |mu * is * dg|) / n: together < 2**-50 of it.
    The arena adds are float64 operations and are compared bit for bit."""
    hip = _hip()
    stride = C + pad
    rng = np.random.default_rng(5000 + C + count + pad)
    scale = np.where(rng.random(C) < 0.1, 0.0, rng.normal(size=C)).astype(np.float32)
    mean = (rng.normal(size=C) * 3).astype(np.float32)
    istd = (1 / np.sqrt(np.exp(rng.uniform(np.log(1e-8), np.log(1e4), C)) + EPS)).astype(np.float32)
    db = rng.normal(size=C) * 10.0 ** rng.uniform(-3, 2, C)
    dg = rng.normal(size=C) * 10.0 ** rng.uniform(-3, 2, C)
    rdb, rdg = L.replicate(db, stride, C, rng, 9.0), L.replicate(dg, stride, C, rng, 9.0)
    gg0, gb0 = rng.normal(size=C) * 3, rng.normal(size=C) * 3
    ref = L.bn_bwd_coef(rdb, rdg, stride, scale, mean, istd, count, gg0, gb0)
    ins = [Buf(a) for a in (rdb, rdg, scale, mean, istd)]
    for arena in (True, False):
        o = [Buf(_nan32(C)) for _ in range(3)]
        bgg, bgb = (Buf(gg0), Buf(gb0)) if arena else (None, None)
        hip.call("gad_bn_bwd_coef", ins[0].ptr, ins[1].ptr, stride, ins[2].ptr, ins[3].ptr, ins[4].ptr, C, hip.Dbl(count), o[0].ptr,
                 o[1].ptr, o[2].ptr, _P(bgg), _P(bgb))
        what = "bn_bwd_coef C %d count %d stride %d arena %d" % (C, count, stride, arena)
        _same(what + ": P", o[0].get("P"), ref["P"])
        for k, b in (("Q", o[1]), ("S", o[2])):
            got = b.get(k)
            assert not np.isnan(got).any()
            e, bound = np.abs(got.astype(np.float64) - ref[k]), 2.0 ** -24 * np.abs(ref[k]) + 2.0 ** -50 * ref["Q_f64"]
            _log("bn_bwd_coef " + k, e, bound)
            assert (e <= bound).all(), "%s: %s beyond its bound, worst err / bound %.3f" % (what, k, (e / np.maximum(bound, 1e-300)).max())
        if arena:
            _same(what + ": gacc_gamma", bgg.get("gacc_gamma"), ref["gacc_gamma"])
            _same(what + ": gacc_beta", bgb.get("gacc_beta"), ref["gacc_beta"])
    for b, a in zip(ins, (rdb, rdg, scale, mean, istd)):
        _same("bn_bwd_coef input", b.get(), a)


# ----------------------------------------------------------------------------- 6. gad_pool_bwd_stats
def _bwd_G(C):
    gl = 256 // min(C, 256)
    return (1, 3, 4 * gl - 1, 4 * gl + 1) + ({32: (16500,), 256: (2100,)}.get(C, ()))


POOL_BWD = [(C, G) for C in (32, 64, 128, 256, 512, 768) for G in _bwd_G(C)]


def _bwd_inputs(rng, C, G):
    rows = 3 * G + 2
    z = rng.normal(size=(rows, C)).astype(np.float32)
    arg = rng.integers(0, rows, (G, C)).astype(np.int32)
    scale = rng.normal(size=C).astype(np.float32)
    scale[3::7] = 0.0
    shift = (rng.normal(size=C) * 0.5).astype(np.float32)
    shift[3], shift[10] = 0.4, -0.4                                  # scale == 0 with a live and with a dead activation
    mean = (rng.normal(size=C) * 0.3).astype(np.float32)
    istd = rng.uniform(0.5, 3.0, C).astype(np.float32)
    dout = rng.normal(size=(G, C)).astype(np.float32)
    routed = z[arg, np.arange(C)[None, :]]
    # what gad_pool_finalize would have saved: the routed row's value, except in scale == 0 channels, where the routed row is
    # the group's first and zmax holds another row's value
    zmax = np.where((scale == 0)[None, :], z[(arg + 1) % rows, np.arange(C)[None, :]], routed).astype(np.float32)
    assert (zmax != routed)[:, scale == 0].any()
    return z, arg, scale, shift, mean, istd, dout, routed, zmax


def _scaled_gate(what, got, r64, r32, scale):
    """optim_reference.within with the errors taken relative to `scale` instead of max |r64|"""
    assert not np.isnan(got).any(), "%s: NaN left in an output" % what
    s = max(float(scale), 1e-300)
    e, e32 = float(np.abs(got - r64).max() / s), float(np.abs(r32.astype(np.float64) - r64).max() / s)
    _log(what, e, max(3.0 * e32, R.FLOOR))
    assert e <= max(3.0 * e32, R.FLOOR), "%s: max err / max sum|terms| = %.3e, float32 reference %.3e" % (what, e, e32)


def _run_pool_bwd(C, G, data, route, mask, what):
    hip = _hip()
    z, arg, scale, shift, mean, istd, dout, routed, zmax = data
    rng = np.random.default_rng(6100 + C + G)
    pitch, stride = C + 4, C + 5
    zp = {"zmax": zmax, "gather": routed, "both": routed}[route]
    r64 = L.pool_bwd_stats(dout, zp, scale, shift, mean, istd, np.float64)
    r32 = L.pool_bwd_stats(dout, zp, scale, shift, mean, istd, np.float32)
    pre_b, pre_g = rng.normal(size=4 * stride) + 3.0, rng.normal(size=4 * stride) - 3.0
    zin = _padded(z, pitch)
    bz, ba, bzm = (None if route == "zmax" else Buf(zin)), (None if route == "zmax" else Buf(arg)), (None if route == "gather" else Buf(zmax))
    vec = [Buf(a) for a in (scale, shift, mean, istd)]
    bd, bdb, bdg = Buf(dout), Buf(pre_b), Buf(pre_g)
    hip.call("gad_pool_bwd_stats", bd.ptr, _P(ba), G, C, _P(bz), pitch, vec[0].ptr, vec[1].ptr, vec[2].ptr, vec[3].ptr, bdb.ptr,
             bdg.ptr, stride, mask, _P(bzm))
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
    _same(what + ": dout", bd.get("dout"), r64["masked"] if mask else dout)
    for b, a in zip(vec + [bz, ba, bzm], (scale, shift, mean, istd, zin, arg, zmax)):
        if b is not None:
            _same(what + ": input", b.get(), a)
    assert r64["live"].any() and not r64["live"].all() or G == 1
    return res


@pytest.mark.parametrize("C,G", POOL_BWD)
def test_pool_bwd_stats(C, G):
    """routes: zmax alone (x_hat from zmax in EVERY channel -- include/gaddpg.h documents that deviation for gamma == 0), z + argmax
    alone (gathered), all three (zmax, except scale == 0 channels: gathered from the routed row)"""
    data = _bwd_inputs(np.random.default_rng(6000 + C + G), C, G)
    for route in ("zmax", "gather", "both"):
        for mask in (0, 1):
            _run_pool_bwd(C, G, data, route, mask, "pool_bwd_stats C %d G %d %s mask %d" % (C, G, route, mask))
    # the two readings of a scale == 0 channel differ in the reference: the "both" case can tell them apart
    z, arg, scale, shift, mean, istd, dout, routed, zmax = data
    a = L.pool_bwd_stats(dout, routed, scale, shift, mean, istd, np.float64)
    b = L.pool_bwd_stats(dout, zmax, scale, shift, mean, istd, np.float64)
    assert np.abs(a["dgamma"] - b["dgamma"])[3] > 1e-3 * a["abs_gamma"][3] > 0


@pytest.mark.parametrize("C", (32, 64, 128, 256, 512, 768))
def test_pool_bwd_stats_deterministic_mode(C):
    """the slot-plane form: the same gate, bit-identical on two calls, added to the pre-filled accumulators like the plain form"""
    hip = _hip()
    G = {32: 16500, 256: 2100}.get(C, 4 * (256 // min(C, 256)) + 1)
    data = _bwd_inputs(np.random.default_rng(6000 + C + G), C, G)
    hip.set_option("deterministic", 1)
    try:
        for mask in (0, 1):
            a = _run_pool_bwd(C, G, data, "both", mask, "pool_bwd_stats deterministic C %d G %d mask %d" % (C, G, mask))
            b = _run_pool_bwd(C, G, data, "both", mask, "pool_bwd_stats deterministic C %d G %d mask %d (again)" % (C, G, mask))
            _same("deterministic dbeta: two calls", a["dbeta"], b["dbeta"])
            _same("deterministic dgamma: two calls", a["dgamma"], b["dgamma"])
    finally:
        hip.set_option("deterministic", hip.get_option_default("deterministic"))


# ----------------------------------------------------------------------------- 7. the chain against torch autograd
def test_bn_chain_against_torch_autograd():
    """statistics -> gad_bn_finalize -> gad_affine_act -> probe gradient -> gad_bn_bwd_coef -> dZ = P * dY - w * (Q + S * z) against
    float64 torch.nn.functional.batch_norm + autograd on the expanded rows; yardstick: the same graph in float32 torch"""
    hip = _hip()
    rng = np.random.default_rng(7000)
    rows, C = 37, 8
    w = rng.integers(1, 4, rows)
    n = int(w.sum())
    z = (rng.normal(size=(rows, C)) * rng.uniform(0.3, 2, C) + rng.normal(size=C)).astype(np.float32)
    gamma, beta = rng.normal(size=C).astype(np.float32), (rng.normal(size=C) * 0.5).astype(np.float32)
    z64 = z.astype(np.float64)
    ssum = L.replicate((w[:, None] * z64).sum(0), C, C, rng)
    ssq = L.replicate((w[:, None] * z64 * z64).sum(0), C, C, rng)
    o = [Buf(_nan32(C)) for _ in range(4)]
    bz, bsum, bsq, bg, bb = Buf(z), Buf(ssum), Buf(ssq), Buf(gamma), Buf(beta)
    hip.call("gad_bn_finalize", bsum.ptr, bsq.ptr, C, bg.ptr, bb.ptr, C, hip.Dbl(n), float(EPS), float(MOM),
             None, None, o[0].ptr, o[1].ptr, o[2].ptr, o[3].ptr)
    by = Buf(_nan32((rows, C)))
    hip.call("gad_affine_act", bz.ptr, C, rows, C, o[0].ptr, o[1].ptr, 0, by.ptr, C)
    scale, mean, istd = o[0].get(), o[2].get(), o[3].get()
    probe = rng.normal(size=(n, C)).astype(np.float32)                 # one gradient per expanded row
    owner = np.repeat(np.arange(rows), w)
    dY = np.zeros((rows, C))
    np.add.at(dY, owner, probe.astype(np.float64))
    xhat = (z64 - mean.astype(np.float64)) * istd.astype(np.float64)
    dbeta, dgamma = dY.sum(0), (dY * xhat).sum(0)
    pre = rng.normal(size=C)
    bgg, bgb = Buf(pre), Buf(-pre)
    c = [Buf(_nan32(C)) for _ in range(3)]
    bdb, bdg = Buf(L.replicate(dbeta, C, C, rng)), Buf(L.replicate(dgamma, C, C, rng))
    hip.call("gad_bn_bwd_coef", bdb.ptr, bdg.ptr, C, o[0].ptr, o[2].ptr, o[3].ptr, C, hip.Dbl(n), c[0].ptr, c[1].ptr, c[2].ptr, bgg.ptr,
             bgb.ptr)
    P, Q, S = (b.get().astype(np.float64) for b in c)
    dZ = P * dY - w[:, None] * (Q + S * z64)
    res = {}
    for dt in (torch.float64, torch.float32):
        x = torch.tensor(np.repeat(z, w, axis=0), dtype=dt, requires_grad=True)
        g, b = torch.tensor(gamma, dtype=dt, requires_grad=True), torch.tensor(beta, dtype=dt, requires_grad=True)
        y = torch.nn.functional.batch_norm(x, None, None, g, b, True, MOM, EPS)
        y.backward(torch.tensor(probe, dtype=dt))
        dx = np.zeros((rows, C), y.detach().numpy().dtype)
        np.add.at(dx, owner, x.grad.numpy())
        res[dt] = (y.detach().numpy()[np.cumsum(w) - 1], dx, g.grad.numpy(), b.grad.numpy())
    r64, r32 = res[torch.float64], res[torch.float32]
    for k, (name, got) in enumerate((("Y", by.get("Y")), ("dZ", dZ), ("dgamma", bgg.get() - pre), ("dbeta", bgb.get() + pre))):
        e, e32 = R.within("chain: " + name, got, r64[k], r32[k])
        _log("chain " + name, e, max(3 * e32, R.FLOOR))
    _same("chain: P is the published scale", c[0].get(), scale)


# ----------------------------------------------------------------------------- 8. argument checks
def test_argument_checks_return_before_any_launch():
    """Host-side checks: every rejected call below would stay inside its buffers even if the check were missing.  Outputs start as
    NaN and must still be NaN afterwards."""
    rows, C, G = 12, 8, 3
    off = Buf(np.array([0, 4, 8, 12], np.int32))
    z = Buf(np.ones((rows, 32), np.float32))
    vec = Buf(np.ones(1024, np.float32))
    dbl = Buf(np.ones(4 * 1024))
    out, arg, key = Buf(_nan32(G * 1024)), Buf(np.ones(G * 1024, np.int32)), Buf(np.ones(G * 128, np.uint64))
    hip = _hip()
    D = hip.Dbl
    untouched = lambda: (_same("out", out.get(), _nan32(G * 1024)), _same("argmax", arg.get(), np.ones(G * 1024, np.int32)),
                         _same("keys", key.get(), np.ones(G * 128, np.uint64)))
    # gad_segment_pool
    sp = lambda **k: _rc("gad_segment_pool", k.get("z", z.ptr), k.get("pitch", 32), k.get("C", C), k.get("scale", vec.ptr),
                         k.get("shift", vec.ptr), k.get("off", off.ptr), k.get("G", G), k.get("out", out.ptr), arg.ptr)
    assert sp(z=None) == ERR_NULL and sp(off=None) == ERR_NULL and sp(out=None) == ERR_NULL
    assert sp(scale=None) == ERR_NULL and sp(shift=None) == ERR_NULL          # scale and shift come together
    assert sp(C=24) == ERR_SHAPE and sp(C=12) == ERR_SHAPE and sp(pitch=30) == ERR_SHAPE
    assert sp(C=16, pitch=8) == ERR_SHAPE and sp(C=32, pitch=28) == ERR_SHAPE and sp(C=-8) == ERR_SHAPE      # pitch < C: rows overlap
    assert sp(G=0) == OK and sp(C=0) == OK
    untouched()
    # gad_affine_act
    aa = lambda **k: _rc("gad_affine_act", k.get("z", z.ptr), k.get("zp", 32), k.get("rows", rows), k.get("C", C), vec.ptr, vec.ptr, 1,
                         k.get("out", out.ptr), k.get("op", 32))
    assert aa(z=None) == ERR_NULL and aa(out=None) == ERR_NULL
    assert aa(zp=7) == ERR_SHAPE and aa(op=7) == ERR_SHAPE and aa(C=-1) == ERR_SHAPE and aa(rows=-1) == ERR_SHAPE
    assert aa(rows=0) == OK and aa(C=0) == OK
    untouched()
    # gad_pool_finalize
    pf = lambda **k: _rc("gad_pool_finalize", k.get("key", key.ptr), k.get("C", C), k.get("G", G), k.get("off", off.ptr),
                         k.get("ssum", dbl.ptr), k.get("ssq", dbl.ptr), 1024, D(k.get("count", 12)), k.get("gamma", vec.ptr),
                         k.get("beta", vec.ptr), float(EPS), float(MOM), None, None, k.get("scale", out.ptr), k.get("shift", out.ptr), None,
                         None, k.get("out", out.ptr), arg.ptr, None)
    for name in ("key", "off", "gamma", "scale", "shift", "out", "ssq", "beta"):
        assert pf(**{name: None}) == ERR_NULL, name
    assert pf(C=6) == ERR_SHAPE and pf(C=-4) == ERR_SHAPE and pf(count=0) == ERR_SHAPE
    assert pf(G=0) == OK and pf(C=0) == OK
    untouched()
    # gad_pool_bwd_stats (C = 32 rows of 32 floats)
    pb = lambda **k: _rc("gad_pool_bwd_stats", k.get("dout", out.ptr), k.get("arg", arg.ptr), k.get("G", G), k.get("C", 32), k.get("z", z.ptr), 32,
                         k.get("scale", vec.ptr), k.get("shift", vec.ptr), k.get("mean", vec.ptr), k.get("istd", vec.ptr), k.get("db", dbl.ptr),
                         k.get("dg", dbl.ptr), 1024, 1, k.get("zmax", vec.ptr))
    for name in ("dout", "scale", "shift", "mean", "istd", "db", "dg"):
        assert pb(**{name: None}) == ERR_NULL, name
    assert pb(zmax=None, z=None) == ERR_NULL and pb(zmax=None, arg=None) == ERR_NULL
    assert pb(C=96) == ERR_SHAPE and pb(C=16) == ERR_SHAPE and pb(C=-32) == ERR_SHAPE
    assert pb(G=0) == OK and pb(C=0) == OK
    untouched()
    _same("accumulators", dbl.get(), np.ones(4 * 1024))
    # the BatchNorm entry points
    bf = lambda **k: _rc("gad_bn_finalize", k.get("ssum", dbl.ptr), k.get("ssq", dbl.ptr), 1024, k.get("gamma", vec.ptr), k.get("beta", vec.ptr),
                         k.get("C", C), D(k.get("count", 12)), float(EPS), float(MOM), None, None, k.get("scale", out.ptr), k.get("shift", out.ptr),
                         None, None)
    for name in ("ssum", "ssq", "gamma", "beta", "scale", "shift"):
        assert bf(**{name: None}) == ERR_NULL, name
    assert bf(count=0) == ERR_SHAPE and bf(count=0.5) == ERR_SHAPE and bf(C=-1) == ERR_SHAPE and bf(C=0) == OK
    bc = lambda **k: _rc("gad_bn_bwd_coef", k.get("db", dbl.ptr), k.get("dg", dbl.ptr), 1024, k.get("scale", vec.ptr), k.get("mean", vec.ptr),
                         k.get("istd", vec.ptr), k.get("C", C), D(k.get("count", 12)), k.get("P", out.ptr), k.get("Q", out.ptr), k.get("S", out.ptr),
                         None, None)
    for name in ("db", "dg", "scale", "mean", "istd", "P", "Q", "S"):
        assert bc(**{name: None}) == ERR_NULL, name
    assert bc(count=0) == ERR_SHAPE and bc(C=-1) == ERR_SHAPE and bc(C=0) == OK          # (count = 0 divided by it; C = 0 launched an empty grid)
    ea = lambda **k: _rc("gad_bn_eval_affine", k.get("gamma", vec.ptr), vec.ptr, vec.ptr, vec.ptr, k.get("C", C), float(EPS), k.get("scale", out.ptr),
                         out.ptr)
    assert ea(gamma=None) == ERR_NULL and ea(scale=None) == ERR_NULL and ea(C=-1) == ERR_SHAPE and ea(C=0) == OK
    ru = lambda **k: _rc("gad_bn_running_update", k.get("mean", vec.ptr), vec.ptr, vec.ptr, k.get("C", C), float(EPS), float(MOM), k.get("rm", out.ptr),
                         out.ptr)
    assert ru(mean=None) == ERR_NULL and ru(rm=None) == ERR_NULL and ru(C=-1) == ERR_SHAPE and ru(C=0) == OK
    untouched()
    torch.cuda.synchronize()
    assert b"C=-1" in hip.lib().gad_last_error()
