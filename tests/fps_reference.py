"""A plain numpy restatement of furthest point sampling as include/gaddpg.h (section A) and oracle/pn2_ref.c describe it -- the
yardstick's yardstick of tests/test_gpu_fps_forms.py, pinned on the CPU against oracle/cref.fps by tests/test_fps_reference.py --
with the distance and the skip norm as PARAMETERS, so that a test can ask what a kernel would pick had a compiler contracted a
product and a sum into one fused multiply-add, and finders of clouds on which that question has a different answer.

The operator.  float32 throughout, every operation rounded.  Pick 0 is index 0.  temp[k] starts at 1e10f.  A point with
|p|^2 < 1e-3f is skipped: never updated, never a candidate.  Each round takes d = |p_k - p_old|^2 of every other point, keeps
`d < temp[k] ? d : temp[k]` (a NaN d leaves temp alone; temp itself is never NaN and never above 1e10f) and picks the maximum of
temp by upstream's block reduction over tie_bs = pow2 <= min(N, 512) "threads": thread t = k mod tie_bs walks its points in
ascending k with a strict '>', holds (-1, index 0) if it has none, and a pairwise tree over strides tie_bs / 2 .. 1 lets slot t + s
replace slot t only if strictly larger.  No candidate at all: index 0.

Fused evaluations.  fma(a, a, c) is emulated as tests/test_gpu_fp_ops._fused_sqdist does it: the product of two float32 values is
exact in float64, the sum is formed there and rounded to float32."""
import collections
import functools

import numpy as np

f32 = np.float32
f64 = np.float64
SKIP = f32(1e-3)                 # skip iff |p|^2 < SKIP (upstream compares the float with the double 1e-3: the same set of floats)
BIG = f32(1e10)


def tie_bs(N):
    """upstream's opt_n_threads: the largest power of two <= min(N, 512)"""
    p = 1
    while p * 2 <= min(N, 512):
        p *= 2
    return p


def bitrev(t, bits):
    r = 0
    for i in range(bits):
        r |= ((t >> i) & 1) << (bits - 1 - i)
    return r


def tie_key(k, N):
    """among equal distances the smallest (bit-reversed thread, index) wins -- what the block reduction amounts to"""
    bs = tie_bs(N)
    return (bitrev(k % bs, bs.bit_length() - 1), k)


# ----------------------------------------------------------------------------- a*a + b*b + c*c, pinned and contracted
def _fma_sq(a, c):
    return (np.asarray(a, f64) * np.asarray(a, f64) + np.asarray(c, f64)).astype(f32)


def _sq(a):
    return (np.asarray(a, f32) * np.asarray(a, f32)).astype(f32)


def _sumsq_pinned(a, b, c):
    return ((_sq(a) + _sq(b)).astype(f32) + _sq(c)).astype(f32)


def _sumsq_yx(a, b, c):          # fma(b, b, a*a) + c*c
    return (_fma_sq(b, _sq(a)) + _sq(c)).astype(f32)


def _sumsq_xy(a, b, c):          # fma(a, a, b*b) + c*c
    return (_fma_sq(a, _sq(b)) + _sq(c)).astype(f32)


def _sumsq_z(a, b, c):           # fma(c, c, a*a + b*b)
    return _fma_sq(c, (_sq(a) + _sq(b)).astype(f32))


def _sumsq_yx_z(a, b, c):        # fma(c, c, fma(b, b, a*a))
    return _fma_sq(c, _fma_sq(b, _sq(a)))


def _sumsq_xy_z(a, b, c):        # fma(c, c, fma(a, a, b*b))
    return _fma_sq(c, _fma_sq(a, _sq(b)))


SUMSQ = collections.OrderedDict([("pinned", _sumsq_pinned), ("yx", _sumsq_yx), ("xy", _sumsq_xy), ("z", _sumsq_z),
                                 ("yx_z", _sumsq_yx_z), ("xy_z", _sumsq_xy_z)])
FUSED = tuple(n for n in SUMSQ if n != "pinned")


def sqnorm(variant="pinned"):
    """-> f(pts (..., 3)) = |p|^2 as `variant` evaluates it"""
    s = SUMSQ[variant]

    def f(pts):
        pts = np.asarray(pts, f32)
        with np.errstate(all="ignore"):
            return s(pts[..., 0], pts[..., 1], pts[..., 2])
    return f


def sqdist(variant="pinned"):
    """-> f(pts (..., 3), q (3,)) = |p - q|^2 as `variant` evaluates it (the difference is one rounded subtraction in all of them)"""
    s = SUMSQ[variant]

    def f(pts, q):
        with np.errstate(all="ignore"):
            d = (np.asarray(pts, f32) - np.asarray(q, f32)).astype(f32)
            return s(d[..., 0], d[..., 1], d[..., 2])
    return f


# ----------------------------------------------------------------------------- the operator
def _pick(temp, keep, bs):
    N = temp.size
    rows = -(-N // bs)
    v = np.full(rows * bs, -1, f32)
    v[:N] = np.where(keep, temp, f32(-1))
    v = v.reshape(rows, bs)
    t = np.arange(bs)
    r = v.argmax(axis=0)                                    # the first row with the thread's maximum: strict '>' in ascending k
    tv = v[r, t]
    ti = np.where(tv < 0, 0, r * bs + t)                    # a thread without a candidate holds (-1, 0)
    s = bs >> 1
    while s >= 1:
        take = tv[s:2 * s] > tv[:s]
        ti[:s] = np.where(take, ti[s:2 * s], ti[:s])
        tv[:s] = np.where(take, tv[s:2 * s], tv[:s])
        s >>= 1
    return int(ti[0])


def fps(xyz, M, sqdist=sqdist(), sqnorm=sqnorm()):
    """xyz (B, N, 3) -> idx (B, M) int32; M > N is allowed, as upstream allows it"""
    xyz = np.asarray(xyz, f32)
    B, N, _ = xyz.shape
    bs = tie_bs(N)
    idx = np.zeros((B, M), np.int32)
    for b in range(B):
        p = xyz[b]
        keep = ~(sqnorm(p) < SKIP)
        temp = np.full(N, BIG, f32)
        old = 0
        for j in range(1, M):
            d = sqdist(p, p[old])
            with np.errstate(invalid="ignore"):
                upd = keep & (d < temp)
            temp[upd] = d[upd]
            old = _pick(temp, keep, bs)
            idx[b, j] = old
    return idx


# ----------------------------------------------------------------------------- clouds
KINDS = ("random", "lattice", "lattice2", "duplicate", "skipped", "far6", "far20", "nan_mid", "nan_start", "inf", "inf_pair")
NONFINITE = ("nan_mid", "nan_start", "inf", "inf_pair", "far6", "far20")


def cloud(kind, N, seed=0):
    """one (N, 3) float32 cloud of a named kind, N >= 1"""
    rng = np.random.default_rng([seed, N, KINDS.index(kind)])
    xyz = (rng.random((N, 3)) * 0.1 + 0.2).astype(f32)
    if kind == "random":                                   # a block inside the skip ball and a run of exact duplicates
        xyz[N // 3: N // 3 + N // 7] *= f32(0.05)
        if N >= 8:
            xyz[N // 2: N // 2 + min(20, N // 4)] = xyz[min(5, N - 1)]
    elif kind in ("lattice", "lattice2"):                  # tests/test_gpu_ops.py::test_fps_exact_ties_on_a_lattice
        xyz = rng.integers(0, 6, size=(N, 3)).astype(f32) * f32(0.125) + f32(0.25)
        if kind == "lattice2":
            xyz[N // 2:] = xyz[: N - N // 2]               # every point twice
            xyz[::7] = 0.0                                 # a seventh of the cloud, the start point included, inside the skip ball
    elif kind == "duplicate":
        xyz[N // 2:] = xyz[: N - N // 2]
    elif kind == "skipped":
        xyz = (rng.random((N, 3)) * 0.015).astype(f32)
    elif kind == "far6":                                   # most d^2 > 1e10: temp stays 1e10f and the rounds are ties at it
        xyz = ((rng.random((N, 3)) - 0.5) * 2e6).astype(f32)
    elif kind == "far20":                                  # most d^2 overflow to inf
        xyz = ((rng.random((N, 3)) - 0.5) * 2e20).astype(f32)
    elif kind == "nan_mid":
        xyz[N // 2, 1] = np.nan
    elif kind == "nan_start":                              # every distance of the first round is NaN
        xyz[0, 2] = np.nan
    elif kind == "inf":
        xyz[N // 3, 0] = np.inf
    elif kind == "inf_pair":                               # inf - inf = NaN once one of the two is the pick
        xyz[(2 * N) // 3, 0] = np.inf
        xyz[N // 3, 0] = -np.inf
    else:
        raise ValueError(kind)
    return xyz


def tie_cloud(N, k1, k2, seed=0):
    """point 0 in the middle of a tight cluster, and ONE far point stored twice, at k1 and k2: the second pick is whichever of the
    two the tie rule prefers"""
    assert 0 < k1 < N and 0 < k2 < N and k1 != k2
    rng = np.random.default_rng([seed, N, k1, k2])
    xyz = (f32(0.5) + (rng.random((N, 3)) - 0.5) * 0.02).astype(f32)
    xyz[0] = 0.5
    xyz[k1] = xyz[k2] = (0.9, 0.8, 0.7)
    return xyz


# directed ties: (fps_cfg, form, T, N, k1, k2, winner).  k1 < k2 hold the same far point; where k1 mod T == k2 mod T one lane of the
# form (lane t owns k = s * T + t) holds both, at s1 < s2, and with R = tie_bs / T the order inside the lane is the bit-reversed
# s mod R first, then s.  winner 2: the HIGHER index wins because its s mod R bit-reverses lower; winner 1: the mirror case.  The
# last two put the pair into different wavefronts.
TIES = [(0, "<4,4>", 256, 1024, 256 + 9, 512 + 9, 2), (0, "<4,4>", 256, 1024, 9, 256 + 9, 1),                    # R = 2
        (0, "<16,4>", 256, 4096, 256 + 9, 512 + 9, 2), (0, "<16,4>", 256, 4096, 512 + 9, 768 + 9, 1),            # R = 2
        (3, "<16,1>", 64, 200, 64 + 5, 128 + 5, 2),                                                              # R = 2
        (3, "<16,1>", 64, 300, 64 + 9, 128 + 9, 2), (3, "<16,1>", 64, 300, 128 + 9, 192 + 9, 1),                 # R = 4
        (3, "<16,1>", 64, 1024, 64 + 9, 256 + 9, 2), (3, "<16,1>", 64, 1024, 256 + 9, 320 + 9, 1),               # R = 8
        (3, "<64,1>", 64, 4096, 64 * 9 + 9, 64 * 12 + 9, 2), (3, "<64,1>", 64, 4096, 64 * 12 + 9, 64 * 13 + 9, 1),   # R = 8, s >= R
        (4, "<8,2>", 128, 300, 128 + 9, 256 + 9, 2),                                                             # R = 2
        (4, "<8,2>", 128, 1024, 128 + 9, 256 + 9, 2), (4, "<8,2>", 128, 1024, 256 + 9, 384 + 9, 1),              # R = 4
        (4, "<32,2>", 128, 4096, 128 * 5 + 9, 128 * 6 + 9, 2), (4, "<32,2>", 128, 4096, 128 * 6 + 9, 128 * 7 + 9, 1),   # R = 4, s >= R
        (0, "<4,4>", 256, 1024, 1, 128, 2), (0, "<4,4>", 256, 1024, 2, 65, 1)]                                   # two wavefronts


# ----------------------------------------------------------------------------- contraction traps
SEARCH_BOUND = 64                # candidate sets a finder may draw before it gives up (and raises)
_PLACES = {"lane": lambda T: (5, 5 + T), "wave": lambda T: (5, 37), "block": lambda T: (5, 64 + 37)}


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _distance_pair(variant):
    """a start point c and two points A, B on a thin shell around it with pinned d2(A) > d2(B) and `variant` d2(A) < d2(B)"""
    pinned, fused = sqdist(), sqdist(variant)
    rng = np.random.default_rng([2024, FUSED.index(variant)])
    for _ in range(SEARCH_BOUND):
        c = (rng.random(3) * 0.4 + 0.3).astype(f32)
        pts = (c + _unit(rng, 1024) * 0.25).astype(f32)    # |p - c|^2 within a few ulp of 0.0625 for all of them
        P, F = pinned(pts, c), fused(pts, c)
        i, j = np.nonzero((P[:, None] > P[None, :]) & (F[:, None] < F[None, :]))
        if i.size:
            return c, pts[i[0]], pts[j[0]]
    raise RuntimeError("no pair of points that %r orders differently within %d candidate sets" % (variant, SEARCH_BOUND))


@functools.lru_cache(maxsize=None)
def distance_trap(variant, N, lanes, T=256):
    """-> (N, 3) cloud (read-only) whose second pick differs between the pinned model and the model that evaluates the distance
    as `variant`.  Point 0 is the start, the fillers lie within 0.01 of it, and the two far candidates A (the pinned pick) and B
    (the fused pick), a few ulp apart in squared distance, sit `lanes` apart for a kernel whose lane t owns k = s * T + t:
    "lane" = one lane, different s; "wave" = two lanes of one wavefront; "block" = two wavefronts."""
    a, b = _PLACES[lanes](T)
    if FUSED.index(variant) % 2:
        a, b = b, a
    if max(a, b) >= N:
        raise ValueError("N=%d is too small for placement %r with T=%d" % (N, lanes, T))
    c, A, B = _distance_pair(variant)
    rng = np.random.default_rng([7, N, a, b])
    xyz = (c + (rng.random((N, 3)) - 0.5) * 0.02).astype(f32)
    xyz[0], xyz[a], xyz[b] = c, A, B
    got, alt = fps(xyz[None], 3)[0], fps(xyz[None], 3, sqdist=sqdist(variant))[0]
    if not (got[1] == a and alt[1] == b):
        raise RuntimeError("distance_trap(%r): the cloud does not separate the evaluations (%r, %r)" % (variant, got, alt))
    xyz.flags.writeable = False
    return xyz


SkipTrap = collections.namedtuple("SkipTrap", "xyz index kept")


@functools.lru_cache(maxsize=None)
def _skip_points(variant):
    """two points at |p|^2 ~ 1e-3: one the pinned norm keeps while `variant` skips it, and one the other way round"""
    pinned, fused = sqnorm(), sqnorm(variant)
    rng = np.random.default_rng([1003, FUSED.index(variant)])
    found = {}
    for _ in range(SEARCH_BOUND):
        pts = (_unit(rng, 4096) * np.sqrt(1e-3)).astype(f32)
        P, F = pinned(pts) < SKIP, fused(pts) < SKIP
        for kept, mask in ((True, ~P & F), (False, P & ~F)):
            if kept not in found and mask.any():
                found[kept] = pts[np.nonzero(mask)[0][0]]
        if len(found) == 2:
            return found[True], found[False]
    raise RuntimeError("no point that %r puts on the other side of the skip threshold within %d candidate sets" % (variant, SEARCH_BOUND))


@functools.lru_cache(maxsize=None)
def skip_trap(variant, N=64, index=None):
    """-> two SkipTrap(xyz (N, 3) read-only, index, kept).  Point `index` (default N - 3) lies at |p|^2 ~ 1e-3, far from everything
    else (a tight cluster around point 0 at 0.5): the pinned norm keeps the first one's (it is the second pick) where `variant`
    skips it; the pinned norm skips the second one's (it is never picked) where `variant` keeps it."""
    index = max(N - 3, 1) if index is None else index
    assert 0 < index < N
    out = []
    for kept, pt in zip((True, False), _skip_points(variant)):
        rng = np.random.default_rng([11, N, index])
        xyz = (f32(0.5) + (rng.random((N, 3)) - 0.5) * 0.02).astype(f32)
        xyz[0] = 0.5
        xyz[index] = pt
        xyz.flags.writeable = False
        out.append(SkipTrap(xyz, index, kept))
    return tuple(out)
