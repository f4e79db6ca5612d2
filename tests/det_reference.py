"""Plain numpy references of what the deterministic mode (option "deterministic") promises for its GEMM-side ordered kernels, and the
seeded input sets the GPU gates of tests/test_gpu_deterministic_kernels.py run them on (pinned on the CPU by
tests/test_det_reference.py).

Exact operands.  The ordered kernels sum what a GEMM produced, so a reference would inherit the GEMM's rounding.  Here it has none:
dZ and W (for dW: dZ and the layer input) are integers in [-3, 3], every row's dZ times a power of two 2^e(r), e from 13 * {0 .. 5}
(scatter: e is the level of the row's point, see scatter_inputs; dW: of the row's split).
Every product and every partial sum inside the GEMM is then a multiple of 2^e below 2^24 * 2^e -- exactly representable in float32
in any order (`exact32` asserts it) -- and the row buffer, or a split's partial dW, is known exactly without restating a kernel.  What
still rounds is the sum ACROSS rows (float32 into dfeat, float64 into daction) or across splits (float64 into the arena): the sums
whose order the mode states.  The exponents are 13 apart because closer ones (5, 7, 9) leave the float64 sums identical in both
orders; `differs` measures, per input set, how much of the output the opposite order changes (the gates need >= 2 %: FLOOR).

The stated orders:
  dfeat[row_pt[r], c]          = fl32(dfeat + rowbuf[r, c]), rows ascending, from the caller's initial values
  daction[row_grp[r] // gps]   = initial + (the float64 sum of the sample's rows, ascending, formed from 0.0)
  arena (dW), linear form      = initial + (((p0 + p1) + p2) + ...) in float64 over the splits' partials, formed from 0.0
  arena (dW), tree form        = initial + the fixed tree of `reduce_tree` (more than 256 slots over at most 4096 columns)
  split s of a dW launch       = rows [s * chunk, (s + 1) * chunk) below the live count, chunk = ceil(ceil(live / splits) / 32) * 32"""
import numpy as np

from tests import group_reference as grp

f32, f64 = np.float32, np.float64
EXPONENTS = 13 * np.arange(6)
FLOOR = 0.02                   # least fraction of the written elements the opposite order must change (a condition on the inputs)
INT_MAX = 2 ** 31 - 1


def exact32(a):
    """a float64 array that is exactly representable in float32 -> that float32 array (asserted)"""
    a = np.asarray(a, f64)
    b = a.astype(f32)
    assert np.array_equal(b.astype(f64), a), "operands are not exact in float32"
    return b


def ints(rng, shape, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, shape).astype(f32)


def wide_values(rng, shape):
    """non-zero float64 initial values of a float64 accumulator, +-(1 .. 1023) * 2^k with k over 0 .. 70: whatever the size of the
    sum that lands on an element, many initial values are of its size -- small ones alone would vanish under a sum near 2^75, and
    a launch that overwrote them would pass"""
    return rng.integers(1, 1024, shape) * rng.choice([-1, 1], shape) * 2.0 ** rng.integers(0, 71, shape)


def row_exponents(rng, rows):
    return EXPONENTS[rng.integers(0, EXPONENTS.size, rows)]


def order_free(A, B, per_row=True):
    """every partial sum of A @ B, in any order, is exact in float32: with each row of A (per_row) or all of A a small integer
    matrix times ONE power of two and B integers, every product is an integer multiple of that power and
    |partial sum| <= sum |terms| stays below 2^24 of it"""
    A, B = np.asarray(A, f64), np.asarray(B, f64)
    top = np.abs(A).max(1, keepdims=True) if per_row else np.abs(A).max(keepdims=True)
    scale = 2.0 ** (np.frexp(np.where(top > 0, top, 1.0))[1] - 3)     # |ints| <= 3: at most a quarter of the power of two in front
    m = A / scale
    return bool(np.array_equal(m, np.round(m)) and np.abs(m).max() <= 12 and np.array_equal(B, np.round(B)) and
                (np.abs(m) @ np.abs(B)).max() < 2 ** 24)


# ----------------------------------------------------------------------------- A. the ordered scatter
def rowbuf(G, W, kv):
    """the rows' input gradients (rows, kv) = G (rows, n_out) @ W (n_out, Kp)[:, :kv], exact"""
    assert order_free(G, np.asarray(W)[:, :kv])
    return exact32(np.asarray(G, f64) @ np.asarray(W, f64)[:, :kv])


def scatter(rb, row_pt, row_grp, gps, feat_c, act_c, dfeat0, daction0, live, order="asc", drop_last=False, zero_start=False):
    """gad_gemm_dx, epilogue 1, deterministic.  rb: the exact row buffer; dfeat0 (npts, feat_c) float32 / daction0 (nsmp, act_c)
    float64: the initial values (None: that output is absent).  -> (dfeat, daction).  order "desc", drop_last (the last live row
    missing) and zero_start (the initial values ignored) are the negative controls."""
    live = rb.shape[0] if live is None else min(int(live), rb.shape[0])
    n = live - 1 if drop_last and live > 0 else live
    rows = range(n) if order == "asc" else range(n - 1, -1, -1)
    dfeat = daction = None
    if dfeat0 is not None:
        dfeat = np.zeros_like(dfeat0) if zero_start else dfeat0.copy()
        for r in rows:
            p = row_pt[r]
            dfeat[p] = dfeat[p] + rb[r, :feat_c]                    # one rounded float32 addition per element
    if daction0 is not None:
        daction = np.zeros_like(daction0) if zero_start else daction0.copy()
        acc = np.zeros_like(daction0)
        for r in rows:
            s = row_grp[r] // gps
            acc[s] = acc[s] + rb[r, feat_c + 3:feat_c + 3 + act_c].astype(f64)
        hit = np.zeros(daction0.shape[0], bool)
        hit[np.asarray(row_grp[:n]) // gps] = True
        daction[hit] = daction[hit] + acc[hit]                      # the run sum is formed from 0.0, then added once
    return dfeat, daction


def written(row_pt, row_grp, gps, npts, nsmp, live):
    """masks of the dfeat rows / daction rows some live row reaches"""
    live = len(row_pt) if live is None else live
    p, s = np.zeros(npts, bool), np.zeros(nsmp, bool)
    p[row_pt[:live]] = True
    s[np.asarray(row_grp[:live]) // gps] = True
    return p, s


def run_heads(row_pt, row_grp, live=None, strict=True):
    """the cut rule, restated directly: group g starts a run when every point the rows of the groups before it reference is below
    (strict) every point the rows from g on reference.  -> bool (G,) over the group ids 0 .. row_grp[live - 1]; an empty group
    takes the bounds INT_MAX / -1.  (strict=False: the `<=` a wrong kernel would use.)"""
    live = len(row_pt) if live is None else live
    if live <= 0:
        return np.zeros(0, bool)
    G = int(row_grp[live - 1]) + 1
    gmin, gmax = np.full(G, INT_MAX, np.int64), np.full(G, -1, np.int64)
    np.minimum.at(gmin, row_grp[:live], row_pt[:live])
    np.maximum.at(gmax, row_grp[:live], row_pt[:live])
    pre = np.concatenate([[-1], np.maximum.accumulate(gmax)[:-1]])
    suf = np.minimum.accumulate(gmin[::-1])[::-1]
    head = pre < suf if strict else pre <= suf
    head[0] = True
    return head


def _ball_maps(rng, B=3, N=64, M=8, S=8, radius=0.45):
    """rows of gad_rows_from_ball_query's reference for B clouds of N points, M centres each (centres = points of the cloud)"""
    xyz = rng.random((B, N, 3)).astype(f32)
    new = np.stack([xyz[b][np.sort(rng.choice(N, M, replace=False))] for b in range(B)])
    idx, cnt = grp.ball_query(new, xyz, radius, S)
    off, row_pt, row_grp, _, n_rows = grp.rows_from_ball_query(idx, cnt, M, N, S)
    return dict(off=off, local=(row_pt - (row_grp // M) * N).astype(np.int32), row_grp=row_grp, B=B, N=N, M=M)


def _maps(name, rng):
    """-> dict(row_pt, row_grp int32, npts, nsmp, gps, live)"""
    B, N, M = 3, 64, 8
    if name in ("samples", "live_in_group", "live0", "live_short_sample", "cols260", "dfeat_only", "daction_only"):
        m = _ball_maps(rng)
        row_pt = (m["row_grp"] // M) * N + m["local"]
        live, off = None, m["off"]
        if name == "live_in_group":                      # ends inside a group and inside a 64-row tile
            g = next(g for g in range(B * M // 2, B * M) if off[g + 1] - off[g] >= 3 and (off[g] + 1) % 64 not in (0, 1))
            live = int(off[g]) + 1
        elif name == "live0":
            live = 0
        elif name == "live_short_sample":                # the last sample keeps 3 of its 8 groups
            live = int(off[(B - 1) * M + 3])
        return dict(row_pt=row_pt, row_grp=m["row_grp"], npts=B * N, nsmp=B, gps=M, live=live)
    if name == "touching":                               # the last point of sample s is the first point of sample s + 1
        m = _ball_maps(rng)
        pt, gr = [], []
        for g in range(B * M):
            s = g // M
            loc = list(m["local"][m["off"][g]:m["off"][g + 1]])
            if g % M == 0 and s > 0:
                loc = [0] * 64 + loc                     # 64 rows on the shared point, on the far side of the boundary
            if g % M == M - 1 and s < B - 1:
                loc = loc + [N - 1] * 64                 # and 64 on the near side
            pt += [s * (N - 1) + v for v in loc]
            gr += [g] * len(loc)
        return dict(row_pt=np.array(pt, np.int32), row_grp=np.array(gr, np.int32), npts=B * (N - 1) + 1, nsmp=B, gps=M, live=None)
    if name == "descending":                             # sample s on the point range of sample B - 1 - s
        m = _ball_maps(rng)
        row_pt = (B - 1 - m["row_grp"] // M) * N + m["local"]
        return dict(row_pt=row_pt, row_grp=m["row_grp"], npts=B * N, nsmp=B, gps=M, live=None)
    if name in ("groups600", "groups513", "groups600_border"):
        G = 513 if name == "groups513" else 600
        lens = []                                        # runs of 1, 2, 3, 2, 1, ... groups: cuts at every offset inside a chunk of 3
        while sum(lens) < G:
            lens.append(min((1, 2, 3, 2)[len(lens) % 4], G - sum(lens)))
        if name == "groups600_border":                   # groups 299 and 300 in one run: no cut at the chunk border 300, cuts at 299 and 301
            starts = np.cumsum([0] + lens)
            cut = set(int(v) for v in starts[:-1])
            cut.discard(300)
            cut |= {299, 301}
            edges = sorted(cut) + [G]
            lens = [b - a for a, b in zip(edges[:-1], edges[1:])]
        pt, gr, g = [], [], 0
        for k, n in enumerate(lens):
            base = 4 * k
            for j in range(n):                           # every group of a run touches the run's lowest and highest point: no cut inside
                mid = [base + 1 + int(v) for v in rng.integers(0, 2, int(rng.integers(0, 3)))]
                pt += [base + 3] + mid + [base]
                gr += [g] * (2 + len(mid))
                g += 1
        return dict(row_pt=np.array(pt, np.int32), row_grp=np.array(gr, np.int32), npts=4 * len(lens), nsmp=(G + 3) // 4, gps=4, live=None)
    if name == "runs1100":                               # more runs than workgroups: one private point and two rows per group
        G = 1100
        row_grp = np.repeat(np.arange(G), 2).astype(np.int32)
        return dict(row_pt=row_grp.copy(), row_grp=row_grp, npts=G, nsmp=G, gps=1, live=None)
    if name in ("gaps", "sparse"):
        G = 200 if name == "sparse" else 50
        n = rng.integers(1, 3, G) if name == "sparse" else rng.integers(2, 6, G)
        ids = 3 * np.arange(G) if name == "sparse" else 2 + np.arange(G) + 2 * (np.arange(G) // 5)      # sparse: last id + 1 > rows
        row_grp = np.repeat(ids, n).astype(np.int32)
        row_pt = (np.repeat(np.arange(G) // 2 * 3, n) + rng.integers(0, 3, row_grp.size)).astype(np.int32)   # two groups share 3 points
        gps = 12 if name == "sparse" else 4
        return dict(row_pt=row_pt, row_grp=row_grp, npts=3 * (G // 2), nsmp=int(ids[-1]) // gps + 1, gps=gps, live=None)
    if name == "one_row":
        return dict(row_pt=np.array([2], np.int32), row_grp=np.array([0], np.int32), npts=4, nsmp=1, gps=1, live=None)
    raise KeyError(name)


SCATTER = ("samples", "touching", "descending", "groups600", "groups513", "groups600_border", "runs1100", "gaps", "sparse",
           "live_in_group", "live0", "live_short_sample", "cols260", "dfeat_only", "daction_only", "one_row")
# input sets in which no destination sums enough terms for an order to exist (nothing is written / one term): the floor cannot apply
UNORDERED = ("live0", "one_row")


def scatter_inputs(name):
    """the whole input set of scatter case `name`: the row maps of _maps, G (rows, n_out) and W (n_out, Kp) exact operands, non-zero
    initial dfeat (float32) / daction (float64), the layer's shape"""
    rng = np.random.default_rng(1000 + SCATTER.index(name))
    m = _maps(name, rng)
    rows = m["row_pt"].size
    feat_c, act_c, Kp, n_out = 4, 6, 16, 24
    if name == "cols260":
        feat_c, Kp, n_out = 260, 272, 8
    if name == "dfeat_only":
        act_c, Kp = 0, 8
    kv = feat_c + 3 + act_c
    # e(r): the level of the row's POINT, and the point's initial value 24 significant bits at twice that level's unit -- a float32
    # sum of few terms rounds differently in the two orders only where its terms overlap partly; with a level per row and small
    # initial values the opposite order changed 0.3 - 2 % of dfeat at 1 - 8 rows per point, with these 10 - 30 %.  A sample's rows
    # still span every level, which is what its float64 sum needs
    level = row_exponents(rng, m["npts"])
    last = (rows if m["live"] is None else m["live"]) - 1
    if last >= 0:                                        # (the last live row at the top level: no sum can swallow it whole, so
        level[m["row_pt"][last]] = EXPONENTS[-1]         # a reference without it differs in dfeat and in daction)
    G = exact32(ints(rng, (rows, n_out)).astype(f64) * 2.0 ** level[m["row_pt"]][:, None])
    W = ints(rng, (n_out, Kp))
    W[:, kv:] = 0
    sh = (m["npts"], feat_c)
    dfeat0 = exact32(rng.integers(2 ** 23, 2 ** 24, sh) * rng.choice([-1, 1], sh) * 2.0 ** (level[:, None] + 1))
    daction0 = wide_values(rng, (m["nsmp"], act_c)) if act_c else None
    if name == "daction_only":
        dfeat0 = None
    assert (np.diff(m["row_grp"]) >= 0).all() and m["row_pt"].max() < m["npts"] and m["row_grp"].max() // m["gps"] < m["nsmp"]
    return dict(m, name=name, rows=rows, feat_c=feat_c, act_c=act_c, Kp=Kp, kv=kv, n_out=n_out, G=G, W=W, dfeat0=dfeat0, daction0=daction0)


def scatter_reference(c, **alter):
    rb = rowbuf(c["G"], c["W"], c["kv"])
    return scatter(rb, c["row_pt"], c["row_grp"], c["gps"], c["feat_c"], c["act_c"], c["dfeat0"], c["daction0"], c["live"], **alter)


def differs(a, b, mask=None):
    """(elements whose bits differ, elements looked at) over the rows of `mask`"""
    if a is None:
        return 0, 0
    if mask is not None:
        a, b = a[mask], b[mask]
    if a.size == 0:
        return 0, 0
    return int((a.view(np.uint8).reshape(a.size, -1) != b.view(np.uint8).reshape(b.size, -1)).any(1).sum()), int(a.size)


def scatter_sensitivity(c):
    """-> {output: (differing, written, ordered)} of the descending-order reference against the ascending one.  ordered: some
    destination of the output sums three terms or more -- two rows on top of dfeat's initial value, three rows of a sample (the run
    sum starts from 0.0 and is added once: two rows commute) -- so that an order exists for the floor to be asked of"""
    asc, desc = scatter_reference(c), scatter_reference(c, order="desc")
    p, s = written(c["row_pt"], c["row_grp"], c["gps"], c["npts"], c["nsmp"], c["live"])
    live = c["rows"] if c["live"] is None else c["live"]
    most_pt = int(np.bincount(c["row_pt"][:live], minlength=1).max())
    most_smp = int(np.bincount(c["row_grp"][:live] // c["gps"], minlength=1).max())
    return {"dfeat": differs(asc[0], desc[0], p) + (most_pt >= 2,), "daction": differs(asc[1], desc[1], s) + (most_smp >= 3,)}


# ----------------------------------------------------------------------------- B. the ordered dW reduce
def dw_chunk(live, splits):
    """rows per split of a generic dW launch: ceil(ceil(live / splits) / 32) * 32 (include/gaddpg.h, row_splits)"""
    per = -(-live // splits)
    return -(-per // 32) * 32


def reduce_linear(parts, order="asc"):
    """(slots, ...) -> the float64 sum over the slots in ascending (descending) order, formed from 0.0"""
    s = np.zeros(parts.shape[1:], f64)
    for i in (range(parts.shape[0]) if order == "asc" else range(parts.shape[0] - 1, -1, -1)):
        s = s + parts[i].astype(f64)
    return s


def reduce_tree(parts, order="asc"):
    """ordered_reduce_tree_kernel: thread t sums the slots t, t + 256, ... in order, then red[t] += red[t + w] for w = 128 .. 1.
    order "desc" (the negative control): every thread's slots backwards and the tree's levels in the opposite order, neighbours
    first (red[t] += red[t + w] over t = 0, 2w, 4w, ... for w = 1 .. 128).  Reversing the slots alone is no control: with n slots it
    moves thread t's set of slots to thread (n - 1 - t) mod 256, which keeps every pair 128, 64, ... apart paired -- the same
    tree with the operands of commutative additions swapped, the same bits."""
    red = np.zeros((256,) + parts.shape[1:], f64)
    for i in (range(parts.shape[0]) if order == "asc" else range(parts.shape[0] - 1, -1, -1)):
        red[i % 256] = red[i % 256] + parts[i].astype(f64)
    if order == "asc":
        w = 128
        while w > 0:
            red[:w] = red[:w] + red[w:2 * w]
            w //= 2
    else:
        w = 1
        while w < 256:
            red[::2 * w] = red[::2 * w] + red[w::2 * w]
            w *= 2
    return red[0]


def ordered_reduce(parts, ncols, order="asc"):
    """the form gad_ordered_reduce takes for `ncols` columns over parts.shape[0] slots"""
    return reduce_tree(parts, order) if ncols <= 4096 and parts.shape[0] > 256 else reduce_linear(parts, order)


# name -> dict(splits, chunk | live, groups n_out, c_in, Kp, gather, static extra rows)
DW = {
    "splits3": dict(splits=3, chunk=64),
    "splits40": dict(splits=40, chunk=32),
    "splits300.tree": dict(splits=300, chunk=32),
    "splits300.linear": dict(splits=300, chunk=32, c_in=60, Kp=64),          # 72 * 64 > 4096 columns: linear although > 256 slots
    "splits40.past_live": dict(splits=40, chunk=32, live_splits=20),        # the last 20 splits lie past the live rows: zeros
    "two_groups": dict(splits=3, chunk=64, n_out=[36, 72]),
    "gathered": dict(splits=3, chunk=64, gather=True, Kp=16),
    "tile.n24": dict(splits=3, chunk=64, n_out=[24]),                       # nmax <= 32: 32 x 128
    "tile.k20": dict(splits=3, chunk=64, c_in=20, Kp=24),                   # k_used <= 32: 128 x 32
    "splits1": dict(splits=1, live=700, flat=True),
    "splits0": dict(splits=0, live=700, flat=True),
}


def dw_inputs(name):
    """the input set of dW case `name`: X (the layer input, integers), dZ (integers times one power of two per split), the arena's
    non-zero initial values.  flat: every exponent 0 (row_splits 1 / 0: only the exact integer sum is promised)"""
    d = dict(n_out=[72], c_in=36, Kp=40, gather=False, flat=False, live_splits=None)
    d.update(DW[name])
    rng = np.random.default_rng(2000 + sorted(DW).index(name))
    splits = d["splits"]
    if "live" in d:
        live = d["live"]
    else:
        live = (d["live_splits"] or splits) * d["chunk"]
        assert dw_chunk(live, splits) == d["chunk"]
    rows = live + 37                                                        # static bound: the live count ends inside a tile row range
    C = sum(d["n_out"])
    e = np.zeros(rows, np.int64)
    if not d["flat"]:
        per = EXPONENTS[rng.integers(0, EXPONENTS.size, splits)]
        if splits == 3:                                                     # three terms round twice only where two of them overlap
            per = rng.permutation(np.array([0, 52, 52]))                   # partly (a gap of 52 under 53 bits) and the third moves the binade
        e = per[np.minimum(np.arange(rows) // d["chunk"], splits - 1)]
    dZ = exact32(ints(rng, (rows, C)).astype(f64) * 2.0 ** e[:, None])
    out = dict(d, name=name, rows=rows, live=live, C=C, dZ=dZ)
    if d["gather"]:
        m = _maps("gaps", rng)
        n = m["row_pt"].size
        rep = -(-rows // n)                                                 # the maps repeated over the rows, group ids kept ascending
        out.update(row_pt=np.tile(m["row_pt"], rep)[:rows].copy(), npts=m["npts"], gps=4, feat_c=4, act_c=6)
        out["row_grp"] = np.sort(np.tile(m["row_grp"], rep)[:rows]).astype(np.int32)
        out["nsmp"] = int(out["row_grp"].max()) // 4 + 1
        ngrp = out["nsmp"] * 4
        out.update(feat=ints(rng, (m["npts"], 4)), src=ints(rng, (m["npts"], 3), 0, 2), ctr=ints(rng, (ngrp, 3), 0, 1),
                   action=ints(rng, (out["nsmp"], 6)))
        X = np.concatenate([out["feat"][out["row_pt"]], out["src"][out["row_pt"]] - out["ctr"][out["row_grp"]],
                            out["action"][out["row_grp"] // 4]], 1)
        out.update(k_used=13, X=[X], zin_off=[0])
    else:
        ng = len(d["n_out"])
        out["zin_off"] = [i * d["c_in"] for i in range(ng)]
        out["zin"] = ints(rng, (rows, ng * d["c_in"]))
        out.update(k_used=d["c_in"], X=[out["zin"][:, o:o + d["c_in"]] for o in out["zin_off"]])
    out["dz_off"] = [int(v) for v in np.cumsum([0] + d["n_out"][:-1])]
    out["w_off"] = [int(v) for v in np.cumsum([0] + [n * d["Kp"] for n in d["n_out"][:-1]])]
    out["total"] = sum(n * d["Kp"] for n in d["n_out"]) + 16
    out["gacc0"] = wide_values(rng, out["total"]) if not d["flat"] else rng.integers(1, 64, out["total"]) * rng.choice([-1, 1], out["total"]) / 8.0
    return out


def dw_partials(c, g):
    """group g's per-split partial dW (splits, n_out, k_used), each exact; a split past the live rows is zeros"""
    n, do, splits = c["n_out"][g], c["dz_off"][g], max(c["splits"], 1)
    chunk = dw_chunk(c["live"], splits)
    parts = np.zeros((splits, n, c["k_used"]), f32)
    for s in range(splits):
        a, b = s * chunk, min((s + 1) * chunk, c["live"])
        if a < b:
            d, x = c["dZ"][a:b, do:do + n], c["X"][g][a:b]
            assert order_free(d.T, x, per_row=False)                 # the split's dZ rows share one power of two
            parts[s] = exact32(d.astype(f64).T @ x.astype(f64))
    return parts


def dw_reference(c, order="asc", drop_split=None, zero_start=False):
    """the arena after the call: initial + the ordered sum of the partials in the form the shape selects (order "desc": the slots
    backwards, see reduce_tree for the tree form; drop_split: that split missing; zero_start: initial values ignored)"""
    out = np.zeros_like(c["gacc0"]) if zero_start else c["gacc0"].copy()
    for g, (n, wo) in enumerate(zip(c["n_out"], c["w_off"])):
        parts = dw_partials(c, g)
        if drop_split is not None:
            parts[drop_split] = 0
        if c["flat"]:                                               # (row_splits 1 / 0: any grouping gives this exact integer sum)
            s = c["dZ"][:c["live"], c["dz_off"][g]:c["dz_off"][g] + n].astype(f64).T @ c["X"][g][:c["live"]].astype(f64)
        else:
            s = ordered_reduce(parts, n * c["Kp"], order)
        blk = out[wo:wo + n * c["Kp"]].reshape(n, c["Kp"])
        blk[:, :c["k_used"]] = blk[:, :c["k_used"]] + s
    return out


def dw_mask(c):
    m = np.zeros(c["total"], bool)
    for n, wo in zip(c["n_out"], c["w_off"]):
        m[wo:wo + n * c["Kp"]].reshape(n, c["Kp"])[:, :c["k_used"]] = True
    return m


# ----------------------------------------------------------------------------- C. slot statistics: exact integer sums
def stats_forward(zin_groups, W_groups, row_w, live):
    """float64 (exact) stat_sum / stat_sq of every group's columns: sum_r w z, sum_r w z^2 over the live rows; and the largest
    |w z^2| summed over 128 rows (must stay below 2^24: the in-block float32 sums are then exact in any order)"""
    s, q, worst = [], [], 0.0
    w = np.ones(live, f64) if row_w is None else row_w[:live].astype(f64)
    for x, W in zip(zin_groups, W_groups):
        z = x[:live].astype(f64) @ W.astype(f64).T
        s.append((w[:, None] * z).sum(0))
        q.append((w[:, None] * z * z).sum(0))
        if live:
            worst = max(worst, float((w[:, None] * z * z).max()) * 128)
    return np.concatenate(s), np.concatenate(q), worst
