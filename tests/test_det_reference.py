"""Pins tests/det_reference.py on the CPU: the references of the deterministic mode's ordered kernels against straight scalar
loops, the exactness of every operand set the GPU gates use, the properties each row map is there for (where its cuts fall), and
the condition the gates rest on -- for every input set, the opposite order of summation changes at least 2 % of the written elements
(FLOOR: a property of the inputs, no tolerance).  No GPU, no library."""
import numpy as np
import pytest

from tests import det_reference as D

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def scatter_sets():
    return {n: D.scatter_inputs(n) for n in D.SCATTER}


@pytest.fixture(scope="module")
def dw_sets():
    return {n: D.dw_inputs(n) for n in D.DW}


# ----------------------------------------------------------------------------- the references against scalar loops
def test_scatter_reference_is_the_scalar_loop():
    rng = np.random.default_rng(7)
    rows, npts, nsmp, gps, fc, ac = 40, 5, 2, 3, 2, 2
    rb = (rng.integers(-600, 600, (rows, fc + 3 + ac)) * 2.0 ** (13 * rng.integers(0, 6, (rows, 1)))).astype(f32)
    pt, gr = rng.integers(0, npts, rows).astype(np.int32), np.sort(rng.integers(0, nsmp * gps, rows)).astype(np.int32)
    d0, a0 = rng.normal(size=(npts, fc)).astype(f32), rng.normal(size=(nsmp, ac))
    for live in (rows, 17, 0):
        for order in ("asc", "desc"):
            d, a = D.scatter(rb, pt, gr, gps, fc, ac, d0, a0, live, order=order)
            wd, acc = d0.copy(), np.zeros((nsmp, ac))
            for r in (range(live) if order == "asc" else reversed(range(live))):
                for c in range(fc):
                    wd[pt[r], c] = f32(wd[pt[r], c] + rb[r, c])
                for j in range(ac):
                    acc[gr[r] // gps, j] = acc[gr[r] // gps, j] + f64(rb[r, fc + 3 + j])
            assert np.array_equal(d, wd) and np.array_equal(a, a0 + acc)
    d, a = D.scatter(rb, pt, gr, gps, fc, ac, d0, a0, rows, drop_last=True)
    d2, a2 = D.scatter(rb[:-1], pt[:-1], gr[:-1], gps, fc, ac, d0, a0, rows - 1)
    assert np.array_equal(d, d2) and np.array_equal(a, a2)
    d, a = D.scatter(rb, pt, gr, gps, fc, ac, d0, a0, rows, zero_start=True)
    d2, a2 = D.scatter(rb, pt, gr, gps, fc, ac, np.zeros_like(d0), np.zeros_like(a0), rows)
    assert np.array_equal(d, d2) and np.array_equal(a, a2)
    assert D.scatter(rb, pt, gr, gps, fc, ac, None, a0, rows)[0] is None and D.scatter(rb, pt, gr, gps, fc, 0, d0, None, rows)[1] is None


def test_reduce_forms_are_the_scalar_loops():
    rng = np.random.default_rng(8)
    for slots in (1, 3, 256, 257, 300, 700):
        p = (rng.integers(-500, 500, (slots, 5)) * 2.0 ** (13 * rng.integers(0, 6, (slots, 1)))).astype(f32)
        lin, tree = D.reduce_linear(p), D.reduce_tree(p)
        for c in range(5):
            s = 0.0
            for i in range(slots):
                s = s + float(p[i, c])
            assert s == lin[c]
            red = [0.0] * 256
            for t in range(256):
                for i in range(t, slots, 256):
                    red[t] = red[t] + float(p[i, c])
            w = 128
            while w:
                for t in range(w):
                    red[t] = red[t] + red[t + w]
                w //= 2
            assert red[0] == tree[c]
        assert np.array_equal(D.reduce_linear(p, "desc"), D.reduce_linear(p[::-1]))
        # reversing the slots alone gives the tree's own bits (see reduce_tree): the control has to turn the tree round as well
        assert np.array_equal(D.reduce_tree(p[::-1]), tree)
    p = np.ones((300, 4097), f32)
    assert D.ordered_reduce(p[:, :4096], 4096)[0] == 300 and D.ordered_reduce(p, 4097)[0] == 300


def test_form_selection_follows_the_shape():
    rng = np.random.default_rng(9)
    p = (rng.integers(-500, 500, (300, 64)) * 2.0 ** (13 * rng.integers(0, 6, (300, 1)))).astype(f32)
    assert np.array_equal(D.ordered_reduce(p, 4096), D.reduce_tree(p)) and np.array_equal(D.ordered_reduce(p, 4097), D.reduce_linear(p))
    assert np.array_equal(D.ordered_reduce(p[:256], 64), D.reduce_linear(p[:256]))
    assert not np.array_equal(D.reduce_tree(p), D.reduce_linear(p))


def test_chunk_rule():
    assert [D.dw_chunk(*a) for a in ((192, 3), (193, 3), (1280, 40), (640, 40), (700, 1), (1, 3), (9600, 300))] == [64, 96, 32, 32, 704, 32, 32]


def test_run_heads_on_hand_made_maps():
    pt = np.array([0, 1, 1, 2, 5, 4, 6], np.int32)
    gr = np.array([0, 0, 1, 1, 2, 3, 5], np.int32)
    # group 1 shares point 1 with group 0; groups 2 and 3 interleave (5, 4); group 4 is empty; group 5 stands alone
    assert D.run_heads(pt, gr).tolist() == [True, False, True, False, True, True]
    assert D.run_heads(pt, gr, live=4).tolist() == [True, False]
    assert D.run_heads(np.array([3, 3], np.int32), np.array([0, 1], np.int32)).tolist() == [True, False]
    assert D.run_heads(np.array([3, 3], np.int32), np.array([0, 1], np.int32), strict=False).tolist() == [True, True]
    assert D.run_heads(pt, gr, live=0).size == 0


# ----------------------------------------------------------------------------- the input sets of the GPU gates
@pytest.mark.parametrize("name", D.SCATTER)
def test_scatter_operands_are_exact(scatter_sets, name):
    c = scatter_sets[name]
    G, W = c["G"].astype(f64), c["W"].astype(f64)
    assert c["n_out"] <= 72 and np.abs(W).max() <= 3 and (W[:, c["kv"]:] == 0).all() and W.shape == (c["n_out"], c["Kp"])
    prod = G @ W[:, :c["kv"]]
    assert np.array_equal(prod.astype(f32).astype(f64), prod)
    assert np.array_equal(D.rowbuf(c["G"], c["W"], c["kv"]).astype(f64), prod)
    mant = np.abs(G) / 2.0 ** np.floor(np.log2(np.maximum(np.abs(G), 1e-300)))
    assert np.isin(mant[G != 0], (1.0, 1.5)).all()                                  # 1, 2, 3 times a power of two
    assert (np.abs(prod).sum() > 0) and c["rows"] <= 2500
    for k in ("dfeat0", "daction0"):
        assert c[k] is None or (c[k] != 0).all()
    assert (np.diff(c["row_grp"]) >= 0).all()


def test_maps_have_the_properties_they_are_there_for(scatter_sets):
    S = scatter_sets
    heads = lambda n, **kw: D.run_heads(S[n]["row_pt"], S[n]["row_grp"], S[n]["live"], **kw)
    h = heads("samples")
    assert h[0] and h[8] and h[16] and h.size == 24                                # a cut in front of every sample
    c = S["touching"]
    assert heads("touching").sum() == 1 and heads("touching", strict=False)[[8, 16]].all()       # `<=` would cut at both boundaries
    for b in (1, 2):                                                               # >= 64 rows on the shared point on each side
        shared = b * 63
        on = c["row_pt"] == shared
        assert (on & (c["row_grp"] // 8 == b - 1)).sum() >= 64 and (on & (c["row_grp"] // 8 == b)).sum() >= 64
    assert heads("descending").sum() == 1
    for n, G in (("groups600", 600), ("groups513", 513), ("groups600_border", 600)):
        h = heads(n)
        assert h.size == G and (G + 255) // 256 == 3
        cuts = np.flatnonzero(h)
        assert (cuts % 3 == 0).any() and (cuts % 3 == 1).any() and (cuts % 3 == 2).any()       # on chunk borders and inside chunks
        assert (~h[np.arange(0, G, 3)]).any()                                                   # and chunk borders without a cut
    h = heads("groups600_border")
    assert h[299] and not h[300] and h[301]
    assert heads("runs1100").sum() == 1100 > 1024 and S["runs1100"]["gps"] == 1 and S["runs1100"]["rows"] == 2200
    g = S["gaps"]["row_grp"]
    assert g[0] != 0 and np.setdiff1d(np.arange(g[0], g[-1]), g).size > 0          # holes, and a first group that is not 0
    s = S["sparse"]
    assert s["row_grp"][-1] + 1 > s["rows"] and (s["row_grp"] % 3 == 0).all()      # more group ids than the bounds arrays hold
    c = S["live_in_group"]
    assert c["row_grp"][c["live"] - 1] == c["row_grp"][c["live"]] and c["live"] % 64 not in (0, 63) and c["live"] < c["rows"]
    assert S["live0"]["live"] == 0
    c = S["live_short_sample"]
    assert c["row_grp"][c["live"] - 1] == 2 * 8 + 2 and c["row_grp"][c["live"]] == 2 * 8 + 3
    c = S["cols260"]
    assert (c["feat_c"], c["Kp"], c["n_out"], c["kv"]) == (260, 272, 8, 269)
    assert S["dfeat_only"]["act_c"] == 0 and S["dfeat_only"]["daction0"] is None and S["daction_only"]["dfeat0"] is None
    assert S["one_row"]["rows"] == 1


@pytest.mark.parametrize("name", D.SCATTER)
def test_scatter_inputs_are_sensitive_to_the_order(scatter_sets, name):
    """the descending-order reference differs from the ascending one in >= 2 % of the written elements of every output in which
    an order exists (scatter_sensitivity: three terms or more on some destination)"""
    c = scatter_sets[name]
    sens = D.scatter_sensitivity(c)
    asked = 0
    for k, (diff, n, ordered) in sens.items():
        if c[k + "0"] is None or not ordered:
            continue
        asked += 1
        assert n > 0 and diff >= D.FLOOR * n, "%s %s: the opposite order changes %d of %d written elements" % (name, k, diff, n)
    assert asked > 0 or name in D.UNORDERED
    if name == "runs1100":                               # two rows per sample: their float64 sum commutes, no order to ask for
        assert not sens["daction"][2] and sens["dfeat"][2]


@pytest.mark.parametrize("name", sorted(D.DW))
def test_dw_inputs_are_exact_and_sensitive(dw_sets, name):
    c = dw_sets[name]
    assert max(c["n_out"]) <= 72 and all(np.abs(x).max() <= 3 and np.array_equal(x, np.round(x)) for x in c["X"])
    splits = max(c["splits"], 1)
    chunk = D.dw_chunk(c["live"], splits)
    for g in range(len(c["n_out"])):
        parts = D.dw_partials(c, g)                      # (asserts every split's product exact in any order)
        d = c["dZ"][:c["live"], c["dz_off"][g]:c["dz_off"][g] + c["n_out"][g]].astype(f64)
        assert np.array_equal(parts.astype(f64).sum(0), d.T @ c["X"][g][:c["live"]].astype(f64)) or not c["flat"]
        live_splits = -(-c["live"] // chunk)
        assert (parts[live_splits:] == 0).all()
    if c["live_splits"]:
        assert -(-c["live"] // chunk) == c["live_splits"] < splits
    elif not c["flat"]:
        assert c["live"] == splits * chunk
    assert (c["gacc0"] != 0).all()
    ref, desc = D.dw_reference(c), D.dw_reference(c, order="desc")
    m = D.dw_mask(c)
    assert np.array_equal(ref[~m], c["gacc0"][~m])
    diff, n = D.differs(ref, desc, m)
    if c["flat"]:                                        # row_splits 1 / 0: the exact integer sum, the same in any order
        assert diff == 0 and np.array_equal(ref, D.dw_reference(dict(c, flat=False, splits=7)))
    else:
        assert diff >= D.FLOOR * n, "%s: the opposite order changes %d of %d written elements" % (name, diff, n)
        assert not np.array_equal(ref, D.dw_reference(c, drop_split=splits // 2 if not c["live_splits"] else 3))
        assert not np.array_equal(ref[m], D.dw_reference(c, zero_start=True)[m])


def test_dw_forms_of_the_cases(dw_sets):
    tree = [n for n, c in dw_sets.items() if max(c["splits"], 1) > 256 and max(c["n_out"]) * c["Kp"] <= 4096]
    assert tree == ["splits300.tree"] and dw_sets["splits300.linear"]["n_out"][0] * dw_sets["splits300.linear"]["Kp"] > 4096
    c = dw_sets["two_groups"]
    assert c["n_out"] == [36, 72] and c["w_off"] == [0, 36 * 40] and c["dz_off"] == [0, 36]


def test_stats_forward_is_exact():
    rng = np.random.default_rng(3)
    x, W, w = D.ints(rng, (130, 8)), D.ints(rng, (5, 8), -1, 1), 2.0 ** rng.integers(0, 3, 130)
    s, q, worst = D.stats_forward([x], [W], w.astype(f32), 100)
    z = x[:100].astype(f64) @ W.astype(f64).T
    assert np.array_equal(s, (w[:100, None] * z).sum(0)) and np.array_equal(q, (w[:100, None] * z * z).sum(0)) and worst < 2 ** 24
    assert D.stats_forward([x], [W], None, 0)[0].tolist() == [0.0] * 5
