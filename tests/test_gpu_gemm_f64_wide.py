"""float64 gates of the layer GEMMs' wide-tile routes (D: gemm_fwd / gemm_dx / gemm_dw (wide) and (wide split), the fused
gemm_bwd(wide)) and SA1 streaming routes of layers 2 / 3 (E: gemm_fwd / gemm_dx / gemm_bwd (stream) and (stream split), mode 2), of
the grid-rows hint (gad_grid_rows_hint) and of the persistent-workgroup loops.  The gate, the case classes and the references are
those of tests/test_gpu_gemm_f64.py (tables A - C): tests/gemm_cases.py, tests/gemm_reference.py; one launch per case through the C
entry point, every case asserts the route it took (gad_last_kernel).  The per-element bound (T + 2) * 2^-24 * sum |terms| is the
same in both arithmetic modes: the split-bf16 form claims 24 significand bits and is held to them here.

Row counts: D -- a static bound of 2304 rows with a device live count of 2049 (one live row in the 33rd 64-row tile) or 2048 + 63;
E -- 32768 + 1000 static, 32768 + 37 live (the smallest the streaming predicates take, live rows ending inside a slab).

GAD_GEMM_F64_REPORT=<file>: the measured worst err / bound and the mean-error ratio against torch's float32 evaluation of every case
and output are written there -- appended when tests/test_gpu_gemm_f64.py wrote its tables to the file in the same session
(profiles/gemm_f64_wide_gates.txt is that file from an MI355X run of this module alone)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

_REPORT = []


class _Cases(object):
    """tests.gemm_cases, imported when a case is built (collection must not need the library)"""

    def __getattr__(self, k):
        from tests import gemm_cases
        return getattr(gemm_cases, k)


gc = _Cases()


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    path = os.environ.get("GAD_GEMM_F64_REPORT")
    if path and _REPORT:
        base = sys.modules.get("tests.test_gpu_gemm_f64")
        with open(path, "a" if base is not None and base._REPORT else "w") as f:
            f.write("# float64 gates of the wide-tile and SA1 streaming GEMM routes (tests/test_gpu_gemm_f64_wide.py)\n"
                    "# command: GAD_GEMM_F64_REPORT=<this file> python -m pytest tests/test_gpu_gemm_f64_wide.py\n"
                    "# case [options] -> route | output, T, worst err / ((T + 2) * 2^-24 * abs_bound), mean |err|, the same for torch's float32\n"
                    "# evaluation of the identical operands, their ratio (gate: 1.5 x + floor), the floor.  ABOVE 1.5 x: a case listed and\n"
                    "# explained in ORDER_COST of the test, held to 1.5 x torch's float32 evaluation in one chain instead\n")
            f.write("\n".join(_REPORT) + "\n")


ROWS, LIVES = 2304, (2049, 2048 + 63)
SROWS, SLIVE = 32768 + 1000, 32768 + 37
F32, SPLIT = {"mfma_split": 0}, {"mfma_split": 1}
G32, G128 = dict(feat_c=32), dict(feat_c=128)
POOL4 = dict(gsz=4)


def _modes(t, name, factory, kind, family, options=None):
    """the case in both arithmetic modes: FP32 MFMA (option mfma_split 0) and split-bf16 (mfma_split on; factory(split=True) hands the
    call the weight mirror its route needs)"""
    options = options or {}
    t[name + ".f32"] = (lambda: factory(False), dict(options, **F32), "gemm_%s(%s)" % (kind, family))
    t[name + ".split"] = (lambda: factory(True), dict(options, **SPLIT), "gemm_%s(%s split)" % (kind, family))


def _dw(rows, Kp, N, live, gather=None, k_valid=None, **dz_kw):
    """gad_gemm_dw of an ACT (BatchNorm + ReLU in front) or gathered layer over a Dx gradient source"""
    if gather is not None:
        inp = gc.Fwd(rows, Kp, [N], gather=gather, live=live, stats=False, zout=False)
    else:
        inp = gc.Fwd(rows, Kp, [N], c_in=Kp, live=live, stats=False, zout=False)
    return gc.Dw(inp, gc.Dx(rows, [N], Kp, k_valid if k_valid is not None else Kp, live=live, **dz_kw))


def _table_d():
    """name -> (factory, options, route)"""
    t = {}
    for L in LIVES:
        s = ".live%d" % L
        # ---- forward, ACT input: one K-tile, an odd number of K-tiles, two column blocks, the largest K
        for Kp, N in ((32, 128), (96, 128), (128, 256), (512, 128)):
            _modes(t, "fwd.k%d.n%d%s" % (Kp, N, s), lambda sp, Kp=Kp, N=N, L=L: gc.Fwd(ROWS, Kp, [N], c_in=Kp, live=L, split=sp), "fwd", "wide")
        _modes(t, "fwd.nozout" + s, lambda sp, L=L: gc.Fwd(ROWS, 96, [128], c_in=96, live=L, zout=False, split=sp), "fwd", "wide")
        _modes(t, "fwd.nostats" + s, lambda sp, L=L: gc.Fwd(ROWS, 96, [128], c_in=96, live=L, stats=False, split=sp), "fwd", "wide")
        f = lambda sp, L=L: gc.Fwd(ROWS, 128, [256], c_in=128, live=L, in_stat=True, split=sp)
        _modes(t, "fwd.in_stat" + s, f, "fwd", "wide")
        _modes(t, "fwd.in_stat.finalize_launch" + s, f, "fwd", "wide", {"fwd_bn_prologue": 0})
        # ---- forward, fused max-pool (the live rows end inside a group of 4)
        _modes(t, "fwd.pool.k64.n128" + s, lambda sp, L=L: gc.Fwd(ROWS, 64, [128], c_in=64, live=L, pool=POOL4, split=sp), "fwd", "wide")
        _modes(t, "fwd.pool.k256.n512.gamma" + s,
               lambda sp, L=L: gc.Fwd(ROWS, 256, [512], c_in=256, live=L, pool=dict(gsz=4, gamma="mixed"), split=sp), "fwd", "wide")
        # ---- forward, gathered input
        _modes(t, "fwd.gather.kp40" + s, lambda sp, L=L: gc.Fwd(ROWS, 40, [128], gather=G32, live=L, split=sp), "fwd", "wide")
        _modes(t, "fwd.gather.kp136" + s, lambda sp, L=L: gc.Fwd(ROWS, 136, [128], gather=G128, live=L, split=sp), "fwd", "wide")
        # ---- dX (the route requires the previous layer's BatchNorm block and store_masked)
        for N, kv in ((32, 128), (96, 128), (160, 256), (512, 128)):
            _modes(t, "dx.n%d.k%d%s" % (N, kv, s), lambda sp, N=N, kv=kv, L=L: gc.Dx(ROWS, [N], kv, kv, prev=True, live=L, split=sp), "dx", "wide")
        _modes(t, "dx.pooled" + s, lambda sp, L=L: gc.Dx(ROWS, [96], 128, 128, prev=True, live=L, pooled=POOL4, split=sp), "dx", "wide")
        _modes(t, "dx.scatter" + s, lambda sp, L=L: gc.Dx(ROWS, [128], 136, 128, live=L, scatter=G128, split=sp), "dx", "wide")
        _modes(t, "dx.bn" + s, lambda sp, L=L: gc.Dx(ROWS, [96], 128, 128, prev=True, live=L, bn=True, split=sp), "dx", "wide")
        # ---- dW (the split kernel forms its own splits: no mirror)
        for Kp in (128, 256):
            _modes(t, "dw.k%d.n128%s" % (Kp, s), lambda sp, Kp=Kp, L=L: _dw(ROWS, Kp, 128, L), "dw", "wide")
        _modes(t, "dw.gather.kp136" + s, lambda sp, L=L: _dw(ROWS, 136, 128, L, gather=G128, k_valid=131), "dw", "wide")
        _modes(t, "dw.pooled" + s, lambda sp, L=L: _dw(ROWS, 128, 128, L, pooled=POOL4), "dw", "wide")
        _modes(t, "dw.bn" + s, lambda sp, L=L: _dw(ROWS, 128, 128, L, bn=True), "dw", "wide")
        for wgs in (4, 1):                   # few splits, each looping over many row chunks
            _modes(t, "dw.k256.wgs%d%s" % (wgs, s), lambda sp, L=L: _dw(ROWS, 256, 128, L), "dw", "wide", {"dw_wide_wgs": wgs})
        # ---- fused backward (option bwd_wide 1; FP32 MFMA only): the three NIT instantiations, the gradient sources, the L1 scatter
        BW = {"bwd_wide": 1}
        for N, kv in ((128, 64), (256, 128), (512, 128)):
            t["bwd.n%d.k%d%s" % (N, kv, s)] = (lambda N=N, kv=kv, L=L: gc.Bwd(gc.Dx(ROWS, [N], kv, kv, prev=True, live=L)), BW, "gemm_bwd(wide)")
        t["bwd.pooled" + s] = (lambda L=L: gc.Bwd(gc.Dx(ROWS, [128], 64, 64, prev=True, live=L, pooled=POOL4)), BW, "gemm_bwd(wide)")
        t["bwd.scatter" + s] = (lambda L=L: gc.Bwd(gc.Dx(ROWS, [128], 136, 128, live=L, scatter=G128)), BW, "gemm_bwd(wide)")
        # (bwd_wide_slab 1 with 512 x 128 weights: 16 partial blocks, the fewest bwd_wide_splits gives, over 36 row tiles)
        t["bwd.n512.slab1" + s] = (lambda L=L: gc.Bwd(gc.Dx(ROWS, [512], 128, 128, prev=True, live=L)), dict(BW, bwd_wide_slab=1), "gemm_bwd(wide)")
        t["bwd.n128.reduce_later" + s] = (lambda L=L: gc.Bwd(gc.Dx(ROWS, [128], 64, 64, prev=True, live=L), later=True), BW, "gemm_bwd(wide)")
    # ---- live count 0: nothing is written, the statistics stay zero
    _modes(t, "fwd.live0", lambda sp: gc.Fwd(ROWS, 96, [128], c_in=96, live=0, split=sp), "fwd", "wide")
    _modes(t, "dx.live0", lambda sp: gc.Dx(ROWS, [96], 128, 128, prev=True, live=0, split=sp), "dx", "wide")
    _modes(t, "dw.live0", lambda sp: _dw(ROWS, 128, 128, 0), "dw", "wide")
    t["bwd.live0"] = (lambda: gc.Bwd(gc.Dx(ROWS, [128], 64, 64, prev=True, live=0)), {"bwd_wide": 1}, "gemm_bwd(wide)")
    # ---- just outside the predicates: the generic tile kernels
    L = LIVES[0]
    t["outside.fwd.rows2047"] = (lambda: gc.Fwd(2047, 96, [128], c_in=96, live=2000), {}, "gemm_fwd")
    t["outside.dx.rows2047"] = (lambda: gc.Dx(2047, [96], 128, 128, prev=True, live=2000), {}, "gemm_dx")
    t["outside.dw.rows2047"] = (lambda: _dw(2047, 128, 128, 2000), {}, "gemm_dw")
    t["outside.fwd.kp544"] = (lambda: gc.Fwd(ROWS, 544, [128], c_in=544, live=L), {}, "gemm_fwd")
    t["outside.fwd.n192"] = (lambda: gc.Fwd(ROWS, 96, [192], c_in=96, live=L), {}, "gemm_fwd")
    t["outside.dx.k192"] = (lambda: gc.Dx(ROWS, [96], 192, 192, prev=True, live=L), {}, "gemm_dx")
    t["outside.dw.kp96"] = (lambda: _dw(ROWS, 96, 128, L), {}, "gemm_dw")
    return t


def _sdx(N, pooled, split=False, live=SLIVE):
    """the dX description the SA1 streaming routes take: 64 input channels, pitches = channel counts, the layer's own scale / shift"""
    return gc.Dx(SROWS, [N], 64, 64, dscale=True, prev=True, pad_cols=0, pooled=pooled, live=live, split=split)


def _table_e():
    t = {}
    g8, g16 = dict(feat_c=4), dict(feat_c=4, act_c=6, gps=4)
    # ---- forward (the kernel splits W itself: no mirror); persistent loop: 3 workgroups x ~44 eight-slab units, and 1 workgroup
    _modes(t, "fwd.stream.n64", lambda sp: gc.Fwd(SROWS, 64, [64], c_in=64, live=SLIVE), "fwd", "stream")
    _modes(t, "fwd.stream.n64.wgs1", lambda sp: gc.Fwd(SROWS, 64, [64], c_in=64, live=SLIVE), "fwd", "stream", {"fwd_stream_wgs": 1})
    f = lambda sp: gc.Fwd(SROWS, 64, [128], c_in=64, live=SLIVE, in_stat=True)
    _modes(t, "fwd.stream.n128.in_stat", f, "fwd", "stream")
    _modes(t, "fwd.stream.n128.in_stat.wgs3", f, "fwd", "stream", {"fwd_stream_wgs": 3})
    f = lambda sp: gc.Fwd(SROWS, 64, [128], c_in=64, live=SLIVE, pool=POOL4)
    _modes(t, "fwd.stream.pool", f, "fwd", "stream")
    _modes(t, "fwd.stream.pool.wgs3", f, "fwd", "stream", {"fwd_stream_wgs": 3})
    _modes(t, "fwd.stream.pool.nozout", lambda sp: gc.Fwd(SROWS, 64, [128], c_in=64, live=SLIVE, pool=POOL4, zout=False), "fwd", "stream")
    # mode 2 (layer 1 recomputed from the gathered rows) exists in FP32 MFMA only: the same route whatever mfma_split says
    for name, gth, pk in (("kp8", g8, 8), ("kp16", g16, 16)):
        f = lambda gth=gth, pk=pk: gc.Fwd(SROWS, 64, [64], c_in=64, gather=gth, pre_Kp=pk, live=SLIVE)
        t["fwd.stream.mode2.%s.f32" % name] = (f, F32, "gemm_fwd(stream)")
        t["fwd.stream.mode2.%s.split_on" % name] = (f, SPLIT, "gemm_fwd(stream)")
    t["fwd.stream.mode2.kp8.wgs3"] = (lambda: gc.Fwd(SROWS, 64, [64], c_in=64, gather=g8, pre_Kp=8, live=SLIVE), dict(F32, fwd_stream_wgs=3),
                                      "gemm_fwd(stream)")
    # ---- dX and the fused backward; bwd_fused 0: the separate kernels (the last launch is the dX one)
    for N in (64, 128):
        for src, pooled in (("dense", None), ("pooled", POOL4)):
            tag = ".n%d.%s" % (N, src)
            _modes(t, "dx.stream" + tag, lambda sp, N=N, pooled=pooled: _sdx(N, pooled, sp), "dx", "stream")
            f = lambda sp, N=N, pooled=pooled: gc.Bwd(_sdx(N, pooled, sp))
            _modes(t, "bwd.stream" + tag, f, "bwd", "stream")
            _modes(t, "bwd.stream" + tag + ".wgs3", f, "bwd", "stream", {"bwd_stream_wgs": 3})
            _modes(t, "bwd.unfused" + tag, f, "dx", "stream", {"bwd_fused": 0})
    # A pooled source with 64 outputs keeps the FP32-MFMA fused kernel whatever mfma_split says (gad_gemm_bwd): on the split fused
    # kernel these two cases measured dW 6.2 x / 5.9 x torch's float32 mean error -- channels 0 .. 31 only, dX exact -- and the route
    # was closed for the shape.  The cases stay and assert the route they must now take.
    for name in ("bwd.stream.n64.pooled.split", "bwd.stream.n64.pooled.wgs3.split"):
        t[name] = (t[name][0], t[name][1], "gemm_bwd(stream)")
    t["bwd.stream.n128.dense.reduce_later"] =(lambda: gc.Bwd(_sdx(128, None), later=True), dict(F32, bwd_stream_wgs=3), "gemm_bwd(stream)")
    # ---- just outside the predicate: 32767 rows take the wide-tile kernel, not a tile kernel
    _modes(t, "outside.fwd.rows32767", lambda sp: gc.Fwd(32767, 64, [128], c_in=64, split=sp), "fwd", "wide")
    return t


D, E = sorted(_table_d()), sorted(_table_e())
# Cases whose mean error lands above 1.5 x torch's float32 evaluation BECAUSE of the order of summation (and pass the one-chain rule
# of gemm_cases.check), with the ratio measured on an MI355X beside each (profiles/gemm_f64_wide_gates.txt)
ORDER_COST = {
}


def _nan_equal(a, b):
    return torch.equal(torch.nan_to_num(a.double(), nan=-7.25), torch.nan_to_num(b.double(), nan=-7.25))


def _verdict(case, out, label, report=None, alter=None, chain_keys=()):
    """-> failures of the gate (and, for the unaltered reference, of the exact checks and the BatchNorm blocks)"""
    got = case.outputs(out) if hasattr(case, "outputs") else out
    bad = gc.check(label, got, case.expect(alter) if alter is not None else case.expect(), report, chain_keys=chain_keys)
    if alter is None:
        bad += case.exact(out)
        if getattr(case, "in_stat", False):
            bad += case.check_in_stat(out)
        dz = case if hasattr(case, "check_bn") else getattr(case, "dz", None)
        if dz is not None and dz.bn:
            bad += dz.check_bn(out)
    return bad


def _gate(table, name, tag=""):
    factory, options, route = table[name]
    case = factory()
    out, routed = case.run(options)
    assert routed == route, "%s: routed to %s, expected %s" % (name, routed, route)
    label = "%s%s %s -> %s" % (name, tag, " ".join("%s=%d" % kv for kv in sorted(options.items())), routed)
    bad = _verdict(case, out, label, _REPORT, chain_keys=ORDER_COST.get(name, ()))
    assert not bad, "\n".join(bad)
    return case, out


@pytest.mark.parametrize("name", D)
def test_wide_tile_routes(name):
    """D: gemm_fwd / gemm_dx / gemm_dw (wide) and (wide split) and the fused gemm_bwd(wide) at 2304 static rows with 2049 and 2111 live:
    one, an odd number and the most K-tiles, one to four column blocks, NULL zout, no statistics, the input layer's BatchNorm in the
    prologue and by a launch of its own, the fused max-pool (mixed gamma signs), gathered inputs, dense / pooled gradient sources, the
    scatter epilogue, the bn_* block, few dW splits, every NIT of the fused backward, its deferred reduce; a live count of 0; shapes
    just outside each predicate, which must take the tile kernels"""
    _gate(_table_d(), name)


@pytest.mark.parametrize("name", E)
def test_sa1_streaming_routes(name):
    """E: gemm_fwd (stream) / (stream split) of SA1 layers 2 and 3 (64 -> 64, 64 -> 128, pooled, NULL zout, the input BatchNorm in the
    prologue, mode 2), gemm_dx and the fused gemm_bwd (stream) / (stream split) with dense and pooled sources, the separate kernels
    under bwd_fused 0, and the persistent-workgroup loops: 3 (and 1) workgroups walking ~44 (132) eight-slab units each, the live rows
    ending inside the last one; the fused backward's split count follows bwd_stream_wgs and its reduce must add every partial"""
    _gate(_table_e(), name)


def test_mode2_is_bit_equal_to_the_stored_first_layer():
    """mode 2 recomputes layer 1 with the same products in the same order as that layer's own launch: its z must be bit-equal to the
    launch that reads the z1 the gathered first layer stored (same operands, same FP32-MFMA route)"""
    for gth, pk in ((dict(feat_c=4), 8), (dict(feat_c=4, act_c=6, gps=4), 16)):
        m = gc.Fwd(SROWS, 64, [64], c_in=64, gather=gth, pre_Kp=pk, live=SLIVE)
        out2, routed = m.run(F32)
        assert routed == "gemm_fwd(stream)"
        first = gc.Fwd(SROWS, pk, [64], gather=gth, live=SLIVE, stats=False)
        for k in ("feat", "src", "ctr", "action", "row_pt", "row_grp", "row_w"):
            setattr(first, k, getattr(m, k))
        first.W = m.pre_W.reshape(-1).contiguous()
        z1, routed = first.run(F32)
        assert routed == "gemm_fwd(stream)"
        second = gc.Fwd(SROWS, 64, [64], c_in=64, live=SLIVE)
        second.zin = torch.nan_to_num(z1["z"], nan=0.0)                  # (rows past the live count: never read into a result)
        second.scale, second.shift, second.W, second.row_w = m.scale, m.shift, m.W, m.row_w
        out1, routed = second.run(F32)
        assert routed == "gemm_fwd(stream)"
        assert _nan_equal(out1["z"], out2["z"]), "pre_Kp %d: mode 2 differs from the stored-z1 launch" % pk


def test_deferred_reduce_is_bit_equal_to_the_one_call_form():
    """GAD_DW_REDUCE_LATER + gad_gemm_dw_reduce against the call that reduces itself.  512 x 128 weights under bwd_wide_slab 1: 16
    partial blocks, which dw_reduce_kernel sums in ONE chunk (DW_RED_CHUNK 16) in split order -- one f64 atomic per arena word, so the
    arena does not depend on the order atomics land in (with more chunks it would, in the last f64 bit, in either form)"""
    opts = {"bwd_wide": 1, "bwd_wide_slab": 1}
    case = gc.Bwd(gc.Dx(ROWS, [512], 128, 128, prev=True, live=LIVES[1]))
    one, routed = case.run(opts)
    assert routed == "gemm_bwd(wide)"
    case.later = True
    two, routed = case.run(opts)
    assert routed == "gemm_bwd(wide)"
    assert not _verdict(case, two, "reduce later")
    assert torch.equal(one["gacc"], two["gacc"]), "dW of the deferred reduce differs from the one-call form"
    assert _nan_equal(one["gout"], two["gout"])


# ------------------------------------------------------------------------------------------------------ the grid-rows hint
HL = LIVES[0]
HINT_ROUTES = {
    "fwd.wide": (lambda: gc.Fwd(ROWS, 96, [128], c_in=96, live=HL), F32, "gemm_fwd(wide)"),
    "dx.wide": (lambda: gc.Dx(ROWS, [96], 128, 128, prev=True, live=HL), F32, "gemm_dx(wide)"),
    "fwd.tile": (lambda: gc.Fwd(ROWS, 96, [128], c_in=96, live=HL), {"fwd_wide": 0}, "gemm_fwd"),
    "dx.tile": (lambda: gc.Dx(ROWS, [96], 128, 128, prev=True, live=HL), {"dx_wide": 0}, "gemm_dx"),
}
HINTS = {"1": 1, "64": 64, "live-1": HL - 1, "live": HL, "above_static": ROWS + 1}


@pytest.mark.parametrize("hint", sorted(HINTS))
@pytest.mark.parametrize("route", sorted(HINT_ROUTES))
def test_grid_rows_hint_changes_no_result(route, hint):
    """gad_grid_rows_hint sizes the grid only: whatever the hint (1, 64, live - 1, live; one above the static row count is ignored),
    the launch passes the gate, its row outputs (z / gout: every element is reduced inside one workgroup, whichever that is) are
    bit-equal to the un-hinted launch, and its reduced outputs (statistics, dbeta, dgamma: per-workgroup float32 sums, regrouped by
    the grid) are inside the gate.  Negative control: the reference of a launch that stopped after `hint` rows must fail."""
    factory, options, want = HINT_ROUTES[route]
    h = HINTS[hint]
    case = factory()
    plain, routed = case.run(options)
    assert routed == want
    case.hint = h
    out, routed = case.run(options)
    assert routed == want
    label = "hint.%s.%s %s -> %s" % (route, hint, " ".join("%s=%d" % kv for kv in sorted(options.items())), routed)
    bad = _verdict(case, out, label, _REPORT)
    assert not bad, "\n".join(bad)
    row_key = "z" if "z" in out else "gout"
    assert _nan_equal(out[row_key], plain[row_key]), "%s differs from the un-hinted launch" % row_key
    if h < case.r:
        assert _verdict(case, out, "altered", alter=("first_rows", h)), "the gate accepted a reference that covers only the first %d rows" % h


def test_grid_rows_hint_without_device_row_count():
    """a hint given to a launch without n_rows_dev is ignored: bit-equal row output and statistics inside the gate"""
    case = gc.Fwd(ROWS, 96, [128], c_in=96)
    plain, routed = case.run(F32)
    assert routed == "gemm_fwd(wide)"
    case.hint = 64
    out, routed = case.run(F32)
    assert routed == "gemm_fwd(wide)"
    assert not _verdict(case, out, "hint without n_rows_dev")
    assert _nan_equal(out["z"], plain["z"])


# ------------------------------------------------------------------------------------------------------ negative controls
NL = LIVES[1]                                # 2111: the last tile's first row (2048) is not the last live row
CONTROLS = {
    "fwd.wide": (lambda: gc.Fwd(ROWS, 128, [256], c_in=128, live=NL), F32, "gemm_fwd(wide)"),
    "dx.wide": (lambda: gc.Dx(ROWS, [160], 256, 256, prev=True, live=NL), F32, "gemm_dx(wide)"),
    "dw.wide": (lambda: _dw(ROWS, 256, 128, NL), F32, "gemm_dw(wide)"),
    "bwd.wide": (lambda: gc.Bwd(gc.Dx(ROWS, [256], 256, 256, prev=True, live=NL)), {"bwd_wide": 1}, "gemm_bwd(wide)"),
    "fwd.stream": (lambda: gc.Fwd(SROWS, 64, [128], c_in=64, live=SLIVE), F32, "gemm_fwd(stream)"),
}
ALTERS = [(c, a) for c in sorted(CONTROLS) for a in ("drop_last_row_stats", "zero_tile_row", "shift_block")
          if not (c == "fwd.stream" and a == "shift_block")]          # (the streaming forward has no columns 128 .. 255)


@pytest.mark.parametrize("control,alter", ALTERS)
def test_gate_rejects_an_altered_reference(control, alter):
    """negative controls (no kernel is altered): the gate must fail a reference with the last live row dropped from the row sums
    (statistics, dbeta / dgamma; for dW the sum over rows IS the output), with the first row of the last 64-row tile zeroed, and with
    the output columns 128 .. 255 shifted by 4 -- and pass the unaltered one"""
    factory, options, want = CONTROLS[control]
    case = factory()
    out, routed = case.run(options)
    assert routed == want
    bad = _verdict(case, out, "control")
    assert not bad, "\n".join(bad)
    bad = _verdict(case, out, "altered", alter=alter)
    assert bad, "the gate accepted a reference with alteration '%s'" % alter
    if alter == "drop_last_row_stats" and control in ("fwd.wide", "dx.wide", "fwd.stream"):
        assert all(("stat" in b or "dbeta" in b or "dgamma" in b) for b in bad), bad


# ------------------------------------------------------------------------------------------------------ option hygiene
def test_options_are_back_at_their_defaults_after_a_case_that_raises():
    """Case.run restores every option it set in its `finally`: after a launch that is refused (Kp no multiple of 8), each of them
    reads its default again, and the next launch takes the default route"""
    from ga_ddpg_amd import hip
    options = {"bwd_wide": 1, "bwd_fused": 0, "bwd_wide_slab": 1, "dw_wide_wgs": 4, "fwd_stream_wgs": 3, "fwd_stream_l1_wgs": 3,
               "bwd_stream_wgs": 3, "fwd_bn_prologue": 0, "mfma_split": 0, "fwd_wide": 0}
    case = gc.Fwd(ROWS, 96, [128], c_in=96, live=HL, split=True)
    case.Kp = 100
    with pytest.raises(RuntimeError, match=r"multiple of 8"):
        case.run(options)
    for k in options:
        assert hip.get_option(k) == gc._default(k), "option %s was left at %d" % (k, hip.get_option(k))
    case.Kp = 96
    out, routed = case.run()
    assert routed == ("gemm_fwd(wide split)" if hip.get_option_default("mfma_split") else "gemm_fwd(wide)")
    assert not _verdict(case, out, "after a refused launch")
