"""CPU pins of tests/fps_reference.py, the numpy model behind tests/test_gpu_fps_forms.py: the model equals the C oracle
(oracle/cref.fps) on every kind of cloud the GPU module uses, and -- the negative controls -- every trap cloud separates the pinned
evaluation from each fused one at the designated pick, and every directed tie is won by the index the GPU module names.  A kernel
that equals the oracle on these clouds therefore cannot have contracted its distance or its skip norm, nor walked a lane's points
in the wrong order.  No GPU: nothing is launched."""
import numpy as np
import pytest

from tests import fps_reference as R

SIZES = (1, 2, 3, 33, 64, 65, 300, 513, 1025)


def _oracle(xyz, M):
    from oracle import cref
    return cref.fps(xyz, M)


@pytest.mark.parametrize("N", SIZES)
def test_model_equals_the_oracle(N):
    """random, lattice, duplicate, all-skipped, non-finite and far clouds at min(N, 64) picks and at M > N"""
    xyz = np.stack([R.cloud(kind, N) for kind in R.KINDS])
    for M in (min(N, 64), N + 3):
        want = _oracle(xyz, M)
        got = R.fps(xyz, M)
        assert got.dtype == np.int32 and got.shape == (len(R.KINDS), M)
        for i, kind in enumerate(R.KINDS):
            np.testing.assert_array_equal(got[i], want[i], err_msg="%s N=%d M=%d" % (kind, N, M))
    assert (want[R.KINDS.index("skipped")] == 0).all()
    assert (want[R.KINDS.index("nan_start")] == 0).all()             # no distance from a NaN start ever updates temp: key 0 wins


def test_model_equals_the_oracle_on_all_picks():
    """M = N: the last rounds run on an exhausted cloud (every distance 0: the tie rule alone picks)"""
    for N in (65, 513):
        xyz = np.stack([R.cloud(kind, N) for kind in ("random", "lattice", "far6")])
        np.testing.assert_array_equal(R.fps(xyz, N), _oracle(xyz, N))


def test_a_nan_distance_never_updates_and_never_wins():
    """upstream's semantics for non-finite coordinates, spelled out on six points: temp of the NaN point stays 1e10f, so it is the
    second pick; from it every distance is NaN, nothing is updated, and it stays the maximum"""
    xyz = np.array([[[0.5, 0.5, 0.5], [0.6, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.9, 0.5, 0.5], [0.5, 0.7, 0.5], [0.5, 0.5, 0.1]]], R.f32)
    want = _oracle(xyz, 4)
    np.testing.assert_array_equal(want, [[0, 2, 2, 2]])
    np.testing.assert_array_equal(R.fps(xyz, 4), want)
    xyz[0, 2, 0] = np.inf                                             # d = inf is not < 1e10f either; inf - inf = NaN from then on
    np.testing.assert_array_equal(_oracle(xyz, 4), [[0, 2, 2, 2]])
    np.testing.assert_array_equal(R.fps(xyz, 4), [[0, 2, 2, 2]])


def test_far_clouds_tie_at_the_initial_distance():
    """coordinates of 1e6 and 1e20: nearly every d^2 is above 1e10f (or inf), temp keeps its initial value and the first rounds are
    decided by the tie rule alone -- the picks walk the bit-reversed thread order"""
    for kind in ("far6", "far20"):
        want = _oracle(R.cloud(kind, 64)[None], 8)[0]
        np.testing.assert_array_equal(want, [0, 32, 16, 48, 8, 40, 24, 56])


@pytest.mark.parametrize("variant", R.FUSED)
def test_fused_sums_differ_from_the_pinned_one(variant):
    rng = np.random.default_rng(5)
    pts = rng.random((4096, 3)).astype(R.f32)
    a, b = R.sqnorm()(pts), R.sqnorm(variant)(pts)
    assert a.dtype == b.dtype == R.f32
    ulp = np.abs(a.view(np.int32) - b.view(np.int32))
    assert ulp.max() >= 1 and (ulp > 0).mean() > 0.05
    assert (R.sqdist(variant)(pts, pts[0]) != R.sqdist()(pts, pts[0])).any()


# (N, placement, T): the shapes tests/test_gpu_fps_forms.py runs the traps at
TRAP_PLACES = [(64, "wave", 64), (1024, "lane", 256), (1024, "wave", 256), (4096, "block", 256), (1024, "lane", 64), (1000, "lane", 400)]


@pytest.mark.parametrize("variant", R.FUSED)
def test_distance_trap_separates_pinned_from_fused(variant):
    """negative control: on the trap cloud the pinned model equals the oracle, and the model that evaluates the distance as
    `variant` picks the other candidate second"""
    for N, lanes, T in TRAP_PLACES:
        xyz = R.distance_trap(variant, N, lanes, T)[None]
        want = _oracle(xyz, 4)
        np.testing.assert_array_equal(R.fps(xyz, 4), want)
        alt = R.fps(xyz, 4, sqdist=R.sqdist(variant))
        assert alt[0, 1] != want[0, 1], (variant, N, lanes)
        a, b = int(want[0, 1]), int(alt[0, 1])
        assert {a, b} == {5, {"lane": 5 + T, "wave": 37, "block": 101}[lanes]}
        d = R.sqdist()(xyz[0, [a, b]], xyz[0, 0])
        assert 0 < d[0].view(np.int32) - d[1].view(np.int32) <= 4      # a few ulp apart, A strictly ahead: no tie rule involved


def test_distance_trap_raises_where_the_placement_does_not_fit():
    with pytest.raises(ValueError):
        R.distance_trap("yx", 64, "lane", 256)


@pytest.mark.parametrize("variant", R.FUSED)
@pytest.mark.parametrize("N", (64, 1024))
def test_skip_trap_separates_pinned_from_fused(variant, N):
    """negative control: the kept point is the oracle's second pick and vanishes from the picks of the model with the fused norm;
    the skipped point is in no oracle pick and is the fused model's second pick"""
    kept, skipped = R.skip_trap(variant, N)
    assert kept.kept and not skipped.kept and kept.index == skipped.index == N - 3
    for trap in (kept, skipped):
        xyz = trap.xyz[None]
        want = _oracle(xyz, 6)
        np.testing.assert_array_equal(R.fps(xyz, 6), want)
        alt = R.fps(xyz, 6, sqnorm=R.sqnorm(variant))
        if trap.kept:
            assert want[0, 1] == trap.index and trap.index not in alt[0]
        else:
            assert trap.index not in want[0] and alt[0, 1] == trap.index


@pytest.mark.parametrize("cfg,form,T,N,k1,k2,winner", R.TIES)
def test_directed_ties_pick_the_index_with_the_smaller_bit_reversed_thread(cfg, form, T, N, k1, k2, winner):
    """the table tests/test_gpu_fps_forms.py runs: the oracle's second pick is the designated index -- the HIGHER one where
    winner == 2 -- and, but for the two cross-wavefront cases, one lane of the form owns both"""
    assert k1 < k2 and ((k1 % T == k2 % T) or (cfg == 0 and k1 % T // 64 != k2 % T // 64))
    xyz = R.tie_cloud(N, k1, k2)[None]
    want = _oracle(xyz, 3)
    np.testing.assert_array_equal(R.fps(xyz, 3), want)
    assert want[0, 1] == (k1, k2)[winner - 1]
    assert (R.tie_key(k2, N) < R.tie_key(k1, N)) == (winner == 2)     # the rule in closed form agrees with the reduction
    assert want[0, 2] not in (k1, k2)                                 # the loser's distance is 0 from then on


def test_the_tie_table_reaches_every_in_lane_order():
    """R = tie_bs / T in {2, 4, 8}, each with a case the higher index wins and (beyond the 200- and 300-point shapes, too small for
    one) its mirror"""
    seen = {(R.tie_bs(N) // T, winner) for _, _, T, N, k1, k2, winner in R.TIES if k1 % T == k2 % T}
    assert seen == {(r, w) for r in (2, 4, 8) for w in (1, 2)}
