"""tests/points_ref.py, the numpy statement of the closest-point query's
definition, against the oracle: the only value the oracle exports is the
signed distance (cpuref.sdf_points), and sqrt of the helper's least d2 must be
its absolute value in every bit. The point sets are the ones the GPU tests
use (test_points_device.py); they reach all seven Voronoi features and both
sides of the r = 0.05 radius.
"""
import numpy as np
import pytest

import cpuref
import points_ref as R


@pytest.fixture(scope="module", params=[("cube.obj", 3000), ("spot.obj", 1500)], ids=["cube", "spot"])
def case(request):
    name, n = request.param
    v, i = R.mesh(name)
    p = R.points(name, n, 11)
    return name, v, i, p, R.brute_force(v, i, p)


def test_distance_is_the_oracles_bit_for_bit(case):
    _, v, i, p, got = case
    ref = cpuref.sdf_points(v, i, p, 16)
    assert np.array_equal(R.bits(np.sqrt(got["d2"])), R.bits(np.abs(ref)))


def test_point_sets_reach_every_feature_and_both_sides_of_the_radius(case):
    _, v, i, p, got = case
    assert set(np.unique(got["feature"])) == set(range(7))
    n = len(p) // 3
    assert np.all(got["d2"][2 * n:] == 0)  # the on-vertex points
    near = np.mean(np.sqrt(got["d2"]) <= np.float32(0.05))
    assert 0.3 < near < 0.8
    assert got["prim"].min() >= 0 and got["prim"].max() < len(i) // 3


def test_closest_point_lies_on_the_winner(case):
    """q is on its triangle: inside the triangle's box, and p - q reproduces d2."""
    _, v, i, p, got = case
    a, b, c = R.corners(v, i)
    t = got["prim"]
    lo = np.minimum(np.minimum(a[t], b[t]), c[t]) - 1e-6
    hi = np.maximum(np.maximum(a[t], b[t]), c[t]) + 1e-6
    q = got["closest"]
    assert np.all((q >= lo) & (q <= hi))
    e = p - q
    assert np.array_equal(R.bits(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]), R.bits(got["d2"]))


def test_radius_rule(case):
    """r >= 0 && d2 <= r*r: the winner within a radius is the unbounded winner
    or nobody; a negative, NaN or too small radius leaves the miss values."""
    _, v, i, p, full = case
    n = len(p)
    r = np.empty(n, np.float32)
    r[0::5], r[1::5], r[2::5], r[3::5], r[4::5] = np.inf, 0.05, 0.0, -1.0, np.nan
    got = R.brute_force(v, i, p, r)
    with np.errstate(invalid="ignore"):
        hit = (r >= 0) & (full["d2"] <= r * r)
    assert hit[0::5].all() and not hit[3::5].any() and not hit[4::5].any()
    assert hit[1::5].any() and not hit[1::5].all() and hit[2::5].any()
    for k in ("d2", "closest", "prim", "feature"):
        assert np.array_equal(got[k][hit], full[k][hit])
    assert np.all(np.isposinf(got["d2"][~hit])) and np.all(got["prim"][~hit] == -1)
    assert np.all(got["feature"][~hit] == -1)
    assert np.array_equal(R.bits(got["closest"][~hit]), R.bits(p[~hit]))


def test_the_large_mesh_shortcut_is_the_brute_force(case):
    """brute_force_near (used for the bunny on the GPU side) leaves out only
    triangles that cannot win: on these meshes it equals the full loop."""
    _, v, i, p, full = case
    got = R.brute_force_near(v, i, p, cpuref.sdf_points(v, i, p, 16), cells=4)
    for k in ("d2", "closest", "prim", "feature"):
        assert np.array_equal(R.bits(got[k]), R.bits(full[k])), k


def test_ties_go_to_the_lowest_triangle(case):
    """An on-vertex point is at d2 = 0 from every triangle around the vertex."""
    _, v, i, p, got = case
    a, b, c = R.corners(v, i)
    n = len(p) // 3
    for k in range(2 * n, 2 * n + 32):
        on = np.flatnonzero((a == p[k]).all(1) | (b == p[k]).all(1) | (c == p[k]).all(1))
        assert on.size >= 2 and got["prim"][k] == on[0]
