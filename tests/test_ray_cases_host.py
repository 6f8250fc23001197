"""The ray recipes of ray_cases.py are real tests: on the oracle alone (no
GPU), every (scene, class, interval) that test_rays_exact_paths.py,
test_instances_exact_paths.py and test_refit_gpu.py trace has the structure it
claims and is discriminating -- the oracle hits at least 100 of its rays, or
the set is listed in ray_cases.MISSES_BY_RULE, and then the set's ulp_twin
gets at least 100 hits and the set itself fewer than half of that. A recipe
that silently became vacuous fails here.

The counts these tests print are recorded in profiles/r15/README.md.
"""
import zlib

import numpy as np
import pytest

import instances_common as IC
import ray_cases as RC
import refit_common as R

PAIRS = RC.PAIRS
CELLS = [(s, c) for s in RC.SCENES for c in RC.plain_sets(s)]
SURVIVORS = [p for p in RC.PATTERNS if not isinstance(p, str) and p[0] == "survivors"]


def _zero_axes(d):
    return (d == 0).any(axis=1)


# ------------------------------------------------------------- structure --
@pytest.mark.parametrize("scene,cls", CELLS)
def test_class_structure(ref, scene, cls):
    o, d = RC.plain_sets(scene)[cls]
    assert o.dtype == np.float32 and d.dtype == np.float32 and o.shape == d.shape == (RC.N, 3)
    assert np.isfinite(o).all() and np.isfinite(d).all()
    assert _zero_axes(d).all(), "a ray of an exact-path class has no zero direction component"
    if "one_zero" in cls or cls in ("scaled", "node_planes"):
        z = d[d == 0]
        assert np.signbit(z).any() and (~np.signbit(z)).any(), "both zero signs"
    if cls == "one_zero":
        assert ((d == 0).sum(axis=1) == 1).all()
    if cls == "lattice_axis":
        assert ((d == 0).sum(axis=1) == 2).all() and (np.abs(d).sum(axis=1) == 1).all()
    if cls == "null_dir":
        assert (d == 0).all()
    if cls == "scaled":
        ln = np.linalg.norm(d.astype(np.float64), axis=1)
        assert ln.min() < 2.0 ** -6 and ln.max() > 2.0 ** 6 and (np.abs(ln - 1) > 1e-3).mean() > 0.9
    if RC.SCENES[scene]["kind"] == "sdf":  # the safety rule
        assert cls not in ("scaled", "null_dir")
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_origins_on_box_bounds(ref):
    """Where the class says lattice, the origin coordinate on a zero axis is on
    it: exactly representable multiples, which the twin moves by one ulp."""
    for scene, step in (("lattice", 0.5), ("flat", 0.25), ("example_grid.grid", 1 / 32), ("sdf_6.octree", 1 / 32)):
        o, d = RC.plain_sets(scene)["one_zero"]
        on = o[d == 0].astype(np.float64) / step
        assert np.array_equal(on, np.round(on)), scene
        to, td = RC.ulp_twin(o, d)
        assert np.array_equal(td.view(np.uint32), d.view(np.uint32))
        moved = to != o
        assert np.array_equal(moved, d == 0)
        up, down = np.nextafter(o, np.float32(np.inf)), np.nextafter(o, np.float32(-np.inf))
        assert ((to == up) | (to == down))[moved].all() and (to == up)[moved].any() and (to == down)[moved].any()
    # integer coordinates of the lattice mesh are triangle planes and box bounds
    o, d = RC.plain_sets("lattice")["lattice_axis"]
    assert (o[d == 0] == np.round(o[d == 0])).mean() > 0.4


# -------------------------------------------------------- discrimination --
@pytest.mark.parametrize("scene,cls", CELLS)
def test_class_is_discriminating(ref, scene, cls):
    hits = [int(RC.oracle(scene, cls, tn, tf)[0].sum()) for tn, tf in PAIRS]
    if cls == "null_dir":
        print(f"{scene} {cls}: oracle hits {hits}")
        assert hits == [0, 0, 0], "the oracle hits a ray that does not move"
        return
    if (scene, cls) in RC.MISSES_BY_RULE:
        twin = [int(RC.oracle(scene, cls, tn, tf, True)[0].sum()) for tn, tf in PAIRS]
        print(f"{scene} {cls}: oracle hits {hits}, ulp_twin {twin} (MISSES_BY_RULE)")
        for h, t in zip(hits, twin):
            assert t >= 100, "the twin of a set missed by rule is hardly hit"
            assert 2 * h < t, "the set is not missed by rule"
    else:
        print(f"{scene} {cls}: oracle hits {hits}")
        assert min(hits) >= 100, "the oracle hardly hits this set"
        assert max(hits) < RC.N, "no ray misses"


def test_misses_by_rule_entries_exist():
    for scene, cls in RC.MISSES_BY_RULE:
        assert cls in RC.plain_sets(scene)


# ------------------------------------------------------------ wave make-up --
def _check_labels(o, d, lab, hi):
    assert len(o) == len(lab) == RC.NWAVES * RC.WAVE
    z = _zero_axes(d)
    assert z[lab == RC.EXACT].all() and not z[lab != RC.EXACT].any()
    if (lab == RC.AWAY).any():
        assert RC.is_away(o[lab == RC.AWAY], d[lab == RC.AWAY], hi).all()


@pytest.mark.parametrize("scene", list(RC.SCENES))
def test_mixed_waves_hold_both_flavours(ref, scene):
    for pattern in ("interleave", "shuffled"):
        o, d, lab = RC.plain_batch(scene, pattern)
        _check_labels(o, d, lab, RC.SCENES[scene]["box"][1])
        per_wave = lab.reshape(-1, RC.WAVE)
        assert ((per_wave == RC.FAST).sum(1) >= 8).all() and ((per_wave == RC.EXACT).sum(1) >= 8).all()
        h = RC.ref_scene(scene).intersect_rays(o, d, *PAIRS[0])[0]
        print(f"{scene} {pattern}: {int(h.sum())} of {len(h)} hit, {int(h[lab == RC.EXACT].sum())} of them exact")
        assert h[lab == RC.FAST].sum() >= 20 and 0 < h.sum() < len(h)
    # the permutation test_rays_device.py applies to its 4,096 rays (an eighth exact, in front)
    _, d = IC.random_rays(RC.N, zlib.crc32(f"rays-device {scene}".encode()))
    z = _zero_axes(d)[RC.shuffle_perm(RC.N)].reshape(-1, RC.WAVE)
    assert (z.sum(1) >= 1).all() and (z.sum(1) <= 63).all(), "a wave of the shuffled batch is of one flavour"
    assert not _zero_axes(d)[RC.N // 8:].any()


@pytest.mark.parametrize("scene", RC.MESH_SCENES)
def test_single_patterns(ref, scene):
    for pattern in RC.PATTERNS:
        if isinstance(pattern, str) or pattern[0] not in ("single", "single_inv"):
            continue
        o, d, lab = RC.plain_batch(scene, pattern)
        _check_labels(o, d, lab, RC.SCENES[scene]["box"][1])
        odd, rest = (RC.EXACT, RC.FAST) if pattern[0] == "single" else (RC.FAST, RC.EXACT)
        per_wave = lab.reshape(-1, RC.WAVE)
        assert (per_wave[:, pattern[1]] == odd).all() and ((per_wave == rest).sum(1) == 63).all()


@pytest.mark.parametrize("scene", RC.MESH_SCENES)
@pytest.mark.parametrize("pattern", SURVIVORS, ids=RC.pattern_id)
def test_survivor_waves(ref, scene, pattern):
    """Exactly k rays of every wave are hit by the oracle, of the flavours
    asked for; every other ray is `away` and misses."""
    _, k, flavour = pattern
    o, d, lab = RC.plain_batch(scene, pattern)
    _check_labels(o, d, lab, RC.SCENES[scene]["box"][1])
    h = RC.ref_scene(scene).intersect_rays(o, d, *PAIRS[0])[0].reshape(-1, RC.WAVE)
    per_wave = lab.reshape(-1, RC.WAVE)
    assert (h.sum(1) == k).all()
    assert np.array_equal(h != 0, per_wave != RC.AWAY)
    nfast = {"fast": k, "exact": 0, "half": k // 2}[flavour]
    assert ((per_wave == RC.FAST).sum(1) == nfast).all() and ((per_wave == RC.EXACT).sum(1) == k - nfast).all()


# ---------------------------------------------------------------- instances --
def test_instanced_poses_are_exact(rt):
    """rt_affine_inverse of the exact poses is the exact inverse, bitwise."""
    M = RC.instanced_M()
    for k, (_, x, _) in enumerate(RC.instanced_def()[:RC.N_EXACT_INST]):
        got = rt.affine_inverse(x)
        assert np.array_equal(got + np.float32(0), M[k] + np.float32(0)), f"instance {k}: {got}"  # (-0 == +0)
        s = np.abs(x[:, :3]).max()
        assert s in (0.5, 1.0, 2.0) and np.array_equal(x[:, 3], np.round(x[:, 3]))
    a, b = RC.TWINS
    assert np.array_equal(RC.instanced_def()[a][1], RC.instanced_def()[b][1])
    assert {float(np.abs(x[:, :3]).max()) for _, x, _ in RC.instanced_def()[:RC.N_EXACT_INST]} == {0.5, 1.0, 2.0}


@pytest.mark.parametrize("cls", list(RC.instanced_sets()))
def test_instanced_class(ref, cls):
    """At least 100 hits per interval; every non-coincident instance wins at
    least once; the lower of the coincident pair wins all its ties. Object-
    space rays of the exact instances keep their zeros and reach box bounds."""
    from rtamd import torch_rays
    o, d = RC.instanced_sets()[cls]
    assert _zero_axes(d).all() and len(o) == RC.N
    lo, hi = RC.instanced_boxes()
    inside = ((o[:, None, :] >= lo[None] - 1) & (o[:, None, :] <= hi[None] + 1)).all(axis=2).any(axis=1)
    assert inside.all(), "an origin lies outside the placed boxes plus a margin of 1"
    M = RC.instanced_M()
    if cls != "null_dir":
        for k in range(RC.N_EXACT_INST):
            oo, dd = IC.to_object(M[k], o, d)
            assert np.array_equal((dd == 0).sum(axis=1), (d == 0).sum(axis=1))
            on = oo[dd == 0]
            # world step 1/2 over a scale of at most 2: at least every fourth coordinate is an integer,
            # which is a triangle plane or a box bound of the lattice mesh
            assert (on == np.round(on)).mean() > 0.2, "object-space origins hardly ever lie on integer planes"
        oo, dd = IC.to_object(M[RC.N_EXACT_INST], o, d)
        assert (dd != 0).all(), "the rotated cube sees a zero direction component"
    for tn, tf in PAIRS:
        hit, t, _, prim = RC.instanced_ref(o, d, tn, tf)
        inst, _ = torch_rays.split_prim(prim)
        wins = np.bincount(inst[inst >= 0], minlength=len(M)).tolist()
        print(f"instanced {cls} [{tn}, {tf}]: {int(hit.sum())} hits, winners {wins}")
        if cls == "null_dir":
            assert int(hit.sum()) == 0
            continue
        assert int(hit.sum()) >= 100
        assert wins[RC.TWINS[1]] == 0, "the upper of the coincident pair won a tie"
        assert all(w > 0 for k, w in enumerate(wins) if k != RC.TWINS[1]), "an instance never wins"


@pytest.mark.parametrize("pattern", RC.PATTERNS, ids=RC.pattern_id)
def test_instanced_waves(ref, pattern):
    o, d, lab = RC.instanced_batch(pattern)
    _check_labels(o, d, lab, float(RC.instanced_boxes()[1][:, 0].max()))
    h = RC.instanced_ref(o, d, *PAIRS[0])[0].reshape(-1, RC.WAVE)
    per_wave = lab.reshape(-1, RC.WAVE)
    if isinstance(pattern, str):
        assert ((per_wave == RC.FAST).sum(1) >= 8).all() and ((per_wave == RC.EXACT).sum(1) >= 8).all()
        assert 20 <= h.sum() < h.size
    elif pattern[0] == "survivors":
        assert (h.sum(1) == pattern[1]).all() and np.array_equal(h != 0, per_wave != RC.AWAY)
    else:
        assert ((per_wave == (RC.EXACT if pattern[0] == "single" else RC.FAST)).sum(1) == 1).all()


# -------------------------------------------------------------------- refit --
def test_refit_sets(ref):
    """test_refit_gpu.py's case: the lattice classes shifted by refit_common's
    exact translation (exact for the origins' lattice coordinates as well), on
    the oracle of the translated vertices: at least 100 hits per interval."""
    v, i = RC.scene_input("lattice")[1]
    rs = ref.RefScene.mesh(R.translate(v), i)
    for cls in ("lattice_axis", "one_zero"):
        o, d = RC.plain_sets("lattice")[cls]
        so = o + R.SHIFT
        exact = so.astype(np.float64) == o.astype(np.float64) + R.SHIFT.astype(np.float64)
        assert exact[d == 0].all(), "a lattice coordinate left the lattice"
        for tn, tf in PAIRS:
            h = rs.intersect_rays(so, d, tn, tf)[0]
            h0 = RC.oracle("lattice", cls, tn, tf)[0]
            print(f"refit {cls} [{tn}, {tf}]: {int(h.sum())} hits on the translated mesh, {int(h0.sum())} before")
            assert int(h.sum()) >= 100
