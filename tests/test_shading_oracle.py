"""The oracle's shading path against an independent restatement, bit for bit.

oracle/cpuref.cpp's Renderer::color, Plane and SceneUnion are what every GPU
parity test trusts. Here they are compared with tests/shading_ref.py, a numpy
float32 restatement written from the reference text, over tilted, non-unit and
never-hit planes, lights inside / below / far from the model, and every
shadow x reflection switch combination: colour words, t bits and hit
primitives of whole frames, and hit / t / normal / primitive of random rays.
No GPU is involved.
"""
import numpy as np
import pytest

import shading_ref as R

# the scenes of tests/test_gpu_shading.py: what it compares the kernels with is checked here
SCENES = ["cube.obj", "stanford-bunny.obj", "rand", "example_grid.grid", "sdf_5.octree", "sdf_6.octree"]
W, H = R.FLOOR_SIZE
FLAT_PLANE, FLAT_CAMERAS = R.FLAT_PLANE, R.FLAT_CAMERAS


def assert_frame(fr, oracle, what):
    c, t, prim = oracle
    assert fr.defined, f"{what}: a shaded channel is NaN or outside [0, 1]"
    assert np.array_equal(np.isfinite(t), np.isfinite(fr.t)), f"{what}: hit mask"
    assert np.array_equal(prim, fr.prim), f"{what}: {int((prim != fr.prim).sum())} primitives differ"
    assert np.array_equal(c, fr.color), f"{what}: {int((c != fr.color).sum())} colour px differ"
    assert np.array_equal(t.view(np.uint32), fr.t.view(np.uint32)), f"{what}: t bits"


@pytest.mark.parametrize("W,H", R.SIZES)
@pytest.mark.parametrize("key", SCENES)
def test_oracle_frames_equal_restatement(ref, key, W, H):
    """Every case of the parameter space: the oracle's frame is the restatement's,
    and no channel it packs is NaN or outside [0, 1]."""
    base = R.base_scene(key)
    for case in R.cases():
        pn, ln, mode, sh, rf = case
        fr = R.render(base, R.plane_for(key, pn), R.params(W, H, R.LIGHTS[ln], mode, sh, rf), W, H)
        assert_frame(fr, R.oracle_case(key, W, H, case), f"{key} {case}")


@pytest.mark.parametrize("key", SCENES)
def test_cases_are_not_vacuous(ref, key):
    R.assert_floors(key)


def test_never_hit_plane_equals_plane_off(ref):
    """The (0, 0, 0) plane is enabled and cannot be hit: the plane-off image."""
    for key in SCENES:
        base = R.base_scene(key)
        for ln in R.LIGHTS:
            case = ("never", ln, R.LAMBERT, True, True)
            off = R.oracle_frame(base, None, R.params(W, H, R.LIGHTS[ln], R.LAMBERT, True, True), W, H)
            on = R.oracle_case(key, W, H, case)
            assert np.array_equal(off[0], on[0]) and np.array_equal(off[1].view(np.uint32), on[1].view(np.uint32))


@pytest.mark.parametrize("key", ["stanford-bunny.obj", "example_grid.grid", "sdf_6.octree"])
def test_batch_frames(ref, key):
    """The six differing frames of the GPU suite's multi-frame launch."""
    base = R.base_scene(key)
    plane = R.plane_for(key, R.BATCH_PLANE)
    for W_, H_ in R.SIZES:
        for k, P in enumerate(R.batch_params(W_, H_)):
            assert_frame(R.render(base, plane, P, W_, H_), R.oracle_frame(base, plane, P, W_, H_), f"{key} frame {k}")


@pytest.mark.parametrize("key", ["stanford-bunny.obj", "sdf_5.octree"])
def test_uniform_finite_tprev(ref, key):
    """tPrev = 2.4 everywhere over a patterned colour buffer: tfar = min(100,
    tPrev) cuts the primary ray only, and unhit pixels keep the pattern."""
    base = R.base_scene(key)
    c0 = (np.arange(W * H, dtype=np.uint32).reshape(H, W) * np.uint32(2654435761)) | np.uint32(1)
    t0 = np.full((H, W), 2.4, np.float32)
    for pn, ln in (("xdom", "side"), ("nonunit", "std")):
        P = R.params(W, H, R.LIGHTS[ln], R.LAMBERT, True, True)
        plane = R.plane_for(key, pn)
        fr = R.render(base, plane, P, W, H, c0, t0)
        oc = R.oracle_frame(base, plane, P, W, H, c0, t0)
        kept = fr.t == np.float32(2.4)
        assert 500 < kept.sum() < W * H - 500, "tPrev must cut some pixels and not others"
        assert np.array_equal(fr.color[kept], c0[kept])
        assert fr.defined
        assert np.array_equal(oc[0], fr.color), f"{key} {pn}: {int((oc[0] != fr.color).sum())} colour px differ"
        assert np.array_equal(oc[1].view(np.uint32), fr.t.view(np.uint32))


@pytest.mark.parametrize("pos", FLAT_CAMERAS)
def test_coplanar_union_ties(ref, pos):
    """120 triangles in the plane y = -0.25 and the plane itself: where both
    report the same t the union returns the plane (albedo of the checkerboard,
    reflectiveness 0.3), elsewhere the nearer one."""
    base = R.base_scene("flat")
    for mode in (R.LAMBERT, R.COLOR):
        P = R.params(W, H, R.LIGHTS["std"], mode, True, True, pos=pos)
        fr = R.render(base, FLAT_PLANE, P, W, H)
        assert fr.ties >= 100, f"only {fr.ties} exact ties: the case is vacuous"
        assert_frame(fr, R.oracle_frame(base, FLAT_PLANE, P, W, H), f"flat {pos} mode {mode}")


@pytest.mark.parametrize("key", ["stanford-bunny.obj", "example_grid.grid", "sdf_5.octree", "sdf_6.octree", "flat"])
def test_oracle_rays_equal_restatement(ref, key):
    """Plane-on intersect_rays on random rays (origins inside the model box too)."""
    base = R.base_scene(key)
    planes = [FLAT_PLANE] if key == "flat" else [R.plane_for(key, pn) for pn in R.PLANES if pn != "base"]
    for plane in planes:
        for tn, tf in ((0.01, 100.0), (-5.0, 100.0)):
            o, d = R.random_rays(key, plane, tn)
            h = R.Scene(base, R.Plane(*plane)).intersect(o, d, tn, tf)
            base.set_plane(True, *plane)
            rh, rt_, rn, rp = base.intersect_rays(o, d, tn, tf)
            what = f"{key} {plane} tn={tn}"
            assert np.array_equal(rh.astype(bool), h.hit), f"{what}: hit mask"
            assert np.array_equal(rp, h.prim), f"{what}: primitives"
            m = h.hit
            assert np.array_equal(rt_[m].view(np.uint32), h.t[m].view(np.uint32)), f"{what}: t"
            assert np.array_equal(rn[m].view(np.uint32), h.normal[m].view(np.uint32)), f"{what}: normal"
            if plane[0] != (0.0, 0.0, 0.0):
                assert (h.prim == -2).sum() > 1000 and (h.prim >= 0).sum() > 1000, what
