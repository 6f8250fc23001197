"""The shading kernels (GENERAL = true: union_intersect, union_occluded,
plane_hit, lambert_color, shade_one; the basis of rt_scene_set_plane) against
the oracle, bit for bit, over plane, light and switch settings.

The parameter space and what the oracle computes for it are in
tests/shading_ref.py; tests/test_shading_oracle.py checks the oracle itself on
the same cases (and that none of them is vacuous or packs an undefined
colour), so here each case is one comparison: the GPU's frame or hits equal
the oracle's. Scenes reach every shading kernel family: meshes of different
stack depths, the grid in its linear and bricked layouts, both octrees.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import rtamd
import scenes as S
import shading_ref as R
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

GRID = "example_grid.grid"
# scene key -> (oracle scene, rtx_set_grid_force value or None)
SCENES = {
    "cube.obj": ("cube.obj", None),
    "stanford-bunny.obj": ("stanford-bunny.obj", None),
    "rand": ("rand", None),
    "grid-linear": (GRID, 0),
    "grid-bricked": (GRID, 1),        # bricked layout, 32-bit buffer loads
    "grid-bricked-wide": (GRID, 3),   # bricked layout, 64-bit address loads
    "sdf_5.octree": ("sdf_5.octree", None),
    "sdf_6.octree": ("sdf_6.octree", None),
}
_soups = {}


@contextlib.contextmanager
def gpu_scene(key):
    """-> (oracle scene key, GPU scene); a grid is created and rendered under
    its forced layout, which is restored afterwards."""
    okey, force = SCENES.get(key, (key, None))
    if force is not None:
        from rtamd import _lib
        L = rtamd.lib()
        L.rtx_set_grid_force.argtypes = [C.c_int]
        _lib.check(L.rtx_set_grid_force(force))
        try:
            gs = rtamd.SDFGrid(*S.inputs(GRID)[1])
            try:
                yield okey, gs
            finally:
                gs.close()
        finally:
            _lib.check(L.rtx_set_grid_force(0))
    elif okey in R.SOUPS:
        if okey not in _soups:
            _soups[okey] = rtamd.BVHBuilder(rtamd.SimpleMesh(*R.soup_mesh(okey)))
        yield okey, _soups[okey]
    else:
        yield okey, S.gpu_scene(okey)


def set_plane(gs, plane):
    gs.set_plane(rtamd.Plane(tuple(float(x) for x in plane[0]), float(plane[1])) if plane is not None else None)


def host_frame(gs, P, W, H):
    c = np.full((H, W), 0xABABABAB, np.uint32)  # clear=True overwrites whatever is there
    t = np.full((H, W), -5.0, np.float32)
    gs.render(P, c, t, clear=True)
    return c, t


# ------------------------------------------------------ a. one-frame kernel --
@pytest.mark.parametrize("W,H", R.SIZES)
@pytest.mark.parametrize("key", list(SCENES))
def test_plane_light_switch_grid(gpu, key, W, H):
    """rt_render on host buffers: every plane x light x switch case."""
    with gpu_scene(key) as (okey, gs):
        for case in R.cases():
            pn, ln, mode, sh, rf = case
            set_plane(gs, R.plane_for(okey, pn))
            got = host_frame(gs, R.params(W, H, R.LIGHTS[ln], mode, sh, rf, module=rtamd), W, H)
            assert_same(R.oracle_case(okey, W, H, case)[:2], got, f"{key} {W}x{H} {case}")


@pytest.mark.parametrize("key", list(SCENES))
def test_device_buffers_subset(gpu, key):
    """rt_render_device: 2 normals x 2 lights x the 4 switch combinations."""
    torch = pytest.importorskip("torch")
    W, H = R.SIZES[1]
    with gpu_scene(key) as (okey, gs):
        for case in R.cases(planes=("xdom", "nonunit"), lights=("side", "below")):
            pn, ln, mode, sh, rf = case
            if mode != R.LAMBERT:
                continue
            set_plane(gs, R.plane_for(okey, pn))
            c = torch.full((H, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            t = torch.full((H, W), -5.0, dtype=torch.float32, device="cuda")
            gs.render_device(R.params(W, H, R.LIGHTS[ln], mode, sh, rf, module=rtamd), c.data_ptr(), t.data_ptr(),
                             W, H, clear=True)
            torch.cuda.synchronize()
            assert_same(R.oracle_case(okey, W, H, case)[:2], (c.cpu().numpy().view(np.uint32), t.cpu().numpy()),
                        f"{key} device {case}")


# ----------------------------------------------------- b. multi-frame launch --
def batch_oracle(okey, W, H):
    base, plane = R.base_scene(okey), R.plane_for(okey, R.BATCH_PLANE)
    return [R.oracle_frame(base, plane, P, W, H)[:2] for P in R.batch_params(W, H)]


def launch_frames(torch, gs, P, npx, W, H, tile=None):
    cs = [torch.full((npx,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in P]
    ts = [torch.full((npx,), -5.0, dtype=torch.float32, device="cuda") for _ in P]
    gs.render_device_frames(P, [c.data_ptr() for c in cs], [t.data_ptr() for t in ts], W, H, rtamd.RT_FLAG_CLEAR,
                            tile=tile)
    torch.cuda.synchronize()
    return [(c.cpu().numpy().view(np.uint32), t.cpu().numpy()) for c, t in zip(cs, ts)]


@pytest.mark.parametrize("W,H", R.SIZES)
@pytest.mark.parametrize("key", ["stanford-bunny.obj", "sdf_6.octree", "grid-linear", "grid-bricked"])
def test_batch_of_differing_frames(gpu, key, W, H):
    """ONE rt_render_device_frames call of six frames that differ in camera,
    light, both switches and shading mode (Lambert, Color and Normal mixed; the
    plane is on, so every frame takes the shading kernels): each frame equals
    the oracle's frame for its own parameters. Whole frames go through
    render_persist_kernel<..., true> (mesh, octree) or render_batch_kernel<...,
    true> (grid)."""
    torch = pytest.importorskip("torch")
    with gpu_scene(key) as (okey, gs):
        set_plane(gs, R.plane_for(okey, R.BATCH_PLANE))
        got = launch_frames(torch, gs, R.batch_params(W, H, module=rtamd), W * H, W, H)
        for k, (ref_f, (c, t)) in enumerate(zip(batch_oracle(okey, W, H), got)):
            assert_same(ref_f, (c.reshape(H, W), t.reshape(H, W)), f"{key} {W}x{H} batch frame {k}")


@pytest.mark.parametrize("band", [8, 12])
def test_batch_row_bands(gpu, band):
    """The same six frames as two ranks' packed row bands (render_batch_kernel
    on a mesh): each rank's rows equal the oracle's rows of that frame."""
    torch = pytest.importorskip("torch")
    W, H = R.SIZES[1]
    with gpu_scene("stanford-bunny.obj") as (okey, gs):
        set_plane(gs, R.plane_for(okey, R.BATCH_PLANE))
        want = batch_oracle(okey, W, H)
        for rank in range(2):
            tile = rtamd.Tile(band, rank, 2, 0)
            rows = rtamd.tiles.rank_rows(H, band, rank, 2)
            npx = int(rtamd.lib().rt_tile_pixels(W, H, C.byref(tile)))
            assert npx == len(rows) * W
            got = launch_frames(torch, gs, R.batch_params(W, H, module=rtamd), npx, W, H, tile=tile)
            for k, ((rc, rt_), (c, t)) in enumerate(zip(want, got)):
                assert_same((rc[rows], rt_[rows]), (c.reshape(-1, W), t.reshape(-1, W)),
                            f"band {band} rank {rank} frame {k}")


# ----------------------------------------------------------------- c. refusal --
def test_mixed_shading_paths_refused(gpu):
    """Plane off: a Normal frame takes the primary-ray kernels and a Lambert
    frame the shading kernels; one launch cannot hold both. RT_E_INVALID, the
    message names the shading path, and no frame buffer is touched."""
    torch = pytest.importorskip("torch")
    W, H = R.SIZES[0]
    with gpu_scene("stanford-bunny.obj") as (_, gs):
        gs.set_plane(None)
        P = [R.params(W, H, R.LIGHTS["std"], mode, True, True, module=rtamd) for mode in (R.NORMAL, R.LAMBERT)]
        pat = (torch.arange(W * H, dtype=torch.int32, device="cuda") * 40503) | 1
        cs = [pat.clone() for _ in P]
        ts = [torch.full((W * H,), 2.4, dtype=torch.float32, device="cuda") for _ in P]
        L = rtamd.lib()
        rc = L.rt_render_device_frames(gs._handle(), (rtamd.RenderParams * 2)(*P), 2,
                                       (C.c_void_p * 2)(*[c.data_ptr() for c in cs]),
                                       (C.c_void_p * 2)(*[t.data_ptr() for t in ts]), W, H, rtamd.RT_FLAG_CLEAR,
                                       None, None)
        torch.cuda.synchronize()
        assert rc == -1  # RT_E_INVALID (include/rtamd.h)
        assert "shading path" in L.rt_last_error().decode()
        for c, t in zip(cs, ts):
            assert torch.equal(c, pat)
            assert bool((t == 2.4).all())


# --------------------------------------------------------------- d. ray level --
def assert_rays(okey, gs, plane):
    base = R.base_scene(okey)
    base.set_plane(True, *plane)
    set_plane(gs, plane)
    for tn, tf in ((0.01, 100.0), (-5.0, 100.0)):
        o, d = R.random_rays(okey, plane, tn)
        rh, rt_, rn, rp = base.intersect_rays(o, d, tn, tf)
        g = gs.intersect(o, d, tn, tf)
        what = f"{okey} plane {plane} tn={tn}"
        if plane[0] != (0.0, 0.0, 0.0):
            assert (rp == -2).sum() > 1000 and (rp >= 0).sum() > 1000, f"{what}: too few hits to be a test"
        assert np.array_equal(rh.astype(bool), g.hitten), f"{what}: hit mask"
        assert np.array_equal(rp, g.prim), f"{what}: primitive ids"
        h = g.hitten
        assert np.array_equal(rt_[h].view(np.uint32), g.t[h].view(np.uint32)), f"{what}: t"
        assert np.array_equal(rn[h].view(np.uint32), g.normal[h].view(np.uint32)), f"{what}: normal"


@pytest.mark.parametrize("key", ["stanford-bunny.obj", "grid-linear", "grid-bricked", "sdf_6.octree"])
def test_intersect_rays_tilted_planes(gpu, key):
    """rt_intersect_rays with every plane but (0, 1, 0), -1: hit mask, primitive
    (-2 for the plane), t and the normal as given (not normalised)."""
    with gpu_scene(key) as (okey, gs):
        for pn in R.PLANES:
            if pn != "base":
                assert_rays(okey, gs, R.plane_for(okey, pn))


# ---------------------------------------------------------- e. coplanar union --
@pytest.mark.parametrize("pos", R.FLAT_CAMERAS)
def test_coplanar_union(gpu, pos):
    """120 triangles in the plane's own plane: where both report the same t the
    union keeps the plane (!(mesh.t < plane.t)), next to pixels where the mesh
    is nearer and pixels where the plane is."""
    base = R.base_scene("flat")
    with gpu_scene("flat") as (_, gs):
        set_plane(gs, R.FLAT_PLANE)
        for W, H in R.SIZES:
            for mode in (R.LAMBERT, R.COLOR):
                P = R.params(W, H, R.LIGHTS["std"], mode, True, True, pos=pos)
                c, t, prim = R.oracle_frame(base, R.FLAT_PLANE, P, W, H)
                if (W, H) == R.FLOOR_SIZE:
                    fr = R.render(base, R.FLAT_PLANE, P, W, H)
                    assert fr.ties >= 100 and np.array_equal(fr.prim, prim), "too few exact ties to be a test"
                    assert (prim >= 0).sum() > 0 and (prim == -2).sum() > fr.ties
                got = host_frame(gs, R.params(W, H, R.LIGHTS["std"], mode, True, True, pos=pos, module=rtamd), W, H)
                assert_same((c, t), got, f"flat {pos} {W}x{H} mode {mode}")


def test_coplanar_union_rays(gpu):
    with gpu_scene("flat") as (_, gs):
        assert_rays("flat", gs, R.FLAT_PLANE)


# --------------------------------------------------------------------- f. basis --
def test_plane_is_stored_as_given(gpu):
    """rt_scene_get_plane returns the normal and the offset bit for bit: no
    normalisation, the sign of a zero kept."""
    with gpu_scene("cube.obj") as (_, gs):
        L = rtamd.lib()
        for normal, offset in R.PLANES.values():
            set_plane(gs, (normal, offset))
            on, n, off = C.c_int(0), np.zeros(3, np.float32), C.c_float(0.0)
            rtamd._lib.check(L.rt_scene_get_plane(gs._handle(), C.byref(on), n.ctypes.data_as(C.c_void_p),
                                                  C.byref(off)))
            assert on.value == 1
            assert np.array_equal(n.view(np.uint32), np.asarray(normal, np.float32).view(np.uint32)), normal
            assert np.float32(off.value).view(np.uint32) == np.float32(offset).view(np.uint32)
