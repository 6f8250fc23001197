"""rt_scene_update_grid_device: a grid scene created from values A takes values
B from a device buffer, and is then bit for bit a fresh SDFGrid of B: a 64x48
frame in primary (normal) and default mode, a ray batch, and the same batch
through a mixed instanced scene that was created before the update. Sizes
5x6x7 and 9^3, each in the linear layout and in the bricked one (forced with
rtx_set_grid_force(1), restored afterwards). B is the SDF of spot on the
scene's lattice, written into a tensor by sdf_grid.
"""
import ctypes as C

import numpy as np
import pytest

import instances_common as IC
import points_ref as R
import ray_cases as RAYS
import sdf_scenes_common as SC

pytestmark = pytest.mark.gpu

RT_E_INVALID, RT_E_STATE = -1, -4
W, H = 64, 48
SIZES = [(5, 6, 7), (9, 9, 9)]


def live(rt):
    out = (C.c_int64 * 4)()
    rt._lib.check(rt.lib().rtx_live_resources(out))
    return tuple(out)


def make_grid(rt, size, values, bricked):
    L = rt.lib()
    L.rtx_set_grid_force.argtypes = [C.c_int]
    rt._lib.check(L.rtx_set_grid_force(1 if bricked else 0))
    try:
        return rt.SDFGrid(size, values)
    finally:
        rt._lib.check(L.rtx_set_grid_force(0))


def values_a(size):
    """a sphere of radius 0.5 on the lattice"""
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, n) for n in size], indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - 0.5).astype(np.float32).ravel()


@pytest.fixture(scope="module")
def rays(gpu):
    import torch
    sets = [RAYS.aimed(1024, (-0.9, 0.9), (-2.5, 2.5), 17), RAYS.lattice_axis(512, -1.0, 1.0, 0.25, 18),
            RAYS.one_zero(512, (-0.8, 0.8), (-1.5, 1.5, 0.25), 19)]
    o = np.concatenate([s[0] for s in sets])
    d = np.concatenate([s[1] for s in sets])
    return torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()


@pytest.fixture(scope="module")
def spot(gpu, rt):
    with rt.SDFMesh(rt.SimpleMesh(*SC.mesh("spot"))) as m:
        yield m


def trace(scene, rays):
    from rtamd import torch_rays
    h = torch_rays.trace(scene, *rays)
    return (h.hit.cpu().numpy(), R.bits(h.t.cpu().numpy()), R.bits(h.normal.cpu().numpy()), h.prim.cpu().numpy())


def frames(rt, scene):
    import torch
    pos = (0.3, 0.4, 2.5)
    vi, pi = rt.camera_matrices(pos, aspect=W / H)
    out = []
    for kw in (dict(mode=rt.ShadingMode.Normal, shadows=False, reflections=False), dict(mode=rt.ShadingMode.Lambert)):
        c = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        t = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        scene.render_device(rt.render_params(pos, vi, pi, **kw), c.data_ptr(), t.data_ptr(), W, H,
                            stream=torch.cuda.current_stream().cuda_stream)
        out += [c.cpu().numpy(), R.bits(t.cpu().numpy())]
    return out


def same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), k


@pytest.mark.parametrize("bricked", [False, True], ids=["linear", "bricked"])
@pytest.mark.parametrize("size", SIZES, ids=["5x6x7", "9x9x9"])
def test_updated_grid_equals_a_fresh_one(gpu, rt, rays, spot, size, bricked):
    from rtamd import torch_rays
    start = live(rt)
    b = torch_rays.sdf_grid(spot, size)
    hb = b.cpu().numpy().ravel()
    inst = [(0, IC.affine(IC.rot(3), (-0.9, 0.0, 0.1))), (1, IC.affine(IC.rot(4), (0.9, 0.1, -0.1)))]
    with rt.BVHBuilder(rt.SimpleMesh(*SC.mesh("cube"))) as cube, make_grid(rt, size, values_a(size), bricked) as g, \
            make_grid(rt, size, hb, bricked) as fresh:
        with rt.InstancedScene([cube, g], inst) as ia, rt.InstancedScene([cube, fresh], inst) as ib:
            old = trace(g, rays)
            assert g.device_bytes() == fresh.device_bytes()
            made = live(rt)
            torch_rays.update_sdf_grid(g, b)  # queued on the stream of sdf_grid's kernel, no wait between
            assert live(rt) == made  # the update allocated nothing
            got = trace(g, rays)
            same(got, trace(fresh, rays))
            assert not np.array_equal(got[1], old[1])  # A and B differ in what the rays see
            same(frames(rt, g), frames(rt, fresh))
            same(trace(ia, rays), trace(ib, rays))
    assert live(rt) == start


def test_refusals(gpu, rt):
    import torch
    v = torch.zeros(27, dtype=torch.float32, device="cuda")
    with rt.BVHBuilder(rt.SimpleMesh(*SC.mesh("cube"))) as cube, rt.SDFGrid((3, 3, 3), np.ones(27, np.float32)) as g:
        with pytest.raises(rt.RtError, match=f"rtamd error {RT_E_STATE}"):
            # (a mesh scene has no update_device: the C entry is called)
            rt._lib.check(rt.lib().rt_scene_update_grid_device(cube._handle(), v.data_ptr(), None))
        with pytest.raises(rt.RtError, match=f"rtamd error {RT_E_INVALID}"):
            g.update_device(0)
        from rtamd import torch_rays
        with pytest.raises(ValueError):
            torch_rays.update_sdf_grid(g, v[:26])
        with pytest.raises(ValueError):
            torch_rays.update_sdf_grid(g, v.cpu())
