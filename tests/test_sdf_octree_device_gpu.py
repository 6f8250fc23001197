"""rt_sdf_mesh_octree_device: an octree scene rebuilt on the device from an
SDF-mesh handle, against the oracle (cpuref.sdf_octree), bit for bit, in three
views: the 36-byte nodes the scene gives back (SDFOctree.nodes), the {child,
masks} words on the device against rth::flatten_octree of the oracle's nodes,
and a ray query against a fresh SDFOctree of the oracle's nodes.

The cases are those test_sdf_scenes_host.py pins: one node, levels below and
above the scan's 1024-cell tile, a root that is never refined, 8-cell levels,
capacities that are exactly the count, and trees that pass the capacity at the
last and at an inner level and must leave the scene as it was. Then a mesh that
deforms, two rebuilds back to back, the scene under instanced scenes, the
refusals and the leak check.
"""
import ctypes as C

import numpy as np
import pytest

import cpuref
import instances_common as IC
import points_ref as R
import ray_cases as RAYS
import sdf_refit_common as SR
import sdf_scenes_common as SC

pytestmark = pytest.mark.gpu

RT_E_STATE = -4
S32 = 1.0 / 32.0


def live(rt):
    out = (C.c_int64 * 4)()
    rt._lib.check(rt.lib().rtx_live_resources(out))
    return tuple(out)


@pytest.fixture(scope="module")
def rays(gpu):
    """3072 rays with unit directions (ray_cases' rule for SDF scenes): aimed
    from outside, axis-parallel on the leaf lattice, one zero component."""
    import torch
    sets = [RAYS.aimed(1024, (-0.9, 0.9), (-2.5, 2.5), 7), RAYS.lattice_axis(1024, -1.0, 1.0, S32, 8),
            RAYS.one_zero(1024, (-0.8, 0.8), (-1.5, 1.5, S32), 9)]
    o = np.concatenate([s[0] for s in sets])
    d = np.concatenate([s[1] for s in sets])
    return torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()


def trace(scene, rays):
    from rtamd import torch_rays
    h = torch_rays.trace(scene, *rays)
    return (h.hit.cpu().numpy(), R.bits(h.t.cpu().numpy()), R.bits(h.normal.cpu().numpy()), h.prim.cpu().numpy())


def same_trace(a, b):
    for x, y, what in zip(a, b, ("hit", "t", "normal", "prim")):
        assert np.array_equal(x, y), what


def check_scene(rt, dyn, want, rays, overflow=0):
    """The scene holds `want` (36-byte nodes): status, nodes, words and a trace."""
    count = want.size // 36
    assert dyn.status() == (count, overflow)
    assert np.array_equal(dyn.nodes(), want)
    assert np.array_equal(SC.scene_words(rt, dyn, count), SC.flatten(rt, want)[2])
    with rt.SDFOctree(want) as fresh:
        same_trace(trace(dyn, rays), trace(fresh, rays))


def sdf_mesh(rt, key, dynamic=False):
    return rt.SDFMesh(rt.SimpleMesh(*SC.mesh(key)), dynamic=dynamic)


@pytest.mark.parametrize("key,depth", [("cube", 0), ("cube", 1), ("cube", 2), ("cube", 4), ("cube", 5), ("cube", 6),
                                       ("spot", 4), ("bunny", 3), ("corner_cube", 4)])
def test_build_equals_the_oracle(gpu, rt, rays, key, depth):
    """max_nodes is exactly the count (cube depth 0: a capacity-1 scene)"""
    want = SC.oracle_nodes(key, depth)
    with sdf_mesh(rt, key) as m, rt.SDFOctree.dynamic(depth, want.size // 36) as dyn:
        assert dyn.status() == (1, 0) and dyn.tree_stats()[2] == depth
        assert not trace(dyn, rays)[0].any()  # the initial tree: one empty leaf
        m.octree_device(dyn)
        check_scene(rt, dyn, want, rays)


def test_bunny_depth_6_equals_the_host_build(gpu, rt, rays):
    with sdf_mesh(rt, "bunny") as m:
        want = m.octree(6)
        with rt.SDFOctree.dynamic(6, want.size // 36) as dyn:
            m.octree_device(dyn)
            check_scene(rt, dyn, want, rays)


def test_far_cube_is_one_node_in_a_depth_3_scene(gpu, rt, rays):
    """outside the oracle's exactness domain: the handle's host build is the
    reference; the stack class (depth 3) is not the fresh scene's (depth 0)"""
    with sdf_mesh(rt, "far_cube") as m, rt.SDFOctree.dynamic(3, 1) as dyn:
        want = m.octree(3)
        assert want.size == 36
        m.octree_device(dyn)
        check_scene(rt, dyn, want, rays)
        assert dyn.tree_stats()[2] == 3


@pytest.mark.parametrize("first,cap", [("spot", 1097), ("corner_cube", 100)])
def test_overflow_keeps_the_tree(gpu, rt, rays, first, cap):
    """the cube's depth-4 tree (2249 nodes) passes 1097 at its last level and
    100 at level 3: the build is dropped, the scene keeps the tree it had"""
    want = SC.oracle_nodes(first, 4)
    with sdf_mesh(rt, first) as m, sdf_mesh(rt, "cube") as cube, rt.SDFOctree.dynamic(4, cap) as dyn:
        m.octree_device(dyn)
        check_scene(rt, dyn, want, rays)
        cube.octree_device(dyn)
        check_scene(rt, dyn, want, rays, overflow=1)
        m.octree_device(dyn)
        check_scene(rt, dyn, want, rays)


def test_deforming_mesh_same_stream_no_wait(gpu, rt, rays):
    import torch
    from rtamd import torch_rays
    v, i = SR.mesh("spot")
    w = SR.shear(v)
    want = np.ascontiguousarray(cpuref.sdf_octree(w, i, 4, 16)).view(np.uint8).reshape(-1)
    with rt.SDFMesh(rt.SimpleMesh(v, i), dynamic=True) as m, rt.SDFOctree.dynamic(4, want.size // 36) as dyn, \
            rt.SDFMesh(rt.SimpleMesh(w, i)) as fresh:
        verts = torch.from_numpy(np.array(w, order="C")).cuda()
        torch_rays.update_sdf_mesh(m, verts)
        torch_rays.update_sdf_octree(m, dyn)
        got = dyn.nodes()
        assert dyn.status() == (want.size // 36, 0)
        assert np.array_equal(got, m.octree(4))
        assert np.array_equal(SC.offsets(got), SC.offsets(want))
        gv, wv = SC.values(got).view(np.float32), SC.values(want).view(np.float32)
        assert np.array_equal(R.bits(np.abs(gv)), R.bits(np.abs(wv)))
        # signs: wherever the winning feature's pseudonormal has the fresh handle's bits
        leaves, p = SC.leaf_corners(want, 4)
        h = torch_rays.closest(m, torch.from_numpy(p.reshape(-1, 3)).cuda(), outputs=("prim", "feature"))
        prim, feat = h.prim.cpu().numpy(), h.feature.cpu().numpy()
        pn, pnf = m.pseudonormals(), fresh.pseudonormals()
        entry = (R.bits(pn[prim, feat, :3]) == R.bits(pnf[prim, feat, :3])).all(1).reshape(-1, 8)
        print(f"{int((~entry).sum())} of {entry.size} corner values excluded from the sign comparison")
        assert (~entry).mean() <= 0.01
        assert np.array_equal(R.bits(gv[leaves])[entry], R.bits(wv[leaves])[entry])
        # (everything but the full-depth leaves is 0 or 1000)
        rest = np.setdiff1d(np.arange(len(gv)), leaves)
        assert np.array_equal(R.bits(gv[rest]), R.bits(wv[rest]))


def test_two_rebuilds_back_to_back_then_one_trace(gpu, rt, rays):
    want = SC.oracle_nodes("spot", 4)
    with sdf_mesh(rt, "cube") as cube, sdf_mesh(rt, "spot") as spot, rt.SDFOctree.dynamic(4, 2249) as dyn, \
            rt.SDFOctree(want) as fresh:
        cube.octree_device(dyn)
        spot.octree_device(dyn)
        got = trace(dyn, rays)
        same_trace(got, trace(fresh, rays))
        check_scene(rt, dyn, want, rays)


@pytest.mark.parametrize("tlas", [False, True])
def test_as_a_bottom_level_scene(gpu, rt, rays, tlas):
    """the instanced scene is made over the empty tree and never touched again"""
    want = SC.oracle_nodes("spot", 4)
    inst = [(0, IC.affine(IC.rot(3), (-0.9, 0.0, 0.1))), (1, IC.affine(IC.rot(4), (0.9, 0.1, -0.1))),
            (1, IC.affine(IC.rot(5) @ np.diag([0.5, 0.5, 0.5]), (0.0, 0.9, 0.0)))]
    with rt.BVHBuilder(rt.SimpleMesh(*SC.mesh("bunny"))) as bunny, sdf_mesh(rt, "spot") as m, \
            rt.SDFOctree.dynamic(4, 1097) as dyn, rt.SDFOctree(want) as fresh:
        with rt.InstancedScene([bunny, dyn], inst, tlas=tlas) as a, rt.InstancedScene([bunny, fresh], inst, tlas=tlas) as b:
            empty = trace(a, rays)
            m.octree_device(dyn)
            got, ref = trace(a, rays), trace(b, rays)
            same_trace(got, ref)
            assert not np.array_equal(got[0], empty[0])  # the octree instances are hit now


def test_refusals_launch_nothing(gpu, rt, rays):
    want = SC.oracle_nodes("cube", 2)
    with sdf_mesh(rt, "cube") as m, rt.SDFOctree(want) as plain, rt.SDFOctree.dynamic(2, 73) as dyn, \
            rt.SDFGrid((3, 3, 3), np.ones(27, np.float32)) as grid:
        m.octree_device(dyn)
        before = dyn.status()
        for target in (plain, grid):
            with pytest.raises(rt.RtError, match=f"rtamd error {RT_E_STATE}"):
                m.octree_device(target)
        with pytest.raises(rt.RtError, match="rtamd error -1"):
            rt._lib.check(rt.lib().rt_sdf_mesh_octree_device(None, dyn._handle(), None))
        assert dyn.status() == before == (73, 0)
        # the getters take any octree scene
        assert plain.status() == (73, 0) and np.array_equal(plain.nodes(), want)
        with pytest.raises(rt.RtError, match=f"rtamd error {RT_E_STATE}"):
            rt._lib.check(rt.lib().rt_scene_octree_status(grid._handle(), None, None))
        check_scene(rt, dyn, want, rays)


def test_handles_give_everything_back(gpu, rt):
    """a dynamic octree holds its two scene arrays at capacity, the status words
    and seven scratch arrays, all counted in device_bytes; a build allocates
    nothing; destruction returns the counters to where they were"""
    import torch
    torch.cuda.synchronize()
    start = live(rt)
    m = sdf_mesh(rt, "cube")
    with_mesh = live(rt)
    dyn = rt.SDFOctree.dynamic(4, 2249)
    made = live(rt)
    assert made[0] - with_mesh[0] == 10 and made[1:] == with_mesh[1:]
    assert dyn.device_bytes() == 2249 * 40 + 8 + 2249 * 48 + 3072 * 4 + 3 * 4 + 32 * 4 + 585 * 4
    m.octree_device(dyn)
    assert dyn.status() == (2249, 0)
    assert live(rt) == made
    dyn.close()
    assert live(rt) == with_mesh
    m.close()
    assert live(rt) == start
