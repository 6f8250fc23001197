"""What a handle holds, and that it gives all of it back.

Every rt_scene and rt_sdf_mesh keeps its device arrays, pinned host blocks,
events and streams in the owners of csrc/rt_mem.h; rtx_live_resources counts
the live ones, in that order. The tests read those four counters around each
step (never the device's free memory, which other users of the card move):
after a scene was created, after every lazily made part was brought in, after
a regrow, on the failure paths, for replicas, and after destruction, where
they are back at their values from before.

Inputs are tiny: the 12-triangle cube, a 3x2x2 grid and a 5x4x3 grid forced
bricked, the depth-1 hand-built octree, instanced scenes of two cubes and
three instances. Frames are 16x16 and 40x24, ray batches 70 rays (one full
wave and one partial wave).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import octree_cases as O
import scenes as S

pytestmark = pytest.mark.gpu

RT_E_DEVICE = -3
RT_BVH_AUTO, RT_BVH_DEVICE = 0, 2
SMALL, LARGE = (16, 16), (40, 24)

KINDS = ["mesh", "dynmesh", "grid", "bricked", "octree", "inst", "inst_mixed", "inst_tlas"]

# (device arrays, pinned blocks) a scene holds right after creation, above
# what its bottom-level scenes hold: nodes + triangles; + index array, vertex
# staging, edge word and the pinned read-back words; the samples (the bricked
# grid's staging array is gone when creation returns); child words + values;
# records + table; + matrices + top-level tree.
ALIVE = {"mesh": (2, 0), "dynmesh": (5, 1), "grid": (1, 0), "bricked": (1, 0), "octree": (2, 0),
         "inst": (2, 0), "inst_mixed": (2, 0), "inst_tlas": (4, 0)}

# rt_scene_device_bytes of each scene. The values are those of the library
# before the scene's fields were regrouped: this file's _build ran against
# that library (RTAMD_LIB=<its librtamd.so>) and printed them.
BYTES = {"mesh": 1184, "dynmesh": 1716, "grid": 48, "bricked": 512, "octree": 480,
         "inst": 304, "inst_mixed": 528, "inst_tlas": 704}


def live(rt):
    out = (C.c_int64 * 4)()
    rt._lib.check(rt.lib().rtx_live_resources(out))
    return tuple(out)


def _cube():
    _, (v, i), _ = S.inputs("cube.obj")
    assert len(i) == 36
    return np.array(v), np.array(i)


def _grid_values(size):
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, n) for n in size], indexing="ij")
    return (np.sqrt(x * x + y * y + z * z) - 0.6).astype(np.float32).ravel()


def _grid(rt, size, force):
    L = rt.lib()
    L.rtx_set_grid_force.argtypes = [C.c_int]
    rt._lib.check(L.rtx_set_grid_force(force))
    try:
        return rt.SDFGrid(size, _grid_values(size))
    finally:
        rt._lib.check(L.rtx_set_grid_force(0))


def _xforms(dx=0.0):
    return [[1, 0, 0, -0.8 + dx, 0, 1, 0, 0, 0, 0, 1, 0], [1, 0, 0, 0.8, 0, 1, 0, dx, 0, 0, 1, 0],
            [0.5, 0, 0, 0, 0, 0.5, 0, 0.9, 0, 0, 0.5, dx]]


def _build(rt, kind):
    """-> (scene, the bottom-level scenes it refers to)."""
    v, i = _cube()
    if kind in ("mesh", "dynmesh"):
        return rt.BVHBuilder(rt.SimpleMesh(v, i), dynamic=kind == "dynmesh"), []
    if kind == "grid":
        return _grid(rt, (3, 2, 2), 0), []
    if kind == "bricked":
        return _grid(rt, (5, 4, 3), 1), []
    if kind == "octree":
        return rt.SDFOctree(O.spine_tree(1, 0, "shuffled", 2, 0)[0]), []
    blas = [rt.BVHBuilder(rt.SimpleMesh(v, i)), rt.BVHBuilder(rt.SimpleMesh(v * np.float32([0.5, 0.5, 0.5, 1]), i))]
    if kind == "inst_mixed":
        blas.append(_grid(rt, (3, 2, 2), 0))
    inst = [(k if kind == "inst_mixed" else k % 2, x) for k, x in enumerate(_xforms())]
    return rt.InstancedScene(blas, inst, tlas=kind == "inst_tlas"), blas


def _params(rt, W, H):
    pos = (0.3, 0.4, 2.5)
    vi, pi = rt.camera_matrices(pos, aspect=W / H)
    return rt.render_params(pos, vi, pi, mode=rt.ShadingMode.Lambert)


def _host_frame(s, rt, size, **kw):
    W, H = size
    c, t = np.zeros((H, W), np.uint32), np.full((H, W), np.inf, np.float32)
    s.render(_params(rt, W, H), c, t, **kw)
    return c, t


def _device_frame(s, rt, size, times=1):
    W, H = size
    c = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    t = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    for _ in range(times):
        s.render_device(_params(rt, W, H), c.data_ptr(), t.data_ptr(), W, H, stream=st.cuda_stream)
    st.synchronize()
    return c.cpu().numpy().view(np.uint32), t.cpu().numpy()


def _rays(n):
    rng = np.random.default_rng(n)
    o = np.tile(np.float32([0.1, 0.2, 3.0]), (n, 1))
    d = np.float32([0, 0, -1]) + rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
    return o, np.ascontiguousarray(d, np.float32)


def _exercise(s, rt, kind):
    """Every lazily made part of a scene; -> the counters after the small and
    after the large rt_render frames (frame scenes), else None."""
    after = None
    if kind.startswith("inst"):
        o, d = (torch.from_numpy(a).cuda() for a in _rays(70))
        hit = torch.zeros(70, dtype=torch.int32, device="cuda")
        t = torch.zeros(70, dtype=torch.float32, device="cuda")
        s.trace_device(o.data_ptr(), d.data_ptr(), 70, hit_ptr=hit.data_ptr(), t_ptr=t.data_ptr())
        torch.cuda.synchronize()
        s.update_instances(np.float32(_xforms(0.1)))
    else:
        after = []
        for size in (SMALL, LARGE):  # the second regrows the frames and the row spans
            _host_frame(s, rt, size, clear=True)
            _host_frame(s, rt, size, cleared=True)
            after.append(live(rt))
        _host_frame(s, rt, LARGE)
        _device_frame(s, rt, LARGE, times=3)  # the schedule's buffers, side stream and events
        p = _params(rt, *LARGE)
        s.bench_frames([p, p], *LARGE)
        s.count_work([p], *LARGE)
    s.intersect(*_rays(5))
    return after


@pytest.mark.parametrize("kind", KINDS)
def test_scene_holds_what_it_says_and_returns_it(gpu, kind):
    rt = gpu
    base = live(rt)
    s, blas = _build(rt, kind)
    made = live(rt)
    held = sum(ALIVE["grid" if isinstance(b, rt.SDFGrid) else "mesh"][0] for b in blas)
    print(kind, "device_bytes", s.device_bytes(), "live", made, "base", base)
    assert (made[0] - base[0] - held, made[1] - base[1]) == ALIVE[kind]
    assert made[2:] == base[2:]  # events and streams come with the first frame
    assert s.device_bytes() == BYTES[kind]
    after = _exercise(s, rt, kind)
    if after:
        assert after[0] == after[1], "a regrow replaces what it grows"
        busy = live(rt)
        assert busy[0] > made[0] and busy[1] > made[1] and busy[2] > made[2] and busy[3] == made[3] + 3
    s.close()
    for b in blas:
        b.close()
    assert live(rt) == base


def test_failed_device_build_leaves_nothing(gpu):
    rt = gpu
    L = rt.lib()
    v, i = _cube()
    base = live(rt)
    h = C.c_void_p()
    rt._lib.check(L.rt_set_bvh_builder(RT_BVH_DEVICE))
    L.rtx_bvh_inject_failure(-1)
    try:
        rc = L.rt_scene_create_mesh(v.ctypes.data_as(C.c_void_p), len(v), i.ctypes.data_as(C.c_void_p), len(i),
                                    C.byref(h))
    finally:
        L.rtx_bvh_inject_failure(0)
        rt._lib.check(L.rt_set_bvh_builder(RT_BVH_AUTO))
    assert rc == RT_E_DEVICE
    assert live(rt) == base


def test_failed_render_leaves_the_scene_usable(gpu):
    rt = gpu
    L = rt.lib()
    L.rtx_render_inject_failure.argtypes = [C.c_int32]
    base = live(rt)
    s, _ = _build(rt, "mesh")
    fresh, _ = _build(rt, "mesh")
    L.rtx_render_inject_failure(1)
    try:
        with pytest.raises(rt.RtError):
            _host_frame(s, rt, LARGE, clear=True)
    finally:
        L.rtx_render_inject_failure(0)
    c, t = _host_frame(s, rt, LARGE, clear=True)
    fc, ft = _host_frame(fresh, rt, LARGE, clear=True)
    assert (c != 0).any()
    assert np.array_equal(c, fc) and np.array_equal(t.view(np.uint32), ft.view(np.uint32))
    s.close()
    fresh.close()
    assert live(rt) == base


def _replica(rt, s):
    out = C.c_void_p()
    rt._lib.check(rt.lib().rt_scene_replicate(s._handle(), 0, C.byref(out)))
    r = rt.IScene()
    r._h = out
    return r


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("kind", ["mesh", "dynmesh", "bricked", "octree"])
def test_replica(gpu, kind):
    rt = gpu
    base = live(rt)
    s, _ = _build(rt, kind)
    made = live(rt)
    r = _replica(rt, s)
    # the geometry only: a replica of a dynamic mesh is a plain snapshot
    geo = ALIVE["mesh" if kind == "dynmesh" else kind]
    assert tuple(x - y for x, y in zip(live(rt), made)) == (geo[0], 0, 0, 0)
    assert r.device_bytes() == BYTES["mesh" if kind == "dynmesh" else kind]
    before = _device_frame(s, rt, LARGE)
    assert (before[0] != 0).any()
    assert _same(_device_frame(r, rt, LARGE), before)
    if kind == "dynmesh":
        v, _ = _cube()
        assert s.device_bytes() - r.device_bytes() == 36 * 4 + len(v) * 16 + 4
        s.update_vertices(v * np.float32([0.5, 1.25, 0.75, 1]))
        moved = _device_frame(s, rt, LARGE)
        assert not _same(moved, before)
        r2 = _replica(rt, s)
        assert _same(_device_frame(r2, rt, LARGE), moved)
        assert _same(_device_frame(r, rt, LARGE), before)  # the earlier snapshot stays
        r2.close()
    r.close()
    s.close()
    assert live(rt) == base


def test_sdf_mesh_handles(gpu):
    rt = gpu
    v, i = _cube()
    base = live(rt)
    pts = np.random.default_rng(7).uniform(-1.5, 1.5, (70, 3)).astype(np.float32)
    ms = [rt.SDFMesh(rt.SimpleMesh(v, i)), rt.SDFMesh(rt.SimpleMesh(v, i), dynamic=True)]
    made = live(rt)
    # tree, triangles, pseudonormals; + 7 topology arrays, staging, 4 scratch arrays and the update's event
    assert tuple(x - y for x, y in zip(made, base)) == (3 + 3 + 12, 0, 1, 0)
    d = [m.points(pts) for m in ms]
    assert np.array_equal(d[0].view(np.uint32), d[1].view(np.uint32))
    # each query brought in its stream, its pinned staging block and two device arrays
    assert tuple(x - y for x, y in zip(live(rt), made)) == (4, 2, 0, 2)
    g = [m.grid(4)[1] for m in ms]
    assert np.array_equal(g[0].view(np.uint32), g[1].view(np.uint32))
    ms[1].update_vertices(v * np.float32([0.5, 0.5, 0.5, 1]))
    assert not np.array_equal(ms[1].points(pts), d[1])
    assert tuple(x - y for x, y in zip(live(rt), made)) == (4, 2, 0, 2)
    for m in ms:
        m.close()
    assert live(rt) == base
