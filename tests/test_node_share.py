"""The shared node fetch of the primary mesh path (RT_NODE_SHARE, mesh_run in
csrc/rt_scenes.h): an expansion whose lanes are all at one node, at least 14
of them, loads the node once for the wave and hands it round through LDS; any
other expansion loads per lane. Colour and t of every case are compared
bitwise with the oracle through the three paths that take it -- the one-frame
kernel, render_device_frames with 3 frames (the persistent queue) and
rt_trace_rays_device on the same eye rays (there: hit, t, normal and primitive
against the oracle's ray query, and t against the frame) -- and the counting
kernel's wave-level counters (count_share) say which form ran.

The cameras were fixed after running them through the CPU model
(tools/trav_sim.cpp --share, wave-level expansions shared / all):

  8 scene radii, 64x64 and 128x72   cube 0 / 0 (its tree is a root over two
      leaves), spot 0 / 39 and 0 / 56, bunny 0 / 67 and 0 / 99. The model sits
      in a few tiles whose rays fan out over the whole tree, so no expansion
      there is shared: at this distance the cases pin the per-lane form beside
      a pad that is never written. Sharing grows with the pixels per node, not
      with the distance (bunny 1920x1080: 39 %).
  bunny 128x72, orbit distance       22 / 422, 17 tiles run both forms
  bunny 128x72, 0.3 radii            473 / 1609, 144 tiles run both forms
  bunny 128x72, (0, 0, 0.55)         385 / 1483: the largest share found at
      this size
  bunny 67x35                        2 / 133 (the two come from whole tiles)
  bunny 5x2                          0 / 6: one tile of 10 rays
"""
import functools

import numpy as np
import pytest

import cpuref
import rtamd
import scenes as S

pytestmark = pytest.mark.gpu

BUNNY, SPOT, CUBE = "stanford-bunny.obj", "spot.obj", "cube.obj"
ORBIT = (0.0, 0.0, 2.5)


def _radius(name):
    v, _ = S.inputs(name)[1]
    return float(np.linalg.norm(v[:, :3] / v[:, 3:4], axis=1).max())


def _at(name, radii, direction=(0.3, 0.2, 1.0)):
    d = np.asarray(direction, np.float64)
    return tuple(float(x) for x in d / np.linalg.norm(d) * radii * _radius(name))


# id: (mesh, W, H, camera)
CASES = {}
for _m in (CUBE, SPOT, BUNNY):
    for _w, _h in ((64, 64), (128, 72)):
        CASES[f"far-{_m.split('.')[0]}-{_w}x{_h}"] = (_m, _w, _h, ("radii", 8.0))
CASES.update({
    "mixed-orbit": (BUNNY, 128, 72, ORBIT),
    "mixed-closeup": (BUNNY, 128, 72, ("radii", 0.3)),
    "mixed-most-shared": (BUNNY, 128, 72, (0.0, 0.0, 0.55)),
    "few-lanes-67x35": (BUNNY, 67, 35, ORBIT),
    "few-lanes-5x2": (BUNNY, 5, 2, ORBIT),
    # the eye at the height of the model's top, from the side: the tiles along
    # the upper silhouette keep a handful of live rays
    "few-lanes-grazing": (BUNNY, 128, 72, (2.5, 0.6167, 0.0)),
    # odd W and H from an axis: d.x is exactly 0 in column 32 and d.y in row 16,
    # so those rays take the exact-slab instantiation (1/d infinite), which
    # shares the load phase
    "axis-65x33": (BUNNY, 65, 33, ORBIT),
    "one-triangle": ("tri", 64, 64, ORBIT),
})
PATHS = ("one_frame", "three_frames", "rays")


def _pos(case):
    mesh, _, _, cam = CASES[case]
    return _at(mesh, cam[1]) if cam[0] == "radii" else cam


@functools.lru_cache(maxsize=None)
def _scenes(mesh):
    if mesh == "tri":
        v = np.array([[-0.6, -0.5, 0.1, 1], [0.7, -0.4, -0.2, 1], [0.0, 0.6, 0.0, 1]], np.float32)
        i = np.arange(3, dtype=np.uint32)
        return cpuref.RefScene.mesh(v, i), rtamd.BVHBuilder(rtamd.SimpleMesh(v, i))
    return S.ref_scene(mesh), S.gpu_scene(mesh)


def _params(case, module):
    _, W, H, _ = CASES[case]
    return S.params(None, W, H, "primary", _pos(case), module)


@functools.lru_cache(maxsize=None)
def _oracle(case):
    """The oracle's frame and its eye rays' query results, once per case."""
    mesh, W, H, _ = CASES[case]
    rs, _ = _scenes(mesh)
    rs.set_plane(False, (0, 1, 0), 0.0)
    P = _params(case, "ref")
    c, t, _, _ = rs.render(P, W, H)
    d = np.ascontiguousarray(cpuref.primary_rays(P, W, H).reshape(-1, 3))
    o = np.tile(np.float32(_pos(case)), (len(d), 1))
    q = rs.intersect_rays(o, d, 0.01, 100.0)
    for a in (c, t, o, d) + tuple(q):
        a.setflags(write=False)
    return c, t, o, d, q


def _gpu(case):
    gs = _scenes(CASES[case][0])[1]
    gs.set_plane(None)
    return gs


def _same(case, path, c, t):
    rc, rt_ = _oracle(case)[:2]
    what = f"{case} {path}"
    assert np.array_equal(np.isfinite(rt_), np.isfinite(t)), f"{what}: coverage differs"
    assert int((rc != c).sum()) == 0, f"{what}: colour differs"
    assert int((rt_.view(np.uint32) != t.view(np.uint32)).sum()) == 0, f"{what}: t differs bitwise"


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", list(CASES))
def test_bitwise_against_the_oracle(gpu, case, path):
    import torch
    _, W, H, _ = CASES[case]
    gs = _gpu(case)
    P = _params(case, "gpu")
    if path == "one_frame":
        c = np.zeros((H, W), np.uint32)
        t = np.full((H, W), np.inf, np.float32)
        gs.render(P, c, t, clear=True)
        _same(case, path, c, t)
    elif path == "three_frames":
        cs = [torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in range(3)]
        ts = [torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(3)]
        gs.render_device_frames([P] * 3, [c.data_ptr() for c in cs], [t.data_ptr() for t in ts], W, H,
                                rtamd.RT_FLAG_CLEAR, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for c, t in zip(cs, ts):
            _same(case, path, c.cpu().numpy().view(np.uint32), t.cpu().numpy())
    else:
        _, rt_, o, d, (qh, qt, qn, qp) = _oracle(case)
        n = W * H
        o_t, d_t = torch.from_numpy(o.copy()).cuda(), torch.from_numpy(d.copy()).cuda()
        hit = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        t = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
        nrm = torch.full((n, 3), -9.0, dtype=torch.float32, device="cuda")
        prim = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        gs.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=hit.data_ptr(), t_ptr=t.data_ptr(),
                        normal_ptr=nrm.data_ptr(), prim_ptr=prim.data_ptr(), tnear=0.01, tfar=100.0)
        torch.cuda.synchronize()
        h = qh.astype(bool)
        assert np.array_equal(qh, hit.cpu().numpy()), f"{case} rays: hit mask differs"
        assert np.array_equal(qp, prim.cpu().numpy()), f"{case} rays: primitive ids differ"
        gt = t.cpu().numpy()
        assert np.array_equal(qt[h].view(np.uint32), gt[h].view(np.uint32)), f"{case} rays: t differs"
        assert np.array_equal(qn[h].view(np.uint32), nrm.cpu().numpy()[h].view(np.uint32)), f"{case} rays: normal differs"
        # and the frame's own t where it stored a hit
        fh = np.isfinite(rt_).ravel()
        assert np.array_equal(rt_.ravel()[fh].view(np.uint32), gt[fh].view(np.uint32)), f"{case} rays: t differs from the frame's"


def _counts(case):
    _, W, H, _ = CASES[case]
    gs = _gpu(case)
    P = _params(case, "gpu")
    cs = gs.count_share([P], W, H)
    cw = gs.count_work([P], W, H)
    print(f"{case}: {cs} bvh_inner {cw['bvh_inner']} rays {cw['rays']}")
    assert 0 <= cs["bvh_shared"] <= cs["bvh_wave_expansions"]
    # every ray counts the root; what is left are lane-level expansions, at
    # most 64 and at least one per wave-level expansion
    below = cw["bvh_inner"] - cw["rays"]
    assert cs["bvh_wave_expansions"] <= below <= 64 * cs["bvh_wave_expansions"]
    # the counting kernel takes the wave path now: its work counters are still the oracle's
    rs = _scenes(CASES[case][0])[0]
    rs.set_plane(False, (0, 1, 0), 0.0)
    cpuref.counters(True)
    rs.render(_params(case, "ref"), W, H)
    ref = cpuref.counters(True)
    keys = ("bvh_inner", "bvh_leaf", "bvh_tri")
    assert {k: cw[k] for k in keys} == {k: ref[k] for k in keys}
    return cs["bvh_shared"], cs["bvh_wave_expansions"]


@pytest.mark.parametrize("case", [c for c in CASES if c.startswith("far-")])
def test_far_camera_counts(gpu, case):
    """8 radii: the model's expansions all run, and none of them can be shared
    (see the module docstring: the CPU model finds no shared expansion here)."""
    shared, waves = _counts(case)
    if CASES[case][0] == CUBE:
        assert waves == 0
    else:
        assert waves > 0
        assert shared < waves


@pytest.mark.parametrize("case", ["mixed-orbit", "mixed-closeup", "mixed-most-shared"])
def test_both_forms_run(gpu, case):
    shared, waves = _counts(case)
    assert shared > 0, "the shared fetch never ran"
    assert waves - shared > 0, "the per-lane form never ran"


@pytest.mark.parametrize("case", ["few-lanes-67x35", "few-lanes-5x2", "few-lanes-grazing", "axis-65x33"])
def test_few_lanes_load_per_lane(gpu, case):
    shared, waves = _counts(case)
    assert waves - shared > 0, "no per-lane expansion"
    if case == "few-lanes-5x2":
        assert shared == 0, "10 rays are fewer than the shared fetch's 14 lanes"


def test_axis_case_has_non_finite_reciprocals(gpu):
    d = _oracle("axis-65x33")[3].reshape(33, 65, 3)
    assert (d[:, 32, 0] == 0).all() and (d[16, :, 1] == 0).all()
    assert np.isfinite(_oracle("axis-65x33")[1][:, 32]).any(), "no hit in the column of exact rays"


def test_root_leaf_counts(gpu):
    cs = _gpu("one-triangle").count_share([_params("one-triangle", "gpu")], 64, 64)
    assert cs == {"bvh_shared": 0, "bvh_wave_expansions": 0}
    assert np.isfinite(_oracle("one-triangle")[1]).sum() > 100
