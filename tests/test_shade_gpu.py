"""Shaded ray queries on the GPU: rt_eye_rays_device and rt_shade_rays_device
(include/rtamd.h; csrc/rt_shade_rays.hip, csrc/rt_shade_instances.hip).

Every comparison is on bits. For meshes, grids and octrees the strongest
reference is the frame kernel itself: the frame's eye rays, shaded, are
rt_render_device's frame. Arbitrary rays and instanced scenes are compared
with the shading oracle of tests/shade_common.py (shading_ref's float32
restatement above the oracle's geometry; for an instanced scene above the
header's loop composed from the oracle's meshes). Output buffers carry guard
words on both sides, as in tests/test_instances_gpu.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cpuref
import instances_common as IC
import rtamd
import scenes as S
import shade_common as SC
import shading_ref as SR
import tlas_common as TC
from rtamd import _lib, api, torch_rays
from test_instances_gpu import _blas

pytestmark = pytest.mark.gpu

GUARD = 64
RT_E_INVALID = -1
PLAIN = ["stanford-bunny.obj", "example_grid.grid", "sdf_5.octree"]
# name: (torch dtype, numpy dtype, sentinel bits)
KINDS = {"color": (torch.int32, np.int32, 0x5A5A5A5A), "t": (torch.float32, np.float32, 0x7FC12345),
         "hit": (torch.int32, np.int32, 0x5A5A5A5A), "prim": (torch.int64, np.int64, 0x5A5A5A5A5A5A5A5A)}
ALL = ("color", "t", "hit", "prim")
W0, H0 = SC.FRAMES[0][0]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _set_plane(gs, plane):
    gs.set_plane(rtamd.Plane(tuple(float(x) for x in plane[0]), float(plane[1])) if plane is not None else None)


def _params(W, H, shading, pos, module=rtamd):
    ln, mode, sh, rf = shading
    return SC.params(W, H, ln, mode, sh, rf, pos, module=module)


def _shade(gs, o_t, d_t, n, P, outputs=ALL, clear=True, tn=0.01, tf=100.0, tn_t=None, tf_t=None, stream=None):
    """One rt_shade_rays_device into sentinel-filled buffers with GUARD
    sentinel elements before and after the n the call may write. clear: every
    element of [0, n) is written. -> {name: numpy [n]} (color as uint32)."""
    buf = {}
    for k in outputs:
        dt, nt, sent = KINDS[k]
        buf[k] = torch.from_numpy(np.full(n + 2 * GUARD, sent, np.int64 if nt == np.int64 else np.int32).view(nt)).cuda()
        assert buf[k].dtype == dt
    ptr = lambda k: buf[k].data_ptr() + GUARD * buf[k].element_size() if k in buf else None
    gs.shade_device(o_t.data_ptr(), d_t.data_ptr(), n, P, ptr("color"), t_ptr=ptr("t"), hit_ptr=ptr("hit"),
                    prim_ptr=ptr("prim"), tnear=tn, tfar=tf, tnear_ptr=tn_t.data_ptr() if tn_t is not None else None,
                    tfar_ptr=tf_t.data_ptr() if tf_t is not None else None, clear=clear, stream=stream)
    torch.cuda.synchronize()
    out = {}
    for k in outputs:
        _, nt, sent = KINDS[k]
        bits = buf[k].cpu().numpy().view(np.int64 if nt == np.int64 else np.int32)
        assert (bits[:GUARD] == sent).all() and (bits[GUARD + n:] == sent).all(), f"{k}: guard elements were written"
        if clear or k in ("hit", "prim"):
            assert not (bits[GUARD:GUARD + n] == sent).any(), f"{k}: elements of [0, {n}) were not written"
        a = bits[GUARD:GUARD + n].view(nt)
        out[k] = a.view(np.uint32) if k == "color" else a
    return out


def _assert_oracle(ref, got, what, min_defined=None):
    """color where the oracle's channels are defined; t, hit and prim everywhere."""
    assert np.array_equal(ref.hit, got["hit"]), f"{what}: hit differs on {int((ref.hit != got['hit']).sum())} rays"
    assert np.array_equal(ref.prim, got["prim"]), f"{what}: prim differs on {int((ref.prim != got['prim']).sum())} rays"
    assert np.array_equal(_bits(ref.t), _bits(got["t"])), f"{what}: t differs on {int((_bits(ref.t) != _bits(got['t'])).sum())} rays"
    bad = (ref.color != got["color"]) & ref.ok
    assert not bad.any(), f"{what}: colour differs on {int(bad.sum())} rays"
    if min_defined is not None:
        left_out = int((~ref.ok).sum())
        print(f"{what}: {left_out} of {len(ref.ok)} rays left out as undefined")
        assert left_out <= (1.0 - min_defined) * len(ref.ok), f"{what}: {left_out} rays have an undefined channel"


def _same(a, b, what):
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs on {int((_bits(a[k]) != _bits(b[k])).sum())} rays"


@functools.lru_cache(maxsize=None)
def _eye(W, H, pos):
    o, d = SC.eye_rays(W, H, pos)
    return o, d, _dev(o), _dev(d)


@functools.lru_cache(maxsize=None)
def _random():
    o, d = IC.random_rays(SC.N_RANDOM, 20261019)
    rng = np.random.default_rng(19)
    cls = rng.integers(0, len(SC.CLASSES), SC.N_RANDOM)
    tn = np.float32([SC.CLASSES[c][0] for c in cls])
    tf = np.float32([SC.CLASSES[c][1] for c in cls])
    assert all((cls == c).sum() > 1000 for c in range(len(SC.CLASSES)))
    return o, d, tn, tf, _dev(o), _dev(d), _dev(tn), _dev(tf)


# ------------------------------------------------------------- 1. eye rays --
@pytest.mark.parametrize("W,H", [(97, 50), (64, 48), (1, 1)])
def test_eye_rays(gpu, W, H):
    """rt_eye_rays_device equals cpuref.primary_rays, the origins are
    camera_pos; an output left NULL is not written; guards stay."""
    pos = (0.6, 0.9, 3.2)
    P = _params(W, H, SC.SHADINGS[0], pos)
    want = np.ascontiguousarray(cpuref.primary_rays(_params(W, H, SC.SHADINGS[0], pos, module=cpuref), W, H), np.float32)
    n, sent = W * H, np.float32(-7.5)
    for which in ("both", "dir", "origin"):
        o = torch.full((3 * (n + 2 * GUARD),), float(sent), dtype=torch.float32, device="cuda")
        d = torch.full((3 * (n + 2 * GUARD),), float(sent), dtype=torch.float32, device="cuda")
        api.eye_rays_device(P, W, H, o.data_ptr() + 12 * GUARD if which != "dir" else None,
                            d.data_ptr() + 12 * GUARD if which != "origin" else None)
        torch.cuda.synchronize()
        oh, dh = o.cpu().numpy().reshape(-1, 3), d.cpu().numpy().reshape(-1, 3)
        for a in (oh, dh):
            assert (a[:GUARD] == sent).all() and (a[GUARD + n:] == sent).all(), "guard elements were written"
        if which != "origin":
            assert np.array_equal(_bits(dh[GUARD:GUARD + n]), _bits(want.reshape(-1, 3))), f"{which}: directions differ"
        else:
            assert (dh == sent).all(), "a NULL d_dir was written"
        if which != "dir":
            assert np.array_equal(oh[GUARD:GUARD + n], np.tile(np.float32(pos), (n, 1))), f"{which}: origins differ"
        else:
            assert (oh == sent).all(), "a NULL d_origin was written"
    ot, dt = torch_rays.eye_rays(P, W, H)
    torch.cuda.synchronize()
    assert ot.shape == (n, 3) and np.array_equal(_bits(dt.cpu().numpy()), _bits(want.reshape(-1, 3)))
    assert np.array_equal(ot.cpu().numpy(), np.tile(np.float32(pos), (n, 1)))


# ---------------------------------- 2. plain kinds equal the frame kernels --
@pytest.mark.parametrize("plane", ["off", "base", "xdom"])
@pytest.mark.parametrize("key", PLAIN)
def test_plain_kinds_equal_the_frame_kernels(gpu, key, plane):
    """The frame's eye rays, shaded with RT_SHADE_CLEAR over [0.01, 100]:
    colour and t are bitwise rt_render_device(RT_FLAG_CLEAR)'s, d_hit is
    t < inf. Lambert with the four switch settings under two lights, Color,
    Normal."""
    W, H = W0, H0
    gs = S.gpu_scene(key)
    _set_plane(gs, None if plane == "off" else SR.plane_for(key, plane))
    hits = 0
    for shading in SC.SHADINGS:
        P = _params(W, H, shading, SR.CAMERA)
        o_t, d_t = torch_rays.eye_rays(P, W, H)
        c = torch.full((H, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        t = torch.full((H, W), -5.0, dtype=torch.float32, device="cuda")
        gs.render_device(P, c.data_ptr(), t.data_ptr(), W, H, clear=True)
        got = _shade(gs, o_t, d_t, W * H, P)
        fc, ft = c.cpu().numpy().view(np.uint32).reshape(-1), t.cpu().numpy().reshape(-1)
        what = f"{key} plane {plane} {shading}"
        assert np.array_equal(fc, got["color"]), f"{what}: colour differs on {int((fc != got['color']).sum())} pixels"
        assert np.array_equal(_bits(ft), _bits(got["t"])), f"{what}: t differs on {int((_bits(ft) != _bits(got['t'])).sum())} pixels"
        assert np.array_equal(got["hit"], (ft < np.inf).astype(np.int32)), f"{what}: d_hit is not t < inf"
        hits += int(got["hit"].sum())
    assert hits > 10 * 150, "the frames are hardly hit"


# ------------------------------------------------------------------ 3. tPrev --
def test_tprev_composition_equals_the_frame_kernel(gpu):
    """A frame that already holds something: shading without RT_SHADE_CLEAR,
    d_tfar aliasing d_t, leaves both buffers bitwise as rt_render_device with
    flags = 0 leaves them, the untouched pixels included. From (0.6, 0.4, 2.1)
    the oracle stores 523 of the bunny's 813 pixels under these t and no pixel
    of the plane: tPrev hides part of the model."""
    W, H = W0, H0
    gs = S.gpu_scene("stanford-bunny.obj")
    _set_plane(gs, SR.PLANES["base"])
    P = _params(W, H, ("std", SR.LAMBERT, True, True), (0.6, 0.4, 2.1))
    c0 = np.full((H, W), 0x11223344, np.int32)
    t0 = np.broadcast_to((2.0 + 0.01 * (np.arange(W) % 7)).astype(np.float32), (H, W)).copy()
    assert t0.max() < 100.0
    fc, ft = _dev(c0), _dev(t0)
    gs.render_device(P, fc.data_ptr(), ft.data_ptr(), W, H, clear=False)
    sc, st = _dev(c0.reshape(-1)), _dev(t0.reshape(-1))
    o_t, d_t = torch_rays.eye_rays(P, W, H)
    r = torch_rays.shade(gs, o_t, d_t, P, tfar=st, clear=False, color=sc, t=st, outputs=("color", "t", "hit"))
    torch.cuda.synchronize()
    assert r.color is sc and r.t is st
    fc, ft = fc.cpu().numpy().reshape(-1), ft.cpu().numpy().reshape(-1)
    assert np.array_equal(fc, sc.cpu().numpy()) and np.array_equal(_bits(ft), _bits(st.cpu().numpy()))
    kept = fc == 0x11223344
    assert 200 < int(kept.sum()) < W * H - 200, "the frame must change some pixels and keep others"
    assert np.array_equal(r.hit.cpu().numpy(), (~kept).astype(np.int32))
    assert np.array_equal(_bits(ft[kept]), _bits(t0.reshape(-1)[kept]))


# ------------------------------------- 4. arbitrary rays against the oracle --
@pytest.mark.parametrize("per_ray", [False, True])
@pytest.mark.parametrize("key", PLAIN)
def test_random_rays_against_the_oracle(gpu, key, per_ray):
    """4096 random rays under the base plane, Lambert with shadows and
    reflections: scalar [0.01, 100], and per-ray d_tnear / d_tfar over three
    classes."""
    o, d, tn, tf, o_t, d_t, tn_t, tf_t = _random()
    gs = S.gpu_scene(key)
    plane = SR.plane_for(key, "base")
    _set_plane(gs, plane)
    P = _params(W0, H0, ("std", SR.LAMBERT, True, True), SR.CAMERA)
    if per_ray:
        ref = SC.shade(SR.base_scene(key), plane, o, d, tn, tf, "std", SR.LAMBERT, True, True)
        got = _shade(gs, o_t, d_t, SC.N_RANDOM, P, tn_t=tn_t, tf_t=tf_t)
    else:
        ref = SC.shade(SR.base_scene(key), plane, o, d, 0.01, 100.0, "std", SR.LAMBERT, True, True)
        got = _shade(gs, o_t, d_t, SC.N_RANDOM, P)
    _assert_oracle(ref, got, f"{key} per_ray={per_ray}", min_defined=0.99)
    assert int((ref.prim >= 0).sum()) > 200 and int((ref.prim == -2).sum()) > 200


# ------------------------------------------------ 5. instanced, flat and tree --
def _build5(tlas):
    names, inst = SC.SCENE5
    return rtamd.InstancedScene([_blas(m) for m in names], inst, tlas=tlas)


@functools.lru_cache(maxsize=None)
def _scene5(tlas):
    return _build5(tlas)


@pytest.mark.parametrize("plane", [True, False])
@pytest.mark.parametrize("frame", [0, 1])
def test_instanced_frames_against_the_composed_oracle(gpu, frame, plane):
    """SCENE5 with M (and the leaf boxes) read back from the device: colour,
    t, hit and prim are bitwise the oracle's in both modes, and the flat
    scene's outputs are bitwise the tree scene's."""
    (W, H), pos = SC.FRAMES[frame]
    o, d, o_t, d_t = _eye(W, H, pos)
    flat, tree = _scene5(False), _scene5(True)
    pl = SC.PLANE if plane else None
    for gs in (flat, tree):
        _set_plane(gs, pl)
    of, ot = SC.device_oracle(flat, SC.SCENE5[0]), SC.device_oracle(tree, SC.SCENE5[0])
    assert of.wbox is None and ot.wbox is not None
    insts = set()
    for shading in SC.SHADINGS:
        P = _params(W, H, shading, pos)
        gf, gt = _shade(flat, o_t, d_t, W * H, P), _shade(tree, o_t, d_t, W * H, P)
        what = f"SCENE5 {W}x{H} plane={plane} {shading}"
        rf = SC.shade(of, pl, o, d, 0.01, 100.0, *shading)
        rt_ = SC.shade(ot, pl, o, d, 0.01, 100.0, *shading)
        _assert_oracle(rf, gf, what + " flat")
        _assert_oracle(rt_, gt, what + " tree")
        _same(gf, gt, what + " flat vs tree")
        insts |= set((gf["prim"][gf["prim"] >= 0] >> 32).tolist())
    assert insts == {0, 1, 2, 3}, "every enabled instance is seen, the disabled one never"


def test_instanced_random_rays_with_per_ray_intervals(gpu):
    o, d, tn, tf, o_t, d_t, tn_t, tf_t = _random()
    P = _params(W0, H0, ("std", SR.LAMBERT, True, True), SR.CAMERA)
    got = []
    for tlas in (False, True):
        gs = _scene5(tlas)
        _set_plane(gs, SC.PLANE)
        ref = SC.shade(SC.device_oracle(gs, SC.SCENE5[0]), SC.PLANE, o, d, tn, tf, "std", SR.LAMBERT, True, True)
        got.append(_shade(gs, o_t, d_t, SC.N_RANDOM, P, tn_t=tn_t, tf_t=tf_t))
        _assert_oracle(ref, got[-1], f"SCENE5 random rays tlas={tlas}", min_defined=0.99)
        assert int((ref.prim >= 0).sum()) > 200
    _same(got[0], got[1], "random rays, flat vs tree")


# --------------------------------------------------------- 6. many instances --
def test_many_instances(gpu):
    """130 instances alternating over two BLAS under the base plane, coherent
    eye rays: tree equals flat equals the oracle (the tree's: the flat
    composition differs from it in no ray, tests/test_tlas_host.py)."""
    names, inst = TC.scene130()
    o, d = TC.eye_rays(64, 64)
    o_t, d_t = _dev(o), _dev(d)
    P = _params(64, 64, ("std", SR.LAMBERT, True, True), (0.3, 0.4, 6.0))
    out = []
    for tlas in (True, False):
        gs = rtamd.InstancedScene([_blas(m) for m in names], inst, tlas=tlas)
        _set_plane(gs, SC.PLANE)
        out.append(_shade(gs, o_t, d_t, len(o), P))
        if tlas:
            ref = SC.shade(SC.device_oracle(gs, names), SC.PLANE, o, d, 0.01, 100.0, "std", SR.LAMBERT, True, True)
        gs.close()
    _assert_oracle(ref, out[0], "scene130 tree")
    _same(out[0], out[1], "scene130 tree vs flat")
    won = np.unique(out[0]["prim"][out[0]["prim"] >= 0] >> 32)
    assert len(won) > 30 and (won % 2 == 0).any() and (won % 2 == 1).any()


# ----------------------------------------------------------- 7. stream order --
@pytest.mark.parametrize("tlas", [False, True])
def test_stream_order_poses(gpu, tlas):
    """update_instances (device poses), eye_rays and shade on one non-default
    stream with no synchronisation between them: the oracle of the new poses."""
    (W, H), pos = SC.FRAMES[1]
    gs = _build5(tlas)
    _set_plane(gs, SC.PLANE)
    names, inst = SC.SCENE5
    p1 = np.stack([t[1] for t in inst]).copy()
    p1[:, :, 3] += np.float32([0.15, 0.1, -0.2])
    P = _params(W, H, ("std", SR.LAMBERT, True, True), pos)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        x = _dev(p1) * 1.0  # produced by a torch kernel on this stream
        torch_rays.update_instances(gs, x)
        o_t, d_t = torch_rays.eye_rays(P, W, H)
        r = torch_rays.shade(gs, o_t, d_t, P, outputs=ALL)
    st.synchronize()
    o, d = SC.eye_rays(W, H, pos)
    ref = SC.shade(SC.device_oracle(gs, names), SC.PLANE, o, d, 0.01, 100.0, "std", SR.LAMBERT, True, True)
    old = SC.shade(SC.device_oracle(_scene5(tlas), names), SC.PLANE, o, d, 0.01, 100.0, "std", SR.LAMBERT, True, True)
    assert int((ref.color != old.color).sum()) > 200, "the new poses must change the picture"
    got = {k: getattr(r, k).cpu().numpy() for k in ALL}
    got["color"] = got["color"].view(np.uint32)
    _assert_oracle(ref, got, f"poses from the device, tlas={tlas}")
    gs.close()


def test_stream_order_dynamic_blas(gpu):
    """update_vertices of a dynamic BLAS, then shade, in both modes: the stale
    table entry (and the tree's boxes) are rewritten in stream order ahead of
    the launch. An exact translation of the lattice mesh, whose refitted tree
    is the tree of a fresh build (tests/test_refit_gpu.py)."""
    import refit_common as R
    v, i = IC.mesh("grid")
    bl = rtamd.BVHBuilder(rtamd.SimpleMesh(v, i), dynamic=True)
    pose = lambda seed, scale, b: IC.affine(IC.rot(seed) @ np.diag(np.float64(scale)), b)

    def placed(seed, scale, b):  # puts the TRANSLATED mesh where pose(seed, scale, b) puts the original: into view
        x = pose(seed, scale, b).astype(np.float64)
        x[:, 3] -= x[:, :3] @ R.SHIFT.astype(np.float64)
        return x.astype(np.float32)

    inst = [(0, placed(70, (0.2, 0.2, 0.2), (-1.2, -0.9, -0.6)), 0), (1, pose(71, (0.6, 0.6, 0.6), (0.5, -0.3, 0.0)), 0)]
    objs = [bl, _blas("cube")]
    scenes = [rtamd.InstancedScene(objs, inst, tlas=tlas) for tlas in (False, True)]
    (W, H), pos = SC.FRAMES[1]
    o, d, o_t, d_t = _eye(W, H, pos)
    P = _params(W, H, ("std", SR.LAMBERT, True, True), pos)
    for gs in scenes:
        _set_plane(gs, SC.PLANE)
    before = [_shade(gs, o_t, d_t, W * H, P) for gs in scenes]
    w = R.translate(v)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        torch_rays.update_vertices(bl, _dev(w))
        res = [torch_rays.shade(gs, o_t, d_t, P, outputs=ALL) for gs in scenes]
    st.synchronize()
    refs = [cpuref.RefScene.mesh(w, i), IC.ref_mesh("cube")]
    for gs, r, b in zip(scenes, res, before):
        ref = SC.shade(SC.device_oracle(gs, refs), SC.PLANE, o, d, 0.01, 100.0, "std", SR.LAMBERT, True, True)
        got = {k: getattr(r, k).cpu().numpy() for k in ALL}
        got["color"] = got["color"].view(np.uint32)
        _assert_oracle(ref, got, f"after the refit, tlas={gs.has_tlas}")
        assert int((got["color"] != b["color"]).sum()) > 50, "the moved mesh must change the picture"
        assert int(((got["prim"] >= 0) & (got["prim"] >> 32 == 0)).sum()) > 50
    for sc in scenes + [bl]:
        sc.close()


# ------------------------------------------------------- 8. stores and sizes --
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4850])
def test_stores_and_sizes(gpu, n):
    """Guards on both sides stay intact; without RT_SHADE_CLEAR a ray that
    misses keeps the sentinel in colour and t, with it every ray is written;
    outputs left NULL are not needed."""
    (W, H), pos = SC.FRAMES[0]
    _, _, o_t, d_t = _eye(W, H, pos)
    P = _params(W, H, ("std", SR.LAMBERT, True, True), pos)
    for gs in (_scene5(False), _scene5(True), S.gpu_scene("stanford-bunny.obj")):
        _set_plane(gs, None)  # no plane: most eye rays miss
        full = _shade(gs, o_t, d_t, n, P)
        kept = _shade(gs, o_t, d_t, n, P, clear=False)
        miss = full["hit"] == 0
        if n == 4850:
            assert 100 < int(miss.sum()) < n - 100
        assert (kept["color"][miss] == 0x5A5A5A5A).all() and (_bits(kept["t"])[miss] == 0x7FC12345).all()
        assert (full["color"][miss] == 0).all() and np.isposinf(full["t"][miss]).all()
        for k in ALL:
            assert np.array_equal(_bits(kept[k])[~miss], _bits(full[k])[~miss])
        assert np.array_equal(kept["hit"], full["hit"]) and np.array_equal(kept["prim"], full["prim"])
        only = _shade(gs, o_t, d_t, n, P, outputs=("color",))
        assert np.array_equal(only["color"], full["color"])
        _same(_shade(gs, o_t, d_t, n, P, outputs=("color", "prim")), {"color": full["color"], "prim": full["prim"]}, "subset")


def test_zero_rays(gpu):
    gs = _scene5(True)
    P = _params(W0, H0, SC.SHADINGS[0], SR.CAMERA)
    c = torch.full((GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    gs.shade_device(c.data_ptr(), c.data_ptr(), 0, P, c.data_ptr(), t_ptr=c.data_ptr(), hit_ptr=c.data_ptr())
    torch.cuda.synchronize()
    assert (c.cpu().numpy() == 0x5A5A5A5A).all()
    z = torch.empty((0, 3), dtype=torch.float32, device="cuda")
    r = torch_rays.shade(gs, z, z, P)
    assert r.color.shape == (0,) and r.t.shape == (0,)


# ------------------------------------------------------------- 9. refusals --
def test_refusals_write_nothing(gpu):
    """Each invalid call returns RT_E_INVALID with a message and launches
    nothing; all four scene kinds are accepted."""
    L = rtamd.lib()
    (W, H), pos = SC.FRAMES[1]
    _, _, o_t, d_t = _eye(W, H, pos)
    n = 256
    bufs = {k: torch.from_numpy(np.full(n, KINDS[k][2], np.int64 if k == "prim" else np.int32).view(KINDS[k][1])).cuda()
            for k in ALL}
    nrm = torch.full((3 * n,), -7.5, dtype=torch.float32, device="cuda")
    good = lambda: _lib.RayBatch(n, o_t.data_ptr(), d_t.data_ptr(), None, None, 0.01, 100.0, bufs["hit"].data_ptr(),
                                 bufs["t"].data_ptr(), None, bufs["prim"].data_ptr())
    P = _params(W, H, ("std", SR.LAMBERT, True, True), pos)
    gs = _scene5(False)
    h = gs._handle()
    color = C.c_void_p(bufs["color"].data_ptr())

    def refused(b, p=P, c=color, flags=_lib.RT_SHADE_CLEAR, scene=h, word=None):
        rc = L.rt_shade_rays_device(scene, C.byref(b) if b is not None else None, C.byref(p) if p is not None else None,
                                    c, flags, None)
        msg = L.rt_last_error()
        assert rc == RT_E_INVALID and msg, (rc, msg)
        if word:
            assert word in msg, msg

    refused(good(), scene=None, word=b"scene")
    refused(None, word=b"batch")
    refused(good(), p=None, word=b"params")
    refused(good(), c=None, word=b"colour")
    b = good(); b.d_origin = None
    refused(b, word=b"origins")
    b = good(); b.d_dir = None
    refused(b, word=b"directions")
    b = good(); b.d_normal = nrm.data_ptr()
    refused(b, word=b"d_normal")
    b = good(); b.n = -1
    refused(b, word=b"negative")
    b = good(); b.n = 2 ** 32
    refused(b, word=b"exceeds one launch")
    refused(good(), flags=2, word=b"flag")
    refused(good(), flags=_lib.RT_SHADE_CLEAR | 4, word=b"flag")
    for mode in (-1, 3):
        p = _params(W, H, ("std", SR.LAMBERT, True, True), pos)
        p.shading_mode = mode
        refused(good(), p=p, word=b"shading mode")
    p = _params(W, H, ("std", SR.LAMBERT, True, True), pos)
    p.reserved = 1
    refused(good(), p=p, word=b"reserved")
    torch.cuda.synchronize()
    for k in ALL:
        bits = bufs[k].cpu().numpy().view(np.int64 if k == "prim" else np.int32)
        assert (bits == KINDS[k][2]).all(), f"a refused call wrote {k}"
    assert (nrm.cpu().numpy() == -7.5).all()
    # every kind is accepted
    for sc in (gs, _scene5(True), S.gpu_scene("stanford-bunny.obj"), S.gpu_scene("example_grid.grid"),
               S.gpu_scene("sdf_5.octree")):
        assert L.rt_shade_rays_device(sc._handle(), C.byref(good()), C.byref(P), color, _lib.RT_SHADE_CLEAR, None) == 0
    torch.cuda.synchronize()
    assert not (bufs["color"].cpu().numpy() == 0x5A5A5A5A).any()
