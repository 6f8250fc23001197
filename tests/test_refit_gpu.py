"""rt_scene_update_vertices / rt_scene_update_vertices_device: the BVH8 refit
on the GPU (csrc/rt_refit.hip) and everything that depends on the refitted
scene: the host constants, frames, ray queries, rt_multi's replicas, torch.

Bars: the device tree after an update is bitwise the host restatement's
(rtx_bvh_refit_host, itself pinned by test_refit_host.py); an exactly
translated mesh is bitwise a fresh build of the translated mesh, tree,
constants, frame and rays; a generally deformed bunny answers every ray exactly
as a fresh build of the deformed mesh does. No tolerance anywhere.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cpuref
import refit_common as R
import scenes as S

pytestmark = pytest.mark.gpu

RT_E_INVALID, RT_E_STATE = -1, -4
RT_BVH_AUTO, RT_BVH_HOST, RT_BVH_DEVICE = 0, 1, 2


def _scene(rt, v, i, dynamic=True):
    return rt.BVHBuilder(rt.SimpleMesh(np.array(v), np.array(i)), dynamic=dynamic)


def _download(rt, s):
    from rtamd._lib import check
    L = rt.lib()
    ni, nt = C.c_int64(0), C.c_int64(0)
    check(L.rtx_scene_mesh_download(s._handle(), None, C.byref(ni), None, C.byref(nt)))
    nodes = np.zeros((ni.value, 56), np.uint32)
    tris = np.zeros((nt.value, 12), np.uint32)
    check(L.rtx_scene_mesh_download(s._handle(), R._p(nodes), C.byref(ni), R._p(tris), C.byref(nt)))
    return nodes, tris


def _constants(rt, s):
    """(root_box[6], root_child[48], dmax2) as uint32 bits."""
    from rtamd._lib import check
    rb, rc, d = np.zeros(6, np.float32), np.zeros(48, np.float32), C.c_float(0)
    check(rt.lib().rtx_scene_mesh_constants(s._handle(), R._p(rb), R._p(rc), C.byref(d)))
    return rb.view(np.uint32), rc.view(np.uint32), np.float32(d.value).view(np.uint32)


def _same_tree(a, b, what):
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape, what
    assert np.array_equal(a[1], b[1]), f"{what}: {(a[1] != b[1]).any(1).sum()} triangles differ"
    assert np.array_equal(a[0], b[0]), f"{what}: {(a[0] != b[0]).any(1).sum()} nodes differ"


def _update(s, w, entry):
    if entry == "host":
        s.update_vertices(w)
        return
    w_t = torch.from_numpy(np.ascontiguousarray(w)).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()  # a non-default stream
    s.update_vertices_device(w_t.data_ptr(), len(w), stream=st.cuda_stream)


MESHES = [("rand", 1), ("signed0", 9), ("grid", 100), ("rand", 1500)]
CASES = [(m, n, b, e) for m, n in MESHES for b in (RT_BVH_HOST, RT_BVH_DEVICE) for e in ("host", "device")]
CASES.append(("bunny", 0, RT_BVH_AUTO, "device"))


@pytest.mark.parametrize("mode,ntri,builder,entry", CASES)
def test_device_refit_is_the_host_restatement(gpu, mode, ntri, builder, entry):
    rt = gpu
    v, i = R.bunny() if mode == "bunny" else R.edge(mode, ntri)
    w = R.deform(v)
    L = rt.lib()
    assert L.rt_set_bvh_builder(builder) == 0
    try:
        s = _scene(rt, v, i)
    finally:
        L.rt_set_bvh_builder(RT_BVH_AUTO)
    with s:
        built = R.host_refit(rt, v, i)
        _same_tree(_download(rt, s), built, "as created")
        _update(s, w, entry)
        _same_tree(_download(rt, s), R.host_refit(rt, v, i, w), "after the update")
        _update(s, np.array(v), entry)  # and back: the identity result
        back = _download(rt, s)
        _same_tree(back, R.host_refit(rt, v, i, v), "back at the creation vertices")
        assert np.array_equal(R.boxes(back[0]), R.boxes(built[0]))  # the built tree, by value


def test_dynamic_bytes_and_plain_creation_unchanged(gpu):
    """flags = 0 is rt_scene_create_mesh, device bytes included; RT_MESH_DYNAMIC
    adds the index array, the staging buffer and the 4-byte edge-bound word."""
    rt = gpu
    v, i = R.edge("rand", 1500)
    with _scene(rt, v, i, dynamic=False) as a, _scene(rt, v, i) as b:
        h = C.c_void_p()
        from rtamd._lib import check
        va, ia = np.array(v), np.array(i)
        check(rt.lib().rt_scene_create_mesh_ex(R._p(va), len(va), R._p(ia), len(ia), 0, C.byref(h)))
        try:
            assert rt.lib().rt_scene_device_bytes(h) == a.device_bytes()
        finally:
            rt.lib().rt_scene_destroy(h)
        assert b.device_bytes() == a.device_bytes() + 4 * len(i) + 16 * len(v) + 4
        _same_tree(_download(rt, a), _download(rt, b), "dynamic against plain")


# ------------------------------------------------- exact, end to end --
def _camera(rt, pos, target, W, H, mode):
    sm, _, sh, rf = S.MODES[mode]
    vi, pi = cpuref.camera_matrices(pos, target, (0, 1, 0), 45.0, W / H, 0.01, 100.0)
    light = tuple(np.float32(target) + np.float32([2, 2, 2]))
    return rt.render_params(pos, vi, pi, light, sm, sh, rf)


def _frame(sc, P, W, H):
    c, t = np.zeros((H, W), np.uint32), np.full((H, W), np.inf, np.float32)
    sc.render(P, c, t, clear=True)
    return c, t


def _rays_at(lo, hi, n, seed):
    """Seeded incoherent rays around the box [lo, hi]: origins in the box blown
    up three times, directions towards random points of the box."""
    rng = np.random.default_rng(seed)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    o = (c + rng.uniform(-3, 3, (n, 3)) * h).astype(np.float32)
    p = (c + rng.uniform(-1, 1, (n, 3)) * h).astype(np.float32)
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def _trace(s, o, d, any_hit=False, stream=None):
    """rt_trace_rays_device -> {output: numpy}, all four outputs (or hit alone)."""
    n = len(o)
    o_t, d_t = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    out = {"hit": torch.full((n,), -7, dtype=torch.int32, device="cuda")}
    if not any_hit:
        out["t"] = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        out["normal"] = torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda")
        out["prim"] = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda k: out[k].data_ptr() if k in out else None
    s.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=ptr("hit"), t_ptr=ptr("t"), normal_ptr=ptr("normal"),
                   prim_ptr=ptr("prim"), any_hit=any_hit, stream=stream)
    torch.cuda.synchronize()
    return {k: a.cpu().numpy() for k, a in out.items()}


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_hits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs in {(_bits(a[k]) != _bits(b[k])).sum()} values"


def test_exact_translation_end_to_end(gpu):
    rt = gpu
    v, i = R.edge("grid", 1500)
    w = R.translate(v)
    lo, hi = w[:, :3].min(0).astype(np.float64), w[:, :3].max(0).astype(np.float64)
    with _scene(rt, v, i) as s, _scene(rt, w, i) as f:
        s.update_vertices(w)
        _same_tree(_download(rt, s), _download(rt, f), "updated against fresh")
        for a, b, what in zip(_constants(rt, s), _constants(rt, f), ("root_box", "root_child", "dmax2")):
            assert np.array_equal(a, b), what
        # a frame from a camera aimed at the MOVED mesh: a stale root box or
        # cull rectangle leaves it without the mesh
        W, H = 160, 90
        target = tuple((lo + hi) / 2)
        pos = (target[0] + 3.0, target[1] + 4.0, target[2] + 14.0)
        P = _camera(rt, pos, target, W, H, "default")
        for sc in (s, f):
            sc.set_plane(rt.Plane((0.0, 1.0, 0.0), float(lo[1])))
        fc, ft = _frame(f, P, W, H)
        sc_, st_ = _frame(s, P, W, H)
        assert np.array_equal(fc, sc_) and np.array_equal(ft.view(np.uint32), st_.view(np.uint32))
        for sc in (s, f):
            sc.set_plane(None)
        mesh_only = _frame(s, _camera(rt, pos, target, W, H, "primary"), W, H)[1]
        assert np.isfinite(mesh_only).sum() > W * H // 20, "the moved mesh is not in the frame"
        # rays: device buffers (closest hit with all outputs, any hit) and host buffers
        o, d = _rays_at(lo, hi, 4096, 41)
        got, ref = _trace(s, o, d), _trace(f, o, d)
        assert 400 < int(ref["hit"].sum()) < 4096
        _same_hits(got, ref, "closest hit")
        _same_hits(_trace(s, o, d, any_hit=True), _trace(f, o, d, any_hit=True), "any hit")
        hs, hf = s.intersect(o, d), f.intersect(o, d)
        for k in ("hitten", "t", "normal", "prim"):
            assert np.array_equal(_bits(getattr(hs, k)), _bits(getattr(hf, k))), f"rt_intersect_rays: {k}"
        assert np.array_equal(hs.hitten, ref["hit"].astype(bool))


def test_refitted_lattice_against_the_oracle_on_exact_path_rays(gpu):
    """A dynamic lattice mesh updated by the exact translation, traced with the
    lattice_axis and one_zero rays of ray_cases.py shifted by the same vector
    (origins on the moved box bounds, 1/d infinite): closest hit and any hit
    are the ORACLE's on the translated vertices, bitwise -- not another GPU
    scene's. test_ray_cases_host.py::test_refit_sets pins at least 100 oracle
    hits per set and interval."""
    import ray_cases as RC
    from test_rays_device import _assert_oracle
    from test_rays_device import _trace as trace_guarded
    rt = gpu
    v, i = RC.scene_input("lattice")[1]
    w = R.translate(v)
    rs = cpuref.RefScene.mesh(w, i)
    with _scene(rt, v, i) as s:
        s.update_vertices(w)
        for cls in ("lattice_axis", "one_zero"):
            o, d = RC.plain_sets("lattice")[cls]
            o = np.ascontiguousarray(o + R.SHIFT)
            o_t, d_t = torch.from_numpy(o).cuda(), torch.from_numpy(np.array(d)).cuda()
            for tn, tf in RC.PAIRS:
                ref = rs.intersect_rays(o, d, tn, tf)
                assert int(ref[0].sum()) >= 100
                what = f"refitted lattice {cls} [{tn}, {tf}]"
                _assert_oracle(ref, trace_guarded(s, o_t, d_t, len(o), tn=tn, tf=tf), what)
                a = trace_guarded(s, o_t, d_t, len(o), outputs=("hit",), tn=tn, tf=tf, any_hit=True)
                assert np.array_equal(ref[0], a["hit"]), f"{what}: any-hit mask differs"


# ------------------------------------------- general deformation, bunny --
@functools.lru_cache(maxsize=None)
def _bunny_deformed():
    v, i = R.bunny()
    w = R.deform(v)
    w.setflags(write=False)
    return w


def _eye_rays(rt, P, W, H, pos):
    d = np.zeros((H * W, 3), np.float32)
    from rtamd._lib import check
    check(rt.lib().rtx_eye_rays(C.byref(P), C.c_int32(W), C.c_int32(H), C.c_void_p(d.ctypes.data)))
    return np.tile(np.float32(pos), (H * W, 1)), d


def _rays_outside(lo, hi, n, seed):
    """Seeded incoherent rays from outside the box [lo, hi]: origins 2 to 3 of
    its circumsphere's radii from its centre, directions towards random points
    of the box. Every hit is at least one radius away: far beyond tNear."""
    rng = np.random.default_rng(seed)
    c, r = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (c + u * rng.uniform(2.0, 3.0, (n, 1)) * r).astype(np.float32)
    p = (c + rng.uniform(-1, 1, (n, 3)) * (hi - lo) / 2).astype(np.float32)
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def _bunny_rays(rt):
    """The 128x64 eye rays of the standard camera and 4096 incoherent rays
    around the deformed bunny."""
    W, H, pos = 128, 64, (0.0, 0.0, 2.5)
    eo, ed = _eye_rays(rt, S.params("stanford-bunny.obj", W, H, "primary", pos, "gpu"), W, H, pos)
    p = _bunny_deformed()
    p = (p[:, :3] / p[:, 3:4]).astype(np.float64)
    io, id_ = _rays_outside(p.min(0), p.max(0), 4096, 97)
    return np.concatenate([eo, io]), np.concatenate([ed, id_])


def test_deformed_bunny_answers_as_a_fresh_build(gpu):
    """The refitted and the freshly built tree differ, the triangles do not. A
    ray's answer can then differ in three ways, none of them an error:
      1. a slab test lies within rounding of a box face;
      2. two triangles give bit-equal t (the first one visited wins);
      3. a triangle is hit before tNear (or behind the origin). The reference's
         triangle test has no t range (ray_pack.ispc:132-165, tri_t): such a
         hit is returned when the triangle's LEAF box reaches into [tNear,
         tFar], so it depends on which triangles share that leaf.
    Case 3 is what a first set of rays met -- origins spread through the
    deformed bunny, 4 to 8 rays of 4096 per seed, every one with t < tNear =
    0.01 in at least one of the two answers (most of them negative) -- and one
    ray of twelve such sets met case 2. These rays start outside the mesh (all
    t > 1), and a float32 restatement of tri_t, bit-equal to the oracle on
    every ray, finds no two nearest triangles with equal t among them."""
    rt = gpu
    v, i = R.bunny()
    w = _bunny_deformed()
    o, d = _bunny_rays(rt)
    with _scene(rt, v, i) as s, _scene(rt, w, i, dynamic=False) as f:
        s.update_vertices(w)
        got, ref = _trace(s, o, d), _trace(f, o, d)
        assert 1000 < int(ref["hit"].sum()) < len(o)
        _same_hits(got, ref, "updated against fresh")
        cs, cf = _constants(rt, s), _constants(rt, f)
        assert np.array_equal(cs[0].view(np.float32), cf[0].view(np.float32))  # root_box, by value
        assert cs[2] == cf[2]  # dmax2, bits


# ----------------------------------------------------------- rt_multi --
def test_multi_follows_the_update(gpu):
    rt = gpu
    v, i = R.bunny()
    w = _bunny_deformed()
    W, H = 160, 90
    P = S.params("stanford-bunny.obj", W, H, "default", (0.0, 0.3, 2.5), "gpu")
    with _scene(rt, v, i) as s:
        s.set_plane(rt.Plane((0.0, 1.0, 0.0), S.inputs("stanford-bunny.obj")[2]))
        with rt.MultiRenderer(s, (0, 0)) as mr:
            first = _frame(mr, P, W, H)
            before = _frame(s, P, W, H)
            assert np.array_equal(first[0], before[0])
            s.update_vertices(w)
            second, single = _frame(mr, P, W, H), _frame(s, P, W, H)
            assert np.array_equal(second[0], single[0])
            assert np.array_equal(second[1].view(np.uint32), single[1].view(np.uint32))
            assert not np.array_equal(single[0], before[0])  # (the update is visible at all)


# ------------------------------------------------------------- errors --
def test_refused_updates_leave_the_scene(gpu):
    rt = gpu
    L = rt.lib()
    v, i = R.edge("rand", 1500)
    w = R.deform(v)
    W, H = 160, 90
    P = S.params("rand", W, H, "primary", (0.0, 0.0, 9.0), "gpu")
    w_t = torch.from_numpy(w).cuda()
    torch.cuda.synchronize()

    def refused(h, ptr, n, code, word):
        host = R._p(w) if ptr is not None else None
        for rc in (L.rt_scene_update_vertices(h, host, n), L.rt_scene_update_vertices_device(h, ptr, n, None)):
            msg = L.rt_last_error()
            assert rc == code and msg and word in msg, (rc, msg)

    with _scene(rt, v, i, dynamic=False) as plain, _scene(rt, v, i) as dyn:
        gname = "example_grid.grid"
        grid = S.gpu_scene(gname)
        S.set_planes(gname, "primary", grid)
        PG = S.params(gname, W, H, "primary", module="gpu")
        frames = [_frame(plain, P, W, H), _frame(dyn, P, W, H), _frame(grid, PG, W, H)]
        assert np.isfinite(frames[0][1]).any() and np.isfinite(frames[2][1]).any()
        ptr = C.c_void_p(w_t.data_ptr())
        refused(plain._handle(), ptr, len(w), RT_E_STATE, b"RT_MESH_DYNAMIC")
        refused(grid._handle(), ptr, len(w), RT_E_STATE, b"not a mesh")
        refused(dyn._handle(), ptr, len(w) - 1, RT_E_INVALID, b"nverts")
        refused(dyn._handle(), ptr, 0, RT_E_INVALID, b"nverts")
        refused(dyn._handle(), None, len(w), RT_E_INVALID, b"NULL")
        again = [_frame(plain, P, W, H), _frame(dyn, P, W, H), _frame(grid, PG, W, H)]
        for a, b in zip(frames, again):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# -------------------------------------------------------------- torch --
@pytest.mark.parametrize("cols", [4, 3])
def test_torch_update_in_stream_order(gpu, cols):
    """The vertices are produced by a torch kernel on a side stream, the update
    and the trace follow on that stream: the result is the fresh scene's."""
    from rtamd import torch_rays
    rt = gpu
    v, i = R.bunny()
    w = _bunny_deformed()
    assert (v[:, 3] == 1).all()
    o, d = _bunny_rays(rt)
    o_t, d_t = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    base_t = torch.from_numpy(np.array(v[:, :cols])).cuda()
    step_t = torch.from_numpy(np.ascontiguousarray((w - v)[:, :cols])).cuda()
    torch.cuda.synchronize()
    with _scene(rt, v, i) as s:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            verts = base_t + step_t  # the kernel whose output the update reads
            torch_rays.update_vertices(s, verts)
            got = torch_rays.trace(s, o_t, d_t)
        side.synchronize()
        # the fresh scene of exactly what that kernel made (v + (w - v) rounds)
        made = verts.cpu().numpy()
        if cols == 3:
            made = np.concatenate([made, np.ones((len(made), 1), np.float32)], axis=1)
        assert np.abs(made - w).max() < 1e-6 and (made[:, 3] == 1).all()
        with _scene(rt, made, i, dynamic=False) as f:
            ref = torch_rays.trace(f, o_t, d_t)
            torch.cuda.synchronize()
        for k in ("hit", "t", "normal", "prim"):
            x, y = getattr(got, k).cpu().numpy(), getattr(ref, k).cpu().numpy()
            assert np.array_equal(_bits(x), _bits(y)), k
        assert 1000 < int(ref.hit.sum()) < len(o)


def test_torch_update_rejects_bad_tensors(gpu):
    from rtamd import torch_rays
    rt = gpu
    v, i = R.edge("rand", 1500)
    with _scene(rt, v, i) as s:
        before = _download(rt, s)
        good = torch.from_numpy(np.array(v)).cuda()
        bad = [np.array(v), good.double(), good.cpu(), good[:, :2].contiguous(), good.reshape(-1), good.t()[:3].t(),
               good[:0]]
        for x in bad:
            with pytest.raises(ValueError):
                torch_rays.update_vertices(s, x)
        _same_tree(_download(rt, s), before, "after the refused tensors")
        with pytest.raises(rt.RtError):  # a wrong vertex count is the library's refusal
            torch_rays.update_vertices(s, good[:-1].contiguous())
        _same_tree(_download(rt, s), before, "after the refused count")
