"""Mixed instanced scenes on the GPU: meshes, SDF grids and SDF octrees as
bottom-level scenes (rt_scene_create_instanced_any, include/rtamd.h;
csrc/rt_instances_mixed.hip).

Every comparison is on bits. The reference is the header's loop composed from
the oracle alone (instances_common.compose, tlas_common.compose_tlas) over
cpuref scenes of all three kinds, on the M and the leaf boxes read back from
the device; shading is shading_ref above that composition. Buffers are
sentinel-filled with guards (tests/test_instances_gpu.py's _trace,
tests/test_shade_gpu.py's _shade). The inputs' conditions (every kind wins,
hits are replaced across kinds) are checked on the CPU in test_mixed_host.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cpuref
import instances_common as IC
import mixed_common as MC
import rtamd
import shade_common as SC
import shading_ref as SR
import tlas_common as TC
from rtamd import _lib, torch_rays
from test_instances_gpu import ALL, PAIRS, PLANE_OFF, _assert_ref, _bits, _same, _set_plane, _trace
from test_shade_gpu import _assert_oracle, _shade

pytestmark = pytest.mark.gpu

N = MC.N
RT_E_INVALID, RT_E_STATE = -1, -4
SCENES = [n for n in MC.DEFS]


@functools.lru_cache(maxsize=None)
def _blas(name):
    return MC.gpu_blas(rtamd, name)


@functools.lru_cache(maxsize=None)
def _scene(name, tlas):
    names, inst = MC.DEFS[name]
    gs = rtamd.InstancedScene([_blas(m) for m in names], inst, tlas=tlas)
    assert gs.mixed
    return gs


@functools.lru_cache(maxsize=None)
def _rays(name, kind="random"):
    o, d = MC.rays(name, kind)
    return o, d, torch.from_numpy(np.array(o)).cuda(), torch.from_numpy(np.array(d)).cuda()  # (writable copies for torch)


def _compose(name, gs, o, d, tn, tf, names=None):
    tab = gs.instances()
    rf = MC.refs(names or MC.DEFS[name][0])
    if gs.has_tlas:
        return TC.compose_tlas(rf, tab.blas, tab.flags, tab.inv, gs.tlas()[0], o, d, tn, tf, tab.skipped)[:4]
    return IC.compose(rf, tab.blas, tab.flags, tab.inv, o, d, tn, tf, tab.skipped)


@functools.lru_cache(maxsize=None)
def _ref(name, tlas, kind, tn, tf):
    """The composed reference of a scene without its plane, once."""
    o, d, _, _ = _rays(name, kind)
    out = _compose(name, _scene(name, tlas), o, d, tn, tf)
    for a in out:
        a.setflags(write=False)
    return out


def _check_all(name, tlas, kind, plane, tn, tf, n=N):
    """Closest hit with all four outputs and any hit against the reference."""
    gs = _scene(name, tlas)
    _set_plane(gs, plane)
    o, d, o_t, d_t = _rays(name, kind)
    ref = tuple(a[:n] for a in _ref(name, tlas, kind, tn, tf))
    if plane:
        ref = IC.with_plane(ref, o[:n], d[:n], tn, tf, PLANE_OFF)
    what = f"{name} tlas={tlas} {kind} plane={plane} [{tn}, {tf}] n={n}"
    _assert_ref(ref, _trace(gs, o_t, d_t, n, tn=tn, tf=tf), what)
    a = _trace(gs, o_t, d_t, n, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
    assert np.array_equal(ref[0], a["hit"]), f"{what}: any-hit mask differs from the closest-hit flag"
    return ref


# ------------------------------------------------- parity with the oracle --
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("tlas", [False, True])
@pytest.mark.parametrize("plane", [False, True])
def test_parity_with_composed_oracle(gpu, name, tlas, plane):
    """4,096 random rays: closest hit with all four outputs, and any hit; the
    small scenes under all three intervals, m130's tree under the first and the
    last, its flat list (130 oracle passes over every ray) under the first."""
    pairs = PAIRS if name != "m130" else (PAIRS[0], PAIRS[2]) if tlas else (PAIRS[0],)
    for tn, tf in pairs:
        ref = _check_all(name, tlas, "random", plane, tn, tf)
        if not plane and tn == 0.01:
            inst, _ = torch_rays.split_prim(ref[3])
            assert int((inst >= 0).sum()) > 100, "the scene is hardly hit"
            if name in ("m3", "m9", "m130"):
                names, defs = MC.DEFS[name]
                kinds = np.array([MC.KIND[names[t[0]]] for t in defs])
                won = kinds[inst[inst >= 0]]
                assert all((won == k).sum() > 50 for k in (MC.MESH, MC.GRID, MC.OCT)), "a kind never wins"
            if name == "m130":
                assert len(np.unique(inst[inst >= 0])) > 64


@pytest.mark.parametrize("name", ["m3", "m9", "m130"])
@pytest.mark.parametrize("tlas", [False, True])
def test_eye_rays(gpu, name, tlas):
    """64 x 64 coherent eye rays: the tree's shared mesh rounds and the flat
    list's wave-level mesh traversal beside per-lane SDF work."""
    ref = _check_all(name, tlas, "eye", False, 0.01, 100.0)
    assert int(ref[0].sum()) > 200
    _check_all(name, tlas, "eye", True, 0.01, 100.0)


@pytest.mark.parametrize("name", ["m9", "m130"])
@pytest.mark.parametrize("tlas", [False, True])
def test_per_ray_intervals(gpu, name, tlas):
    """d_tnear / d_tfar arrays (each ray draws one of the three intervals): the
    per-lane mesh traversal everywhere; with and without the plane."""
    gs = _scene(name, tlas)
    o, d, o_t, d_t = _rays(name)
    pick = np.random.default_rng(22).integers(0, 3, N)
    tn = np.float32([p[0] for p in PAIRS])[pick]
    tf = np.float32([p[1] for p in PAIRS])[pick]
    tn_t, tf_t = torch.from_numpy(tn).cuda(), torch.from_numpy(tf).cuda()
    base = _compose(name, gs, o, d, tn, tf)
    for plane in (False, True):
        _set_plane(gs, plane)
        ref = IC.with_plane(base, o, d, tn, tf, PLANE_OFF) if plane else base
        kw = dict(tn=0.25, tf=3.0, tn_t=tn_t, tf_t=tf_t)
        _assert_ref(ref, _trace(gs, o_t, d_t, N, **kw), f"{name} tlas={tlas} per-ray plane={plane}")
        got = _trace(gs, o_t, d_t, N, outputs=("hit",), any_hit=True, **kw)
        assert np.array_equal(ref[0], got["hit"]), "any-hit mask differs"


@pytest.mark.parametrize("blas", ["grid17", "example_grid", "oct2", "sdf_5"])
@pytest.mark.parametrize("tlas", [False, True])
def test_m1_is_the_plain_kind(gpu, blas, tlas):
    """One SDF instance under the identity: output for output the plain scene's
    rt_trace_rays_device, prim's high word 0, with and without the plane; and
    rt_intersect_rays on host buffers. The normal of an object hit is the plain
    kind's under the header's formula with M = I: w = n, then w / sqrt((w.x w.x
    + w.y w.y) + w.z w.z) in float32, which may move the last bit of a vector
    that is already normalised (tests/test_instances_gpu.py has the same note)."""
    gs, plain = _scene(f"m1-{blas}", tlas), _blas(blas)
    o, d, o_t, d_t = _rays("m1")
    for plane in (False, True):
        _set_plane(gs, plane)
        _set_plane(plain, plane)
        for tn, tf in PAIRS:
            a, b = _trace(gs, o_t, d_t, N, tn=tn, tf=tf), _trace(plain, o_t, d_t, N, tn=tn, tf=tf)
            x = _trace(gs, o_t, d_t, N, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
            y = _trace(plain, o_t, d_t, N, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
            # the tree's definition asks the BLAS only for rays that pass its world box
            # (under tNear < 0 the cube may lie wholly behind a ray the plain march still hits)
            ask = TC.box_pass(gs.tlas()[0][0], o, d, tn, tf) if tlas else np.ones(N, bool)
            assert (a["prim"][~ask] < 0).all() and int(ask.sum()) > N // 4
            a, b, x, y = ({k: v[ask] for k, v in r.items()} for r in (a, b, x, y))
            obj = b["prim"] >= 0
            assert np.array_equal(a["prim"][obj] >> 32, np.zeros(int(obj.sum()), np.int64))
            assert np.array_equal(a["prim"][obj] & 0xFFFFFFFF, b["prim"][obj]) and np.array_equal(a["prim"][~obj], b["prim"][~obj])
            _same({k: a[k] for k in ("hit", "t")}, {k: b[k] for k in ("hit", "t")}, f"m1 {blas} [{tn}, {tf}]")
            w = b["normal"]
            ln = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
            assert ln.dtype == np.float32
            want = np.where(obj[:, None], w / ln[:, None], w).astype(np.float32)
            assert np.array_equal(_bits(a["normal"]), _bits(want)), f"m1 {blas} [{tn}, {tf}]: normal differs"
            assert int(obj.sum()) > 100
            assert np.array_equal(x["hit"], y["hit"])
    _set_plane(plain, False)
    _set_plane(gs, False)
    h = gs.intersect(o, d, 0.01, 100.0)
    ref = _trace(gs, o_t, d_t, N)
    _same(ref, {"hit": h.hitten.astype(np.int32), "t": h.t, "normal": h.normal, "prim": h.prim}, "host entry")


def test_grid_address_paths(gpu):
    """The 17 x 9 x 13 grid created under rtx_set_grid_force 0 (linear, buffer
    loads), 1 (bricked, buffer loads) and 3 (bricked, 64-bit addresses): the
    three launch modes of rt_dispatch.h. The mixed scenes over them agree bit
    for bit, flat and tree, and with the oracle."""
    L = rtamd.lib()
    names, inst = MC.DEFS["m3"]
    o, d, o_t, d_t = _rays("m3")
    outs, keep = {}, []
    try:
        for force in (0, 1, 3):
            _lib.check(L.rtx_set_grid_force(force))
            g = MC.gpu_blas(rtamd, "grid17")
            for tlas in (False, True):
                gs = rtamd.InstancedScene([_blas("bunny"), g, _blas("sdf_5")], inst, tlas=tlas)
                outs[force, tlas] = (_trace(gs, o_t, d_t, N), _trace(gs, o_t, d_t, N, outputs=("hit",), any_hit=True))
                keep.append(gs)
            keep.append(g)
    finally:
        _lib.check(L.rtx_set_grid_force(0))
    for tlas in (False, True):
        ref = _ref("m3", tlas, "random", 0.01, 100.0)
        for force in (0, 1, 3):
            _assert_ref(ref, outs[force, tlas][0], f"grid force {force} tlas={tlas}")
            assert np.array_equal(ref[0], outs[force, tlas][1]["hit"])
            _same(outs[0, tlas][0], outs[force, tlas][0], f"grid force {force} against 0")
    for s in keep:
        s.close()


# ------------------------------------- against the mesh-only kernels --
def _mesh_defs():
    return ("cube", "bunny"), [(0, IC.affine(IC.rot(81) @ np.diag([0.6, 0.9, 0.5]), (-0.3, 0.1, 0.2)), 0),
                               (1, IC.affine(IC.rot(82) @ np.diag([1.1, 0.8, 1.0]), (0.1, -0.1, 0.0)), 0),
                               (0, IC.affine(IC.rot(83) @ np.diag([0.5, 0.5, 1.2]), (0.4, 0.2, -0.3)), 0)]


@pytest.mark.parametrize("tlas", [False, True])
def test_meshes_plus_an_idle_sdf_instance(gpu, tlas):
    """Meshes plus one SDF instance placed last, disabled or far outside every
    ray's reach: the outputs of the mesh-only scene of
    rt_scene_create_instanced_ex, random and eye rays, closest and any hit."""
    names, inst = _mesh_defs()
    meshes = [_blas(m) for m in names]
    plain = rtamd.InstancedScene(meshes, inst, tlas=tlas)
    assert not plain.mixed
    far = IC.affine(np.eye(3), (500.0, 400.0, -300.0))
    for last in ((2, IC.IDENTITY, IC.DISABLED), (2, far, 0)):
        for sdf in ("grid17", "sdf_5"):
            gs = rtamd.InstancedScene(meshes + [_blas(sdf)], inst + [last], tlas=tlas)
            assert gs.mixed
            for kind in ("random", "eye"):
                _, _, o_t, d_t = _rays("m3", kind)
                for tn, tf in (PAIRS[0], PAIRS[2]):
                    a, b = _trace(gs, o_t, d_t, N, tn=tn, tf=tf), _trace(plain, o_t, d_t, N, tn=tn, tf=tf)
                    _same(a, b, f"idle {sdf} flags={last[2]} {kind}")
                    assert tn != 0.01 or int(b["hit"].sum()) > 100  # (the eye rays reach nothing before t = 2)
                    x = _trace(gs, o_t, d_t, N, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
                    assert np.array_equal(x["hit"], b["hit"])
            gs.close()
    plain.close()


@pytest.mark.parametrize("tlas", [False, True])
def test_mesh_only_list_is_the_old_scene(gpu, tlas):
    """A mesh-only list through the new entry: equal rt_scene_device_bytes, equal outputs."""
    L = rtamd.lib()
    names, inst = _mesh_defs()
    hs = (C.c_void_p * len(names))(*[_blas(m)._handle() for m in names])
    arr = (_lib.Instance * len(inst))()
    for k, t in enumerate(inst):
        arr[k].blas, arr[k].flags = t[0], t[2]
        arr[k].xform[:] = np.asarray(t[1], np.float32).reshape(12).tolist()
    fl = _lib.RT_INSTANCED_TLAS if tlas else 0
    h_any, h_ex = C.c_void_p(), C.c_void_p()
    assert L.rt_scene_create_instanced_any(hs, len(names), arr, len(inst), fl, C.byref(h_any)) == 0
    assert L.rt_scene_create_instanced_ex(hs, len(names), arr, len(inst), fl, C.byref(h_ex)) == 0
    K, P = len(inst), TC.leaf_count(len(inst))
    want = K * 64 + len(names) * 56 + (K * 48 + 2 * P * 32 if tlas else 0)
    assert L.rt_scene_device_bytes(h_any) == L.rt_scene_device_bytes(h_ex) == want
    _, _, o_t, d_t = _rays("m3")
    outs = []
    for h in (h_any, h_ex):
        hit = torch.zeros(N, dtype=torch.int32, device="cuda")
        t = torch.zeros(N, dtype=torch.float32, device="cuda")
        nrm = torch.zeros((N, 3), dtype=torch.float32, device="cuda")
        prim = torch.zeros(N, dtype=torch.int64, device="cuda")
        b = _lib.RayBatch(N, o_t.data_ptr(), d_t.data_ptr(), None, None, 0.01, 100.0, hit.data_ptr(), t.data_ptr(),
                          nrm.data_ptr(), prim.data_ptr())
        assert L.rt_trace_rays_device(h, C.byref(b), 0, None) == 0
        torch.cuda.synchronize()
        outs.append({"hit": hit.cpu().numpy(), "t": t.cpu().numpy(), "normal": nrm.cpu().numpy(), "prim": prim.cpu().numpy()})
        assert L.rt_scene_destroy(h) == 0
    _same(outs[0], outs[1], "mesh-only list")
    assert int(outs[0]["hit"].sum()) > 100


def test_flat_and_tree_agree_on_m130(gpu):
    """On m130 the flat list and the tree: the count of rays that differ in any
    output is reported (the tree's definition has the box_pass line); each
    already equals its own reference."""
    for kind in ("random", "eye"):
        _, _, o_t, d_t = _rays("m130", kind)
        a, b = _trace(_scene("m130", False), o_t, d_t, N), _trace(_scene("m130", True), o_t, d_t, N)
        differ = np.zeros(N, bool)
        for k in ALL:
            differ |= (_bits(a[k]) != _bits(b[k])).reshape(N, -1).any(axis=1)
        print(f"m130 {kind}: {int(differ.sum())} of {N} rays differ between the flat list and the tree")
        fa, fb = _ref("m130", False, kind, 0.01, 100.0), _ref("m130", True, kind, 0.01, 100.0)
        want = np.zeros(N, bool)
        for x, y in zip(fa, fb):
            want |= (_bits(x) != _bits(y)).reshape(N, -1).any(axis=1)
        assert np.array_equal(differ, want), "the kernels differ on other rays than the two definitions do"


# ------------------------------------------------ sizes, unwanted outputs --
@pytest.mark.parametrize("tlas", [False, True])
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_partial_waves(gpu, tlas, n):
    """[0, n) fully written, misses included, the 64 elements behind it not."""
    _check_all("m9", tlas, "random", False, 0.01, 100.0, n=n)
    _check_all("m9", tlas, "eye", True, 0.01, 100.0, n=n)


@pytest.mark.parametrize("tlas", [False, True])
def test_no_rays_and_output_subsets(gpu, tlas):
    """n = 0 launches nothing; an output left NULL is not computed or written
    (its buffer does not exist: _trace's guards cover the others), every subset
    equals the full query's values."""
    gs = _scene("m9", tlas)
    _set_plane(gs, False)
    _, _, o_t, d_t = _rays("m9")
    hit = torch.full((8,), 77, dtype=torch.int32, device="cuda")
    gs.trace_device(o_t.data_ptr(), d_t.data_ptr(), 0, hit_ptr=hit.data_ptr())
    torch.cuda.synchronize()
    assert (hit.cpu().numpy() == 77).all()
    full = _trace(gs, o_t, d_t, N)
    for outs in (("hit",), ("t",), ("normal",), ("prim",), ("t", "prim"), ("hit", "normal")):
        got = _trace(gs, o_t, d_t, N, outputs=outs)
        _same(got, {k: full[k] for k in outs}, f"outputs {outs}")


# ------------------------------------------------------------- updates --
@pytest.mark.parametrize("tlas", [False, True])
def test_updates_in_stream_order(gpu, tlas):
    """Poses from the device move an SDF instance with no host wait; a singular
    matrix makes its instance skipped; rt_scene_update_instances moves an
    instance from a mesh to a grid. Each state equals a scene created fresh."""
    names, inst = MC.DEFS["m3"]
    objs = [_blas(m) for m in names]
    gs = rtamd.InstancedScene(objs, inst, tlas=tlas)
    fresh = lambda items: rtamd.InstancedScene(objs, items, tlas=tlas)
    _, _, o_t, d_t = _rays("m3")
    before = _trace(gs, o_t, d_t, N)
    moved = [inst[0], (1, MC.rigid(91, (0.5, -0.4, 0.3)), 0), (2, MC.rigid(92, (-0.6, 0.3, -0.2)), 0)]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        x = torch.from_numpy(np.stack([t[1] for t in moved[1:]])).cuda() * 1.0  # produced by a torch kernel on this stream
        torch_rays.update_instances(gs, x, first=1)
        r = torch_rays.trace(gs, o_t, d_t)
    st.synchronize()
    f1 = fresh(moved)
    want = _trace(f1, o_t, d_t, N)
    _same({k: getattr(r, k).cpu().numpy() for k in ALL}, want, "poses from the device")
    assert not np.array_equal(_bits(before["t"]), _bits(want["t"]))
    if tlas:
        assert np.array_equal(_bits(gs.tlas()[0]), _bits(f1.tlas()[0]))
        assert np.array_equal(_bits(gs.tlas()[0][1]), _bits(TC.world_box(moved[1][1], MC.UNIT_CUBE)))
    _assert_ref(_compose("m3", gs, *_rays("m3")[:2], 0.01, 100.0), want, "poses from the device: the oracle")
    # a matrix the inverse refuses: the instance is skipped until its next update
    bad = np.array(moved[2][1])[None].copy()
    bad[0, 2, :3] = bad[0, 1, :3]
    torch_rays.update_instances(gs, torch.from_numpy(bad).cuda(), first=2)
    assert gs.instances().skipped.tolist() == [0, 0, 1]
    without = fresh([moved[0], moved[1], (2, moved[2][1], IC.DISABLED)])
    _same(_trace(gs, o_t, d_t, N), _trace(without, o_t, d_t, N), "a skipped instance")
    if tlas:
        assert np.array_equal(gs.tlas()[0][2], TC.EMPTY)
    torch_rays.update_instances(gs, torch.from_numpy(np.array(moved[2][1])[None].copy()).cuda(), first=2)
    _same(_trace(gs, o_t, d_t, N), want, "the instance is back")
    # the host entry moves instance 0 from the mesh (BLAS 0) to the grid (BLAS 1)
    gs.update_instances(np.array(moved[0][1])[None], first=0, blas=[1])
    f2 = fresh([(1, moved[0][1], 0), moved[1], moved[2]])
    got = _trace(gs, o_t, d_t, N)
    _same(got, _trace(f2, o_t, d_t, N), "an instance moved to a BLAS of another kind")
    assert gs.instances().blas.tolist() == [1, 1, 2] and not np.array_equal(_bits(got["t"]), _bits(want["t"]))
    for s in (gs, f1, f2, without):
        s.close()


@pytest.mark.parametrize("tlas", [False, True])
def test_dynamic_mesh_blas_is_seen(gpu, tlas):
    """A dynamic cube BLAS refitted on the same stream is seen by the next
    trace of a mixed scene: outputs (and leaf boxes) of a scene created
    afterwards; an exact translation equals the oracle on the moved cube."""
    v, i = IC.mesh("cube")
    cube = rtamd.BVHBuilder(rtamd.SimpleMesh(v, i), dynamic=True)
    objs = [cube, _blas("grid17"), _blas("oct2")]
    inst = [(0, IC.affine(IC.rot(95) @ np.diag([0.6, 0.5, 0.7]), (0.1, 0.0, 0.1)), 0), (1, MC.rigid(96, (-0.7, 0.1, 0.0)), 0),
            (2, MC.rigid(97, (0.8, 0.0, -0.1)), 0)]
    gs = rtamd.InstancedScene(objs, inst, tlas=tlas)
    o, d, o_t, d_t = _rays("m3")
    before = _trace(gs, o_t, d_t, N)
    w = np.array(v)
    w[:, :3] += np.float32([0.5, -0.25, 0.75])  # exact in float32 on the cube's corners
    torch_rays.update_vertices(cube, torch.from_numpy(w).cuda())
    after = _trace(gs, o_t, d_t, N)
    again = rtamd.InstancedScene(objs, inst, tlas=tlas)
    _same(after, _trace(again, o_t, d_t, N), "after the refit")
    assert not np.array_equal(_bits(before["t"]), _bits(after["t"]))
    if tlas:
        assert np.array_equal(_bits(gs.tlas()[0]), _bits(again.tlas()[0]))
    tab = gs.instances()
    rf = {0: cpuref.RefScene.mesh(w, i), 1: MC.ref_blas("grid17"), 2: MC.ref_blas("oct2")}
    if tlas:
        ref = TC.compose_tlas(rf, tab.blas, tab.flags, tab.inv, gs.tlas()[0], o, d, 0.01, 100.0)[:4]
    else:
        ref = IC.compose(rf, tab.blas, tab.flags, tab.inv, o, d, 0.01, 100.0)
    _assert_ref(ref, after, "after the refit: the oracle")
    inst_hit, _ = torch_rays.split_prim(ref[3])
    assert all((inst_hit == k).sum() > 30 for k in range(3))
    for s in (gs, again, cube):
        s.close()


# ------------------------------------------------------------- shading --
SHADINGS = [("std", SR.LAMBERT, True, True), ("std", SR.NORMAL, True, True), ("std", SR.COLOR, True, True)]
SHADE_PLANE = ((0.0, 1.0, 0.0), -1.4)


def _shade_params(name, shading, module=rtamd):
    ln, mode, sh, rf = shading
    return SC.params(64, 64, ln, mode, sh, rf, MC.EYE_POS[name], module=module)


@pytest.mark.parametrize("name", ["m3", "m9"])
@pytest.mark.parametrize("tlas", [False, True])
def test_shaded_eye_rays(gpu, name, tlas):
    """64 x 64 eye rays through torch_rays.eye_rays and the shade entry:
    Lambert with shadows and reflections, Normal and Color, with the plane on
    and off, against shading_ref over the composed intersection."""
    gs = _scene(name, tlas)
    orc = SC.device_oracle(gs, [MC.ref_blas(m) for m in MC.DEFS[name][0]])
    for shading in SHADINGS:
        P = _shade_params(name, shading)
        o_t, d_t = torch_rays.eye_rays(P, 64, 64)
        torch.cuda.synchronize()
        o, d = o_t.cpu().numpy(), d_t.cpu().numpy()
        for plane in (SHADE_PLANE, None):
            if plane is None and shading[1] != SR.LAMBERT:
                continue
            gs.set_plane(rtamd.Plane(*plane) if plane else None)
            ref = SC.shade(orc, plane, o, d, 0.01, 100.0, *shading)
            got = _shade(gs, o_t, d_t, N, P)
            _assert_oracle(ref, got, f"{name} tlas={tlas} {shading} plane={plane is not None}", min_defined=0.98)
            assert int(ref.hit.sum()) > 500
            if plane is not None and shading[1] == SR.LAMBERT:
                r = torch_rays.shade(gs, o_t, d_t, P, outputs=("color", "t", "hit", "prim"))
                assert np.array_equal(r.color.cpu().numpy().view(np.uint32), got["color"])
    gs.set_plane(None)


@pytest.mark.parametrize("tlas", [False, True])
def test_shaded_random_rays_and_depth_composition(gpu, tlas):
    """4,096 random rays with per-ray intervals under the plane; then
    RT_SHADE_CLEAR off with d_tfar = d_t: a second scene shaded into the
    buffers of the first composes by depth."""
    gs = _scene("m9", tlas)
    orc = SC.device_oracle(gs, [MC.ref_blas(m) for m in MC.DEFS["m9"][0]])
    shading = SHADINGS[0]
    P = _shade_params("m9", shading)
    o, d, o_t, d_t = _rays("m9")
    cls = np.random.default_rng(23).integers(0, len(SC.CLASSES), N)
    tn = np.float32([SC.CLASSES[c][0] for c in cls])
    tf = np.float32([SC.CLASSES[c][1] for c in cls])
    gs.set_plane(rtamd.Plane(*SHADE_PLANE))
    ref = SC.shade(orc, SHADE_PLANE, o, d, tn, tf, *shading)
    got = _shade(gs, o_t, d_t, N, P, tn_t=torch.from_numpy(tn).cuda(), tf_t=torch.from_numpy(tf).cuda())
    _assert_oracle(ref, got, f"m9 tlas={tlas} random rays", min_defined=0.98)
    gs.set_plane(None)
    # depth composition on the first 512 rays: m3 first (cleared), then m9 with
    # tFar = the t buffer (+inf where m3 missed) and clear off
    n = 512
    o, d, o_t, d_t = o[:n], d[:n], o_t[:n].contiguous(), d_t[:n].contiguous()
    first = _scene("m3", tlas)
    first.set_plane(None)
    a = torch_rays.shade(first, o_t, d_t, P, outputs=("color", "t"))
    color, t = a.color.clone(), a.t.clone()
    torch_rays.shade(gs, o_t, d_t, P, tfar=t, clear=False, color=color, t=t)
    torch.cuda.synchronize()
    r1 = SC.shade(SC.device_oracle(first, [MC.ref_blas(m) for m in MC.DEFS["m3"][0]]), None, o, d, 0.01, 100.0, *shading)
    r2 = SC.shade(orc, None, o, d, 0.01, r1.t, *shading)
    take = r2.hit != 0
    want_t = np.where(take, r2.t, r1.t).astype(np.float32)
    want_c = np.where(take, r2.color, r1.color)
    ok = np.where(take, r2.ok, r1.ok)
    assert np.array_equal(_bits(t.cpu().numpy()), _bits(want_t))
    bad = (color.cpu().numpy().view(np.uint32) != want_c) & ok
    assert not bad.any(), f"depth composition: colour differs on {int(bad.sum())} rays"
    assert int(take.sum()) > 20 and int((~take & (r1.hit != 0)).sum()) > 20


# ------------------------------------------------------------ refusals --
def test_refusals(gpu):
    """The argument rules of the new entry; the frame entries still return
    RT_E_STATE; refused calls write nothing and leave answers unchanged."""
    L = gpu.lib()
    names, inst = MC.DEFS["m3"]
    objs = [_blas(m) for m in names]
    hs = (C.c_void_p * 3)(*[b._handle() for b in objs])
    mk = lambda items: _instances(items)
    arr = mk(inst)
    out = C.c_void_p()
    assert L.rt_scene_create_instanced_any(hs, 3, arr, 3, 2, C.byref(out)) == RT_E_INVALID and not out.value
    gs = _scene("m3", True)
    nested = (C.c_void_p * 2)(objs[0]._handle(), gs._handle())
    assert L.rt_scene_create_instanced_any(nested, 2, arr, 1, 0, C.byref(out)) == RT_E_STATE and not out.value
    nulls = (C.c_void_p * 2)(objs[1]._handle(), None)
    assert L.rt_scene_create_instanced_any(nulls, 2, arr, 1, 0, C.byref(out)) == RT_E_INVALID and not out.value
    assert L.rt_scene_create_instanced_any(hs, 3, mk([(3, IC.IDENTITY, 0)]), 1, 0, C.byref(out)) == RT_E_INVALID
    assert L.rt_scene_create_instanced_any(hs, 3, mk([(1, IC.IDENTITY, 4)]), 1, 0, C.byref(out)) == RT_E_INVALID
    assert L.rt_scene_create_instanced_any(hs, 3, mk([(1, np.zeros((3, 4), np.float32), 0)]), 1, 0, C.byref(out)) == RT_E_INVALID
    assert not out.value and L.rt_last_error()
    # the old entries keep refusing an SDF BLAS
    assert L.rt_scene_create_instanced_ex(hs, 3, arr, 3, 0, C.byref(out)) == RT_E_STATE and not out.value
    # the entries that do not take the kind; a refused update changes nothing
    h = gs._handle()
    _set_plane(gs, False)
    _, _, o_t, d_t = _rays("m3")
    before = _trace(gs, o_t, d_t, N)
    P = rtamd.render_params((0, 0, 2.5), *cpuref.camera_matrices((0, 0, 2.5), aspect=1.0))
    c = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    t = torch.zeros((8, 8), dtype=torch.float32, device="cuda")
    hc, ht = np.zeros((8, 8), np.uint32), np.zeros((8, 8), np.float32)
    cp, tp = (C.c_void_p * 1)(c.data_ptr()), (C.c_void_p * 1)(t.data_ptr())
    mean, total, rep = C.c_float(), C.c_float(), C.c_void_p()
    pv = lambda a: C.c_void_p(a.ctypes.data)
    state = {
        "rt_render": L.rt_render(h, C.byref(P), pv(hc), pv(ht), 8, 8, 1, None),
        "rt_render_device": L.rt_render_device(h, C.byref(P), c.data_ptr(), t.data_ptr(), 8, 8, 1, None, None),
        "rt_render_device_frames": L.rt_render_device_frames(h, C.byref(P), 1, cp, tp, 8, 8, 1, None, None),
        "rt_bench_frames": L.rt_bench_frames(h, C.byref(P), 1, 8, 8, 1, C.byref(mean), C.byref(total)),
        "rt_scene_replicate": L.rt_scene_replicate(h, 0, C.byref(rep)),
        "update: blas out of range": L.rt_scene_update_instances(h, 0, 1, mk([(3, IC.IDENTITY, 0)])),
        "update: singular": L.rt_scene_update_instances(h, 1, 1, mk([(1, np.zeros((3, 4), np.float32), 0)])),
        "update: range": L.rt_scene_update_instances(h, 2, 2, mk(inst[:2])),
    }
    want = {k: RT_E_STATE if k.startswith("rt_") else RT_E_INVALID for k in state}
    assert state == want
    torch.cuda.synchronize()
    assert not rep.value and not hc.any() and int(c.sum()) == 0
    assert L.rt_scene_kind(h) == _lib.RT_SCENE_INSTANCED and L.rt_scene_device(h) == 0
    assert L.rt_scene_device_bytes(h) == 3 * 64 + 3 * 112 + 3 * 48 + 2 * 4 * 32
    assert L.rt_scene_device_bytes(_scene("m3", False)._handle()) == 3 * 64 + 3 * 112
    _same(before, _trace(gs, o_t, d_t, N), "after the refused calls")


def _instances(items):
    a = (_lib.Instance * len(items))()
    for k, t in enumerate(items):
        a[k].blas, a[k].flags = t[0], t[2]
        a[k].xform[:] = np.asarray(t[1], np.float32).reshape(12).tolist()
    return a
