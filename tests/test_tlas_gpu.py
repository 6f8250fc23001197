"""Instanced scenes with a top-level tree on the GPU (RT_INSTANCED_TLAS,
include/rtamd.h; trace_tlas_kernel, csrc/rt_tlas.hip).

Bar, as tests/test_instances_gpu.py: sentinel-filled buffers with guards, and
every value bitwise the reference's. The reference is tlas_common.compose_tlas:
the oracle's mesh intersection per instance in index order for the rays that
pass the instance's world box, on the M and the boxes read back from the
device; the boxes themselves are checked against the definition separately.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cpuref
import instances_common as IC
import ray_cases as RC
import rtamd
import tlas_common as TC
from rtamd import _lib, torch_rays
from test_instances_gpu import ALL, DEFS, N, PAIRS, PLANE_OFF, _assert_ref, _bits, _blas, _pose, _same, _set_plane, _trace

pytestmark = pytest.mark.gpu

RT_E_INVALID, RT_E_STATE = -1, -4
SCENE_DEFS = {"a-tri": DEFS["a-tri"], "b": DEFS["b"], "c": DEFS["c"], "d": DEFS["d"], "130": TC.scene130(),
              "exact": (RC.INST_MESHES, RC.instanced_def())}
SCENES = list(SCENE_DEFS)


def _build(name, tlas=True):
    names, inst = SCENE_DEFS[name]
    return rtamd.InstancedScene([_blas(m) for m in names], inst, tlas=tlas)


@functools.lru_cache(maxsize=None)
def _scene(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def _flat(name):
    return _build(name, tlas=False)


def _refs(name):
    return {k: IC.ref_mesh(m) for k, m in enumerate(SCENE_DEFS[name][0])}


def _dev(o, d):
    return torch.from_numpy(np.ascontiguousarray(o)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()


@functools.lru_cache(maxsize=None)
def _rays(name, kind="random"):
    """random: instances_common.random_rays (the exact scene: its lattice_axis
    class, rays with exact zeros: the rule for a non-finite 1/d); eye: 64 x 64
    pinhole rays, coherent waves."""
    if kind == "eye":
        o, d = TC.eye_rays()
    elif name == "exact":
        o, d = RC.instanced_sets()["lattice_axis"]
    else:
        o, d = IC.random_rays(N, 20261014)
    o, d = np.array(o, np.float32), np.array(d, np.float32)  # writable copies
    return (o, d) + _dev(o, d)


def _compose(name, gs, o, d, tn, tf):
    tab = gs.instances()
    leaf, _ = gs.tlas()
    return TC.compose_tlas(_refs(name), tab.blas, tab.flags, tab.inv, leaf, o, d, tn, tf, tab.skipped)


@functools.lru_cache(maxsize=None)
def _ref(name, kind, tn, tf):
    """The composed reference of scene `name` without its plane, once:
    (hit, t, normal, prim, BLAS traversals per ray)."""
    o, d, _, _ = _rays(name, kind)
    out = _compose(name, _scene(name), o, d, tn, tf)
    for a in out:
        a.setflags(write=False)
    return out


def _ref_plane(name, kind, plane, tn, tf, n=N):
    o, d, _, _ = _rays(name, kind)
    res = tuple(a[:n] for a in _ref(name, kind, tn, tf)[:4])
    return IC.with_plane(res, o[:n], d[:n], tn, tf, PLANE_OFF) if plane else res


def _umin(v):
    _lib.check(rtamd.lib().rtx_set_tlas_uniform_min(int(v)))


@pytest.fixture
def default_umin():
    yield
    _umin(0)  # any value outside 1 .. 65 restores the shipped default


def _check_all(name, kind, plane, tn, tf, what, n=N):
    gs = _scene(name)
    _set_plane(gs, plane)
    ref = _ref_plane(name, kind, plane, tn, tf, n)
    _, _, o_t, d_t = _rays(name, kind)
    _assert_ref(ref, _trace(gs, o_t, d_t, n, tn=tn, tf=tf), what)
    a = _trace(gs, o_t, d_t, n, outputs=("hit",), tn=tn, tf=tf, any_hit=True)
    assert np.array_equal(ref[0], a["hit"]), f"{what}: any-hit mask differs from the closest-hit flag"
    return ref


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("plane", [False, True])
@pytest.mark.parametrize("tn,tf", PAIRS)
def test_parity_with_composed_oracle(gpu, name, plane, tn, tf):
    """Closest hit with all four outputs, and any hit (the closest-hit flag),
    on 4,096 rays under the shipped threshold."""
    ref = _check_all(name, "random", plane, tn, tf, f"{name} plane={plane} [{tn}, {tf}]")
    if not plane and tn == 0.01:
        inst, _ = torch_rays.split_prim(ref[3])
        assert int((inst >= 0).sum()) > 100, "the scene is hardly hit"
        if name in ("d", "130"):
            assert len(np.unique(inst[inst >= 0])) > 64
        if name == "130":  # both meshes win: neighbouring candidates differ in their MeshDev
            assert (inst[inst >= 0] % 2 == 0).sum() > 50 and (inst[inst >= 0] % 2 == 1).sum() > 50
        if name == "exact":
            a, b = RC.TWINS
            assert (inst == a).any() and not (inst == b).any()


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("umin", [1, 65])
def test_both_processing_paths(gpu, default_umin, name, umin):
    """The same batches with every round on the shared path (1) and on the
    per-lane path (65): each equals the reference, with and without the normal,
    with the plane, and on coherent eye rays."""
    _umin(umin)
    gs = _scene(name)
    for kind, plane, (tn, tf) in (("random", False, PAIRS[0]), ("random", True, PAIRS[1]), ("eye", False, PAIRS[0])):
        ref = _check_all(name, kind, plane, tn, tf, f"{name} umin={umin} {kind} plane={plane}")
        _, _, o_t, d_t = _rays(name, kind)
        _assert_ref(ref, _trace(gs, o_t, d_t, N, outputs=("t", "prim"), tn=tn, tf=tf), f"{name} umin={umin} no normal")


@pytest.mark.parametrize("name", ["d", "130"])
def test_eye_rays_and_traversal_counts(gpu, name):
    """64 x 64 pinhole eye rays under the shipped threshold; the kernel's count
    of BLAS traversals per ray is the reference's, ray by ray, and far below K."""
    ref = _check_all(name, "eye", False, 0.01, 100.0, f"{name} eye rays")
    assert int(ref[0].sum()) > 200
    gs = _scene(name)
    _, _, o_t, d_t = _rays(name, "eye")
    cnt = torch.full((N + 64,), -1, dtype=torch.int32, device="cuda")
    try:
        _lib.check(rtamd.lib().rtx_set_tlas_count(C.c_void_p(cnt.data_ptr())))
        _trace(gs, o_t, d_t, N)
    finally:
        _lib.check(rtamd.lib().rtx_set_tlas_count(None))
    got = cnt.cpu().numpy()
    want = _ref(name, "eye", 0.01, 100.0)[4]
    assert (got[N:] == -1).all() and np.array_equal(got[:N], want)
    print(f"{name}: BLAS traversals per eye ray {len(gs)} -> {want.mean():.2f}")
    assert want.mean() < 0.2 * len(gs)


@pytest.mark.parametrize("name", ["b", "d"])
@pytest.mark.parametrize("n", [1, 65, 4096])
def test_ray_counts(gpu, name, n):
    """[0, n) fully written, misses included, the 64 elements behind it not."""
    gs = _scene(name)
    _set_plane(gs, False)
    ref = _ref_plane(name, "random", False, 0.01, 100.0, n)
    _, _, o_t, d_t = _rays(name)
    _assert_ref(ref, _trace(gs, o_t, d_t, n), f"{name} n={n}")
    a = _trace(gs, o_t, d_t, n, outputs=("hit",), any_hit=True)
    assert np.array_equal(ref[0], a["hit"])


@pytest.mark.parametrize("name", ["c", "130"])
@pytest.mark.parametrize("umin", [0, 1, 65])
def test_per_ray_intervals(gpu, default_umin, name, umin):
    """d_tnear / d_tfar tensors: each ray draws one of the three intervals;
    also one of the two pointers NULL; with and without the plane."""
    _umin(umin)
    gs = _scene(name)
    o, d, o_t, d_t = _rays(name)
    pick = np.random.default_rng(5).integers(0, 3, N)
    tn = np.float32([p[0] for p in PAIRS])[pick]
    tf = np.float32([p[1] for p in PAIRS])[pick]
    tn_t, tf_t = torch.from_numpy(tn).cuda(), torch.from_numpy(tf).cuda()
    for plane, use_tn, use_tf in ((False, True, True), (True, True, False), (False, False, True)):
        _set_plane(gs, plane)
        a = tn if use_tn else np.full(N, 0.25, np.float32)
        b = tf if use_tf else np.full(N, 3.0, np.float32)
        ref = _per_ray_ref(name, use_tn, use_tf)
        if plane:
            ref = IC.with_plane(ref, o, d, a, b, PLANE_OFF)
        kw = dict(tn=0.25, tf=3.0, tn_t=tn_t if use_tn else None, tf_t=tf_t if use_tf else None)
        _assert_ref(ref, _trace(gs, o_t, d_t, N, **kw), f"{name} per-ray tn={use_tn} tf={use_tf}")
        got = _trace(gs, o_t, d_t, N, outputs=("hit",), any_hit=True, **kw)
        assert np.array_equal(ref[0], got["hit"]), "any-hit mask differs"


@functools.lru_cache(maxsize=None)
def _per_ray_ref(name, use_tn, use_tf):
    o, d, _, _ = _rays(name)
    pick = np.random.default_rng(5).integers(0, 3, N)
    a = np.float32([p[0] for p in PAIRS])[pick] if use_tn else np.full(N, 0.25, np.float32)
    b = np.float32([p[1] for p in PAIRS])[pick] if use_tf else np.full(N, 3.0, np.float32)
    return _compose(name, _scene(name), o, d, a, b)[:4]


def test_host_entry(gpu):
    """One rt_intersect_rays call on host buffers: the same reference."""
    gs = _scene("c")
    _set_plane(gs, True)
    ref = _ref_plane("c", "random", True, 0.01, 100.0)
    o, d, _, _ = _rays("c")
    h = gs.intersect(o, d, 0.01, 100.0)
    _assert_ref(ref, {"hit": h.hitten.astype(np.int32), "t": h.t, "normal": h.normal, "prim": h.prim}, "host entry")


# ------------------------------------------------------------------ boxes --
def _root_box(bl):
    rb = np.zeros(6, np.float32)
    _lib.check(rtamd.lib().rtx_scene_mesh_constants(bl._handle(), C.c_void_p(rb.ctypes.data), None, None))
    return rb


def _want_leaves(names, inst, blas_objs=None, skipped=None):
    """The definition's leaf boxes from host data: rt_instance_world_box of the
    given matrix and the BLAS's root_box (a one-triangle BLAS: unbounded)."""
    objs = blas_objs or [_blas(m) for m in names]
    boxes = [None if m == "tri" else _root_box(b) for m, b in zip(names, objs)]
    out = np.tile(TC.EMPTY, (len(inst), 1))
    for i, t in enumerate(inst):
        fl = t[2] if len(t) > 2 else 0
        if fl & IC.DISABLED or (skipped is not None and skipped[i]):
            continue
        rb = boxes[t[0]]
        out[i] = TC.UNBOUNDED if rb is None else rtamd.instance_world_box(t[1], rb)
    return out


def _assert_boxes(gs, want_leaves, what):
    leaf, node = gs.tlas()
    K, P = len(want_leaves), TC.leaf_count(len(want_leaves))
    assert leaf.shape == (K, 6) and node.shape == (2 * P, 6), what
    assert np.array_equal(_bits(leaf), _bits(want_leaves)), f"{what}: leaf boxes differ from the definition"
    assert np.array_equal(_bits(node), _bits(TC.tree(leaf))), f"{what}: node boxes differ from the numpy union"
    assert np.array_equal(_bits(node[P + K:]), _bits(np.tile(TC.EMPTY, (P - K, 1)))), f"{what}: a padded leaf is not empty"


@pytest.mark.parametrize("name", SCENES)
def test_boxes(gpu, name):
    """Device leaf boxes are rt_instance_world_box(xform, root_box) bitwise, and
    the numpy restatement's; node boxes the numpy union; padded and disabled
    leaves empty; the leaf-root BLAS unbounded. device_bytes counts the tree
    and the matrices."""
    names, inst = SCENE_DEFS[name]
    gs = _scene(name)
    want = _want_leaves(names, inst)
    _assert_boxes(gs, want, name)
    for i, t in enumerate(inst):
        if names[t[0]] != "tri" and not (len(t) > 2 and t[2] & IC.DISABLED):
            assert np.array_equal(_bits(want[i]), _bits(TC.world_box(t[1], _root_box(_blas(names[t[0]]))))), i
    K, P = len(inst), TC.leaf_count(len(inst))
    assert {"a-tri": 1, "d": 128, "130": 256}.get(name, P) == P
    assert gs.device_bytes() == K * 64 + len(names) * 56 + K * 48 + 2 * P * 32
    if name == "a-tri":
        assert np.array_equal(gs.tlas()[0][0], TC.UNBOUNDED)
    if name == "c":
        assert np.array_equal(gs.tlas()[0][4], TC.EMPTY) and np.array_equal(gs.tlas()[0][0], TC.UNBOUNDED)


# ---------------------------------------------------------------- updates --
def test_poses_from_the_device(gpu):
    """update_instances_device of all poses, then of the sub-range first = 3,
    count = 5, on a non-default stream: boxes and traced outputs equal those of
    a TLAS scene created fresh with those poses, bit for bit; a singular matrix
    gives a skipped instance and an empty leaf, its next good matrix restores it."""
    names, inst = SCENE_DEFS["d"]
    K = len(inst)
    gs = _build("d")
    _, _, o_t, d_t = _rays("d")
    fresh = lambda poses, flags=None: rtamd.InstancedScene(
        [_blas(m) for m in names], [(inst[k][0], poses[k], 0 if flags is None else flags[k]) for k in range(K)], tlas=True)
    rng = np.random.default_rng(77)
    p1 = np.stack([_pose(400 + k, rng.uniform(0.15, 0.3, 3), rng.uniform(-1.5, 1.5, 3)) for k in range(K)])
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        x = torch.from_numpy(p1).cuda() * 1.0  # produced by a torch kernel on this stream
        torch_rays.update_instances(gs, x)
        r = torch_rays.trace(gs, o_t, d_t)
    st.synchronize()
    f1 = fresh(p1)
    _assert_boxes(gs, f1.tlas()[0], "all poses from the device")
    _assert_boxes(gs, _want_leaves(names, [(inst[k][0], p1[k], 0) for k in range(K)]), "all poses: the definition")
    _same({k: getattr(r, k).cpu().numpy() for k in ALL}, _trace(f1, o_t, d_t, N), "all poses from the device")
    # the sub-range first = 3, count = 5
    p2 = p1.copy()
    p2[3:8] = np.stack([_pose(500 + k, (0.3, 0.2, 0.25), (0.2 * k - 0.4, 0.1, -0.3)) for k in range(5)])
    with torch.cuda.stream(st):
        torch_rays.update_instances(gs, (torch.from_numpy(p2[3:8]).cuda() * 1.0).reshape(5, 12), first=3)
    st.synchronize()
    f2 = fresh(p2)
    _assert_boxes(gs, f2.tlas()[0], "a sub-range from the device")
    _same(_trace(gs, o_t, d_t, N), _trace(f2, o_t, d_t, N), "a sub-range from the device")
    # a singular matrix: skipped, its leaf empty, until its next update
    bad = p2[4:5].copy()
    bad[0, 2, :3] = bad[0, 1, :3]
    torch_rays.update_instances(gs, torch.from_numpy(bad).cuda(), first=4)
    assert gs.instances().skipped.tolist() == [int(k == 4) for k in range(K)]
    fl = [IC.DISABLED if k == 4 else 0 for k in range(K)]
    without = fresh(p2, fl)
    assert np.array_equal(gs.tlas()[0][4], TC.EMPTY)
    _assert_boxes(gs, without.tlas()[0], "a skipped instance")
    _same(_trace(gs, o_t, d_t, N), _trace(without, o_t, d_t, N), "a skipped instance")
    torch_rays.update_instances(gs, torch.from_numpy(p2[4:5]).cuda(), first=4)
    assert not gs.instances().skipped.any()
    _assert_boxes(gs, f2.tlas()[0], "the instance is back")
    _same(_trace(gs, o_t, d_t, N), _trace(f2, o_t, d_t, N), "the instance is back")
    for s in (gs, f1, f2, without):
        s.close()


def test_host_pose_update_toggles_disabled(gpu):
    """update_instances from host matrices with new flags: as a fresh scene;
    DISABLED empties the leaf, clearing it brings the box back."""
    names, inst = SCENE_DEFS["b"]
    gs = _build("b")
    _, _, o_t, d_t = _rays("b")
    p = np.stack([_pose(60 + k, (0.9, 0.8, 0.7), (0.1, 0.1 * k, -0.1)) for k in range(2)])
    for flags in ([IC.DISABLED, 0], [0, 0], [0, IC.DISABLED]):
        gs.update_instances(p, first=1, flags=flags)
        now = [inst[0], (1, p[0], flags[0]), (0, p[1], flags[1])]
        want = rtamd.InstancedScene([_blas(m) for m in names], now, tlas=True)
        _assert_boxes(gs, _want_leaves(names, now), f"host update {flags}")
        _same(_trace(gs, o_t, d_t, N), _trace(want, o_t, d_t, N), f"host update {flags}")
        assert gs.instances().flags.tolist() == [0] + flags
        want.close()
    gs.close()


def test_dynamic_blas(gpu):
    """After update_vertices of a dynamic BLAS the next trace sees the new
    boxes. An exact translation of the lattice mesh (the refitted tree is then
    the tree of a fresh build, tests/test_refit_gpu.py): the trace equals the
    reference on the new mesh. A general deformation (the refit keeps the
    topology, which the oracle's own build would not): boxes and outputs equal
    those of a TLAS scene created afterwards."""
    import refit_common as R
    v, i = IC.mesh("grid")
    bl = rtamd.BVHBuilder(rtamd.SimpleMesh(v, i), dynamic=True)

    def placed(seed, scale, b):  # the pose that puts the TRANSLATED mesh where _pose(seed, scale, b) puts the original
        x = _pose(seed, scale, b).astype(np.float64)
        x[:, 3] -= x[:, :3] @ R.SHIFT.astype(np.float64)
        return x.astype(np.float32)

    inst = [(0, placed(70, (0.3, 0.25, 0.3), (-0.8, -0.7, -0.9)), 0), (1, _pose(71, (0.9, 0.9, 0.9), (0.3, 0.2, 0.0)), 0),
            (0, placed(72, (0.1, 0.1, 0.1), (0.9, 0.9, 0.5)), 0)]
    names, objs = ("grid", "cube"), [bl, _blas("cube")]
    gs = rtamd.InstancedScene(objs, inst, tlas=True)
    o, d, o_t, d_t = _rays("b")
    _assert_boxes(gs, _want_leaves(names, inst, objs), "before the refit")
    before = _trace(gs, o_t, d_t, N)
    leaf_before = gs.tlas()[0]
    w = R.translate(v)
    torch_rays.update_vertices(bl, torch.from_numpy(w).cuda())
    after = _trace(gs, o_t, d_t, N)
    want = _want_leaves(names, inst, objs)
    assert not np.array_equal(want[0], leaf_before[0]) and np.array_equal(want[1], leaf_before[1])  # only the lattice moved
    _assert_boxes(gs, want, "after the translation")
    tab = gs.instances()
    refs = {0: cpuref.RefScene.mesh(w, i), 1: IC.ref_mesh("cube")}
    ref = TC.compose_tlas(refs, tab.blas, tab.flags, tab.inv, gs.tlas()[0], o, d, 0.01, 100.0)
    _assert_ref(ref[:4], after, "after the translation")
    inst_hit, _ = torch_rays.split_prim(ref[3])
    assert (inst_hit == 0).sum() > 50 and (inst_hit == 1).sum() > 50
    assert not np.array_equal(_bits(before["t"]), _bits(after["t"]))
    a = _trace(gs, o_t, d_t, N, outputs=("hit",), any_hit=True)
    assert np.array_equal(a["hit"], ref[0])
    # a general deformation: as a scene created afterwards
    w2 = np.array(w)
    w2[:, :3] += np.random.default_rng(72).normal(scale=0.3, size=(len(w2), 3)).astype(np.float32)
    torch_rays.update_vertices(bl, torch.from_numpy(w2).cuda())
    deformed = _trace(gs, o_t, d_t, N)
    again = rtamd.InstancedScene(objs, inst, tlas=True)
    _assert_boxes(gs, again.tlas()[0], "after the deformation")
    _assert_boxes(gs, _want_leaves(names, inst, objs), "after the deformation: the definition")
    _same(deformed, _trace(again, o_t, d_t, N), "after the deformation")
    assert not np.array_equal(_bits(deformed["t"]), _bits(after["t"]))
    for sc in (gs, again, bl):
        sc.close()


# ------------------------------------------------- against the flat list --
@pytest.mark.parametrize("name", SCENES)
def test_agrees_with_the_flat_list(gpu, name):
    """On the same poses and rays the TLAS scene and the flat scene differ on 0
    rays, in every output, random and eye rays."""
    gs, fl = _scene(name), _flat(name)
    _set_plane(gs, False)
    _set_plane(fl, False)
    for kind in ("random", "eye"):
        _, _, o_t, d_t = _rays(name, kind)
        for tn, tf in PAIRS:
            a, b = _trace(gs, o_t, d_t, N, tn=tn, tf=tf), _trace(fl, o_t, d_t, N, tn=tn, tf=tf)
            differ = np.zeros(N, bool)
            for k in ALL:
                differ |= (_bits(a[k]) != _bits(b[k])).reshape(N, -1).any(axis=1)
            assert int(differ.sum()) == 0, f"{name} {kind} [{tn}, {tf}]: {int(differ.sum())} rays differ from the flat list"


def _instance_array(items):
    a = (_lib.Instance * len(items))()
    for k, t in enumerate(items):
        a[k].blas, a[k].flags = t[0], t[2] if len(t) > 2 else 0
        a[k].xform[:] = np.asarray(t[1], np.float32).reshape(12).tolist()
    return a


def test_flat_scenes_are_unchanged_and_argument_rules(gpu):
    """rt_scene_create_instanced_ex(..., 0, ...) equals rt_scene_create_instanced
    output for output and holds no tree; an unknown flag bit is RT_E_INVALID;
    the render entries still return RT_E_STATE for a TLAS scene."""
    L = gpu.lib()
    names, inst = SCENE_DEFS["c"]
    hs = (C.c_void_p * len(names))(*[_blas(m)._handle() for m in names])
    arr = _instance_array(inst)
    h_old, h_ex, h_bad = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.rt_scene_create_instanced(hs, len(names), arr, len(inst), C.byref(h_old)) == 0
    assert L.rt_scene_create_instanced_ex(hs, len(names), arr, len(inst), 0, C.byref(h_ex)) == 0
    for bad in (2, 3, 0x80000000):
        assert L.rt_scene_create_instanced_ex(hs, len(names), arr, len(inst), bad, C.byref(h_bad)) == RT_E_INVALID
        assert not h_bad.value and L.rt_last_error()
    _, _, o_t, d_t = _rays("c")
    outs = []
    for h in (h_old, h_ex):
        assert L.rt_scene_device_bytes(h) == len(inst) * 64 + len(names) * 56
        assert L.rt_scene_get_tlas(h, None, None, None) == RT_E_STATE
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
    _same(outs[0], outs[1], "flags = 0")
    assert int(outs[0]["hit"].sum()) > 100
    assert L.rt_scene_get_tlas(None, None, None, None) == RT_E_INVALID
    assert L.rt_scene_get_tlas(_blas("cube")._handle(), None, None, None) == RT_E_STATE
    # the entries that do not take the kind, on a TLAS scene
    gs = _scene("b")
    h = gs._handle()
    P = rtamd.render_params((0, 0, 2.5), *cpuref.camera_matrices((0, 0, 2.5), aspect=1.0))
    c = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    t = torch.zeros((8, 8), dtype=torch.float32, device="cuda")
    hc, ht = np.zeros((8, 8), np.uint32), np.zeros((8, 8), np.float32)
    cp, tp = (C.c_void_p * 1)(c.data_ptr()), (C.c_void_p * 1)(t.data_ptr())
    mean, total, out = C.c_float(), C.c_float(), C.c_void_p()
    pv = lambda a: C.c_void_p(a.ctypes.data)
    state = {
        "rt_render": L.rt_render(h, C.byref(P), pv(hc), pv(ht), 8, 8, 1, None),
        "rt_render_device": L.rt_render_device(h, C.byref(P), c.data_ptr(), t.data_ptr(), 8, 8, 1, None, None),
        "rt_render_device_frames": L.rt_render_device_frames(h, C.byref(P), 1, cp, tp, 8, 8, 1, None, None),
        "rt_bench_frames": L.rt_bench_frames(h, C.byref(P), 1, 8, 8, 1, C.byref(mean), C.byref(total)),
        "rt_scene_replicate": L.rt_scene_replicate(h, 0, C.byref(out)),
    }
    assert state == {k: RT_E_STATE for k in state}
    torch.cuda.synchronize()
    assert not out.value and not hc.any() and int(c.sum()) == 0
    assert L.rt_scene_kind(h) == _lib.RT_SCENE_INSTANCED
    leaves = C.c_int32(0)
    assert L.rt_scene_get_tlas(h, None, None, C.byref(leaves)) == 0 and leaves.value == 4
